"""GPU tests on the reference's held-out corpora (tests/golden/heldout.npz and graph2.npz, made by make_golden_heldout.py and
make_golden_graph.py 2; reach4.npz is followed in test_gpu_reach.py):
  * the human replays of "006 both flavours of ramp jumping" (ramp jumps and slope landings: crease and depenetration code, the
    DPP group reductions of npp_kernels.hip) plus corpus replays, under every launch geometry and build variant, each against
    the reference's fixture AND the oracle's multiply-square twin, every tick, bit for bit;
  * random-action rollouts on all 16 of `nclone/test_maps/` through npp_step with in-kernel auto-reset (Simulator.reset first,
    Simulator.fast_reset after, truncation at 240 frames), one env per map and replicated into mixed-level workgroups;
  * the graph observation rows of the 16 test maps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GS_TOL = 2e-6   # as test_gpu_parity.py
TRUNC = 240     # make_golden_heldout.py: TRUNC
# test_gpu_parity.test_launch_geometries_bit_identical's list: (lanes per env, waves per block, G = 16 build variant)
GEOMETRIES = [(1, 1, 0), (1, 4, 0), (2, 2, 0), (4, 4, 0), (8, 1, 0), (8, 4, 0), (16, 4, 0), (16, 4, 1), (16, 4, 2), (16, 2, 1),
              (32, 2, 0), (64, 4, 0)]


def _disc(i):
    return i[:, :20].clip(0, 255).astype(np.uint8)


def _replay_set(golden):
    """The 6 held-out ramp-jumping replays and 5 corpus replays: (maps, inputs, fixture t, fixture d, final rows)."""
    h, c, t = golden.z("heldout"), golden.z("corpus"), golden.z("traj")
    names = golden.names("heldout")
    new = [i for i, nm in enumerate(names) if "ramp jumping" in nm]
    assert len(new) == 6
    out = [(h["m%d" % i], h["in%d" % i], h["t%d" % i], h["d%d" % i], h["final"][i]) for i in new]
    for i in golden.in_scope_replays()[::21]:
        out.append((c["m%d" % i], c["in%d" % i], t["t%d" % i], t["d%d" % i], c["final"][i]))
    return out


def test_heldout_replays_every_geometry_vs_reference_and_oracle(golden, oracle_mod):
    """Every (G, waves per block, variant) of the geometry list, 2 envs per replay: every tick's fp64 state equals the reference's
    fixture and the `mul` oracle's bits (normals and old velocities included), the discrete fields and the end state match."""
    from nclone_amd.engine import NppBatch

    rs = _replay_set(golden)
    nr = len(rs)
    n = 2 * nr
    T = [len(r[2]) for r in rs]
    tmax = max(T)
    inputs = np.zeros((tmax, n), dtype=np.uint8)
    for e in range(n):
        inputs[: T[e % nr], e] = rs[e % nr][1][: T[e % nr]]
    d_in = torch.from_numpy(inputs).cuda()
    # the oracle's trajectories once: fp64 row and 22 discrete fields per tick
    orf, ord_ = [], []
    for k, (m, inp, _t, _d, _f) in enumerate(rs):
        o = oracle_mod.Oracle("mul")
        assert o.load(np.asarray(m, dtype=np.float64)) == 0
        fr, dr = [], []
        for tick in range(T[k]):
            hh, j = oracle_mod.controls(int(inp[tick]))
            o.tick(hh, j)
            f, d = o.core()
            fr.append(np.array(f))
            dr.append(np.array(d[:22]))
        orf.append(np.stack(fr))
        ord_.append(np.stack(dr))
    ticks = 0
    for g, wpb, var in GEOMETRIES:
        b = NppBatch(n, autoreset=False)
        b.load_levels([r[0] for r in rs])
        b.set_launch_geometry(g, wpb)
        b.set_step_variant(var)
        assert b.launch_geometry()[0] == g
        assert b.step_variant() == (var if g == 16 else 0, True)
        b.assign_levels(np.arange(n) % nr)
        for tick in range(tmax):
            b.tick(d_in[tick : tick + 1])
            f, di = b.dump_state()
            disc = _disc(di)
            for e in range(n):
                k = e % nr
                if tick >= T[k]:
                    continue
                ref = rs[k][2][tick]
                assert np.array_equal(f[e, :4], ref), (g, wpb, var, k, tick, f[e, :4], ref)
                assert np.array_equal(disc[e], rs[k][3][tick]), (g, wpb, var, k, tick)
                assert np.array_equal(f[e], orf[k][tick]), (g, wpb, var, k, tick)
                assert np.array_equal(di[e, :22], ord_[k][tick]), (g, wpb, var, k, tick)
                if tick == T[k] - 1:
                    fin = rs[k][4]
                    assert int(fin[0]) == T[k] and di[e, 0] == int(fin[1]) and np.array_equal(f[e, :2], fin[2:4])
                ticks += 1
        b.close()
    assert ticks == len(GEOMETRIES) * 2 * sum(T)


def _test_map_expectations(golden):
    """Per map and step: executed ticks, end kind, frame, the fp64 row / discrete row at the step's last tick, game_state, mask
    bits and entity checksum, as arrays [16, steps, ...]."""
    h = golden.z("heldout")
    names = golden.names("heldout", "rnames")
    assert len(names) == 16
    maps = [h["rm%d" % r] for r in range(16)]
    acts = np.stack([h["ra%d" % r] for r in range(16)])
    S = np.stack([h["rs%d" % r] for r in range(16)])
    last = np.cumsum(S[:, :, 0], axis=1) - 1
    Tend = np.stack([h["rt%d" % r][last[r]] for r in range(16)])
    Dend = np.stack([h["rd%d" % r][last[r]] for r in range(16)])
    G = np.stack([h["rg%d" % r] for r in range(16)])
    K = np.stack([h["rk%d" % r] for r in range(16)])
    E = np.stack([h["re%d" % r] for r in range(16)])
    return names, maps, acts, S, Tend, Dend, G, K, E


def _run_test_maps(golden, level_of_env):
    """Step the envs (env e plays map level_of_env[e] with that map's recorded actions) with in-kernel auto-reset and compare
    every env at every step with the fixture; returns the per-step fp64 states for the replica check."""
    from nclone_amd.engine import NppBatch

    names, maps, acts, S, Tend, Dend, G, K, E = _test_map_expectations(golden)
    lv = np.asarray(level_of_env)
    n = len(lv)
    b = NppBatch(n, autoreset=True, fast_reset=True)   # first reset of an env: Simulator.reset, later ones fast_reset
    b.load_levels(maps)
    b.assign_levels(lv)
    b.set_truncation_limit(TRUNC)
    d_acts = torch.from_numpy(np.ascontiguousarray(acts[lv].T)).cuda()   # [steps, n]
    states = []
    kinds_seen = set()
    worst = 0.0
    for s in range(acts.shape[1]):
        b.step(d_acts[s], frame_skip=4)
        b.sync()
        flags = b.flags.cpu().numpy().astype(np.int64)
        frames = b.frames.cpu().numpy().astype(np.int64)
        gs = b.game_state.cpu().numpy()
        tgs = b.terminal_state.cpu().numpy()
        mask = b.action_mask.cpu().numpy()
        cs = b.entity_checksum()
        f, di = b.dump_state()
        states.append((f, di[:, :27].copy()))
        ex, kind, frame = S[lv, s, 0], S[lv, s, 1], S[lv, s, 2]
        got_kind = np.where(flags & 1, 1, np.where(flags & 2, 2, np.where(flags & 8, 3, 0)))
        assert np.array_equal(frames, ex), (s, [names[lv[e]] for e in np.flatnonzero(frames != ex)][:4])
        assert np.array_equal(got_kind, kind), (s, [names[lv[e]] for e in np.flatnonzero(got_kind != kind)][:4])
        kinds_seen |= set(kind.tolist())
        obs = np.where((kind != 0)[:, None], tgs, gs)
        d = np.abs(obs[:, :40] - G[lv, s]).max(axis=1)
        worst = max(worst, float(d.max()))
        assert (d <= GS_TOL).all(), (s, [names[lv[e]] for e in np.flatnonzero(d > GS_TOL)][:4])
        tr = np.maximum(0.0, (TRUNC - frame) / TRUNC).astype(np.float32)
        assert (np.abs(obs[:, 40] - tr) <= 1e-7).all(), s
        live = kind == 0
        bits = (mask.astype(np.int64) << np.arange(6)).sum(axis=1)
        assert np.array_equal(bits[live], K[lv, s][live].astype(np.int64)), s
        assert np.array_equal(f[live, :4], Tend[lv, s][live]), (s, [names[lv[e]] for e in np.flatnonzero(live)[
            (f[live, :4] != Tend[lv, s][live]).any(axis=1)]][:4])
        assert np.array_equal(_disc(di)[live], Dend[lv, s][live]), s
        # entity checksum: sums of positions / speeds within 1e-9, the state codes exact (test_gpu_round2.py's bars)
        assert np.allclose(cs[live], E[lv, s][live], rtol=0, atol=1e-9), (s, np.abs(cs[live] - E[lv, s][live]).max())
        assert np.array_equal(cs[live, 4:], E[lv, s][live, 4:]), s
        assert (di[~live, 22] == 0).all() and (di[~live, 0] == 0).all(), s   # auto-reset: spawn state again
    assert kinds_seen == {0, 1, 2, 3}
    print("test-map rollouts: %d envs x %d steps, worst game_state diff %.3g" % (n, acts.shape[1], worst))
    b.close()
    return states


def test_test_map_rollouts_one_env_per_map(golden):
    _run_test_maps(golden, np.arange(16))


def test_test_map_rollouts_mixed_workgroups_ragged(golden):
    """16 * 64 + 37 envs, env e on map e % 16: every workgroup holds all 16 maps (the global-memory path), the last one is
    partial.  Each env matches the fixture, and the replicas of a map hold identical bits at every step."""
    n = 16 * 64 + 37
    lv = np.arange(n) % 16
    states = _run_test_maps(golden, lv)
    for s, (f, di) in enumerate(states):
        for r in range(16):
            assert np.array_equal(f[lv == r], np.tile(f[r], ((lv == r).sum(), 1))), (s, r)
            assert np.array_equal(di[lv == r], np.tile(di[r], ((lv == r).sum(), 1))), (s, r)


def test_graph_rows_of_the_test_maps():
    """The device's graph observation for every test map, after reset, against graph2.npz (the reference's build_graph +
    create_graph_data), byte for byte, padding included; 4 envs per map."""
    import os

    from nclone_amd.engine import NppBatch

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graph2.npz"))
    names = bytes(z["names"]).decode().split("\n")
    assert len(names) == 16
    maps = [z["m%d" % k] for k in range(16)]
    n = 64
    lv = np.arange(n) % 16
    b = NppBatch(n)
    b.load_levels(maps)
    b.assign_levels(lv)
    b.reset()
    out = b.graph_observation()
    feats = out["graph_node_feats"].cpu().numpy()
    assert out["graph_edge_index"].dtype == torch.uint16
    edges = out["graph_edge_index"].contiguous().view(torch.uint8).cpu().numpy().view(np.uint16).reshape(n, 2, 20000)
    nmask = out["graph_node_mask"].cpu().numpy()
    emask = out["graph_edge_mask"].cpu().numpy()
    for e in range(n):
        k = int(lv[e])
        nn, ne = int(z["nn%d" % k]), int(z["ne%d" % k])
        assert feats[e].shape == (2500, 6) and edges[e].shape == (2, 20000), names[k]
        assert feats[e, :nn].tobytes() == z["f%d" % k].tobytes() and not feats[e, nn:].any(), names[k]
        assert np.array_equal(edges[e, :, :ne], z["e%d" % k]) and not edges[e, :, ne:].any(), names[k]
        assert np.array_equal(nmask[e], (np.arange(2500) < nn).astype(nmask.dtype)), names[k]
        assert np.array_equal(emask[e], (np.arange(20000) < ne).astype(emask.dtype)), names[k]
    b.close()
