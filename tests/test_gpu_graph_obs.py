"""GPU tests of the graph observations (npp_graph_observation, npp_graph.hip).  The expected rows of an env are
npp_graph_compile's output for the level it plays (pinned against the reference by tests/test_graph_host.py), padded to the
reference's shapes; every row of every env is compared byte for byte."""
import numpy as np
import pytest
import torch

from nclone_amd import _native as nat

pytestmark = pytest.mark.gpu

KEYS = ("graph_node_feats", "graph_edge_index", "graph_node_mask", "graph_edge_mask")


class Expected:
    """Per-level rows on the device, as bytes (uint16 has few torch kernels): check(obs, levels) compares every env's rows."""

    DTYPES = {"graph_node_feats": (np.float32, torch.float32), "graph_edge_index": (np.uint16, torch.uint16),
              "graph_node_mask": (np.uint8, torch.uint8), "graph_edge_mask": (np.uint8, torch.uint8)}

    def __init__(self, levels):
        from nclone_amd.engine import graph_tables

        rows = {k: [] for k in KEYS}
        for m in levels:
            feats, edges, nn, ne = graph_tables(m)
            rows["graph_node_feats"].append(feats)
            rows["graph_edge_index"].append(edges)
            rows["graph_node_mask"].append((np.arange(2500) < nn).astype(np.uint8))
            rows["graph_edge_mask"].append((np.arange(20000) < ne).astype(np.uint8))
        self.shape = {k: rows[k][0].shape for k in KEYS}
        self.t = {k: torch.from_numpy(np.stack(v).reshape(len(levels), -1).view(np.uint8)).cuda() for k, v in rows.items()}

    def check(self, obs, levels, what=""):
        lv = torch.from_numpy(np.asarray(_np(levels), dtype=np.int64)).cuda()
        for k in KEYS:
            got = obs[k]
            n = got.shape[0]
            assert tuple(got.shape) == (len(lv),) + self.shape[k], (k, what)
            if isinstance(got, np.ndarray):
                assert got.dtype == self.DTYPES[k][0], (k, what)
                got = torch.from_numpy(np.ascontiguousarray(got).reshape(n, -1).view(np.uint8)).cuda()
            else:
                assert got.dtype == self.DTYPES[k][1] and got.is_contiguous(), (k, what)
                got = got.view(torch.uint8).view(n, -1)
            bad = (got != self.t[k].index_select(0, lv)).any(dim=1)   # bytes: keeps -0.0 and 0.0 apart
            assert not bool(bad.any()), (k, what, torch.nonzero(bad).flatten()[:8].tolist())


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _same(x, y):
    """Byte equality of two observation entries (device tensors are compared on the device)."""
    if isinstance(x, torch.Tensor):
        return x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
    x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))


def _mixed():
    from nclone_amd.levels import c3_mixed_levels

    return c3_mixed_levels()[0]


def test_rows_after_reset_doors_mines_zoo():
    from nclone_amd.engine import NppBatch
    from nclone_amd.levels import door_levels, mine_levels, zoo_levels

    levels = door_levels()[0] + mine_levels()[0] + zoo_levels()[0]
    exp = Expected(levels)
    n = 4 * len(levels)
    b = NppBatch(n)
    b.load_levels(levels)
    ids = np.arange(n) % len(levels)
    b.assign_levels(ids)
    b.reset()
    out = b.graph_observation()
    exp.check(out, ids, "reset")
    assert int(out["graph_node_mask"].sum()) > 0 and int(out["graph_edge_mask"].sum()) > 0
    b.close()


def _pool_run(n, output, overlap):
    from nclone_amd.vec_env import NppVecEnvironment

    levels = _mixed()
    exp = Expected(levels)
    w = np.linspace(1.0, 2.0, len(levels))
    kw = dict(truncation_limit=60, level_weights=w, level_seed=7, autoreset=True)
    env = NppVecEnvironment(levels, n, output=output, enable_graph_observations=True, **kw)
    twin = NppVecEnvironment(levels, n, output=output, **kw)   # graph observations off
    ovl = NppVecEnvironment(levels, n, output=output, enable_graph_observations=True, obs_overlap=50, **kw) if overlap else None
    envs = [e for e in (env, twin, ovl) if e is not None]
    obs = [e.reset(seed=3)[0] for e in envs]
    lv = env.batch.env_levels()
    exp.check(obs[0], lv, "reset")
    if ovl is not None:
        exp.check(obs[2], lv, "reset overlap")
    rng = np.random.default_rng(11)
    prev = None
    changed = 0
    for t in range(300):
        a = rng.integers(0, 6, size=n).astype(np.uint8)
        res = [e.step(a) for e in envs]
        o, r, term, trunc, info = res[0]
        lv_now = _np(info["level_id"])
        exp.check(o, lv_now, "step %d" % t)
        if prev is not None and (n <= 1000 or t % 10 == 0):   # numpy: the previous step's arrays are still what they were
            exp.check(prev[0], prev[1], "previous of step %d" % t)
        if output == "numpy":
            prev = ({k: o[k] for k in KEYS}, lv_now)
        for (o2, r2, term2, trunc2, info2), name in zip(res[1:], ("twin", "overlap")[: len(res) - 1]):
            assert np.array_equal(_np(info2["level_id"]), lv_now), (name, t)
            assert np.array_equal(_np(r2), _np(r)) and np.array_equal(_np(term2), _np(term)) and np.array_equal(_np(trunc2), _np(trunc))
            for k in o:
                if k in KEYS and name == "twin":
                    continue
                assert k in o2, (name, k)
                assert _same(o2[k], o[k]), (name, k, t)
            if name == "twin":
                assert not any(k in o2 for k in KEYS)
        changed += int((lv_now != lv).sum())
        lv = lv_now
    assert changed > n // 2   # the rows followed many level changes
    for e in envs:
        e.close()
    torch.cuda.synchronize()


@pytest.mark.parametrize("n,output,overlap", [(1000, "torch", True), (8192, "torch", True), (1000, "numpy", False),
                                              (8192, "numpy", False)])
def test_level_pool_rows_follow_level(n, output, overlap):
    _pool_run(n, output, overlap)


def test_assign_snapshot_restore_and_checkpoint_resets():
    from nclone_amd.vec_env import NppVecEnvironment

    levels = _mixed()[:64]
    exp = Expected(levels)
    n = 512
    env = NppVecEnvironment(levels, n, truncation_limit=60, level_weights=np.ones(len(levels)), level_seed=5,
                            enable_graph_observations=True)
    b = env.batch
    env.reset(seed=1)
    rng = np.random.default_rng(2)
    for _ in range(5):
        env.step(rng.integers(0, 6, size=n).astype(np.uint8))
    env.snapshot()
    lv_snap = b.env_levels()
    for _ in range(40):   # episodes end every 60 frames at the latest: most envs draw another level
        o = env.step(rng.integers(0, 6, size=n).astype(np.uint8))[0]
    assert (b.env_levels() != lv_snap).sum() > n // 4
    o, _ = env.reset(options={"checkpoint": "snapshot"})   # back across the level change
    assert np.array_equal(b.env_levels(), lv_snap)
    exp.check(o, lv_snap, "restore")
    o, _ = env.reset(options={"checkpoint": [2, 2, 5, 0]})   # replay from the spawn of the current levels
    exp.check(o, b.env_levels(), "replay")
    # npp_assign_levels mid-run (the batch's own call, behind the env's back)
    new = (np.arange(n) * 7 + 3) % len(levels)
    b.assign_levels(new)
    b.reset()
    o = env.step(np.zeros(n, dtype=np.uint8))[0]
    exp.check(o, b.env_levels(), "assign")
    env.close()
    torch.cuda.synchronize()


def test_rewrite_all_and_fresh_buffers():
    from nclone_amd.engine import GRAPH_KEYS, NppBatch

    levels = _mixed()[:16]
    exp = Expected(levels)
    n = 300
    b = NppBatch(n)
    b.load_levels(levels)
    ids = np.arange(n) % len(levels)
    b.assign_levels(ids)
    b.reset()
    out = b.graph_observation()
    out["graph_node_feats"][5, 0, 0] = 7.0
    out["graph_node_mask"][9, 2499] = 3
    out["graph_edge_index"].view(torch.int16)[17].fill_(-1)
    out["graph_edge_mask"][299, :] = 9
    b.graph_observation()   # unchanged levels: nothing is rewritten
    assert float(out["graph_node_feats"][5, 0, 0]) == 7.0 and int(out["graph_node_mask"][9, 2499]) == 3
    b.graph_observation(rewrite_all=True)
    exp.check(out, ids, "rewrite all")
    fresh = {"graph_node_feats": torch.full((n, 2500, 6), float("nan"), device="cuda"),
             "graph_edge_index": torch.full((n, 2, 20000), 0x5A5A, dtype=torch.int16, device="cuda").view(torch.uint16),
             "graph_node_mask": torch.full((n, 2500), 0xA5, dtype=torch.uint8, device="cuda"),
             "graph_edge_mask": torch.full((n, 20000), 0xA5, dtype=torch.uint8, device="cuda")}
    assert set(fresh) == set(GRAPH_KEYS)
    exp.check(b.graph_observation(*[fresh[k] for k in KEYS]), ids, "fresh set")
    # an odd node-mask row offset: rows start at every alignment modulo 16
    base = torch.zeros(n * 2500 + 16, dtype=torch.uint8, device="cuda")
    fresh["graph_node_mask"] = base[4:4 + n * 2500].view(n, 2500)
    got = b.graph_observation(*[fresh[k] for k in KEYS])
    exp.check(got, ids, "node mask at offset 4")
    assert not base[:4].any() and not base[4 + n * 2500:].any()
    b.close()


def test_set_entity_pos_refused_and_several_exits_served():
    from nclone_amd.engine import NppBatch, graph_tables
    from nclone_amd.levels import curriculum0_levels

    base = next(m for m in curriculum0_levels()[0] if int(m[1156]) == 1 and int(m[1235]) == 3 and int(m[1240]) == 4)
    m = np.asarray(base, dtype=np.float64)
    door, switch, rest = m[1235:1240], m[1240:1245], m[1245:]
    door2, switch2 = door.copy(), switch.copy()
    door2[1] += 8
    switch2[1] += 8
    two = np.concatenate([m[:1235], door, door2, switch, switch2, rest])
    two[1156] = 2
    exp = Expected([base, two])
    b = NppBatch(64)
    b.load_levels([base, two])
    ids = np.arange(64) % 2
    b.assign_levels(ids)
    b.reset()
    exp.check(b.graph_observation(), ids, "two exits")
    assert graph_tables(two)[3] > 0
    b.set_entity_pos(3, 0, 200.0, 200.0)
    with pytest.raises(nat.NppError) as e:
        b.graph_observation()
    assert e.value.code == nat.NPP_ERR_UNSUPPORTED
    b.close()
    torch.cuda.synchronize()


def test_single_env_keys_match_observation_space():
    from nclone_amd.levels import door_levels
    from nclone_amd.vec_env import NppEnvironment

    env = NppEnvironment(map_data=door_levels()[0][0], enable_graph_observations=True)
    obs, _ = env.reset()
    for _ in range(3):
        obs = env.step(2)[0]
    space = env.observation_space
    for k in KEYS:
        assert k in space.keys() and k in obs
        assert obs[k].shape == space[k].shape and obs[k].dtype == space[k].dtype, k
    exp = Expected([door_levels()[0][0]])
    exp.check({k: obs[k][None] for k in KEYS}, [0], "single env")
    env.close()
    plain = NppEnvironment(map_data=door_levels()[0][0])
    assert not any(k in plain.observation_space.keys() for k in KEYS)
    assert not any(k in plain.reset()[0] for k in KEYS)
    plain.close()
    torch.cuda.synchronize()
