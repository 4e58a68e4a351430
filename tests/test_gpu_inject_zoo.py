"""The step kernel on injected ninja and mover states at the entity code's thresholds (tests/inject_zoo_states.py): every
row of the table is one env of one NppBatch; reset (the `fresh` rows are not), NppBatch.set_ninja_state, NppBatch.set_mover_state, then
TICKS single ticks with dumps after each.  The 12 state doubles, the 22 discrete columns and the entity checksum of EVERY env, and the
entity dump and the mover dump (npp_dump_movers: the checksum is a sum and cannot pin one mover) of every DUMP_STRIDE-th env are compared
BIT FOR BIT with the oracle's multiply-square twin, every tick up to and including the one that leaves the env terminal.

The PLAIN level runs alone -- a level set without zoo entities launches the plain kernels -- under the nine launch geometries / build
variants of tests/test_gpu_inject.py; the four zoo levels run together under four geometries.  There the host may raise the lanes per env
so that the zoo blocks of a workgroup fit in LDS: the requested geometry and the one that ran are recorded, and
test_zoo_effective_geometries requires three distinct effective lane counts among them.  Env orders as in tests/test_gpu_inject.py: `grouped` (levels in blocks of 64
envs: tables staged in LDS) and `interleaved` (round robin over the levels).  Every case is also compared with the first one of its
batch that ran.  tests/test_inject_zoo_host.py asserts from the oracle that the rows reach the thresholds they are built for.
"""
import os

import numpy as np
import pytest

from tests import inject_zoo_states as gen

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

POS_TOL = 1e-5   # the project's bars against the reference's fixtures (tests/test_gpu_zoo.py)
ENT_TOL = 1e-9
PLAIN_GEOMETRIES = [(1, 1, 0), (2, 2, 0), (4, 4, 0), (8, 4, 0), (32, 2, 0), (64, 1, 0), (16, 4, 0), (16, 4, 1), (16, 4, 2)]
ZOO_GEOMETRIES = [(1, 1, -1), (4, 2, -1), (16, 4, -1), (64, 1, -1)]   # variant -1: the handle's own choice, as in tests/test_gpu_zoo.py
ORDERS = ("grouped", "interleaved")
DUMP_STRIDE = 23
BATCHES = {"plain": (gen.PLAIN,), "zoo": (gen.STATIC, gen.MOVERS, gen.BALLS, gen.REAL)}
FIXTURE_RUN = {"plain": ((16, 4, 0), "grouped"), "zoo": ((16, 4, -1), "grouped")}


def _order(batch, name):
    """env -> row of the table (see tests/test_gpu_inject.py _order), over the rows of the batch's levels"""
    level = gen.states()["level"]
    lvs = BATCHES[batch]
    if name == "grouped":
        blocks = []
        for lv in lvs:
            rows = np.nonzero(level == lv)[0]
            blocks.append(np.concatenate([rows, rows[:-len(rows) % 64]]))
        return np.concatenate(blocks)
    rows = np.nonzero(np.isin(level, lvs))[0]
    rank = np.zeros(len(rows), dtype=np.int64)
    for lv in lvs:
        m = level[rows] == lv
        rank[m] = np.arange(m.sum())
    return rows[np.lexsort((level[rows], rank))]


def _runs(envs):
    """consecutive runs of a sorted env list as (first, count)"""
    if not len(envs):
        return []
    cut = np.nonzero(np.diff(envs) != 1)[0] + 1
    return [(int(r[0]), len(r)) for r in np.split(envs, cut)]


def _set_movers(b, perm):
    s = gen.states()
    for j in range(2):
        slot, field = s["mslot"][perm, j], s["mfield"][perm, j]
        for sl in np.unique(slot[slot >= 0]):
            for keep in (True, False):
                envs = np.nonzero((slot == sl) & ((field == gen.KEEP) == keep))[0]
                for e0, cnt in _runs(envs):
                    rows = perm[e0:e0 + cnt]
                    b.set_mover_state(int(sl), s["mxyab"][rows, j], None if keep else field[e0:e0 + cnt], env0=e0)


_DEVICE = {}    # (batch, geometry, order) -> run; only the first run of a batch and its FIXTURE_RUN are kept
_RAN = {}       # requested zoo geometry -> the one that ran


def _fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inject_zoo.npz"))


def _dumped_rows(batch, with_fixture):
    """every DUMP_STRIDE-th row of the batch; in its FIXTURE_RUN the fixture's rows too"""
    level = gen.states()["level"]
    rows = np.nonzero(np.isin(level, BATCHES[batch]))[0][::DUMP_STRIDE]
    if with_fixture:
        z = _fixture()
        rows = np.union1d(rows, z["idx"][np.isin(z["level"], BATCHES[batch])])
    return rows


def _device_run(batch, geometry, order):
    """dict F f64 [n, TICKS, 12], D i32 [n, TICKS, 22], C f64 [n, TICKS, 6] in table row order (rows of other batches stay 0), rows
    (the rows whose entities and movers were dumped), E i32 [len(rows), TICKS, 64], M f64 [len(rows), TICKS, N_MOVERS_MAX, 5]"""
    key = (batch, tuple(geometry), order)
    if key in _DEVICE:
        return _DEVICE[key]
    from nclone_amd.engine import NppBatch

    s = gen.states()
    perm = _order(batch, order)
    n = len(s["level"])
    lanes, waves, variant = geometry
    lvs = BATCHES[batch]
    b = NppBatch(len(perm), autoreset=False)
    b.load_levels([gen.level_maps()[lv] for lv in lvs])
    b.set_launch_geometry(lanes, waves)
    if variant >= 0:
        b.set_step_variant(variant)
    b.assign_levels(np.searchsorted(lvs, s["level"][perm]).astype(np.int64))   # first creation of the entities
    b.reset((~s["fresh"][perm]).astype(np.uint8))                               # ... which only the fresh rows keep
    b.set_ninja_state(s["xyv"][perm])
    _set_movers(b, perm)
    rows = _dumped_rows(batch, key[1:] == FIXTURE_RUN[batch])
    env_of = np.full(n, -1, dtype=np.int64)
    env_of[perm[::-1]] = np.arange(len(perm))[::-1]   # the first env that plays a row
    d_inputs = torch.from_numpy(np.ascontiguousarray(gen.inputs()[:, perm])).cuda()
    out = {"F": np.zeros((n, gen.TICKS, 12)), "D": np.zeros((n, gen.TICKS, 22), dtype=np.int32), "C": np.zeros((n, gen.TICKS, 6)), "rows": rows,
           "E": np.full((len(rows), gen.TICKS, 64), -1, dtype=np.int32), "M": np.full((len(rows), gen.TICKS, gen.N_MOVERS_MAX, 5), np.nan)}
    for t in range(gen.TICKS):
        b.tick(d_inputs[t:t + 1])
        f, di = b.dump_state()
        out["F"][perm, t], out["D"][perm, t], out["C"][perm, t] = f, di[:, :22], b.entity_checksum()
        for i, k in enumerate(rows):
            e = b.dump_entities(int(env_of[k]))
            out["E"][i, t, :len(e)] = e
            if batch == "zoo":
                m = b.dump_movers(int(env_of[k]))
                out["M"][i, t, :len(m)] = m
    ran = b.launch_geometry()
    if batch == "plain":
        assert ran == (lanes, waves) and b.step_variant()[0] == variant
    else:
        _RAN[(tuple(geometry), order)] = ran
    b.close()
    for a in out.values():
        a.setflags(write=False)
    first = not any(k[0] == batch for k in _DEVICE)
    if first or key[1:] == FIXTURE_RUN[batch]:
        _DEVICE[key] = out
    return out


def _compare(batch, run, want, rows_want):
    """run: a device run; want: dict with F, D, C, E, M over table rows (the oracle's run) or another device run (rows_want: its
    dumped rows, None for the oracle).  Bits, not values."""
    s = gen.states()
    valid = gen._ORACLE["mul"]["valid"]
    mine = np.isin(s["level"], BATCHES[batch])
    live = valid & mine[:, None]
    bad = live & ((run["F"].view(np.int64) != want["F"].view(np.int64)).any(axis=2) | (run["D"] != want["D"]).any(axis=2)
                  | (run["C"].view(np.int64) != want["C"].view(np.int64)).any(axis=2))
    if bad.any():
        k, t = (int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(("first of %d mismatching env-ticks" % int(bad.sum()), "row", k, gen.LEVEL_NAMES[s["level"][k]],
                              gen.FAMILY_NAMES[s["family"][k]], "tick", t, "injected", s["xyv"][k].tolist(), s["mslot"][k].tolist(),
                              s["mxyab"][k].tolist(), s["mfield"][k].tolist(), "device", run["F"][k, t].tolist(), run["D"][k, t].tolist(),
                              run["C"][k, t].tolist(), "expected", want["F"][k, t].tolist(), want["D"][k, t].tolist(), want["C"][k, t].tolist()))
    rows = run["rows"]
    if rows_want is None:
        wE, wM = want["E"][rows], want["M"][rows]
    else:
        common = np.intersect1d(rows, rows_want)
        sel, rows = np.searchsorted(rows, common), common
        wE, wM = want["E"][np.searchsorted(rows_want, common)], want["M"][np.searchsorted(rows_want, common)]
        run = {"E": run["E"][sel], "M": run["M"][sel]}
    lv = valid[rows]
    badE = lv & (run["E"] != wE).any(axis=2)
    assert not badE.any(), ("entity dump", int(rows[np.argwhere(badE)[0][0]]), np.argwhere(badE)[0].tolist())
    if batch == "zoo":
        badM = lv & (np.ascontiguousarray(run["M"]).view(np.int64) != np.ascontiguousarray(wM).view(np.int64)).any(axis=(2, 3))
        if badM.any():
            i, t = (int(v) for v in np.argwhere(badM)[0])
            k = int(rows[i])
            raise AssertionError(("mover dump: first of %d" % int(badM.sum()), "row", k, gen.FAMILY_NAMES[s["family"][k]], "tick", t, s["mslot"][k].tolist(),
                                  s["mxyab"][k].tolist(), s["mfield"][k].tolist(), "device", run["M"][i, t].tolist(), "expected", wM[i, t].tolist()))


def _case(batch, geometry, order, oracle_mod):
    want = gen.oracle_run(oracle_mod, "mul")
    first = next((v for k, v in _DEVICE.items() if k[0] == batch), None)
    run = _device_run(batch, geometry, order)
    _compare(batch, run, want, None)
    if first is not None and first is not run:
        _compare(batch, run, first, first["rows"])


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("geometry", PLAIN_GEOMETRIES, ids=lambda g: "g%dw%dv%d" % g)
def test_plain_level_bit_exact(geometry, order, oracle_mod):
    _case("plain", geometry, order, oracle_mod)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("geometry", ZOO_GEOMETRIES, ids=lambda g: "g%dw%d" % g[:2])
def test_zoo_levels_bit_exact(geometry, order, oracle_mod):
    _case("zoo", geometry, order, oracle_mod)
    print("requested", geometry[:2], order, "ran", _RAN[(tuple(geometry), order)])


def test_zoo_effective_geometries():
    """the host may raise the lanes per env so that the zoo blocks of a workgroup fit in LDS: what ran is recorded, not asserted
    equal to the request, but the four requests must still give three distinct lane counts"""
    from nclone_amd.engine import NppBatch

    ran = {}
    for lanes, waves, _ in ZOO_GEOMETRIES:
        b = NppBatch(64, autoreset=False)
        b.load_levels([gen.level_maps()[lv] for lv in BATCHES["zoo"]])
        b.set_launch_geometry(lanes, waves)
        b.assign_levels(np.arange(64) % len(BATCHES["zoo"]))
        b.tick(torch.zeros((1, 64), dtype=torch.uint8, device="cuda"))
        ran[(lanes, waves)] = b.launch_geometry()
        b.close()
    print("requested -> ran:", sorted(ran.items()), "; in the cases above:", sorted(_RAN.items()))
    for (g, order), got in _RAN.items():
        assert got == ran[g[:2]], (g, order, got)
    assert len({g[0] for g in ran.values()}) >= 3, ran


@pytest.mark.parametrize("batch", ["plain", "zoo"])
def test_vs_reference_fixture(batch):
    """the reference's own run of the fixture's subset of the rows under the project's bars: discrete rows identical, the ninja's
    four doubles within POS_TOL, the entity checksum and every mover's four doubles within ENT_TOL (the device squares by
    multiplication, the reference by pow)"""
    z = _fixture()
    s = gen.states()
    sel = np.isin(z["level"], BATCHES[batch])
    idx = z["idx"][sel]
    assert np.array_equal(np.ascontiguousarray(s["xyv"][idx]).view(np.uint64), z["xyv"][sel])
    assert np.array_equal(np.ascontiguousarray(s["mxyab"][idx]).view(np.uint64), z["mxyab"][sel])
    run = _device_run(batch, *FIXTURE_RUN[batch])
    live = np.arange(gen.TICKS)[None, :] < z["nt"][sel].astype(np.int64)[:, None]
    ref = z["t"][sel].view(np.float64)
    err = np.abs(run["F"][idx][:, :, :4] - ref)
    cerr = np.abs(run["C"][idx] - z["e"][sel])
    print("%s: max |device - reference| over %d state-ticks: ninja %.3g, checksum %.3g" % (batch, int(live.sum()), err[live].max(), cerr[live].max()))
    bad = live & ((err > POS_TOL).any(axis=2) | (run["D"][idx][:, :, :20].clip(0, 255) != z["d"][sel]).any(axis=2) | (cerr > ENT_TOL).any(axis=2))
    assert not bad.any(), ("first of %d" % bad.sum(), int(idx[np.argwhere(bad)[0][0]]), np.argwhere(bad)[0].tolist())
    if batch == "zoo":
        at = np.searchsorted(run["rows"], idx)
        assert np.array_equal(run["rows"][at], idx)
        merr = np.abs(np.nan_to_num(run["M"][at][:, :, :, :4], nan=0.0) - z["m"][sel].view(np.float64)).max(axis=(2, 3))
        print("zoo: max |device - reference| over the movers' doubles: %.3g" % merr[live].max())
        assert not (live & (merr > ENT_TOL)).any(), int(idx[np.argwhere(live & (merr > ENT_TOL))[0][0]])


def test_set_mover_state_writes_one_record_only(oracle_mod):
    """the aid itself: the four doubles and the 2-bit field of the named slot of the named envs and nothing else -- not the state
    dump, the entity dump, the other movers or the other envs, and (shown by the oracle twin staying equal over the following ticks)
    not the cell or the list-order number; refusals leave everything as it was"""
    from nclone_amd.engine import NppBatch

    n = 64
    lv = gen.MOVERS
    b = NppBatch(n, autoreset=False)
    b.load_levels([gen.level_maps()[lv], gen.level_maps()[gen.PLAIN]])
    b.assign_levels(np.zeros(n, dtype=np.int64))
    b.reset()
    acts = torch.full((n,), 2, dtype=torch.uint8, device="cuda")
    for _ in range(3):
        b.step(acts, 4)   # some history
    sims, done = [], np.zeros(n, dtype=bool)

    def twin_step(e):   # without auto-reset a terminal env is not stepped again
        if not done[e]:
            done[e] = sims[e].env_step(2, 4)[1] != 0

    for e in range(n):
        o = oracle_mod.Oracle("mul")
        o.load(gen.level_maps()[lv])
        o.reset()
        sims.append(o)
        for _ in range(3):
            twin_step(e)

    def snap():
        f, i = b.dump_state()
        return f, i, b.entity_checksum(), [b.dump_entities(e) for e in range(n)], np.stack([b.dump_movers(e) for e in range(n)])

    def same(a, c, movers=True):
        return (np.array_equal(a[0].view(np.int64), c[0].view(np.int64)) and np.array_equal(a[1], c[1]) and all(np.array_equal(x, y) for x, y in zip(a[3], c[3]))
                and (not movers or (np.array_equal(a[4].view(np.int64), c[4].view(np.int64)) and np.array_equal(a[2], c[2]))))

    s0 = snap()
    for e in range(n):
        assert np.array_equal(s0[4][e].view(np.int64), sims[e].dump_movers().view(np.int64)), e
    kinds = {k: t for k, t, _, _, _ in gen.movers(lv)}
    slot = {t: k for k, t in kinds.items()}   # one slot per type (the last thwump)
    e0, cnt = 7, 20
    # a thwump: x, y and the state; a drone: x, y, target and dir; a ball: x, y, speed
    writes = [(slot[20], np.column_stack([np.linspace(200, 400, cnt), np.full(cnt, 321.5), np.zeros(cnt), np.zeros(cnt)]), np.arange(cnt) % 3 - 1),
              (slot[14], np.column_stack([np.linspace(300, 500, cnt), np.full(cnt, 222.0), np.linspace(310, 510, cnt), np.full(cnt, 222.0)]), np.arange(cnt) % 4),
              (slot[25], np.column_stack([np.linspace(600, 700, cnt), np.linspace(150, 250, cnt), np.full(cnt, -3.25), np.full(cnt, -0.0)]), None)]
    prev = s0
    for sl, xyab, field in writes:
        b.set_mover_state(sl, xyab, field, env0=e0)
        for i in range(cnt):
            sims[e0 + i].set_mover(sl, *xyab[i], None if field is None else int(field[i]))
        s1 = snap()
        assert same(prev, s1, movers=False)   # state dump, entity dump
        want = prev[4].copy()
        want[e0:e0 + cnt, sl, :4] = xyab
        if field is not None:
            want[e0:e0 + cnt, sl, 4] = field
        assert np.array_equal(s1[4].view(np.int64), want.view(np.int64))   # bits: the -0.0 too; every other mover and env as before
        prev = s1
    # refusals: nothing written
    good = writes[0][1]
    for bad_call in (lambda: b.set_mover_state(len(kinds), good, env0=e0),                        # a slot past the level's movers
                     lambda: b.set_mover_state(slot[20], good, np.full(cnt, 2), env0=e0),           # a state a thwump does not have
                     lambda: b.set_mover_state(slot[14], good, np.full(cnt, 4), env0=e0),           # a dir a drone does not have
                     lambda: b.set_mover_state(slot[25], good, np.zeros(cnt, dtype=int), env0=e0),  # a ball has no field
                     lambda: b.set_mover_state(slot[28], good, np.zeros(cnt, dtype=int), env0=e0),  # a shove thwump's state is not writable
                     lambda: b.set_mover_state(slot[20], writes[1][1], env0=e0),                    # a thwump has no third / fourth value
                     lambda: b.set_mover_state(slot[20], good, env0=n - 10),                        # past the last env
                     lambda: b.set_mover_state(slot[20], good[:, :3], env0=e0)):
        with pytest.raises(ValueError):
            bad_call()
        assert same(prev, snap())
    for v in (np.nan, np.inf, -np.inf):
        x = good.copy()
        x[13, 1] = v
        with pytest.raises(ValueError):
            b.set_mover_state(slot[20], x, env0=e0)
        assert same(prev, snap())
    with pytest.raises(ValueError):
        sims[0].set_mover(slot[20], 1.0, 2.0, 0.0, 0.0, 2)
    with pytest.raises(ValueError):
        sims[0].set_mover(len(kinds), 1.0, 2.0, 0.0, 0.0)
    # a level without movers in the same level set: refused for its envs
    b.assign_levels(np.array([1]), env_ids=np.array([n - 1]))
    with pytest.raises(ValueError):
        b.set_mover_state(0, good[:1], env0=n - 1)
    b.assign_levels(np.array([0]), env_ids=np.array([n - 1]))
    sims[n - 1].load(gen.level_maps()[lv])
    done[n - 1] = False
    # cell and list-order number were left alone, like Entity.cell in the reference: the twin, whose setter leaves them alone by
    # construction, stays equal while the movers move on from where they were put
    for _ in range(4):
        b.step(acts, 4)
        for e in range(n):
            twin_step(e)
    f, i = b.dump_state()
    cs = b.entity_checksum()
    for e in range(n):
        of, od = sims[e].core()
        assert np.array_equal(f[e].view(np.int64), of.view(np.int64)) and np.array_equal(i[e, :22], od[:22]), e
        assert np.array_equal(cs[e], sims[e].entity_checksum()), e
        assert np.array_equal(b.dump_movers(e).view(np.int64), sims[e].dump_movers().view(np.int64)), e
    b.close()
