"""Host-side tests of the cell index over the checkpoint archive (include/npp_amd.h npp_archive_cells_create): the
six C entries are declared, exported and bound; the two GPU-free entries equal the Python restatement (tests/cell_archive_ref.py)
on hand-made rows and table fillings; the refusals of the host classes that need no device.  The kernels are tested in
tests/test_gpu_cell_archive.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from tests import cell_archive_ref as ref

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"npp_archive_cells_create": 3, "npp_archive_explore": 4, "npp_archive_select": 3, "npp_archive_cells_view": 7,
           "npp_archive_cell_keys_host": 8, "npp_archive_cell_pick_host": 8}


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def test_entries_declared_exported_and_bound():
    from nclone_amd import _native as nat

    hdr = open(os.path.join(ROOT, "include", "npp_amd.h")).read()
    lib = nat.lib()
    for name, argc in ENTRIES.items():
        assert "int %s(" % name in hdr, name
        assert name in nat.EXPORTS, name
        fn = getattr(lib, name)   # AttributeError when the library does not export it
        assert fn.argtypes is not None and len(fn.argtypes) == argc and fn.restype is C.c_int, name
    for cite in ("demo_checkpoint_seeder.py", ":283-287", ":427-435", ":118-153", ":1-13"):
        assert cite in hdr, cite
    # without a handle the entries answer instead of crashing
    assert lib.npp_archive_cells_create(None, 1, 0) == nat.NPP_ERR_INVALID
    assert lib.npp_archive_explore(None, None, None, None) == nat.NPP_ERR_INVALID
    assert lib.npp_archive_select(None, None, None) == nat.NPP_ERR_INVALID
    assert lib.npp_archive_cells_view(None, None, None, None, None, None, None) == nat.NPP_ERR_INVALID
    assert lib.npp_archive_cell_keys_host(None, 0, 0, None, None, None, 0, None) == nat.NPP_ERR_INVALID
    assert lib.npp_archive_cell_pick_host(None, None, None, 0, 0, None, 0, None) == nat.NPP_ERR_INVALID


def _rows(door):
    """About 100 hand-made rows (x, y, ninja state, switch state) around the borders the rule has, for a level whose door is `door`."""
    rows = []
    inside = (100.5, 200.25)
    # positions exactly on cell borders, the grid's edges and outside it (negative coordinates and -0.0 included)
    for c in (0, 1, 2, 17, 43, 44, 45):
        rows.append((24.0 * c, 24.0 * 3, 0, 1))
        rows.append((np.nextafter(24.0 * c, -np.inf), 30.0, 0, 1))
    for c in (0, 1, 24, 25, 26):
        rows.append((24.0 * 5, 24.0 * c, 1, 1))
        rows.append((130.0, np.nextafter(24.0 * c, -np.inf), 1, 1))
    for x, y in ((-0.0, -0.0), (-1e-300, 5.0), (5.0, -1e-300), (-24.0, 100.0), (100.0, -0.5), (1056.0, 599.999), (1055.999, 600.0),
                 (1e300, 10.0), (10.0, -1e300), (float("nan"), 10.0), (10.0, float("inf")), (float("-inf"), 10.0), (1055.999, 599.999)):
        rows.append((x, y, 0, 1))
        rows.append((x, y, 0, 0))
    # every ninja state, every switch state
    for state in range(10):
        for sw in (0, 1, 2):
            rows.append((inside[0] + state, inside[1] + 24.0 * sw, state, sw))
    rows += [(inside[0], inside[1], -1, 1), (inside[0], inside[1], 15, 1)]
    # the exit filter: 71.999, 72.0 and 72.001 px from the door, along an axis and along a 3-4-5 diagonal, switch on (0, 2) and off (1)
    for d in (71.999, 72.0, 72.001, 0.0, 500.0):
        for ux, uy in ((1.0, 0.0), (0.0, -1.0), (-0.6, 0.8), (0.8, 0.6)):
            for sw in (0, 1, 2):
                rows.append((door[0] + d * ux, door[1] + d * uy, 0, sw))
    return rows


def test_cell_keys_host_equals_the_restatement():
    from nclone_amd import _native as nat
    from nclone_amd import levels as lv

    lib = nat.lib()
    total = 0
    for level, m in ((0, lv.door_levels()[0][0]), (3, lv.mine_levels()[0][0])):
        door = ref.door_of(m)
        assert door is not None
        rows = _rows(door)
        total += len(rows)
        xy = np.array([[r[0], r[1]] for r in rows], dtype=np.float64)
        state = np.array([r[2] for r in rows], dtype=np.int32)
        sw = np.array([r[3] for r in rows], dtype=np.int32)
        want = np.array([ref.key_in_level(int(s), int(w), float(x), float(y), door) for (x, y), s, w in zip(xy, state, sw)])
        want = np.where(want < 0, -1, level * ref.CELLS_PER_LEVEL + want).astype(np.int32)
        got = np.full(len(rows), -7, dtype=np.int32)
        mm = np.ascontiguousarray(np.asarray(m, dtype=np.float64))
        rc = lib.npp_archive_cell_keys_host(mm.ctypes.data_as(C.POINTER(C.c_double)), len(mm), level, _ptr(xy), _ptr(state), _ptr(sw),
                                            len(rows), _ptr(got))
        assert rc == nat.NPP_OK
        assert np.array_equal(got, want), np.nonzero(got != want)[0]
        # the rows do exercise both answers of every test of the rule
        on_axis = [k for k, r in enumerate(rows) if r[3] != 1 and abs(math.hypot(r[0] - door[0], r[1] - door[1]) - 72.0) < 0.01]
        assert {int(want[k]) < 0 for k in on_axis} == {True, False}
        assert (want >= 0).sum() > 40 and (want < 0).sum() > 40
        assert len({(k % ref.CELLS_PER_LEVEL) // 1100 for k in want if k >= 0}) == 2   # both switch planes
    assert total >= 200


def _fillings():
    K = ref.CELLS_PER_LEVEL
    rng = np.random.default_rng(17)
    empty = (np.full(K, -1, np.int32), np.zeros(K, np.uint32), np.zeros(K, np.uint32))
    one = (np.full(K, -1, np.int32), rng.integers(0, 50, K).astype(np.uint32), np.zeros(K, np.uint32))
    one[0][1234] = 7
    full = (rng.permutation(K).astype(np.int32), np.zeros(K, np.uint32), np.zeros(K, np.uint32))
    slot = np.full(K, -1, np.int32)
    occ = rng.choice(K, size=300, replace=False)
    slot[occ] = rng.permutation(300).astype(np.int32)
    visits = rng.integers(0, 2000, K).astype(np.uint32)
    visits[occ[:20]] = (2 ** 31 - rng.integers(0, 3, 20)).astype(np.uint32)   # visits up to 2^31
    visits[occ[20:40]] = 0
    chosen = rng.integers(0, 40, K).astype(np.uint32)
    return {"empty": empty, "one": one, "full": full, "mixed": (slot, visits, chosen)}


@pytest.mark.parametrize("filling", ["empty", "one", "full", "mixed"])
def test_cell_pick_host_equals_the_restatement(filling):
    from nclone_amd import _native as nat

    lib = nat.lib()
    slot, visits, chosen = _fillings()[filling]
    envs = np.concatenate([np.arange(60), [8191, 65535, 2 ** 20 + 3, 2 ** 31 - 1]]).astype(np.int32)   # 64 envs
    seed = 0x9E3779B97F4A7C15
    seen = set()
    for call in (0, 1, 2, 77, 2 ** 32 - 1):
        got = np.full(len(envs), -7, dtype=np.int32)
        rc = lib.npp_archive_cell_pick_host(_ptr(slot), _ptr(visits), _ptr(chosen), seed, call, _ptr(envs), len(envs), _ptr(got))
        assert rc == nat.NPP_OK
        want = np.array([ref.pick_in_level(slot, visits, chosen, seed, call, int(e))[0] for e in envs], dtype=np.int32)
        assert np.array_equal(got, want), (call, np.nonzero(got != want)[0])
        seen.update(got.tolist())
    if filling == "empty":
        assert seen == {-1}
    elif filling == "one":
        assert seen == {7}
    else:
        assert -1 not in seen and len(seen) > 100   # the draws spread over the occupied keys


def test_weight_is_the_count_rule():
    assert ref.weight(0, 0) == 1048576 and ref.weight(3, 0) == 524288 and ref.weight(1, 2) == 524288
    assert ref.weight(2 ** 31, 5) == int(math.floor(1048576.0 / math.sqrt(2.0 ** 31 + 6.0))) > 0
    assert ref.ordered_bits(-0.0) < ref.ordered_bits(0.0) < ref.ordered_bits(1.0) < ref.ordered_bits(float("inf"))
    assert 0 < ref.ordered_bits(float("-inf")) < ref.ordered_bits(-1.0) < ref.ordered_bits(-0.0)


def test_refusals_need_no_device():
    from nclone_amd.async_env import NppAsyncVecEnvironment
    from nclone_amd.engine import check_cell_arg
    from nclone_amd.vec_env import NppEnvironment, NppVecEnvironment

    lvl = [np.zeros(1)]
    with pytest.raises(ValueError, match="checkpoint_cells needs checkpoint_slots"):
        NppVecEnvironment(lvl, 64, checkpoint_cells=True)
    with pytest.raises(ValueError, match="checkpoint_cells needs checkpoint_slots"):
        NppEnvironment(map_data=lvl[0], checkpoint_cells=True)
    with pytest.raises(ValueError, match="checkpoint_slots with level_weights"):
        NppVecEnvironment(lvl, 64, checkpoint_slots=8, checkpoint_cells=True, level_weights=[1.0])
    with pytest.raises(NotImplementedError, match="checkpoint archive"):
        NppAsyncVecEnvironment(lvl, 64, checkpoint_cells=True)
    # the per-env arguments of archive_explore / archive_select
    assert check_cell_arg([1, 0, 1], torch.uint8, 3, "mask").dtype == np.uint8
    assert check_cell_arg(np.array([True, False]), torch.uint8, 2, "mask").tolist() == [1, 0]
    assert check_cell_arg(torch.tensor([True, False]), torch.uint8, 2, "mask").dtype == torch.uint8
    assert check_cell_arg([1, 2.5], torch.float32, 2, "score").dtype == np.float32
    with pytest.raises(ValueError, match=r"score must be \[3\]"):
        check_cell_arg([1.0, 2.0], torch.float32, 3, "score")
    with pytest.raises(ValueError, match="one value per env"):
        check_cell_arg(np.zeros((2, 2)), torch.float32, 2, "score")
    with pytest.raises(TypeError, match="score must be a float32 tensor"):
        check_cell_arg(torch.zeros(2, dtype=torch.float64), torch.float32, 2, "score")
    with pytest.raises(TypeError, match="mask must be a uint8 tensor"):
        check_cell_arg(torch.zeros(2, dtype=torch.int32), torch.uint8, 2, "mask")
