"""Host-side tests of the checkpoint archive (include/npp_amd.h npp_archive_create): the C entries are declared,
exported and bound; the list checks of NppBatch.archive_store / archive_restore that need no device; the constructor refusals.
The kernels are tested in tests/test_gpu_archive.py."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("npp_archive_create", "npp_archive_store", "npp_archive_restore", "npp_archive_meta_view", "npp_archive_num_slots")


def test_entries_declared_exported_and_bound():
    from nclone_amd import _native as nat

    hdr = open(os.path.join(ROOT, "include", "npp_amd.h")).read()
    lib = nat.lib()
    for name in ENTRIES:
        assert "int %s(npp_handle h" % name in hdr, name
        assert name in nat.EXPORTS, name
        fn = getattr(lib, name)   # AttributeError when the library does not export it
        assert fn.argtypes is not None and fn.argtypes[0] is C.c_void_p and fn.restype is C.c_int, name
    assert len(lib.npp_archive_store.argtypes) == 5 and len(lib.npp_archive_restore.argtypes) == 5
    assert len(lib.npp_archive_meta_view.argtypes) == 3 and len(lib.npp_archive_create.argtypes) == 2
    # the reference lines the feature answers to
    for cite in ("state_checkpoint.py:26", "base_environment.py:1769-1789", "demo_checkpoint_seeder.py:284-287", "truncation_checker.py:53-58"):
        assert cite in hdr, cite
    # without a handle the entries answer instead of crashing
    assert lib.npp_archive_num_slots(None) == 0
    assert lib.npp_archive_create(None, 4) == nat.NPP_ERR_INVALID
    assert lib.npp_archive_store(None, None, None, 0, None) == nat.NPP_ERR_INVALID


def test_list_checks_need_no_device():
    from nclone_amd.engine import check_archive_lists

    ok = check_archive_lists([3, 70, 130], [5, 0, 2], "slots", "archive_store")
    assert ok["envs"].tolist() == [3, 70, 130] and ok["slots"].tolist() == [5, 0, 2]
    # one slot into many envs is the normal restore; one env into many slots is a fine store
    check_archive_lists([10, 150, 100], [5, 5, 0], "envs", "archive_restore")
    check_archive_lists([3, 3], [0, 1], "slots", "archive_store")
    with pytest.raises(ValueError, match="archive_restore: the same env comes twice"):
        check_archive_lists([10, 10], [5, 0], "envs", "archive_restore")
    with pytest.raises(ValueError, match="archive_store: the same slot comes twice"):
        check_archive_lists([1, 2], [4, 4], "slots", "archive_store")
    # skipped entries (a negative env or slot: the padding of a fixed-length list) are no duplicates
    check_archive_lists([-1, -1, 7, 7], [2, 3, -1, 1], "envs", "archive_restore")
    check_archive_lists([0, 1, 2], [-1, -1, 4], "slots", "archive_store")
    with pytest.raises(ValueError, match="differ in length"):
        check_archive_lists([1, 2, 3], [0, 1], "envs", "archive_restore")
    with pytest.raises(ValueError, match="one-dimensional"):
        check_archive_lists([[1, 2]], [[0, 1]], "envs", "archive_restore")
    with pytest.raises(TypeError, match="slots must hold integers"):
        check_archive_lists([1, 2], [0.0, 1.0], "envs", "archive_restore")
    with pytest.raises(TypeError, match="envs must be an int32 tensor"):
        check_archive_lists(torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), "envs", "archive_restore")
    # tensors are taken as they are: the device decides every entry
    t = check_archive_lists(torch.tensor([1, 1], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32), "envs", "archive_restore")
    assert isinstance(t["envs"], torch.Tensor)


def test_constructor_refusals_need_no_device():
    from nclone_amd.async_env import NppAsyncVecEnvironment
    from nclone_amd.vec_env import NppEnvironment, NppVecEnvironment

    lvl = [np.zeros(1)]
    with pytest.raises(ValueError, match="checkpoint_slots with level_weights"):
        NppVecEnvironment(lvl, 64, checkpoint_slots=8, level_weights=[1.0])
    with pytest.raises(ValueError, match="checkpoint_slots must be >= 0"):
        NppVecEnvironment(lvl, 64, checkpoint_slots=-1)
    with pytest.raises(ValueError, match="checkpoint_slots must be >= 0"):
        NppEnvironment(map_data=lvl[0], checkpoint_slots=-1)
    with pytest.raises(NotImplementedError, match="checkpoint archive"):
        NppAsyncVecEnvironment(lvl, 64, checkpoint_slots=8)
