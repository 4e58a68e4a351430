"""Frame stacking without a GPU: the numpy model (tests/frame_stack_ref.py) against the reference wrapper's own output
(tests/golden/stack.npz, make_golden_stack.py), the stacked observation spaces, and the argument checks."""
import numpy as np
import pytest

from nclone_amd import spaces
from tests.frame_stack_ref import StackModel

PAD = ("zero", "repeat")


def _cfgs(golden):
    return [tuple(int(v) for v in row) for row in golden.z("stack")["cfg"]]


def test_fixture_covers_the_issue_grid(golden):
    cfg = _cfgs(golden)
    assert {c[0] for c in cfg} >= {1, 2, 4, 12} and {c[2] for c in cfg} == {0, 1}
    assert {c[3] for c in cfg} == {0, 1} and {c[4] for c in cfg} == {0, 1} and any(c[5] == 0 for c in cfg)


def test_model_reproduces_reference_wrapper(golden):
    z = golden.z("stack")
    ev = z["events"]
    for c, (vk, sk, pad, ven, sen, with_pf) in enumerate(_cfgs(golden)):
        assert z["c%d_pass" % c].all()   # global_view / action_mask passed through unchanged
        keys = [("gs", "gs_in", sk if sen else 0)]
        if with_pf:
            keys.append(("pf", "pf_in", vk if ven else 0))
        for name, src, k in keys:
            want = z["c%d_%s" % (c, name)]
            inp = z[src]
            if not k:   # not stacked: the observation itself
                np.testing.assert_array_equal(want, inp)
                continue
            m = StackModel(k, PAD[pad])
            for i in range(len(ev)):
                got = m.push(inp[i][None], np.array([ev[i] != 0]))[0]
                assert got.dtype == want.dtype and got.shape == want[i].shape
                np.testing.assert_array_equal(got, want[i], err_msg="config %d key %s call %d" % (c, name, i))


def test_model_terminal_stack():
    m = StackModel(3, "zero")
    x = np.arange(4 * 2, dtype=np.float32).reshape(4, 2)
    m.push(x[:1], [True])
    m.push(x[1:2], [False])
    new, term = m.push(x[2:3], [True], terminal=x[3:4])
    np.testing.assert_array_equal(new[0], [[0, 0], [0, 0], [4, 5]])
    np.testing.assert_array_equal(term[0], [[0, 1], [2, 3], [6, 7]])


def test_stacked_observation_space_matches_reference(golden):
    z = golden.z("stack")
    for c, (vk, sk, pad, ven, sen, with_pf) in enumerate(_cfgs(golden)):
        sp = spaces.observation_space(visual=bool(with_pf), visual_stack=vk if ven and with_pf else 0, state_stack=sk if sen else 0)
        dts = z["c%d_space_dt" % c]
        for j, (key, name) in enumerate((("player_frame", "pf"), ("game_state", "gs"))):
            if "c%d_space_%s" % (c, name) not in z.files:
                assert key not in sp.spaces
                continue
            ref = z["c%d_space_%s" % (c, name)]
            b = sp[key]
            assert tuple(b.shape) == tuple(int(v) for v in ref[2:]), (c, key)
            assert np.dtype(b.dtype).num == int(dts[j]), (c, key)
            assert float(np.min(b.low)) == ref[0] and float(np.max(b.high)) == ref[1], (c, key)
        if with_pf:
            assert tuple(sp["global_view"].shape) == (176, 100, 1)


def test_unstacked_space_unchanged():
    sp = spaces.observation_space(visual=True)
    assert tuple(sp["player_frame"].shape) == (84, 84, 1) and tuple(sp["game_state"].shape) == (41,)


@pytest.mark.parametrize("kw,idx", [({"visual_stack_size": 0}, 0), ({"visual_stack_size": 13}, 1), ({"state_stack_size": 0}, 2),
                                    ({"state_stack_size": 13}, 3), ({"padding_type": "edge"}, 4)])
def test_argument_errors_match_reference(golden, kw, idx):
    msg = bytes(golden.z("stack")["errors"]).decode().split("\n")[idx]
    assert msg
    with pytest.raises(ValueError) as e:
        spaces.check_frame_stack(**kw)
    assert str(e.value) == msg
    # the envs check before touching the device
    from nclone_amd.vec_env import NppEnvironment, NppVecEnvironment

    ekw = {{"padding_type": "frame_stack_padding_type"}.get(k, k): v for k, v in kw.items()}
    with pytest.raises(ValueError) as e:
        NppVecEnvironment([np.zeros(1335)], 1, enable_visual_frame_stacking=True, enable_state_stacking=True, **ekw)
    assert str(e.value) == msg
    with pytest.raises(ValueError) as e:
        NppEnvironment(map_data=np.zeros(1335), **ekw)
    assert str(e.value) == msg


def test_valid_sizes_accepted():
    for k in (1, 12):
        spaces.check_frame_stack(k, k, "zero")
        spaces.check_frame_stack(k, k, "repeat")
