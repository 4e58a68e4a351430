"""GPU tests of the snapshot slot (include/npp_amd.h npp_snapshot / npp_restore; DESIGN.md 16, identity mode): the slot is one record
per env in the checkpoint archive's layout, moved by the archive's kernel with entry i = env i = record i under an env mask.
The shape: 70 envs (more than one wavefront of entries, and no multiple of the kernel's 4 entries per workgroup, so the last
workgroup is partial) assigned round-robin to one mine, one door and one zoo level (n_words_max exceeds some level's own word
count, and the zoo block is present)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N = 70
LEVEL_IDS = np.arange(N) % 3
TRUNCATED = 8   # NPP_F_TRUNCATED


def _levels():
    from nclone_amd import levels as lv

    return [getattr(lv, which + "_levels")()[0][0] for which in ("mine", "door", "zoo")]


def _batch(levels=None, level_ids=LEVEL_IDS):
    from nclone_amd.engine import NppBatch

    b = NppBatch(N, outputs=("spatial_context",))
    b.load_levels(_levels() if levels is None else levels)
    b.assign_levels(level_ids)
    return b


def _acts(seed, steps):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 6, size=(steps, N)).astype(np.uint8)).cuda()


def _full(b, observe=False):
    """Everything the parity hooks show of every env, and its spatial_context row (of the last step, or of an observe() now)."""
    if observe:
        b.observe()
    f, i = b.dump_state()
    return {"f": f, "i": i, "cs": b.entity_checksum(), "ent": [b.dump_entities(e) for e in range(N)],
            "sc": b.to_host(("spatial_context",))["spatial_context"].copy()}


def _rows_equal(a, b, e):
    return (np.array_equal(a["f"][e], b["f"][e]) and np.array_equal(a["i"][e], b["i"][e]) and
            np.array_equal(a["cs"][e], b["cs"][e], equal_nan=True) and np.array_equal(a["ent"][e], b["ent"][e]) and
            np.array_equal(a["sc"][e], b["sc"][e]))


def test_masked_restore_against_a_twin():
    a, b = _batch(), _batch()
    acts = _acts(11, 35)
    for t in range(20):
        a.step(acts[t])
        b.step(acts[t])
    a.snapshot()
    b.snapshot()
    at_snapshot = _full(a)
    for t in range(20, 35):
        a.step(acts[t])
        b.step(acts[t])
    first_time = _full(a)
    assert not np.array_equal(first_time["f"], at_snapshot["f"])
    mask = (np.arange(N) % 3 == 0).astype(np.uint8)
    a.restore(mask)
    after, twin = _full(a, observe=True), _full(b, observe=True)
    for e in range(N):
        assert _rows_equal(after, at_snapshot if mask[e] else twin, e), e
    for t in range(20, 35):   # the earlier 15 actions again: the masked envs do what they did the first time
        a.step(acts[t])
    again = _full(a)
    for e in np.flatnonzero(mask):
        assert _rows_equal(again, first_time, e), e
    a.close()
    b.close()


def test_truncation_limit_set_after_the_snapshot_survives_restore_without_a_pool():
    """Without a level pool npp_restore leaves the live truncation limits alone: the step that crosses the new limit truncates."""
    limit, steps = 1234, 330
    b = _batch()
    b.set_truncation_limit(100000)
    noop = torch.zeros(N, dtype=torch.uint8).cuda()
    for _ in range(3):
        b.step(noop)
    b.snapshot()
    b.set_truncation_limit(limit)
    b.step(noop)
    b.restore()
    frame0 = b.dump_state()[1][:, 22].astype(np.int64)   # (dump column 22: the frame count the limit is compared with)
    flags = torch.zeros((steps, N), dtype=torch.uint8).cuda()
    ticks = torch.zeros((steps, N), dtype=torch.int16).cuda()
    for t in range(steps):
        b.step(noop)
        flags[t].copy_(b.flags)
        ticks[t].copy_(b.frames)
    b.sync()
    flags, ticks = flags.cpu().numpy(), ticks.cpu().numpy().astype(np.int64)
    checked = 0
    for e in range(N):
        ended = np.flatnonzero(flags[:, e] & (1 | 2 | TRUNCATED))
        if len(ended) == 0 or flags[ended[0], e] & 3:
            continue   # won or died first: that episode's frame count never reached the limit
        t = ended[0]
        frame = frame0[e] + np.cumsum(ticks[: t + 1, e])
        assert frame[t] >= limit and (t == 0 or frame[t - 1] < limit), (e, t, frame[t])
        checked += 1
    assert checked > 0   # (envs of one level all do the same under no-ops: a level's envs get there together or not at all)
    b.close()


def test_restore_after_a_layout_change_needs_a_new_snapshot():
    from nclone_amd import _native as nat

    b = _batch()
    b.archive_create(1)
    before = b.archive_record_bytes()
    acts = _acts(13, 10)
    for t in range(5):
        b.step(acts[t])
    b.snapshot()
    b.load_levels(_levels()[:1])   # the mine level alone: another n_words_max and zoo block, so another record layout
    b.archive_create(1)
    assert b.archive_record_bytes() != before
    with pytest.raises(nat.NppError) as ei:
        b.restore()
    assert ei.value.code == nat.NPP_ERR_STATE
    for t in range(5):
        b.step(acts[t])
    b.snapshot()
    at_snapshot = _full(b)
    for t in range(5, 10):
        b.step(acts[t])
    assert not np.array_equal(_full(b)["f"], at_snapshot["f"])
    b.restore()
    after = _full(b, observe=True)
    for e in range(N):
        assert _rows_equal(after, at_snapshot, e), e
    b.close()
