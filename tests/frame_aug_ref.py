"""Numpy model of the frame augmentation (include/npp_amd.h, npp_set_frame_augmentation; nclone_amd/csrc/npp_augment.hpp;
DESIGN.md 15).  The transforms, their order and gates are the reference's pipeline (gym_environment/frame_augmentation.py:56-103);
the pixels are the project's own integer definition -- parity with albumentations' pixels is unpinned -- and the draws are a
counter-based hash, not numpy's stream.

Parameters of one frame: 14 int32 words
    0 gate mask (1 translate, 2 flip, 4 dropout, 8 brightness / contrast)   1 sx  2 sy (1/32 px)   3 hole count
    4-7 hole 0 (h, w, y0, x0)   8-11 hole 1   12 a   13 b
Draw for env e, augmentation call count c, target t (0 player_frame 84 x 84, 1 global_view 176 x 100):
    base = mix(mix((e << 32) | c) ^ seed ^ (t * 0xD1B54A32D192ED03)), word j = mix(base + j)
    words: 0 translate gate, 1 sx, 2 sy, 3 flip gate, 4 dropout gate, 5 hole count, 6-9 hole 0, 10-13 hole 1, 14 b/c gate, 15 a, 16 b
    gate: (word >> 11) * 2^-53 < probability; integer in [lo, hi]: lo + (((word >> 32) * (hi - lo + 1)) >> 32)
"""
import numpy as np

from tests.level_pool_ref import _mix

_U = np.uint64
WORDS = 14
TRANSLATE, FLIP, DROPOUT, BC = 1, 2, 4, 8
SCALE10 = {"light": 7, "medium": 10, "strong": 13}   # s = 0.7 / 1.0 / 1.3
SHAPES = ((84, 84), (176, 100))                      # target 0 player_frame, 1 global_view (H, W)
GATE_P = (0.8, 0.4, 0.5, 0.4)                        # translate, flip, dropout, brightness / contrast: times p


def limits(intensity, H, W):
    """The ranges of the draw, in exact integers: Qx = floor(32 * 4 s / 84 * W), Qy likewise, holes int(6 s) .. int(12 s),
    A = round(25.6 s), B = round(6528 s) (0.1 s * 255 in 1/256 grey levels)."""
    s10 = SCALE10[intensity]
    return {"qx": 128 * s10 * W // 840, "qy": 128 * s10 * H // 840, "hole_lo": 6 * s10 // 10, "hole_hi": 12 * s10 // 10,
            "A": (256 * s10 + 50) // 100, "B": (6528 * s10 + 5) // 10}


def _uniform(word, lo, hi):
    lo = np.asarray(lo, dtype=np.int64)
    span = (np.asarray(hi, dtype=np.int64) - lo + 1).astype(np.uint64)
    with np.errstate(over="ignore"):
        return lo + (((word >> _U(32)) * span) >> _U(32)).astype(np.int64)


def _gate(word, prob):
    return (word >> _U(11)).astype(np.float64) * (2.0 ** -53) < prob


def draw(seed, envs, counts, targets, p=0.5, intensity="medium"):
    """int32 [n, 14]: the parameters env envs[i] draws at augmentation call counts[i] for target targets[i]."""
    e = np.asarray(envs).astype(np.uint64).ravel()
    c = np.asarray(counts).astype(np.uint64).ravel()
    t = np.asarray(targets).astype(np.int64).ravel()
    with np.errstate(over="ignore"):
        base = _mix(_mix((e << _U(32)) | c) ^ _U(int(seed) & (2**64 - 1)) ^ (t.astype(np.uint64) * _U(0xD1B54A32D192ED03)))
        w = [_mix(base + _U(j)) for j in range(17)]
    H = np.where(t == 1, SHAPES[1][0], SHAPES[0][0])
    W = np.where(t == 1, SHAPES[1][1], SHAPES[0][1])
    L0, L1 = limits(intensity, *SHAPES[0]), limits(intensity, *SHAPES[1])
    qx = np.where(t == 1, L1["qx"], L0["qx"])
    qy = np.where(t == 1, L1["qy"], L0["qy"])
    lo, hi, A, B = L0["hole_lo"], L0["hole_hi"], L0["A"], L0["B"]
    out = np.zeros((len(e), WORDS), dtype=np.int64)
    out[:, 0] = (_gate(w[0], GATE_P[0] * p) * TRANSLATE + _gate(w[3], GATE_P[1] * p) * FLIP + _gate(w[4], GATE_P[2] * p) * DROPOUT
                 + _gate(w[14], GATE_P[3] * p) * BC)
    out[:, 1] = _uniform(w[1], -qx, qx)
    out[:, 2] = _uniform(w[2], -qy, qy)
    out[:, 3] = _uniform(w[5], 1, 2)
    for i in range(2):
        h = _uniform(w[6 + 4 * i], lo, hi)
        ww = _uniform(w[7 + 4 * i], lo, hi)
        out[:, 4 + 4 * i] = h
        out[:, 5 + 4 * i] = ww
        out[:, 6 + 4 * i] = _uniform(w[8 + 4 * i], 0, H - h)
        out[:, 7 + 4 * i] = _uniform(w[9 + 4 * i], 0, W - ww)
    out[:, 12] = _uniform(w[15], 256 - A, 256 + A)
    out[:, 13] = _uniform(w[16], -B, B)
    return out.astype(np.int32)


def make_params(mask=0, sx=0, sy=0, holes=0, hole0=(0, 0, 0, 0), hole1=(0, 0, 0, 0), a=256, b=0):
    """One parameter row from named values (tests that force parameters)."""
    return np.array([mask, sx, sy, holes, *hole0, *hole1, a, b], dtype=np.int32)


def _taps(f, yi, xi):
    """f [n, H, W] at rows yi [n, H], columns xi [n, W]; pixels outside the image count as 0."""
    n, H, W = f.shape
    vy, vx = (yi >= 0) & (yi < H), (xi >= 0) & (xi < W)
    g = f[np.arange(n)[:, None, None], np.clip(yi, 0, H - 1)[:, :, None], np.clip(xi, 0, W - 1)[:, None, :]]
    return g * (vy[:, :, None] & vx[:, None, :])


def apply(frame, params):
    """The augmented frame(s).  frame: u8 [H, W] with params [14], or [n, H, W] with params [n, 14] (row i for frame i).

    1. translate: X = 32 x - sx, x0 = X >> 5, fx = X & 31 (same for y), v = ((32 - fx)(32 - fy) p00 + fx (32 - fy) p01 +
       (32 - fx) fy p10 + fx fy p11 + 512) >> 10, pixels outside the image 0;  2. flip: column x reads translated column W - 1 - x;
    3. dropout: the first `hole count` holes become 0, in output coordinates;  4. v = clamp((a v + b) >> 8, 0, 255), holes included.
    """
    f = np.asarray(frame)
    q = np.asarray(params, dtype=np.int64)
    single = f.ndim == 2
    if single:
        f, q = f[None], q[None]
    assert f.dtype == np.uint8 and f.ndim == 3 and q.shape == (f.shape[0], WORDS)
    n, H, W = f.shape
    v = f.astype(np.int64)
    mask = q[:, 0]
    tr = (mask & TRANSLATE) != 0
    sx, sy = np.where(tr, q[:, 1], 0), np.where(tr, q[:, 2], 0)   # (a zero shift is the identity: fx = fy = 0)
    X = 32 * np.arange(W)[None, :] - sx[:, None]
    Y = 32 * np.arange(H)[None, :] - sy[:, None]
    x0, fx, y0, fy = X >> 5, (X & 31)[:, None, :], Y >> 5, (Y & 31)[:, :, None]
    v = ((32 - fx) * (32 - fy) * _taps(v, y0, x0) + fx * (32 - fy) * _taps(v, y0, x0 + 1) + (32 - fx) * fy * _taps(v, y0 + 1, x0)
         + fx * fy * _taps(v, y0 + 1, x0 + 1) + 512) >> 10
    v = np.where(((mask & FLIP) != 0)[:, None, None], v[:, :, ::-1], v)
    yy, xx = np.arange(H)[None, :, None], np.arange(W)[None, None, :]
    for i in range(2):
        h, w, ty, tx = (q[:, 4 + 4 * i + j][:, None, None] for j in range(4))
        on = (((mask & DROPOUT) != 0) & (q[:, 3] > i))[:, None, None]
        v = np.where(on & (yy >= ty) & (yy < ty + h) & (xx >= tx) & (xx < tx + w), 0, v)
    bc = ((mask & BC) != 0)[:, None, None]
    v = np.where(bc, np.clip((q[:, 12][:, None, None] * v + q[:, 13][:, None, None]) >> 8, 0, 255), v)
    out = v.astype(np.uint8)
    return out[0] if single else out


def apply_stack(frames, params):
    """frames u8 [n, K, H, W] (a player_frame stack per env), params [n, 14]: every frame of env i under params[i]."""
    f = np.asarray(frames)
    n, K = f.shape[:2]
    return apply(f.reshape((n * K,) + f.shape[2:]), np.repeat(np.asarray(params), K, axis=0)).reshape(f.shape)
