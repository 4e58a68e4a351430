"""The bit layout of the five packed per-env state words (csrc/npp_state.hpp; DESIGN.md section 3, "packed state layout"), pinned on
the CPU: npp_state_decode_host runs npp_dump_state's own decode of one env's words, and the expected columns are restated here in
numpy from the layout table, column by column -- never taken from the library."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, B, C_, D, E = range(5)
# name: (word, first bit, width) -- the table of DESIGN.md section 3, restated by hand: the layout the library had before
# npp_state.hpp existed, which that header must keep
FIELDS = {
    "state": (A, 0, 4), "airborn": (A, 4, 1), "airborn_old": (A, 5, 1), "walled": (A, 6, 1), "wn+1": (A, 7, 2), "jio": (A, 9, 1),
    "hor+1": (A, 10, 2), "jump": (A, 12, 1), "gjump": (A, 13, 1), "dslow": (A, 14, 1), "jbuf+1": (A, 15, 3), "fbuf+1": (A, 18, 3),
    "wbuf+1": (A, 21, 3), "lbuf+1": (A, 24, 3), "cause": (A, 27, 2), "timpact": (A, 29, 1),
    "jdur": (B, 0, 6), "fcount": (B, 6, 8), "ccount": (B, 14, 8), "pstate": (B, 22, 4),
    "fair": (C_, 0, 16), "scf": (C_, 16, 16),
    "frame": (D, 0, 16), "gold": (D, 16, 8), "doors": (D, 24, 8),
    "pcell": (E, 0, 16), "scvalid": (E, 16, 1), "fast_ordered": (E, 17, 1), "fresh": (E, 18, 1), "episode": (E, 19, 13),
}


def _inputs():
    rows = [np.zeros(5, dtype=np.uint32), np.full(5, 0xFFFFFFFF, dtype=np.uint32)]
    for word, shift, width in FIELDS.values():   # each field alone at its maximum
        r = np.zeros(5, dtype=np.uint32)
        r[word] = ((1 << width) - 1) << shift
        rows.append(r)
    rnd = np.random.default_rng(20260).integers(0, 1 << 32, size=(10000, 5), dtype=np.uint64).astype(np.uint32)
    return np.ascontiguousarray(np.concatenate([np.stack(rows), rnd]))


def _field(W, name):
    word, shift, width = FIELDS[name]
    return ((W[:, word].astype(np.int64) >> shift) & ((1 << width) - 1)).astype(np.int64)


def _expected(W):
    """npp_dump_state's i32 row ("state dump layout"): columns 3-7 are the stored, biased values; 11 and 12 are "gravity is
    FALL" / "drag is REGULAR"; 13 and 27 (exit switch, level) are not in the words: the host entry reports 2 and 0; 28-31 are zero."""
    o = np.zeros((len(W), 32), dtype=np.int64)
    o[:, 0] = _field(W, "state")
    o[:, 1] = _field(W, "airborn")
    o[:, 2] = _field(W, "walled")
    o[:, 3] = _field(W, "wn+1")
    o[:, 4] = _field(W, "jbuf+1")
    o[:, 5] = _field(W, "fbuf+1")
    o[:, 6] = _field(W, "wbuf+1")
    o[:, 7] = _field(W, "lbuf+1")
    o[:, 8] = _field(W, "fcount")
    o[:, 9] = _field(W, "ccount")
    o[:, 10] = _field(W, "jdur")
    o[:, 11] = 1 - _field(W, "gjump")
    o[:, 12] = 1 - _field(W, "dslow")
    o[:, 13] = 2
    o[:, 14] = _field(W, "gold")
    o[:, 15] = _field(W, "doors")
    o[:, 16] = _field(W, "fair")
    o[:, 17] = _field(W, "scf")
    o[:, 18] = _field(W, "airborn_old")
    o[:, 19] = _field(W, "jio")
    o[:, 20] = _field(W, "cause")
    o[:, 21] = _field(W, "timpact")
    o[:, 22] = _field(W, "frame")
    o[:, 23] = _field(W, "hor+1") - 1
    o[:, 24] = _field(W, "jump")
    o[:, 25] = _field(W, "pstate")
    o[:, 26] = _field(W, "pcell")
    o[:, 27] = 0
    return o


def test_table_covers_every_bit_once():
    """The restatement itself: per word the fields are disjoint; A leaves bits 30-31 free, B bits 26-31, C, D and E none."""
    used = [0] * 5
    for word, shift, width in FIELDS.values():
        m = ((1 << width) - 1) << shift
        assert used[word] & m == 0 and m < (1 << 32)
        used[word] |= m
    assert used == [(1 << 30) - 1, (1 << 26) - 1, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF]


def test_decode_matches_the_layout_table():
    from nclone_amd import _native as nat
    from nclone_amd import build_native

    build_native.build()
    lib = nat.lib()
    assert nat.DUMP_I32 == 32
    hdr = open(os.path.join(ROOT, "include", "npp_amd.h")).read()
    assert "int npp_state_decode_host(const uint32_t words[5], int32_t *out /* NPP_DUMP_I32 */);" in hdr
    W = _inputs()
    got = np.full((len(W), 32), -7, dtype=np.int32)
    base_w, base_o, decode = W.ctypes.data, got.ctypes.data, lib.npp_state_decode_host
    for i in range(len(W)):
        assert decode(base_w + 20 * i, base_o + 128 * i) == nat.NPP_OK
    want = _expected(W)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (bad[:5], got[bad[0][0]], want[bad[0][0]])
    assert lib.npp_state_decode_host(None, None) == nat.NPP_ERR_INVALID

    # the minimal observation's encoder reads word A through the same definitions: it must agree with the decode on state, airborn,
    # walled, wall normal and the four buffers
    n = len(W)
    a = np.ascontiguousarray(W[:, 0])
    planes = np.zeros((n, 4), dtype=np.float64)
    obs = np.full((n, 40), 7.0, dtype=np.float32)
    assert lib.npp_minimal_encode_host(a.ctypes.data, planes.ctypes.data, n, obs.ctypes.data) == nat.NPP_OK
    g = got.astype(np.int64)
    onehot = np.zeros((n, 5), dtype=np.float32)
    onehot[np.arange(n), np.minimum(g[:, 0], 4)] = 1.0
    assert np.array_equal(obs[:, 2:7], onehot)
    assert np.array_equal(obs[:, 7], np.where(g[:, 1] == 1, 1.0, -1.0).astype(np.float32))
    assert np.array_equal(obs[:, 8], np.where(g[:, 2] == 1, 1.0, -1.0).astype(np.float32))
    assert np.array_equal(obs[:, 9], np.where(g[:, 2] == 1, g[:, 3] - 1.0, 0.0).astype(np.float32))
    for col, src, span in ((36, 4, 5.0), (37, 5, 5.0), (38, 6, 5.0), (39, 7, 4.0)):
        buf = g[:, src] - 1.0
        assert np.array_equal(obs[:, col], np.where(buf >= 0, buf / span, -1.0).astype(np.float32)), col
