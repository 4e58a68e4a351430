"""Python model of the action-route rule (nclone_amd/csrc/npp_route.hpp; include/npp_amd.h npp_set_routes), written
from the rule's text, not from the C++: one env's header (16 ints) and its two buffers, and the events that change them.  The CPU
tests hold npp_route_apply_host against it, the GPU tests hold the device against it."""
import numpy as np

LEN, BITS, FS, FRAMES, FLAGS, LEVEL = range(6)
FINISHED, CUR = 6, 12
OVERFLOW, BROKEN = 1, 2
END = 1 | 2 | 8   # won | dead | truncated
EMPTY = [0, 0, 0, 0, 0, -1]


class Route:
    """One env: .hdr list of 16 ints, .buf uint8 [2, cap]."""

    def __init__(self, cap, autoreset):
        assert cap > 0 and cap % 16 == 0
        self.cap, self.autoreset = cap, bool(autoreset)
        self.hdr = EMPTY + EMPTY + [0, 0, 0, 0]
        self.buf = np.zeros((2, cap), dtype=np.uint8)

    def empty(self):
        return self.hdr[LEN] == 0 and self.hdr[BITS] == 0

    def flip(self):
        if self.empty():
            return
        self.hdr[FINISHED:FINISHED + 6] = self.hdr[0:6]
        self.hdr[CUR] ^= 1
        self.hdr[0:6] = EMPTY

    def step(self, a, f, x, fs, level):
        h = self.hdr
        if x > 0:
            if self.empty():
                h[FS], h[LEVEL] = fs, level
            elif h[FS] != fs:
                h[BITS] |= BROKEN
            if h[LEN] < self.cap:
                self.buf[h[CUR], h[LEN]] = a
                h[LEN] += 1
            else:
                h[BITS] |= OVERFLOW
            h[FRAMES] += x
            h[FLAGS] = f
        if self.autoreset and (f & END):
            self.flip()

    def reset(self):
        self.flip()

    def tick(self):
        self.hdr[BITS] |= BROKEN

    def restore(self, src_hdr, src_bytes):
        self.hdr[0:6] = [int(v) for v in src_hdr[:6]]
        n = int(src_hdr[LEN])
        self.buf[self.hdr[CUR], :n] = np.asarray(src_bytes[:n], dtype=np.uint8)

    # views
    def current(self):
        return self.buf[self.hdr[CUR], :self.hdr[LEN]].copy()

    def finished(self):
        return self.buf[1 - self.hdr[CUR], :self.hdr[FINISHED + LEN]].copy()


def apply_events(route, events, restore_bytes=None):
    """events: rows of 8 ints as npp_route_apply_host takes them."""
    for ev in events:
        kind = int(ev[0])
        if kind == 0:
            route.step(int(ev[1]), int(ev[2]), int(ev[3]), int(ev[4]), int(ev[5]))
        elif kind == 1:
            route.reset()
        elif kind == 2:
            route.tick()
        elif kind == 3:
            off = int(ev[7])
            route.restore(ev[1:7], restore_bytes[off:off + int(ev[1])])
        else:
            raise ValueError(kind)


def random_events(rng, cap, n, restore_pool):
    """A seeded event list with everything the rule distinguishes: steps with x == 0, episode ends, resets (of empty routes too, by
    repetition), a frame_skip change, ticks and restores.  restore_pool: uint8 bytes the restore events index into."""
    ev = np.zeros((n, 8), dtype=np.int32)
    fs = 4
    for i in range(n):
        r = rng.random()
        if r < 0.78:
            end = rng.random() < 0.08
            f = int(rng.choice([1, 2, 8, 2 | 16, 2 | 32])) if end else 0
            f |= 4 if rng.random() < 0.3 else 0
            if rng.random() < 0.03:
                fs = int(rng.choice([1, 2, 4]))
            x = 0 if rng.random() < 0.1 else int(rng.integers(1, fs + 1))
            ev[i, :6] = [0, rng.integers(0, 6), f, x, fs, rng.integers(0, 3)]
        elif r < 0.88:
            ev[i, 0] = 1   # (two in a row, or one after an auto-reset flip: a reset of an empty route)
        elif r < 0.92:
            ev[i, 0] = 2
        else:
            ln = int(rng.integers(0, cap + 1))
            off = int(rng.integers(0, len(restore_pool) - cap))
            ev[i] = [3, ln, int(rng.choice([0, 0, 1, 2, 3])), 4, 4 * ln, int(rng.choice([0, 1, 2, 8])), rng.integers(0, 3), off]
    return ev
