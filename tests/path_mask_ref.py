"""The mask stage of path-direction action masking (ninja.py:766-800) in ten lines: which actions survive a direction.
Test infrastructure, independent of npp_pathmask.hpp; checked against the reference-made tests/golden/pathmask.npz."""
import numpy as np

NONE, LEFT, RIGHT, DOWN = 0, 1, 2, 3
# actions: 0 NOOP, 1 LEFT, 2 RIGHT, 3 JUMP, 4 JUMP+LEFT, 5 JUMP+RIGHT; bit a of a keep-mask = action a stays valid
KEEP = np.array([0b111111,    # none: nothing removed
                 0b000011,    # left keeps NOOP and LEFT
                 0b000101,    # right keeps NOOP and RIGHT
                 0b000111],   # down removes the three jump actions
                dtype=np.uint8)


def hard_mask_bits(inert_bits, direction):
    """bits of the hard mask from the bits of the inert mask and the direction (arrays or scalars)"""
    return np.asarray(inert_bits, dtype=np.uint8) & KEEP[np.asarray(direction, dtype=np.int64)]


def mask_bits(mask):
    """i8 [..., 6] mask -> u8 [...] bits"""
    return (np.asarray(mask).astype(np.uint8) << np.arange(6, dtype=np.uint8)).sum(axis=-1).astype(np.uint8)
