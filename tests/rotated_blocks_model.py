"""numpy model of the binary quantizer's block-rotated rows (the reference has no counterpart).

The rotation of rotated_model.py without the pad: the hashed signs of i < dim (rotated_model.sign_bits), then the butterfly
stages s = 1, 2, 4, ..., B / 2 with one f32 numpy operation per add, B the largest power of two that divides dim.  No pair
leaves its B-aligned block, so this is dim / B Hadamard transforms of size B side by side.  No code shared with the
library.  What follows the rotation is the model of a plain store of dim dimensions: two_bit_model and
two_bit_scalar_model take y, rotated_model.one_bit_rows its signs.
"""
import numpy as np

from rotated_model import sign_bits

f32 = np.float32
u32 = np.uint32
MAX_DIM = 16384
MIN_BLOCK = 64  # dim is a multiple of it
BLOCKS = 16  # the flag on a qamd_bin_encoding, legal only beside rotated_model.ROTATED
ONE_BIT_ROTATED_BLOCKS, TWO_BITS_ROTATED_BLOCKS = 20, 21


def block(dim):
    """B: the largest power of two that divides dim."""
    assert dim > 0
    return dim & -dim


def rotate(x, b=None):
    """[rows, dim] f32 -> [rows, dim] f32; `b` overrides B (a power of two that divides dim) for the tests of the model."""
    x = np.atleast_2d(np.asarray(x, dtype=f32))
    rows, dim = x.shape
    b = block(dim) if b is None else b
    assert dim % b == 0 and b & (b - 1) == 0
    y = (np.ascontiguousarray(x).view(u32) ^ (sign_bits(dim) << u32(31))).view(f32)  # the sign bit flipped: exact
    s = 1
    with np.errstate(all="ignore"):
        while s < b:
            v = y.reshape(rows, dim // (2 * s), 2, s)  # [.., 0, :] are the j with (j & s) == 0, [.., 1, :] their j + s
            lo, hi = v[:, :, 0, :], v[:, :, 1, :]
            y = np.stack([(lo + hi).astype(f32), (lo - hi).astype(f32)], axis=2).reshape(rows, dim)
            s *= 2
    return y
