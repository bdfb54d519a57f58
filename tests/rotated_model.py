"""numpy model of the binary quantizer's rotated rows (the reference has no counterpart).

The randomized Hadamard rotation exactly as the specification orders it - the pad, the hashed signs in u32 arithmetic, the
butterfly stages s = 1, 2, 4, ... with one f32 numpy operation per add - with no code shared with the library.  What
follows the rotation is the model of a plain store of P dimensions: two_bit_model and two_bit_scalar_model take y.
"""
import numpy as np

f32 = np.float32
u32 = np.uint32
MAX_DIM = 16384
ROTATED = 4  # the flag on a qamd_bin_encoding


def padded_dim(dim):
    """P: the smallest power of two >= dim, 1 for dim = 1."""
    p = 1
    while p < dim:
        p <<= 1
    return p


def sign_bits(p):
    """uint32[p]: 1 where y_i is negated - the low bit of the hash of i, every step in u32 arithmetic."""
    with np.errstate(over="ignore"):
        h = np.arange(p, dtype=u32) * u32(0x9E3779B1)
        h ^= h >> u32(16)
        h *= u32(0x85EBCA6B)
        h ^= h >> u32(13)
        h *= u32(0xC2B2AE35)
        h ^= h >> u32(16)
    return h & u32(1)


def rotate(x):
    """[rows, dim] f32 -> [rows, P] f32."""
    x = np.atleast_2d(np.asarray(x, dtype=f32))
    rows, dim = x.shape
    p = padded_dim(dim)
    y = np.zeros((rows, p), dtype=f32)  # +0.0f
    y[:, :dim] = x
    y = (y.view(u32) ^ (sign_bits(p) << u32(31))).view(f32)  # the sign bit flipped: exact, NaN payloads and all
    s = 1
    with np.errstate(all="ignore"):
        while s < p:
            v = y.reshape(rows, p // (2 * s), 2, s)  # [.., 0, :] are the j with (j & s) == 0, [.., 1, :] their j + s
            a, b = v[:, :, 0, :], v[:, :, 1, :]
            y = np.stack([(a + b).astype(f32), (a - b).astype(f32)], axis=2).reshape(rows, p)
            s *= 2
    return y


def one_bit_rows(y, nb):
    """[rows, nb] u8 of rotated values y [rows, P]: bit i = y_i > 0, byte i // 8, bit i % 8, pads zero."""
    y = np.atleast_2d(y)
    out = np.zeros((y.shape[0], nb * 8), dtype=np.uint8)
    with np.errstate(invalid="ignore"):
        out[:, :y.shape[1]] = y > f32(0.0)
    return np.packbits(out, axis=1, bitorder="little")
