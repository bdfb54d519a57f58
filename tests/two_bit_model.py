"""numpy model of the binary quantizer's two-bit rows (the reference has no counterpart).

Statistics, thresholds, rows and scores exactly as the specification orders them, with no code shared with the library:
the tests compare raw bits against these functions.
"""
import numpy as np

BLOCK = 4096
DOT, L1, L2 = 0, 1, 2
U8, U128 = 0, 1


def stats(data):
    """(n u64, S f64, Q f64) per column of a [rows, dim] f32 array: per block of 4096 rows a sequential f64 sum from +0.0
    over the finite entries (np.cumsum adds in index order, nothing pairwise), then a sequential fold over the blocks."""
    data = np.asarray(data, dtype=np.float32)
    rows, dim = data.shape
    n = np.zeros(dim, dtype=np.uint64)
    s = np.zeros(dim, dtype=np.float64)
    q = np.zeros(dim, dtype=np.float64)
    zero = np.zeros((1, dim), dtype=np.float64)
    with np.errstate(all="ignore"):
        for r0 in range(0, rows, BLOCK):
            blk = data[r0:r0 + BLOCK]
            fin = np.isfinite(blk)
            x = np.where(fin, blk, np.float32(0.0)).astype(np.float64)  # + 0.0 leaves a sum that began at +0.0 as it is
            bs = np.cumsum(np.concatenate([zero, x]), axis=0)[-1]
            bq = np.cumsum(np.concatenate([zero, x * x]), axis=0)[-1]
            s = s + bs
            q = q + bq
            n = n + fin.sum(axis=0).astype(np.uint64)
    return n, s, q


def thresholds(n, s, q, t=0.43):
    """(lo, hi) f32: single f64 operations in the specification's order."""
    n = np.asarray(n, dtype=np.uint64)
    s = np.asarray(s, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    t = np.float64(t)
    with np.errstate(all="ignore"):
        cnt = np.where(n == 0, np.float64(1.0), n.astype(np.float64))
        mean = np.where(n == 0, np.float64(0.0), s / cnt)
        var = np.where(n == 0, np.float64(0.0), q / cnt - mean * mean)
        var = np.where(var > 0, var, np.float64(0.0))
        sd = np.sqrt(var)
        w = t * sd
        return (mean - w).astype(np.float32), (mean + w).astype(np.float32)


def row_bytes(bits, store):
    """get_storage_size * size_of of a row of `bits` bits (encoded_vectors_binary.rs:99-116, :152-159)."""
    if store == U128:
        return (bits // 128 + (bits % 128 != 0)) * 16
    unit = 16 if bits > 128 else 8 if bits > 64 else 4 if bits > 32 else 1
    return (bits // (8 * unit) + (bits % (8 * unit) != 0)) * unit


def levels(x, lo, hi):
    """0, 1 or 2 per entry: how many of the two strict f32 compares hold."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (x > lo).astype(np.int64) + (x > hi).astype(np.int64)


def encode(x, lo, hi, store):
    """[rows, row_bytes(2 dim)] u8: bit i = x_i > lo_i, bit dim + i = x_i > hi_i, byte j // 8, bit j % 8, pads zero."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float32))
    rows, dim = x.shape
    with np.errstate(invalid="ignore"):
        bits = np.concatenate([x > np.asarray(lo, np.float32), x > np.asarray(hi, np.float32)], axis=1)
    nb = row_bytes(2 * dim, store)
    out = np.zeros((rows, nb * 8), dtype=np.uint8)
    out[:, :2 * dim] = bits
    return np.packbits(out, axis=1, bitorder="little")


def xor_count(rows, qrow):
    return np.unpackbits(np.bitwise_xor(rows, qrow), axis=-1).sum(axis=-1).astype(np.int64)


def metric(xor, dim, dist, invert):
    """calculate_metric (:237-252) with code_bits = 2 dim in place of dim; f32."""
    xor = np.asarray(xor).astype(np.float32)
    zeros = np.float32(2 * dim) - xor
    return (zeros - xor if (dist == DOT) != bool(invert) else xor - zeros).astype(np.float32)


def score_all(rows, qrow, dim, dist, invert):
    return metric(xor_count(rows, qrow), dim, dist, invert)
