"""numpy model of weighted 4- / 8-bit scalar queries against two-bit rows (the reference has no
counterpart), read dimension by dimension: no bit planes and no popcounts in the oracle itself.  Integers are int64; the
only f32 steps are the ones the specification names, one numpy operation each.  No code shared with the library, and none
with the one-bit oracle of util.py: tests/test_binary_two_bit_scalar_model.py checks the two against each other.
"""
import numpy as np

import two_bit_model as m

f32 = np.float32


def weights(query, lo, hi):
    """w_i = q_i * h_i with h_i = hi_i - lo_i, h_i = 0 where that is not finite, and a NaN product as 0.0f."""
    q = np.asarray(query, dtype=f32).ravel()
    with np.errstate(all="ignore"):
        h = (np.asarray(hi, dtype=f32) - np.asarray(lo, dtype=f32)).astype(f32)
        h = np.where(np.isfinite(h), h, f32(0.0)).astype(f32)
        w = (q * h).astype(f32)
    return np.where(np.isnan(w), f32(0.0), w).astype(f32)


def codes_of(w, bits):
    """(codes uint32[dim], a f32) of the values w: a = max |w_i| over the finite w_i (0 without one); a == 0 -> every code
    (L + 1) / 2; else scale = (float)L / (a + a), t_i = (w_i + a) * scale, c_i = min(L, (uint32)(t_i + 0.5f)), a NaN w_i
    taken as 0.0f; last +inf -> L and -inf -> 0."""
    w = np.asarray(w, dtype=f32).ravel()
    L = (1 << bits) - 1
    fin = np.isfinite(w)
    a = f32(np.abs(w[fin]).max()) if fin.any() else f32(0.0)
    c = np.full(w.size, (L + 1) // 2, dtype=np.uint32)
    if a != 0:
        scale = f32(f32(L) / f32(a + a))
        v = np.where(fin, w, f32(0.0)).astype(f32)
        t = ((v + a).astype(f32) * scale).astype(f32)
        c[:] = np.minimum(L, np.trunc((t + f32(0.5)).astype(f32)).astype(np.int64))
    c[np.isposinf(w)] = L
    c[np.isneginf(w)] = 0
    return c, a


def weighted_codes(query, lo, hi, bits):
    """(codes uint32[dim], a f32) of a weighted `bits`-bit query."""
    return codes_of(weights(query, lo, hi), bits)


def xor_from_levels(levels, codes, bits):
    """int64 X of rows given as levels [n, dim] in {0, 1, 2}: per dimension level 0 adds 2 c_i, level 1 adds L and level 2
    adds 2 (L - c_i).  codes [dim] -> X [n]; codes [queries, dim] -> X [queries, n].  The sums run in float64, where every
    term and partial sum is an integer below 2^53: exact in any order."""
    L = (1 << bits) - 1
    c = np.asarray(codes, dtype=np.int64)
    lv = np.asarray(levels)
    table = (2 * c, np.full_like(c, L), 2 * (L - c))
    x = 0
    for l in range(3):
        x = x + table[l].astype(np.float64) @ (lv == l).astype(np.float64).T
    return np.asarray(x).astype(np.int64)


def metric(x, dim, bits, dist, invert):
    """calculate_metric on X with code_bits * L = 2 dim L in place of dim, in f32; dist: 0 is Dot."""
    dim_l = 2 * dim * ((1 << bits) - 1)
    assert dim_l < 1 << 24, "past this the f32 steps below would round"
    xor = np.asarray(x).astype(f32)
    zeros = (f32(dim_l) - xor).astype(f32)
    return ((zeros - xor) if (int(dist) == m.DOT) != bool(invert) else (xor - zeros)).astype(f32)


def scores(levels, codes, dim, bits, dist, invert):
    return metric(xor_from_levels(levels, codes, bits), dim, bits, dist, invert)


def planes(codes, dim, bits, store):
    """uint8[bits, row_bytes(2 dim)]: the stored form - bit b of c_i at bit i AND bit dim + i of plane b, byte j // 8, bit
    j % 8, pad bits zero."""
    c = np.asarray(codes, dtype=np.uint32)
    nb = m.row_bytes(2 * dim, store)
    out = np.zeros((bits, nb * 8), dtype=np.uint8)
    for b in range(bits):
        bit = ((c >> b) & 1).astype(np.uint8)
        out[b, :dim] = bit
        out[b, dim:2 * dim] = bit
    return np.packbits(out, axis=1, bitorder="little")


def xor_from_planes(rows, query_planes):
    """int64[n]: sum_b 2^b popcount(plane_b xor row) over stored rows [n, nb] - the restatement the kernels compute."""
    x = np.zeros(rows.shape[0], dtype=np.int64)
    for b in range(query_planes.shape[0]):
        x += m.xor_count(rows, query_planes[b]) << b
    return x

