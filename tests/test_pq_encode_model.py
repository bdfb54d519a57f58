"""The inputs tests/test_gpu_pq_encode_edges.py feeds the PQ assignment kernels, checked against the oracle alone (no GPU).

The encoder's parity claim is that `pq_encode_kernel` and `pq_encode_cs_kernel<CS>` (csrc/pq.hip) walk the 256 centroids
in index order with the reference's strict '<' on a sequential, uncontracted f32 sum (encode_vector,
encoded_vectors_pq.rs:237-265).  Random data cannot tell: its nearest centroid is unique by a wide margin.  This file proves
that the generators in tests/util.py produce rows on which each of those properties DECIDES the code - so a kernel that
contracts `d += t * t`, sums in another order, uses '<=' or visits a pair's halves in the wrong order gives other bytes:

  * `pq_near_tie_case`: per tested chunk length >= 2 at least 100 cells whose code changes under the contracted chain
    d = f32(f64(t) * f64(t) + f64(d)), at least 100 whose code changes under the reversed sum, and at least 100 exact f32
    ties (length 1: ties only - fma(t, t, 0) is t * t; length 2: no sum order to be sensitive to - a two-term f32 sum
    commutes - so there the reversed sum must change nothing);
  * `pq_special_case`: NaN, infinities, overflowing differences, subnormals and -0.0, with the codes stated literally;
  * the oracle itself stays within the f64 bound of a sequential f32 sum of squares, and never picks the higher index of
    two identical centroids.
"""
import numpy as np
import pytest

import util
from util import PQ_SPECIAL_ROWS, PQ_TIE_SLOTS, pq_near_tie_case, pq_near_tie_table, pq_special_case, pq_sq_dist

LENGTHS = (1, 2, 3, 4, 7, 8, 10, 16, 20, 24, 32, 33)  # every chunk length test_gpu_pq_encode_edges.py encodes


@pytest.fixture(scope="module", params=LENGTHS)
def tie_case(request):
    return pq_near_tie_case(request.param, 1000, seed=11)


def test_near_tie_rows_are_decided_by_contraction_order_and_strict_less(tie_case, qo):
    case = tie_case
    m, length = case.m, case.length
    codes = qo.pq_encode(case.data, length, case.cen)
    # the oracle walks the plain chain: numpy's restatement of it gives the same codes, and they are the slot's own two
    assert np.array_equal(codes, case.want)
    at = np.arange(m)[None, :]
    assert np.all((codes == case.lo[at, case.slot]) | (codes == case.hi[at, case.slot])), "another slot's centroid was nearer"
    used = np.zeros((m, PQ_TIE_SLOTS), dtype=bool)
    used[at, case.slot] = True
    n_contract, n_order, n_tie = (int((f & used).sum()) for f in (case.contract, case.order, case.tie))
    print(f"length {length}: {int(used.sum())} cells, contraction-sensitive {n_contract}, order-sensitive {n_order}, "
          f"exact ties {n_tie}")
    assert n_tie >= 100
    if length >= 2:
        assert n_contract >= 100
    else:
        assert n_contract == 0  # fma(t, t, 0) is t * t
    if length >= 3:
        assert n_order >= 100
        # cells that either index wins outright, next to the exact ties (the lower index wins)
        decided = used & ~case.tie
        assert (decided & (case.d_hi < case.d_lo)).sum() >= 50 and (decided & (case.d_lo < case.d_hi)).sum() >= 50
    else:
        assert n_order == 0  # f32 addition commutes: (0 + x) + y and (0 + y) + x are the same two roundings
    assert (case.tie & used)[0::2].sum() >= 30, "ties inside one centroid pair (2p, 2p + 1)"
    if m > 1:
        assert (case.tie & used)[1::2].sum() >= 30, "ties across two pairs (2p + 1, 2p + 2)"


def test_near_tie_flags_mean_what_they_say(tie_case):
    """Recompute every cell's two distances from the finished arrays (not the generator's intermediates) under the three
    evaluation orders: `contract` / `order` / `tie` are exactly the cells where the code depends on it."""
    case = tie_case
    m, length = case.m, case.length
    for c in range(m):
        cols = slice(c * length, (c + 1) * length)
        rows = np.array([np.flatnonzero(case.slot[:, c] == s)[0] for s in range(PQ_TIE_SLOTS)])
        a = case.data[rows, cols]
        lo, hi = case.cen[case.lo[c], cols], case.cen[case.hi[c], cols]
        pick = {mode: pq_sq_dist(a, hi, mode) < pq_sq_dist(a, lo, mode) for mode in ("plain", "fma", "rev")}
        assert np.array_equal(pick["fma"] != pick["plain"], case.contract[c])
        assert np.array_equal(pick["rev"] != pick["plain"], case.order[c])
        assert np.array_equal(pq_sq_dist(a, lo) == pq_sq_dist(a, hi), case.tie[c])
        assert np.array_equal(util.bits(pq_sq_dist(a, lo)), util.bits(case.d_lo[c]))


def test_near_tie_positions_cover_the_packed_kernel():
    """Slots: both halves of a pair, across two pairs, every pipeline-step boundary of pq_encode_cs_kernel (U pairs per
    step, U = 16 / CS below CS = 16, else 1: the step boundary sits between indices 2 U st - 1 and 2 U st), 0 / 1 and
    254 / 255."""
    even = {util.pq_tie_slot_indices(0, s) for s in range(PQ_TIE_SLOTS)}
    odd = {util.pq_tie_slot_indices(1, s) for s in range(PQ_TIE_SLOTS)}
    assert (0, 1) in even and (254, 255) in even and all(hi == lo + 1 and lo % 2 == 0 for lo, hi in even)
    for cs in (1, 2, 4, 8, 16, 32):
        u = 1 if cs >= 16 else 16 // cs
        for st in range(1, 128 // u):
            assert (2 * u * st - 1, 2 * u * st) in odd
    for layout in (even, odd):
        assert sorted(i for pair in layout for i in pair) == list(range(256)), "every centroid index belongs to one slot"


@pytest.mark.parametrize("dim,chunk", [(10, 3), (100, 7), (50, 20), (24, 24), (33, 40), (131, 1), (392, 3), (6, 2), (7, 3)])
def test_near_tie_table_ragged_shapes(dim, chunk, qo):
    """The side-by-side table for (dim, chunk) with a ragged last chunk: the oracle's codes are the stated ones."""
    data, cen, cases = pq_near_tie_table(dim, chunk, 300, seed=5)
    codes = qo.pq_encode(data, chunk, cen)
    assert codes.shape == (300, qo.pq_chunks(dim, chunk))
    covered = 0
    for c0, case in cases:
        assert np.array_equal(codes[:, c0:c0 + case.m], case.want)
        covered += case.m
    assert covered == codes.shape[1]


@pytest.mark.parametrize("chunk,dim", util.PQ_EDGE_CS_SHAPES + util.PQ_EDGE_GENERIC_SHAPES)
def test_tables_the_gpu_file_encodes_hold_100_cells_of_each_kind(chunk, dim, qo):
    """The same conditions on the very tables tests/test_gpu_pq_encode_edges.py feeds the kernels (its shapes, seeds and
    row counts; three tables per shape), per distinct chunk length of the shape - the ragged last chunk, and shapes of
    one chunk, included: a single chunk has 128 cells per table, so each of the three tables leads with another kind."""
    tables = util.pq_edge_tie_tables(chunk, dim)
    assert [t[0].shape[0] for t in tables] == list(util.PQ_EDGE_ROW_COUNTS)
    counts = {}
    for data, cen, cases in tables:
        codes = qo.pq_encode(data, chunk, cen)
        for c0, case in cases:
            assert np.array_equal(codes[:, c0:c0 + case.m], case.want)
            used = np.zeros((case.m, PQ_TIE_SLOTS), dtype=bool)
            used[np.arange(case.m)[None, :], case.slot] = True
            got = counts.setdefault(case.length, np.zeros(3, dtype=np.int64))
            got += [int((f & used).sum()) for f in (case.contract, case.order, case.tie)]
    for length, (n_contract, n_order, n_tie) in counts.items():
        print(f"chunk {chunk} dim {dim} length {length}: contraction {n_contract}, order {n_order}, ties {n_tie}")
        assert n_tie >= 100
        assert n_contract >= 100 if length >= 2 else n_contract == 0
        assert n_order >= 100 if length >= 3 else n_order == 0


@pytest.mark.parametrize("chunk", [1, 4, 7, 8, 16, 20, 32])
def test_oracle_stays_inside_the_f64_bound(chunk, qo):
    """Independent of every f32 restatement: the f64 distance of the chosen centroid is at most
    min_f64 * (1 + 2 (len + 3) 2^-24).  Per side of the comparison: one rounding in t (relative 2^-24, twice in t^2),
    one in t * t, len - 1 in the sequential sum of non-negative terms - (len + 2) 2^-24 to first order, and the
    comparison has two sides; the bound is rounded up to len + 3 for the second-order terms.  Differences stay in the
    normal range (here 2^-60 <= |t| <= 2^60).  Centroid 100 = centroid 7 and 255 = 0: never chosen at the higher index."""
    rng = np.random.default_rng(chunk)
    n, dim = 600, 3 * chunk
    data = (rng.random((n, dim), dtype=np.float32) - 0.5).astype(np.float32)
    cen = (rng.random((256, dim), dtype=np.float32) - 0.5).astype(np.float32)
    cen[100], cen[255] = cen[7], cen[0]
    data[:40] = cen[rng.integers(0, 256, 40)] + rng.standard_normal((40, dim)).astype(np.float32) * np.float32(1e-3)
    data[40:48] = cen[[7, 0, 100, 255, 7, 0, 100, 255]]  # rows equal to a duplicated centroid
    codes = qo.pq_encode(data, chunk, cen)
    assert not np.any(codes == 100) and not np.any(codes == 255)
    assert np.any(codes == 7) and np.any(codes == 0)
    for c in range(3):
        cols = slice(c * chunk, (c + 1) * chunk)
        t = data[:, None, cols].astype(np.float64) - cen[None, :, cols].astype(np.float64)
        nz = np.abs(t[t != 0])
        assert nz.min() >= 2.0 ** -60 and nz.max() <= 2.0 ** 60
        d = (t * t).sum(axis=2)
        chosen = d[np.arange(n), codes[:, c]]
        assert np.all(chosen <= d.min(axis=1) * (1 + 2 * (chunk + 3) * 2.0 ** -24))


@pytest.mark.parametrize("dim,chunk", [(8, 1), (8, 2), (8, 4), (16, 8), (32, 16), (64, 32), (10, 3), (100, 7), (50, 20),
                                       (24, 24), (33, 40)])
def test_special_values_codes_are_the_stated_ones(dim, chunk, qo):
    """The rule, literally (PQ_SPECIAL_ROWS): a NaN distance is never '<' anything, a distance that overflows to +inf is
    not '< f32::MAX', subnormal differences are kept and their squares underflow to a tie at zero, exact ties go to the
    lower index."""
    data, cen, want = pq_special_case(dim, chunk)
    codes = qo.pq_encode(data, chunk, cen)
    names = ["nan_in_chunk_0"] + [name for name, _v, _c in PQ_SPECIAL_ROWS]
    for i, name in enumerate(names):
        assert codes[i].tolist() == want[i].tolist(), name
    assert codes[0, 0] == 0 and np.all(codes[0, 1:] == 1)
    # the literals once more, as numbers: one row per case
    by_name = dict(zip(names, codes[:, -1].tolist()))
    m = codes.shape[1]
    assert by_name == {"nan_in_chunk_0": 1 if m > 1 else 0, "one": 1, "plus_inf": 0, "minus_inf": 0, "big": 5,
                       "minus_big": 6, "overflow": 0, "subnormal": 0, "minus_subnormal": 0, "minus_zero": 0, "tiny": 11,
                       "last": 255, "midway": 0, "nearer_one": 1}
    # what makes them so, on the first chunk's columns
    cols = slice(0, min(chunk, dim))
    with np.errstate(all="ignore"):
        d = {name: pq_sq_dist(np.broadcast_to(data[i, cols], cen[:, cols].shape), cen[:, cols]) for i, name in enumerate(names)}
    assert np.all(np.isnan(d["nan_in_chunk_0"]))
    assert np.isnan(d["one"][2]) and d["one"][1] == 0
    assert np.all(np.isnan(d["plus_inf"]) | np.isposinf(d["plus_inf"])) and np.isnan(d["plus_inf"][3])
    assert np.all(np.isnan(d["overflow"]) | np.isposinf(d["overflow"]))
    assert d["big"][5] == 0 and np.isposinf(d["big"][6])
    assert all(d["subnormal"][k] == 0 for k in (0, 7, 8, 9, 10))
    one = pq_sq_dist(np.broadcast_to(data[names.index("tiny"), 1:2], (256, 1)), cen[:, 1:2]) if dim > 1 else d["tiny"]
    assert 0 < one[11] < one[0] < 1.1754944e-38 and one[0] == one[7], "squares of 1e-20 and 2e-20 are subnormal"
    assert 0 < d["tiny"][11] < d["tiny"][0] and d["tiny"][0] == d["tiny"][7]
    assert d["midway"][0] == d["midway"][1] == d["midway"][9]
    assert d["minus_zero"][0] == 0 and not np.signbit(d["minus_zero"][0])


def test_nan_aware_bit_comparison():
    a = np.array([1.0, -0.0, np.nan, np.inf], dtype=np.float32)
    other_nan = a.copy()
    other_nan.view(np.uint32)[2] ^= 0x80000001  # another sign and payload
    util.assert_bits_equal_nan(other_nan, a)
    for i, v in ((1, 0.0), (2, 1.0), (3, -np.inf), (0, np.nan)):
        b = a.copy()
        b[i] = v
        with pytest.raises(AssertionError):
            util.assert_bits_equal_nan(b, a)
