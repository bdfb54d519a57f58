"""Weighted scalar queries against two-bit rows without a GPU: the per-dimension oracle against a
restatement on bit planes and against the one-bit oracle of util.py, the recall the design rests on (a numpy model on
synthetic data; nothing here says anything about real embeddings), and the entry points' declaration and export."""
import numpy as np
import pytest

import two_bit_model as m
import two_bit_scalar_model as w
import util

from quantization_amd import _lib


def test_header_declares_and_library_exports_the_entry_points():
    new = ["qamd_bin_encode_query_scalar_w", "qamd_bin_encode_query_batch_scalar_w"]
    declared = set(_lib.declared_symbols())
    L = _lib.lib()
    assert not [s for s in new if s not in declared or not hasattr(L, s)]


def _case(dim, seed):
    rng = np.random.default_rng(seed)
    lo = rng.normal(size=dim).astype(np.float32)
    hi = (lo + rng.random(dim).astype(np.float32) * rng.uniform(0.1, 3.0, size=dim).astype(np.float32)).astype(np.float32)
    hi = np.maximum(lo, hi)
    lo[::7], hi[::7] = hi[::7].copy(), hi[::7].copy()  # lo == hi: weight 0
    if dim > 4:
        lo[4], hi[4] = -np.inf, np.inf  # not finite: weight 0
    x = rng.normal(size=(50, dim)).astype(np.float32) * 2
    q = rng.normal(size=dim).astype(np.float32)
    return lo, hi, x, q


@pytest.mark.parametrize("bits", [4, 8])
@pytest.mark.parametrize("dim", [1, 20, 33, 64, 100])
def test_oracle_against_the_planes(dim, bits):
    lo, hi, x, q = _case(dim, dim + bits)
    L = (1 << bits) - 1
    for k, query in enumerate([q, np.zeros(dim, np.float32), np.abs(q), -np.abs(q)]):
        query = query.copy()
        if k == 0 and dim > 2:
            query[0], query[1], query[-1] = np.nan, np.inf, -np.inf
        codes, a = w.weighted_codes(query, lo, hi, bits)
        ucodes, ua = util.scalar_codes(w.weights(query, lo, hi), bits)  # 3.2d on w: the one-bit oracle agrees
        assert np.array_equal(codes, ucodes) and np.float32(a).view(np.uint32) == np.float32(ua).view(np.uint32)
        assert codes.max() <= L
        for store in (m.U8, m.U128):
            rows = m.encode(x, lo, hi, store)
            pl = w.planes(codes, dim, bits, store)
            assert pl.shape == (bits, m.row_bytes(2 * dim, store))
            assert not np.unpackbits(pl, axis=1, bitorder="little")[:, 2 * dim:].any()
            want = w.xor_from_levels(m.levels(x, lo, hi), codes, bits)
            assert np.array_equal(w.xor_from_planes(rows, pl), want)
            # and the one-bit oracle on a query of 2 dim codes against the same bytes
            assert np.array_equal(util.scalar_xor(rows, np.concatenate([codes, codes]), 2 * dim, bits), want)
        if k == 1:
            assert a == 0 and (codes == (L + 1) // 2).all()


def test_special_weights():
    f = np.float32
    lo = f([0.0, 1.0, -np.inf, -np.inf, 0.0, 0.0, 0.0])
    hi = f([1.0, 1.0, np.inf, 0.0, 2.0, 3e38, 1.0])
    q = f([np.nan, 5.0, 1.0, 1.0, np.inf, 3e38, -0.0])
    wv = w.weights(q, lo, hi)
    #        NaN q  lo==hi  inf-(-inf)  inf h  inf q  overflow  -0
    assert np.array_equal(wv.view(np.uint32), f([0.0, 0.0, 0.0, 0.0, np.inf, np.inf, -0.0]).view(np.uint32))
    codes, a = w.weighted_codes(q, lo, hi, 8)
    assert a == 0 and list(codes) == [128, 128, 128, 128, 255, 255, 128]
    # inf * 0 is NaN and counts as 0
    assert w.weights(f([np.inf]), f([1.0]), f([1.0]))[0] == 0


def _recall(seed, n=4000, dim=256, n_queries=100, k=10):
    """The recipe of tests/test_binary_two_bit_model.py::_recall; recall@10 against the exact dot-product top-10, stable
    sorts on both sides, of: the two-bit store's own query, 8-bit scalar queries against one-bit rows, unweighted 8-bit
    codes (w = q) against two-bit rows, and the weighted 8- and 4-bit queries."""
    rng = np.random.default_rng(seed)
    scale = rng.uniform(0.3, 1.5, size=dim)
    data = (rng.normal(size=(n, dim)) * scale).astype(np.float32)
    picks = rng.integers(0, n, size=n_queries)
    queries = (data[picks] + 0.5 * rng.normal(size=(n_queries, dim))).astype(np.float32)
    data /= np.linalg.norm(data, axis=1, keepdims=True)
    queries /= np.linalg.norm(queries, axis=1, keepdims=True)
    exact = np.argsort(-(queries.astype(np.float64) @ data.astype(np.float64).T), axis=1, kind="stable")[:, :k]
    lo, hi = m.thresholds(*m.stats(data), 0.43)
    lv = m.levels(data, lo, hi)
    sign = 2 * (data > 0).astype(np.int64) - 1
    two_rows, two_q = m.encode(data, lo, hi, m.U8), m.encode(queries, lo, hi, m.U8)
    hits = dict.fromkeys(("two", "one8", "plain8", "w8", "w4"), 0)
    for qi in range(n_queries):
        q = queries[qi]
        c8, _ = util.scalar_codes(q, 8)
        x = {
            "two": m.xor_count(two_rows, two_q[qi]),
            "one8": (dim * 255 - sign @ (2 * c8.astype(np.int64) - 255)) // 2,
            "plain8": w.xor_from_levels(lv, c8, 8),
            "w8": w.xor_from_levels(lv, w.weighted_codes(q, lo, hi, 8)[0], 8),
            "w4": w.xor_from_levels(lv, w.weighted_codes(q, lo, hi, 4)[0], 4),
        }
        for name, xs in x.items():
            got = np.argsort(xs, kind="stable")[:k]
            hits[name] += len(set(got.tolist()) & set(exact[qi].tolist()))
    return {name: h / (n_queries * k) for name, h in hits.items()}


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_weighted_queries_recall_more(seed):
    r = _recall(seed)
    print(f"seed {seed}: recall@10 two-bit query {r['two']:.3f}, one bit + 8-bit scalar {r['one8']:.3f}, two bits + "
          f"unweighted 8-bit {r['plain8']:.3f}, two bits + weighted 8-bit {r['w8']:.3f}, weighted 4-bit {r['w4']:.3f}")
    assert r["w8"] > r["two"]
    assert r["w8"] > r["one8"]
    assert r["w8"] > r["plain8"]
