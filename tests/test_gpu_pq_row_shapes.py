"""The PQ scan, top-k, list and pair kernels on every row-length shape, bit for bit against the oracle.

csrc/pq.hip picks its kernels by m, the chunks (= code bytes) of a row: pq_scan_skew_kernel for whole, doubled and
padded ring rows and per slice of a planar image, pq_scan_fast_kernel<NVS> for everything else from 4096 rows on (one
slice up to 144 chunks, 128-byte-pitch slices beyond), pq_scan_kernel for small stores and id lists, pq_topk_small_kernel
for the single-launch top-k, pq_lists_kernel / pq_lists_staged_kernel<NP> for bursts of (query, id list) pairs,
pq_internal_pairs_kernel for stored-row pairs and pq_scan_seq_kernel<NVS> / pq_scan_seq_rows_kernel for a stored row
against the whole store.  tests/pq_row_shapes.py restates that dispatch and holds the case lists;
tests/test_pq_row_shapes_model.py (no GPU) asserts that the lists reach every instantiation and that, on these inputs, a
chunk read too many or too few changes nearly every score.

Stores come from from_storage over util.pq_shape_store: random codes, centroids in (-0.5, 0.5) with two all-zero ones, a
short last chunk, rows of all code 0, all 255 and all a zero centroid.  Expected values: qo.pq_encode_query +
qo.pq_score_all(order=ORDER_SSE) for encoded queries; for stored rows util.pq_seq_scores (one running f32 sum in chunk
order over util.pq_row_table), checked in every test against qo.pq_score_internal on a few pairs.  Everything is compared
on raw bits (assert_bits_equal; topk_want for ids and scores).

A fused top-k whose filter pass comes up short redoes the query exactly and would hide a FILTER kernel that loses rows,
so every FILTER case runs once more in a child process on the developer library with QAMD_DEBUG_TOPK=1, and every line
it prints must end "0 queries redone".  A second child runs with QAMD_PQ_SKEW=0, where rows of 16 .. 128 chunks take the
SIMPLE forms of pq_scan_fast_kernel that the product library never reaches.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import pq_row_shapes as M
from util import (DIST_IDS, assert_bits_equal, bits, pq_row_table, pq_seq_scores, pq_shape_queries, pq_shape_store,
                  topk_want)

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
torch = pytest.importorskip("torch")
from oracle import qoracle as qo  # noqa: E402

D = qa.DistanceType
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")
LARGEST = (True, False)


# ------------------------------------------------------------------ stores and what the oracle says of them
def open_store(rows, cen, dim, chunk, dist, inv):
    return qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(dim, rows.shape[0], D[dist], inv), chunk, cen)


def query_of(dim, seed=0):
    return pq_shape_queries(dim, 1, seed)[0]


_WANT = {}


def query_want(m, n, chunk, dist, inv, seed=0):
    """Scores of query_of(dim, seed) against the store (m, n, chunk), kept (a store of fewer rows is a prefix)."""
    key = ("q", m, n, chunk, dist, inv, seed)
    if key not in _WANT:
        rows, cen, dim, _ = pq_shape_store(m, n, chunk)
        lut = qo.pq_encode_query(query_of(dim, seed), chunk, cen, DIST_IDS[dist], inv)
        _WANT[key] = qo.pq_score_all(rows, lut, order=qo.ORDER_SSE)
    return _WANT[key]


def row_want(m, n, chunk, dist, inv, i):
    """score_internal(i, j) for every j of the store (m, n, chunk): the chunk-order restatement, first held against the
    oracle's own pair function on a few pairs."""
    key = ("r", m, n, chunk, dist, inv, i)
    if key not in _WANT:
        rows, cen, dim, _ = pq_shape_store(m, n, chunk)
        want = pq_seq_scores(rows, pq_row_table(rows, cen, dim, chunk, dist, i), inv)
        for j in (0, 1, 2, i, n - 1):
            assert bits(want[j:j + 1])[0] == bits(qo.pq_score_internal(rows, dim, chunk, cen, DIST_IDS[dist], inv, i, j))[0], \
                f"m {m} {dist} invert={inv}: the restatement differs from the oracle on ({i}, {j})"
        _WANT[key] = want
    return _WANT[key]


def check_topk(got, want, k, largest, what):
    ids, sc = got
    wi, ws = topk_want(want, k, largest)
    what = f"{what}: topk {k} largest={largest}"
    ids = np.asarray(ids).ravel()
    assert np.array_equal(ids, wi), f"{what}: ids differ, first at {int(np.flatnonzero(ids != wi)[0])}"
    assert_bits_equal(sc, ws, what + " scores")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def device_topk(call, k):
    oi = torch.empty(k, dtype=torch.int32, device="cuda")
    os_ = torch.empty(k, dtype=torch.float32, device="cuda")
    call(oi, os_)
    torch.cuda.synchronize()
    return oi.cpu().numpy().view(np.uint32), os_.cpu().numpy()


def both_ways(call, offs, ids, rows=None):
    """The same burst through host lists and through device lists with a device output."""
    host = call(offs, ids, rows, None)
    out = torch.empty(ids.size, dtype=torch.float32, device="cuda")
    call(dev(offs), dev(ids), dev(rows) if rows is not None else None, out)
    torch.cuda.synchronize()
    assert_bits_equal(out.cpu().numpy(), host, "device lists against host lists")
    return host


def groups_of(ms, size):
    return [tuple(ms[at:at + size]) for at in range(0, len(ms), size)]


def group_id(ms):
    return f"m{ms[0]}-{ms[-1]}"


# ------------------------------------------------------------------ (a) whole-store query scan, score form
@pytest.mark.parametrize("m", M.SCAN_MS)
def test_query_scan_score_form(m):
    """score_all from 4096 rows on: pq_scan_skew_kernel (whole, doubled, padded ring rows; SLICED) and
    pq_scan_fast_kernel<NVS, 4, false, SIMPLE> in one slice and on the 128-byte pitch, at exactly 4096 rows, a last tile
    ragged by one row and one workgroup more; host and device output."""
    ns = M.scan_rows(M.scan_tile(m, 4096))
    rows, cen, dim, chunk = pq_shape_store(m, ns[-1], M.CHUNK)
    query = query_of(dim)
    for dist, inv in M.metrics_of(m, "scan"):
        want = query_want(m, ns[-1], chunk, dist, inv)
        for n in ns:
            enc = open_store(rows[:n], cen, dim, chunk, dist, inv)
            assert enc.scan_kernel() == M.scan_kernel_name(m, n), (m, n)
            q = enc.encode_query(query)
            what = f"m {m}, {n} rows, {dist} invert={inv}"
            assert_bits_equal(enc.score_all(q), want[:n], what)
        out = torch.empty(ns[-1], dtype=torch.float32, device="cuda")
        enc.score_all(q, out=out)
        torch.cuda.synchronize()
        assert_bits_equal(out.cpu().numpy(), want, what + ", device output")


# ------------------------------------------------------------------ (b) whole-store query scan, FILTER form
def filter_calls(m, family="scan"):
    return [(dist, inv, largest) for dist, inv in M.metrics_of(m, family) for largest in LARGEST]


@pytest.mark.parametrize("m", M.SCAN_MS)
def test_query_scan_filter_form(m):
    """topk(k = 100) at 32 805 rows: a pivot from a sample (r = 32), then the FILTER twin of every form of (a)
    (test_filter_forms_redo_no_query shows that the filter's own answer is what comes back)."""
    n, k = M.FUSED_ROWS, M.FUSED_K
    assert M.topk_route(m, n, k) == ("fused", M.launch_fast(m, n, True))
    rows, cen, dim, chunk = pq_shape_store(m, n, M.CHUNK)
    query = query_of(dim)
    encs = {}
    for dist, inv, largest in filter_calls(m):
        if (dist, inv) not in encs:
            encs[dist, inv] = open_store(rows, cen, dim, chunk, dist, inv)
        enc = encs[dist, inv]
        assert enc.scan_kernel() == M.scan_kernel_name(m, n)
        want = query_want(m, n, chunk, dist, inv)
        q = enc.encode_query(query)
        what = f"m {m}, {n} rows, {dist} invert={inv}"
        check_topk(enc.topk(q, k, largest), want, k, largest, what)
    got = device_topk(lambda oi, os_: enc.topk(q, k, largest, out_ids=oi, out_scores=os_), k)
    check_topk(got, want, k, largest, what + ", device outputs")


# ------------------------------------------------------------------ (c) pq_scan_kernel, pq_lists_kernel: small stores
SMALL_GROUPS = groups_of(M.SMALL_SCAN_MS[:64], 8) + [M.SMALL_SCAN_MS[64:]]
SHORT_OFFS = np.array([0, 40, 40, 41, 150], dtype=np.uint32)  # lists of unequal length, one of them empty


@pytest.mark.parametrize("ms", SMALL_GROUPS, ids=group_id)
def test_small_store_scan_and_short_lists(ms):
    """301 rows: score_all, score_ids and score_point take pq_scan_kernel<false, VEC16> and score_ids_batch with short
    lists pq_lists_kernel<VEC16>, at every m from 1 to 64 and at 159, 160 and 512 - every remainder of the m / 4 groups,
    the four-group vector loop and the m % 4 tail, dword rows (m < 13) and 16-byte rows.  Distinct queries per list: an
    entry of the next query's table is what a chunk read too many would add."""
    n = M.SMALL_SCAN_ROWS
    for m in ms:
        rows, cen, dim, chunk = pq_shape_store(m, n, M.CHUNK)
        query = query_of(dim)
        rng = np.random.default_rng(m)
        ids = np.concatenate([[0, 1, 2, n - 1, 7, 7], rng.integers(0, n, 200)]).astype(np.uint32)
        for dist, inv in sorted(set(M.metrics_of(m, "small_scan") + M.metrics_of(m, "lists"))):
            enc = open_store(rows, cen, dim, chunk, dist, inv)
            assert enc.scan_kernel() == M.scan_kernel_name(m, n) == ("pq_scan_kernel", 1)
            want = query_want(m, n, chunk, dist, inv)
            what = f"m {m}, {n} rows, {dist} invert={inv}"
            q = enc.encode_query(query)
            assert_bits_equal(enc.score_all(q), want, what + ": score_all")
            assert_bits_equal(enc.score_ids(q, ids), want[ids], what + ": score_ids")
            out = torch.empty(ids.size, dtype=torch.float32, device="cuda")
            enc.score_ids(q, dev(ids), out=out)
            torch.cuda.synchronize()
            assert_bits_equal(out.cpu().numpy(), want[ids], what + ": score_ids, device ids")
            for i in (0, n - 1):
                assert_bits_equal(enc.score_point(q, i), want[i], what + f": score_point({i})")
            queries = pq_shape_queries(dim, 4, seed=5)
            batch = enc.encode_query_batch(queries)
            got = both_ways(lambda o, i, r, out: enc.score_ids_batch(batch, o, i, out=out), SHORT_OFFS, ids[:150])
            for l in range(4):
                a, b = int(SHORT_OFFS[l]), int(SHORT_OFFS[l + 1])
                lut = qo.pq_encode_query(queries[l], chunk, cen, DIST_IDS[dist], inv)
                assert_bits_equal(got[a:b], qo.pq_score_all(rows[ids[a:b]], lut, order=qo.ORDER_SSE) if b > a else got[a:b],
                                  what + f": score_ids_batch, list {l}")


@pytest.mark.parametrize("m", M.LDS_SCAN_MS)
def test_small_rows_scan_with_the_lut_in_lds(m):
    """4109 rows of fewer than 16 chunks: pq_scan_kernel<true, VEC16> (dword rows up to m = 12, 16-byte rows from 13)."""
    n = M.LDS_SCAN_ROWS
    assert M.scan_launch(m, n, n) == [("pq_scan_kernel", True, m >= 13)]
    rows, cen, dim, chunk = pq_shape_store(m, n, M.CHUNK)
    query = query_of(dim)
    for dist, inv in M.metrics_of(m, "lds_scan"):
        enc = open_store(rows, cen, dim, chunk, dist, inv)
        assert enc.scan_kernel() == ("pq_scan_kernel", 1)
        q = enc.encode_query(query)
        want = query_want(m, n, chunk, dist, inv)
        what = f"m {m}, {n} rows, {dist} invert={inv}"
        assert_bits_equal(enc.score_all(q), want, what)
        out = torch.empty(n, dtype=torch.float32, device="cuda")
        enc.score_all(q, out=out)
        torch.cuda.synchronize()
        assert_bits_equal(out.cpu().numpy(), want, what + ", device output")


@pytest.mark.parametrize("m", M.IDS_SCAN_MS)
def test_score_ids_on_both_sides_of_the_lds_budget(m):
    """4100 ids: m = 159 stages its 159 KiB LUT (pq_scan_kernel<true, true>), m = 160 gathers from memory."""
    n, n_ids = M.SMALL_SCAN_ROWS, M.IDS_SCAN_IDS
    assert M.scan_launch(m, n_ids, n, ids=True) == [("pq_scan_kernel", m == 159, True)]
    rows, cen, dim, chunk = pq_shape_store(m, n, M.CHUNK)
    dist, inv = M.metric_of(m)
    enc = open_store(rows, cen, dim, chunk, dist, inv)
    q = enc.encode_query(query_of(dim))
    want = query_want(m, n, chunk, dist, inv)
    ids = np.concatenate([np.arange(n), np.random.default_rng(m).integers(0, n, n_ids - n)]).astype(np.uint32)
    assert_bits_equal(enc.score_ids(q, ids), want[ids], f"m {m}: score_ids of {n_ids}")
    out = torch.empty(n_ids, dtype=torch.float32, device="cuda")
    enc.score_ids(q, dev(ids), out=out)
    torch.cuda.synchronize()
    assert_bits_equal(out.cpu().numpy(), want[ids], f"m {m}: score_ids of {n_ids}, device ids")


# ------------------------------------------------------------------ (d) single-launch top-k
@pytest.mark.parametrize("m", M.SMALL_TOPK_MS + (M.NOT_SMALL_TOPK_M,))
def test_single_launch_topk(m):
    """pq_topk_small_kernel<VEC16> on three workgroups, the last one ragged, k = 1 and 64; m = 129 (a LUT over 128 KiB)
    takes the score array of pq_scan_kernel and the exact select, and gives the same answer."""
    n = M.SMALL_TOPK_ROWS
    small = m != M.NOT_SMALL_TOPK_M
    rows, cen, dim, chunk = pq_shape_store(m, n, M.CHUNK)
    query = query_of(dim)
    for dist, inv in (M.metrics_of(m, "small_topk") if small else [M.metric_of(m)]):
        enc = open_store(rows, cen, dim, chunk, dist, inv)
        q = enc.encode_query(query)
        want = query_want(m, n, chunk, dist, inv)
        for k in M.SMALL_TOPK_KS:
            assert M.topk_route(m, n, k)[0] == ("small" if small else "classic")
            for largest in LARGEST:
                what = f"m {m}, {n} rows, {dist} invert={inv}"
                check_topk(enc.topk(q, k, largest), want, k, largest, what)
        got = device_topk(lambda oi, os_: enc.topk(q, k, largest, out_ids=oi, out_scores=os_), k)
        check_topk(got, want, k, largest, what + ", device outputs")


# ------------------------------------------------------------------ (e) long lists
@pytest.mark.parametrize("m", M.STAGED_FIRST_MS + M.STAGED_LAST_MS + M.NOT_STAGED_MS)
def test_long_lists(m):
    """score_ids_batch with long lists: pq_lists_staged_kernel<NP> at the first and last m of NP = 1 .. 9 (m = 150 and
    160 are not staged: pq_lists_kernel<true>).  Lists end inside, on and across the 1024-pair workgroup ranges, two are
    empty, segments of 127 pairs gather and of 128 stage; with device lists an id out of range scores NaN."""
    n = M.LISTS_ROWS
    lens = np.array(M.LONG_LIST_LENS, dtype=np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    rows, cen, dim, chunk = pq_shape_store(m, n, M.CHUNK)
    rng = np.random.default_rng(m)
    ids = rng.integers(0, n, int(offs[-1])).astype(np.uint32)
    ids[:3] = (0, 1, 2)
    queries = pq_shape_queries(dim, len(lens), seed=9)
    for dist, inv in (M.metrics_of(m, "staged")):
        enc = open_store(rows, cen, dim, chunk, dist, inv)
        batch = enc.encode_query_batch(queries)
        want = np.empty(ids.size, dtype=np.float32)
        for l in range(len(lens)):
            a, b = int(offs[l]), int(offs[l + 1])
            if b > a:
                lut = qo.pq_encode_query(queries[l], chunk, cen, DIST_IDS[dist], inv)
                want[a:b] = qo.pq_score_all(rows[ids[a:b]], lut, order=qo.ORDER_SSE)
        what = f"m {m}, {dist} invert={inv}: score_ids_batch, long lists"
        assert_bits_equal(both_ways(lambda o, i, r, out: enc.score_ids_batch(batch, o, i, out=out), offs, ids), want, what)
    bad = ids.copy()
    bad[4000] = n + 7
    out = torch.empty(ids.size, dtype=torch.float32, device="cuda")
    enc.score_ids_batch(batch, dev(offs), dev(bad), out=out)
    got = out.cpu().numpy()
    assert np.isnan(got[4000])
    keep = np.arange(ids.size) != 4000
    assert_bits_equal(got[keep], want[keep], what + ", one id out of range")


# ------------------------------------------------------------------ (f) stored-row pairs
@pytest.mark.parametrize("m", M.PAIR_MS)
def test_internal_pairs(m):
    """pq_internal_pairs_kernel behind score_internal, score_internal_ids and score_internal_ids_batch: one trip of its
    16-lane loop with idle lanes, an exact trip, a second trip of one lane, ten trips; chunk sizes 1, 3 and 8 with a
    short last chunk."""
    n = M.PAIR_ROWS
    for chunk in M.PAIR_CHUNKS:
        rows, cen, dim, _ = pq_shape_store(m, n, chunk)
        rng = np.random.default_rng(m + chunk)
        ids = np.concatenate([[0, 1, 2, n - 1, 7, 7], rng.integers(0, n, 194)]).astype(np.uint32)
        lrows = np.array([n - 1, 3, 0, int(ids[12])], dtype=np.uint32)
        for dist, inv in M.metrics_of(m, "pairs"):
            enc = open_store(rows, cen, dim, chunk, dist, inv)
            what = f"m {m} chunk {chunk} {dist} invert={inv}"
            for i in (0, n // 2, n - 1):
                want = row_want(m, n, chunk, dist, inv, i)
                assert_bits_equal(enc.score_internal_ids(i, ids), want[ids], what + f": score_internal_ids({i})")
                out = torch.empty(ids.size, dtype=torch.float32, device="cuda")
                enc.score_internal_ids(i, dev(ids), out=out)
                torch.cuda.synchronize()
                assert_bits_equal(out.cpu().numpy(), want[ids], what + f": score_internal_ids({i}), device ids")
                assert_bits_equal(enc.score_internal(i, n - 1), want[n - 1], what + f": score_internal({i}, {n - 1})")
            got = both_ways(lambda o, i, r, out: enc.score_internal_ids_batch(r, o, i, out=out), SHORT_OFFS, ids[:150], lrows)
            for l in range(4):
                a, b = int(SHORT_OFFS[l]), int(SHORT_OFFS[l + 1])
                assert_bits_equal(got[a:b], row_want(m, n, chunk, dist, inv, int(lrows[l]))[ids[a:b]],
                                  what + f": score_internal_ids_batch, list {l}")


# ------------------------------------------------------------------ (g) a stored row against the whole store
def internal_rows(n):
    return (0, n // 2, n - 1)


@pytest.mark.parametrize("m", M.SEQ_MS)
def test_internal_scan_score_form(m):
    """score_internal_all from 4096 rows on: pq_scan_seq_kernel<NVS, UNROLL, false> at the first and last m of NVS 1 .. 9,
    on planar slices and on pitch slices of 1, 2 and 8 pieces; exactly 4096 rows, a ragged last tile, a workgroup more."""
    ns = M.scan_rows(M.seq_tile(m, 4096))
    rows, cen, dim, chunk = pq_shape_store(m, ns[-1], M.CHUNK)
    for dist, inv in M.metrics_of(m, "seq"):
        for n in ns:
            enc = open_store(rows[:n], cen, dim, chunk, dist, inv)
            for i in internal_rows(n)[1:] if n != ns[-1] else internal_rows(n):
                want = row_want(m, n, chunk, dist, inv, i)
                what = f"m {m}, {n} rows, {dist} invert={inv}, row {i}"
                assert_bits_equal(enc.score_internal_all(i), want, what)
        out = torch.empty(n, dtype=torch.float32, device="cuda")
        enc.score_internal_all(i, out=out)
        torch.cuda.synchronize()
        assert_bits_equal(out.cpu().numpy(), want, what + ", device output")


@pytest.mark.parametrize("m", M.SEQ_MS)
def test_internal_scan_filter_form(m):
    """topk_internal(k = 100) at 32 805 rows: the FILTER twins of pq_scan_seq_kernel."""
    n, k = M.FUSED_ROWS, M.FUSED_K
    assert M.topk_internal_route(m, n, k) == ("fused", M.seq_launch(m, n, True))
    rows, cen, dim, chunk = pq_shape_store(m, n, M.CHUNK)
    encs = {}
    for dist, inv, largest in filter_calls(m, "seq"):
        if (dist, inv) not in encs:
            encs[dist, inv] = open_store(rows, cen, dim, chunk, dist, inv)
        enc = encs[dist, inv]
        for i in (0, n - 1):
            want = row_want(m, n, chunk, dist, inv, i)
            what = f"m {m}, {n} rows, {dist} invert={inv}, row {i}"
            check_topk(enc.topk_internal(i, k, largest), want, k, largest, what)
    got = device_topk(lambda oi, os_: enc.topk_internal(i, k, largest, out_ids=oi, out_scores=os_), k)
    check_topk(got, want, k, largest, what + ", device outputs")


@pytest.mark.parametrize("m", M.SEQ_ROWS_STAGED_MS + M.SEQ_ROWS_MS)
def test_internal_scan_of_small_rows_and_small_stores(m):
    """pq_scan_seq_rows_kernel<true> (4109 rows of fewer than 16 chunks) and <false> (301 rows); their top-k is the
    exact select over that score array."""
    n = M.LDS_SCAN_ROWS if m in M.SEQ_ROWS_STAGED_MS else M.SMALL_SCAN_ROWS
    assert M.seq_launch(m, n) == [("pq_scan_seq_rows_kernel", m in M.SEQ_ROWS_STAGED_MS)]
    rows, cen, dim, chunk = pq_shape_store(m, n, M.CHUNK)
    for dist, inv in M.metrics_of(m, "seq_rows"):
        enc = open_store(rows, cen, dim, chunk, dist, inv)
        for i in internal_rows(n):
            want = row_want(m, n, chunk, dist, inv, i)
            what = f"m {m}, {n} rows, {dist} invert={inv}, row {i}"
            assert_bits_equal(enc.score_internal_all(i), want, what)
        for largest in LARGEST:
            check_topk(enc.topk_internal(i, 65, largest), want, 65, largest, what)


# ------------------------------------------------------------------ the children: developer library
def _step(name):
    sys.stderr.write(f"STEP {name}\n")
    sys.stderr.flush()


def _pack(ids, sc):
    return np.stack([np.asarray(ids).ravel().view(np.float32), np.asarray(sc).ravel()])


def child_main(which, out_path):
    """"filter": every FILTER case of (b) and (g) with a STEP line before each call.  "simple": with QAMD_PQ_SKEW=0, the
    score form and the FILTER form of rows of 16 .. 128 chunks."""
    R, names = {}, {}
    n, k = M.FUSED_ROWS, M.FUSED_K
    if which == "filter":
        for m in M.SCAN_MS:
            rows, cen, dim, chunk = pq_shape_store(m, n, M.CHUNK)
            for dist, inv, largest in filter_calls(m):
                enc = open_store(rows, cen, dim, chunk, dist, inv)
                q = enc.encode_query(query_of(dim))
                name = f"q/{m}/{dist}{int(inv)}/{int(largest)}"
                _step(name)
                R[name] = _pack(*enc.topk(q, k, largest))
        for m in M.SEQ_MS:
            rows, cen, dim, chunk = pq_shape_store(m, n, M.CHUNK)
            for dist, inv, largest in filter_calls(m, "seq"):
                enc = open_store(rows, cen, dim, chunk, dist, inv)
                name = f"r/{m}/{dist}{int(inv)}/{int(largest)}"
                _step(name)
                R[name] = _pack(*enc.topk_internal(n - 1, k, largest))
    else:
        for m in M.SIMPLE_MS:
            dist, inv = M.metric_of(m)
            ns = M.scan_rows(M.scan_tile(m, 4096, False))
            rows, cen, dim, chunk = pq_shape_store(m, n, M.CHUNK)
            for nn in ns + (n,):
                enc = open_store(rows[:nn], cen, dim, chunk, dist, inv)
                q = enc.encode_query(query_of(dim))
                name, launches = enc.scan_kernel()
                names[f"{m}/{nn}"] = f"{name}/{launches}"
                R[f"s/{m}/{nn}"] = enc.score_all(q)
            for largest in LARGEST:
                name = f"f/{m}/{int(largest)}"
                _step(name)
                R[name] = _pack(*enc.topk(q, k, largest))
    _step("end")
    R["names"] = np.array([f"{a}={b}" for a, b in names.items()] or [""])
    np.savez(out_path, **R)
    print("DONE")


def run_child(tmp_path, which, env_add):
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
    env.update(env_add, QAMD_LIB_PATH=DEV_LIB, QAMD_DEBUG_TOPK="1")
    out = os.path.join(str(tmp_path), which + ".npz")
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_pq_row_shapes as T\nT.child_main(%r, %r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), which, out))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0 and "DONE" in res.stdout, f"exit {res.returncode}\n{res.stderr[-4000:]}"
    lines, cur = {}, None
    for ln in res.stderr.splitlines():
        if ln.startswith("STEP "):
            cur = ln[5:].strip()
            lines[cur] = []
        elif ln.startswith("[qamd"):
            lines.setdefault(cur, []).append(ln)
    return dict(np.load(out)), lines


def check_line(lines, name):
    n, k = M.FUSED_ROWS, M.FUSED_K
    assert len(lines[name]) == 1 and lines[name][0].startswith(f"[qamd topk] n={n} k={k} r=32 "), (name, lines[name])
    assert lines[name][0].endswith(" 0 queries redone"), f"{name}: the filter's answer was not used: {lines[name][0]}"


@pytest.mark.skipif(not os.path.exists(DEV_LIB), reason="the developer library is not built")
def test_filter_forms_redo_no_query(tmp_path):
    """Every FILTER case of (b) and (g) again, in a fresh process on the developer library: the answers are the
    oracle's, each call printed its one debug line, and every line ends "0 queries redone" - the filter pass neither
    flooded nor came up short, so what the tests above compared was the FILTER kernel's own output."""
    got, lines = run_child(tmp_path, "filter", {})
    n, k = M.FUSED_ROWS, M.FUSED_K
    assert M.fused_policy(n, k)[2] == 32
    calls = 0
    for m in M.SCAN_MS:
        for dist, inv, largest in filter_calls(m):
            name = f"q/{m}/{dist}{int(inv)}/{int(largest)}"
            check_topk((got[name][0].view(np.uint32), got[name][1]), query_want(m, n, M.CHUNK, dist, inv), k, largest, name)
            check_line(lines, name)
            calls += 1
    for m in M.SEQ_MS:
        for dist, inv, largest in filter_calls(m, "seq"):
            name = f"r/{m}/{dist}{int(inv)}/{int(largest)}"
            check_topk((got[name][0].view(np.uint32), got[name][1]), row_want(m, n, M.CHUNK, dist, inv, n - 1), k, largest, name)
            check_line(lines, name)
            calls += 1
    assert calls == sum(len(filter_calls(m)) for m in M.SCAN_MS) + sum(len(filter_calls(m, "seq")) for m in M.SEQ_MS)
    assert set(lines) == set(got) - {"names"} | {"end"}


@pytest.mark.skipif(not os.path.exists(DEV_LIB), reason="the developer library is not built")
def test_simple_fast_forms_with_the_skew_kernel_off(tmp_path):
    """QAMD_PQ_SKEW=0 (a developer switch the product library ignores): rows of 16, 32 .. 128 chunks take
    pq_scan_fast_kernel<NVS, 4, FILTER, true>, NVS = 1 .. 8 - the forms a store past the skew row limit takes.  Score
    form at the three row counts of its tile and at 32 805 rows, FILTER form (k = 100, no query redone), all against the
    oracle."""
    got, lines = run_child(tmp_path, "simple", {"QAMD_PQ_SKEW": "0"})
    n, k = M.FUSED_ROWS, M.FUSED_K
    names = dict(s.split("=") for s in got["names"].tolist())
    for m in M.SIMPLE_MS:
        dist, inv = M.metric_of(m)
        assert M.launch_fast(m, n, True, skew=False) == [("pq_scan_fast_kernel", m // 16, 4, True, True)]
        want = query_want(m, n, M.CHUNK, dist, inv)
        for nn in M.scan_rows(64) + (n,):
            assert names[f"{m}/{nn}"] == "pq_scan_fast_kernel/1" and M.scan_kernel_name(m, nn, skew=False) == ("pq_scan_fast_kernel", 1)
            assert_bits_equal(got[f"s/{m}/{nn}"], want[:nn], f"m {m}, {nn} rows, {dist} invert={inv}, skew kernel off")
        for largest in LARGEST:
            name = f"f/{m}/{int(largest)}"
            check_topk((got[name][0].view(np.uint32), got[name][1]), want, k, largest, name)
            check_line(lines, name)
