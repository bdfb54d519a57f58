"""The binary scan, top-k and pair kernels on every row-length shape, bit for bit against the per-dimension oracle.

csrc/bin.hip picks its single-query kernels from a ladder over rc = ds / 16, the 16-byte pieces of a row: bin_words_kernel
for rows of 4 and 8 bytes (W4, W8) and of more than 64 pieces (WL), bin_scan_kernel<G, ITERS, UNROLL> for rc 1, 2, 3..4,
5..8, 9..16, 17..32, 33..48, 49..64 (S1 .. S64).  A row that does not fill its shape takes the masked form, which clamps
its loads to the row's last piece and relies on q xor q = 0 (one-bit queries) or on zeroed plane pieces (4- and 8-bit
scalar queries, PLANES 4 and 8).  bin_topk_small_kernel (the single-launch top-k), bin_scan_multi_kernel (2, 4 or 8
binary queries per pass) and the FILTER forms behind the fused top-k routes repeat that ladder; bin_pairs_kernel has
three paths by piece count.  tests/binary_row_shapes.py restates all of it and holds the case lists;
tests/test_binary_row_shapes_model.py (no GPU) asserts that the lists reach every instantiation.

Stores come from from_storage over uniform random bits with zero pad bits (util.bin_random_rows).  Every expected value
is util.scalar_scores - the per-dimension oracle, which knows nothing of pieces or planes; a one-bit query is bits = 1
with codes (q_i > 0) - and util.topk_want, compared on raw score bits and ids.  One-bit scores are also compared with
qo.bin_score_all.  Stores of 32 805 rows of more than 2048 bits take their expectation from planes_xor, the plane-wise
popcount sum, which the same test checks against the oracle on the first 2048 rows.  Every query has a positive last
dimension (query_of), and eight more fused stores hold scores of one sign only (fused_rows_query): without the first a
query piece that escaped its mask can be all zero, without the second a candidate offered at 0.0 never passes the pivot.

A fused top-k whose candidate lists flood falls back to the exact route and would hide a wrong filter, so the fused
cases run once more in a child process on the developer library with QAMD_DEBUG_TOPK=1, and every line it prints must
end "0 queries redone".
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import binary_row_shapes as M
from util import (BinOracle, assert_bits_equal, bin_open_rows, bin_query_codes, bin_query_of, bin_random_rows, gaussian,
                  scalar_metric, scalar_planes, scalar_xor, topk_want)

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
D = qa.DistanceType
U8, U128 = qa.BitsStoreType.U8, qa.BitsStoreType.U128
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")

STORES = [(d, U8) for d in M.DIMS] + [(d, U128) for d in M.U128_DIMS]
S_STORES = [(d, U8) for d in M.S_DIMS] + [(d, U128) for d in M.U128_DIMS]
PAIR_ROWS = 301
FUSED_STORES = [("d", d) for d in M.FUSED_DIMS] + [("s", d) for d in M.ONE_SIGN_DIMS]
ORACLE_ROWS = 2048  # rows of more than this many bits, 32 805 of them: planes_xor, checked on this many rows


def store_id(case):
    return f"{case[0]}-{case[1].name}"


def query_of(dim, seed):
    """A query whose last dimension is positive.  At the first rc of a shape that dimension is the only bit of the row's
    last piece, the piece every clamped load reads: a zero bit there would hide a query piece that was not masked."""
    q = bin_query_of(dim, seed)
    q[dim - 1] = abs(q[dim - 1]) + np.float32(0.25)
    return q


def queries_of(rng, count, dim):
    qs = gaussian(rng, (count, dim))
    qs[:, dim - 1] = np.abs(qs[:, dim - 1]) + np.float32(0.25)
    return qs


def metrics_of(dim, kind=U8):
    """One metric per dim, rotating, all six at one dim per shape; the two U128 dims (tiny rows) take all six."""
    return [(D[d], inv) for d, inv in (M.METRICS if kind == U128 else M.metrics_of(dim))]


# ------------------------------------------------------------------ stores and what the oracle says of them
_CASES = {}


def case_of(n, dim, kind=U8):
    """(rows, query, BinOracle) of n random rows, built once; a store of fewer rows is a prefix of them."""
    key = (n, dim, int(kind))
    if key not in _CASES:
        rows = bin_random_rows(n, dim, 31 * n + dim, kind)
        query = query_of(dim, n)
        _CASES[key] = (rows, query, BinOracle(rows, query, dim))
    return _CASES[key]


def qo_scores(qo, rows, query, dim, dist, inv, kind=U8):
    return qo.bin_score_all(rows, qo.bin_encode(query[None, :], int(kind))[0], dim, int(dist), inv, int(kind))


def planes_xor(rows, codes, dim, bits):
    """int64[..., n]: X = sum_b 2^b popcount(plane_b xor row) over whole 8-byte words; codes [dim] or [queries, dim]."""
    codes = np.asarray(codes)
    if codes.ndim == 2:
        return np.stack([planes_xor(rows, c, dim, bits) for c in codes])
    nb = rows.shape[1]
    assert nb % 8 == 0
    words = np.ascontiguousarray(rows).view(np.uint64)
    planes = scalar_planes(codes, bits, nb).view(np.uint64)
    x = np.zeros(rows.shape[0], dtype=np.int64)
    for b in range(bits):
        x += np.bitwise_count(words ^ planes[b][None, :]).sum(axis=1, dtype=np.int64) << b
    return x


def big_xor(rows, codes, dim, bits):
    """X of the 32 805-row stores: the oracle, or past 2048 bits planes_xor checked against it on the first 2048 rows."""
    if dim <= 2048:
        return scalar_xor(rows, codes, dim, bits)
    x = planes_xor(rows, codes, dim, bits)
    assert np.array_equal(x[..., :ORACLE_ROWS], scalar_xor(rows[:ORACLE_ROWS], codes, dim, bits)), \
        f"dim {dim} bits {bits}: the popcount restatement differs from the oracle"
    return x


_BIG = {}


def fused_rows_query(tag, dim):
    """Tag "d": uniform random bits.  Tag "s": every score has one sign - seven bits of eight are set and no query
    dimension is positive, so X is far above half its range - and 0.0, the value a lane that holds no row's score
    carries in bin_scan_kernel, would beat every row in the directions of ONE_SIGN_CALLS (binary_row_shapes.py)."""
    rows = bin_random_rows(M.FUSED_ROWS, dim, 7 * dim + 1)
    if tag == "d":
        return rows, query_of(dim, 100)
    rows |= bin_random_rows(M.FUSED_ROWS, dim, 7 * dim + 2) | bin_random_rows(M.FUSED_ROWS, dim, 7 * dim + 3)
    return rows, -np.abs(bin_query_of(dim, 200))


def fused_case(tag, dim):
    """(rows, query, {planes: X}) of a fused single-query store; the rows are made again on every call, the oracle's
    X is kept."""
    rows, query = fused_rows_query(tag, dim)
    if (tag, dim) not in _BIG:
        _BIG[tag, dim] = {p: big_xor(rows, bin_query_codes(query, p), dim, p) for p in M.PLANES}
    return rows, query, _BIG[tag, dim]


def fused_calls(tag, dim):
    """[(distance, invert, largest)] of the top-k calls a fused store is run with."""
    if tag == "s":
        return [(D[d], inv, largest) for d, inv, largest in M.ONE_SIGN_CALLS]
    return [(dist, inv, largest) for dist, inv in metrics_of(dim) for largest in (True, False)]


def filter_queries(dim, queries):
    return queries_of(np.random.default_rng(500 + dim + queries), queries, dim)


def filter_case(dim, queries):
    """(rows, queries, X [queries, rows]) of a multi-query FILTER case."""
    rows = bin_random_rows(M.FUSED_ROWS, dim, 11 * dim + queries)
    qs = filter_queries(dim, queries)
    if ("filter", dim, queries) not in _BIG:
        _BIG["filter", dim, queries] = big_xor(rows, np.stack([bin_query_codes(q, 1) for q in qs]), dim, 1)
    return rows, qs, _BIG["filter", dim, queries]


def check_topk(got, want, k, largest, what):
    ids, sc = got
    wi, ws = topk_want(want, k, largest)
    what = f"{what}: topk {k} largest={largest}"
    ids = np.asarray(ids).ravel()
    assert np.array_equal(ids, wi), f"{what}: ids differ, first at {int(np.flatnonzero(ids != wi)[0])}"
    assert_bits_equal(sc, ws, what + " scores")


# ------------------------------------------------------------------ (a) whole-store scan, score form
@pytest.mark.parametrize("case", STORES, ids=store_id)
def test_score_form_on_every_shape(qo, case):
    """bin_scan_kernel<G, ITERS, UNROLL, EXACT, false, PLANES> (bin_words_kernel on W4, W8, WL) at a lone row, a ragged
    single tile, a second wave, and a second workgroup with a ragged tile."""
    dim, kind = case
    ds = M.ds_of(dim, kind)
    for planes in M.PLANES:
        ns = M.scan_rows(ds, planes)
        rows, query, oracle = case_of(max(M.scan_rows(ds, 1)), dim, kind)
        for dist, inv in metrics_of(dim, kind):
            want = oracle.scores(planes, dist, inv)
            if planes == 1:
                assert_bits_equal(qo_scores(qo, rows, query, dim, dist, inv, kind), want, f"dim {dim}: the two oracles")
            for n in ns:
                enc = bin_open_rows(rows[:n], dim, dist, inv, kind)
                q = enc.encode_query(query, query_bits=planes)
                what = f"dim {dim} {kind.name}, {n} rows, {dist.name} invert={inv}, planes {planes}"
                assert_bits_equal(enc.score_all(q), want[:n], what)


# ------------------------------------------------------------------ (b) pairs
def row_codes(rows, i, dim):
    return np.unpackbits(rows[i], bitorder="little")[:dim].astype(np.uint32)


@pytest.mark.parametrize("case", STORES, ids=store_id)
def test_pairs_on_every_row_length(qo, case):
    """bin_pairs_kernel<VEC16, PLANES> behind every random-access entry point: dword rows, one piece per lane, the
    4-in-flight loop (9, 32, 33 and 65 pieces among its lengths) and the plane loop."""
    dim, kind = case
    n = PAIR_ROWS
    rows, query, oracle = case_of(n, dim, kind)
    dist, inv = metrics_of(dim, kind)[0]
    enc = bin_open_rows(rows, dim, dist, inv, kind)
    rng = np.random.default_rng(dim)
    ids = np.concatenate([[0, n - 1, 7, 7, n - 1, 0], rng.integers(0, n, 200)]).astype(np.uint32)
    offs = np.array([0, 40, 40, 41, 150], dtype=np.uint32)  # lists of unequal length, one of them empty
    queries = queries_of(rng, 4, dim)
    what = f"dim {dim} {kind.name} {dist.name} invert={inv}"
    for planes in M.PLANES:
        q = enc.encode_query(query, query_bits=planes)
        want = oracle.scores(planes, dist, inv)
        for i in (0, n - 1, int(ids[8])):
            assert_bits_equal(enc.score_point(q, i), want[i], f"{what} planes {planes}: score_point({i})")
        assert_bits_equal(enc.score_ids(q, ids), want[ids], f"{what} planes {planes}: score_ids")
        codes = np.stack([bin_query_codes(qq, planes) for qq in queries])
        wants = scalar_metric(scalar_xor(rows, codes, dim, planes), dim, planes, dist, inv)
        got = enc.score_ids_batch(enc.encode_query_batch(queries, query_bits=planes), offs, ids[:150])
        for l in range(4):
            a, b = int(offs[l]), int(offs[l + 1])
            assert_bits_equal(got[a:b], wants[l][ids[a:b]], f"{what} planes {planes}: score_ids_batch, list {l}")
    # stored rows as queries: one plane
    lrows = np.array([n - 1, 3, 0, int(ids[12])], dtype=np.uint32)
    internal = {int(i): scalar_metric(scalar_xor(rows, row_codes(rows, int(i), dim), dim, 1), dim, 1, dist, inv)
                for i in {0, n - 1, 5, int(ids[9]), int(ids[11])} | set(lrows.tolist())}
    for i, j in ((0, n - 1), (n - 1, 0), (5, 5), (int(ids[9]), int(ids[10]))):
        assert_bits_equal(enc.score_internal(i, j), internal[i][j], f"{what}: score_internal({i}, {j})")
        assert_bits_equal(qo.bin_score_internal(rows, dim, int(dist), inv, i, j, int(kind)), internal[i][j],
                          f"{what}: the two oracles on ({i}, {j})")
    for i in (0, n - 1, int(ids[11])):
        assert_bits_equal(enc.score_internal_ids(i, ids[:70]), internal[i][ids[:70]], f"{what}: score_internal_ids({i})")
    got = enc.score_internal_ids_batch(lrows, offs, ids[:150])
    for l in range(4):
        a, b = int(offs[l]), int(offs[l + 1])
        assert_bits_equal(got[a:b], internal[int(lrows[l])][ids[a:b]], f"{what}: score_internal_ids_batch, list {l}")


# ------------------------------------------------------------------ (c) single-launch top-k
@pytest.mark.parametrize("case", S_STORES, ids=store_id)
def test_single_launch_topk_on_every_shape(qo, case):
    """bin_topk_small_kernel<G, ITERS, EXACT, PLANES> on three workgroups, the last one ragged; plane queries on rows
    of up to 16 pieces.  Binary scores tie heavily: the answer is the stable best k, ties to the lower id."""
    dim, kind = case
    ds = M.ds_of(dim, kind)
    n = M.small_rows(ds)
    rows, query, oracle = case_of(n, dim, kind)
    for planes in M.PLANES:
        if M.small_shape(ds, planes) is None:
            continue
        for dist, inv in metrics_of(dim, kind):
            enc = bin_open_rows(rows, dim, dist, inv, kind)
            q = enc.encode_query(query, query_bits=planes)
            one = enc.encode_query_batch(query[None, :], query_bits=planes)
            want = oracle.scores(planes, dist, inv)
            what = f"dim {dim} {kind.name}, {n} rows, {dist.name} invert={inv}, planes {planes}"
            if planes == 1:
                assert_bits_equal(qo_scores(qo, rows, query, dim, dist, inv, kind), want, what + ": the two oracles")
            for k in M.SMALL_KS:
                assert enc.batch_kernel(one, k) == "bin_topk_small_kernel", what
                for largest in (True, False):
                    check_topk(enc.topk(q, k, largest), want, k, largest, what)


# ------------------------------------------------------------------ (d) classic and fused top-k
@pytest.mark.parametrize("dim", M.CLASSIC_DIMS)
def test_classic_topk_on_every_shape(dim):
    """k = 65 leaves the single launch, and the store is too small for the fused route: the score array of
    bin_scan_kernel's masked form (S1, S2: their only form) and the exact radix select."""
    ds = M.ds_of(dim)
    n = M.small_rows(ds)
    rows, query, oracle = case_of(n, dim)
    dist, inv = metrics_of(dim)[0]
    enc = bin_open_rows(rows, dim, dist, inv)
    for planes in M.PLANES:
        q = enc.encode_query(query, query_bits=planes)
        want = oracle.scores(planes, dist, inv)
        for largest in (True, False):
            check_topk(enc.topk(q, M.CLASSIC_K, largest), want, M.CLASSIC_K, largest,
                       f"dim {dim}, {n} rows, {dist.name} invert={inv}, planes {planes}")


@pytest.mark.parametrize("tag,dim", FUSED_STORES)
def test_fused_topk_on_every_shape(tag, dim):
    """k = 100 at 32 805 rows: a pivot from a sample (r = 32), then the FILTER form of bin_scan_kernel, masked and
    EXACT, at every plane count (test_fused_routes_redo_no_query shows that the filter's answer is the one returned).
    The "s" stores have scores of one sign only: there a candidate offered with the score 0.0 would win."""
    rows, query, xs = fused_case(tag, dim)
    enc = {}
    for dist, inv, largest in fused_calls(tag, dim):
        if (dist, inv) not in enc:
            enc[dist, inv] = bin_open_rows(rows, dim, dist, inv)
        for planes in M.PLANES:
            q = enc[dist, inv].encode_query(query, query_bits=planes)
            want = scalar_metric(xs[planes], dim, planes, dist, inv)
            if tag == "s":
                assert want.max() < 0 if largest else want.min() > 0
            check_topk(enc[dist, inv].topk(q, M.FUSED_K, largest), want, M.FUSED_K, largest,
                       f"{tag} dim {dim}, {M.FUSED_ROWS} rows, {dist.name} invert={inv}, planes {planes}")


# ------------------------------------------------------------------ (e) multi-query scan, score form
@pytest.mark.parametrize("dim", M.MULTI_DIMS)
def test_multi_query_scan_score_form(qo, dim):
    """score_batch of 15 binary queries below the matrix-core gate: bin_scan_multi_kernel in steps of 8 + 4 + 2 and a
    single scan (4 + 4 + 4 + 2 + 1 past 32 pieces).  The queries are distinct: a wrong multi_query_of swaps rows."""
    n, nq = M.MULTI_ROWS, M.MULTI_QUERIES
    rows, _, _ = case_of(n, dim)
    dist, inv = metrics_of(dim)[0]
    enc = bin_open_rows(rows, dim, dist, inv)
    queries = queries_of(np.random.default_rng(dim), nq, dim)
    batch = enc.encode_query_batch(queries)
    assert enc.batch_kernel(batch, 0) == "bin_scan_multi_kernel"
    got = enc.score_batch(batch)
    assert got.shape == (nq, n)
    want = scalar_metric(scalar_xor(rows, np.stack([bin_query_codes(q, 1) for q in queries]), dim, 1), dim, 1, dist, inv)
    for qi in range(nq):
        what = f"dim {dim}, {n} rows, {dist.name} invert={inv}: score_batch of {nq}, query {qi}"
        assert_bits_equal(got[qi], want[qi], what)
        if qi in (0, 7, 8, nq - 1):
            assert_bits_equal(qo_scores(qo, rows, queries[qi], dim, dist, inv), want[qi], what + ": the two oracles")


# ------------------------------------------------------------------ (f) multi-query scan, FILTER form
@pytest.mark.parametrize("dim,queries", M.MULTI_FILTER_CASES)
def test_multi_query_scan_filter_form(dim, queries):
    """topk_batch(k = 100) of binary queries off the matrix cores at 32 805 rows: the FILTER form of
    bin_scan_multi_kernel in steps of 8 + 2 and a single query (4 + 4 + 2 + 1 past 32 pieces), 4 and 2 on 1024 bits."""
    rows, qs, xs = filter_case(dim, queries)
    dist, inv = metrics_of(dim)[0]
    enc = bin_open_rows(rows, dim, dist, inv)
    batch = enc.encode_query_batch(qs)
    assert enc.batch_kernel(batch, M.FUSED_K) == "bin_scan_multi_kernel"
    want = scalar_metric(xs, dim, 1, dist, inv)
    for largest in (True, False):
        ids, sc = enc.topk_batch(batch, M.FUSED_K, largest)
        for qi in range(queries):
            check_topk((ids[qi], sc[qi]), want[qi], M.FUSED_K, largest,
                       f"dim {dim}, {dist.name} invert={inv}: topk_batch of {queries}, query {qi}")


# ------------------------------------------------------------------ the fused routes kept their filter's answer
def child_main(out_path):
    """On the developer library with QAMD_DEBUG_TOPK=1: every fused call of (d) and (f), a STEP line before each."""
    R = {}

    def step(name):
        sys.stderr.write(f"STEP {name}\n")
        sys.stderr.flush()

    for tag, dim in FUSED_STORES:
        rows, query = fused_rows_query(tag, dim)
        enc = {}
        for dist, inv, largest in fused_calls(tag, dim):
            if (dist, inv) not in enc:
                enc[dist, inv] = bin_open_rows(rows, dim, dist, inv)
            for planes in M.PLANES:
                q = enc[dist, inv].encode_query(query, query_bits=planes)
                name = f"{tag}/{dim}/{dist.name}{int(inv)}/{planes}/{int(largest)}"
                step(name)
                ids, sc = enc[dist, inv].topk(q, M.FUSED_K, largest)
                R[name] = np.stack([np.asarray(ids).view(np.float32), np.asarray(sc)])
    for dim, queries in M.MULTI_FILTER_CASES:
        rows = bin_random_rows(M.FUSED_ROWS, dim, 11 * dim + queries)
        qs = filter_queries(dim, queries)
        dist, inv = metrics_of(dim)[0]
        enc = bin_open_rows(rows, dim, dist, inv)
        batch = enc.encode_query_batch(qs)
        for largest in (True, False):
            name = f"f/{dim}/{queries}/{int(largest)}"
            step(name)
            ids, sc = enc.topk_batch(batch, M.FUSED_K, largest)
            R[name] = np.stack([np.asarray(ids).view(np.float32), np.asarray(sc)])
    step("end")
    np.savez(out_path, **R)
    print("DONE")


def test_fused_routes_redo_no_query(tmp_path):
    """Every fused case of (d) and (f) again, in a fresh process on the developer library: the answers are the oracle's,
    each call printed its one debug line, and every line ends "0 queries redone" - the candidate lists (64 x 256 slots)
    neither flooded nor fell short of k, so what the tests above compared was the filter's own answer.  The candidate
    counts are printed (-s) for the record."""
    assert os.path.exists(DEV_LIB), "the developer library is built with the product one (make -C quantization_amd/csrc)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
    env.update(QAMD_LIB_PATH=DEV_LIB, QAMD_DEBUG_TOPK="1")
    out = os.path.join(str(tmp_path), "fused.npz")
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_binary_row_shapes as T\nT.child_main(%r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), out))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "DONE" in res.stdout, f"exit {res.returncode}\n{res.stderr[-4000:]}"
    lines, cur = {}, None
    for ln in res.stderr.splitlines():
        if ln.startswith("STEP "):
            cur = ln[5:].strip()
            lines[cur] = []
        elif ln.startswith("[qamd"):
            lines.setdefault(cur, []).append(ln)
    got = dict(np.load(out))
    n, k = M.FUSED_ROWS, M.FUSED_K
    assert M.fused_policy(n, k)[2] == 32
    counts = {}
    for tag, dim in FUSED_STORES:
        _, _, xs = fused_case(tag, dim)
        for dist, inv, largest in fused_calls(tag, dim):
            for planes in M.PLANES:
                want = scalar_metric(xs[planes], dim, planes, dist, inv)
                name = f"{tag}/{dim}/{dist.name}{int(inv)}/{planes}/{int(largest)}"
                check_topk((got[name][0].view(np.uint32), got[name][1]), want, k, largest, name)
                assert len(lines[name]) == 1 and lines[name][0].startswith(f"[qamd topk] n={n} k={k} r=32 "), (name, lines[name])
                assert lines[name][0].endswith(" 0 queries redone"), f"{name}: the filter's answer was not used: {lines[name][0]}"
                counts.setdefault(f"{tag} {dim} planes {planes}", []).append(int(re.search(r"candidates=(\d+)", lines[name][0]).group(1)))
    for dim, queries in M.MULTI_FILTER_CASES:
        _, _, xs = filter_case(dim, queries)
        dist, inv = metrics_of(dim)[0]
        want = scalar_metric(xs, dim, 1, dist, inv)
        steps = [s for s in M.multi_steps(M.ds_of(dim), queries) if s > 1]
        for largest in (True, False):
            name = f"f/{dim}/{queries}/{int(largest)}"
            ids, sc = got[name][0].view(np.uint32), got[name][1]
            for qi in range(queries):
                check_topk((ids[qi], sc[qi]), want[qi], k, largest, f"{name} query {qi}")
            assert len(lines[name]) == 1 and lines[name][0].startswith(f"[qamd fused_topk_batch] Q={queries} r=32 "), (name, lines[name])
            assert lines[name][0].endswith(" 0 queries redone"), f"{name}: a query took the exact route: {lines[name][0]}"
            m = re.search(r"candidates min/mean/max = (\d+)/(\d+)/(\d+), side by side (\d+) x (\d+),", lines[name][0])
            assert (int(m.group(4)), int(m.group(5))) == (len(steps), max(steps)), (name, lines[name][0])
            counts.setdefault(f"f {dim} queries {queries}", []).extend([int(m.group(1)), int(m.group(3))])
    slots = 64 * 256
    assert all(k <= min(v) and max(v) < slots for v in counts.values())
    print("candidates (min..max over the calls; %d slots): " % slots
          + ", ".join(f"{name}: {min(v)}..{max(v)}" for name, v in counts.items()))
