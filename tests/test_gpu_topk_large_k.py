"""Every top-k route at large k against a plain reference.

include/quantization_amd.h promises the same thing for every top-k entry point: the exact best k, ties to the lower row id,
sorted best-first, any k up to 1024.  Past k = 64 every route runs other code (the emit kernels' sort instead of the wave
lists, no single-launch small-store kernel, samples and candidate lists sized by 3k), so each route is taken here at
k in KS and compared, id for id and bit for bit, with the stable best-k of the oracle's whole-store scores (util.topk_want).
A batch is checked query by query against the oracle, not against the single-query loop (that loop shares the emit code).

The route of each case is named next to it, with the dispatch condition that sends it there:
  csrc/topk.hip        fused_policy (fused: n >= 32768 and r <= 64), fused_topk, fused_topk_batch (small stores: n <= 2M, k <= 64)
  csrc/u8_batch.hip    qamd_u8_topk_batch (lane mode 1 / vector-ALU scans / matrix cores; fused: n >= 32768 and r <= 64),
                       u8_gemm_route() (csrc/u8_gemm_route.hpp)
  csrc/bin.hip         qamd_bin_topk_batch (matrix cores: 3 or 5+ queries on 512/768/1024/1536-bit rows, 12+ elsewhere,
                       n >= 32768), bin_topk_batch_mfma (r <= 64)
  csrc/pq.hip          qamd_pq_topk_batch (side by side: n >= 2^20 and 256 CUs), launch_fast (sliced rows: m > 144)
At k = 1024 the fused routes need about 100k rows (r = ceil(S * 3072 / n) <= 64 with S = 2048 below 2^20 rows); smaller stores
go to the exact classic path (score array + radix select) for that k, which is a route of its own here.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from util import assert_bits_equal, topk_want

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
torch = pytest.importorskip("torch")
D = qa.DistanceType
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

KS = (1, 64, 65, 256, 1000, 1024)


def _same(got, scores, k, largest, tag, want=None):
    """`want`: topk_want(scores, K >= k, largest), whose first k entries are the answer for k (a stable order's prefix)."""
    gi, gs = got
    wi, ws = topk_want(scores, k, largest) if want is None else (want[0][:k], want[1][:k])
    gi, gs = np.asarray(gi).ravel(), np.asarray(gs).ravel()
    if not np.array_equal(gi, wi):
        bad = np.flatnonzero(gi != wi)
        raise AssertionError(f"{tag} k={k} largest={largest}: {bad.size} ids differ, first at {bad[0]}: "
                             f"got {gi[bad[0]]} want {wi[bad[0]]}")
    assert_bits_equal(gs, ws, f"{tag} k={k} largest={largest} scores")


# ------------------------------------------------------------------ stores and their oracle scores
class _U8:
    def __init__(self, qo, n, dim, dist=D.Dot, seed=0, data=None):
        rng = np.random.default_rng(seed)
        self.qo, self.dim = qo, dim
        self.data = rng.random((n, dim), dtype=np.float32) if data is None else data
        self.enc = qa.EncodedVectorsU8.encode(self.data, qa.VectorParameters(dim, n, dist, False))
        self.rows, self.meta = qo.u8_encode(self.data, int(dist), False)
        self.mode = 0

    def queries(self, nq, seed=1):
        return np.random.default_rng(seed).random((nq, self.dim), dtype=np.float32)

    def want(self, query):
        codes, qoff = self.qo.u8_encode_query(self.meta, query)
        # lane mode 0: the integer sum rounded once; lane mode 1: avx2.c's eight-lane f32 order
        order = self.qo.ORDER_AVX2 if self.mode == 1 else self.qo.ORDER_SIMPLE
        return self.qo.u8_score_all(self.meta, self.rows, codes, qoff, order=order)


class _Bin:
    def __init__(self, qo, n, dim, dist=D.Dot, seed=0):
        rng = np.random.default_rng(seed)
        self.qo, self.dim, self.dist = qo, dim, dist
        self.rows = rng.integers(0, 256, size=(n, dim // 8), dtype=np.uint8)
        self.enc = qa.EncodedVectorsBin.from_storage(self.rows, qa.VectorParameters(dim, n, dist, False))

    def queries(self, nq, seed=1):
        return np.random.default_rng(seed).standard_normal((nq, self.dim)).astype(np.float32)

    def want(self, query):
        qbits = self.qo.bin_encode(query[None, :])[0]
        return self.qo.bin_score_all(self.rows, qbits, self.dim, int(self.dist), False)


class _PQ:
    def __init__(self, qo, n, m, chunk=1, dist=D.Dot, seed=0):
        rng = np.random.default_rng(seed)
        self.qo, self.dim, self.chunk, self.dist = qo, m * chunk, chunk, dist
        self.cen = (rng.random((256, self.dim), dtype=np.float32) - 0.5).astype(np.float32)
        self.rows = rng.integers(0, 256, size=(n, m), dtype=np.uint8)
        self.enc = qa.EncodedVectorsPQ.from_storage(self.rows, qa.VectorParameters(self.dim, n, dist, False), chunk, self.cen)

    def queries(self, nq, seed=1):
        return (np.random.default_rng(seed).random((nq, self.dim), dtype=np.float32) - 0.5).astype(np.float32)

    def want(self, query):
        lut = self.qo.pq_encode_query(query, self.chunk, self.cen, int(self.dist), False)
        return self.qo.pq_score_all(self.rows, lut, order=self.qo.ORDER_SSE)


def _single_all_k(st, tag, ks=KS, nq=2):
    qobj = None
    for qi, query in enumerate(st.queries(nq)):
        want = st.want(query)
        qobj = st.enc.encode_query(query, reuse=qobj)
        for k in ks:
            for largest in (True, False):
                _same(st.enc.topk(qobj, k, largest=largest), want, k, largest, f"{tag} topk query {qi}")


def _batch_all_k(st, nq, tag, ks=KS, seed=1):
    queries = st.queries(nq, seed)
    kmax = max(ks)
    wants = {}
    for qi, query in enumerate(queries):
        s = st.want(query)
        for largest in (True, False):
            wants[qi, largest] = topk_want(s, kmax, largest)
    batch = st.enc.encode_query_batch(queries)
    for k in ks:
        for largest in (True, False):
            ids, sc = st.enc.topk_batch(batch, k, largest=largest)
            assert ids.shape == (nq, k)
            for qi in range(nq):
                _same((ids[qi], sc[qi]), None, k, largest, f"{tag} topk_batch query {qi}/{nq}", wants[qi, largest])


# ------------------------------------------------------------------ single-query topk, all three quantizers
@pytest.mark.parametrize("kind", ["u8", "bin", "pq"])
def test_single_query_topk_every_route(kind, qo):
    """100_003 rows: k <= 64 the single-launch small-store kernel (*_topk_small_kernel: n <= 2M, k <= kSmallTopkMaxK),
    k >= 65 fused_topk (n >= 32768, r = 11 .. 63 <= 64) and fused_emit_kernel's bitonic sort (k > kSmallTopkMaxK).
    20_000 rows: k <= 64 the small-store kernel, k >= 65 the classic path (fused_policy: n < 32768)."""
    for n in (100_003, 20_000):
        st = {"u8": lambda: _U8(qo, n, 64, seed=n),
              "bin": lambda: _Bin(qo, n, 1024, seed=n),
              "pq": lambda: _PQ(qo, n, 96, seed=n)}[kind]()
        _single_all_k(st, f"{kind} n={n}")


def test_single_query_pq_fused_on_a_million_rows(qo):
    """1_100_003 rows (>= 2^20): k <= 64 still the small-store kernel (n <= 2M); k >= 65 fused_topk with the large sample
    (S = 16384, r = 31 .. 46) and the scan's FILTER mode keyed by blockIdx.x (one query per launch)."""
    _single_all_k(_PQ(qo, 1_100_003, 96, seed=5), "pq n=1.1M", nq=1)


# ------------------------------------------------------------------ u8 topk_batch
@pytest.mark.parametrize("n,dim,nq,route", [
    (140_001, 96, 20, "rs"),       # u8_gemm_rs_kernel: one 32-query tile fits in LDS (one tile)
    (140_001, 96, 385, "qs"),      # query-streaming kernel: 131072+ rows, frag_nkb = 1 <= 3 -> qs_min_queries = 385
    (100_003, 1168, 65, "pp"),     # ping-pong kernel: only 64-query tiles fit 1168-byte rows and two would be needed (not rs),
                                   # 65 < qs_min_queries(10) = 129 (not qs); ping-pong: 128 < actual_dim <= 32768
])
def test_u8_batch_matrix_core_routes(n, dim, nq, route, qo):
    """The fused matrix-core path (n >= 32768, r <= 64 at every k: r = 63 at k = 1024 on 100_003 rows): k <= 64
    batch_emit_wave_kernel, k >= 65 batch_emit_kernel (the bitonic sort)."""
    _batch_all_k(_U8(qo, n, dim, seed=n + dim), nq, f"u8 {route} {n}x{dim}")


@pytest.mark.parametrize("dist,nq", [(D.Dot, 2), (D.L1, 3)])
def test_u8_batch_vector_alu_scans(dist, nq, qo):
    """n > 2M: two Dot queries, or L1 with any count, take u8_topk_batch_scans (qamd_u8_topk_batch: one vector-ALU
    u8_scan_multi_kernel filter pass per group of queries) -> fused_topk_batch; n > 2M so never the small-store kernel."""
    n, dim = 2_200_003, 32
    st = _U8(qo, n, dim, dist=dist, seed=nq)
    _batch_all_k(st, nq, f"u8 scans {dist.name}", ks=(1, 64, 65, 1024))


def test_u8_batch_lane_mode_1(qo):
    """set_lane_mode(1) (Dot, actual_dim 2304 > 2080, where avx2.c's order differs from the exact sum): every batch goes through
    u8_topk_batch_scans in the lane order (qamd_u8_topk_batch: u8_lane_order(h)); 40_000 rows: k <= 64 the small-store kernel,
    65 .. 256 fused_topk_batch (r <= 64), 1000 / 1024 the classic path (r = 154 / 158 > 64)."""
    n, dim = 40_000, 2304
    rng = np.random.default_rng(2304)
    data = rng.integers(100, 128, size=(n, dim)).astype(np.float32)
    data[0] = 0.0  # codes are then the values themselves: products past 10^4, sums past 2^24
    st = _U8(qo, n, dim, data=data)
    st.enc.set_lane_mode(1)
    st.mode = 1
    try:
        q = np.random.default_rng(7).integers(100, 128, size=(3, dim)).astype(np.float32)
        st.queries = lambda nq, seed=1: q[:nq]
        _batch_all_k(st, 3, "u8 lane mode 1")
    finally:
        st.enc.set_lane_mode(0)


# ------------------------------------------------------------------ binary topk_batch
@pytest.mark.parametrize("n,dim,nq,route", [
    (100_003, 1024, 12, "rs4"),    # bin_gemm_rs4_kernel: fp4 rows (1024 bits), Q >= 5, the batch's nibble image fits in LDS
    (100_003, 1536, 193, "qs4"),   # bin_gemm_qs4_kernel: 1536-bit rows, 193 queries no longer fit the rs4 image
    (100_003, 2304, 16, "rs"),     # bin_gemm_rs_kernel: 2304-bit rows are no fp4 shape, Q >= kRs4MinQueries = 12
    (100_003, 2048, 11, "valu"),   # fewer than 12 queries on 2048-bit rows: fused_topk_batch, bin_scan_multi_kernel filter
                                   # passes of 8, then 2, then one query alone
])
def test_binary_batch_routes(n, dim, nq, route, qo):
    """Matrix cores (qamd_bin_topk_batch: n >= 32768, r <= 64 in bin_topk_batch_mfma - 63 at k = 1024 on 100_003 rows),
    k <= 64 batch_emit_wave_kernel, else batch_emit_kernel; binary scores tie (dim + 1 values), so queries whose lists
    over/underflow are redone exactly - the answer must not show it."""
    _batch_all_k(_Bin(qo, n, dim, seed=dim + nq), nq, f"bin {route} {dim}")


# ------------------------------------------------------------------ PQ topk_batch
@pytest.mark.parametrize("n,m,nq,route", [
    (1_100_003, 96, 7, "side by side"),   # n >= 2^20, 256 CUs: filter passes of 4 and 2 queries in one launch (SkewBatch), then one alone
    (1_050_011, 192, 5, "sliced"),        # m = 192 > 144: the planar image, slice by slice; 4 side by side, then one
    (120_000, 96, 9, "small"),            # below 2^20 rows: no side-by-side pass; k <= 64 pq_topk_small per query, else the fused
                                          # pipeline query by query (r <= 64)
])
def test_pq_batch_routes(n, m, nq, route, qo):
    _batch_all_k(_PQ(qo, n, m, seed=m + nq), nq, f"pq {route}")


# ------------------------------------------------------------------ edges
def test_batch_k_at_and_past_the_store_size(qo):
    """n = 1000 rows: k = n exactly and k = 1024 > n on the batch path of all three quantizers (small stores: n < 32768 ->
    the per-query exact path); the tail past n holds id 0xFFFFFFFF and -inf (largest) / +inf."""
    n = 1000
    for st, tag in ((_U8(qo, n, 64, seed=1), "u8"), (_Bin(qo, n, 256, seed=1), "bin"), (_PQ(qo, n, 32, seed=1), "pq")):
        _batch_all_k(st, 3, f"{tag} n=1000", ks=(n, 1024))
        ids, sc = st.enc.topk_batch(st.enc.encode_query_batch(st.queries(2)), 1024, largest=False)
        assert np.all(ids[:, n:] == 0xFFFFFFFF) and np.all(np.isposinf(sc[:, n:])), tag


def test_tie_group_straddling_rank_k(qo):
    """600 identical rows whose shared score lands across rank 1000 of query 0: the tie must go to the lowest ids, on the
    fused matrix-core batch path (u8_gemm_rs_kernel, 20 queries, 140_001 rows) and on the single-query fused_topk."""
    n, dim, k = 140_001, 96, 1000
    rng = np.random.default_rng(1000)
    data = rng.random((n, dim), dtype=np.float32)
    queries = rng.random((20, dim), dtype=np.float32)
    first = _U8(qo, n, dim, data=data)
    s0 = first.want(queries[0])
    v = data[int(np.argsort(-s0, kind="stable")[800])].copy()  # a row near rank 800
    data[70_000:70_600] = v
    st = _U8(qo, n, dim, data=data)
    want = st.want(queries[0])
    wi, _ = topk_want(want, k, True)
    inside = np.count_nonzero((wi >= 70_000) & (wi < 70_600))
    assert 0 < inside < 600, f"the tie group must straddle rank {k} (got {inside} of 600 inside)"
    ids, sc = st.enc.topk_batch(st.enc.encode_query_batch(queries), k)
    _same((ids[0], sc[0]), want, k, True, "tie group, batch")
    _same(st.enc.topk(st.enc.encode_query(queries[0]), k), want, k, True, "tie group, single")
    for qi in (1, 19):
        _same((ids[qi], sc[qi]), st.want(queries[qi]), k, True, f"tie group store, query {qi}")


def _heavy_tie_rows(rng, n):
    """Binary dim 128 rows drawn from 16 patterns: a query has at most 16 distinct scores, each shared by ~n / 16 rows.  (Random
    128-bit rows, at most 129 values, do not do it at k = 1024: near the pivot a value is shared by ~1500 of 300_000 rows, and
    the lists hold every candidate.)  At 300_000 rows the best value alone has ~18750 rows, more than the 8192 slots."""
    return rng.integers(0, 256, size=(16, 16), dtype=np.uint8)[rng.integers(0, 16, size=n)]


def test_heavy_ties_at_large_k(qo):
    """Heavy ties at k = 1024 (_heavy_tie_rows): every candidate list overflows, so every query is redone exactly
    (bin_topk_batch_mfma -> fused_topk_batch -> classic radix select; single query: fused_topk -> classic) - the answer is
    still the stable best-k, its ties to the lowest ids."""
    st = _Bin(qo, 300_000, 128, seed=128)
    st.rows = _heavy_tie_rows(np.random.default_rng(128), 300_000)
    st.enc = qa.EncodedVectorsBin.from_storage(st.rows, qa.VectorParameters(128, 300_000, D.Dot, False))
    _batch_all_k(st, 40, "bin dim 128", ks=(1024,))
    _single_all_k(st, "bin dim 128", ks=(1024,), nq=1)


def test_k_1025_is_refused_and_k_0_writes_nothing(qo):
    for st, tag in ((_U8(qo, 40_000, 64, seed=3), "u8"), (_Bin(qo, 40_000, 1024, seed=3), "bin"), (_PQ(qo, 40_000, 32, seed=3), "pq")):
        queries = st.queries(13)  # 13: the matrix-core path of every quantizer
        q = st.enc.encode_query(queries[0])
        batch = st.enc.encode_query_batch(queries)
        with pytest.raises(qa.EncodingError, match="1025"):
            st.enc.topk(q, 1025)
        with pytest.raises(qa.EncodingError, match="1025"):
            st.enc.topk_batch(batch, 1025)
        ids = np.full(8, 77, dtype=np.uint32)
        sc = np.full(8, 5.0, dtype=np.float32)
        st.enc.topk(q, 0, out_ids=ids, out_scores=sc)
        assert np.all(ids == 77) and np.all(sc == 5.0), tag
        d_ids = torch.full((16,), 77, dtype=torch.int32, device="cuda")
        d_sc = torch.full((16,), 5.0, dtype=torch.float32, device="cuda")
        st.enc.topk_batch(batch, 0, out_ids=d_ids, out_scores=d_sc)
        torch.cuda.synchronize()
        assert bool((d_ids == 77).all()) and bool((d_sc == 5.0).all()), tag


def test_sharded_binary_and_pq_batches_at_the_limit(qo):
    """8 shards x k = 1024 (the 8192 merge slots exactly): ShardedVectorsBin / ShardedVectorsPQ topk_batch equal the single
    handle's, which equals the oracle's best-k."""
    n, nq = 40_000, 3
    b = _Bin(qo, n, 512, seed=8)
    p = _PQ(qo, n, 32, seed=8)
    vb = qa.VectorParameters(512, n, D.Dot, False)
    vp = qa.VectorParameters(p.dim, n, D.Dot, False)
    shb = qa.ShardedVectorsBin.from_storage(b.rows, vb, [0] * 8)
    shp = qa.ShardedVectorsPQ.from_storage(p.rows, vp, 1, p.cen, [0] * 8)
    for st, sh, tag in ((b, shb, "bin"), (p, shp, "pq")):
        queries = st.queries(nq)
        for largest in (True, False):
            ids, sc = sh.topk_batch(sh.encode_query_batch(queries), 1024, largest=largest)
            ids1, sc1 = st.enc.topk_batch(st.enc.encode_query_batch(queries), 1024, largest=largest)
            assert np.array_equal(np.asarray(ids), ids1), tag
            assert_bits_equal(sc, sc1, f"{tag} sharded vs single handle")
            for qi in range(nq):
                _same((ids1[qi], sc1[qi]), st.want(queries[qi]), 1024, largest, f"{tag} single handle query {qi}")


# ------------------------------------------------------------------ fallbacks, counted (developer library)
# The developer library prints one line per fused top-k call under QAMD_DEBUG_TOPK, ending "<N> queries redone" (the queries
# whose candidate list over- or underflowed and went to the exact path).  Which shard a candidate lands in is set by the
# workgroup index and the sample ids are fixed, so these counts do not depend on timing.
FALLBACK_SCRIPT = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
import quantization_amd as qa
D = qa.DistanceType
step = sys.argv[1]
rng = np.random.default_rng(2026)
def mark(name):
    print("STEP " + name, file=sys.stderr, flush=True)
if step in ("pq", "all"):
    # PQ side by side: 4.2M rows (S = 16384, r = 12 at k = 1024: ~3072 candidates, spread ~30 %%), 24 queries in groups of 4
    # (and 2 x 2 below); the single-query fused_topk on the same store
    n, m = 4_200_000, 96
    cen = (rng.random((256, m), dtype=np.float32) - 0.5).astype(np.float32)
    rows = rng.integers(0, 256, size=(n, m), dtype=np.uint8)
    enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(m, n, D.Dot, False), 1, cen)
    queries = (rng.random((24, m), dtype=np.float32) - 0.5).astype(np.float32)
    mark("pq_side4")
    enc.topk_batch(enc.encode_query_batch(queries), 1024)
    mark("pq_side2")
    enc.topk_batch(enc.encode_query_batch(queries[:2]), 1024)
    enc.topk_batch(enc.encode_query_batch(queries[2:4]), 1024)
    mark("pq_single")
    for q in queries[:4]:
        enc.topk(enc.encode_query(q), 1024)
    mark("end")
if step in ("u8", "all"):
    # u8 matrix cores: 300_000 x 128, 20 queries (u8_gemm_rs_kernel; S = 2048, r = 21)
    n, dim = 300_000, 128
    data = rng.random((n, dim), dtype=np.float32)
    enc = qa.EncodedVectorsU8.encode(data, qa.VectorParameters(dim, n, D.Dot, False))
    mark("u8_batch")
    enc.topk_batch(enc.encode_query_batch(rng.random((20, dim), dtype=np.float32)), 1024)
    mark("u8_single")
    enc.topk(enc.encode_query(rng.random(dim, dtype=np.float32)), 1024)
    mark("end")
if step in ("bin", "all"):
    # binary matrix cores: 1024-bit rows (a few hundred rows per score value near the pivot), 12 queries (bin_gemm_rs4_kernel)
    n = 400_000
    rows = rng.integers(0, 256, size=(n, 128), dtype=np.uint8)
    enc = qa.EncodedVectorsBin.from_storage(rows, qa.VectorParameters(1024, n, D.Dot, False))
    mark("bin_batch")
    enc.topk_batch(enc.encode_query_batch(rng.standard_normal((12, 1024)).astype(np.float32)), 1024)
    # heavy ties: 128-bit rows drawn from 16 patterns (test_heavy_ties_at_large_k): ~18750 rows share each score
    rows = rng.integers(0, 256, size=(16, 16), dtype=np.uint8)[rng.integers(0, 16, size=300_000)]
    enc = qa.EncodedVectorsBin.from_storage(rows, qa.VectorParameters(128, 300_000, D.Dot, False))
    mark("bin_ties")
    enc.topk_batch(enc.encode_query_batch(rng.standard_normal((40, 128)).astype(np.float32)), 1024)
    enc.topk(enc.encode_query(rng.standard_normal(128).astype(np.float32)), 1024)
    mark("end")
print("DONE")
"""


def run_fallback_script(lib_path, step="all", timeout=600):
    """Runs FALLBACK_SCRIPT in a fresh process on `lib_path` (None: the product library) with QAMD_DEBUG_TOPK=1; returns
    {step name: [(debug line, redone count), ...]}."""
    env = dict(os.environ, QAMD_DEBUG_TOPK="1")
    env.pop("QAMD_LIB_PATH", None)
    if lib_path:
        env["QAMD_LIB_PATH"] = lib_path
    res = subprocess.run([sys.executable, "-c", FALLBACK_SCRIPT % ROOT, step], capture_output=True, text=True,
                         timeout=timeout, env=env)
    assert res.returncode == 0 and "DONE" in res.stdout, res.stderr[-3000:]
    steps, cur = {}, None
    for ln in res.stderr.splitlines():
        if ln.startswith("STEP "):
            cur = ln[5:].strip()
            steps.setdefault(cur, [])
            continue
        mt = re.search(r"(\d+) queries redone", ln)
        if mt and ln.startswith("[qamd"):
            steps.setdefault(cur, []).append((ln, int(mt.group(1))))
    return steps


def test_fallbacks_counted_at_k_1024():
    """Distinct scores at k = 1024: no query is redone on the PQ side-by-side route (groups of 4 and 2), the u8 and binary
    matrix-core routes and the single-query fused route; the heavy-tie binary store redoes at least one (the exact fallback
    really runs).  The product library ignores the switch."""
    dev_lib = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")
    if not os.path.exists(dev_lib):
        pytest.skip("tools/lib/libquantization_amd_dev.so not built (make -C quantization_amd/csrc dev)")
    steps = run_fallback_script(dev_lib)
    for name in ("pq_side4", "pq_side2", "pq_single", "u8_batch", "u8_single", "bin_batch"):
        lines = steps.get(name, [])
        assert lines, f"{name}: no debug line (the route was not the fused one)"
        redone = sum(c for _, c in lines)
        assert redone == 0, f"{name}: {redone} queries redone\n" + "\n".join(ln for ln, _ in lines)
    assert any(ln.startswith("[qamd fused_topk_batch]") for ln, _ in steps["pq_side4"]), steps["pq_side4"]
    assert any(ln.startswith("[qamd bin topk_batch]") for ln, _ in steps["bin_batch"]), steps["bin_batch"]
    assert sum(c for _, c in steps.get("bin_ties", [])) >= 1, steps.get("bin_ties")
    # the product library: same calls, no debug output
    env = dict(os.environ, QAMD_DEBUG_TOPK="1")
    env.pop("QAMD_LIB_PATH", None)
    code = ("import sys; sys.path.insert(0, %r)\nimport numpy as np, quantization_amd as qa\n"
            "rows = np.random.default_rng(1).integers(0, 256, size=(200_000, 32), dtype=np.uint8)\n"
            "enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(32, 200_000, qa.DistanceType.Dot, False), 1,"
            " np.random.default_rng(2).random((256, 32), dtype=np.float32))\n"
            "enc.topk(enc.encode_query(np.ones(32, dtype=np.float32)), 1024)\nprint('DONE')\n") % ROOT
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "DONE" in res.stdout, res.stderr[-2000:]
    assert "[qamd" not in res.stderr, "the product library must ignore QAMD_DEBUG_TOPK"
