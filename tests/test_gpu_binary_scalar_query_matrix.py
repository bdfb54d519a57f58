"""Scalar (4- and 8-bit) queries against binary rows across routes, metrics, store kinds and entry points.

Every expected value is util.scalar_scores - the per-dimension oracle of DESIGN.md 3.2d, which knows nothing of bit
planes (checked without a GPU in test_binary_scalar_query_model.py) - on the store's own storage_bytes() or on the
bytes handed to from_storage, and util.topk_want.  Everything is exact: score bits and ids.

Routes of csrc/bin.hip as the tests name them:
  one launch     bin_topk_small_kernel: up to 2M rows, k <= 64, rows of 1..16 16-byte pieces
  classic        the score array (bin_scan_kernel or bin_words_kernel) and the exact radix select
  fused filter   pivot from a sample (bin_words_kernel), then the FILTER form of bin_scan_kernel; under
                 QAMD_DEBUG_TOPK the developer library prints one "[qamd topk] n=.. k=.. r=.." line per such call,
                 ending "1 queries redone" when the candidate lists overflowed and the classic route answered;
                 the other two routes print nothing
"""
import json
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import quantization_amd as qa
from util import BinOracle as Oracle, assert_bits_equal, bin_open_rows as open_rows, bin_query_of as query_of
from util import bin_random_rows as random_rows, gaussian, scalar_codes, scalar_planes, topk_want

pytestmark = pytest.mark.gpu

D = qa.DistanceType
U8, U128 = qa.BitsStoreType.U8, qa.BitsStoreType.U128
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")
METRICS = [(dist, inv) for dist in (D.Dot, D.L1, D.L2) for inv in (False, True)]
BITS = (4, 8)

# (a): n, dim, store kind, ks, route
TOPK_SHAPES = [
    (3_000, 256, U8, (1, 10, 64), "one launch"),
    (3_000, 5_000, U8, (100,), "classic"),      # planes on rows of more than 16 pieces skip the one-launch kernel
    (32_768, 1_024, U8, (100,), "fused"),       # fused_policy (topk.hip): n >= 32768 and r = ceil(2048 * 512 / n) = 32 <= 64
    (3_000, 33, U8, (100,), "classic"),         # 8-byte rows: bin_words_kernel and the radix select
]
# (b): 8 bit patterns at dim 128.  k = 100 takes the fused route from 32 768 rows on (r = ceil(2048 * 512 / 40000) = 27).
# k = 1024 does not at 40 000 rows (r = ceil(2048 * 3072 / 40000) = 158 > 64: classic); 98 304 is the smallest count
# at which fused_policy picks the fused route for it (r = 2048 * 3072 / n <= 64).
TIE_SHAPES = [(40_000, 100), (98_304, 1_024)]
TIE_DIM = 128


# ------------------------------------------------------------------ data and the oracle
def tie_rows(n):
    rng = np.random.default_rng(8 + n)
    return np.ascontiguousarray(rng.integers(0, 256, size=(8, TIE_DIM // 8), dtype=np.uint8)[rng.integers(0, 8, size=n)])


_ORACLES = {}


def shared_oracle(key, make):
    """(rows, query, Oracle) of a shape several tests use, built once."""
    if key not in _ORACLES:
        rows, query, dim = make()
        _ORACLES[key] = (rows, query, Oracle(rows, query, dim))
    return _ORACLES[key]


def topk_shape(n, dim, kind):
    return shared_oracle(("topk", n, dim), lambda: (random_rows(n, dim, n + dim, kind), query_of(dim, n), dim))


def tie_shape(n):
    return shared_oracle(("ties", n), lambda: (tie_rows(n), query_of(TIE_DIM, n), TIE_DIM))


def check_topk(enc, q, want, k, largest, what):
    ids, sc = enc.topk(q, k, largest=largest)
    wi, ws = topk_want(want, k, largest)
    assert np.array_equal(ids, wi), f"{what} k={k} largest={largest}: ids differ"
    assert_bits_equal(sc, ws, f"{what} k={k} largest={largest}")


# ------------------------------------------------------------------ (a) top-k across metrics and directions
@pytest.mark.parametrize("n,dim,kind,ks,route", TOPK_SHAPES, ids=[f"{s[0]}x{s[1]}" for s in TOPK_SHAPES])
def test_topk_across_metrics_and_directions(n, dim, kind, ks, route):
    rows, query, oracle = topk_shape(n, dim, kind)
    for dist, inv in METRICS:
        enc = open_rows(rows, dim, dist, inv, kind)
        for bits in BITS:
            q = enc.encode_query(query, query_bits=bits)
            want = oracle.scores(bits, dist, inv)
            for k in ks:
                for largest in (True, False):
                    check_topk(enc, q, want, k, largest, f"{route} {n}x{dim} {dist.name} invert={inv} bits {bits}")


# ------------------------------------------------------------------ (b) the fused filter under heavy ties
@pytest.mark.parametrize("n,k", TIE_SHAPES)
def test_fused_filter_under_heavy_ties(n, k):
    """At most 8 distinct scores: the rows at least as good as the pivot overflow the candidate lists or fall short of
    k, and the call must still return the exact best k, lower id first (test_routes_... reads the debug line)."""
    rows, query, oracle = tie_shape(n)
    for dist in (D.Dot, D.L2):
        enc = open_rows(rows, TIE_DIM, dist)
        for bits in BITS:
            q = enc.encode_query(query, query_bits=bits)
            want = oracle.scores(bits, dist, False)
            assert np.unique(want).size <= 8
            for largest in (True, False):
                check_topk(enc, q, want, k, largest, f"heavy ties {n} rows {dist.name} bits {bits}")


# ------------------------------------------------------------------ (c) score_ids at length
N_IDS_ROWS = 1_500
IDS_STORES = [(33, U8), (33, U128), (387, U8), (1_024, U8), (2_065, U8), (8_322, U8)]
# 140 001 is past one pass of the 16-byte pairs kernel on a 256-CU device (32 pairs per workgroup and pass, 8 workgroups
# per CU): there a workgroup walks k += GROUPS more than once
IDS_LENGTHS = (1, 7, 8, 9, 2_047, 2_049, 20_011, 140_001)


def id_list(rng, length, n):
    ids = rng.integers(0, n, size=length).astype(np.uint32)
    if length >= 7:
        ids[1] = ids[0]               # duplicates
        ids[length // 2] = 0          # the first row
        ids[length - 2] = n - 1       # the last row
        ids[length - 1] = ids[2]
    return ids


@pytest.mark.parametrize("dim,kind", IDS_STORES, ids=[f"{d}-{k.name}" for d, k in IDS_STORES])
def test_score_ids_at_length(dim, kind):
    torch = pytest.importorskip("torch")
    n = N_IDS_ROWS
    rows = random_rows(n, dim, 5 * dim + int(kind), kind)
    query = query_of(dim, 3)
    oracle = Oracle(rows, query, dim)
    enc = open_rows(rows, dim, D.L2, True, kind)
    rng = np.random.default_rng(dim)
    lists = [id_list(rng, length, n) for length in IDS_LENGTHS]
    for bits in BITS:
        q = enc.encode_query(query, query_bits=bits)
        want = oracle.scores(bits, D.L2, True)
        for ids in lists:
            what = f"dim {dim} {kind.name} bits {bits}, {ids.size} ids"
            assert_bits_equal(enc.score_ids(q, ids), want[ids], what + " (host)")
            d_ids = torch.from_numpy(ids.view(np.int32)).cuda()
            d_out = torch.full((ids.size,), 7.0, dtype=torch.float32, device="cuda")
            assert enc.score_ids(q, d_ids, out=d_out) is d_out
            torch.cuda.synchronize()
            assert_bits_equal(d_out.cpu().numpy(), want[ids], what + " (device)")
    # Row ids >= n.  What the entry point does is established on a binary query: host ids are validated before
    # anything runs and the call fails with OutOfRange (the reference panics on the slice index); device ids cannot
    # be validated, the kernel writes NaN at those positions and exact scores at the others.
    bad = lists[4].copy()
    at = np.array([0, 9, 31, 32, 1_000, bad.size - 1])
    bad[at] = [n, n + 5, 0xFFFFFFFF, n, 1 << 31, n]
    ok = np.ones(bad.size, dtype=bool)
    ok[at] = False
    d_bad = torch.from_numpy(bad.view(np.int32)).cuda()
    for bits in (1,) + BITS:
        q = enc.encode_query(query, query_bits=bits)
        want = oracle.scores(bits, D.L2, True)
        with pytest.raises(IndexError) as e:  # how the binding raises the library's OutOfRange
            enc.score_ids(q, bad)
        assert e.value.__cause__.kind == "OutOfRange", bits
        with pytest.raises(IndexError) as e:
            enc.score_point(q, n)
        assert e.value.__cause__.kind == "OutOfRange", bits
        d_out = torch.full((bad.size,), 7.0, dtype=torch.float32, device="cuda")
        enc.score_ids(q, d_bad, out=d_out)
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        assert np.all(np.isnan(got[at])), f"bits {bits}: an out-of-range id must score NaN"
        assert_bits_equal(got[ok], want[bad[ok]], f"dim {dim} {kind.name} bits {bits}: in-range ids next to bad ones")


# ------------------------------------------------------------------ (d) row-count tails on every mapping
TAIL_ROWS = (1, 3, 5, 31, 33, 63, 65, 255, 257)
# G = 1, 2, 4, 16 lanes per row; two, three and four masked pieces per lane; the words kernel (8-byte and > 64-piece rows)
TAIL_DIMS = (128, 256, 512, 2_048, 3_000, 5_000, 8_000, 33, 8_322)


@pytest.mark.parametrize("dim", TAIL_DIMS)
def test_row_count_tails_on_every_mapping(dim):
    for i, n in enumerate(TAIL_ROWS):
        rows = random_rows(n, dim, 1_000 * dim + n)
        query = query_of(dim, n)
        oracle = Oracle(rows, query, dim)
        dist, inv = METRICS[i % len(METRICS)]
        enc = open_rows(rows, dim, dist, inv)
        for bits in BITS:
            q = enc.encode_query(query, query_bits=bits)
            want = oracle.scores(bits, dist, inv)
            what = f"dim {dim}, {n} rows, {dist.name} invert={inv}, bits {bits}"
            assert_bits_equal(enc.score_all(q), want, what)
            assert_bits_equal(enc.score_point(q, n - 1), want[n - 1], what + ": last row")


# ------------------------------------------------------------------ (e) U128 stores scored
@pytest.mark.parametrize("dim", [1, 33, 129, 387])
def test_u128_stores_scored(dim):
    n = 1_000
    data = gaussian(np.random.default_rng(128 + dim), (n, dim))
    rng = np.random.default_rng(dim)
    ids = id_list(rng, 777, n)
    for dist, inv in ((D.Dot, False), (D.L1, False), (D.L2, True)):
        enc = qa.EncodedVectorsBin.encode(data, qa.VectorParameters(dim, n, dist, inv), store=U128)
        rows = enc.storage_bytes()
        assert rows.shape == (n, 16 * -(-dim // 128))
        query = query_of(dim, 5)
        oracle = Oracle(rows, query, dim)
        for bits in BITS:
            q = enc.encode_query(query, query_bits=bits)
            assert np.array_equal(q.encoded_vector, scalar_planes(scalar_codes(query, bits)[0], bits, rows.shape[1])), \
                f"dim {dim} bits {bits}: planes"
            want = oracle.scores(bits, dist, inv)
            what = f"U128 dim {dim} {dist.name} invert={inv} bits {bits}"
            assert_bits_equal(enc.score_all(q), want, what + ": score_all")
            assert_bits_equal(enc.score_ids(q, ids), want[ids], what + ": score_ids")
            for largest in (True, False):
                check_topk(enc, q, want, 10, largest, what)


# ------------------------------------------------------------------ (f) rescoring
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("dim", [33, 256, 5_000])
def test_topk_rescored_equals_rerank_of_the_candidates(dim, dtype):
    n, k, cand = 3_000, 10, 100
    data = gaussian(np.random.default_rng(3_000 + dim), (n, dim))
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    enc = qa.EncodedVectorsBin.encode(data, vp)
    orig = qa.OriginalVectors.from_data(data, vp, dtype=dtype)
    assert orig.dtype == dtype
    query = query_of(dim, 9)
    oracle = Oracle(enc.storage_bytes(), query, dim)
    for bits in BITS:
        q = enc.encode_query(query, query_bits=bits)
        for largest in (True, False):
            what = f"dim {dim} {dtype} bits {bits} largest={largest}"
            ids, _ = enc.topk(q, cand, largest=largest)
            assert np.array_equal(ids, topk_want(oracle.scores(bits), cand, largest)[0]), what + ": candidates"
            wi, ws = orig.rerank(query, ids, k, largest=largest)
            gi, gs = enc.topk_rescored(q, orig, query, k, cand, largest=largest)
            assert np.array_equal(gi, wi), what
            assert_bits_equal(gs, ws, what + ": rescored scores")


# ------------------------------------------------------------------ (g) routes proven, and a partitioned GPU
ROUTE_METRICS = [(D.Dot, False), (D.L2, True)]


def route_calls():
    """(tag, rows key, dim, k, largest) of every top-k the children run; the tag's first field names its store."""
    calls = []
    for n, dim, kind, ks, route in TOPK_SHAPES:
        for k in ks:
            calls.append((f"a/{n}x{dim}", ("a", n, dim, int(kind)), dim, k, route))
    for n, k in TIE_SHAPES:
        calls.append((f"b/{n}x{TIE_DIM}", ("b", n), TIE_DIM, k, "fused"))
    return calls


def route_rows(key):
    if key[0] == "a":
        _, n, dim, kind = key
        return topk_shape(n, dim, qa.BitsStoreType(kind))
    return tie_shape(key[1])


def child_main(out_path):
    R = {}
    for tag, key, dim, k, _ in route_calls():
        rows, query, _ = route_rows(key)
        kind = qa.BitsStoreType(key[3]) if key[0] == "a" else U8
        for dist, inv in ROUTE_METRICS:
            enc = open_rows(rows, dim, dist, inv, kind)
            for bits in BITS:
                q = enc.encode_query(query, query_bits=bits)
                name = f"{tag}/{dist.name}{int(inv)}/{bits}"
                if name + "/all" not in R:
                    R[name + "/all"] = enc.score_all(q)
                for largest in (True, False):
                    sys.stderr.write(f"STEP {name}/{k}/{int(largest)}\n")
                    sys.stderr.flush()
                    ids, sc = enc.topk(q, k, largest=largest)
                    R[f"{name}/{k}/{int(largest)}"] = np.stack([np.asarray(ids).view(np.float32), np.asarray(sc)])
    sys.stderr.write("STEP end\n")
    np.savez(out_path, **R)
    print("DONE")


def run_child(tmp_dir, name, env_add, timeout=600):
    """A fresh process on the developer library with QAMD_DEBUG_TOPK=1: (results, {step: [debug lines]})."""
    assert os.path.exists(DEV_LIB), "the developer library is built with the product one (make -C quantization_amd/csrc)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
    env.update(env_add, QAMD_LIB_PATH=DEV_LIB, QAMD_DEBUG_TOPK="1")
    out = os.path.join(str(tmp_dir), name + ".npz")
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_binary_scalar_query_matrix as T\nT.child_main(%r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), out))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=env)
    assert res.returncode == 0 and "DONE" in res.stdout, f"{name}: exit {res.returncode}\n{res.stderr[-4000:]}"
    lines, cur = {}, None
    for ln in res.stderr.splitlines():
        if ln.startswith("STEP "):
            cur = ln[5:].strip()
            lines[cur] = []
        elif ln.startswith("[qamd"):
            lines.setdefault(cur, []).append(ln)
    return dict(np.load(out)), lines


def test_routes_proven_and_a_partitioned_gpu(tmp_path):
    """Two children, the whole device and one sized as 40 CUs (QAMD_DEV_CU_COUNT): byte-identical results, equal to the
    oracle, and each top-k on the route the comments of (a) and (b) claim.  A child that fails ends this test at once.
    The debug line proves fused against not fused only: the one-launch and the classic route both print nothing, so
    this test cannot tell a plane query that left bin_topk_small_kernel for the classic route.  That the 3 000 x 256
    shape is served by one launch with no read-back is shown by test_one_launch_topk_is_capturable alone."""
    whole = run_child(tmp_path, "whole", {})
    cu40 = run_child(tmp_path, "cu40", {"QAMD_DEV_CU_COUNT": "40"})
    assert sorted(whole[0]) == sorted(cu40[0])
    for name in whole[0]:
        assert np.array_equal(whole[0][name].view(np.uint32), cu40[0][name].view(np.uint32)), f"{name}: 40 CUs differ"
    report = {}
    for tag, key, dim, k, route in route_calls():
        _, _, oracle = route_rows(key)
        n = oracle.rows.shape[0]
        for dist, inv in ROUTE_METRICS:
            for bits in BITS:
                name = f"{tag}/{dist.name}{int(inv)}/{bits}"
                want = oracle.scores(bits, dist, inv)
                assert_bits_equal(whole[0][name + "/all"], want, name + ": score_all")
                for largest in (True, False):
                    step = f"{name}/{k}/{int(largest)}"
                    got = whole[0][step]
                    wi, ws = topk_want(want, k, largest)
                    assert np.array_equal(got[0].view(np.uint32), wi), step + ": ids"
                    assert_bits_equal(got[1], ws, step + ": scores")
                    for run in (whole, cu40):
                        lines = run[1][step]
                        if route == "fused":
                            assert len(lines) == 1 and lines[0].startswith(f"[qamd topk] n={n} k={k} r="), (step, lines)
                            redone = int(re.search(r"(\d+) queries redone$", lines[0]).group(1))
                            if tag.startswith("a/"):
                                assert redone == 0, f"{step}: the filter's answer was not used: {lines[0]}"
                            report.setdefault(f"{tag} k={k}", set()).add(f"fused, {redone} redone")
                        else:
                            assert lines == [], f"{step}: expected the {route} route, got {lines}"
                            report.setdefault(f"{tag} k={k}", set()).add(route + " (no fused line)")
    print("routes: " + json.dumps({k: sorted(v) for k, v in report.items()}))


# ------------------------------------------------------------------ (h) device outputs, stream, capture, threads
def test_device_outputs_on_a_side_stream():
    torch = pytest.importorskip("torch")
    n, dim = 3_000, 256
    rows, query, oracle = topk_shape(n, dim, U8)
    enc = open_rows(rows, dim, D.L1, False)
    ids = id_list(np.random.default_rng(1), 2_049, n)
    side = torch.cuda.Stream()
    for bits in BITS:
        want = oracle.scores(bits, D.L1, False)
        host_q = enc.encode_query(query, query_bits=bits)
        h_all, h_ids, (h_ti, h_ts) = enc.score_all(host_q), enc.score_ids(host_q, ids), enc.topk(host_q, 10)
        assert_bits_equal(h_all, want, f"bits {bits}: host score_all")
        with torch.cuda.stream(side):
            q = enc.encode_query(torch.from_numpy(query).cuda(), query_bits=bits, stream=side)
            d_all = torch.empty(n, dtype=torch.float32, device="cuda")
            d_sc = torch.empty(ids.size, dtype=torch.float32, device="cuda")
            d_ti = torch.empty(10, dtype=torch.int32, device="cuda")
            d_ts = torch.empty(10, dtype=torch.float32, device="cuda")
            enc.score_all(q, out=d_all, stream=side)
            enc.score_ids(q, torch.from_numpy(ids.view(np.int32)).cuda(), out=d_sc, stream=side)
            enc.topk(q, 10, out_ids=d_ti, out_scores=d_ts, stream=side)
            side.synchronize()
        assert_bits_equal(d_all.cpu().numpy(), h_all, f"bits {bits}: score_all to a device buffer")
        assert_bits_equal(d_sc.cpu().numpy(), h_ids, f"bits {bits}: score_ids to a device buffer")
        assert np.array_equal(d_ti.cpu().numpy().view(np.uint32), h_ti), f"bits {bits}: topk ids to a device buffer"
        assert_bits_equal(d_ts.cpu().numpy(), h_ts, f"bits {bits}: topk scores to a device buffer")


@pytest.mark.parametrize("bits", BITS)
def test_one_launch_topk_is_capturable(bits):
    """As test_small_store_topk_is_capturable_with_device_outputs does for a u8 query: encode_query + topk with device
    outputs only enqueue on the one-launch route, so they replay from a graph."""
    torch = pytest.importorskip("torch")
    n, dim, k = 3_000, 256, 10
    rows, _, _ = topk_shape(n, dim, U8)
    enc = open_rows(rows, dim)
    qbuf = torch.from_numpy(query_of(dim, 50)).cuda()
    d_ids = torch.empty(k, dtype=torch.int32, device="cuda")
    d_sc = torch.empty(k, dtype=torch.float32, device="cuda")
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        qobj = enc.encode_query(qbuf, query_bits=bits)
        enc.topk(qobj, k, out_ids=d_ids, out_scores=d_sc)  # warm-up: workspace allocation happens here
        side.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            enc.encode_query(qbuf, reuse=qobj, query_bits=bits)
            enc.topk(qobj, k, out_ids=d_ids, out_scores=d_sc)
    for trial in range(2):
        query = query_of(dim, 51 + trial)
        qbuf.copy_(torch.from_numpy(query))
        g.replay()
        torch.cuda.synchronize()
        want = Oracle(rows, query, dim).scores(bits)
        wi, ws = topk_want(want, k, True)
        ei, es = enc.topk(enc.encode_query(query, query_bits=bits), k)
        assert np.array_equal(ei, wi) and np.array_equal(d_ids.cpu().numpy().view(np.uint32), wi), (bits, trial)
        assert_bits_equal(es, ws, f"bits {bits} replay {trial}: eager scores")
        assert_bits_equal(d_sc.cpu().numpy(), ws, f"bits {bits} replay {trial}: replayed scores")


def test_two_threads_on_one_store():
    n, dim, rounds = 20_000, 512, 30
    rows = random_rows(n, dim, 20_512)
    enc = open_rows(rows, dim)
    queries = {bits: [query_of(dim, 100 * bits + r) for r in range(3)] for bits in BITS}
    want = {}
    for bits in BITS:  # the single-threaded answers, themselves checked against the oracle
        for r, query in enumerate(queries[bits]):
            q = enc.encode_query(query, query_bits=bits)
            sc, (ti, ts) = enc.score_all(q), enc.topk(q, 10)
            w = Oracle(rows, query, dim).scores(bits)
            assert_bits_equal(sc, w, f"bits {bits} query {r}")
            assert np.array_equal(ti, topk_want(w, 10, True)[0])
            want[bits, r] = (sc, ti, ts)
    errors = []

    def work(bits):
        try:
            h = enc.encode_query(queries[bits][0], query_bits=bits)
            for i in range(rounds):
                r = i % 3
                assert enc.encode_query(queries[bits][r], reuse=h, query_bits=bits) is h
                sc, (ti, ts) = enc.score_all(h), enc.topk(h, 10)
                w_sc, w_ti, w_ts = want[bits, r]
                assert_bits_equal(sc, w_sc, f"bits {bits} round {i}: score_all")
                assert np.array_equal(ti, w_ti), f"bits {bits} round {i}: topk ids"
                assert_bits_equal(ts, w_ts, f"bits {bits} round {i}: topk scores")
        except BaseException as e:  # noqa: BLE001 - reported by the parent thread
            errors.append(e)
        finally:
            qa.thread_release()

    threads = [threading.Thread(target=work, args=(bits,)) for bits in (8, 4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
