"""Rescoring with the original f32 vectors (qamd_f32_*, *_topk_rescored) against the oracle's restatement of
DistanceType::distance (encoded_vectors.rs:37-45; oracle qo_metric_f32): every comparison is bit-exact, there are no
tolerances.  The expected top-k is tests/util.py topk_want applied to the oracle's exact scores of the listed ids, taken
in ascending id order so that its tie rule (lower position) is the contract's (lower id)."""
import os
import sys
import threading

import numpy as np
import pytest

from util import assert_bits_equal, topk_want

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
torch = pytest.importorskip("torch")
from oracle import qoracle as qo  # noqa: E402

D = qa.DistanceType
PAD = 0xFFFFFFFF
METRICS = [(D.Dot, False), (D.Dot, True), (D.L1, False), (D.L1, True), (D.L2, False), (D.L2, True)]


def exact(dist, invert, q, data, ids):
    """qo_metric_f32(dist, q, data[id]) for every id, sign flipped for invert."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    data = np.ascontiguousarray(data, dtype=np.float32)
    fn, dim, base, qp = qo.lib().qo_metric_f32, data.shape[1], data.ctypes.data, q.ctypes.data
    out = np.array([fn(int(dist), qp, base + int(i) * dim * 4, dim) for i in ids], dtype=np.float32)
    return -out if invert else out


def want_rerank(dist, invert, q, data, ids, k, largest):
    ids = np.asarray(ids, dtype=np.uint32).ravel()
    valid = np.sort(ids[ids != PAD], kind="stable")
    pos, sc = topk_want(exact(dist, invert, q, data, valid), k, largest)
    out = np.full(k, PAD, dtype=np.uint32)
    out[pos != PAD] = valid[pos[pos != PAD]]
    return out, sc


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def special_data(rng, n, dim):
    data = rng.standard_normal((n, dim)).astype(np.float32)
    data[0] = np.where(np.arange(dim) % 2 == 0, 0.0, -0.0)
    data[1] = (rng.standard_normal(dim) * 1e-40).astype(np.float32)  # subnormals
    data[2] = np.float32(np.finfo(np.float32).max / dim) * rng.uniform(0.5, 1.0, dim).astype(np.float32)
    data[3] = -data[2]
    data[4, ::3] = np.float32(1e-39)
    return data


def special_query(rng, dim):
    q = rng.standard_normal(dim).astype(np.float32)
    q[::5] = np.float32(3e-41)
    q[1::7] = -0.0
    return q


# ------------------------------------------------------------------------------------------------ 1. score_ids
@pytest.mark.parametrize("dim", [1, 3, 64, 65, 768, 1536, 4099])
@pytest.mark.parametrize("dist,invert", METRICS)
def test_score_ids_is_the_oracle_metric(dim, dist, invert):
    rng = np.random.default_rng(dim * 10 + int(dist) * 2 + invert)
    n = 300
    data = special_data(rng, n, dim)
    orig = qa.OriginalVectors.from_data(data, qa.VectorParameters(dim, n, dist, invert))
    ids = np.concatenate([np.arange(8), rng.integers(0, n, 192)]).astype(np.uint32)
    for q in (rng.standard_normal(dim).astype(np.float32), special_query(rng, dim)):
        want = exact(dist, invert, q, data, ids)
        assert_bits_equal(orig.score_ids(q, ids), want, "host ids, host out")
        out = torch.empty(ids.size, device="cuda")
        orig.score_ids(q, ids, out=out)
        assert_bits_equal(out.cpu().numpy(), want, "host ids, device out")
        assert_bits_equal(orig.score_ids(q, dev_u32(ids)), want, "device ids, host out")
        out = torch.empty(ids.size, device="cuda")
        orig.score_ids(torch.from_numpy(q).cuda(), dev_u32(ids), out=out)
        torch.cuda.synchronize()
        assert_bits_equal(out.cpu().numpy(), want, "device query, ids and out")
    # a long host list leaves the mapped scratch (more than 1024 ids)
    many = rng.integers(0, n, 1500).astype(np.uint32)
    assert_bits_equal(orig.score_ids(q, many), exact(dist, invert, q, data, many), "1500 host ids")


def test_score_ids_out_of_range():
    rng = np.random.default_rng(5)
    data = rng.standard_normal((50, 20)).astype(np.float32)
    orig = qa.OriginalVectors.from_data(data, qa.VectorParameters(20, 50, D.L2, False))
    q = rng.standard_normal(20).astype(np.float32)
    with pytest.raises(IndexError):
        orig.score_ids(q, np.array([1, 50], dtype=np.uint32))
    ids = np.array([3, 50, 7, PAD, 49], dtype=np.uint32)
    got = orig.score_ids(q, dev_u32(ids))
    assert np.isnan(got[1]) and np.isnan(got[3])
    keep = [0, 2, 4]
    assert_bits_equal(got[keep], exact(D.L2, False, q, data, ids[keep]), "in-range device ids beside bad ones")
    with pytest.raises(qa.EncodingError):
        orig.score_ids(q[:19], ids[:1])


# ------------------------------------------------------------------------------------------------ 2. score_ids_batch
@pytest.mark.parametrize("dist,invert", [(D.Dot, False), (D.L1, True), (D.L2, False)])
@pytest.mark.parametrize("dim", [3, 65, 768])
def test_score_ids_batch_is_score_ids_per_list(dim, dist, invert):
    rng = np.random.default_rng(dim + int(dist))
    n = 400
    data = special_data(rng, n, dim)
    orig = qa.OriginalVectors.from_data(data, qa.VectorParameters(dim, n, dist, invert))
    lens = [3, 0, 70, 1, 0, 300, 64, 130, 0]  # ragged, empty lists, lists longer than a workgroup's 256 pairs
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    ids = rng.integers(0, n, int(offs[-1])).astype(np.uint32)
    queries = rng.standard_normal((len(lens), dim)).astype(np.float32)
    queries[2] = special_query(rng, dim)
    want = np.concatenate([exact(dist, invert, queries[l], data, ids[offs[l]:offs[l + 1]]) for l in range(len(lens))])
    assert_bits_equal(orig.score_ids_batch(queries, offs, ids), want, "host lists, host out")
    out = torch.empty(ids.size, device="cuda")
    orig.score_ids_batch(queries, offs, ids, out=out)
    assert_bits_equal(out.cpu().numpy(), want, "host lists, device out")
    out = torch.empty(ids.size, device="cuda")
    orig.score_ids_batch(torch.from_numpy(queries).cuda(), dev_u32(offs), dev_u32(ids), out=out)
    torch.cuda.synchronize()
    assert_bits_equal(out.cpu().numpy(), want, "device lists, device out")
    # a small burst rides in the mapped scratch
    small_offs = np.array([0, 2, 2, 5], dtype=np.uint32)
    want = np.concatenate([exact(dist, invert, queries[l], data, ids[small_offs[l]:small_offs[l + 1]]) for l in range(3)])
    assert_bits_equal(orig.score_ids_batch(queries[:3], small_offs, ids[:5]), want, "small burst")
    with pytest.raises(IndexError):
        orig.score_ids_batch(queries[:1], np.array([0, 1], dtype=np.uint32), np.array([n], dtype=np.uint32))


# ------------------------------------------------------------------------------------------------ 3. rerank
def tie_data(rng, n, dim):
    """Rows with engineered exact ties: every row of the second half repeats a row of the first half."""
    data = rng.standard_normal((n, dim)).astype(np.float32)
    data[n // 2:] = data[rng.integers(0, n // 2, n - n // 2)]
    return data


@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("k", [1, 10, 1024])
def test_rerank_is_topk_want_of_the_oracle_scores(k, largest):
    rng = np.random.default_rng(k + largest)
    n, dim = 9000, 24
    data = tie_data(rng, n, dim)
    for dist, invert in ((D.Dot, False), (D.L2, True)):
        orig = qa.OriginalVectors.from_data(data, qa.VectorParameters(dim, n, dist, invert))
        q = rng.standard_normal(dim).astype(np.float32)
        for n_ids in sorted({k, 1000, 8192}):
            ids = rng.permutation(n)[:n_ids].astype(np.uint32)
            want_ids, want_sc = want_rerank(dist, invert, q, data, ids, k, largest)
            got_ids, got_sc = orig.rerank(q, ids, k, largest)
            assert np.array_equal(got_ids, want_ids), (dist, n_ids)
            assert_bits_equal(got_sc, want_sc, f"rerank scores {dist} {n_ids}")
            oi, osc = torch.empty(k, dtype=torch.int32, device="cuda"), torch.empty(k, device="cuda")
            orig.rerank(torch.from_numpy(q).cuda(), dev_u32(ids), k, largest, out_ids=oi, out_scores=osc)
            torch.cuda.synchronize()
            assert np.array_equal(host_u32(oi), want_ids)
            assert_bits_equal(osc.cpu().numpy(), want_sc, "rerank, device buffers")
            # the padding id is skipped wherever it stands
            padded = ids.copy()
            padded[rng.integers(0, n_ids, max(1, n_ids // 7))] = PAD
            want_ids, want_sc = want_rerank(dist, invert, q, data, padded, k, largest)
            got_ids, got_sc = orig.rerank(q, padded, k, largest)
            assert np.array_equal(got_ids, want_ids), ("padded", dist, n_ids)
            assert_bits_equal(got_sc, want_sc, "rerank of a padded list")
        with pytest.raises(qa.EncodingError):
            orig.rerank(q, np.zeros(8193, dtype=np.uint32), k, largest)
    with pytest.raises(qa.EncodingError):
        orig.rerank(q, ids, 1025, largest)
    with pytest.raises(IndexError):
        orig.rerank(q, np.array([0, n], dtype=np.uint32), 1, largest)


def test_rerank_ties_go_to_the_lower_id_and_short_lists_are_padded():
    rng = np.random.default_rng(11)
    n, dim = 64, 7
    data = rng.standard_normal((n, dim)).astype(np.float32)
    data[40] = data[5]
    data[41] = data[5]
    orig = qa.OriginalVectors.from_data(data, qa.VectorParameters(dim, n, D.Dot, False))
    q = data[5].copy()
    ids = np.array([41, 9, 5, PAD, 40, 12], dtype=np.uint32)
    for largest in (True, False):
        got_ids, got_sc = orig.rerank(q, ids, 8, largest)
        want_ids, want_sc = want_rerank(D.Dot, False, q, data, ids, 8, largest)
        assert np.array_equal(got_ids, want_ids)
        assert_bits_equal(got_sc, want_sc, "ties and padding")
        tied = [int(i) for i in got_ids if i in (5, 40, 41)]
        assert tied == [5, 40, 41]
        assert list(got_ids[5:]) == [PAD] * 3 and np.all(np.isinf(got_sc[5:]))
    got_ids, _ = orig.rerank(q, np.array([PAD, PAD], dtype=np.uint32), 3, True)
    assert list(got_ids) == [PAD] * 3


@pytest.mark.parametrize("largest", [False, True])
def test_rerank_batch(largest):
    rng = np.random.default_rng(3 + largest)
    n, dim = 3000, 65
    data = tie_data(rng, n, dim)
    for (dist, invert), nq, n_ids, k in (((D.L2, False), 5, 100, 10), ((D.Dot, True), 3, 1000, 1024), ((D.L1, False), 70, 37, 1)):
        orig = qa.OriginalVectors.from_data(data, qa.VectorParameters(dim, n, dist, invert))
        queries = rng.standard_normal((nq, dim)).astype(np.float32)
        ids = np.stack([rng.permutation(n)[:n_ids] for _ in range(nq)]).astype(np.uint32)
        ids[0, ::9] = PAD
        got_ids, got_sc = orig.rerank_batch(queries, ids, k, largest)
        oi, osc = torch.empty((nq, k), dtype=torch.int32, device="cuda"), torch.empty((nq, k), device="cuda")
        orig.rerank_batch(torch.from_numpy(queries).cuda(), dev_u32(ids), k, largest, out_ids=oi, out_scores=osc)
        torch.cuda.synchronize()
        for j in range(nq):
            want_ids, want_sc = want_rerank(dist, invert, queries[j], data, ids[j], k, largest)
            assert np.array_equal(got_ids[j], want_ids), (dist, j)
            assert_bits_equal(got_sc[j], want_sc, f"rerank_batch query {j}")
            assert np.array_equal(host_u32(oi)[j], want_ids)
            assert_bits_equal(osc.cpu().numpy()[j], want_sc, f"rerank_batch query {j}, device buffers")


# ------------------------------------------------------------------------------------------------ 4.-6. the fused calls
def make_store(kind, data, vp, rng):
    if kind == "u8":
        return qa.EncodedVectorsU8.encode(data, vp)
    if kind == "pq":
        cen = rng.standard_normal((256, vp.dim)).astype(np.float32)
        return qa.EncodedVectorsPQ.encode(data, vp, 8, centroids=cen)
    return qa.EncodedVectorsBin.encode(data, vp)


STORES = [("u8", 64), ("pq", 64), ("pq", 68), ("bin", 64)]


def want_rescored(enc, q, dist, invert, q_f32, data, k, candidates, largest):
    cand, _ = enc.topk(q, candidates, largest)
    return want_rerank(dist, invert, q_f32, data, cand, k, largest)


@pytest.mark.parametrize("kind,dim", STORES)
@pytest.mark.parametrize("largest", [False, True])
def test_topk_rescored_is_topk_then_exact_rerank(kind, dim, largest):
    rng = np.random.default_rng(dim + largest)
    n = 50_000
    data = tie_data(rng, n, dim)
    dist, invert = (D.Dot, False) if largest else (D.L2, False)
    vp = qa.VectorParameters(dim, n, dist, invert)
    enc = make_store(kind, data, vp, rng)
    orig = qa.OriginalVectors.from_data(data, vp)
    q_f32 = rng.standard_normal(dim).astype(np.float32)
    q = enc.encode_query(q_f32)
    for k in (1, 10, 30, 1024):
        for candidates in sorted({k, 100, 1024}):
            if candidates < k:
                continue
            want_ids, want_sc = want_rescored(enc, q, dist, invert, q_f32, data, k, candidates, largest)
            got_ids, got_sc = enc.topk_rescored(q, orig, q_f32, k, candidates, largest)
            assert np.array_equal(got_ids, want_ids), (kind, k, candidates)
            assert_bits_equal(got_sc, want_sc, f"{kind} topk_rescored({k}, {candidates})")
            oi, osc = torch.empty(k, dtype=torch.int32, device="cuda"), torch.empty(k, device="cuda")
            enc.topk_rescored(q, orig, torch.from_numpy(q_f32).cuda(), k, candidates, largest, out_ids=oi, out_scores=osc)
            assert np.array_equal(host_u32(oi), want_ids), (kind, k, candidates, "device")
            assert_bits_equal(osc.cpu().numpy(), want_sc, f"{kind} topk_rescored({k}, {candidates}), device outputs")
    with pytest.raises(qa.EncodingError):
        enc.topk_rescored(q, orig, q_f32, 11, 10, largest)  # k > candidates
    with pytest.raises(qa.EncodingError):
        enc.topk_rescored(q, orig, q_f32, 10, 1025, largest)
    other = D.L1 if dist != D.L1 else D.Dot
    for bad_data, bad_vp in ((data[:-1], qa.VectorParameters(dim, n - 1, dist, invert)),
                             (np.ascontiguousarray(data[:, :-1]), qa.VectorParameters(dim - 1, n, dist, invert)),
                             (data, qa.VectorParameters(dim, n, other, invert)),
                             (data, qa.VectorParameters(dim, n, dist, not invert))):
        bad = qa.OriginalVectors.from_data(bad_data, bad_vp)
        with pytest.raises(qa.EncodingError) as e:
            enc.topk_rescored(q, bad, q_f32[: bad_vp.dim], 10, 100, largest)
        assert "do not belong" in str(e.value)


@pytest.mark.parametrize("kind", ["u8", "pq", "bin"])
@pytest.mark.parametrize("n", [700, 5])
def test_small_stores_give_the_exact_brute_force_topk(kind, n):
    """count <= candidates: every row is a candidate, so the result is the exact top-k of the whole data set."""
    rng = np.random.default_rng(n)
    dim = 64
    data = tie_data(rng, n, dim) if n > 8 else rng.standard_normal((n, dim)).astype(np.float32)
    for dist, invert, largest in ((D.Dot, False, True), (D.L2, False, False)):
        vp = qa.VectorParameters(dim, n, dist, invert)
        enc = make_store(kind, data, vp, rng)
        orig = qa.OriginalVectors.from_data(data, vp)
        q_f32 = rng.standard_normal(dim).astype(np.float32)
        q = enc.encode_query(q_f32)
        for k, candidates in ((10, 1024), (30, 700), (1024, 1024)):
            want_ids, want_sc = topk_want(exact(dist, invert, q_f32, data, np.arange(n)), k, largest)
            got_ids, got_sc = enc.topk_rescored(q, orig, q_f32, k, candidates, largest)
            assert np.array_equal(got_ids, want_ids), (kind, n, k)
            assert_bits_equal(got_sc, want_sc, f"{kind} brute force n={n} k={k}")
            if n < k:
                assert np.all(got_ids[n:] == PAD) and np.all(got_sc[n:] == (-np.inf if largest else np.inf))


@pytest.mark.parametrize("kind", ["u8", "pq", "bin"])
def test_topk_batch_rescored_is_the_single_call_row_by_row(kind):
    rng = np.random.default_rng(8)
    n, dim = 40_000, 64
    data = tie_data(rng, n, dim)
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    enc = make_store(kind, data, vp, rng)
    orig = qa.OriginalVectors.from_data(data, vp)
    for nq in (1, 3, 64, 257):
        queries = rng.standard_normal((nq, dim)).astype(np.float32)
        batch = enc.encode_query_batch(queries)
        k, candidates = (10, 100) if nq != 3 else (30, 1024)
        got_ids, got_sc = enc.topk_batch_rescored(batch, orig, queries, k, candidates, True)
        oi, osc = torch.empty((nq, k), dtype=torch.int32, device="cuda"), torch.empty((nq, k), device="cuda")
        enc.topk_batch_rescored(batch, orig, torch.from_numpy(queries).cuda(), k, candidates, True, out_ids=oi, out_scores=osc)
        for j in range(nq):
            one_ids, one_sc = enc.topk_rescored(enc.encode_query(queries[j]), orig, queries[j], k, candidates, True)
            assert np.array_equal(got_ids[j], one_ids), (kind, nq, j)
            assert_bits_equal(got_sc[j], one_sc, f"{kind} batch of {nq}, query {j}")
            assert np.array_equal(host_u32(oi)[j], one_ids)
            assert_bits_equal(osc.cpu().numpy()[j], one_sc, f"{kind} batch of {nq}, query {j}, device outputs")
    with pytest.raises(qa.EncodingError):
        enc.topk_batch_rescored(batch, orig, queries[:-1], 10, 100, True)


# ------------------------------------------------------------------------------------------------ 7. borrowed originals
def test_borrowed_and_copied_originals_give_identical_bits():
    rng = np.random.default_rng(21)
    n, dim = 5000, 131
    data = rng.standard_normal((n, dim)).astype(np.float32)
    vp = qa.VectorParameters(dim, n, D.L2, False)
    dev = torch.from_numpy(data).cuda()
    copied = qa.OriginalVectors.from_data(data, vp)
    copied_from_dev = qa.OriginalVectors.from_data(dev, vp)
    borrowed = qa.OriginalVectors.from_data(dev, vp, borrow=True)
    assert borrowed._keep is dev
    q = rng.standard_normal(dim).astype(np.float32)
    ids = rng.integers(0, n, 700).astype(np.uint32)
    want = exact(D.L2, False, q, data, ids)
    for o in (copied, copied_from_dev, borrowed):
        assert_bits_equal(o.score_ids(q, ids), want, "copied / borrowed")
        assert np.array_equal(o.rerank(q, ids, 20, False)[0], copied.rerank(q, ids, 20, False)[0])
    # the borrowed handle reads the caller's memory: a changed row is seen
    dev[int(ids[0])] += 1.0
    torch.cuda.synchronize()
    changed = data.copy()
    changed[int(ids[0])] += np.float32(1.0)
    assert_bits_equal(borrowed.score_ids(q, ids[:1]), exact(D.L2, False, q, changed, ids[:1]), "borrowed memory is read in place")
    assert_bits_equal(copied_from_dev.score_ids(q, ids[:1]), want[:1], "a copy is not")
    with pytest.raises(qa.EncodingError):
        qa.OriginalVectors.from_data(data, vp, borrow=True)
    p = borrowed.get_parameters()
    assert (p.dim, p.count, p.distance_type, p.invert) == (dim, n, D.L2, False)


# ------------------------------------------------------------------------------------------------ 8. monotonicity
def protocol_mixture(rows, dim, queries, seed):
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import ann_protocol

    data, qs = ann_protocol.mixture(rows, dim, queries, seed, torch.device("cpu"))
    return data, qs, ann_protocol


@pytest.mark.parametrize("metric", ["angular", "euclidean"])
def test_rescoring_never_loses_a_true_neighbour(metric):
    """Exact re-ranking of a superset of topk(10)'s rows cannot lose a true neighbour, so per query and quantizer the
    number of true top-10 ids in topk_rescored(10, 100) is >= that in topk(10); for the binary store the sum over the
    queries is strictly greater.  Data: tools/ann_protocol.mixture(20000, 64, 50 queries, seed 2090) drawn with the CPU
    generator.  Chosen after confirming on the CPU (oracle binary scores + numpy) that on this data binary topk(10)
    leaves true neighbours outside its top 10 but inside its top 100: angular 228 of the 500 true neighbours are in
    its top 10 and 453 in its top 100; euclidean 178 and 409."""
    rows, dim, nq = 20_000, 64, 50
    data_t, queries_t, ap = protocol_mixture(rows, dim, nq, 2090)
    angular = metric == "angular"
    if angular:
        data_t, queries_t = ap.cosine_preprocess(data_t), ap.cosine_preprocess(queries_t)
    data, queries = data_t.numpy(), queries_t.numpy()
    dist, largest = (D.Dot, True) if angular else (D.L2, False)
    vp = qa.VectorParameters(dim, rows, dist, False)
    truth = [set(int(i) for i in topk_want(exact(dist, False, q, data, np.arange(rows)), 10, largest)[0]) for q in queries]
    orig = qa.OriginalVectors.from_data(torch.from_numpy(data).cuda(), vp, borrow=True)
    rng = np.random.default_rng(1)
    for kind in ("u8", "pq", "bin"):
        enc = qa.EncodedVectorsPQ.encode(data, vp, 8) if kind == "pq" else make_store(kind, data, vp, rng)
        plain = rescored = 0
        for j, q_f32 in enumerate(queries):
            q = enc.encode_query(q_f32)
            a = len(truth[j] & set(int(i) for i in enc.topk(q, 10, largest)[0]))
            b = len(truth[j] & set(int(i) for i in enc.topk_rescored(q, orig, q_f32, 10, 100, largest)[0]))
            assert b >= a, (kind, j, a, b)
            plain += a
            rescored += b
        print(f"{metric} {kind}: true neighbours in topk(10) {plain}/500, in topk_rescored(10, 100) {rescored}/500")
        if kind == "bin":
            assert rescored > plain, (plain, rescored)


# ------------------------------------------------------------------------------------------------ 9. threads
def test_two_threads_rescoring_on_one_handle_pair():
    rng = np.random.default_rng(30)
    n, dim, nthreads = 100_000, 96, 2
    data = rng.standard_normal((n, dim)).astype(np.float32)
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    enc = qa.EncodedVectorsU8.encode(data, vp)
    orig = qa.OriginalVectors.from_data(data, vp)
    queries = rng.standard_normal((nthreads, dim)).astype(np.float32)
    want = [enc.topk_rescored(enc.encode_query(q), orig, q, 30, 1000, True) for q in queries]
    want_b = enc.topk_batch_rescored(enc.encode_query_batch(queries), orig, queries, 10, 100, True)
    errors = []
    start = threading.Barrier(nthreads)

    def worker(i):
        try:
            stream = torch.cuda.Stream()
            start.wait()
            with torch.cuda.stream(stream):
                for _ in range(20):
                    ids, sc = enc.topk_rescored(enc.encode_query(queries[i]), orig, queries[i], 30, 1000, True)
                    if not (np.array_equal(ids, want[i][0]) and np.array_equal(sc.view(np.uint32), want[i][1].view(np.uint32))):
                        errors.append(f"thread {i}: topk_rescored differs")
                    ids, sc = enc.topk_batch_rescored(enc.encode_query_batch(queries), orig, queries, 10, 100, True)
                    if not (np.array_equal(ids, want_b[0]) and np.array_equal(sc.view(np.uint32), want_b[1].view(np.uint32))):
                        errors.append(f"thread {i}: topk_batch_rescored differs")
        except Exception as e:  # pragma: no cover
            errors.append(f"thread {i}: {e!r}")

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(nthreads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:3]
