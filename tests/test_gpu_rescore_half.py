"""Rescoring with f16 / bf16 originals (qamd_f32_from_data_typed) against the oracle's restatement of
DistanceType::distance (encoded_vectors.rs:37-45; oracle qo_metric_f32) applied to the rows WIDENED to f32: f16 by
`astype(np.float32)`, bf16 by `(bits.astype(np.uint32) << 16).view(np.float32)`.  Widening is exact, so every comparison
is bit-exact; a NaN is checked as a NaN, never by its bit pattern, and -0.0 orders as +0.0 (tests/util.py topk_want)."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from util import bits, topk_want

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
torch = pytest.importorskip("torch")
from oracle import qoracle as qo  # noqa: E402

D = qa.DistanceType
PAD = 0xFFFFFFFF
METRICS = [(D.Dot, False), (D.Dot, True), (D.L1, False), (D.L1, True), (D.L2, False), (D.L2, True)]
KINDS = ["f16", "bf16"]


def assert_same(got, want, what=""):
    """Bit-equal, except that where `want` is NaN `got` must be a NaN of any pattern."""
    got, want = np.asarray(got, dtype=np.float32).ravel(), np.asarray(want, dtype=np.float32).ravel()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaNs at {np.flatnonzero(np.isnan(got) != nan)[:5]}"
    bad = np.flatnonzero((bits(got) != bits(want)) & ~nan)
    assert bad.size == 0, f"{what}: {bad.size}/{got.size} differ; first at {bad[0]}: got {got[bad[0]]!r} want {want[bad[0]]!r}"


def to_store(f32, kind):
    """f32 values as the store's numpy form: float16 (numpy's round to nearest even), or bf16 bit patterns in uint16
    (the integer round to nearest even; finite inputs)."""
    f32 = np.ascontiguousarray(f32, dtype=np.float32)
    if kind == "f16":
        with np.errstate(over="ignore"):
            return f32.astype(np.float16)
    u = f32.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def widen(stored, kind):
    if kind == "f16":
        return stored.astype(np.float32)
    return (stored.astype(np.uint32) << 16).view(np.float32)


def as_torch(stored, kind):
    if kind == "f16":
        return torch.from_numpy(stored)
    return torch.from_numpy(stored.view(np.int16)).view(torch.bfloat16)


def exact(dist, invert, q, rows_f32, ids):
    """qo_metric_f32(dist, q, rows_f32[id]) for every id, sign flipped for invert."""
    q = np.ascontiguousarray(q, dtype=np.float32)
    rows_f32 = np.ascontiguousarray(rows_f32, dtype=np.float32)
    fn, dim, base, qp = qo.lib().qo_metric_f32, rows_f32.shape[1], rows_f32.ctypes.data, q.ctypes.data
    out = np.array([fn(int(dist), qp, base + int(i) * dim * 4, dim) for i in ids], dtype=np.float32)
    return -out if invert else out


def want_rerank(dist, invert, q, rows_f32, ids, k, largest):
    ids = np.asarray(ids, dtype=np.uint32).ravel()
    valid = np.sort(ids[ids != PAD], kind="stable")
    pos, sc = topk_want(exact(dist, invert, q, rows_f32, valid), k, largest)
    out = np.full(k, PAD, dtype=np.uint32)
    out[pos != PAD] = valid[pos[pos != PAD]]
    return out, sc


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def host_u32(t):
    return t.cpu().numpy().view(np.uint32)


def special_store(rng, n, dim, kind):
    """(stored, widened f32): normal rows plus +-0, subnormals of the store type, its largest values."""
    stored = to_store(rng.standard_normal((n, dim)), kind)
    alt = np.arange(dim) % 2 == 0
    if kind == "f16":
        stored[0] = np.where(alt, 0.0, -0.0).astype(np.float16)
        stored[1] = (rng.integers(1, 1024, dim) * np.float64(2.0 ** -24)).astype(np.float16)  # f16 subnormals
        stored[1, 0] = np.float16(6e-8)  # the smallest one, 2^-24
        stored[2] = np.float16(65504.0)
        stored[3] = np.where(alt, 65504.0, -65504.0).astype(np.float16)
        stored[4, ::3] = np.float16(6e-8)
        assert stored[1].view(np.uint16).max() < 0x0400 and stored[1, 0].view(np.uint16) == 1
    else:
        stored[0] = np.where(alt, 0x0000, 0x8000).astype(np.uint16)
        stored[1] = rng.integers(1, 0x80, dim).astype(np.uint16)  # exponent 0: f32 subnormals
        stored[1, ::2] |= 0x8000
        big = np.float32(np.finfo(np.float32).max / dim) * rng.uniform(0.5, 1.0, dim).astype(np.float32)
        stored[2] = (big.view(np.uint32) >> 16).astype(np.uint16)  # truncated: stays below f32::MAX / dim
        stored[3] = stored[2] | 0x8000
        stored[4, ::3] = 0x0001
    return stored, widen(stored, kind)


def special_query(rng, dim):
    q = rng.standard_normal(dim).astype(np.float32)
    q[::5] = np.float32(3e-41)
    q[1::7] = -0.0
    return q


def make(stored, kind, vp, **kw):
    return qa.OriginalVectors.from_data(stored, vp, dtype=kind, **kw)


# ------------------------------------------------------------------------------------------------ 1. score_ids
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [1, 2, 3, 63, 64, 65, 127, 128, 768, 1536, 4099])
@pytest.mark.parametrize("dist,invert", METRICS)
def test_score_ids_is_the_oracle_metric_of_the_widened_rows(dim, dist, invert, kind):
    rng = np.random.default_rng(dim * 10 + int(dist) * 2 + invert)
    n = 300
    stored, rows = special_store(rng, n, dim, kind)
    orig = make(stored, kind, qa.VectorParameters(dim, n, dist, invert))
    assert orig.dtype == kind
    ids = np.concatenate([np.arange(8), rng.integers(0, n, 192), [n - 1]]).astype(np.uint32)
    for q in (rng.standard_normal(dim).astype(np.float32), special_query(rng, dim)):
        want = exact(dist, invert, q, rows, ids)
        assert_same(orig.score_ids(q, ids), want, "host ids, host out")
        out = torch.empty(ids.size, device="cuda")
        orig.score_ids(q, ids, out=out)
        assert_same(out.cpu().numpy(), want, "host ids, device out")
        assert_same(orig.score_ids(q, dev_u32(ids)), want, "device ids, host out")
        out = torch.empty(ids.size, device="cuda")
        orig.score_ids(torch.from_numpy(q).cuda(), dev_u32(ids), out=out)
        torch.cuda.synchronize()
        assert_same(out.cpu().numpy(), want, "device query, ids and out")
    # a long host list leaves the mapped scratch (more than 1024 ids)
    many = rng.integers(0, n, 1500).astype(np.uint32)
    assert_same(orig.score_ids(q, many), exact(dist, invert, q, rows, many), "1500 host ids")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [20, 21])
def test_score_ids_out_of_range(kind, dim):
    rng = np.random.default_rng(5)
    stored = to_store(rng.standard_normal((50, dim)), kind)
    orig = make(stored, kind, qa.VectorParameters(dim, 50, D.L2, False))
    q = rng.standard_normal(dim).astype(np.float32)
    with pytest.raises(IndexError):
        orig.score_ids(q, np.array([1, 50], dtype=np.uint32))
    ids = np.array([3, 50, 7, PAD, 49], dtype=np.uint32)
    got = orig.score_ids(q, dev_u32(ids))
    assert np.isnan(got[1]) and np.isnan(got[3])
    keep = [0, 2, 4]
    assert_same(got[keep], exact(D.L2, False, q, widen(stored, kind), ids[keep]), "in-range device ids beside bad ones")
    with pytest.raises(qa.EncodingError):
        orig.score_ids(q[:dim - 1], ids[:1])


# ------------------------------------------------------------------------------------------------ 2. score_ids_batch
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dist,invert", [(D.Dot, False), (D.L1, True), (D.L2, False)])
@pytest.mark.parametrize("dim", [3, 65, 130, 768])
def test_score_ids_batch_is_score_ids_per_list(dim, dist, invert, kind):
    rng = np.random.default_rng(dim + int(dist))
    n = 400
    stored, rows = special_store(rng, n, dim, kind)
    orig = make(stored, kind, qa.VectorParameters(dim, n, dist, invert))
    # ragged, empty lists, lists longer than a workgroup's 256 pairs; the list of 300 holds whole waves of one list
    # (the wave-uniform query path), the short ones share waves (the straddling path)
    lens = [3, 0, 70, 1, 0, 300, 64, 130, 0]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    ids = rng.integers(0, n, int(offs[-1])).astype(np.uint32)
    queries = rng.standard_normal((len(lens), dim)).astype(np.float32)
    queries[2] = special_query(rng, dim)
    want = np.concatenate([exact(dist, invert, queries[l], rows, ids[offs[l]:offs[l + 1]]) for l in range(len(lens))])
    assert_same(orig.score_ids_batch(queries, offs, ids), want, "host lists, host out")
    out = torch.empty(ids.size, device="cuda")
    orig.score_ids_batch(queries, offs, ids, out=out)
    assert_same(out.cpu().numpy(), want, "host lists, device out")
    out = torch.empty(ids.size, device="cuda")
    orig.score_ids_batch(torch.from_numpy(queries).cuda(), dev_u32(offs), dev_u32(ids), out=out)
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy(), want, "device lists, device out")
    small_offs = np.array([0, 2, 2, 5], dtype=np.uint32)
    want = np.concatenate([exact(dist, invert, queries[l], rows, ids[small_offs[l]:small_offs[l + 1]]) for l in range(3)])
    assert_same(orig.score_ids_batch(queries[:3], small_offs, ids[:5]), want, "small burst")
    with pytest.raises(IndexError):
        orig.score_ids_batch(queries[:1], np.array([0, 1], dtype=np.uint32), np.array([n], dtype=np.uint32))


# ------------------------------------------------------------------------------------------------ 3. rerank
def tie_store(rng, n, dim, kind):
    """Rows with engineered exact ties: every row of the second half repeats a row of the first half."""
    stored = to_store(rng.standard_normal((n, dim)), kind)
    stored[n // 2:] = stored[rng.integers(0, n // 2, n - n // 2)]
    return stored, widen(stored, kind)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("largest", [False, True])
@pytest.mark.parametrize("k", [1, 10, 1024])
def test_rerank_is_topk_want_of_the_oracle_scores(k, largest, kind):
    rng = np.random.default_rng(k + largest)
    n = 9000
    for (dist, invert), dim in (((D.Dot, False), 24), ((D.L2, True), 25)):
        stored, rows = tie_store(rng, n, dim, kind)
        orig = make(stored, kind, qa.VectorParameters(dim, n, dist, invert))
        q = rng.standard_normal(dim).astype(np.float32)
        for n_ids in sorted({k, 1000, 8192}):
            ids = rng.permutation(n)[:n_ids].astype(np.uint32)
            want_ids, want_sc = want_rerank(dist, invert, q, rows, ids, k, largest)
            got_ids, got_sc = orig.rerank(q, ids, k, largest)
            assert np.array_equal(got_ids, want_ids), (dist, n_ids)
            assert_same(got_sc, want_sc, f"rerank scores {dist} {n_ids}")
            oi, osc = torch.empty(k, dtype=torch.int32, device="cuda"), torch.empty(k, device="cuda")
            orig.rerank(torch.from_numpy(q).cuda(), dev_u32(ids), k, largest, out_ids=oi, out_scores=osc)
            torch.cuda.synchronize()
            assert np.array_equal(host_u32(oi), want_ids)
            assert_same(osc.cpu().numpy(), want_sc, "rerank, device buffers")
            padded = ids.copy()  # the padding id is skipped wherever it stands
            padded[rng.integers(0, n_ids, max(1, n_ids // 7))] = PAD
            want_ids, want_sc = want_rerank(dist, invert, q, rows, padded, k, largest)
            got_ids, got_sc = orig.rerank(q, padded, k, largest)
            assert np.array_equal(got_ids, want_ids), ("padded", dist, n_ids)
            assert_same(got_sc, want_sc, "rerank of a padded list")
        with pytest.raises(qa.EncodingError):
            orig.rerank(q, np.zeros(8193, dtype=np.uint32), k, largest)
    with pytest.raises(qa.EncodingError):
        orig.rerank(q, ids, 1025, largest)
    with pytest.raises(IndexError):
        orig.rerank(q, np.array([0, n], dtype=np.uint32), 1, largest)


@pytest.mark.parametrize("kind", KINDS)
def test_rerank_ties_go_to_the_lower_id_and_short_lists_are_padded(kind):
    rng = np.random.default_rng(11)
    n, dim = 64, 7
    stored = to_store(rng.standard_normal((n, dim)), kind)
    stored[40] = stored[5]
    stored[41] = stored[5]
    rows = widen(stored, kind)
    orig = make(stored, kind, qa.VectorParameters(dim, n, D.Dot, False))
    q = rows[5].copy()
    ids = np.array([41, 9, 5, PAD, 40, 12], dtype=np.uint32)
    for largest in (True, False):
        got_ids, got_sc = orig.rerank(q, ids, 8, largest)
        want_ids, want_sc = want_rerank(D.Dot, False, q, rows, ids, 8, largest)
        assert np.array_equal(got_ids, want_ids)
        assert_same(got_sc, want_sc, "ties and padding")
        assert [int(i) for i in got_ids if i in (5, 40, 41)] == [5, 40, 41]
        assert list(got_ids[5:]) == [PAD] * 3 and np.all(np.isinf(got_sc[5:]))
    got_ids, _ = orig.rerank(q, np.array([PAD, PAD], dtype=np.uint32), 3, True)
    assert list(got_ids) == [PAD] * 3


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("largest", [False, True])
def test_rerank_batch(largest, kind):
    rng = np.random.default_rng(3 + largest)
    n = 3000
    for (dist, invert), dim, nq, n_ids, k in (((D.L2, False), 65, 5, 100, 10), ((D.Dot, True), 66, 3, 1000, 1024),
                                               ((D.L1, False), 65, 70, 37, 1)):
        stored, rows = tie_store(rng, n, dim, kind)
        orig = make(stored, kind, qa.VectorParameters(dim, n, dist, invert))
        queries = rng.standard_normal((nq, dim)).astype(np.float32)
        ids = np.stack([rng.permutation(n)[:n_ids] for _ in range(nq)]).astype(np.uint32)
        ids[0, ::9] = PAD
        got_ids, got_sc = orig.rerank_batch(queries, ids, k, largest)
        oi, osc = torch.empty((nq, k), dtype=torch.int32, device="cuda"), torch.empty((nq, k), device="cuda")
        orig.rerank_batch(torch.from_numpy(queries).cuda(), dev_u32(ids), k, largest, out_ids=oi, out_scores=osc)
        torch.cuda.synchronize()
        for j in range(nq):
            want_ids, want_sc = want_rerank(dist, invert, queries[j], rows, ids[j], k, largest)
            assert np.array_equal(got_ids[j], want_ids), (dist, j)
            assert_same(got_sc[j], want_sc, f"rerank_batch query {j}")
            assert np.array_equal(host_u32(oi)[j], want_ids)
            assert_same(osc.cpu().numpy()[j], want_sc, f"rerank_batch query {j}, device buffers")


# ------------------------------------------------------------------------------------------------ 4. narrowing
def narrowing_inputs(rng, n, dim):
    """f32 rows whose narrowing rounds: random values, exact halfway cases of both types (to even, both ways), values
    that round up to inf and values just below that, subnormal results, +-0."""
    data = (rng.standard_normal((n, dim)) * np.exp(rng.uniform(-20, 12, (n, dim)))).astype(np.float32)
    flat = data.reshape(-1)
    u = rng.integers(0x30000000, 0x4F000000, 4096).astype(np.uint32)
    halves = [(u & 0xFFFFE000) | 0x1000,  # f16: the 13 dropped bits are 1000...0 -> tie, even or odd kept bit
              (u & 0xFFFF0000) | 0x8000,  # bf16: the 16 dropped bits are 1000...0
              (u & 0xFFFFE000) | 0x1001, (u & 0xFFFF0000) | 0x7FFF]
    special = np.concatenate([h.astype(np.uint32).view(np.float32) for h in halves] + [np.array(
        [65504.0, 65519.996, 65520.0, 65536.0, -65520.0, 1e6, -1e30, 3.3895314e38, 3.4028235e38, -3.4028235e38, 3.39e38,
         0.0, -0.0, 6e-8, 2.98e-8, 2.9802322e-8, 2.9802326e-8, 8.9e-8, 1e-40, -1e-40, 6.1e-5, 6.0975552e-5, 1e-45],
        dtype=np.float32)])
    sign = np.where(rng.random(special.size) < 0.5, -1.0, 1.0).astype(np.float32)
    special = special * sign
    assert special.size <= flat.size
    flat[rng.permutation(flat.size)[:special.size]] = special
    return data


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [96, 97, 6])
@pytest.mark.parametrize("where", ["host", "device", "device, 4-byte aligned"])
def test_narrowing_by_the_library_is_round_to_nearest_even(kind, dim, where):
    rng = np.random.default_rng(dim)
    n = 3001
    data = narrowing_inputs(rng, n, dim)
    stored = to_store(data, kind)  # f16: numpy's astype; bf16: (u + 0x7FFF + ((u >> 16) & 1)) >> 16, all inputs finite
    rows = widen(stored, kind)
    assert np.isfinite(data).all() and np.isinf(rows).any()  # some round to inf
    if where == "host":
        src = data
    elif where == "device":
        src = torch.from_numpy(data).cuda()
    else:  # one f32 into an allocation: no 16-byte loads
        flat = torch.empty(n * dim + 1, device="cuda")
        flat[1:] = torch.from_numpy(data).reshape(-1)
        src = flat[1:].view(n, dim)
        assert src.data_ptr() % 16 == 4
    # every value read back on its own: as a store of dim 1, Dot with the query [1.0] is +0.0 + 1.0 * value
    one = qa.VectorParameters(1, n * dim, D.Dot, False)
    narrowed = make(src.reshape(-1, 1), kind, one)  # f32 in, narrowed on the device
    given = make(stored.reshape(-1, 1), kind, one)  # already narrow
    assert narrowed.dtype == given.dtype == kind
    ids = np.arange(n * dim, dtype=np.uint32)
    q1 = np.ones(1, dtype=np.float32)
    got = narrowed.score_ids(q1, ids)
    assert_same(got, given.score_ids(q1, ids), "narrowed by the library vs given narrow")
    assert_same(got, exact(D.Dot, False, q1, rows.reshape(-1, 1), ids), "narrowed by the library vs the oracle on the widened values")
    # and as rows
    vp = qa.VectorParameters(dim, n, D.L1, False)
    q = rng.standard_normal(dim).astype(np.float32)
    ids = np.arange(n, dtype=np.uint32)
    got = make(src, kind, vp).score_ids(q, ids)
    assert_same(got, make(stored, kind, vp).score_ids(q, ids), "rows: narrowed vs given")
    assert_same(got, exact(D.L1, False, q, rows, ids), "rows: narrowed vs oracle")


@pytest.mark.parametrize("kind", KINDS)
def test_narrowing_keeps_nan_and_inf(kind):
    data = np.zeros((4, 8), dtype=np.float32)
    data[0, 0], data[1, 1], data[2, 2] = np.nan, np.inf, -np.inf
    data[3, 3] = np.array([0x7F800001], dtype=np.uint32).view(np.float32)[0]  # a NaN whose payload is in the low bits
    orig = make(data, kind, qa.VectorParameters(8, 4, D.L1, False))
    got = orig.score_ids(np.zeros(8, dtype=np.float32), np.arange(4, dtype=np.uint32))
    assert np.isnan(got[0]) and got[1] == np.inf and got[2] == np.inf and np.isnan(got[3])


def test_narrowing_in_staged_pieces():
    """Host f32 data larger than one staging piece is narrowed piece by piece: QAMD_DEV_STAGE_BYTES (read by the
    developer build of the library only, once per process) = 64 KiB gives pieces of 496 rows of 33 values."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dev_lib = os.path.join(root, "tools", "lib", "libquantization_amd_dev.so")
    assert os.path.exists(dev_lib), "the developer library is built with the product one (make -C quantization_amd/csrc)"
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import numpy as np, quantization_amd as qa\n"
        "rng = np.random.default_rng(1); n, dim = 3001, 33\n"
        "data = rng.standard_normal((n, dim)).astype(np.float32)\n"
        "vp = qa.VectorParameters(dim, n, qa.DistanceType.L2, False)\n"
        "q = rng.standard_normal(dim).astype(np.float32); ids = np.arange(n, dtype=np.uint32)\n"
        "for kind, half in (('f16', data.astype(np.float16)), ('bf16', None)):\n"
        "    if half is None:\n"
        "        u = data.view(np.uint32).astype(np.uint64)\n"
        "        half = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)\n"
        "    a = qa.OriginalVectors.from_data(data, vp, dtype=kind).score_ids(q, ids)\n"
        "    b = qa.OriginalVectors.from_data(half, vp, dtype=kind).score_ids(q, ids)\n"
        "    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), kind\n"
        "print('pieces OK')\n" % root)
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
    env.update(QAMD_DEV_STAGE_BYTES=str(64 * 1024), QAMD_LIB_PATH=dev_lib)
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "pieces OK" in res.stdout, (res.stdout + res.stderr)[-2000:]


# ------------------------------------------------------------------------------------------------ 5. the fused calls
def make_quantized(which, data, vp, rng):
    if which == "u8":
        return qa.EncodedVectorsU8.encode(data, vp)
    if which == "pq":
        cen = rng.standard_normal((256, vp.dim)).astype(np.float32)
        return qa.EncodedVectorsPQ.encode(data, vp, 8, centroids=cen)
    return qa.EncodedVectorsBin.encode(data, vp)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("which", ["u8", "pq", "bin"])
def test_fused_calls_equal_topk_then_rerank_on_the_half_store(which, kind):
    rng = np.random.default_rng(17)
    n, dim = 6000, 64
    data = rng.standard_normal((n, dim)).astype(np.float32)
    data[n // 2:] = data[rng.integers(0, n // 2, n - n // 2)]  # exact ties
    for dist, largest in ((D.Dot, True), (D.L2, False)):
        vp = qa.VectorParameters(dim, n, dist, False)
        enc = make_quantized(which, data, vp, rng)
        orig = make(data, kind, vp)  # narrowed by the library
        rows = widen(to_store(data, kind), kind)
        queries = rng.standard_normal((5, dim)).astype(np.float32)
        for k, candidates in ((1, 1), (10, 100), (30, 1024), (1024, 1024)):
            q = enc.encode_query(queries[0])
            cand, _ = enc.topk(q, candidates, largest)
            via_ids, via_sc = orig.rerank(queries[0], cand, k, largest)
            want_ids, want_sc = want_rerank(dist, False, queries[0], rows, cand, k, largest)
            got_ids, got_sc = enc.topk_rescored(q, orig, queries[0], k, candidates, largest)
            assert np.array_equal(got_ids, via_ids) and np.array_equal(got_ids, want_ids), (which, k, candidates)
            assert_same(got_sc, via_sc, "fused vs rerank")
            assert_same(got_sc, want_sc, "fused vs oracle")
            oi, osc = torch.empty(k, dtype=torch.int32, device="cuda"), torch.empty(k, device="cuda")
            enc.topk_rescored(q, orig, torch.from_numpy(queries[0]).cuda(), k, candidates, largest, out_ids=oi, out_scores=osc)
            assert np.array_equal(host_u32(oi), want_ids)
            assert_same(osc.cpu().numpy(), want_sc, "fused, device outputs")
        batch = enc.encode_query_batch(queries)
        got_ids, got_sc = enc.topk_batch_rescored(batch, orig, queries, 10, 100, largest)
        cand, _ = enc.topk_batch(batch, 100, largest)
        via_ids, via_sc = orig.rerank_batch(queries, cand, 10, largest)
        assert np.array_equal(got_ids, via_ids)
        assert_same(got_sc, via_sc, "fused batch vs rerank_batch")
        for j in range(len(queries)):
            want_ids, want_sc = want_rerank(dist, False, queries[j], rows, cand[j], 10, largest)
            assert np.array_equal(got_ids[j], want_ids), (which, j)
            assert_same(got_sc[j], want_sc, f"fused batch vs oracle, query {j}")
    # a store that does not belong is refused, whatever its element type
    other = D.L1
    for bad_data, bad_vp in ((data[:-1], qa.VectorParameters(dim, n - 1, dist, False)),
                             (np.ascontiguousarray(data[:, :-1]), qa.VectorParameters(dim - 1, n, dist, False)),
                             (data, qa.VectorParameters(dim, n, other, False)),
                             (data, qa.VectorParameters(dim, n, dist, True))):
        bad = make(bad_data, kind, bad_vp)
        with pytest.raises(qa.EncodingError) as e:
            enc.topk_rescored(q, bad, queries[0][: bad_vp.dim], 10, 100, largest)
        assert "do not belong" in str(e.value)
    if torch.cuda.device_count() > 1:
        with torch.cuda.device(1):
            elsewhere = make(torch.from_numpy(data).to("cuda:1"), kind, vp)
        with pytest.raises((qa.EncodingError, ValueError)):
            enc.topk_rescored(q, elsewhere, queries[0], 10, 100, largest)


# ------------------------------------------------------------------------------------------------ 6. borrowed originals
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim", [131, 132])
def test_a_borrowed_half_tensor_is_read_in_place(kind, dim):
    rng = np.random.default_rng(21)
    n = 5000
    stored = to_store(rng.standard_normal((n, dim)), kind)
    rows = widen(stored, kind)
    vp = qa.VectorParameters(dim, n, D.L2, False)
    dev = as_torch(stored, kind).cuda()
    assert dev.dtype == (torch.float16 if kind == "f16" else torch.bfloat16)
    copied = make(stored, kind, vp)
    copied_from_dev = make(dev, kind, vp)
    borrowed = make(dev, kind, vp, borrow=True)
    assert borrowed._keep is dev
    assert borrowed.dtype == copied.dtype == copied_from_dev.dtype == kind
    q = rng.standard_normal(dim).astype(np.float32)
    ids = rng.integers(0, n, 700).astype(np.uint32)
    want = exact(D.L2, False, q, rows, ids)
    for o in (copied, copied_from_dev, borrowed):
        assert_same(o.score_ids(q, ids), want, "copied / borrowed")
        assert np.array_equal(o.rerank(q, ids, 20, False)[0], copied.rerank(q, ids, 20, False)[0])
    # the borrowed handle reads the caller's memory: a changed row is seen
    dev[int(ids[0])] = 2.0
    torch.cuda.synchronize()
    changed = rows.copy()
    changed[int(ids[0])] = np.float32(2.0)
    assert_same(borrowed.score_ids(q, ids[:1]), exact(D.L2, False, q, changed, ids[:1]), "borrowed memory is read in place")
    assert_same(copied_from_dev.score_ids(q, ids[:1]), want[:1], "a copy is not")
    # a view that starts one element into a buffer is only 2-byte aligned: still legal to borrow
    flat = torch.empty(n * dim + 1, dtype=dev.dtype, device="cuda")
    flat[1:] = dev.reshape(-1)
    odd = flat[1:].view(n, dim)
    assert odd.data_ptr() % 4 == 2 and odd.is_contiguous()
    assert_same(make(odd, kind, vp, borrow=True).score_ids(q, ids), borrowed.score_ids(q, ids), "a 2-byte aligned base")
    # what cannot be borrowed
    with pytest.raises(qa.EncodingError):
        make(stored, kind, vp, borrow=True)  # host memory
    with pytest.raises(ValueError):
        make(dev.float(), kind, vp, borrow=True)  # f32 would have to be narrowed
    with pytest.raises(ValueError):
        make(dev, "bf16" if kind == "f16" else "f16", vp, borrow=True)
    with pytest.raises(ValueError):
        qa.OriginalVectors.from_data(dev, vp, borrow=True)  # dtype=None keeps f32: a half tensor cannot be read in place
    p = borrowed.get_parameters()
    assert (p.dim, p.count, p.distance_type, p.invert) == (dim, n, D.L2, False)


def test_dtype_round_trips_and_the_f32_store_is_unchanged():
    rng = np.random.default_rng(2)
    data = rng.standard_normal((40, 10)).astype(np.float32)
    vp = qa.VectorParameters(10, 40, D.Dot, False)
    q = rng.standard_normal(10).astype(np.float32)
    ids = np.arange(40, dtype=np.uint32)
    plain = qa.OriginalVectors.from_data(data, vp)
    typed = qa.OriginalVectors.from_data(data, vp, dtype="f32")
    assert plain.dtype == typed.dtype == "f32"
    assert_same(plain.score_ids(q, ids), exact(D.Dot, False, q, data, ids), "f32")
    assert_same(typed.score_ids(q, ids), plain.score_ids(q, ids), "dtype='f32' is the f32 store")
    for kind in KINDS:
        assert make(data, kind, vp).dtype == kind
        assert make(torch.from_numpy(data), kind, vp).dtype == kind
        host_half = as_torch(to_store(data, kind), kind)
        assert_same(make(host_half, kind, vp).score_ids(q, ids), make(to_store(data, kind), kind, vp).score_ids(q, ids),
                    "host torch half tensor")


# ------------------------------------------------------------------------------------------------ 7. threads
@pytest.mark.parametrize("kind", KINDS)
def test_two_threads_on_one_half_store(kind):
    rng = np.random.default_rng(30)
    n, dim, nthreads = 20_000, 96, 2
    data = rng.standard_normal((n, dim)).astype(np.float32)
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    enc = qa.EncodedVectorsU8.encode(data, vp)
    orig = make(data, kind, vp)
    queries = rng.standard_normal((nthreads, dim)).astype(np.float32)
    ids = rng.integers(0, n, (nthreads, 2000)).astype(np.uint32)
    want = [enc.topk_rescored(enc.encode_query(q), orig, q, 30, 1000, True) for q in queries]
    want_r = orig.rerank_batch(queries, ids, 10, True)
    errors = []
    start = threading.Barrier(nthreads)

    def worker(i):
        try:
            stream = torch.cuda.Stream()
            start.wait()
            with torch.cuda.stream(stream):
                for _ in range(20):
                    got = enc.topk_rescored(enc.encode_query(queries[i]), orig, queries[i], 30, 1000, True)
                    if not (np.array_equal(got[0], want[i][0]) and np.array_equal(bits(got[1]), bits(want[i][1]))):
                        errors.append(f"thread {i}: topk_rescored differs")
                    got = orig.rerank_batch(queries, ids, 10, True)
                    if not (np.array_equal(got[0], want_r[0]) and np.array_equal(bits(got[1]), bits(want_r[1]))):
                        errors.append(f"thread {i}: rerank_batch differs")
        except Exception as e:  # pragma: no cover
            errors.append(f"thread {i}: {e!r}")

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(nthreads)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[:3]
