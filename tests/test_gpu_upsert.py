"""Upsert: rows of a built store overwritten and appended in place, for the three quantizers and the
originals.

The yardstick is a FRESH handle built in one go over the final data with the same parameters (the streaming encoders with
alpha_offset / centroids given, the binary encoder with lo / hi given, from_data for the originals): rows, every scoring
call, both top-k forms and the saved files must be bit-identical to it, and the rows equal to the CPU restatements
(oracle, tests/two_bit_model.py) under the store's own parameters.  Row counts: 1000 rows, then +1 (inside a 64-row
block), +63 and +24 (across blocks and the 1024-row tile), +3000 (growth), an overwrite of 990..1100 and +120 (past the
4096-row gates of the whole-store PQ scan and the binary matrix-core batches); the large case reserves 40000 rows and
appends up to 33000 across the 4096- and 32768-row gates.  Capacity is checked after every step against the stated rule.
The image checks run in a child process on the developer library (tools/lib), as tests/test_gpu_u8_packed.py does.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import two_bit_model as tb
from util import assert_bits_equal, qa_meta, store_rows

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
from quantization_amd import _lib  # noqa: E402

D = qa.DistanceType
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")

N0 = 1000
# (first_row or None = append, rows)
STEPS = [(None, 1), (None, 63), (None, 24), (None, 3000), (990, 111), (None, 120)]
N_FINAL = N0 + 1 + 63 + 24 + 3000 + 120


class Capacity:
    """The stated rule: builders leave capacity = count; reserve(c) with c > capacity gives c; an upsert that needs more
    than capacity first reserves max(needed, capacity + capacity / 2)."""

    def __init__(self, count):
        self.cap = count

    def upsert(self, end):
        if end > self.cap:
            self.cap = max(end, self.cap + self.cap // 2)


def run_steps(store, data0, more, steps=STEPS):
    """Applies `steps` to `store` (built over data0) taking new rows from `more` in order; returns the final data."""
    final = data0.copy()
    cap = Capacity(len(data0))
    assert store.capacity == cap.cap == store.count
    at = 0
    for first, n in steps:
        rows = more[at:at + n]
        at += n
        if first is None:
            first = len(final)
            store.append(rows)
        else:
            store.upsert(first, rows)
        end = first + n
        if end > len(final):
            final = np.concatenate([final, np.zeros((end - len(final), final.shape[1]), dtype=final.dtype)])
        final[first:end] = rows
        cap.upsert(end)
        assert store.count == len(final) and store.vector_parameters.count == len(final), (first, n)
        assert store.capacity == cap.cap, (first, n, store.capacity, cap.cap)
    return final


def mixed_ids(n, old, rng):
    """ids spanning old and new rows, the first and last of each among them."""
    return np.concatenate([[0, old - 1, old, n - 1], rng.integers(0, n, 60)]).astype(np.uint32)


def same_files(tmp_path, a, b):
    for s, tag in ((a, "a"), (b, "b")):
        s.save(str(tmp_path / f"{tag}.bin"), str(tmp_path / f"{tag}.json"))
    assert (tmp_path / "a.bin").read_bytes() == (tmp_path / "b.bin").read_bytes(), "saved rows"
    assert (tmp_path / "a.json").read_bytes() == (tmp_path / "b.json").read_bytes(), "saved metadata"


def assert_same_store(up, fresh, queries, old, tmp_path, rng, encode=None, up_queries=None, what=""):
    """Every comparison of the module's docstring; `up_queries`: queries encoded on `up` before it was upserted."""
    encode = encode or (lambda s, q: s.encode_query(q))
    n = fresh.count
    assert up.count == n
    assert np.array_equal(np.asarray(up.storage_bytes()), np.asarray(fresh.storage_bytes())), what + " rows"
    ids = mixed_ids(n, old, rng)
    for qi, query in enumerate(queries):
        qu = up_queries[qi] if up_queries is not None else encode(up, query)
        qf = encode(fresh, query)
        assert_bits_equal(up.score_all(qu), fresh.score_all(qf), f"{what} score_all q{qi}")
        assert_bits_equal(up.score_ids(qu, ids), fresh.score_ids(qf, ids), f"{what} score_ids q{qi}")
        iu, su = up.topk(qu, 30)
        jf, sf = fresh.topk(qf, 30)
        assert np.array_equal(iu, jf), f"{what} topk ids q{qi}"
        assert_bits_equal(su, sf, f"{what} topk scores q{qi}")
    for i, j in ((0, n - 1), (old - 1, old), (n - 1, n - 2), (int(ids[5]), int(ids[6]))):
        assert_bits_equal(up.score_internal(i, j), fresh.score_internal(i, j), f"{what} score_internal {i} {j}")
    bu, bf = up.encode_query_batch(queries), fresh.encode_query_batch(queries)
    assert_bits_equal(up.score_batch(bu), fresh.score_batch(bf), what + " score_batch")
    iu, su = up.topk_batch(bu, 30)
    jf, sf = fresh.topk_batch(bf, 30)
    assert np.array_equal(iu, jf), what + " topk_batch ids"
    assert_bits_equal(su, sf, what + " topk_batch scores")
    same_files(tmp_path, up, fresh)


def make(dim, n, seed, scale=1.0):
    rng = np.random.default_rng([dim, n, seed])
    return (rng.standard_normal((n, dim)) * scale).astype(np.float32)


# ------------------------------------------------------------------ u8
def u8_fresh(final, vp, alpha, offset, cut=1500):
    vp = qa.VectorParameters(vp.dim, len(final), vp.distance_type, vp.invert)
    return qa.EncodedVectorsU8.encode_stream(lambda: iter([final[:cut], final[cut:]]), vp, alpha_offset=(alpha, offset))


# the shortest row with a packed image, 9 chunks, the bench's row, no image (7 chunks), the generic kernel (129 chunks)
@pytest.mark.parametrize("dim,dist,lane", [(128, D.Dot, 0), (144, D.L2, 0), (768, D.Dot, 0), (100, D.Dot, 0),
                                           (2064, D.Dot, 0), (128, D.L1, 0), (1536, D.Dot, 1)])
def test_u8_upsert_equals_a_fresh_store(qo, tmp_path, dim, dist, lane):
    rng = np.random.default_rng(dim)
    data0, more, queries = make(dim, N0, 1), make(dim, N_FINAL - N0 + 111, 2, scale=1.3), make(dim, 5, 3)
    up = qa.EncodedVectorsU8.encode(data0, qa.VectorParameters(dim, N0, dist, False))
    md = up.metadata
    alpha, offset = float(md["alpha"]), float(md["offset"])
    bytes_per_row = up.scan_bytes_per_row()
    if lane:
        up.set_lane_mode(1)
    final = run_steps(up, data0, more)  # (scale 1.3: some new values lie outside the interval and saturate)
    assert len(final) == N_FINAL
    md2 = up.metadata
    assert (md2["alpha"], md2["offset"], md2["multiplier"]) == (md["alpha"], md["offset"], md["multiplier"])
    rows, _ = qo.u8_encode_with(final, int(dist), False, alpha, offset)
    got = up.storage_bytes()
    assert np.array_equal(got, rows), "rows are not qo_u8_encode_row of the store's alpha / offset"
    assert got[:, 4:].max() <= 127
    fresh = u8_fresh(final, md["vector_parameters"], alpha, offset)
    if lane:
        fresh.set_lane_mode(1)
    assert up.scan_bytes_per_row() == fresh.scan_bytes_per_row() == bytes_per_row
    assert_same_store(up, fresh, queries, N0, tmp_path, rng, what=f"u8 {dim}")


def test_u8_rows_from_another_producer_stay_without_an_image(qo, tmp_path):
    """A from_rows store that holds a code above 127 has no packed image; after upserts it has none and is correct."""
    dim, dist = 768, D.Dot
    rng = np.random.default_rng(5)
    rows0, _ = store_rows(dim, N0)
    rows0[N0 // 2, 4 + 700] = 200
    md = qa_meta(dim, N0, dist)
    up = qa.EncodedVectorsU8.from_storage(rows0, md)
    more, queries = rng.random((N_FINAL - N0 + 111, dim), dtype=np.float32), rng.random((5, dim), dtype=np.float32)
    final_rows = rows0.copy()
    at = 0
    for first, n in STEPS:
        new = more[at:at + n]
        at += n
        first = len(final_rows) if first is None else first
        up.upsert(first, new)
        enc, _ = qo.u8_encode_with(new, int(dist), False, float(md["alpha"]), 0.0)
        end = first + n
        if end > len(final_rows):
            final_rows = np.concatenate([final_rows, np.zeros((end - len(final_rows), final_rows.shape[1]), dtype=np.uint8)])
        final_rows[first:end] = enc
    assert final_rows[N0 // 2, 4 + 700] == 200  # (row 500 was not overwritten)
    fresh = qa.EncodedVectorsU8.from_storage(final_rows, qa_meta(dim, len(final_rows), dist))
    assert_same_store(up, fresh, queries, N0, tmp_path, rng, what="u8 code 200")


# ------------------------------------------------------------------ the packed image and the planar limit (developer library)
def numpy_blocked(codes, padded_rows):
    """The blocked 7-bit image (u8_internal.hpp) of byte codes [n, 16 rc], padded_rows rows long, as bytes."""
    from test_gpu_u8_packed import numpy_pack

    n = codes.shape[0]
    p = numpy_pack(codes).reshape(n, -1, 16)
    img = np.zeros((padded_rows // 64, p.shape[1], 64, 16), dtype=np.uint8)
    r = np.arange(n)
    img[r // 64, :, r % 64] = p
    return img.reshape(-1)


RANGE_CASES = ((144, 8), (256, 8), (48, 4))  # (dim, bits)


def child_main(out_path):
    import u8_four_bit_model as fm
    from test_gpu_u8_packed import _device_bytes

    L = qa.lib()
    L.qamd_dev_u8_last_scan_packed.restype = C.c_int
    info = {}
    for dim in (128, 768, 100):
        data0, more, queries = make(dim, N0, 1), make(dim, N_FINAL - N0 + 111, 2, scale=1.3), make(dim, 1, 3)
        up = qa.EncodedVectorsU8.encode(data0, qa.VectorParameters(dim, N0, D.Dot, False))
        ptr, chunks, brows = C.c_void_p(), C.c_uint32(), C.c_uint32()
        L.qamd_dev_u8_packed_blocked(up._h, C.byref(ptr), C.byref(chunks), C.byref(brows))
        info[f"{dim}/chunks_before"] = int(chunks.value)
        run_steps(up, data0, more)
        L.qamd_dev_u8_packed_blocked(up._h, C.byref(ptr), C.byref(chunks), C.byref(brows))
        info[f"{dim}/chunks_after"] = int(chunks.value)
        up.score_all(up.encode_query(queries[0]))
        info[f"{dim}/scan_read_image"] = int(L.qamd_dev_u8_last_scan_packed(up._h))
        if chunks.value:
            padded = -(-up.capacity // 1024) * 1024 + 1024
            got = _device_bytes(ptr, padded * chunks.value * 16)
            want = numpy_blocked(up.storage_bytes()[:, 4:], padded)
            info[f"{dim}/image_equal"] = bool(np.array_equal(got, want))  # zero past count, block by block
    # one pack kernel writes both formats at a row base: rows 60..69 of 130 - the end of one block and the start of the
    # next, nothing else touched - at 9 chunks (a rest group), 16 (two extra chunks) and, 4-bit, 3 (the odd last chunk)
    for dim, bits in RANGE_CASES:
        data0 = make(dim, 130, 5)
        up = qa.EncodedVectorsU8.encode(data0, qa.VectorParameters(dim, 130, D.Dot, False), bits=bits)
        before = up.storage_bytes()
        up.upsert(60, make(dim, 10, 6, scale=1.3))
        codes = up.storage_bytes()[:, 4:]
        L.qamd_dev_u8_packed_blocked(up._h, C.byref(ptr), C.byref(chunks), C.byref(brows))
        padded = -(-up.capacity // 1024) * 1024 + 1024
        got = _device_bytes(ptr, padded * chunks.value * 16) if chunks.value else None
        want = numpy_blocked(codes, padded) if bits == 8 else fm.block_image(fm.pack_rows(codes), padded)
        changed = np.flatnonzero((before[:, 4:] != codes).any(axis=1))
        info[f"range/{dim}/{bits}"] = [int(chunks.value), got is not None and bool(np.array_equal(got, want)),
                                       int(changed.min()), int(changed.max())]
    # a PQ store with a planar image may not reach the row count at which a builder would give it none
    dim, chunk = 384, 2
    cen = np.random.default_rng(1).random((256, dim), dtype=np.float32)
    data = make(dim, 6000, 4)
    pq = qa.EncodedVectorsPQ.encode(data[:5000], qa.VectorParameters(dim, 5000, D.Dot, False), chunk, centroids=cen)
    for first, n, key in ((5000, 1000, "across"), (5000, 999, "below")):
        try:
            pq.upsert(first, data[first:first + n])
            info["planar/" + key] = "ok"
        except qa.EncodingError as e:
            info["planar/" + key] = e.kind
    info["planar/count"] = pq.count
    try:
        pq.reserve(6000)
        info["planar/reserve"] = "ok"
    except qa.EncodingError as e:
        info["planar/reserve"] = e.kind
    with open(out_path, "w") as f:
        json.dump(info, f)
    print("DONE")


def test_u8_image_follows_and_the_planar_limit_is_refused(tmp_path):
    assert os.path.exists(DEV_LIB), "the developer library is built with the product one (make -C quantization_amd/csrc)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
    env.update(QAMD_LIB_PATH=DEV_LIB, QAMD_DEV_PQ_PLANAR_ROWS="6000")
    out = str(tmp_path / "info.json")
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_upsert as T\nT.child_main(%r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), out))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "DONE" in res.stdout, f"exit {res.returncode}\n{res.stderr[-4000:]}"
    with open(out) as f:
        info = json.load(f)
    for dim, chunks in ((128, 7), (768, 42)):
        assert info[f"{dim}/chunks_before"] == info[f"{dim}/chunks_after"] == chunks, info
        assert info[f"{dim}/scan_read_image"] == 1 and info[f"{dim}/image_equal"] is True, info
    assert info["100/chunks_before"] == info["100/chunks_after"] == 0 and info["100/scan_read_image"] == 0, info
    for (dim, bits), chunks in zip(RANGE_CASES, (8, 14, 2)):
        # the new rows differ from the old ones at both ends of the range, and the WHOLE image is the packer's
        assert info[f"range/{dim}/{bits}"] == [chunks, True, 60, 69], (dim, bits, info)
    assert info["planar/across"] == "ArgumentsError" and info["planar/below"] == "ok" and info["planar/count"] == 5999, info
    assert info["planar/reserve"] == "ArgumentsError", info


# ------------------------------------------------------------------ PQ
# m = 96: pq_scan_skew_kernel; m = 80: its padded ring; m = 192 (dim 384, chunk 2): the planar image in two slices;
# dim 100, chunk 8: a short last chunk
@pytest.mark.parametrize("dim,chunk", [(768, 8), (640, 8), (384, 2), (100, 8)])
def test_pq_upsert_equals_a_fresh_store(qo, tmp_path, dim, chunk):
    rng = np.random.default_rng(dim + chunk)
    cen = rng.random((256, dim), dtype=np.float32)
    data0, more, queries = rng.random((N0, dim), dtype=np.float32), rng.random((N_FINAL - N0 + 111, dim), dtype=np.float32), \
        rng.random((5, dim), dtype=np.float32)
    vp = qa.VectorParameters(dim, N0, D.Dot, False)
    up = qa.EncodedVectorsPQ.encode(data0, vp, chunk, centroids=cen)
    final = run_steps(up, data0, more)
    assert np.array_equal(up.centroids, cen)
    assert np.array_equal(np.asarray(up.storage_bytes()).reshape(len(final), -1), qo.pq_encode(final, chunk, cen)), "rows"
    fresh = qa.EncodedVectorsPQ.encode_stream(lambda: iter([final[:1500], final[1500:]]),
                                              qa.VectorParameters(dim, len(final), D.Dot, False), chunk, centroids=cen)
    assert_same_store(up, fresh, queries, N0, tmp_path, rng, what=f"pq {dim}/{chunk}")


# ------------------------------------------------------------------ binary
@pytest.mark.parametrize("dim", [100, 1024])
@pytest.mark.parametrize("store", [qa.BitsStoreType.U8, qa.BitsStoreType.U128])
@pytest.mark.parametrize("encoding", [qa.BinaryEncoding.OneBit, qa.BinaryEncoding.TwoBits])
def test_bin_upsert_equals_a_fresh_store(qo, tmp_path, dim, store, encoding):
    rng = np.random.default_rng(dim + int(store))
    data0, more, queries = make(dim, N0, 1), make(dim, N_FINAL - N0 + 111, 2), make(dim, 5, 3)
    two = encoding == qa.BinaryEncoding.TwoBits
    thr = (-0.3 - 0.2 * np.abs(make(dim, 1, 7)[0]), 0.3 + 0.2 * np.abs(make(dim, 1, 8)[0])) if two else None  # lo < hi
    kw = dict(store=store, encoding=encoding, thresholds=thr)
    up = qa.EncodedVectorsBin.encode(data0, qa.VectorParameters(dim, N0, D.Dot, False), **kw)
    # queries encoded BEFORE the upsert, scored after it: binary, 4-bit, 8-bit and weighted 8-bit (two-bit rows take
    # scalar queries only in the weighted form)
    kinds = [dict(), dict(query_bits=4, weighted=two), dict(query_bits=8, weighted=two), dict(query_bits=8, weighted=True)]
    before = [[up.encode_query(q, **k) for q in queries[:2]] for k in kinds]
    batch_before = up.encode_query_batch(queries, **kinds[1])
    final = run_steps(up, data0, more)
    fresh = qa.EncodedVectorsBin.encode(final, qa.VectorParameters(dim, len(final), D.Dot, False), **kw)
    got = np.asarray(up.storage_bytes()).reshape(len(final), -1)
    want = tb.encode(final, thr[0], thr[1], int(store)) if two else qo.bin_encode(final, int(store))
    assert np.array_equal(got, want), "rows are not the CPU restatement's"
    if two:
        lo, hi = up.thresholds
        assert np.array_equal(lo, thr[0].astype(np.float32)) and np.array_equal(hi, thr[1].astype(np.float32))
    for k, qs in zip(kinds, before):
        assert_same_store(up, fresh, queries[:2], N0, tmp_path, rng, encode=lambda s, q, k=k: s.encode_query(q, **k),
                          up_queries=qs, what=f"bin {dim} {k}")
    fb = fresh.encode_query_batch(queries, **kinds[1])
    assert_bits_equal(up.score_batch(batch_before), fresh.score_batch(fb), "a scalar batch encoded before the upsert")
    iu, su = up.topk_batch(batch_before, 30)
    jf, sf = fresh.topk_batch(fb, 30)
    assert np.array_equal(iu, jf)
    assert_bits_equal(su, sf, "topk_batch of a scalar batch encoded before the upsert")


# ------------------------------------------------------------------ 33 000 rows: reserve, then upserts across the gates
BIG = [(None, 3000), (None, 100), (None, 28700), (None, 200)]  # 1000 -> 4000 -> 4100 -> 32800 -> 33000


def big_case(build, fresh_of, dim, tmp_path, rows_of):
    rng = np.random.default_rng(dim + 33)
    data0, more, queries = rows_of(N0, 1), rows_of(32000, 2), rows_of(16, 3)
    more[-200:] *= 1.25  # the last piece holds the best Dot rows: a stale pivot sample would not know them
    up = build(data0)
    up.reserve(40000)
    assert up.capacity == 40000 and up.count == N0
    up.reserve(2000)  # below the capacity: a no-op
    assert up.capacity == 40000
    final = data0
    at = 0
    for _first, n in BIG:
        up.append(more[at:at + n])
        final = np.concatenate([final, more[at:at + n]])
        at += n
        assert up.count == len(final) and up.capacity == 40000
        if len(final) in (4100, 32800):  # the batch routes past the gate run (and gather their pivot sample) before the next upsert
            b = up.encode_query_batch(queries)
            ids, _ = up.topk_batch(b, 30)
            assert ids.max() < len(final)
    fresh = fresh_of(final)
    assert_same_store(up, fresh, queries, 32800, tmp_path, rng, what=f"33000 x {dim}")


def test_u8_upserts_across_the_batch_gates(tmp_path):
    dim = 768
    vp = lambda n: qa.VectorParameters(dim, n, D.Dot, False)
    ao = {}

    def build(data0):
        up = qa.EncodedVectorsU8.encode(data0, vp(len(data0)))
        ao["v"] = (float(up.metadata["alpha"]), float(up.metadata["offset"]))
        return up

    big_case(build, lambda final: u8_fresh(final, vp(len(final)), *ao["v"], cut=20000), dim, tmp_path,
             lambda n, seed: make(dim, n, seed))


def test_bin_upserts_across_the_batch_gates(tmp_path):
    dim = 1024
    vp = lambda n: qa.VectorParameters(dim, n, D.Dot, False)
    kw = dict(store=qa.BitsStoreType.U128)
    big_case(lambda d: qa.EncodedVectorsBin.encode(d, vp(len(d)), **kw),
             lambda final: qa.EncodedVectorsBin.encode(final, vp(len(final)), **kw), dim, tmp_path,
             lambda n, seed: make(dim, n, seed))


def test_pq_upserts_across_the_batch_gates(tmp_path):
    dim, chunk = 768, 8
    cen = np.random.default_rng(9).random((256, dim), dtype=np.float32)
    vp = lambda n: qa.VectorParameters(dim, n, D.Dot, False)
    big_case(lambda d: qa.EncodedVectorsPQ.encode(d, vp(len(d)), chunk, centroids=cen),
             lambda final: qa.EncodedVectorsPQ.encode(final, vp(len(final)), chunk, centroids=cen), dim, tmp_path,
             lambda n, seed: np.random.default_rng([n, seed]).random((n, dim), dtype=np.float32))


# ------------------------------------------------------------------ the originals
@pytest.mark.parametrize("dtype", ["f32", "f16", "bf16"])
def test_originals_upsert_equals_fresh_and_rescoring_follows(dtype):
    dim = 100  # (odd row pitch for the half types' dword loads: 200 bytes)
    rng = np.random.default_rng(11)
    data0, more, queries = make(dim, N0, 1), make(dim, N_FINAL - N0 + 111, 2), make(dim, 3, 3)
    vp = qa.VectorParameters(dim, N0, D.Dot, False)
    orig = qa.OriginalVectors.from_data(data0, vp, dtype=dtype)
    final = run_steps(orig, data0, more)
    assert orig.dtype == dtype and orig.get_parameters().count == N_FINAL
    vpn = qa.VectorParameters(dim, N_FINAL, D.Dot, False)
    fresh = qa.OriginalVectors.from_data(final, vpn, dtype=dtype)
    ids = np.arange(N_FINAL, dtype=np.uint32)
    for q in queries:
        assert_bits_equal(orig.score_ids(q, ids), fresh.score_ids(q, ids), f"{dtype} originals")
    if dtype == "f16":  # rows already of the store's type are taken as they are
        half = more[:50].astype(np.float16)
        orig.upsert(10, half)
        fresh2 = final.copy()
        fresh2[10:60] = half.astype(np.float32)
        want = qa.OriginalVectors.from_data(fresh2, vpn, dtype=dtype).score_ids(queries[0], ids)
        assert_bits_equal(orig.score_ids(queries[0], ids), want, "f16 rows upserted as f16")
        orig.upsert(10, final[10:60])
    # rescoring: the quantized store and the originals extended together equal the fresh pair; one alone is refused
    u8 = qa.EncodedVectorsU8.encode(data0, vp)
    md = u8.metadata
    short = qa.OriginalVectors.from_data(data0, vp, dtype=dtype)
    u8.append(final[N0:1500])
    q8 = u8.encode_query(queries[0])
    with pytest.raises(qa.EncodingError, match="do not belong"):
        u8.topk_rescored(q8, short, queries[0], 10, 100)
    short.append(final[N0:1500])
    u8f = u8_fresh(final[:1500], vp, float(md["alpha"]), float(md["offset"]), cut=700)
    of = qa.OriginalVectors.from_data(final[:1500], qa.VectorParameters(dim, 1500, D.Dot, False), dtype=dtype)
    got = u8.topk_rescored(q8, short, queries[0], 10, 100)
    want = u8f.topk_rescored(u8f.encode_query(queries[0]), of, queries[0], 10, 100)
    assert np.array_equal(got[0], want[0])
    assert_bits_equal(got[1], want[1], "topk_rescored after both were extended")
    short.append(final[1500:1501])
    with pytest.raises(qa.EncodingError, match="do not belong"):
        u8.topk_rescored(q8, short, queries[0], 10, 100)


# ------------------------------------------------------------------ refusals
def small_stores():
    dim = 128
    data = make(dim, 300, 1)
    vp = qa.VectorParameters(dim, 300, D.Dot, False)
    cen = np.random.default_rng(2).random((256, dim), dtype=np.float32)
    return data, [qa.EncodedVectorsU8.encode(data, vp), qa.EncodedVectorsPQ.encode(data, vp, 8, centroids=cen),
                  qa.EncodedVectorsBin.encode(data, vp), qa.OriginalVectors.from_data(data, vp)]


def test_refusals_leave_the_store_as_it_was():
    data, stores = small_stores()
    L = qa.lib()
    for s in stores:
        before = None if isinstance(s, qa.OriginalVectors) else np.asarray(s.storage_bytes()).copy()
        with pytest.raises(qa.EncodingError, match="hole") as e:
            s.upsert(301, data[:2])  # a hole
        assert e.value.status == _lib.ERR_ARGUMENTS
        s.upsert(300, data[:0])  # no rows: QAMD_OK, nothing touched
        s.upsert(0, data[:0])
        s.reserve(10)  # below the capacity: a no-op
        assert s.count == 300 and s.capacity == 300
        # null data with n_rows > 0, straight through the C ABI
        name = "f32" if isinstance(s, qa.OriginalVectors) else s._prefix
        args = (s._h, 0, None) + ((_lib.DTYPE_F32,) if name == "f32" else ()) + (_lib.MEM_HOST, 2, None)
        assert getattr(L, f"qamd_{name}_upsert")(*args) == _lib.ERR_ARGUMENTS
        assert b"data is null" in L.qamd_last_error()
        if before is not None:
            assert np.array_equal(np.asarray(s.storage_bytes()), before)
    # an f16 store takes no bf16 rows
    half = qa.OriginalVectors.from_data(data, qa.VectorParameters(128, 300, D.Dot, False), dtype="f16")
    with pytest.raises(ValueError):
        half.upsert(0, np.zeros((1, 128), dtype=np.uint16))
    assert L.qamd_f32_upsert(half._h, 0, data.ctypes.data, _lib.DTYPE_BF16, _lib.MEM_HOST, 1, None) == _lib.ERR_ARGUMENTS


def test_a_borrowed_original_store_is_refused():
    torch = pytest.importorskip("torch")
    t = torch.from_numpy(make(64, 100, 1)).cuda()
    orig = qa.OriginalVectors.from_data(t, qa.VectorParameters(64, 100, D.Dot, False), borrow=True)
    assert orig.capacity == 100
    for call in (lambda: orig.upsert(0, t[:1]), lambda: orig.append(t[:1]), lambda: orig.reserve(1000)):
        with pytest.raises(qa.EncodingError, match="borrowed") as e:
            call()
        assert e.value.status == _lib.ERR_ARGUMENTS
    assert orig.count == 100


def test_a_u8_store_built_empty_is_refused_and_an_empty_shard_with_an_interval_is_not(qo):
    dim = 128
    vp0 = qa.VectorParameters(dim, 0, D.Dot, False)
    empty = qa.EncodedVectorsU8.encode(np.zeros((0, dim), dtype=np.float32), vp0)
    assert empty.metadata["alpha"] == 0
    with pytest.raises(qa.EncodingError, match="alpha is 0"):
        empty.append(make(dim, 3, 1))
    assert empty.count == 0
    # the same empty store with its interval given (an empty shard, qamd_u8_encode) can be filled
    data = make(dim, 70, 1)
    shard = qa.EncodedVectorsU8.encode(np.zeros((0, dim), dtype=np.float32), vp0, alpha_offset=(0.05, -3.0))
    shard.append(data)
    rows, _ = qo.u8_encode_with(data, int(D.Dot), False, 0.05, -3.0)
    assert shard.count == 70 and np.array_equal(shard.storage_bytes(), rows)


def test_a_shard_of_a_sharded_handle_raises():
    dim = 128
    data = make(dim, 600, 1)
    vp = qa.VectorParameters(dim, 600, D.Dot, False)
    cen = np.random.default_rng(2).random((256, dim), dtype=np.float32)
    for sh in (qa.ShardedVectorsU8.encode(data, vp, [0, 0]), qa.ShardedVectorsBin.encode(data, vp, [0, 0]),
               qa.ShardedVectorsPQ.encode(data, vp, 8, [0, 0], centroids=cen)):
        view, _base = sh.shard(1)
        for call in (lambda: view.upsert(0, data[:1]), lambda: view.append(data[:1]), lambda: view.reserve(1000)):
            with pytest.raises(ValueError, match="shard"):
                call()
        assert view.count == 300
