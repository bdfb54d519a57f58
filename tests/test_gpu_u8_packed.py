"""The packed u8 scan image (csrc/u8.hip build_packed), checked against the byte codes and the oracle.

Every u8 store of 8 to 128 chunks keeps, beside its byte codes, an image of the codes at 7 bits each that the Dot and L2
scans of lane mode 0 read (u8_internal.hpp).  It may never change a result: the pair sum is the same exact integer,
added in another order.  Each configuration runs in a fresh child process on the developer library (tools/lib), once
as built and once with QAMD_DEV_U8_PACKED=0 (no image: every scan reads the bytes).  The parent compares the two runs bit
for bit with each other and with the oracle, and reads which image served each call (qamd_dev_u8_last_scan_packed).
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from util import assert_bits_equal, topk_want

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
D = qa.DistanceType
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")

KS = (1, 30, 1024)
# (dim, rows, distance): rc % 8 zero and not, exact and clamped tiles (packed chunks 7, 8, 14, 42, 57, 84, 112), row
# counts that are no multiple of any tile
CASES = [(128, 5003, D.Dot), (144, 4099, D.L2), (240, 3001, D.Dot), (768, 20011, D.Dot), (768, 20011, D.L2),
         (1040, 3007, D.Dot), (1536, 4001, D.L2), (2048, 2003, D.Dot), (768, 5003, D.L1)]
BIG = (144, 2_100_003, D.Dot)  # past the single-launch top-k's 2^21 rows: k = 1 and 30 take the fused top-k too
LAYOUT_DIMS = (128, 240, 768, 1040)
EXTRA_DIMS = (128, 256)  # 8 and 16 chunks: one extra chunk, two


def packed_chunks(dim, dist):
    rc = -(-dim // 16)
    return 0 if dist == D.L1 or rc < 8 or rc > 128 else rc - rc // 8


def numpy_pack(codes):
    """The packed image of byte codes [n, 16 * rc] (u8_internal.hpp): [n, 16 * P] bytes."""
    n, ad = codes.shape
    rc = ad // 16
    e, p = rc // 8, rc - rc // 8
    ch = codes.reshape(n, rc, 16)
    out = (ch[:, :p] & 0x7F).copy()
    for j in range(7 * e):
        plane = (ch[:, p + j // 7] >> (j % 7)) & 1
        out[:, j] |= (plane << 7).astype(np.uint8)
    return out.reshape(n, p * 16)


def data_of(dim, n, seed=0):
    rng = np.random.default_rng(dim * 7 + n + seed)
    return rng.standard_normal((n, dim)).astype(np.float32), rng.standard_normal((2, dim)).astype(np.float32)


# ------------------------------------------------------------------ the child: one configuration, results to an .npz
def _image(enc):
    return int(qa.lib().qamd_dev_u8_last_scan_packed(enc._h))


def _store_chunks(enc):
    ptr, chunks = C.c_void_p(), C.c_uint32()
    qa.lib().qamd_dev_u8_packed(enc._h, C.byref(ptr), C.byref(chunks))
    return int(chunks.value)


def _store(R, info, tag, enc, queries, ks=KS):
    info[tag + "/chunks"] = _store_chunks(enc)
    for qi, query in enumerate(queries):
        q = enc.encode_query(query)
        R[f"{tag}/q{qi}/all"] = enc.score_all(q)
        info[f"{tag}/q{qi}/all"] = _image(enc)
        for k in ks:
            ids, sc = enc.topk(q, k)
            R[f"{tag}/q{qi}/topk{k}"] = np.stack([np.asarray(ids).view(np.float32), np.asarray(sc)])
            info[f"{tag}/q{qi}/topk{k}"] = _image(enc)


def _device_bytes(ptr, nbytes):
    import torch
    hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    out = np.empty(nbytes, dtype=np.uint8)
    assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), ptr, C.c_size_t(nbytes), 2) == 0  # hipMemcpyDeviceToHost
    return out


def child_main(out_path, tmp_dir):
    L = qa.lib()
    L.qamd_dev_u8_last_scan_packed.restype = C.c_int
    R, info = {}, {}
    for dim, n, dist in CASES + [BIG]:
        data, queries = data_of(dim, n)
        enc = qa.EncodedVectorsU8.encode(data, qa.VectorParameters(dim, n, dist, False))
        _store(R, info, f"enc{dim}x{n}/{int(dist)}", enc, queries)
        if dim in LAYOUT_DIMS and dist != D.L1:
            ptr, chunks = C.c_void_p(), C.c_uint32()
            L.qamd_dev_u8_packed(enc._h, C.byref(ptr), C.byref(chunks))
            if chunks.value:
                R[f"layout{dim}"] = _device_bytes(ptr, n * chunks.value * 16).reshape(n, -1)
                R[f"codes{dim}"] = enc.storage_bytes()[:, 4:]
    # the streaming encoder, save + load (through from_rows), lane mode 1
    dim, n = 768, 20011
    data, queries = data_of(dim, n)
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    st = qa.EncodedVectorsU8.encode_stream(lambda: iter([data[:7000], data[7000:]]), vp)
    _store(R, info, "stream", st, queries)
    st.save(os.path.join(tmp_dir, "s.bin"), os.path.join(tmp_dir, "s.json"))
    ld = qa.EncodedVectorsU8.load(os.path.join(tmp_dir, "s.bin"), os.path.join(tmp_dir, "s.json"), vp)
    _store(R, info, "load", ld, queries)
    st.set_lane_mode(1)
    _store(R, info, "lanes", st, queries, ks=(30,))
    # rows from another producer: all 127, all 0, and codes of 128 / 255 (the image must be dropped)
    rows = st.storage_bytes()
    for name, fill in (("r127", 127), ("r0", 0), ("r128", 128), ("r255", 255)):
        r = rows.copy()
        if fill in (127, 0):
            r[:, 4:] = fill
        else:
            r[n // 2, 4 + 700] = fill  # one code of one row, in an extra chunk
        enc = qa.EncodedVectorsU8.from_storage(r, st.metadata)
        _store(R, info, name, enc, queries)
    # the same at the shortest rows: one code of 128 in the last extra chunk of row 65 of 70 (the second, partial block),
    # which only the pack threads that take their bit plane from that chunk read
    for xdim in EXTRA_DIMS:
        xdata, xqueries = data_of(xdim, 70)
        small = qa.EncodedVectorsU8.encode(xdata, qa.VectorParameters(xdim, 70, D.Dot, False))
        info[f"x128/{xdim}/chunks_clean"] = _store_chunks(small)
        r = small.storage_bytes().copy()
        r[65, 4 + xdim - 16 + 5] = 128
        _store(R, info, f"x128/{xdim}", qa.EncodedVectorsU8.from_storage(r, small.metadata), xqueries, ks=())
        R[f"x128/{xdim}/rows"] = r
    # a two-shard handle builds its shards through the same builders
    sh = qa.ShardedVectorsU8.encode(data, vp, [0, 0])
    for qi, query in enumerate(queries):
        q = sh.encode_query(query)
        R[f"shard/q{qi}/all"] = sh.score_all(q)
        for k in KS:
            ids, sc = sh.topk(q, k)
            R[f"shard/q{qi}/topk{k}"] = np.stack([np.asarray(ids).view(np.float32), np.asarray(sc)])
    np.savez(out_path, **R)
    with open(out_path + ".json", "w") as f:
        json.dump(info, f)
    print("DONE")


def run_child(tmp_dir, name, env_add, timeout=900):
    assert os.path.exists(DEV_LIB), "the developer library is built with the product one (make -C quantization_amd/csrc)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
    env.update(env_add, QAMD_LIB_PATH=DEV_LIB)
    out = os.path.join(str(tmp_dir), name + ".npz")
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_u8_packed as T\nT.child_main(%r, %r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), out, str(tmp_dir)))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=env)
    assert res.returncode == 0 and "DONE" in res.stdout, f"{name}: exit {res.returncode}\n{res.stderr[-4000:]}"
    with open(out + ".json") as f:
        info = json.load(f)
    return dict(np.load(out)), info


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("u8_packed")
    return {"packed": run_child(d, "packed", {}), "bytes": run_child(d, "bytes", {"QAMD_DEV_U8_PACKED": "0"})}


def _want(qo, data, dist, query):
    rows, meta = qo.u8_encode(data, int(dist), False)
    codes, qoff = qo.u8_encode_query(meta, query)
    return qo.u8_score_all(meta, rows, codes, qoff, order=qo.ORDER_AVX2), rows, meta


def _check_topk(got, scores, k, tag):
    wi, ws = topk_want(scores, k, True)
    assert np.array_equal(got[0].view(np.uint32), wi), f"{tag}: ids differ"
    assert_bits_equal(got[1], ws, tag + " scores")


def _same_runs(runs, prefix):
    P, B = runs["packed"][0], runs["bytes"][0]
    keys = [k for k in P if k.startswith(prefix)]
    assert keys, prefix
    for k in keys:
        assert_bits_equal(P[k], B[k], f"{k}: packed vs byte image")


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("case", CASES + [BIG], ids=lambda c: f"{c[0]}x{c[1]}-{c[2].name}")
def test_packed_scan_equals_bytes_and_oracle(runs, qo, case):
    dim, n, dist = case
    tag = f"enc{dim}x{n}/{int(dist)}"
    _same_runs(runs, tag + "/")
    (P, pinfo), (_, binfo) = runs["packed"], runs["bytes"]
    want_chunks = packed_chunks(dim, dist)
    assert pinfo[tag + "/chunks"] == want_chunks and binfo[tag + "/chunks"] == 0
    data, queries = data_of(dim, n)
    for qi, query in enumerate(queries):
        want = _want(qo, data, dist, query)[0]
        assert_bits_equal(P[f"{tag}/q{qi}/all"], want, f"{tag} score_all")
        assert pinfo[f"{tag}/q{qi}/all"] == (1 if want_chunks else 0)
        for k in KS:
            _check_topk(P[f"{tag}/q{qi}/topk{k}"], want, k, f"{tag} topk {k}")
            # k <= 64 on up to 2^21 rows: the single-launch top-k, which reads the bytes
            fused = k > 64 or n > (2 << 20)
            assert pinfo[f"{tag}/q{qi}/topk{k}"] == (1 if want_chunks and fused else 0), (tag, k)
            assert binfo[f"{tag}/q{qi}/topk{k}"] == 0


@pytest.mark.parametrize("dim", LAYOUT_DIMS)
def test_packed_layout_matches_numpy_packer(runs, dim):
    R = runs["packed"][0]
    assert np.array_equal(R[f"layout{dim}"], numpy_pack(R[f"codes{dim}"])), f"dim {dim}: packed image"


def test_stream_load_lane_mode_and_foreign_rows(runs, qo):
    (P, pinfo), (_, binfo) = runs["packed"], runs["bytes"]
    for prefix in ("stream/", "load/", "lanes/", "r127/", "r0/", "r128/", "r255/", "shard/"):
        _same_runs(runs, prefix)
    dim, n = 768, 20011
    data, queries = data_of(dim, n)
    for tag in ("stream", "load"):
        assert pinfo[tag + "/chunks"] == 42
    assert pinfo["r127/chunks"] == 42 and pinfo["r0/chunks"] == 42
    assert pinfo["r128/chunks"] == 0 and pinfo["r255/chunks"] == 0, "a code above 127 must drop the image"
    assert pinfo["lanes/q0/all"] == 0 and pinfo["lanes/q0/topk30"] == 0, "lane mode 1 reads the bytes"
    for qi, query in enumerate(queries):
        want, rows, meta = _want(qo, data, D.Dot, query)
        for tag in ("stream", "load", "lanes", "shard"):
            assert_bits_equal(P[f"{tag}/q{qi}/all"], want, f"{tag} score_all")
        for k in KS:
            for tag in ("stream", "load", "shard"):
                _check_topk(P[f"{tag}/q{qi}/topk{k}"], want, k, f"{tag} topk {k}")
        codes, qoff = qo.u8_encode_query(meta, query)
        for tag, fill in (("r127", 127), ("r0", 0)):
            r = rows.copy()
            r[:, 4:] = fill
            w = qo.u8_score_all(meta, r, codes, qoff, order=qo.ORDER_AVX2)
            assert_bits_equal(P[f"{tag}/q{qi}/all"], w, f"{tag} score_all")
            assert pinfo[f"{tag}/q{qi}/all"] == 1
            for k in KS:
                _check_topk(P[f"{tag}/q{qi}/topk{k}"], w, k, f"{tag} topk {k}")


@pytest.mark.parametrize("dim", EXTRA_DIMS)
def test_a_foreign_code_in_an_extra_chunk_drops_the_image(runs, qo, dim):
    (P, pinfo), (B, binfo) = runs["packed"], runs["bytes"]
    tag = f"x128/{dim}"
    assert pinfo[tag + "/chunks_clean"] == packed_chunks(dim, D.Dot), "without the foreign code the store has an image"
    assert pinfo[tag + "/chunks"] == 0 and binfo[tag + "/chunks"] == 0, "a code of 128 in an extra chunk must drop the image"
    _same_runs(runs, tag + "/q")
    data, queries = data_of(dim, 70)
    rows, meta = qo.u8_encode(data, int(D.Dot), False)
    r = P[tag + "/rows"]
    at = dim - 16 + 5  # the code that was replaced: the rest of the rows is the oracle's, and its chunk is an extra one
    assert np.argwhere(r != rows).tolist() == [[65, 4 + at]] and at // 16 >= packed_chunks(dim, D.Dot)
    for qi, query in enumerate(queries):
        codes, qoff = qo.u8_encode_query(meta, query)
        want = qo.u8_score_all(meta, r, codes, qoff, order=qo.ORDER_AVX2)
        assert_bits_equal(P[f"{tag}/q{qi}/all"], want, f"{tag} score_all")
        assert pinfo[f"{tag}/q{qi}/all"] == 0, "the scan read an image the store must not have"
