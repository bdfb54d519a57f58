"""The blocked packed scan (csrc/u8.hip u8_scan_image_kernel<Image7>) against the byte codes and the oracle.

The packed image of a u8 store (u8_internal.hpp) lies in blocks of 64 rows: chunk j of row r is the 16 bytes at index
((r / 64) * P + j) * 64 + r % 64.  One wave scans one block, a row per lane, in groups of 7 chunks that share one extra
chunk, then the rc % 8 chunks that carry no plane; stores too small to fill the GPU launch 2, 4 or 8 waves per block,
whose partial sums meet in LDS.  None of that may change a result.  Each configuration runs in a fresh child process
on the developer library (tools/lib): as built, with QAMD_DEV_U8_PACKED=0 (no image: every scan reads the bytes), and
with QAMD_DEV_CU_COUNT=1, where the dispatch rule (launch_scan_image: one wave per block once the blocks number
16 * CUs) takes one wave per block from 1024 rows on.  The parent compares the runs bit for bit with each other and
with the oracle and reads which image and how many waves per block served each call.

Stores come from from_storage with uniform random codes 0..127 (Gaussian data never sets the high planes of the extra
chunks), so the test owns every byte.  The numpy model of one lane's arithmetic is checked against the oracle
without a GPU.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from util import assert_bits_equal, oracle_meta, qa_meta, store_rows, topk_want, u8_actual_dim as actual_dim

qa = pytest.importorskip("quantization_amd")
D = qa.DistanceType
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")

BLOCK = 64
# 8: one group, no rest; 9: one group + one plain chunk; 15: one group + seven plain; 16: two groups; 48: six groups;
# 65: odd, with a rest; 127, 128: the upper limit.  Dim 130 pads to 144 (rc 9).
RCS = (8, 9, 15, 16, 48, 65, 127, 128)
DIMS = tuple(16 * rc for rc in RCS) + (130,)
# partial last block, exactly one block, padding blocks; all small enough for several waves per block on a whole GPU
ROWS = (1, 63, 64, 65, 1023, 1025, 4099)
L2_ROWS = (65, 1025)
PLANE_RCS = (16, 48)  # stores in which one plane of one extra chunk is set
PLANE_ROWS = 70
TOPK_KS = (100, 1024)
TOPK_CASES = [(768, 20011), (144, 4099)]  # k > 64: the fused top-k, whose filtering pass is the FILTER form
BIG = (144, 2_100_003)  # past the single-launch top-k's 2^21 rows; 32 813 blocks: one wave per block on any GPU
LAYOUT = [(128, 1), (144, 65), (768, 1025), (2048, 130)]


def plane_codes(rc, e, b, n):
    """Only plane b of extra chunk e (chunk P + e of the row) is set, in all of its 16 codes."""
    p = rc - rc // 8
    codes = np.zeros((n, 16 * rc), dtype=np.uint8)
    codes[:, 16 * (p + e):16 * (p + e + 1)] = 1 << b
    return codes


def numpy_pack_blocked(codes):
    """The blocked packed image of byte codes [n, 16 * rc]: [ceil(n / 64), P, 64, 16] bytes, padding rows zero."""
    n, ad = codes.shape
    rc = ad // 16
    e, p = rc // 8, rc - rc // 8
    ch = codes.reshape(n, rc, 16)
    img = (ch[:, :p] & 0x7F).copy()
    for j in range(7 * e):
        img[:, j] |= (((ch[:, p + j // 7] >> (j % 7)) & 1) << 7).astype(np.uint8)
    blocks = -(-n // BLOCK)
    out = np.zeros((blocks * BLOCK, p, 16), dtype=np.uint8)
    out[:n] = img
    return out.reshape(blocks, BLOCK, p, 16).transpose(0, 2, 1, 3).copy()


def model_sums(image, rc, qcodes):
    """The integer pair sums as one lane of u8_scan_image_kernel<Image7> adds them: groups of 7 chunks with the group's
    extra chunk, plane shift 7 - j % 7, then the chunks without a plane.  image: numpy_pack_blocked's array."""
    e, p = rc // 8, rc - rc // 8
    q = qcodes.reshape(rc, 16).astype(np.int64)
    blocks = image.shape[0]
    acc = np.zeros((blocks, BLOCK), dtype=np.int64)
    for g in range(e):
        qx = q[p + g]
        for i in range(7):
            v = image[:, 7 * g + i].astype(np.int64)  # [blocks, 64, 16]
            acc += (v & 0x7F) @ q[7 * g + i] + (((v & 0x80) @ qx) >> (7 - i))
    for j in range(7 * e, p):
        acc += (image[:, j].astype(np.int64) & 0x7F) @ q[j]
    return acc.reshape(-1)


def expected_split(n, cu):
    blocks, split = -(-n // BLOCK), 1
    while split < 8 and blocks * split < 16 * cu:
        split *= 2
    return split


def score_cases():
    cases = [(dim, n, D.Dot) for dim in DIMS for n in ROWS] + [(dim, n, D.L2) for dim in DIMS for n in L2_ROWS]
    return cases


# ------------------------------------------------------------------ the child: one configuration, results to an .npz
def child_main(out_path, mode):
    L = qa.lib()
    L.qamd_dev_u8_last_scan_packed.restype = C.c_int
    L.qamd_dev_u8_last_scan_split.restype = C.c_int
    L.qamd_dev_cu_count.restype = C.c_int
    R, info = {}, {"cu": int(L.qamd_dev_cu_count())}

    def seen(enc):
        return [int(L.qamd_dev_u8_last_scan_packed(enc._h)), int(L.qamd_dev_u8_last_scan_split(enc._h))]

    def score(tag, rows, query, dim, n, dist):
        enc = qa.EncodedVectorsU8.from_storage(rows, qa_meta(dim, n, dist))
        R[tag] = enc.score_all(enc.encode_query(query))
        info[tag] = seen(enc)
        return enc

    for dim, n, dist in score_cases():
        rows, query = store_rows(dim, n)
        score(f"all/{dim}x{n}/{int(dist)}", rows, query, dim, n, dist)
    # every code 127 at rc 128 against a query of 127s: the sum 33 032 192 is past 2^24 and is rounded once
    dim, n = 2048, 1025
    rows, _ = store_rows(dim, n, codes=np.full((n, dim), 127, dtype=np.uint8))
    score("all127", rows, np.full(dim, 2.0, dtype=np.float32), dim, n, D.Dot)
    for rc in PLANE_RCS:
        for e in range(rc // 8):
            for b in range(7):
                rows, query = store_rows(16 * rc, PLANE_ROWS, seed=e * 7 + b, codes=plane_codes(rc, e, b, PLANE_ROWS))
                score(f"plane/{rc}/{e}/{b}", rows, query, 16 * rc, PLANE_ROWS, D.Dot)
    if mode != "cu1":
        for dim, n in TOPK_CASES + [BIG]:
            rows, query = store_rows(dim, n)
            enc = score(f"topk/{dim}x{n}/all", rows, query, dim, n, D.Dot)
            q = enc.encode_query(query)
            for k in TOPK_KS:
                ids, sc = enc.topk(q, k)
                R[f"topk/{dim}x{n}/{k}"] = np.stack([np.asarray(ids).view(np.float32), np.asarray(sc)])
                info[f"topk/{dim}x{n}/{k}"] = seen(enc)
        import torch
        hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
        for dim, n in LAYOUT:
            rows, _ = store_rows(dim, n)
            enc = qa.EncodedVectorsU8.from_storage(rows, qa_meta(dim, n, D.Dot))
            ptr, chunks, brows = C.c_void_p(), C.c_uint32(), C.c_uint32()
            L.qamd_dev_u8_packed_blocked(enc._h, C.byref(ptr), C.byref(chunks), C.byref(brows))
            info[f"layout/{dim}x{n}"] = [int(chunks.value), int(brows.value)]
            if chunks.value:
                out = np.empty(-(-n // BLOCK) * BLOCK * chunks.value * 16, dtype=np.uint8)
                assert hip.hipMemcpy(C.c_void_p(out.ctypes.data), ptr, C.c_size_t(out.size), 2) == 0  # DeviceToHost
                R[f"layout/{dim}x{n}"] = out
    np.savez(out_path, **R)
    with open(out_path + ".json", "w") as f:
        json.dump(info, f)
    print("DONE")


def run_child(tmp_dir, name, env_add, timeout=600):
    assert os.path.exists(DEV_LIB), "the developer library is built with the product one (make -C quantization_amd/csrc)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
    env.update(env_add, QAMD_LIB_PATH=DEV_LIB)
    out = os.path.join(str(tmp_dir), name + ".npz")
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_u8_blocked as T\nT.child_main(%r, %r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), out, name))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=env)
    assert res.returncode == 0 and "DONE" in res.stdout, f"{name}: exit {res.returncode}\n{res.stderr[-4000:]}"
    with open(out + ".json") as f:
        info = json.load(f)
    return dict(np.load(out)), info


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("u8_blocked")
    return {"blocked": run_child(d, "blocked", {}), "bytes": run_child(d, "bytes", {"QAMD_DEV_U8_PACKED": "0"}),
            "cu1": run_child(d, "cu1", {"QAMD_DEV_CU_COUNT": "1"})}


_WANT = {}


def want_scores(qo, key, dim, n, dist, rows, query):
    """The oracle's scores of store `key` (and the query's codes), computed once and shared by the tests."""
    if key not in _WANT:
        meta = oracle_meta(qo, dim, n, dist)
        codes, qoff = qo.u8_encode_query(meta, query)
        _WANT[key] = (qo.u8_score_all(meta, rows, codes, qoff, order=qo.ORDER_AVX2), codes)
    return _WANT[key]


def check_tag(runs, qo, tag, dim, n, dist, rows, query, names=("blocked", "bytes", "cu1")):
    want, _ = want_scores(qo, tag, dim, n, dist, rows, query)
    for name in names:
        R, info = runs[name]
        assert_bits_equal(R[tag], want, f"{tag} ({name})")
        packed, split = info[tag]
        if name == "bytes":
            assert packed == 0, (tag, name)
        else:
            assert packed == 1, f"{tag} ({name}): the blocked scan did not run"
            assert split == expected_split(n, info["cu"]), (tag, name, split)


# ------------------------------------------------------------------ tests
@pytest.mark.parametrize("rc", RCS)
def test_numpy_model_of_a_lane_matches_the_oracle(qo, rc):
    """No GPU: the decode order of u8_scan_image_kernel<Image7>, restated in numpy on the numpy packer's image, gives the
    oracle's scores (the exact integer sum, then the f32 epilogue)."""
    dim, n = 16 * rc, 131
    rows, query = store_rows(dim, n, seed=1)
    want, qcodes = want_scores(qo, f"model/{rc}", dim, n, D.Dot, rows, query)
    sums = model_sums(numpy_pack_blocked(rows[:, 4:]), rc, qcodes)[:n]
    assert np.array_equal(sums, rows[:, 4:].astype(np.int64) @ qcodes.astype(np.int64)), "integer sums"
    meta = oracle_meta(qo, dim, n, D.Dot)
    _, qoff = qo.u8_encode_query(meta, query)
    got = (np.float32(meta.multiplier) * sums.astype(np.float32) + np.float32(qoff)) + rows[:, :4].copy().view(np.float32)[:, 0]
    assert_bits_equal(got, want, f"rc {rc}: model scores")


@pytest.mark.gpu
@pytest.mark.parametrize("dim", DIMS)
def test_blocked_scan_equals_bytes_and_oracle(runs, qo, dim):
    for d, n, dist in score_cases():
        if d == dim:
            rows, query = store_rows(dim, n)
            check_tag(runs, qo, f"all/{dim}x{n}/{int(dist)}", dim, n, dist, rows, query)


@pytest.mark.gpu
def test_both_dispatch_forms_ran(runs):
    """Several waves per block on the whole GPU, one wave per block where the rule says so (QAMD_DEV_CU_COUNT=1)."""
    info = runs["blocked"][1]
    assert info["cu"] >= 8, "these row counts are chosen for a GPU of at least 8 CUs"
    assert all(info[f"all/768x{n}/{int(D.Dot)}"][1] > 1 for n in ROWS)
    one = runs["cu1"][1]
    assert one["cu"] == 1
    assert [one[f"all/768x{n}/{int(D.Dot)}"][1] for n in ROWS] == [8, 8, 8, 8, 1, 1, 1]
    assert info[f"topk/{BIG[0]}x{BIG[1]}/all"] == [1, 1], "the big store takes one wave per block"


@pytest.mark.gpu
def test_sum_past_2_pow_24_is_rounded_once(runs, qo):
    dim, n = 2048, 1025
    rows, _ = store_rows(dim, n, codes=np.full((n, dim), 127, dtype=np.uint8))
    query = np.full(dim, 2.0, dtype=np.float32)
    _, codes = want_scores(qo, "all127", dim, n, D.Dot, rows, query)
    assert int(codes.astype(np.int64).sum()) * 127 == 33_032_192
    check_tag(runs, qo, "all127", dim, n, D.Dot, rows, query)


@pytest.mark.gpu
@pytest.mark.parametrize("rc", PLANE_RCS)
def test_single_planes_of_the_extra_chunks(runs, qo, rc):
    """A wrong plane shift or a wrong group index changes exactly these scores."""
    for e in range(rc // 8):
        for b in range(7):
            rows, query = store_rows(16 * rc, PLANE_ROWS, seed=e * 7 + b, codes=plane_codes(rc, e, b, PLANE_ROWS))
            check_tag(runs, qo, f"plane/{rc}/{e}/{b}", 16 * rc, PLANE_ROWS, D.Dot, rows, query)


@pytest.mark.gpu
@pytest.mark.parametrize("case", TOPK_CASES + [BIG], ids=lambda c: f"{c[0]}x{c[1]}")
def test_topk_through_the_filter_form(runs, qo, case):
    dim, n = case
    rows, query = store_rows(dim, n)
    check_tag(runs, qo, f"topk/{dim}x{n}/all", dim, n, D.Dot, rows, query, names=("blocked", "bytes"))
    want, _ = want_scores(qo, f"topk/{dim}x{n}/all", dim, n, D.Dot, rows, query)
    for k in TOPK_KS:
        wi, ws = topk_want(want, k, True)
        for name in ("blocked", "bytes"):
            R, info = runs[name]
            got = R[f"topk/{dim}x{n}/{k}"]
            assert np.array_equal(got[0].view(np.uint32), wi), f"{dim}x{n} topk {k} ({name}): ids differ"
            assert_bits_equal(got[1], ws, f"{dim}x{n} topk {k} ({name}) scores")
            assert info[f"topk/{dim}x{n}/{k}"][0] == (1 if name == "blocked" else 0), (name, k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LAYOUT, ids=lambda c: f"{c[0]}x{c[1]}")
def test_blocked_layout_matches_numpy_packer(runs, case):
    dim, n = case
    R, info = runs["blocked"]
    rc = actual_dim(dim) // 16
    assert info[f"layout/{dim}x{n}"] == [rc - rc // 8, BLOCK]
    assert runs["bytes"][1][f"layout/{dim}x{n}"][0] == 0
    rows, _ = store_rows(dim, n)
    want = numpy_pack_blocked(rows[:, 4:])
    assert np.array_equal(R[f"layout/{dim}x{n}"], want.reshape(-1)), f"{dim}x{n}: blocked image"
