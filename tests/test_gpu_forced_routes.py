"""Routes that only huge stores and partitioned GPUs take, forced at small shapes and checked against the oracle.

Some dispatch gates depend on a store size no test can afford or on a device property that never changes on the test
machine.  The developer library (tools/lib, -DQAMD_DEV) lets a test move them (csrc/common.hpp):
  QAMD_DEV_PQ_PLANAR_ROWS   pq.hip alloc_store: from this many rows (2^28) a PQ store keeps no planar scan image; rows of
                            m > 144 chunks then sit on a 128-byte pitch and pq_scan_fast_kernel scans them slice by slice
  QAMD_DEV_PQ_SKEW_ROWS     skew_rows_per_ring_row / skew_padded_ring: from this many rows (2^30) no pq_scan_skew_kernel
  QAMD_DEV_CU_COUNT         device_info().cu_count: every grid, the side-by-side PQ filter and the rq kernels (256 CUs only)
  QAMD_DEV_STAGE_BYTES      every 256 MiB host staging piece and 8 GiB device batch of the encoders, loads and exports
  QAMD_DEV_HOST_WHOLE=0     the one-shot u8 encoder keeps host input on the host (min/max, quantile sample, quantize staged)
None of these routes may change a result: every score is an exact function of the codes in a fixed lane order, and the
k-means sums run in ascending row order whatever the segment count.  So each configuration runs in a fresh child process
(the variables are read once per process), writes its results to an .npz, and the parent compares them bit for bit with
the oracle and with the same calls on the default route.  The kernel name (scan_kernel) or the QAMD_DEBUG_TOPK line of
each call proves that the forced route really ran.
"""
import json
import os
import re
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

GATE = 7001  # the forced row threshold of the planar image and of the skew kernel (fast_capable needs n >= 4096)
BIG = (1 << 20) + 7  # side-by-side PQ filter: n >= 2^20
STAGE = 1_000_003  # forced staging bytes: pieces of a ragged number of rows, none of them a multiple of 16
KS = (1, 50, 1024)

CONFIGS = {
    "planar": ({"QAMD_DEV_PQ_PLANAR_ROWS": str(GATE)}, ["pq_planar"]),
    "skew": ({"QAMD_DEV_PQ_PLANAR_ROWS": str(GATE), "QAMD_DEV_PQ_SKEW_ROWS": str(GATE)}, ["pq_skew"]),
    "cu256": ({}, ["cu"]),
    "cu32": ({"QAMD_DEV_CU_COUNT": "32"}, ["cu"]),
    "cu64": ({"QAMD_DEV_CU_COUNT": "64"}, ["cu"]),
    "cu128": ({"QAMD_DEV_CU_COUNT": "128"}, ["cu"]),
    "cu40": ({"QAMD_DEV_CU_COUNT": "40"}, ["cu"]),
    "stage": ({"QAMD_DEV_STAGE_BYTES": str(STAGE), "QAMD_DEV_HOST_WHOLE": "0"}, ["stage"]),
    "stage_default": ({}, ["stage"]),
}
ALL_OVERRIDES = {"QAMD_DEV_PQ_PLANAR_ROWS": str(GATE), "QAMD_DEV_PQ_SKEW_ROWS": str(GATE), "QAMD_DEV_CU_COUNT": "40",
                 "QAMD_DEV_STAGE_BYTES": str(STAGE), "QAMD_DEV_HOST_WHOLE": "0"}


# ------------------------------------------------------------------ inputs (the child and the parent draw the same ones)
def pq_case(m, n, chunk=1, seed=0, nq=2):
    rng = np.random.default_rng(m * 7919 + n + seed)
    dim = m * chunk
    cen = (rng.random((256, dim), dtype=np.float32) - 0.5).astype(np.float32)
    rows = rng.integers(0, 256, size=(n, m), dtype=np.uint8)
    queries = (rng.random((nq, dim), dtype=np.float32) - 0.5).astype(np.float32)
    return rows, cen, queries


def pq_data(m, n, seed=0):
    """Float rows for the PQ encoders (chunk 1) and the centroids they are encoded with."""
    rng = np.random.default_rng(m * 31 + n + seed)
    return ((rng.random((n, m), dtype=np.float32) - 0.5).astype(np.float32),
            (rng.random((256, m), dtype=np.float32) - 0.5).astype(np.float32))


def u8_data(n, dim, seed=0, grow=True):
    """grow: rows whose spread grows with the row id, so that a quantile sample of the first rows differs from the strided
    one (the best rows of a query then sit at the end of the store: do not use such rows for the top-k routes)."""
    rng = np.random.default_rng(n + dim + seed)
    data = rng.standard_normal((n, dim)).astype(np.float32)
    if grow:
        data *= (1.0 + 3.0 * np.arange(n, dtype=np.float32) / n)[:, None]
    return data


def bin_data(n, dim, seed=0):
    return np.random.default_rng(n + dim + seed).standard_normal((n, dim)).astype(np.float32)


def ragged(data, sizes=(1000, 2503, 777)):
    """make_batches for encode_stream: batches of the given sizes, then the rest."""
    def make():
        r = 0
        for s in sizes:
            if r < data.shape[0]:
                yield data[r:r + s]
                r += s
        if r < data.shape[0]:
            yield data[r:]
    return make


PLANAR_SHAPES = [(m, n) for m in (192, 288, 256, 512) for n in (20_011, GATE)]
SKEW_SHAPES = [(m, GATE) for m in (16, 32, 48, 64, 80, 96, 100, 112, 128, 192)] + [(16, 20_011), (48, 20_013)]
# 768-byte rows: 129 .. 192 queries fit one group of rq tiles (u8_gemm_rk16_kernel at 256 CUs); 200 need two, which the
# queries-in-registers kernel keeps up to 256 queries (rq_selected)
U8_N, U8_DIM, U8_QS = 131_075, 768, (1, 7, 64, 160, 200)
KM_N, KM_DIM, KM_CHUNK = 6000, 64, 2  # 32 chunks: the segment count P = ceil(2 * cu / 32) capped by ceil(6000 / 1024)


# ------------------------------------------------------------------ the child: one configuration, results to an .npz
def _mark(name):
    print("STEP " + name, file=sys.stderr, flush=True)


def _pq_store_results(R, info, tag, enc, queries, rng_seed):
    info[tag + "/kernel"] = list(enc.scan_kernel())
    n = enc.count
    for qi, query in enumerate(queries):
        q = enc.encode_query(query)
        R[f"{tag}/q{qi}/all"] = enc.score_all(q)
        for k in KS:
            for largest in (True, False):
                ids, sc = enc.topk(q, k, largest=largest)
                R[f"{tag}/q{qi}/topk{k}{'L' if largest else 'S'}"] = np.stack([np.asarray(ids).view(np.float32), sc])
        ids = np.random.default_rng(rng_seed).permutation(n).astype(np.uint32)[:5000]
        R[f"{tag}/q{qi}/ids"] = ids
        R[f"{tag}/q{qi}/score_ids"] = enc.score_ids(q, ids)
    R[f"{tag}/internal"] = np.array([enc.score_internal(i, j) for i, j in ((0, n - 1), (n // 2, 3), (n - 1, n - 2))],
                                    dtype=np.float32)
    R[f"{tag}/export"] = enc.storage_bytes()
    R[f"{tag}/range"] = enc.storage_rows(1001, n - 2000)


def _pq_batch(R, tag, enc, queries, ks):
    b = enc.encode_query_batch(queries)
    for k in ks:
        _mark(f"{tag}/batch{k}")
        ids, sc = enc.topk_batch(b, k)
        R[f"{tag}/batch{k}"] = np.stack([np.asarray(ids).view(np.float32), sc])


def step_pq_planar(R, info):
    for m, n in PLANAR_SHAPES:
        rows, cen, queries = pq_case(m, n)
        enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(m, n, D.Dot, False), 1, cen)
        _pq_store_results(R, info, f"pq{m}x{n}", enc, queries, m)
    for m in (192, 288, 256, 512):  # the same stores from the one-shot and the streaming encoder
        data, cen = pq_data(m, GATE)
        vp = qa.VectorParameters(m, GATE, D.Dot, False)
        for how, enc in (("encode", qa.EncodedVectorsPQ.encode(data, vp, 1, centroids=cen)),
                         ("stream", qa.EncodedVectorsPQ.encode_stream(ragged(data), vp, 1, centroids=cen))):
            info[f"enc{m}/{how}/kernel"] = list(enc.scan_kernel())
            R[f"enc{m}/{how}/rows"] = enc.storage_bytes()
            R[f"enc{m}/{how}/all"] = enc.score_all(enc.encode_query(data[5]))
    rows, cen, queries = pq_case(192, GATE - 1)  # one row short of the gate: the planar image is kept
    enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(192, GATE - 1, D.Dot, False), 1, cen)
    info["below/kernel"] = list(enc.scan_kernel())
    R["below/all"] = enc.score_all(enc.encode_query(queries[0]))
    rows, cen, queries = pq_case(192, BIG, nq=5)
    enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(192, BIG, D.Dot, False), 1, cen)
    info["big192/kernel"] = list(enc.scan_kernel())
    _pq_batch(R, "big192", enc, queries, (100, 1024))


def step_pq_skew(R, info):
    for m, n in SKEW_SHAPES:
        rows, cen, queries = pq_case(m, n, nq=3)
        enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(m, n, D.Dot, False), 1, cen)
        tag = f"pq{m}x{n}"
        info[tag + "/kernel"] = list(enc.scan_kernel())
        q = enc.encode_query(queries[0])
        R[tag + "/all"] = enc.score_all(q)
        for k in KS:
            for largest in (True, False):
                ids, sc = enc.topk(q, k, largest=largest)
                R[f"{tag}/topk{k}{'L' if largest else 'S'}"] = np.stack([np.asarray(ids).view(np.float32), sc])
        _pq_batch(R, tag, enc, queries, (10, 1024))
    for m in (16, 48, 96, 80):  # one row short of the gate: pq_scan_skew_kernel
        rows, cen, queries = pq_case(m, GATE - 1)
        enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(m, GATE - 1, D.Dot, False), 1, cen)
        info[f"below{m}/kernel"] = list(enc.scan_kernel())
        R[f"below{m}/all"] = enc.score_all(enc.encode_query(queries[0]))
    rows, cen, queries = pq_case(96, BIG, nq=5)
    enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(96, BIG, D.Dot, False), 1, cen)
    info["big96/kernel"] = list(enc.scan_kernel())
    _pq_batch(R, "big96", enc, queries, (1024,))


def step_cu(R, info):
    info["cu_count"] = int(qa.lib().qamd_dev_cu_count())
    data = u8_data(U8_N, U8_DIM, grow=False)
    enc = qa.EncodedVectorsU8.encode(data, qa.VectorParameters(U8_DIM, U8_N, D.Dot, False))
    R["u8/rows"] = enc.storage_bytes()
    queries = np.random.default_rng(3).standard_normal((max(U8_QS), U8_DIM)).astype(np.float32)
    q = enc.encode_query(queries[0])
    R["u8/all"] = enc.score_all(q)
    for k in (10, 1024):
        _mark(f"u8/topk{k}")
        ids, sc = enc.topk(q, k)
        R[f"u8/topk{k}"] = np.stack([np.asarray(ids).view(np.float32), sc])
    R["u8/score_batch"] = enc.score_batch(enc.encode_query_batch(queries[:7]))
    for nq in U8_QS:
        b = enc.encode_query_batch(queries[:nq])
        for k in (10, 1024):
            _mark(f"u8/batch{nq}/{k}")
            ids, sc = enc.topk_batch(b, k)
            R[f"u8/batch{nq}/{k}"] = np.stack([np.asarray(ids).view(np.float32), sc])
    # binary matrix cores (bin_gemm_rs4_kernel: 1024-bit rows, 12 queries)
    rows = np.random.default_rng(12).integers(0, 256, size=(100_003, 128), dtype=np.uint8)
    benc = qa.EncodedVectorsBin.from_storage(rows, qa.VectorParameters(1024, 100_003, D.Dot, False))
    bq = np.random.default_rng(13).standard_normal((12, 1024)).astype(np.float32)
    for k in (10, 1024):
        _mark(f"bin/batch{k}")
        ids, sc = benc.topk_batch(benc.encode_query_batch(bq), k)
        R[f"bin/batch{k}"] = np.stack([np.asarray(ids).view(np.float32), sc])
    ids, sc = benc.topk(benc.encode_query(bq[0]), 10)  # the single-launch small-store kernel
    R["bin/topk10"] = np.stack([np.asarray(ids).view(np.float32), sc])
    # PQ: the side-by-side filter (256 CUs) or query by query; the small-store kernel per query at k <= 64
    prow, cen, pqs = pq_case(96, BIG, nq=5)
    penc = qa.EncodedVectorsPQ.from_storage(prow, qa.VectorParameters(96, BIG, D.Dot, False), 1, cen)
    _pq_batch(R, "pq", penc, pqs, (10, 1024))
    ids, sc = penc.topk(penc.encode_query(pqs[0]), 10)
    R["pq/topk10"] = np.stack([np.asarray(ids).view(np.float32), sc])
    # u8 encoding with a quantile (min/max grid, strided sample gather) from HBM
    import torch
    qdata = u8_data(150_000, 64, seed=1)
    qenc = qa.EncodedVectorsU8.encode(torch.from_numpy(qdata).cuda(), qa.VectorParameters(64, 150_000, D.Dot, False),
                                      quantile=0.99)
    R["u8q/rows"] = qenc.storage_bytes()
    R["u8q/meta"] = np.array([qenc.metadata["alpha"], qenc.metadata["offset"]], dtype=np.float32)
    # PQ k-means: the segment count of the grouping step follows the CU count
    kdata = np.random.default_rng(77).random((KM_N, KM_DIM), dtype=np.float32)
    R["km/centroids"] = qa.EncodedVectorsPQ.find_centroids(kdata, KM_CHUNK)


def step_stage(R, info):
    vp = qa.VectorParameters(64, 150_000, D.Dot, False)
    data = u8_data(150_000, 64, seed=2)
    for tag, quantile in (("plain", None), ("q99", 0.99)):
        for how, enc in (("encode", qa.EncodedVectorsU8.encode(data, vp, quantile=quantile)),
                         ("stream", qa.EncodedVectorsU8.encode_stream(ragged(data, (20_000, 33_333, 7)), vp,
                                                                      quantile=quantile))):
            R[f"u8/{tag}/{how}/rows"] = enc.storage_bytes()
            R[f"u8/{tag}/{how}/meta"] = np.array([enc.metadata["alpha"], enc.metadata["offset"]], dtype=np.float32)
        if quantile is not None:
            back = qa.EncodedVectorsU8.from_storage(R[f"u8/{tag}/encode/rows"], enc.metadata)
            R["u8/range"] = back.storage_rows(10_001, 100_000)
            R["u8/all"] = back.score_all(back.encode_query(data[9]))
    bdata = bin_data(20_011, 1000)
    bvp = qa.VectorParameters(1000, 20_011, D.Dot, False)
    for store in (qa.BitsStoreType.U8, qa.BitsStoreType.U128):
        for how, enc in (("encode", qa.EncodedVectorsBin.encode(bdata, bvp, store=store)),
                         ("stream", qa.EncodedVectorsBin.encode_stream(ragged(bdata), bvp, store=store))):
            R[f"bin{int(store)}/{how}/rows"] = enc.storage_bytes()
        back = qa.EncodedVectorsBin.from_storage(R[f"bin{int(store)}/encode/rows"], bvp, store=store)
        R[f"bin{int(store)}/range"] = back.storage_rows(3001, 15_000)
    pdata, cen = pq_data(192, 20_011)
    pvp = qa.VectorParameters(192, 20_011, D.Dot, False)
    for how, enc in (("encode", qa.EncodedVectorsPQ.encode(pdata, pvp, 1, centroids=cen)),
                     ("stream", qa.EncodedVectorsPQ.encode_stream(ragged(pdata), pvp, 1, centroids=cen))):
        info[f"pq/{how}/kernel"] = list(enc.scan_kernel())
        R[f"pq/{how}/rows"] = enc.storage_bytes()
        R[f"pq/{how}/all"] = enc.score_all(enc.encode_query(pdata[3]))  # through the planar image
    back = qa.EncodedVectorsPQ.from_storage(R["pq/encode/rows"], pvp, 1, cen)
    R["pq/range"] = back.storage_rows(3001, 15_000)
    tdata = np.random.default_rng(5).random((KM_N + 1, 16), dtype=np.float32)
    tvp = qa.VectorParameters(16, KM_N + 1, D.L2, False)
    for how, enc in (("encode", qa.EncodedVectorsPQ.encode(tdata, tvp, 2)),
                     ("stream", qa.EncodedVectorsPQ.encode_stream(ragged(tdata), tvp, 2))):
        R[f"pqt/{how}/rows"] = enc.storage_bytes()
        R[f"pqt/{how}/centroids"] = enc.centroids


def step_guard(R, info):
    rows, cen, queries = pq_case(192, GATE)
    enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(192, GATE, D.Dot, False), 1, cen)
    info["guard/kernel"] = list(enc.scan_kernel())
    R["guard/all"] = enc.score_all(enc.encode_query(queries[0]))
    data = u8_data(40_000, 64, seed=4)
    uenc = qa.EncodedVectorsU8.encode(data, qa.VectorParameters(64, 40_000, D.Dot, False))
    R["guard/u8rows"] = uenc.storage_bytes()
    ids, sc = uenc.topk_batch(uenc.encode_query_batch(data[:20]), 100)
    R["guard/u8batch"] = np.stack([np.asarray(ids).view(np.float32), sc])


STEPS = {"pq_planar": step_pq_planar, "pq_skew": step_pq_skew, "cu": step_cu, "stage": step_stage, "guard": step_guard}


def child_main(steps, out_path):
    R, info = {}, {}
    for s in steps:
        _mark(s)
        STEPS[s](R, info)
    _mark("end")
    np.savez(out_path, **R)
    with open(out_path + ".json", "w") as f:
        json.dump(info, f)
    print("DONE")


# ------------------------------------------------------------------ the parent
def run_child(tmp_dir, name, env_add, steps, lib=DEV_LIB, timeout=900):
    """Runs `steps` in a fresh process on `lib` (None: the product library) with QAMD_DEBUG_TOPK=1 and `env_add`;
    returns (results, info, {step mark: [debug lines]})."""
    assert os.path.exists(DEV_LIB), "the developer library is built with the product one (make -C quantization_amd/csrc)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
    env.update(env_add, QAMD_DEBUG_TOPK="1")
    if lib:
        env["QAMD_LIB_PATH"] = lib
    out = os.path.join(str(tmp_dir), name + ".npz")
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_forced_routes as T\nT.child_main(%r, %r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), steps, out))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=env)
    assert res.returncode == 0 and "DONE" in res.stdout, f"{name}: exit {res.returncode}\n{res.stderr[-4000:]}"
    lines, cur = {}, None
    for ln in res.stderr.splitlines():
        if ln.startswith("STEP "):
            cur = ln[5:].strip()
            lines.setdefault(cur, [])
        elif ln.startswith("[qamd"):
            lines.setdefault(cur, []).append(ln)
    with open(out + ".json") as f:
        info = json.load(f)
    return dict(np.load(out)), info, lines


_RUNS = {}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Each configuration's child, run once per module (several tests read the default runs)."""
    d = tmp_path_factory.mktemp("forced_routes")

    def get(name):
        if name not in _RUNS:
            env_add, steps = CONFIGS[name]
            _RUNS[name] = run_child(d, name, env_add, steps)
        return _RUNS[name]
    yield get
    _RUNS.clear()


def _topk_equal(got, scores, k, largest, tag):
    ids = got[0].view(np.uint32)
    wi, ws = topk_want(scores, k, largest)
    if not np.array_equal(ids, wi):
        bad = np.flatnonzero(ids != wi)
        raise AssertionError(f"{tag}: {bad.size} ids differ, first at {bad[0]}: got {ids[bad[0]]} want {wi[bad[0]]}")
    assert_bits_equal(got[1], ws, tag + " scores")


def _batch_equal(got, wants, k, tag, largest=True):
    for qi, w in wants.items():
        _topk_equal(got[:, qi], w, k, largest, f"{tag} query {qi}")


def _pq_want(qo, rows, cen, query, chunk=1):
    return qo.pq_score_all(rows, qo.pq_encode_query(query, chunk, cen, qo.DOT, False), order=qo.ORDER_SSE)


def _side_by_side(lines):
    """(launches, width) of the '[qamd fused_topk_batch] ... side by side L x W' lines; None when there is no such line."""
    got = [re.search(r"side by side (\d+) x (\d+),", ln) for ln in lines if ln.startswith("[qamd fused_topk_batch]")]
    got = [g for g in got if g]
    return (sum(int(g.group(1)) for g in got), max(int(g.group(2)) for g in got)) if got else None


def _redone(lines):
    return sum(int(re.search(r"(\d+) queries redone$", ln).group(1)) for ln in lines)


# ------------------------------------------------------------------ a. PQ without a planar image
def test_pq_fast_kernel_no_planar_image(runs, qo):
    """QAMD_DEV_PQ_PLANAR_ROWS=7001: rows of m = 192 / 288 / 256 / 512 chunks on the 128-byte pitch, pq_scan_fast_kernel in
    ceil(m / 128) slices through the 16 B/row partial sums; every entry point against the oracle, stores from the given rows,
    the one-shot encoder and the streaming encoder; 7000 rows keep the image (the gate is count >= threshold)."""
    R, info, lines = runs("planar")
    for m, n in PLANAR_SHAPES:
        tag = f"pq{m}x{n}"
        rows, cen, queries = pq_case(m, n)
        assert info[tag + "/kernel"] == ["pq_scan_fast_kernel", -(-m // 128)], (tag, info[tag + "/kernel"])
        for qi, query in enumerate(queries):
            want = _pq_want(qo, rows, cen, query)
            assert_bits_equal(R[f"{tag}/q{qi}/all"], want, f"{tag} score_all")
            for k in KS:
                for largest in (True, False):
                    _topk_equal(R[f"{tag}/q{qi}/topk{k}{'L' if largest else 'S'}"], want, k, largest, f"{tag} topk {k}")
            assert_bits_equal(R[f"{tag}/q{qi}/score_ids"], want[R[f"{tag}/q{qi}/ids"]], f"{tag} score_ids")
        internal = [qo.pq_score_internal(rows, m, 1, cen, qo.DOT, False, i, j) for i, j in ((0, n - 1), (n // 2, 3), (n - 1, n - 2))]
        assert_bits_equal(R[tag + "/internal"], internal, f"{tag} score_internal")
        assert np.array_equal(R[tag + "/export"], rows), f"{tag} storage_bytes"
        assert np.array_equal(R[tag + "/range"], rows[1001:n - 999]), f"{tag} storage_rows"
    for m in (192, 288, 256, 512):
        data, cen = pq_data(m, GATE)
        want_rows = qo.pq_encode(data, 1, cen)
        want = _pq_want(qo, want_rows, cen, data[5])
        for how in ("encode", "stream"):
            assert info[f"enc{m}/{how}/kernel"][0] == "pq_scan_fast_kernel"
            assert np.array_equal(R[f"enc{m}/{how}/rows"], want_rows), f"m={m} {how}: codes"
            assert_bits_equal(R[f"enc{m}/{how}/all"], want, f"m={m} {how}: scores")
    rows, cen, queries = pq_case(192, GATE - 1)
    assert info["below/kernel"] == ["pq_scan_skew_kernel<SLICED>", 2], info["below/kernel"]
    assert_bits_equal(R["below/all"], _pq_want(qo, rows, cen, queries[0]), "7000 rows, planar image")
    # 2^20 + 7 rows: no planar image, so the side-by-side filter has nothing to launch and goes query by query
    rows, cen, queries = pq_case(192, BIG, nq=5)
    assert info["big192/kernel"] == ["pq_scan_fast_kernel", 2]
    wants = {qi: _pq_want(qo, rows, cen, q) for qi, q in enumerate(queries)}
    for k in (100, 1024):
        _batch_equal(R[f"big192/batch{k}"], wants, k, f"m=192 2^20+7 rows topk_batch k={k}")
        assert _side_by_side(lines[f"big192/batch{k}"]) == (0, 0), lines[f"big192/batch{k}"]


# ------------------------------------------------------------------ b. PQ past the skew limit
def test_pq_fast_kernel_past_skew_limit(runs, qo):
    """QAMD_DEV_PQ_SKEW_ROWS=7001 with QAMD_DEV_PQ_PLANAR_ROWS=7001 (at real size both gates are crossed together): whole
    rows (m = 32 .. 128), padded ring rows (m = 80, 100, 112) and two rows per ring row (m = 16, 48, odd n: a lone last row)
    all take pq_scan_fast_kernel; 7000 rows still take pq_scan_skew_kernel."""
    R, info, lines = runs("skew")
    for m, n in SKEW_SHAPES:
        tag = f"pq{m}x{n}"
        rows, cen, queries = pq_case(m, n, nq=3)
        assert info[tag + "/kernel"] == ["pq_scan_fast_kernel", -(-m // 128) if m > 144 else 1], (tag, info[tag + "/kernel"])
        want = _pq_want(qo, rows, cen, queries[0])
        assert_bits_equal(R[tag + "/all"], want, f"{tag} score_all")
        for k in KS:
            for largest in (True, False):
                _topk_equal(R[f"{tag}/topk{k}{'L' if largest else 'S'}"], want, k, largest, f"{tag} topk {k}")
        wants = {qi: _pq_want(qo, rows, cen, q) for qi, q in enumerate(queries)}
        for k in (10, 1024):
            _batch_equal(R[f"{tag}/batch{k}"], wants, k, f"{tag} topk_batch k={k}")
    for m in (16, 48, 96, 80):
        rows, cen, queries = pq_case(m, GATE - 1)
        assert info[f"below{m}/kernel"] == ["pq_scan_skew_kernel", 1], (m, info[f"below{m}/kernel"])
        assert_bits_equal(R[f"below{m}/all"], _pq_want(qo, rows, cen, queries[0]), f"m={m} 7000 rows")
    rows, cen, queries = pq_case(96, BIG, nq=5)
    assert info["big96/kernel"] == ["pq_scan_fast_kernel", 1]
    _batch_equal(R["big96/batch1024"], {qi: _pq_want(qo, rows, cen, q) for qi, q in enumerate(queries)}, 1024,
                 "m=96 2^20+7 rows topk_batch")
    assert _side_by_side(lines["big96/batch1024"]) == (0, 0), lines["big96/batch1024"]


# ------------------------------------------------------------------ c. partitioned devices
_CU_ORACLE = {}


def _cu_oracle(qo):
    """The oracle's answers for step_cu, computed once."""
    if _CU_ORACLE:
        return _CU_ORACLE
    O = _CU_ORACLE
    data = u8_data(U8_N, U8_DIM, grow=False)
    rows, meta = qo.u8_encode(data, qo.DOT, False)
    O["u8/rows"] = rows
    queries = np.random.default_rng(3).standard_normal((max(U8_QS), U8_DIM)).astype(np.float32)
    u8s = {}
    for qi in sorted({0, 1, 2, 3, 4, 5, 6, 63, 64, 150, 159, 160, 199}):
        codes, qoff = qo.u8_encode_query(meta, queries[qi])
        u8s[qi] = qo.u8_score_all(meta, rows, codes, qoff, order=qo.ORDER_SIMPLE)
    O["u8"] = u8s
    brows = np.random.default_rng(12).integers(0, 256, size=(100_003, 128), dtype=np.uint8)
    bq = np.random.default_rng(13).standard_normal((12, 1024)).astype(np.float32)
    O["bin"] = {qi: qo.bin_score_all(brows, qo.bin_encode(bq[qi][None, :])[0], 1024, qo.DOT, False) for qi in range(12)}
    prow, cen, pqs = pq_case(96, BIG, nq=5)
    O["pq"] = {qi: _pq_want(qo, prow, cen, q) for qi, q in enumerate(pqs)}
    qdata = u8_data(150_000, 64, seed=1)
    sample = qdata[qo.pq_sample_rows(150_000, 100_000).astype(np.int64)]
    alpha, offset = qo.alpha_offset(*qo.find_quantile_interval(sample, 0.99))
    O["u8q/rows"], _ = qo.u8_encode_with(qdata, qo.DOT, False, alpha, offset)
    O["u8q/meta"] = np.array([alpha, offset], dtype=np.float32)
    kdata = np.random.default_rng(77).random((KM_N, KM_DIM), dtype=np.float32)
    O["km/centroids"] = qo.find_centroids(kdata, KM_CHUNK)[0]
    return O


def _check_cu_run(R, lines, O, tag):
    assert np.array_equal(R["u8/rows"], O["u8/rows"]), f"{tag}: u8 codes"
    u8 = O["u8"]
    assert_bits_equal(R["u8/all"], u8[0], f"{tag}: u8 score_all")
    for k in (10, 1024):
        _topk_equal(R[f"u8/topk{k}"], u8[0], k, True, f"{tag}: u8 topk {k}")
    assert_bits_equal(R["u8/score_batch"], np.stack([u8[qi] for qi in range(7)]), f"{tag}: u8 score_batch")
    for nq in U8_QS:
        for k in (10, 1024):
            _batch_equal(R[f"u8/batch{nq}/{k}"], {qi: s for qi, s in u8.items() if qi < nq}, k, f"{tag}: u8 topk_batch Q={nq} k={k}")
    for k in (10, 1024):
        _batch_equal(R[f"bin/batch{k}"], O["bin"], k, f"{tag}: binary topk_batch k={k}")
        _batch_equal(R[f"pq/batch{k}"], O["pq"], k, f"{tag}: PQ topk_batch k={k}")
    _topk_equal(R["bin/topk10"], O["bin"][0], 10, True, f"{tag}: binary small-store topk")
    _topk_equal(R["pq/topk10"], O["pq"][0], 10, True, f"{tag}: PQ small-store topk")
    assert np.array_equal(R["u8q/rows"], O["u8q/rows"]), f"{tag}: u8 codes with quantile 0.99"
    assert_bits_equal(R["u8q/meta"], O["u8q/meta"], f"{tag}: u8 (alpha, offset) with quantile 0.99")
    assert_bits_equal(R["km/centroids"], O["km/centroids"], f"{tag}: k-means centroids")


def test_default_device_routes(runs, qo):
    """The unforced run (256 CUs) against the oracle; its debug lines show the routes a partitioned device must not take:
    the rq kernel for 160 queries on 768-byte rows and the side-by-side PQ filter."""
    R, info, lines = runs("cu256")
    if info["cu_count"] != 256:
        pytest.fail(f"the test machine reports {info['cu_count']} CUs, not an unpartitioned MI355X")
    _check_cu_run(R, lines, _cu_oracle(qo), "256 CUs")
    assert any("filter u8_gemm_rk16_kernel," in ln for ln in lines["u8/batch160/1024"]), lines["u8/batch160/1024"]
    assert (_side_by_side(lines["pq/batch1024"]) or (0, 0))[0] >= 1, lines["pq/batch1024"]


@pytest.mark.parametrize("cus", [32, 64, 128, 40], ids=["cpx-32cu", "qpx-64cu", "dpx-128cu", "irregular-40cu"])
def test_partitioned_device(runs, qo, cus):
    """QAMD_DEV_CU_COUNT: every grid sized for a CPX / QPX / DPX partition (and an irregular 40): u8 scans, top-k and batches
    (no rq kernel), binary matrix cores, PQ batches query by query (no side-by-side filter), the small-store kernels, the
    quantile encode and k-means (a different segment count P) - all bit-identical to the oracle and to the 256-CU run."""
    R, info, lines = runs(f"cu{cus}")
    assert info["cu_count"] == cus
    _check_cu_run(R, lines, _cu_oracle(qo), f"{cus} CUs")
    R0, _, lines0 = runs("cu256")
    for key in R0:
        assert R[key].tobytes() == R0[key].tobytes(), f"{cus} CUs against 256: {key}"
    u8_rq = [ln for ln in lines["u8/batch160/1024"] if ln.startswith("[qamd topk_batch]")]
    assert u8_rq and all(re.search(r"filter u8_gemm_\w+,", ln) and not re.search(r"filter u8_gemm_r[qk]16_kernel", ln)
                         for ln in u8_rq), u8_rq
    assert _side_by_side(lines["pq/batch1024"]) == (0, 0), lines["pq/batch1024"]
    redone = {key: _redone(v) for key, v in lines.items() if key.endswith("/1024") or key.endswith("batch1024")}
    print(f"\nREDONE cu={cus} " + " ".join(f"{k}={v}" for k, v in sorted(redone.items())) +
          " | cu=256 " + " ".join(f"{k}={_redone(lines0[k])}" for k in sorted(redone)))


# ------------------------------------------------------------------ d. host-staged encoding
def test_host_staged_encoding(runs, qo):
    """QAMD_DEV_STAGE_BYTES=1000003, QAMD_DEV_HOST_WHOLE=0: the one-shot u8 encoder keeps 150_000 host rows on the host
    (min/max, the strided quantile sample gathered on the host, quantize - batch after batch at r0 > 0), the binary and PQ
    encoders (planar image built per batch), the streaming encoders, loads and exports in pieces of a ragged row count."""
    R, info, _ = runs("stage")
    R0, info0, _ = runs("stage_default")
    for key in R0:
        assert R[key].tobytes() == R0[key].tobytes(), f"staged against default: {key}"
    assert info == info0
    data = u8_data(150_000, 64, seed=2)
    rows, meta = qo.u8_encode(data, qo.DOT, False)
    sample = data[qo.pq_sample_rows(150_000, 100_000).astype(np.int64)]
    alpha, offset = qo.alpha_offset(*qo.find_quantile_interval(sample, 0.99))
    rows_q, meta_q = qo.u8_encode_with(data, qo.DOT, False, alpha, offset)
    for tag, (r, m) in (("plain", (rows, meta)), ("q99", (rows_q, meta_q))):
        for how in ("encode", "stream"):
            assert np.array_equal(R[f"u8/{tag}/{how}/rows"], r), f"u8 {tag} {how}: codes"
            assert_bits_equal(R[f"u8/{tag}/{how}/meta"], [m.alpha, m.offset], f"u8 {tag} {how}: (alpha, offset)")
    assert np.array_equal(R["u8/range"], rows_q[10_001:110_001]), "u8 storage_rows"
    codes, qoff = qo.u8_encode_query(meta_q, data[9])
    assert_bits_equal(R["u8/all"], qo.u8_score_all(meta_q, rows_q, codes, qoff), "u8 scores of the loaded store")
    bdata = bin_data(20_011, 1000)
    for store in (qo.STORE_U8, qo.STORE_U128):
        want = qo.bin_encode(bdata, store)
        for how in ("encode", "stream"):
            assert np.array_equal(R[f"bin{store}/{how}/rows"], want), f"binary store {store} {how}"
        assert np.array_equal(R[f"bin{store}/range"], want[3001:18_001]), f"binary store {store} storage_rows"
    pdata, cen = pq_data(192, 20_011)
    want_rows = qo.pq_encode(pdata, 1, cen)
    want = _pq_want(qo, want_rows, cen, pdata[3])
    for how in ("encode", "stream"):
        assert info[f"pq/{how}/kernel"] == ["pq_scan_skew_kernel<SLICED>", 2]
        assert np.array_equal(R[f"pq/{how}/rows"], want_rows), f"PQ {how}: codes"
        assert_bits_equal(R[f"pq/{how}/all"], want, f"PQ {how}: scores through the planar image")
    assert np.array_equal(R["pq/range"], want_rows[3001:18_001]), "PQ storage_rows"
    tdata = np.random.default_rng(5).random((KM_N + 1, 16), dtype=np.float32)
    tcen = qo.find_centroids(tdata, 2)[0]
    for how in ("encode", "stream"):
        assert_bits_equal(R[f"pqt/{how}/centroids"], tcen, f"PQ trained {how}: centroids")
        assert np.array_equal(R[f"pqt/{how}/rows"], qo.pq_encode(tdata, 2, tcen)), f"PQ trained {how}: codes"


# ------------------------------------------------------------------ e. the product library ignores every override
def test_product_library_ignores_overrides(tmp_path, qo):
    """Every QAMD_DEV_* variable set (and QAMD_DEBUG_TOPK): the product library keeps the planar image and the default
    routes, prints nothing and answers as the oracle."""
    R, info, lines = run_child(tmp_path, "guard", ALL_OVERRIDES, ["guard"], lib=None)
    assert not any(v for v in lines.values()), lines
    assert info["guard/kernel"] == ["pq_scan_skew_kernel<SLICED>", 2], info["guard/kernel"]
    rows, cen, queries = pq_case(192, GATE)
    assert_bits_equal(R["guard/all"], _pq_want(qo, rows, cen, queries[0]), "product library PQ scores")
    data = u8_data(40_000, 64, seed=4)
    urows, meta = qo.u8_encode(data, qo.DOT, False)
    assert np.array_equal(R["guard/u8rows"], urows), "product library u8 codes"
    for qi in (0, 19):
        codes, qoff = qo.u8_encode_query(meta, data[qi])
        _topk_equal(R["guard/u8batch"][:, qi], qo.u8_score_all(meta, urows, codes, qoff), 100, True, f"product topk_batch {qi}")
