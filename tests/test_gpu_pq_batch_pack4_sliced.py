"""PQ topk_batch through pq_scan_pack4_kernel<SLICED>: rows of 160, 192, 224 and 256 chunks, whose packed 8-bit table no longer
fits the LDS, take the four-query filter pass slice by slice over the planar scan image; a row's four 16-bit sums wait in one
8-byte word between the slice launches (csrc/pq_pack4.hpp, csrc/pq.hip).  Ids and score bits must be the single-query top-k's
and, one case per metric, the oracle's.  k > 64 and 70 003 rows as in test_gpu_pq_batch_pack4.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
D = qa.DistanceType
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, CHUNK = 70_003, 2
METRICS = {"dot": (D.Dot, False), "l2": (D.L2, True), "l1": (D.L1, True)}


def _check(m, metric, queries, k, rows=None, qo=None, plant=False):
    """topk_batch == the single-query loop, both directions; with `qo`, query 2 (inside a group) against the oracle's scores.
    plant: rows 11.. and 40 011.. get, in every chunk, the code of the largest / smallest entry of query 0's table."""
    dist, invert = METRICS[metric]
    rng = np.random.default_rng(1000 * m)
    cen = (rng.random((256, m * CHUNK), dtype=np.float32) - 0.5).astype(np.float32)
    rows = rng.integers(0, 256, size=(N, m), dtype=np.uint8) if rows is None else rows
    if plant:
        lut = qo.pq_encode_query(queries[0], CHUNK, cen, int(dist), invert).reshape(m, 256)
        rows[11:14], rows[40_011:40_014] = lut.argmax(axis=1).astype(np.uint8), lut.argmin(axis=1).astype(np.uint8)
    enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(m * CHUNK, N, dist, invert), CHUNK, cen)
    for largest in (True, False):
        ids, sc = enc.topk_batch(enc.encode_query_batch(queries), k, largest=largest)
        qobj = None
        for qi in range(len(queries)):
            qobj = enc.encode_query(queries[qi], reuse=qobj)
            wi, ws = enc.topk(qobj, k, largest=largest)
            assert np.array_equal(ids[qi], wi), (m, metric, qi, largest)
            assert np.array_equal(sc[qi].view(np.uint32), ws.view(np.uint32)), (m, metric, qi, largest)
        if plant:
            assert set(range(11, 14) if largest else range(40_011, 40_014)) <= set(ids[0].tolist())
        elif qo is not None:
            want = qo.pq_score_all(rows, qo.pq_encode_query(queries[2], CHUNK, cen, int(dist), invert), order=qo.ORDER_SSE)
            order = np.lexsort((np.arange(N), -want if largest else want))[:k]
            assert np.array_equal(ids[2], order) and np.array_equal(sc[2].view(np.uint32), want[order].view(np.uint32)), "vs oracle"


# m: 128 + 32, 96 + 96, 128 + 96, 128 + 128 chunks; Q: whole groups, a last group of 3 (7), of 1 (5, 9)
@pytest.mark.parametrize("m,metric,nq,k", [(m, metric, (4, 5, 7, 9)[(i + j) % 4], (65, 100)[(i + j) % 2])
                                           for i, m in enumerate((160, 192, 224, 256)) for j, metric in enumerate(METRICS)])
def test_batch_equals_single_query_loop(m, metric, nq, k, qo):
    queries = (np.random.default_rng(m + nq).random((nq, m * CHUNK), dtype=np.float32) - 0.5).astype(np.float32)
    _check(m, metric, queries, k, qo=qo if m == 192 else None)


@pytest.mark.parametrize("ties", [False, True])
def test_hard_inputs(ties):
    """Ties at the pivot (half the rows are copies of one row); a huge coordinate (a coarse step: nearly every row passes the
    integer test); queries that cannot be bounded - an infinite coordinate, all zeros (step 0) - and take the exact route."""
    rows = np.random.default_rng(5).integers(0, 256, size=(N, 192), dtype=np.uint8)
    if ties:
        rows[::2] = rows[1]
    queries = (np.random.default_rng(6).random((7, 192 * CHUNK), dtype=np.float32) - 0.5).astype(np.float32)
    queries[1, 17], queries[2, 40], queries[5] = 1.0e6, np.inf, 0.0
    _check(192, "dot", queries, 100, rows=rows)


def test_field_width(qo):
    """m = 256: rows whose every code is the best (worst) of query 0's table have entry 255 in all 256 chunks, the integer sum
    65280 that just fits 16 bits - a carry into the neighbouring field, or a lost word between the slices, changes the answer."""
    queries = (np.random.default_rng(8).random((4, 256 * CHUNK), dtype=np.float32) - 0.5).astype(np.float32)
    _check(256, "dot", queries, 100, qo=qo, plant=True)


@pytest.mark.parametrize("m,pack4,want", [(192, None, "side by side 2 x 4, filter pq_scan_pack4_kernel<SLICED>, 0 queries redone"),
                                          (192, "0", "side by side 0 x 0, filter pq_scan_skew_kernel<SLICED>, 0 queries redone"),
                                          (288, None, "side by side 0 x 0, filter pq_scan_skew_kernel<SLICED>, 0 queries redone"),
                                          (288, "0", "side by side 0 x 0, filter pq_scan_skew_kernel<SLICED>, 0 queries redone")])
def test_route(m, pack4, want):
    """The developer library's debug line names the filter that ran; QAMD_PQ_PACK4=0 (developer switch) and rows past 256 chunks
    are the pass per query."""
    dev_lib = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")
    if not os.path.exists(dev_lib):
        pytest.skip("developer build not present")
    code = f"""
import sys; sys.path.insert(0, {ROOT!r})
import numpy as np, quantization_amd as qa
rng = np.random.default_rng(3)
cen = (rng.random((256, {2 * m}), dtype=np.float32) - 0.5).astype(np.float32)
rows = rng.integers(0, 256, size=({N}, {m}), dtype=np.uint8)
enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters({2 * m}, {N}, qa.DistanceType.Dot, False), 2, cen)
enc.topk_batch(enc.encode_query_batch((rng.random((8, {2 * m}), dtype=np.float32) - 0.5).astype(np.float32)), 100)
print("ok")
"""
    env = dict(os.environ, QAMD_LIB_PATH=dev_lib, QAMD_DEBUG_TOPK="1", **({} if pack4 is None else {"QAMD_PQ_PACK4": pack4}))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), (res.stdout + res.stderr)[-3000:]
    lines = [ln for ln in res.stderr.splitlines() if ln.startswith("[qamd fused_topk_batch]")]
    assert len(lines) == 1 and lines[0].endswith(want), res.stderr[-3000:]
