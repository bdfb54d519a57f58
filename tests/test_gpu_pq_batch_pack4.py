"""PQ topk_batch through pq_scan_pack4_kernel: four queries share one filter pass through a packed 8-bit table (csrc/pq_pack4.hpp),
the exact f32 score of the survivors decides.  Ids and score bits must be the single-query top-k's and, one case per metric, the
oracle's.  k > 64 (below, small stores take the single-launch top-k); 70 003 rows reach the filter pass, a multiple of no block size."""
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


def _check(m, metric, queries, k, rows=None, qo=None):
    """topk_batch == the single-query loop, both directions; with `qo`, query 2 (inside a group) against the oracle's scores."""
    dist, invert = METRICS[metric]
    rng = np.random.default_rng(1000 * m)
    cen = (rng.random((256, m * CHUNK), dtype=np.float32) - 0.5).astype(np.float32)
    rows = rng.integers(0, 256, size=(N, m), dtype=np.uint8) if rows is None else rows
    enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(m * CHUNK, N, dist, invert), CHUNK, cen)
    for largest in (True, False):
        ids, sc = enc.topk_batch(enc.encode_query_batch(queries), k, largest=largest)
        qobj = None
        for qi in range(len(queries)):
            qobj = enc.encode_query(queries[qi], reuse=qobj)
            wi, ws = enc.topk(qobj, k, largest=largest)
            assert np.array_equal(ids[qi], wi), (m, metric, qi, largest)
            assert np.array_equal(sc[qi].view(np.uint32), ws.view(np.uint32)), (m, metric, qi, largest)
        if qo is not None:
            want = qo.pq_score_all(rows, qo.pq_encode_query(queries[2], CHUNK, cen, int(dist), invert), order=qo.ORDER_SSE)
            order = np.lexsort((np.arange(N), -want if largest else want))[:k]
            assert np.array_equal(ids[2], order) and np.array_equal(sc[2].view(np.uint32), want[order].view(np.uint32)), "vs oracle"


# m: 16, 48 two store rows per ring row, 80 padded, 96 plain, 128 the whole LDS; Q: whole groups, a last group of 3 (7), of 1 (5, 9)
@pytest.mark.parametrize("m,metric,nq,k", [(m, metric, (4, 5, 7, 9)[(i + j) % 4], (65, 100)[(i + j) % 2])
                                           for i, m in enumerate((16, 48, 80, 96, 128)) for j, metric in enumerate(METRICS)])
def test_batch_equals_single_query_loop(m, metric, nq, k, qo):
    queries = (np.random.default_rng(m + nq).random((nq, m * CHUNK), dtype=np.float32) - 0.5).astype(np.float32)
    _check(m, metric, queries, k, qo=qo if m == 96 else None)


@pytest.mark.parametrize("ties", [False, True])
def test_hard_inputs(ties):
    """Ties at the pivot (half the rows are copies of one row); a huge coordinate (a coarse step: nearly every row passes the
    integer test); queries that cannot be bounded - an infinite coordinate, all zeros (step 0) - and take the exact route."""
    rows = np.random.default_rng(5).integers(0, 256, size=(N, 96), dtype=np.uint8)
    if ties:
        rows[::2] = rows[1]
    queries = (np.random.default_rng(6).random((7, 96 * CHUNK), dtype=np.float32) - 0.5).astype(np.float32)
    queries[1, 17], queries[2, 40], queries[5] = 1.0e6, np.inf, 0.0
    _check(96, "dot", queries, 100, rows=rows)


@pytest.mark.parametrize("pack4,want", [(None, "side by side 2 x 4, filter pq_scan_pack4_kernel, 0 queries redone"),
                                        ("0", "side by side 0 x 0, filter pq_scan_skew_kernel, 0 queries redone")])
def test_route(pack4, want):
    """The developer library's debug line names the filter that ran; QAMD_PQ_PACK4=0 (developer switch) is the pass per query."""
    dev_lib = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")
    if not os.path.exists(dev_lib):
        pytest.skip("developer build not present")
    code = f"""
import sys; sys.path.insert(0, {ROOT!r})
import numpy as np, quantization_amd as qa
rng = np.random.default_rng(3)
cen = (rng.random((256, 192), dtype=np.float32) - 0.5).astype(np.float32)
rows = rng.integers(0, 256, size=({N}, 96), dtype=np.uint8)
enc = qa.EncodedVectorsPQ.from_storage(rows, qa.VectorParameters(192, {N}, qa.DistanceType.Dot, False), 2, cen)
enc.topk_batch(enc.encode_query_batch((rng.random((8, 192), dtype=np.float32) - 0.5).astype(np.float32)), 100)
print("ok")
"""
    env = dict(os.environ, QAMD_LIB_PATH=dev_lib, QAMD_DEBUG_TOPK="1", **({} if pack4 is None else {"QAMD_PQ_PACK4": pack4}))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), (res.stdout + res.stderr)[-3000:]
    lines = [ln for ln in res.stderr.splitlines() if ln.startswith("[qamd fused_topk_batch]")]
    assert len(lines) == 1 and lines[0].endswith(want), res.stderr[-3000:]
