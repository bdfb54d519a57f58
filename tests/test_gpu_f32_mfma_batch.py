"""OriginalVectors.topk_batch through f32_mfma_filter_kernel (csrc/f32_mfma.hip): ids and score bits must be those of the single-query
top-k and, one case per element type, of the oracle's qo_metric_f32 over the widened rows.  70 003 rows: a multiple of no tile."""
import functools
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

import util
from oracle import qoracle as qo

pytestmark = pytest.mark.gpu
qa = pytest.importorskip("quantization_amd")
from quantization_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 70_003


def narrow(data, kind):
    if kind == "f16":
        return data.astype(np.float16)
    u = data.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def widen(stored, kind):
    return stored.astype(np.float32) if kind == "f16" else (stored.astype(np.uint32) << 16).view(np.float32)


@functools.lru_cache(maxsize=None)
def uniform_rows(dim):
    return (np.random.default_rng(dim).random((N, dim), dtype=np.float32) - np.float32(0.5)).astype(np.float32)


def make_queries(nq, dim):
    return (np.random.default_rng(1000 + nq + dim).random((nq, dim), dtype=np.float32) - np.float32(0.5)).astype(np.float32)


def store(rows, kind, invert=False, dist=None):
    vp = qa.VectorParameters(rows.shape[1], rows.shape[0], qa.DistanceType.Dot if dist is None else dist, invert)
    return qa.OriginalVectors.from_data(rows if kind == "f32" else narrow(rows, kind), vp, dtype=kind)


def topk_prefix(ov, queries, k, largest, n_ids):
    nq, dim = queries.shape
    ids, sc = np.empty((nq, k), np.uint32), np.empty((nq, k), np.float32)
    st = _lib.lib().qamd_f32_rerank_batch(ov._h, queries.ctypes.data, nq, dim, _lib.MEM_HOST, None, n_ids, _lib.MEM_DEVICE, k,
                                          int(largest), ids.ctypes.data, sc.ctypes.data, _lib.MEM_HOST, None)
    assert st == _lib.OK, _lib.lib().qamd_last_error()
    return ids, sc


def check(ov, queries, k, n_ids=None, oracle=None):
    """topk_batch == the single-query loop, both directions; with `oracle` (the widened rows, invert) query 2 against qo_metric_f32."""
    for largest in (True, False):
        ids, sc = ov.topk_batch(queries, k, largest=largest) if n_ids is None else topk_prefix(ov, queries, k, largest, n_ids)
        for qi in range(len(queries)):
            wi, ws = ov.topk(queries[qi], k, largest=largest) if n_ids is None else topk_prefix(ov, queries[qi:qi + 1], k, largest, n_ids)
            assert np.array_equal(ids[qi], np.ravel(wi)), (qi, largest)
            util.assert_bits_equal(sc[qi], np.ravel(ws), f"query {qi} largest {largest}")
        if oracle is not None:
            (rows, invert), q = oracle, np.ascontiguousarray(queries[2])
            fn, dim, base = qo.lib().qo_metric_f32, rows.shape[1], rows.ctypes.data
            exact = np.array([fn(qo.DOT, q.ctypes.data, base + i * dim * 4, dim) for i in range(N)], dtype=np.float32)
            wi, ws = util.topk_total_order(-exact if invert else exact, k, largest)
            assert np.array_equal(ids[2], wi) and np.array_equal(util.bits(sc[2]), util.bits(ws)), "vs oracle"


# dim: less than one K step of 16, one and a half, a K tail (264 = 4 * 64 + 8), the workload's row; nq: a whole group of 16, one
# more, an odd count; k and invert rotate over the cases (k = 1024 keeps the scan route here: its sample would be half the store)
CASES = [(kind, dim, nq, (1, 100, 1024)[(i + i // 3) % 3], bool((i // 3 + i // 12) % 2))
         for i, (kind, dim, nq) in enumerate(itertools.product(("f16", "bf16"), (8, 24, 264, 768), (16, 17, 33)))]


@pytest.mark.parametrize("kind,dim,nq,k,invert", CASES)
def test_batch_equals_single_query_loop(kind, dim, nq, k, invert):
    rows = uniform_rows(dim)
    check(store(rows, kind, invert), make_queries(nq, dim), k,
          oracle=(widen(narrow(rows, kind), kind), invert) if (dim, nq) == (264, 17) else None)


@pytest.mark.parametrize("case", ["ties", "inf_nan_rows", "queries", "huge_amax", "upsert", "prefix"])
def test_hard_inputs(case):
    """Ties at the threshold; an infinite and a NaN row (every query is redone); a query that cannot be bounded and one of zeros; a
    huge amax (everything survives: redone); a row above amax written by upsert after the first batch; a prefix of the rows."""
    kind, dim = ("f16", "bf16")[len(case) % 2], 264
    rows, queries = uniform_rows(dim).copy(), make_queries(17, dim)
    if case == "ties":
        rows[::2] = rows[1]
    elif case == "inf_nan_rows":
        rows[5, 0], rows[9, 0] = np.inf, np.nan
    elif case == "queries":
        queries[1, 3], queries[4] = np.inf, 0.0
    elif case == "huge_amax":
        rows[77] *= np.float32(3.0e4)
    ov = store(rows, kind)
    check(ov, queries, 100, n_ids=40_000 if case == "prefix" else None)
    if case == "upsert":
        ov.upsert(1234, rows[1234:1235] * np.float32(64.0))
        check(ov, queries, 100)


CHILD = """
import sys; sys.path[:0] = [{root!r}, {tests!r}]
import numpy as np, quantization_amd as qa, test_gpu_f32_mfma_batch as t
ov = t.store(t.uniform_rows(264), {kind!r}, dist=getattr(qa.DistanceType, {dist!r}))
t.check(ov, t.make_queries({nq}, 264), 100)
print("ok")
"""


# the uniform bf16 case fills at most 1500 of a list's 8192 slots (S = 8192: about k n / S = 855 rows pass): nothing is redone
@pytest.mark.parametrize("kind,dist,nq,switch,want", [("bf16", "Dot", 17, None, "0 queries redone"), ("bf16", "Dot", 17, "0", None),
                                                      ("bf16", "Dot", 15, None, None), ("f32", "Dot", 17, None, None),
                                                      ("bf16", "L2", 17, None, None)])
def test_route(kind, dist, nq, switch, want):
    """The developer library's debug line names the filter; the switch, 15 queries, f32 and L2 keep the scan route: no line."""
    dev_lib = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")
    if not os.path.exists(dev_lib):
        pytest.skip("developer build not present")
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), kind=kind, dist=dist, nq=nq)
    env = dict(os.environ, QAMD_LIB_PATH=dev_lib, QAMD_DEBUG_TOPK="1", **({} if switch is None else {"QAMD_F32_MFMA": switch}))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), (res.stdout + res.stderr)[-3000:]
    lines = [ln for ln in res.stderr.splitlines() if ln.startswith("[qamd f32_topk_batch]")]
    if want is None:
        assert not lines, lines
    else:  # one call per direction
        assert len(lines) == 2 and all("f32_mfma_filter_kernel" in ln and ln.endswith(want) for ln in lines), res.stderr[-3000:]
