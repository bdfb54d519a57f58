"""Full-range scalar-u8 stores on the GPU against u8_full_range_model's numpy restatement, on raw f32
bits: the encoder, every scoring call, and batches - which must equal the single-query answers bit for bit, through
u8_full_batch_kernel for the large ones and u8_scan_multi_kernel for the small ones (read from the developer library)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import u8_full_range_model as wm
import u8_rotated_model as um

qa = pytest.importorskip("quantization_amd")
pytestmark = pytest.mark.gpu

f32, u32 = np.float32, np.uint32
D = qa.DistanceType
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")
METRICS = [(D.Dot, False), (D.Dot, True), (D.L2, False), (D.L2, True), (D.L1, False), (D.L1, True)]


def same(got, want, what=""):
    assert np.array_equal(np.ascontiguousarray(got, f32).view(u32), np.ascontiguousarray(want, f32).view(u32)), what


def ranked(sc, k, largest=True, ids=None):
    """The best k of scores sc: the total order on the score bits, ties to the lower id."""
    key = np.ascontiguousarray(sc, f32).view(u32).astype(np.int64)
    key = np.where(key >> 31, 0x7FFFFFFF - (key & 0x7FFFFFFF), key + 0x80000000)
    ids = np.arange(sc.size) if ids is None else ids
    order = np.lexsort((ids, -key if largest else key))[:k]
    return ids[order].astype(u32), sc[order]


def check_topk(got, sc, k, what, largest=True, ids=None):
    wi, ws = ranked(sc, k, largest, ids)
    assert np.array_equal(got[0], wi), what
    same(got[1], ws, what)


# ------------------------------------------------------------------------------------------------------- encoder
def encoder_data(n, dim, nan):
    x = np.random.default_rng(dim * 1000 + n).random((n, dim), dtype=f32)
    x[0], x[n - 1] = 0.0, 1.0  # the min and the max row: alpha = 1 / 255
    if n > 4:
        x[1, :] = (f32(0.5) + np.arange(dim, dtype=f32) % 255) * (f32(1) / f32(255))  # exactly on code boundaries
        x[2, ::3], x[:, dim // 2] = f32(0.25), f32(0.75)  # a constant column set
        if nan:
            x[3, 0] = np.nan
    return x


@pytest.mark.parametrize("dim,rotated,dist", [(dim, rot, dist) for dim, rot in ((1, False), (15, False), (16, False), (65, False),
                                                                                  (768, False), (64, True), (192, True))
                                              for dist in (D.Dot, D.L2, D.L1) if not (rot and dist == D.L1)])  # (refused)
@pytest.mark.parametrize("n", [1, 130])
def test_encoder(dim, rotated, n, dist, tmp_path):
    import torch
    x = encoder_data(n, dim, nan=not rotated)
    y = um.rotate(x) if rotated else x
    alpha, offset = wm.interval(y)
    rows, meta = wm.encode(y, int(dist), dist != D.Dot, alpha, offset)
    vp = qa.VectorParameters(dim, n, dist, dist != D.Dot)
    for data in (x, torch.from_numpy(x).cuda()):
        enc = qa.EncodedVectorsU8.encode(data, vp, rotated=rotated, full_range=True)
        assert np.array_equal(enc.storage_bytes(), rows)
    assert enc.full_range and enc.bits == 8 and enc.scan_bytes_per_row() == meta["actual_dim"] + 4
    same(enc.metadata["alpha"], alpha)
    for step in (1, 63, 130):
        st = qa.EncodedVectorsU8.encode_stream(lambda: (x[i:i + step] for i in range(0, n, step)), vp, rotated=rotated, full_range=True)
        assert np.array_equal(st.storage_bytes(), rows), step
    assert np.array_equal(qa.EncodedVectorsU8.from_storage(rows, enc.metadata).storage_bytes(), rows)
    enc.save(tmp_path / "d.bin", tmp_path / "m.json")
    assert (tmp_path / "d.bin").read_bytes() == rows.tobytes()
    text = (tmp_path / "m.json").read_text()
    assert text.endswith(',"full_range":true}') and list(json.loads(text))[-1] == "full_range"
    back = qa.EncodedVectorsU8.load(tmp_path / "d.bin", tmp_path / "m.json", vp)
    assert back.full_range and back.rotated == rotated and np.array_equal(back.storage_bytes(), rows)
    qc, qoff = wm.encode_query(meta, um.rotate(x[n // 2])[0] if rotated else x[n // 2])
    eq = enc.encode_query(x[n // 2])
    assert np.array_equal(eq.encoded_query, qc)
    same(eq.offset, qoff)
    with pytest.raises(qa.EncodingError):
        enc.set_lane_mode(1)
    enc.set_lane_mode(0)


def test_quantile_interval_and_refusals(tmp_path):
    x = np.random.default_rng(5).standard_normal((500, 64)).astype(f32)
    lo, hi = qa.EncodedVectorsU8.find_quantile_interval(x, 0.99)
    rows, _ = wm.encode(x, 0, False, f32((hi - lo) / f32(255)), lo)
    enc = qa.EncodedVectorsU8.encode(x, qa.VectorParameters(64, 500, D.Dot, False), 0.99, full_range=True)
    assert np.array_equal(enc.storage_bytes(), rows)
    for what, st, want, out in wm.refusals(qa._lib, tmp_path):
        assert st == want and out is None, (what, st, want)


# ------------------------------------------------------------------------------------------------------- stores
@functools.lru_cache(maxsize=8)
def store(kind, dist, invert):
    """(encoded store, rows, meta, query values, originals): "all255_<dim>" (65 rows of 255s against a query of 255s), or
    "<dim>x<rows>" random rows with more than half of the codes above 127."""
    if kind.startswith("all255"):
        dim, n = int(kind.split("_")[1]), 65
        x, q = np.full((n, dim), 255.0, f32), np.full(dim, 300.0, f32)
        rows, meta = wm.encode(x, int(dist), invert, 1.0, 0.0)
    else:
        dim, n = map(int, kind.split("x"))
        rng = np.random.default_rng(dim + n)
        x = rng.random((n, dim), dtype=f32) ** f32(0.4)
        x[0, 0], x[0, -1] = 0.0, 1.0
        rows, meta = wm.encode(x, int(dist), invert, *wm.interval(x))
        assert n * dim < 64 or (rows[:, 4:4 + dim] > 127).mean() > 0.5
        q = rng.random(dim, dtype=f32) ** f32(0.4)
    vp = qa.VectorParameters(dim, n, dist, invert)
    md = {"actual_dim": meta["actual_dim"], "alpha": meta["alpha"], "offset": meta["offset"], "multiplier": meta["multiplier"],
          "vector_parameters": vp, "full_range": True}
    return qa.EncodedVectorsU8.from_storage(rows, md), rows, meta, q, qa.OriginalVectors.from_data(x, vp)


STORES = ["all255_260", "all255_16384", "768x33000"] + [f"{d}x{n}" for d in (16, 65, 768) for n in (1, 63, 64, 65, 4099)]


@pytest.mark.parametrize("kind", STORES)
@pytest.mark.parametrize("dist,invert", METRICS)
def test_every_scoring_call(kind, dist, invert):
    enc, rows, meta, qv, orig = store(kind, dist, invert)
    n = rows.shape[0]
    q = enc.encode_query(qv)
    qc, qoff = wm.encode_query(meta, qv)
    assert np.array_equal(q.encoded_query, qc)
    want = wm.scores(meta, rows, qc, qoff)
    if kind == "all255_260" and dist != D.L1:
        assert int(wm.pair_sums(meta, rows, qc)[0]) == 16906500 > 1 << 24
    same(enc.score_all(q), want, "score_all")
    k, i, sel = min(30, n), n // 3, np.array([0, n - 1, n // 2, 0], u32)
    check_topk(enc.topk(q, k), want, k, "topk")
    same(enc.score_ids(q, sel), want[sel], "score_ids")
    same(enc.score_point(q, n - 1), want[n - 1], "score_point")
    wint = wm.scores_internal(meta, rows, i)
    same(enc.score_internal(i, n - 1), wint[n - 1], "score_internal")
    same(enc.score_internal_ids(i, sel), wint[sel], "score_internal_ids")
    same(enc.score_internal_all(i), wint, "score_internal_all")
    check_topk(enc.topk_internal(i, k, largest=False), wint, k, "topk_internal", largest=False)
    offs = np.array([0, 2, 2, 4], u32)  # three lists, one empty
    same(enc.score_ids_batch(enc.encode_query_batch(np.stack([qv, qv, qv])), offs, sel), want[sel], "burst of score_point pairs")
    same(enc.score_internal_ids_batch(np.array([i, 0, i], u32), offs, sel), wint[sel], "burst of score_internal pairs")
    cand = np.sort(enc.topk(q, min(100, n))[0])  # the rescored top-k: the candidates re-ranked by the originals' exact metric
    check_topk(enc.topk_rescored(q, orig, qv, min(10, n), min(100, n)), orig.score_ids(qv, cand), min(10, n), "topk_rescored", ids=cand)


# ------------------------------------------------------------------------------------------------------- batches
# dims 64 / 200 (a padded last k-block) / 768: the register forms of 4 and 12 k-blocks; 1000: 16; all255_16384: the form
# that re-reads the query fragment, at the i32 edge of the bias identity; 64x1048576: four tiles per wave; 768x33000:
# topk_batch from the filter gate on
@pytest.mark.parametrize("kind,sizes", [("64x4099", (2, 3, 8, 9, 17, 130)), ("200x4099", (2, 3, 8, 9, 17, 130)),
                                        ("768x4099", (2, 3, 8, 9, 17, 130)), ("1000x130", (5, 17)), ("all255_16384", (3, 17)),
                                        ("64x1048576", (5,)), ("768x33000", (9,))])
@pytest.mark.parametrize("dist,invert", [(D.Dot, False), (D.L2, True)])
def test_batches(kind, sizes, dist, invert):
    enc, rows, meta, qv, _ = store(kind, dist, invert)
    n, dim = rows.shape[0], meta["dim"]
    qs = np.random.default_rng(dim).random((max(sizes), dim), dtype=f32) ** f32(0.4) * (f32(300) if kind.startswith("all255") else f32(1))
    want = np.stack([wm.scores(meta, rows, *wm.encode_query(meta, q)) for q in qs])
    for nq in sizes:
        b = enc.encode_query_batch(qs[:nq])
        got = enc.score_batch(b)
        same(got, want[:nq], f"score_batch of {nq}")
        same(got[nq - 1], enc.score_all(enc.encode_query(qs[nq - 1])), "the single-query answer")
        for k in (30, 1024) if n < 1 << 20 else ():
            ids, sc = enc.topk_batch(b, min(k, n))
            for j in (0, nq - 1):
                check_topk((ids[j], sc[j]), want[j], min(k, n), f"topk_batch({k}) of {nq}, query {j}")
        lrows = np.arange(nq, dtype=u32) * 31 % n
        wint = np.stack([wm.scores_internal(meta, rows, int(r)) for r in lrows])
        same(enc.score_internal_all_batch(lrows), wint, f"score_internal_all_batch of {nq}")
        if n < 1 << 20:
            ids, sc = enc.topk_internal_batch(lrows, min(30, n))
            check_topk((ids[nq - 1], sc[nq - 1]), wint[nq - 1], min(30, n), f"topk_internal_batch of {nq}")


@pytest.mark.parametrize("nq", [2, 5, 17])
def test_batches_of_an_empty_store(nq):
    """count = 0: nothing is scored, and topk_batch pads as the single-query top-k does."""
    md = {"actual_dim": 208, "alpha": f32(0.5), "offset": f32(0), "multiplier": f32(0.25),
          "vector_parameters": qa.VectorParameters(200, 0, D.Dot, False), "full_range": True}
    enc = qa.EncodedVectorsU8.from_storage(np.zeros((0, 212), np.uint8), md)
    qs = np.random.default_rng(0).random((nq, 200), dtype=f32)
    b = enc.encode_query_batch(qs)
    assert enc.score_batch(b).size == 0
    ids, sc = enc.topk_batch(b, 3)
    wi, ws = enc.topk(enc.encode_query(qs[0]), 3)
    assert ids.shape == (nq, 3) and all(np.array_equal(ids[j], wi) for j in range(nq))
    same(sc, np.tile(ws, (nq, 1)))


def test_upsert_and_append():
    rng = np.random.default_rng(9)
    x = rng.random((100, 200), dtype=f32)
    x[0, 0], x[0, 1] = 0.0, 1.0
    enc = qa.EncodedVectorsU8.encode(x, qa.VectorParameters(200, 100, D.L2, False), full_range=True)
    new = rng.random((40, 200), dtype=f32) * f32(0.3) + f32(0.7)  # codes above 127
    enc.upsert(90, new[:20])
    enc.append(new[20:])
    rows, meta = wm.encode(np.concatenate([x[:90], new]), 2, False, enc.metadata["alpha"], enc.metadata["offset"])
    assert enc.count == 130 and np.array_equal(enc.storage_bytes(), rows) and (rows[90:, 4:204] > 127).all()
    same(enc.score_batch(enc.encode_query_batch(new[:9])), np.stack([wm.scores(meta, rows, *wm.encode_query(meta, q)) for q in new[:9]]))


# ------------------------------------------------------------------------------------------------------- which kernel ran
def child_main(out_path):
    L, info = qa.lib(), {}
    for dim in (64, 200, 768):
        enc = store(f"{dim}x4099", D.Dot, False)[0]
        qs = np.random.default_rng(1).random((17, dim), dtype=f32)
        for nq in (2, 3, 4, 5, 9, 17):
            for call in ("score_batch", "internal"):
                if call == "score_batch":
                    enc.score_batch(enc.encode_query_batch(qs[:nq]))
                else:
                    enc.score_internal_all_batch(np.arange(nq, dtype=u32))
                info[f"{dim}:{nq}:{call}"] = [int(L.qamd_dev_u8_last_full_batch(C.c_void_p(enc._h.value))),
                                              int(L.qamd_dev_u8_last_scan_queries(C.c_void_p(enc._h.value)))]
    with open(out_path, "w") as f:
        json.dump(info, f)
    print("DONE")


def test_route_of_batches(tmp_path):
    """Up to one pass of u8_scan_multi_kernel (4 queries at dims 200 and 768) the scan serves a batch - its last launch
    held the whole batch, or its second half - and u8_full_batch_kernel ran not; beyond, the new kernel served all queries.
    Rows of dim 64 have no multi-query form: from 3 queries on the new kernel."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
    env.update(QAMD_LIB_PATH=DEV_LIB)
    out = str(tmp_path / "info.json")
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_u8_full_range as T\nT.child_main(%r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), out))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "DONE" in res.stdout, f"exit {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    with open(out) as f:
        info = json.load(f)
    for dim, least in ((64, 3), (200, 5), (768, 5)):
        for nq in (2, 3, 4, 5, 9, 17):
            for call in ("score_batch", "internal"):
                full, scan = info[f"{dim}:{nq}:{call}"]
                assert full == (nq if nq >= least else 0), (dim, nq, call, info)
                assert nq >= least or dim == 64 or scan == nq, (dim, nq, call, info)
