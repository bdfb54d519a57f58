"""Batches of full-range u8 stores through the control flow that only production shapes take, at the
smallest shapes that reach it: four tiles per wave of u8_full_batch_kernel (2^20 rows and more) with a partial wave, a
partial tile and surplus waves; more than two filter passes and a q_pad boundary; the scans' side of the filter gate;
the second trip of the group loop below the gate; device-resident outputs; rotated stores.  Everything against
u8_full_range_model (int64 sums, the f32 epilogue) on raw bits, ranked by the total order on the score bits with ties to
the lower id.

Big stores are built as test_gpu_u8_full_filter's "edge" kind is: the metadata of wm.encode of a zero row (alpha 1 / 255,
offset 0: value v gets code round(255 v)), random bytes for the codes and small random offsets, so no f32 originals of
2^20 rows are held; the model is scored in row slices."""
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
f32, u32, D = np.float32, np.uint32, qa.DistanceType
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(got, want, what=""):
    assert np.array_equal(np.ascontiguousarray(got, f32).view(u32), np.ascontiguousarray(want, f32).view(u32)), what


def ranked(sc, k, largest):
    key = np.ascontiguousarray(sc, f32).view(u32).astype(np.int64)
    key = np.where(key >> 31, 0x7FFFFFFF - (key & 0x7FFFFFFF), key + 0x80000000)
    key = -key if largest else key
    cand = np.flatnonzero(key <= np.partition(key, k - 1)[k - 1]) if k < key.size else np.arange(key.size)  # (lexsort of 2^20 is slow)
    order = cand[np.lexsort((cand, key[cand]))][:k]
    return order.astype(u32), sc[order]


def check_topk(got, j, sc, k, largest, what):
    wi, ws = ranked(sc, k, largest)
    assert np.array_equal(np.asarray(got[0][j]), wi), what
    same(got[1][j], ws, what)


def raw_rows(dim, n, dist, invert, seed, or_mask=0):
    """(rows [n, actual_dim + 4], meta): random byte codes (zero in the padding columns), offsets N(0, 0.05)."""
    meta = wm.encode(np.zeros((1, dim), f32), int(dist), invert, f32(1) / f32(255), 0)[1]
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, meta["actual_dim"] + 4), np.uint8)
    rows[:, 4:4 + dim] = np.frombuffer(rng.bytes(n * dim), np.uint8).reshape(n, dim)
    rows[:, 4:4 + dim] |= np.uint8(or_mask)
    rows[:, :4] = (rng.standard_normal(n).astype(f32) * f32(0.05)).view(np.uint8).reshape(n, 4)
    return rows, meta


def adopt(rows, meta, dim, dist, invert):
    md = {key: meta[key] for key in ("actual_dim", "alpha", "offset", "multiplier")}
    md.update(vector_parameters=qa.VectorParameters(dim, len(rows), dist, invert), full_range=True)
    return qa.EncodedVectorsU8.from_storage(rows, md)


def model(meta, rows, q):
    """The model's scores of query values q against every row, in slices: it widens the codes to int64."""
    qc, qoff = wm.encode_query(meta, q)
    step = max(256, (1 << 23) // rows.shape[1])
    return np.concatenate([wm.scores(meta, rows[i:i + step], qc, qoff) for i in range(0, len(rows), step)])


def sums(meta, rows, q):
    qc = wm.encode_query(meta, q)[0]
    step = max(256, (1 << 23) // rows.shape[1])
    return np.concatenate([wm.pair_sums(meta, rows[i:i + step], qc) for i in range(0, len(rows), step)])


# ------------------------------------------------------------------------------------------------ A: four tiles per wave
N_A = 2 ** 20 + 64 * 5 + 40  # 16390 tiles, 4098 waves of four: the last real wave owns two tiles, the second of 40 rows; two
#                              waves of the last workgroup have nothing
HIGH_A, LOW_A = (0, 64, 256, N_A - 40), (63, 255, N_A - 41, N_A - 1)  # first / last rows of a wave's first, second, last tile
CHECKED_A = (0, 4, 15, 30)  # query 0 and the last query of batches of 5, 16 and 31


@functools.lru_cache(maxsize=1)
def store_a(dim, dist, invert, with_model=True):
    """(store, 31 queries, model scores of CHECKED_A).  Query 0 is all 255s; rows HIGH_A are all 255s and rows LOW_A all
    zeros, so they are the extremes of query 0: a dropped tile or row changes its answer."""
    rows, meta = raw_rows(dim, N_A, dist, invert, dim + N_A)
    rows[list(HIGH_A), 4:4 + dim], rows[list(LOW_A), 4:4 + dim] = 255, 0
    qs = np.random.default_rng(dim).random((31, dim), dtype=f32)
    qs[0] = 1.0
    want = {j: model(meta, rows, qs[j]) for j in CHECKED_A} if with_model else {}
    return adopt(rows, meta, dim, dist, invert), qs, want


@pytest.mark.parametrize("dim,dist,invert", [(16, D.Dot, False), (16, D.Dot, True), (16, D.L2, False), (16, D.L2, True),
                                             (272, D.Dot, False)])  # NKB 4; NKB 12 with a padded last k-block
def test_four_tiles_per_wave(dim, dist, invert):
    assert (N_A + 63) // 64 == 16390 and (16390 + 3) // 4 == 4098 and N_A >= 1 << 20
    enc, qs, want = store_a(dim, dist, invert)
    top, bottom = (set(ranked(want[0], 30, lg)[0].tolist()) for lg in (True, False))
    planted = (set(HIGH_A), set(LOW_A))
    assert (top & set(HIGH_A + LOW_A), bottom & set(HIGH_A + LOW_A)) in (planted, planted[::-1])
    for nq in (5, 16):
        got = enc.score_batch(enc.encode_query_batch(qs[:nq]))
        for j in (0, nq - 1):
            same(got[j], want[j], f"score_batch of {nq}, query {j}")
    del got
    for nq in (5, 16, 31):
        b = enc.encode_query_batch(qs[:nq])
        for k, largest in [(k, lg) for k in (30, 1024) for lg in (True, False)]:  # pivot ranks 16 and 48: the fused pass
            got = enc.topk_batch(b, k, largest=largest)
            for j in (0, nq - 1):
                check_topk(got, j, want[j], k, largest, f"topk_batch({k}, {largest}) of {nq}, query {j}")


# ------------------------------------------------------------------------------------------------ B: many passes
N_B = 33000
CHECKED_B = (0, 14, 15, 29, 30, 44, 45, 254, 255, 256)
PLANT_B = [(j * 127 + 5) % N_B for j in range(257)]  # spread over the store, all different (127 * 256 < 33000)


def mask_b(j):
    """Nine of 64 dims, one of each of the pairs (2 b, 2 b + 1) by bit b of j: two query indices share at most eight."""
    m = np.zeros(64, bool)
    m[[2 * b + (j >> b & 1) for b in range(9)]] = True
    return m


@functools.lru_cache(maxsize=2)
def store_b(dist, invert):
    """(store, 257 queries, model scores of CHECKED_B).  Query j is 255 on mask_b(j) and 0 elsewhere, row PLANT_B[j] too: the
    one row whose sum with query j is 9 * 255^2, so every query has another best row."""
    rows, meta = raw_rows(64, N_B, dist, invert, 64 + N_B)
    qs = np.stack([mask_b(j) for j in range(257)]).astype(f32)
    rows[PLANT_B, 4:] = (qs * 255).astype(np.uint8)
    return adopt(rows, meta, 64, dist, invert), qs, {j: model(meta, rows, qs[j]) for j in CHECKED_B}


@pytest.mark.parametrize("dist,invert", [(D.Dot, False), (D.L2, True)])
@pytest.mark.parametrize("nq,checked", [(46, (0, 14, 15, 29, 30, 44, 45)), (257, (0, 254, 255, 256))])  # passes of 15, 15, 15, 1; 18 passes, q_pad 512
def test_many_passes(nq, checked, dist, invert):
    assert len(set(PLANT_B)) == 257
    enc, qs, want = store_b(dist, invert)
    for j in checked:  # the answer of another query's slot cannot pass
        assert ranked(want[j], 1, True)[0][0] == PLANT_B[j], j
    b = enc.encode_query_batch(qs[:nq])
    for largest in (True, False):
        got = enc.topk_batch(b, 30, largest=largest)
        for j in checked:
            check_topk(got, j, want[j], 30, largest, f"topk_batch(30, {largest}) of {nq}, query {j}")


# ------------------------------------------------------------------------------------------------ C: the scans' side of the gate
# name: (dim, rows, metric, invert, code bits set in every row, multiplier in place of the store's, batch sizes, checked)
GATE = {"768": (768, 33000, D.Dot, False, 0, None, (2, 3, 4), None),
        "768-l2inv": (768, 33000, D.L2, True, 0, None, (2, 3, 4), None),
        "200": (200, 33000, D.Dot, False, 0, None, (2, 3, 4), None),
        "200-l2inv": (200, 33000, D.L2, True, 0, None, (2, 3, 4), None),
        "64": (64, 33000, D.Dot, False, 0, None, (2,), None),  # no multi form: a single scan per query
        "l1": (200, 33000, D.L1, False, 0, None, (5, 16), None),
        "l1-inv": (200, 33000, D.L1, True, 0, None, (5, 16), None),
        "multiplier-0": (200, 33000, D.Dot, False, 0, 0.0, (5,), None),
        "multiplier-inf": (200, 33000, D.Dot, False, 0x10, np.inf, (5,), None),  # every sum positive: no 0 * inf
        "8272": (8272, 32768, D.Dot, False, 0, None, (5,), (0, 4))}  # sums past 2^29: beyond the integer pre-filter
ROW_8272 = 12345


@functools.lru_cache(maxsize=2)
def store_c(name, with_model=True):
    """(store, queries, model scores of the checked queries, meta, rows)."""
    dim, n, dist, invert, or_mask, mult, sizes, checked = GATE[name]
    rows, meta = raw_rows(dim, n, dist, invert, dim + n, or_mask)
    qs = np.random.default_rng(dim).random((max(sizes), dim), dtype=f32) * f32(0.9) + f32(0.1)  # (no zero code)
    if mult is not None:
        meta["multiplier"] = f32(mult)
    if name == "8272":
        rows[ROW_8272, 4:], qs[0] = 255, 1.0
    want = {j: model(meta, rows, qs[j]) for j in (checked or range(max(sizes)))} if with_model else {}
    return adopt(rows, meta, dim, dist, invert), qs, want, meta, rows


@pytest.mark.parametrize("name", list(GATE))
def test_scans_side_of_the_gate(name):
    enc, qs, want, meta, rows = store_c(name)
    if name == "multiplier-inf":
        assert all(sums(meta, rows, qs[j]).min() > 0 for j in want) and all(np.all(np.isposinf(w)) for w in want.values())
    if name == "8272":
        assert int(sums(meta, rows, qs[0])[ROW_8272]) == 537886800 > 1 << 29
    for nq in GATE[name][6]:
        b = enc.encode_query_batch(qs[:nq])
        for largest in (True, False):
            got = enc.topk_batch(b, 30, largest=largest)
            for j in (j for j in want if j < nq):
                check_topk(got, j, want[j], 30, largest, f"topk_batch(30, {largest}) of {nq}, query {j}")


# ------------------------------------------------------------------------------------------------ D: the group loop
def test_group_loop_second_trip():
    n, nq = 32767, 2050
    assert (256 << 20) // (4 * n) == 2048 < nq and n < 32768  # below the gate; queries 2048 and 2049 are the second trip
    rows, meta = raw_rows(16, n, D.Dot, False, 16 + n)
    qs = np.random.default_rng(2050).random((nq, 16), dtype=f32)
    enc = adopt(rows, meta, 16, D.Dot, False)
    got = enc.topk_batch(enc.encode_query_batch(qs), 30)
    for j in (0, 2047, 2048, 2049):
        check_topk(got, j, model(meta, rows, qs[j]), 30, True, f"query {j}")


# ------------------------------------------------------------------------------------------------ E: device outputs
@functools.lru_cache(maxsize=1)
def store_ties():
    """Every row from 40 on equals row 40: the tie sits at the pivot, every list overflows, every query is redone."""
    rows, meta = raw_rows(768, 33000, D.Dot, False, 7)
    rows[40:] = rows[40]
    return adopt(rows, meta, 768, D.Dot, False), np.random.default_rng(8).random((16, 768), dtype=f32), meta, rows


@pytest.mark.parametrize("kind", ["768", "ties"])
def test_device_outputs(kind):
    import torch
    if kind == "ties":
        enc, qs, meta, rows = store_ties()
        want0 = model(meta, rows, qs[0])
    else:
        enc, qs, want, _, _ = store_c("768")
        qs, want0 = np.concatenate([qs, qs[::-1] * f32(0.5), qs * f32(0.25), qs[::-1]]), want[0]  # 16 queries
    for nq in (5, 16):
        b = enc.encode_query_batch(qs[:nq])
        for largest in (True, False):
            ids, sc = enc.topk_batch(b, 30, largest=largest)
            check_topk((ids, sc), 0, want0, 30, largest, f"host outputs, {nq} queries")
            d_ids = torch.full((nq * 30,), -1, dtype=torch.int32, device="cuda")
            d_sc = torch.full((nq * 30,), float("nan"), dtype=torch.float32, device="cuda")
            enc.topk_batch(b, 30, largest=largest, out_ids=d_ids, out_scores=d_sc)
            torch.cuda.synchronize()
            assert np.array_equal(d_ids.cpu().numpy().view(u32).reshape(nq, 30), ids), (nq, largest)
            same(d_sc.cpu().numpy().reshape(nq, 30), sc, (nq, largest))


# ------------------------------------------------------------------------------------------------ G: rotated stores
@pytest.mark.parametrize("dim,n", [(192, 4099), (64, 33000)])
def test_rotated_batches(dim, n):
    rng = np.random.default_rng(dim + n)
    x, qs = rng.standard_normal((n, dim)).astype(f32), rng.standard_normal((9, dim)).astype(f32)
    y = um.rotate(x)
    rows, meta = wm.encode(y, wm.DOT, False, *wm.interval(y))
    enc = qa.EncodedVectorsU8.encode(x, qa.VectorParameters(dim, n, D.Dot, False), rotated=True, full_range=True)
    assert np.array_equal(enc.storage_bytes(), rows)
    want = [model(meta, rows, q) for q in um.rotate(qs)]
    b = enc.encode_query_batch(qs)
    same(enc.score_batch(b), np.stack(want), "score_batch")
    for largest in (True, False):
        got = enc.topk_batch(b, 30, largest=largest)
        for j in range(9):
            check_topk(got, j, want[j], 30, largest, f"topk_batch(30, {largest}), query {j}")


# ------------------------------------------------------------------------------------------------ which kernel ran
def child_main():
    """On the developer library: [queries through the filter form, of those redone] of the last topk_batch(30)."""
    L, info = qa.lib(), {}
    seen = lambda enc: [int(fn(C.c_void_p(enc._h.value))) for fn in (L.qamd_dev_u8_last_full_filter, L.qamd_dev_u8_last_full_redone)]
    enc, qs, _ = store_a(16, D.Dot, False, with_model=False)
    for nq in (5, 16, 31):
        enc.topk_batch(enc.encode_query_batch(qs[:nq]), 30)
        info[f"four-tiles:{nq}"] = seen(enc)
    del enc
    for name, nq in (("768", 4), ("64", 2), ("l1", 16), ("multiplier-0", 5), ("multiplier-inf", 5), ("8272", 5)):
        enc, qs = store_c(name, with_model=False)[:2]
        enc.topk_batch(enc.encode_query_batch(qs[:nq]), 30)
        info[f"{name}:{nq}"] = seen(enc)
    print("INFO " + json.dumps(info))


def test_which_kernel_ran():
    """The 2^20-row store sends every query through the filter form and redoes none; everything on the scans' side of the
    gate sends none."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
    env.update(QAMD_LIB_PATH=os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so"))
    code = "import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_u8_full_large_forms as T\nT.child_main()\n" % (ROOT, os.path.join(ROOT, "tests"))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "INFO " in res.stdout, f"exit {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    assert json.loads(res.stdout.split("INFO ")[1]) == {"four-tiles:5": [5, 0], "four-tiles:16": [16, 0], "four-tiles:31": [31, 0],
                                                        "768:4": [0, 0], "64:2": [0, 0], "l1:16": [0, 0], "multiplier-0:5": [0, 0],
                                                        "multiplier-inf:5": [0, 0], "8272:5": [0, 0]}
