"""Compact 4-bit scalar-u8 stores on the GPU: every comparison on raw bit patterns, against
u8_four_bit_model (through the oracle's scores on the model's rows) and against the 4-bit store built from the same
arguments without the flag.

Shapes: actual_dim 32 (one image chunk), 48 (dim 40: odd row_chunks - the zero high nibbles of the last chunk - and
query padding), 768 and 1536 (rotated, several 16-chunk steps of the pair kernel), 2048 (the widest); rows 1, 63, 64, 65,
1024, 1025, 4099 (block and padding edges); Dot and L2, each plain and inverted.  One child process on the developer
library reads the device bytes both stores own and repeats the builders with 64 KiB tiles, so that every one of them
goes through many tiles at these sizes."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import u8_compact_model as cm
import u8_four_bit_model as fm
from oracle import qoracle as qo
from util import assert_bits_equal, topk_want

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
from quantization_amd import _lib  # noqa: E402

E = qa.EncodedVectorsU8
D = qa.DistanceType
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")

# (dim, rotated, rows, metric, invert)
CASES = [(32, False, 1, D.Dot, False), (32, False, 65, D.L2, True), (40, False, 63, D.Dot, True), (40, False, 1025, D.Dot, False),
         (40, False, 1025, D.L2, False), (40, False, 1025, D.L2, True), (768, True, 4099, D.Dot, False),
         (768, True, 4099, D.Dot, True), (768, True, 4099, D.L2, False), (768, True, 4099, D.L2, True),
         (1536, True, 1024, D.L2, False), (2048, False, 64, D.Dot, True), (2048, True, 1025, D.L2, True)]
IDS = [f"{d}{'r' if r else ''}x{n}-{m.name}{'-inv' if i else ''}" for d, r, n, m, i in CASES]


def _data(n, dim, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, dim)).astype(f32)
    x[:, (7 * dim) // 13] *= f32(4.0)
    return x


@functools.lru_cache(maxsize=None)
def _case(dim, rotated, n, dist, invert):
    """Data, the model's store, the plain and the compact handle of a shape: built once, shared, never written to."""
    x = _data(n, dim, dim * 7 + n)
    rows, meta = fm.encode(x, int(dist), invert, rotated)
    rng = np.random.default_rng(dim + n)
    qs = rng.normal(size=(9, dim)).astype(f32)
    for a in (x, rows, qs):
        a.setflags(write=False)
    vp = qa.VectorParameters(dim, n, dist, invert)
    plain = E.encode(x, vp, rotated=rotated, bits=4)
    comp = E.encode(x, vp, rotated=rotated, bits=4, compact=True)
    return {"x": x, "vp": vp, "rows": rows, "meta": meta, "qs": qs, "rotated": rotated, "plain": plain, "comp": comp, "n": n,
            "ad": meta.actual_dim}


def _same_store(comp, other, what):
    """Same metadata but for the flag, same exported rows."""
    a, b = comp.metadata, other.metadata
    assert a.pop("compact") is True and comp.compact and "compact" not in b and not other.compact, what
    assert a.keys() == b.keys() and a["vector_parameters"] == b["vector_parameters"] and a["bits"] == b["bits"] == 4, what
    assert_bits_equal(np.array([a["alpha"], a["offset"], a["multiplier"]], f32),
                      np.array([b["alpha"], b["offset"], b["multiplier"]], f32), what)
    assert np.array_equal(comp.storage_bytes(), other.storage_bytes()), f"{what}: exported rows"


def _topk_same(got, want, what):
    assert np.array_equal(np.asarray(got[0]), np.asarray(want[0])), f"{what}: ids"
    assert_bits_equal(got[1], want[1], f"{what}: scores")


def _ids_of(n, rng, m):
    ids = rng.integers(0, n, size=m).astype(np.uint32)
    ids[-1] = n - 1  # the last row
    if m > 2:
        ids[1] = ids[0]  # a duplicate
    return ids


def _check_scoring(comp, plain, c, what):
    """Every scoring call of the compact handle against the plain one; score_all also against the model."""
    n, qs, rng = c["n"], c["qs"], np.random.default_rng(c["n"])
    qc, qp = comp.encode_query(qs[0]), plain.encode_query(qs[0])
    codes, off = fm.encode_query(c["meta"], qs[0], c["rotated"])
    assert np.array_equal(qc.encoded_query, codes), what
    want_all = plain.score_all(qp)
    assert_bits_equal(comp.score_all(qc), want_all, f"{what}: score_all")
    if "rows_now" not in c:  # (after an upsert the model's rows are no longer the store's)
        assert_bits_equal(want_all, qo.u8_score_all(c["meta"], c["rows"], codes, off), f"{what}: score_all against the model")
    for k in (1, 30, 1024):
        if k > 30 and n < 4099:
            continue
        for largest in (True, False):
            got = comp.topk(qc, k, largest)
            _topk_same(got, plain.topk(qp, k, largest), f"{what}: topk {k} {largest}")
            _topk_same(got, topk_want(want_all, k, largest), f"{what}: topk {k} {largest} against the scores")
    for i in sorted({0, n - 1, min(n - 1, 37)}):  # the first, the last, a row inside a block
        assert_bits_equal([comp.score_point(qc, i)], [want_all[i]], f"{what}: score_point {i}")
    ids = _ids_of(n, rng, 70)
    assert_bits_equal(comp.score_ids(qc, ids), want_all[ids], f"{what}: score_ids")
    # bursts: three queries, lists of 0, 1 and many ids; stored rows against lists
    lists = np.array([0, 0, 1, 41], np.uint32)
    bids = _ids_of(n, rng, 41)
    bc, bp = comp.encode_query_batch(qs[:3]), plain.encode_query_batch(qs[:3])
    assert_bits_equal(comp.score_ids_batch(bc, lists, bids), plain.score_ids_batch(bp, lists, bids), f"{what}: score_ids_batch")
    srows = np.array([0, n - 1, min(n - 1, 37)], np.uint32)
    assert_bits_equal(comp.score_internal_ids_batch(srows, lists, bids), plain.score_internal_ids_batch(srows, lists, bids),
                      f"{what}: score_internal_ids_batch")
    # score_internal and its whole-store forms
    i, j = min(n - 1, 37), n - 1
    assert_bits_equal([comp.score_internal(i, j)], [plain.score_internal(i, j)], f"{what}: score_internal")
    assert_bits_equal(comp.score_internal_ids(i, ids), plain.score_internal_ids(i, ids), f"{what}: score_internal_ids")
    want_int = plain.score_internal_all(i)
    assert_bits_equal(comp.score_internal_all(i), want_int, f"{what}: score_internal_all")
    assert_bits_equal(comp.score_internal_ids(i, ids), want_int[ids], f"{what}: score_internal_ids against the scan")
    assert_bits_equal(comp.score_internal_ids(j, None, n_rows=min(n, 70)), plain.score_internal_ids(j, None, n_rows=min(n, 70)),
                      f"{what}: score_internal_ids of a prefix")
    k = min(n, 30)
    _topk_same(comp.topk_internal(i, k), plain.topk_internal(i, k), f"{what}: topk_internal")
    assert_bits_equal(comp.score_internal_all_batch(srows), plain.score_internal_all_batch(srows),  # the null id list
                      f"{what}: score_internal_ids_batch, null ids")
    # batches of 1, 3 and 9 queries: one image scan per query against the plain store's multi-query and matrix-core routes
    for nq in (1, 3, 9):
        bc, bp = comp.encode_query_batch(qs[:nq]), plain.encode_query_batch(qs[:nq])
        got = comp.score_batch(bc)
        assert_bits_equal(got, plain.score_batch(bp), f"{what}: score_batch {nq}")
        assert_bits_equal(got[0], want_all, f"{what}: score_batch {nq} against score_all")
        kk = min(n, 30)
        _topk_same(comp.topk_batch(bc, kk), plain.topk_batch(bp, kk), f"{what}: topk_batch {nq}")


@pytest.mark.parametrize("dim,rotated,n,dist,invert", CASES, ids=IDS)
def test_every_scoring_call(dim, rotated, n, dist, invert):
    c = _case(dim, rotated, n, dist, invert)
    comp, plain = c["comp"], c["plain"]
    assert comp.bits == 4 and comp.rotated == rotated and comp.vector_parameters == c["vp"] and comp.count == n
    _same_store(comp, plain, "one-shot")
    assert np.array_equal(comp.storage_bytes(), c["rows"])  # the model's rows
    per_row = 16 * cm.chunks_of(c["ad"]) + 4
    assert comp.scan_bytes_per_row() == plain.scan_bytes_per_row() == per_row  # unchanged: the image is what is scanned
    _check_scoring(comp, plain, c, "one-shot")


def test_lane_mode_1_changes_nothing():
    c = _case(768, True, 4099, D.Dot, False)
    comp = E.from_storage(c["rows"], c["comp"].metadata)
    assert comp.compact
    comp.set_lane_mode(1)
    _check_scoring(comp, c["plain"], c, "lane mode 1")


def test_rescored_against_plain_originals():
    c = _case(768, True, 4099, D.L2, False)
    comp, plain, q = c["comp"], c["plain"], c["qs"][1]
    orig = qa.OriginalVectors.from_data(c["x"], c["vp"])
    got = comp.topk_rescored(comp.encode_query(q), orig, q, 5, 50)
    _topk_same(got, plain.topk_rescored(plain.encode_query(q), orig, q, 5, 50), "topk_rescored")
    cids, _ = comp.topk(comp.encode_query(q), 50)
    _topk_same(got, orig.rerank(q, cids, 5), "topk_rescored against rerank")


BUILD_CASES = [(40, False, 1025, D.L2, True), (768, True, 4099, D.Dot, False), (2048, False, 64, D.Dot, True)]


@pytest.mark.parametrize("dim,rotated,n,dist,invert", BUILD_CASES, ids=[IDS[CASES.index(b)] for b in BUILD_CASES])
def test_every_builder(dim, rotated, n, dist, invert, tmp_path):
    import torch

    c = _case(dim, rotated, n, dist, invert)
    x, vp, plain = c["x"], c["vp"], c["plain"]
    kw = {"rotated": rotated, "bits": 4, "compact": True}
    # one-shot from device data; the quantile interval; a given interval
    _same_store(E.encode(torch.from_numpy(x.copy()).cuda(), vp, **kw), plain, "device data")
    _same_store(E.encode(x, vp, 0.99, **kw), E.encode(x, vp, 0.99, rotated=rotated, bits=4), "quantile")
    # the streaming encoder with batches that split blocks
    for step in (1, 63, 130):
        if step == 1 and n > 100:
            continue
        batches = lambda: iter([x[r:r + step] for r in range(0, n, step)])
        h = E.encode_stream(batches, vp, **kw)
        _same_store(h, plain, f"stream {step}")
    _check_scoring(h, plain, c, "stream")
    # from_rows of exported bytes: the flag from the metadata and from the argument; a code of 16 is refused
    rows = plain.storage_bytes()
    md = c["comp"].metadata
    assert md["compact"] is True
    for h in (E.from_storage(rows, md), E.from_storage(rows, plain.metadata, compact=True),
              E.from_storage(torch.from_numpy(rows.copy()).cuda(), md)):
        _same_store(h, plain, "from_rows")
    _check_scoring(h, plain, c, "from_rows")
    bad = rows.copy()
    bad[n - 1, 4 + c["ad"] - 1] = 16
    with pytest.raises(qa.EncodingError) as e:
        E.from_storage(bad, md)
    assert e.value.status == _lib.ERR_ARGUMENTS
    assert E.from_storage(bad, plain.metadata).scan_bytes_per_row() == c["ad"] + 4  # the plain store goes without an image
    # save / load: the data file is the plain store's byte for byte, the metadata ends in "bits":4,"compact":true
    paths = [str(tmp_path / f) for f in ("c.bin", "c.json", "p.bin", "p.json")]
    c["comp"].save(paths[0], paths[1])
    plain.save(paths[2], paths[3])
    assert open(paths[0], "rb").read() == open(paths[2], "rb").read()
    text, ptext = open(paths[1]).read(), open(paths[3]).read()
    assert text == ptext[:-1] + ',"compact":true}' and ptext.endswith(',"bits":4}')
    assert json.loads(text)["vector_parameters"]["distance_type"] == dist.name  # the base metric
    h = E.load(paths[0], paths[1], vp)
    _same_store(h, plain, "load")
    _check_scoring(h, plain, c, "load")
    assert not E.load(paths[2], paths[3], vp).compact


@pytest.mark.parametrize("dim,rotated,n,dist,invert", [(40, False, 1025, D.Dot, False), (768, True, 4099, D.L2, True)],
                         ids=["40x1025", "768rx4099"])
def test_upsert_append_reserve(dim, rotated, n, dist, invert):
    c = dict(_case(dim, rotated, n, dist, invert))
    c["rows_now"] = True
    comp, plain = (E.encode(c["x"], c["vp"], rotated=rotated, bits=4, compact=compact) for compact in (True, False))
    more = _data(3000, dim, 99)

    def both(fn):
        for h in (comp, plain):
            fn(h)
        _same_store(comp, plain, "after a write")
        assert comp.count == plain.count and comp.capacity == plain.capacity

    both(lambda h: h.upsert(37, more[:1]))            # one row inside a block
    both(lambda h: h.upsert(60, more[1:11]))          # across a block edge
    both(lambda h: h.upsert(n - 2, more[11:16]))      # over the end: appends inside the padding
    c["n"] = comp.count
    _check_scoring(comp, plain, c, "upsert")
    both(lambda h: h.append(more[16:16 + 2100]))      # past the capacity: both stores grow
    both(lambda h: h.reserve(h.count + 5000))
    both(lambda h: h.append(more[2200:2265]))
    c["n"] = comp.count
    assert comp.capacity >= comp.count and comp.compact
    _check_scoring(comp, plain, c, "append and reserve")


def test_refusals_on_the_gpu_machine(tmp_path):
    got = cm.refusals(_lib, tmp_path)
    assert len(got) == cm.N_REFUSALS
    for what, st, want, out in got:
        assert st == want and out is None, (what, st, want)


# ------------------------------------------------------------------ the developer library: bytes owned, and small tiles
CHILD_CASES = [(40, False, 1025, D.L2, True), (768, True, 4099, D.Dot, False)]


def child_main(out_path):
    L = qa.lib()
    L.qamd_dev_u8_store_bytes.restype = C.c_uint64
    L.qamd_dev_u8_store_bytes.argtypes = [C.c_void_p]
    info = {}
    for case in CHILD_CASES:
        dim, rotated, n = case[:3]
        c = _case(*case)  # built here with 64 KiB tiles: 1025 rows of 48 codes are one tile, 4099 of 768 are 65
        tag = f"{dim}x{n}"
        padded = -(-n // 1024) * 1024 + 1024
        info[tag + "/bytes"] = [int(L.qamd_dev_u8_store_bytes(c["comp"]._h)), int(L.qamd_dev_u8_store_bytes(c["plain"]._h)),
                                padded, c["ad"]]
        _same_store(c["comp"], c["plain"], "small tiles, one-shot")
        assert np.array_equal(c["comp"].storage_bytes(), c["rows"])
        _check_scoring(c["comp"], c["plain"], c, "small tiles")
        x, vp = c["x"], c["vp"]
        kw = {"rotated": rotated, "bits": 4, "compact": True}
        h = E.encode_stream(lambda: iter([x[r:r + 130] for r in range(0, n, 130)]), vp, **kw)
        _same_store(h, c["plain"], "small tiles, stream")
        h = E.from_storage(c["rows"], c["comp"].metadata)
        _same_store(h, c["plain"], "small tiles, from_rows")
        assert np.array_equal(h.storage_rows(60, min(n - 60, 900)), c["rows"][60:60 + min(n - 60, 900)])
        more = _data(700, dim, 5)
        p = E.from_storage(c["rows"], c["plain"].metadata)
        for s in (h, p):
            s.upsert(60, more)
            s.append(more[:300])
        _same_store(h, p, "small tiles, upsert and append")
        info[tag + "/bytes_after"] = [int(L.qamd_dev_u8_store_bytes(h._h)), -(-h.capacity // 1024) * 1024 + 1024]
    with open(out_path, "w") as f:
        json.dump(info, f)
    print("DONE")


def test_memory_and_small_tiles(tmp_path):
    assert os.path.exists(DEV_LIB), "the developer library is built with the product one (make -C quantization_amd/csrc)"
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
    env.update(QAMD_LIB_PATH=DEV_LIB, QAMD_DEV_STAGE_BYTES=str(64 * 1024))
    out = str(tmp_path / "info.json")
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_u8_compact as T\nT.child_main(%r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), out))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "DONE" in res.stdout, f"exit {res.returncode}\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}"
    with open(out) as f:
        info = json.load(f)
    for dim, _, n, _, _ in CHILD_CASES:
        comp, plain, padded, ad = info[f"{dim}x{n}/bytes"]
        print(f"{dim}x{n}: compact {comp} bytes, plain {plain} bytes, {padded} padded rows")
        assert comp <= cm.store_bytes(padded, ad) == padded * (16 * -(-ad // 32) + 4)
        assert plain == comp + padded * ad  # the byte codes are what the flag saves
        after, padded_after = info[f"{dim}x{n}/bytes_after"]
        assert after <= cm.store_bytes(padded_after, ad)  # the staging buffer went back after the writes
