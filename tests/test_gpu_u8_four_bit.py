"""4-bit scalar-u8 stores on the GPU, every comparison on raw bits.

1. Encode and query parity with the model (u8_four_bit_model.py), plain and rotated, through every conversion path of
   the encoder: the 16-lanes-per-row kernel (aligned rows of dim % 4 == 0), the dword kernel (any other source), both
   forms of the rotating kernel, and the query encoders; a sweep over the values at which code() changes.
2. The nibble scan (csrc/u8.hip u8_scan_image_kernel<Image4>) against the byte codes and the oracle, by the method of
   test_gpu_u8_blocked.py: child processes on the developer library - as built, with QAMD_DEV_U8_PACKED=0 and with
   QAMD_DEV_CU_COUNT=1 - over stores adopted from uniform random codes 0..15, so the test owns every byte.
3. One case for each route that reads the byte codes, and the write paths.

The ring of the nibble kernel holds R = 8 image chunks, 16 code chunks: rc = 16, 17, 18 and 32 are one full group, one
group and the odd last chunk, one group and a rest chunk, and two groups; 2 and 3 are one chunk and one and a half;
127 and 128 the upper limit; 1 and 129 have no image."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import u8_four_bit_model as fm
import u8_rotated_model as um
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

# ================================================================================================ 1. encode parity
# dim: (rotated, metric, invert)
PLAIN = {20: (D.Dot, False), 32: (D.L2, True), 130: (D.L2, False), 768: (D.Dot, True)}
ROTATED = {64: (D.Dot, False), 128: (D.L2, True), 192: (D.Dot, False), 768: (D.L2, False), 1536: (D.Dot, True),
           2112: (D.L2, True), 4096: (D.L2, False)}
ROWS = (1, 65, 1025)
CASES = [(False, dim, n) for dim in PLAIN for n in ROWS] + [(True, dim, n) for dim in ROTATED for n in ROWS]
# Every K = ceil(dim / 256) of the rotation's wave-per-row frame, its chunk stages taken (256, 512, 1024, 2048) and not
# taken (832, 1984: B = 64, idle lanes), and the ends of the workgroup-per-row frame (12288 = 3 x 4096, 16384), at 65
# rows: one pass of several workgroups.
ROTATED_MORE = {256: (D.Dot, False), 320: (D.L2, False), 512: (D.Dot, True), 832: (D.L2, True), 1024: (D.L2, False),
                1280: (D.Dot, False), 1792: (D.L2, True), 1984: (D.Dot, True), 2048: (D.L2, False), 12288: (D.Dot, False),
                16384: (D.L2, False)}
ROTATED.update(ROTATED_MORE)
CASES += [(True, dim, 65) for dim in ROTATED_MORE]


def _data(n, dim, seed):
    """Gaussian rows with one column 100 x the rest, and -0.0 entries."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, dim)).astype(f32)
    x[:, (7 * dim) // 13] *= f32(100.0)
    x[n // 2, ::5] = f32(-0.0)
    return x


def _specials(x, nan_only):
    """x with a NaN planted and (unless nan_only) +inf and -inf, in different rows where there are three."""
    n, dim = x.shape
    x = x.copy()
    x[0, dim // 3] = np.nan
    if not nan_only:
        x[(n // 3) % n, dim // 2] = np.inf
        x[(2 * n // 3) % n, dim - 1] = -np.inf
    return x


@functools.lru_cache(maxsize=None)
def _case(rotated, dim, n):
    """The data and the model's store of a shape, computed once and shared (nothing here is written to)."""
    dist, invert = (ROTATED if rotated else PLAIN)[dim]
    x = _data(n, dim, dim * 10 + n + rotated)
    rows, meta = fm.encode(x, int(dist), invert, rotated)
    rng = np.random.default_rng(dim + n)
    q = rng.normal(size=dim).astype(f32)
    qs = rng.normal(size=(5, dim)).astype(f32)
    for a in (x, rows, q, qs):
        a.setflags(write=False)
    return {"x": x, "dist": dist, "invert": invert, "vp": qa.VectorParameters(dim, n, dist, invert), "rows": rows,
            "meta": meta, "q": q, "qs": qs, "rotated": rotated}


def _check_store(h, rows, meta, rotated, what, nan_offsets=False):
    md = h.metadata
    assert h.bits == 4 and md["bits"] == 4 and h.rotated == rotated, what
    assert_bits_equal(np.array([md["alpha"], md["offset"], md["multiplier"]], f32),
                      np.array([meta.alpha, meta.offset, meta.multiplier], f32), f"{what}: alpha, offset, multiplier")
    got = h.storage_bytes()
    assert got[:, 4:].max(initial=0) <= 15, what
    if nan_offsets:  # an infinite interval: every row offset is a NaN, whose sign and payload are the machine's
        assert np.array_equal(got[:, 4:], rows[:, 4:]), f"{what}: codes differ from the model"
        g, w = np.ascontiguousarray(got[:, :4]).view(f32), np.ascontiguousarray(rows[:, :4]).view(f32)
        assert np.array_equal(g, w, equal_nan=True), f"{what}: row offsets"
    else:
        bad = np.flatnonzero((got != rows).any(axis=1))
        assert bad.size == 0, f"{what}: {bad.size} rows differ from the model, first {bad[:1]}"


def _check_query(h, meta, q, rotated, what, src=None):
    """`src`: the same query where the store is to take it from (a device tensor)."""
    eq = h.encode_query(q if src is None else src)
    codes, off = fm.encode_query(meta, q, rotated)
    assert np.array_equal(eq.encoded_query, codes), f"{what}: query codes"
    assert_bits_equal(np.array([eq.offset], f32), np.array([off], f32), f"{what}: query offset")
    return eq


@pytest.mark.parametrize("rotated,dim,n", CASES)
def test_encode_parity(rotated, dim, n):
    import torch

    c = _case(rotated, dim, n)
    x, vp, dist, invert = c["x"], c["vp"], int(c["dist"]), c["invert"]
    kw = {"rotated": rotated, "bits": 4}
    # min/max: a device tensor (encoded in place), host rows (staged), a device tensor that is not 16-byte aligned
    off1 = torch.zeros(n * dim + 1, dtype=torch.float32, device="cuda")
    off1[1:] = torch.from_numpy(x.copy()).cuda().reshape(-1)
    for name, src in (("device", torch.from_numpy(x.copy()).cuda()), ("host", x), ("misaligned", off1[1:].view(n, dim))):
        h = E.encode(src, vp, **kw)
        _check_store(h, c["rows"], c["meta"], rotated, f"min/max, {name}")
        assert h.vector_parameters == vp  # the base metric: distance_type stays a DistanceType
    # one query from the host and from the device, and many at once (their scores: the batch keeps its codes on the device)
    _check_query(h, c["meta"], c["q"], rotated, "host query")
    _check_query(h, c["meta"], c["q"], rotated, "device query", src=torch.from_numpy(c["q"].copy()).cuda())
    got = h.score_batch(h.encode_query_batch(c["qs"]))
    for i in (0, len(c["qs"]) - 1):
        codes, off = fm.encode_query(c["meta"], c["qs"][i], rotated)
        assert_bits_equal(got[i], qo.u8_score_all(c["meta"], c["rows"], codes, off), f"batch query {i}")
    # quantile (a no-op below 127 rows, as in the reference)
    rows, meta = fm.encode(x, dist, invert, rotated, quantile=0.99)
    h = E.encode(x, vp, 0.99, **kw)
    _check_store(h, rows, meta, rotated, "quantile")
    _check_query(h, meta, c["q"], rotated, "quantile")
    # a given interval, from a source that is not 16-byte aligned, rows holding NaN and +-inf
    xs = _specials(x, nan_only=False)
    ao = (float(c["meta"].alpha), float(c["meta"].offset))
    rows, meta = fm.encode(xs, dist, invert, rotated, alpha_offset=ao)
    flat = torch.zeros(n * dim + 1, dtype=torch.float32, device="cuda")
    flat[1:] = torch.from_numpy(xs).cuda().reshape(-1)
    _check_store(E.encode(flat[1:].view(n, dim), vp, alpha_offset=ao, **kw), rows, meta, rotated, "alpha_offset, misaligned, specials")
    _check_store(E.encode(torch.from_numpy(xs).cuda(), vp, alpha_offset=ao, **kw), rows, meta, rotated, "alpha_offset, device, specials")
    # min/max skips NaN as the reference's `value < min` does, and takes infinities for what they are
    xn = _specials(x, nan_only=True)
    rows, meta = fm.encode(xn, dist, invert, rotated)
    _check_store(E.encode(xn, vp, **kw), rows, meta, rotated, "min/max with NaN")
    rows, meta = fm.encode(xs, dist, invert, rotated)
    _check_store(E.encode(xs, vp, **kw), rows, meta, rotated, "min/max with +-inf", nan_offsets=True)


@pytest.mark.parametrize("alpha,offset", [(0.1, -0.75), (1.0 / 15.0, 0.0), (3.7e-3, 1.3), (0.25, -2.0), (1e-20, 0.0), (3e9, -1e10)])
def test_boundary_sweep(alpha, offset):
    """Values on, and up to two ulp either side of, every point where (v - offset) / alpha is a half-integer from -0.5 to
    15.5 - where code() steps - through the 16-lanes-per-row kernel, the dword kernel and both query encoders."""
    import torch

    a, o = f32(alpha), f32(offset)
    vals = []
    for k in range(-1, 17):
        v = f32(o + a * f32(k + 0.5))
        lo = hi = v
        vals.append(v)
        for _ in range(2):
            lo, hi = np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf))
            vals += [lo, hi]
    vals = np.array(vals, f32)
    assert vals.size == 90
    codes = fm.code(vals, a, o)
    assert 0 < np.count_nonzero(np.diff(np.sort(codes)))  # several levels are hit
    for dim in (92, 90):  # dim % 4 == 0: quantize16_kernel; 90: the dword kernel (and pad codes)
        x = np.zeros((3, dim), f32)
        x[0, :90], x[1, :90], x[2, :90] = vals, vals[::-1], np.roll(vals, 7)
        for dist in (D.Dot, D.L2):
            vp = qa.VectorParameters(dim, 3, dist, False)
            rows, meta = fm.encode(x, int(dist), False, False, alpha_offset=(a, o))
            for src in (torch.from_numpy(x).cuda(), x):
                h = E.encode(src, vp, alpha_offset=(float(a), float(o)), bits=4)
                _check_store(h, rows, meta, False, f"sweep dim {dim}")
            _check_query(h, meta, x[0], False, "sweep query")
            b = h.encode_query_batch(x[:2])
            got = h.score_batch(b)
            for i in range(2):
                qc, qoff = fm.encode_query(meta, x[i], False)
                assert_bits_equal(got[i], qo.u8_score_all(meta, rows, qc, qoff), f"sweep batch query {i}")


# ================================================================================================ 2. the nibble scan
BLOCK, RING = 64, 8
IMAGE_RCS = (2, 3, 2 * RING, 2 * RING + 1, 2 * RING + 2, 4 * RING, 48, 96, 127, 128)
BYTE_RCS = (1, 129)
SCAN_ROWS = (1, 63, 64, 65, 1023, 1025, 4099)
VARIANT_ROWS = (65, 1025)
VARIANTS = ((D.Dot, True), (D.L2, False), (D.L2, True))
TOPK_CASES = [(768, 20011, (100, 1024)), (144, 2_100_003, (30,))]
LAYOUT = [(32, 1), (48, 65), (272, 70), (768, 1025), (2048, 130)]
ALPHA = f32(1.0 / 15.0)


def store4(dim, n, dist=D.Dot, invert=False, seed=0, top=16):
    """(rows, from_storage metadata, oracle Meta, query): uniform random codes 0..top-1, alpha 1 / 15, offset 0."""
    rng = np.random.default_rng(dim * 131 + n * 7 + seed)
    rows = np.zeros((n, dim + 4), dtype=np.uint8)
    rows[:, :4] = rng.standard_normal(n).astype(f32).view(np.uint8).reshape(n, 4)
    rows[:, 4:] = rng.integers(0, top, size=(n, dim), dtype=np.uint8)
    meta = fm.make_meta(dim, n, int(dist), invert, ALPHA, f32(0.0))
    md = {"actual_dim": dim, "alpha": ALPHA, "offset": f32(0.0), "multiplier": f32(meta.multiplier),
          "vector_parameters": qa.VectorParameters(dim, n, dist, invert), "bits": 4}
    return rows, md, meta, rng.random(dim, dtype=f32)


def score_cases():
    cases = [(16 * rc, n, D.Dot, False) for rc in IMAGE_RCS + BYTE_RCS for n in SCAN_ROWS]
    return cases + [(16 * rc, n, dist, inv) for rc in IMAGE_RCS + BYTE_RCS for n in VARIANT_ROWS for dist, inv in VARIANTS]


def tag_of(dim, n, dist, inv):
    return f"all/{dim}x{n}/{int(dist)}{int(inv)}"


def expected_split(n, cu):
    blocks, split = -(-n // BLOCK), 1
    while split < 8 and blocks * split < 16 * cu:
        split *= 2
    return split


def child_main(out_path, mode):
    L = qa.lib()
    L.qamd_dev_u8_last_scan_packed.restype = C.c_int
    L.qamd_dev_u8_last_scan_split.restype = C.c_int
    L.qamd_dev_cu_count.restype = C.c_int
    R, info = {}, {"cu": int(L.qamd_dev_cu_count())}

    def seen(enc):
        return [int(L.qamd_dev_u8_last_scan_packed(enc._h)), int(L.qamd_dev_u8_last_scan_split(enc._h)), enc.scan_bytes_per_row()]

    def score(tag, rows, md, query):
        enc = E.from_storage(rows, md)
        R[tag] = enc.score_all(enc.encode_query(query))
        info[tag] = seen(enc)
        return enc

    for dim, n, dist, inv in score_cases():
        rows, md, _, query = store4(dim, n, dist, inv)
        score(tag_of(dim, n, dist, inv), rows, md, query)
    # every code 15 against a query of 15s at rc 128: the largest sums the kernel holds
    rows, md, _, _ = store4(2048, 130)
    rows[:, 4:] = 15
    score("all15", rows, md, np.full(2048, 2.0, f32))
    # one code of 16 (bytes another producer wrote): no image, the bytes are scanned
    rows, md, _, query = store4(768, 1025, seed=3)
    rows[1000, 4 + 700] = 16
    score("code16", rows, md, query)
    # the same at rc 3, row 65 of 70: in chunk 1, the high-nibble source of image chunk 0, and in chunk 2, the low-nibble
    # source of the odd last image chunk
    for chunk in (1, 2):
        rows, md, _, query = store4(48, 70, seed=chunk)
        rows[65, 4 + 16 * chunk + 5] = 16
        score(f"code16/chunk{chunk}", rows, md, query)
    if mode != "cu1":
        for dim, n, ks in TOPK_CASES:
            rows, md, _, query = store4(dim, n)
            enc = score(f"topk/{dim}x{n}/all", rows, md, query)
            q = enc.encode_query(query)
            for k in ks:
                ids, sc = enc.topk(q, k)
                R[f"topk/{dim}x{n}/{k}"] = np.stack([np.asarray(ids).view(f32), np.asarray(sc)])
                info[f"topk/{dim}x{n}/{k}"] = seen(enc)
            if n < 100_000:  # score_internal's epilogue on the scan and on the FILTER form, and the null id list
                i = n // 3
                R[f"internal/{dim}x{n}/all"] = enc.score_internal_all(i)
                info[f"internal/{dim}x{n}/all"] = seen(enc)
                ids, sc = enc.topk_internal(i, 100)
                R[f"internal/{dim}x{n}/topk"] = np.stack([np.asarray(ids).view(f32), np.asarray(sc)])
                info[f"internal/{dim}x{n}/topk"] = seen(enc)
                R[f"internal/{dim}x{n}/batch"] = enc.score_internal_all_batch(np.array([i, 5, n - 1], np.uint32), n_rows=4099)
                R[f"internal/{dim}x{n}/prefix"] = enc.score_internal_ids(i, None, n_rows=1025)
                info[f"internal/{dim}x{n}/prefix"] = seen(enc)
        import torch
        hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
        for dim, n in LAYOUT + [(768, 1026)]:
            rows, md, _, _ = store4(dim, n, seed=3 if n == 1026 else 0)
            if n == 1026:
                rows[1000, 4 + 700] = 16
            enc = E.from_storage(rows, md)
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
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_u8_four_bit as T\nT.child_main(%r, %r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), out, name))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=env)
    assert res.returncode == 0 and "DONE" in res.stdout, f"{name}: exit {res.returncode}\n{res.stderr[-4000:]}"
    with open(out + ".json") as f:
        info = json.load(f)
    return dict(np.load(out)), info


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("u8_four_bit")
    return {"nibble": run_child(d, "nibble", {}), "bytes": run_child(d, "bytes", {"QAMD_DEV_U8_PACKED": "0"}),
            "cu1": run_child(d, "cu1", {"QAMD_DEV_CU_COUNT": "1"})}


_WANT = {}


def want_scores(key, rows, meta, query):
    """The oracle's scores of store `key` on the model's query codes, computed once and shared by the tests."""
    if key not in _WANT:
        codes, qoff = fm.encode_query(meta, query, False)
        _WANT[key] = qo.u8_score_all(meta, rows, codes, qoff)
    return _WANT[key]


def check_tag(runs, tag, dim, n, rows, meta, query, names=("nibble", "bytes", "cu1"), image=True):
    want = want_scores(tag, rows, meta, query)
    rc = dim // 16
    for name in names:
        R, info = runs[name]
        assert_bits_equal(R[tag], want, f"{tag} ({name})")
        packed, split, per_row = info[tag]
        if name == "bytes" or not image:
            assert packed == 0 and per_row == dim + 4, (tag, name, packed, per_row)
        else:
            assert packed == 2, f"{tag} ({name}): the nibble scan did not run"
            assert split == expected_split(n, info["cu"]), (tag, name, split)
            assert per_row == 16 * ((rc + 1) // 2) + 4, (tag, name, per_row)


@pytest.mark.parametrize("rc", IMAGE_RCS + BYTE_RCS)
def test_nibble_scan_equals_bytes_and_oracle(runs, rc):
    for dim, n, dist, inv in score_cases():
        if dim == 16 * rc:
            rows, _, meta, query = store4(dim, n, dist, inv)
            check_tag(runs, tag_of(dim, n, dist, inv), dim, n, rows, meta, query, image=rc in IMAGE_RCS)


def test_both_dispatch_forms_ran(runs):
    info = runs["nibble"][1]
    assert info["cu"] >= 8, "these row counts are chosen for a GPU of at least 8 CUs"
    assert all(info[tag_of(768, n, D.Dot, False)][1] > 1 for n in SCAN_ROWS)
    one = runs["cu1"][1]
    assert one["cu"] == 1
    assert [one[tag_of(768, n, D.Dot, False)][1] for n in SCAN_ROWS] == [8, 8, 8, 8, 1, 1, 1]
    assert info["topk/144x2100003/all"][:2] == [2, 1], "the big store takes one wave per block"
    assert info["topk/768x20011/all"][2] == 388 and runs["bytes"][1]["topk/768x20011/all"][2] == 772


def test_largest_sums_and_a_code_of_16(runs):
    rows, _, meta, _ = store4(2048, 130)
    rows[:, 4:] = 15
    query = np.full(2048, 2.0, f32)
    assert fm.encode_query(meta, query, False)[0].min() == 15
    check_tag(runs, "all15", 2048, 130, rows, meta, query)
    rows, _, meta, query = store4(768, 1025, seed=3)
    rows[1000, 4 + 700] = 16
    check_tag(runs, "code16", 768, 1025, rows, meta, query, image=False)
    assert runs["nibble"][1]["layout/768x1026"][0] == 0
    for chunk in (1, 2):  # either source chunk of an image chunk drops the image
        rows, _, meta, query = store4(48, 70, seed=chunk)
        rows[65, 4 + 16 * chunk + 5] = 16
        check_tag(runs, f"code16/chunk{chunk}", 48, 70, rows, meta, query, image=False)


@pytest.mark.parametrize("case", TOPK_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_topk_through_the_filter_form(runs, case):
    dim, n, ks = case
    rows, _, meta, query = store4(dim, n)
    check_tag(runs, f"topk/{dim}x{n}/all", dim, n, rows, meta, query, names=("nibble", "bytes"))
    want = want_scores(f"topk/{dim}x{n}/all", rows, meta, query)
    for k in ks:
        wi, ws = topk_want(want, k, True)
        for name in ("nibble", "bytes"):
            R, info = runs[name]
            got = R[f"topk/{dim}x{n}/{k}"]
            assert np.array_equal(got[0].view(np.uint32), wi), f"{dim}x{n} topk {k} ({name}): ids differ"
            assert_bits_equal(got[1], ws, f"{dim}x{n} topk {k} ({name}) scores")
            assert info[f"topk/{dim}x{n}/{k}"][0] == (2 if name == "nibble" else 0), (name, k)


def test_score_internal_forms(runs):
    """score_internal_all, topk_internal (FILTER with score_internal's epilogue) and the null id lists."""
    dim, n = 768, 20011
    rows, _, meta, _ = store4(dim, n)
    i = n // 3
    want = {r: np.array([qo.u8_score_internal(meta, rows, r, j) for j in range(n if r == i else 4099)], f32) for r in (i, 5, n - 1)}
    wi, ws = topk_want(want[i], 100, True)
    for name in ("nibble", "bytes"):
        R, info = runs[name]
        assert_bits_equal(R[f"internal/{dim}x{n}/all"], want[i], f"score_internal_all ({name})")
        got = R[f"internal/{dim}x{n}/topk"]
        assert np.array_equal(got[0].view(np.uint32), wi), f"topk_internal ({name}): ids differ"
        assert_bits_equal(got[1], ws, f"topk_internal ({name})")
        for l, r in enumerate((i, 5, n - 1)):
            assert_bits_equal(R[f"internal/{dim}x{n}/batch"][l], want[r][:4099], f"score_internal_all_batch row {r} ({name})")
        assert_bits_equal(R[f"internal/{dim}x{n}/prefix"], want[i][:1025], f"score_internal_ids, null list ({name})")
        served = 2 if name == "nibble" else 0
        assert [info[f"internal/{dim}x{n}/{t}"][0] for t in ("all", "topk", "prefix")] == [served] * 3, name


@pytest.mark.parametrize("case", LAYOUT, ids=lambda c: f"{c[0]}x{c[1]}")
def test_image_matches_numpy_pack(runs, case):
    dim, n = case
    R, info = runs["nibble"]
    rc = dim // 16
    assert info[f"layout/{dim}x{n}"] == [(rc + 1) // 2, BLOCK]
    assert runs["bytes"][1][f"layout/{dim}x{n}"][0] == 0
    rows, _, _, _ = store4(dim, n)
    want = fm.block_image(fm.pack_rows(rows[:, 4:]), -(-n // BLOCK) * BLOCK)
    assert np.array_equal(R[f"layout/{dim}x{n}"], want), f"{dim}x{n}: nibble image"


# ================================================================================================ 3. the byte routes
@functools.lru_cache(maxsize=None)
def _served():
    """A rotated 4-bit store of 1025 x 768 (L2) and the model's, shared by the route tests."""
    c = _case(True, 768, 1025)
    return c, E.encode(c["x"], c["vp"], rotated=True, bits=4)


def test_point_ids_and_a_burst():
    c, h = _served()
    n = 1025
    q = h.encode_query(c["q"])
    codes, off = fm.encode_query(c["meta"], c["q"], True)
    want = qo.u8_score_all(c["meta"], c["rows"], codes, off)
    rng = np.random.default_rng(1)
    ids = rng.integers(0, n, size=200).astype(np.uint32)
    assert_bits_equal(np.array([h.score_point(q, 77)], f32), want[77:78], "score_point")
    assert_bits_equal(h.score_ids(q, ids), want[ids], "score_ids")
    assert_bits_equal(h.score_all(q), want, "score_all")
    offs = np.array([0, 3, 3, 120, 200], np.uint32)  # ragged, one empty list
    got = h.score_ids_batch(h.encode_query_batch(c["qs"][:4]), offs, ids)
    srows = np.array([5, 1024, 0, 512], np.uint32)
    got_i = h.score_internal_ids_batch(srows, offs, ids)
    for l in range(4):
        sel = ids[offs[l]:offs[l + 1]]
        qc, qoff = fm.encode_query(c["meta"], c["qs"][l], True)
        assert_bits_equal(got[offs[l]:offs[l + 1]], qo.u8_score_all(c["meta"], c["rows"], qc, qoff)[sel], f"burst list {l}")
        w = np.array([qo.u8_score_internal(c["meta"], c["rows"], int(srows[l]), int(j)) for j in sel], f32)
        assert_bits_equal(got_i[offs[l]:offs[l + 1]], w, f"score_internal burst list {l}")
    assert_bits_equal(np.array([h.score_internal(3, 900)], f32),
                      np.array([qo.u8_score_internal(c["meta"], c["rows"], 3, 900)], f32), "score_internal")


@pytest.mark.parametrize("nq", [5, 40])
def test_batches(nq):
    c, h = _served()
    qs = np.random.default_rng(nq).normal(size=(nq, 768)).astype(f32)
    b = h.encode_query_batch(qs)
    got = h.score_batch(b)
    ids, sc = h.topk_batch(b, 10)
    for i in (0, nq // 2, nq - 1):
        qc, qoff = fm.encode_query(c["meta"], qs[i], True)
        want = qo.u8_score_all(c["meta"], c["rows"], qc, qoff)
        assert_bits_equal(got[i], want, f"score_batch query {i}")
        wi, ws = topk_want(want, 10, True)
        assert np.array_equal(ids[i], wi), f"topk_batch query {i}"
        assert_bits_equal(sc[i], ws, f"topk_batch query {i}")


def test_rescored_and_lane_mode_1():
    c, h = _served()
    q = h.encode_query(c["q"])
    orig = qa.OriginalVectors.from_data(c["x"], c["vp"])  # plain originals: the base metric matches
    cids, _ = h.topk(q, 50)
    ids_r, sc_r = h.topk_rescored(q, orig, c["q"], 5, 50)
    ids_w, sc_w = orig.rerank(c["q"], cids, 5)
    assert np.array_equal(ids_r, ids_w)
    assert_bits_equal(sc_r, sc_w, "rescored")
    other = qa.OriginalVectors.from_data(c["x"], qa.VectorParameters(768, 1025, D.Dot, c["invert"]))
    with pytest.raises(qa.EncodingError):
        h.topk_rescored(q, other, c["q"], 1, 1)
    codes, off = fm.encode_query(c["meta"], c["q"], True)
    lanes = E.from_storage(h.storage_bytes(), h.metadata)
    lanes.set_lane_mode(1)
    assert lanes.scan_bytes_per_row() == 388  # the image is there; lane mode 1 reads the bytes all the same
    assert_bits_equal(lanes.score_all(lanes.encode_query(c["q"])),
                      qo.u8_score_all(c["meta"], c["rows"], codes, off, order=qo.ORDER_AVX2), "lane mode 1")


# ================================================================================================ the write paths
@pytest.mark.parametrize("rotated,dim", [(False, 130), (True, 768)])
def test_write_paths(rotated, dim, tmp_path):
    n = 65
    c = _case(rotated, dim, n)
    x, vp, dist, invert = c["x"], c["vp"], int(c["dist"]), c["invert"]
    kw = {"rotated": rotated, "bits": 4}
    cuts = [0, 1, 38, 39, n]

    def batches():
        yield x[:0]
        for a, b in zip(cuts[:-1], cuts[1:]):
            yield x[a:b]

    st = E.encode_stream(batches, vp, **kw)
    _check_store(st, c["rows"], c["meta"], rotated, "streaming, min/max")
    assert np.array_equal(st.storage_bytes(), E.encode(x, vp, **kw).storage_bytes())
    x130 = _data(130, dim, 9)  # from 127 rows on the quantile counts
    rows_q, meta_q = fm.encode(x130, dist, invert, rotated, quantile=0.98)
    st_q = E.encode_stream(lambda: iter([x130[:50], x130[50:]]), qa.VectorParameters(dim, 130, c["dist"], invert), 0.98, **kw)
    _check_store(st_q, rows_q, meta_q, rotated, "streaming, quantile")
    # upsert across the edge of the first 64-row block, append past the capacity: the final data under the store's interval
    p4 = (qo.u8_actual_dim(dim) // 16 + 1) // 2
    assert st.capacity == n and st.scan_bytes_per_row() == 16 * p4 + 4
    rng = np.random.default_rng(n + dim)
    extra = rng.normal(size=(4 + 1100, dim)).astype(f32)
    final = np.concatenate([x, extra[4:]])
    final[62:66] = extra[:4]
    st.upsert(62, extra[:4])  # rows 62 .. 64 overwritten, row 65 appended
    st.append(extra[5:])
    ao = (float(c["meta"].alpha), float(c["meta"].offset))
    rows_f, meta_f = fm.encode(final, dist, invert, rotated, alpha_offset=ao)
    assert st.count == n + 1100 and st.capacity >= st.count and st.bits == 4 and st.rotated == rotated
    assert np.array_equal(st.storage_bytes(), rows_f), "upsert / append"
    assert st.scan_bytes_per_row() == 16 * p4 + 4, "the image followed the rows"
    q_enc = _check_query(st, c["meta"], c["q"], rotated, "after upsert")
    codes, off = fm.encode_query(c["meta"], c["q"], rotated)
    want = qo.u8_score_all(meta_f, rows_f, codes, off)
    assert_bits_equal(st.score_all(q_enc), want, "scores after upsert")
    ids, sc = st.topk(q_enc, 100)
    wi, ws = topk_want(want, 100, True)
    assert np.array_equal(ids, wi)
    assert_bits_equal(sc, ws, "topk after upsert")
    # save -> load and metadata -> from_storage
    st.save(tmp_path / "rows.bin", tmp_path / "meta.json")
    text = (tmp_path / "meta.json").read_text()
    assert text.endswith((',"rotation":"HadamardBlocks"' if rotated else "}") + ',"bits":4}'), text
    assert f'"distance_type":"{c["dist"].name}"' in text and text.count('"bits"') == 1
    ld = E.load(tmp_path / "rows.bin", tmp_path / "meta.json", qa.VectorParameters(dim, n + 1100, c["dist"], invert))
    fs = E.from_storage(st.storage_bytes(), st.metadata)
    for h in (ld, fs):
        assert h.bits == 4 and h.rotated == rotated and h.metadata == st.metadata
        assert np.array_equal(h.storage_bytes(), rows_f)
        assert h.scan_bytes_per_row() == 16 * p4 + 4
        _check_query(h, c["meta"], c["q"], rotated, "reloaded")
        assert_bits_equal(h.score_all(h.encode_query(c["q"])), want, "reloaded scores")
    # a store without the flag writes exactly what it wrote before the flag existed, and stays a 7-bit store
    plain = E.encode(x, vp, rotated=rotated)
    plain.save(tmp_path / "p.bin", tmp_path / "p.json")
    rows7, meta7 = um.encode(x, dist, invert) if rotated else qo.u8_encode(x, dist, invert)
    m = plain.metadata
    text = (tmp_path / "p.json").read_text()
    assert '"bits"' not in text and "bits" not in m and plain.bits == 8
    assert text.startswith('{"actual_dim":%d,"alpha":' % m["actual_dim"])
    assert text.endswith('"vector_parameters":{"dim":%d,"count":%d,"distance_type":"%s","invert":%s}%s}'
                         % (dim, n, c["dist"].name, "true" if invert else "false", ',"rotation":"HadamardBlocks"' if rotated else ""))
    assert json.loads(text)["alpha"] == pytest.approx(float(meta7.alpha), rel=1e-6)
    assert (tmp_path / "p.bin").read_bytes() == rows7.tobytes()
    back = E.load(tmp_path / "p.bin", tmp_path / "p.json", vp)
    assert back.bits == 8 and back.scan_bytes_per_row() == qo.u8_actual_dim(dim) + 4


def test_refusals(tmp_path):
    got = fm.refusals(_lib, tmp_path)
    assert len(got) == 11 * 3 + 4 * 14 + 9
    for what, st, want, out in got:
        assert st == want and out is None, (what, st, want)
    x = np.ones((4, 128), f32)
    with pytest.raises(qa.EncodingError, match="Dot and L2"):
        E.encode(x, qa.VectorParameters(128, 4, D.L1, False), bits=4)
    with pytest.raises(qa.EncodingError, match="multiple of 64"):
        E.encode_stream(lambda: iter([x[:, :96]]), qa.VectorParameters(96, 4, D.L2, False), rotated=True, bits=4)
    with pytest.raises(qa.EncodingError, match="4-bit"):
        qa.ShardedVectorsU8.encode(x, qa.VectorParameters(128, 4, D.Dot, False), [0, 0], bits=4)
