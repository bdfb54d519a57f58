"""Model of a 4-bit scalar-u8 store (the reference has no counterpart), in numpy f32.

y = the row (plain) or u8_rotated_model.rotate(row) (rotated); [min, max] of all y from the oracle's find_min_max (which
keeps the first of equal values, so a zero extreme has the sign of the first zero) or find_quantile_interval;
offset = min, alpha = (max - min) / 15;  code(v) = trunc(clamp((v - offset) / alpha + 0.5, 0, 15)), NaN -> 0: subtract,
divide and add are three f32 operations, each rounded on its own.  Row offset, query offset and multiplier are the
reference's formulas (encoded_vectors_u8.rs:94-128, 307-324) in its operation order; the code sums are exact integers
far below 2^24, so the sequential f32 sum of the reference is that integer.  Scores are the oracle's on these rows and a
hand-filled Meta.  No code shared with the library.
"""
import numpy as np

import u8_rotated_model as um
from oracle import qoracle as qo

f32 = np.float32
BITS4, DOT_BITS4, L2_BITS4, DOT_ROTATED_BITS4, L2_ROTATED_BITS4 = 32, 32, 34, 40, 42
LEVELS = f32(15.0)


def code(v, alpha, offset, rounded=True):
    """u8 codes 0..15 of f32 values.  rounded=False: the truncating code the reference's f32_to_u8 would give at 15
    levels (the recall comparison alone uses it)."""
    v = np.asarray(v, dtype=f32)
    with np.errstate(all="ignore"):
        x = (v - f32(offset)) / f32(alpha)
        if rounded:
            x = x + f32(0.5)
        assert x.dtype == f32
        x = np.where(x < 0, f32(0), x)
        x = np.where(x > LEVELS, LEVELS, x)
        return np.where(np.isnan(x), f32(0), x).astype(np.uint8)  # 0 <= x <= 15: astype truncates


def interval(y, quantile=None):
    """(alpha, offset) of the values y [count, dim]."""
    mn, mx = qo.find_min_max(y)
    if quantile is not None:
        found = qo.find_quantile_interval(y, quantile)
        if found is not None:
            mn, mx = found
    with np.errstate(all="ignore"):
        return f32(f32(mx) - f32(mn)) / LEVELS, f32(mn)


def multiplier(alpha, distance, invert):
    alpha = f32(alpha)
    m = alpha * alpha if distance == qo.DOT else f32(-2.0) * alpha * alpha
    return f32(-m if invert else m)


def make_meta(dim, count, distance, invert, alpha, offset):
    m = qo.Meta()
    m.actual_dim, m.dim, m.count = qo.u8_actual_dim(dim), dim, count
    m.alpha, m.offset, m.multiplier = f32(alpha), f32(offset), multiplier(alpha, distance, invert)
    m.distance_type, m.invert = distance, int(bool(invert))
    return m


def _codes_and_sums(y, dim, alpha, offset, distance, rounded):
    ad = qo.u8_actual_dim(dim)
    codes = np.empty((y.shape[0], ad), np.uint8)
    codes[:, :dim] = code(y, alpha, offset, rounded)
    if ad != dim:  # the reference's placeholders, through code()
        codes[:, dim:] = code(f32(0.0) if distance == qo.DOT else f32(offset), alpha, offset, rounded)
    c = codes.astype(np.int64)
    s = c.sum(axis=1) if distance == qo.DOT else (c * c).sum(axis=1)
    assert s.max(initial=0) < 1 << 24  # exact in f32: the sequential sum is the integer
    return codes, s.astype(f32)


def encode_values(y, distance, invert, alpha, offset, rounded=True):
    """(rows [count, actual_dim + 4] u8, Meta) of values y that are quantized as they are."""
    y = np.atleast_2d(np.asarray(y, dtype=f32))
    count, dim = y.shape
    alpha, offset = f32(alpha), f32(offset)
    codes, s = _codes_and_sums(y, dim, alpha, offset, distance, rounded)
    D = f32(codes.shape[1])
    with np.errstate(all="ignore"):
        vo = D * offset * offset + (s * alpha * offset if distance == qo.DOT else s * alpha * alpha)
    vo = (-vo if invert else vo).astype(f32)
    rows = np.empty((count, codes.shape[1] + 4), np.uint8)
    rows[:, :4] = vo.view(np.uint8).reshape(count, 4)
    rows[:, 4:] = codes
    return rows, make_meta(dim, count, distance, invert, alpha, offset)


def encode(x, distance, invert, rotated, quantile=None, alpha_offset=None, rounded=True):
    """(rows, Meta) of the 4-bit store of x; `distance` is the base metric."""
    x = np.atleast_2d(np.asarray(x, dtype=f32))
    y = um.rotate(x) if rotated else x
    alpha, offset = alpha_offset if alpha_offset is not None else interval(y, quantile)
    return encode_values(y, distance, invert, alpha, offset, rounded)


def encode_query(meta, q, rotated, rounded=True):
    """(codes [actual_dim] u8, offset f32) of a query against the store."""
    q = np.asarray(q, dtype=f32)
    y = um.rotate(q)[0] if rotated else q
    alpha, offset = f32(meta.alpha), f32(meta.offset)
    codes, s = _codes_and_sums(y[None, :], y.shape[0], alpha, offset, meta.distance_type, rounded)
    with np.errstate(all="ignore"):
        off = s[0] * alpha * offset if meta.distance_type == qo.DOT else s[0] * alpha * alpha
    return codes[0], f32(-off if meta.invert else off)


# ------------------------------------------------------------------------------------------------------- nibble image
def pack_rows(codes):
    """[rows, 16 rc] codes 0..15 -> [rows, ceil(rc / 2), 16] image chunks: byte b of chunk j = codes[32 j + b] |
    codes[32 j + 16 + b] << 4, high nibbles of the last chunk zero when rc is odd."""
    codes = np.asarray(codes, np.uint8)
    n, ad = codes.shape
    rc = ad // 16
    p4 = (rc + 1) // 2
    c = np.zeros((n, 2 * p4, 16), np.uint8)
    c[:, :rc] = codes.reshape(n, rc, 16)
    return c[:, 0::2] | (c[:, 1::2] << 4)


def block_image(img, padded_rows):
    """[rows, P4, 16] -> the blocked image as bytes: chunk j of row r at 16-byte index ((r / 64) * P4 + j) * 64 + r % 64,
    padding rows zero."""
    n, p4, _ = img.shape
    full = np.zeros((padded_rows, p4, 16), np.uint8)
    full[:n] = img
    return full.reshape(padded_rows // 64, 64, p4, 16).transpose(0, 2, 1, 3).reshape(-1)


def lane_sum(img_row, qcodes, rc):
    """What one lane of the nibble scan adds up for its row: per image chunk the low nibbles against query chunk 2j and the
    unshifted high nibbles against chunk 2j + 1 (not read when the row has none), the high sum shifted once at the end."""
    q = np.asarray(qcodes, np.int64).reshape(rc, 16)
    lo = hi = 0
    for j in range(img_row.shape[0]):
        v = img_row[j].astype(np.int64)
        lo += int(((v & 0x0F) * q[2 * j]).sum())
        if 2 * j + 1 < rc:
            hi += int(((v & 0xF0) * q[2 * j + 1]).sum())
    assert hi % 16 == 0 and hi < 1 << 32 and lo < 1 << 32
    return lo + (hi >> 4)


# ------------------------------------------------------------------------------------------------------- refusals
def refusals(lib_mod, tmp_path=None):
    """(what, status, wanted status, out handle) of every call the 4-bit flag must be refused by, each before any device
    call: null data and rows, as in u8_rotated_model.refusals."""
    import ctypes as C
    import json
    import os

    L = lib_mod.lib()
    VPC, MC, stop = lib_mod.VectorParametersC, lib_mod.U8MetadataC, lib_mod.STOP_FN()
    out, dev0 = C.c_void_p(), (C.c_int * 1)(0)
    got = []

    def note(what, st, want=lib_mod.ERR_ARGUMENTS):
        msg = L.qamd_last_error()
        got.append((f"{what}: {msg.decode() if msg else ''}", st, want, out.value))

    def vp(dim, dt, count=0):
        return VPC(dim, count, dt, 0)

    def meta(dim, dt):
        return MC(dim, 1.0, 0.0, 1.0, vp(dim, dt))

    # the scalar-u8 constructors: L1 with the flag, other bits, the rotated form's dim rules
    for what, v in (("L1", vp(128, 1 | 32)), ("L1 rotated", vp(128, 1 | 8 | 32)), ("3 | 32", vp(128, 35)),
                    ("bit 16", vp(128, 16 | 32)), ("bit 16 rotated", vp(128, 16 | 8 | 32)), ("bit 64", vp(128, 64 | 32)),
                    ("bit 4", vp(128, 4 | 32)), ("rotated dim 100", vp(100, DOT_ROTATED_BITS4)),
                    ("rotated dim 96", vp(96, L2_ROTATED_BITS4)), ("rotated dim 0", vp(0, DOT_ROTATED_BITS4)),
                    ("rotated dim 16448", vp(16448, L2_ROTATED_BITS4))):
        note(f"u8_encode {what}", L.qamd_u8_encode(None, 0, C.byref(v), None, None, stop, None, None, C.byref(out)))
        note(f"u8_encoder_begin {what}", L.qamd_u8_encoder_begin(C.byref(v), None, None, stop, None, None, C.byref(out)))
        m = meta(v.dim, v.distance_type)
        note(f"u8_from_rows {what}", L.qamd_u8_from_rows(None, 0, C.byref(m), None, C.byref(out)))
    # every other constructor refuses the flag as such, on a shape a u8 store would take
    for dt in (DOT_BITS4, L2_BITS4, DOT_ROTATED_BITS4, L2_ROTATED_BITS4):
        v, m = vp(128, dt), meta(128, dt)
        b = C.byref(v)
        note("pq_encode", L.qamd_pq_encode(None, 0, b, 8, None, 1, stop, None, None, C.byref(out)))
        note("pq_from_rows", L.qamd_pq_from_rows(None, 0, b, 8, C.c_void_p(1), None, C.byref(out)))
        note("pq_encoder_begin", L.qamd_pq_encoder_begin(b, 8, None, 1, stop, None, None, C.byref(out)))
        note("bin_encode", L.qamd_bin_encode(None, 0, b, 0, stop, None, None, C.byref(out)))
        note("bin_encode_enc", L.qamd_bin_encode_enc(None, 0, b, 0, 20, None, None, stop, None, None, C.byref(out)))
        note("bin_from_rows", L.qamd_bin_from_rows(None, 0, b, 0, None, C.byref(out)))
        note("bin_encoder_begin", L.qamd_bin_encoder_begin(b, 0, stop, None, None, C.byref(out)))
        note("f32_from_data", L.qamd_f32_from_data(None, 0, b, 0, None, C.byref(out)))
        note("u8_sharded_encode", L.qamd_u8_sharded_encode(None, 0, b, None, None, stop, None, dev0, 1, None, C.byref(out)))
        note("u8_sharded_from_rows", L.qamd_u8_sharded_from_rows(None, 0, C.byref(m), dev0, 1, None, C.byref(out)))
        note("bin_sharded_encode", L.qamd_bin_sharded_encode(None, 0, b, 0, stop, None, dev0, 1, None, C.byref(out)))
        note("bin_sharded_from_rows", L.qamd_bin_sharded_from_rows(None, 0, b, 0, dev0, 1, None, C.byref(out)))
        note("pq_sharded_encode", L.qamd_pq_sharded_encode(None, 0, b, 8, None, 1, stop, None, dev0, 1, None, C.byref(out)))
        note("pq_sharded_from_rows", L.qamd_pq_sharded_from_rows(None, 0, b, 8, C.c_void_p(1), dev0, 1, None, C.byref(out)))
    if tmp_path is not None:  # load: a value other than 4, a repeated key, the key beside L1
        data = tmp_path / "rows.bin"
        data.write_bytes(b"")

        def load(what, dist, tail):
            text = json.dumps({"actual_dim": 128, "alpha": 1.0, "offset": 0.0, "multiplier": 1.0,
                               "vector_parameters": {"dim": 128, "count": 0, "distance_type": dist, "invert": False}})
            path = tmp_path / "meta.json"
            path.write_text(text[:-1] + tail + "}")
            v = vp(128, 0)
            note(f"u8_load {what}", L.qamd_u8_load(os.fsencode(data), os.fsencode(path), C.byref(v), C.byref(out)),
                 lib_mod.ERR_IO)

        load("bits 8", "Dot", ',"bits":8')
        load("bits 7", "L2", ',"bits":7')
        load("bits 4.5", "Dot", ',"bits":4.5')
        load("bits -4", "Dot", ',"bits":-4')
        load("bits as a string", "Dot", ',"bits":"4"')
        load("bits null", "Dot", ',"bits":null')
        load("bits twice", "Dot", ',"bits":4,"bits":4')
        load("bits beside L1", "L1", ',"bits":4')
        load("bits beside L1, rotated", "L1", ',"rotation":"HadamardBlocks","bits":4')
    return got
