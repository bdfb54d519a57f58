"""Full-range scalar-u8 stores in plain numpy: the quantizer with 255 levels, the row and query offsets,
the scores from int64 code sums through the f32 epilogue in the order 3.1w states, and the refusals of the flag."""
import ctypes as C
import json
import os

import numpy as np

f32 = np.float32
FULL, DOT, L1, L2 = 64, 0, 1, 2
LEGAL = (64, 65, 66, 72, 74)


def actual_dim(dim):
    return (dim + 15) // 16 * 16


def codes_of(v, alpha, offset):
    """trunc(clamp((v - offset) / alpha + 0.5, 0, 255)), each operation rounded to f32; NaN (a NaN value, a zero interval) -> 0."""
    with np.errstate(all="ignore"):
        x = np.clip((np.asarray(v, f32) - f32(offset)) / f32(alpha) + f32(0.5), f32(0), f32(255))
    return np.where(np.isnan(x), 0, x).astype(np.uint8)


def seq_sum(c):
    """Per row of c, the f32 sum of code terms: the exact integer below 2^24, else the sequential f32 sum in index order."""
    s = c.sum(axis=1)
    return np.where(s < 1 << 24, s.astype(f32), np.add.accumulate(c.astype(f32), axis=1, dtype=f32)[:, -1])


def interval(y):
    """alpha, offset of the min/max interval (NaN is no extreme)."""
    mn, mx = f32(np.nanmin(y)), f32(np.nanmax(y))
    return f32((mx - mn) / f32(255)), mn


def offsets_of(codes, meta, row):
    """Row offsets (row=True: with the D offset^2 head) or query offsets of [n, actual_dim] codes."""
    alpha, offset, c = meta["alpha"], meta["offset"], codes.astype(np.int64)
    with np.errstate(all="ignore"):
        tail = {DOT: lambda: seq_sum(c) * alpha * offset, L2: lambda: seq_sum(c * c) * alpha * alpha,
                L1: lambda: np.zeros(len(c), f32)}[meta["dist"]]()
        if row and meta["dist"] != L1:
            tail = f32(meta["actual_dim"]) * offset * offset + tail
    return (-tail if meta["invert"] else tail).astype(f32)


def pad_codes(values, meta):
    """[n, dim] values -> [n, actual_dim] codes, the pad being code(0) for Dot and code(offset) otherwise."""
    values = np.atleast_2d(np.asarray(values, f32))
    pad = codes_of(f32(0) if meta["dist"] == DOT else meta["offset"], meta["alpha"], meta["offset"])
    codes = np.full((len(values), meta["actual_dim"]), pad, np.uint8)
    codes[:, :values.shape[1]] = codes_of(values, meta["alpha"], meta["offset"])
    return codes


def encode(y, dist, invert, alpha, offset):
    """(rows [n, actual_dim + 4] u8 in the reference's row format, meta) of values y (already rotated for a rotated store)."""
    y = np.atleast_2d(np.asarray(y, f32))
    alpha, offset = f32(alpha), f32(offset)
    with np.errstate(all="ignore"):
        m = alpha * alpha if dist == DOT else alpha if dist == L1 else f32(-2) * alpha * alpha
    meta = dict(alpha=alpha, offset=offset, multiplier=f32(-m if invert else m), dist=dist, invert=invert, dim=y.shape[1],
                actual_dim=actual_dim(y.shape[1]))
    codes = pad_codes(y, meta)
    return np.concatenate([offsets_of(codes, meta, True).view(np.uint8).reshape(-1, 4), codes], axis=1), meta


def encode_query(meta, q):
    c = pad_codes(q, meta)
    return c[0], offsets_of(c, meta, False)[0]


def pair_sums(meta, rows, qcodes):
    """int64 [n]: sum c q, or sum |c - q| for L1."""
    c, q = rows[:, 4:].astype(np.int64), qcodes.astype(np.int64)
    return np.abs(c - q).sum(axis=1) if meta["dist"] == L1 else c @ q


def scores(meta, rows, qcodes, qoff):
    """(multiplier * f32(S) + q_off) + v_off, S converted once."""
    voff = np.ascontiguousarray(rows[:, :4]).view(f32)[:, 0]
    with np.errstate(all="ignore"):
        return ((meta["multiplier"] * pair_sums(meta, rows, qcodes).astype(f32) + f32(qoff)) + voff).astype(f32)


def scores_internal(meta, rows, i):
    """multiplier * f32(S) + ((off_i + off_j) - diff), diff = actual_dim * offset * offset (negated for invert)."""
    voff = np.ascontiguousarray(rows[:, :4]).view(f32)[:, 0]
    with np.errstate(all="ignore"):
        diff = f32(meta["actual_dim"]) * meta["offset"] * meta["offset"]
        diff = -diff if meta["invert"] else diff
        return (meta["multiplier"] * pair_sums(meta, rows, rows[i, 4:]).astype(f32) + ((voff[i] + voff) - diff)).astype(f32)


def refusals(lib_mod, tmp_path):
    """(what, status, wanted status, out handle) of every call that must refuse the flag before any device call."""
    L = lib_mod.lib()
    VPC, MC, stop = lib_mod.VectorParametersC, lib_mod.U8MetadataC, lib_mod.STOP_FN()
    out, dev0, got = C.c_void_p(), (C.c_int * 1)(0), []

    def note(what, st, want=lib_mod.ERR_ARGUMENTS):
        got.append((f"{what}: {(L.qamd_last_error() or b'').decode()}", st, want, out.value))

    for what, dim, dt in (("bits4", 128, 64 | 32), ("bits4 L2 rotated", 128, 64 | 42), ("compact", 128, 64 | 160),
                          ("L1 rotated", 128, 64 | 9), ("rotated dim 100", 100, 72), ("rotated dim 0", 0, 74),
                          ("rotated dim 16448", 16448, 74), ("dim 16385", 16385, 64), ("dim 20000 L1", 20000, 65),
                          ("3", 128, 67), ("bit 16", 128, 64 | 16), ("bit 256", 128, 64 | 256)):
        v = VPC(dim, 0, dt, 0)
        m = MC(actual_dim(dim), 1.0, 0.0, 1.0, v)
        note(f"u8_encode {what}", L.qamd_u8_encode(None, 0, C.byref(v), None, None, stop, None, None, C.byref(out)))
        note(f"u8_encoder_begin {what}", L.qamd_u8_encoder_begin(C.byref(v), None, None, stop, None, None, C.byref(out)))
        note(f"u8_from_rows {what}", L.qamd_u8_from_rows(None, 0, C.byref(m), None, C.byref(out)))
    for dt in LEGAL:
        v = VPC(128, 0, dt, 0)
        m, b = MC(128, 1.0, 0.0, 1.0, v), C.byref(v)
        note("pq_encode", L.qamd_pq_encode(None, 0, b, 8, None, 1, stop, None, None, C.byref(out)))
        note("pq_from_rows", L.qamd_pq_from_rows(None, 0, b, 8, C.c_void_p(1), None, C.byref(out)))
        note("pq_encoder_begin", L.qamd_pq_encoder_begin(b, 8, None, 1, stop, None, None, C.byref(out)))
        note("bin_encode", L.qamd_bin_encode(None, 0, b, 0, stop, None, None, C.byref(out)))
        note("bin_from_rows", L.qamd_bin_from_rows(None, 0, b, 0, None, C.byref(out)))
        note("bin_encoder_begin", L.qamd_bin_encoder_begin(b, 0, stop, None, None, C.byref(out)))
        note("f32_from_data", L.qamd_f32_from_data(None, 0, b, 0, None, C.byref(out)))
        note("u8_sharded_encode", L.qamd_u8_sharded_encode(None, 0, b, None, None, stop, None, dev0, 1, None, C.byref(out)))
        note("u8_sharded_from_rows", L.qamd_u8_sharded_from_rows(None, 0, C.byref(m), dev0, 1, None, C.byref(out)))
        note("bin_sharded_encode", L.qamd_bin_sharded_encode(None, 0, b, 0, stop, None, dev0, 1, None, C.byref(out)))
        note("pq_sharded_encode", L.qamd_pq_sharded_encode(None, 0, b, 8, None, 1, stop, None, dev0, 1, None, C.byref(out)))
    (tmp_path / "rows.bin").write_bytes(b"")
    for what, tail, dist, dim in (("false", ',"full_range":false', "Dot", 128), ("1", ',"full_range":1', "Dot", 128),
                                  ("a string", ',"full_range":"true"', "L2", 128), ("null", ',"full_range":null', "L1", 128),
                                  ("twice", ',"full_range":true,"full_range":true', "Dot", 128),
                                  ("beside bits", ',"bits":4,"full_range":true', "Dot", 128),
                                  ("before bits", ',"full_range":true,"bits":4', "L2", 128),
                                  ("dim 16385", ',"full_range":true', "Dot", 16385)):
        text = json.dumps({"actual_dim": actual_dim(dim), "alpha": 1.0, "offset": 0.0, "multiplier": 1.0,
                           "vector_parameters": {"dim": dim, "count": 0, "distance_type": dist, "invert": False}})
        (tmp_path / "meta.json").write_text(text[:-1] + tail + "}")
        v = VPC(dim, 0, 0, 0)
        note(f"u8_load full_range {what}", L.qamd_u8_load(os.fsencode(tmp_path / "rows.bin"), os.fsencode(tmp_path / "meta.json"),
                                                           C.byref(v), C.byref(out)), lib_mod.ERR_IO)
    return got
