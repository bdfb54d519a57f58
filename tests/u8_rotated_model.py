"""Model of a rotated scalar-u8 store (the reference has no counterpart).

y^ = c * rotated_blocks_model.rotate(x), c = 2^(-log2(B) / 2) rounded to f32 and one f32 multiply per value; everything
after y^ is the oracle's u8 encoder and query encoder (oracle/qoracle.py) run on y^.  No code shared with the library.
"""
from fractions import Fraction

import numpy as np

import rotated_blocks_model as bm
from oracle import qoracle as qo

f32 = np.float32
ROTATED, DOT_ROTATED, L2_ROTATED = 8, 8, 10
ROTATION_NAME = "HadamardBlocks"


def scale(b):
    """c for a block of b values: 2^(-k / 2), k = log2(b).  Exact for even k; for odd k the f32 nearest to
    sqrt(2^-k), found with exact rationals: among the double estimate's f32 and its two neighbours, walk upwards while
    sqrt(2^-k) lies above the midpoint to the next one, i.e. while 2^-k > midpoint^2."""
    k = b.bit_length() - 1
    assert b == 1 << k
    if k % 2 == 0:
        return f32(2.0 ** (-(k // 2)))
    est = f32(2.0 ** (-k / 2.0))
    cands = [np.nextafter(est, f32(0)), est, np.nextafter(est, f32(1))]
    best = cands[0]
    for nxt in cands[1:]:
        mid = (Fraction(float(best)) + Fraction(float(nxt))) / 2
        if Fraction(1, 1 << k) > mid * mid:
            best = nxt
    return f32(best)


def rotate(x):
    """[rows, dim] f32 -> y^ [rows, dim] f32."""
    x = np.atleast_2d(np.asarray(x, dtype=f32))
    with np.errstate(all="ignore"):
        return (bm.rotate(x) * scale(bm.block(x.shape[1]))).astype(f32)


def encode(x, distance, invert, quantile=None, alpha_offset=None):
    """(rows [count, dim + 4] u8, oracle Meta) of the rotated store of x; `distance` is the base metric."""
    y = rotate(x)
    if alpha_offset is not None:
        return qo.u8_encode_with(y, distance, invert, alpha_offset[0], alpha_offset[1])
    return qo.u8_encode(y, distance, invert, quantile)


def encode_query(meta, q):
    """(codes, offset) of a query against the rotated store."""
    return qo.u8_encode_query(meta, rotate(q)[0])


# ------------------------------------------------------------------------------------------------------- refusals
def refusals(lib_mod, tmp_path=None):
    """(what, status, wanted status) of every call a rotated flag must be refused by, each before any device call: the C
    entry points are called with null data and rows, which a call that got past its argument checks would report as such
    - with the same status - so `what` carries the library's message too.  Used by the CPU and the GPU test."""
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

    # the scalar-u8 constructors: L1 with the flag, a dim that is no multiple of 64, a dim above 16384, flags beyond 8
    for what, v in (("L1", vp(128, 9)), ("dim 100", vp(100, DOT_ROTATED)), ("dim 96", vp(96, L2_ROTATED)),
                    ("dim 0", vp(0, DOT_ROTATED)), ("dim 16448", vp(16448, L2_ROTATED)), ("bits", vp(128, 16 | 8)),
                    ("3 | 8", vp(128, 11))):
        note(f"u8_encode {what}", L.qamd_u8_encode(None, 0, C.byref(v), None, None, stop, None, None, C.byref(out)))
        note(f"u8_encoder_begin {what}", L.qamd_u8_encoder_begin(C.byref(v), None, None, stop, None, None, C.byref(out)))
        m = meta(v.dim, v.distance_type)
        note(f"u8_from_rows {what}", L.qamd_u8_from_rows(None, 0, C.byref(m), None, C.byref(out)))
    # every other constructor refuses the flag as such, on a shape a u8 store would take
    for dt in (DOT_ROTATED, L2_ROTATED):
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
    if tmp_path is not None:  # load: an unknown rotation, and the key beside L1 or a dim no rotated store has
        data = tmp_path / "rows.bin"
        data.write_bytes(b"")

        def load(what, dim, dist, rotation):
            obj = {"actual_dim": dim, "alpha": 1.0, "offset": 0.0, "multiplier": 1.0,
                   "vector_parameters": {"dim": dim, "count": 0, "distance_type": dist, "invert": False}}
            if rotation is not None:
                obj["rotation"] = rotation
            path = tmp_path / "meta.json"
            path.write_text(json.dumps(obj))
            v = vp(dim, 0)
            note(f"u8_load {what}", L.qamd_u8_load(os.fsencode(data), os.fsencode(path), C.byref(v), C.byref(out)),
                 lib_mod.ERR_IO)

        load("unknown rotation", 128, "Dot", "Hadamard")
        load("rotation of another type", 128, "Dot", 1)
        load("L1", 128, "L1", ROTATION_NAME)
        load("dim 96", 96, "Dot", ROTATION_NAME)
        load("dim 16448", 16448, "L2", ROTATION_NAME)
    return got
