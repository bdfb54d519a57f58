"""Model of a compact 4-bit scalar-u8 store in numpy: what the two kernels that read the nibble image
in place of byte codes compute, restated from the image format alone, and the calls the flag must be refused by.

A compact store is a 4-bit store (u8_four_bit_model) that keeps its row offsets and the blocked nibble image and nothing
else, so the model of its answers is u8_four_bit_model's; what is new is the address a pair kernel gathers a row's
chunks from and the expansion of a chunk back into codes.  No code shared with the library.
"""
import numpy as np

import u8_four_bit_model as fm

COMPACT = 128
DOT_BITS4_COMPACT, L2_BITS4_COMPACT, DOT_ROTATED_BITS4_COMPACT, L2_ROTATED_BITS4_COMPACT = 160, 162, 168, 170
LEGAL = (DOT_BITS4_COMPACT, L2_BITS4_COMPACT, DOT_ROTATED_BITS4_COMPACT, L2_ROTATED_BITS4_COMPACT)
BLOCK = 64


def chunks_of(actual_dim):
    """16-byte image chunks per row: ceil(actual_dim / 32)."""
    return (actual_dim // 16 + 1) // 2


def gather_index(r, j, chunks):
    """16-byte index of image chunk j of row r: ((r / 64) * chunks + j) * 64 + r % 64."""
    return ((r // BLOCK) * chunks + j) * BLOCK + r % BLOCK


def unpack_row(blocked, r, rc):
    """The 16 rc byte codes of row r out of the blocked image (bytes): chunk j gives code chunk 2j from its low nibbles and,
    where the row has it, code chunk 2j + 1 from its high nibbles."""
    img = np.asarray(blocked, np.uint8).reshape(-1, 16)
    p = (rc + 1) // 2
    out = np.empty((rc, 16), np.uint8)
    for j in range(p):
        w = img[gather_index(r, j, p)]
        out[2 * j] = w & 0x0F
        if 2 * j + 1 < rc:
            out[2 * j + 1] = w >> 4
    return out.reshape(-1)


def pair_sum(blocked, r, rc, qcodes=None, qrow=None):
    """The integer a 16-lane group of the pair kernel adds up for row r: lane `sub` takes chunks sub, sub + 16, ..., low
    nibbles against query chunk 2j and high nibbles against 2j + 1 (not read when the row has none); the query is byte
    codes, or stored row `qrow` expanded the same way."""
    img = np.asarray(blocked, np.uint8).reshape(-1, 16)
    p = (rc + 1) // 2
    q = None if qcodes is None else np.asarray(qcodes, np.int64).reshape(rc, 16)
    lanes = [0] * 16
    for j in range(p):
        w = img[gather_index(r, j, p)].astype(np.int64)
        if q is None:
            wq = img[gather_index(qrow, j, p)].astype(np.int64)
            qa, qb = wq & 0x0F, wq >> 4
        else:
            qa, qb = q[2 * j], (q[2 * j + 1] if 2 * j + 1 < rc else np.zeros(16, np.int64))
        lanes[j % 16] += int(((w & 0x0F) * qa).sum()) + int(((w >> 4) * qb).sum())
    return sum(lanes)


def store_bytes(padded_rows, actual_dim):
    """Device bytes of a compact store: the image and the f32 offsets."""
    return padded_rows * (16 * chunks_of(actual_dim) + 4)


# ------------------------------------------------------------------------------------------------------- refusals
def refusals(lib_mod, tmp_path=None):
    """(what, status, wanted status, out handle) of every call the compact flag must be refused by, each before any
    device call: null data and rows, as in u8_four_bit_model.refusals."""
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
        return MC((dim + 15) // 16 * 16, 1.0, 0.0, 1.0, vp(dim, dt))

    # the scalar-u8 constructors: the flag without QAMD_BITS4, with L1, with an unknown bit, on rows without a nibble image
    for what, v in (("alone", vp(128, 128)), ("alone on L2", vp(128, 2 | 128)), ("rotated, no bits", vp(128, 8 | 128)),
                    ("L1", vp(128, 1 | 32 | 128)), ("L1 rotated", vp(128, 1 | 8 | 32 | 128)), ("3", vp(128, 3 | 32 | 128)),
                    ("bit 64", vp(128, 64 | 160)), ("bit 16", vp(128, 16 | 160)), ("bit 4 rotated", vp(128, 4 | 168)),
                    ("bit 256", vp(128, 256 | 162)), ("dim 16", vp(16, 160)), ("dim 1", vp(1, 162)), ("dim 0", vp(0, 160)),
                    ("dim 2049", vp(2049, 160)), ("dim 4096", vp(4096, 162)), ("rotated dim 4096", vp(4096, 168)),
                    ("rotated dim 100", vp(100, 170))):
        note(f"u8_encode {what}", L.qamd_u8_encode(None, 0, C.byref(v), None, None, stop, None, None, C.byref(out)))
        note(f"u8_encoder_begin {what}", L.qamd_u8_encoder_begin(C.byref(v), None, None, stop, None, None, C.byref(out)))
        m = meta(v.dim, v.distance_type)
        note(f"u8_from_rows {what}", L.qamd_u8_from_rows(None, 0, C.byref(m), None, C.byref(out)))
    # every other constructor refuses the flag as such, on a shape a compact u8 store would take
    for dt in LEGAL:
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
    # the flag with only the 128 bit set among the u8 flags reaches the others as an unknown metric
    v = vp(128, 128)
    note("pq_encode 128", L.qamd_pq_encode(None, 0, C.byref(v), 8, None, 1, stop, None, None, C.byref(out)))
    note("bin_encode 128", L.qamd_bin_encode(None, 0, C.byref(v), 0, stop, None, None, C.byref(out)))
    note("f32_from_data 128", L.qamd_f32_from_data(None, 0, C.byref(v), 0, None, C.byref(out)))
    if tmp_path is not None:  # load: a value other than true, a repeated key, the key without "bits":4, rows with no image
        data = tmp_path / "rows.bin"
        data.write_bytes(b"")

        def load(what, tail, dist="Dot", dim=128):
            text = json.dumps({"actual_dim": (dim + 15) // 16 * 16, "alpha": 1.0, "offset": 0.0, "multiplier": 1.0,
                               "vector_parameters": {"dim": dim, "count": 0, "distance_type": dist, "invert": False}})
            path = tmp_path / "meta.json"
            path.write_text(text[:-1] + tail + "}")
            v = vp(dim, 0)
            note(f"u8_load {what}", L.qamd_u8_load(os.fsencode(data), os.fsencode(path), C.byref(v), C.byref(out)),
                 lib_mod.ERR_IO)

        load("compact false", ',"bits":4,"compact":false')
        load("compact 1", ',"bits":4,"compact":1')
        load("compact as a string", ',"bits":4,"compact":"true"')
        load("compact null", ',"bits":4,"compact":null')
        load("compact twice", ',"bits":4,"compact":true,"compact":true')
        load("compact without bits", ',"compact":true')
        load("compact without bits, rotated", ',"rotation":"HadamardBlocks","compact":true')
        load("compact before a bad bits", ',"compact":true,"bits":8')
        load("compact beside L1", ',"bits":4,"compact":true', dist="L1")
        load("compact at dim 16", ',"bits":4,"compact":true', dim=16)
        load("compact at dim 2049", ',"bits":4,"compact":true', dim=2049)
    return got


N_REFUSALS = 17 * 3 + 4 * 14 + 3 + 11
