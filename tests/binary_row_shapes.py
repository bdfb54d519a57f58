"""The row-length dispatch of csrc/bin.hip restated in Python, and the case lists built on it.

tests/test_gpu_binary_row_shapes.py runs these lists on the GPU; tests/test_binary_row_shapes_model.py (no GPU) asserts
that they reach every instantiation the dispatch can launch, so that a change to a ladder in bin.hip or to a list here
turns that test red instead of quietly losing coverage.  Nothing here calls the library except ds_of().

A row of `ds` device bytes is rc = ds / 16 sixteen-byte pieces.  The single-query kernels take it as
  W4 / W8   bin_words_kernel: rows of 4 and 8 bytes (up to 32 and 64 dimensions of the U8 store kind)
  S1 .. S64 bin_scan_kernel<G, ITERS, UNROLL>: G lanes per row, ITERS pieces per lane, (64 / G) * UNROLL rows per wave;
            EXACT when rc == G * ITERS, else the masked form (clamped loads, zeroed pieces)
  WL        bin_words_kernel: rc > 64
"""
import math

# ------------------------------------------------------------------ the case lists
# Per shape: its first rc at a dim that does not fill the last piece, its last masked rc, its EXACT rc.
SHAPE_DIMS = {
    "W4": (1, 32),
    "W8": (33, 64),
    "S1": (65, 128),
    "S2": (129, 256),
    "S4": (257, 384, 512),
    "S8": (513, 896, 1024),
    "S16": (1025, 1920, 2048),
    "S32": (2049, 3968, 4096),
    "S48": (4097, 6016, 6144),
    "S64": (6145, 8064, 8192),
    "WL": (8193, 8320),
}
U128_DIMS = (1, 100)  # S1 in the U128 store kind: 16-byte rows of few dimensions
S_SHAPES = ("S1", "S2", "S4", "S8", "S16", "S32", "S48", "S64")
PLANE_SMALL_SHAPES = ("S1", "S2", "S4", "S8", "S16")  # the single-launch top-k takes plane queries up to 16 pieces
PLANES = (1, 4, 8)
DIMS = [d for dims in SHAPE_DIMS.values() for d in dims]  # ascending
S_DIMS = [d for s in S_SHAPES for d in SHAPE_DIMS[s]]
METRICS = [(dist, inv) for dist in ("Dot", "L1", "L2") for inv in (False, True)]  # (DistanceType name, invert)
ALL_METRICS_DIMS = [dims[-1] for dims in SHAPE_DIMS.values()]  # all six metrics at one dim per shape

SMALL_KS = (1, 64)
CLASSIC_K = 65
FUSED_K = 100
FUSED_ROWS = 32768 + 37
# one masked dim (S1 and S2 have none: their unaligned dim) and the EXACT dim of every S shape
FUSED_DIMS = [d for s in S_SHAPES for d in (SHAPE_DIMS[s][-2], SHAPE_DIMS[s][-1])]
CLASSIC_DIMS = [SHAPE_DIMS[s][-2] for s in S_SHAPES]
# Fused stores whose scores all have one sign, on the shapes whose UNROLL is below G (a lane that holds no row's score
# passes bin_scan_kernel's epilogue only by its `sub <= u - first`, and what it holds is 0.0): a masked and the EXACT dim
ONE_SIGN_DIMS = [d for s in ("S16", "S32", "S48", "S64") for d in SHAPE_DIMS[s][-2:]]
ONE_SIGN_CALLS = [("Dot", False, True), ("L2", False, False)]  # negative scores, the largest; positive, the smallest
MULTI_ROWS = 4095  # below the 4096-row matrix-core gate of score_batch
MULTI_QUERIES = 15
MULTI_DIMS = (1024, 1025, 2048, 2049, 4096, 4097, 6145, 8192)
MULTI_FILTER_CASES = [(1025, 11), (2049, 11), (4097, 11), (8192, 11), (1024, 4), (1024, 2)]  # (dim, queries)
PAIR_TRIP_DIMS = {1025: 9, 4096: 32, 4097: 33, 8193: 65}  # dim -> pieces of the pair kernel's 4-in-flight loop


def metric_of(dim):
    """The (distance, invert) a dim is run with where a test takes one metric per dim: rotating with the dim."""
    return METRICS[DIMS.index(dim) % len(METRICS)]


def metrics_of(dim):
    return METRICS if dim in ALL_METRICS_DIMS else [metric_of(dim)]


def shape_of_dim(dim):
    return next(s for s, dims in SHAPE_DIMS.items() if dim in dims)


# ------------------------------------------------------------------ row sizes
def ds_of(dim, kind=0):
    """Device row stride of a store: get_quantized_vector_size_from_params, rows below 8 bytes held at 4."""
    from util import bin_row_bytes

    nb = bin_row_bytes(dim, kind)
    return nb if nb >= 8 else 4


def fused_capable(ds):
    return ds % 16 == 0 and ds // 16 <= 64


# ------------------------------------------------------------------ scan_planes / launch_bin
# name, G, ITERS, UNROLL, first rc, last rc
SCAN_LADDER = [("S1", 1, 1, 4, 1, 1), ("S2", 2, 1, 4, 2, 2), ("S4", 4, 1, 8, 3, 4), ("S8", 8, 1, 16, 5, 8),
               ("S16", 16, 1, 8, 9, 16), ("S32", 16, 2, 4, 17, 32), ("S48", 16, 3, 4, 33, 48), ("S64", 16, 4, 2, 49, 64)]
WORDS = (16, 0, 1)  # bin_words_kernel: 16 lanes per row at dword granularity, four rows per wave and step


def scan_shape(ds, planes=1):
    """scan_bits: (name, G, ITERS, UNROLL, exact); exact is None for bin_words_kernel."""
    if not fused_capable(ds):
        return ("W4" if ds == 4 else "W8" if ds == 8 else "WL",) + WORDS + (None,)
    rc = ds // 16
    for name, g, iters, unroll, _first, last in SCAN_LADDER:
        if rc <= last:
            if name == "S8" and planes > 1:
                unroll = 8
            return name, g, iters, unroll, rc == g * iters
    raise AssertionError(rc)


def scan_tile(ds, planes=1):
    _, g, _, unroll, _ = scan_shape(ds, planes)
    return (64 // g) * unroll


def scan_rows(ds, planes=1):
    """Row counts of the score-form test: a lone row, a ragged single tile, a second wave, a second workgroup (eight
    waves) whose last tile is ragged."""
    _, g, _, _, _ = scan_shape(ds, planes)
    tile = scan_tile(ds, planes)
    return (1, tile - 1, tile + 1, 8 * tile + 64 // g + 1)


# ------------------------------------------------------------------ launch_small / bin_small_plan / small_topk_plan
def small_shape(ds, planes=1):
    """(name, G, ITERS, exact) of bin_topk_small_kernel, None where the single launch does not apply."""
    if not fused_capable(ds) or (planes != 1 and ds // 16 > 16):
        return None
    name, g, iters, _, exact = scan_shape(ds)
    return name, g, iters, exact


def round_up(x, m):
    return -(-x // m) * m


def small_tile_least(ds):
    g = scan_shape(ds)[1]
    tile = 2 * (64 // g)
    return tile, round_up(max(16 * tile, (128 * 1024) // ds, tile), tile)


def small_topk_plan(n, k, tile, min_rows_per_wg, cus=256):
    """topk.hip small_topk_plan: (workgroups, rows per workgroup), None where the single launch does not apply."""
    if n == 0 or n > 2 << 20 or k == 0 or k > 64:
        return None
    least = round_up(max(min_rows_per_wg, tile), tile)
    wgs = min(cus, 256, -(-n // least))
    per = round_up(-(-n // wgs), tile)
    return -(-n // per), per


def small_plan(n, k, ds, planes=1, cus=256):
    """(workgroups, rows per workgroup) of the single launch, None where it does not apply."""
    if small_shape(ds, planes) is None:
        return None
    tile, least = small_tile_least(ds)
    return small_topk_plan(n, k, tile, least, cus)


def small_rows(ds):
    """Rows of the single-launch tests: at least three workgroups, the last one ragged."""
    tile, least = small_tile_least(ds)
    return 2 * least + tile + 1


# ------------------------------------------------------------------ multi_step / the batch loops
def multi_shape(ds, nq):
    """(G, ITERS, UNROLL, exact) of bin_scan_multi_kernel for a step of nq in (8, 4, 2) queries, None: no such step."""
    rc = ds // 16
    if ds % 16 or rc < 8 or rc > 64:
        return None
    if rc == 8:
        g, iters, unroll = 8, 1, 8
    elif rc <= 16:
        g, iters, unroll = 16, 1, 4
    elif rc <= 32:
        g, iters, unroll = 16, 2, 2
    elif nq <= 4:
        g, iters, unroll = 16, 4, 2
    else:
        return None
    return g, iters, unroll, rc == g * iters


def multi_steps(ds, queries):
    """The steps qamd_bin_score_batch and the filter pass of fused_topk_batch take over a binary batch off the matrix
    cores: the widest of 8, 4, 2 that fits what is left and has a form, else a single-query scan."""
    out, left = [], queries
    while left:
        took = next((nq for nq in (8, 4, 2) if left >= nq and multi_shape(ds, nq)), 1)
        out.append(took)
        left -= took
    return out


def mfma_capable(ds, dim):
    return fused_capable(ds) and 32 * ((ds // 16) * 128 + 16) + 2048 <= 160 * 1024 and dim >= 64


def score_batch_on_mfma(ds, dim, n, queries):
    return queries >= 5 and n >= 4096 and mfma_capable(ds, dim)


def topk_batch_on_mfma(ds, dim, n, queries, k):
    """Binary batches: 3 or 5+ queries on 512 / 768 / 1024 / 1536-bit rows, kRs4MinQueries = 12 elsewhere."""
    enough = (queries == 3 or queries >= 5) if ds in (64, 96, 128, 192) else queries >= 12
    return enough and n >= 32768 and k <= 1024 and mfma_capable(ds, dim)


def fused_policy(n, k):
    """topk.hip: (fused?, sample size S, pivot rank r)."""
    small = n < 1 << 20
    target = max(512.0 if small else 2048.0, 3.0 * k)
    sample = int(min(131072.0, max(2048.0 if small else 16384.0, float(round_up(int(8.0 * n / target), 1024)))))
    r = math.ceil(sample * target / max(n, 1))
    return n >= 32768 and r <= 64, sample, r


# ------------------------------------------------------------------ bin_pairs_kernel
def pairs_path(ds, planes=1):
    """("dword",): rows of 4 and 8 bytes; ("planes", pieces): the plane loop, 8 lanes; ("piece", pieces): one piece per
    lane; ("loop", pieces, trips, live slots of the last trip): four pieces in flight per lane, 32 per trip."""
    if ds % 16:
        return ("dword",)
    chunks = ds // 16
    if planes > 1:
        return "planes", chunks
    if chunks <= 8:
        return "piece", chunks
    trips = -(-chunks // 32)
    return "loop", chunks, trips, chunks - 32 * (trips - 1)
