"""The row-length dispatch of csrc/pq.hip restated in Python, and the case lists built on it.

tests/test_gpu_pq_row_shapes.py runs these lists on the GPU; tests/test_pq_row_shapes_model.py (no GPU) asserts that they
reach every instantiation the dispatch can launch, so that a change to a ladder in pq.hip or to a list here turns that
test red instead of quietly losing coverage.  Nothing here calls the library: it is arithmetic on m, the chunks (= code
bytes) of a row, and on row counts.

An instantiation is a tuple (kernel name, template arguments ...):
  ("pq_scan_skew_kernel", NV, R, FILTER, SLICED, COAL, PAD)   ("pq_scan_fast_kernel", NVS, UNROLL, FILTER, SIMPLE)
  ("pq_scan_kernel", LUT_IN_LDS, VEC16)                       ("pq_topk_small_kernel", VEC16)
  ("pq_lists_kernel", VEC16)                                  ("pq_lists_staged_kernel", NP)
  ("pq_scan_seq_kernel", NVS, UNROLL, FILTER)                 ("pq_scan_seq_rows_kernel", STAGE)
pq_internal_pairs_kernel has no template arguments; its paths are the trips of its 16-lane loop (pairs_path).
"""
from binary_row_shapes import fused_policy, round_up, small_topk_plan  # topk.hip, restated once for both quantizers

CENTROIDS = 256
LDS_BUDGET = 160 * 1024 - 1024              # kLdsBudget
MAX_SLICE_PIECES, SLICE_PIECES_ALIGNED = 9, 8
PLANAR_MAX_ROWS, SKEW_MAX_ROWS = 1 << 28, 1 << 30
LIST_STAGE_MIN, LIST_STAGE_PAIRS = 128, 1024
CUS = 256
CHUNK = 4                                    # chunk size of the stores; their dim, 4 m - 1, leaves the last chunk short

# ------------------------------------------------------------------ the case lists
# Query scan (score_all at >= 4096 rows, topk(100) at FUSED_ROWS): one m per instantiation of launch_fast
WHOLE_RING_MS = (16, 32, 48, 64, 96, 128)                  # whole ring rows; 16 and 48: two store rows per ring row
PADDED_MS = {200: 20, 416: 40, 400: 56, 616: 76, 600: 88, 816: 104, 800: 120}  # pad / 16 * 100 + pad_bytes -> m
PLANAR_MS = (160, 192, 224, 320)                           # SLICED: 128 + 32, 96 + 96, 128 + 96, 128 + 128 + 64
FAST_FIRST_MS = tuple(16 * (nvs - 1) + 1 for nvs in range(2, 10))   # 17 .. 129: m % 4 == 1, a nearly empty last piece
FAST_LAST_MS = tuple(16 * nvs - 1 for nvs in range(2, 10))          # 31 .. 143: m % 4 == 3
FAST_OTHER_MS = (132, 144)                                 # m % 4 == 0 past the padded ring rows; the product's one SIMPLE
PITCH_MS = (257, 145, 161, 177, 193, 209, 225, 241)        # 128-byte pitch: a last slice of 1, 2, ... 8 pieces
SCAN_MS = sorted(WHOLE_RING_MS + tuple(PADDED_MS.values()) + PLANAR_MS + FAST_FIRST_MS + FAST_LAST_MS + FAST_OTHER_MS + PITCH_MS)
SIMPLE_MS = tuple(range(16, 129, 16))                      # with the skew kernel off: SIMPLE fast forms NVS 1 .. 8
FUSED_K = 100
FUSED_ROWS = 32768 + 37

# pq_scan_kernel: every groups % 4 x m % 4 remainder of both VEC16 forms, the LUT read from global memory
SMALL_SCAN_MS = tuple(range(1, 65)) + (159, 160, 512)
SMALL_SCAN_ROWS = 301
LDS_SCAN_MS = (1, 3, 8, 12, 13, 15)                        # LUT_IN_LDS: >= 4096 rows of fewer than 16 chunks
LDS_SCAN_ROWS = 4096 + 13
IDS_SCAN_MS = (159, 160)                                   # score_ids with >= 4096 ids on both sides of the LDS budget
IDS_SCAN_IDS = 4100

SMALL_TOPK_MS = (1, 3, 8, 12, 13, 17, 31, 128)
SMALL_TOPK_KS = (1, 64)
SMALL_TOPK_ROWS = 2 * 512 + 16 + 1                         # three workgroups, the last one ragged by a tile of one row
NOT_SMALL_TOPK_M = 129

# score_ids_batch: pq_lists_kernel over SMALL_SCAN_MS (short lists), pq_lists_staged_kernel<NP> at the first and last m
STAGED_FIRST_MS = (13, 15) + tuple(16 * (np_ - 1) + 1 for np_ in range(2, 10))  # ds = 16 from m = 13 on; 15: odd tail
STAGED_LAST_MS = tuple(16 * np_ for np_ in range(1, 10))
NOT_STAGED_MS = (150, 160)                                 # 256-byte rows (NP would be 16); a 160 KiB LUT
# the long-list layout of test_gpu_bursts.py with one list more (839 pairs), which ends a list on a workgroup range (4096)
LONG_LIST_LENS = (3000, 0, 130, 127, 839, 1500, 1, 0, 700, 1024, 1024, 4000, 128, 5)
LISTS_ROWS = 3000

PAIR_MS = (1, 15, 16, 17, 31, 32, 33, 150)
PAIR_CHUNKS = (1, 3, 8)                                    # chunk sizes; dim leaves the last chunk short where it can
PAIR_ROWS = 250                                            # every last-chunk code but the planted ones at most once

SEQ_FIRST_MS = (16,) + tuple(16 * (nvs - 1) + 1 for nvs in range(2, 10))
SEQ_LAST_MS = tuple(16 * nvs for nvs in range(1, 10))
SEQ_PLANAR_MS = (160, 192, 320)
SEQ_PITCH_MS = (257, 145, 241)                             # a last pitch slice of 1, 2 and 8 pieces
SEQ_MS = sorted(set(SEQ_FIRST_MS + SEQ_LAST_MS + SEQ_PLANAR_MS + SEQ_PITCH_MS))
SEQ_ROWS_STAGED_MS = (1, 7, 15)                            # pq_scan_seq_rows_kernel<true>, LDS_SCAN_ROWS rows
SEQ_ROWS_MS = (3, 100, 200)                                # pq_scan_seq_rows_kernel<false>, SMALL_SCAN_ROWS rows

METRICS = [(dist, inv) for dist in ("Dot", "L1", "L2") for inv in (False, True)]  # (DistanceType name, invert)
ALL_MS = sorted(set(SCAN_MS) | set(SMALL_SCAN_MS) | set(SEQ_MS) | set(PAIR_MS) | set(STAGED_FIRST_MS + STAGED_LAST_MS + NOT_STAGED_MS)
                | set(SEQ_ROWS_MS + SEQ_ROWS_STAGED_MS + SMALL_TOPK_MS + (NOT_SMALL_TOPK_M,) + LDS_SCAN_MS + IDS_SCAN_MS))
# all six metrics on one m per kernel of each family
ALL_METRICS_MS = {"scan": (96, 104, 192, 143, 257), "small_scan": (15, 63), "lds_scan": (12, 15), "small_topk": (12, 31),
                  "staged": (144,), "lists": (15, 63), "pairs": (33,), "seq": (97, 144, 192, 257), "seq_rows": (15, 100)}


def metric_of(m):
    """The (distance, invert) an m is run with where a test takes one metric per m: rotating with the m."""
    return METRICS[ALL_MS.index(m) % len(METRICS)]


def metrics_of(m, family):
    return METRICS if m in ALL_METRICS_MS[family] else [metric_of(m)]


def dim_chunk_of(m, chunk=CHUNK):
    """(dim, chunk size) of the stores: a last chunk one dimension short (chunk size 1 has none)."""
    return (m * chunk - 1 if chunk > 1 else m), chunk


# ------------------------------------------------------------------ alloc_store / plan_slices
def valid_pieces(m):
    return (m + 15) // 16


def plan_slices(m):
    """[(first chunk, chunks)] of the planar scan image, [] where the store has none."""
    if valid_pieces(m) <= MAX_SLICE_PIECES or m % 32:
        return []
    per = 96 if m % 96 == 0 and m <= 288 else 128
    return [(c, min(per, m - c)) for c in range(0, m, per)]


def planar(m, n=0):
    return bool(plan_slices(m)) and n < PLANAR_MAX_ROWS


def ds_of(m, n=0):
    """Device row stride: dword rows below 16 chunks, 16-byte pieces, the 128-byte pitch for rows of several slices that
    have no planar image."""
    if m < 16:
        return round_up(max(m, 1), 4)
    if valid_pieces(m) > MAX_SLICE_PIECES and not planar(m, n):
        return round_up(m, 16 * SLICE_PIECES_ALIGNED)
    return round_up(m, 16)


# ------------------------------------------------------------------ launch_fast
def skew_waves(m_ring):
    return 8 if m_ring > 96 else 16


def skew_rows_per_ring_row(m, n, skew=True):
    if not skew or ds_of(m, n) != m or n >= SKEW_MAX_ROWS:
        return 0
    if m % 32 == 0 and m <= 128:
        return 1
    return 2 if m in (48, 16) else 0


def skew_padded_ring(m, n, skew=True):
    """(chunks of the padded ring row, its bytes past ds); (0, 0): not a padded shape."""
    ds = ds_of(m, n)
    if not skew or n >= SKEW_MAX_ROWS or m % 4 or ds % 16 or ds < 32 or ds > 128 or ds != round_up(m, 16):
        return 0, 0
    ring = round_up(ds, 32)
    if ring == m or m in (48, 16):
        return 0, 0
    return ring, ring - ds


PADDED_KEYS = {200: (2, 0), 400: (4, 0), 416: (4, 16), 600: (6, 0), 616: (6, 16), 800: (8, 0), 816: (8, 16)}  # -> (NV, PAD)


def skew_run_shift(n, rows_per_ring_row, grid, m_ring):
    n_blocks = (-(-n // rows_per_ring_row) + 15) // 16
    return 2 if n_blocks >= 16 * grid * skew_waves(m_ring) else 0


def launch_fast(m, n, filt, skew=True, cus=CUS):
    """One entry per launch of a whole-store scan that is fast_capable."""
    pieces = valid_pieces(m)
    per = pieces if pieces <= MAX_SLICE_PIECES else SLICE_PIECES_ALIGNED
    n_slices = -(-pieces // per)
    grid = min(cus, -(-n // 1024))
    ring_rows = skew_rows_per_ring_row(m, n, skew)
    pad, pad_bytes = skew_padded_ring(m, n, skew)
    if pad or ring_rows:
        if pad:
            nv, pd = PADDED_KEYS[pad // 16 * 100 + pad_bytes]
            r = 1
        elif ring_rows == 2:
            nv, r, pd = (6 if m == 48 else 2), 2, 0
        else:
            nv, r, pd = m // 16, 1, 0
            assert nv in (2, 4, 6, 8)
        run_shift = skew_run_shift(n, 1 if pad else ring_rows, grid, pad if pad else ring_rows * m)
        return [("pq_scan_skew_kernel", nv, r, filt, False, (not filt) and r == 1 and run_shift == 2, pd)]
    if skew and planar(m, n):
        out, slices = [], plan_slices(m)
        for i, (_c0, chunks) in enumerate(slices):
            assert chunks // 16 in (2, 4, 6, 8) and chunks % 16 == 0
            coal = (not filt) and skew_run_shift(n, 1, grid, chunks) == 2 and i + 1 == len(slices)
            out.append(("pq_scan_skew_kernel", chunks // 16, 1, filt, True, coal, 0))
        return out
    simple = n_slices == 1 and m % 16 == 0
    return [("pq_scan_fast_kernel", min(per, pieces - sl * per), 4, filt, simple) for sl in range(n_slices)]


def fast_capable(m, n, count):
    return n >= 4096 and m >= 16 and n == count


def scan_launch(m, n, count, ids=False, filt=False, skew=True):
    """scan_launch: a scan of n rows (ids: of n ids) of a store of `count` rows."""
    if not ids and fast_capable(m, n, count):
        return launch_fast(m, n, filt, skew)
    assert not filt
    in_lds = m * CENTROIDS * 4 <= LDS_BUDGET and n >= 4096
    return [("pq_scan_kernel", in_lds, ds_of(m, count) % 16 == 0)]


def scan_kernel_name(m, n, skew=True):
    """qamd_pq_scan_kernel: (name, launches) of the whole-store scan."""
    if not fast_capable(m, n, n):
        return "pq_scan_kernel", 1
    launches = launch_fast(m, n, False, skew)
    name = launches[0][0]
    if name == "pq_scan_skew_kernel" and launches[0][4]:
        name += "<SLICED>"
    return name, len(launches)


def scan_tile(m, n, skew=True):
    """Rows a wave takes per step of the whole-store scan: 16 * UNROLL; the skew kernel's blocks of 16 ring rows."""
    first = launch_fast(m, n, False, skew)[0]
    return 16 * first[2]


def scan_rows(tile):
    """Row counts of the score-form tests: exactly 4096 rows (four full workgroups), a last tile ragged by one row, and
    one more workgroup than that, of one row."""
    ragged = 4096 + tile - 1
    return 4096, ragged, 1024 * -(-ragged // 1024) + 1


# ------------------------------------------------------------------ topk
def topk_route(m, n, k, skew=True):
    """("small", VEC16) | ("classic", launches) | ("fused", filter launches) | ("classic-fast", launches)."""
    if m >= 1 and m * CENTROIDS * 4 <= 128 * 1024 and small_topk_plan(n, k, 16, 512) is not None:
        return "small", [("pq_topk_small_kernel", ds_of(m, n) % 16 == 0)]
    if not fast_capable(m, n, n):
        return "classic", scan_launch(m, n, n)
    if fused_policy(n, k)[0]:
        return "fused", scan_launch(m, n, n, filt=True, skew=skew)
    return "classic-fast", scan_launch(m, n, n, skew=skew)


# ------------------------------------------------------------------ qamd_pq_score_ids_batch
def lists_launch(m, count, n_pairs, n_lists):
    ds = ds_of(m, count)
    if (n_pairs >= 4096 and n_pairs // n_lists >= 2 * LIST_STAGE_MIN and m * CENTROIDS * 4 <= LDS_BUDGET
            and ds % 16 == 0 and ds // 16 <= 10):
        return [("pq_lists_staged_kernel", ds // 16)]
    return [("pq_lists_kernel", ds % 16 == 0)]


# ------------------------------------------------------------------ score_internal_all / topk_internal
def seq_quad_capable(m, n):
    return n >= 4096 and m >= 16


def seq_slices(m, n):
    """Chunks per slice of seq_launch_quad: the planar image's slices, else launch_fast's pieces of the row-major image."""
    if planar(m, n):
        return [chunks for _c0, chunks in plan_slices(m)]
    pieces = valid_pieces(m)
    per = pieces if pieces <= MAX_SLICE_PIECES else SLICE_PIECES_ALIGNED
    return [min(per * 16, m - p0 * 16) for p0 in range(0, pieces, per)]


def seq_launch(m, n, filt=False):
    if seq_quad_capable(m, n):
        return [("pq_scan_seq_kernel", -(-c // 16), 2 if -(-c // 16) == 9 else 4, filt) for c in seq_slices(m, n)]
    assert not filt
    return [("pq_scan_seq_rows_kernel", m < 16 and n >= 4096)]


def seq_tile(m, n):
    return 16 * seq_launch(m, n)[0][2]


def topk_internal_route(m, n, k):
    if not seq_quad_capable(m, n):
        return "classic", seq_launch(m, n)
    if fused_policy(n, k)[0]:
        return "fused", seq_launch(m, n, True)
    return "classic-fast", seq_launch(m, n)


# ------------------------------------------------------------------ the remainders of the four-lanes-per-row kernels
def quad_path(m, n=0):
    """pq_scan_kernel / pq_topk_small_kernel / pq_lists_kernel: (VEC16, trips of the four-group vector loop > 0,
    groups left to the dword loop, chunks of the m % 4 tail)."""
    vec16 = ds_of(m, n) % 16 == 0
    groups = m // 4
    return vec16, (groups // 4 > 0) if vec16 else False, groups % 4 if vec16 else min(groups, 4), m % 4


def pairs_path(m):
    """pq_internal_pairs_kernel: (trips of the 16-lane loop, live lanes of the last trip)."""
    trips = -(-m // 16)
    return trips, m - 16 * (trips - 1)


# ------------------------------------------------------------------ what exists, and what nothing reaches
def existing():
    """Every instantiation the launch code of pq.hip names, by family."""
    skew = set()
    for filt in (False, True):
        coals = (False,) if filt else (False, True)
        for nv in (2, 4, 6, 8):
            for sliced in (False, True):
                skew |= {("pq_scan_skew_kernel", nv, 1, filt, sliced, coal, 0) for coal in coals}
        skew |= {("pq_scan_skew_kernel", nv, 1, filt, False, coal, 16) for nv in (4, 6, 8) for coal in coals}
        skew |= {("pq_scan_skew_kernel", 6, 2, filt, False, False, 0), ("pq_scan_skew_kernel", 2, 2, filt, False, False, 0)}
    return {
        "skew": skew,
        "fast": {("pq_scan_fast_kernel", nvs, 4, f, s) for nvs in range(1, 10) for f in (False, True) for s in (False, True)},
        "scan": {("pq_scan_kernel", l, v) for l in (False, True) for v in (False, True)},
        "small": {("pq_topk_small_kernel", v) for v in (False, True)},
        "lists": {("pq_lists_kernel", v) for v in (False, True)},
        "staged": {("pq_lists_staged_kernel", np_) for np_ in range(1, 11)},
        "seq": {("pq_scan_seq_kernel", nvs, 2 if nvs == 9 else 4, f) for nvs in range(1, 10) for f in (False, True)},
        "seq_rows": {("pq_scan_seq_rows_kernel", s) for s in (False, True)},
    }


# Forms that exist and that no store of 1 .. 1024 chunks reaches in the product library at the row counts of these tests.
UNREACHABLE = {
    "staged": {("pq_lists_staged_kernel", 10):
               "ds = 160 is m = 160 alone (m = 145 .. 159 sit on the 128-byte pitch, ds = 256), and its LUT, 160 KiB, "
               "is over kLdsBudget"},
    "fast": {("pq_scan_fast_kernel", nvs, 4, f, True):
             "m = 16 NVS <= 128 is a shape of pq_scan_skew_kernel; only QAMD_PQ_SKEW=0 (developer library), a device that "
             "refuses the skew kernel's LDS or a store of 2^30 rows leaves it to this form"
             for nvs in range(1, 9) for f in (False, True)},
    "skew": {e: "the run / coalesced-store form needs 16 runs of four blocks per wave: about a million rows "
                "(test_pq_skewed_scan_shapes reaches it)"
             for e in existing()["skew"] if e[5]},
}


# ------------------------------------------------------------------ the stores of the GPU file
def stores():
    """[(family, m, rows, chunk size)] of every store tests/test_gpu_pq_row_shapes.py builds (util.pq_shape_store); a
    test that runs fewer rows takes a prefix.  "query" families are scored with encoded queries, "row" with stored rows."""
    out = []
    for m in SCAN_MS:
        out += [("query", m, scan_rows(scan_tile(m, 4096))[-1], CHUNK), ("query", m, FUSED_ROWS, CHUNK)]
    for m in SIMPLE_MS:
        out += [("query", m, scan_rows(64)[-1], CHUNK), ("query", m, FUSED_ROWS, CHUNK)]
    out += [("query", m, SMALL_SCAN_ROWS, CHUNK) for m in SMALL_SCAN_MS + IDS_SCAN_MS]
    out += [("query", m, LDS_SCAN_ROWS, CHUNK) for m in LDS_SCAN_MS]
    out += [("query", m, SMALL_TOPK_ROWS, CHUNK) for m in SMALL_TOPK_MS + (NOT_SMALL_TOPK_M,)]
    out += [("query", m, LISTS_ROWS, CHUNK) for m in STAGED_FIRST_MS + STAGED_LAST_MS + NOT_STAGED_MS]
    out += [("row", m, PAIR_ROWS, chunk) for m in PAIR_MS for chunk in PAIR_CHUNKS]
    for m in SEQ_MS:
        out += [("row", m, scan_rows(seq_tile(m, 4096))[-1], CHUNK), ("row", m, FUSED_ROWS, CHUNK)]
    out += [("row", m, LDS_SCAN_ROWS, CHUNK) for m in SEQ_ROWS_STAGED_MS]
    out += [("row", m, SMALL_SCAN_ROWS, CHUNK) for m in SEQ_ROWS_MS]
    return sorted(set(out))
