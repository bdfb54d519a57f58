"""The u8 ENCODER's dispatch (csrc/u8.hip) restated, and the case lists of the tests that pin it.

Shared by tests/test_u8_encode_shapes_model.py (no GPU: keeps the lists honest, and proves on the oracle alone that
the data shows what it is meant to show) and tests/test_gpu_u8_encode_shapes.py (every case against the oracle, bit
for bit).  Nothing here needs a GPU or the library.

launch_quantize: an aligned source with dim % 4 == 0 goes to quantize16_kernel<IT, FAST> - 16 lanes per row, IT
float4 per lane from per_lane = ceil(actual_dim / 64), IT = 0 a run-time loop of 4-deep batches; FAST (the
division-free conversion) for alpha in 2^-60 .. 2^60.  Everything else goes to quantize_kernel (a wave per row, dword
loads).  MinMaxAcc::feed: an aligned source of at least 4 values goes to minmax_stream_kernel (a wave per tile of
1024 float4, whole or partial, 64 slots shared by the waves modulo 64) plus one scalar launch for the 1..3 values
behind the last float4; everything else to the grid-wide scalar minmax_kernel.
"""
import numpy as np

F32 = np.float32
TILE_F4 = 1024    # float4 per wave in minmax_stream_kernel
SLOTS = 64        # kMinmaxSlots
SAMPLE = 100_000  # kQuantileSample


def actual_dim(dim):
    return -(-dim // 16) * 16


def query_pad(dim):
    """Pad codes behind a query (or a row) of `dim` values."""
    return actual_dim(dim) - dim


# ------------------------------------------------------------------ launch_quantize
Q16_FORMS = (2, 4, 6, 8, 12, 16, 0)
FAST_LO, FAST_HI = F32(2.0 ** -60), F32(2.0 ** 60)


def fast_alpha(alpha):
    return bool(FAST_LO <= F32(alpha) <= FAST_HI)


def q16_iters(dim):
    per_lane = (actual_dim(dim) // 4 + 15) // 16
    for it in Q16_FORMS[:-1]:
        if per_lane <= it:
            return it
    return 0


def quantize_route(dim, aligned, alpha):
    """("q16", IT, fast) or ("rows",)."""
    if dim % 4 == 0 and aligned:
        return "q16", q16_iters(dim), fast_alpha(alpha)
    return ("rows",)


def q16_geometry(dim):
    """(dwords of a row, float4 of a row, dwords per batch): dwords - float4 pad dwords follow the data."""
    it = q16_iters(dim)
    return actual_dim(dim) // 4, dim // 4, 16 * (it or 4)


# ------------------------------------------------------------------ MinMaxAcc::feed
def minmax_route(n_values, aligned):
    """Which launches one feed() makes: {"full", "partial", "tail", "scalar", "wrap"} -> bool."""
    out = dict(full=False, partial=False, tail=False, scalar=False, wrap=False)
    if n_values == 0:
        return out
    if aligned and n_values >= 4:
        n4 = n_values // 4
        out["full"] = n4 >= TILE_F4
        out["partial"] = n4 % TILE_F4 != 0
        out["tail"] = n_values % 4 != 0
        out["wrap"] = -(-n4 // TILE_F4) > SLOTS
    else:
        out["scalar"] = True
    return out


def tile_position(wave, j, lane, comp):
    """Flat index of component `comp` of the float4 that lane `lane` loads as its piece `j` in tile `wave`."""
    return ((wave * TILE_F4 + j * 64 + lane) * 4) + comp


# ------------------------------------------------------------------ case lists: quantize16_kernel
# per form: the first dim with dim % 4 == 0 (only the low lanes are live in the last piece, the later pieces break),
# the last dim (exact), and a dim of dim % 16 == 12 (the row's last dword is padding)
Q16_DIMS = {
    2: dict(first=4, last=128, padded=124),
    4: dict(first=132, last=256, padded=252),
    6: dict(first=260, last=384, padded=380),
    8: dict(first=388, last=512, padded=508),
    12: dict(first=516, last=768, padded=764),
    16: dict(first=772, last=1024, padded=1020),
    0: dict(first=1028, padded=2044, whole=1280, partial=1100),  # no last dim; 1280: five whole batches; 1100: 4 + 20 / 64
}
ROWS_DIMS = [1, 2, 3, 17, 65, 257, 1101, 1102, 1103]  # quantize_kernel by dim % 4 != 0: short rows and rows past one 64-dword slab
UNALIGNED_DIMS = [64, 768, 1100]                      # quantize_kernel with dim % 4 == 0: the source is not 16-byte aligned
UNALIGNED_ODD_DIM = 65
ROW_COUNTS = (1, 2, 3, 5, 33, 131)                    # 1, 2, 3 mod 4 (row_ok / the clamped rc), more than one workgroup of 32 rows
SLOW_PAIRS = [(1e-25, 0.0), (1e25, 3.0)]              # alpha outside 2^-60 .. 2^60: FAST = false
BOUNDARY_PAIR = (1.0 / 127.0, -0.5)
STREAM_BATCHES = (1, 2, 5, 67)                        # then the rest: row0 = 1, 3, 8, 75
STREAM_ROWS = 131
UPSERT_FIRST_ROWS = (1, 2, 3, 6)
REPLAY_DIMS = [1100, 1101, 1102]
QUERY_DIMS = [1, 15, 16, 17, 65, 100, 1101]
QUERY_BATCHES = (1, 3, 65)


def all_q16_dims():
    return sorted(d for roles in Q16_DIMS.values() for d in roles.values())


def padded_dims():
    """One padded dim of each form (the row-offset and the boundary tests use them)."""
    return [Q16_DIMS[it]["padded"] for it in Q16_FORMS]


def metrics_of(dim, n):
    """[(metric name, invert)]: Dot, L2 and L1, `invert` rotating with the dim's place in the lists, the row count and
    the metric."""
    dims = all_q16_dims() + ROWS_DIMS + [UNALIGNED_ODD_DIM] + UNALIGNED_DIMS
    turn = dims.index(dim) + (ROW_COUNTS.index(n) if n in ROW_COUNTS else 0)
    return [(name, bool((turn + i) % 2)) for i, name in enumerate(("Dot", "L2", "L1"))]


# ------------------------------------------------------------------ data
# Values that leave a min / max interval alone (NaN never wins a comparison), and values that blow it up to infinity:
# rows with the second kind are encoded with a given (alpha, offset).
SOFT_SPECIALS = np.array([np.nan, 0.0, -0.0, 1e-45, -1e-45, 1e-39], dtype=F32)
HARD_SPECIALS = np.array([np.inf, -np.inf, 3.4e38, -3.4e38], dtype=F32)


def plant(data, values, shift=0):
    """`values` in the first and the last column and in the last row."""
    n, dim = data.shape
    for i, v in enumerate(values):
        data[(i + shift) % n, 0] = v
        data[(i + shift + 3) % n, dim - 1] = values[-1 - i]
        data[n - 1, (7 * (i + shift) + 1) % dim] = v
    return data


def signed_data(n, dim, seed=0):
    """Values in [-1, 1] with NaN, both zeros and denormals planted; from dim 8 on -1 and 1 are present, so that the
    minimum is negative (the Dot pad code is not 0) and the interval is the same for every row count."""
    rng = np.random.default_rng(1_000_003 * dim + 101 * n + seed)
    data = (rng.random((n, dim), dtype=F32) * F32(2) - F32(1)).astype(F32)
    plant(data, SOFT_SPECIALS)
    if dim >= 8:
        data[0, 2], data[0, 3] = F32(-1), F32(1)
    return data


def with_hard_specials(data):
    """A copy with +-inf and +-3.4e38 planted as well, behind the soft ones."""
    return plant(data.copy(), HARD_SPECIALS, shift=len(SOFT_SPECIALS))


def interval_data(n, dim, alpha, offset, seed=0):
    """offset + alpha * U(-2, 130), evaluated in f64 and rounded once."""
    rng = np.random.default_rng(7_000_001 * dim + 13 * n + seed)
    u = rng.uniform(-2.0, 130.0, (n, dim))
    with np.errstate(over="ignore"):
        return (np.float64(F32(offset)) + np.float64(F32(alpha)) * u).astype(F32)


def boundary_values(alpha, offset):
    """The f32 values within +-6 ulp of every code boundary offset + alpha * k, k = -2 .. 130."""
    a32, o32 = F32(alpha), F32(offset)
    vals = []
    for k in range(-2, 131):
        centre = F32(np.float64(o32) + np.float64(a32) * k)
        b = int(centre.view(np.int32))
        vals += [np.int32(b + d).view(F32) for d in range(-6, 7)]
    return np.array(vals, dtype=F32)


def boundary_data(dim, alpha, offset, seed=0):
    """Rows of boundary values laid out so that every row ENDS on them: the last real dword of each row (next to the
    pad dwords, if any) and its first dword hold boundary values; the rest is drawn from the interval."""
    vals = boundary_values(alpha, offset)
    n = -(-vals.size // 8) + 3
    data = interval_data(n, dim, alpha, offset, seed)
    for i in range(n):
        take = vals[(8 * i + np.arange(8)) % vals.size]
        k = min(4, dim)
        data[i, dim - k:] = take[:k]
        data[i, :k] = take[4:4 + k]
    return data


def replay_data(n, dim, seed=0):
    """L2 rows whose sum of squared codes passes 2^24: the minimum 0 and the maximum 1 are present, so alpha = 1 / 127
    and offset = 0.  Even rows are drawn from [0.75, 1] (codes 95 .. 127: 1104 of them stay below 2^24, the integer
    rounded once is the answer), odd rows from [0.975, 1] (codes 123 .. 127, sums of 1.7e7: the sequential f32 sum)."""
    rng = np.random.default_rng(33_331 * dim + n + seed)
    data = (F32(0.75) + rng.random((n, dim), dtype=F32) * F32(0.25)).astype(F32)
    data[1::2] = (F32(0.975) + rng.random(data[1::2].shape, dtype=F32) * F32(0.025)).astype(F32)
    data[0, 0] = F32(0.0)
    data[0, 1] = F32(1.0)
    return data


def seq_f32_sum_of_squares(codes):
    s = F32(0.0)
    for c in np.asarray(codes, dtype=F32):
        s = F32(s + c * c)
    return s


# ------------------------------------------------------------------ min / max: planted extremes
# (name, n_values, aligned, flat position of the minimum, flat position of the maximum)
def planted_cases():
    cases = []
    n = 2 * TILE_F4 * 4  # two whole tiles
    for lane in range(64):  # every lane; component and piece rotate along
        lo = tile_position(0, lane % 16, lane, lane % 4)
        other = (lane + 21) % 64
        hi = tile_position(1, (lane + 5) % 16, other, (lane + 1) % 4)
        cases.append((f"lane{lane}", n, True, lo, hi))
    for j in range(16):     # every piece and component at one lane
        for comp in range(4):
            cases.append((f"piece{j}.{comp}", n, True, tile_position(1, j, 37, comp), tile_position(0, 15 - j, 38, 3 - comp)))
    n4 = TILE_F4 + 300      # a whole and a partial tile
    cases.append(("partial_last_f4", n4 * 4, True, n4 * 4 - 1, n4 * 4 - 4))
    cases.append(("partial_last_f4_swapped", n4 * 4, True, n4 * 4 - 3, n4 * 4 - 2))
    cases.append(("tile_boundary", 12_000, True, TILE_F4 * 4 - 1, TILE_F4 * 4))
    cases.append(("tile_boundary_swapped", 12_000, True, 2 * TILE_F4 * 4, 2 * TILE_F4 * 4 - 2))
    for t in (1, 2, 3):     # the 1..3 values behind the last float4
        for p in range(t):
            cases.append((f"tail{t}.{p}_min", n4 * 4 + t, True, n4 * 4 + p, 5))
            cases.append((f"tail{t}.{p}_max", n4 * 4 + t, True, 4099, n4 * 4 + p))
    big = 270_000           # 66 tiles: waves 64 and 65 share the slots of waves 0 and 1
    cases.append(("wave64_min", big, True, tile_position(64, 3, 17, 2), tile_position(0, 9, 40, 1)))
    cases.append(("wave64_max", big, True, tile_position(0, 9, 40, 1), tile_position(64, 3, 17, 2)))
    cases.append(("wave65_min", big, True, tile_position(65, 2, 5, 0), tile_position(1, 0, 63, 3)))
    cases.append(("wave65_max", big, True, tile_position(1, 0, 63, 3), tile_position(65, 2, 5, 0)))
    m = 5003                # the scalar form: an unaligned device pointer
    cases.append(("scalar_first_min", m, False, 0, m - 1))
    cases.append(("scalar_first_max", m, False, m - 1, 0))
    cases.append(("scalar_middle", m, False, 2501, 1023))
    for k in (1, 2, 3):     # fewer than 4 values: scalar, aligned or not
        cases.append((f"short{k}", k, True, 0, k - 1))
    return cases


def planted_array(n_values, lo_at, hi_at, seed=0):
    """Values in [1, 2] with one unique minimum 0.5 and one unique maximum 3.0 (one value: the minimum only)."""
    data = (F32(1) + np.random.default_rng(n_values + seed).random(n_values, dtype=F32)).astype(F32)
    data[hi_at] = F32(3.0)
    data[lo_at] = F32(0.5)
    return data


# ------------------------------------------------------------------ signed zero
# (name, rows, dim, flat position of +0.0, flat position of -0.0, "min" | "max"); data in (0, 1] for "min", [-1, 0) for "max"
ZERO_CASES = [
    ("lane_min_plus_first", 2, 130, 4, 256, "min"),
    ("lane_min_minus_first", 2, 130, 256, 4, "min"),
    ("slot_min_plus_first", 2, 131_200, 0, 64 * 4096, "min"),
    ("slot_min_minus_first", 2, 131_200, 64 * 4096, 0, "min"),
    ("lane_max_plus_first", 2, 130, 4, 256, "max"),
    ("lane_max_minus_first", 2, 130, 256, 4, "max"),
    ("slot_max_plus_first", 2, 131_200, 0, 64 * 4096, "max"),
    ("slot_max_minus_first", 2, 131_200, 64 * 4096, 0, "max"),
]


def zero_array(rows, dim, plus_at, minus_at, which, seed=0):
    rng = np.random.default_rng(rows * dim + seed)
    data = (F32(1) - rng.random((rows, dim), dtype=F32)).astype(F32)  # (0, 1]
    if which == "max":
        data = -data
    flat = data.reshape(-1)
    flat[plus_at] = F32(0.0)
    flat[minus_at] = F32(-0.0)
    return data


def mixed_zeros(rows, dim, first_negative):
    """All zeros, the signs mixed; the first value decides."""
    data = np.where(np.random.default_rng(dim).random((rows, dim)) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
    data[0, 0] = F32(-0.0) if first_negative else F32(0.0)
    data[0, 1] = F32(0.0) if first_negative else F32(-0.0)
    return data


# ------------------------------------------------------------------ quantile
QUANTILES = (0.5, 0.9, 0.99)
QUANTILE_SHAPES = [(100_000, 1), (40_000, 3), (15_000, 8)]  # (count, dim): count <= 100 000, up to 120 000 values
SAMPLED_SHAPES = [(100_003, 4), (100_003, 7), (150_000, 4), (150_000, 7)]
SAMPLED_BATCH = 33_332  # at 150 000 rows the second batch begins on a row that is no sample row
SAMPLED_QUANTILE = 0.98


def quantile_cut(count, dim, quantile):
    """quantile.rs:52-56 for the sample of min(count, 100 000) vectors."""
    s = min(count, SAMPLE)
    return max(1, min((s * dim - 1) // 2, int(F32(F32(F32(s) * F32(F32(1.0) - F32(quantile))) / F32(2.0)))))


def clustered_data(count, dim, seed=0):
    """Values that share their top 24 bits, under both signs: a radix select decides only in its last digit."""
    rng = np.random.default_rng(count * dim + seed)
    low = rng.integers(0, 256, count * dim, dtype=np.uint32)
    sign = rng.integers(0, 2, count * dim, dtype=np.uint32) << np.uint32(31)
    return (np.uint32(0x3FC0_0100) | low | sign).view(F32).reshape(count, dim)


def repeated_data(count, dim, quantile, seed=0):
    """70 000 copies of 1.5 laid over the lower cut rank (or as many as fit), distinct values around them, no zero."""
    n = count * dim
    cut = quantile_cut(count, dim, quantile)
    copies = min(70_000, n - 200)
    below = min(max(cut - 10, 50), n - copies - 50)
    rng = np.random.default_rng(n + seed)
    data = np.empty(n, dtype=F32)
    data[:below] = (F32(-2) + rng.random(below, dtype=F32)).astype(F32)                         # [-2, -1)
    data[below:below + copies] = F32(1.5)
    data[below + copies:] = (F32(2) + rng.random(n - below - copies, dtype=F32)).astype(F32)    # [2, 3)
    return rng.permutation(data).reshape(count, dim)


def sample_rows(n):
    """Sample slot k of a store of n > 100 000 rows holds row floor(k * n / 100 000)."""
    return (np.arange(SAMPLE, dtype=np.int64) * n) // SAMPLE
