"""The u8 ENCODER's kernels on every shape their dispatch knows, against the oracle, bit for bit.

The scan side is pinned shape by shape in test_gpu_u8_byte_kernels.py; this file does the same for the kernels behind
`encode`, `encode_stream`, `upsert`, `find_min_max`, `find_quantile_interval`, `encode_query` and `encode_query_batch`
(csrc/u8.hip): the fourteen quantize16_kernel<IT, FAST> forms at the first, the last and a padded dim of each,
quantize_kernel (dim % 4 != 0, or a source that is not 16-byte aligned), minmax_stream_kernel and minmax_kernel with
the extremes PLANTED at chosen lanes, pieces, components, tiles and tails, the three routes that gather the quantile
sample of a store above 100 000 rows, and the two query encoders.  tests/u8_encode_shapes.py restates the dispatch and
holds the case lists; tests/test_u8_encode_shapes_model.py (no GPU) keeps them honest and proves on the oracle alone
that the data shows what it is meant to show (a non-zero pad code, sums past 2^24 whose sequential f32 sum differs).

Every comparison is with oracle/qoracle.py on the raw bits: codes, vector offsets, the three metadata floats.  No
tolerance appears anywhere.

The sign of a zero minimum or maximum is the sign of the FIRST zero in row order (quantile.rs:5-19 keeps the first of
equal values): pinned for find_min_max, encode, encode_stream across batches and the sharded encoder across shards.

Two places where the data differs from a literal reading of the issue that asked for this file, both forced by its own
checks: rows with +-inf or +-3.4e38 are encoded with a GIVEN interval (a min / max interval over them is infinite and
every code 0 - the clean rows beside them pin the interval), and the sum-replay rows alternate between [0.75, 1] and
[0.975, 1] (1104 codes of 95 .. 127 sum to 1.4e7, below 2^24; codes of 123 .. 127 pass it).  The quantile's zero sign
at the two ranks is left open by the reference's unstable select, so the quantile data holds no zero.
"""
import numpy as np
import pytest

import u8_encode_shapes as S
from util import assert_bits_equal, bits

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
D = qa.DistanceType
F32 = np.float32
U8 = qa.EncodedVectorsU8


def vp_of(dim, n, name, invert):
    return qa.VectorParameters(dim, n, D[name], invert)


def same_bits(a, b):
    return bits(a)[0] == bits(b)[0]


def check_meta(md, meta, what):
    for field in ("alpha", "offset", "multiplier"):
        assert same_bits(md[field], getattr(meta, field)), f"{what}: metadata {field} {md[field]!r}, want {getattr(meta, field)!r}"
    assert md["actual_dim"] == meta.actual_dim


def check_store(enc, rows, meta, what):
    got = enc.storage_bytes()
    bad = np.argwhere(got[:, 4:] != rows[:, 4:])
    assert bad.size == 0, (f"{what}: {len(bad)} codes differ, first at row {bad[0][0]} byte {bad[0][1]}: "
                           f"got {got[bad[0][0], 4 + bad[0][1]]} want {rows[bad[0][0], 4 + bad[0][1]]}")
    assert_bits_equal(got[:, :4].copy().view(F32), rows[:, :4].copy().view(F32), what + ": vector offsets")
    check_meta(enc.metadata, meta, what)


def unaligned(torch, data, shift):
    """`data` on the device, `shift` floats behind a 16-byte boundary."""
    flat = torch.empty(data.size + shift, dtype=torch.float32, device="cuda")
    flat[shift:] = torch.from_numpy(np.ascontiguousarray(data).reshape(-1)).cuda()
    view = flat[shift:].view(*data.shape)
    assert view.data_ptr() % 16 == (4 * shift) % 16 != 0
    return view


def batches_of(data, sizes):
    """[data[0:s0], data[s0:s0+s1], ..., the rest]."""
    out, at = [], 0
    for s in sizes:
        out.append(data[at:at + s])
        at += s
    if at < data.shape[0]:
        out.append(data[at:])
    return [b for b in out if b.shape[0]]


# ------------------------------------------------------------------ 1. the quantize forms
@pytest.mark.parametrize("dim", S.all_q16_dims() + S.ROWS_DIMS)
def test_every_quantize_form_min_max_interval_and_specials(qo, dim):
    """encode over rows in [-1, 1] with NaN, both zeros and denormals among them (pass 1 and pass 2), then the same rows
    with +-inf and +-3.4e38 added under the interval just found (FAST with its specials at every form)."""
    for n in S.ROW_COUNTS:
        data = S.signed_data(n, dim)
        hard = S.with_hard_specials(data)
        for name, invert in S.metrics_of(dim, n):
            what = f"dim {dim}, {n} rows, {name} invert={invert}"
            vp = vp_of(dim, n, name, invert)
            rows, meta = qo.u8_encode(data, int(D[name]), invert)
            check_store(U8.encode(data, vp), rows, meta, what)
            rows, meta = qo.u8_encode_with(hard, int(D[name]), invert, meta.alpha, meta.offset)
            enc = U8.encode(hard, vp, alpha_offset=(meta.alpha, meta.offset))
            check_store(enc, rows, meta, what + ", infinite and huge values under a given interval")


@pytest.mark.parametrize("dim", S.all_q16_dims() + S.ROWS_DIMS)
def test_every_quantize_form_outside_the_fast_band(qo, dim):
    """alpha = 1e-25 and 1e25: quantize16_kernel<IT, false>, the exact division."""
    for alpha, offset in S.SLOW_PAIRS:
        for n in S.ROW_COUNTS:
            data = S.interval_data(n, dim, alpha, offset)
            for name, invert in S.metrics_of(dim, n):
                rows, meta = qo.u8_encode_with(data, int(D[name]), invert, alpha, offset)
                enc = U8.encode(data, vp_of(dim, n, name, invert), alpha_offset=(alpha, offset))
                check_store(enc, rows, meta, f"dim {dim}, {n} rows, {name} invert={invert}, alpha {alpha}")
                assert len(np.unique(rows[:, 4:4 + dim])) > min(100, n * dim // 4), "the rows use the code range"


@pytest.mark.parametrize("dim", S.padded_dims() + [S.ROWS_DIMS[-1]])
def test_code_boundaries_at_every_form(qo, dim):
    """The +-6 ulp sweep around every code boundary (test_gpu_u8.py runs it at dim 64) at a padded dim of every form:
    each row ends on boundary values, in the last real dword, next to the pad dword."""
    alpha, offset = S.BOUNDARY_PAIR
    data = S.boundary_data(dim, alpha, offset)
    n = data.shape[0]
    for name, invert in S.metrics_of(dim, 0):
        rows, meta = qo.u8_encode_with(data, int(D[name]), invert, alpha, offset)
        enc = U8.encode(data, vp_of(dim, n, name, invert), alpha_offset=(alpha, offset))
        check_store(enc, rows, meta, f"boundary rows, dim {dim}, {name} invert={invert}")


# ------------------------------------------------------------------ 2. row offsets
@pytest.mark.parametrize("dim", S.padded_dims() + [1101])
def test_row_offsets_streaming_and_upsert(qo, dim):
    """launch_quantize at row0 = 1, 3, 8, 75 (encode_stream) and 1, 2, 3, 6 (upsert): dst and offsets carry row0."""
    n = S.STREAM_ROWS
    data = S.signed_data(n, dim)
    for name, invert in S.metrics_of(dim, 0):
        what = f"dim {dim}, {name} invert={invert}"
        vp = vp_of(dim, n, name, invert)
        rows, meta = qo.u8_encode(data, int(D[name]), invert)
        enc = U8.encode_stream(lambda: iter(batches_of(data, S.STREAM_BATCHES)), vp)
        check_store(enc, rows, meta, what + ": encode_stream")
        enc = U8.encode_stream(lambda: iter(batches_of(data, S.STREAM_BATCHES)), vp, alpha_offset=(meta.alpha, meta.offset))
        check_store(enc, rows, meta, what + ": encode_stream under a given interval")
        want = rows.copy()
        for first in S.UPSERT_FIRST_ROWS:
            new = S.signed_data(first + 1, dim, seed=first)  # 2, 3, 4, 7 rows
            enc.upsert(first, new)
            want[first:first + new.shape[0]] = qo.u8_encode_with(new, int(D[name]), invert, meta.alpha, meta.offset)[0]
            assert np.array_equal(enc.storage_bytes(), want), what + f": upsert at row {first}"


# ------------------------------------------------------------------ 3. an unaligned device source
@pytest.mark.parametrize("dim", S.UNALIGNED_DIMS + [S.UNALIGNED_ODD_DIM])
def test_unaligned_device_source(qo, dim):
    """flat[1:] and flat[2:] of a device tensor: quantize_kernel (at dim % 4 == 0 too) and the grid-wide minmax_kernel."""
    torch = pytest.importorskip("torch")
    n = S.STREAM_ROWS
    data = S.signed_data(n, dim)
    new = S.signed_data(5, dim, seed=9)
    for shift in (1, 2):
        src = unaligned(torch, data, shift)
        mn, mx = U8.find_min_max(src)
        wmn, wmx = qo.find_min_max(data)
        assert same_bits(mn, wmn) and same_bits(mx, wmx), f"dim {dim}, shift {shift}: find_min_max ({mn}, {mx}), want ({wmn}, {wmx})"
        for name, invert in S.metrics_of(dim, 0)[shift - 1:shift + 1]:
            what = f"dim {dim}, shift {shift}, {name} invert={invert}"
            vp = vp_of(dim, n, name, invert)
            rows, meta = qo.u8_encode(data, int(D[name]), invert)
            enc = U8.encode(src, vp)
            check_store(enc, rows, meta, what + ": encode")
            assert np.array_equal(enc.storage_bytes(), U8.encode(torch.from_numpy(data).cuda(), vp).storage_bytes()), what + ": aligned run"
            pieces = batches_of(data, S.STREAM_BATCHES)  # each batch on its own unaligned buffer
            dev = [unaligned(torch, p, shift) for p in pieces]
            check_store(U8.encode_stream(lambda: iter(dev), vp), rows, meta, what + ": encode_stream")
            want = rows.copy()
            for first in S.UPSERT_FIRST_ROWS:
                enc.upsert(first, unaligned(torch, new, shift))
                want[first:first + 5] = qo.u8_encode_with(new, int(D[name]), invert, meta.alpha, meta.offset)[0]
                assert np.array_equal(enc.storage_bytes(), want), what + f": upsert at row {first}"


# ------------------------------------------------------------------ 4. the probe store of the query encoders
def probe_store(qo, dim, name, invert, alpha, offset):
    """A store that shows an encoded query through its scores: row j holds code 127 at byte j and nothing else, the
    last row nothing at all, every vector offset is +0.0.  The last row's score is the query offset's own bits (a -0.0
    offset reads +0.0), row j
    adds multiplier * 127 * code j (steps of 0.0079 at alpha 1 / 127: far above the rounding of the sum)."""
    ad = S.actual_dim(dim)
    rows = np.zeros((ad + 1, ad + 4), dtype=np.uint8)
    rows[np.arange(ad), 4 + np.arange(ad)] = 127
    _, meta = qo.u8_encode_with(np.zeros((1, dim), dtype=F32), int(D[name]), invert, alpha, offset)
    meta.count = ad + 1
    md = {"actual_dim": ad, "alpha": F32(meta.alpha), "offset": F32(meta.offset), "multiplier": F32(meta.multiplier),
          "vector_parameters": vp_of(dim, ad + 1, name, invert)}
    return U8.from_storage(rows, md), rows, meta


def check_queries(qo, torch, enc, rows, meta, queries, what, batches=S.QUERY_BATCHES):
    want = [qo.u8_encode_query(meta, q) for q in queries]
    for i, q in enumerate(queries[:4]):
        for src, where in ((q, "host"), (torch.from_numpy(q).cuda(), "device")):
            got = enc.encode_query(src)
            assert np.array_equal(got.encoded_query, want[i][0]), f"{what}: codes of query {i} from {where}"
            assert same_bits(got.offset, want[i][1]), f"{what}: offset of query {i} from {where}: {got.offset!r} want {want[i][1]!r}"
    scores = [qo.u8_score_all(meta, rows, c, o, order=qo.ORDER_SIMPLE) for c, o in want]
    for i, (c, o) in enumerate(want):
        assert scores[i][-1] == o and (o == 0 or same_bits(scores[i][-1], o)), "the empty row's score is the query offset (0 + -0.0 is +0.0)"
    for size in batches:
        for src, where in ((queries[:size], "host"), (torch.from_numpy(queries[:size]).cuda(), "device")):
            got = enc.score_batch(enc.encode_query_batch(src))
            for i in range(size):
                assert_bits_equal(got[i], scores[i], f"{what}: encode_query_batch of {size} from {where}, query {i}, seen through the probe store")


@pytest.mark.parametrize("dim", S.QUERY_DIMS)
def test_query_encoders_pad_and_sum(qo, dim):
    """encode_query_kernel and encode_queries_kernel: Dot under a negative offset (pad code 63) and L2."""
    torch = pytest.importorskip("torch")
    alpha, offset = S.BOUNDARY_PAIR
    rng = np.random.default_rng(dim)
    queries = (rng.random((max(S.QUERY_BATCHES), dim), dtype=F32) * F32(1.4) - F32(0.7)).astype(F32)  # past both ends of the interval
    queries[1, 0], queries[2, dim - 1], queries[3, dim // 2] = np.nan, np.inf, -np.inf
    queries[0, dim - 1] = F32(-0.0)
    for name, invert in (("Dot", False), ("L2", True), ("Dot", True), ("L2", False)):
        enc, rows, meta = probe_store(qo, dim, name, invert, alpha, offset)
        check_queries(qo, torch, enc, rows, meta, queries, f"dim {dim}, {name} invert={invert}")


# ------------------------------------------------------------------ 5. sum replay
@pytest.mark.parametrize("dim", S.REPLAY_DIMS)
def test_sum_of_squares_past_2_24_is_the_sequential_f32_sum(qo, dim):
    """quantize16_kernel<0> (1100), quantize_kernel (1101, 1102, and 1100 from an unaligned source) and both query
    encoders: from 2^24 on the vector offset takes the reference's sequential f32 sum, below it the integer."""
    torch = pytest.importorskip("torch")
    data = S.replay_data(6, dim)
    queries = S.replay_data(5, dim, seed=1)
    for invert in (False, True):
        what = f"dim {dim}, L2 invert={invert}"
        vp = vp_of(dim, 6, "L2", invert)
        rows, meta = qo.u8_encode(data, qo.L2, invert)
        check_store(U8.encode(data, vp), rows, meta, what + ": rows")
        check_store(U8.encode(unaligned(torch, data, 1), vp), rows, meta, what + ": rows from an unaligned source")
        enc, probe, pmeta = probe_store(qo, dim, "L2", invert, meta.alpha, meta.offset)
        check_queries(qo, torch, enc, probe, pmeta, queries, what + ": queries", batches=(1, 5))


# ------------------------------------------------------------------ 6. min / max with the extremes planted
def test_planted_extremes_at_every_lane_piece_component_tile_and_tail(qo):
    """Values in [1, 2] with ONE minimum and ONE maximum at chosen flat positions: a wrong DPP control, a missed
    readlane row, a lost float4 component, the NaN fill of the partial tile, the tail launch and two waves in one slot
    each lose exactly one of these."""
    torch = pytest.importorskip("torch")
    for name, n, aligned, lo_at, hi_at in S.planted_cases():
        data = S.planted_array(n, lo_at, hi_at)
        src = data.reshape(1, n) if aligned else unaligned(torch, data.reshape(1, n), 1)
        mn, mx = U8.find_min_max(src)
        wmn, wmx = qo.find_min_max(data)
        assert (wmn, wmx) == ((0.5, 3.0) if n > 1 else (0.5, 0.5))
        assert same_bits(mn, wmn) and same_bits(mx, wmx), f"{name}: ({mn}, {mx}), want ({wmn}, {wmx})"
    fmax = np.finfo(F32).max
    for n in (3, 5, 4096, 5300, 5303):
        for aligned in (True, False):
            shape = lambda a: a.reshape(1, n) if aligned else unaligned(torch, a.reshape(1, n), 1)
            nan = np.full(n, np.nan, dtype=F32)
            assert U8.find_min_max(shape(nan)) == (fmax, -fmax) == qo.find_min_max(nan), f"{n} NaNs, aligned={aligned}"
            for at in (0, n // 2, n - 1):  # all NaN but one value: it is both extremes
                one = nan.copy()
                one[at] = F32(-7.25)
                assert U8.find_min_max(shape(one)) == (-7.25, -7.25) == qo.find_min_max(one), f"{n} values, one at {at}, aligned={aligned}"
            inf = S.planted_array(n, 0, n - 1)
            inf[n - 1], inf[0], inf[n // 2] = np.inf, -np.inf, np.nan
            assert U8.find_min_max(shape(inf)) == (-np.inf, np.inf) == qo.find_min_max(inf), f"{n} values, infinite extremes, aligned={aligned}"


# ------------------------------------------------------------------ 7. the sign of a zero extreme
def zero_checks(qo, data, what):
    rows_n, dim = data.shape
    wmn, wmx = qo.find_min_max(data)
    mn, mx = U8.find_min_max(data)
    assert same_bits(mn, wmn) and same_bits(mx, wmx), f"{what}: find_min_max ({mn!r}, {mx!r}), want ({wmn!r}, {wmx!r})"
    for name in ("Dot", "L2"):
        vp = vp_of(dim, rows_n, name, False)
        rows, meta = qo.u8_encode(data, int(D[name]), False)
        for enc, how in ((U8.encode(data, vp), "encode"),
                         (U8.encode_stream(lambda: (data[i:i + 1] for i in range(rows_n)), vp), "encode_stream, a row per batch"),
                         (qa.ShardedVectorsU8.encode(data, vp, [0] * rows_n), "sharded encode, a row per shard")):
            md = enc.metadata
            assert same_bits(md["offset"], meta.offset), f"{what}, {name}: {how}: offset {md['offset']!r}, want {F32(meta.offset)!r}"
            assert same_bits(md["alpha"], meta.alpha) and same_bits(md["multiplier"], meta.multiplier), f"{what}, {name}: {how}"
            if how.startswith("encode"):
                check_store(enc, rows, meta, f"{what}, {name}: {how}")
                query = np.linspace(0.1, 0.9, dim, dtype=F32)
                codes, qoff = qo.u8_encode_query(meta, query)
                q = enc.encode_query(query)
                assert np.array_equal(q.encoded_query, codes) and same_bits(q.offset, qoff), f"{what}, {name}: {how}: query offset {q.offset!r}, want {qoff!r}"


@pytest.mark.parametrize("case", S.ZERO_CASES, ids=lambda c: c[0])
def test_zero_extreme_has_the_sign_of_the_first_zero(qo, case):
    """+0.0 and -0.0 compare equal, and the reference keeps the first value that wins `value < min`: the first zero in
    row order - within a wave (lane 1 holds the earlier zero, lane 0 the later one), across two waves that share a slot,
    across batches and across shards."""
    name, rows_n, dim, plus_at, minus_at, which = case
    zero_checks(qo, S.zero_array(rows_n, dim, plus_at, minus_at, which), name)


@pytest.mark.parametrize("first_negative", [False, True])
def test_all_zero_rows_of_mixed_signs(qo, first_negative):
    zero_checks(qo, S.mixed_zeros(3, 130, first_negative), f"all zeros, the first one {'-' if first_negative else '+'}0.0")


# ------------------------------------------------------------------ 8. the quantile interval
@pytest.mark.parametrize("count,dim", S.QUANTILE_SHAPES)
def test_quantile_interval_on_clustered_and_repeated_values(qo, count, dim):
    """select_kth_f32 over every row (count <= 100 000): values that share their top 24 bits under both signs, and
    70 000 copies of one value over the lower cut rank.  No zero is near either rank: the reference's unstable select
    leaves the sign of a zero there open."""
    torch = pytest.importorskip("torch")
    sets = [("clustered", None, S.clustered_data(count, dim))] + [("repeated", q, S.repeated_data(count, dim, q)) for q in S.QUANTILES]
    for kind, only, data in sets:
        for q in S.QUANTILES if only is None else (only,):
            want = qo.find_quantile_interval(data, q)
            assert want is not None
            for src, where in ((data, "host"), (torch.from_numpy(data).cuda(), "device")):
                got = U8.find_quantile_interval(src, q)
                assert got is not None and same_bits(got[0], want[0]) and same_bits(got[1], want[1]), \
                    f"{kind} {count} x {dim}, quantile {q}, {where}: {got}, want {want}"


@pytest.mark.parametrize("n,dim", S.SAMPLED_SHAPES)
def test_sampled_quantile_is_the_interval_of_the_strided_sample(qo, n, dim):
    """Above 100 000 rows the sample is row floor(k * n / 100 000), k = 0 .. 99 999: restated in numpy and pinned on
    the host gather, gather_strided_rows_kernel and gather_sample_batch_kernel (batches that cut the sample)."""
    torch = pytest.importorskip("torch")
    q = S.SAMPLED_QUANTILE
    data = np.random.default_rng(n + dim).standard_normal((n, dim)).astype(F32)
    want = qo.find_quantile_interval(data[S.sample_rows(n)], q)
    alpha, offset = qo.alpha_offset(*want)
    dev = torch.from_numpy(data).cuda()
    for src, where in ((data, "host gather"), (dev, "gather_strided_rows_kernel")):
        got = U8.find_quantile_interval(src, q)
        assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]), f"{n} x {dim}: {where}: {got}, want {want}"
    vp = vp_of(dim, n, "Dot", False)
    rows, meta = qo.u8_encode_with(data, qo.DOT, False, alpha, offset)
    cuts = range(0, n, S.SAMPLED_BATCH)
    for enc, how in ((U8.encode(data, vp, q), "encode from the host"), (U8.encode(dev, vp, q), "encode from the device"),
                     (U8.encode_stream(lambda: (data[a:a + S.SAMPLED_BATCH] for a in cuts), vp, q), "encode_stream, host batches"),
                     (U8.encode_stream(lambda: (dev[a:a + S.SAMPLED_BATCH] for a in cuts), vp, q), "encode_stream, device batches")):
        check_meta(enc.metadata, meta, f"{n} x {dim}: {how}")
        assert np.array_equal(enc.storage_bytes(), rows), f"{n} x {dim}: {how}: rows"
