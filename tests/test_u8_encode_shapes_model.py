"""The case lists of tests/u8_encode_shapes.py against the u8 encoder's dispatch, without a GPU.

The dispatch of launch_quantize and MinMaxAcc::feed (csrc/u8.hip) is restated in u8_encode_shapes.py; here it is
enumerated over dim = 1 .. 4096 x aligned x fast and the lists are held against it: every quantize16_kernel form at
its first, its last and a padded dim, both situations of quantize_kernel, every outcome of feed().  Each list has a
stated length and every role is asserted, so deleting any one case turns a test red.  The rest proves on the oracle
alone that the data shows what it is meant to show: a non-zero pad code under Dot, sums of squares past 2^24 whose
sequential f32 sum differs from the integer rounded once, no zero at a quantile's two ranks.
"""
import numpy as np
import pytest

import u8_encode_shapes as S

F32 = np.float32
ALPHAS = {True: [1.0 / 127.0, S.BOUNDARY_PAIR[0], 2.0 ** -60, 2.0 ** 60],
          False: [a for a, _ in S.SLOW_PAIRS] + [float(np.nextafter(F32(2.0 ** -60), F32(0))), float(np.nextafter(F32(2.0 ** 60), F32(np.inf)))]}


def test_fast_band():
    for fast, alphas in ALPHAS.items():
        assert all(S.fast_alpha(a) == fast for a in alphas)
    assert all(S.fast_alpha(a) for a, _ in [S.BOUNDARY_PAIR]) and not any(S.fast_alpha(a) for a, _ in S.SLOW_PAIRS)
    assert len(S.SLOW_PAIRS) == 2 and S.SLOW_PAIRS[0][0] < 2.0 ** -60 and S.SLOW_PAIRS[1][0] > 2.0 ** 60  # both ends of the band


def test_lists_reach_every_quantize16_form_at_its_first_last_and_a_padded_dim():
    routes = {(d, al): S.quantize_route(d, al, 1.0 / 127.0) for d in range(1, 4097) for al in (True, False)}
    forms = {r[1] for r in routes.values() if r[0] == "q16"}
    assert forms == set(S.Q16_FORMS) == set(S.Q16_DIMS) and len(S.Q16_FORMS) == 7
    by_form = {it: sorted(d for (d, al), r in routes.items() if al and r[:2] == ("q16", it)) for it in forms}
    for it in S.Q16_FORMS:
        roles = S.Q16_DIMS[it]
        assert set(roles) == ({"first", "last", "padded"} if it else {"first", "padded", "whole", "partial"}), it
        assert all(d % 4 == 0 for d in by_form[it])
        assert roles["first"] == by_form[it][0]
        dwords, f4, _batch = S.q16_geometry(roles["first"])
        assert dwords > f4 and dwords % 16 == 4, "the first dim: a short last piece, and pad dwords in it"
        if it:
            assert roles["last"] == by_form[it][-1] and roles["last"] == 64 * it
            dwords, f4, batch = S.q16_geometry(roles["last"])
            assert dwords == f4 == batch == 16 * it, "the last dim fills every lane of every piece"
        pad = roles["padded"]
        assert pad in by_form[it] and pad % 16 == 12 and S.q16_geometry(pad)[0] - S.q16_geometry(pad)[1] == 1
        assert pad not in (roles["first"], roles.get("last"))
    zero = S.Q16_DIMS[0]
    dwords, f4, batch = S.q16_geometry(zero["whole"])
    assert batch == 64 and dwords == f4 == 5 * batch, "whole batches only, no padding"
    dwords, f4, batch = S.q16_geometry(zero["partial"])
    assert dwords % batch == 20 and dwords - f4 == 1, "a last batch of one whole piece and four lanes of the next, the last one padding"
    dims = S.all_q16_dims()
    assert len(dims) == len(set(dims)) == 22
    # all fourteen forms: every dim runs under an alpha inside and two outside the FAST band
    want = {("q16", it, fast) for it in forms for fast in (True, False)}
    assert len(want) == 14
    got = {S.quantize_route(d, True, a) for d in dims for a in [1.0 / 127.0, S.BOUNDARY_PAIR[0]] + [a for a, _ in S.SLOW_PAIRS]}
    assert got == want
    assert {S.q16_iters(d) for d in S.padded_dims()} == forms and len(S.padded_dims()) == 7


def test_lists_reach_both_quantize_kernel_situations():
    assert len(S.ROWS_DIMS) == len(set(S.ROWS_DIMS)) == 9
    seen = set()
    for d in S.ROWS_DIMS:
        assert S.quantize_route(d, True, 1.0) == S.quantize_route(d, False, 1.0) == ("rows",)
        seen.add((d % 4, S.actual_dim(d) // 4 > 64))
    assert {m for m, _ in seen} == {1, 2, 3} and {(1, False), (2, False), (3, False), (1, True), (2, True), (3, True)} == seen
    assert sum(1 for d in S.ROWS_DIMS if S.actual_dim(d) // 4 <= 64) == 5, "1, 2, 3: one dword; 17, 65: two and twenty"
    assert len(S.UNALIGNED_DIMS) == 3
    assert [S.quantize_route(d, False, 1.0) for d in S.UNALIGNED_DIMS] == [("rows",)] * 3
    assert [S.quantize_route(d, True, 1.0)[1] for d in S.UNALIGNED_DIMS] == [2, 12, 0], "aligned, the same dims take three forms"
    assert [S.query_pad(d) for d in S.UNALIGNED_DIMS] == [0, 0, 4] and S.quantize_route(S.UNALIGNED_ODD_DIM, False, 1.0) == ("rows",)
    # the row counts: every residue mod 4 but 0 twice over, and more than one workgroup of 8 waves x 4 rows
    assert sorted(n % 4 for n in S.ROW_COUNTS) == [1, 1, 1, 2, 3, 3] and max(S.ROW_COUNTS) > 4 * 32 and len(S.ROW_COUNTS) == 6
    row0 = np.cumsum((0,) + S.STREAM_BATCHES)
    assert list(row0) == [0, 1, 3, 8, 75] and {int(r) % 4 for r in row0[1:]} == {0, 1, 3} and S.STREAM_ROWS - row0[-1] == 56
    assert {r % 4 for r in S.UPSERT_FIRST_ROWS} == {1, 2, 3} and len(S.UPSERT_FIRST_ROWS) == 4
    for dim in S.all_q16_dims() + S.ROWS_DIMS:
        for n in S.ROW_COUNTS:
            assert [m for m, _ in S.metrics_of(dim, n)] == ["Dot", "L2", "L1"]
        for i in range(3):
            assert {S.metrics_of(dim, n)[i][1] for n in S.ROW_COUNTS} == {False, True}


def decode(pos):
    f4, comp = divmod(pos, 4)
    wave, t = divmod(f4, S.TILE_F4)
    j, lane = divmod(t, 64)
    return wave, j, lane, comp


def test_planted_extremes_reach_every_lane_piece_component_and_route():
    cases = S.planted_cases()
    assert len(cases) == len({c[0] for c in cases}) == 64 + 64 + 4 + 12 + 4 + 3 + 3
    by = {c[0]: c for c in cases}
    for name, n, aligned, lo, hi in cases:
        assert 0 <= lo < n and 0 <= hi < n and (lo != hi or n == 1), name
    lanes = [by[f"lane{l}"] for l in range(64)]
    assert {decode(c[3])[2] for c in lanes} == set(range(64)) == {decode(c[4])[2] for c in lanes}
    assert {decode(c[3])[1] for c in lanes} == set(range(16)) and {decode(c[3])[3] for c in lanes} == set(range(4))
    assert all(decode(c[3])[0] == 0 and decode(c[4])[0] == 1 and S.minmax_route(c[1], True) ==
               dict(full=True, partial=False, tail=False, scalar=False, wrap=False) for c in lanes)
    pieces = [by[f"piece{j}.{c}"] for j in range(16) for c in range(4)]
    assert {decode(c[3])[1:] for c in pieces} == {(j, 37, c) for j in range(16) for c in range(4)}
    assert {decode(c[4])[1:] for c in pieces} == {(j, 38, c) for j in range(16) for c in range(4)}
    # the partial tile: its last valid float4, every component between the two cases
    a, b = by["partial_last_f4"], by["partial_last_f4_swapped"]
    assert S.minmax_route(a[1], True) == dict(full=True, partial=True, tail=False, scalar=False, wrap=False)
    assert {a[3], a[4], b[3], b[4]} == {a[1] - 4, a[1] - 3, a[1] - 2, a[1] - 1} and decode(a[1] - 1)[0] == 1
    # the float4 just before a tile boundary and the one behind it
    a, b = by["tile_boundary"], by["tile_boundary_swapped"]
    assert decode(a[3]) == (0, 15, 63, 3) and decode(a[4]) == (1, 0, 0, 0) and decode(b[4]) == (1, 15, 63, 2) and decode(b[3]) == (2, 0, 0, 0)
    # each of the 1..3 tail values, as the minimum and as the maximum
    for t in (1, 2, 3):
        for p in range(t):
            for kind, at in (("min", 3), ("max", 4)):
                c = by[f"tail{t}.{p}_{kind}"]
                n4 = c[1] // 4
                assert c[1] % 4 == t and c[at] == n4 * 4 + p and S.minmax_route(c[1], True)["tail"] and c[7 - at] < n4 * 4
    # two waves in one slot
    for w, other in ((64, 0), (65, 1)):
        for kind, at in (("min", 3), ("max", 4)):
            c = by[f"wave{w}_{kind}"]
            assert decode(c[at])[0] == w and decode(c[7 - at])[0] == other and w % S.SLOTS == other
            assert S.minmax_route(c[1], True) == dict(full=True, partial=True, tail=False, scalar=False, wrap=True)
            assert -(-(c[1] // 4) // S.TILE_F4) == 66
    # the scalar form
    scalar = [c for c in cases if c[0].startswith("scalar")]
    assert all(S.minmax_route(c[1], c[2]) == dict(full=False, partial=False, tail=False, scalar=True, wrap=False) for c in scalar)
    assert {(c[3], c[4]) for c in scalar} >= {(0, scalar[0][1] - 1), (scalar[0][1] - 1, 0)}
    assert [S.minmax_route(by[f"short{k}"][1], True)["scalar"] for k in (1, 2, 3)] == [True] * 3
    # every outcome of feed() is among them
    outcomes = {tuple(sorted(k for k, v in S.minmax_route(c[1], c[2]).items() if v)) for c in cases}
    assert outcomes == {("full",), ("full", "partial"), ("full", "partial", "tail"), ("full", "partial", "wrap"), ("scalar",)}
    assert S.minmax_route(5, True) == dict(full=False, partial=True, tail=True, scalar=False, wrap=False)  # the signed-zero rows below
    data = S.planted_array(12_000, 4095, 4096)
    assert data[4095] == data.min() == 0.5 and data[4096] == data.max() == 3 and (data == 0.5).sum() == (data == 3).sum() == 1


def test_signed_zero_cases_sit_where_the_folds_differ(qo):
    assert len(S.ZERO_CASES) == 8 and len({c[1:] for c in S.ZERO_CASES}) == 8
    seen = set()
    for name, rows, dim, plus_at, minus_at, which in S.ZERO_CASES:
        data = S.zero_array(rows, dim, plus_at, minus_at, which)
        flat = data.reshape(-1)
        assert (flat == 0).sum() == 2 and not np.signbit(flat[plus_at]) and np.signbit(flat[minus_at])
        assert plus_at // dim != minus_at // dim, "the two zeros lie in different rows: encode_stream feeds them in two batches"
        mn, mx = qo.find_min_max(data)
        first_negative = minus_at < plus_at
        got = mn if which == "min" else mx
        assert got == 0 and bool(np.signbit(got)) == first_negative, name
        assert (flat.min() == 0) if which == "min" else (flat.max() == 0)
        a, b = decode(min(plus_at, minus_at)), decode(max(plus_at, minus_at))
        if name.startswith("lane"):  # one wave: the later zero is lane 0's, the earlier one lane 1's
            assert a == (0, 0, 1, 0) and b == (0, 1, 0, 0) and S.minmax_route(rows * dim, True)["partial"]
        else:                        # two waves of one slot
            assert a == (0, 0, 0, 0) and b == (64, 0, 0, 0) and S.minmax_route(rows * dim, True)["wrap"]
        seen.add((name.split("_")[0], which, first_negative))
    assert len(seen) == 8
    for first_negative in (False, True):
        data = S.mixed_zeros(3, 130, first_negative)
        mn, mx = qo.find_min_max(data)
        assert not data.any() and 20 < np.signbit(data).sum() < 370
        assert bool(np.signbit(mn)) == bool(np.signbit(mx)) == first_negative


def test_padded_dot_rows_carry_a_nonzero_pad_code(qo):
    """The pad dwords of quantize16_kernel (and the pad bytes of quantize_kernel and of the query encoders) show only
    when the pad code is not 0: Dot with a negative minimum."""
    dims = [d for d in S.all_q16_dims() + S.ROWS_DIMS + [S.UNALIGNED_ODD_DIM] + S.UNALIGNED_DIMS if S.query_pad(d) and d >= 8]
    assert set(S.padded_dims()) <= set(dims) and {S.Q16_DIMS[it]["first"] for it in S.Q16_FORMS if it != 2} <= set(dims)
    for dim in dims:
        for n in (1, 5):
            data = S.signed_data(n, dim)
            rows, meta = qo.u8_encode(data, qo.DOT, False)
            pads = rows[:, 4 + dim:]
            assert meta.offset == -1 and pads.shape[1] == S.query_pad(dim) and pads.min() == pads.max() == 63, dim
            hard = S.with_hard_specials(data)
            assert np.isinf(hard).sum() >= 2 and (np.abs(hard) > 3e38).sum() >= 4 and np.isnan(data).any()
    a, o = S.BOUNDARY_PAIR
    rows, _ = qo.u8_encode_with(S.boundary_data(124, a, o), qo.DOT, False, a, o)
    assert rows[:, 4 + 124:].min() == rows[:, 4 + 124:].max() == 63
    for dim in S.QUERY_DIMS:
        if S.query_pad(dim):
            _, meta = qo.u8_encode_with(np.zeros((1, dim), dtype=F32), qo.DOT, False, a, o)
            codes, _ = qo.u8_encode_query(meta, np.zeros(dim, dtype=F32))
            assert codes[dim:].min() == codes[dim:].max() == 63
    assert [S.query_pad(d) for d in S.QUERY_DIMS] == [15, 1, 0, 15, 15, 12, 3] and len(S.QUERY_BATCHES) == 3


def test_boundary_rows_put_a_boundary_value_into_the_last_real_dword(qo):
    a, o = S.BOUNDARY_PAIR
    vals = S.boundary_values(a, o)
    assert vals.size == 133 * 13
    for dim in S.padded_dims():
        data = S.boundary_data(dim, a, o)
        ends = data[:, dim - 4:].reshape(-1)
        assert set(vals.view(np.uint32)) <= set(data.view(np.uint32).reshape(-1)), "every boundary value is in the rows"
        assert set(ends.view(np.uint32)) <= set(vals.view(np.uint32)), "every row ends on boundary values, next to its pad dword"
        # they are boundary values: neighbours of one row's end get different codes somewhere
        rows, _ = qo.u8_encode_with(data, qo.L2, False, a, o)
        assert len(np.unique(rows[:, 4 + dim - 4:4 + dim])) > 100


@pytest.mark.parametrize("dim", S.REPLAY_DIMS)
def test_replay_rows_pass_2_24_and_the_sequential_sum_differs(qo, dim):
    assert len(S.REPLAY_DIMS) == 3 and [S.quantize_route(d, True, 1 / 127)[0] for d in S.REPLAY_DIMS] == ["q16", "rows", "rows"]
    for seed, n in ((0, 6), (1, 5)):  # the rows, the queries
        data = S.replay_data(n, dim, seed)
        rows, meta = qo.u8_encode(data, qo.L2, False)
        assert meta.offset == 0 and F32(meta.alpha) == F32(1) / F32(127)
        codes = rows[:, 4:].astype(np.int64)
        s2 = (codes * codes).sum(axis=1)
        assert (s2[1::2] >= 1 << 24).all() and (s2[0::2] < 1 << 24).all(), s2
        differ = 0
        for r in range(1, n, 2):
            seq = S.seq_f32_sum_of_squares(codes[r])
            differ += int(seq.view(np.uint32) != F32(s2[r]).view(np.uint32))
            # and the oracle's vector offset is the sequential sum's
            want = F32(F32(F32(codes.shape[1]) * F32(0) * F32(0)) + F32(F32(seq * F32(meta.alpha)) * F32(meta.alpha)))
            assert rows[r, :4].view(F32)[0].view(np.uint32) == want.view(np.uint32)
        assert differ >= 1, "no row whose sequential f32 sum differs from the integer rounded once: the case proves nothing"


def test_quantile_data_has_no_zero_at_the_ranks_and_the_copies_straddle_the_cut(qo):
    assert len(S.QUANTILE_SHAPES) == 3 and {d for _, d in S.QUANTILE_SHAPES} == {1, 3, 8} and len(S.QUANTILES) == 3
    for count, dim in S.QUANTILE_SHAPES:
        assert count <= S.SAMPLE and 100_000 <= count * dim <= 120_000
        data = S.clustered_data(count, dim)
        assert len(np.unique(data.view(np.uint32) >> 8 & 0x7FFFFF)) == 1 and (data > 0).any() and (data < 0).any() and not (data == 0).any()
        for q in S.QUANTILES:
            rep = S.repeated_data(count, dim, q)
            assert (rep == 1.5).sum() == 70_000 and not (rep == 0).any()
            lo, hi = qo.find_quantile_interval(rep, q)
            assert lo == 1.5 and hi >= 1.5, "the lower rank falls into the copies"
            assert S.quantile_cut(count, dim, q) >= 1


def test_sampled_shapes_cut_batches_between_sample_rows():
    assert len(S.SAMPLED_SHAPES) == 4 and {n for n, _ in S.SAMPLED_SHAPES} == {100_003, 150_000} and {d for _, d in S.SAMPLED_SHAPES} == {4, 7}
    for n, dim in S.SAMPLED_SHAPES:
        rows = S.sample_rows(n)
        assert n > S.SAMPLE and rows.size == S.SAMPLE and rows[0] == 0 and rows[-1] < n and (np.diff(rows) >= 1).all()
        assert len(set(np.diff(rows))) == 2, "some rows are skipped, irregularly"
        assert n * dim * 4 <= 5_000_000
        cuts = np.arange(S.SAMPLED_BATCH, n, S.SAMPLED_BATCH)
        assert len(cuts) >= 3 and (n < 150_000 or not np.isin(cuts, rows).all()), "a batch begins on a row that is no sample row"
        assert all(0 < np.searchsorted(rows, c) < S.SAMPLE for c in cuts), "every batch holds sample rows"
