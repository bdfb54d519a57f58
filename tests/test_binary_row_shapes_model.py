"""The case lists of tests/binary_row_shapes.py reach every instantiation csrc/bin.hip can launch (no GPU).

The dispatch ladders are restated in binary_row_shapes.py (scan_planes / launch_bin, launch_small / bin_small_plan /
small_topk_plan, multi_step and the batch loops, the three paths of bin_pairs_kernel); here the dim lists go through
get_quantized_vector_size_from_params and those restatements, and every set of reached forms is compared with the set
that exists.  Removing a dim from a list, or moving a rung of a ladder, fails one of the equalities below.
"""
import numpy as np
import pytest

import binary_row_shapes as M
from util import bin_query_codes, bin_query_of, bin_random_rows, scalar_xor

U8, U128 = 0, 1
LADDER = {name: (g, iters, unroll, first, last) for name, g, iters, unroll, first, last in M.SCAN_LADDER}


def test_dims_are_first_last_masked_and_exact_rc_of_every_shape():
    assert M.DIMS == sorted(set(M.DIMS)) and len(M.DIMS) == 28
    for name, dims in M.SHAPE_DIMS.items():
        for dim in dims:
            assert M.scan_shape(M.ds_of(dim))[0] == name, (name, dim)
    for name in M.S_SHAPES:
        g, iters, _, first, last = LADDER[name]
        rcs = [M.ds_of(d) // 16 for d in M.SHAPE_DIMS[name]]
        # the first rc, the last masked rc (S1 and S2 have none), the EXACT rc
        assert rcs == ([first, last] if first == last else [first, max(first, last - 1), last]), (name, rcs)
        assert last == g * iters
        assert M.SHAPE_DIMS[name][0] % 64 == 1, "the first dim of a shape leaves its last piece all but empty"
        assert M.SHAPE_DIMS[name][-1] == 128 * last
        # the neighbours of the shape's ends belong to other shapes
        assert first == 1 or M.scan_shape(16 * (first - 1))[0] != name
        assert M.scan_shape(16 * (last + 1))[0] != name
    assert [M.ds_of(d) for d in M.SHAPE_DIMS["W4"]] == [4, 4] and [M.ds_of(d) for d in M.SHAPE_DIMS["W8"]] == [8, 8]
    assert [M.ds_of(d) // 16 for d in M.SHAPE_DIMS["WL"]] == [65, 65] and M.ds_of(8320) == 1040
    assert [M.ds_of(d, U128) for d in M.U128_DIMS] == [16, 16]
    assert M.ds_of(1, U8) == 4 and M.ds_of(65, U8) == 16 and M.ds_of(129, U8) == 32


def test_score_form_reaches_every_scan_instantiation():
    """(a), and the FILTER form of (d): every (shape, EXACT | masked) that exists, at every plane count."""
    exists = set()
    for name, g, iters, unroll, first, last in M.SCAN_LADDER:
        for planes in M.PLANES:
            u = 8 if name == "S8" and planes > 1 else unroll
            exists.add((name, g, iters, u, True, planes))
            if first != last:  # S1 and S2 serve one rc each: no masked launch
                exists.add((name, g, iters, u, False, planes))
    assert len(exists) == 3 * (8 + 6)
    score = {M.scan_shape(M.ds_of(d), p) + (p,) for d in M.S_DIMS for p in M.PLANES}
    assert score == exists
    fused = {M.scan_shape(M.ds_of(d), p) + (p,) for d in M.FUSED_DIMS for p in M.PLANES}
    assert fused == exists
    classic = {M.scan_shape(M.ds_of(d))[:3] + (M.scan_shape(M.ds_of(d))[4],) for d in M.CLASSIC_DIMS}
    assert classic == {(n, g, it, n in ("S1", "S2")) for n, g, it, _, _, _ in M.SCAN_LADDER}
    assert {M.scan_shape(M.ds_of(d))[0] for d in M.DIMS} == set(M.SHAPE_DIMS)
    assert all(M.scan_shape(M.ds_of(d, U128))[:2] == ("S1", 1) for d in M.U128_DIMS)
    # the stores of one-sign scores: both forms of every shape whose lanes outnumber its unroll steps
    one_sign = {M.scan_shape(M.ds_of(d), p) + (p,) for d in M.ONE_SIGN_DIMS for p in M.PLANES}
    assert one_sign == {e for e in exists if e[3] < e[1]} and len(one_sign) == 3 * 4 * 2
    # the fused route is the one fused_policy takes at these rows and k, with pivot rank 32
    assert M.fused_policy(M.FUSED_ROWS, M.FUSED_K) == (True, 2048, 32)
    assert not M.fused_policy(M.small_rows(16), M.CLASSIC_K)[0]


def test_row_counts_cross_tile_wave_and_workgroup_ends():
    """(a): a lone row, a ragged single tile, a second wave, a second workgroup with a ragged tile."""
    most = 0
    for dim in M.DIMS:
        for planes in M.PLANES:
            ds = M.ds_of(dim)
            _, g, _, _, _ = M.scan_shape(ds, planes)
            tile = M.scan_tile(ds, planes)
            one, ragged, second_wave, second_wg = M.scan_rows(ds, planes)
            assert one == 1 and 0 < ragged < tile and ragged % (64 // g)      # one tile, its last row slots idle
            assert tile < second_wave <= 2 * tile                            # a second wave of one row
            most = max(most, second_wg)
            if M.shape_of_dim(dim) in M.S_SHAPES:  # nine waves (8 fill a 512-thread workgroup); the last tile: one
                assert -(-second_wg // tile) == 9 and second_wg % tile == 64 // g + 1  # unroll step and a row
            else:                                  # bin_words_kernel: 256 threads walk 16 rows per step
                assert second_wg > 2 * 16 and second_wg % 4
    assert most == 2113 == M.scan_rows(16)[3]
    assert M.scan_rows(M.ds_of(8192)) == (1, 7, 9, 69) and M.scan_rows(M.ds_of(1024), 4) == (1, 63, 65, 521)
    assert M.scan_rows(M.ds_of(1024)) == (1, 127, 129, 1033) and M.scan_rows(4) == (1, 3, 5, 37)
    # the store epilogue writes (u % G == G - 1 or the last u): with UNROLL > G a lane keeps several rows' scores
    assert {n for n, g, _, u, _, _ in M.SCAN_LADDER if u > g} == {"S1", "S2", "S4", "S8"}


def test_single_launch_cases_reach_every_small_instantiation():
    """(c): bin_topk_small_kernel<G, ITERS, EXACT, PLANES>, and a plan of three workgroups with a ragged last one."""
    exists = set()
    for name, g, iters, _, first, last in M.SCAN_LADDER:
        for planes in M.PLANES:
            if planes > 1 and name not in M.PLANE_SMALL_SHAPES:
                continue
            exists.add((name, g, iters, True, planes))
            if first != last:
                exists.add((name, g, iters, False, planes))
    got = set()
    for dim in M.S_DIMS:
        ds = M.ds_of(dim)
        n = M.small_rows(ds)
        tile, least = M.small_tile_least(ds)
        for planes in M.PLANES:
            shape = M.small_shape(ds, planes)
            assert (shape is None) == (planes > 1 and M.shape_of_dim(dim) not in M.PLANE_SMALL_SHAPES)
            if shape is None:
                assert all(M.small_plan(n, k, ds, planes) is None for k in M.SMALL_KS)
                continue
            got.add(shape + (planes,))
            for k in M.SMALL_KS:
                wgs, per = M.small_plan(n, k, ds, planes)
                assert wgs == 3 and per % tile == 0 and n > 2 * least
                last_rows = n - 2 * per
                assert 0 < last_rows < per and last_rows % tile, (dim, last_rows)   # ragged: a tile of one live row
        assert M.small_plan(n, M.CLASSIC_K, ds) is None                            # k = 65 leaves the single launch
    assert got == exists
    assert M.small_rows(16) == 16513 and M.small_tile_least(16) == (128, 8192)
    for dim in M.SHAPE_DIMS["W4"] + M.SHAPE_DIMS["W8"] + M.SHAPE_DIMS["WL"]:
        assert M.small_shape(M.ds_of(dim)) is None


def test_multi_query_cases_reach_every_multi_instantiation():
    """(e) and (f): bin_scan_multi_kernel<G, ITERS, UNROLL, NQ, EXACT, FILTER>."""
    shapes = [(8, 1, 8), (16, 1, 4), (16, 2, 2), (16, 4, 2)]
    exists = set()
    for g, iters, unroll in shapes:
        for nq in (8, 4, 2):
            if (g, iters) == (16, 4) and nq == 8:
                continue
            exists.add((g, iters, unroll, True, nq))
            if g == 16:  # <8, 1, 8> serves rc 8 alone: no masked launch
                exists.add((g, iters, unroll, False, nq))
    score = set()
    for dim in M.MULTI_DIMS:
        ds = M.ds_of(dim)
        steps = M.multi_steps(ds, M.MULTI_QUERIES)
        assert steps == ([8, 4, 2, 1] if ds // 16 <= 32 else [4, 4, 4, 2, 1]), dim
        assert not M.score_batch_on_mfma(ds, dim, M.MULTI_ROWS, M.MULTI_QUERIES)
        assert M.score_batch_on_mfma(ds, dim, M.MULTI_ROWS + 1, M.MULTI_QUERIES) == (ds // 16 <= 39)
        score |= {M.multi_shape(ds, nq) + (nq,) for nq in steps if nq > 1}
    assert score == exists
    filt = set()
    for dim, queries in M.MULTI_FILTER_CASES:
        ds = M.ds_of(dim)
        assert not M.topk_batch_on_mfma(ds, dim, M.FUSED_ROWS, queries, M.FUSED_K), (dim, queries)
        assert M.small_plan(M.FUSED_ROWS, M.FUSED_K, ds) is None
        steps = M.multi_steps(ds, queries)
        want = {11: [8, 2, 1] if ds // 16 <= 32 else [4, 4, 2, 1], 4: [4], 2: [2]}[queries]
        assert steps == want, (dim, queries)
        filt |= {M.multi_shape(ds, nq) + (nq,) for nq in steps if nq > 1}
    # the FILTER form: the 8-wide step on both masked shapes that have it, the 4- and 2-wide on ITERS = 4 in both forms,
    # and the 8-lane shape (rc 8; the matrix cores take its batches of 3 and of 5 and more)
    assert filt == {(16, 1, 4, False, 8), (16, 1, 4, False, 2), (16, 2, 2, False, 8), (16, 2, 2, False, 2),
                    (16, 4, 2, False, 4), (16, 4, 2, False, 2), (16, 4, 2, True, 4), (16, 4, 2, True, 2),
                    (8, 1, 8, True, 4), (8, 1, 8, True, 2)}
    assert M.topk_batch_on_mfma(128, 1024, M.FUSED_ROWS, 3, M.FUSED_K) and M.topk_batch_on_mfma(128, 1024, M.FUSED_ROWS, 5, M.FUSED_K)
    assert M.topk_batch_on_mfma(M.ds_of(1025), 1025, M.FUSED_ROWS, 12, M.FUSED_K)


def test_pair_cases_reach_every_path_and_trip_boundary():
    """(b): dword rows, the plane loop, one piece per lane, and the 4-in-flight loop at its trip boundaries."""
    paths = {d: M.pairs_path(M.ds_of(d)) for d in M.DIMS}
    assert {p[0] for p in paths.values()} == {"dword", "piece", "loop"}
    assert {d for d, p in paths.items() if p[0] == "dword"} == set(M.SHAPE_DIMS["W4"] + M.SHAPE_DIMS["W8"])
    assert {p[1] for p in paths.values() if p[0] == "piece"} == {1, 2, 3, 4, 5, 7, 8}
    assert {d: paths[d][1] for d in M.PAIR_TRIP_DIMS} == M.PAIR_TRIP_DIMS
    assert paths[1025] == ("loop", 9, 1, 9)     # a first trip with masked slots: lane 0 holds pieces 0 and 8
    assert paths[4096] == ("loop", 32, 1, 32)   # an exact trip
    assert paths[4097] == ("loop", 33, 2, 1)    # a second trip of one piece
    assert paths[8193] == ("loop", 65, 3, 1)    # three trips
    assert paths[8192] == ("loop", 64, 2, 32) and paths[2048] == ("loop", 16, 1, 16)
    for planes in (4, 8):
        got = {M.pairs_path(M.ds_of(d), planes) for d in M.DIMS}
        assert ("dword",) in got and {p[1] for p in got if p[0] == "planes"} >= {1, 8, 9, 33, 65}
    assert all(M.pairs_path(M.ds_of(d, U128)) == ("piece", 1) for d in M.U128_DIMS)


def test_metrics_rotate_and_every_shape_runs_all_six():
    assert len(M.METRICS) == 6 and len(M.ALL_METRICS_DIMS) == len(M.SHAPE_DIMS)
    assert {M.shape_of_dim(d) for d in M.ALL_METRICS_DIMS} == set(M.SHAPE_DIMS)
    for at in range(len(M.DIMS) - 5):
        assert {M.metric_of(d) for d in M.DIMS[at:at + 6]} == set(M.METRICS)
    assert all(M.metrics_of(d) == (M.METRICS if d in M.ALL_METRICS_DIMS else [M.metric_of(d)]) for d in M.DIMS)
    for dims in (M.MULTI_DIMS, M.FUSED_DIMS, [d for d, _ in M.MULTI_FILTER_CASES]):
        assert len({M.metric_of(d) for d in dims}) >= 3


@pytest.mark.parametrize("dim", [65, 387, 2049])
def test_oracle_takes_a_block_of_queries_and_the_rows_pad_with_zeros(dim):
    """scalar_xor with codes [queries, dim] is scalar_xor query by query; bin_random_rows leaves the pad bits zero and
    the others uniform enough to be a test (no all-zero or all-one column in 200 rows)."""
    rows = bin_random_rows(200, dim, dim)
    unpacked = np.unpackbits(rows, axis=1, bitorder="little")
    assert rows.shape[1] * 8 >= dim and not unpacked[:, dim:].any()
    assert np.all(unpacked[:, :dim].any(axis=0)) and not np.any(unpacked[:, :dim].all(axis=0))
    for bits in M.PLANES:
        codes = np.stack([bin_query_codes(bin_query_of(dim, s), bits) for s in range(3)])
        both = scalar_xor(rows, codes, dim, bits)
        assert both.shape == (3, 200)
        for s in range(3):
            assert np.array_equal(both[s], scalar_xor(rows, codes[s], dim, bits))
