"""The case lists of tests/pq_row_shapes.py reach every instantiation csrc/pq.hip can launch (no GPU).

pq_row_shapes.py restates alloc_store, plan_slices, launch_fast, scan_launch, the gate of pq_topk_small, the staged /
gathered choice of qamd_pq_score_ids_batch and the sequential scans; here every family is enumerated over m = 1 .. 1024
at the row counts the GPU file uses, and the set of forms found is compared with the set the case lists reach and with
the set that exists less the table of unreachable forms.  Every list is also pinned entry by entry (what each m launches),
so that removing an m from a list, or moving a rung of a ladder, fails one of the equalities below.  The last test is
about the inputs: on the oracle alone, a last chunk left out changes the score of at least 99 % of the rows of every
store the GPU file builds.
"""
import numpy as np
import pytest

import pq_row_shapes as M
from util import (DIST_IDS, PQ_ZERO_CODES, bits, pq_row_table, pq_seq_scores, pq_shape_queries, pq_shape_store)

ALL_M = range(1, 1025)
F, T = False, True


def fast(nvs, filt=F, simple=F):
    return ("pq_scan_fast_kernel", nvs, 4, filt, simple)


def skew(nv, r=1, filt=F, sliced=F, pad=0):
    return ("pq_scan_skew_kernel", nv, r, filt, sliced, F, pad)


def with_filter(launches):
    return [e[:3] + (T,) + e[4:] for e in launches]


def score_rows_of(m, skew_on=True):
    return M.scan_rows(M.scan_tile(m, 4096, skew_on))


ROWS_USED = sorted({M.SMALL_SCAN_ROWS, M.SMALL_TOPK_ROWS, M.LDS_SCAN_ROWS, M.LISTS_ROWS, M.FUSED_ROWS}
                   | {n for tile in (16, 32, 64) for n in M.scan_rows(tile)})


def test_row_strides_and_slices():
    """alloc_store and plan_slices: dword rows, 16-byte pieces, the planar image, the 128-byte pitch."""
    assert [M.ds_of(m) for m in (1, 4, 5, 12, 13, 15, 16, 17, 144, 145, 159, 160, 161, 192, 256, 257, 288, 512)] == \
           [4, 4, 8, 12, 16, 16, 16, 32, 144, 256, 256, 160, 256, 192, 256, 384, 288, 512]
    assert {m: M.plan_slices(m) for m in M.PLANAR_MS + (144, 176, 288, 512)} == {
        160: [(0, 128), (128, 32)], 192: [(0, 96), (96, 96)], 224: [(0, 128), (128, 96)],
        320: [(0, 128), (128, 128), (256, 64)], 144: [], 176: [], 288: [(0, 96), (96, 96), (192, 96)],
        512: [(0, 128), (128, 128), (256, 128), (384, 128)]}
    assert M.ds_of(160, M.PLANAR_MAX_ROWS) == 256 and M.ds_of(160, M.PLANAR_MAX_ROWS - 1) == 160
    # a row is on the pitch exactly when it has more than nine pieces and no planar image
    for m in ALL_M:
        ds = M.ds_of(m)
        assert ds >= m and ds % 4 == 0 and ds - m < (4 if m < 16 else 128 if ds % 128 == 0 and m > 144 else 16)
        assert (ds % 128 == 0 and ds != m and m > 144) == (m > 144 and m % 32 != 0)


def test_query_scan_lists_are_the_first_last_and_only_m_of_each_form():
    """Each list pinned entry by entry: what launch_fast starts for it, score form; the FILTER twins are the same."""
    n = 4096
    assert {m: M.launch_fast(m, n, F) for m in M.WHOLE_RING_MS} == {
        16: [skew(2, 2)], 32: [skew(2)], 48: [skew(6, 2)], 64: [skew(4)], 96: [skew(6)], 128: [skew(8)]}
    assert {key: M.skew_padded_ring(m, n) for key, m in M.PADDED_MS.items()} == {
        200: (32, 0), 416: (64, 16), 400: (64, 0), 616: (96, 16), 600: (96, 0), 816: (128, 16), 800: (128, 0)}
    assert {key: M.launch_fast(m, n, F) for key, m in M.PADDED_MS.items()} == {
        key: [skew(nv, pad=pad)] for key, (nv, pad) in M.PADDED_KEYS.items()}
    # every padded key there is, and no m outside 20 .. 124 is padded
    keys = {}
    for m in ALL_M:
        ring, pad = M.skew_padded_ring(m, n)
        if ring:
            keys.setdefault(ring // 16 * 100 + pad, []).append(m)
    assert set(keys) == set(M.PADDED_MS) == set(M.PADDED_KEYS) and all(M.PADDED_MS[k] in ms for k, ms in keys.items())
    assert min(min(v) for v in keys.values()) == 20 and max(max(v) for v in keys.values()) == 124
    assert {m: M.launch_fast(m, n, F) for m in M.PLANAR_MS} == {
        160: [skew(8, sliced=T), skew(2, sliced=T)], 192: [skew(6, sliced=T)] * 2,
        224: [skew(8, sliced=T), skew(6, sliced=T)], 320: [skew(8, sliced=T), skew(8, sliced=T), skew(4, sliced=T)]}
    assert M.FAST_FIRST_MS == (17, 33, 49, 65, 81, 97, 113, 129) and M.FAST_LAST_MS == (31, 47, 63, 79, 95, 111, 127, 143)
    for at, nvs in enumerate(range(2, 10)):
        first, last = M.FAST_FIRST_MS[at], M.FAST_LAST_MS[at]
        assert M.launch_fast(first, n, F) == M.launch_fast(last, n, F) == [fast(nvs)]
        assert first % 4 == 1 and first - 16 * (nvs - 1) == 1 and last % 4 == 3 and 16 * nvs - last == 1
        # the neighbours belong to other forms: the m below `first` fills nvs - 1 pieces, the m above `last` is a
        # multiple of 16 (a ring row of the skew kernel up to 128, the SIMPLE form at 144)
        assert M.launch_fast(first - 1, n, F) != [fast(nvs)] and M.launch_fast(last + 1, n, F) != [fast(nvs)]
    assert {m: M.launch_fast(m, n, F) for m in M.FAST_OTHER_MS} == {132: [fast(9)], 144: [fast(9, simple=T)]}
    assert M.skew_padded_ring(132, n) == (0, 0) and M.ds_of(132) == 144
    assert {m: M.launch_fast(m, n, F) for m in M.PITCH_MS} == {
        257: [fast(8), fast(8), fast(1)], 145: [fast(8), fast(2)], 161: [fast(8), fast(3)], 177: [fast(8), fast(4)],
        193: [fast(8), fast(5)], 209: [fast(8), fast(6)], 225: [fast(8), fast(7)], 241: [fast(8), fast(8)]}
    assert len(M.SCAN_MS) == len(set(M.SCAN_MS)) == 6 + 7 + 4 + 8 + 8 + 2 + 8
    for m in M.SCAN_MS:
        assert M.launch_fast(m, M.FUSED_ROWS, T) == with_filter(M.launch_fast(m, n, F)), m
        name, launches = M.scan_kernel_name(m, n)
        assert launches == len(M.launch_fast(m, n, F)) and name.startswith(M.launch_fast(m, n, F)[0][0])
    # with the skew kernel off (developer library): the SIMPLE forms NVS 1 .. 8
    assert {m: M.launch_fast(m, n, F, skew=False) for m in M.SIMPLE_MS} == {16 * v: [fast(v, simple=T)] for v in range(1, 9)}
    assert all(M.launch_fast(m, M.FUSED_ROWS, T, skew=False) == [fast(m // 16, T, T)] for m in M.SIMPLE_MS)


def test_query_scan_cases_reach_every_instantiation():
    """The forms launch_fast can start over m = 1 .. 1024 at the row counts used = the forms the lists reach = the
    forms that exist less the unreachable ones."""
    exists = M.existing()
    big = [n for n in ROWS_USED if n >= 4096]
    reachable = {filt: {e for m in ALL_M if m >= 16 for n in big for e in M.launch_fast(m, n, filt)} for filt in (F, T)}
    score = {e for m in M.SCAN_MS for n in score_rows_of(m) for e in M.launch_fast(m, n, F)}
    filt = {e for m in M.SCAN_MS for e in M.launch_fast(m, M.FUSED_ROWS, T)}
    assert score == reachable[F] and filt == reachable[T]
    both = exists["skew"] | exists["fast"]
    gone = set(M.UNREACHABLE["skew"]) | set(M.UNREACHABLE["fast"])
    assert gone <= both and score | filt == both - gone
    assert len(exists["skew"]) == 2 * (8 + 3 + 2) + (8 + 3) and len(exists["fast"]) == 36 and len(score) == len(filt) == 13 + 10
    # what the developer-library child adds: exactly the SIMPLE forms below NVS 9
    simple = {e for m in M.SIMPLE_MS for n in score_rows_of(m, False) for e in M.launch_fast(m, n, F, skew=False)}
    simple |= {e for m in M.SIMPLE_MS for e in M.launch_fast(m, M.FUSED_ROWS, T, skew=False)}
    assert simple == set(M.UNREACHABLE["fast"])
    assert all(not e[5] for e in score | filt if e[0] == "pq_scan_skew_kernel")  # no run / coalesced-store form at these row counts
    # a million rows of whole ring rows do take it (test_pq_skewed_scan_shapes)
    assert M.launch_fast(96, 1 << 20, F) == [("pq_scan_skew_kernel", 6, 1, F, F, T, 0)]


def test_fused_route_and_row_counts():
    assert M.fused_policy(M.FUSED_ROWS, M.FUSED_K) == (True, 2048, 32)
    for m in M.SCAN_MS:
        assert M.topk_route(m, M.FUSED_ROWS, M.FUSED_K) == ("fused", M.launch_fast(m, M.FUSED_ROWS, T))
    for m in M.SEQ_MS:
        assert M.topk_internal_route(m, M.FUSED_ROWS, M.FUSED_K) == ("fused", M.seq_launch(m, M.FUSED_ROWS, T))
    # score form: exactly 4096 rows, a last tile ragged by one row, one more workgroup of one row
    tiles = {m: M.scan_tile(m, 4096) for m in M.SCAN_MS}
    assert {t for t in tiles.values()} == {16, 32, 64} and {m for m, t in tiles.items() if t == 32} == {16, 48}
    assert all((t == 64) == (M.launch_fast(m, 4096, F)[0][0] == "pq_scan_fast_kernel") for m, t in tiles.items())
    for tile in (16, 32, 64):
        exact, ragged, more = M.scan_rows(tile)
        assert exact == 4096 and exact % tile == 0 and ragged % tile == tile - 1 and ragged > exact
        assert more % tile == 1 and -(-more // 1024) == -(-ragged // 1024) + 1 == 6
    assert M.scan_rows(64) == (4096, 4159, 5121)
    assert {M.seq_tile(m, 4096) for m in M.SEQ_MS} == {32, 64}
    assert {m for m in M.SEQ_MS if M.seq_tile(m, 4096) == 32} == {129, 144}


def test_small_store_scan_cases():
    """pq_scan_kernel<LUT_IN_LDS, VEC16>: every remainder of both VEC16 forms without LDS, both forms with it."""
    assert M.SMALL_SCAN_MS == tuple(range(1, 65)) + (159, 160, 512) and M.SMALL_SCAN_ROWS < 4096
    paths = {M.quad_path(m) for m in M.SMALL_SCAN_MS}
    assert paths == {M.quad_path(m) for m in ALL_M}
    assert {p for p in paths if not p[0]} == {(F, F, g, t) for g in range(4) for t in range(4) if (g, t) != (0, 0) and 4 * g + t <= 12}
    assert {p for p in paths if p[0]} == {(T, F, 3, t) for t in (1, 2, 3)} | {(T, T, g, t) for g in range(4) for t in range(4)}
    assert {m for m in M.SMALL_SCAN_MS if not M.quad_path(m)[0]} == set(range(1, 13))
    got = {e for m in M.SMALL_SCAN_MS for e in M.scan_launch(m, M.SMALL_SCAN_ROWS, M.SMALL_SCAN_ROWS)}
    assert got == {("pq_scan_kernel", F, F), ("pq_scan_kernel", F, T)}
    assert {m: M.scan_launch(m, M.LDS_SCAN_ROWS, M.LDS_SCAN_ROWS) for m in M.LDS_SCAN_MS} == {
        1: [("pq_scan_kernel", T, F)], 3: [("pq_scan_kernel", T, F)], 8: [("pq_scan_kernel", T, F)],
        12: [("pq_scan_kernel", T, F)], 13: [("pq_scan_kernel", T, T)], 15: [("pq_scan_kernel", T, T)]}
    assert M.IDS_SCAN_IDS >= 4096
    assert {m: M.scan_launch(m, M.IDS_SCAN_IDS, M.SMALL_SCAN_ROWS, ids=True) for m in M.IDS_SCAN_MS} == {
        159: [("pq_scan_kernel", T, T)], 160: [("pq_scan_kernel", F, T)]}
    got |= {e for m in M.LDS_SCAN_MS for e in M.scan_launch(m, M.LDS_SCAN_ROWS, M.LDS_SCAN_ROWS)}
    reachable = {e for m in ALL_M for n in ROWS_USED for ids in (F, T) for e in M.scan_launch(m, n, n, ids=ids)
                 if e[0] == "pq_scan_kernel"}
    assert got == reachable == M.existing()["scan"]
    assert M.scan_kernel_name(15, M.LDS_SCAN_ROWS) == M.scan_kernel_name(512, M.SMALL_SCAN_ROWS) == ("pq_scan_kernel", 1)


def test_single_launch_topk_cases():
    """pq_topk_small_kernel<VEC16>: three workgroups, the last one ragged; m = 129 leaves the single launch."""
    n = M.SMALL_TOPK_ROWS
    assert M.SMALL_TOPK_KS == (1, 64)  # the least and the most the single launch takes
    for k in M.SMALL_TOPK_KS:
        wgs, per = M.small_topk_plan(n, k, 16, 512)
        assert wgs == 3 and per % 16 == 0 and 0 < n - 2 * per < per and (n - 2 * per) % 16 == 1
    assert M.small_topk_plan(n, 65, 16, 512) is None
    assert {m: M.topk_route(m, n, 64) for m in M.SMALL_TOPK_MS} == {
        m: ("small", [("pq_topk_small_kernel", m >= 13)]) for m in (1, 3, 8, 12, 13, 17, 31, 128)}
    assert {M.quad_path(m)[1:] for m in M.SMALL_TOPK_MS} == {(F, 0, 1), (F, 0, 3), (F, 2, 0), (F, 3, 0), (F, 3, 1), (T, 0, 1),
                                                             (T, 3, 3), (T, 0, 0)}
    assert M.topk_route(M.NOT_SMALL_TOPK_M, n, 64) == ("classic", [("pq_scan_kernel", F, T)])
    assert M.topk_route(128, n, 65)[0] == "classic"
    reachable = {e for m in ALL_M for nn in ROWS_USED for k in M.SMALL_TOPK_KS for e in M.topk_route(m, nn, k)[1]
                 if e[0] == "pq_topk_small_kernel"}
    assert reachable == {e for m in M.SMALL_TOPK_MS for e in M.topk_route(m, n, 1)[1]} == M.existing()["small"]


def test_list_cases():
    """qamd_pq_score_ids_batch: the gathered kernel in both VEC16 forms, the staged one at the first and last m of
    NP = 1 .. 9; NP = 10 is unreachable."""
    lens = M.LONG_LIST_LENS
    assert lens == (3000, 0, 130, 127, 839, 1500, 1, 0, 700, 1024, 1024, 4000, 128, 5)
    pairs, lists = sum(lens), len(lens)
    assert pairs >= 4096 and pairs // lists >= 2 * M.LIST_STAGE_MIN
    assert {m: M.lists_launch(m, M.LISTS_ROWS, pairs, lists) for m in M.STAGED_FIRST_MS} == {
        m: [("pq_lists_staged_kernel", np_)] for m, np_ in zip((13, 15, 17, 33, 49, 65, 81, 97, 113, 129), (1, 1, 2, 3, 4, 5, 6, 7, 8, 9))}
    assert {m: M.lists_launch(m, M.LISTS_ROWS, pairs, lists) for m in M.STAGED_LAST_MS} == {
        16 * np_: [("pq_lists_staged_kernel", np_)] for np_ in range(1, 10)}
    assert M.lists_launch(12, M.LISTS_ROWS, pairs, lists) == [("pq_lists_kernel", F)]  # below the first m of NP = 1
    assert {m: M.lists_launch(m, M.LISTS_ROWS, pairs, lists) for m in M.NOT_STAGED_MS} == {
        150: [("pq_lists_kernel", T)], 160: [("pq_lists_kernel", T)]}
    assert (M.ds_of(150), M.ds_of(159), M.ds_of(160)) == (256, 256, 160) and 160 * 1024 > M.LDS_BUDGET >= 159 * 1024
    reachable = {e for m in ALL_M for e in M.lists_launch(m, M.LISTS_ROWS, pairs, lists) if e[0] == "pq_lists_staged_kernel"}
    got = {e for m in M.STAGED_FIRST_MS + M.STAGED_LAST_MS for e in M.lists_launch(m, M.LISTS_ROWS, pairs, lists)}
    assert got == reachable == M.existing()["staged"] - set(M.UNREACHABLE["staged"])
    assert set(M.UNREACHABLE["staged"]) == {("pq_lists_staged_kernel", 10)}
    # short lists: the gathered kernel over the remainders of test_small_store_scan_cases
    short = {e for m in M.SMALL_SCAN_MS for e in M.lists_launch(m, M.SMALL_SCAN_ROWS, 150, 4)}
    assert short == M.existing()["lists"]
    # the segment layout: lists ending inside, on and across the 1024-pair workgroup ranges, empty lists, segments of
    # 127 (gathered) and 128 (staged) pairs
    offs = np.concatenate([[0], np.cumsum(lens)])
    segs = []
    for p0 in range(0, pairs, M.LIST_STAGE_PAIRS):
        p1 = min(p0 + M.LIST_STAGE_PAIRS, pairs)
        cuts = sorted({p0, p1} | {int(o) for o in offs if p0 < o < p1})
        segs += [b - a for a, b in zip(cuts, cuts[1:])]
    assert 127 in segs and 128 in segs and 1024 in segs and 1 in segs and min(segs) >= 1
    assert any(o % 1024 == 0 for o in offs[1:-1]) and any(o % 1024 for o in offs[1:-1]) and lens.count(0) == 2
    assert any(a // 1024 != (b - 1) // 1024 for a, b in zip(offs, offs[1:]) if b > a)


def test_pair_cases():
    """pq_internal_pairs_kernel: one trip with idle lanes, an exact trip, a second trip of one lane, ten trips."""
    assert {m: M.pairs_path(m) for m in M.PAIR_MS} == {1: (1, 1), 15: (1, 15), 16: (1, 16), 17: (2, 1), 31: (2, 15),
                                                      32: (2, 16), 33: (3, 1), 150: (10, 6)}
    assert M.PAIR_CHUNKS == (1, 3, 8)
    assert [M.dim_chunk_of(33, c) for c in M.PAIR_CHUNKS] == [(33, 1), (98, 3), (263, 8)]


def test_internal_scan_cases():
    """pq_scan_seq_kernel<NVS, UNROLL, FILTER> at the first and last m of NVS 1 .. 9, the planar and the pitch slices;
    pq_scan_seq_rows_kernel<STAGE>."""
    def seq(nvs, filt=F):
        return ("pq_scan_seq_kernel", nvs, 2 if nvs == 9 else 4, filt)

    n = 4096
    assert M.SEQ_FIRST_MS == (16, 17, 33, 49, 65, 81, 97, 113, 129) and M.SEQ_LAST_MS == tuple(range(16, 145, 16))
    for nvs in range(1, 10):
        first, last = M.SEQ_FIRST_MS[nvs - 1], M.SEQ_LAST_MS[nvs - 1]
        assert M.seq_launch(first, n) == M.seq_launch(last, n) == [seq(nvs)]
        assert M.seq_launch(first - 1, n) != [seq(nvs)] and M.seq_launch(last + 1, n) != [seq(nvs)]
    assert {m: M.seq_launch(m, n) for m in M.SEQ_PLANAR_MS + M.SEQ_PITCH_MS} == {
        160: [seq(8), seq(2)], 192: [seq(6), seq(6)], 320: [seq(8), seq(8), seq(4)],
        257: [seq(8), seq(8), seq(1)], 145: [seq(8), seq(2)], 241: [seq(8), seq(8)]}
    assert {m: M.seq_slices(m, n) for m in (145, 241, 257, 160)} == {145: [128, 17], 241: [128, 113], 257: [128, 128, 1], 160: [128, 32]}
    score = {e for m in M.SEQ_MS for e in M.seq_launch(m, n)}
    filt = {e for m in M.SEQ_MS for e in M.seq_launch(m, M.FUSED_ROWS, T)}
    reach = {f: {e for m in ALL_M if m >= 16 for e in M.seq_launch(m, M.FUSED_ROWS, f)} for f in (F, T)}
    assert score == reach[F] and filt == reach[T] and score | filt == M.existing()["seq"]
    assert {m: M.seq_launch(m, M.LDS_SCAN_ROWS) for m in M.SEQ_ROWS_STAGED_MS} == {m: [("pq_scan_seq_rows_kernel", T)] for m in (1, 7, 15)}
    assert {m: M.seq_launch(m, M.SMALL_SCAN_ROWS) for m in M.SEQ_ROWS_MS} == {m: [("pq_scan_seq_rows_kernel", F)] for m in (3, 100, 200)}
    rows = {e for m in ALL_M for nn in ROWS_USED for e in M.seq_launch(m, nn) if e[0] == "pq_scan_seq_rows_kernel"}
    assert rows == M.existing()["seq_rows"]
    assert M.topk_internal_route(15, M.LDS_SCAN_ROWS, 64)[0] == "classic"


def test_unreachable_forms_are_exactly_what_the_enumeration_misses():
    """Over m = 1 .. 1024, the row counts used and both values of every switch the product library has, the forms found
    are the existing ones less the table - and every entry of the table carries its reason."""
    exists = M.existing()
    big = [n for n in ROWS_USED if n >= 4096]
    found = {e for m in ALL_M for n in ROWS_USED for ids in (F, T) for e in M.scan_launch(m, n, n, ids=ids)}
    found |= {e for m in ALL_M if m >= 16 for n in big for e in M.launch_fast(m, n, T)}
    found |= {e for m in ALL_M for n in ROWS_USED for k in (1, 64, 65) for e in M.topk_route(m, n, k)[1]}
    pairs, lists = sum(M.LONG_LIST_LENS), len(M.LONG_LIST_LENS)
    found |= {e for m in ALL_M for p, l in ((pairs, lists), (150, 4)) for e in M.lists_launch(m, M.LISTS_ROWS, p, l)}
    found |= {e for m in ALL_M for n in ROWS_USED for e in M.seq_launch(m, n)}
    found |= {e for m in ALL_M if m >= 16 for n in big for e in M.seq_launch(m, n, T)}
    everything = set().union(*exists.values())
    table = {e: why for fam in M.UNREACHABLE.values() for e, why in fam.items()}
    assert found == everything - set(table) and set(table) <= everything
    assert len(table) == 1 + 16 + 11 and all(len(why) > 20 for why in table.values())


def test_metrics_rotate_and_every_kernel_runs_all_six():
    assert len(M.METRICS) == 6
    for at in range(len(M.ALL_MS) - 5):
        assert {M.metric_of(m) for m in M.ALL_MS[at:at + 6]} == set(M.METRICS)
    # all six on one m per kernel: skew whole, padded, sliced; fast in one slice and on the pitch; ...
    n = 4096
    assert [M.launch_fast(m, n, F)[0][:1] + (M.launch_fast(m, n, F)[0][4],) for m in M.ALL_METRICS_MS["scan"][:3]] == [
        ("pq_scan_skew_kernel", F), ("pq_scan_skew_kernel", F), ("pq_scan_skew_kernel", T)]
    assert M.skew_padded_ring(104, n)[0] and not M.skew_padded_ring(96, n)[0]
    assert [len(M.launch_fast(m, n, F)) for m in M.ALL_METRICS_MS["scan"][3:]] == [1, 3]
    assert {M.quad_path(m)[0] for m in M.ALL_METRICS_MS["small_scan"]} == {T} and M.quad_path(12)[0] is F
    assert {M.quad_path(m)[0] for m in M.ALL_METRICS_MS["lds_scan"]} == {F, T} == {M.quad_path(m)[0] for m in M.ALL_METRICS_MS["small_topk"]}
    assert {M.seq_tile(m, n) for m in M.ALL_METRICS_MS["seq"]} == {32, 64}
    for family, ms, fam_ms in (("scan", M.SCAN_MS, None), ("small_scan", M.SMALL_SCAN_MS, None), ("seq", M.SEQ_MS, None)):
        assert set(M.ALL_METRICS_MS[family]) <= set(ms), family
        assert len({M.metric_of(m) for m in ms}) == 6
    assert M.metrics_of(96, "scan") == M.METRICS and M.metrics_of(97, "scan") == [M.metric_of(97)]


# ------------------------------------------------------------------ the inputs
def test_store_generator_plants_the_edge_codes():
    rows, cen, dim, chunk = pq_shape_store(33, 301)
    assert rows.shape == (301, 33) and cen.shape == (256, 131) and (dim, chunk) == (131, 4)
    assert not rows[0].any() and (rows[1] == 255).all() and (rows[2] == PQ_ZERO_CODES[0]).all()
    assert not cen[list(PQ_ZERO_CODES)].any() and np.abs(cen).max() < 0.5 and cen[0].any() and cen[255].any()
    last = rows[3:, -1]
    assert not np.isin(last, (0, 255) + PQ_ZERO_CODES).any() and np.bincount(last, minlength=256).max() <= 2
    assert np.array_equal(pq_shape_store(33, 100)[0], rows[:100])  # a smaller store is a prefix
    q = pq_shape_queries(dim, 3)
    assert q.shape == (3, dim) and (q[:, -1] >= 0.25).all() and np.abs(q).max() < 0.75 and len({bytes(x) for x in q}) == 3


def test_a_chunk_left_out_changes_nearly_every_score(qo):
    """On the oracle alone: for every store of the GPU file, the scores with the last chunk left out differ in their bits
    from the full ones on at least 99 % of the rows - so a kernel that reads one chunk too few cannot pass, and since the
    table entries in play are not zeros, neither can one that adds a table entry too many.  Query families with the
    metric the store is run with (pq_score_all, SSE order), stored-row families with pq_seq_scores, which is first
    checked against the oracle's pq_score_internal."""
    worst = 1.0
    for family, m, n, chunk in M.stores():
        rows, cen, dim, chunk = pq_shape_store(m, n, chunk)
        dist, inv = M.metric_of(m)
        if family == "query":
            lut = qo.pq_encode_query(pq_shape_queries(dim, 1)[0], chunk, cen, DIST_IDS[dist], inv)
            full = qo.pq_score_all(rows, lut, order=qo.ORDER_SSE)
            less = qo.pq_score_all(rows[:, :m - 1], lut[:(m - 1) * 256], order=qo.ORDER_SSE) if m > 1 else np.zeros(n, np.float32)
            same = float(np.mean(bits(full) == bits(less)))
            assert same <= 0.01, (family, m, n, same)
            worst = min(worst, 1.0 - same)
            continue
        for i in (0, n // 2, n - 1):
            table = pq_row_table(rows, cen, dim, chunk, dist, i)
            full = pq_seq_scores(rows, table, inv)
            for j in (0, 1, 2, i, n - 1):
                assert bits(full[j:j + 1])[0] == bits(qo.pq_score_internal(rows, dim, chunk, cen, DIST_IDS[dist], inv, i, j))[0], (m, i, j)
            same = float(np.mean(bits(full) == bits(pq_seq_scores(rows, table, inv, chunks=m - 1))))
            assert same <= 0.01, (family, m, n, i, same)
            worst = min(worst, 1.0 - same)
    assert worst >= 0.99
