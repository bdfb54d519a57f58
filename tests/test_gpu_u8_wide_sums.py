"""u8 pair sums of 2^24 and more, through every scoring entry point.

Past 2^24 the f32 score depends on the order of summation.  Lane mode 0 (the default) is the exact integer sum
rounded once (the reference's scalar path); lane mode 1 is impl_score_dot_avx's 8-lane f32 order (an AVX2 host),
for Dot and L2 -- L1 is the exact sum in both modes.  Every entry point must answer in the handle's mode: each is
checked bit for bit against the oracle (ORDER_SIMPLE in mode 0, ORDER_AVX2 in mode 1), and score_all, the anchor,
against the oracle directly.  For codes <= 127 the two orders are equal up to actual_dim 2080
(test_oracle_golden.py); the shapes below sit on both sides of that: 1056 and 2048 (the modes agree), 2096 (the
first actual_dim where they can differ, on constructed rows), 4096 and 32768 (random near-saturated rows), 32784
(past the matrix cores' integer pre-filter bound, mode 0).

Every mode-1 case asserts that the two orders really differ on the rows it checks, so an entry point that ignored the
mode could not pass.  The top-k cases carry planted rounding ties: two rows whose exact sums differ but round to the
same f32, the larger sum on the higher id -- the lower id must come first.
"""
import functools

import numpy as np
import pytest

from util import assert_bits_equal, bits, wide_dot_pair_2096

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
D = qa.DistanceType

N_SMALL = 2999          # ragged: not a multiple of any tile
BIG = {4096: 40_000, 32768: 33_000}  # topk_batch's pre-filtered matrix-core pass needs n >= 32768
TIE_OFF = np.float32(4e9)  # vector offset of the planted tie pairs: one pair on top, one at the bottom
KPPLIM_OFF = np.float32(3e9)  # |v_off / multiplier| > 2^29: pp_bound clamps to kPpLim


def _topk_want(scores, k, largest):
    n = scores.size
    order = np.lexsort((np.arange(n), -scores if largest else scores))[: min(k, n)]
    return order.astype(np.uint32), scores[order]


def _order(qo, mode):
    return qo.ORDER_AVX2 if mode == 1 else qo.ORDER_SIMPLE


def _meta(qo, ad, n, dist):
    mult = {D.Dot: 1.0, D.L2: -2.0, D.L1: -1.0}[dist]
    md = {"actual_dim": ad, "alpha": 1.0, "offset": 0.0, "multiplier": mult,
          "vector_parameters": qa.VectorParameters(ad, n, dist, False)}
    return md, qo.Meta(ad, 1.0, 0.0, mult, ad, n, int(dist), 0)


def _dot(a, b):
    return int(np.dot(a.astype(np.int64), b.astype(np.int64)))


def _plant_tie(qo, qcodes, codes, i):
    """Rows i and i + 1: all 127 but for a query byte j of code 1, where row i + 1 has 127 - e and row i 127 - e - d.
    Their exact sums S - d < S round to the same f32 in both orders.  Returns the two exact sums."""
    ad = qcodes.size
    L = qo.lib()

    def f(x):
        return (L.qo_dot_simple(qcodes.ctypes.data, x.ctypes.data, ad), L.qo_dot_avx2_order(qcodes.ctypes.data, x.ctypes.data, ad))

    for j in np.flatnonzero(qcodes == 1):
        for e in range(4):
            for d in range(1, 8):
                a, b = np.full(ad, 127, dtype=np.uint8), np.full(ad, 127, dtype=np.uint8)
                b[j] = 127 - e
                a[j] = 127 - e - d
                if f(a) == f(b):
                    codes[i], codes[i + 1] = a, b
                    return _dot(qcodes, a), _dot(qcodes, b)
    raise AssertionError("no rounding tie found")


def _query0(dim):
    """Query codes (alpha 1, offset 0: the f32 values ARE the codes).  At 2096 the constructed query; elsewhere
    near-saturated codes ([126, 127] below 2048: the planted ties need sums past 2^24).  Bytes 3, 5 and 77 are 1:
    room for the ties."""
    if dim == 2096:
        q = wide_dot_pair_2096()[0]
    else:
        q = np.random.default_rng(dim).integers(126 if dim < 2048 else 110, 128, size=dim, dtype=np.uint8)
        q[5] = q[77] = 1
    q[3] = 1
    return q


def _queries(dim, nq, seed):
    """Query 0 is _query0 (the planted ties are ties for it); the others vary it: a few odd-lane bytes set at 2096,
    fresh near-saturated codes elsewhere."""
    rng = np.random.default_rng(seed)
    q0 = _query0(dim)
    qs = np.repeat(q0[None], nq, axis=0)
    for r in range(1, nq):
        if dim == 2096:
            j = rng.choice(np.flatnonzero((np.arange(dim) % 4) >= 2), size=4, replace=False)
            qs[r, j] = rng.integers(1, 6, size=4)
        else:
            qs[r] = rng.integers(126 if dim < 2048 else 110, 128, size=dim, dtype=np.uint8)
    return qs


@functools.lru_cache(maxsize=None)
def _crafted_rows(dim, dist, n, kpplim=False):
    """Crafted rows for from_storage(): row 0 all 127, row 1 127 on the even lanes only, near-saturated random rows
    (at 2096: the constructed row and rows near it), and two planted tie pairs (offsets +-TIE_OFF)."""
    from oracle import qoracle as qo

    rng = np.random.default_rng(dim * 7 + int(dist))
    ad = dim
    even = (np.arange(ad) % 4) < 2
    rows = np.empty((n, ad + 4), dtype=np.uint8)
    codes = rows[:, 4:]
    if dim == 2096:
        codes[:] = rng.integers(0, 128, size=(n, ad), dtype=np.uint8)
        codes[:, even] = 127
        for r in range(n):  # the even-lane half sum just above 2^24: deficits of < 720 in all
            idx = rng.choice(np.flatnonzero(even), size=int(rng.integers(1, 12)), replace=False)
            codes[r, idx] -= rng.integers(0, 60, idx.size).astype(np.uint8)
        codes[2] = wide_dot_pair_2096()[1]
    else:
        lo = np.where(rng.random(n) < 0.5, 64, 110).astype(np.uint8)[:, None]
        for r0 in range(0, n, 2048):
            codes[r0:r0 + 2048] = rng.integers(lo[r0:r0 + 2048], 128, size=(min(2048, n - r0), ad), dtype=np.uint8)
    codes[0] = 127
    codes[1] = np.where(even, 127, 0)
    offs = (rng.standard_normal(n) * 100).astype(np.float32)
    if kpplim:
        big = rng.random(n) < 0.3
        offs[big] = np.where(rng.random(big.sum()) < 0.5, KPPLIM_OFF, -KPPLIM_OFF)
    ties = (n // 2, n - 3)
    sums = [_plant_tie(qo, _query0(dim), codes, t) for t in ties]
    offs[ties[0]] = offs[ties[0] + 1] = TIE_OFF
    offs[ties[1]] = offs[ties[1] + 1] = -TIE_OFF
    rows[:, :4] = offs.view(np.uint8).reshape(n, 4)
    md, meta = _meta(qo, ad, n, dist)
    return rows, md, meta, ties, sums


@functools.lru_cache(maxsize=None)
def _crafted(dim, dist, n, kpplim=False):
    rows, md, meta, ties, sums = _crafted_rows(dim, dist, n, kpplim)
    return qa.EncodedVectorsU8.from_storage(rows, md), rows, meta, ties, sums


@functools.lru_cache(maxsize=None)
def _oracle_scores(dim, dist, n, kpplim, qbytes, order):
    """The oracle's scores of a crafted store for one query (cached: query 0 recurs across batch sizes)."""
    from oracle import qoracle as qo

    rows, _, meta, _, _ = _crafted_rows(dim, dist, n, kpplim)
    c, qoff = qo.u8_encode_query(meta, np.frombuffer(qbytes, dtype=np.uint8).astype(np.float32))
    return qo.u8_score_all(meta, rows, c, qoff, order=order)


def _encode_query(qo, enc, meta, qcodes):
    q = enc.encode_query(qcodes.astype(np.float32))
    codes, qoff = qo.u8_encode_query(meta, qcodes.astype(np.float32))
    assert np.array_equal(q.encoded_query, codes)
    return q, codes, qoff


def _differ(qo, meta, rows, codes, qoff):
    """Rows where the two orders give different scores (lane mode 1 has teeth there)."""
    a = qo.u8_score_all(meta, rows, codes, qoff, order=qo.ORDER_AVX2)
    s = qo.u8_score_all(meta, rows, codes, qoff, order=qo.ORDER_SIMPLE)
    return bits(a) != bits(s)


def _guard(qo, meta, rows, codes, qoff, mode, dim, what):
    """The shape's edge: modes agree up to 2080, differ on >= 10 % of the rows past it.  Returns the differing rows."""
    diff = _differ(qo, meta, rows, codes, qoff)
    if dim <= 2080:
        assert not diff.any(), f"{what}: the orders differ at actual_dim {dim}"
    elif mode == 1 and meta.distance_type != qo.L1:
        assert diff.mean() >= 0.10, f"{what}: only {diff.sum()}/{diff.size} rows tell the orders apart"
    return np.flatnonzero(diff)


def _check_ties(qo, want, ties, sums, ids, largest, what):
    """The planted pairs: equal score bits, different exact sums; where the pair is in a top-k list, the lower id
    (smaller sum) comes first."""
    ids = list(ids)
    for t, (sa, sb) in zip(ties, sums):
        assert want[t].view(np.uint32) == want[t + 1].view(np.uint32) and sa < sb, f"{what}: planted tie at {t} is not a tie"
        if t in ids or t + 1 in ids:
            assert t in ids and (t + 1 not in ids or ids.index(t) < ids.index(t + 1)), f"{what}: tie at {t} broken by sum"


# ---------------------------------------------------------------------------------------------- shapes
SMALL = [(1056, (0, 1)), (2048, (0, 1)), (2096, (0, 1)), (4096, (0, 1)), (32768, (0, 1)), (32784, (0,))]
CASES = [pytest.param(dim, mode, dist, id=f"{dim}-mode{mode}-{dist.name}")
         for dim, modes in SMALL for mode in modes for dist in (D.Dot, D.L2)]


@pytest.mark.parametrize("dim,mode,dist", CASES)
def test_pairs_entry_points(qo, dim, mode, dist):
    """score_all (anchor), score_point, score_ids, score_internal, score_internal_ids and the two bursts."""
    enc, rows, meta, ties, _ = _crafted(dim, dist, N_SMALL, False)
    enc.set_lane_mode(mode)
    try:
        order = _order(qo, mode)
        n = N_SMALL
        tag = f"{dim} mode {mode} {dist.name}"
        qcodes = _queries(dim, 3, 1)
        q, codes, qoff = _encode_query(qo, enc, meta, qcodes[0])
        diff = _guard(qo, meta, rows, codes, qoff, mode, dim, tag)
        want = qo.u8_score_all(meta, rows, codes, qoff, order=order)
        assert_bits_equal(enc.score_all(q), want, tag + " score_all")

        pts = sorted({0, 1, 2, n - 1, ties[0], ties[0] + 1} | set(diff[:4].tolist()))
        for i in pts:
            assert_bits_equal([enc.score_point(q, i)], [want[i]], f"{tag} score_point {i}")
        ids = np.concatenate([np.arange(n)[::-1], [n - 1, 0, n - 1]]).astype(np.uint32)
        assert_bits_equal(enc.score_ids(q, ids), want[ids], tag + " score_ids")

        # score_internal: stored row i is the query; the teeth are the pairs where the orders differ
        rng = np.random.default_rng(dim + mode)
        rows_i = [0, 2, int(rng.integers(0, n))]
        for i in rows_i:
            want_i = np.array([qo.u8_score_internal(meta, rows, i, j, order) for j in range(n)], dtype=np.float32)
            if mode == 1 and dim > 2080:
                alt = np.array([qo.u8_score_internal(meta, rows, i, j, qo.ORDER_SIMPLE) for j in range(0, n, 7)],
                               dtype=np.float32)
                assert (bits(alt) != bits(want_i[::7])).mean() >= 0.10, f"{tag}: score_internal({i}, .) has no edge"
            for j in (0, 1, n - 1, int(rng.integers(0, n))):
                assert_bits_equal([enc.score_internal(i, j)], [want_i[j]], f"{tag} score_internal {i} {j}")
            assert_bits_equal(enc.score_internal_ids(i, np.arange(n, dtype=np.uint32)), want_i, f"{tag} score_internal_ids {i}")

        # bursts: lists of uneven length (one empty), queries of a batch / stored rows
        batch = enc.encode_query_batch(qcodes.astype(np.float32))
        offs = np.array([0, 0, 1500, n + 500], dtype=np.uint32)
        bids = np.concatenate([np.arange(n), rng.integers(0, n, 500)]).astype(np.uint32)
        got = enc.score_ids_batch(batch, offs, bids)
        for l in range(3):
            c, qo_l = qo.u8_encode_query(meta, qcodes[l].astype(np.float32))
            w = qo.u8_score_all(meta, rows, c, qo_l, order=order)
            sel = bids[offs[l]:offs[l + 1]]
            if sel.size and mode == 1 and dim > 2080:
                assert _differ(qo, meta, rows, c, qo_l)[sel].any(), f"{tag}: burst list {l} has no edge"
            assert_bits_equal(got[offs[l]:offs[l + 1]], w[sel], f"{tag} score_ids_batch list {l}")
        lrows = np.array([2, 0, n - 1], dtype=np.uint32)
        offs = np.array([0, 300, 300, 700], dtype=np.uint32)
        bids = rng.integers(0, n, 700).astype(np.uint32)
        got = enc.score_internal_ids_batch(lrows, offs, bids)
        w = np.array([qo.u8_score_internal(meta, rows, int(lrows[l]), int(j), order)
                      for l in range(3) for j in bids[offs[l]:offs[l + 1]]], dtype=np.float32)
        assert_bits_equal(got, w, tag + " score_internal_ids_batch")
        if mode == 1 and dim > 2080:
            w0 = np.array([qo.u8_score_internal(meta, rows, int(lrows[l]), int(j), qo.ORDER_SIMPLE)
                           for l in range(3) for j in bids[offs[l]:offs[l + 1]]], dtype=np.float32)
            assert (bits(w0) != bits(w)).any(), f"{tag}: score_internal_ids_batch has no edge"
    finally:
        enc.set_lane_mode(0)


@pytest.mark.parametrize("dim,mode,dist", CASES)
def test_topk(qo, dim, mode, dist):
    enc, rows, meta, ties, sums = _crafted(dim, dist, N_SMALL, False)
    enc.set_lane_mode(mode)
    try:
        tag = f"{dim} mode {mode} {dist.name}"
        q, codes, qoff = _encode_query(qo, enc, meta, _queries(dim, 1, 0)[0])
        diff = set(_guard(qo, meta, rows, codes, qoff, mode, dim, tag).tolist())
        want = qo.u8_score_all(meta, rows, codes, qoff, order=_order(qo, mode))
        seen = set()
        for k in (1, 30, 1024):
            for largest in (True, False):
                gi, gs = enc.topk(q, k, largest)
                wi, ws = _topk_want(want, k, largest)
                assert np.array_equal(gi, wi), f"{tag} topk k={k} largest={largest} ids"
                assert_bits_equal(gs, ws, f"{tag} topk k={k} largest={largest} scores")
                _check_ties(qo, want, ties, sums, gi, largest, f"{tag} topk k={k}")
                seen |= set(gi.tolist())
        # the tie pairs hold the extremes: top-1 is the lower id of one of them either way round
        assert {int(enc.topk(q, 1, True)[0][0]), int(enc.topk(q, 1, False)[0][0])} == set(ties)
        if mode == 1 and dim > 2080:
            assert seen & diff, f"{tag}: no returned row tells the orders apart"
    finally:
        enc.set_lane_mode(0)


@pytest.mark.parametrize("dim,mode,dist", CASES)
def test_score_batch(qo, dim, mode, dist):
    """nq 2, 3 (vector-ALU multi-query scan where it serves), 5, 64, 130 (matrix cores): every row equals that query's
    score_all, and the first and last query equal the oracle."""
    enc, rows, meta, _, _ = _crafted(dim, dist, N_SMALL, False)
    enc.set_lane_mode(mode)
    try:
        tag = f"{dim} mode {mode} {dist.name}"
        order = _order(qo, mode)
        for nq in (2, 3, 5, 64, 130):
            qcodes = _queries(dim, nq, nq)
            got = enc.score_batch(enc.encode_query_batch(qcodes.astype(np.float32)))
            for qi in range(nq):
                assert_bits_equal(got[qi], enc.score_all(enc.encode_query(qcodes[qi].astype(np.float32))),
                                  f"{tag} score_batch nq={nq} query {qi} vs score_all")
            for qi in (0, nq - 1):
                c, qoff = qo.u8_encode_query(meta, qcodes[qi].astype(np.float32))
                _guard(qo, meta, rows, c, qoff, mode, dim, f"{tag} nq={nq} query {qi}")
                assert_bits_equal(got[qi], qo.u8_score_all(meta, rows, c, qoff, order=order),
                                  f"{tag} score_batch nq={nq} query {qi}")
    finally:
        enc.set_lane_mode(0)


def _check_topk_batch(qo, enc, key, qcodes, mode, tag, oracle_queries=(0,)):
    """topk_batch (k 30 and 1024, both directions) against a stable sort of every query's score_all; score_all and
    the result of the oracle queries against the oracle itself (there the planted ties and the edge are checked)."""
    rows, _, meta, ties, sums = _crafted_rows(*key)
    dim, nq = key[0], qcodes.shape[0]
    order = _order(qo, mode)
    batch = enc.encode_query_batch(qcodes.astype(np.float32))
    oracle = {}
    for qi in oracle_queries:
        w = _oracle_scores(*key, qcodes[qi].tobytes(), order)
        other = _oracle_scores(*key, qcodes[qi].tobytes(), qo.ORDER_SIMPLE if mode == 1 else qo.ORDER_AVX2)
        diff = bits(w) != bits(other)
        if dim <= 2080:
            assert not diff.any()
        elif mode == 1:
            assert diff.mean() >= 0.10, f"{tag} query {qi}: only {diff.sum()} rows tell the orders apart"
        oracle[qi] = (w, set(np.flatnonzero(diff).tolist()))
    anchors = [enc.score_all(enc.encode_query(qcodes[qi].astype(np.float32))) for qi in range(nq)]
    for qi, (w, _) in oracle.items():
        assert_bits_equal(anchors[qi], w, f"{tag} score_all query {qi}")
    for k in (30, 1024):
        for largest in (True, False):
            gi, gs = enc.topk_batch(batch, k, largest)
            seen = set()
            for qi in range(nq):
                wi, ws = _topk_want(anchors[qi], k, largest)
                assert np.array_equal(gi[qi], wi), f"{tag} topk_batch k={k} largest={largest} query {qi} ids"
                assert_bits_equal(gs[qi], ws, f"{tag} topk_batch k={k} largest={largest} query {qi} scores")
                if qi in oracle:
                    seen |= set(gi[qi].tolist()) & oracle[qi][1]
                if qi == 0:  # the ties are planted for query 0
                    _check_ties(qo, oracle[qi][0], ties, sums, gi[qi], largest, f"{tag} topk_batch query {qi}")
            if mode == 1 and dim > 2080:
                assert seen, f"{tag} topk_batch k={k} largest={largest}: no checked row tells the orders apart"


@pytest.mark.parametrize("dim,mode,dist", CASES)
def test_topk_batch_small_store(qo, dim, mode, dist):
    enc = _crafted(dim, dist, N_SMALL, False)[0]
    enc.set_lane_mode(mode)
    try:
        for nq in (2, 5, 64, 300):
            _check_topk_batch(qo, enc, (dim, dist, N_SMALL, False), _queries(dim, nq, nq), mode,
                              f"{dim} mode {mode} {dist.name} nq={nq}", oracle_queries=(0, nq - 1))
    finally:
        enc.set_lane_mode(0)


@pytest.mark.parametrize("dim", sorted(BIG))
@pytest.mark.parametrize("mode", [0, 1])
def test_topk_batch_large_store(qo, dim, mode):
    """n >= 32768: the pre-filtered matrix-core pass (mode 0; at 32768 with vector offsets past the pre-filter's
    clamp) or the per-query lane-order scans (mode 1)."""
    key = (dim, D.Dot, BIG[dim], dim == 32768)
    enc = _crafted(*key)[0]
    enc.set_lane_mode(mode)
    try:
        for nq in (2, 5, 64, 300):
            _check_topk_batch(qo, enc, key, _queries(dim, nq, nq), mode, f"{dim} x {BIG[dim]} mode {mode} nq={nq}")
    finally:
        enc.set_lane_mode(0)


# ---------------------------------------------------------------------------------- encode() stores
@functools.lru_cache(maxsize=None)
def _encoded(dist, invert):
    """Real alpha / offset / multiplier: values in [0.75, 1] plus one 0, so the codes land in about [95, 127]."""
    from oracle import qoracle as qo

    dim, n = 4096, N_SMALL
    rng = np.random.default_rng(int(dist) * 2 + invert)
    data = (np.float32(0.75) + np.float32(0.25) * rng.random((n, dim), dtype=np.float32))
    data[n // 3, 17] = 0.0
    vp = qa.VectorParameters(dim, n, dist, invert)
    enc = qa.EncodedVectorsU8.encode(data, vp)
    rows, meta = qo.u8_encode(data, int(dist), invert)
    assert np.array_equal(enc.storage_bytes(), rows)
    assert rows[:, 4:].min() == 0 and np.percentile(rows[:, 4:], 1) >= 90
    queries = np.float32(0.75) + np.float32(0.25) * rng.random((64, dim), dtype=np.float32)
    return enc, rows, meta, queries


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("dist", [D.Dot, D.L2])
def test_encoded_store(qo, dist, invert, mode):
    enc, rows, meta, queries = _encoded(dist, invert)
    enc.set_lane_mode(mode)
    try:
        n, tag = N_SMALL, f"encoded {dist.name} invert={invert} mode {mode}"
        order = _order(qo, mode)
        q = enc.encode_query(queries[0])
        codes, qoff = qo.u8_encode_query(meta, queries[0])
        assert np.array_equal(q.encoded_query, codes)
        diff = _guard(qo, meta, rows, codes, qoff, mode, 4096, tag)
        want = qo.u8_score_all(meta, rows, codes, qoff, order=order)
        assert_bits_equal(enc.score_all(q), want, tag + " score_all")
        for i in sorted({0, n - 1} | set(diff[:3].tolist())):
            assert_bits_equal([enc.score_point(q, i)], [want[i]], f"{tag} score_point {i}")
        assert_bits_equal(enc.score_ids(q, np.arange(n, dtype=np.uint32)), want, tag + " score_ids")
        want_i = np.array([qo.u8_score_internal(meta, rows, 5, j, order) for j in range(n)], dtype=np.float32)
        assert_bits_equal(enc.score_internal_ids(5, np.arange(n, dtype=np.uint32)), want_i, tag + " score_internal_ids")
        assert_bits_equal([enc.score_internal(5, n - 1)], [want_i[n - 1]], tag + " score_internal")
        for k, largest in ((1, True), (30, False), (1024, True)):
            gi, gs = enc.topk(q, k, largest)
            wi, ws = _topk_want(want, k, largest)
            assert np.array_equal(gi, wi) and np.array_equal(bits(gs), bits(ws)), f"{tag} topk k={k}"
        for nq in (2, 5, 64):
            got = enc.score_batch(enc.encode_query_batch(queries[:nq]))
            for qi in (0, nq - 1):
                c, o = qo.u8_encode_query(meta, queries[qi])
                assert_bits_equal(got[qi], qo.u8_score_all(meta, rows, c, o, order=order), f"{tag} score_batch nq={nq} {qi}")
        gi, gs = enc.topk_batch(enc.encode_query_batch(queries[:5]), 30, True)
        for qi in (0, 4):
            c, o = qo.u8_encode_query(meta, queries[qi])
            wi, ws = _topk_want(qo.u8_score_all(meta, rows, c, o, order=order), 30, True)
            assert np.array_equal(gi[qi], wi) and np.array_equal(bits(gs[qi]), bits(ws)), f"{tag} topk_batch {qi}"
    finally:
        enc.set_lane_mode(0)


# ---------------------------------------------------------------------------------------------- L1, sharded
def test_l1_is_the_exact_sum_in_both_modes(qo):
    """L1 has no lane order: mode 1 == mode 0 == ORDER_SIMPLE at 8320, where the reference's AVX2 kernel wraps its
    u16 lanes (all-0 against all-127: 8064 instead of 1056640) -- a known divergence."""
    dim, n = 8320, 600
    rng = np.random.default_rng(8320)
    codes = rng.integers(0, 18, size=(n, dim), dtype=np.uint8)
    codes[0] = 127
    rows = np.zeros((n, dim + 4), dtype=np.uint8)
    rows[:, 4:] = codes
    md, meta = _meta(qo, dim, n, D.L1)
    enc = qa.EncodedVectorsU8.from_storage(rows, md)
    qz = np.zeros(dim, dtype=np.float32)
    qcodes = np.concatenate([np.zeros((1, dim)), rng.integers(110, 128, size=(4, dim))]).astype(np.float32)
    q, c, qoff = _encode_query(qo, enc, meta, qz)
    want = qo.u8_score_all(meta, rows, c, qoff, order=qo.ORDER_SIMPLE)
    assert want[0] == np.float32(-1056640.0)
    assert qo.u8_score_all(meta, rows, c, qoff, order=qo.ORDER_AVX2)[0] == np.float32(-8064.0)
    for mode in (0, 1):
        enc.set_lane_mode(mode)
        tag = f"L1 8320 mode {mode}"
        assert_bits_equal(enc.score_all(q), want, tag + " score_all")
        assert_bits_equal([enc.score_point(q, 0)], [want[0]], tag + " score_point")
        assert_bits_equal(enc.score_ids(q, np.arange(n, dtype=np.uint32)), want, tag + " score_ids")
        assert_bits_equal([enc.score_internal(0, 1)], [qo.u8_score_internal(meta, rows, 0, 1)], tag + " score_internal")
        gi, gs = enc.topk(q, 30, False)
        wi, ws = _topk_want(want, 30, False)
        assert np.array_equal(gi, wi) and np.array_equal(bits(gs), bits(ws)), tag + " topk"
        got = enc.score_batch(enc.encode_query_batch(qcodes))
        for qi in range(qcodes.shape[0]):
            c_i, o_i = qo.u8_encode_query(meta, qcodes[qi])
            assert_bits_equal(got[qi], qo.u8_score_all(meta, rows, c_i, o_i, order=qo.ORDER_SIMPLE), f"{tag} score_batch {qi}")
    enc.set_lane_mode(0)


def test_sharded_answers_in_mode_0(qo):
    """Sharded handles have no lane switch: at 4096 they give the exact sum rounded once."""
    dim = 4096
    enc, rows, meta, ties, sums = _crafted(dim, D.Dot, N_SMALL, False)
    md, _ = _meta(qo, dim, N_SMALL, D.Dot)
    sh = qa.ShardedVectorsU8.from_storage(rows, md, [0, 0, 0])
    qcodes = _queries(dim, 5, 3)
    q = sh.encode_query(qcodes[0].astype(np.float32))
    c, qoff = qo.u8_encode_query(meta, qcodes[0].astype(np.float32))
    assert _differ(qo, meta, rows, c, qoff).mean() >= 0.10
    want = qo.u8_score_all(meta, rows, c, qoff, order=qo.ORDER_SIMPLE)
    assert_bits_equal(sh.score_all(q), want, "sharded score_all")
    for k, largest in ((1, True), (30, False), (1024, True)):
        gi, gs = sh.topk(q, k, largest)
        wi, ws = _topk_want(want, k, largest)
        assert np.array_equal(gi, wi) and np.array_equal(bits(gs), bits(ws)), f"sharded topk k={k} largest={largest}"
        _check_ties(qo, want, ties, sums, gi, largest, "sharded topk")
    gi, gs = sh.topk_batch(sh.encode_query_batch(qcodes.astype(np.float32)), 30, True)
    for qi in range(5):
        c, qoff = qo.u8_encode_query(meta, qcodes[qi].astype(np.float32))
        wi, ws = _topk_want(qo.u8_score_all(meta, rows, c, qoff, order=qo.ORDER_SIMPLE), 30, True)
        assert np.array_equal(gi[qi], wi) and np.array_equal(bits(gs[qi]), bits(ws)), f"sharded topk_batch {qi}"
