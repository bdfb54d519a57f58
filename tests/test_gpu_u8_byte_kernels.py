"""Every u8 kernel that reads the plain byte codes, on every row-length shape, against the oracle.

csrc/u8.hip compiles the byte-code kernels once per row length and picks the instantiation from rc = actual_dim / 16:
one, two, four or eight lanes per row for rc 1, 2, 3..4, 5..8 (G1, G2, G4, G8), sixteen lanes with ITERS = ceil(rc / 16)
= 1..8 pieces per lane for rc 9..128 (E1..E8), a run-time loop beyond.  A row that does not fill its shape takes the
non-EXACT form, which clamps the load address and zeroes the lanes past the row end.  The same switch drives
launch_scan, launch_small, launch_multi (E shapes, 2 / 4 / 8 queries per pass, multi_reduce.hpp) and the ITERS of
u8_score_pairs_kernel.  Since the Dot / L2 whole-store scan reads the packed image, these kernels serve L1 stores, short
rows, stores with a code above 127 ("foreign" rows: no image), every top-k of k <= 64 and every random-access call --
none of it on the benchmark's path.

Stores come from from_storage: uniform random codes 0..127, a distinct vector offset per row (the oracle's epilogue
adds it under every metric, L1 included), metadata as the oracle's encoder writes it.  Foreign Dot / L2 stores carry a
few codes of 128..255 in addition.  Each shape is run at its first rc (only lane sub == 0 is live in the last step), at
its last rc (the EXACT form) and at a dim that is no multiple of 16.  Every comparison is bit for bit with the oracle
in qo.ORDER_SIMPLE (the exact integer, rounded once); the library's own output is the reference only for the stores
above 2M rows, as stated there.  test_case_lists_reach_every_instantiation (no GPU) restates the dispatch and keeps
the lists below honest.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from util import assert_bits_equal, bits, oracle_meta, oracle_metas, qa_meta, store_rows, topk_want, u8_actual_dim

qa = pytest.importorskip("quantization_amd")
D = qa.DistanceType
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV_LIB = os.path.join(ROOT, "tools", "lib", "libquantization_amd_dev.so")

# ------------------------------------------------------------------ the case lists
# (first rc, last rc) of the twelve templated shapes, in launch_scan's order.  E1 begins at rc 9, behind G8: its first
# dims are 139 and 144 (16 * 1 - 5 and 16 are G1's).
G_SHAPES = [(1, 1), (2, 2), (3, 4), (5, 8)]
E_SHAPES = [(9, 16)] + [(16 * (it - 1) + 1, 16 * it) for it in range(2, 9)]


def _shape_dims(first, last):
    # a dim that is no multiple of 16, the first rc, the last rc
    return [16 * first - 5, 16 * first] + ([16 * last] if last != first else [])


G_DIMS = [d for first, last in G_SHAPES for d in _shape_dims(first, last)] + [112]  # 112: rc 7, inside G8
E_DIMS = [d for first, last in E_SHAPES for d in _shape_dims(first, last)]           # sixteen lanes per row
GENERIC_DIM = 2064                                                                    # rc 129: the run-time loop
DIMS = sorted(G_DIMS + E_DIMS + [GENERIC_DIM])
FUSED_QUERY_BYTES = 896  # a host query of up to this many code bytes rides in the top-k kernel's arguments

SCAN_ROWS = (1, 31, 33, 255, 257, 1025, 4099)  # the largest tile is 256 rows (G1), a workgroup eight waves
PAIR_ROWS = 4099
TOPK_ROWS = (1, 63, 65, 1025, 4099, 20_011)    # 20 011: even 16-byte rows span several workgroups of the one launch
SMALL_KS = (1, 30, 64)
LARGE_KS = (100, 1024)
MULTI_ROWS = (1, 17, 65, 257, 1025, 4099)
# batch sizes that walk u8_score_batch_scans' grouping: 8-wide passes with 5 and 7 live queries, 8 + 1, 8 + 3 riding a
# 4-wide pass; 4-wide with 3 live, 4 + 1; 2 + 1
MULTI_BATCHES = {1: (2, 3, 4, 5, 7, 8, 9, 11), 2: (2, 3, 4, 5, 7, 8, 9, 11), 3: (2, 3, 4, 5, 7, 8, 9, 11),
                 4: (2, 3, 4, 5), 5: (2, 3, 4, 5), 6: (2, 3, 4, 5), 7: (2, 3), 8: (2, 3)}
BIG_ROWS = 2_100_003  # the smallest ragged count above topk_batch's 2 097 152-row gate
# (kind, dim, queries): the FILTER form of u8_scan_multi_kernel at E2 (8-wide), E5 (4-wide, one slot repeated), E6, E7
FILTER_CASES = [("l1", 272, 5), ("l1", 1040, 3), ("l1", 1296, 4), ("l1", 1552, 2), ("foreign", 1040, 2)]
PROOF_ROWS = 257
PROOF_DIMS = [d for first, last in E_SHAPES for d in (16 * first, 16 * last)]

KINDS = ("l1", "foreign")
FOREIGN_METRICS = [(D.Dot, False), (D.L2, True), (D.L2, False), (D.Dot, True)]
_ROW_ORDER = {}
for _rows in (SCAN_ROWS, TOPK_ROWS, MULTI_ROWS):
    for _i, _n in enumerate(_rows):
        _ROW_ORDER.setdefault(_n, _i)


def metric_of(kind, dim, n):
    """L1 with `invert` alternating with the row count; Dot / L2 and `invert` rotating with the row count (and from
    one dim to the next, so that a count does not keep one metric over all dims)."""
    i = _ROW_ORDER.get(n, 0)
    if kind == "l1":
        return D.L1, bool(i % 2)
    return FOREIGN_METRICS[(i + DIMS.index(dim)) % len(FOREIGN_METRICS)]


# ------------------------------------------------------------------ the dispatch of csrc/u8.hip, restated
def row_chunks(dim):
    return u8_actual_dim(dim) // 16


def scan_shape(dim):
    """launch_scan / launch_small: dim -> (G, ITERS, exact); (16, 0, None) is the generic kernel."""
    rc = row_chunks(dim)
    if rc == 1:
        g, iters = 1, 1
    elif rc == 2:
        g, iters = 2, 1
    elif rc <= 4:
        g, iters = 4, 1
    elif rc <= 8:
        g, iters = 8, 1
    elif rc <= 128:
        g, iters = 16, (rc + 15) // 16
    else:
        return 16, 0, None
    return g, iters, rc == g * iters


def pairs_iters(dim):
    """launch_pairs: the ITERS of u8_score_pairs_kernel (0: any row length)."""
    iters = (row_chunks(dim) + 15) // 16
    return iters if iters <= 8 else 0


def multi_width(dim, l1):
    rc = row_chunks(dim)
    iters = (rc + 15) // 16
    if rc < 9 or iters > 8:
        return 0
    return 8 if l1 and iters <= 3 else 4 if iters <= 6 else 2


def multi_passes(dim, l1, queries):
    """u8_score_batch_scans' grouping and launch_multi's choice: [(NQ of the pass, live queries)]; NQ 1 is a
    single-query scan."""
    iters, width, out, q = (row_chunks(dim) + 15) // 16, multi_width(dim, l1), [], 0
    while q < queries:
        live = min(width, queries - q)
        if live < 2:
            out.append((1, 1))
            q += 1
            continue
        if l1 and iters <= 3 and live > 4:
            nq = 8
        elif live > 2:
            nq = 4 if iters <= 6 else 2
        else:
            nq = 2
        out.append((nq, live))
        q += live
    return out


# ------------------------------------------------------------------ stores and what the oracle says of them
class Store:
    def __init__(self, qo, kind, dim, n):
        self.kind, self.dim, self.n = kind, dim, n
        self.dist, self.invert = metric_of(kind, dim, n)
        self.rows, self.query = store_rows(dim, n, seed=1 + KINDS.index(kind))
        if kind == "foreign":
            add_high_codes(self.rows, dim * 977 + n)
        self.md, self.meta = oracle_metas(qo, dim, n, self.dist, self.invert)
        self.codes, self.qoff = qo.u8_encode_query(self.meta, self.query)
        self.want = qo.u8_score_all(self.meta, self.rows, self.codes, self.qoff, order=qo.ORDER_SIMPLE)
        self.what = f"{kind} dim {dim}, {n} rows, {self.dist.name} invert={self.invert}"

    def open(self):
        return qa.EncodedVectorsU8.from_storage(self.rows, self.md)

    def scores(self, qo, query):
        codes, qoff = qo.u8_encode_query(self.meta, query)
        return qo.u8_score_all(self.meta, self.rows, codes, qoff, order=qo.ORDER_SIMPLE)

    def internal(self, qo, i, ids):
        return np.array([qo.u8_score_internal(self.meta, self.rows, int(i), int(j), order=qo.ORDER_SIMPLE) for j in ids],
                        dtype=np.float32)


def add_high_codes(rows, seed):
    """Codes of 128..255 in the last chunk of the last row, in chunk 0 of row 0 and at a handful of random places:
    the store gets no packed image, and bit 7 goes through dot16."""
    rng = np.random.default_rng(seed)
    n, ad = rows.shape[0], rows.shape[1] - 4
    high = lambda: rng.integers(128, 256, dtype=np.uint8)
    rows[n - 1, 4 + ad - 1 - int(rng.integers(0, 8))] = high()
    rows[0, 4 + int(rng.integers(0, 8))] = high()
    for _ in range(5):
        rows[int(rng.integers(0, n)), 4 + int(rng.integers(0, ad))] = high()


_STORES = {}


def get_store(qo, kind, dim, n):
    """The store (kind, dim, n) with the oracle's scores of its query, computed once for the tests that follow each
    other on it; the few last ones are kept."""
    key = (kind, dim, n)
    if key not in _STORES:
        while len(_STORES) >= 16:
            _STORES.pop(next(iter(_STORES)))
        _STORES[key] = Store(qo, kind, dim, n)
    return _STORES[key]


def check_topk(enc, q, want, k, largest, what):
    ids, sc = enc.topk(q, k, largest)
    wi, ws = topk_want(want, k, largest)
    what = f"{what}: topk {k} largest={largest}"
    assert np.array_equal(ids, wi), f"{what}: ids differ, first at {int(np.flatnonzero(ids != wi)[0])}"
    assert_bits_equal(sc, ws, what + " scores")


# ------------------------------------------------------------------ 0. the lists reach every instantiation (no GPU)
def test_case_lists_reach_every_instantiation(qo):
    assert len(DIMS) == len(set(DIMS)) == 36
    # launch_scan, launch_small (score, FILTER and single-launch forms share DIMS).  G1 and G2 serve one rc each, so
    # they have no non-EXACT launch; every other shape has both forms.
    shapes = [(1, 1), (2, 1), (4, 1), (8, 1)] + [(16, it) for it in range(1, 9)]
    want = {(g, it, True) for g, it in shapes} | {(g, it, False) for g, it in shapes if g > 2} | {(16, 0, None)}
    assert {scan_shape(d) for d in DIMS} == want
    # the first rc of every shape (one live lane in the last step) and a dim that pads its last chunk
    for first, last in G_SHAPES + E_SHAPES:
        assert 16 * first in DIMS and 16 * last in DIMS and 16 * first - 5 in DIMS
        assert scan_shape(16 * first)[:2] == scan_shape(16 * last)[:2] == scan_shape(16 * first - 5)[:2]
        assert first == 1 or scan_shape(16 * (first - 1))[:2] != scan_shape(16 * first)[:2]
        assert scan_shape(16 * last + 16)[:2] != scan_shape(16 * last)[:2]
    # the single-launch top-k that quantises a host query itself: every form a row of up to 896 bytes can take
    fused = {scan_shape(d) for d in DIMS if u8_actual_dim(d) <= FUSED_QUERY_BYTES}
    assert fused == {s for s in want if s[2] is not None and (s[0] < 16 or s[1] <= 3 or s == (16, 4, False))}
    # u8_score_pairs_kernel
    assert {pairs_iters(d) for d in DIMS} == set(range(9))
    # launch_multi, score form: L1 stores walk MULTI_BATCHES, foreign Dot / L2 stores take two queries
    can = {(it, nq) for it in range(1, 9) for nq in (2, 4, 8) if nq <= (8 if it <= 3 else 4 if it <= 6 else 2)}
    ran, live_seen, two = set(), set(), set()
    for dim in E_DIMS:
        _, it, exact = scan_shape(dim)
        assert multi_width(dim, True) == max(nq for i, nq in can if i == it)
        for queries in MULTI_BATCHES[it]:
            for nq, live in multi_passes(dim, True, queries):
                ran.add((it, nq, exact))
                live_seen.add((it, nq, live))
        assert multi_passes(dim, False, 2) == [(2, 2)]
        two.add((it, exact))
    assert ran == {(it, nq, ex) for it, nq in can for ex in (True, False)} | {(it, 1, ex) for it in range(1, 9) for ex in (True, False)}
    assert two == {(it, ex) for it in range(1, 9) for ex in (True, False)}
    for it in (1, 2, 3):  # 8-wide passes with 5 and 7 live queries; 8 + 3 leaves a 4-wide pass with 3
        assert {(it, 8, 5), (it, 8, 7), (it, 8, 8), (it, 4, 3), (it, 4, 4), (it, 2, 2)} <= live_seen
    for it in (4, 5, 6):
        assert {(it, 4, 3), (it, 4, 4), (it, 2, 2), (it, 1, 1)} <= live_seen
    assert all(d not in E_DIMS or multi_width(d, True) for d in DIMS) and not any(multi_width(d, True) for d in G_DIMS)
    # launch_multi, FILTER form: the four shapes no other test reaches
    got = [(scan_shape(dim)[1], multi_passes(dim, kind == "l1", queries)) for kind, dim, queries in FILTER_CASES]
    assert got == [(2, [(8, 5)]), (5, [(4, 3)]), (6, [(4, 4)]), (7, [(2, 2)]), (5, [(2, 2)])]
    assert BIG_ROWS > 2 << 20 and BIG_ROWS % 256
    # the metadata the stores are opened with is the reference encoder's own
    for dist in (D.Dot, D.L2):
        md, meta = oracle_metas(qo, 43, 7, dist, False)
        mine, ref = qa_meta(43, 7, dist), oracle_meta(qo, 43, 7, dist)
        assert all(md[k] == mine[k] for k in mine), (md, mine)
        assert all(getattr(meta, f) == getattr(ref, f) for f, _ in qo.Meta._fields_)
    for dist in D:
        for invert in (False, True):
            md, meta = oracle_metas(qo, 43, 7, dist, invert)
            assert md["multiplier"] == -oracle_metas(qo, 43, 7, dist, not invert)[0]["multiplier"] != 0
            assert (meta.actual_dim, meta.dim, meta.count, meta.distance_type, meta.invert) == (48, 43, 7, int(dist), int(invert))
    # the rotation gives every foreign metric and both L1 signs to every list of row counts
    assert [metric_of("l1", 768, n)[1] for n in SCAN_ROWS] == [False, True, False, True, False, True, False]
    for rows in (SCAN_ROWS, TOPK_ROWS, MULTI_ROWS):
        assert {metric_of("l1", 768, n) for n in rows} == {(D.L1, False), (D.L1, True)}
        for n in rows:  # a row count meets every foreign metric within any four neighbouring dims
            for at in range(len(E_DIMS) - 3):
                assert {metric_of("foreign", d, n) for d in E_DIMS[at:at + 4]} == set(FOREIGN_METRICS)
    assert len({metric_of("foreign", 768, n) for n in SCAN_ROWS}) == 4
    # foreign rows do carry codes above 127, in the first chunk of row 0 and the last chunk of the last row
    rows, _ = store_rows(267, 33)
    add_high_codes(rows, 5)
    assert rows[0, 4:20].max() > 127 and rows[32, -16:].max() > 127 and 2 <= int((rows[:, 4:] > 127).sum()) <= 7


# ------------------------------------------------------------------ 1. whole-store scan, score form
@pytest.mark.gpu
@pytest.mark.parametrize("dim", DIMS)
def test_whole_store_scan_on_every_shape(qo, dim):
    """u8_scan_kernel<G, ITERS, .., EXACT, false> (u8_scan_generic_kernel at rc 129), L1 and Dot / L2, at row counts
    that cross wave, tile and workgroup ends; score_point of the last row is u8_score_pairs_kernel."""
    for kind in KINDS:
        for n in SCAN_ROWS:
            st = get_store(qo, kind, dim, n)
            enc = st.open()
            q = enc.encode_query(st.query)
            assert_bits_equal(enc.score_all(q), st.want, st.what + ": score_all")
            assert_bits_equal(enc.score_point(q, n - 1), st.want[n - 1], st.what + ": score_point of the last row")


# ------------------------------------------------------------------ 2. pairs kernel
@pytest.mark.gpu
@pytest.mark.parametrize("dim", DIMS)
def test_pairs_kernel_on_every_row_length(qo, dim):
    """u8_score_pairs_kernel<IS_L1, ITERS> behind every random-access entry point."""
    torch = pytest.importorskip("torch")
    n = PAIR_ROWS
    for kind in KINDS:
        st = get_store(qo, kind, dim, n)
        enc = st.open()
        rng = np.random.default_rng(dim)
        ids = np.concatenate([[0, n - 1, 7, 7, n - 1, 0], rng.integers(0, n, 200)]).astype(np.uint32)
        q = enc.encode_query(st.query)
        assert_bits_equal(enc.score_ids(q, ids), st.want[ids], st.what + ": score_ids, host ids")
        dev_ids = torch.from_numpy(ids.astype(np.int32)).cuda()
        assert_bits_equal(enc.score_ids(q, dev_ids), st.want[ids], st.what + ": score_ids, device ids")
        for i, j in ((0, n - 1), (n - 1, 0), (5, 5), (int(ids[9]), int(ids[10]))):
            assert_bits_equal(enc.score_internal(i, j), st.internal(qo, i, [j]), st.what + f": score_internal({i}, {j})")
        for i in (0, n - 1, int(ids[11])):
            assert_bits_equal(enc.score_internal_ids(i, ids[:70]), st.internal(qo, i, ids[:70]),
                              st.what + f": score_internal_ids({i})")
        # bursts: lists of unequal length, one of them empty
        offs = np.array([0, 40, 40, 41, 150], dtype=np.uint32)
        queries = rng.random((4, dim), dtype=np.float32)
        lrows = np.array([n - 1, 3, 0, int(ids[12])], dtype=np.uint32)
        got_q = enc.score_ids_batch(enc.encode_query_batch(queries), offs, ids[:150])
        got_i = enc.score_internal_ids_batch(lrows, offs, ids[:150])
        for l in range(4):
            a, b = int(offs[l]), int(offs[l + 1])
            assert_bits_equal(got_q[a:b], st.scores(qo, queries[l])[ids[a:b]], st.what + f": score_ids_batch, list {l}")
            assert_bits_equal(got_i[a:b], st.internal(qo, lrows[l], ids[a:b]), st.what + f": score_internal_ids_batch, list {l}")


# ------------------------------------------------------------------ 3. top-k
@pytest.mark.gpu
@pytest.mark.parametrize("dim", DIMS)
def test_topk_on_every_shape(qo, dim):
    """k <= 64 with a device-resident query: u8_topk_small_kernel; with a host query of up to 896 code bytes:
    u8_topk_small_fused_kernel, which leaves the encoded query behind; k > 64: the fused route, whose filtering pass is
    the FILTER form of u8_scan_kernel.  Expected: the stable best k of the oracle's scores (short L1 rows tie heavily)."""
    torch = pytest.importorskip("torch")
    for kind in KINDS:
        for n in TOPK_ROWS:
            st = get_store(qo, kind, dim, n)
            enc = st.open()
            on_device = enc.encode_query(torch.from_numpy(st.query).cuda())
            for largest in (True, False):
                for k in SMALL_KS + LARGE_KS:
                    check_topk(enc, on_device, st.want, k, largest, st.what + ", device query")
                if u8_actual_dim(dim) > FUSED_QUERY_BYTES:
                    continue
                for k in SMALL_KS:
                    q = enc.encode_query(st.query)  # a fresh host query each time: the kernel encodes it
                    check_topk(enc, q, st.want, k, largest, st.what + ", host query")
                    assert np.array_equal(q.encoded_query, st.codes), st.what + ": codes the top-k kernel left behind"
                    assert bits(q.offset)[0] == bits(st.qoff)[0], st.what + ": query offset the top-k kernel left behind"


# ------------------------------------------------------------------ 4. multi-query scan
@pytest.mark.gpu
@pytest.mark.parametrize("dim", E_DIMS)
def test_multi_query_scan_score_form(qo, dim):
    """score_batch on an L1 store is u8_scan_multi_kernel alone (8-, 4- and 2-wide passes, then single scans); two
    queries on a Dot / L2 store take its 2-wide pass.  The queries are distinct: a wrong multi_query_of swaps rows."""
    iters = scan_shape(dim)[1]
    for n in MULTI_ROWS:
        for kind in KINDS:
            st = get_store(qo, kind, dim, n)
            enc = st.open()
            sizes = MULTI_BATCHES[iters] if kind == "l1" else (2,)
            queries = np.random.default_rng(dim + n).random((max(sizes), dim), dtype=np.float32)
            want = np.stack([st.scores(qo, query) for query in queries])
            for size in sizes:
                got = enc.score_batch(enc.encode_query_batch(queries[:size]))
                assert got.shape == (size, n)
                for qi in range(size):
                    assert_bits_equal(got[qi], want[qi], st.what + f": score_batch of {size}, query {qi}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,dim,queries", FILTER_CASES, ids=lambda v: str(v))
def test_multi_query_scan_filter_form(qo, kind, dim, queries):
    """topk_batch above the 2 097 152-row gate: the FILTER form of u8_scan_multi_kernel.  The rows are made on the
    device; at this size the top-k is compared with the single-query topk and with the stable sort of the library's own
    score_all, and score_all with the oracle on 2002 sampled rows.  A pass that is wrong on so many rows that a query's
    candidate list overflows or stays short of k sends that query to the exact single-query route, which hides the
    mistake here (dropping the zeroing select of the clamped loads does that); the score form above has no such net."""
    torch = pytest.importorskip("torch")
    n, ad = BIG_ROWS, u8_actual_dim(dim)
    dist, invert = (D.L1, FILTER_CASES.index((kind, dim, queries)) % 2 == 1) if kind == "l1" else (D.Dot, False)
    g = torch.Generator(device="cuda")
    g.manual_seed(dim + queries)
    rows = torch.randint(0, 128, (n, ad + 4), dtype=torch.uint8, device="cuda", generator=g)
    rows[:, :4] = torch.randn(n, dtype=torch.float32, device="cuda", generator=g).view(torch.uint8).view(n, 4)
    if kind == "foreign":
        rows[n - 1, 4 + ad - 3] = 201
        rows[0, 4 + 2] = 255
        rows[n // 2, 4 + ad // 2] = 128
    idx = torch.cat([torch.tensor([0, n - 1], device="cuda"), torch.randint(0, n, (2000,), device="cuda", generator=g)])
    sample = rows[idx].cpu().numpy()
    idx = idx.cpu().numpy()
    md, _ = oracle_metas(qo, dim, n, dist, invert)
    _, sample_meta = oracle_metas(qo, dim, idx.size, dist, invert)
    enc = qa.EncodedVectorsU8.from_storage(rows, md)
    del rows
    what = f"{kind} dim {dim}, {n} rows, {dist.name} invert={invert}"
    qs = np.random.default_rng(dim).random((queries, dim), dtype=np.float32)
    batch = enc.encode_query_batch(qs)
    found = {largest: enc.topk_batch(batch, 30, largest) for largest in (True, False)}
    for qi in range(queries):
        q = enc.encode_query(qs[qi])
        scores = enc.score_all(q)
        codes, qoff = qo.u8_encode_query(sample_meta, qs[qi])
        assert_bits_equal(scores[idx], qo.u8_score_all(sample_meta, sample, codes, qoff, order=qo.ORDER_SIMPLE),
                          what + f": score_all of query {qi} on sampled rows")
        for largest, (ids, sc) in found.items():
            tag = what + f": topk_batch of {queries}, query {qi}, largest={largest}"
            wi, ws = topk_want(scores, 30, largest)
            assert np.array_equal(ids[qi], wi), tag + ": ids differ from the sorted score_all"
            assert_bits_equal(sc[qi], ws, tag + " scores")
            si, ss = enc.topk(q, 30, largest)
            assert np.array_equal(ids[qi], si), tag + ": ids differ from the single-query topk"
            assert_bits_equal(sc[qi], ss, tag + " scores against the single-query topk")


# ------------------------------------------------------------------ 5. the foreign Dot / L2 stores ran the byte kernel
def child_main():
    """On the developer library: which image the last scan of each store read."""
    from oracle import qoracle as qo

    L = qa.lib()
    L.qamd_dev_u8_last_scan_packed.restype = C.c_int
    info = {}
    for dim in PROOF_DIMS:
        st = Store(qo, "foreign", dim, PROOF_ROWS)
        assert st.rows[:, 4:].max() > 127
        masked = st.rows.copy()
        masked[:, 4:] &= 0x7F
        for name, rows in (("foreign", st.rows), ("masked", masked)):
            enc = qa.EncodedVectorsU8.from_storage(rows, st.md)
            enc.score_all(enc.encode_query(st.query))
            info[f"{dim}/{name}"] = int(L.qamd_dev_u8_last_scan_packed(enc._h))
    print("RESULT " + json.dumps(info))


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(DEV_LIB), reason="the developer library is not built")
def test_foreign_stores_scan_the_byte_codes():
    """L1 stores and rows of fewer than 8 chunks have no packed image by construction.  A Dot / L2 store of a G16 shape
    has one unless a code is above 127: the same rows with the high codes masked to 7 bits scan the image."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("QAMD_")}
    env["QAMD_LIB_PATH"] = DEV_LIB
    code = ("import sys; sys.path[:0] = [%r, %r]\nimport test_gpu_u8_byte_kernels as T\nT.child_main()\n"
            % (ROOT, os.path.join(ROOT, "tests")))
    res = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    lines = [line for line in res.stdout.splitlines() if line.startswith("RESULT ")]
    assert res.returncode == 0 and lines, f"exit {res.returncode}\n{res.stderr[-4000:]}"
    info = json.loads(lines[-1][len("RESULT "):])
    assert {scan_shape(d)[:2] for d in PROOF_DIMS} == {(16, it) for it in range(1, 9)}
    for dim in PROOF_DIMS:
        assert info[f"{dim}/foreign"] == 0, f"dim {dim}: a store with a code above 127 scanned the packed image"
        assert info[f"{dim}/masked"] == 1, f"dim {dim}: 7-bit rows did not scan the packed image"
