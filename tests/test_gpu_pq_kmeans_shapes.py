"""GPU k-means (csrc/pq.hip km_* kernels) at the shapes tests/test_gpu_kmeans.py does not reach.  Same contract: the
centroids are BIT-identical to qo.find_centroids on qo.pq_sample_rows(n), the iteration count is equal, and the
precondition - no empty cluster - is asserted on both sides.

  * km_shift_sum_kernel gathers a chunk's 256 x len shifts in tiles of 4096 values and thread 0 adds them in order: chunk
    lengths above 16 need several tiles, and the parity claim rests on the running sum going on across them;
  * km_count_kernel / km_fill_kernel cut the sample into P segments; a last segment whose length is no multiple of 16 has
    zero padding that looks like centroid 0 (`if (kc == 0) n -= words * 4 - n_rows`);
  * km_update_kernel restates the reference's worker ranges (S / T rows each, the last takes the remainder), on data
    whose f64 partial sums round differently when a range ends elsewhere;
  * assignment ties while iterating (data on a coarse grid), resolved to the lower index as in kmeans.rs:139-166;
  * km_gather_rows_kernel takes the strided sample out of device-resident data.
Samples stay near 2000 rows so that the oracle's CPU loop takes well under a second per case."""
import numpy as np
import pytest

import util

pytestmark = pytest.mark.gpu

qa = pytest.importorskip("quantization_amd")
torch = pytest.importorskip("torch")
D = qa.DistanceType

N = 2051
KM_SHIFT_TILE = 4096   # kKmShiftTile
KM_MAX_SEGMENTS = 16   # kKmMaxSegments


def _check(qo, data, chunk, threads=1):
    n, dim = data.shape
    enc = qa.EncodedVectorsPQ.encode(data, qa.VectorParameters(dim, n, D.Dot, False), chunk, max_kmeans_threads=threads)
    iters, empties = enc.kmeans_info()
    want, its, o_empties = qo.find_centroids(data, chunk, qo.pq_sample_rows(n), max_threads=threads)
    assert o_empties == 0 and empties == 0, "parity is conditional on no empty cluster"
    assert iters == int(its.max())
    cen = enc.centroids
    if not np.array_equal(cen.view(np.uint32), want.view(np.uint32)):
        bad = np.argwhere(cen.view(np.uint32) != want.view(np.uint32))
        k, j = bad[0]
        raise AssertionError(f"{len(bad)} centroid values differ from kmeans.rs (iterations per chunk {its.tolist()}); first: "
                             f"centroid {k} column {j} (chunk {j // chunk}): got {cen[k, j]!r} want {want[k, j]!r}")
    assert np.array_equal(enc.storage_bytes(), qo.pq_encode(data, chunk, want))
    return enc, want, its


def _segments(S, m):
    """train_from_sample's P / seg_rows arithmetic (pq.hip) -> the segment lengths."""
    cu = torch.cuda.get_device_properties(0).multi_processor_count
    P = max(1, min(KM_MAX_SEGMENTS, (2 * cu + m - 1) // max(m, 1)))
    P = max(1, min(P, (S + 1023) // 1024))
    seg_rows = ((S + P - 1) // P + 15) // 16 * 16
    P = (S + seg_rows - 1) // seg_rows
    return [min(seg_rows, S - p * seg_rows) for p in range(P)]


@pytest.mark.parametrize("dim,chunk,values", [(64, 32, [8192, 8192]), (48, 24, [6144, 6144]), (34, 17, [4352, 4352]),
                                              (50, 20, [5120, 5120, 2560]), (32, 16, [4096, 4096])])
def test_kmeans_shift_sum_across_tiles(qo, dim, chunk, values):
    """A chunk's shift sum is over 256 * len values: two full tiles, one and a half, one tile and 256 values, chunks of
    different tile counts in one launch (20, 20, 10), and exactly one tile.  chunk 32 / 16: pq_encode_cs_kernel assigns,
    the others pq_encode_kernel."""
    m = qo.pq_chunks(dim, chunk)
    assert [256 * min(chunk, dim - c * chunk) for c in range(m)] == values
    assert any(v > KM_SHIFT_TILE for v in values) or values == [KM_SHIFT_TILE] * m
    rng = np.random.default_rng(dim * 100 + chunk)
    _enc, _want, its = _check(qo, rng.random((N, dim), dtype=np.float32), chunk)
    assert its.min() >= 3, "the stopping rule compared several sums before it fired"


@pytest.mark.parametrize("dim,chunk", [(8, 4), (3, 1), (10, 3)])
def test_kmeans_grouping_with_a_ragged_last_segment(qo, dim, chunk):
    """n = 2051 with few chunks: several segments, the last one not a multiple of 16 rows (on a full MI355X 688, 688
    and 675), so the padding correction of centroid 0's count runs where it matters."""
    segs = _segments(N, qo.pq_chunks(dim, chunk))
    assert len(segs) >= 2 and sum(segs) == N and segs[-1] % 16 != 0 and all(s % 16 == 0 for s in segs[:-1])
    rng = np.random.default_rng(dim * 100 + chunk)
    _check(qo, rng.random((N, dim), dtype=np.float32), chunk)


def _two_row_clusters(length, second):
    """512 rows of one chunk: row k < 256 is (4 k, 0, 0, ...), the initial centroid k, and row 256 + k its only
    companion, equal to it except for `second[k]` in coordinate 1.  The clusters never change; centroid k moves by
    second[k] / 2 in coordinate 1 in the first iteration and by nothing afterwards."""
    x = np.zeros((512, length), dtype=np.float32)
    x[:, 0] = 4 * (np.arange(512) % 256)
    x[256:, 1] = second
    return x


@pytest.mark.parametrize("dim,chunk", [(32, 32), (17, 17), (48, 24)])
def test_kmeans_shift_sum_order_decides_at_the_threshold(qo, dim, chunk):
    """The sum ORDER across tiles, not only their coverage: the first iteration's shifts are B = 1e-5f - 1 ulp (2^-40)
    at value 1 of the first tile and 2^-42 - a quarter of that ulp - at four values of the second tile (centroids 250 ..
    253: values 250 len + 1 >= 4096 for len >= 17).  One after the other each 2^-42 is rounded away, the sum stays B <
    KMEANS_ACCURACY and training stops after ONE iteration.  Summed per tile first, the four make a whole ulp, the sum is
    1e-5f, not below it, and a second iteration runs: the iteration count tells."""
    f32 = np.float32
    acc = f32(1e-5)
    B = np.nextafter(acc, f32(0))
    assert acc - B == f32(2.0 ** -40) and 250 * chunk + 1 >= KM_SHIFT_TILE
    second = np.zeros(256, dtype=f32)
    second[0] = 2 * B
    second[250:254] = f32(2.0 ** -41)
    data = np.ascontiguousarray(np.concatenate([_two_row_clusters(chunk, second)] * (dim // chunk), axis=1))
    # the two orders, restated: sequential f32 over [centroid][j], and tile by tile
    shifts = np.zeros((256, chunk), dtype=f32)
    shifts[:, 1] = second / 2
    flat = shifts.ravel()
    seq = f32(0)
    for v in flat[flat != 0]:
        seq = f32(seq + v)
    tiled = f32(flat[:KM_SHIFT_TILE].astype(np.float64).sum()) + f32(flat[KM_SHIFT_TILE:].astype(np.float64).sum())
    assert seq == B and seq < acc and f32(tiled) == acc
    enc, _want, its = _check(qo, data, chunk)
    assert its.tolist() == [1] * (dim // chunk) and enc.kmeans_info()[0] == 1


WORKER_PROBE_N = 2051


def _worker_probe_data(chunks=2):
    """Data on which the worker ranges of update_centroids (kmeans.rs:77-107) reach the centroids.  Cluster k is row k,
    (1000 k, 1), and two consecutive rows r, r + 1 >= 256 holding (1000 k, -1) and (1000 k, 2^-60); every other row is
    (1000 k', 0).  In f64, -1 + 2^-60 is -1: if r and r + 1 fall into the same worker's range (and row k into an earlier
    one) the cluster's sum in coordinate 1 is 1 + (-1) = 0, and if a range ends between them it is (1 - 1) + 2^-60.  So
    centroid k tells whether a boundary lies after row r.  Probes sit before and after the boundaries of T = 5, 64 and
    300 (per = S / T rows), and where a wrong remainder rule would put one (ceil(S / T) rows each; the remainder as a
    worker of its own: after rows 2049, 2047, 1799)."""
    n = WORKER_PROBE_N
    wanted = []
    for t in (5, 64, 300):
        per, up = n // t, -(-n // t)
        ends = [per * w for w in range(1, t)] + [per * t, up, 2 * up, up * (t - 1)]
        for e in sorted(set(ends), key=lambda e: -e):
            wanted += [e - 1, e, e - 2]
    probes, taken = [], set()
    for r in wanted:
        if 256 <= r and r + 1 < n and r not in taken and r + 1 not in taken and r - 1 not in taken and len(probes) < 256:
            probes.append(r)
            taken.update((r, r + 1))
    assert len(probes) == 256
    sub = np.zeros((n, 2), dtype=np.float32)
    sub[:256, 0] = 1000 * np.arange(256)
    sub[:256, 1] = 1
    free = np.array([r for r in range(256, n) if r not in taken])
    sub[free, 0] = 1000 * (np.arange(free.size) % 256)
    for k, r in enumerate(probes):
        sub[r] = (1000 * k, -1)
        sub[r + 1] = (1000 * k, 2.0 ** -60)
    return np.ascontiguousarray(np.concatenate([sub] * chunks, axis=1)), probes


@pytest.mark.parametrize("threads", [5, 64, 300])
def test_kmeans_worker_boundaries(qo, threads):
    """S / T leaves a remainder that the last worker takes: 411 rows against 410 (T = 5), 35 against 32 (T = 64), 257
    against 6 (T = 300).  T stays <= S / 2: the reference has no behaviour beyond S.  On _worker_probe_data a centroid's
    second coordinate is 0 or 2^-60 / count depending on whether a worker's range ends between its two probe rows, so
    the centroids differ between T = 1 and every tested T and between the tested T (asserted on the oracle), and a
    kernel with other boundaries - ceil(S / T) rows per worker, or the remainder left to a worker of its own - gives
    other bits."""
    n = WORKER_PROBE_N
    per = n // threads
    last = n - per * (threads - 1)
    assert threads <= n // 2 and last > per
    assert (per, last) == {5: (410, 411), 64: (32, 35), 300: (6, 257)}[threads]
    data, probes = _worker_probe_data()
    rows = qo.pq_sample_rows(n)
    want = qo.find_centroids(data, 2, rows, max_threads=threads)[0]
    # the rule, restated on the probes: zero exactly where rows r and r + 1 share a worker's range that row k is not in
    worker = lambda r: min(r // per, threads - 1)
    assert [bool(want[k, 1] == 0) for k in range(256)] == [worker(r) == worker(r + 1) != worker(k)
                                                            for k, r in enumerate(probes)]
    assert 0 < np.count_nonzero(want[:, 1]) < 256
    for other in {1, 5, 64, 300} - {threads}:
        assert not np.array_equal(want, qo.find_centroids(data, 2, rows, max_threads=other)[0])
    _check(qo, data, 2, threads=threads)


def _grid_data(seed, n=N, dim=4, chunk=2, levels=32):
    """Values k / 8 on a coarse grid; per chunk the first 256 rows (the initial centroids) are distinct points."""
    rng = np.random.default_rng(seed)
    data = np.zeros((n, dim), dtype=np.float32)
    for c in range(dim // chunk):
        idx = np.concatenate([rng.permutation(levels ** chunk)[:256], rng.integers(0, levels ** chunk, n - 256)])
        for j in range(chunk):
            data[:, c * chunk + j] = ((idx // levels ** j) % levels) / 8.0
    return data


def _tie_counts(qo, sub):
    """Rows with an exact f32 tie for the nearest centroid, per iteration of the oracle's k-means on `sub`: the
    centroids of every iteration are rebuilt from the oracle's trace (f64 sums in row order, one worker) and must end
    at the oracle's own."""
    cen, iters, _em, trace = qo.kmeans(sub, trace=True)
    cur = sub[:256].copy()
    counts = []
    for it in range(iters):
        d = util.pq_sq_dist(sub[:, None, :], cur[None, :, :])
        assert np.array_equal(d.argmin(axis=1), trace[it]), "ties go to the lower index"
        counts.append(int(((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum()))
        acc = np.zeros(cur.shape, dtype=np.float64)
        np.add.at(acc, trace[it], sub.astype(np.float64))
        cur = (acc / np.bincount(trace[it], minlength=256)[:, None]).astype(np.float32)
    assert np.array_equal(cur.view(np.uint32), cen.view(np.uint32))
    return counts


def test_kmeans_ties_inside_training(qo):
    """Grid data: rows equidistant from two centroids occur while iterating - in the first iteration (centroids are grid
    points) and in later ones (centroids are means)."""
    data = _grid_data(seed=0)
    for c in range(2):
        counts = _tie_counts(qo, np.ascontiguousarray(data[:, 2 * c:2 * c + 2]))
        assert counts[0] >= 100 and sum(1 for v in counts[1:] if v) >= 1, counts
    _check(qo, data, 2)


def test_kmeans_device_resident_input(qo):
    """km_gather_rows_kernel: the 10 000-row strided sample of 12 347 device-resident rows (a stride that is no
    integer).  Centroids equal those from host input and the oracle's."""
    n, dim, chunk = 12_347, 8, 4
    rng = np.random.default_rng(12347)
    data = rng.random((n, dim), dtype=np.float32)
    rows = qo.pq_sample_rows(n)
    assert rows.size == 10_000 and rows[1] == 1 and rows[-1] == 12_345 and len(set(np.diff(rows).tolist())) == 2
    vp = qa.VectorParameters(dim, n, D.Dot, False)
    dev = qa.EncodedVectorsPQ.encode(torch.from_numpy(data).cuda(), vp, chunk, max_kmeans_threads=2)
    host = qa.EncodedVectorsPQ.encode(data, vp, chunk, max_kmeans_threads=2)
    assert dev.kmeans_info() == host.kmeans_info() and dev.kmeans_info()[1] == 0
    assert np.array_equal(dev.centroids.view(np.uint32), host.centroids.view(np.uint32))
    assert np.array_equal(dev.storage_bytes(), host.storage_bytes())
    want, its, em = qo.find_centroids(data, chunk, rows, max_threads=2)
    assert em == 0 and dev.kmeans_info()[0] == int(its.max())
    assert np.array_equal(dev.centroids.view(np.uint32), want.view(np.uint32))


def test_kmeans_stops_at_the_100_iteration_cap(qo):
    """KMEANS_MAX_ITERATIONS: 7000 log-normal values in one dimension are still moving after 100 iterations (found by a
    CPU search over 120 seeded one-dimensional samples of 3000 - 7000 rows; seed 10 is the first that reaches the cap
    without an empty cluster).  The second column converges early and stays frozen while the first runs on."""
    n = 7000
    slow = np.random.default_rng(10).lognormal(size=(n, 1)).astype(np.float32)
    data = np.ascontiguousarray(np.concatenate([slow, np.random.default_rng(11).random((n, 1), dtype=np.float32)], axis=1))
    assert qo.kmeans(slow, max_iterations=130)[1] > 100, "the cap binds: left alone the oracle goes on"
    enc, _want, its = _check(qo, data, 1)
    assert its.tolist()[0] == 100 and its[1] < 100 and enc.kmeans_info()[0] == 100
