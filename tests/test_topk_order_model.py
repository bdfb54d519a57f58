"""The top-k order on special scores, without a GPU: the host model tests/util.py topk_total_order (what every device
route is compared with in test_gpu_topk_special_scores.py) on bit patterns written out by hand, its agreement with
topk_want where floats can state the rule, and quantization_amd.sharded.merge_topk (the numpy stand-in of
merge_topk_kernel) on the same vectors."""
import numpy as np
import pytest

from util import assert_bits_equal, topk_order_keys, topk_total_order, topk_want

from quantization_amd import sharded

PAD = 0xFFFFFFFF

# id: bit pattern.  Ascending order of the rule, written out by hand:
#   -NaN (larger payload first: below), -inf, -max, -denormal, -0, +0, +denormal, 1.0 (twice), +max, +inf, +NaN
SPECIAL_BITS = [
    0x7FC00000,  # 0  +NaN, the default quiet NaN
    0xFF800000,  # 1  -inf
    0x00000000,  # 2  +0
    0x3F800000,  # 3  1.0
    0xFFC00000,  # 4  -NaN
    0x7F7FFFFF,  # 5  +max
    0x80000001,  # 6  -denormal
    0x7FC00001,  # 7  +NaN, payload 1
    0x80000000,  # 8  -0
    0x3F800000,  # 9  1.0 again: ties with id 3
    0xFF7FFFFF,  # 10 -max
    0x7F800000,  # 11 +inf
    0x00000001,  # 12 +denormal
    0xFFC00001,  # 13 -NaN, payload 1
]
ASCENDING = [13, 4, 1, 10, 6, 8, 2, 12, 3, 9, 5, 11, 0, 7]
# largest: the same order reversed, except that equal bit patterns still go to the lower id (3 before 9)
DESCENDING = [7, 0, 11, 5, 3, 9, 12, 2, 8, 6, 10, 1, 4, 13]


def special_scores():
    return np.array(SPECIAL_BITS, dtype=np.uint32).view(np.float32)


@pytest.mark.parametrize("largest,want", [(False, ASCENDING), (True, DESCENDING)])
@pytest.mark.parametrize("k", [1, 5, 14, 20])
def test_model_on_hand_written_bit_patterns(largest, want, k):
    scores = special_scores()
    ids, sc = topk_total_order(scores, k, largest)
    n = len(want)
    assert ids.dtype == np.uint32 and sc.dtype == np.float32 and ids.shape == sc.shape == (k,)
    assert ids[: min(k, n)].tolist() == want[:k]
    assert sc[: min(k, n)].view(np.uint32).tolist() == [SPECIAL_BITS[i] for i in want[:k]]  # the rows' own bits
    assert np.all(ids[n:] == PAD)
    assert_bits_equal(sc[n:], np.full(max(k - n, 0), -np.inf if largest else np.inf, dtype=np.float32), "padding")


def test_keys_are_the_device_key():
    """topk_ordered_bits of csrc/topk_device.hpp, value by value: u ^= sign ? 0xFFFFFFFF : 0x80000000, ~u for largest."""
    for b in SPECIAL_BITS:
        u = b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)
        f = np.array([b], dtype=np.uint32).view(np.float32)
        assert int(topk_order_keys(f, False)[0]) == u
        assert int(topk_order_keys(f, True)[0]) == u ^ 0xFFFFFFFF
        assert int(sharded.topk_order_keys(f, False)[0]) == u
        assert int(sharded.topk_order_keys(f, True)[0]) == u ^ 0xFFFFFFFF


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("n,k", [(1000, 1), (1000, 37), (1000, 999), (1000, 1000), (1000, 1300), (1, 3), (0, 4)])
def test_model_equals_topk_want_where_floats_can_state_the_rule(n, k, largest):
    """Finite scores without zeros, with repeated values: on those the float compare and the key order agree."""
    rng = np.random.default_rng(n + k)
    scores = rng.standard_normal(n).astype(np.float32)
    scores[scores == 0] = 1.0
    if n > 10:
        scores[rng.integers(0, n, n // 3)] = scores[rng.integers(0, n, n // 3)]  # ties
    ids, sc = topk_total_order(scores, k, largest)
    want_ids, want_sc = topk_want(scores, k, largest)
    assert np.array_equal(ids, want_ids)
    assert_bits_equal(sc, want_sc, "scores")


def _split(scores, bounds, k, largest, pad_ids=True):
    """Per-shard lists [world, k] of the rows [bounds[g], bounds[g + 1]) by the model, local ids, padded to k."""
    ids = np.full((len(bounds) - 1, k), PAD, dtype=np.uint32)
    sc = np.zeros((len(bounds) - 1, k), dtype=np.float32)
    for g in range(len(bounds) - 1):
        ids[g], sc[g] = topk_total_order(scores[bounds[g]:bounds[g + 1]], k, largest)
    return ids, sc


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("k", [1, 3, 6, 14, 20])
def test_merge_topk_takes_the_models_order(largest, k):
    """The hand-written vector in 3 shards of 5, 3 and 6 rows (one shorter than k from k = 4 on, all of them from
    k = 7: their lists carry padding ids), merged with the shard bases: the model's list of the whole vector."""
    scores = special_scores()
    bounds = [0, 5, 8, 14]
    ids, sc = _split(scores, bounds, k, largest)
    if k > 3:
        assert (ids[1] == PAD).any()
    got_ids, got_sc = sharded.merge_topk(ids, sc, bounds[:-1], k, largest)
    want_ids, want_sc = topk_total_order(scores, k, largest)
    assert np.array_equal(got_ids, want_ids), (got_ids, want_ids)
    assert_bits_equal(got_sc, want_sc, "merged scores")


@pytest.mark.parametrize("largest", [True, False])
def test_merge_topk_padding_scores_do_not_take_part(largest):
    """A padding entry carries -inf (largest) or +inf: it must not be ranked against real -NaN / +NaN rows, which the
    rule puts behind it."""
    worst = np.array([0xFFC00000 if largest else 0x7FC00000] * 2, dtype=np.uint32).view(np.float32)
    ids = np.array([[0, PAD, PAD], [0, PAD, PAD]], dtype=np.uint32)
    pad = np.float32(-np.inf if largest else np.inf)
    sc = np.array([[worst[0], pad, pad], [worst[1], pad, pad]], dtype=np.float32)
    sc.view(np.uint32)[:, 0] = worst.view(np.uint32)
    got_ids, got_sc = sharded.merge_topk(ids, sc, [0, 7], 3, largest)
    assert got_ids.tolist() == [0, 7, PAD]
    assert got_sc.view(np.uint32)[:2].tolist() == worst.view(np.uint32).tolist()
    assert got_sc[2] == pad


@pytest.mark.parametrize("largest", [True, False])
def test_merge_topk_random_specials_many_shards(largest):
    """Random finite scores with every special pattern sprinkled in, 4 uneven shards, k below and above a shard."""
    rng = np.random.default_rng(5)
    n = 300
    scores = rng.standard_normal(n).astype(np.float32)
    at = rng.choice(n, 6 * len(SPECIAL_BITS), replace=False)
    scores.view(np.uint32)[at] = np.tile(np.array(SPECIAL_BITS, dtype=np.uint32), 6)
    bounds = [0, 10, 150, 151, 300]
    for k in (7, 40, 200):
        ids, sc = _split(scores, bounds, k, largest)
        got_ids, got_sc = sharded.merge_topk(ids, sc, bounds[:-1], k, largest)
        want_ids, want_sc = topk_total_order(scores, k, largest)
        assert np.array_equal(got_ids, want_ids), k
        assert_bits_equal(got_sc, want_sc, f"k = {k}")


class _FakeDist:
    """all_gather_into_tensor of a torch.distributed group whose other ranks' packs are given."""

    def __init__(self, packs):
        self.packs = packs

    def get_backend(self):
        return "gloo"

    def all_gather_into_tensor(self, out, mine, group=None):
        import torch

        out.copy_(torch.cat([p.reshape(-1) for p in self.packs]))


@pytest.mark.parametrize("largest", [True, False])
def test_sharded_topk_batch_host_merge_takes_the_models_order(largest):
    """ShardedTopKBatch.exchange on CPU tensors (the [world, 2, n_queries, k] form of the gloo path): 3 shards, 2 queries,
    k = 6 with one shard shorter than k, on the hand-written vector and a shuffled copy of it."""
    torch = pytest.importorskip("torch")
    k, nq, bounds = 6, 2, [0, 5, 8, 14]
    rng = np.random.default_rng(3)
    queries = [special_scores(), special_scores()[rng.permutation(14)]]
    packs = []
    for g in range(3):
        pack = np.zeros((2, nq, k), dtype=np.int32)
        for qi in range(nq):
            ids, sc = topk_total_order(queries[qi][bounds[g]:bounds[g + 1]], k, largest)
            pack[0, qi], pack[1, qi] = ids.view(np.int32), sc.view(np.int32)
        packs.append(torch.from_numpy(pack))
    ex = sharded.ShardedTopKBatch(_FakeDist(packs), torch, nq, k, "cpu", rank=0, world=3, count=14)
    assert ex.bases == [0, 4, 9]  # shard_range(14, g, 3)
    ex.bases = bounds[:-1]
    ex.pack.copy_(packs[0])
    got_ids, got_sc = ex.exchange(largest)
    for qi in range(nq):
        want_ids, want_sc = topk_total_order(queries[qi], k, largest)
        assert np.array_equal(got_ids[qi], want_ids), qi
        assert_bits_equal(got_sc[qi], want_sc, f"query {qi}")


def test_special_score_batch_shapes_reach_the_kernels_they_name(tmp_path):
    """tests/test_gpu_topk_special_scores.py names the matrix-core kernel of each u8 batch case; no call reports it
    for a handle, so u8_gemm_route() itself (csrc/u8_gemm_route.hpp, plain host C++) is asked here: 256 CUs, filter pass,
    the multipliers of an ordinary Dot (> 0) and L2 (< 0) encode, and 0 / inf for u8_gemm_kernel."""
    import os
    import subprocess

    from util import SPECIAL_U8_FAMILIES, SPECIAL_U8_GEMM_SHAPE, SPECIAL_U8_SHORT_ROW_BATCHES

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "u8_gemm_route_shapes")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
                    os.path.join(root, "tests", "cpu", "u8_gemm_route_shapes.cpp"), "-o", exe], check=True)
    ad = lambda dim: (dim + 15) // 16 * 16
    cases = []
    for family, n, dim, nq in SPECIAL_U8_FAMILIES:
        for mult in ("6.2e-05", "-1.24e-04"):
            cases.append((f"u8_gemm_{family}_kernel", f"{ad(dim)}:{n}:{mult}:{nq}"))
    n, dim, nq = SPECIAL_U8_GEMM_SHAPE
    cases += [("u8_gemm_kernel", f"{ad(dim)}:{n}:{mult}:{nq}") for mult in ("0", "inf")]
    cases += [("u8_gemm_rs_kernel", f"{ad(dim)}:{n}:6.2e-05:{nq}") for n, dim, nq in SPECIAL_U8_SHORT_ROW_BATCHES]
    got = subprocess.run([exe] + [c[1] for c in cases], capture_output=True, text=True, check=True).stdout.split()
    assert got == [c[0] for c in cases], list(zip(got, cases))
