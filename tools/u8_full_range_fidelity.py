"""recall@10 of the scalar-u8 quantizer's Dot scores at 127 levels (the reference's truncating code) against 255 levels
(QAMD_FULL, rounded to nearest), in a numpy model on the CPU: 20000 x 128 rows, 100 queries = rows plus
noise, the exact f32 ranking as the truth.  Sets: column scales exp(N(0, 1)) (the recipe of tests/test_u8_rotated_model),
plain and through the block rotation, and a clustered mixture (64 centres, within-cluster sigma 0.3).  Synthetic rows:
the figures say nothing about real embeddings.  Usage: python tools/u8_full_range_fidelity.py > profiles/u8_full_range_fidelity.txt"""
import argparse
import os
import sys

import numpy as np

sys.path[:0] = [os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"),
                os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")]
import u8_rotated_model as um  # noqa: E402

f32 = np.float32


def codes(v, alpha, offset, levels):
    x = (v - offset) / alpha + (0.0 if levels == 127 else 0.5)
    return np.floor(np.clip(x, 0, levels))


def recall(x, q, levels, quantile=None, k=10):
    exact = q.astype(np.float64) @ x.astype(np.float64).T
    lo, hi = (x.min(), x.max()) if quantile is None else np.quantile(x, [(1 - quantile) / 2, 1 - (1 - quantile) / 2])
    alpha, offset = (hi - lo) / levels, lo
    c, cq = codes(x, alpha, offset, levels), codes(q, alpha, offset, levels)
    # the dot product of the dequantised vectors: alpha^2 c.cq + alpha offset (sum c + sum cq) + dim offset^2
    got = alpha * alpha * (cq @ c.T) + alpha * offset * (c.sum(1)[None, :] + cq.sum(1)[:, None])
    hits = sum(len(set(np.argsort(-got[i], kind="stable")[:k]) & set(np.argsort(-exact[i], kind="stable")[:k])) for i in range(len(q)))
    return hits / (len(q) * k)


def dataset(kind, seed, n=20000, dim=128, nq=100):
    rng = np.random.default_rng(seed)
    if kind == "clustered":
        x = rng.normal(size=(64, dim))[rng.integers(0, 64, n)] + 0.3 * rng.normal(size=(n, dim))
    else:
        x = rng.normal(size=(n, dim)) * np.exp(rng.normal(size=dim))
    x = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(f32)
    q = x[rng.choice(n, nq, replace=False)] + (0.3 / np.sqrt(dim)) * rng.normal(size=(nq, dim))
    q = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)
    return x, q


if __name__ == "__main__":
    argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter).parse_args()
    print("# recall@10, numpy model of Dot scores, 20000 x 128 synthetic rows, 100 queries; levels 127 (truncating) / 255 (rounded)")
    for kind in ("lognormal", "lognormal rotated", "clustered", "clustered rotated"):
        for quantile in (None, 0.99):
            for seed in (1, 2, 3):
                x, q = dataset(kind.split()[0], seed)
                if kind.endswith("rotated"):
                    x, q = um.rotate(x), um.rotate(q)
                r127, r255 = recall(x, q, 127, quantile), recall(x, q, 255, quantile)
                print(f"{kind:18s} interval {'min/max' if quantile is None else 'q0.99  '} seed {seed}: 127 -> {r127:.3f}   255 -> {r255:.3f}")
