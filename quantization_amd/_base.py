"""Scoring methods shared by the three quantizers: the C ABI gives them identical shapes
(`qamd_{u8,bin,pq}_score_*`), as `trait EncodedVectors` does in the reference
(quantization/src/encoded_vectors.rs:21-35)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .encoded_vectors import (EncodingError, VectorParameters, check, check_same_device, flatten_rows, in_buf, out_buf,
                              stream_ptr)


class EncodedQueryBase:
    _prefix = ""

    def __init__(self, handle: C.c_void_p):
        self._h = handle

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                getattr(_lib.lib(), f"qamd_{self._prefix}_query_free")(self._h)
            except Exception:  # interpreter shutdown: module globals already torn down
                pass
            self._h = None


class EncodedQueryBatch:
    """n encoded queries resident in HBM (n x EncodedQuery*), for the many-queries-at-once calls."""

    _prefix = ""

    def __init__(self, handle: C.c_void_p, n_queries: int, prefix: str | None = None):
        self._h = handle
        self.n_queries = n_queries
        if prefix is not None:
            self._prefix = prefix

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                getattr(_lib.lib(), f"qamd_{self._prefix}_query_batch_free")(self._h)
            except Exception:
                pass
        self._h = None


class EncodedVectorsBase:
    _prefix = ""
    _query_cls = EncodedQueryBase
    _batch_cls = EncodedQueryBatch

    def __init__(self, handle: C.c_void_p, device: int | None = None, owned: bool = True):
        self._h = handle
        self._device = device  # where the store lives; device buffers of every call must match
        self._owned = owned    # False: a shard borrowed from a sharded handle
        self._count = None

    def _fn(self, name):
        return getattr(_lib.lib(), f"qamd_{self._prefix}_{name}")

    @property
    def device(self) -> int | None:
        return self._device

    @property
    def count(self) -> int:
        if self._count is None:  # changes only in upsert, which resets it: one ABI round trip, not one per query
            self._count = int(self.vector_parameters.count)
        return self._count

    def encode_query(self, query, reuse=None, stream=None):
        """EncodedVectors::encode_query.  `reuse` recycles an encoded-query object (no
        allocation in a query loop)."""
        check_same_device(self._device, query)
        buf = in_buf(query, np.float32)
        n = int(np.prod(tuple(query.shape))) if hasattr(query, "shape") else len(query)
        h = reuse._h if reuse is not None else C.c_void_p()
        check(self._fn("encode_query")(self._h, buf.ptr, n, buf.mem, stream_ptr(stream), C.byref(h)))
        return reuse if reuse is not None else self._query_cls(h)

    def score_point(self, query, i: int) -> np.float32:
        """EncodedVectors::score_point — one (query, row) pair.  A kernel launch per call:
        use score_all / score_ids / topk on the hot path."""
        out = C.c_float()
        check(self._fn("score_point")(self._h, query._h, int(i), C.byref(out)))
        return np.float32(out.value)

    def score_internal(self, i: int, j: int) -> np.float32:
        """EncodedVectors::score_internal — rows i and j of the store."""
        out = C.c_float()
        check(self._fn("score_internal")(self._h, int(i), int(j), C.byref(out)))
        return np.float32(out.value)

    def score_all(self, query, out=None, stream=None):
        """scores[i] = score_point(query, i) for every row: the batched form of the caller
        loop in demos/src/ann_benchmark.rs:247-252."""
        check_same_device(self._device, out)
        buf, ret = out_buf(out, self.count, np.float32)
        check(self._fn("score_all")(self._h, query._h, buf.ptr, buf.mem, stream_ptr(stream)))
        return ret

    def score_ids(self, query, ids, out=None, stream=None):
        """scores[k] = score_point(query, ids[k]) (random access, demos/benches/encode.rs)."""
        check_same_device(self._device, ids, out)
        ib = in_buf(ids, np.uint32)
        n = int(ids.numel()) if hasattr(ids, "numel") else len(ids)
        buf, ret = out_buf(out, n, np.float32)
        check(self._fn("score_ids")(self._h, query._h, ib.ptr, n, ib.mem, buf.ptr, buf.mem,
                                    stream_ptr(stream)))
        return ret

    # ------------------------------------------------------------------ bursts of pairs (the HNSW caller)
    def score_internal_ids(self, i: int, ids, out=None, stream=None, n_rows=None):
        """scores[k] = score_internal(i, ids[k]): one stored row against many, one launch.  `ids=None` stands for the
        rows 0 .. n_rows - 1 (default: every row): score_internal_all's scan over a prefix of the store."""
        check_same_device(self._device, ids, out)
        ib = in_buf(ids, np.uint32)
        if ids is None:
            n = self.count if n_rows is None else int(n_rows)
        else:
            n = int(ids.numel()) if hasattr(ids, "numel") else len(ids)
        buf, ret = out_buf(out, n, np.float32)
        check(self._fn("score_internal_ids")(self._h, int(i), ib.ptr, n, ib.mem, buf.ptr, buf.mem, stream_ptr(stream)))
        return ret

    def _lists(self, list_offsets, ids, rows=None):
        bufs = [in_buf(list_offsets, np.uint32), in_buf(ids, np.uint32)] + ([in_buf(rows, np.uint32)] if rows is not None else [])
        if len({b.mem for b in bufs}) != 1:
            raise ValueError("list_offsets, ids and rows must all be host or all be device buffers")
        count = lambda x: int(x.numel()) if hasattr(x, "numel") else len(x)
        n_lists, n_ids = count(list_offsets) - 1, count(ids)
        if rows is not None and count(rows) != n_lists:
            raise ValueError("one row per list")
        return bufs, n_lists, n_ids

    def score_ids_batch(self, batch, list_offsets, ids, out=None, stream=None):
        """One launch for many (query, id list) pairs - one hop of every in-flight HNSW search: list l =
        ids[list_offsets[l]:list_offsets[l + 1]] is scored against query l of `batch`;
        scores[p] = score_point(query l, ids[p])."""
        check_same_device(self._device, list_offsets, ids, out)
        (ob, ib), n_lists, n_ids = self._lists(list_offsets, ids)
        buf, ret = out_buf(out, n_ids, np.float32)
        check(self._fn("score_ids_batch")(self._h, batch._h, ob.ptr, n_lists, ib.ptr, n_ids, ib.mem, buf.ptr, buf.mem,
                                          stream_ptr(stream)))
        return ret

    def score_internal_ids_batch(self, rows, list_offsets, ids, out=None, stream=None):
        """One launch for many (stored row, id list) pairs - graph construction:
        scores[p] = score_internal(rows[l], ids[p]) for the ids p of list l."""
        check_same_device(self._device, rows, list_offsets, ids, out)
        (ob, ib, rb), n_lists, n_ids = self._lists(list_offsets, ids, rows)
        buf, ret = out_buf(out, n_ids, np.float32)
        check(self._fn("score_internal_ids_batch")(self._h, rb.ptr, ob.ptr, n_lists, ib.ptr, n_ids, ib.mem, buf.ptr,
                                                   buf.mem, stream_ptr(stream)))
        return ret

    def topk(self, query, k: int, largest: bool = True, out_ids=None, out_scores=None, stream=None):
        """Best-k rows of the scan (demos/src/ann_benchmark_data.rs:151-167 keeps 30 in a heap),
        sorted best-first; ties go to the lower row id.  Returns (ids, scores)."""
        check_same_device(self._device, out_ids, out_scores)
        ib, ids = out_buf(out_ids, k, np.uint32)
        sb, sc = out_buf(out_scores, k, np.float32)
        if ib.mem != sb.mem:
            raise ValueError("out_ids and out_scores must both be host or both be device buffers")
        check(self._fn("topk")(self._h, query._h, int(k), int(bool(largest)), ib.ptr, sb.ptr, sb.mem,
                               stream_ptr(stream)))
        return ids, sc

    # ------------------------------------------------------------------ score_internal against the whole store
    def score_internal_all(self, i: int, out=None, stream=None):
        """scores[j] = score_internal(i, j) for every row j, bit for bit (row i itself included): one scan of the
        store, where score_internal_ids(i, arange(count)) is count random-access pairs."""
        check_same_device(self._device, out)
        buf, ret = out_buf(out, self.count, np.float32)
        check(self._fn("score_internal_all")(self._h, int(i), buf.ptr, buf.mem, stream_ptr(stream)))
        return ret

    def topk_internal(self, i: int, k: int, largest: bool = True, out_ids=None, out_scores=None, stream=None):
        """The k best rows of score_internal_all(i), ordered as topk orders (ties to the lower row id, best first); row
        i is among them unless the caller drops it.  Returns (ids, scores)."""
        check_same_device(self._device, out_ids, out_scores)
        ib, ids = out_buf(out_ids, k, np.uint32)
        sb, sc = out_buf(out_scores, k, np.float32)
        if ib.mem != sb.mem:
            raise ValueError("out_ids and out_scores must both be host or both be device buffers")
        check(self._fn("topk_internal")(self._h, int(i), int(k), int(bool(largest)), ib.ptr, sb.ptr, sb.mem,
                                        stream_ptr(stream)))
        return ids, sc

    # ------------------------------------------------------------------ many stored rows against the whole store
    _BATCH_BLOCK_BYTES = 512 << 20  # device score block of topk_internal_batch

    def score_internal_all_batch(self, rows, n_rows=None, out=None, stream=None):
        """scores[l, j] = score_internal(rows[l], j) for j < n_rows (default: every row), bit for bit: the null-list form
        of score_internal_ids_batch - the store is read once for a group of rows instead of once per row.  `rows` and
        `out` follow the score_internal_ids_batch rules: host rows with a host or device output, device rows (a torch
        CUDA tensor) with a device output, where a row >= count gives a NaN list.  Returns [len(rows), n_rows]."""
        check_same_device(self._device, rows, out)
        rb = in_buf(rows, np.uint32)
        n_lists = int(rows.numel()) if hasattr(rows, "numel") else len(rows)
        n = self.count if n_rows is None else int(n_rows)
        buf, ret = out_buf(out, n_lists * n, np.float32)
        check(self._fn("score_internal_ids_batch")(self._h, rb.ptr, None, n_lists, None, n, rb.mem, buf.ptr, buf.mem,
                                                   stream_ptr(stream)))
        if isinstance(ret, np.ndarray):
            return ret[:n_lists * n].reshape(n_lists, n)
        return ret

    def topk_internal_batch(self, rows, k: int, largest: bool = True, out_ids=None, out_scores=None, stream=None):
        """topk_internal(rows[l], k, largest) for every l, [len(rows), k] ids and scores: groups of rows are scored into
        a device block of at most 512 MiB (score_internal_all_batch), then each row of the block is ranked by
        topk_scores - the same contract: total order on the score bits, ties to the lower id, best first, padding
        when k > count.  Needs torch for the device block."""
        import torch

        from . import topk_scores

        check_same_device(self._device, rows, out_ids, out_scores)
        n_lists = int(rows.numel()) if hasattr(rows, "numel") else len(rows)
        k, n = int(k), self.count
        ib, ids = out_buf(out_ids, n_lists * k, np.uint32)
        sb, sc = out_buf(out_scores, n_lists * k, np.float32)
        if ib.mem != sb.mem:
            raise ValueError("out_ids and out_scores must both be host or both be device buffers")
        flat = lambda x: x.reshape(-1) if hasattr(x, "reshape") else x
        ids_f, sc_f = flat(ids), flat(sc)
        if n_lists and k and n == 0:  # an empty store: topk_internal's padding
            for l in range(n_lists):
                self.topk_internal(int(rows[l]), k, largest, ids_f[l * k:(l + 1) * k], sc_f[l * k:(l + 1) * k], stream)
        elif n_lists and k:
            device = torch.device("cuda", self._device if self._device is not None else torch.cuda.current_device())
            group = max(1, min(n_lists, self._BATCH_BLOCK_BYTES // (4 * n)))
            block = torch.empty(group * n, dtype=torch.float32, device=device)
            if stream is not None:  # the block is used on the caller's stream: torch must not hand it out before that
                block.record_stream(torch.cuda.ExternalStream(stream, device=device) if isinstance(stream, int) else stream)
            for g in range(0, n_lists, group):
                m = min(group, n_lists - g)
                self.score_internal_all_batch(rows[g:g + m], out=block, stream=stream)
                for l in range(m):
                    o = (g + l) * k
                    topk_scores(block[l * n:(l + 1) * n], n, k, largest, ids_f[o:o + k], sc_f[o:o + k], stream)
        if isinstance(ids, np.ndarray):
            return ids[:n_lists * k].reshape(n_lists, k), sc[:n_lists * k].reshape(n_lists, k)
        return ids, sc

    # ------------------------------------------------------------------ many queries at once
    def encode_query_batch(self, queries, reuse=None, stream=None):
        """encode_query for a [n_queries, dim] block of queries (the caller's outer loop,
        demos/src/ann_benchmark.rs:245-260)."""
        nq, qdim = int(queries.shape[0]), int(queries.shape[1])
        check_same_device(self._device, queries)
        buf = in_buf(queries, np.float32)
        h = reuse._h if reuse is not None else C.c_void_p()
        check(self._fn("encode_query_batch")(self._h, buf.ptr, nq, qdim, buf.mem, stream_ptr(stream), C.byref(h)))
        if reuse is not None:
            reuse.n_queries = nq
            return reuse
        return self._batch_cls(h, nq, self._prefix)

    def score_batch(self, batch, out=None, stream=None):
        """scores[q, i] = score_point(query q, i) — bit-identical to score_all per query."""
        n = self.count
        check_same_device(self._device, out)
        buf, ret = out_buf(out, batch.n_queries * n, np.float32)
        check(self._fn("score_batch")(self._h, batch._h, buf.ptr, buf.mem, stream_ptr(stream)))
        return ret.reshape(batch.n_queries, n) if isinstance(ret, np.ndarray) else ret

    def topk_batch(self, batch, k: int, largest: bool = True, out_ids=None, out_scores=None, stream=None):
        """Per-query best-k (ann_benchmark_data.rs:151-167), [n_queries, k] ids and scores."""
        nq = batch.n_queries
        check_same_device(self._device, out_ids, out_scores)
        ib, ids = out_buf(out_ids, nq * k, np.uint32)
        sb, sc = out_buf(out_scores, nq * k, np.float32)
        if ib.mem != sb.mem:
            raise ValueError("out_ids and out_scores must both be host or both be device buffers")
        check(self._fn("topk_batch")(self._h, batch._h, int(k), int(bool(largest)), ib.ptr, sb.ptr, sb.mem,
                                     stream_ptr(stream)))
        if isinstance(ids, np.ndarray):
            return ids.reshape(nq, k), sc.reshape(nq, k)
        return ids, sc

    # ------------------------------------------------------------------ rescoring with the original vectors
    def topk_rescored(self, query, orig, query_f32, k: int, candidates: int, largest: bool = True, out_ids=None,
                      out_scores=None, stream=None):
        """orig.rerank(query_f32, ids of topk(query, candidates, largest), k) in one call: the candidates stay on the
        device.  `query` is the encoded form of `query_f32`; `orig` the OriginalVectors of this store;
        k <= candidates <= 1024.  Returns (ids, scores) with the exact scores."""
        check_same_device(self._device, query_f32, out_ids, out_scores)
        qb = in_buf(query_f32, np.float32)
        qdim = int(query_f32.numel()) if hasattr(query_f32, "numel") else int(np.size(query_f32))
        ib, ids = out_buf(out_ids, k, np.uint32)
        sb, sc = out_buf(out_scores, k, np.float32)
        if ib.mem != sb.mem:
            raise ValueError("out_ids and out_scores must both be host or both be device buffers")
        check(self._fn("topk_rescored")(self._h, query._h, orig._h, qb.ptr, qdim, qb.mem, int(k), int(candidates),
                                        int(bool(largest)), ib.ptr, sb.ptr, sb.mem, stream_ptr(stream)))
        return ids, sc

    def topk_batch_rescored(self, batch, orig, queries_f32, k: int, candidates: int, largest: bool = True, out_ids=None,
                            out_scores=None, stream=None):
        """topk_rescored for every query of `batch`; `queries_f32` [n_queries, dim] are their f32 forms.  Returns
        [n_queries, k] ids and scores."""
        check_same_device(self._device, queries_f32, out_ids, out_scores)
        nq, qdim = int(queries_f32.shape[0]), int(queries_f32.shape[1])
        qb = in_buf(queries_f32, np.float32)
        ib, ids = out_buf(out_ids, nq * k, np.uint32)
        sb, sc = out_buf(out_scores, nq * k, np.float32)
        if ib.mem != sb.mem:
            raise ValueError("out_ids and out_scores must both be host or both be device buffers")
        check(self._fn("topk_batch_rescored")(self._h, batch._h, orig._h, qb.ptr, nq, qdim, qb.mem, int(k), int(candidates),
                                              int(bool(largest)), ib.ptr, sb.ptr, sb.mem, stream_ptr(stream)))
        if isinstance(ids, np.ndarray):
            return ids.reshape(nq, k), sc.reshape(nq, k)
        return ids, sc

    # ------------------------------------------------------------------ upsert: overwrite / append rows in place
    def _writable(self):
        if not self._owned:
            raise ValueError("a shard borrowed from a sharded handle cannot be written: the sharded handle's row bases are fixed")

    def upsert(self, first_row: int, data, stream=None) -> None:
        """Rows first_row .. first_row + len(data) become the encodings of `data` [n, dim] under the store's own
        parameters (nothing is learnt again); rows past the end extend the store, `first_row > count` is refused.  A
        writer: no other call on this store may be running.  Upstream's later `upsert_vector(id, vector)`, for a row
        range; the reference snapshot has no counterpart."""
        self._writable()
        vp = self.vector_parameters
        data = flatten_rows(data, vp.dim)
        shape = tuple(data.shape)
        if len(shape) != 2 or (shape[0] and shape[1] != vp.dim):
            raise EncodingError(_lib.ERR_ARGUMENTS, f"upsert takes [n, {vp.dim}] rows, got {shape}")
        check_same_device(self._device, data)
        buf = in_buf(data, np.float32)
        check(self._fn("upsert")(self._h, int(first_row), buf.ptr, buf.mem, int(shape[0]), stream_ptr(stream)))
        self._count = None  # the cached count: one ABI round trip again
        if hasattr(self, "_vp"):
            self._vp = VectorParameters(vp.dim, max(vp.count, int(first_row) + int(shape[0])), vp.distance_type, vp.invert)

    def append(self, data, stream=None) -> None:
        """upsert(count, data)."""
        self._writable()
        self.upsert(self.count, data, stream)

    def reserve(self, n: int, stream=None) -> None:
        """Room for `n` rows, so that upserts up to there do not reallocate; no-op when there already is."""
        self._writable()
        check(self._fn("reserve")(self._h, int(n), stream_ptr(stream)))

    @property
    def capacity(self) -> int:
        """Rows the store has room for without reallocating."""
        return int(self._fn("capacity")(self._h))

    def __del__(self):
        if getattr(self, "_h", None) and getattr(self, "_owned", True):
            try:
                self._fn("free")(self._h)
            except Exception:  # interpreter shutdown
                pass
        self._h = None
