"""The original vectors of a store, kept as f32, f16 or bf16, for exact re-scoring of what a quantized scan returns
(`qamd_f32_*` in include/quantization_amd.h).  A score is `DistanceType::distance`
(quantization/src/encoded_vectors.rs:37-45) of (f32 query, row widened exactly to f32), negated for `invert`."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .encoded_vectors import (Buf, VectorParameters, check, check_same_device, creating_on, flatten_rows, in_buf, out_buf,
                              stream_ptr, validate)

MAX_RERANK_IDS = 8192
PAD_ID = 0xFFFFFFFF


DTYPES = {"f32": _lib.DTYPE_F32, "f16": _lib.DTYPE_F16, "bf16": _lib.DTYPE_BF16}


def _element_type(x) -> str | None:
    """ "f32" / "f16" / "bf16" for float data of that type, "u16" for numpy uint16, None for anything else."""
    name = str(x.dtype).replace("torch.", "")
    return {"float32": "f32", "float16": "f16", "bfloat16": "bf16", "uint16": "u16"}.get(name)


def _raw_buf(x) -> Buf:
    """`x` (f16 / bf16 values or uint16 bit patterns) as it lies in memory, made contiguous."""
    if isinstance(x, np.ndarray):
        a = np.ascontiguousarray(x)
        return Buf(C.c_void_p(a.ctypes.data), _lib.MEM_HOST, a)
    t = x.contiguous()
    return Buf(C.c_void_p(t.data_ptr()), _lib.MEM_DEVICE if t.is_cuda else _lib.MEM_HOST, t)


def _count(x) -> int:
    return int(x.numel()) if hasattr(x, "numel") else int(np.size(x))


class OriginalVectors:
    """count x dim rows (f32, f16 or bf16) resident in HBM, with the metric (`distance_type`, `invert`) of the
    quantized store they belong to."""

    def __init__(self, handle: C.c_void_p, vector_parameters: VectorParameters, device: int | None, keep=None):
        self._h = handle
        self.vector_parameters = vector_parameters
        self._device = device
        self._keep = keep  # the borrowed tensor: the handle reads the caller's memory

    @classmethod
    def from_data(cls, data, vector_parameters: VectorParameters, borrow: bool = False, stream=None,
                  dtype: str | None = None) -> "OriginalVectors":
        """`data`: [count, dim], numpy array or torch tensor.  borrow=False copies it into library-owned HBM.
        borrow=True keeps reading the caller's CUDA tensor, which this object keeps referenced (no second copy of a
        30 GB tensor); host data cannot be borrowed.

        `dtype`: what the store keeps - "f32", "f16" or "bf16"; None = f32 from whatever is given.  f16 / bf16 rows
        take half the HBM and score as their exact f32 widening.  With a `dtype`, data that is already f16 (numpy /
        torch float16) or bf16 (torch bfloat16, or numpy uint16 holding the bit patterns) must be of that type and
        is taken as it is; anything else is read as f32 and, for a half `dtype`, narrowed by the library on the
        device (round to nearest even).  A borrowed tensor must already be of the store's type."""
        if dtype is not None and dtype not in DTYPES:
            raise ValueError(f"dtype must be one of {sorted(DTYPES)} or None, got {dtype!r}")
        data = flatten_rows(data, vector_parameters.dim)
        given = _element_type(data)
        if given == "u16":
            if dtype != "bf16":
                raise ValueError("uint16 data is taken as bf16 bit patterns: pass dtype='bf16'")
            given = "bf16"
        if dtype is not None and given in ("f16", "bf16") and given != dtype:
            raise ValueError(f"{given} data cannot be kept as {dtype}: only f32 data is converted")
        validate(data, vector_parameters)
        if dtype is not None and given == dtype and given != "f32":
            buf = _raw_buf(data)
        else:
            buf, given = in_buf(data, np.float32), "f32"
        if borrow and buf.mem == _lib.MEM_DEVICE and (buf.obj is not data or given != (dtype or "f32")):
            raise ValueError(f"a borrowed tensor must be contiguous and already {dtype or 'f32'}: the handle reads it in place")
        vp = vector_parameters.to_c()
        out = C.c_void_p()
        with creating_on(data) as dev:
            if dtype is None:
                check(_lib.lib().qamd_f32_from_data(buf.ptr, buf.mem, C.byref(vp), int(bool(borrow)), stream_ptr(stream),
                                                    C.byref(out)))
            else:
                check(_lib.lib().qamd_f32_from_data_typed(buf.ptr, DTYPES[given], buf.mem, C.byref(vp), DTYPES[dtype],
                                                          int(bool(borrow)), stream_ptr(stream), C.byref(out)))
        return cls(out, vector_parameters, dev, keep=buf.obj if borrow else None)

    @property
    def dtype(self) -> str:
        """What the rows are kept as: "f32", "f16" or "bf16"."""
        d = C.c_int()
        check(_lib.lib().qamd_f32_get_dtype(self._h, C.byref(d)))
        return next(name for name, v in DTYPES.items() if v == d.value)

    @property
    def device(self) -> int | None:
        return self._device

    @property
    def count(self) -> int:
        return int(self.vector_parameters.count)

    def get_parameters(self) -> VectorParameters:
        c = _lib.VectorParametersC()
        check(_lib.lib().qamd_f32_get_parameters(self._h, C.byref(c)))
        return VectorParameters.from_c(c)

    # ------------------------------------------------------------------ upsert: overwrite / append rows in place
    def upsert(self, first_row: int, data, stream=None) -> None:
        """Rows first_row .. first_row + len(data) become `data` [n, dim]: data of the store's own element type (f16,
        bf16, or uint16 bit patterns for a bf16 store) is taken as it is, anything else is read as f32 and narrowed.
        Rows past the end extend the store; `first_row > count` and a borrowed store are refused.  A writer: no other
        call on this store may be running."""
        dim, kept = self.vector_parameters.dim, self.dtype
        data = flatten_rows(data, dim)
        shape = tuple(data.shape)
        if len(shape) != 2 or (shape[0] and shape[1] != dim):
            raise ValueError(f"upsert takes [n, {dim}] rows, got {shape}")
        given = _element_type(data)
        if given == "u16":
            if kept != "bf16":
                raise ValueError("uint16 data is taken as bf16 bit patterns: the store keeps " + kept)
            given = "bf16"
        if given in ("f16", "bf16") and given != kept:
            raise ValueError(f"{given} data cannot be kept as {kept}: only f32 data is converted")
        check_same_device(self._device, data)
        if given == kept and given != "f32":
            buf = _raw_buf(data)
        else:
            buf, given = in_buf(data, np.float32), "f32"
        check(_lib.lib().qamd_f32_upsert(self._h, int(first_row), buf.ptr, DTYPES[given], buf.mem, int(shape[0]),
                                         stream_ptr(stream)))
        self.vector_parameters = self.get_parameters()  # the cached parameters: count may have grown

    def append(self, data, stream=None) -> None:
        """upsert(count, data)."""
        self.upsert(self.count, data, stream)

    def reserve(self, n: int, stream=None) -> None:
        """Room for `n` rows, so that upserts up to there do not reallocate; no-op when there already is."""
        check(_lib.lib().qamd_f32_reserve(self._h, int(n), stream_ptr(stream)))

    @property
    def capacity(self) -> int:
        """Rows the store has room for without reallocating (a borrowed store: its count)."""
        return int(_lib.lib().qamd_f32_capacity(self._h))

    def _query(self, q):
        check_same_device(self._device, q)
        return in_buf(q, np.float32)

    def score_ids(self, query, ids, out=None, stream=None):
        """scores[k] = distance(query, row ids[k]), exact."""
        check_same_device(self._device, ids, out)
        qb, ib = self._query(query), in_buf(ids, np.uint32)
        n = _count(ids)
        buf, ret = out_buf(out, n, np.float32)
        check(_lib.lib().qamd_f32_score_ids(self._h, qb.ptr, _count(query), qb.mem, ib.ptr, n, ib.mem, buf.ptr, buf.mem,
                                            stream_ptr(stream)))
        return ret

    def score_ids_batch(self, queries, list_offsets, ids, out=None, stream=None):
        """List l = ids[list_offsets[l]:list_offsets[l + 1]] against query l of `queries` [n_queries, dim];
        scores[p] = distance(query l, row ids[p])."""
        check_same_device(self._device, list_offsets, ids, out)
        qb, ob, ib = self._query(queries), in_buf(list_offsets, np.uint32), in_buf(ids, np.uint32)
        if ob.mem != ib.mem:
            raise ValueError("list_offsets and ids must both be host or both be device buffers")
        nq, qdim = int(queries.shape[0]), int(queries.shape[1])
        n_lists, n_ids = _count(list_offsets) - 1, _count(ids)
        buf, ret = out_buf(out, n_ids, np.float32)
        check(_lib.lib().qamd_f32_score_ids_batch(self._h, qb.ptr, nq, qdim, qb.mem, ob.ptr, n_lists, ib.ptr, n_ids,
                                                  ib.mem, buf.ptr, buf.mem, stream_ptr(stream)))
        return ret

    def rerank(self, query, ids, k: int, largest: bool = True, out_ids=None, out_scores=None, stream=None):
        """The best k of `ids` by exact score: best first, ties to the lower id, padded with 0xFFFFFFFF and
        -inf / +inf; id 0xFFFFFFFF is skipped.  Returns (ids, scores)."""
        check_same_device(self._device, ids, out_ids, out_scores)
        qb, ib = self._query(query), in_buf(ids, np.uint32)
        ob, ret_ids = out_buf(out_ids, k, np.uint32)
        sb, ret_sc = out_buf(out_scores, k, np.float32)
        if ob.mem != sb.mem:
            raise ValueError("out_ids and out_scores must both be host or both be device buffers")
        check(_lib.lib().qamd_f32_rerank(self._h, qb.ptr, _count(query), qb.mem, ib.ptr, _count(ids), ib.mem, int(k),
                                         int(bool(largest)), ob.ptr, sb.ptr, sb.mem, stream_ptr(stream)))
        return ret_ids, ret_sc

    def rerank_batch(self, queries, ids, k: int, largest: bool = True, out_ids=None, out_scores=None, stream=None):
        """rerank for queries [n_queries, dim] and ids [n_queries, n_ids]; returns [n_queries, k] ids and scores."""
        check_same_device(self._device, ids, out_ids, out_scores)
        nq, qdim = int(queries.shape[0]), int(queries.shape[1])
        if int(ids.shape[0]) != nq:
            raise ValueError("one id list per query")
        n_ids = int(ids.shape[1])
        qb, ib = self._query(queries), in_buf(ids, np.uint32)
        ob, ret_ids = out_buf(out_ids, nq * k, np.uint32)
        sb, ret_sc = out_buf(out_scores, nq * k, np.float32)
        if ob.mem != sb.mem:
            raise ValueError("out_ids and out_scores must both be host or both be device buffers")
        check(_lib.lib().qamd_f32_rerank_batch(self._h, qb.ptr, nq, qdim, qb.mem, ib.ptr, n_ids, ib.mem, int(k),
                                               int(bool(largest)), ob.ptr, sb.ptr, sb.mem, stream_ptr(stream)))
        if isinstance(ret_ids, np.ndarray):
            return ret_ids.reshape(nq, k), ret_sc.reshape(nq, k)
        return ret_ids, ret_sc

    # ------------------------------------------------------------------ the whole store: a null id list = rows 0 .. count - 1
    def score_all(self, query, out=None, stream=None):
        """scores[i] = distance(query, row i) for every row, exact: one scan of the rows in order, where
        score_ids(query, arange(count)) gathers them by id."""
        check_same_device(self._device, out)
        qb = self._query(query)
        n = self.count
        buf, ret = out_buf(out, n, np.float32)
        check(_lib.lib().qamd_f32_score_ids(self._h, qb.ptr, _count(query), qb.mem, None, n, _lib.MEM_DEVICE, buf.ptr, buf.mem,
                                            stream_ptr(stream)))
        return ret

    def topk(self, query, k: int, largest: bool = True, out_ids=None, out_scores=None, stream=None):
        """The best k rows of the whole store by exact score (an exact, brute-force search): best first, ties to the
        lower row id, padded with 0xFFFFFFFF and -inf / +inf when k > count.  Returns (ids, scores)."""
        check_same_device(self._device, out_ids, out_scores)
        qb = self._query(query)
        ob, ret_ids = out_buf(out_ids, k, np.uint32)
        sb, ret_sc = out_buf(out_scores, k, np.float32)
        if ob.mem != sb.mem:
            raise ValueError("out_ids and out_scores must both be host or both be device buffers")
        check(_lib.lib().qamd_f32_rerank(self._h, qb.ptr, _count(query), qb.mem, None, self.count, _lib.MEM_DEVICE, int(k),
                                         int(bool(largest)), ob.ptr, sb.ptr, sb.mem, stream_ptr(stream)))
        return ret_ids, ret_sc

    def topk_batch(self, queries, k: int, largest: bool = True, out_ids=None, out_scores=None, stream=None):
        """topk for queries [n_queries, dim]: up to 8 queries share each pass over the rows.  Returns [n_queries, k]
        ids and scores."""
        check_same_device(self._device, out_ids, out_scores)
        nq, qdim = int(queries.shape[0]), int(queries.shape[1])
        qb = self._query(queries)
        ob, ret_ids = out_buf(out_ids, nq * k, np.uint32)
        sb, ret_sc = out_buf(out_scores, nq * k, np.float32)
        if ob.mem != sb.mem:
            raise ValueError("out_ids and out_scores must both be host or both be device buffers")
        check(_lib.lib().qamd_f32_rerank_batch(self._h, qb.ptr, nq, qdim, qb.mem, None, self.count, _lib.MEM_DEVICE, int(k),
                                               int(bool(largest)), ob.ptr, sb.ptr, sb.mem, stream_ptr(stream)))
        if isinstance(ret_ids, np.ndarray):
            return ret_ids.reshape(nq, k), ret_sc.reshape(nq, k)
        return ret_ids, ret_sc

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                _lib.lib().qamd_f32_free(self._h)
            except Exception:  # interpreter shutdown
                pass
        self._h = None
        self._keep = None
