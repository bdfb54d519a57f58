"""EncodedVectorsBin — host-side mirror of quantization/src/encoded_vectors_binary.rs."""
from __future__ import annotations

import ctypes as C
import enum
import os

import numpy as np

from . import _lib
from ._base import EncodedQueryBase, EncodedQueryBatch, EncodedVectorsBase
from .encoded_vectors import (EncodingError, VectorParameters, check, check_same_device, creating_on,
                              flatten_rows, get_device, in_buf, make_stop, out_buf, stream_ptr, validate)


class BitsStoreType(enum.IntEnum):
    """The two `impl BitsStoreType` of the reference (:44, :119).  Byte layout is the same on
    little-endian; only the row padding differs (:99-116 vs :152-159)."""

    U8 = 0
    U128 = 1


class BinaryEncoding(enum.IntEnum):
    """Bits kept per stored dimension.  TwoBits has no counterpart in the reference: two compares per dimension against
    thresholds mean -+ t * deviation of that dimension's data.  The Rotated kinds (no counterpart
    either) put a randomized Hadamard rotation before the bits: a vector of dim becomes one of P values, P
    the power of two at or above dim (dim <= 16384), and the store is served as a plain store of P dimensions.  The
    RotatedBlocks kinds rotate without the pad: dim is a multiple of 64, B is the largest power of two
    that divides dim (768 = 3 x 256, 1536 = 3 x 512), the vector is rotated as dim / B blocks of B values by the same
    network cut off after stage B / 2, and the store is served as a plain store of dim dimensions - a row of 768
    dimensions keeps 768 bits.  For a power-of-two dim, B = dim and the rows are those of the Rotated kinds."""

    OneBit = 0
    TwoBits = 1
    OneBitRotated = 4
    TwoBitsRotated = 5
    OneBitRotatedBlocks = 20
    TwoBitsRotatedBlocks = 21

    @property
    def two_bits(self) -> bool:
        return bool(self.value & 1)

    @property
    def rotated(self) -> bool:
        return bool(self.value & 4)

    @property
    def blocks(self) -> bool:
        return bool(self.value & 16)

    def encoder_dim(self, dim: int) -> int:
        """The dimensions the bits are taken from: dim, or P of a rotated encoding without blocks."""
        return _encoder_dim(self, dim)


def _encoder_dim(encoding, dim: int) -> int:
    """encoder_dim for an encoding given as any integer (an unknown one is the library's to refuse)."""
    if not int(encoding) & 4 or int(encoding) & 16 or dim <= 1:
        return dim
    return 1 << (dim - 1).bit_length()


def _thresholds_arg(thresholds, dim: int):
    """(lo, hi) -> two contiguous f32 arrays of dim entries and their pointers; None -> NULL pointers."""
    if thresholds is None:
        return None, None, None
    lo = np.ascontiguousarray(thresholds[0], dtype=np.float32).reshape(-1)
    hi = np.ascontiguousarray(thresholds[1], dtype=np.float32).reshape(-1)
    if lo.size != dim or hi.size != dim:
        raise EncodingError(_lib.ERR_ARGUMENTS, f"thresholds of {lo.size} and {hi.size} entries for dim {dim}")
    return (lo, hi), C.c_void_p(lo.ctypes.data), C.c_void_p(hi.ctypes.data)


class EncodedBinVector(EncodedQueryBase):
    """encoded_vectors_binary.rs:17-19."""

    _prefix = "bin"

    def _info(self):
        bits, max_abs = C.c_uint32(), C.c_float()
        check(_lib.lib().qamd_bin_query_info(self._h, C.byref(bits), C.byref(max_abs)))
        return int(bits.value), np.float32(max_abs.value)

    @property
    def bits(self) -> int:
        """Bits kept per query dimension: 1 (the reference's query), or the 4 / 8 of a scalar query."""
        return self._info()[0]

    @property
    def max_abs(self) -> np.float32:
        """The largest finite |q_i| a scalar query's codes are scaled by; 0 for a binary query."""
        return self._info()[1]

    @property
    def encoded_vector(self) -> np.ndarray:
        """The row of bits, shape (nb,); for a scalar query its bit planes, shape (bits, nb), plane 0 first."""
        n = C.c_uint64()
        check(_lib.lib().qamd_bin_query_read(self._h, None, 0, C.byref(n)))
        bits = np.zeros(n.value, dtype=np.uint8)
        if n.value:
            check(_lib.lib().qamd_bin_query_read(self._h, C.c_void_p(bits.ctypes.data), n.value, None))
        planes = self.bits
        return bits if planes == 1 else bits.reshape(planes, -1)


class EncodedBinQueryBatch(EncodedQueryBatch):
    """n x EncodedBinVector in HBM: binary queries, or 4- / 8-bit scalar queries."""

    _prefix = "bin"

    @property
    def bits(self) -> int:
        """Bits kept per query dimension: 1, 4 or 8."""
        bits = C.c_uint32()
        check(_lib.lib().qamd_bin_query_batch_info(self._h, C.byref(bits), None))
        return int(bits.value)

    def encoded_vector(self, q: int) -> np.ndarray:
        """Query q as EncodedBinVector.encoded_vector gives it: its row of bits, shape (nb,), or its bit planes, shape
        (bits, nb), plane 0 first.  A read-back for tests."""
        n = C.c_uint64()
        check(_lib.lib().qamd_bin_query_batch_read(self._h, int(q), None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=np.uint8)
        if n.value:
            check(_lib.lib().qamd_bin_query_batch_read(self._h, int(q), C.c_void_p(out.ctypes.data), n.value, None))
        planes = self.bits
        return out if planes == 1 else out.reshape(planes, -1)


class EncodedVectorsBin(EncodedVectorsBase):
    _prefix = "bin"
    _query_cls = EncodedBinVector
    _batch_cls = EncodedBinQueryBatch

    def __init__(self, handle, vector_parameters: VectorParameters, store: BitsStoreType, device=None,
                 owned: bool = True):
        super().__init__(handle, device, owned)
        self._vp = vector_parameters
        self._store = BitsStoreType(store)
        enc = C.c_int()
        check(_lib.lib().qamd_bin_get_encoding(self._h, C.byref(enc), None))
        self._encoding = BinaryEncoding(enc.value)
        self._edim = self._encoding.encoder_dim(vector_parameters.dim)

    @property
    def encoding(self) -> BinaryEncoding:
        return self._encoding

    @property
    def thresholds(self):
        """(lo, hi), dim f32 entries each (P each for rotated rows without blocks), of a two-bit store; None for one bit."""
        if not self._encoding.two_bits:
            return None
        lo, hi = np.zeros(self._edim, dtype=np.float32), np.zeros(self._edim, dtype=np.float32)
        check(_lib.lib().qamd_bin_get_thresholds(self._h, C.c_void_p(lo.ctypes.data), C.c_void_p(hi.ctypes.data)))
        return lo, hi

    @property
    def code_bits(self) -> int:
        """Bits of a stored row: dim, 2 dim (the block-rotated encodings too), or P and 2 P of the rotated encodings."""
        bits = C.c_uint64()
        check(_lib.lib().qamd_bin_get_encoding(self._h, None, C.byref(bits)))
        return int(bits.value)

    @property
    def vector_parameters(self) -> VectorParameters:
        return self._vp

    @property
    def metadata(self) -> dict:
        if self._encoding.two_bits:
            return {"vector_parameters": self._vp, "encoding": self._encoding, "thresholds": self.thresholds}
        if self._encoding.rotated:
            return {"vector_parameters": self._vp, "encoding": self._encoding}
        return {"vector_parameters": self._vp}  # :21-24

    @classmethod
    def encode(cls, orig_data, vector_parameters: VectorParameters, stop_condition=None, *,
               store: BitsStoreType = BitsStoreType.U8, stream=None,
               encoding: BinaryEncoding = BinaryEncoding.OneBit, thresholds=None) -> "EncodedVectorsBin":
        """EncodedVectorsBin::<TBitsStoreType, _>::encode (:165-191).  encoding = TwoBits: `thresholds` = (lo, hi), or
        None to take them from the data (find_stats, then thresholds_from_stats with t = 0.43).  OneBitRotated /
        TwoBitsRotated: the same on the rotated vectors, thresholds of P entries.  OneBitRotatedBlocks /
        TwoBitsRotatedBlocks (3.2h): dim % 64 == 0, thresholds of dim entries."""
        data = flatten_rows(orig_data, vector_parameters.dim)
        validate(data, vector_parameters)
        vp = vector_parameters.to_c()
        buf = in_buf(data, np.float32)
        stop = make_stop(stop_condition)
        out = C.c_void_p()
        keep, lo, hi = _thresholds_arg(thresholds, _encoder_dim(encoding, vector_parameters.dim))
        with creating_on(data) as dev:
            check(_lib.lib().qamd_bin_encode_enc(buf.ptr, buf.mem, C.byref(vp), int(store), int(encoding), lo, hi, stop,
                                                 None, stream_ptr(stream), C.byref(out)))
        return cls(out, vector_parameters, store, dev)

    @staticmethod
    def find_stats(data, stream=None):
        """(n, sum, sumsq) per dimension of a [n_rows, dim] block of f32 rows (qamd_bin_find_stats): u64 counts of the
        finite entries and their f64 sums, bit-exact whatever the batch a caller later encodes in."""
        n_rows, dim = int(data.shape[0]), int(data.shape[1])
        buf = in_buf(data, np.float32)
        n, s, q = np.zeros(dim, dtype=np.uint64), np.zeros(dim, dtype=np.float64), np.zeros(dim, dtype=np.float64)
        with creating_on(data):
            check(_lib.lib().qamd_bin_find_stats(buf.ptr, buf.mem, n_rows, dim, stream_ptr(stream), C.c_void_p(n.ctypes.data),
                                                 C.c_void_p(s.ctypes.data), C.c_void_p(q.ctypes.data)))
        return n, s, q

    @staticmethod
    def thresholds_from_stats(n, sum, sumsq, t: float = 0.43):
        """(lo, hi) = mean -+ t * deviation per dimension (qamd_bin_thresholds_from_stats; host only)."""
        n = np.ascontiguousarray(n, dtype=np.uint64)
        s = np.ascontiguousarray(sum, dtype=np.float64)
        q = np.ascontiguousarray(sumsq, dtype=np.float64)
        dim = n.size
        if s.size != dim or q.size != dim:
            raise EncodingError(_lib.ERR_ARGUMENTS, "n, sum and sumsq have one entry per dimension each")
        lo, hi = np.zeros(dim, dtype=np.float32), np.zeros(dim, dtype=np.float32)
        check(_lib.lib().qamd_bin_thresholds_from_stats(dim, C.c_void_p(n.ctypes.data), C.c_void_p(s.ctypes.data),
                                                        C.c_void_p(q.ctypes.data), float(t), C.c_void_p(lo.ctypes.data),
                                                        C.c_void_p(hi.ctypes.data)))
        return lo, hi

    def encode_query(self, query, reuse=None, stream=None, *, query_bits: int = 1, weighted: bool = False):
        """EncodedVectors::encode_query (:288-291).  query_bits = 4 or 8 keeps that many bits per query dimension
        against the same one-bit rows (no counterpart in the reference); every single-query scoring
        call takes the result.  weighted = True: against two-bit rows the codes come from
        q_i * (hi_i - lo_i) and sit at both planes of a row; against one-bit rows it changes nothing.  Without it a
        two-bit store refuses query_bits other than 1."""
        if query_bits == 1 and not weighted:
            return super().encode_query(query, reuse, stream)
        check_same_device(self._device, query)
        buf = in_buf(query, np.float32)
        n = int(np.prod(tuple(query.shape))) if hasattr(query, "shape") else len(query)
        h = reuse._h if reuse is not None else C.c_void_p()
        L = _lib.lib()
        fn = L.qamd_bin_encode_query_scalar_w if weighted else L.qamd_bin_encode_query_scalar
        check(fn(self._h, buf.ptr, n, buf.mem, int(query_bits), stream_ptr(stream), C.byref(h)))
        return reuse if reuse is not None else self._query_cls(h)

    def encode_query_batch(self, queries, reuse=None, stream=None, *, query_bits: int = 1, weighted: bool = False):
        """encode_query for a [n_queries, dim] block of queries.  query_bits = 4 or 8: query q of the batch is
        encode_query(queries[q], query_bits=...), with weighted = True that of
        encode_query(queries[q], query_bits=..., weighted=True); score_batch, score_ids_batch,
        topk_batch and topk_batch_rescored take either kind of batch."""
        nq, qdim = int(queries.shape[0]), int(queries.shape[1])
        check_same_device(self._device, queries)
        buf = in_buf(queries, np.float32)
        h = reuse._h if reuse is not None else C.c_void_p()
        L = _lib.lib()
        fn = L.qamd_bin_encode_query_batch_scalar_w if weighted else L.qamd_bin_encode_query_batch_scalar
        check(fn(self._h, buf.ptr, nq, qdim, buf.mem, int(query_bits), stream_ptr(stream), C.byref(h)))
        if reuse is not None:
            reuse.n_queries = nq
            return reuse
        return self._batch_cls(h, nq, self._prefix)

    def batch_kernel(self, batch, k: int = 0) -> str:
        """The kernel score_batch (k = 0) or the filter of topk_batch (k > 0) takes for this store and batch
        (qamd_bin_batch_kernel)."""
        name = _lib.lib().qamd_bin_batch_kernel(self._h, batch._h, int(k))
        if name is None:
            raise EncodingError(_lib.ERR_ARGUMENTS, "the batch does not belong to this store")
        return name.decode()

    @classmethod
    def encode_stream(cls, make_batches, vector_parameters: VectorParameters, stop_condition=None, *,
                      store: BitsStoreType = BitsStoreType.U8, stream=None,
                      encoding: BinaryEncoding = BinaryEncoding.OneBit, thresholds=None) -> "EncodedVectorsBin":
        """encode from the reference's iterator contract (:165-191 walks it once): `make_batches()`
        returns an iterator over [n_i, dim] f32 batches; rows are appended in order.  TwoBits without thresholds walks
        it twice: every batch is observed first (the per-dimension statistics), then pushed."""
        L = _lib.lib()
        vp = vector_parameters.to_c()
        stop = make_stop(stop_condition)
        first = next(iter(make_batches()), None)
        enc = C.c_void_p()
        keep, lo, hi = _thresholds_arg(thresholds, _encoder_dim(encoding, vector_parameters.dim))
        with creating_on(first) as dev:
            check(L.qamd_bin_encoder_begin_enc(C.byref(vp), int(store), int(encoding), lo, hi, stop, None,
                                               stream_ptr(stream), C.byref(enc)))
        passes = [L.qamd_bin_encoder_push]
        if int(encoding) in (BinaryEncoding.TwoBits, BinaryEncoding.TwoBitsRotated,
                             BinaryEncoding.TwoBitsRotatedBlocks) and thresholds is None:
            passes.insert(0, L.qamd_bin_encoder_observe)
        try:
            for feed in passes:
                for batch in make_batches():
                    if len(batch.shape) != 2 or (batch.shape[0] and batch.shape[1] != vector_parameters.dim):
                        raise EncodingError(_lib.ERR_ARGUMENTS, f"Vector length {batch.shape[-1]} does not match "
                                                                f"vector parameters dim {vector_parameters.dim}")
                    check_same_device(dev, batch)
                    buf = in_buf(batch, np.float32)
                    check(feed(enc, buf.ptr, int(batch.shape[0]), buf.mem))
            out = C.c_void_p()
            h, enc = enc, None
            check(L.qamd_bin_encoder_finish(h, C.byref(out)))
        finally:
            if enc is not None:
                L.qamd_bin_encoder_abort(enc)
        return cls(out, vector_parameters, store, dev)

    @classmethod
    def from_storage(cls, rows, vector_parameters: VectorParameters,
                     store: BitsStoreType = BitsStoreType.U8, stream=None,
                     encoding: BinaryEncoding = BinaryEncoding.OneBit, thresholds=None) -> "EncodedVectorsBin":
        """A store from rows encoded elsewhere.  TwoBits needs `thresholds` = (lo, hi): queries are encoded with them."""
        vp = vector_parameters.to_c()
        buf = in_buf(rows, np.uint8)
        out = C.c_void_p()
        keep, lo, hi = _thresholds_arg(thresholds, _encoder_dim(encoding, vector_parameters.dim))
        with creating_on(rows) as dev:
            check(_lib.lib().qamd_bin_from_rows_enc(buf.ptr, buf.mem, C.byref(vp), int(store), int(encoding), lo, hi,
                                                    stream_ptr(stream), C.byref(out)))
        return cls(out, vector_parameters, store, dev)

    @classmethod
    def load(cls, data_path, meta_path, vector_parameters: VectorParameters,
             store: BitsStoreType = BitsStoreType.U8) -> "EncodedVectorsBin":
        """EncodedVectors::load (:270-286)."""
        vp = vector_parameters.to_c()
        out = C.c_void_p()
        check(_lib.lib().qamd_bin_load(os.fsencode(data_path), os.fsencode(meta_path), C.byref(vp), int(store),
                                       C.byref(out)))
        import json
        m = json.load(open(meta_path))["vector_parameters"]
        from .encoded_vectors import DistanceType
        eff = VectorParameters(vector_parameters.dim, vector_parameters.count,
                               DistanceType[m["distance_type"]], bool(m["invert"]))
        return cls(out, eff, store, get_device())

    def save(self, data_path, meta_path) -> None:
        """EncodedVectors::save (:260-268)."""
        check(_lib.lib().qamd_bin_save(self._h, os.fsencode(data_path), os.fsencode(meta_path)))

    @staticmethod
    def get_quantized_vector_size_from_params(vector_parameters: VectorParameters,
                                              store: BitsStoreType = BitsStoreType.U8,
                                              encoding: BinaryEncoding = BinaryEncoding.OneBit) -> int:
        """:210-213, bytes per row."""
        vp = vector_parameters.to_c()
        return int(_lib.lib().qamd_bin_quantized_vector_size_enc(C.byref(vp), int(store), int(encoding)))

    def storage_bytes(self, out=None, stream=None):
        n = self._vp.count
        nb = self.get_quantized_vector_size_from_params(self._vp, self._store, self._encoding)
        check_same_device(self._device, out)
        buf, ret = out_buf(out, n * nb, np.uint8)
        check(_lib.lib().qamd_bin_export_rows(self._h, buf.ptr, buf.mem, stream_ptr(stream)))
        return ret.reshape(n, nb) if isinstance(ret, np.ndarray) else ret

    def storage_rows(self, first_row: int, n_rows: int, out=None, stream=None):
        """Rows [first_row, first_row + n_rows) as push_vector_data would receive them (encoded_storage.rs:17-25)."""
        nb = self.get_quantized_vector_size_from_params(self._vp, self._store, self._encoding)
        check_same_device(self._device, out)
        buf, ret = out_buf(out, n_rows * nb, np.uint8)
        check(_lib.lib().qamd_bin_export_rows_range(self._h, int(first_row), int(n_rows), buf.ptr, buf.mem,
                                                    stream_ptr(stream)))
        return ret.reshape(n_rows, nb) if isinstance(ret, np.ndarray) else ret
