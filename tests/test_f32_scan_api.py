"""The surface of the whole-store exact scan of the original vectors (no GPU): the three OriginalVectors methods, the
null-id-list convention in the header, the unchanged count of entry points, and null handles refused before any device
call - with the null list too."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

qa = pytest.importorskip("quantization_amd")
from quantization_amd import _lib  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "quantization_amd.h")).read()


def params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_methods_and_signatures():
    E = inspect.Parameter.empty
    assert params(qa.OriginalVectors.score_all) == [("self", E), ("query", E), ("out", None), ("stream", None)]
    want = [("self", E), ("query", E), ("k", E), ("largest", True), ("out_ids", None), ("out_scores", None), ("stream", None)]
    assert params(qa.OriginalVectors.topk) == want
    want[1] = ("queries", E)
    assert params(qa.OriginalVectors.topk_batch) == want
    # named and shaped like the quantizers' methods of the same names
    for name in ("score_all", "topk", "topk_batch"):
        theirs = params(getattr(qa.EncodedVectorsU8, name))
        assert [p for p, _ in theirs[2:]] == [p for p, _ in params(getattr(qa.OriginalVectors, name))[2:]], name
    # the list methods stay
    for name in ("score_ids", "score_ids_batch", "rerank", "rerank_batch"):
        assert callable(getattr(qa.OriginalVectors, name))


def comment_before(symbol):
    """The comment block that ends right before the declaration of `symbol`."""
    at = HEADER.index("QAMD_API qamd_status " + symbol + "(")
    start = HEADER.rindex("/*", 0, at)
    assert HEADER.index("*/", start) < at
    return re.sub(r"\s*\n\s*\*\s*", " ", HEADER[start:at])


@pytest.mark.parametrize("symbol", ["qamd_f32_score_ids", "qamd_f32_rerank"])
def test_header_states_the_null_list_convention(symbol):
    text = comment_before(symbol)
    assert "NULL id list stands for the rows 0, 1, ..., n_ids - 1" in text
    assert "n_ids <= count" in text
    assert "QAMD_ERR_OUT_OF_RANGE before any launch" in text
    assert "`ids_mem` is ignored" in text
    out_of_scope = text[text.index("Out of scope"):]
    for what in ("sharded handles", "qamd_f32_score_ids_batch", "scores-of-all-queries output", "_topk_rescored"):
        assert what in out_of_scope, (symbol, what)


def test_header_states_the_limits():
    rerank = comment_before("qamd_f32_rerank")
    assert "k <= 1024" in rerank and "8192" in rerank and "only for a list that is given" in rerank
    assert "synchronise `stream`" in rerank
    batch = comment_before("qamd_f32_rerank_batch")
    assert "ids = NULL" in batch and "groups of up to 8" in batch and "512 MiB" in batch
    assert "n_queries * n_ids < 2^32" in batch and "does not apply" in batch
    lists = comment_before("qamd_f32_score_ids_batch")
    assert "lists are required" in lists


def test_no_new_entry_point():
    assert len(_lib.declared_symbols()) == 192
    assert "192 entry points" in HEADER


def test_null_handles_are_refused_with_a_null_list():
    L = _lib.lib()
    q = np.zeros(4, dtype=np.float32)
    out = np.zeros(8, dtype=np.float32)
    ids = np.zeros(8, dtype=np.uint32)
    qp, op, ip = (C.c_void_p(a.ctypes.data) for a in (q, out, ids))
    H, none = _lib.MEM_HOST, None
    assert L.qamd_f32_score_ids(none, qp, 4, H, none, 8, H, op, H, none) == _lib.ERR_ARGUMENTS
    assert b"null handle" in L.qamd_last_error()
    assert L.qamd_f32_rerank(none, qp, 4, H, none, 8, H, 2, 1, ip, op, H, none) == _lib.ERR_ARGUMENTS
    assert b"null handle" in L.qamd_last_error()
    assert L.qamd_f32_rerank_batch(none, qp, 1, 4, H, none, 8, H, 2, 1, ip, op, H, none) == _lib.ERR_ARGUMENTS
    assert b"null handle" in L.qamd_last_error()
    # and with n_ids past the 8192 of a given list: still the handle, not the list
    assert L.qamd_f32_rerank(none, qp, 4, H, none, 10_000, H, 2, 1, ip, op, H, none) == _lib.ERR_ARGUMENTS
    assert b"null handle" in L.qamd_last_error()
