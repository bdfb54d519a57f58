"""The null-list form of *_score_internal_ids_batch / *_score_internal_ids: many stored rows against the
whole store with no new entry point.  The header states the convention at the burst calls and keeps its 192 entry points,
null handles are refused before any device call, the Python methods exist on the three quantizers and the sharded classes
do not have them.  No GPU is needed (the refusals that need a handle are in tests/test_gpu_internal_batch.py)."""
import inspect
import os
import re

import numpy as np

import quantization_amd as qa
from quantization_amd import _lib

KINDS = ("u8", "pq", "bin")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "quantization_amd.h")).read()


def flat(text):
    return re.sub(r"\s+", " ", re.sub(r"\n\s*\*", " ", text))


def comment_before(hdr, symbol):
    at = hdr.index(f" {symbol}(")
    return flat(hdr[hdr.rindex("/*", 0, at):at])


def test_header_states_the_convention_at_the_burst_calls():
    hdr = header()
    c = comment_before(hdr, "qamd_u8_score_internal_ids_batch")
    assert "ids == NULL stands, for EVERY list, for the rows 0 .. n_ids - 1" in c
    assert "n_ids is then the length of each list, not the total" in c
    assert "out[l * n_ids + j] has the bits of *_score_internal(h, rows[l], j)" in c
    assert "Row rows[l] itself is included" in c and "duplicates in rows are allowed" in c
    assert "list_offsets without ids is QAMD_ERR_ARGUMENTS" in c
    assert "n_ids > count is QAMD_ERR_OUT_OF_RANGE before any launch" in c
    assert "n_lists == 0 or n_ids == 0 is QAMD_OK and nothing is written" in c
    assert "a null handle is refused before any device call" in c
    assert "a row >= count is QAMD_ERR_OUT_OF_RANGE before any launch" in c
    assert "a row >= count gives NaN in all n_ids outputs of its list" in c
    assert "Device rows need a device output" in c
    assert "within 512 MiB" in c and "never allocates n_lists * n_ids * 4 bytes" in c
    assert "lane mode" in c and "without centroids is QAMD_ERR_ARGUMENTS" in c
    assert "no entry point of its own" in c
    c = comment_before(hdr, "qamd_u8_score_internal_ids")
    assert "ids == NULL stands for the rows 0 .. n_ids - 1" in c
    assert "ids_mem is ignored" in c and "n_ids > count is QAMD_ERR_OUT_OF_RANGE" in c
    for k in ("bin", "pq"):  # the other two point back at that text
        c = comment_before(hdr, f"qamd_{k}_score_internal_ids")
        assert "ids == NULL" in c and "as stated at qamd_u8_score_internal_ids and qamd_u8_score_internal_ids_batch" in c, k
    # the whole-store block tells where the many-row form is
    c = comment_before(hdr, "qamd_u8_score_internal_all")
    assert "the scores of many rows come from the null-list form of *_score_internal_ids_batch" in c
    assert "ranking them is qamd_topk_scores per row" in c


def test_the_header_keeps_its_192_entry_points():
    assert len(_lib.declared_symbols()) == 192
    L = _lib.lib()
    assert not [s for s in _lib.declared_symbols() if not hasattr(L, s)]


def test_documents_have_the_section():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 3.12" in design and "192 entry points" in design
    sec = flat(design[design.index("### 3.12"):design.index("## 4. Parity")])
    for left_out in ("harded handles", "fused filter top-k", "matrix-core", "rescored variant"):
        assert left_out in sec, left_out
    assert "score_internal_all_batch" in sec and "512 MiB" in sec
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "std::ptr::null()" in integ and "NULL id list" in integ
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "192 entry points" in readme and "§3.12" in readme


def test_null_handles_are_refused_before_any_device_call():
    L = _lib.lib()
    out = np.zeros(4, dtype=np.float32)
    rows = np.zeros(2, dtype=np.uint32)
    for k in KINDS:
        batch, one = getattr(L, f"qamd_{k}_score_internal_ids_batch"), getattr(L, f"qamd_{k}_score_internal_ids")
        assert batch(None, rows.ctypes.data, None, 2, None, 2, _lib.MEM_HOST, out.ctypes.data, _lib.MEM_HOST, None) == _lib.ERR_ARGUMENTS, k
        assert b"null handle" in L.qamd_last_error()
        assert one(None, 0, None, 4, _lib.MEM_HOST, out.ctypes.data, _lib.MEM_HOST, None) == _lib.ERR_ARGUMENTS, k
        assert b"null handle" in L.qamd_last_error()
    assert not out.any()


def test_python_surface():
    for cls in (qa.EncodedVectorsU8, qa.EncodedVectorsPQ, qa.EncodedVectorsBin):
        sig = inspect.signature(cls.score_internal_all_batch)
        assert list(sig.parameters) == ["self", "rows", "n_rows", "out", "stream"], cls
        assert all(sig.parameters[p].default is None for p in ("n_rows", "out", "stream"))
        sig = inspect.signature(cls.topk_internal_batch)
        assert list(sig.parameters) == ["self", "rows", "k", "largest", "out_ids", "out_scores", "stream"], cls
        assert sig.parameters["largest"].default is True
        assert all(sig.parameters[p].default is None for p in ("out_ids", "out_scores", "stream"))
        # the older calls keep their leading parameters
        assert list(inspect.signature(cls.score_internal_ids).parameters)[:5] == ["self", "i", "ids", "out", "stream"]
        assert list(inspect.signature(cls.score_internal_all).parameters) == ["self", "i", "out", "stream"]


def test_the_sharded_classes_do_not_have_them():
    for cls in (qa.ShardedVectorsU8, qa.ShardedVectorsPQ, qa.ShardedVectorsBin):
        assert not hasattr(cls, "score_internal_all_batch") and not hasattr(cls, "topk_internal_batch"), cls
