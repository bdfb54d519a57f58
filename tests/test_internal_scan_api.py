"""CPU-side checks of score_internal against the whole store: the header declares the six entry points with
their signatures and states the contract, the library exports them, the ctypes mirror binds them, null handles are refused
before any device call, the Python methods exist and the sharded classes do not have them.  No GPU is needed.  (A handle
cannot exist without a GPU: the refusals that need one are in tests/test_gpu_internal_scan.py.)"""
import inspect
import os
import re

import quantization_amd as qa
from quantization_amd import _lib

KINDS = ("u8", "pq", "bin")
NEW = [f"qamd_{k}_{f}" for k in KINDS for f in ("score_internal_all", "topk_internal")]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "quantization_amd.h")).read()


def flat(text):
    """A comment as one line of words: the ` * ` of continuation lines and the line breaks removed."""
    return re.sub(r"\s+", " ", re.sub(r"\n\s*\*", " ", text))


def test_header_declares_the_entry_points_with_their_signatures():
    hdr = header()
    declared = set(_lib.declared_symbols())
    assert not [s for s in NEW if s not in declared]
    assert len(declared) == 192
    for k in KINDS:
        assert re.search(rf"qamd_status qamd_{k}_score_internal_all\(const qamd_{k} \*h, uint32_t i, float \*out, "
                         rf"qamd_mem out_mem,\s*void \*stream\);", hdr), k
        assert re.search(rf"qamd_status qamd_{k}_topk_internal\(const qamd_{k} \*h, uint32_t i, uint32_t k, int largest,\s*"
                         rf"uint32_t \*out_ids, float \*out_scores, qamd_mem out_mem, void \*stream\);", hdr), k
        # declared next to the quantizer's score_internal_ids: after it, before its score_all
        assert hdr.index(f" qamd_{k}_score_internal_ids(") < hdr.index(f" qamd_{k}_score_internal_all(") \
            < hdr.index(f" qamd_{k}_score_all("), k


def test_header_states_the_contract():
    hdr = header()
    at = hdr.index(" qamd_u8_score_internal_all(")
    comment = flat(hdr[hdr.rindex("/*", 0, at):at])
    assert "out[j] has the bits of *_score_internal(h, i, j) for every j < count" in comment
    assert "Row i itself is included" in comment
    assert "ties to the lower id" in comment and "best first" in comment and "NaN" in comment
    assert "k <= 1024" in comment and "k == 0 is QAMD_OK" in comment
    assert "i >= count is QAMD_ERR_ARGUMENTS, refused before any launch" in comment
    assert "a null handle is refused before any device call" in comment
    assert "an empty store is QAMD_OK" in comment
    assert re.search(r"synchronise exactly as \*_score_all / \*_topk do", comment)
    for cite in ("encoded_vectors_u8.rs:386-453", "encoded_vectors_pq.rs:566-593", "encoded_vectors_binary.rs:302-314"):
        assert cite in comment, cite
    assert "the whole-store form has no counterpart there" in comment
    assert "192 entry points" in comment
    # what is left out, as sentences
    assert re.search(r"Sharded handles have no whole-store score_internal\.", comment)
    assert re.search(r"no batched topk_internal_batch", comment)
    assert re.search(r"no rescored variant", comment)
    assert "without centroids" in comment
    # the other two quantizers point back at this contract and cite their own lines
    for k, cite in (("bin", ":302-314"), ("pq", ":566-593")):
        at = hdr.index(f" qamd_{k}_score_internal_all(")
        c = flat(hdr[hdr.rindex("/*", 0, at):at])
        assert cite in c and "contract as qamd_u8_score_internal_all" in c, k


def test_documents_agree_on_the_count_and_on_what_is_left_out():
    readme = open(os.path.join(ROOT, "README.md")).read()
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "192 entry points" in readme and "192 entry points" in design
    assert "3.10" in design
    for doc in (design, integ):
        assert "score_internal_all" in doc and "topk_internal" in doc
    sec = flat(design[design.index("3.10"):])
    assert re.search(r"[Ss]harded handles", sec) and "topk_internal_batch" in sec and re.search(r"rescored variant", sec)


def test_library_exports_and_the_mirror_binds_them():
    L = _lib.lib()
    assert not [s for s in _lib.declared_symbols() if not hasattr(L, s)]
    for k in KINDS:
        assert len(getattr(L, f"qamd_{k}_score_internal_all").argtypes) == 5, k
        assert len(getattr(L, f"qamd_{k}_topk_internal").argtypes) == 8, k


def test_null_handles_are_refused_before_any_device_call():
    import numpy as np

    L = _lib.lib()
    out = np.zeros(4, dtype=np.float32)
    ids = np.zeros(4, dtype=np.uint32)
    for k in KINDS:
        assert getattr(L, f"qamd_{k}_score_internal_all")(None, 0, out.ctypes.data, _lib.MEM_HOST, None) == _lib.ERR_ARGUMENTS, k
        assert b"null handle" in L.qamd_last_error()
        assert getattr(L, f"qamd_{k}_topk_internal")(None, 0, 4, 1, ids.ctypes.data, out.ctypes.data, _lib.MEM_HOST,
                                                      None) == _lib.ERR_ARGUMENTS, k
        assert b"null handle" in L.qamd_last_error()
        # ... even where nothing is asked for (k == 0 is QAMD_OK only on a handle)
        assert getattr(L, f"qamd_{k}_topk_internal")(None, 0, 0, 1, None, None, _lib.MEM_HOST, None) == _lib.ERR_ARGUMENTS, k


def test_python_surface():
    for cls in (qa.EncodedVectorsU8, qa.EncodedVectorsPQ, qa.EncodedVectorsBin):
        assert list(inspect.signature(cls.score_internal_all).parameters) == ["self", "i", "out", "stream"], cls
        assert list(inspect.signature(cls.topk_internal).parameters) == ["self", "i", "k", "largest", "out_ids", "out_scores",
                                                                         "stream"], cls
        assert inspect.signature(cls.topk_internal).parameters["largest"].default is True
        for name in ("out", "stream"):
            assert inspect.signature(cls.score_internal_all).parameters[name].default is None


def test_the_sharded_classes_do_not_have_them():
    for cls in (qa.ShardedVectorsU8, qa.ShardedVectorsPQ, qa.ShardedVectorsBin):
        assert not hasattr(cls, "score_internal_all") and not hasattr(cls, "topk_internal"), cls
