"""u8_full_route() (u8_gemm_route.hpp) without a GPU: from the filter gate on, the sample and filter passes of a full-range
store take u8_full_batch_kernel when the batch is past one scan pass, rows are at most 8256 bytes and the multiplier is
finite and not zero; everything else is routed as before, and score passes look at none of it."""
import os
import subprocess

import pytest

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpu", "u8_full_route_dump.cpp")
SCORE, SAMPLE, FILTER = 0, 1, 2


@pytest.fixture(scope="module")
def by_scans(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("route") / "u8_full_route_dump")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)

    def run(*args):  # pass, rows, actual_dim, multiplier, n_queries, multi_width
        out = subprocess.run([exe, *map(str, args)], capture_output=True, check=True, timeout=60, text=True).stdout.split()
        assert out[1:] == ["0", "0", "15"], out  # no wave lists, the Q x S sample, 15 queries per launch
        return out[0] == "1"
    return run


@pytest.mark.parametrize("pass_", [SAMPLE, FILTER])
@pytest.mark.parametrize("rows,ad,multiplier,nq,width,scans", [
    *[(rows, ad, m, nq, 0 if ad == 16 else 4, False) for rows in (32768, 10 ** 7) for ad in (16, 768, 8256) for m in ("0.5", "-0.5")
      for nq in (3 if ad == 16 else 5, 15, 16, 128)],  # (one-chunk rows have no multi-query scan: full_batch_min is 3, else 5)
    (32767, 768, "0.5", 5, 4, False),  # below the gate: the score-block route, as before
    (32768, 8272, "0.5", 5, 4, True),  # 255 * 255 * 8272 >= 2^29: past the pre-filter's range
    *[(32768, 768, m, 5, 4, True) for m in ("0", "inf", "-inf", "nan")],
    (32768, 768, "0.5", 4, 4, True), (32767, 768, "0.5", 4, 4, True), (32768, 16, "0.5", 2, 0, True)])  # one scan pass holds the batch
def test_sample_and_filter_passes(by_scans, pass_, rows, ad, multiplier, nq, width, scans):
    assert by_scans(pass_, rows, ad, multiplier, nq, width) == scans


@pytest.mark.parametrize("rows,ad,multiplier", [(r, ad, m) for r in (32767, 32768) for ad in (768, 8272) for m in ("0.5", "0", "nan")])
def test_score_passes_are_unchanged(by_scans, rows, ad, multiplier):
    assert by_scans(SCORE, rows, ad, multiplier, 4, 4) and not by_scans(SCORE, rows, ad, multiplier, 5, 4)
