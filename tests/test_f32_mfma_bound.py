"""The error bound of the matrix-core filter of OriginalVectors.topk_batch (csrc/f32_mfma_bound.hpp) without a GPU:
tests/cpu/f32_mfma_bound.cpp, host C++17, built plain and with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpu", "f32_mfma_bound.cpp")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]])
def test_models_of_the_matrix_unit_stay_within_the_bound(tmp_path, flags):
    exe = str(tmp_path / "f32_mfma_bound")
    subprocess.run(["g++", "-std=c++17", *flags, "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), (res.stdout + res.stderr)[-3000:]
