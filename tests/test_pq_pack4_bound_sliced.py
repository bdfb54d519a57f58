"""The packed 8-bit filter bound (csrc/pq_pack4.hpp) for rows of 160 .. 256 chunks, summed slice by slice, without a GPU:
tests/cpu/pq_pack4_bound_sliced.cpp, host C++17, built plain and with the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpu", "pq_pack4_bound_sliced.cpp")


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]])
def test_no_reaching_row_is_rejected_and_sums_fit_16_bits(tmp_path, flags):
    exe = str(tmp_path / "pq_pack4_bound_sliced")
    subprocess.run(["g++", "-std=c++17", *flags, "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip().endswith("ok"), (res.stdout + res.stderr)[-3000:]
