"""Which matrix-core kernel serves a batch of u8 queries (quantization_amd/csrc/u8_gemm_route.hpp), without a GPU:
tests/cpu/u8_gemm_route_dump.cpp is compiled with g++ alone - the route header is plain host C++17 - and prints the
route over a grid of row lengths, store sizes, CU counts, multipliers, passes and developer switches as change points
along the batch size (keys with the same change points listed together).  Its output must equal
tests/golden/u8_gemm_route_table.txt byte for byte.  That table was generated from the selection predicates
u8_batch.hip had before the route was one function (lifted verbatim into a harness), so a differing line is a batch
that changed kernel, launch slicing or candidate-list bookkeeping."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu", "u8_gemm_route_dump.cpp")
TABLE = os.path.join(ROOT, "tests", "golden", "u8_gemm_route_table.txt")


def test_route_table_is_unchanged(tmp_path):
    exe = str(tmp_path / "u8_gemm_route_dump")
    # no ROCm include path, no library: the header must stand alone
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", SRC, "-o", exe], check=True)
    got = subprocess.run([exe], capture_output=True, check=True, timeout=300).stdout
    with open(TABLE, "rb") as f:
        want = f.read()
    if got != want:
        g, w = got.decode().splitlines(), want.decode().splitlines()
        first = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b), min(len(g), len(w)))
        raise AssertionError(f"route table differs from line {first + 1} (of {len(g)} / {len(w)}): "
                             f"got {g[first:first + 1]}, want {w[first:first + 1]}")
    assert len(want) < 512 * 1024


def test_route_table_names_only_kernels_that_exist():
    """Every kernel the table names is one the source defines, and every u8_gemm_*_kernel the source defines is reached
    somewhere on the product grid (none is dead weight behind a developer switch)."""
    import re
    with open(os.path.join(ROOT, "quantization_amd", "csrc", "u8_batch.hip")) as f:
        defined = set(re.findall(r"void (u8_gemm_\w*kernel)\(", f.read()))
    named, product = set(), set()
    with open(TABLE) as f:
        grid = ""
        for ln in f:
            if ln.startswith("=="):
                grid = ln.split()[1]
            if not ln.startswith(" "):
                continue
            short = ln.split()[1]
            name = "u8_gemm_kernel" if short == "gemm" else f"u8_gemm_{short}_kernel"
            named.add(name)
            if grid == "product":
                product.add(name)
    assert named == defined, (sorted(named), sorted(defined))
    assert product == defined, sorted(defined - product)
