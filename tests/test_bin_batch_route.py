"""Which kernel serves a batch of binary or scalar queries (quantization_amd/csrc/bin_batch_route.hpp) and which pivot
sample a matrix-core topk_batch takes (quantization_amd/csrc/batch_plan.hpp), without a GPU:
tests/cpu/bin_batch_route_dump.cpp is compiled with g++ alone - both headers are plain host C++17 - and prints the route
over a grid of row lengths, store sizes, query bits, k and developer switches as change points along the batch size, and
the sample plan over a grid of store sizes, batch sizes and k.  Its output must equal
tests/golden/bin_batch_route_table.txt byte for byte.  That table was generated from the predicates bin.hip had and the
sample arithmetic u8_batch.hip and bin.hip shared before either header existed (lifted verbatim into a harness), so a
differing line is a batch that changed kernel, launch shape, candidate-list bookkeeping or pivot sample."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpu", "bin_batch_route_dump.cpp")
TABLE = os.path.join(ROOT, "tests", "golden", "bin_batch_route_table.txt")


def test_route_table_is_unchanged(tmp_path):
    exe = str(tmp_path / "bin_batch_route_dump")
    # no ROCm include path, no library: the headers must stand alone
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
    """Every kernel the table names is one bin.hip defines, and every bin_gemm_*_kernel it defines is reached somewhere
    on the product grid (none is dead weight behind a developer switch)."""
    with open(os.path.join(ROOT, "quantization_amd", "csrc", "bin.hip")) as f:
        defined = set(re.findall(r"void (bin_gemm_\w*kernel)\(", f.read()))
    named, product = set(), set()
    with open(TABLE) as f:
        grid = ""
        for ln in f:
            if ln.startswith("=="):
                grid = ln.split()[1]
            if not ln.startswith("  ") or ln.split()[1] == "-":
                continue
            name = f"bin_gemm_{ln.split()[1]}_kernel"
            named.add(name)
            if grid == "product":
                product.add(name)
    assert named == defined, (sorted(named), sorted(defined))
    assert product == defined, sorted(defined - product)
