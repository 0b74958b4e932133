"""The K5 work mapping (rectified_spaattn_amd/csrc/rsa_walk_order.h) on the host: the header is plain C++, so the same functions
the kernels inline are compiled here with the system compiler and every grid index of a launch is mapped (walk_order_check.cpp).

Cases: BH in {1, 3, 24} x NBv in {1, 7, 165, 168, 902} x generation of 32 / 64 / 128 workgroups per XCD x {no text rows, text pieces
last} x {no tail split, tail split where the plan has one} x {no table, identity table, a random permutation per head}.
Checked: every (head, unit) comes up exactly once among the whole walks or exactly tail_p times as the pieces 0 .. tail_p - 1;
the pieces of a split tail walk the eighth map's units whatever the table says; padding workgroups are exactly the table's pad
entries; the `gen` work indices of one (generation, XCD) take `gen` consecutive
sequence positions and the positions are a bijection; without a table (k5_walk_order = 0, and every kernel that is never given
one) the map is rsa_walk_unit's, as before."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_walk_order_mapping_on_the_host(tmp_path):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.fail("no system C++ compiler found (CXX, c++, g++, clang++)")
    exe = str(tmp_path / "walk_order_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "rectified_spaattn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "walk_order_check.cpp"), "-o", exe])
    res = subprocess.run([exe], capture_output=True, text=True)
    print(res.stdout)
    assert res.returncode == 0, res.stdout[-4000:] + res.stderr[-2000:]
    assert " 0 failures" in res.stdout
