"""The strided LDS image of the Bloom leaf builds (turtle_kv_amd/csrc/tkv_amq_lds_stride.h) as plain
host C++: for images of 1..65 blocks the (block, word) -> address map is injective, in range,
4-byte aligned, has the word at address bits 5..8, and the write-out's inverse returns every
(block, word) (tests/cpp/test_lds_stride.cpp).  No device and no library: the header only."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("lds_stride") / "test_lds_stride")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-O1", "-std=c++17", "-Wall", "-Werror",
                    "-I" + os.path.join(ROOT, "turtle_kv_amd", "csrc"), "-o", path,
                    os.path.join(ROOT, "tests", "cpp", "test_lds_stride.cpp")], check=True,
                   capture_output=True)
    return path


def test_lds_stride_layout(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
