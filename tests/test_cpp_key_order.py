"""The order of two keys (turtle_kv_amd/csrc/tkv_amq_key_order.h) as plain host C++ under
AddressSanitizer and UBSan: key_compare against std::string_view's order, the 16- and 24-byte fast
modes against the any-shape mode, bound() against std::lower_bound / std::upper_bound, the mode
chooser and leaf_key_range's clamping, every key in a heap allocation of exactly its length
(tests/cpp/test_key_order.cpp).  No device and no library: the header only, in a stand-alone
program run directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("key_order") / "test_key_order")
    subprocess.run(["/opt/rocm/bin/hipcc", "-x", "c++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "turtle_kv_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                    "-o", path, os.path.join(ROOT, "tests", "cpp", "test_key_order.cpp")], check=True,
                   capture_output=True)
    return path


def test_key_order(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
