"""KeyQuery::find_in_leaves of the C++ host mirror (include/turtle_kv_amd/filter_builder.hpp),
compiled against libtkv_amq.so: without a device it answers Unavailable (and tkv_amq_find_keys
itself InvalidArgument for a bad call); on the GPU one Bloom and one VQF batch are built, walked by
candidate_leaves without truth, searched, and compared with std::lower_bound on the host
(tests/cpp/test_find.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """The test program, compiled once for both tests."""
    from turtle_kv_amd import _build
    _build.build()
    path = str(tmp_path_factory.mktemp("find") / "test_find")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    "-o", path, os.path.join(ROOT, "tests", "cpp", "test_find.cpp"),
                    "-L" + os.path.join(ROOT, "turtle_kv_amd"), "-ltkv_amq",
                    "-Wl,-rpath," + os.path.join(ROOT, "turtle_kv_amd")], check=True,
                   capture_output=True)
    return path


def test_find_compiles_and_answers_without_a_device(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    # (with a device visible the program runs the whole round trip instead: the gpu test below)
    assert r.stdout.startswith("NODEVICE-OK") or r.stdout.startswith("OK"), r.stdout + r.stderr


@pytest.mark.gpu
def test_find_gpu(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
