"""merge_levels of the C++ host mirror (include/turtle_kv_amd/filter_builder.hpp) and the K-way merge
entry points, compiled against libtkv_amq.so: the layouts, the host functions and the argument checks
with or without a device (a bad call is InvalidArgument, a good one Unavailable without a device); on
the GPU merge_levels equals a cascade of std::merge followed by the compaction loop in every byte, range
and count, for one to five levels (tests/cpp/test_levels.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """The test program, compiled once for both tests."""
    from turtle_kv_amd import _build
    _build.build()
    path = str(tmp_path_factory.mktemp("levels") / "test_levels")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    "-o", path, os.path.join(ROOT, "tests", "cpp", "test_levels.cpp"),
                    "-L" + os.path.join(ROOT, "turtle_kv_amd"), "-ltkv_amq", "-pthread",
                    "-Wl,-rpath," + os.path.join(ROOT, "turtle_kv_amd")], check=True,
                   capture_output=True)
    return path


def test_levels_compiles_and_answers_without_a_device(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    # (with a device visible the program runs the device merge too: the gpu test below)
    assert r.stdout.startswith("NODEVICE-OK") or r.stdout.startswith("OK"), r.stdout + r.stderr


@pytest.mark.gpu
def test_levels_gpu(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
