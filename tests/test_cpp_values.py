"""TreeIndex::get_values_host and KeyQuery::get_values of the C++ host mirror (include/turtle_kv_amd/
filter_builder.hpp), compiled against libtkv_amq.so: get_values_host is held to a hand-written
expectation (deltas summed across two levels, a node and a child; a tombstone; a flushed ADD that is
not taken; bad combinations) with or without a device, so the CPU suite covers the mirror's logic;
the device path answers Unavailable without one (and the entry points themselves InvalidArgument
for a bad call); on the GPU KeyQuery::get_values equals get_values_host in every field, in the
counts and in the gathered bytes on a tree of height 3 (tests/cpp/test_values.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """The test program, compiled once for both tests."""
    from turtle_kv_amd import _build
    _build.build()
    path = str(tmp_path_factory.mktemp("values") / "test_values")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    "-o", path, os.path.join(ROOT, "tests", "cpp", "test_values.cpp"),
                    "-L" + os.path.join(ROOT, "turtle_kv_amd"), "-ltkv_amq", "-pthread",
                    "-Wl,-rpath," + os.path.join(ROOT, "turtle_kv_amd")], check=True,
                   capture_output=True)
    return path


def test_values_compiles_and_answers_without_a_device(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    # (with a device visible the program runs the device lookup too: the gpu test below)
    assert r.stdout.startswith("NODEVICE-OK") or r.stdout.startswith("OK"), r.stdout + r.stderr


@pytest.mark.gpu
def test_values_gpu(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
