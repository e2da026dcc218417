"""verify_members / FilterBatchBuilder::verify of the C++ host mirror (include/turtle_kv_amd/
filter_builder.hpp), compiled against libtkv_amq.so: without a device they answer
InvalidArgument for a bad call and Unavailable for a good one; on the GPU one Bloom and one VQF
batch are built and verified clean, damaged and verified against tkv_amq_probe's answers, opened
and verified with the key CSR (tests/cpp/test_verify.cpp)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    """The test program, compiled once for both tests."""
    from turtle_kv_amd import _build
    _build.build()
    path = str(tmp_path_factory.mktemp("verify") / "test_verify")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                    "-o", path, os.path.join(ROOT, "tests", "cpp", "test_verify.cpp"),
                    "-L" + os.path.join(ROOT, "turtle_kv_amd"), "-ltkv_amq",
                    "-Wl,-rpath," + os.path.join(ROOT, "turtle_kv_amd")], check=True,
                   capture_output=True)
    return path


def test_verify_compiles_and_answers_without_a_device(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    # (with a device visible the program runs the whole round trip instead: the gpu test below)
    assert r.stdout.startswith("NODEVICE-OK") or r.stdout.startswith("OK"), r.stdout + r.stderr


@pytest.mark.gpu
def test_verify_gpu(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout + r.stderr
