"""csrc/linear.h -- the one place that decides which form a large Linear layer's products run in and queues their launches, for
the classification net (net.cpp) and for frcnn_linear_forward / frcnn_linear_backward (api.cpp) alike -- is plain host code:
tests/linear_host_check.cpp compiles it against logging stand-ins for the launchers and checks the launch sequences against
tables written out by hand.  Built with the address and undefined-behaviour sanitizers as a program of its own.  No GPU, nothing
loaded into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("linear_host") / "linear_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "linear_host_check.cpp"), "-o", out])
    return out


# the two switches of the environment are read once per process: one run per setting
@pytest.mark.parametrize("env", [{}, {"FRCNN_GEMM_F16": "0"}, {"FRCNN_GEMM_WGRAD_F16": "0"}], ids=["default", "gemm_f16_off", "wgrad_f16_off"])
def test_linear_launch_sequences_under_sanitizers(exe, env):
    e = {k: v for k, v in os.environ.items() if k not in ("FRCNN_GEMM_F16", "FRCNN_GEMM_WGRAD_F16")}
    e.update(env)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, env=e)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout
