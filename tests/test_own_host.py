"""csrc/own.h -- the types that own the model's events, device buffers and page-locked ring (net.cpp) -- are plain host code:
tests/own_host_check.cpp exercises them against counting stand-ins for the runtime calls, built with the address and
undefined-behaviour sanitizers as a program of its own.  No GPU, nothing loaded into this process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_event_and_buffer_ownership_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "own_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "own_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout
