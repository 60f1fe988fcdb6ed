"""csrc/pack_tables.h -- the one place that decides which weight tensor of the proposal net gets which pack job, and names the
spans of the three device job tables that the forward prologue, frcnn_pnet_refresh_packs and the dense anchor-net backward launch
from -- is plain host code: tests/pack_tables_host_check.cpp compiles it against recording stand-ins for the job constructors and
the block-assignment functions and checks every span against lists written out by hand.  Built with the address and
undefined-behaviour sanitizers as a program of its own.  No GPU, nothing loaded into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    out = str(tmp_path_factory.mktemp("pack_tables_host") / "pack_tables_host_check")
    subprocess.check_call([cxx, "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "pack_tables_host_check.cpp"), "-o", out])
    return out


def test_pack_table_spans_under_sanitizers(exe):
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "0 failures" in r.stdout, r.stdout
