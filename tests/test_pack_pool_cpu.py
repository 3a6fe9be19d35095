"""The host-ingest pack pool (keyword-spotting_amd/csrc/kws_pack_pool.h) as plain host code under sanitizers.

``PackPool`` is the one piece of hand-written thread code in the library: a generation counter, two condition variables and a
slice computation whose last slices are empty when there are more threads than 4 KiB granules.  tests/native/pack_pool_check.cpp
drives it through pools of 0, 1, 3, 5 and 64 threads and copy sizes around the 1 MiB threshold, with guard bytes around every
destination.  Here that program is built twice -- ``-fsanitize=thread`` and ``-fsanitize=address,undefined`` -- and each binary runs
as a child process: exit status 0 and no sanitizer report.  Nothing is preloaded and nothing is loaded into Python; no GPU."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(REPO, "tests", "native", "pack_pool_check.cpp")
INCLUDE = os.path.join(REPO, "keyword-spotting_amd", "csrc")
SANITIZERS = {"thread": "thread", "address_undefined": "address,undefined"}
REPORT_MARKS = ("Sanitizer", "runtime error:", "SUMMARY:")


def _compilers():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    found = []
    for cand in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++"),
                 shutil.which("clang++"), shutil.which("g++"), shutil.which("c++")):
        if cand and os.path.exists(cand) and os.path.realpath(cand) not in [os.path.realpath(f) for f in found]:
            found.append(cand)
    return found


@pytest.fixture(scope="module")
def compilers():
    found = _compilers()
    if not found:
        pytest.skip("neither the ROCm clang++ nor a system C++ compiler is installed")
    return found


def _build(compilers, sanitize, out):
    """The first compiler that builds and links the program with this sanitizer's runtime; every attempt's output on failure."""
    log = []
    for cxx in compilers:
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", f"-fsanitize={sanitize}", "-fno-sanitize-recover=all",
               "-pthread", "-I", INCLUDE, SOURCE, "-o", out]
        proc = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        if proc.returncode == 0:
            return cxx
        log.append(f"$ {' '.join(cmd)}\n{proc.stdout}{proc.stderr}")
    pytest.fail("no compiler built pack_pool_check.cpp with -fsanitize=" + sanitize + ":\n" + "\n".join(log))


@pytest.mark.parametrize("name", sorted(SANITIZERS))
def test_pack_pool_is_clean_under(name, compilers, tmp_path):
    exe = str(tmp_path / f"pack_pool_check_{name}")
    cxx = _build(compilers, SANITIZERS[name], exe)
    proc = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    detail = f"{cxx} -fsanitize={SANITIZERS[name]}\nstdout:\n{proc.stdout}\nstderr:\n{proc.stderr}"
    assert proc.returncode == 0, detail
    assert not any(mark in proc.stderr for mark in REPORT_MARKS), detail
    # 5 pools x 8 sizes x 3 repeats
    assert "pack_pool_check: 120 copies, 0 failures" in proc.stdout, detail
