"""The layout of a call's device arrays and ceil_log2 of the fixed-point shifts (csrc/scratch_layout.h: what Scratch
allocates and what the ray calls place into the context's ray buffer) as a stand-alone C++ program under the address
and undefined-behaviour sanitizers, in a host buffer.  Runs on the CPU; nothing of it is loaded into the interpreter."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uoparallel-seismic-project_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "scratch_layout_main.cpp")


def test_scratch_layout_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "scratch_layout")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, SRC], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "scratch layout ok" in run.stdout
