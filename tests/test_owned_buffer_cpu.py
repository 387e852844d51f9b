"""The owner of a block of device memory (csrc/owned_buffer.h: DevBuf of ttsweep_ctx.h, the block of a call's
Scratch) as a stand-alone C++ program under the address and undefined-behaviour sanitizers, over a malloc / free
policy that counts, records and fails on request.  It shows that a block is released exactly once, also when a
release or an allocation fails, which no GPU test may provoke.  Runs on the CPU; nothing of it is loaded into the
interpreter."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uoparallel-seismic-project_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "owned_buffer_main.cpp")


def test_owned_buffer_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "owned_buffer")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, SRC], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "owned buffer ok" in run.stdout
