"""The host-side rules of the solve drivers (csrc/driver_rules.h: ring lists and fill marks, the gate distance of a
unit, the column driver's claim sequences, resident grids, the wall-clock limit, what may run in place) as a stand-alone
C++ program under the address and undefined-behaviour sanitizers.  Runs on the CPU; nothing of it is loaded into the interpreter."""
import os
import shutil
import subprocess


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uoparallel-seismic-project_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "driver_rules_main.cpp")


def test_driver_rules_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path / "driver_rules")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, SRC], capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "driver rules ok" in run.stdout
