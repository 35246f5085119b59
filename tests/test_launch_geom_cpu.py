"""csrc/launch_geom.h is plain C++: tests/host/launch_geom_check.cpp sweeps its width rule against the seven predicates the
sampler launchers used to spell out, exhaustively over sizes and pointer offsets, and asserts what an 8-wide launch needs
for its vector accesses.  Built here with the host compiler under the address and undefined-behaviour sanitizers and run
as a program of its own; no GPU, no HIP."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "inferbiomechanics_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "launch_geom_check.cpp")


def _host_compiler():
    for c in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if c and shutil.which(c):
            return shutil.which(c)
    return None


def test_launch_geom_header_includes_no_hip_header():
    text = open(os.path.join(CSRC, "launch_geom.h")).read()
    assert re.findall(r"#\s*include\s*([<\"][^>\"]+[>\"])", text) == ["<stdint.h>"]
    assert re.findall(r"#\s*include\s*\"([^\"]+)\"", open(SRC).read()) == ["launch_geom.h"]


def test_width_rule_equals_the_seven_it_replaced(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "launch_geom_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, SRC, "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    m = re.search(r"(\d+) combinations checked, all equal", r.stdout)
    assert m and int(m.group(1)) > 1_000_000, r.stdout
