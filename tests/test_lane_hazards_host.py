"""CPU: the overlap lane's hazard tracker (csrc/aeth_lane_hazards.h) -- which launches may run beside each other, decided
from the byte ranges they touch.  The header is free of HIP, so tests/cpp/lane_hazards_sanitize.cpp, a stand-alone
program, is built with plain g++ under -fsanitize=address,undefined and run: the three hazard kinds, ranges that touch
without overlapping, the refresh of an equal record, a full lane reporting "join" without dropping a record, and reset."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "lane_hazards_sanitize.cpp")
INC = os.path.join(ROOT, "aether_primitives_amd", "csrc")
OUT = os.path.join(ROOT, "tests", "cpp", "build")


def test_lane_hazards_under_asan_ubsan():
    os.makedirs(OUT, exist_ok=True)
    exe = os.path.join(OUT, "lane_hazards_address")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", INC, SRC, "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert p.returncode == 0 and "lane_hazards: ok" in p.stdout, p.stdout + p.stderr
    assert "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr


def test_the_library_uses_this_tracker():
    """the lane protocol consults the tested header and nothing else for its hazards"""
    rt = open(os.path.join(INC, "aeth_runtime.hip")).read()
    assert '#include "aeth_lane_hazards.h"' in open(os.path.join(INC, "aeth_internal.h")).read()
    assert "hazards.hazards(" in rt and "hazards.note(" in rt and "ranges_touch(" not in rt
