"""CPU test of rejit_amd/csrc/plane_network.h: the nine three-input operations that answer "at most one of the window's eight
codes differs from the base" in the plane kernels (plane_count.hip), and the join of a piece's four code bytes.  Off the device
the header evaluates every operation bit by bit from the very truth-table constant the kernel hands to v_bitop3_b32, so the
stand-alone program tests/support/plane_network_exec.cc checks the immediates themselves: all 256 inputs per bit position
against "at most one zero", on words whose 32 bit positions hold 32 different inputs, and codes16 for every code_shift 0..6
against the per-byte definition.  The program is built with the address and undefined sanitizers (their runtimes linked
statically: nothing is preloaded, and nothing is loaded into Python)."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "support", "plane_network_exec.cc")
HEADER = os.path.join(ROOT, "rejit_amd", "csrc", "plane_network.h")
EXE = os.path.join(HERE, "support", "plane_network_exec_asan")


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(out) < os.path.getmtime(d) for d in (SRC, HEADER))


def test_the_network_and_the_join_against_their_definitions():
    if _stale(EXE):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan", "-o", EXE, SRC])
    r = subprocess.run([EXE], capture_output=True, timeout=120)
    out = r.stdout.decode()
    assert r.returncode == 0, (out[-1000:], r.stderr.decode()[-2000:])
    m = re.search(r"checked (\d+) cases\s*$", out)
    # 256 uniform words + 8 in order + 64 x 8 shuffled, 64 x 5 tables, 7 shifts x 2000 pieces
    assert m and int(m.group(1)) == 256 + 8 + 512 + 320 + 14000, out[-400:]

