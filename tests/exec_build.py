"""What the CPU tests of the record headers (tests/test_record_*.py) share: the build of a test-only driver
tests/support/<name>.cc with g++ -- as a shared library for ctypes, and as a stand-alone program under the address and
undefined-behaviour sanitizers -- rebuilt when the driver or one of the headers it includes is newer, and the ctypes array
the tests hand their tables over in."""
import ctypes
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SUPPORT = os.path.join(HERE, "support")
CSRC = os.path.join(os.path.dirname(HERE), "rejit_amd", "csrc")


def headers(csrc=(), support=()):
    """-> the paths of headers of rejit_amd/csrc and of tests/support: a module's DEPS"""
    return [os.path.join(CSRC, h) for h in csrc] + [os.path.join(SUPPORT, h) for h in support]


def _arr(xs, ty=ctypes.c_uint64):
    return (ty * max(len(xs), 1))(*xs)


def _stale(target, deps):
    return not os.path.exists(target) or any(os.path.getmtime(target) < os.path.getmtime(s) for s in deps)


def shared_driver(name, deps):
    """tests/support/<name>.cc as tests/support/lib<name>.so, loaded"""
    src, so = os.path.join(SUPPORT, name + ".cc"), os.path.join(SUPPORT, "lib" + name + ".so")
    if _stale(so, [src] + deps):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, src])
    return ctypes.CDLL(so)


def sanitized_program(name, deps):
    """tests/support/<name>.cc with its own main() (-D<NAME>_MAIN) as tests/support/<name>_asan -> its path.  The sanitizers'
    runtimes are linked statically: the program is run directly, nothing is preloaded."""
    src, exe = os.path.join(SUPPORT, name + ".cc"), os.path.join(SUPPORT, name + "_asan")
    if _stale(exe, [src] + deps):
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               "-static-libasan", "-static-libubsan", "-D" + name.upper() + "_MAIN", "-o", exe, src])
    return exe
