#!/usr/bin/env python3
"""Writes rejit_amd/csrc/pow10_table.h: the 128-bit powers of ten that record_format.h's shortest-digits step (Schubfach)
multiplies by (rj_scan_records_format).  Python integers only; no float is touched.

For every k in [-292, 324] one entry of two 64-bit words (high, low), 617 entries, 9 872 bytes:

    g(k) = floor(10^k x 2^-r) + 1,   r = floor(log2(10^k)) - 127,   so that 2^127 <= g(k) < 2^128

ALWAYS rounded up, also where 10^k x 2^-r is an integer (0 <= k <= 55): that is the g the proof of the algorithm assumes
(Giulietti, "The Schubfach way to render doubles", 2020: with 10^k = B 2^r it takes g = floor(B) + 1).  pow5_table.h's entries
are floors for q >= 0, which that proof does not cover, so the format has a table of its own.

usage: gen_pow10_table.py [--check] [path]      writes the header (default: rejit_amd/csrc/pow10_table.h); --check compares it"""
import os
import sys

K_MIN, K_MAX = -292, 324
ENTRIES = K_MAX - K_MIN + 1
MASK64 = (1 << 64) - 1


def power_words(k):
    """-> (high, low): the 128 bits of g(k)"""
    if k >= 0:
        p = 10 ** k
        r = p.bit_length() - 1 - 127              # floor(log2(10^k)) - 127
        g = (p >> r if r >= 0 else p << -r) + 1
    else:
        p = 10 ** -k
        # floor(log2(10^k)) = -ceil(log2(10^-k)) = -bit_length(10^-k): 10^-k is no power of two
        r = -p.bit_length() - 127
        g = (1 << -r) // p + 1
    assert (1 << 127) <= g < (1 << 128)
    return g >> 64, g & MASK64


def table():
    return [power_words(k) for k in range(K_MIN, K_MAX + 1)]


def header_text():
    lines = ["// rejit_amd/csrc/pow10_table.h -- WRITTEN BY tools/gen_pow10_table.py; do not edit (tests/test_record_format.py regenerates",
             "// it and compares every word).  The 128-bit powers of ten of record_format.h's shortest-digits step: entry k - kPow10MinK",
             "// holds (high, low) of g(k) = floor(10^k x 2^-r) + 1, r = floor(log2(10^k)) - 127 -- rounded up for EVERY k.",
             "#ifndef REJIT_AMD_POW10_TABLE_H_",
             "#define REJIT_AMD_POW10_TABLE_H_",
             "",
             "#include <stdint.h>",
             "",
             "namespace rejit_amd {",
             "namespace numformat {",
             "",
             "constexpr int kPow10MinK = %d, kPow10MaxK = %d, kPow10Entries = %d;" % (K_MIN, K_MAX, ENTRIES),
             "",
             "#if defined(__HIP_DEVICE_COMPILE__)",
             "__device__",
             "#endif",
             "    const uint64_t kPow10[2 * kPow10Entries] = {"]
    for hi, lo in table():
        lines.append("        0x%016xull, 0x%016xull," % (hi, lo))
    lines += ["};", "", "}  // namespace numformat", "}  // namespace rejit_amd", "#endif", ""]
    return "\n".join(lines)


def main(argv):
    check = "--check" in argv
    paths = [a for a in argv if a != "--check"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = paths[0] if paths else os.path.join(root, "rejit_amd", "csrc", "pow10_table.h")
    text = header_text()
    if check:
        with open(path) as fh:
            if fh.read() != text:
                sys.exit("%s differs from what tools/gen_pow10_table.py writes" % path)
        return
    with open(path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
