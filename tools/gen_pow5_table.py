#!/usr/bin/env python3
"""Writes rejit_amd/csrc/pow5_table.h: the 128-bit truncated powers of five that record_parse.h's Eisel-Lemire product reads
(RJ_PARSE_WIDE).  Python integers only; no float is touched.

For every q in [-342, 308] one entry of two 64-bit words (high, low), 651 entries, 10 416 bytes:

    q >= 0   floor of 5^q normalised to 128 bits: 5^q shifted until its top bit is bit 127, the bits below bit 0 dropped
    q <  0   2^b / 5^-q + 1, truncated to 128 bits; with 2^(z - 1) < 5^-q < 2^z, b = z + 127 for q >= -27 (the quotient has its
             128 bits at once) and b = 2 z + 128 below (halved until 128 bits are left): the reciprocal is rounded UP, which is
             what the proof that no fallback is needed assumes of the table

(Mushtak and Lemire, "Fast Number Parsing Without Fallback", 2023; Lemire, "Number Parsing at a Gigabyte per Second", 2021.)

usage: gen_pow5_table.py [--check] [path]      writes the header (default: rejit_amd/csrc/pow5_table.h); --check compares it"""
import os
import sys

Q_MIN, Q_MAX = -342, 308
ENTRIES = Q_MAX - Q_MIN + 1
MASK64 = (1 << 64) - 1


def power_words(q):
    """-> (high, low): the 128 bits of the table's entry for 10^q = 5^q x 2^q"""
    if q >= 0:
        c = 5 ** q
        while c < (1 << 127):
            c <<= 1
        while c >= (1 << 128):
            c >>= 1
    else:
        p = 5 ** -q
        z = p.bit_length()                       # 2^(z - 1) < 5^-q < 2^z
        if q >= -27:                             # 5^-q fits 64 bits: b = z + 127 gives the 128 bits at once
            c = (1 << (z + 127)) // p + 1
        else:
            c = (1 << (2 * z + 128)) // p + 1
            while c >= (1 << 128):
                c >>= 1
    assert (1 << 127) <= c < (1 << 128)
    return c >> 64, c & MASK64


def table():
    return [power_words(q) for q in range(Q_MIN, Q_MAX + 1)]


def header_text():
    lines = ["// rejit_amd/csrc/pow5_table.h -- WRITTEN BY tools/gen_pow5_table.py; do not edit (tests/test_record_parse_wide.py regenerates",
             "// it and compares every word).  The 128-bit truncated powers of five of record_parse.h's Eisel-Lemire product: entry",
             "// q - kPow5MinQ holds (high, low) of 5^q normalised to 128 bits -- the floor for q >= 0, 2^b / 5^-q + 1 truncated for q < 0.",
             "#ifndef REJIT_AMD_POW5_TABLE_H_",
             "#define REJIT_AMD_POW5_TABLE_H_",
             "",
             "#include <stdint.h>",
             "",
             "namespace rejit_amd {",
             "namespace numparse {",
             "",
             "constexpr int kPow5MinQ = %d, kPow5MaxQ = %d, kPow5Entries = %d;" % (Q_MIN, Q_MAX, ENTRIES),
             "",
             "#if defined(__HIP_DEVICE_COMPILE__)",
             "__device__",
             "#endif",
             "    const uint64_t kPow5[2 * kPow5Entries] = {"]
    for hi, lo in table():
        lines.append("        0x%016xull, 0x%016xull," % (hi, lo))
    lines += ["};", "", "}  // namespace numparse", "}  // namespace rejit_amd", "#endif", ""]
    return "\n".join(lines)


def main(argv):
    check = "--check" in argv
    paths = [a for a in argv if a != "--check"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = paths[0] if paths else os.path.join(root, "rejit_amd", "csrc", "pow5_table.h")
    text = header_text()
    if check:
        with open(path) as fh:
            if fh.read() != text:
                sys.exit("%s differs from what tools/gen_pow5_table.py writes" % path)
        return
    with open(path, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main(sys.argv[1:])
