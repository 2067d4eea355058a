"""The coverage of tests/csv_sweep.py's seam planner, asserted without a GPU: every (seam class, motif, byte of the motif,
offset) is visited, every planted byte stands where the plan says, and the seams are the seams of record_csv.h's geometry."""
import csv_cases as cc
import csv_sweep as sw


def test_the_geometries_have_every_seam_class():
    have = {g: sw.seams(*sw.GEOMETRIES[g]) for g in sw.GEOMETRIES}
    assert set(have["one_group"]) == set(sw.SEAM_CLASSES)
    assert set(have["two_groups"]) == {"lane", "wave", "span"}          # every wave one unit: a unit seam is a span seam
    for g, where in have.items():
        unit, grid, n = sw.GEOMETRIES[g]
        assert (unit, sw.GROUP, sw.STEP) == (4096, 16, 1024) and n % unit == 17
        for cls, p in where.items():
            assert sw.seam_class(unit, grid, n, p) == cls
            assert p % 16 == 0 and (p % 1024 == 0) == (cls != "lane") and (p % unit == 0) == (cls in ("unit", "span"))
        cuts = sw.spans(unit, grid, n)
        assert cuts[0] == 0 and cuts[-1] == n and cuts == sorted(set(cuts)) and len(cuts) - 1 <= grid * 4
        assert (where["span"] in cuts) and all(where[c] not in cuts for c in where if c != "span")
        places = sorted(where.values())
        assert all(b - a > 64 for a, b in zip(places, places[1:])) and places[0] > 64 and places[-1] < n - 64
    # three units and 17 bytes on two workgroups: more units than workgroups; nine on one: more than one unit per wave
    assert sw.spans(*sw.GEOMETRIES["two_groups"]) == [0, 4096, 8192, 12288, 12305]
    assert sw.spans(*sw.GEOMETRIES["one_group"]) == [0, 12288, 24576, 36864, 36881]


def test_every_seam_motif_byte_and_offset_is_visited():
    for g in sw.GEOMETRIES:
        unit, grid, n = sw.GEOMETRIES[g]
        where = sw.seams(unit, grid, n)
        seen = set()
        for name, byte, offset, starts in sw.plan(g):
            text = sw.planted(g, name, starts)
            assert len(text) == n
            for cls, start in starts.items():
                at = start + byte
                assert at == where[cls] - 8 + offset and text[start:start + len(sw.MOTIFS[name])] == sw.MOTIFS[name]
                assert text[at] == sw.MOTIFS[name][byte]
                seen.add((cls, name, byte, offset))
        want = {(cls, name, byte, offset) for cls in where for name, m in sw.MOTIFS.items() for byte in range(len(m)) for offset in sw.OFFSETS}
        assert seen == want
        # offset 8 puts the byte on the seam's first byte, offset 7 on the last byte before it
        assert all((cls, name, 0, 8) in seen and (cls, name, len(m) - 1, 7) in seen for cls in where for name, m in sw.MOTIFS.items())


def test_the_filler_is_well_formed_and_the_motifs_mean_what_they_say():
    base = sw.base_text(5000)
    tb = cc.tables(base)
    assert not any(tb["field_flags"]) and tb["stats"]["n_quoted"] == 0 and b"\r\n" in base
    cc.check_against_python(base, tb)
    for name, want in (("quoted_comma", "a,b"), ("escape", 'x"y'), ("quoted_crlf", "\r\n")):
        text = b"k" + sw.MOTIFS[name] + b"z\n"
        tb = cc.tables(text)
        assert cc.values(text, tb) == [["k", want, "z"]] and not any(f & cc.MALFORMED for f in tb["field_flags"])
    assert cc.values(b"k," + sw.MOTIFS["crlf"] + b",z", cc.tables(b"k," + sw.MOTIFS["crlf"] + b",z")) == [["k", "a"], ["b", "z"]]
