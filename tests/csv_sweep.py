"""The seam planner of tests/test_gpu_record_csv.py (its coverage is asserted without a GPU by tests/test_csv_records_plan.py):
small texts in which each byte of each motif falls on, and around, every kind of seam of rj_scan_records_csv's walk.

The walk (rejit_amd/csrc/record_csv.h): a lane takes 16 bytes (GROUP), a wave 64 lanes = 1024 bytes a step (STEP), the text is
cut into units of RJ_CSV_UNIT bytes, and each of the RJ_CSV_GRID x 4 waves owns one contiguous span of ceil(units / waves)
units.  So a text has four kinds of seams: between two lanes, between two steps of a wave, between two units of one span,
and between two spans -- where the next wave, in another workgroup every fourth time, takes over with the entry the resolve
gave it (what a grid-strided walk would call the grid's wrap)."""
GROUP, STEP, WAVES_PER_GROUP = 16, 1024, 4
DEFAULT_UNIT, DEFAULT_GRID = 4096, 2048

# the planted bytes: the motif between the delimiters that make it a field of its own (the line break motif needs none)
MOTIFS = {"quoted_comma": b',"a,b",', "escape": b',"x""y",', "quoted_crlf": b',"\r\n",', "crlf": b"a\r\nb"}
SEAM_CLASSES = ("lane", "wave", "unit", "span")
OFFSETS = range(16)

# (RJ_CSV_UNIT, RJ_CSV_GRID, text length): the issue's three units and 17 bytes on two workgroups -- every wave one unit --
# and nine units and 17 bytes on one workgroup: four spans of three units, so that a unit seam inside a span exists
GEOMETRIES = {"two_groups": (4096, 2, 3 * 4096 + 17), "one_group": (4096, 1, 9 * 4096 + 17)}


def spans(unit, grid, n):
    """the spans' begins and the text's end, as record_csv.h's geometry() cuts them"""
    units = -(-n // unit)
    waves = grid * WAVES_PER_GROUP
    per = -(-units // waves)
    return [min(v * per * unit, n) for v in range(-(-units // per))] + [n]


def seam_class(unit, grid, n, p):
    """what kind of seam lies between bytes p - 1 and p (None: none)"""
    if p <= 0 or p >= n or p % GROUP:
        return None
    if p in spans(unit, grid, n):
        return "span"
    if p % unit == 0:
        return "unit"
    return "wave" if p % STEP == 0 else "lane"


def seams(unit, grid, n):
    """one seam of every class that the geometry has, far from one another: {class: position}"""
    first = lambda cls, lo: next((p for p in range(lo, n - 64, GROUP) if seam_class(unit, grid, n, p) == cls), None)
    out = {"lane": first("lane", 2 * STEP + 3 * GROUP), "wave": first("wave", STEP), "unit": first("unit", unit), "span": first("span", unit)}
    return {k: v for k, v in out.items() if v is not None}


def base_text(n):
    """a well-formed filler: short plain fields, a line break every 61 bytes, a \\r\\n now and then"""
    row = b"abcdef,ghi,jklmnopq,rstuv,wx,yz01234,56789,ABCDEFGHIJ,KLMNOP\n"
    assert len(row) == 61
    text = bytearray((row * (n // len(row) + 1))[:n])
    for at in range(7 * 61 - 2, n - 1, 13 * 61):
        text[at:at + 2] = b"\r\n"
    return bytes(text)


def plan(geometry):
    """-> [(motif, byte, offset, {seam class: the motif's first position})]: byte `byte` of the motif stands at seam - 8 + offset,
    so it is seen on each of the 16 positions around the seam, the seam itself among them"""
    unit, grid, n = GEOMETRIES[geometry]
    where = seams(unit, grid, n)
    out = []
    for name, motif in MOTIFS.items():
        for byte in range(len(motif)):
            for offset in OFFSETS:
                out.append((name, byte, offset, {cls: seam - 8 + offset - byte for cls, seam in where.items()}))
    return out


def planted(geometry, name, starts):
    unit, grid, n = GEOMETRIES[geometry]
    text = bytearray(base_text(n))
    for start in starts.values():
        text[start:start + len(MOTIFS[name])] = MOTIFS[name]
    return bytes(text)
