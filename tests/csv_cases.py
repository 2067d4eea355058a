"""What the tests of rj_scan_records_csv expect (tests/test_record_csv.py, tests/test_gpu_record_csv.py): the rule of
include/rejit_hip.h restated byte by byte in Python -- no masks, no groups, no units, independent of the library --, the same
rule with numpy for well-formed texts of megabytes, Python's csv as the outside reference, and the builders of the cases."""
import csv
import io
import random

ESCAPED, BAD_QUOTE, BAD_CLOSE, BARE_CR, OPEN = 1, 2, 4, 8, 16
MALFORMED = BAD_QUOTE | BAD_CLOSE | BARE_CR | OPEN
NONE = (1 << 64) - 1
STATS = ("n_rows", "n_fields", "n_quoted", "n_escapes", "n_bad_quote", "n_bad_close", "n_bare_cr", "open_at_end", "first_bad")


def tables(t, d=44, q=34):
    """-> dict: row_first, row_begin, row_end, field_begin, field_end, field_flags (lists) and stats (dict; first_bad NONE: none)"""
    t = bytes(t)
    n = len(t)
    ins = [0] * (n + 1)
    for p in range(n):
        ins[p + 1] = ins[p] ^ (1 if q is not None and t[p] == q else 0)
    out = {k: [] for k in ("row_begin", "row_end", "field_begin", "field_end", "field_flags")}
    out["row_first"] = [0]
    st = dict.fromkeys(STATS, 0)
    bad_at = []
    fb, rb, flags = 0, 0, 0

    def close(fe, last):
        begin = fb + 1 if (q is not None and fb < fe and t[fb] == q) else fb
        is_open = last and ins[n] == 1
        end = fe - 1 if (q is not None and fe > begin and t[fe - 1] == q and not is_open) else fe
        out["field_begin"].append(begin)
        out["field_end"].append(end)
        out["field_flags"].append(flags | (OPEN if is_open else 0))
        st["n_quoted"] += begin != fb

    for p in range(n):
        c = t[p]
        if q is not None and c == q:
            if ins[p] == 0:
                if p != fb and t[p - 1] == q:
                    flags |= ESCAPED
                    st["n_escapes"] += 1
                elif p != fb:
                    flags |= BAD_QUOTE
                    st["n_bad_quote"] += 1
                    bad_at.append(p)
            else:
                follows = t[p + 1:p + 3]
                if not (p + 1 == n or follows[0] in (d, 10, q) or follows == b"\r\n"):
                    flags |= BAD_CLOSE
                    st["n_bad_close"] += 1
                    bad_at.append(p)
        if c == 13 and ins[p] == 0 and t[p + 1:p + 2] != b"\n":
            flags |= BARE_CR
            st["n_bare_cr"] += 1
            bad_at.append(p)
        if ins[p] == 0 and c in (d, 10):
            fe = p - 1 if (c == 10 and p > fb and t[p - 1] == 13) else p
            close(fe, False)
            fb, flags = p + 1, 0
            if c == 10:
                out["row_begin"].append(rb)
                out["row_end"].append(fe)
                out["row_first"].append(len(out["field_begin"]))
                rb = p + 1
    if n and not (t[n - 1] == 10 and ins[n - 1] == 0):
        close(n, True)
        out["row_begin"].append(rb)
        out["row_end"].append(n)
        out["row_first"].append(len(out["field_begin"]))
    st["n_rows"], st["n_fields"] = len(out["row_begin"]), len(out["field_begin"])
    st["open_at_end"] = ins[n]
    st["first_bad"] = min(bad_at) if bad_at else (n if ins[n] else NONE)
    out["stats"] = st
    return out


def rows_of(tb):
    """the fields of every row: [[(begin, end, flags), ...], ...]"""
    f = list(zip(tb["field_begin"], tb["field_end"], tb["field_flags"]))
    return [f[a:b] for a, b in zip(tb["row_first"], tb["row_first"][1:])]


def value(t, field, q=34):
    begin, end, flags = field
    v = bytes(t[begin:end])
    return v.replace(bytes([q, q]), bytes([q])) if flags & ESCAPED else v


def values(t, tb, q=34):
    return [[value(t, f, q).decode("latin-1") for f in row] for row in rows_of(tb)]


def python_rows(t, d=44, q=34):
    """-> (rows of csv.reader(strict=True) up to its first error, [] read as [''], the error or None)"""
    out = []
    kw = {"quoting": csv.QUOTE_NONE} if q is None else {"quotechar": chr(q)}
    try:
        for r in csv.reader(io.StringIO(bytes(t).decode("latin-1"), newline=""), strict=True, delimiter=chr(d), **kw):
            out.append(r or [""])
    except csv.Error as e:
        return out, str(e)
    return out, None


def check_against_python(t, tb, d=44, q=34):
    """claims (a) and (b) of the header: no MALFORMED flag -> Python's rows exactly; else every row before the first flagged one"""
    mine = values(t, tb, 34 if q is None else q)
    flagged = [any(f[2] & MALFORMED for f in row) for row in rows_of(tb)]
    theirs, err = python_rows(t, d, q)
    k = flagged.index(True) if any(flagged) else len(mine)
    if k == len(mine):
        assert err is None and theirs == mine, (bytes(t), mine, theirs, err)
    else:
        assert theirs[:k] == mine[:k], (bytes(t), k, mine, theirs, err)


def tables_numpy(t, d=44, q=34):
    """the rule for a WELL-FORMED text (no MALFORMED flag: asserted), vectorised: dict of numpy int64 arrays row_first, row_begin,
    row_end, field_begin, field_end, field_flags"""
    import numpy as np

    a = np.frombuffer(bytes(t), dtype=np.uint8)
    n = a.size
    assert n > 0
    isq = (a == q) if q is not None else np.zeros(n, dtype=bool)
    ins = np.concatenate(([0], np.cumsum(isq)))[:-1] & 1                 # ins(p)
    assert (int(isq.sum()) & 1) == 0
    prev = np.concatenate(([0], a[:-1])).astype(np.int64)
    prev[0] = -1
    nxt = np.concatenate((a[1:], [0])).astype(np.int64)
    nxt[-1] = -1
    nl = (a == 10) & (ins == 0)
    s = ((a == d) & (ins == 0)) | nl
    pos = np.nonzero(s)[0]
    tail = not bool(nl[-1])
    fbs = np.concatenate(([0], pos + 1))                                # raw begins (the last one may be n)
    if not tail:
        fbs = fbs[:-1]
    crlf = nl[pos] & (prev[pos] == 13)
    fes = pos - crlf
    if tail:
        fes = np.concatenate((fes, [n]))
    begin = fbs + ((fbs < n) & (a[np.minimum(fbs, n - 1)] == (q if q is not None else -1)) & (fbs < fes))
    end = fes - ((fes > begin) & (a[np.maximum(fes, 1) - 1] == (q if q is not None else -1)))
    at_begin = np.zeros(n, dtype=bool)
    at_begin[fbs[fbs < n]] = True
    esc = isq & (ins == 0) & ~at_begin & (prev == (q if q is not None else -1))
    assert not (isq & (ins == 0) & ~at_begin & ~esc).any(), "a bad quote"
    assert not ((a == 13) & (ins == 0) & (nxt != 10)).any(), "a bare \\r"
    ok_close = (nxt == -1) | (nxt == d) | (nxt == 10) | (nxt == (q if q is not None else -1)) | ((nxt == 13) & (np.concatenate((a[2:], [0, 0])) == 10))
    assert not (isq & (ins == 1) & ~ok_close).any(), "a bad close"
    field_of = np.cumsum(s) - s                                         # structural bytes before p
    flags = np.zeros(fbs.size, dtype=np.int64)
    flags[field_of[esc]] = ESCAPED
    rows_at = np.nonzero(nl)[0]
    row_first = np.concatenate(([0], field_of[rows_at] + 1))
    row_begin = np.concatenate(([0], rows_at + 1))
    row_end = rows_at - (prev[rows_at] == 13)
    if tail:
        row_first = np.concatenate((row_first, [fbs.size]))
        row_end = np.concatenate((row_end, [n]))
    else:
        row_begin = row_begin[:-1]
    return {"row_first": row_first.astype(np.int64), "row_begin": row_begin.astype(np.int64), "row_end": row_end.astype(np.int64),
            "field_begin": begin.astype(np.int64), "field_end": end.astype(np.int64), "field_flags": flags}


# ------------------------------------------------------------------------------------------------------------------ builders
def small_texts(alphabet=b'a",\n\r', upto=6):
    """every text of up to `upto` bytes over the alphabet"""
    import itertools

    for length in range(upto + 1):
        for t in itertools.product(alphabet, repeat=length):
            yield bytes(t)


def random_texts(count, seed, alphabet=b'ab"\t\t\n\n\r",', lo=8, hi=28):
    rng = random.Random(seed)
    for _ in range(count):
        yield bytes(rng.choice(alphabet) for _ in range(rng.randint(lo, hi)))


FIELD_KINDS = ("plain", "number", "comma", "break", "escape", "empty", "empty_quoted", "quoted", "crlf_inside")


def field_text(kind, rng, d=b","):
    word = lambda: bytes(rng.choice(b"abcdefghij xyz") for _ in range(rng.randint(1, 9)))
    if kind == "plain":
        return word(), None
    if kind == "number":
        v = str(rng.randint(-99999, 99999)).encode()
        return (b'"' + v + b'"', v) if rng.random() < 0.3 else (v, v)
    inner = {"comma": lambda: word() + d + word(), "break": lambda: word() + b"\n" + word(), "escape": lambda: word() + b'"' + word() + b'"' * rng.randint(0, 2),
             "empty": lambda: None, "empty_quoted": lambda: b"", "quoted": word, "crlf_inside": lambda: word() + b"\r\n" + word()}[kind]()
    if inner is None:
        return b"", b""
    return b'"' + inner.replace(b'"', b'""') + b'"', inner


def generated(n_rows, seed, n_cols=6, d=b",", crlf_every=3, final_break=True, kinds=FIELD_KINDS):
    """-> (text, values): a well-formed CSV with every kind of field; values[r][c] as bytes; every crlf_every-th row ends in \\r\\n"""
    rng = random.Random(seed)
    parts, vals = [], []
    for r in range(n_rows):
        row, rv = [], []
        for c in range(n_cols):
            kind = kinds[(r + c * 5 + rng.randrange(len(kinds))) % len(kinds)]
            raw, v = field_text(kind, rng, d)
            row.append(raw)
            rv.append(raw if v is None else v)
        parts.append(d.join(row))
        parts.append(b"\r\n" if crlf_every and r % crlf_every == crlf_every - 1 else b"\n")
        vals.append(rv)
    if not final_break:
        parts.pop()
    return b"".join(parts), vals


def plant(text, at, what):
    """the text with the bytes `what` written over those at `at`"""
    return text[:at] + what + text[at + len(what):]
