"""Plain Python reference of the values stage (hg_count_values, include/hypergrep_amd.h): the matched parts grouped by their
bytes.  Nothing here is shared with the stage: a dict from key to [first, count] over a list of parts and the text."""
from __future__ import annotations


def spans(parts, starts, seg_start=None):
    """(src, length) per part, None for a part whose piece has no record.  parts: (line, from, to, pattern[, segment]) rows in
    the scan's order; starts: {(segment, line): start of the piece's record}; seg_start: the files' offsets after segments."""
    out = []
    for p in parts:
        seg = p[4] if len(p) > 4 else 0
        start = starts.get((seg, p[0]))
        out.append(None if start is None else ((seg_start[seg] if seg_start is not None else 0) + start + p[1], p[2] - p[1]))
    return out


def groups(text: bytes, parts, starts, by_pattern: bool = False, seg_start=None):
    """The stage's result: a list of dicts {value, count, first, pattern, line_number, segment} ordered by first."""
    table = {}
    for q, (p, s) in enumerate(zip(parts, spans(parts, starts, seg_start))):
        if s is None:
            continue
        value = text[s[0]:s[0] + s[1]]
        assert len(value) == s[1] > 0
        key = (p[3], value) if by_pattern else value
        if key in table:
            table[key][1] += 1
        else:
            table[key] = [q, 1]
    out = []
    for key, (first, count) in sorted(table.items(), key=lambda kv: kv[1][0]):
        p = parts[first]
        out.append({"value": key[1] if by_pattern else key, "count": count, "first": first, "pattern": p[3], "line_number": p[0], "segment": p[4] if len(p) > 4 else 0})
    return out


def arrays(rows, segments: bool = False):
    """The rows as the stage's arrays (lists), for one comparison per array."""
    off = [0]
    for r in rows:
        off.append(off[-1] + len(r["value"]))
    return {"bytes": b"".join(r["value"] for r in rows), "off": off, "count": [r["count"] for r in rows], "first": [r["first"] for r in rows],
            "pattern": [r["pattern"] for r in rows], "line_number": [r["line_number"] for r in rows], "segment": [r["segment"] for r in rows] if segments else None}


def ranked(rows, by_pattern: bool = False):
    """hypergrep_amd.count_values' rows: (value, count) or (value, pattern, count), by count descending, then value (then pattern)."""
    if by_pattern:
        return sorted(((r["value"], r["pattern"], r["count"]) for r in rows), key=lambda r: (-r[2], r[0], r[1]))
    return sorted(((r["value"], r["count"]) for r in rows), key=lambda r: (-r[1], r[0]))
