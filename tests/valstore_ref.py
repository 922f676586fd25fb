"""Plain Python reference of the value store (hg_accumulate_values, hg_rank_accumulated; include/hypergrep_amd.h): matched
values accumulated over many scans.  Nothing here is shared with the stage: a dict from key to [first ordinal, count, pattern,
line] over the calls' part lists, one after the other, and the ranking's sort and cut."""
from __future__ import annotations


class Store:
    def __init__(self, by_pattern: bool = False):
        self.by_pattern = by_pattern
        self.table = {}
        self.n_parts = 0

    def add(self, text: bytes, parts, starts, seg_start=None):
        """One call: parts are (line, from, to, pattern[, segment]) rows in the scan's order, starts {(segment, line): start of the
        piece's record}, seg_start the files' offsets after a scan with segments.  A part whose piece has no record is not
        counted, but has an ordinal.  Returns the number of values the call added."""
        before = len(self.table)
        for q, p in enumerate(parts):
            seg = p[4] if len(p) > 4 else 0
            start = starts.get((seg, p[0]))
            if start is None:
                continue
            src = (seg_start[seg] if seg_start is not None else 0) + start + p[1]
            value = text[src:src + p[2] - p[1]]
            assert len(value) == p[2] - p[1] > 0
            key = (p[3], value) if self.by_pattern else value
            if key in self.table:
                self.table[key][1] += 1
            else:
                self.table[key] = [self.n_parts + q, 1, p[3], p[0]]
        self.n_parts += len(parts)
        return len(self.table) - before

    def rows(self, top: int = 0, order_first: bool = False):
        """The ranking: dicts {value, count, first, pattern, line_number} by (count descending, first), or by first alone, cut
        to the first `top` (0: all)."""
        out = [{"value": k[1] if self.by_pattern else k, "first": v[0], "count": v[1], "pattern": v[2], "line_number": v[3]} for k, v in self.table.items()]
        out.sort(key=(lambda r: r["first"]) if order_first else (lambda r: (-r["count"], r["first"])))
        return out[:top] if top else out


def arrays(rows):
    """The rows as the stage's arrays (lists), for one comparison per array."""
    off = [0]
    for r in rows:
        off.append(off[-1] + len(r["value"]))
    return {"bytes": b"".join(r["value"] for r in rows), "off": off, "count": [r["count"] for r in rows], "first": [r["first"] for r in rows],
            "pattern": [r["pattern"] for r in rows], "line_number": [r["line_number"] for r in rows]}


def ranked(rows, by_pattern: bool = False):
    """hypergrep_amd.count_values_top's rows: (value, count) or (value, pattern, count), by count descending, then value (then pattern)."""
    if by_pattern:
        return sorted(((r["value"], r["pattern"], r["count"]) for r in rows), key=lambda r: (-r[2], r[0], r[1]))
    return sorted(((r["value"], r["count"]) for r in rows), key=lambda r: (-r[1], r[0]))
