"""Plain Python reference of the rank stage (hg_rank_values, include/hypergrep_amd.h): the matched parts grouped by (segment,
[pattern,] bytes), ordered by segment, descending count and first occurrence, and cut to the `top` first groups of the scan or of
every segment.  Nothing here is shared with the stage: a dict from key to [first, count], a sort and a slice."""
from __future__ import annotations

import values_ref as vr


def ranking(text: bytes, parts, starts, by_pattern: bool = False, per_segment: bool = False, top: int = 0, seg_start=None, n_seg: int = 0):
    """(rows, per-segment arrays or None, n_distinct).  parts: (line, from, to, pattern[, segment]) rows in the scan's order;
    starts: {(segment, line): start of the piece's record}; seg_start: the files' offsets after a scan with segments.  rows:
    dicts {value, count, first, pattern, line_number, segment} in the stage's order, after the cut."""
    table = {}
    for q, (p, s) in enumerate(zip(parts, vr.spans(parts, starts, seg_start))):
        if s is None:
            continue
        value = text[s[0]:s[0] + s[1]]
        assert len(value) == s[1] > 0
        seg = p[4] if len(p) > 4 else 0
        key = (seg if per_segment else 0, p[3] if by_pattern else 0, value)
        if key in table:
            table[key][1] += 1
        else:
            table[key] = [q, 1]
    groups = sorted(((key[0], -count, first, key[2]) for key, (first, count) in table.items()))
    rows, seg_arrays = [], None
    n_groups = n_seg if per_segment else 1
    first_value, distinct, seg_parts = [0], [], []
    for s in range(n_groups):
        mine = [g for g in groups if g[0] == s]
        distinct.append(len(mine))
        seg_parts.append(sum(-g[1] for g in mine))
        kept = mine[:top] if top else mine
        for _s, neg, first, value in kept:
            p = parts[first]
            rows.append({"value": value, "count": -neg, "first": first, "pattern": p[3], "line_number": p[0], "segment": p[4] if len(p) > 4 else 0})
        first_value.append(len(rows))
    if per_segment:
        seg_arrays = {"first_value": first_value, "seg_distinct": distinct, "seg_parts": seg_parts}
    return rows, seg_arrays, len(groups)


def arrays(rows, segments: bool = False):
    """The rows as the stage's arrays (lists), for one comparison per array."""
    return vr.arrays(rows, segments=segments)
