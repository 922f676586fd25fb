"""Counts per report id (hg_count_records): the plain Python yardstick every counts test uses."""
from collections import Counter, defaultdict


def counts(records):
    """records: (segment, line, id) rows in any order -> {id: (distinct (segment, line), rows)} for the ids that occur."""
    reports, lines = Counter(), defaultdict(set)
    for seg, line, rid in records:
        reports[rid] += 1
        lines[rid].add((seg, line))
    return {rid: (len(lines[rid]), n) for rid, n in reports.items()}
