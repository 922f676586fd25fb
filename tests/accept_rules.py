"""Which expressions are legal: the oracle's decision, and the product's documented reasons for refusing what the oracle takes.

Shared by the tests and tools/fuzz_*.py that draw random expressions.  A randomized harness must not drop a set one compiler
refuses without asking the other: `Tally.decide` asserts the two decisions agree before the caller skips the set.

The oracle knows the flag bits 0..15 only; feature flags of the product (HS_FLAG_SOM_LEFTMOST ...) are masked off before it
is asked, and the product may then refuse for a documented rule of that feature (FEATURE_RULES).
"""
from __future__ import annotations

import re

import oracle_py

ORACLE_FLAG_MASK = 15

# (name, fragment of the CompileError text in hypergrep_amd/csrc/hg_compile.cpp): sizes the product bounds more tightly than
# the oracle (orx.c bounds an expression by ORX_MAX_INST = 400000 instructions only)
CAPACITY_LIMITS = [
    ("pattern too large", "pattern too large"),  # HG_HUGE_MAX_NODES positions / nodes, HG_HUGE_MAX_EDGES, HG_HUGE_MAX_PROGRAM
    ("pattern set too large", "pattern set too large"),
    ("HG_MAX_NODES", "nodes (HG_MAX_NODES)"),  # start of match, approximate matching: automata of at most 1024 nodes
]
# rules of features the oracle does not have (hg_compile.cpp, hg_hsface.hip)
FEATURE_RULES = [
    ("som+singlematch", "HS_FLAG_SOM_LEFTMOST cannot be combined with HS_FLAG_SINGLEMATCH"),
    ("som shared id", "must all carry HS_FLAG_SOM_LEFTMOST, or none of them"),
    ("stream positions", "positions, too large for stream mode"),
    ("stream som positions", "positions, too large for start of match in stream mode"),
    ("stream min_length", "min_length that can remove reports is not supported in stream mode"),
]
_INDEX = re.compile(r"^(?:-?\d+: |expression \d+: )")


def oracle_accepts(pats, flags) -> bool:
    return oracle_py.check_patterns(list(pats), flags=[f & ORACLE_FLAG_MASK for f in flags]) == 0


def first_rejected(pats, flags):
    """Index of the first expression the oracle refuses on its own, or None."""
    for i, (p, f) in enumerate(zip(pats, flags)):
        if not oracle_accepts([p], [f]):
            return i
    return None


def explained_rejection(error_text, features: bool = False):
    """Name of the documented capacity limit (or, with `features`, feature rule) the product's error text states, or None."""
    text = _INDEX.sub("", error_text or "")
    for name, fragment in CAPACITY_LIMITS + (FEATURE_RULES if features else []):
        if fragment in text:
            return name
    return None


def error_index(error_text):
    """The expression index a host harness's error text starts with ("<index>: message"), or None."""
    m = re.match(r"^(-?\d+): ", error_text or "")
    return int(m.group(1)) if m else None


class Tally:
    """generated / oracle_rejected / product_only_rejected / done of one randomized run."""

    def __init__(self):
        self.generated = self.oracle_rejected = self.product_only_rejected = self.done = 0
        self.limits: dict = {}

    def decide(self, pats, flags, product_ok: bool, error_text, features: bool = False) -> bool:
        """Asserts the product's decision on the set equals the oracle's (a product-only rejection must state a documented
        limit) and counts it; True when both accept, i.e. the caller goes on to scan."""
        self.generated += 1
        if not oracle_accepts(pats, flags):
            self.oracle_rejected += 1
            assert not product_ok, f"the oracle rejects what the product accepts: {list(pats)!r} flags {list(flags)}"
            return False
        if not product_ok:
            why = explained_rejection(error_text, features)
            assert why, f"the product rejects what the oracle accepts, without a documented limit: {list(pats)!r} flags {list(flags)}: {error_text}"
            self.product_only_rejected += 1
            self.limits[why] = self.limits.get(why, 0) + 1
            return False
        return True

    def accepts(self, compile_one, features: bool = False):
        """accepts(pattern, flags) for regex_gen.end_offset_cases: compile_one(pattern, flags) returns the product's
        (ok, error text); the decision is compared with the oracle's before the case is kept or dropped."""
        return lambda p, f: self.decide([p], [f], *compile_one(p, f), features=features)

    def report(self) -> str:
        return (f"generated {self.generated} oracle_rejected {self.oracle_rejected} product_only_rejected {self.product_only_rejected} "
                f"{self.limits or ''} done {self.done}")
