"""Accept/reject parity of the product's compiler (hg_compile.cpp through tests/native/hostsim.cpp) with the oracle (orx.c).

The oracle refuses an expression that can match the empty string by SYNTAX: every assertion counts as satisfiable, so
`\\b\\B|a` is refused although its empty branch can never match.  The product used to decide the same rule on the exact,
assertion-aware answer and accepted such expressions; nothing noticed, because every randomized harness dropped the sets the
oracle refuses without asking the product.  Here both compilers are asked about every generated case.

Sizes (about 450 expression pairs per second, both compilers, one core; about a minute in all):
  test_random_single_expressions   10 seeds x (1000 random_pattern + 1000 assertion_heavy_pattern) = 20 000 expressions
  test_random_sets                  8 seeds x 150 sets of 2..5 expressions                         =  1 200 sets
Observed with the oracle alone, flag words {14, 15, 10, 6, 12, 2, 7, 4} drawn uniformly:
  random_pattern            9.5 % rejected / 90.5 % accepted (4 000 cases, Random(3))
  assertion_heavy_pattern  16.9 % rejected / 83.1 % accepted (4 000 cases, Random(3))
  a run of test_random_single_expressions (both halves): 11.6 % .. 13.4 % rejected over the ten seeds
  a run of test_random_sets: 16.0 % .. 19.3 % of the sets rejected over the eight seeds
  product-only rejections (capacity limits): 0 of 20 000 expressions, 0 of 1 200 sets
(random_pattern alone falls below 10 % rejected with these eight flag words — five of them are multiline, where embedded
anchors are legal — so a parametrized run draws from both generators and the caps are asserted on the run.)
Before the compiler decided the rule by syntax, 2.5 % of assertion_heavy_pattern's cases (101 of 4 000) and 1 in 4 000 of
random_pattern's were accepted by the product and refused by the oracle, none the other way: 70 of the 72 fixed-list cases
(two of the fuzz-found expressions are refused under flag word 10 for an embedded anchor as well), all ten seeds of
test_random_single_expressions and seeds 0-5 and 7 of test_random_sets failed.
"""
from __future__ import annotations

import random

import pytest

import accept_rules
import hgsim_py
import oracle_py
import regex_gen

FLAG_WORDS = [14, 15, 10, 6, 12, 2, 7, 4]

# empty-matchable by syntax, although no context (or not every context) satisfies the assertions on the empty path
KNOWN = [
    r"\b\B|a", r"(a|\b)\B", r"^\b=*$", r"a*\b\Ba*", r"(\b\B|\d)", r"(z*\B)\b", r"(?:a|^)\B\bz*",
    r"(a|\b\B)", r"(\b|a)\B", r"\b(\B|a)",
]
# found by 35 138 draws of regex_gen.random_pattern(rng); rng.choice([14, 15, 10, 6, 12, 2]) from random.Random(1)
# (draws 1488, 1767, 2880, 13359, 13607, 13644, 25799, 34282)
FOUND_BY_FUZZ = [
    r"_*^($[xyz]|x{1}|\b(z[-=_]9|c y)?)+$",
    r"\b(?:b{3,4}9)*(\b|[xyz](_c|x?|[a-c])*(?:c)){1,}((1| *\-+\d|xy)\S{3,6}.|\B)",
    r"\b([^\n]{2,2}\s+\-?|^)$",
    r"(z0| z|\B)\b",
    r"(\b|z=[-=_]?)\B",
    r"b?z*([a-c0-1_]|\b1*(\B\-*|[a-c0-1_][^a]\s|.)+)$",
    r"(\D*.?)?(={3}9*.|\b^)$",
    r"^^(z? y+|aa|(?:$)\b)$",
]
NEIGHBOURS = ["foo", "ba+r[0-9]"]


@pytest.mark.parametrize("flags", [14, 6, 10, 15])
@pytest.mark.parametrize("pat", KNOWN + FOUND_BY_FUZZ)
def test_syntactically_nullable_expressions_are_rejected(pat, flags):
    assert oracle_py.check_patterns([pat], flags=[flags]) == 4
    db = hgsim_py.Db([pat], [flags])
    assert not db.ok(), "the product accepts what the oracle rejects"
    assert db.error.startswith("0: "), db.error
    assert oracle_py.check_patterns(NEIGHBOURS, flags=[flags] * 2) == 0 and hgsim_py.Db(NEIGHBOURS, [flags] * 2).ok()
    for at in (0, 1, 2):
        pats = NEIGHBOURS[:at] + [pat] + NEIGHBOURS[at:]
        assert oracle_py.check_patterns(pats, flags=[flags] * 3) == 4
        db = hgsim_py.Db(pats, [flags] * 3, [0, 1, 2])
        assert not db.ok(), (pats, "the product accepts what the oracle rejects")
        assert db.error.startswith(f"{at}: "), (pats, db.error)


def _single(gen, rng, tally, failures):
    pat, flags = gen(rng), rng.choice(FLAG_WORDS)
    db = hgsim_py.Db([pat], [flags])
    try:
        tally.decide([pat], [flags], db.ok(), db.error)
    except AssertionError as e:
        failures.append(str(e))


@pytest.mark.parametrize("seed", range(10))
def test_random_single_expressions(seed):
    rng = random.Random(31000 + seed)
    failures = []
    tallies = {}
    for gen in (regex_gen.random_pattern, regex_gen.assertion_heavy_pattern):
        tally = tallies[gen.__name__] = accept_rules.Tally()
        for _ in range(1000):
            _single(gen, rng, tally, failures)
        print(f"seed {seed} {gen.__name__}: {tally.report()}")
    assert not failures, (len(failures), failures[:5])
    generated = sum(t.generated for t in tallies.values())
    rejected = sum(t.oracle_rejected for t in tallies.values())
    product_only = sum(t.product_only_rejected for t in tallies.values())
    assert generated == 2000
    assert rejected >= 0.10 * generated and generated - rejected >= 0.70 * generated, (rejected, generated)
    assert product_only <= 0.01 * generated, {k: t.limits for k, t in tallies.items()}


@pytest.mark.parametrize("seed", range(8))
def test_random_sets(seed):
    """A set is accepted iff each member is accepted alone, and the error names the first member that is not.  (Flag words
    0..15 only: the set-wide rules — shared-id start of match, combinations — are pinned by REJECTION_RULES in
    test_compiler_hostsim.py and by test_comb_host.py.)"""
    rng = random.Random(32000 + seed)
    tally = accept_rules.Tally()
    failures = []
    for _ in range(150):
        k = rng.randint(2, 5)
        gen = rng.choice([regex_gen.random_pattern, regex_gen.assertion_heavy_pattern])
        pats, flags = [], []
        while len(pats) < k:
            p, f = gen(rng), rng.choice(FLAG_WORDS)
            # two in three of the members the oracle refuses are redrawn, so that at least 70 % of the SETS stay legal
            if oracle_py.check_patterns([p], flags=[f]) == 0 or rng.random() < 0.35:
                pats.append(p)
                flags.append(f)
        ids = [rng.randint(0, 2) for _ in range(k)] if rng.random() < 0.5 else list(range(k))
        first_bad = accept_rules.first_rejected(pats, flags)
        db = hgsim_py.Db(pats, flags, ids)
        try:
            assert oracle_py.check_patterns(pats, flags=flags, ids=ids) == (0 if first_bad is None else 4), "the oracle's set decision is not its members'"
            both = tally.decide(pats, flags, db.ok(), db.error)
            if first_bad is not None:
                assert accept_rules.error_index(db.error) == first_bad, f"wrong index: {pats!r} flags {flags}: {db.error} (first rejected member {first_bad})"
            elif not both:  # a member beyond a capacity limit: named by its own index, and refused alone as well
                at = accept_rules.error_index(db.error)
                alone = hgsim_py.Db([pats[at]], [flags[at]])
                assert not alone.ok() and accept_rules.explained_rejection(alone.error), (pats, flags, db.error)
        except AssertionError as e:
            failures.append(str(e))
    print(f"seed {seed}: {tally.report()}")
    assert not failures, (len(failures), failures[:5])
    assert tally.generated == 150
    assert tally.oracle_rejected >= 0.10 * tally.generated and tally.generated - tally.oracle_rejected >= 0.70 * tally.generated, tally.report()
    assert tally.product_only_rejected <= 0.01 * tally.generated, tally.limits


def test_generator_split_with_the_oracle_alone():
    """assertion_heavy_pattern keeps the split the differential needs: at least 10 % rejected, at least 70 % accepted."""
    rng = random.Random(3)
    n = 1500
    rejected = sum(oracle_py.check_patterns([regex_gen.assertion_heavy_pattern(rng)], flags=[rng.choice(FLAG_WORDS)]) != 0 for _ in range(n))
    print(f"assertion_heavy_pattern: {rejected} of {n} rejected by the oracle")
    assert 0.10 * n <= rejected <= 0.30 * n


def test_explained_rejection_knows_the_documented_limits():
    for pats, flags, name in ((["(a{1000}){1000}"], [14], "pattern too large"), (["foo.{0,3000}bar"], [256 | 6], "HG_MAX_NODES")):
        db = hgsim_py.Db(pats, flags)
        assert not db.ok() and accept_rules.explained_rejection(db.error) == name, db.error
    assert accept_rules.explained_rejection("1: expression can match the empty string (HS_FLAG_ALLOWEMPTY is not supported)") is None
    assert accept_rules.explained_rejection("0: embedded start anchors are not supported") is None
    som = "0: HS_FLAG_SOM_LEFTMOST cannot be combined with HS_FLAG_SINGLEMATCH"
    assert accept_rules.explained_rejection(som) is None and accept_rules.explained_rejection(som, features=True) == "som+singlematch"
