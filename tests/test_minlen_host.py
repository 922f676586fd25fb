"""min_length (hs_expr_ext_t) on the host: the compiler's acceptance rules through every compile entry point, and the
match-length filter in its place before the report rules (hg_som.h replayed through tests/native/minlensim.cpp) against a
Python `re` brute force.  No GPU needed."""
from __future__ import annotations

import pytest

import accept_rules
import extsim_py
import minlensim_py
import regex_gen
import somsim_py
from minlensim_py import COMBINATION, QUIET, SINGLE, SOM, expected_piece, ext, exts_for, spans

HS_MODE_BLOCK, HS_MODE_STREAM = 1, 2
STREAM_RULE = "min_length that can remove reports is not supported in stream mode"

# (expression, ext, the rule's words in the message)
REJECTIONS = [
    ("foobar", ext(edit=1, min_length=6), ["min_length 6 could remove reports"]),
    ("foo[a-z]{2,}bar", ext(hamming=1, min_length=9), ["min_length 9 could remove reports"]),
    ("foobar", ext(min_length=7), ["min_length 7 could remove reports", "no match of the expression can be that long"]),
    ("foo[0-9]{1,3}bar", ext(min_length=10), ["min_length 10 could remove reports", "no match of the expression can be that long"]),
    ("foo[a-z]*bar", ext(min_length=2**31), ["min_length 2147483648 could remove reports", "no match of the expression can be that long"]),
    ("foo.{0,3000}bar", ext(min_length=100), ["min_length 100 could remove reports", "1024", "HG_MAX_NODES"]),
]


def _hg(pats, flags, exts):
    from hypergrep_amd import device

    try:
        device.Database(pats, flags=flags, ids=list(range(len(pats))), ext=exts)
    except device.CompileError as e:
        return str(e)
    return None


def _hs(pats, flags, exts, mode):
    from hypergrep_amd import device

    h, err = device.hs_compile(pats, flags, list(range(len(pats))), exts, mode)
    if err is None:
        device.face_a().hs_free_database(h)
        return None
    return f"{err[1]}: {err[0]}"


@pytest.mark.parametrize("expr,x,words", REJECTIONS, ids=[f"{i}-{r[2][-1]}" for i, r in enumerate(REJECTIONS)])
def test_rejections_name_the_expression_and_the_rule(expr, x, words):
    import hypergrep_amd

    pats, flags, exts = ["hello", "world", expr], [0, 0, 0], [None, None, x]  # the bad expression is index 2
    msgs = {"hg": _hg(pats, flags, exts), "hs block": _hs(pats, flags, exts, HS_MODE_BLOCK), "hs stream": _hs(pats, flags, exts, HS_MODE_STREAM)}
    for name, msg in msgs.items():
        assert msg is not None and msg.startswith("2: "), (name, msg)
        for w in words:
            assert w in msg, (name, msg)
    assert hypergrep_amd.check_compatibility(pats, flags=flags, ids=[0, 1, 2], ext=exts) == 4
    assert hypergrep_amd.check_compatibility(pats, flags=flags, ids=[0, 1, 2]) == 0


def test_a_filtering_min_length_compiles():
    """foo[a-z]*bar with min_length = 12: rejected before the match-length pass existed."""
    import hypergrep_amd

    pats, flags, exts = ["hello", "foo[a-z]*bar"], [0, 0], [None, ext(min_length=12)]
    assert _hg(pats, flags, exts) is None
    assert _hs(pats, flags, exts, HS_MODE_BLOCK) is None
    assert hypergrep_amd.check_compatibility(pats, flags=flags, ids=[0, 1], ext=exts) == 0
    db = minlensim_py.Db(pats, flags, exts=exts)
    assert db.ok(), db.error
    info = db.info()
    assert info["filtering"] == 1 and info["nsom"] == 0
    assert [p["min_length"] for p in info["patterns"]] == [0, 12]
    assert [p["reverse_tables"] for p in info["patterns"]] == [0, 1]  # the transposed follow table, without the SOM flag


def test_stream_mode_rejects_a_filtering_min_length_and_takes_a_trivial_one():
    pats, flags = ["hello", "foo[a-z]*bar"], [0, 0]
    msg = _hs(pats, flags, [None, ext(min_length=12)], HS_MODE_STREAM)
    assert msg is not None and msg.startswith("1: ") and STREAM_RULE in msg, msg
    assert _hs(pats, flags, [None, ext(min_length=6)], HS_MODE_STREAM) is None
    assert _hs(["foobar"], [0], [ext(min_length=6)], HS_MODE_STREAM) is None


def test_a_trivial_min_length_leaves_the_database_unchanged():
    pats, flags = ["foo[a-z]*bar", "abcde", r"\bx+y"], [0, SINGLE, 6]
    plain = extsim_py.Db(pats, flags, mode="plain").digest()
    assert extsim_py.Db(pats, flags, exts=[ext(min_length=6), ext(min_length=5), ext(min_length=2)]).digest() == plain
    assert extsim_py.Db(pats, flags, exts=[ext(min_length=7), None, None]).digest() != plain
    db = minlensim_py.Db(pats, flags, exts=[ext(min_length=6), ext(min_length=5), ext(min_length=2)])
    assert db.info()["filtering"] == 0


def test_singlematch_with_a_filtering_min_length_emits_every_end():
    info = minlensim_py.Db(["fo+", "fo+", "ba+r"], [SINGLE, SINGLE, SINGLE], exts=exts_for([4, 2, None])).info()
    assert [p["single"] for p in info["patterns"]] == [0, 1, 1]  # (min_length 2 is the shortest match: dropped)
    assert [p["min_length"] for p in info["patterns"]] == [4, 0, 0]


# ---- the filter in its place: fixed cases

def check_text(pats, flags, min_lengths, data, buffer_size=1 << 20, ids=None, min_removed=1):
    """Every piece's delivered (id, to, from) equal the brute-force expectation.  Returns (delivered, removed by the filter)."""
    ids = ids or list(range(len(pats)))
    db = minlensim_py.Db(pats, flags, ids, exts_for(min_lengths))
    assert db.ok(), db.error
    plain = minlensim_py.Db(pats, flags, ids)
    delivered = removed = 0
    for _, _, line in somsim_py.pieces(data, buffer_size):
        got, _ = db.piece(line)
        want = expected_piece(pats, flags, ids, min_lengths, line)
        assert [r[:3] for r in got] == want, (pats, flags, min_lengths, line)
        delivered += len(got)
        removed += len(plain.piece(line)[0]) - len(got)
    assert removed >= min_removed, (pats, data)
    return delivered, removed


@pytest.mark.parametrize("pat,flags,need,data", [
    ("foo[a-z]*bar", 6, 12, b"foobar fooxxxxxxbar fooxxxbar\nfooabcdefghibar foobar\n"),
    (r"\bfoo\w*", 6, 5, b"foo foot foots xfoots foo_1\n"),
    (r"^ab+", 6, 3, b"ab abb\nabbb ab\n abbb\n"),
    (r"a+$", 6, 2, b"baaa\na\nxa a\naa"),
    (r"a+$", 2, 3, b"baaa\naa\nxaaa"),
    (r"\Bbar\w*\b", 6, 5, b"xbar xbarab bar_ab zbarabc.\n"),
    ("(ab|b)c+", 6, 3, b"abc bc bcc xabcabcc\n"),
    (r"x\d{2,5}y", 6, 6, b"x12y x1234y xx99yy x12345y\n"),
    ("hel+o", 7, 6, b"HeLLo helllo hELLLLO helo\n"),
    (".*x", 6, 4, b"abx\nabcxdefx\nx x\n"),
])
def test_fixed_cases(pat, flags, need, data):
    delivered, _ = check_text([pat], [flags], [need], data)
    assert delivered  # some reports go (check_text) and some stay


def test_singlematch_delivers_the_first_end_that_is_long_enough():
    # the first end of fo+ is too short; under SINGLEMATCH the smallest end of a long enough match is delivered
    data = b"fo foo fooo\nfoooo fo\nfo fo\n"
    delivered, removed = check_text(["fo+", "ba+r"], [6 | SINGLE, 6 | SINGLE], [4, None], data + b"bar fo baar fooo\n")
    assert delivered == 4 and removed >= 1
    db = minlensim_py.Db(["fo+"], [6 | SINGLE], exts=exts_for([4]))
    assert [r[:2] for r in db.piece(b"fo foo fooo\n")[0]] == [(0, 11)]
    assert db.piece(b"fo fo\n")[0] == []


def test_two_expressions_on_one_id_with_different_lengths():
    # (7, to) is delivered once if at least one of the expressions produces it and passes its own min_length
    pats, flags, ids = ["ab+", "[ab]+b", "c+"], [6, 6, 6], [7, 7, 8]
    check_text(pats, flags, [4, 6, None], b"abb abbb aabbbb ccc\nabbbbb bab\n", ids=ids)
    check_text(pats, [6 | SINGLE, 6, 6], [3, 5, 2], b"ab abb aabbbb c cc\nabbbbb bab\n", ids=ids)


def test_som_with_min_length_and_shared_som_ids():
    # alone on its id: `from` is the leftmost start, unchanged; shared id: the smallest start over the expressions whose own
    # report at `to` survives ([ab]+c starts further left, but only where it is long enough does its start count)
    check_text(["fo+bar"], [6 | SOM], [7], b"foobar fooobar xfoooobar\n")
    pats, flags, ids = ["b+c", "[ab]+c", "x+"], [6 | SOM, 6 | SOM, 6], [3, 3, 4]
    check_text(pats, flags, [None, 6, None], b"abbc aaabbc bc xx\naaaaabc c\n", ids=ids, min_removed=0)  # (only starts change)
    check_text(pats, flags, [3, 6, 2], b"abbc aaabbc bc xx x\naaaaabc c\n", ids=ids)
    db = minlensim_py.Db(pats, flags, ids, exts_for([None, 6, None]))
    assert [r[:3] for r in db.piece(b"abbc aaabbc\n")[0]] == [(3, 4, 1), (3, 11, 5)]


def test_combination_whose_operand_is_filtered_away():
    # `1 & !2`: operand 2 (fo+, at least 4 bytes) is true only from a long enough match on
    pats = ["bar", "fo+", "1 & !2"]
    flags, ids = [6, 6, COMBINATION], [1, 2, 100]
    db = minlensim_py.Db(pats, flags, ids, exts_for([None, 4, None]))
    assert db.ok(), db.error
    assert [r[:2] for r in db.piece(b"foo bar\n")[0]] == [(1, 7), (100, 7)]
    assert [r[:2] for r in db.piece(b"fooo bar\n")[0]] == [(1, 8), (2, 4)]
    check_text(pats, flags, [None, 4, None], b"foo bar\nfooo bar\nbar fo bar foooo bar\n", ids=ids)


def test_quiet_operand_with_min_length():
    pats = ["bar", "fo+", "1 & 2"]
    flags, ids = [6, 6 | QUIET, COMBINATION], [1, 2, 100]
    db = minlensim_py.Db(pats, flags, ids, exts_for([None, 4, None]))
    assert db.ok(), db.error
    assert [r[:2] for r in db.piece(b"foo bar\n")[0]] == [(1, 7)]  # the quiet operand never became true
    assert [r[:2] for r in db.piece(b"fooo bar\n")[0]] == [(1, 8), (100, 8)]
    check_text(pats, flags, [None, 4, None], b"foo bar\nfooo bar\nbar fo bar foooo bar\n", ids=ids)


def test_leading_nuls_and_split_pieces():
    # the origin of `to` and of the length is the piece after its leading NULs; a line split by buffer_size is several pieces
    pats, flags, need = ["fo+", r"\bba+r\b"], [6, 6], [4, 5]
    data = b"\0\0fooo fo\n\0foo\0fooo\nfoooooooo baaar\nbaaaaaaaaaaar fo\n"
    for bs in (1 << 20, 9, 6):
        check_text(pats, flags, need, data, buffer_size=bs)
    db = minlensim_py.Db(pats, flags, exts=exts_for(need))
    assert [r[:2] for r in db.piece(b"fooo fo\n")[0]] == [(0, 4)]
    # a match cut by the piece boundary counts with the bytes of its piece only
    assert [p for _, _, p in somsim_py.pieces(b"xxfoooo\n", 6)] == [b"xxfoo", b"oo\n"]
    assert db.piece(b"xxfoo")[0] == []


def test_the_scalar_routine_early_exits():
    db = minlensim_py.Db(["a+"], [6], exts=exts_for([3]))
    line = b"aaaaa b"
    for to in range(1, 6):
        for need in range(1, 8):
            assert db.long_enough(0, line, to, need) == (need <= to), (to, need)
    assert not db.long_enough(0, line, 7, 1)  # no match ends there


# ---- random expressions against Python `re`

def _cases():
    def compile_one(p, f):
        db = somsim_py.Db([p], [f | SOM])
        return db.ok(), db.error

    accepts = accept_rules.Tally().accepts(compile_one, features=True)  # (the cases of the start-of-match tests)
    for seed in range(12):
        for pat, flags, data, _ in regex_gen.end_offset_cases(seed, accepts=accepts):
            yield seed, pat, flags, data


def test_random_expressions_against_python_re():
    """Per case min_length = the largest match length among the brute-force reports: some reports go and some stay wherever
    the case has reports of two distinct lengths.  Cases with one length (or no report) take that length + 1 where the
    compiler accepts it, and expect nothing."""
    mixed = ran = 0
    for seed, pat, flags, data in _cases():
        lines = [line for _, _, line in somsim_py.pieces(data, 1 << 20)]
        lengths = {to - s for line in lines for s, to in spans(pat, flags, line)}
        need = max(lengths) if len(lengths) >= 2 else max(lengths, default=0) + 1
        db = minlensim_py.Db([pat], [flags], exts=exts_for([need]))
        if not db.ok():
            assert len(lengths) < 2 and "could remove reports" in db.error, (pat, flags, need, db.error)  # (longer than any match)
            continue
        ran += 1
        kept = 0
        for line in lines:
            got, _ = db.piece(line)
            want = expected_piece([pat], [flags], [0], [need], line)
            assert [r[:3] for r in got] == want, (seed, pat, flags, need, line)
            kept += len(got)
        if len(lengths) >= 2:
            mixed += 1
            assert kept, (seed, pat, flags, need)
        else:
            assert kept == 0, (seed, pat, flags, need)
    assert mixed >= 15, (mixed, ran)
