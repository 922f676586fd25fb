"""The fixed table of the parts tests (host replay and GPU): (name, patterns, flags, text, buffer_size, expected part strings
or None).  Where strings are listed they are the parts in order over the whole text, as bytes; every row is also compared
with parts_ref in full (line, from, to, pattern)."""
from __future__ import annotations

A = 6  # DOTALL | MULTILINE: all-matches mode
CASELESS, DOTALL, MULTILINE, SINGLE = 1, 2, 4, 8
BIG = 1 << 20

TABLE = [
    ("leftmost-longest alternation", ["a|aaa"], [A], b"aaaa\n", BIG, [b"aaa", b"a"]),
    ("leftmost beats first end", ["abcd", "bc"], [A, A], b"xabcdx\n", BIG, [b"abcd"]),
    ("longest over expressions", ["ab", "abc"], [A, A], b"abcab\n", BIG, [b"abc", b"ab"]),
    ("lowest index on a tie", ["abc", "ab|abc"], [A, A], b"abcab\n", BIG, [b"abc", b"ab"]),
    ("adjacent parts", ["ab"], [A], b"ababab\n", BIG, [b"ab", b"ab", b"ab"]),
    ("anchored start", ["^a"], [A], b"aaa\n", BIG, [b"a"]),
    ("word boundary", [r"\bfoo"], [A], b"foo xfoo foofoo\n", BIG, [b"foo", b"foo"]),
    ("dollar multiline", ["a+$"], [A], b"baaa\naa a\nxa", BIG, [b"aaa", b"a", b"a"]),
    ("dollar not multiline", ["a+$"], [DOTALL], b"baaa\naa a\nxa", BIG, [b"aaa", b"a", b"a"]),
    ("caseless", ["hello"], [A | CASELESS], b"HeLLo hello hELLO\n", BIG, [b"HeLLo", b"hello", b"hELLO"]),
    ("dotall consumes the newline", ["foo.*"], [A], b"xfoo bar\nfoo\n", BIG, [b"foo bar\n", b"foo\n"]),
    ("no dotall stops before it", ["foo.*"], [MULTILINE], b"xfoo bar\n", BIG, [b"foo bar"]),
    ("several state words", [r"x\d{2,40}y"], [A], b"x12y x1y x123456789012y xx99yy\n", BIG, [b"x12y", b"x123456789012y", b"x99y"]),
    ("just under HG_MAX_NODES", ["[a-z]{1000}x"], [A], b"q" * 1000 + b"x\n" + b"q" * 40 + b"x\n", BIG, [b"q" * 1000 + b"x"]),
    ("match at offset 0", ["foo"], [A], b"foo\nxfoo\n", BIG, [b"foo", b"foo"]),
    ("ends at the last byte, final newline", ["bar"], [A], b"xbar\n", BIG, [b"bar"]),
    ("ends at the last byte, no final newline", ["bar"], [A], b"xx\nxbar", BIG, [b"bar"]),
    ("leading and inner NULs", ["foo", "ba+r"], [A, A], b"\0\0foo baar\nfoo\0bar\n\0bar foo\0\n", BIG, [b"foo", b"baar", b"foo", b"bar", b"foo"]),
    ("buffer_size 8 cuts lines", ["ab+", "cd"], [A, A], b"abbbbbbbbcd abcdabcd\nab\n", 8, None),
    ("grep() flags: all-zero ids, SINGLEMATCH", ["foo", "o+", "ba."], [A | SINGLE] * 3, b"foo boo bar\nbaz\n", BIG, [b"foo", b"oo", b"bar", b"baz"]),
    ("simple and multi-word together", ["needle", r"k\d{3,70}z"], [A, A], b"a needle k12345z needlek999z\n", BIG, [b"needle", b"k12345z", b"needle", b"k999z"]),
]
# (ids of every row: all zero, as grep() compiles them)
