"""Accept/reject parity through the product's real entry points (run with `-m gpu`): check_compatibility (Face B's
check_patterns), Face A's hs_compile_multi and the device API's hg_db_compile take and refuse exactly what the oracle takes and
refuses, and name the same expression.  The host differential over 20 000 cases is tests/test_accept_parity.py; this is the
same decision on a few hundred cases from both generators plus the fixed list, through the library that ships."""
from __future__ import annotations

import ctypes
import os
import random

import pytest

import accept_rules
import oracle_py
import regex_gen
from test_accept_parity import FLAG_WORDS, FOUND_BY_FUZZ, KNOWN, NEIGHBOURS
from test_gpu_parity import _HsErr, _loaded_native, torch_cuda  # noqa: F401  (torch_cuda: the module's GPU fixture)

pytestmark = pytest.mark.gpu


def _hs_compile(lib, pats, flags, ids):
    """(rc, error->expression or None) of hs_compile_multi in block mode."""
    n = len(pats)
    lib.hs_compile_multi.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint), ctypes.c_uint,
                                     ctypes.c_uint, ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.POINTER(_HsErr))]
    lib.hs_compile_multi.restype = ctypes.c_int
    lib.hs_free_database.argtypes = [ctypes.c_void_p]
    lib.hs_free_compile_error.argtypes = [ctypes.c_void_p]
    db, err = ctypes.c_void_p(), ctypes.POINTER(_HsErr)()
    rc = lib.hs_compile_multi((ctypes.c_char_p * n)(*[p.encode() for p in pats]), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*ids), n, 1, None,
                              ctypes.byref(db), ctypes.byref(err))
    expression = err.contents.expression if err else None
    if err:
        lib.hs_free_compile_error(err)
    if db:
        lib.hs_free_database(db)
    return rc, expression


def _cases():
    """(patterns, flags): the fixed list alone and at each index of a three-expression set, then single expressions and small
    sets from both generators."""
    for i, pat in enumerate(KNOWN + FOUND_BY_FUZZ):
        for j, f in enumerate((14, 6, 10, 15)):
            yield [pat], [f]
            at = (i + j) % 3
            yield NEIGHBOURS[:at] + [pat] + NEIGHBOURS[at:], [f] * 3
    rng = random.Random(33000)
    for gen in (regex_gen.random_pattern, regex_gen.assertion_heavy_pattern):
        for _ in range(150):
            yield [gen(rng)], [rng.choice(FLAG_WORDS)]
        for _ in range(40):
            k = rng.randint(2, 4)
            yield [gen(rng) for _ in range(k)], [rng.choice(FLAG_WORDS) for _ in range(k)]


def test_entry_points_accept_and_reject_like_the_oracle(torch_cuda):  # noqa: F811
    import hypergrep_amd
    from hypergrep_amd import device, utils

    product = utils._get_hyperscanner_lib()
    oracle = ctypes.CDLL(os.path.join(oracle_py.ORACLE_DIR, "_build", "libhs.so.5"))
    tally = accept_rules.Tally()
    failures = []
    for pats, flags in _cases():
        ids = list(range(len(pats)))
        want = oracle_py.check_patterns(pats, flags=flags, ids=ids)
        want_rc, want_at = _hs_compile(oracle, pats, flags, ids)
        assert want in (0, 4) and want_rc == (0 if want == 0 else -4) and (want_at is None) == (want == 0)
        try:
            device.Database(pats, flags=flags, ids=ids)
            error = None
        except device.CompileError as e:
            error = str(e)
        got = hypergrep_amd.check_compatibility(pats, flags=flags, ids=ids)
        got_rc, got_at = _hs_compile(product, pats, flags, ids)
        try:
            both = tally.decide(pats, flags, error is None, error)
            if want == 0 and not both:  # a documented capacity limit: every entry point states the same refusal
                assert got == 4 and got_rc == -4, (pats, flags, got, got_rc)
                continue
            assert got == want, f"check_compatibility {got}, the oracle's check_patterns {want}: {pats!r} flags {flags}"
            assert (got_rc, got_at) == (want_rc, want_at), f"hs_compile_multi {(got_rc, got_at)}, the oracle's {(want_rc, want_at)}: {pats!r} flags {flags}"
        except AssertionError as e:
            failures.append(str(e))
    print(tally.report())
    assert _loaded_native()
    assert not failures, (len(failures), failures[:5])
    assert tally.generated >= 500 and tally.oracle_rejected >= 0.10 * tally.generated, tally.report()
    assert tally.product_only_rejected <= 0.01 * tally.generated, tally.report()
