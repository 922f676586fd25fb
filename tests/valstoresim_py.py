"""ctypes face of tests/native/libvalstoresim.so, a TEST-ONLY host replay of hypergrep_amd/csrc/hg_valstore.h (see
tests/native/valstoresim.cpp): a value store over many calls, its rankings, and the two-source comparison on its own."""
from __future__ import annotations

import ctypes
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "valstoresim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libvalstoresim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")

_lib = None


def build() -> None:
    deps = [SRC, os.path.join(REPO, "include", "hypergrep_amd.h")] + [os.path.join(CSRC, f) for f in ("hg_valstore.h", "hg_values.h", "hg_partlines.h", "hg_gather.h", "hg_parts.h",
                                                                                                     "hg_core.h", "hg_db.h")]
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in deps):
        return
    tmp = f"{LIB}.{os.getpid()}.tmp"  # built aside and renamed into place (parallel test workers)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-fPIC", "-shared", "-o", tmp, SRC])
    os.replace(tmp, LIB)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        u32, u64, p8, p32, p64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.c_void_p
        _lib.valstoresim_new.restype = vp
        _lib.valstoresim_new.argtypes = [u32, u32, u32]
        _lib.valstoresim_free.argtypes = [vp]
        _lib.valstoresim_add.restype = ctypes.c_long
        _lib.valstoresim_add.argtypes = [vp, p8, u64, u64, p64, u64, p64, u64, u64, u64, p64]
        _lib.valstoresim_rank.restype = ctypes.c_long
        _lib.valstoresim_rank.argtypes = [vp, u64, ctypes.c_int, u64, ctypes.POINTER(ctypes.c_uint8), u64, u64, p64, p64, p64, p32, p64, p64]
        _lib.valstoresim_trace.argtypes = [vp, p64, u64, p64, u64, p64, p64]
        _lib.valstoresim_equal.argtypes = [p8, u64, u64, p8, u64, u64, u32, ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
        _lib.valstoresim_sizes.argtypes = [p32]
    return _lib


SIZES = ("sizeof_params", "sizeof_result", "sizeof_rank_result", "p.flags", "p.hash_bits", "p.table_log2", "p.store_log2", "r.n_distinct", "r.n_added", "r.n_groups", "r.n_parts",
         "r.n_parts_total", "r.n_bytes", "r.store_log2", "r.acc_us", "k.n_values", "k.n_distinct", "k.n_parts", "k.n_bytes", "k.d_bytes", "k.d_off", "k.d_count", "k.d_first",
         "k.d_pattern", "k.d_line_number", "k.store_log2", "k.rank_us", "by_pattern", "reset", "order_first", "sizeof_values_result", "sizeof_rank_values_result")


def sizes() -> dict:
    out = (ctypes.c_uint32 * len(SIZES))()
    lib().valstoresim_sizes(out)
    return dict(zip(SIZES, out))


def equal(a: bytes, sa: int, b: bytes, sb: int, n: int, wave: bool) -> bool:
    """Are a[sa:sa + n] and b[sb:sb + n] equal, by a lane's path or a wave's shares?  Neither may be read outside its bytes
    rounded up to 4."""
    bad = ctypes.c_int()
    eq = lib().valstoresim_equal(a, len(a), sa, b, len(b), sb, n, 1 if wave else 0, ctypes.byref(bad))
    assert not bad.value, "a read left the text or the arena"
    return bool(eq)


class Store:
    """A replayed store.  add() takes a text, its records (line, start, len) and its parts (line, from, to, pattern), both in
    the scan's order; rank() gives the arrays valstore_ref.arrays gives."""

    NOMEM = -5

    def __init__(self, by_pattern: bool = False, hash_bits: int = 0, store_log2: int = 0, order_seed: int = 0, tile: int = 16384, base: int = 0):
        self._h = lib().valstoresim_new(1 if by_pattern else 0, hash_bits, store_log2)
        self.order_seed, self.tile, self.base = order_seed, tile, base
        self.info = {}

    def __del__(self):
        if getattr(self, "_h", None):
            lib().valstoresim_free(self._h)
            self._h = None

    def add(self, text: bytes, records, parts, allow_nomem: bool = False) -> int:
        n, nr = len(parts), len(records)
        c_recs = (ctypes.c_uint64 * max(3 * nr, 1))(*[v for r in records for v in (r[0], r[1] + self.base, r[2])])
        c_parts = (ctypes.c_uint64 * max(4 * n, 1))(*[v for p in parts for v in p[:4]])
        totals = (ctypes.c_uint64 * 6)()
        rc = lib().valstoresim_add(self._h, text, len(text), self.base, c_recs, nr, c_parts, n, self.order_seed, self.tile, totals)
        if rc == self.NOMEM and allow_nomem:
            return rc
        assert rc == 0, f"valstoresim_add returned {rc}"
        self.info = {"n_distinct": totals[0], "n_added": totals[1], "n_groups": totals[2], "store_log2": totals[3], "rehashes": totals[4], "probes": totals[5]}
        return 0

    GROUP_COLS = ("tier", "found", "probes", "wrapped")  # tier: 1 lane, 2 wave
    VALUE_COLS = ("home_old", "home_new")               # home_old NONE (2^64 - 1) while the store had no table
    CALL_COLS = ("log2_old", "log2_new", "rehashed", "arena_tail", "tail16", "new_bytes", "sort_bits", "n_long")

    def trace(self, max_groups: int = 1 << 16, max_values: int = 1 << 16):
        """The read-outs of the last add() that returned 0 (valstoresim.cpp, Store::tr_*): {"groups": a dict of GROUP_COLS per
        group of the call, in the order of first, "values": one of VALUE_COLS per stored value, "call": one of CALL_COLS}."""
        g, v = (ctypes.c_uint64 * (len(self.GROUP_COLS) * max_groups))(), (ctypes.c_uint64 * (len(self.VALUE_COLS) * max_values))()
        call, counts = (ctypes.c_uint64 * len(self.CALL_COLS))(), (ctypes.c_uint64 * 2)()
        lib().valstoresim_trace(self._h, g, max_groups, v, max_values, call, counts)
        assert counts[0] <= max_groups and counts[1] <= max_values
        ng, nv, gc, vc = counts[0], counts[1], len(self.GROUP_COLS), len(self.VALUE_COLS)
        return {"groups": [dict(zip(self.GROUP_COLS, g[gc * j:gc * (j + 1)])) for j in range(ng)], "values": [dict(zip(self.VALUE_COLS, v[vc * i:vc * (i + 1)])) for i in range(nv)],
                "call": dict(zip(self.CALL_COLS, call))}

    def rank(self, top: int = 0, order_first: bool = False, max_rows: int = 1 << 16, max_bytes: int = 1 << 22):
        out = (ctypes.c_uint8 * max_bytes)()
        off, count, first, line = ((ctypes.c_uint64 * (max_rows + 1))() for _ in range(4))
        pattern = (ctypes.c_uint32 * (max_rows + 1))()
        totals = (ctypes.c_uint64 * 4)()
        rc = lib().valstoresim_rank(self._h, top, 1 if order_first else 0, self.tile, out, max_bytes, max_rows, off, count, first, pattern, line, totals)
        assert rc == 0, f"valstoresim_rank returned {rc}"
        nv, nb = totals[0], totals[1]
        return ({"bytes": bytes(out[:nb]), "off": list(off[:nv + 1]), "count": list(count[:nv]), "first": list(first[:nv]), "pattern": list(pattern[:nv]),
                 "line_number": list(line[:nv])}, {"n_distinct": totals[2], "n_parts": totals[3]})
