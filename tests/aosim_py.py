"""ctypes face of tests/native/libaosim.so — TEST-ONLY placement accessor of the always-on tier: which unit of
hg_always_on_fast_kernel (or the scalar kernel) each expression of a compiled set lands in, and what decides the routine the
unit runs in (see tests/native/aosim.cpp).  It labels test cells; it never produces an expected hit."""
from __future__ import annotations

import ctypes
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "aosim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libaosim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")
UNIT_WORDS = 40
NONE = 0xFFFFFFFF
KINDS = ("group", "single", "scalar", "huge")

_lib = None


def build() -> None:
    deps = [SRC, os.path.join(REPO, "tests", "native", "hostsim.cpp")] + [
        os.path.join(CSRC, f) for f in ("hg_compile.cpp", "hg_compile.h", "hg_core.h", "hg_db.h", "hg_post.h")]
    if os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in deps):
        return
    tmp = f"{LIB}.{os.getpid()}.tmp"  # built aside and renamed into place (parallel test workers)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-fPIC", "-shared", "-o", tmp, SRC, os.path.join(CSRC, "hg_compile.cpp")])
    os.replace(tmp, LIB)


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        build()
        _lib = ctypes.CDLL(LIB)
        _lib.hgsim_compile.restype = ctypes.c_void_p
        _lib.hgsim_compile.argtypes = [ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_uint), ctypes.c_uint, ctypes.c_char_p, ctypes.c_size_t]
        _lib.hgsim_pattern_tier.restype = ctypes.c_uint32
        _lib.hgsim_pattern_tier.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        _lib.hgsim_free.argtypes = [ctypes.c_void_p]
        _lib.aosim_units.restype = ctypes.c_uint32
        _lib.aosim_units.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32]
    return _lib


def _u64(w, i):
    return w[i] | (w[i + 1] << 32)


def placement(patterns, flags, ids=None) -> dict:
    """{"ngroups", "nslow_fast", "nslow_grouped", "nslow", "tiers": [tier of each expression], "units": [dict per unit, in
    kernel order]}.  A unit: kind ("group", "single", "scalar", "huge"), members (expression indices), ctx, nw, nnodes, nt,
    nexc (exception nodes; more than 2: no shift form), shift_form (one word: the shift form is taken), masks (which of
    M0..M3 are non-zero), M (the four masks), src (exception sources), F (their follow rests), max_len (0: unbounded),
    nl_accepts, lean2 (two words: lean-eligible), single_mask."""
    n = len(patterns)
    enc = [p.encode() if isinstance(p, str) else p for p in patterns]
    err = ctypes.create_string_buffer(256)
    h = lib().hgsim_compile((ctypes.c_char_p * n)(*enc), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*(ids if ids is not None else range(n))), n, err, 256)
    if not h:
        raise ValueError(f"the set did not compile: {err.value.decode()}")
    try:
        tiers = [lib().hgsim_pattern_tier(h, i) for i in range(n)]
        head = (ctypes.c_uint32 * 4)()
        cap = n + 1
        out = (ctypes.c_uint32 * (UNIT_WORDS * cap))()
        nunits = lib().aosim_units(h, head, out, cap)
        assert nunits <= cap
        units = []
        for u in range(nunits):
            w = out[u * UNIT_WORDS:(u + 1) * UNIT_WORDS]
            units.append({
                "kind": KINDS[w[0]], "members": tuple(w[2:2 + w[1]]), "ctx": bool(w[10]), "nw": w[11], "nnodes": w[12], "nt": w[13], "nexc": w[14],
                "masks": tuple(k for k in range(4) if w[15] >> k & 1), "src": tuple(x for x in w[16:18] if x != NONE), "max_len": w[18],
                "nl_accepts": bool(w[19]), "lean2": bool(w[20]), "single_mask": w[21], "shift_form": bool(w[22]),
                "M": tuple(_u64(w, 24 + 2 * k) for k in range(4)), "F": tuple(_u64(w, 32 + 2 * k) for k in range(2)),
            })
        return {"ngroups": head[0], "nslow_fast": head[1], "nslow_grouped": head[2], "nslow": head[3], "tiers": tiers, "units": units}
    finally:
        lib().hgsim_free(h)
