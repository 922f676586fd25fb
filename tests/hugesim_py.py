"""ctypes face of tests/native/libhugesim.so — TEST-ONLY placement accessor of the huge automata (more than 1024 positions,
hypergrep_amd/csrc/hg_huge.hip): which routine each huge expression of a compiled set runs in, and the shape of its exception
edges (see tests/native/hugesim.cpp).  The routine is restated here from huge_stage_words, clamp_stage and huge_prepare of
hg_huge.hip.  It labels test cells; it never produces an expected hit."""
from __future__ import annotations

import ctypes
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "hugesim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libhugesim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")
HUGE_WORDS = 16
STAGE_MAX = 12288  # HG_HUGE_STAGE_MAX
LDS_ROOM = (160 * 1024 - 256) // 4  # clamp_stage: the words of a CU's LDS a huge workgroup may take
REG_MAX_NW = 256  # huge_prepare: the register-resident routine holds up to 4 words per lane

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
        _lib.hgsim_free.argtypes = [ctypes.c_void_p]
        _lib.hugesim_exprs.restype = ctypes.c_uint32
        _lib.hugesim_exprs.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32]
    return _lib


def stage_need(nw: int, ncls: int, ctxfree: bool) -> int:
    """huge_stage_words (hg_huge.hip): the LDS words of one expression's staged per-byte tables."""
    return 64 + nw * (ncls + 4 + (1 if ctxfree else 36))


def clamp_stage(huge_max_nw: int, stage_words: int) -> int:
    """clamp_stage (hg_huge.hip): the staging cap left after the two state copies of the largest automaton."""
    state = 2 * huge_max_nw
    return 0 if state >= LDS_ROOM else min(stage_words, LDS_ROOM - state)


def routine(nw: int, need: int, cap: int) -> str:
    """huge_prepare + huge_run_unit (hg_huge.hip)."""
    if need > cap:
        return "lds_l2"
    if nw > REG_MAX_NW:
        return "lds_staged"
    return "reg1" if nw <= 64 else "reg2" if nw <= 128 else "reg4"


def placement(patterns, flags, ids=None) -> dict:
    """{"huge_max_nw", "huge_stage_words", "nhuge", "nslow_huge", "cap" (the staging cap the kernels get), "exprs": {expression
    index: dict}}.  An expression: tier, mode, nw, nnodes, ncls, ctxfree, init_hi, single, nsources, nranges, widest (the
    widest target range in words), lower (a target lies in a lower word than its source), crosses_slab (a range crosses a
    multiple of 64 words), top_target (the highest target word), need (staged words), routine."""
    n = len(patterns)
    enc = [p.encode() if isinstance(p, str) else p for p in patterns]
    err = ctypes.create_string_buffer(256)
    h = lib().hgsim_compile((ctypes.c_char_p * n)(*enc), (ctypes.c_uint * n)(*flags), (ctypes.c_uint * n)(*(ids if ids is not None else range(n))), n, err, 256)
    if not h:
        raise ValueError(f"the set did not compile: {err.value.decode()}")
    try:
        head = (ctypes.c_uint32 * 4)()
        out = (ctypes.c_uint32 * (HUGE_WORDS * n))()
        k = lib().hugesim_exprs(h, head, out, n)
        assert k <= n
        cap = clamp_stage(head[0], head[1])
        exprs = {}
        for u in range(k):
            w = out[u * HUGE_WORDS:(u + 1) * HUGE_WORDS]
            need = stage_need(w[3], w[4], bool(w[5]))
            exprs[w[0]] = {"tier": w[1], "mode": w[2], "nw": w[3], "ncls": w[4], "ctxfree": bool(w[5]), "init_hi": w[6], "nsources": w[7], "nranges": w[8], "widest": w[9],
                           "lower": bool(w[10]), "crosses_slab": bool(w[11]), "single": bool(w[12]), "top_target": w[13], "nnodes": w[14], "need": need,
                           "routine": routine(w[3], need, cap)}
        return {"huge_max_nw": head[0], "huge_stage_words": head[1], "nhuge": head[2], "nslow_huge": head[3], "cap": cap, "exprs": exprs}
    finally:
        lib().hgsim_free(h)
