"""ctypes face of tests/native/libtilesim.so, a TEST-ONLY host replay of the tile scan's three kernels with the functions of
hypergrep_amd/csrc/hg_post.h (see tests/native/tilesim.cpp)."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "tilesim.cpp")
LIB = os.path.join(REPO, "tests", "native", "libtilesim.so")
CSRC = os.path.join(REPO, "hypergrep_amd", "csrc")

_lib = None


def build() -> None:
    deps = [SRC] + [os.path.join(CSRC, f) for f in ("hg_post.h", "hg_core.h", "hg_db.h")]
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
        u32, u64, p, p64 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64)
        _lib.tilesim_scan.restype = u32
        _lib.tilesim_scan.argtypes = [p, u64, u64, u64, p64, p]
        _lib.tilesim_walk.argtypes = [p, u64, u64, u64, p64, p]
        _lib.tilesim_tree.argtypes = [p, u64, u64, u64, u32, p64]
        _lib.tilesim_sizes.argtypes = [ctypes.POINTER(u32)]
    return _lib


def sizes() -> dict:
    out = (ctypes.c_uint32 * 4)()
    lib().tilesim_sizes(out)
    return dict(zip(("sizeof_sum", "sizeof_base", "sizeof_elem", "tile_bytes"), out))


def _run(fn, sums: np.ndarray, tile_begin: int, tile_end: int, bs1: int, state, bases: np.ndarray):
    assert sums.dtype == np.uint32 and sums.flags.c_contiguous and sums.shape[1] == 4 and tile_end <= len(sums)
    assert bases.dtype == np.uint64 and bases.flags.c_contiguous and bases.shape == (len(sums), 2)
    st = (ctypes.c_uint64 * 2)(*state)
    blocks = fn(sums.ctypes.data, tile_begin, tile_end, bs1, st, bases.ctypes.data)
    return (int(st[0]), int(st[1])), blocks


def scan(sums, tile_begin, tile_end, bs1, state, bases):
    """The three kernels' decomposition over tiles [tile_begin, tile_end): fills bases[tile] = (cs, L); returns (state at
    tile_end, blocks)."""
    return _run(lib().tilesim_scan, sums, tile_begin, tile_end, bs1, state, bases)


def walk(sums, tile_begin, tile_end, bs1, state, bases):
    """The sequential hg_tile_apply walk over the same tiles."""
    return _run(lib().tilesim_walk, sums, tile_begin, tile_end, bs1, state, bases)[0]


def tree(sums, a, b, bs1, split, state):
    """hg_tile_combine over tiles [a, b) in a tree order chosen by `split`, applied to `state`."""
    st = (ctypes.c_uint64 * 2)(*state)
    lib().tilesim_tree(sums.ctypes.data, a, b, bs1, split, st)
    return int(st[0]), int(st[1])
