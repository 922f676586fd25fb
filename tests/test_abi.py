"""CPU tests of the C-ABI boundary: the shared library loads without a GPU (every symbol resolved) and exports
exactly the entry points include/hypergrep_amd.h declares; compile-only entry points work without a GPU and the
scan entry points fail loudly instead of falling back to a CPU path."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "hypergrep_amd.h")
LIB = os.path.join(REPO, "hypergrep_amd", "lib", "libhyperscanner.so")


def declared_functions() -> list[str]:
    text = open(HEADER, encoding="utf-8").read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"^\s*(?:const\s+)?(?:int|void|char|uint64_t)\s*\*?\s*(\w+)\s*\(", text, flags=re.M)
    return sorted(set(n for n in names if n.startswith(("hg_", "hs_")) or n in ("hyperscan", "check_patterns")))


def test_header_declares_the_three_faces():
    names = declared_functions()
    for must in ("hyperscan", "check_patterns", "hs_compile_multi", "hs_free_compile_error", "hs_alloc_scratch", "hs_scan",
                 "hs_free_scratch", "hs_free_database", "hg_db_compile", "hg_scan_device", "hg_copy_hits"):
        assert must in names


def test_library_loads_with_all_symbols_resolved():
    # RTLD_NOW: an unresolved kernel stub or helper would fail here, on a box without any GPU
    lib = ctypes.CDLL(LIB, mode=os.RTLD_NOW)
    for name in declared_functions():
        assert hasattr(lib, name), f"{name} is declared in include/hypergrep_amd.h but not exported"


def test_only_the_c_abi_is_exported():
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB], text=True)
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    extra = {s for s in exported if not (s in declared_functions() or s in ("_init", "_fini"))}
    assert not extra, f"unexpected exported symbols: {sorted(extra)[:10]}"


def test_compile_only_entry_points_need_no_gpu():
    import hypergrep_amd

    assert hypergrep_amd.check_compatibility(["foobar", "user=[a-z0-9_]{4,12} status=5[0-9]{2}"]) == 0
    assert hypergrep_amd.check_compatibility(["(?<!foo)bar"]) == 4
    with pytest.raises(ValueError):
        hypergrep_amd.prepare_patterns([""])
    with pytest.raises(ValueError):
        hypergrep_amd.prepare_patterns(["a"], flags=[1, 2])
    with pytest.raises(ValueError):
        hypergrep_amd.prepare_patterns(["a"], ids=[1, 2])
    pa, fa, ia = hypergrep_amd.prepare_patterns(["a", "b"])
    assert list(fa) == [14, 14] and list(ia) == [0, 0]


def test_python_api_error_paths_match_the_reference(tmp_path):
    import hypergrep_amd

    with pytest.raises(FileNotFoundError):
        hypergrep_amd.grep(str(tmp_path / "missing"), ["x"])
    assert hypergrep_amd.grep(str(tmp_path / "missing"), ["x"], no_messages=True) == ([], 101)
    with pytest.raises(ValueError):
        hypergrep_amd.grep(str(tmp_path), ["x"])
    assert hypergrep_amd.grep(str(tmp_path), ["x"], no_messages=True) == ([], 101)
    assert hypergrep_amd.RC_INVALID_FILE == 101 and hypergrep_amd.HS_FLAG_SINGLEMATCH == 8
    assert ctypes.sizeof(hypergrep_amd.Result) == 24
    assert hypergrep_amd.Result.line_number.offset == 8 and hypergrep_amd.Result.line.offset == 16


def test_no_cpu_fallback_without_gpu(tmp_path):
    import torch

    if torch.cuda.is_available():
        pytest.skip("this box has a GPU")
    import hypergrep_amd
    from hypergrep_amd import device

    path = tmp_path / "f.txt"
    path.write_text("needle_in_haystack\n")
    called = []
    assert hypergrep_amd.scan(str(path), ["needle_in_haystack"], lambda m, c: called.append(c)) == 3  # HYPERSCANNER_SCRATCH
    assert not called
    with pytest.raises(device.DeviceError):
        device.Scanner(device.Database(["needle_in_haystack"]))


def test_synthetic_generator_is_deterministic_on_host():
    from hypergrep_amd import benchspec, device

    patterns, needles, hpm = benchspec.c3_spec()
    a = device.synth_host(100000, 5, needles, hpm)
    b = device.synth_host(100000, 5, needles, hpm)
    assert a == b and a.count(b"\n") > 500
    # a shard starting at block 3 equals the corresponding slice of the whole
    whole = device.synth_host(5 * device.SYNTH_BLOCK, 5, needles, hpm)
    part = device.synth_host(2 * device.SYNTH_BLOCK, 5, needles, hpm, first_block=3)
    assert whole[3 * device.SYNTH_BLOCK:] == part


def test_streaming_kernels_stay_in_registers():
    """Per-kernel resources recorded by the build (hypergrep_amd/build.py, compiler remarks).  The dword-aligned stream
    kernels must not touch scratch and, for filters up to 32 KiB, must keep six waves per SIMD: a by-value argument one
    field too large once cost 20 % of the stream pass while every parity test stayed green."""
    import json

    path = os.path.join(REPO, "hypergrep_amd", "lib", "kernel_resources.json")
    if not os.path.exists(path):
        pytest.skip("library built by an older build.py (no kernel_resources.json)")
    table = json.load(open(path, encoding="utf-8"))
    stream = {k: v for k, v in table.items() if k.startswith("_Z16hg_stream_kernelILi")}
    assert len(stream) >= 23 and sum(1 for k in stream if "ELb0ELi0E" in k) == 10  # (dword-aligned single-probe filters: with and without the fold instruction)
    for name, res in stream.items():
        log2 = int(re.match(r"_Z16hg_stream_kernelILi(\d+)E", name).group(1))
        byte_aligned = "ELb0ELi1E" in name or "ELb0ELi2E" in name
        if byte_aligned:  # sixteen probes per chunk: a handful of spilled registers in the drain path is tolerated
            assert res["VGPRs Spill"] <= 12 and res["ScratchSize [bytes/lane]"] <= 96, (name, res)
        else:  # (one or two prologue values folded into scratch are tolerated, hypergrep_amd/build.py; nothing inside the tile loop)
            assert res["VGPRs Spill"] <= 2 and res["ScratchSize [bytes/lane]"] <= 16, (name, res)
        if log2 <= 13:
            assert res["Occupancy [waves/SIMD]"] >= 6, (name, res)
    # the side passes: a struct that grew by five fields once put the hit sink of every confirm kernel on the stack
    for prefix in ("_Z16hg_verify_kernel", "_Z22hg_confirm_fast_kernel", "_Z24hg_always_on_fast_kernel", "_Z26hg_always_on_finish_kernel",
                   "_Z25hg_confirm_generic_kernel"):
        names = [k for k in table if k.startswith(prefix)]
        assert names, prefix
        for name in names:
            assert table[name]["ScratchSize [bytes/lane]"] == 0 and table[name]["VGPRs Spill"] == 0, (name, table[name])


def test_face_a_artefact_has_the_soname_the_reference_shim_needs():
    """hypergrep/utils.py:63,75 loads the configured libhs first; the shim's DT_NEEDED `libhs.so.5` is then satisfied only
    by an object whose SONAME is exactly that.  The build links hypergrep_amd/lib/libhs.so.5 for it."""
    libhs = os.path.join(REPO, "hypergrep_amd", "lib", "libhs.so.5")
    assert os.path.exists(libhs), "hypergrep_amd/build.py did not produce the Face A artefact"
    dyn = subprocess.check_output(["readelf", "-d", libhs], text=True)
    assert re.search(r"SONAME.*\[libhs\.so\.5\]", dyn)
    lib = ctypes.CDLL(libhs, mode=os.RTLD_NOW)
    for name in ("hs_compile_multi", "hs_free_compile_error", "hs_alloc_scratch", "hs_scan", "hs_free_scratch", "hs_free_database"):
        assert hasattr(lib, name), name
    # unversioned symbols, like the ones the shipped shim imports
    syms = subprocess.check_output(["nm", "-D", "--defined-only", libhs], text=True)
    assert re.search(r" T hs_scan$", syms, flags=re.M)
    # compile-only entry points work without a GPU through this object too; the free functions accept NULL
    # (hyperscanner.c:140 after a success, :323-324 on the error paths)
    db = ctypes.c_void_p()
    pa = (ctypes.c_char_p * 1)(b"foo[0-9]+bar")
    fa = (ctypes.c_uint * 1)(14)
    ia = (ctypes.c_uint * 1)(0)
    assert lib.hs_compile_multi(pa, fa, ia, 1, 1, None, ctypes.byref(db), None) == 0 and db.value
    assert lib.hs_free_compile_error(None) == 0 and lib.hs_free_scratch(None) == 0
    assert lib.hs_free_database(db) == 0 and lib.hs_free_database(None) == 0


def test_reference_loader_accepts_the_face_a_artefact(tmp_path):
    """The north-star boundary: the reference's Python (hypergrep/utils.py:125-144 configure_libraries, :55-83 loaders) loads
    the configured `libhs` by path with ctypes' default mode, then its prebuilt shim, whose DT_NEEDED libhs.so.5 (no RPATH /
    RUNPATH) can only bind to an already-loaded object of that SONAME.  The shim's link requirements are recorded in
    tests/golden/reference_shim_abi.json; tests/native/libhs_consumer.c stands in for the shim with the same libhs imports,
    linked against the ORACLE's libhs.so.5 as the shim was linked against real Hyperscan, and is loaded the same way after
    hypergrep_amd/lib/libhs.so.5.  Its compile calls then run this repository's compiler.  No GPU is needed for the compile
    path; a scan through the same stack stops at hs_alloc_scratch without one, never on a CPU fallback.  Runs in a child
    process: a loaded libhs stays bound for the life of the process."""
    import json
    import sys

    with open(os.path.join(REPO, "tests", "golden", "reference_shim_abi.json"), encoding="utf-8") as f:
        shim = json.load(f)
    assert "libhs.so.5" in shim["needed"] and not shim["runpath"]
    libhs = os.path.realpath(os.path.join(REPO, "hypergrep_amd", "lib", "libhs.so.5"))
    oracle_libhs = os.path.realpath(os.path.join(REPO, "oracle", "_build", "libhs.so.5"))
    assert os.path.exists(oracle_libhs), "build() makes oracle/_build/libhs.so.5"
    # every symbol the shim imports from libhs is exported, unversioned, by the artefact
    syms = subprocess.check_output(["nm", "-D", "--defined-only", libhs], text=True)
    for name in shim["libhs_imports"]:
        assert re.search(rf" T {name}$", syms, flags=re.M), name
    # the stand-in: same libhs imports, same DT_NEEDED, no search path of its own
    consumer = str(tmp_path / "libhs_consumer.so")
    subprocess.check_call(["gcc", "-std=c99", "-O2", "-Wall", "-Wextra", "-fPIC", "-shared", "-I", os.path.join(REPO, "include"),
                           "-o", consumer, os.path.join(REPO, "tests", "native", "libhs_consumer.c"),
                           "-L", os.path.dirname(oracle_libhs), "-l:libhs.so.5"])
    dyn = subprocess.check_output(["readelf", "-d", consumer], text=True)
    assert "Shared library: [libhs.so.5]" in dyn and "RPATH" not in dyn and "RUNPATH" not in dyn
    imports = subprocess.check_output(["nm", "-D", "--undefined-only", consumer], text=True)
    assert sorted(line.split()[-1] for line in imports.splitlines() if line.split()[-1].startswith("hs_")) == shim["libhs_imports"]
    code = """
import ctypes, json, sys
libhs, consumer = sys.argv[1:3]
ctypes.cdll.LoadLibrary(libhs)  # by path, ctypes' default mode: what the reference's loader does
c = ctypes.cdll.LoadLibrary(consumer)
def check(ps):
    n = len(ps)
    return c.consumer_compile((ctypes.c_char_p * n)(*[p.encode() for p in ps]), (ctypes.c_uint * n)(*[14] * n), (ctypes.c_uint * n)(*[0] * n), n)
ok, bad = check(["foobar", "status=5[0-9]{2}"]), check(["(?<!a)b"])
maps = open("/proc/self/maps").read()
alloc = ctypes.c_int(0)
reports = c.consumer_scan(b"bar", b"foo\\nbar\\nfoobar\\n", 15, ctypes.byref(alloc))
print(json.dumps({"ok": ok, "bad": bad, "ours": libhs in maps, "oracle": sys.argv[3] in maps, "alloc": alloc.value, "reports": reports}))
"""
    out = subprocess.run([sys.executable, "-c", code, libhs, consumer, oracle_libhs], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["ok"] == 0 and res["bad"] == -4  # HS_SUCCESS; HS_COMPILER_ERROR from this repository's compiler
    assert res["ours"] and not res["oracle"], "the consumer's DT_NEEDED libhs.so.5 did not bind to this repository's artefact"
    import torch

    if not torch.cuda.is_available():
        assert res["alloc"] != 0 and res["reports"] == -1  # no GPU, and no CPU path
    else:
        assert res["alloc"] == 0 and res["reports"] == 1  # (SINGLEMATCH: one report per id and scan call)


def test_compile_cache_hits_and_bound():
    """The reference recompiles the database for every file (hyperscanner.c:296); here identical pattern sets share one
    compiled database: a repeated set is a cache hit, and the cache holds at most 16 sets (least recently used evicted).
    check_patterns() goes through the same cache and needs no GPU."""
    import hypergrep_amd
    from hypergrep_amd import device

    before = device.faceb_stats()
    assert hypergrep_amd.check_compatibility(["cache_probe_alpha", "beta[0-9]+"]) == 0
    mid = device.faceb_stats()
    assert mid["db_cache_misses"] == before["db_cache_misses"] + 1
    assert hypergrep_amd.check_compatibility(["cache_probe_alpha", "beta[0-9]+"]) == 0
    after = device.faceb_stats()
    assert after["db_cache_hits"] == mid["db_cache_hits"] + 1 and after["db_cache_misses"] == mid["db_cache_misses"]
    # same expressions, other flags or ids: a different database
    assert hypergrep_amd.check_compatibility(["cache_probe_alpha", "beta[0-9]+"], flags=[14, 6]) == 0
    assert device.faceb_stats()["db_cache_misses"] == after["db_cache_misses"] + 1
    for i in range(20):
        assert hypergrep_amd.check_compatibility([f"cache_filler_{i:02d}"]) == 0
    full = device.faceb_stats()
    assert full["db_cache_entries"] == 16
    # the first set was evicted meanwhile: compiling it again is a miss; a rejected set is never cached
    assert hypergrep_amd.check_compatibility(["cache_probe_alpha", "beta[0-9]+"]) == 0
    assert device.faceb_stats()["db_cache_misses"] == full["db_cache_misses"] + 1
    assert hypergrep_amd.check_compatibility(["(?<!x)y"]) == 4 and hypergrep_amd.check_compatibility(["(?<!x)y"]) == 4
    assert device.faceb_stats()["db_cache_entries"] == 16


def test_faceb_device_selection(monkeypatch):
    """Concurrent hyperscan() calls shard files over the node's GPUs round-robin; HYPERGREP_DEVICE pins one (hg_shim.hip
    checkout -> hg_faceb_next_device)."""
    from hypergrep_amd import device

    monkeypatch.delenv("HYPERGREP_DEVICE", raising=False)
    first = device.faceb_next_device(8)
    assert [device.faceb_next_device(8) for _ in range(16)] == [(first + 1 + i) % 8 for i in range(16)]
    assert device.faceb_next_device(1) == 0 and device.faceb_next_device(0) == -1
    monkeypatch.setenv("HYPERGREP_DEVICE", "5")
    assert [device.faceb_next_device(8) for _ in range(4)] == [5, 5, 5, 5]
    assert device.faceb_next_device(4) == 1  # (taken modulo the devices present)
