"""CPU: the C-ABI library loads and exports every symbol include/mvs_hip.h declares; without a GPU the
product path fails loudly instead of falling back."""
import os
import re

import pytest

from metagenome_vector_sketches_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    with open(os.path.join(ROOT, "include", "mvs_hip.h")) as f:
        text = f.read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mvs_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound():
    lib = _capi.load_library()
    declared = _header_symbols()
    assert len(declared) >= 20
    bound = {name for name, _, _ in _capi.SYMBOLS}
    for name in declared:
        assert hasattr(lib, name), name
        assert name in bound, "no ctypes signature for " + name
    assert b"gfx950" in lib.mvs_version()


def test_stream_dense_stats_refuses_a_null_context():
    lib = _capi.load_library()
    assert lib.mvs_ctx_stream_dense_stats(None, None, None, None, None) == _capi.MVS_E_INVALID


def test_pure_host_helpers_match_reference_formulas():
    # src/pairwise_comp_optimized.cpp:903-906, :938-940
    assert _capi.chunk_size(12, 2048) == 192
    assert _capi.chunk_size(12, 4096) == 48
    assert _capi.shard_rows(61, 2, 0) == (0, 31)
    assert _capi.shard_rows(61, 2, 1) == (31, 61)
    assert _capi.shard_rows(100, 8, 7) == (91, 100)
    assert _capi.shard_rows(3, 8, 7) == (3, 3)
    assert [_capi.limbs_for_max_abs(x) for x in (0, 127, 128, 8127, 8128, 32639, 32640, 8355711, 8355712, 2**31)] == \
        [1, 1, 2, 2, 2, 2, 3, 3, 4, 4]


def test_no_silent_fallback_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_capi.MvsError) as ei:
        _capi.Context(0)
    assert ei.value.code == _capi.MVS_E_HIP


def test_product_package_never_imports_oracle():
    pkg = os.path.join(ROOT, "metagenome_vector_sketches_amd")
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".cpp", ".h", ".hpp")):
                with open(os.path.join(dirpath, fn)) as f:
                    src = f.read()
                assert "pyoracle" not in src and "mvs_oracle" not in src and "libmvs_oracle" not in src, fn


def test_library_reads_the_environment_only_when_a_context_is_created():
    """tuning switches live in the context (mvs_ctx_set_option); below the C ABI exactly one getenv exists, in the
    function that seeds a new context's options, and the k-loop ablations are not part of the product library"""
    csrc = os.path.join(ROOT, "metagenome_vector_sketches_amd", "csrc")
    hits = []
    for fn in sorted(os.listdir(csrc)):
        if fn.endswith((".hip", ".h")):
            with open(os.path.join(csrc, fn)) as f:
                for i, line in enumerate(f, 1):
                    if "getenv(" in line:
                        hits.append((fn, i, line.strip()))
    assert len(hits) == 1 and hits[0][0] == "mvs_capi.hip", hits
    with open(os.path.join(csrc, "mvs_capi.hip")) as f:
        text = f.read()
    assert text.index("void options_from_env") < text.index("getenv(") < text.index("int check_kernel")
    lib = _capi.load_library()
    assert not hasattr(lib, "mvs_ctx_debug")                       # no debug entry points
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", _capi.LIB_PATH], capture_output=True, text=True).stdout
    assert "mvs_ctx_set_option" in syms and "mvs_comm_create" in syms and "mvs_allgather_planes" in syms


def test_generated_code_of_the_hand_counted_loads():
    """`make check-isa`: the direct-B ping-pong kernels (k_pairwise_pp<..., BD = 1>) issue their B-fragment loads as inline asm
    and count vmcnt by hand; the compiler believes the results are there at once.  tools/check_isa.py disassembles the gfx950
    code object inside the library that ships and checks that nothing touches a loaded fragment register before the wait that
    retires it and that every MFMA's B operand is such a register -- and that it would notice: three mutated variants of the
    real code (a register copy right after the load, a foreign B operand, weakened waits) must be rejected."""
    import subprocess
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "check_isa.py"), "--self-test"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "direct-B kernels pass" in r.stdout and "all 3 mutations" in r.stdout


@pytest.mark.gpu
def test_handles_close_once_and_in_order():
    """Cluster, Linkage, Derep and HashSet share one base (_capi._Handle): the context closes its children before itself, a
    second close is a no-op, and each is a context manager"""
    import numpy as np
    ctx = _capi.Context(0)
    try:
        n2 = np.ones(8)
        kids = [_capi.Cluster(ctx, 8), _capi.Linkage(ctx, 8, 64, n2), _capi.Derep(ctx, 8),
                ctx.hash_set(np.arange(16, dtype=np.uint64), np.arange(0, 17, 2, dtype=np.int64))]
        sset = ctx.sketch_set(np.ones((8, 64), dtype=np.int32))
        assert [type(k).__name__ for k in kids] == ["Cluster", "Linkage", "Derep", "HashSet"]
        assert all(isinstance(k, _capi._Handle) and k._h for k in kids) and sset._h
        calls = []
        for k in kids + [sset]:
            k.close = (lambda k=k, close=k.close: (calls.append(type(k).__name__), close()))
        ctx.close()
        assert ctx._h is None and all(k._h is None for k in kids) and sset._h is None
        assert calls[0] == "SketchSet" and sorted(calls[1:]) == ["Cluster", "Derep", "HashSet", "Linkage"]
        for k in kids + [sset]:
            del k.close
            k.close()                                                         # closed already: nothing happens
            assert k._h is None
        ctx.close()
    finally:
        ctx.close()
    ctx = _capi.Context(0)
    try:
        with _capi.Cluster(ctx, 4) as k:
            assert k._h
        assert k._h is None
        with _capi.Derep(ctx, 4) as k2, _capi.Linkage(ctx, 4, 64, np.ones(4)) as k3:
            assert k2._h and k3._h
        assert k2._h is None and k3._h is None
    finally:
        ctx.close()
