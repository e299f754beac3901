"""Ranking on the device, the parts that need no GPU: the constants the GPU tests and the Python binding
restate are those of the sources, and the shipped library exports the entry points."""
import re
from pathlib import Path

import aux_hooks
from libcluster_amd import capi

ROOT = Path(__file__).resolve().parents[1]


def test_chunk_constant_of_the_gpu_tests_is_that_of_the_source():
    """tests/test_gpu_top_rows.py restates lck::TOP_CHUNK_ROWS to place its row counts on both sides of a chunk boundary
    (read as text: importing the GPU test module here would mark nothing and prove nothing more)"""
    def const(text, name):
        m = re.findall(r"\b" + name + r"\s*=\s*(\d+)", text)
        assert len(m) == 1, (name, m)
        return int(m[0])

    src = (ROOT / "libcluster_amd" / "csrc" / "lc_kernels.h").read_text()
    test = (ROOT / "tests" / "test_gpu_top_rows.py").read_text()
    assert const(src, "TOP_CHUNK_ROWS") == const(test, "TOP_CHUNK_ROWS")
    assert const(src, "TOP_MAX_M") == 64  # the header's 1 ... 64
    assert "BIG_N = 3 * TOP_CHUNK_ROWS + 17" in test


def test_rank_constants_are_the_headers():
    txt = capi.HEADER.read_text()
    m = re.search(r"enum\s*\{\s*LC_RANK_QZ\s*=\s*(\d+),\s*LC_RANK_LOGZ\s*=\s*(\d+),\s*LC_RANK_LOGP\s*=\s*(\d+)\s*\}", txt)
    assert m, "enum { LC_RANK_QZ, LC_RANK_LOGZ, LC_RANK_LOGP } not found in the header"
    assert (capi.RANK_QZ, capi.RANK_LOGZ, capi.RANK_LOGP) == tuple(int(v) for v in m.groups())
    assert capi.TopRows._fields == ("count", "group", "row", "score")


def test_shipped_library_exports_the_entry_points(lib):
    names = capi.declared_symbols()
    shipped = aux_hooks.exported_symbols(aux_hooks.SHIPPED_LIB)
    for n in ("lc_ctx_top_rows", "lc_model_exemplars"):
        assert n in names, f"{n} is not declared in include/libcluster_hip.h"
        assert n in shipped, f"{n} is not exported by the shipped library"
        assert hasattr(lib, n)
