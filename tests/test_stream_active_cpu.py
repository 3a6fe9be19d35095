"""CPU tests of the sparse live sets (kws_stream_deactivate, kws_stream_activate, kws_stream_active): the boundary carries the three
entries (header, exports, ctypes signatures), the list builder's rule -- restated in tests/_active_ref.py -- gives the ascending list
at word and chunk edges, and the unit that holds the ACTIVE instantiations of the DS-CNN kernel passes the hazard lint."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import _active_ref as ar
from conftest import REPO

native = pytest.importorskip("kws._native")

ENTRIES = {
    "kws_stream_deactivate": (["kws_ctx* ctx", "const int32_t* streams", "int n"], [C.c_void_p, C.c_void_p, C.c_int]),
    "kws_stream_activate": (["kws_ctx* ctx", "const int32_t* streams", "int n"], [C.c_void_p, C.c_void_p, C.c_int]),
    "kws_stream_active": (["kws_ctx* ctx", "uint8_t* out", "int* n_active"], [C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
}


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_header_exports_and_signature_agree(name):
    text = open(os.path.join(REPO, "include", "kws_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.findall(r"\bint\s+" + name + r"\s*\(([^()]*)\)\s*;", text)
    assert len(m) == 1
    params, ctypes_args = ENTRIES[name]
    assert [" ".join(p.split()) for p in m[0].split(",")] == params
    res, args = native.SIGNATURES[name]
    assert res is C.c_int and args == ctypes_args and len(args) == len(params)
    assert hasattr(native.lib(), name)
    assert native.lib().kws_abi_version() == 1
    assert callable(getattr(native.Context, name[len("kws_"):]))


def _bits(S, on):
    a = np.zeros(S, bool)
    a[list(on)] = True
    return a


@pytest.mark.parametrize("S,on,launches", [
    (5, [], []),
    (5, [1, 3, 4], [(0, 0)]),
    (130, [0, 63, 64, 129], [(0, 0)]),                              # bit 63 of word 0, bit 0 of word 1
    (1030, [0, 63, 64, 1023, 1024, 1029], [(0, 0), (1024, 4)]),      # the last stream of chunk 0, the first and last of chunk 1
    (1030, [1024], [(1024, 0)]),                                     # an empty first chunk launches nothing
    (2049, [1023, 2047, 2048], [(0, 0), (1024, 1), (2048, 2)]),
    (70, [s for s in range(70) if s not in (3, 10, 33, 64, 69)], [(0, 0)]),
    (1030, list(range(1030)), [(0, 0), (1024, 1024)]),               # all set
    (1024, list(range(1024)), [(0, 0)]),
])
def test_the_list_builder_at_word_and_chunk_edges(S, on, launches):
    words = ar.mask_words(_bits(S, on))
    assert len(words) == -(-S // 64) and all(0 <= w < 1 << 64 for w in words)
    got, where = ar.build_list(words, S)
    assert got == sorted(on) and where == launches


def test_the_cluster_follows_the_active_count():
    assert [ar.default_cluster(n) for n in (1, 6, 64, 65, 128, 129, 1024)] == [4, 4, 4, 2, 2, 1, 1]


def test_tables_of_a_plan():
    plan = {0: [("deactivate", [0, 2])], 3: [("activate", [2]), ("deactivate", [1])], 4: [("reset", [0])]}
    t = ar.active_table(3, 5, plan)
    assert t.tolist() == [[False, True, False]] * 3 + [[False, False, True]] * 2
    pcm = np.arange(3 * 5 * 2, dtype=np.int16).reshape(3, 10) + 1
    a, b = ar.two_inputs(pcm, t, 2)
    idle = np.repeat(~t.T, 2, axis=1)
    assert (np.abs(a[idle].astype(int)) == 32767).all() and not b[idle].any()
    assert np.array_equal(a[~idle], pcm[~idle]) and np.array_equal(b[~idle], pcm[~idle])
    assert ar.dense_plan(plan)[3] == [("reset", [2]), ("reset", [1])]


def test_the_active_unit_passes_the_hazard_lint():
    """kws_dscnn_active.hip holds the F_STREAM | F_ACTIVE and F_STREAM | F_CLUSTER | F_ACTIVE instantiations (modes 4 and 5) in a
    unit of their own; tests/test_isa_hazards.py lints kws_dscnn.hip, this is the same lint over the new unit."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import isa_hazard_lint as lint

    if not os.path.exists(lint.HIPCC):
        pytest.skip("no hipcc on this machine")
    findings, _, isa = lint.lint_file(os.path.join(REPO, "keyword-spotting_amd", "csrc", "kws_dscnn_active.hip"))
    flat = [(fn[:60], line, rule, msg) for fn, fs in findings.items() for line, rule, msg in fs]
    assert not flat, flat[:5]
    body = open(isa).read()
    kernels = re.findall(r"\.amdhsa_kernel\s+(\S+)", body)
    # <MODE, DIAG, PRECONV, STREAM, CLUSTER, PERSIST, SCAN, ACTIVE>: modes 4 and 5, with and without time tiles, all ACTIVE
    flags = sorted(re.search(r"kws_dscnn_fwd_kernelILi(\d)ELb0ELb0ELb1ELb([01])ELb0ELb0ELb1EE", k).groups() for k in kernels)
    assert flags == [("4", "0"), ("4", "1"), ("5", "0"), ("5", "1")]
    assert body.count("v_mfma_f32_32x32x16_bf16") > 100 and body.count("v_mfma_f32_32x32x16_f16") > 100
