"""The host side of ecg_matmul_ptrs_lens and ecg_obj_ec_singv_encode_dev: the launch plan
(ecg_lens_plan) against a restatement, the argument checks that come before the context check, in
their documented order, and the symbols in the version script, the headers and the bindings.  The
addresses are never dereferenced.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

from daos_amd import ecg

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CELLS, VALUES, PARITY = 0x10000000, 0x20000000, 0x30000000
SPAN, COL = 65536, 4096
OC_8P2, OC_REPL = (37 << 24) | 1, (1 << 24) | 1


def plan_py(lens):
    """include/ecg.h: ceil(L / 64 KiB) spans per stripe; the most 4 KiB columns in any span."""
    spans = sum(-(-L // SPAN) for L in lens)
    cols = max([min(16, -(-L // COL)) for L in lens if L] or [0])
    return spans, cols


LENGTHS = [0, 1, 4095, 4096, 4097, 65536, 65537, 3 * 65536 + 4096 + 5]


def test_span_is_16_columns():
    header = open(os.path.join(ROOT, "include", "ecg.h")).read()
    assert re.search(r"#define ECG_LENS_SPAN_BYTES 65536u", header)
    assert ecg.LENS_SPAN_BYTES == SPAN == 16 * COL


@pytest.mark.parametrize("lens", [[L] for L in LENGTHS] + [LENGTHS, LENGTHS[::-1], [0, 0, 0], [], [0, 4097, 0, 1],
                                                          [65535, 65536 + 4096], [8192, 8193]])
def test_lens_plan(lens):
    assert ecg.lens_plan(lens) == plan_py(lens)


def test_lens_plan_values():
    """The restatement itself, by hand: one span of one column up to 4096 bytes, a second column at
    4097, 16 columns at 64 KiB, a second span of one column one byte later, and 3 * 64 KiB + 4 KiB
    + 5 as three whole spans and one of two columns."""
    assert [ecg.lens_plan([L]) for L in LENGTHS] == [(0, 0), (1, 1), (1, 1), (1, 1), (1, 2), (1, 16), (2, 16),
                                                      (4, 16)]
    assert ecg.lens_plan([3 * 65536 + 4096 + 5 - 3 * 65536]) == (1, 2)
    assert ecg.lens_plan(LENGTHS) == (11, 16)
    assert ecg.lens_plan([0, 0, 0]) == (0, 0) and ecg.lens_plan([]) == (0, 0)


def test_lens_plan_null_arguments():
    L = ecg.lib()
    lens = (C.c_uint64 * 2)(1, 2)
    n, m = C.c_uint64(7), C.c_uint32(7)
    for args in ((None, 2, C.byref(n), C.byref(m)), (lens, 2, None, C.byref(m)), (lens, 2, C.byref(n), None)):
        assert L.ecg_lens_plan(*args) == -ecg.DER_INVAL
        assert b"lens_plan:" in L.ecg_strerror()
    assert L.ecg_lens_plan(None, 0, C.byref(n), C.byref(m)) == 0 and (n.value, m.value) == (0, 0)
    assert L.ecg_lens_plan(None, 0, None, None) == 0


def lens_call(ctx=None, k=4, rows=2, coef=True, nstripes=3, cells=True, lens=True):
    n = max(1, nstripes * (k + rows))
    arr = (C.c_void_p * n)(*[CELLS + 4096 * i for i in range(n)]) if cells else None
    co = (C.c_ubyte * 128)(*([1] * 128)) if coef else None
    ln = (C.c_uint64 * max(1, nstripes))(*([100, 200, 300] * nstripes)[:nstripes]) if lens else None
    return ecg.lib().ecg_matmul_ptrs_lens(ctx, k, rows, co, nstripes, arr, ln, None)


def lens_fails(what, **kw):
    assert lens_call(**kw) == -ecg.DER_INVAL, kw
    msg = ecg.lib().ecg_strerror()
    assert msg.startswith(b"matmul_ptrs_lens:") and what in msg, (kw, msg)


def test_matmul_ptrs_lens_argument_checks():
    for k, rows in ((0, 2), (17, 2), (4, 0), (4, 9), (17, 9)):
        lens_fails(b"k=%d rows=%d" % (k, rows), k=k, rows=rows)
    lens_fails(b"coef", coef=False)
    lens_fails(b"cell_bytes", lens=False)
    lens_fails(b"NULL context")
    lens_fails(b"NULL context", nstripes=0, lens=False, cells=False)      # nothing is read for an empty batch


def test_matmul_ptrs_lens_checks_come_in_the_documented_order():
    """Each check with every later one failing too (the context stays NULL throughout)."""
    late = {"coef": False, "lens": False, "cells": False}
    lens_fails(b"k=17", k=17, **late)
    lens_fails(b"rows=9", rows=9, **late)
    lens_fails(b"coef", **late)
    del late["coef"]
    lens_fails(b"cell_bytes", **late)
    del late["lens"]
    lens_fails(b"NULL context", **late)                                   # before the cells are looked at


def singv_call(ctx=None, oc=OC_8P2, sizes=(17, 4096, 70001), values=True, parity=True, null_value=None,
               null_parity=None, nvalues=None):
    n = len(sizes) if nvalues is None else nvalues
    sz = (C.c_uint64 * max(1, len(sizes)))(*sizes) if sizes is not None else None
    va = (C.c_void_p * max(1, n))(*[None if i == null_value else VALUES + 0x100000 * i + 1 for i in range(n)])
    pa = (C.c_void_p * max(1, 2 * n))(*[None if i == null_parity else PARITY + 0x100000 * i for i in range(2 * n)])
    return ecg.lib().ecg_obj_ec_singv_encode_dev(ctx, oc, n, sz, va if values else None, pa if parity else None,
                                                 None)


def singv_fails(what, **kw):
    assert singv_call(**kw) == -ecg.DER_INVAL, kw
    msg = ecg.lib().ecg_strerror()
    assert msg.startswith(b"singv_encode_dev:") and what in msg, (kw, msg)


def test_singv_encode_dev_argument_checks():
    singv_fails(b"not an EC class", oc=OC_REPL)
    singv_fails(b"NULL argument", sizes=None, nvalues=3)
    singv_fails(b"NULL argument", values=False)
    singv_fails(b"NULL argument", parity=False)
    singv_fails(b"value 1: zero iod_size", sizes=(17, 0, 70001))
    singv_fails(b"value 2: NULL value", null_value=2)
    singv_fails(b"value 1: NULL parity cell 1", null_parity=3)
    singv_fails(b"NULL context")
    singv_fails(b"NULL context", sizes=(), values=False, parity=False)    # an empty batch reads no array
    singv_fails(b"not an EC class", oc=OC_REPL, sizes=(0,), null_value=0)  # the class comes first


def test_symbols_are_exported_declared_and_bound():
    exports = open(os.path.join(ROOT, "daos_amd", "csrc", "exports.map")).read()
    ecg_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ecg.h")).read(), flags=re.S)
    daos_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ecg_daos.h")).read(), flags=re.S)
    for name, header in (("ecg_matmul_ptrs_lens", ecg_h), ("ecg_lens_plan", ecg_h),
                         ("ecg_obj_ec_singv_encode_dev", daos_h)):
        assert re.search(r"^\s*%s;" % name, exports, flags=re.M)
        assert re.search(r"\bint %s\(" % name, header)
        assert hasattr(ecg.lib(), name) and name in ecg.EXPORTED
    assert callable(ecg.Context.matmul_ptrs_lens) and callable(ecg.Context.singv_encode_dev)
