"""The host side of ecg_verify_ptrs, ecg_repair_ptrs and ecg_scrub_ptrs: the argument checks that
need no device, in their documented order and named after the call, and the symbols in the
version script, the header and the bindings.  The addresses are never dereferenced.  No GPU
needed."""
import ctypes as C
import os
import re

import pytest

from daos_amd import ecg

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CELLS, STATUS, RESULT, RESULT2 = 0x10000000, 0x20000000, 0x30000000, 0x30000100
CALLS = ["verify_ptrs", "repair_ptrs", "scrub_ptrs"]


def call(fn, ctx=None, k=4, p=2, status=STATUS, result=RESULT, result2=RESULT2, nstripes=4, cell_bytes=4096,
         cells=True):
    n = max(1, nstripes * (k + p))
    arr = (C.c_void_p * n)(*[CELLS + 4096 * i for i in range(n)]) if cells else None
    f = getattr(ecg.lib(), "ecg_" + fn)
    if fn == "scrub_ptrs":
        return f(ctx, k, p, cell_bytes, nstripes, arr, status, result, result2, None)
    return f(ctx, k, p, cell_bytes, nstripes, arr, status, result, None)


def fails(fn, what, **kw):
    assert call(fn, **kw) == -ecg.DER_INVAL, (fn, kw)
    msg = ecg.lib().ecg_strerror()
    assert msg.startswith(fn.encode() + b": "), (fn, kw, msg)          # prefixed by the call's name
    assert what in msg, (fn, kw, msg)


@pytest.mark.parametrize("fn", CALLS)
def test_shape_limits(fn):
    for k, p in ((17, 2), (0, 2), (4, 9), (4, 0), (17, 9), (-1, 2), (4, -1)):
        fails(fn, b"k=%d p=%d outside 1..16 / 1..8" % (k, p), k=k, p=p)
    for k, p in ((16, 8), (1, 1), (5, 4)):                              # inside: the next check answers
        fails(fn, b"NULL context", k=k, p=p)


@pytest.mark.parametrize("fn", CALLS)
def test_argument_checks(fn):
    fails(fn, b"NULL context")
    fails(fn, b"result must be 8-byte aligned", result=RESULT + 4)
    fails(fn, b"result must be 8-byte aligned", result=None)
    fails(fn, b"status must be 4-byte aligned", status=STATUS + 2)
    fails(fn, b"status must be 4-byte aligned", status=None)
    fails(fn, b"NULL context", status=None, nstripes=0)                 # no status is read for an empty batch
    fails(fn, b"NULL context", status=STATUS + 2, nstripes=0)
    fails(fn, b"NULL context", cells=False)                             # the context comes before the cells
    fails(fn, b"NULL context", cells=False, cell_bytes=0)


def test_scrub_takes_two_different_results():
    fails("scrub_ptrs", b"verify_result must be 8-byte aligned", result=RESULT + 4)
    fails("scrub_ptrs", b"verify_result must be 8-byte aligned", result=None)
    fails("scrub_ptrs", b"repair_result must be 8-byte aligned", result2=RESULT2 + 4)
    fails("scrub_ptrs", b"repair_result must be 8-byte aligned", result2=None)
    fails("scrub_ptrs", b"same address", result2=RESULT)
    # verify_result first, then repair_result, then the two being one
    fails("scrub_ptrs", b"verify_result", result=None, result2=None)
    fails("scrub_ptrs", b"repair_result", result=RESULT, result2=RESULT + 4)
    fails("scrub_ptrs", b"verify_result", result=RESULT + 4, result2=RESULT + 4)


@pytest.mark.parametrize("fn", CALLS)
def test_argument_checks_come_in_the_documented_order(fn):
    """Each check with every later one failing too (the context stays NULL throughout)."""
    late = {"result": RESULT + 4, "status": None, "cells": False}
    if fn == "scrub_ptrs":
        late["result2"] = RESULT + 4
    fails(fn, b"k=17", k=17, **late)
    fails(fn, b"p=9", p=9, **late)
    fails(fn, b"verify_result" if fn == "scrub_ptrs" else b"result must be", **late)
    late["result"] = RESULT
    if fn == "scrub_ptrs":
        fails(fn, b"repair_result", **late)
        late["result2"] = RESULT
        fails(fn, b"same address", **late)
        late["result2"] = RESULT2
    fails(fn, b"status must be", **late)
    late["status"] = STATUS + 1
    fails(fn, b"status must be", **late)
    late["status"] = STATUS
    fails(fn, b"NULL context", **late)                                  # before the cells are looked at


@pytest.mark.parametrize("fn", CALLS)
def test_symbol_is_exported_declared_and_bound(fn):
    exports = open(os.path.join(ROOT, "daos_amd", "csrc", "exports.map")).read()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ecg.h")).read(), flags=re.S)
    assert re.search(r"^\s*ecg_%s;" % fn, exports, flags=re.M)
    assert re.search(r"\bint ecg_%s\(" % fn, header)
    assert hasattr(ecg.lib(), "ecg_" + fn)
    assert callable(getattr(ecg.Context, fn))

