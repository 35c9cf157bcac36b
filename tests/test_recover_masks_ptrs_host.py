"""The host side of ecg_recover_masks_ptrs: the argument checks that need no device, in their
documented order, and the symbol in the version script, the header and the bindings.  The
addresses are never dereferenced.  No GPU needed."""
import ctypes as C
import os
import re

from daos_amd import ecg

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CELLS, MASKS, RESULT, CTX = 0x10000000, 0x20000000, 0x30000000, 0x40000000


def call(ctx=None, k=4, p=2, masks=MASKS, result=RESULT, flags=0, nstripes=4, cells=True):
    n = max(1, nstripes * (k + p))
    arr = (C.c_void_p * n)(*[CELLS + 4096 * i for i in range(n)]) if cells else None
    return ecg.lib().ecg_recover_masks_ptrs(ctx, k, p, 4096, nstripes, arr, masks, result, flags, None)


def fails(what, **kw):
    assert call(**kw) == -ecg.DER_INVAL, kw
    assert what in ecg.lib().ecg_strerror(), (kw, ecg.lib().ecg_strerror())


def test_shape_limits():
    for k, p in ((17, 2), (0, 2), (4, 4), (4, 0), (17, 4)):
        fails(b"k <= 16", k=k, p=p)
        fails(b"p <= 3", k=k, p=p)


def test_argument_checks():
    fails(b"NULL context")
    fails(b"result", result=RESULT + 4)
    fails(b"result", result=None)
    fails(b"masks", masks=MASKS + 2)
    fails(b"masks", masks=None)
    fails(b"flags", flags=2)
    fails(b"flags", flags=0x80000000)
    fails(b"NULL context", masks=None, nstripes=0)              # no masks are read for an empty batch


def test_argument_checks_come_in_the_documented_order():
    """Each check with every later one failing too (the context stays NULL throughout)."""
    late = {"flags": 4, "result": RESULT + 4, "masks": None, "cells": False}
    fails(b"k <= 16", k=17, **late)
    fails(b"p <= 3", p=4, **late)
    fails(b"flags", **late)
    del late["flags"]
    fails(b"result", **late)
    del late["result"]
    fails(b"masks", **late)
    del late["masks"]
    fails(b"NULL context", **late)                              # before the cells are looked at


def test_symbol_is_exported_declared_and_bound():
    exports = open(os.path.join(ROOT, "daos_amd", "csrc", "exports.map")).read()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ecg.h")).read(), flags=re.S)
    assert re.search(r"^\s*ecg_recover_masks_ptrs;", exports, flags=re.M)
    assert re.search(r"\bint ecg_recover_masks_ptrs\(", header)
    assert hasattr(ecg.lib(), "ecg_recover_masks_ptrs")
    assert callable(ecg.Context.recover_masks_ptrs)
