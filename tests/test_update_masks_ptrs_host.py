"""The host side of ecg_update_masks_ptrs: the symbol in the version script, the header and the
binding, its 10 arguments, and every argument error in front of the context check -- each returned
with a NULL context, its message prefixed by the call's name.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

from daos_amd import ecg

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAME = "ecg_update_masks_ptrs"
PREFIX = b"update_masks_ptrs:"
# device addresses the checks below never dereference
MASKS, RESULT = 0x40000000, 0x50000000
K, P, C_, S_ = 4, 2, 4096, 4


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ecg.h")).read(), flags=re.S)


def test_symbol_is_exported_declared_and_bound():
    exports = open(os.path.join(ROOT, "daos_amd", "csrc", "exports.map")).read()
    assert re.search(rf"^\s*{NAME};", exports, flags=re.M)
    assert re.search(rf"\bint {NAME}\(", header())
    assert hasattr(ecg.lib(), NAME)
    assert NAME in ecg.EXPORTED
    assert callable(ecg.Context.update_masks_ptrs)


def test_prototype_has_10_arguments():
    args = re.search(rf"\bint {NAME}\((.*?)\);", header(), flags=re.S).group(1)
    assert len(args.split(",")) == 10
    assert len(dict((s[0], s) for s in ecg._SIGS)[NAME][2]) == 10


def call(ctx=None, k=K, p=P, C__=C_, S__=S_, masks=MASKS, result=RESULT, flags=0):
    n = S_ * (2 * k + p)
    cells = (C.c_void_p * n)(*[0x10000000 + i * 2 * C_ for i in range(n)])
    return ecg.lib().ecg_update_masks_ptrs(ctx, k, p, C__, S__, cells, masks, result, flags, None)


ERRORS = [
    ({"k": 17}, b"k <= 16"), ({"k": 0}, b"k <= 16"), ({"p": 9}, b"p <= 8"), ({"p": 0}, b"p <= 8"),
    ({"flags": 4}, b"unknown flags"), ({"flags": 0x80000000}, b"unknown flags"),
    ({"flags": ecg.UM_PACKED}, b"ECG_UM_PACKED"), ({"flags": ecg.UM_PACKED | ecg.RM_SPARSE}, b"ECG_UM_PACKED"),
    ({"masks": None}, b"masks"), ({"masks": MASKS + 2}, b"masks"), ({"masks": MASKS + 1}, b"masks"),
    ({"result": None}, b"result"), ({"result": RESULT + 4}, b"result"),
    # an empty batch still rejects them
    ({"masks": None, "S__": 0}, b"masks"), ({"masks": MASKS + 2, "S__": 0}, b"masks"),
    ({"result": None, "S__": 0}, b"result"), ({"result": RESULT + 4, "S__": 0}, b"result"),
]


@pytest.mark.parametrize("kw,what", ERRORS, ids=[str(i) for i in range(len(ERRORS))])
def test_argument_errors_come_before_the_context_check(kw, what):
    L = ecg.lib()
    assert call(**kw) == -ecg.DER_INVAL, kw
    msg = L.ecg_strerror()
    assert msg.startswith(PREFIX), (kw, msg)
    assert what in msg, (kw, msg)
    assert b"NULL context" not in msg


def test_the_checks_come_in_the_documented_order():
    """limits, flags, masks, result: each earlier error wins over every later one."""
    L = ecg.lib()
    later = {"flags": 4, "masks": None, "result": None}
    for kw, what in (({"k": 17}, b"k <= 16"), ({}, b"unknown flags")):
        assert call(**dict(later, **kw)) == -ecg.DER_INVAL
        assert what in L.ecg_strerror(), L.ecg_strerror()
    assert call(masks=None, result=None) == -ecg.DER_INVAL
    assert b"masks" in L.ecg_strerror()


def test_valid_arguments_reach_the_context_check():
    L = ecg.lib()
    for kw in ({}, {"flags": ecg.RM_SPARSE}, {"k": 16, "p": 8}, {"k": 1, "p": 1}, {"S__": 0}, {"C__": 0},
               {"S__": 0, "C__": 0}):
        assert call(**kw) == -ecg.DER_INVAL, kw
        assert L.ecg_strerror() == PREFIX + b" NULL context", (kw, L.ecg_strerror())
