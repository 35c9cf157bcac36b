"""The host side of ecg_update_masks: the symbol in the version script, the header and the
binding, its 15 arguments, ECG_UM_PACKED, and every argument error in front of the context
check -- each returned with a NULL context, its message naming the argument.  No GPU needed."""
import os
import re

import pytest

from daos_amd import ecg

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAME = "ecg_update_masks"
# device addresses the checks below never dereference
OLD, NEW, PARITY, MASKS, RESULT = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
K, P, C_, S_ = 4, 2, 4096, 4
PITCH = S_ * C_ + 256                   # a padded row pitch of the client layout [p][S][C]
SPAN = (P - 1) * PITCH + S_ * C_        # bytes from the first parity byte to the last


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ecg.h")).read(), flags=re.S)


def test_symbol_is_exported_declared_and_bound():
    exports = open(os.path.join(ROOT, "daos_amd", "csrc", "exports.map")).read()
    assert re.search(rf"^\s*{NAME};", exports, flags=re.M)
    assert re.search(rf"\bint {NAME}\(", header())
    assert hasattr(ecg.lib(), NAME)
    assert NAME in ecg.EXPORTED
    assert callable(ecg.Context.update_masks)


def test_prototype_has_15_arguments():
    args = re.search(rf"\bint {NAME}\((.*?)\);", header(), flags=re.S).group(1)
    assert len(args.split(",")) == 15
    assert len(dict((s[0], s) for s in ecg._SIGS)[NAME][2]) == 15


def test_um_packed_is_0x2():
    assert re.search(r"#define\s+ECG_UM_PACKED\s+0x2u", header())
    assert re.search(r"#define\s+ECG_RM_SPARSE\s+0x1u", header())
    assert (ecg.UM_PACKED, ecg.RM_SPARSE) == (2, 1)


def call(ctx=None, k=K, p=P, C__=C_, S__=S_, old=OLD, new=NEW, parity=PARITY, masks=MASKS, result=RESULT, flags=0):
    return ecg.lib().ecg_update_masks(ctx, k, p, C__, S__, old, new, K * C_, parity, PITCH, C_, masks, result, flags,
                                      None)


ERRORS = [
    ({"k": 17}, b"k <= 16"), ({"k": 0}, b"k <= 16"), ({"p": 9}, b"p <= 8"), ({"p": 0}, b"p <= 8"),
    ({"flags": 4}, b"flags"), ({"flags": 0x80000000}, b"flags"), ({"flags": 7}, b"flags"),
    ({"masks": None}, b"masks"), ({"masks": MASKS + 2}, b"masks"), ({"masks": MASKS + 1}, b"masks"),
    ({"result": None}, b"result"), ({"result": RESULT + 4}, b"result"),
    # an empty batch still rejects them
    ({"masks": None, "S__": 0}, b"masks"), ({"masks": MASKS + 2, "S__": 0}, b"masks"),
    ({"result": None, "S__": 0}, b"result"), ({"result": RESULT + 4, "S__": 0}, b"result"),
    ({"old": None}, b"old_cells"), ({"new": None}, b"new_cells"), ({"parity": None}, b"parity"),
    # masks or result inside the byte span of the parity (the pad between two rows included)
    ({"masks": PARITY}, b"masks overlaps the parity"), ({"masks": PARITY + SPAN - 4}, b"masks overlaps the parity"),
    ({"masks": PARITY - 4 * S_ + 4}, b"masks overlaps the parity"),
    ({"masks": PARITY + S_ * C_ + 64}, b"masks overlaps the parity"),
    ({"result": PARITY}, b"result overlaps the parity"), ({"result": PARITY + SPAN - 8}, b"result overlaps the parity"),
    ({"result": PARITY - 24}, b"result overlaps the parity"),
]


@pytest.mark.parametrize("kw,what", ERRORS, ids=[str(i) for i in range(len(ERRORS))])
def test_argument_errors_come_before_the_context_check(kw, what):
    L = ecg.lib()
    assert call(**kw) == -ecg.DER_INVAL, kw
    assert what in L.ecg_strerror(), (kw, L.ecg_strerror())
    assert b"NULL context" not in L.ecg_strerror()


def test_valid_arguments_reach_the_context_check():
    """Both flags, the limits themselves, arrays that end where the parity begins or begin where
    it ends, old == new and old_cells interleaved with the parity all pass the argument checks."""
    L = ecg.lib()
    for kw in ({}, {"flags": ecg.UM_PACKED}, {"flags": ecg.RM_SPARSE}, {"flags": ecg.UM_PACKED | ecg.RM_SPARSE},
               {"k": 16, "p": 8}, {"k": 1, "p": 1}, {"masks": PARITY - 4 * S_}, {"masks": PARITY + SPAN},
               {"result": PARITY - 32}, {"result": PARITY + SPAN}, {"new": OLD}, {"old": PARITY - K * C_},
               {"S__": 0}, {"C__": 0}, {"S__": 0, "masks": PARITY}, {"C__": 0, "result": PARITY}):
        assert call(**kw) == -ecg.DER_INVAL, kw
        assert b"NULL context" in L.ecg_strerror(), (kw, L.ecg_strerror())
