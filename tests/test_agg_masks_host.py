"""The host side of ecg_agg_masks / ecg_agg_masks_ptrs: the symbols in the version script, the
header and the binding, their 16 and 11 arguments, ECG_AGG_AUTO, ecg_agg_threshold over every
shape, and every argument error in front of the context check -- each returned with a NULL
context in the documented order, its message prefixed with the call's name.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

from daos_amd import ecg

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NAMES = ("ecg_agg_masks", "ecg_agg_masks_ptrs")
# device addresses the checks below never dereference
OLD, NEW, PARITY, MASKS, RESULT = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
K, P, C_, S_ = 4, 2, 4096, 4
PITCH = S_ * C_ + 256                   # a padded row pitch of the client layout [p][S][C]
SPAN = (P - 1) * PITCH + S_ * C_        # bytes from the first parity byte to the last


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ecg.h")).read(), flags=re.S)


def test_symbols_are_exported_declared_and_bound():
    exports = open(os.path.join(ROOT, "daos_amd", "csrc", "exports.map")).read()
    for name in NAMES + ("ecg_agg_threshold",):
        assert hasattr(ecg.lib(), name)
        assert re.search(rf"^\s*{name};", exports, flags=re.M)
        assert re.search(rf"\bint {name}\(", header())
        assert name in ecg.EXPORTED
    assert callable(ecg.Context.agg_masks) and callable(ecg.Context.agg_masks_ptrs)


@pytest.mark.parametrize("name,n", zip(NAMES, (16, 11)))
def test_prototypes_have_16_and_11_arguments(name, n):
    args = re.search(rf"\bint {name}\((.*?)\);", header(), flags=re.S).group(1)
    assert len(args.split(",")) == n
    assert len(dict((s[0], s) for s in ecg._SIGS)[name][2]) == n


def test_launcher_reports_the_kernel_name():
    """ecg_k_launch_agg_masks, declared beside its host callers, hands the kernel's name back as
    the launchers of ecg_kabi.h do, and is defined extern "C" with the same arguments."""
    csrc = os.path.join(ROOT, "daos_amd", "csrc")
    host = re.sub(r"/\*.*?\*/", "", open(os.path.join(csrc, "host", "ecg_internal.h")).read(), flags=re.S)
    kern = open(os.path.join(csrc, "kernels", "ecg_update_masks_kernels.hip")).read()
    decl = re.search(r"\bint ecg_k_launch_agg_masks\(([^;]*?)\);", host, flags=re.S).group(1)
    defn = re.search(r'extern "C" int ecg_k_launch_agg_masks\(([^{]*?)\)\s*\{', kern, flags=re.S).group(1)
    assert " ".join(decl.split()) == " ".join(defn.split())
    assert " ".join(decl.split(",")[-1].split()) == "const char **kernel"


def test_agg_auto_is_all_ones():
    assert re.search(r"#define\s+ECG_AGG_AUTO\s+0xffffffffu", header())
    assert ecg.AGG_AUTO == 0xFFFFFFFF


def test_threshold_is_the_arithmetic_break_even():
    L = ecg.lib()
    for k in range(1, 17):
        for p in range(1, 9):
            want = (k - p) // 2 if k > p else 0
            assert L.ecg_agg_threshold(k, p) == want == ecg.agg_threshold(k, p), (k, p)
            # the delta's (2n + 2p) cells against the re-encode's (k + p): the tie to the delta
            assert all((2 * n + 2 * p <= k + p) == (n <= want) for n in range(1, k + 1)), (k, p)
    for k, p in ((0, 1), (17, 2), (4, 0), (4, 9), (-1, 2)):
        assert L.ecg_agg_threshold(k, p) == -ecg.DER_INVAL, (k, p)
        with pytest.raises(ecg.EcgError):
            ecg.agg_threshold(k, p)


def call(ctx=None, k=K, p=P, C__=C_, S__=S_, old=OLD, new=NEW, parity=PARITY, masks=MASKS, result=RESULT, T=1,
         flags=0):
    return ecg.lib().ecg_agg_masks(ctx, k, p, C__, S__, old, new, K * C_, parity, PITCH, C_, masks, result, T, flags,
                                   None)


def call_ptrs(ctx=None, k=K, p=P, C__=C_, S__=S_, cells=None, masks=MASKS, result=RESULT, T=1, flags=0):
    return ecg.lib().ecg_agg_masks_ptrs(ctx, k, p, C__, S__, cells, masks, result, T, flags, None)


COMMON = [
    ({"k": 17}, b"k <= 16"), ({"k": 0}, b"k <= 16"), ({"p": 9}, b"p <= 8"), ({"p": 0}, b"p <= 8"),
    ({"flags": 4}, b"unknown flags"), ({"flags": 0x80000000}, b"unknown flags"), ({"flags": 7}, b"unknown flags"),
    ({"flags": ecg.UM_PACKED}, b"ECG_UM_PACKED"), ({"flags": ecg.UM_PACKED | ecg.RM_SPARSE}, b"ECG_UM_PACKED"),
    ({"T": K + 1}, b"recalc_above"), ({"T": 0xFFFFFFFE}, b"recalc_above"), ({"T": 17, "k": 16}, b"recalc_above"),
    ({"T": 2, "k": 1}, b"recalc_above"),
    ({"masks": None}, b"masks"), ({"masks": MASKS + 2}, b"masks"), ({"masks": MASKS + 1}, b"masks"),
    ({"result": None}, b"result"), ({"result": RESULT + 4}, b"result"),
    # an empty batch still rejects them
    ({"masks": None, "S__": 0}, b"masks"), ({"masks": MASKS + 2, "S__": 0}, b"masks"),
    ({"result": None, "S__": 0}, b"result"), ({"result": RESULT + 4, "S__": 0}, b"result"),
    ({"T": K + 1, "S__": 0}, b"recalc_above"),
]
STRIDED = COMMON + [
    ({"old": None}, b"old_cells"), ({"new": None}, b"new_cells"), ({"parity": None}, b"parity"),
    # masks or result inside the byte span of the parity (the pad between two rows included)
    ({"masks": PARITY}, b"masks overlaps the parity"), ({"masks": PARITY + SPAN - 4}, b"masks overlaps the parity"),
    ({"masks": PARITY - 4 * S_ + 4}, b"masks overlaps the parity"),
    ({"masks": PARITY + S_ * C_ + 64}, b"masks overlaps the parity"),
    ({"result": PARITY}, b"result overlaps the parity"), ({"result": PARITY + SPAN - 8}, b"result overlaps the parity"),
    ({"result": PARITY - 24}, b"result overlaps the parity"),
]


@pytest.mark.parametrize("kw,what", STRIDED, ids=[str(i) for i in range(len(STRIDED))])
def test_argument_errors_come_before_the_context_check(kw, what):
    L = ecg.lib()
    assert call(**kw) == -ecg.DER_INVAL, kw
    assert what in L.ecg_strerror(), (kw, L.ecg_strerror())
    assert L.ecg_strerror().startswith(b"agg_masks: ")
    assert b"NULL context" not in L.ecg_strerror()


@pytest.mark.parametrize("kw,what", COMMON, ids=[str(i) for i in range(len(COMMON))])
def test_ptrs_argument_errors_come_before_the_context_check(kw, what):
    L = ecg.lib()
    assert call_ptrs(**kw) == -ecg.DER_INVAL, kw
    assert what in L.ecg_strerror(), (kw, L.ecg_strerror())
    assert L.ecg_strerror().startswith(b"agg_masks_ptrs: ")
    assert b"NULL context" not in L.ecg_strerror()


ORDER = [   # each call breaks the rule named and every later one: the earliest is reported
    ({"k": 17, "flags": 4, "T": 99, "masks": None, "result": None, "old": None}, b"k <= 16"),
    ({"flags": 4 | ecg.UM_PACKED, "T": 99, "masks": None, "result": None, "old": None}, b"unknown flags"),
    ({"flags": ecg.UM_PACKED, "T": 99, "masks": None, "result": None, "old": None}, b"ECG_UM_PACKED"),
    ({"T": 99, "masks": None, "result": None, "old": None}, b"recalc_above"),
    ({"masks": None, "result": None, "old": None}, b"masks must"),
    ({"result": None, "old": None, "parity": None}, b"result must"),
    ({"old": None, "new": None, "parity": None}, b"NULL old_cells"),
    ({"new": None, "parity": None}, b"NULL new_cells"),
    ({"parity": None}, b"NULL parity"),
    ({"masks": PARITY, "result": PARITY + 64}, b"masks overlaps"),
    ({"result": PARITY + 64}, b"result overlaps"),
]


@pytest.mark.parametrize("kw,what", ORDER, ids=[str(i) for i in range(len(ORDER))])
def test_argument_errors_are_reported_in_the_documented_order(kw, what):
    L = ecg.lib()
    assert call(**kw) == -ecg.DER_INVAL, kw
    assert what in L.ecg_strerror(), (kw, L.ecg_strerror())
    if what.startswith((b"NULL", b"masks overlaps", b"result overlaps")):
        return                                                  # the strided operands: that form alone
    assert call_ptrs(**{n: v for n, v in kw.items() if n not in ("old", "new", "parity")}) == -ecg.DER_INVAL, kw
    assert what in L.ecg_strerror(), (kw, L.ecg_strerror())


def test_valid_arguments_reach_the_context_check():
    """Every threshold 0 .. k and ECG_AGG_AUTO, the sparse flag, the limits themselves, arrays that
    end where the parity begins or begin where it ends, old == new and old_cells interleaved with
    the parity all pass the argument checks."""
    L = ecg.lib()
    cells = (C.c_void_p * (S_ * (2 * K + P)))(*[OLD] * (S_ * (2 * K + P)))
    for kw in ({}, {"T": 0}, {"T": K}, {"T": ecg.AGG_AUTO}, {"flags": ecg.RM_SPARSE}, {"k": 16, "p": 8, "T": 16},
               {"k": 1, "p": 1, "T": 1}, {"k": 2, "p": 3, "T": ecg.AGG_AUTO}, {"S__": 0}, {"C__": 0},
               {"S__": 0, "T": ecg.AGG_AUTO}):
        assert call(**kw) == -ecg.DER_INVAL, kw
        assert L.ecg_strerror() == b"agg_masks: NULL context", (kw, L.ecg_strerror())
        for c in (None, cells):
            assert call_ptrs(cells=c, **kw) == -ecg.DER_INVAL, kw
            assert L.ecg_strerror() == b"agg_masks_ptrs: NULL context", (kw, L.ecg_strerror())
    for kw in ({"masks": PARITY - 4 * S_}, {"masks": PARITY + SPAN}, {"result": PARITY - 32},
               {"result": PARITY + SPAN}, {"new": OLD}, {"old": PARITY - K * C_}, {"S__": 0, "masks": PARITY},
               {"C__": 0, "result": PARITY}):
        assert call(**kw) == -ecg.DER_INVAL, kw
        assert L.ecg_strerror() == b"agg_masks: NULL context", (kw, L.ecg_strerror())
