"""The host side of ecg_recover_masks and ecg_csum_mask: the numbering of erasure sets
(ecg_erasure_sets, ecg_erasure_set_index), the argument checks that need no device, and the
four new symbols in the version script and the headers.  No GPU needed."""
import math
import os
import re
from itertools import combinations

import pytest

from daos_amd import ecg

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SHAPES = [(2, 1, 3), (4, 2, 21), (8, 2, 55), (16, 2, 171), (8, 3, 231), (16, 3, 1159), (5, 2, 28)]
NEW = ("ecg_recover_masks", "ecg_erasure_sets", "ecg_erasure_set_index", "ecg_csum_mask")
# device addresses the checks below never dereference
STRIPES, MASKS, RESULT, CSUMS = 0x10000000, 0x20000000, 0x30000000, 0x40000000


def bits(cells):
    return sum(1 << c for c in cells)


@pytest.mark.parametrize("k,p,n", SHAPES)
def test_erasure_sets_is_the_sum_of_binomials(k, p, n):
    assert sum(math.comb(k + p, e) for e in range(1, p + 1)) == n
    assert ecg.erasure_sets(k, p) == n


@pytest.mark.parametrize("k,p,n", SHAPES)
def test_erasure_set_index_is_a_bijection(k, p, n):
    idx = [ecg.erasure_set_index(k, p, bits(cs)) for e in range(1, p + 1) for cs in combinations(range(k + p), e)]
    assert len(idx) == n
    assert sorted(idx) == list(range(n))


@pytest.mark.parametrize("k,p,n", SHAPES)
def test_erasure_set_index_of_masks_that_name_no_set(k, p, n):
    L = ecg.lib()
    assert L.ecg_erasure_set_index(k, p, 0) == -1
    assert ecg.erasure_set_index(k, p, 0) == -1
    assert L.ecg_erasure_set_index(k, p, bits(range(p + 1))) == -ecg.DER_DATA_LOSS
    assert L.ecg_erasure_set_index(k, p, bits(range(k - 1, k + p))) == -ecg.DER_DATA_LOSS
    assert L.ecg_erasure_set_index(k, p, 1 << (k + p)) == -ecg.DER_INVAL
    assert L.ecg_erasure_set_index(k, p, 1 | 1 << (k + p)) == -ecg.DER_INVAL
    assert L.ecg_erasure_set_index(k, p, 1 << 31) == -ecg.DER_INVAL
    assert L.ecg_erasure_set_index(k, p, 0xFFFFFFFF) == -ecg.DER_INVAL
    with pytest.raises(ecg.EcgError) as ei:
        ecg.erasure_set_index(k, p, bits(range(p + 1)))
    assert ei.value.rc == -ecg.DER_DATA_LOSS


def test_shape_limits():
    L = ecg.lib()
    for k, p in ((17, 2), (0, 2), (4, 4), (4, 0), (17, 4)):
        assert L.ecg_erasure_sets(k, p) == -ecg.DER_INVAL, (k, p)
        assert L.ecg_erasure_set_index(k, p, 1) == -ecg.DER_INVAL, (k, p)
        assert L.ecg_recover_masks(None, k, p, 4096, 4, STRIPES, (k + p) * 4096, MASKS, RESULT, 0,
                                   None) == -ecg.DER_INVAL
        assert b"k <= 16" in L.ecg_strerror() and b"p <= 3" in L.ecg_strerror()     # names the limit
    with pytest.raises(ecg.EcgError):
        ecg.erasure_sets(17, 2)


def test_recover_masks_argument_checks():
    L = ecg.lib()

    def call(ctx=None, masks=MASKS, result=RESULT, flags=0):
        return L.ecg_recover_masks(ctx, 4, 2, 4096, 4, STRIPES, 6 * 4096, masks, result, flags, None)

    for kw, what in (({}, b"NULL context"), ({"result": RESULT + 4}, b"result"), ({"result": None}, b"result"),
                     ({"masks": MASKS + 2}, b"masks"), ({"masks": None}, b"masks"), ({"flags": 2}, b"flags")):
        assert call(**kw) == -ecg.DER_INVAL, kw
        assert what in L.ecg_strerror(), (kw, L.ecg_strerror())


def test_csum_mask_argument_checks():
    L = ecg.lib()

    def call(htype=2, ncells=6, first=0, masks=MASKS):
        return L.ecg_csum_mask(None, htype, CSUMS, CSUMS + 4096, 4, ncells, 1, 6, 1, first, masks, None)

    for kw, what in (({}, b"NULL context"), ({"first": 27}, b"> 32"), ({"first": 32, "ncells": 1}, b"> 32"),
                     ({"ncells": 33}, b"> 32"), ({"first": 0xFFFFFFFF, "ncells": 2}, b"> 32"),
                     ({"htype": 0}, b"hash type"), ({"htype": 99}, b"hash type"),
                     ({"masks": None}, b"masks"), ({"masks": MASKS + 1}, b"masks")):
        assert call(**kw) == -ecg.DER_INVAL, kw
        assert what in L.ecg_strerror(), (kw, L.ecg_strerror())
    assert call(first=26) == -ecg.DER_INVAL and b"NULL context" in L.ecg_strerror()  # 26 + 6 == 32 fits


def test_new_symbols_are_exported_and_declared():
    exports = open(os.path.join(ROOT, "daos_amd", "csrc", "exports.map")).read()
    headers = {h: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", h)).read(), flags=re.S)
               for h in ("ecg.h", "ecg_csum.h")}
    for name in NEW:
        assert re.search(rf"^\s*{name};", exports, flags=re.M), name
        home = "ecg_csum.h" if name == "ecg_csum_mask" else "ecg.h"
        assert re.search(rf"\bint {name}\(", headers[home]), name
        assert hasattr(ecg.lib(), name)
    assert re.search(r"#define\s+ECG_RM_SPARSE\s+0x1u", headers["ecg.h"])
    assert ecg.RM_SPARSE == 1
    for method in ("recover_masks", "csum_mask"):
        assert callable(getattr(ecg.Context, method))
