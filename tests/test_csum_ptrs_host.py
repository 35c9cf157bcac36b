"""The host side of the cell-table checksum calls -- ecg_csum_masked_ptrs, ecg_csum_cells_ptrs and
ecg_recover_masks_ptrs_csum: the three symbols in the version script and the header with their
argument counts, and every argument error that needs no context, in the documented order: each is
found with a NULL context, i.e. in front of the context check, and the context check comes before
the table is looked at.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

from daos_amd import ecg

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = {"ecg_csum_masked_ptrs": 15, "ecg_csum_cells_ptrs": 9, "ecg_recover_masks_ptrs_csum": 15}
# device addresses the checks below never dereference
CELLS, MASKS, RESULT, CSUMS, SRC = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
K, P, C_, S_ = 4, 2, 4096, 4
NCH = 2                                 # chunks of a cell at chunksize 2048
ARR = S_ * (K + P) * NCH * 4            # bytes of a crc32 checksum array
TABLE = [CELLS + i * 2 * C_ for i in range(S_ * (K + P))]
NOTHING = object()


def table(cells):
    return None if cells is None else (C.c_void_p * len(cells))(*cells)


def header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ecg_csum.h")).read(), flags=re.S)


def test_new_symbols_are_exported_and_declared():
    exports = open(os.path.join(ROOT, "daos_amd", "csrc", "exports.map")).read()
    for name in NEW:
        assert re.search(rf"^\s*{name};", exports, flags=re.M), name
        assert re.search(rf"\bint {name}\(", header()), name
        assert hasattr(ecg.lib(), name)
        assert name in ecg.EXPORTED
    for method in ("csum_masked_ptrs", "csum_cells_ptrs", "recover_masks_ptrs_csum"):
        assert callable(getattr(ecg.Context, method))


def test_prototypes_have_the_declared_argument_counts():
    for name, n in NEW.items():
        args = re.search(rf"\bint {name}\((.*?)\);", header(), flags=re.S).group(1)
        assert len(args.split(",")) == n, name
        assert len(dict((s[0], s) for s in ecg._SIGS)[name][2]) == n


def masked(ctx=None, htype=2, chunksize=2048, rec_size=1, k=K, p=P, C__=C_, S__=S_, cells=NOTHING, masks=MASKS,
           which=1, csums=CSUMS, result=RESULT, flags=0):
    return ecg.lib().ecg_csum_masked_ptrs(ctx, htype, chunksize, rec_size, k, p, C__, S__,
                                          table(TABLE if cells is NOTHING else cells), masks, which, csums, result,
                                          flags, None)


def every(ctx=None, htype=2, chunksize=2048, rec_size=1, C__=C_, ncells=len(TABLE), cells=NOTHING, csums=CSUMS):
    return ecg.lib().ecg_csum_cells_ptrs(ctx, htype, chunksize, rec_size, C__, ncells,
                                         table(TABLE if cells is NOTHING else cells), csums, None)


def composite(ctx=None, k=K, p=P, C__=C_, S__=S_, cells=NOTHING, masks=MASKS, result=RESULT, flags=0, htype=2,
              chunksize=2048, rec_size=1, csums=CSUMS, src=None):
    return ecg.lib().ecg_recover_masks_ptrs_csum(ctx, k, p, C__, S__, table(TABLE if cells is NOTHING else cells),
                                                 masks, result, flags, htype, chunksize, rec_size, csums, src, None)


# ecg_csum_masked's own checks, in its words; all found with a NULL context
MASKED_ERRORS = [
    ({"k": 17}, b"k <= 16"), ({"k": 0}, b"k <= 16"), ({"p": 4}, b"p <= 3"), ({"p": 0}, b"p <= 3"),
    ({"which": 0}, b"which"), ({"which": 4}, b"which"),
    ({"flags": 2}, b"flags"), ({"flags": 0x80000000}, b"flags"),
    ({"chunksize": 0}, b"chunksize"), ({"rec_size": 0}, b"rec_size"),
    ({"rec_size": 3}, b"multiple of rec_size"), ({"C__": 4097, "rec_size": 2}, b"multiple of rec_size"),
    ({"masks": None}, b"masks"), ({"masks": MASKS + 2}, b"masks"), ({"masks": None, "S__": 0}, b"masks"),
    ({"result": None}, b"result"), ({"result": RESULT + 4}, b"result"),
    ({"csums": None}, b"NULL csums"),
]


@pytest.mark.parametrize("kw,what", MASKED_ERRORS, ids=[str(i) for i in range(len(MASKED_ERRORS))])
def test_csum_masked_ptrs_argument_errors(kw, what):
    L = ecg.lib()
    assert masked(**kw) == -ecg.DER_INVAL, kw
    assert what in L.ecg_strerror(), (kw, L.ecg_strerror())
    assert L.ecg_strerror().startswith(b"csum_masked_ptrs:"), L.ecg_strerror()


def test_csum_masked_ptrs_check_order():
    """An earlier error wins over every later one; the hash type comes first of all, the context
    after ecg_csum_masked's checks and before the table: a NULL table, a NULL entry and an array
    inside a cell all report the NULL context."""
    L = ecg.lib()
    chain = [({"htype": 99}, b"hash type"), ({"k": 17}, b"k <= 16"), ({"which": 4}, b"which"),
             ({"flags": 2}, b"flags"), ({"chunksize": 0}, b"chunksize"), ({"rec_size": 3}, b"multiple of rec_size"),
             ({"masks": MASKS + 2}, b"masks"), ({"result": RESULT + 4}, b"result"), ({"csums": None}, b"NULL csums"),
             ({"cells": None}, b"NULL context")]
    for i, (kw, what) in enumerate(chain):
        later = {}
        for more, _ in chain[i + 1:]:
            later.update(more)
        rc = masked(**{**later, **kw})
        assert rc == (-ecg.DER_NOTSUPPORTED if i == 0 else -ecg.DER_INVAL), kw
        assert what in L.ecg_strerror(), (kw, L.ecg_strerror())
    for htype in (0, 4, 5, 6, 8, 99, -1):
        assert masked(htype=htype) == -ecg.DER_NOTSUPPORTED, htype
        assert b"hash type" in L.ecg_strerror()
    for kw in ({}, {"cells": None}, {"cells": TABLE[:5] + [None] + TABLE[6:]}, {"csums": TABLE[3] + 8},
               {"masks": TABLE[3] + 8}, {"result": TABLE[3] + 8}, {"csums": MASKS}, {"which": 2}, {"which": 3},
               {"flags": ecg.RM_SPARSE}, {"htype": 1}, {"htype": 3}, {"htype": 7},
               {"S__": 0, "cells": None, "csums": None}, {"C__": 0, "cells": None, "csums": None},
               {"rec_size": 4096, "chunksize": 1}):
        assert masked(**kw) == -ecg.DER_INVAL, kw
        assert b"csum_masked_ptrs: NULL context" in L.ecg_strerror(), (kw, L.ecg_strerror())


CELLS_ERRORS = [
    ({"chunksize": 0}, b"chunksize"), ({"rec_size": 0}, b"rec_size"), ({"rec_size": 3}, b"multiple of rec_size"),
    ({"C__": 4097, "rec_size": 2}, b"multiple of rec_size"),
    ({"ncells": 1 << 62}, b"too many checksums"), ({"ncells": (1 << 64) - 1}, b"too many checksums"),
    ({"C__": 1 << 40, "chunksize": 1}, b"too many checksums"),          # more than 2^32 chunks per cell
    ({}, b"NULL context"), ({"cells": None}, b"NULL context"), ({"csums": None}, b"NULL context"),
    ({"cells": [None] + TABLE[1:]}, b"NULL context"), ({"csums": TABLE[0]}, b"NULL context"),
    ({"ncells": 0, "cells": None, "csums": None}, b"NULL context"), ({"htype": 1}, b"NULL context"),
    ({"htype": 3}, b"NULL context"), ({"htype": 7}, b"NULL context"),
]


@pytest.mark.parametrize("kw,what", CELLS_ERRORS, ids=[str(i) for i in range(len(CELLS_ERRORS))])
def test_csum_cells_ptrs_argument_errors(kw, what):
    L = ecg.lib()
    assert every(**kw) == -ecg.DER_INVAL, kw
    assert what in L.ecg_strerror(), (kw, L.ecg_strerror())
    assert L.ecg_strerror().startswith(b"csum_cells_ptrs:"), L.ecg_strerror()


def test_csum_cells_ptrs_hash_type_first():
    L = ecg.lib()
    for htype in (0, 4, 99, -1):
        assert every(htype=htype, chunksize=0, rec_size=0) == -ecg.DER_NOTSUPPORTED, htype
        assert b"hash type" in L.ecg_strerror()
    assert every(chunksize=0, C__=4097, ncells=1 << 62) == -ecg.DER_INVAL       # rcs before the rest
    assert b"chunksize" in L.ecg_strerror()
    assert every(rec_size=3, ncells=1 << 62) == -ecg.DER_INVAL                  # rec_size before the count
    assert b"multiple of rec_size" in L.ecg_strerror()


COMPOSITE_ERRORS = [
    # the recovery half
    ({"k": 17}, b"k <= 16"), ({"p": 0}, b"p <= 3"), ({"flags": 2}, b"flags"),
    ({"result": None}, b"result"), ({"result": RESULT + 4}, b"result"),
    ({"masks": None}, b"masks"), ({"masks": MASKS + 2}, b"masks"),
    # the checksum half
    ({"chunksize": 0}, b"chunksize"), ({"rec_size": 0}, b"rec_size"), ({"rec_size": 3}, b"multiple of rec_size"),
    ({"masks": None, "S__": 0}, b"masks"), ({"csums": None}, b"NULL csums"),
    ({"src": CSUMS + 4}, b"src_csums must be csums itself"), ({"src": CSUMS - ARR + 1}, b"src_csums must be csums"),
    ({"src": CSUMS + ARR - 1}, b"src_csums must be csums"),
]


@pytest.mark.parametrize("kw,what", COMPOSITE_ERRORS, ids=[str(i) for i in range(len(COMPOSITE_ERRORS))])
def test_recover_masks_ptrs_csum_argument_errors(kw, what):
    L = ecg.lib()
    assert composite(**kw) == -ecg.DER_INVAL, kw
    assert what in L.ecg_strerror(), (kw, L.ecg_strerror())
    assert L.ecg_strerror().startswith(b"recover_masks_ptrs_csum:"), L.ecg_strerror()


def test_recover_masks_ptrs_csum_both_halves_before_the_context_check():
    L = ecg.lib()
    for htype in (0, 4, 99):
        assert composite(htype=htype) == -ecg.DER_NOTSUPPORTED, htype
    # the recovery half's errors come before the checksum half's
    assert composite(k=17, htype=99) == -ecg.DER_INVAL and b"k <= 16" in L.ecg_strerror()
    assert composite(result=RESULT + 4, chunksize=0) == -ecg.DER_INVAL and b"result" in L.ecg_strerror()
    assert composite(chunksize=0, src=CSUMS + 4) == -ecg.DER_INVAL and b"chunksize" in L.ecg_strerror()
    for kw in ({}, {"src": SRC}, {"src": CSUMS}, {"src": CSUMS + ARR}, {"src": CSUMS - ARR}, {"cells": None},
               {"cells": [None] + TABLE[1:]}, {"csums": TABLE[2] + 8}, {"src": TABLE[2] + 8},
               {"flags": ecg.RM_SPARSE}, {"htype": 1}, {"htype": 3}, {"htype": 7}):
        assert composite(**kw) == -ecg.DER_INVAL, kw
        assert b"recover_masks_ptrs_csum: NULL context" in L.ecg_strerror(), (kw, L.ecg_strerror())
