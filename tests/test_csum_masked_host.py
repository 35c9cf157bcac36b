"""The host side of ecg_csum_masked and ecg_recover_masks_csum: the two symbols in the version
script and the header, every argument error in front of the context check, and the pin that the
SURVIVORS selection -- the k lowest cells a set does not name -- is ecg_recov_matrix's dec_idx.
No GPU needed."""
import os
import re
from itertools import combinations

import pytest

from daos_amd import ecg

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
NEW = ("ecg_csum_masked", "ecg_recover_masks_csum")
# device addresses the checks below never dereference
STRIPES, MASKS, RESULT, CSUMS, SRC = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000
K, P, C_, S_ = 4, 2, 4096, 4
NCH = 2                                 # chunks of a cell at chunksize 2048
IMG = S_ * (K + P) * C_                 # bytes of the stripes image
ARR = S_ * (K + P) * NCH * 4            # bytes of a crc32 checksum array


def lowest_clear(mask, k, p):
    """The k lowest cells of 0..k+p-1 the mask does not name."""
    return [c for c in range(k + p) if not mask >> c & 1][:k]


def test_new_symbols_are_exported_and_declared():
    exports = open(os.path.join(ROOT, "daos_amd", "csrc", "exports.map")).read()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ecg_csum.h")).read(), flags=re.S)
    for name in NEW:
        assert re.search(rf"^\s*{name};", exports, flags=re.M), name
        assert re.search(rf"\bint {name}\(", header), name
        assert hasattr(ecg.lib(), name)
        assert name in ecg.EXPORTED
    assert re.search(r"#define\s+ECG_CM_ERASED\s+0x1u", header)
    assert re.search(r"#define\s+ECG_CM_SURVIVORS\s+0x2u", header)
    assert (ecg.CM_ERASED, ecg.CM_SURVIVORS) == (1, 2)
    for method in ("csum_masked", "recover_masks_csum"):
        assert callable(getattr(ecg.Context, method))


def test_prototypes_have_the_issue_argument_counts():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ecg_csum.h")).read(), flags=re.S)
    for name, n in (("ecg_csum_masked", 16), ("ecg_recover_masks_csum", 16)):
        args = re.search(rf"\bint {name}\((.*?)\);", header, flags=re.S).group(1)
        assert len(args.split(",")) == n, name
        assert len(dict((s[0], s) for s in ecg._SIGS)[name][2]) == n


def masked(ctx=None, htype=2, chunksize=2048, rec_size=1, k=K, p=P, C__=C_, S__=S_, stripes=STRIPES,
           masks=MASKS, which=1, csums=CSUMS, result=RESULT, flags=0):
    return ecg.lib().ecg_csum_masked(ctx, htype, chunksize, rec_size, k, p, C__, S__, stripes, (K + P) * C_, masks,
                                     which, csums, result, flags, None)


def composite(ctx=None, k=K, p=P, C__=C_, S__=S_, stripes=STRIPES, masks=MASKS, result=RESULT, flags=0, htype=2,
              chunksize=2048, rec_size=1, csums=CSUMS, src=None):
    return ecg.lib().ecg_recover_masks_csum(ctx, k, p, C__, S__, stripes, (K + P) * C_, masks, result, flags, htype,
                                            chunksize, rec_size, csums, src, None)


# every error below is found with a NULL context, i.e. in front of the context check
MASKED_ERRORS = [
    ({"k": 17}, b"k <= 16"), ({"k": 0}, b"k <= 16"), ({"p": 4}, b"p <= 3"), ({"p": 0}, b"p <= 3"),
    ({"which": 0}, b"which"), ({"which": 4}, b"which"), ({"which": 7}, b"which"),
    ({"flags": 2}, b"flags"), ({"flags": 0x80000000}, b"flags"),
    ({"chunksize": 0}, b"chunksize"), ({"rec_size": 0}, b"rec_size"),
    ({"rec_size": 3}, b"multiple of rec_size"), ({"C__": 4097, "rec_size": 2}, b"multiple of rec_size"),
    ({"masks": None}, b"masks"), ({"masks": MASKS + 2}, b"masks"), ({"masks": None, "S__": 0}, b"masks"),
    ({"result": None}, b"result"), ({"result": RESULT + 4}, b"result"),
    ({"stripes": None}, b"NULL"), ({"csums": None}, b"NULL"),
    ({"csums": STRIPES}, b"overlaps the stripes"), ({"csums": STRIPES + IMG - 1}, b"overlaps the stripes"),
    ({"csums": STRIPES - ARR + 1}, b"overlaps the stripes"),
    ({"csums": MASKS}, b"overlaps the masks"), ({"csums": MASKS + 4 * S_ - 1}, b"overlaps the masks"),
    ({"csums": MASKS - ARR + 1}, b"overlaps the masks"),
]


@pytest.mark.parametrize("kw,what", MASKED_ERRORS, ids=[str(i) for i in range(len(MASKED_ERRORS))])
def test_csum_masked_argument_errors(kw, what):
    L = ecg.lib()
    assert masked(**kw) == -ecg.DER_INVAL, kw
    assert what in L.ecg_strerror(), (kw, L.ecg_strerror())


def test_csum_masked_hash_types_and_the_context_check_last():
    L = ecg.lib()
    for htype in (0, 4, 5, 6, 8, 99, -1):
        assert masked(htype=htype) == -ecg.DER_NOTSUPPORTED, htype
        assert b"hash type" in L.ecg_strerror()
    # arrays that end where the stripes or the masks begin do not overlap them: all four hash
    # types and every `which` then reach the context check
    for kw in ({}, {"csums": STRIPES - ARR}, {"csums": STRIPES + IMG}, {"csums": MASKS + 4 * S_},
               {"csums": MASKS - ARR}, {"which": 2}, {"which": 3}, {"flags": ecg.RM_SPARSE},
               {"htype": 1}, {"htype": 3}, {"htype": 7}, {"S__": 0, "stripes": None, "csums": None},
               {"C__": 0, "stripes": None, "csums": None}, {"rec_size": 4096, "chunksize": 1}):
        assert masked(**kw) == -ecg.DER_INVAL, kw
        assert b"NULL context" in L.ecg_strerror(), (kw, L.ecg_strerror())


COMPOSITE_ERRORS = [
    # the recovery half
    ({"k": 17}, b"k <= 16"), ({"p": 0}, b"p <= 3"), ({"flags": 2}, b"flags"),
    ({"result": None}, b"result"), ({"result": RESULT + 4}, b"result"),
    ({"masks": None}, b"masks"), ({"masks": MASKS + 2}, b"masks"),
    ({"stripes": None}, b"NULL stripes"), ({"masks": STRIPES + 64}, b"masks overlaps the stripes"),
    # the checksum half
    ({"chunksize": 0}, b"chunksize"), ({"rec_size": 0}, b"rec_size"), ({"rec_size": 3}, b"multiple of rec_size"),
    ({"masks": None, "S__": 0}, b"masks"),
    ({"csums": None}, b"NULL"), ({"csums": STRIPES + 8}, b"csums overlaps the stripes"),
    ({"csums": MASKS}, b"csums overlaps the masks"),
    ({"src": STRIPES + 8}, b"src_csums overlaps the stripes"), ({"src": MASKS - 4}, b"src_csums overlaps the masks"),
    ({"src": CSUMS + 4}, b"src_csums must be csums itself"), ({"src": CSUMS - ARR + 1}, b"src_csums must be csums"),
    ({"src": CSUMS + ARR - 1}, b"src_csums must be csums"),
]


@pytest.mark.parametrize("kw,what", COMPOSITE_ERRORS, ids=[str(i) for i in range(len(COMPOSITE_ERRORS))])
def test_recover_masks_csum_argument_errors(kw, what):
    L = ecg.lib()
    assert composite(**kw) == -ecg.DER_INVAL, kw
    assert what in L.ecg_strerror(), (kw, L.ecg_strerror())


def test_recover_masks_csum_hash_types_and_the_context_check_last():
    L = ecg.lib()
    for htype in (0, 4, 99):
        assert composite(htype=htype) == -ecg.DER_NOTSUPPORTED, htype
    for kw in ({}, {"src": SRC}, {"src": CSUMS}, {"src": CSUMS + ARR}, {"src": CSUMS - ARR},
               {"flags": ecg.RM_SPARSE}, {"htype": 1}, {"htype": 3}, {"htype": 7}):
        assert composite(**kw) == -ecg.DER_INVAL, kw
        assert b"NULL context" in L.ecg_strerror(), (kw, L.ecg_strerror())


@pytest.mark.parametrize("k,p", [(4, 2), (8, 2), (8, 3), (16, 3)])
def test_k_lowest_clear_bits_are_recov_matrix_dec_idx(k, p):
    """For every erasure set, listed in ascending order as the set table lists it, the cells
    ecg_recov_matrix reads (dec_idx) are the k lowest the set does not name -- the all-parity
    sets, where it re-encodes from cells 0..k-1, included."""
    all_parity = 0
    for e in range(1, p + 1):
        for cs in combinations(range(k + p), e):
            mask = sum(1 << c for c in cs)
            _, dec, reused = ecg.recov_matrix(k, p, list(cs))
            assert [int(d) for d in dec] == lowest_clear(mask, k, p), cs
            if reused:
                all_parity += 1
                assert cs == tuple(range(k, k + p)) and [int(d) for d in dec] == list(range(k))
    assert all_parity == 1
