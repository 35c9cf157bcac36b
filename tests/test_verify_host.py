"""ecg_verify's host side, no GPU: the algebra bad-cell location rests on
(the Cauchy1 ratios g[r][j] / g[0][j] are pairwise distinct over j), the
ecg_verify_cell truth table, the exports and the NULL-context path."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
CLASSES = [(k, p) for k in (2, 4, 8, 16) for p in (2, 3)] + [(5, 2)]


def st(rows: int, cand: int) -> int:
    """A status word: rows in bits 0-7, candidate data cells in bits 8-23."""
    return (rows & 0xff) | ((cand & 0xffff) << 8)


@pytest.mark.parametrize("k,p", CLASSES)
def test_cauchy_ratios_injective(ecglib, k, p):
    """A data cell j wrong by e gives the syndrome s_r = g[r][j] * e, so cell
    j' explains it iff g[r][j'] / g[0][j'] == g[r][j] / g[0][j]: location
    needs those ratios pairwise distinct over j for each r >= 1."""
    g = ecglib.cauchy1(k, p)[k:]
    assert g.min() > 0                           # every parity row sees every data cell
    for j in range(k):                           # ... so a wrong data cell dirties all p rows
        assert ecglib.verify_cell(st((1 << p) - 1, 1 << j), k, p) == j
    for r in range(1, p):
        ratios = [ecglib.gf_mul(int(g[r][j]), ecglib.gf_inv(int(g[0][j]))) for j in range(k)]
        assert len(set(ratios)) == k, (r, ratios)
        for a, b in itertools.combinations(range(k), 2):    # the form the kernel tests
            for e in (1, 0x53, 0xff):
                s0, sr = ecglib.gf_mul(int(g[0][a]), e), ecglib.gf_mul(int(g[r][a]), e)
                assert ecglib.gf_mul(int(g[0][a]), sr) == ecglib.gf_mul(int(g[r][a]), s0)
                assert ecglib.gf_mul(int(g[0][b]), sr) != ecglib.gf_mul(int(g[r][b]), s0)


@pytest.mark.parametrize("k,p", [(2, 2), (4, 2), (8, 2), (16, 2), (8, 3), (16, 3), (5, 2)])
def test_verify_cell_truth_table(ecglib, k, p):
    vc = ecglib.verify_cell
    allrows, allcand = (1 << p) - 1, (1 << k) - 1
    assert vc(st(0, allcand), k, p) == -1                     # clean, as the host presets it
    assert vc(st(0, 0), k, p) == -1
    for r in range(p):                                        # one parity row alone
        assert vc(st(1 << r, 0), k, p) == k + r
    for j in range(k):                                        # every row + one candidate
        assert vc(st(allrows, 1 << j), k, p) == j
    assert vc(st(allrows, 0), k, p) == -2                     # every row, nobody explains it
    for a, b in itertools.combinations(range(k), 2):          # two candidates left
        assert vc(st(allrows, (1 << a) | (1 << b)), k, p) == -2
    if p == 3:                                                # a proper subset of the rows
        for rows in (0b011, 0b101, 0b110):
            assert vc(st(rows, 0), k, p) == -2
            assert vc(st(rows, 1), k, p) == -2
    # candidate bits at or above k are not cells of this stripe
    assert vc(st(allrows, 1 << k), k, p) == -2


def test_verify_cell_single_parity(ecglib):
    """p == 1: parity row 0 and any data cell are indistinguishable."""
    for k in (2, 4, 8, 16):
        assert ecglib.verify_cell(st(0, (1 << k) - 1), k, 1) == -1
        assert ecglib.verify_cell(st(1, (1 << k) - 1), k, 1) == -2
        assert ecglib.verify_cell(st(1, 1), k, 1) == -2
        assert ecglib.verify_cell(st(1, 0), k, 1) == -2


def test_verify_macros_match_encoding():
    """ECG_VERIFY_ROWS / ECG_VERIFY_CAND of include/ecg.h are the fields st() packs."""
    src = open(os.path.join(ROOT, "include", "ecg.h")).read()
    assert "#define ECG_VERIFY_ROWS(st)  ((st) & 0xffu)" in src
    assert "#define ECG_VERIFY_CAND(st)  (((st) >> 8) & 0xffffu)" in src


def test_verify_exported(ecglib):
    out = subprocess.run(["nm", "-D", "--defined-only", ecglib.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"ecg_verify", "ecg_verify_cell"} <= syms
    assert {"ecg_verify", "ecg_verify_cell"} <= set(ecglib.EXPORTED)
    assert callable(ecglib.Context.verify) and callable(ecglib.verify_cell)


def test_verify_null_context(ecglib):
    L = ecglib.lib()
    res = (C.c_uint64 * 4)()
    stw = (C.c_uint32 * 4)()
    rc = L.ecg_verify(None, 4, 2, 4096, 4, 16, 4 * 4096, 16, 4 * 4096, 4096, C.addressof(stw), C.addressof(res),
                      None)
    assert rc == -ecglib.DER_INVAL
    assert b"NULL context" in L.ecg_strerror()
