"""ecg_repair's host side, no GPU: the row ecg_repair applies for every cell
(ecg_repair_row) against the Cauchy1 matrix, the decode rows of
ecg_recov_matrix and an oracle-encoded stripe; argument errors, the exports
and the NULL-context path."""
import ctypes as C
import subprocess

import numpy as np
import pytest

CLASSES = [(k, p) for k in (2, 4, 8, 16) for p in (2, 3)] + [(5, 2)]
CELL = 333                                       # bytes per cell of the applied rows: odd, a few SIMD widths


def stripe(oracle, k, p):
    """One oracle-encoded stripe [k+p][CELL]."""
    data = np.random.default_rng(k * 131 + p).integers(0, 256, (k, CELL), dtype=np.uint8)
    return np.concatenate([data, oracle.encode_data(oracle.cauchy1(k, p)[k:], data)])


@pytest.mark.parametrize("k,p", CLASSES)
def test_parity_rows_are_the_cauchy_rows(ecglib, oracle, k, p):
    g = ecglib.cauchy1(k, p)
    assert np.array_equal(g, oracle.cauchy1(k, p))
    for cell in range(k, k + p):
        coef, idx = ecglib.repair_row(k, p, cell)
        assert np.array_equal(coef, g[cell])
        assert list(idx) == list(range(k))


@pytest.mark.parametrize("k,p", CLASSES)
def test_data_rows_are_the_decode_rows(ecglib, k, p):
    """Slot i != cell reads data cell i, slot `cell` parity row 0 (logical k): the
    coefficients and survivors of ecg_recov_matrix(err_list=[cell]), which lists
    the same survivors in ascending cell order."""
    g = ecglib.cauchy1(k, p)
    for cell in range(k):
        coef, idx = ecglib.repair_row(k, p, cell)
        assert list(idx) == [k if i == cell else i for i in range(k)]
        rows, dec, reused = ecglib.recov_matrix(k, p, [cell])
        assert not reused
        assert list(dec) == sorted(int(i) for i in idx)                   # the same survivors ...
        assert dict(zip((int(i) for i in idx), (int(c) for c in coef))) == \
            dict(zip((int(i) for i in dec), (int(c) for c in rows[0])))   # ... with the same coefficients
        inv = ecglib.gf_inv(int(g[k][cell]))                              # and the closed form of the header
        assert int(coef[cell]) == inv
        assert all(int(coef[i]) == ecglib.gf_mul(int(g[k][i]), inv) for i in range(k) if i != cell)


@pytest.mark.parametrize("k,p", CLASSES)
def test_rows_reproduce_every_cell(ecglib, oracle, k, p):
    st = stripe(oracle, k, p)
    for cell in range(k + p):
        coef, idx = ecglib.repair_row(k, p, cell)
        assert cell not in idx                   # a cell is never one of its own sources
        out = np.full(CELL, 0xEE, dtype=np.uint8)
        ecglib.cpu_matmul(coef.reshape(1, k), [np.ascontiguousarray(st[int(i)]) for i in idx], [out])
        assert np.array_equal(out, st[cell]), cell


def test_repair_row_argument_errors(ecglib):
    L = ecglib.lib()
    coef = (C.c_ubyte * 16)()
    idx = (C.c_uint32 * 16)()
    for k, p, cell in ((4, 2, 6), (4, 2, -1), (17, 2, 0), (4, 0, 0), (0, 2, 0), (4, 9, 0)):
        assert L.ecg_repair_row(k, p, cell, coef, idx) == -ecglib.DER_INVAL, (k, p, cell)
    assert L.ecg_repair_row(4, 2, 5, None, idx) == -ecglib.DER_INVAL
    assert L.ecg_repair_row(4, 2, 5, coef, idx) == 0
    with pytest.raises(ecglib.EcgError) as ei:
        ecglib.repair_row(4, 2, 6)
    assert ei.value.rc == -ecglib.DER_INVAL and "cell 6" in str(ei.value)


def test_repair_null_context(ecglib):
    L = ecglib.lib()
    res = (C.c_uint64 * 4)()
    stw = (C.c_uint32 * 4)()
    rc = L.ecg_repair(None, 4, 2, 4096, 4, 16, 4 * 4096, 16, 4 * 4096, 4096, C.addressof(stw), C.addressof(res),
                      None)
    assert rc == -ecglib.DER_INVAL
    assert b"NULL context" in L.ecg_strerror()


def test_repair_exported(ecglib):
    out = subprocess.run(["nm", "-D", "--defined-only", ecglib.LIB_PATH], check=True, capture_output=True,
                         text=True).stdout
    syms = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {"ecg_repair", "ecg_repair_row"} <= syms
    assert {"ecg_repair", "ecg_repair_row"} <= set(ecglib.EXPORTED)
    assert callable(ecglib.Context.repair) and callable(ecglib.repair_row)
