"""Seeded random geometry through ecg_update_masks_ptrs, byte for byte against the CPU oracle: 48
cases on the rig of tests.test_gpu_update_masks_ptrs (one allocation, 0xA5 wherever no cell lies,
compared whole after the call), numbered and sized as tests.test_gpu_fuzz_masks numbers its own.
Drawn per case: (k, p) from all k <= 16, p <= 8; cell_bytes from the multiples of 16 up to three
columns or from odd lengths; 1..70 stripes; where the cells lie -- every cell in a shuffled slot of
its own with a skew that is a multiple of 16 or any byte, or three strided groups at drawn pads --;
mask words valid, zero and invalid; ECG_RM_SPARSE; ecg_set_launch's grid and variant.  The kernel
that ran must be the one `predict` names by the header's rule (include/ecg.h): the strided kernels
for a table that is three strided groups, else the cell-table ones; 16-byte lanes iff every
address (strided: every base and stride) and cell_bytes are multiples of 16 and the variant is not
2."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import test_gpu_fuzz_masks as fz
from tests import test_gpu_update_masks as um
from tests import test_gpu_update_masks_ptrs as ump

N, GUARD, SLACK = fz.N, ump.GUARD, ump.SLACK
MODES = ["slots16", "slots_any", "groups16", "slots16", "groups_any", "slots16"]
ODD = [1, 3, 17, 255, 4095, 4097, 8191, 8200 + 1]


def three_groups(off, k, p, C_):
    """host/ecg_update_masks.c um_three_groups over offsets [S][2k+p].  -> (is, us, pc, ps)"""
    S_ = len(off)
    o0, n0, p0 = int(off[0][0]), int(off[0][k]), int(off[0][2 * k])
    us = int(off[1][0]) - o0 if S_ > 1 else k * C_
    pc = int(off[0][2 * k + 1]) - p0 if p > 1 else C_
    ps = int(off[1][2 * k]) - p0 if S_ > 1 else C_
    ok = all(int(off[s][j]) == o0 + s * us + j * C_ and int(off[s][k + j]) == n0 + s * us + j * C_
             for s in range(S_) for j in range(k))
    ok = ok and all(int(off[s][2 * k + r]) == p0 + s * ps + r * pc for s in range(S_) for r in range(p))
    return ok, us, pc, ps


def draw(seed):
    rng = np.random.default_rng(210000 + seed)
    d = SimpleNamespace(seed=seed, mode=MODES[seed % len(MODES)])
    d.p = seed % 8 + 1
    d.k = int(rng.integers(1, 17))
    any_byte = d.mode.endswith("any")
    d.C = ODD[int(rng.integers(len(ODD)))] if seed % 4 == 3 else 16 * int(rng.integers(1, 3 * 256 + 1))
    d.S = int(rng.integers(1, 71))
    k, p, C_, S_ = d.k, d.p, d.C, d.S
    n = 2 * k + p
    unit = 1 if any_byte else 16

    def skew(hi):
        return int(rng.integers(hi // unit)) * unit

    if d.mode.startswith("slots"):
        slot = (C_ + ump.GAP + 15) // 16 * 16
        perm = rng.permutation(S_ * n)
        d.off = np.array([GUARD + int(perm[i]) * slot + skew(ump.GAP) for i in range(S_ * n)]).reshape(S_, n)
        d.size = GUARD + S_ * n * slot + SLACK * slot + GUARD
    else:
        us, pc = k * C_ + skew(64), C_ + skew(64)
        ps = p * pc + skew(64)
        o0 = GUARD + skew(64)
        n0 = o0 + S_ * us + 64 + skew(64)
        p0 = n0 + S_ * us + 64 + skew(64)
        d.off = np.array([[o0 + s * us + j * C_ for j in range(k)] + [n0 + s * us + j * C_ for j in range(k)] +
                          [p0 + s * ps + r * pc for r in range(p)] for s in range(S_)])
        d.size = p0 + S_ * ps + SLACK * C_ + GUARD
    kinds = rng.integers(0, 10, S_)
    d.masks = []
    for s in range(S_):
        if kinds[s] < 6:
            d.masks.append(int(rng.integers(1, 1 << k)))
        elif kinds[s] < 8:
            d.masks.append(0)
        else:
            d.masks.append(int(rng.integers(0, 1 << 32)) | 1 << int(rng.integers(k, 32)))
    d.masks[int(rng.integers(S_))] = int(rng.integers(1, 1 << k))          # one stripe at least has work
    d.flags = int(rng.integers(2))
    d.grid = (int(rng.integers(1, 4)), int(rng.integers(1, 5))) if rng.integers(3) == 0 else (0, 0)
    d.variant = 2 if seed % 11 == 5 else 0
    d.strided, us, pc, ps = three_groups(d.off, k, p, C_)
    if d.strided:
        bits = int(d.off[0][0]) | int(d.off[0][k]) | int(d.off[0][2 * k]) | us | pc | ps | C_
    else:
        bits = int(np.bitwise_or.reduce(d.off.reshape(-1))) | C_
    d.lanes = bits % 16 == 0 and d.variant != 2
    d.ragged = d.lanes and C_ % 4096 != 0
    return d


def cells_of(oracle, d):
    """[S][2k+p][C] of one case: old cells, new cells (every one differs), the oracle's parity of
    old.  Not kept: 48 cases of up to 30 MB."""
    rng = np.random.default_rng(310000 + d.seed)
    old = rng.integers(0, 256, (d.S, d.k, d.C), dtype=np.uint8)
    new = old ^ rng.integers(1, 256, (d.S, d.k, d.C), dtype=np.uint8)
    par = oracle.encode_batch(d.k, d.p, d.C, d.S, old.reshape(-1)).reshape(d.p, d.S, d.C)
    return np.concatenate([old, new, par.transpose(1, 0, 2)], axis=1)


def predict(d):
    r = d.p if d.p <= 3 else 0
    if d.strided:
        return f"ecg_update_masks_kernel<{r}>" if d.lanes else um.BYTE_KERNEL
    return f"ecg_update_masks_ptr_kernel<{r}>" if d.lanes else ump.BYTE_KERNEL


def test_the_draws_reach_every_class():
    ds = [draw(seed) for seed in range(N)]
    names = {predict(d) for d in ds}
    assert {f"ecg_update_masks_ptr_kernel<{r}>" for r in (1, 2, 3, 0)} <= names      # every R and R = 0
    assert ump.BYTE_KERNEL in names
    assert any(d.strided for d in ds) and any(d.strided and d.lanes for d in ds)       # the strided route
    assert any(not d.strided and d.ragged for d in ds)                                # a ragged last column
    assert any(not d.strided and d.lanes and d.C > 8192 for d in ds)                   # three columns
    for flags in (0, 1):                                                               # both grids
        assert any(not d.strided and d.flags == flags and d.grid == (0, 0) for d in ds)
    assert any(not d.strided and d.grid != (0, 0) for d in ds)
    assert any(not d.strided and d.variant == 2 for d in ds)
    kinds = {("zero" if m == 0 else "valid" if um.valid(m, d.k) else "invalid") for d in ds for m in d.masks}
    assert kinds == {"zero", "valid", "invalid"}
    assert all(d.C <= 64 * 1024 for d in ds)


@pytest.mark.gpu
@pytest.mark.parametrize("lo", range(0, N, 8))
def test_update_masks_ptrs(ctx, ecglib, oracle, lo):
    for seed in range(lo, lo + 8):
        d = draw(seed)
        what = f"seed {seed}: {d.mode} k={d.k} p={d.p} C={d.C} S={d.S} flags={d.flags} grid={d.grid} " \
               f"variant={d.variant}"
        rig = ump.PtrRig(ctx, d.k, d.p, d.C, cells_of(oracle, d), off=d.off, size=d.size)
        ctx.set_launch(d.grid[0], d.grid[1], d.variant)
        try:
            want = rig.expect(oracle, d.masks)
            got, res, name = rig.run(ecglib, d.masks, d.flags)
            assert name == predict(d), f"{what}: ran {name}, predicted {predict(d)}"
            assert res == um.model(d.masks, d.k), what
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (what, bad[:8], bad.size)
        finally:
            ctx.set_launch(0, 0, 0)
            rig.free()
