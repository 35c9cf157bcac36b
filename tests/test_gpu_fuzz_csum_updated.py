"""Seeded random draws through ecg_csum_updated and ecg_csum_updated_ptrs, each checked whole
against the numpy model of tests/test_gpu_csum_updated.py (whose rig this is: the parity arena is
0xA5 where no cell lies, the checksum array 0xEE between 0xA5 guards, both compared whole after
the call, the masks and the arena as read only).

Drawn per seed: (k, p); the cell size, chunk size and record size; the number of stripes; the
two parity strides -- either order of nesting, padding, each of them negative or not -- or a
scattered table; the skew of the parity base and of the checksum array; the two checksum strides
in either accepted order with padding, and the array's offset; mask words over all 32 bits; the
strided call, an affine table or a scattered one; the launch cap.  A draw is pure and host-only;
the failing draw is printed with its seed."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests.test_gpu_csum_updated import CL, PRE, Rig, expect_sums, read, same, scattered, words

pytestmark = pytest.mark.gpu

NSEEDS = 64
SEED0 = 310000
SHAPES = [(2, 1), (4, 2), (8, 2), (8, 3), (16, 2), (5, 4), (8, 8), (16, 8), (1, 1), (3, 5)]
CELLS = [32, 64, 96, 100, 1040, 2048, 4096, 4099, 5136]
CHUNKS = [24, 32, 64, 1000, 1024, 2048, 4096, 1 << 20]
RECS = [1, 1, 2, 4, 8, 16]
FORMS = ["strided", "strided", "affine", "scattered", "scattered"]
BLOCKS = [0, 0, 1, 3]


def draw(seed):
    rng = np.random.default_rng(SEED0 + seed)
    d = SimpleNamespace(seed=seed)
    d.k, d.p = SHAPES[seed % len(SHAPES)]
    d.htype = (1, 2, 3, 7)[seed // 2 % 4]
    d.form = FORMS[seed % len(FORMS)]
    while True:                                     # the documented precondition C % rec_size == 0
        d.C, d.rec = int(rng.choice(CELLS)), int(rng.choice(RECS))
        if d.C % d.rec == 0:
            break
    d.chunksize = int(rng.choice(CHUNKS))
    d.S = int(rng.integers(1, 13))
    d.skew = int(rng.choice([0, 0, 0, 1, 4, 8, 16]))
    d.cskew = int(rng.integers(0, 8))
    d.blocks = BLOCKS[seed // 3 % len(BLOCKS)]
    # parity: rows nested in stripes or stripes in rows, padded, either stride negative
    pad = [int(rng.choice([0, 0, 16, 48, 5, 512])) for _ in range(2)]
    if rng.random() < 0.5:
        d.pc = d.C + pad[0]
        d.ps = (d.p - 1) * d.pc + d.C + pad[1]
    else:
        d.ps = d.C + pad[0]
        d.pc = (d.S - 1) * d.ps + d.C + pad[1]
    d.pc *= int(rng.choice([1, 1, -1]))
    d.ps *= int(rng.choice([1, 1, -1]))
    d.gap = int(rng.choice([0, 13, 16, 48]))        # of a scattered table
    # checksums: either accepted order, padded, somewhere inside the array
    d.corder = "rows_in_stripe" if rng.random() < 0.5 else "stripes_in_row"
    d.cpad = [int(rng.integers(0, 4)) for _ in range(2)]
    d.coff = int(rng.integers(0, 5))
    kinds = rng.random(d.S)
    full = rng.integers(0, 1 << 32, d.S, dtype=np.uint64)
    low = rng.integers(1, 1 << d.k, d.S, dtype=np.uint64) if d.k > 0 else full
    edge = rng.choice(np.array([0, 1, (1 << d.k) - 1, 1 << d.k, 0x80000000, 0xFFFFFFFF, 1 << (d.k - 1)],
                               dtype=np.uint64), d.S)
    d.masks = [int(np.where(x < 0.45, lo, np.where(x < 0.6, 0, np.where(x < 0.8, e, f))))
               for x, lo, e, f in zip(kinds, low, edge, full)]
    d.data_seed = int(rng.integers(1 << 31))
    return d


def describe(d):
    return f"seed {d.seed}: " + " ".join(f"{k}={v}" for k, v in vars(d).items() if k != "seed")


def test_draws_cover_the_ground():
    ds = [draw(s) for s in range(NSEEDS)]
    assert {d.form for d in ds} == set(FORMS) and {d.htype for d in ds} == {1, 2, 3, 7}
    assert any(d.pc < 0 for d in ds) and any(d.ps < 0 for d in ds) and any(d.blocks for d in ds)
    assert {d.corder for d in ds} == {"rows_in_stripe", "stripes_in_row"}
    assert any(d.p > 3 for d in ds) and any(d.S == 1 for d in ds) and any(d.skew for d in ds)
    assert any(read(m, d.k) == 0 for d in ds for m in d.masks) and any(read(m, d.k) < 0 for d in ds for m in d.masks)


@pytest.mark.parametrize("seed", range(NSEEDS))
def test_draw(ctx, ecglib, oracle, seed):
    d = draw(seed)
    L = ecglib.lib()
    k, p, C_, S_ = d.k, d.p, d.C, d.S
    cells = np.random.default_rng(d.data_seed).integers(0, 256, (S_, p, C_), dtype=np.uint8)
    v = oracle.csum_extents(d.htype, d.chunksize, d.rec, 0, C_ // d.rec, cells.reshape(-1), C_, S_ * p)
    cl, nch = CL[d.htype], v.shape[1]
    ref = np.ascontiguousarray(v).view(np.uint8).reshape(S_, p, nch, cl)
    if d.corder == "rows_in_stripe":
        ccs = nch + d.cpad[0]
        css = (p - 1) * ccs + nch + d.cpad[1]
    else:
        css = nch + d.cpad[0]
        ccs = (S_ - 1) * css + nch + d.cpad[1]
    nslots = d.coff + (S_ - 1) * css + (p - 1) * ccs + nch
    if d.form == "scattered":
        off = scattered(S_, p, C_, gap=d.gap, seed=d.seed)[0]
    else:
        off = np.array([[s * d.ps + r * d.pc for r in range(p)] for s in range(S_)])
    rig = Rig(ctx, k, cells, off, nslots, cl, d.skew, d.cskew)
    rcs = L.ecg_csum_record_chunksize(d.chunksize, d.rec)
    try:
        assert L.ecg_set_csum_launch(ctx.h, d.blocks) == 0
        got, res, name = rig.run(ecglib, d.masks, d.htype, d.chunksize, d.rec, (d.pc, d.ps), css, ccs, d.coff,
                                 table=None if d.form == "strided" else rig.table())
        # the kernel a restated rule names: a table whose parity entries are p0 + s*ps + r*pc (one
        # or two cells always are) is the strided call
        flat = [rig.addr(s, r) for s in range(S_) for r in range(p)]
        if d.form == "strided":
            pc, ps, strided = d.pc, d.ps, True
        else:
            pc = flat[1] - flat[0] if p > 1 else C_
            ps = flat[p] - flat[0] if S_ > 1 else C_
            strided = all(flat[s * p + r] == flat[0] + s * ps + r * pc for s in range(S_) for r in range(p))
            assert strided or d.form == "scattered", describe(d)
        if strided:
            bits, kernel = flat[0] | (pc & 15) | (ps & 15) | C_ | rcs, "updated_kernel"
        else:
            bits, kernel = C_ | rcs, "updated_ptr_kernel"
            for a in flat:
                bits |= a
        assert kernel in name and ("bytes" in name) == (bits % 16 != 0), (name, describe(d))
        assert res == words(d.masks, k, p), (res, describe(d))
        want = np.full((nslots, cl), PRE, dtype=np.uint8)
        want[d.coff:] = expect_sums(ref, d.masks, k, css, ccs, nslots - d.coff)
        same(got, rig.sums_image(want))
    except AssertionError:
        print(describe(d))
        raise
    finally:
        L.ecg_set_csum_launch(ctx.h, 0)
        rig.free()
