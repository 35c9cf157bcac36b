"""Seeded fuzz of ecg_matmul_ptrs_lens against the CPU oracle: drawn shapes, up to 64 stripes of
log-uniform lengths from 1 byte to 200 KiB with about one in ten zero, every cell at a random
address inside its own slot, at most 32 MiB of cells per case.  Bit-exact, and every byte outside
the output cells untouched."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (4, 2), (8, 2), (8, 3), (16, 2), (16, 3), (3, 2), (5, 4), (10, 3), (16, 8), (1, 1)]
MAX_LEN, CAP, PAD = 200 << 10, 32 << 20, 96


def draw(seed):
    rng = np.random.default_rng([20261021, seed])
    k, rows = SHAPES[int(rng.integers(0, len(SHAPES)))]
    S = int(rng.integers(1, 65))
    unit = (1, 1, 4, 16)[int(rng.integers(0, 4))]          # lengths: any, dwords, 16-byte pieces
    align = (1, 1, 4, 16)[int(rng.integers(0, 4))]         # addresses likewise
    lens = []
    for _ in range(S):
        L = int(math.exp(rng.uniform(0, math.log(MAX_LEN))))
        L = max(unit, L // unit * unit)
        lens.append(0 if rng.random() < 0.1 else min(L, MAX_LEN))
    while sum(lens) * (k + rows) > CAP:                    # the cap: drop stripes from the end
        lens.pop()
    variant = (0, 0, 0, 0, 1, 2)[int(rng.integers(0, 6))]
    return rng, k, rows, lens, align, variant


@pytest.mark.parametrize("seed", range(36))
def test_fuzz_matmul_ptrs_lens(oracle, ecglib, ctx, seed):
    rng, k, rows, lens, align, variant = draw(seed)
    n = k + rows
    coef = rng.integers(0, 256, (rows, k), dtype=np.uint8)
    ids = [(s, j) for s, L in enumerate(lens) if L for j in range(n)]
    off, at = {}, 0
    for i in rng.permutation(len(ids)):
        s, j = ids[int(i)]
        off[(s, j)] = at + int(rng.integers(0, 64 // align)) * align        # anywhere in the slot's slack
        at += (lens[s] + 15) // 16 * 16 + PAD
    host = rng.integers(1, 256, max(at, 16), dtype=np.uint8)
    exp = host.copy()
    for s, L in enumerate(lens):
        if L == 0:
            continue
        cells = np.stack([host[off[(s, j)]:][:L] for j in range(k)])
        want = oracle.encode_data(coef, cells)
        for r in range(rows):
            exp[off[(s, k + r)]:][:L] = want[r]
    buf = ctx.alloc(host.size)
    try:
        buf.upload(host)
        table = [buf.ptr + off[(s, j)] if L else None for s, L in enumerate(lens) for j in range(n)]
        ctx.set_launch(0, 0, variant)
        try:
            ctx.matmul_ptrs_lens(k, rows, coef, table, lens)
            ctx.sync()
        finally:
            ctx.set_launch(0, 0, 0)
        live = [L for L in lens if L]
        if live and not (len(live) == len(lens) and len(set(live)) == 1):
            assert ecglib.last_kernel().startswith("ecg_mm_ptr_lens_"), ecglib.last_kernel()
            if variant == 2:
                assert ecglib.last_kernel() == "ecg_mm_ptr_lens_byte_kernel"
        dev = buf.download()
        bad = np.flatnonzero(dev != exp)
        assert bad.size == 0, (k, rows, lens, align, variant, int(bad[0]), bad.size)
    finally:
        buf.free()
