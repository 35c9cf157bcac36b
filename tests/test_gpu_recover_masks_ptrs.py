"""ecg_recover_masks_ptrs on the GPU: ecg_recover_masks with the cells of every stripe given by
address.  The rig is one device allocation between 0xA5 guards in which cell (s, c) lives at
base + perm[s*(k+p)+c] * (C + gap): perm a seeded permutation, gap 48 bytes of 0xA5, 24 cells of
0xA5 slack at the end, so a cell written anywhere but where it belongs shows up.  Every
comparison is exact and covers the whole allocation."""
import ctypes as C

import numpy as np
import pytest

from tests import test_gpu_recover_masks as rm

pytestmark = pytest.mark.gpu

U64MAX, GUARD, FILL, ERASED, SLACK, GAP = rm.U64MAX, rm.GUARD, rm.FILL, rm.ERASED, rm.SLACK, 48
BYTE_KERNEL = "ecg_recover_masks_ptr_byte_kernel"


def ptr_kernel(k, p):
    return f"ecg_recover_masks_ptr_kernel<{k if k in (2, 4, 8, 16) else 0}, {p}>"


class PtrRig:
    """cells: [S][k+p][C] to start from.  skew(s, c): byte offset of a cell inside its slot
    (below gap); permute = False with gap = 0 is the contiguous image [S][k+p][C]."""

    def __init__(self, ctx, k, p, C_, cells, skew=None, permute=True, gap=GAP):
        self.ctx, self.k, self.p, self.C, self.S = ctx, k, p, C_, cells.shape[0]
        self.n = n = k + p
        slot, nc = C_ + gap, self.S * n
        perm = np.random.default_rng(31 * k + p + nc).permutation(nc) if permute else np.arange(nc)
        self.off = np.array([GUARD + int(perm[i]) * slot + (skew(i // n, i % n) if skew else 0)
                             for i in range(nc)]).reshape(self.S, n)
        assert skew is None or gap >= 4
        self.img = np.full(GUARD + nc * slot + SLACK * slot + GUARD, FILL, dtype=np.uint8)
        self.scatter(self.img, cells)
        self.buf = ctx.alloc(self.img.size)
        assert self.buf.ptr % 16 == 0
        self.masks, self.result = ctx.alloc(4 * self.S), ctx.alloc(32)

    def cell(self, img, s, c):
        return img[self.off[s, c]:self.off[s, c] + self.C]

    def scatter(self, img, cells):
        for s in range(self.S):
            for c in range(self.n):
                self.cell(img, s, c)[:] = cells[s, c]

    def gather(self, img):
        return np.stack([np.stack([self.cell(img, s, c) for c in range(self.n)]) for s in range(self.S)])

    def table(self, order=None):
        """The addresses, row s those of stripe order[s]."""
        return [self.buf.ptr + int(o) for s in (range(self.S) if order is None else order) for o in self.off[s]]

    def erase(self, masks):
        for s, m in enumerate(masks):
            for c in rm.cells_of(int(m)):
                if c < self.n:
                    self.cell(self.img, s, c)[:] = ERASED

    def run(self, ecglib, masks, flags=0, table=None):
        """Upload image and masks, one call, one sync.  -> (image, result words, kernel)."""
        words = np.array(masks, dtype=np.uint32)
        self.buf.upload(self.img)
        self.masks.upload(words.view(np.uint8))
        self.result.fill(0xEE)
        self.ctx.recover_masks_ptrs(self.k, self.p, self.C, self.S, self.table() if table is None else table,
                                    self.masks.ptr, self.result.ptr, flags)
        name = ecglib.last_kernel()
        self.ctx.sync()
        assert np.array_equal(self.masks.download().view(np.uint32), words)         # read only
        return self.buf.download(), self.words(), name

    def words(self):
        return [int(v) for v in self.result.download().view(np.uint64)]

    def free(self):
        for b in (self.buf, self.masks, self.result):
            b.free()


def same(got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], bad.size)


def strided_twin(ctx, rig, masks):
    """What ecg_recover_masks leaves of the same cells gathered into one image [S][k+p][C],
    scattered back into a copy of rig.img; and its result words."""
    cells = np.ascontiguousarray(rig.gather(rig.img))
    twin, mk, res = ctx.alloc(cells.size), ctx.alloc(4 * rig.S), ctx.alloc(32)
    try:
        twin.upload(cells.reshape(-1))
        mk.upload(np.array(masks, dtype=np.uint32).view(np.uint8))
        ctx.recover_masks(rig.k, rig.p, rig.C, rig.S, twin.ptr, rig.n * rig.C, mk.ptr, res.ptr, 0)
        ctx.sync()
        want = rig.img.copy()
        rig.scatter(want, twin.download().reshape(rig.S, rig.n, rig.C))
        return want, [int(v) for v in res.download().view(np.uint64)]
    finally:
        for b in (twin, mk, res):
            b.free()


def check_every_set(ctx, ecglib, oracle, k, p, C_, kernel, **rig_args):
    """Stripe i carries set i, its erased cells overwritten; then mask 0, p+1 bits, bit k+p."""
    sets = rm.sets_by_index(ecglib, k, p)
    n = len(sets)
    masks = sets + [0, rm.bits(range(p + 1)), 1 | 1 << (k + p)]
    rig = PtrRig(ctx, k, p, C_, rm.codewords(oracle, k, p, C_, n + 3), **rig_args)
    try:
        want = rig.img.copy()
        rig.erase(masks)
        for s in (n + 1, n + 2):                # the unrecoverable stripes keep their 0x5A cells
            for c in range(k + p):
                rig.cell(want, s, c)[:] = rig.cell(rig.img, s, c)
        got, res, name = rig.run(ecglib, masks)
        assert name == kernel, name
        assert res == [n, n + 1, sum(bin(m).count("1") for m in sets), 2]
        same(got, want)
    finally:
        rig.free()


# ------------------------------------------------------------ 1. every erasure set
@pytest.mark.parametrize("k,p", rm.SHAPES)
def test_every_erasure_set_small_cell(ctx, ecglib, oracle, k, p):
    check_every_set(ctx, ecglib, oracle, k, p, 16, ptr_kernel(k, p))


@pytest.mark.parametrize("k,p", [kp for kp in rm.SHAPES if rm.NSETS[kp] <= 231])
def test_every_erasure_set_lane_masked_last_column(ctx, ecglib, oracle, k, p):
    check_every_set(ctx, ecglib, oracle, k, p, 8192 + 48, ptr_kernel(k, p))


# --------------------------- 2. the bytes of ecg_recover_masks, on non-codewords
@pytest.mark.parametrize("k,p", [(4, 2), (8, 3), (16, 2)])
def test_identical_to_recover_masks_on_non_codewords(ctx, ecglib, k, p):
    """Random, inconsistent stripes: the bytes written depend on which survivors are read and in
    which order the rows are written."""
    masks = rm.sets_by_index(ecglib, k, p)
    rig = PtrRig(ctx, k, p, 4096, rm.random_cells(k, p, 4096, len(masks)))
    try:
        want, words = strided_twin(ctx, rig, masks)
        assert not np.array_equal(want, rig.img)                        # the twin did write
        got, res, name = rig.run(ecglib, masks)
        assert name == ptr_kernel(k, p)
        assert res == words == rm.model(masks, k, p)[1]
        for s in range(rig.S):                                          # cell by cell, then the rest
            for c in range(k + p):
                assert np.array_equal(rig.cell(got, s, c), rig.cell(want, s, c)), (s, c)
        same(got, want)
    finally:
        rig.free()


# ------------------------------------------------------- 3. any mask value is safe
@pytest.mark.parametrize("k,p", [(4, 2), (16, 3)])
def test_any_mask_value_is_safe(ctx, ecglib, k, p):
    """The mask mix of the strided call's test over 200 stripes of random bytes: every grid,
    kernel and flag gives the image and the result words of ecg_recover_masks."""
    rng = np.random.default_rng(20 + k)
    n = k + p
    sets = rm.sets_by_index(ecglib, k, p)
    masks = [int(rng.integers(0, 1 << 32)) for _ in range(60)]
    masks += [int(rng.integers(0, 1 << n)) & int(rng.integers(0, 1 << n)) for _ in range(60)]
    masks += [sets[int(i)] for i in rng.integers(0, len(sets), 60)]
    masks += [0xFFFFFFFF, 0, 1 << 31, 1 << n, 1 << (n + 1), 1 << 19, 1 << 20, (1 << n) - 1, 1 | 1 << 31,
              rm.bits(range(p + 1)), rm.bits(range(k, n)), rm.bits(range(k - 1, n)), 1 << (n - 1), 1,
              0x80000001 >> 1]
    masks += [0] * (200 - len(masks))
    rig = PtrRig(ctx, k, p, 4096, rm.random_cells(k, p, 4096, 200))
    try:
        ok, words = rm.model(masks, k, p)
        assert len(ok) >= 60 and words[3] >= 60
        want, twin_words = strided_twin(ctx, rig, masks)
        assert twin_words == words
        for grid in ((0, 0), (1, 2)):
            for variant in (0, 2):
                for flags in (0, ecglib.RM_SPARSE):
                    ctx.set_launch(grid[0], grid[1], variant)
                    try:
                        got, res, name = rig.run(ecglib, masks, flags)
                    finally:
                        ctx.set_launch(0, 0, 0)
                    assert name == (BYTE_KERNEL if variant == 2 else ptr_kernel(k, p))
                    assert res == words, (grid, variant, flags)
                    same(got, want)
    finally:
        rig.free()


# ------------------------------------------------------------------ 4. byte kernel
@pytest.mark.parametrize("C_", [1, 4099, 4096])
@pytest.mark.parametrize("k,p", [(4, 2), (8, 3), (5, 2), (2, 1)])
def test_byte_kernel_mixed_alignments(ctx, ecglib, oracle, k, p, C_):
    check_every_set(ctx, ecglib, oracle, k, p, C_, BYTE_KERNEL, skew=lambda s, c: (s + c) % 4)


@pytest.mark.parametrize("k,p", [(4, 2), (8, 3)])
def test_one_misaligned_cell_sends_the_whole_launch_to_the_byte_kernel(ctx, ecglib, oracle, k, p):
    check_every_set(ctx, ecglib, oracle, k, p, 4096, ptr_kernel(k, p))          # all aligned: the lanes
    check_every_set(ctx, ecglib, oracle, k, p, 4096, BYTE_KERNEL,
                    skew=lambda s, c: 4 if (s, c) == (3, 1) else 0)


@pytest.mark.parametrize("k,p", [(4, 2), (16, 2), (5, 2)])
def test_byte_kernel_forced_on_aligned_cells(ctx, ecglib, oracle, k, p):
    ctx.set_launch(0, 0, 2)
    try:
        check_every_set(ctx, ecglib, oracle, k, p, 8192 + 48, BYTE_KERNEL)
    finally:
        ctx.set_launch(0, 0, 0)


# ------------------------------------------------------------------ 5. affine route
@pytest.mark.parametrize("k,p", [(4, 2), (5, 2), (16, 3)])
def test_affine_table_is_the_strided_call(ctx, ecglib, oracle, k, p):
    C_, S_ = 4096, k + p + 3
    masks = rm.seeded_masks(k, p, S_)
    rig = PtrRig(ctx, k, p, C_, rm.codewords(oracle, k, p, C_, S_), permute=False, gap=0)
    try:
        want = rig.img.copy()
        rig.erase(masks)
        words = [S_, U64MAX, sum(bin(m).count("1") for m in masks), 0]
        got, res, name = rig.run(ecglib, masks)
        assert name == rm.kernel_name(k, p)                             # the contiguous image: strided
        assert res == words
        same(got, want)
        order = list(range(S_))
        order[1], order[S_ - 2] = order[S_ - 2], order[1]
        got, res, name = rig.run(ecglib, [masks[s] for s in order], table=rig.table(order))
        assert name == ptr_kernel(k, p)                                 # two rows exchanged: no stride
        assert res == words
        same(got, want)
        # one stripe whose cells are C apart is affine whatever lies around it
        rig.buf.upload(rig.img)
        ctx.recover_masks_ptrs(k, p, C_, 1, rig.table([order[1]]), rig.masks.ptr + 4, rig.result.ptr)
        assert ecglib.last_kernel() == rm.kernel_name(k, p)
        ctx.sync()
        assert rig.words() == [1, U64MAX, bin(masks[order[1]]).count("1"), 0]
        for c in range(k + p):
            rig.cell(rig.img, order[1], c)[:] = rig.cell(want, order[1], c)
        same(rig.buf.download(), rig.img)
    finally:
        rig.free()


# ------------------------------------------------------------ 6. column loop strides
@pytest.mark.parametrize("k,p", rm.SHAPES)
def test_more_columns_than_column_blocks(ctx, ecglib, oracle, k, p):
    C_, S_ = 128 * 1024, k + p + 3
    masks = rm.seeded_masks(k, p, S_)            # asserts every cell index and every e <= p occurs
    rig = PtrRig(ctx, k, p, C_, rm.codewords(oracle, k, p, C_, S_))
    try:
        want = rig.img.copy()
        rig.erase(masks)
        ctx.set_launch(3, 0, 0)                 # 32 columns on 3 column blocks: the column loop strides
        try:
            got, res, name = rig.run(ecglib, masks, ecglib.RM_SPARSE)
        finally:
            ctx.set_launch(0, 0, 0)
        assert name == ptr_kernel(k, p)
        assert res == [S_, U64MAX, sum(bin(m).count("1") for m in masks), 0]
        same(got, want)
        for flags in (0, ecglib.RM_SPARSE):     # and the default grids
            got, res2, _ = rig.run(ecglib, masks, flags)
            assert res2 == res
            same(got, want)
    finally:
        rig.free()


# ----------------------------------------------------- 7. one allocation per stripe
def test_one_allocation_per_stripe(ctx, ecglib, oracle):
    """The rebuild / queue shape: every stripe a buffer of its own."""
    k, p, C_, S_ = 8, 2, 4096, 12
    n = k + p
    cw = rm.codewords(oracle, k, p, C_, S_)
    masks = rm.seeded_masks(k, p, S_)
    bufs = [ctx.alloc(n * C_) for _ in range(S_)]
    bufs = [bufs[int(i)] for i in np.random.default_rng(S_).permutation(S_)]       # in no address order
    mk, res = ctx.alloc(4 * S_), ctx.alloc(32)
    try:
        for s, b in enumerate(bufs):
            broken = cw[s].copy()
            broken[rm.cells_of(masks[s])] = ERASED
            b.upload(broken.reshape(-1))
        mk.upload(np.array(masks, dtype=np.uint32).view(np.uint8))
        ctx.recover_masks_ptrs(k, p, C_, S_, [b.ptr + c * C_ for b in bufs for c in range(n)], mk.ptr, res.ptr)
        ctx.sync()
        assert [int(v) for v in res.download().view(np.uint64)] == \
            [S_, U64MAX, sum(bin(m).count("1") for m in masks), 0]
        for s, b in enumerate(bufs):
            assert np.array_equal(b.download(), cw[s].reshape(-1)), s
    finally:
        for b in bufs + [mk, res]:
            b.free()


# ---------------------------------------------------------- 8. the table is staged
def test_the_table_is_copied_before_the_call_returns(ctx, ecglib, oracle):
    """B = A with its rows rotated by one; the caller's array holds A at the call and B before
    the sync.  The result is A's: a late reader would recover every stripe with its neighbour's
    set -- wrong bytes, never a wild address."""
    k, p, C_, S_ = 8, 2, 64 * 1024, 14
    masks = rm.seeded_masks(k, p, S_)
    assert all(masks[s] != masks[(s + 1) % S_] for s in range(S_))
    rig = PtrRig(ctx, k, p, C_, rm.codewords(oracle, k, p, C_, S_))
    try:
        want = rig.img.copy()
        rig.erase(masks)
        a, b = rig.table(), rig.table([(s + 1) % S_ for s in range(S_)])
        arr = (C.c_void_p * len(a))(*a)
        rig.buf.upload(rig.img)
        rig.masks.upload(np.array(masks, dtype=np.uint32).view(np.uint8))
        ctx.recover_masks_ptrs(k, p, C_, S_, arr, rig.masks.ptr, rig.result.ptr)
        arr[:] = b
        ctx.sync()
        assert rig.words() == [S_, U64MAX, sum(bin(m).count("1") for m in masks), 0]
        same(rig.buf.download(), want)
    finally:
        rig.free()


def test_two_calls_back_to_back_on_one_stream(ctx, ecglib, oracle):
    shapes = [(8, 2, 4096, 11), (4, 2, 8192, 9)]
    rigs = [PtrRig(ctx, k, p, C_, rm.codewords(oracle, k, p, C_, S_)) for k, p, C_, S_ in shapes]
    try:
        wants, every = [], []
        for rig in rigs:
            masks = rm.seeded_masks(rig.k, rig.p, rig.S)
            wants.append(rig.img.copy())
            rig.erase(masks)
            rig.buf.upload(rig.img)
            rig.masks.upload(np.array(masks, dtype=np.uint32).view(np.uint8))
            every.append(masks)
        ctx.sync()
        for rig in rigs:                        # no sync in between
            ctx.recover_masks_ptrs(rig.k, rig.p, rig.C, rig.S, rig.table(), rig.masks.ptr, rig.result.ptr)
        ctx.sync()
        for rig, want, masks in zip(rigs, wants, every):
            assert rig.words() == [rig.S, U64MAX, sum(bin(m).count("1") for m in masks), 0]
            same(rig.buf.download(), want)
    finally:
        for rig in rigs:
            rig.free()


# ------------------------------------------------------------------- 9. arguments
def test_argument_errors(ctx, ecglib):
    L = ecglib.lib()
    k, p, C_, S_ = 4, 2, 4096, 9
    n = k + p
    rig = PtrRig(ctx, k, p, C_, rm.random_cells(k, p, C_, S_))
    try:
        rig.buf.upload(rig.img)
        rig.masks.upload(np.full(S_, 1, dtype=np.uint32).view(np.uint8))
        tab = rig.table()

        def call(C__=C_, S__=S_, cells=tab, masks=rig.masks.ptr, result=rig.result.ptr):
            arr = None if cells is None else (C.c_void_p * len(cells))(*cells)
            return L.ecg_recover_masks_ptrs(ctx.h, k, p, C__, S__, arr, masks, result, 0, None)

        assert call(cells=None) == -ecglib.DER_INVAL
        assert b"NULL cells" in L.ecg_strerror()
        for i in (0, 7, S_ * n - 1):
            assert call(cells=tab[:i] + [None] + tab[i + 1:]) == -ecglib.DER_INVAL
            assert b"NULL cell %d" % i in L.ecg_strerror(), L.ecg_strerror()
        cell = tab[2 * n + 3]
        for inside in (cell, cell + C_ - 4, cell - 4 * S_ + 4):
            assert call(masks=inside) == -ecglib.DER_INVAL              # masks inside a cell
            assert b"overlaps" in L.ecg_strerror()
        for inside in (cell, cell + C_ - 8, cell - 24):
            assert call(result=inside) == -ecglib.DER_INVAL             # result inside a cell
            assert b"overlaps" in L.ecg_strerror()
        # an empty batch and empty cells preset the result and touch nothing else
        for kw in ({"S__": 0, "cells": None}, {"C__": 0}):
            rig.result.fill(0xEE)
            assert call(**kw) == 0
            ctx.sync()
            assert rig.words() == [0, U64MAX, 0, 0]
        assert np.array_equal(rig.buf.download(), rig.img)              # none of the calls above wrote a cell
    finally:
        rig.free()


def test_counts_one_launch_and_no_recover_stripes(ctx, ecglib, oracle):
    rig = PtrRig(ctx, 4, 2, 4096, rm.codewords(oracle, 4, 2, 4096, 6))
    try:
        rig.run(ecglib, [1] * 6)                # builds and uploads the set table
        before = ctx.stats()
        _, _, name = rig.run(ecglib, [1] * 6)
        after = ctx.stats()
        assert name == ptr_kernel(4, 2)
        assert after["launches"] == before["launches"] + 1
        assert after["recover_stripes"] == before["recover_stripes"]    # the count lives on the device
        assert after["recover_bytes"] == before["recover_bytes"]
    finally:
        rig.free()
