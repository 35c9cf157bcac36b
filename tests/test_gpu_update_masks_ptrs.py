"""ecg_update_masks_ptrs on the GPU: ecg_update_masks with the cells of every stripe given by
address, 2k + p of them per stripe (k old, k new, p parity).  The rig is one device allocation
between 0xA5 guards in which cell (s, c) lives at a seeded permuted slot of C + 48 bytes, 24 cells
of 0xA5 slack at the end, so a cell written anywhere but where it belongs shows up.  Every
comparison is exact and covers the whole allocation; the mask words are verified unchanged.

The expectation is the CPU oracle alone, by linearity (tests.test_gpu_update_masks): expected
parity = parity0 ^ oracle.encode_batch(delta), delta = old ^ new in the cells a valid mask names,
computed from the bytes the table's row addresses hold -- so it also covers tables that are not
one-to-one.  The strided twin (ecg_update_masks over the gathered cells) is the one second
witness."""
import ctypes as C

import numpy as np
import pytest

from tests import test_gpu_update_masks as um

pytestmark = pytest.mark.gpu

U64MAX, GUARD, FILL, SLACK, GAP = um.U64MAX, um.GUARD, um.FILL, um.SLACK, 48
BYTE_KERNEL = "ecg_update_masks_ptr_byte_kernel"
SHAPES = [(1, 1), (2, 1), (4, 2), (8, 2), (8, 3), (16, 2), (16, 3), (5, 4), (3, 8), (16, 8)]


def ptr_kernel(p):
    return f"ecg_update_masks_ptr_kernel<{p if p <= 3 else 0}>"


def contents(oracle, k, p, C_, S_):
    """[S][2k+p][C]: old cells, new cells, parity of old (um.images: computed once per shape)."""
    old, new, par = um.images(oracle, k, p, C_, S_)
    return np.concatenate([old, new, par.transpose(1, 0, 2)], axis=1)


def same(got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], bad.size)


class PtrRig:
    """cells: [S][2k+p][C] to start from.  skew(s, c): byte offset of a cell inside its slot (below
    the gap).  off: explicit byte offsets [S][2k+p] into an allocation of `size` bytes instead of
    the permuted slots.  masks_at: byte offset of the mask words inside the allocation (else a
    buffer of their own)."""

    def __init__(self, ctx, k, p, C_, cells, skew=None, off=None, size=None, masks_at=None):
        self.ctx, self.k, self.p, self.C, self.S = ctx, k, p, C_, cells.shape[0]
        self.n = n = 2 * k + p
        slot, nc = C_ + GAP, self.S * n
        if off is None:
            perm = np.random.default_rng(31 * k + p + nc).permutation(nc)
            off = np.array([GUARD + int(perm[i]) * slot + (skew(i // n, i % n) if skew else 0)
                            for i in range(nc)]).reshape(self.S, n)
            size = GUARD + nc * slot + SLACK * slot + GUARD
        self.off = np.asarray(off).reshape(self.S, n)
        self.img = np.full(size, FILL, dtype=np.uint8)
        for s in range(self.S):
            for c in range(n):
                self.cell(self.img, s, c)[:] = cells[s, c]
        self.buf = ctx.alloc(size)
        assert self.buf.ptr % 16 == 0
        self.masks_at = masks_at
        self.own_masks = ctx.alloc(4 * max(1, self.S)) if masks_at is None else None
        self.masks_ptr = self.own_masks.ptr if masks_at is None else self.buf.ptr + masks_at
        self.result = ctx.alloc(32)

    def cell(self, img, s, c):
        return img[self.off[s, c]:self.off[s, c] + self.C]

    def rows(self, order=None):
        """The table as offsets, row s those of stripe order[s]."""
        return np.array([self.off[s] for s in (range(self.S) if order is None else order)])

    def table(self, rows=None):
        return [self.buf.ptr + int(o) for o in (self.rows() if rows is None else rows).reshape(-1)]

    def expect(self, oracle, masks, rows=None):
        """The image after the call over the table `rows` (offsets), from the bytes it names."""
        rows = self.rows() if rows is None else rows
        k, p, C_, S_ = self.k, self.p, self.C, len(rows)
        at = lambda o: self.img[int(o):int(o) + C_]     # noqa: E731
        delta = np.zeros((S_, k, C_), np.uint8)
        for s, m in enumerate(masks):
            if um.valid(int(m), k):
                for j in um.cells_of(int(m)):
                    delta[s, j] = at(rows[s][j]) ^ at(rows[s][k + j])
        enc = oracle.encode_batch(k, p, C_, S_, delta.reshape(-1)).reshape(p, S_, C_)
        want = self.img.copy()
        for s in range(S_):
            for r in range(p):
                o = int(rows[s][2 * k + r])
                want[o:o + C_] ^= enc[r, s]
        return want

    def upload(self, masks):
        self.words = np.array(masks, dtype=np.uint32)
        if self.masks_at is not None:
            self.img[self.masks_at:self.masks_at + 4 * len(masks)] = self.words.view(np.uint8)
        self.buf.upload(self.img)
        if self.masks_at is None and len(masks):
            self.own_masks.upload(self.words.view(np.uint8))
        self.result.fill(0xEE)

    def finish(self):
        """One sync.  -> (image, result words); the masks are checked to be as they were."""
        self.ctx.sync()
        if self.masks_at is None:
            assert np.array_equal(self.own_masks.download()[:4 * len(self.words)].view(np.uint32), self.words)
        return self.buf.download(), [int(v) for v in self.result.download().view(np.uint64)]

    def run(self, ecglib, masks, flags=0, rows=None):
        """Upload image and masks, one call, one sync.  -> (image, result words, kernel)."""
        self.upload(masks)
        tab = self.table(rows)
        self.ctx.update_masks_ptrs(self.k, self.p, self.C, len(masks), tab, self.masks_ptr, self.result.ptr, flags)
        name = ecglib.last_kernel()
        return self.finish() + (name,)

    def free(self):
        for b in (self.buf, self.own_masks, self.result):
            if b is not None:
                b.free()


def check(ctx, ecglib, oracle, k, p, C_, masks, kernel, flags=0, **rig_args):
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, len(masks)), **rig_args)
    try:
        want = rig.expect(oracle, masks)
        assert not np.array_equal(want, rig.img)                # the masks name work
        got, res, name = rig.run(ecglib, masks, flags)
        assert name == kernel, name
        assert res == um.model(masks, k), res
        same(got, want)
        return got
    finally:
        rig.free()


# ------------------------------------------------------------- 1. shapes, kernels, every mask
@pytest.mark.parametrize("k,p", SHAPES)
def test_every_shape_lane_masked_only_column(ctx, ecglib, oracle, k, p):
    check(ctx, ecglib, oracle, k, p, 48, um.some_masks(k), ptr_kernel(p))


@pytest.mark.parametrize("k", [4, 8])
def test_every_mask(ctx, ecglib, oracle, k):
    check(ctx, ecglib, oracle, k, 2, 16, um.every_mask(k), ptr_kernel(2))


def test_k16_masks_whole_column(ctx, ecglib, oracle):
    check(ctx, ecglib, oracle, 16, 3, 4096, um.k16_masks(), ptr_kernel(3))


# ------------------------------------------------------------------------ 2. column handling
@pytest.mark.parametrize("C_", [16, 4096, 4096 + 16, 8192 + 48])
@pytest.mark.parametrize("k,p", [(4, 2), (16, 8)])
def test_cell_sizes(ctx, ecglib, oracle, k, p, C_):
    check(ctx, ecglib, oracle, k, p, C_, um.some_masks(k), ptr_kernel(p))


@pytest.mark.parametrize("k,p", [(4, 2), (16, 8)])
def test_column_and_row_loops_stride(ctx, ecglib, oracle, k, p):
    """3 columns on 2 column blocks, 7 stripes on 3 block rows."""
    masks = [m for m in um.some_masks(k) if m][:5] + [0, 1 << k]
    assert len(masks) == 7
    ctx.set_launch(2, 3, 0)
    try:
        for flags in (0, ecglib.RM_SPARSE):
            check(ctx, ecglib, oracle, k, p, 8192 + 48, masks, ptr_kernel(p), flags=flags)
    finally:
        ctx.set_launch(0, 0, 0)


@pytest.mark.parametrize("variant", [0, 2])
def test_work_at_the_ends_of_the_block_rows(ctx, ecglib, oracle, variant):
    """S = 130: work only at stripes 0, 63, 64, 127, 128 and 129 and an invalid word at 65, with and
    without ECG_RM_SPARSE."""
    k, p, C_, S_ = 8, 2, 4096 + 16, 130
    masks = [0] * S_
    masks[0], masks[63], masks[64], masks[127], masks[128], masks[129] = 0x81, 0xFF, 0x02, 0x10, 0x03, 0x7E
    masks[65] = 1 << k
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, S_))
    ctx.set_launch(0, 0, variant)
    try:
        want = rig.expect(oracle, masks)
        for flags in (0, ecglib.RM_SPARSE):
            got, res, name = rig.run(ecglib, masks, flags)
            assert name == (BYTE_KERNEL if variant else ptr_kernel(p))
            assert res == [6, 65, 2 + 8 + 1 + 1 + 2 + 6, 1] == um.model(masks, k)
            same(got, want)
    finally:
        ctx.set_launch(0, 0, 0)
        rig.free()


# ------------------------------------------------------------------------------ 3. byte kernel
@pytest.mark.parametrize("c", [1, 4 + 2, 2 * 4 + 1], ids=["old", "new", "parity"])
def test_one_entry_off_16_bytes_sends_the_whole_launch_to_the_byte_kernel(ctx, ecglib, oracle, c):
    k, p = 4, 2
    masks = um.some_masks(k)
    check(ctx, ecglib, oracle, k, p, 4096, masks, ptr_kernel(p))                # all aligned: the lanes
    check(ctx, ecglib, oracle, k, p, 4096, masks, BYTE_KERNEL, skew=lambda s, cc: 8 if (s, cc) == (3, c) else 0)


@pytest.mark.parametrize("C_", [1, 17, 4097])
@pytest.mark.parametrize("k,p", [(4, 2), (8, 3), (5, 4), (16, 8)])
def test_byte_kernel_every_cell_skewed(ctx, ecglib, oracle, k, p, C_):
    check(ctx, ecglib, oracle, k, p, C_, um.some_masks(k), BYTE_KERNEL, skew=lambda s, c: (s + c) % 16)


@pytest.mark.parametrize("k,p", [(4, 2), (16, 3), (8, 4)])
def test_byte_kernel_forced_gives_the_lane_kernels_bytes(ctx, ecglib, oracle, k, p):
    masks = um.some_masks(k)
    lane = check(ctx, ecglib, oracle, k, p, 4096 + 16, masks, ptr_kernel(p))
    ctx.set_launch(0, 0, 2)
    try:
        byte = check(ctx, ecglib, oracle, k, p, 4096 + 16, masks, BYTE_KERNEL)
    finally:
        ctx.set_launch(0, 0, 0)
    assert np.array_equal(lane, byte)


# ---------------------------------------------------------------------------- 4. strided twin
@pytest.mark.parametrize("k,p,C_", [(4, 2, 4096 + 16), (8, 3, 4096), (16, 8, 48), (5, 4, 17)])
def test_identical_to_update_masks_over_the_gathered_cells(ctx, ecglib, oracle, k, p, C_):
    """The rig's cells gathered into old / new / parity images and passed through
    ecg_update_masks: the parity scattered back and the result words equal the table call's."""
    masks = um.some_masks(k)
    S_ = len(masks)
    skew = (lambda s, c: (s + c) % 16) if C_ % 16 else None
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, S_), skew=skew)
    old = np.stack([np.stack([rig.cell(rig.img, s, j) for j in range(k)]) for s in range(S_)])
    new = np.stack([np.stack([rig.cell(rig.img, s, k + j) for j in range(k)]) for s in range(S_)])
    par = np.stack([np.stack([rig.cell(rig.img, s, 2 * k + r) for r in range(p)]) for s in range(S_)])
    bufs = [ctx.to_device(np.ascontiguousarray(a).reshape(-1)) for a in (old, new, par)]
    mk, res = ctx.alloc(4 * S_), ctx.alloc(32)
    try:
        mk.upload(np.array(masks, dtype=np.uint32).view(np.uint8))
        ctx.update_masks(k, p, C_, S_, bufs[0].ptr, bufs[1].ptr, k * C_, bufs[2].ptr, C_, p * C_, mk.ptr, res.ptr, 0)
        ctx.sync()
        twin = bufs[2].download().reshape(S_, p, C_)
        want = rig.img.copy()
        for s in range(S_):
            for r in range(p):
                rig.cell(want, s, 2 * k + r)[:] = twin[s, r]
        words = [int(v) for v in res.download().view(np.uint64)]
        got, res2, name = rig.run(ecglib, masks)
        assert name == (BYTE_KERNEL if C_ % 16 else ptr_kernel(p))
        assert res2 == words == um.model(masks, k)
        assert not np.array_equal(want, rig.img)
        same(got, want)
        same(got, rig.expect(oracle, masks))
    finally:
        for b in bufs + [mk, res]:
            b.free()
        rig.free()


# -------------------------------------------------------------------------- 5. strided routing
def groups(k, p, C_, S_, hole=0):
    """Three strided groups in one allocation: old [S][k][C], new [S][k][C], parity [S][p][C] with
    `hole` bytes after every stripe's parity cells.  -> (offsets [S][2k+p], size, first hole)."""
    o0 = GUARD
    n0 = o0 + S_ * k * C_ + 64
    p0 = n0 + S_ * k * C_ + 64
    ps = p * C_ + hole
    off = [[o0 + s * k * C_ + j * C_ for j in range(k)] + [n0 + s * k * C_ + j * C_ for j in range(k)] +
           [p0 + s * ps + r * C_ for r in range(p)] for s in range(S_)]
    return np.array(off), p0 + S_ * ps + SLACK * C_ + GUARD, p0 + p * C_


@pytest.mark.parametrize("k,p", [(4, 2), (5, 4), (16, 3)])
def test_three_strided_groups_are_the_strided_call(ctx, ecglib, oracle, k, p):
    C_ = 4096
    masks = um.some_masks(k)
    S_ = len(masks)
    off, size, _ = groups(k, p, C_, S_, hole=64)
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, S_), off=off, size=size)
    try:
        got, res, name = rig.run(ecglib, masks)
        assert name == um.lane_kernel(p)                        # three strided images: the strided call
        assert res == um.model(masks, k)
        same(got, rig.expect(oracle, masks))
        order = list(range(S_))
        order[0], order[S_ - 1] = order[S_ - 1], order[0]       # two valid stripes exchanged: no stride
        pm = [masks[s] for s in order]
        got, res, name = rig.run(ecglib, pm, rows=rig.rows(order))
        assert name == ptr_kernel(p)
        assert res == um.model(pm, k)
        same(got, rig.expect(oracle, pm, rig.rows(order)))
    finally:
        rig.free()


@pytest.mark.parametrize("k,p", [(4, 2), (16, 3)])
def test_one_stripe_is_strided_wherever_its_groups_lie(ctx, ecglib, oracle, k, p):
    """S = 1: old cells C apart, new cells C apart, parity cells evenly spaced, the three groups
    anywhere."""
    C_, m = 4096, (1 << k) - 2
    n0 = GUARD                                  # new first, then old, then parity
    o0 = n0 + k * C_ + 32
    p0 = o0 + k * C_ + 4096 + 16
    off = [[o0 + j * C_ for j in range(k)] + [n0 + j * C_ for j in range(k)] +
           [p0 + r * (C_ + 160) for r in range(p)]]
    size = p0 + p * (C_ + 160) + SLACK * C_ + GUARD
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, 1), off=np.array(off), size=size)
    try:
        got, res, name = rig.run(ecglib, [m])
        assert name == um.lane_kernel(p)
        assert res == um.model([m], k)
        want = rig.expect(oracle, [m])
        assert not np.array_equal(want, rig.img)
        same(got, want)
    finally:
        rig.free()


def test_masks_in_a_gap_of_the_parity_span_run_the_table_kernel(ctx, ecglib, oracle):
    """The strided call would refuse masks inside the parity's byte span; no cell shares a byte
    with them, so the table kernel runs, and runs right."""
    k, p, C_ = 4, 2, 4096
    masks = um.some_masks(k)
    S_ = len(masks)
    assert 4 * S_ <= 64
    off, size, hole = groups(k, p, C_, S_, hole=64)
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, S_), off=off, size=size, masks_at=hole)
    try:
        rig.upload(masks)                                       # the words are part of the image now
        want = rig.expect(oracle, masks)
        got, res, name = rig.run(ecglib, masks)
        assert name == ptr_kernel(p)
        assert res == um.model(masks, k)
        same(got, want)                                         # the mask words included
    finally:
        rig.free()


# ------------------------------------------------------- 6. tables that are not one-to-one
def test_rows_in_a_permuted_stripe_order(ctx, ecglib, oracle):
    k, p, C_ = 8, 2, 4096 + 16
    masks = um.some_masks(k)
    S_ = len(masks)
    order = [int(i) for i in np.random.default_rng(7).permutation(S_)]
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, S_))
    try:
        want = rig.expect(oracle, masks, rig.rows(order))
        assert not np.array_equal(want, rig.expect(oracle, masks))
        got, res, name = rig.run(ecglib, masks, rows=rig.rows(order))
        assert name == ptr_kernel(p)
        assert res == um.model(masks, k)
        same(got, want)
    finally:
        rig.free()


def test_old_entry_equal_to_its_new_entry_contributes_nothing(ctx, ecglib, oracle):
    k, p, C_ = 8, 2, 4096
    masks = um.some_masks(k)
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, len(masks)))
    try:
        rows = rig.rows()
        rows[:, k + 0] = rows[:, 0]                             # cell 0: new entry = old entry
        rows[:, 3] = rows[:, k + 3]                             # cell 3: old entry = new entry
        want = rig.expect(oracle, masks, rows)
        other = [m & ~0b1001 for m in masks]
        assert np.array_equal(want, rig.expect(oracle, [m if um.valid(m, k) else 0 for m in other]))
        got, res, name = rig.run(ecglib, masks, rows=rows)
        assert name == ptr_kernel(p)
        assert res == um.model(masks, k)                        # named cells count, whatever they hold
        same(got, want)
    finally:
        rig.free()


def test_all_rows_share_one_old_cell(ctx, ecglib, oracle):
    k, p, C_ = 4, 2, 4096
    masks = um.every_mask(k)
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, len(masks)))
    try:
        rows = rig.rows()
        rows[:, 1] = rows[0, 1]
        want = rig.expect(oracle, masks, rows)
        got, res, name = rig.run(ecglib, masks, rows=rows)
        assert name == ptr_kernel(p)
        assert res == um.model(masks, k)
        same(got, want)
    finally:
        rig.free()


# -------------------------------------------------------------------- 7. any mask, nothing to do
def test_any_mask_value_is_safe(ctx, ecglib, oracle):
    """64 seeded random 32-bit words and the edge values: no byte outside the parity cells of the
    valid stripes changes, whichever kernel, grid and flag."""
    k, p, C_ = 5, 2, 4096
    rng = np.random.default_rng(5)
    masks = [int(x) for x in rng.integers(0, 1 << 32, 64)] + [0xFFFFFFFF, 1 << k, 1 << 31]
    masks += [int(x) for x in rng.integers(0, 1 << (k + 1), 29)]
    words = um.model(masks, k)
    assert words[0] >= 5 and words[3] >= 64
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, len(masks)))
    try:
        want = rig.expect(oracle, masks)
        for grid in ((0, 0), (1, 2)):
            for variant in (0, 2):
                for flags in (0, ecglib.RM_SPARSE):
                    ctx.set_launch(grid[0], grid[1], variant)
                    try:
                        got, res, name = rig.run(ecglib, masks, flags)
                    finally:
                        ctx.set_launch(0, 0, 0)
                    assert name == (BYTE_KERNEL if variant else ptr_kernel(p))
                    assert res == words, (grid, variant, flags)
                    same(got, want)
    finally:
        rig.free()


def test_nothing_to_do_presets_the_result(ctx, ecglib, oracle):
    k, p, C_, S_ = 4, 2, 4096, 6
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, S_))
    L = ecglib.lib()
    try:
        rig.upload([3] * S_)
        arr = (C.c_void_p * (S_ * rig.n))(*rig.table())
        for S__, C__, cells in ((0, C_, None), (S_, 0, None), (0, 0, None), (0, C_, arr), (S_, 0, arr)):
            rig.result.fill(0xEE)
            assert L.ecg_update_masks_ptrs(ctx.h, k, p, C__, S__, cells, rig.masks_ptr, rig.result.ptr, 0, None) == 0
            got, res = rig.finish()
            assert res == [0, U64MAX, 0, 0]
            same(got, rig.img)
        got, res, _ = rig.run(ecglib, [0] * S_)                 # all-zero masks
        assert res == [0, U64MAX, 0, 0]
        same(got, rig.img)
    finally:
        rig.free()


# ----------------------------------------------------------------------------- 8. table lifetime
def test_the_table_is_copied_before_the_call_returns(ctx, ecglib, oracle):
    k, p, C_, S_ = 8, 2, 64 * 1024, 12
    masks = [m if um.valid(m, k) else 0x5 for m in um.some_masks(k)]
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, S_))
    try:
        want = rig.expect(oracle, masks)
        tab = rig.table()
        arr = (C.c_void_p * len(tab))(*tab)
        rig.upload(masks)
        ctx.update_masks_ptrs(k, p, C_, S_, arr, rig.masks_ptr, rig.result.ptr)
        arr[:] = [rig.buf.ptr + GUARD] * len(tab)              # garbage: every entry one address
        got, res = rig.finish()
        assert res == um.model(masks, k)
        same(got, want)
    finally:
        rig.free()


def test_two_calls_back_to_back_on_one_stream(ctx, ecglib, oracle):
    shapes = [(8, 2, 4096), (4, 2, 8192)]
    rigs = [PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, len(um.some_masks(k)))) for k, p, C_ in shapes]
    try:
        wants = []
        for rig in rigs:
            masks = um.some_masks(rig.k)
            wants.append(rig.expect(oracle, masks))
            rig.upload(masks)
        ctx.sync()
        for rig in rigs:                        # no sync in between
            ctx.update_masks_ptrs(rig.k, rig.p, rig.C, rig.S, rig.table(), rig.masks_ptr, rig.result.ptr)
        for rig, want in zip(rigs, wants):
            got, res = rig.finish()
            assert res == um.model(um.some_masks(rig.k), rig.k)
            same(got, want)
    finally:
        for rig in rigs:
            rig.free()


# ------------------------------------------------- 9. the device chain over one table
@pytest.mark.parametrize("k,p", [(4, 2), (8, 3)])
def test_checksum_driven_update_over_one_table(ctx, ecglib, oracle, k, p):
    """csum_cells_ptrs over the [S][2k+p] table, memset(masks), csum_mask(got = the old cells'
    slots, want = the new cells' slots), update_masks_ptrs: one stream, one sync.  The new cells
    differ from the old in chosen cells only; the parity comes out as the oracle's encode of the
    new data for the changed stripes, clean stripes untouched."""
    C_, S_, htype, n = 8192, 10, ecglib.HASH_CRC32, 2 * k + p
    old, _, par = um.images(oracle, k, p, C_, S_)
    changed = {0: [0], 1: [k - 1], 3: [1, 2, k - 1], 4: list(range(k)), 7: [k // 2], 9: [0, k - 1]}
    new = old.copy()
    for s, js in changed.items():
        for i, j in enumerate(js):
            new[s, j, (s * 131 + i * 977 + (4096 if i % 2 else 0)) % C_] ^= 0x40 >> (i % 7)    # one bit per cell
    want_masks = [sum(1 << j for j in changed.get(s, [])) for s in range(S_)]
    rig = PtrRig(ctx, k, p, C_, np.concatenate([old, new, par.transpose(1, 0, 2)], axis=1))
    nch = ecglib.lib().ecg_csum_chunk_count(4096, 1, 0, C_)
    assert nch == 2
    sums = ctx.alloc(4 * S_ * n * nch)
    try:
        rig.upload([0] * S_)
        rig.own_masks.fill(0xEE)
        tab = rig.table()
        ctx.csum_cells_ptrs(htype, 4096, 1, C_, tab, sums.ptr)
        rig.own_masks.fill(0)
        ctx.csum_mask(htype, sums.ptr, sums.ptr + 4 * k * nch, S_, k, nch, n * nch, nch, 0, rig.masks_ptr)
        ctx.update_masks_ptrs(k, p, C_, S_, tab, rig.masks_ptr, rig.result.ptr)
        assert ecglib.last_kernel() == ptr_kernel(p)
        rig.words = np.array(want_masks, np.uint32)             # what csum_mask is to have written
        got, res = rig.finish()
        assert res == [len(changed), U64MAX, sum(len(js) for js in changed.values()), 0]
        enc = oracle.encode_batch(k, p, C_, S_, new.reshape(-1)).reshape(p, S_, C_)
        want = rig.img.copy()
        for s in changed:
            for r in range(p):
                rig.cell(want, s, 2 * k + r)[:] = enc[r, s]
        assert not np.array_equal(want, rig.img)
        same(got, want)
    finally:
        sums.free()
        rig.free()


# ------------------------------------------------------------------------ 10. arguments, stats
def test_argument_errors_on_a_live_context(ctx, ecglib, oracle):
    L = ecglib.lib()
    k, p, C_, S_ = 4, 2, 4096, 9
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, S_))
    n = rig.n
    try:
        rig.upload([1] * S_)
        tab = rig.table()

        def call(cells=tab, masks=rig.masks_ptr, result=rig.result.ptr, flags=0):
            arr = None if cells is None else (C.c_void_p * len(cells))(*cells)
            return L.ecg_update_masks_ptrs(ctx.h, k, p, C_, S_, arr, masks, result, flags, None)

        assert call(cells=None) == -ecglib.DER_INVAL
        assert L.ecg_strerror() == b"update_masks_ptrs: NULL cells"
        for i in (0, 7, S_ * n - 1):
            assert call(cells=tab[:i] + [None] + tab[i + 1:]) == -ecglib.DER_INVAL
            assert L.ecg_strerror() == b"update_masks_ptrs: NULL cell %d" % i, L.ecg_strerror()
        for i in (2 * n + 1, 2 * n + k + 1, 2 * n + 2 * k + 1):        # an old, a new and a parity cell
            cell = tab[i]
            for inside in (cell, cell + C_ - 4, cell - 4 * S_ + 4):
                assert call(masks=inside) == -ecglib.DER_INVAL          # masks inside a cell
                assert b"update_masks_ptrs: masks overlaps cell" in L.ecg_strerror(), L.ecg_strerror()
            for inside in (cell, cell + C_ - 8, cell - 24):
                assert call(result=inside) == -ecglib.DER_INVAL         # result inside a cell
                assert b"update_masks_ptrs: result overlaps cell" in L.ecg_strerror(), L.ecg_strerror()
        assert call(masks=tab[5]) == -ecglib.DER_INVAL
        assert L.ecg_strerror() == b"update_masks_ptrs: masks overlaps cell 5", L.ecg_strerror()
        for flags in (ecglib.UM_PACKED, ecglib.UM_PACKED | ecglib.RM_SPARSE):
            assert call(flags=flags) == -ecglib.DER_INVAL
            assert b"update_masks_ptrs: ECG_UM_PACKED" in L.ecg_strerror()
        got, _ = rig.finish()
        same(got, rig.img)                                      # none of the calls above wrote a cell
    finally:
        rig.free()


def test_counts_one_launch_and_no_update_cells(ctx, ecglib, oracle):
    rig = PtrRig(ctx, 4, 2, 4096, contents(oracle, 4, 2, 4096, 6))
    masks = [1, 3, 0, 15, 2, 8]
    try:
        rig.run(ecglib, masks)
        before = ctx.stats()
        _, _, name = rig.run(ecglib, masks)
        after = ctx.stats()
        assert name == ptr_kernel(2)
        assert after["launches"] == before["launches"] + 1
        assert after["update_cells"] == before["update_cells"]          # the count lives on the device
        assert after["update_bytes"] == before["update_bytes"]
    finally:
        rig.free()
