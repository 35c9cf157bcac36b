"""The cell-table checksum calls on the GPU: ecg_csum_masked_ptrs, ecg_csum_cells_ptrs and
ecg_recover_masks_ptrs_csum.  The cells live where test_gpu_recover_masks_ptrs.PtrRig puts them --
permuted slots of one allocation with 48-byte 0xA5 gaps -- and the expected checksums come from one
oracle.csum_extents call over the gathered cells (test_gpu_csum_masked.reference); that module's
numpy model of the selection rule picks the slots and gives the result words.  Every comparison is
exact and covers whole allocations: a checksum array is pre-filled with 0xA5 between 0xA5 guards, so
a write to a slot that is not selected, or outside the array, shows; the image and the masks are
read only for the checksum calls and are compared as well."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from tests import test_gpu_csum_masked as cm
from tests.test_gpu_csum_masked import GEOMETRY, TYPES, expect_array, reference, seeded_masks, words
from tests.test_gpu_recover_masks_ptrs import PtrRig

gpu = pytest.mark.gpu

U64MAX, GUARD, FILL, CL = cm.U64MAX, cm.GUARD, cm.FILL, cm.CL
CRC = {1: "crc16", 2: "crc32", 3: "crc64"}


def ptr_kernel(htype, bytewise, family="masked"):
    if htype == 7:
        return f"ecg_adler_{family}_ptr_kernel" + ("<bytes>" if bytewise else "")
    return f"ecg_crc_{family}_ptr_kernel<{CRC[htype]}" + (",bytes>" if bytewise else ">")


def strided_kernel(htype, bytewise=False):
    if htype == 7:
        return "ecg_adler_masked_kernel" + ("<bytes>" if bytewise else "")
    return f"ecg_crc_masked_kernel<{CRC[htype]}" + (",bytes>" if bytewise else ">")


def same(got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8], bad.size)


def blank(shape):
    return np.full(shape, FILL, dtype=np.uint8)


class Sums:
    """A checksum array of `shape` bytes ([rows][k+p][nch][cl]) at byte cskew of its 16-byte aligned
    place between 0xA5 guards; the pre-fill is 0xA5 too."""

    def __init__(self, ctx, shape, cskew=0):
        self.shape, self.base, self.bytes = tuple(shape), GUARD + cskew, int(np.prod(shape))
        self.buf = ctx.alloc(self.base + self.bytes + GUARD)
        self.ptr = self.buf.ptr + self.base

    def image(self, arr=None):
        a = blank(self.base + self.bytes + GUARD)
        if arr is not None:
            a[self.base:self.base + self.bytes] = arr.reshape(-1)
        return a

    def reset(self):
        self.buf.upload(self.image())

    def free(self):
        self.buf.free()


def load(rig, masks, *sums):
    w = np.array(masks, dtype=np.uint32)
    rig.buf.upload(rig.img)
    rig.masks.upload(w.view(np.uint8))
    rig.result.fill(0xEE)
    for s in sums:
        s.reset()
    return w


def run(ctx, ecglib, rig, sums, masks, htype, cs, rec, which, flags=0, table=None):
    """Upload everything, one ecg_csum_masked_ptrs over len(masks) table rows, one sync.
    -> (checksum allocation, result words, kernel); the image and the masks must be unchanged."""
    w = load(rig, masks, sums)
    ctx.csum_masked_ptrs(htype, cs, rec, rig.k, rig.p, rig.C, len(masks), rig.table() if table is None else table,
                         rig.masks.ptr, which, sums.ptr, rig.result.ptr, flags)
    name = ecglib.last_kernel()
    ctx.sync()
    assert np.array_equal(rig.masks.download(4 * len(masks)).view(np.uint32), w)
    same(rig.buf.download(), rig.img)
    return sums.buf.download(), rig.words(), name


def strided_twin(ctx, k, p, cells, masks, htype, cs, rec, which, nch):
    """ecg_csum_masked over the same cells gathered into one image [S][k+p][C]:
    -> (the [S][k+p][nch][cl] array it leaves of a 0xA5 pre-fill, its result words)."""
    S_, n, C_ = cells.shape
    img, mk, res = ctx.to_device(cells.reshape(-1)), ctx.alloc(4 * S_), ctx.alloc(32)
    out = ctx.alloc(S_ * n * nch * CL[htype])
    try:
        mk.upload(np.array(masks, dtype=np.uint32).view(np.uint8))
        out.fill(FILL)
        ctx.csum_masked(htype, cs, rec, k, p, C_, S_, img.ptr, n * C_, mk.ptr, which, out.ptr, res.ptr)
        ctx.sync()
        return out.download().reshape(S_, n, nch, CL[htype]), [int(v) for v in res.download().view(np.uint64)]
    finally:
        for b in (img, mk, res, out):
            b.free()


# ------------------------------------------------------------ 1. every erasure set
@gpu
@pytest.mark.parametrize("which", [1, 2, 3])
@pytest.mark.parametrize("k,p,htype", [(2, 1, 2), (4, 2, 1), (4, 2, 2), (4, 2, 3), (4, 2, 7), (16, 3, 2)])
def test_every_erasure_set(ctx, ecglib, oracle, k, p, htype, which):
    """Stripe i carries set i; then mask 0, p+1 bits and bit k+p.  Chunks of 32 and 16 bytes."""
    C_, cs = 48, 32
    masks = cm.all_sets(k, p) + [0, cm.bits(range(p + 1)), 1 | 1 << (k + p)]
    cells = cm.random_cells(k, p, C_, len(masks))
    rig = PtrRig(ctx, k, p, C_, cells)
    gathered = np.ascontiguousarray(rig.gather(rig.img))
    ref = reference(oracle, ("rnd", k, p, C_, len(masks)), htype, cs, 1, gathered)
    assert ref.shape[2] == 2
    sums = Sums(ctx, ref.shape)
    try:
        got, res, name = run(ctx, ecglib, rig, sums, masks, htype, cs, 1, which)
        assert name == ptr_kernel(htype, False), name
        want = expect_array(ref, masks, k, p, which, start=blank(ref.shape))
        same(got, sums.image(want))
        twin, twin_words = strided_twin(ctx, k, p, gathered, masks, htype, cs, 1, which, 2)
        assert res == words(masks, k, p, which) == twin_words
        assert np.array_equal(twin, want)
    finally:
        rig.free()
        sums.free()


# --------------------------------------------------------------------- 2. geometry
@gpu
@pytest.mark.parametrize("htype", TYPES)
@pytest.mark.parametrize("C_,cs,rec,skew,bytewise", GEOMETRY)
def test_geometry(ctx, ecglib, oracle, C_, cs, rec, skew, bytewise, htype):
    k, p, S_ = 4, 2, 8
    masks = seeded_masks(k, p, S_)
    masks[5] = 0                                # a clean stripe among them
    cells = cm.random_cells(k, p, C_, S_)
    ref = reference(oracle, ("rnd", k, p, C_, S_), htype, cs, rec, cells)
    rig = PtrRig(ctx, k, p, C_, cells, skew=(lambda s, c: skew) if skew else None)
    sums = Sums(ctx, ref.shape)
    try:
        for which in (3, 1):
            got, res, name = run(ctx, ecglib, rig, sums, masks, htype, cs, rec, which)
            assert name == ptr_kernel(htype, bytewise), name
            assert res == words(masks, k, p, which)
            same(got, sums.image(expect_array(ref, masks, k, p, which, start=blank(ref.shape))))
    finally:
        rig.free()
        sums.free()


@gpu
@pytest.mark.parametrize("htype", TYPES)
def test_one_misaligned_entry_sends_the_whole_launch_to_the_byte_kernel(ctx, ecglib, oracle, htype):
    k, p, S_, C_, cs = 4, 2, 8, 8192 + 48, 4096
    masks = seeded_masks(k, p, S_)
    cells = cm.random_cells(k, p, C_, S_)
    ref = reference(oracle, ("rnd", k, p, C_, S_), htype, cs, 1, cells)
    sums = Sums(ctx, ref.shape)
    try:
        for skew, bytewise in ((None, False), (lambda s, c: 1 if (s, c) == (3, 1) else 0, True)):
            rig = PtrRig(ctx, k, p, C_, cells, skew=skew)
            try:
                assert sum(a % 16 != 0 for a in rig.table()) == (1 if bytewise else 0)
                # no mask selects the one skewed cell: every entry counts, selected or not
                only = [(m & ~(1 << 1) or 1) if s == 3 else m for s, m in enumerate(masks)]
                got, res, name = run(ctx, ecglib, rig, sums, only, htype, cs, 1, 1)
                assert name == ptr_kernel(htype, bytewise), name
                assert res == words(only, k, p, 1)
                same(got, sums.image(expect_array(ref, only, k, p, 1, start=blank(ref.shape))))
            finally:
                rig.free()
    finally:
        sums.free()


# ------------------------------------------------------ 3. csums at odd byte offsets
@gpu
@pytest.mark.parametrize("htype,cskew", [(1, 1), (3, 3)])
def test_checksum_array_at_odd_bytes(ctx, ecglib, oracle, htype, cskew):
    k, p, S_, C_, cs = 4, 2, 8, 300, 100
    masks = seeded_masks(k, p, S_)
    cells = cm.random_cells(k, p, C_, S_)
    ref = reference(oracle, ("rnd", k, p, C_, S_), htype, cs, 1, cells)
    rig, sums = PtrRig(ctx, k, p, C_, cells), Sums(ctx, ref.shape, cskew=cskew)
    try:
        assert sums.ptr % 2 == 1
        for which in (1, 3):
            got, res, _ = run(ctx, ecglib, rig, sums, masks, htype, cs, 1, which)
            assert res == words(masks, k, p, which)
            same(got, sums.image(expect_array(ref, masks, k, p, which, start=blank(ref.shape))))
    finally:
        rig.free()
        sums.free()


# ------------------------------------------------------- 4. any mask value is safe
@gpu
def test_any_mask_value_is_safe(ctx, ecglib, oracle):
    k, p, C_, cs, htype = 4, 2, 256, 128, 2
    rng = np.random.default_rng(404)
    masks = [int(rng.integers(0, 1 << 32)) for _ in range(64)] + [0xFFFFFFFF]
    cells = cm.random_cells(k, p, C_, len(masks))
    ref = reference(oracle, ("rnd", k, p, C_, len(masks)), htype, cs, 1, cells)
    rig, sums = PtrRig(ctx, k, p, C_, cells), Sums(ctx, ref.shape)
    try:
        for which in (1, 2, 3):
            got, res, name = run(ctx, ecglib, rig, sums, masks, htype, cs, 1, which)     # image unchanged: in run
            assert name == ptr_kernel(htype, False)
            assert res == words(masks, k, p, which)
            same(got, sums.image(expect_array(ref, masks, k, p, which, start=blank(ref.shape))))
        # and every one of them a set once the high bits are cut: the slots do fill
        low = [m & 0x21 or 1 for m in masks]
        got, res, _ = run(ctx, ecglib, rig, sums, low, htype, cs, 1, 3)
        assert res == words(low, k, p, 3) and res[0] == len(masks)
        same(got, sums.image(expect_array(ref, low, k, p, 3, start=blank(ref.shape))))
    finally:
        rig.free()
        sums.free()


# ----------------------------------------------------------------- 5. table handling
@gpu
def test_rows_reordered_and_duplicated(ctx, ecglib, oracle):
    """Row r of the table is stripe order[r]; stripe 2 is listed twice, under two different
    masks, and both rows' slots fill."""
    k, p, S_, C_, cs, htype = 4, 2, 8, 4096 + 16, 4096, 2
    cells = cm.random_cells(k, p, C_, S_)
    ref = reference(oracle, ("rnd", k, p, C_, S_), htype, cs, 1, cells)
    order = [5, 2, 7, 0, 2, 1, 6, 3]
    masks = seeded_masks(k, p, len(order))
    assert masks[1] != masks[4]
    rig = PtrRig(ctx, k, p, C_, cells)
    sums = Sums(ctx, (len(order),) + ref.shape[1:])
    try:
        for which in (1, 3):
            got, res, name = run(ctx, ecglib, rig, sums, masks, htype, cs, 1, which, table=rig.table(order))
            assert name == ptr_kernel(htype, False)
            assert res == words(masks, k, p, which)
            same(got, sums.image(expect_array(ref[order], masks, k, p, which, start=blank(sums.shape))))
    finally:
        rig.free()
        sums.free()


@gpu
def test_cells_in_two_allocations(ctx, ecglib, oracle):
    k, p, C_, cs, htype = 4, 2, 4096, 2048, 3
    a = PtrRig(ctx, k, p, C_, cm.random_cells(k, p, C_, 5))
    b = PtrRig(ctx, k, p, C_, cm.random_cells(k, p, C_, 4))
    cells = np.concatenate([cm.random_cells(k, p, C_, 5), cm.random_cells(k, p, C_, 4)])
    ref = reference(oracle, ("rnd5+4", k, p, C_), htype, cs, 1, cells)
    masks = seeded_masks(k, p, 9)
    mk, sums = ctx.alloc(4 * 9), Sums(ctx, ref.shape)
    try:
        for r in (a, b):
            r.buf.upload(r.img)
        mk.upload(np.array(masks, dtype=np.uint32).view(np.uint8))
        sums.reset()
        ctx.csum_masked_ptrs(htype, cs, 1, k, p, C_, 9, a.table() + b.table(), mk.ptr, 3, sums.ptr, a.result.ptr)
        ctx.sync()
        assert a.words() == words(masks, k, p, 3)
        same(sums.buf.download(), sums.image(expect_array(ref, masks, k, p, 3, start=blank(ref.shape))))
        for r in (a, b):
            same(r.buf.download(), r.img)
    finally:
        for r in (a, b, mk, sums):
            r.free()


@gpu
def test_the_table_is_copied_before_the_call_returns(ctx, ecglib, oracle):
    """The caller's array is zeroed as soon as the call is back and before the sync: a late
    reader would chase NULL."""
    k, p, S_, C_, cs, htype = 8, 2, 12, 16384, 4096, 2
    cells = cm.random_cells(k, p, C_, S_)
    ref = reference(oracle, ("rnd", k, p, C_, S_), htype, cs, 1, cells)
    masks = seeded_masks(k, p, S_)
    rig, sums = PtrRig(ctx, k, p, C_, cells), Sums(ctx, ref.shape)
    try:
        load(rig, masks, sums)
        tab = rig.table()
        arr = (C.c_void_p * len(tab))(*tab)
        ctx.sync()
        ctx.csum_masked_ptrs(htype, cs, 1, k, p, C_, S_, arr, rig.masks.ptr, 3, sums.ptr, rig.result.ptr)
        C.memset(arr, 0, C.sizeof(arr))
        ctx.sync()
        assert rig.words() == words(masks, k, p, 3)
        same(sums.buf.download(), sums.image(expect_array(ref, masks, k, p, 3, start=blank(ref.shape))))
        same(rig.buf.download(), rig.img)
    finally:
        rig.free()
        sums.free()


@gpu
def test_two_calls_back_to_back_on_one_stream(ctx, ecglib, oracle):
    """Two tables through the scratch slots with no sync in between, then a third call that must
    wait for the first one's slot."""
    shapes = [(8, 2, 4096, 11, 2), (4, 2, 8192, 9, 3), (2, 1, 4096, 7, 1)]
    rigs, every, refs, sums = [], [], [], []
    try:
        for k, p, C_, S_, htype in shapes:
            cells = cm.random_cells(k, p, C_, S_)
            refs.append(reference(oracle, ("rnd", k, p, C_, S_), htype, 4096, 1, cells))
            rigs.append(PtrRig(ctx, k, p, C_, cells))
            sums.append(Sums(ctx, refs[-1].shape))
            every.append(seeded_masks(k, p, S_))
            load(rigs[-1], every[-1], sums[-1])
        ctx.sync()
        for rig, sm, masks, (_, _, _, _, htype) in zip(rigs, sums, every, shapes):       # no sync in between
            ctx.csum_masked_ptrs(htype, 4096, 1, rig.k, rig.p, rig.C, rig.S, rig.table(), rig.masks.ptr, 3, sm.ptr,
                                 rig.result.ptr)
        ctx.sync()
        for rig, sm, masks, ref in zip(rigs, sums, every, refs):
            assert rig.words() == words(masks, rig.k, rig.p, 3)
            same(sm.buf.download(), sm.image(expect_array(ref, masks, rig.k, rig.p, 3, start=blank(ref.shape))))
    finally:
        for r in rigs + sums:
            r.free()


@gpu
def test_different_table_users_hand_the_two_slots_to_each_other(ecglib, oracle):
    """Two rounds of recover_masks_ptrs, csum_masked_ptrs, csum_cells_ptrs, matmul_ptrs, update_ptrs
    and recover_masks_ptrs_csum on one stream of a fresh context with no sync in between: every call
    takes the slot the call before last used.  csum_cells_ptrs brings a 72 000-byte table, above the
    64 KiB a slot starts with, so its slot is re-allocated while the other still has a reader.  Each
    call has its own buffers; every output is compared with the oracle after the one sync."""
    k, p, C_, S_, cs, htype, NC = 4, 2, 4096, 5, 2048, 2, 9000
    n, order = k + p, [3, 0, 4, 1, 2]
    masks = seeded_masks(k, p, S_)                              # of the stripes; row r is stripe order[r]
    rows = [masks[s] for s in order]
    nbits = sum(bin(m).count("1") for m in masks)
    cw, rnd = cm.codewords(oracle, k, p, C_, S_), cm.random_cells(k, p, C_, S_)
    ref_cw = reference(oracle, ("cw", k, p, C_, S_), htype, cs, 1, cw)
    ref_rnd = reference(oracle, ("rnd", k, p, C_, S_), htype, cs, 1, rnd)
    small = np.random.default_rng(9000).integers(0, 256, (1, NC, 64), dtype=np.uint8)
    ref_small = reference(oracle, ("small", NC), htype, cs, 1, small)
    perm = np.random.default_rng(9001).permutation(NC)
    en = oracle.cauchy1(k, p)[k:]
    c2 = ecglib.Context(0)
    held = []

    def keep(b):
        held.append(b)
        return b

    def one_round():
        r = SimpleNamespace()
        r.rec, r.clean = erased_rig(c2, oracle, k, p, C_, S_, masks)
        r.msk, r.msums = PtrRig(c2, k, p, C_, rnd), Sums(c2, ref_rnd.shape)
        r.cells, r.csums = c2.alloc(NC * 64), Sums(c2, ref_small.shape)
        r.mm, r.upd = PtrRig(c2, k, p, C_, rnd), PtrRig(c2, k, p, C_, rnd)
        r.both, _ = erased_rig(c2, oracle, k, p, C_, S_, masks)
        r.bsums = Sums(c2, ref_cw.shape)
        for b in vars(r).values():
            if hasattr(b, "free"):
                keep(b)
        return r

    def start(r):
        load(r.rec, rows)
        load(r.msk, rows, r.msums)
        r.cells.upload(small.reshape(-1))
        r.csums.reset()
        for rig in (r.mm, r.upd):
            rig.buf.upload(rig.img)
        load(r.both, rows, r.bsums)

    def calls(r):
        c2.recover_masks_ptrs(k, p, C_, S_, r.rec.table(order), r.rec.masks.ptr, r.rec.result.ptr)
        c2.csum_masked_ptrs(htype, cs, 1, k, p, C_, S_, r.msk.table(order), r.msk.masks.ptr, 3, r.msums.ptr,
                            r.msk.result.ptr)
        c2.csum_cells_ptrs(htype, cs, 1, 64, [r.cells.ptr + 64 * int(i) for i in perm], r.csums.ptr)
        c2.matmul_ptrs(k, p, en, C_, S_, r.mm.table(order))
        assert ecglib.last_kernel().startswith("ecg_mm_ptr_kernel<"), ecglib.last_kernel()
        at = r.upd.buf.ptr + r.upd.off
        c2.update_ptrs(k, p, C_, [(s % k, int(at[s, 0]), int(at[s, 1]), [int(a) for a in at[s, k:]]) for s in order])
        composite(r)

    def composite(r):
        c2.recover_masks_ptrs_csum(k, p, C_, S_, r.both.table(order), r.both.masks.ptr, r.both.result.ptr, htype, cs,
                                   1, r.bsums.ptr)

    def check(r):
        for rig in (r.rec, r.both):
            same(rig.buf.download(), r.clean)
            assert rig.words() == [S_, U64MAX, nbits, 0]
        same(r.msk.buf.download(), r.msk.img)
        assert r.msk.words() == words(rows, k, p, 3)
        same(r.msums.buf.download(), r.msums.image(expect_array(ref_rnd[order], rows, k, p, 3,
                                                                start=blank(ref_rnd.shape))))
        same(r.cells.download(), small.reshape(-1))
        same(r.csums.buf.download(), r.csums.image(ref_small[:, perm]))
        want = r.mm.img.copy()
        for s in range(S_):
            for i, cell in enumerate(oracle.encode_data(en, rnd[s, :k])):
                r.mm.cell(want, s, k + i)[:] = cell
        same(r.mm.buf.download(), want)
        want = r.upd.img.copy()
        for s in range(S_):
            for i, cell in enumerate(oracle.encode_data_update(en, s % k, rnd[s, 0] ^ rnd[s, 1], rnd[s, k:])):
                r.upd.cell(want, s, k + i)[:] = cell
        same(r.upd.buf.download(), want)
        same(r.bsums.buf.download(), r.bsums.image(expect_array(ref_cw[order], rows, k, p, 1,
                                                                start=blank(ref_cw.shape))))

    try:
        rounds = [one_round(), one_round()]
        # the set table and the CRC tables are built, synchronously, on first use: not inside the sequence
        # (one small table: both slots stay at their first 64 KiB)
        start(rounds[0])
        composite(rounds[0])
        c2.sync()
        for r in rounds:
            start(r)
        c2.sync()
        for r in rounds:                                        # no sync in between
            calls(r)
        name = ecglib.last_kernel()
        c2.sync()
        assert name == ptr_kernel(htype, False), name           # a cell-table kernel: no affine route
        for r in rounds:
            check(r)
    finally:
        for b in held:
            b.free()
        c2.close()


@gpu
def test_table_argument_errors(ctx, ecglib):
    """What the host test cannot reach without a context: the table itself."""
    L = ecglib.lib()
    k, p, C_, S_ = 4, 2, 4096, 5
    n = k + p
    rig = PtrRig(ctx, k, p, C_, cm.random_cells(k, p, C_, S_))
    sums = Sums(ctx, (S_, n, 2, 4))
    try:
        load(rig, [1] * S_, sums)
        tab = rig.table()

        def call(cells=tab, masks=rig.masks.ptr, result=rig.result.ptr, csums=sums.ptr):
            arr = None if cells is None else (C.c_void_p * len(cells))(*cells)
            return L.ecg_csum_masked_ptrs(ctx.h, 2, 2048, 1, k, p, C_, S_, arr, masks, 1, csums, result, 0, None)

        assert call(cells=None) == -ecglib.DER_INVAL and b"NULL cells" in L.ecg_strerror()
        for i in (0, 7, S_ * n - 1):
            assert call(cells=tab[:i] + [None] + tab[i + 1:]) == -ecglib.DER_INVAL
            assert b"NULL cell %d" % i in L.ecg_strerror(), L.ecg_strerror()
        cell = tab[2 * n + 3]
        for kw, what in (({"csums": cell + 8}, b"csums overlaps cell %d" % (2 * n + 3)),
                         ({"csums": cell - sums.bytes + 1}, b"csums overlaps cell"),
                         ({"masks": cell + C_ - 4}, b"masks overlaps cell %d" % (2 * n + 3)),
                         ({"result": cell - 24}, b"result overlaps cell %d" % (2 * n + 3)),
                         ({"csums": rig.masks.ptr - sums.bytes + 1}, b"csums overlaps the masks")):
            assert call(**kw) == -ecglib.DER_INVAL, kw
            assert what in L.ecg_strerror(), (kw, L.ecg_strerror())
        assert L.ecg_csum_cells_ptrs(ctx.h, 2, 2048, 1, C_, len(tab), (C.c_void_p * len(tab))(*tab), cell + C_ - 1,
                                     None) == -ecglib.DER_INVAL
        assert b"csums overlaps cell" in L.ecg_strerror()
        # duplicate entries and overlapping cells are legal: the cells are read only
        assert call(cells=tab[:n] * S_) == 0
        assert call(cells=[tab[0] + 16 * i for i in range(S_ * n)]) == 0
        # an empty batch and empty cells preset the result and touch nothing else
        for S__, C__, cells in ((0, C_, None), (S_, 0, None)):
            rig.result.fill(0xEE)
            assert L.ecg_csum_masked_ptrs(ctx.h, 2, 2048, 1, k, p, C__, S__, cells, rig.masks.ptr, 1,
                                          sums.ptr if cells else None, rig.result.ptr, 0, None) == 0
            ctx.sync()
            assert rig.words() == [0, U64MAX, 0, 0]
        ctx.sync()
        same(rig.buf.download(), rig.img)
    finally:
        rig.free()
        sums.free()


# ------------------------------------------------------------------ 6. affine tables
@gpu
@pytest.mark.parametrize("htype", [2, 7])
def test_affine_table_is_the_strided_call(ctx, ecglib, oracle, htype):
    k, p, S_, C_, cs = 4, 2, 9, 4096, 2048
    cells = cm.random_cells(k, p, C_, S_)
    ref = reference(oracle, ("rnd", k, p, C_, S_), htype, cs, 1, cells)
    masks = seeded_masks(k, p, S_)
    rig = PtrRig(ctx, k, p, C_, cells, permute=False, gap=0)
    sums = Sums(ctx, ref.shape)
    try:
        before = ctx.stats()["launches"]
        got, res, name = run(ctx, ecglib, rig, sums, masks, htype, cs, 1, 3)
        assert name == strided_kernel(htype), name              # contiguous: the strided kernel
        want = sums.image(expect_array(ref, masks, k, p, 3, start=blank(ref.shape)))
        assert res == words(masks, k, p, 3)
        same(got, want)
        down = list(range(S_))[::-1]                            # descending: a negative stride
        got, res, name = run(ctx, ecglib, rig, sums, [masks[s] for s in down], htype, cs, 1, 3,
                             table=rig.table(down))
        assert name == strided_kernel(htype), name
        assert res == words(masks, k, p, 3)
        same(got, sums.image(expect_array(ref[down], [masks[s] for s in down], k, p, 3, start=blank(ref.shape))))
        swapped = list(range(S_))
        swapped[1], swapped[S_ - 2] = swapped[S_ - 2], swapped[1]
        got, res, name = run(ctx, ecglib, rig, sums, [masks[s] for s in swapped], htype, cs, 1, 3,
                             table=rig.table(swapped))
        assert name == ptr_kernel(htype, False), name           # two rows exchanged: no stride
        same(got, sums.image(expect_array(ref[swapped], [masks[s] for s in swapped], k, p, 3,
                                          start=blank(ref.shape))))
        # one stripe whose cells are C apart is affine whatever lies around it
        one = Sums(ctx, (1,) + ref.shape[1:])
        try:
            got, res, name = run(ctx, ecglib, rig, one, [masks[4]], htype, cs, 1, 3, table=rig.table([4]))
            assert name == strided_kernel(htype), name
            same(got, one.image(expect_array(ref[4:5], [masks[4]], k, p, 3, start=blank(one.shape))))
        finally:
            one.free()
        assert ctx.stats()["launches"] == before + 4            # one launch a call, the table's fetch not counted
    finally:
        rig.free()
        sums.free()


# ------------------------------------------------------------ 7. ecg_csum_cells_ptrs
@gpu
@pytest.mark.parametrize("skewed", [False, True])
@pytest.mark.parametrize("htype", TYPES)
def test_csum_cells_ptrs(ctx, ecglib, oracle, htype, skewed):
    """A 40-cell table, three chunks a cell with a 48-byte last one, csums at an odd byte."""
    k, p, S_, C_, cs = 4, 1, 8, 8192 + 48, 4096
    cells = cm.random_cells(k, p, C_, S_)
    ref = reference(oracle, ("rnd", k, p, C_, S_), htype, cs, 1, cells)
    rig = PtrRig(ctx, k, p, C_, cells, skew=(lambda s, c: (3 * s + c) % 16) if skewed else None)
    sums = Sums(ctx, ref.shape, cskew=3)
    try:
        assert len(rig.table()) == 40 and ref.shape[2] == 3
        rig.buf.upload(rig.img)
        sums.reset()
        ctx.csum_cells_ptrs(htype, cs, 1, C_, rig.table(), sums.ptr)    # builds and uploads the CRC tables
        ctx.sync()
        sums.reset()
        before = ctx.stats()
        ctx.csum_cells_ptrs(htype, cs, 1, C_, rig.table(), sums.ptr)
        name = ecglib.last_kernel()
        ctx.sync()
        after = ctx.stats()
        assert name == ptr_kernel(htype, skewed, "cells"), name
        assert after["csum_chunks"] == before["csum_chunks"] + 40 * 3
        assert after["launches"] == before["launches"] + 1
        same(sums.buf.download(), sums.image(ref))
        same(rig.buf.download(), rig.img)
        # the empty table and empty cells: nothing queued, nothing written
        sums.reset()
        ctx.csum_cells_ptrs(htype, cs, 1, C_, None, None)
        ctx.csum_cells_ptrs(htype, cs, 1, 0, rig.table(), sums.ptr)
        ctx.sync()
        assert [ctx.stats()[f] for f in ("launches", "csum_chunks")] == [after[f] for f in ("launches", "csum_chunks")]
        same(sums.buf.download(), sums.image())
    finally:
        rig.free()
        sums.free()


# ------------------------------------------------------------------- 8. composite
def erased_rig(ctx, oracle, k, p, C_, S_, masks, **kw):
    rig = PtrRig(ctx, k, p, C_, cm.codewords(oracle, k, p, C_, S_), **kw)
    clean = rig.img.copy()
    rig.erase(masks)
    return rig, clean


@gpu
@pytest.mark.parametrize("one_array", [False, True])
@pytest.mark.parametrize("k,p,htype,C_", [(4, 2, 2, 8192), (8, 3, 3, 4096 + 48), (5, 2, 7, 4099)])
def test_composite_equals_the_two_calls(ctx, ecglib, oracle, k, p, htype, C_, one_array):
    """recover_masks_ptrs, then csum_masked_ptrs (ERASED into csums, SURVIVORS into src_csums; or
    both into one array), run separately from the same start, against the composite: the image,
    both arrays and the result words.  Stripe 3 is clean, stripe 5 cannot be recovered."""
    S_, cs = 9, 4096
    masks = seeded_masks(k, p, S_)
    masks[3], masks[5] = 0, cm.bits(range(p + 1))
    rig, clean = erased_rig(ctx, oracle, k, p, C_, S_, masks)
    nch = -(-C_ // cs)
    shape = (S_, k + p, nch, CL[htype])
    sums, src, res2 = Sums(ctx, shape, cskew=1), Sums(ctx, shape), ctx.alloc(32)
    try:
        load(rig, masks, sums, src)
        ctx.recover_masks_ptrs(k, p, C_, S_, rig.table(), rig.masks.ptr, rig.result.ptr)
        if one_array:
            ctx.csum_masked_ptrs(htype, cs, 1, k, p, C_, S_, rig.table(), rig.masks.ptr, 3, sums.ptr, res2.ptr)
        else:
            ctx.csum_masked_ptrs(htype, cs, 1, k, p, C_, S_, rig.table(), rig.masks.ptr, 1, sums.ptr, res2.ptr)
            ctx.csum_masked_ptrs(htype, cs, 1, k, p, C_, S_, rig.table(), rig.masks.ptr, 2, src.ptr, res2.ptr)
        ctx.sync()
        want = rig.buf.download(), sums.buf.download(), src.buf.download(), rig.words()
        # what the two calls leave is the recovered image and the oracle's checksums of it
        expect = clean.copy()
        for c in range(k + p):
            rig.cell(expect, 5, c)[:] = rig.cell(rig.img, 5, c)
        same(want[0], expect)
        ref = reference(oracle, ("composite", k, p, C_, S_), htype, cs, 1, np.ascontiguousarray(rig.gather(expect)))
        same(want[1], sums.image(expect_array(ref, masks, k, p, 3 if one_array else 1, start=blank(shape))))
        same(want[2], src.image(None if one_array else expect_array(ref, masks, k, p, 2, start=blank(shape))))
        assert want[3] == [S_ - 2, 5, sum(bin(m).count("1") for s, m in enumerate(masks) if s not in (3, 5)), 1]

        load(rig, masks, sums, src)
        before = ctx.stats()["launches"]
        ctx.recover_masks_ptrs_csum(k, p, C_, S_, rig.table(), rig.masks.ptr, rig.result.ptr, htype, cs, 1, sums.ptr,
                                    sums.ptr if one_array else src.ptr)
        name = ecglib.last_kernel()
        ctx.sync()
        assert name == ptr_kernel(htype, C_ % 16 != 0), name
        assert ctx.stats()["launches"] == before + (2 if one_array else 3)
        same(rig.buf.download(), want[0])
        same(sums.buf.download(), want[1])
        same(src.buf.download(), want[2])
        assert rig.words() == want[3]
        # without src_csums: the erased cells' slots alone
        load(rig, masks, sums, src)
        ctx.recover_masks_ptrs_csum(k, p, C_, S_, rig.table(), rig.masks.ptr, rig.result.ptr, htype, cs, 1, sums.ptr)
        ctx.sync()
        same(rig.buf.download(), want[0])
        same(sums.buf.download(), sums.image(expect_array(ref, masks, k, p, 1, start=blank(shape))))
        same(src.buf.download(), src.image())
        assert rig.words() == want[3]
    finally:
        for b in (rig, sums, src, res2):
            b.free()


@gpu
def test_composite_src_csums_overlap_and_table_errors(ctx, ecglib, oracle):
    L = ecglib.lib()
    k, p, C_, S_, cs = 4, 2, 4096, 6, 4096
    masks = seeded_masks(k, p, S_)
    rig, _ = erased_rig(ctx, oracle, k, p, C_, S_, masks)
    sums = Sums(ctx, (2 * S_, k + p, 1, 4))
    try:
        load(rig, masks, sums)
        tab = rig.table()

        def call(cells=tab, csums=sums.ptr, src=None):
            arr = None if cells is None else (C.c_void_p * len(cells))(*cells)
            return L.ecg_recover_masks_ptrs_csum(ctx.h, k, p, C_, S_, arr, rig.masks.ptr, rig.result.ptr, 0, 2, cs, 1,
                                                 csums, src, None)

        half = sums.bytes // 2
        for src in (sums.ptr + 4, sums.ptr + half - 1, sums.ptr - half + 1):
            assert call(src=src) == -ecglib.DER_INVAL
            assert b"src_csums must be csums itself" in L.ecg_strerror(), L.ecg_strerror()
        assert call(cells=None) == -ecglib.DER_INVAL and b"NULL cells" in L.ecg_strerror()
        assert call(cells=tab[:4] + [None] + tab[5:]) == -ecglib.DER_INVAL and b"NULL cell 4" in L.ecg_strerror()
        assert call(csums=tab[7] + 8) == -ecglib.DER_INVAL and b"csums overlaps cell 7" in L.ecg_strerror()
        assert call(src=tab[9] + C_ - 100) == -ecglib.DER_INVAL and b"src_csums overlaps cell 9" in L.ecg_strerror()
        ctx.sync()
        same(rig.buf.download(), rig.img)                       # nothing was queued
        same(sums.buf.download(), sums.image())
        assert call(src=sums.ptr + half) == 0                   # the two halves side by side
        ctx.sync()
        assert rig.words() == [S_, U64MAX, sum(bin(m).count("1") for m in masks), 0]
    finally:
        rig.free()
        sums.free()


@gpu
@pytest.mark.parametrize("one_array", [False, True])
def test_composite_affine_table_reaches_the_strided_kernels(ctx, ecglib, oracle, one_array):
    k, p, C_, S_, cs, htype = 4, 2, 4096, 7, 2048, 2
    masks = seeded_masks(k, p, S_)
    rig, clean = erased_rig(ctx, oracle, k, p, C_, S_, masks, permute=False, gap=0)
    ref = reference(oracle, ("cw", k, p, C_, S_), htype, cs, 1, cm.codewords(oracle, k, p, C_, S_))
    sums, src = Sums(ctx, ref.shape), Sums(ctx, ref.shape)
    try:
        load(rig, masks, sums, src)
        ctx.recover_masks_ptrs_csum(k, p, C_, S_, rig.table(), rig.masks.ptr, rig.result.ptr, htype, cs, 1, sums.ptr,
                                    sums.ptr if one_array else src.ptr)
        name = ecglib.last_kernel()
        ctx.sync()
        assert name == strided_kernel(htype), name
        assert rig.words() == [S_, U64MAX, sum(bin(m).count("1") for m in masks), 0]
        same(rig.buf.download(), clean)
        same(sums.buf.download(), sums.image(expect_array(ref, masks, k, p, 3 if one_array else 1,
                                                          start=blank(ref.shape))))
        same(src.buf.download(), src.image(None if one_array else expect_array(ref, masks, k, p, 2,
                                                                               start=blank(ref.shape))))
    finally:
        for b in (rig, sums, src):
            b.free()


# ------------------------------------------------------------ 9. scrub over a table
@gpu
@pytest.mark.parametrize("k,p", [(4, 1), (8, 3)])
def test_scrub_over_a_table(ctx, ecglib, oracle, k, p):
    """csum_cells_ptrs (good image) -> corrupt -> csum_cells_ptrs -> memset -> csum_mask ->
    recover_masks_ptrs_csum, one sync: the image is the original again, the repaired cells'
    slots hold their stored checksums, and the masks name the corrupted cells."""
    C_, S_, cs, htype = 4096 + 32, 20, 4096, 2
    n, nch = k + p, 2
    cw = cm.codewords(oracle, k, p, C_, S_)
    rig = PtrRig(ctx, k, p, C_, cw)
    shape = (S_, n, nch, 4)
    want, got, fresh = Sums(ctx, shape), Sums(ctx, shape), Sums(ctx, shape, cskew=2)
    try:
        clean = rig.img.copy()
        rig.buf.upload(clean)
        for s in (want, got, fresh):
            s.reset()
        ctx.csum_cells_ptrs(htype, cs, 1, C_, rig.table(), want.ptr)
        ctx.sync()
        ref = reference(oracle, ("cw", k, p, C_, S_), htype, cs, 1, cw)
        same(want.buf.download(), want.image(ref))
        if p == 1:
            wrong = {s: [s % n] for s in range(0, S_, 2)}
        else:
            wrong = {0: [0, 1], 1: [k - 1, k, k + 2], 2: [k, k + 1], 3: [5, 6, 7], 7: [k + 1, 2], 8: [0, k + 2, 3],
                     19: [2, 7]}
        for s, cs_ in wrong.items():
            for i, c in enumerate(cs_):
                rig.cell(rig.img, s, c)[(s * 131 + i * 977) % C_] ^= 0x40 >> i
        rig.buf.upload(rig.img)
        rig.result.fill(0xEE)
        rig.masks.fill(0xEE)
        ctx.csum_cells_ptrs(htype, cs, 1, C_, rig.table(), got.ptr)
        rig.masks.fill(0)
        ctx.csum_mask(htype, got.ptr, want.ptr, S_, n, nch, n * nch, nch, 0, rig.masks.ptr)
        ctx.recover_masks_ptrs_csum(k, p, C_, S_, rig.table(), rig.masks.ptr, rig.result.ptr, htype, cs, 1, fresh.ptr,
                                    flags=ecglib.RM_SPARSE)
        ctx.sync()
        found = [int(m) for m in rig.masks.download().view(np.uint32)]
        assert found == [cm.bits(wrong.get(s, [])) for s in range(S_)]
        assert rig.words() == [len(wrong), U64MAX, sum(len(c) for c in wrong.values()), 0]
        same(rig.buf.download(), clean)
        same(fresh.buf.download(), fresh.image(expect_array(ref, found, k, p, 1, start=blank(shape))))
    finally:
        for b in (rig, want, got, fresh):
            b.free()


# ---------------------------------------------------------------- 10. seeded fuzz
NFUZZ = 24
SHAPES = [(2, 1), (4, 2), (8, 2), (8, 3), (16, 3), (5, 2), (3, 1), (10, 3)]


def draw(i):
    """Case i of the fuzz: every quantity from one seeded generator.  Even cases keep every
    address and size a multiple of 16 (the 16-byte body), odd ones draw them freely."""
    rng = np.random.default_rng(7000 + i)
    k, p = SHAPES[int(rng.integers(len(SHAPES)))]
    aligned = i % 2 == 0
    rec = 16 * int(rng.integers(1, 9)) if aligned else int(rng.choice([1, 1, 2, 3, 4, 7, 8, 24, 33, 100]))
    C_ = rec * int(rng.integers(1, 12288 // rec + 1))
    # about 1 .. 5 chunks a cell; a chunksize below rec makes a record the chunk
    chunksize = max(1, -(-C_ // int(rng.integers(1, 6))) + int(rng.integers(-rec, rec + 1)))
    S_ = int(rng.integers(1, 13))
    n = k + p
    masks = []
    for _ in range(S_):
        kind = rng.integers(10)
        if kind < 7:
            masks.append(cm.bits(rng.choice(n, int(rng.integers(1, p + 1)), replace=False)))
        else:
            masks.append(0 if kind == 7 else int(rng.integers(0, 1 << 32)))
    return SimpleNamespace(k=k, p=p, htype=TYPES[i // 2] if i < 8 else TYPES[int(rng.integers(4))],
                           which=i % 3 + 1, rec=rec, C=C_, chunksize=chunksize, S=S_, aligned=aligned, masks=masks,
                           skew=np.zeros((S_, n), dtype=int) if aligned else rng.integers(0, 16, (S_, n)),
                           order=[int(s) for s in rng.permutation(S_)], cskew=0 if aligned else int(rng.integers(8)),
                           seed=int(rng.integers(1 << 31)))


def test_every_fuzz_draw_is_a_legal_call():
    """No GPU: the generator alone never draws a case the call would refuse, so none is skipped."""
    from daos_amd import ecg

    cases = [draw(i) for i in range(NFUZZ)]
    for d in cases:
        rcs = ecg.lib().ecg_csum_record_chunksize(d.chunksize, d.rec)
        assert d.rec > 0 and d.C % d.rec == 0 and rcs > 0, vars(d)
        assert 0 < d.C <= 12 * 1024 and 1 <= d.S <= 12 and 1 <= d.k <= 16 and 1 <= d.p <= 3
        assert -(-d.C // rcs) <= 12 * 1024 and len(d.masks) == d.S and sorted(d.order) == list(range(d.S))
        if d.aligned:
            assert d.C % 16 == 0 and rcs % 16 == 0 and not d.skew.any()
    assert {d.htype for d in cases} == set(TYPES) and {d.which for d in cases} == {1, 2, 3}
    assert any(d.skew.any() for d in cases) and len({(d.k, d.p) for d in cases}) >= 4


@gpu
@pytest.mark.parametrize("i", range(NFUZZ))
def test_fuzz(ctx, ecglib, oracle, i):
    d = draw(i)
    k, p = d.k, d.p
    cells = np.random.default_rng(d.seed).integers(0, 256, (d.S, k + p, d.C), dtype=np.uint8)
    ref = reference(oracle, ("fuzz", i), d.htype, d.chunksize, d.rec, cells)
    rig = PtrRig(ctx, k, p, d.C, cells, skew=None if d.aligned else (lambda s, c: int(d.skew[s, c])))
    sums = Sums(ctx, ref.shape, cskew=d.cskew)
    try:
        rcs = ecglib.lib().ecg_csum_record_chunksize(d.chunksize, d.rec)
        assert ref.shape[2] == -(-d.C // rcs)
        tab = rig.table(d.order)
        bytewise = any(a % 16 for a in tab) or d.C % 16 != 0 or rcs % 16 != 0
        assert not (d.aligned and bytewise)
        masks = [d.masks[s] for s in d.order]
        got, res, name = run(ctx, ecglib, rig, sums, masks, d.htype, d.chunksize, d.rec, d.which, table=tab)
        assert name == ptr_kernel(d.htype, bytewise), (name, vars(d))
        assert res == words(masks, k, p, d.which), vars(d)
        same(got, sums.image(expect_array(ref[d.order], masks, k, p, d.which, start=blank(ref.shape))))
    finally:
        rig.free()
        sums.free()
