"""ecg_csum_updated, ecg_csum_updated_ptrs and the composites ecg_update_masks_csum /
ecg_update_masks_ptrs_csum on the GPU: the checksums of the parity cells of the stripes a masked
update rewrote, at checksum index s*csum_stripe_stride + r*csum_cell_stride + c.

The expected checksums of a batch come from one oracle.csum_extents call over all its S*p parity
cells; a numpy model of the selection and slot rules (written from the calls' specification)
places them.  Every comparison is exact and covers whole allocations: the checksum array is
pre-filled with 0xEE between 0xA5 guards, so a write to a slot that is not selected or outside the
array shows; the parity arena (cells between 0xA5 filler and guards), the masks and -- for the
composites -- the old and new images are compared as well.

Mask words: every shape sees 0, one bit, all k bits, 1 << k, 0x80000000, 0xFFFFFFFF and bit k-1
alone.  A batch of seven or more stripes carries all seven (the rest seeded); the batches of five
stripes are run twice, with the first and with the last five of them."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U64MAX = (1 << 64) - 1
GUARD = 256                 # keeps arenas 16-byte aligned inside their (256-byte aligned) allocations
FILL, PRE = 0xA5, 0xEE
CL = {1: 2, 2: 4, 3: 8, 7: 4}
TYPES = [1, 2, 3, 7]

_CELLS, _SUMS = {}, {}


# ------------------------------------------------------------------ the model
def read(m, k):
    """ecg_update_mask_read: 0 nothing, -1 a bit at or above k, else the number of cells."""
    return 0 if m == 0 else -1 if m >> k else bin(m).count("1")


def words(masks, k, p):
    ok = [s for s, m in enumerate(masks) if read(int(m), k) > 0]
    bad = [s for s, m in enumerate(masks) if read(int(m), k) < 0]
    return [len(ok), min(bad) if bad else U64MAX, p * len(ok), len(bad)]


def update_words(masks, k):
    """What ecg_update_masks leaves: word 2 counts the data cells applied."""
    w = words(masks, k, 1)
    w[2] = sum(bin(int(m)).count("1") for m in masks if read(int(m), k) > 0)
    return w


def required(k):
    return [0, 1, (1 << k) - 1, 1 << k, 0x80000000, 0xFFFFFFFF, 1 << (k - 1)]


def batches(k, S_, seed=1):
    req = required(k)
    if S_ < len(req):
        return [req[:S_], req[-S_:]]
    rng = np.random.default_rng(1000 * k + S_ + seed)
    rest = [int(rng.integers(0, 1 << k)) if rng.random() < 0.8 else int(rng.integers(0, 1 << 32))
            for _ in range(S_ - len(req))]
    m = np.array(req + rest, dtype=np.uint64)
    rng.shuffle(m)
    return [[int(v) for v in m]]


def expect_sums(ref, masks, k, css, ccs, nslots, start=None):
    """The checksum array, nslots slots of cl bytes, after a call: `start` (default 0xEE
    everywhere) with chunk c of row r of a selected stripe s at index s*css + r*ccs + c."""
    S_, p, nch, cl = ref.shape
    out = np.full((nslots, cl), PRE, dtype=np.uint8) if start is None else start.reshape(nslots, cl).copy()
    for s, m in enumerate(masks):
        if read(int(m), k) > 0:
            for r in range(p):
                at = s * css + r * ccs
                out[at:at + nch] = ref[s, r]
    return out


def random_cells(S_, p, C_):
    key = (S_, p, C_)
    if key not in _CELLS:
        a = np.random.default_rng(31 * S_ + 7 * p + C_).integers(0, 256, (S_, p, C_), dtype=np.uint8)
        a.setflags(write=False)
        _CELLS[key] = a
    return _CELLS[key]


def reference(oracle, key, htype, chunksize, rec, cells):
    """Checksum bytes [S][p][nch][cl] of every parity cell of `cells` ([S][p][C]): one oracle call,
    kept under `key` (which names the cells) and never modified."""
    key = (key, htype, chunksize, rec)
    if key not in _SUMS:
        S_, p, C_ = cells.shape
        v = oracle.csum_extents(htype, chunksize, rec, 0, C_ // rec, cells.reshape(-1), C_, S_ * p)
        b = np.ascontiguousarray(v).view(np.uint8).reshape(S_, p, v.shape[1], CL[htype]).copy()
        b.setflags(write=False)
        _SUMS[key] = b
    return _SUMS[key]


def same(got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8] - GUARD, bad.size)


# -------------------------------------------------------------------- the rig
def client(S_, p, C_, pad=0):
    """[p][S][C] with a row pitch of S*C + pad: (offsets[s][r], cell stride, stripe stride)."""
    pc, ps = S_ * C_ + pad, C_
    return np.array([[r * pc + s * ps for r in range(p)] for s in range(S_)]), pc, ps


def recovery(S_, k, p, C_):
    """The parity columns of [S][k+p][C]."""
    pc, ps = C_, (k + p) * C_
    return np.array([[k * C_ + s * ps + r * pc for r in range(p)] for s in range(S_)]), pc, ps


def descending(S_, p, C_, pad=0):
    """The client layout read from its last stripe down: a negative stripe stride."""
    off, pc, ps = client(S_, p, C_, pad)
    return off[::-1].copy(), pc, -ps


def scattered(S_, p, C_, gap=48, seed=5):
    """Every parity cell in a place of its own, gap bytes and more apart (no two cells share a
    byte); every place 16-byte aligned when C and gap are multiples of 16."""
    order = np.random.default_rng(seed + S_ * p).permutation(S_ * p)
    return (order * (C_ + gap + 32) + (order % 3) * 16).reshape(S_, p), None, None


class Rig:
    """S*p parity cells at byte offsets off[s][r] of a device arena (0xA5 elsewhere, guards around
    it), the mask words, the result, and a checksum array of nslots slots between guards.  skew:
    byte offset of the arena from its 16-byte aligned place; cskew: the same for the checksums."""

    def __init__(self, ctx, k, cells, off, nslots, cl, skew=0, cskew=0):
        self.ctx, self.k = ctx, k
        self.S, self.p, self.C = cells.shape
        self.off = off - off.min()
        self.base = GUARD + skew
        self.img = np.full(self.base + int(self.off.max()) + self.C + GUARD, FILL, dtype=np.uint8)
        for s in range(self.S):
            for r in range(self.p):
                self.cell(self.img, s, r)[:] = cells[s, r]
        self.buf = ctx.alloc(self.img.size)
        self.masks, self.result = ctx.alloc(4 * self.S), ctx.alloc(32)
        self.nslots, self.cl = nslots, cl
        self.cbase, self.cbytes = GUARD + cskew, nslots * cl
        self.csums = ctx.alloc(self.cbase + self.cbytes + GUARD)
        self.cptr = self.csums.ptr + self.cbase
        self.bufs = [self.buf, self.masks, self.result, self.csums]

    def cell(self, img, s, r):
        at = self.base + int(self.off[s, r])
        return img[at:at + self.C]

    def addr(self, s, r):
        return self.buf.ptr + self.base + int(self.off[s, r])

    def sums_image(self, arr=None):
        a = np.full(self.cbase + self.cbytes + GUARD, FILL, dtype=np.uint8)
        a[self.cbase:self.cbase + self.cbytes] = PRE if arr is None else arr.reshape(-1)
        return a

    def load(self, masks):
        self.words = np.array(masks, dtype=np.uint32)
        self.buf.upload(self.img)
        self.masks.upload(self.words.view(np.uint8))
        self.csums.upload(self.sums_image())
        self.result.fill(0xEE)

    def table(self, data=None):
        """The update table [S][2k+p]: the parity addresses, and for the data entries `data`
        ([S][2k] addresses) or addresses that are no memory at all (never NULL)."""
        n, k = 2 * self.k + self.p, self.k
        t = []
        for s in range(self.S):
            t += [int(a) for a in data[s]] if data is not None else [0x1000 + 8 * (s * n + j) + 1 for j in range(2 * k)]
            t += [self.addr(s, r) for r in range(self.p)]
        return t

    def run(self, ecglib, masks, htype, chunksize, rec, strides, css, ccs, coff=0, flags=0, table=None):
        """Upload everything, one call, one sync -> (checksum allocation, result words, kernel); the
        parity arena and the masks are checked to be unchanged."""
        self.load(masks)
        at = self.cptr + coff * self.cl
        if table is not None:
            self.ctx.csum_updated_ptrs(htype, chunksize, rec, self.k, self.p, self.C, self.S, table, self.masks.ptr,
                                       at, css, ccs, self.result.ptr, flags)
        else:
            pc, ps = strides
            self.ctx.csum_updated(htype, chunksize, rec, self.k, self.p, self.C, self.S, self.addr(0, 0), pc, ps,
                                  self.masks.ptr, at, css, ccs, self.result.ptr, flags)
        name = ecglib.last_kernel()
        self.ctx.sync()
        self.read_only()
        return self.csums.download(), self.words64(), name

    def read_only(self):
        assert np.array_equal(self.masks.download().view(np.uint32), self.words)
        assert np.array_equal(self.buf.download(), self.img)

    def words64(self):
        return [int(v) for v in self.result.download().view(np.uint64)]

    def free(self):
        for b in self.bufs:
            b.free()


def check(ctx, ecglib, oracle, k, p, C_, S_, htype, cs, layout, *, rec=1, skew=0, cskew=0, sums="pSn", table=None,
          kernel="updated_kernel", bytes_=False, blocks=0, pad=0):
    """One shape through ecg_csum_updated (or, table = "scattered" / "odd" / "affine",
    ecg_csum_updated_ptrs), every batch of its mask words, against the model."""
    cells = random_cells(S_, p, C_)
    ref = reference(oracle, ("rnd", S_, p, C_), htype, cs, rec, cells)
    nch, cl = ref.shape[2], CL[htype]
    if table in ("scattered", "odd"):
        off, pc, ps = scattered(S_, p, C_)
        if table == "odd":
            off[S_ // 2, p - 1] += 4                                    # one entry off its 16 bytes
    else:
        off, pc, ps = {"client": lambda: client(S_, p, C_, pad), "recovery": lambda: recovery(S_, k, p, C_),
                       "descending": lambda: descending(S_, p, C_, pad)}[layout]()
    # [p][S][nch] with a padded row, or the parity columns of [S][k+p][nch]
    css, ccs, coff, nslots = {"pSn": (nch, S_ * nch + 1, 0, (p - 1) * (S_ * nch + 1) + S_ * nch),
                              "Skpn": ((k + p) * nch, nch, k * nch, S_ * (k + p) * nch)}[sums]
    rig = Rig(ctx, k, cells, off, nslots, cl, skew, cskew)
    L = ecglib.lib()
    try:
        assert L.ecg_set_csum_launch(ctx.h, blocks) == 0
        for masks in batches(k, S_):
            before = ctx.stats()
            got, res, name = rig.run(ecglib, masks, htype, cs, rec, (pc, ps), css, ccs, coff,
                                     table=rig.table() if table else None)
            after = ctx.stats()
            assert kernel in name and ("bytes" in name) == bytes_, name
            assert res == words(masks, k, p), (res, masks)
            want = np.full((nslots, cl), PRE, dtype=np.uint8)
            want[coff:] = expect_sums(ref, masks, k, css, ccs, nslots - coff)
            same(got, rig.sums_image(want))
            if sums == "Skpn":                                          # the data columns stay as they were
                assert (got[rig.cbase:rig.cbase + rig.cbytes].reshape(S_, k + p, nch * cl)[:, :k] == PRE).all()
            assert after["launches"] - before["launches"] == 1
            assert after["csum_chunks"] == before["csum_chunks"]
    finally:
        L.ecg_set_csum_launch(ctx.h, 0)
        rig.free()


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("htype", TYPES)
def test_first_shape_every_hash_type(ctx, ecglib, oracle, htype):
    """(4, 2), C = 4096, two chunks, five stripes: the client layout with a padded pitch."""
    check(ctx, ecglib, oracle, 4, 2, 4096, 5, htype, 2048, "client", pad=512)


@pytest.mark.parametrize("htype", [2, 3])
@pytest.mark.parametrize("k,p", [(2, 1), (16, 3), (8, 8), (16, 8)])
def test_code_shapes_beyond_csum_masked(ctx, ecglib, oracle, k, p, htype):
    check(ctx, ecglib, oracle, k, p, 4096, 7, htype, 2048, "client")


@pytest.mark.parametrize("htype", [2, 3])
def test_ragged_last_chunk(ctx, ecglib, oracle, htype):
    check(ctx, ecglib, oracle, 4, 2, 5136, 5, htype, 2048, "client", pad=16)


@pytest.mark.parametrize("htype", [2, 3, 7])
@pytest.mark.parametrize("skew", [1, 4, 8])
def test_odd_cells_and_skewed_base_run_the_byte_kernels(ctx, ecglib, oracle, htype, skew):
    check(ctx, ecglib, oracle, 4, 2, 4099, 5, htype, 2048, "client", skew=skew, cskew=skew, bytes_=True)


@pytest.mark.parametrize("htype", [2, 3])
def test_skewed_base_alone_runs_the_byte_kernels(ctx, ecglib, oracle, htype):
    check(ctx, ecglib, oracle, 4, 2, 4096, 5, htype, 2048, "client", skew=8, bytes_=True)
    check(ctx, ecglib, oracle, 4, 2, 4096, 5, htype, 2048, "client", pad=8, bytes_=True)     # a stride alone


@pytest.mark.parametrize("htype", [2, 3])
def test_chunk_size_off_16_forces_the_byte_kernels(ctx, ecglib, oracle, htype):
    check(ctx, ecglib, oracle, 4, 2, 4096, 5, htype, 2040, "client", bytes_=True)


@pytest.mark.parametrize("htype", [2, 3])
def test_grid_stride_wraps_under_a_launch_cap(ctx, ecglib, oracle, htype):
    check(ctx, ecglib, oracle, 4, 2, 4096, 130, htype, 2048, "client", blocks=1)


# ----------------------------------------------------------------- 2. layouts
@pytest.mark.parametrize("htype", [1, 2, 3])
def test_recovery_layout_into_the_parity_columns_at_an_odd_byte(ctx, ecglib, oracle, htype):
    check(ctx, ecglib, oracle, 4, 2, 4096, 5, htype, 2048, "recovery", sums="Skpn", cskew=3)


@pytest.mark.parametrize("htype", [2, 3])
def test_descending_image(ctx, ecglib, oracle, htype):
    check(ctx, ecglib, oracle, 4, 2, 4096, 5, htype, 2048, "descending", pad=256)
    check(ctx, ecglib, oracle, 4, 2, 4096, 5, htype, 2048, "descending", sums="Skpn")


def test_csum_mask_sees_the_new_parity_checksums(ctx, ecglib, oracle):
    """The parity columns of an [S][k+p][nch] array that held other checksums: ecg_csum_mask over
    the array names exactly the parity cells of the selected stripes."""
    k, p, C_, S_, htype, cs = 4, 2, 4096, 7, 2, 2048
    cells = random_cells(S_, p, C_)
    ref = reference(oracle, ("rnd", S_, p, C_), htype, cs, 1, cells)
    nch, cl = ref.shape[2], CL[htype]
    off, pc, ps = recovery(S_, k, p, C_)
    rig = Rig(ctx, k, cells, off, S_ * (k + p) * nch, cl)
    stale, out = ctx.alloc(rig.cbytes), ctx.alloc(4 * S_)
    try:
        masks = batches(k, S_)[0]
        stale.upload(rig.sums_image()[rig.cbase:rig.cbase + rig.cbytes])
        got, res, _ = rig.run(ecglib, masks, htype, cs, 1, (pc, ps), (k + p) * nch, nch, k * nch)
        out.fill(0)
        ctx.csum_mask(htype, rig.cptr, stale.ptr, S_, k + p, nch, (k + p) * nch, nch, 0, out.ptr)
        ctx.sync()
        want = [((1 << p) - 1) << k if read(m, k) > 0 else 0 for m in masks]
        assert [int(v) for v in out.download().view(np.uint32)] == want
    finally:
        rig.free()
        stale.free()
        out.free()


# -------------------------------------------------------------- 3. table form
@pytest.mark.parametrize("htype", TYPES)
def test_table_scattered_aligned(ctx, ecglib, oracle, htype):
    check(ctx, ecglib, oracle, 4, 2, 4096, 7, htype, 2048, None, table="scattered", kernel="updated_ptr_kernel")


@pytest.mark.parametrize("htype", [2, 3])
def test_table_one_odd_entry_takes_the_whole_launch_bytewise(ctx, ecglib, oracle, htype):
    check(ctx, ecglib, oracle, 4, 2, 4096, 7, htype, 2048, None, table="odd", kernel="updated_ptr_kernel",
          bytes_=True)


@pytest.mark.parametrize("htype", [2, 3])
def test_table_more_rows_than_csum_masked_and_a_cap(ctx, ecglib, oracle, htype):
    check(ctx, ecglib, oracle, 16, 8, 4099, 7, htype, 2048, None, table="scattered", kernel="updated_ptr_kernel",
          bytes_=True, blocks=1, sums="Skpn", cskew=1)


@pytest.mark.parametrize("layout", ["client", "recovery", "descending"])
def test_affine_table_is_the_strided_call(ctx, ecglib, oracle, layout):
    """Parity entries p0 + s*ps + r*pc: the strided kernel runs; the data entries point at no
    memory at all and are never read."""
    check(ctx, ecglib, oracle, 4, 2, 4096, 7, 2, 2048, layout, table="affine", kernel="updated_kernel", pad=512)


# -------------------------------------------------------------- 4. composites
def update_case(oracle, k, p, C_, S_, masks, seed):
    """old and new images [S][k][C] that differ in every data cell, the oracle's parity of the old
    one [S][p][C], and the parity after the update: re-encoded from the merged image where the
    mask reads as 1..k cells, untouched elsewhere."""
    rng = np.random.default_rng(seed)
    old = rng.integers(0, 256, (S_, k, C_), dtype=np.uint8)
    new = old ^ rng.integers(1, 256, (S_, k, C_), dtype=np.uint8)
    merged = old.copy()
    for s, m in enumerate(masks):
        if read(int(m), k) > 0:
            for j in range(k):
                if m >> j & 1:
                    merged[s, j] = new[s, j]
    par = oracle.encode_batch(k, p, C_, S_, old.reshape(-1)).reshape(p, S_, C_).transpose(1, 0, 2).copy()
    after = oracle.encode_batch(k, p, C_, S_, merged.reshape(-1)).reshape(p, S_, C_).transpose(1, 0, 2).copy()
    return old, new, par, after


def pack(img, masks, k):
    """The ECG_UM_PACKED image: the cell of the i-th set bit of a valid mask at slot i."""
    out = np.full_like(img, FILL)
    for s, m in enumerate(masks):
        if read(int(m), k) > 0:
            for i, j in enumerate(j for j in range(k) if m >> j & 1):
                out[s, i] = img[s, j]
    return out


@pytest.mark.parametrize("mode", ["strided", "packed", "same", "table", "affine"])
@pytest.mark.parametrize("k,p,C_,htype", [(4, 2, 4096, 2), (8, 8, 4099, 3)])
def test_update_then_checksums(ctx, ecglib, oracle, k, p, C_, htype, mode):
    """The composites: the parity of the updated stripes is the oracle's encode of the merged image
    and the others are untouched; the checksums are those of the new parity in the selected
    stripes' slots; result is what a plain ecg_update_masks leaves for the same masks."""
    S_, cs = 7, 2048
    masks = batches(k, S_, seed=p)[0]
    old, new, par, after = update_case(oracle, k, p, C_, S_, masks, 17 * k + p + C_)
    if mode == "same":
        new, after = old, par
    ref = reference(oracle, ("upd", k, p, C_, mode == "same"), htype, cs, 1, after)
    nch, cl = ref.shape[2], CL[htype]
    off, pc, ps = scattered(S_, p, C_, gap=48 if C_ % 16 == 0 else 13) if mode == "table" else client(S_, p, C_, 512)
    css, ccs, nslots = nch, S_ * nch, p * S_ * nch
    rig = Rig(ctx, k, par, off, nslots, cl)
    flags = ecglib.UM_PACKED if mode == "packed" else 0
    oimg, nimg = (pack(old, masks, k), pack(new, masks, k)) if mode == "packed" else (old, new)
    dold, dnew = ctx.to_device(oimg), ctx.to_device(nimg)
    plain, plain_res = ctx.alloc(rig.img.size), ctx.alloc(32)
    try:
        rig.load(masks)
        if mode in ("table", "affine"):
            if mode == "table":                                         # the data cells in an order of their own
                order = np.random.default_rng(3).permutation(S_ * k).reshape(S_, k)
                oimg = oimg.reshape(S_ * k, C_)[np.argsort(order.reshape(-1))].copy()
                nimg = nimg.reshape(S_ * k, C_)[np.argsort(order.reshape(-1))].copy()
                dold.upload(oimg)
                dnew.upload(nimg)
            else:
                order = np.arange(S_ * k).reshape(S_, k)
            data = [[dold.ptr + int(order[s, j]) * C_ for j in range(k)] +
                    [dnew.ptr + int(order[s, j]) * C_ for j in range(k)] for s in range(S_)]
            before = ctx.stats()
            ctx.update_masks_ptrs_csum(k, p, C_, S_, rig.table(data), rig.masks.ptr, rig.result.ptr, htype, cs, 1,
                                       rig.cptr, css, ccs)
            launches = ctx.stats()["launches"] - before["launches"]
            name = ecglib.last_kernel()
            assert ("updated_ptr_kernel" if mode == "table" else "updated_kernel") in name, name
            assert launches == 2, launches
        else:
            ctx.update_masks_csum(k, p, C_, S_, dold.ptr, dnew.ptr, k * C_, rig.addr(0, 0), pc, ps, rig.masks.ptr,
                                  rig.result.ptr, htype, cs, 1, rig.cptr, css, ccs, flags)
            assert "updated_kernel" in ecglib.last_kernel(), ecglib.last_kernel()
        assert ("bytes" in ecglib.last_kernel()) == (C_ % 16 != 0)
        ctx.sync()
        # the parity arena: updated stripes re-encoded, everything else as it was
        want = rig.img.copy()
        for s in range(S_):
            for r in range(p):
                rig.cell(want, s, r)[:] = after[s, r]
        same(rig.buf.download(), want)
        assert rig.words64() == update_words(masks, k)
        same(rig.csums.download(), rig.sums_image(expect_sums(ref, masks, k, css, ccs, nslots)))
        assert np.array_equal(dold.download(), oimg.reshape(-1)) and np.array_equal(dnew.download(), nimg.reshape(-1))
        assert np.array_equal(rig.masks.download().view(np.uint32), rig.words)
        # result: a plain ecg_update_masks on a copy of the old parity
        if mode != "table":
            plain.upload(rig.img)
            ctx.update_masks(k, p, C_, S_, dold.ptr, dnew.ptr, k * C_, plain.ptr + rig.base, pc, ps, rig.masks.ptr,
                             plain_res.ptr, flags)
            ctx.sync()
            assert [int(v) for v in plain_res.download().view(np.uint64)] == rig.words64()
            same(plain.download(), want)
    finally:
        rig.free()
        for b in (dold, dnew, plain, plain_res):
            b.free()


def test_csum_updated_counts_what_update_masks_counts(ctx, ecglib, oracle):
    """Words 0, 1 and 3 of ecg_csum_updated are ecg_update_masks's for the same masks; word 2 is p
    times word 0."""
    k, p, C_, S_ = 4, 2, 4096, 7
    masks = batches(k, S_)[0]
    cells = random_cells(S_, p, C_)
    off, pc, ps = client(S_, p, C_)
    rig = Rig(ctx, k, cells, off, p * S_ * 2, 4)
    data, res = ctx.alloc(S_ * k * C_), ctx.alloc(32)
    try:
        _, mine, _ = rig.run(ecglib, masks, 2, 2048, 1, (pc, ps), 2, S_ * 2)
        data.fill(0)
        ctx.update_masks(k, p, C_, S_, data.ptr, data.ptr, k * C_, rig.addr(0, 0), pc, ps, rig.masks.ptr, res.ptr)
        ctx.sync()
        theirs = [int(v) for v in res.download().view(np.uint64)]
        assert (mine[0], mine[1], mine[3]) == (theirs[0], theirs[1], theirs[3]) and mine[2] == p * mine[0]
    finally:
        rig.free()
        data.free()
        res.free()


# ------------------------------------------------------------------- 5. empty
@pytest.mark.parametrize("S_,C_", [(0, 4096), (5, 0)])
def test_nothing_to_do(ctx, ecglib, S_, C_):
    """nstripes == 0 or cell_bytes == 0: result = {0, UINT64_MAX, 0, 0} and nothing else touched, no
    launch -- all four calls."""
    k, p = 4, 2
    masks, result, csums = ctx.alloc(64), ctx.alloc(32), ctx.alloc(256)
    tab = (C.c_void_p * max(1, S_ * (2 * k + p)))(*([0x1000] * max(1, S_ * (2 * k + p))))
    calls = [
        lambda: ctx.csum_updated(2, 2048, 1, k, p, C_, S_, csums.ptr, 4096, 4096, masks.ptr, csums.ptr, 0, 0, result.ptr),
        lambda: ctx.csum_updated_ptrs(2, 2048, 1, k, p, C_, S_, tab, masks.ptr, csums.ptr, 0, 0, result.ptr),
        lambda: ctx.update_masks_csum(k, p, C_, S_, csums.ptr, csums.ptr, 0, csums.ptr, 0, 0, masks.ptr, result.ptr, 2,
                                      2048, 1, csums.ptr, 0, 0),
        lambda: ctx.update_masks_ptrs_csum(k, p, C_, S_, tab, masks.ptr, result.ptr, 2, 2048, 1, csums.ptr, 0, 0),
    ]
    try:
        for call in calls:
            masks.fill(0x11)
            csums.fill(PRE)
            result.fill(0x77)
            ctx.sync()
            before = ctx.stats()["launches"]
            call()
            ctx.sync()
            assert ctx.stats()["launches"] == before
            assert [int(v) for v in result.download().view(np.uint64)] == [0, U64MAX, 0, 0]
            assert (csums.download() == PRE).all() and (masks.download() == 0x11).all()
    finally:
        for b in (masks, result, csums):
            b.free()
