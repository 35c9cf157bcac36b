"""ecg_csum_masked and ecg_recover_masks_csum on the GPU: the checksums of the cells each stripe's
mask word selects, in their slots of a [S][k+p][nch] array.  The expected checksums of a whole
image come from one oracle.csum_extents call over all S*(k+p) cells; a numpy model of the
selection rule picks the slots.  Every comparison is exact and covers whole allocations: the
checksum array is pre-filled with 0xEE between 0xA5 guards, so a write to a slot that is not
selected or outside the array shows; the stripes image (between 0xA5 guards and followed by
0xA5 slack of 24 cells) and the masks are read only and are compared as well."""
from itertools import combinations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U64MAX = (1 << 64) - 1
GUARD = 256                 # keeps image and checksums aligned inside their (256-byte aligned) allocations
FILL, PRE, ERASED = 0xA5, 0xEE, 0x5A
SLACK = 24                  # cells
CL = {1: 2, 2: 4, 3: 8, 7: 4}
TYPES = [1, 2, 3, 7]

_CW, _SUMS = {}, {}


def bits(cells):
    return sum(1 << int(c) for c in cells)


def cells_of(m):
    return [c for c in range(32) if m >> c & 1]


def valid(m, k, p):
    return m != 0 and m >> (k + p) == 0 and bin(m).count("1") <= p


def sel(m, k, p, which):
    """The selection rule, from the issue."""
    if not valid(m, k, p):
        return 0
    surv = [c for c in range(k + p) if not m >> c & 1][:k]
    return (m if which & 1 else 0) | (bits(surv) if which & 2 else 0)


def words(masks, k, p, which):
    """The four result words, from the issue."""
    ok = [s for s, m in enumerate(masks) if valid(m, k, p)]
    bad = [s for s, m in enumerate(masks) if m != 0 and not valid(m, k, p)]
    return [len(ok), min(bad) if bad else U64MAX, sum(bin(sel(masks[s], k, p, which)).count("1") for s in ok),
            len(bad)]


def all_sets(k, p):
    return [bits(cs) for e in range(1, p + 1) for cs in combinations(range(k + p), e)]


def random_cells(k, p, C_, S_):
    key = ("rnd", k, p, C_, S_)
    if key not in _CW:
        a = np.random.default_rng(7 * k + p + S_ + C_).integers(0, 256, (S_, k + p, C_), dtype=np.uint8)
        a.setflags(write=False)
        _CW[key] = a
    return _CW[key]


def codewords(oracle, k, p, C_, S_):
    """[S][k+p][C] codewords of the oracle, computed once per shape and never modified."""
    key = ("cw", k, p, C_, S_)
    if key not in _CW:
        data = np.random.default_rng(k * 1000003 + p * 101 + C_ + S_).integers(0, 256, (S_, k, C_), dtype=np.uint8)
        par = oracle.encode_batch(k, p, C_, S_, data.reshape(-1)).reshape(p, S_, C_)
        cw = np.concatenate([data, par.transpose(1, 0, 2)], axis=1)
        cw.setflags(write=False)
        _CW[key] = cw
    return _CW[key]


def reference(oracle, key, htype, chunksize, rec, cells):
    """Checksum bytes [S][k+p][nch][cl] of every cell of `cells` ([S][k+p][C]): one oracle call,
    kept under `key` (which names the cells) and never modified."""
    key = (key, htype, chunksize, rec)
    if key not in _SUMS:
        S_, n, C_ = cells.shape
        v = oracle.csum_extents(htype, chunksize, rec, 0, C_ // rec, cells.reshape(-1), C_, S_ * n)
        b = np.ascontiguousarray(v).view(np.uint8).reshape(S_, n, v.shape[1], CL[htype]).copy()
        b.setflags(write=False)
        _SUMS[key] = b
    return _SUMS[key]


def expect_array(ref, masks, k, p, which, start=None):
    """The [S][k+p][nch][cl] array after a call: `start` (default 0xEE everywhere) with the slots of
    the selected cells taken from ref."""
    out = np.full(ref.shape, PRE, dtype=np.uint8) if start is None else start.copy()
    for s, m in enumerate(masks):
        for c in cells_of(sel(int(m), k, p, which)):
            out[s, c] = ref[s, c]
    return out


class Rig:
    """S stripes [S][k+p][C] on the host (self.img: guards, image, slack) and on the device, the
    mask words, the result and one checksum array between guards.  skew: byte offset of the
    image from its 16-byte aligned place; cskew: the same for the checksum array."""

    def __init__(self, ctx, k, p, C_, cells, nch, cl, skew=0, cskew=0):
        self.ctx, self.k, self.p, self.C, self.S = ctx, k, p, C_, cells.shape[0]
        self.base, self.stride = GUARD + skew, (k + p) * C_
        self.img = np.full(self.base + self.S * self.stride + SLACK * C_ + GUARD, FILL, dtype=np.uint8)
        self.view(self.img)[:] = cells
        self.buf = ctx.alloc(self.img.size)
        self.masks, self.result = ctx.alloc(4 * self.S), ctx.alloc(32)
        self.shape = (self.S, k + p, nch, cl)
        self.cbase, self.cbytes = GUARD + cskew, self.S * (k + p) * nch * cl
        self.csums = self.sums_buffer()
        self.ptr, self.cptr = self.buf.ptr + self.base, self.csums.ptr + self.cbase
        self.bufs = [self.buf, self.masks, self.result, self.csums]

    def sums_buffer(self):
        b = self.ctx.alloc(self.cbase + self.cbytes + GUARD)
        self.bufs = getattr(self, "bufs", []) + [b]
        return b

    def view(self, img):
        return img[self.base:self.base + self.S * self.stride].reshape(self.S, self.k + self.p, self.C)

    def sums_image(self, arr=None):
        """The whole checksum allocation: guards around arr (default: the 0xEE pre-fill)."""
        a = np.full(self.cbase + self.cbytes + GUARD, FILL, dtype=np.uint8)
        a[self.cbase:self.cbase + self.cbytes] = PRE if arr is None else arr.reshape(-1)
        return a

    def erase(self, masks):
        v = self.view(self.img)
        for s, m in enumerate(masks):
            for c in cells_of(int(m)):
                if c < self.k + self.p:
                    v[s, c] = ERASED

    def load(self, masks):
        self.words = np.array(masks, dtype=np.uint32)
        self.buf.upload(self.img)
        self.masks.upload(self.words.view(np.uint8))
        self.csums.upload(self.sums_image())
        self.result.fill(0xEE)

    def run(self, ecglib, masks, htype, chunksize, rec, which, flags=0):
        """Upload everything, one call, one sync.  -> (checksum allocation, result words, kernel);
        the image and the masks are checked to be unchanged."""
        self.load(masks)
        self.ctx.csum_masked(htype, chunksize, rec, self.k, self.p, self.C, self.S, self.ptr, self.stride,
                             self.masks.ptr, which, self.cptr, self.result.ptr, flags)
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


def same(got, want):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8] - GUARD, bad.size)


# ------------------------------------------------------------ 1. every erasure set
@pytest.mark.parametrize("which", [1, 2, 3])
@pytest.mark.parametrize("k,p,htype", [(2, 1, 2), (4, 2, 1), (4, 2, 2), (4, 2, 3), (4, 2, 7), (8, 3, 2), (16, 3, 2)])
def test_every_erasure_set(ctx, ecglib, oracle, k, p, htype, which):
    """Stripe i carries set i; then mask 0, p+1 bits and bit k+p.  Two chunks of 32 bytes."""
    C_, cs = 64, 32
    masks = all_sets(k, p) + [0, bits(range(p + 1)), 1 | 1 << (k + p)]
    cells = random_cells(k, p, C_, len(masks))
    ref = reference(oracle, ("rnd", k, p, C_, len(masks)), htype, cs, 1, cells)
    assert ref.shape[2] == 2
    rig = Rig(ctx, k, p, C_, cells, 2, CL[htype])
    try:
        got, res, name = rig.run(ecglib, masks, htype, cs, 1, which)
        assert "masked_kernel" in name and "bytes" not in name, name
        assert res == words(masks, k, p, which)
        same(got, rig.sums_image(expect_array(ref, masks, k, p, which)))
        if which == 1:                          # word for word what recover_masks leaves
            ctx.recover_masks(k, p, C_, rig.S, rig.ptr, rig.stride, rig.masks.ptr, rig.result.ptr)
            ctx.sync()
            assert rig.words64() == res
    finally:
        rig.free()


# --------------------------------------------------------------------- 2. geometry
def seeded_masks(k, p, S_):
    """S masks from a fixed seed in which every cell index and every e <= p occurs."""
    rng = np.random.default_rng(97 * k + p)
    order = rng.permutation(k + p)
    masks, at = [], 0
    for s in range(S_):
        e = s % p + 1
        masks.append(bits(order[(at + i) % (k + p)] for i in range(e)))
        at += e
    assert {c for m in masks for c in cells_of(m)} == set(range(k + p))
    return masks


GEOMETRY = [
    # C, chunksize, rec_size, image skew, the byte-granular kernel
    (8192 + 48, 4096, 1, 0, False),             # ragged last chunk of 48 bytes
    (4099, 4096, 1, 0, True),                   # a 3-byte chunk: the tail-only path
    (32768 + 16, 32768, 1, 0, False),           # several Horner steps per lane
    (300, 100, 3, 0, True),                     # record chunk of 99 bytes: chunk bases off 16-byte boundaries
    (4800, 100, 3, 0, True),                    # the same inside an image whose cells all start aligned
    (8192 + 48, 4096, 1, 1, True),
    (8192 + 48, 4096, 1, 3, True),
]


@pytest.mark.parametrize("htype", TYPES)
@pytest.mark.parametrize("C_,cs,rec,skew,bytewise", GEOMETRY)
def test_geometry(ctx, ecglib, oracle, C_, cs, rec, skew, bytewise, htype):
    k, p, S_ = 8, 2, 13
    masks = seeded_masks(k, p, S_)
    masks[5] = 0                                # a clean stripe among them
    cells = random_cells(k, p, C_, S_)
    ref = reference(oracle, ("rnd", k, p, C_, S_), htype, cs, rec, cells)
    nch = ref.shape[2]
    assert nch == -(-C_ // (cs // rec * rec))
    rig = Rig(ctx, k, p, C_, cells, nch, CL[htype], skew=skew)
    try:
        for which in (3, 1):
            got, res, name = rig.run(ecglib, masks, htype, cs, rec, which)
            assert name.startswith("ecg_adler_masked_kernel" if htype == 7 else "ecg_crc_masked_kernel"), name
            assert ("bytes" in name) == bytewise, name      # which of the two load paths ran
            assert res == words(masks, k, p, which)
            same(got, rig.sums_image(expect_array(ref, masks, k, p, which)))
    finally:
        rig.free()


@pytest.mark.parametrize("htype", TYPES)
def test_checksum_array_at_any_byte(ctx, ecglib, oracle, htype):
    """csums off its natural alignment: the slots are written bytewise, neighbours intact."""
    k, p, S_, C_, cs = 8, 2, 13, 300, 100
    masks = seeded_masks(k, p, S_)
    cells = random_cells(k, p, C_, S_)
    ref = reference(oracle, ("rnd", k, p, C_, S_), htype, cs, 1, cells)
    for cskew in (1, 2):
        rig = Rig(ctx, k, p, C_, cells, 3, CL[htype], cskew=cskew)
        try:
            got, res, _ = rig.run(ecglib, masks, htype, cs, 1, 1)
            assert res == words(masks, k, p, 1)
            same(got, rig.sums_image(expect_array(ref, masks, k, p, 1)))
        finally:
            rig.free()


# ------------------------------------------------------- 3. any mask value is safe
@pytest.mark.parametrize("k,p", [(4, 2), (16, 3)])
def test_any_mask_value_is_safe(ctx, ecglib, oracle, k, p):
    """200 stripes; a third of the masks are 32 random bits, a third random bits below k+p (some
    of them sets), the rest sets; then the edge values.  With and without ECG_RM_SPARSE, on the
    default grid and on two workgroups (the grid strides): the same array, nothing else written."""
    rng = np.random.default_rng(20 + k)
    n, C_, cs, htype = k + p, 256, 128, 2
    sets = all_sets(k, p)
    masks = [int(rng.integers(0, 1 << 32)) for _ in range(60)]
    masks += [int(rng.integers(0, 1 << n)) & int(rng.integers(0, 1 << n)) for _ in range(60)]
    masks += [sets[int(i)] for i in rng.integers(0, len(sets), 60)]
    masks += [0xFFFFFFFF, 0, 1 << 31, 1 << n, 1 << (n + 1), 1 << 19, 1 << 20, (1 << n) - 1, 1 | 1 << 31,
              bits(range(p + 1)), bits(range(k, n)), bits(range(k - 1, n)), 1 << (n - 1), 1, 0x80000001 >> 1]
    masks += [0] * (200 - len(masks))
    cells = random_cells(k, p, C_, 200)
    ref = reference(oracle, ("rnd", k, p, C_, 200), htype, cs, 1, cells)
    want_words = words(masks, k, p, 3)
    assert want_words[0] >= 60 and want_words[3] >= 60
    rig = Rig(ctx, k, p, C_, cells, 2, 4)
    try:
        want = rig.sums_image(expect_array(ref, masks, k, p, 3))
        for blocks in (0, 2):
            for flags in (0, ecglib.RM_SPARSE):
                L = ecglib.lib()
                assert L.ecg_set_csum_launch(ctx.h, blocks) == 0
                try:
                    got, res, _ = rig.run(ecglib, masks, htype, cs, 1, 3, flags)
                finally:
                    assert L.ecg_set_csum_launch(ctx.h, 0) == 0
                assert res == want_words, (blocks, flags)
                same(got, want)
    finally:
        rig.free()


# --------------------------------------- 4. the composite equals the homogeneous calls
@pytest.mark.parametrize("one_array", [False, True])
@pytest.mark.parametrize("htype", [2, 3])
@pytest.mark.parametrize("errs", [[0, 1], [3, 9], [8, 9], [5]])
def test_composite_equals_homogeneous_calls(ctx, ecglib, oracle, errs, htype, one_array):
    k, p, C_, S_, cs = 8, 2, 8192, 6, 4096
    n, nch, cl = k + p, 2, CL[htype]
    masks = [bits(errs)] * S_
    cw = codewords(oracle, k, p, C_, S_)
    rig = Rig(ctx, k, p, C_, cw, nch, cl)
    src = rig.csums if one_array else rig.sums_buffer()
    twin, hc, hs = ctx.alloc(rig.img.size), ctx.alloc(len(errs) * S_ * nch * cl), ctx.alloc(k * S_ * nch * cl)
    rig.bufs += [twin, hc, hs]
    try:
        clean = rig.img.copy()
        rig.erase(masks)
        # the homogeneous calls on a twin of the erased image
        twin.upload(rig.img)
        src_idx = ctx.recover_csum_all(k, p, C_, S_, twin.ptr + rig.base, rig.stride, errs, htype, cs, 1, hc.ptr,
                                       hs.ptr)
        ctx.sync()
        rows = hc.download().reshape(len(errs), S_, nch, cl)
        srows = hs.download().reshape(k, S_, nch, cl)
        same(twin.download(), clean)
        twin.upload(rig.img)
        ctx.recover_csum(k, p, C_, S_, twin.ptr + rig.base, rig.stride, errs, htype, cs, 1, hc.ptr)
        ctx.sync()
        assert np.array_equal(hc.download().reshape(rows.shape), rows)
        want_c = np.full(rig.shape, PRE, dtype=np.uint8)
        want_s = want_c if one_array else want_c.copy()
        for i, c in enumerate(errs):
            want_c[:, c] = rows[i]
        for i, c in enumerate(src_idx):
            want_s[:, c] = srows[i]
        # the composite
        rig.load(masks)
        src.upload(rig.sums_image())
        ctx.recover_masks_csum(k, p, C_, S_, rig.ptr, rig.stride, rig.masks.ptr, rig.result.ptr, htype, cs, 1,
                               rig.cptr, src.ptr + rig.cbase)
        ctx.sync()
        assert rig.words64() == [S_, U64MAX, len(errs) * S_, 0]
        same(rig.buf.download(), clean)
        same(rig.csums.download(), rig.sums_image(want_c))
        same(src.download(), rig.sums_image(want_s))
        assert np.array_equal(rig.masks.download().view(np.uint32), rig.words)
        # and without src_csums: the erased cells' slots only
        rig.load(masks)
        ctx.recover_masks_csum(k, p, C_, S_, rig.ptr, rig.stride, rig.masks.ptr, rig.result.ptr, htype, cs, 1,
                               rig.cptr)
        ctx.sync()
        only = np.full(rig.shape, PRE, dtype=np.uint8)
        for i, c in enumerate(errs):
            only[:, c] = rows[i]
        same(rig.csums.download(), rig.sums_image(only))
        same(rig.buf.download(), clean)
    finally:
        rig.free()


# ----------------------------------- 5. verified degraded read, one stream, one sync
def test_verified_degraded_read(ctx, ecglib, oracle):
    """Mixed erasure sets, the erased cells overwritten; one byte of a survivor flipped in two
    stripes.  The composite regenerates, and checksums what it read into src_csums, which starts
    as a device copy of the stored checksums so that the slots it leaves alone compare equal.
    Compared with the stored checksums on the device, exactly those two cells' chunks differ,
    and csum_mask ORs those cells into a second mask array."""
    k, p, C_, S_, cs, htype = 8, 2, 8192, 20, 4096, 2
    n, nch, cl = k + p, 2, 4
    cw = codewords(oracle, k, p, C_, S_)
    ref = reference(oracle, ("cw", k, p, C_, S_), htype, cs, 1, cw)
    masks = seeded_masks(k, p, S_)
    masks[4] = 0
    rig = Rig(ctx, k, p, C_, cw, nch, cl)
    src = rig.sums_buffer()
    stored, cmp_res, found = ctx.alloc(rig.cbytes), ctx.alloc(16), ctx.alloc(4 * S_)
    rig.bufs += [stored, cmp_res, found]
    try:
        rig.erase(masks)
        flips = []                              # (stripe, a survivor the recovery reads, chunk)
        for s, nth, at in ((2, 3, 5000), (11, 0, 17)):
            c = cells_of(sel(masks[s], k, p, 2))[nth]
            rig.view(rig.img)[s, c, at] ^= 0x10
            flips.append((s, c, at // cs))
        stored.upload(ref.reshape(-1))
        rig.load(masks)
        src.upload(rig.sums_image())
        sptr = src.ptr + rig.cbase
        ecglib._chk(ecglib.lib().ecg_memcpy(ctx.h, sptr, stored.ptr, rig.cbytes, 2, None), "D2D")
        found.fill(0)
        ctx.recover_masks_csum(k, p, C_, S_, rig.ptr, rig.stride, rig.masks.ptr, rig.result.ptr, htype, cs, 1,
                               rig.cptr, sptr)
        ctx.csum_compare(htype, sptr, stored.ptr, S_ * n * nch, cmp_res.ptr)
        ctx.csum_mask(htype, sptr, stored.ptr, S_, n, nch, n * nch, nch, 0, found.ptr)
        ctx.sync()
        assert rig.words64() == words(masks, k, p, 1)
        cnt, lo = (int(v) for v in cmp_res.download().view(np.uint64))
        assert cnt == 2 and lo == min((s * n + c) * nch + ch for s, c, ch in flips)
        got_s = src.download()
        same(got_s[:rig.cbase], rig.sums_image()[:rig.cbase])
        same(got_s[rig.cbase + rig.cbytes:], rig.sums_image()[rig.cbase + rig.cbytes:])
        got_s = got_s[rig.cbase:rig.cbase + rig.cbytes].reshape(rig.shape)
        differ = {(int(s), int(c), int(ch)) for s, c, ch in zip(*np.nonzero((got_s != ref).any(axis=3)))}
        assert differ == set(flips)
        want_found = [0] * S_
        for s, c, _ in flips:
            want_found[s] |= 1 << c
        assert [int(m) for m in found.download().view(np.uint32)] == want_found
        # csums: the erased cells' slots alone; what was regenerated from a flipped survivor is
        # wrong in the flipped chunk (every decode coefficient of an MDS code is non-zero)
        got_c = rig.csums.download()
        want_c = expect_array(ref, masks, k, p, 1)
        at_flip = np.zeros(rig.shape[:3], dtype=bool)
        for s, _, ch in flips:
            for e in cells_of(masks[s]):
                at_flip[s, e, ch] = True
        got_v = got_c[rig.cbase:rig.cbase + rig.cbytes].reshape(rig.shape)
        assert ((got_v != want_c).any(axis=3) == at_flip).all()
        got_v = got_v.copy()
        got_v[at_flip] = want_c[at_flip]
        same(rig.sums_image(got_v), rig.sums_image(want_c))
        same(got_c[:rig.cbase], rig.sums_image()[:rig.cbase])
        same(got_c[rig.cbase + rig.cbytes:], rig.sums_image()[rig.cbase + rig.cbytes:])
    finally:
        rig.free()


# ------------------------------------------------------ 6. scrub with confirmation
@pytest.mark.parametrize("k,p", [(2, 1), (8, 2)])
def test_scrub_with_confirmation(ctx, ecglib, oracle, k, p):
    """csum_extents -> memset -> csum_mask -> recover_masks -> csum_masked(ERASED) into `fresh` ->
    csum_compare(fresh, stored), one stream, one sync: the rewritten cells carry their stored
    checksums again (0 mismatches) and the image is clean."""
    C_, S_, htype = 4096, 20, 2
    n = k + p
    cw = codewords(oracle, k, p, C_, S_)
    rig = Rig(ctx, k, p, C_, cw, 1, 4)
    stored, cmp_res, res2 = ctx.alloc(rig.cbytes), ctx.alloc(16), ctx.alloc(32)
    rig.bufs += [stored, cmp_res, res2]
    try:
        clean = rig.img.copy()
        rig.buf.upload(clean)
        ctx.csum_extents(htype, 4096, 1, 0, C_, rig.ptr, C_, S_ * n, stored.ptr)
        ctx.sync()
        v = rig.view(rig.img)
        if p == 1:
            wrong = {s: [s % n] for s in range(0, S_, 2)}
        else:
            wrong = {0: [0, 1], 1: [k - 1, k], 2: [k, k + 1], 3: [5, 6], 7: [k + 1, 2], 8: [0, k + 1], 19: [2, 7]}
        for s, cs_ in wrong.items():
            for i, c in enumerate(cs_):
                v[s, c, (s * 131 + i * 977) % C_] ^= 0x40 >> i
        rig.buf.upload(rig.img)
        rig.csums.upload(rig.sums_image())
        rig.result.fill(0xEE)
        rig.masks.fill(0xEE)
        fresh = rig.cptr
        ctx.csum_extents(htype, 4096, 1, 0, C_, rig.ptr, C_, S_ * n, fresh)
        rig.masks.fill(0)
        ctx.csum_mask(htype, fresh, stored.ptr, S_, n, 1, n, 1, 0, rig.masks.ptr)
        ctx.recover_masks(k, p, C_, S_, rig.ptr, rig.stride, rig.masks.ptr, rig.result.ptr, ecglib.RM_SPARSE)
        ctx.csum_masked(htype, 4096, 1, k, p, C_, S_, rig.ptr, rig.stride, rig.masks.ptr, ecglib.CM_ERASED, fresh,
                        res2.ptr, ecglib.RM_SPARSE)
        ctx.csum_compare(htype, fresh, stored.ptr, S_ * n, cmp_res.ptr)
        ctx.sync()
        assert [int(m) for m in rig.masks.download().view(np.uint32)] == \
            [bits(wrong.get(s, [])) for s in range(S_)]
        want = [len(wrong), U64MAX, sum(len(c) for c in wrong.values()), 0]
        assert rig.words64() == want
        assert [int(x) for x in res2.download().view(np.uint64)] == want
        assert [int(x) for x in cmp_res.download().view(np.uint64)] == [0, U64MAX]
        same(rig.buf.download(), clean)
        same(rig.csums.download(), rig.sums_image(stored.download()))
    finally:
        rig.free()


# -------------------------------------------------------------------- 7. telemetry
def test_launches_advance_and_csum_chunks_does_not(ctx, ecglib, oracle):
    k, p, C_, S_ = 4, 2, 4096, 6
    rig = Rig(ctx, k, p, C_, codewords(oracle, k, p, C_, S_), 1, 4)
    try:
        rig.run(ecglib, [1] * S_, 2, 4096, 1, 3)            # builds and uploads the CRC tables
        before = ctx.stats()
        rig.run(ecglib, [1] * S_, 2, 4096, 1, 3)
        mid = ctx.stats()
        assert mid["launches"] == before["launches"] + 1
        assert mid["csum_chunks"] == before["csum_chunks"]  # the count lives on the device
        rig.load([3] * S_)                                  # (set table of recover_masks: first use)
        ctx.recover_masks_csum(k, p, C_, S_, rig.ptr, rig.stride, rig.masks.ptr, rig.result.ptr, 2, 4096, 1,
                               rig.cptr)
        ctx.sync()
        for src, nlaunch in ((None, 2), (rig.cptr, 2)):     # src_csums == csums: still one checksum launch
            a = ctx.stats()
            ctx.recover_masks_csum(k, p, C_, S_, rig.ptr, rig.stride, rig.masks.ptr, rig.result.ptr, 2, 4096, 1,
                                   rig.cptr, src)
            ctx.sync()
            b = ctx.stats()
            assert b["launches"] == a["launches"] + nlaunch
            assert b["csum_chunks"] == a["csum_chunks"]
        other = rig.sums_buffer()
        a = ctx.stats()
        ctx.recover_masks_csum(k, p, C_, S_, rig.ptr, rig.stride, rig.masks.ptr, rig.result.ptr, 2, 4096, 1,
                               rig.cptr, other.ptr + rig.cbase)
        ctx.sync()
        assert ctx.stats()["launches"] == a["launches"] + 3     # separate arrays: one more launch
        # an empty batch presets the result and launches nothing
        rig.result.fill(0xEE)
        a = ctx.stats()
        ctx.csum_masked(2, 4096, 1, k, p, C_, 0, rig.ptr, rig.stride, rig.masks.ptr, 3, rig.cptr, rig.result.ptr)
        ctx.csum_masked(2, 4096, 1, k, p, 0, S_, rig.ptr, rig.stride, rig.masks.ptr, 3, rig.cptr, rig.result.ptr)
        ctx.sync()
        assert rig.words64() == [0, U64MAX, 0, 0]
        assert ctx.stats()["launches"] == a["launches"]
    finally:
        rig.free()
