"""ecg_recover_masks and ecg_csum_mask on the GPU: recovery with one erasure set per stripe,
the sets given as mask words in device memory.  Stripes in the recovery layout [S][k+p][C]
from the CPU oracle (or random bytes, where the point is which survivors are read).  Every
comparison is exact and covers the whole allocation: the image lies between 0xA5 guard bytes
and is followed by 0xA5 slack of 24 cells, so a cell index the kernel failed to bound shows up
as changed bytes."""
from itertools import combinations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (4, 2), (8, 2), (16, 2), (8, 3), (16, 3), (5, 2)]
NSETS = {(2, 1): 3, (4, 2): 21, (8, 2): 55, (16, 2): 171, (8, 3): 231, (16, 3): 1159, (5, 2): 28}
U64MAX = (1 << 64) - 1
GUARD = 256                 # keeps the image 16-byte aligned inside its (256-byte aligned) allocation
FILL, ERASED = 0xA5, 0x5A
SLACK = 24                  # cells

_REF = {}


def codewords(oracle, k, p, C_, S_):
    """[S][k+p][C] codewords of the oracle, computed once per shape and never modified."""
    key = (k, p, C_, S_)
    if key not in _REF:
        data = np.random.default_rng(k * 1000003 + p * 101 + C_ + S_).integers(0, 256, (S_, k, C_), dtype=np.uint8)
        par = oracle.encode_batch(k, p, C_, S_, data.reshape(-1)).reshape(p, S_, C_)
        cw = np.concatenate([data, par.transpose(1, 0, 2)], axis=1)
        cw.setflags(write=False)
        _REF[key] = cw
    return _REF[key]


def bits(cells):
    return sum(1 << int(c) for c in cells)


def cells_of(m):
    return [c for c in range(32) if m >> c & 1]


def sets_by_index(ecglib, k, p):
    """masks[i] = the mask whose ecg_erasure_set_index is i."""
    out = {ecglib.erasure_set_index(k, p, bits(cs)): bits(cs)
           for e in range(1, p + 1) for cs in combinations(range(k + p), e)}
    assert sorted(out) == list(range(NSETS[k, p]))
    return [out[i] for i in range(len(out))]


def model(masks, k, p):
    """The validity rule, from the issue: -> (stripes rewritten, the four result words)."""
    ok, left = [], []
    for s, m in enumerate(int(m) for m in masks):
        if m == 0:
            continue
        (left if m >> (k + p) or bin(m).count("1") > p else ok).append(s)
    ncell = sum(bin(int(masks[s])).count("1") for s in ok)
    return ok, [len(ok), min(left) if left else U64MAX, ncell, len(left)]


def kernel_name(k, p):
    return f"ecg_recover_masks_kernel<{k if k in (2, 4, 8, 16) else 0}, {p}>"


class Rig:
    """S stripes [S][k+p][C] on the host (self.img: guards, image, slack) and on the device,
    the mask words and the result.  cells: [S][k+p][C] to start from.  skew: byte offset of the
    image from its 16-byte aligned place."""

    def __init__(self, ctx, k, p, C_, cells, skew=0):
        self.ctx, self.k, self.p, self.C, self.S = ctx, k, p, C_, cells.shape[0]
        self.base, self.stride = GUARD + skew, (k + p) * C_
        self.img = np.full(self.base + self.S * self.stride + SLACK * C_ + GUARD, FILL, dtype=np.uint8)
        self.view(self.img)[:] = cells
        self.buf = ctx.alloc(self.img.size)
        self.masks, self.result = ctx.alloc(4 * self.S), ctx.alloc(32)
        self.ptr = self.buf.ptr + self.base

    def view(self, img):
        return img[self.base:self.base + self.S * self.stride].reshape(self.S, self.k + self.p, self.C)

    def erase(self, masks):
        """Overwrite the cells the masks name (those that exist) with 0x5A."""
        v = self.view(self.img)
        for s, m in enumerate(masks):
            for c in cells_of(int(m)):
                if c < self.k + self.p:
                    v[s, c] = ERASED

    def run(self, ecglib, masks, flags=0):
        """Upload image and masks, one call, one sync.  -> (image, result words, kernel)."""
        words = np.array(masks, dtype=np.uint32)
        self.buf.upload(self.img)
        self.masks.upload(words.view(np.uint8))
        self.result.fill(0xEE)
        self.ctx.recover_masks(self.k, self.p, self.C, self.S, self.ptr, self.stride, self.masks.ptr,
                               self.result.ptr, flags)
        name = ecglib.last_kernel()
        self.ctx.sync()
        assert np.array_equal(self.masks.download().view(np.uint32), words)         # read only
        return self.buf.download(), [int(v) for v in self.result.download().view(np.uint64)], name

    def free(self):
        for b in (self.buf, self.masks, self.result):
            b.free()


def same(got, want, rig):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8] - rig.base, bad.size)


def check_every_set(ctx, ecglib, oracle, k, p, C_, kernel, skew=0):
    """Stripe i carries set i, its erased cells overwritten; then mask 0, p+1 bits, bit k+p."""
    sets = sets_by_index(ecglib, k, p)
    n = len(sets)
    masks = sets + [0, bits(range(p + 1)), 1 | 1 << (k + p)]
    rig = Rig(ctx, k, p, C_, codewords(oracle, k, p, C_, n + 3), skew=skew)
    try:
        want = rig.img.copy()
        rig.erase(masks)
        for s in (n + 1, n + 2):                # the unrecoverable stripes keep their 0x5A cells
            rig.view(want)[s] = rig.view(rig.img)[s]
        got, res, name = rig.run(ecglib, masks)
        assert name == kernel, name
        assert res == [n, n + 1, sum(bin(m).count("1") for m in sets), 2]
        same(got, want, rig)
    finally:
        rig.free()


# ------------------------------------------------------------ 1. every erasure set
@pytest.mark.parametrize("k,p", SHAPES)
def test_every_erasure_set_small_cell(ctx, ecglib, oracle, k, p):
    check_every_set(ctx, ecglib, oracle, k, p, 16, kernel_name(k, p))


@pytest.mark.parametrize("k,p", [kp for kp in SHAPES if NSETS[kp] <= 231])
def test_every_erasure_set_lane_masked_last_column(ctx, ecglib, oracle, k, p):
    check_every_set(ctx, ecglib, oracle, k, p, 8192 + 48, kernel_name(k, p))


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
    assert {bin(m).count("1") for m in masks} == set(range(1, p + 1))
    return masks


@pytest.mark.parametrize("k,p", SHAPES)
def test_more_columns_than_column_blocks(ctx, ecglib, oracle, k, p):
    C_, S_ = 128 * 1024, k + p + 3
    masks = seeded_masks(k, p, S_)
    rig = Rig(ctx, k, p, C_, codewords(oracle, k, p, C_, S_))
    try:
        want = rig.img.copy()
        rig.erase(masks)
        ctx.set_launch(3, 0, 0)                 # 32 columns on 3 column blocks: the column loop strides
        try:
            got, res, name = rig.run(ecglib, masks, ecglib.RM_SPARSE)
        finally:
            ctx.set_launch(0, 0, 0)
        assert name == kernel_name(k, p)
        assert res == [S_, U64MAX, sum(bin(m).count("1") for m in masks), 0]
        same(got, want, rig)
        for flags in (0, ecglib.RM_SPARSE):     # and the default grids
            got, res2, _ = rig.run(ecglib, masks, flags)
            assert res2 == res
            same(got, want, rig)
    finally:
        rig.free()


# ------------------------------------- 2. the bytes of ecg_recover, on non-codewords
def random_cells(k, p, C_, S_):
    return np.random.default_rng(7 * k + p + S_).integers(0, 256, (S_, k + p, C_), dtype=np.uint8)


def recover_per_stripe(ctx, rig, masks):
    """The twin: one ecg_recover(nstripes = 1) per valid stripe on a copy of rig.img."""
    k, p = rig.k, rig.p
    twin = ctx.alloc(rig.img.size)
    try:
        twin.upload(rig.img)
        for s in model(masks, k, p)[0]:
            ctx.recover(k, p, rig.C, 1, twin.ptr + rig.base + s * rig.stride, rig.stride, cells_of(int(masks[s])))
        ctx.sync()
        return twin.download()
    finally:
        twin.free()


@pytest.mark.parametrize("k,p", [(4, 2), (8, 3), (16, 2)])
def test_identical_to_recover_on_non_codewords(ctx, ecglib, k, p):
    """Random, inconsistent stripes: the bytes written depend on which survivors are read and in
    which order the rows are written, so this pins ecg_recov_rows's choice for every set."""
    masks = sets_by_index(ecglib, k, p)
    rig = Rig(ctx, k, p, 4096, random_cells(k, p, 4096, len(masks)))
    try:
        want = recover_per_stripe(ctx, rig, masks)
        assert not np.array_equal(want, rig.img)                        # recover did write
        got, res, name = rig.run(ecglib, masks)
        assert name == kernel_name(k, p)
        assert res == model(masks, k, p)[1]
        same(got, want, rig)
    finally:
        rig.free()


# ------------------------------------------------------- 3. any mask value is safe
@pytest.mark.parametrize("k,p", [(4, 2), (16, 3)])
def test_any_mask_value_is_safe(ctx, ecglib, k, p):
    """200 stripes of random bytes, so that any cell written would change.  A third of the masks
    are 32 random bits, a third random bits below k+p (some of them sets), the rest sets; then
    the edge values.  Every grid, kernel and flag gives the image of the per-stripe recover."""
    rng = np.random.default_rng(20 + k)
    n = k + p
    sets = sets_by_index(ecglib, k, p)
    masks = [int(rng.integers(0, 1 << 32)) for _ in range(60)]
    masks += [int(rng.integers(0, 1 << n)) & int(rng.integers(0, 1 << n)) for _ in range(60)]
    masks += [sets[int(i)] for i in rng.integers(0, len(sets), 60)]
    masks += [0xFFFFFFFF, 0, 1 << 31, 1 << n, 1 << (n + 1), 1 << 19, 1 << 20, (1 << n) - 1, 1 | 1 << 31,
              bits(range(p + 1)), bits(range(k, n)), bits(range(k - 1, n)), 1 << (n - 1), 1, 0x80000001 >> 1]
    masks += [0] * (200 - len(masks))
    rig = Rig(ctx, k, p, 4096, random_cells(k, p, 4096, 200))
    try:
        ok, words = model(masks, k, p)
        assert len(ok) >= 60 and words[3] >= 60
        want = recover_per_stripe(ctx, rig, masks)
        untouched = [s for s in range(200) if s not in ok]
        assert np.array_equal(rig.view(want)[untouched], rig.view(rig.img)[untouched])
        for grid in ((0, 0), (1, 2)):
            for variant in (0, 2):
                for flags in (0, ecglib.RM_SPARSE):
                    ctx.set_launch(grid[0], grid[1], variant)
                    try:
                        got, res, name = rig.run(ecglib, masks, flags)
                    finally:
                        ctx.set_launch(0, 0, 0)
                    assert name == ("ecg_recover_masks_byte_kernel" if variant == 2 else kernel_name(k, p))
                    assert res == words, (grid, variant, flags)
                    same(got, want, rig)
    finally:
        rig.free()


# ------------------------------------------------------------------ 4. byte kernel
@pytest.mark.parametrize("skew,C_", [(1, 1), (3, 1), (1, 4099), (3, 4099), (0, 4099), (1, 4096)])
@pytest.mark.parametrize("k,p", [(4, 2), (8, 3), (5, 2), (2, 1)])
def test_byte_kernel(ctx, ecglib, oracle, k, p, skew, C_):
    check_every_set(ctx, ecglib, oracle, k, p, C_, "ecg_recover_masks_byte_kernel", skew=skew)


@pytest.mark.parametrize("k,p", [(4, 2), (16, 2), (5, 2)])
def test_byte_kernel_forced_on_aligned_operands(ctx, ecglib, oracle, k, p):
    ctx.set_launch(0, 0, 2)
    try:
        check_every_set(ctx, ecglib, oracle, k, p, 8192 + 48, "ecg_recover_masks_byte_kernel")
    finally:
        ctx.set_launch(0, 0, 0)


# -------------------------------------------------------------------- 5. csum_mask
@pytest.mark.parametrize("nch", [1, 3])
@pytest.mark.parametrize("layout", ["cell_major", "stripe_major"])
@pytest.mark.parametrize("htype,cl", [(1, 2), (2, 4), (3, 8)])
def test_csum_mask(ctx, ecglib, htype, cl, layout, nch):
    """Checksums are opaque to the comparison: random bytes, one checksum changed at chosen
    (stripe, cell, chunk) positions.  cell_major: the separate data [k][S][nch] and parity
    [p][S][nch] arrays of encode_csum_all, two calls, the second with first_cell = k;
    stripe_major: [S][k+p][nch] of csum_extents over a recovery-layout image, one call."""
    k, p, S_ = 8, 2, 70
    n = k + p
    rng = np.random.default_rng(htype * 10 + nch)
    want = rng.integers(0, 256, (S_, n, nch, cl), dtype=np.uint8)       # [s][cell][chunk]
    got = want.copy()
    hits = [(0, 0, 0), (0, n - 1, nch - 1), (3, 2, nch // 2), (3, k, 0), (3, k - 1, nch - 1), (64, 5, 0),
            (69, n - 1, 0), (69, 0, nch - 1), (31, k + 1, nch - 1)]
    for i, (s, c, ch) in enumerate(hits):
        got[s, c, ch, i % cl] ^= 1 << (i % 8)                             # one bit of one byte
    preset = rng.integers(0, 1 << 32, S_, dtype=np.uint32)
    preset[::2] = 0
    expect = preset.copy()
    for s, c, _ in hits:
        expect[s] |= np.uint32(1 << c)
    bufs = [ctx.alloc(got.size) for _ in range(4)] + [ctx.alloc(4 * S_)]
    gd, wd, gp, wp, masks = bufs
    try:
        masks.upload(preset.view(np.uint8))
        if layout == "cell_major":
            for dev, a in ((gd, got[:, :k]), (wd, want[:, :k]), (gp, got[:, k:]), (wp, want[:, k:])):
                dev.upload(np.ascontiguousarray(a.transpose(1, 0, 2, 3)).reshape(-1))
            ctx.csum_mask(htype, gd.ptr, wd.ptr, S_, k, nch, nch, S_ * nch, 0, masks.ptr)
            ctx.csum_mask(htype, gp.ptr, wp.ptr, S_, p, nch, nch, S_ * nch, k, masks.ptr)
        else:
            gd.upload(got.reshape(-1))
            wd.upload(want.reshape(-1))
            ctx.csum_mask(htype, gd.ptr, wd.ptr, S_, n, nch, n * nch, nch, 0, masks.ptr)
        assert ecglib.last_kernel() == "ecg_csum_mask_kernel"
        ctx.sync()
        assert np.array_equal(masks.download().view(np.uint32), expect)
    finally:
        for b in bufs:
            b.free()


# ------------------------------------------ 6. the scrub verify / repair cannot do
@pytest.mark.parametrize("k,p", [(2, 1), (8, 2)])
def test_checksum_driven_scrub(ctx, ecglib, oracle, k, p):
    """Stored checksums of the clean image; then one wrong cell per stripe with p = 1, where
    ecg_verify attributes nothing, and with (8, 2) two wrong cells in some stripes (data+data,
    data+parity, parity+parity), where it may miscorrect.  csum_extents -> memset -> csum_mask ->
    recover_masks on one stream with one sync."""
    C_, S_, htype = 4096, 20, ecglib.HASH_CRC32
    n = k + p
    rig = Rig(ctx, k, p, C_, codewords(oracle, k, p, C_, S_))
    stored, fresh = ctx.alloc(4 * S_ * n), ctx.alloc(4 * S_ * n)
    try:
        clean = rig.img.copy()
        rig.buf.upload(clean)
        ctx.csum_extents(htype, 4096, 1, 0, C_, rig.ptr, C_, S_ * n, stored.ptr)
        ctx.sync()
        v = rig.view(rig.img)
        if p == 1:
            wrong = {s: [s % n] for s in range(0, S_, 2)}
        else:
            wrong = {0: [0, 1], 1: [k - 1, k], 2: [k, k + 1], 3: [5], 7: [k + 1], 8: [0, k + 1], 19: [2, 7]}
        for s, cs in wrong.items():
            for i, c in enumerate(cs):
                v[s, c, (s * 131 + i * 977) % C_] ^= 0x40 >> i
        rig.buf.upload(rig.img)
        rig.result.fill(0xEE)
        rig.masks.fill(0xEE)
        ctx.csum_extents(htype, 4096, 1, 0, C_, rig.ptr, C_, S_ * n, fresh.ptr)
        rig.masks.fill(0)
        ctx.csum_mask(htype, fresh.ptr, stored.ptr, S_, n, 1, n, 1, 0, rig.masks.ptr)
        ctx.recover_masks(k, p, C_, S_, rig.ptr, rig.stride, rig.masks.ptr, rig.result.ptr, ecglib.RM_SPARSE)
        ctx.sync()
        assert [int(m) for m in rig.masks.download().view(np.uint32)] == \
            [bits(wrong.get(s, [])) for s in range(S_)]
        res = [int(x) for x in rig.result.download().view(np.uint64)]
        assert res == [len(wrong), U64MAX, sum(len(cs) for cs in wrong.values()), 0]
        same(rig.buf.download(), clean, rig)
    finally:
        for b in (stored, fresh):
            b.free()
        rig.free()


# ------------------------------------------------------------------- 7. arguments
def test_argument_errors(ctx, ecglib):
    L = ecglib.lib()
    k, p, C_, S_ = 4, 2, 4096, 9
    rig = Rig(ctx, k, p, C_, random_cells(k, p, C_, S_))
    try:
        rig.buf.upload(rig.img)
        rig.masks.upload(np.full(S_, 1, dtype=np.uint32).view(np.uint8))

        def call(k_=k, p_=p, C__=C_, S__=S_, masks=rig.masks.ptr, result=rig.result.ptr, flags=0):
            return L.ecg_recover_masks(ctx.h, k_, p_, C__, S__, rig.ptr, rig.stride, masks, result, flags, None)

        for kk, pp in ((17, 2), (0, 2), (4, 4), (4, 0)):
            assert call(k_=kk, p_=pp) == -ecglib.DER_INVAL, (kk, pp)
            assert b"k <= 16" in L.ecg_strerror()
        assert call(result=rig.result.ptr + 4) == -ecglib.DER_INVAL
        assert call(masks=rig.masks.ptr + 2) == -ecglib.DER_INVAL
        assert call(masks=None) == -ecglib.DER_INVAL
        assert call(flags=4) == -ecglib.DER_INVAL
        for inside in (rig.ptr, rig.ptr + 64, rig.ptr + S_ * rig.stride - 4, rig.ptr - 4 * S_ + 4):
            assert call(masks=inside) == -ecglib.DER_INVAL              # masks inside the stripes
            assert b"overlaps" in L.ecg_strerror()
        # an empty batch and empty cells preset the result and touch nothing else
        for kw in ({"S__": 0, "masks": None}, {"C__": 0}):
            rig.result.fill(0xEE)
            assert call(**kw) == 0
            ctx.sync()
            assert [int(x) for x in rig.result.download().view(np.uint64)] == [0, U64MAX, 0, 0]
        assert np.array_equal(rig.buf.download(), rig.img)              # none of the calls above wrote a cell
    finally:
        rig.free()


def test_counts_one_launch_and_no_recover_stripes(ctx, ecglib, oracle):
    rig = Rig(ctx, 4, 2, 4096, codewords(oracle, 4, 2, 4096, 6))
    try:
        rig.run(ecglib, [1] * 6)                # builds and uploads the set table
        before = ctx.stats()
        rig.run(ecglib, [1] * 6)
        after = ctx.stats()
        assert after["launches"] == before["launches"] + 1
        assert after["recover_stripes"] == before["recover_stripes"]    # the count lives on the device
        assert after["recover_bytes"] == before["recover_bytes"]
    finally:
        rig.free()
