"""ecg_update_masks on the GPU: the aggregation delta parity update with one set of changed cells
per stripe, the sets given as mask words in device memory.

The reference is the CPU oracle alone, by linearity: expected parity = parity0 ^
oracle.encode_batch(delta), where a masked cell of delta holds old ^ new and every other cell 0
(a stripe whose mask is 0 or names a cell at or above k has an all-zero delta).  Every comparison
is exact and covers the whole allocation of the old image, the new image and the parity: each
lies between 0xA5 guard bytes and is followed by 0xA5 slack of 24 cells, so a cell index the
kernel failed to bound shows up as changed bytes.  The mask words are compared after every call."""
from itertools import combinations

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (4, 2), (8, 2), (16, 2), (8, 3), (16, 3), (5, 2), (8, 4), (16, 8)]
U64MAX = (1 << 64) - 1
GUARD = 256                 # keeps an image 16-byte aligned inside its (256-byte aligned) allocation
FILL = 0xA5
SLACK = 24                  # cells
ROW_PAD = 4096              # ECG_PARITY_ROW_PAD
BYTE_KERNEL = "ecg_update_masks_byte_kernel"

_REF = {}


def images(oracle, k, p, C_, S_):
    """old [S][k][C], new [S][k][C] (every cell differs from old's) and parity0 [p][S][C] = the
    oracle's encode of old; computed once per shape and never modified."""
    key = (k, p, C_, S_)
    if key not in _REF:
        rng = np.random.default_rng(k * 1000003 + p * 101 + C_ * 7 + S_)
        old = rng.integers(0, 256, (S_, k, C_), dtype=np.uint8)
        new = old ^ rng.integers(1, 256, (S_, k, C_), dtype=np.uint8)
        par = oracle.encode_batch(k, p, C_, S_, old.reshape(-1)).reshape(p, S_, C_)
        for a in (old, new, par):
            a.setflags(write=False)
        _REF[key] = (old, new, par)
    return _REF[key]


def cells_of(m):
    return [c for c in range(32) if m >> c & 1]


def valid(m, k):
    return m != 0 and m >> k == 0


def model(masks, k):
    """The rule of the issue: the four result words."""
    ok = [s for s, m in enumerate(masks) if valid(int(m), k)]
    bad = [s for s, m in enumerate(masks) if int(m) >> k]
    return [len(ok), min(bad) if bad else U64MAX, sum(bin(int(masks[s])).count("1") for s in ok), len(bad)]


def invalid_words(k):
    return [1 << k, 1 << 31, 0xFFFFFFFF]


def every_mask(k):
    return list(range(1 << k)) + invalid_words(k)


def k16_masks():
    rng = np.random.default_rng(16)
    singles = [1 << j for j in range(16)]
    pairs = [1 << a | 1 << b for a, b in combinations(range(16), 2)]
    return singles + pairs + [0xFFFF] + [int(x) for x in rng.integers(0, 1 << 16, 64)] + invalid_words(16)


def some_masks(k, n=12):
    """n seeded masks in which every cell occurs, with the full set, a clean stripe and the
    invalid words among them."""
    rng = np.random.default_rng(31 * k + n)
    masks = [(1 << k) - 1, 0, 1, 1 << (k - 1)] + invalid_words(k)
    masks += [int(x) for x in rng.integers(1, 1 << k, max(0, n - len(masks)))]
    assert {c for m in masks if valid(m, k) for c in cells_of(m)} == set(range(k))
    return masks


def lane_kernel(p):
    return f"ecg_update_masks_kernel<{p if p <= 3 else 0}>"


class Rig:
    """Old image, new image and parity on the host (guards, image, slack) and on the device, the
    mask words and the result.  layout "client": data [S][k][C], parity [p][S][C] at the padded
    row pitch; "recovery": stripes [S][k+p][C], old_cells = stripes, parity = stripes + k*C, the
    new image at the same stripe stride.  packed: the old / new images hold the cell of the i-th
    set bit of a stripe's mask in slot i and filler elsewhere (client layout).  skew: byte offset
    of every image from its 16-byte aligned place, or one offset each for (old, new, parity)."""

    def __init__(self, ctx, oracle, k, p, C_, masks, layout="client", skew=0, packed=False, data=None):
        self.ctx, self.k, self.p, self.C, self.S = ctx, k, p, C_, len(masks)
        self.masks_h = [int(m) for m in masks]
        S_ = self.S
        old, new, par = data if data is not None else images(oracle, k, p, C_, S_)
        self.old, self.new = old, new
        so, sn, sp = skew if isinstance(skew, tuple) else (skew, skew, skew)
        self.base, self.nbase = GUARD + so, GUARD + sn
        self.recovery = layout == "recovery"
        cells = k + p if self.recovery else k
        self.ustride = cells * C_
        size = GUARD + 16 + S_ * self.ustride + SLACK * C_ + GUARD
        self.old_img, self.new_img = np.full(size, FILL, np.uint8), np.full(size, FILL, np.uint8)
        ov, nv = self.cells(self.old_img, cells), self.cells(self.new_img, cells, self.nbase)
        if packed:
            assert not self.recovery
            for s, m in enumerate(self.masks_h):
                for i, j in enumerate(cells_of(m & ((1 << k) - 1))):
                    ov[s, i], nv[s, i] = old[s, j], new[s, j]
        else:
            ov[:, :k], nv[:, :k] = old, new
        if self.recovery:
            ov[:, k:] = par.transpose(1, 0, 2)
            self.par_img = self.old_img
            self.pcs, self.pss, self.poff = C_, self.ustride, self.base + k * C_
        else:
            self.pcs, self.pss, self.poff = S_ * C_ + ROW_PAD, C_, GUARD + sp
            self.par_img = np.full(self.poff + p * self.pcs + SLACK * C_ + GUARD, FILL, np.uint8)
            self.rows(self.par_img)[:] = par
        self.old_d, self.new_d = ctx.alloc(size), ctx.alloc(size)
        self.par_d = self.old_d if self.recovery else ctx.alloc(self.par_img.size)
        self.masks, self.result = ctx.alloc(4 * max(1, S_)), ctx.alloc(32)
        self.old_ptr, self.new_ptr = self.old_d.ptr + self.base, self.new_d.ptr + self.nbase
        self.par_ptr = self.par_d.ptr + self.poff

    def cells(self, img, n, base=None):
        base = self.base if base is None else base
        return img[base:base + self.S * self.ustride].reshape(self.S, n, self.C)

    def rows(self, img):
        """[p][S][C] view of the parity cells inside a parity image."""
        return np.lib.stride_tricks.as_strided(img[self.poff:], (self.p, self.S, self.C), (self.pcs, self.pss, 1))

    def expect(self, oracle):
        """The parity image after the call: the image as built with the oracle's encode of the
        masked delta XORed into the parity cells."""
        delta = np.zeros((self.S, self.k, self.C), np.uint8)
        for s, m in enumerate(self.masks_h):
            if valid(m, self.k):
                js = cells_of(m)
                delta[s, js] = self.old[s, js] ^ self.new[s, js]
        want = self.par_img.copy()
        self.rows(want)[:] ^= oracle.encode_batch(self.k, self.p, self.C, self.S, delta.reshape(-1)).reshape(
            self.p, self.S, self.C)
        return want

    def upload(self):
        self.old_d.upload(self.old_img)
        self.new_d.upload(self.new_img)
        if not self.recovery:
            self.par_d.upload(self.par_img)
        self.words = np.array(self.masks_h, dtype=np.uint32)
        if self.S:
            self.masks.upload(self.words.view(np.uint8))
        self.result.fill(0xEE)

    def call(self, flags=0, new_ptr=None):
        self.ctx.update_masks(self.k, self.p, self.C, self.S, self.old_ptr, new_ptr or self.new_ptr, self.ustride,
                              self.par_ptr, self.pcs, self.pss, self.masks.ptr, self.result.ptr, flags)

    def finish(self):
        """One sync.  -> (parity image, result words); the old and the new image and the masks
        are checked to be as they were."""
        self.ctx.sync()
        assert np.array_equal(self.masks.download()[:4 * self.S].view(np.uint32), self.words)      # read only
        if not self.recovery:
            same(self.old_d.download(), self.old_img, self)
        same(self.new_d.download(), self.new_img, self)
        return self.par_d.download(), [int(v) for v in self.result.download().view(np.uint64)]

    def run(self, ecglib, flags=0, **kw):
        """Upload, one call, one sync.  -> (parity image, result words, kernel)."""
        self.upload()
        self.call(flags, **kw)
        name = ecglib.last_kernel()
        return self.finish() + (name,)

    def free(self):
        for b in {self.old_d, self.new_d, self.par_d, self.masks, self.result}:
            b.free()


def same(got, want, rig):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:8] - rig.base, bad.size)


def check(ctx, ecglib, oracle, k, p, C_, masks, kernel, flags=0, **kw):
    rig = Rig(ctx, oracle, k, p, C_, masks, **kw)
    try:
        want = rig.expect(oracle)
        assert not np.array_equal(want, rig.par_img)            # the masks name work
        got, res, name = rig.run(ecglib, flags)
        assert name == kernel, name
        assert res == model(masks, k), res
        same(got, want, rig)
        return got
    finally:
        rig.free()


# ------------------------------------------------------------- 1. shapes, kernels, every mask
@pytest.mark.parametrize("k,p", SHAPES)
def test_every_shape_small_cell(ctx, ecglib, oracle, k, p):
    masks = every_mask(k) if k <= 8 else k16_masks()
    check(ctx, ecglib, oracle, k, p, 16, masks, lane_kernel(p))


@pytest.mark.parametrize("k,p", [(4, 2), (8, 2), (8, 4)])
def test_every_mask_lane_masked_last_column(ctx, ecglib, oracle, k, p):
    check(ctx, ecglib, oracle, k, p, 4096 + 16, every_mask(k), lane_kernel(p))


def test_k16_masks_whole_column(ctx, ecglib, oracle):
    check(ctx, ecglib, oracle, 16, 3, 4096, k16_masks(), lane_kernel(3))


@pytest.mark.parametrize("C_", [4096, 4096 + 16, 8192 + 48])
@pytest.mark.parametrize("k,p", SHAPES)
def test_cell_sizes(ctx, ecglib, oracle, k, p, C_):
    check(ctx, ecglib, oracle, k, p, C_, some_masks(k), lane_kernel(p))


@pytest.mark.parametrize("k,p", [(4, 2), (16, 8)])
def test_column_and_row_loops_stride(ctx, ecglib, oracle, k, p):
    """3 columns on 2 column blocks, 12 stripes on 5 block rows."""
    ctx.set_launch(2, 5, 0)
    try:
        for flags in (0, ecglib.RM_SPARSE):
            check(ctx, ecglib, oracle, k, p, 8192 + 48, some_masks(k), lane_kernel(p), flags=flags)
    finally:
        ctx.set_launch(0, 0, 0)


# --------------------------------------------------------------------------- 2. byte kernel
@pytest.mark.parametrize("k,p", [(4, 2), (8, 3), (5, 2), (16, 8)])
def test_byte_kernel_skewed_images(ctx, ecglib, oracle, k, p):
    check(ctx, ecglib, oracle, k, p, 4099, some_masks(k), BYTE_KERNEL, skew=1)


@pytest.mark.parametrize("k,p", [(4, 2), (16, 3), (8, 4)])
def test_byte_kernel_forced_gives_the_lane_kernels_bytes(ctx, ecglib, oracle, k, p):
    masks = some_masks(k)
    lane = check(ctx, ecglib, oracle, k, p, 4096 + 16, masks, lane_kernel(p))
    ctx.set_launch(0, 0, 2)
    try:
        byte = check(ctx, ecglib, oracle, k, p, 4096 + 16, masks, BYTE_KERNEL)
    finally:
        ctx.set_launch(0, 0, 0)
    assert np.array_equal(lane, byte)


@pytest.mark.parametrize("what", ["cell", "old", "new", "parity"])
def test_any_operand_off_16_bytes_takes_the_byte_kernel(ctx, ecglib, oracle, what):
    """The lane kernel needs every operand and stride a 16-byte multiple: cells of 8 bytes more
    (every stride then 8 off), or one of the three images 8 bytes off, runs the byte kernel."""
    k, p = 4, 2
    C_ = 4096 + 8 if what == "cell" else 4096
    skew = {"cell": 0, "old": (8, 0, 0), "new": (0, 8, 0), "parity": (0, 0, 8)}[what]
    check(ctx, ecglib, oracle, k, p, C_, [0b0101, 0, 0b1111, 1 << k, 0b1000], BYTE_KERNEL, skew=skew)


# ------------------------------------------------------------------- 3. layouts and flags
@pytest.mark.parametrize("k,p,C_", [(4, 2, 4096 + 16), (8, 3, 4096), (16, 8, 16), (5, 2, 4099)])
def test_recovery_layout_old_cells_are_the_stripes(ctx, ecglib, oracle, k, p, C_):
    check(ctx, ecglib, oracle, k, p, C_, some_masks(k), lane_kernel(p) if C_ % 16 == 0 else BYTE_KERNEL,
          layout="recovery")


@pytest.mark.parametrize("k,p,C_,variant", [(4, 2, 16, 0), (8, 2, 4096 + 16, 0), (16, 3, 4096, 0), (8, 4, 4099, 0),
                                            (8, 2, 4096 + 16, 2)])
def test_packed_equals_the_full_image_form(ctx, ecglib, oracle, k, p, C_, variant):
    masks = every_mask(k) if k <= 4 else some_masks(k, 20)
    kernel = lane_kernel(p) if C_ % 16 == 0 and variant == 0 else BYTE_KERNEL
    ctx.set_launch(0, 0, variant)
    try:
        full = check(ctx, ecglib, oracle, k, p, C_, masks, kernel)
        packed = check(ctx, ecglib, oracle, k, p, C_, masks, kernel, flags=ecglib.UM_PACKED, packed=True)
    finally:
        ctx.set_launch(0, 0, 0)
    assert np.array_equal(full, packed)


# ---------------------------------------------------------------- 4. scan and edge cases
@pytest.mark.parametrize("variant", [0, 2])
def test_work_at_the_ends_of_the_block_rows(ctx, ecglib, oracle, variant):
    """S = 130: work only at stripes 0, 63, 64 and 129, with and without ECG_RM_SPARSE."""
    k, p, C_, S_ = 8, 2, 4096 + 16, 130
    masks = [0] * S_
    masks[0], masks[63], masks[64], masks[129] = 0x81, 0xFF, 0x02, 0x7E
    rig = Rig(ctx, oracle, k, p, C_, masks)
    ctx.set_launch(0, 0, variant)
    try:
        want = rig.expect(oracle)
        out = [rig.run(ecglib, flags) for flags in (0, ecglib.RM_SPARSE)]
        for got, res, name in out:
            assert name == (BYTE_KERNEL if variant else lane_kernel(p))
            assert res == [4, U64MAX, 2 + 8 + 1 + 6, 0]
            same(got, want, rig)
    finally:
        ctx.set_launch(0, 0, 0)
        rig.free()


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_nothing_to_do_changes_nothing(ctx, ecglib, oracle, flags):
    """All-zero masks, nstripes = 0 and cell_bytes = 0: no byte changes, result {0, MAX, 0, 0}."""
    k, p, C_, S_ = 4, 2, 4096, 70
    rig = Rig(ctx, oracle, k, p, C_, [0] * S_)
    L = ecglib.lib()
    try:
        got, res, _ = rig.run(ecglib, flags)
        assert res == [0, U64MAX, 0, 0]
        same(got, rig.par_img, rig)
        rig.masks.upload(np.full(S_, 3, np.uint32).view(np.uint8))
        rig.words[:] = 3
        for S__, C__ in ((0, C_), (S_, 0)):
            rig.result.fill(0xEE)
            assert L.ecg_update_masks(ctx.h, k, p, C__, S__, rig.old_ptr, rig.new_ptr, rig.ustride, rig.par_ptr,
                                      rig.pcs, rig.pss, rig.masks.ptr, rig.result.ptr, flags, None) == 0
            got, res = rig.finish()
            assert res == [0, U64MAX, 0, 0]
            same(got, rig.par_img, rig)
    finally:
        rig.free()


def test_any_mask_value_is_safe(ctx, ecglib, oracle):
    """200 random 32-bit words and the edge values on k = 5: only the stripes the model calls
    valid change, whichever kernel, grid and flag."""
    k, p, C_ = 5, 2, 4096
    rng = np.random.default_rng(5)
    masks = [int(x) for x in rng.integers(0, 1 << 32, 100)] + [int(x) for x in rng.integers(0, 1 << 6, 80)]
    masks += [0xFFFFFFFF, 0, 1 << 31, 1 << k, 1 << 16, 1 << 17, 0x80000001, (1 << k) - 1, 1 << (k - 1), 0x10000 | 1]
    masks += [0] * (200 - len(masks))
    words = model(masks, k)
    assert words[0] >= 30 and words[3] >= 100
    rig = Rig(ctx, oracle, k, p, C_, masks)
    try:
        want = rig.expect(oracle)
        for grid in ((0, 0), (1, 2)):
            for variant in (0, 2):
                for flags in (0, ecglib.RM_SPARSE):
                    ctx.set_launch(grid[0], grid[1], variant)
                    try:
                        got, res, _ = rig.run(ecglib, flags)
                    finally:
                        ctx.set_launch(0, 0, 0)
                    assert res == words, (grid, variant, flags)
                    same(got, want, rig)
    finally:
        rig.free()


# -------------------------------------------------------------- 5. against existing calls
@pytest.mark.parametrize("k,p,C_,idx", [(8, 2, 4096 + 16, [1, 6]), (16, 3, 4096, [0, 7, 15]), (4, 2, 4099, [3]),
                                        (16, 8, 4096, [2, 3, 4, 11])])
def test_homogeneous_batch_equals_update(ctx, ecglib, oracle, k, p, C_, idx):
    """One mask for every stripe: byte for byte the parity ecg_update leaves with the same
    cell_idx over the same (packed) cells."""
    S_ = 6
    m = sum(1 << j for j in idx)
    rig = Rig(ctx, oracle, k, p, C_, [m] * S_, packed=True)
    twin = ctx.alloc(rig.par_img.size)
    try:
        twin.upload(rig.par_img)
        rig.upload()
        ctx.update(k, p, C_, S_, idx, rig.old_ptr, rig.new_ptr, rig.ustride, twin.ptr + rig.poff, rig.pcs, rig.pss)
        rig.call(ecglib.UM_PACKED)
        got, res = rig.finish()
        assert res == [S_, U64MAX, len(idx) * S_, 0]
        want = twin.download()
        assert not np.array_equal(want, rig.par_img)
        same(got, want, rig)
        same(got, rig.expect(oracle), rig)
    finally:
        twin.free()
        rig.free()


def test_old_equal_new_leaves_the_parity(ctx, ecglib, oracle):
    k, p, C_ = 8, 2, 4096 + 16
    masks = some_masks(k)
    rig = Rig(ctx, oracle, k, p, C_, masks)
    try:
        got, res, name = rig.run(ecglib, new_ptr=rig.old_ptr)
        assert name == lane_kernel(p)
        assert res == model(masks, k)
        same(got, rig.par_img, rig)
    finally:
        rig.free()


def test_two_calls_back_to_back_on_one_stream(ctx, ecglib, oracle):
    """old -> mid with one set of masks, then mid -> new with another, queued without a sync in
    between: the parity of the oracle's encode of new."""
    k, p, C_, S_ = 8, 2, 4096 + 16, 9
    old, new, par = images(oracle, k, p, C_, S_)
    rng = np.random.default_rng(9)
    m1 = [int(x) for x in rng.integers(0, 1 << k, S_)]
    m2 = [int(x) for x in rng.integers(0, 1 << k, S_)]
    m1[0], m2[1] = 0, 0
    mid = old.copy()
    for s in range(S_):
        mid[s, cells_of(m1[s])] = new[s, cells_of(m1[s])]
    end = mid.copy()
    for s in range(S_):
        js = cells_of(m2[s])
        end[s, js] = mid[s, js] ^ 0x3C
    rig = Rig(ctx, oracle, k, p, C_, m1, data=(old, mid, par))
    end_d = ctx.alloc(rig.new_img.size)
    masks2, result2 = ctx.alloc(4 * S_), ctx.alloc(32)
    try:
        end_img = rig.new_img.copy()
        rig.cells(end_img, k, rig.nbase)[:] = end
        end_d.upload(end_img)
        masks2.upload(np.array(m2, np.uint32).view(np.uint8))
        rig.upload()
        rig.call()
        ctx.update_masks(k, p, C_, S_, rig.new_ptr, end_d.ptr + rig.nbase, rig.ustride, rig.par_ptr, rig.pcs, rig.pss,
                         masks2.ptr, result2.ptr)
        got, res = rig.finish()
        assert res == model(m1, k)
        assert [int(v) for v in result2.download().view(np.uint64)] == model(m2, k)
        want = rig.par_img.copy()
        rig.rows(want)[:] = oracle.encode_batch(k, p, C_, S_, end.reshape(-1)).reshape(p, S_, C_)
        same(got, want, rig)
        same(end_d.download(), end_img, rig)
    finally:
        for b in (end_d, masks2, result2):
            b.free()
        rig.free()


# -------------------------------------------------- 6. the device chain, no host round trip
@pytest.mark.parametrize("k,p", [(8, 2), (16, 3)])
def test_checksum_driven_update(ctx, ecglib, oracle, k, p):
    """csum_extents(old), csum_extents(new), memset, csum_mask, update_masks on one stream with
    one sync: the new image differs from the old in chosen cells only, the masks come out as
    those cells and the parity as the oracle's encode of the new data."""
    C_, S_, htype = 8192, 12, ecglib.HASH_CRC64
    old, _, par = images(oracle, k, p, C_, S_)
    changed = {0: [0], 1: [k - 1], 3: [1, 2, k - 1], 4: list(range(k)), 7: [k // 2], 11: [0, k - 1]}
    new = old.copy()
    for s, js in changed.items():
        for i, j in enumerate(js):
            new[s, j, (s * 131 + i * 977 + (4096 if i % 2 else 0)) % C_] ^= 0x40 >> (i % 7)    # one bit per cell
    want_masks = [sum(1 << j for j in changed.get(s, [])) for s in range(S_)]
    rig = Rig(ctx, oracle, k, p, C_, [0] * S_, data=(old, new, par))
    nch = ecglib.lib().ecg_csum_chunk_count(4096, 1, 0, C_)
    assert nch == 2
    cs_old, cs_new = ctx.alloc(8 * S_ * k * nch), ctx.alloc(8 * S_ * k * nch)
    try:
        rig.upload()
        rig.masks.fill(0xEE)
        ctx.csum_extents(htype, 4096, 1, 0, C_, rig.old_ptr, C_, S_ * k, cs_old.ptr)
        ctx.csum_extents(htype, 4096, 1, 0, C_, rig.new_ptr, C_, S_ * k, cs_new.ptr)
        rig.masks.fill(0)
        ctx.csum_mask(htype, cs_new.ptr, cs_old.ptr, S_, k, nch, k * nch, nch, 0, rig.masks.ptr)
        rig.call()
        assert ecglib.last_kernel() == lane_kernel(p)
        rig.words = np.array(want_masks, np.uint32)             # what csum_mask is to have written
        got, res = rig.finish()
        assert res == [len(changed), U64MAX, sum(len(js) for js in changed.values()), 0]
        want = rig.par_img.copy()
        rig.rows(want)[:] = oracle.encode_batch(k, p, C_, S_, new.reshape(-1)).reshape(p, S_, C_)
        same(got, want, rig)
    finally:
        for b in (cs_old, cs_new):
            b.free()
        rig.free()


# ------------------------------------------------------------------- 7. arguments, stats
def test_argument_errors_on_a_live_context(ctx, ecglib, oracle):
    k, p, C_, S_ = 4, 2, 4096, 9
    rig = Rig(ctx, oracle, k, p, C_, [1] * S_)
    L = ecglib.lib()
    try:
        rig.upload()

        def call(k_=k, p_=p, masks=rig.masks.ptr, result=rig.result.ptr, flags=0, old=rig.old_ptr, parity=rig.par_ptr):
            return L.ecg_update_masks(ctx.h, k_, p_, C_, S_, old, rig.new_ptr, rig.ustride, parity, rig.pcs, rig.pss,
                                      masks, result, flags, None)

        for kk, pp in ((17, 2), (0, 2), (4, 9), (4, 0)):
            assert call(k_=kk, p_=pp) == -ecglib.DER_INVAL, (kk, pp)
            assert b"k <= 16" in L.ecg_strerror()
        assert call(result=rig.result.ptr + 4) == -ecglib.DER_INVAL
        assert call(masks=rig.masks.ptr + 2) == -ecglib.DER_INVAL
        assert call(masks=None) == -ecglib.DER_INVAL
        assert call(flags=4) == -ecglib.DER_INVAL
        assert call(old=None) == -ecglib.DER_INVAL
        assert call(parity=None) == -ecglib.DER_INVAL
        for inside in (rig.par_ptr, rig.par_ptr + rig.pcs - 64, rig.par_ptr + rig.pcs + S_ * C_ - 4):
            assert call(masks=inside) == -ecglib.DER_INVAL
            assert b"masks overlaps the parity" in L.ecg_strerror()
            assert call(result=inside - inside % 8) == -ecglib.DER_INVAL
            assert b"result overlaps the parity" in L.ecg_strerror()
        got, _ = rig.finish()
        same(got, rig.par_img, rig)                             # none of the calls above wrote a cell
    finally:
        rig.free()


def test_counts_one_launch_and_no_update_cells(ctx, ecglib, oracle):
    rig = Rig(ctx, oracle, 4, 2, 4096, [1, 3, 0, 15, 2, 8])
    try:
        rig.run(ecglib)
        before = ctx.stats()
        rig.run(ecglib)
        after = ctx.stats()
        assert after["launches"] == before["launches"] + 1
        assert after["update_cells"] == before["update_cells"]          # the count lives on the device
        assert after["update_bytes"] == before["update_bytes"]
    finally:
        rig.free()
