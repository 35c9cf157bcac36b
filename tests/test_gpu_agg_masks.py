"""ecg_agg_masks on the GPU: ecg_update_masks with a route per stripe -- the delta update for a
stripe whose mask names at most T cells, a re-encode of the merged stripe for one that names more.

The reference is the CPU oracle alone (oracle.encode_batch), per stripe: an invalid or zero mask
leaves the parity as it was; a delta stripe gets parity0 ^ encode(masked delta); a recalc stripe
gets encode(merged stripe), merged = the new cell where the mask has a bit, else the old cell.
The stored parity is STALE on purpose -- parity0 = encode(old) ^ noise, the noise non-zero in every
byte -- so the two routes differ in every parity byte: a delta stripe comes out as encode(merged)
^ noise, a recalc stripe as encode(merged) exactly, and a stripe that took the wrong route fails.
Every comparison is exact and covers the whole allocation of the old image, the new image and the
parity between 0xA5 guards with 24 cells of slack (the Rig of tests.test_gpu_update_masks); the
mask words are compared after every call."""
import numpy as np
import pytest

from tests import test_gpu_update_masks as um

pytestmark = pytest.mark.gpu

SHAPES = um.SHAPES
U64MAX = um.U64MAX
BYTE_KERNEL = "ecg_agg_masks_byte_kernel"
AUTO = 0xFFFFFFFF

_STALE = {}


def lane_kernel(p):
    return f"ecg_agg_masks_kernel<{p if p <= 3 else 0}>"


def eff(T, k, p):
    """The effective threshold: the issue's arithmetic for ECG_AGG_AUTO."""
    return ((k - p) // 2 if k > p else 0) if T == AUTO else T


def thresholds(k):
    """T of the issue's route test, {0, 1, AUTO, k-1, k}, each once."""
    return sorted({0, min(1, k), k - 1, k}) + [AUTO]


def route(m, k, T):
    """None: the stripe stays; else 'delta' or 'recalc' (T effective)."""
    if not um.valid(m, k):
        return None
    return "recalc" if bin(m).count("1") > T else "delta"


def stale(oracle, k, p, C_, S_):
    """um.images with the parity XORed with noise that is non-zero in every byte: (old, new, parity0,
    noise), computed once per shape and never modified."""
    key = (k, p, C_, S_)
    if key not in _STALE:
        old, new, par = um.images(oracle, k, p, C_, S_)
        noise = np.random.default_rng(77 + k + 17 * p + C_ + S_).integers(1, 256, par.shape, dtype=np.uint8)
        par0 = par ^ noise
        for a in (noise, par0):
            a.setflags(write=False)
        _STALE[key] = (old, new, par0, noise)
    return _STALE[key]


class Rig(um.Rig):
    """um.Rig over a stale parity, calling ecg_agg_masks."""

    def __init__(self, ctx, oracle, k, p, C_, masks, data=None, noise=None, **kw):
        if data is None:
            old, new, par0, noise = stale(oracle, k, p, C_, len(masks))
            data = (old, new, par0)
        self.noise = noise
        super().__init__(ctx, oracle, k, p, C_, masks, data=data, **kw)
        self.T = AUTO

    def expect(self, oracle, T=AUTO, new=None, masks=None):
        """The parity image after the call with threshold T (over `new` instead of the new image)."""
        k, p, C_, S_ = self.k, self.p, self.C, self.S
        new = self.new if new is None else new
        masks = self.masks_h if masks is None else masks
        T = eff(T, k, p)
        delta, merged = np.zeros((S_, k, C_), np.uint8), self.old.copy()
        for s, m in enumerate(masks):
            if um.valid(m, k):
                js = um.cells_of(m)
                delta[s, js] = self.old[s, js] ^ new[s, js]
                merged[s, js] = new[s, js]
        enc_d = oracle.encode_batch(k, p, C_, S_, delta.reshape(-1)).reshape(p, S_, C_)
        enc_m = oracle.encode_batch(k, p, C_, S_, merged.reshape(-1)).reshape(p, S_, C_)
        want = self.par_img.copy()
        rows = self.rows(want)
        for s, m in enumerate(masks):
            r = route(m, k, T)
            if r == "delta":
                rows[:, s] ^= enc_d[:, s]
                if self.noise is not None:      # the stale parity carried forward
                    assert np.array_equal(rows[:, s], enc_m[:, s] ^ self.noise[:, s])
            elif r == "recalc":
                rows[:, s] = enc_m[:, s]
        return want

    def call(self, flags=0, new_ptr=None, T=None):
        self.ctx.agg_masks(self.k, self.p, self.C, self.S, self.old_ptr, new_ptr or self.new_ptr, self.ustride,
                           self.par_ptr, self.pcs, self.pss, self.masks.ptr, self.result.ptr,
                           self.T if T is None else T, flags)

    def run(self, ecglib, flags=0, T=AUTO, **kw):
        self.T = T
        return super().run(ecglib, flags, **kw)


def check(ctx, ecglib, oracle, k, p, C_, masks, kernel, Ts=None, flags=0, **kw):
    """One rig, one run per threshold; -> the parity images."""
    rig = Rig(ctx, oracle, k, p, C_, masks, **kw)
    out = []
    try:
        for T in thresholds(k) if Ts is None else Ts:
            want = rig.expect(oracle, T)
            assert not np.array_equal(want, rig.par_img)        # the masks name work
            got, res, name = rig.run(ecglib, flags, T=T)
            assert name == kernel, name
            assert res == um.model(masks, k), (T, res)
            um.same(got, want, rig)
            out.append(got)
        return out
    finally:
        rig.free()


# ------------------------------------------------------------------ 1. the route per stripe
@pytest.mark.parametrize("k,p", SHAPES + [(2, 3)])
def test_route_every_mask_every_threshold(ctx, ecglib, oracle, k, p):
    """The test that pins the feature: over a stale parity, delta stripes come out as encode(merged)
    ^ noise, recalc stripes as encode(merged), invalid and zero stripes stay -- for T in {0, 1, AUTO,
    k-1, k} and every mask (k <= 8) or the k16 set."""
    masks = um.every_mask(k) if k <= 8 else um.k16_masks()
    routes = {route(m, k, eff(AUTO, k, p)) for m in masks}
    assert routes == ({None, "delta", "recalc"} if k > p + 1 else {None, "recalc"})
    check(ctx, ecglib, oracle, k, p, 16, masks, lane_kernel(p))


@pytest.mark.parametrize("C_", [4096, 4096 + 16, 8192 + 48])
@pytest.mark.parametrize("k,p", SHAPES + [(2, 3)])
def test_route_cell_sizes(ctx, ecglib, oracle, k, p, C_):
    check(ctx, ecglib, oracle, k, p, C_, um.some_masks(k), lane_kernel(p))


@pytest.mark.parametrize("k,p,C_", [(8, 2, 4096 + 16), (16, 3, 4096), (5, 2, 4099), (16, 8, 16)])
def test_threshold_k_is_update_masks(ctx, ecglib, oracle, k, p, C_):
    """T = k: byte for byte what ecg_update_masks leaves on the same stale-parity inputs."""
    masks = um.some_masks(k, 20)
    rig = Rig(ctx, oracle, k, p, C_, masks)
    twin = ctx.alloc(rig.par_img.size)
    try:
        twin.upload(rig.par_img)
        rig.upload()
        ctx.update_masks(k, p, C_, rig.S, rig.old_ptr, rig.new_ptr, rig.ustride, twin.ptr + rig.poff, rig.pcs, rig.pss,
                         rig.masks.ptr, rig.result.ptr)
        ctx.sync()
        words = [int(v) for v in rig.result.download().view(np.uint64)]
        rig.result.fill(0xEE)
        rig.call(T=k)
        got, res = rig.finish()
        assert res == words == um.model(masks, k)
        want = twin.download()
        assert not np.array_equal(want, rig.par_img)
        um.same(got, want, rig)
        um.same(got, rig.expect(oracle, k), rig)
    finally:
        twin.free()
        rig.free()


@pytest.mark.parametrize("k,p,C_", [(8, 2, 4096 + 16), (16, 3, 4096), (4, 2, 16), (16, 8, 8192 + 48)])
def test_threshold_0_is_encode_of_the_merged_image(ctx, ecglib, oracle, k, p, C_):
    """T = 0: on every valid non-zero stripe byte for byte what ecg_encode writes for the merged
    image; the other stripes keep their stale parity."""
    masks = um.some_masks(k, 20)
    rig = Rig(ctx, oracle, k, p, C_, masks)
    merged = rig.old.copy()
    for s, m in enumerate(masks):
        if um.valid(m, k):
            merged[s, um.cells_of(m)] = rig.new[s, um.cells_of(m)]
    data, twin = ctx.to_device(merged.reshape(-1)), ctx.alloc(rig.par_img.size)
    try:
        twin.upload(rig.par_img)
        ctx.encode(k, p, C_, rig.S, data.ptr, k * C_, twin.ptr + rig.poff, rig.pcs, rig.pss)
        got, res, _ = rig.run(ecglib, T=0)
        assert res == um.model(masks, k)
        enc = rig.rows(twin.download())
        want = rig.par_img.copy()
        for s, m in enumerate(masks):
            if um.valid(m, k):
                rig.rows(want)[:, s] = enc[:, s]
        assert not np.array_equal(want, rig.par_img)
        um.same(got, want, rig)
        um.same(got, rig.expect(oracle, 0), rig)
    finally:
        for b in (data, twin):
            b.free()
        rig.free()


# ------------------------------------------------------------------------- 2. kernel selection
@pytest.mark.parametrize("k,p", [(4, 2), (8, 3), (5, 2), (16, 8)])
def test_byte_kernel_skewed_images(ctx, ecglib, oracle, k, p):
    check(ctx, ecglib, oracle, k, p, 4099, um.some_masks(k), BYTE_KERNEL, skew=1)


@pytest.mark.parametrize("k,p", [(4, 2), (16, 3), (8, 4)])
def test_byte_kernel_forced_gives_the_lane_kernels_bytes(ctx, ecglib, oracle, k, p):
    masks = um.some_masks(k)
    lane = check(ctx, ecglib, oracle, k, p, 4096 + 16, masks, lane_kernel(p))
    ctx.set_launch(0, 0, 2)
    try:
        byte = check(ctx, ecglib, oracle, k, p, 4096 + 16, masks, BYTE_KERNEL)
    finally:
        ctx.set_launch(0, 0, 0)
    assert all(np.array_equal(a, b) for a, b in zip(lane, byte))


@pytest.mark.parametrize("what", ["cell", "old", "new", "parity"])
def test_any_operand_off_16_bytes_takes_the_byte_kernel(ctx, ecglib, oracle, what):
    k, p = 4, 2
    C_ = 4096 + 8 if what == "cell" else 4096
    skew = {"cell": 0, "old": (8, 0, 0), "new": (0, 8, 0), "parity": (0, 0, 8)}[what]
    check(ctx, ecglib, oracle, k, p, C_, [0b0101, 0, 0b1111, 1 << k, 0b1000], BYTE_KERNEL, Ts=[1, AUTO], skew=skew)


# ------------------------------------------------------------------------------ 3. grid and scan
@pytest.mark.parametrize("k,p", [(4, 2), (16, 8)])
def test_column_and_row_loops_stride(ctx, ecglib, oracle, k, p):
    """3 columns on 2 column blocks, 12 stripes on 5 block rows, both grids."""
    ctx.set_launch(2, 5, 0)
    try:
        for flags in (0, ecglib.RM_SPARSE):
            check(ctx, ecglib, oracle, k, p, 8192 + 48, um.some_masks(k), lane_kernel(p), Ts=[AUTO, 1], flags=flags)
    finally:
        ctx.set_launch(0, 0, 0)


@pytest.mark.parametrize("variant", [0, 2])
def test_work_at_the_ends_of_the_block_rows(ctx, ecglib, oracle, variant):
    """S = 130: work only at stripes 0, 63, 64 and 129, two on each route (T = AUTO = 3), with and
    without ECG_RM_SPARSE."""
    k, p, C_, S_ = 8, 2, 4096 + 16, 130
    masks = [0] * S_
    masks[0], masks[63], masks[64], masks[129] = 0x81, 0xFF, 0x02, 0x7E
    assert [route(masks[s], k, 3) for s in (0, 63, 64, 129)] == ["delta", "recalc", "delta", "recalc"]
    rig = Rig(ctx, oracle, k, p, C_, masks)
    ctx.set_launch(0, 0, variant)
    try:
        want = rig.expect(oracle, AUTO)
        for flags in (0, ecglib.RM_SPARSE):
            got, res, name = rig.run(ecglib, flags)
            assert name == (BYTE_KERNEL if variant else lane_kernel(p))
            assert res == [4, U64MAX, 2 + 8 + 1 + 6, 0]
            um.same(got, want, rig)
    finally:
        ctx.set_launch(0, 0, 0)
        rig.free()


def test_any_mask_value_is_safe(ctx, ecglib, oracle):
    """200 random 32-bit words and the edge values on k = 5: only the stripes the model calls valid
    change, each by its route, whichever kernel, grid and flag."""
    k, p, C_ = 5, 2, 4096
    rng = np.random.default_rng(5)
    masks = [int(x) for x in rng.integers(0, 1 << 32, 100)] + [int(x) for x in rng.integers(0, 1 << 6, 80)]
    masks += [0xFFFFFFFF, 0, 1 << 31, 1 << k, 1 << 16, 1 << 17, 0x80000001, (1 << k) - 1, 1 << (k - 1), 0x10000 | 1]
    masks += [0] * (200 - len(masks))
    words = um.model(masks, k)
    assert words[0] >= 30 and words[3] >= 100
    assert {route(m, k, 1) for m in masks} == {None, "delta", "recalc"}
    rig = Rig(ctx, oracle, k, p, C_, masks)
    try:
        want = rig.expect(oracle, AUTO)
        for grid in ((0, 0), (1, 2)):
            for variant in (0, 2):
                for flags in (0, ecglib.RM_SPARSE):
                    ctx.set_launch(grid[0], grid[1], variant)
                    try:
                        got, res, _ = rig.run(ecglib, flags)
                    finally:
                        ctx.set_launch(0, 0, 0)
                    assert res == words, (grid, variant, flags)
                    um.same(got, want, rig)
    finally:
        rig.free()


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("T", [0, AUTO])
def test_nothing_to_do_changes_nothing(ctx, ecglib, oracle, flags, T):
    """All-zero masks, nstripes = 0 and cell_bytes = 0: no byte changes, result {0, MAX, 0, 0}."""
    k, p, C_, S_ = 4, 2, 4096, 70
    rig = Rig(ctx, oracle, k, p, C_, [0] * S_)
    L = ecglib.lib()
    try:
        got, res, _ = rig.run(ecglib, flags, T=T)
        assert res == [0, U64MAX, 0, 0]
        um.same(got, rig.par_img, rig)
        rig.masks.upload(np.full(S_, 3, np.uint32).view(np.uint8))
        rig.words[:] = 3
        for S__, C__ in ((0, C_), (S_, 0)):
            rig.result.fill(0xEE)
            assert L.ecg_agg_masks(ctx.h, k, p, C__, S__, rig.old_ptr, rig.new_ptr, rig.ustride, rig.par_ptr,
                                   rig.pcs, rig.pss, rig.masks.ptr, rig.result.ptr, T, flags, None) == 0
            got, res = rig.finish()
            assert res == [0, U64MAX, 0, 0]
            um.same(got, rig.par_img, rig)
    finally:
        rig.free()


# ----------------------------------------------------------------------- 4. layouts and operands
@pytest.mark.parametrize("k,p,C_", [(4, 2, 4096 + 16), (8, 3, 4096), (16, 8, 16), (5, 2, 4099)])
def test_recovery_layout_old_cells_are_the_stripes(ctx, ecglib, oracle, k, p, C_):
    """old_cells = stripes [S][k+p][C], the parity inside them: the recalc route reads the k data
    cells of a stripe and none of its parity cells."""
    check(ctx, ecglib, oracle, k, p, C_, um.some_masks(k), lane_kernel(p) if C_ % 16 == 0 else BYTE_KERNEL,
          layout="recovery")


def test_negative_strides(ctx, ecglib, oracle):
    """The batch walked from its last stripe to its first: all three stripe strides negative, the
    mask words in the call's order."""
    k, p, C_ = 8, 2, 4096 + 16
    masks = um.some_masks(k)
    S_ = len(masks)
    rig = Rig(ctx, oracle, k, p, C_, masks)
    try:
        want = rig.expect(oracle, AUTO)
        rig.upload()
        rig.words = np.array(masks[::-1], dtype=np.uint32)
        rig.masks.upload(rig.words.view(np.uint8))
        last = (S_ - 1) * rig.ustride
        ctx.agg_masks(k, p, C_, S_, rig.old_ptr + last, rig.new_ptr + last, -rig.ustride,
                      rig.par_ptr + (S_ - 1) * rig.pss, rig.pcs, -rig.pss, rig.masks.ptr, rig.result.ptr)
        assert ecglib.last_kernel() == lane_kernel(p)
        got, res = rig.finish()
        assert res == um.model(masks[::-1], k)
        um.same(got, want, rig)
    finally:
        rig.free()


def test_old_equal_new_reencodes_the_old_data(ctx, ecglib, oracle):
    """old_cells == new_cells: T = 0 leaves encode(old) on every stripe with work, whatever the
    stale parity held; T = k leaves every parity byte as it was."""
    k, p, C_ = 8, 2, 4096 + 16
    masks = um.some_masks(k)
    rig = Rig(ctx, oracle, k, p, C_, masks)
    try:
        want = rig.par_img.copy()
        for s, m in enumerate(masks):
            if um.valid(m, k):
                rig.rows(want)[:, s] ^= rig.noise[:, s]         # parity0 = encode(old) ^ noise
        um.same(want, rig.expect(oracle, 0, new=rig.old), rig)
        got, res, name = rig.run(ecglib, T=0, new_ptr=rig.old_ptr)
        assert name == lane_kernel(p)
        assert res == um.model(masks, k)
        um.same(got, want, rig)
        got, res, _ = rig.run(ecglib, T=k, new_ptr=rig.old_ptr)
        assert res == um.model(masks, k)
        um.same(got, rig.par_img, rig)
    finally:
        rig.free()


def test_two_calls_back_to_back_on_one_stream(ctx, ecglib, oracle):
    """old -> mid with one set of masks, then mid -> end with another, queued without a sync in
    between over a consistent parity: the oracle's encode of end, whichever routes were taken."""
    k, p, C_, S_ = 8, 2, 4096 + 16, 9
    old, new, par = um.images(oracle, k, p, C_, S_)
    rng = np.random.default_rng(9)
    m1 = [int(x) for x in rng.integers(0, 1 << k, S_)]
    m2 = [int(x) for x in rng.integers(0, 1 << k, S_)]
    m1[0], m2[1], m1[2], m2[3] = 0, 0, 0xFF, 0xFF
    mid = old.copy()
    for s in range(S_):
        mid[s, um.cells_of(m1[s])] = new[s, um.cells_of(m1[s])]
    end = mid.copy()
    for s in range(S_):
        js = um.cells_of(m2[s])
        end[s, js] = mid[s, js] ^ 0x3C
    assert {route(m, k, 3) for m in m1 + m2} == {None, "delta", "recalc"}
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
        ctx.agg_masks(k, p, C_, S_, rig.new_ptr, end_d.ptr + rig.nbase, rig.ustride, rig.par_ptr, rig.pcs, rig.pss,
                      masks2.ptr, result2.ptr)
        got, res = rig.finish()
        assert res == um.model(m1, k)
        assert [int(v) for v in result2.download().view(np.uint64)] == um.model(m2, k)
        want = rig.par_img.copy()
        rig.rows(want)[:] = oracle.encode_batch(k, p, C_, S_, end.reshape(-1)).reshape(p, S_, C_)
        um.same(got, want, rig)
        um.same(end_d.download(), end_img, rig)
    finally:
        for b in (end_d, masks2, result2):
            b.free()
        rig.free()


# -------------------------------------------------- 5. the device chain, no host round trip
@pytest.mark.parametrize("k,p", [(8, 2), (16, 3)])
def test_checksum_driven_aggregation(ctx, ecglib, oracle, k, p):
    """csum_extents(old), csum_extents(new), memset, csum_mask, agg_masks(AUTO), csum_updated on one
    stream with one sync: some stripes changed in one cell, some in all k.  The masks come out as
    those cells, the parity as the oracle's encode of the new data, and the checksums of the
    rewritten parity cells as ecg_csum_extents over them."""
    C_, S_, htype = 8192, 12, ecglib.HASH_CRC64
    old, _, par = um.images(oracle, k, p, C_, S_)
    changed = {0: [0], 1: [k - 1], 3: list(range(k)), 4: list(range(k)), 7: [k // 2], 11: list(range(k))}
    new = old.copy()
    for s, js in changed.items():
        for i, j in enumerate(js):
            new[s, j, (s * 131 + i * 977 + (4096 if i % 2 else 0)) % C_] ^= 0x40 >> (i % 7)    # one bit per cell
    want_masks = [sum(1 << j for j in changed.get(s, [])) for s in range(S_)]
    assert {route(m, k, eff(AUTO, k, p)) for m in want_masks} == {None, "delta", "recalc"}
    rig = Rig(ctx, oracle, k, p, C_, [0] * S_, data=(old, new, par))
    nch = ecglib.lib().ecg_csum_chunk_count(4096, 1, 0, C_)
    assert nch == 2
    cs_old, cs_new = ctx.alloc(8 * S_ * k * nch), ctx.alloc(8 * S_ * k * nch)
    cs_par, cs_ref, result2 = ctx.alloc(8 * S_ * p * nch), ctx.alloc(8 * S_ * p * nch), ctx.alloc(32)
    try:
        rig.upload()
        rig.masks.fill(0xEE)
        cs_par.fill(0)
        ctx.csum_extents(htype, 4096, 1, 0, C_, rig.old_ptr, C_, S_ * k, cs_old.ptr)
        ctx.csum_extents(htype, 4096, 1, 0, C_, rig.new_ptr, C_, S_ * k, cs_new.ptr)
        rig.masks.fill(0)
        ctx.csum_mask(htype, cs_new.ptr, cs_old.ptr, S_, k, nch, k * nch, nch, 0, rig.masks.ptr)
        rig.call()
        assert ecglib.last_kernel() == lane_kernel(p)
        ctx.csum_updated(htype, 4096, 1, k, p, C_, S_, rig.par_ptr, rig.pcs, rig.pss, rig.masks.ptr, cs_par.ptr,
                         p * nch, nch, result2.ptr)
        rig.words = np.array(want_masks, np.uint32)             # what csum_mask is to have written
        got, res = rig.finish()
        assert res == [len(changed), U64MAX, sum(len(js) for js in changed.values()), 0]
        want = rig.par_img.copy()
        rig.rows(want)[:] = oracle.encode_batch(k, p, C_, S_, new.reshape(-1)).reshape(p, S_, C_)
        um.same(got, want, rig)
        # the checksums of the rewritten cells: ecg_csum_extents over each parity row [S][C]
        for r in range(p):
            ctx.csum_extents(htype, 4096, 1, 0, C_, rig.par_ptr + r * rig.pcs, rig.pss, S_, cs_ref.ptr + 8 * r * S_ * nch)
        ctx.sync()
        ref = cs_ref.download().view(np.uint64).reshape(p, S_, nch)
        sums = cs_par.download().view(np.uint64).reshape(S_, p, nch)
        for s in range(S_):
            assert np.array_equal(sums[s], ref[:, s] if s in changed else np.zeros((p, nch), np.uint64)), s
        assert [int(v) for v in result2.download().view(np.uint64)] == [len(changed), U64MAX, p * len(changed), 0]
    finally:
        for b in (cs_old, cs_new, cs_par, cs_ref, result2):
            b.free()
        rig.free()


# ------------------------------------------------------------------------- 6. arguments, stats
def test_argument_errors_on_a_live_context(ctx, ecglib, oracle):
    k, p, C_, S_ = 4, 2, 4096, 9
    rig = Rig(ctx, oracle, k, p, C_, [1] * S_)
    L = ecglib.lib()
    try:
        rig.upload()

        def call(k_=k, masks=rig.masks.ptr, result=rig.result.ptr, T=1, flags=0, old=rig.old_ptr, parity=rig.par_ptr):
            return L.ecg_agg_masks(ctx.h, k_, p, C_, S_, old, rig.new_ptr, rig.ustride, parity, rig.pcs, rig.pss,
                                   masks, result, T, flags, None)

        assert call(k_=17) == -ecglib.DER_INVAL
        assert call(T=k + 1) == -ecglib.DER_INVAL
        assert L.ecg_strerror().startswith(b"agg_masks: recalc_above=5")
        assert call(T=AUTO - 1) == -ecglib.DER_INVAL
        for flags in (ecglib.UM_PACKED, ecglib.UM_PACKED | ecglib.RM_SPARSE):
            assert call(flags=flags) == -ecglib.DER_INVAL
            assert L.ecg_strerror().startswith(b"agg_masks: ECG_UM_PACKED")
        assert call(flags=4) == -ecglib.DER_INVAL
        assert call(masks=rig.masks.ptr + 2) == -ecglib.DER_INVAL
        assert call(result=rig.result.ptr + 4) == -ecglib.DER_INVAL
        assert call(old=None) == -ecglib.DER_INVAL
        assert call(parity=None) == -ecglib.DER_INVAL
        assert call(masks=rig.par_ptr + rig.pcs - 64) == -ecglib.DER_INVAL
        assert b"agg_masks: masks overlaps the parity" in L.ecg_strerror()
        assert call(result=rig.par_ptr) == -ecglib.DER_INVAL
        assert b"agg_masks: result overlaps the parity" in L.ecg_strerror()
        got, _ = rig.finish()
        um.same(got, rig.par_img, rig)                          # none of the calls above wrote a cell
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
