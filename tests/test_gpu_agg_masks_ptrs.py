"""ecg_agg_masks_ptrs on the GPU: ecg_agg_masks with the cells of every stripe given by address,
2k + p of them per stripe (k old, k new, p parity), over the rig of
tests.test_gpu_update_masks_ptrs: one device allocation between 0xA5 guards, cell (s, c) at a
seeded permuted slot, 24 cells of slack.  Every comparison is exact and covers the whole
allocation; the mask words are verified unchanged.

The expectation is the CPU oracle alone, computed from the bytes the table's row addresses hold (so
it covers tables that are not one-to-one): an invalid or zero mask leaves the parity; a delta
stripe gets parity0 ^ encode(masked delta); a recalc stripe gets encode(merged stripe).  The stored
parity is stale (encode(old) ^ noise, the noise non-zero in every byte; tests.test_gpu_agg_masks),
so a stripe that took the wrong route fails in every parity byte."""
import ctypes as C

import numpy as np
import pytest

from tests import test_gpu_agg_masks as am
from tests import test_gpu_update_masks as um
from tests import test_gpu_update_masks_ptrs as ump

pytestmark = pytest.mark.gpu

U64MAX, GUARD, AUTO = um.U64MAX, um.GUARD, am.AUTO
BYTE_KERNEL = "ecg_agg_masks_ptr_byte_kernel"
SHAPES = um.SHAPES + [(2, 3)]


def ptr_kernel(p):
    return f"ecg_agg_masks_ptr_kernel<{p if p <= 3 else 0}>"


def contents(oracle, k, p, C_, S_):
    """[S][2k+p][C]: old cells, new cells, the stale parity of old."""
    old, new, par0, _ = am.stale(oracle, k, p, C_, S_)
    return np.concatenate([old, new, par0.transpose(1, 0, 2)], axis=1)


class PtrRig(ump.PtrRig):
    def expect(self, oracle, masks, T=AUTO, rows=None):
        """The image after the call over the table `rows` (offsets), from the bytes it names."""
        rows = self.rows() if rows is None else rows
        k, p, C_, S_ = self.k, self.p, self.C, len(rows)
        T = am.eff(T, k, p)
        at = lambda o: self.img[int(o):int(o) + C_]     # noqa: E731
        delta, merged = np.zeros((S_, k, C_), np.uint8), np.zeros((S_, k, C_), np.uint8)
        for s, m in enumerate(masks):
            for j in range(k):
                named = um.valid(int(m), k) and int(m) >> j & 1
                merged[s, j] = at(rows[s][k + j]) if named else at(rows[s][j])
                if named:
                    delta[s, j] = at(rows[s][j]) ^ at(rows[s][k + j])
        enc_d = oracle.encode_batch(k, p, C_, S_, delta.reshape(-1)).reshape(p, S_, C_)
        enc_m = oracle.encode_batch(k, p, C_, S_, merged.reshape(-1)).reshape(p, S_, C_)
        want = self.img.copy()
        for s, m in enumerate(masks):
            how = am.route(int(m), k, T)
            for r in range(p):
                o = int(rows[s][2 * k + r])
                if how == "delta":
                    want[o:o + C_] ^= enc_d[r, s]
                elif how == "recalc":
                    want[o:o + C_] = enc_m[r, s]
        return want

    def call(self, masks, T=AUTO, flags=0, rows=None, tab=None):
        self.ctx.agg_masks_ptrs(self.k, self.p, self.C, len(masks), self.table(rows) if tab is None else tab,
                                self.masks_ptr, self.result.ptr, T, flags)

    def run(self, ecglib, masks, T=AUTO, flags=0, rows=None):
        """Upload image and masks, one call, one sync.  -> (image, result words, kernel)."""
        self.upload(masks)
        self.call(masks, T, flags, rows)
        name = ecglib.last_kernel()
        return self.finish() + (name,)


def check(ctx, ecglib, oracle, k, p, C_, masks, kernel, Ts=None, flags=0, **rig_args):
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, len(masks)), **rig_args)
    out = []
    try:
        for T in am.thresholds(k) if Ts is None else Ts:
            want = rig.expect(oracle, masks, T)
            assert not np.array_equal(want, rig.img)            # the masks name work
            got, res, name = rig.run(ecglib, masks, T, flags)
            assert name == kernel, name
            assert res == um.model(masks, k), (T, res)
            ump.same(got, want)
            out.append(got)
        return out
    finally:
        rig.free()


# ------------------------------------------------------------------ 1. the route per stripe
@pytest.mark.parametrize("k,p", SHAPES)
def test_route_every_mask_every_threshold(ctx, ecglib, oracle, k, p):
    """Scattered cells, a stale parity, T in {0, 1, AUTO, k-1, k}, every mask (k <= 8) or the k16
    set: each stripe comes out by its route and nothing else changes."""
    check(ctx, ecglib, oracle, k, p, 16, um.every_mask(k) if k <= 8 else um.k16_masks(), ptr_kernel(p))


@pytest.mark.parametrize("C_", [4096, 4096 + 16, 8192 + 48])
@pytest.mark.parametrize("k,p", [(4, 2), (8, 3), (5, 2), (16, 8), (2, 3)])
def test_route_cell_sizes(ctx, ecglib, oracle, k, p, C_):
    check(ctx, ecglib, oracle, k, p, C_, um.some_masks(k), ptr_kernel(p))


@pytest.mark.parametrize("k,p", [(4, 2), (16, 8)])
def test_column_and_row_loops_stride(ctx, ecglib, oracle, k, p):
    """3 columns on 2 column blocks, 7 stripes on 5 block rows (dense) or one (sparse)."""
    masks = [m for m in um.some_masks(k) if m][:5] + [0, 1 << k]
    ctx.set_launch(2, 5, 0)
    try:
        for flags in (0, ecglib.RM_SPARSE):
            check(ctx, ecglib, oracle, k, p, 8192 + 48, masks, ptr_kernel(p), Ts=[AUTO, 1], flags=flags)
    finally:
        ctx.set_launch(0, 0, 0)


@pytest.mark.parametrize("variant", [0, 2])
def test_work_at_the_ends_of_the_block_rows(ctx, ecglib, oracle, variant):
    """S = 130: work only at stripes 0, 63, 64 and 129, two on each route, and an invalid word at
    65, with and without ECG_RM_SPARSE."""
    k, p, C_, S_ = 8, 2, 4096 + 16, 130
    masks = [0] * S_
    masks[0], masks[63], masks[64], masks[129], masks[65] = 0x81, 0xFF, 0x02, 0x7E, 1 << k
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, S_))
    ctx.set_launch(0, 0, variant)
    try:
        want = rig.expect(oracle, masks)
        for flags in (0, ecglib.RM_SPARSE):
            got, res, name = rig.run(ecglib, masks, flags=flags)
            assert name == (BYTE_KERNEL if variant else ptr_kernel(p))
            assert res == [4, 65, 2 + 8 + 1 + 6, 1] == um.model(masks, k)
            ump.same(got, want)
    finally:
        ctx.set_launch(0, 0, 0)
        rig.free()


# ------------------------------------------------------------------------------ 2. byte kernel
@pytest.mark.parametrize("c", [1, 4 + 2, 2 * 4 + 1], ids=["old", "new", "parity"])
def test_one_entry_off_16_bytes_sends_the_whole_launch_to_the_byte_kernel(ctx, ecglib, oracle, c):
    k, p = 4, 2
    check(ctx, ecglib, oracle, k, p, 4096, um.some_masks(k), BYTE_KERNEL, Ts=[AUTO, 0],
          skew=lambda s, cc: 8 if (s, cc) == (3, c) else 0)


@pytest.mark.parametrize("C_", [1, 17, 4099])
@pytest.mark.parametrize("k,p", [(4, 2), (8, 3), (5, 4), (16, 8)])
def test_byte_kernel_every_cell_at_an_odd_address(ctx, ecglib, oracle, k, p, C_):
    check(ctx, ecglib, oracle, k, p, C_, um.some_masks(k), BYTE_KERNEL, Ts=[AUTO, 1, k],
          skew=lambda s, c: 1 + 2 * ((s + c) % 8))


@pytest.mark.parametrize("k,p", [(4, 2), (16, 3), (8, 4)])
def test_byte_kernel_forced_gives_the_lane_kernels_bytes(ctx, ecglib, oracle, k, p):
    masks = um.some_masks(k)
    lane = check(ctx, ecglib, oracle, k, p, 4096 + 16, masks, ptr_kernel(p))
    ctx.set_launch(0, 0, 2)
    try:
        byte = check(ctx, ecglib, oracle, k, p, 4096 + 16, masks, BYTE_KERNEL)
    finally:
        ctx.set_launch(0, 0, 0)
    assert all(np.array_equal(a, b) for a, b in zip(lane, byte))


# -------------------------------------------------------------------------- 3. strided routing
@pytest.mark.parametrize("k,p", [(4, 2), (5, 4), (16, 3)])
def test_three_strided_groups_are_the_strided_call(ctx, ecglib, oracle, k, p):
    """A table that is three strided groups names the strided kernel and leaves what ecg_agg_masks
    leaves over the same operands; two rows exchanged and it is a table again."""
    C_ = 4096
    masks = um.some_masks(k)
    S_ = len(masks)
    off, size, _ = ump.groups(k, p, C_, S_, hole=64)
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, S_), off=off, size=size)
    try:
        for T in (AUTO, 1):
            got, res, name = rig.run(ecglib, masks, T)
            assert name == am.lane_kernel(p)                    # three strided images: the strided call
            assert res == um.model(masks, k)
            ump.same(got, rig.expect(oracle, masks, T))
            rig.upload(masks)
            ctx.agg_masks(k, p, C_, S_, rig.buf.ptr + int(off[0][0]), rig.buf.ptr + int(off[0][k]), k * C_,
                          rig.buf.ptr + int(off[0][2 * k]), C_, p * C_ + 64, rig.masks_ptr, rig.result.ptr, T)
            twin, res2 = rig.finish()
            assert res2 == res
            ump.same(got, twin)
        order = list(range(S_))
        order[0], order[S_ - 1] = order[S_ - 1], order[0]       # two valid stripes exchanged: no stride
        pm = [masks[s] for s in order]
        got, res, name = rig.run(ecglib, pm, rows=rig.rows(order))
        assert name == ptr_kernel(p)
        assert res == um.model(pm, k)
        ump.same(got, rig.expect(oracle, pm, rows=rig.rows(order)))
    finally:
        rig.free()


def test_negative_strides_between_the_rows(ctx, ecglib, oracle):
    """Three strided groups listed from the last stripe to the first: the strided call with all
    three stripe strides negative."""
    k, p, C_ = 4, 2, 4096
    masks = um.some_masks(k)
    S_ = len(masks)
    off, size, _ = ump.groups(k, p, C_, S_, hole=64)
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, S_), off=off, size=size)
    try:
        rows = rig.rows(list(range(S_))[::-1])
        got, res, name = rig.run(ecglib, masks, rows=rows)
        assert name == am.lane_kernel(p)
        assert res == um.model(masks, k)
        ump.same(got, rig.expect(oracle, masks, rows=rows))
    finally:
        rig.free()


# ------------------------------------------------------- 4. tables that are not one-to-one
def test_old_entry_equal_to_its_new_entry(ctx, ecglib, oracle):
    """Read-only duplicates: cell 0's new entry is its old entry and cell 3's old entry its new
    one -- the delta route gets nothing from them, the recalc route reads the one cell they name."""
    k, p, C_ = 8, 2, 4096
    masks = um.some_masks(k)
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, len(masks)))
    try:
        rows = rig.rows()
        rows[:, k + 0] = rows[:, 0]
        rows[:, 3] = rows[:, k + 3]
        for T in (AUTO, 0, k):
            want = rig.expect(oracle, masks, T, rows)
            got, res, name = rig.run(ecglib, masks, T, rows=rows)
            assert name == ptr_kernel(p)
            assert res == um.model(masks, k)                    # named cells count, whatever they hold
            ump.same(got, want)
    finally:
        rig.free()


def test_all_rows_share_one_old_cell(ctx, ecglib, oracle):
    k, p, C_ = 4, 2, 4096
    masks = um.every_mask(k)
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, len(masks)))
    try:
        rows = rig.rows()
        rows[:, 1] = rows[0, 1]
        for T in (AUTO, 0):
            want = rig.expect(oracle, masks, T, rows)
            assert not np.array_equal(want, rig.expect(oracle, masks, T))
            got, res, name = rig.run(ecglib, masks, T, rows=rows)
            assert name == ptr_kernel(p)
            assert res == um.model(masks, k)
            ump.same(got, want)
    finally:
        rig.free()


def test_old_table_equal_new_table_reencodes_the_old_data(ctx, ecglib, oracle):
    k, p, C_ = 8, 3, 4096 + 16
    masks = um.some_masks(k)
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, len(masks)))
    try:
        rows = rig.rows()
        rows[:, k:2 * k] = rows[:, :k]
        want = rig.expect(oracle, masks, 0, rows)
        assert not np.array_equal(want, rig.img)
        got, res, _ = rig.run(ecglib, masks, 0, rows=rows)
        assert res == um.model(masks, k)
        ump.same(got, want)
        got, res, _ = rig.run(ecglib, masks, k, rows=rows)
        ump.same(got, rig.img)
    finally:
        rig.free()


# -------------------------------------------------------------------- 5. any mask, nothing to do
def test_any_mask_value_is_safe(ctx, ecglib, oracle):
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
                        got, res, name = rig.run(ecglib, masks, flags=flags)
                    finally:
                        ctx.set_launch(0, 0, 0)
                    assert name == (BYTE_KERNEL if variant else ptr_kernel(p))
                    assert res == words, (grid, variant, flags)
                    ump.same(got, want)
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
            assert L.ecg_agg_masks_ptrs(ctx.h, k, p, C__, S__, cells, rig.masks_ptr, rig.result.ptr, 0, 0, None) == 0
            got, res = rig.finish()
            assert res == [0, U64MAX, 0, 0]
            ump.same(got, rig.img)
        got, res, _ = rig.run(ecglib, [0] * S_, 0)              # all-zero masks
        assert res == [0, U64MAX, 0, 0]
        ump.same(got, rig.img)
    finally:
        rig.free()


# ----------------------------------------------------------------------------- 6. table lifetime
def test_the_table_is_copied_before_the_call_returns(ctx, ecglib, oracle):
    k, p, C_, S_ = 8, 2, 64 * 1024, 12
    masks = [m if um.valid(m, k) else 0x5 for m in um.some_masks(k)]
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, S_))
    try:
        want = rig.expect(oracle, masks)
        tab = rig.table()
        arr = (C.c_void_p * len(tab))(*tab)
        rig.upload(masks)
        rig.call(masks, tab=arr)
        arr[:] = [rig.buf.ptr + GUARD] * len(tab)              # garbage: every entry one address
        got, res = rig.finish()
        assert res == um.model(masks, k)
        ump.same(got, want)
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
            rig.call(um.some_masks(rig.k))
        for rig, want in zip(rigs, wants):
            got, res = rig.finish()
            assert res == um.model(um.some_masks(rig.k), rig.k)
            ump.same(got, want)
    finally:
        for rig in rigs:
            rig.free()


# ------------------------------------------------- 7. the device chain over one table
@pytest.mark.parametrize("k,p", [(4, 2), (8, 3)])
def test_checksum_driven_aggregation_over_one_table(ctx, ecglib, oracle, k, p):
    """csum_cells_ptrs over the [S][2k+p] table, memset(masks), csum_mask, agg_masks_ptrs(AUTO),
    csum_updated_ptrs: one stream, one sync.  Some stripes changed in one cell, some in all k; the
    parity of the changed stripes comes out as the oracle's encode of the new data and its
    checksums as those of the cells' final bytes (csum_cells_ptrs again)."""
    C_, S_, htype, n = 8192, 10, ecglib.HASH_CRC32, 2 * k + p
    old, _, par = um.images(oracle, k, p, C_, S_)
    changed = {0: [0], 1: [k - 1], 3: list(range(k)), 4: list(range(k)), 7: [k // 2], 9: list(range(k))}
    new = old.copy()
    for s, js in changed.items():
        for i, j in enumerate(js):
            new[s, j, (s * 131 + i * 977 + (4096 if i % 2 else 0)) % C_] ^= 0x40 >> (i % 7)    # one bit per cell
    want_masks = [sum(1 << j for j in changed.get(s, [])) for s in range(S_)]
    assert {am.route(m, k, am.eff(AUTO, k, p)) for m in want_masks} == {None, "delta", "recalc"}
    rig = PtrRig(ctx, k, p, C_, np.concatenate([old, new, par.transpose(1, 0, 2)], axis=1))
    nch = ecglib.lib().ecg_csum_chunk_count(4096, 1, 0, C_)
    assert nch == 2
    sums, after, upd, result2 = ctx.alloc(4 * S_ * n * nch), ctx.alloc(4 * S_ * n * nch), ctx.alloc(4 * S_ * p * nch), \
        ctx.alloc(32)
    try:
        rig.upload([0] * S_)
        rig.own_masks.fill(0xEE)
        upd.fill(0)
        tab = rig.table()
        ctx.csum_cells_ptrs(htype, 4096, 1, C_, tab, sums.ptr)
        rig.own_masks.fill(0)
        ctx.csum_mask(htype, sums.ptr, sums.ptr + 4 * k * nch, S_, k, nch, n * nch, nch, 0, rig.masks_ptr)
        rig.call([0] * S_, tab=tab)
        assert ecglib.last_kernel() == ptr_kernel(p)
        ctx.csum_updated_ptrs(htype, 4096, 1, k, p, C_, S_, tab, rig.masks_ptr, upd.ptr, p * nch, nch, result2.ptr)
        ctx.csum_cells_ptrs(htype, 4096, 1, C_, tab, after.ptr)
        rig.words = np.array(want_masks, np.uint32)             # what csum_mask is to have written
        got, res = rig.finish()
        assert res == [len(changed), U64MAX, sum(len(js) for js in changed.values()), 0]
        enc = oracle.encode_batch(k, p, C_, S_, new.reshape(-1)).reshape(p, S_, C_)
        want = rig.img.copy()
        for s in changed:
            for r in range(p):
                rig.cell(want, s, 2 * k + r)[:] = enc[r, s]
        assert not np.array_equal(want, rig.img)
        ump.same(got, want)
        ref = after.download().view(np.uint32).reshape(S_, n, nch)[:, 2 * k:]
        got_sums = upd.download().view(np.uint32).reshape(S_, p, nch)
        for s in range(S_):
            assert np.array_equal(got_sums[s], ref[s] if s in changed else np.zeros((p, nch), np.uint32)), s
        assert [int(v) for v in result2.download().view(np.uint64)] == [len(changed), U64MAX, p * len(changed), 0]
    finally:
        for b in (sums, after, upd, result2):
            b.free()
        rig.free()


# ------------------------------------------------------------------------ 8. arguments, stats
def test_argument_errors_on_a_live_context(ctx, ecglib, oracle):
    L = ecglib.lib()
    k, p, C_, S_ = 4, 2, 4096, 9
    rig = PtrRig(ctx, k, p, C_, contents(oracle, k, p, C_, S_))
    n = rig.n
    try:
        rig.upload([1] * S_)
        tab = rig.table()

        def call(cells=tab, masks=rig.masks_ptr, result=rig.result.ptr, T=1, flags=0):
            arr = None if cells is None else (C.c_void_p * len(cells))(*cells)
            return L.ecg_agg_masks_ptrs(ctx.h, k, p, C_, S_, arr, masks, result, T, flags, None)

        assert call(cells=None) == -ecglib.DER_INVAL
        assert L.ecg_strerror() == b"agg_masks_ptrs: NULL cells"
        for i in (0, 7, S_ * n - 1):
            assert call(cells=tab[:i] + [None] + tab[i + 1:]) == -ecglib.DER_INVAL
            assert L.ecg_strerror() == b"agg_masks_ptrs: NULL cell %d" % i, L.ecg_strerror()
        for i in (2 * n + 1, 2 * n + k + 1, 2 * n + 2 * k + 1):        # an old, a new and a parity cell
            cell = tab[i]
            for inside in (cell, cell + C_ - 4, cell - 4 * S_ + 4):
                assert call(masks=inside) == -ecglib.DER_INVAL          # masks inside a cell
                assert b"agg_masks_ptrs: masks overlaps cell" in L.ecg_strerror(), L.ecg_strerror()
            for inside in (cell, cell + C_ - 8, cell - 24):
                assert call(result=inside) == -ecglib.DER_INVAL         # result inside a cell
                assert b"agg_masks_ptrs: result overlaps cell" in L.ecg_strerror(), L.ecg_strerror()
        assert call(masks=tab[5]) == -ecglib.DER_INVAL
        assert L.ecg_strerror() == b"agg_masks_ptrs: masks overlaps cell 5", L.ecg_strerror()
        for flags in (ecglib.UM_PACKED, ecglib.UM_PACKED | ecglib.RM_SPARSE):
            assert call(flags=flags) == -ecglib.DER_INVAL
            assert b"agg_masks_ptrs: ECG_UM_PACKED" in L.ecg_strerror()
        assert call(T=k + 1) == -ecglib.DER_INVAL
        assert L.ecg_strerror().startswith(b"agg_masks_ptrs: recalc_above=5")
        got, _ = rig.finish()
        ump.same(got, rig.img)                                  # none of the calls above wrote a cell
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
