"""ecg_verify_ptrs, ecg_repair_ptrs and ecg_scrub_ptrs on the GPU: the parity scrub with the
cells of every stripe given by address.  The cells live where tests.test_gpu_recover_masks_ptrs
PtrRig puts them (a seeded permutation, 48-byte 0xA5 gaps, guards), so a cell read or written
anywhere but where it belongs shows up; every comparison is exact and covers the whole
allocation.  The expected status words come from tests.test_gpu_verify's derivations and its
model_status (CPU, numpy), and every run is also held against a strided twin: ecg_verify /
ecg_repair on the same cells gathered into one image [S][k+p][C], scattered back."""
import ctypes as C

import numpy as np
import pytest

from tests import test_gpu_recover_masks as rm
from tests import test_gpu_repair as rp
from tests import test_gpu_verify as vg
from tests.test_gpu_recover_masks_ptrs import PtrRig, same

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (4, 2), (8, 2), (16, 2), (8, 3), (5, 2)]
CELLS = [16, 4096, 8192 + 48]       # one lane has work; one full column; a lane-masked last column
S = 5
U64MAX = rm.U64MAX
VERIFY_BYTE, REPAIR_BYTE = "ecg_verify_ptr_byte_kernel", "ecg_repair_ptr_byte_kernel"


def verify_kernel(k, p):
    return f"ecg_verify_ptr_kernel<{k},{p}>" if k in (2, 4, 8, 16) and p in (1, 2, 3) else "ecg_verify_ptr_kernel<0,0>"


def repair_kernel(k):
    return f"ecg_repair_ptr_kernel<{k if k in (2, 4, 8, 16) else 0}>"


def clean_word(k):
    return ((1 << k) - 1) << 8


def words(buf, dtype=np.uint64):
    return [int(v) for v in buf.download().view(dtype)]


class Scrub:
    """A PtrRig with the status words and result buffers of a scrub, and a strided twin of its
    cells on the device ([S][k+p][C], kept equal to the rig by poke / upload)."""

    def __init__(self, ctx, k, p, C_, cells, **rig_args):
        self.ctx, self.k, self.p, self.C, self.S, self.n = ctx, k, p, C_, cells.shape[0], k + p
        self.rig = PtrRig(ctx, k, p, C_, cells, **rig_args)
        self.clean = self.rig.img.copy()
        self.status = [ctx.alloc(4 * self.S) for _ in range(2)]
        self.result = [ctx.alloc(32) for _ in range(4)]
        self.twin = ctx.alloc(self.S * self.n * C_)
        self.tstatus, self.tresult = ctx.alloc(4 * self.S), [ctx.alloc(32), ctx.alloc(32)]
        self.geo = (k, p, C_, self.S)
        self.upload()

    def upload(self):
        """The host image (self.rig.img) to the device, and its cells into the twin."""
        self.rig.buf.upload(self.rig.img)
        self.twin.upload(np.ascontiguousarray(self.rig.gather(self.rig.img)).reshape(-1))

    def poke(self, s, c, i, x):
        """XOR x into byte i of cell c of stripe s: host image, device and twin."""
        cell = self.rig.cell(self.rig.img, s, c)
        cell[i] ^= x
        byte = np.array([cell[i]], dtype=np.uint8)
        self.rig.buf.upload(byte, int(self.rig.off[s, c]) + i)
        self.twin.upload(byte, (s * self.n + c) * self.C + i)

    def put(self, s, c, data):
        self.rig.cell(self.rig.img, s, c)[:] = data
        self.rig.buf.upload(np.ascontiguousarray(data), int(self.rig.off[s, c]))
        self.twin.upload(np.ascontiguousarray(data), (s * self.n + c) * self.C)

    def restore(self):
        self.rig.img[:] = self.clean
        self.upload()

    def twin_args(self):
        n, C_ = self.n, self.C
        return (self.twin.ptr, n * C_, self.twin.ptr + self.k * C_, C_, n * C_)

    def twin_verify(self):
        """ecg_verify on the gathered image -> (status words, result words)."""
        self.tstatus.fill(0xEE)
        self.tresult[0].fill(0xEE)
        self.ctx.verify(*self.geo, *self.twin_args(), self.tstatus.ptr, self.tresult[0].ptr)
        self.ctx.sync()
        return words(self.tstatus, np.uint32), words(self.tresult[0])

    def twin_repair(self, status=None):
        """ecg_repair on the gathered image with the twin's status words (or `status`) -> (result
        words, the rig's image as it is on the host with the twin's cells scattered back)."""
        if status is not None:
            self.tstatus.upload(np.array(status, dtype=np.uint32).view(np.uint8))
        self.tresult[1].fill(0xEE)
        self.ctx.repair(*self.geo, *self.twin_args(), self.tstatus.ptr, self.tresult[1].ptr)
        self.ctx.sync()
        want = self.rig.img.copy()
        self.rig.scatter(want, self.twin.download().reshape(self.S, self.n, self.C))
        return words(self.tresult[1]), want

    def verify(self, ecglib, table=None, i=0):
        """One ecg_verify_ptrs, one sync -> (status words, result words, kernel)."""
        self.status[i].fill(0xEE)
        self.result[i].fill(0xEE)
        self.ctx.verify_ptrs(*self.geo, self.rig.table() if table is None else table, self.status[i].ptr,
                             self.result[i].ptr)
        name = ecglib.last_kernel()
        self.ctx.sync()
        return words(self.status[i], np.uint32), words(self.result[i]), name

    def free(self):
        self.rig.free()
        for b in self.status + self.result + self.tresult + [self.twin, self.tstatus]:
            b.free()


def check(ecglib, sc, bad, kernel=None, table=None, order=None):
    """bad: {stripe: (rows, candidate bits, cell or -2)}, derived by the caller from what it
    injected; status, result and verify_cell equal them and the strided twin's."""
    k, p = sc.k, sc.p
    status, result, name = sc.verify(ecglib, table)
    assert name == (kernel or verify_kernel(k, p)), name
    want = [clean_word(k)] * sc.S
    for s, (rows, cand, _) in bad.items():
        want[s] = rows | (cand << 8)
    tstatus, tresult = sc.twin_verify()
    assert want == tstatus and [int(v) for v in np.array(want)[order if order is not None else slice(None)]] == status, \
        ([hex(v) for v in status], [hex(v) for v in want], [hex(v) for v in tstatus])
    for s in range(sc.S):
        assert ecglib.verify_cell(want[s], k, p) == (bad[s][2] if s in bad else -1), s
    one = sum(1 for v in bad.values() if v[2] >= 0)
    rows_of = sorted(s if order is None else list(order).index(s) for s in bad)      # their table rows
    assert result == [len(bad), rows_of[0] if bad else U64MAX, one, len(bad) - one]
    if order is None:
        assert result == tresult


@pytest.fixture(params=[(k, p, C_) for k, p in SHAPES for C_ in CELLS], ids=lambda t: f"{t[0]}p{t[1]}-{t[2]}")
def sc(request, ctx, oracle):
    k, p, C_ = request.param
    s = Scrub(ctx, k, p, C_, rm.codewords(oracle, k, p, C_, S))
    yield s
    same(s.rig.buf.download(), s.rig.img)       # whatever the test did, the device holds what it expects
    s.free()


def offsets(C_):
    return [o for o in vg.offsets(C_) if o < C_]


# ---------------------------------------------------------------------- 1. verify
def test_clean_and_read_only(ecglib, sc):
    check(ecglib, sc, {})
    same(sc.rig.buf.download(), sc.clean)       # cells, gaps, slack and guards


def test_one_byte_in_each_data_cell(ecglib, sc):
    k, p = sc.k, sc.p
    n = 0
    for j in range(k):
        for off in offsets(sc.C):
            s = n % sc.S
            n += 1
            x = 1 + (n * 37) % 255
            sc.poke(s, j, off, x)
            check(ecglib, sc, {s: vg.data_flip(k, p, j)})
            sc.poke(s, j, off, x)
    same(sc.rig.buf.download(), sc.clean)       # verify wrote nothing, the flips were put back


def test_one_byte_in_each_parity_row(ecglib, sc):
    k, p = sc.k, sc.p
    for r in range(p):
        for n, off in enumerate(offsets(sc.C)):
            s = (n + r) % sc.S
            sc.poke(s, k + r, off, 0x80 >> (n % 8))
            check(ecglib, sc, {s: vg.parity_flip(k, p, r)})
            sc.poke(s, k + r, off, 0x80 >> (n % 8))


def test_whole_data_cell_replaced(ecglib, oracle, sc):
    """Every block of the stripe takes the dirty path and ANDs into the same word."""
    k, p = sc.k, sc.p
    j, s = k - 1, 2
    junk = np.random.default_rng(99).integers(0, 256, sc.C, dtype=np.uint8)
    cells = sc.rig.gather(sc.clean)[s]
    keep = cells[j].copy()
    stripe = cells.copy()
    stripe[j] = junk
    rows, cand = vg.model_status(oracle, k, p, stripe[:k], stripe[k:])
    want = vg.data_flip(k, p, j)
    assert (rows, cand) == want[:2] or p == 1       # the model agrees with the derivation
    sc.put(s, j, junk)
    check(ecglib, sc, {s: want})
    sc.put(s, j, keep)


def test_two_cells_wrong(ecglib, sc):
    k, p = sc.k, sc.p
    far = 4096 + 7 if sc.C > 4096 else (2000 if sc.C > 2000 else sc.C - 1)
    flips = [(3, 0, 5, 0x11), (3, k - 1, far, 0xC3)]
    for f in flips:
        sc.poke(*f)
    check(ecglib, sc, {3: vg.unattributable(k, p)})
    for f in flips:
        sc.poke(*f)
    flips = [(4, k, 9, 0x40)] if p < 2 else [(4, k, 9, 0x40), (4, k + 1, sc.C - 3, 0x02)]
    for f in flips:
        sc.poke(*f)
    check(ecglib, sc, {4: vg.unattributable(k, p, rows=None if p < 2 else 0b11)})
    for f in flips:
        sc.poke(*f)


def several(sc):
    k, p, C_ = sc.k, sc.p, sc.C
    flips = [(1, k - 1, C_ - 1, 0x7f), (3, k + p - 1, 0, 0x01), (4, 0, 1, 0x10), (4, 1, C_ // 2, 0x20)]
    bad = {1: vg.data_flip(k, p, k - 1), 3: vg.parity_flip(k, p, p - 1), 4: vg.unattributable(k, p)}
    return flips, bad


def test_several_bad_stripes(ecglib, sc):
    flips, bad = several(sc)
    for f in flips:
        sc.poke(*f)
    check(ecglib, sc, bad)
    for f in flips:
        sc.poke(*f)


# ------------------------------------------------------------- 2. table variations
@pytest.mark.parametrize("k,p", [(4, 2), (5, 2), (8, 3)])
def test_status_belongs_to_the_table_row(ctx, ecglib, oracle, k, p):
    """Table rows in a permuted stripe order: status[s] describes table row s."""
    sc = Scrub(ctx, k, p, 4096, rm.codewords(oracle, k, p, 4096, S))
    try:
        flips, bad = several(sc)
        for f in flips:
            sc.poke(*f)
        order = [3, 0, 4, 2, 1]
        check(ecglib, sc, bad, table=sc.rig.table(order), order=order)
    finally:
        sc.free()


def scrub_expect(sc):
    """`several` applied: -> (flips, bad, image a correct repair leaves, the four repair words)."""
    k, p = sc.k, sc.p
    flips, bad = several(sc)
    for f in flips:
        sc.poke(*f)
    want = sc.clean.copy()
    left = [s for s, v in bad.items() if v[2] < 0]
    for s in left:
        for c in range(sc.n):
            sc.rig.cell(want, s, c)[:] = sc.rig.cell(sc.rig.img, s, c)
    fixed = [v[2] for v in bad.values() if v[2] >= 0]
    return bad, want, left, [len(fixed), min(left) if left else U64MAX, sum(1 for c in fixed if c < k), len(left)]


def test_the_table_is_copied_before_the_call_returns(ctx, ecglib, oracle):
    """The caller's array is overwritten right after each call and before the sync -- with the
    table's rows rotated by one, so that a late reader would put every status word and every
    repair one stripe off: wrong answers, never a wild address."""
    k, p, C_ = 8, 2, 8192 + 48
    sc = Scrub(ctx, k, p, C_, rm.codewords(oracle, k, p, C_, S))
    try:
        bad, want, left, rwords = scrub_expect(sc)
        tab = sc.rig.table()
        arr = (C.c_void_p * len(tab))(*tab)
        junk = sc.rig.table([(s + 1) % S for s in range(S)])
        for b in sc.status + sc.result:
            b.fill(0xEE)
        ctx.verify_ptrs(*sc.geo, arr, sc.status[0].ptr, sc.result[0].ptr)
        arr[:] = junk
        arr[:] = tab
        ctx.repair_ptrs(*sc.geo, arr, sc.status[0].ptr, sc.result[1].ptr)
        arr[:] = junk
        ctx.sync()
        st0 = words(sc.status[0], np.uint32)
        assert st0 == [bad[s][0] | bad[s][1] << 8 if s in bad else clean_word(k) for s in range(S)]
        assert words(sc.result[1]) == rwords
        same(sc.rig.buf.download(), want)
        sc.restore()
        scrub_expect(sc)
        arr[:] = tab
        ctx.scrub_ptrs(*sc.geo, arr, sc.status[1].ptr, sc.result[2].ptr, sc.result[3].ptr)
        arr[:] = junk
        ctx.sync()
        assert words(sc.status[1], np.uint32) == st0
        assert words(sc.result[2]) == words(sc.result[0]) and words(sc.result[3]) == rwords
        same(sc.rig.buf.download(), want)
    finally:
        sc.free()


def scrub_both_ways(ecglib, sc, vname, rname, table=None):
    """`several`, then verify_ptrs + repair_ptrs with no sync in between, then the same through
    scrub_ptrs: status, results, bytes and kernel names as derived and as the strided twin's."""
    ctx, k, p = sc.ctx, sc.k, sc.p
    tab = sc.rig.table() if table is None else table
    for mode in ("pair", "scrub"):
        sc.restore()
        bad, want, left, rwords = scrub_expect(sc)
        tstatus, tverify = sc.twin_verify()
        trepair, twant = sc.twin_repair()
        same(twant, want)
        assert trepair == rwords
        for b in sc.status + sc.result:
            b.fill(0xEE)
        if mode == "pair":
            ctx.verify_ptrs(*sc.geo, tab, sc.status[0].ptr, sc.result[0].ptr)
            assert ecglib.last_kernel() == vname, ecglib.last_kernel()
            ctx.repair_ptrs(*sc.geo, tab, sc.status[0].ptr, sc.result[1].ptr)
        else:
            ctx.scrub_ptrs(*sc.geo, tab, sc.status[0].ptr, sc.result[0].ptr, sc.result[1].ptr)
        assert ecglib.last_kernel() == rname, ecglib.last_kernel()
        ctx.verify_ptrs(*sc.geo, tab, sc.status[1].ptr, sc.result[2].ptr)
        ctx.sync()
        st0 = words(sc.status[0], np.uint32)
        assert st0 == tstatus == [bad[s][0] | bad[s][1] << 8 if s in bad else clean_word(k) for s in range(sc.S)]
        assert words(sc.result[0]) == tverify
        assert words(sc.result[1]) == rwords, mode
        same(sc.rig.buf.download(), want)
        sc.rig.img[:] = want
        st1 = words(sc.status[1], np.uint32)
        assert [s for s, w in enumerate(st1) if ecglib.verify_cell(w, k, p) != -1] == left
        assert [st1[s] for s in left] == [st0[s] for s in left]
        assert words(sc.result[2]) == [len(left), min(left) if left else U64MAX, 0, len(left)]


@pytest.mark.parametrize("k,p", [(2, 1), (4, 2), (8, 3), (5, 2)])
def test_one_misaligned_entry_sends_the_whole_launch_to_the_byte_kernels(ctx, ecglib, oracle, k, p):
    C_ = 4099
    sc = Scrub(ctx, k, p, C_, rm.codewords(oracle, k, p, C_, S), skew=lambda s, c: 1 if (s, c) == (2, 1) else 0)
    try:
        check(ecglib, sc, {}, kernel=VERIFY_BYTE)
        for j, off in ((0, 0), (k - 1, 4098), (1, 4096)):
            sc.poke(2, j, off, 0x21)
            check(ecglib, sc, {2: vg.data_flip(k, p, j)}, kernel=VERIFY_BYTE)
            sc.poke(2, j, off, 0x21)
        scrub_both_ways(ecglib, sc, VERIFY_BYTE, REPAIR_BYTE)
    finally:
        sc.free()


@pytest.mark.parametrize("k,p", [(4, 2), (16, 2), (5, 2)])
def test_variant_2_equals_the_lane_kernels(ctx, ecglib, oracle, k, p):
    C_ = 8192 + 48
    sc = Scrub(ctx, k, p, C_, rm.codewords(oracle, k, p, C_, S))
    try:
        scrub_both_ways(ecglib, sc, verify_kernel(k, p), repair_kernel(k))
        ctx.set_launch(0, 0, 2)
        try:
            scrub_both_ways(ecglib, sc, VERIFY_BYTE, REPAIR_BYTE)      # the same derived status, result and bytes
        finally:
            ctx.set_launch(0, 0, 0)
    finally:
        sc.free()


@pytest.mark.parametrize("k,p", [(4, 2), (5, 2), (8, 3)])
def test_affine_table_is_the_strided_calls(ctx, ecglib, oracle, k, p):
    C_ = 4096
    sc = Scrub(ctx, k, p, C_, rm.codewords(oracle, k, p, C_, S), permute=False, gap=0)
    try:
        scrub_both_ways(ecglib, sc, vg.kernel_name(k, p), rp.kernel_name(k))
        order = [0, 3, 2, 1, 4]                                         # two rows exchanged: no stride
        sc.restore()
        flips, bad = several(sc)
        for f in flips:
            sc.poke(*f)
        check(ecglib, sc, bad, table=sc.rig.table(order), order=order)
    finally:
        sc.free()


def test_status_in_a_gap_between_stripes(ctx, ecglib, oracle):
    """A strided table whose status words lie between two stripes: ecg_repair refuses such
    operands, so the answers must come out the same whichever route takes the calls."""
    k, p, C_ = 4, 2, 4096
    n, stride = k + p, (k + p) * 4096 + 256
    cw = rm.codewords(oracle, k, p, C_, S)
    img = np.full(S * stride, 0xA5, dtype=np.uint8)
    bad = {1: (k - 1, C_ - 1, 0x7f), 3: (k + 1, 0, 0x01)}
    for s in range(S):
        img[s * stride:s * stride + n * C_] = cw[s].reshape(-1)
    want = img.copy()
    for s, (c, i, x) in bad.items():
        img[s * stride + c * C_ + i] ^= x
    buf, res = ctx.alloc(img.size), [ctx.alloc(32) for _ in range(4)]
    try:
        tab = [buf.ptr + s * stride + c * C_ for s in range(S) for c in range(n)]
        status = buf.ptr + n * C_ + 16                                  # in stripe 0's gap
        expect = [clean_word(k)] * S
        expect[1], expect[3] = rp.attributing(k, p, k - 1), rp.attributing(k, p, k + 1)
        for mode in ("pair", "scrub"):
            buf.upload(img)
            if mode == "pair":
                ctx.verify_ptrs(k, p, C_, S, tab, status, res[0].ptr)
                ctx.repair_ptrs(k, p, C_, S, tab, status, res[1].ptr)
            else:
                ctx.scrub_ptrs(k, p, C_, S, tab, status, res[0].ptr, res[1].ptr)
            ctx.sync()
            got = buf.download()
            assert [int(v) for v in got[n * C_ + 16:n * C_ + 16 + 4 * S].view(np.uint32)] == expect
            assert words(res[0]) == [2, 1, 2, 0] and words(res[1]) == [2, U64MAX, 1, 0]
            got[n * C_ + 16:n * C_ + 16 + 4 * S] = 0xA5
            same(got, want)
    finally:
        for b in [buf] + res:
            b.free()


# --------------------------------------------------------------------- 3. striding
def test_many_stripes(ctx, ecglib, oracle):
    """More stripes than a grid dimension holds: the verify kernel's stripe loop strides."""
    k, p, C_, S_ = 2, 1, 64, 70000
    sc = Scrub(ctx, k, p, C_, rm.codewords(oracle, k, p, C_, S_))
    try:
        tab = sc.rig.table()
        status, result, name = sc.verify(ecglib, tab)
        assert name == "ecg_verify_ptr_kernel<2,1>"
        assert result == [0, U64MAX, 0, 0] and set(status) == {clean_word(k)}
        sc.poke(S_ - 1, 1, 63, 0x80)
        status, result, _ = sc.verify(ecglib, tab)
        assert result == [1, S_ - 1, 0, 1]
        assert status[S_ - 1] == 1 | (0b11 << 8) and set(status[:S_ - 1]) == {clean_word(k)}
        assert (status, result) == sc.twin_verify()
        sc.poke(S_ - 1, 1, 63, 0x80)
    finally:
        sc.free()


@pytest.mark.parametrize("mode", ["pair", "scrub"])
def test_repair_walks_groups_of_64_stripes(ctx, ecglib, oracle, mode):
    """130 stripes are two whole groups and a partial one; bad stripes at their edges."""
    k, p, C_, S_ = 4, 2, 4096, 130
    sc = Scrub(ctx, k, p, C_, rm.codewords(oracle, k, p, C_, S_))
    try:
        cellof = {0: 0, 63: k + 1, 64: k - 1, 129: 2}
        for s, c in cellof.items():
            sc.poke(s, c, (s * 37) % C_, 0x01 + s)
        tab = sc.rig.table()
        if mode == "pair":
            ctx.verify_ptrs(*sc.geo, tab, sc.status[0].ptr, sc.result[0].ptr)
            ctx.repair_ptrs(*sc.geo, tab, sc.status[0].ptr, sc.result[1].ptr)
        else:
            ctx.scrub_ptrs(*sc.geo, tab, sc.status[0].ptr, sc.result[0].ptr, sc.result[1].ptr)
        assert ecglib.last_kernel() == repair_kernel(k)
        ctx.sync()
        st0 = words(sc.status[0], np.uint32)
        assert st0 == [rp.attributing(k, p, cellof[s]) if s in cellof else clean_word(k) for s in range(S_)]
        assert st0 == sc.twin_verify()[0]
        assert words(sc.result[0]) == [4, 0, 4, 0]
        assert words(sc.result[1]) == [4, U64MAX, 3, 0]
        same(sc.rig.buf.download(), sc.clean)
        sc.rig.img[:] = sc.clean
    finally:
        sc.free()


# ------------------------------------------------------------ 4. repair and scrub
@pytest.mark.parametrize("C_", CELLS)
@pytest.mark.parametrize("k,p", SHAPES)
def test_verify_then_repair_and_scrub(ctx, ecglib, oracle, k, p, C_):
    sc = Scrub(ctx, k, p, C_, rm.codewords(oracle, k, p, C_, S))
    try:
        scrub_both_ways(ecglib, sc, verify_kernel(k, p), repair_kernel(k))
    finally:
        sc.free()


@pytest.mark.parametrize("C_", CELLS)
@pytest.mark.parametrize("k,p", [kp for kp in SHAPES if kp[1] >= 2])
def test_repair_identical_to_the_strided_twin_on_non_codewords(ctx, ecglib, k, p, C_):
    """Random, inconsistent stripes, one per cell index and status words written by hand: the
    bytes depend on which sources are read; then what a scrub makes of them, miscorrection
    included."""
    sc = Scrub(ctx, k, p, C_, rm.random_cells(k, p, C_, k + p))
    try:
        status = [rp.attributing(k, p, s) for s in range(k + p)]
        twords, want = sc.twin_repair(status)
        assert twords == [k + p, U64MAX, k, 0] and not np.array_equal(want, sc.rig.img)
        sc.status[0].upload(np.array(status, dtype=np.uint32).view(np.uint8))
        sc.result[1].fill(0xEE)
        ctx.repair_ptrs(*sc.geo, sc.rig.table(), sc.status[0].ptr, sc.result[1].ptr)
        assert ecglib.last_kernel() == repair_kernel(k)
        ctx.sync()
        assert words(sc.status[0], np.uint32) == status                 # read only
        assert words(sc.result[1]) == twords
        same(sc.rig.buf.download(), want)
        # the scrub of the same stripes: whatever the check makes of them, the twin's bytes
        sc.upload()
        tstatus, tverify = sc.twin_verify()
        twords, want = sc.twin_repair()
        ctx.scrub_ptrs(*sc.geo, sc.rig.table(), sc.status[1].ptr, sc.result[2].ptr, sc.result[3].ptr)
        ctx.sync()
        assert words(sc.status[1], np.uint32) == tstatus
        assert words(sc.result[2]) == tverify and words(sc.result[3]) == twords
        same(sc.rig.buf.download(), want)
    finally:
        sc.free()


@pytest.mark.parametrize("k", [4, 8])
def test_miscorrection_equals_the_strided_twin(ctx, ecglib, oracle, k):
    """p = 2: cells 0 and 1 wrong at one byte by amounts that add up to the syndrome of cell 2
    alone.  The scrub rewrites cell 2 to another codeword, exactly as the strided calls do."""
    from oracle.gf_np import MUL

    p, C_, s, off, c = 2, 4096, 2, 100, 2
    g = oracle.cauchy1(k, p)[k:]
    pair = [(ea, eb) for ea in range(1, 256) for eb in range(1, 256)
            if all(int(MUL[g[r][0]][ea]) ^ int(MUL[g[r][1]][eb]) == int(g[r][c]) for r in range(p))]
    assert pair
    sc = Scrub(ctx, k, p, C_, rm.codewords(oracle, k, p, C_, S))
    try:
        sc.poke(s, 0, off, pair[0][0])
        sc.poke(s, 1, off, pair[0][1])
        stripe = sc.rig.gather(sc.rig.img)[s]
        assert vg.model_status(oracle, k, p, stripe[:k], stripe[k:]) == vg.data_flip(k, p, c)[:2]
        check(ecglib, sc, {s: vg.data_flip(k, p, c)})
        tstatus, tverify = sc.twin_verify()
        twords, want = sc.twin_repair()
        assert twords == [1, U64MAX, 1, 0] and want[sc.rig.off[s, c] + off] == sc.clean[sc.rig.off[s, c] + off] ^ 1
        ctx.scrub_ptrs(*sc.geo, sc.rig.table(), sc.status[0].ptr, sc.result[0].ptr, sc.result[1].ptr)
        ctx.verify_ptrs(*sc.geo, sc.rig.table(), sc.status[1].ptr, sc.result[2].ptr)
        ctx.sync()
        assert words(sc.status[0], np.uint32) == tstatus and words(sc.result[1]) == twords
        same(sc.rig.buf.download(), want)
        assert words(sc.result[2]) == [0, U64MAX, 0, 0]                 # a codeword again, not the one written
    finally:
        sc.free()


@pytest.mark.parametrize("k,p", SHAPES)
def test_any_status_word_is_safe(ctx, ecglib, k, p):
    """Hand-written words with candidate bits at or above k or row bits at or above p, on
    inconsistent stripes, so that any cell written would change: none may be, and they are
    counted as the strided call counts them."""
    allrows, allcand, st = (1 << p) - 1, (1 << k) - 1, rp.st
    status = [0xFFFFFFFF, st(1 << p, 0), st(0x80, 1), st(allrows | (1 << p), 1),
              st(allrows, 1 << k) if k < 16 else st(allrows, 0) | (1 << 24),
              st(allrows, 0xffff & ~allcand), 0xFFFFFF00 | allrows, st(0, 0), st(0, allcand), 0xFFFFFF00,
              st(allrows, 0b11), st(allrows, allcand), st(allrows, 0)]
    sc = Scrub(ctx, k, p, 8192 + 48, rm.random_cells(k, p, 8192 + 48, len(status)))
    try:
        cells = [ecglib.verify_cell(w, k, p) for w in status]
        assert set(cells) == {-1, -2}
        left = [s for s, c in enumerate(cells) if c == -2]
        twords, want = sc.twin_repair(status)
        assert twords == [0, min(left), 0, len(left)]
        sc.status[0].upload(np.array(status, dtype=np.uint32).view(np.uint8))
        for variant in (0, 2):
            ctx.set_launch(0, 0, variant)
            try:
                sc.result[1].fill(0xEE)
                ctx.repair_ptrs(*sc.geo, sc.rig.table(), sc.status[0].ptr, sc.result[1].ptr)
                ctx.sync()
            finally:
                ctx.set_launch(0, 0, 0)
            assert words(sc.result[1]) == twords
            same(sc.rig.buf.download(), sc.rig.img)
        same(want, sc.rig.img)
    finally:
        sc.free()


# -------------------------------------------------------- 5. arguments and counters
def test_argument_validation(ctx, ecglib, oracle):
    L = ecglib.lib()
    k, p, C_ = 4, 2, 4096
    n = k + p
    sc = Scrub(ctx, k, p, C_, rm.codewords(oracle, k, p, C_, S))
    try:
        tab = sc.rig.table()
        stw, res, res2 = sc.status[0].ptr, sc.result[0].ptr, sc.result[1].ptr
        sc.status[0].upload(np.full(S, clean_word(k), dtype=np.uint32).view(np.uint8))

        def call(fn, C__=C_, S__=S, cells=tab, status=stw, result=res, result2=res2):
            arr = None if cells is None else (C.c_void_p * len(cells))(*cells)
            if fn == "scrub_ptrs":
                return L.ecg_scrub_ptrs(ctx.h, k, p, C__, S__, arr, status, result, result2, None)
            return getattr(L, "ecg_" + fn)(ctx.h, k, p, C__, S__, arr, status, result, None)

        for fn in ("verify_ptrs", "repair_ptrs", "scrub_ptrs"):
            assert call(fn, cells=None) == -ecglib.DER_INVAL
            assert L.ecg_strerror() == b"%s: NULL cells" % fn.encode(), L.ecg_strerror()
            for i in (0, 7, S * n - 1):
                assert call(fn, cells=tab[:i] + [None] + tab[i + 1:]) == -ecglib.DER_INVAL
                assert L.ecg_strerror() == b"%s: NULL cell %d" % (fn.encode(), i), L.ecg_strerror()
            cell = tab[2 * n + 3]
            for inside in (cell, cell + C_ - 4, cell - 4 * S + 4):
                assert call(fn, status=inside) == -ecglib.DER_INVAL
                assert b"%s: status overlaps cell" % fn.encode() in L.ecg_strerror(), L.ecg_strerror()
            for inside in (cell, cell + C_ - 8, cell - 24):
                assert call(fn, result=inside) == -ecglib.DER_INVAL
                assert b"result overlaps cell" in L.ecg_strerror() and L.ecg_strerror().startswith(fn.encode())
            # an empty batch presets the result(s) and touches nothing else; empty cells preset
            # the status words of the calls that write them as well
            for kw, st_preset in (({"S__": 0, "cells": None, "status": None}, False), ({"C__": 0}, fn != "repair_ptrs")):
                for b in (sc.result[0], sc.result[1], sc.status[0]):
                    b.fill(0xEE)
                assert call(fn, **kw) == 0
                ctx.sync()
                assert words(sc.result[0]) == [0, U64MAX, 0, 0]
                assert words(sc.result[1]) == ([0, U64MAX, 0, 0] if fn == "scrub_ptrs" else [0xEEEEEEEEEEEEEEEE] * 4)
                assert words(sc.status[0], np.uint32) == [clean_word(k) if st_preset else 0xEEEEEEEE] * S
        assert call("scrub_ptrs", result2=tab[5] + 64) == -ecglib.DER_INVAL
        assert b"scrub_ptrs: repair_result overlaps cell 5" == L.ecg_strerror(), L.ecg_strerror()
        same(sc.rig.buf.download(), sc.clean)                           # none of the calls above wrote a cell
    finally:
        sc.free()


def test_counts_launches(ctx, ecglib, oracle):
    sc = Scrub(ctx, 4, 2, 4096, rm.codewords(oracle, 4, 2, 4096, S))
    try:
        tab = sc.rig.table()
        sc.verify(ecglib, tab)
        ctx.repair_ptrs(*sc.geo, tab, sc.status[0].ptr, sc.result[1].ptr)           # builds the row tables
        ctx.sync()
        at = [ctx.stats()]
        sc.verify(ecglib, tab)
        assert ecglib.last_kernel() == verify_kernel(4, 2)
        at.append(ctx.stats())
        ctx.repair_ptrs(*sc.geo, tab, sc.status[0].ptr, sc.result[1].ptr)
        assert ecglib.last_kernel() == repair_kernel(4)
        at.append(ctx.stats())
        ctx.scrub_ptrs(*sc.geo, tab, sc.status[0].ptr, sc.result[0].ptr, sc.result[1].ptr)
        assert ecglib.last_kernel() == repair_kernel(4)
        at.append(ctx.stats())
        ctx.sync()
        assert [b["launches"] - a["launches"] for a, b in zip(at, at[1:])] == [2, 1, 3]
        assert at[-1]["recover_stripes"] == at[0]["recover_stripes"]
    finally:
        sc.free()
