"""ecg_repair on the GPU: stripes from the CPU oracle, cells corrupted, then
verify -> repair -> verify on one stream with one synchronisation at the end.
Every comparison is exact and covers the whole allocation: each image lies
between 0xA5 guard bytes and is followed by 0xA5 slack of 16 cells + 8 parity
rows, so a cell index the kernel failed to mask shows up as changed bytes.

Shapes: a 16-byte cell, one 4 KiB column, a lane-masked last column
(8192 + 48) and more columns than blocks per stripe (128 KiB), in the client
layout (data [S][k][C], parity [p][S][C]) and the recovery layout
([S][k+p][C]); the specialised kernels, the runtime-shaped one (k = 5), the
byte-granular one, and p = 1, where nothing is ever attributable."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(4, 2), (8, 2), (16, 2), (8, 3), (5, 2), (2, 1)]
CELLS = [16, 4096, 8192 + 48, 128 * 1024]
LAYOUTS = ["client", "recov"]
U64MAX = (1 << 64) - 1
GUARD = 256                 # keeps the image 16-byte aligned inside its (256-byte aligned) allocation
FILL = 0xA5

_REF = {}


def reference(oracle, k, p, C_, S_):
    """(data [S][k][C], parity [p][S][C]) of the oracle, computed once per shape and never modified."""
    key = (k, p, C_, S_)
    if key not in _REF:
        data = np.random.default_rng(k * 1000003 + p * 101 + C_ + S_).integers(0, 256, (S_, k, C_), dtype=np.uint8)
        par = oracle.encode_batch(k, p, C_, S_, data.reshape(-1)).reshape(p, S_, C_)
        data.setflags(write=False)
        par.setflags(write=False)
        _REF[key] = (data, par)
    return _REF[key]


def st(rows, cand):
    """A status word: rows in bits 0-7, candidate data cells in bits 8-23."""
    return (rows & 0xff) | ((cand & 0xffff) << 8)


def attributing(k, p, c):
    """The status word ecg_verify leaves for a stripe whose cell c alone is wrong."""
    return st((1 << p) - 1, 1 << c) if c < k else st(1 << (c - k), 0)


def kernel_name(k):
    return f"ecg_repair_kernel<{k}>" if k in (2, 4, 8, 16) else "ecg_repair_kernel<0>"


class Rig:
    """Host and device copies of S stripes in one of the two layouts: cells 0..k-1 data, k..k+p-1
    parity.  self.img: the host copy of each allocation (guards and slack included), which the
    tests edit and upload(), and compare whole with download().  skew: byte offset of the images
    from their 16-byte aligned place.  codeword=False: random parity, so no stripe is consistent."""

    def __init__(self, ctx, oracle, k, p, C_, layout, S_=None, skew=0, codeword=True):
        S_ = k + p + 3 if S_ is None else S_
        self.ctx, self.k, self.p, self.C, self.S, self.layout, self.skew = ctx, k, p, C_, S_, layout, skew
        data, par = reference(oracle, k, p, C_, S_)
        if not codeword:
            par = np.random.default_rng(7 * k + p).integers(0, 256, par.shape, dtype=np.uint8)
        self.base = GUARD + skew
        if layout == "client":
            sizes = {"d": S_ * k * C_ + 16 * C_, "p": p * S_ * C_ + 8 * S_ * C_}
        else:
            sizes = {"d": S_ * (k + p) * C_ + 24 * C_}
        self.img = {n: np.full(self.base + sz + GUARD, FILL, dtype=np.uint8) for n, sz in sizes.items()}
        self.buf = {n: ctx.alloc(a.size) for n, a in self.img.items()}
        for s in range(S_):
            for c in range(k + p):
                self.cell(self.img, s, c)[:] = data[s, c] if c < k else par[c - k, s]
        d = self.buf["d"].ptr + self.base
        if layout == "client":
            self.args = (d, k * C_, self.buf["p"].ptr + self.base, S_ * C_, C_)
        else:
            self.args = (d, (k + p) * C_, d + k * C_, C_, (k + p) * C_)
        self.status = [ctx.alloc(4 * S_), ctx.alloc(4 * S_)]
        self.result = [ctx.alloc(32) for _ in range(3)]          # verify, repair, verify

    def cell(self, img, s, c):
        """The bytes of cell c of stripe s inside the host images `img` (a view)."""
        k, p, C_, S_ = self.k, self.p, self.C, self.S
        if self.layout == "recov":
            name, off = "d", (s * (k + p) + c) * C_
        elif c < k:
            name, off = "d", (s * k + c) * C_
        else:
            name, off = "p", ((c - k) * S_ + s) * C_
        return img[name][self.base + off:self.base + off + C_]

    def copy(self):
        return {n: a.copy() for n, a in self.img.items()}

    def upload(self):
        for n, a in self.img.items():
            self.buf[n].upload(a)

    def download(self):
        return {n: b.download() for n, b in self.buf.items()}

    def same(self, want):
        got = self.download()
        return all(np.array_equal(got[n], want[n]) for n in want)

    def words(self, buf, dtype):
        return [int(v) for v in buf.download().view(dtype)]

    def scrub(self, ecglib):
        """verify -> repair -> verify, one stream, one sync.  -> (status before, verify result,
        repair result, status after, verify result, the repair's kernel)."""
        ctx, geo = self.ctx, (self.k, self.p, self.C, self.S)
        for b in self.status + self.result:
            b.fill(0xEE)
        ctx.verify(*geo, *self.args, self.status[0].ptr, self.result[0].ptr)
        ctx.repair(*geo, *self.args, self.status[0].ptr, self.result[1].ptr)
        name = ecglib.last_kernel()
        ctx.verify(*geo, *self.args, self.status[1].ptr, self.result[2].ptr)
        ctx.sync()
        return (self.words(self.status[0], np.uint32), self.words(self.result[0], np.uint64),
                self.words(self.result[1], np.uint64), self.words(self.status[1], np.uint32),
                self.words(self.result[2], np.uint64), name)

    def repair(self, ecglib, status):
        """ecg_repair alone on hand-made status words.  -> (result, kernel)."""
        self.status[0].upload(np.array(status, dtype=np.uint32).view(np.uint8))
        self.result[1].fill(0xEE)
        self.ctx.repair(self.k, self.p, self.C, self.S, *self.args, self.status[0].ptr, self.result[1].ptr)
        name = ecglib.last_kernel()
        self.ctx.sync()
        assert self.words(self.status[0], np.uint32) == [int(v) for v in status]      # read only
        return self.words(self.result[1], np.uint64), name

    def free(self):
        for b in list(self.buf.values()) + self.status + self.result:
            b.free()


def model_cell(ecglib, oracle, k, p, cells, par):
    """ecg_verify_cell of one stripe from first principles: cells [k][n], stored parity [p][n]."""
    from oracle.gf_np import MUL

    g = oracle.cauchy1(k, p)[k:]
    syn = par ^ oracle.encode_data(g, np.ascontiguousarray(cells))
    rows = sum(1 << r for r in range(p) if syn[r].any())
    cand = 0
    for j in range(k):
        if all(np.array_equal(MUL[g[0][j]][syn[r]], MUL[g[r][j]][syn[0]]) for r in range(1, p)):
            cand |= 1 << j
    return ecglib.verify_cell(st(rows, cand), k, p)


def break_two_cells(ecglib, oracle, rig, s, a, b):
    """Make cells a and b of stripe s wrong (one byte each, at different bytes where the cell has
    two) so that no single cell explains the stripe; the second error value is searched for,
    because at one and the same byte two errors can look like a third cell's."""
    k, p, C_ = rig.k, rig.p, rig.C
    offs = sorted({5 % C_, (C_ - 2) % C_})
    oa, ob = offs[0], offs[-1]
    cols = np.array(offs)
    for eb in range(1, 256):
        stripe = np.stack([rig.cell(rig.img, s, c)[cols] for c in range(k + p)])
        stripe[a, offs.index(oa)] ^= 0x11
        stripe[b, offs.index(ob)] ^= eb
        if model_cell(ecglib, oracle, k, p, stripe[:k], stripe[k:]) == -2:
            rig.cell(rig.img, s, a)[oa] ^= 0x11
            rig.cell(rig.img, s, b)[ob] ^= eb
            return
    pytest.fail("no error pair without a single-cell explanation")


def corrupt_batch(ecglib, oracle, rig):
    """Stripe s < k+p: cell s wrong -- its first byte, its last byte, a byte of its last 4 KiB
    column or the whole cell, in turn; then one clean stripe, one with two wrong data cells and
    one with a wrong data cell and a wrong parity row (whatever of those S leaves room for).
    Edits rig.img; -> (the image a correct repair leaves, the stripes it must leave bad)."""
    k, p, C_, S_ = rig.k, rig.p, rig.C, rig.S
    want = rig.copy()
    rng = np.random.default_rng(k * 31 + p + C_)
    for s in range(min(k + p, S_)):
        cell = rig.cell(rig.img, s, s)
        kind = s % 4
        if kind == 0:
            cell[0] ^= 0x01 + s
        elif kind == 1:
            cell[C_ - 1] ^= 0x80 >> (s % 8)
        elif kind == 2:
            cell[(C_ - 1) // 4096 * 4096 + (C_ - 1) % 4096 // 2] ^= 0x5a
        else:
            cell[:] ^= rng.integers(1, 256, C_, dtype=np.uint8)           # every byte differs
    left = []
    if S_ > k + p + 1:
        break_two_cells(ecglib, oracle, rig, k + p + 1, 0, k - 1)
        left.append(k + p + 1)
    if S_ > k + p + 2:
        break_two_cells(ecglib, oracle, rig, k + p + 2, 1, k)
        left.append(k + p + 2)
    if p < 2:                                   # nothing is attributable: every bad stripe stays
        left = list(range(min(k + p, S_))) + left
    for s in left:
        for c in range(k + p):
            rig.cell(want, s, c)[:] = rig.cell(rig.img, s, c)
    return want, left


def scrub_and_check(ecglib, oracle, rig, kernel):
    k, p, S_ = rig.k, rig.p, rig.S
    want, left = corrupt_batch(ecglib, oracle, rig)
    rig.upload()
    st0, v0, rep, st1, v1, name = rig.scrub(ecglib)
    assert name == kernel, name
    nbad = min(k + p, S_) + len([s for s in left if s >= k + p])
    cells = [ecglib.verify_cell(w, k, p) for w in st0]
    if p >= 2:
        assert cells[:k + p] == list(range(min(k + p, S_)))             # verify located every cell
        assert rep == [k + p, min(left) if left else U64MAX, k, len(left)]
    else:
        assert rep == [0, 0, 0, nbad]
    assert v0[0] == nbad
    got = rig.download()
    for n in want:                              # the images, their slack and their guards
        bad = np.flatnonzero(got[n] != want[n])
        assert bad.size == 0, (n, bad[:8] - rig.base, bad.size)
    assert [s for s, w in enumerate(st1) if ecglib.verify_cell(w, k, p) != -1] == left
    assert v1 == [len(left), min(left) if left else U64MAX, 0, len(left)]


# ------------------------------------------------ 1. one bad cell per stripe
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("C_", CELLS)
@pytest.mark.parametrize("k,p", SHAPES)
def test_scrub_repairs_every_cell_index(ctx, ecglib, oracle, k, p, C_, layout):
    rig = Rig(ctx, oracle, k, p, C_, layout)
    try:
        scrub_and_check(ecglib, oracle, rig, kernel_name(k))
    finally:
        rig.free()


# ------------------------------------------- 2. byte-identical to ecg_recover
@pytest.mark.parametrize("C_", CELLS)
@pytest.mark.parametrize("k,p", [kp for kp in SHAPES if kp[1] >= 2])
def test_identical_to_recover(ctx, ecglib, oracle, k, p, C_):
    """Random, inconsistent stripes: the bytes written depend on which survivors are read, so
    this pins ecg_recover's choice (the other data cells and parity row 0)."""
    rig = Rig(ctx, oracle, k, p, C_, "recov", S_=k + p, codeword=False)
    twin = ctx.alloc(rig.img["d"].size)
    try:
        rig.upload()
        twin.upload(rig.img["d"])
        stride = (k + p) * C_
        for s in range(k + p):
            ctx.recover(k, p, C_, 1, twin.ptr + rig.base + s * stride, stride, [s])
        ctx.sync()
        res, name = rig.repair(ecglib, [attributing(k, p, s) for s in range(k + p)])
        assert name == kernel_name(k)
        assert res == [k + p, U64MAX, k, 0]
        got, want = rig.download()["d"], twin.download()
        assert not np.array_equal(want, rig.img["d"])                   # recover did write
        assert np.array_equal(got, want)
    finally:
        twin.free()
        rig.free()


# ---------------------------------------------- 3. idempotent on clean stripes
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,p,C_", [(4, 2, 8192 + 48), (8, 3, 4096), (16, 2, 16), (5, 2, 128 * 1024)])
def test_rewriting_a_clean_cell_changes_nothing(ctx, ecglib, oracle, k, p, C_, layout):
    rig = Rig(ctx, oracle, k, p, C_, layout, S_=k + p)
    try:
        rig.upload()
        res, name = rig.repair(ecglib, [attributing(k, p, s) for s in range(k + p)])
        assert name == kernel_name(k)
        assert res == [k + p, U64MAX, k, 0]
        assert rig.same(rig.img)
    finally:
        rig.free()


# --------------------------------------- 4. status words verify never writes
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,p", SHAPES)
def test_any_status_word_is_safe(ctx, ecglib, oracle, k, p, layout):
    """Inconsistent stripes, so that any cell written would change: none may be."""
    allrows, allcand = (1 << p) - 1, (1 << k) - 1
    words = [0xFFFFFFFF,
             st(1 << p, 0), st(0x80, 1), st(allrows | (1 << p), 1),            # row bits at or above p
             st(allrows, 1 << k) if k < 16 else st(allrows, 0) | (1 << 24),    # a lone candidate outside the stripe
             st(allrows, 0xffff & ~allcand), 0xFFFFFF00 | allrows,
             st(0, 0), st(0, allcand), 0xFFFFFF00,                             # no rows: clean whatever else is set
             st(allrows, 0b11), st(allrows, allcand), st(allrows, 0)]          # two candidates, all, none
    if p == 3:
        words += [st(0b011, 1), st(0b101, 0), st(0b110, 2)]                    # a proper subset of the rows
    rig = Rig(ctx, oracle, k, p, 8192 + 48, layout, S_=len(words), codeword=False)
    try:
        rig.upload()
        cells = [ecglib.verify_cell(w, k, p) for w in words]
        assert set(cells) == {-1, -2}
        res, _ = rig.repair(ecglib, words)
        left = [s for s, c in enumerate(cells) if c == -2]
        assert res == [0, min(left), 0, len(left)]
        assert rig.same(rig.img)
    finally:
        rig.free()


# ------------------------------------------------------------ 5. strided grid
@pytest.mark.parametrize("layout", LAYOUTS)
def test_strided_grid(ctx, ecglib, oracle, layout):
    """2 blocks for a stripe's 3 columns: the column loop strides, and the block walks the 7
    stripes of its one group of status words in turn; of the 3 block rows two find no group
    (the group loop itself strides in test_more_stripes_than_a_block_row_reads)."""
    rig = Rig(ctx, oracle, 2, 2, 8192 + 48, layout, S_=7)
    ctx.set_launch(2, 3, 0)
    try:
        scrub_and_check(ecglib, oracle, rig, "ecg_repair_kernel<2>")
    finally:
        ctx.set_launch(0, 0, 0)
        rig.free()


@pytest.mark.parametrize("grid", [(0, 0), (1, 2)])
@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_more_stripes_than_a_block_row_reads(ctx, ecglib, oracle, layout, variant, grid):
    """A block row reads the status words of 64 stripes at a time: 200 stripes are four such
    groups, the last one partial; bad stripes at the groups' edges, several in one group, whole
    groups clean; with 2 block rows the group loop strides, with 1 column block the column loop."""
    k, p, C_, S_ = 4, 2, 4096 + 16, 200
    rig = Rig(ctx, oracle, k, p, C_, layout, S_=S_)
    singles = {s: i % (k + p) for i, s in enumerate([0, 1, 62, 63, 64, 65, 127, 191, 192, 199])}
    doubles = [66, 198]
    want = rig.copy()
    for s, c in singles.items():
        rig.cell(rig.img, s, c)[(s * 37) % C_] ^= 0x01 + s % 255
    for s in doubles:
        break_two_cells(ecglib, oracle, rig, s, 0, k - 1)
        for c in range(k + p):
            rig.cell(want, s, c)[:] = rig.cell(rig.img, s, c)
    ctx.set_launch(grid[0], grid[1], variant)
    try:
        rig.upload()
        st0, v0, rep, st1, v1, name = rig.scrub(ecglib)
    finally:
        ctx.set_launch(0, 0, 0)
        got = rig.download()
        rig.free()
    assert name == ("ecg_repair_byte_kernel" if variant == 2 else kernel_name(k))
    assert {s: ecglib.verify_cell(w, k, p) for s, w in enumerate(st0) if w & 0xff} == \
        {**singles, **{s: -2 for s in doubles}}
    assert rep == [len(singles), min(doubles), sum(1 for c in singles.values() if c < k), len(doubles)]
    assert all(np.array_equal(got[n], want[n]) for n in want)
    assert [s for s, w in enumerate(st1) if w & 0xff] == doubles
    assert v1 == [len(doubles), min(doubles), 0, len(doubles)]


# ----------------------------------------------------- 6. byte-granular kernel
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("skew,C_", [(1, 1), (3, 1), (1, 4099), (3, 4099), (0, 4099), (1, 4096)])
@pytest.mark.parametrize("k,p", [(4, 2), (8, 3), (5, 2), (2, 1)])
def test_byte_kernel(ctx, ecglib, oracle, k, p, skew, C_, layout):
    rig = Rig(ctx, oracle, k, p, C_, layout, skew=skew)
    try:
        scrub_and_check(ecglib, oracle, rig, "ecg_repair_byte_kernel")
    finally:
        rig.free()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,p", [(4, 2), (16, 2), (5, 2)])
def test_byte_kernel_forced_on_aligned_operands(ctx, ecglib, oracle, k, p, layout):
    rig = Rig(ctx, oracle, k, p, 8192 + 48, layout)
    ctx.set_launch(0, 0, 2)
    try:
        scrub_and_check(ecglib, oracle, rig, "ecg_repair_byte_kernel")
    finally:
        ctx.set_launch(0, 0, 0)
        rig.free()


# ---------------------------------------------------------------- 7. arguments
def test_argument_errors(ctx, ecglib, oracle):
    L = ecglib.lib()
    k, p, C_ = 4, 2, 4096
    rig = Rig(ctx, oracle, k, p, C_, "client", codeword=False)
    try:
        rig.upload()
        a, S_, stw, res = rig.args, rig.S, rig.status[0].ptr, rig.result[1].ptr
        rig.status[0].upload(np.array([attributing(k, p, 0)] * S_, dtype=np.uint32).view(np.uint8))

        def call(k_=k, p_=p, C__=C_, S__=S_, status=stw, result=res):
            return L.ecg_repair(ctx.h, k_, p_, C__, S__, a[0], a[1], a[2], a[3], a[4], status, result, None)

        for kk, pp in ((17, 2), (0, 2), (4, 9), (4, 0)):
            assert call(k_=kk, p_=pp) == -ecglib.DER_INVAL, (kk, pp)
        assert call(result=res + 4) == -ecglib.DER_INVAL
        assert b"result" in L.ecg_strerror()
        assert call(result=None) == -ecglib.DER_INVAL
        assert call(status=None) == -ecglib.DER_INVAL
        assert call(status=stw + 2) == -ecglib.DER_INVAL
        for inside in (a[0], a[0] + S_ * k * C_ - 4, a[2] + 64, a[2] + p * S_ * C_ - 4):
            assert call(status=inside) == -ecglib.DER_INVAL             # status inside the data or parity
            assert b"overlaps" in L.ecg_strerror()
        # an empty batch and empty cells preset the result and touch nothing else
        for kw in ({"S__": 0, "status": None}, {"C__": 0}):
            rig.result[1].fill(0xEE)
            assert call(**kw) == 0
            ctx.sync()
            assert rig.words(rig.result[1], np.uint64) == [0, U64MAX, 0, 0]
        assert rig.same(rig.img)                                        # none of the calls above wrote a cell
    finally:
        rig.free()


def test_counts_one_launch_and_no_recover_stripes(ctx, ecglib, oracle):
    rig = Rig(ctx, oracle, 4, 2, 4096, "recov", S_=6)
    try:
        rig.upload()
        before = ctx.stats()
        rig.repair(ecglib, [attributing(4, 2, s) for s in range(6)])
        after = ctx.stats()
        assert after["launches"] == before["launches"] + 1
        assert after["recover_stripes"] == before["recover_stripes"]    # the count lives on the device
    finally:
        rig.free()
