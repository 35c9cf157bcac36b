"""ecg_verify on the GPU: parity from the CPU oracle, corruption injected
byte by byte, and the status words, the 4-word result and ecg_verify_cell
derived here from what was injected.  Everything is exact.

Shapes: one 4 KiB column, a lane-masked last column (8192 + 48) and many
blocks per stripe (128 KiB), each in the client layout (data [S][k][C],
parity [p][S][C]) and the recovery layout ([S][k+p][C]); the specialised
kernels, the runtime-shaped one (k = 5) and the byte-granular fallback."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1), (4, 2), (8, 2), (16, 2), (8, 3), (5, 2)]
CELLS = [4096, 8192 + 48, 128 * 1024]
LAYOUTS = ["client", "recov"]
S = 5
U64MAX = (1 << 64) - 1

_REF = {}


def reference(oracle, k, p, C_, S_=S):
    """(data [S][k][C], parity [p][S][C]) of the oracle, computed once per shape and never modified."""
    key = (k, p, C_, S_)
    if key not in _REF:
        data = np.random.default_rng(k * 1000003 + p * 101 + C_).integers(0, 256, (S_, k, C_), dtype=np.uint8)
        par = oracle.encode_batch(k, p, C_, S_, data.reshape(-1)).reshape(p, S_, C_)
        data.setflags(write=False)
        par.setflags(write=False)
        _REF[key] = (data, par)
    return _REF[key]


class Rig:
    """Device copy of a shape's stripes in one of the two layouts; cells 0..k-1 data, k..k+p-1 parity.
    skew: byte offset of the data and parity from their (256-byte aligned) allocations."""

    def __init__(self, ctx, oracle, k, p, C_, layout, S_=S, skew=0):
        self.ctx, self.k, self.p, self.C, self.S, self.layout = ctx, k, p, C_, S_, layout
        self.data, self.par = reference(oracle, k, p, C_, S_)
        if layout == "client":
            self.dbuf = ctx.alloc(self.data.size + skew + 64)
            self.pbuf = ctx.alloc(self.par.size + skew + 64)
            self.dbuf.fill(0xA5)
            self.pbuf.fill(0xA5)
            self.dbuf.upload(self.data, skew)
            self.pbuf.upload(self.par, skew)
            self.args = (self.dbuf.ptr + skew, k * C_, self.pbuf.ptr + skew, S_ * C_, C_)
        else:
            st = np.concatenate([self.data, self.par.transpose(1, 0, 2)], axis=1)      # [S][k+p][C]
            self.dbuf = self.pbuf = ctx.alloc(st.size + skew + 64)
            self.dbuf.fill(0xA5)
            self.dbuf.upload(st, skew)
            self.args = (self.dbuf.ptr + skew, (k + p) * C_, self.dbuf.ptr + skew + k * C_, C_, (k + p) * C_)
        self.skew = skew
        self.status = ctx.alloc(4 * S_)
        self.result = ctx.alloc(32)
        self.before = self.snapshot()

    def where(self, s, cell, i):
        """(buffer, byte offset in it, clean value) of byte i of `cell` of stripe s."""
        k, p, C_, S_ = self.k, self.p, self.C, self.S
        val = int(self.data[s, cell, i]) if cell < k else int(self.par[cell - k, s, i])
        if self.layout == "recov":
            return self.dbuf, self.skew + (s * (k + p) + cell) * C_ + i, val
        if cell < k:
            return self.dbuf, self.skew + (s * k + cell) * C_ + i, val
        return self.pbuf, self.skew + ((cell - k) * S_ + s) * C_ + i, val

    @contextlib.contextmanager
    def corrupt(self, flips):
        """flips: (stripe, cell, byte, xor != 0), or (stripe, cell, None, bytes) for a whole cell."""
        undo = []
        for s, cell, i, x in flips:
            if i is None:
                buf, off, _ = self.where(s, cell, 0)
                clean = self.data[s, cell] if cell < self.k else self.par[cell - self.k, s]
                assert x.shape == clean.shape
                buf.upload(x, off)
                undo.append((buf, off, clean))
            else:
                buf, off, val = self.where(s, cell, i)
                assert 0 < x < 256
                buf.upload(np.array([val ^ x], dtype=np.uint8), off)
                undo.append((buf, off, np.array([val], dtype=np.uint8)))
        try:
            yield
        finally:
            for buf, off, clean in undo:
                buf.upload(clean, off)

    def run(self):
        self.status.fill(0xEE)
        self.result.fill(0xEE)
        self.ctx.verify(self.k, self.p, self.C, self.S, *self.args, self.status.ptr, self.result.ptr)
        self.ctx.sync()
        return (self.status.download().view(np.uint32).copy(),
                [int(v) for v in self.result.download().view(np.uint64)])

    def snapshot(self):
        return self.dbuf.download(), self.pbuf.download()

    def free(self):
        bufs = {id(b): b for b in (self.dbuf, self.pbuf, self.status, self.result)}
        for b in bufs.values():
            b.free()


def kernel_name(k, p):
    return f"ecg_verify_kernel<{k},{p}>" if k in (2, 4, 8, 16) and p in (1, 2, 3) else "ecg_verify_kernel<0,0>"


def check(ecglib, rig, bad, kernel=None):
    """bad: {stripe: (rows, candidate bits, cell or -2)}, derived by the caller from what it injected."""
    k, p = rig.k, rig.p
    status, result = rig.run()
    assert ecglib.last_kernel() == (kernel or kernel_name(k, p)), ecglib.last_kernel()
    want = np.full(rig.S, ((1 << k) - 1) << 8, dtype=np.uint32)
    for s, (rows, cand, _) in bad.items():
        want[s] = rows | (cand << 8)
    assert [hex(v) for v in status] == [hex(v) for v in want]
    for s in range(rig.S):
        assert ecglib.verify_cell(int(status[s]), k, p) == (bad[s][2] if s in bad else -1), s
    one = sum(1 for v in bad.values() if v[2] >= 0)
    assert result == [len(bad), min(bad) if bad else U64MAX, one, len(bad) - one]


def data_flip(k, p, j):
    """One data cell wrong: every parity row differs, only j explains it (p == 1: not attributable)."""
    return ((1 << p) - 1, 1 << j, j) if p >= 2 else (1, (1 << k) - 1, -2)


def parity_flip(k, p, r):
    return (1 << r, 0, k + r) if p >= 2 else (1, (1 << k) - 1, -2)


def unattributable(k, p, rows=None):
    return ((1 << p) - 1 if rows is None else rows, 0 if p >= 2 else (1 << k) - 1, -2)


def offsets(C_):
    offs = [0, 15, 16, 4095, C_ - 1]
    if C_ > 4096:
        offs.append(4096)
    if C_ % 4096:
        offs.append(C_ - C_ % 4096)         # first byte of the partial column (its last byte is C - 1)
    return sorted(set(offs))


def model_status(oracle, k, p, cells, par):
    """Status word of one stripe from first principles: cells [k][C], stored parity [p][C]."""
    from oracle.gf_np import MUL

    g = oracle.cauchy1(k, p)[k:]
    syn = par ^ oracle.encode_data(g, cells)
    rows = sum(1 << r for r in range(p) if syn[r].any())
    cand = 0
    for j in range(k):
        if all(np.array_equal(MUL[g[0][j]][syn[r]], MUL[g[r][j]][syn[0]]) for r in range(1, p)):
            cand |= 1 << j
    return rows, cand


@pytest.fixture(params=[(k, p, C_, lay) for k, p in SHAPES for C_ in CELLS for lay in LAYOUTS],
                ids=lambda t: f"{t[0]}p{t[1]}-{t[2]}-{t[3]}")
def rig(request, ctx, oracle):
    k, p, C_, lay = request.param
    r = Rig(ctx, oracle, k, p, C_, lay)
    yield r
    r.free()


def test_clean_and_read_only(ecglib, rig):
    check(ecglib, rig, {})
    after = rig.snapshot()
    assert np.array_equal(after[0], rig.before[0]) and np.array_equal(after[1], rig.before[1])


def test_one_byte_in_a_data_cell(ecglib, rig):
    k, p = rig.k, rig.p
    n = 0
    for j in range(k):
        for off in offsets(rig.C):
            s = n % rig.S
            n += 1
            with rig.corrupt([(s, j, off, 1 + (n * 37) % 255)]):
                check(ecglib, rig, {s: data_flip(k, p, j)})
    after = rig.snapshot()                  # verify wrote nothing, the flips were put back
    assert np.array_equal(after[0], rig.before[0]) and np.array_equal(after[1], rig.before[1])


def test_one_byte_in_a_parity_row(ecglib, rig):
    k, p = rig.k, rig.p
    for r in range(p):
        for n, off in enumerate(offsets(rig.C)):
            s = (n + r) % rig.S
            with rig.corrupt([(s, k + r, off, 0x80 >> (n % 8))]):
                check(ecglib, rig, {s: parity_flip(k, p, r)})


def test_whole_data_cell_replaced(ecglib, oracle, rig):
    """Every block of the stripe takes the dirty path and ANDs into the same word."""
    k, p = rig.k, rig.p
    j, s = k - 1, 2
    junk = np.random.default_rng(99).integers(0, 256, rig.C, dtype=np.uint8)
    cells = rig.data[s].copy()
    cells[j] = junk
    rows, cand = model_status(oracle, k, p, cells, rig.par[:, s])
    want = data_flip(k, p, j)
    assert (rows, cand) == want[:2] or p == 1       # the model agrees with the derivation
    with rig.corrupt([(s, j, None, junk)]):
        check(ecglib, rig, {s: want})


def test_same_cell_bad_in_two_places(ecglib, rig):
    k, p = rig.k, rig.p
    far = 4096 + 7 if rig.C > 4096 else 2000        # another column, or another wave of the only one
    for j in (0, k - 1):
        with rig.corrupt([(1, j, 5, 0x11), (1, j, far, 0xC3), (1, j, rig.C - 2, 0x01)]):
            check(ecglib, rig, {1: data_flip(k, p, j)})


def test_two_data_cells_bad_in_different_places(ecglib, rig):
    k, p = rig.k, rig.p
    far = 4096 + 7 if rig.C > 4096 else 2000
    with rig.corrupt([(3, 0, 5, 0x11), (3, k - 1, far, 0xC3)]):
        check(ecglib, rig, {3: unattributable(k, p)})


def test_two_data_cells_bad_at_the_same_byte(ecglib, oracle, rig):
    """The two errors are chosen so that no third cell explains their syndrome."""
    k, p = rig.k, rig.p
    s, a, b, off = 0, 0, k - 1, 16 * 3 + 1
    for eb in range(1, 256):
        cells = rig.data[s].copy()
        cells[a, off] ^= 0x01
        cells[b, off] ^= eb
        rows, cand = model_status(oracle, k, p, cells[:, off:off + 1], rig.par[:, s, off:off + 1])
        if p == 1 and rows:
            break
        if p >= 2 and rows == (1 << p) - 1 and cand == 0:
            break
    else:
        pytest.fail("no error pair without a third explanation")
    with rig.corrupt([(s, a, off, 0x01), (s, b, off, eb)]):
        check(ecglib, rig, {s: unattributable(k, p)})


def test_two_parity_rows_bad(ecglib, rig):
    k, p = rig.k, rig.p
    if p < 2:
        with rig.corrupt([(4, k, 9, 0x40)]):          # (2,1): detected, never attributable
            check(ecglib, rig, {4: unattributable(k, p)})
        return
    with rig.corrupt([(4, k, 9, 0x40), (4, k + 1, rig.C - 3, 0x02)]):
        check(ecglib, rig, {4: unattributable(k, p, rows=0b11)})


def test_several_bad_stripes(ecglib, rig):
    k, p = rig.k, rig.p
    with rig.corrupt([(1, k - 1, rig.C - 1, 0x7f), (3, k + p - 1, 0, 0x01),
                      (4, 0, 1, 0x10), (4, 1, rig.C // 2, 0x20)]):
        check(ecglib, rig, {1: data_flip(k, p, k - 1), 3: parity_flip(k, p, p - 1), 4: unattributable(k, p)})


# ------------------------------------------------------------------ fallback
@pytest.mark.parametrize("k,p", [(2, 1), (4, 2), (8, 3), (5, 2)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_byte_kernel_misaligned(ctx, ecglib, oracle, k, p, layout):
    """Data and parity one byte off, C = 4099: the byte-granular kernel, same answers."""
    rig = Rig(ctx, oracle, k, p, 4099, layout, skew=1)
    try:
        name = "ecg_verify_byte_kernel"
        check(ecglib, rig, {}, kernel=name)
        n = 0
        for j in range(k):
            for off in (0, 15, 16, 4095, 4096, 4098):
                s = n % rig.S
                n += 1
                with rig.corrupt([(s, j, off, 1 + (n * 29) % 255)]):
                    check(ecglib, rig, {s: data_flip(k, p, j)}, kernel=name)
        for r in range(p):
            with rig.corrupt([(r, k + r, 4098 - r, 0x08)]):
                check(ecglib, rig, {r: parity_flip(k, p, r)}, kernel=name)
        with rig.corrupt([(2, 0, 3, 0x11), (2, k - 1, 4097, 0xC3)]):
            check(ecglib, rig, {2: unattributable(k, p)}, kernel=name)
        after = rig.snapshot()
        assert np.array_equal(after[0], rig.before[0]) and np.array_equal(after[1], rig.before[1])
    finally:
        rig.free()


@pytest.mark.parametrize("k,p", [(4, 2), (8, 3), (5, 2)])
def test_byte_kernel_equals_lane_kernel(ctx, ecglib, oracle, k, p):
    """The same aligned, corrupted stripes through both kernels: identical status and result."""
    rig = Rig(ctx, oracle, k, p, 8192 + 48, "client")
    junk = np.random.default_rng(5).integers(0, 256, rig.C, dtype=np.uint8)
    try:
        with rig.corrupt([(0, 1, None, junk), (1, k, 8192 + 47, 0x04), (3, 0, 77, 0x31), (3, 2, 4100, 0x32),
                          (4, k - 1, 8192, 0x55)]):
            fast = rig.run()
            assert ecglib.last_kernel() == kernel_name(k, p)
            ctx.set_launch(0, 0, 2)
            try:
                slow = rig.run()
                assert ecglib.last_kernel() == "ecg_verify_byte_kernel"
            finally:
                ctx.set_launch(0, 0, 0)
        assert np.array_equal(fast[0], slow[0]) and fast[1] == slow[1]
        assert fast[1] == [4, 0, 3, 1]
        assert [ecglib.verify_cell(int(v), k, p) for v in fast[0]] == [1, k, -1, -2, k - 1]
    finally:
        rig.free()


# -------------------------------------------------------------- grid striding
def test_many_stripes(ctx, ecglib, oracle):
    """More stripes than a grid dimension holds: the stripe loop strides."""
    k, p, C_, S_ = 2, 1, 64, 70000
    rig = Rig(ctx, oracle, k, p, C_, "client", S_=S_)
    try:
        check(ecglib, rig, {})
        with rig.corrupt([(S_ - 1, 1, 63, 0x80)]):
            status, result = rig.run()
        assert ecglib.last_kernel() == "ecg_verify_kernel<2,1>"
        assert result == [1, S_ - 1, 0, 1]
        assert int(status[S_ - 1]) == 1 | (0b11 << 8) and not (status[:S_ - 1] & 0xff).any()
        assert ecglib.verify_cell(int(status[S_ - 1]), k, p) == -2
    finally:
        rig.free()


# ------------------------------------------------------------------ arguments
def test_argument_validation(ctx, ecglib, oracle):
    L = ecglib.lib()
    rig = Rig(ctx, oracle, 4, 2, 4096, "client")
    try:
        a = rig.args
        for k, p in ((17, 2), (0, 2), (4, 9), (4, 0)):
            assert L.ecg_verify(ctx.h, k, p, 4096, S, a[0], a[1], a[2], a[3], a[4], rig.status.ptr, rig.result.ptr,
                                None) == -ecglib.DER_INVAL, (k, p)
        assert b"k=17" in L.ecg_strerror() or b"p=0" in L.ecg_strerror()
        assert L.ecg_verify(ctx.h, 4, 2, 4096, S, a[0], a[1], a[2], a[3], a[4], rig.status.ptr, rig.result.ptr + 4,
                            None) == -ecglib.DER_INVAL
        assert L.ecg_verify(ctx.h, 4, 2, 4096, S, a[0], a[1], a[2], a[3], a[4], rig.status.ptr, None,
                            None) == -ecglib.DER_INVAL
        assert L.ecg_verify(ctx.h, 4, 2, 4096, S, a[0], a[1], a[2], a[3], a[4], None, rig.result.ptr,
                            None) == -ecglib.DER_INVAL
        # an empty batch presets the result and touches nothing else
        rig.result.fill(0xEE)
        rig.status.fill(0xEE)
        assert L.ecg_verify(ctx.h, 4, 2, 4096, 0, a[0], a[1], a[2], a[3], a[4], None, rig.result.ptr, None) == 0
        ctx.sync()
        assert [int(v) for v in rig.result.download().view(np.uint64)] == [0, U64MAX, 0, 0]
        assert (rig.status.download() == 0xEE).all()
    finally:
        rig.free()


def test_counts_launches(ctx, ecglib, oracle):
    rig = Rig(ctx, oracle, 4, 2, 4096, "recov")
    try:
        before = ctx.stats()["launches"]
        rig.run()
        assert ctx.stats()["launches"] == before + 2        # the syndrome pass and the summary
    finally:
        rig.free()
