"""GPU parity of the pointer-table product with a cell length per stripe (ecg_matmul_ptrs_lens) and
of the batched single-value encode on device buffers (ecg_obj_ec_singv_encode_dev) against the CPU
oracle.  Bit-exact; every byte of the buffer outside the output cells must stay as it was."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64
SPAN = 65536
# 0 (entries NULL); around the dword and the 16-byte lane; around a 4 KiB column; exactly one span; a
# second span of one partial column (16 and 1 bytes); three spans and a fourth of two columns
MIX = [0, 1, 3, 4, 15, 16, 17, 4095, 4096, 4097, 4112, SPAN, SPAN + 16, SPAN + 1, 3 * SPAN + 4096 + 5]
MIX16 = [0, 16, 4096, 4112, SPAN, SPAN + 16, 4080, 3 * SPAN + 4096 + 16]       # every length % 16 == 0


@functools.lru_cache(maxsize=None)
def _reference(oracle_mod, k, rows, lens, seed, decode=False):
    """(coef, cells[s] = [k, L] inputs, want[s] = [rows, L]) of a batch, drawn once per batch and
    shared by every test that runs it.  decode: the inputs are the survivors of cells 1 and k lost
    from encoded stripes, coef the rows that regenerate them."""
    rng = np.random.default_rng([seed, k, rows])
    if decode:
        from daos_amd import ecg
        rws, dec, _ = ecg.recov_matrix(k, rows, [1, k])
        coef = np.ascontiguousarray(rws)
    else:
        coef = rng.integers(0, 256, (rows, k), dtype=np.uint8)
    cells, want = [], []
    for s, L in enumerate(lens):
        rng = np.random.default_rng([seed, k, rows, s])     # a stripe's bytes do not depend on the others' lengths
        if decode:
            data = rng.integers(0, 256, (k, L), dtype=np.uint8)
            full = np.concatenate([data, oracle_mod.encode_data(oracle_mod.cauchy1(k, rows)[k:], data)]) \
                if L else np.zeros((k + rows, 0), np.uint8)
            cells.append(np.ascontiguousarray(full[[int(i) for i in dec]]))
            want.append(np.ascontiguousarray(full[[1, k]]))         # the original cells, not a product
        else:
            cells.append(rng.integers(0, 256, (k, L), dtype=np.uint8))
            want.append(oracle_mod.encode_data(coef, cells[-1]) if L else np.zeros((rows, 0), np.uint8))
    return coef, cells, want


class Batch:
    """The cells of a batch scattered over one device buffer: every cell of every stripe of
    non-zero length in its own slot (shuffled, or in table order with shuffle=False), followed by GUARD
    bytes; the whole buffer is non-zero garbage but for the input cells.  skew[(s, j)] moves cell j of
    stripe s off its 16-byte aligned slot start."""

    def __init__(self, ctx, oracle, k, rows, lens, seed=1, skew=None, shuffle=True, decode=False):
        self.ctx, self.k, self.rows, self.lens = ctx, k, rows, list(lens)
        self.coef, self.cells, self.want = _reference(oracle, k, rows, tuple(lens), seed, decode)
        rng = np.random.default_rng([seed, 77])
        skew = skew or {}
        ids = [(s, j) for s, L in enumerate(lens) if L for j in range(k + rows)]
        order = rng.permutation(len(ids)) if shuffle else range(len(ids))
        self.off, at = {}, 0
        for i in order:
            s, j = ids[int(i)]
            self.off[(s, j)] = at + skew.get((s, j), 0)
            at += (lens[s] + 15) // 16 * 16 + GUARD + 16
        self.host = rng.integers(1, 256, max(at, 16), dtype=np.uint8)
        for (s, j), o in self.off.items():
            if j < k:
                self.host[o:o + lens[s]] = self.cells[s][j]
        self.buf = ctx.alloc(self.host.size)
        self.buf.upload(self.host)

    def table(self):
        n = self.k + self.rows
        return [self.buf.ptr + self.off[(s, j)] if L else None for s, L in enumerate(self.lens) for j in range(n)]

    def run(self):
        self.ctx.matmul_ptrs_lens(self.k, self.rows, self.coef, self.table(), self.lens)
        self.ctx.sync()

    def check(self):
        """The whole buffer: the outputs as the oracle has them, every other byte untouched."""
        exp = self.host.copy()
        for s, L in enumerate(self.lens):
            for r in range(self.rows if L else 0):
                o = self.off[(s, self.k + r)]
                exp[o:o + L] = self.want[s][r]
        dev = self.buf.download()
        bad = np.flatnonzero(dev != exp)
        assert bad.size == 0, (int(bad[0]), bad.size, self._where(int(bad[0])))
        return dev

    def outputs(self, dev):
        return [[dev[self.off[(s, self.k + r)]:][:L] for r in range(self.rows)] for s, L in enumerate(self.lens) if L]

    def _where(self, at):
        for (s, j), o in self.off.items():
            if o <= at < o + self.lens[s] + GUARD:
                return "stripe %d cell %d byte %d of %d" % (s, j, at - o, self.lens[s])
        return "between slots"

    def free(self):
        self.buf.free()


def _lens_name(k, rows, g):
    shape = "%d,%d" % (k, rows) if (k in (2, 4, 8, 16) and rows <= 3) else "0,0"
    return "ecg_mm_ptr_lens_kernel<%s%s>" % (shape, "" if g == 16 else ",g%d" % g)


@pytest.mark.parametrize("k,rows", [(2, 1), (4, 2), (8, 3), (16, 2), (3, 4)])
def test_length_mix(oracle, ecglib, ctx, k, rows):
    """One batch over every length class; cells 16-byte aligned, so the one odd length alone puts
    the launch on dword lanes."""
    b = Batch(ctx, oracle, k, rows, MIX)
    try:
        before = ctx.stats()["launches"]
        b.run()
        assert ecglib.last_kernel() == _lens_name(k, rows, 4)
        assert ctx.stats()["launches"] == before + 1
        b.check()
    finally:
        b.free()


def test_plan_of_the_mix(ecglib):
    assert ecglib.lens_plan(MIX) == (19, 16) and ecglib.lens_plan(MIX16) == (11, 16)


@pytest.mark.parametrize("k,rows,odd", [(4, 2, 1), (8, 2, 4), (8, 2, 1), (16, 2, 3)])
def test_granules(oracle, ecglib, ctx, k, rows, odd):
    """The lanes by ecg_last_kernel, as ecg_matmul_ptrs chooses them: 16-byte lanes when every
    address and every length is a multiple of 16, dword lanes for one length that is not, the
    funnel-shifted lanes for one input off its alignment (g2 for k = 8, else g1), the byte kernel
    for launch variant 2 -- and the same bytes from all of them."""
    outs = {}

    def one(name, lens, skew=None, variant=0, kernel=None):
        b = Batch(ctx, oracle, k, rows, lens, seed=2, skew=skew)
        try:
            ctx.set_launch(0, 0, variant)
            try:
                b.run()
            finally:
                ctx.set_launch(0, 0, 0)
            assert ecglib.last_kernel() == kernel, name
            outs[name] = b.outputs(b.check())
        finally:
            b.free()

    lens4 = list(MIX16)
    lens4[3] += 4
    one("g16", MIX16, kernel=_lens_name(k, rows, 16))
    one("g4", lens4, kernel=_lens_name(k, rows, 4))
    one("skew", MIX16, skew={(4, k - 1): odd}, kernel=_lens_name(k, rows, 2 if k == 8 else 1))
    one("outskew", MIX16, skew={(4, k): 3}, kernel=_lens_name(k, rows, 4))    # an output off a dword
    one("byte", MIX16, variant=2, kernel="ecg_mm_ptr_lens_byte_kernel")
    one("generic", MIX16, variant=1, kernel="ecg_mm_ptr_lens_kernel<0,0>")
    for name in ("skew", "outskew", "byte", "generic"):
        for a, c in zip(outs["g16"], outs[name]):
            assert all(np.array_equal(x, y) for x, y in zip(a, c)), name
    same = [i for i in range(len(outs["g16"])) if i != 2]        # MIX16[3] is the 3rd non-zero stripe
    for i in same:
        assert all(np.array_equal(x, y) for x, y in zip(outs["g16"][i], outs["g4"][i])), i


@pytest.mark.parametrize("gx,gy", [(1, 1), (3, 2)])
@pytest.mark.parametrize("variant", [0, 2])
def test_grid_overrides(oracle, ecglib, ctx, gx, gy, variant):
    """ecg_set_launch's grid_x / grid_y: a block walks several columns of a span and several spans."""
    b = Batch(ctx, oracle, 4, 2, MIX)
    try:
        ctx.set_launch(gx, gy, variant)
        try:
            b.run()
        finally:
            ctx.set_launch(0, 0, 0)
        assert ecglib.last_kernel() == ("ecg_mm_ptr_lens_byte_kernel" if variant else _lens_name(4, 2, 4))
        b.check()
    finally:
        b.free()


@pytest.mark.parametrize("L,shuffle", [(4112, True), (SPAN + 5, True), (8192, False)])
def test_equal_lengths_are_matmul_ptrs(oracle, ecglib, ctx, L, shuffle):
    """No zero and one length: ecg_matmul_ptrs's route and kernel (the offset kernel for the affine
    table), and its bytes."""
    k, rows, S = 4, 2, 5
    b = Batch(ctx, oracle, k, rows, [L] * S, seed=3, shuffle=shuffle)
    try:
        b.run()
        name = ecglib.last_kernel()
        got = b.check()
        b.buf.upload(b.host)
        ctx.matmul_ptrs(k, rows, b.coef, L, S, b.table())
        ctx.sync()
        assert ecglib.last_kernel() == name
        assert name.startswith("ecg_mm_ptr_kernel<4,2" if shuffle else "ecg_mm_kernel<4,2,"), name
        assert np.array_equal(b.buf.download(), got)
    finally:
        b.free()


def test_equal_lengths_with_a_skipped_stripe(oracle, ecglib, ctx):
    """One length but a zero among them: the per-stripe kernel (the NULL row is never read)."""
    b = Batch(ctx, oracle, 4, 2, [4096, 0, 4096, 4096], seed=4)
    try:
        b.run()
        assert ecglib.last_kernel() == _lens_name(4, 2, 16)
        b.check()
    finally:
        b.free()


def test_nothing_to_do(ecglib, ctx):
    before = ctx.stats()["launches"]
    coef = np.ones((2, 4), np.uint8)
    ctx.matmul_ptrs_lens(4, 2, coef, [None] * 18, [0, 0, 0])
    ctx.matmul_ptrs_lens(4, 2, coef, [], [])
    assert ctx.stats()["launches"] == before


def test_null_entry_is_named(ecglib, ctx):
    with pytest.raises(ecglib.EcgError) as ei:
        ctx.matmul_ptrs_lens(4, 2, np.ones((2, 4), np.uint8), [None] * 6 + [4096] * 5 + [None], [0, 64])
    assert ei.value.rc == -ecglib.DER_INVAL
    assert b"matmul_ptrs_lens: NULL cell 11" in ecglib.lib().ecg_strerror()


@pytest.mark.parametrize("k,p", [(4, 2), (8, 2)])
def test_decode_rows(oracle, ecglib, ctx, k, p):
    """Recovery rows of ecg_recov_matrix over a mixed-length batch: cells 1 and k regenerated from
    the survivors, against the original cells."""
    b = Batch(ctx, oracle, k, p, MIX, seed=5, decode=True)
    try:
        b.run()
        assert ecglib.last_kernel() == _lens_name(k, p, 4)
        b.check()
    finally:
        b.free()


# ---- single values --------------------------------------------------------

OC = {(2, 1): 32, (8, 2): 37, (16, 2): 39}
SIZES = [17, 4096, 8200, 8569, 70001]      # 17: with k = 16 thirteen cells are padding alone


@pytest.mark.parametrize("k,p", [(2, 1), (8, 2), (16, 2)])
def test_singv_encode_dev(oracle, ecglib, ctx, k, p):
    """Values at odd addresses, each followed by 0xFF; parity against the oracle's single-value
    encode, and every byte outside the parity cells untouched."""
    L = ecglib.lib()
    oc = (OC[(k, p)] << 24) | 1
    rng = np.random.default_rng(900 + k)
    vals = [rng.integers(0, 256, n, dtype=np.uint8) for n in SIZES]
    cbs = [L.ecg_obj_ec_singv_cell_bytes(oc, n) for n in SIZES]
    assert cbs == [oracle.singv_cell_bytes(n, k) for n in SIZES] and len(set(cbs)) > 1
    voff, at = [], 0
    for n in SIZES:
        voff.append(at + 1)                                             # odd
        at += (n + 1 + 15) // 16 * 16 + GUARD
    poff = []
    for cb in cbs:
        for _ in range(p):
            poff.append(at)
            at += cb + GUARD
    host = np.full(at, 0xFF, dtype=np.uint8)
    for o, v in zip(voff, vals):
        host[o:o + v.size] = v
    buf = ctx.alloc(at)
    try:
        buf.upload(host)
        before = ctx.stats()["launches"]
        ctx.singv_encode_dev(oc, SIZES, [buf.ptr + o for o in voff], [buf.ptr + o for o in poff])
        ctx.sync()
        kern = ecglib.last_kernel()
        # odd inputs: funnel-shifted lanes (16-byte ones for k = 8); cell sizes are multiples of 8
        assert kern == _lens_name(k, p, 2 if k == 8 else 1), kern
        assert ctx.stats()["launches"] == before + 1
        exp = host.copy()
        for i, v in enumerate(vals):
            want = oracle.singv_encode(k, p, v)
            for r in range(p):
                exp[poff[i * p + r]:][:cbs[i]] = want[r]
        dev = buf.download()
        bad = np.flatnonzero(dev != exp)
        assert bad.size == 0, (int(bad[0]), bad.size)
    finally:
        buf.free()


def test_singv_encode_dev_one_size(oracle, ecglib, ctx):
    """Values of one cell size: the fixed-length kernel over the same staged table."""
    k, p, oc = 8, 2, (37 << 24) | 1
    sizes = [8569, 8570, 8575]                                          # ceil(n / 8) -> 1072 for all
    rng = np.random.default_rng(31)
    vals = [rng.integers(0, 256, n, dtype=np.uint8) for n in sizes]
    cb = oracle.singv_cell_bytes(sizes[0], k)
    assert all(oracle.singv_cell_bytes(n, k) == cb for n in sizes)
    stride = 8592 + GUARD
    host = np.full(3 * stride + 3 * p * (cb + GUARD), 0xFF, dtype=np.uint8)
    for i, v in enumerate(vals):
        host[i * stride:][:v.size] = v
    poff = [3 * stride + j * (cb + GUARD) for j in range(3 * p)]
    buf = ctx.alloc(host.size)
    try:
        buf.upload(host)
        ctx.singv_encode_dev(oc, sizes, [buf.ptr + i * stride for i in range(3)], [buf.ptr + o for o in poff])
        ctx.sync()
        assert ecglib.last_kernel().startswith("ecg_mm_ptr_kernel<8,2"), ecglib.last_kernel()
        exp = host.copy()
        for i, v in enumerate(vals):
            want = oracle.singv_encode(k, p, v)
            for r in range(p):
                exp[poff[i * p + r]:][:cb] = want[r]
        assert np.array_equal(buf.download(), exp)
    finally:
        buf.free()
