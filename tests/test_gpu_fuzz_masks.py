"""Seeded random strides, layouts and far offsets through the mask-driven calls: ecg_recover_masks,
ecg_recover_masks_ptrs, ecg_csum_masked, ecg_recover_masks_csum, ecg_csum_mask, ecg_update_masks,
ecg_verify and ecg_repair, byte for byte against the CPU oracle.

The calls' own modules are thorough on the words (every erasure set, every mask value) and use
the two tight layouts; here the addressing is drawn: every stride parameter on its own (tight,
padded by a multiple of 16, padded off 16 so that the stride alone picks the byte kernel, gapped
parity rows, parity interleaved apart from the data, images that descend in address), base skews,
flags, grid overrides and stripe counts around the 64-stripe block row.  Every allocation is
0xA5 where no cell lies (256 guard bytes in front, slack behind, every gap a padded stride
opens) and is compared whole after the call, and the kernel that ran must be the one `predict`
names: the header's rule (include/ecg.h) that the 16-byte lane kernel runs iff every pointer,
every stride and cell_bytes are multiples of 16 and ecg_set_launch's variant is not 2.

test_offsets_past_4GiB puts stripes 2^32 - 2048 bytes apart in an allocation of several GiB, of
which only windows around the cells (and where an offset cut to 32 bits would land) are ever
uploaded and compared."""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import test_gpu_csum_masked as cm
from tests import test_gpu_recover_masks as rm
from tests import test_gpu_recover_masks_ptrs as rmp
from tests import test_gpu_repair as rep
from tests import test_gpu_update_masks as um
from tests import test_gpu_verify as ver

N = 48
CELLS = [1, 16, 17, 48, 4096, 4096 + 16, 4099, 8192 + 48, 12288 + 20]
CELLS16 = [c for c in CELLS if c % 16 == 0]
STRIPES = [1, 2, 63, 64, 65, 130]
MAX_BYTES = 8 << 20         # S * (k+p) * C of one case
GUARD, FILL, ERASED, PRE = 256, 0xA5, 0x5A, 0xEE
SLACK = 24                  # cells
U64MAX = (1 << 64) - 1
CALLS = ["recover_masks", "recover_masks_ptrs", "csum_masked", "recover_masks_csum", "csum_mask", "update_masks",
         "verify", "repair"]
SEED0 = {c: 10000 * (i + 1) for i, c in enumerate(CALLS)}
RECOV_MODES = ["tight", "pad16", "padodd", "desc"]
CLIENT_MODES = ["tight", "pad16", "padodd", "gapped", "split", "desc"]
PTR_MODES = ["scattered", "desc", "swapped", "padded"]
CSUM_MASK_MODES = ["stripe_major", "cell_major", "stripe_major_padded", "cell_major_padded"]
MASKED_NAMES = {1: "ecg_crc_masked_kernel<crc16%s>", 2: "ecg_crc_masked_kernel<crc32%s>",
                3: "ecg_crc_masked_kernel<crc64%s>", 7: "ecg_adler_masked_kernel%s"}


# --------------------------------------------------------------------- the layout rig
class Arr:
    """S x n cells of C bytes placed by explicit strides: cell (s, c) at s*ss + c*cs from the
    array's base pointer; either stride may be negative."""

    def __init__(self, S, n, C, ss, cs):
        self.S, self.n, self.C, self.ss, self.cs = S, n, C, ss, cs

    def off(self, s, c):
        return s * self.ss + c * self.cs

    def offsets(self):
        return [self.off(s, c) for s in range(self.S) for c in range(self.n)]


def place(arrs, skew=0):
    """One allocation for arrays [(Arr, byte offset of its base from the first one's)]: guard,
    the cells, slack of 24 cells, guard.  -> (size, [offset of each base in the allocation]).
    The first base sits `skew` bytes off a 16-byte boundary (allocations are 256-byte aligned);
    no two cells may overlap."""
    C = arrs[0][0].C
    offs = sorted(rel + o for a, rel in arrs for o in a.offsets())
    assert all(b - a >= C for a, b in zip(offs, offs[1:])), "cells overlap"
    zero = GUARD + (-offs[0] + 15) // 16 * 16 + skew
    return zero + offs[-1] + C + SLACK * C + GUARD, [zero + rel for _, rel in arrs]


def merge(windows, size):
    out = []
    for lo, hi in sorted((max(0, lo), min(size, hi)) for lo, hi in windows):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [(lo, hi) for lo, hi in out]


class Mem:
    """The host image of one allocation, 0xA5 until cells are put into it.  windows = None: the
    whole allocation; else only those byte ranges of it exist on the host, are uploaded,
    downloaded and compared (an allocation too large to fill)."""

    def __init__(self, size, windows=None):
        self.size, self.far = size, windows is not None
        self.iv = merge(windows, size) if self.far else [(0, size)]
        self.img = [np.full(hi - lo, FILL, dtype=np.uint8) for lo, hi in self.iv]

    def at(self, off, n):
        for (lo, hi), a in zip(self.iv, self.img):
            if lo <= off and off + n <= hi:
                return a[off - lo:off - lo + n]
        raise AssertionError(f"bytes {off}..{off + n} lie in no window")

    def copy(self):
        m = Mem.__new__(Mem)
        m.size, m.far, m.iv, m.img = self.size, self.far, self.iv, [a.copy() for a in self.img]
        return m

    def put(self, base, arr, cells):
        """cells [S][n][C] into the places of arr."""
        for s in range(arr.S):
            for c in range(arr.n):
                self.at(base + arr.off(s, c), arr.C)[:] = cells[s, c]

    @staticmethod
    def of(arr):
        """A whole allocation that is to hold `arr`."""
        m = Mem(arr.size)
        m.img[0][:] = arr
        return m


class Device:
    """The device buffers of one case, freed on the way out whatever happened."""

    def __init__(self, ctx, ecglib):
        self.ctx, self.ecglib, self.bufs = ctx, ecglib, []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()

    def alloc(self, n, fill=None):
        b = self.ctx.alloc(n)
        self.bufs.append(b)
        if fill is not None:
            b.fill(fill)
        return b

    def load(self, mem):
        """The allocation of `mem` with its windows uploaded.  Only an allocation of several
        GiB that the device refuses skips."""
        try:
            b = self.alloc(mem.size)
        except self.ecglib.EcgError as e:
            if mem.far:
                pytest.skip(f"no {mem.size >> 20} MiB of device memory: {e}")
            raise
        for (lo, _), a in zip(mem.iv, mem.img):
            b.upload(a, lo)
        return b

    def words(self, seq, dtype=np.uint32):
        a = np.array(seq, dtype=dtype)
        b = self.alloc(max(a.nbytes, 4))
        if a.size:
            b.upload(a.view(np.uint8))
        return b


def same(buf, want, what, name):
    """The whole allocation (every window of a far one) against its host image."""
    for (lo, hi), a in zip(want.iv, want.img):
        bad = np.flatnonzero(buf.download(hi - lo, lo) != a)
        assert bad.size == 0, f"{what}: {name}: {bad.size} bytes differ, first at {lo + int(bad[0])}"


def read_words(buf, dtype, n=None):
    return [int(v) for v in buf.download().view(dtype)[:n]]


def uncached(cache, fn, *args):
    """A reference of one of the calls' own modules for one case; it is not kept in that
    module's cache, which lives as long as the session."""
    had = set(cache)
    out = fn(*args)
    for key in set(cache) - had:
        del cache[key]
    return out


def launch(ctx, d, fn):
    ctx.set_launch(d.gx, d.gy, d.variant)
    try:
        fn()
        ctx.sync()
    finally:
        ctx.set_launch(0, 0, 0)


# --------------------------------------------------------------------------- the draw
def pad_of(rng, mode):
    if mode == "pad16":
        return 16 * int(rng.choice([1, 2, 3, 17, 100, 256]))        # 16 .. 4096
    if mode == "padodd":
        return int(rng.choice([4, 8, 12, 1, 3, 7, 21, 4097]))
    return 0


def bits(cells):
    return sum(1 << int(c) for c in cells)


def draw_common(rng, seed, shapes, mode, nops, need_rows=False):
    """What every call draws: the shape, the launch overrides and one operand's skew.  A
    pad-odd case keeps C, the pointers and the variant out of the lane choice: the stride alone
    is to make it."""
    d = SimpleNamespace(mode=mode)
    d.k, d.p = (int(v) for v in shapes[int(rng.integers(len(shapes)))])
    cells = CELLS16 if mode == "padodd" else CELLS
    d.C = cells[seed // 2 % len(cells)]     # every size in turn, whatever the mode (seed % 4 or % 6)
    while True:
        fits = [S for S in STRIPES if S * (d.k + d.p) * d.C <= MAX_BYTES]
        if not need_rows or fits[-1] >= 63:
            break
        d.C = int(rng.choice(cells))
    if need_rows:
        fits = [S for S in fits if S >= 63]
    d.S = fits[int(rng.integers(len(fits)))]
    d.gx, d.gy = (int(rng.choice([0, 1, 3])), int(rng.choice([0, 1, 2]))) if rng.integers(2) else (0, 0)
    d.variant = 2 if rng.integers(4) == 0 and mode != "padodd" else 0
    d.skews = [0] * nops
    if rng.integers(4) == 0 and mode != "padodd":
        d.skews[int(rng.integers(nops))] = int(rng.integers(1, 16))
    return d


def draw_words(rng, S, limit, maxbits):
    """One word per stripe: valid sets (1 .. maxbits cells below limit), 0, too many bits, a bit
    at or above limit, raw 32-bit words."""
    out = []
    for _ in range(S):
        u = rng.random()
        if u < 0.45:
            m = bits(rng.choice(limit, int(rng.integers(1, maxbits + 1)), replace=False))
        elif u < 0.65:
            m = 0
        elif u < 0.75 and maxbits < limit:
            m = bits(rng.choice(limit, int(rng.integers(maxbits + 1, limit + 1)), replace=False))
        elif u < 0.87:
            m = bits(rng.choice(limit, int(rng.integers(0, maxbits + 1)), replace=False)) | 1 << int(
                rng.integers(limit, 32))
        else:
            m = int(rng.integers(0, 1 << 32))
        out.append(m)
    return out


def word_kinds(words, is_valid):
    """(valid, invalid, zero) counts."""
    v = sum(1 for m in words if is_valid(m))
    z = sum(1 for m in words if m == 0)
    return v, len(words) - v - z, z


def draw_recov(call, seed):
    """ecg_recover_masks, ecg_csum_masked, ecg_recover_masks_csum: stripes [S][k+p][C] at a free
    stripe stride."""
    rng = np.random.default_rng(SEED0[call] + seed)
    mode = RECOV_MODES[seed % len(RECOV_MODES)]
    d = draw_common(rng, seed, rm.SHAPES, mode, 1 if call == "recover_masks" else 2)
    n = d.k + d.p
    d.stride = n * d.C + pad_of(rng, mode)
    if mode == "desc":
        d.stride = -(n * d.C + pad_of(rng, "pad16" if rng.integers(2) else "tight"))
    d.size, (d.base,) = place([(Arr(d.S, n, d.C, d.stride, d.C), 0)], d.skews[0])
    d.windows = None
    d.masks = draw_words(rng, d.S, n, d.p)
    d.flags = int(rng.integers(2))
    d.kinds = word_kinds(d.masks, lambda m: cm.valid(m, d.k, d.p))
    d.modes = {mode}
    d.ptrs, d.strides, d.rule_variant = [d.base], [d.stride], d.variant
    if call != "recover_masks":
        d.cskew = d.skews[1]
        d.htype = int(rng.choice(cm.TYPES))
        d.cs = int(rng.choice([4096, 1024] if mode == "padodd" else [4096, 1024, 100]))
        d.which = int(rng.integers(1, 4))
        d.src = ["none", "same", "separate"][int(rng.integers(3))]
        # the checksum kernels take no variant; their chunks start aligned only if the chunk size is too
        d.strides, d.rule_variant = [d.stride, d.cs], 0
    return d


def table_affine(offs, S, n, C):
    """ecg_recover_masks.c rmp_table: every entry is cells[0] + s*stride + c*C.  -> (affine, stride)"""
    st = offs[n] - offs[0] if S > 1 else n * C
    return all(offs[s * n + c] == offs[0] + s * st + c * C for s in range(S) for c in range(n)), st


def draw_ptrs(call, seed):
    """ecg_recover_masks_ptrs: a table of S*(k+p) addresses (d.offs, offsets in one allocation)."""
    rng = np.random.default_rng(SEED0[call] + seed)
    mode = PTR_MODES[seed % len(PTR_MODES)]
    pad = ("pad16", "padodd")[seed // len(PTR_MODES) % 2] if mode == "padded" else None
    d = draw_common(rng, seed, rm.SHAPES, "padodd" if pad == "padodd" else mode, 1, need_rows=mode == "swapped")
    d.mode = mode
    k, p, C, S = d.k, d.p, d.C, d.S
    n, skew = k + p, d.skews[0]
    if mode == "scattered":         # every cell in a slot of its own, slots shuffled; one cell skewed
        slot, perm = C + rmp.GAP, rng.permutation(S * n)
        d.offs = [GUARD + int(perm[i]) * slot for i in range(S * n)]
        d.offs[int(rng.integers(S * n))] += skew
    elif mode == "padded":          # an ascending image at a padded stride: affine
        stride = n * C + pad_of(rng, pad)
        d.offs = [GUARD + skew + s * stride + c * C for s in range(S) for c in range(n)]
    else:                           # a tight image, rows in falling address order; swapped: two exchanged
        order = list(range(S))
        if mode == "swapped":
            order[0], order[1] = 1, 0
        top = GUARD + skew + (S - 1) * n * C
        d.offs = [top - s * n * C + c * C for s in order for c in range(n)]
    assert all(b - a >= C for a, b in zip(sorted(d.offs), sorted(d.offs)[1:])), "cells overlap"
    d.size = max(d.offs) + C + SLACK * C + GUARD
    d.masks = draw_words(rng, S, n, p)
    d.flags = int(rng.integers(2))
    d.kinds = word_kinds(d.masks, lambda m: cm.valid(m, k, p))
    d.modes = {mode}
    d.affine, stride = table_affine(d.offs, S, n, C)
    d.ptrs, d.strides = ([d.offs[0]], [stride]) if d.affine else (d.offs, [])
    d.rule_variant = d.variant
    return d


def draw_client_strides(rng, mode, k, p, C, S):
    """The three strides of the client-layout calls.  -> (data stripe stride, parity cell stride,
    parity stripe stride, the parity lies in the data's buffer at + k*C, the modes present)."""
    n = k + p
    if mode == "tight":             # the two layouts of the calls' own tests
        if rng.integers(2):
            return n * C, C, n * C, True, {"tight"}
        return k * C, S * C, C, False, {"tight"}
    if mode in ("pad16", "padodd"):     # each stride on its own: padded or tight, one at least padded
        which = [bool(rng.integers(2)) for _ in range(3)]
        which[int(rng.integers(3))] = True
        pd = [pad_of(rng, mode) if w else 0 for w in which]
        pss = C + pd[1]
        return k * C + pd[0], S * pss + pd[2], pss, False, {mode} | (set() if all(which) else {"tight"})
    if mode == "gapped":            # parity rows with gaps between the cells and between the rows
        unit = "pad16" if rng.integers(4) else "padodd"
        pss = C + pad_of(rng, unit)
        return (k * C + (pad_of(rng, "pad16") if rng.integers(2) else 0), S * pss + pad_of(rng, unit), pss, False,
                {"gapped"})
    if mode == "split":             # data tight; parity [S][p][C] in a buffer of its own
        return k * C, C, p * C + (pad_of(rng, "pad16") if rng.integers(2) else 0), False, {"split"}
    assert mode == "desc"
    pad = pad_of(rng, "pad16") if rng.integers(2) else 0
    if rng.integers(2):             # the recovery layout, stripes falling
        return -(n * C + pad), C, -(n * C + pad), True, {"desc"}
    pss = C + pad                   # the client layout, stripes and parity rows falling
    return -(k * C + pad), -(S * pss + pad), -pss, False, {"desc"}


def client_rule(d):
    """What the lane choice of ecg_verify / ecg_repair looks at (kernels/ecg_mm_dev.h
    align_granule over r * parity_cell_stride, r < p: one parity row is addressed by no cell
    stride)."""
    return [d.dbase, d.pbase], [d.dss, d.pss] + ([d.pcs] if d.p > 1 else [])


def draw_scrub(call, seed):
    """ecg_verify and ecg_repair: data [S][k][C] and parity rows at three free strides, and per
    stripe what is wrong with it."""
    rng = np.random.default_rng(SEED0[call] + seed)
    mode = CLIENT_MODES[seed % len(CLIENT_MODES)]
    d = draw_common(rng, seed, ver.SHAPES if call == "verify" else rep.SHAPES, mode, 2)
    k, p, C, S = d.k, d.p, d.C, d.S
    d.dss, d.pcs, d.pss, d.same_buf, d.modes = draw_client_strides(rng, mode, k, p, C, S)
    data, par = Arr(S, k, C, d.dss, C), Arr(S, p, C, d.pss, d.pcs)
    if d.same_buf:
        d.dsize, (d.dbase, d.pbase) = place([(data, 0), (par, k * C)], d.skews[0])
        d.psize = 0
    else:
        d.dsize, (d.dbase,) = place([(data, 0)], d.skews[0])
        d.psize, (d.pbase,) = place([(par, 0)], d.skews[1])
    d.dwin = d.pwin = None
    d.hits = []                     # (kind, cell, second cell, where the wrong bytes lie, seed of the bytes)
    for _ in range(S):
        u = rng.random()
        kind = "clean" if u < 0.3 else "data" if u < 0.55 else "parity" if u < 0.75 else "two"
        a, b = (int(v) for v in rng.choice(k + p, 2, replace=False))
        if kind == "data":
            a = int(rng.integers(k))
        elif kind == "parity":
            a = k + int(rng.integers(p))
        d.hits.append((kind, a, b, ["first", "last", "whole"][int(rng.integers(3))], int(rng.integers(1 << 31))))
    kinds = [h[0] for h in d.hits]
    d.kinds = (kinds.count("data") + kinds.count("parity"), kinds.count("two"), kinds.count("clean"))
    (d.ptrs, d.strides), d.rule_variant = client_rule(d), d.variant
    return d


def draw_update(call, seed):
    """ecg_update_masks: old and new images [S][k][C] at one free stride, parity rows at two."""
    rng = np.random.default_rng(SEED0[call] + seed)
    mode = CLIENT_MODES[seed % len(CLIENT_MODES)]
    d = draw_common(rng, seed, um.SHAPES, mode, 3)
    k, p, C, S = d.k, d.p, d.C, d.S
    d.uss, d.pcs, d.pss, d.same_buf, d.modes = draw_client_strides(rng, mode, k, p, C, S)
    upd, par = Arr(S, k, C, d.uss, C), Arr(S, p, C, d.pss, d.pcs)
    if d.same_buf:
        d.osize, (d.obase, d.pbase) = place([(upd, 0), (par, k * C)], d.skews[0])
        d.psize = 0
    else:
        d.osize, (d.obase,) = place([(upd, 0)], d.skews[0])
        d.psize, (d.pbase,) = place([(par, 0)], d.skews[2])
    d.nsize, (d.nbase,) = place([(upd, 0)], d.skews[1])
    d.owin = d.nwin = d.pwin = None
    d.masks = draw_words(rng, S, k, k)
    d.packed = not d.same_buf and bool(rng.integers(2))     # the old image of the recovery layout is never packed
    d.flags = int(rng.integers(2)) | (2 if d.packed else 0)
    d.kinds = word_kinds(d.masks, lambda m: um.valid(m, k))
    d.ptrs, d.strides, d.rule_variant = [d.obase, d.nbase, d.pbase], [d.uss, d.pcs, d.pss], d.variant
    return d


def draw_csum_mask(call, seed):
    """ecg_csum_mask: two arrays of checksums, checksum c of cell i of stripe s at index
    s*ss + i*cs + c; both strides free, counted in checksums."""
    rng = np.random.default_rng(SEED0[call] + seed)
    mode = CSUM_MASK_MODES[seed % len(CSUM_MASK_MODES)]
    d = SimpleNamespace(mode=mode, modes={mode})
    d.htype = int(rng.choice(cm.TYPES))
    d.ncells = int(rng.integers(1, 25))
    d.first = int(rng.integers(0, 33 - d.ncells))
    d.nch = int(rng.choice([1, 2, 3, 5]))
    d.S = int(rng.choice(STRIPES))
    a, b = (int(rng.integers(1, 4)), int(rng.integers(0, 8))) if mode.endswith("padded") else (0, 0)
    if mode.startswith("stripe_major"):
        d.cs = d.nch + a
        d.ss = d.ncells * d.cs + b
    else:
        d.ss = d.nch + a
        d.cs = d.S * d.ss + b
    d.count = (d.S - 1) * d.ss + (d.ncells - 1) * d.cs + d.nch
    d.skews = [int(rng.integers(16)) if rng.integers(2) else 0 for _ in range(2)]     # of got, of want
    nhit = int(rng.integers(0, 13))
    d.hitlist = [(int(rng.integers(d.S)), int(rng.integers(d.ncells)), int(rng.integers(d.nch)),
                  int(rng.integers(cm.CL[d.htype])), int(rng.integers(8))) for _ in range(nhit)]
    d.preset = [int(rng.integers(1 << 32)) if rng.integers(2) else 0 for _ in range(d.S)]
    d.data_seed = int(rng.integers(1 << 31))
    return d


DRAW = {"recover_masks": draw_recov, "csum_masked": draw_recov, "recover_masks_csum": draw_recov,
        "recover_masks_ptrs": draw_ptrs, "csum_mask": draw_csum_mask, "update_masks": draw_update,
        "verify": draw_scrub, "repair": draw_scrub}


def draw(call, seed):
    d = DRAW[call](call, seed)
    d.call, d.seed = call, seed
    return d


# ------------------------------------------------------------------------- the predict
def lane(d):
    """The header's rule: the 16-byte lane kernel iff every pointer, every stride the call is
    given and C are multiples of 16 and the variant is not 2 (pointers as offsets in a 256-byte
    aligned allocation)."""
    return d.rule_variant != 2 and all(v % 16 == 0 for v in [d.C, *d.ptrs, *d.strides])


def stride_alone(d):
    """The byte kernel chosen by a stride alone."""
    return (d.rule_variant != 2 and d.C % 16 == 0 and all(v % 16 == 0 for v in d.ptrs)
            and any(v % 16 for v in d.strides))


def predict(d, call=None):
    call = call or d.call
    if call == "csum_mask":
        return "ecg_csum_mask_kernel"
    ln = lane(d)
    if call == "recover_masks":
        return rm.kernel_name(d.k, d.p) if ln else "ecg_recover_masks_byte_kernel"
    if call == "recover_masks_ptrs":
        if d.affine:                # the strided call itself
            return rm.kernel_name(d.k, d.p) if ln else "ecg_recover_masks_byte_kernel"
        return rmp.ptr_kernel(d.k, d.p) if ln else rmp.BYTE_KERNEL
    if call in ("csum_masked", "recover_masks_csum"):       # the composite's last launch is a checksum launch
        return MASKED_NAMES[d.htype] % ("" if ln else ",bytes" if d.htype != 7 else "<bytes>")
    if call == "update_masks":
        return um.lane_kernel(d.p) if ln else um.BYTE_KERNEL
    if call == "verify":
        return ver.kernel_name(d.k, d.p) if ln else "ecg_verify_byte_kernel"
    assert call == "repair"
    return rep.kernel_name(d.k) if ln else "ecg_repair_byte_kernel"


def describe(d):
    skip = ("windows", "dwin", "pwin", "owin", "nwin", "ptrs")
    return f"{d.call} seed {d.seed}: " + " ".join(f"{k}={v}" for k, v in vars(d).items() if k not in skip)


# ---------------------------------------------------------------- 3. the draw is worth running
def test_draw_covers_every_class():
    """Host only: over the 48 seeds of each call the draw meets every class the GPU tests are
    there for.  Conditions on the draw, not measurements."""
    for call in CALLS:
        ds = [draw(call, seed) for seed in range(N)]
        modes = {"csum_mask": CSUM_MASK_MODES, "recover_masks_ptrs": PTR_MODES, "update_masks": CLIENT_MODES,
                 "verify": CLIENT_MODES, "repair": CLIENT_MODES}.get(call, RECOV_MODES)
        for m in modes:
            assert sum(1 for d in ds if m in d.modes) >= 4, (call, m)
        assert sum(1 for d in ds if d.S >= 63) >= 10, call
        assert {d.S for d in ds} == set(STRIPES), call
        if call == "csum_mask":     # one kernel, no flags, no grid; its words are checksum differences
            assert sum(1 for d in ds if not d.hitlist) >= 1 and sum(1 for d in ds if len(d.hitlist) >= 6) >= 10
            assert sum(1 for d in ds if any(d.skews)) >= 10
            assert {d.htype for d in ds} == set(cm.TYPES)
            continue
        names = [predict(d) for d in ds]
        nlane = sum(1 for d in ds if lane(d))
        assert nlane >= 6 and N - nlane >= 6, (call, nlane)
        assert sum(1 for n in names if "byte" in n) == N - nlane, call
        assert sum(1 for d in ds if stride_alone(d)) >= 3, call
        assert {d.C for d in ds} == set(CELLS), call
        assert any(d.k not in (2, 4, 8, 16) for d in ds), call
        assert sum(1 for d in ds if d.gx or d.gy) >= 8, call
        assert sum(1 for d in ds if d.variant == 2) >= 4 and sum(1 for d in ds if any(d.skews)) >= 4, call
        if call not in ("verify", "repair"):
            assert sum(1 for d in ds if d.flags & 1) >= 10 and sum(1 for d in ds if not d.flags & 1) >= 10, call
        if call == "update_masks":
            assert sum(1 for d in ds if d.packed) >= 6
            assert max(d.p for d in ds) == 8
        if call == "recover_masks_ptrs":
            assert all(d.affine == (d.mode in ("desc", "padded")) for d in ds)
            assert sum(1 for d in ds if d.mode == "desc" and d.S > 1) >= 4
        if call in ("csum_masked", "recover_masks_csum"):
            assert {d.htype for d in ds} == set(cm.TYPES) and {d.which for d in ds} == {1, 2, 3}
            assert {d.src for d in ds} == {"none", "same", "separate"}
        valid, invalid, zero = (sum(d.kinds[i] for d in ds) for i in range(3))
        total = valid + invalid + zero
        assert total == sum(d.S for d in ds)
        assert 3 * valid >= total and 10 * invalid >= total and 10 * zero >= total, (call, valid, invalid, zero)
    # the rule itself, on hand-made draws
    d = SimpleNamespace(C=4096, ptrs=[256], strides=[6 * 4096 + 16], rule_variant=0)
    assert lane(d) and not stride_alone(d)
    d.strides = [-(6 * 4096 + 32)]
    assert lane(d)
    d.strides = [6 * 4096 + 4]
    assert not lane(d) and stride_alone(d)
    d.ptrs = [257]
    assert not lane(d) and not stride_alone(d)
    assert table_affine([300, 310, 200, 210, 100, 110], 3, 2, 10) == (True, -100)
    assert table_affine([200, 210, 300, 310, 100, 110], 3, 2, 10)[0] is False


# ------------------------------------------------------------------- 2. one run per call
def run_recov(ctx, oracle, ecglib, d, call):
    """ecg_recover_masks, ecg_csum_masked or ecg_recover_masks_csum on the stripes d places."""
    k, p, C, S = d.k, d.p, d.C, d.S
    n, what = k + p, describe(d)
    arr = Arr(S, n, C, d.stride, C)
    cw = uncached(rm._REF, rm.codewords, oracle, k, p, C, S)
    ok, rm_words = rm.model(d.masks, k, p)
    img = Mem(d.size, d.windows)
    img.put(d.base, arr, cw)
    want = img.copy()
    if call != "csum_masked":       # the cells the masks name are lost; a stripe left alone keeps them so
        for s, m in enumerate(d.masks):
            for c in rm.cells_of(m):
                if c < n:
                    img.at(d.base + arr.off(s, c), C)[:] = ERASED
                    if s not in ok:
                        want.at(d.base + arr.off(s, c), C)[:] = ERASED
    with Device(ctx, ecglib) as dev:
        buf, mk, res = dev.load(img), dev.words(d.masks), dev.alloc(32, 0xEE)
        ptr = buf.ptr + d.base
        assert buf.ptr % 256 == 0
        if call != "recover_masks":
            ref = uncached(cm._SUMS, cm.reference, oracle, ("fuzz", k, p, C, S), d.htype, d.cs, 1, cw)
            cbytes, cbase = ref.size, GUARD + d.cskew
            pre = np.full(cbase + cbytes + GUARD, FILL, dtype=np.uint8)
            pre[cbase:cbase + cbytes] = PRE
            sums = dev.alloc(pre.size)
            sums.upload(pre)
            src = sums if d.src == "same" else dev.alloc(pre.size) if d.src == "separate" else None
            if d.src == "separate":
                src.upload(pre)

            def sums_image(which):
                a = pre.copy()
                a[cbase:cbase + cbytes] = cm.expect_array(ref, d.masks, k, p, which).reshape(-1)
                return a
        name = []
        if call == "recover_masks":
            launch(ctx, d, lambda: (ctx.recover_masks(k, p, C, S, ptr, d.stride, mk.ptr, res.ptr, d.flags),
                                    name.append(ecglib.last_kernel())))
            want_words = rm_words
        elif call == "csum_masked":
            launch(ctx, d, lambda: (ctx.csum_masked(d.htype, d.cs, 1, k, p, C, S, ptr, d.stride, mk.ptr, d.which,
                                                    sums.ptr + cbase, res.ptr, d.flags),
                                    name.append(ecglib.last_kernel())))
            want_words = cm.words(d.masks, k, p, d.which)
            same(sums, Mem.of(sums_image(d.which)), what, "csums")
        else:
            launch(ctx, d, lambda: (ctx.recover_masks_csum(k, p, C, S, ptr, d.stride, mk.ptr, res.ptr, d.htype, d.cs,
                                                           1, sums.ptr + cbase, src.ptr + cbase if src else None,
                                                           d.flags),
                                    name.append(ecglib.last_kernel())))
            want_words = rm_words
            same(sums, Mem.of(sums_image(3 if d.src == "same" else 1)), what, "csums")
            if d.src == "separate":
                same(src, Mem.of(sums_image(2)), what, "src_csums")
        same(buf, want, what, "stripes")
        assert read_words(res, np.uint64) == want_words, what
        assert read_words(mk, np.uint32, S) == d.masks, what
        assert name[0] == predict(d, call), f"{what}: ran {name[0]}, predicted {predict(d, call)}"
    return name[0]


def run_ptrs(ctx, oracle, ecglib, d):
    k, p, C, S = d.k, d.p, d.C, d.S
    n, what = k + p, describe(d)
    cw = uncached(rm._REF, rm.codewords, oracle, k, p, C, S)
    ok, want_words = rm.model(d.masks, k, p)
    img = Mem(d.size)
    for s in range(S):
        for c in range(n):
            img.at(d.offs[s * n + c], C)[:] = cw[s, c]
    want = img.copy()
    for s, m in enumerate(d.masks):
        for c in rm.cells_of(m):
            if c < n:
                img.at(d.offs[s * n + c], C)[:] = ERASED
                if s not in ok:
                    want.at(d.offs[s * n + c], C)[:] = ERASED
    with Device(ctx, ecglib) as dev:
        buf, mk, res = dev.load(img), dev.words(d.masks), dev.alloc(32, 0xEE)
        assert buf.ptr % 256 == 0
        name = []
        launch(ctx, d, lambda: (ctx.recover_masks_ptrs(k, p, C, S, [buf.ptr + o for o in d.offs], mk.ptr, res.ptr,
                                                       d.flags),
                                name.append(ecglib.last_kernel())))
        same(buf, want, what, "cells")
        assert read_words(res, np.uint64) == want_words, what
        assert read_words(mk, np.uint32, S) == d.masks, what
        assert name[0] == predict(d), f"{what}: ran {name[0]}, predicted {predict(d)}"
        if d.mode == "desc":        # rows in falling address order are a strided image
            assert name[0] in (rm.kernel_name(k, p), "ecg_recover_masks_byte_kernel"), what
        if d.mode == "swapped":
            assert name[0] in (rmp.ptr_kernel(k, p), rmp.BYTE_KERNEL), what
    return name[0]


def classify(rows, cand, k, p):
    """The reading of a status word include/ecg.h gives for ecg_verify_cell."""
    if rows == 0:
        return -1
    if p < 2:
        return -2
    if bin(rows).count("1") == 1:
        return k + rows.bit_length() - 1
    if rows == (1 << p) - 1 and bin(cand).count("1") == 1:
        return cand.bit_length() - 1
    return -2


def corrupt(oracle, d, cw):
    """The stripes with what d.hits says is wrong with them.  -> (cells [S][k+p][C], the status
    word of every stripe from first principles, its reading).  Two wrong cells are chosen so
    that no single cell explains them: the second cell's one wrong byte takes the first value
    with which the model says so."""
    k, p, C = d.k, d.p, d.C
    bad = cw.copy()
    status, cells = [((1 << k) - 1) << 8] * d.S, [-1] * d.S

    def model(s):
        cols = np.flatnonzero((bad[s] != cw[s]).any(axis=0))
        return ver.model_status(oracle, k, p, bad[s, :k][:, cols], bad[s, k:][:, cols])

    for s, (kind, a, b, where, sub) in enumerate(d.hits):
        if kind == "clean":
            continue
        r = np.random.default_rng(sub)
        lo, hi = ((C - 1) // 4096 * 4096, C) if where == "last" else (0, min(C, 4096))
        if where == "whole":
            bad[s, a] ^= r.integers(1, 256, C, dtype=np.uint8)
        else:
            pos = np.unique(r.integers(lo, hi, int(r.integers(1, 4))))
            bad[s, a, pos] ^= r.integers(1, 256, pos.size, dtype=np.uint8)
        if kind == "two":
            at = int(r.integers(lo, hi))
            for eb in range(1, 256):
                bad[s, b, at] = cw[s, b, at] ^ eb
                rows, cand = model(s)
                if classify(rows, cand, k, p) == -2:
                    break
            else:
                raise AssertionError(f"{describe(d)}: stripe {s}: no error pair without a single-cell explanation")
        else:
            rows, cand = model(s)
        status[s], cells[s] = rep.st(rows, cand), classify(rows, cand, k, p)
    return bad, status, cells


def run_scrub(ctx, oracle, ecglib, d, repair):
    """ecg_verify, and with repair ecg_repair queued behind it with no sync in between."""
    k, p, C, S = d.k, d.p, d.C, d.S
    n, what = k + p, describe(d)
    data, par = Arr(S, k, C, d.dss, C), Arr(S, p, C, d.pss, d.pcs)
    cw = uncached(rm._REF, rm.codewords, oracle, k, p, C, S)
    bad, status, cells = corrupt(oracle, d, cw)
    D = Mem(d.dsize, d.dwin)
    P = D if d.same_buf else Mem(d.psize, d.pwin)
    D.put(d.dbase, data, bad[:, :k])
    P.put(d.pbase, par, bad[:, k:])
    wantD = D.copy()
    wantP = wantD if d.same_buf else P.copy()
    if repair:
        for s, c in enumerate(cells):
            if c >= 0:
                for j in range(k):
                    wantD.at(d.dbase + data.off(s, j), C)[:] = cw[s, j]
                for r in range(p):
                    wantP.at(d.pbase + par.off(s, r), C)[:] = cw[s, k + r]
    for s, (kind, a, _, _, _) in enumerate(d.hits):
        if kind == "clean":
            assert status[s] == ((1 << k) - 1) << 8 and cells[s] == -1, what
        elif kind != "two" and p >= 2:      # one wrong cell: every row for a data cell, its own for a parity row
            assert status[s] & 0xff == ((1 << p) - 1 if a < k else 1 << (a - k)) and cells[s] == a, (what, s)
        else:
            assert cells[s] == -2, (what, s)
    with Device(ctx, ecglib) as dev:
        dbuf = dev.load(D)
        pbuf = dbuf if d.same_buf else dev.load(P)
        st, vres, rres = dev.alloc(4 * S, 0xEE), dev.alloc(32, 0xEE), dev.alloc(32, 0xEE)
        args = (k, p, C, S, dbuf.ptr + d.dbase, d.dss, pbuf.ptr + d.pbase, d.pcs, d.pss, st.ptr)
        names = []

        def calls():
            ctx.verify(*args, vres.ptr)
            names.append(ecglib.last_kernel())
            if repair:
                ctx.repair(*args, rres.ptr)
                names.append(ecglib.last_kernel())

        launch(ctx, d, calls)
        got = read_words(st, np.uint32)
        for s in range(S):
            assert got[s] == status[s], f"{what}: stripe {s} ({d.hits[s][0]}): status {got[s]:#x}, model {status[s]:#x}"
            assert ecglib.verify_cell(got[s], k, p) == cells[s], (what, s)
        nbad = [s for s, c in enumerate(cells) if c != -1]
        left = [s for s, c in enumerate(cells) if c == -2]
        assert read_words(vres, np.uint64) == [len(nbad), min(nbad) if nbad else U64MAX, len(nbad) - len(left),
                                               len(left)], what
        if repair:
            assert read_words(rres, np.uint64) == [len(nbad) - len(left), min(left) if left else U64MAX,
                                                   sum(1 for c in cells if 0 <= c < k), len(left)], what
        same(dbuf, wantD, what, "data")
        if not d.same_buf:
            same(pbuf, wantP, what, "parity")
        assert names[0] == predict(d, "verify"), f"{what}: ran {names[0]}, predicted {predict(d, 'verify')}"
        if repair:
            assert names[1] == predict(d, "repair"), f"{what}: ran {names[1]}, predicted {predict(d, 'repair')}"
    return names[-1]


def run_update(ctx, oracle, ecglib, d):
    k, p, C, S = d.k, d.p, d.C, d.S
    what = describe(d)
    upd, par = Arr(S, k, C, d.uss, C), Arr(S, p, C, d.pss, d.pcs)
    old, new, par0 = uncached(um._REF, um.images, oracle, k, p, C, S)
    O, Nw = Mem(d.osize, d.owin), Mem(d.nsize, d.nwin)
    P = O if d.same_buf else Mem(d.psize, d.pwin)
    delta = np.zeros((S, k, C), dtype=np.uint8)
    for s, m in enumerate(d.masks):
        js = um.cells_of(m & ((1 << k) - 1)) if d.packed else list(range(k))
        for i, j in enumerate(js):      # packed: the cell of the i-th set bit in slot i, filler elsewhere
            O.at(d.obase + upd.off(s, i), C)[:] = old[s, j]
            Nw.at(d.nbase + upd.off(s, i), C)[:] = new[s, j]
        if um.valid(m, k):
            js = um.cells_of(m)
            delta[s, js] = old[s, js] ^ new[s, js]
    P.put(d.pbase, par, par0.transpose(1, 0, 2))
    want = P.copy()
    enc = oracle.encode_batch(k, p, C, S, delta.reshape(-1)).reshape(p, S, C)
    for s in range(S):
        for r in range(p):
            want.at(d.pbase + par.off(s, r), C)[:] ^= enc[r, s]
    with Device(ctx, ecglib) as dev:
        obuf, nbuf = dev.load(O), dev.load(Nw)
        pbuf = obuf if d.same_buf else dev.load(P)
        mk, res = dev.words(d.masks), dev.alloc(32, 0xEE)
        name = []
        launch(ctx, d, lambda: (ctx.update_masks(k, p, C, S, obuf.ptr + d.obase, nbuf.ptr + d.nbase, d.uss,
                                                 pbuf.ptr + d.pbase, d.pcs, d.pss, mk.ptr, res.ptr, d.flags),
                                name.append(ecglib.last_kernel())))
        same(pbuf, want, what, "parity")
        if not d.same_buf:
            same(obuf, O, what, "old image")
        same(nbuf, Nw, what, "new image")
        assert read_words(res, np.uint64) == um.model(d.masks, k), what
        assert read_words(mk, np.uint32, S) == d.masks, what
        assert name[0] == predict(d, "update_masks"), f"{what}: ran {name[0]}, predicted {predict(d, 'update_masks')}"
    return name[0]


def run_csum_mask(ctx, oracle, ecglib, d):
    """Checksums are opaque to the comparison: random bytes, single bits flipped at the drawn
    (stripe, cell, chunk) places; the gaps the strides open differ between the two arrays in
    every byte, so a checksum read from a gap sets a bit."""
    what, cl = describe(d), cm.CL[d.htype]
    rng = np.random.default_rng(d.data_seed)
    got = np.full((d.count, cl), FILL, dtype=np.uint8)
    wnt = np.full((d.count, cl), ERASED, dtype=np.uint8)
    expect = list(d.preset)
    for s in range(d.S):
        for i in range(d.ncells):
            at = s * d.ss + i * d.cs
            got[at:at + d.nch] = wnt[at:at + d.nch] = rng.integers(0, 256, (d.nch, cl), dtype=np.uint8)
    for s, i, c, byte, bit in d.hitlist:
        got[s * d.ss + i * d.cs + c, byte] ^= 1 << bit
    for s in range(d.S):            # numpy: which cells differ
        for i in range(d.ncells):
            at = s * d.ss + i * d.cs
            if (got[at:at + d.nch] != wnt[at:at + d.nch]).any():
                expect[s] |= 1 << (d.first + i)
    imgs = []
    for a, skew in zip((got, wnt), d.skews):
        m = Mem(GUARD + skew + a.size + GUARD)
        m.at(GUARD + skew, a.size)[:] = a.reshape(-1)
        imgs.append(m)
    with Device(ctx, ecglib) as dev:
        gbuf, wbuf, mk = dev.load(imgs[0]), dev.load(imgs[1]), dev.words(d.preset)
        ctx.csum_mask(d.htype, gbuf.ptr + GUARD + d.skews[0], wbuf.ptr + GUARD + d.skews[1], d.S, d.ncells, d.nch,
                      d.ss, d.cs, d.first, mk.ptr)
        name = ecglib.last_kernel()
        ctx.sync()
        assert read_words(mk, np.uint32, d.S) == expect, what
        same(gbuf, imgs[0], what, "got")
        same(wbuf, imgs[1], what, "want")
        assert name == predict(d), what
    return name


RUN = {"recover_masks": lambda *a: run_recov(*a, "recover_masks"),
       "csum_masked": lambda *a: run_recov(*a, "csum_masked"),
       "recover_masks_csum": lambda *a: run_recov(*a, "recover_masks_csum"),
       "recover_masks_ptrs": run_ptrs, "csum_mask": run_csum_mask, "update_masks": run_update,
       "verify": lambda *a: run_scrub(*a, False), "repair": lambda *a: run_scrub(*a, True)}


def run_case(ctx, oracle, ecglib, d):
    """One case; an error the library reports names the seed and the draw like a failed assert."""
    try:
        return RUN[d.call](ctx, oracle, ecglib, d)
    except ecglib.EcgError as e:
        raise AssertionError(f"{describe(d)}: {e}") from e


def run_all(ctx, oracle, ecglib, call):
    kernels = {}
    for seed in range(N):
        got = run_case(ctx, oracle, ecglib, draw(call, seed))
        kernels[got] = kernels.get(got, 0) + 1
    print(call, "kernels:", kernels)
    return kernels


@pytest.mark.gpu
def test_recover_masks(ctx, oracle, ecglib):
    assert "ecg_recover_masks_byte_kernel" in run_all(ctx, oracle, ecglib, "recover_masks")


@pytest.mark.gpu
def test_recover_masks_ptrs(ctx, oracle, ecglib):
    kernels = run_all(ctx, oracle, ecglib, "recover_masks_ptrs")
    assert {"ecg_recover_masks_byte_kernel", rmp.BYTE_KERNEL} <= set(kernels), kernels


@pytest.mark.gpu
def test_csum_masked(ctx, oracle, ecglib):
    run_all(ctx, oracle, ecglib, "csum_masked")


@pytest.mark.gpu
def test_recover_masks_csum(ctx, oracle, ecglib):
    run_all(ctx, oracle, ecglib, "recover_masks_csum")


@pytest.mark.gpu
def test_csum_mask(ctx, oracle, ecglib):
    run_all(ctx, oracle, ecglib, "csum_mask")


@pytest.mark.gpu
def test_update_masks(ctx, oracle, ecglib):
    assert um.BYTE_KERNEL in run_all(ctx, oracle, ecglib, "update_masks")


@pytest.mark.gpu
def test_verify(ctx, oracle, ecglib):
    assert "ecg_verify_byte_kernel" in run_all(ctx, oracle, ecglib, "verify")


@pytest.mark.gpu
def test_repair(ctx, oracle, ecglib):
    assert "ecg_repair_byte_kernel" in run_all(ctx, oracle, ecglib, "repair")


# --------------------------------------------------------------- 4. offsets past 4 GiB
FAR_K, FAR_P, FAR_C, FAR_S = 4, 2, 4096, 3      # EC_4P2
FAR_STRIDE = 2 ** 32 - 2048         # stripe 1's first cell straddles byte offset 2^32, stripe 2 lies beyond it
WINDOW = 64 << 10


def far_place(offs, C):
    """An allocation of which only windows exist on the host: every cell (at base + an offset of
    offs) with 64 KiB on each side, and 64 KiB where its offset cut to 32 bits would land.
    -> (size, base, windows)"""
    base, win = WINDOW, []
    for o in offs:
        win.append((base + o - WINDOW, base + o + C + WINDOW))
        win.append((base + o % 2 ** 32, base + o % 2 ** 32 + WINDOW))
    return base + max(offs) + C + WINDOW, base, win


def far_case(call, layout, stride):
    k, p, C, S = FAR_K, FAR_P, FAR_C, FAR_S
    n = k + p
    d = SimpleNamespace(call=call, seed=f"far-{layout}", k=k, p=p, C=C, S=S, gx=0, gy=0, variant=0, flags=0,
                        rule_variant=0, mode=layout)
    image = [s * stride + c * C for s in range(S) for c in range(n)]       # stripes [S][k+p][C], far apart
    rows = [r * stride + s * C for r in range(p) for s in range(S)]         # parity [p][S][C], rows far apart
    if call in ("recover_masks", "csum_masked", "recover_masks_csum"):
        d.stride = stride
        d.size, d.base, d.windows = far_place(image, C)
        d.masks = [0b100001, 0b000010, 0b010100]
        d.cskew, d.htype, d.cs, d.which, d.src = 0, 2, 4096, 3, "same"
        d.ptrs, d.strides = [d.base], [stride, d.cs]
        return d
    if layout == "stripes":         # the recovery layout: data and parity of a stripe together
        ss, d.pcs, d.pss, d.same_buf = stride, C, stride, True
        size, base, win = far_place(image, C)
        sizes, bases, wins = [size, 0], [base, base + k * C], [win, None]
    else:                           # the client layout: data tight, parity rows far apart
        ss, d.pcs, d.pss, d.same_buf = k * C, stride, C, False
        size, (base,) = place([(Arr(S, k, C, ss, C), 0)])
        psize, pbase, pwin = far_place(rows, C)
        sizes, bases, wins = [size, psize], [base, pbase], [None, pwin]
    if call == "update_masks":
        d.uss, d.masks, d.packed = ss, [0b0101, 0b1000, 0b0011], False
        (d.osize, d.psize), (d.obase, d.pbase), (d.owin, d.pwin) = sizes, bases, wins
        if layout == "stripes":
            d.nsize, d.nbase, d.nwin = far_place([s * stride + j * C for s in range(S) for j in range(k)], C)
        else:
            d.nsize, d.nbase, d.nwin = d.osize, d.obase, None
        d.ptrs, d.strides = [d.obase, d.nbase, d.pbase], [d.uss, d.pcs, d.pss]
    else:
        d.dss = ss
        (d.dsize, d.psize), (d.dbase, d.pbase), (d.dwin, d.pwin) = sizes, bases, wins
        d.hits = [("data", 1, 0, "first", 11), ("parity", k + 1, 0, "last", 12), ("data", k - 1, 0, "whole", 13)]
        d.ptrs, d.strides = client_rule(d)
    return d


FAR = [("recover_masks", "stripes"), ("csum_masked", "stripes"), ("recover_masks_csum", "stripes"),
       ("update_masks", "stripes"), ("update_masks", "rows"), ("verify", "stripes"), ("verify", "rows"),
       ("repair", "stripes"), ("repair", "rows")]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["lane", "byte"])
@pytest.mark.parametrize("call,layout", FAR)
def test_offsets_past_4GiB(ctx, oracle, ecglib, call, layout, kernel):
    """A stripe stride ("stripes"; about 8.6 GiB per image, two of them for ecg_update_masks) or
    a parity cell stride ("rows", about 4.3 GiB) of 2^32 - 2048, + 4 for the byte kernels.
    Skips only if the device refuses the allocation."""
    d = far_case(call, layout, FAR_STRIDE + (0 if kernel == "lane" else 4))
    assert lane(d) == (kernel == "lane")
    name = run_case(ctx, oracle, ecglib, d)
    assert ("byte" in name) == (kernel == "byte"), name
