"""Seeded random byte movement through the scatter-gather calls: the segment copies of
ecg_copy_segs_kernel (reached through the single-value fill-back), the gather walk of the client
encode (ecg_obj_ec_recx_encode) and the array fill-back (ecg_obj_ec_recov_fill_back after
ecg_recover), byte for byte against oracle/sgl_py.py, the CPU codec and plain numpy.

The calls' own modules (test_gpu_sgl.py, test_recx_encode_sgl in test_gpu_ptrs.py) are a dozen
hand-picked cases; here the addressing is drawn: every iov at its own byte skew with an odd gap
to the next, the source skew, segment lengths around the head / body / tail split and the
16 KiB tile, segment counts on both sides of the 64 and 4096 steps of the kernel's 64-ary
search, iovs that cut a cell into hundreds of pieces, empty iovs at the very front and back,
sgls shorter than what is to be copied, parity buffers at their own skews in either address
order.  The rig is test_gpu_fuzz_masks.py's: every allocation is 0xA5 where no payload lies,
has 256 guard bytes in front and behind, and is compared whole after the single sync -- the
destination, and the source too.

A draw is pure and host-only; one seed gives one case.  Where a seed is assigned a goal (a
length class together with an aligned or a misaligned source, a piece count) it is redrawn from
its own generator until it meets it, so the classes the host-only coverage tests ask for are
there by construction.  split / rounds / walk restate the kernel's segment split, its search
depth and the encode's gather walk only to classify the draws; no expected byte comes from
them.

The last two tests hand the two scratch slots of a fresh context between the encode (which keeps
its gathered cells in the slot's device half until the product has read them), the fill-back's
segment table and a pointer table, with no sync in between."""
import ctypes as ct
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import sgl_py
from tests.sgl_cases import expected_user_bytes, make_case, stripe_image, user_offsets
from tests.test_gpu_fuzz_masks import FILL, GUARD, Device, Mem, merge, same
from tests.test_gpu_ptrs import _oc

N = 48
MAX_BYTES = 8 << 20         # payload of one case
ERASED = 0x5A


def describe(d):
    """The draw without its long lists: scalars whole, of a list its length and its first entries."""
    def short(v):
        if isinstance(v, (list, tuple)) and len(v) > 8:
            return f"[{', '.join(str(x) for x in v[:8])}, ... {len(v)} in all]"
        return v

    skip = ("call", "seed", "case")
    return f"{d.call} seed {d.seed}: " + " ".join(f"{k}={short(v)}" for k, v in vars(d).items() if k not in skip)


def lay(rng, caps, skew, gap_hi):
    """iovs of the given capacities in one allocation: the first `skew` bytes off a 16-byte
    boundary behind the front guard, 1 .. gap_hi bytes between one and the next, a guard behind.
    -> (offsets, size)"""
    gaps = rng.integers(1, gap_hi + 1, len(caps)).tolist()
    offs, pos = [], GUARD + skew
    for cap, gap in zip(caps, gaps):
        offs.append(pos)
        pos += cap + gap
    return offs, pos + GUARD


def disjoint(offs, caps, size):
    """No two iovs touch, none reaches into a guard."""
    iv = [(o, o + c) for o, c in zip(offs, caps) if c]
    return merge(iv, size) == sorted(iv) and all(GUARD <= lo and hi <= size - GUARD for lo, hi in iv)


def device_sgl(ecglib, buf, offs, caps):
    iovs = (ecglib.Iov * max(1, len(caps)))(*[ecglib.Iov(buf.ptr + o, c, 0) for o, c in zip(offs, caps)])
    return iovs, ecglib.Sgl(len(caps), 0, iovs)


def sgl_image(size, offs, bufs):
    m = Mem(size)
    for o, b in zip(offs, bufs):
        m.at(o, len(b))[:] = b
    return m


# ------------------------------------------------------ A. segment copies (single-value fill-back)
COUNTS = [1, 2, 63, 64, 65, 200, 4096, 4097, 5000]
EXACT = (1, 2, 64, 65, 4096, 4097)      # counts that must reach the kernel as they are: no empty iov, no lost last one
TILE_WORDS = 256 * 4                    # CP_BLOCK * CP_WORDS: 16-byte words of a 16 KiB tile
CLASSES = ["head_only", "head_tail", "one_word", "w1023", "w1024", "w1025", "tiles"]
GOALS = [(c, al) for al in (False, True) for c in CLASSES]
SIZE_MODES = ["exact", "less", "more"]
SMALL = 40                              # the longest iov of a count >= 200, the few long ones apart


def split(dst, n):
    """ecg_copy_kernels.hip: (head bytes up to the first 16-byte boundary of dst, 16-byte body
    words, tail bytes) of a segment of n bytes."""
    head = min(-dst % 16, n)
    nw = (n - head) // 16
    return head, nw, n - head - 16 * nw


def length_class(dst, n):
    head, nw, tail = split(dst, n)
    if 0 < n < -dst % 16:
        return "head_only"
    if nw == 0:
        return "head_tail" if head and tail else "other"
    if nw in (1, TILE_WORDS - 1, TILE_WORDS, TILE_WORDS + 1):
        return {1: "one_word"}.get(nw, f"w{nw}")
    return "tiles" if nw > 2 * TILE_WORDS and nw % TILE_WORDS else "other"


def rounds(nseg):
    """Rounds of the kernel's 64-ary search over nseg segments: each one narrows the bracket to
    (nseg + 63) / 64 entries."""
    r = 0
    while nseg > 1:
        nseg, r = (nseg + 63) // 64, r + 1
    return r


def class_len(rng, cls, full_head):
    """A length of the class for a destination full_head bytes short of a 16-byte boundary;
    None where that destination has none."""
    if cls == "head_only":
        return int(rng.integers(1, full_head)) if full_head >= 2 else None
    if cls == "head_tail":
        return full_head + int(rng.integers(1, 16)) if full_head else None
    if cls == "short":
        return int(rng.integers(1, SMALL + 1))
    words = {"one_word": 1, "w1023": TILE_WORDS - 1, "w1024": TILE_WORDS, "w1025": TILE_WORDS + 1,
             "tiles": (2 + int(rng.integers(2))) * TILE_WORDS + int(rng.integers(1, TILE_WORDS))}[cls]
    return full_head + 16 * words + int(rng.integers(16))


def segments(d):
    """What the single-value walk makes of the draw: (dst offset, src offset, len) per non-empty
    iov, the source running on, cut where iod_size ends."""
    out, pos = [], 0
    for off, cap in zip(d.offs, d.caps):
        n = min(cap, d.iod_size - pos)
        if n > 0:
            out.append((off, d.src_skew + pos, n))
            pos += n
    return out


def classify_copy(d):
    """(class, source aligned) of every segment, the dst & 15 values met, the sh values met by
    segments that have body words (shift_pair's 4 x 4 cases, sh = 0 apart)."""
    d.combos, d.dst15, d.shs = set(), set(), set()
    segs = segments(d)
    for dst, src, n in segs:
        sh = (src + split(dst, n)[0]) % 16
        d.combos.add((length_class(dst, n), sh == 0))
        d.dst15.add(dst % 16)
        if split(dst, n)[1]:
            d.shs.add(sh)
    d.nseg, d.rounds = len(segs), rounds(len(segs))
    d.last_words = split(segs[-1][0], segs[-1][2])[1]
    by_off = {dst: split(dst, n)[1] for dst, _, n in segs}
    d.long_words = min(by_off.get(d.offs[i], 0) for i in d.long_at)


def draw_copy_once(rng, seed, n, goal):
    d = SimpleNamespace(call="copy_segs", seed=seed, n=n, goal=goal, size_mode=SIZE_MODES[seed // len(COUNTS) % 3])
    d.src_skew = int(rng.integers(16))
    step = (n + 63) // 64
    # of a long list only these are long: the ends, the middle, the last entry of the first bracket of
    # the search's first round and the first entry of its last one
    long_at = {0, n // 2, n - 1, step - 1, (n - 1) // step * step} if n >= 200 else set(range(n))
    goal_at = sorted(long_at)[int(rng.integers(len(long_at)))]
    free = CLASSES
    if n >= 200:                    # each of them has whole tiles; a goal without body words goes to a short one
        free = CLASSES[3:]
        if goal[0] not in free:
            goal_at = next(i for i in rng.permutation(n).tolist() if i not in long_at)
    d.caps, d.offs, d.long_at = [], [], sorted(long_at)
    pos, src = GUARD, d.src_skew
    for i in range(n):
        cls = goal[0] if i == goal_at else free[int(rng.integers(len(free)))] if i in long_at else "short"
        want_al = goal[1] if i == goal_at else rng.random() < 0.25
        if n not in EXACT and i != goal_at and (n < 200 or i not in long_at) and rng.random() < 0.04:
            cls = "empty"
        for _ in range(64 if i == goal_at else 8):  # a gap, a length of the class, the source aligned as wished
            gap = int(rng.integers(1, 41))
            ln = 0 if cls == "empty" else class_len(rng, cls, -(pos + gap) % 16)
            if ln is not None and (cls == "empty" or ((src + split(pos + gap, ln)[0]) % 16 == 0) == want_al):
                break
        else:
            if i == goal_at:
                return None
            ln = ln if ln is not None else class_len(rng, "short", 0)
        d.offs.append(pos + gap)
        d.caps.append(ln)
        pos, src = pos + gap + ln, src + ln
    d.size, d.total = pos + GUARD, sum(d.caps)
    few = int(rng.integers(1, 9))
    if d.size_mode == "less":       # the last iov part filled; of an exact count it still gets a byte
        few = min(few, d.caps[-1] - 1 if n in EXACT else d.total - 1)
    d.iod_size = d.total + {"exact": 0, "less": -few, "more": few}[d.size_mode]
    if d.iod_size <= 0:
        return None
    classify_copy(d)
    return d if goal in d.combos and d.total <= MAX_BYTES else None


def draw_copy(seed):
    rng = np.random.default_rng(30000 + seed)
    while True:
        d = draw_copy_once(rng, seed, COUNTS[seed % len(COUNTS)], GOALS[seed % len(GOALS)])
        if d is not None:
            return d


def test_copy_draw_covers_every_class():
    """Host only: what the 48 seeds of section A reach together."""
    ds = [draw_copy(seed) for seed in range(N)]
    assert set().union(*(d.dst15 for d in ds)) == set(range(16))
    assert set().union(*(d.shs for d in ds)) == set(range(16))
    combos = set().union(*(d.combos for d in ds))
    for goal in GOALS:
        assert goal in combos, goal
    assert {d.n for d in ds} == set(COUNTS)
    assert set(EXACT) <= {d.nseg for d in ds}
    assert {1, 2, 3} <= {d.rounds for d in ds}
    for r in (2, 3):                # a tile of body words on the last segment, found through r rounds
        assert any(d.rounds == r and d.last_words >= 1 for d in ds), r
    assert {d.size_mode for d in ds if d.rounds == 3} == set(SIZE_MODES)
    assert any(0 in d.caps for d in ds)
    for d in ds:
        assert disjoint(d.offs, d.caps, d.size) and 0 < d.iod_size and d.total <= MAX_BYTES, describe(d)
        if d.n >= 200:              # cheap: all short but the handful, and each of those has a whole tile
            assert sum(1 for c in d.caps if c > SMALL) <= 6 and d.long_words >= TILE_WORDS - 1, describe(d)
    # the restated rules on hand-made values
    assert split(256 + 3, 5) == (5, 0, 0) and split(256 + 3, 13 + 32 + 2) == (13, 2, 2) and split(256, 15) == (0, 0, 15)
    assert length_class(259, 12) == "head_only" and length_class(259, 13) == "other"
    assert length_class(259, 20) == "head_tail" and length_class(256, 16 * 1024) == "w1024"
    assert length_class(256, 16 * 2048) == "other" and length_class(256, 16 * 2049 + 1) == "tiles"
    assert [rounds(n) for n in (1, 2, 64, 65, 4096, 4097, 5000)] == [0, 1, 1, 2, 2, 3, 3]


class CopyCase:
    """One single-value fill-back: d.iod_size source bytes into the iovs d lays out."""

    def __init__(self, d):
        self.d, self.what = d, describe(d)
        data = np.random.default_rng(31000 + d.seed).integers(0, 256, max(d.iod_size, d.total), dtype=np.uint8)
        self.S = Mem(GUARD + 16 + data.size + GUARD)
        self.S.at(GUARD + d.src_skew, data.size)[:] = data
        self.D = Mem(d.size)
        # consecutive source bytes into the iov ranges, nothing of the walk
        self.want, pos = self.D.copy(), 0
        for off, cap in zip(d.offs, d.caps):
            n = max(0, min(cap, d.iod_size - pos))
            self.want.at(off, n)[:] = data[pos:pos + n]
            pos += n
        self.ref = sgl_py.Sgl([np.full(c, FILL, np.uint8) for c in d.caps])
        sgl_py.recov_fill_back(d.iod_size, [], self.ref, [], [], data, 0, 1, singv=True)
        walked = sgl_image(d.size, d.offs, self.ref.bufs)
        assert np.array_equal(walked.img[0], self.want.img[0]), f"{self.what}: sgl_py and the numpy image differ"

    def load(self, dev, ecglib):
        self.sbuf, self.dbuf = dev.load(self.S), dev.load(self.D)
        assert self.sbuf.ptr % 256 == 0 and self.dbuf.ptr % 256 == 0
        self.iovs, self.sgl = device_sgl(ecglib, self.dbuf, self.d.offs, self.d.caps)

    def call(self, ctx, ecglib, stream=None):
        rc = ecglib.lib().ecg_obj_ec_recov_fill_back(ctx.h, self.d.iod_size, 1, None, 0, ct.byref(self.sgl), None, 0,
                                                     None, 0, self.sbuf.ptr + GUARD + self.d.src_skew, 0, 1, stream)
        assert rc == 0, f"{self.what}: {ecglib.lib().ecg_strerror()}"
        self.kernel = ecglib.last_kernel()

    def check(self):
        same(self.dbuf, self.want, self.what, "iovs")
        same(self.sbuf, self.S, self.what, "source")
        assert [self.iovs[i].iov_len for i in range(self.d.n)] == self.ref.iov_len, self.what
        assert self.sgl.sg_nr_out == self.ref.nr_out, self.what
        assert self.kernel == "ecg_copy_segs_kernel", f"{self.what}: ran {self.kernel}"


# ------------------------------------------------------------- B. the gather walk of the encode
KP = [(2, 1), (2, 2), (4, 1), (4, 2), (8, 1), (8, 2), (16, 1), (16, 2), (4, 3), (8, 3), (16, 3)]    # what _oc knows
CELLS = [1, 16, 17, 48, 1000, 4096, 4099, 8192 + 48]
SPLITS = ["one", "cell_multiples", "random", "tiny", "zeros", "slack"]
TINY_MAX = 512 << 10        # k*C*S of a tiny split: some ten thousand iovs at the most


def walk(caps, recxs, k, C):
    """ecg_ptrs.c sgl_walk, to classify: (gathered cells, pieces, most pieces of one cell).  A
    cell the current iov holds whole is used in place, any other is gathered piece by piece."""
    cur = [0, 0]

    def left():
        return caps[cur[0]] - cur[1] if cur[0] < len(caps) else 0

    def move(dist):
        moved = 0
        while moved < dist and cur[0] < len(caps):
            step = min(left(), dist - moved)
            cur[1] += step
            moved += step
            if left() == 0:
                cur[:] = [cur[0] + 1, 0]
        return moved

    last = ngather = npieces = most = 0
    for off, cnt in recxs:
        move(off - last)
        last = off + cnt * k * C
        for _ in range(cnt * k):
            if left() >= C:
                move(C)
                continue
            ngather, copied, cut = ngather + 1, 0, 0
            while copied < C:
                assert cur[0] < len(caps), "sgl shorter than the recxs"
                cp = min(left(), C - copied)
                if cp == 0:
                    cur[:] = [cur[0] + 1, 0]
                    continue
                cut += 1
                copied += move(cp)
            npieces, most = npieces + cut, max(most, cut)
    return ngather, npieces, most


def cut_at(total, cuts):
    return np.diff([0] + sorted(set(int(c) for c in cuts if 0 < c < total)) + [total]).tolist()


def make_encode(rng, seed, mode, k, p, C, counts):
    """An encode of len(counts) recxs of that many stripes each over an sgl split by `mode`."""
    d = SimpleNamespace(call="recx_encode", seed=seed, mode=mode, k=k, p=p, C=C)
    gaps = [0, 1, 7, 16, 100, C, k * C + 3]
    d.recxs, pos = [], 0
    for cnt in counts:              # a leading gap, gaps between the recxs
        pos += int(rng.choice(gaps))
        d.recxs.append((pos, cnt))
        pos += cnt * k * C
    d.S, total = sum(counts), pos
    if mode == "one":
        caps = [total]
    elif mode == "cell_multiples":  # cuts between cells only: every cell in place
        bounds = [off + j * C for off, cnt in d.recxs for j in range(cnt * k + 1)]
        caps = cut_at(total, rng.choice(bounds, min(len(bounds), int(rng.integers(2, 13))), replace=False))
    elif mode == "tiny":
        caps = rng.integers(1, 41, total + 1)       # more than enough: the first of them that cover the stream
        ends = np.cumsum(caps)
        last = int(np.searchsorted(ends, total))
        caps = caps[:last + 1].tolist()
        caps[-1] -= int(ends[last]) - total
    else:
        caps = cut_at(total, rng.integers(1, max(2, total), int(rng.integers(1, 40))))
    if mode == "zeros":             # empty iovs: the first, the last, some between
        for _ in range(int(rng.integers(1, 4))):
            caps.insert(int(rng.integers(1, len(caps) + 1)), 0)
        caps = [0] + caps + [0]
    if mode == "slack":             # a trailing iov the recxs do not reach
        caps.append(int(rng.integers(1, 5000)))
    d.caps = caps
    d.offs, d.size = lay(rng, caps, int(rng.integers(16)), 64)
    d.desc = bool(rng.integers(2))
    # every parity buffer (S cells) at a skew of its own, in rising or falling address order
    d.poffs, at = [0] * p, GUARD
    for m in (reversed(range(p)) if d.desc else range(p)):
        at += 16 - at % 16 + int(rng.integers(16))
        d.poffs[m] = at
        at += d.S * C + int(rng.integers(1, 65))
    d.psize = at + GUARD
    d.ngather, d.npieces, d.most = walk(caps, d.recxs, k, C)
    return d


def draw_encode(seed):
    """Every (split mode, cell size) pair once over the 48 seeds; a tiny split of large cells is
    to give more than 4096 pieces, so its k*C*S is redrawn into 110 .. 512 KiB."""
    rng = np.random.default_rng(40000 + seed)
    mode, C = SPLITS[seed % len(SPLITS)], CELLS[seed // len(SPLITS) % len(CELLS)]
    k, p = KP[5 * seed % len(KP)]   # every class in turn, whatever the mode (seed % 6); a redraw takes any
    while True:
        counts = [int(rng.integers(1, 7)) for _ in range(int(rng.integers(1, 4)))]
        if mode == "tiny" and not (110 << 10 if C >= 4096 else 0) <= k * C * sum(counts) <= TINY_MAX:
            k, p = KP[int(rng.integers(len(KP)))]
            continue
        d = make_encode(rng, seed, mode, k, p, C, counts)
        if mode != "tiny" or C < 4096 or d.npieces > 4096:
            return d


def test_encode_draw_covers_every_class():
    """Host only: what the 48 seeds of section B reach together."""
    ds = [draw_encode(seed) for seed in range(N)]
    assert {(d.mode, d.C) for d in ds} == {(m, c) for m in SPLITS for c in CELLS}
    for C in (1, 17, 4099):         # C = 1 is gathered only behind an empty iov
        assert any(d.ngather and d.C == C for d in ds), C
    assert {(d.k, d.p) for d in ds} == set(KP)
    for mode in SPLITS:
        assert len({d.p for d in ds if d.mode == mode}) >= 2, mode
    assert any(d.most >= 64 for d in ds)
    assert any(1 <= d.npieces <= 64 for d in ds) and any(65 <= d.npieces <= 4096 for d in ds)
    assert sum(1 for d in ds if d.npieces > 4096) >= 2
    assert {d.p for d in ds} == {1, 2, 3}
    assert sum(1 for d in ds if d.desc and d.p > 1) >= 6 and sum(1 for d in ds if not d.desc and d.p > 1) >= 6
    assert sum(1 for d in ds if d.ngather == 0) >= 8            # every cell in place: no gather launch
    assert any(d.recxs[0][0] and len(d.recxs) > 1 and d.ngather for d in ds)      # gaps together with gathers
    for d in ds:
        assert disjoint(d.offs, d.caps, d.size) and d.k * d.C * d.S <= MAX_BYTES, describe(d)
        assert disjoint(d.poffs, [d.S * d.C] * d.p, d.psize), describe(d)
        if d.mode in ("one", "cell_multiples"):
            assert d.ngather == 0, describe(d)
        if d.mode == "zeros":
            assert d.caps[0] == 0 and d.caps[-1] == 0
        if d.mode == "slack":
            assert sum(d.caps[:-1]) == d.recxs[-1][0] + d.recxs[-1][1] * d.k * d.C
    # cells 2..6 and 6..10 in place, 10..14 behind an empty iov gathered in two pieces, 14..18 in place
    assert walk([10, 0, 3, 5], [(2, 2)], 2, 4) == (1, 2, 2)
    assert walk([2, 8], [(2, 1)], 2, 4) == (0, 0, 0)


class EncodeCase:
    def __init__(self, oracle, d):
        self.d, self.what = d, describe(d)
        k, p, C = d.k, d.p, d.C
        stream = np.random.default_rng(41000 + d.seed).integers(0, 256, sum(d.caps), dtype=np.uint8)
        cuts = np.cumsum([0] + d.caps)
        self.G = sgl_image(d.size, d.offs, [stream[a:b] for a, b in zip(cuts, cuts[1:])])
        self.P = Mem(d.psize)
        self.want, en, n = self.P.copy(), oracle.cauchy1(k, p), 0
        for off, cnt in d.recxs:
            for j in range(cnt):
                par = oracle.encode_data(en[k:], stream[off + j * k * C:off + (j + 1) * k * C].reshape(k, C))
                for m in range(p):
                    self.want.at(d.poffs[m] + n * C, C)[:] = par[m]
                n += 1

    def load(self, dev, ecglib):
        d = self.d
        self.gbuf, self.pbuf = dev.load(self.G), dev.load(self.P)
        assert self.gbuf.ptr % 256 == 0 and self.pbuf.ptr % 256 == 0
        self.iovs, _ = device_sgl(ecglib, self.gbuf, d.offs, d.caps)
        self.rx = (ecglib.EcRecx * len(d.recxs))(*[ecglib.EcRecx(off, cnt, 0) for off, cnt in d.recxs])
        self.pb = (ct.c_void_p * d.p)(*[self.pbuf.ptr + o for o in d.poffs])

    def call(self, ctx, ecglib, stream=None):
        d = self.d
        rc = ecglib.lib().ecg_obj_ec_recx_encode(ctx.h, _oc(d.k, d.p), d.C, self.iovs, len(d.caps), self.rx,
                                                 len(d.recxs), self.pb, stream)
        assert rc == 0, f"{self.what}: {ecglib.lib().ecg_strerror()}"
        self.kernel = ecglib.last_kernel()

    def check(self):
        same(self.pbuf, self.want, self.what, "parity")
        same(self.gbuf, self.G, self.what, "sgl")
        prefix = "ecg_mm_ptr_kernel<" if self.d.ngather else "ecg_mm"
        assert self.kernel.startswith(prefix), f"{self.what}: ran {self.kernel}"


# ------------------------------------------------------------------------ C. array fill-back
IOD_SIZES = [1, 3, 5, 8, 17]
IOVS = [1, 5, 31, 120, 300]


def draw_fill(seed):
    rng = np.random.default_rng(50000 + seed)
    d = SimpleNamespace(call="fill_back", seed=seed, p=2)
    d.iod_size, d.n_iov = IOD_SIZES[seed % 5], IOVS[seed // 5 % 5]
    d.k, d.e_len = int(rng.choice([2, 4, 8, 16])), int(rng.choice([16, 32, 64, 100, 256]))
    d.nstripes, d.n_iod, d.n_recov = int(rng.integers(2, 9)), int(rng.integers(1, 6)), int(rng.integers(1, 9))
    d.args = (60000 + seed, d.k, d.e_len, d.iod_size, d.nstripes, d.n_iod, d.n_iov, d.n_recov, int(rng.integers(4)),
              int(rng.choice([0, 1, 17])))
    d.kw = dict(on_boundary=seed % 2 == 0, short=float(rng.uniform(0.05, 0.95)) if seed % 4 == 3 else None,
                zero_front=int(rng.integers(3)), zero_back=int(rng.integers(3)))
    d.lost = sorted(int(c) for c in rng.choice(d.k + d.p, int(rng.integers(1, 3)), replace=False))
    d.case = make_case(*d.args, **d.kw)
    # The walk takes the first stripe of the list that overlaps a record and refuses one that begins
    # behind the record's start (the reference asserts), so the list has to rise in address, as it
    # does for recxs that come in rising order; a draw whose list does not gets its recxs sorted.
    starts = [s["idx"] for s in sgl_py.stripe_list_init(d.case["srn"], d.case["recov"])]
    d.sorted = starts != sorted(starts)
    if d.sorted:
        d.case["recov"].sort(key=lambda r: r["idx"])
    d.caps = d.case["lens"]
    d.offs, d.size = lay(rng, d.caps, int(rng.integers(16)), 40)
    d.full = sum(n for _, n in d.case["iod"]) * d.iod_size
    d.is_short = sum(d.caps) < d.full
    ends = set(np.cumsum(d.caps).tolist())
    d.on_end = sum(1 for off in user_offsets(d.case) if 0 < off and off in ends)
    return d


def test_fill_draw_covers_every_class():
    """Host only: what the 48 seeds of section C reach together."""
    ds = [draw_fill(seed) for seed in range(N)]
    assert {d.iod_size for d in ds} == {1, 3, 5, 8, 17}
    assert sum(1 for d in ds if len(d.caps) >= 200) >= 4 and min(len(d.caps) for d in ds) <= 3
    assert sum(1 for d in ds if d.is_short) >= 8
    assert any(d.is_short and max(user_offsets(d.case)) >= sum(d.caps) for d in ds)    # a copy wholly beyond the sgl
    assert sum(1 for d in ds if d.caps[0] == 0 and d.caps[-1] == 0) >= 6
    assert sum(1 for d in ds if d.on_end) >= 12                 # sgl_skip's pre[lo + 1] == off
    assert any(d.on_end and d.is_short for d in ds)
    assert sum(1 for d in ds if not d.sorted and d.n_recov >= 3) >= 12     # recxs in the order they were drawn
    for d in ds:
        assert disjoint(d.offs, d.caps, d.size) and sum(d.caps) > 0, describe(d)


class FillCase:
    def __init__(self, oracle, d):
        self.d, self.what = d, describe(d)
        case, k, p = d.case, d.k, d.p
        self.C = C = d.e_len * d.iod_size
        self.stripes = sgl_py.stripe_list_init(case["srn"], case["recov"])
        en = oracle.cauchy1(k, p)
        img = stripe_image(case, self.stripes, p, parity_fn=lambda x: oracle.encode_data(en[k:], x))
        self.nst = img.size // ((k + p) * C)
        broken = img.reshape(self.nst, k + p, C).copy()
        broken[:, d.lost] = ERASED
        self.I, self.whole = Mem(GUARD + img.size + GUARD), Mem(GUARD + img.size + GUARD)
        self.I.at(GUARD, img.size)[:] = broken.reshape(-1)
        self.whole.at(GUARD, img.size)[:] = img
        self.D = Mem(d.size)
        self.ref = sgl_py.Sgl([np.full(c, FILL, np.uint8) for c in d.caps])
        sgl_py.recov_fill_back(d.iod_size, case["iod"], self.ref, case["recov"], self.stripes, img, (k + p) * C,
                               case["srn"])
        got = np.concatenate(self.ref.bufs)
        full = expected_user_bytes(case, fill=FILL, size=max(got.size, d.full))     # short: the front of it
        assert np.array_equal(got, full[:got.size]), f"{self.what}: sgl_py against the records' user offsets"
        self.want = sgl_image(d.size, d.offs, self.ref.bufs)

    def load(self, dev, ecglib):
        d, case = self.d, self.d.case
        self.ibuf, self.dbuf = dev.load(self.I), dev.load(self.D)
        self.iovs, self.sgl = device_sgl(ecglib, self.dbuf, d.offs, d.caps)
        isz = d.iod_size
        self.iod = (ecglib.Recx * len(case["iod"]))(*[ecglib.Recx(a, n) for a, n in case["iod"]])
        self.rec = (ecglib.RecxEp * len(case["recov"]))(
            *[ecglib.RecxEp(ecglib.Recx(r["idx"], r["nr"]), r["ep"], isz, r["type"]) for r in case["recov"]])
        self.st = (ecglib.RecxEp * len(self.stripes))(
            *[ecglib.RecxEp(ecglib.Recx(s["idx"], s["nr"]), s["ep"], isz, s["type"]) for s in self.stripes])

    def call(self, ctx, ecglib, stream=None):
        d, case, n = self.d, self.d.case, self.d.k + self.d.p
        ctx.recover(d.k, d.p, self.C, self.nst, self.ibuf.ptr + GUARD, n * self.C, d.lost, stream)
        rc = ecglib.lib().ecg_obj_ec_recov_fill_back(ctx.h, d.iod_size, 0, self.iod, len(case["iod"]),
                                                     ct.byref(self.sgl), self.rec, len(case["recov"]), self.st,
                                                     len(self.stripes), self.ibuf.ptr + GUARD, n * self.C, case["srn"],
                                                     stream)
        assert rc == 0, f"{self.what}: {ecglib.lib().ecg_strerror()}"

    def check(self):
        same(self.dbuf, self.want, self.what, "iovs")
        same(self.ibuf, self.whole, self.what, "stripes")
        lens = [self.iovs[i].iov_len for i in range(len(self.d.caps))]
        assert lens == self.ref.iov_len, self.what
        assert self.sgl.sg_nr_out == self.ref.nr_out, self.what
        assert all(ln <= cap for ln, cap in zip(lens, self.d.caps)), self.what


# ------------------------------------------------------------------------------- the runs
def run_case(ctx, ecglib, case):
    """One case: loaded, called, synced once, compared whole; its buffers freed whatever happens.
    An error the library reports names the seed and the draw like a failed assert."""
    with Device(ctx, ecglib) as dev:
        try:
            case.load(dev, ecglib)
            case.call(ctx, ecglib)
            ctx.sync()
        except ecglib.EcgError as e:
            raise AssertionError(f"{case.what}: {e}") from e
        case.check()


@pytest.mark.gpu
def test_copy_segs(ctx, ecglib):
    for seed in range(N):
        run_case(ctx, ecglib, CopyCase(draw_copy(seed)))


@pytest.mark.gpu
def test_recx_encode(ctx, oracle, ecglib):
    kernels = {}
    for seed in range(N):
        case = EncodeCase(oracle, draw_encode(seed))
        run_case(ctx, ecglib, case)
        kernels[case.kernel] = kernels.get(case.kernel, 0) + 1
    print("recx_encode kernels:", kernels)


@pytest.mark.gpu
def test_fill_back(ctx, oracle, ecglib):
    for seed in range(N):
        run_case(ctx, ecglib, FillCase(oracle, draw_fill(seed)))


# ----------------------------------------------------------- D. the two scratch slots handed on
class MatmulCase:
    """ecg_matmul_ptrs over cells in shuffled slots of one allocation: no affine table."""

    def __init__(self, oracle, seed, k=4, rows=2, C=4096, S=5):
        self.what = f"matmul_ptrs seed {seed}: k={k} rows={rows} C={C} S={S}"
        self.k, self.rows, self.C, self.S = k, rows, C, S
        rng = np.random.default_rng(seed)
        n, slot = k + rows, C + 48
        self.offs = [GUARD + int(i) * slot for i in rng.permutation(S * n)]
        self.coef = oracle.cauchy1(k, rows)[k:]
        self.M = Mem(GUARD + S * n * slot + GUARD)
        cells = rng.integers(0, 256, (S, k, C), dtype=np.uint8)
        for s in range(S):
            for j in range(k):
                self.M.at(self.offs[s * n + j], C)[:] = cells[s, j]
        self.want = self.M.copy()
        for s in range(S):
            for r, cell in enumerate(oracle.encode_data(self.coef, cells[s])):
                self.want.at(self.offs[s * n + k + r], C)[:] = cell

    def load(self, dev, ecglib):
        self.buf = dev.load(self.M)

    def call(self, ctx, ecglib, stream=None):
        ctx.matmul_ptrs(self.k, self.rows, self.coef, self.C, self.S, [self.buf.ptr + o for o in self.offs], stream)
        self.kernel = ecglib.last_kernel()

    def check(self):
        same(self.buf, self.want, self.what, "cells")
        assert self.kernel.startswith("ecg_mm_ptr_kernel<"), f"{self.what}: ran {self.kernel}"


def handover_cases(oracle):
    """A gathering encode, a fill-back of 65 segments, an encode whose gathered cells (24 of
    4096 bytes, in some 4800 pieces) and tables need more than the 64 KiB a slot starts with, a
    pointer table, a third gathering encode."""
    rng = np.random.default_rng(70000)
    first = EncodeCase(oracle, make_encode(rng, 70001, "random", 4, 2, 4096, [3, 2]))
    big = EncodeCase(oracle, make_encode(rng, 70002, "tiny", 4, 2, 4096, [4, 2]))
    third = EncodeCase(oracle, make_encode(rng, 70003, "zeros", 8, 3, 1000, [2, 1, 2]))
    assert first.d.ngather and third.d.ngather and big.d.ngather * big.d.C > 64 << 10 and big.d.npieces > 4096
    copy = CopyCase(draw_copy(4))
    assert copy.d.n == 65
    return [first, copy, big, MatmulCase(oracle, 70004), third]


def test_handover_cases_are_what_they_say(oracle):
    """Host only (the CPU codec builds the expectations): handover_cases' own asserts."""
    handover_cases(oracle)


def hand_over(ecglib, oracle, own_stream):
    cases = handover_cases(oracle)
    c2 = ecglib.Context(0)
    stream = None
    try:
        with Device(c2, ecglib) as dev:
            for c in cases:
                c.load(dev, ecglib)
            # what a context builds, synchronously, on first use: not inside the sequence (the encode
            # writes the same parity again below)
            cases[0].call(c2, ecglib)
            c2.sync()
            if own_stream:
                stream = c2.stream()
            cases[0].call(c2, ecglib, stream)
            for c in cases[1:]:                                 # no sync in between
                c.call(c2, ecglib)
            if own_stream:
                c2.sync(stream)
            c2.sync()
            for c in cases:
                c.check()
    finally:
        if stream is not None:
            c2.destroy_stream(stream)
        c2.close()


@pytest.mark.gpu
def test_gathered_cells_and_segment_tables_hand_the_two_slots_to_each_other(ecglib, oracle):
    """On the default stream of a fresh context with no sync in between: recx_encode with gathers,
    fill-back, a recx_encode that outgrows its slot (re-allocated while the other slot still has a
    reader), matmul_ptrs, recx_encode.  The encode's product reads its gathered cells from the
    slot after the call has returned; the call after next takes that slot.  Each call has its own
    buffers; everything is compared whole after the one sync."""
    hand_over(ecglib, oracle, own_stream=False)


@pytest.mark.gpu
def test_slot_hand_over_across_streams(ecglib, oracle):
    """The same sequence with the first call on a stream of its own and the rest on the context's
    default stream: the third call takes the first one's slot and has stream order no longer on
    its side, only the slot's `done` event.  This exercises that path; it cannot prove a race
    absent: a missing wait shows only if the first call's product is still running when the third
    call rewrites the slot, which nothing here forces."""
    hand_over(ecglib, oracle, own_stream=True)
