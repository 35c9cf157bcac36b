"""Seeded random geometry, strides and alignment through the checksum calls: ecg_csum_extents,
ecg_encode_csum, ecg_encode_csum_all, ecg_recover_csum, ecg_recover_csum_all and
ecg_csum_compare, byte for byte against the CPU oracle.

The calls' own modules (test_gpu_csum.py, test_gpu_csum_all.py) are hand-written lists on the
tight layouts; here the chunk geometry, every stride parameter, the base skews, the place of the
checksum arrays and the launch settings are drawn.  The layout rig is test_gpu_fuzz_masks.py's:
every allocation is 0xA5 where nothing belongs (256 guard bytes in front, slack behind, every
gap a padded stride opens) and is compared whole after the call; a checksum array lies exactly
between its guards, so one checksum too many is a failure.  The kernel that ran must be the one a
restated rule names (`extents_class` for ecg_csum_extents, `fused_causes` for the fused product
+ checksum kernels), csum_chunks must advance by the chunks the call computed, and every launch
setting is back at 0 after the case.

A draw is pure and host-only.  Where a seed's draw has to meet a class (its `goal`: a kernel
shape, a fallback cause standing alone, the SRC kernel) or a documented precondition (C %
rec_size, cells that do not overlap), it is redrawn from the same generator until it does, so
no seed is skipped and the classes test_draws_cover_every_class asks for are there by
construction, not by luck.  The first pass through the 13 shapes x 3 CRC types of the fused
calls (seeds below 39) asks for the fused kernel; the later seeds draw freely, or ask for one
fallback cause alone.

test_offsets_past_4GiB puts extents and stripes 2^32 - 2048 bytes apart in an allocation of
several GiB of which only windows are ever uploaded and compared."""
import contextlib
import math
from types import SimpleNamespace

import numpy as np
import pytest

from tests.test_gpu_csum_all import FUSED_DEFAULT
from tests.test_gpu_fuzz_masks import (ERASED, FAR_STRIDE, GUARD, Arr, Device, Mem, far_place, launch, pad_of, place,
                                        same)

TYPES = (1, 2, 3, 7)
CRCS = (1, 2, 3)
CL = {1: 2, 2: 4, 3: 8, 7: 4}
TNAME = {1: "crc16", 2: "crc32", 3: "crc64"}
PRE = 0xEE                  # what a checksum array holds before the call
CSLACK = 4096               # bytes behind a checksum array, in front of its rear guard
MAX_BYTES = 8 << 20         # the cells of one case
MAX_EXT = 256 << 10         # one extent of ecg_csum_extents
U64MAX = (1 << 64) - 1
CALLS = ["csum_extents", "encode_csum", "encode_csum_all", "recover_csum", "recover_csum_all", "csum_compare"]
NSEEDS = {"csum_extents": 64, "encode_csum": 72, "encode_csum_all": 72, "recover_csum": 72, "recover_csum_all": 72,
          "csum_compare": 48}
SEED0 = {c: 20000 * (i + 1) for i, c in enumerate(CALLS)}
NKH_CACHE = 8               # ECG_NKH_CACHE: multiplier tables a context keeps

# ecg_csum_extents
CHUNKS = [24, 64, 100, 1040, 4096, 8192, 8208, 12288, 15376, 16384, 20480 + 48, 40960]
RECS = [1, 2, 6, 8, 16, "larger"]
IDX_KINDS = ["zero", "one", "in_first", "in_later"]
NEXT_KINDS = [1, 2, 5, "many"]
EXT_MODES = ["tight", "pad16", "padodd", "zero"]
EXT_GOALS = ["any", "split", "group", "wave", "bytes", "stride_alone", "split3", "many", "tiny", "last1",
             "rec_nodiv", "any", "any", "any", "any", "any"]
BLOCKS = [0, 1, 3]

# the fused product + checksum calls
KS, ROWS = (2, 4, 8, 16), (1, 2, 3)
SHAPES12 = [(k, r) for k in KS for r in ROWS]
CELLS = [4096, 4096 + 16, 8192 + 48, 12288, 5 * 4096 + 1024 + 16, 4100]
FCHUNKS = [4096, 8192, 12288, 20480, 6000]
FRECS = [1, 8, 4096]
STRIPES = [1, 2, 5, 9]
COLS = [0, 1, 2, 3, 5]
GRIDS = [(0, 0), (1, 0), (3, 2), (0, 1), (64, 0), (0, 64)]     # the last two: above the item / stripe counts
ENC_MODES = ["tight", "padded", "gapped", "interleaved"]
REC_MODES = ["tight", "pad16", "padodd"]
FIRST_PASS = 39             # seeds below: every shape x CRC type once, asked to run fused
FREE_GOALS = ["free", "skew", "free", "csmis", "chunk", "stride"]

# ecg_csum_compare
CAP = 1024 * 256            # threads of the largest grid
CMP_N = [0, 1, 255, 256, 257, CAP - 1, CAP, CAP + 300]
CMP_COUNTS = [0, 1, 2, 40, "all"]


# ------------------------------------------------------------------ the rules, restated
def rcs_of(cs, rb):
    """ecg_csum_record_chunksize"""
    return rb if rb > cs else cs // rb * rb


def steps_of(n):
    """1 KiB steps of a wave over n bytes"""
    return (n // 16 + 63) // 64


def split_steps(n):
    """ECG_CSUM_STEPS: the step count the split kernel tabulates a chunk length by"""
    return (steps_of(n) + 3) // 4 * 4


def extents_geom(cs, rb, idx, nr):
    """-> (record chunk bytes, chunks, bytes of the first chunk, bytes of the last)"""
    rcs = rcs_of(cs, rb)
    per = rcs // rb
    nch = (idx + nr - 1) // per - idx // per + 1
    first = min(per - idx % per, nr) * rb
    last = nr * rb - first - (nch - 2) * rcs if nch >= 2 else first
    return rcs, nch, first, last


def extents_class(htype, rcs, first, base, stride, n_ext, nch):
    """ecg_csum.c ecg_csum_extents and ecg_csum_kernels.hip ecg_k_launch_csum: the byte kernel
    unless base, stride, first-chunk bytes and chunk bytes are all multiples of 16; a workgroup
    per chunk for fewer than 4096 chunks of >= 16 steps; a 16-lane group per chunk of <= 8
    steps (CRC only); else a wave per chunk."""
    if any(v % 16 for v in (base, stride, first, rcs)):
        return "bytes"
    if n_ext * nch < 4096 and steps_of(rcs) >= 16:
        return "split"
    return "group" if steps_of(rcs) <= 8 and htype != 7 else "wave"


def extents_kernel(htype, cls):
    if htype == 7:
        return {"bytes": "ecg_adler_kernel<bytes>", "split": "ecg_adler_split_kernel", "wave": "ecg_adler_kernel"}[cls]
    t = TNAME[htype]
    return {"bytes": f"ecg_crc_kernel<{t},bytes>", "split": f"ecg_crc_split_kernel<{t}>",
            "group": f"ecg_crc_group_kernel<{t}>", "wave": f"ecg_crc_kernel<{t}>"}[cls]


def class_of(name):
    """The class of a kernel name that ran."""
    if name.startswith("ecg_mm_csum_kernel"):
        return "src" if name.endswith(",src>") else "fused"
    for c in ("bytes", "split", "group"):
        if c in name:
            return c
    return "wave"


def fused_name(htype, k, rows, src):
    shape = f"{k},{rows}" if k in KS and rows in ROWS else "0,0"
    return f"ecg_mm_csum_kernel<{shape},{TNAME[htype]}{',src' if src else ''}>"


def fused_ncols(override, m, htype, k, rows, src):
    """ecg_csum.c fused_cols (ECG_FUSED_COLS unset): 4 KiB columns per work item"""
    if override:
        return min(override, m)
    dflt = 8 if src else 2 if htype == 2 and k == 8 and rows == 2 else 4 if rows == 1 or k >= 8 else 8
    return min(m, dflt)


def fused_causes(d, csum_off):
    """Why the fused kernel does not take the case (ecg_core.c matmul_csum, ecg_csum.c
    ecg_csum_fused_params, ecg_fused_kernels.hip ecg_k_launch_matmul_csum); [] = it does."""
    why = []
    if d.htype == 7:
        why.append("adler")
    if d.k > 16 or d.rows > 8:
        why.append("shape")
    if d.rcs % 4096:
        why.append("chunk")
    if d.C % 16:
        why.append("cell")
    if csum_off % (8 if d.htype == 3 else 4):
        why.append("csmis")
    if any(v % 16 for v in d.ptrs + d.strides + d.offs):
        why.append("align")
    return why


def recov_order(k, p, errs):
    """ecg_gf.c ecg_recov_rows: (the cells the product reads: the first k survivors; the cells
    its rows write: data cells first, each group in err_list order)."""
    dec = [c for c in range(k + p) if c not in errs][:k]
    if len(errs) == p and all(e >= k for e in errs):
        return dec, list(range(k, k + p))
    return dec, [e for e in errs if e < k] + [e for e in errs if e >= k]


def finish_fused(d):
    """The prediction for a fused call's draw: d.src / d.fused (which kernel is the last), d.kernel,
    d.chunks, d.khkey (the multiplier table the case needs, None without a fused launch)."""
    all_ = d.call.endswith("_all")
    d.rcs, d.nch, first, _ = extents_geom(d.cs, d.rb, 0, d.C // d.rb)
    d.why = fused_causes(d, d.coff[0])
    src_ok = all_ and not d.why and d.coff[1] % (8 if d.htype == 3 else 4) == 0
    d.src = src_ok and (d.route == 1 or (d.route == 0 and (d.htype, d.k, d.rows) in FUSED_DEFAULT))
    d.fused = not d.why and not all_
    if d.src or d.fused:
        d.kernel = fused_name(d.htype, d.k, d.rows, d.src)
    else:       # the last launch: ecg_csum_extents over the last source cell (_all) or the last output row
        base, stride = d.last_src if all_ else d.last_out
        d.kernel = extents_kernel(d.htype, extents_class(d.htype, d.rcs, first, base, stride, d.S, d.nch))
    d.chunks = (d.rows + (d.k if all_ else 0)) * d.S * d.nch
    d.khkey = None
    if not d.why:
        last = d.C - (d.nch - 1) * d.rcs
        d.khkey = (d.htype, d.rcs, last, fused_ncols(d.cols, d.rcs // 4096, d.htype, d.k, d.rows, d.src))
    return d


def describe(d):
    skip = ("win", "dwin", "ptrs", "offs")
    return f"{d.call} seed {d.seed}: " + " ".join(f"{k}={v}" for k, v in vars(d).items() if k not in skip)


# --------------------------------------------------------------------------- the draws
def extents_once(rng, htype):
    d = SimpleNamespace(htype=htype, gx=0, gy=0, variant=0, cols=0, route=0)
    d.cs = int(rng.choice(CHUNKS))
    d.rec = RECS[int(rng.integers(len(RECS)))]
    d.rb = d.cs + int(rng.choice([16, 8, 1])) if d.rec == "larger" else d.rec
    rcs = rcs_of(d.cs, d.rb)
    per = rcs // d.rb
    al = 16 // math.gcd(16, d.rb)       # records from one 16-byte boundary to the next
    d.idx_kind = IDX_KINDS[int(rng.integers(len(IDX_KINDS)))]
    r = int(rng.integers(1, per)) if per > 1 else 0
    if rng.integers(2):                 # a first chunk that ends and starts on 16 bytes
        r -= r % al
    d.idx = {"zero": 0, "one": 1, "in_first": r, "in_later": per * int(rng.integers(1, 4)) + r}[d.idx_kind]
    first_rec = per - d.idx % per
    nch = int(rng.integers(1, max(1, min(7, MAX_EXT // rcs)) + 1))
    d.last_rec = None
    if nch == 1:                # to the end of the chunk, or short of it; or shorter than 16 bytes
        tiny = d.rb < 16 and rng.integers(3) == 0
        d.nr = int(rng.integers(1, min(first_rec, 15 // d.rb if tiny else first_rec) + 1))
        if not tiny and rng.integers(3) == 0:
            d.nr = first_rec
    else:
        d.last_rec = [1, per, int(rng.integers(1, per + 1))][int(rng.integers(3))]
        d.nr = first_rec + (nch - 2) * per + d.last_rec
    d.rcs, d.nch, d.first, d.last = extents_geom(d.cs, d.rb, d.idx, d.nr)
    d.ext = d.nr * d.rb
    assert d.nch == nch and d.ext <= MAX_EXT
    d.next_kind = NEXT_KINDS[int(rng.integers(len(NEXT_KINDS)))]
    if d.next_kind == "many":           # the smallest count with >= 4096 chunks; the extents overlap
        d.n_ext, d.mode = -(-4096 // nch), "many"
        d.stride = int(rng.choice([0, 16]))
    else:
        d.n_ext, d.mode = d.next_kind, EXT_MODES[int(rng.integers(len(EXT_MODES)))]
        if d.mode in ("pad16", "padodd"):       # off 16: the stride alone picks the byte kernel
            d.stride = (d.ext + 15) // 16 * 16 + pad_of(rng, d.mode)
        else:
            d.stride = d.ext if d.mode == "tight" else 0
    d.skew = int(rng.integers(1, 16)) if rng.integers(4) == 0 else 0
    d.blocks = int(rng.choice(BLOCKS))
    d.coff = GUARD + CL[htype] * int(rng.choice([0, 1, 3]))     # a multiple of the checksum length, no more
    d.data_seed = int(rng.integers(1 << 31))
    d.base = GUARD + d.skew
    d.span = (d.n_ext - 1) * d.stride + d.ext
    d.size = d.base + d.span + CSLACK + GUARD
    d.cls = extents_class(htype, d.rcs, d.first, d.base, d.stride, d.n_ext, d.nch)
    d.kernel = extents_kernel(htype, d.cls)
    d.chunks = d.n_ext * d.nch
    d.win = None
    return d


def stride_alone(d):
    """The byte kernel chosen by the stride alone."""
    return d.n_ext > 1 and d.stride % 16 != 0 and not any(v % 16 for v in (d.base, d.first, d.rcs))


def three_lengths(d):
    """The split kernel with first, whole and last chunk of three different tabulated lengths."""
    return (d.cls == "split" and d.nch >= 3
            and len({split_steps(d.first), split_steps(d.rcs), split_steps(d.last)}) == 3)


EXT_MET = {
    "any": lambda d: True,
    "split": lambda d: d.cls == "split",
    "group": lambda d: steps_of(d.rcs) <= 8 and d.cls == ("group" if d.htype != 7 else "wave"),
    "wave": lambda d: d.cls == "wave" and steps_of(d.rcs) > 8 and d.chunks < 4096,
    "bytes": lambda d: d.cls == "bytes",
    "stride_alone": stride_alone,
    "split3": three_lengths,
    "many": lambda d: d.chunks >= 4096 and steps_of(d.rcs) >= 16 and d.cls == "wave",
    "tiny": lambda d: d.ext < 16,
    "last1": lambda d: d.nch >= 2 and d.last_rec == 1 and d.rcs > d.rb and d.first < d.rcs,
    "rec_nodiv": lambda d: d.rb <= d.cs and d.cs % d.rb != 0 and d.idx != 0,
}


def draw_csum_extents(seed):
    """ecg_csum_extents: n_ext extents of rx_nr records from record index rx_idx, ext_stride apart."""
    rng = np.random.default_rng(SEED0["csum_extents"] + seed)
    goal = EXT_GOALS[seed // 4 % len(EXT_GOALS)]
    while True:
        d = extents_once(rng, TYPES[seed % 4])
        if EXT_MET[goal](d) and d.size <= MAX_BYTES:
            break
    d.goal = goal
    return d


def fused_goal(call, seed):
    if seed % 6 == 5:
        return "adler_alone" if seed % 12 == 5 else "adler"
    if seed < FIRST_PASS:
        if call.endswith("_all"):
            return "src_default" if seed == 20 else "src"       # seed 20: crc32 8+2, the default route's
        return "fused"
    if call.endswith("_all") and seed in (44, 50, 56):          # 50: crc16 16+3, two passes by default; 56: crc32 4+2, fused
        return {44: "srcmis", 50: "two_pass_default", 56: "two_pass_forced"}[seed]
    return FREE_GOALS[(seed - FIRST_PASS) % len(FREE_GOALS)]


def skew_alone(d):
    """A base off 16 bytes is all that keeps the fused kernel away."""
    return d.why == ["align"] and any(d.skews) and not any(v % 16 for v in d.strides + d.offs)


def fused_stride_alone(d):
    """A stride off 16 bytes is all that keeps the fused kernel away."""
    return d.why == ["align"] and not any(d.skews)


def src_array_alone(d):
    """Only the sources' checksum array is off its alignment: two passes, the first of them fused."""
    return not d.why and d.coff[1] % (8 if d.htype == 3 else 4) != 0


FUSED_MET = {
    "free": lambda d: True,
    "adler": lambda d: True,
    "adler_alone": lambda d: d.why == ["adler"],
    "fused": lambda d: d.fused,
    "src": lambda d: d.src,
    "src_default": lambda d: d.src and d.route == 0,
    "two_pass_forced": lambda d: not d.why and d.route == 2 and d.coff[1] % 8 == 0,
    "two_pass_default": lambda d: not d.why and d.route == 0 and not d.src and d.coff[1] % 8 == 0,
    "skew": lambda d: skew_alone(d),
    "srcmis": lambda d: src_array_alone(d) and d.route == 1,
    "csmis": lambda d: d.why == ["csmis"] or d.htype == 2,      # crc32 arrays are never drawn off 4 bytes
    "chunk": lambda d: d.why == ["chunk"],
    "stride": lambda d: fused_stride_alone(d) or d.mode in ("tight", "pad16"),     # modes with no stride off 16
}


def encode_strides(rng, mode, k, p, C, S):
    """-> (data stripe stride, parity cell stride, parity stripe stride, parity in the data's buffer at + k*C)"""
    if mode == "tight":
        return k * C, S * C, C, False
    if mode == "padded":
        return k * C + pad_of(rng, "pad16" if rng.integers(3) else "padodd"), S * C, C, False
    if mode == "gapped":        # gaps between the cells of a parity row and between the rows
        unit = "pad16" if rng.integers(4) else "padodd"
        pss = C + pad_of(rng, unit)
        return k * C + (pad_of(rng, "pad16") if rng.integers(2) else 0), S * pss + pad_of(rng, unit), pss, False
    assert mode == "interleaved"
    st = (k + p) * C + pad_of(rng, ["tight", "pad16", "pad16", "padodd"][int(rng.integers(4))])
    return st, C, st, True


def fused_once(rng, call, seed):
    enc, all_ = call.startswith("encode"), call.endswith("_all")
    d = SimpleNamespace(call=call, seed=seed, variant=0, blocks=0)
    d.k, d.rows = SHAPES12[seed % 13] if seed % 13 < 12 else [(5, 2), (8, 4)][seed // 13 % 2]
    d.htype = 7 if seed % 6 == 5 else CRCS[seed // 13 % 3]
    d.C = int(rng.choice(CELLS))
    d.cs = int(rng.choice(FCHUNKS))
    while True:                 # a cell is whole records
        d.rb = int(rng.choice(FRECS))
        if d.C % d.rb == 0:
            break
    d.S = int(rng.choice(STRIPES))
    d.cols = int(rng.choice(COLS))
    d.route = int(rng.integers(3)) if all_ else 0
    d.gx, d.gy = GRIDS[int(rng.integers(len(GRIDS)))]
    mis = (2 if d.htype == 1 else 4) if d.htype in (1, 3) and rng.integers(8) == 0 else 0
    which = int(rng.integers(3)) if all_ else 0         # the outputs' array, the sources', both
    d.coff = [GUARD + (mis if which in (0, 2) else 0), GUARD + (mis if which in (1, 2) else 0)]
    d.skews = [0, 0]
    if rng.integers(4) == 0:
        d.skews[int(rng.integers(2))] = int(rng.integers(1, 16))
    k, C, S = d.k, d.C, d.S
    if enc:
        d.p = p = d.rows
        d.mode = ENC_MODES[seed % len(ENC_MODES)]
        d.dss, d.pcs, d.pss, d.same_buf = encode_strides(rng, d.mode, k, p, C, S)
        data, par = Arr(S, k, C, d.dss, C), Arr(S, p, C, d.pss, d.pcs)
        if d.same_buf:
            d.dsize, (d.dbase, d.pbase) = place([(data, 0), (par, k * C)], d.skews[0])
            d.psize = 0
        else:
            d.dsize, (d.dbase,) = place([(data, 0)], d.skews[0])
            d.psize, (d.pbase,) = place([(par, 0)], d.skews[1])
        d.ptrs, d.strides = [d.dbase, d.pbase], [d.dss, d.pss]
        d.offs = [j * C for j in range(k)] + [r * d.pcs for r in range(p)]
        d.last_src, d.last_out = (d.dbase + (k - 1) * C, d.dss), (d.pbase + (p - 1) * d.pcs, d.pss)
    else:
        d.p = p = d.rows if d.rows == 4 else d.rows + int(rng.integers(0, 4 - d.rows))
        d.mode = REC_MODES[int(rng.integers(len(REC_MODES)))]
        d.errs = [int(e) for e in rng.choice(k + p, d.rows, replace=False)]
        d.stride = (k + p) * C + pad_of(rng, d.mode)
        d.dsize, (d.dbase,) = place([(Arr(S, k + p, C, d.stride, C), 0)], d.skews[0])
        dec, out = recov_order(k, p, d.errs)
        d.ptrs, d.strides, d.offs = [d.dbase], [d.stride], [c * C for c in dec + out]
        d.last_src, d.last_out = (d.dbase + dec[-1] * C, d.stride), (d.dbase + out[-1] * C, d.stride)
    d.dwin = None
    d.data_seed = int(rng.integers(1 << 31))
    return finish_fused(d)


def draw_fused(call, seed):
    rng = np.random.default_rng(SEED0[call] + seed)
    goal = fused_goal(call, seed)
    while True:
        d = fused_once(rng, call, seed)
        if FUSED_MET[goal](d) and d.S * (d.k + d.p) * d.C <= MAX_BYTES:
            break
    d.goal = goal
    return d


def draw_encode_csum(seed):
    return draw_fused("encode_csum", seed)


def draw_encode_csum_all(seed):
    return draw_fused("encode_csum_all", seed)


def draw_recover_csum(seed):
    return draw_fused("recover_csum", seed)


def draw_recover_csum_all(seed):
    return draw_fused("recover_csum_all", seed)


def draw_csum_compare(seed):
    """ecg_csum_compare: n checksums, some of them with one bit flipped."""
    rng = np.random.default_rng(SEED0["csum_compare"] + seed)
    d = SimpleNamespace(htype=TYPES[seed % 4], n=CMP_N[seed // 4 % len(CMP_N)])
    d.count = CMP_COUNTS[(seed // 4 * 3 + seed % 4) % len(CMP_COUNTS)]
    d.skews = [int(rng.integers(16)), int(rng.integers(16))]       # of got, of want
    d.pick = int(rng.integers(2))
    d.data_seed = int(rng.integers(1 << 31))
    return d


def compare_positions(d):
    """The indices that differ (sorted): all of them, or index >= CAP first where n allows, then 0
    or n - 1 (d.pick; both from three on), then drawn ones."""
    n = d.n
    if d.count == "all":
        return np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(d.data_seed + 1)
    must = ([int(rng.integers(CAP, n))] if n > CAP else []) + [[0, n - 1][d.pick], [n - 1, 0][d.pick]]
    pos = []
    for i in must + [int(v) for v in rng.choice(n, min(n, 64), replace=False)]:
        if len(pos) < min(d.count, n) and 0 <= i < n and i not in pos:
            pos.append(i)
    return np.array(sorted(pos), dtype=np.int64)


DRAW = {"csum_extents": draw_csum_extents, "encode_csum": draw_encode_csum, "encode_csum_all": draw_encode_csum_all,
        "recover_csum": draw_recover_csum, "recover_csum_all": draw_recover_csum_all,
        "csum_compare": draw_csum_compare}


def draw(call, seed):
    d = DRAW[call](seed)
    d.call, d.seed = call, seed
    return d


# --------------------------------------------------- what a run of all seeds has to reach
def extents_reached(ds, names):
    """Every kernel class each hash type has."""
    for t in TYPES:
        got = {class_of(n) for d, n in zip(ds, names) if d.htype == t}
        assert got == ({"split", "group", "wave", "bytes"} if t != 7 else {"split", "wave", "bytes"}), (t, got)


def fused_reached(call, ds, names):
    """Every specialised shape and the generic one in fused form, both table kinds of crc32 (8+2:
    byte tables, else 5-bit) and crc64, a fallback; for _all the SRC kernel on every shape."""
    ran = [n for n in names if n.startswith("ecg_mm_csum_kernel") and n.endswith(",src>") == call.endswith("_all")]
    shapes = {",".join(n.split("<")[1].split(",")[:2]) for n in ran}
    assert shapes == {f"{k},{r}" for k, r in SHAPES12} | {"0,0"}, (call, sorted(shapes))
    assert any("<8,2,crc32" in n for n in ran) and any("crc32" in n and "<8,2," not in n for n in ran), call
    assert any("crc64" in n for n in ran) and any("crc16" in n for n in ran), call
    assert any(not n.startswith("ecg_mm_csum_kernel") for n in names), call


def compare_reached(ds):
    assert any(d.n > CAP and compare_positions(d).size and compare_positions(d).max() >= CAP for d in ds)


# ---------------------------------------------------------------- 3. the draw is worth running
def test_draws_cover_every_class():
    """Host only: every seed yields a case that fits, and over its seeds each call meets every
    class the GPU tests are there for.  Conditions on the draws, not measurements."""
    ds = [draw("csum_extents", s) for s in range(NSEEDS["csum_extents"])]
    assert all(d.size <= MAX_BYTES and d.ext <= MAX_EXT and 1 <= d.nch <= 7 for d in ds)
    extents_reached(ds, [d.kernel for d in ds])
    for t in TYPES:
        mine = [d for d in ds if d.htype == t]
        assert any(stride_alone(d) and d.cls == "bytes" for d in mine), t
        assert any(three_lengths(d) for d in mine), t
        assert any(d.chunks >= 4096 for d in mine) and any(d.ext < 16 for d in mine), t
    assert {d.cs for d in ds} == set(CHUNKS) and {d.rec for d in ds} == set(RECS)
    assert {d.idx_kind for d in ds} == set(IDX_KINDS) and {d.next_kind for d in ds} == set(NEXT_KINDS)
    assert {d.mode for d in ds} == set(EXT_MODES) | {"many"} and {d.blocks for d in ds} == set(BLOCKS)
    assert {d.nch for d in ds} == set(range(1, 8))
    assert sum(1 for d in ds if d.skew) >= 6 and {(d.coff - GUARD) // CL[d.htype] for d in ds} == {0, 1, 3}
    assert any(EXT_MET["last1"](d) for d in ds if d.nch >= 2) and any(EXT_MET["rec_nodiv"](d) for d in ds)
    assert extents_geom(32768, 6, 7, 30001) == (32766, 6, 32724, 16218)         # a geometry worked by hand
    assert extents_class(2, 16384, 16384, 256, 16, 4096, 1) == "wave"
    assert extents_class(2, 16384, 16384, 256, 16, 4095, 1) == "split"
    assert extents_class(7, 8192, 8192, 256, 0, 1, 1) == "wave" and extents_class(1, 8192, 8192, 256, 0, 1, 1) == "group"
    assert extents_class(3, 8208, 8208, 256, 8208, 2, 1) == "wave" and extents_class(3, 4096, 4096, 256, 4100, 2, 1) == "bytes"

    for call in CALLS[1:5]:
        all_ = call.endswith("_all")
        ds = [draw(call, s) for s in range(NSEEDS[call])]
        assert all(d.S * (d.k + d.p) * d.C <= MAX_BYTES and d.C % d.rb == 0 for d in ds), call
        fused_reached(call, ds, [d.kernel for d in ds])
        assert any(d.why == ["adler"] for d in ds) and any(d.why == ["chunk"] for d in ds), call
        assert any(d.why == ["csmis"] for d in ds), call
        assert any(skew_alone(d) for d in ds), call
        assert any(fused_stride_alone(d) for d in ds), call
        assert any("cell" in d.why for d in ds), call
        assert len({d.khkey for d in ds if d.khkey}) > NKH_CACHE, call              # the table cache evicts
        assert {d.C for d in ds} == set(CELLS) and {d.cs for d in ds} == set(FCHUNKS), call
        assert {d.rb for d in ds} == set(FRECS) and {d.S for d in ds} == set(STRIPES), call
        assert {d.cols for d in ds} == set(COLS) and {(d.gx, d.gy) for d in ds} == set(GRIDS), call
        for g in GRIDS[-2:]:            # an override above the counts reaches the fused kernel
            assert any((d.gx, d.gy) == g and not d.why for d in ds), (call, g)
        assert {d.mode for d in ds} == set(ENC_MODES if call.startswith("encode") else REC_MODES), call
        if all_:
            assert {d.route for d in ds} == {0, 1, 2}, call
            assert any(d.src and d.route == 1 and (d.htype, d.k, d.rows) not in FUSED_DEFAULT for d in ds), call
            assert any(d.src and d.route == 0 for d in ds), call
            assert any(not d.why and not d.src and d.route == 2 and (d.htype, d.k, d.rows) in FUSED_DEFAULT
                       for d in ds), call
            assert any(not d.why and not d.src and d.route == 0 for d in ds), call
            assert any(src_array_alone(d) and not d.src and d.route == 1 for d in ds), call
        if call.startswith("recover"):
            assert any(all(e >= d.k for e in d.errs) and len(d.errs) == d.p for d in ds), call  # the encode rows again
            assert any(any(e < d.k for e in d.errs) and any(e >= d.k for e in d.errs) for d in ds), call
            assert any(d.errs != sorted(d.errs) for d in ds), call
    assert recov_order(4, 2, [5, 4]) == ([0, 1, 2, 3], [4, 5]) and recov_order(4, 2, [5, 1]) == ([0, 2, 3, 4], [1, 5])
    assert fused_ncols(0, 5, 2, 8, 2, False) == 2 and fused_ncols(0, 5, 2, 8, 2, True) == 5 and fused_ncols(3, 2, 1, 4, 1, False) == 2

    ds = [draw("csum_compare", s) for s in range(NSEEDS["csum_compare"])]
    compare_reached(ds)
    assert {(d.htype, d.n) for d in ds} == {(t, n) for t in TYPES for n in CMP_N}
    assert {d.count for d in ds} == set(CMP_COUNTS)
    for d in ds:
        pos = compare_positions(d)
        assert pos.size == (d.n if d.count == "all" else min(d.count, d.n)), describe(d)
    assert any(d.n > CAP and compare_positions(d).size == 1 for d in ds)        # the lowest index is beyond the grid
    assert any(d.n >= 256 and {0, d.n - 1} <= set(compare_positions(d).tolist()) and d.count != "all" for d in ds)


# ------------------------------------------------------------------- 2. one run per call
@contextlib.contextmanager
def settings(ctx, ecglib, d):
    """The launch settings of a case; all back at 0 whatever happened (launch() sees to ecg_set_launch)."""
    L = ecglib.lib()
    try:
        assert L.ecg_set_fused_cols(ctx.h, d.cols) == 0 and L.ecg_set_csum_launch(ctx.h, d.blocks) == 0
        ctx.set_csum_all_route(d.route)
        yield
    finally:
        L.ecg_set_fused_cols(ctx.h, 0)
        L.ecg_set_csum_launch(ctx.h, 0)
        ctx.set_csum_all_route(0)
        ctx.set_launch(0, 0, 0)


def csum_array(coff, sums):
    """The allocation of a checksum array: guard, the array exactly, slack, guard.  -> (its image
    before the call, after it)"""
    raw = np.ascontiguousarray(sums).reshape(-1).view(np.uint8)
    pre = Mem(coff + raw.size + CSLACK + GUARD)
    pre.at(coff, raw.size)[:] = PRE
    want = pre.copy()
    want.at(coff, raw.size)[:] = raw
    return pre, want


def cell_csums(oracle, d, cells):
    """The oracle's checksums of every cell (last axis) as an extent from record index 0."""
    flat = np.ascontiguousarray(cells).reshape(-1, d.C)
    out = oracle.csum_extents(d.htype, d.cs, d.rb, 0, d.C // d.rb, flat.reshape(-1), ext_stride=d.C,
                              n_ext=flat.shape[0])
    return out.reshape(cells.shape[:-1] + (d.nch,))


def called(ctx, ecglib, d, fn, what):
    """fn() under the case's settings; -> the kernel it ran last.  csum_chunks advances by d.chunks."""
    name = []
    before = ctx.stats()["csum_chunks"]
    with settings(ctx, ecglib, d):
        launch(ctx, d, lambda: (fn(), name.append(ecglib.last_kernel())))
    assert ctx.stats()["csum_chunks"] - before == d.chunks, what
    assert name[0] == d.kernel, f"{what}: ran {name[0]}, predicted {d.kernel}"
    return name[0]


def run_extents(ctx, oracle, ecglib, d):
    what = describe(d)
    rng = np.random.default_rng(d.data_seed)
    img = Mem(d.size, d.win)
    if d.stride >= d.ext or d.n_ext == 1:
        for e in range(d.n_ext):
            img.at(d.base + e * d.stride, d.ext)[:] = rng.integers(0, 256, d.ext, dtype=np.uint8)
    else:                       # extents that overlap: one run of bytes under all of them
        img.at(d.base, d.span)[:] = rng.integers(0, 256, d.span, dtype=np.uint8)
    geom = (d.htype, d.cs, d.rb, d.idx, d.nr)
    if d.stride == 0:
        sums = np.tile(oracle.csum_extents(*geom, img.at(d.base, d.ext)), (d.n_ext, 1))
    elif d.n_ext <= 5:
        sums = np.concatenate([oracle.csum_extents(*geom, img.at(d.base + e * d.stride, d.ext)) for e in range(d.n_ext)])
    else:
        sums = oracle.csum_extents(*geom, img.at(d.base, d.span), ext_stride=d.stride, n_ext=d.n_ext)
    assert sums.shape == (d.n_ext, d.nch), what
    pre, want = csum_array(d.coff, sums)
    with Device(ctx, ecglib) as dev:
        buf, out = dev.load(img), dev.load(pre)
        assert buf.ptr % 256 == 0 and out.ptr % 256 == 0
        name = called(ctx, ecglib, d, lambda: ctx.csum_extents(*geom, buf.ptr + d.base, d.stride, d.n_ext,
                                                               out.ptr + d.coff), what)
        same(out, want, what, "csums")
        same(buf, img, what, "extents")
    return name


def run_encode(ctx, oracle, ecglib, d):
    k, p, C, S = d.k, d.p, d.C, d.S
    what, all_ = describe(d), d.call.endswith("_all")
    rng = np.random.default_rng(d.data_seed)
    cells = rng.integers(0, 256, (S, k, C), dtype=np.uint8)
    coef = oracle.cauchy1(k, p)[k:]
    parity = np.stack([oracle.encode_data(coef, cells[s]) for s in range(S)])
    data, par = Arr(S, k, C, d.dss, C), Arr(S, p, C, d.pss, d.pcs)
    D = Mem(d.dsize, d.dwin)
    P = D if d.same_buf else Mem(d.psize)
    D.put(d.dbase, data, cells)
    P.put(d.pbase, par, np.full((S, p, C), ERASED, dtype=np.uint8))
    wantD = D.copy()
    wantP = wantD if d.same_buf else P.copy()
    wantP.put(d.pbase, par, parity)
    ppre, pwant = csum_array(d.coff[0], cell_csums(oracle, d, parity).transpose(1, 0, 2))      # [p][S][nch]
    if all_:
        dpre, dwant = csum_array(d.coff[1], cell_csums(oracle, d, cells).transpose(1, 0, 2))   # [k][S][nch]
    with Device(ctx, ecglib) as dev:
        dbuf = dev.load(D)
        pbuf = dbuf if d.same_buf else dev.load(P)
        pcs = dev.load(ppre)
        dcs = dev.load(dpre) if all_ else None
        args = (k, p, C, S, dbuf.ptr + d.dbase, d.dss, pbuf.ptr + d.pbase, d.pcs, d.pss, d.htype, d.cs, d.rb)
        if all_:
            name = called(ctx, ecglib, d, lambda: ctx.encode_csum_all(*args, dcs.ptr + d.coff[1], pcs.ptr + d.coff[0]),
                          what)
            same(dcs, dwant, what, "data_csums")
        else:
            name = called(ctx, ecglib, d, lambda: ctx.encode_csum(*args, pcs.ptr + d.coff[0]), what)
        same(pcs, pwant, what, "parity csums")
        same(dbuf, wantD, what, "data")
        if not d.same_buf:
            same(pbuf, wantP, what, "parity")
    return name


def run_recover(ctx, oracle, ecglib, d):
    k, p, C, S = d.k, d.p, d.C, d.S
    what, all_ = describe(d), d.call.endswith("_all")
    rng = np.random.default_rng(d.data_seed)
    stripes = np.empty((S, k + p, C), dtype=np.uint8)
    stripes[:, :k] = rng.integers(0, 256, (S, k, C), dtype=np.uint8)
    coef = oracle.cauchy1(k, p)[k:]
    for s in range(S):
        stripes[s, k:] = oracle.encode_data(coef, stripes[s, :k])
    arr = Arr(S, k + p, C, d.stride, C)
    want = Mem(d.dsize)
    want.put(d.dbase, arr, stripes)
    img = want.copy()
    broken = stripes.copy()
    broken[:, d.errs] = ERASED
    img.put(d.dbase, arr, broken)
    sums = cell_csums(oracle, d, stripes).transpose(1, 0, 2)        # [k+p][S][nch]
    dec, _ = recov_order(k, p, d.errs)
    opre, owant = csum_array(d.coff[0], sums[d.errs])               # rows in err_list order
    spre, swant = csum_array(d.coff[1], sums[dec])
    with Device(ctx, ecglib) as dev:
        buf, out = dev.load(img), dev.load(opre)
        sout = dev.load(spre) if all_ else None
        args = (k, p, C, S, buf.ptr + d.dbase, d.stride, d.errs, d.htype, d.cs, d.rb, out.ptr + d.coff[0])
        if all_:
            idx = []
            name = called(ctx, ecglib, d, lambda: idx.extend(ctx.recover_csum_all(*args, sout.ptr + d.coff[1])), what)
            assert idx == [int(c) for c in ecglib.recov_matrix(k, p, d.errs)[1]] == dec, what
            same(sout, swant, what, "src_csums")
        else:
            name = called(ctx, ecglib, d, lambda: ctx.recover_csum(*args), what)
        same(out, owant, what, "csums")
        same(buf, want, what, "stripes")
    return name


def run_compare(ctx, oracle, ecglib, d):
    what, cl = describe(d), CL[d.htype]
    rng = np.random.default_rng(d.data_seed)
    want = rng.integers(0, 256, (d.n, cl), dtype=np.uint8)
    got = want.copy()
    pos = compare_positions(d)
    got[pos, rng.integers(0, cl, pos.size)] ^= (1 << rng.integers(0, 8, pos.size)).astype(np.uint8)
    assert int((got != want).any(axis=1).sum()) == pos.size
    imgs = []
    for a, skew in zip((got, want), d.skews):
        m = Mem(GUARD + skew + a.size + GUARD)
        m.at(GUARD + skew, a.size)[:] = a.reshape(-1)
        imgs.append(m)
    rpre = Mem(GUARD + 16 + GUARD)
    rpre.at(GUARD, 16)[:] = ERASED
    rwant = rpre.copy()
    rwant.at(GUARD, 16)[:] = np.array([pos.size, int(pos[0]) if pos.size else U64MAX], dtype=np.uint64).view(np.uint8)
    with Device(ctx, ecglib) as dev:
        gbuf, wbuf, res = dev.load(imgs[0]), dev.load(imgs[1]), dev.load(rpre)
        ctx.csum_compare(d.htype, gbuf.ptr + GUARD + d.skews[0], wbuf.ptr + GUARD + d.skews[1], d.n, res.ptr + GUARD)
        name = ecglib.last_kernel() if d.n else "none"
        ctx.sync()
        same(res, rwant, what, "result")
        same(gbuf, imgs[0], what, "got")
        same(wbuf, imgs[1], what, "want")
        assert name == ("ecg_csum_compare_kernel" if d.n else "none"), what
    return name


RUN = {"csum_extents": run_extents, "encode_csum": run_encode, "encode_csum_all": run_encode,
       "recover_csum": run_recover, "recover_csum_all": run_recover, "csum_compare": run_compare}


def run_draw(ctx, oracle, ecglib, d):
    """One case; an error the library reports names the seed and the draw like a failed assert."""
    try:
        return RUN[d.call](ctx, oracle, ecglib, d)
    except ecglib.EcgError as e:
        raise AssertionError(f"{describe(d)}: {e}") from e


def run_case(ctx, oracle, ecglib, call, seed):
    return run_draw(ctx, oracle, ecglib, draw(call, seed))


def run_all(ctx, oracle, ecglib, call):
    """Every seed of a call.  -> (the draws, the kernel each ran last)"""
    ds = [draw(call, seed) for seed in range(NSEEDS[call])]
    names = [run_draw(ctx, oracle, ecglib, d) for d in ds]
    hist = {}
    for n in names:
        hist[n] = hist.get(n, 0) + 1
    print(call, "kernels:", dict(sorted(hist.items())))
    if call not in ("csum_extents", "csum_compare"):
        print(call, "multiplier-table keys:", len({d.khkey for d in ds if d.khkey}))
    return ds, names


@pytest.mark.gpu
def test_csum_extents(ctx, oracle, ecglib):
    extents_reached(*run_all(ctx, oracle, ecglib, "csum_extents"))


@pytest.mark.gpu
def test_encode_csum(ctx, oracle, ecglib):
    fused_reached("encode_csum", *run_all(ctx, oracle, ecglib, "encode_csum"))


@pytest.mark.gpu
def test_encode_csum_all(ctx, oracle, ecglib):
    fused_reached("encode_csum_all", *run_all(ctx, oracle, ecglib, "encode_csum_all"))


@pytest.mark.gpu
def test_recover_csum(ctx, oracle, ecglib):
    fused_reached("recover_csum", *run_all(ctx, oracle, ecglib, "recover_csum"))


@pytest.mark.gpu
def test_recover_csum_all(ctx, oracle, ecglib):
    fused_reached("recover_csum_all", *run_all(ctx, oracle, ecglib, "recover_csum_all"))


@pytest.mark.gpu
def test_csum_compare(ctx, oracle, ecglib):
    ds, names = run_all(ctx, oracle, ecglib, "csum_compare")
    compare_reached(ds)
    assert set(names) == {"ecg_csum_compare_kernel", "none"}


# --------------------------------------------------------------- 4. offsets past 4 GiB
def far_extents(stride):
    """3 extents of three chunks and a tail, `stride` apart."""
    d = SimpleNamespace(call="csum_extents", seed=f"far-{stride % 16}", htype=2, gx=0, gy=0, variant=0, cols=0, route=0,
                        blocks=0, cs=16384, rb=1, idx=0, nr=3 * 16384 + 100, n_ext=3, stride=stride, skew=0,
                        coff=GUARD, data_seed=41)
    d.rcs, d.nch, d.first, d.last = extents_geom(d.cs, d.rb, d.idx, d.nr)
    d.ext = d.nr
    d.size, d.base, d.win = far_place([e * stride for e in range(d.n_ext)], d.ext)
    d.span = (d.n_ext - 1) * stride + d.ext
    d.cls = extents_class(d.htype, d.rcs, d.first, d.base, d.stride, d.n_ext, d.nch)
    d.kernel, d.chunks = extents_kernel(d.htype, d.cls), d.n_ext * d.nch
    return d


def far_encode():
    """EC_4P2, S = 3, the stripes' data far apart, the parity rows tight in a buffer of their own."""
    k, p, C, S = 4, 2, 8192 + 48, 3
    d = SimpleNamespace(call="encode_csum", seed="far", htype=2, k=k, rows=p, p=p, C=C, S=S, cs=4096, rb=1, cols=0,
                        route=0, blocks=0, gx=0, gy=0, variant=0, coff=[GUARD, GUARD], skews=[0, 0], mode="far",
                        dss=FAR_STRIDE, pcs=S * C, pss=C, same_buf=False, data_seed=42)
    d.dsize, d.dbase, d.dwin = far_place([s * d.dss + j * C for s in range(S) for j in range(k)], C)
    d.psize, (d.pbase,) = place([(Arr(S, p, C, d.pss, d.pcs), 0)])
    d.ptrs, d.strides = [d.dbase, d.pbase], [d.dss, d.pss]
    d.offs = [j * C for j in range(k)] + [r * d.pcs for r in range(p)]
    d.last_src, d.last_out = (d.dbase + (k - 1) * C, d.dss), (d.pbase + (p - 1) * d.pcs, d.pss)
    return finish_fused(d)


@pytest.mark.gpu
def test_offsets_past_4GiB(ctx, oracle, ecglib):
    """An extent stride (the split kernel; + 4: the byte kernel) and a data stripe stride (the
    fused kernel) of 2^32 - 2048, each in an allocation of about 8.6 GiB.  Skips only if the
    device refuses the allocation."""
    for stride, cls in ((FAR_STRIDE, "split"), (FAR_STRIDE + 4, "bytes")):
        d = far_extents(stride)
        assert d.cls == cls
        assert run_draw(ctx, oracle, ecglib, d) == extents_kernel(2, cls)
    d = far_encode()
    assert d.fused and d.kernel == "ecg_mm_csum_kernel<4,2,crc32>"
    assert run_draw(ctx, oracle, ecglib, d) == d.kernel
