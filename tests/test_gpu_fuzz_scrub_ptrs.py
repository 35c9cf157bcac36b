"""Seeded random shapes, sizes, alignments and corruption through ecg_scrub_ptrs (and so through
ecg_verify_ptrs and ecg_repair_ptrs): 48 cases.  Drawn per case: (k, p) from all k <= 16, p <= 8;
the cell size from 1 .. 12 KiB at any residue; a skew of 0 .. 47 bytes per cell (or, half of the
time, cells and size on 16 bytes, so that the lane kernels run); 1 .. 150 stripes (fewer when
the stripes would pass 8 MiB); 0 .. 6 corrupted stripes with one or two wrong cells at drawn
bytes.  Expected: every status word and the verify result from test_gpu_verify.model_status on the
CPU, the kernel named from the drawn alignment, the repair result from the classified words, and
the bytes from the strided twin (ecg_verify + ecg_repair on the gathered image).  No case is
skipped or filtered: the model gives an expectation for every draw."""
import numpy as np
import pytest

from tests import test_gpu_scrub_ptrs as sp
from tests import test_gpu_verify as vg
from tests.test_gpu_recover_masks_ptrs import same

pytestmark = pytest.mark.gpu

N = 48
MAX_BYTES = 8 << 20         # S * (k+p) * C of one case
U64MAX = (1 << 64) - 1


def draw(seed):
    rng = np.random.default_rng(77000 + seed)
    k, p = int(rng.integers(1, 17)), int(rng.integers(1, 9))
    aligned = bool(rng.integers(0, 2))
    C_ = int(rng.integers(1, 12 * 1024 + 1))
    if aligned:
        C_ = max(16, C_ // 16 * 16)
    S_ = min(int(rng.integers(1, 151)), max(1, MAX_BYTES // ((k + p) * C_)))
    skews = rng.integers(0, 3, (S_, k + p)) * 16 if aligned else rng.integers(0, 48, (S_, k + p))
    aligned = aligned or (C_ % 16 == 0 and not (skews % 16).any())
    flips = []
    for s in rng.permutation(S_)[:int(rng.integers(0, 7))]:
        for c in rng.permutation(k + p)[:int(rng.integers(1, 3))]:
            flips.append((int(s), int(c), int(rng.integers(0, C_)), int(rng.integers(1, 256))))
    return k, p, C_, S_, aligned, skews, flips


def codewords(oracle, k, p, C_, S_, seed):
    data = np.random.default_rng(88000 + seed).integers(0, 256, (S_, k, C_), dtype=np.uint8)
    par = oracle.encode_batch(k, p, C_, S_, data.reshape(-1)).reshape(p, S_, C_)
    return np.concatenate([data, par.transpose(1, 0, 2)], axis=1)


@pytest.mark.parametrize("seed", range(N))
def test_fuzz_scrub_ptrs(ctx, ecglib, oracle, seed):
    k, p, C_, S_, aligned, skews, flips = draw(seed)
    sc = sp.Scrub(ctx, k, p, C_, codewords(oracle, k, p, C_, S_, seed), skew=lambda s, c: int(skews[s, c]))
    try:
        for f in flips:
            sc.poke(*f)
        # the model: status words, their reading, the two results
        status = [sp.clean_word(k)] * S_
        for s in sorted({f[0] for f in flips}):
            stripe = np.stack([sc.rig.cell(sc.rig.img, s, c) for c in range(k + p)])
            rows, cand = vg.model_status(oracle, k, p, stripe[:k], stripe[k:])
            status[s] = rows | cand << 8
        cells = [ecglib.verify_cell(w, k, p) for w in status]
        bad = [s for s, c in enumerate(cells) if c != -1]
        one = [s for s in bad if cells[s] >= 0]
        many = [s for s in bad if cells[s] == -2]
        vwords = [len(bad), min(bad) if bad else U64MAX, len(one), len(many)]
        rwords = [len(one), min(many) if many else U64MAX, sum(1 for s in one if cells[s] < k), len(many)]
        # the strided twin
        tstatus, tverify = sc.twin_verify()
        twords, want = sc.twin_repair()
        assert tstatus == status and tverify == vwords and twords == rwords
        # the call
        for b in sc.status + sc.result:
            b.fill(0xEE)
        tab = sc.rig.table()
        ctx.scrub_ptrs(*sc.geo, tab, sc.status[0].ptr, sc.result[0].ptr, sc.result[1].ptr)
        assert ecglib.last_kernel() == (sp.repair_kernel(k) if aligned else sp.REPAIR_BYTE), (ecglib.last_kernel(), aligned)
        ctx.verify_ptrs(*sc.geo, tab, sc.status[1].ptr, sc.result[2].ptr)
        assert ecglib.last_kernel() == (sp.verify_kernel(k, p) if aligned else sp.VERIFY_BYTE), ecglib.last_kernel()
        ctx.sync()
        assert sp.words(sc.status[0], np.uint32) == status
        assert sp.words(sc.result[0]) == vwords and sp.words(sc.result[1]) == rwords
        same(sc.rig.buf.download(), want)
        # the second check reports what the twin's second check reports of the repaired bytes
        assert (sp.words(sc.status[1], np.uint32), sp.words(sc.result[2])) == sc.twin_verify()
        if len(many) == 0 and all(len({f[1] for f in flips if f[0] == s}) == 1 for s in one):
            same(want, sc.clean)                                        # one wrong cell per stripe: all put right
    finally:
        sc.free()
