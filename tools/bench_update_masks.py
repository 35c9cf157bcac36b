"""ecg_update_masks (include/ecg.h) against the routes it replaces.  EC_8P2 and
EC_16P2 at 128 KiB and 1 MiB cells, 512 MiB of one cell column per batch as the
EC_8P2_1MiB_update_*cell rows of bench.py (S = 512 at 1 MiB, 4096 at 128 KiB);
parity [p][S][C] at the padded row pitch.  A delta update XORs into the
parity, so every variant may run any number of times on the same buffers.

  (1) homogeneous   every stripe changed the same n cells (n = 1: cell 3, n = 2:
                    cells 1 and 6):
        update          ecg_update(cell_idx) over packed cells [S][n][C] -- the
                        reference; timed in 4 repeats, whose spread is the margin
        masks_packed    ecg_update_masks(ECG_UM_PACKED) over the same buffers
        masks_full      ecg_update_masks over full images [S][k][C]
        masks_full_pad  the same with the images' stripes k*C + 4 KiB apart
                        instead of k*C, a power of two (what the parity row pitch
                        does for the rows)
  (2) mixed         stripes with 1..4 random changed cells, one in eight clean:
        masks           one ecg_update_masks over the full images (masks_pad:
                        their stripes k*C + 4 KiB apart)
        update_per_mask today's route (a): one ecg_update per distinct mask on
                        sub-batches already gathered into [Sg][n][C] (the gather
                        itself is not timed)
        update_ptrs     today's route (b): one ecg_update_ptrs over one request
                        per changed cell, the pointer table already built
      all three by the host clock around the calls and a stream sync, so the
      host work of update_ptrs (sorting, folding, colouring, staging) counts;
      masks and update_per_mask by device events too
  (3) clean         S = 8192 zero masks (k = 8, p = 2), without and with
                    ECG_RM_SPARSE: the grp = 1 grid against the grp = 64 one.
                    No cell is read or written, so the 1 MiB case passes the
                    128 KiB case's buffers with strides of 0.

ms, GiB/s of updated cells, and the fraction of the 8 TB/s HBM spec of the
derived (2n + 2p) * C * S bytes.  Device events around blocks of ~1 ms of
back-to-back launches, the variants of a row alternating (bench.py
time_interleaved), median of ITERS blocks.
-> the JSON file given with --out PATH (default build/bench_update_masks.json).
Bench infrastructure (no oracle)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from daos_amd import ecg  # noqa: E402
from tools.datagen import stripe_bytes  # noqa: E402

ITERS, WARM, REPEATS = 15, 5, 4
SHAPES = ((8, 2, 1 << 20), (8, 2, 128 << 10), (16, 2, 1 << 20), (16, 2, 128 << 10))
COLUMN = 512 << 20              # bytes of one cell column of a batch
HOMOG = ([3], [1, 6])
HBM = bench.HBM_PEAK_GBS
GIB = float(1 << 30)
U64MAX = (1 << 64) - 1


def main():
    quick = "--quick" in sys.argv           # a rehearsal at toy sizes
    column = (4 << 20) if quick else COLUMN
    ctx = ecg.Context(0)
    L = ecg.lib()

    def filled(nbytes, seed):
        buf = ctx.alloc(nbytes)
        blk = stripe_bytes(min(256 << 20, nbytes), seed)
        buf.upload(blk)
        for off in range(blk.size, nbytes, blk.size):
            ecg._chk(L.ecg_memcpy(ctx.h, buf.ptr + off, buf.ptr, min(blk.size, nbytes - off), 2, None), "D2D")
        ctx.sync()
        return buf

    def words(x):
        return [int(v) for v in x.download().view(np.uint64)]

    def masks_dev(m):
        d = ctx.alloc(4 * len(m))
        d.upload(np.asarray(m, dtype=np.uint32).view(np.uint8))
        return d

    def rates(ms, n_cells, n_stripes, p, Cb):
        """n_cells updated cells in n_stripes stripes with work, ms per call."""
        alg = (2 * n_cells + 2 * p * n_stripes) * Cb
        return {"ms": round(ms, 4), "GiBps_updated": round(n_cells * Cb / (ms / 1e3) / GIB, 1),
                "hbm_frac": round(alg / ms / 1e6 / HBM, 4)}

    def host_ms(fn, reps=9):
        fn()
        ctx.sync()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ctx.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
        return sorted(ts)[len(ts) // 2]

    res = {"iters": ITERS, "repeats": REPEATS, "shapes": {}}
    for k, p, Cb in SHAPES:
        S = column // Cb
        name = f"EC_{k}P{p}_{Cb >> 10}KiB_x{S}"
        pitch = S * Cb + bench.PARITY_ROW_PAD
        upad = k * Cb + bench.PARITY_ROW_PAD
        old, new = filled(S * upad, 12), filled(S * upad, 13)
        par = filled(p * pitch, 14)
        result = ctx.alloc(32)
        row = {}

        # ---- (1) homogeneous: the packed buffers are the first n cell slots of the images
        for cells in HOMOG:
            n = len(cells)
            m = masks_dev([sum(1 << j for j in cells)] * S)
            fns = [lambda: ctx.update(k, p, Cb, S, cells, old.ptr, new.ptr, n * Cb, par.ptr, pitch, Cb),
                   lambda: ctx.update_masks(k, p, Cb, S, old.ptr, new.ptr, n * Cb, par.ptr, pitch, Cb, m.ptr,
                                            result.ptr, ecg.UM_PACKED),
                   lambda: ctx.update_masks(k, p, Cb, S, old.ptr, new.ptr, k * Cb, par.ptr, pitch, Cb, m.ptr,
                                            result.ptr, 0),
                   lambda: ctx.update_masks(k, p, Cb, S, old.ptr, new.ptr, upad, par.ptr, pitch, Cb, m.ptr,
                                            result.ptr, 0)]
            reps = [bench.time_interleaved(ctx, fns, ITERS, WARM) for _ in range(REPEATS)]
            kern = ecg.last_kernel()
            ctx.sync()
            assert words(result) == [S, U64MAX, n * S, 0], words(result)
            upd = [r[0] for r in reps]
            names = ("update", "masks_packed", "masks_full", "masks_full_pad")
            med = [sorted(r[i] for r in reps)[REPEATS // 2] for i in range(len(names))]
            h = {"update": rates(med[0], n * S, S, p, Cb), "masks_packed": rates(med[1], n * S, S, p, Cb),
                 "masks_full": rates(med[2], n * S, S, p, Cb), "masks_full_pad": rates(med[3], n * S, S, p, Cb),
                 "kernel": kern, "ms_repeats": {v: [round(r[i], 4) for r in reps] for i, v in enumerate(names)},
                 "update_spread": round(max(upd) / min(upd), 4),
                 "update_over_masks_packed": round(med[0] / med[1], 4),
                 "update_over_masks_full": round(med[0] / med[2], 4),
                 "update_over_masks_full_pad": round(med[0] / med[3], 4)}
            row[f"homog_{n}cell"] = h
            print(name, f"homog_{n}cell", json.dumps(h), flush=True)
            m.free()

        # ---- (2) mixed: 1..4 random cells, one stripe in eight clean
        rng = np.random.default_rng(1000 * k + p)
        mixed = []
        for s in range(S):
            js = rng.choice(k, int(rng.integers(1, 5)), replace=False)
            mixed.append(0 if s % 8 == 7 else sum(1 << int(j) for j in js))
        ncell = sum(bin(x).count("1") for x in mixed)
        nwork = sum(1 for x in mixed if x)
        m = masks_dev(mixed)
        groups = {}
        for s, x in enumerate(mixed):
            if x:
                groups.setdefault(x, []).append(s)
        # the gathered sub-batches of route (a): group g's packed cells follow the groups before
        # it in the images' memory, its parity cells in the parity rows
        plan, cell_at, stripe_at = [], 0, 0
        for x, ss in sorted(groups.items()):
            js = [j for j in range(k) if x >> j & 1]
            plan.append((js, len(ss), cell_at * Cb, stripe_at * Cb))
            cell_at += len(js) * len(ss)
            stripe_at += len(ss)

        def per_mask():
            for js, sg, coff, poff in plan:
                ctx.update(k, p, Cb, sg, js, old.ptr + coff, new.ptr + coff, len(js) * Cb, par.ptr + poff, pitch, Cb)

        # route (b): one request per changed cell on the full images, the table built once
        reqs = [(j, s) for s, x in enumerate(mixed) for j in range(k) if x >> j & 1]
        tab = (C.c_void_p * (len(reqs) * (2 + p)))()
        vec = np.array([j for j, _ in reqs], dtype=np.uint8)
        for i, (j, s) in enumerate(reqs):
            tab[i * (2 + p)] = old.ptr + (s * k + j) * Cb
            tab[i * (2 + p) + 1] = new.ptr + (s * k + j) * Cb
            for r in range(p):
                tab[i * (2 + p) + 2 + r] = par.ptr + r * pitch + s * Cb
        vecp = vec.ctypes.data_as(C.POINTER(C.c_ubyte))

        def ptrs():
            ecg._chk(L.ecg_update_ptrs(ctx.h, k, p, Cb, len(reqs), tab, vecp, None), "update_ptrs")

        def masks():
            ctx.update_masks(k, p, Cb, S, old.ptr, new.ptr, k * Cb, par.ptr, pitch, Cb, m.ptr, result.ptr, 0)

        def masks_pad():
            ctx.update_masks(k, p, Cb, S, old.ptr, new.ptr, upad, par.ptr, pitch, Cb, m.ptr, result.ptr, 0)

        ev = bench.time_interleaved(ctx, [masks, per_mask, masks_pad], ITERS, WARM)
        hm = [host_ms(f) for f in (masks, per_mask, ptrs)]
        masks()
        ctx.sync()
        assert words(result) == [nwork, U64MAX, ncell, 0], words(result)
        mx = {"stripes": S, "stripes_with_work": nwork, "cells": ncell, "distinct_masks": len(groups),
              "requests": len(reqs),
              "masks": dict(rates(ev[0], ncell, nwork, p, Cb), host_ms=round(hm[0], 4)),
              "masks_pad": rates(ev[2], ncell, nwork, p, Cb),
              "update_per_mask": {"ms": round(ev[1], 4), "host_ms": round(hm[1], 4), "launches": len(plan)},
              "update_ptrs": {"host_ms": round(hm[2], 4)},
              "per_mask_over_masks": round(hm[1] / hm[0], 3), "ptrs_over_masks": round(hm[2] / hm[0], 3)}
        row["mixed"] = mx
        print(name, "mixed", json.dumps(mx), flush=True)
        m.free()

        res["shapes"][name] = row
        for x in (old, new, par, result):
            x.free()
    # ---- (3) a clean batch of 8192 stripes on each grid.  No cell is read or written: the
    # images are allocated for the 128 KiB case, and the 1 MiB case passes them with strides of 0
    k, p, Cb, SC = 8, 2, 128 << 10, 64 if quick else 8192
    pitch = SC * Cb + bench.PARITY_ROW_PAD
    old, par, result = ctx.alloc(SC * k * Cb), ctx.alloc(p * pitch), ctx.alloc(32)
    zero = masks_dev([0] * SC)
    res["clean"] = {}
    for cb2, ustride, pcs, pss in ((Cb, k * Cb, pitch, Cb), (1 << 20, 0, 0, 0)):
        fns = [lambda fl=fl: ctx.update_masks(k, p, cb2, SC, old.ptr, old.ptr, ustride, par.ptr, pcs, pss, zero.ptr,
                                              result.ptr, fl) for fl in (0, ecg.RM_SPARSE)]
        reps = [bench.time_interleaved(ctx, fns, ITERS, WARM) for _ in range(REPEATS)]
        ctx.sync()
        assert words(result) == [0, U64MAX, 0, 0]
        cl = {"stripes": SC, "ms_grp1": [round(r[0], 4) for r in reps],
              "ms_grp64_sparse": [round(r[1], 4) for r in reps]}
        res["clean"][f"EC_8P2_{cb2 >> 10}KiB_x{SC}"] = cl
        print("clean", f"{cb2 >> 10}KiB", json.dumps(cl), flush=True)
    for x in (old, par, result, zero):
        x.free()
    out = os.path.join(ROOT, "build", "bench_update_masks.json")
    if "--out" in sys.argv:
        out = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
