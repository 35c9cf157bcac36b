"""ecg_agg_masks (include/ecg.h) against the two calls it chooses between, on the batches of
tools/bench_update_masks.py: EC_8P2 and EC_16P2 at 1 MiB x 512 and 128 KiB x 4096 stripes, full
images [S][k][C], parity [p][S][C] at the padded row pitch.  Every call may run any number of
times on the same buffers (the timing does not depend on what the cells hold).

  (1) homogeneous   every stripe names the same n cells (the low n), n = 1 .. k:
        update_masks    ecg_update_masks -- the reference of (a); its REPEATS repeats give the
                        margin (max / min)
        agg_Tk          ecg_agg_masks(recalc_above = k): every stripe on the delta route   (a)
        agg_T0          ecg_agg_masks(recalc_above = 0): every stripe re-encoded           (b)
        encode          ecg_encode of a full image at the same strides                     (b)
        agg_auto        ecg_agg_masks(ECG_AGG_AUTO): the route the arithmetic picks        (c)
      "crossover_measured": the lowest n from which agg_T0 stays faster than agg_Tk, beside
      ecg_agg_threshold(k, p) + 1, the lowest n ECG_AGG_AUTO re-encodes
  (2) mixed         half the stripes name 1 cell, half all k (alternating):
        agg_auto against update_masks (and encode, which rewrites every stripe)         (d)

  --update-only     time ecg_update_masks alone, n = 1 .. k -- with --lib PATH the row of a
                    library built from another tree (the parent commit's, for (a))
  --lib PATH        load that libecg.so instead of the tree's
  --quick           a rehearsal at toy sizes
  --out PATH        the JSON result (default build/bench_agg_masks.json)

ms and the fraction of the 8 TB/s HBM spec of the bytes each route has to move ((2n + 2p) C S for
the delta, (k + p) C S for the re-encode).  Device events around blocks of ~1 ms of back-to-back
launches, the calls of a row alternating (bench.py time_interleaved), median of ITERS blocks,
then the median of REPEATS such runs.  Bench infrastructure (no oracle)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from daos_amd import ecg  # noqa: E402
from tools.datagen import stripe_bytes  # noqa: E402

ITERS, WARM, REPEATS = 15, 5, 4
SHAPES = ((8, 2, 1 << 20), (8, 2, 128 << 10), (16, 2, 1 << 20), (16, 2, 128 << 10))
COLUMN = 512 << 20              # bytes of one cell column of a batch
HBM = bench.HBM_PEAK_GBS
U64MAX = (1 << 64) - 1


def main():
    quick = "--quick" in sys.argv
    only = "--update-only" in sys.argv
    if "--lib" in sys.argv:         # possibly a library from before ecg_agg_masks: bind what it has
        ecg.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
        probe = C.CDLL(ecg.LIB_PATH)
        ecg._SIGS[:] = [sig for sig in ecg._SIGS if hasattr(probe, sig[0])]
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

    def med(reps, i):
        return sorted(r[i] for r in reps)[len(reps) // 2]

    def frac(ms, nbytes):
        return round(nbytes / ms / 1e6 / HBM, 4)

    res = {"iters": ITERS, "repeats": REPEATS, "library": sys.argv[sys.argv.index("--lib") + 1] if "--lib" in sys.argv else "tree",
           "build": ecg.build_info().get("src_sha256"), "shapes": {}}
    for k, p, Cb in SHAPES:
        S = column // Cb
        name = f"EC_{k}P{p}_{Cb >> 10}KiB_x{S}"
        pitch = S * Cb + bench.PARITY_ROW_PAD
        old, new, par = filled(S * k * Cb, 12), filled(S * k * Cb, 13), filled(p * pitch, 14)
        result = ctx.alloc(32)
        T_auto = None if only else ecg.agg_threshold(k, p)
        row = {"auto_recalcs_from_n": None if only else T_auto + 1, "homog": {}}

        def update(m):
            return lambda: ctx.update_masks(k, p, Cb, S, old.ptr, new.ptr, k * Cb, par.ptr, pitch, Cb, m.ptr,
                                            result.ptr, 0)

        def agg(m, T):
            return lambda: ctx.agg_masks(k, p, Cb, S, old.ptr, new.ptr, k * Cb, par.ptr, pitch, Cb, m.ptr, result.ptr,
                                         T, 0)

        def encode():
            ctx.encode(k, p, Cb, S, new.ptr, k * Cb, par.ptr, pitch, Cb)

        delta_b = lambda n: (2 * n + 2 * p) * Cb * S      # noqa: E731
        enc_b = (k + p) * Cb * S
        for n in range(1, k + 1):
            m = masks_dev([(1 << n) - 1] * S)
            names = ("update_masks",) if only else ("update_masks", "agg_Tk", "agg_T0", "encode", "agg_auto")
            fns = [update(m)] if only else [update(m), agg(m, k), agg(m, 0), encode, agg(m, ecg.AGG_AUTO)]
            reps = [bench.time_interleaved(ctx, fns, ITERS, WARM) for _ in range(REPEATS)]
            ctx.sync()
            if not only:                # the last call counted: agg_auto
                assert words(result) == [S, U64MAX, n * S, 0], words(result)
                assert ecg.last_kernel() == "ecg_agg_masks_kernel<2>", ecg.last_kernel()
            um = [r[0] for r in reps]
            h = {"ms": {v: round(med(reps, i), 4) for i, v in enumerate(names)},
                 "ms_repeats": {v: [round(r[i], 4) for r in reps] for i, v in enumerate(names)},
                 "update_masks_spread": round(max(um) / min(um), 4),
                 "update_masks_hbm_frac": frac(med(reps, 0), delta_b(n))}
            if not only:
                h.update({"agg_Tk_over_update_masks": round(med(reps, 1) / med(reps, 0), 4),
                          "agg_T0_over_encode": round(med(reps, 2) / med(reps, 3), 4),
                          "agg_T0_hbm_frac": frac(med(reps, 2), enc_b),
                          "auto_route": "recalc" if n > T_auto else "delta",
                          "agg_auto_over_best": round(med(reps, 4) / min(med(reps, 1), med(reps, 2)), 4)})
            row["homog"][str(n)] = h
            print(name, f"n={n}", json.dumps(h), flush=True)
            m.free()
        if not only:
            faster = [row["homog"][str(n)]["ms"]["agg_T0"] < row["homog"][str(n)]["ms"]["agg_Tk"]
                      for n in range(1, k + 1)]
            row["crossover_measured"] = next((n for n in range(1, k + 1) if all(faster[n - 1:])), None)

            # ---- (2) mixed: n = 1 and n = k alternating
            mixed = [(1 << (s // 2 % k)) if s % 2 == 0 else (1 << k) - 1 for s in range(S)]
            ncell = sum(bin(x).count("1") for x in mixed)
            m = masks_dev(mixed)
            fns = [agg(m, ecg.AGG_AUTO), update(m), encode]
            reps = [bench.time_interleaved(ctx, fns, ITERS, WARM) for _ in range(REPEATS)]
            fns[0]()
            ctx.sync()
            assert words(result) == [S, U64MAX, ncell, 0], words(result)
            um = [r[1] for r in reps]
            auto_b = sum(enc_b // S if bin(x).count("1") > T_auto else (2 * bin(x).count("1") + 2 * p) * Cb
                         for x in mixed)
            mx = {"stripes": S, "cells": ncell,
                  "ms": {"agg_auto": round(med(reps, 0), 4), "update_masks": round(med(reps, 1), 4),
                         "encode": round(med(reps, 2), 4)},
                  "ms_repeats": {v: [round(r[i], 4) for r in reps]
                                 for i, v in enumerate(("agg_auto", "update_masks", "encode"))},
                  "update_masks_spread": round(max(um) / min(um), 4),
                  "update_masks_over_agg_auto": round(med(reps, 1) / med(reps, 0), 4),
                  "bytes_ratio_update_masks_over_agg_auto": round((2 * ncell + 2 * p * S) * Cb / auto_b, 4),
                  "agg_auto_hbm_frac": frac(med(reps, 0), auto_b)}
            row["mixed"] = mx
            print(name, "mixed", json.dumps(mx), flush=True)
            m.free()
        res["shapes"][name] = row
        for x in (old, new, par, result):
            x.free()
    out = os.path.join(ROOT, "build", "bench_agg_masks.json")
    if "--out" in sys.argv:
        out = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
