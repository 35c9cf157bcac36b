"""ecg_update_masks_ptrs (include/ecg.h) against the strided call and against the routes callers
with separately allocated stripes have today.  EC_8P2 and EC_16P2 at 128 KiB and 1 MiB cells, the
mixed batch of bench_update_masks.py: 1..4 random changed cells per stripe, one stripe in eight
clean.  The cells are three images (old [S][k][C], new [S][k][C], parity [p][S][C] at the padded
row pitch); the table lists the stripes in a random order, so it is not affine and the cell-table
kernel runs over the very bytes the strided call reads and writes.

  ptrs_permuted   ecg_update_masks_ptrs over the permuted table
  strided         ecg_update_masks over the same cells as three images: the reference row
  ptrs_affine     the table in stripe order: three strided groups, so the strided kernel must run
  gather          the route without the call and with the masks on the device only: every cell
                  copied into three scratch images (one ecg_dev_copy_kernel launch per image at the
                  box's copy rate: the gather at its best, and of ALL cells, since the host does
                  not know which changed), ecg_update_masks there, the parity copied back
  update_ptrs     ecg_update_ptrs over one request per changed cell, for a host that does know
                  them: host clock around call + sync (its sort, fold, colouring and staging
                  count), beside the same clock around the two mask calls

Device events around blocks of back-to-back launches, the variants interleaved (bench.py
time_interleaved), REPEATS repeats per row, ms = their median; table / strided is reported beside
the max/min spread of the strided row's repeats.  The result words are checked after the timed
calls.  -> the JSON file given with --out PATH (default build/bench_update_masks_ptrs.json).
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
COLUMN = 256 << 20              # bytes of one cell column of a batch
U64MAX = (1 << 64) - 1
NAMES = ("ptrs_permuted", "strided", "ptrs_affine", "gather")


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
        old, new, par = filled(S * k * Cb, 12), filled(S * k * Cb, 13), filled(p * pitch, 14)
        g_old, g_new, g_par = ctx.alloc(S * k * Cb), ctx.alloc(S * k * Cb), ctx.alloc(p * pitch)
        result = ctx.alloc(32)

        rng = np.random.default_rng(1000 * k + p)
        mixed = []
        for s in range(S):
            js = rng.choice(k, int(rng.integers(1, 5)), replace=False)
            mixed.append(0 if s % 8 == 7 else sum(1 << int(j) for j in js))
        ncell = sum(bin(x).count("1") for x in mixed)
        nwork = sum(1 for x in mixed if x)
        order = [int(s) for s in rng.permutation(S)]
        m, m_perm = masks_dev(mixed), masks_dev([mixed[s] for s in order])

        def row_of(s):
            return ([old.ptr + (s * k + j) * Cb for j in range(k)] + [new.ptr + (s * k + j) * Cb for j in range(k)] +
                    [par.ptr + r * pitch + s * Cb for r in range(p)])

        n = 2 * k + p
        t_perm = (C.c_void_p * (S * n))(*[a for s in order for a in row_of(s)])
        t_aff = (C.c_void_p * (S * n))(*[a for s in range(S) for a in row_of(s)])

        # one request per changed cell, the table built once
        reqs = [(j, s) for s, x in enumerate(mixed) for j in range(k) if x >> j & 1]
        tab = (C.c_void_p * (len(reqs) * (2 + p)))()
        vec = np.array([j for j, _ in reqs], dtype=np.uint8)
        for i, (j, s) in enumerate(reqs):
            tab[i * (2 + p)] = old.ptr + (s * k + j) * Cb
            tab[i * (2 + p) + 1] = new.ptr + (s * k + j) * Cb
            for r in range(p):
                tab[i * (2 + p) + 2 + r] = par.ptr + r * pitch + s * Cb
        vecp = vec.ctypes.data_as(C.POINTER(C.c_ubyte))

        def ptrs_permuted():
            ctx.update_masks_ptrs(k, p, Cb, S, t_perm, m_perm.ptr, result.ptr, 0)

        def strided():
            ctx.update_masks(k, p, Cb, S, old.ptr, new.ptr, k * Cb, par.ptr, pitch, Cb, m.ptr, result.ptr, 0)

        def ptrs_affine():
            ctx.update_masks_ptrs(k, p, Cb, S, t_aff, m.ptr, result.ptr, 0)

        def gather():
            ctx.copy_kernel(g_old.ptr, old.ptr, S * k * Cb)
            ctx.copy_kernel(g_new.ptr, new.ptr, S * k * Cb)
            ctx.copy_kernel(g_par.ptr, par.ptr, p * pitch)
            ctx.update_masks(k, p, Cb, S, g_old.ptr, g_new.ptr, k * Cb, g_par.ptr, pitch, Cb, m.ptr, result.ptr, 0)
            ctx.copy_kernel(par.ptr, g_par.ptr, p * pitch)

        def update_ptrs():
            ecg._chk(L.ecg_update_ptrs(ctx.h, k, p, Cb, len(reqs), tab, vecp, None), "update_ptrs")

        fns = [ptrs_permuted, strided, ptrs_affine, gather]
        kern = {}
        for v, fn in zip(NAMES, fns):
            fn()
            kern[v] = ecg.last_kernel()
            ctx.sync()
            assert words(result) == [nwork, U64MAX, ncell, 0], (v, words(result))
        assert kern["ptrs_permuted"] == f"ecg_update_masks_ptr_kernel<{p}>", kern
        assert kern["ptrs_affine"] == kern["strided"] == f"ecg_update_masks_kernel<{p}>", kern
        reps = [bench.time_interleaved(ctx, fns, ITERS, WARM) for _ in range(REPEATS)]
        hm = {v: host_ms(f) for v, f in (("ptrs_permuted", ptrs_permuted), ("strided", strided),
                                         ("update_ptrs", update_ptrs))}
        for fn in (strided, ptrs_permuted):     # what the timed calls computed: the result words
            fn()
            ctx.sync()
            assert words(result) == [nwork, U64MAX, ncell, 0], words(result)

        row = {"stripes": S, "stripes_with_work": nwork, "cells": ncell, "requests": len(reqs),
               "table_bytes": 8 * n * S, "kernels": kern}
        med = {}
        for i, v in enumerate(NAMES):
            ts = [r[i] for r in reps]
            med[v] = sorted(ts)[REPEATS // 2]
            row[v] = {"ms_repeats": [round(t, 4) for t in ts], "ms": round(med[v], 4),
                      "spread": round(max(ts) / min(ts), 4)}
        alg = (2 * ncell + 2 * p * nwork) * Cb
        for v in ("ptrs_permuted", "strided"):
            row[v]["hbm_frac"] = round(alg / med[v] / 1e6 / bench.HBM_PEAK_GBS, 4)
        row["ptrs_over_strided"] = {"median": round(med["ptrs_permuted"] / med["strided"], 4),
                                    "repeats": [round(r[0] / r[1], 4) for r in reps],
                                    "strided_spread": row["strided"]["spread"]}
        row["affine_over_strided"] = round(med["ptrs_affine"] / med["strided"], 4)
        row["gather_over_ptrs"] = round(med["gather"] / med["ptrs_permuted"], 4)
        row["host_ms"] = {v: round(t, 4) for v, t in hm.items()}
        row["update_ptrs_over_ptrs_host"] = round(hm["update_ptrs"] / hm["ptrs_permuted"], 3)
        row["update_ptrs_over_strided_host"] = round(hm["update_ptrs"] / hm["strided"], 3)
        res["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
        for x in (old, new, par, g_old, g_new, g_par, result, m, m_perm):
            x.free()
    out = os.path.join(ROOT, "build", "bench_update_masks_ptrs.json")
    if "--out" in sys.argv:
        out = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    print("self-check passed", flush=True)


if __name__ == "__main__":
    main()
