"""ecg_csum_masked_ptrs, ecg_csum_cells_ptrs and ecg_recover_masks_ptrs_csum (include/ecg_csum.h)
against the strided calls over the same bytes and against the route they replace.  Stripes in the
recovery layout [S][k+p][C], encoded on the device; the table lists the same memory with the
stripes in a random order, so it is not affine and the cell-table kernels run.  Recovering a cell
that is already right moves the same bytes, so the batch stays a batch of codewords and no variant
needs a restore between calls.  Every stripe has p erasures, the sets drawn at random over the
batch.  Per hash type (crc32, crc64) at 32 KiB chunks:

  (a)  ptrs              ecg_csum_masked_ptrs(ECG_CM_ERASED) on the permuted table
  (b)  strided           ecg_csum_masked(ECG_CM_ERASED) over the same bytes as one image: the
                         reference pace
  (b') strided_again     the same call a second time in every round: b'/b is the A/A noise that
                         a/b has to be read against
  (c)  composite_ptrs    ecg_recover_masks_ptrs_csum on the permuted table
       gather_composite_scatter   what it replaces: ecg_dev_copy_kernel of the whole batch into a
                         scratch image, ecg_recover_masks_csum there, ecg_dev_copy_kernel back.
                         One copy launch each way at the box's copy rate is the gather at its
                         best: S separate buffers would take S launches or a segment table.
       composite_strided ecg_recover_masks_csum on the image itself, beside them
       ptrs_clean, strided_clean   (a) and (b) on a batch of zero masks: no cell is read, so
                         their difference is what the table itself costs a call (its upload,
                         a launch that reads 8*(k+p)*S bytes of pinned host memory, in front of
                         the checksum kernel), to be read beside a - b
       cells_ptrs        ecg_csum_cells_ptrs over all S*(k+p) cells of the table
       extents_all       ecg_csum_extents over the same cells as one image

Device events, one warm-up, median of 9 per variant per round; after one discarded pass the
variants alternate within each of ROUNDS rounds in one process, on one context; reported is the
median of the round medians and their spread.  After timing, checked calls: the checksums of the
table calls against ecg_csum_extents' for the same cells, compared on the device, the result
words, and ecg_verify clean after the composite has regenerated overwritten cells.
-> the JSON file given with --out PATH (default build/bench_csum_masked_ptrs.json).
Bench infrastructure (no oracle)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from daos_amd import ecg  # noqa: E402
from tools.datagen import stripe_bytes  # noqa: E402

ROUNDS, REPS = 3, 9
SHAPES = ((8, 2, 1 << 20, 512), (4, 2, 1 << 20, 1024), (16, 2, 128 << 10, 1024), (8, 3, 1 << 20, 512))
HASHES = (("crc32", ecg.HASH_CRC32, 4), ("crc64", ecg.HASH_CRC64, 8))
CHUNK = 32 << 10
U64MAX = (1 << 64) - 1
RATIOS = (("ptrs", "strided"), ("strided_again", "strided"), ("gather_composite_scatter", "composite_ptrs"),
          ("composite_ptrs", "composite_strided"), ("cells_ptrs", "extents_all"))


def main():
    ctx = ecg.Context(0)
    L = ecg.lib()
    a, b = ctx.event(), ctx.event()

    def timed(fn):
        fn()
        ctx.sync()
        ts = []
        for _ in range(REPS):
            ctx.record(a); fn(); ctx.record(b)
            ctx.sync()
            ts.append(ctx.elapsed_ms(a, b))
        ts.sort()
        return ts[len(ts) // 2]

    def d2d(dst, src, n):
        ecg._chk(L.ecg_memcpy(ctx.h, dst, src, n, 2, None), "D2D")

    def words(x, dtype=np.uint64):
        return [int(v) for v in x.download().view(dtype)]

    blk = stripe_bytes(256 << 20, 12)
    res = {"rounds": ROUNDS, "reps": REPS, "chunksize": CHUNK, "shapes": {}}
    for k, p, C_, S in SHAPES:
        n, stride, nch = k + p, (k + p) * C_, C_ // CHUNK
        buf, scratch = ctx.alloc(S * stride), ctx.alloc(S * stride)
        buf.upload(blk[: min(blk.size, S * stride)])
        for off in range(blk.size, S * stride, blk.size):
            d2d(buf.ptr + off, buf.ptr, min(blk.size, S * stride - off))
        ctx.encode(k, p, C_, S, buf.ptr, stride, buf.ptr + k * C_, C_, stride)
        ctx.sync()

        rng = np.random.default_rng(1000 * k + p)
        sets = [sorted(int(c) for c in rng.choice(n, p, replace=False)) for _ in range(S)]
        m_dense = np.array([sum(1 << c for c in cs) for cs in sets], dtype=np.uint32)
        order = [int(s) for s in rng.permutation(S)]
        dev = {}
        for name, m in (("dense", m_dense), ("dense_perm", m_dense[order]), ("clean", np.zeros(S, dtype=np.uint32))):
            dev[name] = ctx.alloc(4 * S)
            dev[name].upload(m.view(np.uint8))
        rr, rv, cmp_res, status = ctx.alloc(32), ctx.alloc(32), ctx.alloc(16), ctx.alloc(4 * S)
        tab = [buf.ptr + s * stride + c * C_ for s in order for c in range(n)]
        t_perm = (C.c_void_p * len(tab))(*tab)
        geo = (k, p, C_, S, buf.ptr, stride)

        for hname, htype, cl in HASHES:
            row_bytes, full = n * nch * cl, S * n * nch * cl
            sums, ref, ref_perm = ctx.alloc(full), ctx.alloc(full), ctx.alloc(full)
            E = ecg.CM_ERASED

            def strided():
                ctx.csum_masked(htype, CHUNK, 1, *geo, dev["dense"].ptr, E, sums.ptr, rr.ptr)

            def gather_composite_scatter():
                ctx.copy_kernel(scratch.ptr, buf.ptr, S * stride)
                ctx.recover_masks_csum(k, p, C_, S, scratch.ptr, stride, dev["dense"].ptr, rr.ptr, htype, CHUNK, 1,
                                       sums.ptr)
                ctx.copy_kernel(buf.ptr, scratch.ptr, S * stride)

            variants = {
                "ptrs": lambda: ctx.csum_masked_ptrs(htype, CHUNK, 1, k, p, C_, S, t_perm, dev["dense_perm"].ptr, E,
                                                     sums.ptr, rr.ptr),
                "strided": strided,
                "strided_again": strided,
                "composite_ptrs": lambda: ctx.recover_masks_ptrs_csum(k, p, C_, S, t_perm, dev["dense_perm"].ptr,
                                                                      rr.ptr, htype, CHUNK, 1, sums.ptr),
                "gather_composite_scatter": gather_composite_scatter,
                "composite_strided": lambda: ctx.recover_masks_csum(*geo, dev["dense"].ptr, rr.ptr, htype, CHUNK, 1,
                                                                    sums.ptr),
                "ptrs_clean": lambda: ctx.csum_masked_ptrs(htype, CHUNK, 1, k, p, C_, S, t_perm, dev["clean"].ptr, E,
                                                           sums.ptr, rr.ptr),
                "strided_clean": lambda: ctx.csum_masked(htype, CHUNK, 1, *geo, dev["clean"].ptr, E, sums.ptr,
                                                         rr.ptr),
                "cells_ptrs": lambda: ctx.csum_cells_ptrs(htype, CHUNK, 1, C_, t_perm, sums.ptr),
                "extents_all": lambda: ctx.csum_extents(htype, CHUNK, 1, 0, C_, buf.ptr, C_, S * n, ref.ptr),
            }
            name = f"EC_{k}P{p}_{C_ >> 10}KiB_x{S}_{hname}"
            rounds = {v: [] for v in variants}
            kern = {}
            for v, fn in variants.items():      # a discarded pass: code objects loaded, clocks up
                print(f"# {name}: warming {v}", flush=True)
                timed(fn)
            for _ in range(ROUNDS):
                for v, fn in variants.items():
                    rounds[v].append(timed(fn))
                    kern[v] = ecg.last_kernel()
            assert "masked_ptr_kernel" in kern["ptrs"] and "masked_ptr_kernel" in kern["composite_ptrs"], kern
            assert "cells_ptr_kernel" in kern["cells_ptrs"] and "bytes" not in kern["ptrs"], kern

            # what the timed calls computed.  ref_perm: ecg_csum_extents' checksums of every cell, the
            # stripes' rows in table order
            ctx.csum_extents(htype, CHUNK, 1, 0, C_, buf.ptr, C_, S * n, ref.ptr)
            for r, s in enumerate(order):
                d2d(ref_perm.ptr + r * row_bytes, ref.ptr + s * row_bytes, row_bytes)
            ctx.csum_cells_ptrs(htype, CHUNK, 1, C_, t_perm, sums.ptr)
            ctx.csum_compare(htype, sums.ptr, ref_perm.ptr, S * n * nch, cmp_res.ptr)
            ctx.sync()
            assert words(cmp_res) == [0, U64MAX], ("cells_ptrs", words(cmp_res))
            for composite in (False, True):
                # sums = the reference with the erased cells' slots zeroed; the call fills them in again
                d2d(sums.ptr, ref_perm.ptr, full)
                for r, s in enumerate(order):
                    for c in sets[s]:
                        ecg._chk(L.ecg_memset(ctx.h, sums.ptr + (r * n + c) * nch * cl, 0, nch * cl, None), "memset")
                        if composite:           # and the cells themselves overwritten
                            ecg._chk(L.ecg_memset(ctx.h, buf.ptr + s * stride + c * C_, 0x5A, C_, None), "memset")
                if composite:
                    ctx.recover_masks_ptrs_csum(k, p, C_, S, t_perm, dev["dense_perm"].ptr, rr.ptr, htype, CHUNK, 1,
                                                sums.ptr)
                    ctx.verify(k, p, C_, S, buf.ptr, stride, buf.ptr + k * C_, C_, stride, status.ptr, rv.ptr)
                else:
                    ctx.csum_masked_ptrs(htype, CHUNK, 1, k, p, C_, S, t_perm, dev["dense_perm"].ptr, E, sums.ptr,
                                         rr.ptr)
                ctx.csum_compare(htype, sums.ptr, ref_perm.ptr, S * n * nch, cmp_res.ptr)
                ctx.sync()
                assert words(rr) == [S, U64MAX, S * p, 0], (composite, words(rr))
                assert words(cmp_res) == [0, U64MAX], (composite, words(cmp_res))
                if composite:
                    assert words(rv) == [0, U64MAX, 0, 0], words(rv)

            row = {"bytes_checksummed_erased": S * p * C_, "bytes_checksummed_all": S * n * C_,
                   "table_bytes": 8 * n * S, "bytes_copied_gather_plus_scatter": 2 * S * stride}
            for v, ts in rounds.items():
                med = sorted(ts)[len(ts) // 2]
                row[v] = {"ms_rounds": [round(t, 4) for t in ts], "ms": round(med, 4),
                          "spread_ms": round(max(ts) - min(ts), 4), "last_kernel": kern[v]}
            for num, den in RATIOS:
                row[f"{num}_vs_{den}"] = {"median": round(row[num]["ms"] / row[den]["ms"], 3),
                                          "rounds": [round(x / y, 3) for x, y in zip(rounds[num], rounds[den])]}
            row["ptrs_minus_strided_us"] = round(1e3 * (row["ptrs"]["ms"] - row["strided"]["ms"]), 1)
            row["ptrs_clean_minus_strided_clean_us"] = round(
                1e3 * (row["ptrs_clean"]["ms"] - row["strided_clean"]["ms"]), 1)
            aa = [abs(x - 1) for x in row["strided_again_vs_strided"]["rounds"]]
            row["ptrs_vs_strided"]["within_aa_noise"] = abs(row["ptrs_vs_strided"]["median"] - 1) <= max(aa)
            res["shapes"][name] = row
            print(name, json.dumps(row), flush=True)
            for x in (sums, ref, ref_perm):
                x.free()
        for x in [buf, scratch, rr, rv, cmp_res, status] + list(dev.values()):
            x.free()
    out = os.path.join(ROOT, "build", "bench_csum_masked_ptrs.json")
    if "--out" in sys.argv:
        out = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    print("self-check passed", flush=True)


if __name__ == "__main__":
    main()
