"""ecg_csum_masked and ecg_recover_masks_csum (include/ecg_csum.h) against the routes they
replace.  Stripes in the recovery layout [S][k+p][C], encoded on the device; recovering a cell
that is already right moves the same bytes, so the batch stays a batch of codewords and no
variant needs a restore between calls.  Per hash type (crc32, crc64) at 32 KiB chunks:

  (a) erased          ecg_csum_masked(ECG_CM_ERASED), every stripe with p erasures, the sets
                      drawn at random over the batch
      extents_same    ecg_csum_extents over S*p cells laid contiguously: the same number of
                      cells at the standalone kernel's own pace
      extents_all     ecg_csum_extents over all S*(k+p) cells: today's route after
                      ecg_recover_masks
      both            ecg_csum_masked(ERASED | SURVIVORS) for the same masks
  (b) composite       ecg_recover_masks_csum on the homogeneous batch, every mask {0..p-1}
      composite_src   the same with src_csums == csums (one which = 3 launch)
      fused           ecg_recover_csum(err_list = {0..p-1}) of the same S: the fused product +
                      checksum kernel; composite / fused is the price of not fusing
      fused_src       ecg_recover_csum_all of the same S, beside composite_src
  (c) pct1, pct1_sparse      1 % of the stripes masked (one cell each), without and with
                             ECG_RM_SPARSE (accepted and ignored: the two must agree)
      clean, clean_sparse    a batch of zero masks
      rm_pct1_sparse, rm_clean_sparse   ecg_recover_masks of the same masks with the flag,
                                        beside them

Device events, one warm-up, median of 9 per variant per round; after one discarded pass the
variants alternate within each of ROUNDS rounds in one process; reported is the median of the
round medians and their spread.  After timing, one checked call per variant: the checksums of
the masked pass against ecg_csum_extents' for the same cells, on the device.
-> the JSON file given with --out PATH (default build/bench_csum_masked.json).
Bench infrastructure (no oracle)."""
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


def main():
    ctx = ecg.Context(0)
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
        ecg._chk(ecg.lib().ecg_memcpy(ctx.h, dst, src, n, 2, None), "D2D")

    def words(x, dtype=np.uint64):
        return [int(v) for v in x.download().view(dtype)]

    blk = stripe_bytes(256 << 20, 12)
    res = {"rounds": ROUNDS, "reps": REPS, "chunksize": CHUNK, "shapes": {}}
    for k, p, C, S in SHAPES:
        n, stride, nch = k + p, (k + p) * C, C // CHUNK
        buf = ctx.alloc(S * stride)
        buf.upload(blk[: min(blk.size, S * stride)])
        for off in range(blk.size, S * stride, blk.size):
            d2d(buf.ptr + off, buf.ptr, min(blk.size, S * stride - off))
        ctx.encode(k, p, C, S, buf.ptr, stride, buf.ptr + k * C, C, stride)
        ctx.sync()

        rng = np.random.default_rng(1000 * k + p)
        sets = [sorted(int(c) for c in rng.choice(n, p, replace=False)) for _ in range(S)]
        m_dense = np.array([sum(1 << c for c in cs) for cs in sets], dtype=np.uint32)
        m_homog = np.full(S, (1 << p) - 1, dtype=np.uint32)
        m_pct1 = np.zeros(S, dtype=np.uint32)
        for i, s in enumerate(range(0, S, 100)):
            m_pct1[s] = 1 << (i * 7 % n)
        host = {"dense": m_dense, "homog": m_homog, "pct1": m_pct1, "clean": np.zeros(S, dtype=np.uint32)}
        dev = {}
        for name, m in host.items():
            dev[name] = ctx.alloc(4 * S)
            dev[name].upload(m.view(np.uint8))
        rr, cmp_res = ctx.alloc(32), ctx.alloc(16)
        geo = (k, p, C, S, buf.ptr, stride)

        for hname, htype, cl in HASHES:
            full = S * n * nch * cl
            sums, ref, fsum, fsrc = ctx.alloc(full), ctx.alloc(full), ctx.alloc(p * S * nch * cl), ctx.alloc(
                k * S * nch * cl)

            def cm(which, sel, flags=0):
                return lambda: ctx.csum_masked(htype, CHUNK, 1, *geo, dev[which].ptr, sel, sums.ptr, rr.ptr, flags)

            def rm(which, flags):
                return lambda: ctx.recover_masks(*geo, dev[which].ptr, rr.ptr, flags)

            E, B = ecg.CM_ERASED, ecg.CM_ERASED | ecg.CM_SURVIVORS
            variants = {
                "erased": cm("dense", E),
                "extents_same": lambda: ctx.csum_extents(htype, CHUNK, 1, 0, C, buf.ptr, C, S * p, ref.ptr),
                "extents_all": lambda: ctx.csum_extents(htype, CHUNK, 1, 0, C, buf.ptr, C, S * n, ref.ptr),
                "both": cm("dense", B),
                "composite": lambda: ctx.recover_masks_csum(*geo, dev["homog"].ptr, rr.ptr, htype, CHUNK, 1,
                                                            sums.ptr),
                "composite_src": lambda: ctx.recover_masks_csum(*geo, dev["homog"].ptr, rr.ptr, htype, CHUNK, 1,
                                                                sums.ptr, sums.ptr),
                "fused": lambda: ctx.recover_csum(*geo, list(range(p)), htype, CHUNK, 1, fsum.ptr),
                "fused_src": lambda: ctx.recover_csum_all(*geo, list(range(p)), htype, CHUNK, 1, fsum.ptr,
                                                          fsrc.ptr),
                "pct1": cm("pct1", E),
                "pct1_sparse": cm("pct1", E, ecg.RM_SPARSE),
                "clean": cm("clean", E),
                "clean_sparse": cm("clean", E, ecg.RM_SPARSE),
                "rm_pct1_sparse": rm("pct1", ecg.RM_SPARSE),
                "rm_clean_sparse": rm("clean", ecg.RM_SPARSE),
            }
            name = f"EC_{k}P{p}_{C >> 10}KiB_x{S}_{hname}"
            rounds = {v: [] for v in variants}
            kern = {}
            for v, fn in variants.items():      # a discarded pass: code objects loaded, clocks up
                print(f"# {name}: warming {v}", flush=True)
                timed(fn)
            for _ in range(ROUNDS):
                for v, fn in variants.items():
                    rounds[v].append(timed(fn))
                    kern[v] = ecg.last_kernel()

            # what the timed calls computed: sums pre-filled with the checksums of every cell
            # (ecg_csum_extents), the selected slots zeroed, one call, then equal again
            ctx.csum_extents(htype, CHUNK, 1, 0, C, buf.ptr, C, S * n, ref.ptr)
            for which, sel, m in (("dense", E, m_dense), ("dense", B, m_dense), ("pct1", E, m_pct1),
                                  ("clean", E, host["clean"])):
                d2d(sums.ptr, ref.ptr, full)
                ncell = 0
                for s in np.flatnonzero(m):
                    cells = [c for c in range(n) if int(m[s]) >> c & 1]
                    if sel & ecg.CM_SURVIVORS:
                        cells += [c for c in range(n) if not int(m[s]) >> c & 1][:k]
                    ncell += len(cells)
                    for c in cells:
                        ecg._chk(ecg.lib().ecg_memset(ctx.h, sums.ptr + (int(s) * n + c) * nch * cl, 0, nch * cl,
                                                      None), "memset")
                for flags in (0, ecg.RM_SPARSE):
                    ctx.csum_masked(htype, CHUNK, 1, *geo, dev[which].ptr, sel, sums.ptr, rr.ptr, flags)
                    ctx.csum_compare(htype, sums.ptr, ref.ptr, S * n * nch, cmp_res.ptr)
                    ctx.sync()
                    assert words(rr) == [int(np.count_nonzero(m)), U64MAX, ncell, 0], (which, sel, words(rr))
                    assert words(cmp_res) == [0, U64MAX], (which, sel, words(cmp_res))
            for srcs in (None, sums.ptr):
                d2d(sums.ptr, ref.ptr, full)
                for s in range(S):
                    ecg._chk(ecg.lib().ecg_memset(ctx.h, sums.ptr + s * n * nch * cl, 0,
                                                  (n if srcs else p) * nch * cl, None), "memset")
                ctx.recover_masks_csum(*geo, dev["homog"].ptr, rr.ptr, htype, CHUNK, 1, sums.ptr, srcs)
                ctx.csum_compare(htype, sums.ptr, ref.ptr, S * n * nch, cmp_res.ptr)
                ctx.sync()
                assert words(rr) == [S, U64MAX, S * p, 0], words(rr)
                assert words(cmp_res) == [0, U64MAX], words(cmp_res)

            row = {"bytes_checksummed_erased": S * p * C, "bytes_checksummed_all": S * n * C}
            for v, ts in rounds.items():
                med = sorted(ts)[len(ts) // 2]
                row[v] = {"ms_rounds": [round(t, 4) for t in ts], "ms": round(med, 4),
                          "spread_ms": round(max(ts) - min(ts), 4), "last_kernel": kern[v]}
            ms = {v: row[v]["ms"] for v in variants}
            row["erased_vs_extents_same"] = round(ms["erased"] / ms["extents_same"], 3)
            row["erased_vs_extents_all"] = round(ms["erased"] / ms["extents_all"], 3)
            row["bytes_ratio_e_over_n"] = round(p / n, 3)
            row["composite_vs_fused"] = round(ms["composite"] / ms["fused"], 3)
            row["composite_src_vs_fused_src"] = round(ms["composite_src"] / ms["fused_src"], 3)
            row["erased_GBps"] = round(S * p * C / ms["erased"] / 1e6, 1)
            res["shapes"][name] = row
            print(name, json.dumps(row), flush=True)
            for x in (sums, ref, fsum, fsrc):
                x.free()
        for x in [buf, rr, cmp_res] + list(dev.values()):
            x.free()
    out = os.path.join(ROOT, "build", "bench_csum_masked.json")
    if "--out" in sys.argv:
        out = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
