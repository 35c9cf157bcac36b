"""ecg_csum_updated and ecg_update_masks_csum (include/ecg_csum.h) against the routes they
replace.  Old and new data images [S][k][C] (the new one a copy of the old, so the update moves
its bytes and leaves every parity byte as it was: no variant needs a restore between calls), the
parity in the client layout [p][S][C], encoded on the device, its checksums [p][S][nch].  Per
hash type (crc32, crc64) at 32 KiB chunks:

  (a) updated_dense    ecg_csum_updated, every stripe's mask one changed cell (drawn per stripe)
      extents_all      ecg_csum_extents over the S*p parity cells, which lie contiguously: the
                       same bytes at the standalone kernel's own pace -- and today's route
                       after ecg_update_masks, whatever the masks
      updated_dense_sm the same call over a stripe-major copy [S][p][C] of the parity with
                       [S][p][nch] checksums: the items then walk memory in ecg_csum_extents'
                       own order, which tells the row pitch's share of any gap
  (b) updated_sparse   ecg_csum_updated, one stripe in 64 changed (one cell), against the same
                       extents_all; the bytes it checksums are 1/64 of that route's
      updated_clean    a batch of zero masks: what a stripe that is not selected costs
  (c) composite_dense, composite_sparse   ecg_update_masks_csum for the masks of (a) and (b)
      twostep_dense, twostep_sparse       ecg_update_masks, then ecg_csum_extents over all S*p
                                          parity cells: today's route
      (the sparse pair passes ECG_RM_SPARSE, the update half's tuning hint, to both routes)

Device events, one warm-up, median of 9 per variant per round; after one discarded pass the
variants alternate within each of ROUNDS rounds in one process; reported is the median of the
round medians and their spread.  After timing, one checked call per mask set and route: the
checksum array pre-filled with ecg_csum_extents' checksums of every parity cell, the selected
stripes' slots zeroed, one call, then ecg_csum_compare against the full array, on the device.
-> the JSON file given with --out PATH (default build/bench_update_masks_csum.json).
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
SHAPES = ((8, 2, 1 << 20, 512), (4, 2, 1 << 20, 1024), (16, 2, 128 << 10, 1024))
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
        us, nch = k * C, C // CHUNK
        old, new, par, par_sm = ctx.alloc(S * us), ctx.alloc(S * us), ctx.alloc(p * S * C), ctx.alloc(p * S * C)
        old.upload(blk[: min(blk.size, S * us)])
        for off in range(blk.size, S * us, blk.size):
            d2d(old.ptr + off, old.ptr, min(blk.size, S * us - off))
        d2d(new.ptr, old.ptr, S * us)
        ctx.encode(k, p, C, S, old.ptr, us, par.ptr, S * C, C)
        d2d(par_sm.ptr, par.ptr, p * S * C)       # the same bytes read as [S][p][C]: timing and its own check
        ctx.sync()

        rng = np.random.default_rng(1000 * k + p)
        m_dense = (1 << rng.integers(0, k, S)).astype(np.uint32)
        m_sparse = np.where(np.arange(S) % 64 == 0, m_dense, 0).astype(np.uint32)
        host = {"dense": m_dense, "sparse": m_sparse, "clean": np.zeros(S, dtype=np.uint32)}
        dev = {}
        for name, m in host.items():
            dev[name] = ctx.alloc(4 * S)
            dev[name].upload(m.view(np.uint8))
        rr, cmp_res = ctx.alloc(32), ctx.alloc(16)
        upd = (k, p, C, S, old.ptr, new.ptr, us, par.ptr, S * C, C)

        for hname, htype, cl in HASHES:
            full = p * S * nch * cl
            sums, ref = ctx.alloc(full), ctx.alloc(full)

            def cu(which):
                return lambda: ctx.csum_updated(htype, CHUNK, 1, k, p, C, S, par.ptr, S * C, C, dev[which].ptr,
                                                sums.ptr, nch, S * nch, rr.ptr)

            def cu_sm():
                ctx.csum_updated(htype, CHUNK, 1, k, p, C, S, par_sm.ptr, C, p * C, dev["dense"].ptr, sums.ptr, p * nch,
                                 nch, rr.ptr)

            def extents():
                ctx.csum_extents(htype, CHUNK, 1, 0, C, par.ptr, C, S * p, ref.ptr)

            def composite(which, flags):
                return lambda: ctx.update_masks_csum(*upd, dev[which].ptr, rr.ptr, htype, CHUNK, 1, sums.ptr, nch,
                                                     S * nch, flags)

            def twostep(which, flags):
                def fn():
                    ctx.update_masks(*upd, dev[which].ptr, rr.ptr, flags)
                    extents()
                return fn

            variants = {
                "updated_dense": cu("dense"),
                "extents_all": extents,
                "updated_dense_sm": cu_sm,
                "updated_sparse": cu("sparse"),
                "updated_clean": cu("clean"),
                "composite_dense": composite("dense", 0),
                "twostep_dense": twostep("dense", 0),
                "composite_sparse": composite("sparse", ecg.RM_SPARSE),
                "twostep_sparse": twostep("sparse", ecg.RM_SPARSE),
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

            # what the timed calls computed: sums pre-filled with the checksums of every parity
            # cell (ecg_csum_extents), the selected stripes' slots zeroed, one call, then equal again
            extents()
            for which, m in host.items():
                nsel = int(np.count_nonzero(m))
                for route in ("updated", "composite"):
                    d2d(sums.ptr, ref.ptr, full)
                    for s in np.flatnonzero(m):
                        for r in range(p):
                            ecg._chk(ecg.lib().ecg_memset(ctx.h, sums.ptr + (r * S + int(s)) * nch * cl, 0, nch * cl,
                                                          None), "memset")
                    if route == "updated":
                        cu(which)()
                        want = [nsel, U64MAX, nsel * p, 0]
                    else:
                        composite(which, 0)()
                        want = [nsel, U64MAX, nsel, 0]                  # one changed cell per stripe
                    ctx.csum_compare(htype, sums.ptr, ref.ptr, p * S * nch, cmp_res.ptr)
                    ctx.sync()
                    assert words(rr) == want, (which, route, words(rr))
                    assert words(cmp_res) == [0, U64MAX], (which, route, words(cmp_res))

            # the stripe-major variant: its slots are ecg_csum_extents' own order over that copy
            ecg._chk(ecg.lib().ecg_memset(ctx.h, sums.ptr, 0, full, None), "memset")
            cu_sm()
            ctx.csum_compare(htype, sums.ptr, ref.ptr, p * S * nch, cmp_res.ptr)
            ctx.sync()
            assert words(rr) == [S, U64MAX, S * p, 0] and words(cmp_res) == [0, U64MAX], (words(rr), words(cmp_res))

            row = {"bytes_checksummed_dense": S * p * C, "bytes_checksummed_sparse": int(np.count_nonzero(m_sparse)) * p * C}
            for v, ts in rounds.items():
                med = sorted(ts)[len(ts) // 2]
                row[v] = {"ms_rounds": [round(t, 4) for t in ts], "ms": round(med, 4),
                          "spread_ms": round(max(ts) - min(ts), 4), "last_kernel": kern[v]}
            ms = {v: row[v]["ms"] for v in variants}
            row["dense_vs_extents_all"] = round(ms["updated_dense"] / ms["extents_all"], 3)
            row["dense_sm_vs_extents_all"] = round(ms["updated_dense_sm"] / ms["extents_all"], 3)
            row["sparse_vs_extents_all"] = round(ms["updated_sparse"] / ms["extents_all"], 3)
            row["bytes_ratio_sparse"] = round(int(np.count_nonzero(m_sparse)) / S, 4)
            row["composite_vs_twostep_dense"] = round(ms["composite_dense"] / ms["twostep_dense"], 3)
            row["composite_vs_twostep_sparse"] = round(ms["composite_sparse"] / ms["twostep_sparse"], 3)
            row["updated_dense_GBps"] = round(S * p * C / ms["updated_dense"] / 1e6, 1)
            res["shapes"][name] = row
            print(name, json.dumps(row), flush=True)
            sums.free()
            ref.free()
        for x in [old, new, par, par_sm, rr, cmp_res] + list(dev.values()):
            x.free()
    out = os.path.join(ROOT, "build", "bench_update_masks_csum.json")
    if "--out" in sys.argv:
        out = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
