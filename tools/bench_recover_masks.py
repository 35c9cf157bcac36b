"""ecg_recover_masks (include/ecg.h) against the routes it replaces.  Stripes in
the recovery layout [S][k+p][C], encoded on the device; recovering a cell that
is already right moves the same bytes, so the batch stays a batch of codewords
and no variant needs a restore between calls.

  (a) dense           ecg_recover_masks, every stripe with p erasures, the sets
                      drawn at random over the batch (flags = 0: the dense grid)
      dense_gxN       the same with grid_x = N column blocks per stripe
      dense_rows2     the same with grid_y = S / 2: every block takes two
                      stripes in turn (half as many, twice as long blocks)
      dense_sparse    the same masks with ECG_RM_SPARSE (the 64-stripe scan
                      grid): what the flag is for
      recover_homog   one homogeneous ecg_recover(err_list = {0..p-1}) of the
                      same S: the reference pace; dense / recover_homog is the
                      cost of per-stripe tables and addresses
  (b) per_stripe      the route callers have today: the same mixed batch as one
                      ecg_recover(nstripes = 1) per stripe
  (c) pct1, pct1_sparse      1 % of the stripes masked (one cell each), without
                             and with ECG_RM_SPARSE
      clean, clean_sparse    a batch of zero masks: what every scrub pays

Device events, one warm-up, median of 9 per variant per round; after one
discarded pass the variants alternate within each of ROUNDS rounds in one
process, so each one's round-to-round spread is visible.
-> the JSON file given with --out PATH (default build/bench_recover_masks.json).
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
GRID_X = (64, 128)
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
    res = {"rounds": ROUNDS, "reps": REPS, "shapes": {}}
    for k, p, C, S in SHAPES:
        n, stride = k + p, (k + p) * C
        buf = ctx.alloc(S * stride)
        buf.upload(blk[: min(blk.size, S * stride)])
        for off in range(blk.size, S * stride, blk.size):
            d2d(buf.ptr + off, buf.ptr, min(blk.size, S * stride - off))
        ctx.encode(k, p, C, S, buf.ptr, stride, buf.ptr + k * C, C, stride)
        ctx.sync()

        rng = np.random.default_rng(1000 * k + p)
        sets = [sorted(int(c) for c in rng.choice(n, p, replace=False)) for _ in range(S)]
        m_dense = np.array([sum(1 << c for c in cs) for cs in sets], dtype=np.uint32)
        m_pct1 = np.zeros(S, dtype=np.uint32)
        for i, s in enumerate(range(0, S, 100)):
            m_pct1[s] = 1 << (i * 7 % n)
        dev = {}
        for name, m in (("dense", m_dense), ("pct1", m_pct1), ("clean", np.zeros(S, dtype=np.uint32))):
            dev[name] = ctx.alloc(4 * S)
            dev[name].upload(m.view(np.uint8))
        rr, rv, status = ctx.alloc(32), ctx.alloc(32), ctx.alloc(4 * S)
        geo = (k, p, C, S, buf.ptr, stride)

        def rm(which, flags=0, gx=0, gy=0):
            def fn():
                if gx or gy:
                    ctx.set_launch(gx, gy, 0)
                try:
                    ctx.recover_masks(*geo, dev[which].ptr, rr.ptr, flags)
                finally:
                    if gx or gy:
                        ctx.set_launch(0, 0, 0)
            return fn

        def per_stripe():
            for s, cs in enumerate(sets):
                ctx.recover(k, p, C, 1, buf.ptr + s * stride, stride, cs)

        name = f"EC_{k}P{p}_{C >> 10}KiB_x{S}"
        variants = {
            "dense": rm("dense"),
            "dense_sparse": rm("dense", ecg.RM_SPARSE),
            "recover_homog": lambda: ctx.recover(k, p, C, S, buf.ptr, stride, list(range(p))),
            "per_stripe": per_stripe,
            "pct1": rm("pct1"),
            "pct1_sparse": rm("pct1", ecg.RM_SPARSE),
            "clean": rm("clean"),
            "clean_sparse": rm("clean", ecg.RM_SPARSE),
        }
        for gx in GRID_X:
            variants[f"dense_gx{gx}"] = rm("dense", 0, gx)
        variants["dense_rows2"] = rm("dense", 0, 0, S // 2)
        rounds = {v: [] for v in variants}
        kern = {}
        for v, fn in variants.items():          # a discarded pass: code objects loaded, clocks up
            print(f"# {name}: warming {v}", flush=True)
            timed(fn)
        for _ in range(ROUNDS):
            for v, fn in variants.items():
                rounds[v].append(timed(fn))
                kern[v] = ecg.last_kernel()

        # what the timed calls computed: the erased cells overwritten, one call, the batch verifies clean
        for which, m in (("dense", m_dense), ("pct1", m_pct1)):
            for flags in (0, ecg.RM_SPARSE):
                for s in np.flatnonzero(m):
                    for c in range(n):
                        if int(m[s]) >> c & 1:
                            ecg._chk(ecg.lib().ecg_memset(ctx.h, buf.ptr + int(s) * stride + c * C, 0x5A, C, None),
                                     "memset")
                ctx.recover_masks(*geo, dev[which].ptr, rr.ptr, flags)
                ctx.verify(k, p, C, S, buf.ptr, stride, buf.ptr + k * C, C, stride, status.ptr, rv.ptr)
                ctx.sync()
                nz = int(np.count_nonzero(m))
                ncell = sum(bin(int(x)).count("1") for x in m)
                assert words(rr) == [nz, U64MAX, ncell, 0], (which, flags, words(rr))
                assert words(rv) == [0, U64MAX, 0, 0], (which, flags, words(rv))

        row = {"stripes_masked_pct1": int(np.count_nonzero(m_pct1)), "bytes_written_dense": S * p * C,
               "bytes_read_dense": S * k * C}
        for v, ts in rounds.items():
            med = sorted(ts)[len(ts) // 2]
            row[v] = {"ms_rounds": [round(t, 4) for t in ts], "ms": round(med, 4),
                      "spread_ms": round(max(ts) - min(ts), 4), "last_kernel": kern[v]}
        row["dense_vs_recover_homog"] = round(row["dense"]["ms"] / row["recover_homog"]["ms"], 3)
        row["dense_vs_per_stripe"] = round(row["dense"]["ms"] / row["per_stripe"]["ms"], 3)
        row["dense_GBps_read_plus_written"] = round(S * (k + p) * C / row["dense"]["ms"] / 1e6, 1)
        res["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
        for x in [buf, rr, rv, status] + list(dev.values()):
            x.free()
    out = os.path.join(ROOT, "build", "bench_recover_masks.json")
    if "--out" in sys.argv:
        out = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
