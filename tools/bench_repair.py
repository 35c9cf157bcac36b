"""ecg_repair (include/ecg.h) against the routes it replaces.  Stripes in the
recovery layout [S][k+p][C] (the one ecg_recover works on), encoded on the
device; 1 % of the stripes get one wrong byte in one cell, the cells spread
over all k+p indices.

  (a) verify          ecg_verify of the clean batch
      repair_clean    ecg_repair of the clean batch (the status words of that
                      verify): what every scrub pays on top of the check
      repair_clean_4k the same call at a 4 KiB cell and the same S: does the
                      cost follow the block count or the bytes?
  (b) scrub_device    ecg_verify + ecg_repair of the dirty batch, two calls
                      queued on one stream
      scrub_host      the route without ecg_repair: ecg_verify, stream sync,
                      status download, ecg_verify_cell on the host, one
                      ecg_recover(nstripes = 1) per bad stripe
      (the wrong bytes are put back before every timed call, outside the
      timed span; device events around the calls, so the host round trip of
      scrub_host shows as the gap it leaves on the stream)
  (c) repair_only     the ecg_repair launch alone for the B bad stripes
                      (status words of the dirty batch; rewriting a cell that
                      is already right moves the same bytes)
      repair_only_gxN the same with grid_x = N column blocks per stripe
                      instead of the default cap (ecg_kabi.h
                      ECG_REPAIR_GRID_X)
      recover_B       one homogeneous ecg_recover(err_list = {0}) of B
                      stripes: the same bytes with full-width parallelism

Device events, one warm-up, median of 9 per variant per round; after one
discarded pass the variants alternate within each of ROUNDS rounds in one
process, so each one's round-to-round spread is visible.
-> the JSON file given with --out PATH (default build/bench_repair.json).
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
GRID_X = (16, 256)
U64MAX = (1 << 64) - 1


def main():
    ctx = ecg.Context(0)
    a, b = ctx.event(), ctx.event()

    def timed(fn, prep=None):
        if prep:
            prep()
        fn()
        ctx.sync()
        ts = []
        for _ in range(REPS):
            if prep:
                prep()
            ctx.record(a); fn(); ctx.record(b)
            ctx.sync()
            ts.append(ctx.elapsed_ms(a, b))
        ts.sort()
        return ts[len(ts) // 2]

    def d2d(dst, src, n):
        ecg._chk(ecg.lib().ecg_memcpy(ctx.h, dst, src, n, 2, None), "D2D")

    def batch(k, p, C, S, blk):
        """S encoded stripes [S][k+p][C] on the device."""
        n = S * (k + p) * C
        buf = ctx.alloc(n)
        buf.upload(blk[: min(blk.size, n)])
        for off in range(blk.size, n, blk.size):
            d2d(buf.ptr + off, buf.ptr, min(blk.size, n - off))
        ctx.encode(k, p, C, S, buf.ptr, (k + p) * C, buf.ptr + k * C, C, (k + p) * C)
        ctx.sync()
        return buf

    blk = stripe_bytes(256 << 20, 12)
    res = {"rounds": ROUNDS, "reps": REPS, "grid_x_default": 64, "shapes": {}}
    for k, p, C, S in SHAPES:
        n, stride = k + p, (k + p) * C
        buf, small = batch(k, p, C, S, blk), batch(k, p, 4096, S, blk)
        bad = list(range(0, S, 100))            # 1 % of the stripes
        B = len(bad)
        cell_of = {s: i * 7 % n for i, s in enumerate(bad)}     # data and parity cells alike
        few = ctx.alloc(B * stride)
        d2d(few.ptr, buf.ptr + stride, B * stride)      # B clean stripes of their own
        status, st_clean, st_small = ctx.alloc(4 * S), ctx.alloc(4 * S), ctx.alloc(4 * S)
        rv, rr = ctx.alloc(32), ctx.alloc(32)
        geo, ops = (k, p, C, S), (buf.ptr, stride, buf.ptr + k * C, C, stride)
        geo4, ops4 = (k, p, 4096, S), (small.ptr, n * 4096, small.ptr + k * 4096, 4096, n * 4096)
        ctx.verify(*geo, *ops, st_clean.ptr, rv.ptr)
        ctx.verify(*geo4, *ops4, st_small.ptr, rv.ptr)
        ctx.sync()

        where = {s: s * stride + c * C + (s * 4099) % C for s, c in cell_of.items()}
        good = {s: buf.download(1, off) for s, off in where.items()}

        def dirty():
            for s, off in where.items():
                buf.upload(good[s] ^ np.uint8(0x5a), off)

        def words(x, dtype=np.uint64):
            return [int(v) for v in x.download().view(dtype)]

        def scrub_device():
            ctx.verify(*geo, *ops, status.ptr, rv.ptr)
            ctx.repair(*geo, *ops, status.ptr, rr.ptr)

        def scrub_host():
            ctx.verify(*geo, *ops, status.ptr, rv.ptr)
            ctx.sync()
            for s, w in enumerate(status.download().view(np.uint32)):
                c = ecg.verify_cell(int(w), k, p) if w & 0xff else -1
                if c >= 0:
                    ctx.recover(k, p, C, 1, buf.ptr + s * stride, stride, [c])

        def repair_gx(gx):
            def fn():
                ctx.set_launch(gx, 0, 0)
                try:
                    ctx.repair(*geo, *ops, status.ptr, rr.ptr)
                finally:
                    ctx.set_launch(0, 0, 0)
            return fn

        # the status words of the dirty batch, for (c)
        dirty()
        ctx.verify(*geo, *ops, status.ptr, rv.ptr)
        ctx.sync()
        assert words(rv) == [B, 0, B, 0], words(rv)
        st_dirty = status.download()
        ctx.repair(*geo, *ops, status.ptr, rr.ptr)      # the batch is clean again
        ctx.sync()

        name = f"EC_{k}P{p}_{C >> 10}KiB_x{S}"
        variants = {
            "verify": (lambda: ctx.verify(*geo, *ops, status.ptr, rv.ptr), None),
            "repair_clean": (lambda: ctx.repair(*geo, *ops, st_clean.ptr, rr.ptr), None),
            "repair_clean_4k": (lambda: ctx.repair(*geo4, *ops4, st_small.ptr, rr.ptr), None),
            "scrub_device": (scrub_device, dirty),
            "scrub_host": (scrub_host, dirty),
            "repair_only": (lambda: ctx.repair(*geo, *ops, status.ptr, rr.ptr), lambda: status.upload(st_dirty)),
            "recover_B": (lambda: ctx.recover(k, p, C, B, few.ptr, stride, [0]), None),
        }
        for gx in GRID_X:
            variants[f"repair_only_gx{gx}"] = (repair_gx(gx), lambda: status.upload(st_dirty))
        rounds = {v: [] for v in variants}
        kern = {}
        for v, (fn, prep) in variants.items():  # a discarded pass: code objects loaded, clocks up
            print(f"# {name}: warming {v}", flush=True)
            timed(fn, prep)
        for _ in range(ROUNDS):
            for v, (fn, prep) in variants.items():
                rounds[v].append(timed(fn, prep))
                kern[v] = ecg.last_kernel()

        # what the timed calls computed
        ctx.repair(*geo, *ops, st_clean.ptr, rr.ptr)
        ctx.sync()
        assert words(rr) == [0, U64MAX, 0, 0], "clean stripes repaired"
        ndata = sum(1 for c in cell_of.values() if c < k)
        for route in (scrub_device, scrub_host):
            dirty()
            route()
            ctx.sync()
            if route is scrub_device:
                assert words(rr) == [B, U64MAX, ndata, 0], words(rr)
            ctx.verify(*geo, *ops, status.ptr, rv.ptr)
            ctx.sync()
            assert words(rv) == [0, U64MAX, 0, 0], (route.__name__, words(rv))

        row = {"bad_stripes": B, "bytes_rewritten": B * C, "bytes_read_by_repair": B * k * C}
        for v, ts in rounds.items():
            med = sorted(ts)[len(ts) // 2]
            row[v] = {"ms_rounds": [round(t, 4) for t in ts], "ms": round(med, 4),
                      "spread_ms": round(max(ts) - min(ts), 4), "last_kernel": kern[v]}
        row["scrub_device_vs_host"] = round(row["scrub_device"]["ms"] / row["scrub_host"]["ms"], 3)
        row["repair_only_vs_recover_B"] = round(row["repair_only"]["ms"] / row["recover_B"]["ms"], 3)
        row["repair_clean_vs_verify_spread"] = round(row["repair_clean"]["ms"] / max(row["verify"]["spread_ms"], 1e-4), 2)
        res["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
        for x in (buf, small, few, status, st_clean, st_small, rv, rr):
            x.free()
    out = os.path.join(ROOT, "build", "bench_repair.json")
    if "--out" in sys.argv:
        out = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
