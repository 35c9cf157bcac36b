"""ecg_verify_ptrs / ecg_scrub_ptrs (include/ecg.h) against the strided calls and against the
route callers with scattered cells have today.  Stripes encoded on the device, so every batch is
a batch of codewords; the table lists the stripes of the image in a random order, so it is not
affine and the cell-table kernels run over the very bytes the strided calls read.

  verify, clean batch:
  (a)  verify_ptrs       ecg_verify_ptrs on the permuted table
  (b)  verify            ecg_verify over the same cells as one strided image: the reference pace
  (b') verify_again      the same call a second time in every round: b'/b is the A/A noise that a/b
                         has to be read against
  (c)  gather_verify     today's route for scattered cells: the whole batch copied into a scratch
                         image (ecg_dev_copy_kernel, one launch at the box's copy rate: the gather at
                         its best), then ecg_verify there
  scrub, 1 % of the stripes bad (16 bytes of one cell overwritten before every timed call,
  outside the timed region; the scrub puts them right again):
       scrub_ptrs        ecg_scrub_ptrs on the permuted table
       verify_repair     ecg_verify + ecg_repair on the image
       gather_scrub      copy into the scratch image, ecg_verify + ecg_repair there, copy back
  host time of a call (clean batch, the stream drained before each, perf_counter around the
  call alone): pair_host_us = one ecg_verify_ptrs + one ecg_repair_ptrs, scrub_host_us = one
  ecg_scrub_ptrs -- the second table pass and upload saved.

Device events, one warm-up, median of 9 per variant per round; after one discarded pass the
variants alternate within each of ROUNDS rounds in one process.  The self-check at the end breaks
the 1 % again, runs one ecg_scrub_ptrs and expects its result words and a clean second check.
-> the JSON file given with --out PATH (default build/bench_verify_ptrs.json).
Bench infrastructure (no oracle)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from daos_amd import ecg  # noqa: E402
from tools.datagen import stripe_bytes  # noqa: E402

ROUNDS, REPS, HOST_REPS = 3, 9, 41
SHAPES = ((4, 2, 128 << 10, 2048), (4, 2, 1 << 20, 512), (8, 2, 128 << 10, 2048), (8, 2, 1 << 20, 256),
          (16, 2, 128 << 10, 1024), (16, 2, 1 << 20, 128))
U64MAX = (1 << 64) - 1
RATIOS = (("verify_ptrs", "verify"), ("verify_again", "verify"), ("gather_verify", "verify_ptrs"),
          ("scrub_ptrs", "verify_repair"), ("gather_scrub", "scrub_ptrs"))


def main():
    ctx = ecg.Context(0)
    L = ecg.lib()
    a, b = ctx.event(), ctx.event()

    def timed(fn, prep=None):
        ts = []
        for i in range(REPS + 1):               # the first one a warm-up
            if prep:
                prep()
            ctx.record(a); fn(); ctx.record(b)
            ctx.sync()
            if i:
                ts.append(ctx.elapsed_ms(a, b))
        ts.sort()
        return ts[len(ts) // 2]

    def host_us(fn):
        ts = []
        for _ in range(HOST_REPS):
            ctx.sync()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e6)
        ctx.sync()
        ts.sort()
        return ts[len(ts) // 2]

    def d2d(dst, src, n):
        ecg._chk(L.ecg_memcpy(ctx.h, dst, src, n, 2, None), "D2D")

    def words(x):
        return [int(v) for v in x.download().view(np.uint64)]

    blk = stripe_bytes(256 << 20, 12)
    res = {"rounds": ROUNDS, "reps": REPS, "host_reps": HOST_REPS, "shapes": {}}
    for k, p, C_, S in SHAPES:
        n, stride = k + p, (k + p) * C_
        buf, scratch = ctx.alloc(S * stride), ctx.alloc(S * stride)
        buf.upload(blk[: min(blk.size, S * stride)])
        for off in range(blk.size, S * stride, blk.size):
            d2d(buf.ptr + off, buf.ptr, min(blk.size, S * stride - off))
        ctx.encode(k, p, C_, S, buf.ptr, stride, buf.ptr + k * C_, C_, stride)
        ctx.sync()
        rng = np.random.default_rng(1000 * k + p)
        order = [int(s) for s in rng.permutation(S)]
        tab = (C.c_void_p * (S * n))(*[buf.ptr + s * stride + c * C_ for s in order for c in range(n)])
        bad = {s: (i * 7) % n for i, s in enumerate(range(0, S, 100))}      # stripe -> its wrong cell
        status, rv, rr = ctx.alloc(4 * S), ctx.alloc(32), ctx.alloc(32)
        geo = (k, p, C_, S)
        img = (buf.ptr, stride, buf.ptr + k * C_, C_, stride)
        scr = (scratch.ptr, stride, scratch.ptr + k * C_, C_, stride)

        def corrupt():
            for s, c in bad.items():
                ecg._chk(L.ecg_memset(ctx.h, buf.ptr + s * stride + c * C_ + 4096, 0x5A, 16, None), "memset")

        def verify_repair(at=img):
            ctx.verify(*geo, *at, status.ptr, rv.ptr)
            ctx.repair(*geo, *at, status.ptr, rr.ptr)

        def gather_verify():
            ctx.copy_kernel(scratch.ptr, buf.ptr, S * stride)
            ctx.verify(*geo, *scr, status.ptr, rv.ptr)

        def gather_scrub():
            ctx.copy_kernel(scratch.ptr, buf.ptr, S * stride)
            verify_repair(scr)
            ctx.copy_kernel(buf.ptr, scratch.ptr, S * stride)

        def pair_ptrs():
            ctx.verify_ptrs(*geo, tab, status.ptr, rv.ptr)
            ctx.repair_ptrs(*geo, tab, status.ptr, rr.ptr)

        def verify():
            ctx.verify(*geo, *img, status.ptr, rv.ptr)

        name = f"EC_{k}P{p}_{C_ >> 10}KiB_x{S}"
        variants = {
            "verify_ptrs": (lambda: ctx.verify_ptrs(*geo, tab, status.ptr, rv.ptr), None),
            "verify": (verify, None),
            "verify_again": (verify, None),
            "gather_verify": (gather_verify, None),
            "scrub_ptrs": (lambda: ctx.scrub_ptrs(*geo, tab, status.ptr, rv.ptr, rr.ptr), corrupt),
            "verify_repair": (verify_repair, corrupt),
            "gather_scrub": (gather_scrub, corrupt),
        }
        rounds = {v: [] for v in variants}
        kern = {}
        for v, (fn, prep) in variants.items():  # a discarded pass: code objects loaded, clocks up
            print(f"# {name}: warming {v}", flush=True)
            timed(fn, prep)
        for _ in range(ROUNDS):
            for v, (fn, prep) in variants.items():
                rounds[v].append(timed(fn, prep))
                kern[v] = ecg.last_kernel()
        assert kern["verify_ptrs"].startswith("ecg_verify_ptr_kernel<"), kern
        assert kern["scrub_ptrs"].startswith("ecg_repair_ptr_kernel<"), kern
        assert words(rv) == [len(bad), 0, len(bad), 0] and words(rr)[0] == len(bad), (words(rv), words(rr))
        host = {"pair_host_us": [], "scrub_host_us": []}
        for _ in range(ROUNDS):
            host["pair_host_us"].append(host_us(pair_ptrs))
            host["scrub_host_us"].append(host_us(lambda: ctx.scrub_ptrs(*geo, tab, status.ptr, rv.ptr, rr.ptr)))

        # what the timed calls computed: the 1 % broken once more, one scrub, a clean second check
        corrupt()
        ctx.scrub_ptrs(*geo, tab, status.ptr, rv.ptr, rr.ptr)
        ctx.sync()
        where = sorted(order.index(s) for s in bad)
        assert words(rv) == [len(bad), where[0], len(bad), 0], words(rv)
        assert words(rr) == [len(bad), U64MAX, sum(1 for c in bad.values() if c < k), 0], words(rr)
        ctx.verify(*geo, *img, status.ptr, rv.ptr)
        ctx.sync()
        assert words(rv) == [0, U64MAX, 0, 0], words(rv)

        row = {"bad_stripes": len(bad), "table_bytes": 8 * n * S, "bytes_read_by_verify": S * stride}
        for v, ts in rounds.items():
            med = sorted(ts)[len(ts) // 2]
            row[v] = {"ms_rounds": [round(t, 4) for t in ts], "ms": round(med, 4),
                      "spread_ms": round(max(ts) - min(ts), 4), "last_kernel": kern[v]}
        for num, den in RATIOS:
            row[f"{num}_vs_{den}"] = {"median": round(row[num]["ms"] / row[den]["ms"], 3),
                                      "rounds": [round(x / y, 3) for x, y in zip(rounds[num], rounds[den])]}
        row["verify_ptrs_vs_verify"]["within_verify_spread"] = \
            abs(row["verify_ptrs"]["ms"] - row["verify"]["ms"]) <= row["verify"]["spread_ms"]
        for h, ts in host.items():
            row[h] = {"rounds": [round(t, 1) for t in ts], "median": round(sorted(ts)[len(ts) // 2], 1)}
        row["verify_ptrs_GBps_read"] = round(S * stride / row["verify_ptrs"]["ms"] / 1e6, 1)
        row["verify_GBps_read"] = round(S * stride / row["verify"]["ms"] / 1e6, 1)
        res["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
        for x in (buf, scratch, status, rv, rr):
            x.free()
    out = os.path.join(ROOT, "build", "bench_verify_ptrs.json")
    if "--out" in sys.argv:
        out = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    print("self-check passed", flush=True)


if __name__ == "__main__":
    main()
