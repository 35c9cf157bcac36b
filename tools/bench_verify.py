"""ecg_verify (include/ecg.h) against its yardstick, the ecg_encode of the
same operands: verify moves exactly the bytes encode moves, all of them as
reads, so the same-run encode time is what it is measured against.

  verify        the whole call on clean stripes: status preset, syndrome
                kernel, summary kernel
  encode        ecg_encode of the same data into a second parity buffer
  verify_dirty  the same call with 1 % of the stripes carrying one wrong byte
                (the parity it reads is the clean parity with g[r][j] * e
                XORed into every row at one byte: byte for byte the syndrome
                of data cell j wrong by e), so the dirty path's cost shows
                where it is taken; the result words are checked
  read          the streaming read-only kernel over the data cells
                (ecg_dev_copy_kernel mode 1): the box's read ceiling, same
                process

Device events, one warm-up, median of 9 per variant per round; after one
discarded pass the variants alternate within each of ROUNDS rounds in one
process, so each one's round-to-round spread is visible.  verify_slower:
verify's fastest round is above encode's slowest by more than encode's own
spread.  Algorithmic bytes: (k + p) * C * S.
-> the JSON file given with --out PATH (default build/bench_verify.json).
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
READ_BLOCKS = 512


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

    blk = stripe_bytes(256 << 20, 12)
    res = {"rounds": ROUNDS, "reps": REPS, "shapes": {}}
    for k, p, C, S in SHAPES:
        alg = (k + p) * C * S
        data = ctx.alloc(S * k * C)
        for off in range(0, S * k * C, blk.size):
            data.upload(blk[: min(blk.size, S * k * C - off)], offset=off)
        pitch = S * C + 4096
        par, par_e, par_d = ctx.alloc(p * pitch), ctx.alloc(p * pitch), ctx.alloc(p * pitch)
        status, result, sink = ctx.alloc(4 * S), ctx.alloc(32), ctx.alloc(READ_BLOCKS * 256 * 16)
        ctx.encode(k, p, C, S, data.ptr, k * C, par.ptr, pitch, C)
        ctx.sync()
        ecg._chk(ecg.lib().ecg_memcpy(ctx.h, par_d.ptr, par.ptr, p * pitch, 2, None), "D2D")
        ctx.sync()
        g = ecg.cauchy1(k, p)[k:]
        bad = list(range(0, S, 100))        # 1 % of the stripes
        for s in bad:
            j, e, i = s % k, 0x5a, (s * 4099) % C
            for r in range(p):
                off = r * pitch + s * C + i
                v = par_d.download(1, off)
                par_d.upload(v ^ np.uint8(ecg.gf_mul(int(g[r][j]), e)), off)

        def verify(pp):
            ctx.verify(k, p, C, S, data.ptr, k * C, pp.ptr, pitch, C, status.ptr, result.ptr)

        def read():
            # bench.py's read ceiling: 512 persistent blocks.  The read kernel writes 16 bytes
            # per thread of the launch to its sink, and an uncapped launch has a block per 16 KiB
            # of source, so the cap also bounds what is written: READ_BLOCKS * 256 * 16 bytes.
            ctx.set_launch(READ_BLOCKS, 0, 0)
            try:
                ctx.copy_kernel(sink.ptr, data.ptr, S * k * C, 1)
            finally:
                ctx.set_launch(0, 0, 0)     # the verify launch follows the context's geometry too

        name = f"EC_{k}P{p}_{C >> 10}KiB_x{S}"
        variants = {"verify": lambda: verify(par),
                    "encode": lambda: ctx.encode(k, p, C, S, data.ptr, k * C, par_e.ptr, pitch, C),
                    "verify_dirty": lambda: verify(par_d),
                    "read": read}
        nbytes = {"verify": alg, "encode": alg, "verify_dirty": alg, "read": S * k * C}
        rounds = {n: [] for n in variants}
        kern = {}
        for n, fn in variants.items():      # a discarded pass: code objects loaded, clocks up
            print(f"# {name}: warming {n}", flush=True)
            timed(fn)
        for _ in range(ROUNDS):
            for n, fn in variants.items():
                rounds[n].append(timed(fn))
                kern[n] = ecg.last_kernel()
        # what the timed calls computed: clean is clean, every dirty stripe is located
        verify(par)
        ctx.sync()
        assert list(result.download().view(np.uint64)) == [0, (1 << 64) - 1, 0, 0], "clean stripes reported bad"
        verify(par_d)
        ctx.sync()
        got = [int(v) for v in result.download().view(np.uint64)]
        assert got == [len(bad), 0, len(bad), 0], got
        st = status.download().view(np.uint32)
        assert all(ecg.verify_cell(int(st[s]), k, p) == s % k for s in bad)

        row = {"alg_bytes": alg, "dirty_stripes": len(bad)}
        for n, ts in rounds.items():
            med = sorted(ts)[len(ts) // 2]
            row[n] = {"ms_rounds": [round(t, 4) for t in ts], "ms": round(med, 4),
                      "spread_ms": round(max(ts) - min(ts), 4), "TBps": round(nbytes[n] / med / 1e9, 3),
                      "last_kernel": kern[n]}
        v, e = rounds["verify"], rounds["encode"]
        row["verify_vs_encode"] = round(row["verify"]["ms"] / row["encode"]["ms"], 3)
        row["dirty_vs_clean"] = round(row["verify_dirty"]["ms"] / row["verify"]["ms"], 3)
        row["verify_slower"] = bool(min(v) > max(e) + (max(e) - min(e)))
        res["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
        for buf in (data, par, par_e, par_d, status, result, sink):
            buf.free()
    out = os.path.join(ROOT, "build", "bench_verify.json")
    if "--out" in sys.argv:
        out = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()


if __name__ == "__main__":
    main()
