"""ecg_matmul_ptrs_lens / ecg_obj_ec_singv_encode_dev (include/ecg.h, ecg_daos.h) against what
callers whose stripes do not share a cell size had before: one ecg_matmul_ptrs per distinct size.

  (a) singv   4096 EC_8P2 single values in device memory, sizes log-uniform from 8 KiB to 1 MiB
      singv_dev       one ecg_obj_ec_singv_encode_dev call
      per_size_ptrs   one ecg_matmul_ptrs call per distinct cell size over the same value buffers
                      (tables built and the values' padded last cells staged outside the timed
                      region, which the new call does inside it)
  (b) lens    512 EC_8P2 stripes of 1 MiB cells through a shuffled (not affine) table
      uniform         ecg_matmul_ptrs: ecg_mm_ptr_kernel
      one_short       ecg_matmul_ptrs_lens with one stripe 16 bytes shorter: ecg_mm_ptr_lens_kernel,
                      the same bytes but 32; the difference is the span records and the per-span
                      scalar loads

Device events, one warm-up, median of 9 per variant per round; after one discarded pass the
variants alternate within each of ROUNDS rounds in one process.  The self-check compares the parity
of the two routes of each part byte for byte.
-> the JSON file given with --out PATH (default build/bench_matmul_ptrs_lens.json).
Bench infrastructure (no oracle)."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from daos_amd import ecg  # noqa: E402
from tools.datagen import stripe_bytes  # noqa: E402

ROUNDS, REPS = 3, 9
K, P, OC = 8, 2, (37 << 24) | 1


def main():
    ctx = ecg.Context(0)
    L = ecg.lib()
    a, b = ctx.event(), ctx.event()
    coef = np.ascontiguousarray(ecg.cauchy1(K, P)[K:]).reshape(-1)
    cptr = ecg._u8(coef)

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

    def fill(buf, blk):
        buf.upload(blk[: min(blk.size, buf.nbytes)])
        for off in range(blk.size, buf.nbytes, blk.size):
            ecg._chk(L.ecg_memcpy(ctx.h, buf.ptr + off, buf.ptr, min(blk.size, buf.nbytes - off), 2, None), "D2D")
        ctx.sync()

    def vparr(addrs):
        return (C.c_void_p * len(addrs))(*addrs)

    def race(variants, check):
        rounds, kern = {v: [] for v in variants}, {}
        for v, fn in variants.items():          # a discarded pass: code objects loaded, clocks up
            print(f"# warming {v}", flush=True)
            timed(fn)
        for _ in range(ROUNDS):
            for v, fn in variants.items():
                rounds[v].append(timed(fn))
                kern[v] = ecg.last_kernel()
        check()
        row = {}
        for v, ts in rounds.items():
            row[v] = {"ms_rounds": [round(t, 4) for t in ts], "ms": round(sorted(ts)[len(ts) // 2], 4),
                      "spread_ms": round(max(ts) - min(ts), 4), "last_kernel": kern[v]}
        return row, rounds

    blk = stripe_bytes(256 << 20, 12)
    res = {"rounds": ROUNDS, "reps": REPS, "build_info": L.ecg_build_info().decode()}

    # ---- (a) single values ----
    N = 4096
    rng = np.random.default_rng(4096)
    sizes = [int(math.exp(x)) for x in rng.uniform(math.log(8 << 10), math.log(1 << 20), N)]
    cbs = [L.ecg_obj_ec_singv_cell_bytes(OC, n) for n in sizes]
    voff, at = [], 0
    for n in sizes:
        voff.append(at)
        at += (n + 255) & ~255
    vals = ctx.alloc(at)
    fill(vals, blk)
    par = [ctx.alloc(P * sum(cbs)) for _ in range(2)]          # [0] singv_dev, [1] per_size_ptrs
    poff, at = [], 0
    for cb in cbs:
        poff += [at + r * cb for r in range(P)]
        at += P * cb
    # per_size_ptrs: the straddling cell of each value zero padded in a side buffer (untimed)
    tail = ctx.alloc(sum(cbs))
    tail.fill(0)
    toff, at = [], 0
    for n, cb, vo in zip(sizes, cbs, voff):
        toff.append(at)
        if n % cb:
            ecg._chk(L.ecg_memcpy(ctx.h, tail.ptr + at, vals.ptr + vo + n // cb * cb, n % cb, 2, None), "D2D")
        at += cb
    ctx.sync()
    groups = {}
    for i, cb in enumerate(cbs):
        groups.setdefault(cb, []).append(i)
    per_size = []
    for cb, members in groups.items():
        tab = []
        for i in members:
            nfull = sizes[i] // cb
            assert nfull + (sizes[i] % cb != 0) == K, (sizes[i], cb)     # >= 8 KiB: no cell of padding alone
            tab += [vals.ptr + voff[i] + j * cb if j < nfull else tail.ptr + toff[i] for j in range(K)]
            tab += [par[1].ptr + poff[i * P + r] for r in range(P)]
        per_size.append((cb, len(members), vparr(tab)))
    sz = (C.c_uint64 * N)(*sizes)
    va = vparr([vals.ptr + o for o in voff])
    pa = vparr([par[0].ptr + o for o in poff])

    def singv_dev():
        ecg._chk(L.ecg_obj_ec_singv_encode_dev(ctx.h, OC, N, sz, va, pa, None), "singv_encode_dev")

    def per_size_ptrs():
        for cb, cnt, tab in per_size:
            ecg._chk(L.ecg_matmul_ptrs(ctx.h, K, P, cptr, cb, cnt, tab, None), "matmul_ptrs")

    def check_a():
        assert np.array_equal(par[0].download(), par[1].download()), "singv_dev != per_size_ptrs"

    row, rounds = race({"singv_dev": singv_dev, "per_size_ptrs": per_size_ptrs}, check_a)
    row.update({"values": N, "value_bytes": sum(sizes), "parity_bytes": P * sum(cbs), "distinct_cell_sizes": len(groups),
                "lens_plan": list(ecg.lens_plan(cbs)),
                "singv_dev_vs_per_size_ptrs": {
                    "median": round(row["singv_dev"]["ms"] / row["per_size_ptrs"]["ms"], 4),
                    "rounds": [round(x / y, 4) for x, y in zip(rounds["singv_dev"], rounds["per_size_ptrs"])]},
                "singv_dev_GBps_read_plus_written": round((sum(sizes) + P * sum(cbs)) / row["singv_dev"]["ms"] / 1e6, 1)})
    res["singv_EC_8P2_x4096_8KiB_1MiB"] = row
    print("singv", json.dumps(row), flush=True)
    for x in [vals, tail] + par:
        x.free()

    # ---- (b) one stripe 16 bytes shorter ----
    S, C_ = 512, 1 << 20
    n = K + P
    buf = ctx.alloc(S * n * C_)
    fill(buf, blk)
    out2 = ctx.alloc(S * P * C_)                                   # the uniform route's parity
    order = [int(s) for s in np.random.default_rng(512).permutation(S)]
    tab_l = vparr([buf.ptr + (s * n + j) * C_ for s in order for j in range(n)])
    tab_u = vparr([buf.ptr + (s * n + j) * C_ if j < K else out2.ptr + (s * P + j - K) * C_
                   for s in order for j in range(n)])
    lens = (C.c_uint64 * S)(*([C_] * S))
    lens[S // 2] = C_ - 16

    def uniform():
        ecg._chk(L.ecg_matmul_ptrs(ctx.h, K, P, cptr, C_, S, tab_u, None), "matmul_ptrs")

    def one_short():
        ecg._chk(L.ecg_matmul_ptrs_lens(ctx.h, K, P, cptr, S, tab_l, lens, None), "matmul_ptrs_lens")

    def check_b():
        for s in range(S):                      # stripe by stripe: the image is 5 GiB
            got = buf.download(P * C_, (s * n + K) * C_).reshape(P, C_)
            want = out2.download(P * C_, s * P * C_).reshape(P, C_)
            m = C_ - 16 if s == order[S // 2] else C_
            assert np.array_equal(got[:, :m], want[:, :m]), ("one_short != uniform", s)

    row, rounds = race({"uniform": uniform, "one_short": one_short}, check_b)
    assert row["uniform"]["last_kernel"] == "ecg_mm_ptr_kernel<8,2>", row
    assert row["one_short"]["last_kernel"] == "ecg_mm_ptr_lens_kernel<8,2>", row
    row.update({"stripes": S, "cell_bytes": C_, "lens_plan": list(ecg.lens_plan(list(lens))),
                "one_short_vs_uniform": {
                    "median": round(row["one_short"]["ms"] / row["uniform"]["ms"], 4),
                    "rounds": [round(x / y, 4) for x, y in zip(rounds["one_short"], rounds["uniform"])]},
                "uniform_GBps_read_plus_written": round(S * n * C_ / row["uniform"]["ms"] / 1e6, 1)})
    res["lens_EC_8P2_1MiB_x512_one_short"] = row
    print("lens", json.dumps(row), flush=True)
    buf.free()
    out2.free()

    out = os.path.join(ROOT, "build", "bench_matmul_ptrs_lens.json")
    if "--out" in sys.argv:
        out = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    print("self-check passed", flush=True)


if __name__ == "__main__":
    main()
