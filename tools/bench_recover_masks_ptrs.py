"""ecg_recover_masks_ptrs (include/ecg.h) against the strided call and against the
routes callers with scattered stripes have today.  Stripes encoded on the device;
recovering a cell that is already right moves the same bytes, so every batch
stays a batch of codewords and no variant needs a restore between calls.  Every
stripe has p erasures, the sets drawn at random over the batch.

  strided         ecg_recover_masks on the contiguous image [S][k+p][C]: the
                  reference pace
  ptrs_permuted   the same memory through a table whose stripes come in a random
                  order, so not affine: the cost of the table and the dependent
                  address loads alone
  ptrs_scattered  every stripe an allocation of its own
  per_set_ptrs    today's route for scattered stripes: the host has grouped the
                  stripes by erasure set (outside the timed region) and issues
                  one ecg_matmul_ptrs per set with the rows of ecg_recov_matrix
  per_stripe      one ecg_recover(nstripes = 1) per stripe on the scattered
                  buffers
  pct1_sparse     the permuted table with 1 % of the stripes masked (one cell
  clean_sparse    each) / with zero masks, ECG_RM_SPARSE: what the upload of the
                  8 * (k+p) * S byte table costs a scrub

Device events, one warm-up, median of 9 per variant per round; after one
discarded pass the variants alternate within each of ROUNDS rounds in one
process, so each one's round-to-round spread is visible.  The self-check at the
end overwrites the erased cells, recovers them with one call per table route and
expects ecg_verify clean and the result words.
-> the JSON file given with --out PATH (default build/bench_recover_masks_ptrs.json).
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
U64MAX = (1 << 64) - 1
RATIOS = (("ptrs_permuted", "strided"), ("ptrs_scattered", "strided"), ("ptrs_scattered", "per_set_ptrs"),
          ("ptrs_scattered", "per_stripe"))


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

    def vparr(addrs):
        return (C.c_void_p * len(addrs))(*addrs)

    blk = stripe_bytes(256 << 20, 12)
    res = {"rounds": ROUNDS, "reps": REPS, "shapes": {}}
    for k, p, C_, S in SHAPES:
        n, stride = k + p, (k + p) * C_
        buf = ctx.alloc(S * stride)
        buf.upload(blk[: min(blk.size, S * stride)])
        for off in range(blk.size, S * stride, blk.size):
            d2d(buf.ptr + off, buf.ptr, min(blk.size, S * stride - off))
        ctx.encode(k, p, C_, S, buf.ptr, stride, buf.ptr + k * C_, C_, stride)
        own = [ctx.alloc(stride) for _ in range(S)]         # the scattered copy of the batch, in no address order
        own = [own[int(i)] for i in np.random.default_rng(S + k).permutation(S)]
        for s, x in enumerate(own):
            d2d(x.ptr, buf.ptr + s * stride, stride)
        ctx.sync()

        rng = np.random.default_rng(1000 * k + p)
        sets = [sorted(int(c) for c in rng.choice(n, p, replace=False)) for _ in range(S)]
        m_dense = np.array([sum(1 << c for c in cs) for cs in sets], dtype=np.uint32)
        m_pct1 = np.zeros(S, dtype=np.uint32)
        for i, s in enumerate(range(0, S, 100)):
            m_pct1[s] = 1 << (i * 7 % n)
        order = [int(s) for s in rng.permutation(S)]
        dev = {}
        for name, m in (("dense", m_dense), ("dense_perm", m_dense[order]), ("pct1_perm", m_pct1[order]),
                        ("clean", np.zeros(S, dtype=np.uint32))):
            dev[name] = ctx.alloc(4 * S)
            dev[name].upload(m.view(np.uint8))
        rr, rv, status = ctx.alloc(32), ctx.alloc(32), ctx.alloc(4 * S)
        t_perm = vparr([buf.ptr + s * stride + c * C_ for s in order for c in range(n)])
        t_own = vparr([x.ptr + c * C_ for x in own for c in range(n)])

        # per_set_ptrs: the grouping and the rows are the host's work before the launches
        groups = {}
        for s, cs in enumerate(sets):
            groups.setdefault(tuple(cs), []).append(s)
        per_set = []
        for cs, members in groups.items():
            rows, dec, _ = ecg.recov_matrix(k, p, list(cs))
            coef = np.ascontiguousarray(rows, dtype=np.uint8).reshape(-1)
            tab = vparr([own[s].ptr + int(c) * C_ for s in members for c in list(dec) + list(cs)])
            per_set.append((coef, ecg._u8(coef), len(members), tab))

        def ptrs(tab, which, flags=0):
            return lambda: ctx.recover_masks_ptrs(k, p, C_, S, tab, dev[which].ptr, rr.ptr, flags)

        def per_set_ptrs():
            for _, coef, cnt, tab in per_set:
                ecg._chk(L.ecg_matmul_ptrs(ctx.h, k, p, coef, C_, cnt, tab, None), "matmul_ptrs")

        def per_stripe():
            for s, cs in enumerate(sets):
                ctx.recover(k, p, C_, 1, own[s].ptr, stride, cs)

        name = f"EC_{k}P{p}_{C_ >> 10}KiB_x{S}"
        variants = {
            "strided": lambda: ctx.recover_masks(k, p, C_, S, buf.ptr, stride, dev["dense"].ptr, rr.ptr, 0),
            "ptrs_permuted": ptrs(t_perm, "dense_perm"),
            "ptrs_scattered": ptrs(t_own, "dense"),
            "per_set_ptrs": per_set_ptrs,
            "per_stripe": per_stripe,
            "pct1_sparse": ptrs(t_perm, "pct1_perm", ecg.RM_SPARSE),
            "clean_sparse": ptrs(t_perm, "clean", ecg.RM_SPARSE),
        }
        rounds = {v: [] for v in variants}
        kern = {}
        for v, fn in variants.items():          # a discarded pass: code objects loaded, clocks up
            print(f"# {name}: warming {v}", flush=True)
            timed(fn)
        for _ in range(ROUNDS):
            for v, fn in variants.items():
                rounds[v].append(timed(fn))
                kern[v] = ecg.last_kernel()
        assert kern["ptrs_permuted"].startswith("ecg_recover_masks_ptr_kernel<"), kern
        assert kern["ptrs_scattered"].startswith("ecg_recover_masks_ptr_kernel<"), kern

        # what the timed calls computed: the erased cells overwritten, one call, the batch verifies clean
        for tab, which, m, flags, scattered in ((t_perm, "dense_perm", m_dense, 0, False),
                                                (t_own, "dense", m_dense, 0, True),
                                                (t_perm, "pct1_perm", m_pct1, ecg.RM_SPARSE, False)):
            for s in np.flatnonzero(m):
                base = own[int(s)].ptr if scattered else buf.ptr + int(s) * stride
                for c in range(n):
                    if int(m[s]) >> c & 1:
                        ecg._chk(L.ecg_memset(ctx.h, base + c * C_, 0x5A, C_, None), "memset")
            ctx.recover_masks_ptrs(k, p, C_, S, tab, dev[which].ptr, rr.ptr, flags)
            if scattered:                       # ecg_verify reads one image
                for s, x in enumerate(own):
                    d2d(buf.ptr + s * stride, x.ptr, stride)
            ctx.verify(k, p, C_, S, buf.ptr, stride, buf.ptr + k * C_, C_, stride, status.ptr, rv.ptr)
            ctx.sync()
            nz = int(np.count_nonzero(m))
            ncell = sum(bin(int(x)).count("1") for x in m)
            assert words(rr) == [nz, U64MAX, ncell, 0], (which, flags, words(rr))
            assert words(rv) == [0, U64MAX, 0, 0], (which, flags, words(rv))

        row = {"stripes_masked_pct1": int(np.count_nonzero(m_pct1)), "erasure_sets_in_batch": len(groups),
               "table_bytes": 8 * n * S, "bytes_written": S * p * C_, "bytes_read": S * k * C_}
        for v, ts in rounds.items():
            med = sorted(ts)[len(ts) // 2]
            row[v] = {"ms_rounds": [round(t, 4) for t in ts], "ms": round(med, 4),
                      "spread_ms": round(max(ts) - min(ts), 4), "last_kernel": kern[v]}
        for num, den in RATIOS:
            row[f"{num}_vs_{den}"] = {
                "median": round(row[num]["ms"] / row[den]["ms"], 3),
                "rounds": [round(x / y, 3) for x, y in zip(rounds[num], rounds[den])]}
            if den == "strided":                # "at the strided pace" = inside the strided row's own max - min
                row[f"{num}_vs_{den}"]["within_strided_spread"] = \
                    abs(row[num]["ms"] - row["strided"]["ms"]) <= row["strided"]["spread_ms"]
        row["ptrs_scattered_GBps_read_plus_written"] = round(S * (k + p) * C_ / row["ptrs_scattered"]["ms"] / 1e6, 1)
        res["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
        for x in [buf, rr, rv, status] + own + list(dev.values()):
            x.free()
    out = os.path.join(ROOT, "build", "bench_recover_masks_ptrs.json")
    if "--out" in sys.argv:
        out = os.path.abspath(sys.argv[sys.argv.index("--out") + 1])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    ctx.close()
    print("self-check passed", flush=True)


if __name__ == "__main__":
    main()
