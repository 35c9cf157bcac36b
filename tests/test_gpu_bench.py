"""A plain `bench.py` run on the GPU: the result line and --dump-outputs.

The plain run no longer checks itself (`verified` belongs to --full), so
this test checks what it dumps against the oracle: of the sampled 4 KiB
pieces, those whose inputs lie in the first 8 MiB of the seeded 256 MiB input
block (tools/datagen.py: a shorter block is a prefix of a longer one).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
PRE = 8 << 20               # input-block prefix regenerated here
BLK = 256 << 20             # bench.fill_device's tile


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path, oracle):
    sys.path.insert(0, ROOT)
    import bench
    from tools.datagen import stripe_bytes

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["metric"] == "EC encode+decode GiB/s (device-resident stripes)" and d["unit"] == "GiB/s"
    assert d["higher_is_better"] is True and d["dtype"] == "u8" and d["steps"] == 3 and d["n_gpus"] == 1
    k, p, C, S = bench.WORKLOADS["enc_dec_4p2"][:4]
    # value and ms_per_step state the same wall time of the timed steps
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] * d["ms_per_step"] / (2 * k * C * S / bench.GIB * 1e3) - 1) < 1e-2   # rounding of ms
    # nothing but the headline ran
    assert "detail" not in d and d["cpu_baseline"] is None and d["verified"] is None
    assert "measured_stream_GBps" not in d["roofline"]

    assert sorted(os.listdir(out)) == ["parity.npy", "recovered.npy"]
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 << 20
    par, rec = np.load(out / "parity.npy"), np.load(out / "recovered.npy")
    share, P = bench.DUMP_BYTES // 2, bench.DUMP_PIECE
    assert par.dtype == rec.dtype == np.float32 and par.shape == rec.shape == (share,)

    coef = oracle.cauchy1(k, p)[k:]
    data_blk, img_blk = stripe_bytes(PRE, 2), stripe_bytes(PRE, 3)     # Workload's config ids
    checked = 0
    for n, j in enumerate(bench.dump_pieces(p * S * C, share, 0)):      # parity [p][S][C]
        row, within = divmod(int(j) * P, S * C)
        s, o = divmod(within, C)
        src = [((s * k + c) * C + o) % BLK for c in range(k)]
        if max(src) + P > PRE:
            continue
        want = oracle.encode_data(coef, np.stack([data_blk[x:x + P] for x in src]))[row]
        assert np.array_equal(par[n * P:(n + 1) * P], want), f"parity piece {j}"
        checked += 1
    assert checked >= 16, checked
    checked = 0
    err, st = [0, 1], (k + p) * C
    for n, j in enumerate(bench.dump_pieces(S * len(err) * C, share, 1)):  # regenerated cells [S][2][C]
        cell, o = divmod(int(j) * P, C)
        src = ((cell // 2) * st + err[cell % 2] * C + o) % BLK
        if src + P > PRE:
            continue
        assert np.array_equal(rec[n * P:(n + 1) * P], img_blk[src:src + P]), f"recovered piece {j}"
        checked += 1
    assert checked >= 16, checked
