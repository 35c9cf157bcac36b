"""GPU parity of the product + checksums of every cell it touches
(include/ecg_csum.h ecg_encode_csum_all / ecg_recover_csum_all /
ecg_csum_compare) against the CPU oracle.  Bit-exact throughout.

The checksums of the cells the product *reads* come either from the fused
kernel's SRC instantiations (`ecg_mm_csum_kernel<k,rows,type,src>`) or from
two passes (the outputs as ecg_encode_csum computes them, then
ecg_csum_extents over the sources).  FUSED_DEFAULT restates the host's
measured default route per (hash type, k, output rows) -- DESIGN §11 carries
the same table; every shape is also run with the fused route forced
(ecg_set_csum_all_route 1), so the SRC kernels are checked where they are not
the default.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = {2: np.uint16, 4: np.uint32, 8: np.uint64}

# (htype, k, rows) whose default route is the fused SRC kernel
# (daos_amd/csrc/host/ecg_csum.c csum_all_fused_default)
FUSED_DEFAULT = {(2, 4, 2), (2, 8, 2), (2, 16, 2), (3, 16, 2)}

SRC_KS, SRC_ROWS = (2, 4, 8, 16), (1, 2, 3)


def _src_kernel(htype, k, rows):
    """Name prefix of the SRC instantiation a shape runs (ecg_fused_kernels.hip
    g_cskernels: its own, else the generic <0,0>), None when there is none."""
    if htype not in (1, 2, 3) or k > 16 or rows > 8:
        return None
    return f"ecg_mm_csum_kernel<{k},{rows}," if k in SRC_KS and rows in SRC_ROWS else "ecg_mm_csum_kernel<0,0,"


def _cell_csums(oracle, htype, cs, rb, cells):
    """oracle checksums of each cell (last axis), as extents at record index 0."""
    C = cells.shape[-1]
    flat = np.ascontiguousarray(cells.reshape(-1, C))
    return oracle.csum_extents(htype, cs, rb, 0, C // rb, flat.reshape(-1), ext_stride=C, n_ext=flat.shape[0])


@functools.lru_cache(maxsize=None)
def _encode_ref(oracle, k, p, C, S, cs, rb, htype, seed):
    """(data [S*k*C], parity [p][S][C], data csums [k][S][nch], parity csums [p][S][nch]) -- computed once,
    shared (read-only) by the tests of one shape."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, S * k * C, dtype=np.uint8)
    par = oracle.encode_batch(k, p, C, S, data, nthreads=8, simd=True).reshape(p, S, C)
    dcells = np.ascontiguousarray(data.reshape(S, k, C).transpose(1, 0, 2))
    dcs = _cell_csums(oracle, htype, cs, rb, dcells).reshape(k, S, -1)
    pcs = _cell_csums(oracle, htype, cs, rb, par).reshape(p, S, -1)
    for a in (data, par, dcs, pcs):
        a.setflags(write=False)
    return data, par, dcs, pcs


def _run_encode_all(ecglib, ctx, case, data, rt, off=0, csoff=0):
    """-> (parity [p][S][C], data csums [k][S][nch], parity csums [p][S][nch], last kernel)."""
    k, p, C, S, cs, rb, htype = case
    L = ecglib.lib()
    nch = L.ecg_csum_chunk_count(cs, rb, 0, C // rb)
    cl = L.ecg_csum_len(htype)
    d = ctx.alloc(data.nbytes + 64)
    par = ctx.alloc(p * S * C + 64)
    dcs = ctx.alloc(k * S * nch * cl + 16)
    pcs = ctx.alloc(p * S * nch * cl + 16)
    try:
        d.upload(data, offset=off)
        dcs.fill(0xA5)
        pcs.fill(0xA5)
        ctx.set_csum_all_route(rt)
        ctx.encode_csum_all(k, p, C, S, d.ptr + off, k * C, par.ptr + off, S * C, C, htype, cs, rb,
                            dcs.ptr + csoff, pcs.ptr + csoff)
        ctx.sync()
        kern = L.ecg_last_kernel().decode()
        return (par.download(p * S * C, offset=off).reshape(p, S, C),
                dcs.download(k * S * nch * cl, offset=csoff).view(DT[cl]).reshape(k, S, nch),
                pcs.download(p * S * nch * cl, offset=csoff).view(DT[cl]).reshape(p, S, nch), kern)
    finally:
        ctx.set_csum_all_route(0)
        d.free(); par.free(); dcs.free(); pcs.free()


FUSED = [
    # (k, p, C, S, chunksize, rec_size, htype)
    (2, 1, 64 << 10, 4, 32768, 1, 2),
    (4, 2, 128 << 10, 3, 32768, 1, 2),
    (8, 2, 128 << 10, 3, 32768, 1, 1),
    (8, 2, 128 << 10, 3, 32768, 1, 2),
    (8, 2, 128 << 10, 3, 32768, 1, 3),
    (16, 2, 128 << 10, 2, 16384, 1, 2),
    (8, 3, 64 << 10, 3, 4096, 1, 3),
    (4, 1, 65536 + 48, 3, 32768, 1, 2),       # ragged last chunk (not a 4 KiB multiple)
    (4, 2, 100000, 3, 8192, 8, 1),            # 8-byte records, ragged
    (16, 3, 40960, 3, 12288, 4096, 3),        # records of 4 KiB, 3 per chunk
    (5, 2, 64 << 10, 2, 32768, 1, 2),         # no <5,2> instantiation: the generic kernel's shape
]


@pytest.mark.parametrize("rt", [0, 1], ids=["default", "fused"])
@pytest.mark.parametrize("case", FUSED)
def test_encode_csum_all_fused(oracle, ecglib, ctx, case, rt):
    """Parity, data checksums and parity checksums equal the oracle's on the
    default route and with the fused route forced; the last kernel is the SRC
    instantiation exactly where the route table says so (forced: wherever one
    exists)."""
    k, p, C, S, cs, rb, htype = case
    data, want_par, want_dcs, want_pcs = _encode_ref(oracle, k, p, C, S, cs, rb, htype, sum(case))
    par, dcs, pcs, kern = _run_encode_all(ecglib, ctx, case, data, rt)
    fused = rt == 1 or (htype, k, p) in FUSED_DEFAULT
    assert kern.endswith(",src>") == fused, kern
    if fused:
        assert kern.startswith(_src_kernel(htype, k, p)), kern
    assert np.array_equal(par, want_par)
    assert np.array_equal(dcs, want_dcs), np.argwhere(dcs != want_dcs)[:5]
    assert np.array_equal(pcs, want_pcs), np.argwhere(pcs != want_pcs)[:5]


ITEM_CASES = [
    # (k, p, C, S, chunksize, htype): the geometries of test_gpu_csum.py ITEM_CASES, the 1 MiB chunk scaled to 256 KiB
    (8, 2, 3 * 65536 + 4096 * 3 + 48, 3, 65536, 2),      # last chunk 3 columns + 48 B
    (4, 1, (1 << 18) + 48, 2, 1 << 18, 1),                 # 64-column chunks, last chunk 48 B
    (8, 3, 5 * 32768, 2, 32768, 3),
    (16, 2, 131072 + 16, 2, 40960, 2),                     # 10-column chunks
]


@pytest.mark.parametrize("cols", [1, 2, 3, 5, 0])
@pytest.mark.parametrize("case", ITEM_CASES)
def test_encode_csum_all_items(oracle, ecglib, ctx, case, cols):
    """Every split of a chunk into work items (ecg_set_fused_cols; 0 = the
    default) yields the same data and parity checksums from the SRC kernel."""
    k, p, C, S, cs, htype = case
    full = (k, p, C, S, cs, 1, htype)
    data, want_par, want_dcs, want_pcs = _encode_ref(oracle, k, p, C, S, cs, 1, htype, sum(case))
    L = ecglib.lib()
    assert L.ecg_set_fused_cols(ctx.h, cols) == 0
    try:
        par, dcs, pcs, kern = _run_encode_all(ecglib, ctx, full, data, 1)
    finally:
        L.ecg_set_fused_cols(ctx.h, 0)
    assert kern.startswith(f"ecg_mm_csum_kernel<{k},{p},") and kern.endswith(",src>"), kern
    assert np.array_equal(par, want_par)
    assert np.array_equal(dcs, want_dcs), np.argwhere(dcs != want_dcs)[:5]
    assert np.array_equal(pcs, want_pcs), np.argwhere(pcs != want_pcs)[:5]


@functools.lru_cache(maxsize=None)
def _stripes_ref(oracle, k, p, C, S, cs, htype, seed):
    """(stripes [S][k+p][C], cell csums [k+p][S][nch])"""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, (S, k, C), dtype=np.uint8)
    en = oracle.cauchy1(k, p)
    stripes = np.zeros((S, k + p, C), dtype=np.uint8)
    for s in range(S):
        stripes[s, :k] = data[s]
        stripes[s, k:] = oracle.encode_data(en[k:], data[s])
    cells = np.ascontiguousarray(stripes.transpose(1, 0, 2))
    ccs = _cell_csums(oracle, htype, cs, 1, cells).reshape(k + p, S, -1)
    stripes.setflags(write=False)
    ccs.setflags(write=False)
    return stripes, ccs


@pytest.mark.parametrize("errs", [[3, 9], [9, 3], [8, 9], [0], [0, 1], [5]])
@pytest.mark.parametrize("htype", (2, 3))
def test_recover_csum_all(oracle, ecglib, ctx, errs, htype):
    """Stripes restored, csums in err_list order, src_idx k distinct
    surviving cells, src_csums[i] the checksums of cell src_idx[i] (a parity
    cell among them when a data cell is lost) -- on both routes."""
    k, p, C, S, cs = 8, 2, 128 << 10, 4, 32768
    L = ecglib.lib()
    nch = C // cs
    cl = L.ecg_csum_len(htype)
    stripes, ccs = _stripes_ref(oracle, k, p, C, S, cs, htype, 77 + htype)
    broken = stripes.copy()
    broken[:, errs] = 0
    d = ctx.alloc(broken.nbytes)
    out = ctx.alloc(len(errs) * S * nch * cl)
    sout = ctx.alloc(k * S * nch * cl)
    try:
        for rt in (0, 1):
            d.upload(broken)
            out.fill(0xA5)
            sout.fill(0xA5)
            ctx.set_csum_all_route(rt)
            idx = ctx.recover_csum_all(k, p, C, S, d.ptr, (k + p) * C, errs, htype, cs, 1, out.ptr, sout.ptr)
            ctx.sync()
            kern = L.ecg_last_kernel().decode()
            fused = rt == 1 or (htype, k, len(errs)) in FUSED_DEFAULT
            assert kern.endswith(",src>") == fused, kern
            assert np.array_equal(d.download().reshape(S, k + p, C), stripes)
            got = out.download().view(DT[cl]).reshape(len(errs), S, nch)
            for i, e in enumerate(errs):
                assert np.array_equal(got[i], ccs[e]), (e, i, rt)
            assert len(idx) == k and len(set(idx)) == k
            assert all(i < k + p and i not in errs for i in idx)
            if any(e < k for e in errs):
                assert any(i >= k for i in idx)      # a parity cell is a source
            sgot = sout.download().view(DT[cl]).reshape(k, S, nch)
            for i, cell in enumerate(idx):
                assert np.array_equal(sgot[i], ccs[cell]), (cell, i, rt)
    finally:
        ctx.set_csum_all_route(0)
        d.free(); out.free(); sout.free()


@pytest.mark.parametrize("variant", ["adler32", "chunk_not_4k", "unaligned", "k_over_16", "csums_2byte_aligned"])
def test_csum_all_fallback(oracle, ecglib, ctx, variant):
    """Shapes the SRC kernel does not take run two passes even with the fused
    route forced: results exact, the last kernel not the fused one."""
    k, p, C, S, cs, rb, htype, off, csoff = 4, 2, 128 << 10, 3, 32768, 1, 2, 0, 0
    if variant == "adler32":
        htype = 7
    elif variant == "chunk_not_4k":
        cs = 6000
    elif variant == "unaligned":
        off = 4
    elif variant == "k_over_16":
        k = 20
    else:
        htype, csoff = 1, 2
    case = (k, p, C, S, cs, rb, htype)
    data, want_par, want_dcs, want_pcs = _encode_ref(oracle, k, p, C, S, cs, rb, htype, 3)
    par, dcs, pcs, kern = _run_encode_all(ecglib, ctx, case, data, 1, off=off, csoff=csoff)
    assert "ecg_mm_csum_kernel" not in kern, kern
    assert np.array_equal(par, want_par)
    assert np.array_equal(dcs, want_dcs)
    assert np.array_equal(pcs, want_pcs)


def test_csum_all_matches_two_pass(oracle, ecglib, ctx):
    """ecg_encode_csum_all (SRC kernel) == ecg_encode_csum + ecg_csum_extents over
    the data, byte for byte; the parity-only call still gives the oracle's."""
    case = k, p, C, S, cs, rb, htype = 8, 2, 128 << 10, 3, 32768, 1, 2
    L = ecglib.lib()
    nch, cl = C // cs, L.ecg_csum_len(htype)
    data, want_par, want_dcs, want_pcs = _encode_ref(oracle, k, p, C, S, cs, rb, htype, sum(case))
    par, dcs, pcs, kern = _run_encode_all(ecglib, ctx, case, data, 1)
    assert kern.endswith(",src>"), kern
    d = ctx.to_device(data)
    par2 = ctx.alloc(p * S * C)
    pcs2 = ctx.alloc(p * S * nch * cl)
    dcs2 = ctx.alloc(k * S * nch * cl)
    try:
        ctx.encode_csum(k, p, C, S, d.ptr, k * C, par2.ptr, S * C, C, htype, cs, rb, pcs2.ptr)
        ctx.sync()
        assert L.ecg_last_kernel().decode() == f"ecg_mm_csum_kernel<{k},{p},crc32>"
        ctx.csum_extents(htype, cs, rb, 0, C // rb, d.ptr, C, S * k, dcs2.ptr)
        ctx.sync()
        got_par2 = par2.download().reshape(p, S, C)
        got_pcs2 = pcs2.download().view(DT[cl]).reshape(p, S, nch)
        got_dcs2 = dcs2.download().view(DT[cl]).reshape(S, k, nch).transpose(1, 0, 2)
        assert np.array_equal(got_par2, want_par) and np.array_equal(got_pcs2, want_pcs)
        assert par.tobytes() == got_par2.tobytes()
        assert pcs.tobytes() == got_pcs2.tobytes()
        assert dcs.tobytes() == np.ascontiguousarray(got_dcs2).tobytes()
    finally:
        d.free(); par2.free(); pcs2.free(); dcs2.free()


@pytest.mark.parametrize("rt", [1, 2], ids=["fused", "two_pass"])
def test_csum_all_stats(oracle, ecglib, ctx, rt):
    """csum_chunks counts the source cells' chunks as well as the outputs', on either route."""
    case = k, p, C, S, cs, rb, htype = 4, 2, 64 << 10, 3, 32768, 1, 2
    data = _encode_ref(oracle, k, p, C, S, cs, rb, htype, sum(case))[0]
    ctx.stats(reset=True)
    _run_encode_all(ecglib, ctx, case, data, rt)
    st = ctx.stats()
    assert st["csum_chunks"] == (k + p) * S * (C // cs)
    assert st["encode_stripes"] == S and st["encode_bytes"] == k * C * S


@pytest.mark.parametrize("rt", [0, 1], ids=["default", "fused"])
@pytest.mark.parametrize("flip", [False, True])
def test_verified_degraded_read(oracle, ecglib, ctx, flip, rt):
    """Encode on the device and keep every cell's checksums; lose two cells,
    corrupt one byte of one surviving cell of one stripe; recover_csum_all +
    csum_compare of the survivors' checksums against the kept rows reports
    exactly that (row, stripe, chunk) -- and nothing without the corruption."""
    k, p, C, S, cs, htype = 8, 2, 128 << 10, 4, 32768, 3
    L = ecglib.lib()
    nch, cl = C // cs, L.ecg_csum_len(htype)
    stripes, ccs = _stripes_ref(oracle, k, p, C, S, cs, htype, 5)
    errs = [2, 9]
    _, dec, _ = ecglib.recov_matrix(k, p, errs)
    victim, vs, vc = int(dec[-1]), 2, 1            # the last source cell, stripe 2, chunk 1
    assert victim >= k                             # a parity cell among the survivors
    st = ctx.alloc(stripes.nbytes)
    kept = ctx.alloc((k + p) * S * nch * cl)       # data rows, then parity rows
    out = ctx.alloc(len(errs) * S * nch * cl)
    sout = ctx.alloc(k * S * nch * cl)
    want = ctx.alloc(k * S * nch * cl)
    res = ctx.alloc(16)
    try:
        host = stripes.copy()
        host[:, k:] = 0
        st.upload(host)
        ctx.set_csum_all_route(rt)
        ctx.encode_csum_all(k, p, C, S, st.ptr, (k + p) * C, st.ptr + k * C, C, (k + p) * C, htype, cs, 1,
                            kept.ptr, kept.ptr + k * S * nch * cl)
        ctx.sync()
        assert np.array_equal(st.download().reshape(S, k + p, C), stripes)
        kept_rows = kept.download().view(DT[cl]).reshape(k + p, S, nch)
        assert np.array_equal(kept_rows, ccs)
        host = st.download().reshape(S, k + p, C)
        host[:, errs] = 0
        if flip:
            host[vs, victim, vc * cs + 12345] ^= 0x40
        st.upload(host)
        idx = ctx.recover_csum_all(k, p, C, S, st.ptr, (k + p) * C, errs, htype, cs, 1, out.ptr, sout.ptr)
        assert idx == [int(i) for i in dec]
        want.upload(np.ascontiguousarray(kept_rows[idx]))
        res.fill(0x5A)
        ctx.csum_compare(htype, sout.ptr, want.ptr, k * S * nch, res.ptr)
        ctx.sync()
        assert L.ecg_last_kernel().decode() == "ecg_csum_compare_kernel"
        count, first = res.download().view(np.uint64)
        if flip:
            assert count == 1
            assert first == (idx.index(victim) * S + vs) * nch + vc
        else:
            assert count == 0 and first == np.uint64(0xFFFFFFFFFFFFFFFF)
            assert np.array_equal(st.download().reshape(S, k + p, C), stripes)
    finally:
        ctx.set_csum_all_route(0)
        for b in (st, kept, out, sout, want, res):
            b.free()


def test_csum_all_errors(ecglib, ctx):
    L = ecglib.lib()
    b = ctx.alloc(1 << 16)
    o = ctx.alloc(4096)
    idx = (ecglib.C.c_uint32 * 4)()
    errs = ecglib._u32([0, 1, 2])
    try:
        assert L.ecg_encode_csum_all(ctx.h, 4, 2, 4096, 1, b.ptr, 4 * 4096, b.ptr, 4096, 4096, 4, 4096, 1, o.ptr,
                                     o.ptr, None) == -2037                       # SHA256
        assert L.ecg_recover_csum_all(ctx.h, 4, 2, 4096, 1, b.ptr, 6 * 4096, errs, 1, 4, 4096, 1, o.ptr, o.ptr,
                                      idx, None) == -2037
        assert L.ecg_csum_compare(ctx.h, 4, o.ptr, o.ptr, 4, o.ptr, None) == -2037
        assert L.ecg_encode_csum_all(ctx.h, 4, 2, 4096, 1, b.ptr, 4 * 4096, b.ptr, 4096, 4096, 2, 4096, 1, None,
                                     o.ptr, None) == -ecglib.DER_INVAL           # NULL data_csums
        assert L.ecg_encode_csum_all(ctx.h, 4, 2, 4097, 1, b.ptr, 4 * 4097, b.ptr, 4097, 4097, 2, 4096, 2, o.ptr,
                                     o.ptr, None) == -ecglib.DER_INVAL           # cell not a multiple of the record
        assert L.ecg_recover_csum_all(ctx.h, 4, 2, 4096, 1, b.ptr, 6 * 4096, errs, 1, 2, 4096, 1, o.ptr, None,
                                      idx, None) == -ecglib.DER_INVAL            # NULL src_csums
        assert L.ecg_recover_csum_all(ctx.h, 4, 2, 4096, 1, b.ptr, 6 * 4096, errs, 3, 2, 4096, 1, o.ptr, o.ptr,
                                      idx, None) == -ecglib.DER_DATA_LOSS        # nerrs > p
        b.fill(0xA5)
        o.fill(0xA5)
        ctx.sync()
        assert L.ecg_recover_csum_all(ctx.h, 4, 2, 4096, 1, b.ptr, 6 * 4096, errs, 0, 2, 4096, 1, o.ptr,
                                      o.ptr + 2048, idx, None) == 0              # nothing to recover
        ctx.sync()
        assert np.all(b.download() == 0xA5) and np.all(o.download() == 0xA5)
    finally:
        b.free(); o.free()
