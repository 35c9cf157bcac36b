"""The stripe walk ecg_repair, ecg_recover_masks and ecg_update_masks share (kernels/
ecg_rows_dev.h), where its parts meet: the sparse grid (block rows of 64 stripes), a row loop
that strides (2 block rows for 3), a ragged last row (S = 130), one column block for two columns
(the last a single 16-byte lane, or 5 bytes in the byte kernels), and the same table needed on
both sides of a row boundary -- stripes 63 and 64 name the same cell or set, so a lane kernel
that stages a table per stripe carries it from one row into the next; stripe 129 names another.
Stripe 65 holds a word the call refuses.

The rigs and references are the three calls' own (test_gpu_repair, test_gpu_recover_masks,
test_gpu_update_masks): images from the CPU oracle between guard bytes, compared whole."""
import numpy as np
import pytest

from tests import test_gpu_recover_masks as rm
from tests import test_gpu_repair as rep
from tests import test_gpu_update_masks as um

pytestmark = pytest.mark.gpu

K, P, S = 4, 2, 130         # EC_4P2; rows of 64 stripes: 0-63, 64-127, 128-129
U64MAX = (1 << 64) - 1


def run_repair(ctx, ecglib, oracle, C_, skew, byte):
    """Cells 1 (data), 4 (parity), 4, 2 (data) of stripes 0, 63, 64, 129 wrong in every byte and
    located; stripe 65 wrong too, its word naming two candidates.  -> units: data cells."""
    located = {0: 1, 63: 4, 64: 4, 129: 2}
    rig = rep.Rig(ctx, oracle, K, P, C_, "recov", S_=S, skew=skew)
    try:
        want = rig.copy()
        noise = np.random.default_rng(C_).integers(1, 256, C_, dtype=np.uint8)
        for s, c in {**located, 65: 0}.items():
            rig.cell(rig.img, s, c)[:] ^= noise
        rig.cell(want, 65, 0)[:] = rig.cell(rig.img, 65, 0)
        status = [0] * S
        for s, c in located.items():
            status[s] = rep.attributing(K, P, c)
        status[65] = rep.st((1 << P) - 1, 0b11)
        rig.upload()
        res, name = rig.repair(ecglib, status)
        assert name == ("ecg_repair_byte_kernel" if byte else rep.kernel_name(K))
        got = rig.download()
        for n in want:
            rm.same(got[n], want[n], rig)
        return res, sum(1 for c in located.values() if c < K)
    finally:
        rig.free()


def run_recover_masks(ctx, ecglib, oracle, C_, skew, byte):
    """Sets {0, 5}, {2}, {2}, {1, 3} at stripes 0, 63, 64, 129; three cells at 65.  -> units:
    cells regenerated."""
    masks = [0] * S
    masks[0], masks[63], masks[64], masks[129], masks[65] = 0b100001, 0b100, 0b100, 0b1010, 0b111
    rig = rm.Rig(ctx, K, P, C_, rm.codewords(oracle, K, P, C_, S), skew=skew)
    try:
        want = rig.img.copy()
        rig.erase(masks)
        rig.view(want)[65] = rig.view(rig.img)[65]
        got, res, name = rig.run(ecglib, masks, ecglib.RM_SPARSE)
        assert name == ("ecg_recover_masks_byte_kernel" if byte else rm.kernel_name(K, P))
        rm.same(got, want, rig)
        return res, 2 + 1 + 1 + 2
    finally:
        rig.free()


def run_update_masks(ctx, ecglib, oracle, C_, skew, byte):
    """Cells {0, 3}, {1, 2}, {1, 2}, {2} at stripes 0, 63, 64, 129; a bit at k at 65.  -> units:
    cells applied."""
    masks = [0] * S
    masks[0], masks[63], masks[64], masks[129], masks[65] = 0b1001, 0b0110, 0b0110, 0b0100, 1 << K | 1
    rig = um.Rig(ctx, oracle, K, P, C_, masks, skew=skew)
    try:
        want = rig.expect(oracle)
        got, res, name = rig.run(ecglib, ecglib.RM_SPARSE)
        assert name == (um.BYTE_KERNEL if byte else um.lane_kernel(P))
        um.same(got, want, rig)
        return res, 2 + 2 + 2 + 1
    finally:
        rig.free()


@pytest.mark.parametrize("variant", [0, 2])
@pytest.mark.parametrize("run", [run_repair, run_recover_masks, run_update_masks])
def test_sparse_rows_stride_and_share_a_table(ctx, ecglib, oracle, run, variant):
    shapes = [(4096 + 16, 0)] + ([(4096 + 5, 1)] if variant == 2 else [])
    ctx.set_launch(1, 2, variant)
    try:
        for C_, skew in shapes:
            res, units = run(ctx, ecglib, oracle, C_, skew, variant == 2)
            assert res == [4, 65, units, 1], (C_, skew)
    finally:
        ctx.set_launch(0, 0, 0)
