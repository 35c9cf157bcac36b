/*
 * ecg_update_masks.c -- aggregation delta parity update with one set of
 * updated cells per stripe (include/ecg.h ecg_update_masks).
 *
 * What it replaces: ecg_update takes one cell_idx list for a whole batch, so
 * a batch whose stripes changed different cells is issued as one call per
 * distinct set, and ecg_update_ptrs takes a host table of one record per
 * updated cell, which the host has to know, sort and stage.  Here the sets
 * are mask words that stay on the device (ecg_csum_mask writes them from the
 * checksums of the old and the new image): one launch reads them, and each
 * block folds the cells its stripe's mask names into the stripe's parity
 * (kernels/ecg_update_masks_kernels.hip).
 *
 * The tables are the Cauchy parity rows of all k columns, which do not depend
 * on the stripe: they travel in the launch's parameters, so the call needs no
 * per-context table and no synchronous upload.
 */
#include <stdlib.h>
#include <string.h>

#include "ecg_internal.h"

int ecg_update_masks(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S,
		     const void *old_cells, const void *new_cells, int64_t upd_stripe_stride,
		     void *parity, int64_t parity_cell_stride, int64_t parity_stripe_stride,
		     const uint32_t *masks, void *result, unsigned flags, void *stream)
{
	unsigned char en[(ECG_MAX_K + ECG_MAX_P) * ECG_MAX_K];
	ecg_mm_params_t *prm;
	hipStream_t st;
	uint32_t kid = 0;
	int rc, e, r, j, bytewise;

	if (k < 1 || k > ECG_KMAX_K || p < 1 || p > ECG_KMAX_R)
		return ecg_fail(-ECG_DER_INVAL, "update_masks: k=%d p=%d outside the limits k <= %d, p <= %d", k, p,
				ECG_KMAX_K, ECG_KMAX_R);
	if (flags & ~(ECG_RM_SPARSE | ECG_UM_PACKED))
		return ecg_fail(-ECG_DER_INVAL, "update_masks: unknown flags 0x%x", flags);
	if (masks == NULL || (uintptr_t)masks % 4u)
		return ecg_fail(-ECG_DER_INVAL, "update_masks: masks must be 4-byte aligned device memory");
	if (result == NULL || (uintptr_t)result % 8u)
		return ecg_fail(-ECG_DER_INVAL, "update_masks: result must be 8-byte aligned device memory");
	if (old_cells == NULL)
		return ecg_fail(-ECG_DER_INVAL, "update_masks: NULL old_cells");
	if (new_cells == NULL)
		return ecg_fail(-ECG_DER_INVAL, "update_masks: NULL new_cells");
	if (parity == NULL)
		return ecg_fail(-ECG_DER_INVAL, "update_masks: NULL parity");
	/* the kernel reads mask words and counts into result while other blocks
	 * write parity cells */
	if (S && C && ecg_cells_overlap(masks, 4ull * S, parity, S, parity_stripe_stride, p, parity_cell_stride, C))
		return ecg_fail(-ECG_DER_INVAL, "update_masks: masks overlaps the parity");
	if (S && C && ecg_cells_overlap(result, 32, parity, S, parity_stripe_stride, p, parity_cell_stride, C))
		return ecg_fail(-ECG_DER_INVAL, "update_masks: result overlaps the parity");
	if (ctx == NULL)
		return ecg_fail(-ECG_DER_INVAL, "update_masks: NULL context");
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);

	/* nothing updated, no invalid mask */
	rc = ecg_result_reset(result, st, "update_masks memset");
	if (rc || S == 0 || C == 0)
		return rc;

	prm = calloc(1, sizeof(*prm));
	if (prm == NULL)
		return ecg_fail(-ECG_DER_NOMEM, "update_masks: calloc");
	prm->src = old_cells;
	prm->src2 = new_cells;
	prm->dst = parity;
	prm->src_stripe_stride = upd_stripe_stride;
	prm->src2_stripe_stride = upd_stripe_stride;
	prm->dst_stripe_stride = parity_stripe_stride;
	prm->cell_bytes = C;
	prm->nstripes = S;
	prm->k = (uint32_t)k;
	prm->rows = (uint32_t)p;
	prm->accumulate = 1;
	prm->diff = 1;
	/* the parity rows of every column: a stripe's mask picks among them */
	ecg_gf_init();
	ecg_gen_cauchy1(k, p, en);
	for (r = 0; r < p; r++) {
		prm->dst_cell_off[r] = (int64_t)r * parity_cell_stride;
		for (j = 0; j < k; j++)
			ecg_build_ptbl(en[(k + r) * k + j], &prm->tbl[r][j]);
	}
	bytewise = ctx->cfg.variant == 2 ||
		   ((uintptr_t)old_cells | (uintptr_t)new_cells | (uintptr_t)parity | (uint64_t)upd_stripe_stride |
		    (uint64_t)parity_cell_stride | (uint64_t)parity_stripe_stride | C) % 16u;

	ecg_trace_push("ecg:update_masks");
	e = ecg_k_launch_update_masks(prm, masks, (uint64_t *)result, (flags & ECG_UM_PACKED) != 0, bytewise,
				      (flags & ECG_RM_SPARSE) != 0, &ctx->cfg, (void *)st, &kid);
	free(prm);
	/* update_cells / update_bytes stay: the count is known on the device only */
	return ecg_launch_done(ctx, e, "update_masks kernel launch", 1, ecg_k_update_masks_kernel_name(kid));
}
