/*
 * ecg_update_masks.c -- aggregation delta parity update with one set of
 * updated cells per stripe (include/ecg.h ecg_update_masks,
 * ecg_update_masks_ptrs).
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
 *
 * ecg_update_masks_ptrs is the same launch for stripes that are not three
 * strided images: a host table of 2k + p cell addresses per stripe (old, new,
 * parity), staged through the one path of the cell-table calls
 * (ecg_internal.h ecg_staged_open / _upload / _close), and the cell-table
 * kernels of the same file.  A table that is three strided images after all
 * is handed to ecg_update_masks.  The two calls share the argument check, the
 * launch helper and its ecg_launch_done; so do their _csum composites and
 * ecg_csum_updated_ptrs (ecg_csum.c), through ecg_internal.h.
 *
 * ecg_agg_masks / ecg_agg_masks_ptrs are the same two calls with a route per
 * stripe: the delta update for a stripe that names few cells, a re-encode of
 * the merged stripe for one that names more than `recalc_above` (ecg_kabi.h
 * ecg_agg_route; the ecg_agg_masks* kernels of the same file).  They take the
 * same checks, widened by the threshold, and the same launch helper.
 */
#include <stdlib.h>
#include <string.h>

#include "ecg_internal.h"

/* The argument checks of both calls in their documented order (fn names the
 * caller in the message; have_ctx = 0 fails where they report a NULL context).
 * strided = 1: ecg_update_masks, whose operands are checked before the
 * context; 0: ecg_update_masks_ptrs, whose table is checked after it (`cells`;
 * its entries by ecg_staged_open) and which has no packed form. */
int ecg_um_check(const char *fn, int strided, int have_ctx, int k, int p, uint64_t C, uint32_t S,
		 const void *old_cells, const void *new_cells, const void *parity, int64_t parity_cell_stride,
		 int64_t parity_stripe_stride, const void *cells, const uint32_t *masks, const void *result,
		 unsigned flags, uint32_t *recalc_above)
{
	if (k < 1 || k > ECG_KMAX_K || p < 1 || p > ECG_KMAX_R)
		return ecg_fail(-ECG_DER_INVAL, "%s: k=%d p=%d outside the limits k <= %d, p <= %d", fn, k, p,
				ECG_KMAX_K, ECG_KMAX_R);
	if (flags & ~(ECG_RM_SPARSE | ECG_UM_PACKED))
		return ecg_fail(-ECG_DER_INVAL, "%s: unknown flags 0x%x", fn, flags);
	if (!strided && (flags & ECG_UM_PACKED))
		return ecg_fail(-ECG_DER_INVAL, "%s: ECG_UM_PACKED has no meaning over a cell table (slot j holds "
				"the address of cell j)", fn);
	if (recalc_above != NULL) {
		if (flags & ECG_UM_PACKED)
			return ecg_fail(-ECG_DER_INVAL, "%s: ECG_UM_PACKED is refused (a re-encoded stripe needs the "
					"unnamed old cells in their slots)", fn);
		if (*recalc_above == ECG_AGG_AUTO)
			*recalc_above = (uint32_t)ecg_agg_threshold(k, p);
		else if (*recalc_above > (uint32_t)k)
			return ecg_fail(-ECG_DER_INVAL, "%s: recalc_above=%u is neither 0 .. k=%d nor ECG_AGG_AUTO", fn,
					*recalc_above, k);
	}
	if (masks == NULL || (uintptr_t)masks % 4u)
		return ecg_fail(-ECG_DER_INVAL, "%s: masks must be 4-byte aligned device memory", fn);
	if (result == NULL || (uintptr_t)result % 8u)
		return ecg_fail(-ECG_DER_INVAL, "%s: result must be 8-byte aligned device memory", fn);
	if (strided) {
		if (old_cells == NULL)
			return ecg_fail(-ECG_DER_INVAL, "%s: NULL old_cells", fn);
		if (new_cells == NULL)
			return ecg_fail(-ECG_DER_INVAL, "%s: NULL new_cells", fn);
		if (parity == NULL)
			return ecg_fail(-ECG_DER_INVAL, "%s: NULL parity", fn);
		/* the kernel reads mask words and counts into result while other
		 * blocks write parity cells */
		if (S && C &&
		    ecg_cells_overlap(masks, 4ull * S, parity, S, parity_stripe_stride, p, parity_cell_stride, C))
			return ecg_fail(-ECG_DER_INVAL, "%s: masks overlaps the parity", fn);
		if (S && C && ecg_cells_overlap(result, 32, parity, S, parity_stripe_stride, p, parity_cell_stride, C))
			return ecg_fail(-ECG_DER_INVAL, "%s: result overlaps the parity", fn);
	}
	if (!have_ctx)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL context", fn);
	if (!strided && S && C && cells == NULL)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL cells", fn);
	return 0;
}

/* The launch of all four calls: agg = 0 the update with its flags, 1
 * ecg_agg_masks / _ptrs with the effective threshold T. */
static int um_launch(ecg_ctx_t *ctx, const char *fn, int agg, uint32_t T, int k, int p, uint64_t C, uint32_t S,
		     const void *old_cells, const void *new_cells, int64_t upd_stripe_stride, void *parity,
		     int64_t parity_cell_stride, int64_t parity_stripe_stride, const uint64_t *cells_dev, int bytewise,
		     const uint32_t *masks, void *result, unsigned flags, hipStream_t st)
{
	unsigned char en[(ECG_MAX_K + ECG_MAX_P) * ECG_MAX_K];
	const int ptrs = cells_dev != NULL;
	ecg_mm_params_t *prm = calloc(1, sizeof(*prm));
	const char *kernel = NULL;
	int e, r, j;

	if (prm == NULL)
		return ecg_fail(-ECG_DER_NOMEM, "%s: calloc", fn);
	if (cells_dev == NULL) {
		prm->src = old_cells;
		prm->src2 = new_cells;
		prm->dst = parity;
		prm->src_stripe_stride = upd_stripe_stride;
		prm->src2_stripe_stride = upd_stripe_stride;
		prm->dst_stripe_stride = parity_stripe_stride;
	}
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
		if (cells_dev == NULL)
			prm->dst_cell_off[r] = (int64_t)r * parity_cell_stride;
		for (j = 0; j < k; j++)
			ecg_build_ptbl(en[(k + r) * k + j], &prm->tbl[r][j]);
	}

	bytewise = ctx->cfg.variant == 2 || bytewise;
	if (agg) {
		ecg_trace_push(ptrs ? "ecg:agg_masks_ptrs" : "ecg:agg_masks");
		e = ecg_k_launch_agg_masks(prm, cells_dev, masks, (uint64_t *)result, T, bytewise,
					   (flags & ECG_RM_SPARSE) != 0, &ctx->cfg, (void *)st, &kernel);
	} else {
		ecg_trace_push(ptrs ? "ecg:update_masks_ptrs" : "ecg:update_masks");
		e = ecg_k_launch_update_masks(prm, cells_dev, masks, (uint64_t *)result, (flags & ECG_UM_PACKED) != 0,
					      bytewise, (flags & ECG_RM_SPARSE) != 0, &ctx->cfg, (void *)st, &kernel);
	}
	free(prm);
	/* update_cells / update_bytes stay: the count is known on the device only */
	return ecg_launch_done(ctx, e, agg ? (ptrs ? "agg_masks_ptrs kernel launch" : "agg_masks kernel launch") :
			       (ptrs ? "update_masks_ptrs kernel launch" : "update_masks kernel launch"), 1, kernel);
}

/* The launch of the update calls (fn names the call in the trace range and
 * the messages): over the three strided images, or with cells_dev over the
 * staged cell table (the strided operands unused). */
int ecg_um_launch(ecg_ctx_t *ctx, const char *fn, int k, int p, uint64_t C, uint32_t S, const void *old_cells,
		  const void *new_cells, int64_t upd_stripe_stride, void *parity, int64_t parity_cell_stride,
		  int64_t parity_stripe_stride, const uint64_t *cells_dev, int bytewise, const uint32_t *masks,
		  void *result, unsigned flags, hipStream_t st)
{
	return um_launch(ctx, fn, 0, 0, k, p, C, S, old_cells, new_cells, upd_stripe_stride, parity, parity_cell_stride,
			 parity_stripe_stride, cells_dev, bytewise, masks, result, flags, st);
}

int ecg_update_masks(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S,
		     const void *old_cells, const void *new_cells, int64_t upd_stripe_stride,
		     void *parity, int64_t parity_cell_stride, int64_t parity_stripe_stride,
		     const uint32_t *masks, void *result, unsigned flags, void *stream)
{
	static const char fn[] = "update_masks";
	hipStream_t st;
	int rc;

	rc = ecg_um_check(fn, 1, ctx != NULL, k, p, C, S, old_cells, new_cells, parity, parity_cell_stride,
		      parity_stripe_stride, NULL, masks, result, flags, NULL);
	if (rc)
		return rc;
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);

	/* nothing updated, no invalid mask */
	rc = ecg_result_reset(result, st, "update_masks memset");
	if (rc || S == 0 || C == 0)
		return rc;
	return ecg_um_launch(ctx, fn, k, p, C, S, old_cells, new_cells, upd_stripe_stride, parity, parity_cell_stride,
			 parity_stripe_stride, NULL,
			 ((uintptr_t)old_cells | (uintptr_t)new_cells | (uintptr_t)parity | (uint64_t)upd_stripe_stride |
			  (uint64_t)parity_cell_stride | (uint64_t)parity_stripe_stride | C) % 16u != 0,
			 masks, result, flags, st);
}

/* Is the parity group of the staged table tab[S][2k + p] strided -- parity
 * (s, r) at p0 + s*ps + r*pc?  *bits = the OR of the parity addresses (the lane
 * choice of a call that reads no other entry).  The strides are differences of
 * addresses and may be negative. */
int ecg_um_parity_group(const uint64_t *tab, int k, int p, uint64_t C, uint32_t S, int64_t *pc, int64_t *ps,
			uint64_t *bits)
{
	const uint32_t n = (uint32_t)(2 * k + p);
	const uint64_t p0 = tab[2 * k];
	const uint64_t c = p > 1 ? tab[2 * k + 1] - p0 : C;
	const uint64_t q = S > 1 ? tab[n + 2 * k] - p0 : C;
	uint64_t all = 0;
	int aff = 1;

	for (uint64_t s = 0; s < S; s++)
		for (int r = 0; r < p; r++) {
			const uint64_t a = tab[s * n + 2 * (uint64_t)k + r];

			aff &= a == p0 + s * q + (uint64_t)r * c;
			all |= a;
		}
	*pc = (int64_t)c;
	*ps = (int64_t)q;
	*bits = all;
	return aff;
}

/* Is the staged table tab[S][2k + p] three strided groups -- old cell (s, j)
 * at o0 + s*us + j*C, new cell (s, j) at n0 + s*us + j*C with the same us,
 * parity (s, r) at p0 + s*ps + r*pc?  One stripe is, when its cells are spaced
 * so.  The strides are differences of addresses and may be negative. */
int ecg_um_three_groups(const uint64_t *tab, int k, int p, uint64_t C, uint32_t S, int64_t *us, int64_t *pc,
			int64_t *ps)
{
	const uint32_t n = (uint32_t)(2 * k + p);
	const uint64_t o0 = tab[0], n0 = tab[k];
	const uint64_t u = S > 1 ? tab[n] - o0 : (uint64_t)k * C;
	uint64_t bits;
	int aff = ecg_um_parity_group(tab, k, p, C, S, pc, ps, &bits);

	for (uint64_t s = 0; s < S; s++) {
		const uint64_t *row = tab + s * n;

		for (int j = 0; j < k; j++) {
			aff &= row[j] == o0 + s * u + (uint64_t)j * C;
			aff &= row[k + j] == n0 + s * u + (uint64_t)j * C;
		}
	}
	*us = (int64_t)u;
	return aff;
}

int ecg_update_masks_ptrs(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S, void *const *cells,
			  const uint32_t *masks, void *result, unsigned flags, void *stream)
{
	static const char fn[] = "update_masks_ptrs";
	/* the kernel reads mask words and counts into result while other blocks
	 * write parity cells */
	const struct ecg_clear clear[2] = {{masks, 4ull * S, "masks"}, {result, 32, "result"}};
	struct ecg_staged t;
	int64_t us, pc, ps;
	hipStream_t st;
	int rc;

	rc = ecg_um_check(fn, 0, ctx != NULL, k, p, C, S, NULL, NULL, NULL, 0, 0, cells, masks, result, flags, NULL);
	if (rc)
		return rc;
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);
	if (S == 0 || C == 0)	/* nothing updated, no invalid mask */
		return ecg_result_reset(result, st, "update_masks_ptrs memset");

	rc = ecg_staged_open(ctx, fn, cells, S, (uint32_t)(2 * k + p), C, clear, 2, &t);
	if (rc)
		return rc;
	/* ecg_update_masks's own layout (and masks and result clear of the whole
	 * parity span, gaps included, as it demands): its launch, with no table
	 * and no dependent address loads */
	if (ecg_um_three_groups(t.sc->pin, k, p, C, S, &us, &pc, &ps) &&
	    !ecg_cells_overlap(masks, 4ull * S, cells[2 * k], S, ps, p, pc, C) &&
	    !ecg_cells_overlap(result, 32, cells[2 * k], S, ps, p, pc, C)) {
		ecg_staged_close(ctx, &t, st, 0);
		return ecg_update_masks(ctx, k, p, C, S, cells[0], cells[k], us, cells[2 * k], pc, ps, masks, result,
					flags, stream);
	}
	rc = ecg_staged_upload(&t, result, st, "update_masks_ptrs memset", "update_masks_ptrs cell table");
	if (rc == 0)
		rc = ecg_um_launch(ctx, fn, k, p, C, S, NULL, NULL, 0, NULL, 0, 0, t.sc->dev, (t.bits | C) % 16u != 0, masks,
			       result, flags, st);
	return ecg_staged_close(ctx, &t, st, rc);
}

int ecg_agg_threshold(int k, int p)
{
	if (k < 1 || k > ECG_KMAX_K || p < 1 || p > ECG_KMAX_R)
		return ecg_fail(-ECG_DER_INVAL, "agg_threshold: k=%d p=%d outside the limits k <= %d, p <= %d", k, p,
				ECG_KMAX_K, ECG_KMAX_R);
	/* delta (2n + 2p) C against re-encode (k + p) C; the tie goes to the delta */
	return k > p ? (k - p) / 2 : 0;
}

int ecg_agg_masks(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S,
		  const void *old_cells, const void *new_cells, int64_t upd_stripe_stride,
		  void *parity, int64_t parity_cell_stride, int64_t parity_stripe_stride,
		  const uint32_t *masks, void *result, uint32_t recalc_above, unsigned flags, void *stream)
{
	static const char fn[] = "agg_masks";
	hipStream_t st;
	int rc;

	rc = ecg_um_check(fn, 1, ctx != NULL, k, p, C, S, old_cells, new_cells, parity, parity_cell_stride,
			  parity_stripe_stride, NULL, masks, result, flags, &recalc_above);
	if (rc)
		return rc;
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);

	/* nothing updated, no invalid mask */
	rc = ecg_result_reset(result, st, "agg_masks memset");
	if (rc || S == 0 || C == 0)
		return rc;
	return um_launch(ctx, fn, 1, recalc_above, k, p, C, S, old_cells, new_cells, upd_stripe_stride, parity,
			 parity_cell_stride, parity_stripe_stride, NULL,
			 ((uintptr_t)old_cells | (uintptr_t)new_cells | (uintptr_t)parity | (uint64_t)upd_stripe_stride |
			  (uint64_t)parity_cell_stride | (uint64_t)parity_stripe_stride | C) % 16u != 0,
			 masks, result, flags, st);
}

int ecg_agg_masks_ptrs(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S, void *const *cells,
		       const uint32_t *masks, void *result, uint32_t recalc_above, unsigned flags, void *stream)
{
	static const char fn[] = "agg_masks_ptrs";
	const struct ecg_clear clear[2] = {{masks, 4ull * S, "masks"}, {result, 32, "result"}};
	struct ecg_staged t;
	int64_t us, pc, ps;
	hipStream_t st;
	int rc;

	rc = ecg_um_check(fn, 0, ctx != NULL, k, p, C, S, NULL, NULL, NULL, 0, 0, cells, masks, result, flags,
			  &recalc_above);
	if (rc)
		return rc;
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);
	if (S == 0 || C == 0)	/* nothing updated, no invalid mask */
		return ecg_result_reset(result, st, "agg_masks_ptrs memset");

	rc = ecg_staged_open(ctx, fn, cells, S, (uint32_t)(2 * k + p), C, clear, 2, &t);
	if (rc)
		return rc;
	/* ecg_agg_masks's own layout, as ecg_update_masks_ptrs finds
	 * ecg_update_masks's: its launch, with no table */
	if (ecg_um_three_groups(t.sc->pin, k, p, C, S, &us, &pc, &ps) &&
	    !ecg_cells_overlap(masks, 4ull * S, cells[2 * k], S, ps, p, pc, C) &&
	    !ecg_cells_overlap(result, 32, cells[2 * k], S, ps, p, pc, C)) {
		ecg_staged_close(ctx, &t, st, 0);
		return ecg_agg_masks(ctx, k, p, C, S, cells[0], cells[k], us, cells[2 * k], pc, ps, masks, result,
				     recalc_above, flags, stream);
	}
	rc = ecg_staged_upload(&t, result, st, "agg_masks_ptrs memset", "agg_masks_ptrs cell table");
	if (rc == 0)
		rc = um_launch(ctx, fn, 1, recalc_above, k, p, C, S, NULL, NULL, 0, NULL, 0, 0, t.sc->dev,
			       (t.bits | C) % 16u != 0, masks, result, flags, st);
	return ecg_staged_close(ctx, &t, st, rc);
}
