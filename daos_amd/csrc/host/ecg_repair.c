/*
 * ecg_repair.c -- rewrite the cell ecg_verify located, on the device
 * (include/ecg.h ecg_repair / ecg_repair_row).
 *
 * What it replaces: after a scrub every bad stripe names a different cell,
 * and ecg_recover takes one err_list for a whole batch -- so the caller drains
 * the stream, downloads the status words, classifies them on the host and
 * issues one ecg_recover per bad stripe.  Here the status words stay on the
 * device: one launch queued behind the verify reads them, and each block
 * chooses its decode row and operand set per stripe
 * (kernels/ecg_repair_kernels.hip).
 *
 * The rows: for a parity cell the Cauchy1 row over the k data cells; for data
 * cell c the decode row of erasure {c} -- the survivors ecg_recover picks (the
 * other k-1 data cells and parity row 0), written with parity row 0 in slot c
 * so that slot i != c still reads data cell i.  From
 *   parity0 = XOR_i g[0][i] * data[i]
 * follows  data[c] = 1/g[0][c] * parity0  ^  XOR_{i != c} g[0][i]/g[0][c] * data[i].
 * The (k + p) x k rows become perm tables once per (k, p) and context, in a
 * device buffer (7.5 KiB at most: too large for kernel arguments next to
 * ecg_mm_params_t).
 *
 * ecg_repair_ptrs is the same launch for stripes that are not one strided
 * image (a host table of cell addresses, the cell-table kernels of the same
 * file; a table that is a strided image after all is handed to ecg_repair),
 * and ecg_scrub_ptrs the whole scrub over one such table: checked and staged
 * once, the verify, its summary and the repair queued behind one upload.  The
 * set-up they share with the strided calls is in ecg_verify.c
 * (ecg_scrub_params, ecg_scrub_strided, ecg_verify_preset, ecg_verify_launch).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ecg_internal.h"

int ecg_repair_row(int k, int p, int cell, unsigned char *coef, uint32_t *src_idx)
{
	unsigned char en[(ECG_KMAX_K + ECG_KMAX_R) * ECG_KMAX_K];
	unsigned char inv;
	int i;

	if (k < 1 || k > ECG_KMAX_K || p < 1 || p > ECG_KMAX_R)
		return ecg_fail(-ECG_DER_INVAL, "repair_row: k=%d p=%d outside 1..%d / 1..%d", k, p, ECG_KMAX_K,
				ECG_KMAX_R);
	if (cell < 0 || cell >= k + p)
		return ecg_fail(-ECG_DER_INVAL, "repair_row: cell %d outside 0..%d", cell, k + p - 1);
	if (coef == NULL || src_idx == NULL)
		return ecg_fail(-ECG_DER_INVAL, "repair_row: NULL argument");
	ecg_gf_init();
	ecg_gen_cauchy1(k, p, en);
	if (cell >= k) {
		for (i = 0; i < k; i++) {
			coef[i] = en[cell * k + i];
			src_idx[i] = (uint32_t)i;
		}
		return 0;
	}
	inv = ecg_gf_inv(en[k * k + cell]);	/* Cauchy1 entries are never zero */
	for (i = 0; i < k; i++) {
		coef[i] = i == cell ? inv : ecg_gf_mul_tbl[inv][en[k * k + i]];
		src_idx[i] = i == cell ? (uint32_t)k : (uint32_t)i;
	}
	return 0;
}

/* Host image of the (k + p) x k row tables (ecg_ctx_kp_table's build). */
static int build_rows(void *img, const void *arg)
{
	const int k = ((const int *)arg)[0], p = ((const int *)arg)[1];
	unsigned char coef[ECG_KMAX_K];
	uint32_t idx[ECG_KMAX_K];
	int rc = 0;

	for (int c = 0; c < k + p && rc == 0; c++) {
		rc = ecg_repair_row(k, p, c, coef, idx);
		for (int j = 0; j < k && rc == 0; j++)
			ecg_build_ptbl(coef[j], (ecg_ptbl_t *)img + c * k + j);
	}
	return rc;
}

/* The row tables of (k, p), one per context: synchronous on first use.  Takes
 * ctx->lock, so the cell-table calls fetch it before they lock their slot. */
static int repair_rowtbl(ecg_ctx_t *ctx, int k, int p, const void **rowtbl)
{
	const int kp[2] = {k, p};

	return ecg_ctx_kp_table(ctx, &ctx->repair_tbl[k - 1][p - 1], (size_t)(k + p) * k * sizeof(ecg_ptbl_t), build_rows,
				kp, "repair tables", rowtbl);
}

/* The launch of every repair call (fn names it in the trace range and the
 * messages): over prm's strided operands, or with cells_dev over a staged cell
 * table. */
static int repair_launch(ecg_ctx_t *ctx, const char *fn, const ecg_mm_params_t *prm, const void *rowtbl,
			 const uint64_t *cells_dev, int bytewise, const uint32_t *status, void *result, hipStream_t st)
{
	char what[48];
	const char *kernel = NULL;
	int e;

	snprintf(what, sizeof(what), "ecg:%s", fn);
	ecg_trace_push(what);
	e = ecg_k_launch_repair(prm, rowtbl, cells_dev, status, (uint64_t *)result, ctx->cfg.variant == 2 || bytewise,
				&ctx->cfg, (void *)st, &kernel);
	snprintf(what, sizeof(what), "%s kernel launch", fn);
	return ecg_launch_done(ctx, e, what, 1, kernel);
}

int ecg_repair(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S,
	       void *data, int64_t data_stripe_stride,
	       void *parity, int64_t parity_cell_stride, int64_t parity_stripe_stride,
	       const uint32_t *status, void *result, void *stream)
{
	const void *rowtbl = NULL;
	ecg_mm_params_t *prm;
	hipStream_t st;
	int rc;

	if (ctx == NULL)
		return ecg_fail(-ECG_DER_INVAL, "repair: NULL context");
	if (k < 1 || k > ECG_KMAX_K || p < 1 || p > ECG_KMAX_R)
		return ecg_fail(-ECG_DER_INVAL, "repair: k=%d p=%d outside 1..%d / 1..%d", k, p, ECG_KMAX_K,
				ECG_KMAX_R);
	if (result == NULL || (uintptr_t)result % 8u)
		return ecg_fail(-ECG_DER_INVAL, "repair: result must be 8-byte aligned device memory");
	if (S && (status == NULL || (uintptr_t)status % 4u))
		return ecg_fail(-ECG_DER_INVAL, "repair: status must be 4-byte aligned device memory");
	if (S && C && (data == NULL || parity == NULL))
		return ecg_fail(-ECG_DER_INVAL, "repair: NULL cells");
	/* the kernel reads status words while other blocks write cells */
	if (S && C &&
	    (ecg_cells_overlap(status, 4ull * S, data, S, data_stripe_stride, k, (int64_t)C, C) ||
	     ecg_cells_overlap(status, 4ull * S, parity, S, parity_stripe_stride, p, parity_cell_stride, C)))
		return ecg_fail(-ECG_DER_INVAL, "repair: status overlaps the data or parity cells");
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);

	/* nothing repaired, nothing left */
	rc = ecg_result_reset(result, st, "repair memset");
	if (rc || S == 0 || C == 0)
		return rc;

	rc = repair_rowtbl(ctx, k, p, &rowtbl);
	if (rc == 0)
		rc = ecg_scrub_params("repair", k, p, C, S, 0, &prm);
	if (rc)
		return rc;
	/* the operands of ecg_verify: data cells as sources, parity rows in the
	 * destination slot; which of them a stripe reads and which one it
	 * writes is the kernel's choice per stripe */
	ecg_scrub_strided(prm, data, data_stripe_stride, parity, parity_cell_stride, parity_stripe_stride);
	rc = repair_launch(ctx, "repair", prm, rowtbl, NULL, ecg_k_align_granule(prm) != 16u || C % 16u, status, result,
			   st);
	free(prm);
	return rc;
}

/* Is the staged table one strided image [S][k+p][C] whose arguments pass
 * ecg_repair's own checks (status clear of the whole image, gaps included)? */
static int repair_affine(const struct ecg_staged *t, void *const *cells, int k, int p, uint64_t C, uint32_t S,
			 const uint32_t *status)
{
	return t->affine && !ecg_cells_overlap(status, 4ull * S, cells[0], S, t->stride, k + p, (int64_t)C, C);
}

int ecg_repair_ptrs(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S, void *const *cells, const uint32_t *status,
		    void *result, void *stream)
{
	static const char fn[] = "repair_ptrs";
	/* the kernel reads status words and counts into result while other
	 * blocks write cells */
	const struct ecg_clear clear[2] = {{status, 4ull * S, "status"}, {result, 32, "result"}};
	const void *rowtbl = NULL;
	ecg_mm_params_t *prm;
	struct ecg_staged t;
	hipStream_t st;
	int rc;

	rc = ecg_scrub_ptrs_check(fn, ctx != NULL, k, p, C, S, cells, status, result, NULL);
	if (rc)
		return rc;
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);
	if (S == 0 || C == 0)	/* nothing repaired, nothing left */
		return ecg_result_reset(result, st, "repair_ptrs memset");

	rc = repair_rowtbl(ctx, k, p, &rowtbl);	/* takes the lock: before open */
	if (rc == 0)
		rc = ecg_staged_open(ctx, fn, cells, S, (uint32_t)(k + p), C, clear, 2, &t);
	if (rc)
		return rc;
	/* ecg_repair's own layout: its launch, with no table and no dependent
	 * address loads */
	if (repair_affine(&t, cells, k, p, C, S, status)) {
		ecg_staged_close(ctx, &t, st, 0);
		return ecg_repair(ctx, k, p, C, S, cells[0], t.stride, (uint8_t *)cells[0] + (uint64_t)k * C, (int64_t)C,
				  t.stride, status, result, stream);
	}
	rc = ecg_scrub_params(fn, k, p, C, S, 0, &prm);
	if (rc)
		return ecg_staged_close(ctx, &t, st, rc);
	rc = ecg_staged_upload(&t, result, st, "repair_ptrs memset", "repair_ptrs cell table");
	if (rc == 0)
		rc = repair_launch(ctx, fn, prm, rowtbl, t.sc->dev, (t.bits | C) % 16u != 0, status, result, st);
	free(prm);
	return ecg_staged_close(ctx, &t, st, rc);
}

int ecg_scrub_ptrs(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S, void *const *cells, uint32_t *status,
		   void *verify_result, void *repair_result, void *stream)
{
	static const char fn[] = "scrub_ptrs";
	const struct ecg_clear clear[3] = {{status, 4ull * S, "status"},
					   {verify_result, 32, "verify_result"},
					   {repair_result, 32, "repair_result"}};
	const void *rr = repair_result;
	const void *rowtbl = NULL;
	ecg_mm_params_t *prm;
	struct ecg_staged t;
	hipStream_t st;
	int rc, bytewise;

	rc = ecg_scrub_ptrs_check(fn, ctx != NULL, k, p, C, S, cells, status, verify_result, &rr);
	if (rc)
		return rc;
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);
	if (S == 0 || C == 0) {	/* the empty batches of both calls */
		rc = ecg_verify_preset(fn, k, S, status, verify_result, st);
		return rc ? rc : ecg_result_reset(repair_result, st, "scrub_ptrs memset");
	}

	rc = repair_rowtbl(ctx, k, p, &rowtbl);	/* takes the lock: before open */
	if (rc == 0)
		rc = ecg_staged_open(ctx, fn, cells, S, (uint32_t)(k + p), C, clear, 3, &t);
	if (rc)
		return rc;
	/* the strided calls' own layout, for both halves or for neither */
	if (repair_affine(&t, cells, k, p, C, S, status)) {
		void *par = (uint8_t *)cells[0] + (uint64_t)k * C;

		ecg_staged_close(ctx, &t, st, 0);
		rc = ecg_verify(ctx, k, p, C, S, cells[0], t.stride, par, (int64_t)C, t.stride, status, verify_result,
				stream);
		return rc ? rc : ecg_repair(ctx, k, p, C, S, cells[0], t.stride, par, (int64_t)C, t.stride, status,
					    repair_result, stream);
	}
	/* one table, one upload; verify, summary and repair queued behind it
	 * (the repair reads no tables from prm: the verify's serve both) */
	rc = ecg_scrub_params(fn, k, p, C, S, 1, &prm);
	if (rc)
		return ecg_staged_close(ctx, &t, st, rc);
	bytewise = (t.bits | C) % 16u != 0;
	rc = ecg_verify_preset(fn, k, S, status, verify_result, st);
	if (rc == 0)
		rc = ecg_staged_upload(&t, repair_result, st, "scrub_ptrs memset", "scrub_ptrs cell table");
	if (rc == 0)
		rc = ecg_verify_launch(ctx, fn, prm, t.sc->dev, bytewise, status, verify_result, st);
	if (rc == 0)
		rc = repair_launch(ctx, fn, prm, rowtbl, t.sc->dev, bytewise, status, repair_result, st);
	free(prm);
	return ecg_staged_close(ctx, &t, st, rc);
}
