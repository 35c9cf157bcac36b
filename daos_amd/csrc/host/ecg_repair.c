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
 */
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

int ecg_repair(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S,
	       void *data, int64_t data_stripe_stride,
	       void *parity, int64_t parity_cell_stride, int64_t parity_stripe_stride,
	       const uint32_t *status, void *result, void *stream)
{
	const int kp[2] = {k, p};
	const void *rowtbl = NULL;
	ecg_mm_params_t *prm;
	hipStream_t st;
	uint32_t kid = 0;
	int rc, e, r, j, bytewise;

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

	/* the row tables of (k, p): synchronous on first use */
	rc = ecg_ctx_kp_table(ctx, &ctx->repair_tbl[k - 1][p - 1], (size_t)(k + p) * k * sizeof(ecg_ptbl_t), build_rows,
			      kp, "repair tables", &rowtbl);
	if (rc)
		return rc;
	prm = calloc(1, sizeof(*prm));
	if (prm == NULL)
		return ecg_fail(-ECG_DER_NOMEM, "repair: calloc");
	/* the operands of ecg_verify: data cells as sources, parity rows in the
	 * destination slot; which of them a stripe reads and which one it
	 * writes is the kernel's choice per stripe */
	prm->src = data;
	prm->dst = parity;
	prm->src_stripe_stride = data_stripe_stride;
	prm->dst_stripe_stride = parity_stripe_stride;
	prm->cell_bytes = C;
	prm->nstripes = S;
	prm->k = (uint32_t)k;
	prm->rows = (uint32_t)p;
	for (j = 0; j < k; j++)
		prm->src_cell_off[j] = (int64_t)j * (int64_t)C;
	for (r = 0; r < p; r++)
		prm->dst_cell_off[r] = (int64_t)r * parity_cell_stride;
	bytewise = ctx->cfg.variant == 2 || ecg_k_align_granule(prm) != 16u || C % 16u;

	ecg_trace_push("ecg:repair");
	e = ecg_k_launch_repair(prm, rowtbl, status, (uint64_t *)result, bytewise, &ctx->cfg, (void *)st, &kid);
	free(prm);
	return ecg_launch_done(ctx, e, "repair kernel launch", 1, ecg_k_repair_kernel_name(kid));
}
