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

/* Device copy of the (k + p) x k row tables, built once per (k, p) and
 * context (ctx->lock); synchronous on first use. */
static int repair_tables(ecg_ctx_t *ctx, int k, int p, const ecg_ptbl_t **out)
{
	int rc = 0;

	pthread_mutex_lock(&ctx->lock);
	if (ctx->repair_tbl[k - 1][p - 1] == NULL) {
		const size_t bytes = (size_t)(k + p) * k * sizeof(ecg_ptbl_t);
		ecg_ptbl_t *img = malloc(bytes);
		void *dev = NULL;
		hipError_t e;

		if (img == NULL) {
			rc = ecg_fail(-ECG_DER_NOMEM, "repair tables");
		} else {
			unsigned char coef[ECG_KMAX_K];
			uint32_t idx[ECG_KMAX_K];

			for (int c = 0; c < k + p && rc == 0; c++) {
				rc = ecg_repair_row(k, p, c, coef, idx);
				for (int j = 0; j < k && rc == 0; j++)
					ecg_build_ptbl(coef[j], &img[c * k + j]);
			}
			if (rc == 0) {
				e = hipMalloc(&dev, bytes);
				if (e == hipSuccess)
					e = hipMemcpy(dev, img, bytes, hipMemcpyHostToDevice);
				if (e != hipSuccess) {
					if (dev)
						(void)hipFree(dev);
					rc = ecg_hip_fail(e, "repair tables");
				} else {
					ctx->repair_tbl[k - 1][p - 1] = dev;
				}
			}
			free(img);
		}
	}
	*out = ctx->repair_tbl[k - 1][p - 1];
	pthread_mutex_unlock(&ctx->lock);
	return rc;
}

void ecg_repair_ctx_fini(ecg_ctx_t *ctx)
{
	for (int k = 0; k < ECG_KMAX_K; k++)
		for (int p = 0; p < ECG_KMAX_R; p++)
			if (ctx->repair_tbl[k][p]) {
				(void)hipFree(ctx->repair_tbl[k][p]);
				ctx->repair_tbl[k][p] = NULL;
			}
}

/* Does [a, a + alen) meet the cells base + i*si + j*sj, i < ni, j < nj, each
 * len bytes long?  (Their bounding range: strides may be negative.) */
int ecg_cells_overlap(const void *a, uint64_t alen, const void *base, int64_t ni, int64_t si, int64_t nj,
			int64_t sj, uint64_t len)
{
	const int64_t ei = (ni - 1) * si, ej = (nj - 1) * sj;
	const int64_t lo = (ei < 0 ? ei : 0) + (ej < 0 ? ej : 0);
	const int64_t hi = (ei > 0 ? ei : 0) + (ej > 0 ? ej : 0);
	const uintptr_t b0 = (uintptr_t)base + (uintptr_t)lo, b1 = (uintptr_t)base + (uintptr_t)hi + len;
	const uintptr_t a0 = (uintptr_t)a, a1 = a0 + alen;

	return a0 < b1 && b0 < a1;
}

int ecg_repair(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S,
	       void *data, int64_t data_stripe_stride,
	       void *parity, int64_t parity_cell_stride, int64_t parity_stripe_stride,
	       const uint32_t *status, void *result, void *stream)
{
	const ecg_ptbl_t *rowtbl = NULL;
	ecg_mm_params_t *prm;
	hipStream_t st;
	hipError_t he;
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

	/* result = {0, UINT64_MAX, 0, 0}: nothing repaired, nothing left */
	he = hipMemsetAsync(result, 0, 32, st);
	if (he == hipSuccess)
		he = hipMemsetAsync((uint8_t *)result + 8, 0xFF, 8, st);
	if (he != hipSuccess)
		return ecg_hip_fail(he, "repair memset");
	if (S == 0 || C == 0)
		return 0;

	rc = repair_tables(ctx, k, p, &rowtbl);
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
	ecg_trace_pop();
	free(prm);
	if (e != 0)
		return ecg_hip_fail((hipError_t)e, "repair kernel launch");
	ECG_STAT_ADD(ctx, launches, 1);
	ecg_set_last_kernel(ecg_k_repair_kernel_name(kid));
	return 0;
}
