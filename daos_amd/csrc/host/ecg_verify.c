/*
 * ecg_verify.c -- parity consistency check with bad-cell location
 * (include/ecg.h ecg_verify / ecg_verify_cell).
 *
 * What it replaces: the EC branch of the object verify path and every
 * consistency pass of a rebuild or aggregation test re-encode the stripe into
 * scratch parity (obj_ec_encode_buf) and memcmp it with the stored one
 * (ref:src/object/obj_verify.c).  Here one read-only launch leaves the
 * syndrome in registers, a status word per stripe says which parity rows
 * differ and which single data cell would explain it
 * (kernels/ecg_verify_kernels.hip), and a summary kernel folds the words into
 * 32 bytes.
 *
 * ecg_verify_ptrs is the same pass for stripes that are not one strided image:
 * a host table of cell addresses, staged as every cell-table call stages its
 * own (ecg_internal.h ecg_staged_open), and the cell-table kernels of the same
 * file.  A table that is a strided image after all is handed to ecg_verify.
 * What the two layouts share is here once: the launch parameters
 * (ecg_scrub_params), the presets (ecg_verify_preset) and the two launches
 * (ecg_verify_launch); ecg_repair.c uses them for ecg_repair_ptrs and
 * ecg_scrub_ptrs.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ecg_internal.h"

int ecg_verify_cell(uint32_t status, int k, int p)
{
	if (k < 1 || k > ECG_KMAX_K || p < 1 || p > ECG_KMAX_R)
		return -2;
	return ecg_verify_classify(status, k, p);
}

/* The launch parameters strided and cell-table calls share: shape, and with
 * `rows` the Cauchy parity rows as perm tables (ecg_verify; ecg_repair reads its
 * rows from the device table and passes 0).  The operands are the caller's. */
int ecg_scrub_params(const char *fn, int k, int p, uint64_t C, uint32_t S, int rows, ecg_mm_params_t **out)
{
	unsigned char en[(ECG_MAX_K + ECG_MAX_P) * ECG_MAX_K];
	ecg_mm_params_t *prm = calloc(1, sizeof(*prm));

	if (prm == NULL)
		return ecg_fail(-ECG_DER_NOMEM, "%s: calloc", fn);
	prm->cell_bytes = C;
	prm->nstripes = S;
	prm->k = (uint32_t)k;
	prm->rows = (uint32_t)p;
	if (rows) {
		ecg_gf_init();
		ecg_gen_cauchy1(k, p, en);
		prm->accumulate = 1;
		for (int r = 0; r < p; r++)
			for (int j = 0; j < k; j++)
				ecg_build_ptbl(en[(size_t)(k + r) * k + j], &prm->tbl[r][j]);
	}
	*out = prm;
	return 0;
}

/* The strided operands of ecg_verify / ecg_repair: the data cells as sources,
 * the parity rows in the product's destination slot. */
void ecg_scrub_strided(ecg_mm_params_t *prm, const void *data, int64_t data_stripe_stride, const void *parity,
		       int64_t parity_cell_stride, int64_t parity_stripe_stride)
{
	prm->src = data;
	prm->dst = (uint8_t *)(uintptr_t)parity;
	prm->src_stripe_stride = data_stripe_stride;
	prm->dst_stripe_stride = parity_stripe_stride;
	for (uint32_t j = 0; j < prm->k; j++)
		prm->src_cell_off[j] = (int64_t)j * (int64_t)prm->cell_bytes;
	for (uint32_t r = 0; r < prm->rows; r++)
		prm->dst_cell_off[r] = (int64_t)r * parity_cell_stride;
}

/* nothing bad; every stripe clean with every data cell still a candidate */
int ecg_verify_preset(const char *fn, int k, uint32_t S, uint32_t *status, void *result, hipStream_t st)
{
	char what[48];
	hipError_t he;
	int rc;

	snprintf(what, sizeof(what), "%s memset", fn);
	rc = ecg_result_reset(result, st, what);
	if (rc || S == 0)
		return rc;
	he = hipMemsetD32Async((hipDeviceptr_t)status, (int)(((1u << k) - 1u) << 8), S, st);
	if (he != hipSuccess) {
		snprintf(what, sizeof(what), "%s status preset", fn);
		return ecg_hip_fail(he, what);
	}
	return 0;
}

/* The syndrome pass and the summary: over prm's strided operands, or with
 * cells_dev over a staged cell table.  The queued launches are counted and
 * the syndrome kernel named (fn: "verify", "verify_ptrs", "scrub_ptrs"). */
int ecg_verify_launch(ecg_ctx_t *ctx, const char *fn, const ecg_mm_params_t *prm, const uint64_t *cells_dev,
		      int bytewise, uint32_t *status, void *result, hipStream_t st)
{
	char what[48];
	const char *kernel = NULL;
	int e;

	snprintf(what, sizeof(what), "ecg:%s", fn);
	ecg_trace_push(what);
	e = ecg_k_launch_verify(prm, cells_dev, status, ctx->cfg.variant == 2 || bytewise, &ctx->cfg, (void *)st,
				&kernel);
	if (e == 0)
		e = ecg_k_launch_verify_summary(status, prm->nstripes, (int)prm->k, (int)prm->rows, (uint64_t *)result,
						(void *)st);
	snprintf(what, sizeof(what), "%s kernel launch", fn);
	return ecg_launch_done(ctx, e, what, 2, kernel);
}

int ecg_verify(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S,
	       const void *data, int64_t data_stripe_stride,
	       const void *parity, int64_t parity_cell_stride, int64_t parity_stripe_stride,
	       uint32_t *status, void *result, void *stream)
{
	ecg_mm_params_t *prm;
	hipStream_t st;
	int rc;

	if (ctx == NULL)
		return ecg_fail(-ECG_DER_INVAL, "verify: NULL context");
	if (k < 1 || k > ECG_KMAX_K || p < 1 || p > ECG_KMAX_R)
		return ecg_fail(-ECG_DER_INVAL, "verify: k=%d p=%d outside 1..%d / 1..%d", k, p, ECG_KMAX_K,
				ECG_KMAX_R);
	if (result == NULL || (uintptr_t)result % 8u)
		return ecg_fail(-ECG_DER_INVAL, "verify: result must be 8-byte aligned device memory");
	if (S && (status == NULL || (uintptr_t)status % 4u))
		return ecg_fail(-ECG_DER_INVAL, "verify: status must be 4-byte aligned device memory");
	if (S && C && (data == NULL || parity == NULL))
		return ecg_fail(-ECG_DER_INVAL, "verify: NULL cells");
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);

	rc = ecg_verify_preset("verify", k, S, status, result, st);
	if (rc || S == 0 || C == 0)
		return rc;

	/* the operands and parity-row tables of ecg_encode, the stored parity
	 * in the product's destination slot (read, never written) */
	rc = ecg_scrub_params("verify", k, p, C, S, 1, &prm);
	if (rc)
		return rc;
	ecg_scrub_strided(prm, data, data_stripe_stride, parity, parity_cell_stride, parity_stripe_stride);
	rc = ecg_verify_launch(ctx, "verify", prm, NULL, ecg_k_align_granule(prm) != 16u || C % 16u, status, result, st);
	free(prm);
	return rc;
}

/* The argument checks of the cell-table scrub calls that need no device, in
 * their documented order (fn names the call; r2: scrub's second result, NULL
 * for the other two; have_ctx = 0 fails where they report a NULL context). */
int ecg_scrub_ptrs_check(const char *fn, int have_ctx, int k, int p, uint64_t C, uint32_t S, void *const *cells,
			 const uint32_t *status, const void *result, const void *const *r2)
{
	if (k < 1 || k > ECG_KMAX_K || p < 1 || p > ECG_KMAX_R)
		return ecg_fail(-ECG_DER_INVAL, "%s: k=%d p=%d outside 1..%d / 1..%d", fn, k, p, ECG_KMAX_K, ECG_KMAX_R);
	if (r2 == NULL) {
		if (result == NULL || (uintptr_t)result % 8u)
			return ecg_fail(-ECG_DER_INVAL, "%s: result must be 8-byte aligned device memory", fn);
	} else {
		if (result == NULL || (uintptr_t)result % 8u)
			return ecg_fail(-ECG_DER_INVAL, "%s: verify_result must be 8-byte aligned device memory", fn);
		if (*r2 == NULL || (uintptr_t)*r2 % 8u)
			return ecg_fail(-ECG_DER_INVAL, "%s: repair_result must be 8-byte aligned device memory", fn);
		if (*r2 == result)
			return ecg_fail(-ECG_DER_INVAL, "%s: verify_result and repair_result are the same address", fn);
	}
	if (S && (status == NULL || (uintptr_t)status % 4u))
		return ecg_fail(-ECG_DER_INVAL, "%s: status must be 4-byte aligned device memory", fn);
	if (!have_ctx)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL context", fn);
	if (S && C && cells == NULL)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL cells", fn);
	return 0;
}

int ecg_verify_ptrs(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S, void *const *cells, uint32_t *status,
		    void *result, void *stream)
{
	static const char fn[] = "verify_ptrs";
	/* the kernels update status words and the summary counts into result
	 * while other blocks read cells */
	const struct ecg_clear clear[2] = {{status, 4ull * S, "status"}, {result, 32, "result"}};
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
	if (S == 0 || C == 0)	/* nothing bad, every stripe clean */
		return ecg_verify_preset(fn, k, S, status, result, st);

	rc = ecg_staged_open(ctx, fn, cells, S, (uint32_t)(k + p), C, clear, 2, &t);
	if (rc)
		return rc;
	/* ecg_verify's own layout (it has no further checks of its own): its
	 * launch, with no table and no dependent address loads */
	if (t.affine) {
		ecg_staged_close(ctx, &t, st, 0);
		return ecg_verify(ctx, k, p, C, S, cells[0], t.stride, (const uint8_t *)cells[0] + (uint64_t)k * C,
				  (int64_t)C, t.stride, status, result, stream);
	}
	rc = ecg_scrub_params(fn, k, p, C, S, 1, &prm);
	if (rc)
		return ecg_staged_close(ctx, &t, st, rc);
	rc = ecg_verify_preset(fn, k, S, status, result, st);
	if (rc == 0)
		rc = ecg_staged_upload(&t, NULL, st, NULL, "verify_ptrs cell table");
	if (rc == 0)
		rc = ecg_verify_launch(ctx, fn, prm, t.sc->dev, (t.bits | C) % 16u != 0, status, result, st);
	free(prm);
	return ecg_staged_close(ctx, &t, st, rc);
}
