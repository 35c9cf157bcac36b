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
 */
#include <stdlib.h>
#include <string.h>

#include "ecg_internal.h"

int ecg_verify_cell(uint32_t status, int k, int p)
{
	if (k < 1 || k > ECG_KMAX_K || p < 1 || p > ECG_KMAX_R)
		return -2;
	return ecg_verify_classify(status, k, p);
}

int ecg_verify(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S,
	       const void *data, int64_t data_stripe_stride,
	       const void *parity, int64_t parity_cell_stride, int64_t parity_stripe_stride,
	       uint32_t *status, void *result, void *stream)
{
	unsigned char en[(ECG_MAX_K + ECG_MAX_P) * ECG_MAX_K];
	ecg_mm_params_t *prm;
	hipStream_t st;
	hipError_t he;
	uint32_t kid = 0;
	int rc, e, r, j, bytewise;

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

	/* nothing bad; every stripe clean with every data cell still a candidate */
	rc = ecg_result_reset(result, st, "verify memset");
	if (rc || S == 0)
		return rc;
	he =hipMemsetD32Async((hipDeviceptr_t)status, (int)(((1u << k) - 1u) << 8), S, st);
	if (he != hipSuccess)
		return ecg_hip_fail(he, "verify status preset");
	if (C == 0)
		return 0;

	ecg_gf_init();
	prm = calloc(1, sizeof(*prm));
	if (prm == NULL)
		return ecg_fail(-ECG_DER_NOMEM, "verify: calloc");
	/* the operands and parity-row tables of ecg_encode, the stored parity
	 * in the product's destination slot (read, never written) */
	ecg_gen_cauchy1(k, p, en);
	prm->src = data;
	prm->dst = (uint8_t *)(uintptr_t)parity;
	prm->src_stripe_stride = data_stripe_stride;
	prm->dst_stripe_stride = parity_stripe_stride;
	prm->cell_bytes = C;
	prm->nstripes = S;
	prm->k = (uint32_t)k;
	prm->rows = (uint32_t)p;
	prm->accumulate = 1;
	for (j = 0; j < k; j++)
		prm->src_cell_off[j] = (int64_t)j * (int64_t)C;
	for (r = 0; r < p; r++) {
		prm->dst_cell_off[r] = (int64_t)r * parity_cell_stride;
		for (j = 0; j < k; j++)
			ecg_build_ptbl(en[(size_t)(k + r) * k + j], &prm->tbl[r][j]);
	}
	bytewise = ctx->cfg.variant == 2 || ecg_k_align_granule(prm) != 16u || C % 16u;

	ecg_trace_push("ecg:verify");
	e = ecg_k_launch_verify(prm, status, bytewise, &ctx->cfg, (void *)st, &kid);
	if (e == 0)
		e = ecg_k_launch_verify_summary(status, S, k, p, (uint64_t *)result, (void *)st);
	free(prm);
	return ecg_launch_done(ctx, e, "verify kernel launch", 2, ecg_k_verify_kernel_name(kid));
}
