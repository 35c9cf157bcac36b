/*
 * ecg_recover_masks.c -- recovery with one erasure set per stripe
 * (include/ecg.h ecg_recover_masks, ecg_erasure_sets, ecg_erasure_set_index).
 *
 * What it replaces: ecg_recover takes one err_list for a whole batch, so a
 * rebuild batch whose stripes lost different shards, or a scrub whose
 * checksums name different cells per stripe, is sorted by erasure set on the
 * host and issued as one launch per set.  Here the sets are mask words that
 * stay on the device (ecg_csum_mask writes them from checksums): one launch
 * reads them, and each block picks its rows, survivors and destinations per
 * stripe (kernels/ecg_recover_masks_kernels.hip).
 *
 * The set table: every nonempty set of at most p of the k + p cells has an
 * index (ecg_kabi.h ecg_erasure_set_read); entry i holds what ecg_recov_rows
 * gives for the set of index i listed in ascending cell order -- e, out_idx,
 * dec_idx and the e x k rows as perm tables, laid out as the kernels stage
 * them (ECG_RM_ENT_Q).  Built once per (k, p) and context and kept until the
 * context goes: 3 entries for EC_2P1, 1159 entries of 1056 bytes (1.2 MB)
 * for k = 16, p = 3, the largest.
 *
 * ecg_recover_masks_ptrs is the same launch for stripes that are not one
 * strided image: a host table of cell addresses and the cell-table kernels of
 * the same file.  A table that is a strided image after all is handed to
 * ecg_recover_masks.
 *
 * How such a table gets to the device is here once, for this call and for the
 * cell-table checksum calls of ecg_csum.c (ecg_csum_masked_ptrs,
 * ecg_csum_cells_ptrs, ecg_recover_masks_ptrs_csum): ecg_staged_open (a scratch
 * slot under ctx->lock and the one checking pass over the table), _drop,
 * _upload and _close (ecg_internal.h).  The set table's fetch and the launch
 * are shared with the composite, which runs this launch in front of its own.
 */
#include <stdlib.h>
#include <string.h>

#include "ecg_internal.h"

static int check_kp(const char *fn, int k, int p)
{
	if (k < 1 || k > ECG_RM_MAX_K || p < 1 || p > ECG_RM_MAX_P)
		return ecg_fail(-ECG_DER_INVAL, "%s: k=%d p=%d outside the limits k <= %d, p <= %d", fn, k, p,
				ECG_RM_MAX_K, ECG_RM_MAX_P);
	return 0;
}

int ecg_erasure_sets(int k, int p)
{
	int rc = check_kp("erasure_sets", k, p);

	return rc ? rc : (int)ecg_erasure_set_count(k, p);
}

int ecg_erasure_set_index(int k, int p, uint32_t mask)
{
	int rc = check_kp("erasure_set_index", k, p);

	if (rc)
		return rc;
	rc = ecg_erasure_set_read(mask, k, p);
	if (rc == ECG_RM_RANGE)
		return ecg_fail(-ECG_DER_INVAL, "erasure_set_index: mask 0x%x names a cell at or above k+p=%d", mask,
				k + p);
	if (rc == ECG_RM_LOSS)
		return ecg_fail(-ECG_DER_DATA_LOSS, "erasure_set_index: mask 0x%x has more than p=%d cells", mask, p);
	return rc;	/* the index, or -1 for the empty set */
}

/* Host image of the (k, p) set table (ecg_ctx_kp_table's build): every mask
 * of at most p bits below k + p fills the entry of its index. */
static int build_sets(void *image, const void *arg)
{
	const int k = ((const int *)arg)[0], p = ((const int *)arg)[1];
	unsigned char en[(ECG_RM_MAX_K + ECG_RM_MAX_P) * ECG_RM_MAX_K];
	const uint32_t entw = 4u * ECG_RM_ENT_Q(k, p);
	const uint32_t nsets = ecg_erasure_set_count(k, p);
	const int n = k + p;
	uint32_t *img = image, seen = 0;

	ecg_gf_init();
	ecg_gen_cauchy1(k, p, en);
	for (uint32_t mask = 1; mask < (1u << n); mask++) {	/* n <= 19 */
		unsigned char rows[ECG_MAX_P * ECG_MAX_K];
		uint32_t err[ECG_RM_MAX_P], out_idx[ECG_MAX_P], dec_idx[ECG_MAX_K], *ent;
		int e = 0, reused, idx, rc;

		if (__builtin_popcount(mask) > p)
			continue;
		for (uint32_t m = mask; m; m &= m - 1u)	/* ascending cell order */
			err[e++] = (uint32_t)__builtin_ctz(m);
		idx = ecg_erasure_set_read(mask, k, p);
		if (idx < 0 || (uint32_t)idx >= nsets)
			return ecg_fail(-ECG_DER_INVAL, "recover_masks: set 0x%x has no index", mask);
		rc = ecg_recov_rows(k, p, en, err, e, rows, out_idx, dec_idx, &reused);
		if (rc)
			return rc;
		ent = img + (size_t)idx * entw;
		ent[0] = (uint32_t)e;
		for (int r = 0; r < e; r++)
			ent[1 + r] = out_idx[r];
		for (int j = 0; j < k; j++) {
			((unsigned char *)(ent + 4))[j] = (unsigned char)dec_idx[j];
			for (int r = 0; r < e; r++) {
				uint32_t *tw = ent + 8 + 4 * ECG_TBL_ROW(p, j, r);
				ecg_ptbl_t t;

				ecg_build_ptbl(rows[r * k + j], &t);
				tw[0] = t.t0lo;
				tw[1] = t.t0hi;
				tw[2] = t.t1lo;
				tw[3] = t.t1hi;
				ent[8 + ECG_TBL_T2(p, j, r)] = t.t2;
			}
		}
		seen++;
	}
	if (seen != nsets)
		return ecg_fail(-ECG_DER_INVAL, "recover_masks: %u sets built, %u expected", seen, nsets);
	return 0;
}

/* The argument checks of ecg_recover_masks in its order, for it and for the
 * composite ecg_recover_masks_csum (fn names the caller in the message;
 * have_ctx = 0 fails where ecg_recover_masks reports a NULL context). */
int ecg_recover_masks_check(const char *fn, int have_ctx, int k, int p, uint64_t C, uint32_t S, const void *stripes,
			    int64_t stripe_stride, const uint32_t *masks, const void *result, unsigned flags)
{
	int rc = check_kp(fn, k, p);

	if (rc)
		return rc;
	if (flags & ~ECG_RM_SPARSE)
		return ecg_fail(-ECG_DER_INVAL, "%s: unknown flags 0x%x", fn, flags);
	if (result == NULL || (uintptr_t)result % 8u)
		return ecg_fail(-ECG_DER_INVAL, "%s: result must be 8-byte aligned device memory", fn);
	if (S && (masks == NULL || (uintptr_t)masks % 4u))
		return ecg_fail(-ECG_DER_INVAL, "%s: masks must be 4-byte aligned device memory", fn);
	if (!have_ctx)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL context", fn);
	if (S && C && stripes == NULL)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL stripes", fn);
	/* the kernel reads mask words while other blocks write cells */
	if (S && C && ecg_cells_overlap(masks, 4ull * S, stripes, S, stripe_stride, k + p, (int64_t)C, C))
		return ecg_fail(-ECG_DER_INVAL, "%s: masks overlaps the stripes", fn);
	return 0;
}

/* The set table of (k, p), one per context: synchronous on first use.  Takes
 * ctx->lock, so it is fetched before ecg_recover_masks_ptrs locks its slot. */
int ecg_rm_settbl(ecg_ctx_t *ctx, int k, int p, const void **settbl)
{
	const int kp[2] = {k, p};

	return ecg_ctx_kp_table(ctx, &ctx->rm_tbl[k - 1][p - 1],
				(size_t)ecg_erasure_set_count(k, p) * 16u * ECG_RM_ENT_Q(k, p), build_sets, kp,
				"recover_masks set table", settbl);
}

/* The launch of both calls (fn names the call in the trace range and the
 * messages): over the strided image `stripes`, or with cells_dev over the
 * staged cell table (stripes NULL). */
int ecg_rm_launch(ecg_ctx_t *ctx, const char *fn, const void *settbl, int k, int p, uint64_t C, uint32_t S,
		  void *stripes, int64_t stripe_stride, const uint64_t *cells_dev, int bytewise,
		  const uint32_t *masks, void *result, unsigned flags, hipStream_t st)
{
	const int ptrs = cells_dev != NULL;
	ecg_mm_params_t *prm = calloc(1, sizeof(*prm));
	const char *kernel = NULL;
	int e;

	if (prm == NULL)
		return ecg_fail(-ECG_DER_NOMEM, "%s: calloc", fn);
	prm->src = stripes;
	prm->dst = stripes;
	prm->src_stripe_stride = stripe_stride;
	prm->dst_stripe_stride = stripe_stride;
	prm->cell_bytes = C;
	prm->nstripes = S;
	prm->k = (uint32_t)k;
	prm->rows = (uint32_t)p;

	ecg_trace_push(ptrs ? "ecg:recover_masks_ptrs" : "ecg:recover_masks");
	e = ecg_k_launch_recover_masks(prm, settbl, cells_dev, masks, (uint64_t *)result,
				       ctx->cfg.variant == 2 || bytewise, (flags & ECG_RM_SPARSE) != 0, &ctx->cfg,
				       (void *)st, &kernel);
	free(prm);
	return ecg_launch_done(ctx, e, ptrs ? "recover_masks_ptrs kernel launch" : "recover_masks kernel launch", 1,
			       kernel);
}

int ecg_recover_masks(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S,
		      void *stripes, int64_t stripe_stride,
		      const uint32_t *masks, void *result, unsigned flags, void *stream)
{
	const void *settbl = NULL;
	hipStream_t st;
	int rc;

	rc = ecg_recover_masks_check("recover_masks", ctx != NULL, k, p, C, S, stripes, stripe_stride, masks, result,
				     flags);
	if (rc)
		return rc;
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);

	/* nothing recovered, nothing left */
	rc = ecg_result_reset(result, st, "recover_masks memset");
	if (rc || S == 0 || C == 0)
		return rc;
	rc = ecg_rm_settbl(ctx, k, p, &settbl);
	if (rc)
		return rc;
	return ecg_rm_launch(ctx, "recover_masks", settbl, k, p, C, S, stripes, stripe_stride, NULL,
			     ((uintptr_t)stripes | (uint64_t)stripe_stride | C) % 16u != 0, masks, result, flags, st);
}

/* The one staging path of the cell-table calls (ecg_internal.h); the table is
 * staged as ecg_matmul_ptrs stages its own, so the caller's array is free again
 * when the call returns.  The pass: a NULL entry fails, and so does any of the
 * nclear ranges `clear` sharing a byte with a cell of C bytes (an empty range
 * shares none); S == 1 is affine at any stride. */
int ecg_staged_open(ecg_ctx_t *ctx, const char *fn, void *const *cells, uint64_t S, uint32_t n, uint64_t C,
		    const struct ecg_clear *clear, int nclear, struct ecg_staged *t)
{
	const uint64_t c0 = (uint64_t)(uintptr_t)cells[0];
	const uint64_t st = S > 1 ? (uint64_t)(uintptr_t)cells[n] - c0 : (uint64_t)n * C;
	uint64_t *tab, all = 0;
	int rc, aff = 1;

	*t = (struct ecg_staged){.bytes = (size_t)S * n * sizeof(uint64_t), .stride = (int64_t)st};
	pthread_mutex_lock(&ctx->lock);
	rc = ecg_scratch_reserve(ctx, t->bytes, t->bytes, &t->sc);
	if (rc)
		return ecg_staged_close(ctx, t, NULL, rc);
	tab = t->sc->pin;
	for (uint64_t s = 0; s < S; s++)
		for (uint32_t c = 0; c < n; c++) {
			const size_t i = (size_t)(s * n + c);
			const uint64_t a = (uint64_t)(uintptr_t)cells[i];

			if (a == 0)
				return ecg_staged_close(ctx, t, NULL, ecg_fail(-ECG_DER_INVAL, "%s: NULL cell %zu", fn, i));
			for (int r = 0; r < nclear; r++) {
				const uint64_t r0 = (uint64_t)(uintptr_t)clear[r].at;

				if (clear[r].len && r0 < a + C && a < r0 + clear[r].len)
					return ecg_staged_close(ctx, t, NULL,
								ecg_fail(-ECG_DER_INVAL, "%s: %s overlaps cell %zu", fn,
									 clear[r].what, i));
			}
			tab[i] = a;
			all |= a;
			aff &= a == c0 + s * st + c * C;
		}
	t->bits = all;
	t->affine = aff;
	return 0;
}

int ecg_staged_upload(struct ecg_staged *t, void *result, hipStream_t st, const char *reset, const char *what)
{
	int rc = result ? ecg_result_reset(result, st, reset) : 0;

	if (rc == 0)
		rc = ecg_table_upload(t->sc, t->bytes, st, what);
	t->queued = rc == 0;
	return rc;
}

int ecg_staged_close(ecg_ctx_t *ctx, struct ecg_staged *t, hipStream_t st, int rc)
{
	if (t->queued)
		rc = ecg_table_done(t->sc, st, rc);
	pthread_mutex_unlock(&ctx->lock);
	return rc;
}

int ecg_recover_masks_ptrs(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S, void *const *cells,
			   const uint32_t *masks, void *result, unsigned flags, void *stream)
{
	static const char fn[] = "recover_masks_ptrs";
	/* the kernel reads mask words and counts into result while other blocks
	 * write cells */
	const struct ecg_clear clear[2] = {{masks, 4ull * S, "masks"}, {result, 32, "result"}};
	const uint32_t n = (uint32_t)(k + p);
	const void *settbl = NULL;
	struct ecg_staged t;
	hipStream_t st;
	int rc;

	/* the checks that need no device, in ecg_recover_masks's order and
	 * words (no stripes: the cells are checked entry by entry below) */
	rc = ecg_recover_masks_check(fn, ctx != NULL, k, p, 0, S, NULL, 0, masks, result, flags);
	if (rc)
		return rc;
	if (S && C && cells == NULL)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL cells", fn);
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);
	if (S == 0 || C == 0)	/* nothing recovered, nothing left */
		return ecg_result_reset(result, st, "recover_masks_ptrs memset");

	rc = ecg_rm_settbl(ctx, k, p, &settbl);	/* ecg_recover_masks's; takes the lock: before open */
	if (rc == 0)
		rc = ecg_staged_open(ctx, fn, cells, S, n, C, clear, 2, &t);
	if (rc)
		return rc;
	/* ecg_recover_masks's own layout (and masks clear of the whole image, as
	 * it demands): its launch, with no table and no dependent address loads */
	if (t.affine && !ecg_cells_overlap(masks, 4ull * S, cells[0], S, t.stride, n, (int64_t)C, C)) {
		ecg_staged_close(ctx, &t, st, 0);
		return ecg_recover_masks(ctx, k, p, C, S, cells[0], t.stride, masks, result, flags, stream);
	}
	rc = ecg_staged_upload(&t, result, st, "recover_masks_ptrs memset", "recover_masks_ptrs cell table");
	if (rc == 0)
		rc = ecg_rm_launch(ctx, fn, settbl, k, p, C, S, NULL, 0, t.sc->dev, (t.bits | C) % 16u != 0, masks, result,
				   flags, st);
	return ecg_staged_close(ctx, &t, st, rc);
}
