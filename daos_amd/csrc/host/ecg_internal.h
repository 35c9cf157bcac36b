/*
 * ecg_internal.h -- private declarations of the C host layer.
 */
#ifndef ECG_INTERNAL_H
#define ECG_INTERNAL_H

#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <pthread.h>
#include <stdint.h>

#include "../../../include/ecg.h"
#include "../ecg_kabi.h"

#define ECG_RCACHE 16	/* recovery-matrix cache entries per context */

struct ecg_rcache_ent {
	int valid;
	int k, p, nerrs;
	uint32_t err_list[ECG_MAX_P];
	unsigned char rows[ECG_MAX_P * ECG_MAX_K];	/* data-first order */
	uint32_t out_idx[ECG_MAX_P];			/* cell each row writes */
	uint32_t dec_idx[ECG_MAX_K];
	uint64_t stamp;
};

/* Host-staging buffers for the PCIe pipeline (per context, 3 slots). */
#define ECG_NSLOT 3
struct ecg_stage {
	size_t dev_bytes;
	void *dev[ECG_NSLOT];
	hipStream_t st[ECG_NSLOT];
	hipEvent_t done[ECG_NSLOT];
};

/* Pointer tables and gathered cells (ecg_ptrs.c): two slots used in turn,
 * each guarded by ctx->lock and the `done` event of the last launch that read
 * it, so a call only waits for the launch before last. */
#ifndef ECG_NSCRATCH
#define ECG_NSCRATCH 2
#endif
struct ecg_scratch_slot {
	void *pin;
	size_t pin_bytes;
	void *dev;
	size_t dev_bytes;
	hipEvent_t done;
	int pending;
};

struct ecg_scratch {
	struct ecg_scratch_slot slot[ECG_NSCRATCH];
	unsigned next;
};

struct ecg_ctx {
	int device;
	hipStream_t stream;
	ecg_launch_cfg_t cfg;
	pthread_mutex_t lock;
	struct ecg_rcache_ent rcache[ECG_RCACHE];
	uint64_t rstamp;
	struct ecg_stage stage;
#define ECG_NCSUM_TBL 4
	void *csum_tbl[ECG_NCSUM_TBL];	/* device CRC tables by hash type (ecg_csum.c) */
	uint32_t csum_blocks;		/* csum grid cap, 0 = kernel default */
	uint32_t fused_cols;		/* fused kernel columns per item, 0 = default */
	uint32_t csum_all_route;	/* ecg_set_csum_all_route: 0 measured default, 1 fused, 2 two passes */
#define ECG_NSPLIT_CACHE 8
	struct ecg_split_ent {		/* workgroup-per-chunk CRC shifts (ecg_csum.c) */
		int valid, type;
		uint64_t m;
		uint64_t sh[ECG_CSUM_SPLIT_NW];
	} split_cache[ECG_NSPLIT_CACHE];
	unsigned split_next;
#define ECG_NKH_CACHE 8
	struct ecg_kh_ent {		/* fused-kernel item multipliers (ecg_csum.c) */
		int valid, type;
		uint64_t rcs, last;
		uint32_t ncols;
		void *dev;
	} kh_cache[ECG_NKH_CACHE];
	unsigned kh_next;
	struct ecg_scratch scratch;
#define ECG_DROPIN_STREAMS 4
	hipStream_t dpool[ECG_DROPIN_STREAMS];	/* device-cell drop-in calls (ecg_stage.c) */
	int ndpool;
	struct ecg_tuner *tuner;	/* blocks-per-CU cap per shape (ecg_tune.c) */
	/* device tables by (k, p), built and uploaded on first use under `lock`
	 * and kept until ecg_ctx_destroy (ecg_ctx_kp_table): the row tables of
	 * ecg_repair, (k + p) x k ecg_ptbl_t (ecg_repair.c), and the set tables of
	 * ecg_recover_masks, one entry per erasure set (ecg_kabi.h ECG_RM_ENT_Q,
	 * ecg_recover_masks.c) */
	void *repair_tbl[ECG_KMAX_K][ECG_KMAX_R];
	void *rm_tbl[ECG_RM_MAX_K][ECG_RM_MAX_P];
	ecg_stats_t stats;		/* telemetry (ecg_get_stats), updated with atomics */
};

/* telemetry: add n to one ecg_stats_t field of ctx (any thread) */
#define ECG_STAT_ADD(ctx, field, n) __atomic_fetch_add(&(ctx)->stats.field, (uint64_t)(n), __ATOMIC_RELAXED)

/* errors (thread-local detail string) */
int ecg_fail(int rc, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int ecg_hip_fail(hipError_t e, const char *what);
/* Pinned-host <-> device staging copy of a contiguous range issued as a 2D
 * copy of rows of a multiple of `row` bytes up to 1 MiB (the remainder, if
 * any, as a 1D copy).  Measured under concurrent traffic
 * in the other direction, the 2D path sustains ~97 % of the raw pinned H2D
 * rate where one 1D copy reaches ~84 % (tools/bench_pcie.py,
 * profiles/r01/pcie.json). */
hipError_t ecg_stage_copy(void *dst, const void *src, size_t bytes, size_t row, hipMemcpyKind kind,
			  hipStream_t st);
/* name: never NULL.  A launcher that finds nothing to launch succeeds and
 * reports no kernel (ecg_kabi.h); almost every caller has returned before that
 * can happen.  The few whose checks let an empty launch through start from
 * ECG_NO_LAUNCH_KERNEL: what ecg_last_kernel() has always shown after such a
 * call (the first product kernel's name), kept until those calls are fixed. */
#define ECG_NO_LAUNCH_KERNEL "ecg_mm_kernel<2,1,0,0>"
void ecg_set_last_kernel(const char *name);

/* GF(2^8) tables (ecg_gf.c) */
void ecg_gf_init(void);
extern unsigned char ecg_gf_mul_tbl[256][256];
void ecg_build_ptbl(unsigned char c, ecg_ptbl_t *t);
/* data-first decode rows: out_idx[i] = logical cell written by rows[i] */
int ecg_recov_rows(int k, int p, const unsigned char *en_matrix,
		   const uint32_t *err_list, int nerrs, unsigned char *rows,
		   uint32_t *out_idx, uint32_t *dec_idx, int *reused_encode);

/* pointer tables (ecg_ptrs.c) */
void ecg_scratch_free(ecg_ctx_t *ctx);
/* ecg_update_ptrs with explicit parity rows coef[rows][k]; *nlaunch (may be
 * NULL) = the ordered launches the batch took */
int ecg_update_ptrs_coef(ecg_ctx_t *ctx, int k, int rows, const unsigned char *coef, uint64_t C, uint32_t nreq,
			 void *const *cells, const uint8_t *vec_i, void *stream, uint32_t *nlaunch);
/* next scratch slot with at least these sizes, free of readers (ctx->lock held) */
int ecg_scratch_reserve(ecg_ctx_t *ctx, size_t pin_bytes, size_t dev_bytes,
			struct ecg_scratch_slot **out);
/* The first `bytes` of sc->pin to sc->dev, queued on st (a fetch kernel:
 * ecg_k_launch_fetch); `what` names the table in the error. */
int ecg_table_upload(struct ecg_scratch_slot *sc, size_t bytes, hipStream_t st, const char *what);
/* The release rule of a slot: once ecg_table_upload has returned 0 for it,
 * every way out of the caller comes here, after the last launch queued on st
 * that reads the slot and however those launches went (rc) -- the fetch reads
 * the pinned half even when nothing follows it.  Records `done` and marks the
 * slot pending, so its next user waits (ctx->lock held); nowhere else does
 * either.  Returns rc, or the event's failure when rc was 0. */
int ecg_table_done(struct ecg_scratch_slot *sc, hipStream_t st, int rc);

/* The launch of ecg_matmul_ptrs_lens over a slot its caller has filled
 * (ecg_ptrs.c; ctx->lock held), shared with ecg_obj_ec_singv_encode_dev
 * (ecg_daos.c).  Slot layout, pinned and device alike:
 *   [0, S*n*8)      the cell table, n = k + rows entries per stripe (a stripe of
 *                   length 0: zeros)
 *   then S*8        the lengths (each below ECG_LENS_MAX_BYTES: a span's first
 *                   column is a 32-bit word)
 *   then nspans*8   the span records, written here -- ecg_lens_table_bytes()
 *                   in all, nspans and max_cols being ecg_lens_plan's
 *   seg_off         with `gather` (NULL: none), its segments; they travel in
 *                   the same upload and run before the product
 *   zero_off        device only: zero_bytes (0: none) set to zero before the
 *                   gather, for cells the table points into it
 * One upload, the memset, the gather, one product launch -- the fixed-length
 * kernel through launch tuner when every length is the same and none is 0 --
 * and ecg_table_done on every way out once the upload is queued. */
#define ECG_LENS_MAX_BYTES (1ull << 44)
struct ecg_segs;
size_t ecg_lens_table_bytes(uint32_t S, int n, uint64_t nspans);
int ecg_lens_launch(ecg_ctx_t *ctx, struct ecg_scratch_slot *sc, int k, int rows, const unsigned char *coef,
		    uint32_t S, uint64_t nspans, uint32_t max_cols, hipStream_t st, const struct ecg_segs *gather,
		    size_t seg_off, size_t zero_off, size_t zero_bytes);

/* batched segment copies (ecg_sgl.c).  A fixed list (cap preset, fixed = 1)
 * writes into caller memory and fails instead of growing. */
struct ecg_segs {
	ecg_copy_seg_t *seg;
	size_t n, cap;
	uint64_t tiles;
	int fixed;
};
int ecg_segs_add(struct ecg_segs *v, uint64_t dst, uint64_t src, uint64_t len);
void ecg_segs_fini(struct ecg_segs *v);
/* launch over a device copy of v->seg already queued on st */
int ecg_segs_launch(const struct ecg_segs *v, const void *segs_dev, hipStream_t st);

/* what ecg_verify and the mask-driven calls share (ecg_core.c) */
/* result = {0, UINT64_MAX, 0, 0} on st, the preset of the kernels' counters
 * (kernels/ecg_rows_dev.h rows_count); `what`: the error text ("repair memset") */
int ecg_result_reset(void *result, hipStream_t st, const char *what);
/* After a launch inside an ecg_trace_push range: ends the range; e != 0 (a
 * hipError_t) fails as `what`, else nlaunch launches and the kernel's name count */
int ecg_launch_done(ecg_ctx_t *ctx, int e, const char *what, unsigned nlaunch, const char *name);
/* Does [a, a + alen) meet the cells base + i*si + j*sj, i < ni, j < nj, each
 * len bytes long?  (Their bounding range: strides may be negative.) */
int ecg_cells_overlap(const void *a, uint64_t alen, const void *base, int64_t ni, int64_t si, int64_t nj,
		      int64_t sj, uint64_t len);
/* The device table *slot (of ctx->repair_tbl or ctx->rm_tbl), built on first
 * use under ctx->lock: build(img, arg) fills the zeroed host image, which is
 * uploaded synchronously.  *out = the table; a failure names it as `what` and
 * leaves the slot NULL. */
int ecg_ctx_kp_table(ecg_ctx_t *ctx, void **slot, size_t bytes, int (*build)(void *img, const void *arg),
		     const void *arg, const char *what, const void **out);
void ecg_ctx_kp_tables_fini(void **slots, int nk, int np);	/* frees nk x np of them */
/* ecg_recover_masks's argument checks, in its order (fn: the caller's name in
 * the message; have_ctx = 0 fails where it reports a NULL context) */
int ecg_recover_masks_check(const char *fn, int have_ctx, int k, int p, uint64_t C, uint32_t S, const void *stripes,
			    int64_t stripe_stride, const uint32_t *masks, const void *result, unsigned flags);
/* what the cell-table calls share (ecg_recover_masks.c): ecg_recover_masks_ptrs
 * and, in ecg_csum.c, ecg_csum_masked_ptrs, ecg_csum_cells_ptrs and
 * ecg_recover_masks_ptrs_csum; ecg_verify_ptrs (ecg_verify.c), ecg_repair_ptrs
 * and ecg_scrub_ptrs (ecg_repair.c); ecg_update_masks_ptrs (ecg_update_masks.c,
 * S x (2k + p) entries and its own three-group strided test) */
/* a range no cell of a table may share a byte with; `what` names it in the error */
struct ecg_clear {
	const void *at;
	uint64_t len;
	const char *what;
};
/* A caller's table of S x n addresses of cells of C bytes in a scratch slot,
 * ctx->lock held.  A call is: its argument checks, open, its own overlap
 * checks and affine test, upload, its launches, and close on every way out. */
struct ecg_staged {
	struct ecg_scratch_slot *sc;
	size_t bytes;		/* of the table */
	uint64_t bits;		/* OR of the addresses: the lane choice */
	int64_t stride;		/* of the strided image it is, if affine */
	int affine;		/* every entry is cells[0] + s * stride + c * C */
	int queued;		/* the upload is: close releases the slot */
};
/* Locks, reserves a slot and passes once over the table: -ECG_DER_INVAL for a
 * NULL entry or a `clear` range inside a cell, naming `fn` and the entry.  On
 * failure closed: unlocked and nothing held. */
int ecg_staged_open(ecg_ctx_t *ctx, const char *fn, void *const *cells, uint64_t S, uint32_t n, uint64_t C,
		    const struct ecg_clear *clear, int nclear, struct ecg_staged *t);
/* ecg_result_reset (result NULL: none), then ecg_table_upload; their error texts */
int ecg_staged_upload(struct ecg_staged *t, void *result, hipStream_t st, const char *reset, const char *what);
/* ecg_table_done if the upload was queued (else nothing was: the affine route,
 * a later argument error), then unlocks; returns what ecg_table_done would */
int ecg_staged_close(ecg_ctx_t *ctx, struct ecg_staged *t, hipStream_t st, int rc);
/* the set table of (k, p), built on first use; takes ctx->lock */
int ecg_rm_settbl(ecg_ctx_t *ctx, int k, int p, const void **settbl);
/* the recover_masks launch over the strided image `stripes`, or with cells_dev
 * over a staged cell table (stripes NULL); fn names the call */
int ecg_rm_launch(ecg_ctx_t *ctx, const char *fn, const void *settbl, int k, int p, uint64_t C, uint32_t S,
		  void *stripes, int64_t stripe_stride, const uint64_t *cells_dev, int bytewise,
		  const uint32_t *masks, void *result, unsigned flags, hipStream_t st);

/* what ecg_update_masks, ecg_update_masks_ptrs and, in ecg_csum.c, their _csum
 * composites and ecg_csum_updated_ptrs share (ecg_update_masks.c) */
/* the argument checks of the update calls in their documented order (fn: the
 * caller's name in the message; have_ctx = 0 fails where they report a NULL
 * context).  strided = 1: ecg_update_masks's operands; 0: the table form
 * (`cells`; its entries are checked by ecg_staged_open), which has no packed
 * form.  recalc_above != NULL: the caller is ecg_agg_masks / _ptrs -- packed is
 * refused, the threshold checked right after the flags and *recalc_above left
 * as the effective one, 0 .. k; NULL: an update call */
int ecg_um_check(const char *fn, int strided, int have_ctx, int k, int p, uint64_t C, uint32_t S,
		 const void *old_cells, const void *new_cells, const void *parity, int64_t parity_cell_stride,
		 int64_t parity_stripe_stride, const void *cells, const uint32_t *masks, const void *result,
		 unsigned flags, uint32_t *recalc_above);
/* the update launch over the three strided images, or with cells_dev over a
 * staged table of S x (2k + p) entries; fn names the call */
int ecg_um_launch(ecg_ctx_t *ctx, const char *fn, int k, int p, uint64_t C, uint32_t S, const void *old_cells,
		  const void *new_cells, int64_t upd_stripe_stride, void *parity, int64_t parity_cell_stride,
		  int64_t parity_stripe_stride, const uint64_t *cells_dev, int bytewise, const uint32_t *masks,
		  void *result, unsigned flags, hipStream_t st);
/* The launcher of ecg_agg_masks and, with cells_dev, ecg_agg_masks_ptrs
 * (kernels/ecg_update_masks_kernels.hip, extern "C"): ecg_k_launch_update_masks's
 * operands (ecg_kabi.h; never packed), counters, lane / byte choice and grids,
 * with the route of a stripe read by ecg_agg_route(masks[s], k, recalc_above):
 * a DELTA stripe gets that launcher's update; a RECALC stripe gets parity[r] =
 * XOR_{j < k} tbl[r][j] * (bit j of the mask ? new_j : old_j), its old parity
 * unread and every data cell read from one image.  recalc_above <= k
 * (hipErrorInvalidValue otherwise).  *kernel: ecg_agg_masks_kernel<p> /
 * ecg_agg_masks_byte_kernel, or their ecg_agg_masks_ptr_* counterparts over a
 * table. */
int ecg_k_launch_agg_masks(const ecg_mm_params_t *p, const uint64_t *cells_dev, const uint32_t *masks,
			   uint64_t *result, uint32_t recalc_above, int bytewise, int sparse,
			   const ecg_launch_cfg_t *cfg, void *stream, const char **kernel);
/* is the parity group of tab[S][2k + p] strided (p0 + s*ps + r*pc)?  *bits: the
 * OR of the parity addresses */
int ecg_um_parity_group(const uint64_t *tab, int k, int p, uint64_t C, uint32_t S, int64_t *pc, int64_t *ps,
			uint64_t *bits);
/* is tab[S][2k + p] three strided groups (old and new with one stride us)? */
int ecg_um_three_groups(const uint64_t *tab, int k, int p, uint64_t C, uint32_t S, int64_t *us, int64_t *pc,
			int64_t *ps);

/* what the strided and the cell-table scrub calls share (ecg_verify.c):
 * ecg_verify, ecg_repair, ecg_verify_ptrs, ecg_repair_ptrs, ecg_scrub_ptrs */
/* zeroed launch parameters with the shape (k, rows = p, C, S) and, with
 * `rows`, the Cauchy parity rows as perm tables and `accumulate`; free() it */
int ecg_scrub_params(const char *fn, int k, int p, uint64_t C, uint32_t S, int rows, ecg_mm_params_t **out);
/* the strided operands: data cells as sources, parity rows as destinations */
void ecg_scrub_strided(ecg_mm_params_t *prm, const void *data, int64_t data_stripe_stride, const void *parity,
		       int64_t parity_cell_stride, int64_t parity_stripe_stride);
/* result = {0, UINT64_MAX, 0, 0} and, S != 0, every status word clean with
 * every data cell a candidate, on st */
int ecg_verify_preset(const char *fn, int k, uint32_t S, uint32_t *status, void *result, hipStream_t st);
/* syndrome pass + summary over prm's strided operands, or with cells_dev over
 * a staged cell table; counts 2 launches and names the syndrome kernel */
int ecg_verify_launch(ecg_ctx_t *ctx, const char *fn, const ecg_mm_params_t *prm, const uint64_t *cells_dev,
		      int bytewise, uint32_t *status, void *result, hipStream_t st);
/* the device-free argument checks of the cell-table scrub calls in their
 * documented order (r2: ecg_scrub_ptrs's repair_result, NULL for the others;
 * have_ctx = 0 fails where they report a NULL context) */
int ecg_scrub_ptrs_check(const char *fn, int have_ctx, int k, int p, uint64_t C, uint32_t S, void *const *cells,
			 const uint32_t *status, const void *result, const void *const *r2);

/* checksums (ecg_csum.c) */
void ecg_csum_ctx_fini(ecg_ctx_t *ctx);
/* The launcher of ecg_csum_updated and, with p->cells_dev, ecg_csum_updated_ptrs
 * (kernels/ecg_csum_kernels.hip, extern "C"; the parameters are ecg_kabi.h's);
 * max_blocks 0 = default.  *kernel: ecg_crc_updated_kernel<type> /
 * ecg_adler_updated_kernel, their ecg_*_updated_ptr_kernel counterparts over a
 * table, <..bytes> when the chunks do not all start and end 16-byte aligned. */
int ecg_k_launch_csum_updated(const ecg_csum_updated_params_t *p, void *stream, uint32_t max_blocks,
			      const char **kernel);
int ecg_csum_fused_params(ecg_ctx_t *ctx, int type, uint64_t chunksize, uint64_t rec_size,
			  uint64_t C, int k, int rows, void *csums, int src, ecg_mmcs_params_t *q);

/* source checksums of ecg_*_csum_all: 1 = try the fused SRC kernel, 0 = two passes */
int ecg_csum_all_route(const ecg_ctx_t *ctx, int type, int k, int rows);

/* product + chunk checksums of every output cell, cells as extents from
 * record index 0; csums[row_slot[r]][s][chunk] (ecg_core.c) */
int ecg_matmul_csum(ecg_ctx_t *ctx, int k, int rows, const unsigned char *coef, uint64_t C,
		    uint32_t S, const void *src, const int64_t *soff, int64_t sstride, void *dst,
		    const int64_t *doff, int64_t dstride, int type, uint64_t chunksize,
		    uint64_t rec_size, void *csums, const uint32_t *row_slot, void *stream);

/* one-cell product, per-stripe coefficient column sel_dev[s] < ncols
 * (coef rows x ncols), 16-byte aligned operands (ecg_core.c) */
int ecg_matmul_sel(ecg_ctx_t *ctx, int ncols, int rows, const unsigned char *coef, uint64_t C, uint32_t S,
		   const void *src, int64_t sstride, const uint8_t *sel_dev, void *dst, const int64_t *doff,
		   int64_t dstride, void *stream);
/* host pipeline with an explicit parity row pitch (ecg_core.c) */
int ecg_encode_host_rows(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S, const void *data,
			 void *parity, size_t prow, uint32_t chunk);
/* "0,1,2" / "all" / NULL -> device list (ecg_multi.c); count or -ECG_DER_INVAL */
int ecg_parse_devices(const char *spec, int *dev, int max);

/* roctx ranges (ecg_trace.c): no-ops without the roctx library or with
 * ECG_ROCTX=0 */
void ecg_trace_push(const char *name);
void ecg_trace_pop(void);
int ecg_trace_active(void);

/* launch tuner (ecg_tune.c): product launches of wide shapes measure the
 * blocks-per-CU cap against none and keep the faster */
#define ECG_NTUNE 16
struct ecg_tuner;
int ecg_tune_init(ecg_ctx_t *ctx);
void ecg_tune_fini(ecg_ctx_t *ctx);
int ecg_tune_launch(ecg_ctx_t *ctx, const ecg_mm_params_t *p, hipStream_t st, const char **kernel);
/* The device whose memory p is; < 0 for host memory: ECG_PTR_HOST (known to
 * the HIP runtime: pinned, registered, managed) or ECG_PTR_UNKNOWN (plain
 * malloc / mmap) (ecg_stage.c). */
#define ECG_PTR_HOST (-1)
#define ECG_PTR_UNKNOWN (-2)
int ecg_ptr_device(const void *p);
/* ecg_ptr_device through the calling thread's short-lived cache of 2 MiB
 * regions of plain host memory (ecg_dropin.c): near-free for a caller's
 * reused malloc'd buffers */
int ecg_ptr_device_cached(const void *p);
/* The same for any launcher of the product (the pointer-table kernel): `g`
 * its lane granule, `layout` its layout class (ECG_TUNE_LAYOUT_*), `fn(p,
 * cfg, stream, kernel, arg)` the launch under a given geometry, which reports
 * the kernel it launched as the ecg_k_launch_* do (every path here calls fn
 * exactly once). */
typedef int (*ecg_mm_launch_fn)(const ecg_mm_params_t *p, const ecg_launch_cfg_t *cfg, void *stream,
				const char **kernel, const void *arg);
#define ECG_TUNE_LAYOUT_SEPARATE 0u	/* source and destination stripe strides differ */
#define ECG_TUNE_LAYOUT_INTERLEAVED 1u	/* one stripe stride: in-place recovery */
#define ECG_TUNE_LAYOUT_PTRS 2u		/* per-stripe pointer table */
int ecg_tune_launch_fn(ecg_ctx_t *ctx, const ecg_mm_params_t *p, uint32_t g, uint32_t layout,
		       ecg_mm_launch_fn fn, const void *arg, hipStream_t st, const char **kernel);

/* synchronous one-stripe product on ctx's GPU; place = ecg_cells_place's
 * placement of the k + rows cells (NULL: all host memory) (ecg_stage.c) */
int ecg_matmul_host_mem(ecg_ctx_t *ctx, int len, int k, int rows, const unsigned char *coef,
			unsigned char *const *src, unsigned char *const *dst, unsigned flags, const signed char *place);
/* Forget every thread's remembered device ranges (ecg_cells_place): called
 * when the library frees device memory. */
void ecg_place_forget(void);
/* placement of every cell of a one-stripe call: place[i] = device or -1
 * (host); returns the device cells' count (*dev their device) or a negative
 * DER code (cells on two devices, a device cell past its allocation) */
int ecg_cells_place(unsigned char *const *src, int k, unsigned char *const *dst, int rows, uint64_t len,
		    int (*query)(const void *), signed char *place, int *dev);
/* every cell [v[i], v[i] + len) inside one allocation of ctx's device, else
 * -DER_INVAL naming `what` (ecg_stage.c) */
int ecg_cells_on_device(ecg_ctx_t *ctx, unsigned char *const *v, int n, uint64_t len, const char *what);
/* drop-in routing (ecg_dropin.c): device cells -> GPU, host cells -> CPU
 * below the crossover or without a usable device, else GPU.  ctx NULL = the
 * calling thread's default context. */
int ecg_dropin_product(const char *fn, ecg_ctx_t *ctx, int len, int k, int rows, const unsigned char *coef,
		       unsigned char *const *src, unsigned char *const *dst, unsigned flags);
/* 1 when the drop-in may use a GPU in this process */
int ecg_dropin_gpu(void);
/* Host cells of `bytes` (len x (k + rows)) compute on the CPU path: below the
 * drop-in crossover, or $ECG_FORCE_CPU=1 (ecg_dropin.c). */
int ecg_dropin_host_on_cpu(uint64_t bytes);
/* the calling thread's default context; NULL without a usable device */
ecg_ctx_t *ecg_dropin_ctx(void);

/* context helpers (ecg_core.c) */
int ecg_ctx_enter(ecg_ctx_t *ctx);
#ifdef ECG_QUEUE_TIMING
void ecg_ptrs_timing_print(void);	/* diagnostic build: update_ptrs call phases */
#endif

/* NUMA placement (ecg_numa.c); the cpu_set_t helpers need _GNU_SOURCE in the
 * including file */
int ecg_numa_enabled(void);
#ifdef _GNU_SOURCE
#include <sched.h>
int ecg_numa_node_cpus(int node, cpu_set_t *set);
int ecg_numa_bind_thread(int device, cpu_set_t *saved);
void ecg_numa_restore_thread(const cpu_set_t *saved);
#endif
hipStream_t ecg_pick_stream(ecg_ctx_t *ctx, void *stream);

#endif
