/*
 * ecg.h -- MI355X-native Reed-Solomon erasure-coding engine for DAOS EC
 * objects: the core C-ABI.
 *
 * Plain C, host pointers / device pointers / sizes only (no HIP, no torch
 * types).  Streams are opaque `void *` (a hipStream_t; NULL = the context's
 * own stream).  Every function returns 0 or a negative DAOS errno
 * (ref:src/include/daos_errno.h); ecg_strerror() gives the detail of the last
 * failure on the calling thread.  All entry points are thread-safe.
 *
 * What this replaces: the arithmetic boundary of DAOS's EC
 * object class -- ISA-L ec_encode_data / ec_encode_data_update / xor_gen as
 * called from ref:src/object/cli_ec.c:540,571,2641,
 * ref:src/object/srv_ec_aggregate.c:693,1092,1099,1136 -- batched over stripes
 * and executed by hand-written gfx950 kernels on device-resident cells.
 * The ISA-L-signature drop-in is ecg_isal.h; the DAOS codec surface
 * (obj_ec_codec_*, obj_ec_encode_buf, recovery codec) is ecg_daos.h.
 *
 * Arithmetic is GF(2^8) with polynomial 0x11d and generator 2, bit-exact with
 * ISA-L's ec_encode_data_base (and therefore with every ISA-L SIMD path).
 */
#ifndef ECG_H
#define ECG_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Negative DAOS errno values (ref:src/include/daos_errno.h). */
#define ECG_DER_INVAL		1003
#define ECG_DER_NOMEM		1009
#define ECG_DER_NOSYS		1010	/* no gfx950 device / HIP runtime */
#define ECG_DER_IO		2001	/* HIP runtime or kernel failure */
#define ECG_DER_REC2BIG		2013
#define ECG_DER_DATA_LOSS	2026	/* more erasures than parity cells */

/* Limits (ref:src/object/obj_ec.h:16-20, ref:src/object/obj_class.c:587-601). */
#define ECG_MAX_K		64
#define ECG_MAX_P		8

/* Parity row pitch.  Client-layout parity [p][S][C] runs fastest with its p
 * rows one buffer at a pitch of S*C + ECG_PARITY_ROW_PAD: rows a large power
 * of two apart, or separately allocated rows the allocator happens to place
 * at such distances, alias in HBM (measured, profiles/r05/: EC_4P2 1 MiB x
 * 1024 encode with the rows as two hipMalloc allocations 0.91 of the padded
 * rate, EC_8P2 x 512 with the unpadded pitch 0.96).  The library's own
 * staging pads its parity rows this way; callers choose their own layout. */
#define ECG_PARITY_ROW_PAD	4096

/* Flags for ecg_matmul */
#define ECG_F_ACCUMULATE	0x1u	/* dst ^= product (else dst = product) */

typedef struct ecg_ctx ecg_ctx_t;

/* ---- context / device ---------------------------------------------------- */
/* Number of usable (gfx950) HIP devices; 0 when none.  Never fails. */
int ecg_device_count(void);
/* Binds a context to `device` (index into the visible HIP devices).
 * -ECG_DER_NOSYS when the device is absent or not gfx950: the batched device
 * API has no CPU fallback (the drop-in surfaces route host cells to the CPU
 * path themselves, ecg_set_dropin_crossover). */
int ecg_ctx_create(int device, ecg_ctx_t **ctx);
void ecg_ctx_destroy(ecg_ctx_t *ctx);
int ecg_ctx_device(const ecg_ctx_t *ctx);
/* 1 when the context's device served misaligned dword loads and stores at
 * creation (the unaligned access mode ROCm enables on gfx9+): destinations
 * off a dword boundary then run on the vector lanes; 0 when it did not (or
 * ECG_UNALIGNED=0 was set): such launches run the byte kernels, same
 * results, ~8x slower.  The probe assumes a misaligned access is served (or
 * rounded), not trapped: on a device configured to FAULT on misaligned
 * accesses, set ECG_UNALIGNED=0 before creating a context. */
int ecg_ctx_unaligned_ok(ecg_ctx_t *ctx);
/* PCI bus id ("0000:c1:00.0") of a visible device: tells ranks or shards
 * that landed on the same physical GPU apart. */
int ecg_device_pci_bus_id(int device, char *buf, int len);
/* NUMA node of a PCI device ("0000:23:00.0", any case) from sysfs
 * (/sys/bus/pci/devices/<bdf>/numa_node), and of a HIP device; -1 when
 * unknown.  ecg_multi workers run on their device's node and queue staging
 * is allocated there; $ECG_NUMA=0 turns that off. */
int ecg_pci_numa_node(const char *pci_bus_id);
int ecg_device_numa_node(int device);
/* The context's default stream (used when a call passes stream == NULL). */
void *ecg_ctx_stream(ecg_ctx_t *ctx);
const char *ecg_strerror(void);
/* Name of the kernel the last ecg_* compute call on this thread launched. */
const char *ecg_last_kernel(void);
/* Identity of this build: "src_sha256=<16 hex>;hipcc=<version>;arch=gfx950",
 * the hash over every source, header and build file of the library
 * (daos_amd/csrc/Makefile HASHED), fixed at build time. */
const char *ecg_build_info(void);

/* ---- field and matrices (host; setup only) ------------------------------- */
unsigned char ecg_gf_mul(unsigned char a, unsigned char b);
unsigned char ecg_gf_inv(unsigned char a);
/* (k+p) x k Cauchy1 encode matrix: identity rows then 1/(i ^ j), the matrix
 * DAOS builds per EC class (ref:src/object/obj_class.c:611-617). */
int ecg_gen_cauchy1(int k, int p, unsigned char *en_matrix);
/* n x n inverse over GF(2^8); `in` is destroyed; -ECG_DER_INVAL if singular. */
int ecg_invert_matrix(unsigned char *in, unsigned char *out, int n);
/* DAOS recovery codec (ref:src/object/cli_ec.c:2152-2250): for LOGICAL error
 * indices err_list[nerrs] (cells 0..k-1 data, k..k+p-1 parity) produce the
 * decode rows (nerrs x k, in err_list order), dec_idx[k] (the surviving cells
 * they consume) and *reused_encode (1 when all p parity cells and no data
 * cell are lost: rows are then the encode parity rows and dec_idx = 0..k-1,
 * ref:src/object/cli_ec.c:2205-2210).  -ECG_DER_DATA_LOSS when nerrs > p. */
int ecg_recov_matrix(int k, int p, const unsigned char *en_matrix,
		     const uint32_t *err_list, int nerrs, unsigned char *de_rows,
		     uint32_t *dec_idx, int *reused_encode);

/* ---- device-resident batched codec (the hot path) ----------------------- */
/*
 * dst cell r of stripe s  (^)=  XOR_{j<k} coef[r*k + j] * (src cell j of s)
 * for every byte i < cell_bytes and every stripe s < nstripes, where
 *   src cell j of s = src + s*src_stripe_stride + src_cell_off[j]
 *   dst cell r of s = dst + s*dst_stripe_stride + dst_cell_off[r]
 * All pointers are device pointers.  k <= 64, rows <= 8 (larger k is split
 * into accumulating launches).  Any alignment: 16-byte aligned cells run
 * 16-byte lanes, dword-aligned sources dword lanes, sources at any byte
 * funnel-shifted dword lanes; outputs at any byte are stored as misaligned
 * dwords by the same lanes.
 * Asynchronous on `stream`.
 */
int ecg_matmul(ecg_ctx_t *ctx, int k, int rows, const unsigned char *coef,
	       uint64_t cell_bytes, uint32_t nstripes,
	       const void *src, const int64_t *src_cell_off, int64_t src_stripe_stride,
	       void *dst, const int64_t *dst_cell_off, int64_t dst_stripe_stride,
	       unsigned flags, void *stream);

/* Full-stripe encode with the Cauchy1 matrix (ISA-L ec_encode_data with the
 * DAOS codec tables).  Data cell j of stripe s at
 *   data + s*data_stripe_stride + j*cell_bytes,
 * parity cell r of stripe s at
 *   parity + r*parity_cell_stride + s*parity_stripe_stride.
 * Client write layout (ref:src/object/cli_ec.c:75-97,638-640): data [S][k][C],
 * parity [p][S][C] => data_stripe_stride = k*C, parity_cell_stride = S*C,
 * parity_stripe_stride = C.  Recovery layout [S][k+p][C] => parity = data +
 * k*C, parity_cell_stride = C, both stripe strides (k+p)*C. */
int ecg_encode(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
	       const void *data, int64_t data_stripe_stride,
	       void *parity, int64_t parity_cell_stride, int64_t parity_stripe_stride,
	       void *stream);

/* In-place degraded-read / rebuild recovery over stripes laid out
 * [S][k+p][cell_bytes] in logical cell order, stripe s at
 * stripes + s*stripe_stride (obj_ec_recov_data, ref:src/object/cli_ec.c:
 * 2814-2885).  Erased cells (logical indices) are regenerated from the first
 * k survivors.  Decode matrices are cached per (k, p, err_list). */
int ecg_recover(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
		void *stripes, int64_t stripe_stride,
		const uint32_t *err_list, int nerrs, void *stream);

/* Aggregation delta parity update (xor_gen + ec_encode_data_update fused,
 * ref:src/object/srv_ec_aggregate.c:1062-1105), batched over stripes:
 *   parity[r] ^= XOR_u coef[r][cell_idx[u]] * (old[u] ^ new[u])
 * for the nupd updated data cells of each stripe.  Cell u of stripe s:
 *   old_cells + s*old_stripe_stride + u*cell_bytes (same for new_cells);
 * parity cell r of stripe s: parity + r*parity_cell_stride + s*parity_stripe_stride. */
int ecg_update(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
	       int nupd, const uint32_t *cell_idx,
	       const void *old_cells, const void *new_cells, int64_t upd_stripe_stride,
	       void *parity, int64_t parity_cell_stride, int64_t parity_stripe_stride,
	       void *stream);

/* ecg_update with one set of updated cells PER STRIPE, in one launch: the
 * batched form of the partial-stripe update agg_update_parity(entry, bit_map,
 * cell_cnt) drives with its bitmap of updated cells (ref:src/object/
 * srv_ec_aggregate.c:1006-1105; ecg_daos.h ecg_agg_update_parity is the
 * one-stripe form), for a batch whose stripes changed different cells.  The
 * sets are mask words in device memory, which ecg_csum_mask writes from the
 * chunk checksums of the old and the new image (ecg_csum.h: ecg_csum_extents
 * (old) -> ecg_csum_extents(new) -> ecg_memset(masks, 0) -> ecg_csum_mask(got =
 * new, want = old) -> ecg_update_masks, five asynchronous calls on one stream;
 * the masks never leave the device and the host need not know which cells
 * changed).
 * Parity addressed exactly as in ecg_update / ecg_encode: the client layout
 * [p][S][C] (a padded row pitch included) and the recovery layout
 * [S][k+p][C] with parity = stripes + k*C alike.  masks: device memory,
 * nstripes words, 4-byte aligned, read only; bit j of masks[s] = data cell j
 * of stripe s changed.  old_cells / new_cells: full stripe images, cell j of
 * stripe s at old_cells + s*upd_stripe_stride + j*cell_bytes (the same for
 * new_cells); only the cells a mask names are read, and with the recovery
 * layout old_cells = stripes, upd_stripe_stride = (k+p)*C is a supported use
 * (the old data and the parity interleave in one buffer).  Any of the three
 * strides may be negative (see ecg_recover_masks).  With
 * ECG_UM_PACKED the AGG_IOV_ODATA / AGG_IOV_DATA layout of the reference: the
 * cell of the i-th set bit of masks[s], in ascending order, is at
 * + s*upd_stripe_stride + i*cell_bytes.  With m = masks[s]:
 *   m == 0                    nothing of the stripe is read or written; it is
 *                             not counted
 *   a bit at or above k set   nothing is written; the stripe is counted in
 *                             result[3] and result[1]
 *   otherwise (1..k bits)     parity[r] ^= XOR_{j in m} g[k+r][j] * (old_j ^
 *                             new_j) for r < p: byte for byte what ecg_update(
 *                             nupd = popcount(m), cell_idx = the set bits of m
 *                             in ascending order, nstripes = 1) leaves for that
 *                             stripe over the same cells, nothing else
 * All 2^32 mask values are safe.  result (device, 4 x uint64, 8-byte aligned)
 * = {stripes updated, lowest stripe with an invalid mask (UINT64_MAX if none),
 * cells applied, stripes with an invalid mask}; nstripes == 0 or cell_bytes ==
 * 0 leaves {0, UINT64_MAX, 0, 0}.  INVALID MASKS ARE REPORTED THROUGH result
 * ONLY: the call itself returns 0.
 * Limits: k <= 16 and p <= 8 (as ecg_update_ptrs).  -ECG_DER_INVAL for k or p
 * beyond them, an unknown flag bit, masks NULL or not 4-byte aligned, result
 * NULL or not 8-byte aligned (both checked for nstripes == 0 too), old_cells,
 * new_cells or parity NULL, and masks or result lying inside the byte span of
 * the parity.  THE CALLER'S CONTRACT, as in ecg_update: no old or new cell a
 * mask names may overlap a parity cell of the batch (it is not checked).
 * old_cells == new_cells is allowed and leaves every parity byte as it was.
 * Any alignment and length: old_cells, new_cells, parity, the three strides
 * and cell_bytes all multiples of 16 run the 16-byte lane kernel, everything
 * else a byte-granular one.
 * flags: ECG_UM_PACKED above.  ECG_RM_SPARSE is a tuning hint and never
 * changes a result -- few stripes changed, so the launch uses the grid whose
 * cost on clean stripes is one mask load per 64 of them; without it every
 * stripe is expected to have work and a block row takes one stripe.
 * ecg_set_launch's grid_x / grid_y override either grid; variant 2 forces the
 * byte kernel.  Asynchronous on `stream`; no table is built or uploaded.
 * Telemetry: ecg_get_stats' update_cells / update_bytes are NOT advanced (how
 * many cells were applied is known on the device only: read result);
 * `launches` counts the launch. */
#define ECG_UM_PACKED 0x2u	/* ECG_RM_SPARSE (0x1u, below) is the other accepted flag */
int ecg_update_masks(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
		     const void *old_cells, const void *new_cells, int64_t upd_stripe_stride,
		     void *parity, int64_t parity_cell_stride, int64_t parity_stripe_stride,
		     const uint32_t *masks, void *result, unsigned flags, void *stream);
/* ecg_update_masks over a TABLE OF CELL ADDRESSES, for callers whose stripes
 * are not three strided images: agg_update_parity works on one stripe's
 * buffers at a time (ref:src/object/srv_ec_aggregate.c:1006-1105), so a batch
 * of stripes is a set of separate allocations.  cells: HOST array of nstripes
 * * (2k+p) device addresses; row s is
 *   cells[s*(2k+p) + j],      j < k   old data cell j of stripe s
 *   cells[s*(2k+p) + k + j],  j < k   new data cell j
 *   cells[s*(2k+p) + 2k + r], r < p   parity cell r
 * every cell cell_bytes long, at any address.  The table is staged internally
 * as in the other _ptrs calls, so the caller may overwrite or free it as soon
 * as the call returns.  Every entry is checked, named by a mask or not (the
 * host never sees the masks).  With the masks on the device (ecg_csum.h:
 * ecg_csum_cells_ptrs over this table -> ecg_memset(masks, 0) -> ecg_csum_mask
 * (got = the old cells' slots, want = the new cells' slots) ->
 * ecg_update_masks_ptrs) the host need not know which cells changed.
 * masks, result, ECG_RM_SPARSE and what happens to a stripe are
 * ecg_update_masks's, word for word: m == 0 leaves the stripe untouched and
 * uncounted; a bit at or above k leaves it untouched and counts it in
 * result[3] and result[1]; any other m leaves parity_r ^= XOR_{j in m}
 * g[k+r][j] * (old_j ^ new_j), the bytes ecg_update_masks leaves on a
 * contiguous copy of that stripe, and nothing else is written.  All 2^32 mask
 * values are safe: an index into a table row is always j, k + j or 2k + r with
 * j a set bit of a word that has no bit at or above k.  result = {0,
 * UINT64_MAX, 0, 0} also for nstripes == 0 or cell_bytes == 0; INVALID MASKS
 * ARE REPORTED THROUGH result ONLY.  Limits k <= 16, p <= 8.
 * flags: ECG_RM_SPARSE, the same tuning hint and the same two grids.
 * ECG_UM_PACKED is refused: a table makes packing pointless, the caller puts
 * an address in slot j.
 * -ECG_DER_INVAL, the message prefixed "update_masks_ptrs:", checked in this
 * order: the k / p limits; an unknown flag, or ECG_UM_PACKED; masks NULL or
 * not 4-byte aligned; result NULL or not 8-byte aligned (both also for
 * nstripes == 0); a NULL context; cells NULL (nstripes and cell_bytes != 0); a
 * NULL entry (the message names its index); masks (4 * nstripes bytes) or
 * result (32 bytes) sharing a byte with any cell ("overlaps", with the cell's
 * index).
 * NOT CHECKED, THE CALLER'S CONTRACT: NO PARITY CELL OF THE TABLE MAY OVERLAP
 * ANY OTHER CELL THE LAUNCH READS OR WRITES -- THE PARITY CELLS OF ANOTHER ROW
 * INCLUDED: TWO STRIPES NAMING ONE PARITY CELL RACE -- AND EVERY CELL IS MEMORY
 * OF THE CONTEXT'S DEVICE.  Read-only duplicates are allowed: an old entry may
 * equal a new entry (that cell then contributes nothing), and old or new cells
 * may be shared between rows.
 * A table that is three strided groups -- old cell (s, j) at o0 + s*us + j*
 * cell_bytes, new cell (s, j) at n0 + s*us + j*cell_bytes with the same us,
 * parity (s, r) at p0 + s*ps + r*pc; one stripe whose cells are spaced so
 * always is -- and whose arguments pass ecg_update_masks's own checks (masks
 * and result clear of the whole parity span, gaps included) IS the call
 * ecg_update_masks(old = o0, new = n0, us, parity = p0, pc, ps): no table is
 * uploaded and ecg_last_kernel names that strided kernel.  Any other table
 * runs ecg_update_masks_ptr_kernel<R> (16-byte lanes) when every entry and
 * cell_bytes are multiples of 16, and ecg_update_masks_ptr_byte_kernel for the
 * WHOLE launch when one is not, or with ecg_set_launch variant 2;
 * ecg_set_launch's grid_x / grid_y override either grid.  Asynchronous on
 * `stream`.  Telemetry as ecg_update_masks: `launches` counts the launch,
 * update_cells / update_bytes are not advanced. */
int ecg_update_masks_ptrs(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
			  void *const *cells, const uint32_t *masks, void *result,
			  unsigned flags, void *stream);

/* ecg_update_masks with a ROUTE PER STRIPE: the delta update for a stripe that
 * changed few cells, a re-encode of the merged stripe for one that changed
 * many -- the choice aggregation makes per stripe between agg_update_parity
 * and agg_recalc_parity / a full-stripe encode (ref:src/object/
 * srv_ec_aggregate.c:1006-1138), made on the device from the mask words, so a
 * batch of mixed change counts stays one launch of the chain ecg_csum_extents
 * x2 -> ecg_csum_mask -> ecg_agg_masks -> ecg_csum_updated.  The delta moves
 * (2n + 2p) * cell_bytes for n changed cells, the re-encode (k + p) *
 * cell_bytes.
 * ecg_agg_masks takes ecg_update_masks's operands and ecg_agg_masks_ptrs
 * ecg_update_masks_ptrs's: old_cells, new_cells, parity, the three strides
 * (negative included), the client and the recovery layout, the table row of
 * 2k + p addresses and its staging (free when the call returns), masks,
 * result, ECG_RM_SPARSE, lane and byte kernels, ecg_set_launch, telemetry --
 * all as documented there.  What differs, for stripe s with m = masks[s], n =
 * popcount(m) and the threshold T:
 *   m == 0                    the stripe is untouched and not counted
 *   a bit at or above k set   untouched; counted in result[3] and result[1]
 *   1 <= n <= T   (delta)     byte for byte what ecg_update_masks leaves for
 *                             the stripe; only the named old and new cells and
 *                             the parity are read
 *   n > T         (recalc)    parity_r = XOR_{j<k} g[k+r][j] * (bit j of m ?
 *                             new_j : old_j) for r < p: byte for byte what
 *                             ecg_encode writes for the merged stripe.  THE OLD
 *                             PARITY IS NOT READ.  All k data cells are read,
 *                             each from one image: never both images of a cell,
 *                             never an unnamed new cell
 * T = recalc_above when it is 0 .. k: 0 re-encodes every stripe with work, k
 * none (the call is then ecg_update_masks).  ECG_AGG_AUTO: T =
 * ecg_agg_threshold(k, p) = (k - p) / 2 for k > p, else 0 -- the break-even of
 * the two traffic figures, a tie going to the delta.  Any other value is
 * -ECG_DER_INVAL.  ecg_agg_threshold is host arithmetic (-ECG_DER_INVAL outside
 * k 1..16, p 1..8).
 * What follows from the two routes:
 *  - They agree only when the stored parity matched the old data.  A recalc
 *    stripe comes out consistent whatever its old parity held; a delta stripe
 *    carries an old inconsistency forward.
 *  - old_cells == new_cells is allowed: delta stripes stay as they were,
 *    recalc stripes are re-encoded from the old data.
 *  - THE CALLER'S CONTRACT WIDENS (not checked): NO OLD OR NEW DATA CELL OF ANY
 *    STRIPE, NAMED BY ITS MASK OR NOT, MAY OVERLAP A PARITY CELL OF THE BATCH.
 *    (The recovery layout, old_cells = stripes, keeps it: data and parity cells
 *    interleave without sharing a byte.)
 *  - ECG_UM_PACKED is refused in both forms (-ECG_DER_INVAL): the recalc route
 *    needs the unnamed old cells in their slots.
 * result: ecg_update_masks's four words with the same meaning whichever route
 * a stripe took -- {stripes updated, lowest invalid, cells named by the
 * updated stripes, invalid stripes} -- so ecg_csum_updated / _ptrs follow with
 * the same masks; {0, UINT64_MAX, 0, 0} for nstripes == 0 or cell_bytes == 0.
 * Which route a stripe took follows from its mask and T and is not reported.
 * All 2^32 mask values are safe: the recalc route indexes j < k, never by mask
 * bits.
 * -ECG_DER_INVAL, prefixed "agg_masks:" / "agg_masks_ptrs:", in the order of
 * ecg_update_masks / ecg_update_masks_ptrs with the ECG_UM_PACKED refusal and
 * the recalc_above range right after the flags check (before masks, result,
 * the operands and the context).
 * Kernels: ecg_agg_masks_kernel<R> / ecg_agg_masks_byte_kernel, over a table
 * ecg_agg_masks_ptr_kernel<R> / ecg_agg_masks_ptr_byte_kernel (ecg_last_kernel);
 * a table that is three strided groups and passes the strided checks IS
 * ecg_agg_masks, as for ecg_update_masks_ptrs.  One launch; update_cells /
 * update_bytes are not advanced. */
#define ECG_AGG_AUTO 0xffffffffu
int ecg_agg_threshold(int k, int p);
int ecg_agg_masks(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
		  const void *old_cells, const void *new_cells, int64_t upd_stripe_stride,
		  void *parity, int64_t parity_cell_stride, int64_t parity_stripe_stride,
		  const uint32_t *masks, void *result, uint32_t recalc_above,
		  unsigned flags, void *stream);
int ecg_agg_masks_ptrs(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
		       void *const *cells, const uint32_t *masks, void *result,
		       uint32_t recalc_above, unsigned flags, void *stream);

/* Parity consistency check: does the stored parity of every stripe still
 * match its stored data -- what the EC branch of the object verify path
 * answers by re-encoding into scratch parity and memcmp
 * (ref:src/object/obj_verify.c) -- in one read-only pass that also says which
 * cell of a bad stripe is wrong.  Operands are addressed exactly as in
 * ecg_encode (client layout and the [S][k+p][C] recovery layout alike; the
 * strides may be negative, see ecg_recover_masks);
 * nothing is written to `data` or `parity`.  k <= 16, p <= 8 (every DAOS EC
 * class); any alignment and length (16-byte aligned cells of a multiple of
 * 16 bytes run the 16-byte lane kernel, everything else a byte-granular one).
 *
 * status[s] (device, nstripes words) describes stripe s:
 *   ECG_VERIFY_ROWS  bit r: stored parity row r differs from row r of G*data
 *                    at some byte
 *   ECG_VERIFY_CAND  bit j: data cell j being wrong, alone, explains every
 *                    differing byte seen (the syndrome s_r = parity_r ^
 *                    (G*data)_r equals g[r][j]*e at each of them; the Cauchy1
 *                    ratios g[r][j]/g[0][j] differ for every j, so at most one
 *                    j survives a real single-cell error); every j < k when
 *                    the stripe is clean
 * result (device, 4 x uint64, 8-byte aligned) = {bad stripes, lowest bad
 * stripe index (UINT64_MAX if none), bad stripes attributable to one cell,
 * bad stripes not attributable}; nstripes == 0 leaves {0, UINT64_MAX, 0, 0}.
 * Asynchronous on `stream`; status and result are valid once it has drained.
 *
 * Location ASSUMES AT MOST ONE WRONG CELL PER STRIPE.  That is inherent in a
 * distance-(p+1) code: two wrong cells can produce the syndrome of a third,
 * and with p == 1 a wrong parity row and a wrong data cell cannot be told
 * apart at all.  Detection (ROWS != 0) holds for up to p wrong cells.  The
 * located cells are rewritten by ecg_repair (below), queued behind this call
 * on the same stream: the status words never leave the device. */
#define ECG_VERIFY_ROWS(st)  ((st) & 0xffu)
#define ECG_VERIFY_CAND(st)  (((st) >> 8) & 0xffffu)
int ecg_verify(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
	       const void *data, int64_t data_stripe_stride,
	       const void *parity, int64_t parity_cell_stride, int64_t parity_stripe_stride,
	       uint32_t *status, void *result, void *stream);
/* Reading of one status word (host only): -1 clean; 0..k+p-1 the single cell
 * (data j, or parity k+r) that explains it -- one parity row alone differing
 * is that parity cell, all p rows differing with exactly one candidate is
 * that data cell; -2 not attributable to one cell (two or more cells wrong,
 * or p == 1, where a bad stripe never is). */
int ecg_verify_cell(uint32_t status, int k, int p);

/* Repair the stripes ecg_verify found bad and attributed to one cell -- the
 * second half of a scrub (the object verify path and the checksum scrubber):
 * ecg_verify, then ecg_repair, two asynchronous calls on one stream.
 * Operands addressed exactly as in ecg_verify / ecg_encode (client layout and
 * [S][k+p][C] alike; negative strides as in ecg_recover_masks).  status: the nstripes words an ecg_verify of the same
 * operands left (device, read only; it may not overlap the cells).  For
 * stripe s with c = ecg_verify_cell(status[s], k, p):
 *   c == -1 or -2   the stripe is not touched
 *   c >= k          parity row c-k  = row c-k of G * data
 *   c <  k          data cell c     = the decode row of erasure {c} over the
 *                   other k-1 data cells and parity row 0
 * i.e. byte for byte what ecg_recover(err_list = {c}, nerrs = 1) writes for
 * that one stripe, and nothing else is written.  Any status value is safe:
 * candidate bits at or above k and row bits at or above p classify as -2.
 * result (device, 4 x uint64, 8-byte aligned) = {stripes repaired, lowest bad
 * stripe left as it is (UINT64_MAX if none), data cells rewritten, bad stripes
 * left as they are}; nstripes == 0 or cell_bytes == 0 leaves {0, UINT64_MAX,
 * 0, 0}.  k <= 16, p <= 8; any alignment and length (16-byte aligned cells of
 * a multiple of 16 bytes run the 16-byte lane kernel, everything else a
 * byte-granular one).  The cost follows the number of bad stripes, not the
 * size of the batch.
 * Asynchronous on `stream`; queued behind the ecg_verify that wrote status it
 * needs no synchronisation in between.  status is never modified: run
 * ecg_verify again to confirm the repair.
 *
 * The caveats are ecg_verify's.  Location ASSUMES ONE WRONG CELL PER STRIPE.
 * With p == 1 nothing is ever attributable, so ecg_repair is a valid call
 * that repairs nothing.  With two or more wrong cells in a stripe a
 * distance-(p+1) code can MISCORRECT: the syndrome may be that of some third
 * cell, which is then rewritten to a different valid codeword (and the
 * second ecg_verify reports the stripe clean).  Callers who keep chunk
 * checksums (ecg_csum.h) should treat those as the authority. */
int ecg_repair(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
	       void *data, int64_t data_stripe_stride,
	       void *parity, int64_t parity_cell_stride, int64_t parity_stripe_stride,
	       const uint32_t *status, void *result, void *stream);
/* The row ecg_repair applies for `cell` (host only, no device needed): coef[k]
 * and src_idx[k], the logical cells (0..k+p-1) it reads.  cell >= k: the
 * Cauchy1 parity row over cells 0..k-1.  cell < k: slot i != cell reads data
 * cell i with g[0][i]/g[0][cell], slot `cell` reads parity row 0 (logical k)
 * with 1/g[0][cell] -- the coefficients and survivors of ecg_recov_matrix for
 * err_list = {cell}, which lists them in ascending cell order.
 * -ECG_DER_INVAL outside 0..k+p-1 or k/p out of range (k <= 16, p <= 8). */
int ecg_repair_row(int k, int p, int cell, unsigned char *coef, uint32_t *src_idx);

/* ecg_verify and ecg_repair over a TABLE OF CELL ADDRESSES, for callers whose
 * stripes are not one strided image -- the object verify path fetches every
 * shard of a stripe into a buffer of its own (ref:src/object/obj_verify.c).
 * cells is exactly the table of ecg_recover_masks_ptrs (below): a HOST array of
 * nstripes * (k+p) device addresses, cells[s*(k+p) + c] logical cell c of
 * stripe s (0..k-1 data, k..k+p-1 parity), cell_bytes long, at any address.
 * One table serves the whole scrub.  It is staged internally, so the caller
 * may overwrite or free it as soon as the call returns.  k <= 16, p <= 8.
 * status and result mean, word for word, what ecg_verify / ecg_repair define;
 * stripe s gives exactly what those calls give for a contiguous copy of that
 * stripe.  ecg_verify_ptrs writes nothing into any cell (aliased entries are
 * harmless for it).  ecg_repair_ptrs writes only the one located cell c of
 * each attributable stripe, the bytes ecg_recover(err_list = {c}) would write:
 * for a data cell from cells[s][j], j != c, and cells[s][k]; for a parity cell
 * from the k data cells.  Any status value is safe: every index into a
 * stripe's table row comes from the classified cell (ecg_verify_cell), never
 * from raw status bits.  nstripes == 0 leaves result {0, UINT64_MAX, 0, 0};
 * cell_bytes == 0 in addition presets the status words (ecg_verify_ptrs), as
 * the strided calls do.
 * ecg_scrub_ptrs is ecg_verify_ptrs then ecg_repair_ptrs on one stream, with
 * one pass over the table and one upload; verify_result and repair_result are
 * the two calls' result words (two different addresses).
 * -ECG_DER_INVAL, the message prefixed by the call's name, checked in this
 * order: the k / p limits; result NULL or not 8-byte aligned (ecg_scrub_ptrs:
 * verify_result, then repair_result, then the two being the same address);
 * status NULL or not 4-byte aligned (nstripes != 0); a NULL context; cells NULL
 * (nstripes and cell_bytes != 0); a NULL entry (the message names its index);
 * status (4 * nstripes bytes) or a result (32 bytes) sharing a byte with a
 * cell ("overlaps").
 * NOT CHECKED, THE CALLER'S CONTRACT: NO CELL ecg_repair_ptrs WRITES (THE
 * LOCATED CELL OF AN ATTRIBUTABLE STRIPE) MAY OVERLAP ANY OTHER CELL THE LAUNCH
 * READS OR WRITES, AND EVERY CELL IS MEMORY OF THE CONTEXT'S DEVICE.
 * A table in which cells[s*(k+p)+c] == cells[0] + s*stride + c*cell_bytes for
 * one stride (one stripe whose cells are cell_bytes apart is always such a
 * table), and whose arguments pass the strided call's own checks, IS the call
 * ecg_verify(data = cells[0], stride, parity = cells[0] + k*cell_bytes,
 * cell_bytes, stride) / ecg_repair of the same operands: no table is uploaded
 * and ecg_last_kernel names that kernel (ecg_repair demands status clear of
 * the whole image, gaps included; ecg_scrub_ptrs takes one route for both
 * halves, by that demand).  Any other table runs ecg_verify_ptr_kernel<K,P> /
 * ecg_repair_ptr_kernel<K> (16-byte lanes) when every entry and cell_bytes are
 * multiples of 16, and ecg_verify_ptr_byte_kernel / ecg_repair_ptr_byte_kernel
 * for the WHOLE launch when one is not, or with ecg_set_launch variant 2.
 * Asynchronous on `stream`.  Telemetry: `launches` counts 2 for
 * ecg_verify_ptrs (syndrome pass + summary), 1 for ecg_repair_ptrs and 3 for
 * ecg_scrub_ptrs; ecg_last_kernel names the syndrome kernel after
 * ecg_verify_ptrs and the repair kernel after the other two.  The caveats are
 * ecg_verify's and ecg_repair's: location ASSUMES ONE WRONG CELL PER STRIPE. */
int ecg_verify_ptrs(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
		    void *const *cells, uint32_t *status, void *result, void *stream);
int ecg_repair_ptrs(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
		    void *const *cells, const uint32_t *status, void *result, void *stream);
int ecg_scrub_ptrs(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
		   void *const *cells, uint32_t *status, void *verify_result, void *repair_result,
		   void *stream);

/* Recovery with one erasure set PER STRIPE, in one launch: a rebuild or
 * degraded-read batch whose stripes lost different shards, and the second
 * half of a checksum-driven scrub (ecg_csum.h: ecg_csum_extents ->
 * ecg_memset(masks, 0) -> ecg_csum_mask -> ecg_recover_masks, four
 * asynchronous calls on one stream; the masks never leave the device).
 * Operands as ecg_recover's: [S][k+p][C] in logical cell order, stripe s at
 * stripes + s*stripe_stride.  The stripe and cell strides of this call and of
 * the other mask-driven calls (ecg_verify, ecg_repair, ecg_update_masks,
 * ecg_csum_masked, ecg_recover_masks_csum) may be negative -- an image that
 * descends in address, stripe s below stripe s-1 -- as long as no two cells
 * overlap.  masks: device memory, nstripes words, 4-byte
 * aligned, read only, not overlapping the stripes (-ECG_DER_INVAL); bit c of
 * masks[s] = logical cell c of stripe s is erased.  With m = masks[s]:
 *   m == 0                      the stripe is not touched and not counted
 *   a bit at or above k+p set,  the stripe is not touched; it is counted in
 *   or more than p bits set     result[3] and result[1] -- the device-side form
 *                               of -ECG_DER_DATA_LOSS, the host never sees m
 *   otherwise                   byte for byte what ecg_recover(err_list = the
 *                               set bits of m in ascending order, nerrs =
 *                               popcount(m), nstripes = 1) writes for that
 *                               stripe (its survivors, rows and output order,
 *                               the all-parity shortcut included), nothing else
 * All 2^32 mask values are safe.  result (device, 4 x uint64, 8-byte aligned)
 * = {stripes recovered, lowest stripe left unrecoverable (UINT64_MAX if
 * none), cells regenerated, stripes left unrecoverable}; nstripes == 0 or
 * cell_bytes == 0 leaves {0, UINT64_MAX, 0, 0}.  UNRECOVERABLE STRIPES ARE
 * REPORTED THROUGH result ONLY: the call itself returns 0.
 * Limits: k <= 16 and p <= 3 (every DAOS EC class), -ECG_DER_INVAL beyond.  Any
 * alignment and length (16-byte aligned stripes and stride with cell_bytes %
 * 16 == 0 run the 16-byte lane kernel, everything else a byte-granular one).
 * flags: ECG_RM_SPARSE is a tuning hint and never changes a result -- few
 * stripes carry erasures (a scrub), so the launch uses the grid whose cost on
 * clean stripes is one mask load per 64 of them; without it every stripe is
 * expected to have work (a rebuild) and the grid is the product's.
 * ecg_set_launch's grid_x / grid_y override either grid; variant 2 forces
 * the byte kernel.  Asynchronous on `stream`.
 * Telemetry: ecg_get_stats' recover_stripes / recover_bytes are NOT advanced
 * (how many stripes had work is known on the device only: read result);
 * `launches` counts the launch.
 * The first call for a (k, p) on a context builds that shape's table of
 * erasure sets and uploads it synchronously (1.2 MB for k = 16, p = 3, the
 * largest; kept until ecg_ctx_destroy). */
#define ECG_RM_SPARSE 0x1u
int ecg_recover_masks(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
		      void *stripes, int64_t stripe_stride,
		      const uint32_t *masks, void *result, unsigned flags, void *stream);
/* ecg_recover_masks over a TABLE OF CELL ADDRESSES, for callers whose stripes
 * are not one strided image: rebuild's one buffer per stripe, the batching
 * queue's one stripe pointer per request, a degraded read whose cells lie
 * where the iovs put them.  cells: HOST array of nstripes * (k+p) device
 * addresses; cells[s*(k+p) + c] is logical cell c of stripe s (0..k-1 data,
 * k..k+p-1 parity), cell_bytes long, at any address.  The table is staged
 * internally as ecg_matmul_ptrs stages its own, so the caller may overwrite or
 * free it as soon as the call returns.
 * masks, result, flags (ECG_RM_SPARSE) and what happens to a stripe are
 * ecg_recover_masks's, word for word: m == 0 leaves the stripe untouched and
 * uncounted; a bit at or above k+p or more than p bits leaves it untouched and
 * counts it in result[3] and result[1]; any other m writes, byte for byte,
 * what ecg_recover(err_list = the set bits ascending, nstripes = 1) writes for
 * a contiguous copy of that stripe, and nothing else.  All 2^32 mask values
 * are safe: every index into a stripe's table row comes from the set-table
 * entry of a validated set index.  result = {0, UINT64_MAX, 0, 0} also for
 * nstripes == 0 or cell_bytes == 0; UNRECOVERABLE STRIPES ARE REPORTED THROUGH
 * result ONLY.  Limits k <= 16, p <= 3.
 * -ECG_DER_INVAL, checked in this order: the k / p limits; an unknown flag;
 * result NULL or not 8-byte aligned; masks NULL or not 4-byte aligned (nstripes
 * != 0); a NULL context; cells NULL (nstripes and cell_bytes != 0); a NULL
 * entry (the message names its index); masks (4 * nstripes bytes) or result
 * (32 bytes) lying inside a cell ("overlaps").
 * NOT CHECKED, THE CALLER'S CONTRACT: NO CELL THIS LAUNCH WRITES (AN ERASED
 * CELL OF A RECOVERABLE STRIPE) MAY OVERLAP ANY OTHER CELL THE LAUNCH READS OR
 * WRITES, AND EVERY CELL IS MEMORY OF THE CONTEXT'S DEVICE.
 * A table in which cells[s*(k+p)+c] == cells[0] + s*stride + c*cell_bytes for
 * one stride (one stripe whose cells are cell_bytes apart is always such a
 * table) IS the call ecg_recover_masks(stripes = cells[0], stripe_stride =
 * stride): no table is uploaded and ecg_last_kernel names that kernel.  Any
 * other table runs ecg_recover_masks_ptr_kernel<K, P> (16-byte lanes) when
 * every entry and cell_bytes are multiples of 16, and
 * ecg_recover_masks_ptr_byte_kernel for the WHOLE launch when one is not, or
 * with ecg_set_launch variant 2.  Asynchronous on `stream`.  Telemetry as
 * ecg_recover_masks: recover_stripes / recover_bytes not advanced, `launches`
 * counts the launch. */
int ecg_recover_masks_ptrs(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
			   void *const *cells, const uint32_t *masks, void *result,
			   unsigned flags, void *stream);
/* The erasure sets ecg_recover_masks knows for (k, p), host only: their
 * number N = sum_{e=1..p} C(k+p, e), and the index 0..N-1 of the set `mask`
 * names (by size, then combinatorial rank C(c1,1) + C(c2,2) + C(c3,3) of its
 * cells c1 < c2 < c3; a bijection).  ecg_erasure_set_index: -1 for mask 0,
 * -ECG_DER_DATA_LOSS for more than p bits, -ECG_DER_INVAL for a bit at or above
 * k+p; both -ECG_DER_INVAL for k > 16 or p > 3. */
int ecg_erasure_sets(int k, int p);
int ecg_erasure_set_index(int k, int p, uint32_t mask);

/* ---- host-resident pipeline (PCIe-inclusive) ---------------------------- */
/* One stripe, ISA-L ec_encode_data calling convention: pointers src[k],
 * dst[rows] (any alignment), `len` bytes each;
 * dst[r] (^)= XOR_j coef[r*k+j] * src[j], on ctx's GPU.  Host cells go
 * through per-thread pinned staging; device cells (src[0] hipMalloc'd: then
 * every cell must lie inside a device allocation, else -ECG_DER_INVAL) run
 * in place on one of the context's ECG_DROPIN_STREAMS (4) drop-in streams,
 * and the call waits only for its own launch.  Synchronous.  k may exceed
 * ECG_MAX_K (xor_gen: accumulating launches). */
int ecg_matmul_host(ecg_ctx_t *ctx, int len, int k, int rows, const unsigned char *coef,
		    unsigned char *const *src, unsigned char *const *dst, unsigned flags);
/* ---- CPU product and drop-in routing (host memory) ----------------------
 * The same product on the calling CPU thread (host pointers only; no device
 * needed): vgf2p8affineqb with AVX-512 or AVX2 GFNI, vpshufb nibble tables
 * with AVX2, byte tables otherwise (widest the CPU has; ecg_cpu_set_isa /
 * $ECG_CPU_ISA choose a narrower one: "avx512-gfni", "avx2-gfni", "avx2",
 * "scalar", "auto").  k <= ECG_MAX_K + 256, rows <= 256.  Synchronous. */
int ecg_cpu_matmul(int len, int k, int rows, const unsigned char *coef,
		   unsigned char *const *src, unsigned char *const *dst, unsigned flags);
const char *ecg_cpu_isa(void);
int ecg_cpu_set_isa(const char *isa);
/* Where the drop-in surfaces (ecg_isal.h data-plane calls, and the
 * synchronous one-stripe calls of ecg_daos.h) run a call: device cells on
 * the GPU; host cells on the CPU when len * (k + rows) is below this
 * crossover (bytes), when the process has no usable gfx950 device, or with
 * $ECG_FORCE_CPU=1; otherwise on the GPU through pinned staging.  Default:
 * the measured crossover, $ECG_DROPIN_CROSSOVER overrides;
 * 0 = host cells always on the GPU, UINT64_MAX = never. */
int ecg_set_dropin_crossover(uint64_t bytes);
uint64_t ecg_dropin_crossover(void);

/* Encode host-resident stripes (data [S][k][C], parity [p][S][C] in host
 * memory; pinned memory from ecg_host_alloc is fastest) by streaming chunks
 * of `chunk_stripes` through device staging on 3 rotating streams
 * (H2D / kernel / D2H overlap); 0 = about 32 MiB of input cells per chunk.
 * Synchronous. */
int ecg_encode_host(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
		    const void *data, void *parity, uint32_t chunk_stripes);
/* Same for recovery over host [S][k+p][C] stripes: only survivors travel
 * H2D, only regenerated cells travel D2H.  Synchronous. */
int ecg_recover_host(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
		     void *stripes, const uint32_t *err_list, int nerrs,
		     uint32_t chunk_stripes);

/* ---- batching facade for one-stripe callers ------------------------------
 * Every reference caller issues ONE stripe per codec call (client write
 * ref:src/object/cli_ec.c:627-659, rebuild ref:src/object/srv_obj_migrate.c:
 * 1116-1177, aggregation ULTs on the offload xstream ref:src/object/
 * srv_ec_aggregate.c:701-734).  An ecg_queue accepts such requests from any
 * number of threads, coalesces compatible ones (same op, k, p, cell size and
 * erasure set) into one device batch, and completes each request through its
 * callback -- the place DAOS sets its ABT_eventual (srv_ec_aggregate.c:696).
 * Host buffers must stay valid until the callback runs.  Callbacks run on the
 * queue's completion threads and must not block on the queue.
 * Cells may be host memory or device memory of one of the queue's devices.
 * Host cells go where the ISA-L drop-in would send them: below its crossover
 * (ecg_set_dropin_crossover; with a GFNI CPU, every size) the queue's
 * completion threads compute them in place on the CPU path -- such a batch
 * closes while a completion thread is free if it is the queue's only work or
 * holds a request per free thread, so a lone request does not wait
 * max_wait_us -- else they are staged through the queue's pinned slots (PCIe
 * both ways).  Device cells (k <= 16): such requests batch into one
 * pointer-table launch on the cells in place (updates: one ecg_update_ptrs
 * call), and a batch launches as soon as the device has fewer than 2 of the
 * queue's batches in flight -- a lone request does not wait either.  A request's cells are all host memory or all
 * memory of one device (-ECG_DER_INVAL naming the odd cell otherwise). */
typedef struct ecg_queue ecg_queue_t;
typedef void (*ecg_done_cb_t)(void *arg, int rc);

typedef struct ecg_queue_attr {
	uint32_t max_batch;	/* stripes per device batch (default 256) */
	uint32_t max_wait_us;	/* longest a request waits for company (default 50) */
	uint64_t max_cell_bytes; /* staging sized for this cell size (default 1 MiB) */
} ecg_queue_attr_t;

/* attr may be NULL for defaults.  ctx NULL (or $ECG_FORCE_CPU=1): the CPU
 * executor -- the same requests, batching and callbacks with no device, the
 * products computed on the queue's completion threads by the CPU path
 * straight from the callers' cells, nothing staged (host cells only; a
 * GPU-less process can use the facade). */
int ecg_queue_create(ecg_ctx_t *ctx, const ecg_queue_attr_t *attr, ecg_queue_t **q);
/* Drains outstanding requests (their callbacks run) then frees the queue. */
void ecg_queue_destroy(ecg_queue_t *q);
/* Encode one stripe: data[k] -> parity[p] (cell_bytes each; host, or device
 * memory of one of the queue's devices). */
int ecg_queue_encode(ecg_queue_t *q, int k, int p, uint64_t cell_bytes,
		     unsigned char *const *data, unsigned char *const *parity,
		     ecg_done_cb_t cb, void *arg);
/* Recover one stripe in place: `stripe` is [k+p][cell_bytes] in logical cell
 * order (host, or device memory of one of the queue's devices); err_list
 * holds the erased logical cells. */
int ecg_queue_recover(ecg_queue_t *q, int k, int p, uint64_t cell_bytes, unsigned char *stripe,
		      const uint32_t *err_list, int nerrs, ecg_done_cb_t cb, void *arg);
/* Aggregation delta update of one stripe's parity (agg_update_parity:
 * xor_gen(old, new -> diff) then ec_encode_data_update(vec_i), ref:src/object/
 * srv_ec_aggregate.c:1086-1102):  parity[r] ^= coef[r][vec_i] * (old ^ new)
 * for the p parity cells (updated in place when the callback runs).  Requests
 * of one (k, p, cell size) batch together whatever their vec_i.  k <= 16.
 * Host cells: on the CPU path the deltas are computed and XORed into the
 * parity on the completion threads; staged, old ^ new crosses PCIe and the
 * deltas are XORed in on the host.
 * Device cells: ecg_update_ptrs batches in place -- requests naming the same
 * parity cells fold into one pass, and the update batches of one device run
 * in order, so concurrent updates of one stripe never lose a delta; a batch
 * ecg_update_ptrs refuses (an old / new cell overlapping a parity cell of
 * the batch) runs its requests one by one, each with its own result.  An
 * old / new cell that is another pending request's parity is read before or
 * after that request's delta, whichever ran first. */
int ecg_queue_update(ecg_queue_t *q, int k, int p, uint64_t cell_bytes, int vec_i,
		     const unsigned char *old_cell, const unsigned char *new_cell,
		     unsigned char *const *parity, ecg_done_cb_t cb, void *arg);
/* Block until every request submitted before the call has completed. */
int ecg_queue_flush(ecg_queue_t *q);
/* Counters: requests completed, device batches launched. */
int ecg_queue_stats(ecg_queue_t *q, uint64_t *requests, uint64_t *batches);

/* ---- memory / streams / timing plumbing --------------------------------- */
int ecg_dev_alloc(ecg_ctx_t *ctx, size_t bytes, void **ptr);
int ecg_dev_free(ecg_ctx_t *ctx, void *ptr);
int ecg_host_alloc(ecg_ctx_t *ctx, size_t bytes, void **ptr);	/* pinned */
int ecg_host_free(ecg_ctx_t *ctx, void *ptr);
/* kind: 0 H2D, 1 D2H, 2 D2D, 3 default (runtime infers). Async on stream. */
int ecg_memcpy(ecg_ctx_t *ctx, void *dst, const void *src, size_t bytes, int kind, void *stream);
int ecg_memset(ecg_ctx_t *ctx, void *dst, int value, size_t bytes, void *stream);
int ecg_stream_create(ecg_ctx_t *ctx, void **stream);
int ecg_stream_destroy(ecg_ctx_t *ctx, void *stream);
int ecg_stream_sync(ecg_ctx_t *ctx, void *stream);
int ecg_event_create(ecg_ctx_t *ctx, void **event);
int ecg_event_destroy(ecg_ctx_t *ctx, void *event);
int ecg_event_record(ecg_ctx_t *ctx, void *event, void *stream);
int ecg_event_elapsed_ms(ecg_ctx_t *ctx, void *start, void *stop, float *ms);
int ecg_device_sync(ecg_ctx_t *ctx);
/* Streaming kernels (16 B/lane) used to measure the achievable HBM rate:
 * mode 0 copy src->dst, 1 read-only (dst receives 16 B per thread of the
 * launch, <= 8 MiB), 2 write-only (fills dst).  ecg_set_launch's grid_x, when
 * set, caps the block count (default: one 4 x 16 B slice per thread). */
int ecg_dev_copy_kernel(ecg_ctx_t *ctx, void *dst, const void *src, size_t bytes, int mode,
			void *stream);

/* ---- telemetry ------------------------------------------------------------
 * The engine counts EC full-stripe and partial updates with GURT telemetry
 * (opm_update_ec_full / _partial, ref:src/object/srv_ec.c:21-87); the codec's
 * own counters, per context since creation or the last reset (relaxed
 * atomics: safe from any thread, a snapshot is not one consistent instant):
 *   encode_*   full-stripe products: stripes and user-data bytes (k*C*S)
 *   recover_*  regenerations: stripes and regenerated bytes (nerrs*C*S)
 *   update_*   partial-stripe parity updates: updated cells and their bytes
 *   csum_chunks  checksums computed (standalone and fused)
 *   launches   codec kernel launches (product, fused, checksum)
 *   h2d_bytes / d2h_bytes  cell bytes the host-resident pipelines and the
 *              batching queue moved over PCIe
 * The batching queue counts its batches on the context of the slot that ran
 * them (encode / recover / update rows above, and launches). */
typedef struct ecg_stats {
	uint64_t encode_stripes, encode_bytes;
	uint64_t recover_stripes, recover_bytes;
	uint64_t update_cells, update_bytes;
	uint64_t csum_chunks;
	uint64_t launches;
	uint64_t h2d_bytes, d2h_bytes;
} ecg_stats_t;
/* Copy the counters to *out (may be NULL) and, if reset != 0, zero them. */
int ecg_get_stats(ecg_ctx_t *ctx, ecg_stats_t *out, int reset);

/* ---- launch tuning (benchmarks; 0 = default) ----------------------------
 * variant: 0 auto, 1 runtime-shaped kernel, 2 byte kernel, 3 dword lanes
 * whatever the operands' alignment (misaligned dword accesses served by the
 * hardware's unaligned access mode; A/B only). */
int ecg_set_launch(ecg_ctx_t *ctx, uint32_t grid_x, uint32_t grid_y, uint32_t variant);
/* Block -> (stripe, 4 KiB column) mapping of the product kernel: 0 = 2D
 * grid (columns x stripes, default); 1 = 1D stripe-fastest; 2 = 1D with each
 * XCD streaming its own eighth of the column-fastest items; 3 = as 2,
 * stripe-fastest.  Tuning only; results never depend on it. */
int ecg_set_launch_order(ecg_ctx_t *ctx, uint32_t order);
/* Blocks per CU of the product kernel's 2D grid: 0 = the per-shape default
 * (currently no cap for any shape), 2..16 = that cap, 255 = no cap.  Enforced
 * with unused dynamic LDS.  Tuning only; results never depend on it. */
int ecg_set_wg_per_cu(ecg_ctx_t *ctx, uint32_t wg_per_cu);
/* Launch tuner (on by default; ECG_AUTOTUNE=0 in the environment turns it off
 * for new contexts): the first 23 product launches of each wide shape (k >= 16,
 * > 2048 blocks) in a context run 4 uncapped then 19 at the candidate cap (2
 * blocks per CU), the last 3 of each arm timed with events on the
 * stream of the launch that started the probe (a switch to a cap runs slow for
 * its first ~10-20 launches); once every timing has completed the faster time
 * per block is kept for the shape (the cap only when it wins by > 1.5 %).  A
 * shape is (k, rows, acc/diff, cell bytes, lane granule, layout class:
 * source and destination sharing one stripe stride or not, or a pointer
 * table from ecg_matmul_ptrs / ecg_obj_ec_recx_encode) -- NOT the batch
 * size, so batches of varying size share one probe and one decision.  Skipped
 * when ecg_set_wg_per_cu or ecg_set_launch / _order set a geometry, and on
 * streams under graph capture.  on: 0 off, 1 on, 2 on and forget every
 * decision (and the counters).  Tuning only; results never depend on it. */
int ecg_set_autotune(ecg_ctx_t *ctx, int on);
/* The tuner's state of a shape (k inputs, rows outputs, acc/diff off, the
 * launch's source and destination stripe strides -- encode: k*C and the
 * parity stripe stride; in-place recovery: (k+p)*C both): 1 decided (*cap =
 * the cap, or 255 = none; both arms' median times per block, scaled to a
 * launch of nstripes stripes), 0 still probing or not seen.  nstripes is not part of the shape (it only has to
 * make the launch tunable, > 2048 blocks, to have been probed). */
int ecg_tune_state(ecg_ctx_t *ctx, int k, int rows, uint64_t cell_bytes, uint32_t nstripes, int64_t sstride,
		   int64_t dstride, uint32_t *cap, float *ms_uncapped, float *ms_capped);
/* The tuner's counters since the context was created (or ecg_set_autotune(ctx,
 * 2)): probe cycles started, launches that ran inside a probe, shapes held. */
int ecg_tune_counters(ecg_ctx_t *ctx, uint64_t *probe_cycles, uint64_t *probe_launches, uint32_t *shapes);

/* Pointer-table product: ISA-L's per-stripe pointer arrays
 * (ec_encode_data(len, k, rows, tbls, data[], coding[])) batched over
 * nstripes.  cells[s*(k+rows) + j] is the DEVICE address of input cell j
 * (j < k) or output cell j-k of stripe s; the table itself is a host array
 * (copied before return is not required: it is staged internally).  k <= 16,
 * rows <= 8; any alignment.  A table whose cells sit at fixed offsets from a
 * per-stripe base (cell j of stripe s at cells[j] + s*stride, one stride for
 * the inputs, one for the outputs -- a contiguous client buffer) runs as the
 * strided product (ecg_matmul) with no table upload.  Asynchronous on
 * `stream`. */
int ecg_matmul_ptrs(ecg_ctx_t *ctx, int k, int rows, const unsigned char *coef,
		    uint64_t cell_bytes, uint32_t nstripes, void *const *cells, void *stream);

/* ecg_matmul_ptrs with a cell length per stripe: cells is the same table, and
 * cell_bytes[s] (a host array) the length of every cell of stripe s -- single
 * values of an EC class, whose cell size follows the value's (ecg_daos.h
 * ecg_obj_ec_singv_encode_dev), rebuild batches across record sizes, an
 * object's short last extent.  Stripe s gets the bytes ecg_matmul_ptrs(
 * cell_bytes[s], nstripes = 1) writes for its row; no byte at or past
 * cell_bytes[s] of an output cell is written.  A stripe of length 0 is skipped:
 * its entries are not looked at and may be NULL; all lengths 0 or nstripes = 0
 * returns 0 and launches nothing.  k <= 16, rows <= 8, any address, any length
 * (below 2^44).  The table, the lengths and the launch plan are staged
 * internally in one upload, so the host arrays are free when the call returns.
 * Asynchronous on `stream`.
 * A batch whose lengths are all the same and none 0 IS ecg_matmul_ptrs with
 * that length (same route, same kernel, the affine shortcut included).  Any
 * other takes one launch of ecg_mm_ptr_lens_kernel: the host cuts every stripe
 * into spans of ECG_LENS_SPAN_BYTES and a block row takes a span, so small
 * stripes cost one block each and long ones a block per 4 KiB column.  The
 * lanes follow the addresses of the stripes that are not skipped as for
 * ecg_matmul_ptrs, with 16-byte lanes only when every length is a multiple of
 * 16.  The launch takes no part in the launch tuner (whose shape includes the
 * cell size); ecg_set_launch's grid_x / grid_y override its grid and variant
 * 2 forces the byte kernel.  Telemetry: one of `launches`.
 * -ECG_DER_INVAL ("matmul_ptrs_lens: ..."), checked in this order: k / rows
 * out of range; coef NULL; cell_bytes NULL with nstripes != 0; a NULL
 * context; cells NULL; a NULL entry in a stripe of non-zero length (the message
 * names its index).  Output cells overlapping anything else are the caller's
 * contract, as for ecg_matmul_ptrs.
 * ecg_lens_plan is the launch plan, host arithmetic only: a stripe of length L
 * contributes ceil(L / ECG_LENS_SPAN_BYTES) spans to *nspans, and *max_cols is
 * the most 4 KiB columns any span holds (1 .. 16; 0 when there is no span).
 * -ECG_DER_INVAL for a NULL pointer with nstripes != 0. */
#define ECG_LENS_SPAN_BYTES 65536u   /* 16 columns of 4 KiB: the unit of the launch plan */
int ecg_matmul_ptrs_lens(ecg_ctx_t *ctx, int k, int rows, const unsigned char *coef,
			 uint32_t nstripes, void *const *cells, const uint64_t *cell_bytes,
			 void *stream);
int ecg_lens_plan(const uint64_t *cell_bytes, uint32_t nstripes, uint64_t *nspans, uint32_t *max_cols);

/* Per-request delta parity updates on DEVICE cells: agg_update_parity's
 * xor_gen(old, new) + ec_encode_data_update(vec_i) of one updated data cell
 * (ref:src/object/srv_ec_aggregate.c:1086-1102), nreq requests in one call:
 *   parity_r ^= coef[r][vec_i[i]] * (old ^ new)        r < p
 * with the codec's Cauchy parity rows.  cells[i*(2+p) + 0] = old cell,
 * + 1 = new cell, + 2 + r = parity cell r of request i (device addresses,
 * cell_bytes each, any alignment).  Requests may name the same parity cells
 * (several cells of one stripe) or overlapping ones: the result is every
 * request applied, as if one after another.  Requests naming the same parity
 * cells are folded into one pass over that parity; the rest run in as few
 * ordered launches as keep every parity byte's read-modify-writes apart.  An
 * old/new cell must not overlap a parity cell of the call; one request's
 * parity cells must not overlap one another (-DER_INVAL).  k <= 16, p <= 8.
 * The table is a host array, staged internally.  Asynchronous on `stream`. */
int ecg_update_ptrs(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nreq,
		    void *const *cells, const uint8_t *vec_i, void *stream);

#ifdef __cplusplus
}
#endif
#endif
