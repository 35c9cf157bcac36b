/*
 * ecg_csum.h -- chunked checksums of device-resident extents, DAOS csummer
 * semantics (checksums on regenerated parity and
 * recovered cells).
 *
 * Replaces, for data already in HBM, the checksum step DAOS runs right after
 * the codec on the rebuild path:
 *   daos_csummer_calc_iods(csummer, &sgl, iod, ...)
 *       ref:src/object/srv_obj_migrate.c:1156 (regenerated parity cells)
 *   -> calc_csum_recx -> calc_csum_recx_with_no_map
 *       ref:src/common/checksum.c:631-664, 467-497
 * with the hash functions DAOS registers (ref:src/common/multihash_isal.c):
 *   ECG_HASH_CRC16   crc16_t10dif      (:27-82)
 *   ECG_HASH_CRC32   crc32_iscsi       (:84-139)
 *   ECG_HASH_CRC64   crc64_ecma_refl   (:195-257)
 *   ECG_HASH_ADLER32 isal_adler32      (:140-193)
 * each reset to 0 before every chunk.  The cryptographic types (SHA1/256/512,
 * ref:src/include/daos/multihash.h:27-29) are not provided: -DER_NOTSUPPORTED.
 *
 * Checksums are written little-endian, csum_len bytes each, extent-major
 * ([n_ext][nchunks]) -- the layout of dcs_csum_info.cs_csum for one recx
 * (ci_idx2csum, ref:src/common/checksum.c:1203-1220).
 */
#ifndef ECG_CSUM_H
#define ECG_CSUM_H

#include <stdint.h>

#include "ecg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* enum DAOS_HASH_TYPE values, ref:src/include/daos/multihash.h:22-33 */
#define ECG_HASH_CRC16		1
#define ECG_HASH_CRC32		2
#define ECG_HASH_CRC64		3
#define ECG_HASH_ADLER32	7

#define ECG_DER_NOTSUPPORTED	2037

/* Checksum length in bytes (daos_csummer_get_csum_len): 2, 4, 8 or 4;
 * -ECG_DER_NOTSUPPORTED for other types. */
int ecg_csum_len(int type);

/* Chunk bytes for a record size (csum_record_chunksize,
 * ref:src/common/checksum.c:1475-1482). */
uint64_t ecg_csum_record_chunksize(uint64_t chunksize, uint64_t rec_size);

/* Number of checksums of one extent (daos_recx_calc_chunks,
 * ref:src/common/checksum.c:1444-1454). */
uint32_t ecg_csum_chunk_count(uint64_t chunksize, uint64_t rec_size, uint64_t rx_idx,
			      uint64_t rx_nr);

/* Checksum n_ext extents on the device.  Extent e holds rx_nr records of
 * rec_size bytes at buf + e * ext_stride and starts at record index rx_idx
 * (the same index for every extent: chunk boundaries fall on multiples of the
 * record chunk size in index space).  csums: device memory for
 * n_ext * ecg_csum_chunk_count(...) * ecg_csum_len(type) bytes, aligned to
 * ecg_csum_len(type): every checksum is written with one store of its own
 * width (ecg_csum_masked, below, takes csums at any byte).  buf, ext_stride and
 * the sizes may be anything; all of them multiples of 16 run the faster
 * kernels.  Asynchronous on `stream` (NULL = the context stream).  Returns 0
 * or a negative errno. */
int ecg_csum_extents(ecg_ctx_t *ctx, int type, uint64_t chunksize, uint64_t rec_size,
		     uint64_t rx_idx, uint64_t rx_nr, const void *buf, int64_t ext_stride,
		     uint32_t n_ext, void *csums, void *stream);

/* Encode with checksums of the parity cells it writes, in one pass: the same
 * operands as ecg_encode (include/ecg.h), plus the hash type, the csummer's
 * chunk size and record size (cell_bytes must be a multiple of rec_size;
 * every parity cell is checksummed as an extent that starts on a chunk
 * boundary, as DAOS cells do when the cell's record count is a multiple of
 * the chunk's).  csums: device memory, [p][nstripes][nch] checksums of
 * ecg_csum_len(type) bytes, nch = ecg_csum_chunk_count(chunksize, rec_size, 0,
 * cell_bytes / rec_size).  Replaces obj_ec_encode_buf + daos_csummer_calc_iods
 * on the rebuild path (ref:src/object/srv_obj_migrate.c:1122-1160).
 * CRC types with a 4 KiB-multiple record chunk and 16-byte aligned cells run
 * as one fused kernel that never re-reads the parity; other shapes run the
 * product and ecg_csum_extents back to back on the stream. */
int ecg_encode_csum(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
		    const void *data, int64_t data_stripe_stride, void *parity,
		    int64_t parity_cell_stride, int64_t parity_stripe_stride, int type,
		    uint64_t chunksize, uint64_t rec_size, void *csums, void *stream);

/* Recover erased cells in place (as ecg_recover) and checksum them:
 * csums[nerrs][nstripes][nch] in err_list order (degraded-read / rebuild of
 * data cells, ref:src/object/cli_ec.c:2626-2643 then the csummer). */
int ecg_recover_csum(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
		     void *stripes, int64_t stripe_stride, const uint32_t *err_list, int nerrs,
		     int type, uint64_t chunksize, uint64_t rec_size, void *csums, void *stream);

/* ecg_encode_csum + checksums of the data cells it reads:
 * data_csums[k][S][nch], parity_csums[p][S][nch].  What the client's
 * full-stripe write needs after obj_ec_req_reasb encodes: obj_csum_update
 * checksums the whole reassembled request (ref:src/object/cli_obj.c:6306).
 * One kernel (the data pieces are checksummed from the registers the product
 * reads them into) for the shapes where that was measured faster than two
 * passes; otherwise ecg_encode_csum followed by ecg_csum_extents over every
 * data cell, on the stream (ecg_set_csum_all_route). */
int ecg_encode_csum_all(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
			const void *data, int64_t data_stripe_stride, void *parity,
			int64_t parity_cell_stride, int64_t parity_stripe_stride, int type,
			uint64_t chunksize, uint64_t rec_size, void *data_csums, void *parity_csums,
			void *stream);

/* ecg_recover_csum + checksums of the k surviving cells it reads:
 * src_csums[k][S][nch], row i being cell src_idx[i] of the stripe (src_idx: host array of k
 * entries, filled before return).  nerrs == 0: returns 0 and touches nothing.
 * A degraded read compares src_csums with the survivors' stored checksums
 * (ecg_csum_compare) before it trusts the regenerated cells. */
int ecg_recover_csum_all(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
			 void *stripes, int64_t stripe_stride, const uint32_t *err_list, int nerrs,
			 int type, uint64_t chunksize, uint64_t rec_size, void *csums, void *src_csums,
			 uint32_t *src_idx, void *stream);

/* Compare n checksums of ecg_csum_len(type) bytes on the device.  result: device memory for
 * two uint64 (8-byte aligned) -- the number of mismatches and the lowest mismatching index
 * (UINT64_MAX if none).  Asynchronous on `stream`. */
int ecg_csum_compare(ecg_ctx_t *ctx, int type, const void *got, const void *want, uint64_t n,
		     void *result, void *stream);

/* Which cells of which stripes have a wrong checksum: the erasure masks of
 * ecg_recover_masks (ecg.h), written on the device.  got / want: checksums of
 * ecg_csum_len(type) bytes (2, 4 or 8); masks: device memory, nstripes words,
 * 4-byte aligned.
 *   masks[s] |= 1u << (first_cell + i)   for s < nstripes, i < ncells
 * when any of the nch checksums at index s*stripe_stride + i*cell_stride + c
 * (c < nch; strides in checksums, not bytes) differs between got and want.  It
 * ORs into masks: zero them first (ecg_memset), then
 *   two calls cover the separate data and parity arrays of
 *     ecg_encode_csum_all, [cell][S][nch]: cell_stride = S*nch, stripe_stride
 *     = nch; (first_cell, ncells) = (0, k) and (k, p);
 *   one call covers ecg_csum_extents over a recovery-layout image,
 *     [S][k+p][nch]: stripe_stride = (k+p)*nch, cell_stride = nch.
 * The scrub ecg_verify / ecg_repair cannot do (p = 1; two or three wrong cells
 * per stripe): ecg_csum_extents -> ecg_memset(masks) -> ecg_csum_mask ->
 * ecg_recover_masks on one stream, no host round trip.
 * -ECG_DER_INVAL when first_cell + ncells > 32, the hash type has no such
 * checksum, or masks is NULL or misaligned.  Asynchronous on `stream`. */
int ecg_csum_mask(ecg_ctx_t *ctx, int type, const void *got, const void *want,
		  uint32_t nstripes, uint32_t ncells, uint32_t nch,
		  uint64_t stripe_stride, uint64_t cell_stride,
		  uint32_t first_cell, uint32_t *masks, void *stream);

/* Checksum only the cells each stripe's mask word names: the step after
 * ecg_recover_masks (ecg.h), whose operands these are -- stripes [S][k+p][C] in
 * logical cell order, stripe s at stripes + s*stripe_stride (negative strides
 * as there), masks device words; both read only.  With m = masks[s], and m valid when it is a set of
 * 1 .. p cells below k + p (ecg_erasure_set_index(k, p, m) >= 0), the cells
 * checksummed are
 *   none                                            m not valid (0 included)
 *   ECG_CM_ERASED     the cells m names: what ecg_recover_masks wrote
 *   ECG_CM_SURVIVORS  the k lowest cells m does not name: what it read
 *                     (ecg_recov_matrix's dec_idx for the set in ascending order)
 * csums: device memory [S][k+p][nch], ecg_csum_len(type) bytes each, nch =
 * ecg_csum_chunk_count(chunksize, rec_size, 0, cell_bytes / rec_size) -- the
 * stripe-major layout of ecg_csum_mask (stripe_stride = (k+p)*nch, cell_stride
 * = nch).  The nch slots of a selected cell receive its checksums, the cell
 * taken as an extent from record index 0 as ecg_recover_csum takes it; no
 * other byte of csums is written.  result: device memory, four uint64 (8-byte
 * aligned): stripes with a valid set, lowest stripe whose non-zero mask is not
 * valid (UINT64_MAX if none), cells checksummed, stripes whose non-zero mask is
 * not valid -- with which = ECG_CM_ERASED the words ecg_recover_masks leaves
 * for the same masks; {0, UINT64_MAX, 0, 0} when nstripes or cell_bytes is 0.
 * k <= 16, p <= 3; which = 1, 2 or 3; cell_bytes % rec_size == 0; masks
 * non-NULL and 4-byte aligned; csums must not overlap the stripes or the
 * masks: otherwise -ECG_DER_INVAL (hash types other than the four above:
 * -ECG_DER_NOTSUPPORTED).  Cells, strides and csums may lie at any byte.
 * flags: ECG_RM_SPARSE is accepted and changes nothing (one launch shape
 * serves dense and clean batches).  ecg_set_csum_launch caps the workgroups.
 * Asynchronous on `stream`.  Telemetry: `launches` counts the launch;
 * `csum_chunks` is not advanced, the count being known on the device only
 * (result word 2 times nch). */
#define ECG_CM_ERASED		0x1u
#define ECG_CM_SURVIVORS	0x2u
int ecg_csum_masked(ecg_ctx_t *ctx, int type, uint64_t chunksize, uint64_t rec_size,
		    int k, int p, uint64_t cell_bytes, uint32_t nstripes,
		    const void *stripes, int64_t stripe_stride, const uint32_t *masks,
		    unsigned which, void *csums, void *result, unsigned flags, void *stream);

/* ecg_recover_masks, then ecg_csum_masked(ECG_CM_ERASED) into csums, on one
 * stream: rebuild of a batch with one erasure set per stripe and the checksums
 * of the regenerated cells (daos_csummer_calc_iods after the codec,
 * ref:src/object/srv_obj_migrate.c:1156).  src_csums != NULL: also
 * ECG_CM_SURVIVORS into src_csums, the checksums a degraded read compares with
 * the survivors' stored ones (ecg_csum_compare / ecg_csum_mask); src_csums ==
 * csums is allowed (the slots are disjoint) and runs as one launch, any other
 * overlap of the two is -ECG_DER_INVAL.  result: ecg_recover_masks's four
 * words.  The argument errors of both halves are returned before anything is
 * queued. */
int ecg_recover_masks_csum(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
			   void *stripes, int64_t stripe_stride, const uint32_t *masks, void *result,
			   unsigned flags, int type, uint64_t chunksize, uint64_t rec_size,
			   void *csums, void *src_csums, void *stream);

/* ecg_csum_masked over a TABLE OF CELL ADDRESSES, the step after
 * ecg_recover_masks_ptrs (ecg.h), whose table this is: cells, a HOST array of
 * nstripes * (k + p) device addresses, cells[s*(k+p) + c] = logical cell c of
 * stripe s, each cell_bytes long and at any byte.  The table is copied before
 * the call returns (the caller may overwrite or free it at once).  The cells
 * are read only: duplicate entries and overlapping cells are allowed.
 * Everything else is ecg_csum_masked's, word for word: the cells
 * ecg_csum_masked_sel picks for masks[s] and `which`, the [S][k+p][nch] slots of
 * csums (at any byte; no byte outside the selected cells' slots is written),
 * the four result words, {0, UINT64_MAX, 0, 0} when nstripes or cell_bytes is
 * 0, ECG_RM_SPARSE accepted and ignored, ecg_set_csum_launch, `launches`
 * advanced and `csum_chunks` not.  Every table index derives from the selection,
 * which is empty for a word that is no valid set: all 2^32 mask values are safe,
 * and a stripe with an invalid or zero mask reads no table entry.
 * Errors, -ECG_DER_INVAL unless noted, in this order: ecg_csum_masked's own
 * argument checks in its order and words (-ECG_DER_NOTSUPPORTED for an unknown
 * hash type); a NULL context; cells == NULL with nstripes and cell_bytes
 * non-zero; a NULL entry (named by its index; every entry is checked, selected
 * or not); csums, masks or result sharing a byte with a cell ("overlaps", and
 * the cell's index); csums overlapping masks.
 * A table with cells[s*(k+p)+c] == cells[0] + s*stride + c*cell_bytes for one
 * stride (negative too; one stripe always) whose arguments pass
 * ecg_csum_masked's checks IS the call ecg_csum_masked(stripes = cells[0],
 * stripe_stride = stride): no table is uploaded and ecg_last_kernel names the
 * strided kernel.  Any other table runs ecg_crc_masked_ptr_kernel<type> /
 * ecg_adler_masked_ptr_kernel with 16-byte loads when EVERY entry, cell_bytes
 * and the record chunk size are multiples of 16, and their <..bytes> forms for
 * the WHOLE launch when one is not. */
int ecg_csum_masked_ptrs(ecg_ctx_t *ctx, int type, uint64_t chunksize, uint64_t rec_size,
			 int k, int p, uint64_t cell_bytes, uint32_t nstripes,
			 void *const *cells, const uint32_t *masks, unsigned which,
			 void *csums, void *result, unsigned flags, void *stream);

/* Checksum EVERY cell of a table: cells, a host array of ncells device
 * addresses as above; csums[i*nch + c] = the checksum of chunk c of cells[i],
 * each cell taken as an extent from record index 0 (ecg_csum_len(type) bytes
 * each; csums at any byte).  Over an [S][k+p] table, ncells = S*(k+p), that is
 * the stripe-major array ecg_csum_mask reads (stripe_stride = (k+p)*nch,
 * cell_stride = nch): the checksum-driven scrub over cell tables is
 * ecg_csum_cells_ptrs -> ecg_memset(masks) -> ecg_csum_mask ->
 * ecg_recover_masks_ptrs_csum, no host round trip.  No masks, no result; always
 * the table kernels (ecg_crc_cells_ptr_kernel<type> / ecg_adler_cells_ptr_kernel,
 * <..bytes> as above).  Telemetry: `csum_chunks` += ncells * nch, `launches`
 * counts the launch.  Errors: -ECG_DER_NOTSUPPORTED for an unknown hash type;
 * -ECG_DER_INVAL for chunksize or rec_size 0, cell_bytes % rec_size != 0, too
 * many checksums, a NULL context, NULL cells or csums (ncells and cell_bytes
 * non-zero), a NULL entry (named), csums overlapping a cell. */
int ecg_csum_cells_ptrs(ecg_ctx_t *ctx, int type, uint64_t chunksize, uint64_t rec_size,
			uint64_t cell_bytes, uint64_t ncells, void *const *cells,
			void *csums, void *stream);

/* ecg_recover_masks_csum over a table of cell addresses: ecg_recover_masks_ptrs,
 * then ECG_CM_ERASED into csums and, with src_csums, ECG_CM_SURVIVORS into
 * src_csums (src_csums == csums: one which = 3 launch; any other overlap of
 * the two is -ECG_DER_INVAL), on one stream.  result: ecg_recover_masks's four
 * words.  The argument errors of both halves are returned before anything is
 * queued, and the table is checked and staged ONCE for all its launches.  An
 * affine table that passes ecg_recover_masks_ptrs's shortcut conditions (and
 * whose checksum arrays are clear of the image) is the call
 * ecg_recover_masks_csum(stripes = cells[0], stride).  As for
 * ecg_recover_masks_ptrs, no cell the launch writes may overlap any other cell
 * (not checked). */
int ecg_recover_masks_ptrs_csum(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
				void *const *cells, const uint32_t *masks, void *result, unsigned flags,
				int type, uint64_t chunksize, uint64_t rec_size,
				void *csums, void *src_csums, void *stream);

/* Checksum the parity cells ecg_update_masks (ecg.h) REWROTE, and no others:
 * the step after a masked update, as ecg_csum_masked is the step after
 * ecg_recover_masks.  The rewritten parity cells are stored with chunk
 * checksums like any other extent; the masks stay on the device, and a sparse
 * batch costs the checksums of the handful of stripes that changed instead of
 * ecg_csum_extents over all nstripes * p parity cells.
 * The parity is addressed exactly as in ecg_update_masks: row r of stripe s at
 * parity + r*parity_cell_stride + s*parity_stripe_stride -- the client layout
 * [p][S][C] (a padded pitch included) and the recovery layout with parity =
 * stripes + k*C alike; either stride may be negative.  parity and masks are read
 * only.  With m = masks[s], read as ecg_update_masks reads it:
 *   m == 0                    nothing of the stripe is read, no slot is written;
 *                             it is not counted
 *   a bit at or above k set   nothing is read or written; the stripe is counted
 *                             in result[3] and result[1]
 *   otherwise (1..k bits)     all p parity cells of the stripe are checksummed
 * All 2^32 mask values are safe.  Each selected cell is taken as an extent from
 * record index 0, as ecg_csum_masked takes its cells: nch = ecg_csum_chunk_count(
 * chunksize, rec_size, 0, cell_bytes / rec_size) checksums of ecg_csum_len(type)
 * bytes, little-endian.  Chunk c of row r of stripe s goes to checksum index
 * s*csum_stripe_stride + r*csum_cell_stride + c of csums (strides in checksums,
 * not bytes, as in ecg_csum_mask; csums at any byte): [p][S][nch], what
 * ecg_encode_csum writes, is cell stride S*nch and stripe stride nch; the parity
 * columns of an [S][k+p][nch] array are csums advanced by k*nch checksums,
 * stripe stride (k+p)*nch, cell stride nch, where an ecg_csum_mask over that
 * array sees the new parity checksums.  No byte outside the selected cells'
 * slots is written.  The nstripes * p ranges of nch slots must lie apart, in one
 * of the two orders that can be proven: cell_stride >= nch and stripe_stride >=
 * (p-1)*cell_stride + nch, or stripe_stride >= nch and cell_stride >=
 * (nstripes-1)*stripe_stride + nch; a stride whose count is 1 (p == 1,
 * nstripes == 1) is not looked at.
 * result: device memory, four uint64 (8-byte aligned): stripes checksummed,
 * lowest stripe with an invalid mask (UINT64_MAX if none), parity cells
 * checksummed (p times word 0), stripes with an invalid mask -- words 0, 1 and
 * 3 are what ecg_update_masks leaves for the same masks; {0, UINT64_MAX, 0, 0}
 * and nothing else touched when nstripes or cell_bytes is 0.  INVALID MASKS ARE
 * REPORTED THROUGH result ONLY.
 * Limits: k <= 16, p <= 8 (ecg_update_masks's, not ecg_csum_masked's p <= 3);
 * the four hash types.  Any alignment: parity, both parity strides, cell_bytes
 * and the record chunk size all multiples of 16 run the 16-byte-load kernels
 * ecg_crc_updated_kernel<type> / ecg_adler_updated_kernel, anything else their
 * <..bytes> forms for the whole launch.  flags: ECG_RM_SPARSE is accepted and
 * changes nothing; ECG_UM_PACKED is refused by name (it packs the data images,
 * not the parity).  ecg_set_csum_launch caps the workgroups.  Asynchronous on
 * `stream`.  Telemetry: `launches` counts the launch; `csum_chunks` is not
 * advanced, the count being known on the device only (result word 2 times nch).
 * Errors, found before the context is used, the message prefixed
 * "csum_updated:", in this order: -ECG_DER_NOTSUPPORTED for an unknown hash
 * type; then -ECG_DER_INVAL for k or p beyond the limits; ECG_UM_PACKED, an
 * unknown flag; chunksize or rec_size 0; cell_bytes % rec_size != 0; too many
 * checksums (nstripes * p * nch checksums, or the farthest slot's byte offset,
 * beyond 64 bits) and the stride rule above (both only with nstripes and
 * cell_bytes non-zero); masks NULL or not 4-byte aligned; result NULL or not
 * 8-byte aligned (both also for nstripes == 0); and, nstripes and cell_bytes
 * non-zero: parity NULL; csums NULL; csums sharing a byte with the parity's byte
 * span, gaps included (the span ecg_update_masks holds its masks and result
 * clear of); csums overlapping the masks; csums overlapping the result.  Last, a
 * NULL context. */
int ecg_csum_updated(ecg_ctx_t *ctx, int type, uint64_t chunksize, uint64_t rec_size,
		     int k, int p, uint64_t cell_bytes, uint32_t nstripes,
		     const void *parity, int64_t parity_cell_stride, int64_t parity_stripe_stride,
		     const uint32_t *masks, void *csums, uint64_t csum_stripe_stride,
		     uint64_t csum_cell_stride, void *result, unsigned flags, void *stream);

/* ecg_csum_updated over the TABLE OF ecg_update_masks_ptrs (ecg.h): cells, a HOST
 * array of nstripes * (2k+p) device addresses, the parity cell r of stripe s
 * being entry s*(2k+p) + 2k + r -- one table serves the update and its
 * checksums.  The table is copied before the call returns (the caller may
 * overwrite or free it at once).  Every entry is checked for NULL, the old and
 * new data entries included (the same table, the same rule as the update call),
 * but the data cells are never read and may alias anything; an item loads its
 * parity entry only after the mask test, at an index that is always 2k + r, r <
 * p, for a word that read as 1..k bits.  Everything else is ecg_csum_updated's,
 * word for word.
 * Errors, all found before the context is used, in this order:
 * ecg_csum_updated's own up to and including the result's (the message prefixed
 * "csum_updated_ptrs:"); then, nstripes and cell_bytes non-zero: csums NULL;
 * csums overlapping the masks or the result; cells NULL; a NULL entry (named by
 * its index); csums, masks or result sharing a byte with a PARITY cell
 * ("overlaps", and the entry's index).  Last, a NULL context.
 * A table whose parity entries are p0 + s*ps + r*pc (negative strides too) and
 * whose arguments pass ecg_csum_updated's own checks IS the call
 * ecg_csum_updated(parity = p0, pc, ps): no table is uploaded and
 * ecg_last_kernel names the strided kernel.  Any other table runs
 * ecg_crc_updated_ptr_kernel<type> / ecg_adler_updated_ptr_kernel with 16-byte
 * loads when EVERY PARITY entry, cell_bytes and the record chunk size are
 * multiples of 16 (the data entries do not matter), and their <..bytes> forms
 * for the WHOLE launch when one is not. */
int ecg_csum_updated_ptrs(ecg_ctx_t *ctx, int type, uint64_t chunksize, uint64_t rec_size,
			  int k, int p, uint64_t cell_bytes, uint32_t nstripes,
			  void *const *cells, const uint32_t *masks, void *csums,
			  uint64_t csum_stripe_stride, uint64_t csum_cell_stride,
			  void *result, unsigned flags, void *stream);

/* ecg_update_masks, then ecg_csum_updated into csums, on one stream: the
 * aggregation update of a batch with one set of changed cells per stripe and
 * the checksums of the parity it rewrote.  Two launches, not a fused kernel.
 * result: ecg_update_masks's four words (the checksum launch counts nothing).
 * flags: ecg_update_masks's; ECG_UM_PACKED is accepted, it affects the update
 * half alone.  The argument errors of both halves are returned before anything
 * is queued, the message prefixed "update_masks_csum:": ecg_update_masks's in
 * their order, then ecg_csum_updated's, then csums sharing a byte with the span
 * of the old or of the new image (every cell the update half may read), then a
 * NULL context. */
int ecg_update_masks_csum(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
			  const void *old_cells, const void *new_cells, int64_t upd_stripe_stride,
			  void *parity, int64_t parity_cell_stride, int64_t parity_stripe_stride,
			  const uint32_t *masks, void *result, unsigned flags, int type,
			  uint64_t chunksize, uint64_t rec_size, void *csums,
			  uint64_t csum_stripe_stride, uint64_t csum_cell_stride, void *stream);

/* ecg_update_masks_csum over a table of cell addresses: ecg_update_masks_ptrs,
 * then ecg_csum_updated_ptrs without a result, on one stream; the table is
 * checked and staged ONCE for both launches.  result: ecg_update_masks's four
 * words.  Errors before anything is queued: ecg_update_masks_ptrs's argument
 * checks up to the result's (ECG_UM_PACKED refused), ecg_csum_updated_ptrs's;
 * then cells NULL and, entry by entry, a NULL entry and masks, result or csums
 * sharing a byte with ANY cell of the table, old and new data cells included;
 * last, a NULL context.
 * An affine table that passes ecg_update_masks_ptrs's shortcut, and whose
 * checksum array is clear of the parity span and of the two image spans, is the
 * call ecg_update_masks_csum.  The caller's contract of ecg_update_masks_ptrs
 * (no parity cell overlaps another cell) holds here too. */
int ecg_update_masks_ptrs_csum(ecg_ctx_t *ctx, int k, int p, uint64_t cell_bytes, uint32_t nstripes,
			       void *const *cells, const uint32_t *masks, void *result, unsigned flags,
			       int type, uint64_t chunksize, uint64_t rec_size, void *csums,
			       uint64_t csum_stripe_stride, uint64_t csum_cell_stride, void *stream);

/* Route of the source checksums of ecg_encode_csum_all / ecg_recover_csum_all:
 * 0 the measured default per (hash type, k, output rows), 1 the fused kernel
 * wherever it can take the request, 2 always two passes.  Same results. */
int ecg_set_csum_all_route(ecg_ctx_t *ctx, uint32_t route);

/* Launch tuning: cap on checksum workgroups (4 chunks in flight each, grid-
 * stride beyond); 0 restores the default. */
int ecg_set_csum_launch(ecg_ctx_t *ctx, uint32_t max_blocks);

/* Launch tuning: 4 KiB columns per work item of the fused product +
 * checksum kernels (ecg_encode_csum / ecg_recover_csum); 0 restores the
 * default (env ECG_FUSED_COLS, else by hash type, k and output rows: 2 for
 * crc32 with k = 8 and two rows, 4 for one row or k >= 8, else 8; 8 for the
 * kernels of ecg_encode_csum_all / ecg_recover_csum_all).  Same results
 * either way. */
int ecg_set_fused_cols(ecg_ctx_t *ctx, uint32_t ncols);

#ifdef __cplusplus
}
#endif

#endif
