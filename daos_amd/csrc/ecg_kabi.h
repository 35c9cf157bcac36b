/*
 * ecg_kabi.h -- the private ABI between the C host layer (daos_amd/csrc/host)
 * and the HIP kernels (daos_amd/csrc/kernels).  Plain C, no HIP types.
 *
 * One launch = one batched GF(2^8) "matrix x cells" product over S stripes:
 *
 *     dst[s][r][i] (^)= XOR_{j<k} coef[r][j] * src[s][j][i]      i in [0, C)
 *
 * which is ISA-L ec_encode_data (ref:src/object/cli_ec.c:540) when coef are
 * the Cauchy parity rows, DAOS recovery (ref:src/object/cli_ec.c:2641) when
 * coef are the decode rows, and ec_encode_data_update / agg_update_parity
 * (ref:src/object/srv_ec_aggregate.c:1089-1101) with `accumulate` and
 * `diff` set (src = old ^ new).
 *
 * Cell j of stripe s lives at  src + s*src_stripe_stride + src_cell_off[j];
 * that covers the DAOS layouts: client data [S][k][C], parity [p][S][C]
 * (ref:src/object/cli_ec.c:75-97,638-640), recovery [S][k+p][C]
 * (ref:src/object/cli_ec.c:2449-2464, 2626-2643), aggregation [k][C]/[p][C]
 * (ref:src/object/srv_ec_aggregate.c:686-691).
 *
 * GF multiply tables ("perm tables"): a byte x splits into bit groups
 * x = (x & 0x07) ^ (x & 0x38) ^ (x & 0xC0) and, GF multiplication being
 * linear over GF(2),  c*x = T0[x & 7] ^ T1[(x >> 3) & 7] ^ T2[x >> 6]  with
 * T0[i] = c*i, T1[i] = c*(i<<3), T2[i] = c*(i<<6).  Each table has <= 8 byte
 * entries, i.e. exactly what one v_perm_b32 can index.  Packed little-endian:
 * t0lo = T0[0..3], t0hi = T0[4..7], t1lo/t1hi likewise, t2 = T2[0..3].
 */
#ifndef ECG_KABI_H
#define ECG_KABI_H

#include <assert.h>	/* static_assert in C */
#include <stdint.h>

#define ECG_KMAX_K 16	/* data cells per launch; host splits larger k */
#define ECG_KMAX_R 8	/* output rows per launch */

typedef struct ecg_ptbl {
	uint32_t t0lo, t0hi, t1lo, t1hi, t2;
} ecg_ptbl_t;

/*
 * The table layout of a product with rm output rows, as 16-byte words: the
 * one every GF kernel stages into LDS and the set table of ecg_recover_masks
 * stores.  Cell-major; source cell j owns ECG_TBL_PER_J(rm) words,
 *   word  j*PER_J + r           row r's {t0lo, t0hi, t1lo, t1hi}      r < rm
 *   words j*PER_J + rm ..       the rows' t2, four to a word: row r's is
 *                               dword r of them
 * so a lane reads one row with one 16-byte load and the t2 of every row with
 * (rm + 3) / 4 more.  ECG_TBL_ROW: the word of (j, r); ECG_TBL_T2: the dword
 * index of its t2 (both from the table's start); ECG_TBL_WORDS: the words of
 * km cells.  The kernels go through ecg_mm_dev.h mm_tbl / tbl_stage, the
 * host's set-table build through these macros.
 */
#define ECG_TBL_PER_J(rm) ((rm) + ((rm) + 3) / 4)
#define ECG_TBL_WORDS(km, rm) ((km) * ECG_TBL_PER_J(rm))
#define ECG_TBL_ROW(rm, j, r) ((j) * ECG_TBL_PER_J(rm) + (r))
#define ECG_TBL_T2(rm, j, r) (4 * ECG_TBL_ROW(rm, j, rm) + (r))

typedef struct ecg_mm_params {
	const uint8_t *src;		/* cell bases (stripe 0) */
	const uint8_t *src2;		/* diff mode: second source, same layout */
	uint8_t *dst;
	int64_t src_stripe_stride;
	int64_t src2_stripe_stride;
	int64_t dst_stripe_stride;
	int64_t src_cell_off[ECG_KMAX_K];
	int64_t src2_cell_off[ECG_KMAX_K];
	int64_t dst_cell_off[ECG_KMAX_R];
	uint64_t cell_bytes;
	uint32_t nstripes;
	uint32_t k;
	uint32_t rows;
	uint32_t accumulate;		/* dst ^= product instead of dst = product */
	uint32_t diff;			/* source cell j = src[j] ^ src2[j] */
	uint32_t order;			/* block -> (stripe, column) map, 0 = 2D grid (ecg_kernels.hip) */
	ecg_ptbl_t tbl[ECG_KMAX_R][ECG_KMAX_K];
} ecg_mm_params_t;

/* launch tuning (host fills; 0 = kernel default) */
typedef struct ecg_launch_cfg {
	uint32_t grid_x;	/* chunks per stripe handled in parallel */
	uint32_t grid_y;	/* stripes handled in parallel */
	uint32_t variant;	/* 0 auto, 1 force generic, 2 force byte kernel, 3 dword
				 * lanes at any alignment (hardware unaligned access) */
	uint32_t order;		/* 0 = 2D grid x columns / y stripes; 1-3 1D orders (ecg_kernels.hip) */
	uint32_t wg_per_cu;	/* product kernel blocks per CU: 0 = per-shape default, 1..16 = cap,
				 * ECG_WG_UNCAPPED = none (ecg_kernels.hip mm_wg_cap) */
	uint32_t no_unaligned;	/* the device did not serve misaligned dword accesses at context
				 * creation (ecg_k_unaligned_check): operands that need them take
				 * the byte kernels */
} ecg_launch_cfg_t;
#define ECG_WG_UNCAPPED 255u


/*
 * Chunked checksums (DAOS csummer semantics, ref:src/common/checksum.c:467-497):
 * n_ext extents at src + e*ext_stride, each ext_bytes long and cut into
 * nchunks chunks: chunk 0 = [0, first_bytes), chunk c >= 1 =
 * [first_bytes + (c-1)*chunk_bytes, ... + chunk_bytes) clipped to ext_bytes.
 * out[e*nchunks + c] = hash of that chunk (2, 4 or 8 bytes, little-endian).
 * CRC tables (host-built, ecg_csum.c) at tbl: W-bit words T
 *   sl[NB][256]  slice tables: sl[j][v] = CRC state after byte v then j zero bytes
 *   sh[NB][256]  "shift by ECG_CSUM_STRIDE zero bytes" as a byte-wise linear map
 *   k[64]        x^(8*16*(63-lane)) mod P, for the final per-lane shift
 *   sh4k[NB][256] shift by ECG_MMCS_STRIDE zero bytes (fused kernels)
 *   k256[256]    x^(8*16*(255-thread)) mod P (host builds the fused kh rows from it)
 *   p2[48]       x^(8*2^j) mod P (shift by any byte count: product over its bits)
 *   sh256[NB][256] shift by ECG_CSUM_GSTRIDE zero bytes (lane-group kernel)
 * with NB = W/8, T = uint32_t (W <= 32) or uint64_t (W = 64).
 */
#define ECG_CSUM_STRIDE 1024	/* bytes a wave consumes per step (64 lanes x 16 B) */

#define ECG_MMCS_STRIDE 4096	/* fused kernels: 256 threads x 16 B per step */
#define ECG_CSUM_NP2 48
/*
 * 5-bit tables (conflict-free LDS lookups: a 32-entry table of 4-byte words
 * covers the 32 banks ds_read_b32 sees, one of 8-byte words the 64 banks of
 * ds_read_b64, so lanes never collide -- the byte tables above run ~3x
 * conflicted on random data).  A 16-byte piece is 4 dwords x 7 fields (bits
 * 5i..5i+4, the 7th field bits 30-31):
 *   p5[28][32]   p5[7j + i][v] = raw CRC of the piece whose dword j is v << 5i
 *   a5*[NA][32]  a register shifted by 1 KiB / 256 B / 4 KiB of zero bytes,
 *                fields of each 32-bit half of the register (NA = 7 per half;
 *                4 for crc16: bits 0-19)
 */
#define ECG_CSUM_NF5 28
#define ECG_CSUM_NA5(NB) ((NB) == 2 ? 4 : 7 * (NB) / 4)
#define ECG_CSUM_OFF_P5(NB) (4 * (NB) * 256 + 64 + 256 + ECG_CSUM_NP2)
#define ECG_CSUM_OFF_A5_1K(NB) (ECG_CSUM_OFF_P5(NB) + ECG_CSUM_NF5 * 32)
#define ECG_CSUM_OFF_A5_256(NB) (ECG_CSUM_OFF_A5_1K(NB) + ECG_CSUM_NA5(NB) * 32)
#define ECG_CSUM_OFF_A5_4K(NB) (ECG_CSUM_OFF_A5_256(NB) + ECG_CSUM_NA5(NB) * 32)
/* s16[16][256]: register after byte v and then j zero bytes, j < 16 (the
 * raw CRC of a 16-byte piece is 16 independent lookups, no serial fold) */
#define ECG_CSUM_OFF_S16(NB) (ECG_CSUM_OFF_A5_4K(NB) + ECG_CSUM_NA5(NB) * 32)
/* positional p5 tables: p5x*[u-1] = p5 followed by u strides (1 KiB / 256 B)
 * of zero bytes, u = 1 .. ECG_CSUM_P5U-1 (the standalone CRC kernels shift the
 * register once per ECG_CSUM_P5U pieces: a5 of 4 KiB / 1 KiB) */
#define ECG_CSUM_P5U 4
#define ECG_CSUM_OFF_P5X_1K(NB) (ECG_CSUM_OFF_S16(NB) + 16 * 256)
#define ECG_CSUM_OFF_P5X_256(NB) (ECG_CSUM_OFF_P5X_1K(NB) + (ECG_CSUM_P5U - 1) * ECG_CSUM_NF5 * 32)
/* the fused workgroup kernel's 4 KiB columns: positional tables of 1 ..
 * ECG_MMCS_P5U-1 columns and the a5 of ECG_MMCS_P5U columns (an item of at
 * most ECG_MMCS_P5U columns needs no register shift at all, so its columns can
 * be walked in any order) */
#define ECG_MMCS_P5U 8
#define ECG_CSUM_OFF_P5X_4K(NB) (ECG_CSUM_OFF_P5X_256(NB) + (ECG_CSUM_P5U - 1) * ECG_CSUM_NF5 * 32)
#define ECG_CSUM_OFF_A5_32K(NB) (ECG_CSUM_OFF_P5X_4K(NB) + (ECG_MMCS_P5U - 1) * ECG_CSUM_NF5 * 32)
/* reflected CRCs (crc32, crc64): the fused workgroup kernel multiplies a
 * lane's value by x^(8*16*(63-lane)) nibble by nibble --
 *   nibl[n][lane] = (n at the register's 4 lowest powers) * x^(8*16*(63-lane))
 *   r4[m]         = m (register bits 0-3) * x^4, the reduction of a 4-bit shift
 * (n-major, so lane l's entries sit in bank l: conflict-free) */
#define ECG_CSUM_OFF_NIBL(NB) (ECG_CSUM_OFF_A5_32K(NB) + ECG_CSUM_NA5(NB) * 32)
#define ECG_CSUM_OFF_R4(NB) (ECG_CSUM_OFF_NIBL(NB) + 16 * 64)
/* nibble tables (4-bit fields, addressed by one SDWA byte select each;
 * ecg_crc_dev.h horner4u): a 16-byte piece is 32 nibbles (nibble t = bits
 * 4t..4t+3 of the piece, little-endian), the register W/4 nibbles.
 *   q4*[u][32][16]  q4[u][t][v] = raw CRC of the piece whose nibble t is v,
 *                   followed by u strides of zero bytes (u = 0 .. U-1)
 *   a4*[16][16]     a4[t][v] = register nibble t = v shifted by the U-stride
 *                   (rows >= W/4 unused)
 * 1 KiB stride (wave kernels, U = ECG_CSUM_P5U; a4 of 4 KiB), 256 B stride
 * (lane-group kernel, U = ECG_CSUM_P5U; a4 of 1 KiB), 4 KiB stride (fused
 * workgroup kernel, U = ECG_MMCS_P5U; a4 of 32 KiB). */
#define ECG_CSUM_NQ4 (32 * 16)
#define ECG_CSUM_OFF_Q4_1K(NB) (ECG_CSUM_OFF_R4(NB) + 16)
#define ECG_CSUM_OFF_A4_4K(NB) (ECG_CSUM_OFF_Q4_1K(NB) + ECG_CSUM_P5U * ECG_CSUM_NQ4)
#define ECG_CSUM_OFF_Q4_256(NB) (ECG_CSUM_OFF_A4_4K(NB) + 256)
#define ECG_CSUM_OFF_A4_1K(NB) (ECG_CSUM_OFF_Q4_256(NB) + ECG_CSUM_P5U * ECG_CSUM_NQ4)
#define ECG_CSUM_OFF_Q4_4K(NB) (ECG_CSUM_OFF_A4_1K(NB) + 256)
#define ECG_CSUM_OFF_A4_32K(NB) (ECG_CSUM_OFF_Q4_4K(NB) + ECG_MMCS_P5U * ECG_CSUM_NQ4)
#define ECG_CSUM_TBL_ENTRIES(NB) (ECG_CSUM_OFF_A4_32K(NB) + 256)
#define ECG_CSUM_OFF_P2(NB) (3 * (NB) * 256 + 64 + 256)
#define ECG_CSUM_OFF_SH256(NB) (3 * (NB) * 256 + 64 + 256 + ECG_CSUM_NP2)
#define ECG_CSUM_GLANES 16	/* lanes per chunk in the lane-group CRC kernel */
#define ECG_CSUM_GSTRIDE (16 * ECG_CSUM_GLANES)	/* bytes a lane group consumes per step */
#define ECG_CSUM_OFF_SH(NB) ((NB) * 256)
#define ECG_CSUM_OFF_K64(NB) (2 * (NB) * 256)
#define ECG_CSUM_OFF_SH4K(NB) (2 * (NB) * 256 + 64)
#define ECG_CSUM_OFF_K256(NB) (3 * (NB) * 256 + 64)

typedef struct ecg_csum_params {
	const uint8_t *src;
	uint8_t *out;
	const void *tbl;
	int64_t ext_stride;
	uint64_t ext_bytes;
	uint64_t first_bytes;
	uint64_t chunk_bytes;
	uint64_t init;			/* CRC register before the first byte */
	uint64_t xorout;		/* XORed into the final register */
	uint64_t poly;			/* reflected (or MSB-first for crc16) polynomial */
	uint32_t n_ext;
	uint32_t nchunks;
	uint32_t type;			/* DAOS hash type: 1 crc16, 2 crc32, 3 crc64, 7 adler32 */
	uint32_t variant;		/* CRC: 0 auto, 1 wave per chunk, 2 workgroup per chunk,
					 * 3 a 16-lane group per chunk */
	uint32_t pad1, pad2;
	/* workgroup-per-chunk CRC: a chunk of m 1 KiB steps is cut into
	 * ECG_CSUM_SPLIT_NW slices; split_sh[c][w] = x^(8 * bytes after slice w)
	 * mod P for the chunk lengths' step counts split_m[c] (first, middle and
	 * last chunk of an extent), filled by the host */
	uint64_t split_m[3];
	uint64_t split_sh[3][8];
} ecg_csum_params_t;

#define ECG_CSUM_SPLIT_NW 8
/* 1 KiB steps of a wave over len bytes (lanes take 16-byte pieces; a zero
 * prefix pads to a whole number of ECG_CSUM_P5U-piece Horner steps), and the
 * steps of each of the split kernel's ECG_CSUM_SPLIT_NW slices */
#define ECG_CSUM_STEPS(len) \
	((((len) / 16 + 63) / 64 + ECG_CSUM_P5U - 1) / ECG_CSUM_P5U * ECG_CSUM_P5U)
#define ECG_CSUM_SPLIT_MS(m) \
	((((m) + ECG_CSUM_SPLIT_NW - 1) / ECG_CSUM_SPLIT_NW + ECG_CSUM_P5U - 1) / ECG_CSUM_P5U * ECG_CSUM_P5U)

/*
 * Fused product + checksum: a launch of the GF product (ecg_mm_params_t)
 * that also checksums every output cell it writes, chunk by chunk, while the
 * bytes are still in registers.  Each output cell starts on a chunk boundary;
 * chunk_bytes is a multiple of ECG_MMCS_STRIDE; cell_bytes a multiple of 16.
 * out[(row_slot[r] * nstripes + s) * nch + c] = checksum of chunk c of output
 * row r of stripe s (zeroed by the host: workgroups XOR their partials in).
 *
 * Work items: chunk c (m 4 KiB columns; m_last for the last chunk of a cell)
 * is cut into sub-chunks of ncols columns, item = (c, h) with h < nh (nh_last
 * for the last chunk), numbered c * nh + h; nitems = (nch - 1) * nh + nh_last.
 * A workgroup Horner-accumulates its sub-chunk's columns per thread and then
 * moves thread t's value to the end of the chunk: a factor x^(8 * (16 * (255 -
 * t) + 4096 * (columns after the sub-chunk))) mod P, times x^(-8Z) in the last
 * chunk's rows, Z being the zero bytes that pad the cell to whole columns.
 * crc16: kh[(row0 + h) * 256 + t] holds that factor (row0 = 0, or nh for the
 * last chunk).  Reflected CRCs: the lane part x^(8*16*(63-lane)) comes from the
 * nibl tables (staged in LDS), each wave XOR-reduces, and the rest f =
 * x^(8 * (1024 * (3 - wave) + 4096 * (columns after))) (* x^(-8Z)) is applied
 * once per wave, bit-parallel: kh[((row0 + h) * 4 + wave) * 64 + b] = e_b * f
 * (e_b = the register with only bit b set, zero for b >= W).  CRC is linear,
 * so the values XOR to the chunk's CRC.
 */
typedef struct ecg_mmcs_params {
	const void *tbl;
	uint8_t *out;
	const void *kh;			/* (nh + nh_last) x 256 (crc16) or x 4 x 64 (reflected:
					 * per-wave bit-products, ecg_csum.c fused_kh), T as tbl */
	uint64_t chunk_bytes;
	uint64_t init, xorout, poly;
	uint32_t nch;
	uint32_t type;
	uint32_t m, m_last;		/* 4 KiB columns per chunk / in the last chunk */
	uint32_t ncols;			/* columns per item */
	uint32_t nh, nh_last;		/* items per chunk / in the last chunk */
	uint32_t nitems;
	uint32_t pad3;
	uint32_t row_slot[ECG_KMAX_R];
	/* source checksums (the SRC instantiations; NULL = outputs only):
	 * src_out[(src_slot[j] * nstripes + s) * nch + c] = checksum of chunk c of
	 * source cell j of stripe s, zeroed by the host like out */
	uint8_t *src_out;
	uint32_t src_slot[ECG_KMAX_K];
} ecg_mmcs_params_t;

/*
 * Batched byte-range copies (kernels/ecg_copy_kernels.hip): segment s copies
 * len bytes from src to dst (device addresses, any alignment, no overlap)
 * and owns the launch's 16 KiB destination tiles [tile0, tile0 +
 * ecg_k_copy_tiles(dst, len)); segments are listed in tile0 order from 0.
 */
typedef struct ecg_copy_seg {
	uint64_t dst;
	uint64_t src;
	uint64_t len;
	uint64_t tile0;
} ecg_copy_seg_t;

/*
 * Parity consistency check (kernels/ecg_verify_kernels.hip, ecg_verify): a
 * launch computes the syndrome stored_parity[r] ^ XOR_j coef[r][j] * data[j]
 * of every stripe and folds it into one status word per stripe,
 *   bits 0-7   row r: the syndrome of parity row r is nonzero somewhere
 *   bits 8-23  candidate j: data cell j alone explains every nonzero
 *              syndrome byte seen (s_r = g[r][j] * e for every row r)
 * preset by the host to no rows and every j < k a candidate; the kernels only
 * clear candidate bits and set row bits (atomicAnd / atomicOr).
 * ecg_verify_classify is the one reading of that word, shared by the host's
 * ecg_verify_cell and the summary kernel: -1 clean, 0..k+p-1 the one cell
 * that explains it, -2 not attributable to one cell.
 */
#ifdef __HIPCC__
#define ECG_KABI_HD __host__ __device__
#else
#define ECG_KABI_HD
#endif
static inline ECG_KABI_HD int ecg_verify_classify(uint32_t status, int k, int p)
{
	const uint32_t rows = status & 0xffu;
	const uint32_t cand = (status >> 8) & 0xffffu & ((1u << k) - 1u);

	if (rows == 0)
		return -1;
	/* one parity row: row 0 and any data cell are indistinguishable */
	if (p < 2 || (rows >> p) != 0)
		return -2;
	if ((rows & (rows - 1u)) == 0)
		return k + __builtin_ctz(rows);
	if (rows == (1u << p) - 1u && cand != 0 && (cand & (cand - 1u)) == 0)
		return __builtin_ctz(cand);
	return -2;
}

/*
 * Every ecg_k_launch_* below that ends in `const char **kernel` reports the
 * kernel it launched: on a launch it stores that kernel's name there, a string
 * with static storage (a literal, or its dispatch table entry's name / pname).
 * kernel may be NULL.  A call that launches nothing -- the early success for an
 * empty batch, and every error return before the launch -- leaves *kernel as
 * it is.
 */

#ifdef __cplusplus
extern "C" {
#endif
/* Syndrome pass of ecg_verify: p->src the data cells, p->dst the stored
 * parity (read only), p->tbl the parity rows; status[nstripes] preset by the
 * host on `stream`.  bytewise = 0: the 16-byte lane kernel (every cell
 * address and stride 16-byte aligned, cell_bytes % 16 == 0); 1: the
 * byte-granular kernel (any alignment and length).  cfg: grid_x / grid_y and
 * wg_per_cu as for the product.
 * cells_dev == NULL: the strided operands above.  Otherwise ecg_verify_ptrs:
 * the same pass with the cells of stripe s at the addresses cells_dev[s * (k +
 * rows) + c], c = 0 .. k-1 the data cells and k .. k+rows-1 the parity rows
 * (device memory, read only for the launch); p->src / dst, the strides and the
 * cell offsets are then unused, and bytewise is the host's lane choice, 0 only
 * when EVERY table entry and cell_bytes are multiples of 16: the launcher does
 * not read the table.  *kernel: ecg_verify_kernel<k,p> / ecg_verify_byte_kernel,
 * or their ecg_verify_ptr_* counterparts over a table. */
int ecg_k_launch_verify(const ecg_mm_params_t *p, const uint64_t *cells_dev, uint32_t *status, int bytewise,
			const ecg_launch_cfg_t *cfg, void *stream, const char **kernel);
/* result[0] += bad stripes, result[1] = min(result[1], lowest bad stripe),
 * result[2] += stripes ecg_verify_classify attributes to one cell, result[3]
 * += bad stripes it does not; the host presets {0, UINT64_MAX, 0, 0}. */
int ecg_k_launch_verify_summary(const uint32_t *status, uint32_t nstripes, int k, int p,
				uint64_t *result, void *stream);
/* Repair pass of ecg_repair (kernels/ecg_repair_kernels.hip): p as for
 * ecg_k_launch_verify (src the data cells, dst the parity rows, rows = p;
 * p->tbl unused), status[nstripes] the words a verify of the same operands
 * left (read only).  For every stripe ecg_verify_classify attributes to one
 * cell c, that cell is rewritten with row c of rowtbl: (k + p) x k perm
 * tables in device memory, row c slot j the coefficient of source j, where
 * the sources of c >= k are the k data cells and those of c < k the data
 * cells with slot c replaced by parity row 0 (host/ecg_repair.c
 * ecg_repair_row).  result[0] += stripes repaired, result[1] = min(result[1],
 * lowest bad stripe left as it is), result[2] += data cells rewritten,
 * result[3] += bad stripes left; the host presets {0, UINT64_MAX, 0, 0}.
 * bytewise as for verify.  cfg: grid_x / grid_y; grid.y runs over groups of
 * 64 stripes (a block row reads its group's status words with one load) and
 * by default at most ECG_REPAIR_GRID_X blocks share a group and stride over
 * a stripe's 4 KiB columns, so a clean batch costs its block count, not its
 * bytes.
 * cells_dev == NULL: the strided operands above.  Otherwise ecg_repair_ptrs:
 * the cells of stripe s at the addresses cells_dev[s * (k + p) + c] in logical
 * cell order (device memory, read only for the launch), p->src / dst, the
 * strides and the cell offsets unused: the sources of c >= k are the entries 0
 * .. k-1, those of c < k the same with entry k in slot c, the destination
 * entry c.  bytewise = 0 then only when EVERY table entry and cell_bytes are
 * multiples of 16 (the host's check).  *kernel: ecg_repair_kernel<k> /
 * ecg_repair_byte_kernel, or their ecg_repair_ptr_* counterparts over a table. */
#define ECG_REPAIR_GRID_X 64u
int ecg_k_launch_repair(const ecg_mm_params_t *p, const ecg_ptbl_t *rowtbl, const uint64_t *cells_dev,
			const uint32_t *status, uint64_t *result, int bytewise, const ecg_launch_cfg_t *cfg,
			void *stream, const char **kernel);
#ifdef __cplusplus
}
#endif

/*
 * Per-stripe erasure sets (kernels/ecg_recover_masks_kernels.hip,
 * ecg_recover_masks): bit c of a stripe's mask word = logical cell c is
 * erased.  The nonempty sets of at most p of the k + p cells are numbered by
 * size, then by combinatorial rank: the set c1 < c2 < .. < ce has index
 *   sum_{i<e} C(k+p, i)  +  C(c1, 1) + C(c2, 2) + .. + C(ce, e)
 * a bijection onto 0 .. N-1, N = sum_{e=1..p} C(k+p, e) (1159 for k = 16,
 * p = 3).  ecg_erasure_set_read is the one reading of a mask word, shared by
 * the host's ecg_erasure_set_index and the kernels: the index, ECG_RM_NONE for
 * mask 0, ECG_RM_LOSS for more than p bits, ECG_RM_RANGE for a bit at or above
 * k + p -- the kernels leave a stripe of the last two as it is and count it.
 */
#define ECG_RM_MAX_K 16
#define ECG_RM_MAX_P 3
#define ECG_RM_NONE (-1)
#define ECG_RM_LOSS (-2)
#define ECG_RM_RANGE (-3)
/* C(n, e) for e <= 3 (n < 20 here) */
static inline ECG_KABI_HD uint32_t ecg_rm_binom(uint32_t n, uint32_t e)
{
	return e == 0 ? 1u : e == 1 ? n : e == 2 ? n * (n - 1u) / 2u : n * (n - 1u) * (n - 2u) / 6u;
}
/* 1 <= k <= ECG_RM_MAX_K, 1 <= p <= ECG_RM_MAX_P (the callers check) */
static inline ECG_KABI_HD uint32_t ecg_erasure_set_count(int k, int p)
{
	uint32_t n = 0;

	for (int e = 1; e <= p; e++)
		n += ecg_rm_binom((uint32_t)(k + p), (uint32_t)e);
	return n;
}
static inline ECG_KABI_HD int ecg_erasure_set_read(uint32_t mask, int k, int p)
{
	const int e = __builtin_popcount(mask);
	uint32_t idx = 0, m = mask;

	if (mask == 0)
		return ECG_RM_NONE;
	if ((mask >> (k + p)) != 0)	/* k + p <= 19 */
		return ECG_RM_RANGE;
	if (e > p)
		return ECG_RM_LOSS;
	for (int i = 1; i < e; i++)
		idx += ecg_rm_binom((uint32_t)(k + p), (uint32_t)i);
	for (int i = 1; i <= e; i++) {
		idx += ecg_rm_binom((uint32_t)__builtin_ctz(m), (uint32_t)i);
		m &= m - 1u;
	}
	return (int)idx;
}
/*
 * Which cells of a stripe ecg_csum_masked checksums (kernels/
 * ecg_csum_kernels.hip), from the stripe's mask word: nothing unless
 * ecg_erasure_set_read reads the word as a set; `which` bit 0 the cells the
 * set names, bit 1 the k lowest cells it does not name -- the dec_idx of
 * ecg_recov_rows for the set in ascending order (its all-parity shortcut
 * reads cells 0 .. k-1, which are the k lowest then too).  Shared by the host
 * and the kernels; *valid = the word reads as a set.
 */
static inline ECG_KABI_HD uint32_t ecg_csum_masked_sel(uint32_t mask, int k, int p, uint32_t which, int *valid)
{
	uint32_t surv, sel = 0;

	*valid = ecg_erasure_set_read(mask, k, p) >= 0;
	if (!*valid)
		return 0;
	/* k + p - e >= k cells survive: drop the highest p - e of them */
	surv = ~mask & ((1u << (k + p)) - 1u);
	for (int i = __builtin_popcount(surv); i > k; i--)
		surv &= ~(0x80000000u >> __builtin_clz(surv));
	if (which & 1u)
		sel |= mask;
	if (which & 2u)
		sel |= surv;
	return sel;
}

/*
 * ecg_csum_masked: stripes [S][k+p][C] at src + s*stripe_stride; a wave takes
 * one (stripe s, r-th selected cell, chunk c) of the S x slots x nch items
 * (slots = the most cells `which` can select: p, k or k + p) and skips those
 * with r >= popcount(sel(masks[s])).  Chunk c of a cell is [c*chunk_bytes,
 * min((c+1)*chunk_bytes, C)); out[(s*(k+p) + cell)*nch + c] = its checksum.
 * The item (s, 0, 0) counts its stripe into result (NULL: not counted):
 * result[0] += stripes with a valid set, result[1] = min(result[1], lowest
 * stripe whose non-zero mask is no set), result[2] += cells checksummed,
 * result[3] += stripes whose non-zero mask is no set.
 * cells_dev == NULL: the strided image above.  Otherwise ecg_csum_masked_ptrs:
 * cell c of stripe s lies at the address cells_dev[s * (k + p) + c] (device
 * memory, read only for the launch; src and stripe_stride unused); an item
 * loads its entry after the sel test, so a skipped item reads none.  bytewise
 * is then the host's lane choice, 0 only when EVERY table entry, cell_bytes and
 * chunk_bytes are multiples of 16: the launcher does not read the table.
 * ecg_csum_cells_ptrs (ecg_k_launch_csum_cells) checksums every cell of a
 * table of ncells entries, item g = chunk g % nch of cell g / nch, out[g] its
 * checksum; it reads cells_dev, out, tbl, cell_bytes, chunk_bytes, nch, type,
 * bytewise and the CRC constants.
 */
typedef struct ecg_csum_masked_params {
	const uint8_t *src;
	uint8_t *out;
	const void *tbl;
	const uint32_t *masks;
	uint64_t *result;
	const uint64_t *cells_dev;
	int64_t stripe_stride;
	uint64_t cell_bytes;
	uint64_t chunk_bytes;
	uint64_t init, xorout, poly;
	uint64_t ncells;
	uint32_t nstripes;
	uint32_t nch;
	uint32_t k, p;
	uint32_t which;
	uint32_t slots;
	uint32_t type;
	uint32_t bytewise;
} ecg_csum_masked_params_t;

/*
 * Per-stripe sets of updated cells (kernels/ecg_update_masks_kernels.hip,
 * ecg_update_masks): bit j of a stripe's mask word = data cell j changed.
 * ecg_update_mask_read is the one reading of a mask word, shared by the host
 * and the kernels: ECG_UM_NONE for mask 0, ECG_UM_RANGE for a bit at or above
 * k (the kernels leave such a stripe as it is and count it), else the number
 * of cells, 1 .. k.  1 <= k <= ECG_KMAX_K (the callers check).
 */
#define ECG_UM_NONE 0
#define ECG_UM_RANGE (-1)
static inline ECG_KABI_HD int ecg_update_mask_read(uint32_t mask, int k)
{
	if (mask == 0)
		return ECG_UM_NONE;
	if ((mask >> k) != 0)	/* k <= 16 */
		return ECG_UM_RANGE;
	return __builtin_popcount(mask);
}

/*
 * ecg_agg_masks' reading of (mask word, k, T), shared by the host and the
 * kernels (kernels/ecg_update_masks_kernels.hip): what a stripe gets.  NOTHING
 * for mask 0; REFUSE for a bit at or above k (left as it is and counted); with
 * n = 1 .. k cells named, DELTA -- ecg_update_masks's update -- for n <= T and
 * RECALC -- the re-encode of the merged stripe -- for n > T.  T = 0 .. k (the
 * callers check): 0 re-encodes every stripe with work, k none.
 */
#define ECG_AGG_REFUSE (-1)
#define ECG_AGG_NOTHING 0
#define ECG_AGG_DELTA 1
#define ECG_AGG_RECALC 2
static inline ECG_KABI_HD int ecg_agg_route(uint32_t mask, int k, uint32_t T)
{
	const int n = ecg_update_mask_read(mask, k);

	if (n == ECG_UM_NONE)
		return ECG_AGG_NOTHING;
	if (n == ECG_UM_RANGE)
		return ECG_AGG_REFUSE;
	return (uint32_t)n > T ? ECG_AGG_RECALC : ECG_AGG_DELTA;
}

/*
 * ecg_csum_updated: the checksums of the parity cells ecg_update_masks rewrote
 * (kernels/ecg_csum_kernels.hip cs_updated).  A wave takes one (stripe s, parity
 * row r, chunk c) of the S x p x nch items and skips it unless
 * ecg_update_mask_read(masks[s], k) > 0, so a clean stripe costs its items one
 * mask load each.  Row r of stripe s lies at src + r*cell_stride +
 * s*stripe_stride (either may be negative); chunk c of a cell is [c*chunk_bytes,
 * min((c+1)*chunk_bytes, C)); its checksum goes to index s*csum_stripe_stride +
 * r*csum_cell_stride + c of out (slots of the checksum's length at any byte).
 * The item (s, 0, 0) counts its stripe into result (NULL: not counted):
 * result[0] += stripes read as 1 .. k cells, result[1] = min(result[1], lowest
 * stripe with a bit at or above k), result[2] += p per stripe of word 0,
 * result[3] += stripes with such a bit.
 * cells_dev == NULL: the strided parity above.  Otherwise
 * ecg_csum_updated_ptrs: the table of ecg_update_masks_ptrs, parity row r of
 * stripe s at the address cells_dev[s * (2k + p) + 2k + r] (device memory, read
 * only for the launch; src and the parity strides unused); an item loads its
 * entry after the mask test, so a skipped item reads none and no item reads an
 * old or new data entry.  bytewise is then the host's lane choice, 0 only when
 * EVERY parity entry, cell_bytes and chunk_bytes are multiples of 16: the
 * launcher does not read the table.
 * Its launcher, ecg_k_launch_csum_updated (kernels/ecg_csum_kernels.hip), is
 * declared in host/ecg_internal.h beside the host code that calls it.
 */
typedef struct ecg_csum_updated_params {
	const uint8_t *src;
	uint8_t *out;
	const void *tbl;
	const uint32_t *masks;
	uint64_t *result;
	const uint64_t *cells_dev;
	int64_t cell_stride, stripe_stride;
	uint64_t csum_stripe_stride, csum_cell_stride;
	uint64_t cell_bytes;
	uint64_t chunk_bytes;
	uint64_t init, xorout, poly;
	uint32_t nstripes;
	uint32_t nch;
	uint32_t k, p;
	uint32_t type;
	uint32_t bytewise;
} ecg_csum_updated_params_t;

/*
 * The set table of one (k, p), device memory, built by host/
 * ecg_recover_masks.c: entry i (the set of index i) is ECG_RM_ENT_Q(k, p)
 * 16-byte words,
 *   word 0      {e, out_idx[0], out_idx[1], out_idx[2]}: the erased cells in the
 *               order ecg_recov_rows writes them (unused slots 0)
 *   word 1      dec_idx[j] in byte j: the k survivors the rows read
 *   words 2..   the e x k perm tables in the product's layout for p output
 *               rows (ECG_TBL_PER_J above), rows >= e zero
 * so a block stages a set with one 16-byte copy per thread.  With p <=
 * ECG_RM_MAX_P = 3 a cell takes p + 1 words: 2 + k * (p + 1) in all.
 */
#define ECG_RM_ENT_Q(k, p) (2u + ECG_TBL_WORDS((uint32_t)(k), (uint32_t)(p)))
static_assert(ECG_RM_ENT_Q(16, 1) == 2u + 16u * 2u && ECG_RM_ENT_Q(16, 2) == 2u + 16u * 3u &&
		      ECG_RM_ENT_Q(16, ECG_RM_MAX_P) == 2u + 16u * 4u,
	      "set-table entry: p + 1 words per cell");

#ifdef __cplusplus
extern "C" {
#endif
/* ecg_recover_masks: p->src = p->dst = the stripes ([S][k+p][C], stripe stride
 * p->src_stripe_stride), p->k, p->rows = p, cell_bytes, nstripes; the cell
 * offsets and p->tbl are unused.  For every stripe whose mask reads as a set,
 * the set's e rows are applied to its dec_idx cells and written to its out_idx
 * cells.  result[0] += stripes recovered, result[1] = min(result[1], lowest
 * stripe left unrecoverable), result[2] += cells regenerated, result[3] +=
 * stripes left unrecoverable; the host presets {0, UINT64_MAX, 0, 0}.
 * bytewise as for verify.  A block row takes `grp` consecutive stripes (1 ..
 * 64: their mask words are one load and a ballot) and at most grid_x blocks
 * share them and stride over a stripe's 4 KiB columns.  sparse = 0: grp =
 * ECG_RM_DENSE_GRP and a block per column up to ECG_RM_DENSE_GRID_X (every
 * stripe has work: the product's grid); 1: grp = 64 and at most
 * ECG_REPAIR_GRID_X column blocks (few stripes have work: a clean batch costs
 * S / 64 * grid_x blocks of one load each).  cfg: grid_x / grid_y override
 * either.
 * cells_dev == NULL: the strided image above (src == dst and equal strides,
 * hipErrorInvalidValue otherwise).  Otherwise ecg_recover_masks_ptrs: the same
 * recovery with the cells of stripe s at the addresses cells_dev[s * (k + p) +
 * c], c = 0 .. k+p-1 in logical cell order (device memory, read only for the
 * launch); p->src / dst and the strides are then unused.
 * bytewise = 0: the 16-byte lane kernel -- strided: base, stride and cell_bytes
 * multiples of 16; cell table: EVERY table entry 16-byte aligned (the host's
 * check: the launcher does not read the table) and cell_bytes % 16 == 0
 * (hipErrorInvalidValue otherwise); 1: the byte-granular kernel.
 * *kernel: ecg_recover_masks_kernel<k, p> / ecg_recover_masks_byte_kernel, or
 * their ecg_recover_masks_ptr_* counterparts over a table. */
#define ECG_RM_DENSE_GRP 1u
#define ECG_RM_DENSE_GRID_X 256u
int ecg_k_launch_recover_masks(const ecg_mm_params_t *p, const void *settbl, const uint64_t *cells_dev,
			       const uint32_t *masks, uint64_t *result, int bytewise, int sparse,
			       const ecg_launch_cfg_t *cfg, void *stream, const char **kernel);
/* ecg_update_masks: p->src / p->src2 = the old / new cells (stripe s at +
 * s * src_stripe_stride, the same stride for both; cell j at + j * cell_bytes,
 * or with `packed` the cell of the mask's i-th set bit at + i * cell_bytes),
 * p->dst = the parity (row r of stripe s at dst_cell_off[r] + s *
 * dst_stripe_stride), p->k, p->rows = p, cell_bytes, nstripes, and p->tbl[r][j]
 * the Cauchy parity rows for every j < k.  For every stripe whose mask reads
 * as 1 .. k cells (ecg_update_mask_read), parity[r] ^= XOR_{j in mask}
 * tbl[r][j] * (old_j ^ new_j).  result[0] += stripes updated, result[1] =
 * min(result[1], lowest stripe with a bit at or above k), result[2] += cells
 * applied, result[3] += stripes with such a bit; the host presets {0,
 * UINT64_MAX, 0, 0}.  bytewise = 0: the 16-byte lane kernel (every address,
 * stride and cell_bytes a multiple of 16; hipErrorInvalidValue otherwise), 1:
 * the byte-granular kernel.  Block rows of `grp` stripes and the two grids as
 * ecg_k_launch_recover_masks (sparse = 0: ECG_RM_DENSE_GRP and up to
 * ECG_RM_DENSE_GRID_X column blocks; 1: 64 and ECG_REPAIR_GRID_X); cfg:
 * grid_x / grid_y override either.
 * cells_dev == NULL: the strided operands above.  Otherwise
 * ecg_update_masks_ptrs: the same update with the cells of stripe s at the
 * addresses cells_dev[s * (2k + p) + c] -- c < k old cell c, k <= c < 2k new
 * cell c - k, 2k <= c parity row c - 2k (device memory, read only for the
 * launch); p->src / src2 / dst, the strides and dst_cell_off are then unused
 * and `packed` must be 0 (hipErrorInvalidValue).  bytewise = 0 over a table:
 * EVERY table entry 16-byte aligned (the host's check: the launcher does not
 * read the table) and cell_bytes % 16 == 0.
 * *kernel: ecg_update_masks_kernel<p> / ecg_update_masks_byte_kernel, or their
 * ecg_update_masks_ptr_* counterparts over a table.
 * The launcher of ecg_agg_masks over the same operands, ecg_k_launch_agg_masks
 * (the same file), is declared in host/ecg_internal.h beside the host code
 * that calls it. */
int ecg_k_launch_update_masks(const ecg_mm_params_t *p, const uint64_t *cells_dev, const uint32_t *masks,
			      uint64_t *result, int packed, int bytewise, int sparse, const ecg_launch_cfg_t *cfg,
			      void *stream, const char **kernel);
/* ecg_csum_mask (kernels/ecg_csum_kernels.hip): masks[s] |= 1u << (first_cell
 * + i) when any of the nch checksums of len (2, 4 or 8) bytes at index
 * s*stripe_stride + i*cell_stride + c differs between got and want. */
int ecg_k_launch_csum_mask(const void *got, const void *want, uint32_t nstripes, uint32_t ncells,
			   uint32_t nch, uint64_t stripe_stride, uint64_t cell_stride, uint32_t first_cell,
			   uint32_t len, uint32_t *masks, void *stream, const char **kernel);
/* ecg_csum_masked and, with p->cells_dev, ecg_csum_masked_ptrs (kernels/
 * ecg_csum_kernels.hip); max_blocks 0 = default. */
int ecg_k_launch_csum_masked(const ecg_csum_masked_params_t *p, void *stream, uint32_t max_blocks,
			     const char **kernel);
/* ecg_csum_cells_ptrs: every cell of the table p->cells_dev (p->ncells entries). */
int ecg_k_launch_csum_cells(const ecg_csum_masked_params_t *p, void *stream, uint32_t max_blocks,
			    const char **kernel);
/* Whether the device serves misaligned dword loads and stores (the unaligned
 * access mode the ROCm driver enables on gfx9+), which the product kernels
 * use for destinations off a dword boundary and for partial columns of
 * unaligned sources: 4 lanes copy dwords from src+1+4i to dst+3+4i of small
 * scratch buffers and the bytes are compared.  *ok = 1 when they arrived
 * intact.  Synchronous on `stream`. */
int ecg_k_unaligned_check(void *stream, int *ok);
/* Tiles one segment occupies (0 when len == 0). */
uint64_t ecg_k_copy_tiles(uint64_t dst, uint64_t len);
/* A launch's table (pointer table, update records, copy segments) from the
 * pinned host buffer it was written into to device memory: a kernel reading
 * the host words over PCIe at system scope, queued on `stream` like any
 * launch -- where a small hipMemcpyAsync behind running work keeps the
 * calling thread busy in the runtime until that work drains. */
int ecg_k_launch_fetch(const uint64_t *host_src, uint64_t *dst, uint32_t nwords, void *stream);
/* One launch of ntiles workgroups over nseg segments (segs_dev in device memory). */
int ecg_k_launch_copy_segs(const ecg_copy_seg_t *segs_dev, uint32_t nseg, uint64_t ntiles,
			   void *stream, const char **kernel);
/* Implemented in kernels/ecg_kernels.hip.  Returns a hipError_t value. */
int ecg_k_launch_matmul(const ecg_mm_params_t *p, const ecg_launch_cfg_t *cfg,
			void *stream, const char **kernel);
/* One-cell product with a per-stripe coefficient column (p->k == 1):
 * dst[s][r] = tbl[r][sel_dev[s]] * src[s]; tables for columns < ncols <= 16.
 * 16-byte aligned operands only (hipErrorInvalidValue otherwise). */
int ecg_k_launch_matmul_sel(const ecg_mm_params_t *p, const uint8_t *sel_dev, uint32_t ncols,
			    void *stream, const char **kernel);
/* Streaming kernels used only to measure the box's achievable HBM rates:
 * mode 0 copy, 1 read-only, 2 write-only. */
int ecg_k_launch_copy(const void *src, void *dst, uint64_t bytes, int mode, void *stream,
		      uint32_t max_blocks, const char **kernel);
/* Fused product + checksum (kernels/ecg_fused_kernels.hip).  Returns 1 (and
 * launches nothing) when the operands are not 16-byte aligned, or when
 * q->src_out is set and the shape has no SRC instantiation. */
int ecg_k_launch_matmul_csum(const ecg_mm_params_t *p, const ecg_mmcs_params_t *q,
			     const ecg_launch_cfg_t *cfg, void *stream, const char **kernel);
/* Compare n checksums of len (2, 4 or 8) bytes: result[0] += mismatches,
 * result[1] = min(result[1], lowest mismatching index); the host presets
 * result to {0, UINT64_MAX} (kernels/ecg_csum_kernels.hip). */
int ecg_k_launch_csum_compare(const void *got, const void *want, uint64_t n, uint32_t len,
			      uint64_t *result, void *stream, const char **kernel);
/* The common alignment (16, 8, 4 or 1 bytes) of every cell address of a
 * product launch: the lane access granule the product kernels use. */
uint32_t ecg_k_align_granule(const ecg_mm_params_t *p);
/* Pointer-table product (kernels/ecg_ptr_kernels.hip): cells_dev[s*(k+rows)+j]
 * = device address of input cell j / output cell j-k of stripe s.  granule:
 * 16 = every address 16-byte aligned; 4 = inputs dword-aligned; 2 = k = 8
 * with an input off a 16-byte boundary (16-byte lanes, funnel-shifted); 1 =
 * an input at any byte -- with outputs at any byte in the last three (stored
 * misaligned, so they need the device's unaligned access mode); 0 = the
 * byte-granular kernel (ecg_ptrs.c ptr_granule).
 * lens_dev == NULL (spans_dev NULL, nspans = max_cols = 0): every cell is
 * p->cell_bytes long.  Otherwise ecg_matmul_ptrs_lens: the cells of stripe s
 * are lens_dev[s] bytes long, and the work is the nspans records spans_dev[i] =
 * stripe | (uint64_t)first column << 32 (4 KiB columns): span i covers at most
 * ECG_LENS_SPAN_COLS columns of its stripe's cells from that column on, the
 * spans of a stripe cover its cells once, a stripe of length 0 has none (its
 * table row is never read).  max_cols = the most columns a span holds, 1 ..
 * ECG_LENS_SPAN_COLS (hipErrorInvalidValue otherwise): grid.x.  p->cell_bytes
 * is then the OR of every length (its low bits choose the lanes as a cell
 * size's do; 0 = nothing to launch) and the kernels read neither it nor
 * p->nstripes.  All three arrays are device memory, read only for the launch.
 * *kernel: ecg_mm_ptr_kernel<k,rows[,gG]> / ecg_mm_ptr_byte_kernel, or their
 * ecg_mm_ptr_lens_* counterparts. */
#define ECG_LENS_SPAN_COLS 16u
int ecg_k_launch_matmul_ptrs(const ecg_mm_params_t *p, const uint64_t *cells_dev, int granule,
			     const uint64_t *lens_dev, const uint64_t *spans_dev, uint32_t nspans, uint32_t max_cols,
			     const ecg_launch_cfg_t *cfg, void *stream, const char **kernel);
/* Per-request delta updates through a pointer table (the batching queue's
 * device-cell aggregation updates, ecg_update_ptrs):  item s of the launch,
 * a record of ECG_UPD_REC(rows) uint64_t at items_dev + s * ECG_UPD_REC(rows):
 *   [0, rows)            parity cell r (device address; updated in place)
 *   rows + 2m, + 2m + 1  old / new cell of pair m (m < ECG_UPD_MU)
 *   rows + 2 MU          byte m = coefficient column of pair m (< ncols)
 *   rows + 2 MU + 1      n, the pairs in use (1 .. ECG_UPD_MU)
 *   parity[r] ^= XOR_{m<n} tbl[r][col_m] * (old_m ^ new_m)
 * p->nstripes = items, p->rows, p->cell_bytes and p->tbl[r][0 .. ncols) are
 * used.  No two items of one launch may share a parity byte (the host splits
 * such requests into ordered launches).  granule: 16 (every address and C
 * 16-byte aligned), 4 (C % 4 == 0; addresses dword-aligned, or any address on
 * a device that serves misaligned dwords), 0 = one byte per lane. */
#define ECG_UPD_MU 8
#define ECG_UPD_REC(rows) ((rows) + 2 * ECG_UPD_MU + 2)
int ecg_k_launch_update_ptrs(const ecg_mm_params_t *p, const uint64_t *items_dev, uint32_t ncols, int granule,
			     void *stream, const char **kernel);
/* Chunked checksums (kernels/ecg_csum_kernels.hip). max_blocks 0 = default. */
int ecg_k_launch_csum(const ecg_csum_params_t *p, void *stream, uint32_t max_blocks,
		      const char **kernel);
#ifdef __cplusplus
}
#endif

#endif
