/*
 * ecg_csum.c -- host side of the chunked checksums (include/ecg_csum.h):
 * CRC tables built from the polynomials, per-context device copies, chunk
 * geometry of an extent (ref:src/common/checksum.c:1444-1565), launch.
 */
#include <stdlib.h>
#include <string.h>

#include "ecg_internal.h"
#include "../../../include/ecg_csum.h"

struct crc_def {
	int width;
	int refl;
	uint64_t poly;		/* reflected for refl, MSB-first otherwise */
	uint64_t init, xorout;
};

/* ISA-L crc16_t10dif / crc32_iscsi / crc64_ecma_refl as DAOS calls them
 * (seed 0; crc64 inverts the register on entry and exit). */
static const struct crc_def g_defs[4] = {
	[ECG_HASH_CRC16] = {16, 0, 0x8BB7, 0, 0},
	[ECG_HASH_CRC32] = {32, 1, 0x82F63B78u, 0, 0},
	[ECG_HASH_CRC64] = {64, 1, 0xC96C5795D7870F42ull, ~0ull, ~0ull},
};

/* CRC table kinds are fixed per kernel (ecg_kernels.hip CS_TB, the tables of
 * ecg_csum_kernels.hip): standalone kernels use the nibble tables
 * (SDWA-addressed, conflict-free; profiles/r03/crc_sq/), their byte-granular
 * variants the 5-bit tables; the fused kernels the byte tables for crc64 and
 * for crc32 at EC_8P2, the 5-bit tables elsewhere (profiles/r02/fused_tables_ab/,
 * profiles/r03/fused_tb3/, fused_tb4/).  The other kinds were A/B builds. */

int ecg_csum_len(int type)
{
	switch (type) {
	case ECG_HASH_CRC16:
		return 2;
	case ECG_HASH_CRC32:
	case ECG_HASH_ADLER32:
		return 4;
	case ECG_HASH_CRC64:
		return 8;
	default:
		return -ECG_DER_NOTSUPPORTED;
	}
}

uint64_t ecg_csum_record_chunksize(uint64_t chunksize, uint64_t rec_size)
{
	if (rec_size == 0 || chunksize == 0)
		return 0;
	if (rec_size > chunksize)
		return rec_size;
	return chunksize / rec_size * rec_size;
}

uint32_t ecg_csum_chunk_count(uint64_t chunksize, uint64_t rec_size, uint64_t rx_idx,
			      uint64_t rx_nr)
{
	const uint64_t rcs = ecg_csum_record_chunksize(chunksize, rec_size);
	uint64_t per, lo, hi_end;

	if (rcs == 0 || rx_nr == 0)
		return 0;
	if (rx_nr == 1)
		return 1;
	per = rcs / rec_size;
	lo = rx_idx / per;
	hi_end = (rx_idx + (rx_nr - 1)) / per;
	return (uint32_t)(hi_end - lo + 1);
}

/* CRC register after one zero byte: c * x^8 mod P */
static uint64_t zero_byte(const struct crc_def *d, uint64_t c)
{
	const uint64_t mask = d->width == 64 ? ~0ull : (1ull << d->width) - 1;

	for (int b = 0; b < 8; b++) {
		if (d->refl)
			c = (c & 1) ? (c >> 1) ^ d->poly : c >> 1;
		else
			c = ((c >> (d->width - 1)) & 1) ? ((c << 1) & mask) ^ d->poly : (c << 1) & mask;
	}
	return c;
}

/* "1" in the register representation */
static uint64_t crc_one(const struct crc_def *d)
{
	return d->refl ? 1ull << (d->width - 1) : 1;
}

/* a * b mod P (same representations as the device mulmod) */
static uint64_t crc_mulmod(const struct crc_def *d, uint64_t a, uint64_t b)
{
	const uint64_t mask = d->width == 64 ? ~0ull : (1ull << d->width) - 1;
	uint64_t p = 0;

	for (int i = d->width - 1; i >= 0; i--) {
		if (d->refl) {
			if ((a >> i) & 1)
				p ^= b;
			b = (b & 1) ? (b >> 1) ^ d->poly : b >> 1;
		} else {
			p = ((p >> (d->width - 1)) & 1) ? ((p << 1) & mask) ^ d->poly : (p << 1) & mask;
			if ((a >> i) & 1)
				p ^= b;
		}
	}
	return p;
}

/* x^(-8z) mod P: x^-1 = (P - 1) / x since P(0) = 1 */
static uint64_t crc_unshift(const struct crc_def *d, uint64_t z)
{
	const uint64_t mask = d->width == 64 ? ~0ull : (1ull << d->width) - 1;
	const uint64_t xinv = d->refl ? (((d->poly << 1) & mask) | 1)
				      : ((1ull << (d->width - 1)) | (d->poly >> 1));
	uint64_t r = crc_one(d), b = xinv;

	for (uint64_t e = 8 * z; e; e >>= 1) {	/* square and multiply */
		if (e & 1)
			r = crc_mulmod(d, r, b);
		b = crc_mulmod(d, b, b);
	}
	return r;
}

/* x^(8n) mod P: "1" moved through n zero bytes, by square and multiply */
static uint64_t crc_xpow8(const struct crc_def *d, uint64_t n)
{
	uint64_t r = crc_one(d), b = zero_byte(d, crc_one(d));

	for (; n; n >>= 1) {
		if (n & 1)
			r = crc_mulmod(d, r, b);
		b = crc_mulmod(d, b, b);
	}
	return r;
}

/* Workgroup-per-chunk CRC: shift of each wave's slice to the end of a chunk
 * of m 1 KiB steps (ecg_kabi.h split_sh), cached per context by (type, m). */
static void split_shifts(ecg_ctx_t *ctx, int type, uint64_t m, uint64_t *sh)
{
	const uint64_t ms = ECG_CSUM_SPLIT_MS(m);
	struct ecg_split_ent *e;

	pthread_mutex_lock(&ctx->lock);
	for (int i = 0; i < ECG_NSPLIT_CACHE; i++) {
		e = &ctx->split_cache[i];
		if (e->valid && e->type == type && e->m == m) {
			memcpy(sh, e->sh, sizeof(e->sh));
			pthread_mutex_unlock(&ctx->lock);
			return;
		}
	}
	e = &ctx->split_cache[ctx->split_next++ % ECG_NSPLIT_CACHE];
	for (int w = 0; w < ECG_CSUM_SPLIT_NW; w++) {
		const uint64_t i0 = w * ms < m ? w * ms : m, i1 = i0 + ms < m ? i0 + ms : m;

		e->sh[w] = crc_xpow8(&g_defs[type], (m - i1) * ECG_CSUM_STRIDE);
	}
	e->type = type;
	e->m = m;
	e->valid = 1;
	memcpy(sh, e->sh, sizeof(e->sh));
	pthread_mutex_unlock(&ctx->lock);
}

/* linear map "shift by n zero bytes" as NB byte tables at t */
static void build_shift(const struct crc_def *d, int n, uint64_t *t)
{
	const int nb = d->width / 8;
	uint64_t basis[64];

	for (int i = 0; i < d->width; i++) {
		uint64_t c = 1ull << i;

		for (int z = 0; z < n; z++)
			c = zero_byte(d, c);
		basis[i] = c;
	}
	for (int j = 0; j < nb; j++)
		for (int v = 0; v < 256; v++) {
			uint64_t c = 0;

			for (int b = 0; b < 8; b++)
				if (v & (1 << b))
					c ^= basis[8 * j + b];
			t[(size_t)j * 256 + v] = c;
		}
}

/* raw CRC (zero register) of len bytes */
static uint64_t crc_raw(const struct crc_def *d, const unsigned char *buf, int len)
{
	const uint64_t mask = d->width == 64 ? ~0ull : (1ull << d->width) - 1;
	uint64_t c = 0;

	for (int i = 0; i < len; i++) {
		c ^= d->refl ? (uint64_t)buf[i] : (uint64_t)buf[i] << (d->width - 8);
		c = zero_byte(d, c) & mask;
	}
	return c;
}

/* basis[k]: the raw CRC of the 16-byte piece whose only set bit is bit k,
 * followed by `zeros` zero bytes -- what the p5 and q4 tables are XORs of */
static void piece_basis(const struct crc_def *d, uint64_t zeros, uint64_t basis[128])
{
	const uint64_t sh = zeros ? crc_xpow8(d, zeros) : 0;
	unsigned char piece[16];

	for (int k = 0; k < 128; k++) {
		memset(piece, 0, sizeof(piece));
		piece[k / 8] = (unsigned char)(1u << (k % 8));
		basis[k] = crc_raw(d, piece, 16);
		if (zeros)
			basis[k] = crc_mulmod(d, basis[k], sh);
	}
}

/* 5-bit field tables (ecg_kabi.h p5 / a5): field (dword j, field i) covers
 * bits 32j + 5i .. +4 of the piece or register; entry v = XOR of the basis
 * images of v's set bits.  a5 for a shift of n zero bytes. */
static void build_p5(const struct crc_def *d, uint64_t zeros, uint64_t *p5)
{
	uint64_t basis[128];

	piece_basis(d, zeros, basis);
	for (int f = 0; f < ECG_CSUM_NF5; f++) {
		const int j = f / 7, i = f % 7;

		for (int v = 0; v < 32; v++) {
			uint64_t c = 0;

			for (int t = 0; t < 5; t++)
				if ((v >> t) & 1 && 5 * i + t < 32)
					c ^= basis[32 * j + 5 * i + t];
			p5[(size_t)f * 32 + v] = c;
		}
	}
}

/* nibble tables (ecg_kabi.h q4 / a4): nibble t covers bits 4t..4t+3 of the
 * piece (q4, the piece followed by `zeros` zero bytes) or of the register
 * shifted by n zero bytes (a4) */
static void build_q4(const struct crc_def *d, uint64_t zeros, uint64_t *q4)
{
	uint64_t basis[128];

	piece_basis(d, zeros, basis);
	for (int t = 0; t < 32; t++)
		for (int v = 0; v < 16; v++) {
			uint64_t c = 0;

			for (int b = 0; b < 4; b++)
				if ((v >> b) & 1)
					c ^= basis[4 * t + b];
			q4[(size_t)t * 16 + v] = c;
		}
}

static void build_a4(const struct crc_def *d, uint64_t n, uint64_t *a4)
{
	const uint64_t sh = crc_xpow8(d, n);

	for (int t = 0; t < d->width / 4; t++)
		for (int v = 0; v < 16; v++) {
			uint64_t c = 0;

			for (int b = 0; b < 4; b++)
				if ((v >> b) & 1)
					c ^= crc_mulmod(d, 1ull << (4 * t + b), sh);
			a4[(size_t)t * 16 + v] = c;
		}
}

static void build_a5(const struct crc_def *d, uint64_t n, uint64_t *a5)
{
	const uint64_t sh = crc_xpow8(d, n);
	const int na = d->width == 16 ? 4 : 7 * d->width / 32;

	for (int f = 0; f < na; f++) {
		const int h = d->width == 16 ? 0 : f / 7, i = d->width == 16 ? f : f % 7;

		for (int v = 0; v < 32; v++) {
			uint64_t c = 0;

			for (int t = 0; t < 5; t++) {
				const int bit = 32 * h + 5 * i + t;

				if ((v >> t) & 1 && 5 * i + t < 32 && bit < d->width)
					c ^= crc_mulmod(d, 1ull << bit, sh);
			}
			a5[(size_t)f * 32 + v] = c;
		}
	}
}

/* Device table image (layout in ecg_kabi.h): sl, sh (1 KiB), k64, sh4k,
 * k256, p2, sh256, p5, a5 (1 KiB, 256 B, 4 KiB); entries of 4 (W <= 32) or
 * 8 (W = 64) bytes. */
static void *build_crc_tables(const struct crc_def *d, size_t *bytes)
{
	const int nb = d->width / 8, es = d->width == 64 ? 8 : 4;
	const size_t n = ECG_CSUM_TBL_ENTRIES(nb);
	uint64_t *t = calloc(n, sizeof(uint64_t));
	unsigned char *img;
	uint64_t c;

	if (t == NULL)
		return NULL;
	/* sl[j][v] (j < NB) and s16[j][v] (j < 16): register after byte v (from
	 * zero) and then j zero bytes */
	for (int v = 0; v < 256; v++) {
		uint64_t c = d->refl ? (uint64_t)v : (uint64_t)v << (d->width - 8);

		c = zero_byte(d, c);
		for (int j = 0; j < 16; j++) {
			if (j < nb)
				t[(size_t)j * 256 + v] = c;
			t[ECG_CSUM_OFF_S16(nb) + (size_t)j * 256 + v] = c;
			c = zero_byte(d, c);
		}
	}
	build_shift(d, ECG_CSUM_STRIDE, t + ECG_CSUM_OFF_SH(nb));
	build_shift(d, ECG_MMCS_STRIDE, t + ECG_CSUM_OFF_SH4K(nb));
	build_shift(d, ECG_CSUM_GSTRIDE, t + ECG_CSUM_OFF_SH256(nb));
	/* k64[lane] = x^(8*16*(63-lane)), k256[t] = x^(8*16*(255-t)) mod P:
	 * "1" moved through that many zero bytes, walking down from the last */
	c = crc_one(d);
	for (int l = 255; l >= 0; l--) {
		if (l >= 192)
			t[ECG_CSUM_OFF_K64(nb) + (l - 192)] = c;
		t[ECG_CSUM_OFF_K256(nb) + l] = c;
		for (int z = 0; z < 16; z++)
			c = zero_byte(d, c);
	}
	/* p2[j] = x^(8*2^j) mod P */
	c = zero_byte(d, crc_one(d));
	for (int j = 0; j < ECG_CSUM_NP2; j++) {
		t[ECG_CSUM_OFF_P2(nb) + j] = c;
		c = crc_mulmod(d, c, c);
	}
	build_p5(d, 0, t + ECG_CSUM_OFF_P5(nb));
	for (int u = 1; u < ECG_CSUM_P5U; u++) {
		build_p5(d, (uint64_t)u * ECG_CSUM_STRIDE,
			 t + ECG_CSUM_OFF_P5X_1K(nb) + (size_t)(u - 1) * ECG_CSUM_NF5 * 32);
		build_p5(d, (uint64_t)u * ECG_CSUM_GSTRIDE,
			 t + ECG_CSUM_OFF_P5X_256(nb) + (size_t)(u - 1) * ECG_CSUM_NF5 * 32);
	}
	for (int u = 1; u < ECG_MMCS_P5U; u++)
		build_p5(d, (uint64_t)u * ECG_MMCS_STRIDE,
			 t + ECG_CSUM_OFF_P5X_4K(nb) + (size_t)(u - 1) * ECG_CSUM_NF5 * 32);
	build_a5(d, (uint64_t)ECG_MMCS_P5U * ECG_MMCS_STRIDE, t + ECG_CSUM_OFF_A5_32K(nb));
	if (d->refl) {
		/* nibl[n][l] = (n << (W - 4)) * x^(8*16*(63-l)); r4[m] = m * x^4 */
		for (int l = 0; l < 64; l++)
			for (int n = 0; n < 16; n++)
				t[ECG_CSUM_OFF_NIBL(nb) + (size_t)n * 64 + l] =
					crc_mulmod(d, (uint64_t)n << (d->width - 4), t[ECG_CSUM_OFF_K64(nb) + l]);
		for (int m = 0; m < 16; m++) {
			uint64_t c = (uint64_t)m;

			for (int b = 0; b < 4; b++)
				c = (c >> 1) ^ (d->poly & (0 - (c & 1)));
			t[ECG_CSUM_OFF_R4(nb) + m] = c;
		}
	}
	build_a5(d, ECG_CSUM_STRIDE, t + ECG_CSUM_OFF_A5_1K(nb));
	build_a5(d, ECG_CSUM_GSTRIDE, t + ECG_CSUM_OFF_A5_256(nb));
	build_a5(d, ECG_MMCS_STRIDE, t + ECG_CSUM_OFF_A5_4K(nb));
	for (int u = 0; u < ECG_CSUM_P5U; u++) {
		build_q4(d, (uint64_t)u * ECG_CSUM_STRIDE, t + ECG_CSUM_OFF_Q4_1K(nb) + (size_t)u * ECG_CSUM_NQ4);
		build_q4(d, (uint64_t)u * ECG_CSUM_GSTRIDE, t + ECG_CSUM_OFF_Q4_256(nb) + (size_t)u * ECG_CSUM_NQ4);
	}
	build_a4(d, (uint64_t)ECG_CSUM_P5U * ECG_CSUM_STRIDE, t + ECG_CSUM_OFF_A4_4K(nb));
	build_a4(d, (uint64_t)ECG_CSUM_P5U * ECG_CSUM_GSTRIDE, t + ECG_CSUM_OFF_A4_1K(nb));
	for (int u = 0; u < ECG_MMCS_P5U; u++)
		build_q4(d, (uint64_t)u * ECG_MMCS_STRIDE, t + ECG_CSUM_OFF_Q4_4K(nb) + (size_t)u * ECG_CSUM_NQ4);
	build_a4(d, (uint64_t)ECG_MMCS_P5U * ECG_MMCS_STRIDE, t + ECG_CSUM_OFF_A4_32K(nb));

	*bytes = n * (size_t)es;
	if (es == 8)
		return t;
	img = malloc(*bytes);
	if (img)
		for (size_t i = 0; i < n; i++) {
			uint32_t w = (uint32_t)t[i];

			memcpy(img + 4 * i, &w, 4);
		}
	free(t);
	return img;
}

/* Device copy of a type's tables, built once per context (ctx->lock). */
static int crc_tables(ecg_ctx_t *ctx, int type, const void **out)
{
	int rc = 0;

	pthread_mutex_lock(&ctx->lock);
	if (ctx->csum_tbl[type] == NULL) {
		size_t bytes = 0;
		void *img = build_crc_tables(&g_defs[type], &bytes), *dev = NULL;
		hipError_t e;

		if (img == NULL) {
			rc = ecg_fail(-ECG_DER_NOMEM, "csum tables");
		} else {
			e = hipMalloc(&dev, bytes);
			if (e == hipSuccess)
				e = hipMemcpy(dev, img, bytes, hipMemcpyHostToDevice);
			if (e != hipSuccess) {
				if (dev)
					(void)hipFree(dev);
				rc = ecg_hip_fail(e, "csum tables");
			} else {
				ctx->csum_tbl[type] = dev;
			}
			free(img);
		}
	}
	*out = ctx->csum_tbl[type];
	pthread_mutex_unlock(&ctx->lock);
	return rc;
}

void ecg_csum_ctx_fini(ecg_ctx_t *ctx)
{
	for (int i = 0; i < ECG_NCSUM_TBL; i++)
		if (ctx->csum_tbl[i]) {
			(void)hipFree(ctx->csum_tbl[i]);
			ctx->csum_tbl[i] = NULL;
		}
	for (int i = 0; i < ECG_NKH_CACHE; i++)
		if (ctx->kh_cache[i].dev) {
			(void)hipFree(ctx->kh_cache[i].dev);
			memset(&ctx->kh_cache[i], 0, sizeof(ctx->kh_cache[i]));
		}
}

/* Columns per fused-kernel work item (a whole chunk when shorter): fewer
 * columns per item walk a chunk with more workgroups in parallel, more
 * amortise the per-item reduction.  Measured A/B in one process on random
 * data (tools/tune12.py, tools/fused_libs.py; profiles/r01/tune12.json,
 * profiles/r02/fused_libs/, profiles/r03/fused_tail/); ecg_set_fused_cols /
 * ECG_FUSED_COLS override. */
static int g_fused_cols_env;
static pthread_once_t g_fused_cols_once = PTHREAD_ONCE_INIT;

static void fused_cols_init(void)
{
	const char *e = getenv("ECG_FUSED_COLS");

	g_fused_cols_env = e ? atoi(e) : 0;
	if (g_fused_cols_env < 0)
		g_fused_cols_env = 0;
}

static uint32_t fused_cols(const ecg_ctx_t *ctx, uint64_t m, int type, int k, int rows, int src)
{
	/* tools/fused_libs.py, profiles/r02/fused_libs/, profiles/r03/fused_tail/:
	 * one output row (a parity shard's rebuild) 4; >= 2 rows: 4 for k >= 8
	 * (EC_8P2 crc32 +8 % vs +18 % at 8; crc64, now that its item tail reads no
	 * HBM, +12.5 % vs +20 %), 8 for k <= 4 (EC_4P2 crc32 +8 % vs +15 % at 4) */
	/* round 3, after the item tail stopped reading HBM: crc32 at EC_8P2 (byte
	 * tables) walks 2 columns best -- +6.0 / +7.3 % vs +9.0 / +9.9 % at 4 on two
	 * boxes; k = 16 and one or three rows keep 4 (profiles/r03/fused_cols/) */
	/* the SRC instantiations finish k + rows registers per item: 8 columns for
	 * every measured shape (tools/bench_csum_all.py --sweep-cols,
	 * profiles/r07/csum_all/: EC_8P2 x 512 x 1 MiB crc32 1.58 ms at 2 columns,
	 * 1.43 at 4, 1.33 at 8, 1.33 at 16; crc64 2.39 / 2.00 / 1.83 / 1.82;
	 * EC_16P2 x 1024 x 128 KiB crc32 0.73 / 0.65 / 0.63 / 0.62) */
	const uint64_t dflt = src ? 8
			    : type == ECG_HASH_CRC32 && k == 8 && rows == 2 ? 2 : rows == 1 ? 4 : k >= 8 ? 4 : 8;
	const int env = ctx->fused_cols ? (int)ctx->fused_cols
					: (pthread_once(&g_fused_cols_once, fused_cols_init), g_fused_cols_env);

	if (env > 0)
		return (uint32_t)((uint64_t)env < m ? (uint64_t)env : m);
	return (uint32_t)(m < dflt ? m : dflt);
}

/* Device table of the fused kernel's per-item multipliers (ecg_kabi.h
 * ecg_mmcs_params kh): row h < nh of a full chunk of m columns, rows nh + h of
 * the last chunk (m_last columns, z padding bytes):
 *   crc16:      kh[row][t] = x^(8*(16*(255-t) + 4096*(columns after item h))) * x^(-8z)
 *   reflected:  the factor f(row, w) = x^(8*(1024*(3-w) + 4096*(columns after
 *               item h))) * x^(-8z) of wave w as its W bit-products,
 *               kh[row][w][b] = e_b * f(row, w) (e_b: the register with only
 *               bit b set; entries b >= W zero) -- the kernel applies the lane
 *               part from the LDS nibl tables and then f bit-parallel, lane b
 *               contributing kh[row][w][b] when bit b of the wave's sum is set
 * Cached per context by (type, chunk bytes, columns per item, last length). */
static int fused_kh(ecg_ctx_t *ctx, int type, uint64_t rcs, uint64_t last, uint32_t ncols,
		    uint32_t nh, uint32_t nh_last, const void **out)
{
	const struct crc_def *d = &g_defs[type];
	const uint64_t m = rcs / ECG_MMCS_STRIDE;
	const uint64_t m_last = (last + ECG_MMCS_STRIDE - 1) / ECG_MMCS_STRIDE;
	const uint64_t z = m_last * ECG_MMCS_STRIDE - last;
	const size_t es = d->width == 64 ? 8 : 4, nrow = (size_t)nh + nh_last;
	/* entries per row: 4 waves x 64 bit-products, or 256 threads */
	const size_t per = d->refl ? 4 * 64 : 256;
	struct ecg_kh_ent *e;
	uint64_t k256[256];
	unsigned char *img;
	void *dev = NULL;
	hipError_t he;
	int rc = 0;

	pthread_mutex_lock(&ctx->lock);
	for (int i = 0; i < ECG_NKH_CACHE; i++) {
		e = &ctx->kh_cache[i];
		if (e->valid && e->type == type && e->rcs == rcs && e->last == last && e->ncols == ncols) {
			*out = e->dev;
			pthread_mutex_unlock(&ctx->lock);
			return 0;
		}
	}
	img = malloc(nrow * per * es);
	if (img == NULL) {
		pthread_mutex_unlock(&ctx->lock);
		return ecg_fail(-ECG_DER_NOMEM, "fused csum multipliers");
	}
	k256[255] = crc_one(d);
	for (int t = 254; t >= 0; t--)
		k256[t] = crc_mulmod(d, k256[t + 1], crc_xpow8(d, 16));
	for (size_t row = 0; row < nrow; row++) {
		const int lastc = row >= nh;
		const uint64_t h = lastc ? row - nh : row, mc = lastc ? m_last : m;
		const uint64_t end = (h + 1) * ncols < mc ? (h + 1) * ncols : mc;
		uint64_t sh = crc_xpow8(d, (mc - end) * ECG_MMCS_STRIDE);

		if (lastc)
			sh = crc_mulmod(d, sh, crc_unshift(d, z));
		uint64_t f = 0;

		for (size_t t = 0; t < per; t++) {
			uint64_t v;

			if (d->refl) {
				/* wave w's factor (k256[64 w + 63] = x^(8*16*(192-64w)) =
				 * x^(8*1024*(3-w))) times the item's shift, as bit-products */
				const size_t w = t / 64, b = t % 64;

				if (b == 0)
					f = crc_mulmod(d, k256[64 * w + 63], sh);
				v = b < (size_t)d->width ? crc_mulmod(d, (uint64_t)1 << b, f) : 0;
			} else {	/* crc16: thread t's */
				v = crc_mulmod(d, k256[t], sh);
			}
			if (es == 8) {
				memcpy(img + (row * per + t) * 8, &v, 8);
			} else {
				const uint32_t w32 = (uint32_t)v;

				memcpy(img + (row * per + t) * 4, &w32, 4);
			}
		}
	}
	he = hipMalloc(&dev, nrow * per * es);
	if (he == hipSuccess)
		he = hipMemcpy(dev, img, nrow * per * es, hipMemcpyHostToDevice);
	free(img);
	if (he != hipSuccess) {
		if (dev)
			(void)hipFree(dev);
		pthread_mutex_unlock(&ctx->lock);
		return ecg_hip_fail(he, "fused csum multipliers");
	}
	e = &ctx->kh_cache[ctx->kh_next++ % ECG_NKH_CACHE];
	if (e->dev) {
		/* launches queued on any stream may still read the evicted table */
		(void)hipDeviceSynchronize();
		(void)hipFree(e->dev);
	}
	e->valid = 1;
	e->type = type;
	e->rcs = rcs;
	e->last = last;
	e->ncols = ncols;
	e->dev = dev;
	*out = dev;
	pthread_mutex_unlock(&ctx->lock);
	return rc;
}

/* The CRC tables of a hash type (NULL for adler32, which has none).  Takes
 * ctx->lock: fetched before a cell-table call opens its table. */
static int hash_tbl(ecg_ctx_t *ctx, int type, const void **tbl)
{
	*tbl = NULL;
	return type == ECG_HASH_ADLER32 ? 0 : crc_tables(ctx, type, tbl);
}

/* tbl / poly / init / xorout of a zeroed parameter block, which ecg_kabi.h's
 * three have under these names (adler32 leaves them 0) */
#define HASH_FILL(prm, type, table)                                                                           \
	((type) == ECG_HASH_ADLER32                                                                           \
		 ? (void)0                                                                                    \
		 : (void)((prm)->tbl = (table), (prm)->poly = g_defs[type].poly,                              \
			  (prm)->init = g_defs[type].init, (prm)->xorout = g_defs[type].xorout))

int ecg_csum_extents(ecg_ctx_t *ctx, int type, uint64_t chunksize, uint64_t rec_size,
		     uint64_t rx_idx, uint64_t rx_nr, const void *buf, int64_t ext_stride,
		     uint32_t n_ext, void *csums, void *stream)
{
	ecg_csum_params_t prm;
	const uint64_t rcs = ecg_csum_record_chunksize(chunksize, rec_size);
	const void *tbl;
	uint64_t per, first_end;
	/* an extent of 2^32 chunks has an nchunks of 0 (ecg_csum_chunk_count
	 * returns 32 bits) and launches nothing */
	const char *kernel = ECG_NO_LAUNCH_KERNEL;
	int rc, e;

	if (ctx == NULL || (n_ext && rx_nr && (buf == NULL || csums == NULL)) || rcs == 0)
		return ecg_fail(-ECG_DER_INVAL, "csum_extents: bad arguments");
	if (ecg_csum_len(type) < 0)
		return ecg_fail(-ECG_DER_NOTSUPPORTED, "csum_extents: hash type %d not supported",
				type);
	if (rx_nr > UINT64_MAX / rec_size || (rx_nr && rx_nr - 1 > UINT64_MAX - rx_idx))
		return ecg_fail(-ECG_DER_INVAL, "csum_extents: extent overflows");
	if (n_ext == 0 || rx_nr == 0)
		return 0;
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	memset(&prm, 0, sizeof(prm));
	rc = hash_tbl(ctx, type, &tbl);
	if (rc)
		return rc;
	HASH_FILL(&prm, type, tbl);
	/* chunk 0 runs from rx_idx to the end of its aligned chunk (clipped);
	 * the rest are whole chunks, the last one clipped
	 * (csum_recx_chunkidx2range, ref:src/common/checksum.c:1489-1565) */
	per = rcs / rec_size;
	first_end = rx_idx - rx_idx % per + (per - 1);
	if (first_end < rx_idx)		/* csum_chunk_align_ceiling overflow guard */
		first_end = UINT64_MAX;
	if (first_end > rx_idx + (rx_nr - 1))
		first_end = rx_idx + (rx_nr - 1);
	prm.src = buf;
	prm.out = csums;
	prm.ext_stride = ext_stride;
	prm.ext_bytes = rx_nr * rec_size;
	prm.first_bytes = (first_end - rx_idx + 1) * rec_size;
	prm.chunk_bytes = rcs;
	prm.n_ext = n_ext;
	prm.nchunks = ecg_csum_chunk_count(chunksize, rec_size, rx_idx, rx_nr);
	prm.type = (uint32_t)type;
	if (type != ECG_HASH_ADLER32) {
		/* a workgroup per chunk when one wave per chunk would leave fewer
		 * than 4 waves per SIMD and each wave still gets >= 2 KiB steps
		 * (tools/bench_csum.py shape_* rows) */
		const uint64_t total = (uint64_t)n_ext * prm.nchunks;
		const uint64_t steps = (rcs / 16 + 63) / 64;
		const int split = total < 4096 && steps >= 2 * ECG_CSUM_SPLIT_NW;
		const uint64_t lens[3] = {
			prm.first_bytes, rcs,
			prm.nchunks >= 2 ? prm.ext_bytes - prm.first_bytes - (uint64_t)(prm.nchunks - 2) * rcs
					 : prm.first_bytes};

		/* short chunks (<= 8 KiB): a 16-lane group each, so the per-lane
		 * final multiply is paid once per >= 8 pieces instead of per 1-2 */
		const int group = !split && steps <= 8;

		prm.variant = split ? 2 : group ? 3 : 1;
		for (int c = 0; split && c < 3; c++) {
			prm.split_m[c] = ECG_CSUM_STEPS(lens[c]);
			split_shifts(ctx, type, prm.split_m[c], prm.split_sh[c]);
		}
	} else {
		prm.variant = 0;	/* adler32: the kernel picks by shape */
	}
	ecg_trace_push("ecg:csum_extents");
	e = ecg_k_launch_csum(&prm, (void *)ecg_pick_stream(ctx, stream), ctx->csum_blocks, &kernel);
	rc = ecg_launch_done(ctx, e, "csum kernel launch", 1, kernel);
	if (rc == 0)
		ECG_STAT_ADD(ctx, csum_chunks, (uint64_t)prm.n_ext * prm.nchunks);
	return rc;
}

int ecg_set_csum_launch(ecg_ctx_t *ctx, uint32_t max_blocks)
{
	if (ctx == NULL)
		return ecg_fail(-ECG_DER_INVAL, "set_csum_launch: NULL context");
	ctx->csum_blocks = max_blocks;
	return 0;
}

/* The measured default of ecg_csum_all_route: 1 = fused.  tools/
 * bench_csum_all.py (profiles/r07/csum_all/, 32 KiB chunks, 3 alternating
 * rounds, ms fused / two passes): crc32 EC_8P2 x 512 x 1 MiB 1.33 / 1.62,
 * EC_4P2 x 1024 x 1 MiB 1.51 / 1.82, EC_16P2 x 1024 x 128 KiB 0.63 / 0.80;
 * crc64 EC_16P2 0.83 / 0.85 -- fused.  crc64 EC_8P2 1.87 / 1.80 and EC_4P2
 * 1.97 / 1.99 (won one run of the tool, lost another): two passes, as for
 * every shape not measured (crc16, one or three output rows, other k). */
static int csum_all_fused_default(int type, int k, int rows)
{
	if (rows != 2)
		return 0;
	if (type == ECG_HASH_CRC32)
		return k == 4 || k == 8 || k == 16;
	return type == ECG_HASH_CRC64 && k == 16;
}

int ecg_set_fused_cols(ecg_ctx_t *ctx, uint32_t ncols)
{
	if (ctx == NULL || ncols > 4096)
		return ecg_fail(-ECG_DER_INVAL, "set_fused_cols: bad arguments");
	ctx->fused_cols = ncols;
	return 0;
}

int ecg_set_csum_all_route(ecg_ctx_t *ctx, uint32_t route)
{
	if (ctx == NULL || route > 2)
		return ecg_fail(-ECG_DER_INVAL, "set_csum_all_route: bad arguments");
	ctx->csum_all_route = route;
	return 0;
}

/* Whether ecg_encode_csum_all / ecg_recover_csum_all try the fused kernel's
 * SRC instantiation for a shape (1) or run two passes (0).  The default is
 * the fused route only where tools/bench_csum_all.py measured it faster than
 * the two passes by more than their round-to-round spread (DESIGN §11,
 * profiles/r07/csum_all/); shapes it did not measure run two passes. */
int ecg_csum_all_route(const ecg_ctx_t *ctx, int type, int k, int rows)
{
	if (ctx->csum_all_route)
		return ctx->csum_all_route == 1;
	return csum_all_fused_default(type, k, rows);
}

int ecg_csum_compare(ecg_ctx_t *ctx, int type, const void *got, const void *want, uint64_t n,
		     void *result, void *stream)
{
	const int cl = ecg_csum_len(type);
	hipStream_t st;
	hipError_t he;
	const char *kernel = NULL;
	int rc, e;

	if (cl < 0)
		return ecg_fail(-ECG_DER_NOTSUPPORTED, "csum_compare: hash type %d not supported", type);
	if (ctx == NULL || result == NULL || (uintptr_t)result % 8u || (n && (got == NULL || want == NULL)))
		return ecg_fail(-ECG_DER_INVAL, "csum_compare: bad arguments");
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);
	he = hipMemsetAsync(result, 0, 8, st);
	if (he == hipSuccess)
		he = hipMemsetAsync((uint8_t *)result + 8, 0xFF, 8, st);
	if (he != hipSuccess)
		return ecg_hip_fail(he, "csum_compare memset");
	if (n == 0)
		return 0;
	ecg_trace_push("ecg:csum_compare");
	e = ecg_k_launch_csum_compare(got, want, n, (uint32_t)cl, result, (void *)st, &kernel);
	return ecg_launch_done(ctx, e, "csum_compare kernel launch", 1, kernel);
}

int ecg_csum_mask(ecg_ctx_t *ctx, int type, const void *got, const void *want,
		  uint32_t nstripes, uint32_t ncells, uint32_t nch,
		  uint64_t stripe_stride, uint64_t cell_stride,
		  uint32_t first_cell, uint32_t *masks, void *stream)
{
	const int cl = ecg_csum_len(type);
	const char *kernel = NULL;
	int rc, e;

	if (cl != 2 && cl != 4 && cl != 8)
		return ecg_fail(-ECG_DER_INVAL, "csum_mask: hash type %d has no 2, 4 or 8 byte checksum", type);
	if ((uint64_t)first_cell + ncells > 32)
		return ecg_fail(-ECG_DER_INVAL, "csum_mask: first_cell %u + ncells %u > 32 mask bits", first_cell,
				ncells);
	if (masks == NULL || (uintptr_t)masks % 4u)
		return ecg_fail(-ECG_DER_INVAL, "csum_mask: masks must be 4-byte aligned device memory");
	if (ctx == NULL)
		return ecg_fail(-ECG_DER_INVAL, "csum_mask: NULL context");
	if (nstripes && ncells && nch && (got == NULL || want == NULL))
		return ecg_fail(-ECG_DER_INVAL, "csum_mask: NULL checksums");
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	if (nstripes == 0 || ncells == 0 || nch == 0)
		return 0;
	ecg_trace_push("ecg:csum_mask");
	e = ecg_k_launch_csum_mask(got, want, nstripes, ncells, nch, stripe_stride, cell_stride, first_cell,
				   (uint32_t)cl, masks, (void *)ecg_pick_stream(ctx, stream), &kernel);
	return ecg_launch_done(ctx, e, "csum_mask kernel launch", 1, kernel);
}

/* [a, a + alen) and [b, b + blen) share a byte */
static int ranges_overlap(const void *a, uint64_t alen, const void *b, uint64_t blen)
{
	return alen && blen && (uintptr_t)a < (uintptr_t)b + blen && (uintptr_t)b < (uintptr_t)a + alen;
}

/* The geometry of an ecg_csum_masked call once its arguments passed */
struct masked_geom {
	uint64_t rcs;		/* record chunk bytes */
	uint64_t bytes;		/* of one [S][k+p][nch] checksum array */
	uint32_t nch;
};

/* Argument checks of ecg_csum_masked for the array `csums` (`what` names it),
 * everything but the context; result == NULL is accepted with need_result = 0.
 * table: the checks of a cell-table call that come before its context check --
 * no stripes; what csums must not overlap is checked entry by entry later. */
static int masked_check(const char *fn, int type, uint64_t chunksize, uint64_t rec_size, int k, int p, uint64_t C,
			uint32_t S, int table, const void *stripes, int64_t stripe_stride, const uint32_t *masks,
			unsigned which, const void *csums, const char *what, const void *result, int need_result,
			unsigned flags, struct masked_geom *g)
{
	const int cl = ecg_csum_len(type);
	const uint64_t rcs = ecg_csum_record_chunksize(chunksize, rec_size);
	uint64_t nch, bytes;

	memset(g, 0, sizeof(*g));
	if (cl < 0)
		return ecg_fail(-ECG_DER_NOTSUPPORTED, "%s: hash type %d not supported", fn, type);
	if (k < 1 || k > ECG_RM_MAX_K || p < 1 || p > ECG_RM_MAX_P)
		return ecg_fail(-ECG_DER_INVAL, "%s: k=%d p=%d outside the limits k <= %d, p <= %d", fn, k, p,
				ECG_RM_MAX_K, ECG_RM_MAX_P);
	if (which < 1 || which > (ECG_CM_ERASED | ECG_CM_SURVIVORS))
		return ecg_fail(-ECG_DER_INVAL, "%s: which 0x%x is not ECG_CM_ERASED, ECG_CM_SURVIVORS or both", fn,
				which);
	if (flags & ~ECG_RM_SPARSE)
		return ecg_fail(-ECG_DER_INVAL, "%s: unknown flags 0x%x", fn, flags);
	if (rcs == 0)
		return ecg_fail(-ECG_DER_INVAL, "%s: chunksize and rec_size must not be 0", fn);
	if (C % rec_size)
		return ecg_fail(-ECG_DER_INVAL, "%s: cell_bytes %llu is not a multiple of rec_size %llu", fn,
				(unsigned long long)C, (unsigned long long)rec_size);
	if (masks == NULL || (uintptr_t)masks % 4u)
		return ecg_fail(-ECG_DER_INVAL, "%s: masks must be 4-byte aligned device memory", fn);
	if ((need_result && result == NULL) || (uintptr_t)result % 8u)
		return ecg_fail(-ECG_DER_INVAL, "%s: result must be 8-byte aligned device memory", fn);
	nch = C / rcs + (C % rcs != 0);
	if (nch > UINT32_MAX || __builtin_mul_overflow(nch * (uint64_t)(k + p), (uint64_t)cl * S, &bytes))
		return ecg_fail(-ECG_DER_INVAL, "%s: too many checksums", fn);
	g->rcs = rcs;
	g->bytes = bytes;
	g->nch = (uint32_t)nch;
	if (table) {
		if (S && C && csums == NULL)
			return ecg_fail(-ECG_DER_INVAL, "%s: NULL %s", fn, what);
		return 0;
	}
	if (S && C && (stripes == NULL || csums == NULL))
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL stripes or %s", fn, what);
	if (S && C && ecg_cells_overlap(csums, bytes, stripes, S, stripe_stride, k + p, (int64_t)C, C))
		return ecg_fail(-ECG_DER_INVAL, "%s: %s overlaps the stripes", fn, what);
	if (C && ranges_overlap(csums, bytes, masks, 4ull * S))
		return ecg_fail(-ECG_DER_INVAL, "%s: %s overlaps the masks", fn, what);
	return 0;
}

/* One ecg_csum_masked launch on st; result NULL = nothing counted.  Over the
 * strided image `stripes`, or with cells_dev over a staged cell table (bytewise:
 * an entry, C or the chunk size is no multiple of 16). */
static int masked_launch(ecg_ctx_t *ctx, int type, const void *tbl, const struct masked_geom *g, int k, int p,
			 uint64_t C, uint32_t S, const void *stripes, int64_t stripe_stride, const uint64_t *cells_dev,
			 int bytewise, const uint32_t *masks, unsigned which, void *csums, void *result, hipStream_t st)
{
	ecg_csum_masked_params_t prm;
	const char *kernel = NULL;
	int e;

	memset(&prm, 0, sizeof(prm));
	HASH_FILL(&prm, type, tbl);
	prm.src = stripes;
	prm.out = csums;
	prm.masks = masks;
	prm.result = result;
	prm.cells_dev = cells_dev;
	prm.bytewise = (uint32_t)bytewise;
	prm.stripe_stride = stripe_stride;
	prm.cell_bytes = C;
	prm.chunk_bytes = g->rcs;
	prm.nstripes = S;
	prm.nch = g->nch;
	prm.k = (uint32_t)k;
	prm.p = (uint32_t)p;
	prm.which = which;
	prm.slots = (which & ECG_CM_ERASED ? (uint32_t)p : 0) + (which & ECG_CM_SURVIVORS ? (uint32_t)k : 0);
	prm.type = (uint32_t)type;
	ecg_trace_push(cells_dev ? "ecg:csum_masked_ptrs" : "ecg:csum_masked");
	e = ecg_k_launch_csum_masked(&prm, (void *)st, ctx->csum_blocks, &kernel);
	return ecg_launch_done(ctx, e, cells_dev ? "csum_masked_ptrs kernel launch" : "csum_masked kernel launch", 1,
			       kernel);
}

/* ECG_RM_SPARSE is accepted and ignored: the one grid serves dense and clean
 * batches alike (a clean stripe's items are one mask load each). */
int ecg_csum_masked(ecg_ctx_t *ctx, int type, uint64_t chunksize, uint64_t rec_size, int k, int p,
		    uint64_t C, uint32_t S, const void *stripes, int64_t stripe_stride, const uint32_t *masks,
		    unsigned which, void *csums, void *result, unsigned flags, void *stream)
{
	struct masked_geom g;
	const void *tbl;
	hipStream_t st;
	int rc;

	rc = masked_check("csum_masked", type, chunksize, rec_size, k, p, C, S, 0, stripes, stripe_stride, masks, which,
			  csums, "csums", result, 1, flags, &g);
	if (rc)
		return rc;
	if (ctx == NULL)
		return ecg_fail(-ECG_DER_INVAL, "csum_masked: NULL context");
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);
	/* result = {0, UINT64_MAX, 0, 0}, as ecg_recover_masks presets it */
	rc = ecg_result_reset(result, st, "csum_masked memset");
	if (rc)
		return rc;
	if (S == 0 || C == 0)
		return 0;
	rc = hash_tbl(ctx, type, &tbl);
	if (rc)
		return rc;
	return masked_launch(ctx, type, tbl, &g, k, p, C, S, stripes, stripe_stride, NULL, 0, masks, which, csums,
			     result, st);
}

/* What a composite (recovery, then the checksums of what it touched) makes of
 * its arguments */
struct composite {
	struct masked_geom g;
	int two;		/* src_csums is a second array: a SURVIVORS launch of its own */
	unsigned first;		/* `which` of the launch into csums: both kinds when src_csums is csums */
};

/* Both halves' argument errors, but the NULL context, before anything is
 * queued: ecg_recover_masks_check, then masked_check for csums and for a second
 * src_csums.  table: a cell-table call (no stripes: the cells are checked entry
 * by entry when the table is opened). */
static int composite_check(const char *fn, int table, int k, int p, uint64_t C, uint32_t S, const void *stripes,
			   int64_t stripe_stride, const uint32_t *masks, const void *result, unsigned flags, int type,
			   uint64_t chunksize, uint64_t rec_size, const void *csums, const void *src_csums,
			   struct composite *c)
{
	int rc;

	c->two = src_csums != NULL && src_csums != csums;
	c->first = src_csums != NULL && !c->two ? ECG_CM_ERASED | ECG_CM_SURVIVORS : ECG_CM_ERASED;
	rc = ecg_recover_masks_check(fn, 1, k, p, table ? 0 : C, S, stripes, stripe_stride, masks, result, flags);
	if (rc == 0)
		rc = masked_check(fn, type, chunksize, rec_size, k, p, C, S, table, stripes, stripe_stride, masks, c->first,
				  csums, "csums", NULL, 0, flags, &c->g);
	if (rc == 0 && c->two)
		rc = masked_check(fn, type, chunksize, rec_size, k, p, C, S, table, stripes, stripe_stride, masks,
				  ECG_CM_SURVIVORS, src_csums, "src_csums", NULL, 0, flags, &c->g);
	if (rc == 0 && c->two && S && C && ranges_overlap(csums, c->g.bytes, src_csums, c->g.bytes))
		rc = ecg_fail(-ECG_DER_INVAL, "%s: src_csums must be csums itself or not overlap it", fn);
	return rc;
}

int ecg_recover_masks_csum(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S, void *stripes,
			   int64_t stripe_stride, const uint32_t *masks, void *result, unsigned flags, int type,
			   uint64_t chunksize, uint64_t rec_size, void *csums, void *src_csums, void *stream)
{
	struct composite c;
	const void *tbl;
	hipStream_t st;
	int rc;

	rc = composite_check("recover_masks_csum", 0, k, p, C, S, stripes, stripe_stride, masks, result, flags, type,
			     chunksize, rec_size, csums, src_csums, &c);
	if (rc)
		return rc;
	if (ctx == NULL)
		return ecg_fail(-ECG_DER_INVAL, "recover_masks_csum: NULL context");
	rc = ecg_recover_masks(ctx, k, p, C, S, stripes, stripe_stride, masks, result, flags, stream);
	if (rc || S == 0 || C == 0)
		return rc;
	rc = hash_tbl(ctx, type, &tbl);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);
	rc = masked_launch(ctx, type, tbl, &c.g, k, p, C, S, stripes, stripe_stride, NULL, 0, masks, c.first, csums, NULL,
			   st);
	if (rc == 0 && c.two)
		rc = masked_launch(ctx, type, tbl, &c.g, k, p, C, S, stripes, stripe_stride, NULL, 0, masks,
				   ECG_CM_SURVIVORS, src_csums, NULL, st);
	return rc;
}

/*
 * The cell-table forms.  Each stages the caller's table through the one path
 * ecg_recover_masks_ptrs takes (ecg_recover_masks.c, ecg_internal.h): its
 * argument checks, ecg_staged_open, its own overlap checks and affine test,
 * ecg_staged_upload, the launches, ecg_staged_close.  Whatever takes ctx->lock
 * itself (the CRC tables, the set table) is fetched before the open.
 */

/* the byte-granular body for the whole launch: an entry, C or the chunk size
 * (rcs; 0 for the recovery) is no multiple of 16 */
static int table_bytewise(const struct ecg_staged *t, uint64_t C, uint64_t rcs)
{
	return (t->bits | C | rcs) % 16u != 0;
}

int ecg_csum_masked_ptrs(ecg_ctx_t *ctx, int type, uint64_t chunksize, uint64_t rec_size, int k, int p, uint64_t C,
			 uint32_t S, void *const *cells, const uint32_t *masks, unsigned which, void *csums,
			 void *result, unsigned flags, void *stream)
{
	static const char fn[] = "csum_masked_ptrs";
	const uint32_t n = (uint32_t)(k + p);
	struct ecg_staged t;
	struct masked_geom g;
	const void *tbl;
	hipStream_t st;
	int rc;

	rc = masked_check(fn, type, chunksize, rec_size, k, p, C, S, 1, NULL, 0, masks, which, csums, "csums", result, 1,
			  flags, &g);
	if (rc)
		return rc;
	if (ctx == NULL)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL context", fn);
	if (S && C && cells == NULL)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL cells", fn);
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);
	if (S == 0 || C == 0)	/* result = {0, UINT64_MAX, 0, 0} and nothing else */
		return ecg_result_reset(result, st, "csum_masked_ptrs memset");
	rc = hash_tbl(ctx, type, &tbl);
	if (rc == 0) {
		const struct ecg_clear clear[3] = {
			{csums, g.bytes, "csums"}, {masks, 4ull * S, "masks"}, {result, 32, "result"}};

		rc = ecg_staged_open(ctx, fn, cells, S, n, C, clear, 3, &t);
	}
	if (rc)
		return rc;
	if (ranges_overlap(csums, g.bytes, masks, 4ull * S))
		return ecg_staged_close(ctx, &t, st, ecg_fail(-ECG_DER_INVAL, "%s: csums overlaps the masks", fn));
	/* ecg_csum_masked's own layout, and csums clear of the whole image as it
	 * demands: its launch, with no table */
	if (t.affine && !ecg_cells_overlap(csums, g.bytes, cells[0], S, t.stride, n, (int64_t)C, C)) {
		ecg_staged_close(ctx, &t, st, 0);
		return ecg_csum_masked(ctx, type, chunksize, rec_size, k, p, C, S, cells[0], t.stride, masks, which, csums,
				       result, flags, stream);
	}
	rc = ecg_staged_upload(&t, result, st, "csum_masked_ptrs memset", "csum_masked_ptrs cell table");
	if (rc == 0)
		rc = masked_launch(ctx, type, tbl, &g, k, p, C, S, NULL, 0, t.sc->dev, table_bytewise(&t, C, g.rcs), masks,
				   which, csums, result, st);
	return ecg_staged_close(ctx, &t, st, rc);
}

int ecg_csum_cells_ptrs(ecg_ctx_t *ctx, int type, uint64_t chunksize, uint64_t rec_size, uint64_t C, uint64_t ncells,
			void *const *cells, void *csums, void *stream)
{
	static const char fn[] = "csum_cells_ptrs";
	const int cl = ecg_csum_len(type);
	const uint64_t rcs = ecg_csum_record_chunksize(chunksize, rec_size);
	ecg_csum_masked_params_t prm;
	struct ecg_staged t;
	const void *tbl;
	uint64_t nch, bytes;
	const char *kernel = NULL;
	hipStream_t st;
	int rc, e;

	if (cl < 0)
		return ecg_fail(-ECG_DER_NOTSUPPORTED, "%s: hash type %d not supported", fn, type);
	if (rcs == 0)
		return ecg_fail(-ECG_DER_INVAL, "%s: chunksize and rec_size must not be 0", fn);
	if (C % rec_size)
		return ecg_fail(-ECG_DER_INVAL, "%s: cell_bytes %llu is not a multiple of rec_size %llu", fn,
				(unsigned long long)C, (unsigned long long)rec_size);
	nch = C / rcs + (C % rcs != 0);
	if (nch > UINT32_MAX || __builtin_mul_overflow(nch * (uint64_t)cl, ncells, &bytes) ||
	    ncells > SIZE_MAX / sizeof(uint64_t))
		return ecg_fail(-ECG_DER_INVAL, "%s: too many checksums", fn);
	if (ctx == NULL)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL context", fn);
	if (ncells && C && (cells == NULL || csums == NULL))
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL cells or csums", fn);
	rc = ecg_ctx_enter(ctx);
	if (rc || ncells == 0 || C == 0)
		return rc;
	st = ecg_pick_stream(ctx, stream);
	rc = hash_tbl(ctx, type, &tbl);
	if (rc == 0) {
		const struct ecg_clear clear = {csums, bytes, "csums"};

		/* a table of ncells rows of one cell; no affine route: ecg_csum_extents
		 * wants csums aligned and picks its kernels by shape */
		rc = ecg_staged_open(ctx, fn, cells, ncells, 1, C, &clear, 1, &t);
	}
	if (rc)
		return rc;
	rc = ecg_staged_upload(&t, NULL, st, NULL, "csum_cells_ptrs cell table");
	if (rc)
		return ecg_staged_close(ctx, &t, st, rc);
	memset(&prm, 0, sizeof(prm));
	HASH_FILL(&prm, type, tbl);
	prm.out = csums;
	prm.cells_dev = t.sc->dev;
	prm.bytewise = (uint32_t)table_bytewise(&t, C, rcs);
	prm.cell_bytes = C;
	prm.chunk_bytes = rcs;
	prm.ncells = ncells;
	prm.nch = (uint32_t)nch;
	prm.type = (uint32_t)type;
	ecg_trace_push("ecg:csum_cells_ptrs");
	e = ecg_k_launch_csum_cells(&prm, (void *)st, ctx->csum_blocks, &kernel);
	rc = ecg_launch_done(ctx, e, "csum_cells_ptrs kernel launch", 1, kernel);
	rc = ecg_staged_close(ctx, &t, st, rc);
	if (rc == 0)
		ECG_STAT_ADD(ctx, csum_chunks, ncells * nch);
	return rc;
}

int ecg_recover_masks_ptrs_csum(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S, void *const *cells,
				const uint32_t *masks, void *result, unsigned flags, int type, uint64_t chunksize,
				uint64_t rec_size, void *csums, void *src_csums, void *stream)
{
	static const char fn[] = "recover_masks_ptrs_csum";
	const uint32_t n = (uint32_t)(k + p);
	const void *settbl = NULL, *tbl;
	struct ecg_staged t;
	struct composite c;
	hipStream_t st;
	int rc;

	rc = composite_check(fn, 1, k, p, C, S, NULL, 0, masks, result, flags, type, chunksize, rec_size, csums, src_csums,
			     &c);
	if (rc)
		return rc;
	if (ctx == NULL)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL context", fn);
	if (S && C && cells == NULL)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL cells", fn);
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);
	if (S == 0 || C == 0)	/* nothing recovered, nothing left */
		return ecg_result_reset(result, st, "recover_masks_ptrs_csum memset");
	rc = ecg_rm_settbl(ctx, k, p, &settbl);
	if (rc == 0)
		rc = hash_tbl(ctx, type, &tbl);
	if (rc == 0) {
		/* the table is checked and staged once for the two or three launches */
		const struct ecg_clear clear[4] = {{masks, 4ull * S, "masks"}, {result, 32, "result"},
						   {csums, c.g.bytes, "csums"},
						   {src_csums, c.two ? c.g.bytes : 0, "src_csums"}};

		rc = ecg_staged_open(ctx, fn, cells, S, n, C, clear, 4, &t);
	}
	if (rc)
		return rc;
	if (ranges_overlap(csums, c.g.bytes, masks, 4ull * S))
		return ecg_staged_close(ctx, &t, st, ecg_fail(-ECG_DER_INVAL, "%s: csums overlaps the masks", fn));
	if (c.two && ranges_overlap(src_csums, c.g.bytes, masks, 4ull * S))
		return ecg_staged_close(ctx, &t, st, ecg_fail(-ECG_DER_INVAL, "%s: src_csums overlaps the masks", fn));
	/* the layout of ecg_recover_masks_csum, and masks and the checksum arrays
	 * clear of the whole image as it demands: that call, with no table */
	if (t.affine && !ecg_cells_overlap(masks, 4ull * S, cells[0], S, t.stride, n, (int64_t)C, C) &&
	    !ecg_cells_overlap(csums, c.g.bytes, cells[0], S, t.stride, n, (int64_t)C, C) &&
	    !(c.two && ecg_cells_overlap(src_csums, c.g.bytes, cells[0], S, t.stride, n, (int64_t)C, C))) {
		ecg_staged_close(ctx, &t, st, 0);
		return ecg_recover_masks_csum(ctx, k, p, C, S, cells[0], t.stride, masks, result, flags, type, chunksize,
					      rec_size, csums, src_csums, stream);
	}
	rc = ecg_staged_upload(&t, result, st, "recover_masks_ptrs_csum memset", "recover_masks_ptrs_csum cell table");
	if (rc == 0)
		rc = ecg_rm_launch(ctx, fn, settbl, k, p, C, S, NULL, 0, t.sc->dev, table_bytewise(&t, C, 0), masks, result,
				   flags, st);
	if (rc == 0)
		rc = masked_launch(ctx, type, tbl, &c.g, k, p, C, S, NULL, 0, t.sc->dev, table_bytewise(&t, C, c.g.rcs),
				   masks, c.first, csums, NULL, st);
	if (rc == 0 && c.two)
		rc = masked_launch(ctx, type, tbl, &c.g, k, p, C, S, NULL, 0, t.sc->dev, table_bytewise(&t, C, c.g.rcs),
				   masks, ECG_CM_SURVIVORS, src_csums, NULL, st);
	/* the fetch and every kernel above read the slot */
	return ecg_staged_close(ctx, &t, st, rc);
}

/*
 * ecg_csum_updated and its kin: the checksums of the parity cells a masked
 * update rewrote, the step after ecg_update_masks / ecg_update_masks_ptrs
 * (ecg_update_masks.c), whose mask reading, parity addressing, table and
 * three-group test these calls share.
 */

/* The geometry of an ecg_csum_updated call once its arguments passed */
struct updated_geom {
	uint64_t rcs;		/* record chunk bytes */
	uint64_t span;		/* bytes from csums to the end of the farthest slot */
	uint32_t nch;
};

/* Do the S x p ranges of nch checksums at index s*ss + r*cs lie apart?  The two
 * orderings that can be proven: rows inside a stripe's range, or stripes inside
 * a row's.  A stride whose count is 1 is not looked at. */
static int updated_strides_ok(uint64_t nch, int p, uint32_t S, uint64_t ss, uint64_t cs)
{
	const int rows = p > 1, stripes = S > 1;
	uint64_t in;
	int a, b;

	a = (!rows || cs >= nch) &&
	    (!stripes || (!__builtin_mul_overflow(rows ? cs : 0, (uint64_t)(p - 1), &in) &&
			  !__builtin_add_overflow(in, nch, &in) && ss >= in));
	b = (!stripes || ss >= nch) &&
	    (!rows || (!__builtin_mul_overflow(stripes ? ss : 0, (uint64_t)(S - 1), &in) &&
		       !__builtin_add_overflow(in, nch, &in) && cs >= in));
	return a || b;
}

/* Argument checks of ecg_csum_updated in their documented order, everything but
 * the context; result == NULL is accepted with need_result = 0 (a composite's
 * checksum launch counts nothing, and passes its update half's result so that
 * csums is held clear of it).  table: the checks of a cell-table call that come
 * before its context check -- no parity; what csums must not overlap there is
 * checked entry by entry later. */
static int updated_check(const char *fn, int type, uint64_t chunksize, uint64_t rec_size, int k, int p, uint64_t C,
			 uint32_t S, int table, const void *parity, int64_t parity_cell_stride,
			 int64_t parity_stripe_stride, const uint32_t *masks, const void *csums, uint64_t css, uint64_t ccs,
			 const void *result, int need_result, unsigned flags, struct updated_geom *g)
{
	const int cl = ecg_csum_len(type);
	const uint64_t rcs = ecg_csum_record_chunksize(chunksize, rec_size);
	uint64_t nch, n, a, b;

	memset(g, 0, sizeof(*g));
	if (cl < 0)
		return ecg_fail(-ECG_DER_NOTSUPPORTED, "%s: hash type %d not supported", fn, type);
	if (k < 1 || k > ECG_KMAX_K || p < 1 || p > ECG_KMAX_R)
		return ecg_fail(-ECG_DER_INVAL, "%s: k=%d p=%d outside the limits k <= %d, p <= %d", fn, k, p,
				ECG_KMAX_K, ECG_KMAX_R);
	if (flags & ECG_UM_PACKED)
		return ecg_fail(-ECG_DER_INVAL, "%s: ECG_UM_PACKED has no meaning here (it packs the data images, "
				"not the parity)", fn);
	if (flags & ~ECG_RM_SPARSE)
		return ecg_fail(-ECG_DER_INVAL, "%s: unknown flags 0x%x", fn, flags);
	if (rcs == 0)
		return ecg_fail(-ECG_DER_INVAL, "%s: chunksize and rec_size must not be 0", fn);
	if (C % rec_size)
		return ecg_fail(-ECG_DER_INVAL, "%s: cell_bytes %llu is not a multiple of rec_size %llu", fn,
				(unsigned long long)C, (unsigned long long)rec_size);
	nch = C / rcs + (C % rcs != 0);
	/* the kernel's item count S * p * nch and every slot's byte offset fit 64 bits */
	if (nch > UINT32_MAX || __builtin_mul_overflow(nch * (uint64_t)p, (uint64_t)cl * S, &n))
		return ecg_fail(-ECG_DER_INVAL, "%s: too many checksums", fn);
	if (S && C) {
		if (__builtin_mul_overflow(S > 1 ? css : 0, (uint64_t)(S - 1), &a) ||
		    __builtin_mul_overflow(p > 1 ? ccs : 0, (uint64_t)(p - 1), &b) || __builtin_add_overflow(a, b, &a) ||
		    __builtin_add_overflow(a, nch, &a) || __builtin_mul_overflow(a, (uint64_t)cl, &g->span))
			return ecg_fail(-ECG_DER_INVAL, "%s: too many checksums", fn);
		if (!updated_strides_ok(nch, p, S, css, ccs))
			return ecg_fail(-ECG_DER_INVAL, "%s: csum strides %llu (stripe) and %llu (cell) do not keep "
					"the %u x %d ranges of %llu checksums apart", fn, (unsigned long long)css,
					(unsigned long long)ccs, S, p, (unsigned long long)nch);
	}
	g->rcs = rcs;
	g->nch = (uint32_t)nch;
	if (masks == NULL || (uintptr_t)masks % 4u)
		return ecg_fail(-ECG_DER_INVAL, "%s: masks must be 4-byte aligned device memory", fn);
	if ((need_result && result == NULL) || (uintptr_t)result % 8u)
		return ecg_fail(-ECG_DER_INVAL, "%s: result must be 8-byte aligned device memory", fn);
	if (S == 0 || C == 0)
		return 0;
	if (!table && parity == NULL)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL parity", fn);
	if (csums == NULL)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL csums", fn);
	/* the span ecg_update_masks holds its masks and result clear of */
	if (!table &&
	    ecg_cells_overlap(csums, g->span, parity, S, parity_stripe_stride, p, parity_cell_stride, C))
		return ecg_fail(-ECG_DER_INVAL, "%s: csums overlaps the parity", fn);
	if (ranges_overlap(csums, g->span, masks, 4ull * S))
		return ecg_fail(-ECG_DER_INVAL, "%s: csums overlaps the masks", fn);
	if (result != NULL && ranges_overlap(csums, g->span, result, 32))
		return ecg_fail(-ECG_DER_INVAL, "%s: csums overlaps the result", fn);
	return 0;
}

/* The table checks of the two cell-table calls, made on the caller's table before
 * the context is used (ecg_staged_open then only copies it): no NULL table, no
 * NULL entry, and no `clear` range inside a cell from column `from` of a row on
 * -- 2k: the parity cells, all that ecg_csum_updated_ptrs reads; 0: every cell.
 * The message names the entry. */
static int updated_table_check(const char *fn, void *const *cells, int k, int p, uint64_t C, uint32_t S,
			       uint32_t from, const struct ecg_clear *clear, int nclear)
{
	const uint32_t n = (uint32_t)(2 * k + p);

	if (S == 0 || C == 0)
		return 0;
	if (cells == NULL)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL cells", fn);
	for (uint64_t s = 0; s < S; s++)
		for (uint32_t c = 0; c < n; c++) {
			const size_t i = (size_t)(s * n + c);

			if (cells[i] == NULL)
				return ecg_fail(-ECG_DER_INVAL, "%s: NULL cell %zu", fn, i);
			for (int r = 0; c >= from && r < nclear; r++)
				if (ranges_overlap(clear[r].at, clear[r].len, cells[i], C))
					return ecg_fail(-ECG_DER_INVAL, "%s: %s overlaps cell %zu", fn, clear[r].what, i);
		}
	return 0;
}

/* One ecg_csum_updated launch on st; result NULL = nothing counted.  Over the
 * strided parity, or with cells_dev over a staged update table (bytewise: a
 * parity entry, C or the chunk size is no multiple of 16). */
static int updated_launch(ecg_ctx_t *ctx, int type, const void *tbl, const struct updated_geom *g, int k, int p,
			  uint64_t C, uint32_t S, const void *parity, int64_t parity_cell_stride,
			  int64_t parity_stripe_stride, const uint64_t *cells_dev, int bytewise, const uint32_t *masks,
			  void *csums, uint64_t css, uint64_t ccs, void *result, hipStream_t st)
{
	ecg_csum_updated_params_t prm;
	const char *kernel = NULL;
	int e;

	memset(&prm, 0, sizeof(prm));
	HASH_FILL(&prm, type, tbl);
	prm.src = parity;
	prm.out = csums;
	prm.masks = masks;
	prm.result = result;
	prm.cells_dev = cells_dev;
	prm.bytewise = (uint32_t)bytewise;
	prm.cell_stride = parity_cell_stride;
	prm.stripe_stride = parity_stripe_stride;
	prm.csum_stripe_stride = css;
	prm.csum_cell_stride = ccs;
	prm.cell_bytes = C;
	prm.chunk_bytes = g->rcs;
	prm.nstripes = S;
	prm.nch = g->nch;
	prm.k = (uint32_t)k;
	prm.p = (uint32_t)p;
	prm.type = (uint32_t)type;
	ecg_trace_push(cells_dev ? "ecg:csum_updated_ptrs" : "ecg:csum_updated");
	e = ecg_k_launch_csum_updated(&prm, (void *)st, ctx->csum_blocks, &kernel);
	return ecg_launch_done(ctx, e, cells_dev ? "csum_updated_ptrs kernel launch" : "csum_updated kernel launch", 1,
			       kernel);
}

/* ECG_RM_SPARSE is accepted and ignored, as in ecg_csum_masked: the one grid
 * serves dense and clean batches alike. */
int ecg_csum_updated(ecg_ctx_t *ctx, int type, uint64_t chunksize, uint64_t rec_size, int k, int p, uint64_t C,
		     uint32_t S, const void *parity, int64_t parity_cell_stride, int64_t parity_stripe_stride,
		     const uint32_t *masks, void *csums, uint64_t css, uint64_t ccs, void *result, unsigned flags,
		     void *stream)
{
	struct updated_geom g;
	const void *tbl;
	hipStream_t st;
	int rc;

	rc = updated_check("csum_updated", type, chunksize, rec_size, k, p, C, S, 0, parity, parity_cell_stride,
			   parity_stripe_stride, masks, csums, css, ccs, result, 1, flags, &g);
	if (rc)
		return rc;
	if (ctx == NULL)
		return ecg_fail(-ECG_DER_INVAL, "csum_updated: NULL context");
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);
	/* result = {0, UINT64_MAX, 0, 0}, as ecg_update_masks presets it */
	rc = ecg_result_reset(result, st, "csum_updated memset");
	if (rc || S == 0 || C == 0)
		return rc;
	rc = hash_tbl(ctx, type, &tbl);
	if (rc)
		return rc;
	return updated_launch(ctx, type, tbl, &g, k, p, C, S, parity, parity_cell_stride, parity_stripe_stride, NULL, 0,
			      masks, csums, css, ccs, result, st);
}

int ecg_csum_updated_ptrs(ecg_ctx_t *ctx, int type, uint64_t chunksize, uint64_t rec_size, int k, int p, uint64_t C,
			  uint32_t S, void *const *cells, const uint32_t *masks, void *csums, uint64_t css,
			  uint64_t ccs, void *result, unsigned flags, void *stream)
{
	static const char fn[] = "csum_updated_ptrs";
	struct ecg_staged t;
	struct updated_geom g;
	const void *tbl;
	int64_t pc, ps;
	uint64_t bits;
	hipStream_t st;
	int rc;

	rc = updated_check(fn, type, chunksize, rec_size, k, p, C, S, 1, NULL, 0, 0, masks, csums, css, ccs, result, 1,
			   flags, &g);
	if (rc == 0) {
		/* held clear of the parity cells only: the old and new data cells
		 * are not read */
		const struct ecg_clear clear[3] = {
			{csums, g.span, "csums"}, {masks, 4ull * S, "masks"}, {result, 32, "result"}};

		rc = updated_table_check(fn, cells, k, p, C, S, 2u * (uint32_t)k, clear, 3);
	}
	if (rc)
		return rc;
	if (ctx == NULL)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL context", fn);
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);
	if (S == 0 || C == 0)	/* result = {0, UINT64_MAX, 0, 0} and nothing else */
		return ecg_result_reset(result, st, "csum_updated_ptrs memset");
	rc = hash_tbl(ctx, type, &tbl);
	if (rc == 0)
		rc = ecg_staged_open(ctx, fn, cells, S, (uint32_t)(2 * k + p), C, NULL, 0, &t);
	if (rc)
		return rc;
	/* ecg_csum_updated's own layout, and csums clear of the whole parity span
	 * as it demands: its launch, with no table */
	if (ecg_um_parity_group(t.sc->pin, k, p, C, S, &pc, &ps, &bits) &&
	    !ecg_cells_overlap(csums, g.span, cells[2 * k], S, ps, p, pc, C)) {
		ecg_staged_close(ctx, &t, st, 0);
		return ecg_csum_updated(ctx, type, chunksize, rec_size, k, p, C, S, cells[2 * k], pc, ps, masks, csums,
					css, ccs, result, flags, stream);
	}
	rc = ecg_staged_upload(&t, result, st, "csum_updated_ptrs memset", "csum_updated_ptrs cell table");
	if (rc == 0)
		rc = updated_launch(ctx, type, tbl, &g, k, p, C, S, NULL, 0, 0, t.sc->dev, (bits | C | g.rcs) % 16u != 0,
				    masks, csums, css, ccs, result, st);
	return ecg_staged_close(ctx, &t, st, rc);
}

/* Both halves' argument errors, but the NULL context, before anything is queued:
 * the update's (ecg_um_check), then updated_check.  ECG_UM_PACKED concerns the
 * update half alone. */
int ecg_update_masks_csum(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S, const void *old_cells,
			  const void *new_cells, int64_t upd_stripe_stride, void *parity, int64_t parity_cell_stride,
			  int64_t parity_stripe_stride, const uint32_t *masks, void *result, unsigned flags, int type,
			  uint64_t chunksize, uint64_t rec_size, void *csums, uint64_t css, uint64_t ccs, void *stream)
{
	static const char fn[] = "update_masks_csum";
	struct updated_geom g;
	const void *tbl;
	int rc;

	rc = ecg_um_check(fn, 1, 1, k, p, C, S, old_cells, new_cells, parity, parity_cell_stride, parity_stripe_stride,
			  NULL, masks, result, flags, NULL);
	if (rc == 0)
		rc = updated_check(fn, type, chunksize, rec_size, k, p, C, S, 0, parity, parity_cell_stride,
				   parity_stripe_stride, masks, csums, css, ccs, result, 0, flags & ~ECG_UM_PACKED, &g);
	/* csums clear of every old and new cell the update half may read (packed
	 * or not, they lie within k cells of a stripe's start) */
	if (rc == 0 && S && C && ecg_cells_overlap(csums, g.span, old_cells, S, upd_stripe_stride, k, (int64_t)C, C))
		rc = ecg_fail(-ECG_DER_INVAL, "%s: csums overlaps the old cells", fn);
	if (rc == 0 && S && C && ecg_cells_overlap(csums, g.span, new_cells, S, upd_stripe_stride, k, (int64_t)C, C))
		rc = ecg_fail(-ECG_DER_INVAL, "%s: csums overlaps the new cells", fn);
	if (rc)
		return rc;
	if (ctx == NULL)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL context", fn);
	rc = ecg_update_masks(ctx, k, p, C, S, old_cells, new_cells, upd_stripe_stride, parity, parity_cell_stride,
			      parity_stripe_stride, masks, result, flags, stream);
	if (rc || S == 0 || C == 0)
		return rc;
	rc = hash_tbl(ctx, type, &tbl);
	if (rc)
		return rc;
	return updated_launch(ctx, type, tbl, &g, k, p, C, S, parity, parity_cell_stride, parity_stripe_stride, NULL, 0,
			      masks, csums, css, ccs, NULL, ecg_pick_stream(ctx, stream));
}

int ecg_update_masks_ptrs_csum(ecg_ctx_t *ctx, int k, int p, uint64_t C, uint32_t S, void *const *cells,
			       const uint32_t *masks, void *result, unsigned flags, int type, uint64_t chunksize,
			       uint64_t rec_size, void *csums, uint64_t css, uint64_t ccs, void *stream)
{
	static const char fn[] = "update_masks_ptrs_csum";
	struct ecg_staged t;
	struct updated_geom g;
	const void *tbl;
	int64_t us, pc, ps;
	uint64_t bits;
	hipStream_t st;
	int rc;

	/* (no stripes, so no table yet: updated_table_check looks at it once both
	 * halves' other arguments passed) */
	rc = ecg_um_check(fn, 0, 1, k, p, C, 0, NULL, NULL, NULL, 0, 0, NULL, masks, result, flags, NULL);
	if (rc == 0)
		rc = updated_check(fn, type, chunksize, rec_size, k, p, C, S, 1, NULL, 0, 0, masks, csums, css, ccs, result,
				   0, flags, &g);
	if (rc == 0) {
		/* csums clear of every cell the update half may read, too */
		const struct ecg_clear clear[3] = {
			{masks, 4ull * S, "masks"}, {result, 32, "result"}, {csums, g.span, "csums"}};

		rc = updated_table_check(fn, cells, k, p, C, S, 0, clear, 3);
	}
	if (rc)
		return rc;
	if (ctx == NULL)
		return ecg_fail(-ECG_DER_INVAL, "%s: NULL context", fn);
	rc = ecg_ctx_enter(ctx);
	if (rc)
		return rc;
	st = ecg_pick_stream(ctx, stream);
	if (S == 0 || C == 0)	/* nothing updated, nothing checksummed */
		return ecg_result_reset(result, st, "update_masks_ptrs_csum memset");
	rc = hash_tbl(ctx, type, &tbl);
	/* the table was checked above and is staged once for the two launches */
	if (rc == 0)
		rc = ecg_staged_open(ctx, fn, cells, S, (uint32_t)(2 * k + p), C, NULL, 0, &t);
	if (rc)
		return rc;
	/* the layout of ecg_update_masks_csum, and masks, result and csums clear of
	 * the spans it demands: that call, with no table */
	if (ecg_um_three_groups(t.sc->pin, k, p, C, S, &us, &pc, &ps) &&
	    !ecg_cells_overlap(masks, 4ull * S, cells[2 * k], S, ps, p, pc, C) &&
	    !ecg_cells_overlap(result, 32, cells[2 * k], S, ps, p, pc, C) &&
	    !ecg_cells_overlap(csums, g.span, cells[2 * k], S, ps, p, pc, C) &&
	    !ecg_cells_overlap(csums, g.span, cells[0], S, us, k, (int64_t)C, C) &&
	    !ecg_cells_overlap(csums, g.span, cells[k], S, us, k, (int64_t)C, C)) {
		ecg_staged_close(ctx, &t, st, 0);
		return ecg_update_masks_csum(ctx, k, p, C, S, cells[0], cells[k], us, cells[2 * k], pc, ps, masks, result,
					     flags, type, chunksize, rec_size, csums, css, ccs, stream);
	}
	(void)ecg_um_parity_group(t.sc->pin, k, p, C, S, &pc, &ps, &bits);
	rc = ecg_staged_upload(&t, result, st, "update_masks_ptrs_csum memset", "update_masks_ptrs_csum cell table");
	if (rc == 0)
		rc = ecg_um_launch(ctx, fn, k, p, C, S, NULL, NULL, 0, NULL, 0, 0, t.sc->dev, (t.bits | C) % 16u != 0, masks,
				   result, flags, st);
	if (rc == 0)
		rc = updated_launch(ctx, type, tbl, &g, k, p, C, S, NULL, 0, 0, t.sc->dev, (bits | C | g.rcs) % 16u != 0,
				    masks, csums, css, ccs, NULL, st);
	/* the fetch and both kernels read the slot */
	return ecg_staged_close(ctx, &t, st, rc);
}

/* Fused product + checksum parameters (ecg_kabi.h) for output cells of C
 * bytes that start on chunk boundaries.  Returns 1 when the fused kernels
 * can take the request, 0 when the caller must run the product and
 * ecg_csum_extents separately, < 0 on error.  src: for the SRC instantiations
 * (their own default columns per item). */
int ecg_csum_fused_params(ecg_ctx_t *ctx, int type, uint64_t chunksize, uint64_t rec_size,
			  uint64_t C, int k, int rows, void *csums, int src, ecg_mmcs_params_t *q)
{
	const uint64_t rcs = ecg_csum_record_chunksize(chunksize, rec_size);
	const struct crc_def *d;
	uint64_t last, m;
	int rc;

	memset(q, 0, sizeof(*q));
	if (type != ECG_HASH_CRC16 && type != ECG_HASH_CRC32 && type != ECG_HASH_CRC64)
		return 0;
	if (rcs == 0 || rcs % ECG_MMCS_STRIDE || C % 16 || C % rec_size)
		return 0;
	/* the kernel XORs partials in with 32-bit (crc16/crc32) or 64-bit atomics */
	if ((uintptr_t)csums % (type == ECG_HASH_CRC64 ? 8u : 4u))
		return 0;
	d = &g_defs[type];
	rc = crc_tables(ctx, type, &q->tbl);
	if (rc)
		return rc;
	q->out = csums;
	q->chunk_bytes = rcs;
	q->nch = (uint32_t)((C + rcs - 1) / rcs);
	q->init = d->init;
	q->xorout = d->xorout;
	q->poly = d->poly;
	q->type = (uint32_t)type;
	last = C - (uint64_t)(q->nch - 1) * rcs;
	m = rcs / ECG_MMCS_STRIDE;
	q->m = (uint32_t)m;
	q->m_last = (uint32_t)((last + ECG_MMCS_STRIDE - 1) / ECG_MMCS_STRIDE);
	q->ncols = fused_cols(ctx, m, type, k, rows, src);
	/* bound the multiplier table (nh + nh_last rows of 256 entries) for
	 * very long chunks: at most 2048 items per chunk */
	if ((m + q->ncols - 1) / q->ncols > 2048)
		q->ncols = (uint32_t)((m + 2047) / 2048);
	q->nh = (uint32_t)((m + q->ncols - 1) / q->ncols);
	q->nh_last = (q->m_last + q->ncols - 1) / q->ncols;
	if ((uint64_t)(q->nch - 1) * q->nh + q->nh_last > UINT32_MAX)
		return 0;
	q->nitems = (q->nch - 1) * q->nh + q->nh_last;
	/* the workgroup kernel for every shape: since its item tail no longer
	 * reads HBM (round 3) it beats the wave-per-chunk kernel of rounds 1-2
	 * for crc64 at EC_4P2 too (+13 % vs +19 % over the plain encode,
	 * profiles/r03/fused_tail/); the wave kernel was retired in round 4 */
	rc = fused_kh(ctx, type, rcs, last, q->ncols, q->nh, q->nh_last, &q->kh);
	if (rc)
		return rc;
	return 1;
}
