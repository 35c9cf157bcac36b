// ecg_csum_kernels.hip -- chunked checksums of device-resident cells for gfx950.
//
// DAOS checksums every chunk of an extent it writes, including the parity
// cells rebuild regenerates (ref:src/object/srv_obj_migrate.c:1156) and the
// cells recovery rebuilds; the csummer hashes each chunk from a reset state
// (ref:src/common/checksum.c:467-497) with one of crc16 / crc32 / crc64 /
// adler32 (ref:src/common/multihash_isal.c:27-256).  This file computes the
// same values on the device, one wavefront per chunk, so regenerated cells
// never leave HBM to be checksummed.
//
// CRC scheme (W-bit register, NB = W/8 bytes):
//  * lane l takes the 16-byte pieces q = 64*i + l - z of its chunk: every
//    load instruction of the wave reads 1 KiB contiguous (coalesced);
//  * z zero pieces are prepended so every lane has the same piece count m;
//    leading zeros do not change a zero-initialised CRC;
//  * per piece: acc = shift_1KiB(acc) ^ crc(piece)  -- Horner over the
//    lane's pieces, the shift being a byte-wise linear map (NB lookups) and
//    crc(piece) slice-by-NB with the register folded in (16 lookups);
//  * lane l's sum is then multiplied by x^(8*16*(63-l)) mod P (GF(2)
//    polynomial multiply, W steps) and the wave XOR-reduces: the chunk's
//    raw CRC of its 16-byte-aligned part; lane 0 finishes the <16 B tail
//    byte by byte;
//  * a non-zero initial register (crc64: ~0) is XORed into the first NB
//    bytes of the chunk, the standard identity for reflected CRCs.
// Tables live in LDS (crc16 4 KiB, crc32 8 KiB, crc64 32 KiB per block) and
// blocks stride over chunks so each block loads them once.
//
// Each kernel family is built from one body.  The wave-per-item kernels of
// extents, of masked cells and of cell tables are crc_wave / adler_wave over an
// addressing struct (cs_extents, cs_masked<PTRS>, cs_updated<PTRS>, cs_cells); the
// group and split kernels keep their own
// loops and take the CRC prologue and finish (crc_lane) and the adler32 sums
// (adler_lane, adler_wave_sum, adler_finish) from the same helpers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../ecg_kabi.h"
#include "ecg_crc_dev.h"

namespace {

using namespace ecg_crc;

constexpr int CS_BLOCK = 256;
constexpr int CS_WAVES = CS_BLOCK / 64;
constexpr uint32_t ADLER_MOD = 65521;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <bool ALIGNED>
__device__ __forceinline__ void load16(const uint8_t *p, uint32_t d[4])
{
	if constexpr (ALIGNED) {
		const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(p));
		d[0] = v.x;
		d[1] = v.y;
		d[2] = v.z;
		d[3] = v.w;
	} else {
#pragma unroll
		for (int j = 0; j < 4; j++)
			d[j] = (uint32_t)p[4 * j] | ((uint32_t)p[4 * j + 1] << 8) |
			       ((uint32_t)p[4 * j + 2] << 16) | ((uint32_t)p[4 * j + 3] << 24);
	}
}

// CRC table kinds (ecg_kabi.h): TK_5 conflict-free 5-bit fields (the
// byte-granular kernels), TK_4 nibble fields addressed by SDWA byte selects
// (the aligned kernels: fewest VALU per lookup, and the CRC kernels are
// VALU-issue bound -- profiles/r03/crc_sq)
constexpr int TK_5 = 0, TK_4 = 2;

// One Horner step of a lane's accumulator over the ECG_CSUM_P5U pieces d (s5 =
// positional q then a): acc * x^(8 * P5U * stride) ^ crc(pieces)
template <int W, int TK, typename T>
__device__ __forceinline__ T horner(T acc, const uint32_t (*d)[4], const T *s5)
{
	if constexpr (TK == TK_4)
		return horner4u<W, ECG_CSUM_P5U>(acc, d, s5, nib_hmask<T>());
	else
		return horner5u<W>(acc, d, s5);
}

// LDS image of one kernel: the positional 5-bit or nibble tables (q, a); UN
// pieces in flight per lane
template <int W, int TK>
struct crc_lds {
	using T = typename reg<W>::T;
	static constexpr int N5 = TK == TK_4 ? f4u<W>::N : f5u<W>::N;
	static constexpr int UN = ECG_CSUM_P5U;
};

// positional tables of stride `q_off` (5-bit p5x / nibble q4) and the
// U-stride shift into LDS
template <int W, int TK, typename T>
__device__ __forceinline__ void stage_tables(T *s5, const T *gt, int p5x_off, int a5_off, int q4_off, int a4_off,
					     int nthreads)
{
	if constexpr (TK == TK_4)
		stage4u<W, ECG_CSUM_P5U>(s5, gt, q4_off, a4_off, nthreads);
	else
		stage5u<W>(s5, gt, p5x_off, a5_off, nthreads);
}

// What a lane of a CRC kernel keeps beside its tables in LDS, and the two ends
// of every chunk.  stage(): the kernel's prologue up to (not including) its
// barrier -- the positional tables of the stride at the four offsets and r4
// into LDS, the lane's constants into registers; kidx is the lane's column of
// k64 / nibl: x^(8*16*(63-kidx)) is its final shift.
template <int W, bool REFL, int TK>
struct crc_lane {
	using T = typename reg<W>::T;
	static constexpr int NB = W / 8;
	const T *gt, *r4;
	uint32_t kidx;
	T klane, poly, init, xorout;

	template <class P>
	__device__ __forceinline__ void stage(const P &p, T *s5, T *r4_, int p5x_off, int a5_off, int q4_off,
					      int a4_off, int nthreads, uint32_t kidx_)
	{
		gt = (const T *)p.tbl;
		r4 = r4_;
		kidx = kidx_;
		stage_tables<W, TK>(s5, gt, p5x_off, a5_off, q4_off, a4_off, nthreads);
		if (REFL && threadIdx.x < 16)
			r4_[threadIdx.x] = gt[ECG_CSUM_OFF_R4(NB) + threadIdx.x];
		klane = REFL ? (T)0 : gt[ECG_CSUM_OFF_K64(NB) + kidx];
		poly = (T)p.poly;
		init = (T)p.init;
		xorout = (T)p.xorout;
	}

	// the lane's final shift: reflected CRCs from the nibl tables (W/4
	// steps), else mulmod
	__device__ __forceinline__ T shift(T acc) const
	{
		if constexpr (REFL)
			return lane_mul_nib<W>(acc, gt + ECG_CSUM_OFF_NIBL(NB), r4, kidx);
		else
			return mulmod<W, REFL>(klane, acc, poly);
	}

	// the checksum of a chunk whose nq whole pieces reduced to acc: the
	// initial register when there was none, then the tail bytes (sl[0] in
	// memory) and the final XOR
	__device__ __forceinline__ T finish(T acc, int64_t nq, const uint8_t *base, uint64_t len) const
	{
		T crc = nq == 0 ? init : acc;

		for (uint64_t b = (uint64_t)nq * 16; b < len; b++)
			crc = byte_step<W, REFL>(crc, base[b], gt);
		return crc ^ xorout;
	}
};

// lane steps of a chunk of nq pieces, `per` pieces per step: a multiple of
// the ECG_CSUM_P5U pieces a Horner step takes
__device__ __forceinline__ int64_t lane_steps(int64_t nq, int64_t per)
{
	const int64_t m = (nq + per - 1) / per;
	return (m + ECG_CSUM_P5U - 1) / ECG_CSUM_P5U * ECG_CSUM_P5U;
}

// the U pieces of lane step i (pieces (i+u)*64 + lane - z): `first` masks
// the zero prefix (q < 0) and folds the initial register into piece 0; later
// steps are unconditional (q > 0 for i >= ECG_CSUM_P5U since z < 64 U)
template <int UN, int W, bool ALIGNED, bool FIRST, typename T>
__device__ __forceinline__ void load_step(const uint8_t *base, int64_t i, int64_t stride_pieces, int64_t lane_q0,
					  int64_t m, T init, uint32_t (*d)[4])
{
#pragma unroll
	for (int u = 0; u < UN; u++) {
		const int64_t q = (i + u) * stride_pieces + lane_q0;
		if constexpr (FIRST) {
			if (i + u < m && q >= 0) {
				load16<ALIGNED>(base + 16 * q, d[u]);
				if (q == 0) {	// fold the initial register into the first bytes
					d[u][0] ^= (uint32_t)init;
					if constexpr (W == 64)
						d[u][1] ^= (uint32_t)((uint64_t)init >> 32);
				}
			} else {
				d[u][0] = d[u][1] = d[u][2] = d[u][3] = 0;
			}
		} else {
			load16<ALIGNED>(base + 16 * q, d[u]);
		}
	}
}

__device__ __forceinline__ void chunk_geom(const ecg_csum_params_t &p, uint64_t g, uint64_t &len,
					   const uint8_t *&base)
{
	const uint64_t e = g / p.nchunks, c = g - e * p.nchunks;
	const uint64_t off = c == 0 ? 0 : p.first_bytes + (c - 1) * p.chunk_bytes;

	len = c == 0 ? p.first_bytes : p.chunk_bytes;
	if (off + len > p.ext_bytes)
		len = p.ext_bytes - off;
	base = p.src + (int64_t)e * p.ext_stride + off;
}

// chunk g's geometry with a 32-bit division when the counts allow (the
// 64-bit one expands to ~100 VALU per chunk)
__device__ __forceinline__ void chunk_geom_fast(const ecg_csum_params_t &p, uint64_t g, uint64_t &len,
						const uint8_t *&base)
{
	if (((g | p.nchunks) >> 32) == 0) {
		const uint32_t e = (uint32_t)g / p.nchunks, c = (uint32_t)g - e * p.nchunks;
		const uint64_t off = c == 0 ? 0 : p.first_bytes + (uint64_t)(c - 1) * p.chunk_bytes;

		len = c == 0 ? p.first_bytes : p.chunk_bytes;
		if (off + len > p.ext_bytes)
			len = p.ext_bytes - off;
		base = p.src + (int64_t)e * p.ext_stride + off;
	} else {
		chunk_geom(p, g, len, base);
	}
}

// ---------------------------------------------------------------------------
// Where the work items of a kernel lie and where their checksums go -- all the
// extent and the masked kernels differ in.  Over the kernel's parameters p:
// total(p): the items; item(p, g, base, len, slot): the bytes of item g and the
// slot of its checksum, false when the item is skipped; store<LEN>(p, slot, v):
// the checksum of LEN bytes; wave(): the wave's index in its block, in a scalar
// register where the kernel wants its items' geometry on the scalar unit.
// ---------------------------------------------------------------------------

// The chunks of n_ext extents, item g = chunk g % nchunks of extent g / nchunks
// (FAST, the CRC kernels: chunk_geom_fast on a scalar g; the adler32 kernels
// keep the 64-bit division on the vector unit); the checksums are an array of
// aligned LEN-byte words indexed by g.
template <bool FAST>
struct cs_extents {
	using params = ecg_csum_params_t;

	static __device__ __forceinline__ uint64_t total(const params &p) { return (uint64_t)p.n_ext * p.nchunks; }
	static __device__ __forceinline__ uint32_t wave()
	{
		if constexpr (FAST)
			return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
		else
			return threadIdx.x >> 6;
	}
	static __device__ __forceinline__ bool item(const params &p, uint64_t g, const uint8_t *&base, uint64_t &len,
						    uint64_t &slot)
	{
		if constexpr (FAST)
			chunk_geom_fast(p, g, len, base);
		else
			chunk_geom(p, g, len, base);
		slot = g;
		return true;
	}
	template <int LEN, typename T>
	static __device__ __forceinline__ void store(const params &p, uint64_t slot, T v)
	{
		if constexpr (LEN == 2)
			((uint16_t *)p.out)[slot] = (uint16_t)v;
		else
			((T *)p.out)[slot] = v;
	}
};

// A checksum of LEN bytes, little-endian, at byte `at` of an array that may lie
// at any byte; a crc16 slot is two bytes wide, so its neighbours may belong to
// cells that are not selected.
template <int LEN, typename T>
__device__ __forceinline__ void store_at(uint8_t *at, T v)
{
	if (((uintptr_t)at & (LEN - 1)) == 0) {
		if constexpr (LEN == 2)
			*(uint16_t *)at = (uint16_t)v;
		else
			*(T *)at = v;
	} else {
#pragma unroll
		for (int b = 0; b < LEN; b++)
			at[b] = (uint8_t)(v >> (8 * b));
	}
}

// Entry i of a cell table, i wave-uniform: the table is read only for the launch
// (an earlier launch on the stream wrote it), so the load may go through the
// constant address space, where a uniform index makes it one scalar load.
__device__ __forceinline__ const uint8_t *table_cell(const uint64_t *tab, uint64_t i)
{
	return (const uint8_t *)(uintptr_t)((const __attribute__((address_space(4))) uint64_t *)tab)[i];
}

// ecg_csum_masked: the checksums of the cells each stripe's mask word selects
// (ecg_kabi.h ecg_csum_masked_sel), a wave per (stripe, selected cell, chunk).
// Item g = (s * slots + r) * nch + c reads masks[s] (wave-uniform), takes the
// r-th set bit of sel as its cell and is skipped when sel has no r-th bit, so a
// clean stripe costs its items one load each; the item (s, 0, 0) counts its
// stripe into result.  Every address derives from sel, which is 0 unless
// ecg_erasure_set_read reads the word as a set and has no bit at or above
// k + p: all 2^32 mask values are safe.
// PTRS (ecg_csum_masked_ptrs): the cell's address is the entry s * (k + p) +
// cell of the table p.cells_dev -- one wave-uniform 8-byte load per item, after
// the sel test, so a skipped item reads no entry and a stripe whose mask is no
// set reads none at all.
template <bool PTRS>
struct cs_masked {
	using params = ecg_csum_masked_params_t;

	static __device__ __forceinline__ uint64_t total(const params &p)
	{
		return (uint64_t)p.nstripes * p.slots * p.nch;
	}
	static __device__ __forceinline__ uint32_t wave() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
	static __device__ __forceinline__ bool item(const params &p, uint64_t g, const uint8_t *&base, uint64_t &len,
						    uint64_t &slot)
	{
		const uint64_t per = (uint64_t)p.slots * p.nch;
		uint64_t s;
		uint32_t r, c;

		if (((g | per) >> 32) == 0) {	// as chunk_geom_fast: 32-bit divisions when the counts allow
			const uint32_t s32 = (uint32_t)g / (uint32_t)per, rem = (uint32_t)g - s32 * (uint32_t)per;

			s = s32;
			r = rem / p.nch;
			c = rem - r * p.nch;
		} else {
			const uint64_t rem = g % per;

			s = g / per;
			r = (uint32_t)(rem / p.nch);
			c = (uint32_t)(rem - (uint64_t)r * p.nch);
		}
		const uint32_t m = p.masks[s];
		int valid;
		uint32_t sel = ecg_csum_masked_sel(m, (int)p.k, (int)p.p, p.which, &valid);

		if (r == 0 && c == 0 && m != 0 && p.result != nullptr && (threadIdx.x & 63) == 0) {
			unsigned long long *res = (unsigned long long *)p.result;

			if (valid) {
				atomicAdd(&res[0], 1ull);
				atomicAdd(&res[2], (unsigned long long)__builtin_popcount(sel));
			} else {
				atomicMin(&res[1], (unsigned long long)s);
				atomicAdd(&res[3], 1ull);
			}
		}
		if (r >= (uint32_t)__builtin_popcount(sel))
			return false;
		for (uint32_t i = 0; i < r; i++)
			sel &= sel - 1u;
		const uint32_t cell = (uint32_t)__builtin_ctz(sel);	// < k + p
		const uint64_t off = (uint64_t)c * p.chunk_bytes;	// < cell_bytes: c < nch

		len = p.cell_bytes - off < p.chunk_bytes ? p.cell_bytes - off : p.chunk_bytes;
		if constexpr (PTRS)
			// (cell comes from a vector load of masks[s]: uniform, but the
			// compiler cannot know)
			base = table_cell(p.cells_dev, s * (p.k + p.p) + __builtin_amdgcn_readfirstlane(cell)) + off;
		else
			base = p.src + (int64_t)s * p.stripe_stride + (uint64_t)cell * p.cell_bytes + off;
		slot = (s * (p.k + p.p) + cell) * p.nch + c;
		return true;
	}
	template <int LEN, typename T>
	static __device__ __forceinline__ void store(const params &p, uint64_t slot, T v)
	{
		store_at<LEN>(p.out + slot * LEN, v);
	}
};

// ecg_csum_updated: the checksums of the parity cells ecg_update_masks rewrote
// (ecg_kabi.h ecg_csum_updated_params_t), a wave per (stripe, parity row, chunk).
// Item g = (s * p + r) * nch + c reads masks[s] (wave-uniform) and is skipped
// unless ecg_update_mask_read reads the word as 1 .. k cells -- the one reading
// the update kernels make of it -- so a clean stripe costs its items one load
// each; the item (s, 0, 0) counts its stripe into result.  No address derives
// from the mask's bits, only from s, r < p and c < nch: all 2^32 mask values are
// safe.
// PTRS (ecg_csum_updated_ptrs): the cell's address is the entry s * (2k + p) +
// 2k + r of the table p.cells_dev -- one wave-uniform 8-byte load per item, after
// the mask test, so a skipped item reads no entry and no item ever reads an old
// or a new data entry.
template <bool PTRS>
struct cs_updated {
	using params = ecg_csum_updated_params_t;

	static __device__ __forceinline__ uint64_t total(const params &p)
	{
		return (uint64_t)p.nstripes * p.p * p.nch;
	}
	static __device__ __forceinline__ uint32_t wave() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
	static __device__ __forceinline__ bool item(const params &p, uint64_t g, const uint8_t *&base, uint64_t &len,
						    uint64_t &slot)
	{
		const uint64_t per = (uint64_t)p.p * p.nch;
		uint64_t s;
		uint32_t r, c;

		if (((g | per) >> 32) == 0) {	// as chunk_geom_fast: 32-bit divisions when the counts allow
			const uint32_t s32 = (uint32_t)g / (uint32_t)per, rem = (uint32_t)g - s32 * (uint32_t)per;

			s = s32;
			r = rem / p.nch;
			c = rem - r * p.nch;
		} else {
			const uint64_t rem = g % per;

			s = g / per;
			r = (uint32_t)(rem / p.nch);
			c = (uint32_t)(rem - (uint64_t)r * p.nch);
		}
		const uint32_t m = p.masks[s];
		const int rd = ecg_update_mask_read(m, (int)p.k);

		if (r == 0 && c == 0 && m != 0 && p.result != nullptr && (threadIdx.x & 63) == 0) {
			unsigned long long *res = (unsigned long long *)p.result;

			if (rd > 0) {
				atomicAdd(&res[0], 1ull);
				atomicAdd(&res[2], (unsigned long long)p.p);
			} else {
				atomicMin(&res[1], (unsigned long long)s);
				atomicAdd(&res[3], 1ull);
			}
		}
		if (rd <= 0)
			return false;
		const uint64_t off = (uint64_t)c * p.chunk_bytes;	// < cell_bytes: c < nch

		len = p.cell_bytes - off < p.chunk_bytes ? p.cell_bytes - off : p.chunk_bytes;
		if constexpr (PTRS)
			// (r comes from a scalar g: uniform, and said so for the scalar load)
			base = table_cell(p.cells_dev,
					  s * (2 * p.k + p.p) + __builtin_amdgcn_readfirstlane(2 * p.k + r)) + off;
		else
			base = p.src + (int64_t)s * p.stripe_stride + (int64_t)r * p.cell_stride + off;
		slot = s * p.csum_stripe_stride + r * p.csum_cell_stride + c;
		return true;
	}
	template <int LEN, typename T>
	static __device__ __forceinline__ void store(const params &p, uint64_t slot, T v)
	{
		store_at<LEN>(p.out + slot * LEN, v);
	}
};

// ecg_csum_cells_ptrs: every chunk of every cell of a table, item g = chunk
// g % nch of the cell at cells_dev[g / nch] (a wave-uniform load); the checksums
// are an array indexed by g that may lie at any byte.
struct cs_cells {
	using params = ecg_csum_masked_params_t;

	static __device__ __forceinline__ uint64_t total(const params &p) { return p.ncells * p.nch; }
	static __device__ __forceinline__ uint32_t wave() { return __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); }
	static __device__ __forceinline__ bool item(const params &p, uint64_t g, const uint8_t *&base, uint64_t &len,
						    uint64_t &slot)
	{
		uint64_t i;
		uint32_t c;

		if ((g >> 32) == 0) {	// as chunk_geom_fast
			const uint32_t i32 = (uint32_t)g / p.nch;

			i = i32;
			c = (uint32_t)g - i32 * p.nch;
		} else {
			i = g / p.nch;
			c = (uint32_t)(g - i * p.nch);
		}
		const uint64_t off = (uint64_t)c * p.chunk_bytes;	// < cell_bytes: c < nch

		len = p.cell_bytes - off < p.chunk_bytes ? p.cell_bytes - off : p.chunk_bytes;
		base = table_cell(p.cells_dev, i) + off;
		slot = g;
		return true;
	}
	template <int LEN, typename T>
	static __device__ __forceinline__ void store(const params &p, uint64_t slot, T v)
	{
		store_at<LEN>(p.out + slot * LEN, v);
	}
};

// A wave per item (the scheme at the top of the file), blocks striding over
// the items of Addr.
template <int W, bool REFL, bool ALIGNED, int TK, class Addr>
__device__ __forceinline__ void crc_wave(const typename Addr::params &p)
{
	using T = typename reg<W>::T;
	using L = crc_lds<W, TK>;
	constexpr int NB = W / 8;
	__shared__ T s5[L::N5];
	__shared__ T r4[REFL ? 16 : 1];
	const int lane = threadIdx.x & 63;
	crc_lane<W, REFL, TK> cl;

	cl.stage(p, s5, r4, ECG_CSUM_OFF_P5X_1K(NB), ECG_CSUM_OFF_A5_4K(NB), ECG_CSUM_OFF_Q4_1K(NB),
		 ECG_CSUM_OFF_A4_4K(NB), CS_BLOCK, (uint32_t)lane);
	__syncthreads();

	const uint64_t total = Addr::total(p);
	const uint32_t wv = Addr::wave();
	for (uint64_t g = (uint64_t)blockIdx.x * CS_WAVES + wv; g < total; g += (uint64_t)gridDim.x * CS_WAVES) {
		uint64_t len, slot;
		const uint8_t *base;

		if (!Addr::item(p, g, base, len, slot))
			continue;
		const int64_t nq = (int64_t)(len / 16);
		const int64_t m = lane_steps(nq, 64);
		const int64_t z = m * 64 - nq;
		T acc = 0;

		if (m > 0) {
			uint32_t d[L::UN][4];

			load_step<L::UN, W, ALIGNED, true>(base, 0, 64, lane - z, m, cl.init, d);
			acc = horner<W, TK>(acc, d, s5);
			for (int64_t i = L::UN; i < m; i += L::UN) {
				load_step<L::UN, W, ALIGNED, false>(base, i, 64, lane - z, m, cl.init, d);
				acc = horner<W, TK>(acc, d, s5);
			}
		}
		acc = cl.shift(acc);
		acc = wave_xor_uniform(acc);	// DPP, no ds_bpermute
		if (lane == 0)
			Addr::template store<NB>(p, slot, cl.finish(acc, nq, base, len));
	}
}

template <int W, bool REFL, bool ALIGNED, int TK>
__global__ __launch_bounds__(CS_BLOCK) void ecg_crc_kernel(ecg_csum_params_t p)
{
	crc_wave<W, REFL, ALIGNED, TK, cs_extents<true>>(p);
}

template <int W, bool REFL, bool ALIGNED, int TK>
__global__ __launch_bounds__(CS_BLOCK) void ecg_crc_masked_kernel(ecg_csum_masked_params_t p)
{
	crc_wave<W, REFL, ALIGNED, TK, cs_masked<false>>(p);
}

template <int W, bool REFL, bool ALIGNED, int TK>
__global__ __launch_bounds__(CS_BLOCK) void ecg_crc_masked_ptr_kernel(ecg_csum_masked_params_t p)
{
	crc_wave<W, REFL, ALIGNED, TK, cs_masked<true>>(p);
}

template <int W, bool REFL, bool ALIGNED, int TK>
__global__ __launch_bounds__(CS_BLOCK) void ecg_crc_updated_kernel(ecg_csum_updated_params_t p)
{
	crc_wave<W, REFL, ALIGNED, TK, cs_updated<false>>(p);
}

template <int W, bool REFL, bool ALIGNED, int TK>
__global__ __launch_bounds__(CS_BLOCK) void ecg_crc_updated_ptr_kernel(ecg_csum_updated_params_t p)
{
	crc_wave<W, REFL, ALIGNED, TK, cs_updated<true>>(p);
}

template <int W, bool REFL, bool ALIGNED, int TK>
__global__ __launch_bounds__(CS_BLOCK) void ecg_crc_cells_ptr_kernel(ecg_csum_masked_params_t p)
{
	crc_wave<W, REFL, ALIGNED, TK, cs_cells>(p);
}

template <typename T>
__device__ __forceinline__ T shfl_xor_t(T v, int s)
{
	if constexpr (sizeof(T) == 8)
		return ((uint64_t)(uint32_t)__shfl_xor((uint32_t)(v >> 32), s) << 32) |
		       (uint32_t)__shfl_xor((uint32_t)v, s);
	else
		return (T)__shfl_xor((uint32_t)v, s);
}

// Short chunks (<= 8 KiB): with a wave per chunk each lane holds only 1-8
// pieces and the per-lane final multiply (W GF(2) steps) dominates.  Here a
// group of G = ECG_CSUM_GLANES lanes takes a chunk (4 chunks per wave): lane
// l of the group takes pieces q = G*i + l - z, so each load instruction still
// reads 4 x 256 B contiguous, Horner-steps by G*16 bytes (the 256 B stride's
// tables), and the group reduces with shuffles after multiplying by
// x^(8*16*(G-1-l)) = k64[64 - G + l].  Otherwise as crc_wave.
template <int W, bool REFL, int TK>
__global__ __launch_bounds__(CS_BLOCK) void ecg_crc_group_kernel(ecg_csum_params_t p)
{
	using T = typename reg<W>::T;
	using L = crc_lds<W, TK>;
	constexpr int NB = W / 8;
	constexpr int G = ECG_CSUM_GLANES;
	constexpr int GPW = 64 / G;		// chunks per wave
	__shared__ T s5[L::N5];
	__shared__ T r4[REFL ? 16 : 1];
	const int lane = threadIdx.x & 63, gl = lane % G;
	using Addr = cs_extents<true>;
	crc_lane<W, REFL, TK> cl;

	cl.stage(p, s5, r4, ECG_CSUM_OFF_P5X_256(NB), ECG_CSUM_OFF_A5_1K(NB), ECG_CSUM_OFF_Q4_256(NB),
		 ECG_CSUM_OFF_A4_1K(NB), CS_BLOCK, (uint32_t)(64 - G + gl));
	__syncthreads();

	const uint64_t total = Addr::total(p);
	const uint64_t waves = (uint64_t)gridDim.x * CS_WAVES;
	// every lane runs the same number of outer iterations (shuffles below
	// need the whole wave): the wave's first chunk decides, idle groups mask
	for (uint64_t g0 = ((uint64_t)blockIdx.x * CS_WAVES + (threadIdx.x >> 6)) * GPW; g0 < total;
	     g0 += waves * GPW) {
		const uint64_t g = g0 + lane / G;
		const bool live = g < total;
		uint64_t len = 0, slot = g;
		const uint8_t *base = p.src;

		if (live)
			Addr::item(p, g, base, len, slot);
		const int64_t nq = (int64_t)(len / 16);
		const int64_t m = lane_steps(nq, G);
		const int64_t z = m * G - nq;
		T acc = 0;

		for (int64_t i = 0; i < m; i += L::UN) {
			uint32_t d[L::UN][4];

			load_step<L::UN, W, true, true>(base, i, G, gl - z, m, cl.init, d);
			acc = horner<W, TK>(acc, d, s5);
		}
		acc = cl.shift(acc);
#pragma unroll
		for (int s = G / 2; s >= 1; s >>= 1)
			acc ^= shfl_xor_t(acc, s);
		if (live && gl == 0)
			Addr::template store<NB>(p, slot, cl.finish(acc, nq, base, len));
	}
}

// Long chunks, few of them (e.g. 1024 chunks of 1 MiB = one wave per SIMD
// with ecg_crc_kernel): one workgroup of NW waves per chunk.  The chunk's
// 1 KiB steps are cut into NW contiguous slices; each wave computes the raw
// CRC of its slice exactly as ecg_crc_kernel does a whole chunk, moves it to
// the end of the chunk's aligned part by multiplying with x^(8 * bytes after
// the slice) mod P -- that power is the product of the p2[j] = x^(8*2^j)
// table entries of its set bits, one bit per lane, multiplied down the wave
// in 6 butterfly steps -- and the waves' values are XORed through LDS (CRC
// is linear: crc(A || B) = crc(A) * x^(8|B|) ^ crc(B) for zero registers).
template <int W, bool REFL, int NW, int TK>
__global__ __launch_bounds__(64 * NW) void ecg_crc_split_kernel(ecg_csum_params_t p)
{
	using T = typename reg<W>::T;
	using L = crc_lds<W, TK>;
	constexpr int NB = W / 8;
	__shared__ T s5[L::N5];
	__shared__ T part[NW];
	__shared__ T r4[REFL ? 16 : 1];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	using Addr = cs_extents<true>;
	crc_lane<W, REFL, TK> cl;

	cl.stage(p, s5, r4, ECG_CSUM_OFF_P5X_1K(NB), ECG_CSUM_OFF_A5_4K(NB), ECG_CSUM_OFF_Q4_1K(NB),
		 ECG_CSUM_OFF_A4_4K(NB), 64 * NW, (uint32_t)lane);
	const T one = REFL ? (T)((T)1 << (W - 1)) : (T)1;
	const T p2 = lane < ECG_CSUM_NP2 ? cl.gt[ECG_CSUM_OFF_P2(NB) + lane] : one;
	__syncthreads();

	const uint64_t total = Addr::total(p);
	for (uint64_t g = blockIdx.x; g < total; g += gridDim.x) {
		uint64_t len, slot;
		const uint8_t *base;

		Addr::item(p, g, base, len, slot);
		static_assert(NW == ECG_CSUM_SPLIT_NW, "host split shifts assume ECG_CSUM_SPLIT_NW slices");
		const int64_t nq = (int64_t)(len / 16);
		const int64_t m = (int64_t)ECG_CSUM_STEPS((uint64_t)len);	// as the host's split_m
		const int64_t z = m * 64 - nq;
		const int64_t ms = (int64_t)ECG_CSUM_SPLIT_MS((uint64_t)m);
		const int64_t i0 = wv * ms < m ? wv * ms : m;
		const int64_t i1 = i0 + ms < m ? i0 + ms : m;
		T acc = 0;

		for (int64_t i = i0; i < i1; i += L::UN) {
			uint32_t d[L::UN][4];

			load_step<L::UN, W, true, true>(base, i, 64, lane - z, i1, cl.init, d);
			acc = horner<W, TK>(acc, d, s5);
		}
		acc = cl.shift(acc);
		acc = wave_xor_uniform(acc);	// DPP, no ds_bpermute
		// x^(8 * (m - i1) KiB): the host's constant for this chunk length,
		// else the product of p2[j] over the set bits j (one bit per lane)
		T f;
		if (m == (int64_t)p.split_m[0] || m == (int64_t)p.split_m[1] || m == (int64_t)p.split_m[2]) {
			const int c = m == (int64_t)p.split_m[0] ? 0 : m == (int64_t)p.split_m[1] ? 1 : 2;
			f = (T)p.split_sh[c][wv];
		} else {
			const uint64_t after = (uint64_t)(m - i1) * ECG_CSUM_STRIDE;
			f = lane < ECG_CSUM_NP2 && ((after >> lane) & 1) ? p2 : one;
#pragma unroll
			for (int s = 32; s >= 1; s >>= 1)
				f = mulmod<W, REFL>(f, shfl_xor_t(f, s), cl.poly);
		}
		acc = mulmod<W, REFL>(f, acc, cl.poly);
		if (lane == 0)
			part[wv] = acc;
		__syncthreads();
		if (threadIdx.x == 0) {
			T crc = 0;

#pragma unroll
			for (int w = 0; w < NW; w++)
				crc ^= part[w];
			Addr::template store<NB>(p, slot, cl.finish(crc, nq, base, len));
		}
		__syncthreads();
	}
}

// adler32 with A = B = 0 at each chunk start (isal_adler32(0, ...)): lanes sum
// bytes and position-weighted bytes of their pieces (v_dot4_u32_u8), the wave
// reduces, A = sum mod 65521, B = L*sum - sum(pos*byte) mod 65521.

// a lane's sums over the pieces q0, q0 + stride, ... below nq, each mod 65521
// (reduced every 256 pieces: a piece adds < 2^12 to s and < 2^16 * len to w)
template <bool ALIGNED>
__device__ __forceinline__ void adler_lane(const uint8_t *base, uint64_t nq, uint64_t q0, uint64_t stride,
					   uint64_t &s, uint64_t &w)
{
	s = 0;
	w = 0;
	for (uint64_t q = q0, it = 0; q < nq; q += stride, it++) {
		uint32_t d[4];
		uint32_t s16 = 0, w16 = 0;

		load16<ALIGNED>(base + 16 * q, d);
#pragma unroll
		for (int j = 0; j < 4; j++) {
			s16 = __builtin_amdgcn_udot4(d[j], 0x01010101u, s16, false);
			// weights 4j .. 4j+3 packed as bytes
			w16 = __builtin_amdgcn_udot4(d[j], 0x03020100u + 0x04040404u * j, w16, false);
		}
		s += s16;
		w += 16 * q * (uint64_t)s16 + w16;
		if ((it & 255) == 255) {
			s %= ADLER_MOD;
			w %= ADLER_MOD;
		}
	}
	s %= ADLER_MOD;
	w %= ADLER_MOD;
}

// wave sum (values < 2^17 each: 64 of them fit easily)
__device__ __forceinline__ void adler_wave_sum(uint64_t &s, uint64_t &w)
{
#pragma unroll
	for (int sft = 32; sft >= 1; sft >>= 1) {
		s += __shfl_xor(s, sft);
		w += __shfl_xor(w, sft);
	}
}

// the checksum of a chunk of len bytes whose nq whole pieces summed to (s, w):
// the tail bytes, then A and B packed
__device__ __forceinline__ uint32_t adler_finish(uint64_t s, uint64_t w, const uint8_t *base, uint64_t nq,
						 uint64_t len)
{
	for (uint64_t b = nq * 16; b < len; b++) {
		s += base[b];
		w += b * (uint64_t)base[b];
	}
	const uint64_t A = s % ADLER_MOD;
	const uint64_t Bp = ((len % ADLER_MOD) * A) % ADLER_MOD;
	const uint64_t B = (Bp + ADLER_MOD - w % ADLER_MOD) % ADLER_MOD;
	return (uint32_t)((B << 16) | A);
}

// A wave per item, as crc_wave.
template <bool ALIGNED, class Addr>
__device__ __forceinline__ void adler_wave(const typename Addr::params &p)
{
	const int lane = threadIdx.x & 63;
	const uint64_t total = Addr::total(p);
	const uint32_t wv = Addr::wave();

	for (uint64_t g = (uint64_t)blockIdx.x * CS_WAVES + wv; g < total; g += (uint64_t)gridDim.x * CS_WAVES) {
		uint64_t len, slot, s, w;
		const uint8_t *base;

		if (!Addr::item(p, g, base, len, slot))
			continue;
		const uint64_t nq = len / 16;

		adler_lane<ALIGNED>(base, nq, lane, 64, s, w);
		adler_wave_sum(s, w);
		if (lane == 0)
			Addr::template store<4>(p, slot, adler_finish(s, w, base, nq, len));
	}
}

template <bool ALIGNED>
__global__ __launch_bounds__(CS_BLOCK) void ecg_adler_kernel(ecg_csum_params_t p)
{
	adler_wave<ALIGNED, cs_extents<false>>(p);
}

template <bool ALIGNED>
__global__ __launch_bounds__(CS_BLOCK) void ecg_adler_masked_kernel(ecg_csum_masked_params_t p)
{
	adler_wave<ALIGNED, cs_masked<false>>(p);
}

template <bool ALIGNED>
__global__ __launch_bounds__(CS_BLOCK) void ecg_adler_masked_ptr_kernel(ecg_csum_masked_params_t p)
{
	adler_wave<ALIGNED, cs_masked<true>>(p);
}

template <bool ALIGNED>
__global__ __launch_bounds__(CS_BLOCK) void ecg_adler_updated_kernel(ecg_csum_updated_params_t p)
{
	adler_wave<ALIGNED, cs_updated<false>>(p);
}

template <bool ALIGNED>
__global__ __launch_bounds__(CS_BLOCK) void ecg_adler_updated_ptr_kernel(ecg_csum_updated_params_t p)
{
	adler_wave<ALIGNED, cs_updated<true>>(p);
}

template <bool ALIGNED>
__global__ __launch_bounds__(CS_BLOCK) void ecg_adler_cells_ptr_kernel(ecg_csum_masked_params_t p)
{
	adler_wave<ALIGNED, cs_cells>(p);
}

// adler32 of long chunks that are few (one wave per chunk would leave the
// CUs idle, e.g. 1024 chunks of 1 MiB): a workgroup of NW waves per chunk.
// The sums use absolute positions within the chunk, so the threads' partial
// sums simply add: thread t takes the 16-byte pieces t, t + 64*NW, ... (every
// load instruction of a wave still reads 1 KiB contiguous), the waves reduce
// with shuffles and combine through LDS.
template <int NW>
__global__ __launch_bounds__(64 * NW) void ecg_adler_split_kernel(ecg_csum_params_t p)
{
	__shared__ uint64_t ps[NW], pw[NW];
	const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
	using Addr = cs_extents<false>;
	const uint64_t total = Addr::total(p);

	for (uint64_t g = blockIdx.x; g < total; g += gridDim.x) {
		uint64_t len, slot, s, w;
		const uint8_t *base;

		Addr::item(p, g, base, len, slot);
		const uint64_t nq = len / 16;

		adler_lane<true>(base, nq, threadIdx.x, 64 * NW, s, w);
		// adler_wave_sum and, below, adler_finish written out: behind the
		// helpers this kernel is not the code it was (the finish keeps
		// thread 0's sums in vector registers, 2 more VGPRs)
#pragma unroll
		for (int sft = 32; sft >= 1; sft >>= 1) {
			s += __shfl_xor(s, sft);
			w += __shfl_xor(w, sft);
		}
		if (lane == 0) {
			ps[wv] = s;
			pw[wv] = w;
		}
		__syncthreads();
		if (threadIdx.x == 0) {
			s = 0;
			w = 0;
#pragma unroll
			for (int i = 0; i < NW; i++) {
				s += ps[i];
				w += pw[i];
			}
			for (uint64_t b = nq * 16; b < len; b++) {
				s += base[b];
				w += b * (uint64_t)base[b];
			}
			const uint64_t A = s % ADLER_MOD;
			const uint64_t Bp = ((len % ADLER_MOD) * A) % ADLER_MOD;
			const uint64_t B = (Bp + ADLER_MOD - w % ADLER_MOD) % ADLER_MOD;
			Addr::template store<4>(p, slot, (uint32_t)((B << 16) | A));
		}
		__syncthreads();
	}
}

// Compare n checksums of LEN bytes (ecg_csum_compare): grid-stride, each
// thread counts its mismatches and keeps the lowest index; threads that saw
// one add to result[0] and lower result[1] ({0, UINT64_MAX} on entry).  Byte
// loads: the arrays need no alignment, and n is small next to the cells.
template <int LEN>
__global__ void __launch_bounds__(CS_BLOCK)
ecg_csum_compare_kernel(const uint8_t *got, const uint8_t *want, uint64_t n, unsigned long long *result)
{
	unsigned long long cnt = 0, lo = ~0ull;

	for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
		uint32_t d = 0;

#pragma unroll
		for (int b = 0; b < LEN; b++)
			d |= (uint32_t)(got[i * LEN + b] ^ want[i * LEN + b]);
		if (d) {
			cnt++;
			if (i < lo)
				lo = i;
		}
	}
	if (cnt) {
		atomicAdd(&result[0], cnt);
		atomicMin(&result[1], lo);
	}
}

// Which cells' checksums differ, per stripe (ecg_csum_mask): a thread takes
// one (stripe, cell) and compares its nch checksums of LEN bytes; a cell with
// a mismatch sets its bit in the stripe's mask word.  Byte loads, as above.
template <int LEN>
__global__ void __launch_bounds__(CS_BLOCK)
ecg_csum_mask_kernel(const uint8_t *got, const uint8_t *want, uint32_t nstripes, uint32_t ncells, uint32_t nch,
		     uint64_t stripe_stride, uint64_t cell_stride, uint32_t first_cell, uint32_t *masks)
{
	const uint64_t n = (uint64_t)nstripes * ncells;

	for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (uint64_t)gridDim.x * blockDim.x) {
		const uint32_t s = (uint32_t)(t / ncells), i = (uint32_t)(t % ncells);
		const uint64_t at = ((uint64_t)s * stripe_stride + (uint64_t)i * cell_stride) * LEN;
		uint32_t d = 0;

		for (uint64_t b = 0; b < (uint64_t)nch * LEN; b++)
			d |= (uint32_t)(got[at + b] ^ want[at + b]);
		if (d)
			atomicOr(&masks[s], 1u << (first_cell + i));
	}
}

// One table per kernel family, a row per (hash type, 16-byte aligned or not);
// the launcher reports the row's name.  One table kind per
// kernel: the nibble tables for 16-byte aligned chunks, the 5-bit tables for
// the byte-granular kernels.
template <class P>
struct csum_entry {
	uint32_t type;
	bool aligned;
	void (*fn)(P);
	const char *name;
};

const csum_entry<ecg_csum_params_t> g_csum[] = {
	{1, true, ecg_crc_kernel<16, false, true, TK_4>, "ecg_crc_kernel<crc16>"},
	{1, false, ecg_crc_kernel<16, false, false, TK_5>, "ecg_crc_kernel<crc16,bytes>"},
	{2, true, ecg_crc_kernel<32, true, true, TK_4>, "ecg_crc_kernel<crc32>"},
	{2, false, ecg_crc_kernel<32, true, false, TK_5>, "ecg_crc_kernel<crc32,bytes>"},
	{3, true, ecg_crc_kernel<64, true, true, TK_4>, "ecg_crc_kernel<crc64>"},
	{3, false, ecg_crc_kernel<64, true, false, TK_5>, "ecg_crc_kernel<crc64,bytes>"},
	{7, true, ecg_adler_kernel<true>, "ecg_adler_kernel"},
	{7, false, ecg_adler_kernel<false>, "ecg_adler_kernel<bytes>"},
};

constexpr int SPLIT_NW = ECG_CSUM_SPLIT_NW;	// waves per chunk in the split kernel
const csum_entry<ecg_csum_params_t> g_split[] = {
	{1, true, ecg_crc_split_kernel<16, false, SPLIT_NW, TK_4>, "ecg_crc_split_kernel<crc16>"},
	{2, true, ecg_crc_split_kernel<32, true, SPLIT_NW, TK_4>, "ecg_crc_split_kernel<crc32>"},
	{3, true, ecg_crc_split_kernel<64, true, SPLIT_NW, TK_4>, "ecg_crc_split_kernel<crc64>"},
	{7, true, ecg_adler_split_kernel<SPLIT_NW>, "ecg_adler_split_kernel"},
};

const csum_entry<ecg_csum_params_t> g_group[] = {
	{1, true, ecg_crc_group_kernel<16, false, TK_4>, "ecg_crc_group_kernel<crc16>"},
	{2, true, ecg_crc_group_kernel<32, true, TK_4>, "ecg_crc_group_kernel<crc32>"},
	{3, true, ecg_crc_group_kernel<64, true, TK_4>, "ecg_crc_group_kernel<crc64>"},
};

const csum_entry<ecg_csum_masked_params_t> g_masked[] = {
	{1, true, ecg_crc_masked_kernel<16, false, true, TK_4>, "ecg_crc_masked_kernel<crc16>"},
	{1, false, ecg_crc_masked_kernel<16, false, false, TK_5>, "ecg_crc_masked_kernel<crc16,bytes>"},
	{2, true, ecg_crc_masked_kernel<32, true, true, TK_4>, "ecg_crc_masked_kernel<crc32>"},
	{2, false, ecg_crc_masked_kernel<32, true, false, TK_5>, "ecg_crc_masked_kernel<crc32,bytes>"},
	{3, true, ecg_crc_masked_kernel<64, true, true, TK_4>, "ecg_crc_masked_kernel<crc64>"},
	{3, false, ecg_crc_masked_kernel<64, true, false, TK_5>, "ecg_crc_masked_kernel<crc64,bytes>"},
	{7, true, ecg_adler_masked_kernel<true>, "ecg_adler_masked_kernel"},
	{7, false, ecg_adler_masked_kernel<false>, "ecg_adler_masked_kernel<bytes>"},
};

// the cell-table kernels of ecg_csum_masked_ptrs and ecg_csum_cells_ptrs
const csum_entry<ecg_csum_masked_params_t> g_masked_ptr[] = {
	{1, true, ecg_crc_masked_ptr_kernel<16, false, true, TK_4>, "ecg_crc_masked_ptr_kernel<crc16>"},
	{1, false, ecg_crc_masked_ptr_kernel<16, false, false, TK_5>, "ecg_crc_masked_ptr_kernel<crc16,bytes>"},
	{2, true, ecg_crc_masked_ptr_kernel<32, true, true, TK_4>, "ecg_crc_masked_ptr_kernel<crc32>"},
	{2, false, ecg_crc_masked_ptr_kernel<32, true, false, TK_5>, "ecg_crc_masked_ptr_kernel<crc32,bytes>"},
	{3, true, ecg_crc_masked_ptr_kernel<64, true, true, TK_4>, "ecg_crc_masked_ptr_kernel<crc64>"},
	{3, false, ecg_crc_masked_ptr_kernel<64, true, false, TK_5>, "ecg_crc_masked_ptr_kernel<crc64,bytes>"},
	{7, true, ecg_adler_masked_ptr_kernel<true>, "ecg_adler_masked_ptr_kernel"},
	{7, false, ecg_adler_masked_ptr_kernel<false>, "ecg_adler_masked_ptr_kernel<bytes>"},
};

// ecg_csum_updated and ecg_csum_updated_ptrs
const csum_entry<ecg_csum_updated_params_t> g_updated[] = {
	{1, true, ecg_crc_updated_kernel<16, false, true, TK_4>, "ecg_crc_updated_kernel<crc16>"},
	{1, false, ecg_crc_updated_kernel<16, false, false, TK_5>, "ecg_crc_updated_kernel<crc16,bytes>"},
	{2, true, ecg_crc_updated_kernel<32, true, true, TK_4>, "ecg_crc_updated_kernel<crc32>"},
	{2, false, ecg_crc_updated_kernel<32, true, false, TK_5>, "ecg_crc_updated_kernel<crc32,bytes>"},
	{3, true, ecg_crc_updated_kernel<64, true, true, TK_4>, "ecg_crc_updated_kernel<crc64>"},
	{3, false, ecg_crc_updated_kernel<64, true, false, TK_5>, "ecg_crc_updated_kernel<crc64,bytes>"},
	{7, true, ecg_adler_updated_kernel<true>, "ecg_adler_updated_kernel"},
	{7, false, ecg_adler_updated_kernel<false>, "ecg_adler_updated_kernel<bytes>"},
};

const csum_entry<ecg_csum_updated_params_t> g_updated_ptr[] = {
	{1, true, ecg_crc_updated_ptr_kernel<16, false, true, TK_4>, "ecg_crc_updated_ptr_kernel<crc16>"},
	{1, false, ecg_crc_updated_ptr_kernel<16, false, false, TK_5>, "ecg_crc_updated_ptr_kernel<crc16,bytes>"},
	{2, true, ecg_crc_updated_ptr_kernel<32, true, true, TK_4>, "ecg_crc_updated_ptr_kernel<crc32>"},
	{2, false, ecg_crc_updated_ptr_kernel<32, true, false, TK_5>, "ecg_crc_updated_ptr_kernel<crc32,bytes>"},
	{3, true, ecg_crc_updated_ptr_kernel<64, true, true, TK_4>, "ecg_crc_updated_ptr_kernel<crc64>"},
	{3, false, ecg_crc_updated_ptr_kernel<64, true, false, TK_5>, "ecg_crc_updated_ptr_kernel<crc64,bytes>"},
	{7, true, ecg_adler_updated_ptr_kernel<true>, "ecg_adler_updated_ptr_kernel"},
	{7, false, ecg_adler_updated_ptr_kernel<false>, "ecg_adler_updated_ptr_kernel<bytes>"},
};

const csum_entry<ecg_csum_masked_params_t> g_cells_ptr[] = {
	{1, true, ecg_crc_cells_ptr_kernel<16, false, true, TK_4>, "ecg_crc_cells_ptr_kernel<crc16>"},
	{1, false, ecg_crc_cells_ptr_kernel<16, false, false, TK_5>, "ecg_crc_cells_ptr_kernel<crc16,bytes>"},
	{2, true, ecg_crc_cells_ptr_kernel<32, true, true, TK_4>, "ecg_crc_cells_ptr_kernel<crc32>"},
	{2, false, ecg_crc_cells_ptr_kernel<32, true, false, TK_5>, "ecg_crc_cells_ptr_kernel<crc32,bytes>"},
	{3, true, ecg_crc_cells_ptr_kernel<64, true, true, TK_4>, "ecg_crc_cells_ptr_kernel<crc64>"},
	{3, false, ecg_crc_cells_ptr_kernel<64, true, false, TK_5>, "ecg_crc_cells_ptr_kernel<crc64,bytes>"},
	{7, true, ecg_adler_cells_ptr_kernel<true>, "ecg_adler_cells_ptr_kernel"},
	{7, false, ecg_adler_cells_ptr_kernel<false>, "ecg_adler_cells_ptr_kernel<bytes>"},
};

// Launch the (type, aligned) row of table t on min(nb, cap) blocks of `threads`
// and report its name.
template <class P, uint32_t N>
int launch_row(const csum_entry<P> (&t)[N], bool aligned, uint64_t nb, uint64_t cap, uint32_t threads, const P *p,
	       void *stream, const char **kernel)
{
	for (uint32_t i = 0; i < N; i++) {
		if (t[i].type != p->type || t[i].aligned != aligned)
			continue;
		hipLaunchKernelGGL(t[i].fn, dim3((uint32_t)(nb < cap ? nb : cap)), dim3(threads), 0,
				   (hipStream_t)stream, *p);
		if (kernel)
			*kernel = t[i].name;
		return (int)hipGetLastError();
	}
	return (int)hipErrorInvalidValue;
}

} // namespace

extern "C" int ecg_k_launch_csum_masked(const ecg_csum_masked_params_t *p, void *stream, uint32_t max_blocks,
					const char **kernel)
{
	const uint64_t total = (uint64_t)p->nstripes * p->slots * p->nch;
	const bool ptrs = p->cells_dev != nullptr;
	// the chunks of every cell start 16-byte aligned only when all four are;
	// of a cell table the host says so, and the sizes must agree
	const bool aligned = ptrs ? !p->bytewise
				  : (((uint64_t)(uintptr_t)p->src | (uint64_t)p->stripe_stride | p->cell_bytes |
				      p->chunk_bytes) & 15u) == 0;

	if (total == 0)
		return (int)hipSuccess;
	if (p->k == 0 || p->k > ECG_RM_MAX_K || p->p == 0 || p->p > ECG_RM_MAX_P || p->which == 0 || p->which > 3 ||
	    p->slots > p->k + p->p || p->masks == nullptr || p->chunk_bytes == 0 ||
	    (uint64_t)(p->nch - 1) * p->chunk_bytes >= p->cell_bytes ||
	    (ptrs && aligned && ((p->cell_bytes | p->chunk_bytes) & 15u)))
		return (int)hipErrorInvalidValue;
	// as ecg_k_launch_csum: 16 blocks per CU, grid-stride beyond
	if (ptrs)
		return launch_row(g_masked_ptr, aligned, (total + CS_WAVES - 1) / CS_WAVES,
				  max_blocks ? max_blocks : 256 * 16, CS_BLOCK, p, stream, kernel);
	return launch_row(g_masked, aligned, (total + CS_WAVES - 1) / CS_WAVES, max_blocks ? max_blocks : 256 * 16,
			  CS_BLOCK, p, stream, kernel);
}

extern "C" int ecg_k_launch_csum_updated(const ecg_csum_updated_params_t *p, void *stream, uint32_t max_blocks,
					 const char **kernel)
{
	const uint64_t total = (uint64_t)p->nstripes * p->p * p->nch;
	const bool ptrs = p->cells_dev != nullptr;
	// as ecg_k_launch_csum_masked: every chunk starts 16-byte aligned only when
	// the base, both parity strides and the two sizes are; of a cell table the
	// host says so, and the sizes must agree
	const bool aligned = ptrs ? !p->bytewise
				  : (((uint64_t)(uintptr_t)p->src | (uint64_t)p->cell_stride |
				      (uint64_t)p->stripe_stride | p->cell_bytes | p->chunk_bytes) & 15u) == 0;

	if (total == 0)
		return (int)hipSuccess;
	if (p->k == 0 || p->k > ECG_KMAX_K || p->p == 0 || p->p > ECG_KMAX_R || p->masks == nullptr ||
	    p->out == nullptr || (!ptrs && p->src == nullptr) || p->chunk_bytes == 0 ||
	    (uint64_t)(p->nch - 1) * p->chunk_bytes >= p->cell_bytes ||
	    (ptrs && aligned && ((p->cell_bytes | p->chunk_bytes) & 15u)))
		return (int)hipErrorInvalidValue;
	// as ecg_k_launch_csum: 16 blocks per CU, grid-stride beyond
	if (ptrs)
		return launch_row(g_updated_ptr, aligned, (total + CS_WAVES - 1) / CS_WAVES,
				  max_blocks ? max_blocks : 256 * 16, CS_BLOCK, p, stream, kernel);
	return launch_row(g_updated, aligned, (total + CS_WAVES - 1) / CS_WAVES, max_blocks ? max_blocks : 256 * 16,
			  CS_BLOCK, p, stream, kernel);
}

extern "C" int ecg_k_launch_csum_cells(const ecg_csum_masked_params_t *p, void *stream, uint32_t max_blocks,
				       const char **kernel)
{
	uint64_t total;

	if (p->ncells == 0 || p->nch == 0)
		return (int)hipSuccess;
	if (p->cells_dev == nullptr || p->out == nullptr || p->chunk_bytes == 0 ||
	    (uint64_t)(p->nch - 1) * p->chunk_bytes >= p->cell_bytes ||
	    __builtin_mul_overflow(p->ncells, (uint64_t)p->nch, &total) ||
	    (!p->bytewise && ((p->cell_bytes | p->chunk_bytes) & 15u)))
		return (int)hipErrorInvalidValue;
	return launch_row(g_cells_ptr, !p->bytewise, (total + CS_WAVES - 1) / CS_WAVES,
			  max_blocks ? max_blocks : 256 * 16, CS_BLOCK, p, stream, kernel);
}

extern "C" int ecg_k_launch_csum_mask(const void *got, const void *want, uint32_t nstripes, uint32_t ncells,
				      uint32_t nch, uint64_t stripe_stride, uint64_t cell_stride,
				      uint32_t first_cell, uint32_t len, uint32_t *masks, void *stream,
				      const char **kernel)
{
	const uint64_t n = (uint64_t)nstripes * ncells;
	uint64_t nb = (n + CS_BLOCK - 1) / CS_BLOCK;

	if (n == 0 || nch == 0)
		return (int)hipSuccess;
	if (nb > 256 * 4)
		nb = 256 * 4;
	void (*fn)(const uint8_t *, const uint8_t *, uint32_t, uint32_t, uint32_t, uint64_t, uint64_t, uint32_t,
		   uint32_t *) =
		len == 2 ? ecg_csum_mask_kernel<2> : len == 4 ? ecg_csum_mask_kernel<4>
		: len == 8 ? ecg_csum_mask_kernel<8> : nullptr;
	if (fn == nullptr || masks == nullptr || first_cell + (uint64_t)ncells > 32)
		return (int)hipErrorInvalidValue;
	hipLaunchKernelGGL(fn, dim3((uint32_t)nb), dim3(CS_BLOCK), 0, (hipStream_t)stream, (const uint8_t *)got,
			   (const uint8_t *)want, nstripes, ncells, nch, stripe_stride, cell_stride, first_cell, masks);
	if (kernel)
		*kernel = "ecg_csum_mask_kernel";
	return (int)hipGetLastError();
}

extern "C" int ecg_k_launch_csum_compare(const void *got, const void *want, uint64_t n, uint32_t len,
					 uint64_t *result, void *stream, const char **kernel)
{
	uint64_t nb = (n + CS_BLOCK - 1) / CS_BLOCK;

	if (n == 0)
		return (int)hipSuccess;
	if (nb > 256 * 4)
		nb = 256 * 4;
	void (*fn)(const uint8_t *, const uint8_t *, uint64_t, unsigned long long *) =
		len == 2 ? ecg_csum_compare_kernel<2> : len == 4 ? ecg_csum_compare_kernel<4>
		: len == 8 ? ecg_csum_compare_kernel<8> : nullptr;
	if (fn == nullptr)
		return (int)hipErrorInvalidValue;
	hipLaunchKernelGGL(fn, dim3((uint32_t)nb), dim3(CS_BLOCK), 0, (hipStream_t)stream, (const uint8_t *)got,
			   (const uint8_t *)want, n, (unsigned long long *)result);
	if (kernel)
		*kernel = "ecg_csum_compare_kernel";
	return (int)hipGetLastError();
}

extern "C" int ecg_k_launch_csum(const ecg_csum_params_t *p, void *stream, uint32_t max_blocks,
				 const char **kernel)
{
	const uint64_t total = (uint64_t)p->n_ext * p->nchunks;
	const bool aligned = (((uint64_t)(uintptr_t)p->src | (uint64_t)p->ext_stride | p->first_bytes |
			       p->chunk_bytes) & 15u) == 0;
	// a workgroup per chunk when one wave per chunk would leave fewer than 4
	// waves per SIMD and every wave still gets >= 2 steps (adler32 too:
	// profiles/r01/bench_csum.json adler32_cs1024K rows)
	const uint64_t steps = (p->chunk_bytes / 16 + 63) / 64;
	const bool split = p->variant == 2 || (p->variant == 0 && total < 4096 && steps >= 2 * SPLIT_NW);

	if (total == 0)
		return (int)hipSuccess;
	if (aligned && split)
		return launch_row(g_split, true, total, max_blocks ? max_blocks : 256 * 8, 64 * SPLIT_NW, p, stream,
				  kernel);
	if (max_blocks == 0)
		max_blocks = 256 * 16;	// 16 blocks per CU, grid-stride beyond
	if (p->type != 7 && aligned && p->variant == 3) {
		const uint32_t per_block = CS_WAVES * (64 / ECG_CSUM_GLANES);

		return launch_row(g_group, true, (total + per_block - 1) / per_block, max_blocks, CS_BLOCK, p, stream,
				  kernel);
	}
	return launch_row(g_csum, aligned, (total + CS_WAVES - 1) / CS_WAVES, max_blocks, CS_BLOCK, p, stream, kernel);
}
