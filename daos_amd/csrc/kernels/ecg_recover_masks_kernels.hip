// ecg_recover_masks_kernels.hip -- recovery with one erasure set per stripe
// (ecg_recover_masks, ecg_recover_masks_ptrs): a rebuild batch whose stripes
// lost different shards, or the second half of a checksum-driven scrub, in one
// launch.
//
// A block row takes `grp` consecutive stripes (1 .. 64) and walks them as
// every mask-driven kernel does (ecg_rows_dev.h rows_scan / rows_next): a lane
// reads a stripe's mask word with the one reading the host shares (ecg_kabi.h
// ecg_erasure_set_read), and a ballot leaves the stripes with a valid set as a
// wave-uniform 64-bit mask.  For a stripe whose mask reads as set i the block
// takes entry i of the (k, p) set table the host keeps on the device (host/
// ecg_recover_masks.c): e, the erased cells in ecg_recov_rows's output order,
// the k survivors, and the e x k perm tables already in the product's LDS
// layout -- staged with one 16-byte copy per thread, and not at all when the
// previous stripe of the block had the same set.  k source addresses and e
// destination addresses follow from the entry (wave-uniform), and the columns
// run the product's column code (ecg_mm_dev.h mm_ptr_item) with rows = e.
//
// Two layouts, one body each for the lane and the byte kernels (rm_lanes,
// rm_bytes): a strided image [S][k+p][C], or a table of cell addresses,
// cells[s * (k + p) + c] = the device address of logical cell c of stripe s,
// for callers whose stripes are separate buffers (rebuild, the batching
// queue's per-request stripes, a degraded read over an sgl).  The bodies ask
// an addressing struct (rm_strided, rm_table) where a stripe's cells are and
// share everything else; the four __global__ entry points only choose it.
//
// Every address derives from the table entry of a validated index, never
// from raw mask bits, so all 2^32 mask values are safe (and read inside the
// stripe's row of a cell table); destinations are erased cells and sources
// survivors, so the in-place write has no hazard.
//
// One kernel, two grids (the launcher's choice, ECG_RM_SPARSE): grp = 1 with
// a block per column when every stripe has work, grp = 64 with a few column
// blocks striding when almost none has -- a clean batch then costs S / 64 *
// grid.x blocks of one load each.  Column-block 0 of a row counts its stripes
// into `result` (ecg_rows_dev.h rows_count).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../ecg_kabi.h"
#include "ecg_mm_dev.h"
#include "ecg_rows_dev.h"

namespace {

// The reader of a mask word (ecg_rows_dev.h): the index of the set the word
// reads as, refused when it reads as none; a regenerated cell is the call's
// unit, the e of the set's table entry.  nsets bounds the index once more (it
// cannot fail: the reading is a bijection onto 0 .. nsets-1).
struct rm_read {
	const uint32_t *__restrict__ masks;
	int k, p;
	uint32_t nsets;
	const u32x4 *__restrict__ settbl;
	uint32_t entq;
	static constexpr int none = ECG_RM_NONE;

	__device__ int load(uint64_t s) const
	{
		const int idx = ecg_erasure_set_read(masks[s], k, p);

		return idx >= (int)nsets ? ECG_RM_RANGE : idx;
	}
	__device__ int verdict(int idx) const { return rows_verdict(idx == ECG_RM_NONE, idx >= 0); }
	__device__ unsigned long long units(int idx) const { return settbl[(uint64_t)idx * entq][0]; }
};

// byte j of the entry's survivor word
__device__ __forceinline__ uint32_t rm_dec(const u32x4 &d, int j)
{
	return (d[j / 4] >> (8 * (j % 4))) & 0xffu;
}

// Where a stripe's cells are -- all the strided and the cell-table kernels
// differ in.  A body positions the struct on a stripe (at), binds each slot of
// the column code's address array (survivor j, destination KM + r) to its
// logical cell once per stripe (bind), asks per column for the slot's address
// at the column's offset (col), and the byte body for a byte of a cell (byte).
// The cell c is always an index out of the set-table entry.

// [S][k+p][C] with a stripe stride: every address is arithmetic on the
// stripe's base, done per column, so nothing is bound.
struct rm_strided {
	const uint8_t *base;
	int64_t stride;
	uint64_t C;
	uint64_t sb;

	__device__ rm_strided(const uint8_t *base_, int64_t stride_, uint64_t C_) : base(base_), stride(stride_), C(C_) {}
	__device__ void at(uint32_t s) { sb = (uint64_t)(uintptr_t)base + (uint64_t)((int64_t)s * stride); }
	__device__ void bind(int, uint32_t) {}
	__device__ uint64_t col(int, uint32_t c, uint64_t cbase) const { return sb + cbase + (uint64_t)c * C; }
	__device__ uint8_t *byte(uint32_t c, uint64_t i) const
	{
		return reinterpret_cast<uint8_t *>((uintptr_t)sb) + (uint64_t)c * C + i;
	}
};

// The stripe's row pt of a cell table: a bound slot is pt[c], loaded once per
// stripe, before the column loop -- one dependent load per cell and stripe,
// not per column (wave-uniform: the set index comes from a readlane, so these
// are scalar loads of a read-only table) -- and a column adds its offset.
struct rm_table {
	const uint64_t *__restrict__ cells;
	uint32_t n;	// k + p
	const uint64_t *__restrict__ pt;
	uint64_t slot[ECG_KMAX_K + ECG_RM_MAX_P];	// those bound, the rest left unset

	__device__ rm_table(const uint64_t *cells_, uint32_t n_) : cells(cells_), n(n_) {}
	__device__ void at(uint32_t s) { pt = cells + (uint64_t)s * n; }
	__device__ void bind(int i, uint32_t c) { slot[i] = pt[c]; }
	__device__ uint64_t col(int i, uint32_t, uint64_t cbase) const { return slot[i] + cbase; }
	__device__ uint8_t *byte(uint32_t c, uint64_t i) const { return reinterpret_cast<uint8_t *>(pt[c]) + i; }
};

// The lane kernels' body.  K as ecg_mm_kernel's (0 = runtime-shaped), RM = p
// output rows at most (a stripe's e <= p rows run with rows = e).  16-byte
// lanes only: every cell address 16-byte aligned and C % 16 == 0 (the
// launcher sends everything else to the byte kernel), so a partial last column
// is a lane mask.  s_tbl: the block's ECG_TBL_WORDS(KM, RM) staged table words.
template <int K, int RM, class Addr>
__device__ __forceinline__ void rm_lanes(const ecg_mm_params_t &P, u32x4 *s_tbl, const u32x4 *__restrict__ settbl,
					 const uint32_t *__restrict__ masks, unsigned long long *result,
					 uint32_t grp, uint32_t nsets, Addr A)
{
	constexpr int KM = K ? K : ECG_KMAX_K;
	const int k = K ? K : (int)P.k;
	const uint64_t C = P.cell_bytes;
	const uint32_t nchunk = (uint32_t)((C + CHUNK_BYTES - 1) / CHUNK_BYTES);
	const uint32_t lo = lane_off<16>();
	const uint32_t entq = ECG_RM_ENT_Q(k, RM);
	const uint32_t nrow = rows_count_rows(P.nstripes, grp);
	const rm_read read = {masks, k, RM, nsets, settbl, entq};
	int staged = -1;	// the set whose tables s_tbl holds

	for (uint32_t row = blockIdx.y; row < nrow; row += gridDim.y) {
		int il, idx;
		uint64_t todo = rows_scan(P.nstripes, row, grp, result, read, &il);

		while (todo) {
			const uint32_t s = rows_next(&todo, row, grp, il, &idx);
			const u32x4 *__restrict__ ent = settbl + (uint64_t)idx * entq;

			if (staged != idx) {
				__syncthreads();	// the previous stripe's columns are done with s_tbl
				if ((int)threadIdx.x < ECG_TBL_WORDS(k, RM))
					s_tbl[threadIdx.x] = ent[2 + threadIdx.x];
				__syncthreads();
				staged = idx;
			}

			// the set's rows, erased cells and survivors (wave-uniform)
			const u32x4 hd = ent[0], dec = ent[1];
			const int e = (int)hd[0];

			A.at(s);
#pragma unroll
			for (int j = 0; j < KM; j++)
				if (j < k)
					A.bind(j, rm_dec(dec, j));
#pragma unroll
			for (int r = 0; r < RM; r++)
				if (r < e)
					A.bind(KM + r, hd[1 + r]);

			for (uint32_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
				const uint64_t cbase = (uint64_t)ch * CHUNK_BYTES;
				uint64_t a[KM + RM];
				uint32_t z = 0;

#pragma unroll
				for (int j = 0; j < KM; j++) {
					if (j < k) {
						a[j] = A.col(j, rm_dec(dec, j), cbase);
						asm volatile("" : "+s"(a[j]));
					}
				}
#pragma unroll
				for (int r = 0; r < RM; r++) {
					if (r < e) {
						a[KM + r] = A.col(KM + r, hd[1 + r], cbase);
						asm volatile("" : "+s"(a[KM + r]));
					}
				}
				asm volatile("" : "+v"(z));
				const u32x4 *tb = s_tbl + z;
				// a partial last column is a lane mask (C % 16 == 0 here)
				if (cbase + CHUNK_BYTES <= C || cbase + lo + 16 <= C)
					mm_ptr_item<KM, RM, 16>(P, tb, k, e, s, cbase, lo, a);
			}
		}
	}
}

// The byte kernels' body.  Any alignment, any length, any k <= 16 and p <= 3:
// a block takes 4 KiB columns of one stripe at a time, a lane the bytes t,
// t + 256, ... of a column.  Same scan, entries and counters as the lane
// body; the set's tables are read where they lie (wave-uniform loads).
template <class Addr>
__device__ __forceinline__ void rm_bytes(const ecg_mm_params_t &P, const u32x4 *__restrict__ settbl,
					 const uint32_t *__restrict__ masks, unsigned long long *result,
					 uint32_t grp, uint32_t nsets, Addr A)
{
	const uint64_t C = P.cell_bytes;
	const uint32_t nchunk = (uint32_t)((C + CHUNK_BYTES - 1) / CHUNK_BYTES);
	const int k = (int)P.k, p = (int)P.rows;
	const uint32_t entq = ECG_RM_ENT_Q(k, p);
	const uint32_t nrow = rows_count_rows(P.nstripes, grp);
	const rm_read read = {masks, k, p, nsets, settbl, entq};

	for (uint32_t row = blockIdx.y; row < nrow; row += gridDim.y) {
		int il, idx;
		uint64_t todo = rows_scan(P.nstripes, row, grp, result, read, &il);

		while (todo) {
			const uint32_t s = rows_next(&todo, row, grp, il, &idx);
			const u32x4 *__restrict__ ent = settbl + (uint64_t)idx * entq;
			const u32x4 hd = ent[0];
			const uint8_t *__restrict__ dec = reinterpret_cast<const uint8_t *>(ent + 1);
			const int e = (int)hd[0];

			A.at(s);
			for (uint32_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
				const uint64_t cbase = (uint64_t)ch * CHUNK_BYTES;

				for (uint64_t i = cbase + threadIdx.x; i < cbase + CHUNK_BYTES && i < C; i += BLOCK) {
					uint32_t o[ECG_RM_MAX_P] = {0u, 0u, 0u};

					for (int j = 0; j < k; j++) {
						const uint32_t x = *A.byte(dec[j], i);
						// the set's tables: p <= 3 rows, one t2 word
						const u32x4 t2 = ent[2 + ECG_TBL_ROW(p, j, p)];

#pragma unroll
						for (int r = 0; r < ECG_RM_MAX_P; r++) {
							if (r < e) {
								const u32x4 t = ent[2 + ECG_TBL_ROW(p, j, r)];
								const ecg_ptbl_t pt = {t[0], t[1], t[2], t[3], t2[r]};

								o[r] ^= gf_mul1(pt, x);
							}
						}
					}
#pragma unroll
					for (int r = 0; r < ECG_RM_MAX_P; r++)
						if (r < e)
							*A.byte(hd[1 + r], i) = (uint8_t)o[r];
				}
			}
		}
	}
}

} // namespace

// The entry points: the strided image P.src == P.dst with its stripe stride
// (ecg_recover_masks), or the table `cells` (ecg_recover_masks_ptrs).
template <int K, int RM>
__global__ void __launch_bounds__(BLOCK, ECG_MM_WPE(K, RM, 16) ? ECG_MM_WPE(K, RM, 16) : 1)
ecg_recover_masks_kernel(const ecg_mm_params_t P, const u32x4 *__restrict__ settbl,
			 const uint32_t *__restrict__ masks, unsigned long long *result, uint32_t grp,
			 uint32_t nsets)
{
	__shared__ u32x4 s_tbl[ECG_TBL_WORDS(K ? K : ECG_KMAX_K, RM)];

	rm_lanes<K, RM>(P, s_tbl, settbl, masks, result, grp, nsets,
			rm_strided(P.src, P.src_stripe_stride, P.cell_bytes));
}

__global__ void __launch_bounds__(BLOCK)
ecg_recover_masks_byte_kernel(const ecg_mm_params_t P, const u32x4 *__restrict__ settbl,
			      const uint32_t *__restrict__ masks, unsigned long long *result, uint32_t grp,
			      uint32_t nsets)
{
	rm_bytes(P, settbl, masks, result, grp, nsets, rm_strided(P.dst, P.dst_stripe_stride, P.cell_bytes));
}

template <int K, int RM>
__global__ void __launch_bounds__(BLOCK, ECG_MM_WPE(K, RM, 16) ? ECG_MM_WPE(K, RM, 16) : 1)
ecg_recover_masks_ptr_kernel(const ecg_mm_params_t P, const u32x4 *__restrict__ settbl,
			     const uint64_t *__restrict__ cells, const uint32_t *__restrict__ masks,
			     unsigned long long *result, uint32_t grp, uint32_t nsets)
{
	__shared__ u32x4 s_tbl[ECG_TBL_WORDS(K ? K : ECG_KMAX_K, RM)];

	rm_lanes<K, RM>(P, s_tbl, settbl, masks, result, grp, nsets,
			rm_table(cells, (uint32_t)((K ? K : (int)P.k) + RM)));
}

__global__ void __launch_bounds__(BLOCK)
ecg_recover_masks_ptr_byte_kernel(const ecg_mm_params_t P, const u32x4 *__restrict__ settbl,
				  const uint64_t *__restrict__ cells, const uint32_t *__restrict__ masks,
				  unsigned long long *result, uint32_t grp, uint32_t nsets)
{
	rm_bytes(P, settbl, masks, result, grp, nsets, rm_table(cells, P.k + P.rows));
}

// ---------------------------------------------------------------------------
// Dispatch: one table for both layouts.  The lane instantiations (the k of
// the DAOS EC classes; the rest runtime-shaped), then the byte kernels; the
// launcher reports an entry's name (strided) or pname (cell table).
// ---------------------------------------------------------------------------
typedef void (*rm_fn_t)(const ecg_mm_params_t, const u32x4 *, const uint32_t *, unsigned long long *, uint32_t,
			uint32_t);
typedef void (*rmp_fn_t)(const ecg_mm_params_t, const u32x4 *, const uint64_t *, const uint32_t *,
			 unsigned long long *, uint32_t, uint32_t);

struct rmentry {
	int k, rm;
	rm_fn_t fn;
	rmp_fn_t pfn;
	const char *name, *pname;
};

#define RME(K_, R_)                                                                                                    \
	{K_, R_, ecg_recover_masks_kernel<K_, R_>, ecg_recover_masks_ptr_kernel<K_, R_>,                               \
	 "ecg_recover_masks_kernel<" #K_ ", " #R_ ">", "ecg_recover_masks_ptr_kernel<" #K_ ", " #R_ ">"}
#define RMK(K_) RME(K_, 1), RME(K_, 2), RME(K_, 3)

static const rmentry g_rm[] = {
	RMK(2), RMK(4), RMK(8), RMK(16), RMK(0),
	{-1, -1, ecg_recover_masks_byte_kernel, ecg_recover_masks_ptr_byte_kernel, "ecg_recover_masks_byte_kernel",
	 "ecg_recover_masks_ptr_byte_kernel"}};
#define N_RM ((uint32_t)(sizeof(g_rm) / sizeof(g_rm[0])))
#define RM_BYTE (N_RM - 1)

extern "C" int ecg_k_launch_recover_masks(const ecg_mm_params_t *p, const void *settbl, const uint64_t *cells_dev,
					  const uint32_t *masks, uint64_t *result, int bytewise, int sparse,
					  const ecg_launch_cfg_t *cfg, void *stream, const char **kernel)
{
	hipStream_t st = (hipStream_t)stream;
	uint32_t gx, gy, id = RM_BYTE;

	if (p->nstripes == 0 || p->cell_bytes == 0)
		return (int)hipSuccess;
	if (p->k == 0 || p->k > ECG_RM_MAX_K || p->rows == 0 || p->rows > ECG_RM_MAX_P || settbl == nullptr ||
	    masks == nullptr || result == nullptr)
		return (int)hipErrorInvalidValue;
	if (cells_dev == nullptr && (p->src != p->dst || p->src_stripe_stride != p->dst_stripe_stride))
		return (int)hipErrorInvalidValue;
	const uint32_t grp = sparse ? 64u : ECG_RM_DENSE_GRP;
	const uint32_t nsets = ecg_erasure_set_count((int)p->k, (int)p->rows);

	rows_grid(p, grp, sparse ? ECG_REPAIR_GRID_X : ECG_RM_DENSE_GRID_X, cfg, &gx, &gy);

	if (!bytewise) {
		// the lane kernel reads and writes dwordx4 at the cells' own addresses;
		// those of a cell table the host has found 16-byte aligned (the table
		// is not read here)
		uint64_t bits = p->cell_bytes;

		if (cells_dev == nullptr)
			bits |= (uint64_t)(uintptr_t)p->src | (uint64_t)p->src_stripe_stride;
		if ((bits & 15u) != 0)
			return (int)hipErrorInvalidValue;
		for (id = 0; id < RM_BYTE; id++)
			if (g_rm[id].rm == (int)p->rows && (g_rm[id].k == (int)p->k || g_rm[id].k == 0))
				break;
		if (id == RM_BYTE)
			return (int)hipErrorInvalidValue;
	}
	if (cells_dev == nullptr)
		hipLaunchKernelGGL(g_rm[id].fn, dim3(gx, gy), dim3(BLOCK), 0, st, *p, (const u32x4 *)settbl, masks,
				   (unsigned long long *)result, grp, nsets);
	else
		hipLaunchKernelGGL(g_rm[id].pfn, dim3(gx, gy), dim3(BLOCK), 0, st, *p, (const u32x4 *)settbl, cells_dev,
				   masks, (unsigned long long *)result, grp, nsets);
	if (kernel)
		*kernel = cells_dev ? g_rm[id].pname : g_rm[id].name;
	return (int)hipGetLastError();
}
