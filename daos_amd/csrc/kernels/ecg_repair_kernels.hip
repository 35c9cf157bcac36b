// ecg_repair_kernels.hip -- rewrite the cell ecg_verify located (ecg_repair):
// the second half of a scrub, queued behind the check on the same stream with
// no host round trip in between.
//
// A block row takes 64 stripes and walks them as every mask-driven kernel does
// (ecg_rows_dev.h rows_scan / rows_next): a lane reads a stripe's status word
// with the one reading of that word the host and the summary kernel share
// (ecg_kabi.h ecg_verify_classify), and a ballot leaves the located stripes
// as a wave-uniform 64-bit mask -- in a batch that is almost always clean it
// is zero and the block is done.  The block walks the set bits; for a located
// cell c it chooses its decode row and its operands per stripe:
//   c >= k  parity row c-k = row c-k of G over the k data cells
//   c <  k  data cell c = the decode row of erasure {c}: the other k-1 data
//           cells in their own slots, parity row 0 in slot c
// i.e. k source addresses and one destination built in registers from the
// strided operands, the k perm tables of row c staged into LDS from the
// (k+p) x k row tables the host keeps on the device (host/ecg_repair.c), and
// the product's column code with one output row (ecg_mm_dev.h mm_ptr_item,
// the pointer-table kernel's).  Every address derives from the classified c
// alone, never from raw status bits, so any of the 2^32 status values is
// safe; the destination is never one of its own sources, so the in-place
// write has no hazard.
//
// The grid is not one block per (column, stripe), nor one block row per
// stripe: grid.y runs over the groups of 64 stripes and grid.x over at most
// ECG_REPAIR_GRID_X columns (blocks stride over the rest), so a clean batch
// costs ECG_REPAIR_GRID_X * S / 64 blocks of one load each whatever the cell
// size, and a bad stripe still has ECG_REPAIR_GRID_X blocks to itself.
// Column-block 0 of a group counts its bad stripes into `result`
// (ecg_rows_dev.h rows_count).
//
// Two layouts, one body each for the lane and the byte kernels (rp_lanes,
// rp_bytes): the strided operands of ecg_verify, or a table of cell addresses,
// cells[s * (k + p) + c] = the device address of logical cell c of stripe s
// (ecg_repair_ptrs).  The bodies ask an addressing struct (rp_strided,
// rp_table) where a stripe's cells are and share everything else; the four
// __global__ entry points only choose it.  Over a table a stripe's sources are
// pt[j], pt[k] in slot c when a data cell is rewritten, and its destination
// pt[c]: indices inside the stripe's table row for any status value.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../ecg_kabi.h"
#include "ecg_mm_dev.h"
#include "ecg_rows_dev.h"

namespace {

// The reader of a status word (ecg_rows_dev.h): the classified cell c of a
// stripe ecg_verify_classify attributes to one cell, refused when it does not;
// a rewritten data cell is the call's unit.
struct repair_read {
	const uint32_t *__restrict__ status;
	int k, p;
	static constexpr int none = -1;	// clean

	__device__ int load(uint64_t s) const { return ecg_verify_classify(status[s], k, p); }
	// the second test cannot fail (classify masks)
	__device__ int verdict(int c) const { return rows_verdict(c == -1, c >= 0 && c < k + p); }
	__device__ unsigned long long units(int c) const { return c < k; }
};

// Where a stripe's cells are -- all the strided and the cell-table kernels
// differ in (as ecg_recover_masks_kernels.hip rm_strided / rm_table).  A body
// positions the struct on a stripe (at) and asks for the address of data cell
// j (src), of parity row 0 (par0) and of the located cell c (dst); c is always
// the classified cell, 0 .. k+p-1.  The launch parameters are handed to each
// of them, not kept in the struct.

// P as ecg_verify's: src the data cells, dst the parity rows (dst_cell_off[r]
// = r * parity_cell_stride)
struct rp_strided {
	uint64_t sb, pb;

	__device__ void at(const ecg_mm_params_t &P, uint32_t s)
	{
		sb = (uint64_t)(uintptr_t)P.src + (uint64_t)((int64_t)s * P.src_stripe_stride);
		pb = (uint64_t)(uintptr_t)P.dst + (uint64_t)((int64_t)s * P.dst_stripe_stride);
	}
	__device__ uint64_t src(const ecg_mm_params_t &P, int j) const { return sb + (uint64_t)P.src_cell_off[j]; }
	__device__ uint64_t par0(const ecg_mm_params_t &P) const { return pb + (uint64_t)P.dst_cell_off[0]; }
	__device__ uint64_t dst(const ecg_mm_params_t &P, int c, int k) const
	{
		return c < k ? sb + (uint64_t)c * P.cell_bytes : pb + (uint64_t)P.dst_cell_off[c - k];
	}
};

// The stripe's row pt of a cell table: pt[c] the address of logical cell c
// (wave-uniform: c comes from a readlane, so these are scalar loads of a
// read-only table), loaded once per stripe, before the column loop.
struct rp_table {
	const uint64_t *__restrict__ cells;
	uint32_t k, n;	// data cells, k + p
	const uint64_t *__restrict__ pt;

	__device__ rp_table(const uint64_t *cells_, uint32_t k_, uint32_t p_) : cells(cells_), k(k_), n(k_ + p_) {}
	__device__ void at(const ecg_mm_params_t &, uint32_t s) { pt = cells + (uint64_t)s * n; }
	__device__ uint64_t src(const ecg_mm_params_t &, int j) const { return pt[j]; }
	__device__ uint64_t par0(const ecg_mm_params_t &) const { return pt[k]; }
	__device__ uint64_t dst(const ecg_mm_params_t &, int c, int) const { return pt[c]; }
};

// The lane kernels' body.  K as ecg_mm_kernel's (0 = runtime-shaped), one
// output row.  16-byte lanes only: every cell address (and stride) 16-byte
// aligned, C % 16 == 0 (the launcher sends everything else to the byte
// kernel), so a partial last column is a lane mask.  s_tbl: the block's
// ECG_TBL_WORDS(KM, 1) staged table words.  (No __restrict__ on the body's
// pointers: the kernels' own arguments carry it.)
template <int K, class Addr>
__device__ __forceinline__ void rp_lanes(const ecg_mm_params_t &P, u32x4 *s_tbl, const ecg_ptbl_t *rowtbl,
					 const uint32_t *status, unsigned long long *result, Addr A)
{
	constexpr int KM = K ? K : ECG_KMAX_K;
	const int k = K ? K : (int)P.k;
	const int p = (int)P.rows;
	const uint64_t C = P.cell_bytes;
	const uint32_t nchunk = (uint32_t)((C + CHUNK_BYTES - 1) / CHUNK_BYTES);
	const uint32_t lo = lane_off<16>();
	const uint32_t ngroup = rows_count_rows(P.nstripes, 64u);
	const repair_read read = {status, k, p};
	int staged = -1;	// the row whose tables s_tbl holds

	for (uint32_t g = blockIdx.y; g < ngroup; g += gridDim.y) {
		int cl, c;
		uint64_t todo = rows_scan(P.nstripes, g, 64u, result, read, &cl);

		while (todo) {
			const uint32_t s = rows_next(&todo, g, 64u, cl, &c);

			if (staged != c) {
				__syncthreads();	// the previous stripe's columns are done with s_tbl
				if ((int)threadIdx.x < k) {
					// written out, the whole t2 word: with mm_tbl<1>::put here
					// the columns of K = 4, 8, 16 were scheduled differently
					const ecg_ptbl_t t = rowtbl[c * k + (int)threadIdx.x];

					s_tbl[ECG_TBL_ROW(1, threadIdx.x, 0)] = (u32x4){t.t0lo, t.t0hi, t.t1lo, t.t1hi};
					s_tbl[ECG_TBL_ROW(1, threadIdx.x, 1)] = (u32x4){t.t2, 0u, 0u, 0u};
				}
				__syncthreads();
				staged = c;
			}

			// the stripe's k sources and its destination (wave-uniform)
			A.at(P, s);
			const uint64_t par0 = A.par0(P);
			uint64_t base[KM + 1];

#pragma unroll
			for (int j = 0; j < KM; j++)
				if (j < k)
					base[j] = j == c ? par0 : A.src(P, j);
			base[KM] = A.dst(P, c, k);

			for (uint32_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
				const uint64_t cbase = (uint64_t)ch * CHUNK_BYTES;
				uint64_t a[KM + 1];
				uint32_t z = 0;

#pragma unroll
				for (int j = 0; j < KM + 1; j++) {
					if (j < k || j == KM) {
						a[j] = base[j] + cbase;
						asm volatile("" : "+s"(a[j]));
					}
				}
				asm volatile("" : "+v"(z));
				const u32x4 *tb = s_tbl + z;
				// a partial last column is a lane mask (C % 16 == 0 here)
				if (cbase + CHUNK_BYTES <= C || cbase + lo + 16 <= C)
					mm_ptr_item<KM, 1, 16>(P, tb, k, 1, s, cbase, lo, a);
			}
		}
	}
}

// The byte kernels' body.  Any alignment, any length: a block takes 4 KiB
// columns of one stripe at a time, a lane the bytes t, t + 256, ... of a
// column.  Same status scan, operands, rows and counters as the lane body;
// the row's tables are read where they lie (wave-uniform loads).
template <class Addr>
__device__ __forceinline__ void rp_bytes(const ecg_mm_params_t &P, const ecg_ptbl_t *rowtbl, const uint32_t *status,
					 unsigned long long *result, Addr A)
{
	const uint64_t C = P.cell_bytes;
	const uint32_t nchunk = (uint32_t)((C + CHUNK_BYTES - 1) / CHUNK_BYTES);
	const int k = (int)P.k, p = (int)P.rows;
	const uint32_t ngroup = rows_count_rows(P.nstripes, 64u);
	const repair_read read = {status, k, p};

	for (uint32_t g = blockIdx.y; g < ngroup; g += gridDim.y) {
		int cl, c;
		uint64_t todo = rows_scan(P.nstripes, g, 64u, result, read, &cl);

		while (todo) {
			const uint32_t s = rows_next(&todo, g, 64u, cl, &c);

			A.at(P, s);
			const uint8_t *par0 = reinterpret_cast<const uint8_t *>((uintptr_t)A.par0(P));
			const ecg_ptbl_t *row = rowtbl + c * k;
			uint8_t *dst = reinterpret_cast<uint8_t *>((uintptr_t)A.dst(P, c, k));

			for (uint32_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
				const uint64_t cbase = (uint64_t)ch * CHUNK_BYTES;

				for (uint64_t i = cbase + threadIdx.x; i < cbase + CHUNK_BYTES && i < C; i += BLOCK) {
					uint32_t o = 0;

					for (int j = 0; j < k; j++) {
						const uint8_t *src =
							j == c ? par0 : reinterpret_cast<const uint8_t *>((uintptr_t)A.src(P, j));

						o ^= gf_mul1(row[j], src[i]);
					}
					dst[i] = (uint8_t)o;
				}
			}
		}
	}
}

} // namespace

// The entry points: the strided operands of P as ecg_verify's (ecg_repair),
// or the table `cells` (ecg_repair_ptrs).
template <int K>
__global__ void __launch_bounds__(BLOCK, ECG_MM_WPE(K, 1, 16) ? ECG_MM_WPE(K, 1, 16) : 1)
ecg_repair_kernel(const ecg_mm_params_t P, const ecg_ptbl_t *__restrict__ rowtbl,
		  const uint32_t *__restrict__ status, unsigned long long *result)
{
	__shared__ u32x4 s_tbl[ECG_TBL_WORDS(K ? K : ECG_KMAX_K, 1)];	// one output row

	rp_lanes<K>(P, s_tbl, rowtbl, status, result, rp_strided());
}

__global__ void __launch_bounds__(BLOCK)
ecg_repair_byte_kernel(const ecg_mm_params_t P, const ecg_ptbl_t *__restrict__ rowtbl,
		       const uint32_t *__restrict__ status, unsigned long long *result)
{
	rp_bytes(P, rowtbl, status, result, rp_strided());
}

template <int K>
__global__ void __launch_bounds__(BLOCK, ECG_MM_WPE(K, 1, 16) ? ECG_MM_WPE(K, 1, 16) : 1)
ecg_repair_ptr_kernel(const ecg_mm_params_t P, const ecg_ptbl_t *__restrict__ rowtbl,
		      const uint64_t *__restrict__ cells, const uint32_t *__restrict__ status,
		      unsigned long long *result)
{
	__shared__ u32x4 s_tbl[ECG_TBL_WORDS(K ? K : ECG_KMAX_K, 1)];

	rp_lanes<K>(P, s_tbl, rowtbl, status, result, rp_table(cells, (uint32_t)(K ? K : (int)P.k), P.rows));
}

__global__ void __launch_bounds__(BLOCK)
ecg_repair_ptr_byte_kernel(const ecg_mm_params_t P, const ecg_ptbl_t *__restrict__ rowtbl,
			   const uint64_t *__restrict__ cells, const uint32_t *__restrict__ status,
			   unsigned long long *result)
{
	rp_bytes(P, rowtbl, status, result, rp_table(cells, P.k, P.rows));
}

// ---------------------------------------------------------------------------
// Dispatch
// ---------------------------------------------------------------------------
typedef void (*repair_fn_t)(const ecg_mm_params_t, const ecg_ptbl_t *, const uint32_t *, unsigned long long *);
typedef void (*repair_pfn_t)(const ecg_mm_params_t, const ecg_ptbl_t *, const uint64_t *, const uint32_t *,
			     unsigned long long *);

// one table for both layouts: the launcher reports an entry's name (strided)
// or pname (cell table)
struct rentry {
	int k;
	repair_fn_t fn;
	repair_pfn_t pfn;
	const char *name, *pname;
};

#define RE(K_) {K_, ecg_repair_kernel<K_>, ecg_repair_ptr_kernel<K_>, "ecg_repair_kernel<" #K_ ">", \
		"ecg_repair_ptr_kernel<" #K_ ">"}

// the k of the DAOS EC classes; the rest runtime-shaped; then the byte kernels
static const rentry g_repair[] = {
	RE(2), RE(4), RE(8), RE(16), RE(0),
	{-1, ecg_repair_byte_kernel, ecg_repair_ptr_byte_kernel, "ecg_repair_byte_kernel",
	 "ecg_repair_ptr_byte_kernel"}};
#define N_REPAIR ((uint32_t)(sizeof(g_repair) / sizeof(g_repair[0])))
#define REPAIR_BYTE (N_REPAIR - 1)

extern "C" int ecg_k_launch_repair(const ecg_mm_params_t *p, const ecg_ptbl_t *rowtbl, const uint64_t *cells_dev,
				   const uint32_t *status, uint64_t *result, int bytewise,
				   const ecg_launch_cfg_t *cfg, void *stream, const char **kernel)
{
	hipStream_t st = (hipStream_t)stream;
	uint32_t gx, gy, id = REPAIR_BYTE;

	if (p->nstripes == 0 || p->cell_bytes == 0)
		return (int)hipSuccess;
	if (p->k == 0 || p->k > ECG_KMAX_K || p->rows == 0 || p->rows > ECG_KMAX_R || rowtbl == nullptr ||
	    status == nullptr || result == nullptr)
		return (int)hipErrorInvalidValue;
	rows_grid(p, 64u, ECG_REPAIR_GRID_X, cfg, &gx, &gy);

	if (!bytewise) {
		// the lane kernels read and write dwordx4 at the cells' own addresses;
		// those of a cell table the host has found 16-byte aligned (the table is
		// not read here)
		if ((cells_dev == nullptr && !aligned16(p)) || p->cell_bytes % 16u)
			return (int)hipErrorInvalidValue;
		for (id = 0; id < REPAIR_BYTE - 1; id++)	// no match: <0>, the last lane entry
			if (g_repair[id].k == (int)p->k)
				break;
	}
	if (cells_dev == nullptr)
		hipLaunchKernelGGL(g_repair[id].fn, dim3(gx, gy), dim3(BLOCK), 0, st, *p, rowtbl, status,
				   (unsigned long long *)result);
	else
		hipLaunchKernelGGL(g_repair[id].pfn, dim3(gx, gy), dim3(BLOCK), 0, st, *p, rowtbl, cells_dev, status,
				   (unsigned long long *)result);
	if (kernel)
		*kernel = cells_dev ? g_repair[id].pname : g_repair[id].name;
	return (int)hipGetLastError();
}
