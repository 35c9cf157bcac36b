// ecg_verify_kernels.hip -- parity consistency check (ecg_verify): does the
// stored parity of a stripe still match its stored data, and if not, which
// cell is wrong?  (DAOS answers the first half with obj_ec_encode_buf into a
// scratch buffer + memcmp, ref:src/object/obj_verify.c.)
//
// One read-only pass: the product kernel's column (ecg_mm_dev.h mm_load +
// mm_compute) run with ACC on the stored parity, the result kept in
// registers and nothing stored, leaves the syndrome
//     s_r = stored_parity[r] ^ XOR_j g[r][j] * data[j]
// of the lane's 16 bytes.  Clean data has s = 0: the wave ballots one "row r
// nonzero" bit per parity row and is done -- no atomics, no LDS traffic, no
// stores.  A wave that saw a nonzero syndrome (rare, wave-uniform) locates:
// had data cell j alone been wrong by e at a byte, s_r = g[r][j] * e for every
// row, so  g[0][j] * s_r == g[r][j] * s_0  for every r >= 1; the Cauchy1
// ratios g[r][j] / g[0][j] are pairwise distinct over j, so the test holds
// for the culprit and no other data cell.  Cells that fail it anywhere are
// struck from the stripe's candidate set (ecg_kabi.h: the status word).  The
// multiplies use the tables the block already staged in LDS for the product.
//
// Location assumes at most one wrong cell per stripe (a distance-(p+1) code
// cannot tell two wrong cells from some third one).
//
// Two layouts: strided operands (ecg_verify), or a table of cell addresses,
// cells[s * (k + p) + c] = the device address of logical cell c of stripe s
// (ecg_verify_ptrs), for callers whose shards were fetched into buffers of
// their own.  The cell-table lane kernel maps work and loads a stripe's
// addresses as the pointer-table product does (ecg_ptr_kernels.hip); the byte
// kernels are one body asking an addressing struct (vb_strided, vb_table)
// where a byte of a cell is.  The ballot, verify_dirty and the status atomics
// are the same code for all of them.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../ecg_kabi.h"
#include "ecg_mm_dev.h"

namespace {

// c * v for the 4 bytes of v (the tables are read back from the block's LDS
// copy: ecg_mm_dev.h mm_tbl::entry)
__device__ __forceinline__ uint32_t gf_mul4v(const ecg_ptbl_t &t, uint32_t v)
{
	return gf_mul4(t, v & 0x07070707u, (v >> 3) & 0x07070707u, (v >> 6) & 0x03030303u);
}

// The located part: the wave saw a nonzero syndrome (rowmask, wave-uniform).
// Every lane tests every data cell j against its own 16 syndrome bytes (a
// zero syndrome passes trivially); j stays a candidate only if all lanes
// agree.  One lane folds the wave's verdict into the stripe's status word.
// Not unrolled over j: this path is rare and must not shape the clean path's
// register allocation.
template <int RM>
__device__ __forceinline__ void verify_dirty(const u32x4 *tb, int k, int rows, const u32x4 *syn,
					     uint32_t rowmask, uint32_t *st)
{
	uint32_t elim = 0;

	if (rows >= 2) {
#pragma nounroll
		for (int j = 0; j < k; j++) {
			const ecg_ptbl_t t0 = mm_tbl<RM>::entry(tb, j, 0);
			uint32_t bad = 0;

#pragma unroll
			for (int r = 1; r < RM; r++) {
				if (r < rows) {
					const ecg_ptbl_t tr = mm_tbl<RM>::entry(tb, j, r);
#pragma unroll
					for (int w = 0; w < 4; w++)
						bad |= gf_mul4v(t0, syn[r][w]) ^ gf_mul4v(tr, syn[0][w]);
				}
			}
			if (__ballot(bad != 0) != 0)
				elim |= 1u << j;
		}
	}
	if ((threadIdx.x & 63u) == 0) {
		if (elim)
			atomicAnd(st, ~(elim << 8));
		atomicOr(st, rowmask);
	}
}

template <int KM, int RM>
__device__ __forceinline__ void verify_item(const ecg_mm_params_t &P, const u32x4 *tb, int k, int rows,
					    uint32_t s, uint64_t cbase, uint32_t lo, u32x4 *syn)
{
	constexpr int PH = (ECG_MM_PHASE(KM, 16) > 0 && ECG_MM_PHASE(KM, 16) < KM && KM % ECG_MM_PHASE(KM, 16) == 0)
				   ? ECG_MM_PHASE(KM, 16) : 0;
	u32x4 x[KM];

	mm_load<KM, false, 16, PH ? PH : KM>(P, k, s, cbase, lo, x);
	mm_compute<KM, RM, true, true, false, 16, PH, false>(P, tb, k, rows, s, cbase, lo, x, syn);
}

// The same column over cells given by address (ecg_mm_dev.h mm_ptr_item's
// loads and fold): a[j] = the wave-uniform address of data cell j at this
// column, a[KM + r] that of parity row r.  The stored parity is loaded before
// the fold, so those loads overlap it; the product stays in registers and
// nothing is stored.
template <int KM, int RM>
__device__ __forceinline__ void verify_ptr_item(const ecg_mm_params_t &P, const u32x4 *tb, int k, int rows,
						uint32_t s, uint64_t cbase, uint32_t lo, const uint64_t *a,
						u32x4 *syn)
{
	constexpr int PH = (ECG_MM_PHASE(KM, 16) > 0 && ECG_MM_PHASE(KM, 16) < KM && KM % ECG_MM_PHASE(KM, 16) == 0)
				   ? ECG_MM_PHASE(KM, 16) : 0;
	u32x4 x[KM], par[RM], outv[RM];

#pragma unroll
	for (int j = 0; j < (PH ? PH : KM); j++)
		if (j < k)
			x[j] = ld_src<16>(reinterpret_cast<const uint8_t *>(a[j]), lo);
#pragma unroll
	for (int r = 0; r < RM; r++)
		if (r < rows)
			par[r] = ld_g<16>(reinterpret_cast<const uint8_t *>(a[KM + r]) + lo);
	mm_compute<KM, RM, false, true, false, 16, PH, false, true>(P, tb, k, rows, s, cbase, lo, x, outv, a);
#pragma unroll
	for (int r = 0; r < RM; r++)
		if (r < rows)
			syn[r] = par[r] ^ outv[r];
}

// The lanes' syndromes of one column -> the stripe's status word: one "row r
// nonzero" ballot per parity row, and the located part when any is.
template <int RM>
__device__ __forceinline__ void verify_fold(const u32x4 *tb, int k, int rows, const u32x4 *syn, uint32_t *st)
{
	uint32_t rowmask = 0;

#pragma unroll
	for (int r = 0; r < RM; r++) {
		if (r < rows) {
			const uint32_t o = syn[r][0] | syn[r][1] | syn[r][2] | syn[r][3];

			if (__ballot(o != 0) != 0)
				rowmask |= 1u << r;
		}
	}
	if (__builtin_expect(rowmask != 0, 0))
		verify_dirty<RM>(tb, k, rows, syn, rowmask, st);
}

// Where a byte of a cell is -- all the strided and the cell-table byte kernels
// differ in.  The body positions the struct on a stripe (at) and asks for byte
// i of data cell j (data) or of parity row r (par), handing each the launch
// parameters.
struct vb_strided {
	const uint8_t *sb, *db;

	__device__ void at(const ecg_mm_params_t &P, uint32_t s)
	{
		sb = P.src + (int64_t)s * P.src_stripe_stride;
		db = P.dst + (int64_t)s * P.dst_stripe_stride;
	}
	__device__ uint32_t data(const ecg_mm_params_t &P, int j, uint64_t i) const { return sb[P.src_cell_off[j] + i]; }
	__device__ uint32_t par(const ecg_mm_params_t &P, int r, uint64_t i) const { return db[P.dst_cell_off[r] + i]; }
};

// the stripe's row pt of a cell table (wave-uniform loads of a read-only table)
struct vb_table {
	const uint64_t *__restrict__ cells;
	uint32_t k, n;	// data cells, k + p
	const uint64_t *__restrict__ pt;

	__device__ vb_table(const uint64_t *cells_, uint32_t k_, uint32_t n_) : cells(cells_), k(k_), n(n_) {}
	__device__ void at(const ecg_mm_params_t &, uint32_t s) { pt = cells + (uint64_t)s * n; }
	__device__ uint32_t data(const ecg_mm_params_t &, int j, uint64_t i) const
	{
		return reinterpret_cast<const uint8_t *>(pt[j])[i];
	}
	__device__ uint32_t par(const ecg_mm_params_t &, int r, uint64_t i) const
	{
		return reinterpret_cast<const uint8_t *>(pt[k + r])[i];
	}
};

// The byte kernels' body.  Any alignment, any length (the role
// ecg_mm_byte_kernel plays for the product): a block takes one 4 KiB column of
// one stripe, a lane its bytes t, t + 256, ... of it, so a wave never spans
// two stripes; each lane folds its bytes' row bits and eliminations, the wave
// ORs them together and one lane updates the stripe's status word.  Same
// status semantics as the lane kernels.
template <class Addr>
__device__ __forceinline__ void verify_bytes(const ecg_mm_params_t &P, uint32_t *status, Addr A)
{
	const uint64_t C = P.cell_bytes;
	const uint32_t nchunk = (uint32_t)((C + CHUNK_BYTES - 1) / CHUNK_BYTES);
	const int k = (int)P.k, rows = (int)P.rows;

	for (uint32_t s = blockIdx.y; s < P.nstripes; s += gridDim.y) {
		A.at(P, s);
		for (uint32_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
			const uint64_t cbase = (uint64_t)ch * CHUNK_BYTES;
			uint32_t rowmask = 0, elim = 0;

			for (uint64_t i = cbase + threadIdx.x; i < cbase + CHUNK_BYTES && i < C; i += BLOCK) {
				// row loops unrolled to the maximum and guarded: o[] stays
				// in registers (a runtime-indexed array would live in scratch)
				uint32_t o[ECG_KMAX_R];
				uint32_t any = 0;

#pragma unroll
				for (int r = 0; r < ECG_KMAX_R; r++)
					o[r] = r < rows ? A.par(P, r, i) : 0u;
				for (int j = 0; j < k; j++) {
					const uint32_t v = A.data(P, j, i);

#pragma unroll
					for (int r = 0; r < ECG_KMAX_R; r++)
						if (r < rows)
							o[r] ^= gf_mul1(P.tbl[r][j], v);
				}
#pragma unroll
				for (int r = 0; r < ECG_KMAX_R; r++)
					if (o[r])
						any |= 1u << r;
				if (any == 0)
					continue;
				rowmask |= any;
				for (int j = 0; j < k; j++) {
#pragma unroll
					for (int r = 1; r < ECG_KMAX_R; r++)
						if (r < rows && gf_mul1(P.tbl[0][j], o[r]) != gf_mul1(P.tbl[r][j], o[0]))
							elim |= 1u << j;
				}
			}
			if (__ballot(rowmask != 0) == 0)
				continue;
#pragma unroll
			for (int d = 32; d >= 1; d >>= 1) {
				rowmask |= (uint32_t)__shfl_xor((int)rowmask, d);
				elim |= (uint32_t)__shfl_xor((int)elim, d);
			}
			if ((threadIdx.x & 63u) == 0) {
				if (elim)
					atomicAnd(status + s, ~(elim << 8));
				atomicOr(status + s, rowmask);
			}
		}
	}
}

} // namespace

// K, R as ecg_mm_kernel's (0 = runtime-shaped).  16-byte lanes only: every
// cell address and stride 16-byte aligned, C % 16 == 0 (the launcher sends
// everything else to the byte kernel), so a partial last column is a lane
// mask and never a ragged tail.  Work mapping, table staging, phased loads of
// k = 8 and register budget are the product kernel's.
template <int K, int R>
__global__ void __launch_bounds__(BLOCK, ECG_MM_WPE(K, R, 16) ? ECG_MM_WPE(K, R, 16) : 1)
ecg_verify_kernel(const ecg_mm_params_t P, uint32_t *__restrict__ status)
{
	constexpr int KM = K ? K : ECG_KMAX_K;
	constexpr int RM = R ? R : ECG_KMAX_R;
	__shared__ u32x4 s_tbl[ECG_TBL_WORDS(KM, RM)];
	const int k = K ? K : (int)P.k;
	const int rows = R ? R : (int)P.rows;
	const uint64_t C = P.cell_bytes;
	const uint32_t nchunk = (uint32_t)((C + CHUNK_BYTES - 1) / CHUNK_BYTES);
	const uint32_t lo = lane_off<16>();

	tbl_stage<RM>(s_tbl, P, KM, k, rows);

	// one item per block; the loops only stride when a grid dimension would
	// exceed 65535
	for (uint32_t s = blockIdx.y; s < P.nstripes; s += gridDim.y) {
		for (uint32_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
			const uint64_t cbase = (uint64_t)ch * CHUNK_BYTES;
			uint32_t z = 0;
			u32x4 syn[RM];

			asm volatile("" : "+v"(z));
			const u32x4 *tb = s_tbl + z;

			if (cbase + CHUNK_BYTES <= C) {
				verify_item<KM, RM>(P, tb, k, rows, s, cbase, lo, syn);
			} else {
				// partial last column: lanes past the cell's end hold a
				// zero syndrome
#pragma unroll
				for (int r = 0; r < RM; r++)
					syn[r] = (u32x4){0u, 0u, 0u, 0u};
				if (cbase + lo + 16 <= C)
					verify_item<KM, RM>(P, tb, k, rows, s, cbase, lo, syn);
			}

			verify_fold<RM>(tb, k, rows, syn, status + s);
		}
	}
}

// The cell-table lane kernel (ecg_verify_ptrs): cells[s * (k + p) + c] = the
// address of logical cell c of stripe s, every one 16-byte aligned and
// C % 16 == 0 (the host's check: the launcher does not read the table).  Work
// mapping and table staging are ecg_mm_ptr_kernel's: one block per (column,
// stripe), a stripe's k + p addresses loaded once per stripe (wave-uniform:
// scalar loads), + cbase per column.
template <int K, int R>
__global__ void __launch_bounds__(BLOCK, ECG_MM_WPE(K, R, 16) ? ECG_MM_WPE(K, R, 16) : 1)
ecg_verify_ptr_kernel(const ecg_mm_params_t P, const uint64_t *__restrict__ cells, uint32_t *__restrict__ status)
{
	constexpr int KM = K ? K : ECG_KMAX_K;
	constexpr int RM = R ? R : ECG_KMAX_R;
	__shared__ u32x4 s_tbl[ECG_TBL_WORDS(KM, RM)];
	const int k = K ? K : (int)P.k;
	const int rows = R ? R : (int)P.rows;
	const uint64_t C = P.cell_bytes;
	const uint32_t nchunk = (uint32_t)((C + CHUNK_BYTES - 1) / CHUNK_BYTES);
	const uint32_t lo = lane_off<16>();

	tbl_stage<RM>(s_tbl, P, KM, k, rows);

	for (uint32_t s = blockIdx.y; s < P.nstripes; s += gridDim.y) {
		const uint64_t *pt = cells + (uint64_t)s * (uint32_t)(k + rows);
		uint64_t base[KM + RM];

#pragma unroll
		for (int j = 0; j < KM + RM; j++)
			if (j < k || (j >= KM && j - KM < rows))
				base[j] = pt[j < KM ? j : k + (j - KM)];
		for (uint32_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
			const uint64_t cbase = (uint64_t)ch * CHUNK_BYTES;
			uint64_t a[KM + RM];
			uint32_t z = 0;
			u32x4 syn[RM];

#pragma unroll
			for (int j = 0; j < KM + RM; j++) {
				if (j < k || (j >= KM && j - KM < rows)) {
					a[j] = base[j] + cbase;
					asm volatile("" : "+s"(a[j]));
				}
			}
			asm volatile("" : "+v"(z));
			const u32x4 *tb = s_tbl + z;

			if (cbase + CHUNK_BYTES <= C) {
				verify_ptr_item<KM, RM>(P, tb, k, rows, s, cbase, lo, a, syn);
			} else {
				// partial last column: lanes past the cell's end hold a
				// zero syndrome
#pragma unroll
				for (int r = 0; r < RM; r++)
					syn[r] = (u32x4){0u, 0u, 0u, 0u};
				if (cbase + lo + 16 <= C)
					verify_ptr_item<KM, RM>(P, tb, k, rows, s, cbase, lo, a, syn);
			}
			verify_fold<RM>(tb, k, rows, syn, status + s);
		}
	}
}

// The byte kernels (verify_bytes above): strided operands, or the cell table.
__global__ void __launch_bounds__(BLOCK)
ecg_verify_byte_kernel(const ecg_mm_params_t P, uint32_t *__restrict__ status)
{
	verify_bytes(P, status, vb_strided());
}

__global__ void __launch_bounds__(BLOCK)
ecg_verify_ptr_byte_kernel(const ecg_mm_params_t P, const uint64_t *__restrict__ cells,
			   uint32_t *__restrict__ status)
{
	verify_bytes(P, status, vb_table(cells, P.k, P.k + P.rows));
}

// The nstripes status words -> result {bad stripes, lowest bad stripe,
// attributable to one cell, not attributable} (preset {0, UINT64_MAX, 0, 0}).
__global__ void __launch_bounds__(BLOCK)
ecg_verify_summary_kernel(const uint32_t *__restrict__ status, uint32_t nstripes, int k, int p,
			  unsigned long long *result)
{
	unsigned long long bad = 0, lo = ~0ull, one = 0, many = 0;

	for (uint64_t s = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; s < nstripes; s += (uint64_t)gridDim.x * BLOCK) {
		const int c = ecg_verify_classify(status[s], k, p);

		if (c == -1)
			continue;
		bad++;
		if (s < lo)
			lo = s;
		if (c >= 0)
			one++;
		else
			many++;
	}
	if (bad) {
		atomicAdd(&result[0], bad);
		atomicMin(&result[1], lo);
		if (one)
			atomicAdd(&result[2], one);
		if (many)
			atomicAdd(&result[3], many);
	}
}

// ---------------------------------------------------------------------------
// Dispatch
// ---------------------------------------------------------------------------
typedef void (*verify_fn_t)(const ecg_mm_params_t, uint32_t *);
typedef void (*verify_pfn_t)(const ecg_mm_params_t, const uint64_t *, uint32_t *);

// one table for both layouts: the launcher reports an entry's name (strided)
// or pname (cell table)
struct ventry {
	int k, r;
	verify_fn_t fn;
	verify_pfn_t pfn;
	const char *name, *pname;
};

#define VE(K_, R_)                                                                                                     \
	{K_, R_, ecg_verify_kernel<K_, R_>, ecg_verify_ptr_kernel<K_, R_>, "ecg_verify_kernel<" #K_ "," #R_ ">",       \
	 "ecg_verify_ptr_kernel<" #K_ "," #R_ ">"}

// every (k, p) of the DAOS EC classes, as the product's; the rest runtime-shaped;
// then the byte kernels
static const ventry g_verify[] = {
	VE(2, 1), VE(2, 2), VE(2, 3),
	VE(4, 1), VE(4, 2), VE(4, 3),
	VE(8, 1), VE(8, 2), VE(8, 3),
	VE(16, 1), VE(16, 2), VE(16, 3),
	VE(0, 0),
	{-1, -1, ecg_verify_byte_kernel, ecg_verify_ptr_byte_kernel, "ecg_verify_byte_kernel",
	 "ecg_verify_ptr_byte_kernel"}};
#define N_VERIFY ((uint32_t)(sizeof(g_verify) / sizeof(g_verify[0])))
#define VERIFY_BYTE (N_VERIFY - 1)

extern "C" int ecg_k_launch_verify(const ecg_mm_params_t *p, const uint64_t *cells_dev, uint32_t *status,
				   int bytewise, const ecg_launch_cfg_t *cfg, void *stream, const char **kernel)
{
	hipStream_t st = (hipStream_t)stream;
	uint32_t gx, gy, id = VERIFY_BYTE;
	size_t lds = 0;

	if (p->nstripes == 0 || p->cell_bytes == 0 || p->rows == 0)
		return (int)hipSuccess;
	if (p->k == 0 || p->k > ECG_KMAX_K || p->rows > ECG_KMAX_R || status == nullptr)
		return (int)hipErrorInvalidValue;
	mm_grid(p, cfg, &gx, &gy);

	if (!bytewise) {
		// the lane kernels read dwordx4 at the cells' own addresses; those of a
		// cell table the host has found 16-byte aligned (the table is not read here)
		if ((cells_dev == nullptr && !aligned16(p)) || p->cell_bytes % 16u)
			return (int)hipErrorInvalidValue;
		for (id = 0; id < VERIFY_BYTE - 1; id++)	// no match: <0,0>, the last lane entry
			if (g_verify[id].k == (int)p->k && g_verify[id].r == (int)p->rows)
				break;
		lds = mm_dyn_lds(mm_wg_cap(p, cfg, (uint64_t)gx * gy), g_verify[id].k, g_verify[id].r);
	}
	if (cells_dev == nullptr)
		hipLaunchKernelGGL(g_verify[id].fn, dim3(gx, gy), dim3(BLOCK), lds, st, *p, status);
	else
		hipLaunchKernelGGL(g_verify[id].pfn, dim3(gx, gy), dim3(BLOCK), lds, st, *p, cells_dev, status);
	if (kernel)
		*kernel = cells_dev ? g_verify[id].pname : g_verify[id].name;
	return (int)hipGetLastError();
}

extern "C" int ecg_k_launch_verify_summary(const uint32_t *status, uint32_t nstripes, int k, int p,
					   uint64_t *result, void *stream)
{
	uint32_t nb = (nstripes + BLOCK - 1) / BLOCK;

	if (nstripes == 0)
		return (int)hipSuccess;
	if (nb > 1024)
		nb = 1024;
	hipLaunchKernelGGL(ecg_verify_summary_kernel, dim3(nb), dim3(BLOCK), 0, (hipStream_t)stream, status,
			   nstripes, k, p, (unsigned long long *)result);
	return (int)hipGetLastError();
}
