// ecg_update_masks_kernels.hip -- aggregation delta parity update with one
// set of updated cells per stripe (ecg_update_masks): agg_update_parity's
// bit_map (ref:src/object/srv_ec_aggregate.c:1006-1105) as a mask word per
// stripe in device memory, a whole batch in one launch.
//
//     parity[s][r] ^= XOR_{j in masks[s]} g[k+r][j] * (old[s][j] ^ new[s][j])
//
// A block row takes `grp` consecutive stripes (1 .. 64) and walks them as
// every mask-driven kernel does (ecg_rows_dev.h rows_scan / rows_next): a lane
// reads a stripe's mask word with the one reading the host shares (ecg_kabi.h
// ecg_update_mask_read), and a ballot leaves the stripes with work as a
// wave-uniform 64-bit mask.  The perm tables of all k columns x p rows do not
// depend on the stripe: they are staged into LDS once per block (ecg_mm_dev.h
// tbl_stage; the layout: ecg_kabi.h ECG_TBL_PER_J).  Per 4 KiB
// column a lane loads its 16 bytes of every parity row first, then walks the
// mask's set bits two at a time -- four cell loads in flight -- folding each
// delta into the rows (ecg_mm_dev.h upd_fold), and stores each parity row
// once: (2 n + 2 p) C bytes per stripe of n changed cells.
//
// A column index is the position of a set bit of a mask that has no bit at or
// above k, so every table and cell address is bounded whatever the word holds:
// all 2^32 mask values are safe.  A stripe's parity cells are written by the
// one block row that owns the stripe, each byte by one lane.
//
// One kernel, two grids (the launcher's choice, ECG_RM_SPARSE): grp = 1 with a
// block per column, grp = 64 with a few column blocks striding -- a clean
// batch then costs S / 64 * grid.x blocks of one load each.  Column-block 0 of
// a row counts its stripes into `result` (ecg_rows_dev.h rows_count).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../ecg_kabi.h"
#include "ecg_mm_dev.h"
#include "ecg_rows_dev.h"

namespace {

// The reader of a mask word (ecg_rows_dev.h): the word itself when it names
// 1 .. k cells, refused with a bit at or above k; an applied cell is the
// call's unit.
struct um_read {
	const uint32_t *__restrict__ masks;
	int k;
	static constexpr uint32_t none = 0;

	__device__ uint32_t load(uint64_t s) const { return masks[s]; }
	__device__ int verdict(uint32_t m) const
	{
		const int n = ecg_update_mask_read(m, k);

		return rows_verdict(n == ECG_UM_NONE, n > 0);
	}
	__device__ unsigned long long units(uint32_t m) const { return ecg_update_mask_read(m, k); }
};

// byte offset of the cell of column j, the i-th set bit of its mask, from the
// stripe's old / new base
__device__ __forceinline__ uint64_t um_cell(uint32_t packed, uint32_t i, uint32_t j, uint64_t C)
{
	return (uint64_t)(packed ? i : j) * C;
}

} // namespace

// R = p parity rows (1..3 specialised; 0 = runtime-shaped, 4..8 rows).
// 16-byte lanes only: every operand, stride and C a 16-byte multiple (the
// launcher sends everything else to the byte kernel), so a partial last
// column is a lane mask.
template <int R>
__global__ void __launch_bounds__(BLOCK)
ecg_update_masks_kernel(const ecg_mm_params_t P, const uint32_t *__restrict__ masks, unsigned long long *result,
			uint32_t grp, uint32_t packed)
{
	constexpr int RM = R ? R : ECG_KMAX_R;
	using TB = mm_tbl<RM>;
	__shared__ u32x4 s_tbl[ECG_TBL_WORDS(ECG_KMAX_K, RM)];
	const int k = (int)P.k;
	const int rows = R ? R : (int)P.rows;
	const uint64_t C = P.cell_bytes;
	const uint32_t nchunk = (uint32_t)((C + CHUNK_BYTES - 1) / CHUNK_BYTES);
	const uint32_t lo = lane_off<16>();
	const uint32_t nrow = rows_count_rows(P.nstripes, grp);
	const um_read read = {masks, k};

	tbl_stage<RM>(s_tbl, P, ECG_KMAX_K, k, rows);

	for (uint32_t row = blockIdx.y; row < nrow; row += gridDim.y) {
		uint32_t mw, m;
		uint64_t todo = rows_scan(P.nstripes, row, grp, result, read, &mw);

		while (todo) {
			const uint32_t s = rows_next(&todo, row, grp, mw, &m);
			const uint8_t *ob = P.src + (int64_t)s * P.src_stripe_stride;
			const uint8_t *nb = P.src2 + (int64_t)s * P.src2_stripe_stride;
			uint8_t *pb = P.dst + (int64_t)s * P.dst_stripe_stride;

			for (uint32_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
				const uint64_t off = (uint64_t)ch * CHUNK_BYTES + lo;
				u32x4 acc[RM];

				// a partial last column is a lane mask (C % 16 == 0 here)
				if (off + 16 > C)
					continue;
#pragma unroll
				for (int r = 0; r < RM; r++)
					if (r < rows)
						acc[r] = ld_g<16>(pb + P.dst_cell_off[r] + off);
				for (uint32_t mm = m, i = 0; mm; i += 2) {
					const uint32_t j0 = (uint32_t)__builtin_ctz(mm);
					const uint64_t c0 = um_cell(packed, i, j0, C) + off;
					const u32x4 x0 = ld_g<16>(ob + c0) ^ ld_g<16>(nb + c0);
					u32x4 x1 = (u32x4){0u, 0u, 0u, 0u};
					uint32_t j1 = 0;

					mm &= mm - 1u;
					const bool two = mm != 0;
					if (two) {
						j1 = (uint32_t)__builtin_ctz(mm);
						mm &= mm - 1u;
						const uint64_t c1 = um_cell(packed, i + 1u, j1, C) + off;
						x1 = ld_g<16>(ob + c1) ^ ld_g<16>(nb + c1);
					}
					// (the unsigned bit index times PER_J, not TB::cell's int:
					// that one folds into another scalar sequence)
					upd_fold<RM>(s_tbl + j0 * TB::PER_J, rows, x0, acc);
					if (two)
						upd_fold<RM>(s_tbl + j1 * TB::PER_J, rows, x1, acc);
				}
#pragma unroll
				for (int r = 0; r < RM; r++)
					if (r < rows)
						st_g<16>(pb + P.dst_cell_off[r] + off, acc[r]);
			}
		}
	}
}

// Any alignment, any length, any p <= 8: a block takes 4 KiB columns of one
// stripe at a time, a lane the bytes t, t + 256, ... of a column.  Same scan
// and counters as the lane kernel; the tables are read where they lie.
__global__ void __launch_bounds__(BLOCK)
ecg_update_masks_byte_kernel(const ecg_mm_params_t P, const uint32_t *__restrict__ masks,
			     unsigned long long *result, uint32_t grp, uint32_t packed)
{
	const uint64_t C = P.cell_bytes;
	const uint32_t nchunk = (uint32_t)((C + CHUNK_BYTES - 1) / CHUNK_BYTES);
	const int k = (int)P.k, rows = (int)P.rows;
	const uint32_t nrow = rows_count_rows(P.nstripes, grp);
	const um_read read = {masks, k};

	for (uint32_t row = blockIdx.y; row < nrow; row += gridDim.y) {
		uint32_t mw, m;
		uint64_t todo = rows_scan(P.nstripes, row, grp, result, read, &mw);

		while (todo) {
			const uint32_t s = rows_next(&todo, row, grp, mw, &m);
			const uint8_t *ob = P.src + (int64_t)s * P.src_stripe_stride;
			const uint8_t *nb = P.src2 + (int64_t)s * P.src2_stripe_stride;
			uint8_t *pb = P.dst + (int64_t)s * P.dst_stripe_stride;

			for (uint32_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
				const uint64_t cbase = (uint64_t)ch * CHUNK_BYTES;

				for (uint64_t b = cbase + threadIdx.x; b < cbase + CHUNK_BYTES && b < C; b += BLOCK) {
					uint32_t o[ECG_KMAX_R];

					for (int r = 0; r < ECG_KMAX_R; r++)
						o[r] = 0;
					for (uint32_t mm = m, i = 0; mm; mm &= mm - 1u, i++) {
						const uint32_t j = (uint32_t)__builtin_ctz(mm);
						const uint64_t c = um_cell(packed, i, j, C) + b;
						const uint32_t v = (uint32_t)ob[c] ^ (uint32_t)nb[c];

#pragma unroll
						for (int r = 0; r < ECG_KMAX_R; r++)
							if (r < rows)
								o[r] ^= gf_mul1(P.tbl[r][j], v);
					}
#pragma unroll
					for (int r = 0; r < ECG_KMAX_R; r++)
						if (r < rows)
							pb[P.dst_cell_off[r] + (int64_t)b] ^= (uint8_t)o[r];
				}
			}
		}
	}
}

// ---------------------------------------------------------------------------
// Dispatch
// ---------------------------------------------------------------------------
typedef void (*um_fn_t)(const ecg_mm_params_t, const uint32_t *, unsigned long long *, uint32_t, uint32_t);

struct umentry {
	int r;
	um_fn_t fn;
	const char *name;
};

#define UME(R_) {R_, ecg_update_masks_kernel<R_>, "ecg_update_masks_kernel<" #R_ ">"}

// the DAOS classes' p = 1..3 specialised, 4..8 parity rows runtime-shaped
static const umentry g_um[] = {UME(1), UME(2), UME(3), UME(0)};
#define N_UM ((uint32_t)(sizeof(g_um) / sizeof(g_um[0])))
#define KID_UM_BYTE (ECG_KID_UPDATE_MASKS + N_UM)

extern "C" const char *ecg_k_update_masks_kernel_name(uint32_t id)
{
	if (id >= ECG_KID_UPDATE_MASKS && id < ECG_KID_UPDATE_MASKS + N_UM)
		return g_um[id - ECG_KID_UPDATE_MASKS].name;
	if (id == KID_UM_BYTE)
		return "ecg_update_masks_byte_kernel";
	return "?";
}

extern "C" int ecg_k_launch_update_masks(const ecg_mm_params_t *p, const uint32_t *masks, uint64_t *result,
					 int packed, int bytewise, int sparse, const ecg_launch_cfg_t *cfg,
					 void *stream, uint32_t *kernel_id)
{
	hipStream_t st = (hipStream_t)stream;
	uint32_t gx, gy;

	if (p->nstripes == 0 || p->cell_bytes == 0)
		return (int)hipSuccess;
	if (p->k == 0 || p->k > ECG_KMAX_K || p->rows == 0 || p->rows > ECG_KMAX_R || masks == nullptr ||
	    result == nullptr || p->src == nullptr || p->src2 == nullptr || p->dst == nullptr ||
	    p->src_stripe_stride != p->src2_stripe_stride)
		return (int)hipErrorInvalidValue;
	const uint32_t grp = sparse ? 64u : ECG_RM_DENSE_GRP;

	rows_grid(p, grp, sparse ? ECG_REPAIR_GRID_X : ECG_RM_DENSE_GRID_X, cfg, &gx, &gy);

	if (bytewise) {
		hipLaunchKernelGGL(ecg_update_masks_byte_kernel, dim3(gx, gy), dim3(BLOCK), 0, st, *p, masks,
				   (unsigned long long *)result, grp, (uint32_t)(packed != 0));
		if (kernel_id)
			*kernel_id = KID_UM_BYTE;
		return (int)hipGetLastError();
	}
	// the lane kernel reads and writes dwordx4 at the cells' own addresses
	uint64_t al = (uint64_t)(uintptr_t)p->src | (uint64_t)(uintptr_t)p->src2 | (uint64_t)(uintptr_t)p->dst |
		      (uint64_t)p->src_stripe_stride | (uint64_t)p->dst_stripe_stride | p->cell_bytes;
	for (uint32_t r = 0; r < p->rows; r++)
		al |= (uint64_t)p->dst_cell_off[r];
	if ((al & 15u) != 0)
		return (int)hipErrorInvalidValue;

	uint32_t id = N_UM;
	for (uint32_t i = 0; i < N_UM && id == N_UM; i++)
		if (g_um[i].r == (int)p->rows || g_um[i].r == 0)
			id = i;
	hipLaunchKernelGGL(g_um[id].fn, dim3(gx, gy), dim3(BLOCK), 0, st, *p, masks, (unsigned long long *)result,
			   grp, (uint32_t)(packed != 0));
	if (kernel_id)
		*kernel_id = ECG_KID_UPDATE_MASKS + id;
	return (int)hipGetLastError();
}
