// ecg_update_masks_kernels.hip -- aggregation delta parity update with one
// set of updated cells per stripe (ecg_update_masks, ecg_update_masks_ptrs):
// agg_update_parity's bit_map (ref:src/object/srv_ec_aggregate.c:1006-1105) as
// a mask word per stripe in device memory, a whole batch in one launch.
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
// Two layouts, one body each for the lane and the byte kernels (um_lanes,
// um_bytes): three strided images (old, new, parity), or a table of cell
// addresses, row s = cells + s * (2k + p): k old cells, k new cells, p parity
// cells, for callers whose stripes are separate buffers (aggregation holds one
// stripe's buffers at a time).  The bodies ask an addressing struct
// (um_strided, um_table) where a stripe's cells are and share everything else;
// the __global__ entry points only choose it.
//
// A column index is the position of a set bit of a mask that has no bit at or
// above k, so every table and cell address is bounded whatever the word holds
// (and read inside the stripe's row of a cell table):
// all 2^32 mask values are safe.  A stripe's parity cells are written by the
// one block row that owns the stripe, each byte by one lane.
//
// One kernel, two grids (the launcher's choice, ECG_RM_SPARSE): grp = 1 with a
// block per column, grp = 64 with a few column blocks striding -- a clean
// batch then costs S / 64 * grid.x blocks of one load each.  Column-block 0 of
// a row counts its stripes into `result` (ecg_rows_dev.h rows_count).
//
// ecg_agg_masks / ecg_agg_masks_ptrs (the ecg_agg_masks* kernels below) take
// the same walk over the same operands and choose per stripe, by the one
// reading the host shares (ecg_kabi.h ecg_agg_route), between that delta
// update and a re-encode of the merged stripe,
//
//     parity[s][r] = XOR_{j < k} g[k+r][j] * (bit j of masks[s] ? new : old)[s][j]
//
// which walks j = 0 .. k-1 two cells at a time, each cell loaded from the one
// image its bit selects (an address select, not two loads), and stores each
// parity row without loading it: (k + p) C bytes, whatever the mask names.
// The word is wave-uniform, so the route is a scalar branch per stripe; the
// re-encode indexes j < k by construction, never by mask bits.

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

// Where a stripe's cells are -- all the strided and the cell-table kernels
// differ in.  A body positions the struct on a stripe (at), binds parity row r
// once per stripe (bind), asks per column for the row's address (par) and,
// per set bit j of the mask (the i-th in ascending order), for the addresses
// of the old and the new cell at the column's offset (pair); the re-encode of
// ecg_agg_masks asks for cell j of one image (cell).

// Three strided images: every address is arithmetic on the stripe's three
// bases, done per column, so nothing is bound.
// The launch's bases and strides are held by value (read once, in front of
// the row loop, where the kernel written without the struct read them).
struct um_strided {
	const uint8_t *src, *src2;
	uint8_t *dst;
	int64_t ss, s2s, ds;
	const int64_t *doff;
	uint64_t C;
	uint32_t packed;
	const uint8_t *ob, *nb;
	uint8_t *pb;

	__device__ um_strided(const ecg_mm_params_t &P, uint32_t packed_)
		: src(P.src), src2(P.src2), dst(P.dst), ss(P.src_stripe_stride), s2s(P.src2_stripe_stride),
		  ds(P.dst_stripe_stride), doff(P.dst_cell_off), C(P.cell_bytes), packed(packed_) {}
	__device__ void at(uint32_t s)
	{
		ob = src + (int64_t)s * ss;
		nb = src2 + (int64_t)s * s2s;
		pb = dst + (int64_t)s * ds;
	}
	__device__ void bind(int) {}
	__device__ uint8_t *par(int r) const { return pb + doff[r]; }
	__device__ void pair(uint32_t i, uint32_t j, uint64_t off, const uint8_t **o, const uint8_t **n) const
	{
		const uint64_t c = um_cell(packed, i, j, C) + off;

		*o = ob + c;
		*n = nb + c;
	}
	// cell j (unpacked) of one image, the new one with fromnew
	__device__ const uint8_t *cell(uint32_t j, uint32_t fromnew, uint64_t off) const
	{
		return (fromnew ? nb : ob) + (uint64_t)j * C + off;
	}
};

// The stripe's row pt of a cell table: old cell j = pt[j], new cell j =
// pt[k + j], parity row r = pt[2k + r].  Wave-uniform: the stripe index and
// the mask word come from a readlane, so these are scalar loads of a read-only
// table.  The RM parity addresses are bound once per stripe, before the column
// loop; the two addresses of a named cell are loaded per set bit inside it,
// which keeps the registers flat (up to 16 named cells would be 64 SGPRs bound)
// and costs the dense grid nothing: there a block takes one column of a stripe.
template <int RM>
struct um_table {
	const uint64_t *__restrict__ cells;
	uint32_t k, n;	// n = 2k + p
	const uint64_t *__restrict__ pt;
	uint64_t slot[RM];	// those bound, the rest left unset

	__device__ um_table(const uint64_t *cells_, uint32_t k_, uint32_t p_) : cells(cells_), k(k_), n(2u * k_ + p_) {}
	__device__ void at(uint32_t s) { pt = cells + (uint64_t)s * n; }
	__device__ void bind(int r) { slot[r] = pt[2u * k + (uint32_t)r]; }
	__device__ uint8_t *par(int r) const { return reinterpret_cast<uint8_t *>(slot[r]); }
	__device__ void pair(uint32_t, uint32_t j, uint64_t off, const uint8_t **o, const uint8_t **n_) const
	{
		*o = reinterpret_cast<const uint8_t *>(pt[j]) + off;
		*n_ = reinterpret_cast<const uint8_t *>(pt[k + j]) + off;
	}
	// one entry of the row: the old or the new cell j, j < k
	__device__ const uint8_t *cell(uint32_t j, uint32_t fromnew, uint64_t off) const
	{
		return reinterpret_cast<const uint8_t *>(pt[(fromnew ? k : 0u) + j]) + off;
	}
};

// um_lanes' walk of a mask's set bits as a function, for ag_lanes: acc[r] ^=
// tbl[r][j] * (old_j ^ new_j) at a lane's 16 bytes `off` of a column, two bits
// at a time -- four cell loads in flight.  (um_lanes keeps the loop in its
// body: calling this from there changes the SGPR figures of
// ecg_update_masks_kernel, which stay those of the kernels as they were.)
template <int RM, class Addr>
__device__ __forceinline__ void um_delta(const Addr &A, const u32x4 *s_tbl, int rows, uint32_t m, uint64_t off,
					 u32x4 *acc)
{
	using TB = mm_tbl<RM>;

	for (uint32_t mm = m, i = 0; mm; i += 2) {
		const uint32_t j0 = (uint32_t)__builtin_ctz(mm);
		const uint8_t *o0, *n0, *o1, *n1;

		A.pair(i, j0, off, &o0, &n0);
		const u32x4 x0 = ld_g<16>(o0) ^ ld_g<16>(n0);
		u32x4 x1 = (u32x4){0u, 0u, 0u, 0u};
		uint32_t j1 = 0;

		mm &= mm - 1u;
		const bool two = mm != 0;
		if (two) {
			j1 = (uint32_t)__builtin_ctz(mm);
			mm &= mm - 1u;
			A.pair(i + 1u, j1, off, &o1, &n1);
			x1 = ld_g<16>(o1) ^ ld_g<16>(n1);
		}
		// (the unsigned bit index times PER_J, not TB::cell's int:
		// that one folds into another scalar sequence)
		upd_fold<RM>(s_tbl + j0 * TB::PER_J, rows, x0, acc);
		if (two)
			upd_fold<RM>(s_tbl + j1 * TB::PER_J, rows, x1, acc);
	}
}

// The merged stripe's column at the same 16 bytes: acc[r] ^= tbl[r][j] * (bit j
// of m ? new_j : old_j) over every j < k, two cell loads in flight.
template <int RM, class Addr>
__device__ __forceinline__ void ag_recalc(const Addr &A, const u32x4 *s_tbl, int k, int rows, uint32_t m,
					  uint64_t off, u32x4 *acc)
{
	using TB = mm_tbl<RM>;

	for (uint32_t j = 0; j < (uint32_t)k; j += 2) {
		const u32x4 x0 = ld_g<16>(A.cell(j, (m >> j) & 1u, off));
		u32x4 x1 = (u32x4){0u, 0u, 0u, 0u};
		const bool two = j + 1u < (uint32_t)k;

		if (two)
			x1 = ld_g<16>(A.cell(j + 1u, (m >> (j + 1u)) & 1u, off));
		upd_fold<RM>(s_tbl + j * TB::PER_J, rows, x0, acc);
		if (two)
			upd_fold<RM>(s_tbl + (j + 1u) * TB::PER_J, rows, x1, acc);
	}
}

// The lane kernels' body.  R = p parity rows (1..3 specialised; 0 =
// runtime-shaped, 4..8 rows).  16-byte lanes only: every cell address (strided:
// every operand and stride) and C a 16-byte multiple (the launcher sends
// everything else to the byte kernel), so a partial last column is a lane
// mask.  s_tbl: the block's ECG_TBL_WORDS(ECG_KMAX_K, RM) staged table words.
template <int R, class Addr>
__device__ __forceinline__ void um_lanes(const ecg_mm_params_t &P, u32x4 *s_tbl, const uint32_t *__restrict__ masks,
					 unsigned long long *result, uint32_t grp, Addr A)
{
	constexpr int RM = R ? R : ECG_KMAX_R;
	using TB = mm_tbl<RM>;
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

			A.at(s);
#pragma unroll
			for (int r = 0; r < RM; r++)
				if (r < rows)
					A.bind(r);

			for (uint32_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
				const uint64_t off = (uint64_t)ch * CHUNK_BYTES + lo;
				u32x4 acc[RM];

				// a partial last column is a lane mask (C % 16 == 0 here)
				if (off + 16 > C)
					continue;
#pragma unroll
				for (int r = 0; r < RM; r++)
					if (r < rows)
						acc[r] = ld_g<16>(A.par(r) + off);
				for (uint32_t mm = m, i = 0; mm; i += 2) {
					const uint32_t j0 = (uint32_t)__builtin_ctz(mm);
					const uint8_t *o0, *n0, *o1, *n1;

					A.pair(i, j0, off, &o0, &n0);
					const u32x4 x0 = ld_g<16>(o0) ^ ld_g<16>(n0);
					u32x4 x1 = (u32x4){0u, 0u, 0u, 0u};
					uint32_t j1 = 0;

					mm &= mm - 1u;
					const bool two = mm != 0;
					if (two) {
						j1 = (uint32_t)__builtin_ctz(mm);
						mm &= mm - 1u;
						A.pair(i + 1u, j1, off, &o1, &n1);
						x1 = ld_g<16>(o1) ^ ld_g<16>(n1);
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
						st_g<16>(A.par(r) + off, acc[r]);
			}
		}
	}
}

// The byte kernels' body.  Any alignment, any length, any p <= 8: a block
// takes 4 KiB columns of one stripe at a time, a lane the bytes t, t + 256, ...
// of a column.  Same scan and counters as the lane body; the tables are read
// where they lie.
template <class Addr>
__device__ __forceinline__ void um_bytes(const ecg_mm_params_t &P, const uint32_t *__restrict__ masks,
					 unsigned long long *result, uint32_t grp, Addr A)
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

			A.at(s);
#pragma unroll
			for (int r = 0; r < ECG_KMAX_R; r++)
				if (r < rows)
					A.bind(r);

			for (uint32_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
				const uint64_t cbase = (uint64_t)ch * CHUNK_BYTES;

				for (uint64_t b = cbase + threadIdx.x; b < cbase + CHUNK_BYTES && b < C; b += BLOCK) {
					uint32_t o[ECG_KMAX_R];

					for (int r = 0; r < ECG_KMAX_R; r++)
						o[r] = 0;
					for (uint32_t mm = m, i = 0; mm; mm &= mm - 1u, i++) {
						const uint32_t j = (uint32_t)__builtin_ctz(mm);
						const uint8_t *oc, *nc;

						A.pair(i, j, b, &oc, &nc);
						const uint32_t v = (uint32_t)*oc ^ (uint32_t)*nc;

#pragma unroll
						for (int r = 0; r < ECG_KMAX_R; r++)
							if (r < rows)
								o[r] ^= gf_mul1(P.tbl[r][j], v);
					}
#pragma unroll
					for (int r = 0; r < ECG_KMAX_R; r++)
						if (r < rows)
							A.par(r)[b] ^= (uint8_t)o[r];
				}
			}
		}
	}
}

// ---------------------------------------------------------------------------
// ecg_agg_masks: the same walk, the route chosen per stripe (ecg_kabi.h
// ecg_agg_route; T = the threshold, a kernel argument).  um_read accepts and
// counts a stripe whichever route it takes.
// ---------------------------------------------------------------------------
template <int R, class Addr>
__device__ __forceinline__ void ag_lanes(const ecg_mm_params_t &P, u32x4 *s_tbl, const uint32_t *__restrict__ masks,
					 unsigned long long *result, uint32_t grp, uint32_t T, Addr A)
{
	constexpr int RM = R ? R : ECG_KMAX_R;
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
			// wave-uniform: a scalar branch per stripe
			const bool recalc = ecg_agg_route(m, k, T) == ECG_AGG_RECALC;

			A.at(s);
#pragma unroll
			for (int r = 0; r < RM; r++)
				if (r < rows)
					A.bind(r);

			for (uint32_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
				const uint64_t off = (uint64_t)ch * CHUNK_BYTES + lo;
				u32x4 acc[RM];

				// a partial last column is a lane mask (C % 16 == 0 here)
				if (off + 16 > C)
					continue;
				if (recalc) {
					// the old parity is not read
#pragma unroll
					for (int r = 0; r < RM; r++)
						acc[r] = (u32x4){0u, 0u, 0u, 0u};
					ag_recalc<RM>(A, s_tbl, k, rows, m, off, acc);
				} else {
#pragma unroll
					for (int r = 0; r < RM; r++)
						if (r < rows)
							acc[r] = ld_g<16>(A.par(r) + off);
					um_delta<RM>(A, s_tbl, rows, m, off, acc);
				}
#pragma unroll
				for (int r = 0; r < RM; r++)
					if (r < rows)
						st_g<16>(A.par(r) + off, acc[r]);
			}
		}
	}
}

// The byte body: um_bytes' walk; a re-encoded stripe's parity bytes are
// written (=) where the delta's are folded in (^=).
template <class Addr>
__device__ __forceinline__ void ag_bytes(const ecg_mm_params_t &P, const uint32_t *__restrict__ masks,
					 unsigned long long *result, uint32_t grp, uint32_t T, Addr A)
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
			const bool recalc = ecg_agg_route(m, k, T) == ECG_AGG_RECALC;

			A.at(s);
#pragma unroll
			for (int r = 0; r < ECG_KMAX_R; r++)
				if (r < rows)
					A.bind(r);

			for (uint32_t ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
				const uint64_t cbase = (uint64_t)ch * CHUNK_BYTES;

				for (uint64_t b = cbase + threadIdx.x; b < cbase + CHUNK_BYTES && b < C; b += BLOCK) {
					uint32_t o[ECG_KMAX_R];

					for (int r = 0; r < ECG_KMAX_R; r++)
						o[r] = 0;
					if (recalc) {
						for (uint32_t j = 0; j < (uint32_t)k; j++) {
							const uint32_t v = *A.cell(j, (m >> j) & 1u, b);

#pragma unroll
							for (int r = 0; r < ECG_KMAX_R; r++)
								if (r < rows)
									o[r] ^= gf_mul1(P.tbl[r][j], v);
						}
#pragma unroll
						for (int r = 0; r < ECG_KMAX_R; r++)
							if (r < rows)
								A.par(r)[b] = (uint8_t)o[r];
						continue;
					}
					for (uint32_t mm = m, i = 0; mm; mm &= mm - 1u, i++) {
						const uint32_t j = (uint32_t)__builtin_ctz(mm);
						const uint8_t *oc, *nc;

						A.pair(i, j, b, &oc, &nc);
						const uint32_t v = (uint32_t)*oc ^ (uint32_t)*nc;

#pragma unroll
						for (int r = 0; r < ECG_KMAX_R; r++)
							if (r < rows)
								o[r] ^= gf_mul1(P.tbl[r][j], v);
					}
#pragma unroll
					for (int r = 0; r < ECG_KMAX_R; r++)
						if (r < rows)
							A.par(r)[b] ^= (uint8_t)o[r];
				}
			}
		}
	}
}

} // namespace

// The entry points: the strided images P.src / P.src2 / P.dst
// (ecg_update_masks), or the table `cells` (ecg_update_masks_ptrs).
template <int R>
__global__ void __launch_bounds__(BLOCK)
ecg_update_masks_kernel(const ecg_mm_params_t P, const uint32_t *__restrict__ masks, unsigned long long *result,
			uint32_t grp, uint32_t packed)
{
	__shared__ u32x4 s_tbl[ECG_TBL_WORDS(ECG_KMAX_K, R ? R : ECG_KMAX_R)];

	um_lanes<R>(P, s_tbl, masks, result, grp, um_strided(P, packed));
}

__global__ void __launch_bounds__(BLOCK)
ecg_update_masks_byte_kernel(const ecg_mm_params_t P, const uint32_t *__restrict__ masks,
			     unsigned long long *result, uint32_t grp, uint32_t packed)
{
	um_bytes(P, masks, result, grp, um_strided(P, packed));
}

template <int R>
__global__ void __launch_bounds__(BLOCK)
ecg_update_masks_ptr_kernel(const ecg_mm_params_t P, const uint64_t *__restrict__ cells,
			    const uint32_t *__restrict__ masks, unsigned long long *result, uint32_t grp)
{
	__shared__ u32x4 s_tbl[ECG_TBL_WORDS(ECG_KMAX_K, R ? R : ECG_KMAX_R)];

	um_lanes<R>(P, s_tbl, masks, result, grp, um_table<R ? R : ECG_KMAX_R>(cells, P.k, R ? R : P.rows));
}

__global__ void __launch_bounds__(BLOCK)
ecg_update_masks_ptr_byte_kernel(const ecg_mm_params_t P, const uint64_t *__restrict__ cells,
				 const uint32_t *__restrict__ masks, unsigned long long *result, uint32_t grp)
{
	um_bytes(P, masks, result, grp, um_table<ECG_KMAX_R>(cells, P.k, P.rows));
}

// ecg_agg_masks / ecg_agg_masks_ptrs: the same two layouts (never packed: the
// re-encode needs the unnamed old cells in their slots).
template <int R>
__global__ void __launch_bounds__(BLOCK)
ecg_agg_masks_kernel(const ecg_mm_params_t P, const uint32_t *__restrict__ masks, unsigned long long *result,
		     uint32_t grp, uint32_t T)
{
	__shared__ u32x4 s_tbl[ECG_TBL_WORDS(ECG_KMAX_K, R ? R : ECG_KMAX_R)];

	ag_lanes<R>(P, s_tbl, masks, result, grp, T, um_strided(P, 0));
}

__global__ void __launch_bounds__(BLOCK)
ecg_agg_masks_byte_kernel(const ecg_mm_params_t P, const uint32_t *__restrict__ masks, unsigned long long *result,
			  uint32_t grp, uint32_t T)
{
	ag_bytes(P, masks, result, grp, T, um_strided(P, 0));
}

template <int R>
__global__ void __launch_bounds__(BLOCK)
ecg_agg_masks_ptr_kernel(const ecg_mm_params_t P, const uint64_t *__restrict__ cells,
			 const uint32_t *__restrict__ masks, unsigned long long *result, uint32_t grp, uint32_t T)
{
	__shared__ u32x4 s_tbl[ECG_TBL_WORDS(ECG_KMAX_K, R ? R : ECG_KMAX_R)];

	ag_lanes<R>(P, s_tbl, masks, result, grp, T, um_table<R ? R : ECG_KMAX_R>(cells, P.k, R ? R : P.rows));
}

__global__ void __launch_bounds__(BLOCK)
ecg_agg_masks_ptr_byte_kernel(const ecg_mm_params_t P, const uint64_t *__restrict__ cells,
			      const uint32_t *__restrict__ masks, unsigned long long *result, uint32_t grp, uint32_t T)
{
	ag_bytes(P, masks, result, grp, T, um_table<ECG_KMAX_R>(cells, P.k, P.rows));
}

// ---------------------------------------------------------------------------
// Dispatch: one table for both layouts and both calls.  The lane
// instantiations, then the byte kernels; a launcher reports an entry's name
// (strided) or pname (cell table), ecg_k_launch_agg_masks its aname / apname.
// ---------------------------------------------------------------------------
// the last argument: `packed` of the update kernels, T of the agg kernels
typedef void (*um_fn_t)(const ecg_mm_params_t, const uint32_t *, unsigned long long *, uint32_t, uint32_t);
typedef void (*ump_fn_t)(const ecg_mm_params_t, const uint64_t *, const uint32_t *, unsigned long long *, uint32_t);
typedef void (*agp_fn_t)(const ecg_mm_params_t, const uint64_t *, const uint32_t *, unsigned long long *, uint32_t,
			 uint32_t);

struct umentry {
	int r;
	um_fn_t fn;
	ump_fn_t pfn;
	const char *name, *pname;
	um_fn_t afn;
	agp_fn_t apfn;
	const char *aname, *apname;
};

#define UME(R_)                                                                                                        \
	{R_, ecg_update_masks_kernel<R_>, ecg_update_masks_ptr_kernel<R_>, "ecg_update_masks_kernel<" #R_ ">",        \
	 "ecg_update_masks_ptr_kernel<" #R_ ">", ecg_agg_masks_kernel<R_>, ecg_agg_masks_ptr_kernel<R_>,              \
	 "ecg_agg_masks_kernel<" #R_ ">", "ecg_agg_masks_ptr_kernel<" #R_ ">"}

// the DAOS classes' p = 1..3 specialised, 4..8 parity rows runtime-shaped
static const umentry g_um[] = {UME(1), UME(2), UME(3), UME(0),
			       {-1, ecg_update_masks_byte_kernel, ecg_update_masks_ptr_byte_kernel,
				"ecg_update_masks_byte_kernel", "ecg_update_masks_ptr_byte_kernel",
				ecg_agg_masks_byte_kernel, ecg_agg_masks_ptr_byte_kernel, "ecg_agg_masks_byte_kernel",
				"ecg_agg_masks_ptr_byte_kernel"}};
#define N_UM ((uint32_t)(sizeof(g_um) / sizeof(g_um[0])))
#define UM_BYTE (N_UM - 1)

// What both launchers check and choose: the operands, the grid and its block
// rows of *grp stripes, and the entry *id of g_um.
static hipError_t um_plan(const ecg_mm_params_t *p, const uint64_t *cells_dev, const uint32_t *masks,
			  const uint64_t *result, int packed, int bytewise, int sparse, const ecg_launch_cfg_t *cfg,
			  uint32_t *grp, uint32_t *gx, uint32_t *gy, uint32_t *id)
{
	if (p->k == 0 || p->k > ECG_KMAX_K || p->rows == 0 || p->rows > ECG_KMAX_R || masks == nullptr ||
	    result == nullptr)
		return hipErrorInvalidValue;
	if (cells_dev == nullptr && (p->src == nullptr || p->src2 == nullptr || p->dst == nullptr ||
				     p->src_stripe_stride != p->src2_stripe_stride))
		return hipErrorInvalidValue;
	if (cells_dev != nullptr && packed)	// a table has an address in slot j
		return hipErrorInvalidValue;
	*grp = sparse ? 64u : ECG_RM_DENSE_GRP;
	rows_grid(p, *grp, sparse ? ECG_REPAIR_GRID_X : ECG_RM_DENSE_GRID_X, cfg, gx, gy);

	*id = UM_BYTE;
	if (!bytewise) {
		// the lane kernel reads and writes dwordx4 at the cells' own addresses;
		// those of a cell table the host has found 16-byte aligned (the table
		// is not read here)
		uint64_t al = p->cell_bytes;

		if (cells_dev == nullptr) {
			al |= (uint64_t)(uintptr_t)p->src | (uint64_t)(uintptr_t)p->src2 | (uint64_t)(uintptr_t)p->dst |
			      (uint64_t)p->src_stripe_stride | (uint64_t)p->dst_stripe_stride;
			for (uint32_t r = 0; r < p->rows; r++)
				al |= (uint64_t)p->dst_cell_off[r];
		}
		if ((al & 15u) != 0)
			return hipErrorInvalidValue;
		for (*id = 0; *id < UM_BYTE; (*id)++)
			if (g_um[*id].r == (int)p->rows || g_um[*id].r == 0)
				break;
		if (*id == UM_BYTE)
			return hipErrorInvalidValue;
	}
	return hipSuccess;
}

extern "C" int ecg_k_launch_update_masks(const ecg_mm_params_t *p, const uint64_t *cells_dev, const uint32_t *masks,
					 uint64_t *result, int packed, int bytewise, int sparse,
					 const ecg_launch_cfg_t *cfg, void *stream, const char **kernel)
{
	hipStream_t st = (hipStream_t)stream;
	uint32_t grp, gx, gy, id;

	if (p->nstripes == 0 || p->cell_bytes == 0)
		return (int)hipSuccess;
	const hipError_t e = um_plan(p, cells_dev, masks, result, packed, bytewise, sparse, cfg, &grp, &gx, &gy, &id);

	if (e != hipSuccess)
		return (int)e;
	if (cells_dev == nullptr)
		hipLaunchKernelGGL(g_um[id].fn, dim3(gx, gy), dim3(BLOCK), 0, st, *p, masks, (unsigned long long *)result,
				   grp, (uint32_t)(packed != 0));
	else
		hipLaunchKernelGGL(g_um[id].pfn, dim3(gx, gy), dim3(BLOCK), 0, st, *p, cells_dev, masks,
				   (unsigned long long *)result, grp);
	if (kernel)
		*kernel = cells_dev ? g_um[id].pname : g_um[id].name;
	return (int)hipGetLastError();
}

// ecg_agg_masks / ecg_agg_masks_ptrs (declared in host/ecg_internal.h): the
// update's operands, never packed, and the threshold T = recalc_above <= k.
extern "C" int ecg_k_launch_agg_masks(const ecg_mm_params_t *p, const uint64_t *cells_dev, const uint32_t *masks,
				      uint64_t *result, uint32_t recalc_above, int bytewise, int sparse,
				      const ecg_launch_cfg_t *cfg, void *stream, const char **kernel)
{
	hipStream_t st = (hipStream_t)stream;
	uint32_t grp, gx, gy, id;

	if (p->nstripes == 0 || p->cell_bytes == 0)
		return (int)hipSuccess;
	if (recalc_above > p->k)
		return (int)hipErrorInvalidValue;
	const hipError_t e = um_plan(p, cells_dev, masks, result, 0, bytewise, sparse, cfg, &grp, &gx, &gy, &id);

	if (e != hipSuccess)
		return (int)e;
	if (cells_dev == nullptr)
		hipLaunchKernelGGL(g_um[id].afn, dim3(gx, gy), dim3(BLOCK), 0, st, *p, masks, (unsigned long long *)result,
				   grp, recalc_above);
	else
		hipLaunchKernelGGL(g_um[id].apfn, dim3(gx, gy), dim3(BLOCK), 0, st, *p, cells_dev, masks,
				   (unsigned long long *)result, grp, recalc_above);
	if (kernel)
		*kernel = cells_dev ? g_um[id].apname : g_um[id].aname;
	return (int)hipGetLastError();
}
