// ecg_rows_dev.h -- the walk the mask-driven kernels share (ecg_repair,
// ecg_recover_masks, ecg_update_masks): one 32-bit word per stripe, in device
// memory, says what a stripe needs.  A block row takes `grp` consecutive
// stripes (1 .. 64): rows_scan reads their words, one per lane, and a ballot
// leaves the stripes with work as a wave-uniform mask; rows_next takes them
// off it one by one.  The for (row) / while (todo) / column loops stay in the
// kernels, with what they stage, address and compute.
//
// A reader is a small struct over the launch's arguments around the reading
// the host shares (ecg_kabi.h).  A lane keeps one value per stripe -- the word
// as the kernel wants it back: the classified cell, the set index, the mask
// -- and the rest follows from that value, so any of the 2^32 words is safe:
//     none        (static constexpr) a stripe past the row or the batch
//     load(s)     the value of stripe s, the one access to its word
//     verdict(w)  ROWS_ACCEPT: work; ROWS_NOTHING, as for none; ROWS_REFUSE: a
//                 word the call leaves as it is and counts
//     units(w)    what an accepted stripe adds to result[2]
#ifndef ECG_ROWS_DEV_H
#define ECG_ROWS_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../ecg_kabi.h"
#include "ecg_mm_dev.h"

enum { ROWS_REFUSE = -1, ROWS_NOTHING = 0, ROWS_ACCEPT = 1 };

__device__ __forceinline__ int rows_verdict(bool nothing, bool accept)
{
	return nothing ? ROWS_NOTHING : accept ? ROWS_ACCEPT : ROWS_REFUSE;
}

// The one definition of the four counters of a mask-driven call, preset by
// the host to {0, UINT64_MAX, 0, 0} (host/ecg_core.c ecg_result_reset):
//   result[0] += stripes accepted (repaired, recovered, updated)
//   result[1]  = min(result[1], lowest stripe refused)
//   result[2] += units of the accepted stripes (data cells rewritten, cells
//                regenerated, cells applied)
//   result[3] += stripes refused
// Stripe s, accepted or refused; one thread per stripe.  The compiler folds
// each atomic into one per wave; the refused branch ends in the min, not in
// its add, because two branches that both end in an add are merged into one
// add at a selected address, which is then issued once per lane.
__device__ __forceinline__ void rows_count(unsigned long long *result, uint32_t s, bool accepted,
					   unsigned long long units)
{
	if (accepted) {
		atomicAdd(&result[0], 1ull);
		atomicAdd(&result[2], units);
	} else {
		atomicAdd(&result[3], 1ull);
		atomicMin(&result[1], (unsigned long long)s);
	}
}

// The row's words: *lw = this lane's word of stripe row * grp + lane, returned
// the mask of the accepted stripes -- the same in every wave of the block, the
// words being read-only for the launch.  Stripes past the row or the batch
// read as nothing without touching memory.  Column-block 0 counts the row's
// stripes into `result`, one lane per stripe.
template <class R, class W>
__device__ __forceinline__ uint64_t rows_scan(uint32_t nstripes, uint32_t row, uint32_t grp,
					      unsigned long long *result, const R &read, W *lw)
{
	const uint32_t l = threadIdx.x & 63u;
	const uint64_t s = (uint64_t)row * grp + l;
	W w = R::none;

	if (l < grp && s < nstripes)
		w = read.load(s);
	const int v = read.verdict(w);
	if (blockIdx.x == 0 && threadIdx.x < 64 && v != ROWS_NOTHING)
		rows_count(result, (uint32_t)s, v == ROWS_ACCEPT, v == ROWS_ACCEPT ? read.units(w) : 0ull);
	*lw = w;
	return __ballot(v == ROWS_ACCEPT);
}

// The next stripe of the row with work: its index returned, its word in *w
// (wave-uniform), its bit cleared from *todo.
template <class W>
__device__ __forceinline__ uint32_t rows_next(uint64_t *todo, uint32_t row, uint32_t grp, W lw, W *w)
{
	const int l = __ffsll((unsigned long long)*todo) - 1;

	*w = (W)__builtin_amdgcn_readlane((int)lw, l);
	*todo &= *todo - 1;
	return row * grp + (uint32_t)l;
}

// block rows of a batch
static inline __host__ __device__ uint32_t rows_count_rows(uint32_t nstripes, uint32_t grp)
{
	return nstripes / grp + (nstripes % grp != 0);
}

// The launchers' grid: at most gxmax column blocks share a block row and
// stride over a stripe's 4 KiB columns, grid.y runs over the block rows of
// `grp` stripes up to the hardware's 65535; cfg's grid_x / grid_y override
// either.
static inline void rows_grid(const ecg_mm_params_t *p, uint32_t grp, uint32_t gxmax, const ecg_launch_cfg_t *cfg,
			     uint32_t *gx, uint32_t *gy)
{
	const uint64_t nchunk = (p->cell_bytes + CHUNK_BYTES - 1) / CHUNK_BYTES;
	const uint32_t nrow = rows_count_rows(p->nstripes, grp);

	*gx = cfg && cfg->grid_x ? cfg->grid_x : (uint32_t)(nchunk < gxmax ? nchunk : gxmax);
	*gy = cfg && cfg->grid_y ? cfg->grid_y : (nrow < 65535 ? nrow : 65535);
}

#endif
