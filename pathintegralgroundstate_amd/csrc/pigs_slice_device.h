// pigs_slice_device.h -- the building blocks that the estimator kernels over slices share: window_slice serves every
// kernel that takes a window slice but k_grv (pigs_bop.hip, pigs_vh.hip, pigs_g3.hip, pigs_atm.hip, pigs_fqt.hip,
// pigs_sqv.hip, pigs_fqv.hip), stage_rows the kernels that stage a slice or a tile of it (pigs_density.hip, pigs_vh.hip,
// pigs_g3.hip), flush_counts those that flush privatised counters at their end (pigs_density.hip,
// pigs_vh.hip).  Stateless __device__ __forceinline__ code only.  Each piece carries its correctness argument here, once;
// the kernels keep their barriers, their launch shapes and their LDS layouts.
// Only what compiles to the code of the loop it replaces lives here.  The pair walks (cyclic in k_grv and k_bop, the
// joined triangle in k_g3 and k_atm), the ballot compaction of k_g3 and k_atm and the radial rule of k_grv, k_bop and
// k_vh stay in their kernels: as helpers they changed the schedule or the registers of those inner loops, and k_grv, whose
// code moved with window_slice alone, is not built on this header (profiles/r07_window_regs.txt has the figures).
#pragma once

#include "pigs_device.h"

namespace pigs {

// Slice a of walker w (a = Nb - window + js for window slice js): DIM rows of NpPad doubles.
template <int DIM>
__device__ __forceinline__ const double *window_slice(const DevParams &P, const double *paths, int w, int a)
{
    return paths + ((size_t)w * P.M + a) * slice_doubles(DIM, P.NpPad);
}

// The workgroup copies `count` particles of the slice S, from particle `first` on, into DIM rows of dst that lie
// dst_stride apart.  Consecutive threads read consecutive global addresses and write consecutive LDS addresses (unit
// stride, no bank conflict); with count == dst_stride the rows are dense.  No barrier: the caller orders the copy against
// the readers of dst on both sides.
template <int DIM>
__device__ __forceinline__ void stage_rows(double *dst, int dst_stride, const double *S, int NpPad, int first, int count)
{
    for (int t = threadIdx.x; t < DIM * count; t += blockDim.x) {
        const int k = t / count, ii = t - k * count;
        dst[k * dst_stride + ii] = S[(size_t)k * NpPad + first + ii];
    }
}

// The workgroup adds the n u32 counters of hist, times scale, to the u64 accumulators dst_of(t), empty ones skipped.  A
// u32 counter cannot wrap if it gains at most 2^32 - 1 counts before the flush: each kernel bounds that by the events of
// one workgroup.  The caller puts the barrier between the last count and the flush.
template <class DstOf>
__device__ __forceinline__ void flush_counts(unsigned int *hist, int n, DstOf dst_of, unsigned long long scale = 1ull)
{
    for (int t = threadIdx.x; t < n; t += blockDim.x) {
        const unsigned int c = hist[t];
        if (c) atomicAdd(dst_of(t), scale * c);
    }
}

} // namespace pigs
