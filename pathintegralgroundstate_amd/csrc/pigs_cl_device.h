// pigs_cl_device.h -- what the two kernels that label the bond graph of a slice share (k_cl of pigs_cl.hip, k_pc of
// pigs_pc.hip): the relaxed LDS load, the bond mask of 64 partners, the mask of the partners above a particle, and the
// labelling loop itself -- one copy of it.  Stateless __device__ __forceinline__ code; the kernels keep their LDS layouts
// and everything after the labels.  pigs_cl.hip's header has the argument why a sweep without a change ends with every
// label at the smallest index of its component.
#pragma once

#include "pigs_device.h"
#include "pigs_kernels.h"

namespace pigs {

__device__ __forceinline__ int lds_load(const int *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the bonds of particle i (at xi) among the partners j0 .. j0 + mj - 1 of the staged slice, bit jj for partner j0 + jj
template <int DIM>
__device__ __forceinline__ unsigned long long bond_mask(const DevParams &P, const double *sx, int Np, const double (&xi)[DIM],
                                                        int j0, int mj, double rc2)
{
    unsigned long long bonds = 0ull;
    for (int jj = 0; jj < mj; ++jj) {
        double d[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) d[k] = xi[k] - sx[k * Np + j0 + jj];
        const double r2 = min_image<DIM>(d, P);
        if (r2 > 0.0 && r2 < rc2) bonds |= 1ull << jj;                 // (j == i: r2 is 0 or NaN)
    }
    return bonds;
}

// the bits of a mask over the partners j0 .. j0 + 63 that lie above particle i
__device__ __forceinline__ unsigned long long above(int i, int j0)
{
    if (i < j0) return ~0ull;
    if (i >= j0 + 63) return 0ull;
    return ~0ull << (i - j0 + 1);
}

// The workgroup of kClThreads threads labels the slice sx (DIM rows of Np): label[i] = i on entry (after a barrier), the
// smallest index of i's component on return (after a barrier: the vote).  ADJ: adj holds the bit rows (nw u64 per
// particle); otherwise every sweep computes the masks again and the first one adds the thread's bonds j > i to nb.
// Returns the number of sweeps.
template <int DIM, bool ADJ>
__device__ __forceinline__ unsigned int label_components(const DevParams &P, const double *sx, int Np, int nw,
                                                         const unsigned long long *adj, int *label, double rc2, int tid,
                                                         unsigned int &nb)
{
    unsigned int nsweep = 0u;
    for (;;) {
        int changed = 0;
        for (int i = tid; i < Np; i += kClThreads) {
            double xi[DIM];
#pragma unroll
            for (int k = 0; k < DIM; ++k) xi[k] = sx[k * Np + i];
            const int li = lds_load(&label[i]);
            int m = li;
            for (int j0 = 0, b = 0; j0 < Np; j0 += 64, ++b) {
                unsigned long long bonds;
                if (ADJ) bonds = adj[(size_t)i * nw + b];
                else {
                    bonds = bond_mask<DIM>(P, sx, Np, xi, j0, min(64, Np - j0), rc2);
                    if (nsweep == 0u) nb += (unsigned int)__popcll(bonds & above(i, j0));
                }
                while (bonds) {
                    const int jj = __ffsll((long long)bonds) - 1;
                    bonds &= bonds - 1ull;
                    m = min(m, lds_load(&label[j0 + jj]));
                }
            }
            if (m < li) {
                atomicMin(&label[li], m);
                atomicMin(&label[i], m);
                changed = 1;
            }
        }
        __syncthreads();
        for (int i = tid; i < Np; i += kClThreads) {
            const int l = lds_load(&label[i]);
            const int ll = lds_load(&label[l]);
            if (ll < l) {
                atomicMin(&label[i], ll);
                changed = 1;
            }
        }
        ++nsweep;
        if (!__syncthreads_or(changed)) break;
    }
    return nsweep;
}

} // namespace pigs
