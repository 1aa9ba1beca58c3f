// pigs_density.hip -- density profiles and pair distribution of a trapped system (pigs_density_*).
//
// The reference allocates dens(Nbin,Nbin) (vpi.f90:198) and has DensityProfile / PrintDensity written
// (sample_mod.f90:598-652), but leaves the call commented out (vpi.f90:471): a trapped run produces energies only.
// k_density fills that gap with three integer histograms of the middle slice Path(:,:,Nb), per walker:
//   planar  over [-h, h)^min(dim,2), bin width b = (2h)/Nbin, flat index j_1 + Nbin*j_2 (x fastest); for dim = 3
//           the column density over (x_1, x_2)
//   radial  over r = |x| in [0, h), bin width br = h/Nbin
//   pair    over the pair distance d in [0, h), width br, +2 per pair i < j (the reference's PairCorrelation); no
//           minimum image (there is no box)
// plus one sample per call.  The planar grid is the one of the reference's dead routine (sample_mod.f90:598-629) with
// its off-by-one fixed: there int((x+0.5 rcut)/rbin), kept only for 1..Nbin, drops the first bin and covers
// [-h+rbin, h+rbin).  The routine is never called, so it is not a parity target.
//
// Every bin decision is taken in double BEFORE any conversion to an integer (a value that fails `0 <= t < Nbin` --
// NaN, +-Inf, 1e300 -- is dropped without undefined behaviour).  Counts are 64-bit integer atomics: the result does
// not depend on the order of additions, and a walker listed twice counts twice.
// Compile with -ffp-contract=off: the squared distances are summed left to right without fused multiply-adds.
// The tile staging and the flush of the LDS counters are pigs_slice_device.h's.
#include "pigs_kernels.h"
#include "pigs_launch.h"
#include "pigs_slice_device.h"

namespace pigs {

namespace {

constexpr int kDensThreads = 256;
constexpr int kDensTile = 1024;       // particles of the slice staged in LDS at a time (24 KB at dim = 3)

// One workgroup per listed walker.  Thread t owns particle i = i0 + t of each block of kDensThreads particles: it bins
// that particle into the planar and radial histograms (straight to global memory: at most Np atomics per walker) and
// walks its partners j > i through LDS tiles of the slice (broadcast reads).  The pair histogram lives in LDS (u32
// pair counts, flushed as 2 x count) when lds_hist, in global memory otherwise.
template <int DIM>
__global__ __launch_bounds__(kDensThreads) void k_density(
    DevParams P, const double *__restrict__ paths, WalkerList list, int tile, int Nbin, double h, double b, double br,
    int lds_hist, unsigned long long *__restrict__ planar, unsigned long long *__restrict__ radial,
    unsigned long long *__restrict__ pair, unsigned long long *__restrict__ samples)
{
    extern __shared__ double lds[];
    double *sx = lds;                                                       // DIM x tile
    unsigned int *hist = reinterpret_cast<unsigned int *>(lds + DIM * tile); // Nbin (lds_hist only)
    constexpr int DP = DIM < 2 ? DIM : 2;
    const int w = list.w[blockIdx.x];
    const int Np = P.Np, NpPad = P.NpPad;
    const double nb = (double)Nbin;
    const double *S = paths + ((size_t)w * P.M + P.Nb) * slice_doubles(DIM, NpPad);
    size_t nplanar = 1;
    for (int k = 0; k < DP; ++k) nplanar *= (size_t)Nbin;
    unsigned long long *pl = planar + (size_t)w * nplanar;
    unsigned long long *ra = radial + (size_t)w * Nbin;
    unsigned long long *pa = pair + (size_t)w * Nbin;
    if (lds_hist)
        for (int t = threadIdx.x; t < Nbin; t += blockDim.x) hist[t] = 0u;   // ordered by the first staging's barrier

    int staged = -1;                                        // first particle of the tile in LDS (uniform over the group)
    for (int i0 = 0; i0 < Np; i0 += blockDim.x) {
        const int i = i0 + (int)threadIdx.x;
        const bool own = i < Np;
        double xi[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) xi[k] = own ? S[(size_t)k * NpPad + i] : 0.0;
        if (own) {
            // planar: t = (x_k + h)/b must satisfy 0 <= t < Nbin for each of the first min(dim,2) coordinates
            bool in = true;
            size_t flat = 0, stride = 1;
#pragma unroll
            for (int k = 0; k < DP; ++k) {
                const double t = (xi[k] + h) / b;
                if (t >= 0.0 && t < nb) flat += (size_t)(int)t * stride;
                else in = false;
                stride *= (size_t)Nbin;
            }
            if (in) atomicAdd(&pl[flat], 1ull);
            // radial: r = |x| summed left to right, u = r/br
            double r2 = xi[0] * xi[0];
#pragma unroll
            for (int k = 1; k < DIM; ++k) r2 = r2 + xi[k] * xi[k];
            const double u = sqrt(r2) / br;
            if (u < nb) atomicAdd(&ra[(int)u], 1ull);
        }
        // pairs (i, j > i): the tiles from the one holding i0 on
        for (int j0 = (i0 / tile) * tile; j0 < Np; j0 += tile) {
            const int m = min(tile, Np - j0);
            if (j0 != staged) {
                __syncthreads();
                stage_rows<DIM>(sx, tile, S, NpPad, j0, m);
                __syncthreads();
                staged = j0;
            }
            if (!own) continue;
            for (int jj = max(0, i + 1 - j0); jj < m; ++jj) {
                double d2;
                {
                    const double d = xi[0] - sx[jj];
                    d2 = d * d;
                }
#pragma unroll
                for (int k = 1; k < DIM; ++k) {
                    const double d = xi[k] - sx[k * tile + jj];
                    d2 = d2 + d * d;
                }
                const double u = sqrt(d2) / br;
                if (u < nb) {
                    if (lds_hist) atomicAdd(&hist[(int)u], 1u);
                    else atomicAdd(&pa[(int)u], 2ull);
                }
            }
        }
    }
    if (lds_hist) {
        __syncthreads();
        flush_counts(hist, Nbin, [&](int t) { return &pa[t]; }, 2ull);
    }
    if (threadIdx.x == 0) atomicAdd(&samples[w], 1ull);
}

} // namespace

hipError_t launch_density(const DevParams &P, const double *paths, int n, const WalkerList &list, int Nbin, double h,
                          double b, double br, unsigned long long *planar, unsigned long long *radial,
                          unsigned long long *pair, unsigned long long *samples, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const int tile = min(P.Np, kDensTile);
    const int lds_hist = Nbin <= kDensLdsBins;
    const size_t lds = (size_t)P.dim * tile * sizeof(double) + (lds_hist ? (size_t)Nbin * sizeof(unsigned int) : 0);
    if (lds > kLdsNoGrant) return hipErrorInvalidValue;
    return with_dim(P.dim, [&](auto D) {
        return launch<k_density<D()>>(dim3(n), dim3(kDensThreads), lds, st, P, paths, list, tile, Nbin, h, b, br, lds_hist, planar,
                                      radial, pair, samples);
    });
}

} // namespace pigs
