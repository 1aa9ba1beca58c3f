// pigs_fqv.hip -- imaginary-time density correlations F(q,tau) of a periodic system on the full reciprocal grid (pigs_fqv_*).
//
// pigs_fqt_* has the lags but only the axis grid; pigs_sqv_* has the full grid but squares rho_q inside its kernel.  This
// one keeps the phase: on the vectors of pigs_sqv_* (same enumeration, sqv_shape) and over the window of pigs_fqt_*,
//   acc[l][iqv] += sum over a = Nb-W .. Nb+W-l (ascending) of C(a) C(a+l) + S(a) S(a+l),      l = 0 .. Ntau
//   C(a) + i S(a) = sum_i exp(i q.x_i(a))
// Lag 0 is what pigs_sqv_accumulate adds, to the last bit: C and S come from the same device function.
//
// Two launches on the context's stream:
//   k_fqv_rho        one workgroup per (listed walker, window slice): sqv_rho_slice (pigs_sqv_device.h), the code that
//                    k_sqv_rho2 runs, storing (C, S) as one 16-byte element per vector instead of C^2 + S^2.  Scratch:
//                    [slot][slice][iqv] of c2.
//   k_fqv_correlate  one workgroup per (listed walker, tile of `width` consecutive vectors).  The tile's (C, S) of all
//                    ns = 2 W + 1 slices is staged in LDS, [slice][vector of the tile] of c2, read from the scratch in
//                    rows that are unit-stride over iqv: every scratch element is read from memory once per launch.
//                    Thread t takes vector t % width and the lags t / width, + 256 / width, ..: the lanes of a wave
//                    run over consecutive vectors, so a 16-byte LDS read of a 16-lane group covers one 256-byte bank
//                    row without conflict, and the lags are shared out over the waves.  One thread sums an (l, vector)
//                    element over a in ascending order and adds it to the accumulator element it alone owns in this
//                    launch (the host never puts a walker twice into one launch).
// No floating-point atomics; every sum has one fixed order that depends on neither the walker list, the launch split
// nor the tile width.  Compile with -ffp-contract=off: only the fma written out in sqv_rho_slice is fused.
#include "pigs_kernels.h"
#include "pigs_launch.h"
#include "pigs_slice_device.h"
#include "pigs_sqv_device.h"

namespace pigs {

namespace {

template <int DIM>
__global__ __launch_bounds__(kSqvThreadsMax) void k_fqv_rho(
    DevParams P, const double *__restrict__ paths, WalkerList list, int window, int nmax, int tile, int nprefix, int nchunk,
    long long Nq, double pi, double *__restrict__ rho)
{
    extern __shared__ c2 tab[];
    const int ns = 2 * window + 1;
    const int slot = blockIdx.x / ns, j = blockIdx.x - slot * ns;
    const int w = list.w[slot];
    const double *X = window_slice<DIM>(P, paths, w, P.Nb - window + j);
    sqv_rho_slice<DIM, true>(P, X, tab, nmax, tile, nprefix, nchunk, Nq, pi, rho + ((size_t)slot * ns + j) * 2 * (size_t)Nq);
}

// rho: [slot][window slice][iqv] of c2; acc: [walker][l][iqv]; st: [slice][vector of the tile], width a power of two
__global__ __launch_bounds__(kFqvThreads) void k_fqv_correlate(
    WalkerList list, int ns, int Ntau, int width, int ntiles, long long Nq, const double *__restrict__ rho,
    double *__restrict__ acc, unsigned long long *__restrict__ samples)
{
    extern __shared__ c2 st[];
    const int slot = blockIdx.x / ntiles, tl = blockIdx.x - slot * ntiles;
    const int w = list.w[slot];
    const long long v0 = (long long)tl * width;
    const int nv = (int)min((long long)width, Nq - v0);
    const c2 *src = reinterpret_cast<const c2 *>(rho) + (size_t)slot * ns * (size_t)Nq + v0;
    const int sh = __ffs(width) - 1;
    for (int t = threadIdx.x; t < ns * width; t += blockDim.x) {
        const int a = t >> sh, v = t & (width - 1);
        if (v < nv) st[t] = src[(size_t)a * Nq + v];
    }
    __syncthreads();
    const int v = threadIdx.x & (width - 1), lg = threadIdx.x >> sh, nlg = blockDim.x >> sh;
    if (v >= nv) return;
    double *dst = acc + (size_t)w * (Ntau + 1) * (size_t)Nq + v0 + v;
    for (int l = lg; l <= Ntau; l += nlg) {
        const c2 *p = st + v, *q = st + (size_t)l * width + v;
        double s = 0.0;
        for (int a = 0; a + l < ns; ++a) {
            const c2 x = p[(size_t)a * width], y = q[(size_t)a * width];
            s = s + (x.x * y.x + x.y * y.y);
        }
        dst[(size_t)l * Nq] = dst[(size_t)l * Nq] + s;
    }
    if (tl == 0 && threadIdx.x == 0) samples[w] = samples[w] + 1ull;
}

} // namespace

int fqv_width(int ns)
{
    int width = kFqvWidthMax;
    while (width > 1 && (size_t)ns * width * sizeof(c2) > kFqvLdsBudget) width /= 2;
    return (size_t)ns * width * sizeof(c2) > kFqvLdsBudget ? 0 : width;
}

hipError_t launch_fqv(const DevParams &P, const double *paths, int n, const WalkerList &list, int window, int Ntau, int nmax,
                      double *rho, double *acc, unsigned long long *samples, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const SqvShape s = sqv_shape(P.dim, nmax);
    const int ns = 2 * window + 1;
    const int width = fqv_width(ns);
    if (!width) return hipErrorInvalidValue;
    const double pi = acos(-1.0);
    const hipError_t e = with_dim(P.dim, [&](auto D) {
        return launch<k_fqv_rho<D()>>(dim3(n * ns), dim3(s.threads), s.lds, st, P, paths, list, window, nmax, s.tile, s.nprefix,
                                      s.nchunk, s.Nq, pi, rho);
    });
    if (e != hipSuccess) return e;
    const long long ntiles = (s.Nq + width - 1) / width;
    if (ntiles * n > 0x7fffffffll) return hipErrorInvalidValue;
    return launch<k_fqv_correlate>(dim3((unsigned)(ntiles * n)), dim3(kFqvThreads), (size_t)ns * width * sizeof(c2), st,
                                   list, ns, Ntau, width, (int)ntiles, s.Nq, rho, acc, samples);
}

} // namespace pigs
