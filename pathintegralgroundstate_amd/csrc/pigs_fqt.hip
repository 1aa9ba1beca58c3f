// pigs_fqt.hip -- imaginary-time density correlations F(q,tau) of a periodic system (pigs_fqt_*).
//
// The reference's structural estimators are equal-time quantities of slice Nb (sample_mod.f90:392-473).  PIGS keeps the
// whole path, so the correlation of the density fluctuations BETWEEN slices is there to be taken:
//   F(q, tau_l) = < rho_q(a+l) rho_-q(a) > / Np = < C(a) C(a+l) + S(a) S(a+l) > / Np,      tau_l = l dt
//   C(s) = sum_i cos(q x_k(i,s)),  S(s) = sum_i sin(q x_k(i,s)),  q = real(iq) * (2 pi / Lbox(k))
// on the S(k) grid of the reference (sample_mod.f90:435-476, vpi.f90:119), the phase formed exactly as k_structure
// forms it.  The slices used are the window Nb-W .. Nb+W; per walker and call
//   acc[l][iq][k] += sum over a = Nb-W .. Nb+W-l (ascending) of C(a) C(a+l) + S(a) S(a+l),      l = 0 .. Ntau
// With W = 0, Ntau = 0 that is the reference's StructureFactor increment of slice Nb.
//
// Two stages on the context's stream:
//   k_fqt_rho        one workgroup per (listed walker, window slice): lanes over particles (unit stride in the slice's
//                    rows), four harmonics of one axis at a time -- 8 accumulators, one direct sincos per harmonic (the
//                    reference's term rounding) -- reduced over the wave by wave_reduce_lds<8>, over the waves in wave
//                    order by one thread per value.  Np beyond the workgroup makes several trips (per-lane sums in
//                    ascending particle order first).  C and S go to a scratch buffer, 2 Nk dim doubles per slice.
//   k_fqt_correlate  one thread per (listed walker, l, iq, k): the ordered sum over a, added to the accumulator element
//                    that this thread alone owns in this launch (the host never puts a walker twice into one launch).
// No floating-point atomics: a fixed tree and fixed orders, so the sums are the same bits for every launch shape.
// Compile with -ffp-contract=off: products and sums round one by one.
#include <algorithm>

#include "pigs_kernels.h"
#include "pigs_launch.h"
#include "pigs_slice_device.h"

namespace pigs {

namespace {

constexpr int kFqtGroupsPerChunk = 32;                  // groups of 4 harmonics whose wave totals wait in LDS together
constexpr int kFqtChunkVals = 8 * kFqtGroupsPerChunk;

// value j = 2 m + cs of group g: harmonic iq = 4 (g % ng) + m + 1 of axis k = g / ng; cs = 0 cosine, 1 sine
template <int DIM>
__global__ __launch_bounds__(256) void k_fqt_rho(
    DevParams P, const double *__restrict__ paths, WalkerList list, int window, int Nk, double pi, double *__restrict__ rho)
{
    __shared__ double red[4 * 8 * kRedStride];         // wave_reduce_lds scratch, one block per wave
    __shared__ double part[4 * kFqtChunkVals];         // wave totals of one chunk of values
    const int ns = 2 * window + 1;
    const int slot = blockIdx.x / ns, j = blockIdx.x - slot * ns;
    const int w = list.w[slot];
    const int Np = P.Np, NpPad = P.NpPad;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const double *S = window_slice<DIM>(P, paths, w, P.Nb - window + j);
    double *out = rho + ((size_t)slot * ns + j) * (2 * (size_t)Nk * DIM);
    const int ng = (Nk + 3) >> 2, G = DIM * ng;

    for (int g0 = 0; g0 < G; g0 += kFqtGroupsPerChunk) {
        const int g1 = min(G, g0 + kFqtGroupsPerChunk);
        for (int g = g0; g < g1; ++g) {
            const int k = g / ng, iq0 = 4 * (g - k * ng) + 1;
            const double qbin = 2.0 * pi / P.Lbox[k];                       // vpi.f90:119
            double v[8];
#pragma unroll
            for (int m = 0; m < 8; ++m) v[m] = 0.0;
            for (int i = threadIdx.x; i < Np; i += blockDim.x) {
                const double x = S[(size_t)k * NpPad + i];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    if (iq0 + m <= Nk) {
                        const double qr = (double)(float)(iq0 + m) * qbin * x;
                        double sn, cs;
                        sincos(qr, &sn, &cs);
                        v[2 * m] = v[2 * m] + cs;
                        v[2 * m + 1] = v[2 * m + 1] + sn;
                    }
                }
            }
            const double t = wave_reduce_lds<8>(v, red + wid * 8 * kRedStride, lane);
            if (lane < 8) part[wid * kFqtChunkVals + (g - g0) * 8 + lane] = t;
        }
        __syncthreads();
        for (int t = threadIdx.x; t < (g1 - g0) * 8; t += blockDim.x) {
            const int g = g0 + (t >> 3), m = (t & 7) >> 1, cs = t & 1;
            const int k = g / ng, iq = 4 * (g - k * ng) + m + 1;
            if (iq > Nk) continue;
            double s = part[t];
            for (int q = 1; q < nw; ++q) s = s + part[q * kFqtChunkVals + t];
            out[2 * ((size_t)(iq - 1) * DIM + k) + cs] = s;
        }
        __syncthreads();
    }
}

// rho: [slot][window slice][(iq-1) dim + k][cos, sin]; acc: [walker][l][(iq-1) dim + k]
__global__ __launch_bounds__(256) void k_fqt_correlate(
    WalkerList list, int n, int window, int Ntau, int T, const double *__restrict__ rho, double *__restrict__ acc,
    unsigned long long *__restrict__ samples)
{
    const size_t per = (size_t)(Ntau + 1) * T;
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= per * n) return;
    const int slot = (int)(id / per);
    const size_t e = id - (size_t)slot * per;
    const int l = (int)(e / T), t = (int)(e - (size_t)l * T);
    const int ns = 2 * window + 1;
    const int w = list.w[slot];
    const double *r = rho + (size_t)slot * ns * 2 * T + 2 * (size_t)t;
    double s = 0.0;
    for (int a = 0; a + l < ns; ++a) {
        const double *p = r + (size_t)a * 2 * T, *q = r + (size_t)(a + l) * 2 * T;
        s = s + (p[0] * q[0] + p[1] * q[1]);
    }
    double *dst = acc + (size_t)w * per + e;
    *dst = *dst + s;
    if (e == 0) samples[w] = samples[w] + 1ull;
}

} // namespace

hipError_t launch_fqt(const DevParams &P, const double *paths, int n, const WalkerList &list, int window, int Ntau, int Nk,
                      double *rho, double *acc, unsigned long long *samples, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const int ns = 2 * window + 1, T = Nk * P.dim;
    const int threads = 64 * std::min(4, (P.Np + 63) / 64);
    const double pi = acos(-1.0);
    const hipError_t e = with_dim(P.dim, [&](auto D) {
        return launch<k_fqt_rho<D()>>(dim3(n * ns), dim3(threads), 0, st, P, paths, list, window, Nk, pi, rho);
    });
    if (e != hipSuccess) return e;
    const size_t total = (size_t)n * (Ntau + 1) * T;
    if ((total + 255) / 256 > 0x7fffffffull) return hipErrorInvalidValue;
    return launch<k_fqt_correlate>(dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, list, n, window, Ntau, T,
                                   rho, acc, samples);
}

} // namespace pigs
