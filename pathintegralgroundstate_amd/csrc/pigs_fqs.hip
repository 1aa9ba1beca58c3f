// pigs_fqs.hip -- the self (incoherent) part of F(q,tau) and the imaginary-time displacement of a periodic system
// (pigs_fqs_*).
//
// pigs_fqv_* correlates rho_q = sum_i exp(i q.x_i) of two slices; this one follows ONE particle along its worldline.  On
// the vectors of pigs_sqv_* (same enumeration, sqv_shape) and over the window and lags of pigs_fqv_*,
//   F[l][iqv] += sum over i = 0 .. Np-1, a = Nb-W .. Nb+W-l of c_i(a) c_i(a+l) + s_i(a) s_i(a+l),   l = 0 .. Ntau
//   c_i(a) + i s_i(a) = exp(i q.x_i(a))
//   D[l][0]   += sum over i, a of r2,   D[l][1] += sum over i, a of r2 r2
//   r2 = |x_i(a+l) - x_i(a)|^2, the difference folded once by min_image<DIM> (the two compares of pbc_mod.f90:40-41)
// exp(i q.x) depends on no wrap of x (q is a reciprocal vector of the box); the displacement is the true one only while
// |d_k| < Lbox[k]/2, which the caller judges.
//
// rho_q per particle cannot go through a global scratch as pigs_fqv.hip's rho_q per slice does (Np times the bytes), so
// the phasors live in LDS and the sums in registers.  Two launches on the context's stream:
//   k_fqs      one workgroup per (listed walker, tile of `width` consecutive vectors), looping over the particles in
//              ascending order.  Per particle:
//                1. tab[a][k][m], m = 0..nmax: the per-axis phasors of all ns = 2 W + 1 window slices, each from one
//                   sincos of the phase (double)(float)m * (2 pi / Lbox[k]) * x_k as sqv_rho_slice forms it (entry 0 is
//                   (1, 0), which is what sincos(0 * ..) gives, without the call);
//                2. st[a][v]: the tile's phasors, the axes multiplied in sqv_rho_slice's order ((e_1 e_2) e_3);
//                3. thread t owns vector t % width and the lags t / width, + 256 / width, .. (at most kFqsLags of them,
//                   one register each, kept across the particle loop): R = R + (x.x * y.x + x.y * y.y) for a ascending.
//              After the last particle acc = acc + R, by the thread that alone owns the element in this launch (the
//              host never puts a walker twice into one launch).  The table is recomputed once per vector tile.
//   k_fqs_msd  one workgroup per (listed walker, lag).  A lane takes the particles lane, lane + blockDim, .. in ascending
//              order and for each the pairs a ascending: s1 = s1 + r2, s2 = s2 + r2 * r2.  Then k_tau's reduction: the
//              wave's butterfly (wave_sum), the waves in wave order, acc += value.
// No floating-point atomics; every sum has one fixed order that depends on neither the walker list, the launch split,
// the tile width (an element's order does not involve the tile) nor the context.  Compile with -ffp-contract=off.
#include <algorithm>

#include "pigs_device.h"
#include "pigs_kernels.h"
#include "pigs_launch.h"
#include "pigs_sqv_device.h"

namespace pigs {

namespace {

// acc: [walker][l][iqv]; tab: [a][k][m = 0..nmax]; st: [a][vector of the tile], width a power of two <= kFqsThreads
template <int DIM>
__global__ __launch_bounds__(kFqsThreads) void k_fqs(
    DevParams P, const double *__restrict__ paths, WalkerList list, int window, int Ntau, int nmax, int width, int ntiles,
    long long Nq, double pi, double *__restrict__ acc, unsigned long long *__restrict__ samples)
{
    extern __shared__ c2 lds[];
    const int ns = 2 * window + 1, ms = nmax + 1;
    c2 *tab = lds;                                   // ns * DIM * ms
    c2 *st = lds + (size_t)ns * DIM * ms;            // ns * width
    double *qbin = reinterpret_cast<double *>(st + (size_t)ns * width);   // DIM
    const int slot = blockIdx.x / ntiles, tl = blockIdx.x - slot * ntiles;
    const int w = list.w[slot];
    const long long v0 = (long long)tl * width;
    const int nv = (int)min((long long)width, Nq - v0);
    const int sh = __ffs(width) - 1;
    const int v = threadIdx.x & (width - 1), lg = threadIdx.x >> sh, nlg = kFqsThreads >> sh;
    const size_t sl = slice_doubles(DIM, P.NpPad);
    const double *X = paths + ((size_t)w * P.M + (P.Nb - window)) * sl;

    // the integer vector of this thread's column (pigs_sqv_vectors: rank iqv + Nq + 1 among all S^dim, n_1 slowest)
    int nk[DIM];
    {
        const int S = 2 * nmax + 1;
        long long r = v0 + (v < nv ? v : 0) + Nq + 1;
#pragma unroll
        for (int k = DIM - 1; k >= 0; --k) {
            nk[k] = (int)(r % S) - nmax;
            r /= S;
        }
    }

    double R[kFqsLags];
#pragma unroll
    for (int j = 0; j < kFqsLags; ++j) R[j] = 0.0;
    // pairs (a, a + l) of this thread's lag j: a < lim[j] (0: the lag is beyond Ntau)
    int lim[kFqsLags];
#pragma unroll
    for (int j = 0; j < kFqsLags; ++j) lim[j] = lg + j * nlg <= Ntau ? ns - (lg + j * nlg) : 0;
    // the table's items t = threadIdx.x + j kFqsThreads as (a, r) without a division per item
    const int dm = DIM * ms, a0 = threadIdx.x / dm, r0 = threadIdx.x - a0 * dm, da = kFqsThreads / dm, dr = kFqsThreads - da * dm;
    if (threadIdx.x < DIM) qbin[threadIdx.x] = 2.0 * pi / P.Lbox[threadIdx.x];   // vpi.f90:119
    __syncthreads();

    for (int i = 0; i < P.Np; ++i) {
        // 1. the per-axis phasor table of particle i (the previous particle's table was consumed before its barrier 2)
        for (int t = threadIdx.x, a = a0, r = r0; t < ns * dm; t += kFqsThreads) {
            const int k = (r >= ms) + (r >= 2 * ms), m = r - k * ms;  // t = a dm + r, r = k ms + m
            c2 e{1.0, 0.0};
            if (m) {
                const double qr = (double)(float)m * qbin[k] * X[(size_t)a * sl + (size_t)k * P.NpPad + i];
                sincos(qr, &e.y, &e.x);
            }
            tab[t] = e;
            a += da; r += dr;
            if (r >= dm) { r -= dm; ++a; }
        }
        __syncthreads();                                              // barrier 1: also, the previous st has been consumed
        // 2. the tile's phasors
        for (int t = threadIdx.x; t < ns * width; t += kFqsThreads) {  // t & (width - 1) == v: blockDim is a multiple of width
            const int a = t >> sh;
            const c2 *row = tab + (size_t)a * DIM * ms;
            c2 e = phasor(row, nk[0]);
#pragma unroll
            for (int k = 1; k < DIM; ++k) {
                const c2 f = phasor(row + k * ms, nk[k]);
                const double br = e.x * f.x - e.y * f.y, bi = e.x * f.y + e.y * f.x;
                e.x = br; e.y = bi;
            }
            st[t] = e;
        }
        __syncthreads();                                              // barrier 2
        // 3. the lag sums of this particle
        if (v < nv) {
            for (int a = 0; a < ns; ++a) {
                const c2 x = st[(size_t)a * width + v];
#pragma unroll
                for (int j = 0; j < kFqsLags; ++j) {
                    if (a < lim[j]) {
                        const c2 y = st[(size_t)(a + lg + j * nlg) * width + v];
                        R[j] = R[j] + (x.x * y.x + x.y * y.y);
                    }
                }
            }
        }
    }
    if (v < nv) {
        double *dst = acc + (size_t)w * (Ntau + 1) * (size_t)Nq + v0 + v;
#pragma unroll
        for (int j = 0; j < kFqsLags; ++j) {
            const int l = lg + j * nlg;
            if (l <= Ntau) dst[(size_t)l * Nq] = dst[(size_t)l * Nq] + R[j];
        }
    }
    if (tl == 0 && threadIdx.x == 0) samples[w] = samples[w] + 1ull;
}

// dsp: [walker][l][2]
template <int DIM>
__global__ __launch_bounds__(256) void k_fqs_msd(
    DevParams P, const double *__restrict__ paths, WalkerList list, int window, int Ntau, double *__restrict__ dsp)
{
    __shared__ double red[2 * 4];
    const int ns = 2 * window + 1;
    const int slot = blockIdx.x / (Ntau + 1), l = blockIdx.x - slot * (Ntau + 1);
    const int w = list.w[slot];
    const size_t sl = slice_doubles(DIM, P.NpPad);
    const double *X = paths + ((size_t)w * P.M + (P.Nb - window)) * sl;

    double s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < P.Np; i += blockDim.x) {
        for (int a = 0; a + l < ns; ++a) {
            double d[DIM];
#pragma unroll
            for (int k = 0; k < DIM; ++k)
                d[k] = X[(size_t)(a + l) * sl + (size_t)k * P.NpPad + i] - X[(size_t)a * sl + (size_t)k * P.NpPad + i];
            const double r2 = min_image<DIM>(d, P);
            s1 = s1 + r2;
            s2 = s2 + r2 * r2;
        }
    }
    s1 = wave_sum(s1); s2 = wave_sum(s2);
    const int nw = blockDim.x >> 6, wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[2 * wid] = s1; red[2 * wid + 1] = s2; }
    __syncthreads();
    if (threadIdx.x < 2) {
        double a = 0.0;
        for (int q = 0; q < nw; ++q) a += red[2 * q + threadIdx.x];
        double *dst = dsp + ((size_t)w * (Ntau + 1) + l) * 2 + threadIdx.x;
        *dst = *dst + a;
    }
}

} // namespace

FqsShape fqs_shape(int dim, int nmax, int window, int Ntau)
{
    const size_t ns = 2 * (size_t)window + 1, tab = ns * dim * (nmax + 1) * sizeof(c2);
    FqsShape s{0, 0};
    for (int width = kFqsWidthMax; width >= 1; width /= 2) {
        const size_t lds = tab + ns * width * sizeof(c2) + 3 * sizeof(double);
        if (lds <= kFqsLdsBudget && (long long)(kFqsThreads / width) * kFqsLags >= Ntau + 1) {
            s.width = width;
            s.lds = lds;
            break;
        }
    }
    return s;
}

hipError_t launch_fqs(const DevParams &P, const double *paths, int n, const WalkerList &list, int window, int Ntau, int nmax,
                      double *acc, double *dsp, unsigned long long *samples, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    if (n > kWalkerListMax) return hipErrorInvalidValue;
    const SqvShape q = sqv_shape(P.dim, nmax);
    const FqsShape s = fqs_shape(P.dim, nmax, window, Ntau);
    if (!s.width) return hipErrorInvalidValue;
    const double pi = acos(-1.0);
    const long long ntiles = (q.Nq + s.width - 1) / s.width;
    if (ntiles * n > 0x7fffffffll || (long long)n * (Ntau + 1) > 0x7fffffffll) return hipErrorInvalidValue;
    const int bs = std::min(256, ((P.Np + 63) / 64) * 64);
    // Order: k_fqs_msd, then k_fqs, which adds 1 to samples, last: a call that fails before its last launch has not
    // counted.  (k_fqs needs no grant that could refuse in between: fqs_shape keeps its LDS within kFqsLdsBudget, which is
    // the limit every kernel has without one.)
    static_assert(kFqsLdsBudget <= kLdsNoGrant, "k_fqs would need its grant before k_fqs_msd is queued");
    return with_dim(P.dim, [&](auto D) {
        const hipError_t e = launch<k_fqs_msd<D()>>(dim3((unsigned)(n * (Ntau + 1))), dim3(bs), 0, st, P, paths, list, window, Ntau, dsp);
        if (e != hipSuccess) return e;
        return launch<k_fqs<D()>>(dim3((unsigned)(ntiles * n)), dim3(kFqsThreads), s.lds, st, P, paths, list, window, Ntau, nmax,
                                  s.width, (int)ntiles, q.Nq, pi, acc, samples);
    });
}

} // namespace pigs
