// pigs_atm.hip -- the Axilrod-Teller-Muto (triple-dipole) geometric sum of a periodic system over a slice window
// (pigs_atm_*): per listed walker and window slice, T = sum over the triplets i < j < k whose three nearest-image sides all
// lie within rc of (1 + 3 cos cos cos) / (r_ij r_ik r_jk)^3, and the number of those triplets.  include/pigs_hip.h has the
// definition word for word.  The coupling nu never reaches the device.
//
// k_atm: one workgroup of kAtmWaves waves per (listed walker, window slice a = Nb-window .. Nb+window).
//   * The slice is staged once in LDS (unit-stride rows, 8 dim Np bytes).  A WAVE owns a vertex i; the vertices go round
//     the waves, i = wave, wave + kAtmWaves, ...  There is no workgroup barrier inside that loop: a wave only reads the
//     slice and its own list.
//   * Pass 1, the legs.  The lanes take 64 partners j > i at a time:
//       d_k = x_k(i) - x_k(j), folded by min_image<DIM>, a2 summed left to right (pigs_grv_*'s arithmetic)
//       leg iff a2 <= rc2 in double; NaN compares false
//     A ballot of the legs gives each its place in the wave's list (the count so far plus the legs in lower lanes), so the
//     list is in ascending j: (x_1(j)..x_DIM(j), a2), SoA with capacity Np per wave.  A vertex has at most Np - 1 legs, so
//     the list cannot overflow.  The list keeps the partner's COORDINATES, not d: the third side is a pair's own folded
//     difference, and consecutive lanes of pass 2 read consecutive addresses.
//   * Pass 2, the triplets.  The n (n - 1) / 2 pairs of the n legs are the rows m = 0..n-2 of a triangle, row m holding
//     the n - 1 - m pairs (m, m+1..n-1).  Row m is joined with row n - 2 - m into one row of exactly n entries (k_g3's
//     walk), and the lanes take the flat index of that rectangle 64 at a time.  A pair (j, k) of list places j < k is a
//     pair of particles j < k: a2 = a2(j), b2 = a2(k), c2 from x(j) - x(k) folded once.  Counted iff c2 <= rc2; then
//       p = (a2 b2) c2;  s = sqrt(p);  num = ((a2 + b2 - c2)(a2 + c2 - b2))(b2 + c2 - a2)
//       t = (p + 0.375 num) / ((p p) s)
//     with the compiler's IEEE sqrt and division.
//   * Summation order, fixed: a lane adds its terms in the order it meets them (vertices ascending, rounds ascending), the
//     wave's butterfly (wave_sum), the waves in wave order, and `acc += value` last, by the one thread that owns the
//     element (w, a) for the launch -- the host never lists a walker twice in ONE launch.  No floating-point atomics.
//   * The DS instructions of one wave execute in issue order; wave_barrier pins the compiler's order between the list's
//     writes (pass 1), its reads (pass 2) and the next vertex's writes.
// Nothing in the order depends on the walker list, the launch split or the context, so the same worldline gives the same
// bits.  Compile with -ffp-contract=off.
// The slice address is pigs_slice_device.h's.
#include "pigs_kernels.h"
#include "pigs_launch.h"
#include "pigs_slice_device.h"

namespace pigs {

namespace {

struct AtmArgs {
    int window, n, cap;                    // n: listed walkers of this launch; cap: entries of one wave's list
    double rc2;
};

// T: [walker][2 window + 1]; ntrip likewise
template <int DIM>
__global__ __launch_bounds__(kAtmThreads) void k_atm(
    DevParams P, const double *__restrict__ paths, WalkerList list, AtmArgs A, double *__restrict__ T,
    unsigned long long *__restrict__ ntrip, unsigned long long *__restrict__ samples)
{
    extern __shared__ double lds[];
    const int Np = P.Np, NpPad = P.NpPad, cap = A.cap;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    double *sx = lds;                                                       // DIM x Np: the slice
    double *lx = sx + (size_t)DIM * Np + (size_t)wave * (DIM + 1) * cap;    // this wave's legs: x_k at [k cap + m], a2 at [DIM cap + m]
    double *la = lx + (size_t)DIM * cap;
    double *red = sx + (size_t)DIM * Np + (size_t)kAtmWaves * (DIM + 1) * cap;   // kAtmWaves sums, then kAtmWaves counts
    unsigned int *redn = reinterpret_cast<unsigned int *>(red + kAtmWaves);

    const int ns = 2 * A.window + 1;
    const int js = blockIdx.x / A.n, slot = blockIdx.x - js * A.n;
    const int w = list.w[slot];
    const int a = P.Nb - A.window + js;
    const double *Sa = window_slice<DIM>(P, paths, w, a);

    for (int t = threadIdx.x; t < DIM * Np; t += blockDim.x) {
        const int k = t / Np, ii = t - k * Np;
        sx[t] = Sa[(size_t)k * NpPad + ii];
    }
    __syncthreads();

    const double rc2 = A.rc2;
    double sum = 0.0;
    unsigned int cnt = 0u;
    for (int i = wave; i < Np - 2; i += kAtmWaves) {
        double xi[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) xi[k] = sx[k * Np + i];
        // pass 1: the legs j > i of i, compacted in ascending j
        int n = 0;
        for (int j0 = i + 1; j0 < Np; j0 += kWave) {
            const int j = j0 + lane;
            double xj[DIM], a2 = 0.0;
            bool leg = false;
            if (j < Np) {
                double d[DIM];
#pragma unroll
                for (int k = 0; k < DIM; ++k) { xj[k] = sx[k * Np + j]; d[k] = xi[k] - xj[k]; }
                a2 = min_image<DIM>(d, P);
                leg = a2 <= rc2;
            }
            const unsigned long long mask = __ballot(leg);
            if (leg) {
                const int m = n + __popcll(mask & ((1ull << lane) - 1ull));     // m <= Np - 2 < cap
#pragma unroll
                for (int k = 0; k < DIM; ++k) lx[k * cap + m] = xj[k];
                la[m] = a2;
            }
            n += __popcll(mask);
        }
        __builtin_amdgcn_wave_barrier();
        // pass 2: the pairs of legs, rows m and n - 2 - m of the triangle joined to n entries
        if (n >= 2) {
            const int total = (n >> 1) * n, q64 = kWave / n, r64 = kWave - q64 * n;
            int row = lane / n, col = lane - row * n;
            for (int t = lane; t < total; t += kWave) {
                const int first = n - 1 - row;                              // entries of row `row`
                int j, k;
                bool ok = true;
                if (col < first) { j = row; k = row + 1 + col; }
                else { j = n - 2 - row; k = j + 1 + (col - first); ok = j != row; }
                if (ok) {
                    double d[DIM];
#pragma unroll
                    for (int e = 0; e < DIM; ++e) d[e] = lx[e * cap + j] - lx[e * cap + k];
                    const double c2 = min_image<DIM>(d, P);
                    if (c2 <= rc2) {
                        const double a2 = la[j], b2 = la[k];
                        const double p = (a2 * b2) * c2;
                        const double s = sqrt(p);
                        const double num = ((a2 + b2 - c2) * (a2 + c2 - b2)) * (b2 + c2 - a2);
                        sum = sum + (p + 0.375 * num) / ((p * p) * s);
                        ++cnt;
                    }
                }
                row += q64;
                col += r64;
                if (col >= n) { col -= n; ++row; }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }

    sum = wave_sum(sum);
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off, kWave);
    if (lane == 0) { red[wave] = sum; redn[wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double v = 0.0;
        unsigned long long c = 0ull;
        for (int q = 0; q < kAtmWaves; ++q) { v += red[q]; c += redn[q]; }
        const size_t e = (size_t)w * ns + js;
        T[e] = T[e] + v;
        ntrip[e] = ntrip[e] + c;
        if (js == 0) samples[w] = samples[w] + 1ull;
    }
}

} // namespace

AtmShape atm_shape(int dim, int Np)
{
    AtmShape s{};
    s.cap = Np;
    s.lds = sizeof(double) * (size_t)dim * (size_t)Np +
            (size_t)kAtmWaves * (size_t)s.cap * sizeof(double) * ((size_t)dim + 1) + kAtmLdsTail;
    s.fits = s.lds <= kAtmLdsBudget;
    return s;
}

hipError_t launch_atm(const DevParams &P, const double *paths, int n, const WalkerList &list, const AtmShape &s, int window,
                      double rc2, double *T, unsigned long long *ntrip, unsigned long long *samples, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    if (n > kWalkerListMax || !s.fits || P.dim < 2) return hipErrorInvalidValue;
    AtmArgs A{};
    A.window = window; A.n = n; A.cap = s.cap; A.rc2 = rc2;
    const int ns = 2 * window + 1;
    return with_flag(P.dim == 2, [&](auto D2) {
        return launch<k_atm<D2() ? 2 : 3>>(dim3(n * ns), dim3(kAtmThreads), s.lds, st, P, paths, list, A, T, ntrip, samples);
    });
}

} // namespace pigs
