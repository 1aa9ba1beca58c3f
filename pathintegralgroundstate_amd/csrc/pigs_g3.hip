// pigs_g3.hip -- the triplet distribution g3(r, s, cos theta) of a periodic system over a slice window (pigs_g3_*): per
// vertex i the histogram of (|d(j)|, |d(k)|, angle between d(j) and d(k)) over the unordered pairs {j, k} of its legs,
// the partners within rmax = Nr rbin.  include/pigs_hip.h has the definition word for word.
//
// k_g3: one workgroup of kG3Waves waves per (listed walker, window slice a = Nb-window .. Nb+window).
//   * The slice is staged once in LDS (unit-stride rows, 8 dim Np bytes).  A WAVE owns a vertex i; the vertices go round
//     the waves, i = wave, wave + kG3Waves, ...  There is no workgroup barrier inside that loop: a wave only reads the
//     slice and its own list.
//   * Pass 1, the legs.  The lanes take 64 partners j at a time:
//       d_k = x_k(i) - x_k(j), folded by min_image<DIM>, r2 summed left to right (pigs_grv_*'s arithmetic)
//       s = sqrt(r2), u = s / rbin; leg iff j != i, 0 < r2 and u < Nr, in double; NaN and +-Inf compare false
//     A ballot of the legs gives each its place in the wave's list (the count so far plus the legs in lower lanes), so the
//     list is in ascending j: (d_1..d_DIM, s, b = (int)u), SoA with capacity Np per wave.  A vertex has at most Np - 1
//     legs, so the list cannot overflow.  Each leg adds +1 to pair[b].
//   * Pass 2, the triplets.  The n (n - 1) / 2 pairs of the n legs are the rows m = 0..n-2 of a triangle, row m holding
//     the n - 1 - m pairs (m, m+1..n-1).  Row m is joined with row n - 2 - m into one row of exactly n entries, n / 2 joined
//     rows in all (for even n the middle row joins itself and its second half is skipped), and the lanes walk the flat
//     index of that rectangle 64 at a time: (row, col) advance by (64 / n, 64 % n) with one carry, no division in the loop
//     and no lane idle but in the last round.  Per pair:
//       dot = d_1(j) d_1(k) + ..., left to right; c = dot / (s(j) s(k)); v = (c + 1.0) (0.5 Na); NaN drops the triplet
//       q = v < 0 ? 0 : v >= Na ? Na - 1 : (int)v         (the clamp is taken in double: no out-of-range conversion)
//       p = lo Nr - lo (lo - 1) / 2 + (hi - lo), lo <= hi the two radial bins; +1 to trip[p][q]
//     Every operation commutes in (j, k).
//   * HIST_LDS: trip and pair are privatised in LDS as u32 counters, Nr (Nr + 1) / 2 Na + Nr of them, and flushed once
//     per workgroup into the walker's u64 accumulators, empty bins skipped.  A counter gains at most one count per
//     triplet of ONE slice, Np (Np - 1)(Np - 2) / 2 in all (or one per ordered pair, Np (Np - 1), which is less from
//     Np = 4 on and at most 6 below), and g3_shape allows the form only where that is <= 2^32 - 1: no u32 counter can
//     wrap.  Otherwise every count is a global u64 atomic.
//   * The DS instructions of one wave execute in issue order; wave_barrier pins the compiler's order between the list's
//     writes (pass 1), its reads (pass 2) and the next vertex's writes.
// Integer atomics only: the result depends on neither the walker list, its order, the launch split, the form nor the
// context.  Compile with -ffp-contract=off.
// The slice address and its staging are pigs_slice_device.h's.
#include "pigs_kernels.h"
#include "pigs_launch.h"
#include "pigs_slice_device.h"

namespace pigs {

namespace {

struct G3Args {
    int window, Nr, Na, n, cap;            // n: listed walkers of this launch; cap: entries of one wave's list
    double rbin;
};

template <int DIM, bool HIST_LDS>
__global__ __launch_bounds__(kG3Threads) void k_g3(
    DevParams P, const double *__restrict__ paths, WalkerList list, G3Args A, unsigned long long *__restrict__ trip,
    unsigned long long *__restrict__ pair, unsigned long long *__restrict__ samples)
{
    extern __shared__ double lds[];
    const int Np = P.Np, NpPad = P.NpPad, Nr = A.Nr, Na = A.Na, cap = A.cap;
    const int ntrip = (Nr * (Nr + 1) / 2) * Na;
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    double *sx = lds;                                                       // DIM x Np: the slice
    double *ld = sx + (size_t)DIM * Np + (size_t)wave * (DIM + 1) * cap;    // this wave's legs: d_k at [k cap + m], s at [DIM cap + m]
    double *ls = ld + (size_t)DIM * cap;
    int *lb0 = reinterpret_cast<int *>(sx + (size_t)DIM * Np + (size_t)kG3Waves * (DIM + 1) * cap);
    int *lb = lb0 + (size_t)wave * cap;                                     // and their radial bins
    unsigned int *hist = reinterpret_cast<unsigned int *>(lb0 + (size_t)kG3Waves * cap);   // ntrip + Nr (HIST_LDS only)

    const int js = blockIdx.x / A.n, slot = blockIdx.x - js * A.n;
    const int w = list.w[slot];
    const int a = P.Nb - A.window + js;
    const double *Sa = window_slice<DIM>(P, paths, w, a);
    unsigned long long *gt = trip + (size_t)w * ntrip;
    unsigned long long *gp = pair + (size_t)w * Nr;

    stage_rows<DIM>(sx, Np, Sa, NpPad, 0, Np);
    if (HIST_LDS)
        for (int t = threadIdx.x; t < ntrip + Nr; t += blockDim.x) hist[t] = 0u;
    __syncthreads();

    const double nr = (double)Nr, naf = (double)Na, ha = 0.5 * naf;
    for (int i = wave; i < Np; i += kG3Waves) {
        double xi[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) xi[k] = sx[k * Np + i];
        // pass 1: the legs of i, compacted in ascending j
        int n = 0;
        for (int j0 = 0; j0 < Np; j0 += kWave) {
            const int j = j0 + lane;
            double d[DIM], s = 0.0;
            int b = 0;
            bool leg = false;
            if (j < Np) {
#pragma unroll
                for (int k = 0; k < DIM; ++k) d[k] = xi[k] - sx[k * Np + j];
                const double r2 = min_image<DIM>(d, P);
                s = sqrt(r2);
                const double u = s / A.rbin;
                leg = j != i && 0.0 < r2 && u < nr;
                if (leg) b = (int)u;
            }
            const unsigned long long mask = __ballot(leg);
            if (leg) {
                const int m = n + __popcll(mask & ((1ull << lane) - 1ull));     // m <= Np - 2 < cap
#pragma unroll
                for (int k = 0; k < DIM; ++k) ld[k * cap + m] = d[k];
                ls[m] = s;
                lb[m] = b;
                if (HIST_LDS) atomicAdd(&hist[ntrip + b], 1u);
                else atomicAdd(&gp[b], 1ull);
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
                    double dot = ld[j] * ld[k];
#pragma unroll
                    for (int e = 1; e < DIM; ++e) dot = dot + ld[e * cap + j] * ld[e * cap + k];
                    const double c = dot / (ls[j] * ls[k]);
                    const double v = (c + 1.0) * ha;
                    if (v == v) {
                        const int q = v < 0.0 ? 0 : (v >= naf ? Na - 1 : (int)v);
                        const int bj = lb[j], bk = lb[k];
                        const int lo = min(bj, bk), hi = max(bj, bk);
                        const int idx = (lo * Nr - lo * (lo - 1) / 2 + (hi - lo)) * Na + q;
                        if (HIST_LDS) atomicAdd(&hist[idx], 1u);
                        else atomicAdd(&gt[idx], 1ull);
                    }
                }
                row += q64;
                col += r64;
                if (col >= n) { col -= n; ++row; }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (HIST_LDS) {
        __syncthreads();
        for (int t = threadIdx.x; t < ntrip + Nr; t += blockDim.x) {
            const unsigned int c = hist[t];
            if (c) atomicAdd(t < ntrip ? &gt[t] : &gp[t - ntrip], (unsigned long long)c);
        }
    }
    if (js == 0 && threadIdx.x == 0) atomicAdd(&samples[w], 1ull);
}

} // namespace

G3Shape g3_shape(int dim, int Np, int Nr, int Na, int form)
{
    G3Shape s{};
    s.cap = Np;
    const size_t slice = sizeof(double) * (size_t)dim * (size_t)Np;
    const size_t lists = (size_t)kG3Waves * (size_t)s.cap * (sizeof(double) * ((size_t)dim + 1) + sizeof(int));
    const size_t hist = sizeof(unsigned int) * ((size_t)Nr * ((size_t)Nr + 1) / 2 * (size_t)Na + (size_t)Nr);
    // the most one u32 counter can gain before the flush (in double: exact far beyond any Np that fits)
    const double most = (double)Np * ((double)Np - 1.0) * ((double)Np - 2.0) / 2.0;
    s.fits = slice + lists <= kG3LdsBudget;
    s.hist_fits = s.fits && slice + lists + hist <= kG3LdsBudget && most <= 4294967295.0;
    s.hist_lds = form == 1 || (form < 0 && s.hist_fits);
    s.lds = slice + lists + (s.hist_lds ? hist : 0);
    return s;
}

hipError_t launch_g3(const DevParams &P, const double *paths, int n, const WalkerList &list, const G3Shape &s, int window,
                     int Nr, double rbin, int Na, unsigned long long *trip, unsigned long long *pair,
                     unsigned long long *samples, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    if (!s.fits || (s.hist_lds && !s.hist_fits) || P.dim < 2) return hipErrorInvalidValue;
    G3Args A{};
    A.window = window; A.Nr = Nr; A.Na = Na; A.n = n; A.cap = s.cap; A.rbin = rbin;
    const int ns = 2 * window + 1;
    return with_flag(s.hist_lds, [&](auto H) {
        return with_flag(P.dim == 2, [&](auto D2) {
            return launch<k_g3<D2() ? 2 : 3, H()>>(dim3(n * ns), dim3(kG3Threads), s.lds, st, P, paths, list, A, trip, pair, samples);
        });
    });
}

} // namespace pigs
