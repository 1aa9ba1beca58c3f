// pigs_vh.hip -- the van Hove functions of a periodic system over a slice window (pigs_vh_*): the histograms of
// |x_i(a+l) - x_j(a)| for i != j (distinct part, G_d) and for j = i (self part, G_s), per lag l = 0..Ntau.
// include/pigs_hip.h has the definition word for word.
//
// k_vh: one workgroup per (listed walker, base slice a = Nb-window .. Nb+window).
//   * Slice a is staged once in LDS (unit-stride rows, 8 dim Np bytes) and serves every lag of this base slice,
//     l = 0 .. min(Ntau, Nb+window-a): Ntau + 1 partner walks per staging.
//   * For each lag the particles of slice a+l are the OWNERS: they come straight from global memory into registers
//     (coalesced; every window slice is read by up to Ntau + 1 workgroups, so these reads hit the caches), and each is
//     walked against the partners j of slice a through LDS reads:
//       d_k = x_k(i, a+l) - x_k(j, a), folded by min_image<DIM>, r2 summed left to right (pigs_grv_*'s arithmetic)
//       j != i: +1 in dist bin (int)u, u = sqrt(r2)/rbin, iff r2 <= rcut2 and u < Nr      (K7's radial rule)
//       j == i: +1 in self bin (int)u, u = sqrt(r2)/sbin, iff u < Ns                       (no rcut)
//     every decision in double before the conversion; NaN and +-Inf compare false and drop out.  Lag 0 takes the same
//     walk, so it counts every unordered pair twice: dist[0] = 2 x pigs_grv_*'s radial.
//   * Owner rounds.  The owners go in rounds of blockDim.  A round of r owners is shared among G = blockDim / rp groups
//     of threads, rp the power of two >= r: thread t takes owner t % rp and the partners [g Np / G, (g + 1) Np / G) of
//     group g = t / rp.  A full round has G = 1 and every lane of a wave reads the same partner (an LDS broadcast); the
//     last round of Np = 257 has G = 256 and each thread visits one or two partners instead of one lane walking 257.
//   * HIST_LDS: the histograms of all lags are privatised in LDS as u32 counters, (Ntau + 1)(Nr + Ns) of them, and
//     flushed once per workgroup into the walker's u64 accumulators, empty bins skipped.  A counter gains at most one
//     count per (owner, partner) of ONE lag of ONE base slice, Np^2 in all, and Np^2 <= 2^32 - 1 up to Np = 65535, beyond
//     what the staged slice allows (8 dim Np <= kVhLdsBudget): no u32 counter can wrap.  Otherwise (the histograms do not
//     fit beside the slice) every count is a global u64 atomic.
//   * Balance.  A base slice near the window's upper end has fewer lags.  The grid is slice-major, walker-minor, so the
//     workgroups with all their lags are dispatched first and the short ones fill in the launch's tail.
// Integer atomics only: the result depends on neither the walker list, its order, the launch split, the form nor the
// context.  Compile with -ffp-contract=off.  The slice address, the staging and the flush are
// pigs_slice_device.h's.
#include "pigs_kernels.h"
#include "pigs_launch.h"
#include "pigs_slice_device.h"

namespace pigs {

namespace {

struct VhArgs {
    int window, Ntau, Nr, Ns, n;           // n: listed walkers of this launch
    double rbin, sbin;
};

template <int DIM, bool HIST_LDS>
__global__ __launch_bounds__(kVhThreads) void k_vh(
    DevParams P, const double *__restrict__ paths, WalkerList list, VhArgs A, unsigned long long *__restrict__ self,
    unsigned long long *__restrict__ dist, unsigned long long *__restrict__ samples)
{
    extern __shared__ double lds[];
    const int Np = P.Np, NpPad = P.NpPad, Nr = A.Nr, Ns = A.Ns, per = Nr + Ns;
    double *sx = lds;                                                       // DIM x Np: slice a
    unsigned int *hist = reinterpret_cast<unsigned int *>(sx + (size_t)DIM * Np);   // (Ntau + 1) x (Nr + Ns) (HIST_LDS only)

    const int js = blockIdx.x / A.n, slot = blockIdx.x - js * A.n;          // slice-major: the long workgroups first
    const int w = list.w[slot];
    const int a = P.Nb - A.window + js;
    const int nlag = min(A.Ntau, 2 * A.window - js) + 1;                    // a + l <= Nb + window
    const double *Sa = window_slice<DIM>(P, paths, w, a);

    stage_rows<DIM>(sx, Np, Sa, NpPad, 0, Np);
    if (HIST_LDS)
        for (int t = threadIdx.x; t < nlag * per; t += blockDim.x) hist[t] = 0u;
    __syncthreads();

    const double nr = (double)Nr, nsf = (double)Ns;
    const double inf = __builtin_huge_val();
    const int T = (int)blockDim.x;
    for (int l = 0; l < nlag; ++l) {
        const double *Sl = Sa + (size_t)l * slice_doubles(DIM, NpPad);      // slice a + l
        unsigned int *hl = hist + l * per;
        unsigned long long *gd = dist + ((size_t)w * (A.Ntau + 1) + l) * Nr;
        unsigned long long *gs = self + ((size_t)w * (A.Ntau + 1) + l) * Ns;
        for (int base = 0; base < Np; base += T) {
            const int r = min(T, Np - base);
            int rp = 1;
            while (rp < r) rp <<= 1;                                        // T is a power of two: rp <= T
            const int G = T / rp;
            const int g = (int)threadIdx.x / rp, i = base + ((int)threadIdx.x - g * rp);
            if (i >= Np) continue;                                          // (no barrier below)
            const int j0 = (int)((long long)g * Np / G), j1 = (int)((long long)(g + 1) * Np / G);
            double xi[DIM];
#pragma unroll
            for (int k = 0; k < DIM; ++k) xi[k] = Sl[(size_t)k * NpPad + i];
#pragma unroll 2
            for (int j = j0; j < j1; ++j) {
                double d[DIM];
#pragma unroll
                for (int k = 0; k < DIM; ++k) d[k] = xi[k] - sx[k * Np + j];
                const double r2 = min_image<DIM>(d, P);
                const bool same = j == i;
                if (r2 <= (same ? inf : P.rcut2)) {
                    const double u = sqrt(r2) / (same ? A.sbin : A.rbin);
                    if (u < (same ? nsf : nr)) {
                        const int b = (int)u;
                        if (HIST_LDS) atomicAdd(&hl[same ? Nr + b : b], 1u);
                        else atomicAdd(same ? &gs[b] : &gd[b], 1ull);
                    }
                }
            }
        }
    }
    if (HIST_LDS) {
        __syncthreads();
        flush_counts(hist, nlag * per, [&](int t) {
            const int l = t / per, b = t - l * per;
            const size_t wl = (size_t)w * (A.Ntau + 1) + l;
            return b < Nr ? &dist[wl * Nr + b] : &self[wl * Ns + (b - Nr)];
        });
    }
    if (js == 0 && threadIdx.x == 0) atomicAdd(&samples[w], 1ull);
}

} // namespace

VhShape vh_shape(int dim, int Np, int Ntau, int Nr, int Ns, int form)
{
    VhShape s{};
    const size_t slice = sizeof(double) * (size_t)dim * (size_t)Np;
    const size_t hist = sizeof(unsigned int) * (size_t)(Ntau + 1) * ((size_t)Nr + (size_t)Ns);
    s.slice_fits = slice <= kVhLdsBudget;
    s.hist_fits = s.slice_fits && slice + hist <= kVhLdsBudget;
    s.hist_lds = form == 1 || (form < 0 && s.hist_fits);
    s.lds = slice + (s.hist_lds ? hist : 0);
    return s;
}

hipError_t launch_vh(const DevParams &P, const double *paths, int n, const WalkerList &list, const VhShape &s, int window,
                     int Ntau, int Nr, double rbin, int Ns, double sbin, unsigned long long *self, unsigned long long *dist,
                     unsigned long long *samples, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    if (!s.slice_fits || (s.hist_lds && !s.hist_fits)) return hipErrorInvalidValue;
    VhArgs A{};
    A.window = window; A.Ntau = Ntau; A.Nr = Nr; A.Ns = Ns; A.n = n; A.rbin = rbin; A.sbin = sbin;
    const int ns = 2 * window + 1;
    return with_flag(s.hist_lds, [&](auto H) {
        return with_dim(P.dim, [&](auto D) {
            return launch<k_vh<D(), H()>>(dim3(n * ns), dim3(kVhThreads), s.lds, st, P, paths, list, A, self, dist, samples);
        });
    });
}

} // namespace pigs
