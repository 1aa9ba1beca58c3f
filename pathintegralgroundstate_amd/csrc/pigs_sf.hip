// pigs_sf.hip -- the superfluid fraction of a periodic system from the diffusion of the centre of mass along imaginary
// time, and the unfolded displacement of a particle (pigs_sf_*).  include/pigs_hip.h has the definition word for word.
// The first family that follows a worldline link by link: every link x(a+1) - x(a) is folded once (min_image<DIM>) and the
// folded links are added up, so the displacement over a lag has no half-box limit.
//
// k_sf_links: one workgroup of kSfThreads threads per listed walker.  Lane = particle, further particles in rounds of
//   kSfThreads; the links a = Nb-window .. Nb+window-1 in ascending order.  Per link a thread reads its particle's
//   coordinates of the two slices (a row per axis: coalesced), folds the difference, counts the compares that fired, adds
//   the link to the particle's unfolded coordinate U_k(i) (one addition after the other; U of the first window slice is
//   0.0) and writes U to the scratch [slot][window slice][axis][NpPad].  With Np <= kSfThreads a thread keeps its
//   particle's U and previous coordinates in registers; with more it reads back what it wrote itself.
//   The link sum s_k(a): lane j adds the links of the particles j, j + kSfThreads, .. in ascending order from 0.0, the
//   wave's butterfly (wave_sum), and the waves' values wait in LDS, kSfChunk links at a time; after the chunk's barrier
//   thread k < DIM adds the waves in wave order from 0.0 and W_k(a+1) = W_k(a) + s_k(a) goes to the scratch
//   [slot][window slice][axis].  One barrier pair per kSfChunk links, not per link.
//   The wraps are counted per thread, added as u32 in LDS and flushed to the walker's u64.
// k_sf_lags: one workgroup per (listed walker, lag l), queued behind k_sf_links on the same stream.
//   D: lane j takes the particles j, j + kSfThreads, .. ascending and per particle a ascending: s_k = s_k + d d with
//   d = U_k(i,a+l) - U_k(i,a) (two coalesced loads per axis; the scratch of a walker stays in L2 / MALL); then the
//   butterfly, the waves in wave order from 0.0, and acc += value by thread k, the one owner of (w, l, k) in the launch --
//   the host never lists a walker twice in ONE launch.
//   C: thread k < DIM runs over a ascending on W: c = c + d d from 0.0, d = W_k(a+l) - W_k(a); acc += c.
//   The workgroup of lag 0 counts the sample.
// No floating-point atomics; nothing in the order depends on the walker list, the launch split, the scratch budget or the
// context.  Compile with -ffp-contract=off.
//
// gfx950 cross-compile (hipcc -O3 -ffp-contract=off --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage):
//   k_sf_links<1> / <2> / <3>: 94 / 68 / 94 VGPRs, no VGPR or SGPR spilled, 0 bytes of scratch memory per lane,
//                              1 032 / 2 056 / 3 080 bytes of LDS, 5 / 7 / 5 waves per SIMD (the link loop is unrolled; the
//                              grid is one workgroup per walker, so the occupancy is not what bounds it)
//   k_sf_lags<1> / <2> / <3>:  16 / 24 / 34 VGPRs, no VGPR or SGPR spilled, 0 bytes of scratch memory per lane,
//                              32 / 64 / 96 bytes of LDS, 8 waves per SIMD
#include "pigs_kernels.h"
#include "pigs_launch.h"
#include "pigs_slice_device.h"

namespace pigs {

namespace {

constexpr int kSfWaves = kSfThreads / 64;
constexpr int kSfChunk = 32;               // links whose wave sums wait in LDS between two barriers

// U: [slot][ns][DIM][NpPad], Wcm: [slot][ns][DIM]
template <int DIM>
__global__ __launch_bounds__(kSfThreads) void k_sf_links(
    DevParams P, const double *__restrict__ paths, WalkerList list, int window, double *__restrict__ U,
    double *__restrict__ Wcm, unsigned long long *__restrict__ nwrap)
{
    __shared__ double red[kSfChunk * DIM * kSfWaves];
    __shared__ unsigned int wraps;
    const int Np = P.Np, NpPad = P.NpPad, ns = 2 * window + 1;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int slot = blockIdx.x, w = list.w[slot];
    const size_t sl = slice_doubles(DIM, NpPad);
    const double *X = window_slice<DIM>(P, paths, w, P.Nb - window);
    double *Us = U + (size_t)slot * ns * sl;
    double *Ws = Wcm + (size_t)slot * ns * DIM;
    const bool single = Np <= kSfThreads;

    if (tid == 0) wraps = 0u;
    for (int i = tid; i < Np; i += kSfThreads) {
#pragma unroll
        for (int k = 0; k < DIM; ++k) Us[(size_t)k * NpPad + i] = 0.0;
    }
    double Wk = 0.0;                                                        // thread k < DIM: W_k of the current slice
    if (tid < DIM) Ws[tid] = 0.0;
    double ur[DIM], xp[DIM];                                                // single: this thread's particle
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
        ur[k] = 0.0;
        xp[k] = single && tid < Np ? X[(size_t)k * NpPad + tid] : 0.0;
    }
    unsigned int nw = 0u;

    for (int c0 = 0; c0 < ns - 1; c0 += kSfChunk) {
        const int cn = min(kSfChunk, ns - 1 - c0);
        __syncthreads();                                                    // the previous chunk's wave sums have been read
        for (int c = 0; c < cn; ++c) {
            const int a = c0 + c;
            const double *Xa = X + (size_t)a * sl, *Xb = Xa + sl;
            double *Ua = Us + (size_t)a * sl, *Ub = Ua + sl;
            double s[DIM];
#pragma unroll
            for (int k = 0; k < DIM; ++k) s[k] = 0.0;
            for (int i = tid; i < Np; i += kSfThreads) {
                double d[DIM], xn[DIM];
#pragma unroll
                for (int k = 0; k < DIM; ++k) {
                    xn[k] = Xb[(size_t)k * NpPad + i];
                    d[k] = xn[k] - (single ? xp[k] : Xa[(size_t)k * NpPad + i]);
                    nw += (d[k] > P.LboxHalf[k] || d[k] < -P.LboxHalf[k]) ? 1u : 0u;
                }
                min_image<DIM>(d, P);
#pragma unroll
                for (int k = 0; k < DIM; ++k) {
                    const double u = (single ? ur[k] : Ua[(size_t)k * NpPad + i]) + d[k];   // (this thread wrote Ua)
                    Ub[(size_t)k * NpPad + i] = u;
                    s[k] = s[k] + d[k];
                    if (single) { ur[k] = u; xp[k] = xn[k]; }
                }
            }
#pragma unroll
            for (int k = 0; k < DIM; ++k) {
                const double t = wave_sum(s[k]);
                if (lane == 0) red[(c * DIM + k) * kSfWaves + wave] = t;
            }
        }
        __syncthreads();
        if (tid < DIM) {
            for (int c = 0; c < cn; ++c) {
                double v = 0.0;
#pragma unroll
                for (int g = 0; g < kSfWaves; ++g) v = v + red[(c * DIM + tid) * kSfWaves + g];
                Wk = Wk + v;
                Ws[(size_t)(c0 + c + 1) * DIM + tid] = Wk;
            }
        }
    }
    if (nw) atomicAdd(&wraps, nw);                                          // (wraps = 0 lies before the first barrier; with
    __syncthreads();                                                        // one slice there is no link and nw = 0)
    if (tid == 0 && wraps) atomicAdd(&nwrap[w], (unsigned long long)wraps);
}

// C, D: [walker][Ntau + 1][DIM]
template <int DIM>
__global__ __launch_bounds__(kSfThreads) void k_sf_lags(
    int Np, int NpPad, int window, int Ntau, WalkerList list, const double *__restrict__ U, const double *__restrict__ Wcm,
    double *__restrict__ C, double *__restrict__ D, unsigned long long *__restrict__ samples)
{
    __shared__ double red[DIM * kSfWaves];
    const int ns = 2 * window + 1;
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int slot = blockIdx.x / (Ntau + 1), l = blockIdx.x - slot * (Ntau + 1);
    const int w = list.w[slot];
    const size_t sl = slice_doubles(DIM, NpPad);
    const double *Us = U + (size_t)slot * ns * sl;
    const double *Ws = Wcm + (size_t)slot * ns * DIM;

    double s[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) s[k] = 0.0;
    for (int i = tid; i < Np; i += kSfThreads) {
        for (int a = 0; a + l < ns; ++a) {
#pragma unroll
            for (int k = 0; k < DIM; ++k) {
                const double d = Us[(size_t)(a + l) * sl + (size_t)k * NpPad + i] - Us[(size_t)a * sl + (size_t)k * NpPad + i];
                s[k] = s[k] + d * d;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
        const double t = wave_sum(s[k]);
        if (lane == 0) red[k * kSfWaves + wave] = t;
    }
    __syncthreads();
    if (tid < DIM) {
        double v = 0.0;
#pragma unroll
        for (int g = 0; g < kSfWaves; ++g) v = v + red[tid * kSfWaves + g];
        double c = 0.0;
        for (int a = 0; a + l < ns; ++a) {
            const double d = Ws[(size_t)(a + l) * DIM + tid] - Ws[(size_t)a * DIM + tid];
            c = c + d * d;
        }
        const size_t e = ((size_t)w * (Ntau + 1) + l) * DIM + tid;
        D[e] = D[e] + v;
        C[e] = C[e] + c;
    }
    if (l == 0 && tid == 0) samples[w] = samples[w] + 1ull;
}

} // namespace

size_t sf_slot_doubles(int dim, int NpPad, int window)
{
    return (2 * (size_t)window + 1) * slice_doubles(dim, NpPad);
}

hipError_t launch_sf(const DevParams &P, const double *paths, int n, const WalkerList &list, int window, int Ntau, double *U,
                     double *Wcm, double *C, double *D, unsigned long long *nwrap, unsigned long long *samples,
                     hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    if (n > kWalkerListMax || Ntau < 0 || Ntau > 2 * window || (long long)n * (Ntau + 1) > 0x7fffffffll) return hipErrorInvalidValue;
    return with_dim(P.dim, [&](auto Dm) {
        const hipError_t e = launch<k_sf_links<Dm()>>(dim3(n), dim3(kSfThreads), 0, st, P, paths, list, window, U, Wcm, nwrap);
        if (e != hipSuccess) return e;
        return launch<k_sf_lags<Dm()>>(dim3((unsigned)(n * (Ntau + 1))), dim3(kSfThreads), 0, st, (int)P.Np, (int)P.NpPad, window,
                                       Ntau, list, (const double *)U, (const double *)Wcm, C, D, samples);
    });
}

} // namespace pigs
