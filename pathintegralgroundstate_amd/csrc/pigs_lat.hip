// pigs_lat.hip -- a crystal seen from its lattice, over a slice window (pigs_lat_*): every particle of a window slice is
// assigned to its nearest lattice site; the moments and histograms of the displacement from that site, the occupation of
// the sites and the hops of a particle between sites along imaginary time.  include/pigs_hip.h has the definition word
// for word.  The first family that takes the lattice as input: the sites sit in device memory as a slice does, dim rows
// of NsPad doubles.
//
// k_lat: one workgroup of kLatThreads threads per (listed walker, window slice a = Nb-window .. Nb+window).
//   * Assignment.  The particles go round the threads, i = thread, thread + kLatThreads, ..; a thread keeps its particle
//     in registers.  The site rows are staged in LDS in tiles of kLatTile sites (stage_rows; every lane of a wave reads
//     the same site: an LDS broadcast), and per site
//       d_k = x_k(i) - R_k(s), folded by min_image<DIM>, r2 summed left to right (pigs_grv_*'s arithmetic)
//       r2 < best, strictly, s ascending, best = +inf at first: the smallest s of the minimal r2; NaN and +inf never win
//     u(i) is recomputed from the winner's row (the same operations, so the same bits) and parked in LDS; a lost particle
//     parks 0.0, which leaves the running sums below bit for bit (they start at +0.0 and cannot reach -0.0).
//   * Centre of mass.  Thread k < DIM adds u_k(i) for i = 0 .. Np-1 from 0.0, one addition after the other, and divides by
//     the number of assigned particles: Np additions against Np nsite distances.
//   * Moments.  v = u - c.  A lane adds |v|^2, |v|^4 and v_k^2 of its particles in ascending i, the wave's butterfly
//     (wave_sum), the waves in wave order from 0.0, and `acc += value` last by the one thread that owns (w, a) for the
//     launch -- the host never lists a walker twice in ONE launch.  No floating-point atomics.
//   * Counts.  The occupancy of the sites and the histograms of |v| and of v_k are u32 counters in LDS with integer
//     atomics; a counter gains at most one count per particle, so it cannot wrap.  The occupancy is classified after a
//     barrier (0, 1, 2, >= 3 particles) and the histograms are flushed into the walker's u64 accumulators (flush_counts).
//   * The assigned site of every particle goes, as int32 (-1: lost), to a scratch [slot][window slice][NpPad].
// k_lat_hops: one workgroup per listed walker, queued behind k_lat on the same stream, reads that scratch: a particle
// whose site differs between two successive window slices is a hop (hop1), between the first and the last a hop across
// the window (hopw); a lost end drops the comparison.  It also counts the sample.
// Nothing in the order depends on the walker list, the launch split or the context.  Compile with -ffp-contract=off.
#include "pigs_kernels.h"
#include "pigs_launch.h"
#include "pigs_slice_device.h"

namespace pigs {

namespace {

constexpr int kLatWaves = kLatThreads / 64;

struct LatArgs {
    int window, n, cm;                     // n: listed walkers of this launch
    int nsite, NsPad, nbin;
    double rmax, rbin;                     // rbin = rmax / nbin, of the radial and of the per-axis histograms alike
};

template <int DIM>
__global__ __launch_bounds__(kLatThreads) void k_lat(
    DevParams P, const double *__restrict__ paths, const double *__restrict__ sites, WalkerList list, LatArgs A,
    double *__restrict__ mom, unsigned long long *__restrict__ nassigned, unsigned long long *__restrict__ nlost,
    unsigned long long *__restrict__ occ, unsigned long long *__restrict__ hr, unsigned long long *__restrict__ hx,
    int *__restrict__ sidx)
{
    extern __shared__ double lds[];
    constexpr int NM = 2 + DIM;                                             // moments per (w, a)
    const int Np = P.Np, NpPad = P.NpPad, nsite = A.nsite, nbin = A.nbin;
    const int T = (int)blockDim.x, tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63;
    double *st = lds;                                                       // DIM x kLatTile: a tile of the site rows
    double *su = st + DIM * kLatTile;                                       // DIM x Np: u of every particle
    double *cc = su + (size_t)DIM * Np;                                     // 4: the centre of mass
    double *red = cc + 4;                                                   // kLatWaves x 8: the waves' partial sums
    unsigned int *hocc = reinterpret_cast<unsigned int *>(red + kLatWaves * 8);   // nsite
    unsigned int *hrad = hocc + nsite;                                      // nbin
    unsigned int *hax = hrad + nbin;                                        // DIM x 2 nbin
    unsigned int *cls = hax + DIM * 2 * nbin;                               // 4 classes of occupancy, then the lost
    const int ncount = nsite + nbin + DIM * 2 * nbin + 8;

    const int ns = 2 * A.window + 1;
    const int js = blockIdx.x / A.n, slot = blockIdx.x - js * A.n;
    const int w = list.w[slot];
    const double *Sa = window_slice<DIM>(P, paths, w, P.Nb - A.window + js);
    int *sid = sidx + ((size_t)slot * ns + js) * NpPad;

    for (int t = tid; t < ncount; t += T) hocc[t] = 0u;
    // (ordered before the first count by the first staging's barriers)

    const double inf = __builtin_huge_val();
    for (int base = 0; base < Np; base += T) {
        const int i = base + tid;
        const bool have = i < Np;
        double x[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) x[k] = have ? Sa[(size_t)k * NpPad + i] : 0.0;
        double best = inf;
        int bs = -1;
        for (int s0 = 0; s0 < nsite; s0 += kLatTile) {
            const int m = min(kLatTile, nsite - s0);
            __syncthreads();                                                // the previous tile has been consumed
            stage_rows<DIM>(st, kLatTile, sites, A.NsPad, s0, m);
            __syncthreads();
            if (have) {
#pragma unroll 4
                for (int j = 0; j < m; ++j) {
                    double d[DIM];
#pragma unroll
                    for (int k = 0; k < DIM; ++k) d[k] = x[k] - st[k * kLatTile + j];
                    const double r2 = min_image<DIM>(d, P);
                    if (r2 < best) { best = r2; bs = s0 + j; }
                }
            }
        }
        if (have) {
            double u[DIM];
#pragma unroll
            for (int k = 0; k < DIM; ++k) u[k] = 0.0;
            if (bs >= 0) {
#pragma unroll
                for (int k = 0; k < DIM; ++k) u[k] = x[k] - sites[(size_t)k * A.NsPad + bs];
                min_image<DIM>(u, P);
                atomicAdd(&hocc[bs], 1u);
            } else {
                atomicAdd(&cls[4], 1u);
            }
#pragma unroll
            for (int k = 0; k < DIM; ++k) su[(size_t)k * Np + i] = u[k];
            sid[i] = bs;
        }
    }
    __syncthreads();

    const int nass = Np - (int)cls[4];
    if (tid < DIM) {
        double c = 0.0;
        if (A.cm && nass > 0) {
            const double *row = su + (size_t)tid * Np;
#pragma unroll 8
            for (int i = 0; i < Np; ++i) c = c + row[i];
            c = c / (double)nass;
        }
        cc[tid] = c;
    }
    __syncthreads();

    double s[NM];
#pragma unroll
    for (int q = 0; q < NM; ++q) s[q] = 0.0;
    const double nr = (double)nbin, nx = (double)(2 * nbin);
    for (int i = tid; i < Np; i += T) {
        if (sid[i] < 0) continue;                                           // (this thread wrote it)
        double v[DIM], m2 = 0.0;
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            v[k] = su[(size_t)k * Np + i];
            if (A.cm) v[k] = v[k] - cc[k];
            m2 = m2 + v[k] * v[k];
        }
        s[0] = s[0] + m2;
        s[1] = s[1] + m2 * m2;
#pragma unroll
        for (int k = 0; k < DIM; ++k) s[2 + k] = s[2 + k] + v[k] * v[k];
        const double ur = sqrt(m2) / A.rbin;                               // the decisions in double, the conversion after
        if (ur < nr) atomicAdd(&hrad[(int)ur], 1u);
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            const double t = (v[k] + A.rmax) / A.rbin;
            if (t >= 0.0 && t < nx) atomicAdd(&hax[k * 2 * nbin + (int)t], 1u);
        }
    }
#pragma unroll
    for (int q = 0; q < NM; ++q) {
        const double t = wave_sum(s[q]);
        if (lane == 0) red[wave * 8 + q] = t;
    }
    // the occupancy is complete since the barrier before the centre of mass
    for (int s0 = 0; s0 < nsite; s0 += T) {
        const int sI = s0 + tid;
        const int c = sI < nsite ? (int)min(hocc[sI], 3u) : -1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const unsigned long long b = __ballot(c == q);
            if (lane == 0 && b) atomicAdd(&cls[q], (unsigned int)__popcll(b));
        }
    }
    __syncthreads();

    const size_t e = (size_t)w * ns + js;
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < NM; ++q) {
            double v = 0.0;
            for (int g = 0; g < kLatWaves; ++g) v = v + red[g * 8 + q];
            mom[e * NM + q] = mom[e * NM + q] + v;
        }
        nassigned[e] = nassigned[e] + (unsigned long long)nass;
        if (cls[4]) atomicAdd(&nlost[w], (unsigned long long)cls[4]);
    }
    if (tid < 4) occ[e * 4 + tid] = occ[e * 4 + tid] + cls[tid];
    flush_counts(hrad, nbin, [&](int t) { return &hr[(size_t)w * nbin + t]; });
    flush_counts(hax, DIM * 2 * nbin, [&](int t) { return &hx[(size_t)w * DIM * 2 * nbin + t]; });
}

// sidx: [slot][ns][NpPad] as k_lat left it
__global__ __launch_bounds__(kLatThreads) void k_lat_hops(
    int Np, int NpPad, int ns, WalkerList list, const int *__restrict__ sidx, unsigned long long *__restrict__ hop1,
    unsigned long long *__restrict__ hopw, unsigned long long *__restrict__ samples)
{
    __shared__ unsigned int cnt[2];
    const int slot = blockIdx.x, w = list.w[slot];
    const int *S = sidx + (size_t)slot * ns * NpPad;
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0u;
    __syncthreads();
    unsigned int h1 = 0u, hw = 0u;
    for (int i = threadIdx.x; i < Np; i += blockDim.x) {
        const int first = S[i];
        int prev = first;
        for (int a = 1; a < ns; ++a) {
            const int cur = S[(size_t)a * NpPad + i];
            if (prev >= 0 && cur >= 0 && cur != prev) ++h1;
            prev = cur;
        }
        if (first >= 0 && prev >= 0 && first != prev) ++hw;
    }
    if (h1) atomicAdd(&cnt[0], h1);
    if (hw) atomicAdd(&cnt[1], hw);
    __syncthreads();
    if (threadIdx.x == 0) {
        if (cnt[0]) atomicAdd(&hop1[w], (unsigned long long)cnt[0]);
        if (cnt[1]) atomicAdd(&hopw[w], (unsigned long long)cnt[1]);
        atomicAdd(&samples[w], 1ull);
    }
}

} // namespace

LatShape lat_shape(int dim, int Np, int nsite, int nbin)
{
    LatShape s{};
    s.lds = sizeof(double) * ((size_t)dim * kLatTile + (size_t)dim * (size_t)Np + 4 + (size_t)kLatWaves * 8) +
            sizeof(unsigned int) * ((size_t)nsite + (size_t)nbin * (1 + 2 * (size_t)dim) + 8);
    s.fits = s.lds <= kLatLdsBudget;
    return s;
}

hipError_t launch_lat(const DevParams &P, const double *paths, int n, const WalkerList &list, const LatShape &s, int window,
                      int cm, int nsite, int NsPad, const double *sites, int nbin, double rmax, double *mom,
                      unsigned long long *nassigned, unsigned long long *nlost, unsigned long long *occ,
                      unsigned long long *hr, unsigned long long *hx, unsigned long long *hop1, unsigned long long *hopw,
                      unsigned long long *samples, int *sidx, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    if (n > kWalkerListMax || !s.fits || P.dim < 2) return hipErrorInvalidValue;
    LatArgs A{};
    A.window = window; A.n = n; A.cm = cm; A.nsite = nsite; A.NsPad = NsPad; A.nbin = nbin;
    A.rmax = rmax; A.rbin = rmax / (double)nbin;
    const int ns = 2 * window + 1;
    const hipError_t e = with_flag(P.dim == 2, [&](auto D2) {
        return launch<k_lat<D2() ? 2 : 3>>(dim3(n * ns), dim3(kLatThreads), s.lds, st, P, paths, sites, list, A, mom,
                                           nassigned, nlost, occ, hr, hx, sidx);
    });
    if (e != hipSuccess) return e;
    return launch<k_lat_hops>(dim3(n), dim3(kLatThreads), 0, st, (int)P.Np, (int)P.NpPad, ns, list, (const int *)sidx, hop1,
                              hopw, samples);
}

} // namespace pigs
