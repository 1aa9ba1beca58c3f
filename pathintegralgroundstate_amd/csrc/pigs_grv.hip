// pigs_grv.hip -- the pair distribution of a periodic system on the vector grid, over a slice window (pigs_grv_*).
//
// The real-space partner of pigs_sqv.hip.  For every listed walker, every slice a = Nb-window .. Nb+window and every pair
// i < j (include/pigs_hip.h has the definition word for word):
//   d_k  = x_k(i) - x_k(j), folded once as pbc_mod.f90:40-41 does (min_image<DIM>: two compares against LboxHalf)
//   r2   = sum of the squares, left to right, no fused multiply-adds
//   vec    +1 in bin j_1 + Nbin j_2 + Nbin^2 j_3, j_k = (int)t_k, t_k = (d_k + LboxHalf[k]) / b_k, b_k = Lbox[k]/Nbin,
//          iff 0 <= t_k < Nbin holds in double for every k (decided BEFORE any conversion to an integer)
//   radial +1 in bin (int)u, u = sqrt(r2)/rbin, iff r2 <= rcut2 and u < Nr (K7's rule, once per pair)
// Counts are integers: LDS u32 and global u64 atomics only, so the result depends on neither the walker list, the launch
// split nor the context.  Compile with -ffp-contract=off.
//
// k_grv: a workgroup takes a listed walker and a run of its window slices.
//   * The slice is staged in LDS in tiles of kGrvTile particles (unit-stride global reads), two tiles A <= B at a time;
//     Np beyond one tile makes several trips over the tile pairs.
//   * The pairs of a tile pair are one flat index range that the threads share out evenly.  A == B (m particles): the
//     cyclic enumeration, element e = (s-1) m + c takes particle c and its partner (c + s) mod m, s = 1..m/2; for even m
//     the last s keeps c < m/2 only.  A < B: the full m_A x m_B rectangle.  In both, consecutive lanes read consecutive
//     LDS addresses, and d keeps the sign of x(lower index) - x(higher index).
//   * VEC_LDS: the vector grid is privatised in LDS as u32 counts and the workgroup keeps it across its whole run of
//     slices -- per (walker, slice) a 32^3 grid has as many bins as an Np = 256 slice has pairs, so a flush per slice would
//     cost as much as the counting.  Otherwise the grid takes global u64 atomics and the run is one slice.
//   * The radial histogram is privatised in LDS up to kDensLdsBins bins, global beyond, as in k_density.
//   * u32 overflow: the host sets flush_every so that flush_every * Np (Np - 1) / 2 <= 2^32 - 1; a bin can gain at most
//     one count per pair, so no LDS counter can wrap between two flushes.  Flushes skip empty bins.
#include <algorithm>

#include "pigs_device.h"
#include "pigs_kernels.h"
#include "pigs_launch.h"

namespace pigs {

namespace {

struct GrvArgs {
    int window, Nbin, Nr, nchunk;          // nchunk runs of slices per walker
    int flush_every;                       // slices between two flushes of the LDS counters
    unsigned int nvec;                     // Nbin^dim (VEC_LDS: the LDS grid)
    double b[3], rbin;
};

// add the non-empty LDS counters to the walker's 64-bit accumulators and clear them
__device__ __forceinline__ void grv_flush(unsigned int *hist, unsigned int n, unsigned long long *base, int w)
{
    unsigned long long *dst = base + (size_t)w * n;
    for (unsigned int t = threadIdx.x; t < n; t += blockDim.x) {
        const unsigned int c = hist[t];
        if (c) {
            atomicAdd(&dst[t], (unsigned long long)c);
            hist[t] = 0u;
        }
    }
}

template <int DIM, bool VEC_LDS, bool RAD_LDS>
__global__ __launch_bounds__(kGrvThreadsMax) void k_grv(
    DevParams P, const double *__restrict__ paths, WalkerList list, GrvArgs A, unsigned long long *__restrict__ vec,
    unsigned long long *__restrict__ radial, unsigned long long *__restrict__ samples)
{
    extern __shared__ double lds[];
    double *sa = lds;                                   // DIM x kGrvTile: tile A
    double *sb = lds + DIM * kGrvTile;                  // DIM x kGrvTile: tile B
    unsigned int *hrad = reinterpret_cast<unsigned int *>(lds + 2 * DIM * kGrvTile);   // Nr (RAD_LDS only)
    unsigned int *hvec = hrad + (RAD_LDS ? A.Nr : 0);                                // nvec (VEC_LDS only)

    const int slot = blockIdx.x / A.nchunk, chunk = blockIdx.x - slot * A.nchunk;
    const int w = list.w[slot];
    const int Np = P.Np, NpPad = P.NpPad;
    const int ns = 2 * A.window + 1;
    const int j0s = (int)((long long)chunk * ns / A.nchunk), j1s = (int)((long long)(chunk + 1) * ns / A.nchunk);
    const double nb = (double)A.Nbin, nr = (double)A.Nr;

    if (RAD_LDS)
        for (int t = threadIdx.x; t < A.Nr; t += blockDim.x) hrad[t] = 0u;
    if (VEC_LDS)
        for (unsigned int t = threadIdx.x; t < A.nvec; t += blockDim.x) hvec[t] = 0u;
    // (ordered before the first count by the first staging's barriers)

    for (int js = j0s; js < j1s; ++js) {
        const double *S = paths + ((size_t)w * P.M + (P.Nb - A.window + js)) * slice_doubles(DIM, NpPad);
        for (int a0 = 0; a0 < Np; a0 += kGrvTile) {
            const int ma = min(kGrvTile, Np - a0);
            __syncthreads();                            // the previous tiles have been consumed
            for (int t = threadIdx.x; t < DIM * ma; t += blockDim.x) {
                const int k = t / ma, ii = t - k * ma;
                sa[k * kGrvTile + ii] = S[(size_t)k * NpPad + a0 + ii];
            }
            for (int b0 = a0; b0 < Np; b0 += kGrvTile) {
                const bool diag = b0 == a0;
                const int mb = min(kGrvTile, Np - b0);
                const double *sj = diag ? sa : sb;
                if (!diag) {
                    __syncthreads();
                    for (int t = threadIdx.x; t < DIM * mb; t += blockDim.x) {
                        const int k = t / mb, ii = t - k * mb;
                        sb[k * kGrvTile + ii] = S[(size_t)k * NpPad + b0 + ii];
                    }
                }
                __syncthreads();
                // element e = row * ma + c, c = column (tile A); rows: the shifts s = row + 1 (diag) or tile B's particles
                const int npairs = diag ? ma * (ma - 1) / 2 : ma * mb;
                const int step_r = (int)blockDim.x / ma, step_c = (int)blockDim.x - step_r * ma;
                int row = (int)threadIdx.x / ma, c = (int)threadIdx.x - row * ma;
                for (int e = threadIdx.x; e < npairs; e += blockDim.x) {
                    int lo = c, hi = row;               // rectangle: A's particle comes first
                    if (diag) {
                        int p = c + row + 1;
                        if (p >= ma) p -= ma;
                        lo = min(c, p);
                        hi = max(c, p);
                    }
                    double d[DIM];
#pragma unroll
                    for (int k = 0; k < DIM; ++k) d[k] = sa[k * kGrvTile + lo] - sj[k * kGrvTile + hi];
                    const double r2 = min_image<DIM>(d, P);
                    // vector grid: the decision in double, the conversion after it
                    bool in = true;
                    unsigned int flat = 0, stride = 1;
#pragma unroll
                    for (int k = 0; k < DIM; ++k) {
                        const double t = (d[k] + P.LboxHalf[k]) / A.b[k];
                        if (t >= 0.0 && t < nb) flat += (unsigned int)(int)t * stride;
                        else in = false;
                        stride *= (unsigned int)A.Nbin;
                    }
                    if (in) {
                        if (VEC_LDS) atomicAdd(&hvec[flat], 1u);
                        else atomicAdd(&vec[(size_t)w * A.nvec + flat], 1ull);
                    }
                    if (r2 <= P.rcut2) {
                        const double u = sqrt(r2) / A.rbin;
                        if (u < nr) {
                            if (RAD_LDS) atomicAdd(&hrad[(int)u], 1u);
                            else atomicAdd(&radial[(size_t)w * A.Nr + (int)u], 1ull);
                        }
                    }
                    row += step_r;
                    c += step_c;
                    if (c >= ma) { c -= ma; ++row; }
                }
            }
        }
        if ((js - j0s + 1) % A.flush_every == 0 && js + 1 < j1s) {   // flush_every slices counted since the last flush
            __syncthreads();
            if (RAD_LDS) grv_flush(hrad, (unsigned int)A.Nr, radial, w);
            if (VEC_LDS) grv_flush(hvec, A.nvec, vec, w);
            // (the next slice's staging barriers order the cleared counters before its counts)
        }
    }
    __syncthreads();
    if (RAD_LDS) grv_flush(hrad, (unsigned int)A.Nr, radial, w);
    if (VEC_LDS) grv_flush(hvec, A.nvec, vec, w);
    if (chunk == 0 && threadIdx.x == 0) atomicAdd(&samples[w], 1ull);
}

} // namespace

GrvShape grv_shape(int dim, int Np, int Nbin, int Nr, int window, int form, int n_list, int n_cu)
{
    GrvShape s{};
    const int ns = 2 * window + 1;
    const unsigned long long pairs = (unsigned long long)Np * (unsigned long long)(Np - 1) / 2;   // per slice
    const unsigned long long u32max = 0xffffffffull;
    unsigned long long nvec = 1;
    for (int k = 0; k < dim; ++k) nvec *= (unsigned long long)Nbin;
    const size_t stage = (size_t)2 * dim * kGrvTile * sizeof(double);
    // radial: in LDS up to kDensLdsBins (a slice's pairs must fit a u32 counter), global beyond
    s.rad_lds = Nr <= kDensLdsBins && pairs <= u32max;
    const size_t base = stage + (s.rad_lds ? (size_t)Nr * sizeof(unsigned int) : 0);
    s.vec_fits = pairs <= u32max && base + nvec * sizeof(unsigned int) <= kGrvLdsBudget;
    s.vec_lds = form == 1 || (form < 0 && s.vec_fits && nvec <= (unsigned long long)kGrvAutoLdsBins);
    if (s.vec_lds && !s.vec_fits) return s;             // forced, and it does not fit: the caller refuses
    s.lds = base + (s.vec_lds ? (size_t)nvec * sizeof(unsigned int) : 0);
    if (s.vec_lds) {
        // as many runs per walker as fill the chip with the workgroups that fit a CU's LDS, but runs long enough that
        // the flush (nvec bins) stays below a quarter of the counting (slices x pairs)
        const int per_cu = (int)std::max<size_t>(1, std::min<size_t>(8, kGrvLdsBudget / s.lds));
        long long want = ((long long)n_cu * per_cu + n_list - 1) / std::max(1, n_list);
        const long long cap = (long long)std::max<unsigned long long>(1, (unsigned long long)ns * pairs / (4 * nvec));
        want = std::min(want, cap);
        s.nchunk = (int)std::max<long long>(1, std::min<long long>(want, ns));
        s.threads = s.lds > 80 * 1024 ? 1024 : s.lds > 40 * 1024 ? 512 : 256;
    } else {
        s.nchunk = ns;                                  // one workgroup per (walker, slice)
        s.threads = 256;
    }
    // u32 counters: at most one count per pair and bin, so flush_every * pairs <= 2^32 - 1 keeps them from wrapping
    const int longest = (ns + s.nchunk - 1) / s.nchunk;
    const unsigned long long safe = pairs ? u32max / pairs : (unsigned long long)longest;
    s.flush_every = (int)std::max<unsigned long long>(1, std::min<unsigned long long>(safe, (unsigned long long)longest));
    return s;
}

hipError_t launch_grv(const DevParams &P, const double *paths, int n, const WalkerList &list, const GrvShape &s, int window,
                      int Nbin, int Nr, double rbin, unsigned long long *vec, unsigned long long *radial,
                      unsigned long long *samples, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    GrvArgs A{};
    A.window = window; A.Nbin = Nbin; A.Nr = Nr; A.nchunk = s.nchunk; A.flush_every = s.flush_every;
    A.nvec = 1;
    for (int k = 0; k < P.dim; ++k) { A.nvec *= (unsigned int)Nbin; A.b[k] = P.Lbox[k] / (double)Nbin; }
    A.rbin = rbin;
    return with_flag(s.vec_lds, [&](auto V) {
        return with_flag(s.rad_lds, [&](auto R) {
            return with_dim(P.dim, [&](auto D) {
                return launch<k_grv<D(), V(), R()>>(dim3(n * s.nchunk), dim3(s.threads), s.lds, st, P, paths, list, A, vec, radial,
                                                    samples);
            });
        });
    });
}

} // namespace pigs
