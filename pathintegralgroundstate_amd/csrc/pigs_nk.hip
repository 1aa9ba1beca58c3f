// pigs_nk.hip -- the momentum distribution n(k) of a periodic system on the box-commensurate vectors, and the one-body
// density matrix on the Cartesian grid of the minimum-image cell (pigs_nk_*).
//
// The off-diagonal partner of pigs_sqv.hip and pigs_grv.hip.  A sample is the end-to-end vector x = head - tail of an open
// worldline, folded once as the OBDM histogram of the sampler folds it (sample_mod.f90:477-526).  For k = 2 pi (n_1/L_1, ..)
// the phase k.x does not depend on the periodic image, so
//   C[w][iq] += sum over the samples of cos(k_iq . x)
// is an exact finite-box estimator on the vectors of pigs_sqv_* (half space, n = 0 left out: its sum is the number of
// samples, nopen).  The same launch counts per sample
//   H[w][flat]  +1 in bin j_1 + nbin j_2 + nbin^2 j_3, j_k = (int)t_k, t_k = (x_k + LboxHalf[k]) / (Lbox[k]/nbin), iff
//               0 <= t_k < nbin holds in double for every k (pigs_grv_*'s cell and bin-edge rule)
//   nopen[w]    +1
//   ninside[w]  +1 iff r2 <= rcut2 in double, r2 the sum of the squares left to right (the OBDM's own comparison)
//
// k_nk: one workgroup per listed walker.  The samples come from a tape: cnt[j] of them at xs + j * stride, j the walker
// (the sampler's end tape) or the position in the request (pigs_nk_add).  A tile of kNkTile samples is staged in LDS as
// per-axis phasor tables e_k[m] = exp(i real(m) (2 pi/Lbox[k]) x_k), m = 0..nmax, each from one sincos of the phase rounded
// as pigs_sqv_* rounds it; m = 0 gives exactly (1, 0).  A thread owns the vectors iq = tid, tid + threads, ..; for each it
// sums Re(e_1[n_1] e_2[n_2] e_3[n_3]) over the samples in tape order in a register and adds once to C[w][iq].  A tape of at
// most one tile is staged once for all of a thread's vectors; a longer one is staged again per pass of `threads` vectors.
// No floating-point atomics and one fixed order: the same tape gives the same bits, and a walker listed twice (in two
// launches) gives exactly twice one count.  Compile with -ffp-contract=off.
#include "pigs_device.h"
#include "pigs_kernels.h"
#include "pigs_launch.h"
#include "pigs_sqv_device.h"

namespace pigs {

namespace {

struct NkArgs {
    int nmax, nbin, by_walker, base;       // by_walker: the tape is indexed by the walker, else by base + slot
    int cap;                               // samples a tape entry holds at most
    long long Nq;
    unsigned int nvec;                     // nbin^dim
    double b[3], pi;
};

// tab: [k][sample of the tile][m = 0..nmax]
template <int DIM>
__global__ __launch_bounds__(kNkThreads) void k_nk(
    DevParams P, WalkerList list, NkArgs A, const int *__restrict__ cnt, const double *__restrict__ xs,
    double *__restrict__ C, unsigned long long *__restrict__ H, unsigned long long *__restrict__ nopen,
    unsigned long long *__restrict__ ninside)
{
    extern __shared__ c2 tab[];
    const int slot = blockIdx.x, w = list.w[slot];
    const int j = A.by_walker ? w : A.base + slot;
    const int ns = min(cnt[j], A.cap);
    if (ns <= 0) return;                                        // (the whole workgroup)
    const double *X = xs + (size_t)j * A.cap * DIM;             // [sample][k]
    const int ms = A.nmax + 1, S = 2 * A.nmax + 1;
    const double nb = (double)A.nbin;

    // ---- the integer counts: one thread per sample
    for (int i = threadIdx.x; i < ns; i += blockDim.x) {
        double r2 = 0.0;
        bool in = true;
        unsigned int flat = 0, stride = 1;
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            const double v = X[(size_t)i * DIM + k];
            r2 = r2 + v * v;
            const double t = (v + P.LboxHalf[k]) / A.b[k];
            if (t >= 0.0 && t < nb) flat += (unsigned int)(int)t * stride;
            else in = false;
            stride *= (unsigned int)A.nbin;
        }
        if (in) atomicAdd(&H[(size_t)w * A.nvec + flat], 1ull);
        if (r2 <= P.rcut2) atomicAdd(&ninside[w], 1ull);
    }
    if (threadIdx.x == 0) nopen[w] = nopen[w] + (unsigned long long)ns;

    // ---- the cosine sums
    const bool one_tile = ns <= kNkTile;
    for (long long q0 = 0; q0 < A.Nq; q0 += blockDim.x) {
        const long long iq = q0 + threadIdx.x;
        const bool live = iq < A.Nq;
        int nv[DIM];                                            // the vector (pigs_sqv_vectors: rank iq + Nq + 1 among all
        long long r = live ? iq + A.Nq + 1 : 0;                 // S^dim vectors, n_1 slowest)
#pragma unroll
        for (int k = DIM - 1; k >= 0; --k) {
            nv[k] = live ? (int)(r % S) - A.nmax : 0;
            r /= S;
        }
        double sum = 0.0;
        for (int i0 = 0; i0 < ns; i0 += kNkTile) {
            const int nt = min(kNkTile, ns - i0);
            if (!one_tile || q0 == 0) {
                __syncthreads();                                // the previous tile has been consumed
                for (int t = threadIdx.x; t < DIM * nt * ms; t += blockDim.x) {
                    const int k = t / (nt * ms), r = t - k * (nt * ms), il = r / ms, m = r - il * ms;
                    const double qbin = 2.0 * A.pi / P.Lbox[k];
                    const double qr = (double)(float)m * qbin * X[(size_t)(i0 + il) * DIM + k];
                    c2 e;
                    sincos(qr, &e.y, &e.x);
                    tab[((size_t)k * kNkTile + il) * ms + m] = e;
                }
                __syncthreads();
            }
            if (live) {
                for (int il = 0; il < nt; ++il) {
                    const c2 e1 = phasor(tab + (size_t)il * ms, nv[0]);
                    double ar = e1.x, ai = e1.y;
#pragma unroll
                    for (int k = 1; k < DIM; ++k) {
                        const c2 e = phasor(tab + ((size_t)k * kNkTile + il) * ms, nv[k]);
                        const double br = ar * e.x - ai * e.y, bi = ar * e.y + ai * e.x;
                        ar = br; ai = bi;
                    }
                    sum = sum + ar;
                }
            }
        }
        if (live) {
            double *dst = C + (size_t)w * A.Nq + iq;
            *dst = *dst + sum;
        }
    }
}

} // namespace

size_t nk_lds_bytes(int dim, int nmax)
{
    return (size_t)dim * kNkTile * (size_t)(nmax + 1) * sizeof(c2);
}

hipError_t launch_nk(const DevParams &P, int n, const WalkerList &list, int nmax, int nbin, long long Nq, int by_walker,
                     int base, int cap, const int *cnt, const double *xs, double *C, unsigned long long *H,
                     unsigned long long *nopen, unsigned long long *ninside, hipStream_t st)
{
    if (n <= 0 || cap <= 0) return hipSuccess;
    NkArgs A{};
    A.nmax = nmax; A.nbin = nbin; A.by_walker = by_walker; A.base = base; A.cap = cap; A.Nq = Nq;
    A.nvec = 1;
    for (int k = 0; k < P.dim; ++k) { A.nvec *= (unsigned int)nbin; A.b[k] = P.Lbox[k] / (double)nbin; }
    A.pi = acos(-1.0);
    const size_t lds = nk_lds_bytes(P.dim, nmax);
    if (lds > kNkLdsBudget) return hipErrorInvalidValue;
    return with_dim(P.dim, [&](auto D) {
        return launch<k_nk<D()>>(dim3(n), dim3(kNkThreads), lds, st, P, list, A, cnt, xs, C, H, nopen, ninside);
    });
}

} // namespace pigs
