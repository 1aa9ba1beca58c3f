// pigs_sqv.hip -- the vector structure factor S(q) of a periodic system on the full reciprocal grid (pigs_sqv_*).
//
// Every other structural estimator here lives on the reference's axis grid (sample_mod.f90:435-476).  This one takes all
// integer vectors n = (n_1..n_dim), |n_k| <= nmax, of the half space (first non-zero component positive), in the order
// that include/pigs_hip.h fixes: ascending lexicographic rank, n_1 slowest.  With S = 2 nmax + 1 and
// Nq = (S^dim - 1)/2 the index of a vector is
//   iqv = sum_k (n_k + nmax) S^(dim-k)  -  Nq  -  1
// (the rank among ALL vectors of the cube minus the rank of n = 0 minus one).  Per walker and call
//   acc[iqv] += sum over a = Nb-W .. Nb+W (ascending) of C(a)^2 + S(a)^2,   C + i S = sum_i exp(i q.x_i(a))
//
// One sincos per (vector, particle) would be thousands per particle.  The work factorises,
//   exp(i q.x) = e_1[n_1] e_2[n_2] e_3[n_3],     e_k[m] = exp(i real(m) qbin_k x_k),  e_k[-m] = conj(e_k[m]),
// with dim*nmax phasors per particle, each from one direct sincos of the phase rounded as k_structure rounds it.
//
// Two launches on the context's stream (the body of the first is sqv_rho_slice in pigs_sqv_device.h, which k_fqv_rho of
// pigs_fqv.hip runs too, keeping C and S instead of their squares):
//   k_sqv_rho2     one workgroup per (listed walker, window slice).  The phasors of a tile of particles are staged in
//                  LDS.  A work item is one prefix (n_1..n_{dim-1}) of the half space (lexicographically >= 0) and one
//                  chunk of kSqvChunk values m = |n_dim|; a thread walks the particles in ascending order, forms the
//                  prefix product a once per particle and adds the four products ar*er, ai*ei, ar*ei, ai*er of every
//                  m to four running sums with one explicit fma each: a e[m] and a conj(e[m]), i.e. n_dim = +m and
//                  -m, are their sums and differences, taken once at the end.  Two fma per (vector, particle) term;
//                  the reads of e_dim[i][m] are the same address for every thread of a chunk (LDS broadcasts).  The
//                  squares C^2 + S^2 go to a scratch of Nq doubles per slice.
//   k_sqv_combine  one thread per (listed walker, vector): the sum over the window slices in ascending order, added to
//                  the accumulator element that this thread alone owns in this launch.
// No floating-point atomics; every sum has one fixed order that depends on neither the walker list nor the launch
// split: the same worldline gives the same bits.  Compile with -ffp-contract=off: only the fma written out is fused.
#include <algorithm>

#include "pigs_kernels.h"
#include "pigs_launch.h"
#include "pigs_slice_device.h"
#include "pigs_sqv_device.h"

namespace pigs {

namespace {

// tab: [k][particle of the tile][m = 0..ms-1], ms = kSqvChunk * nchunk + 1 (sqv_rho_slice, pigs_sqv_device.h)
template <int DIM>
__global__ __launch_bounds__(kSqvThreadsMax) void k_sqv_rho2(
    DevParams P, const double *__restrict__ paths, WalkerList list, int window, int nmax, int tile, int nprefix, int nchunk,
    long long Nq, double pi, double *__restrict__ rho2)
{
    extern __shared__ c2 tab[];
    const int ns = 2 * window + 1;
    const int slot = blockIdx.x / ns, j = blockIdx.x - slot * ns;
    const int w = list.w[slot];
    const double *X = window_slice<DIM>(P, paths, w, P.Nb - window + j);
    sqv_rho_slice<DIM, false>(P, X, tab, nmax, tile, nprefix, nchunk, Nq, pi, rho2 + ((size_t)slot * ns + j) * (size_t)Nq);
}

// rho2: [slot][window slice][iqv]; acc: [walker][iqv]
__global__ __launch_bounds__(256) void k_sqv_combine(
    WalkerList list, int n, int ns, long long Nq, const double *__restrict__ rho2, double *__restrict__ acc,
    unsigned long long *__restrict__ samples)
{
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (size_t)Nq * n) return;
    const int slot = (int)(id / (size_t)Nq);
    const size_t e = id - (size_t)slot * Nq;
    const int w = list.w[slot];
    const double *r = rho2 + (size_t)slot * ns * Nq + e;
    double s = 0.0;
    for (int a = 0; a < ns; ++a) s = s + r[(size_t)a * Nq];
    double *dst = acc + (size_t)w * Nq + e;
    *dst = *dst + s;
    if (e == 0) samples[w] = samples[w] + 1ull;
}

} // namespace

SqvShape sqv_shape(int dim, int nmax)
{
    SqvShape s{};
    long long Sp = 1;
    for (int k = 1; k < dim; ++k) Sp *= 2 * nmax + 1;
    s.Nq = (Sp * (2 * nmax + 1) - 1) / 2;
    s.nprefix = (int)((Sp + 1) / 2);
    s.nchunk = (nmax + kSqvChunk - 1) / kSqvChunk;
    const size_t per = (size_t)dim * (kSqvChunk * s.nchunk + 1) * sizeof(c2);       // table bytes per particle
    s.tile = 64;
    while (s.tile > 8 && s.tile * per > kSqvLdsBudget) s.tile /= 2;
    s.lds = s.tile * per;
    s.threads = std::min(kSqvThreadsMax, 64 * ((s.nprefix * s.nchunk + 63) / 64));
    return s;
}

hipError_t launch_sqv(const DevParams &P, const double *paths, int n, const WalkerList &list, int window, int nmax,
                      double *rho2, double *acc, unsigned long long *samples, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const SqvShape s = sqv_shape(P.dim, nmax);
    const int ns = 2 * window + 1;
    const double pi = acos(-1.0);
    const hipError_t e = with_dim(P.dim, [&](auto D) {
        return launch<k_sqv_rho2<D()>>(dim3(n * ns), dim3(s.threads), s.lds, st, P, paths, list, window, nmax, s.tile, s.nprefix,
                                       s.nchunk, s.Nq, pi, rho2);
    });
    if (e != hipSuccess) return e;
    const size_t total = (size_t)n * s.Nq;
    return launch<k_sqv_combine>(dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, list, n, ns, s.Nq, rho2, acc,
                                 samples);
}

} // namespace pigs
