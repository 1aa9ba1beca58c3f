// pigs_cl.hip -- the cluster-size distribution of a periodic system over a slice window (pigs_cl_*): connected
// components of the bond graph 0 < r2 < rc2, their sizes, the largest one, the bonds and the radius of gyration per size.
// include/pigs_hip.h has the definition word for word.  The first family whose pass is iterative and data dependent; the
// result is a partition, which has no summation order, so the integer sums are unique and rg2 is summed in one fixed order.
//
// k_cl<DIM, ADJ>: one workgroup of kClThreads threads per (listed walker, window slice), the slice staged in LDS
//   (stage_rows, unit-stride rows).  Thread t owns the particles t, t + kClThreads, ..
//   * Neighbour pass.  k_bop's: for its particle a thread walks ALL partners j in ascending order through broadcast LDS
//     reads, d = x(i) - x(j) folded by min_image<DIM>, r2 summed left to right, and marks the bonds of 64 partners in a
//     bit mask (so the particle itself, a coincident partner and a non-finite r2 are no bonds).  The bits with j > i are
//     the slice's bonds.  ADJ (Np <= kClAdjNpMax): the masks are kept as the particle's bit row of ceil(Np/64) u64 in LDS
//     and the sweeps below read the rows; otherwise every sweep computes the distances again.
//   * Labelling (label_components of pigs_cl_device.h, shared with k_pc of pigs_pc.hip).  label[i] = i; then sweeps
//     of (hook) m = min(label[i], label[j] of every bonded j), and where m is
//     smaller, atomicMin of m into label[i] and into label[label[i]]; barrier; (jump) label[i] = label[label[i]]; until
//     a workgroup-wide vote (__syncthreads_or) says that a whole sweep changed nothing.  A label is always the index of a
//     particle of the same component and never above the particle's own index, and labels only fall, so concurrent reads
//     of a sweep may see older or newer values but never wrong ones.  A sweep without a change read final values only:
//     then no bonded pair differs and label[label[i]] == label[i], so a component's labels are all one index L with
//     label[L] == L, and its smallest index m has label[m] <= m inside the component, hence label[m] == m == L.  The
//     number of sweeps follows the data, never a fixed count; the largest one of a launch goes to `sweeps` (atomicMax).
//   * Sizes.  Integer LDS atomics on the root's counter; a root (label[r] == r) adds its size to the slice's u32 size
//     histogram and to the maximum.  The histogram goes to nsize by flush_counts (u32 -> u64, at most Np per counter),
//     the largest size, the bonds and the sample by one thread.
//   * Rg^2.  t_i: the owner of i runs over j = i+1..Np-1 ascending with label[j] == label[i] (singles skip it), the same
//     d, fold and r2 as above.  T: the owner of a root runs over its members ascending, g = T / (s s) in double.
//     G_slice[s]: the owner of size s runs over the roots ascending.  G_slice goes to scratch [slot][slice][Np], zeros
//     for the sizes that did not occur.
// k_cl_combine: one thread per (listed walker, size): rg2 = rg2 + G_slice over the slices in ascending order, by the one
//   owner of that element in the launch -- the host never lists a walker twice in ONE launch.
// No floating-point atomics; nothing in the order depends on the walker list, the launch split, the scratch budget or the
// context.  Compile with -ffp-contract=off.
//
// gfx950 cross-compile (hipcc -O3 -ffp-contract=off --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage):
//   k_cl<1> / <2> / <3>, bit rows:    21 / 28 / 34 VGPRs, no VGPR or SGPR spilled, 0 bytes of scratch memory per lane,
//                                     8 waves per SIMD
//   k_cl<1> / <2> / <3>, recomputed:  25 / 32 / 38 VGPRs, no VGPR or SGPR spilled, 0 bytes of scratch memory per lane,
//                                     8 waves per SIMD
//     both: 256 bytes of static LDS (the vote of __syncthreads_or) beside the dynamic cl_lds_bytes: 21 512 bytes at
//     Np = 256 in 3D with the bit rows, 15 608 bytes at Np = 300 without
//   k_cl_combine:                     11 VGPRs, no spills, no scratch memory, no LDS, 8 waves per SIMD
#include "pigs_kernels.h"
#include "pigs_launch.h"
#include "pigs_slice_device.h"
#include "pigs_cl_device.h"

namespace pigs {

namespace {

// scratch: [slot][2 window + 1][Np]; nsize, nlarge: [walker][Np]
template <int DIM, bool ADJ>
__global__ __launch_bounds__(kClThreads) void k_cl(
    DevParams P, const double *__restrict__ paths, WalkerList list, int window, double rc2, double *__restrict__ scratch,
    unsigned long long *__restrict__ nsize, unsigned long long *__restrict__ nlarge, unsigned long long *__restrict__ nbond,
    unsigned long long *__restrict__ samples, unsigned int *__restrict__ sweeps)
{
    extern __shared__ double lds[];
    const int Np = P.Np, nw = (Np + 63) / 64;
    double *sx = lds;                                                  // DIM x Np: the slice
    double *tt = sx + (size_t)DIM * Np;                                // Np: t_i
    double *gg = tt + Np;                                              // Np: g of the cluster rooted at r
    unsigned long long *adj = reinterpret_cast<unsigned long long *>(gg + Np);   // ADJ: Np x nw bit rows
    int *label = reinterpret_cast<int *>(adj + (ADJ ? (size_t)Np * nw : 0));     // Np
    unsigned int *cnt = reinterpret_cast<unsigned int *>(label + Np);  // Np: members, at the root
    unsigned int *hsz = cnt + Np;                                      // Np: clusters of size s at s - 1
    unsigned int *misc = hsz + Np;                                     // the largest size, the bonds

    const int ns = 2 * window + 1;
    const int slot = blockIdx.x / ns, js = blockIdx.x - slot * ns;
    const int w = list.w[slot];
    const int tid = (int)threadIdx.x;
    const double *S = window_slice<DIM>(P, paths, w, P.Nb - window + js);

    stage_rows<DIM>(sx, Np, S, P.NpPad, 0, Np);
    for (int i = tid; i < Np; i += kClThreads) { label[i] = i; cnt[i] = 0u; hsz[i] = 0u; }
    if (tid < 2) misc[tid] = 0u;
    __syncthreads();

    // ---- neighbour pass (ADJ: the bit rows; otherwise the first sweep counts the bonds)
    unsigned int nb = 0u;
    if (ADJ) {
        for (int i = tid; i < Np; i += kClThreads) {
            double xi[DIM];
#pragma unroll
            for (int k = 0; k < DIM; ++k) xi[k] = sx[k * Np + i];
            for (int j0 = 0, b = 0; j0 < Np; j0 += 64, ++b) {
                const unsigned long long bonds = bond_mask<DIM>(P, sx, Np, xi, j0, min(64, Np - j0), rc2);
                adj[(size_t)i * nw + b] = bonds;                       // (its owner alone reads the row)
                nb += (unsigned int)__popcll(bonds & above(i, j0));
            }
        }
    }

    // ---- labelling: hook and pointer jump until a whole sweep changes nothing
    const unsigned int nsweep = label_components<DIM, ADJ>(P, sx, Np, nw, adj, label, rc2, tid, nb);
    if (tid == 0 && sweeps) atomicMax(sweeps, nsweep);

    // ---- sizes
    for (int i = tid; i < Np; i += kClThreads) atomicAdd(&cnt[label[i]], 1u);
    if (nb) atomicAdd(&misc[1], nb);
    __syncthreads();
    for (int r = tid; r < Np; r += kClThreads) {
        if (label[r] != r) continue;
        const unsigned int s = cnt[r];
        atomicAdd(&hsz[s - 1u], 1u);
        atomicMax(&misc[0], s);
    }

    // ---- t_i: the pairs of a cluster above i, j ascending
    for (int i = tid; i < Np; i += kClThreads) {
        const int li = label[i];
        double t = 0.0;
        if (cnt[li] > 1u) {
            double xi[DIM];
#pragma unroll
            for (int k = 0; k < DIM; ++k) xi[k] = sx[k * Np + i];
            for (int j = i + 1; j < Np; ++j) {
                if (label[j] != li) continue;
                double d[DIM];
#pragma unroll
                for (int k = 0; k < DIM; ++k) d[k] = xi[k] - sx[k * Np + j];
                const double r2 = min_image<DIM>(d, P);
                t = t + r2;
            }
        }
        tt[i] = t;
    }
    __syncthreads();                                                   // tt, hsz and the maximum are complete

    // ---- g of every cluster, by the owner of its root, members ascending
    for (int r = tid; r < Np; r += kClThreads) {
        if (label[r] != r) continue;
        const unsigned int s = cnt[r];
        double T = 0.0;
        unsigned int seen = 0u;
        for (int i = r; i < Np && seen < s; ++i) {
            if (label[i] != r) continue;
            T = T + tt[i];
            ++seen;
        }
        gg[r] = T / ((double)s * (double)s);
    }
    flush_counts(hsz, Np, [&](int t) { return &nsize[(size_t)w * Np + t]; });
    if (tid == 0) {
        atomicAdd(&nlarge[(size_t)w * Np + (misc[0] - 1u)], 1ull);
        if (misc[1]) atomicAdd(&nbond[w], (unsigned long long)misc[1]);
        atomicAdd(&samples[w], 1ull);
    }
    __syncthreads();                                                   // gg is complete

    // ---- G_slice per size, roots ascending
    double *o = scratch + ((size_t)slot * ns + js) * Np;
    for (int t = tid; t < Np; t += kClThreads) {
        double G = 0.0;
        if (hsz[t]) {
            const unsigned int s = (unsigned int)t + 1u;
            for (int r = 0; r < Np; ++r)
                if (label[r] == r && cnt[r] == s) G = G + gg[r];
        }
        o[t] = G;
    }
}

__global__ __launch_bounds__(256) void k_cl_combine(
    WalkerList list, int n, int ns, int Np, const double *__restrict__ scratch, double *__restrict__ rg2)
{
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (size_t)Np * n) return;
    const int slot = (int)(id / (size_t)Np);
    const int e = (int)(id - (size_t)slot * Np);
    const int w = list.w[slot];
    const double *r = scratch + (size_t)slot * ns * Np + e;
    double *dst = rg2 + (size_t)w * Np + e;
    double s = *dst;
    for (int a = 0; a < ns; ++a) s = s + r[(size_t)a * Np];
    *dst = s;
}

} // namespace

size_t cl_lds_bytes(int dim, int Np)
{
    const size_t np = (size_t)Np, nw = (np + 63) / 64;
    return sizeof(double) * ((size_t)dim * np + 2 * np) + (Np <= kClAdjNpMax ? 8 * np * nw : 0) + 4 * (3 * np + 2);
}

size_t cl_slot_doubles(int Np, int window)
{
    return (2 * (size_t)window + 1) * (size_t)Np;
}

hipError_t launch_cl_combine(const WalkerList &list, int n, int ns, int Np, const double *scratch, double *rg2, hipStream_t st)
{
    const size_t total = (size_t)n * Np;
    return launch<k_cl_combine>(dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, list, n, ns, Np, scratch, rg2);
}

hipError_t launch_cl(const DevParams &P, const double *paths, int n, const WalkerList &list, int window, double rc2,
                     double *scratch, unsigned long long *nsize, unsigned long long *nlarge, unsigned long long *nbond,
                     unsigned long long *samples, double *rg2, unsigned int *sweeps, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const int ns = 2 * window + 1;
    if (n > kWalkerListMax || P.Np < 1 || P.Np > kClNpMax || (long long)n * ns > 0x7fffffffll) return hipErrorInvalidValue;
    const size_t lds = cl_lds_bytes(P.dim, P.Np);
    if (lds > kClLdsBudget) return hipErrorInvalidValue;
    const hipError_t e = with_dim(P.dim, [&](auto D) {
        return with_flag(P.Np <= kClAdjNpMax, [&](auto A) {
            return launch<k_cl<D(), A()>>(dim3((unsigned)(n * ns)), dim3(kClThreads), lds, st, P, paths, list, window, rc2, scratch,
                                          nsize, nlarge, nbond, samples, sweeps);
        });
    });
    if (e != hipSuccess) return e;
    return launch_cl_combine(list, n, ns, P.Np, scratch, rg2, st);
}

} // namespace pigs
