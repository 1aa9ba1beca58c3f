// pigs_pc.hip -- wrapping clusters, their unfolded extent and the persistence of clusters along tau (pigs_pc_*), beside
// pigs_cl.hip: which clusters of the bond graph 0 < r2 < rc2 close on themselves through the faces of the box, the finite
// n(s) and the radius of gyration of the finite clusters from unfolded separations, and how many pairs of particles
// that share a cluster in slice a still share one in slice a + l.  include/pigs_hip.h has the definition word for word.
//
// k_pc<DIM, ADJ>: one workgroup of kClThreads threads per (listed walker, window slice), the slice staged in LDS, thread t
//   owning the particles t, t + kClThreads, .. -- k_cl's shape, bit rows (ADJ, Np <= kClAdjNpMax) and labelling loop
//   (label_components of pigs_cl_device.h: one copy for both kernels).  After the labels:
//   * Image numbers.  One LDS word per particle holds the assigned bit (the top one) and DIM fields of m_i[k] + bias; a
//     word is read and written whole (relaxed atomics of workgroup scope), so a reader never sees half an update.  32 bits
//     with fields of 30 (1D) or 15 bits (2D); in 3D 64 bits with fields of 21, because |m_i[k]| can reach Np - 1 = 2047 on a
//     racy path (below) and 3 x 12 bits and the assigned bit pass 32.  Roots start assigned with m = 0.  In a sweep every
//     unassigned particle walks its bonds and takes m_j + n_ij from the first assigned partner it meets; a
//     __syncthreads_or vote ends the sweeps when one assigned nobody.  Such a sweep read final words only, and then no
//     unassigned particle has an assigned partner: every component holds its root, so everybody is assigned.  Which j a
//     particle meets first depends on the timing of the other threads; m_i is the sum of n along a simple path from the
//     root either way (|m_i[k]| <= Np - 1: no field leaves its bits), in a finite cluster every path gives the same sum,
//     and of a wrapping one only the mask is used.  The sweep count follows the data (Np - 1 for a chain whose root is at
//     an end); the largest one goes to sweeps[1] beside the labelling's in sweeps[0].
//   * Wrap mask.  The owner of i runs over its bonds j > i and compares m_i - m_j with n_ij per axis; a mismatch along k
//     sets bit k of the root's mask (integer atomicOr in LDS).  A bond of the spanning structure the sweeps built matches
//     by construction, every other bond closes a walk whose fold numbers add up to the mismatch.
//   * Counts.  cnt[root] by LDS atomics; a root adds 1 and its size to the eight counters of its mask, its mask to the
//     slice's OR, and, when finite, 1 to the slice's u32 histogram of finite sizes.  Out by integer atomics and
//     flush_counts.
//   * rg2u.  k_cl's three fixed-order loops (t_i over j ascending, T over the members ascending, G_slice over the roots
//     ascending) over the FINITE clusters, with du[k] = (x_i[k] - x_j[k]) - c L[k], c = (double)(m_i[k] - m_j[k]): product
//     first, then the subtraction, nothing fused; ru2 summed left to right from 0.0.  G_slice goes to scratch
//     [slot][slice][Np] and k_cl_combine (pigs_cl.hip) adds the slices in ascending order.
//   * The final labels go to an int32 scratch [slot][slice][Np] for k_pc_persist.
// k_pc_persist: one workgroup per (slot, origin a).  The labels of slice a stay in LDS; lag by lag, l = 0..min(ntau, last
//   slice - a), those of slice a + l are staged beside them.  The owner of i walks ALL j (broadcast LDS reads, every
//   thread the same trip count) and counts the ordered pairs j != i that are together in a, in a + l and in both, in
//   u32 (at most Np^2 = 2^22 per workgroup); one wave reduction, one LDS add per wave, and one thread per counter adds
//   half the total -- the unordered pairs -- to its u64 sum by one atomic per (walker, lag, counter).
// No floating-point atomics; nothing in the order depends on the walker list, the launch split, the scratch budget or the
// context.  Compile with -ffp-contract=off.
//
// gfx950 cross-compile (hipcc -O3 -ffp-contract=off --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage):
//   k_pc<1> / <2> / <3>, bit rows:    60 / 60 / 62 VGPRs, no VGPR or SGPR spilled, 0 bytes of scratch memory per lane,
//                                     8 waves per SIMD
//   k_pc<1> / <2> / <3>, recomputed:  62 / 62 / 62 VGPRs, no VGPR or SGPR spilled, 0 bytes of scratch memory per lane,
//                                     8 waves per SIMD
//     both: 256 bytes of static LDS (the vote of __syncthreads_or) beside the dynamic pc_lds_bytes: 24 644 bytes at
//     Np = 256 in 3D with the bit rows, 19 268 bytes at Np = 300 without, 131 140 bytes at Np = kClNpMax = 2048 (of
//     kClLdsBudget = 163 840; the grant of launch<> starts at Np = 1023 in 3D, 1260 in 2D, 1488 in 1D)
//   k_pc_persist:                     50 VGPRs, no spills, no scratch memory, 12 bytes of static LDS beside 8 Np dynamic,
//                                     8 waves per SIMD
//   k_cl with the labelling loop from pigs_cl_device.h keeps the figures of pigs_cl.hip's header, form by form.
#include "pigs_kernels.h"
#include "pigs_launch.h"
#include "pigs_slice_device.h"
#include "pigs_cl_device.h"

#include <type_traits>

namespace pigs {

namespace {

// the packed image numbers of a particle: the assigned bit on top, field k at bit k * bits holding m[k] + bias
template <int DIM>
struct Img {
    using word = std::conditional_t<DIM == 3, unsigned long long, unsigned int>;
    static constexpr int bits = DIM == 1 ? 30 : DIM == 2 ? 15 : 21;
    static constexpr word one = 1;
    static constexpr word assigned = one << (8 * sizeof(word) - 1);
    static constexpr word field_mask = (one << bits) - 1;
    __device__ static constexpr word root()
    {
        word r = assigned;
        for (int k = 0; k < DIM; ++k) r |= (one << (bits - 1)) << (k * bits);
        return r;
    }
    __device__ static __forceinline__ word load(const word *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ static __forceinline__ void store(word *p, word v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ static __forceinline__ int field(word w, int k) { return (int)((w >> (k * bits)) & field_mask); }
    // w with n[k] in {-1, 0, +1} added to field k (no field of an assigned word is 0 or full: no borrow, no carry)
    __device__ static __forceinline__ word plus(word w, const int (&n)[DIM])
    {
#pragma unroll
        for (int k = 0; k < DIM; ++k) w += (word)(std::make_signed_t<word>)n[k] * (one << (k * bits));
        return w;
    }
};

// the fold min_image<DIM> applies to d = x(i) - x(j): +1 where it takes v - L, -1 where it takes v + L
template <int DIM>
__device__ __forceinline__ void fold_numbers(const DevParams &P, const double *sx, int Np, const double (&xi)[DIM], int j,
                                             int (&n)[DIM])
{
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
        const double v = xi[k] - sx[k * Np + j];
        n[k] = v > P.LboxHalf[k] ? 1 : (v < -P.LboxHalf[k] ? -1 : 0);
    }
}

// scratch: [slot][2 window + 1][Np] doubles; labels: the same shape in int32; nwrap, mwrap, swrap: [walker][8];
// nfin: [walker][Np]; sweeps: the labelling's and the image numbers' largest count
template <int DIM, bool ADJ>
__global__ __launch_bounds__(kClThreads) void k_pc(
    DevParams P, const double *__restrict__ paths, WalkerList list, int window, double rc2, double *__restrict__ scratch,
    int *__restrict__ labels, unsigned long long *__restrict__ nwrap, unsigned long long *__restrict__ mwrap,
    unsigned long long *__restrict__ swrap, unsigned long long *__restrict__ nfin, unsigned long long *__restrict__ samples,
    unsigned int *__restrict__ sweeps)
{
    using I = Img<DIM>;
    using word = typename I::word;
    extern __shared__ double lds[];
    const int Np = P.Np, nw = (Np + 63) / 64;
    double *sx = lds;                                                  // DIM x Np: the slice
    double *tt = sx + (size_t)DIM * Np;                                // Np: t_i
    double *gg = tt + Np;                                              // Np: g of the finite cluster rooted at r
    unsigned long long *adj = reinterpret_cast<unsigned long long *>(gg + Np);   // ADJ: Np x nw bit rows
    word *img = reinterpret_cast<word *>(adj + (ADJ ? (size_t)Np * nw : 0));     // Np: the packed image numbers
    int *label = reinterpret_cast<int *>(img + Np);                    // Np
    unsigned int *cnt = reinterpret_cast<unsigned int *>(label + Np);  // Np: members, at the root
    unsigned int *wmask = cnt + Np;                                    // Np: the wrap mask, at the root
    unsigned int *hfin = wmask + Np;                                   // Np: finite clusters of size s at s - 1
    unsigned int *c8 = hfin + Np;                                      // 8: clusters per mask; 8: their particles; the OR
    unsigned int *m8 = c8 + 8;
    unsigned int *sor = m8 + 8;

    const int ns = 2 * window + 1;
    const int slot = blockIdx.x / ns, js = blockIdx.x - slot * ns;
    const int w = list.w[slot];
    const int tid = (int)threadIdx.x;
    const double *S = window_slice<DIM>(P, paths, w, P.Nb - window + js);

    stage_rows<DIM>(sx, Np, S, P.NpPad, 0, Np);
    for (int i = tid; i < Np; i += kClThreads) { label[i] = i; cnt[i] = 0u; wmask[i] = 0u; hfin[i] = 0u; }
    if (tid < 17) c8[tid] = 0u;                                        // c8, m8 and sor
    __syncthreads();

    if (ADJ) {
        for (int i = tid; i < Np; i += kClThreads) {
            double xi[DIM];
#pragma unroll
            for (int k = 0; k < DIM; ++k) xi[k] = sx[k * Np + i];
            for (int j0 = 0, b = 0; j0 < Np; j0 += 64, ++b)
                adj[(size_t)i * nw + b] = bond_mask<DIM>(P, sx, Np, xi, j0, min(64, Np - j0), rc2);   // (its owner alone reads the row)
        }
    }

    // ---- labels
    unsigned int nb = 0u;
    const unsigned int nsweep = label_components<DIM, ADJ>(P, sx, Np, nw, adj, label, rc2, tid, nb);

    // ---- image numbers: the roots assigned, then sweeps until one assigns nobody
    for (int i = tid; i < Np; i += kClThreads) {
        img[i] = label[i] == i ? I::root() : (word)0;
        atomicAdd(&cnt[label[i]], 1u);
    }
    __syncthreads();
    unsigned int isweep = 0u;
    for (;;) {
        int changed = 0;
        for (int i = tid; i < Np; i += kClThreads) {
            if (I::load(&img[i]) & I::assigned) continue;
            double xi[DIM];
#pragma unroll
            for (int k = 0; k < DIM; ++k) xi[k] = sx[k * Np + i];
            bool found = false;
            for (int j0 = 0, b = 0; j0 < Np && !found; j0 += 64, ++b) {
                unsigned long long bonds = ADJ ? adj[(size_t)i * nw + b] : bond_mask<DIM>(P, sx, Np, xi, j0, min(64, Np - j0), rc2);
                while (bonds) {
                    const int j = j0 + __ffsll((long long)bonds) - 1;
                    bonds &= bonds - 1ull;
                    const word wj = I::load(&img[j]);
                    if (!(wj & I::assigned)) continue;
                    int n[DIM];
                    fold_numbers<DIM>(P, sx, Np, xi, j, n);
                    I::store(&img[i], I::plus(wj, n));                 // m_i = m_j + n_ij
                    found = true;
                    changed = 1;
                    break;
                }
            }
        }
        ++isweep;
        if (!__syncthreads_or(changed)) break;
    }
    if (tid == 0) { atomicMax(&sweeps[0], nsweep); atomicMax(&sweeps[1], isweep); }

    // ---- wrap masks: the bonds j > i whose image numbers do not differ by the fold number
    for (int i = tid; i < Np; i += kClThreads) {
        const int li = label[i];
        if (cnt[li] < 2u) continue;
        double xi[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) xi[k] = sx[k * Np + i];
        const word wi = img[i];
        unsigned int mk = 0u;
        for (int j0 = (i + 1) & ~63, b = j0 >> 6; j0 < Np; j0 += 64, ++b) {
            unsigned long long bonds = (ADJ ? adj[(size_t)i * nw + b] : bond_mask<DIM>(P, sx, Np, xi, j0, min(64, Np - j0), rc2)) &
                                       above(i, j0);
            while (bonds) {
                const int j = j0 + __ffsll((long long)bonds) - 1;
                bonds &= bonds - 1ull;
                const word wj = img[j];
                int n[DIM];
                fold_numbers<DIM>(P, sx, Np, xi, j, n);
#pragma unroll
                for (int k = 0; k < DIM; ++k)
                    if (I::field(wi, k) - I::field(wj, k) != n[k]) mk |= 1u << k;
            }
        }
        if (mk) atomicOr(&wmask[li], mk);
    }
    __syncthreads();                                                   // the masks are complete

    // ---- counts per mask, the slice's OR and the finite sizes
    for (int r = tid; r < Np; r += kClThreads) {
        if (label[r] != r) continue;
        const unsigned int s = cnt[r], mk = wmask[r];
        atomicAdd(&c8[mk], 1u);
        atomicAdd(&m8[mk], s);
        if (mk) atomicOr(sor, mk);
        else atomicAdd(&hfin[s - 1u], 1u);
    }

    // ---- t_i of the finite clusters: the pairs above i, j ascending, unfolded by the image numbers
    for (int i = tid; i < Np; i += kClThreads) {
        const int li = label[i];
        double t = 0.0;
        if (cnt[li] > 1u && wmask[li] == 0u) {
            double xi[DIM];
#pragma unroll
            for (int k = 0; k < DIM; ++k) xi[k] = sx[k * Np + i];
            const word wi = img[i];
            for (int j = i + 1; j < Np; ++j) {
                if (label[j] != li) continue;
                const word wj = img[j];
                double r2 = 0.0;
#pragma unroll
                for (int k = 0; k < DIM; ++k) {
                    const double c = (double)(I::field(wi, k) - I::field(wj, k));
                    const double du = (xi[k] - sx[k * Np + j]) - c * P.Lbox[k];
                    r2 = r2 + du * du;
                }
                t = t + r2;
            }
        }
        tt[i] = t;
    }
    int *lab = labels + ((size_t)slot * ns + js) * Np;
    for (int i = tid; i < Np; i += kClThreads) lab[i] = label[i];
    __syncthreads();                                                   // tt, c8, m8, sor and hfin are complete

    // ---- g of every finite cluster, by the owner of its root, members ascending
    for (int r = tid; r < Np; r += kClThreads) {
        if (label[r] != r || wmask[r] != 0u) continue;
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
    flush_counts(hfin, Np, [&](int t) { return &nfin[(size_t)w * Np + t]; });
    if (tid < 8) {
        if (c8[tid]) atomicAdd(&nwrap[(size_t)w * 8 + tid], (unsigned long long)c8[tid]);
        if (m8[tid]) atomicAdd(&mwrap[(size_t)w * 8 + tid], (unsigned long long)m8[tid]);
    }
    if (tid == 0) {
        atomicAdd(&swrap[(size_t)w * 8 + sor[0]], 1ull);
        atomicAdd(&samples[w], 1ull);
    }
    __syncthreads();                                                   // gg is complete

    // ---- G_slice per size, finite roots ascending
    double *o = scratch + ((size_t)slot * ns + js) * Np;
    for (int t = tid; t < Np; t += kClThreads) {
        double G = 0.0;
        if (hfin[t]) {
            const unsigned int s = (unsigned int)t + 1u;
            for (int r = 0; r < Np; ++r)
                if (label[r] == r && cnt[r] == s && wmask[r] == 0u) G = G + gg[r];
        }
        o[t] = G;
    }
}

// first, second, both, norig: [walker][ntau + 1]
__global__ __launch_bounds__(kClThreads) void k_pc_persist(
    WalkerList list, int Np, int ns, int ntau, const int *__restrict__ labels, unsigned long long *__restrict__ first,
    unsigned long long *__restrict__ second, unsigned long long *__restrict__ both, unsigned long long *__restrict__ norig)
{
    extern __shared__ int pl[];
    __shared__ unsigned int acc[3];
    int *la = pl, *lb = pl + Np;
    const int slot = blockIdx.x / ns, a = blockIdx.x - slot * ns;
    const int w = list.w[slot];
    const int tid = (int)threadIdx.x;
    const int *base = labels + (size_t)slot * ns * Np;
    for (int i = tid; i < Np; i += kClThreads) la[i] = base[(size_t)a * Np + i];
    const int lmax = min(ntau, ns - 1 - a);
    for (int l = 0; l <= lmax; ++l) {
        __syncthreads();                                               // the last lag's readers of lb and acc are through
        for (int i = tid; i < Np; i += kClThreads) lb[i] = base[(size_t)(a + l) * Np + i];
        if (tid < 3) acc[tid] = 0u;
        __syncthreads();
        unsigned int c[3] = {0u, 0u, 0u};
        for (int i = tid; i < Np; i += kClThreads) {
            const int ai = la[i], bi = lb[i];
            unsigned int f = 0u, s = 0u, b = 0u;
            for (int j = 0; j < Np; ++j) {
                const unsigned int ta = la[j] == ai, tb = lb[j] == bi;
                f += ta;
                s += tb;
                b += ta & tb;
            }
            c[0] += f - 1u;                                            // (j == i is together with itself in all three)
            c[1] += s - 1u;
            c[2] += b - 1u;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) c[q] += __shfl_xor(c[q], off, kWave);
            if ((tid & (kWave - 1)) == 0 && c[q]) atomicAdd(&acc[q], c[q]);
        }
        __syncthreads();
        const size_t e = (size_t)w * (ntau + 1) + l;
        if (tid < 3) {
            unsigned long long *dst = tid == 0 ? first : tid == 1 ? second : both;
            if (acc[tid]) atomicAdd(&dst[e], (unsigned long long)(acc[tid] >> 1));   // ordered pairs -> i < j
        } else if (tid == 3) {
            atomicAdd(&norig[e], 1ull);
        }
    }
}

} // namespace

size_t pc_lds_bytes(int dim, int Np)
{
    const size_t np = (size_t)Np, nw = (np + 63) / 64;
    return sizeof(double) * ((size_t)dim * np + 2 * np) + (Np <= kClAdjNpMax ? 8 * np * nw : 0) + (dim == 3 ? 8 : 4) * np +
           4 * (4 * np + 17);
}

size_t pc_slot_bytes(int Np, int window)
{
    return (2 * (size_t)window + 1) * (size_t)Np * (sizeof(double) + sizeof(int));
}

hipError_t launch_pc(const DevParams &P, const double *paths, int n, const WalkerList &list, int window, int ntau, double rc2,
                     double *scratch, int *labels, const PcSums &s, unsigned int *sweeps, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    const int ns = 2 * window + 1;
    if (n > kWalkerListMax || P.Np < 1 || P.Np > kClNpMax || ntau < 0 || ntau > 2 * window || (long long)n * ns > 0x7fffffffll)
        return hipErrorInvalidValue;
    const size_t lds = pc_lds_bytes(P.dim, P.Np);
    if (lds > kClLdsBudget) return hipErrorInvalidValue;
    hipError_t e = with_dim(P.dim, [&](auto D) {
        return with_flag(P.Np <= kClAdjNpMax, [&](auto A) {
            return launch<k_pc<D(), A()>>(dim3((unsigned)(n * ns)), dim3(kClThreads), lds, st, P, paths, list, window, rc2, scratch,
                                          labels, s.nwrap, s.mwrap, s.swrap, s.nfin, s.samples, sweeps);
        });
    });
    if (e != hipSuccess) return e;
    e = launch_cl_combine(list, n, ns, P.Np, scratch, s.rg2u, st);
    if (e != hipSuccess) return e;
    return launch<k_pc_persist>(dim3((unsigned)(n * ns)), dim3(kClThreads), 2 * sizeof(int) * (size_t)P.Np, st, list, (int)P.Np, ns,
                                ntau, (const int *)labels, s.first, s.second, s.both, s.norig);
}

} // namespace pigs
