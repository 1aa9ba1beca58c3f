// pigs_bop.hip -- bond-orientational order of a periodic system over a slice window (pigs_bop_*): the Steinhardt
// invariants Q4, Q6 with their local distributions (3D), psi4, psi6 (2D), and the bond-orientational correlation G6(r).
// include/pigs_hip.h has the definition word for word.
//
// k_bop: one workgroup per (listed walker, window slice), the whole slice staged in LDS (unit-stride rows).
//   * Neighbour pass.  Thread t owns the particles t, t + blockDim, ..; for each it walks ALL partners j in ascending
//     order through broadcast LDS reads: d = x(i) - x(j) folded by min_image<DIM>, r2 summed left to right, a bond iff
//     0 < r2 < rnb2 in double (so the particle itself, a coincident partner and a non-finite r2 are no bonds).  Bonds are
//     a few per cent of the pairs, and with 64 lanes a branch per pair would run the harmonics for almost every j with
//     two or three lanes alive; instead the lane marks the bonds of 64 partners in a bit mask (distance work only), then
//     works the set bits off, so the wave pays the harmonics max-over-lanes(bonds per 64 partners) times.
//   * Harmonics from the Cartesian unit vector, one 1/r per bond, no sincos/acos: powers of (x + i y) by recurrence times
//     the m-th derivative of P_l in z, pre-scaled by s_lm = sqrt(w_m (l-m)!/(l+m)!) (w_0 = 1, w_m = 2: the -m partner),
//     m = 0..l.  With a_lm(i) the bond mean of these, 4 pi/(2l+1) sum_{m=-l..l} |q_lm|^2 = sum_{m>=0} |a_lm|^2, and
//     (4 pi/13) Re sum_m q_6m(i) q_6m(j)* is the plain dot product of the 13 stored doubles.  2D: powers of (x + i y)/r.
//   * Per particle: the invariants go to the int64 histograms by global integer atomics (bin decided in double before
//     the conversion), the l = 6 components to an LDS table (Nr > 0), the particle sums to per-thread registers in
//     ascending particle order; these are reduced by the fixed wave butterfly, then over the waves in wave order.
//   * Correlation pass (Nr > 0): k_grv's cyclic i < j enumeration over the staged slice and the table, K7's radial rule,
//     c_ij 2^40 rounded to nearest into an int64 LDS histogram (order-free), the pair counts beside it.
//   * The slice's 8 scalars and Nr bins (converted to double once) go to the (slot, slice) scratch; the pair counts to
//     the walker's int64 accumulator by global atomics.
// k_bop_combine: one thread per (listed walker, scalar or bin): the slices in ascending order, added to the accumulator
//   element that this thread alone owns in this launch.
// No floating-point atomics: the same worldline gives the same bits whatever the list, the split or the context.
// Compile with -ffp-contract=off.
#include "pigs_kernels.h"
#include "pigs_launch.h"
#include "pigs_slice_device.h"

namespace pigs {

namespace {

struct BopArgs {
    int window, Nh, Nr;
    double rnb2, rbin;
};

// The per-bond terms and the layout of a particle's components a[NA]: the first N4 doubles belong to l (n) = 4, the
// other NT to l (n) = 6 -- the ones the table keeps.
template <int DIM> struct Bop;

template <> struct Bop<3> {
    static constexpr int N4 = 9, NT = 13, NA = N4 + NT;     // m = 0 is real; (re, im) of m = 1..l
    __device__ static __forceinline__ void add(double (&a)[NA], const double (&d)[3], double r2)
    {
        // s_lm, from the factorials (17 digits)
        constexpr double s41 = 0.31622776601683794, s42 = 0.07453559924999299, s43 = 0.019920476822239894,
                         s44 = 0.0070429521227376385;
        constexpr double s61 = 0.21821789023599236, s62 = 0.03450327796711771, s63 = 0.005750546327852952,
                         s64 = 0.00104990131391452, s65 = 0.00022383971222927231, s66 = 6.461695905544936e-05;
        const double rinv = 1.0 / sqrt(r2);
        const double x = d[0] * rinv, y = d[1] * rinv, z = d[2] * rinv, z2 = z * z;
        // d^m P_l / dz^m, scaled
        const double t40 = ((35.0 * z2 - 30.0) * z2 + 3.0) * 0.125;
        const double t41 = z * (35.0 * z2 - 15.0) * (0.5 * s41);
        const double t42 = (105.0 * z2 - 15.0) * (0.5 * s42);
        const double t43 = z * (105.0 * s43);
        const double t44 = 105.0 * s44;
        const double t60 = (((231.0 * z2 - 315.0) * z2 + 105.0) * z2 - 5.0) * 0.0625;
        const double t61 = z * ((693.0 * z2 - 630.0) * z2 + 105.0) * (0.125 * s61);
        const double t62 = ((3465.0 * z2 - 1890.0) * z2 + 105.0) * (0.125 * s62);
        const double t63 = z * (3465.0 * z2 - 945.0) * (0.5 * s63);
        const double t64 = (10395.0 * z2 - 945.0) * (0.5 * s64);
        const double t65 = z * (10395.0 * s65);
        const double t66 = 10395.0 * s66;
        // (x + i y)^m
        const double c2 = x * x - y * y, e2 = 2.0 * (x * y);
        const double c3 = c2 * x - e2 * y, e3 = c2 * y + e2 * x;
        const double c4 = c2 * c2 - e2 * e2, e4 = 2.0 * (c2 * e2);
        const double c5 = c4 * x - e4 * y, e5 = c4 * y + e4 * x;
        const double c6 = c4 * c2 - e4 * e2, e6 = c4 * e2 + e4 * c2;
        a[0] = a[0] + t40;
        a[1] = a[1] + t41 * x;   a[2] = a[2] + t41 * y;
        a[3] = a[3] + t42 * c2;  a[4] = a[4] + t42 * e2;
        a[5] = a[5] + t43 * c3;  a[6] = a[6] + t43 * e3;
        a[7] = a[7] + t44 * c4;  a[8] = a[8] + t44 * e4;
        a[9] = a[9] + t60;
        a[10] = a[10] + t61 * x;  a[11] = a[11] + t61 * y;
        a[12] = a[12] + t62 * c2; a[13] = a[13] + t62 * e2;
        a[14] = a[14] + t63 * c3; a[15] = a[15] + t63 * e3;
        a[16] = a[16] + t64 * c4; a[17] = a[17] + t64 * e4;
        a[18] = a[18] + t65 * c5; a[19] = a[19] + t65 * e5;
        a[20] = a[20] + t66 * c6; a[21] = a[21] + t66 * e6;
    }
};

template <> struct Bop<2> {
    static constexpr int N4 = 2, NT = 2, NA = N4 + NT;      // psi4, psi6
    __device__ static __forceinline__ void add(double (&a)[NA], const double (&d)[2], double r2)
    {
        const double rinv = 1.0 / sqrt(r2);
        const double x = d[0] * rinv, y = d[1] * rinv;
        const double c2 = x * x - y * y, e2 = 2.0 * (x * y);
        const double c4 = c2 * c2 - e2 * e2, e4 = 2.0 * (c2 * e2);
        const double c6 = c4 * c2 - e4 * e2, e6 = c4 * e2 + e4 * c2;
        a[0] = a[0] + c4; a[1] = a[1] + e4;
        a[2] = a[2] + c6; a[3] = a[3] + e6;
    }
};

// sqrt of the sum of squares of v[lo..hi), left to right
template <int N>
__device__ __forceinline__ double norm_of(const double (&v)[N], int lo, int hi, double &sq)
{
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < N; ++k)
        if (k >= lo && k < hi) s = s + v[k] * v[k];
    sq = s;
    return sqrt(s);
}

// bin of an invariant q >= 0 over [0, 1]: min(int(q Nh), Nh - 1), decided in double before the conversion
__device__ __forceinline__ int bop_bin(double q, int Nh)
{
    const double t = q * (double)Nh;
    return t < (double)Nh ? (int)t : Nh - 1;
}

template <int DIM>
__global__ __launch_bounds__(kBopThreads) void k_bop(
    DevParams P, const double *__restrict__ paths, WalkerList list, BopArgs A, double *__restrict__ scratch,
    unsigned long long *__restrict__ hist, unsigned long long *__restrict__ gn)
{
    using B = Bop<DIM>;
    constexpr int NA = B::NA, N4 = B::N4, NT = B::NT, NV = NA + 3;     // + sum q4(i), sum q6(i), sum n_i
    extern __shared__ double lds[];
    const int Np = P.Np, Nr = A.Nr;
    double *sx = lds;                                                  // DIM x Np: the slice
    double *tab = sx + (size_t)DIM * Np;                               // NT x Np: the l = 6 components (Nr > 0)
    unsigned long long *gsum = reinterpret_cast<unsigned long long *>(tab + (Nr > 0 ? (size_t)NT * Np : 0));   // Nr
    unsigned long long *gcnt = gsum + Nr;                              // Nr
    double *red = reinterpret_cast<double *>(gcnt + Nr);               // waves x NV

    const int ns = 2 * A.window + 1;
    const int slot = blockIdx.x / ns, js = blockIdx.x - slot * ns;
    const int w = list.w[slot];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const double *S = window_slice<DIM>(P, paths, w, P.Nb - A.window + js);

    for (int t = threadIdx.x; t < DIM * Np; t += blockDim.x) {
        const int k = t / Np, ii = t - k * Np;
        sx[t] = S[(size_t)k * P.NpPad + ii];
    }
    for (int t = threadIdx.x; t < 2 * Nr; t += blockDim.x) gsum[t] = 0ull;    // (gsum and gcnt are adjacent)
    __syncthreads();

    // ---- neighbour pass
    double v[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] = 0.0;
    for (int i = threadIdx.x; i < Np; i += blockDim.x) {
        double xi[DIM], a[NA];
#pragma unroll
        for (int k = 0; k < DIM; ++k) xi[k] = sx[k * Np + i];
#pragma unroll
        for (int k = 0; k < NA; ++k) a[k] = 0.0;
        int n = 0;
        for (int j0 = 0; j0 < Np; j0 += 64) {
            const int mj = min(64, Np - j0);
            unsigned long long bonds = 0ull;
            for (int jj = 0; jj < mj; ++jj) {
                double d[DIM];
#pragma unroll
                for (int k = 0; k < DIM; ++k) d[k] = xi[k] - sx[k * Np + j0 + jj];
                const double r2 = min_image<DIM>(d, P);
                if (r2 > 0.0 && r2 < A.rnb2) bonds |= 1ull << jj;      // (j == i: r2 is 0 or NaN)
            }
            while (bonds) {
                const int jj = __ffsll((long long)bonds) - 1;
                bonds &= bonds - 1ull;
                double d[DIM];
#pragma unroll
                for (int k = 0; k < DIM; ++k) d[k] = xi[k] - sx[k * Np + j0 + jj];
                const double r2 = min_image<DIM>(d, P);
                B::add(a, d, r2);
                ++n;
            }
        }
        const double inv = n > 0 ? 1.0 / (double)n : 0.0;
#pragma unroll
        for (int k = 0; k < NA; ++k) a[k] = a[k] * inv;
        double sq;
        const double q4 = norm_of(a, 0, N4, sq), q6 = norm_of(a, N4, NA, sq);
        atomicAdd(&hist[((size_t)w * 2 + 0) * A.Nh + bop_bin(q4, A.Nh)], 1ull);
        atomicAdd(&hist[((size_t)w * 2 + 1) * A.Nh + bop_bin(q6, A.Nh)], 1ull);
        if (Nr > 0) {
#pragma unroll
            for (int k = 0; k < NT; ++k) tab[k * Np + i] = a[N4 + k];
        }
#pragma unroll
        for (int k = 0; k < NA; ++k) v[k] = v[k] + a[k];
        v[NA] = v[NA] + q4;
        v[NA + 1] = v[NA + 1] + q6;
        v[NA + 2] = v[NA + 2] + (double)n;                             // an exact integer
    }
    // the wave (fixed butterfly), then the waves in wave order
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const double s = wave_sum(v[k]);
        if (lane == 0) red[wave * NV + k] = s;
    }
    __syncthreads();                                                   // red and tab are complete
    if (threadIdx.x == 0) {
        const int nw = (int)blockDim.x / kWave;
        double tot[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            double s = red[k];
            for (int g = 1; g < nw; ++g) s = s + red[g * NV + k];
            tot[k] = s;
        }
        const double np = (double)Np;
        double Q[NA];
#pragma unroll
        for (int k = 0; k < NA; ++k) Q[k] = tot[k] / np;
        double sq4, sq6;
        const double Q4 = norm_of(Q, 0, N4, sq4), Q6 = norm_of(Q, N4, NA, sq6);
        double *o = scratch + ((size_t)slot * ns + js) * (8 + Nr);
        o[0] = Q4; o[1] = sq4; o[2] = Q6; o[3] = sq6;
        o[4] = tot[NA] / np; o[5] = tot[NA + 1] / np; o[6] = tot[NA + 2]; o[7] = 0.0;
    }
    if (Nr == 0) return;

    // ---- correlation pass: the cyclic enumeration of k_grv over the whole slice, element e = row * Np + c
    const double nr = (double)Nr;
    const int npairs = Np * (Np - 1) / 2;
    const int step_r = (int)blockDim.x / Np, step_c = (int)blockDim.x - step_r * Np;
    int row = (int)threadIdx.x / Np, c = (int)threadIdx.x - row * Np;
    for (int e = threadIdx.x; e < npairs; e += blockDim.x) {
        int p = c + row + 1;
        if (p >= Np) p -= Np;
        const int lo = min(c, p), hi = max(c, p);
        double d[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) d[k] = sx[k * Np + lo] - sx[k * Np + hi];
        const double r2 = min_image<DIM>(d, P);
        if (r2 <= P.rcut2) {
            const double u = sqrt(r2) / A.rbin;
            if (u < nr) {
                double cij = 0.0;
#pragma unroll
                for (int k = 0; k < NT; ++k) cij = cij + tab[k * Np + lo] * tab[k * Np + hi];
                // |cij| <= 1 up to rounding (bond means of unit-modulus terms): the conversion cannot overflow
                const long long fx = __double2ll_rn(cij * kBopFixScale);
                atomicAdd(&gsum[(int)u], (unsigned long long)fx);
                atomicAdd(&gcnt[(int)u], 1ull);
            }
        }
        row += step_r;
        c += step_c;
        if (c >= Np) { c -= Np; ++row; }
    }
    __syncthreads();
    double *o = scratch + ((size_t)slot * ns + js) * (8 + Nr) + 8;
    for (int t = threadIdx.x; t < Nr; t += blockDim.x) {
        o[t] = (double)(long long)gsum[t] * (1.0 / kBopFixScale);
        const unsigned long long cnt = gcnt[t];
        if (cnt) atomicAdd(&gn[(size_t)w * Nr + t], cnt);
    }
}

__global__ __launch_bounds__(256) void k_bop_combine(
    WalkerList list, int n, int ns, int Nr, const double *__restrict__ scratch, double *__restrict__ S, double *__restrict__ G,
    unsigned long long *__restrict__ samples)
{
    const int per = 8 + Nr;
    const size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (size_t)per * n) return;
    const int slot = (int)(id / (size_t)per);
    const int e = (int)(id - (size_t)slot * per);
    const int w = list.w[slot];
    const double *r = scratch + (size_t)slot * ns * per + e;
    double s = 0.0;
    for (int a = 0; a < ns; ++a) s = s + r[(size_t)a * per];
    double *dst = e < 8 ? S + (size_t)w * 8 + e : G + (size_t)w * Nr + (e - 8);
    *dst = *dst + s;
    if (e == 0) samples[w] = samples[w] + 1ull;
}

} // namespace

size_t bop_lds_bytes(int dim, int Np, int Nr)
{
    const size_t nt = dim == 3 ? 13 : 2, nv = (dim == 3 ? 22 : 4) + 3;
    return sizeof(double) * ((size_t)dim * Np + (Nr > 0 ? nt * Np : 0) + 2 * (size_t)Nr + (size_t)(kBopThreads / kWave) * nv);
}

hipError_t launch_bop(const DevParams &P, const double *paths, int n, const WalkerList &list, int window, int Nh, int Nr,
                      double rnb2, double rbin, double *scratch, double *S, unsigned long long *hist, double *G,
                      unsigned long long *gn, unsigned long long *samples, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    BopArgs A{};
    A.window = window; A.Nh = Nh; A.Nr = Nr; A.rnb2 = rnb2; A.rbin = rbin;
    const int ns = 2 * window + 1;
    const size_t lds = bop_lds_bytes(P.dim, P.Np, Nr);
    // (dim = 1 never comes here: pigs_bop_init refuses it, so with_dim's first case takes no instantiation of its own)
    const hipError_t e = with_dim(P.dim, [&](auto D) {
        return launch<k_bop<(D() == 2 ? 2 : 3)>>(dim3(n * ns), dim3(kBopThreads), lds, st, P, paths, list, A, scratch, hist, gn);
    });
    if (e != hipSuccess) return e;
    const size_t total = (size_t)n * (8 + Nr);
    return launch<k_bop_combine>(dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, list, n, ns, Nr, scratch, S, G, samples);
}

} // namespace pigs
