// pigs_tau.hip -- imaginary-time profiles of the potential energy, the virial and the link lengths (pigs_tau_*).
//
// PIGS keeps the whole path: the potential energy of slice b falls from the trial function's value at the two ends
// (b = 0, 2Nb) to a plateau around the middle, and the plateau is the part of the path on which the windowed estimators
// (pigs_fqt_*, pigs_sqv_*, pigs_fqv_*, pigs_grv_*) may be taken.  Per listed walker w and slice b = 0..2Nb one call adds
//   Q[w][b][0]  Vpair = sum_{i<j} v(r_ij)               v  = Interpolate opt 0 on VTable  (sample_mod.f90:13-150)
//   Q[w][b][1]  Vext  = sum_i sum_k TrapPot(0,a_ho(k),x_k(i))   (trap; exactly 0 in a periodic system, system_mod.f90:238-252)
//   Q[w][b][2]  W     = sum_{i<j} r_ij v'(r_ij)         v' = Interpolate opt 1 on VTable  (the force terms' derivative, :113-114)
//   Q[w][b][3]  D2    = sum_i |x_i(b) - x_i(b+1)|^2     (exactly 0 for b = 2Nb; periodic: folded once, counted inside the
//                                                        cutoff only, quirk Q8, sample_mod.f90:377)
// Pairs as PotentialEnergy takes them: periodic -- one fold, counted iff r^2 <= rcut2, the exact-term forms of
// pigs_device.h (min_image_mag, sqrt_exact, flerp_setup, finterp01: every term v and r v' has the reference's bits);
// trap -- plain distance, no cutoff, the plain forms (lerp_setup, interp0, interp1) with K2's index clamps.
// The short per-pair arithmetic (fcell_setup, ~1 ulp per interpolation) is NOT used here: v' is the difference of two
// interpolations of |F| ~ 10 divided by 2 dr, so near the potential minimum, where v' passes through zero, an ulp of
// each interpolation is ~1e-11 absolute in r v' while the term itself -- and any bound on the sum that scales with
// its terms -- vanishes.  A slice of few pairs shows it (Np = 2: one term).  Exact terms leave the summation order as
// the only difference from the reference.
//
// Each pair once: thread i owns particle i and takes the next floor(Np/2) partners around the ring (K2's walk on
// V-only slices), carrying v and r v' together.  One kernel form, k_tau: one workgroup per (listed walker, slice), the
// slice staged in LDS, the table gathered from global memory.  (A persistent form with the table image in LDS, K2's
// k_slice_energy_lds shape, was built and measured 3 % slower at config 3's shape: DESIGN.md section 4; it is gone.)
// Summation order, fixed: a lane adds its particles' sums in ascending particle order (Np beyond the workgroup makes
// several trips), the wave's butterfly (wave_sum), the waves in wave order, and `acc += value` last, by the one thread
// that owns the element (w, b) for the launch -- the host never lists a walker twice in ONE launch.  No floating-point
// atomics.
// Compile with -ffp-contract=off.
#include <algorithm>

#include "pigs_device.h"
#include "pigs_kernels.h"
#include "pigs_launch.h"

namespace pigs {

namespace {

// the four per-particle sums of particle i of the slice staged in sx (SoA, stride NpPad); S1: the same particle's
// row of slice b+1 in global memory (nullptr for b = 2Nb)
template <int DIM, bool TRAP>
__device__ __forceinline__ void tau_particle(const DevParams &P, const double *sx, const double *__restrict__ tab,
                                             const double *S1, int i,
                                             double &vp, double &ve, double &ww, double &d2)
{
    const int Np = P.Np, NpPad = P.NpPad;
    double xi[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
        xi[k] = sx[k * NpPad + i];
        if (TRAP) ve = ve + trap_pot(0, P.a_ho[k], xi[k]);                       // sample_mod.f90:33-42
    }
    // the next h partners around the ring (for even Np the opposite partner belongs to the lower half only)
    const int h = (Np & 1) ? (Np - 1) / 2 : (i < Np / 2 ? Np / 2 : Np / 2 - 1);
    double poti = 0.0, viri = 0.0;
    int j = i;
    for (int q = 0; q < h; ++q) {
        j = j + 1 == Np ? 0 : j + 1;
        double d[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) d[k] = xi[k] - sx[k * NpPad + j];
        if (TRAP) {
            const double r = sqrt(plain_r2<DIM>(d));                              // no cutoff in the trap (:64)
            Lerp L = lerp_setup(r, P.dr, P.Nmax);
            L.ix  = max(L.ix, 1);                                                 // (identity for every finite r: keeps the loads in the table)
            L.im2 = max(L.ix - 2, 0);
            poti = poti + interp0(tab, L, P.dr);
            viri = viri + r * interp1(tab, L, P.dr);
        } else {
            const double r2 = min_image_mag<DIM>(d, P);                           // the single fold, |.| only
            if (r2 <= P.rcut2) {                                                  // :98
                const double r = sqrt_exact(r2);
                FLerp L = flerp_setup(r, P);
                L.ix  = max(L.ix, 1);                                             // (identity for every finite r: keeps the loads in the table)
                L.im2 = max(L.ix - 2, 0);
                double v0, v1;
                finterp01(tab, L, P, v0, v1);
                poti = poti + v0;
                viri = viri + r * v1;
            }
        }
    }
    vp = vp + poti;
    ww = ww + viri;
    if (S1) {                                                                     // sample_mod.f90:359-380 (Q8)
        double d[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) d[k] = xi[k] - S1[(size_t)k * NpPad + i];
        const double r2 = TRAP ? plain_r2<DIM>(d) : min_image<DIM>(d, P);
        if (TRAP || r2 <= P.rcut2) d2 = d2 + r2;
    }
}

// acc: [walker][2Nb+1][4]
template <int DIM, bool TRAP>
__global__ __launch_bounds__(256) void k_tau(
    DevParams P, const double *__restrict__ paths, const double *__restrict__ VT, WalkerList list, double *__restrict__ acc,
    unsigned long long *__restrict__ samples)
{
    extern __shared__ double lds[];
    double *sx  = lds;                       // DIM * NpPad doubles
    double *red = lds + DIM * P.NpPad;       // 4 * (blockDim/64) doubles

    const int slot = blockIdx.x / P.M, b = blockIdx.x - slot * P.M;
    const int w = list.w[slot];
    const size_t sl = slice_doubles(DIM, P.NpPad);
    const double *S = paths + ((size_t)w * P.M + b) * sl;
    const double *S1 = b + 1 < P.M ? S + sl : nullptr;

    for (int t = threadIdx.x; t < DIM * P.NpPad; t += blockDim.x) sx[t] = S[t];
    __syncthreads();

    double vp = 0.0, ve = 0.0, ww = 0.0, d2 = 0.0;
    for (int i = threadIdx.x; i < P.Np; i += blockDim.x) tau_particle<DIM, TRAP>(P, sx, VT, S1, i, vp, ve, ww, d2);

    vp = wave_sum(vp); ve = wave_sum(ve); ww = wave_sum(ww); d2 = wave_sum(d2);
    const int nw = blockDim.x >> 6, wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[4 * wid] = vp; red[4 * wid + 1] = ve; red[4 * wid + 2] = ww; red[4 * wid + 3] = d2; }
    __syncthreads();
    if (threadIdx.x < 4) {
        double a = 0.0;
        for (int q = 0; q < nw; ++q) a += red[4 * q + threadIdx.x];
        double *dst = acc + ((size_t)w * P.M + b) * 4 + threadIdx.x;
        *dst = *dst + a;
    }
    if (b == 0 && threadIdx.x == 0) samples[w] = samples[w] + 1ull;
}

} // namespace

hipError_t launch_tau(const DevParams &P, const double *paths, const double *VT, int n, const WalkerList &list, double *acc,
                      unsigned long long *samples, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    if (n > kWalkerListMax) return hipErrorInvalidValue;
    const int n_slots = n * P.M;
    const int bs = std::min(256, ((P.Np + 63) / 64) * 64);
    const size_t lds = ((size_t)P.dim * P.NpPad + 4 * (bs / 64)) * sizeof(double);
    if (lds > kLdsNoGrant) return hipErrorInvalidValue;
    return with_flag(P.trap, [&](auto T) {
        return with_dim(P.dim, [&](auto D) {
            return launch<k_tau<D(), T()>>(dim3(n_slots), dim3(bs), lds, st, P, paths, VT, list, acc, samples);
        });
    });
}

} // namespace pigs
