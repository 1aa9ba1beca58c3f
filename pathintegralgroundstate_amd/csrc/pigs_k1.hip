// pigs_k1.hip -- K1: batched Delta S of proposal beads on gfx950.
//
// Replaces the reference's `call UpdateAction` (vpi_mod.f90:2491-2530) with its callees
// UpdatePot (2660-2841), UpdateWf (2534-2656) and GreenFunction opt 0 (global_mod.f90:19-72),
// batched over (walker, particle, bead) proposal items.
//
// Work decomposition: ONE wave64 per item (an item's 255 partners are 4 lane-strided passes
// over one contiguous 6 KB SoA slice: 512-B coalesced loads per coordinate); no workgroup
// barrier anywhere in the item loop.  Kernels in this file (pigs_set_tuning("k1_variant"); measurements in
// DESIGN.md section 4 and profiles/; the A/B history of the forms that lost -- LDS table in the plain grid,
// in-cutoff compaction, prefetch-only, the first persistent kernel -- is archived in profiles/r01_k1_variants_ab*.txt):
//    1 v1    plain statement (IEEE `/`, sqrt(), tables gathered from global memory)
//    2 v2    exact-term: exact short division / fused sqrt+1/r (pigs_device.h), one LDS-transpose reduction for all
//            accumulators.  v1 and v2 sum bit-identical per-pair terms; only the summation order differs.
//    7 / 8   v2 with the short arithmetic on the global table (FastTab; 8: partner loads issued up front) -- the
//            form for Np > 256
//   12 pipe2 persistent, one 1024-thread workgroup per CU, table image with its zero cell in LDS, branch-free short
//            arithmetic, per-workgroup item queue, item records and partner coordinates requested ahead: the default
//            for large launches of a periodic system with Np <= 256
//   13 grid  the SAME per-item arithmetic as pipe2 (pipe_pair on the global table image, passes and sides in the same
//            order) on a plain grid: what small launches of such a system run, so that an item's Delta S does not
//            depend on how many other items share its launch
//   14 reference order (validation): exact-term arithmetic, per-partner terms parked in LDS and added by one lane
//            per accumulator in the reference's jp order -- every bit of Delta S equals the reference's

#include "pigs_device.h"
#include "pigs_k1_device.h"
#include "pigs_kernels.h"
#include "pigs_launch.h"

namespace pigs {

// =====================================================================================
// K1 v1 (plain form, kept as the readable reference of the kernel and for A/B timing):
// one wave64 per proposal item; lane l visits partners jp = l, l+64, ... of the
// item's slice (unit-stride 512-B loads per coordinate), accumulates its partial sums
// in registers, then one butterfly per accumulator.  Wave-uniform control flow per item
// (bead parity / end bead), so no divergence except the physical cutoff test.
// Algorithmic bytes per item: dim*Np*8 (slice) + 2*dim*8 (xnew,xold) + 8 (DeltaS)
// (+12 B of indices), i.e. 6 200 B at Np=256 for Np-1=255 bead-pair evaluations.
// =====================================================================================
template <int DIM, bool TRAP>
__global__ __launch_bounds__(256) void k_delta_action_v1(
    DevParams P, const double *__restrict__ paths, const double *__restrict__ VT,
    const double *__restrict__ WF, int n_items, const int32_t *__restrict__ walker,
    const int32_t *__restrict__ ipv, const int32_t *__restrict__ ibv,
    const double *__restrict__ xnew, const double *__restrict__ xold,
    double *__restrict__ out, double *__restrict__ parts)
{
    const int lane  = threadIdx.x & (kWave - 1);
    const int wid   = threadIdx.x >> 6;
    const int nwave = gridDim.x * (blockDim.x >> 6);
    const size_t sl = slice_doubles(DIM, P.NpPad);

    for (int item = blockIdx.x * (blockDim.x >> 6) + wid; item < n_items; item += nwave) {
        const int it = __builtin_amdgcn_readfirstlane(item);
        const int w  = walker[it];
        const int p  = ipv[it] - 1;          // 0-based moved particle
        const int b  = ibv[it];
        if ((unsigned)w >= (unsigned)P.nW || (unsigned)p >= (unsigned)P.Np || (unsigned)b >= (unsigned)P.M) {
            if (lane == 0) out[it] = __builtin_nan("");      // bad index: never touch memory with it
            continue;
        }
        double xn[DIM], xo[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            xn[k] = xnew[(size_t)it * DIM + k];
            xo[k] = xold[(size_t)it * DIM + k];
        }
        const double *S   = paths + ((size_t)w * P.M + b) * sl;
        const bool odd    = (b & 1) != 0;                    // UpdateAction: force term on odd beads
        const bool endb   = (b == 0) || (b == 2 * P.Nb);     // UpdateWf only on the two end beads

        double potN = 0.0, potO = 0.0, psiN = 0.0, psiO = 0.0;
        double fN[DIM], fO[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) { fN[k] = 0.0; fO[k] = 0.0; }

        if (TRAP && lane == 0) {                              // vpi_mod.f90:2688-2695, 2555-2560
#pragma unroll
            for (int k = 0; k < DIM; ++k) {
                potN = potN + trap_pot(0, P.a_ho[k], xn[k]);
                potO = potO + trap_pot(0, P.a_ho[k], xo[k]);
                fO[k] = trap_pot(1, P.a_ho[k], xo[k]);
                fN[k] = trap_pot(1, P.a_ho[k], xn[k]);
                if (endb) {
                    psiO = psiO + trap_psi(0, P.a_ho[k], xo[k]);
                    psiN = psiN + trap_psi(0, P.a_ho[k], xn[k]);
                }
            }
        }

        for (int j0 = 0; j0 < P.Np; j0 += kWave) {
            const int j = j0 + lane;
            if (j < P.Np && j != p) {                        // vpi_mod.f90:2699: never read row ip
                double dnew[DIM], dold[DIM];
#pragma unroll
                for (int k = 0; k < DIM; ++k) {
                    const double rj = S[(size_t)k * P.NpPad + j];
                    dnew[k] = xn[k] - rj;                      // :2706
                    dold[k] = xo[k] - rj;                      // :2707
                }
                double r2n, r2o;
                if (TRAP) { r2o = plain_r2<DIM>(dold); r2n = plain_r2<DIM>(dnew); }
                else      { r2o = min_image<DIM>(dold, P); r2n = min_image<DIM>(dnew, P); }

                if (TRAP || r2n <= P.rcut2) {                // :2723 (Q5) / :2771
                    const double r = sqrt(r2n);
                    const Lerp L = lerp_setup(r, P.dr, P.Nmax);
                    potN = potN + interp0(VT, L, P.dr);
                    if (odd) {
                        const double dv = interp1(VT, L, P.dr);
#pragma unroll
                        for (int k = 0; k < DIM; ++k) fN[k] = fN[k] + dv * dnew[k] / r;   // :2784
                    }
                    if (endb) psiN = psiN + (P.wf_table ? interp0(WF, L, P.dr) : log_psi(0, P.Rm, r));   // :2637-2641
                }
                if (r2o <= P.rcut2) {                        // :2745 / :2795
                    const double r = sqrt(r2o);
                    const Lerp L = lerp_setup(r, P.dr, P.Nmax);
                    potO = potO + interp0(VT, L, P.dr);
                    if (odd) {
                        const double dv = interp1(VT, L, P.dr);
#pragma unroll
                        for (int k = 0; k < DIM; ++k) fO[k] = fO[k] + dv * dold[k] / r;   // :2808
                    }
                    if (endb) psiO = psiO + (P.wf_table ? interp0(WF, L, P.dr) : log_psi(0, P.Rm, r));   // :2623-2627
                } else if (TRAP && endb) {
                    // UpdateWf's trap branch has no cutoff on either distance (vpi_mod.f90:2595-2615)
                    const double r = sqrt(r2o);
                    const Lerp L = lerp_setup(r, P.dr, P.Nmax);
                    psiO = psiO + (P.wf_table ? interp0(WF, L, P.dr) : log_psi(0, P.Rm, r));
                }
            }
        }

        potN = wave_sum(potN);
        potO = wave_sum(potO);
        double dF2 = 0.0, dPsi = 0.0;
        if (odd) {
            double fn2 = 0.0, fo2 = 0.0;
#pragma unroll
            for (int k = 0; k < DIM; ++k) {
                const double a = wave_sum(fN[k]);
                const double c = wave_sum(fO[k]);
                fn2 = fn2 + a * a;                            // :2831
                fo2 = fo2 + c * c;                            // :2832
            }
            dF2 = fn2 - fo2;                                  // :2835
        }
        if (endb) {
            psiN = wave_sum(psiN);
            psiO = wave_sum(psiO);
            dPsi = psiN - psiO;                               // :2653
        }
        if (lane == 0) {
            const double dPot = potN - potO;                  // :2838
            out[it] = -dPsi + green_function(0, b, P.Nb, P.dt, dPot, dF2);   // :2527
            if (parts) {
                parts[(size_t)it * 3 + 0] = dPot;
                parts[(size_t)it * 3 + 1] = dF2;
                parts[(size_t)it * 3 + 2] = dPsi;
            }
        }
    }
}


// =====================================================================================
// K1 v2 (exact-term; FAST: short arithmetic on the global table)
// =====================================================================================
// LDS (dynamic): per wave kWaveLds bytes of reduction scratch (8 x 65 doubles)
template <int DIM, bool TRAP, int BLOCK, bool PREFETCH = false, bool FAST = false>
__global__ __launch_bounds__(BLOCK) void k_delta_action_v2(
    DevParams P, const double *__restrict__ paths, const double *__restrict__ VT,
    const double *__restrict__ WF, int n_items, const int32_t *__restrict__ walker,
    const int32_t *__restrict__ ipv, const int32_t *__restrict__ ibv,
    const double *__restrict__ xnew, const double *__restrict__ xold,
    double *__restrict__ out, double *__restrict__ parts)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane  = threadIdx.x & (kWave - 1);
    const int wid   = threadIdx.x >> 6;
    const int nwave = gridDim.x * (BLOCK >> 6);
    const size_t sl = slice_doubles(DIM, P.NpPad);
    double *red = reinterpret_cast<double *>(smem + (size_t)wid * kWaveLds);

    for (int item = blockIdx.x * (BLOCK >> 6) + wid; item < n_items; item += nwave) {
        const int it = __builtin_amdgcn_readfirstlane(item);
        const int w  = walker[it];
        const int p  = ipv[it] - 1;
        const int b  = ibv[it];
        if ((unsigned)w >= (unsigned)P.nW || (unsigned)p >= (unsigned)P.Np || (unsigned)b >= (unsigned)P.M) {
            if (lane == 0) out[it] = __builtin_nan("");
            continue;
        }
        double xn[DIM], xo[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            xn[k] = xnew[(size_t)it * DIM + k];
            xo[k] = xold[(size_t)it * DIM + k];
        }
        const double *S = paths + ((size_t)w * P.M + b) * sl;
        double *o = out + it;
        double *q = parts ? parts + (size_t)it * 3 : nullptr;
        if (FAST && !TRAP) {                                    // short arithmetic (pigs_device.h, FastTab)
            if (PREFETCH) item_eval_prefetch<DIM, TRAP>(P, FastTab{VT}, WF, S, p, b, xn, xo, lane, red, o, q);
            else          item_eval<DIM, TRAP>(P, FastTab{VT}, WF, S, p, b, xn, xo, lane, red, o, q);
        } else if (PREFETCH) {
            item_eval_prefetch<DIM, TRAP>(P, VT, WF, S, p, b, xn, xo, lane, red, o, q);
        } else {
            item_eval<DIM, TRAP>(P, VT, WF, S, p, b, xn, xo, lane, red, o, q);
        }
    }
}

// =====================================================================================
// K1 "grid" (variant 13): pipe2's per-item arithmetic on a plain grid -- pipe_pair on the global table image
// (pigs_k1_device.h: item_eval_pipe = the four passes in order, new distance then old, the same accumulators and
// the same reduction as pipe2_item).  Small launches of a periodic system run this, large ones pipe2: the bits of an
// item's Delta S do not depend on the launch it travels in (a walker's Metropolis chain in the host-driven sampler
// must not depend on how many walkers share the stage or on how they are sharded over GPUs).
// =====================================================================================
template <int DIM>
__global__ __launch_bounds__(256) void k_delta_action_grid(
    DevParams P, const double *__restrict__ paths, const double *__restrict__ VTimg,
    const double *__restrict__ WF, int n_items, const int32_t *__restrict__ walker,
    const int32_t *__restrict__ ipv, const int32_t *__restrict__ ibv,
    const double *__restrict__ xnew, const double *__restrict__ xold,
    double *__restrict__ out, double *__restrict__ parts)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane  = threadIdx.x & (kWave - 1);
    const int wid   = threadIdx.x >> 6;
    const int nwave = gridDim.x * 4;
    const size_t sl = slice_doubles(DIM, P.NpPad);
    double *red = reinterpret_cast<double *>(smem + (size_t)wid * kWaveLds);
    const PipeTab VT{VTimg + 2, P.Nmax + 3};

    for (int item = blockIdx.x * 4 + wid; item < n_items; item += nwave) {
        const int it = __builtin_amdgcn_readfirstlane(item);
        const int w  = walker[it];
        const int p  = ipv[it] - 1;
        const int b  = ibv[it];
        if ((unsigned)w >= (unsigned)P.nW || (unsigned)p >= (unsigned)P.Np || (unsigned)b >= (unsigned)P.M) {
            if (lane == 0) out[it] = __builtin_nan("");
            continue;
        }
        double xn[DIM], xo[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            xn[k] = xnew[(size_t)it * DIM + k];
            xo[k] = xold[(size_t)it * DIM + k];
        }
        item_eval_pipe<DIM>(P, VT, WF, paths + ((size_t)w * P.M + b) * sl, p, b, xn, xo, lane, red, out + it,
                            parts ? parts + (size_t)it * 3 : nullptr);
    }
}

// =====================================================================================
// K1 "reference order" (variant 14, validation): one wave per item, one item per workgroup.  Every partner's terms
// are computed with the exact-term arithmetic (bit-identical to the reference's per-pair terms) and parked in LDS
// (Np x 8 doubles); then lane q adds column q over jp = 1..Np in the reference's order (vpi_mod.f90:2697-2823:
// PotNew, PotOld, Fnew(k), Fold(k); UpdateWf 2580-2650: PsiNew, PsiOld), starting from the trap's one-body terms
// exactly where the reference starts from them.  A partner outside the cutoff parks +0.0, which leaves a sum's bits
// alone.  Delta S then equals the reference's bit for bit -- BASELINE config 2's "pair-action kernel vs CPU
// bit-compare" taken literally (tests/test_gpu_parity.py::test_reference_order_kernel_is_bit_identical).
// =====================================================================================
template <int DIM, bool TRAP, int CLS>
__device__ __forceinline__ void reforder_item(const DevParams &P, const double *__restrict__ VT, const double *__restrict__ WF,
                                              const double *__restrict__ S, int p, int b, const double (&xn)[DIM],
                                              const double (&xo)[DIM], int lane, double *T, double *out, double *parts)
{
    // columns: 0 potN 1 potO 2..4 fN 5..7 fO (odd) / 2 psiN 3 psiO (end)
    for (int j = lane; j < P.Np; j += kWave) {
        Acc<DIM, CLS> A;
        if (j != p) {
            double rj[DIM];
#pragma unroll
            for (int k = 0; k < DIM; ++k) rj[k] = S[(size_t)k * P.NpPad + j];
            partner_accumulate_at<DIM, TRAP, CLS>(P, VT, WF, rj, xn, xo, A);
        }
        double *t = T + (size_t)j * 8;
        t[0] = A.potN; t[1] = A.potO;
        if (CLS == CLS_ODD) {
#pragma unroll
            for (int k = 0; k < DIM; ++k) { t[2 + k] = A.fN[k]; t[5 + k] = A.fO[k]; }
        } else if (CLS == CLS_END) {
            t[2] = A.psiN; t[3] = A.psiO;
        }
    }
    __builtin_amdgcn_wave_barrier();
    __syncthreads();
    double s = 0.0;
    if (lane < 8) {
        if (TRAP) {                                               // the one-body terms come first: vpi_mod.f90:2688-2695, 2555-2560
            Acc<DIM, CLS> A0;
            trap_terms<DIM, TRAP, CLS>(P, xn, xo, A0);
            double col[8] = {A0.potN, A0.potO, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (CLS == CLS_ODD) {
#pragma unroll
                for (int k = 0; k < DIM; ++k) { col[2 + k] = A0.fN[k]; col[5 + k] = A0.fO[k]; }
            } else if (CLS == CLS_END) {
                col[2] = A0.psiN; col[3] = A0.psiO;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) if (lane == q) s = col[q];
        }
        for (int j = 0; j < P.Np; ++j) {
            if (j == p) continue;                                 // vpi_mod.f90:2699
            s = s + T[(size_t)j * 8 + lane];
        }
    }
    const double c0 = read_lane(s, 0), c1 = read_lane(s, 1);
    double dF2 = 0.0, dPsi = 0.0;
    if (CLS == CLS_ODD) {
        double fn2 = 0.0, fo2 = 0.0;
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            const double a = read_lane(s, 2 + k), c = read_lane(s, 5 + k);
            fn2 = fn2 + a * a;                                    // :2831-2832
            fo2 = fo2 + c * c;
        }
        dF2 = fn2 - fo2;                                          // :2835
    } else if (CLS == CLS_END) {
        dPsi = read_lane(s, 2) - read_lane(s, 3);                 // :2653
    }
    const double dPot = c0 - c1;                                  // :2838
    if (lane == 0) {
        *out = -dPsi + green_function(0, b, P.Nb, P.dt, dPot, dF2);   // :2527 (plain IEEE divisions)
        if (parts) { parts[0] = dPot; parts[1] = dF2; parts[2] = dPsi; }
    }
}

template <int DIM, bool TRAP>
__global__ __launch_bounds__(64) void k_delta_action_reforder(
    DevParams P, const double *__restrict__ paths, const double *__restrict__ VT,
    const double *__restrict__ WF, int n_items, const int32_t *__restrict__ walker,
    const int32_t *__restrict__ ipv, const int32_t *__restrict__ ibv,
    const double *__restrict__ xnew, const double *__restrict__ xold,
    double *__restrict__ out, double *__restrict__ parts)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double *T = reinterpret_cast<double *>(smem);
    const int lane = threadIdx.x;
    const size_t sl = slice_doubles(DIM, P.NpPad);
    for (int it = blockIdx.x; it < n_items; it += gridDim.x) {
        const int w = walker[it], p = ipv[it] - 1, b = ibv[it];
        if ((unsigned)w >= (unsigned)P.nW || (unsigned)p >= (unsigned)P.Np || (unsigned)b >= (unsigned)P.M) {
            if (lane == 0) out[it] = __builtin_nan("");
            continue;
        }
        double xn[DIM], xo[DIM];
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            xn[k] = xnew[(size_t)it * DIM + k];
            xo[k] = xold[(size_t)it * DIM + k];
        }
        const double *S = paths + ((size_t)w * P.M + b) * sl;
        double *o = out + it;
        double *q = parts ? parts + (size_t)it * 3 : nullptr;
        const bool odd  = (b & 1) != 0;
        const bool endb = (b == 0) || (b == 2 * P.Nb);
        if (odd)       reforder_item<DIM, TRAP, CLS_ODD>(P, VT, WF, S, p, b, xn, xo, lane, T, o, q);
        else if (endb) reforder_item<DIM, TRAP, CLS_END>(P, VT, WF, S, p, b, xn, xo, lane, T, o, q);
        else           reforder_item<DIM, TRAP, CLS_EVEN>(P, VT, WF, S, p, b, xn, xo, lane, T, o, q);
        __syncthreads();
    }
}

// =====================================================================================
// Pieces of the persistent kernel: the LDS image of the VTable
// =====================================================================================
__device__ __forceinline__ size_t pipe_tab_bytes(int nt) { return ((size_t)(nt + 6) * sizeof(double) + 15) & ~(size_t)15; }

// Staging the table image with the LDS-DMA form of the global load (global_load_lds_dwordx4: 16 bytes per lane
// straight into LDS at M0 + lane*16, no VGPRs, no ds_write).  Completion is a vmcnt matter, and vmcnt retires in
// order.  The chunks are no quick L2 hits -- every CU of an XCD pulls the same table through that XCD's L2 at the same
// moment -- so nothing the first item needs may queue behind them.  The order of a wave's head is therefore:
//   1. the static first record, through the scalar unit (pipe2_request_first: lgkmcnt, independent of vmcnt);
//   2. the table chunks, then the odd last entry (the last wave: one more LDS-DMA load, two lanes of a dword each);
//   3. as soon as the record is in (lgkmcnt(0), the chunks still in flight): the first item's slice loads.
// The wait before the workgroup barrier (pipe_table_dma_finish) then leaves exactly those slice loads -- the last VMEM
// requests the wave issued -- in flight, so a wave's own loads cost max(table, record + slice) and the barrier
// overlaps the rest of the slice latency.  (With the record on vector loads behind the chunks, the slice's HBM
// latency started only after the table was in: max(table, record) + slice.)  A wave issues the chunk
// [u*blockDim + wid*64, +64) only if it starts inside the table; lanes past the end are masked off.  The odd last
// entry stays ahead of the slice loads so that the same wait covers it, and goes to LDS by DMA like the rest: as a
// load into a register it stayed pending in the compiler's books past that wait, and drew a vmcnt(0) of its own.

constexpr int kPipeThreads = 1024;                  // the persistent kernel's workgroup: 16 waves, a constant so that the
                                                    // chunk loop needs no dispatch-packet load behind the first record's

__device__ __forceinline__ void pipe_table_dma_issue(unsigned char *smem, const double *__restrict__ VTg, int nt, int wid, int lane)
{
#ifndef PIGS_EXPERIMENT_NO_STAGE
    const double2 *src = reinterpret_cast<const double2 *>(VTg);
    const int n2 = nt / 2;
    for (int cb = wid * kWave; cb < n2; cb += kPipeThreads) {         // wave-uniform
        const int idx = cb + lane;
        auto *l = reinterpret_cast<__attribute__((address_space(3))) void *>(
            (__attribute__((address_space(3))) unsigned char *)smem + 16 + (size_t)cb * 16);
        // lanes past the end of the table are masked off (EXEC): they neither load nor write their LDS slot
        if (idx < n2) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + idx), l, 16, 0, 0);
    }
    if ((nt & 1) && wid == kPipeThreads / kWave - 1) {                // the odd last entry: two dwords, lanes 0 and 1 of the last wave
        const int32_t *t = reinterpret_cast<const int32_t *>(VTg + (nt - 1));
        auto *l = reinterpret_cast<__attribute__((address_space(3))) void *>(
            (__attribute__((address_space(3))) unsigned char *)smem + 16 + (size_t)(nt - 1) * 8);
        if (lane < 2) __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(t + lane), l, 4, 0, 0);
    }
#endif
}

// after this and a workgroup barrier the image is complete.  IN_FLIGHT: the VMEM requests the wave issued after
// the table chunks (its first item's slice loads) that may stay outstanding.  The wait is the builtin, not inline
// assembly: the compiler has to see it.  Its own books count an LDS-DMA load as pending on vmcnt out of order until a
// wait it knows of; nothing else in the head waits on vmcnt any more, and without this one it put a vmcnt(0) -- the
// slice loads included -- in front of the barrier.  (gfx9 encoding: vmcnt in bits 3:0, expcnt 6:4 and lgkmcnt 11:8
// left at their maxima.)
template <int IN_FLIGHT>
__device__ __forceinline__ PipeTab pipe_table_dma_finish(unsigned char *smem, int nt)
{
    double *base = reinterpret_cast<double *>(smem);          // base[1] = leading copy, base[2..] = table
    double *tab  = base + 2;
    static_assert(IN_FLIGHT >= 0 && IN_FLIGHT < 16, "vmcnt beyond the low four bits");
    __builtin_amdgcn_s_waitcnt(0x0F70 | IN_FLIGHT);
    if (threadIdx.x == 0) {
        base[0] = 0.0; base[1] = tab[0];                          // wave 0 staged chunk 0 itself: tab[0] has landed
        tab[nt] = 0.0; tab[nt + 1] = 0.0; tab[nt + 2] = 0.0; tab[nt + 3] = 0.0;
    }
    return PipeTab{tab, nt + 1};
}

// =====================================================================================
// K1 "pipe2": the short-arithmetic item evaluation as a persistent, software-pipelined kernel (PBC, Np <= 256).
// One 1024-thread workgroup per CU keeps the VTable image in LDS -- the table gather was what kept the texture
// addresser 60-65 % busy in v2 and held every wave on s_waitcnt; LDS gathers count on lgkmcnt, so they never wait
// for outstanding global loads -- and its 16 waves draw the workgroup's items (blockIdx + k*gridDim: one walker's
// consecutive beads spread over all CUs) from an LDS counter, because odd beads cost more than even ones.  The two
// distances of a pass are branch-free, independent chains (masked lanes look up the table's zero cell).  A wave
// that started every item with its dependent chain -- scalar loads of the item record, then the slice loads whose
// address they give, ~3 us -- reached 78 % VALU occupancy; here (a) a wave draws its next item from the queue at the
// top of the current one and requests that record with vector loads before anything else (vmcnt is in order, so the
// record lands ahead of the pass-2 coordinates the wave has to wait for anyway; unlike scalar loads, vector loads do
// not force an lgkmcnt drain at the next LDS gather); it is decoded after pass 1 with v_readfirstlane / v_readlane;
// (b) the partner coordinates run two passes ahead: pass m+2 of this item, then passes 0/1 of the next item, are
// requested before pass m is evaluated, in the same 4 x DIM registers.  A wave thus owns its current item and ONE
// claimed item, never two: when the queue runs dry no wave sits on two unstarted items while another has none.
// =====================================================================================
template <int DIM>
struct ItemMeta {                                   // wave-uniform (SGPRs)
    int    p, b, ok;
    const double *S;
    int    nb;                                      // bytes of a coordinate row (0 for a malformed or empty record)
    int    np;                                      // partners' rows: Np (0 likewise).  Per item on purpose: tested against
                                                    // P.Np, the four passes' lane masks are loop invariants that get hoisted and then spill
    double xn[DIM], xo[DIM];
};

// an item record as it arrives: walker / ip / ib in every lane (wave-uniform loads), xnew / xold in lanes 0..DIM-1
struct ItemRaw {
    int    w, ip, ib;
    double xn, xo;
};

// the item arrays of a launch and the workgroup's queue over them (wave-uniform)
struct PipeQueue {
    const int32_t *walker, *ipv, *ibv;
    const double *xnew, *xold;
    int *next;                                      // LDS counter: the next queue index nobody has drawn yet
    int n_local;                                    // items of this workgroup: blockIdx + k * gridDim, k < n_local
};

constexpr int kPipeBufFlags = 0x00020000;           // raw buffer, 32-bit data format: out-of-range lanes read 0

// Request the record of queue index k.  The index is wave-uniform, so the five addresses are SALU work: each field
// comes through a buffer descriptor that covers exactly that item's entry -- 4 bytes of walker / ip / ib at offset 0
// (no VGPR address at all), DIM*8 bytes of xnew / xold at the lane's lane*8 (lanes >= DIM are out of range: 0).
// Vector loads all the same (see above: vmcnt is in order and leaves lgkmcnt to the LDS gathers).  k >= n_local:
// empty descriptors, no memory traffic, and the record reads as ip = 0 -- a malformed record, so whatever looks ahead
// through it gets the empty slice without a case of its own.
template <int DIM>
__device__ __forceinline__ ItemRaw pipe2_request(const PipeQueue &Q, int k, int lane)
{
    const bool has = k < Q.n_local;
    const int it = (int)blockIdx.x + (has ? k : 0) * (int)gridDim.x;
    const int ni = has ? 4 : 0, nx = has ? DIM * 8 : 0;
    const auto ld_i = [&](const int32_t *a) {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t *>(a + it), 0, ni, kPipeBufFlags);
        return (int)__builtin_amdgcn_raw_buffer_load_b32(rs, 0, 0, 0);
    };
    const auto ld_x = [&](const double *a) {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(a + (size_t)it * DIM), 0, nx, kPipeBufFlags);
        return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, (unsigned)lane * 8u, 0, 0));
    };
    ItemRaw r;
    r.w  = ld_i(Q.walker);
    r.ip = ld_i(Q.ipv);
    r.ib = ld_i(Q.ibv);
    r.xn = ld_x(Q.xnew);
    r.xo = ld_x(Q.xold);
    return r;
}

// The record of a wave's STATIC first item (queue index wid), at the kernel's entry only: through the scalar unit.
// Its address is known from the launch alone, and scalar loads count on lgkmcnt, so the record does not queue behind
// the wave's table chunks on the in-order vmcnt (see pipe_table_dma_issue); the lgkmcnt drain that keeps scalar loads
// out of the steady state costs nothing here, where no LDS gather has been issued yet.  The fields land in SGPRs:
// no readlanes.  A wave without a first item reads nothing and gets the empty record of pipe2_request (ip = 0).
template <int DIM>
struct ItemFirst {                                  // wave-uniform (SGPRs)
    int    w, ip, ib;
    double xn[DIM], xo[DIM];
};

template <int DIM>
__device__ __forceinline__ ItemFirst<DIM> pipe2_request_first(const PipeQueue &Q, int it, bool has)
{
    ItemFirst<DIM> r = {};
    if (has) {                                      // wave-uniform: `it` is blockIdx + wid * gridDim
        r.w  = Q.walker[it];
        r.ip = Q.ipv[it];
        r.ib = Q.ibv[it];
#pragma unroll
        for (int k = 0; k < DIM; ++k) {
            r.xn[k] = Q.xnew[(size_t)it * DIM + k];
            r.xo[k] = Q.xold[(size_t)it * DIM + k];
        }
    }
    return r;
}

__device__ __forceinline__ double bcast_lane(double v, int lane_id)
{
    union { double d; int i[2]; } u;
    u.d = v;
    u.i[0] = __builtin_amdgcn_readlane(u.i[0], lane_id);
    u.i[1] = __builtin_amdgcn_readlane(u.i[1], lane_id);
    return u.d;
}

// The two halves of a record's decode.  The slice half (indices, range check, slice address) is what the coordinate
// look-ahead needs mid-item; the coordinate half waits for the item's own turn, so that two items' xnew / xold never
// compete for SGPRs.  A malformed or empty record gets nb = 0: every load of its slice is a no-op.
template <int DIM>
__device__ __forceinline__ void pipe2_slice_of(const DevParams &P, const double *__restrict__ paths, int w, int ip, int ib,
                                               size_t sl, ItemMeta<DIM> &R)
{
    R.p = ip - 1;
    R.b = ib;
    R.ok = (unsigned)w < (unsigned)P.nW && (unsigned)R.p < (unsigned)P.Np && (unsigned)R.b < (unsigned)P.M;
    R.S = paths + (R.ok ? ((size_t)w * P.M + R.b) * sl : 0);
    R.nb = R.ok ? P.NpPad * 8 : 0;
    R.np = R.ok ? P.Np : 0;
}

template <int DIM>
__device__ __forceinline__ void pipe2_decode_slice(const DevParams &P, const double *__restrict__ paths, const ItemRaw &r,
                                                   size_t sl, ItemMeta<DIM> &R)
{
    pipe2_slice_of<DIM>(P, paths, __builtin_amdgcn_readfirstlane(r.w), __builtin_amdgcn_readfirstlane(r.ip),
                        __builtin_amdgcn_readfirstlane(r.ib), sl, R);
}

template <int DIM>
__device__ __forceinline__ void pipe2_decode_coords(const ItemRaw &r, ItemMeta<DIM> &R)
{
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
        R.xn[k] = bcast_lane(r.xn, k);
        R.xo[k] = bcast_lane(r.xo, k);
    }
}

// Partner coordinates of pass m through one buffer descriptor per coordinate row (base S + k NpPad, NpPad*8 bytes;
// SALU work only): the lane's byte offset is lane*8 + m*512, one compare and select per pass.
// The range check does the rest -- a lane past NpPad (passes beyond NpPad exist when Np < 256) gets 0.0 and reads
// nothing, never the next row or the next slice, and so does the moved particle's own row, which is given an offset
// past the end (vpi_mod.f90:2699: row p is never read).  Every lane gets finite data; the lanes that are not partners
// are masked through the table's zero cell as before, and contribute exactly +0 whatever finite values they hold.
// nbytes = 0 (no next item, malformed record) makes every load of the slice a no-op.
constexpr unsigned kPipeRowOff = 0x40000000u;                         // an offset past any coordinate row

template <int DIM>
__device__ __forceinline__ void pipe2_load(const DevParams &P, const double *__restrict__ S, int nbytes, int p, int m,
                                           int lane, double (&rj)[DIM])
{
    const unsigned off = (lane == p - m * kWave ? kPipeRowOff : (unsigned)lane * 8u) + (unsigned)(m * kWave * 8);
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
        const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(S + (size_t)k * P.NpPad), 0, nbytes, 0x00020000);
        rj[k] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, 0));
    }
}

template <int DIM, int CLS, int M>
__device__ __forceinline__ void pipe2_pass(const DevParams &P, PipeTab VT, const double *__restrict__ WF,
                                           const ItemMeta<DIM> &R, const double (&rjm)[DIM], int lane, Acc<DIM, CLS> &A)
{
    const int j = M * kWave + lane;
    const bool valid = j < R.np && j != R.p;
    double dn[DIM], dold[DIM];
#pragma unroll
    for (int k = 0; k < DIM; ++k) {
        double rj = rjm[k];
        asm volatile("; class %1 pass %2" : "+v"(rj) : "n"(CLS), "n"(M));     // opaque per (class, pass): keeps the optimiser
                                                                              // from hoisting all four passes' distance arithmetic above the class branch (spills)
        dn[k] = R.xn[k] - rj; dold[k] = R.xo[k] - rj;
    }
    const double r2o = pipe_r2<DIM, CLS>(dold, P);
    const double r2n = pipe_r2<DIM, CLS>(dn, P);
    pipe_pair<DIM, CLS, false>(P, VT, WF, floor_r2(r2n), valid && r2n <= P.rcut2, dn, A);
    pipe_pair<DIM, CLS, true>(P, VT, WF, floor_r2(r2o), valid && r2o <= P.rcut2, dold, A);
    __builtin_amdgcn_sched_barrier(0);
}

// per-wave pipeline state that crosses items
template <int DIM>
struct PipeState {
    int k_next;               // queue index of the claimed item (>= n_local: none, and its record is empty)
    ItemRaw raw_next;         // its record: requested at the top of the current item, coordinates decoded at its turn
    ItemMeta<DIM> next;       // the slice half of its decode (after pass 1); xn / xo follow at its turn
    double a0[DIM], a1[DIM];  // passes 0/1: of the current item on entry, of the claimed item on exit
};

// The look-ahead of one item in three steps, shared by pipe2_item and by the malformed-record path of the kernel:
//   claim   draw the next queue index and request its record -- the first VMEM instructions of the item, so the record
//           lands before the item's own pass-2 coordinates do.  A draw past the end tells the wave that the current
//           item is its last; the record request and the loads below still run (a branch there costs ~40 spilled
//           VGPRs), on empty descriptors: no memory traffic at all;
//   ahead0  (after pass 1) decode the record's slice and request its pass-0 coordinates;
//   ahead1  request its pass-1 coordinates.
template <int DIM>
__device__ __forceinline__ void pipe2_claim(const PipeQueue &Q, int lane, PipeState<DIM> &st)
{
    int kn = 0;
    if (lane == 0) kn = atomicAdd(Q.next, 1);
    st.k_next = __builtin_amdgcn_readfirstlane(kn);
    st.raw_next = pipe2_request<DIM>(Q, st.k_next, lane);
}

template <int DIM>
__device__ __forceinline__ void pipe2_ahead0(const DevParams &P, const double *__restrict__ paths, size_t sl, int lane,
                                             PipeState<DIM> &st)
{
    pipe2_decode_slice<DIM>(P, paths, st.raw_next, sl, st.next);
    pipe2_load<DIM>(P, st.next.S, st.next.nb, st.next.p, 0, lane, st.a0);
}

template <int DIM>
__device__ __forceinline__ void pipe2_ahead1(const DevParams &P, int lane, PipeState<DIM> &st)
{
    pipe2_load<DIM>(P, st.next.S, st.next.nb, st.next.p, 1, lane, st.a1);
}

template <int DIM, int CLS>
__device__ __forceinline__ void pipe2_item(const DevParams &P, PipeTab VT, const double *__restrict__ WF,
                                           const double *__restrict__ paths, size_t sl, const PipeQueue &Q,
                                           const ItemMeta<DIM> &R, PipeState<DIM> &st, int lane, double *red,
                                           double *out, double *parts)
{
    Acc<DIM, CLS> A;
    double b0[DIM], b1[DIM];
    pipe2_claim<DIM>(Q, lane, st);
    pipe2_load<DIM>(P, R.S, R.nb, R.p, 2, lane, b0);
    pipe2_pass<DIM, CLS, 0>(P, VT, WF, R, st.a0, lane, A);
    pipe2_load<DIM>(P, R.S, R.nb, R.p, 3, lane, b1);
    pipe2_pass<DIM, CLS, 1>(P, VT, WF, R, st.a1, lane, A);
    pipe2_ahead0<DIM>(P, paths, sl, lane, st);
    pipe2_pass<DIM, CLS, 2>(P, VT, WF, R, b0, lane, A);
    pipe2_ahead1<DIM>(P, lane, st);
    pipe2_pass<DIM, CLS, 3>(P, VT, WF, R, b1, lane, A);
    finish_item<DIM, CLS>(P, lane, R.b, A, red, out, parts);
}

// -DPIGS_EXPERIMENT_K1_CLOCK (experiment builds only): lane 0 of every pipe2 wave records, with an ordinary global
// store at its end, four s_memrealtime stamps (100 MHz, one clock for the whole chip) and its item count into
// k1_clock[(blockIdx * 16 + wave) * 5]: entry, its table chunks and first records landed (its first slice loads still
// in flight), past the workgroup barrier (the first table lookup follows within one pass's distance arithmetic), end.
// The last launch's record is read by pigs_k1_clock_read(); scripts/k1_head.py turns it into the head / tail split of
// profiles/r04_* and r05_*.
#ifdef PIGS_EXPERIMENT_K1_CLOCK
constexpr int kK1ClockWaves = 16 * 1024;
__device__ unsigned long long k1_clock[kK1ClockWaves * 5];
#define K1STAMP(v) const unsigned long long v = __builtin_amdgcn_s_memrealtime()
#else
#define K1STAMP(v) do { } while (0)
#endif

template <int DIM>
__global__ __launch_bounds__(kPipeThreads) void k_delta_action_pipe2(
    DevParams P, const double *__restrict__ paths, const double *__restrict__ VTg,
    const double *__restrict__ WF, int n_items, const int32_t *__restrict__ walker,
    const int32_t *__restrict__ ipv, const int32_t *__restrict__ ibv,
    const double *__restrict__ xnew, const double *__restrict__ xold,
    double *__restrict__ out, double *__restrict__ parts)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int next_local;                                  // this workgroup's item queue
    const int lane  = threadIdx.x & (kWave - 1);
    const int wid   = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t sl = slice_doubles(DIM, P.NpPad);
    const int n_local = (n_items - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;

    // only the first item of a wave is static (k = wid); the queue starts behind those 16, and every further item is
    // drawn from it one item ahead (pipe2_claim)
    int k_cur = wid;
    const PipeQueue Q{walker, ipv, ibv, xnew, xold, &next_local, n_local};
    ItemMeta<DIM> cur;
    PipeState<DIM> st;
    const int nt = P.Nmax + 2;
    K1STAMP(t_entry);
    // the head: record (scalar, lgkmcnt) -> table chunks + tail (vmcnt) -> slice loads behind them, issued as soon as
    // the record is in and while the chunks are still in flight.  it0 < n_items is wid < n_local without the division.
    const int it0 = (int)blockIdx.x + wid * (int)gridDim.x;
    const ItemFirst<DIM> r0 = pipe2_request_first<DIM>(Q, it0, it0 < n_items);   // (no first item: the empty record)
    pipe_table_dma_issue(smem, VTg, nt, wid, lane);
    {
        pipe2_slice_of<DIM>(P, paths, r0.w, r0.ip, r0.ib, sl, cur);
#pragma unroll
        for (int k = 0; k < DIM; ++k) { cur.xn[k] = r0.xn[k]; cur.xo[k] = r0.xo[k]; }
        pipe2_load<DIM>(P, cur.S, cur.nb, cur.p, 0, lane, st.a0);
        pipe2_load<DIM>(P, cur.S, cur.nb, cur.p, 1, lane, st.a1);
    }

    const PipeTab VT = pipe_table_dma_finish<2 * DIM>(smem, nt);   // passes 0/1 stay in flight
    K1STAMP(t_loaded);
    if (threadIdx.x == 0) next_local = 16;
    double *red = reinterpret_cast<double *>(smem + pipe_tab_bytes(nt) + (size_t)wid * kWaveLds);
    __syncthreads();                                            // the only workgroup barrier
    K1STAMP(t_ready);
#ifdef PIGS_EXPERIMENT_K1_CLOCK
    int n_done = 0;
#endif

    while (k_cur < n_local) {                                   // wave-uniform
        const int it = (int)blockIdx.x + k_cur * (int)gridDim.x;
        double *o = out + it;
        double *q = nullptr;                                     // the (DeltaPot, DeltaF2, DeltaPsi) diagnostic runs on the plain grid
        if (!cur.ok) {
            // malformed item: NaN result; keep the pipeline moving without evaluating anything
            if (lane == 0) *o = __builtin_nan("");
            pipe2_claim<DIM>(Q, lane, st);
            pipe2_ahead0<DIM>(P, paths, sl, lane, st);
            pipe2_ahead1<DIM>(P, lane, st);
        } else {
            const bool odd  = (cur.b & 1) != 0;
            const bool endb = (cur.b == 0) || (cur.b == 2 * P.Nb);
            if (odd)       pipe2_item<DIM, CLS_ODD>(P, VT, WF, paths, sl, Q, cur, st, lane, red, o, q);
            else if (endb) pipe2_item<DIM, CLS_END>(P, VT, WF, paths, sl, Q, cur, st, lane, red, o, q);
            else           pipe2_item<DIM, CLS_EVEN>(P, VT, WF, paths, sl, Q, cur, st, lane, red, o, q);
        }
        pipe2_decode_slice<DIM>(P, paths, st.raw_next, sl, cur);  // arrived long ago: readlanes only
        pipe2_decode_coords<DIM>(st.raw_next, cur);
        k_cur = st.k_next;
#ifdef PIGS_EXPERIMENT_K1_CLOCK
        ++n_done;
#endif
    }
#ifdef PIGS_EXPERIMENT_K1_CLOCK
    K1STAMP(t_end);
    const int slot = (int)blockIdx.x * 16 + wid;
    if (lane == 0 && slot < kK1ClockWaves) {
        unsigned long long *c = k1_clock + (size_t)slot * 5;
        c[0] = t_entry; c[1] = t_loaded; c[2] = t_ready; c[3] = t_end; c[4] = (unsigned long long)n_done;
    }
#endif
}

// bit-for-bit check of the short division / sqrt forms against the compiler's IEEE ones
__global__ void k_selftest_fastmath(DevParams P, unsigned long long seed, int iters, unsigned long long *bad)
{
    unsigned long long s = seed ^ (0x9E3779B97F4A7C15ull * (blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x + 1));
    unsigned long long b0 = 0, b1 = 0, b2 = 0, b3 = 0;
    for (int i = 0; i < iters; ++i) {
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        const double u1 = (double)(s >> 11) * (1.0 / 9007199254740992.0);
        s ^= s << 13; s ^= s >> 7; s ^= s << 17;
        const double u2 = (double)(s >> 11) * (1.0 / 9007199254740992.0);
        const double rmax2 = 4.0 * P.rcut2;
        const double x = (i & 1) ? u1 * rmax2 : u1 * u1 * 1e-3 + 1e-12;       // r^2 samples
        double sq, y;
        sqrt_rinv(x, sq, y);
        if (sq != sqrt(x)) ++b0;
        const double num = (u2 - 0.5) * ((i & 2) ? 1e6 : 3.0);
        if (div_by(num, sq, y) != num / sq) ++b1;
        if (div_by(sq, P.dr, P.rdr) != sq / P.dr) ++b2;
        if (div_by(num, P.dr, P.rdr) != num / P.dr) ++b3;
    }
    atomicAdd(&bad[0], b0); atomicAdd(&bad[1], b1); atomicAdd(&bad[2], b2); atomicAdd(&bad[3], b3);
}

// =====================================================================================
// launcher
// =====================================================================================
static int k1_grid(int n_items, int waves_per_block, int cap_blocks)
{
    int blocks = (n_items + waves_per_block - 1) / waves_per_block;
    return blocks < cap_blocks ? (blocks > 0 ? blocks : 1) : cap_blocks;
}

hipError_t launch_delta_action(const DevParams &P, int variant, const double *paths, const double *VT,
                               const double *VTimg, const double *WF, int n_items, const int32_t *walker,
                               const int32_t *ip, const int32_t *ib, const double *xnew,
                               const double *xold, double *out, double *parts, hipStream_t st)
{
    if (n_items <= 0) return hipSuccess;
    const size_t pipe_bytes = (((size_t)(P.Nmax + 2 + 6) * sizeof(double)) + 15) & ~(size_t)15;   // pipe_tab_bytes()
    const bool can_pipe = !P.trap && P.Np <= 256 && VTimg && pipe_bytes + 16 * kWaveLds <= 160 * 1024;
    if (variant == K1_AUTO) {
        // The arithmetic form follows from the SYSTEM, never from the size of the launch: trapped systems the exact-term
        // form; periodic systems with Np <= 256 the pipe arithmetic -- persistent LDS-table kernel once a launch fills its
        // 16 waves per CU several times over, the same per-item code on a plain grid below that (identical bits);
        // periodic systems beyond 256 particles the short arithmetic on the global table.
        if (P.trap) variant = K1_V2;
        else if (can_pipe) variant = (n_items >= 16 * device_cus() && !parts) ? K1_PIPE2 : K1_GRID;
        else variant = K1_FAST;
    }
    if ((variant == K1_PIPE2 || variant == K1_GRID) && !can_pipe) variant = P.trap ? K1_V2 : K1_FAST;
    if (variant == K1_PIPE2 && parts) variant = K1_GRID;        // pipe2 has no registers to spare for the diagnostic output: same arithmetic on the grid
    if (variant == K1_FAST_PREFETCH && P.Np > 256) variant = K1_FAST;
    if ((variant == K1_FAST || variant == K1_FAST_PREFETCH) && P.trap) variant = K1_V2;   // no cutoff in the trap: exact path
    switch (variant) {
    case K1_V1:
        return with_flag(P.trap, [&](auto T) {
            return with_dim(P.dim, [&](auto D) {
                return launch<k_delta_action_v1<D(), T()>>(dim3(k1_grid(n_items, 4, 2048)), dim3(256), 0, st, P, paths, VT, WF,
                                                           n_items, walker, ip, ib, xnew, xold, out, parts);
            });
        });
    case K1_V2:
    case K1_FAST:
    case K1_FAST_PREFETCH: {
        const size_t lds = 4 * kWaveLds;
        const dim3 grid(k1_grid(n_items, 4, 1 << 22));
        return with_flag(P.trap, [&](auto T) {
            return with_dim(P.dim, [&](auto D) {
                if (variant == K1_V2)
                    return launch<k_delta_action_v2<D(), T(), 256, false, false>>(grid, dim3(256), lds, st, P, paths, VT, WF, n_items,
                                                                                 walker, ip, ib, xnew, xold, out, parts);
                if (variant == K1_FAST)
                    return launch<k_delta_action_v2<D(), T(), 256, false, true>>(grid, dim3(256), lds, st, P, paths, VT, WF, n_items,
                                                                                walker, ip, ib, xnew, xold, out, parts);
                return launch<k_delta_action_v2<D(), T(), 256, true, true>>(grid, dim3(256), lds, st, P, paths, VT, WF, n_items,
                                                                           walker, ip, ib, xnew, xold, out, parts);
            });
        });
    }
    case K1_GRID:
        return with_dim(P.dim, [&](auto D) {
            return launch<k_delta_action_grid<D()>>(dim3(k1_grid(n_items, 4, 1 << 22)), dim3(256), 4 * kWaveLds, st, P, paths,
                                                    VTimg, WF, n_items, walker, ip, ib, xnew, xold, out, parts);
        });
    case K1_PIPE2: {
        const size_t lds = pipe_bytes + 16 * kWaveLds;
        int blocks = (n_items + 15) / 16;
        if (blocks > device_cus()) blocks = device_cus();       // persistent grid: one 1024-thread workgroup per CU
        return with_dim(P.dim, [&](auto D) {
            return launch<k_delta_action_pipe2<D()>>(dim3(blocks), dim3(kPipeThreads), lds, st, P, paths, VT, WF, n_items, walker, ip, ib,
                                                     xnew, xold, out, parts);
        });
    }
    case K1_REFORDER: {
        const size_t lds = (size_t)P.Np * 8 * sizeof(double);
        if (lds > 160 * 1024) return hipErrorInvalidValue;
        const int grid = n_items < (1 << 16) ? n_items : (1 << 16);
        return with_flag(P.trap, [&](auto T) {
            return with_dim(P.dim, [&](auto D) {
                return launch<k_delta_action_reforder<D(), T()>>(dim3(grid), dim3(64), lds, st, P, paths, VT, WF, n_items, walker,
                                                                 ip, ib, xnew, xold, out, parts);
            });
        });
    }
    default:
        return hipErrorInvalidValue;
    }
}

#ifdef PIGS_EXPERIMENT_K1_CLOCK
// the clock records of the last pipe2 launch (n_waves x 5 words, see k1_clock); synchronises the device
extern "C" int pigs_k1_clock_read(unsigned long long *dst, int n_waves)
{
    if (!dst || n_waves <= 0 || n_waves > kK1ClockWaves) return -1;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(k1_clock), (size_t)n_waves * 5 * sizeof(unsigned long long), 0,
                               hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
}
#endif

hipError_t launch_selftest_fastmath(const DevParams &P, unsigned long long seed, int blocks, int iters,
                                    unsigned long long *d_bad, hipStream_t st)
{
    return launch<k_selftest_fastmath>(dim3(blocks), dim3(256), 0, st, P, seed, iters, d_bad);
}

} // namespace pigs
