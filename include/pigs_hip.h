/* pigs_hip.h -- C ABI of libpigs_hip.so: the MI355X (gfx950) drop-in for the PIGS
 * action / energy hot path of amaciarey/PathIntegralGroundState.
 *
 * The reference has no FFI: its boundary is the Fortran procedure interface
 * (SURVEY.md §8b).  Each entry point below names the reference procedure(s) it
 * replaces (file:line under the reference tree).  A Fortran host binds these with
 * ISO_C_BINDING (pathintegralgroundstate_amd/host/pigs_capi.f90).
 *
 * Conventions (identical to the reference so that a Fortran caller passes its arrays
 * unchanged): fp64 everywhere; arrays column-major; Path(dim,Np,0:2*Nb); tables
 * F(0:Nmax+1) with the pointer at element 0; particle indices ip are 1-BASED, bead
 * indices ib 0-BASED, walker indices 0-based (walkers are new: the reference has one).
 * Every function returns PIGS_OK (0) or a negative pigs_status; nothing calls exit/stop.
 * A context is bound to one device and one stream; calls on one context must be
 * serialized by the caller (one host thread per GPU); there is no global mutable state.
 */
#ifndef PIGS_HIP_H
#define PIGS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PIGS_ABI_VERSION 1
#define PIGS_MAXDIM 3

typedef enum pigs_status {
    PIGS_OK              = 0,
    PIGS_ERR_ARG         = -1,  /* bad argument / out-of-range index               */
    PIGS_ERR_HIP         = -2,  /* HIP runtime error (pigs_last_error has the text) */
    PIGS_ERR_NO_DEVICE   = -3,  /* no gfx950 device visible                        */
    PIGS_ERR_UNSUPPORTED = -4,  /* e.g. v_table=F with force terms (reference Q3)  */
    PIGS_ERR_COMM        = -5   /* RCCL error                                      */
} pigs_status;

/* The module globals the reference hot path reads implicitly
 * (global_mod.f90:5-12: dim,Np,Nb,Nmax,dr,rcut2,wf_table,v_table,Lbox,LboxHalf;
 *  system_mod.f90:8-9: Rm,a_ho) plus dt, which the reference passes per call. */
typedef struct pigs_params {
    int32_t dim, Np, Nb, Nmax;
    int32_t trap, wf_table, v_table, reserved;
    double  dr, rcut2, dt, Rm;
    double  Lbox[PIGS_MAXDIM];
    double  a_ho[PIGS_MAXDIM];
} pigs_params;

typedef struct pigs_ctx pigs_ctx;

/* ---- lifetime ------------------------------------------------------------------ */
/* Replaces the module-global set-up of vpi.f90:76-153 for the hot path: uploads both
 * tables (built host-side by the caller exactly as vpi_mod.f90:84-145 builds them, or
 * by pigs_build_tables) and reserves HBM for n_walkers resident worldlines. */
/* wf_table = 0 (the reference's default, vpi_mod.f90:59): the trial function is evaluated analytically (McMillan
 * u(r) = -0.5 (Rm/r)^5, system_mod.f90:38-66) and LogWF may be NULL.  v_table = 1 is mandatory (quirk Q3). */
int pigs_ctx_create(const pigs_params *p, const double *VTable, const double *LogWF,
                    int32_t n_walkers, int32_t device_id, pigs_ctx **out);
int pigs_ctx_destroy(pigs_ctx *ctx);
const char *pigs_last_error(void);
int pigs_abi_version(void);
int pigs_device_count(int32_t *n);
/* Blocks until all work queued on the context's stream has finished. */
int pigs_sync(pigs_ctx *ctx);
/* The context's hipStream_t (as void*) so a host can order its own work against it. */
int pigs_stream(pigs_ctx *ctx, void **hip_stream);

/* Tuning knobs.
 *   "k1_variant": which Delta-S kernel pigs_delta_action_* runs.
 *        0  auto (default).  The arithmetic follows from the SYSTEM, never from the size of a launch (an item's bits
 *           must not depend on what else travels with it): periodic systems with Np <= 256 use the short arithmetic
 *           -- every per-pair term to ~1 ulp, cutoff membership unchanged -- in the persistent
 *           LDS-table kernel (12) for launches of >= 16 items per CU and in its plain-grid twin (13, identical bits)
 *           below that; periodic systems beyond 256 particles use 7; trapped systems use 2
 *        1  plain statement of the reference's arithmetic          2  same terms bit for bit, short exact division
 *        7  short arithmetic on the global table                   8  7 + partner loads issued up front
 *        12 persistent LDS-table kernel, branch-free short arithmetic, look-ahead loads
 *        13 the per-item arithmetic of 12 on a plain grid (global table image)
 *        14 validation: the terms of 2 added in the reference's jp order -- Delta S, DeltaPot, DeltaF2 and DeltaLogPsi
 *           equal the reference's bit for bit (BASELINE config 2's "pair-action kernel vs CPU bit-compare")
 *      1, 2 and 14 sum bit-identical terms (1 / 2 in lane-strided order); 7-13 agree with them to ~1e-15 per term.
 *      (3-6, 9-11 were A/B forms of round 1 and are gone.)
 *      The environment variable PIGS_K1_VARIANT presets this key at pigs_ctx_create (test hook).
 *   "sweep_threads": workgroup size of the device-resident sampler (>= 512: the one-workgroup-per-CU form, 256: three
 *      workgroups per CU).  "sweep_split": 1 runs the diagonal bisection moves of a periodic system in the stage-machine
 *      kernel (pigs_diag.hip, three launches per MC step) instead of the one-launch kernel; it is chosen automatically
 *      for Nlev > 4.
 *   "cm_split": the TranslateChain moves of a periodic system (Np <= 256) by H cooperating workgroups per walker
 *      (pigs_cm.hip: bead ranges on H CUs, Delta S exchanged and added in bead order -- the trajectory does not depend
 *      on H, bit for bit).  -1 (default): H = min(4, CUs / walkers), at least 1 (one workgroup per walker exchanges
 *      nothing and is still the faster TranslateChain); 0: inside the sweep kernel; 1..4: at most that many.  H > 1 only
 *      while the context is the process's only one on its device; a cooperating workgroup that waits in vain (several
 *      PROCESSES crowding one chip: set 1 there) gives up after seconds and the next pigs_sync returns PIGS_ERR_HIP.
 *   "cm_exclusive": 1 = the caller vouches that the process's other contexts on this device are idle while this one
 *      samples, so H > 1 stays allowed although it is not the only live context (bench.py's extra legs).
 *   "cm_shared": 1 = several contexts of this process sample on this device AT ONCE (walker shards on one GPU): their
 *      TranslateChain kernels are chained through one event per device, never two at a time, so that H > 1 stays safe
 *      next to the other contexts' sweep kernels -- set "cm_split" so that H x walkers + the others' walkers <= CUs
 *      (two contexts of 64 walkers on 256 CUs: 3).  The shards then run staggered: one's TranslateChain on the CUs the
 *      other's bisection phase leaves idle.
 *   "cm_fault": TEST ONLY -- forces the time-out of that exchange once.
 *   "sf_scratch_mib": the MiB that the unfolded paths of one pigs_sf_accumulate launch may take (1..2048, default 256);
 *      the next pigs_sf_init reads it. */
int pigs_set_tuning(pigs_ctx *ctx, const char *key, int32_t value);
/* Device self-test: the kernels' short exact division / sqrt forms against IEEE `/` and sqrt()
 * on blocks*256*iters random operands; bad[0..3] = mismatch counts (sqrt, n/r, r/dr, n/dr). */
int pigs_selftest_fastmath(pigs_ctx *ctx, int32_t blocks, int32_t iters, uint64_t bad[4]);
/* Device self-test: the log() inside the device-resident sampler's Box-Muller transform (csrc/pigs_log_host.h: glibc's
 * algorithm and constants, the reference's `log` of random_mod.f90:213) against THIS host's libm, bit for bit, on n
 * arguments of the sampler's domain (stream uniforms, polar radii, random mantissas, the near-one branch).
 * *mismatches must come back 0 for the sampler's worldlines to be bit-identical to the reference's; *first_bad (may be
 * NULL) = one differing argument. */
int pigs_selftest_log(pigs_ctx *ctx, int64_t n, uint64_t seed, uint64_t *mismatches, double *first_bad);
/* Measurement aid: `reps` plain streaming reads of the context's resident worldlines (the bytes a full-chain Delta-S
 * stage reads) by a kernel that does nothing else; *bytes per pass, *seconds per pass (HIP events on the context's
 * stream).  bench.py quotes it next to K1's roofline as the rate this chip's memory system delivers to a reader. */
int pigs_selftest_stream_read(pigs_ctx *ctx, int32_t reps, double *bytes, double *seconds);

/* Host-side table fill: JastrowTable / PotentialTable (vpi_mod.f90:84-145) over
 * LogPsi / Potential (system_mod.f90:38-66,136-182), including dr = rmax/real(Nmax-1)
 * and the ghost cells.  Arrays hold Nmax+2 doubles. */
int pigs_build_tables(int32_t Nmax, double Rm, double rmax, double *VTable, double *LogWF,
                      double *dr_out);
/* Same with a choice of pair potential.  The reference selects its potential by editing
 * system_mod.f90 and recompiling: kind 0 = Aziz-II HFD-B(HE) (the active code,
 * system_mod.f90:136-182), 1 = Lennard-Jones V0*(1/r^6-1)/r^6 with V0 = 22.0228 (the commented
 * block system_mod.f90:70-83; BASELINE config 2), 2 = dipolar 1/r^3 (BASELINE config 5). */
#define PIGS_POT_AZIZ2 0
#define PIGS_POT_LJ 1
#define PIGS_POT_DIPOLAR 2
int pigs_build_tables_kind(int32_t kind, int32_t Nmax, double Rm, double rmax, double *VTable,
                           double *LogWF, double *dr_out);

/* ---- worldline residency (replaces the host array Path, vpi.f90:134) ------------ */
int pigs_path_upload(pigs_ctx *ctx, int32_t walker, const double *Path);
int pigs_path_download(pigs_ctx *ctx, int32_t walker, double *Path);
/* all walkers back to back: Paths(dim,Np,0:2*Nb,n_walkers) */
int pigs_path_upload_all(pigs_ctx *ctx, const double *Paths);
int pigs_path_download_all(pigs_ctx *ctx, double *Paths);

/* ---- K1: batched Delta S  (replaces the 24 `call UpdateAction` sites of vpi_mod.f90,
 * i.e. UpdateAction/UpdatePot/UpdateWf, vpi_mod.f90:2491-2841, + GreenFunction opt 0,
 * global_mod.f90:19-72) --------------------------------------------------------------
 * Item i moves bead ib[i] of particle ip[i] of walker walker[i] from xold(:,i) to
 * xnew(:,i); DeltaS[i] has exactly the semantics of UpdateAction's output.  Row ip of
 * the resident slice is never read (the reference's aliasing contract).
 * xnew/xold are (dim,n_items) column-major.  Host-pointer form: synchronous. */
int pigs_delta_action_batch(pigs_ctx *ctx, int64_t n_items,
                            const int32_t *walker, const int32_t *ip, const int32_t *ib,
                            const double *xnew, const double *xold, double *DeltaS);
/* Same with DEVICE pointers, asynchronous on the context's stream (inputs resident in HBM). */
int pigs_delta_action_batch_dev(pigs_ctx *ctx, int64_t n_items,
                                const int32_t *d_walker, const int32_t *d_ip, const int32_t *d_ib,
                                const double *d_xnew, const double *d_xold, double *d_DeltaS);
/* Latency-critical form for a host-driven sampler: the library owns PINNED, device-mapped
 * staging arrays that the host fills and the kernels read in place over PCIe (no memcpy calls);
 * DeltaS is written by the kernel straight into pinned host memory.  pigs_stage_reserve returns
 * (and, when growing, preserves the first `keep` items of) the item arrays;
 * pigs_delta_action_staged evaluates items [0,n) and returns when DeltaS[0,n) is valid. */
int pigs_stage_reserve(pigs_ctx *ctx, int64_t capacity, int64_t keep, int32_t **walker, int32_t **ip,
                       int32_t **ib, double **xnew, double **xold, double **DeltaS);
int pigs_delta_action_staged(pigs_ctx *ctx, int64_t n_items);
/* Same for commits: arrays (walker, ip, ib, x); pigs_commit_staged is asynchronous -- the arrays
 * may be rewritten only after the next synchronous call on this context has returned. */
int pigs_commit_reserve(pigs_ctx *ctx, int64_t capacity, int64_t keep, int32_t **walker, int32_t **ip,
                        int32_t **ib, double **x);
int pigs_commit_staged(pigs_ctx *ctx, int64_t n);

/* Test hook: the components UpdateAction combines (DeltaPot, DeltaF2, DeltaLogPsi), 3 per item. */
int pigs_delta_action_parts(pigs_ctx *ctx, int64_t n_items,
                            const int32_t *walker, const int32_t *ip, const int32_t *ib,
                            const double *xnew, const double *xold, double *parts);

/* A commit list is a sequence of assignments in the caller's program order: if a bead appears more than once, the last
 * value wins. */
/* ---- K5: commit (replaces `Path(k,ip,ib)=xnew(k)` on accept / OldChain restore, e.g.
 * vpi_mod.f90:370-374,948,987-995) -------------------------------------------------- */
int pigs_commit_beads(pigs_ctx *ctx, int64_t n, const int32_t *walker, const int32_t *ip,
                      const int32_t *ib, const double *x /* (dim,n) */);
/* Swap accept branch, vpi_mod.f90:2454-2464: exchange beads Nb..2Nb of particles iw, ik. */
int pigs_swap_tails(pigs_ctx *ctx, int32_t walker, int32_t iw, int32_t ik);

/* ---- K6: device-resident sampler (reference vpi.f90:297-439 with the movers TranslateChain and
 * MoveHeadBisection, MoveTailBisection, Bisection (sampling='bis') or MoveHead, MoveTail, Staging
 * (sampling='sta') of vpi_mod.f90).
 * One launch advances EVERY resident walker by one MC step with no host round trip: random
 * numbers (each walker's own MT19937 stream, identical to the reference's for its seed),
 * proposals, Delta S, Metropolis and commit all run on the GPU.  With CWorm > 0 the worm sector is
 * sampled too (OpenChain, CloseChain, TranslateHalfChain, MoveHead/TailHalfChain, StagingHalfChain,
 * Swap, OBDM histogram: vpi_mod.f90:383-476,1376-2487, sample_mod.f90:477-526); with CWorm = 0 the
 * reference's never-accepted open attempt (quirk Q11) is drawn so that the stream stays aligned. */
typedef struct pigs_sweep_params {
    int32_t Nlev, Nstag, CMFreq, Lstag;   /* namelist samp: bisection level, repetitions, CM period, Lstag */
    double  delta_cm;                     /* effective CM step (vpi.f90:93/123 scaling already applied)      */
    /* worm sector (namelist obdm); CWorm = 0 keeps every walker in the diagonal sector */
    double  CWorm, density, rbin;         /* rbin = rcut/real(Nbin) (vpi.f90:128), for the OBDM histogram     */
    int32_t swapping, Nobdm, Nbin, Npw;
    int32_t sampling, reserved;           /* diagonal movers: 0 = 'bis' (bisection), 1 = 'sta' (staging) */
} pigs_sweep_params;
/* Success means that pigs_sampler_step runs this input: PIGS_ERR_UNSUPPORTED when the sampler's LDS staging does not
 * hold the worldline, or when a periodic 'bis' input with Nlev > 4 needs the stage-machine kernel and that kernel does
 * not fit (odd Nmax, or table plus chain buffers beyond LDS).  A caller may then pick the host-driven sampler. */
int pigs_sampler_init(pigs_ctx *ctx, const pigs_sweep_params *sp);
/* seed walker's stream as the reference's sgrnd(seed) does */
int pigs_sampler_seed(pigs_ctx *ctx, int32_t walker, int32_t seed);
/* continue from a generator state in the reference's block form (mti, mt(0:623)) */
int pigs_sampler_set_rng(pigs_ctx *ctx, int32_t walker, int32_t mti, const int32_t mt[624]);
/* the walker's generator state, again in the reference's block form (what mtsavef writes) */
int pigs_sampler_get_rng(pigs_ctx *ctx, int32_t walker, int32_t *mti, int32_t mt[624]);
/* one MC step (istep is the 1-based step number: CM moves when mod(istep,CMFreq)==0); asynchronous */
int pigs_sampler_step(pigs_ctx *ctx, int32_t istep);
/* the form the sampler runs in (read only, changes nothing): out[0] threads per workgroup of the sweep kernel,
 * out[1] H = workgroups per walker of the TranslateChain kernel in the last step with CM moves (0: TranslateChain ran
 * inside the sweep kernel; -1: no such step yet), out[2] 1 if the last step ran the stage-machine kernel (pigs_diag.hip),
 * out[3] 1 if the context samples next to other contexts on its device (tuning key "cm_shared") */
int pigs_sampler_form(pigs_ctx *ctx, int32_t out[4]);
/* accepted-move counters per walker since pigs_sampler_init: acc[4*w+{0,1,2,3}] = CM, head, tail, bisection */
int pigs_sampler_counters(pigs_ctx *ctx, int64_t *acc);
/* accepted/attempted counters per walker since pigs_sampler_init, 16 per walker:
 * 0 cm 1 head 2 tail 3 bisection 4 try_open 5 acc_open 6 try_close 7 acc_close 8 cm_half 9 head_half
 * 10 tail_half 11 staging_half 12 try_swap 13 acc_swap 14 try_cm 15 try_stag */
int pigs_sampler_counters16(pigs_ctx *ctx, int64_t *cnt);
/* worm state of every walker: isopen[w], iworm[w] (1-based), xend(dim,2,w) */
int pigs_sampler_get_worm(pigs_ctx *ctx, int32_t *isopen, int32_t *iworm, double *xend);
int pigs_sampler_set_worm(pigs_ctx *ctx, const int32_t *isopen, const int32_t *iworm, const double *xend);
/* events of the LAST step, pigs_sampler_event_ints() = max(64, 4 + 2*(1+Nobdm)) ints per walker: [0] n, [1] isopen after
 * the step, then (code,arg) pairs in order: 1 open accepted (arg iworm) 2 close accepted 3 swap accepted (arg partner) */
int pigs_sampler_event_ints(pigs_ctx *ctx, int32_t *n);
int pigs_sampler_events(pigs_ctx *ctx, int32_t *events);
/* OBDM histogram nrho(0:Npw,Nbin,w) accumulated on the device since walker w's last reset; reset == NULL
 * keeps everything, otherwise walker w's histogram is zeroed after the copy where reset[w] != 0 (the
 * reference zeroes nrho only in blocks that normalise it, vpi.f90:520-532) */
int pigs_sampler_nrho(pigs_ctx *ctx, double *nrho, const int32_t *reset);
/* slice ib of every walker in the reference layout R(dim,Np,n_walkers) (for host-side g(r), S(k)) */
int pigs_slice_download(pigs_ctx *ctx, int32_t ib, double *R);

/* ---- K2/K3: estimator-side sums --------------------------------------------------- */
/* PotentialEnergy (sample_mod.f90:13-150) on one resident slice (test hook). */
int pigs_potential_energy_slice(pigs_ctx *ctx, int32_t walker, int32_t ib, int32_t want_F2,
                                double *Pot, double *F2);
/* ThermEnergy (sample_mod.f90:323-388) for walkers[0..n): E, Ec, Ep per walker.
 * walkers == NULL means walkers 0..n-1. */
int pigs_therm_energy_batch(pigs_ctx *ctx, int32_t n, const int32_t *walkers,
                            double *E, double *Ec, double *Ep);
/* ---- K4: LocalEnergy (sample_mod.f90:154-319) on slice ib (0 or 2*Nb in vpi.f90:443-444). */
int pigs_local_energy_batch(pigs_ctx *ctx, int32_t n, const int32_t *walkers, int32_t ib,
                            double *E, double *Kin, double *Pot);

/* ---- K7: structural estimators of slice ib (vpi.f90:466-469 uses ib = Nb): PairCorrelation and
 * StructureFactor (sample_mod.f90:392-473) for walkers[0..n).  gr(Nbin,n) receives this slice's
 * histogram increments (+2 per pair inside the cutoff, exact), Sk(dim,Nk,n) the per-k increments.
 * The caller accumulates and normalises as the reference does.  PBC only. */
int pigs_structure_batch(pigs_ctx *ctx, int32_t n, const int32_t *walkers, int32_t ib, int32_t Nbin,
                         double rbin, int32_t Nk, double *gr, double *Sk);
/* Every diagonal-sector estimator of one MC step (what vpi.f90:443-469 evaluates after a diagonal step) for n walkers in
 * ONE call: LocalEnergy at slices 0 and 2Nb (sample_mod.f90:154-319), ThermEnergy (sample_mod.f90:323-388), and -- when
 * gr and Sk are given (PBC runs) -- g(r) and S(k) at slice Nb (sample_mod.f90:392-473).  walkers may be NULL (0..n-1).
 * en[9*i + 0..2] = E, Kin, Pot at slice 0; [3..5] the same at slice 2Nb; [6..8] = E, Ec, Ep of ThermEnergy.
 * gr: n x Nbin, Sk: n x Nk x dim, laid out as pigs_structure_batch does.  Same results as the separate entry points
 * (the same kernels), one synchronisation instead of four. */
int pigs_diagonal_estimators(pigs_ctx *ctx, int32_t n, const int32_t *walkers, int32_t Nbin, double rbin, int32_t Nk,
                             double *en, double *gr, double *Sk);
/* The same overlapped with the sampler.  _begin snapshots the resident worldlines (a device-to-device copy ordered on the
 * context's stream: after every step queued so far, before whatever the caller queues next) and starts the estimator
 * kernels on a second stream of the context, on half of the chip; _end waits for them and returns the results in the
 * layout of pigs_diagonal_estimators (gr / Sk only if `structure` was non-zero).  Between the two the caller may queue the
 * next pigs_sampler_step: at 128 walkers per GPU the sampler leaves half of the CUs idle, where a step's estimators
 * (vpi.f90:443-469) then run for free.  Same kernels on a bit-identical copy: same results.  One pending batch per context. */
int pigs_diagonal_estimators_begin(pigs_ctx *ctx, int32_t n, const int32_t *walkers, int32_t Nbin, double rbin, int32_t Nk,
                                   int32_t structure);
int pigs_diagonal_estimators_end(pigs_ctx *ctx, double *en, double *gr, double *Sk);

/* ---- density profiles and pair distribution of a TRAPPED system (new: the reference allocates dens(Nbin,Nbin),
 * vpi.f90:198, and leaves its DensityProfile call commented out, vpi.f90:471) ---------------------------------------
 * Three histograms of the middle slice Path(:,:,Nb), 64-bit integer counts per walker, accumulated on the device:
 *   planar  Nbin^min(dim,2) bins of width b = (2h)/Nbin over [-h, h) in the first min(dim,2) coordinates, flat index
 *           j_1 + Nbin*j_2 (x fastest; for dim = 3 the column density over x_1, x_2).  t = (x_k + h)/b; the particle
 *           counts if 0 <= t < Nbin for each of those coordinates, in bin (int)t
 *   radial  Nbin bins of width br = h/Nbin over r = |x| in [0, h): u = r/br counts if u < Nbin, in bin (int)u
 *   pair    Nbin bins of width br over the pair distance d (no minimum image): +2 per pair i < j with d/br < Nbin
 *   samples +1 per accumulate.
 * Decisions are taken in double before any conversion to an integer (NaN, +-Inf, huge values drop out).  b and br are
 * computed once by pigs_density_init in double exactly as written above.  Normalisation is the caller's (per walker and
 * block, with S = the block's samples: planar c/(S b^min(dim,2)), radial c/(S dV_j), pair c/(S Np dV_j), where
 * dV_j = V_d((j+1)br) - V_d(j br) and V_d the volume of the d-ball).
 *
 * pigs_density_init allocates and zeroes the accumulators (again: resizes and zeroes).  PIGS_ERR_UNSUPPORTED on a
 * periodic context, PIGS_ERR_ARG for Nbin < 1 or !(half_width > 0). */
int pigs_density_init(pigs_ctx *ctx, int32_t Nbin, double half_width);
/* Adds slice Nb of walkers[0..n) (NULL: 0..n-1; a walker listed twice counts twice).  Queued on the context's stream,
 * no host synchronisation: it sees the worldline every call queued before it left (a pigs_diagonal_estimators_begin
 * just before it snapshots the same one), never the next step's.  PIGS_ERR_ARG before pigs_density_init or for a
 * walker out of range. */
int pigs_density_accumulate(pigs_ctx *ctx, int32_t n, const int32_t *walkers);
/* All walkers' accumulators, walker-major: planar (Nbin^min(dim,2) per walker), radial, pair (Nbin each), samples (1);
 * then zeroes those of the walkers w with reset[w] != 0 (reset == NULL: none).  Synchronises the context. */
int pigs_density_read(pigs_ctx *ctx, int64_t *planar, int64_t *radial, int64_t *pair, int64_t *samples,
                      const int32_t *reset);

/* ---- imaginary-time density correlations F(q,tau) of a PERIODIC system (new: the reference has equal-time estimators
 * only; PIGS keeps the whole path, and the worldlines are resident on the device) --------------------------------------
 *   F(q, tau_l) = < rho_q(tau0 + tau_l) rho_-q(tau0) > / Np,    tau_l = l dt  (l links of the path)
 * on the reference's S(k) grid (sample_mod.f90:435-476, vpi.f90:119): for axis k = 1..dim and iq = 1..Nk,
 *   q = real(iq) * (2 pi / Lbox(k)),  C(s) = sum_i cos(q x_k(i,s)),  S(s) = sum_i sin(q x_k(i,s))
 * with the phase q x formed as pigs_structure_batch forms it.  The slices used are the window Nb-window .. Nb+window
 * (0 <= window <= Nb), the lags l = 0 .. Ntau (0 <= Ntau <= 2 window).  Per walker and accumulate call the device adds
 *   acc[walker][l][iq][k] += sum over a = Nb-window .. Nb+window-l (ascending) of C(a) C(a+l) + S(a) S(a+l)
 * and 1 to samples[walker].  n_pairs(l) = 2 window + 1 - l terms per call, so the estimator is
 *   F(q_{k,iq}; tau_l) = acc / (samples * n_pairs(l) * Np)          (the caller's division; profiles.normalize_fqt)
 * and its l = 0 value is S(q) averaged over the window; with window = 0, Ntau = 0 the increment is exactly the
 * reference's StructureFactor term of slice Nb.  The sums are taken in fixed orders without floating-point atomics: the
 * same worldline gives the same bits whatever the walker list.  The window must stay inside the part of the path where
 * the projection has converged (PIGS expectation values are ground-state ones only that far from the ends): choosing it
 * is the caller's business, the library does not judge it.
 *
 * pigs_fqt_init allocates and zeroes the sums (again: resizes and zeroes).  PIGS_ERR_UNSUPPORTED on a trapped context,
 * PIGS_ERR_ARG for Nk < 1, window < 0, window > Nb, Ntau < 0 or Ntau > 2 window. */
int pigs_fqt_init(pigs_ctx *ctx, int32_t Nk, int32_t Ntau, int32_t window);
/* Adds the window of walkers[0..n) (NULL: 0..n-1; a walker listed twice counts twice).  Queued on the context's stream,
 * no host synchronisation: it sees the worldline every call queued before it left, never the next step's.  PIGS_ERR_ARG
 * before pigs_fqt_init or for a walker out of range. */
int pigs_fqt_accumulate(pigs_ctx *ctx, int32_t n, const int32_t *walkers);
/* All walkers' raw sums F[n_walkers][Ntau+1][Nk][dim] (k fastest) and samples[n_walkers]; then zeroes those of the
 * walkers w with reset[w] != 0 (reset == NULL: none).  Synchronises the context. */
int pigs_fqt_read(pigs_ctx *ctx, double *F, int64_t *samples, const int32_t *reset);

/* ---- vector structure factor S(q) of a PERIODIC system on the full reciprocal grid (new: the reference's S(k) and
 * pigs_fqt_* live on the axis grid q = iq 2 pi / L along the box axes only, which reaches neither the (1,1,1)-type
 * Bragg vectors of a solid nor the |q| shells between the axis harmonics) ------------------------------------------------
 * The vectors are the integer ones n = (n_1 .. n_dim) with |n_k| <= nmax of the half space: the first non-zero component
 * is positive, so n = 0 is left out and q, -q are counted once.  For each
 *   q_k = real(n_k) * (2 pi / Lbox(k)),     Nq = ((2 nmax + 1)^dim - 1) / 2  vectors.
 * ENUMERATION ORDER: ascending lexicographic order of (n_1, .., n_dim), n_1 slowest.  With S = 2 nmax + 1 vector iqv
 * (0-based) is the one whose rank sum_k (n_k + nmax) S^(dim-k) among ALL S^dim vectors is iqv + Nq + 1 (the half space
 * is exactly what follows n = 0).  3D, nmax = 1: (0,0,1), (0,1,-1), (0,1,0), (0,1,1), (1,-1,-1), ..., (1,1,1).
 * pigs_sqv_vectors hands the list out; no caller needs to restate it.  In 1D the grid is the axis grid n = 1..nmax.
 * The slices used are the window Nb-window .. Nb+window (0 <= window <= Nb), as for F(q,tau).  Per walker and
 * accumulate call the device adds
 *   acc[walker][iqv] += sum over a = Nb-window .. Nb+window (ascending) of C(a)^2 + S(a)^2
 *   C(a) = sum_i cos(q . x_i(a)),  S(a) = sum_i sin(q . x_i(a))
 * and 1 to samples[walker], so the estimator is
 *   S(q) = acc / (samples * (2 window + 1) * Np)                     (the caller's division; profiles.normalize_sqv)
 * exp(i q.x) is formed as the product of per-axis phasors exp(i real(m) (2 pi/Lbox(k)) x_k), m = |n_k|, each from one
 * sincos of the phase rounded as pigs_structure_batch rounds it.  The sums are taken in fixed orders without
 * floating-point atomics: the same worldline gives the same bits whatever the walker list, the launch split or the
 * context.  The window must stay inside the converged part of the path; the library does not judge it.
 *
 * pigs_sqv_init allocates and zeroes the sums (again: resizes and zeroes).  PIGS_ERR_UNSUPPORTED on a trapped context,
 * PIGS_ERR_ARG for nmax < 1, nmax > 16 in 3D, nmax > 64 in 1D or 2D, window < 0 or window > Nb. */
int pigs_sqv_init(pigs_ctx *ctx, int32_t nmax, int32_t window);
/* Nq, and the vectors n[Nq][dim] in the enumeration order above.  PIGS_ERR_ARG before pigs_sqv_init. */
int pigs_sqv_count(pigs_ctx *ctx, int64_t *Nq);
int pigs_sqv_vectors(pigs_ctx *ctx, int32_t *n);
/* Adds the window of walkers[0..n) (NULL: 0..n-1; a walker listed twice counts twice).  Queued on the context's stream,
 * no upload, no host synchronisation: it sees the worldline every call queued before it left, never the next step's.
 * PIGS_ERR_ARG before pigs_sqv_init or for a walker out of range. */
int pigs_sqv_accumulate(pigs_ctx *ctx, int32_t n, const int32_t *walkers);
/* All walkers' raw sums S[n_walkers][Nq] and samples[n_walkers]; then zeroes those of the walkers w with
 * reset[w] != 0 (reset == NULL: none).  Synchronises the context. */
int pigs_sqv_read(pigs_ctx *ctx, double *S, int64_t *samples, const int32_t *reset);

/* ---- imaginary-time density correlations F(q,tau) of a PERIODIC system on the full reciprocal grid (new: pigs_fqt_* has
 * the lags on the axis grid only, pigs_sqv_* the full grid at equal times only; the analytic continuation to S(q,omega)
 * wants both: every |q| shell, and 6-48 symmetry-related vectors per shell to average over) ---------------------------
 * The vectors are exactly those of pigs_sqv_*, in its enumeration order (half space, |n_k| <= nmax, ascending
 * lexicographic, n_1 slowest, Nq = ((2 nmax + 1)^dim - 1)/2); pigs_fqv_vectors hands the same list out.  The slices and
 * lags are those of pigs_fqt_*: the window Nb-window .. Nb+window (0 <= window <= Nb), the lags l = 0 .. Ntau
 * (0 <= Ntau <= 2 window).  Per listed walker and accumulate call the device adds
 *   acc[walker][l][iqv] += sum over a = Nb-window .. Nb+window-l (ascending) of C(a) C(a+l) + S(a) S(a+l)
 *   C(a) + i S(a) = sum_i exp(i q . x_i(a))
 * and 1 to samples[walker].  C and S are formed exactly as pigs_sqv_* forms them (per-axis phasors from one sincos of
 * the phase rounded as pigs_structure_batch rounds it, prefix product, fused multiply-adds over the particles in
 * ascending order: one piece of device code serves both).  The two products and their sum are not fused; the sum over a
 * runs left to right from 0.0 and is then added to the accumulator.  So lag 0 is bit-identical to what
 * pigs_sqv_accumulate adds for the same nmax, window and worldline.  The estimator is
 *   F(q; tau_l) = acc / (samples * (2 window + 1 - l) * Np)          (the caller's division; profiles.normalize_fqv)
 * No floating-point atomics, every sum in one fixed order: the same worldline gives the same bits whatever the walker
 * list, the launch split or the context.  The window must stay inside the converged part of the path; the library does
 * not judge it.
 *
 * pigs_fqv_init allocates and zeroes the sums (again: resizes and zeroes).  PIGS_ERR_UNSUPPORTED on a trapped context;
 * PIGS_ERR_ARG for nmax < 1, nmax > 16 in 3D, nmax > 64 in 1D or 2D, window < 0, window > Nb, Ntau < 0, Ntau > 2 window,
 * accumulators larger than 2 GiB in total, or a window of more than 4096 slices (one vector's slices must fit the
 * 64 KiB of LDS the lag kernel stages them in). */
int pigs_fqv_init(pigs_ctx *ctx, int32_t nmax, int32_t Ntau, int32_t window);
/* Nq, and the vectors n[Nq][dim] in the enumeration order of pigs_sqv_vectors.  PIGS_ERR_ARG before pigs_fqv_init. */
int pigs_fqv_count(pigs_ctx *ctx, int64_t *Nq);
int pigs_fqv_vectors(pigs_ctx *ctx, int32_t *n);
/* Adds the window of walkers[0..n) (NULL: 0..n-1; a walker listed twice counts twice).  Queued on the context's stream,
 * no upload, no host synchronisation: it sees the worldline every call queued before it left, never the next step's.
 * The list travels in the kernel arguments, at most 256 walkers per launch (fewer where the (C, S) scratch of a launch,
 * 16 (2 window + 1) Nq bytes per walker, would pass 256 MiB) and more in further launches.  PIGS_ERR_ARG before
 * pigs_fqv_init or for a walker out of range. */
int pigs_fqv_accumulate(pigs_ctx *ctx, int32_t n, const int32_t *walkers);
/* All walkers' raw sums F[n_walkers][Ntau+1][Nq] (iqv fastest) and samples[n_walkers]; then zeroes those of the walkers
 * w with reset[w] != 0 (reset == NULL: none).  Synchronises the context.  PIGS_ERR_ARG before pigs_fqv_init. */
int pigs_fqv_read(pigs_ctx *ctx, double *F, int64_t *samples, const int32_t *reset);

/* ---- self (incoherent) part of F(q,tau) and the imaginary-time displacement of a PERIODIC system (new: pigs_fqt_* and
 * pigs_fqv_* give the coherent <rho_q(tau) rho_-q(0)>; this follows ONE particle along its worldline, which needs particle
 * labels that are continuous in imaginary time: the resident paths have them, pigs_swap_tails keeps them) ---------------
 * The vectors, the window and the lags are exactly those of pigs_fqv_*: the half-space integer vectors |n_k| <= nmax in
 * the enumeration order of pigs_sqv_vectors (pigs_fqs_vectors hands the same list out), the slices Nb-window .. Nb+window
 * (0 <= window <= Nb), the lags l = 0 .. Ntau (0 <= Ntau <= 2 window).  Per listed walker w and accumulate call the device
 * adds, with n_pairs(l) = 2 window + 1 - l slice pairs (a, a+l), a = Nb-window .. Nb+window-l,
 *   F[w][l][iqv] += sum over the particles i and the pairs a of c_i(a) c_i(a+l) + s_i(a) s_i(a+l)
 *   c_i(a) + i s_i(a) = exp(i q . x_i(a))
 *   D[w][l][0]   += sum over i and a of r2
 *   D[w][l][1]   += sum over i and a of r2 * r2
 * and 1 to samples[w].
 * - Phasors.  exp(i q.x) is the product of per-axis phasors exp(i real(m) (2 pi/Lbox(k)) x_k), m = |n_k| (conjugated for
 *   n_k < 0), each from one sincos of the phase (double)(float)m * (2 pi/Lbox[k]) * x_k as pigs_sqv_* rounds it; the axes
 *   are multiplied in its order, (e_1 e_2) e_3, each complex product as (ar br - ai bi, ar bi + ai br), nothing fused.  A
 *   reciprocal vector of the box does not notice a wrap of x, so F needs no unfolded path.
 * - Displacement.  d_k = x_k(i, a+l) - x_k(i, a), folded ONCE as pbc_mod.f90:40-41 does (the two compares, each against
 *   LboxHalf); r2 is the sum of the squares, left to right, nothing fused.  Lag 0 adds exactly 0.0.  THIS IS THE
 *   DISPLACEMENT ONLY WHILE |d_k| STAYS BELOW Lbox[k]/2, which holds for the imaginary-time spans in use (a particle
 *   diffuses ~ sqrt(2 lambda tau) << L/2 there); the library does not judge it.
 * - Summation order of F.  One running sum per element (w, l, iqv) and call starts at 0.0 and takes the terms
 *   t = c c' + s s' (two products and their sum, not fused) as sum = sum + t with the particles i ascending and, per
 *   particle, a ascending; the call's sum is then added to the accumulator.
 * - Summation order of D.  With B = min(256, Np rounded up to a multiple of 64) lanes, lane j takes the particles j,
 *   j + B, .. in ascending order and, per particle, a ascending: s1 = s1 + r2, s2 = s2 + r2 * r2.  The 64 lanes of a wave
 *   are added by a butterfly (partner lane ^ 32, 16, .., 1), the waves in wave order from 0.0, then acc += value.
 * No floating-point atomics: the same worldline gives the same bits whatever the walker list, its order, the launch
 * split or the number of walkers of the context.  The estimators are the caller's divisions
 *   F_s(q; tau_l)      = F / (samples * n_pairs(l) * Np)                          (profiles.normalize_fqs)
 *   <dr^2>(tau_l)      = D[..][0] / (samples * n_pairs(l) * Np)                   (profiles.normalize_msd)
 *   alpha_2(tau_l)     = dim <dr^4> / ((dim + 2) <dr^2>^2) - 1,  <dr^4> from D[..][1]   (the non-Gaussian parameter)
 * F_s(q; 0) = 1 and <dr^2>(0) = 0.  The window must stay inside the converged part of the path; the library does not
 * judge it.
 *
 * pigs_fqs_init allocates and zeroes the sums (again: resizes and zeroes).  PIGS_ERR_UNSUPPORTED on a trapped context;
 * PIGS_ERR_ARG for nmax < 1, nmax > 16 in 3D, nmax > 64 in 1D or 2D, window < 0, window > Nb, Ntau < 0, Ntau > 2 window,
 * accumulators larger than 2 GiB in total, more than 3072 lags, or a window whose phasors do not fit the kernel's 64 KiB
 * of LDS: 16 (2 window + 1) (dim (nmax + 1) + 1) bytes at the least. */
int pigs_fqs_init(pigs_ctx *ctx, int32_t nmax, int32_t Ntau, int32_t window);
/* Nq, and the vectors n[Nq][dim] in the enumeration order of pigs_sqv_vectors.  PIGS_ERR_ARG before pigs_fqs_init. */
int pigs_fqs_count(pigs_ctx *ctx, int64_t *Nq);
int pigs_fqs_vectors(pigs_ctx *ctx, int32_t *n);
/* Adds the window of walkers[0..n) (NULL: 0..n-1; a walker listed twice counts twice).  Queued on the context's stream,
 * no upload, no host synchronisation: it sees the worldline every call queued before it left, never the next step's.
 * The list travels in the kernel arguments, at most 256 walkers per launch and more in further launches; there is no
 * scratch.  PIGS_ERR_ARG before pigs_fqs_init, for n < 0 or for a walker out of range. */
int pigs_fqs_accumulate(pigs_ctx *ctx, int32_t n, const int32_t *walkers);
/* All walkers' raw sums F[n_walkers][Ntau+1][Nq] (iqv fastest), D[n_walkers][Ntau+1][2] and samples[n_walkers]; then
 * zeroes those of the walkers w with reset[w] != 0 (reset == NULL: none).  Synchronises the context.  PIGS_ERR_ARG before
 * pigs_fqs_init. */
int pigs_fqs_read(pigs_ctx *ctx, double *F, double *D, int64_t *samples, const int32_t *reset);

/* ---- pair distribution of a PERIODIC system on the vector grid, over a slice window (new: the only g(r) of a periodic
 * system was pigs_structure_batch's radial histogram of one slice; this is the real-space partner of pigs_sqv_*) --------
 * Two integer histograms per walker, accumulated on the device: g(r) on the Cartesian grid of the minimum-image cell and
 * the radial one with the reference's PairCorrelation rule.
 * For every listed walker, every slice a = Nb-window..Nb+window, and every pair i < j (0-based particle index):
 * - Displacement.  Take d_k = x_k(i) - x_k(j).  Fold it once as pbc_mod.f90:40-41 does (min_image<DIM>: the two compares,
 *   each against LboxHalf).  Let r2 be the sum of the squares, left to right, with no fused multiply-adds.
 * - Vector histogram.
 *   - The bin width is b_k = Lbox[k] / (double)Nbin.
 *   - The bin coordinate is t_k = (d_k + LboxHalf[k]) / b_k.
 *   - The pair counts +1 in the bin with flat index j_1 + Nbin*j_2 + Nbin^2*j_3 (x fastest, as `planar` of
 *     pigs_density_*), where j_k = (int)t_k.
 *   - It counts if and only if 0 <= t_k < Nbin holds in double for every k.  Otherwise it is dropped.
 *   - The decision is taken before any conversion to an integer.  NaN, +-Inf, and a difference that one fold leaves
 *     outside the cell are dropped without undefined behaviour.
 *   - Only the ordered pair i < j is counted.  The partner -d is the host's business (profiles.normalize_grv
 *     symmetrises by index reflection).
 * - Radial histogram.  If r2 <= rcut2, take u = sqrt(r2)/rbin.  If u < Nr, the pair counts +1 in bin (int)u.  This is
 *   pigs_structure_batch's rule, so 2*radial equals its `gr` summed over the window slices.
 * - Samples.  samples[w] counts calls, not slices, as pigs_sqv_* does.
 * Accumulators: 64-bit integers per walker; vec is [n_walkers][Nbin^dim], radial is [n_walkers][Nr], samples is
 * [n_walkers].  The estimators are
 *   g(r_vec) = (vec[j] + vec[reflected j]) / (samples (2 window + 1) Np density prod_k b_k)    (1 - 1/Np for an ideal gas)
 *   g(r)     = 2 radial / (samples (2 window + 1) Np density shell volume)                      (the reference's NormAvGr)
 * Counts are integer atomics (LDS u32, flushed before they could wrap, and global u64): the result depends on neither
 * the walker list, the launch split nor the context.  The vector grid is privatised in LDS where it fits and the
 * automatic choice takes it (tuning key "grv_form": -1 automatic, 0 global atomics, 1 LDS; a forced LDS form whose grid
 * does not fit returns PIGS_ERR_ARG at the next accumulate).
 *
 * pigs_grv_init allocates and zeroes the counts (again: resizes and zeroes).  PIGS_ERR_UNSUPPORTED on a trapped context;
 * PIGS_ERR_ARG for Nbin < 1, Nbin > 4096 in 1D, > 1024 in 2D, > 128 in 3D, Nr < 1, !(rbin > 0) or rbin not finite,
 * window < 0 or window > Nb, or accumulators larger than 2 GiB in total. */
int pigs_grv_init(pigs_ctx *ctx, int32_t Nbin, int32_t Nr, double rbin, int32_t window);
/* Adds the window of walkers[0..n) (NULL: 0..n-1; a walker listed twice counts twice).  Queued on the context's stream,
 * no upload, no host synchronisation: it sees the worldline every call queued before it left, never the next step's.
 * The list travels in the kernel arguments, at most 256 walkers per launch and more in further launches.
 * PIGS_ERR_ARG before pigs_grv_init or for a walker out of range. */
int pigs_grv_accumulate(pigs_ctx *ctx, int32_t n, const int32_t *walkers);
/* All walkers' counts vec[n_walkers][Nbin^dim], radial[n_walkers][Nr] and samples[n_walkers]; then zeroes those of the
 * walkers w with reset[w] != 0 (reset == NULL: none).  Synchronises the context.  PIGS_ERR_ARG before pigs_grv_init. */
int pigs_grv_read(pigs_ctx *ctx, int64_t *vec, int64_t *radial, int64_t *samples, const int32_t *reset);

/* ---- the van Hove functions G_s(r,tau) and G_d(r,tau) of a PERIODIC system, over a slice window (new: nothing in real
 * space had a lag; these are to pigs_grv_* what pigs_fqs_* and pigs_fqv_* are to pigs_sqv_*) ------------------------------
 * Two integer histograms per walker and lag, accumulated on the device.  Scope: periodic contexts with dim = 1, 2 or 3.
 * - Window, lags and slice pairs.  The window and lags are those of pigs_fqv_*: slices Nb-window .. Nb+window
 *   (0 <= window <= Nb) and lags l = 0 .. Ntau (0 <= Ntau <= 2 window).  For every listed walker w and every lag l there
 *   are n_pairs(l) = 2 window + 1 - l slice pairs (a, a+l), with a = Nb-window .. Nb+window-l.
 * - Displacements.  Take d_k = x_k(i, a+l) - x_k(j, a).  Fold it once as pbc_mod.f90:40-41 does (min_image<DIM>: the two
 *   compares against LboxHalf).  Let r2 be the sum of the squares, left to right, with nothing fused.  This is exactly
 *   pigs_grv_*'s arithmetic.
 * - Distinct part (all ordered pairs i != j).  If r2 <= rcut2, take u = sqrt(r2)/rbin.  If u < Nr holds in double, add +1
 *   to dist[w][l][(int)u].  This is pigs_grv_*'s radial rule, so at l = 0 dist equals 2 x pigs_grv_read's `radial` for
 *   the same Nr, rbin, window and worldline, bin for bin.
 * - Self part (j = i).  Take u = sqrt(r2)/sbin.  If u < Ns holds in double, add +1 to self[w][l][(int)u].  No rcut
 *   condition applies.  The self part has its own grid (Ns, sbin): an imaginary-time displacement is a few tenths of
 *   sigma, while the distinct part lives on 0..rcut, so one grid cannot serve both.  At lag 0 every particle lands in
 *   bin 0.  As for pigs_fqs_*, this is the true displacement only while |d_k| stays below Lbox[k]/2 (particle labels are
 *   continuous in imaginary time: pigs_swap_tails keeps them so).  The library does not judge that.
 * - Decisions.  Every decision is taken in double before any conversion to an integer.  NaN, +-Inf and a difference that
 *   one fold leaves far outside drop out without undefined behaviour.
 * - Samples.  samples[w] counts calls, as every other family does.
 * Accumulators: 64-bit integers per walker; self is [n_walkers][Ntau+1][Ns], dist is [n_walkers][Ntau+1][Nr], samples is
 * [n_walkers].  The estimators are the caller's divisions (tau_l = l dt):
 *   G_d(r_b; tau_l) = dist / (samples n_pairs(l) Np density dV_b)    dV_b the shell volume of the reference's NormAvGr,
 *                                                                    as in grw_vpi.out; 1 - 1/Np for an ideal gas
 *   G_s(r_b; tau_l) = self / (samples n_pairs(l) Np dV_b)            on the self grid: a probability density whose
 *                                                                    integral over space is 1 when nothing was dropped
 * Counts are integer atomics only (LDS u32 flushed into global u64, or global u64): the result depends on neither the
 * walker list, its order, the launch split at 256 walkers, the kernel form nor the context.
 * Kernel forms and limits.  One workgroup holds the base slice a in LDS, 8 dim Np bytes, and pigs_vh_init refuses
 * (PIGS_ERR_ARG) a system with
 *   8 dim Np > 163840                                  (the 160 KiB of a CU: Np <= 6826 in 3D, 10240 in 2D, 20480 in 1D).
 * The histograms of all lags are privatised in LDS as u32 counters beside the slice where
 *   8 dim Np + 4 (Ntau + 1) (Nr + Ns) <= 163840,
 * and take global u64 atomics otherwise (tuning key "vh_form": -1 automatic, 0 global atomics, 1 LDS; a forced LDS form
 * that does not fit returns PIGS_ERR_ARG at the next accumulate and queues nothing).  A u32 counter belongs to one lag of
 * one base slice and gains at most one count per (i, j), Np^2 in all, before the workgroup's single flush; Np^2 stays
 * below 2^32 up to Np = 65535, which the slice limit above never lets through: no u32 counter can wrap.
 *
 * pigs_vh_init allocates and zeroes the counts (again: resizes and zeroes).  PIGS_ERR_UNSUPPORTED on a trapped context;
 * PIGS_ERR_ARG for Nr < 1 or Ns < 1, rbin or sbin not finite and positive, window < 0 or window > Nb, Ntau < 0 or
 * Ntau > 2 window, accumulators larger than 2 GiB in total, or the slice limit above. */
int pigs_vh_init(pigs_ctx *ctx, int32_t Ntau, int32_t window, int32_t Nr, double rbin, int32_t Ns, double sbin);
/* Adds the window of walkers[0..n) (NULL: 0..n-1; a walker listed twice counts twice).  Queued on the context's stream,
 * no upload, no host synchronisation: it sees the worldline every call queued before it left, never the next step's.
 * The list travels in the kernel arguments, at most 256 walkers per launch and more in further launches.
 * PIGS_ERR_ARG before pigs_vh_init, for n < 0 or for a walker out of range. */
int pigs_vh_accumulate(pigs_ctx *ctx, int32_t n, const int32_t *walkers);
/* All walkers' counts self[n_walkers][Ntau+1][Ns], dist[n_walkers][Ntau+1][Nr] and samples[n_walkers]; then zeroes those of
 * the walkers w with reset[w] != 0 (reset == NULL: none).  Synchronises the context.  PIGS_ERR_ARG before pigs_vh_init. */
int pigs_vh_read(pigs_ctx *ctx, int64_t *self, int64_t *dist, int64_t *samples, const int32_t *reset);

/* ---- the triplet distribution g3(r, s, cos theta) of a PERIODIC system in 2D or 3D, over a slice window (new: every
 * family above comes from pair visits; this is the first three-body correlation: the Kirkwood superposition test, and in
 * its first-shell section the bond-angle distribution P(cos theta)) ------------------------------------------------------
 * Scope: periodic contexts with dim = 2 or 3.
 * Parameters: Nr, rbin: the radial grid, the radius is rmax = Nr rbin.  Na: the number of bins of cos theta on [-1, 1].
 * window: slices a = Nb-window .. Nb+window.
 * For every listed walker w, every window slice a and every vertex i:
 * - Legs.  For each j != i take d_k(j) = x_k(i,a) - x_k(j,a), folded once by min_image<DIM> (the two compares against
 *   LboxHalf).  r2(j) is the sum of the squares, left to right, with nothing fused.  s(j) = sqrt(r2(j)) and
 *   u(j) = s(j)/rbin.  j is a leg of i iff 0 < r2(j) and u(j) < Nr both hold in double.  So a coincident partner, a partner
 *   at exactly rmax, and a NaN or +-Inf are not legs.  Its radial bin is b(j) = (int)u(j).  Every leg adds +1 to
 *   pair[w][b(j)].  These are ordered pairs, so each pair is counted from both ends.
 * - Triplets.  For every unordered pair {j,k} of legs of i take dot = d_1(j) d_1(k) + ... + d_DIM(j) d_DIM(k), products
 *   summed left to right and unfused.  Take c = dot / (s(j) s(k)) and v = (c + 1.0) (0.5 Na).  If v is NaN the triplet is
 *   dropped.  Otherwise the angle bin is q = v < 0 ? 0 : min((int)v, Na-1) (v >= Na, +Inf included, gives Na-1 without a
 *   conversion).  This clamps c rounded past +-1 and keeps collinear triplets.  With lo = min(b(j),b(k)) and
 *   hi = max(b(j),b(k)), add +1 to trip[w][p][q], where p = lo Nr - lo(lo-1)/2 + (hi - lo) indexes the packed upper
 *   triangle of Nr(Nr+1)/2 leg pairs.  Every operation commutes in (j,k), so the count does not depend on the order in
 *   which a pair of legs is met.
 * - Samples.  samples[w] gains 1 per call and listed walker.
 * Accumulators: 64-bit integers per walker; trip is [n_walkers][Nr(Nr+1)/2][Na], pair is [n_walkers][Nr], samples is
 * [n_walkers].  Integer atomics only: the result depends on neither the walker list, its order, the split at 256 walkers
 * per launch, the kernel form nor the context.
 * Normalisation, on the host (profiles.normalize_g3, pigs_estimators.f90).  S = samples (2 window + 1); vol(b) is the
 * d-ball shell volume of bin b, as normalize_grv uses it:
 *   g2(b)       = pair[b] / (S Np density vol(b))
 *   g3(lo,hi,q) = trip / (S Np density^2 vol(lo) vol(hi) w(q) m),   m = 1 for lo < hi and 1/2 for lo = hi,
 *   w(q) = 1/Na in 3D;  w(q) = (acos(c_q) - acos(c_{q+1}))/pi in 2D, with c_q = -1 + 2q/Na.
 * An uncorrelated system gives 1 up to O(1/Np).
 * Kernel forms and limits.  One workgroup of 4 waves holds a slice in LDS, 8 dim Np bytes, and each wave a list of the
 * legs of its vertex with room for all Np - 1 partners, 8 (dim + 1) + 4 bytes each: a list cannot overflow whatever the
 * configuration.  pigs_g3_init refuses (PIGS_ERR_ARG) a system with
 *   8 dim Np + 4 Np (8 (dim + 1) + 4) > 163840            (the 160 KiB of a CU: Np <= 975 in 3D, 1280 in 2D),
 * so every Np <= 512 is served with rmax up to half the box.  The counters are privatised in LDS as u32 beside them where
 *   8 dim Np + 4 Np (8 (dim + 1) + 4) + 4 (Nr(Nr+1)/2 Na + Nr) <= 163840   and   Np (Np-1)(Np-2)/2 <= 2^32 - 1,
 * and take global u64 atomics otherwise (tuning key "g3_form": -1 automatic, 0 global atomics, 1 LDS; a forced LDS form
 * that does not fit returns PIGS_ERR_ARG at the next accumulate and queues nothing).  A u32 counter belongs to one slice of
 * one walker and gains at most one count per triplet of that slice before the workgroup's single flush; a slice has at most
 * Np (Np-1)(Np-2)/2 triplets (and Np (Np-1) ordered pairs, which is less from Np = 4 on), so under the second condition no
 * u32 counter can wrap.  (The LDS limit above keeps Np far below the 2050 where it would first fail.)
 *
 * pigs_g3_init allocates and zeroes the counts (again: resizes and zeroes).  PIGS_ERR_UNSUPPORTED on a trapped context
 * or dim = 1; PIGS_ERR_ARG for Nr < 1 or Na < 1, Nr or Na > 1024, rbin not finite and positive, rmax beyond half the
 * shortest side (as pigs_bop_init treats rnb; Nr rbin may pass it by 4 ulps, so that rbin = half / Nr is always taken), window < 0 or window > Nb, accumulators larger than 2 GiB in total, or the
 * size limit above. */
int pigs_g3_init(pigs_ctx *ctx, int32_t Nr, double rbin, int32_t Na, int32_t window);
/* Adds the window of walkers[0..n) (NULL: 0..n-1; a walker listed twice counts twice).  Queued on the context's stream,
 * no upload, no host synchronisation: it sees the worldline every call queued before it left, never the next step's.
 * The list travels in the kernel arguments, at most 256 walkers per launch and more in further launches.
 * PIGS_ERR_ARG before pigs_g3_init, for n < 0 or for a walker out of range. */
int pigs_g3_accumulate(pigs_ctx *ctx, int32_t n, const int32_t *walkers);
/* All walkers' counts trip[n_walkers][Nr(Nr+1)/2][Na], pair[n_walkers][Nr] and samples[n_walkers]; then zeroes those of
 * the walkers w with reset[w] != 0 (reset == NULL: none).  Synchronises the context.  PIGS_ERR_ARG before pigs_g3_init. */
int pigs_g3_read(pigs_ctx *ctx, int64_t *trip, int64_t *pair, int64_t *samples, const int32_t *reset);

/* ---- the Axilrod-Teller-Muto (triple-dipole) three-body energy <V3> of a PERIODIC system in 2D or 3D, over a slice window
 * (new: the first three-body ENERGY; evaluated perturbatively on the configurations that the pair potential sampled) -------
 * Scope: periodic contexts with dim = 2 or 3.
 * Parameters: rc, the cutoff of every side of a triplet; window: slices a = Nb-window .. Nb+window.
 * For a listed walker w and every window slice a = Nb-window .. Nb+window:
 * 1. For each pair of particles, take the coordinate difference, fold it once by min_image<DIM>, and sum r^2 left to right.
 *    This is pigs_grv_*'s arithmetic.
 * 2. For every triplet i < j < k, let a2 = r^2(i,j), b2 = r^2(i,k), c2 = r^2(j,k).  Each pair is at its own nearest image.
 * 3. The triplet counts if and only if  a2 <= rc2 && b2 <= rc2 && c2 <= rc2,  compared in double.  NaN compares false and
 *    drops the triplet.  The host computes rc2 = rc*rc.
 * 4. The triplet's term, with -ffp-contract=off, is exactly these operations in this order:
 *      p   = (a2 * b2) * c2
 *      s   = sqrt(p)
 *      num = ((a2 + b2 - c2) * (a2 + c2 - b2)) * (b2 + c2 - a2)
 *      t   = (p + 0.375 * num) / ((p * p) * s)
 *    This equals (1 + 3 cos(gamma_i) cos(gamma_j) cos(gamma_k)) / (r_ij r_ik r_jk)^3.
 * The term is a function of the three side lengths only.  It is therefore defined when the three nearest images do not
 * close into a triangle, which can happen once rc > L/4 (three particles on a line at 0, 0.4 L and 0.8 L have the sides
 * 0.4 L, 0.2 L and 0.4 L: the term is the isosceles triangle's, not a collinear one's).
 * One accumulate call adds per (w, a):
 *   T[w][a]     += sum of t, as a double
 *   ntrip[w][a] += the number of counted triplets, as int64
 *   samples[w]  += 1
 * The coupling nu never reaches the device.  The estimators are the caller's divisions (profiles.normalize_atm,
 * pigs_estimators.f90):
 *   V3/N(tau_a) = nu T / (samples Np);   V3/N averages that over the window.
 *   Pressure contribution P3 = 9 nu <T> / (dim Volume): the sum is homogeneous of degree -9.  It is cut at rc and has no
 *   tail correction, which is the same policy as the pair virial.
 * A coincident pair (p = 0) gives a non-finite term.  That term stays in its own (w, a) element, as in pigs_tau_*.
 * Summation.  No floating-point atomics and one fixed order: per lane, then across the wave, then across the waves in wave
 * order, then acc += value by the one thread that owns (w, a) in the launch.  The same worldline gives the same bits
 * whatever the walker list, its order, the launch split or the number of walkers in the context; a walker listed twice
 * counts twice (in two launches), with bits equal to 2 x one count.  An element of one term (Np = 3) has that term's bits.
 * Limit.  One workgroup of 4 waves holds a slice in LDS, 8 dim Np bytes, and each wave a list of the legs of its vertex
 * with room for all Np - 1 partners, 8 (dim + 1) bytes each (the partner's coordinates and a2): a list cannot overflow
 * whatever the configuration.  pigs_atm_init refuses (PIGS_ERR_ARG) a system with
 *   8 dim Np + 4 Np 8 (dim + 1) + 64 > 163840             (the 160 KiB of a CU: Np <= 1077 in 3D, 1462 in 2D),
 * which serves every system that pigs_g3_init serves.
 *
 * pigs_atm_init allocates and zeroes the sums (again: resizes and zeroes).  PIGS_ERR_UNSUPPORTED on a trapped context or
 * dim = 1; PIGS_ERR_ARG unless rc is finite with 0 < rc <= half the shortest side and 0 <= window <= Nb, and for the size
 * limit above. */
int pigs_atm_init(pigs_ctx *ctx, double rc, int32_t window);
/* Adds the window of walkers[0..n) (NULL: 0..n-1; a walker listed twice counts twice).  Queued on the context's stream,
 * no upload, no host synchronisation: it sees the worldline every call queued before it left, never the next step's.
 * The list travels in the kernel arguments, at most 256 walkers per launch and more in further launches.
 * PIGS_ERR_ARG before pigs_atm_init, for n < 0 or for a walker out of range. */
int pigs_atm_accumulate(pigs_ctx *ctx, int32_t n, const int32_t *walkers);
/* All walkers' sums T[n_walkers][2 window + 1], counts ntrip[n_walkers][2 window + 1] and samples[n_walkers]; then zeroes
 * those of the walkers w with reset[w] != 0 (reset == NULL: none).  Synchronises the context.  PIGS_ERR_ARG before
 * pigs_atm_init. */
int pigs_atm_read(pigs_ctx *ctx, double *T, int64_t *ntrip, int64_t *samples, const int32_t *reset);

/* ---- the momentum distribution n(k) and the one-body density matrix rho1(r) of a PERIODIC system (new: the first
 * off-diagonal estimator beyond the reference's radial histogram nrho, which is cut at rcut, binned and angle-averaged) ------
 * Scope: periodic contexts.  A SAMPLE is the end-to-end vector of an open worldline, x_k = head_k - tail_k, folded once:
 *   if (x_k >  LboxHalf(k)) x_k = x_k - Lbox(k);   if (x_k < -LboxHalf(k)) x_k = x_k + Lbox(k)
 * which is what the sampler's OBDM histogram takes (sample_mod.f90:477-526).
 * Vectors: exactly those of pigs_sqv_*, in its enumeration order (half space, |n_k| <= nmax, n = 0 left out);
 * pigs_nk_count and pigs_nk_vectors hand them out.  For k = 2 pi (n_1/Lbox(1), ..) the phase k.x does not depend on the
 * periodic image, so every sample counts, those beyond rcut too.  Per sample of a listed walker w the device adds
 *   C[w][iq]   += cos(k_iq . x)                as a double, the samples in tape order, one add to C per launch
 *   H[w][flat] += 1   flat = j_1 + nbin j_2 + nbin^2 j_3, j_k = (int)t_k, t_k = (x_k + LboxHalf(k)) / (Lbox(k)/nbin), iff
 *                     0 <= t_k < nbin holds in double for every k: the cell and bin-edge rule of pigs_grv_*
 *   nopen[w]   += 1   (this is the sum of the vector n = 0: C(0) = nopen exactly)
 *   ninside[w] += 1   iff r2 <= rcut2 in double, r2 = sum_k x_k^2 left to right: the histogram's own comparison
 * cos(k.x) is the real part of the product of per-axis phasors exp(i real(m) (2 pi/Lbox(k)) x_k), m = |n_k|, each from one
 * sincos of the phase rounded as pigs_sqv_* rounds it (m = 0 gives exactly 1), multiplied in the order k = 1..dim.
 * No floating-point atomics and one fixed order: the same samples give the same bits, and a walker listed twice counts
 * twice (in two launches) with bits equal to 2 x one count.
 * The estimators are the caller's divisions (profiles.normalize_nk, normalize_nrvec; pigs_estimators.f90), in the
 * reference's NormalizeNr convention with zconf the number of diagonal configurations of the block:
 *   n(k) = C / (CWorm zconf Nobdm),   n(0) = nopen / (CWorm zconf Nobdm),   n0 = n(0)/Np,   sum over all k of n(k) = Np
 *   rho1(bin)/density = H / (CWorm zconf Nobdm density cell volume/nbin^dim)
 * Samples are staged in tiles of PIGS_NK_TILE in LDS, 16 dim PIGS_NK_TILE (nmax + 1) bytes.  A walker with at most one tile
 * of samples (every Nobdm <= PIGS_NK_TILE on the tape path) has its table built once.  With more, the tables of all its
 * tiles are built again for every 256 vectors (Nq/256 times: 70 at nmax = 16 in 3D): correct, but pigs_nk_add is then
 * cheaper in calls of at most PIGS_NK_TILE pairs per walker.
 *
 * pigs_nk_init allocates and zeroes the sums (again: resizes and zeroes).  PIGS_ERR_UNSUPPORTED on a trapped context
 * (there rho1 is not translation-invariant, and the reference takes no OBDM either); PIGS_ERR_ARG for nmax < 1, nmax > 16
 * in 3D, nmax > 64 in 1D or 2D (pigs_sqv_init's limits), nbin < 1, nbin > 128 in 3D, 1024 in 2D, 4096 in 1D, or sums
 * beyond 2 GiB (pigs_grv_init's limits). */
#define PIGS_NK_TILE 64
int pigs_nk_init(pigs_ctx *ctx, int32_t nmax, int32_t nbin);
/* Nq, and the vectors n[Nq][dim] in the enumeration order of pigs_sqv_vectors.  PIGS_ERR_ARG before pigs_nk_init. */
int pigs_nk_count(pigs_ctx *ctx, int64_t *Nq);
int pigs_nk_vectors(pigs_ctx *ctx, int32_t *n);
/* Adds, for walkers[0..n) (NULL: 0..n-1; a walker listed twice counts twice), the samples of the LAST pigs_sampler_step:
 * the Nobdm end-to-end vectors that its worm loop handed to the OBDM histogram if the walker went through that loop
 * (it was open after the open / close attempt), none otherwise.  Queued on the context's stream, no upload, no host
 * synchronisation.  It must be queued before the next pigs_sampler_step, which overwrites the tape.  A second call after
 * the same step counts that step's samples again.  Before the first step it adds nothing.
 * PIGS_ERR_ARG before pigs_nk_init, unless pigs_sampler_init was called with CWorm > 0, for n < 0 or for a walker out of
 * range. */
int pigs_nk_accumulate(pigs_ctx *ctx, int32_t n, const int32_t *walkers);
/* The same sums from the host (the host-driven sampler, tests; needs no sampler): listed walker i brings nsamp[i] >= 0
 * pairs, xend(dim, 2, sum nsamp) in Fortran order: head (dim doubles) then tail of every pair, the pairs of walker 0 first.
 * Folds head - tail once as above and runs the kernel of pigs_nk_accumulate.  Uploads and waits for the upload.
 * PIGS_ERR_ARG before pigs_nk_init, for n < 0, a negative nsamp or a walker out of range. */
int pigs_nk_add(pigs_ctx *ctx, int32_t n, const int32_t *walkers, const int32_t *nsamp, const double *xend);
/* All walkers' C[n_walkers][Nq], H[n_walkers][nbin^dim] (x fastest), nopen[n_walkers] and ninside[n_walkers]; then zeroes
 * those of the walkers w with reset[w] != 0 (reset == NULL: none).  Synchronises the context.  PIGS_ERR_ARG before
 * pigs_nk_init. */
int pigs_nk_read(pigs_ctx *ctx, double *C, int64_t *H, int64_t *nopen, int64_t *ninside, const int32_t *reset);

/* ---- a crystal seen from its lattice: Lindemann moments, site occupancy and site hops of a PERIODIC system in 2D or 3D,
 * over a slice window (new: every family above is translation-invariant; this is the first that takes the lattice the
 * run was started from as input) -----------------------------------------------------------------------------------------
 * Scope: periodic contexts with dim = 2 or 3.
 * Sites: R(dim, nsite), column-major like Path (site s at sites[s*dim .. s*dim + dim)), uploaded once by pigs_lat_init into
 * rows laid out as a slice's.  nsite need not equal Np: nsite = Np + 1 is a vacancy run, nsite = Np - 1 forces a double
 * occupancy.
 * For a listed walker w, every window slice a = Nb-window .. Nb+window and every particle i:
 * 1. Assignment.  For every site s take d_k = x_k(i) - R_k(s), fold it once by min_image<DIM> (the two compares, each
 *    against LboxHalf) and sum r2 left to right, nothing fused: pigs_grv_*'s arithmetic.  The assigned site s(i) is the
 *    smallest s of the minimal r2: `r2 < best`, strictly, with s ascending and best = +infinity at first.  A NaN never
 *    wins, nor does +infinity: a particle none of whose r2 compares below +infinity is LOST: s(i) = -1, it adds to no sum
 *    and no histogram, to no occupancy and no hop, and it counts in nlost.  u(i) is the folded d of the assigned site.
 *    THE SINGLE FOLD GIVES THE NEAREST IMAGE ONLY WHILE |x_k(i) - R_k(s)| < 3 Lbox[k]/2.  Both samplers wrap every bead
 *    they move once into [-Lbox/2, Lbox/2] (pigs_sampler.f90 wrap_coord and its device twin), and their proposals lie
 *    within a fraction of the box of a bead that is inside, so the beads stay in the primary cell; with sites inside it
 *    too |d_k| < Lbox[k] and the fold is exact.  Sites or uploaded paths far outside the primary cell are the caller's;
 *    the library does not judge it.
 * 2. Centre of mass, cm = 1: c_k = (sum_i u_k(i)) / n_assigned, the sum in ASCENDING PARTICLE ORDER from 0.0, one addition
 *    after the other (a lost particle adds 0.0) -- numpy's cumsum has its bits.  v(i) = u(i) - c.  cm = 0: v = u.
 *    The assignment itself always uses the uncorrected positions, whatever cm.
 * 3. Per assigned particle: m2 = sum_k v_k*v_k left to right, m4 = m2*m2.
 * One accumulate call adds per walker, js = a - (Nb - window):
 *   mom[w][js][0] += sum_i m2;  mom[w][js][1] += sum_i m4;  mom[w][js][2 + k] += sum_i v_k*v_k        (doubles)
 *   nassigned[w][js] += the assigned particles;   nlost[w] += the lost ones of every window slice
 *   occ[w][js][q] += the sites that hold q = 0, 1, 2 particles, q = 3: three or more
 *   hr[w][b] += 1, b = (int)t, t = sqrt(m2)/rbin, iff t < nbin in double, rbin = rmax/nbin (k_vh's self rule: every
 *     decision in double before the conversion, NaN drops out), over every window slice
 *   hx[w][k][b] += 1, b = (int)t, t = (v_k + rmax)/rbin, iff 0 <= t < 2 nbin in double: v_k over [-rmax, rmax)
 *   hop1[w] += sum over the window slices a but the last and over i of [s_i(a+1) != s_i(a)]
 *   hopw[w] += sum over i of [s_i(first slice) != s_i(last slice)]; a lost end drops the comparison in both
 *   samples[w] += 1
 * The hops follow a particle LABEL along tau, which the resident worldlines keep (pigs_fqs_* relies on the same).
 * Summation of mom.  No floating-point atomics and one fixed order: with 256 lanes, lane j takes the particles j, j + 256,
 * .. in ascending order; the 64 lanes of a wave are added by a butterfly (partner lane ^ 32, 16, .., 1), the waves in
 * wave order from 0.0, then acc += value by the one thread that owns (w, a) in the launch.  The same worldline gives the
 * same bits whatever the walker list, its order, the launch split or the number of walkers of the context; a walker
 * listed twice counts twice (in two launches), with bits equal to 2 x one count.
 * The estimators are the caller's divisions (profiles.normalize_lat, pigs_estimators.f90):
 *   <u^2>(tau_a) = mom[..][0]/nassigned, the Lindemann ratio gamma = sqrt(<u^2>)/a_nn with a_nn the sites' nearest-
 *   neighbour distance, alpha_2 = dim <u^4> / ((dim + 2) <u^2>^2) - 1, the vacant fraction occ[0]/(samples nsite), ...
 * Limit.  A workgroup keeps a tile of 256 sites, u of the slice, the occupancy and the histograms in LDS; pigs_lat_init
 * refuses (PIGS_ERR_ARG) a system with
 *   8 (256 dim + dim Np + 36) + 4 (nsite + (1 + 2 dim) nbin + 8) > 65536,
 * which serves Np = nsite = 1077 in 3D with up to 1032 bins.
 *
 * pigs_lat_init uploads the sites, allocates and zeroes the sums (again: resizes and zeroes).  PIGS_ERR_UNSUPPORTED on a
 * trapped context or dim = 1; PIGS_ERR_ARG for nsite < 1, a site coordinate that is not finite, nbin < 1, rmax not finite
 * or not > 0, window < 0 or window > Nb, cm not 0 or 1, and for the size limit above. */
int pigs_lat_init(pigs_ctx *ctx, int32_t nsite, const double *sites, int32_t nbin, double rmax, int32_t window, int32_t cm);
/* Adds the window of walkers[0..n) (NULL: 0..n-1; a walker listed twice counts twice).  Queued on the context's stream,
 * no upload, no host synchronisation: it sees the worldline every call queued before it left, never the next step's.
 * The list travels in the kernel arguments, at most 256 walkers per launch and more in further launches.
 * PIGS_ERR_ARG before pigs_lat_init, for n < 0 or for a walker out of range. */
int pigs_lat_accumulate(pigs_ctx *ctx, int32_t n, const int32_t *walkers);
/* All walkers' mom[n_walkers][2 window + 1][2 + dim], nassigned[n_walkers][2 window + 1], nlost[n_walkers],
 * occ[n_walkers][2 window + 1][4], hr[n_walkers][nbin], hx[n_walkers][dim][2 nbin], hop1, hopw and samples [n_walkers];
 * then zeroes those of the walkers w with reset[w] != 0 (reset == NULL: none).  Synchronises the context.  PIGS_ERR_ARG
 * before pigs_lat_init. */
int pigs_lat_read(pigs_ctx *ctx, double *mom, int64_t *nassigned, int64_t *nlost, int64_t *occ, int64_t *hr, int64_t *hx,
                  int64_t *hop1, int64_t *hopw, int64_t *samples, const int32_t *reset);

/* ---- the superfluid fraction from the diffusion of the centre of mass along imaginary time, and the unfolded
 * displacement of a particle, of a PERIODIC system (new: every family above is either blind to a wrap -- phasors at box
 * vectors -- or folds a displacement once; this one follows a worldline link by link) ---------------------------------
 * A ground-state path has no winding number.  The estimator used at T = 0 (Zhang, Kawashima, Carlson and Gubernatis 1995;
 * the one diffusion Monte Carlo uses) is
 *   rho_s,k / rho = lim_{tau -> inf} < ( sum_i [x_k(i, tau0 + tau) - x_k(i, tau0)] )^2 > / (2 lambda Np tau),  per box axis k
 * with lambda = hbar^2/2m and the displacement of every particle followed UNFOLDED through the periodic box.
 * Scope.  Periodic contexts with dim = 1, 2 or 3.  A trapped context gets PIGS_ERR_UNSUPPORTED.
 * Window and lags.  These are the rules of pigs_fqs_*:
 *   window slices a0 = Nb-window .. a1 = Nb+window, ns = 2 window + 1;
 *   links a = a0 .. a1-1;
 *   lags l = 0 .. Ntau with 0 <= Ntau <= 2 window;
 *   n_pairs(l) = ns - l.
 * For a listed walker w:
 * 1. Link vector.
 *    d_k(i,a) = x_k(i,a+1) - x_k(i,a), folded once by min_image<DIM>.  That is the two compares, each against LboxHalf,
 *    with nothing fused.
 *    nwrap[w] += the number of (i, a, k) on which a compare fired: raw d_k > LboxHalf[k] or < -LboxHalf[k].
 *    THE FOLD GIVES THE TRUE LINK ONLY WHILE THE LINK IS SHORTER THAN Lbox[k]/2.  This holds for any sampled path, since a
 *    link is about sqrt(dt).  The library does not judge it.
 * 2. Unfolded particle path.  U_k(i,a0) = 0.0 and U_k(i,a+1) = U_k(i,a) + d_k(i,a), one addition after the other.  numpy's
 *    cumsum has these bits.
 * 3. Centre of mass.
 *    The link sum is s_k(a) = sum_i d_k(i,a) in the lattice family's order: 256 lanes, lane j takes particles j, j+256, ..
 *    ascending from 0.0, then wave_sum (partner lane ^32, 16, .., 1), then the waves in wave order from 0.0.
 *    W_k(a0) = 0.0 and W_k(a+1) = W_k(a) + s_k(a).
 *    W is Np times the unfolded centre of mass.
 *    This order is restatable bit for bit in numpy: pad to 256 with +0.0, add the strided rows, then apply
 *    v = v + v[idx ^ m] per wave for each m.  tests/sf_numpy.py restates it that way.
 * 4. Sums of one call.
 *    C[w][l][k] += one running sum from 0.0 over a = a0 .. a1-l ascending of delta*delta, with
 *    delta = W_k(a+l) - W_k(a).  Given the orders above, C of a single call has the restatement's bits.
 *    D[w][l][k] += sum over i and a of delta_i*delta_i, with delta_i = U_k(i,a+l) - U_k(i,a).  The order is that of
 *    pigs_fqs_*'s D:
 *      lane j takes particles j, j+256, .. ascending;
 *      per particle, a ascending;
 *      then butterfly, then waves in wave order from 0.0;
 *      then acc += value by the one thread that owns (w, l, k) in the launch.
 *    Lag 0 adds exactly 0.0 to both.
 *    samples[w] += 1.
 * Determinism.  No floating-point atomics.  The same worldline gives the same bits whatever the walker list, its order,
 * the launch split or the number of walkers of the context.  A walker listed twice counts twice, in two launches.
 * Caller's divisions.  profiles.normalize_sf(got, Np, dt, lam=0.5) returns:
 *   tau_l = l dt;
 *   Dcm[l][k] = C/(samples n_pairs Np);
 *   rhos[l][k] = Dcm/(2 lam tau_l), NaN at l = 0, and its mean over the axes;
 *   msd[l][k] = D/(samples n_pairs Np);
 *   cross = Dcm - msd.
 * lam = 1/2 is the run's own unit: the spring term of ThermEnergy is 1/2 |dr|^2/dt^2, so a free link has variance dt per
 * axis.  profiles.superfluid_fraction(tau, Dcm_k, tmin) is the least-squares slope of Dcm over tau >= tmin, divided by
 * 2 lam, with the fit's own standard error.
 * (The lanes are 256 whatever Np, so with Np < 256 the idle lanes add +0.0: unlike pigs_fqs_*'s D, whose lanes follow Np.)
 * Scratch.  The unfolded paths of one launch, 8 (2 window + 1) dim NpPad bytes per walker, sit in device memory between
 * the two kernels of a launch.  pigs_sf_init allocates min(n_walkers, 256, what fits 256 MiB) walkers of it, one at the
 * least, and pigs_sf_accumulate puts no more walkers into a launch; pigs_set_tuning "sf_scratch_mib" (1..2048, read by the
 * next pigs_sf_init) sets another budget.  The bits do not depend on it.
 *
 * pigs_sf_init allocates and zeroes the sums (again: resizes and zeroes).  PIGS_ERR_UNSUPPORTED on a trapped context;
 * PIGS_ERR_ARG for window < 0, window > Nb, Ntau < 0, Ntau > 2 window, more than 3072 lags, or accumulators beyond 2 GiB. */
int pigs_sf_init(pigs_ctx *ctx, int32_t Ntau, int32_t window);
/* Adds the window of walkers[0..n) (NULL: 0..n-1; a walker listed twice counts twice).  Queued on the context's stream,
 * no upload, no host synchronisation: it sees the worldline every call queued before it left, never the next step's.
 * The list travels in the kernel arguments, at most 256 walkers per launch and more in further launches.
 * PIGS_ERR_ARG before pigs_sf_init, for n < 0 or for a walker out of range. */
int pigs_sf_accumulate(pigs_ctx *ctx, int32_t n, const int32_t *walkers);
/* All walkers' C[n_walkers][Ntau+1][dim] and D[n_walkers][Ntau+1][dim] (doubles), nwrap[n_walkers] and samples[n_walkers]
 * (int64); then zeroes those of the walkers w with reset[w] != 0 (reset == NULL: none).  Synchronises the context.
 * PIGS_ERR_ARG before pigs_sf_init. */
int pigs_sf_read(pigs_ctx *ctx, double *C, double *D, int64_t *nwrap, int64_t *samples, const int32_t *reset);

/* ---- the cluster-size distribution of a PERIODIC system, over a slice window (new: the structural families above look
 * at pairs or triplets inside a radius; this one says which particles belong together -- connected components of the
 * bond graph, an iterative, data-dependent pass whose result, a partition, has no summation order) -------------------
 * Scope.  Periodic contexts with dim = 1, 2 or 3 and Np <= PIGS_CL_NP_MAX.  A trapped context gets PIGS_ERR_UNSUPPORTED.
 * The window covers slices a = Nb-window .. Nb+window.  For each window slice of a listed walker:
 * Bond.  i != j are bonded iff 0 < r2 < rc2 in double.  This is pigs_bop_*'s rule, so a coincident pair and a non-finite
 *   r2 are no bond.
 *   r2 is the squares of d = x(i) - x(j) summed left to right, d folded once by min_image<DIM>.
 *   rc2 = rc*rc is computed once on the host.
 *   Padding particles (index >= Np) never take part.
 * Label.  label(i) is the smallest particle index in i's connected component of the bond graph.  A cluster's root is that
 *   index, and its size s is the number of its members.
 * Integer sums (int64, per walker w):
 *   nsize[w][s-1] += 1 per cluster of size s (s = 1..Np).
 *   nlarge[w][smax-1] += 1 per slice, smax being the slice's largest size.
 *   nbond[w] += the slice's bonds (i < j).
 *   samples[w] += 1 per slice.
 *   It follows that sum_s s nsize = Np samples and sum_s nlarge = samples.
 * Radius of gyration (double, rg2[w][s-1]), summed in one fixed order:
 *   For each i: t_i = 0.0; for j = i+1..Np-1 ascending with label(j) == label(i): t_i = t_i + r2_ij (the r2 above).
 *   For each cluster: T = 0.0; over its members i ascending: T = T + t_i; then g = T / ((double)s*(double)s).  For s = 1
 *   this gives g = 0.
 *   For each size: G_slice[s] = 0.0, plus the g of that size's clusters in ascending root order.
 *   rg2[w][s-1] = rg2[w][s-1] + G_slice[s], slices ascending, one add per slice and size.
 *   No floating-point atomics.
 *   g = (1/s^2) sum_{i<j} r_ij^2 is the true Rg^2 of the cluster ONLY WHILE THE CLUSTER'S EXTENT STAYS BELOW HALF THE BOX:
 *   beyond, the folded r_ij of two members is no longer their separation along the cluster.  The library does not judge it.
 * Determinism.  The same worldline gives the same counts and the same bits of rg2 whatever the walker list, its order, the
 * launch split, the scratch budget or the number of walkers of the context.  A walker listed twice counts twice, in two
 * launches.
 * Caller's divisions.  profiles.normalize_cl(got, Np) returns n(s) per sample, the particle fraction s n(s)/Np,
 * P_largest(s), <Rg^2>(s) = rg2/nsize (NaN where n(s) = 0), the mean number of clusters, <smax>/Np, the mean cluster size
 * S = sum s^2 n(s) / sum s n(s) and the bonds per particle.
 * Kernel.  One workgroup labels a slice in LDS by min-label hooking and pointer jumping until a sweep changes nothing
 * (a vote, not a fixed count).  Up to 256 particles the bonds are kept as bit rows in LDS; beyond, every sweep computes the
 * distances again.  The counts do not depend on it.  PIGS_CL_NP_MAX is what the slice, the labels and the counters of one
 * workgroup hold in LDS.
 * Scratch.  The per-slice sums of one launch, 8 (2 window + 1) Np bytes per walker, sit in device memory between the two
 * kernels of a launch.  pigs_cl_init allocates min(n_walkers, 256, what fits 256 MiB) walkers of it, one at the least, and
 * pigs_cl_accumulate puts no more walkers into a launch; pigs_set_tuning "cl_scratch_mib" (1..2048, read by the next
 * pigs_cl_init) sets another budget.  The bits do not depend on it.
 *
 * pigs_cl_init allocates and zeroes the sums (again: resizes and zeroes).  PIGS_ERR_UNSUPPORTED on a trapped context;
 * PIGS_ERR_ARG for rc not finite or <= 0, rc beyond half the shortest side, window < 0, window > Nb, Np > PIGS_CL_NP_MAX,
 * or sums beyond 2 GiB. */
#define PIGS_CL_NP_MAX 2048
int pigs_cl_np_max(void);                /* PIGS_CL_NP_MAX of the library that is loaded */
int pigs_cl_init(pigs_ctx *ctx, double rc, int32_t window);
/* Adds every window slice of walkers[0..n) (NULL: 0..n-1; a walker listed twice counts twice).  Queued on the context's
 * stream, no upload, no host synchronisation: it sees the worldline every call queued before it left, never the next
 * step's.  The list travels in the kernel arguments, at most 256 walkers per launch and more in further launches.
 * PIGS_ERR_ARG before pigs_cl_init, for n < 0 or for a walker out of range. */
int pigs_cl_accumulate(pigs_ctx *ctx, int32_t n, const int32_t *walkers);
/* All walkers' nsize[n_walkers][Np], nlarge[n_walkers][Np], nbond[n_walkers], samples[n_walkers] (int64) and
 * rg2[n_walkers][Np] (doubles); then zeroes those of the walkers w with reset[w] != 0 (reset == NULL: none).
 * Synchronises the context.  PIGS_ERR_ARG before pigs_cl_init. */
int pigs_cl_read(pigs_ctx *ctx, int64_t *nsize, int64_t *nlarge, int64_t *nbond, int64_t *samples, double *rg2,
                 const int32_t *reset);
/* The largest number of labelling sweeps that any (walker, slice) needed since pigs_cl_init: a report for benchmarks, no
 * part of the result.  Synchronises the context.  PIGS_ERR_ARG before pigs_cl_init. */
int pigs_cl_sweeps(pigs_ctx *ctx, int32_t *max_sweeps);

/* ---- wrapping clusters, their true extent and cluster persistence along tau (new: pigs_cl_* above cannot tell a cluster
 * that wraps the box, its rg2 is no extent beyond half a box side, and it never compares the clusters of two slices) -----
 * Periodic systems only.  Everything is per slice of the window Nb-window .. Nb+window of a walker.
 * Bonds and clusters are pigs_cl_*'s.  Take d = x(i) - x(j), folded once per axis by min_image, with r2 summed left to
 *   right.  A bond exists iff 0 < r2 < rc2.  A cluster is a connected component, labelled by its smallest index.
 * Fold number.  n_ij[k] describes the fold min_image applied to d[k]: +1 where v - L was taken, -1 where v + L was taken,
 *   0 where none was.  n_ji = -n_ij, because d == +-L/2 folds in neither direction.  For a bond every |folded d[k]| < rc
 *   <= L_k/2.
 * Wrapping.  A cluster wraps along axis k iff it contains a closed walk of bonds whose fold numbers add up to a non-zero
 *   value along k.
 *   Its wrap mask has bit k set for every such axis.  Mask 0 means finite.
 *   The definition is free of any spanning tree.
 *   Equivalently, choose image numbers m_i (integers per axis, m_root = 0) with m_i = m_j + n_ij along the edges of any
 *   spanning tree.  Bit k is set iff some bond of the cluster has m_i[k] - m_j[k] != n_ij[k].
 *   For a finite cluster the m_i are unique.
 * Unfolded separation in a finite cluster: du[k] = (x_i[k] - x_j[k]) - c*L[k] with c = (double)(m_i[k] - m_j[k]).
 *   The product comes first, then the subtraction, nothing fused.
 *   ru2 is summed left to right from 0.0.
 *   With c in {0, +-1} this has min_image's bits.  On a cluster whose pairs all lie within half the box, g below therefore
 *   equals pigs_cl's g bit for bit.
 * Sums per walker.  Every integer sum is int64 and must equal any correct algorithm's:
 *   nwrap[8]   (index = mask)  clusters with that wrap mask
 *   mwrap[8]   (index = mask)  particles in clusters with that wrap mask
 *   swrap[8]   (index = mask)  slices whose OR over all cluster masks is that mask
 *   nfin[Np]   (index s-1)     finite clusters of size s
 *   samples                    slices
 *   rg2u[Np]   (double)        over the finite clusters of size s, the sum of g = sum_{i<j} ru2 / s^2
 *   rg2u is summed in pigs_cl's fixed order: t_i over j ascending, T over the members ascending, the roots ascending, the
 *   slices ascending.  Wrapping clusters contribute nothing to nfin or rg2u.
 * Persistence.  For the lags l = 0..ntau and every origin a with a and a+l both in the window, call i<j "together in
 *   slice a" when they carry the same label there.  Each of the following has shape [ntau+1]:
 *   first[l]  += pairs together in a.
 *   second[l] += pairs together in a+l.
 *   both[l]   += pairs together in both.
 *   norig[l]  += 1.
 *   At l = 0 the three pair counts are sum_clusters s(s-1)/2.
 * Determinism.  As pigs_cl_*: the same worldline gives the same counts and the same bits of rg2u whatever the walker list,
 * its order, the launch split, the scratch budget or the number of walkers of the context.  A walker listed twice counts
 * twice, in two launches.
 * Caller's divisions.  profiles.normalize_pc(got, Np) returns the wrapping probabilities per axis, for any and for all
 * axes, the strength P_inf, the finite n(s)/Np, the mean finite cluster size, <Rg^2>(s) of the finite clusters, the
 * persistence C(l) = both/first and the Jaccard index both/(first + second - both); NaN where a denominator is zero.
 * Kernel.  pigs_cl's labelling; then image numbers spread from every root over the bonds, sweep by sweep, until a vote
 * finds a sweep that assigned nobody (at most Np - 1 sweeps, for a chain), the wrap check over the bonds, and a second
 * kernel that counts the pairs per (walker, origin).  Limits: PIGS_CL_NP_MAX particles.
 * Scratch.  The per-slice sums and the labels of one launch, 12 (2 window + 1) Np bytes per walker, sit in device memory
 * between the kernels of a launch.  pigs_pc_init allocates min(n_walkers, 256, what fits 256 MiB) walkers of it, one at the
 * least, and pigs_pc_accumulate puts no more walkers into a launch; pigs_set_tuning "pc_scratch_mib" (1..2048, read by the
 * next pigs_pc_init) sets another budget.  The bits do not depend on it.
 *
 * pigs_pc_init allocates and zeroes the sums (again: resizes and zeroes).  PIGS_ERR_UNSUPPORTED on a trapped context;
 * PIGS_ERR_ARG for rc not finite or <= 0, rc beyond half the shortest side, window < 0, window > Nb, ntau < 0,
 * ntau > 2 window, Np > PIGS_CL_NP_MAX, or sums beyond 2 GiB.  It works beside an initialised pigs_cl_* of the context. */
int pigs_pc_np_max(void);                /* PIGS_CL_NP_MAX of the library that is loaded */
int pigs_pc_init(pigs_ctx *ctx, double rc, int32_t window, int32_t ntau);
/* pigs_cl_accumulate's contract: adds every window slice of walkers[0..n) (NULL: 0..n-1; a walker listed twice counts
 * twice), queued on the context's stream with no upload and no host synchronisation, at most 256 walkers per launch.
 * PIGS_ERR_ARG before pigs_pc_init, for n < 0 or for a walker out of range. */
int pigs_pc_accumulate(pigs_ctx *ctx, int32_t n, const int32_t *walkers);
/* All walkers' nwrap, mwrap, swrap [n_walkers][8], nfin [n_walkers][Np], samples [n_walkers] (int64), rg2u [n_walkers][Np]
 * (doubles) and first, second, both, norig [n_walkers][ntau+1] (int64); then zeroes those of the walkers w with
 * reset[w] != 0 (reset == NULL: none).  Synchronises the context.  PIGS_ERR_ARG before pigs_pc_init. */
int pigs_pc_read(pigs_ctx *ctx, int64_t *nwrap, int64_t *mwrap, int64_t *swrap, int64_t *nfin, int64_t *samples, double *rg2u,
                 int64_t *first, int64_t *second, int64_t *both, int64_t *norig, const int32_t *reset);
/* The largest numbers of labelling sweeps and of image-number sweeps that any (walker, slice) needed since pigs_pc_init: a
 * report for benchmarks, no part of the result.  Synchronises the context.  PIGS_ERR_ARG before pigs_pc_init. */
int pigs_pc_sweeps(pigs_ctx *ctx, int32_t *label_sweeps, int32_t *image_sweeps);

/* ---- bond-orientational order of a PERIODIC system in 2D or 3D, over a slice window (new: every family above is a
 * density correlation; this one tells fcc from hcp from bcc, a hexatic from a liquid, and gives a per-particle measure)
 * Scope: periodic contexts with dim = 2 or 3.  pigs_bop_init returns PIGS_ERR_UNSUPPORTED on a trapped context and for
 * dim = 1.
 * For every listed walker and every slice a = Nb-window..Nb+window:
 * - Bonds.  For particles i and j take d_k = x_k(i) - x_k(j), folded once as pbc_mod.f90:40-41 does (min_image<DIM>: the
 *   two compares, each against LboxHalf), and r2 the sum of the squares, left to right, with no fused multiply-adds
 *   (pigs_grv_*'s arithmetic; r2 of (j, i) has the bits of r2 of (i, j)).  j is a neighbour of i if and only if
 *   0 < r2 and r2 < rnb*rnb hold in double.  The particle itself, a coincident partner (r2 = 0) and a non-finite r2 are
 *   no bonds.  n_i is the number of neighbours of i.  rnb <= min_k Lbox[k]/2 makes the minimum image of a bond unique.
 * - 3D, l = 4 and 6.  q_lm(i) = (1/n_i) sum_j Y_lm(d_ij/|d_ij|), and 0 where n_i = 0; only m = 0..l are kept (Y_l,-m
 *   follows by symmetry).  q_l(i) = sqrt(4 pi/(2l+1) sum_{m=-l..l} |q_lm(i)|^2) is the local invariant, and
 *   Q_l = sqrt(4 pi/(2l+1) sum_m |Q_lm|^2) with Q_lm = (1/Np) sum_i q_lm(i) the slice invariant.
 * - 2D, n = 4 and 6.  psi_n(i) = (1/n_i) sum_j e^{i n theta_ij}; |psi_n(i)| and Psi_n = |(1/Np) sum_i psi_n(i)| take the
 *   slots of q_l(i) and Q_l in every array below.
 * - Correlation (Nr > 0).  For the pairs i < j with r2 <= rcut2 and u = sqrt(r2)/rbin < Nr (pigs_grv_*'s radial rule,
 *   coincident pairs included), c_ij = (4 pi/13) Re sum_{m=-6..6} q_6m(i) q_6m(j)* in 3D and Re psi_6(i) psi_6(j)* in 2D
 *   (|c_ij| <= 1) is added to bin (int)u, and 1 to the bin's pair count.  G6(r) = G/GN.
 * Accumulators per walker, all 8-byte elements:
 *   S[w][8]      doubles, each summed over the window slices of every call: Q4, Q4^2, Q6, Q6^2, (1/Np) sum_i q4(i),
 *                (1/Np) sum_i q6(i), sum_i n_i (an exact integer), and a reserved slot that stays 0
 *   H[w][2][Nh]  int64: the counts of q4(i) and of q6(i) over [0, 1], bin min((int)(q Nh), Nh - 1), decided in double
 *                before the conversion (a particle without neighbours counts in bin 0); every slice adds Np to each
 *   G[w][Nr]     doubles: the sums of c_ij per radial bin;  GN[w][Nr] int64: the pairs per bin
 *   samples[w]   int64: calls, not slices, as pigs_sqv_* counts them; a call adds 2 window + 1 slices
 * Order of the sums (no floating-point atomics; the same worldline gives the same bits whatever the walker list, its
 * order, the launch split at 256 walkers or the number of walkers of the context): the bonds of a particle in ascending
 * j; the particle sums per lane in ascending i, the wave by a fixed butterfly, the waves in wave order; the slices in
 * ascending order, then acc += value.  The per-bin sums of c_ij are kept in fixed point within a slice: c_ij 2^40
 * rounded to nearest, added as int64 (which no order changes), converted to double once per slice and bin -- each
 * c_ij carries an error of at most 2^-41 from it.  A bin holds at most Np (Np - 1)/2 pairs of a slice, and
 * Np (Np - 1)/2 2^40 stays below 2^63 up to Np = 4096; pigs_bop_init refuses a larger Np where Nr > 0.
 * One workgroup holds a slice in LDS: 8 dim Np bytes for the positions, with Nr > 0 another 8 c Np for the l = 6
 * components (c = 13 in 3D, 2 in 2D) and 16 Nr for the bins, and 800 (3D) or 224 (2D) bytes of reduction space;
 * pigs_bop_init refuses (PIGS_ERR_ARG) what passes the 160 KiB of a CU.  Without the correlation that is Np <= 6793 in
 * 3D and Np <= 10226 in 2D; with Nr = 100 it is Np <= 1261 in 3D, and in 2D the rule above (4096) comes first.
 *
 * pigs_bop_init allocates and zeroes the accumulators (again: resizes and zeroes).  PIGS_ERR_ARG unless rnb is finite
 * with 0 < rnb <= min_k Lbox[k]/2, 0 <= window <= Nb, 1 <= Nh <= 4096, Nr >= 0 (0 switches the correlation off; rbin
 * is then ignored), and for Nr > 0 rbin is finite and positive; and for the two limits on Np above. */
int pigs_bop_init(pigs_ctx *ctx, double rnb, int32_t window, int32_t Nh, int32_t Nr, double rbin);
/* Adds the window of walkers[0..n) (NULL: 0..n-1; a walker listed twice counts twice).  Queued on the context's stream,
 * no upload, no host synchronisation: it sees the worldline every call queued before it left, never the next step's.
 * The list travels in the kernel arguments, at most 256 walkers per launch and more in further launches.
 * PIGS_ERR_ARG before pigs_bop_init, for n < 0 or for a walker out of range. */
int pigs_bop_accumulate(pigs_ctx *ctx, int32_t n, const int32_t *walkers);
/* All walkers' S[n_walkers][8], H[n_walkers][2][Nh], G[n_walkers][Nr], GN[n_walkers][Nr] and samples[n_walkers]; then
 * zeroes those of the walkers w with reset[w] != 0 (reset == NULL: none).  G and GN may be NULL where Nr = 0.
 * Synchronises the context.  PIGS_ERR_ARG before pigs_bop_init. */
int pigs_bop_read(pigs_ctx *ctx, double *S, int64_t *H, double *G, int64_t *GN, int64_t *samples, const int32_t *reset);

/* ---- imaginary-time profiles of the potential energy, the virial and the link lengths (new: pigs_fqt_*, pigs_sqv_*,
 * pigs_fqv_*, pigs_grv_* and the density profiles all take a slice window "inside the converged part of the path"; this
 * is the quantity that shows where that part is) ----------------------------------------------------------------------
 * Periodic and trapped contexts.  Per listed walker w and EVERY slice b = 0..2Nb an accumulate call adds four sums,
 *   Q[w][b][0]  Vpair = sum_{i<j} v(r_ij)          v  = Interpolate opt 0 on VTable, the reference's indexing
 *   Q[w][b][1]  Vext  = sum_i sum_k TrapPot(0, a_ho(k), x_k(i))       (trap; exactly 0.0 in a periodic system)
 *   Q[w][b][2]  W     = sum_{i<j} r_ij v'(r_ij)    v' = Interpolate opt 1 on VTable, the derivative of the force terms
 *   Q[w][b][3]  D2    = sum_i |x_i(b) - x_i(b+1)|^2                   (exactly 0.0 for b = 2Nb)
 * and 1 to samples[w].  Pairs as PotentialEnergy takes them (sample_mod.f90:13-150): periodic -- the difference folded
 * once, counted if and only if r^2 <= rcut2, every term v and r v' with the reference's own rounding (only the order
 * of the sum differs); trap -- plain distance, no cutoff, the plain arithmetic, table indices clamped to the table.  D2 of a
 * periodic system folds the link once and counts a particle only if the folded |link|^2 <= rcut2 (quirk Q8, as
 * ThermEnergy's spring term); in the trap it is the plain distance.  The estimators are the caller's divisions
 * (profiles.normalize_tau): per particle Vpair/(samples Np), Vext/(samples Np), W/(samples Np), and the kinetic
 * estimator of link b, dim/(2 dt) - D2[b]/(2 dt^2 Np samples); tau_b = (b - Nb) dt.  The pressure of a periodic system
 * follows from the virial, P = density/dim (2 K/N - W/N); pairs beyond rcut are not in W and no tail correction is made.
 * V(tau_b) falls from the trial function's value at b = 0, 2Nb to a plateau: the plateau is the usable window.
 * The library still does not judge it.
 * The sums are taken in fixed orders without floating-point atomics (per-lane sums in ascending particle order, the wave,
 * the waves in wave order, then acc += value): the same worldline gives the same bits whatever the walker list, its
 * order, the launch split or the number of walkers of the context (there is one kernel form and no tuning key).  A
 * non-finite term (a coincident pair) stays in its own element (w, b, quantity).
 *
 * pigs_tau_init allocates and zeroes the sums (again: zeroes). */
int pigs_tau_init(pigs_ctx *ctx);
/* Adds every slice of walkers[0..n) (NULL: 0..n-1; a walker listed twice counts twice).  Queued on the context's stream,
 * no upload, no host synchronisation: it sees the worldline every call queued before it left, never the next step's.
 * The list travels in the kernel arguments, at most 256 walkers per launch and more in further launches.
 * PIGS_ERR_ARG before pigs_tau_init, for n < 0 or for a walker out of range. */
int pigs_tau_accumulate(pigs_ctx *ctx, int32_t n, const int32_t *walkers);
/* All walkers' raw sums Q[n_walkers][2Nb+1][4] and samples[n_walkers]; then zeroes those of the walkers w with
 * reset[w] != 0 (reset == NULL: none).  Synchronises the context.  PIGS_ERR_ARG before pigs_tau_init. */
int pigs_tau_read(pigs_ctx *ctx, double *Q, int64_t *samples, const int32_t *reset);

/* ---- multi-GPU: block-estimator reduction (new) ------------------------ */
/* RCCL communicator over `nranks` contexts.  Single-process form (one host thread per
 * GPU, the Fortran host: pigs_vpi's &gpu n_gpus = G): pigs_comm_init_all.  Multi-process form: rank 0 obtains an id
 * with pigs_comm_unique_id, distributes the 128 bytes out of band, every rank calls
 * pigs_comm_init_rank.  pigs_comm_init_all on contexts that share a device (a one-GPU rehearsal) sets up an
 * in-process reduction instead of RCCL: same semantics (ranks added in rank order), no xGMI. */
int pigs_comm_unique_id(char id[128]);
int pigs_comm_init_rank(pigs_ctx *ctx, int32_t nranks, int32_t rank, const char id[128]);
int pigs_comm_init_all(pigs_ctx **ctxs, int32_t nranks);
/* Sum vec[0..n) (host memory, fp64) over all ranks, in place. */
int pigs_estimators_allreduce(pigs_ctx *ctx, double *vec, int32_t n);

#ifdef __cplusplus
}
#endif
#endif /* PIGS_HIP_H */
