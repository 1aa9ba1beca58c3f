// pigs_kernels.h -- host-callable launchers of the gfx950 kernels (pigs_kernels.hip).
// All launches are asynchronous on the given stream and allocate nothing.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pigs_device.h"
#include "pigs_walker_split.h"

namespace pigs {

// K1 kernel variants (pigs_k1.hip).  The numbers are part of the tuning interface (pigs_set_tuning "k1_variant");
// 3-6 and 9-11 were A/B forms of round 1 (LDS table / compaction / prefetch-only / first persistent kernel) that
// measured slower and are gone: profiles/r01_k1_variants_ab*.txt keeps their numbers.
enum K1Variant {
    K1_AUTO = 0,            // library's choice (by system, never by launch size: see launch_delta_action)
    K1_V1 = 1,              // plain statement
    K1_V2 = 2,              // exact-term: exact short division, fused sqrt/rinv, one LDS-transpose reduction
    K1_FAST = 7,            // v2 with the short arithmetic (~1 ulp per term instead of the reference's rounding; PBC)
    K1_FAST_PREFETCH = 8,   // + all partner loads of an item issued up front (Np <= 256)
    K1_PIPE2 = 12,          // persistent: LDS table image, branch-free short arithmetic, item queue, look-ahead loads (Np <= 256)
    K1_GRID = 13,           // pipe2's per-item arithmetic on a plain grid (global table image): identical bits, small launches
    K1_REFORDER = 14        // validation: exact terms added in the reference's jp order -- Delta S bit-identical to the reference
};
inline bool k1_variant_valid(int v)
{
    return v == K1_AUTO || v == K1_V1 || v == K1_V2 || v == K1_FAST || v == K1_FAST_PREFETCH || v == K1_PIPE2 ||
           v == K1_GRID || v == K1_REFORDER;
}

hipError_t launch_delta_action(const DevParams &P, int variant, const double *paths, const double *VT,
                               const double *VTimg, const double *WF, int n_items, const int32_t *walker,
                               const int32_t *ip, const int32_t *ib, const double *xnew,
                               const double *xold, double *out, double *parts, hipStream_t st);

// max_blocks > 0 caps the persistent form's grid (estimators that run NEXT TO the sampler take half the chip)
hipError_t launch_slice_energy(const DevParams &P, const double *paths, const double *VT, const double *VTimg,
                               int n_slots, const int32_t *slot_walker, const int32_t *slot_ib,
                               int force_mode, int want_spring, double *out, hipStream_t st, int max_blocks = 0);

hipError_t launch_therm_combine(const DevParams &P, int n, const double *slices, double *E,
                                double *Ec, double *Ep, hipStream_t st);

hipError_t launch_local_energy(const DevParams &P, const double *paths, const double *VT,
                               const double *WF, int n_slots, const int32_t *slot_walker, int ib,
                               double *out, hipStream_t st);

hipError_t launch_structure(const DevParams &P, const double *paths, int n_slots, const int32_t *slot_walker,
                            int ib, int Nbin, double rbin, int Nk, double *gr, double *Sk, hipStream_t st);

// pigs_density.hip: planar / radial density and pair distribution of slice Nb of a trapped system, 64-bit counts
// accumulated per walker (pigs_density_accumulate).  The walker list travels in the kernel arguments (WalkerList,
// pigs_walker_split.h: at most kWalkerListMax walkers per launch), here and in the six families below.  The pair
// histogram is staged in LDS for Nbin <= kDensLdsBins and added with global atomics beyond.
constexpr int kDensLdsBins = 8192;
hipError_t launch_density(const DevParams &P, const double *paths, int n, const WalkerList &list, int Nbin, double h,
                          double b, double br, unsigned long long *planar, unsigned long long *radial,
                          unsigned long long *pair, unsigned long long *samples, hipStream_t st);

// pigs_fqt.hip: imaginary-time density correlations F(q,tau) of a periodic system (pigs_fqt_accumulate).  Stage 1 writes
// C(s), S(s) of the window slices Nb-window .. Nb+window of the n listed walkers to rho ([slot][slice][(iq-1) dim + k][2]
// doubles), stage 2 adds the ordered pair sums of the lags 0..Ntau to acc ([walker][l][(iq-1) dim + k]) and 1 to samples.
// One thread owns an accumulator element per launch: the caller never lists a walker twice in ONE launch.
hipError_t launch_fqt(const DevParams &P, const double *paths, int n, const WalkerList &list, int window, int Ntau, int Nk,
                      double *rho, double *acc, unsigned long long *samples, hipStream_t st);

// pigs_sqv.hip: the vector structure factor on the full reciprocal grid (pigs_sqv_accumulate).  Stage 1 writes
// C^2 + S^2 of every stored vector for the window slices Nb-window .. Nb+window of the n listed walkers to rho2
// ([slot][slice][iqv] doubles), stage 2 adds their sum over the slices (ascending) to acc ([walker][iqv]) and 1 to samples.
// One thread owns an accumulator element per launch: the caller never lists a walker twice in ONE launch.  sqv_shape
// gives the sizes that follow from (dim, nmax) alone: Nq vectors, the prefixes and chunks of the work items, the
// particle tile and its LDS bytes.
constexpr int kSqvChunk = 8;                     // values of |n_dim| per work item: 4 * 8 running sums in registers
constexpr int kSqvThreadsMax = 512;
constexpr size_t kSqvLdsBudget = 40 * 1024;      // phasor table of one particle tile: several workgroups share a CU
struct SqvShape { long long Nq; int nprefix, nchunk, tile, threads; size_t lds; };
SqvShape sqv_shape(int dim, int nmax);
hipError_t launch_sqv(const DevParams &P, const double *paths, int n, const WalkerList &list, int window, int nmax,
                      double *rho2, double *acc, unsigned long long *samples, hipStream_t st);

// pigs_fqv.hip: F(q,tau) on the vectors of pigs_sqv_* (pigs_fqv_accumulate).  Stage 1 writes (C, S) of every stored vector
// for the window slices of the n listed walkers to rho ([slot][slice][iqv][2] doubles) with the device code of k_sqv_rho2,
// stage 2 stages tiles of fqv_width(ns) vectors x ns slices in LDS and adds the ordered pair sums of the lags 0..Ntau to
// acc ([walker][l][iqv]) and 1 to samples.  One thread owns an accumulator element per launch: the caller never lists a
// walker twice in ONE launch.  fqv_width is the largest power of two <= kFqvWidthMax whose tile fits kFqvLdsBudget
// (0: not even one vector's ns slices fit, which pigs_fqv_init refuses).
constexpr int kFqvThreads = 256;
constexpr int kFqvWidthMax = 64;                 // one wave of lanes over consecutive vectors
constexpr size_t kFqvLdsBudget = 64 * 1024;      // 16 bytes per (slice, vector): 64 wide up to 64 slices, 16 wide at 161
int fqv_width(int ns);
hipError_t launch_fqv(const DevParams &P, const double *paths, int n, const WalkerList &list, int window, int Ntau, int nmax,
                      double *rho, double *acc, unsigned long long *samples, hipStream_t st);

// pigs_fqs.hip: the self part of F(q,tau) on the vectors of pigs_sqv_* and the imaginary-time displacement
// (pigs_fqs_accumulate).  k_fqs_msd adds the sums of r2 and r2^2 of the lags 0..Ntau to dsp ([walker][l][2]); k_fqs loops
// over the particles with their phasors in LDS (the per-axis table of all window slices, then a tile of fqs_shape().width
// vectors x ns slices) and the lag sums in registers, at most kFqsLags lags per thread, and adds them to acc
// ([walker][l][iqv]) and 1 to samples.  One thread owns an accumulator element per launch: the caller never lists a
// walker twice in ONE launch.  fqs_shape gives the largest power of two <= kFqsWidthMax whose table and tile fit
// kFqsLdsBudget and whose kFqsThreads / width lag groups cover Ntau + 1 lags (width 0: none, which pigs_fqs_init refuses).
constexpr int kFqsThreads = 256;
constexpr int kFqsWidthMax = 64;                 // one wave of lanes over consecutive vectors
constexpr int kFqsLags = 12;                     // lag sums a thread keeps in registers across the particle loop
constexpr size_t kFqsLdsBudget = 64 * 1024;      // 16 bytes per (slice, axis, m) and per (slice, vector)
struct FqsShape { int width; size_t lds; };
FqsShape fqs_shape(int dim, int nmax, int window, int Ntau);
hipError_t launch_fqs(const DevParams &P, const double *paths, int n, const WalkerList &list, int window, int Ntau, int nmax,
                      double *acc, double *dsp, unsigned long long *samples, hipStream_t st);

// pigs_grv.hip: the pair distribution of a periodic system on the vector grid and radially, over the window slices
// Nb-window .. Nb+window (pigs_grv_accumulate): 64-bit counts per walker, vec [walker][Nbin^dim] (x fastest) and radial
// [walker][Nr].  A walker may be listed twice in one launch (integer atomics).  grv_shape decides the form: the vector grid privatised in LDS (form 1, or
// automatic up to kGrvAutoLdsBins bins where it fits kGrvLdsBudget next to the staging tiles and the radial histogram) with
// nchunk runs of slices per walker, or global atomics with one workgroup per (walker, slice); vec_lds && !vec_fits is
// a forced LDS form that does not fit, which the caller refuses.
constexpr int kGrvTile = 256;                    // particles of a slice staged per tile
constexpr int kGrvThreadsMax = 1024;
constexpr size_t kGrvLdsBudget = 160 * 1024;     // LDS of one CU on gfx950
constexpr long long kGrvAutoLdsBins = 1ll << 15; // automatic form: LDS up to 32^3 bins (measured)
struct GrvShape { int vec_lds, vec_fits, rad_lds, nchunk, threads, flush_every; size_t lds; };
GrvShape grv_shape(int dim, int Np, int Nbin, int Nr, int window, int form, int n_list, int n_cu);
hipError_t launch_grv(const DevParams &P, const double *paths, int n, const WalkerList &list, const GrvShape &s, int window,
                      int Nbin, int Nr, double rbin, unsigned long long *vec, unsigned long long *radial,
                      unsigned long long *samples, hipStream_t st);

// pigs_tau.hip: imaginary-time profiles (pigs_tau_accumulate): per listed walker and slice b = 0..2Nb the sums Vpair, Vext,
// W = sum r v'(r) and D2 = sum_i |x_i(b) - x_i(b+1)|^2 are added to acc ([walker][2Nb+1][4]) and 1 to samples.  One
// workgroup owns an accumulator element per launch: the caller never lists a walker twice in ONE launch.
hipError_t launch_tau(const DevParams &P, const double *paths, const double *VT, int n, const WalkerList &list, double *acc,
                      unsigned long long *samples, hipStream_t st);

// pigs_bop.hip: bond-orientational order over the window slices (pigs_bop_accumulate).  k_bop, one workgroup per (listed
// walker, slice) with the whole slice and the table of the particles' l = 6 components in LDS, adds the local invariants
// to hist ([walker][2][Nh], integer atomics) and the pair counts of G6(r) to gn ([walker][Nr]), and writes the slice's 8
// scalars and Nr bins to scratch ([slot][slice][8 + Nr]); k_bop_combine adds the slices in ascending order to S
// ([walker][8]) and G ([walker][Nr]) and 1 to samples.  One thread owns an accumulator element per launch: the caller
// never lists a walker twice in ONE launch.  The per-bin sums of c_ij are kept in fixed point, c 2^40 rounded to nearest
// in an int64, which no order of the pairs changes; a bin holds at most Np (Np - 1) / 2 pairs with |c| <= 1, which stays
// below 2^63 up to kBopNpMax particles.  bop_lds_bytes is the dynamic LDS of k_bop, which has to fit kBopLdsBudget.
constexpr int kBopThreads = 256;
constexpr double kBopFixScale = 1099511627776.0; // 2^40
constexpr int kBopNpMax = 4096;                  // 4096 * 4095 / 2 < 2^23
constexpr int kBopHistMax = 4096;
constexpr size_t kBopLdsBudget = 160 * 1024;     // LDS of one CU on gfx950
size_t bop_lds_bytes(int dim, int Np, int Nr);
hipError_t launch_bop(const DevParams &P, const double *paths, int n, const WalkerList &list, int window, int Nh, int Nr,
                      double rnb2, double rbin, double *scratch, double *S, unsigned long long *hist, double *G,
                      unsigned long long *gn, unsigned long long *samples, hipStream_t st);

// pigs_vh.hip: the van Hove functions over the window slices (pigs_vh_accumulate): 64-bit counts per walker and lag,
// self [walker][Ntau + 1][Ns] and dist [walker][Ntau + 1][Nr].  k_vh, one workgroup per (listed walker, base slice), holds
// the base slice in LDS and walks the particles of the slices a + l against it.  A walker may be listed twice in one
// launch (integer atomics).  vh_shape decides the form: the histograms of all lags privatised in LDS as u32 (form 1, or
// automatic wherever 8 dim Np + 4 (Ntau + 1)(Nr + Ns) <= kVhLdsBudget), or global u64 atomics (form 0); the slice itself
// always sits in LDS, 8 dim Np <= kVhLdsBudget, which pigs_vh_init checks.  hist_lds && !hist_fits is a forced LDS form
// that does not fit, which the caller refuses.
constexpr int kVhThreads = 256;                  // a power of two (the owner rounds split by powers of two)
constexpr size_t kVhLdsBudget = 160 * 1024;      // LDS of one CU on gfx950
struct VhShape { int slice_fits, hist_fits, hist_lds; size_t lds; };
VhShape vh_shape(int dim, int Np, int Ntau, int Nr, int Ns, int form);
hipError_t launch_vh(const DevParams &P, const double *paths, int n, const WalkerList &list, const VhShape &s, int window,
                     int Ntau, int Nr, double rbin, int Ns, double sbin, unsigned long long *self, unsigned long long *dist,
                     unsigned long long *samples, hipStream_t st);

// pigs_g3.hip: the triplet distribution over the window slices (pigs_g3_accumulate): 64-bit counts per walker, trip
// [walker][Nr (Nr + 1) / 2][Na] and pair [walker][Nr].  k_g3, one workgroup of kG3Waves waves per (listed walker, slice),
// holds the slice in LDS; a wave owns a vertex, compacts its legs into a list of its own in LDS (capacity Np: a vertex
// has at most Np - 1 legs) and shares the pairs of legs among its lanes.  A walker may be listed twice in one launch
// (integer atomics).  g3_shape decides the form.  The slice and the lists always sit in LDS,
//   8 dim Np + kG3Waves Np (8 (dim + 1) + 4) <= kG3LdsBudget         (fits; pigs_g3_init checks it),
// and the counters are privatised beside them as u32 (form 1, or automatic) wherever
//   that + 4 (Nr (Nr + 1) / 2 Na + Nr) <= kG3LdsBudget   and   Np (Np - 1)(Np - 2) / 2 <= 2^32 - 1   (hist_fits),
// global u64 atomics otherwise (form 0).  hist_lds && !hist_fits is a forced LDS form that does not fit, which the
// caller refuses.
constexpr int kG3Waves = 4;
constexpr int kG3Threads = kG3Waves * 64;
constexpr int kG3GridMax = 1024;                 // Nr and Na at most
constexpr size_t kG3LdsBudget = 160 * 1024;      // LDS of one CU on gfx950
struct G3Shape { int fits, hist_fits, hist_lds, cap; size_t lds; };
G3Shape g3_shape(int dim, int Np, int Nr, int Na, int form);
hipError_t launch_g3(const DevParams &P, const double *paths, int n, const WalkerList &list, const G3Shape &s, int window,
                     int Nr, double rbin, int Na, unsigned long long *trip, unsigned long long *pair,
                     unsigned long long *samples, hipStream_t st);

// pigs_atm.hip: the Axilrod-Teller-Muto geometric sum over the window slices (pigs_atm_accumulate): per walker and slice
// a double T and a 64-bit count of the triplets within rc.  k_atm, one workgroup of kAtmWaves waves per (listed walker,
// slice), holds the slice in LDS; a wave owns a vertex i, compacts its legs j > i into a list of its own in LDS (capacity
// Np: a vertex has at most Np - 1 legs) and shares the pairs of legs among its lanes.  One thread owns an element (w, a)
// per launch: a walker must not be listed twice in ONE launch.  The slice, the lists and the reduction's tail always sit in
// LDS,
//   8 dim Np + kAtmWaves Np 8 (dim + 1) + kAtmLdsTail <= kAtmLdsBudget         (fits; pigs_atm_init checks it).
constexpr int kAtmWaves = 4;
constexpr int kAtmThreads = kAtmWaves * 64;
constexpr size_t kAtmLdsTail = 64;                // the waves' partial sums and counts
constexpr size_t kAtmLdsBudget = 160 * 1024;      // LDS of one CU on gfx950
struct AtmShape { int fits, cap; size_t lds; };
AtmShape atm_shape(int dim, int Np);
hipError_t launch_atm(const DevParams &P, const double *paths, int n, const WalkerList &list, const AtmShape &s, int window,
                      double rc2, double *T, unsigned long long *ntrip, unsigned long long *samples, hipStream_t st);

// pigs_nk.hip: the momentum distribution on the vectors of pigs_sqv_* and the one-body density matrix on the Cartesian grid
// of the minimum-image cell (pigs_nk_accumulate, pigs_nk_add).  k_nk, one workgroup of kNkThreads threads per listed walker,
// reads that walker's samples (once-folded end-to-end vectors) from a tape: cnt[j] samples (at most cap) at
// xs + j cap dim, j the walker (by_walker: the sampler's end tape) or base + the position in the list (pigs_nk_add).  Tiles of
// kNkTile samples are staged in LDS as per-axis phasor tables, nk_lds_bytes = 16 dim kNkTile (nmax + 1) <= kNkLdsBudget for
// every nmax that pigs_nk_init accepts.  A thread owns vectors and adds once to C [walker][Nq]; H [walker][nbin^dim],
// nopen and ninside [walker] are 64-bit counts.  One thread owns an element of C per launch: a walker must not be listed
// twice in ONE launch.
constexpr int kNkThreads = 256;
constexpr int kNkTile = 64;                      // samples staged per tile (PIGS_NK_TILE of include/pigs_hip.h)
constexpr size_t kNkLdsBudget = 160 * 1024;      // LDS of one CU on gfx950
size_t nk_lds_bytes(int dim, int nmax);
hipError_t launch_nk(const DevParams &P, int n, const WalkerList &list, int nmax, int nbin, long long Nq, int by_walker,
                     int base, int cap, const int *cnt, const double *xs, double *C, unsigned long long *H,
                     unsigned long long *nopen, unsigned long long *ninside, hipStream_t st);

// pigs_lat.hip: a crystal seen from its lattice over the window slices (pigs_lat_accumulate): the nearest site of every
// particle, the moments and histograms of its displacement from that site, the occupation of the sites and the hops
// between sites along imaginary time.  k_lat, one workgroup per (listed walker, slice), stages the site rows in LDS in
// tiles of kLatTile and leaves every particle's site in the scratch sidx [slot][2 window + 1][NpPad]; k_lat_hops, one
// workgroup per listed walker, reads it.  One thread owns an element (w, a) per launch: a walker must not be listed twice
// in ONE launch.  A site tile, u of the slice, the occupancy and the histograms always sit in LDS,
//   8 (dim kLatTile + dim Np + 4 + 8 kLatThreads/64) + 4 (nsite + (1 + 2 dim) nbin + 8) <= kLatLdsBudget
// (fits; pigs_lat_init checks it), within what a kernel may ask for without a grant.
constexpr int kLatThreads = 256;
constexpr int kLatTile = 256;
constexpr size_t kLatLdsBudget = 64 * 1024;
struct LatShape { int fits; size_t lds; };
LatShape lat_shape(int dim, int Np, int nsite, int nbin);
hipError_t launch_lat(const DevParams &P, const double *paths, int n, const WalkerList &list, const LatShape &s, int window,
                      int cm, int nsite, int NsPad, const double *sites, int nbin, double rmax, double *mom,
                      unsigned long long *nassigned, unsigned long long *nlost, unsigned long long *occ,
                      unsigned long long *hr, unsigned long long *hx, unsigned long long *hop1, unsigned long long *hopw,
                      unsigned long long *samples, int *sidx, hipStream_t st);

// pigs_sf.hip: the diffusion of the centre of mass along imaginary time and the unfolded displacement of a particle
// (pigs_sf_accumulate).  k_sf_links, one workgroup per listed walker, folds every link of the window once, adds the
// folded links up and leaves the unfolded coordinates in the scratch U [slot][2 window + 1][dim][NpPad] and the unfolded
// centre of mass (times Np) in Wcm [slot][2 window + 1][dim]; k_sf_lags, one workgroup per (listed walker, lag), reads
// both.  One thread owns an element (w, l, k) per launch: a walker must not be listed twice in ONE launch.  A slot of U
// takes sf_slot_doubles doubles; pigs_sf_init sizes the scratch (at most kSfScratchMiB MiB by default, one slot at the
// least) and pigs_sf_accumulate cuts its launches to the slots there are.  Static LDS only.
constexpr int kSfThreads = 256;
constexpr int kSfScratchMiB = 256;
constexpr int kSfLagsMax = 3072;
size_t sf_slot_doubles(int dim, int NpPad, int window);
hipError_t launch_sf(const DevParams &P, const double *paths, int n, const WalkerList &list, int window, int Ntau, double *U,
                     double *Wcm, double *C, double *D, unsigned long long *nwrap, unsigned long long *samples,
                     hipStream_t st);

// pigs_cl.hip: the cluster-size distribution over the window slices (pigs_cl_accumulate).  k_cl, one workgroup per (listed
// walker, slice) with the slice in LDS, labels the connected components of the bond graph 0 < r2 < rc2 by hook and
// pointer jump until a sweep changes nothing, adds the sizes to nsize and the largest to nlarge ([walker][Np]), the bonds
// to nbond and 1 per slice to samples (integer atomics), and writes the slice's sums of g per size to scratch
// ([slot][slice][Np]); k_cl_combine adds the slices in ascending order to rg2 ([walker][Np]).  One thread owns an element
// of rg2 per launch: the caller never lists a walker twice in ONE launch.  Up to kClAdjNpMax particles the bonds are kept
// as bit rows in LDS beside the slice (Np^2/8 bytes: 8 KB at 256, under the 64 KB that need no grant); beyond, every sweep
// computes the distances again.  kClNpMax: the u32 counters and the slice, labels and sums in LDS (cl_lds_bytes, which has
// to fit kClLdsBudget).  A slot of the scratch takes cl_slot_doubles doubles; pigs_cl_init sizes it (kClScratchMiB MiB by
// default, one slot at the least) and pigs_cl_accumulate cuts its launches to the slots there are.  sweeps (may be null):
// the largest number of labelling sweeps of any workgroup so far.
constexpr int kClThreads = 256;
constexpr int kClAdjNpMax = 256;
constexpr int kClNpMax = 2048;
constexpr int kClScratchMiB = 256;
constexpr size_t kClLdsBudget = 160 * 1024;      // LDS of one CU on gfx950
size_t cl_lds_bytes(int dim, int Np);
size_t cl_slot_doubles(int Np, int window);
hipError_t launch_cl(const DevParams &P, const double *paths, int n, const WalkerList &list, int window, double rc2,
                     double *scratch, unsigned long long *nsize, unsigned long long *nlarge, unsigned long long *nbond,
                     unsigned long long *samples, double *rg2, unsigned int *sweeps, hipStream_t st);
// k_cl_combine alone: dst[walker][Np] += scratch[slot][slice][Np], slices ascending (pigs_pc.hip ends its launch with it too)
hipError_t launch_cl_combine(const WalkerList &list, int n, int ns, int Np, const double *scratch, double *dst, hipStream_t st);

// pigs_pc.hip: wrapping clusters, the unfolded extent of the finite ones and the persistence of clusters along tau
// (pigs_pc_accumulate).  k_pc has k_cl's shape, limits (kClThreads, kClAdjNpMax, kClNpMax, kClLdsBudget) and labelling loop
// (pigs_cl_device.h); after the labels it spreads image numbers from every root over the bonds until a sweep assigns
// nobody, takes the wrap mask of every cluster from the bonds that the image numbers do not explain, counts clusters and
// particles per mask (nwrap, mwrap: [walker][8]), slices per OR of their masks (swrap: [walker][8]), the finite clusters
// per size (nfin: [walker][Np]) and the slices (samples), and writes the finite clusters' sums of g per size, from
// unfolded separations, to scratch and the labels to `labels` (both [slot][slice][Np]).  k_cl_combine adds the slices to
// rg2u ([walker][Np]); k_pc_persist, one workgroup per (slot, origin), counts the pairs together in slice a, in a + l
// and in both for l = 0..ntau (first, second, both, norig: [walker][ntau + 1]).  One thread owns an element of rg2u per
// launch: the caller never lists a walker twice in ONE launch.  A slot of the two scratches takes pc_slot_bytes bytes.
// sweeps: two counters, the largest number of labelling and of image sweeps of any workgroup so far.
constexpr int kPcScratchMiB = 256;
struct PcSums {
    unsigned long long *nwrap, *mwrap, *swrap, *nfin, *samples, *first, *second, *both, *norig;
    double *rg2u;
};
size_t pc_lds_bytes(int dim, int Np);
size_t pc_slot_bytes(int Np, int window);
hipError_t launch_pc(const DevParams &P, const double *paths, int n, const WalkerList &list, int window, int ntau, double rc2,
                     double *scratch, int *labels, const PcSums &s, unsigned int *sweeps, hipStream_t st);

hipError_t launch_commit_beads(const DevParams &P, double *paths, int64_t n, const int32_t *walker,
                               const int32_t *ip, const int32_t *ib, const double *x, hipStream_t st);

hipError_t launch_swap_tails(const DevParams &P, double *paths, int walker, int iw, int ik,
                             hipStream_t st);

// K6: device-resident sampler (pigs_sampler.hip)
// per-walker generator state in global memory: 624 sliding words, 624 block-form words, position
constexpr int kRngWords = 2 * 624 + 1;
constexpr int kCounters = 16;       // per-walker move counters (pigs_sampler.hip)
constexpr int kWormDoubles = 8;     // isopen, iworm, xend(:,1), xend(:,2)
constexpr int kEvInts = 64;         // event log of one MC step: at least this many ints per walker (SweepParams.ev_ints)
struct SweepParams {
    int32_t Nlev, Nstag, Lstag, do_cm;
    int32_t open_attempt, parts, worm, swapping;  // worm: CWorm > 0 (open/close/swap sector sampled); parts: sections of the
                                                  // step a launch runs (1 open/close attempt, 2 diagonal moves, 4 worm moves)
    int32_t Nobdm, Nbin, Npw, staging;            // staging: sampling = 'sta' in the diagonal sector
    int32_t ev_ints, cm_fault;                    // ints per walker of the event log: max(kEvInts, 4 + 2*(1+Nobdm)); cm_fault: TEST
                                                  // ONLY (tuning key "cm_fault"): the last range of every walker in k_cm withholds
                                                  // its Delta S and waiting workgroups give up after 2048 polls (forces the time-out path)
    double  delta_cm, log_cworm_density, rbin;
    // the end tape (null: none): per walker and step, tape_count[w] = Nobdm if the worm loop ran, 0 otherwise, and
    // tape_x[w][iobdm][dim] the once-folded end-to-end vector that the OBDM histogram of iteration iobdm took (pigs_nk_*)
    int32_t *tape_count;
    double  *tape_x;
};
hipError_t launch_sweep(const DevParams &P, const SweepParams &sp, int threads, double *paths, const double *VT,
                        const double *VTimg, const double *WF, uint32_t *rng, unsigned long long *counters, double *worm,
                        int *evlog, double *nrho, const double *dklog, hipStream_t st);
hipError_t launch_slice_gather(const DevParams &P, const double *paths, int ib, double *out, hipStream_t st);
size_t sweep_lds_bytes(const DevParams &P, const SweepParams &sp, int threads);
// pigs_diag.hip: the diagonal moves of a periodic system with sampling = 'bis' as a stage machine (one workgroup per walker)
bool diag_supported(const DevParams &P, const SweepParams &sp);
int diag_form(const DevParams &P, const SweepParams &sp, int threads);      // workgroup size launch_diag uses (0: does not fit)
hipError_t launch_diag(const DevParams &P, const SweepParams &sp, int threads, double *paths, const double *VTimg,
                       const double *WF, uint32_t *rng, unsigned long long *counters, const double *worm, hipStream_t st);
// pigs_cm.hip: the TranslateChain moves of a periodic system by H cooperating workgroups per walker
int cm_helpers(const DevParams &P, const SweepParams &sp, int n_cu);        // H the chip and the kernel allow (0: none)
bool cm_fits(const DevParams &P, int H);                                    // the kernel fits with exactly H workgroups per walker
size_t cm_exchange_words(const DevParams &P);                               // 64-bit words of the exchange buffer
hipError_t launch_cm(const DevParams &P, const SweepParams &sp, int H, unsigned int seq0, double *paths, const double *VTimg,
                     const double *WF, uint32_t *rng, unsigned long long *counters, const double *worm,
                     unsigned long long *xch, int *err, hipStream_t st);
int sweep_form(const DevParams &P, const SweepParams &sp, int threads);   // workgroup size launch_sweep uses for a request

hipError_t launch_stream_read(const double *a, size_t doubles, int blocks, double *sink, hipStream_t st);
// argument `idx` of the log self-test (pigs_selftest_log): the device sampler's domain -- a uniform of the stream
// k/(2^32-1); a polar radius u1^2+u2^2 <= 1 of two such uniforms; a random mantissa over 2^-69 .. 2; the near-one branch
__host__ __device__ inline double selftest_log_arg(unsigned long long idx, unsigned long long seed)
{
    unsigned long long z = (idx + 1) * 0x9E3779B97F4A7C15ull + seed;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    unsigned long long y = (z + 0x632BE59BD9B4E019ull) * 0xD1342543DE82EF95ull; y ^= y >> 29;
    const double ua = (double)(unsigned int)z / 4294967295.0, ub = (double)(unsigned int)y / 4294967295.0;
    switch (idx & 3) {
    case 0: return ua;
    case 1: { const double u1 = 2.0 * ua - 1.0, u2 = 2.0 * ub - 1.0; const double q = u1 * u1 + u2 * u2; return q > 1.0 ? q - 1.0 : q; }
    case 2: { const unsigned long long ix = (z >> 12) | ((unsigned long long)(0x3ff - (y % 70)) << 52);
              double x; __builtin_memcpy(&x, &ix, 8); return x; }
    default: return 0.9375 + (double)(z >> 11) * (1.0 / 9007199254740992.0) * 0.13;
    }
}
hipError_t launch_selftest_log(unsigned long long first, unsigned long long n, unsigned long long seed, double *d_out, hipStream_t st);
hipError_t launch_selftest_fastmath(const DevParams &P, unsigned long long seed, int blocks, int iters,
                                    unsigned long long *d_bad, hipStream_t st);

hipError_t launch_pack(const DevParams &P, double *paths, const double *raw, int w0, int nw,
                       hipStream_t st);
hipError_t launch_unpack(const DevParams &P, const double *paths, double *raw, int w0, int nw,
                         hipStream_t st);

} // namespace pigs
