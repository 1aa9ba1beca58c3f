// pigs_capi.hip -- the C ABI of include/pigs_hip.h over the gfx950 kernels.
//
// A context owns one device, one stream, the resident worldlines of its walkers (SoA
// layout of pigs_device.h), both tables, and grow-only scratch buffers; nothing is
// allocated inside the *_dev / launch paths (graph-capture safe).  There is NO CPU
// fallback anywhere in this library: without a HIP device every call fails loudly.
#include "../../include/pigs_hip.h"

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <utility>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <unordered_set>
#include <atomic>
#include <vector>
#include <thread>
#include <algorithm>

#include "pigs_comm.h"
#include "pigs_kernels.h"
#include "pigs_launch.h"

using namespace pigs;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(expr)                                                                     \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess)                                                            \
            return fail(PIGS_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_),    \
                        __FILE__, __LINE__);                                             \
    } while (0)

// Device memory owned by its holder (move-only): `alloc` for the fixed arrays, `reserve` for the grow-only scratch.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    ~DevBuf() { release(); }
    // exactly n elements: a no-op at that size already, otherwise the old contents are dropped
    hipError_t alloc(size_t n)
    {
        if (p && n == cap) return hipSuccess;
        release();
        hipError_t e = hipMalloc((void **)&p, n * sizeof(T));
        if (e == hipSuccess) cap = n; else p = nullptr;
        return e;
    }
    hipError_t reserve(size_t n) { return n <= cap ? hipSuccess : alloc(n + n / 4 + 64); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// pinned, device-mapped host arrays (move-only): the staged (low-latency) entry points, the estimators' result block
struct PinBuf {
    void *h = nullptr, *d = nullptr;
    size_t bytes = 0;
    PinBuf() = default;
    PinBuf(PinBuf &&o) noexcept : h(std::exchange(o.h, nullptr)), d(std::exchange(o.d, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    ~PinBuf() { if (h) (void)hipHostFree(h); }
    hipError_t reserve(size_t want, size_t keep_bytes = 0)
    {
        if (want <= bytes) return hipSuccess;
        void *nh = nullptr, *nd = nullptr;
        hipError_t e = hipHostMalloc(&nh, want, hipHostMallocMapped);
        if (e != hipSuccess) return e;
        e = hipHostGetDevicePointer(&nd, nh, 0);
        if (e != hipSuccess) { (void)hipHostFree(nh); return e; }
        if (h && keep_bytes) memcpy(nh, h, keep_bytes < bytes ? keep_bytes : bytes);
        if (h) (void)hipHostFree(h);
        h = nh; d = nd; bytes = want;
        return hipSuccess;
    }
};

// a stream, event or communicator handle destroyed by its holder (move-only)
template <typename H, auto Destroy>
struct Handle {
    H h = nullptr;
    Handle() = default;
    Handle(Handle &&o) noexcept : h(std::exchange(o.h, nullptr)) {}
    ~Handle() { reset(); }
    void reset() { if (h) (void)Destroy(h); h = nullptr; }
    operator H() const { return h; }
};
using Stream = Handle<hipStream_t, hipStreamDestroy>;
using Event  = Handle<hipEvent_t, hipEventDestroy>;
using Comm   = Handle<pigs_comm *, pigs_comm_destroy>;

// One batch of the diagonal estimators (pigs_diagonal_estimators and its overlapped form) for n walkers, validated.
// Slot lists: [0, nslot) the ThermEnergy slices 0..2Nb-1 (Q8) of every walker, [nslot, nslot + n) the walkers themselves
// (K4, K7).  Result block (nres doubles): [LocalEnergy slice 0: 3n][LocalEnergy slice 2Nb: 3n][E n][Ec n][Ep n][gr][Sk].
struct EstBatch {
    int n = 0, Nbin = 0, Nk = 0;
    double rbin = 0.0;
    bool structure = false;
    size_t ns = 0, nslot = 0, ng = 0, nk = 0, nres = 0;
    std::vector<int32_t> w;                 // the walkers
};

// the device buffers a batch runs in: slot lists, ThermEnergy slices, result block
struct EstBufs {
    DevBuf<int32_t> slotw, slotb;
    DevBuf<double>  slices, res;
    hipError_t reserve(const EstBatch &b)
    {
        hipError_t e = slotw.reserve(b.nslot + b.n);
        if (e == hipSuccess) e = slotb.reserve(b.nslot);
        if (e == hipSuccess) e = slices.reserve(b.nslot * 3);
        if (e == hipSuccess) e = res.reserve(b.nres);
        return e;
    }
};

} // namespace

// several contexts of one process meeting in host memory (pigs_comm_init_all on duplicate devices: rehearsal only)
struct HostGroup {
    int n = 0, arrived = 0, generation = 0;
    std::mutex m;
    std::condition_variable cv;
    std::vector<std::vector<double>> slot;
    std::vector<double> sum;
};

struct pigs_ctx {
    pigs_params hp;
    DevParams   P;
    int         device    = 0;
    int         n_walkers = 0;
    Stream      stream;
    DevBuf<double> d_paths, d_VT, d_WF;
    std::shared_ptr<HostGroup> hgroup;   // rehearsal form of the estimator reduction (several contexts on one GPU)
    int hrank = 0;
    DevBuf<double> d_VTimg;              // [0, VT(0)] VT(0..Nmax+1) [0 0 0 0]: PipeTab image for the sampler (pigs_k1_device.h)
    size_t  path_doubles = 0;        // resident doubles per walker (padded SoA)
    size_t  raw_doubles  = 0;        // dim*Np*(2Nb+1): reference layout per walker
    DevBuf<int32_t> d_walker, d_ip, d_ib;
    DevBuf<double>  d_xnew, d_xold, d_out, d_parts, d_stage;
    EstBufs     est;                         // estimators on the context's stream (also the scratch of K2/K3, K4, K7 alone)
    Comm        comm;
    int         k1_variant = K1_AUTO;
    PinBuf      st_w, st_ip, st_ib, st_xn, st_xo, st_out;      // staged items
    PinBuf      cs_w, cs_ip, cs_ib, cs_x;                      // staged commits
    int64_t     st_cap = 0, cs_cap = 0;
    // device-resident sampler
    DevBuf<uint32_t> d_rng;
    DevBuf<unsigned long long> d_counters;
    DevBuf<double> d_worm, d_nrho, d_dklog;
    DevBuf<int> d_evlog;
    size_t      nrho_doubles = 0;
    SweepParams sweep{};
    int         cm_freq = 1;
    int         sweep_threads = 512;
    bool        sweep_split = false;    // diagonal moves of periodic 'bis' systems in pigs_diag.hip's kernel (see pigs_sampler_step)
    int         n_cu = 256;
    // TranslateChain by several workgroups per walker (pigs_cm.hip): -1 as many as fit (default), 0 off, H >= 1 at most H
    int         cm_split = -1;
    bool        cm_exclusive = false;       // the caller vouches that no other context's kernels run on this device meanwhile
    bool        cm_shared = false;          // several contexts of this process sample on this device at once: see g_cm_gate
    DevBuf<unsigned long long> d_xch;       // exchange buffer of the cooperating workgroups
    PinBuf      h_cm_err;                   // (one int) set by a workgroup whose partner never answered
    unsigned int cm_seq = 1;                // sequence tags of the exchange: advanced by every launch
    int         form_cm = -1;               // H of the last step's TranslateChain (0: inside the sweep kernel): pigs_sampler_form
    bool        form_diag = false;          // the last step ran the stage-machine kernel
    bool        sampler_ready = false;
    // asynchronous estimators (pigs_diagonal_estimators_begin / _end): a snapshot of the worldlines and a second stream
    Stream      stream2;
    Event       ev_snap;
    DevBuf<double> d_shadow;
    EstBufs     a_buf;
    PinBuf      a_host;                     // results land here (pinned: the copy is truly asynchronous)
    std::vector<int32_t> a_sw, a_sb;        // slot lists: must outlive the asynchronous upload
    struct { bool on = false, launched = false; EstBatch b; } a_pend;
    Event       ev_gate;                    // recorded behind the TranslateChain kernel of the next step (see launch_pending_estimators)
    // the launches of the accumulator families below (each_launch): which walkers the current one holds
    WalkerMarks list_marks;
    // density profiles of a trapped system (pigs_density_*): per-walker 64-bit counts, walker-major
    DevBuf<unsigned long long> d_dplanar, d_dradial, d_dpair, d_dsamples;
    int         dens_nbin = 0;              // 0: pigs_density_init not called yet
    size_t      dens_nplanar = 0;           // planar bins per walker: Nbin^min(dim,2)
    double      dens_h = 0.0, dens_b = 0.0, dens_br = 0.0;
    // imaginary-time density correlations of a periodic system (pigs_fqt_*): raw sums [walker][l][iq][k], the samples per
    // walker, and the C/S scratch of one launch's window slices ([fqt_slots][2 window + 1][Nk dim][2])
    DevBuf<double> d_fqt_acc, d_fqt_rho;
    DevBuf<unsigned long long> d_fqt_samples;
    int         fqt_nk = 0;                 // 0: pigs_fqt_init not called yet
    int         fqt_ntau = 0, fqt_window = 0, fqt_slots = 0;
    // vector structure factor on the full reciprocal grid (pigs_sqv_*): raw sums [walker][iqv], the samples per walker,
    // and the C^2 + S^2 scratch of one launch's window slices ([sqv_slots][2 window + 1][Nq])
    DevBuf<double> d_sqv_acc, d_sqv_rho2;
    DevBuf<unsigned long long> d_sqv_samples;
    int         sqv_nmax = 0;               // 0: pigs_sqv_init not called yet
    int         sqv_window = 0, sqv_slots = 0;
    int64_t     sqv_nq = 0;
    // F(q,tau) on the vectors of pigs_sqv_* (pigs_fqv_*): raw sums [walker][l][iqv], the samples per walker, and the
    // (C, S) scratch of one launch's window slices ([fqv_slots][2 window + 1][Nq][2])
    DevBuf<double> d_fqv_acc, d_fqv_rho;
    DevBuf<unsigned long long> d_fqv_samples;
    int         fqv_nmax = 0;               // 0: pigs_fqv_init not called yet
    int         fqv_ntau = 0, fqv_window = 0, fqv_slots = 0;
    int64_t     fqv_nq = 0;
    // self part of F(q,tau) and the imaginary-time displacement (pigs_fqs_*): raw sums F [walker][l][iqv] and
    // D [walker][l][2], the samples per walker; no scratch (pigs_fqs.hip keeps the phasors in LDS)
    DevBuf<double> d_fqs_acc, d_fqs_dsp;
    DevBuf<unsigned long long> d_fqs_samples;
    int         fqs_nmax = 0;               // 0: pigs_fqs_init not called yet
    int         fqs_ntau = 0, fqs_window = 0;
    int64_t     fqs_nq = 0;
    // pair distribution on the vector grid over a slice window (pigs_grv_*): per-walker 64-bit counts, walker-major
    DevBuf<unsigned long long> d_grv_vec, d_grv_radial, d_grv_samples;
    int         grv_nbin = 0;               // 0: pigs_grv_init not called yet
    int         grv_nr = 0, grv_window = 0;
    int         grv_form = -1;              // tuning key "grv_form": -1 automatic, 0 global atomics, 1 grid privatised in LDS
    size_t      grv_nvec = 0;               // vector bins per walker: Nbin^dim
    double      grv_rbin = 0.0;
    // imaginary-time profiles (pigs_tau_*): raw sums [walker][2Nb+1][4] and the samples per walker
    DevBuf<double> d_tau_acc;
    DevBuf<unsigned long long> d_tau_samples;
    bool        tau_ready = false;          // pigs_tau_init called
    // bond-orientational order over a slice window (pigs_bop_*): raw sums S [walker][8] and G [walker][Nr], the counts
    // H [walker][2][Nh] and GN [walker][Nr], the samples per walker, and the scratch of one launch's window slices
    // ([bop_slots][2 window + 1][8 + Nr])
    DevBuf<double> d_bop_S, d_bop_G, d_bop_scratch;
    DevBuf<unsigned long long> d_bop_H, d_bop_GN, d_bop_samples;
    int         bop_nh = 0;                 // 0: pigs_bop_init not called yet
    int         bop_nr = 0, bop_window = 0, bop_slots = 0;
    double      bop_rnb2 = 0.0, bop_rbin = 0.0;
    // van Hove functions over a slice window (pigs_vh_*): per-walker 64-bit counts, self [walker][Ntau+1][Ns] and dist
    // [walker][Ntau+1][Nr], and the samples per walker
    DevBuf<unsigned long long> d_vh_self, d_vh_dist, d_vh_samples;
    int         vh_nr = 0;                  // 0: pigs_vh_init not called yet
    int         vh_ns = 0, vh_ntau = 0, vh_window = 0;
    int         vh_form = -1;               // tuning key "vh_form": -1 automatic, 0 global atomics, 1 histograms privatised in LDS
    double      vh_rbin = 0.0, vh_sbin = 0.0;
    // triplet distribution over a slice window (pigs_g3_*): per-walker 64-bit counts, trip [walker][Nr (Nr + 1) / 2][Na] and
    // pair [walker][Nr], and the samples per walker
    DevBuf<unsigned long long> d_g3_trip, d_g3_pair, d_g3_samples;
    int         g3_nr = 0;                  // 0: pigs_g3_init not called yet
    int         g3_na = 0, g3_window = 0;
    int         g3_form = -1;               // tuning key "g3_form": -1 automatic, 0 global atomics, 1 counters privatised in LDS
    double      g3_rbin = 0.0;
    // Axilrod-Teller-Muto geometric sum over a slice window (pigs_atm_*): raw sums T [walker][2 window + 1], the triplets
    // counted ntrip [walker][2 window + 1], and the samples per walker
    DevBuf<double> d_atm_T;
    DevBuf<unsigned long long> d_atm_ntrip, d_atm_samples;
    bool        atm_ready = false;          // pigs_atm_init called
    int         atm_window = 0;
    double      atm_rc2 = 0.0;
    // the sampler's end tape (periodic context, CWorm > 0): per walker the samples of the last step and their once-folded
    // end-to-end vectors [walker][Nobdm][dim] (SweepParams.tape_count, tape_x)
    DevBuf<int32_t> d_tape_count;
    DevBuf<double>  d_tape_x;
    // momentum distribution and one-body density matrix (pigs_nk_*): cosine sums C [walker][Nq], counts H [walker][nbin^dim],
    // nopen and ninside [walker]; the samples that pigs_nk_add brings from the host ([position][cap][dim] and their numbers)
    DevBuf<double> d_nk_C, d_nk_x;
    DevBuf<unsigned long long> d_nk_H, d_nk_nopen, d_nk_ninside;
    DevBuf<int32_t> d_nk_cnt;
    int         nk_nmax = 0;                // 0: pigs_nk_init not called yet
    int         nk_nbin = 0;
    int64_t     nk_nq = 0;
    size_t      nk_nvec = 0;
    // a crystal seen from its lattice (pigs_lat_*): the site rows [dim][NsPad], per walker the moments
    // mom [2 window + 1][2 + dim], nassigned [2 window + 1], occ [2 window + 1][4], hr [nbin], hx [dim][2 nbin], nlost, hop1,
    // hopw and samples; the assigned sites of one launch, sidx [min(n_walkers, 256)][2 window + 1][NpPad]
    DevBuf<double> d_lat_sites, d_lat_mom;
    DevBuf<unsigned long long> d_lat_nass, d_lat_nlost, d_lat_occ, d_lat_hr, d_lat_hx, d_lat_hop1, d_lat_hopw, d_lat_samples;
    DevBuf<int32_t> d_lat_sidx;
    bool        lat_ready = false;          // pigs_lat_init called
    int         lat_nsite = 0, lat_nspad = 0, lat_nbin = 0, lat_window = 0, lat_cm = 0;
    double      lat_rmax = 0.0;
    // centre-of-mass diffusion along tau (pigs_sf_*): per walker C and D [Ntau + 1][dim], nwrap and samples; the unfolded
    // coordinates of one launch, U [sf_slots][2 window + 1][dim][NpPad], and its centre of mass Wcm [sf_slots][2 window + 1][dim]
    DevBuf<double> d_sf_C, d_sf_D, d_sf_U, d_sf_W;
    DevBuf<unsigned long long> d_sf_nwrap, d_sf_samples;
    bool        sf_ready = false;           // pigs_sf_init called
    int         sf_ntau = 0, sf_window = 0;
    int         sf_slots = 0;               // walkers per launch: what the scratch holds
    int         sf_scratch_mib = kSfScratchMiB;   // pigs_set_tuning "sf_scratch_mib": the budget of U at the next pigs_sf_init
    // cluster-size distribution over a slice window (pigs_cl_*): per walker nsize, nlarge and rg2 [Np], nbond and samples;
    // the per-slice sums of g per size of one launch ([cl_slots][2 window + 1][Np]); the largest sweep count so far
    DevBuf<unsigned long long> d_cl_nsize, d_cl_nlarge, d_cl_nbond, d_cl_samples;
    DevBuf<double> d_cl_rg2, d_cl_scratch;
    DevBuf<unsigned int> d_cl_sweeps;
    bool        cl_ready = false;           // pigs_cl_init called
    int         cl_window = 0;
    int         cl_slots = 0;               // walkers per launch: what the scratch holds
    double      cl_rc2 = 0.0;
    int         cl_scratch_mib = kClScratchMiB;   // pigs_set_tuning "cl_scratch_mib": the budget of the scratch at the next pigs_cl_init
    // wrapping clusters and cluster persistence over a slice window (pigs_pc_*): per walker nwrap, mwrap, swrap [8], nfin and
    // rg2u [Np], samples, and first, second, both, norig [ntau + 1]; the per-slice sums of g and the labels of one launch
    // ([pc_slots][2 window + 1][Np] each); the largest labelling and image sweep counts so far
    DevBuf<unsigned long long> d_pc_nwrap, d_pc_mwrap, d_pc_swrap, d_pc_nfin, d_pc_samples, d_pc_first, d_pc_second, d_pc_both,
                               d_pc_norig;
    DevBuf<double> d_pc_rg2u, d_pc_scratch;
    DevBuf<int> d_pc_labels;
    DevBuf<unsigned int> d_pc_sweeps;
    bool        pc_ready = false;           // pigs_pc_init called
    int         pc_window = 0, pc_ntau = 0;
    int         pc_slots = 0;               // walkers per launch: what the two scratches hold
    double      pc_rc2 = 0.0;
    int         pc_scratch_mib = kPcScratchMiB;   // pigs_set_tuning "pc_scratch_mib": the budget of the scratches at the next pigs_pc_init
};

// live contexts per device of this process: the TranslateChain helpers (pigs_cm.hip) assume that the walkers of ONE
// context have the chip to themselves
static std::atomic<int> g_live_ctx[64];
static std::atomic<int> g_ctx_serial[64];   // contexts ever created per device (stream priority: see pigs_ctx_create)

// Several sampling contexts on ONE device (walker shards of the front end with `same_device`, tuning key "cm_shared"): the
// TranslateChain kernels of all of them are chained through one event per device, so that never two of them run at once --
// their workgroups wait for each other and must all be resident; next to the OTHER contexts' sweep kernels (one CU per
// walker, finite) they are, as long as H x walkers of the launching context + the walkers of the others <= CUs (the caller
// sets "cm_split" accordingly: 2 contexts x 64 walkers on 256 CUs -> H = 3).  The effect is a staggered schedule: one
// shard's TranslateChain on the CUs the other shard's bisection phase leaves idle.
static std::mutex g_cm_mutex[64];
static hipEvent_t g_cm_gate[64];

static int check_ctx(pigs_ctx *c)
{
    if (!c) return fail(PIGS_ERR_ARG, "null context");
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return fail(PIGS_ERR_HIP, "hipSetDevice(%d): %s", c->device, hipGetErrorString(e));
    return PIGS_OK;
}

// A commit list is a SEQUENCE of assignments Path(:,ip,ib) = x (the caller's program order): when a bead appears more than
// once the last value must win, as it does in the reference's sequential code.  The kernel writes all entries in
// parallel, so earlier duplicates are marked here (walker = -1: the kernel skips them).  Found by the sharded front end
// test: a worm's bead Nb is re-selected (xend(:,1) / xend(:,2)) between half-chain moves and could be queued twice
// before one flush.
static void mark_superseded(int64_t n, int32_t *w, const int32_t *ip, const int32_t *ib, int M, int Np)
{
    if (n < 2) return;
    std::unordered_set<uint64_t> seen;
    seen.reserve((size_t)n * 2);
    for (int64_t i = n - 1; i >= 0; --i) {
        const uint64_t key = ((uint64_t)(uint32_t)w[i] * (uint64_t)M + (uint64_t)ib[i]) * (uint64_t)(Np + 1) + (uint64_t)ip[i];
        if (!seen.insert(key).second) w[i] = -1;
    }
}

extern "C" {

const char *pigs_last_error(void) { return g_err; }
int pigs_abi_version(void) { return PIGS_ABI_VERSION; }

int pigs_device_count(int32_t *n)
{
    if (!n) return fail(PIGS_ERR_ARG, "null pointer");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *n = 0; return fail(PIGS_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *n = c;
    return PIGS_OK;
}

int pigs_ctx_create(const pigs_params *p, const double *VTable, const double *LogWF,
                    int32_t n_walkers, int32_t device_id, pigs_ctx **out)
{
    if (!p || !out) return fail(PIGS_ERR_ARG, "null pointer");
    *out = nullptr;
    if (p->dim < 1 || p->dim > PIGS_MAXDIM) return fail(PIGS_ERR_ARG, "dim=%d not in 1..3", p->dim);
    if (p->Np < 2 || p->Nb < 1 || p->Nmax < 4 || n_walkers < 1)
        return fail(PIGS_ERR_ARG, "bad sizes Np=%d Nb=%d Nmax=%d n_walkers=%d", p->Np, p->Nb, p->Nmax, n_walkers);
    if (!(p->dr > 0.0) || !(p->dt > 0.0)) return fail(PIGS_ERR_ARG, "dr and dt must be positive");
    // Reference quirk Q3: Force() is an empty stub, so the analytic (table-less) branch is
    // unusable for the force terms; and the kernels consume tables only.
    if (!p->v_table || !VTable) return fail(PIGS_ERR_UNSUPPORTED, "v_table=T with a VTable is mandatory (reference Force() is a stub)");
    // wf_table = F (the reference's default): the trial function is evaluated analytically (McMillan, pigs_device.h
    // log_psi) and LogWF may be null
    if (p->wf_table && !LogWF) return fail(PIGS_ERR_ARG, "wf_table=T needs a LogWF table");

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(PIGS_ERR_NO_DEVICE, "no HIP device visible (%s); libpigs_hip has no CPU fallback",
                    e == hipSuccess ? "count=0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= ndev) return fail(PIGS_ERR_ARG, "device_id=%d of %d", device_id, ndev);
    HIPCHK(hipSetDevice(device_id));

    std::unique_ptr<pigs_ctx> c(new (std::nothrow) pigs_ctx());
    if (!c) return fail(PIGS_ERR_ARG, "out of host memory");
    c->hp = *p;
    c->device = device_id;
    if (const char *ev = getenv("PIGS_K1_VARIANT")) {           // test / tuning hook: same as pigs_set_tuning("k1_variant")
        const int v = atoi(ev);
        if (k1_variant_valid(v)) c->k1_variant = v;
    }
    c->n_walkers = n_walkers;
    DevParams &P = c->P;
    memset(&P, 0, sizeof P);
    P.dim = p->dim; P.Np = p->Np; P.Nb = p->Nb; P.M = 2 * p->Nb + 1; P.Nmax = p->Nmax;
    P.NpPad = (p->Np + 7) & ~7;
    P.trap = p->trap; P.wf_table = p->wf_table; P.v_table = p->v_table; P.nW = n_walkers;
    P.dr = p->dr; P.rcut2 = p->rcut2; P.dt = p->dt; P.Rm = p->Rm;
    P.rdr = 1.0 / p->dr;                               // correctly rounded reciprocal (div_by)
    P.hrdr = 0.5 * P.rdr;
    for (int k = 0; k < 3; ++k) {
        P.Lbox[k]     = k < p->dim ? p->Lbox[k] : 1.0;
        P.LboxHalf[k] = 0.5 * P.Lbox[k];                 // vpi.f90:118
        P.rLbox[k]    = 1.0 / P.Lbox[k];
        P.a_ho[k]     = k < p->dim ? p->a_ho[k] : 1.0;
    }
    c->path_doubles = slice_doubles(P.dim, P.NpPad) * P.M;
    c->raw_doubles  = (size_t)P.dim * P.Np * P.M;

    {
        // Contexts on one device alternate between the normal and the high stream priority: the runtime maps streams onto
        // a few hardware queues PER PRIORITY (GPU_MAX_HW_QUEUES = 4 by default, shared with every other stream of the
        // process), and two sampling shards whose streams land on one hardware queue run one after the other instead of
        // side by side (round 3: bench.py's two-shard leg at 77 instead of 38.5 ms per MC step).  Different priorities
        // are different queues for certain; with CUs to spare the priority itself decides nothing.
        int least = 0, greatest = 0;
        const int serial = g_ctx_serial[device_id & 63].fetch_add(1);
        if ((serial & 1) && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && greatest != least)
            HIPCHK(hipStreamCreateWithPriority(&c->stream.h, hipStreamNonBlocking, greatest));
        else
            HIPCHK(hipStreamCreateWithFlags(&c->stream.h, hipStreamNonBlocking));
    }
    const size_t nt = (size_t)p->Nmax + 2, tb = nt * sizeof(double), np = c->path_doubles * n_walkers;
    HIPCHK(c->d_VT.alloc(nt));
    HIPCHK(c->d_WF.alloc(nt));
    HIPCHK(c->d_paths.alloc(np));
    HIPCHK(hipMemcpy(c->d_VT.p, VTable, tb, hipMemcpyHostToDevice));
    HIPCHK(LogWF && p->wf_table ? hipMemcpy(c->d_WF.p, LogWF, tb, hipMemcpyHostToDevice) : hipMemset(c->d_WF.p, 0, tb));
    std::vector<double> img(nt + 6, 0.0);
    img[1] = VTable[0];
    memcpy(&img[2], VTable, tb);
    HIPCHK(c->d_VTimg.alloc(img.size()));
    HIPCHK(hipMemcpy(c->d_VTimg.p, img.data(), img.size() * sizeof(double), hipMemcpyHostToDevice));
    // on the context's own stream, and waited for: that stream is non-blocking, so a fill on the default stream is not
    // ordered against the first upload, which could then be overwritten with zeros in part
    HIPCHK(hipMemsetAsync(c->d_paths.p, 0, np * sizeof(double), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->n_cu = device_cus();                     // (the context's device is current since hipSetDevice above)
    g_live_ctx[device_id & 63].fetch_add(1);
    *out = c.release();
    return PIGS_OK;
}

int pigs_ctx_destroy(pigs_ctx *c)
{
    if (!c) return PIGS_OK;
    g_live_ctx[c->device & 63].fetch_sub(1);
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    delete c;                                   // every resource is released by the member that owns it
    return PIGS_OK;
}

// after a synchronisation: did a cooperating workgroup of the TranslateChain kernel give up waiting (pigs_cm.hip)?
static int check_cm(pigs_ctx *c)
{
    if (c->h_cm_err.h && *(volatile int *)c->h_cm_err.h)
        return fail(PIGS_ERR_HIP, "TranslateChain kernel: a cooperating workgroup timed out; the worldlines of this context are invalid");
    return PIGS_OK;
}

// every entry point that waits for the stream and then hands state of the walkers to the caller (worldlines, counters,
// events, generator, estimators) ends here: after a time-out in pigs_cm.hip none of it may be returned as if it were valid
static int sync_checked(pigs_ctx *c)
{
    HIPCHK(hipStreamSynchronize(c->stream));
    return check_cm(c);
}
#define SYNC_CHECKED(c)                          \
    do {                                         \
        const int rc_ = sync_checked(c);         \
        if (rc_) return rc_;                     \
    } while (0)

int pigs_sync(pigs_ctx *c)
{
    int rc = check_ctx(c); if (rc) return rc;
    return sync_checked(c);
}

int pigs_stream(pigs_ctx *c, void **s)
{
    if (!c || !s) return fail(PIGS_ERR_ARG, "null pointer");
    *s = (void *)c->stream.h;
    return PIGS_OK;
}

int pigs_set_tuning(pigs_ctx *c, const char *key, int32_t value)
{
    if (!c || !key) return fail(PIGS_ERR_ARG, "null pointer");
    if (!strcmp(key, "k1_variant")) {
        if (!k1_variant_valid(value)) return fail(PIGS_ERR_ARG, "k1_variant=%d", value);
        c->k1_variant = value;
        return PIGS_OK;
    }
    if (!strcmp(key, "sweep_split")) {          // 1: stage-machine kernel (pigs_diag.hip) for the diagonal bisection moves; 0 (default): one kernel
        c->sweep_split = value != 0;
        return PIGS_OK;
    }
    if (!strcmp(key, "cm_split")) {             // TranslateChain by H workgroups per walker (pigs_cm.hip): -1 auto, 0 off, H = 1..4
        if (value < -1 || value > 4) return fail(PIGS_ERR_ARG, "cm_split=%d", value);
        c->cm_split = value;
        return PIGS_OK;
    }
    if (!strcmp(key, "cm_fault")) {             // TEST ONLY: force the time-out path of the TranslateChain exchange (pigs_cm.hip)
        c->sweep.cm_fault = (c->sweep.cm_fault & ~1) | (value != 0 ? 1 : 0);
        return PIGS_OK;
    }
    if (!strcmp(key, "cm_shared")) {            // 1: several contexts of this process sample on this device at once (see g_cm_gate);
        c->cm_shared = value != 0;              // set "cm_split" so that H x walkers + the other contexts' walkers <= CUs
        return PIGS_OK;
    }
    if (!strcmp(key, "cm_exclusive")) {         // 1: other contexts of this process on the device are idle while this one samples
        c->cm_exclusive = value != 0;           // (bench.py's extra legs next to its main context): cooperating workgroups allowed
        return PIGS_OK;
    }
    if (!strcmp(key, "vh_form")) {              // histograms of pigs_vh_accumulate: -1 automatic, 0 global atomics, 1 privatised in LDS
        if (value < -1 || value > 1) return fail(PIGS_ERR_ARG, "vh_form=%d", value);
        c->vh_form = value;
        return PIGS_OK;
    }
    if (!strcmp(key, "g3_form")) {              // counters of pigs_g3_accumulate: -1 automatic, 0 global atomics, 1 privatised in LDS
        if (value < -1 || value > 1) return fail(PIGS_ERR_ARG, "g3_form=%d", value);
        c->g3_form = value;
        return PIGS_OK;
    }
    if (!strcmp(key, "grv_form")) {             // vector grid of pigs_grv_accumulate: -1 automatic, 0 global atomics, 1 privatised in LDS
        if (value < -1 || value > 1) return fail(PIGS_ERR_ARG, "grv_form=%d", value);
        c->grv_form = value;
        return PIGS_OK;
    }
    if (!strcmp(key, "sf_scratch_mib")) {       // MiB the unfolded paths of one pigs_sf_accumulate launch may take; read by pigs_sf_init
        if (value < 1 || value > 2048) return fail(PIGS_ERR_ARG, "sf_scratch_mib=%d", value);
        c->sf_scratch_mib = value;
        return PIGS_OK;
    }
    if (!strcmp(key, "cl_scratch_mib")) {       // MiB the per-slice sums of one pigs_cl_accumulate launch may take; read by pigs_cl_init
        if (value < 1 || value > 2048) return fail(PIGS_ERR_ARG, "cl_scratch_mib=%d", value);
        c->cl_scratch_mib = value;
        return PIGS_OK;
    }
    if (!strcmp(key, "pc_scratch_mib")) {       // MiB the per-slice sums and labels of one pigs_pc_accumulate launch may take; read by pigs_pc_init
        if (value < 1 || value > 2048) return fail(PIGS_ERR_ARG, "pc_scratch_mib=%d", value);
        c->pc_scratch_mib = value;
        return PIGS_OK;
    }
    if (!strcmp(key, "sweep_threads")) {
        if (value != 256 && value != 512 && value != 768 && value != 1024) return fail(PIGS_ERR_ARG, "sweep_threads=%d", value);
        c->sweep_threads = value;
        return PIGS_OK;
    }
    return fail(PIGS_ERR_ARG, "unknown tuning key '%s'", key);
}

int pigs_selftest_fastmath(pigs_ctx *c, int32_t blocks, int32_t iters, uint64_t bad[4])
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!bad || blocks < 1 || iters < 1) return fail(PIGS_ERR_ARG, "bad arguments");
    DevBuf<unsigned long long> d;
    HIPCHK(d.alloc(4));
    HIPCHK(hipMemsetAsync(d.p, 0, 4 * sizeof(unsigned long long), c->stream));
    HIPCHK(launch_selftest_fastmath(c->P, 0x1234567ull, blocks, iters, d.p, c->stream));
    unsigned long long h[4];
    HIPCHK(hipMemcpyAsync(h, d.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
    SYNC_CHECKED(c);
    for (int i = 0; i < 4; ++i) bad[i] = h[i];
    return PIGS_OK;
}

// Device log of the sampler's Gaussians (pigs_log_host.h) against THIS host's libm, bit for bit, on n arguments of the
// sampler's domain (selftest_log_arg): chunks of 2^24 results come back over PCIe and are compared by host threads
// while the device computes the next chunk.
int pigs_selftest_log(pigs_ctx *c, int64_t n, uint64_t seed, uint64_t *mismatches, double *first_bad)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!mismatches || n < 1) return fail(PIGS_ERR_ARG, "bad arguments");
    const size_t chunk = (size_t)1 << 24;
    DevBuf<double> d[2];
    PinBuf hb[2];
    double *h[2] = {nullptr, nullptr};
    uint64_t bad = 0; double firstx = 0.0; bool have = false;
    hipError_t e = hipSuccess;
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        e = d[k].alloc(chunk);
        if (e == hipSuccess) e = hb[k].reserve(chunk * sizeof(double));
        h[k] = (double *)hb[k].h;
    }
    auto compare = [&](const double *res, uint64_t first, size_t m) {
        const unsigned nt = std::max(1u, std::min(32u, std::thread::hardware_concurrency()));
        std::vector<std::thread> th;
        std::vector<uint64_t> nb(nt, 0); std::vector<double> fx(nt, 0.0);
        for (unsigned t = 0; t < nt; ++t)
            th.emplace_back([&, t] {
                for (size_t i = t; i < m; i += nt) {
                    const double x = selftest_log_arg(first + i, seed), want = std::log(x), got = res[i];
                    if (memcmp(&want, &got, 8) != 0 && !(want != want && got != got)) { if (!nb[t]) fx[t] = x; ++nb[t]; }
                }
            });
        for (auto &x : th) x.join();
        for (unsigned t = 0; t < nt; ++t) { if (nb[t] && !have) { firstx = fx[t]; have = true; } bad += nb[t]; }
    };
    uint64_t done = 0; int cur = 0; size_t prev_m = 0; uint64_t prev_first = 0;
    while (e == hipSuccess && done < (uint64_t)n) {
        const size_t m = (size_t)std::min<uint64_t>(chunk, (uint64_t)n - done);
        e = launch_selftest_log(done, m, seed, d[cur].p, c->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(h[cur], d[cur].p, m * sizeof(double), hipMemcpyDeviceToHost, c->stream);
        if (prev_m) compare(h[cur ^ 1], prev_first, prev_m);            // overlaps the chunk in flight
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        prev_m = m; prev_first = done; done += m; cur ^= 1;
    }
    if (e == hipSuccess && prev_m) compare(h[cur ^ 1], prev_first, prev_m);
    if (e != hipSuccess) return fail(PIGS_ERR_HIP, "pigs_selftest_log: %s", hipGetErrorString(e));
    *mismatches = bad;
    if (first_bad) *first_bad = firstx;
    return PIGS_OK;
}

int pigs_selftest_stream_read(pigs_ctx *c, int32_t reps, double *bytes, double *seconds)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!bytes || !seconds || reps < 1) return fail(PIGS_ERR_ARG, "bad arguments");
    const size_t nd = c->path_doubles * (size_t)c->n_walkers;
    DevBuf<double> sink;
    Event e0, e1;
    float ms = 0.f;
    hipError_t e = sink.alloc(1);
    if (e == hipSuccess) e = hipEventCreate(&e0.h);
    if (e == hipSuccess) e = hipEventCreate(&e1.h);
    for (int r = 0; r < 3 && e == hipSuccess; ++r) e = launch_stream_read(c->d_paths.p, nd, c->n_cu, sink.p, c->stream);
    if (e == hipSuccess) e = hipEventRecord(e0, c->stream);
    for (int r = 0; r < reps && e == hipSuccess; ++r) e = launch_stream_read(c->d_paths.p, nd, c->n_cu, sink.p, c->stream);
    if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e != hipSuccess) return fail(PIGS_ERR_HIP, "pigs_selftest_stream_read: %s", hipGetErrorString(e));
    *bytes = (double)(nd * sizeof(double));
    *seconds = 1e-3 * (double)ms / reps;
    return PIGS_OK;
}

// ---- residency -------------------------------------------------------------------------
static int upload_range(pigs_ctx *c, int w0, int nw, const double *raw)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!raw) return fail(PIGS_ERR_ARG, "null Path");
    if (w0 < 0 || nw < 1 || w0 + nw > c->n_walkers) return fail(PIGS_ERR_ARG, "walker range %d+%d of %d", w0, nw, c->n_walkers);
    // stage in chunks of <= 64 walkers so the scratch stays small
    const int chunk = 64;
    for (int a = 0; a < nw; a += chunk) {
        const int m = nw - a < chunk ? nw - a : chunk;
        HIPCHK(c->d_stage.reserve(c->raw_doubles * m));
        HIPCHK(hipMemcpyAsync(c->d_stage.p, raw + c->raw_doubles * a, c->raw_doubles * m * sizeof(double),
                              hipMemcpyHostToDevice, c->stream));
        HIPCHK(launch_pack(c->P, c->d_paths.p, c->d_stage.p, w0 + a, m, c->stream));
        SYNC_CHECKED(c);
    }
    return PIGS_OK;
}

static int download_range(pigs_ctx *c, int w0, int nw, double *raw)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!raw) return fail(PIGS_ERR_ARG, "null Path");
    if (w0 < 0 || nw < 1 || w0 + nw > c->n_walkers) return fail(PIGS_ERR_ARG, "walker range %d+%d of %d", w0, nw, c->n_walkers);
    const int chunk = 64;
    for (int a = 0; a < nw; a += chunk) {
        const int m = nw - a < chunk ? nw - a : chunk;
        HIPCHK(c->d_stage.reserve(c->raw_doubles * m));
        HIPCHK(launch_unpack(c->P, c->d_paths.p, c->d_stage.p, w0 + a, m, c->stream));
        HIPCHK(hipMemcpyAsync(raw + c->raw_doubles * a, c->d_stage.p, c->raw_doubles * m * sizeof(double),
                              hipMemcpyDeviceToHost, c->stream));
        SYNC_CHECKED(c);
    }
    return PIGS_OK;
}

int pigs_path_upload(pigs_ctx *c, int32_t walker, const double *Path) { return upload_range(c, walker, 1, Path); }
int pigs_path_download(pigs_ctx *c, int32_t walker, double *Path) { return download_range(c, walker, 1, Path); }
int pigs_path_upload_all(pigs_ctx *c, const double *Paths) { return c ? upload_range(c, 0, c->n_walkers, Paths) : fail(PIGS_ERR_ARG, "null context"); }
int pigs_path_download_all(pigs_ctx *c, double *Paths) { return c ? download_range(c, 0, c->n_walkers, Paths) : fail(PIGS_ERR_ARG, "null context"); }

// ---- K1 ----------------------------------------------------------------------------------
static int check_items(pigs_ctx *c, int64_t n, const int32_t *walker, const int32_t *ip, const int32_t *ib)
{
    if (n < 0 || n > 0x7fffffff) return fail(PIGS_ERR_ARG, "n_items=%lld out of range", (long long)n);
    if (n && (!walker || !ip || !ib)) return fail(PIGS_ERR_ARG, "null index array");
    for (int64_t i = 0; i < n; ++i) {
        if (walker[i] < 0 || walker[i] >= c->n_walkers || ip[i] < 1 || ip[i] > c->P.Np || ib[i] < 0 || ib[i] >= c->P.M)
            return fail(PIGS_ERR_ARG, "item %lld: walker=%d ip=%d ib=%d out of range", (long long)i, walker[i], ip[i], ib[i]);
    }
    return PIGS_OK;
}

static int delta_action_host(pigs_ctx *c, int64_t n, const int32_t *walker, const int32_t *ip,
                             const int32_t *ib, const double *xnew, const double *xold,
                             double *DeltaS, double *parts)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_items(c, n, walker, ip, ib); if (rc) return rc;
    if (n == 0) return PIGS_OK;
    if (!xnew || !xold || (!DeltaS && !parts)) return fail(PIGS_ERR_ARG, "null pointer");
    const size_t nd = (size_t)n * c->P.dim;
    HIPCHK(c->d_walker.reserve(n)); HIPCHK(c->d_ip.reserve(n)); HIPCHK(c->d_ib.reserve(n));
    HIPCHK(c->d_xnew.reserve(nd)); HIPCHK(c->d_xold.reserve(nd)); HIPCHK(c->d_out.reserve(n));
    if (parts) HIPCHK(c->d_parts.reserve((size_t)n * 3));
    hipStream_t s = c->stream;
    HIPCHK(hipMemcpyAsync(c->d_walker.p, walker, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_ip.p, ip, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_ib.p, ib, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_xnew.p, xnew, nd * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_xold.p, xold, nd * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(launch_delta_action(c->P, c->k1_variant, c->d_paths.p, c->d_VT.p, c->d_VTimg.p, c->d_WF.p, (int)n, c->d_walker.p, c->d_ip.p,
                               c->d_ib.p, c->d_xnew.p, c->d_xold.p, c->d_out.p,
                               parts ? c->d_parts.p : nullptr, s));
    if (DeltaS) HIPCHK(hipMemcpyAsync(DeltaS, c->d_out.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    if (parts) HIPCHK(hipMemcpyAsync(parts, c->d_parts.p, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    SYNC_CHECKED(c);
    return PIGS_OK;
}

int pigs_delta_action_batch(pigs_ctx *c, int64_t n, const int32_t *walker, const int32_t *ip,
                            const int32_t *ib, const double *xnew, const double *xold, double *DeltaS)
{
    if (!DeltaS && n) return fail(PIGS_ERR_ARG, "null DeltaS");
    return delta_action_host(c, n, walker, ip, ib, xnew, xold, DeltaS, nullptr);
}

int pigs_delta_action_parts(pigs_ctx *c, int64_t n, const int32_t *walker, const int32_t *ip,
                            const int32_t *ib, const double *xnew, const double *xold, double *parts)
{
    if (!parts && n) return fail(PIGS_ERR_ARG, "null parts");
    return delta_action_host(c, n, walker, ip, ib, xnew, xold, nullptr, parts);
}

int pigs_delta_action_batch_dev(pigs_ctx *c, int64_t n, const int32_t *d_walker, const int32_t *d_ip,
                                const int32_t *d_ib, const double *d_xnew, const double *d_xold,
                                double *d_DeltaS)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (n < 0 || n > 0x7fffffff) return fail(PIGS_ERR_ARG, "n_items=%lld out of range", (long long)n);
    if (n == 0) return PIGS_OK;
    if (!d_walker || !d_ip || !d_ib || !d_xnew || !d_xold || !d_DeltaS) return fail(PIGS_ERR_ARG, "null device pointer");
    // indices are range-checked on the device (out-of-range items produce NaN, never a fault)
    HIPCHK(launch_delta_action(c->P, c->k1_variant, c->d_paths.p, c->d_VT.p, c->d_VTimg.p, c->d_WF.p, (int)n, d_walker, d_ip, d_ib,
                               d_xnew, d_xold, d_DeltaS, nullptr, c->stream));
    return PIGS_OK;
}

// ---- staged (pinned, zero-copy) forms --------------------------------------------------------
int pigs_stage_reserve(pigs_ctx *c, int64_t cap, int64_t keep, int32_t **walker, int32_t **ip, int32_t **ib,
                       double **xnew, double **xold, double **DeltaS)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (cap < 1 || cap > 0x7fffffff || keep < 0 || !walker || !ip || !ib || !xnew || !xold || !DeltaS)
        return fail(PIGS_ERR_ARG, "bad stage_reserve arguments");
    if (cap > c->st_cap) {
        SYNC_CHECKED(c);
        const size_t d = c->P.dim, k = (size_t)(keep < c->st_cap ? keep : c->st_cap);
        HIPCHK(c->st_w.reserve(cap * sizeof(int32_t), k * sizeof(int32_t)));
        HIPCHK(c->st_ip.reserve(cap * sizeof(int32_t), k * sizeof(int32_t)));
        HIPCHK(c->st_ib.reserve(cap * sizeof(int32_t), k * sizeof(int32_t)));
        HIPCHK(c->st_xn.reserve(cap * d * sizeof(double), k * d * sizeof(double)));
        HIPCHK(c->st_xo.reserve(cap * d * sizeof(double), k * d * sizeof(double)));
        HIPCHK(c->st_out.reserve(cap * sizeof(double), k * sizeof(double)));
        c->st_cap = cap;
    }
    *walker = (int32_t *)c->st_w.h; *ip = (int32_t *)c->st_ip.h; *ib = (int32_t *)c->st_ib.h;
    *xnew = (double *)c->st_xn.h; *xold = (double *)c->st_xo.h; *DeltaS = (double *)c->st_out.h;
    return PIGS_OK;
}

int pigs_delta_action_staged(pigs_ctx *c, int64_t n)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (n < 0 || n > c->st_cap) return fail(PIGS_ERR_ARG, "n_items=%lld exceeds the staged capacity %lld", (long long)n, (long long)c->st_cap);
    if (n == 0) return PIGS_OK;
    // indices are range-checked on the device (bad item -> NaN)
    HIPCHK(launch_delta_action(c->P, c->k1_variant, c->d_paths.p, c->d_VT.p, c->d_VTimg.p, c->d_WF.p, (int)n,
                               (const int32_t *)c->st_w.d, (const int32_t *)c->st_ip.d, (const int32_t *)c->st_ib.d,
                               (const double *)c->st_xn.d, (const double *)c->st_xo.d, (double *)c->st_out.d,
                               nullptr, c->stream));
    SYNC_CHECKED(c);
    return PIGS_OK;
}

int pigs_commit_reserve(pigs_ctx *c, int64_t cap, int64_t keep, int32_t **walker, int32_t **ip, int32_t **ib, double **x)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (cap < 1 || cap > 0x7fffffff || keep < 0 || !walker || !ip || !ib || !x) return fail(PIGS_ERR_ARG, "bad commit_reserve arguments");
    if (cap > c->cs_cap) {
        SYNC_CHECKED(c);
        const size_t d = c->P.dim, k = (size_t)(keep < c->cs_cap ? keep : c->cs_cap);
        HIPCHK(c->cs_w.reserve(cap * sizeof(int32_t), k * sizeof(int32_t)));
        HIPCHK(c->cs_ip.reserve(cap * sizeof(int32_t), k * sizeof(int32_t)));
        HIPCHK(c->cs_ib.reserve(cap * sizeof(int32_t), k * sizeof(int32_t)));
        HIPCHK(c->cs_x.reserve(cap * d * sizeof(double), k * d * sizeof(double)));
        c->cs_cap = cap;
    }
    *walker = (int32_t *)c->cs_w.h; *ip = (int32_t *)c->cs_ip.h; *ib = (int32_t *)c->cs_ib.h; *x = (double *)c->cs_x.h;
    return PIGS_OK;
}

int pigs_commit_staged(pigs_ctx *c, int64_t n)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (n < 0 || n > c->cs_cap) return fail(PIGS_ERR_ARG, "n=%lld exceeds the staged capacity %lld", (long long)n, (long long)c->cs_cap);
    if (n == 0) return PIGS_OK;
    const int32_t *w = (const int32_t *)c->cs_w.h, *ip = (const int32_t *)c->cs_ip.h, *ib = (const int32_t *)c->cs_ib.h;
    rc = check_items(c, n, w, ip, ib); if (rc) return rc;
    mark_superseded(n, (int32_t *)c->cs_w.h, ip, ib, c->P.M, c->P.Np);
    HIPCHK(launch_commit_beads(c->P, c->d_paths.p, n, (const int32_t *)c->cs_w.d, (const int32_t *)c->cs_ip.d,
                               (const int32_t *)c->cs_ib.d, (const double *)c->cs_x.d, c->stream));
    return PIGS_OK;
}

// ---- K5 ----------------------------------------------------------------------------------
int pigs_commit_beads(pigs_ctx *c, int64_t n, const int32_t *walker, const int32_t *ip,
                      const int32_t *ib, const double *x)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_items(c, n, walker, ip, ib); if (rc) return rc;
    if (n == 0) return PIGS_OK;
    if (!x) return fail(PIGS_ERR_ARG, "null x");
    const size_t nd = (size_t)n * c->P.dim;
    HIPCHK(c->d_walker.reserve(n)); HIPCHK(c->d_ip.reserve(n)); HIPCHK(c->d_ib.reserve(n));
    HIPCHK(c->d_xnew.reserve(nd));
    hipStream_t s = c->stream;
    std::vector<int32_t> wl(walker, walker + n);
    mark_superseded(n, wl.data(), ip, ib, c->P.M, c->P.Np);
    HIPCHK(hipMemcpyAsync(c->d_walker.p, wl.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_ip.p, ip, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_ib.p, ib, n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->d_xnew.p, x, nd * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(launch_commit_beads(c->P, c->d_paths.p, n, c->d_walker.p, c->d_ip.p, c->d_ib.p, c->d_xnew.p, s));
    SYNC_CHECKED(c);
    return PIGS_OK;
}

int pigs_swap_tails(pigs_ctx *c, int32_t walker, int32_t iw, int32_t ik)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (walker < 0 || walker >= c->n_walkers || iw < 1 || iw > c->P.Np || ik < 1 || ik > c->P.Np)
        return fail(PIGS_ERR_ARG, "swap_tails(walker=%d, iw=%d, ik=%d) out of range", walker, iw, ik);
    if (iw == ik) return PIGS_OK;
    HIPCHK(launch_swap_tails(c->P, c->d_paths.p, walker, iw, ik, c->stream));
    SYNC_CHECKED(c);
    return PIGS_OK;
}

// ---- K6: device-resident sampler ----------------------------------------------------------------
namespace {
// reference random_mod.f90:5-31 (seeding) and the conversion of a block-form state (mti, mt) to
// the sliding form the kernel keeps: the first `mti` steps of the block twist are applied, so slot
// k < mti already holds element k+624 and the next output is slot mti.
void mt_seed_words(uint32_t seed, uint32_t *w)
{
    w[0] = seed;
    for (int i = 1; i < 624; ++i) w[i] = 69069u * w[i - 1];
}
void mt_twist_prefix(int n, uint32_t *w)
{
    for (int i = 0; i < n; ++i) {
        const uint32_t y = (w[i] & 0x80000000u) | (w[(i + 1) % 624] & 0x7fffffffu);
        w[i] = w[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
}
// st: [624 sliding][624 block form][pos] from the reference's block form (mti, words)
void mt_block_to_device(int mti, const uint32_t *words, uint32_t *st)
{
    uint32_t *sl = st, *blk = st + 624;
    memcpy(blk, words, 624 * sizeof(uint32_t));
    if (mti >= 624) { mt_twist_prefix(624, blk); mti = 0; }        // block exhausted: next block, nothing consumed
    memcpy(sl, blk, 624 * sizeof(uint32_t));
    mt_twist_prefix(mti, sl);                                        // consumed slots already slid on
    st[1248] = (uint32_t)mti;
}
} // namespace

int pigs_sampler_init(pigs_ctx *c, const pigs_sweep_params *sp)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!sp) return fail(PIGS_ERR_ARG, "null sweep params");
    const bool sta = sp->sampling == 1;
    if (sp->sampling != 0 && sp->sampling != 1) return fail(PIGS_ERR_ARG, "sampling must be 0 ('bis') or 1 ('sta')");
    const bool worm0 = sp->CWorm > 0.0;
    // Nlev: any 2^Nlev <= 2 Nb up to 7 levels for periodic systems (pigs_diag.hip beyond 4), 4 for trapped ones;
    // Lstag <= Nb is a requirement of the worm's half-chain moves only (vpi_mod.f90:1376-1817): with CWorm = 0 any
    // Lstag <= 2 Nb works, as in the reference
    // (head / tail moves bisect 2^nl beads with nl = 2 .. max(Nlev, 2): vpi_mod.f90:1023)
    if ((!sta && (sp->Nlev < 1 || sp->Nlev > (c->P.trap ? 4 : 7) || (1 << (sp->Nlev > 2 ? sp->Nlev : 2)) > 2 * c->P.Nb)) || sp->Nstag < 0 || sp->CMFreq < 1 ||
        sp->Lstag < 2 || sp->Lstag > (worm0 ? c->P.Nb : 2 * c->P.Nb))
        return fail(PIGS_ERR_ARG, "sweep params out of range (Nlev=%d Nstag=%d CMFreq=%d Lstag=%d)", sp->Nlev, sp->Nstag, sp->CMFreq, sp->Lstag);
    const bool worm = sp->CWorm > 0.0;
    if (worm && (sp->Nobdm < 0 || sp->Nbin < 1 || sp->Npw < 0 || !(sp->rbin > 0.0) || !(sp->density > 0.0)))
        return fail(PIGS_ERR_ARG, "worm parameters out of range");
    c->sampler_ready = false;                 // until this call has gone through
    c->form_cm = -1;
    c->form_diag = false;
    SweepParams &k = c->sweep;
    memset(&k, 0, sizeof k);
    k.Nlev = sta ? 1 : sp->Nlev; k.Nstag = sp->Nstag; k.Lstag = sp->Lstag; k.staging = sta;
    k.delta_cm = sp->delta_cm; k.open_attempt = 1; k.do_cm = 1;
    k.worm = worm; k.swapping = sp->swapping != 0; k.Nobdm = worm ? sp->Nobdm : 0;
    k.Nbin = worm ? sp->Nbin : 1; k.Npw = worm ? sp->Npw : 0; k.rbin = worm ? sp->rbin : 1.0;
    k.log_cworm_density = worm ? std::log(sp->CWorm * sp->density) : 0.0;      // host libm, as the reference
    c->cm_freq = sp->CMFreq;
    // one workgroup per walker: the 8-wave form (periodic: table image in LDS) while every walker gets a CU of its own,
    // the 4-wave form (three workgroups per CU) beyond that (measured: scripts/sampler_bench.py)
    c->sweep_threads = sweep_form(c->P, c->sweep, c->n_walkers > c->n_cu ? 256 : 1024);
    if (sweep_lds_bytes(c->P, c->sweep, c->sweep_threads) > 160 * 1024) c->sweep_threads = sweep_form(c->P, c->sweep, 256);
    if (sweep_lds_bytes(c->P, c->sweep, c->sweep_threads) > 160 * 1024) return fail(PIGS_ERR_UNSUPPORTED, "worldline too long for the sampler's LDS staging");
    // periodic 'bis' inputs beyond four levels need the stage-machine kernel (pigs_sampler_step): refused here, so that
    // a caller can pick the host-driven sampler instead
    if (!c->P.trap && !k.staging && k.Nlev > 4 && !diag_supported(c->P, k))
        return fail(PIGS_ERR_UNSUPPORTED, "Nlev=%d needs the stage-machine kernel, which does not fit this worldline", k.Nlev);
    const size_t W = c->n_walkers;
    // a step logs at most one open / close event and one swap per OBDM iteration
    k.ev_ints = kEvInts > 4 + 2 * (1 + k.Nobdm) ? kEvInts : 4 + 2 * (1 + k.Nobdm);
    c->nrho_doubles = W * (size_t)k.Nbin * (k.Npw + 1);
    // 0.5d0*real(dim)*log(2.d0*pi*real(Ls)*dt) of vpi_mod.f90:1873, tabulated with the host libm
    std::vector<double> dk(sp->Lstag + 2, 0.0);
    const double pi = std::acos(-1.0);
    for (int Ls = 1; Ls <= sp->Lstag + 1; ++Ls)
        dk[Ls] = 0.5 * (double)(float)c->P.dim * std::log(2.0 * pi * (double)(float)Ls * c->P.dt);
    HIPCHK(c->d_rng.alloc(W * kRngWords));
    HIPCHK(c->d_counters.alloc(W * kCounters));
    HIPCHK(c->d_worm.alloc(W * kWormDoubles));
    HIPCHK(c->d_evlog.alloc(W * k.ev_ints));
    HIPCHK(c->d_nrho.alloc(c->nrho_doubles));
    HIPCHK(c->d_dklog.alloc(dk.size()));
    hipStream_t s = c->stream;
    if (worm && !c->P.trap) {
        // the end tape of pigs_nk_accumulate: a step writes every walker's count, the worm loop the vectors
        HIPCHK(c->d_tape_count.alloc(W));
        HIPCHK(c->d_tape_x.alloc(std::max<size_t>(1, W * (size_t)k.Nobdm * c->P.dim)));
        HIPCHK(hipMemsetAsync(c->d_tape_count.p, 0, W * sizeof(int32_t), s));
        HIPCHK(hipMemsetAsync(c->d_tape_x.p, 0, c->d_tape_x.cap * sizeof(double), s));
        k.tape_count = c->d_tape_count.p;
        k.tape_x = c->d_tape_x.p;
    }
    HIPCHK(hipMemcpyAsync(c->d_dklog.p, dk.data(), dk.size() * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemsetAsync(c->d_counters.p, 0, W * kCounters * sizeof(unsigned long long), s));
    HIPCHK(hipMemsetAsync(c->d_worm.p, 0, W * kWormDoubles * sizeof(double), s));
    HIPCHK(hipMemsetAsync(c->d_evlog.p, 0, W * k.ev_ints * sizeof(int), s));
    HIPCHK(hipMemsetAsync(c->d_nrho.p, 0, c->nrho_doubles * sizeof(double), s));
    std::vector<uint32_t> st(W * kRngWords);
    for (size_t w = 0; w < W; ++w) {
        uint32_t seedw[624];
        mt_seed_words(4357u, seedw);
        mt_block_to_device(624, seedw, &st[w * kRngWords]);
    }
    HIPCHK(hipMemcpyAsync(c->d_rng.p, st.data(), st.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    SYNC_CHECKED(c);
    c->sampler_ready = true;
    return PIGS_OK;
}

int pigs_sampler_set_rng(pigs_ctx *c, int32_t walker, int32_t mti, const int32_t mt[624])
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->sampler_ready) return fail(PIGS_ERR_ARG, "pigs_sampler_init first");
    if (walker < 0 || walker >= c->n_walkers || !mt || mti < 0 || mti > 624) return fail(PIGS_ERR_ARG, "bad rng state");
    uint32_t st[kRngWords];
    mt_block_to_device(mti, (const uint32_t *)mt, st);
    HIPCHK(hipMemcpyAsync(c->d_rng.p + (size_t)walker * kRngWords, st, sizeof st, hipMemcpyHostToDevice, c->stream));
    SYNC_CHECKED(c);
    return PIGS_OK;
}

int pigs_sampler_get_rng(pigs_ctx *c, int32_t walker, int32_t *mti, int32_t mt[624])
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->sampler_ready) return fail(PIGS_ERR_ARG, "pigs_sampler_init first");
    if (walker < 0 || walker >= c->n_walkers || !mt || !mti) return fail(PIGS_ERR_ARG, "bad rng request");
    uint32_t st[kRngWords];
    HIPCHK(hipMemcpyAsync(st, c->d_rng.p + (size_t)walker * kRngWords, sizeof st, hipMemcpyDeviceToHost, c->stream));
    SYNC_CHECKED(c);
    memcpy(mt, st + 624, 624 * sizeof(uint32_t));                    // block form: what mtsavef would hold
    *mti = (int32_t)st[1248];
    return PIGS_OK;
}

int pigs_sampler_seed(pigs_ctx *c, int32_t walker, int32_t seed)
{
    uint32_t w[624];
    mt_seed_words((uint32_t)seed, w);
    return pigs_sampler_set_rng(c, walker, 624, (const int32_t *)w);
}

static int launch_pending_estimators(pigs_ctx *c, hipEvent_t gate);

int pigs_sampler_step(pigs_ctx *c, int32_t istep)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->sampler_ready) return fail(PIGS_ERR_ARG, "pigs_sampler_init first");
    rc = check_cm(c); if (rc) return rc;                      // an earlier step's TranslateChain kernel gave up: stop here
    SweepParams sp = c->sweep;
    sp.do_cm = (istep % c->cm_freq) == 0;
    // Two forms of the diagonal bisection moves of a periodic system: inside the one-launch kernel (pigs_sampler.hip;
    // Nlev <= 4), or the stage machine of pigs_diag.hip between two launches of that kernel for the open / close attempt
    // and the worm moves (any Nlev with 2^Nlev <= 2 Nb, Nlev <= 7).  Measured at N=256, 161 beads, 128 walkers: 48.1 ms
    // vs 56.5 ms per MC step (profiles/r02_k6_stage_machine.txt), so the stage machine runs only where the other form
    // cannot, or on request (pigs_set_tuning "sweep_split" = 1).
    //
    // TranslateChain -- the one arithmetic-bound stage -- goes to its own kernel (pigs_cm.hip): H cooperating workgroups
    // per walker while the chip has H >= 2 CUs per walker, one otherwise (bit-identical trajectory whatever H): open /
    // close attempt, that kernel, the rest.
    int H = 0;
    if (c->cm_split != 0 && sp.do_cm) {
        H = cm_helpers(c->P, sp, c->n_cu);                    // what the chip holds (0: the kernel does not apply)
        if (c->cm_split > 0 && H > c->cm_split) H = c->cm_split;
        // cooperating workgroups wait for each other: only while this context has the chip to itself.  One workgroup per
        // walker (H = 1) exchanges nothing and is still the faster TranslateChain (sixteen waves on the LDS table image:
        // 46.8 -> 44.8 ms per MC step at 256 walkers, 95 -> 74 ms at 512, where the sweep kernel runs its 4-wave form)
        if (H > 1 && g_live_ctx[c->device & 63].load() != 1 && !c->cm_exclusive && !c->cm_shared) H = 1;
        // a lowered H means longer bead ranges per workgroup: 321 beads fit two workgroups per walker but not one (rows, LDS)
        // -- then TranslateChain stays inside the sweep kernel (round 3: the BASELINE-config-5 leg of bench.py next to a
        // second live context, and the sharded front end on one GPU, failed here with "invalid argument")
        if (H >= 1 && !cm_fits(c->P, H)) H = 0;
    }
    if (sp.do_cm) c->form_cm = H;
    bool cm_done = false;
    if (H >= 1) {
        if (!c->d_xch.p) {
            HIPCHK(c->d_xch.alloc(cm_exchange_words(c->P)));
            HIPCHK(hipMemsetAsync(c->d_xch.p, 0, c->d_xch.cap * sizeof(unsigned long long), c->stream));
        }
        if (!c->h_cm_err.h) {
            HIPCHK(c->h_cm_err.reserve(sizeof(int)));
            *(int *)c->h_cm_err.h = 0;
        }
        sp.parts = 1;
        HIPCHK(launch_sweep(c->P, sp, c->sweep_threads, c->d_paths.p, c->d_VT.p, c->d_VTimg.p, c->d_WF.p, c->d_rng.p, c->d_counters.p,
                            c->d_worm.p, c->d_evlog.p, c->d_nrho.p, c->d_dklog.p, c->stream));
        int *d_err = (int *)c->h_cm_err.d;
        hipError_t e = hipSuccess;
        if (c->cm_shared && H > 1) {
            std::lock_guard<std::mutex> lk(g_cm_mutex[c->device & 63]);
            hipEvent_t &gate = g_cm_gate[c->device & 63];
            if (!gate) e = hipEventCreateWithFlags(&gate, hipEventDisableTiming);
            else       e = hipStreamWaitEvent(c->stream, gate, 0);           // the device's previous TranslateChain kernel, whoever launched it
            if (e == hipSuccess) e = launch_cm(c->P, sp, H, c->cm_seq, c->d_paths.p, c->d_VTimg.p, c->d_WF.p, c->d_rng.p, c->d_counters.p,
                                               c->d_worm.p, c->d_xch.p, d_err, c->stream);
            if (e == hipSuccess) e = hipEventRecord(gate, c->stream);
        } else {
            e = launch_cm(c->P, sp, H, c->cm_seq, c->d_paths.p, c->d_VTimg.p, c->d_WF.p, c->d_rng.p, c->d_counters.p,
                          c->d_worm.p, c->d_xch.p, d_err, c->stream);
        }
        HIPCHK(e);
        c->cm_seq += (unsigned int)c->P.Np + 1;
        sp.do_cm = 0;
        cm_done = true;                                       // (the open / close attempt ran as well)
        // estimators of the previous step waiting for their turn (pigs_diagonal_estimators_begin): the TranslateChain
        // kernel fills the chip, the sweep kernel that follows leaves the CUs beyond one per walker idle -- they start there
        if (c->a_pend.on && !c->a_pend.launched) {
            HIPCHK(hipEventRecord(c->ev_gate, c->stream));
            rc = launch_pending_estimators(c, c->ev_gate); if (rc) return rc;
        }
    }
    if (c->a_pend.on && !c->a_pend.launched) {                // a step without the TranslateChain kernel: beside the whole step
        rc = launch_pending_estimators(c, c->ev_snap); if (rc) return rc;
    }
    // (pigs_sampler_init refused the inputs that need the stage machine where it does not fit)
    const bool need_split = !c->P.trap && !sp.staging && sp.Nlev > 4;
    c->form_diag = (c->sweep_split || need_split) && diag_supported(c->P, sp);
    if (c->form_diag) {
        if (!cm_done) {
            sp.parts = 1;
            HIPCHK(launch_sweep(c->P, sp, c->sweep_threads, c->d_paths.p, c->d_VT.p, c->d_VTimg.p, c->d_WF.p, c->d_rng.p, c->d_counters.p,
                                c->d_worm.p, c->d_evlog.p, c->d_nrho.p, c->d_dklog.p, c->stream));
        }
        HIPCHK(launch_diag(c->P, sp, 512, c->d_paths.p, c->d_VTimg.p, c->d_WF.p, c->d_rng.p, c->d_counters.p, c->d_worm.p, c->stream));
        if (sp.worm) {
            sp.parts = 4;
            HIPCHK(launch_sweep(c->P, sp, c->sweep_threads, c->d_paths.p, c->d_VT.p, c->d_VTimg.p, c->d_WF.p, c->d_rng.p, c->d_counters.p,
                                c->d_worm.p, c->d_evlog.p, c->d_nrho.p, c->d_dklog.p, c->stream));
        }
    } else {
        sp.parts = cm_done ? 6 : 7;
        HIPCHK(launch_sweep(c->P, sp, c->sweep_threads, c->d_paths.p, c->d_VT.p, c->d_VTimg.p, c->d_WF.p, c->d_rng.p, c->d_counters.p,
                            c->d_worm.p, c->d_evlog.p, c->d_nrho.p, c->d_dklog.p, c->stream));
    }
    return PIGS_OK;
}

int pigs_sampler_form(pigs_ctx *c, int32_t out[4])
{
    if (!c || !out) return fail(PIGS_ERR_ARG, "null pointer");
    if (!c->sampler_ready) return fail(PIGS_ERR_ARG, "pigs_sampler_init first");
    out[0] = sweep_form(c->P, c->sweep, c->sweep_threads);   // what launch_sweep makes of the tuned value
    out[1] = c->form_cm;
    out[2] = c->form_diag ? 1 : 0;
    out[3] = c->cm_shared ? 1 : 0;
    return PIGS_OK;
}

int pigs_sampler_counters16(pigs_ctx *c, int64_t *cnt)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->sampler_ready || !cnt) return fail(PIGS_ERR_ARG, "pigs_sampler_init first / null output");
    HIPCHK(hipMemcpyAsync(cnt, c->d_counters.p, (size_t)c->n_walkers * kCounters * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    SYNC_CHECKED(c);
    return PIGS_OK;
}

int pigs_sampler_counters(pigs_ctx *c, int64_t *acc)
{
    if (!c || !acc) return fail(PIGS_ERR_ARG, "null pointer");
    std::vector<int64_t> all((size_t)c->n_walkers * kCounters);
    int rc = pigs_sampler_counters16(c, all.data()); if (rc) return rc;
    for (int w = 0; w < c->n_walkers; ++w)
        for (int q = 0; q < 4; ++q) acc[4 * w + q] = all[(size_t)w * kCounters + q];
    return PIGS_OK;
}

int pigs_sampler_get_worm(pigs_ctx *c, int32_t *isopen, int32_t *iworm, double *xend)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->sampler_ready || !isopen || !iworm || !xend) return fail(PIGS_ERR_ARG, "pigs_sampler_init first / null output");
    std::vector<double> h((size_t)c->n_walkers * kWormDoubles);
    HIPCHK(hipMemcpyAsync(h.data(), c->d_worm.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    SYNC_CHECKED(c);
    const int d = c->P.dim;
    for (int w = 0; w < c->n_walkers; ++w) {
        isopen[w] = (int32_t)h[(size_t)w * kWormDoubles];
        iworm[w]  = (int32_t)h[(size_t)w * kWormDoubles + 1];
        for (int t = 0; t < 2 * d; ++t) xend[(size_t)w * 2 * d + t] = h[(size_t)w * kWormDoubles + 2 + t];
    }
    return PIGS_OK;
}

int pigs_sampler_set_worm(pigs_ctx *c, const int32_t *isopen, const int32_t *iworm, const double *xend)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->sampler_ready || !isopen || !iworm || !xend) return fail(PIGS_ERR_ARG, "pigs_sampler_init first / null input");
    std::vector<double> h((size_t)c->n_walkers * kWormDoubles, 0.0);
    const int d = c->P.dim;
    for (int w = 0; w < c->n_walkers; ++w) {
        if (isopen[w] && (iworm[w] < 1 || iworm[w] > c->P.Np)) return fail(PIGS_ERR_ARG, "walker %d: iworm=%d", w, iworm[w]);
        h[(size_t)w * kWormDoubles]     = isopen[w] ? 1.0 : 0.0;
        h[(size_t)w * kWormDoubles + 1] = (double)iworm[w];
        for (int t = 0; t < 2 * d; ++t) h[(size_t)w * kWormDoubles + 2 + t] = xend[(size_t)w * 2 * d + t];
    }
    HIPCHK(hipMemcpyAsync(c->d_worm.p, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    SYNC_CHECKED(c);
    return PIGS_OK;
}

int pigs_sampler_event_ints(pigs_ctx *c, int32_t *n)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->sampler_ready || !n) return fail(PIGS_ERR_ARG, "pigs_sampler_init first / null output");
    *n = c->sweep.ev_ints;
    return PIGS_OK;
}

int pigs_sampler_events(pigs_ctx *c, int32_t *events)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->sampler_ready || !events) return fail(PIGS_ERR_ARG, "pigs_sampler_init first / null output");
    HIPCHK(hipMemcpyAsync(events, c->d_evlog.p, (size_t)c->n_walkers * c->sweep.ev_ints * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    SYNC_CHECKED(c);
    return PIGS_OK;
}

int pigs_sampler_nrho(pigs_ctx *c, double *nrho, const int32_t *reset)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->sampler_ready || !nrho) return fail(PIGS_ERR_ARG, "pigs_sampler_init first / null output");
    HIPCHK(hipMemcpyAsync(nrho, c->d_nrho.p, c->nrho_doubles * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (reset) {
        // zero the histograms of the flagged walkers, one memset per run of consecutive walkers
        const size_t per = c->nrho_doubles / (size_t)c->n_walkers;
        for (int w = 0; w < c->n_walkers;) {
            if (!reset[w]) { ++w; continue; }
            int e = w;
            while (e < c->n_walkers && reset[e]) ++e;
            HIPCHK(hipMemsetAsync(c->d_nrho.p + (size_t)w * per, 0, (size_t)(e - w) * per * sizeof(double), c->stream));
            w = e;
        }
    }
    SYNC_CHECKED(c);
    return PIGS_OK;
}

int pigs_slice_download(pigs_ctx *c, int32_t ib, double *R)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!R || ib < 0 || ib >= c->P.M) return fail(PIGS_ERR_ARG, "bad slice request");
    const size_t n = (size_t)c->P.dim * c->P.Np * c->n_walkers;
    HIPCHK(c->d_stage.reserve(n));
    HIPCHK(launch_slice_gather(c->P, c->d_paths.p, ib, c->d_stage.p, c->stream));
    HIPCHK(hipMemcpyAsync(R, c->d_stage.p, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    SYNC_CHECKED(c);
    return PIGS_OK;
}

// ---- K2/K3 -------------------------------------------------------------------------------
int pigs_potential_energy_slice(pigs_ctx *c, int32_t walker, int32_t ib, int32_t want_F2,
                                double *Pot, double *F2)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!Pot) return fail(PIGS_ERR_ARG, "null Pot");
    if (walker < 0 || walker >= c->n_walkers || ib < 0 || ib >= c->P.M) return fail(PIGS_ERR_ARG, "walker=%d ib=%d out of range", walker, ib);
    HIPCHK(c->est.slotw.reserve(1)); HIPCHK(c->est.slotb.reserve(1)); HIPCHK(c->est.slices.reserve(3));
    hipStream_t s = c->stream;
    HIPCHK(hipMemcpyAsync(c->est.slotw.p, &walker, sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->est.slotb.p, &ib, sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(launch_slice_energy(c->P, c->d_paths.p, c->d_VT.p, c->d_VTimg.p, 1, c->est.slotw.p, c->est.slotb.p, want_F2 ? 2 : 0, 0, c->est.slices.p, s));
    double h[3];
    HIPCHK(hipMemcpyAsync(h, c->est.slices.p, sizeof h, hipMemcpyDeviceToHost, s));
    SYNC_CHECKED(c);
    *Pot = h[0];
    if (F2) *F2 = want_F2 ? h[1] : 0.0;
    return PIGS_OK;
}

// the walkers of a request -- walkers[i], or 0..n-1 when the list is left out -- range-checked
static int walker_list(const pigs_ctx *c, int n, const int32_t *walkers, std::vector<int32_t> &sw)
{
    sw.resize(n);
    for (int i = 0; i < n; ++i) {
        sw[i] = walkers ? walkers[i] : i;
        if (sw[i] < 0 || sw[i] >= c->n_walkers) return fail(PIGS_ERR_ARG, "walker %d out of range", sw[i]);
    }
    return PIGS_OK;
}

// ---- the diagonal-estimator batch (EstBatch): shared by ThermEnergy and both forms of pigs_diagonal_estimators ------
static int est_describe(const pigs_ctx *c, int n, const int32_t *walkers, bool structure, int Nbin, double rbin, int Nk,
                        EstBatch &b)
{
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    if (structure && (Nbin < 1 || Nk < 0 || !(rbin > 0.0))) return fail(PIGS_ERR_ARG, "bad structure request");
    if (structure && c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "structural estimators are defined for PBC runs only (vpi.f90:466)");
    const int rc = walker_list(c, n, walkers, b.w); if (rc) return rc;
    b.n = n; b.Nbin = Nbin; b.rbin = rbin; b.Nk = Nk; b.structure = structure;
    b.ns = 2 * (size_t)c->P.Nb;                       // ThermEnergy: slices 0..2Nb-1 (Q8)
    b.nslot = (size_t)n * b.ns;
    b.ng = structure ? (size_t)n * Nbin : 0;
    b.nk = structure ? (size_t)n * Nk * c->P.dim : 0;
    b.nres = (size_t)9 * n + b.ng + b.nk;
    return PIGS_OK;
}

static void est_slots(const EstBatch &b, std::vector<int32_t> &sw, std::vector<int32_t> &sb)
{
    sw.resize(b.nslot + b.n); sb.resize(b.nslot);
    for (int i = 0; i < b.n; ++i) {
        for (size_t s = 0; s < b.ns; ++s) { sw[i * b.ns + s] = b.w[i]; sb[i * b.ns + s] = (int32_t)s; }
        sw[b.nslot + i] = b.w[i];
    }
}

// on stream s: the slot lists up into d, the five launches on the worldlines `paths` (ThermEnergy's slices on at most
// cu_cap workgroups; 0: no cap), the result block down to `host`.  sw, sb and host must outlive the copies.
static int est_launch(pigs_ctx *c, const EstBatch &b, const double *paths, EstBufs &d, const std::vector<int32_t> &sw,
                      const std::vector<int32_t> &sb, double *host, hipStream_t s, int cu_cap)
{
    const size_t n = b.n;
    HIPCHK(hipMemcpyAsync(d.slotw.p, sw.data(), sw.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(d.slotb.p, sb.data(), sb.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    double *r = d.res.p;
    const int32_t *dw = d.slotw.p + b.nslot;
    HIPCHK(launch_local_energy(c->P, paths, c->d_VT.p, c->d_WF.p, b.n, dw, 0, r, s));
    HIPCHK(launch_local_energy(c->P, paths, c->d_VT.p, c->d_WF.p, b.n, dw, 2 * c->P.Nb, r + 3 * n, s));
    HIPCHK(launch_slice_energy(c->P, paths, c->d_VT.p, c->d_VTimg.p, (int)b.nslot, d.slotw.p, d.slotb.p, 1, 1, d.slices.p, s, cu_cap));
    HIPCHK(launch_therm_combine(c->P, b.n, d.slices.p, r + 6 * n, r + 7 * n, r + 8 * n, s));
    if (b.structure)
        HIPCHK(launch_structure(c->P, paths, b.n, dw, c->P.Nb, b.Nbin, b.rbin, b.Nk, r + 9 * n, r + 9 * n + b.ng, s));
    HIPCHK(hipMemcpyAsync(host, r, b.nres * sizeof(double), hipMemcpyDeviceToHost, s));
    return PIGS_OK;
}

// a result block on the host into en (9 per walker), gr and Sk
static void est_unpack(const EstBatch &b, const double *h, double *en, double *gr, double *Sk)
{
    const size_t n = b.n;
    for (size_t i = 0; i < n; ++i) {
        for (int q = 0; q < 3; ++q) { en[9 * i + q] = h[3 * i + q]; en[9 * i + 3 + q] = h[3 * n + 3 * i + q]; }
        en[9 * i + 6] = h[6 * n + i]; en[9 * i + 7] = h[7 * n + i]; en[9 * i + 8] = h[8 * n + i];
    }
    if (b.structure) {
        memcpy(gr, h + 9 * n, b.ng * sizeof(double));
        if (b.nk) memcpy(Sk, h + 9 * n + b.ng, b.nk * sizeof(double));
    }
}

int pigs_therm_energy_batch(pigs_ctx *c, int32_t n, const int32_t *walkers, double *E, double *Ec, double *Ep)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (n < 0 || (n > c->n_walkers && !walkers)) return fail(PIGS_ERR_ARG, "n=%d walkers", n);
    if (n == 0) return PIGS_OK;
    if (!E || !Ec || !Ep) return fail(PIGS_ERR_ARG, "null output");
    EstBatch b;
    std::vector<int32_t> sw, sb;
    rc = est_describe(c, n, walkers, false, 0, 0.0, 0, b); if (rc) return rc;
    est_slots(b, sw, sb);
    HIPCHK(c->est.reserve(b));
    hipStream_t s = c->stream;
    double *r = c->est.res.p;
    HIPCHK(hipMemcpyAsync(c->est.slotw.p, sw.data(), b.nslot * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(c->est.slotb.p, sb.data(), b.nslot * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(launch_slice_energy(c->P, c->d_paths.p, c->d_VT.p, c->d_VTimg.p, (int)b.nslot, c->est.slotw.p, c->est.slotb.p, 1, 1, c->est.slices.p, s));
    HIPCHK(launch_therm_combine(c->P, n, c->est.slices.p, r, r + n, r + 2 * (size_t)n, s));
    HIPCHK(hipMemcpyAsync(E, r, n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(Ec, r + n, n * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(Ep, r + 2 * (size_t)n, n * sizeof(double), hipMemcpyDeviceToHost, s));
    SYNC_CHECKED(c);   // sw/sb must outlive the async copies
    return PIGS_OK;
}

// ---- K4 ----------------------------------------------------------------------------------
int pigs_local_energy_batch(pigs_ctx *c, int32_t n, const int32_t *walkers, int32_t ib,
                            double *E, double *Kin, double *Pot)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    if (n == 0) return PIGS_OK;
    if (!E || !Kin || !Pot) return fail(PIGS_ERR_ARG, "null output");
    if (ib < 0 || ib >= c->P.M) return fail(PIGS_ERR_ARG, "ib=%d out of range", ib);
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    HIPCHK(c->est.slotw.reserve(n)); HIPCHK(c->est.res.reserve((size_t)n * 3));
    hipStream_t s = c->stream;
    HIPCHK(hipMemcpyAsync(c->est.slotw.p, sw.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(launch_local_energy(c->P, c->d_paths.p, c->d_VT.p, c->d_WF.p, n, c->est.slotw.p, ib, c->est.res.p, s));
    std::vector<double> h((size_t)n * 3);
    HIPCHK(hipMemcpyAsync(h.data(), c->est.res.p, h.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    SYNC_CHECKED(c);
    for (int i = 0; i < n; ++i) { E[i] = h[3 * i]; Kin[i] = h[3 * i + 1]; Pot[i] = h[3 * i + 2]; }
    return PIGS_OK;
}

// ---- K7 ----------------------------------------------------------------------------------
int pigs_structure_batch(pigs_ctx *c, int32_t n, const int32_t *walkers, int32_t ib, int32_t Nbin,
                         double rbin, int32_t Nk, double *gr, double *Sk)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (n < 0 || Nbin < 1 || Nk < 0 || !(rbin > 0.0) || ib < 0 || ib >= c->P.M) return fail(PIGS_ERR_ARG, "bad structure request");
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "structural estimators are defined for PBC runs only (vpi.f90:466)");
    if (n == 0) return PIGS_OK;
    if (!gr || !Sk) return fail(PIGS_ERR_ARG, "null output");
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    const size_t ng = (size_t)n * Nbin, ns = (size_t)n * Nk * c->P.dim;
    HIPCHK(c->est.slotw.reserve(n)); HIPCHK(c->est.res.reserve(ng + ns));
    hipStream_t s = c->stream;
    HIPCHK(hipMemcpyAsync(c->est.slotw.p, sw.data(), n * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIPCHK(launch_structure(c->P, c->d_paths.p, n, c->est.slotw.p, ib, Nbin, rbin, Nk, c->est.res.p, c->est.res.p + ng, s));
    HIPCHK(hipMemcpyAsync(gr, c->est.res.p, ng * sizeof(double), hipMemcpyDeviceToHost, s));
    if (ns) HIPCHK(hipMemcpyAsync(Sk, c->est.res.p + ng, ns * sizeof(double), hipMemcpyDeviceToHost, s));
    SYNC_CHECKED(c);
    return PIGS_OK;
}

// ---- all diagonal-sector estimators of one MC step in one call ------------------------------
// What vpi.f90:443-469 evaluates after a diagonal step -- LocalEnergy at slices 0 and 2Nb (K4), ThermEnergy (K2/K3),
// g(r) and S(k) at slice Nb (K7) -- for n walkers: one upload of the slot lists, five launches, ONE result copy, one
// synchronisation (the separate entry points cost four round trips: ~1.6 ms per step of 128 walkers in round 2's bench).
// en[9*i ..] = E,Kin,Pot (slice 0), E,Kin,Pot (slice 2Nb), E,Ec,Ep (ThermEnergy) of walker i; gr (n x Nbin) and
// Sk (n x Nk x dim) may both be NULL (trapped systems: vpi.f90:466 computes them for PBC runs only).
int pigs_diagonal_estimators(pigs_ctx *c, int32_t n, const int32_t *walkers, int32_t Nbin, double rbin, int32_t Nk,
                             double *en, double *gr, double *Sk)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (n < 0 || !en) return fail(PIGS_ERR_ARG, "n=%d / null output", n);
    if (n == 0) return PIGS_OK;
    if (!gr != !Sk) return fail(PIGS_ERR_ARG, "bad structure request");
    EstBatch b;
    std::vector<int32_t> sw, sb;
    rc = est_describe(c, n, walkers, gr != nullptr, Nbin, rbin, Nk, b); if (rc) return rc;
    est_slots(b, sw, sb);
    HIPCHK(c->est.reserve(b));
    std::vector<double> h(b.nres);
    rc = est_launch(c, b, c->d_paths.p, c->est, sw, sb, h.data(), c->stream, 0); if (rc) return rc;
    SYNC_CHECKED(c);
    est_unpack(b, h.data(), en, gr, Sk);
    return PIGS_OK;
}

// ---- the same, overlapped with the sampler ------------------------------------------------------
// At BASELINE's 128 walkers per GPU the device-resident sampler keeps 128 of the 256 CUs busy for 30 of a step's 38 ms,
// and the estimators of a step (3.6 ms of kernels and copies on the whole chip) then wait for nothing but the step's
// worldline.  _begin snapshots the worldlines (one device-to-device copy on the context's stream: 127 MB, ~50 us) and
// queues the estimator kernels on a SECOND stream of the context, on half the chip; the caller goes on -- typically
// with the next pigs_sampler_step -- and collects the results with _end.  Same kernels on the same bits as
// pigs_diagonal_estimators, hence the same results.  One batch can be pending per context.
// the kernels of the pending batch, on the second stream, once `gate` (an event of the first stream) has passed
static int launch_pending_estimators(pigs_ctx *c, hipEvent_t gate)
{
    if (!c->a_pend.on || c->a_pend.launched) return PIGS_OK;
    c->a_pend.launched = true;
    if (c->a_pend.b.n == 0) return PIGS_OK;
    HIPCHK(hipStreamWaitEvent(c->stream2, gate, 0));
    const int half = c->n_cu / 2 > 0 ? c->n_cu / 2 : 1;
    return est_launch(c, c->a_pend.b, c->d_shadow.p, c->a_buf, c->a_sw, c->a_sb, (double *)c->a_host.h, c->stream2, half);
}

int pigs_diagonal_estimators_begin(pigs_ctx *c, int32_t n, const int32_t *walkers, int32_t Nbin, double rbin, int32_t Nk,
                                   int32_t structure)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (c->a_pend.on) return fail(PIGS_ERR_ARG, "an estimator batch is pending: pigs_diagonal_estimators_end first");
    rc = check_cm(c); if (rc) return rc;
    EstBatch b;
    rc = est_describe(c, n, walkers, structure != 0, Nbin, rbin, Nk, b); if (rc) return rc;
    if (n > 0) {
        const size_t nd = c->path_doubles * (size_t)c->n_walkers;
        if (!c->stream2) HIPCHK(hipStreamCreateWithFlags(&c->stream2.h, hipStreamNonBlocking));
        if (!c->ev_snap) HIPCHK(hipEventCreateWithFlags(&c->ev_snap.h, hipEventDisableTiming));
        if (!c->ev_gate) HIPCHK(hipEventCreateWithFlags(&c->ev_gate.h, hipEventDisableTiming));
        HIPCHK(c->d_shadow.alloc(nd));
        HIPCHK(c->a_buf.reserve(b));
        HIPCHK(c->a_host.reserve(b.nres * sizeof(double)));
        est_slots(b, c->a_sw, c->a_sb);
        // the snapshot is ordered on the context's stream: after everything queued so far, before whatever comes next.
        // The kernels themselves are launched by the next pigs_sampler_step behind its TranslateChain kernel (which fills
        // the chip: estimators started beside it would only take CUs away from it) or, failing that, by _end.
        HIPCHK(hipMemcpyAsync(c->d_shadow.p, c->d_paths.p, nd * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipEventRecord(c->ev_snap, c->stream));
    }
    c->a_pend.b = std::move(b);
    c->a_pend.launched = false;
    c->a_pend.on = true;
    return PIGS_OK;
}

int pigs_diagonal_estimators_end(pigs_ctx *c, double *en, double *gr, double *Sk)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->a_pend.on) return fail(PIGS_ERR_ARG, "no estimator batch is pending: pigs_diagonal_estimators_begin first");
    const EstBatch &b = c->a_pend.b;
    if (b.n > 0 && (!en || (b.structure && (!gr || !Sk)))) return fail(PIGS_ERR_ARG, "null output");   // (still pending)
    rc = launch_pending_estimators(c, c->ev_snap);        // no sampler step came in between: start them now
    c->a_pend.on = false;
    if (rc || b.n == 0) return rc;
    HIPCHK(hipStreamSynchronize(c->stream2));
    rc = check_cm(c); if (rc) return rc;
    est_unpack(b, (const double *)c->a_host.h, en, gr, Sk);
    return PIGS_OK;
}

// ---- what the per-walker accumulator families below share -----------------------------------------
extern "C++" {      // templates

// *_init, once the request is accepted: no accumulate may be in flight on the buffers being replaced, and until the new
// ones stand the family counts as uninitialised (`ready` is the field its entry points test)
template <typename Flag>
static int init_begin(pigs_ctx *c, Flag &ready)
{
    HIPCHK(hipStreamSynchronize(c->stream));
    ready = Flag();
    return PIGS_OK;
}

// exactly n elements, and their zeroing queued on the context's stream
template <typename T>
static hipError_t alloc_zeroed(pigs_ctx *c, DevBuf<T> &b, size_t n)
{
    const hipError_t e = b.alloc(n);
    return e == hipSuccess ? hipMemsetAsync(b.p, 0, n * sizeof(T), c->stream) : e;
}

// *_accumulate: `launch(m, list)` for every launch that take_walkers (pigs_walker_split.h has the rule) cuts out of the
// checked list sw, at most `cap` walkers each; `walkers` is the caller's list (null: left out), `what` names the launcher
template <typename Launch>
static int each_launch(pigs_ctx *c, const std::vector<int32_t> &sw, const int32_t *walkers, bool unique, int cap,
                       const char *what, Launch launch)
{
    if (unique && walkers) c->list_marks.last.resize(c->n_walkers, 0);
    for (int i0 = 0; i0 < (int)sw.size();) {
        WalkerList L{};
        const int m = take_walkers(sw, walkers != nullptr, i0, cap, unique, c->list_marks, L);
        const hipError_t e = launch(m, L);
        if (e != hipSuccess) return fail(PIGS_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
        i0 += m;
    }
    return PIGS_OK;
}

} // extern "C++"

// *_read: one accumulator array of 8-byte elements, `per` of them per walker (0: an array that is switched off), walker-major,
// and where its copy goes
struct AccArray { void *dev; size_t per; void *host; };

// copy every array to the host, then zero the flagged walkers (one memset per array and run of consecutive walkers), wait
static int read_and_reset(pigs_ctx *c, std::initializer_list<AccArray> arrays, const int32_t *reset)
{
    const size_t W = (size_t)c->n_walkers, u = 8;
    hipStream_t s = c->stream;
    for (const AccArray &a : arrays)
        if (a.per) HIPCHK(hipMemcpyAsync(a.host, a.dev, W * a.per * u, hipMemcpyDeviceToHost, s));
    for (size_t w = 0; reset && w < W;) {
        if (!reset[w]) { ++w; continue; }
        size_t e = w;
        while (e < W && reset[e]) ++e;
        for (const AccArray &a : arrays)
            if (a.per) HIPCHK(hipMemsetAsync((char *)a.dev + w * a.per * u, 0, (e - w) * a.per * u, s));
        w = e;
    }
    SYNC_CHECKED(c);
    return PIGS_OK;
}

// pigs_{sqv,fqv,fqs}_count and _vectors: the family's nmax (0: not initialised) and Nq
static int grid_count(pigs_ctx *c, const char *family, int nmax, int64_t nq, int64_t *Nq)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!nmax) return fail(PIGS_ERR_ARG, "pigs_%s_init first", family);
    if (!Nq) return fail(PIGS_ERR_ARG, "null output");
    *Nq = nq;
    return PIGS_OK;
}

// vector iqv has rank iqv + Nq + 1 among all (2 nmax + 1)^dim vectors, n_1 slowest (include/pigs_hip.h)
static int grid_vectors(pigs_ctx *c, const char *family, int nmax, int64_t nq, int32_t *n)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!nmax) return fail(PIGS_ERR_ARG, "pigs_%s_init first", family);
    if (!n) return fail(PIGS_ERR_ARG, "null output");
    const int dim = c->P.dim, S = 2 * nmax + 1;
    for (int64_t iqv = 0; iqv < nq; ++iqv) {
        int64_t r = iqv + nq + 1;
        for (int k = dim - 1; k >= 0; --k) {
            n[iqv * dim + k] = (int32_t)(r % S) - nmax;
            r /= S;
        }
    }
    return PIGS_OK;
}

// ---- density profiles of a trapped system ------------------------------------------------------
// Three per-walker histograms of slice Nb (pigs_density.hip) accumulated on the device and read per block.  The widths
// are computed here, once, in double: b = (2h)/Nbin for the planar grid over [-h, h), br = h/Nbin for r and d in [0, h).
int pigs_density_init(pigs_ctx *c, int32_t Nbin, double half_width)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "density profiles are defined for trapped systems only");
    if (Nbin < 1 || !(half_width > 0.0)) return fail(PIGS_ERR_ARG, "pigs_density_init: Nbin=%d half_width=%g", Nbin, half_width);
    const int dp = c->P.dim < 2 ? c->P.dim : 2;
    size_t np = 1;
    for (int k = 0; k < dp; ++k) np *= (size_t)Nbin;
    const size_t W = (size_t)c->n_walkers;
    rc = init_begin(c, c->dens_nbin); if (rc) return rc;
    HIPCHK(alloc_zeroed(c, c->d_dplanar, W * np));
    HIPCHK(alloc_zeroed(c, c->d_dradial, W * Nbin));
    HIPCHK(alloc_zeroed(c, c->d_dpair, W * Nbin));
    HIPCHK(alloc_zeroed(c, c->d_dsamples, W));
    SYNC_CHECKED(c);
    c->dens_nbin = Nbin;
    c->dens_nplanar = np;
    c->dens_h = half_width;
    c->dens_b = (2.0 * half_width) / Nbin;
    c->dens_br = half_width / Nbin;
    return PIGS_OK;
}

int pigs_density_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->dens_nbin) return fail(PIGS_ERR_ARG, "pigs_density_init first");
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    // integer atomics: a walker may appear twice in one launch
    return each_launch(c, sw, walkers, false, kWalkerListMax, "launch_density", [&](int m, const WalkerList &L) {
        return launch_density(c->P, c->d_paths.p, m, L, c->dens_nbin, c->dens_h, c->dens_b, c->dens_br, c->d_dplanar.p,
                              c->d_dradial.p, c->d_dpair.p, c->d_dsamples.p, c->stream);
    });
}

int pigs_density_read(pigs_ctx *c, int64_t *planar, int64_t *radial, int64_t *pair, int64_t *samples, const int32_t *reset)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->dens_nbin) return fail(PIGS_ERR_ARG, "pigs_density_init first");
    if (!planar || !radial || !pair || !samples) return fail(PIGS_ERR_ARG, "null output");
    const size_t nb = (size_t)c->dens_nbin;
    return read_and_reset(c, {{c->d_dplanar.p, c->dens_nplanar, planar}, {c->d_dradial.p, nb, radial}, {c->d_dpair.p, nb, pair},
                              {c->d_dsamples.p, 1, samples}}, reset);
}

// ---- imaginary-time density correlations F(q,tau) of a periodic system ---------------------------
// Raw sums per walker, lag, harmonic and axis (pigs_fqt.hip), accumulated on the device and read per block.
int pigs_fqt_init(pigs_ctx *c, int32_t Nk, int32_t Ntau, int32_t window)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "F(q,tau) is defined for periodic systems only (the q grid is the box's)");
    if (Nk < 1 || window < 0 || window > c->P.Nb || Ntau < 0 || Ntau > 2 * window)
        return fail(PIGS_ERR_ARG, "pigs_fqt_init: Nk=%d Ntau=%d window=%d (Nb=%d)", Nk, Ntau, window, c->P.Nb);
    const size_t W = (size_t)c->n_walkers, per = (size_t)(Ntau + 1) * Nk * c->P.dim;
    const int slots = std::min(c->n_walkers, kWalkerListMax);
    rc = init_begin(c, c->fqt_nk); if (rc) return rc;
    HIPCHK(alloc_zeroed(c, c->d_fqt_acc, W * per));
    HIPCHK(alloc_zeroed(c, c->d_fqt_samples, W));
    HIPCHK(c->d_fqt_rho.alloc((size_t)slots * (2 * window + 1) * 2 * Nk * c->P.dim));
    SYNC_CHECKED(c);
    c->fqt_nk = Nk;
    c->fqt_ntau = Ntau;
    c->fqt_window = window;
    c->fqt_slots = slots;
    return PIGS_OK;
}

int pigs_fqt_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (!c->fqt_nk) return fail(PIGS_ERR_ARG, "pigs_fqt_init first");
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    // one thread owns an accumulator element per launch, and the scratch holds fqt_slots walkers
    return each_launch(c, sw, walkers, true, c->fqt_slots, "launch_fqt", [&](int m, const WalkerList &L) {
        return launch_fqt(c->P, c->d_paths.p, m, L, c->fqt_window, c->fqt_ntau, c->fqt_nk, c->d_fqt_rho.p, c->d_fqt_acc.p,
                          c->d_fqt_samples.p, c->stream);
    });
}

int pigs_fqt_read(pigs_ctx *c, double *F, int64_t *samples, const int32_t *reset)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->fqt_nk) return fail(PIGS_ERR_ARG, "pigs_fqt_init first");
    if (!F || !samples) return fail(PIGS_ERR_ARG, "null output");
    const size_t per = (size_t)(c->fqt_ntau + 1) * c->fqt_nk * c->P.dim;
    return read_and_reset(c, {{c->d_fqt_acc.p, per, F}, {c->d_fqt_samples.p, 1, samples}}, reset);
}

// ---- imaginary-time profiles: V(tau), the virial and the link lengths of every slice --------------
// Raw sums per walker, slice and quantity (pigs_tau.hip), accumulated on the device and read per block.
int pigs_tau_init(pigs_ctx *c)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    const size_t W = (size_t)c->n_walkers, per = (size_t)c->P.M * 4;
    rc = init_begin(c, c->tau_ready); if (rc) return rc;
    HIPCHK(alloc_zeroed(c, c->d_tau_acc, W * per));
    HIPCHK(alloc_zeroed(c, c->d_tau_samples, W));
    SYNC_CHECKED(c);
    c->tau_ready = true;
    return PIGS_OK;
}

int pigs_tau_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (!c->tau_ready) return fail(PIGS_ERR_ARG, "pigs_tau_init first");
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    // one workgroup owns an accumulator element per launch
    return each_launch(c, sw, walkers, true, kWalkerListMax, "launch_tau", [&](int m, const WalkerList &L) {
        return launch_tau(c->P, c->d_paths.p, c->d_VT.p, m, L, c->d_tau_acc.p, c->d_tau_samples.p, c->stream);
    });
}

int pigs_tau_read(pigs_ctx *c, double *Q, int64_t *samples, const int32_t *reset)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->tau_ready) return fail(PIGS_ERR_ARG, "pigs_tau_init first");
    if (!Q || !samples) return fail(PIGS_ERR_ARG, "null output");
    return read_and_reset(c, {{c->d_tau_acc.p, (size_t)c->P.M * 4, Q}, {c->d_tau_samples.p, 1, samples}}, reset);
}

// ---- vector structure factor S(q) on the full reciprocal grid of a periodic system ----------------
// Raw sums per walker and vector (pigs_sqv.hip), accumulated on the device and read per block.
constexpr size_t kSqvScratchMax = (size_t)256 << 20;      // bytes of slice scratch behind one launch

int pigs_sqv_init(pigs_ctx *c, int32_t nmax, int32_t window)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the vector S(q) is defined for periodic systems only (the q grid is the box's)");
    if (nmax < 1 || nmax > (c->P.dim == 3 ? 16 : 64) || window < 0 || window > c->P.Nb)
        return fail(PIGS_ERR_ARG, "pigs_sqv_init: nmax=%d (1..%d in %dD) window=%d (0..Nb=%d)", nmax, c->P.dim == 3 ? 16 : 64,
                    c->P.dim, window, c->P.Nb);
    const SqvShape sh = sqv_shape(c->P.dim, nmax);
    const size_t W = (size_t)c->n_walkers, per = (size_t)sh.Nq, slice = (size_t)(2 * window + 1) * per;
    // as many walkers per launch as the list holds and the scratch cap allows, one at the least
    const int slots = (int)std::max<size_t>(1, std::min<size_t>(std::min(c->n_walkers, kWalkerListMax),
                                                                kSqvScratchMax / (slice * sizeof(double))));
    rc = init_begin(c, c->sqv_nmax); if (rc) return rc;
    HIPCHK(alloc_zeroed(c, c->d_sqv_acc, W * per));
    HIPCHK(alloc_zeroed(c, c->d_sqv_samples, W));
    HIPCHK(c->d_sqv_rho2.alloc((size_t)slots * slice));
    SYNC_CHECKED(c);
    c->sqv_nmax = nmax;
    c->sqv_window = window;
    c->sqv_slots = slots;
    c->sqv_nq = sh.Nq;
    return PIGS_OK;
}

int pigs_sqv_count(pigs_ctx *c, int64_t *Nq)
{
    return c ? grid_count(c, "sqv", c->sqv_nmax, c->sqv_nq, Nq) : fail(PIGS_ERR_ARG, "null context");
}

int pigs_sqv_vectors(pigs_ctx *c, int32_t *n)
{
    return c ? grid_vectors(c, "sqv", c->sqv_nmax, c->sqv_nq, n) : fail(PIGS_ERR_ARG, "null context");
}

int pigs_sqv_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (!c->sqv_nmax) return fail(PIGS_ERR_ARG, "pigs_sqv_init first");
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    // one thread owns an accumulator element per launch, and the scratch holds sqv_slots walkers
    return each_launch(c, sw, walkers, true, c->sqv_slots, "launch_sqv", [&](int m, const WalkerList &L) {
        return launch_sqv(c->P, c->d_paths.p, m, L, c->sqv_window, c->sqv_nmax, c->d_sqv_rho2.p, c->d_sqv_acc.p,
                          c->d_sqv_samples.p, c->stream);
    });
}

int pigs_sqv_read(pigs_ctx *c, double *S, int64_t *samples, const int32_t *reset)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->sqv_nmax) return fail(PIGS_ERR_ARG, "pigs_sqv_init first");
    if (!S || !samples) return fail(PIGS_ERR_ARG, "null output");
    return read_and_reset(c, {{c->d_sqv_acc.p, (size_t)c->sqv_nq, S}, {c->d_sqv_samples.p, 1, samples}}, reset);
}

// ---- F(q,tau) on the full reciprocal grid of a periodic system -----------------------------------
// Raw sums per walker, lag and vector (pigs_fqv.hip): the vectors of pigs_sqv_*, the window and lags of pigs_fqt_*.
int pigs_fqv_init(pigs_ctx *c, int32_t nmax, int32_t Ntau, int32_t window)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the vector F(q,tau) is defined for periodic systems only (the q grid is the box's)");
    if (nmax < 1 || nmax > (c->P.dim == 3 ? 16 : 64) || window < 0 || window > c->P.Nb || Ntau < 0 || Ntau > 2 * window)
        return fail(PIGS_ERR_ARG, "pigs_fqv_init: nmax=%d (1..%d in %dD) Ntau=%d (0..2 window) window=%d (0..Nb=%d)", nmax,
                    c->P.dim == 3 ? 16 : 64, c->P.dim, Ntau, window, c->P.Nb);
    if (!fqv_width(2 * window + 1))
        return fail(PIGS_ERR_ARG, "pigs_fqv_init: %d window slices of one vector pass the %zu bytes of LDS staging", 2 * window + 1,
                    kFqvLdsBudget);
    const SqvShape sh = sqv_shape(c->P.dim, nmax);
    const size_t W = (size_t)c->n_walkers, per = (size_t)(Ntau + 1) * (size_t)sh.Nq;
    const size_t slice = (size_t)(2 * window + 1) * 2 * (size_t)sh.Nq;
    if ((double)W * ((double)per + 1.0) * 8.0 > 2147483648.0)
        return fail(PIGS_ERR_ARG, "pigs_fqv_init: %zu walkers x (%d x %lld + 1) sums pass 2 GiB", W, Ntau + 1, (long long)sh.Nq);
    // as many walkers per launch as the list holds and the scratch cap (that of pigs_sqv_*) allows, one at the least
    const int slots = (int)std::max<size_t>(1, std::min<size_t>(std::min(c->n_walkers, kWalkerListMax),
                                                                kSqvScratchMax / (slice * sizeof(double))));
    rc = init_begin(c, c->fqv_nmax); if (rc) return rc;
    HIPCHK(alloc_zeroed(c, c->d_fqv_acc, W * per));
    HIPCHK(alloc_zeroed(c, c->d_fqv_samples, W));
    HIPCHK(c->d_fqv_rho.alloc((size_t)slots * slice));
    SYNC_CHECKED(c);
    c->fqv_nmax = nmax;
    c->fqv_ntau = Ntau;
    c->fqv_window = window;
    c->fqv_slots = slots;
    c->fqv_nq = sh.Nq;
    return PIGS_OK;
}

int pigs_fqv_count(pigs_ctx *c, int64_t *Nq)
{
    return c ? grid_count(c, "fqv", c->fqv_nmax, c->fqv_nq, Nq) : fail(PIGS_ERR_ARG, "null context");
}

int pigs_fqv_vectors(pigs_ctx *c, int32_t *n)
{
    return c ? grid_vectors(c, "fqv", c->fqv_nmax, c->fqv_nq, n) : fail(PIGS_ERR_ARG, "null context");
}

int pigs_fqv_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (!c->fqv_nmax) return fail(PIGS_ERR_ARG, "pigs_fqv_init first");
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    // one thread owns an accumulator element per launch, and the scratch holds fqv_slots walkers
    return each_launch(c, sw, walkers, true, c->fqv_slots, "launch_fqv", [&](int m, const WalkerList &L) {
        return launch_fqv(c->P, c->d_paths.p, m, L, c->fqv_window, c->fqv_ntau, c->fqv_nmax, c->d_fqv_rho.p, c->d_fqv_acc.p,
                          c->d_fqv_samples.p, c->stream);
    });
}

int pigs_fqv_read(pigs_ctx *c, double *F, int64_t *samples, const int32_t *reset)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->fqv_nmax) return fail(PIGS_ERR_ARG, "pigs_fqv_init first");
    if (!F || !samples) return fail(PIGS_ERR_ARG, "null output");
    const size_t per = (size_t)(c->fqv_ntau + 1) * (size_t)c->fqv_nq;
    return read_and_reset(c, {{c->d_fqv_acc.p, per, F}, {c->d_fqv_samples.p, 1, samples}}, reset);
}

// ---- self part of F(q,tau) and the imaginary-time displacement of a periodic system ---------------
// Raw sums per walker, lag and vector, and per walker and lag (pigs_fqs.hip): the vectors, window and lags of pigs_fqv_*.
int pigs_fqs_init(pigs_ctx *c, int32_t nmax, int32_t Ntau, int32_t window)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the self part of F(q,tau) is defined for periodic systems only (the q grid is the box's)");
    if (nmax < 1 || nmax > (c->P.dim == 3 ? 16 : 64) || window < 0 || window > c->P.Nb || Ntau < 0 || Ntau > 2 * window)
        return fail(PIGS_ERR_ARG, "pigs_fqs_init: nmax=%d (1..%d in %dD) Ntau=%d (0..2 window) window=%d (0..Nb=%d)", nmax,
                    c->P.dim == 3 ? 16 : 64, c->P.dim, Ntau, window, c->P.Nb);
    if (!fqs_shape(c->P.dim, nmax, window, Ntau).width)
        return fail(PIGS_ERR_ARG, "pigs_fqs_init: the phasors of %d window slices (nmax=%d, %dD) pass the %zu bytes of LDS, or %d lags"
                    " the %d a workgroup takes", 2 * window + 1, nmax, c->P.dim, kFqsLdsBudget, Ntau + 1, kFqsThreads * kFqsLags);
    const SqvShape sh = sqv_shape(c->P.dim, nmax);
    const size_t W = (size_t)c->n_walkers, per = (size_t)(Ntau + 1) * (size_t)sh.Nq, perd = (size_t)(Ntau + 1) * 2;
    if ((double)W * ((double)per + (double)perd + 1.0) * 8.0 > 2147483648.0)
        return fail(PIGS_ERR_ARG, "pigs_fqs_init: %zu walkers x (%d x (%lld + 2) + 1) sums pass 2 GiB", W, Ntau + 1, (long long)sh.Nq);
    rc = init_begin(c, c->fqs_nmax); if (rc) return rc;
    HIPCHK(alloc_zeroed(c, c->d_fqs_acc, W * per));
    HIPCHK(alloc_zeroed(c, c->d_fqs_dsp, W * perd));
    HIPCHK(alloc_zeroed(c, c->d_fqs_samples, W));
    SYNC_CHECKED(c);
    c->fqs_nmax = nmax;
    c->fqs_ntau = Ntau;
    c->fqs_window = window;
    c->fqs_nq = sh.Nq;
    return PIGS_OK;
}

int pigs_fqs_count(pigs_ctx *c, int64_t *Nq)
{
    return c ? grid_count(c, "fqs", c->fqs_nmax, c->fqs_nq, Nq) : fail(PIGS_ERR_ARG, "null context");
}

int pigs_fqs_vectors(pigs_ctx *c, int32_t *n)
{
    return c ? grid_vectors(c, "fqs", c->fqs_nmax, c->fqs_nq, n) : fail(PIGS_ERR_ARG, "null context");
}

int pigs_fqs_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (!c->fqs_nmax) return fail(PIGS_ERR_ARG, "pigs_fqs_init first");
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    // one thread owns an accumulator element per launch
    return each_launch(c, sw, walkers, true, kWalkerListMax, "launch_fqs", [&](int m, const WalkerList &L) {
        return launch_fqs(c->P, c->d_paths.p, m, L, c->fqs_window, c->fqs_ntau, c->fqs_nmax, c->d_fqs_acc.p, c->d_fqs_dsp.p,
                          c->d_fqs_samples.p, c->stream);
    });
}

int pigs_fqs_read(pigs_ctx *c, double *F, double *D, int64_t *samples, const int32_t *reset)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->fqs_nmax) return fail(PIGS_ERR_ARG, "pigs_fqs_init first");
    if (!F || !D || !samples) return fail(PIGS_ERR_ARG, "null output");
    const size_t per = (size_t)(c->fqs_ntau + 1) * (size_t)c->fqs_nq, perd = (size_t)(c->fqs_ntau + 1) * 2;
    return read_and_reset(c, {{c->d_fqs_acc.p, per, F}, {c->d_fqs_dsp.p, perd, D}, {c->d_fqs_samples.p, 1, samples}}, reset);
}

// ---- pair distribution of a periodic system on the vector grid, over a slice window ---------------
// Integer counts per walker (pigs_grv.hip), accumulated on the device and read per block.
int pigs_grv_init(pigs_ctx *c, int32_t Nbin, int32_t Nr, double rbin, int32_t window)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the vector g(r) is defined for periodic systems only (its grid is the box's)");
    const int nbmax = c->P.dim == 3 ? 128 : c->P.dim == 2 ? 1024 : 4096;
    if (Nbin < 1 || Nbin > nbmax || Nr < 1 || !(rbin > 0.0) || !std::isfinite(rbin) || window < 0 || window > c->P.Nb)
        return fail(PIGS_ERR_ARG, "pigs_grv_init: Nbin=%d (1..%d in %dD) Nr=%d rbin=%g window=%d (0..Nb=%d)", Nbin, nbmax,
                    c->P.dim, Nr, rbin, window, c->P.Nb);
    size_t nv = 1;
    for (int k = 0; k < c->P.dim; ++k) nv *= (size_t)Nbin;
    const size_t W = (size_t)c->n_walkers;
    const double bytes = (double)W * ((double)nv + (double)Nr + 1.0) * 8.0;
    if (bytes > 2147483648.0)
        return fail(PIGS_ERR_ARG, "pigs_grv_init: %zu walkers x (%zu + %d + 1) counters pass 2 GiB", W, nv, Nr);
    rc = init_begin(c, c->grv_nbin); if (rc) return rc;
    HIPCHK(alloc_zeroed(c, c->d_grv_vec, W * nv));
    HIPCHK(alloc_zeroed(c, c->d_grv_radial, W * Nr));
    HIPCHK(alloc_zeroed(c, c->d_grv_samples, W));
    SYNC_CHECKED(c);
    c->grv_nbin = Nbin;
    c->grv_nr = Nr;
    c->grv_window = window;
    c->grv_nvec = nv;
    c->grv_rbin = rbin;
    return PIGS_OK;
}

int pigs_grv_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (!c->grv_nbin) return fail(PIGS_ERR_ARG, "pigs_grv_init first");
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    // integer atomics: a walker may appear twice in one launch.  The form follows from the launch's size; a forced LDS
    // form that does not fit is refused at that launch, the launches before it stay queued.
    bool fits = true;
    rc = each_launch(c, sw, walkers, false, kWalkerListMax, "launch_grv", [&](int m, const WalkerList &L) {
        const GrvShape sh = grv_shape(c->P.dim, c->P.Np, c->grv_nbin, c->grv_nr, c->grv_window, c->grv_form, m, c->n_cu);
        fits = !(sh.vec_lds && !sh.vec_fits);
        if (!fits) return hipErrorInvalidValue;
        return launch_grv(c->P, c->d_paths.p, m, L, sh, c->grv_window, c->grv_nbin, c->grv_nr, c->grv_rbin, c->d_grv_vec.p,
                          c->d_grv_radial.p, c->d_grv_samples.p, c->stream);
    });
    if (!fits) return fail(PIGS_ERR_ARG, "pigs_grv_accumulate: grv_form = 1, but a grid of %zu bins does not fit the LDS", c->grv_nvec);
    return rc;
}

int pigs_grv_read(pigs_ctx *c, int64_t *vec, int64_t *radial, int64_t *samples, const int32_t *reset)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->grv_nbin) return fail(PIGS_ERR_ARG, "pigs_grv_init first");
    if (!vec || !radial || !samples) return fail(PIGS_ERR_ARG, "null output");
    return read_and_reset(c, {{c->d_grv_vec.p, c->grv_nvec, vec}, {c->d_grv_radial.p, (size_t)c->grv_nr, radial},
                              {c->d_grv_samples.p, 1, samples}}, reset);
}

// ---- bond-orientational order of a periodic system over a slice window ---------------------------
// Raw sums and integer counts per walker (pigs_bop.hip), accumulated on the device and read per block.
int pigs_bop_init(pigs_ctx *c, double rnb, int32_t window, int32_t Nh, int32_t Nr, double rbin)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "bond-orientational order is defined for periodic systems only (bonds are minimum images)");
    if (c->P.dim < 2) return fail(PIGS_ERR_UNSUPPORTED, "bond-orientational order is defined in 2D and 3D only");
    bool rnb_ok = std::isfinite(rnb) && rnb > 0.0;
    for (int k = 0; k < c->P.dim; ++k) rnb_ok = rnb_ok && rnb <= c->P.LboxHalf[k];
    if (!rnb_ok || window < 0 || window > c->P.Nb || Nh < 1 || Nh > kBopHistMax || Nr < 0 ||
        (Nr > 0 && (!(rbin > 0.0) || !std::isfinite(rbin))))
        return fail(PIGS_ERR_ARG, "pigs_bop_init: rnb=%g (0 < rnb <= half the shortest side) window=%d (0..Nb=%d) Nh=%d (1..%d) Nr=%d rbin=%g",
                    rnb, window, c->P.Nb, Nh, kBopHistMax, Nr, rbin);
    if (Nr > 0 && c->P.Np > kBopNpMax)
        return fail(PIGS_ERR_ARG, "pigs_bop_init: Np=%d passes %d, where a fixed-point bin of G6(r) could overflow", c->P.Np, kBopNpMax);
    const size_t lds = bop_lds_bytes(c->P.dim, c->P.Np, Nr);
    if (lds > kBopLdsBudget)
        return fail(PIGS_ERR_ARG, "pigs_bop_init: Np=%d Nr=%d need %zu bytes of LDS for one slice (%zu at most)", c->P.Np, Nr, lds,
                    kBopLdsBudget);
    const size_t W = (size_t)c->n_walkers, per = (size_t)8 + Nr;
    const int slots = std::min(c->n_walkers, kWalkerListMax);
    rc = init_begin(c, c->bop_nh); if (rc) return rc;
    HIPCHK(alloc_zeroed(c, c->d_bop_S, W * 8));
    HIPCHK(alloc_zeroed(c, c->d_bop_H, W * 2 * Nh));
    HIPCHK(alloc_zeroed(c, c->d_bop_G, W * std::max(Nr, 1)));
    HIPCHK(alloc_zeroed(c, c->d_bop_GN, W * std::max(Nr, 1)));
    HIPCHK(alloc_zeroed(c, c->d_bop_samples, W));
    HIPCHK(c->d_bop_scratch.alloc((size_t)slots * (2 * window + 1) * per));
    SYNC_CHECKED(c);
    c->bop_nh = Nh;
    c->bop_nr = Nr;
    c->bop_window = window;
    c->bop_slots = slots;
    c->bop_rnb2 = rnb * rnb;
    c->bop_rbin = Nr > 0 ? rbin : 1.0;
    return PIGS_OK;
}

int pigs_bop_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (!c->bop_nh) return fail(PIGS_ERR_ARG, "pigs_bop_init first");
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    // one thread owns an accumulator element per launch, and the scratch holds bop_slots walkers
    return each_launch(c, sw, walkers, true, c->bop_slots, "launch_bop", [&](int m, const WalkerList &L) {
        return launch_bop(c->P, c->d_paths.p, m, L, c->bop_window, c->bop_nh, c->bop_nr, c->bop_rnb2, c->bop_rbin,
                          c->d_bop_scratch.p, c->d_bop_S.p, c->d_bop_H.p, c->d_bop_G.p, c->d_bop_GN.p, c->d_bop_samples.p,
                          c->stream);
    });
}

int pigs_bop_read(pigs_ctx *c, double *S, int64_t *H, double *G, int64_t *GN, int64_t *samples, const int32_t *reset)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->bop_nh) return fail(PIGS_ERR_ARG, "pigs_bop_init first");
    if (!S || !H || !samples || (c->bop_nr > 0 && (!G || !GN))) return fail(PIGS_ERR_ARG, "null output");
    const size_t nr = (size_t)c->bop_nr;
    return read_and_reset(c, {{c->d_bop_S.p, 8, S}, {c->d_bop_H.p, (size_t)2 * c->bop_nh, H}, {c->d_bop_G.p, nr, G},
                              {c->d_bop_GN.p, nr, GN}, {c->d_bop_samples.p, 1, samples}}, reset);
}

// ---- van Hove functions G_s(r,tau), G_d(r,tau) of a periodic system over a slice window -----------
// Integer counts per walker and lag (pigs_vh.hip), accumulated on the device and read per block.
int pigs_vh_init(pigs_ctx *c, int32_t Ntau, int32_t window, int32_t Nr, double rbin, int32_t Ns, double sbin)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the van Hove functions are defined for periodic systems only (their displacements are minimum images)");
    if (Nr < 1 || Ns < 1 || !(rbin > 0.0) || !std::isfinite(rbin) || !(sbin > 0.0) || !std::isfinite(sbin) || window < 0 ||
        window > c->P.Nb || Ntau < 0 || Ntau > 2 * window)
        return fail(PIGS_ERR_ARG, "pigs_vh_init: Ntau=%d (0..2 window) window=%d (0..Nb=%d) Nr=%d rbin=%g Ns=%d sbin=%g", Ntau, window,
                    c->P.Nb, Nr, rbin, Ns, sbin);
    const size_t W = (size_t)c->n_walkers, nl = (size_t)Ntau + 1;
    if ((double)W * ((double)nl * ((double)Nr + (double)Ns) + 1.0) * 8.0 > 2147483648.0)
        return fail(PIGS_ERR_ARG, "pigs_vh_init: %zu walkers x (%zu x (%d + %d) + 1) counters pass 2 GiB", W, nl, Nr, Ns);
    if (!vh_shape(c->P.dim, c->P.Np, Ntau, Nr, Ns, 0).slice_fits)
        return fail(PIGS_ERR_ARG, "pigs_vh_init: a slice of Np=%d particles in %dD needs %zu bytes of LDS (%zu at most)", c->P.Np,
                    c->P.dim, sizeof(double) * (size_t)c->P.dim * (size_t)c->P.Np, kVhLdsBudget);
    rc = init_begin(c, c->vh_nr); if (rc) return rc;
    HIPCHK(alloc_zeroed(c, c->d_vh_self, W * nl * Ns));
    HIPCHK(alloc_zeroed(c, c->d_vh_dist, W * nl * Nr));
    HIPCHK(alloc_zeroed(c, c->d_vh_samples, W));
    SYNC_CHECKED(c);
    c->vh_nr = Nr;
    c->vh_ns = Ns;
    c->vh_ntau = Ntau;
    c->vh_window = window;
    c->vh_rbin = rbin;
    c->vh_sbin = sbin;
    return PIGS_OK;
}

int pigs_vh_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (!c->vh_nr) return fail(PIGS_ERR_ARG, "pigs_vh_init first");
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    // a forced LDS form that does not fit is refused before anything is queued
    const VhShape sh = vh_shape(c->P.dim, c->P.Np, c->vh_ntau, c->vh_nr, c->vh_ns, c->vh_form);
    if (sh.hist_lds && !sh.hist_fits)
        return fail(PIGS_ERR_ARG, "pigs_vh_accumulate: vh_form = 1, but %d x (%d + %d) counters do not fit the LDS beside the slice",
                    c->vh_ntau + 1, c->vh_nr, c->vh_ns);
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    // integer atomics: a walker may appear twice in one launch
    return each_launch(c, sw, walkers, false, kWalkerListMax, "launch_vh", [&](int m, const WalkerList &L) {
        return launch_vh(c->P, c->d_paths.p, m, L, sh, c->vh_window, c->vh_ntau, c->vh_nr, c->vh_rbin, c->vh_ns, c->vh_sbin,
                         c->d_vh_self.p, c->d_vh_dist.p, c->d_vh_samples.p, c->stream);
    });
}

int pigs_vh_read(pigs_ctx *c, int64_t *self, int64_t *dist, int64_t *samples, const int32_t *reset)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->vh_nr) return fail(PIGS_ERR_ARG, "pigs_vh_init first");
    if (!self || !dist || !samples) return fail(PIGS_ERR_ARG, "null output");
    const size_t nl = (size_t)c->vh_ntau + 1;
    return read_and_reset(c, {{c->d_vh_self.p, nl * c->vh_ns, self}, {c->d_vh_dist.p, nl * c->vh_nr, dist},
                              {c->d_vh_samples.p, 1, samples}}, reset);
}

// ---- triplet distribution g3(r, s, cos theta) of a periodic system over a slice window ------------
// Integer counts per walker (pigs_g3.hip), accumulated on the device and read per block.
int pigs_g3_init(pigs_ctx *c, int32_t Nr, double rbin, int32_t Na, int32_t window)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the triplet distribution is defined for periodic systems only (its legs are minimum images)");
    if (c->P.dim < 2) return fail(PIGS_ERR_UNSUPPORTED, "the triplet distribution is defined in 2D and 3D only");
    if (Nr < 1 || Nr > kG3GridMax || Na < 1 || Na > kG3GridMax || !(rbin > 0.0) || !std::isfinite(rbin) || window < 0 ||
        window > c->P.Nb)
        return fail(PIGS_ERR_ARG, "pigs_g3_init: Nr=%d Na=%d (1..%d) rbin=%g window=%d (0..Nb=%d)", Nr, Na, kG3GridMax, rbin, window,
                    c->P.Nb);
    // rbin = (half a side) / Nr is the natural call, and Nr rbin may then round a few ulps past the half side
    const double rmax = (double)Nr * rbin;
    bool rmax_ok = std::isfinite(rmax);
    for (int k = 0; k < c->P.dim; ++k) rmax_ok = rmax_ok && rmax <= c->P.LboxHalf[k] * (1.0 + 4.0 * DBL_EPSILON);
    if (!rmax_ok) return fail(PIGS_ERR_ARG, "pigs_g3_init: rmax = Nr rbin = %g (0 < rmax <= half the shortest side)", rmax);
    const size_t W = (size_t)c->n_walkers, ntrip = (size_t)Nr * ((size_t)Nr + 1) / 2 * (size_t)Na;
    if ((double)W * ((double)ntrip + (double)Nr + 1.0) * 8.0 > 2147483648.0)
        return fail(PIGS_ERR_ARG, "pigs_g3_init: %zu walkers x (%zu + %d + 1) counters pass 2 GiB", W, ntrip, Nr);
    const G3Shape sh = g3_shape(c->P.dim, c->P.Np, Nr, Na, 0);
    if (!sh.fits)
        return fail(PIGS_ERR_ARG, "pigs_g3_init: a slice of Np=%d particles in %dD and its leg lists need %zu bytes of LDS (%zu at most)",
                    c->P.Np, c->P.dim, sh.lds, kG3LdsBudget);
    rc = init_begin(c, c->g3_nr); if (rc) return rc;
    HIPCHK(alloc_zeroed(c, c->d_g3_trip, W * ntrip));
    HIPCHK(alloc_zeroed(c, c->d_g3_pair, W * Nr));
    HIPCHK(alloc_zeroed(c, c->d_g3_samples, W));
    SYNC_CHECKED(c);
    c->g3_nr = Nr;
    c->g3_na = Na;
    c->g3_window = window;
    c->g3_rbin = rbin;
    return PIGS_OK;
}

int pigs_g3_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (!c->g3_nr) return fail(PIGS_ERR_ARG, "pigs_g3_init first");
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    // a forced LDS form that does not fit is refused before anything is queued
    const G3Shape sh = g3_shape(c->P.dim, c->P.Np, c->g3_nr, c->g3_na, c->g3_form);
    if (sh.hist_lds && !sh.hist_fits)
        return fail(PIGS_ERR_ARG, "pigs_g3_accumulate: g3_form = 1, but %d x %d x %d / 2 counters do not fit the LDS beside the slice and the leg lists",
                    c->g3_nr, c->g3_nr + 1, c->g3_na);
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    // integer atomics: a walker may appear twice in one launch
    return each_launch(c, sw, walkers, false, kWalkerListMax, "launch_g3", [&](int m, const WalkerList &L) {
        return launch_g3(c->P, c->d_paths.p, m, L, sh, c->g3_window, c->g3_nr, c->g3_rbin, c->g3_na, c->d_g3_trip.p,
                         c->d_g3_pair.p, c->d_g3_samples.p, c->stream);
    });
}

int pigs_g3_read(pigs_ctx *c, int64_t *trip, int64_t *pair, int64_t *samples, const int32_t *reset)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->g3_nr) return fail(PIGS_ERR_ARG, "pigs_g3_init first");
    if (!trip || !pair || !samples) return fail(PIGS_ERR_ARG, "null output");
    const size_t ntrip = (size_t)c->g3_nr * ((size_t)c->g3_nr + 1) / 2 * (size_t)c->g3_na;
    return read_and_reset(c, {{c->d_g3_trip.p, ntrip, trip}, {c->d_g3_pair.p, (size_t)c->g3_nr, pair},
                              {c->d_g3_samples.p, 1, samples}}, reset);
}

// ---- Axilrod-Teller-Muto three-body geometric sum of a periodic system over a slice window -------
// Raw sums per walker and window slice (pigs_atm.hip), accumulated on the device and read per block.
int pigs_atm_init(pigs_ctx *c, double rc, int32_t window)
{
    int rc_ = check_ctx(c); if (rc_) return rc_;
    rc_ = check_cm(c); if (rc_) return rc_;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the three-body energy is defined for periodic systems only (its sides are minimum images)");
    if (c->P.dim < 2) return fail(PIGS_ERR_UNSUPPORTED, "the three-body energy is defined in 2D and 3D only");
    if (!(rc > 0.0) || !std::isfinite(rc) || window < 0 || window > c->P.Nb)
        return fail(PIGS_ERR_ARG, "pigs_atm_init: rc=%g window=%d (0..Nb=%d)", rc, window, c->P.Nb);
    for (int k = 0; k < c->P.dim; ++k)
        if (!(rc <= c->P.LboxHalf[k]))
            return fail(PIGS_ERR_ARG, "pigs_atm_init: rc = %g (0 < rc <= half the shortest side)", rc);
    const AtmShape sh = atm_shape(c->P.dim, c->P.Np);
    if (!sh.fits)
        return fail(PIGS_ERR_ARG, "pigs_atm_init: a slice of Np=%d particles in %dD and its leg lists need %zu bytes of LDS (%zu at most)",
                    c->P.Np, c->P.dim, sh.lds, kAtmLdsBudget);
    const size_t W = (size_t)c->n_walkers, per = 2 * (size_t)window + 1;
    rc_ = init_begin(c, c->atm_ready); if (rc_) return rc_;
    HIPCHK(alloc_zeroed(c, c->d_atm_T, W * per));
    HIPCHK(alloc_zeroed(c, c->d_atm_ntrip, W * per));
    HIPCHK(alloc_zeroed(c, c->d_atm_samples, W));
    SYNC_CHECKED(c);
    c->atm_window = window;
    c->atm_rc2 = rc * rc;
    c->atm_ready = true;
    return PIGS_OK;
}

int pigs_atm_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (!c->atm_ready) return fail(PIGS_ERR_ARG, "pigs_atm_init first");
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    const AtmShape sh = atm_shape(c->P.dim, c->P.Np);
    // one workgroup owns an accumulator element per launch
    return each_launch(c, sw, walkers, true, kWalkerListMax, "launch_atm", [&](int m, const WalkerList &L) {
        return launch_atm(c->P, c->d_paths.p, m, L, sh, c->atm_window, c->atm_rc2, c->d_atm_T.p, c->d_atm_ntrip.p,
                          c->d_atm_samples.p, c->stream);
    });
}

int pigs_atm_read(pigs_ctx *c, double *T, int64_t *ntrip, int64_t *samples, const int32_t *reset)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->atm_ready) return fail(PIGS_ERR_ARG, "pigs_atm_init first");
    if (!T || !ntrip || !samples) return fail(PIGS_ERR_ARG, "null output");
    const size_t per = 2 * (size_t)c->atm_window + 1;
    return read_and_reset(c, {{c->d_atm_T.p, per, T}, {c->d_atm_ntrip.p, per, ntrip}, {c->d_atm_samples.p, 1, samples}}, reset);
}

// ---- momentum distribution n(k) and one-body density matrix of a periodic system -----------------
// Cosine sums per walker and vector and integer counts per walker (pigs_nk.hip) of the end-to-end vectors of open
// worldlines, taken from the sampler's end tape (pigs_nk_accumulate) or from the host (pigs_nk_add); read per block.
int pigs_nk_init(pigs_ctx *c, int32_t nmax, int32_t nbin)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the momentum distribution is defined for periodic systems only (in a trap the one-body density matrix is not translation-invariant)");
    const int nmmax = c->P.dim == 3 ? 16 : 64, nbmax = c->P.dim == 3 ? 128 : c->P.dim == 2 ? 1024 : 4096;
    if (nmax < 1 || nmax > nmmax || nbin < 1 || nbin > nbmax)
        return fail(PIGS_ERR_ARG, "pigs_nk_init: nmax=%d (1..%d in %dD) nbin=%d (1..%d in %dD)", nmax, nmmax, c->P.dim, nbin, nbmax, c->P.dim);
    size_t nv = 1;
    for (int k = 0; k < c->P.dim; ++k) nv *= (size_t)nbin;
    const SqvShape sh = sqv_shape(c->P.dim, nmax);
    const size_t W = (size_t)c->n_walkers;
    const double bytes = (double)W * ((double)nv + (double)sh.Nq + 2.0) * 8.0;
    if (bytes > 2147483648.0)
        return fail(PIGS_ERR_ARG, "pigs_nk_init: %zu walkers x (%zu + %lld + 2) accumulators pass 2 GiB", W, nv, (long long)sh.Nq);
    rc = init_begin(c, c->nk_nmax); if (rc) return rc;
    HIPCHK(alloc_zeroed(c, c->d_nk_C, W * (size_t)sh.Nq));
    HIPCHK(alloc_zeroed(c, c->d_nk_H, W * nv));
    HIPCHK(alloc_zeroed(c, c->d_nk_nopen, W));
    HIPCHK(alloc_zeroed(c, c->d_nk_ninside, W));
    SYNC_CHECKED(c);
    c->nk_nmax = nmax;
    c->nk_nbin = nbin;
    c->nk_nq = sh.Nq;
    c->nk_nvec = nv;
    return PIGS_OK;
}

int pigs_nk_count(pigs_ctx *c, int64_t *Nq)
{
    return c ? grid_count(c, "nk", c->nk_nmax, c->nk_nq, Nq) : fail(PIGS_ERR_ARG, "null context");
}

int pigs_nk_vectors(pigs_ctx *c, int32_t *n)
{
    return c ? grid_vectors(c, "nk", c->nk_nmax, c->nk_nq, n) : fail(PIGS_ERR_ARG, "null context");
}

int pigs_nk_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (!c->nk_nmax) return fail(PIGS_ERR_ARG, "pigs_nk_init first");
    if (!c->sampler_ready || !c->sweep.worm || !c->sweep.tape_count)
        return fail(PIGS_ERR_ARG, "pigs_nk_accumulate: pigs_sampler_init with CWorm > 0 first (there is no open sector to sample)");
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    // one thread owns an element of C per launch
    return each_launch(c, sw, walkers, true, kWalkerListMax, "launch_nk", [&](int m, const WalkerList &L) {
        return launch_nk(c->P, m, L, c->nk_nmax, c->nk_nbin, c->nk_nq, 1, 0, c->sweep.Nobdm, c->sweep.tape_count, c->sweep.tape_x,
                         c->d_nk_C.p, c->d_nk_H.p, c->d_nk_nopen.p, c->d_nk_ninside.p, c->stream);
    });
}

int pigs_nk_add(pigs_ctx *c, int32_t n, const int32_t *walkers, const int32_t *nsamp, const double *xend)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (!c->nk_nmax) return fail(PIGS_ERR_ARG, "pigs_nk_init first");
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    if (n > 0 && !nsamp) return fail(PIGS_ERR_ARG, "null nsamp");
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    int cap = 0;
    size_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (nsamp[i] < 0) return fail(PIGS_ERR_ARG, "nsamp[%d]=%d", i, nsamp[i]);
        cap = std::max(cap, (int)nsamp[i]);
        total += (size_t)nsamp[i];
    }
    if (total && !xend) return fail(PIGS_ERR_ARG, "null xend");
    if (!total) return PIGS_OK;
    // head - tail of every pair, folded once as the sampler's OBDM histogram folds it, at [position][cap][dim]
    const int d = c->P.dim;
    std::vector<double> x((size_t)n * cap * d, 0.0);
    const double *src = xend;
    for (int i = 0; i < n; ++i)
        for (int s = 0; s < nsamp[i]; ++s, src += 2 * d)
            for (int k = 0; k < d; ++k) {
                double v = src[k] - src[d + k];
                if (v >  c->P.LboxHalf[k]) v = v - c->P.Lbox[k];
                if (v < -c->P.LboxHalf[k]) v = v + c->P.Lbox[k];
                x[((size_t)i * cap + s) * d + k] = v;
            }
    // (a grown buffer is a new allocation: freeing the old one waits for the launches that read it)
    HIPCHK(c->d_nk_x.reserve(x.size()));
    HIPCHK(c->d_nk_cnt.reserve((size_t)n));
    HIPCHK(hipMemcpyAsync(c->d_nk_x.p, x.data(), x.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d_nk_cnt.p, nsamp, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                 // x leaves scope: the copies have left the host
    int base = 0;
    return each_launch(c, sw, walkers, true, kWalkerListMax, "launch_nk", [&](int m, const WalkerList &L) {
        const hipError_t e = launch_nk(c->P, m, L, c->nk_nmax, c->nk_nbin, c->nk_nq, 0, base, cap, c->d_nk_cnt.p, c->d_nk_x.p,
                                       c->d_nk_C.p, c->d_nk_H.p, c->d_nk_nopen.p, c->d_nk_ninside.p, c->stream);
        base += m;
        return e;
    });
}

int pigs_nk_read(pigs_ctx *c, double *C, int64_t *H, int64_t *nopen, int64_t *ninside, const int32_t *reset)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->nk_nmax) return fail(PIGS_ERR_ARG, "pigs_nk_init first");
    if (!C || !H || !nopen || !ninside) return fail(PIGS_ERR_ARG, "null output");
    return read_and_reset(c, {{c->d_nk_C.p, (size_t)c->nk_nq, C}, {c->d_nk_H.p, c->nk_nvec, H}, {c->d_nk_nopen.p, 1, nopen},
                              {c->d_nk_ninside.p, 1, ninside}}, reset);
}

// ---- a crystal seen from its lattice: Lindemann moments, site occupancy and site hops over a slice window ------
// Raw sums per walker (pigs_lat.hip), accumulated on the device and read per block.  The first family with an input of its
// own: the sites are uploaded here, once, into rows laid out as a slice's.
int pigs_lat_init(pigs_ctx *c, int32_t nsite, const double *sites, int32_t nbin, double rmax, int32_t window, int32_t cm)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the lattice estimators are defined for periodic systems only (a site is reached by a minimum image)");
    if (c->P.dim < 2) return fail(PIGS_ERR_UNSUPPORTED, "the lattice estimators are defined in 2D and 3D only");
    if (nsite < 1 || !sites || nbin < 1 || !(rmax > 0.0) || !std::isfinite(rmax) || window < 0 || window > c->P.Nb || (cm != 0 && cm != 1))
        return fail(PIGS_ERR_ARG, "pigs_lat_init: nsite=%d nbin=%d rmax=%g window=%d (0..Nb=%d) cm=%d (0 or 1)", nsite, nbin, rmax,
                    window, c->P.Nb, cm);
    const int dim = c->P.dim;
    for (size_t t = 0; t < (size_t)dim * (size_t)nsite; ++t)
        if (!std::isfinite(sites[t])) return fail(PIGS_ERR_ARG, "pigs_lat_init: site %zu has a coordinate that is not finite", t / dim);
    const LatShape sh = lat_shape(dim, c->P.Np, nsite, nbin);
    if (!sh.fits)
        return fail(PIGS_ERR_ARG, "pigs_lat_init: Np=%d particles, %d sites and %d bins in %dD need %zu bytes of LDS (%zu at most)",
                    c->P.Np, nsite, nbin, dim, sh.lds, kLatLdsBudget);
    const size_t W = (size_t)c->n_walkers, ns = 2 * (size_t)window + 1;
    const int NsPad = (nsite + 7) / 8 * 8;
    std::vector<double> rows((size_t)dim * NsPad, 0.0);               // R(dim, nsite) column-major -> dim rows of NsPad
    for (int s = 0; s < nsite; ++s)
        for (int k = 0; k < dim; ++k) rows[(size_t)k * NsPad + s] = sites[(size_t)s * dim + k];
    rc = init_begin(c, c->lat_ready); if (rc) return rc;
    HIPCHK(c->d_lat_sites.alloc(rows.size()));
    HIPCHK(hipMemcpyAsync(c->d_lat_sites.p, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(alloc_zeroed(c, c->d_lat_mom, W * ns * (2 + (size_t)dim)));
    HIPCHK(alloc_zeroed(c, c->d_lat_nass, W * ns));
    HIPCHK(alloc_zeroed(c, c->d_lat_occ, W * ns * 4));
    HIPCHK(alloc_zeroed(c, c->d_lat_hr, W * (size_t)nbin));
    HIPCHK(alloc_zeroed(c, c->d_lat_hx, W * (size_t)dim * 2 * (size_t)nbin));
    HIPCHK(alloc_zeroed(c, c->d_lat_nlost, W));
    HIPCHK(alloc_zeroed(c, c->d_lat_hop1, W));
    HIPCHK(alloc_zeroed(c, c->d_lat_hopw, W));
    HIPCHK(alloc_zeroed(c, c->d_lat_samples, W));
    HIPCHK(alloc_zeroed(c, c->d_lat_sidx, std::min(W, (size_t)kWalkerListMax) * ns * (size_t)c->P.NpPad));
    SYNC_CHECKED(c);                                                  // (rows lives until here)
    c->lat_nsite = nsite; c->lat_nspad = NsPad; c->lat_nbin = nbin; c->lat_window = window; c->lat_cm = cm;
    c->lat_rmax = rmax;
    c->lat_ready = true;
    return PIGS_OK;
}

int pigs_lat_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (!c->lat_ready) return fail(PIGS_ERR_ARG, "pigs_lat_init first");
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    const LatShape sh = lat_shape(c->P.dim, c->P.Np, c->lat_nsite, c->lat_nbin);
    // one workgroup owns an accumulator element per launch; a launch's distinct walkers fit the scratch
    return each_launch(c, sw, walkers, true, kWalkerListMax, "launch_lat", [&](int m, const WalkerList &L) {
        return launch_lat(c->P, c->d_paths.p, m, L, sh, c->lat_window, c->lat_cm, c->lat_nsite, c->lat_nspad, c->d_lat_sites.p,
                          c->lat_nbin, c->lat_rmax, c->d_lat_mom.p, c->d_lat_nass.p, c->d_lat_nlost.p, c->d_lat_occ.p,
                          c->d_lat_hr.p, c->d_lat_hx.p, c->d_lat_hop1.p, c->d_lat_hopw.p, c->d_lat_samples.p, c->d_lat_sidx.p,
                          c->stream);
    });
}

int pigs_lat_read(pigs_ctx *c, double *mom, int64_t *nassigned, int64_t *nlost, int64_t *occ, int64_t *hr, int64_t *hx,
                  int64_t *hop1, int64_t *hopw, int64_t *samples, const int32_t *reset)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->lat_ready) return fail(PIGS_ERR_ARG, "pigs_lat_init first");
    if (!mom || !nassigned || !nlost || !occ || !hr || !hx || !hop1 || !hopw || !samples) return fail(PIGS_ERR_ARG, "null output");
    const size_t ns = 2 * (size_t)c->lat_window + 1, dim = (size_t)c->P.dim, nb = (size_t)c->lat_nbin;
    return read_and_reset(c, {{c->d_lat_mom.p, ns * (2 + dim), mom}, {c->d_lat_nass.p, ns, nassigned}, {c->d_lat_nlost.p, 1, nlost},
                              {c->d_lat_occ.p, ns * 4, occ}, {c->d_lat_hr.p, nb, hr}, {c->d_lat_hx.p, dim * 2 * nb, hx},
                              {c->d_lat_hop1.p, 1, hop1}, {c->d_lat_hopw.p, 1, hopw}, {c->d_lat_samples.p, 1, samples}}, reset);
}

// ---- the superfluid fraction: centre-of-mass diffusion along tau and the unfolded displacement --------------------
// Raw sums per walker, lag and axis (pigs_sf.hip), accumulated on the device and read per block.  The unfolded paths of a
// launch sit in a scratch whose size pigs_sf_init bounds; the launches are cut to the walkers it holds.
int pigs_sf_init(pigs_ctx *c, int32_t Ntau, int32_t window)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the centre-of-mass diffusion is defined for periodic systems only (a link is unfolded through the box)");
    if (window < 0 || window > c->P.Nb || Ntau < 0 || Ntau > 2 * window || Ntau + 1 > kSfLagsMax)
        return fail(PIGS_ERR_ARG, "pigs_sf_init: Ntau=%d (0..2 window, %d lags at most) window=%d (0..Nb=%d)", Ntau, kSfLagsMax,
                    window, c->P.Nb);
    const size_t W = (size_t)c->n_walkers, per = (size_t)(Ntau + 1) * (size_t)c->P.dim, ns = 2 * (size_t)window + 1;
    if ((double)W * (2.0 * (double)per + 2.0) * 8.0 > 2147483648.0)
        return fail(PIGS_ERR_ARG, "pigs_sf_init: %zu walkers x (2 x %d x %d + 2) sums pass 2 GiB", W, Ntau + 1, c->P.dim);
    const size_t slot = sf_slot_doubles(c->P.dim, c->P.NpPad, window);
    const size_t fit = ((size_t)c->sf_scratch_mib << 20) / (slot * sizeof(double));
    const size_t slots = std::max<size_t>(1, std::min({W, (size_t)kWalkerListMax, fit}));
    rc = init_begin(c, c->sf_ready); if (rc) return rc;
    HIPCHK(alloc_zeroed(c, c->d_sf_C, W * per));
    HIPCHK(alloc_zeroed(c, c->d_sf_D, W * per));
    HIPCHK(alloc_zeroed(c, c->d_sf_nwrap, W));
    HIPCHK(alloc_zeroed(c, c->d_sf_samples, W));
    HIPCHK(alloc_zeroed(c, c->d_sf_U, slots * slot));
    HIPCHK(alloc_zeroed(c, c->d_sf_W, slots * ns * (size_t)c->P.dim));
    SYNC_CHECKED(c);
    c->sf_ntau = Ntau; c->sf_window = window; c->sf_slots = (int)slots;
    c->sf_ready = true;
    return PIGS_OK;
}

int pigs_sf_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (!c->sf_ready) return fail(PIGS_ERR_ARG, "pigs_sf_init first");
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    // one thread owns an accumulator element per launch; a launch's walkers fit the scratch
    return each_launch(c, sw, walkers, true, c->sf_slots, "launch_sf", [&](int m, const WalkerList &L) {
        return launch_sf(c->P, c->d_paths.p, m, L, c->sf_window, c->sf_ntau, c->d_sf_U.p, c->d_sf_W.p, c->d_sf_C.p, c->d_sf_D.p,
                         c->d_sf_nwrap.p, c->d_sf_samples.p, c->stream);
    });
}

int pigs_sf_read(pigs_ctx *c, double *C, double *D, int64_t *nwrap, int64_t *samples, const int32_t *reset)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->sf_ready) return fail(PIGS_ERR_ARG, "pigs_sf_init first");
    if (!C || !D || !nwrap || !samples) return fail(PIGS_ERR_ARG, "null output");
    const size_t per = (size_t)(c->sf_ntau + 1) * (size_t)c->P.dim;
    return read_and_reset(c, {{c->d_sf_C.p, per, C}, {c->d_sf_D.p, per, D}, {c->d_sf_nwrap.p, 1, nwrap},
                              {c->d_sf_samples.p, 1, samples}}, reset);
}

// ---- the cluster-size distribution of a periodic system over a slice window -----------------------
// Integer counts and the sums of Rg^2 per walker and size (pigs_cl.hip), accumulated on the device and read per block.  The
// per-slice sums of a launch sit in a scratch whose size pigs_cl_init bounds; the launches are cut to the walkers it holds.
int pigs_cl_np_max(void) { return kClNpMax; }

int pigs_cl_init(pigs_ctx *c, double rc, int32_t window)
{
    int st = check_ctx(c); if (st) return st;
    st = check_cm(c); if (st) return st;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "clusters are defined for periodic systems only (bonds are minimum images)");
    bool rc_ok = std::isfinite(rc) && rc > 0.0;
    for (int k = 0; k < c->P.dim; ++k) rc_ok = rc_ok && rc <= c->P.LboxHalf[k];
    if (!rc_ok || window < 0 || window > c->P.Nb)
        return fail(PIGS_ERR_ARG, "pigs_cl_init: rc=%g (0 < rc <= half the shortest side) window=%d (0..Nb=%d)", rc, window, c->P.Nb);
    if (c->P.Np > kClNpMax || cl_lds_bytes(c->P.dim, c->P.Np) > kClLdsBudget)
        return fail(PIGS_ERR_ARG, "pigs_cl_init: Np=%d passes the %d particles a workgroup labels in LDS", c->P.Np, kClNpMax);
    const size_t W = (size_t)c->n_walkers, np = (size_t)c->P.Np;
    if ((double)W * (3.0 * (double)np + 2.0) * 8.0 > 2147483648.0)
        return fail(PIGS_ERR_ARG, "pigs_cl_init: %zu walkers x (3 x %d + 2) sums pass 2 GiB", W, c->P.Np);
    const size_t slot = cl_slot_doubles(c->P.Np, window);
    const size_t fit = ((size_t)c->cl_scratch_mib << 20) / (slot * sizeof(double));
    const size_t slots = std::max<size_t>(1, std::min({W, (size_t)kWalkerListMax, fit}));
    st = init_begin(c, c->cl_ready); if (st) return st;
    HIPCHK(alloc_zeroed(c, c->d_cl_nsize, W * np));
    HIPCHK(alloc_zeroed(c, c->d_cl_nlarge, W * np));
    HIPCHK(alloc_zeroed(c, c->d_cl_nbond, W));
    HIPCHK(alloc_zeroed(c, c->d_cl_samples, W));
    HIPCHK(alloc_zeroed(c, c->d_cl_rg2, W * np));
    HIPCHK(alloc_zeroed(c, c->d_cl_scratch, slots * slot));
    HIPCHK(alloc_zeroed(c, c->d_cl_sweeps, 1));
    SYNC_CHECKED(c);
    c->cl_window = window; c->cl_slots = (int)slots; c->cl_rc2 = rc * rc;
    c->cl_ready = true;
    return PIGS_OK;
}

int pigs_cl_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int st = check_ctx(c); if (st) return st;
    st = check_cm(c); if (st) return st;
    if (!c->cl_ready) return fail(PIGS_ERR_ARG, "pigs_cl_init first");
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    std::vector<int32_t> sw;
    st = walker_list(c, n, walkers, sw); if (st) return st;
    // one thread owns an element of rg2 per launch; a launch's walkers fit the scratch
    return each_launch(c, sw, walkers, true, c->cl_slots, "launch_cl", [&](int m, const WalkerList &L) {
        return launch_cl(c->P, c->d_paths.p, m, L, c->cl_window, c->cl_rc2, c->d_cl_scratch.p, c->d_cl_nsize.p, c->d_cl_nlarge.p,
                         c->d_cl_nbond.p, c->d_cl_samples.p, c->d_cl_rg2.p, c->d_cl_sweeps.p, c->stream);
    });
}

int pigs_cl_read(pigs_ctx *c, int64_t *nsize, int64_t *nlarge, int64_t *nbond, int64_t *samples, double *rg2, const int32_t *reset)
{
    int st = check_ctx(c); if (st) return st;
    if (!c->cl_ready) return fail(PIGS_ERR_ARG, "pigs_cl_init first");
    if (!nsize || !nlarge || !nbond || !samples || !rg2) return fail(PIGS_ERR_ARG, "null output");
    const size_t np = (size_t)c->P.Np;
    return read_and_reset(c, {{c->d_cl_nsize.p, np, nsize}, {c->d_cl_nlarge.p, np, nlarge}, {c->d_cl_nbond.p, 1, nbond},
                              {c->d_cl_samples.p, 1, samples}, {c->d_cl_rg2.p, np, rg2}}, reset);
}

int pigs_cl_sweeps(pigs_ctx *c, int32_t *max_sweeps)
{
    int st = check_ctx(c); if (st) return st;
    if (!c->cl_ready) return fail(PIGS_ERR_ARG, "pigs_cl_init first");
    if (!max_sweeps) return fail(PIGS_ERR_ARG, "null output");
    unsigned int v = 0u;
    HIPCHK(hipMemcpyAsync(&v, c->d_cl_sweeps.p, sizeof(v), hipMemcpyDeviceToHost, c->stream));
    SYNC_CHECKED(c);
    *max_sweeps = (int32_t)v;
    return PIGS_OK;
}

// ---- wrapping clusters, their unfolded extent and the persistence of clusters along tau -------------
// Integer counts, the finite clusters' sums of Rg^2 and the pair counts per lag (pigs_pc.hip), accumulated on the device and
// read per block.  The per-slice sums and the labels of a launch sit in two scratches whose size pigs_pc_init bounds; the
// launches are cut to the walkers they hold.
int pigs_pc_np_max(void) { return kClNpMax; }

int pigs_pc_init(pigs_ctx *c, double rc, int32_t window, int32_t ntau)
{
    int st = check_ctx(c); if (st) return st;
    st = check_cm(c); if (st) return st;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "wrapping clusters are defined for periodic systems only (bonds are minimum images)");
    bool rc_ok = std::isfinite(rc) && rc > 0.0;
    for (int k = 0; k < c->P.dim; ++k) rc_ok = rc_ok && rc <= c->P.LboxHalf[k];
    if (!rc_ok || window < 0 || window > c->P.Nb || ntau < 0 || ntau > 2 * window)
        return fail(PIGS_ERR_ARG, "pigs_pc_init: rc=%g (0 < rc <= half the shortest side) window=%d (0..Nb=%d) ntau=%d (0..2 window)",
                    rc, window, c->P.Nb, ntau);
    if (c->P.Np > kClNpMax || pc_lds_bytes(c->P.dim, c->P.Np) > kClLdsBudget)
        return fail(PIGS_ERR_ARG, "pigs_pc_init: Np=%d passes the %d particles a workgroup labels in LDS", c->P.Np, kClNpMax);
    const size_t W = (size_t)c->n_walkers, np = (size_t)c->P.Np, nl = (size_t)ntau + 1;
    if ((double)W * (2.0 * (double)np + 25.0 + 4.0 * (double)nl) * 8.0 > 2147483648.0)
        return fail(PIGS_ERR_ARG, "pigs_pc_init: %zu walkers x (2 x %d + 25 + 4 x %zu) sums pass 2 GiB", W, c->P.Np, nl);
    const size_t per = (2 * (size_t)window + 1) * np;
    const size_t fit = ((size_t)c->pc_scratch_mib << 20) / pc_slot_bytes(c->P.Np, window);
    const size_t slots = std::max<size_t>(1, std::min({W, (size_t)kWalkerListMax, fit}));
    st = init_begin(c, c->pc_ready); if (st) return st;
    HIPCHK(alloc_zeroed(c, c->d_pc_nwrap, W * 8));
    HIPCHK(alloc_zeroed(c, c->d_pc_mwrap, W * 8));
    HIPCHK(alloc_zeroed(c, c->d_pc_swrap, W * 8));
    HIPCHK(alloc_zeroed(c, c->d_pc_nfin, W * np));
    HIPCHK(alloc_zeroed(c, c->d_pc_samples, W));
    HIPCHK(alloc_zeroed(c, c->d_pc_first, W * nl));
    HIPCHK(alloc_zeroed(c, c->d_pc_second, W * nl));
    HIPCHK(alloc_zeroed(c, c->d_pc_both, W * nl));
    HIPCHK(alloc_zeroed(c, c->d_pc_norig, W * nl));
    HIPCHK(alloc_zeroed(c, c->d_pc_rg2u, W * np));
    HIPCHK(alloc_zeroed(c, c->d_pc_scratch, slots * per));
    HIPCHK(alloc_zeroed(c, c->d_pc_labels, slots * per));
    HIPCHK(alloc_zeroed(c, c->d_pc_sweeps, 2));
    SYNC_CHECKED(c);
    c->pc_window = window; c->pc_ntau = ntau; c->pc_slots = (int)slots; c->pc_rc2 = rc * rc;
    c->pc_ready = true;
    return PIGS_OK;
}

int pigs_pc_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int st = check_ctx(c); if (st) return st;
    st = check_cm(c); if (st) return st;
    if (!c->pc_ready) return fail(PIGS_ERR_ARG, "pigs_pc_init first");
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    std::vector<int32_t> sw;
    st = walker_list(c, n, walkers, sw); if (st) return st;
    const PcSums sums{c->d_pc_nwrap.p, c->d_pc_mwrap.p, c->d_pc_swrap.p, c->d_pc_nfin.p, c->d_pc_samples.p, c->d_pc_first.p,
                      c->d_pc_second.p, c->d_pc_both.p, c->d_pc_norig.p, c->d_pc_rg2u.p};
    // one thread owns an element of rg2u per launch; a launch's walkers fit the scratches
    return each_launch(c, sw, walkers, true, c->pc_slots, "launch_pc", [&](int m, const WalkerList &L) {
        return launch_pc(c->P, c->d_paths.p, m, L, c->pc_window, c->pc_ntau, c->pc_rc2, c->d_pc_scratch.p, c->d_pc_labels.p, sums,
                         c->d_pc_sweeps.p, c->stream);
    });
}

int pigs_pc_read(pigs_ctx *c, int64_t *nwrap, int64_t *mwrap, int64_t *swrap, int64_t *nfin, int64_t *samples, double *rg2u,
                 int64_t *first, int64_t *second, int64_t *both, int64_t *norig, const int32_t *reset)
{
    int st = check_ctx(c); if (st) return st;
    if (!c->pc_ready) return fail(PIGS_ERR_ARG, "pigs_pc_init first");
    if (!nwrap || !mwrap || !swrap || !nfin || !samples || !rg2u || !first || !second || !both || !norig)
        return fail(PIGS_ERR_ARG, "null output");
    const size_t np = (size_t)c->P.Np, nl = (size_t)c->pc_ntau + 1;
    return read_and_reset(c, {{c->d_pc_nwrap.p, 8, nwrap}, {c->d_pc_mwrap.p, 8, mwrap}, {c->d_pc_swrap.p, 8, swrap},
                              {c->d_pc_nfin.p, np, nfin}, {c->d_pc_samples.p, 1, samples}, {c->d_pc_rg2u.p, np, rg2u},
                              {c->d_pc_first.p, nl, first}, {c->d_pc_second.p, nl, second}, {c->d_pc_both.p, nl, both},
                              {c->d_pc_norig.p, nl, norig}}, reset);
}

int pigs_pc_sweeps(pigs_ctx *c, int32_t *label_sweeps, int32_t *image_sweeps)
{
    int st = check_ctx(c); if (st) return st;
    if (!c->pc_ready) return fail(PIGS_ERR_ARG, "pigs_pc_init first");
    if (!label_sweeps || !image_sweeps) return fail(PIGS_ERR_ARG, "null output");
    unsigned int v[2] = {0u, 0u};
    HIPCHK(hipMemcpyAsync(v, c->d_pc_sweeps.p, sizeof(v), hipMemcpyDeviceToHost, c->stream));
    SYNC_CHECKED(c);
    *label_sweeps = (int32_t)v[0];
    *image_sweeps = (int32_t)v[1];
    return PIGS_OK;
}

// ---- multi-GPU ---------------------------------------------------------------------------
int pigs_comm_unique_id(char id[128])
{
    if (!id) return fail(PIGS_ERR_ARG, "null id");
    const char *err = pigs_comm_get_unique_id(id);
    return err ? fail(PIGS_ERR_COMM, "%s", err) : PIGS_OK;
}

int pigs_comm_init_rank(pigs_ctx *c, int32_t nranks, int32_t rank, const char id[128])
{
    int rc = check_ctx(c); if (rc) return rc;
    if (nranks < 1 || rank < 0 || rank >= nranks || !id) return fail(PIGS_ERR_ARG, "bad rank %d/%d", rank, nranks);
    c->comm.reset();
    const char *err = pigs_comm_create_rank(&c->comm.h, nranks, rank, id);
    return err ? fail(PIGS_ERR_COMM, "%s", err) : PIGS_OK;
}

int pigs_comm_init_all(pigs_ctx **ctxs, int32_t nranks)
{
    if (!ctxs || nranks < 1) return fail(PIGS_ERR_ARG, "bad arguments");
    std::vector<int> devs(nranks);
    std::vector<pigs_comm *> comms(nranks, nullptr);
    bool distinct = true;
    for (int i = 0; i < nranks; ++i) {
        if (!ctxs[i]) return fail(PIGS_ERR_ARG, "null context %d", i);
        devs[i] = ctxs[i]->device;
        for (int k = 0; k < i; ++k) distinct = distinct && devs[k] != devs[i];
    }
    for (int i = 0; i < nranks; ++i) {
        ctxs[i]->comm.reset();
        ctxs[i]->hgroup.reset();
    }
    if (!distinct) {
        // REHEARSAL form (several contexts on one GPU, e.g. a one-GPU test box: RCCL wants one device per rank): the
        // vectors meet in host memory, every rank adds the ranks' vectors in rank order (deterministic).  Not a
        // multi-GPU path: the product form is the RCCL communicator below.
        auto g = std::make_shared<HostGroup>();
        g->n = nranks;
        g->slot.resize(nranks);
        // (several contexts share one chip here: one workgroup per walker in pigs_cm.hip -- cooperating workgroups assume
        // that the walkers of ONE context have the chip to themselves -- except for TWO shards: their TranslateChain kernels
        // are chained device-wide (g_cm_gate) and take the CUs the other shard's sweep kernel leaves, H x own walkers +
        // the other's walkers <= CUs.  The shards then run staggered -- 38.5 instead of 39.9 ms per MC step of 2 x 64
        // walkers at N=256, scripts/k6_stagger.py.  More than two shards would share the process's four hardware queues.)
        for (int i = 0; i < nranks; ++i) {
            ctxs[i]->hgroup = g; ctxs[i]->hrank = i; ctxs[i]->cm_split = 1;
            if (nranks == 2 && ctxs[i]->n_walkers > 0) {
                int H = (ctxs[i]->n_cu - ctxs[1 - i]->n_walkers) / ctxs[i]->n_walkers;
                H = H > 4 ? 4 : H;
                if (H >= 2) { ctxs[i]->cm_split = H; ctxs[i]->cm_shared = true; }
            }
        }
        return PIGS_OK;
    }
    const char *err = pigs_comm_create_all(comms.data(), nranks, devs.data());
    if (err) return fail(PIGS_ERR_COMM, "%s", err);
    for (int i = 0; i < nranks; ++i) ctxs[i]->comm.h = comms[i];
    return PIGS_OK;
}

int pigs_estimators_allreduce(pigs_ctx *c, double *vec, int32_t n)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (n < 0 || (n && !vec)) return fail(PIGS_ERR_ARG, "bad vector");
    if (n == 0) return PIGS_OK;
    if (c->hgroup) {
        HostGroup &g = *c->hgroup;
        std::unique_lock<std::mutex> lk(g.m);
        g.slot[c->hrank].assign(vec, vec + n);
        const int gen = g.generation;
        if (++g.arrived == g.n) {
            g.sum.assign(n, 0.0);
            for (int r = 0; r < g.n; ++r) {
                if ((int)g.slot[r].size() != n) { g.arrived = 0; ++g.generation; g.cv.notify_all(); return fail(PIGS_ERR_ARG, "ranks disagree on the vector length"); }
                for (int k = 0; k < n; ++k) g.sum[k] += g.slot[r][k];
            }
            g.arrived = 0;
            ++g.generation;
            g.cv.notify_all();
        } else {
            g.cv.wait(lk, [&] { return g.generation != gen; });
        }
        if ((int)g.sum.size() != n) return fail(PIGS_ERR_ARG, "ranks disagree on the vector length");
        memcpy(vec, g.sum.data(), (size_t)n * sizeof(double));
        return PIGS_OK;
    }
    if (!c->comm) return fail(PIGS_ERR_COMM, "no communicator: call pigs_comm_init_rank / pigs_comm_init_all first");
    HIPCHK(c->est.res.reserve(n));
    hipStream_t s = c->stream;
    HIPCHK(hipMemcpyAsync(c->est.res.p, vec, n * sizeof(double), hipMemcpyHostToDevice, s));
    const char *err = pigs_comm_allreduce_sum_f64(c->comm, c->est.res.p, n, s);
    if (err) return fail(PIGS_ERR_COMM, "%s", err);
    HIPCHK(hipMemcpyAsync(vec, c->est.res.p, n * sizeof(double), hipMemcpyDeviceToHost, s));
    SYNC_CHECKED(c);
    return PIGS_OK;
}

} // extern "C"
