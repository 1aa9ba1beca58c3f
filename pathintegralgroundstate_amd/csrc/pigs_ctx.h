// pigs_ctx.h -- the context behind the C ABI and what its translation units share (host side, internal to the library):
// pigs_capi.hip holds the context, K1..K7, the sampler and the communicator, pigs_capi_families.hip the per-walker
// accumulator families.  Every resource is owned by the member that holds it.
#pragma once

#include "../../include/pigs_hip.h"

#include <hip/hip_runtime.h>

#include <condition_variable>
#include <cstring>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "pigs_comm.h"
#include "pigs_kernels.h"

struct pigs_ctx;

namespace pigs {

#define PIGS_INTERNAL __attribute__((visibility("hidden")))

// sets pigs_last_error of the calling thread and returns `code` (defined in pigs_capi.hip)
PIGS_INTERNAL int fail(int code, const char *fmt, ...);

#define HIPCHK(expr)                                                                     \
    do {                                                                                 \
        hipError_t e_ = (expr);                                                          \
        if (e_ != hipSuccess)                                                            \
            return ::pigs::fail(PIGS_ERR_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                __FILE__, __LINE__);                                     \
    } while (0)

// the context is usable on this thread (its device made current)
PIGS_INTERNAL int check_ctx(pigs_ctx *c);
// after a synchronisation: did a cooperating workgroup of the TranslateChain kernel give up waiting (pigs_cm.hip)?
PIGS_INTERNAL int check_cm(pigs_ctx *c);
// every entry point that waits for the stream and then hands state of the walkers to the caller (worldlines, counters,
// events, generator, estimators) ends here: after a time-out in pigs_cm.hip none of it may be returned as if it were valid
PIGS_INTERNAL int sync_checked(pigs_ctx *c);
#define SYNC_CHECKED(c)                          \
    do {                                         \
        const int rc_ = ::pigs::sync_checked(c); \
        if (rc_) return rc_;                     \
    } while (0)
// the walkers of a request -- walkers[i], or 0..n-1 when the list is left out -- range-checked
PIGS_INTERNAL int walker_list(const pigs_ctx *c, int n, const int32_t *walkers, std::vector<int32_t> &sw);

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

// several contexts of one process meeting in host memory (pigs_comm_init_all on duplicate devices: rehearsal only)
struct HostGroup {
    int n = 0, arrived = 0, generation = 0;
    std::mutex m;
    std::condition_variable cv;
    std::vector<std::vector<double>> slot;
    std::vector<double> sum;
};

// ---- the per-walker accumulator families (pigs_capi_families.hip) -----------------------------------------------------
// One accumulator array of a family: 8-byte elements, walker-major, `per` of them per walker.  *_init sizes it, once
// (alloc), and *_read takes the size from here (read_and_reset); per == 0 is an array that is switched off.
template <typename T>
struct Acc {
    static_assert(sizeof(T) == 8, "read_and_reset copies and zeroes accumulators as 8-byte elements");
    DevBuf<T> buf;
    size_t per = 0;
    // n_walkers x max(per, 1) elements, their zeroing queued on the context's stream
    hipError_t alloc(pigs_ctx *c, size_t per_walker);
    operator T *() const { return buf.p; }
};
using AccD = Acc<double>;
using AccN = Acc<unsigned long long>;

// A family's state: its accumulators, the scratch of one launch, `ready` (its *_init stood; until then its other entry
// points refuse), the parameters of that *_init, and its tuning value where it has one (which outlives a second *_init).

// density profiles of a trapped system (pigs_density_*): per-walker counts, planar [Nbin^min(dim,2)], radial and pair [Nbin]
struct DensityState {
    AccN planar, radial, pair, samples;
    bool ready = false;
    int nbin = 0;
    double h = 0.0, b = 0.0, br = 0.0;
};
// imaginary-time density correlations of a periodic system (pigs_fqt_*): raw sums [walker][l][iq][k], the samples per
// walker, and the C/S scratch of one launch's window slices ([slots][2 window + 1][Nk dim][2])
struct FqtState {
    AccD acc;
    AccN samples;
    DevBuf<double> rho;
    bool ready = false;
    int nk = 0, ntau = 0, window = 0, slots = 0;
};
// imaginary-time profiles (pigs_tau_*): raw sums [walker][2Nb+1][4] and the samples per walker
struct TauState {
    AccD acc;
    AccN samples;
    bool ready = false;
};
// vector structure factor on the full reciprocal grid (pigs_sqv_*): raw sums [walker][iqv], the samples per walker,
// and the C^2 + S^2 scratch of one launch's window slices ([slots][2 window + 1][Nq])
struct SqvState {
    AccD acc;
    AccN samples;
    DevBuf<double> rho2;
    bool ready = false;
    int nmax = 0, window = 0, slots = 0;
    int64_t nq = 0;
};
// F(q,tau) on the vectors of pigs_sqv_* (pigs_fqv_*): raw sums [walker][l][iqv], the samples per walker, and the
// (C, S) scratch of one launch's window slices ([slots][2 window + 1][Nq][2])
struct FqvState {
    AccD acc;
    AccN samples;
    DevBuf<double> rho;
    bool ready = false;
    int nmax = 0, ntau = 0, window = 0, slots = 0;
    int64_t nq = 0;
};
// self part of F(q,tau) and the imaginary-time displacement (pigs_fqs_*): raw sums F [walker][l][iqv] and
// D [walker][l][2], the samples per walker; no scratch (pigs_fqs.hip keeps the phasors in LDS)
struct FqsState {
    AccD acc, dsp;
    AccN samples;
    bool ready = false;
    int nmax = 0, ntau = 0, window = 0;
    int64_t nq = 0;
};
// pair distribution on the vector grid over a slice window (pigs_grv_*): per-walker counts, vec [Nbin^dim] and radial [Nr]
struct GrvState {
    AccN vec, radial, samples;
    bool ready = false;
    int nbin = 0, nr = 0, window = 0;
    int form = -1;                      // tuning key "grv_form": -1 automatic, 0 global atomics, 1 grid privatised in LDS
    double rbin = 0.0;
};
// bond-orientational order over a slice window (pigs_bop_*): raw sums S [walker][8] and G [walker][Nr], the counts
// H [walker][2][Nh] and GN [walker][Nr], the samples per walker, and the scratch of one launch's window slices
// ([slots][2 window + 1][8 + Nr])
struct BopState {
    AccD S, G;
    AccN H, GN, samples;
    DevBuf<double> scratch;
    bool ready = false;
    int nh = 0, nr = 0, window = 0, slots = 0;
    double rnb2 = 0.0, rbin = 0.0;
};
// van Hove functions over a slice window (pigs_vh_*): per-walker counts, self [walker][Ntau+1][Ns] and dist
// [walker][Ntau+1][Nr], and the samples per walker
struct VhState {
    AccN self, dist, samples;
    bool ready = false;
    int nr = 0, ns = 0, ntau = 0, window = 0;
    int form = -1;                      // tuning key "vh_form": -1 automatic, 0 global atomics, 1 histograms privatised in LDS
    double rbin = 0.0, sbin = 0.0;
};
// triplet distribution over a slice window (pigs_g3_*): per-walker counts, trip [walker][Nr (Nr + 1) / 2][Na] and
// pair [walker][Nr], and the samples per walker
struct G3State {
    AccN trip, pair, samples;
    bool ready = false;
    int nr = 0, na = 0, window = 0;
    int form = -1;                      // tuning key "g3_form": -1 automatic, 0 global atomics, 1 counters privatised in LDS
    double rbin = 0.0;
};
// Axilrod-Teller-Muto geometric sum over a slice window (pigs_atm_*): raw sums T [walker][2 window + 1], the triplets
// counted ntrip [walker][2 window + 1], and the samples per walker
struct AtmState {
    AccD T;
    AccN ntrip, samples;
    bool ready = false;
    int window = 0;
    double rc2 = 0.0;
};
// momentum distribution and one-body density matrix (pigs_nk_*): cosine sums C [walker][Nq], counts H [walker][nbin^dim],
// nopen and ninside [walker]; the samples that pigs_nk_add brings from the host ([position][cap][dim] and their numbers)
struct NkState {
    AccD C;
    AccN H, nopen, ninside;
    DevBuf<double> x;
    DevBuf<int32_t> cnt;
    bool ready = false;
    int nmax = 0, nbin = 0;
    int64_t nq = 0;
};
// a crystal seen from its lattice (pigs_lat_*): the site rows [dim][NsPad], per walker the moments
// mom [2 window + 1][2 + dim], nassigned [2 window + 1], occ [2 window + 1][4], hr [nbin], hx [dim][2 nbin], nlost, hop1,
// hopw and samples; the assigned sites of one launch, sidx [min(n_walkers, 256)][2 window + 1][NpPad]
struct LatState {
    AccD mom;
    AccN nass, nlost, occ, hr, hx, hop1, hopw, samples;
    DevBuf<double> sites;
    DevBuf<int32_t> sidx;
    bool ready = false;
    int nsite = 0, nspad = 0, nbin = 0, window = 0, cm = 0;
    double rmax = 0.0;
};
// centre-of-mass diffusion along tau (pigs_sf_*): per walker C and D [Ntau + 1][dim], nwrap and samples; the unfolded
// coordinates of one launch, U [slots][2 window + 1][dim][NpPad], and its centre of mass Wcm [slots][2 window + 1][dim]
struct SfState {
    AccD C, D;
    AccN nwrap, samples;
    DevBuf<double> U, W;
    bool ready = false;
    int ntau = 0, window = 0;
    int slots = 0;                      // walkers per launch: what the scratch holds
    int scratch_mib = kSfScratchMiB;    // pigs_set_tuning "sf_scratch_mib": the budget of U at the next pigs_sf_init
};
// cluster-size distribution over a slice window (pigs_cl_*): per walker nsize, nlarge and rg2 [Np], nbond and samples;
// the per-slice sums of g per size of one launch ([slots][2 window + 1][Np]); the largest sweep count so far
struct ClState {
    AccN nsize, nlarge, nbond, samples;
    AccD rg2;
    DevBuf<double> scratch;
    DevBuf<unsigned int> sweeps;
    bool ready = false;
    int window = 0;
    int slots = 0;                      // walkers per launch: what the scratch holds
    double rc2 = 0.0;
    int scratch_mib = kClScratchMiB;    // pigs_set_tuning "cl_scratch_mib": the budget of the scratch at the next pigs_cl_init
};
// wrapping clusters and cluster persistence over a slice window (pigs_pc_*): per walker nwrap, mwrap, swrap [8], nfin and
// rg2u [Np], samples, and first, second, both, norig [ntau + 1]; the per-slice sums of g and the labels of one launch
// ([slots][2 window + 1][Np] each); the largest labelling and image sweep counts so far
struct PcState {
    AccN nwrap, mwrap, swrap, nfin, samples, first, second, both, norig;
    AccD rg2u;
    DevBuf<double> scratch;
    DevBuf<int> labels;
    DevBuf<unsigned int> sweeps;
    bool ready = false;
    int window = 0, ntau = 0;
    int slots = 0;                      // walkers per launch: what the two scratches hold
    double rc2 = 0.0;
    int scratch_mib = kPcScratchMiB;    // pigs_set_tuning "pc_scratch_mib": the budget of the scratches at the next pigs_pc_init
};

} // namespace pigs

struct pigs_ctx {
    pigs_params hp;
    pigs::DevParams P;
    int         device    = 0;
    int         n_walkers = 0;
    pigs::Stream stream;
    pigs::DevBuf<double> d_paths, d_VT, d_WF;
    std::shared_ptr<pigs::HostGroup> hgroup;   // rehearsal form of the estimator reduction (several contexts on one GPU)
    int hrank = 0;
    pigs::DevBuf<double> d_VTimg;        // [0, VT(0)] VT(0..Nmax+1) [0 0 0 0]: PipeTab image for the sampler (pigs_k1_device.h)
    size_t  path_doubles = 0;        // resident doubles per walker (padded SoA)
    size_t  raw_doubles  = 0;        // dim*Np*(2Nb+1): reference layout per walker
    pigs::DevBuf<int32_t> d_walker, d_ip, d_ib;
    pigs::DevBuf<double>  d_xnew, d_xold, d_out, d_parts, d_stage;
    pigs::EstBufs est;                       // estimators on the context's stream (also the scratch of K2/K3, K4, K7 alone)
    pigs::Comm  comm;
    int         k1_variant = pigs::K1_AUTO;
    pigs::PinBuf st_w, st_ip, st_ib, st_xn, st_xo, st_out;     // staged items
    pigs::PinBuf cs_w, cs_ip, cs_ib, cs_x;                     // staged commits
    int64_t     st_cap = 0, cs_cap = 0;
    // device-resident sampler
    pigs::DevBuf<uint32_t> d_rng;
    pigs::DevBuf<unsigned long long> d_counters;
    pigs::DevBuf<double> d_worm, d_nrho, d_dklog;
    pigs::DevBuf<int> d_evlog;
    size_t      nrho_doubles = 0;
    pigs::SweepParams sweep{};
    int         cm_freq = 1;
    int         sweep_threads = 512;
    bool        sweep_split = false;    // diagonal moves of periodic 'bis' systems in pigs_diag.hip's kernel (see pigs_sampler_step)
    int         n_cu = 256;
    // TranslateChain by several workgroups per walker (pigs_cm.hip): -1 as many as fit (default), 0 off, H >= 1 at most H
    int         cm_split = -1;
    bool        cm_exclusive = false;       // the caller vouches that no other context's kernels run on this device meanwhile
    bool        cm_shared = false;          // several contexts of this process sample on this device at once: see g_cm_gate
    pigs::DevBuf<unsigned long long> d_xch; // exchange buffer of the cooperating workgroups
    pigs::PinBuf h_cm_err;                  // (one int) set by a workgroup whose partner never answered
    unsigned int cm_seq = 1;                // sequence tags of the exchange: advanced by every launch
    int         form_cm = -1;               // H of the last step's TranslateChain (0: inside the sweep kernel): pigs_sampler_form
    bool        form_diag = false;          // the last step ran the stage-machine kernel
    bool        sampler_ready = false;
    // asynchronous estimators (pigs_diagonal_estimators_begin / _end): a snapshot of the worldlines and a second stream
    pigs::Stream stream2;
    pigs::Event ev_snap;
    pigs::DevBuf<double> d_shadow;
    pigs::EstBufs a_buf;
    pigs::PinBuf a_host;                    // results land here (pinned: the copy is truly asynchronous)
    std::vector<int32_t> a_sw, a_sb;        // slot lists: must outlive the asynchronous upload
    struct { bool on = false, launched = false; pigs::EstBatch b; } a_pend;
    pigs::Event ev_gate;                    // recorded behind the TranslateChain kernel of the next step (see launch_pending_estimators)
    // the sampler's end tape (periodic context, CWorm > 0): per walker the samples of the last step and their once-folded
    // end-to-end vectors [walker][Nobdm][dim] (SweepParams.tape_count, tape_x)
    pigs::DevBuf<int32_t> d_tape_count;
    pigs::DevBuf<double>  d_tape_x;
    // the launches of the accumulator families (each_launch): which walkers the current one holds
    pigs::WalkerMarks list_marks;
    pigs::DensityState density;
    pigs::FqtState fqt;
    pigs::TauState tau;
    pigs::SqvState sqv;
    pigs::FqvState fqv;
    pigs::FqsState fqs;
    pigs::GrvState grv;
    pigs::BopState bop;
    pigs::VhState  vh;
    pigs::G3State  g3;
    pigs::AtmState atm;
    pigs::NkState  nk;
    pigs::LatState lat;
    pigs::SfState  sf;
    pigs::ClState  cl;
    pigs::PcState  pc;
};

namespace pigs {

// exactly n elements, and their zeroing queued on the context's stream
template <typename T>
inline hipError_t alloc_zeroed(pigs_ctx *c, DevBuf<T> &b, size_t n)
{
    const hipError_t e = b.alloc(n);
    return e == hipSuccess ? hipMemsetAsync(b.p, 0, n * sizeof(T), c->stream) : e;
}

template <typename T>
inline hipError_t Acc<T>::alloc(pigs_ctx *c, size_t per_walker)
{
    per = per_walker;
    return alloc_zeroed(c, buf, (size_t)c->n_walkers * (per_walker ? per_walker : 1));
}

} // namespace pigs
