// pigs_capi_families.hip -- the per-walker accumulator families of include/pigs_hip.h: density, fqt, tau, sqv, fqv, fqs,
// grv, bop, vh, g3, atm, nk, lat, sf, cl and pc.  Each has its state in the context (pigs_ctx.h) and three entry points
// on one path: *_init validates, sizes every accumulator once (Acc::alloc) and allocates; *_accumulate queues launches
// (each_launch); *_read copies the accumulators out and zeroes the flagged walkers (read_and_reset).
#include <cfloat>
#include <cmath>
#include <algorithm>
#include <initializer_list>

#include "pigs_ctx.h"
#include "pigs_family_sizes.h"
#include "pigs_launch.h"

using namespace pigs;

// ---- what the families share ---------------------------------------------------------------------

// *_init, once the request is accepted: no accumulate may be in flight on the buffers being replaced, and until the new
// ones stand the family counts as uninitialised
template <typename State>
static int init_begin(pigs_ctx *c, State &st)
{
    HIPCHK(hipStreamSynchronize(c->stream));
    st.ready = false;
    return PIGS_OK;
}

// *_read, *_count, *_vectors and *_sweeps begin here: the context, then "pigs_<fam>_init first".  (The family goes as a
// member pointer: a null context is check_ctx's to refuse.)
template <typename State>
static int read_begin(pigs_ctx *c, State pigs_ctx::*st, const char *fam, bool cm = false)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (cm) { rc = check_cm(c); if (rc) return rc; }
    if (!(c->*st).ready) return fail(PIGS_ERR_ARG, "pigs_%s_init first", fam);
    return PIGS_OK;
}

// *_accumulate begins here: the context, a time-out of pigs_cm.hip, "pigs_<fam>_init first" ...
template <typename State>
static int acc_begin(pigs_ctx *c, State pigs_ctx::*st, const char *fam) { return read_begin(c, st, fam, true); }

// ... the count and the checked walkers (in two calls where a family has a refusal of its own in between)
static int acc_walkers(const pigs_ctx *c, int n, const int32_t *walkers, std::vector<int32_t> &sw)
{
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    return walker_list(c, n, walkers, sw);
}

template <typename State>
static int acc_begin(pigs_ctx *c, State pigs_ctx::*st, const char *fam, int n, const int32_t *walkers, std::vector<int32_t> &sw)
{
    const int rc = acc_begin(c, st, fam);
    return rc ? rc : acc_walkers(c, n, walkers, sw);
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

// *_read: one accumulator array and where its copy goes
struct AccOut {
    void *dev; size_t per; void *host;
    AccOut(const AccD &a, double *h) : dev(a.buf.p), per(a.per), host(h) {}
    AccOut(const AccN &a, int64_t *h) : dev(a.buf.p), per(a.per), host(h) {}
};

// copy every array to the host, then zero the flagged walkers (one memset per array and run of consecutive walkers), wait
static int read_and_reset(pigs_ctx *c, std::initializer_list<AccOut> arrays, const int32_t *reset)
{
    const size_t W = (size_t)c->n_walkers, u = 8;
    hipStream_t s = c->stream;
    for (const AccOut &a : arrays)
        if (a.per) HIPCHK(hipMemcpyAsync(a.host, a.dev, W * a.per * u, hipMemcpyDeviceToHost, s));
    for (size_t w = 0; reset && w < W;) {
        if (!reset[w]) { ++w; continue; }
        size_t e = w;
        while (e < W && reset[e]) ++e;
        for (const AccOut &a : arrays)
            if (a.per) HIPCHK(hipMemsetAsync((char *)a.dev + w * a.per * u, 0, (e - w) * a.per * u, s));
        w = e;
    }
    SYNC_CHECKED(c);
    return PIGS_OK;
}

// pigs_{sqv,fqv,fqs,nk}_count and _vectors: the family's nmax and Nq
template <typename State>
static int grid_count(pigs_ctx *c, State pigs_ctx::*st, const char *fam, int64_t *Nq)
{
    int rc = read_begin(c, st, fam); if (rc) return rc;
    if (!Nq) return fail(PIGS_ERR_ARG, "null output");
    *Nq = (c->*st).nq;
    return PIGS_OK;
}

// vector iqv has rank iqv + Nq + 1 among all (2 nmax + 1)^dim vectors, n_1 slowest (include/pigs_hip.h)
template <typename State>
static int grid_vectors(pigs_ctx *c, State pigs_ctx::*st, const char *fam, int32_t *n)
{
    int rc = read_begin(c, st, fam); if (rc) return rc;
    if (!n) return fail(PIGS_ERR_ARG, "null output");
    const int dim = c->P.dim, nmax = (c->*st).nmax, S = 2 * nmax + 1;
    const int64_t nq = (c->*st).nq;
    for (int64_t iqv = 0; iqv < nq; ++iqv) {
        int64_t r = iqv + nq + 1;
        for (int k = dim - 1; k >= 0; --k) {
            n[iqv * dim + k] = (int32_t)(r % S) - nmax;
            r /= S;
        }
    }
    return PIGS_OK;
}

// the sweep counters of pigs_cl_* and pigs_pc_*
static int read_sweeps(pigs_ctx *c, const DevBuf<unsigned int> &d, unsigned int *v, size_t n)
{
    HIPCHK(hipMemcpyAsync(v, d.p, n * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    SYNC_CHECKED(c);
    return PIGS_OK;
}

constexpr size_t kMiB = (size_t)1 << 20;

extern "C" {

// ---- density profiles of a trapped system ------------------------------------------------------
// Three per-walker histograms of slice Nb (pigs_density.hip) accumulated on the device and read per block.  The widths
// are computed here, once, in double: b = (2h)/Nbin for the planar grid over [-h, h), br = h/Nbin for r and d in [0, h).
// (Alone among the families, its entry points do not test for a time-out of pigs_cm.hip: hence read_begin throughout.)
int pigs_density_init(pigs_ctx *c, int32_t Nbin, double half_width)
{
    int rc = check_ctx(c); if (rc) return rc;
    if (!c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "density profiles are defined for trapped systems only");
    if (Nbin < 1 || !(half_width > 0.0)) return fail(PIGS_ERR_ARG, "pigs_density_init: Nbin=%d half_width=%g", Nbin, half_width);
    const int dp = c->P.dim < 2 ? c->P.dim : 2;
    size_t np = 1;
    for (int k = 0; k < dp; ++k) np *= (size_t)Nbin;
    DensityState &d = c->density;
    rc = init_begin(c, d); if (rc) return rc;
    HIPCHK(d.planar.alloc(c, np));
    HIPCHK(d.radial.alloc(c, Nbin));
    HIPCHK(d.pair.alloc(c, Nbin));
    HIPCHK(d.samples.alloc(c, 1));
    SYNC_CHECKED(c);
    d.nbin = Nbin;
    d.h = half_width;
    d.b = (2.0 * half_width) / Nbin;
    d.br = half_width / Nbin;
    d.ready = true;
    return PIGS_OK;
}

int pigs_density_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = read_begin(c, &pigs_ctx::density, "density"); if (rc) return rc;
    std::vector<int32_t> sw;
    rc = acc_walkers(c, n, walkers, sw); if (rc) return rc;
    const DensityState &d = c->density;
    // integer atomics: a walker may appear twice in one launch
    return each_launch(c, sw, walkers, false, kWalkerListMax, "launch_density", [&](int m, const WalkerList &L) {
        return launch_density(c->P, c->d_paths.p, m, L, d.nbin, d.h, d.b, d.br, d.planar, d.radial, d.pair, d.samples, c->stream);
    });
}

int pigs_density_read(pigs_ctx *c, int64_t *planar, int64_t *radial, int64_t *pair, int64_t *samples, const int32_t *reset)
{
    int rc = read_begin(c, &pigs_ctx::density, "density"); if (rc) return rc;
    if (!planar || !radial || !pair || !samples) return fail(PIGS_ERR_ARG, "null output");
    const DensityState &d = c->density;
    return read_and_reset(c, {{d.planar, planar}, {d.radial, radial}, {d.pair, pair}, {d.samples, samples}}, reset);
}

// ---- imaginary-time density correlations F(q,tau) of a periodic system ---------------------------
// Raw sums per walker, lag, harmonic and axis (pigs_fqt.hip), accumulated on the device and read per block.
int pigs_fqt_init(pigs_ctx *c, int32_t Nk, int32_t Ntau, int32_t window)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "F(q,tau) is defined for periodic systems only (the q grid is the box's)");
    if (Nk < 1 || !window_ok(window, c->P.Nb) || !lags_ok(Ntau, window))
        return fail(PIGS_ERR_ARG, "pigs_fqt_init: Nk=%d Ntau=%d window=%d (Nb=%d)", Nk, Ntau, window, c->P.Nb);
    const int slots = std::min(c->n_walkers, kWalkerListMax);
    FqtState &f = c->fqt;
    rc = init_begin(c, f); if (rc) return rc;
    HIPCHK(f.acc.alloc(c, (size_t)(Ntau + 1) * Nk * c->P.dim));
    HIPCHK(f.samples.alloc(c, 1));
    HIPCHK(f.rho.alloc((size_t)slots * (2 * window + 1) * 2 * Nk * c->P.dim));
    SYNC_CHECKED(c);
    f.nk = Nk;
    f.ntau = Ntau;
    f.window = window;
    f.slots = slots;
    f.ready = true;
    return PIGS_OK;
}

int pigs_fqt_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    std::vector<int32_t> sw;
    int rc = acc_begin(c, &pigs_ctx::fqt, "fqt", n, walkers, sw); if (rc) return rc;
    const FqtState &f = c->fqt;
    // one thread owns an accumulator element per launch, and the scratch holds f.slots walkers
    return each_launch(c, sw, walkers, true, f.slots, "launch_fqt", [&](int m, const WalkerList &L) {
        return launch_fqt(c->P, c->d_paths.p, m, L, f.window, f.ntau, f.nk, f.rho.p, f.acc, f.samples, c->stream);
    });
}

int pigs_fqt_read(pigs_ctx *c, double *F, int64_t *samples, const int32_t *reset)
{
    int rc = read_begin(c, &pigs_ctx::fqt, "fqt"); if (rc) return rc;
    if (!F || !samples) return fail(PIGS_ERR_ARG, "null output");
    return read_and_reset(c, {{c->fqt.acc, F}, {c->fqt.samples, samples}}, reset);
}

// ---- imaginary-time profiles: V(tau), the virial and the link lengths of every slice --------------
// Raw sums per walker, slice and quantity (pigs_tau.hip), accumulated on the device and read per block.
int pigs_tau_init(pigs_ctx *c)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    TauState &t = c->tau;
    rc = init_begin(c, t); if (rc) return rc;
    HIPCHK(t.acc.alloc(c, (size_t)c->P.M * 4));
    HIPCHK(t.samples.alloc(c, 1));
    SYNC_CHECKED(c);
    t.ready = true;
    return PIGS_OK;
}

int pigs_tau_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    std::vector<int32_t> sw;
    int rc = acc_begin(c, &pigs_ctx::tau, "tau", n, walkers, sw); if (rc) return rc;
    // one workgroup owns an accumulator element per launch
    return each_launch(c, sw, walkers, true, kWalkerListMax, "launch_tau", [&](int m, const WalkerList &L) {
        return launch_tau(c->P, c->d_paths.p, c->d_VT.p, m, L, c->tau.acc, c->tau.samples, c->stream);
    });
}

int pigs_tau_read(pigs_ctx *c, double *Q, int64_t *samples, const int32_t *reset)
{
    int rc = read_begin(c, &pigs_ctx::tau, "tau"); if (rc) return rc;
    if (!Q || !samples) return fail(PIGS_ERR_ARG, "null output");
    return read_and_reset(c, {{c->tau.acc, Q}, {c->tau.samples, samples}}, reset);
}

// ---- vector structure factor S(q) on the full reciprocal grid of a periodic system ----------------
// Raw sums per walker and vector (pigs_sqv.hip), accumulated on the device and read per block.
constexpr size_t kSqvScratchMax = 256 * kMiB;             // bytes of slice scratch behind one launch

int pigs_sqv_init(pigs_ctx *c, int32_t nmax, int32_t window)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the vector S(q) is defined for periodic systems only (the q grid is the box's)");
    if (nmax < 1 || nmax > (c->P.dim == 3 ? 16 : 64) || !window_ok(window, c->P.Nb))
        return fail(PIGS_ERR_ARG, "pigs_sqv_init: nmax=%d (1..%d in %dD) window=%d (0..Nb=%d)", nmax, c->P.dim == 3 ? 16 : 64,
                    c->P.dim, window, c->P.Nb);
    const SqvShape sh = sqv_shape(c->P.dim, nmax);
    const size_t slice = (size_t)(2 * window + 1) * (size_t)sh.Nq;
    const int slots = scratch_slots(c->n_walkers, kWalkerListMax, kSqvScratchMax, slice * sizeof(double));
    SqvState &q = c->sqv;
    rc = init_begin(c, q); if (rc) return rc;
    HIPCHK(q.acc.alloc(c, (size_t)sh.Nq));
    HIPCHK(q.samples.alloc(c, 1));
    HIPCHK(q.rho2.alloc((size_t)slots * slice));
    SYNC_CHECKED(c);
    q.nmax = nmax;
    q.window = window;
    q.slots = slots;
    q.nq = sh.Nq;
    q.ready = true;
    return PIGS_OK;
}

int pigs_sqv_count(pigs_ctx *c, int64_t *Nq) { return grid_count(c, &pigs_ctx::sqv, "sqv", Nq); }
int pigs_sqv_vectors(pigs_ctx *c, int32_t *n) { return grid_vectors(c, &pigs_ctx::sqv, "sqv", n); }

int pigs_sqv_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    std::vector<int32_t> sw;
    int rc = acc_begin(c, &pigs_ctx::sqv, "sqv", n, walkers, sw); if (rc) return rc;
    const SqvState &q = c->sqv;
    // one thread owns an accumulator element per launch, and the scratch holds q.slots walkers
    return each_launch(c, sw, walkers, true, q.slots, "launch_sqv", [&](int m, const WalkerList &L) {
        return launch_sqv(c->P, c->d_paths.p, m, L, q.window, q.nmax, q.rho2.p, q.acc, q.samples, c->stream);
    });
}

int pigs_sqv_read(pigs_ctx *c, double *S, int64_t *samples, const int32_t *reset)
{
    int rc = read_begin(c, &pigs_ctx::sqv, "sqv"); if (rc) return rc;
    if (!S || !samples) return fail(PIGS_ERR_ARG, "null output");
    return read_and_reset(c, {{c->sqv.acc, S}, {c->sqv.samples, samples}}, reset);
}

// ---- F(q,tau) on the full reciprocal grid of a periodic system -----------------------------------
// Raw sums per walker, lag and vector (pigs_fqv.hip): the vectors of pigs_sqv_*, the window and lags of pigs_fqt_*.
int pigs_fqv_init(pigs_ctx *c, int32_t nmax, int32_t Ntau, int32_t window)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the vector F(q,tau) is defined for periodic systems only (the q grid is the box's)");
    if (nmax < 1 || nmax > (c->P.dim == 3 ? 16 : 64) || !window_ok(window, c->P.Nb) || !lags_ok(Ntau, window))
        return fail(PIGS_ERR_ARG, "pigs_fqv_init: nmax=%d (1..%d in %dD) Ntau=%d (0..2 window) window=%d (0..Nb=%d)", nmax,
                    c->P.dim == 3 ? 16 : 64, c->P.dim, Ntau, window, c->P.Nb);
    if (!fqv_width(2 * window + 1))
        return fail(PIGS_ERR_ARG, "pigs_fqv_init: %d window slices of one vector pass the %zu bytes of LDS staging", 2 * window + 1,
                    kFqvLdsBudget);
    const SqvShape sh = sqv_shape(c->P.dim, nmax);
    const size_t W = (size_t)c->n_walkers, per = (size_t)(Ntau + 1) * (size_t)sh.Nq;
    const size_t slice = (size_t)(2 * window + 1) * 2 * (size_t)sh.Nq;
    if (acc_bytes_pass_2gib(W, per + 1))
        return fail(PIGS_ERR_ARG, "pigs_fqv_init: %zu walkers x (%d x %lld + 1) sums pass 2 GiB", W, Ntau + 1, (long long)sh.Nq);
    // the scratch cap is that of pigs_sqv_*
    const int slots = scratch_slots(W, kWalkerListMax, kSqvScratchMax, slice * sizeof(double));
    FqvState &f = c->fqv;
    rc = init_begin(c, f); if (rc) return rc;
    HIPCHK(f.acc.alloc(c, per));
    HIPCHK(f.samples.alloc(c, 1));
    HIPCHK(f.rho.alloc((size_t)slots * slice));
    SYNC_CHECKED(c);
    f.nmax = nmax;
    f.ntau = Ntau;
    f.window = window;
    f.slots = slots;
    f.nq = sh.Nq;
    f.ready = true;
    return PIGS_OK;
}

int pigs_fqv_count(pigs_ctx *c, int64_t *Nq) { return grid_count(c, &pigs_ctx::fqv, "fqv", Nq); }
int pigs_fqv_vectors(pigs_ctx *c, int32_t *n) { return grid_vectors(c, &pigs_ctx::fqv, "fqv", n); }

int pigs_fqv_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    std::vector<int32_t> sw;
    int rc = acc_begin(c, &pigs_ctx::fqv, "fqv", n, walkers, sw); if (rc) return rc;
    const FqvState &f = c->fqv;
    // one thread owns an accumulator element per launch, and the scratch holds f.slots walkers
    return each_launch(c, sw, walkers, true, f.slots, "launch_fqv", [&](int m, const WalkerList &L) {
        return launch_fqv(c->P, c->d_paths.p, m, L, f.window, f.ntau, f.nmax, f.rho.p, f.acc, f.samples, c->stream);
    });
}

int pigs_fqv_read(pigs_ctx *c, double *F, int64_t *samples, const int32_t *reset)
{
    int rc = read_begin(c, &pigs_ctx::fqv, "fqv"); if (rc) return rc;
    if (!F || !samples) return fail(PIGS_ERR_ARG, "null output");
    return read_and_reset(c, {{c->fqv.acc, F}, {c->fqv.samples, samples}}, reset);
}

// ---- self part of F(q,tau) and the imaginary-time displacement of a periodic system ---------------
// Raw sums per walker, lag and vector, and per walker and lag (pigs_fqs.hip): the vectors, window and lags of pigs_fqv_*.
int pigs_fqs_init(pigs_ctx *c, int32_t nmax, int32_t Ntau, int32_t window)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the self part of F(q,tau) is defined for periodic systems only (the q grid is the box's)");
    if (nmax < 1 || nmax > (c->P.dim == 3 ? 16 : 64) || !window_ok(window, c->P.Nb) || !lags_ok(Ntau, window))
        return fail(PIGS_ERR_ARG, "pigs_fqs_init: nmax=%d (1..%d in %dD) Ntau=%d (0..2 window) window=%d (0..Nb=%d)", nmax,
                    c->P.dim == 3 ? 16 : 64, c->P.dim, Ntau, window, c->P.Nb);
    if (!fqs_shape(c->P.dim, nmax, window, Ntau).width)
        return fail(PIGS_ERR_ARG, "pigs_fqs_init: the phasors of %d window slices (nmax=%d, %dD) pass the %zu bytes of LDS, or %d lags"
                    " the %d a workgroup takes", 2 * window + 1, nmax, c->P.dim, kFqsLdsBudget, Ntau + 1, kFqsThreads * kFqsLags);
    const SqvShape sh = sqv_shape(c->P.dim, nmax);
    const size_t W = (size_t)c->n_walkers, per = (size_t)(Ntau + 1) * (size_t)sh.Nq, perd = (size_t)(Ntau + 1) * 2;
    if (acc_bytes_pass_2gib(W, per + perd + 1))
        return fail(PIGS_ERR_ARG, "pigs_fqs_init: %zu walkers x (%d x (%lld + 2) + 1) sums pass 2 GiB", W, Ntau + 1, (long long)sh.Nq);
    FqsState &f = c->fqs;
    rc = init_begin(c, f); if (rc) return rc;
    HIPCHK(f.acc.alloc(c, per));
    HIPCHK(f.dsp.alloc(c, perd));
    HIPCHK(f.samples.alloc(c, 1));
    SYNC_CHECKED(c);
    f.nmax = nmax;
    f.ntau = Ntau;
    f.window = window;
    f.nq = sh.Nq;
    f.ready = true;
    return PIGS_OK;
}

int pigs_fqs_count(pigs_ctx *c, int64_t *Nq) { return grid_count(c, &pigs_ctx::fqs, "fqs", Nq); }
int pigs_fqs_vectors(pigs_ctx *c, int32_t *n) { return grid_vectors(c, &pigs_ctx::fqs, "fqs", n); }

int pigs_fqs_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    std::vector<int32_t> sw;
    int rc = acc_begin(c, &pigs_ctx::fqs, "fqs", n, walkers, sw); if (rc) return rc;
    const FqsState &f = c->fqs;
    // one thread owns an accumulator element per launch
    return each_launch(c, sw, walkers, true, kWalkerListMax, "launch_fqs", [&](int m, const WalkerList &L) {
        return launch_fqs(c->P, c->d_paths.p, m, L, f.window, f.ntau, f.nmax, f.acc, f.dsp, f.samples, c->stream);
    });
}

int pigs_fqs_read(pigs_ctx *c, double *F, double *D, int64_t *samples, const int32_t *reset)
{
    int rc = read_begin(c, &pigs_ctx::fqs, "fqs"); if (rc) return rc;
    if (!F || !D || !samples) return fail(PIGS_ERR_ARG, "null output");
    return read_and_reset(c, {{c->fqs.acc, F}, {c->fqs.dsp, D}, {c->fqs.samples, samples}}, reset);
}

// ---- pair distribution of a periodic system on the vector grid, over a slice window ---------------
// Integer counts per walker (pigs_grv.hip), accumulated on the device and read per block.
int pigs_grv_init(pigs_ctx *c, int32_t Nbin, int32_t Nr, double rbin, int32_t window)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the vector g(r) is defined for periodic systems only (its grid is the box's)");
    const int nbmax = c->P.dim == 3 ? 128 : c->P.dim == 2 ? 1024 : 4096;
    if (Nbin < 1 || Nbin > nbmax || Nr < 1 || !(rbin > 0.0) || !std::isfinite(rbin) || !window_ok(window, c->P.Nb))
        return fail(PIGS_ERR_ARG, "pigs_grv_init: Nbin=%d (1..%d in %dD) Nr=%d rbin=%g window=%d (0..Nb=%d)", Nbin, nbmax,
                    c->P.dim, Nr, rbin, window, c->P.Nb);
    size_t nv = 1;
    for (int k = 0; k < c->P.dim; ++k) nv *= (size_t)Nbin;
    const size_t W = (size_t)c->n_walkers;
    if (acc_bytes_pass_2gib(W, nv + (size_t)Nr + 1))
        return fail(PIGS_ERR_ARG, "pigs_grv_init: %zu walkers x (%zu + %d + 1) counters pass 2 GiB", W, nv, Nr);
    GrvState &g = c->grv;
    rc = init_begin(c, g); if (rc) return rc;
    HIPCHK(g.vec.alloc(c, nv));
    HIPCHK(g.radial.alloc(c, Nr));
    HIPCHK(g.samples.alloc(c, 1));
    SYNC_CHECKED(c);
    g.nbin = Nbin;
    g.nr = Nr;
    g.window = window;
    g.rbin = rbin;
    g.ready = true;
    return PIGS_OK;
}

int pigs_grv_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    std::vector<int32_t> sw;
    int rc = acc_begin(c, &pigs_ctx::grv, "grv", n, walkers, sw); if (rc) return rc;
    const GrvState &g = c->grv;
    // integer atomics: a walker may appear twice in one launch.  The form follows from the launch's size; a forced LDS
    // form that does not fit is refused at that launch, the launches before it stay queued.
    bool fits = true;
    rc = each_launch(c, sw, walkers, false, kWalkerListMax, "launch_grv", [&](int m, const WalkerList &L) {
        const GrvShape sh = grv_shape(c->P.dim, c->P.Np, g.nbin, g.nr, g.window, g.form, m, c->n_cu);
        fits = !(sh.vec_lds && !sh.vec_fits);
        if (!fits) return hipErrorInvalidValue;
        return launch_grv(c->P, c->d_paths.p, m, L, sh, g.window, g.nbin, g.nr, g.rbin, g.vec, g.radial, g.samples, c->stream);
    });
    if (!fits) return fail(PIGS_ERR_ARG, "pigs_grv_accumulate: grv_form = 1, but a grid of %zu bins does not fit the LDS", g.vec.per);
    return rc;
}

int pigs_grv_read(pigs_ctx *c, int64_t *vec, int64_t *radial, int64_t *samples, const int32_t *reset)
{
    int rc = read_begin(c, &pigs_ctx::grv, "grv"); if (rc) return rc;
    if (!vec || !radial || !samples) return fail(PIGS_ERR_ARG, "null output");
    return read_and_reset(c, {{c->grv.vec, vec}, {c->grv.radial, radial}, {c->grv.samples, samples}}, reset);
}

// ---- bond-orientational order of a periodic system over a slice window ---------------------------
// Raw sums and integer counts per walker (pigs_bop.hip), accumulated on the device and read per block.
int pigs_bop_init(pigs_ctx *c, double rnb, int32_t window, int32_t Nh, int32_t Nr, double rbin)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "bond-orientational order is defined for periodic systems only (bonds are minimum images)");
    if (c->P.dim < 2) return fail(PIGS_ERR_UNSUPPORTED, "bond-orientational order is defined in 2D and 3D only");
    if (!cutoff_in_box(c->P.dim, c->P.LboxHalf, rnb, 0.0) || !window_ok(window, c->P.Nb) || Nh < 1 || Nh > kBopHistMax || Nr < 0 ||
        (Nr > 0 && (!(rbin > 0.0) || !std::isfinite(rbin))))
        return fail(PIGS_ERR_ARG, "pigs_bop_init: rnb=%g (0 < rnb <= half the shortest side) window=%d (0..Nb=%d) Nh=%d (1..%d) Nr=%d rbin=%g",
                    rnb, window, c->P.Nb, Nh, kBopHistMax, Nr, rbin);
    if (Nr > 0 && c->P.Np > kBopNpMax)
        return fail(PIGS_ERR_ARG, "pigs_bop_init: Np=%d passes %d, where a fixed-point bin of G6(r) could overflow", c->P.Np, kBopNpMax);
    const size_t lds = bop_lds_bytes(c->P.dim, c->P.Np, Nr);
    if (lds > kBopLdsBudget)
        return fail(PIGS_ERR_ARG, "pigs_bop_init: Np=%d Nr=%d need %zu bytes of LDS for one slice (%zu at most)", c->P.Np, Nr, lds,
                    kBopLdsBudget);
    const int slots = std::min(c->n_walkers, kWalkerListMax);
    BopState &b = c->bop;
    rc = init_begin(c, b); if (rc) return rc;
    HIPCHK(b.S.alloc(c, 8));
    HIPCHK(b.H.alloc(c, (size_t)2 * Nh));
    HIPCHK(b.G.alloc(c, Nr));                        // Nr = 0: G6(r) is switched off
    HIPCHK(b.GN.alloc(c, Nr));
    HIPCHK(b.samples.alloc(c, 1));
    HIPCHK(b.scratch.alloc((size_t)slots * (2 * window + 1) * ((size_t)8 + Nr)));
    SYNC_CHECKED(c);
    b.nh = Nh;
    b.nr = Nr;
    b.window = window;
    b.slots = slots;
    b.rnb2 = rnb * rnb;
    b.rbin = Nr > 0 ? rbin : 1.0;
    b.ready = true;
    return PIGS_OK;
}

int pigs_bop_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    std::vector<int32_t> sw;
    int rc = acc_begin(c, &pigs_ctx::bop, "bop", n, walkers, sw); if (rc) return rc;
    const BopState &b = c->bop;
    // one thread owns an accumulator element per launch, and the scratch holds b.slots walkers
    return each_launch(c, sw, walkers, true, b.slots, "launch_bop", [&](int m, const WalkerList &L) {
        return launch_bop(c->P, c->d_paths.p, m, L, b.window, b.nh, b.nr, b.rnb2, b.rbin, b.scratch.p, b.S, b.H, b.G, b.GN,
                          b.samples, c->stream);
    });
}

int pigs_bop_read(pigs_ctx *c, double *S, int64_t *H, double *G, int64_t *GN, int64_t *samples, const int32_t *reset)
{
    int rc = read_begin(c, &pigs_ctx::bop, "bop"); if (rc) return rc;
    const BopState &b = c->bop;
    if (!S || !H || !samples || (b.nr > 0 && (!G || !GN))) return fail(PIGS_ERR_ARG, "null output");
    return read_and_reset(c, {{b.S, S}, {b.H, H}, {b.G, G}, {b.GN, GN}, {b.samples, samples}}, reset);
}

// ---- van Hove functions G_s(r,tau), G_d(r,tau) of a periodic system over a slice window -----------
// Integer counts per walker and lag (pigs_vh.hip), accumulated on the device and read per block.
int pigs_vh_init(pigs_ctx *c, int32_t Ntau, int32_t window, int32_t Nr, double rbin, int32_t Ns, double sbin)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the van Hove functions are defined for periodic systems only (their displacements are minimum images)");
    if (Nr < 1 || Ns < 1 || !(rbin > 0.0) || !std::isfinite(rbin) || !(sbin > 0.0) || !std::isfinite(sbin) ||
        !window_ok(window, c->P.Nb) || !lags_ok(Ntau, window))
        return fail(PIGS_ERR_ARG, "pigs_vh_init: Ntau=%d (0..2 window) window=%d (0..Nb=%d) Nr=%d rbin=%g Ns=%d sbin=%g", Ntau, window,
                    c->P.Nb, Nr, rbin, Ns, sbin);
    const size_t W = (size_t)c->n_walkers, nl = (size_t)Ntau + 1;
    if (acc_bytes_pass_2gib(W, nl * ((size_t)Nr + (size_t)Ns) + 1))
        return fail(PIGS_ERR_ARG, "pigs_vh_init: %zu walkers x (%zu x (%d + %d) + 1) counters pass 2 GiB", W, nl, Nr, Ns);
    if (!vh_shape(c->P.dim, c->P.Np, Ntau, Nr, Ns, 0).slice_fits)
        return fail(PIGS_ERR_ARG, "pigs_vh_init: a slice of Np=%d particles in %dD needs %zu bytes of LDS (%zu at most)", c->P.Np,
                    c->P.dim, sizeof(double) * (size_t)c->P.dim * (size_t)c->P.Np, kVhLdsBudget);
    VhState &v = c->vh;
    rc = init_begin(c, v); if (rc) return rc;
    HIPCHK(v.self.alloc(c, nl * Ns));
    HIPCHK(v.dist.alloc(c, nl * Nr));
    HIPCHK(v.samples.alloc(c, 1));
    SYNC_CHECKED(c);
    v.nr = Nr;
    v.ns = Ns;
    v.ntau = Ntau;
    v.window = window;
    v.rbin = rbin;
    v.sbin = sbin;
    v.ready = true;
    return PIGS_OK;
}

int pigs_vh_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = acc_begin(c, &pigs_ctx::vh, "vh"); if (rc) return rc;
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    const VhState &v = c->vh;
    // a forced LDS form that does not fit is refused before anything is queued
    const VhShape sh = vh_shape(c->P.dim, c->P.Np, v.ntau, v.nr, v.ns, v.form);
    if (sh.hist_lds && !sh.hist_fits)
        return fail(PIGS_ERR_ARG, "pigs_vh_accumulate: vh_form = 1, but %d x (%d + %d) counters do not fit the LDS beside the slice",
                    v.ntau + 1, v.nr, v.ns);
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    // integer atomics: a walker may appear twice in one launch
    return each_launch(c, sw, walkers, false, kWalkerListMax, "launch_vh", [&](int m, const WalkerList &L) {
        return launch_vh(c->P, c->d_paths.p, m, L, sh, v.window, v.ntau, v.nr, v.rbin, v.ns, v.sbin, v.self, v.dist, v.samples,
                         c->stream);
    });
}

int pigs_vh_read(pigs_ctx *c, int64_t *self, int64_t *dist, int64_t *samples, const int32_t *reset)
{
    int rc = read_begin(c, &pigs_ctx::vh, "vh"); if (rc) return rc;
    if (!self || !dist || !samples) return fail(PIGS_ERR_ARG, "null output");
    return read_and_reset(c, {{c->vh.self, self}, {c->vh.dist, dist}, {c->vh.samples, samples}}, reset);
}

// ---- triplet distribution g3(r, s, cos theta) of a periodic system over a slice window ------------
// Integer counts per walker (pigs_g3.hip), accumulated on the device and read per block.
int pigs_g3_init(pigs_ctx *c, int32_t Nr, double rbin, int32_t Na, int32_t window)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the triplet distribution is defined for periodic systems only (its legs are minimum images)");
    if (c->P.dim < 2) return fail(PIGS_ERR_UNSUPPORTED, "the triplet distribution is defined in 2D and 3D only");
    if (Nr < 1 || Nr > kG3GridMax || Na < 1 || Na > kG3GridMax || !(rbin > 0.0) || !std::isfinite(rbin) || !window_ok(window, c->P.Nb))
        return fail(PIGS_ERR_ARG, "pigs_g3_init: Nr=%d Na=%d (1..%d) rbin=%g window=%d (0..Nb=%d)", Nr, Na, kG3GridMax, rbin, window,
                    c->P.Nb);
    // rbin = (half a side) / Nr is the natural call, and Nr rbin may then round a few ulps past the half side
    const double rmax = (double)Nr * rbin;
    if (!cutoff_in_box(c->P.dim, c->P.LboxHalf, rmax, 4.0 * DBL_EPSILON))
        return fail(PIGS_ERR_ARG, "pigs_g3_init: rmax = Nr rbin = %g (0 < rmax <= half the shortest side)", rmax);
    const size_t W = (size_t)c->n_walkers, ntrip = (size_t)Nr * ((size_t)Nr + 1) / 2 * (size_t)Na;
    if (acc_bytes_pass_2gib(W, ntrip + (size_t)Nr + 1))
        return fail(PIGS_ERR_ARG, "pigs_g3_init: %zu walkers x (%zu + %d + 1) counters pass 2 GiB", W, ntrip, Nr);
    const G3Shape sh = g3_shape(c->P.dim, c->P.Np, Nr, Na, 0);
    if (!sh.fits)
        return fail(PIGS_ERR_ARG, "pigs_g3_init: a slice of Np=%d particles in %dD and its leg lists need %zu bytes of LDS (%zu at most)",
                    c->P.Np, c->P.dim, sh.lds, kG3LdsBudget);
    G3State &g = c->g3;
    rc = init_begin(c, g); if (rc) return rc;
    HIPCHK(g.trip.alloc(c, ntrip));
    HIPCHK(g.pair.alloc(c, Nr));
    HIPCHK(g.samples.alloc(c, 1));
    SYNC_CHECKED(c);
    g.nr = Nr;
    g.na = Na;
    g.window = window;
    g.rbin = rbin;
    g.ready = true;
    return PIGS_OK;
}

int pigs_g3_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = acc_begin(c, &pigs_ctx::g3, "g3"); if (rc) return rc;
    if (n < 0) return fail(PIGS_ERR_ARG, "n=%d", n);
    const G3State &g = c->g3;
    // a forced LDS form that does not fit is refused before anything is queued
    const G3Shape sh = g3_shape(c->P.dim, c->P.Np, g.nr, g.na, g.form);
    if (sh.hist_lds && !sh.hist_fits)
        return fail(PIGS_ERR_ARG, "pigs_g3_accumulate: g3_form = 1, but %d x %d x %d / 2 counters do not fit the LDS beside the slice and the leg lists",
                    g.nr, g.nr + 1, g.na);
    std::vector<int32_t> sw;
    rc = walker_list(c, n, walkers, sw); if (rc) return rc;
    // integer atomics: a walker may appear twice in one launch
    return each_launch(c, sw, walkers, false, kWalkerListMax, "launch_g3", [&](int m, const WalkerList &L) {
        return launch_g3(c->P, c->d_paths.p, m, L, sh, g.window, g.nr, g.rbin, g.na, g.trip, g.pair, g.samples, c->stream);
    });
}

int pigs_g3_read(pigs_ctx *c, int64_t *trip, int64_t *pair, int64_t *samples, const int32_t *reset)
{
    int rc = read_begin(c, &pigs_ctx::g3, "g3"); if (rc) return rc;
    if (!trip || !pair || !samples) return fail(PIGS_ERR_ARG, "null output");
    return read_and_reset(c, {{c->g3.trip, trip}, {c->g3.pair, pair}, {c->g3.samples, samples}}, reset);
}

// ---- Axilrod-Teller-Muto three-body geometric sum of a periodic system over a slice window -------
// Raw sums per walker and window slice (pigs_atm.hip), accumulated on the device and read per block.
int pigs_atm_init(pigs_ctx *c, double rc, int32_t window)
{
    int rc_ = check_ctx(c); if (rc_) return rc_;
    rc_ = check_cm(c); if (rc_) return rc_;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the three-body energy is defined for periodic systems only (its sides are minimum images)");
    if (c->P.dim < 2) return fail(PIGS_ERR_UNSUPPORTED, "the three-body energy is defined in 2D and 3D only");
    if (!(rc > 0.0) || !std::isfinite(rc) || !window_ok(window, c->P.Nb))
        return fail(PIGS_ERR_ARG, "pigs_atm_init: rc=%g window=%d (0..Nb=%d)", rc, window, c->P.Nb);
    if (!cutoff_in_box(c->P.dim, c->P.LboxHalf, rc, 0.0))
        return fail(PIGS_ERR_ARG, "pigs_atm_init: rc = %g (0 < rc <= half the shortest side)", rc);
    const AtmShape sh = atm_shape(c->P.dim, c->P.Np);
    if (!sh.fits)
        return fail(PIGS_ERR_ARG, "pigs_atm_init: a slice of Np=%d particles in %dD and its leg lists need %zu bytes of LDS (%zu at most)",
                    c->P.Np, c->P.dim, sh.lds, kAtmLdsBudget);
    const size_t per = 2 * (size_t)window + 1;
    AtmState &a = c->atm;
    rc_ = init_begin(c, a); if (rc_) return rc_;
    HIPCHK(a.T.alloc(c, per));
    HIPCHK(a.ntrip.alloc(c, per));
    HIPCHK(a.samples.alloc(c, 1));
    SYNC_CHECKED(c);
    a.window = window;
    a.rc2 = rc * rc;
    a.ready = true;
    return PIGS_OK;
}

int pigs_atm_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    std::vector<int32_t> sw;
    int rc = acc_begin(c, &pigs_ctx::atm, "atm", n, walkers, sw); if (rc) return rc;
    const AtmState &a = c->atm;
    const AtmShape sh = atm_shape(c->P.dim, c->P.Np);
    // one workgroup owns an accumulator element per launch
    return each_launch(c, sw, walkers, true, kWalkerListMax, "launch_atm", [&](int m, const WalkerList &L) {
        return launch_atm(c->P, c->d_paths.p, m, L, sh, a.window, a.rc2, a.T, a.ntrip, a.samples, c->stream);
    });
}

int pigs_atm_read(pigs_ctx *c, double *T, int64_t *ntrip, int64_t *samples, const int32_t *reset)
{
    int rc = read_begin(c, &pigs_ctx::atm, "atm"); if (rc) return rc;
    if (!T || !ntrip || !samples) return fail(PIGS_ERR_ARG, "null output");
    return read_and_reset(c, {{c->atm.T, T}, {c->atm.ntrip, ntrip}, {c->atm.samples, samples}}, reset);
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
    if (acc_bytes_pass_2gib(W, nv + (size_t)sh.Nq + 2))
        return fail(PIGS_ERR_ARG, "pigs_nk_init: %zu walkers x (%zu + %lld + 2) accumulators pass 2 GiB", W, nv, (long long)sh.Nq);
    NkState &k = c->nk;
    rc = init_begin(c, k); if (rc) return rc;
    HIPCHK(k.C.alloc(c, (size_t)sh.Nq));
    HIPCHK(k.H.alloc(c, nv));
    HIPCHK(k.nopen.alloc(c, 1));
    HIPCHK(k.ninside.alloc(c, 1));
    SYNC_CHECKED(c);
    k.nmax = nmax;
    k.nbin = nbin;
    k.nq = sh.Nq;
    k.ready = true;
    return PIGS_OK;
}

int pigs_nk_count(pigs_ctx *c, int64_t *Nq) { return grid_count(c, &pigs_ctx::nk, "nk", Nq); }
int pigs_nk_vectors(pigs_ctx *c, int32_t *n) { return grid_vectors(c, &pigs_ctx::nk, "nk", n); }

int pigs_nk_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    int rc = acc_begin(c, &pigs_ctx::nk, "nk"); if (rc) return rc;
    if (!c->sampler_ready || !c->sweep.worm || !c->sweep.tape_count)
        return fail(PIGS_ERR_ARG, "pigs_nk_accumulate: pigs_sampler_init with CWorm > 0 first (there is no open sector to sample)");
    std::vector<int32_t> sw;
    rc = acc_walkers(c, n, walkers, sw); if (rc) return rc;
    const NkState &k = c->nk;
    // one thread owns an element of C per launch
    return each_launch(c, sw, walkers, true, kWalkerListMax, "launch_nk", [&](int m, const WalkerList &L) {
        return launch_nk(c->P, m, L, k.nmax, k.nbin, k.nq, 1, 0, c->sweep.Nobdm, c->sweep.tape_count, c->sweep.tape_x, k.C, k.H,
                         k.nopen, k.ninside, c->stream);
    });
}

int pigs_nk_add(pigs_ctx *c, int32_t n, const int32_t *walkers, const int32_t *nsamp, const double *xend)
{
    int rc = acc_begin(c, &pigs_ctx::nk, "nk"); if (rc) return rc;
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
    NkState &k = c->nk;
    // (a grown buffer is a new allocation: freeing the old one waits for the launches that read it)
    HIPCHK(k.x.reserve(x.size()));
    HIPCHK(k.cnt.reserve((size_t)n));
    HIPCHK(hipMemcpyAsync(k.x.p, x.data(), x.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(k.cnt.p, nsamp, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                 // x leaves scope: the copies have left the host
    int base = 0;
    return each_launch(c, sw, walkers, true, kWalkerListMax, "launch_nk", [&](int m, const WalkerList &L) {
        const hipError_t e = launch_nk(c->P, m, L, k.nmax, k.nbin, k.nq, 0, base, cap, k.cnt.p, k.x.p, k.C, k.H, k.nopen, k.ninside,
                                       c->stream);
        base += m;
        return e;
    });
}

int pigs_nk_read(pigs_ctx *c, double *C, int64_t *H, int64_t *nopen, int64_t *ninside, const int32_t *reset)
{
    int rc = read_begin(c, &pigs_ctx::nk, "nk"); if (rc) return rc;
    if (!C || !H || !nopen || !ninside) return fail(PIGS_ERR_ARG, "null output");
    const NkState &k = c->nk;
    return read_and_reset(c, {{k.C, C}, {k.H, H}, {k.nopen, nopen}, {k.ninside, ninside}}, reset);
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
    if (nsite < 1 || !sites || nbin < 1 || !(rmax > 0.0) || !std::isfinite(rmax) || !window_ok(window, c->P.Nb) || (cm != 0 && cm != 1))
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
    LatState &l = c->lat;
    rc = init_begin(c, l); if (rc) return rc;
    HIPCHK(l.sites.alloc(rows.size()));
    HIPCHK(hipMemcpyAsync(l.sites.p, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(l.mom.alloc(c, ns * (2 + (size_t)dim)));
    HIPCHK(l.nass.alloc(c, ns));
    HIPCHK(l.occ.alloc(c, ns * 4));
    HIPCHK(l.hr.alloc(c, (size_t)nbin));
    HIPCHK(l.hx.alloc(c, (size_t)dim * 2 * (size_t)nbin));
    HIPCHK(l.nlost.alloc(c, 1));
    HIPCHK(l.hop1.alloc(c, 1));
    HIPCHK(l.hopw.alloc(c, 1));
    HIPCHK(l.samples.alloc(c, 1));
    HIPCHK(alloc_zeroed(c, l.sidx, std::min(W, (size_t)kWalkerListMax) * ns * (size_t)c->P.NpPad));
    SYNC_CHECKED(c);                                                  // (rows lives until here)
    l.nsite = nsite; l.nspad = NsPad; l.nbin = nbin; l.window = window; l.cm = cm;
    l.rmax = rmax;
    l.ready = true;
    return PIGS_OK;
}

int pigs_lat_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    std::vector<int32_t> sw;
    int rc = acc_begin(c, &pigs_ctx::lat, "lat", n, walkers, sw); if (rc) return rc;
    const LatState &l = c->lat;
    const LatShape sh = lat_shape(c->P.dim, c->P.Np, l.nsite, l.nbin);
    // one workgroup owns an accumulator element per launch; a launch's distinct walkers fit the scratch
    return each_launch(c, sw, walkers, true, kWalkerListMax, "launch_lat", [&](int m, const WalkerList &L) {
        return launch_lat(c->P, c->d_paths.p, m, L, sh, l.window, l.cm, l.nsite, l.nspad, l.sites.p, l.nbin, l.rmax, l.mom, l.nass,
                          l.nlost, l.occ, l.hr, l.hx, l.hop1, l.hopw, l.samples, l.sidx.p, c->stream);
    });
}

int pigs_lat_read(pigs_ctx *c, double *mom, int64_t *nassigned, int64_t *nlost, int64_t *occ, int64_t *hr, int64_t *hx,
                  int64_t *hop1, int64_t *hopw, int64_t *samples, const int32_t *reset)
{
    int rc = read_begin(c, &pigs_ctx::lat, "lat"); if (rc) return rc;
    if (!mom || !nassigned || !nlost || !occ || !hr || !hx || !hop1 || !hopw || !samples) return fail(PIGS_ERR_ARG, "null output");
    const LatState &l = c->lat;
    return read_and_reset(c, {{l.mom, mom}, {l.nass, nassigned}, {l.nlost, nlost}, {l.occ, occ}, {l.hr, hr}, {l.hx, hx},
                              {l.hop1, hop1}, {l.hopw, hopw}, {l.samples, samples}}, reset);
}

// ---- the superfluid fraction: centre-of-mass diffusion along tau and the unfolded displacement --------------------
// Raw sums per walker, lag and axis (pigs_sf.hip), accumulated on the device and read per block.  The unfolded paths of a
// launch sit in a scratch whose size pigs_sf_init bounds; the launches are cut to the walkers it holds.
int pigs_sf_init(pigs_ctx *c, int32_t Ntau, int32_t window)
{
    int rc = check_ctx(c); if (rc) return rc;
    rc = check_cm(c); if (rc) return rc;
    if (c->P.trap) return fail(PIGS_ERR_UNSUPPORTED, "the centre-of-mass diffusion is defined for periodic systems only (a link is unfolded through the box)");
    if (!window_ok(window, c->P.Nb) || !lags_ok(Ntau, window) || Ntau + 1 > kSfLagsMax)
        return fail(PIGS_ERR_ARG, "pigs_sf_init: Ntau=%d (0..2 window, %d lags at most) window=%d (0..Nb=%d)", Ntau, kSfLagsMax,
                    window, c->P.Nb);
    const size_t W = (size_t)c->n_walkers, per = (size_t)(Ntau + 1) * (size_t)c->P.dim, ns = 2 * (size_t)window + 1;
    if (acc_bytes_pass_2gib(W, 2 * per + 2))
        return fail(PIGS_ERR_ARG, "pigs_sf_init: %zu walkers x (2 x %d x %d + 2) sums pass 2 GiB", W, Ntau + 1, c->P.dim);
    SfState &f = c->sf;
    const size_t slot = sf_slot_doubles(c->P.dim, c->P.NpPad, window);
    const size_t slots = scratch_slots(W, kWalkerListMax, (size_t)f.scratch_mib * kMiB, slot * sizeof(double));
    rc = init_begin(c, f); if (rc) return rc;
    HIPCHK(f.C.alloc(c, per));
    HIPCHK(f.D.alloc(c, per));
    HIPCHK(f.nwrap.alloc(c, 1));
    HIPCHK(f.samples.alloc(c, 1));
    HIPCHK(alloc_zeroed(c, f.U, slots * slot));
    HIPCHK(alloc_zeroed(c, f.W, slots * ns * (size_t)c->P.dim));
    SYNC_CHECKED(c);
    f.ntau = Ntau; f.window = window; f.slots = (int)slots;
    f.ready = true;
    return PIGS_OK;
}

int pigs_sf_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    std::vector<int32_t> sw;
    int rc = acc_begin(c, &pigs_ctx::sf, "sf", n, walkers, sw); if (rc) return rc;
    const SfState &f = c->sf;
    // one thread owns an accumulator element per launch; a launch's walkers fit the scratch
    return each_launch(c, sw, walkers, true, f.slots, "launch_sf", [&](int m, const WalkerList &L) {
        return launch_sf(c->P, c->d_paths.p, m, L, f.window, f.ntau, f.U.p, f.W.p, f.C, f.D, f.nwrap, f.samples, c->stream);
    });
}

int pigs_sf_read(pigs_ctx *c, double *C, double *D, int64_t *nwrap, int64_t *samples, const int32_t *reset)
{
    int rc = read_begin(c, &pigs_ctx::sf, "sf"); if (rc) return rc;
    if (!C || !D || !nwrap || !samples) return fail(PIGS_ERR_ARG, "null output");
    const SfState &f = c->sf;
    return read_and_reset(c, {{f.C, C}, {f.D, D}, {f.nwrap, nwrap}, {f.samples, samples}}, reset);
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
    if (!cutoff_in_box(c->P.dim, c->P.LboxHalf, rc, 0.0) || !window_ok(window, c->P.Nb))
        return fail(PIGS_ERR_ARG, "pigs_cl_init: rc=%g (0 < rc <= half the shortest side) window=%d (0..Nb=%d)", rc, window, c->P.Nb);
    if (c->P.Np > kClNpMax || cl_lds_bytes(c->P.dim, c->P.Np) > kClLdsBudget)
        return fail(PIGS_ERR_ARG, "pigs_cl_init: Np=%d passes the %d particles a workgroup labels in LDS", c->P.Np, kClNpMax);
    const size_t W = (size_t)c->n_walkers, np = (size_t)c->P.Np;
    if (acc_bytes_pass_2gib(W, 3 * np + 2))
        return fail(PIGS_ERR_ARG, "pigs_cl_init: %zu walkers x (3 x %d + 2) sums pass 2 GiB", W, c->P.Np);
    ClState &l = c->cl;
    const size_t slot = cl_slot_doubles(c->P.Np, window);
    const size_t slots = scratch_slots(W, kWalkerListMax, (size_t)l.scratch_mib * kMiB, slot * sizeof(double));
    st = init_begin(c, l); if (st) return st;
    HIPCHK(l.nsize.alloc(c, np));
    HIPCHK(l.nlarge.alloc(c, np));
    HIPCHK(l.nbond.alloc(c, 1));
    HIPCHK(l.samples.alloc(c, 1));
    HIPCHK(l.rg2.alloc(c, np));
    HIPCHK(alloc_zeroed(c, l.scratch, slots * slot));
    HIPCHK(alloc_zeroed(c, l.sweeps, 1));
    SYNC_CHECKED(c);
    l.window = window; l.slots = (int)slots; l.rc2 = rc * rc;
    l.ready = true;
    return PIGS_OK;
}

int pigs_cl_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    std::vector<int32_t> sw;
    int st = acc_begin(c, &pigs_ctx::cl, "cl", n, walkers, sw); if (st) return st;
    const ClState &l = c->cl;
    // one thread owns an element of rg2 per launch; a launch's walkers fit the scratch
    return each_launch(c, sw, walkers, true, l.slots, "launch_cl", [&](int m, const WalkerList &L) {
        return launch_cl(c->P, c->d_paths.p, m, L, l.window, l.rc2, l.scratch.p, l.nsize, l.nlarge, l.nbond, l.samples, l.rg2,
                         l.sweeps.p, c->stream);
    });
}

int pigs_cl_read(pigs_ctx *c, int64_t *nsize, int64_t *nlarge, int64_t *nbond, int64_t *samples, double *rg2, const int32_t *reset)
{
    int st = read_begin(c, &pigs_ctx::cl, "cl"); if (st) return st;
    if (!nsize || !nlarge || !nbond || !samples || !rg2) return fail(PIGS_ERR_ARG, "null output");
    const ClState &l = c->cl;
    return read_and_reset(c, {{l.nsize, nsize}, {l.nlarge, nlarge}, {l.nbond, nbond}, {l.samples, samples}, {l.rg2, rg2}}, reset);
}

int pigs_cl_sweeps(pigs_ctx *c, int32_t *max_sweeps)
{
    int st = read_begin(c, &pigs_ctx::cl, "cl"); if (st) return st;
    if (!max_sweeps) return fail(PIGS_ERR_ARG, "null output");
    unsigned int v = 0u;
    st = read_sweeps(c, c->cl.sweeps, &v, 1); if (st) return st;
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
    if (!cutoff_in_box(c->P.dim, c->P.LboxHalf, rc, 0.0) || !window_ok(window, c->P.Nb) || !lags_ok(ntau, window))
        return fail(PIGS_ERR_ARG, "pigs_pc_init: rc=%g (0 < rc <= half the shortest side) window=%d (0..Nb=%d) ntau=%d (0..2 window)",
                    rc, window, c->P.Nb, ntau);
    if (c->P.Np > kClNpMax || pc_lds_bytes(c->P.dim, c->P.Np) > kClLdsBudget)
        return fail(PIGS_ERR_ARG, "pigs_pc_init: Np=%d passes the %d particles a workgroup labels in LDS", c->P.Np, kClNpMax);
    const size_t W = (size_t)c->n_walkers, np = (size_t)c->P.Np, nl = (size_t)ntau + 1;
    if (acc_bytes_pass_2gib(W, 2 * np + 25 + 4 * nl))
        return fail(PIGS_ERR_ARG, "pigs_pc_init: %zu walkers x (2 x %d + 25 + 4 x %zu) sums pass 2 GiB", W, c->P.Np, nl);
    PcState &p = c->pc;
    const size_t slot = (2 * (size_t)window + 1) * np;
    const size_t slots = scratch_slots(W, kWalkerListMax, (size_t)p.scratch_mib * kMiB, pc_slot_bytes(c->P.Np, window));
    st = init_begin(c, p); if (st) return st;
    HIPCHK(p.nwrap.alloc(c, 8));
    HIPCHK(p.mwrap.alloc(c, 8));
    HIPCHK(p.swrap.alloc(c, 8));
    HIPCHK(p.nfin.alloc(c, np));
    HIPCHK(p.samples.alloc(c, 1));
    HIPCHK(p.first.alloc(c, nl));
    HIPCHK(p.second.alloc(c, nl));
    HIPCHK(p.both.alloc(c, nl));
    HIPCHK(p.norig.alloc(c, nl));
    HIPCHK(p.rg2u.alloc(c, np));
    HIPCHK(alloc_zeroed(c, p.scratch, slots * slot));
    HIPCHK(alloc_zeroed(c, p.labels, slots * slot));
    HIPCHK(alloc_zeroed(c, p.sweeps, 2));
    SYNC_CHECKED(c);
    p.window = window; p.ntau = ntau; p.slots = (int)slots; p.rc2 = rc * rc;
    p.ready = true;
    return PIGS_OK;
}

int pigs_pc_accumulate(pigs_ctx *c, int32_t n, const int32_t *walkers)
{
    std::vector<int32_t> sw;
    int st = acc_begin(c, &pigs_ctx::pc, "pc", n, walkers, sw); if (st) return st;
    const PcState &p = c->pc;
    const PcSums sums{p.nwrap, p.mwrap, p.swrap, p.nfin, p.samples, p.first, p.second, p.both, p.norig, p.rg2u};
    // one thread owns an element of rg2u per launch; a launch's walkers fit the scratches
    return each_launch(c, sw, walkers, true, p.slots, "launch_pc", [&](int m, const WalkerList &L) {
        return launch_pc(c->P, c->d_paths.p, m, L, p.window, p.ntau, p.rc2, p.scratch.p, p.labels.p, sums, p.sweeps.p, c->stream);
    });
}

int pigs_pc_read(pigs_ctx *c, int64_t *nwrap, int64_t *mwrap, int64_t *swrap, int64_t *nfin, int64_t *samples, double *rg2u,
                 int64_t *first, int64_t *second, int64_t *both, int64_t *norig, const int32_t *reset)
{
    int st = read_begin(c, &pigs_ctx::pc, "pc"); if (st) return st;
    if (!nwrap || !mwrap || !swrap || !nfin || !samples || !rg2u || !first || !second || !both || !norig)
        return fail(PIGS_ERR_ARG, "null output");
    const PcState &p = c->pc;
    return read_and_reset(c, {{p.nwrap, nwrap}, {p.mwrap, mwrap}, {p.swrap, swrap}, {p.nfin, nfin}, {p.samples, samples},
                              {p.rg2u, rg2u}, {p.first, first}, {p.second, second}, {p.both, both}, {p.norig, norig}}, reset);
}

int pigs_pc_sweeps(pigs_ctx *c, int32_t *label_sweeps, int32_t *image_sweeps)
{
    int st = read_begin(c, &pigs_ctx::pc, "pc"); if (st) return st;
    if (!label_sweeps || !image_sweeps) return fail(PIGS_ERR_ARG, "null output");
    unsigned int v[2] = {0u, 0u};
    st = read_sweeps(c, c->pc.sweeps, v, 2); if (st) return st;
    *label_sweeps = (int32_t)v[0];
    *image_sweeps = (int32_t)v[1];
    return PIGS_OK;
}

} // extern "C"
