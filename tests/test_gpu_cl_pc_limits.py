"""The cluster families (pigs_cl_*, pigs_pc_*) on the MI355X at their size limit, with image numbers far from zero, with
walker lists past one launch and beside the other families.

1. kClNpMax particles -- eight particles per thread, 32 mask words per bit-row sweep -- and the dynamic-LDS grant: above
   about 1000 particles k_cl and k_pc ask launch<> for more than kLdsNoGrant.  The constants come from the headers and
   cl_lds_bytes / pc_lds_bytes are restated here.  THE SEQUENCE TESTS COME FIRST IN THIS FILE: they run last-without-grant
   -> first-with-grant -> 65 -> kClNpMax per kernel instantiation in one process, and a larger grant of that instantiation
   before them would hide a missing first one.
2. The helices of tests/pc_numpy.py: one finite cluster whose image numbers run to +-23 at 300 particles and past 150 at
   kClNpMax, in one or in two fields at once, and the double winding whose closing bond misses by 2.
3. Lists of 300 walkers, beyond the kWalkerListMax = 256 of one launch, with repeated walkers.
4. cl and pc between bop, vh, grv, sf and lat on one context: every family keeps the bits it has alone.

The rules are those of test_gpu_cl.py and test_gpu_pc.py: every integer array EQUAL to the restatement (cl_numpy,
pc_numpy), rg2 / rg2u within 1e-12 * Sum|terms| per element with the restatement's bits where an element holds one term,
nothing masked or skipped.  Conditions on inputs are asserted on the restatement alone.

Largest |got - want| / bound, the sweep counts at kClNpMax and the wall times seen on the MI355X: DESIGN.md (the cluster
and the percolation section)."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import cl_numpy as cn
import lat_numpy
import pc_numpy as pn
from helpers import same_bits
from test_gpu_cl import ADJ_MAX, DENSITY, ST, _cfg
from test_gpu_cl import _assert_same as cl_same
from test_gpu_lds_grant import _product
from test_gpu_pc import SECOND_RADIUS
from test_gpu_pc import _assert_same as pc_same

pytestmark = pytest.mark.gpu

NP_MAX = _product("kClNpMax")
LDS_BUDGET = _product("kClLdsBudget")
NO_GRANT = _product("kLdsNoGrant", "pigs_launch.h")
LIST_MAX = _product("kWalkerListMax", "pigs_walker_split.h")
THREADS = _product("kClThreads")
SMALL = 65
ONE_D_SEED = 6                                         # chosen on the CPU: see test_one_dimension_with_a_cluster_beyond_1024


def cl_lds(dim, Np):
    """cl_lds_bytes (pigs_cl.hip): the slice, t and g in doubles, the bit rows up to kClAdjNpMax, three u32 arrays and two
    counters."""
    nw = (Np + 63) // 64
    return 8 * (dim * Np + 2 * Np) + (8 * Np * nw if Np <= ADJ_MAX else 0) + 4 * (3 * Np + 2)


def pc_lds(dim, Np):
    """pc_lds_bytes (pigs_pc.hip): the same doubles and bit rows, the packed image numbers (8 bytes in 3D, else 4), four
    u32 arrays and 17 counters."""
    nw = (Np + 63) // 64
    return 8 * (dim * Np + 2 * Np) + (8 * Np * nw if Np <= ADJ_MAX else 0) + (8 if dim == 3 else 4) * Np + 4 * (4 * Np + 17)


LDS = {"cl": cl_lds, "pc": pc_lds}


def crossing(fam, dim):
    """(the last Np whose launch asks for no grant, the first that asks for one) beyond the bit-row form."""
    first = min(n for n in range(ADJ_MAX + 1, NP_MAX + 1) if LDS[fam](dim, n) > NO_GRANT)
    return first - 1, first


def test_every_instantiation_crosses_the_grant_within_the_limit():
    """(No device work.)  The issue's figures: about 1023 for k_pc<3>, about 1260 for k_pc<2> and k_cl<3>, and about
    131 KB at the limit for k_pc<3>."""
    assert (NP_MAX, ADJ_MAX, LDS_BUDGET, NO_GRANT, LIST_MAX, THREADS) == (2048, 256, 160 * 1024, 64 * 1024, 256, 256)
    for fam in ("cl", "pc"):
        for dim in (1, 2, 3):
            last, first = crossing(fam, dim)
            f = LDS[fam]
            assert f(dim, SMALL) <= f(dim, last) <= NO_GRANT < f(dim, first) < f(dim, NP_MAX) <= LDS_BUDGET, (fam, dim)
            assert all(f(dim, n) < f(dim, n + 1) for n in range(ADJ_MAX + 1, NP_MAX)), (fam, dim)
    assert crossing("pc", 3) == (1022, 1023) and crossing("pc", 2) == (1259, 1260) and crossing("cl", 3) == (1260, 1261)
    assert pc_lds(2, 1259) == NO_GRANT                                  # k_pc<2>'s last size without a grant asks for exactly the limit
    assert pc_lds(3, NP_MAX) == 131140 and (NP_MAX + THREADS - 1) // THREADS == 8 and (NP_MAX + 63) // 64 == 32


# ---- the random slices, restated once ------------------------------------------------------------------------------------
class Case:
    """One walker of uniform points at DENSITY in the box of unequal sides; the restatements are computed on demand, once."""

    def __init__(self, dim, Np, window=0, ntau=0):
        self.dim, self.Np, self.window, self.ntau, self.Nb = dim, Np, window, ntau, max(window, 1)
        self.cfg = _cfg(dim, Np, self.Nb)
        self.L = self.cfg.Lbox[:dim]
        self.rc = cn.threshold_rc(dim, DENSITY[dim], self.L)
        self.P = cn.random_paths(1, 2 * self.Nb + 1, Np, self.L, np.random.default_rng(1000 * dim + Np))
        self._exp = {}

    def _timed(self, key, make):
        if key not in self._exp:
            t0 = time.perf_counter()
            self._exp[key] = make()
            print(f"restating {key} of dim {self.dim} Np {self.Np} window {self.window}: {time.perf_counter() - t0:.1f} s on the CPU")
        return self._exp[key]

    @property
    def cl(self):
        return self._timed("cl", lambda: cn.Window(self.P, self.Nb, self.window, self.L, self.rc).expected([0]))

    def pc(self, factor):
        return self._timed(f"pc x {factor}", lambda: pn.Window(self.P, self.Nb, self.window, self.L, factor * self.rc,
                                                                 self.ntau).expected([0]))


@functools.lru_cache(maxsize=None)
def random_case(dim, Np, window=0, ntau=0):
    return Case(dim, Np, window, ntau)


def conditions_at_the_limit(case, fam):
    """On the restatement alone, the middle slice at the threshold radius: bonds, a spread of sizes, a cluster of more than
    1024 particles (members in most of the 32 mask words and in all eight particle rounds; in 1D no radius of this kind
    gives one, see test_one_dimension_with_a_cluster_beyond_1024).  For pc in 2D and 3D a wrapping cluster of more than
    1024 particles, and at one of the two radii finite clusters of several particles with rg2u > 0."""
    mid = cn.slice_sums(case.P[0, case.Nb], case.L, case.rc)
    sizes = np.nonzero(mid[0])[0] + 1
    assert mid[2] > 0 and sizes.size >= 3, sizes
    if case.dim >= 2:
        assert sizes.max() > 1024, sizes.max()
        if fam == "pc":
            at, below = case.pc(1.0), case.pc(SECOND_RADIUS)
            assert at["nwrap"][0, 1:].sum() >= 1 and at["mwrap"][0, 1:].max() > 1024
            assert any(e["nfin"][0, 2:].sum() >= 3 and np.count_nonzero(e["rg2u"][0]) >= 3 for e in (at, below))


def run_cl(gpu_lib, cfg, P, rc, window, exp, what):
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=P.shape[0]) as ctx:
        ctx.upload_all(P)
        ctx.cl_init(rc, window)
        ctx.cl_accumulate()
        cl_same(ctx.cl_read(), exp, what)
        return ctx.cl_sweeps()


def run_pc(gpu_lib, cfg, P, rcs, window, ntau, exps, what):
    """pc_init again per radius on the one context; returns the sweep counts of the last."""
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=P.shape[0]) as ctx:
        ctx.upload_all(P)
        for rc, exp in zip(rcs, exps):
            ctx.pc_init(rc, window, ntau)
            ctx.pc_accumulate()
            got = ctx.pc_read()
            assert (got["window"], got["ntau"]) == (window, ntau)
            pc_same(got, exp, f"{what} rc {rc:.4f}")
        return ctx.pc_sweeps()


# ---- 1a. last without a grant -> first with one -> small -> the limit, per instantiation, in this order --------------------
@pytest.mark.parametrize("fam,dim", [("pc", 3), ("pc", 2), ("cl", 3)])
def test_grant_sequence_then_the_limit(gpu_lib, fam, dim):
    """grant_lds' grow-then-small-then-larger sequence.  (On the MI355X's runtime a launch above kLdsNoGrant also ran
    without the attribute having been set -- DESIGN.md, the percolation section -- so this pins the values at those sizes
    and that a grant, where asked, is not refused; it cannot tell that one was asked.)"""
    last, first = crossing(fam, dim)
    f = LDS[fam]
    sizes = [last, first, SMALL, NP_MAX]
    assert f(dim, SMALL) <= f(dim, last) <= NO_GRANT < f(dim, first) < f(dim, NP_MAX) <= LDS_BUDGET
    for Np in sizes:
        c = random_case(dim, Np)
        if Np == NP_MAX:
            conditions_at_the_limit(c, fam)
        what = f"k_{fam}<{dim}> Np {Np} lds {f(dim, Np)}"
        if fam == "cl":
            print(what, "sweeps", run_cl(gpu_lib, c.cfg, c.P, c.rc, 0, c.cl, what))
        else:
            print(what, "sweeps", run_pc(gpu_lib, c.cfg, c.P, [c.rc, SECOND_RADIUS * c.rc], 0, 0, [c.pc(1.0), c.pc(SECOND_RADIUS)], what))


# ---- 1b. the remaining instantiations at the limit alone, and 1077 (five rounds, one short) ---------------------------------
@pytest.mark.parametrize("fam,dim,Np", [("cl", 1, NP_MAX), ("cl", 2, NP_MAX), ("pc", 1, NP_MAX), ("cl", 3, 1077), ("pc", 3, 1077),
                                        ("pc", 2, 1077)])
def test_limit_alone_and_1077(gpu_lib, fam, dim, Np):
    """k_pc<1> at the limit runs window 1 with the lags 0..2: three slices of 2048 through k_pc_persist as well."""
    window, ntau = (1, 2) if (fam, dim) == ("pc", 1) else (0, 0)
    c = random_case(dim, Np, window, ntau)
    assert (Np + THREADS - 1) // THREADS == (8 if Np == NP_MAX else 5)
    if Np == NP_MAX:
        assert LDS[fam](dim, Np) > NO_GRANT
        conditions_at_the_limit(c, fam)
    else:
        mid = cn.slice_sums(c.P[0, c.Nb], c.L, c.rc)
        assert Np % THREADS == 53 and mid[2] > 0 and np.count_nonzero(mid[0]) >= 3 and mid[1] > 512
    what = f"k_{fam}<{dim}> Np {Np} window {window}"
    if fam == "cl":
        print(what, "sweeps", run_cl(gpu_lib, c.cfg, c.P, c.rc, window, c.cl, what))
    else:
        if window:
            at = c.pc(1.0)
            assert np.all(at["first"][0] > 0) and np.all(at["both"][0, 1:] < at["first"][0, 1:])
        print(what, "sweeps", run_pc(gpu_lib, c.cfg, c.P, [c.rc, SECOND_RADIUS * c.rc], window, ntau,
                                     [c.pc(1.0), c.pc(SECOND_RADIUS)], what))


def test_one_dimension_with_a_cluster_beyond_1024(gpu_lib):
    """In 1D no radius percolates: threshold_rc bonds 95 % of the gaps and the clusters stay short.  2.2 of it bonds all
    but a few gaps of 2048, and the seed leaves one cluster of more than 1024 particles beside smaller ones."""
    cfg = _cfg(1, NP_MAX, 1)
    L = cfg.Lbox[:1]
    rc = 2.2 * cn.threshold_rc(1, DENSITY[1], L)
    P = cn.random_paths(1, 3, NP_MAX, L, np.random.default_rng(ONE_D_SEED))
    cl = cn.Window(P, 1, 0, L, rc).expected([0])
    pc = pn.Window(P, 1, 0, L, rc).expected([0])
    sizes = np.nonzero(cl["nsize"][0])[0] + 1
    assert sizes.max() > 1024 and sizes.size >= 3 and pc["nfin"][0, 1024:].sum() == 1 and pc["rg2u"][0, sizes.max() - 1] > 0, sizes
    print("1D sweeps", run_cl(gpu_lib, cfg, P, rc, 0, cl, "k_cl<1> one large cluster"),
          run_pc(gpu_lib, cfg, P, [rc], 0, 0, [pc], "k_pc<1> one large cluster"))


# ---- 1c. chains and rings at the limit -----------------------------------------------------------------------------------
def orders(n):
    return {"ascending": np.arange(n), "shuffled": np.random.default_rng(n).permutation(n), "ends": cn.order_both_ends(n)}


def one_slice_both(gpu_lib, X, Lbox, rc, what):
    """X as the middle slice of one walker, cl and pc initialised on the one context: (cl_read, pc_read, label sweeps of
    cl, (label, image) sweeps of pc, seconds of the device part)."""
    Np, dim = X.shape
    cfg = _cfg(dim, Np, 1, Lbox=list(Lbox))
    P = cn.as_paths(X, 3)
    cl_exp = cn.Window(P, 1, 0, Lbox, rc).expected([0])
    pc_exp = pn.Window(P, 1, 0, Lbox, rc).expected([0])
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=1) as ctx:
        ctx.upload_all(P)
        ctx.cl_init(rc, 0)
        ctx.pc_init(rc, 0, 0)
        ctx.sync()
        t0 = time.perf_counter()
        ctx.cl_accumulate()
        ctx.pc_accumulate()
        cl, pc = ctx.cl_read(), ctx.pc_read()
        dt = time.perf_counter() - t0
        sw = ctx.cl_sweeps(), ctx.pc_sweeps()
    cl_same(cl, cl_exp, what)
    pc_same(pc, pc_exp, what)
    print(f"{what}: {sw[0]} labelling sweeps (cl), {sw[1][0]} labelling and {sw[1][1]} image sweeps (pc), {dt:.3f} s on the device")
    assert 1 <= sw[0] <= Np + 1 and 1 <= sw[1][0] <= Np + 1 and 1 <= sw[1][1] <= Np
    return cl, pc, cl_exp, pc_exp, sw


@pytest.mark.parametrize("order", ["ascending", "shuffled", "ends"])
@pytest.mark.parametrize("cut", [False, True])
def test_chain_at_the_limit(gpu_lib, order, cut):
    """kClNpMax particles on a line at 0.9 rc: one cluster of 2048 whatever the order of the indices; with one spacing of
    1.1 rc, two.  The ascending order is the slow one: up to Np - 1 image sweeps."""
    n, rc = NP_MAX, 1.0
    sp = np.full(n - 1, 0.9 * rc)
    if cut:
        sp[777] = 1.1 * rc
    Lbox = [4096.0, 8.0, 8.0]
    X = cn.chain(n, sp, orders(n)[order], origin=[-1000.0, 1.0, -2.0])
    assert np.all(np.abs(X) < 0.5 * np.asarray(Lbox))
    cl, pc, cl_exp, pc_exp, _ = one_slice_both(gpu_lib, X, Lbox, rc, f"chain {order} cut {cut}")
    sizes = [778, n - 778] if cut else [n]
    assert cl_exp["nbond"][0] == n - len(sizes) and sorted(np.nonzero(cl_exp["nsize"][0])[0] + 1) == sorted(sizes)
    assert all(cl["nsize"][0, s - 1] == 1 and pc["nfin"][0, s - 1] == 1 for s in sizes) and pc["nwrap"][0, 0] == len(sizes)
    assert same_bits(pc["rg2u"], cl["rg2"])                             # shorter than half the box: unfolded is folded


@pytest.mark.parametrize("order", ["ascending", "shuffled", "ends"])
def test_ring_at_the_limit(gpu_lib, order):
    n, rc = NP_MAX, 1.0
    Lbox = [0.9 * n, 8.0, 8.0]
    X = pn.ring(n, Lbox, 3, orders(n)[order], origin=[-140.0, 1.0, -2.0])
    cl, pc, cl_exp, pc_exp, _ = one_slice_both(gpu_lib, X, Lbox, rc, f"ring {order}")
    assert cl_exp["nbond"][0] == n and cl["nsize"][0, n - 1] == 1
    assert pc["nwrap"][0].tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and pc["mwrap"][0, 1] == n and pc["swrap"][0, 1] == 1
    assert not np.any(pc["nfin"]) and not np.any(pc["rg2u"])


# ---- 1d. the refusal ------------------------------------------------------------------------------------------------------
def test_library_refuses_one_particle_more(gpu_lib):
    """A real context of kClNpMax + 1 particles: the raw inits, and accumulate and read after them, answer PIGS_ERR_ARG;
    at exactly kClNpMax PIGS_OK."""
    ARG, OK = ST["PIGS_ERR_ARG"], ST["PIGS_OK"]
    for Np, want in ((NP_MAX + 1, ARG), (NP_MAX, OK)):
        cfg = _cfg(3, Np, 1)
        VT, WF = gpu_lib.build_tables(cfg)
        with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=1) as ctx:
            assert ctx.L.pigs_cl_np_max() == ctx.L.pigs_pc_np_max() == NP_MAX
            assert ctx.L.pigs_cl_init(ctx.h, C.c_double(1.0), 0) == want
            assert ctx.L.pigs_pc_init(ctx.h, C.c_double(1.0), 0, 0) == want
            d, l = np.zeros(Np + 8), np.zeros(Np + 8, np.int64)
            dp, lp = d.ctypes.data_as(C.POINTER(C.c_double)), l.ctypes.data_as(C.POINTER(C.c_int64))
            if want == ARG:
                assert ctx.L.pigs_cl_accumulate(ctx.h, 1, None) == ARG and ctx.L.pigs_pc_accumulate(ctx.h, 1, None) == ARG
                assert ctx.L.pigs_cl_read(ctx.h, lp, lp, lp, lp, dp, None) == ARG
                assert ctx.L.pigs_pc_read(ctx.h, lp, lp, lp, lp, lp, dp, lp, lp, lp, lp, None) == ARG
                with pytest.raises(gpu_lib.PigsError, match="Np"):
                    ctx.cl_init(1.0, 0)
                with pytest.raises(gpu_lib.PigsError, match="Np"):
                    ctx.pc_init(1.0, 0, 0)
            else:
                assert ctx.L.pigs_cl_accumulate(ctx.h, 0, None) == OK and ctx.L.pigs_pc_accumulate(ctx.h, 0, None) == OK
            ctx.sync()


# ---- 2. image numbers far from zero --------------------------------------------------------------------------------------
FAR = pn.far_images()


def far_slice(gpu_lib, name, X, L, rc):
    cl, pc, cl_exp, pc_exp, sw = one_slice_both(gpu_lib, X, L, rc, name)
    n = X.shape[0]
    m = pn.components(pn.bonds_of(X, L, rc), pn.fold_numbers(X, np.asarray(L, dtype=np.float64)))[1]
    print(f"{name}: the restatement's image numbers span {m.min(axis=0).tolist()} .. {m.max(axis=0).tolist()}")
    return cl, pc, cl_exp, pc_exp, m


def helix_asserts(name, n, cl, pc, cl_exp, pc_exp):
    assert pc["nfin"][0, n - 1] == 1 and pc["nfin"].sum() == 1 and pc["nwrap"][0].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    assert cl["nsize"][0, n - 1] == 1
    factor = pc_exp["rg2u"][0, n - 1] / cl_exp["rg2"][0, n - 1]
    got = pc["rg2u"][0, n - 1] / cl["rg2"][0, n - 1]
    print(f"{name}: rg2u {pc['rg2u'][0, n - 1]!r} over the folded rg2 {cl['rg2'][0, n - 1]!r} = {got:.6g} (restatements: {factor:.6g})")
    assert factor > 10.0 and pc["rg2u"][0, n - 1] > 0.999999 * factor * cl["rg2"][0, n - 1] > 0


@pytest.mark.parametrize("name", sorted(k for k in FAR if "helix" in k))
def test_helix_of_300(gpu_lib, name):
    X, L, rc, _ = FAR[name]
    cl, pc, cl_exp, pc_exp, m = far_slice(gpu_lib, name, X, L, rc)
    axes = (0, 1) if name.startswith("double") else (0,)
    assert all(m[:, k].max() >= 5 and m[:, k].min() <= -5 and np.abs(m[:, k]).max() >= 15 for k in axes)
    helix_asserts(name, X.shape[0], cl, pc, cl_exp, pc_exp)


def test_double_winding_of_300(gpu_lib):
    X, L, rc, _ = FAR["double_winding"]
    cl, pc, cl_exp, pc_exp, m = far_slice(gpu_lib, "double winding", X, L, rc)
    assert pc["nwrap"][0, 3] == 1 and pc["swrap"][0, 3] == 1 and pc["mwrap"][0, 3] == X.shape[0] and pc["nwrap"].sum() == 1


@pytest.mark.parametrize("dim", [2, 3])
def test_helix_at_the_limit(gpu_lib, dim):
    X, L, rc, _ = pn.helix(NP_MAX, dim)
    cl, pc, cl_exp, pc_exp, m = far_slice(gpu_lib, f"helix {dim}D at {NP_MAX}", X, L, rc)
    assert np.abs(m[:, 0]).max() >= 150 and min(m[:, 0].max(), -m[:, 0].min()) >= 70 and not np.any(m[:, 1:])
    helix_asserts(f"helix {dim}D at {NP_MAX}", NP_MAX, cl, pc, cl_exp, pc_exp)


# ---- 3. lists beyond one launch -------------------------------------------------------------------------------------------
def test_lists_of_300_walkers_with_repeats(gpu_lib):
    """300 walkers of five particles (two distinct worldlines, tiled), window 1 with the lags 0..2.  No list; then a list of
    300 entries in which walker 100 stands at 100 and at 270 -- on both sides of position kWalkerListMax -- and walker 3
    at 3 and at 10, inside the first launch."""
    W, Np, Nb, window, ntau, dim = 300, 5, 2, 1, 2, 3
    assert W > LIST_MAX
    cfg = _cfg(dim, Np, Nb)
    L = cfg.Lbox
    rc = cn.threshold_rc(dim, DENSITY[dim], L)
    P = cn.random_paths(2, 2 * Nb + 1, Np, L, np.random.default_rng(300))[np.arange(W) % 2].copy()
    lst = np.arange(W)
    lst[10], lst[270] = 3, 100
    mult = np.bincount(lst, minlength=W)
    assert mult[3] == 2 and mult[100] == 2 and mult[10] == 0 and mult[270] == 0 and mult.sum() == W
    assert list(lst).index(100) < LIST_MAX < W - 1 - list(lst[::-1]).index(100)
    ns = 2 * window + 1
    cw, pw = cn.Window(P, Nb, window, L, rc), pn.Window(P, Nb, window, L, rc, ntau)
    one = cw.expected([0, 1])
    assert one["nbond"][:2].min() > 0 and np.count_nonzero(one["nsize"][:2].sum(axis=0)) >= 2 and np.any(one["rg2"][:2] > 0)
    assert not np.array_equal(one["nsize"][0], one["nsize"][1])          # two worldlines that differ in what is counted
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for walkers, flat in ((None, list(range(W))), (lst, lst.tolist())):
            ctx.cl_init(rc, window)
            ctx.pc_init(rc, window, ntau)
            ctx.cl_accumulate(walkers)
            ctx.pc_accumulate(walkers)
            cl, pc = ctx.cl_read(), ctx.pc_read()
            want = ns * np.bincount(flat, minlength=W)
            assert cl["samples"].tolist() == want.tolist() and pc["samples"].tolist() == want.tolist()
            what = "no list" if walkers is None else "300 entries"
            cl_same(cl, cw.expected(flat), what)
            pc_same(pc, pw.expected(flat), what)
            assert np.array_equal(pc["norig"][:, 0], want)


# ---- 4. beside the other families ------------------------------------------------------------------------------------------
ROUND_1 = [("cl", None), ("bop", [2, 0, 2]), ("pc", [1, 1, 0]), ("vh", [2, 2, 1]), ("cl", [2, 0, 2]), ("grv", [1, 1, 0]),
           ("sf", [2, 0, 2]), ("pc", None), ("lat", [2, 2, 1])]
ROUND_2 = [("lat", None), ("pc", [0, 2, 0]), ("sf", [1]), ("cl", [1, 1]), ("grv", None), ("vh", [0, 0, 0]), ("pc", [2]),
           ("bop", None), ("cl", [0])]


def test_cl_and_pc_between_five_families_keep_their_own_bits(gpu_lib):
    """test_interleaved_thirteen_families_keep_their_own_bits' pattern on a periodic 3D context of 70 particles: cl and pc
    between bop, vh, grv, sf and lat, walkers repeated within the lists, two rounds in two call orders.  Every family has
    the bits of its own calls alone; cl and pc equal the restatement as well."""
    W, Np, Nb, window = 3, 70, 3, 2
    cfg = _cfg(3, Np, Nb)
    L = cfg.Lbox
    P = cn.random_paths(W, 2 * Nb + 1, Np, L, np.random.default_rng(70))
    rc = 0.9 * cn.threshold_rc(3, DENSITY[3], L)
    r = 0.5 * min(L)
    init = {"cl": (rc, window), "pc": (rc, window, 3), "bop": (rc, window, 20, 8, r / 8.0), "vh": (2, window, 6, r / 6.0, 4, r / 4.0),
            "grv": (4, window, 6, r / 6.0), "sf": (3, window), "lat": (lat_numpy.grid_sites(3, 5, L, Np), 4, r, window, 1)}
    calls = ROUND_1 + ROUND_2
    assert set(init) == {c[0] for c in ROUND_1} == {c[0] for c in ROUND_2} and [c[0] for c in ROUND_1] != [c[0] for c in ROUND_2]
    VT, WF = gpu_lib.build_tables(cfg)

    def run(families):
        with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
            ctx.upload_all(P)
            for f in families:
                getattr(ctx, f + "_init")(*init[f])
            for f, walkers in calls:
                if f in families:
                    getattr(ctx, f + "_accumulate")(walkers)
            return {f: getattr(ctx, f + "_read")() for f in families}

    together = run(list(init))
    for f in init:
        alone = run([f])[f]
        assert sorted(alone) == sorted(together[f])
        flat = [w for g, wl in calls if g == f for w in (range(W) if wl is None else wl)]
        assert alone["samples"].tolist() == ((2 * window + 1) ** (f in ("cl", "pc")) * np.bincount(flat, minlength=W)).tolist(), f
        assert any(np.any(a != 0) for k, a in alone.items() if isinstance(a, np.ndarray) and k != "samples"), f
        for k, a in alone.items():
            t = together[f][k]
            if not isinstance(a, np.ndarray):
                assert a == t, (f, k)
                continue
            assert a.shape == t.shape and a.dtype == t.dtype, (f, k)
            assert same_bits(a, t) if a.dtype == np.float64 else np.array_equal(a, t), (f, k)
        if f == "cl":
            exp = cn.Window(P, Nb, window, L, rc).expected(flat)
            assert np.any(exp["terms"] > 1)
            cl_same(together[f], exp, "cl between the others")
        if f == "pc":
            exp = pn.Window(P, Nb, window, L, rc, 3).expected(flat)
            assert exp["nwrap"][:, 1:].sum() > 0 and exp["nfin"][:, 1:].sum() > 0
            pc_same(together[f], exp, "pc between the others")
