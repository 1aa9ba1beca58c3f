"""Every per-walker accumulator family initialised a second time on the MI355X, with another shape: each array's size per
walker is written once, in the family's *_init, and *_read takes it from there (csrc/pigs_ctx.h: Acc), so after
init(A), accumulate, init(B) a family must be exactly a fresh context's init(B) -- B's shapes, all zeros, then the same
bits -- and before its *_init every entry point refuses.  The system of test_gpu_accumulator_families.py (dim 2, Np 5,
Nb 3, three walkers); density on a trapped context of the same size, nk through nk_add."""
import numpy as np
import pytest

import lat_numpy
from pathintegralgroundstate_amd import SystemConfig
from pathintegralgroundstate_amd.api import PigsError

pytestmark = pytest.mark.gpu

W = 3
CFG = SystemConfig(dim=2, Np=5, Nb=3, density=0.25)
TRAP = SystemConfig(dim=2, Np=5, Nb=3, trap=True, a_ho=[1.0, 1.3], Nmax=2000, Rm=1.2, dt=0.01)
RC = CFG.rcut
# the shapes a family is given one after the other: every size parameter changes from one to the next, and where a family
# has a switch one step crosses it (bop: Nr 3 -> 0 -> 3, G6(r) off and on again; sf, cl: the window 1 -> 2; pc: ntau 0 -> 2)
SHAPES = {
    "density": [(4, 2.0), (7, 3.0)],                                                    # Nbin, half_width
    "fqt": [(3, 2, 1), (2, 3, 2)],                                                      # Nk, Ntau, window
    "tau": [(), ()],
    "sqv": [(2, 1), (1, 2)],                                                            # nmax, window
    "fqv": [(2, 2, 1), (1, 3, 2)],                                                      # nmax, Ntau, window
    "fqs": [(2, 2, 1), (1, 3, 2)],
    "grv": [(4, 1, 3, RC / 3.0), (5, 2, 4, RC / 4.0)],                                  # Nbin, window, Nr, rbin
    "bop": [(RC, 1, 4, 3, RC / 3.0), (0.9 * RC, 2, 5, 0, 0.0), (RC, 3, 6, 3, RC / 3.0)],  # rnb, window, Nh, Nr, rbin
    "vh": [(2, 1, 3, RC / 3.0, 4, RC / 4.0), (3, 2, 5, RC / 5.0, 3, RC / 3.0)],         # Ntau, window, Nr, rbin, Ns, sbin
    "g3": [(2, RC / 2.0, 3, 1), (3, RC / 3.0, 2, 2)],                                   # Nr, rbin, Na, window
    "atm": [(RC, 1), (0.8 * RC, 2)],                                                    # rc, window
    "nk": [(2, 3), (1, 4)],                                                             # nmax, nbin
    "lat": [(lat_numpy.grid_sites(2, 3, CFG.Lbox, 5), 4, RC, 2, 1),                     # sites, nbin, rmax, window, cm
            (lat_numpy.grid_sites(2, 3, CFG.Lbox, 7), 5, 0.8 * RC, 1, 0)],
    "sf": [(1, 1), (3, 2)],                                                             # Ntau, window
    "cl": [(RC, 1), (0.8 * RC, 2)],                                                     # rc, window
    "pc": [(RC, 1, 0), (0.8 * RC, 2, 2)],                                               # rc, window, ntau
}
FAMILIES = list(SHAPES)
FIRST = [2, 0, 2]                   # the walkers of the accumulate under the first shape: one listed twice
LATER = [1, 2, 1, 0]                # under every later shape: all of them, one listed twice
# set before the first *_init; they live in the family's state and must outlive every later *_init.  What this file can see
# of that: the forms through test_forced_forms_outlive_a_second_init; of the scratch budget, at this size where one MiB
# holds every walker, only that a context carrying it keeps the bits (tests/test_gpu_sf_windows.py has the sizes it cuts).
TUNING = {"vh": ("vh_form", 0), "g3": ("g3_form", 0), "grv": ("grv_form", 0), "sf": ("sf_scratch_mib", 1)}


@pytest.fixture(scope="module")
def system(gpu_lib):
    """per kind of context (trapped or periodic): config, tables, worldlines; and the head/tail pairs of nk_add"""
    rng = np.random.default_rng(20261020)
    L = np.asarray(CFG.Lbox[:CFG.dim])
    out = {"periodic": (CFG,) + tuple(gpu_lib.build_tables(CFG)) + (rng.uniform(-0.5, 0.5, (W,) + tuple(CFG.path_shape)) * L,),
           "trap": (TRAP,) + tuple(gpu_lib.build_tables(TRAP)) + (rng.normal(0.0, 0.8, (W,) + tuple(TRAP.path_shape)),)}
    out["pairs"] = rng.uniform(-0.5, 0.5, (2 * len(LATER), 2, CFG.dim)) * L
    return out


def _context(gpu_lib, system, fam):
    cfg, VT, WF, P = system["trap" if fam == "density" else "periodic"]
    ctx = gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W)
    ctx.upload_all(P)
    if fam in TUNING:
        ctx.set_tuning(*TUNING[fam])
    return ctx


def _accumulate(ctx, system, fam, walkers):
    if fam == "nk":                 # two pairs per listed walker
        ctx.nk_add(walkers, [2] * len(walkers), system["pairs"][:2 * len(walkers)])
    else:
        getattr(ctx, fam + "_accumulate")(walkers)


def _same_bits(a, b, what):
    assert list(a) == list(b), what
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and a[k].dtype.itemsize == 8, (what, k)
            assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), (what, k)
        else:                       # the plain entries: window, ntau
            assert type(a[k]) is int and a[k] == b[k], (what, k)


@pytest.mark.parametrize("fam", FAMILIES)
def test_second_init_is_a_fresh_init(gpu_lib, system, fam):
    shapes = SHAPES[fam]
    count = "nopen" if fam == "nk" else "samples"
    with _context(gpu_lib, system, fam) as ctx:
        getattr(ctx, fam + "_init")(*shapes[0])
        _accumulate(ctx, system, fam, FIRST)
        n = getattr(ctx, fam + "_read")()[count]
        assert n[0] > 0 and n[1] == 0 and n[2] == 2 * n[0], (fam, n)                    # a walker listed twice is added twice
        for shape in shapes[1:]:
            with _context(gpu_lib, system, fam) as fresh:
                getattr(fresh, fam + "_init")(*shape)
                empty = getattr(fresh, fam + "_read")()
                _accumulate(fresh, system, fam, LATER)
                want = getattr(fresh, fam + "_read")()
            getattr(ctx, fam + "_init")(*shape)
            got = getattr(ctx, fam + "_read")()
            _same_bits(got, empty, (fam, shape, "after init"))
            assert not any(np.any(v) for v in got.values() if isinstance(v, np.ndarray)), (fam, shape)
            _accumulate(ctx, system, fam, LATER)
            got = getattr(ctx, fam + "_read")()
            _same_bits(got, want, (fam, shape, "accumulated"))
            assert np.all(got[count] > 0) and got[count][1] == 2 * got[count][0], (fam, shape)
        # the last shape: a read that resets walker 1 returns what stood, and zeroes walker 1 alone in every array
        _same_bits(getattr(ctx, fam + "_read")(reset=[0, 1, 0]), want, (fam, "the read that resets"))
        after = getattr(ctx, fam + "_read")()
        for k, v in after.items():
            if isinstance(v, np.ndarray):
                assert not np.any(v[1]), (fam, k)
                assert np.array_equal(v[[0, 2]].view(np.uint64), want[k][[0, 2]].view(np.uint64)), (fam, k)


@pytest.mark.parametrize("fam", FAMILIES)
def test_before_init_every_entry_point_refuses(gpu_lib, system, fam):
    """pigs_<fam>_read and _accumulate (nk: _add too) before pigs_<fam>_init: PIGS_ERR_ARG, "pigs_<fam>_init first" -- asked
    of the library itself, with null outputs (the init check comes before theirs)."""
    text = "pigs_%s_init first" % fam
    with _context(gpu_lib, system, fam) as ctx:
        names = ["read", "accumulate"] + (["add"] if fam == "nk" else [])
        for name in names:
            fn = getattr(ctx.L, "pigs_%s_%s" % (fam, name))
            args = [None] * (len(fn.argtypes) - 1)
            if name != "read":
                args[0] = W
            assert fn(ctx.h, *args) == -1, (fam, name)                                  # PIGS_ERR_ARG
            assert ctx.L.pigs_last_error().decode() == text, (fam, name)
        with pytest.raises(PigsError, match=text):
            _accumulate(ctx, system, fam, FIRST)
        with pytest.raises(PigsError, match="%s_init first" % fam):
            getattr(ctx, fam + "_read")()


def test_forced_forms_outlive_a_second_init(gpu_lib, system):
    """vh_form set before the first pigs_vh_init, then a second pigs_vh_init whose 7 x (20000 + 20000) counters are far too
    many for the LDS.  The forced 0 (global atomics) still runs there; 1 is still accepted as a value, and as it was set
    before the third pigs_vh_init and refuses the accumulate after it, the form is the state's, not the *_init's."""
    big = (6, 3, 20000, RC / 20000.0, 20000, RC / 20000.0)
    with _context(gpu_lib, system, "vh") as ctx:                                        # (vh_form = 0 is set in there)
        ctx.vh_init(*SHAPES["vh"][0])
        ctx.vh_accumulate(FIRST)
        ctx.vh_init(*big)
        ctx.vh_accumulate(LATER)
        got = ctx.vh_read()
        n = got["samples"]
        assert n[0] > 0 and n[1] == 2 * n[0] and n[2] == n[0] and got["self"].shape == (W, 7, 20000) and got["self"].sum() > 0
        ctx.set_tuning("vh_form", 1)
        ctx.vh_init(*big)
        with pytest.raises(PigsError, match="vh_form = 1, but 7 x \\(20000 \\+ 20000\\) counters do not fit the LDS"):
            ctx.vh_accumulate(LATER)
        assert not np.any(ctx.vh_read()["samples"])
        ctx.vh_init(*SHAPES["vh"][1])                                                   # where the forced 1 fits, it runs
        ctx.vh_accumulate(LATER)
        forced = ctx.vh_read()
    with _context(gpu_lib, system, "vh") as fresh:
        fresh.vh_init(*SHAPES["vh"][1])
        fresh.vh_accumulate(LATER)
        _same_bits(forced, fresh.vh_read(), "vh form 1 against form 0")
