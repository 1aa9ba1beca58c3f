"""The floating-point outputs of the slice-window kernels, bit for bit (pigs_atm.hip's T; pigs_bop.hip's S and G).

test_gpu_atm.py and test_gpu_bop.py hold these sums to numpy within a tolerance.  They are IEEE operations in a fixed order
under -ffp-contract=off, so their bits are a property of the source: tests/golden/window_bits.npz (written by
tests/golden/make_window_bits.py, by hand, on a commit whose kernels passed those tolerance tests) keeps the worldlines
themselves and every array that atm_read() and bop_read() returned for them.  A change of a kernel's arithmetic or of its
order of summation moves a bit here; a change that is meant to do so records the fixture again and says so.

Shapes: three walkers listed out of order in one list; (Nb, window) = (1, 0) and (2, 2), i.e. 1 and 5 slices, the first on
the three middle slices of the same worldlines.
  atm  Np = 3 (one triplet), 5 and 6 (a cluster within rc: every partner a leg, odd and even leg counts, a middle row of the
       joined triangle that joins itself), 66 (a second round of 64 partners), 131 (a vertex with more than 64 legs: the
       pair walk's row step is 0 and only its column carries); rc = half the box.
  bop  Np = 5, 66, 257 (more particles than the workgroup has threads); Nr = 0 and 8; rnb a first-shell radius.
No comparison masks or skips an element."""
import numpy as np
import pytest

from conftest import load_golden
from helpers import same_bits
from pathintegralgroundstate_amd import SystemConfig

pytestmark = pytest.mark.gpu
DENSITY = {2: 0.25, 3: 0.365}
WINDOWS = ((1, 0), (2, 2))                                          # (Nb, window)
ORDER = [2, 0, 1]                                                   # the walker list
ATM_NP = (3, 5, 6, 66, 131)
BOP_NP = (5, 66, 257)
BOP_NR = (0, 8)
NH = 20


def config(fix, dim, Np, Nb):
    """The box side comes from the fixture, not from a power function of this machine."""
    return SystemConfig(dim=dim, Np=Np, Nb=Nb, density=DENSITY[dim], Lbox=[float(fix[f"box_d{dim}_n{Np}"])] * dim)


def worldlines(fix, dim, Np, Nb):
    """[3, 2 Nb + 1, Np, dim]: the stored worldlines have five slices (Nb = 2); Nb = 1 takes the three in the middle."""
    P = fix[f"paths_d{dim}_n{Np}"]
    assert P.shape == (3, 5, Np, dim) and P.dtype == np.float64
    return np.ascontiguousarray(P[:, 2 - Nb:3 + Nb])


def atm_arrays(api, fix, dim, Np, Nb, window):
    """{name in the fixture: array} of atm_read() after one call with the list ORDER."""
    cfg = config(fix, dim, Np, Nb)
    VT, WF = api.build_tables(cfg)
    with api.PigsContext(cfg, VT, WF, n_walkers=3) as ctx:
        ctx.upload_all(worldlines(fix, dim, Np, Nb))
        ctx.atm_init(cfg.rcut, window)
        ctx.atm_accumulate(ORDER)
        got = ctx.atm_read()
    return {f"atm_d{dim}_n{Np}_b{Nb}_{k}": v for k, v in got.items()}


def bop_arrays(api, fix, dim, Np, Nb, window):
    """{name in the fixture: array} of bop_read() after one call with the list ORDER, for every Nr of BOP_NR."""
    cfg = config(fix, dim, Np, Nb)
    VT, WF = api.build_tables(cfg)
    out = {}
    with api.PigsContext(cfg, VT, WF, n_walkers=3) as ctx:
        ctx.upload_all(worldlines(fix, dim, Np, Nb))
        for Nr in BOP_NR:
            ctx.bop_init(float(fix[f"rnb_d{dim}_n{Np}"]), window, NH, Nr, cfg.rcut / Nr if Nr else 0.0)
            ctx.bop_accumulate(ORDER)
            out.update({f"bop_d{dim}_n{Np}_b{Nb}_r{Nr}_{k}": v for k, v in ctx.bop_read().items()})
    return out


@pytest.fixture(scope="module")
def fix():
    return load_golden("window_bits")


def _assert_recorded(fix, got, floats):
    """Every array of `got` against the fixture's; `floats`: the names that are float64, the others are int64."""
    assert any(k.rsplit("_", 1)[1] in floats for k in got)
    for k, v in got.items():
        assert v.shape == fix[k].shape and v.dtype == fix[k].dtype, (k, v.shape, v.dtype)
        assert v.dtype == (np.float64 if k.rsplit("_", 1)[1] in floats else np.int64), (k, v.dtype)
        assert same_bits(v, fix[k]), (k, int(np.count_nonzero(v != fix[k])), v.size)
        assert v.any() or v.size == 0, k                                # (Nr = 0: G and GN have no bins)


@pytest.mark.parametrize("Nb,window", WINDOWS)
@pytest.mark.parametrize("Np", ATM_NP)
@pytest.mark.parametrize("dim", [2, 3])
def test_atm_has_the_recorded_bits(gpu_lib, fix, dim, Np, Nb, window):
    _assert_recorded(fix, atm_arrays(gpu_lib, fix, dim, Np, Nb, window), ("T",))


@pytest.mark.parametrize("Nb,window", WINDOWS)
@pytest.mark.parametrize("Np", BOP_NP)
@pytest.mark.parametrize("dim", [2, 3])
def test_bop_has_the_recorded_bits(gpu_lib, fix, dim, Np, Nb, window):
    _assert_recorded(fix, bop_arrays(gpu_lib, fix, dim, Np, Nb, window), ("S", "G"))
