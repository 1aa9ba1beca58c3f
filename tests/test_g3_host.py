"""The triplet key on a machine without a GPU: the Fortran normalisation and writers of the front end (pigs_estimators
normalize_g3 / write_g3 / write_g3ang, through the host library's hook hs_g3_files) against
pathintegralgroundstate_amd.profiles.normalize_g3 / bond_angle, profiles.kirkwood_g3 on an analytic g2, and the front
end's refusals on the CPU twin (the host built against tests/shim, which does not provide pigs_g3_*)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from hostlib import build_cpu_host
from pathintegralgroundstate_amd import profiles

RUNS = os.path.join(GOLDEN, "vpi_runs")
PBC = os.path.join(RUNS, "he4_cworm0", "vpi.in")                  # 2D
TRAP = os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")
PRINT = 1.0000001e-9                                             # the files carry 10 significant digits


def _key(extra=""):
    return f"&gpu\n triplet = T{extra}\n/\n"


@pytest.fixture(scope="module")
def cpu_host():
    return build_cpu_host()


@pytest.fixture(scope="module")
def cpu_exe(cpu_host):
    return cpu_host[2]


def _run(exe, txt, wd):
    os.makedirs(wd, exist_ok=True)
    with open(os.path.join(wd, "vpi.in"), "w") as f:
        f.write(txt)
    with open(os.path.join(wd, "vpi.in")) as fin:
        r = subprocess.run([exe], stdin=fin, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=wd, timeout=600)
    return r.returncode, r.stdout.decode(errors="replace")


def _short(txt):
    txt = re.sub(r"Nblock\s*=\s*\d+", "Nblock = 2", txt)
    return re.sub(r"Nstep\s*=\s*\d+", "Nstep = 3", txt)


def _hook(cpu_host):
    _, hostlib, _ = cpu_host
    # the host library finds the shim it was linked against by its run path.  The shim is NOT loaded into the global
    # scope: this file runs before the GPU tests of a whole-suite run, and the shim's pigs_* symbols would then take the
    # place of libpigs_hip.so's own in that library's internal calls.
    H = C.CDLL(hostlib)
    lp, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    H.hs_g3_files.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, lp, lp, lp,
                              dp, dp, dp, C.c_char_p, C.c_char_p]
    H.hs_g3_files.restype = None

    def call(dim, Np, density, window, Nr, rbin, Na, S, ctrip, cpair, f3, fa):
        nb, npk = len(S), Nr * (Nr + 1) // 2
        assert ctrip.shape == (nb, npk, Na) and cpair.shape == (nb, Nr) and ctrip.dtype == np.int64
        g2, g3, pa = np.zeros(Nr), np.zeros((npk, Na)), np.zeros(Na)
        H.hs_g3_files(dim, Np, density, window, Nr, rbin, Na, nb, S.ctypes.data_as(lp), ctrip.ctypes.data_as(lp),
                      cpair.ctypes.data_as(lp), g2.ctypes.data_as(dp), g3.ctypes.data_as(dp), pa.ctypes.data_as(dp),
                      f3.encode(), fa.encode())
        return g2, g3, pa
    return call


@pytest.mark.parametrize("dim", [2, 3])
def test_fortran_normalisation_and_writers_match_the_package(cpu_host, tmp_path, dim):
    """Random counts of three blocks of one walker: the last block's g2, g3, P(cos theta) from Fortran against
    normalize_g3 / bond_angle, and g3_vpi.out / g3ang_vpi.out (mean, error over the blocks) against numpy on the
    package's block values."""
    call = _hook(cpu_host)
    rng = np.random.default_rng(40 + dim)
    Np, density, window, Nr, rbin, Na, nb = 37, 0.365, 3, 5, 0.37, 7, 3
    npk = Nr * (Nr + 1) // 2
    S = np.array([4, 1, 7], np.int64)
    ctrip = rng.integers(0, 100000, (nb, npk, Na)).astype(np.int64)
    cpair = rng.integers(0, 1000, (nb, Nr)).astype(np.int64)
    f3, fa = str(tmp_path / "g3_vpi.out"), str(tmp_path / "g3ang_vpi.out")
    g2, g3, pa = call(dim, Np, density, window, Nr, rbin, Na, S, ctrip, cpair, f3, fa)
    blocks = [profiles.normalize_g3({"trip": ctrip[b], "pair": cpair[b], "samples": S[b]}, Np, window, density, rbin, dim)
              for b in range(nb)]
    angs = [profiles.bond_angle(ctrip[b], Nr) for b in range(nb)]
    assert np.allclose(g2, blocks[-1]["g2"], rtol=1e-13, atol=0) and np.allclose(g3, blocks[-1]["g3"], rtol=1e-13, atol=0)
    assert np.allclose(pa, angs[-1], rtol=1e-13, atol=0) and g3.min() > 0
    assert abs(pa.sum() * 2.0 / Na - 1.0) < 1e-13                       # P(cos theta) integrates to 1
    n = blocks[0]
    lead3 = np.stack([np.repeat(n["r"][n["lo"]], Na), np.repeat(n["r"][n["hi"]], Na), np.tile(n["cos"], npk)], axis=1)
    for f, x, lead in ((f3, np.stack([b["g3"] for b in blocks]).reshape(nb, -1), lead3), (fa, np.stack(angs), n["cos"][:, None])):
        tab = np.loadtxt(f)
        assert tab.shape == (x.shape[1], lead.shape[1] + 2), (f, tab.shape)
        mean = x.mean(axis=0)
        err = np.sqrt(np.maximum((x * x).mean(axis=0) - mean * mean, 0.0) / nb)
        assert np.allclose(tab[:, :-2], lead, rtol=PRINT, atol=0)
        assert np.allclose(tab[:, -2], mean, rtol=PRINT, atol=0)
        assert np.all(np.abs(tab[:, -1] - err) <= np.sqrt(4.0 * mean * PRINT * mean) + PRINT * err)


@pytest.mark.parametrize("dim", [2, 3])
def test_angle_weights_sum_to_one_and_the_diagonal_carries_one_half(cpu_host, tmp_path, dim):
    """The same count T in every bin: T / (g3 S Np density^2 vol_lo vol_hi m) is the angle weight w(q) of the Fortran side.
    It sums to 1 over q for every leg pair when m = 1/2 on the diagonal and 1 off it; in 2D it is the arc share of the
    bin, in 3D 1/Na."""
    call = _hook(cpu_host)
    Np, density, window, Nr, rbin, Na, T = 11, 0.3, 1, 4, 0.4, 6, 1000
    npk = Nr * (Nr + 1) // 2
    S = np.array([2], np.int64)
    ctrip = np.full((1, npk, Na), T, np.int64)
    cpair = np.full((1, Nr), 5, np.int64)
    _, g3, pa = call(dim, Np, density, window, Nr, rbin, Na, S, ctrip, cpair, str(tmp_path / "a"), str(tmp_path / "b"))
    r = (np.arange(Nr) + 0.5) * rbin
    vol = profiles.unit_ball(dim) * ((r + 0.5 * rbin) ** dim - (r - 0.5 * rbin) ** dim)
    lo, hi = profiles.g3_pairs(Nr)
    m = np.where(lo == hi, 0.5, 1.0)
    w = T / (g3 * (S[0] * (2 * window + 1) * Np * density ** 2) * (vol[lo] * vol[hi] * m)[:, None])
    assert np.allclose(w.sum(axis=1), 1.0, rtol=1e-13, atol=0)
    assert np.allclose(w, profiles.g3_angle_weights(Na, dim)[None, :], rtol=1e-12, atol=0)
    if dim == 2:
        edges = np.arccos(np.clip(-1.0 + 2.0 * np.arange(Na + 1) / Na, -1, 1))
        assert np.allclose(w[0], (edges[:-1] - edges[1:]) / np.pi, rtol=1e-12) and w[0, 0] > w[0, Na // 2]
    else:
        assert np.allclose(w, 1.0 / Na, rtol=1e-13)
    # the 1/2: a diagonal bin reads twice what the same count gives off the diagonal at the same volumes
    d = profiles.normalize_g3({"trip": ctrip[0], "pair": cpair[0], "samples": S[0]}, Np, window, density, rbin, dim)["g3"]
    u = profiles.unpack_g3(d)
    assert np.allclose(u[1, 1] * vol[1] * vol[1], 2.0 * u[1, 2] * vol[1] * vol[2], rtol=1e-13)
    assert np.array_equal(u, u.transpose(1, 0, 2)) and np.allclose(pa, 0.5, rtol=1e-13)


def test_kirkwood_on_an_analytic_g2():
    """g(r) = 1 + r/2 is linear, so the interpolation between mid-points is exact: g(r) g(s) g(t) in closed form wherever t
    lies between the first and the last mid-point, NaN from rmax on, the end values outside the mid-points."""
    Nr, rbin, Na = 8, 0.25, 9
    r = (np.arange(Nr) + 0.5) * rbin
    g = 1.0 + 0.5 * r
    k = profiles.kirkwood_g3(g, rbin, Na)
    lo, hi = profiles.g3_pairs(Nr)
    c = -1.0 + (np.arange(Na) + 0.5) * 2.0 / Na
    t = np.sqrt((r[lo] ** 2 + r[hi] ** 2)[:, None] - 2.0 * (r[lo] * r[hi])[:, None] * c)
    assert k.shape == (Nr * (Nr + 1) // 2, Na)
    assert np.array_equal(np.isnan(k), t >= Nr * rbin) and np.isnan(k).any()
    mid = (t >= r[0]) & (t <= r[-1])
    assert mid.sum() > 100
    assert np.allclose(k[mid], ((g[lo] * g[hi])[:, None] * (1.0 + 0.5 * t))[mid], rtol=1e-13)
    below, above = t < r[0], (t > r[-1]) & (t < Nr * rbin)
    assert below.any() and above.any()
    assert np.allclose(k[below], ((g[lo] * g[hi])[:, None] * g[0] * np.ones_like(t))[below], rtol=1e-14)
    assert np.allclose(k[above], ((g[lo] * g[hi])[:, None] * g[-1] * np.ones_like(t))[above], rtol=1e-14)
    assert np.allclose(profiles.kirkwood_g3(np.ones(Nr), rbin, Na)[~np.isnan(k)], 1.0)     # no correlation: 1


def test_bond_angle_takes_the_legs_below_nshell():
    Nr, Na = 4, 5
    trip = np.arange(Nr * (Nr + 1) // 2 * Na, dtype=np.int64).reshape(-1, Na) + 1
    u = profiles.unpack_g3(trip)
    for nshell in (1, 2, 4):
        i, j = np.triu_indices(nshell)
        h = u[i, j].sum(axis=0).astype(float)
        p = profiles.bond_angle(trip, nshell)
        assert np.allclose(p, h / (h.sum() * 2.0 / Na), rtol=1e-14) and abs(p.sum() * 2.0 / Na - 1.0) < 1e-14
    assert not profiles.bond_angle(np.zeros_like(trip), 2).any()
    with pytest.raises(ValueError):
        profiles.bond_angle(trip, Nr + 1)


def test_cpu_twin_still_links_against_the_unchanged_shim(cpu_exe):
    """The front end names no pigs_g3_* symbol at link time: the shim does not define them and it still links."""
    nm = subprocess.run(["nm", "-u", cpu_exe], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
    assert b"pigs_ctx_create" in nm.stdout and b"pigs_g3" not in nm.stdout
    assert b"g3_rmax" in open(cpu_exe, "rb").read()            # the front end knows the keys


def test_key_is_refused_by_a_backend_without_the_entry_points(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(", g3_nr = 4"), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "triplet" in out and "backend" in out and all(s in out for s in ("pigs_g3_init", "_accumulate", "_read")), out
    assert not os.path.exists(tmp_path / "g3_vpi.out") and not os.path.exists(tmp_path / "e_vpi.out")


def test_key_is_refused_for_a_trapped_system(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, open(TRAP).read() + _key(), str(tmp_path))
    assert rc == 2
    assert "triplet" in out and "periodic" in out and "pigs_g3" not in out, out


@pytest.mark.parametrize("extra,word", [(", g3_window = 1000", "g3_window"), (", g3_nr = 0", "g3_nr"), (", g3_nr = 1025", "g3_nr"),
                                        (", g3_na = 0", "g3_na"), (", g3_na = 1025", "g3_na"), (", g3_rmax = 1.d3", "g3_rmax")])
def test_out_of_range_keys_are_refused(cpu_exe, tmp_path, extra, word):
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(extra), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "triplet" in out and word in out and "pigs_g3" not in out, out          # refused for the values, not the backend
    assert not os.path.exists(tmp_path / "e_vpi.out")


def test_limits_and_defaults_are_accepted_for_their_values(cpu_exe, tmp_path):
    """g3_rmax left out (the run's rcut), zero or at half the side, g3_window left out, g3_nr = g3_na = 1024: the value
    checks pass (and the run is then refused for the backend)."""
    for extra in ("", ", g3_rmax = 0.d0, g3_nr = 1024, g3_na = 1024", ", g3_rmax = -1.d0, g3_window = 0"):
        rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(extra), str(tmp_path))
        assert rc == 2 and "pigs_g3" in out, out


def test_run_without_the_key_is_its_golden_files(cpu_exe, tmp_path):
    """The golden run with the key spelled out as off: byte-identical to the golden files."""
    gold = os.path.join(RUNS, "he4_cworm0")
    rc, out = _run(cpu_exe, open(PBC).read() + "&gpu\n triplet = F, g3_nr = 3, g3_na = 4, g3_rmax = 1.5\n/\n", str(tmp_path))
    assert rc == 0 and "Triplet" not in out, out[-2000:]
    assert not set(os.listdir(tmp_path)) & {"g3_vpi.out", "g3ang_vpi.out"}
    for f in ("e_vpi.out", "et_vpi.out", "gr_vpi.out", "sk_vpi.out", "nr_vpi.out"):
        assert open(tmp_path / f, "rb").read() == open(os.path.join(gold, f), "rb").read(), f
