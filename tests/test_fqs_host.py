"""The self part of F(q,tau) and the imaginary-time displacement without a GPU: the normalisations
(profiles.normalize_fqs, profiles.normalize_msd) and the numpy restatement (tests/fqs_numpy.py) that the GPU tests compare
against, checked against closed forms; and the front end on the CPU twin (the host built against tests/shim, which does not
provide pigs_fqs_*): it links, refuses the key, and runs unchanged without it."""
import os
import re
import subprocess

import numpy as np
import pytest

import fqs_numpy
import fqv_numpy
from conftest import GOLDEN
from hostlib import build_cpu_host
from pathintegralgroundstate_amd.profiles import normalize_fqs, normalize_fqv, normalize_msd


def rigid_shift_path(M, base, delta, L):
    """path[M, Np, dim]: slice b is the lattice `base` shifted rigidly by b*delta and folded back into [-L/2, L/2)."""
    b = np.arange(M, dtype=np.float64)[:, None, None]
    return np.mod(base[None] + b * delta[None, None, :] + 0.5 * L, L) - 0.5 * L


def lattice(m, L):
    dim = L.size
    g = np.stack(np.meshgrid(*([np.arange(m)] * dim), indexing="ij"), axis=-1).reshape(-1, dim)
    return -0.5 * L + (g + 0.25) * (L / m)


def test_normalize_fqs_and_msd_on_hand_made_sums():
    Np, window, dim = 5, 2, 3                            # n_pairs = 5, 4, 3
    F = np.zeros((3, 3, 2))
    F[0] = [[25.0, 25.0], [20.0, 10.0], [15.0, -7.5]]
    F[1] = 3.0 * F[0]
    samples = np.array([1, 3, 0])                        # the last walker has no samples
    with np.errstate(all="raise"):
        Fs = normalize_fqs(F, samples, Np, window)
    want = np.array([[1.0, 1.0], [1.0, 0.5], [1.0, -0.5]])
    assert np.array_equal(Fs[0], want) and np.array_equal(Fs[1], want) and np.all(np.isnan(Fs[2]))
    assert np.array_equal(Fs[:2], normalize_fqv(F[:2], samples[:2], Np, window))
    # every one of the n_pairs * Np displacements has r2 = 2 l: msd = 2 l, <r^4> = 4 l^2, alpha2 = dim/(dim+2) - 1
    D = np.zeros((3, 3, 2))
    for l, npairs in enumerate((5, 4, 3)):
        D[0, l] = [npairs * Np * 2.0 * l, npairs * Np * 4.0 * l * l]
    D[1] = 3.0 * D[0]
    with np.errstate(all="raise"):
        msd, a2 = normalize_msd(D, samples, Np, window, dim)
    assert msd.shape == a2.shape == (3, 3)
    assert np.array_equal(msd[0], [0.0, 2.0, 4.0]) and np.array_equal(msd[1], msd[0]) and np.all(np.isnan(msd[2]))
    assert np.isnan(a2[0, 0]) and np.allclose(a2[:2, 1:], dim / (dim + 2.0) - 1.0, rtol=1e-15, atol=0)
    m1, b1 = normalize_msd(D[1], 3, Np, window, dim)                             # one walker, scalar samples
    assert np.array_equal(m1, msd[0]) and np.array_equal(b1[1:], a2[0, 1:])
    # a Gaussian displacement in `dim` dimensions has alpha2 = 0: <r^4> = (1 + 2/dim) <r^2>^2
    G = np.zeros((2, 2))
    G[1] = [4 * Np * 3.0, 4 * Np * (1.0 + 2.0 / dim) * 9.0]
    assert abs(normalize_msd(G, 1, Np, window, dim)[1][1]) < 1e-15
    with pytest.raises(ValueError):
        normalize_msd(np.zeros((1, 6, 2)), [1], Np, window, dim)                 # 6 lags in a window of 5 slices
    with pytest.raises(ValueError):
        normalize_msd(np.zeros((1, 3, 3)), [1], Np, window, dim)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_restatement_identical_slices(dim):
    """Every slice the same lattice: F = n_pairs * Np within the bound, D exactly 0.0."""
    Nb, window, Ntau, nmax, m = 4, 3, 5, 3, 3
    L = np.array([7.0, 8.5, 6.25])[:dim]
    base = lattice(m, L)
    Np = base.shape[0]
    path = np.broadcast_to(base, (2 * Nb + 1, Np, dim)).copy()
    n = fqs_numpy.vectors(dim, nmax)
    F, Fb, D, Db = fqs_numpy.fqs_sums(path, Nb, window, Ntau, n, L)
    npairs = fqs_numpy.n_pairs(window, Ntau)
    assert npairs.tolist() == [7, 6, 5, 4, 3, 2] and np.array_equal(npairs, fqv_numpy.n_pairs(window, Ntau))
    assert F.shape == Fb.shape == (Ntau + 1, n.shape[0]) and D.shape == Db.shape == (Ntau + 1, 2)
    assert np.array_equal(Fb, 1e-12 * (npairs * float(Np))[:, None] * np.ones_like(F))
    assert np.all(np.abs(F - (npairs * float(Np))[:, None]) <= Fb)
    assert not D.any() and not Db.any()
    assert np.allclose(normalize_fqs(F, 1, Np, window), 1.0, rtol=1e-12, atol=0)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_restatement_rigid_shift_with_wrap(dim):
    """Slice a+1 is slice a shifted by delta and folded back into the box, so that particles wrap inside the window:
    F_s(q, l) = Np n_pairs cos(l q.delta) and D[l][0] = n_pairs Np |l delta|^2, D[l][1] = n_pairs Np |l delta|^4."""
    Nb, window, Ntau, nmax, m = 5, 4, 4, 3, 3
    L = np.array([7.0, 8.5, 6.25])[:dim]
    delta = np.array([0.61, -0.43, 0.37])[:dim]
    assert np.all(np.abs(Ntau * delta) < 0.5 * L - 1e-6 * L)             # |l delta_k| < L/2, and not near it
    base = lattice(m, L)
    Np = base.shape[0]
    path = rigid_shift_path(2 * Nb + 1, base, delta, L)
    win = path[Nb - window:Nb + window + 1]
    assert np.any(np.abs(np.diff(win, axis=0)) > 0.5 * L)                # some particle wraps inside the window
    n = fqs_numpy.vectors(dim, nmax)
    F, Fb, D, Db = fqs_numpy.fqs_sums(path, Nb, window, Ntau, n, L)
    npairs = fqs_numpy.n_pairs(window, Ntau).astype(np.float64)
    l = np.arange(Ntau + 1, dtype=np.float64)
    qd = (n * (2.0 * np.pi / L)) @ delta                                 # [Nq]
    assert np.all(np.abs(F - Np * npairs[:, None] * np.cos(l[:, None] * qd[None, :])) <= Fb)
    r2 = l * l * (delta @ delta)
    assert np.all(np.abs(D[:, 0] - npairs * Np * r2) <= 1e-12 * npairs * Np * r2)
    assert np.all(np.abs(D[:, 1] - npairs * Np * r2 * r2) <= 1e-12 * npairs * Np * r2 * r2)
    assert D[0, 0] == 0.0 and D[0, 1] == 0.0
    msd, a2 = normalize_msd(D, 1, Np, window, dim)
    assert np.allclose(msd, r2, rtol=1e-12, atol=0)
    assert np.allclose(a2[1:], dim / (dim + 2.0) - 1.0, rtol=1e-11, atol=0)      # one sharp |dr|: <r^4> = <r^2>^2


def test_restatement_sum_rule_and_repeats():
    """Random worldlines: F_s(q, 0) = 1 and <dr^2>(0) = 0; expected() counts a repeated walker twice; the lag-0 row of
    the self part summed with the distinct part is the coherent F of fqv_numpy at lag 0 for Np = 1 per slice pair."""
    rng = np.random.default_rng(3)
    Nb, window, Ntau, nmax, Np, dim = 4, 2, 3, 2, 7, 3
    L = np.array([7.0, 8.5, 6.25])
    paths = rng.uniform(-0.5, 0.5, (2, 2 * Nb + 1, Np, dim)) * L
    n = fqs_numpy.vectors(dim, nmax)
    F, Fb, D, Db = fqs_numpy.fqs_sums(paths[0], Nb, window, Ntau, n, L)
    assert np.all(np.abs(F[0] - (2 * window + 1) * Np) <= Fb[0]) and D[0, 0] == 0.0 and D[0, 1] == 0.0
    assert np.all(D[1:] > 0) and np.all(np.abs(F) <= (fqs_numpy.n_pairs(window, Ntau) * Np)[:, None] * (1 + 1e-12))
    e = fqs_numpy.expected(paths, [1, 0, 1], Nb, window, Ntau, n, L)
    assert e["samples"].tolist() == [1, 2]
    assert np.array_equal(e["F"][0], F) and np.array_equal(e["D"][0], D) and np.array_equal(e["Fb"][0], Fb)
    one = fqs_numpy.fqs_sums(paths[1], Nb, window, Ntau, n, L)
    assert np.array_equal(e["F"][1], one[0] + one[0]) and np.array_equal(e["Db"][1], one[3] + one[3])
    # one particle: the self part IS the coherent F(q,tau)
    solo = paths[0][:, :1]
    Fs = fqs_numpy.fqs_sums(solo, Nb, window, Ntau, n, L)[0]
    Fc = fqv_numpy.fqv_sums(solo, Nb, window, Ntau, n, L)[0]
    assert np.all(np.abs(Fs - Fc) <= 1e-12 * fqs_numpy.n_pairs(window, Ntau)[:, None])


# ---- the front end on the CPU twin -------------------------------------------------------------------------------------
RUNS = os.path.join(GOLDEN, "vpi_runs")
PBC = os.path.join(RUNS, "he4_cworm0", "vpi.in")                  # 2D, periodic
TRAP = os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")


def _key(extra=""):
    return f"&gpu\n fq_self = T{extra}\n/\n"


@pytest.fixture(scope="module")
def cpu_exe():
    _, _, exe = build_cpu_host()
    return exe


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


def test_cpu_twin_still_links_against_the_unchanged_shim(cpu_exe):
    """The front end names no pigs_fqs_* symbol at link time: the shim does not define them and it still links."""
    assert os.path.exists(cpu_exe)
    nm = subprocess.run(["nm", "-u", cpu_exe], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
    assert b"pigs_ctx_create" in nm.stdout                     # nm lists the backend's symbols: the check has teeth
    assert b"pigs_fqs" not in nm.stdout
    assert b"fq_self" in open(cpu_exe, "rb").read()             # the front end knows the key


def test_periodic_run_without_the_key_is_unchanged(cpu_exe, tmp_path):
    """Within this binary: a run without the key against one with the key spelled out as off."""
    txt = _short(open(PBC).read())
    rc, out = _run(cpu_exe, txt, str(tmp_path / "plain"))
    assert rc == 0, out[-2000:]
    assert "Self F_s(q,tau)" not in out
    files = set(os.listdir(tmp_path / "plain"))
    assert {"e_vpi.out", "sk_vpi.out", "gr_vpi.out", "worldlines_final.bin"} <= files
    assert not {"fqself_vpi.out", "fqssh_vpi.out", "msd_vpi.out"} & files
    rc, out2 = _run(cpu_exe, txt + "&gpu\n fq_self = F, fqs_nmax = 4, fqs_ntau = 2, fqs_window = 1\n/\n", str(tmp_path / "off"))
    assert rc == 0, out2[-2000:]
    assert set(os.listdir(tmp_path / "off")) == files
    for f in files - {"vpi.in"}:
        assert open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "off" / f, "rb").read(), f
    strip = lambda s: [ln for ln in s.splitlines() if "Time per block" not in ln and "host threads" not in ln]
    assert strip(out) == strip(out2)


def test_key_is_refused_by_a_backend_without_the_entry_points(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(", fqs_nmax = 4, fqs_ntau = 2"), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "fq_self" in out and "backend" in out and "pigs_fqs" in out, out
    assert not os.path.exists(tmp_path / "fqself_vpi.out") and not os.path.exists(tmp_path / "e_vpi.out")


def test_key_is_refused_for_a_trapped_system(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, open(TRAP).read() + _key(), str(tmp_path))
    assert rc == 2
    assert "fq_self" in out and "periodic" in out, out
    assert not os.path.exists(tmp_path / "e_vpi.out")


@pytest.mark.parametrize("extra,word", [(", fqs_nmax = 0", "fqs_nmax"),
                                        (", fqs_nmax = 65", "fqs_nmax"),          # the fixture is 2D: 64 is the limit
                                        (", fqs_ntau = -1", "fqs_ntau"),
                                        (", fqs_ntau = 3, fqs_window = 1", "fqs_ntau"),       # > 2 window
                                        (", fqs_window = 1000", "fqs_window"),                # > Nb
                                        (", fqs_ntau = 2001", "fqs_window")])     # the default window passes Nb
def test_out_of_range_keys_are_refused(cpu_exe, tmp_path, extra, word):
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(extra), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "fq_self" in out and word in out and "pigs_fqs" not in out, out        # refused for the values, not the backend
    assert not os.path.exists(tmp_path / "e_vpi.out")
