"""F(q,tau) on the vector grid without a GPU: the normalisation (profiles.normalize_fqv), the numpy restatement
(tests/fqv_numpy.py) that the GPU tests compare against, and the front end on the CPU twin (the host built against
tests/shim, which does not provide pigs_fqv_*): it links, refuses the key, and runs unchanged without it."""
import os
import re
import subprocess

import numpy as np
import pytest

import fqt_numpy
import fqv_numpy
import sqv_numpy
from conftest import GOLDEN
from hostlib import build_cpu_host
from pathintegralgroundstate_amd.profiles import normalize_fqv, normalize_sqv, shell_average

RUNS = os.path.join(GOLDEN, "vpi_runs")
PBC = os.path.join(RUNS, "he4_cworm0", "vpi.in")                  # 2D, periodic
TRAP = os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")


def test_normalize_fqv_on_hand_made_sums():
    Np, window = 5, 2                                    # n_pairs = 5, 4, 3
    raw = np.zeros((3, 3, 2))
    raw[0] = [[50.0, 100.0], [40.0, 20.0], [30.0, -15.0]]
    raw[1] = 3.0 * raw[0]
    samples = np.array([1, 3, 0])                        # the last walker has no samples
    with np.errstate(all="raise"):                       # a walker without samples divides quietly
        F = normalize_fqv(raw, samples, Np, window)
    want = np.array([[2.0, 4.0], [2.0, 1.0], [2.0, -1.0]])
    assert F.shape == raw.shape
    assert np.array_equal(F[0], want) and np.array_equal(F[1], want) and np.all(np.isnan(F[2]))
    assert np.array_equal(normalize_fqv(raw[1], 3, Np, window), want)           # one walker, scalar samples
    assert np.array_equal(normalize_fqv(raw, samples, Np, window)[:2, 0], normalize_sqv(raw[:2, 0], samples[:2], Np, window))
    with pytest.raises(ValueError):
        normalize_fqv(np.zeros((1, 6, 2)), [1], Np, window)                     # 6 lags in a window of 5 slices
    # shell_average takes the leading axes as they are: (1,0) and (0,1) share a shell, (1,1) has its own
    n = np.array([[0, 1], [1, -1], [1, 0], [1, 1]])
    tab = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    q, mean, mult = shell_average(n, [2.0, 2.0], tab)
    assert mean.shape == (2, 3, 2) and mult.tolist() == [4, 4]
    assert np.array_equal(mean[..., 0], 0.5 * (tab[..., 0] + tab[..., 2]))
    assert np.array_equal(mean[..., 1], 0.5 * (tab[..., 1] + tab[..., 3]))


@pytest.mark.parametrize("dim,Np", [(1, 5), (2, 33), (3, 64)])
def test_restatement_on_axis_vectors_is_fqt_numpy(dim, Np):
    """fqv_numpy at the vectors (n,0,..), (0,n,..), .. against fqt_numpy, which states the axis grid on its own."""
    rng = np.random.default_rng(dim)
    Nb, window, Ntau, nmax = 5, 3, 6, 4
    L = np.array([7.0, 8.5, 6.25])[:dim]
    path = rng.uniform(-0.5, 0.5, (2 * Nb + 1, Np, dim)) * L
    n = fqv_numpy.vectors(dim, nmax)
    assert n.shape == (fqv_numpy.n_vectors(dim, nmax), dim) and np.array_equal(n, sqv_numpy.vectors(dim, nmax))
    acc, bound = fqv_numpy.fqv_sums(path, Nb, window, Ntau, n, L)
    assert acc.shape == bound.shape == (Ntau + 1, n.shape[0]) and np.all(bound > 0)
    axis, abound = fqt_numpy.fqt_sums(path, Nb, window, Ntau, nmax, L)
    for k in range(dim):
        for iq in range(1, nmax + 1):
            v = np.zeros(dim, np.int32)
            v[k] = iq
            hit = np.flatnonzero((n == v).all(axis=1))
            assert hit.size == 1
            want = axis[:, iq - 1, k]
            assert np.all(np.abs(acc[:, hit[0]] - want) <= 1e-12 * np.abs(want)), (k, iq)
            assert np.allclose(bound[:, hit[0]], abound[:, iq - 1, k], rtol=1e-9)
    # lag 0 is sqv_numpy's sum, and expected() counts a repeated walker twice
    s0 = sqv_numpy.sqv_sums(path, Nb, window, n, L)[0]
    assert np.allclose(acc[0], s0, rtol=1e-14, atol=0)
    F, B, cnt = fqv_numpy.expected(path[None], [0, 0], Nb, window, Ntau, n, L)
    assert cnt.tolist() == [2] and np.array_equal(F[0], acc + acc) and np.array_equal(B[0], bound + bound)
    assert fqv_numpy.n_pairs(window, Ntau).tolist() == [7, 6, 5, 4, 3, 2, 1]


# ---- the front end on the CPU twin -------------------------------------------------------------------------------------
def _key(extra=""):
    return f"&gpu\n fq_vector = T{extra}\n/\n"


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
    """The front end names no pigs_fqv_* symbol at link time: the shim does not define them and it still links."""
    assert os.path.exists(cpu_exe)
    nm = subprocess.run(["nm", "-u", cpu_exe], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
    assert b"pigs_ctx_create" in nm.stdout                     # nm lists the backend's symbols: the check has teeth
    assert b"pigs_fqv" not in nm.stdout
    assert b"fq_vector" in open(cpu_exe, "rb").read()           # the front end knows the key


def test_periodic_run_without_the_key_is_unchanged(cpu_exe, tmp_path):
    """Within this binary: a run without the key against one with the key spelled out as off."""
    txt = _short(open(PBC).read())
    rc, out = _run(cpu_exe, txt, str(tmp_path / "plain"))
    assert rc == 0, out[-2000:]
    assert "Vector F(q,tau)" not in out
    files = set(os.listdir(tmp_path / "plain"))
    assert {"e_vpi.out", "sk_vpi.out", "gr_vpi.out", "worldlines_final.bin"} <= files
    assert "fqvec_vpi.out" not in files and "fqsh_vpi.out" not in files
    rc, out2 = _run(cpu_exe, txt + "&gpu\n fq_vector = F, fqv_nmax = 4, fqv_ntau = 2, fqv_window = 1\n/\n", str(tmp_path / "off"))
    assert rc == 0, out2[-2000:]
    assert set(os.listdir(tmp_path / "off")) == files
    for f in files - {"vpi.in"}:
        assert open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "off" / f, "rb").read(), f
    strip = lambda s: [ln for ln in s.splitlines() if "Time per block" not in ln and "host threads" not in ln]
    assert strip(out) == strip(out2)


def test_key_is_refused_by_a_backend_without_the_entry_points(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(", fqv_nmax = 4, fqv_ntau = 2"), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "fq_vector" in out and "backend" in out and "pigs_fqv" in out, out
    assert not os.path.exists(tmp_path / "fqvec_vpi.out") and not os.path.exists(tmp_path / "e_vpi.out")


def test_key_is_refused_for_a_trapped_system(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, open(TRAP).read() + _key(), str(tmp_path))
    assert rc == 2
    assert "fq_vector" in out and "periodic" in out, out
    assert not os.path.exists(tmp_path / "e_vpi.out")


@pytest.mark.parametrize("extra,word", [(", fqv_nmax = 0", "fqv_nmax"),
                                        (", fqv_nmax = 65", "fqv_nmax"),          # the fixture is 2D: 64 is the limit
                                        (", fqv_ntau = -1", "fqv_ntau"),
                                        (", fqv_ntau = 3, fqv_window = 1", "fqv_ntau"),       # > 2 window
                                        (", fqv_window = 1000", "fqv_window"),                # > Nb
                                        (", fqv_ntau = 2001", "fqv_window")])     # the default window passes Nb
def test_out_of_range_keys_are_refused(cpu_exe, tmp_path, extra, word):
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(extra), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "fq_vector" in out and word in out and "pigs_fqv" not in out, out      # refused for the values, not the backend
    assert not os.path.exists(tmp_path / "e_vpi.out")


def test_nmax_limit_depends_on_the_dimension(cpu_exe, tmp_path):
    """3D stops at 16: 17 is refused for its value; 2D takes 64 (and is then refused for the backend)."""
    txt3 = _short(open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read())
    rc, out = _run(cpu_exe, txt3 + _key(", fqv_nmax = 17"), str(tmp_path / "a"))
    assert rc == 2 and "fqv_nmax" in out and "pigs_fqv" not in out, out
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(", fqv_nmax = 64"), str(tmp_path / "b"))
    assert rc == 2 and "pigs_fqv" in out, out
