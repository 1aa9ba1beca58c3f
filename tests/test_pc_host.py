"""The percolation key on a machine without a GPU: profiles.normalize_pc on literal sums, the ctypes signatures against the
header text, the Fortran normalisation and writers of the front end (pigs_estimators normalize_pc / write_perc_block /
write_percsz / write_clpers over block_series, through the host library's hook hs_pc_files) against profiles.normalize_pc,
and the front end's refusals on the CPU twin (the host built against tests/shim, which does not provide pigs_pc_*).

The files define their block errors as test_cl_host.py states them; <Rg^2>(s), C(l) and the Jaccard index are ratios of
block means."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from pathintegralgroundstate_amd import api, profiles
from test_cl_host import PERIODIC, PRINT, TRAP, _run, _short, block_error, cpu_exe, cpu_host  # noqa: F401 (fixtures)

KEY = "&gpu\n percolation = T\n/\n"
RAW = ("nwrap", "mwrap", "swrap", "nfin", "samples", "rg2u", "first", "second", "both", "norig")


def test_normalize_pc_on_literal_sums():
    Np = 10
    got = {"nwrap": np.array([[3, 1, 0, 0, 0, 0, 0, 0], [4, 0, 1, 1, 0, 0, 0, 0]]),
           "mwrap": np.array([[4, 6, 0, 0, 0, 0, 0, 0], [6, 0, 7, 7, 0, 0, 0, 0]]),
           "swrap": np.array([[1, 1, 0, 0, 0, 0, 0, 0], [0, 0, 1, 1, 0, 0, 0, 0]]),
           "nfin": np.array([[2, 1] + [0] * 8, [2, 2] + [0] * 8]), "samples": np.array([2, 2]),
           "rg2u": np.array([[0, 0.5] + [0.0] * 8, [0, 3.0] + [0.0] * 8]),
           "first": np.array([[10, 5], [4, 0]]), "second": np.array([[10, 6], [4, 2]]), "both": np.array([[10, 1], [4, 0]]),
           "norig": np.array([[2, 1], [2, 1]])}
    n = profiles.normalize_pc(got, Np, 2)
    assert n["p_wrap"].tolist() == [[0.5, 0.0], [0.5, 1.0]] and n["p_any"].tolist() == [0.5, 1.0] and n["p_all"].tolist() == [0.0, 0.5]
    assert n["p_inf"].tolist() == [6 / 20, 14 / 20] and n["n_fin"][0, :2].tolist() == [2 / 20, 1 / 20]
    assert n["mean_size"].tolist() == [(2 + 4) / (2 + 2), (2 + 8) / (2 + 4)]
    assert n["rg2"][0, 1] == 0.5 and n["rg2"][1, 1] == 1.5 and n["rg2"][0, 0] == 0 and np.isnan(n["rg2"][0, 2])
    assert n["persistence"][0].tolist() == [1.0, 0.2] and n["jaccard"][0].tolist() == [1.0, 0.1]
    assert n["persistence"][1, 0] == 1.0 and np.isnan(n["persistence"][1, 1]) and n["jaccard"][1, 1] == 0.0
    t = profiles.normalize_pc(got, Np, 2, summed=True)
    assert t["p_wrap"].tolist() == [0.5, 0.5] and t["p_inf"] == 20 / 40 and t["persistence"].tolist() == [1.0, 0.2]
    one = profiles.normalize_pc({k: v[1] for k, v in got.items()}, Np, 2)
    assert one["p_all"] == 0.5 and one["mean_size"] == n["mean_size"][1]
    empty = profiles.normalize_pc({k: np.zeros_like(v[0]) for k, v in got.items()}, Np, 2)
    assert np.isnan(empty["p_any"]) and np.isnan(empty["mean_size"]) and np.all(np.isnan(empty["jaccard"]))
    with pytest.raises(ValueError):
        profiles.normalize_pc(got, Np + 1, 2)
    with pytest.raises(ValueError):
        profiles.normalize_pc(got, Np, 4)


def test_ctypes_signatures_agree_with_the_header():
    """Every pigs_pc_* prototype of include/pigs_hip.h against the argtypes that api.load_library sets."""
    from pathintegralgroundstate_amd.build import build
    build()
    L = api.load_library()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pigs_hip.h")).read(), flags=re.S)
    protos = dict(re.findall(r"\bint\s+(pigs_pc_\w+)\s*\(([^)]*)\)\s*;", txt))
    assert sorted(protos) == ["pigs_pc_accumulate", "pigs_pc_init", "pigs_pc_np_max", "pigs_pc_read", "pigs_pc_sweeps"]
    ctype = {"pigs_ctx *": C.c_void_p, "double": C.c_double, "int32_t": C.c_int32, "int64_t *": C.POINTER(C.c_int64),
             "double *": C.POINTER(C.c_double), "const int32_t *": C.POINTER(C.c_int32), "int32_t *": C.POINTER(C.c_int32)}
    for name, args in protos.items():
        want = []
        for a in (x.strip() for x in args.split(",")):
            if a == "void":
                continue
            m = re.fullmatch(r"((?:const\s+)?\w+(?:\s*\*)?)\s*\w+", a)
            want.append(ctype[re.sub(r"\s*\*", " *", m.group(1))])
        assert list(getattr(L, name).argtypes) == want, name
        assert name in api.ABI_SYMBOLS
    assert L.pigs_pc_np_max() == api.CL_NP_MAX


def check_files(fb, fs, fp, raws, Np, dim, dt, block_ids=None):
    """perc_vpi.out, percsz_vpi.out and clpers_vpi.out of ONE walker against the raw block sums `raws` (pc_read dicts)."""
    nb = len(raws)
    norm = [profiles.normalize_pc(r, Np, dim) for r in raws]
    lines = open(fb).read().split("\n")
    assert lines[0].startswith("# block, wrapping probability along x, y, z")
    b = np.loadtxt(fb, ndmin=2)
    ids = block_ids if block_ids is not None else list(range(1, nb + 1))
    assert b.shape == (nb, 8) and b[:, 0].tolist() == [float(i) for i in ids]
    want = np.array([list(x["p_wrap"]) + [0.0] * (3 - dim) + [x["p_any"], x["p_all"], x["p_inf"],
                     0.0 if np.isnan(x["mean_size"]) else x["mean_size"]] for x in norm], dtype=float)
    assert np.allclose(b[:, 1:], want, rtol=PRINT, atol=0)
    S = np.array([float(r["samples"]) for r in raws])
    nfin = np.stack([r["nfin"] / (Np * s) for r, s in zip(raws, S)])
    G = np.stack([r["rg2u"] / s for r, s in zip(raws, S)])
    seen = np.nonzero(nfin.sum(axis=0) > 0)[0]
    t = np.loadtxt(fs, ndmin=2).reshape(-1, 5)                         # (a block series without a finite cluster: no line)
    assert t.shape == (seen.size, 5) and np.array_equal(t[:, 0], seen + 1.0)
    nm = nfin[:, seen].mean(axis=0)
    assert np.allclose(t[:, 1], nm, rtol=PRINT, atol=0)
    assert np.allclose(t[:, 2], block_error(nfin[:, seen]), rtol=1e-6, atol=1e-6 * np.abs(nfin).max())
    assert np.allclose(t[:, 3], G[:, seen].mean(axis=0) / (nm * Np), rtol=PRINT, atol=PRINT * np.abs(G).max())
    assert np.allclose(t[:, 4], block_error(G[:, seen]) / (nm * Np), rtol=1e-6, atol=1e-6 * max(np.abs(G).max(), 1e-300))
    per = np.stack([np.stack([r[k] / r["norig"] for k in ("first", "second", "both")], axis=1) for r in raws])   # [nb, nl, 3]
    p = np.loadtxt(fp, ndmin=2)
    nl = per.shape[1]
    assert p.shape == (nl, 10) and p[:, 0].tolist() == list(range(nl)) and np.allclose(p[:, 1], np.arange(nl) * dt, rtol=PRINT)
    m = per.mean(axis=0)
    for j in range(3):
        assert np.allclose(p[:, 2 + 2 * j], m[:, j], rtol=PRINT, atol=0), j
        assert np.allclose(p[:, 3 + 2 * j], block_error(per[:, :, j]), rtol=1e-6, atol=1e-6 * np.abs(per).max()), j
    with np.errstate(all="ignore"):
        assert np.allclose(p[:, 8], np.where(m[:, 0] > 0, m[:, 2] / m[:, 0], 0.0), rtol=PRINT, atol=0)
        den = m[:, 0] + m[:, 1] - m[:, 2]
        assert np.allclose(p[:, 9], np.where(den > 0, m[:, 2] / den, 0.0), rtol=PRINT, atol=0)


def test_fortran_normalisation_and_writers_match_the_package(cpu_host, tmp_path):
    """Three blocks of one walker from the restatement's sums of random slices near the threshold (wrapping and finite
    clusters, a size that occurs in one block only): the three files against profiles.normalize_pc of every block."""
    import cl_numpy as cn
    import pc_numpy as pn
    H = C.CDLL(cpu_host[1])
    lp, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    H.hs_pc_files.argtypes = [C.c_int] * 4 + [C.c_double] * 2 + [C.c_int] + [lp] * 5 + [dp] + [lp] * 4 + [C.c_char_p] * 3
    H.hs_pc_files.restype = None
    Np, nb, L, window, ntau, dt = 37, 3, [9.0, 7.0], 2, 3, 0.0125
    rc = 0.9 * cn.threshold_rc(2, Np / 63.0, L)
    P = cn.random_paths(nb, 5, Np, L, np.random.default_rng(37))
    raws = []
    for b in range(nb):
        e = pn.Window(P, 2, window, L, rc, ntau).expected([b] * (b + 1))    # 5, 10 and 15 slices
        raws.append({k: e[k][b] for k in RAW})
    S = np.array([r["samples"] for r in raws], np.int64)
    assert S.tolist() == [5, 10, 15]
    st = {k: np.ascontiguousarray(np.stack([r[k] for r in raws])) for k in RAW}
    assert st["swrap"][:, 1:].sum() > 0 and st["swrap"][:, 0].sum() > 0 and np.any((st["nfin"] > 0).sum(axis=0) == 1)
    f = [str(tmp_path / n).encode() for n in ("perc_vpi.out", "percsz_vpi.out", "clpers_vpi.out")]
    a = lambda k: st[k].ctypes.data_as(dp if k == "rg2u" else lp)
    H.hs_pc_files(Np, 2, window, ntau, rc, dt, nb, S.ctypes.data_as(lp), a("nwrap"), a("mwrap"), a("swrap"), a("nfin"), a("rg2u"),
                  a("first"), a("second"), a("both"), a("norig"), *f)
    check_files(*(x.decode() for x in f), raws, Np, 2, dt)


def test_key_is_refused_by_a_backend_without_the_entry_points(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, _short(open(PERIODIC).read()) + KEY, str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "percolation" in out and "backend" in out and all(s in out for s in ("pigs_pc_init", "_accumulate", "_read")), out
    assert not os.path.exists(tmp_path / "perc_vpi.out") and not os.path.exists(tmp_path / "e_vpi.out")


def test_key_is_refused_for_a_trapped_system(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, open(TRAP).read() + KEY, str(tmp_path))
    assert rc == 2
    assert "percolation" in out and "periodic" in out and "pigs_pc" not in out, out
    assert not os.path.exists(tmp_path / "e_vpi.out")


@pytest.mark.parametrize("keys,word", [("pc_rc = 1000.0", "pc_rc"), ("pc_window = 1000", "pc_window"),
                                       ("pc_window = 1, pc_ntau = 3", "pc_ntau"), ("pc_ntau = -1", "pc_ntau")])
def test_out_of_range_keys_are_refused_for_their_value(cpu_exe, tmp_path, keys, word):
    rc, out = _run(cpu_exe, _short(open(PERIODIC).read()) + f"&gpu\n percolation = T, {keys}\n/\n", str(tmp_path))
    assert rc == 2 and "percolation" in out and word in out and "pigs_pc" not in out, out[-2000:]
    assert not os.path.exists(tmp_path / "e_vpi.out")
