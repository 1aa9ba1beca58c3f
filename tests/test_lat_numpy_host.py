"""Pins tests/lat_numpy.py, the restatement that tests/test_gpu_lat.py holds the device to, on the CPU: against a literal
triple loop and against configurations whose sums are known in closed form.  Also pins block_stats_numpy.norm_lat, the
independent statement of the family's normalisation, to figures divided by hand, and holds profiles.normalize_lat to it."""
import numpy as np
import pytest

import lat_numpy as ln
from pathintegralgroundstate_amd.profiles import nearest_neighbour_distance, normalize_lat

L3 = [6.0, 7.5, 9.0]


def _literal(X, R, Lbox, nbin, rmax, cm):
    """Scalar loops over particles, sites and axes."""
    Np, dim = X.shape
    site, U = [], []
    for i in range(Np):
        best, bs, bu = float("inf"), -1, [0.0] * dim
        for s in range(R.shape[0]):
            d, r2 = [], 0.0
            for k in range(dim):
                v = float(X[i, k]) - float(R[s, k])
                if v > 0.5 * Lbox[k]:
                    v = v - Lbox[k]
                if v < -0.5 * Lbox[k]:
                    v = v + Lbox[k]
                d.append(v)
                r2 = r2 + v * v
            if r2 < best:
                best, bs, bu = r2, s, d
        site.append(bs)
        U.append(bu)
    nass = sum(s >= 0 for s in site)
    c = [0.0] * dim
    if cm and nass:
        for k in range(dim):
            t = 0.0
            for i in range(Np):
                t = t + U[i][k]
            c[k] = t / float(nass)
    mom = [0.0] * (2 + dim)
    hr, hx, per = [0] * nbin, [[0] * (2 * nbin) for _ in range(dim)], [0] * R.shape[0]
    rbin = rmax / float(nbin)
    for i in range(Np):
        if site[i] < 0:
            continue
        per[site[i]] += 1
        v = [U[i][k] - c[k] for k in range(dim)] if cm else U[i]
        m2 = 0.0
        for k in range(dim):
            m2 = m2 + v[k] * v[k]
            mom[2 + k] += v[k] * v[k]
            t = (v[k] + rmax) / rbin
            if 0.0 <= t < 2.0 * nbin:
                hx[k][int(t)] += 1
        mom[0] += m2
        mom[1] += m2 * m2
        t = m2 ** 0.5 / rbin
        if t < float(nbin):
            hr[int(t)] += 1
    occ = [0, 0, 0, 0]
    for n in per:
        occ[min(n, 3)] += 1
    return site, mom, nass, occ, hr, hx


@pytest.mark.parametrize("cm", [0, 1])
@pytest.mark.parametrize("dim,dn", [(2, 0), (3, 1), (3, -1)])
def test_literal_loop(dim, dn, cm):
    Np = 11
    Lbox = L3[:dim]
    R = ln.grid_sites(dim, 3 if dim == 3 else 4, Lbox, Np + dn)
    X = ln.jittered(R, 1, 1, Np, Lbox, np.random.default_rng(dim + dn), 0.3)[0, 0]
    got = ln.slice_sums(X, R, Lbox, 6, 0.35, cm)
    site, mom, nass, occ, hr, hx = _literal(X, R, Lbox, 6, 0.35, cm)
    assert got["site"].tolist() == site and got["nassigned"] == nass and got["occ"].tolist() == occ
    assert got["hr"].tolist() == hr and got["hx"].tolist() == hx
    assert np.allclose(got["mom"], mom, rtol=1e-14, atol=0.0)


def _window(P, R, Lbox, nbin=8, rmax=1.0, cm=0, Nb=1, window=1):
    return ln.Window(P, Nb, window, Lbox, R, nbin, rmax, cm).expected(range(P.shape[0]))


def test_particles_on_the_sites():
    R = ln.grid_sites(3, 3, L3)
    P = np.broadcast_to(R, (2, 3, 27, 3)).copy()
    e = _window(P, R, L3, cm=1)
    assert not np.any(e["mom"]) and np.all(e["occ"] == [0, 27, 0, 0]) and not np.any(e["hop1"]) and not np.any(e["hopw"])
    assert np.all(e["hr"][:, 0] == 81) and np.all(e["hx"][:, :, 8] == 81) and e["samples"].tolist() == [1, 1]


def test_uniform_shift():
    R = ln.grid_sites(3, 3, L3)
    a = nearest_neighbour_distance(R, L3)
    assert a == pytest.approx(2.0)
    delta = np.array([0.3, -0.2, 0.4])
    assert np.linalg.norm(delta) < 0.5 * a
    P = np.broadcast_to(R + delta, (1, 3, 27, 3)).copy()
    e0, e1 = _window(P, R, L3, cm=0), _window(P, R, L3, cm=1)
    assert np.allclose(e0["mom"][0, :, 0], 27 * delta @ delta, rtol=1e-13)
    assert np.allclose(e0["mom"][0, :, 2:], 27 * delta * delta, rtol=1e-13)
    assert np.all(e1["mom"] <= 27 * 1e-30)
    n = normalize_lat(e0, 27, 27, a, 1.0)
    assert n["gamma"][0] == pytest.approx(np.linalg.norm(delta) / a) and n["alpha2"][0] == pytest.approx(3 / 5 - 1)
    assert n["vacant"][0] == 0 and n["multiple"][0] == 0 and n["hops_link"][0] == 0


def test_one_site_more_and_one_fewer():
    R = ln.grid_sites(3, 3, L3)
    P = np.broadcast_to(R[:26], (1, 3, 26, 3)).copy()
    e = _window(P, R, L3)
    assert np.all(e["occ"] == [1, 26, 0, 0])
    assert normalize_lat(e, 26, 27, 2.0, 1.0)["vacant"][0] == pytest.approx(1 / 27)
    X = np.concatenate([R[:26], R[:1] + 0.1])                          # 27 particles on 26 sites
    P = np.broadcast_to(X, (1, 3, 27, 3)).copy()
    e = _window(P, R[:26], L3)
    assert np.all(e["occ"] == [0, 25, 1, 0])
    assert normalize_lat(e, 27, 26, 2.0, 1.0)["multiple"][0] == pytest.approx(1 / 26)


def test_exchange_on_the_upper_half():
    R = ln.grid_sites(2, 4, L3[:2])
    Nb = 2
    P = np.broadcast_to(R, (1, 5, 16, 2)).copy()
    P[0, Nb + 1:, [0, 1]] = P[0, Nb + 1:, [1, 0]]
    e = _window(P, R, L3[:2], Nb=Nb, window=Nb)
    assert e["hop1"].tolist() == [2] and e["hopw"].tolist() == [2]
    n = normalize_lat(e, 16, 16, 1.5, 1.0)
    assert n["hops_link"][0] == pytest.approx(2 / (16 * 4)) and n["hops_window"][0] == pytest.approx(2 / 16)


def test_tie_takes_the_lower_index():
    R = np.array([[-1.0, 0.0], [1.0, 0.0], [0.0, 3.0]])
    site, u = ln.assign(np.array([[0.0, 0.0]]), R, [20.0, 20.0])
    assert site.tolist() == [0] and u.tolist() == [[1.0, 0.0]]
    site, _ = ln.assign(np.array([[0.0, 0.0]]), R[[1, 0, 2]], [20.0, 20.0])
    assert site.tolist() == [0]


def test_beyond_half_the_box_folds_once():
    Lbox = [10.0, 10.0]
    R = np.array([[4.5, 0.0], [0.0, 0.0]])
    site, u = ln.assign(np.array([[-4.75, 0.0]]), R, Lbox)              # d = -9.25 -> +0.75 round the box
    assert site.tolist() == [0] and u.tolist() == [[0.75, 0.0]]


def test_nan_coordinate_is_lost():
    R = ln.grid_sites(3, 3, L3)
    P = ln.jittered(R, 1, 3, 27, L3, np.random.default_rng(4), 0.2)
    clean = _window(P, R, L3)
    P[0, 1, 5, 2] = np.nan
    e = _window(P, R, L3)
    assert e["nlost"].tolist() == [1] and e["nassigned"].tolist() == [[27, 26, 27]]
    assert e["occ"][0].tolist() == [[0, 27, 0, 0], [1, 26, 0, 0], [0, 27, 0, 0]]
    assert np.array_equal(e["mom"][0, ::2], clean["mom"][0, ::2]) and np.all(np.isfinite(e["mom"]))
    assert e["hop1"].tolist() == [0] and e["hr"].sum() == clean["hr"].sum() - 1


def test_nearest_neighbour_distance_is_minimum_image():
    R = np.array([[-4.5, 0.0], [4.5, 0.0], [0.0, 3.0]])
    assert nearest_neighbour_distance(R, [10.0, 10.0]) == pytest.approx(1.0)
    assert nearest_neighbour_distance(R[:1], [10.0, 10.0]) == np.inf


def test_site_density_integrates_to_the_occupation():
    R = ln.grid_sites(3, 3, L3)
    P = ln.jittered(R, 2, 3, 27, L3, np.random.default_rng(8), 0.2)
    e = _window(P, R, L3, nbin=10, rmax=1.0, cm=1)
    n = normalize_lat(e, 27, 27, 2.0, 1.0)
    edges = np.arange(11) * 0.1
    shell = 4 * np.pi / 3 * np.diff(edges ** 3)
    assert np.allclose((n["rho_site"] * shell).sum(axis=-1), 1.0) and np.allclose(n["pu"].sum(axis=-1) * 0.1, 1.0)
    assert np.allclose(n["uk2"].sum(axis=-1), n["u2"]) and n["x"][0] == pytest.approx(-0.95) and n["r"][-1] == pytest.approx(0.95)


# ---- the independent normalisation, block_stats_numpy.norm_lat -----------------------------------------------------------
def _both(raw, Np, nsite, a_nn, rmax):
    """norm_lat and profiles.normalize_lat on the same sums."""
    import block_stats_numpy as bs
    with np.errstate(all="ignore"):
        return bs.norm_lat_raw(raw, Np, nsite, a_nn, rmax), normalize_lat(raw, Np, nsite, a_nn, rmax)


def test_norm_lat_one_slice_2d_by_hand():
    """One sample of one slice in 2D, four particles on five sites (two vacant, one doubly occupied), rmax = 2 in two bins:
    shell areas pi and 3 pi.  Every figure divides by hand; the site fractions divide by the SITES (2/5, 1/5), not by the
    particles (2/4, 1/4); one slice has no link."""
    raw = {"mom": np.array([[8.0, 32.0, 4.0, 4.0]]), "nassigned": np.array([4]), "nlost": 0, "occ": np.array([[2, 2, 1, 0]]),
           "hr": np.array([1, 3]), "hx": np.array([[4, 0, 0, 0], [0, 2, 1, 0]]), "hop1": 0, "hopw": 0, "samples": 1}
    for n in _both(raw, 4, 5, 2.0, 2.0):
        assert n["u2"].tolist() == [2.0] and n["uk2"].tolist() == [[1.0, 1.0]] and n["u2_mean"] == 2.0
        assert n["gamma_tau"].tolist() == [2.0 ** 0.5 / 2.0] and n["gamma"] == 2.0 ** 0.5 / 2.0
        assert n["alpha2"] == 2 * 8.0 / (4 * 4.0) - 1 == 0.0
        assert n["vacant"] == pytest.approx(0.4, rel=1e-15) and n["multiple"] == pytest.approx(0.2, rel=1e-15)
        assert n["hops_link"] == 0.0 and n["hops_window"] == 0.0
        assert np.allclose(n["rho_site"], [1 / (5 * np.pi), 3 / (5 * 3 * np.pi)], rtol=1e-15, atol=0)
        assert n["pu"].tolist() == [[1.0, 0.0, 0.0, 0.0], [0.0, 0.5, 0.25, 0.0]]


def test_norm_lat_three_slices_3d_by_hand():
    """Two samples of three slices in 3D, Np = 4 on nsite = 3, four particles lost on the last slice: the window's means
    weigh the slices by their assigned particles, the hops divide by the PARTICLES (8 / (2 4 2), not 8 / (2 3 2)), the
    shells are 4 pi / 3 (1, 7)."""
    raw = {"mom": np.array([[16.0, 40.0, 8.0, 4.0, 4.0], [8.0, 20.0, 4.0, 2.0, 2.0], [4.0, 10.0, 2.0, 1.0, 1.0]]),
           "nassigned": np.array([8, 8, 4]), "nlost": 4, "occ": np.array([[2, 3, 1, 0], [3, 2, 0, 1], [4, 1, 1, 0]]),
           "hr": np.array([18, 126]), "hx": np.array([[20, 0, 0, 0], [0, 10, 5, 0], [0, 0, 0, 40]]), "hop1": 8, "hopw": 2,
           "samples": 2}
    v = 4.0 * np.pi / 3.0
    for n in _both(raw, 4, 3, 0.5, 2.0):
        assert n["u2"].tolist() == [2.0, 1.0, 1.0] and n["uk2"].tolist() == [[1.0, 0.5, 0.5], [0.5, 0.25, 0.25], [0.5, 0.25, 0.25]]
        assert n["gamma_tau"].tolist() == [2.0 ** 0.5 / 0.5, 2.0, 2.0]
        assert n["u2_mean"] == pytest.approx(1.4, rel=1e-15) and n["gamma"] == pytest.approx(1.4 ** 0.5 / 0.5, rel=1e-15)
        assert n["alpha2"] == pytest.approx(3 * 3.5 / (5 * 1.96) - 1.0, rel=1e-14)
        assert n["vacant"] == 9.0 / 18.0 and n["multiple"] == pytest.approx(3.0 / 18.0, rel=1e-15)
        assert n["hops_link"] == 0.5 and n["hops_window"] == 0.25
        assert np.allclose(n["rho_site"], [18 / (18 * v), 126 / (18 * 7 * v)], rtol=1e-15, atol=0)
        assert n["pu"].tolist() == [[1.0, 0.0, 0.0, 0.0], [0.0, 0.5, 0.25, 0.0], [0.0, 0.0, 0.0, 2.0]]


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("ns", [1, 5])
def test_normalize_lat_equals_norm_lat_on_random_sums(dim, ns):
    """profiles.normalize_lat against the helper on random sums of [W, Nblock] walkers and blocks, nsite != Np, every output."""
    import block_stats_numpy as bs
    rng = np.random.default_rng(10 * dim + ns)
    lead, nbin, Np, nsite = (3, 4), 7, 11, 13
    raw = {"mom": rng.uniform(0.5, 9.0, lead + (ns, 2 + dim)), "nassigned": rng.integers(1, 60, lead + (ns,)),
           "nlost": rng.integers(0, 5, lead), "occ": rng.integers(0, 50, lead + (ns, 4)), "hr": rng.integers(0, 90, lead + (nbin,)),
           "hx": rng.integers(0, 90, lead + (dim, 2 * nbin)), "hop1": rng.integers(0, 30, lead), "hopw": rng.integers(0, 30, lead),
           "samples": rng.integers(1, 6, lead)}
    mine, theirs = _both(raw, Np, nsite, 1.7, 0.9)
    for k in bs.LAT_OUT:
        assert np.shape(theirs[k]) == mine[k].shape and np.all(np.isfinite(mine[k])), k
        assert np.allclose(theirs[k], mine[k], rtol=1e-13, atol=0), k
        assert np.any(mine[k] != 0) or (k == "hops_link" and ns == 1), k
    # one walker's slice of the dict, as the docstring of normalize_lat allows
    one = {k: v[1, 2] for k, v in raw.items()}
    mine1, theirs1 = _both(one, Np, nsite, 1.7, 0.9)
    for k in bs.LAT_OUT:
        assert np.allclose(theirs1[k], mine[k][1, 2], rtol=1e-13, atol=0) and np.array_equal(mine1[k], mine[k][1, 2]), k
