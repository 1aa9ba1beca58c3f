"""The numpy restatement of the pigs_sf_* sums (tests/sf_numpy.py) and the caller's divisions (profiles.normalize_sf,
profiles.superfluid_fraction), pinned on the CPU: against a literal scalar loop that walks the kernel's order lane by
lane, against closed forms on a dyadic grid where every operation is exact, against figures divided by hand, and against
the free gas, whose superfluid fraction is 1."""
import math

import numpy as np
import pytest

import sf_numpy as sn
from helpers import same_bits
from pathintegralgroundstate_amd.profiles import normalize_sf, superfluid_fraction


# ---- 1. the literal loop ------------------------------------------------------------------------------------------------
def _wave_sum(v):
    """The butterfly of one wave of 64 lanes, every lane's value."""
    v = list(v)
    m = 32
    while m >= 1:
        v = [v[j] + v[j ^ m] for j in range(64)]
        m //= 2
    return v


def _block_sum(lanes):
    """256 lanes -> the butterfly of every wave, then the waves in wave order from 0.0."""
    tot = 0.0
    for g in range(4):
        tot = tot + _wave_sum(lanes[64 * g:64 * g + 64])[0]
    return tot


def literal(X, Lbox, Ntau):
    """One walker's window X [ns, Np, dim] in plain Python floats, in the order of pigs_hip.h."""
    ns, Np, dim = X.shape
    X = X.tolist()
    L = [float(v) for v in Lbox]
    U = [[[0.0] * dim for _ in range(Np)] for _ in range(ns)]
    W = [[0.0] * dim for _ in range(ns)]
    nwrap = 0
    for a in range(ns - 1):
        lanes = [[0.0] * 256 for _ in range(dim)]
        for i in range(Np):
            for k in range(dim):
                d = X[a + 1][i][k] - X[a][i][k]
                if d > 0.5 * L[k] or d < -0.5 * L[k]:
                    nwrap += 1
                if d > 0.5 * L[k]:
                    d = d - L[k]
                if d < -0.5 * L[k]:
                    d = d + L[k]
                U[a + 1][i][k] = U[a][i][k] + d
                lanes[k][i % 256] = lanes[k][i % 256] + d
        for k in range(dim):
            W[a + 1][k] = W[a][k] + _block_sum(lanes[k])
    C = np.zeros((Ntau + 1, dim))
    D = np.zeros((Ntau + 1, dim))
    for l in range(Ntau + 1):
        for k in range(dim):
            c = 0.0
            for a in range(ns - l):
                t = W[a + l][k] - W[a][k]
                c = c + t * t
            C[l, k] = c
            lanes = [0.0] * 256
            for i in range(Np):
                for a in range(ns - l):
                    t = U[a + l][i][k] - U[a][i][k]
                    lanes[i % 256] = lanes[i % 256] + t * t
            D[l, k] = _block_sum(lanes)
    return C, D, nwrap


@pytest.mark.parametrize("Np", [3, 64, 65, 257, 300])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_restatement_against_the_literal_loop(dim, Np):
    Lbox = [5.0, 8.0, 6.5][:dim]
    Nb, window, Ntau = 2, 2, 3
    P = sn.random_walk(1, 2 * Nb + 1, Np, Lbox, np.random.default_rng(10 * Np + dim), 0.05)
    w = sn.Window(P, Nb, window, Lbox, Ntau)
    C, D, nwrap = literal(P[0], Lbox, Ntau)
    assert nwrap > 0 or Np == 3
    assert w.nwrap[0] == nwrap
    assert same_bits(w.C[0], C) and same_bits(w.D[0], D)
    assert not np.any(C[0]) and not np.any(D[0]) and np.all(D[1:] > 0)


def test_wraps_are_counted_in_the_smallest_case():
    P = sn.random_walk(1, 5, 3, [5.0, 8.0], np.random.default_rng(4), 0.2)
    w = sn.Window(P, 2, 2, [5.0, 8.0], 2)
    assert w.nwrap[0] == literal(P[0], [5.0, 8.0], 2)[2] > 0


def test_lane_sum_is_not_a_plain_sum():
    """The order matters: on numbers of mixed size the butterfly differs from the sequential sum in the last bits."""
    x = np.random.default_rng(1).normal(0, 1, 300) * 10.0 ** np.random.default_rng(2).integers(-6, 6, 300)
    lanes = [0.0] * 256
    for i, v in enumerate(x.tolist()):
        lanes[i % 256] = lanes[i % 256] + v
    assert sn.lane_sum(x) == _block_sum(lanes)
    assert sn.lane_sum(x) != float(np.cumsum(x)[-1])


# ---- 2. closed forms on a dyadic grid -----------------------------------------------------------------------------------
@pytest.mark.parametrize("Np", [4, 66, 300])
def test_rigid_translation_and_counter_flow(Np):
    Lbox, c = [8.0, 16.0, 4.0], [0.375, -1.25, 1.0 / 64]
    Nb, Ntau = 4, 8
    ns = 2 * Nb + 1
    lags = np.arange(Ntau + 1.0)
    npairs = ns - lags
    rigid = sn.Window(sn.drift(Np, ns, Lbox, c, np.ones(Np), np.random.default_rng(Np)), Nb, Nb, Lbox, Ntau)
    assert rigid.nwrap[0] > 0
    wantC = npairs[:, None] * (Np * lags[:, None] * np.asarray(c)) ** 2
    wantD = Np * npairs[:, None] * (lags[:, None] * np.asarray(c)) ** 2
    assert same_bits(rigid.C[0], wantC) and same_bits(rigid.D[0], wantD)
    sign = np.where(np.arange(Np) % 2 == 0, 1.0, -1.0)
    counter = sn.Window(sn.drift(Np, ns, Lbox, c, sign, np.random.default_rng(Np)), Nb, Nb, Lbox, Ntau)
    assert same_bits(counter.C[0], np.zeros_like(wantC)) and same_bits(counter.D[0], wantD)


def test_expected_counts_a_walker_per_listing():
    P = sn.random_walk(3, 5, 7, [5.0, 8.0], np.random.default_rng(0), 0.05)
    w = sn.Window(P, 2, 1, [5.0, 8.0], 2)
    e = w.expected([2, 0, 2])
    assert e["samples"].tolist() == [1, 0, 2] and e["nwrap"].tolist() == [w.nwrap[0], 0, 2 * w.nwrap[2]]
    assert same_bits(e["C"][2], 2 * w.C[2]) and same_bits(e["D"][0], w.D[0]) and not np.any(e["C"][1])


# ---- 3. the caller's divisions ------------------------------------------------------------------------------------------
def test_normalize_sf_by_hand():
    """window 1 (ns = 3, n_pairs 3, 2, 1), Np 4, dt 0.25, two samples."""
    got = {"C": np.array([[0.0, 0.0], [48.0, 96.0], [64.0, 16.0]]), "D": np.array([[0.0, 0.0], [24.0, 48.0], [8.0, 32.0]]),
           "nwrap": np.int64(5), "samples": np.int64(2), "window": 1}
    n = normalize_sf(got, 4, 0.25)
    assert n["tau"].tolist() == [0.0, 0.25, 0.5]
    assert n["Dcm"].tolist() == [[0.0, 0.0], [3.0, 6.0], [8.0, 2.0]]          # /(2*3*4), /(2*2*4), /(2*1*4)
    assert n["msd"].tolist() == [[0.0, 0.0], [1.5, 3.0], [1.0, 4.0]]
    assert n["cross"].tolist() == [[0.0, 0.0], [1.5, 3.0], [7.0, -2.0]]
    assert np.all(np.isnan(n["rhos"][0])) and n["rhos"][1:].tolist() == [[12.0, 24.0], [16.0, 4.0]]    # lam 1/2: Dcm / tau
    assert math.isnan(n["rhos_mean"][0]) and n["rhos_mean"][1:].tolist() == [18.0, 10.0]
    assert normalize_sf(got, 4, 0.25, lam=2.0)["rhos"][1:].tolist() == [[3.0, 6.0], [4.0, 1.0]]
    many = {"C": np.stack([got["C"], 0 * got["C"]]), "D": np.stack([got["D"], 0 * got["D"]]), "samples": np.array([2, 0])}
    m = normalize_sf(many, 4, 0.25, window=1)
    assert m["Dcm"].shape == (2, 3, 2) and same_bits(m["Dcm"][0], n["Dcm"]) and same_bits(m["cross"][0], n["cross"])
    assert all(np.all(np.isnan(m[k][1])) for k in ("Dcm", "msd", "rhos", "cross", "rhos_mean"))   # a walker without samples
    with pytest.raises(ValueError):
        normalize_sf(many, 4, 0.25)                                          # no window
    with pytest.raises(ValueError):
        normalize_sf(got, 4, 0.25, window=0)                                 # three lags in one slice


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_block_stats_norm_sf_equals_normalize_sf(dim):
    """block_stats_numpy.norm_sf, which the front-end tests take their expected block values from, against
    profiles.normalize_sf: random positive sums of two walkers x three blocks, one of them without a sample; then the
    figures of test_normalize_sf_by_hand, divided there by hand."""
    import block_stats_numpy as bs
    rng = np.random.default_rng(40 + dim)
    window, Ntau, Np, dt = 3, 5, 37, 0.0125
    S = np.array([[4, 0, 7], [1, 3, 2]], np.int64)
    lag = np.arange(Ntau + 1.0)[:, None]
    Cs = rng.uniform(0.5, 2.0, (2, 3, Ntau + 1, dim)) * lag * np.maximum(S, 1)[..., None, None] * Np
    Ds = rng.uniform(0.5, 2.0, (2, 3, Ntau + 1, dim)) * lag * np.maximum(S, 1)[..., None, None] * Np
    Cs[0, 1], Ds[0, 1] = 0.0, 0.0                                          # what a read leaves of a block without a sample
    mine = bs.norm_sf(Cs, Ds, S, window, Np, dt)
    want = normalize_sf({"C": Cs, "D": Ds, "samples": S, "window": window}, Np, dt)
    assert sorted(mine) == sorted(k for k in want if k != "tau")
    for k, v in mine.items():
        assert v.shape == want[k].shape and np.array_equal(np.isnan(v), np.isnan(want[k])), k
        assert np.allclose(v, want[k], rtol=1e-14, atol=0, equal_nan=True), k
        assert np.all(np.isnan(v[0, 1])), k                                # the block without a sample
        fin = v[S > 0]
        assert np.all(np.isfinite(fin[:, 1:])) and (np.all(np.isnan(fin[:, 0])) if k.startswith("rhos") else not np.any(fin[:, 0])), k
    assert np.all(mine["Dcm"][S > 0][:, 1:] > 0) and np.all(mine["rhos"][S > 0][:, 1:] > 0)
    for k, v in bs.norm_sf(Cs, Ds, S, window, Np, dt, lam=2.0).items():
        assert np.allclose(v, normalize_sf({"C": Cs, "D": Ds, "samples": S, "window": window}, Np, dt, lam=2.0)[k],
                           rtol=1e-14, atol=0, equal_nan=True), k
    if dim == 2:
        n = bs.norm_sf([[0.0, 0.0], [48.0, 96.0], [64.0, 16.0]], [[0.0, 0.0], [24.0, 48.0], [8.0, 32.0]], 2, 1, 4, 0.25)
        assert n["Dcm"].tolist() == [[0.0, 0.0], [3.0, 6.0], [8.0, 2.0]] and n["msd"].tolist() == [[0.0, 0.0], [1.5, 3.0], [1.0, 4.0]]
        assert n["cross"].tolist() == [[0.0, 0.0], [1.5, 3.0], [7.0, -2.0]] and n["rhos"][1:].tolist() == [[12.0, 24.0], [16.0, 4.0]]
        assert n["rhos_mean"][1:].tolist() == [18.0, 10.0] and np.all(np.isnan(n["rhos"][0])) and math.isnan(n["rhos_mean"][0])


def test_superfluid_fraction_on_a_straight_line():
    tau = 0.125 * np.arange(9)
    y = 0.75 * tau + 0.5
    y[:3] = [0.0, 0.4, 0.6]                                                   # the short lags are off the line
    rho, err = superfluid_fraction(tau, y, 0.375)
    assert rho == 0.75 and err == 0.0
    assert superfluid_fraction(tau, y, 0.375, lam=1.5)[0] == 0.25
    rho2, err2 = superfluid_fraction(tau, y, 7 * 0.125)
    assert rho2 == 0.75 and math.isnan(err2)
    with pytest.raises(ValueError):
        superfluid_fraction(tau, y, 1.0)
    bent, e = superfluid_fraction(tau, y, 0.0)
    assert bent != 0.75 and e > 0


# ---- 4. the free gas ------------------------------------------------------------------------------------------------------
def test_free_gaussian_walks_flow_entirely():
    """Free particles: every link is N(0, dt) per axis (lam = 1/2), so Dcm = tau and rhos = 1 at every lag.  The squares
    (W_k(a+l) - W_k(a))^2 / (Np l dt) are chi^2 of one degree, variance 2.  The pairs of a lag overlap; the mean over
    them is a weighted mean of l means over NON-overlapping pairs (offsets 0 .. l-1), each of at least
    floor((ns - l) / l) independent squares per walker, and the variance of a weighted mean of estimators does not pass
    the largest of theirs: the standard error is at most sqrt(2 / M), M = walkers * floor((ns - l) / l)."""
    nW, Np, Nb, dim, dt, Ntau = 24, 16, 40, 3, 0.01, 6
    Lbox = [3.0, 4.0, 5.0]
    ns = 2 * Nb + 1
    rng = np.random.default_rng(1995)
    L = np.asarray(Lbox)
    P = rng.uniform(-0.5, 0.5, (nW, 1, Np, dim)) * L + np.cumsum(rng.normal(0.0, math.sqrt(dt), (nW, ns, Np, dim)), axis=1)
    P = P - L * np.floor((P + 0.5 * L) / L)
    w = sn.Window(P, Nb, Nb, Lbox, Ntau)
    assert sum(w.nwrap) > 0
    got = w.expected(range(nW))
    got["window"] = Nb
    pooled = {"C": got["C"].sum(axis=0), "D": got["D"].sum(axis=0), "samples": got["samples"].sum(), "window": Nb}
    n = normalize_sf(pooled, Np, dt)
    for l in range(1, Ntau + 1):
        se = math.sqrt(2.0 / (nW * ((ns - l) // l)))
        for k in range(dim):
            print(f"lag {l} axis {k}: rhos = {n['rhos'][l, k]:.4f}, (rhos - 1) / se = {(n['rhos'][l, k] - 1.0) / se:+.2f}")
            assert abs(n["rhos"][l, k] - 1.0) <= 5.0 * se
        # the single-particle displacement diffuses alike, with Np times the squares, and the cross term is their difference
        assert abs(n["msd"][l].mean() / (l * dt) - 1.0) <= 5.0 * math.sqrt(2.0 / (nW * Np * dim * ((ns - l) // l)))
