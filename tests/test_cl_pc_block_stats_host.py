"""block_stats_numpy.norm_cl / norm_pc, the restatement of what the front end makes of the cluster families' raw sums (no
GPU): against profiles.normalize_cl / normalize_pc on literal sums, and against hand-written values for a block without
finite clusters and for a block in which one walker counted nothing."""
import numpy as np

import block_stats_numpy as bs
from pathintegralgroundstate_amd import profiles

NP = 10


def _pc_sums():
    """test_pc_host.py's literal sums: two walkers, two slices each."""
    return {"nwrap": np.array([[3, 1, 0, 0, 0, 0, 0, 0], [4, 0, 1, 1, 0, 0, 0, 0]]),
            "mwrap": np.array([[4, 6, 0, 0, 0, 0, 0, 0], [6, 0, 7, 7, 0, 0, 0, 0]]),
            "swrap": np.array([[1, 1, 0, 0, 0, 0, 0, 0], [0, 0, 1, 1, 0, 0, 0, 0]]),
            "nfin": np.array([[2, 1] + [0] * 8, [2, 2] + [0] * 8]), "samples": np.array([2, 2]),
            "rg2u": np.array([[0, 0.5] + [0.0] * 8, [0, 3.0] + [0.0] * 8]),
            "first": np.array([[10, 5], [4, 0]]), "second": np.array([[10, 6], [4, 2]]), "both": np.array([[10, 1], [4, 0]]),
            "norig": np.array([[2, 1], [2, 1]])}


def _norm_pc(g, dim=2):
    return bs.norm_pc(g["nwrap"], g["mwrap"], g["swrap"], g["nfin"], g["rg2u"], g["first"], g["second"], g["both"], g["norig"],
                      g["samples"], NP, dim)


def test_norm_pc_against_profiles_and_by_hand():
    g = _pc_sums()
    v, p = _norm_pc(g), profiles.normalize_pc(g, NP, 2)
    assert np.array_equal(v["block"][:, :2], p["p_wrap"]) and not v["block"][:, 2].any()        # no z in 2D
    assert np.array_equal(v["block"][:, 3], p["p_any"]) and np.array_equal(v["block"][:, 4], p["p_all"])
    assert np.array_equal(v["block"][:, 5], p["p_inf"]) and np.array_equal(v["block"][:, 6], p["mean_size"])
    assert np.array_equal(v["nfin"], p["n_fin"])
    assert v["block"].tolist() == [[0.5, 0.0, 0.0, 0.5, 0.0, 0.3, 1.5], [0.5, 1.0, 0.0, 1.0, 0.5, 0.7, 10.0 / 6.0]]
    assert v["G"][:, 1].tolist() == [0.25, 1.5] and v["nfin"][0, :2].tolist() == [0.1, 0.05]
    assert v["pairs"][0].tolist() == [[5.0, 5.0, 5.0], [5.0, 6.0, 1.0]] and v["pairs"][1].tolist() == [[2.0, 2.0, 2.0], [0.0, 2.0, 0.0]]
    # <Rg^2>(s) of one block: G / (Np nfin) = rg2u / nfin, profiles' rg2
    with np.errstate(all="ignore"):
        assert np.array_equal(bs.ratio_of_means(v["G"], NP * v["nfin"])[:, 1], p["rg2"][:, 1])
    assert bs.ratio_of_means(v["pairs"][0, :, 2], v["pairs"][0, :, 0]).tolist() == p["persistence"][0].tolist()
    den = v["pairs"][..., 0] + v["pairs"][..., 1] - v["pairs"][..., 2]
    assert np.array_equal(bs.ratio_of_means(v["pairs"][..., 2], den), p["jaccard"])
    assert bs.ratio_of_means(v["pairs"][1, :, 2], v["pairs"][1, :, 0]).tolist() == [1.0, 0.0]   # 0 where profiles has NaN
    # in 3D the same sums: masks 1, 2, 3 wrap along x, y, both; none along z and none along all three
    assert _norm_pc(g, 3)["block"][1, :5].tolist() == [0.5, 1.0, 0.0, 1.0, 0.0]


def test_a_block_without_finite_clusters_has_mean_size_zero():
    """Every cluster wraps: profiles gives NaN, the front end's block value is 0 and enters the means as 0."""
    g = {k: v[:1].copy() for k, v in _pc_sums().items()}
    g["nfin"][:], g["rg2u"][:] = 0, 0.0
    g["nwrap"][0], g["mwrap"][0], g["swrap"][0] = [0, 2, 0, 0, 0, 0, 0, 0], [0, 20, 0, 0, 0, 0, 0, 0], [0, 2, 0, 0, 0, 0, 0, 0]
    v = _norm_pc(g)
    assert np.isnan(profiles.normalize_pc(g, NP, 2)["mean_size"][0])
    assert v["block"][0].tolist() == [1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.0] and not v["nfin"].any() and not v["G"].any()
    # two blocks of one walker, the second with finite pairs: the file's mean of the last column is (0 + 2) / 2
    b = np.stack([v["block"][0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0]])[None]
    m, e, n = bs.walker_stats(b, np.ones((1, 2), bool), 0)
    assert n == 2 and m[6] == 1.0 and e[6] == np.sqrt((2.0 - 1.0) / 2.0)


def _cl_sums():
    """Two walkers, Np = 10: walker 0 over 2 slices (sizes 1 1 1 2 5 and 1 2 2 5), walker 1 over 1 slice (10)."""
    nsize = np.zeros((2, NP), np.int64)
    nsize[0, [0, 1, 4]], nsize[1, 9] = [4, 3, 2], 1
    nlarge = np.zeros((2, NP), np.int64)
    nlarge[0, 4], nlarge[1, 9] = 2, 1
    rg2 = np.zeros((2, NP))
    rg2[0, [1, 4]], rg2[1, 9] = [0.75, 3.0], 7.0
    return {"nsize": nsize, "nlarge": nlarge, "nbond": np.array([14, 12]), "samples": np.array([2, 1]), "rg2": rg2}


def test_norm_cl_against_profiles_and_by_hand():
    g = _cl_sums()
    v = bs.norm_cl(g["nsize"], g["nlarge"], g["nbond"], g["rg2"], g["samples"], NP)
    p = profiles.normalize_cl(g, NP)
    for a, b in (("n", "n"), ("fraction", "fraction"), ("p_largest", "p_largest")):
        assert np.array_equal(v[a], p[b]), a
    want = np.stack([p["n_clusters"], p["smax"], p["mean_size"], p["bonds"]], axis=-1)
    assert np.array_equal(v["block"], want)
    assert v["block"].tolist() == [[4.5, 0.5, (4 + 12 + 50) / 20.0, 0.7], [1.0, 1.0, 10.0, 1.2]]
    assert v["n"][0, [0, 1, 4]].tolist() == [2.0, 1.5, 1.0] and v["G"][0, [1, 4]].tolist() == [0.375, 1.5] and v["G"][1, 9] == 7.0
    with np.errstate(all="ignore"):
        seen = g["nsize"] > 0
        assert np.array_equal(bs.ratio_of_means(v["G"], v["n"])[seen], p["rg2"][seen])


def test_a_block_that_one_walker_did_not_count():
    """Two walkers, two blocks; walker 1 has no sample in block 1.  Its 0 / 0 block values must not reach the averaged file:
    block 1 is walker 0's alone, block 0 the mean of both, and <Rg^2>(s) is the ratio of the two block means."""
    g = _cl_sums()
    blocks = []
    for b in range(2):
        S = g["samples"] if b == 0 else np.array([2, 0])
        z = (lambda a: a) if b == 0 else (lambda a: np.where(np.arange(2).reshape((2,) + (1,) * (a.ndim - 1)) == 1, 0, a))
        blocks.append(bs.norm_cl(z(g["nsize"]), z(g["nlarge"]), z(g["nbond"]), z(g["rg2"]), S, NP))
    counted = np.array([[True, True], [True, False]])
    n = np.stack([b["n"] for b in blocks], axis=1)                      # [W, Nblock, Np]
    G = np.stack([b["G"] for b in blocks], axis=1)
    assert np.all(np.isnan(n[1, 1]))                                    # 0 / 0: what the counted mask keeps out
    n[~counted], G[~counted] = 0.0, 0.0
    av, cb = bs.walker_average(n, counted)
    assert cb.tolist() == [True, True] and av[0, [0, 1, 4, 9]].tolist() == [1.0, 0.75, 0.5, 0.5] and av[1, [0, 1, 4, 9]].tolist() == [2.0, 1.5, 1.0, 0.0]
    mn, _, k = bs.average_stats(n, counted)
    mG, eG, _ = bs.average_stats(G, counted)
    assert k == 2 and mn[[4, 9]].tolist() == [0.75, 0.25] and mG[[4, 9]].tolist() == [1.125, 1.75]
    rg = bs.ratio_of_means(mG, mn)
    assert rg[4] == 1.5 and rg[9] == 7.0 and rg[2] == 0.0
    # the error of the numerator over <n(s)>: size 10 occurred in block 0 only, G = 3.5 and 0
    assert bs.ratio_of_means(eG, mn)[9] == np.sqrt((3.5 ** 2 / 2 - 1.75 ** 2) / 2) / 0.25
