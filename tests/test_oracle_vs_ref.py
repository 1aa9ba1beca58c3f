"""The C restatement against the unmodified reference itself (oracle/_ref/libvpiref.so, built
from the reference's sources by oracle/Makefile) on fresh seeded inputs: bit-exact.  Where the
reference build is absent, its answers come from the recorded tapes (tests/reftape.py)."""
import numpy as np
import pytest

from helpers import same_bits
from oracle.pyoracle import System
from reftape import digest, rng_array


def _wrap(x, L):
    x = np.where(x > L / 2, x - L, x)
    return np.where(x < -L / 2, x + L, x)


@pytest.mark.parametrize("kw", [
    dict(dim=3, Np=64, Nb=40),
    dict(dim=3, Np=37, Nb=5),                       # ragged particle count
    dict(dim=2, Np=20, Nb=4, density=0.3),
    dict(dim=1, Np=5, Nb=3, density=0.4),
    dict(dim=3, Np=9, Nb=4, trap=True, a_ho=[0.9, 1.1, 1.4]),
    dict(dim=1, Np=2, Nb=10, trap=True, a_ho=[1.0]),
    # boxes with unequal sides (crystal = T, vpi.f90:99-122): the shortest side, which sets rcut, is not axis 0
    dict(dim=3, Np=37, Nb=5, Lbox=[7.3, 4.1, 5.9], density=37 / (7.3 * 4.1 * 5.9)),
    dict(dim=3, Np=24, Nb=4, Lbox=[2 * 1.6, 3 * 1.6, 4 * 1.6], density=24 / (24 * 1.6 ** 3)),
    dict(dim=2, Np=12, Nb=4, Lbox=[5.0, 8.0], density=12 / 40.0),
])
def test_hot_path_vs_reference(oracle, tape, kw):
    S = System(**kw)
    ref = tape.ref
    VT, WF = oracle.tables(S)
    if ref:
        VTr, WFr = ref.tables(S)
        ref.set_system(S)
    assert tape.digest(lambda: VTr) == digest(VT) and tape.digest(lambda: WFr) == digest(WF)
    seed = 4242 + S.Np
    P, _ = oracle.init_path(S, seed)
    assert tape.digest(lambda: ref.init(seed)[0]) == digest(P)
    rng = np.random.default_rng(S.Np * 1000 + S.dim)
    P = P + rng.normal(0, 0.3, P.shape)
    if not S.trap:
        P = _wrap(P, S.Lbox[:S.dim])
    for _ in range(300):
        ip = int(rng.integers(1, S.Np + 1))
        ib = int(rng.choice([0, 2 * S.Nb, int(rng.integers(0, S.M))]))
        xold = P[ib, ip - 1].copy()
        xnew = xold + rng.normal(0, 0.4, S.dim)
        if not S.trap:
            xnew = _wrap(xnew, S.Lbox[:S.dim])
        a = tape.scalars(lambda: ref.update_action(WF, VT, P, ip, ib, xnew, xold))[0]
        b = oracle.update_action(S, WF, VT, P, ip, ib, xnew, xold)
        assert same_bits([a], [b]), (ip, ib, a, b)
    for ib in range(S.M):
        for w in (False, True):
            assert same_bits(tape.scalars(lambda: ref.potential_energy(VT, P[ib], w)), oracle.potential_energy(S, VT, P[ib], w))
    for ib in (0, 2 * S.Nb):
        assert same_bits(tape.scalars(lambda: ref.local_energy(WF, VT, P[ib])), oracle.local_energy(S, WF, VT, P[ib]))
    assert same_bits(tape.scalars(lambda: ref.therm_energy(VT, P)), oracle.therm_energy(S, VT, P))


def _structural_estimators(oracle, tape, S):
    ref = tape.ref
    if ref:
        ref.set_system(S)
    P, _ = oracle.init_path(S, 11)
    assert tape.digest(lambda: ref.init(11)[0]) == digest(P)
    assert tape.digest(lambda: ref.pair_correlation(P[S.Nb])) == digest(oracle.pair_correlation(S, P[S.Nb]))
    assert tape.digest(lambda: ref.structure_factor(50, P[S.Nb])) == digest(oracle.structure_factor(S, 50, P[S.Nb]))
    rng = np.random.default_rng(5)
    for _ in range(50):
        xe = rng.uniform(-S.Lbox / 2, S.Lbox / 2, (2, 3))
        assert tape.digest(lambda: ref.obdm(xe)) == digest(oracle.obdm(S, xe))


def test_structural_estimators_vs_reference(oracle, tape):
    _structural_estimators(oracle, tape, System(dim=3, Np=64, Nb=4, Npw=2))


def test_structural_estimators_vs_reference_unequal_sides(oracle, tape):
    """g(r), S(k) (qbin per axis) and the OBDM in the box [7.3, 4.1, 5.9]: rbin and the cutoff come from axis 1."""
    S = System(dim=3, Np=37, Nb=4, Npw=2, Lbox=[7.3, 4.1, 5.9], density=37 / (7.3 * 4.1 * 5.9))
    assert S.rcut == 2.05
    _structural_estimators(oracle, tape, S)


def test_box_and_primitives_vs_reference(oracle, tape):
    ref = tape.ref
    for Np, dim, rho in ((64, 3, 0.365), (256, 3, 0.365), (20, 2, 0.3), (7, 1, 0.11)):
        L = tape.scalars(lambda: ref.box_length(Np, dim, rho))[0]
        assert L == oracle.L.po_box_length(Np, dim, rho)
        S = System(dim=dim, Np=Np, Nb=2, density=rho)
        assert S.Lbox[0] == L
    S = System(dim=3, Np=64, Nb=40)
    _minimum_image(oracle, tape, S)
    for opt in (0, 1):
        for ib in (0, 1, 2, 40, 79, 80):
            for pot, f2 in ((1.7, -3.3), (-2e5, 9e9)):
                assert tape.scalars(lambda: ref.green_function(opt, ib, 5e-3, pot, f2))[0] == \
                    oracle.green_function(opt, ib, S.Nb, 5e-3, pot, f2)


def _minimum_image(oracle, tape, S):
    ref = tape.ref
    if ref:
        ref.set_system(S)
    rng = np.random.default_rng(3)
    for _ in range(500):
        x = rng.uniform(-1.5 * S.Lbox, 1.5 * S.Lbox, 3)
        a = tape.scalars(lambda: np.append(*ref.minimum_image(x)))
        b, r2b = oracle.minimum_image(S, x)
        assert same_bits(a[:3], b) and a[3] == r2b


def test_minimum_image_vs_reference_unequal_sides(oracle, tape):
    """The single fold per axis with inputs from +-1.5 L_k of the box [7.3, 4.1, 5.9]: a fold by another axis' length shows."""
    _minimum_image(oracle, tape, System(dim=3, Np=37, Nb=4, Lbox=[7.3, 4.1, 5.9], density=37 / (7.3 * 4.1 * 5.9)))


def test_rng_vs_reference(oracle, tape):
    ref = tape.ref
    for seed in (1982, 1, 4357, 2**31 - 1):
        if ref:
            ref.sgrnd(seed)
        g = oracle.rng(seed)
        assert tape.digest(lambda: [ref.grnd() for _ in range(1500)]) == digest([oracle.grnd(g) for _ in range(1500)])
        assert tape.digest(lambda: [ref.rangauss(0.7, 0.1) for _ in range(200)]) == \
            digest([oracle.rangauss(g, 0.7, 0.1) for _ in range(200)])
        assert tape.digest(lambda: rng_array(*ref.rng_get_state())) == digest(rng_array(g.mti, np.array(g.mt[:], np.uint32)))
