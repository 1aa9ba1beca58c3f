"""The magnitude form of the minimum image (pigs_device.h, min_image_mag) that even and end beads of K1 use:

    m = min(|v|, L - |v|)        r2 = m0*m0 + m1*m1 + m2*m2

m*m must equal, bit for bit, the square of the reference's two-compare fold (pbc_mod.f90:40-41) for every float64
input, and the rounding sequence of r2 must stay the reference's.  numpy float64 follows IEEE round-to-nearest like
the GPU's v_add_f64 / v_min_f64 / v_mul_f64 (numpy.minimum propagates NaN where v_min_f64 returns the other operand,
but both operands are NaN whenever one is).
"""
import numpy as np
import pytest

from helpers import same_bits

BOXES = [1.0, 3.5189, 9.283177667225558, 17.2, 0.1234567, 2.0 ** 40 / 3.0]


def fold_twice_compare(v, L):
    """pbc_mod.f90:40-41: if (v > L/2) v = v - L; if (v < -L/2) v = v + L."""
    h = 0.5 * L
    v = np.where(v > h, v - L, v)
    return np.where(v < -h, v + L, v)


def magnitude(v, L):
    a = np.abs(v)
    with np.errstate(invalid="ignore"):
        return np.minimum(a, L - a)


def rint_fold(v, L):
    """min_image_rn: the fold decided on RN(|v| * RN(1/L)), at most once."""
    t = np.clip(np.abs(v) * (1.0 / L), 0.0, 1.0)
    n = np.copysign(np.rint(t), v)
    return v - L * n                        # L*n is exact (n is 0 or +-1): one rounding, as the fma


def edges(L):
    h = 0.5 * L
    out = [0.0, -0.0, h, L, 1.5 * L, 2.0 * L, 3.0 * L, 5.25 * L, 1e-300, 5e-324, np.inf, -np.inf, np.nan]
    for c in (h, L, 1.5 * L, 2.0 * L):
        x = c
        for _ in range(6):
            x = np.nextafter(x, np.inf)
            out.append(x)
        x = c
        for _ in range(6):
            x = np.nextafter(x, 0.0)
            out.append(x)
    out = np.array(out, dtype=np.float64)
    return np.concatenate([out, -out])


@pytest.mark.parametrize("L", BOXES)
def test_square_of_the_magnitude_is_the_square_of_the_reference_fold(L):
    rng = np.random.default_rng(int(L * 1000) % 2 ** 32)
    v = np.concatenate([edges(L),
                        rng.uniform(-1.0, 1.0, 200000) * L,
                        rng.uniform(-6.0, 6.0, 200000) * L,
                        rng.normal(0.0, 1.0, 50000) * 1e6 * L,
                        0.5 * L * (1.0 + rng.integers(-64, 65, 20000) * np.finfo(float).eps)])
    with np.errstate(invalid="ignore", over="ignore"):
        ref = fold_twice_compare(v, L)
        m = magnitude(v, L)
        assert same_bits(m * m, ref * ref)
        # the magnitude itself: |m| is |fold| wherever the fold is defined
        fin = np.isfinite(v)
        assert same_bits(np.abs(m[fin]), np.abs(ref[fin]))


@pytest.mark.parametrize("L", BOXES)
def test_r2_keeps_the_reference_rounding_sequence(L):
    rng = np.random.default_rng(7)
    d = np.concatenate([rng.uniform(-3.0, 3.0, (100000, 3)) * L,
                        np.tile(edges(L)[:, None], (1, 3)) * np.array([1.0, -1.0, 1.0]),
                        rng.choice(edges(L), (20000, 3))])
    with np.errstate(invalid="ignore", over="ignore"):
        ref = fold_twice_compare(d, L)
        r2_ref = (0.0 + ref[:, 0] * ref[:, 0]) + ref[:, 1] * ref[:, 1]
        r2_ref = r2_ref + ref[:, 2] * ref[:, 2]
        m = magnitude(d, L)
        r2 = (0.0 + m[:, 0] * m[:, 0]) + m[:, 1] * m[:, 1]
        r2 = r2 + m[:, 2] * m[:, 2]
    assert same_bits(r2, r2_ref)


def test_the_rint_fold_differs_from_the_reference_only_next_to_half_the_box():
    """Why the magnitude form can move a result at all: min_image_rn (still used on odd beads and by K2) decides the fold
    on RN(|v| RN(1/L)) and so disagrees with the two compares within an ulp or so of L/2 -- and nowhere else."""
    for L in BOXES:
        rng = np.random.default_rng(3)
        h = 0.5 * L
        v = np.concatenate([edges(L), rng.uniform(-4.0, 4.0, 200000) * L,
                            h * (1.0 + rng.integers(-8, 9, 20000) * np.finfo(float).eps)])
        v = v[np.isfinite(v)]
        with np.errstate(invalid="ignore", over="ignore"):
            a = rint_fold(v, L)
            ref = fold_twice_compare(v, L)
        diff = (a * a) != (ref * ref)
        if diff.any():
            near = np.abs(np.abs(v[diff]) - h) <= 4.0 * np.spacing(h)
            assert near.all(), (L, v[diff][~near][:4])
