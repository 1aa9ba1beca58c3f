"""The |q| shells of the stored vectors off the cubic branch: host/pigs_estimators.f90 sqv_shells (what the front end
writes sq_vpi.out, fqsh_vpi.out and fqssh_vpi.out from, through its C-callable handle est_sqv_shells) against
pathintegralgroundstate_amd.profiles.shell_average -- two statements of one rule, "vectors whose |q|^2 agree to 1e-12
relative share a shell", that only a box with unequal sides reaches.  Shell of every vector, shell count, multiplicities
and |q| (to the rounding of the shell's sum) must all match.  No GPU: the host library linked against tests/shim."""
import ctypes as C

import numpy as np
import pytest

from hostlib import build_cpu_host
from pathintegralgroundstate_amd.profiles import shell_average
from sqv_numpy import vectors


@pytest.fixture(scope="module")
def host():
    shim, lib, _ = build_cpu_host()
    C.CDLL(shim, mode=C.RTLD_GLOBAL)
    H = C.CDLL(lib)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    H.est_sqv_shells.argtypes = [C.c_int, dp, C.c_int, ip, ip, ip, dp, ip]
    H.est_sqv_shells.restype = None
    return H


def fortran_shells(H, n, Lbox):
    n = np.ascontiguousarray(n, np.int32)                    # [Nq, dim] C order == nv(dim, Nq)
    Nq, dim = n.shape
    L = np.ascontiguousarray(Lbox[:dim], float)
    shell, mult, q = np.zeros(Nq, np.int32), np.zeros(Nq, np.int32), np.zeros(Nq)
    nsh = C.c_int32()
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    H.est_sqv_shells(dim, L.ctypes.data_as(dp), Nq, n.ctypes.data_as(ip), shell.ctypes.data_as(ip), C.byref(nsh),
                     q.ctypes.data_as(dp), mult.ctypes.data_as(ip))
    return shell, nsh.value, q[:nsh.value], mult[:nsh.value]


def check(H, n, Lbox):
    """shell_average of the indicator of each Fortran shell recovers it: the same partition, |q| and multiplicities."""
    shell, nsh, q, mult = fortran_shells(H, n, Lbox)
    onehot = (shell[None, :] == np.arange(1, nsh + 1)[:, None]).astype(float)        # [nsh, Nq]
    pq, mean, pmult = shell_average(n, Lbox, onehot)
    assert len(pq) == nsh and np.array_equal(pmult, mult), (len(pq), nsh)
    assert np.array_equal(mean, np.eye(nsh)), "a vector sits in different shells on the two sides"
    # |q| = sqrt(sum of the shell's cnt values of |q|^2 / cnt): the two sides add the same positive terms in different
    # orders (at most cnt - 1 roundings of half an ulp each, on either side), then divide and take the root
    assert np.all(np.abs(pq - q) <= (mult // 2 + 2) * np.spacing(q)), np.max(np.abs(pq - q) / np.spacing(q))
    assert np.all(np.diff(q) > 0) and mult.sum() == 2 * len(n)
    return nsh, q, mult


@pytest.mark.parametrize("Lbox,dim,nmax", [([7.3, 4.1, 5.9], 3, 2), ([7.3, 4.1, 5.9], 3, 3), ([7.3, 4.1, 5.9], 3, 8),
                                           ([5.0, 8.0], 2, 20), ([3.2, 4.8, 6.4], 3, 6)])
def test_shells_of_a_box_with_unequal_sides(host, Lbox, dim, nmax):
    n = vectors(dim, nmax)
    nsh, q, mult = check(host, n, np.array(Lbox))
    print(f"Lbox {Lbox} nmax {nmax}: {len(n)} vectors in {nsh} shells, largest multiplicity {mult.max()}")
    if Lbox[0] == 7.3:                      # incommensurate sides: only (+-n_1, +-n_2, +-n_3) share a |q|
        assert mult.max() <= 8
    else:                                   # 5:8 and 2:3:4: (8,0) and (0,5) resp. (2,0,0), (0,3,0), (0,0,4) coincide
        assert mult.max() > 2 ** dim or nsh < len({tuple(np.abs(v)) for v in n})


def test_the_cubic_branch_still_agrees(host):
    for dim, nmax in ((3, 4), (2, 9)):
        n = vectors(dim, nmax)
        nsh, q, mult = check(host, n, np.full(dim, 6.25))
        assert nsh == len(set((n.astype(int) ** 2).sum(1).tolist()))


@pytest.mark.parametrize("rel,merged", [(1e-13, True), (1e-11, False)])
def test_near_degenerate_shells(host, rel, merged):
    """Sides chosen so that |q|^2 of (1,0,0) and (0,1,0) differ by `rel` relative: below 1e-12 they share a shell, above
    they do not; (0,0,1) is far off.  The construction is checked on the numbers both sides compute from."""
    L0 = 6.0
    L = np.array([L0, L0 * (1.0 + 0.5 * rel), 4.5])          # q2 ~ L^-2: a relative shift of rel / 2 in L is rel in q2
    n = vectors(3, 2)
    qb = 2.0 * np.pi / L
    q2 = ((n * qb) ** 2).sum(axis=1)
    a = int(np.flatnonzero((n == [1, 0, 0]).all(1))[0])
    b = int(np.flatnonzero((n == [0, 1, 0]).all(1))[0])
    gap = (q2[a] - q2[b]) / q2[a]
    assert L[0] != L[1] and q2[a] > q2[b]
    assert (0.5e-13 < gap < 2e-13) if merged else (0.5e-11 < gap < 2e-11), gap
    shell, nsh, q, mult = fortran_shells(host, n, L)
    assert (shell[a] == shell[b]) == merged
    check(host, n, L)
