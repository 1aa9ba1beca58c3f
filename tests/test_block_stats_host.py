"""The block statistics behind every estimator file of the front end: host/pigs_block_stats.f90 (a series' per-walker
sums, its slice of the all-reduced block vector, the walker average taken from it, a family's count) through its
C-callable handle bs_series_run, against a Python loop in the same order, bit for bit, and against the independent
block_stats_numpy.  Three walkers in two shards (2 + 1) over four blocks: one block that nobody counts, one walker that
counts only some blocks.  A second series without a slice of the vector follows the first as the |q|-shell means follow
their vectors: per walker the group sums of the walker's value, for the walker average those of the averaged vector.
No GPU: the host library linked against tests/shim."""
import ctypes as C

import numpy as np
import pytest

import block_stats_numpy as bs
from helpers import same_bits
from hostlib import build_cpu_host

N, NW, NW1, NBLOCK, M, VEC0 = 5, 3, 2, 4, 2, 7
GROUP = np.array([1, 2, 2, 1, 2], np.int32)                  # element -> group 1..M
#                    block 0  1  2  3
COUNTED = np.array([[1, 1, 0, 1],                            # shard 1
                    [1, 0, 0, 1],                            # shard 1: counts only some blocks
                    [1, 1, 0, 0]], np.int32)                 # shard 2; block 2 is counted for nobody


def group_sums(x):
    y = np.zeros(M)
    for i in range(N):
        y[GROUP[i] - 1] = y[GROUP[i] - 1] + x[i]
    return y


@pytest.fixture(scope="module")
def run():
    shim, lib, _ = build_cpu_host()
    C.CDLL(shim, mode=C.RTLD_GLOBAL)
    H = C.CDLL(lib)
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    H.bs_series_run.argtypes = [C.c_int] * 5 + [ip, dp, ip, C.c_int] + [dp] * 8 + [ip, ip]
    H.bs_series_run.restype = None
    # values with full mantissas, so that every sum and every division rounds
    b = np.random.default_rng(20).standard_normal((NW, NBLOCK, N)) * np.array([1.0, 1e-3, 7.0, 1e4, 0.3]) + 0.5
    out = {k: np.zeros(s) for k, s in dict(wsum=(NW, N), wsq=(NW, N), asum=N, asq=N, gsum=(NW, M), gsq=(NW, M),
                                           gasum=M, gasq=M).items()}
    nav, nvec = C.c_int32(), C.c_int32()
    bf = np.ascontiguousarray(b.transpose(1, 0, 2))          # [Nblock, NW, N] C order == b(n,NW,Nblock)
    cf = np.ascontiguousarray(COUNTED.T)                     # [Nblock, NW] C order == counted(NW,Nblock)
    H.bs_series_run(N, NW, NW1, NBLOCK, M, GROUP.ctypes.data_as(ip), bf.ctypes.data_as(dp), cf.ctypes.data_as(ip), VEC0,
                    *[out[k].ctypes.data_as(dp) for k in ("wsum", "wsq", "asum", "asq", "gsum", "gsq", "gasum", "gasq")],
                    C.byref(nav), C.byref(nvec))
    return b, out, nav.value, nvec.value


def test_series_against_the_same_loop_bit_for_bit(run):
    b, out, nav, nvec = run
    assert nvec == VEC0 + N + 1, "the series with a slice claims n doubles, the count one, the other series none"
    shards = [range(0, NW1), range(NW1, NW)]
    wsum, wsq, gsum, gsq = np.zeros((NW, N)), np.zeros((NW, N)), np.zeros((NW, M)), np.zeros((NW, M))
    asum, asq, gasum, gasq, n_av = np.zeros(N), np.zeros(N), np.zeros(M), np.zeros(M), 0
    for k in range(NBLOCK):
        vec, cnt = [np.zeros(N), np.zeros(N)], [0.0, 0.0]
        for ish, ws in enumerate(shards):
            for w in ws:
                if not COUNTED[w, k]:
                    continue
                g = group_sums(b[w, k])
                wsum[w] = wsum[w] + b[w, k]
                wsq[w] = wsq[w] + b[w, k] * b[w, k]
                gsum[w] = gsum[w] + g
                gsq[w] = gsq[w] + g * g
                vec[ish] = vec[ish] + b[w, k]
                cnt[ish] = cnt[ish] + 1.0
        red, c = vec[0] + vec[1], int(round(cnt[0] + cnt[1]))
        if c > 0:
            n_av += 1
            mean = red / c
            g = group_sums(mean)
            asum, asq = asum + mean, asq + mean * mean
            gasum, gasq = gasum + g, gasq + g * g
    assert nav == n_av == 3
    for name, want in dict(wsum=wsum, wsq=wsq, asum=asum, asq=asq, gsum=gsum, gsq=gsq, gasum=gasum, gasq=gasq).items():
        assert same_bits(out[name], want), name


def test_means_and_errors_against_block_stats_numpy(run):
    b, out, nav, _ = run
    counted = COUNTED.astype(bool)
    g = np.array([[group_sums(b[w, k]) for k in range(NBLOCK)] for w in range(NW)])

    def file_columns(s1, s2, n):
        mean = s1 / n
        return mean, np.sqrt(np.maximum((s2 / n - mean * mean) / n, 0.0))

    for w in range(NW):
        for vals, s1, s2 in ((b, out["wsum"][w], out["wsq"][w]), (g, out["gsum"][w], out["gsq"][w])):
            mean, err, n = bs.walker_stats(vals, counted, w)
            assert n == counted[w].sum()
            m, e = file_columns(s1, s2, n)
            np.testing.assert_allclose(m, mean, rtol=1e-13, atol=0)
            np.testing.assert_allclose(e, err, rtol=1e-13, atol=0)
    avg, any_counted = bs.walker_average(b, counted)
    mean, err, n = bs.moments(avg, any_counted)
    assert n == nav
    m, e = file_columns(out["asum"], out["asq"], n)
    np.testing.assert_allclose(m, mean, rtol=1e-13, atol=0)
    np.testing.assert_allclose(e, err, rtol=1e-13, atol=0)
    # the series without a slice: the group sums of the averaged vector, not an average of group sums
    gavg = np.array([group_sums(avg[k]) for k in range(NBLOCK)])
    mean, err, n = bs.moments(gavg, any_counted)
    m, e = file_columns(out["gasum"], out["gasq"], n)
    np.testing.assert_allclose(m, mean, rtol=1e-13, atol=0)
    np.testing.assert_allclose(e, err, rtol=1e-13, atol=0)
