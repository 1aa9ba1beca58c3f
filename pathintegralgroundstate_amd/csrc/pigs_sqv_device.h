// pigs_sqv_device.h -- rho_q of one slice on the full reciprocal grid: the device code that k_sqv_rho2 (pigs_sqv.hip) and
// k_fqv_rho (pigs_fqv.hip) both run.  One statement of the phasor table, the prefix product, the chunks and the four fma
// sums, so that the two kernels give the same C and S to the last bit; they differ only in what they store of them.
#pragma once

#include "pigs_device.h"
#include "pigs_kernels.h"

namespace pigs {

struct __align__(16) c2 { double x, y; };

// e^(i n phase) from the table row of one particle and axis (entry m = |n|; entry 0 is 1)
__device__ __forceinline__ c2 phasor(const c2 *row, int n)
{
    c2 e = row[n < 0 ? -n : n];
    if (n < 0) e.y = -e.y;
    return e;
}

// what a kernel keeps of rho_q = C + i S: PHASE false, C^2 + S^2 in a double; PHASE true, (C, S) in a c2
template <bool PHASE>
__device__ __forceinline__ void sqv_store(double *out, long long iqv, double c, double s)
{
    if (PHASE) reinterpret_cast<c2 *>(out)[iqv] = c2{c, s};
    else out[iqv] = c * c + s * s;
}

// The whole workgroup calls this for one slice X ([k][NpPad] rows of a walker's slice); out holds Nq elements of the
// slice (doubles, or c2 with PHASE).  tab: [k][particle of the tile][m = 0..ms-1], ms = kSqvChunk * nchunk + 1, in LDS.
template <int DIM, bool PHASE>
__device__ __forceinline__ void sqv_rho_slice(
    const DevParams &P, const double *__restrict__ X, c2 *tab, int nmax, int tile, int nprefix, int nchunk, long long Nq,
    double pi, double *__restrict__ out)
{
    const int Np = P.Np, NpPad = P.NpPad;
    const int S = 2 * nmax + 1, ms = kSqvChunk * nchunk + 1;
    const int nitems = nprefix * nchunk;
    long long Sp = 1;                                                 // S^(dim-1): the prefixes of the whole cube
    for (int k = 1; k < DIM; ++k) Sp *= S;

    for (int item0 = 0; item0 < nitems; item0 += blockDim.x) {
        const int item = item0 + threadIdx.x;
        const bool live = item < nitems;
        const int chunk = live ? item / nprefix : 0, p = live ? item - chunk * nprefix : 0;
        const long long rp = p + (Sp - 1) / 2;                        // rank of the prefix in its cube; p = 0 is the zero prefix
        int n1 = 0, n2 = 0;
        if (DIM == 2) n1 = (int)rp - nmax;
        if (DIM == 3) { n1 = (int)(rp / S) - nmax; n2 = (int)(rp - (rp / S) * S) - nmax; }
        const int m0 = kSqvChunk * chunk + 1;
        double a0r = 0.0, a0i = 0.0;                                  // m = 0 (chunk 0 keeps it)
        double p1[kSqvChunk], p2[kSqvChunk], p3[kSqvChunk], p4[kSqvChunk];
#pragma unroll
        for (int m = 0; m < kSqvChunk; ++m) p1[m] = p2[m] = p3[m] = p4[m] = 0.0;

        for (int i0 = 0; i0 < Np; i0 += tile) {
            const int nt = min(tile, Np - i0);
            __syncthreads();                                          // the previous tile has been consumed
            for (int t = threadIdx.x; t < DIM * nt * ms; t += blockDim.x) {
                const int k = t / (nt * ms), r = t - k * (nt * ms), il = r / ms, m = r - il * ms;
                const double qbin = 2.0 * pi / P.Lbox[k];             // vpi.f90:119
                const double qr = (double)(float)m * qbin * X[(size_t)k * NpPad + i0 + il];
                c2 e;
                sincos(qr, &e.y, &e.x);
                tab[((size_t)k * tile + il) * ms + m] = e;
            }
            __syncthreads();
            if (live) {
                for (int il = 0; il < nt; ++il) {
                    double ar = 1.0, ai = 0.0;
                    if (DIM >= 2) {
                        const c2 e = phasor(tab + (size_t)il * ms, n1);
                        ar = e.x; ai = e.y;
                    }
                    if (DIM == 3) {
                        const c2 e = phasor(tab + ((size_t)tile + il) * ms, n2);
                        const double br = ar * e.x - ai * e.y, bi = ar * e.y + ai * e.x;
                        ar = br; ai = bi;
                    }
                    a0r = a0r + ar; a0i = a0i + ai;
                    const c2 *last = tab + ((size_t)(DIM - 1) * tile + il) * ms + m0;
#pragma unroll
                    for (int m = 0; m < kSqvChunk; ++m) {
                        const c2 e = last[m];
                        p1[m] = __builtin_fma(ar, e.x, p1[m]);
                        p2[m] = __builtin_fma(ai, e.y, p2[m]);
                        p3[m] = __builtin_fma(ar, e.y, p3[m]);
                        p4[m] = __builtin_fma(ai, e.x, p4[m]);
                    }
                }
            }
        }
        if (live) {
            // index of (prefix, n_dim = 0); the stored vectors are those with index >= 0
            const long long base = rp * S + nmax - Nq - 1;
            if (chunk == 0 && base >= 0) sqv_store<PHASE>(out, base, a0r, a0i);
#pragma unroll
            for (int m = 0; m < kSqvChunk; ++m) {
                const int mm = m0 + m;
                if (mm > nmax) continue;
                const double cp = p1[m] - p2[m], sp = p3[m] + p4[m];      // a e[m]
                const double cm = p1[m] + p2[m], sm = p4[m] - p3[m];      // a conj(e[m])
                sqv_store<PHASE>(out, base + mm, cp, sp);
                if (base - mm >= 0) sqv_store<PHASE>(out, base - mm, cm, sm);
            }
        }
    }
}

} // namespace pigs
