// The fp64 transform the spectral metric families share (bands.hip, coherence.hip; DESIGN.md §3.22, "the transform"): a complex radix-2
// decimation in time on two LDS arrays (re, im) of n_fft doubles, run by a team of `ts` threads (`tl` the thread's place in it).  Every
// output is one fixed expression tree: which thread takes which butterfly changes no bit.  Element i lives at swz(i): the 32 lanes of an LDS
// read group then meet 32 different 8-byte banks in every pass (the passes with a half-span below 32 would otherwise put lanes l and l + 16
// on one bank).  The barriers are the workgroup's: every team of a workgroup calls these functions in step.
//
// Contraction is off for everything below, whatever the including file does: every product and sum rounds on its own.
#pragma once

#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

__device__ __forceinline__ int swz(int i) { return i ^ ((i & 32) ? 31 : 0); }

// z[bitrev(j)] = ((double)x[j] (double)win[j], 0) for j < n_frame, (0, 0) up to nf = 1 << log2n; ends with a barrier
__device__ __forceinline__ void fft_f64_load(double* zre, double* zim, const float* x, const float* win, int n_frame, int nf, int log2n, int tl,
                                             int ts) {
    for (int i = tl; i < nf; i += ts) {
        const int r = swz((int)(__brev((unsigned)i) >> (32 - log2n)));
        zre[r] = i < n_frame ? (double)x[i] * (double)win[i] : 0.0;
        zim[r] = 0.0;
    }
    __syncthreads();
}

// the log2n passes of nf / 2 butterflies on the twiddle table tw [nf / 2][2], a barrier after each
__device__ __forceinline__ void fft_f64_passes(double* zre, double* zim, const double* tw, int nf, int log2n, int tl, int ts) {
    for (int s = 1; s <= log2n; ++s) {
        const int hf = 1 << (s - 1), tstep = nf >> s;
        for (int q = tl; q < (nf >> 1); q += ts) {
            const int j = q & (hf - 1);
            const int ia = ((q >> (s - 1)) << s) | j;
            const int sa = swz(ia), sb = swz(ia + hf);
            const double wr = tw[2 * j * tstep], wi = tw[2 * j * tstep + 1];
            const double ar = zre[sa], ai = zim[sa], br = zre[sb], bi = zim[sb];
            const double tr = wr * br - wi * bi, ti = wr * bi + wi * br;
            zre[sa] = ar + tr, zim[sa] = ai + ti;
            zre[sb] = ar - tr, zim[sb] = ai - ti;
        }
        __syncthreads();
    }
}
