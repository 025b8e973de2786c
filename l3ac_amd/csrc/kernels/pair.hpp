// An unevaluated sum hi + lo of two doubles (Dekker / Knuth): what the state scans of loudness.hip and iir.hip carry.  A matrix that
// advances a recursive filter's state over a whole segment has entries some 1e4 times its eigenvalues (a near-double pole: n p^n), so a
// matrix rounded to fp64, or a product summed in fp64, moves the decay of a free tail by 1e-9 a segment; with pairs the scan adds nothing
// to what the passes' own fp64 recursion costs.  The one fma here is spelled out; contraction is off from here to the end of the
// including file, which both files ask for anyway (the product of a multiply must not be fused into the add that follows it).
#pragma once

#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

struct Pair {
    double hi, lo;
};
__device__ __forceinline__ Pair fast_two_sum(double a, double b) {  // |a| >= |b|
    const double s = a + b;
    return {s, b - (s - a)};
}
__device__ __forceinline__ Pair pair_add(Pair a, Pair b) {
    const double s = a.hi + b.hi, bb = s - a.hi;
    const double err = (a.hi - (s - bb)) + (b.hi - bb);
    return fast_two_sum(s, err + (a.lo + b.lo));
}
__device__ __forceinline__ Pair pair_mul(Pair a, Pair b) {
    const double p = a.hi * b.hi;
    const double err = fma(a.hi, b.hi, -p);
    return fast_two_sum(p, err + (a.hi * b.lo + a.lo * b.hi));
}
