// Spans of 4-byte elements moved or zeroed by a whole grid row: what chunk.hip and stream.hip (section 3.9) share.
// Elements are moved as 32-bit integers: int32 tokens and fp32 samples / features share the code, no floating-point instruction touches them.
// Where source and destination are congruent modulo 16 bytes a span is a scalar head up to the destination's next 16-byte boundary, a
// body of 16-byte loads and stores, and a scalar tail; otherwise every lane moves one dword per step (still one coalesced 256-byte access
// per wave).  The choice depends on the two addresses only, so it is uniform over every workgroup that works on the span.  `tid` / `stride`:
// this lane's index among, and the number of, the lanes that share the span; every element is written by exactly one of them.
#pragma once

#include <algorithm>

#include "../common.hpp"

namespace {

constexpr int SPAN_THREADS = 256;

__device__ __forceinline__ void copy_span(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, int64_t n, int64_t tid,
                                          int64_t stride) {
    const uintptr_t da = reinterpret_cast<uintptr_t>(dst), sa = reinterpret_cast<uintptr_t>(src);
    if (((da ^ sa) & 15) == 0) {
        int64_t head = (int64_t)(((16 - (da & 15)) & 15) >> 2);
        if (head > n) head = n;
        const int64_t body = (n - head) >> 2;
        if (tid < head) dst[tid] = src[tid];
        const uint4* s4 = reinterpret_cast<const uint4*>(src + head);
        uint4* d4 = reinterpret_cast<uint4*>(dst + head);
        for (int64_t e = tid; e < body; e += stride) d4[e] = s4[e];
        const int64_t done = head + body * 4;
        if (tid < n - done) dst[done + tid] = src[done + tid];
    } else {
        for (int64_t e = tid; e < n; e += stride) dst[e] = src[e];
    }
}

__device__ __forceinline__ void zero_span(uint32_t* __restrict__ dst, int64_t n, int64_t tid, int64_t stride) {
    const uintptr_t da = reinterpret_cast<uintptr_t>(dst);
    int64_t head = (int64_t)(((16 - (da & 15)) & 15) >> 2);
    if (head > n) head = n;
    const int64_t body = (n - head) >> 2;
    if (tid < head) dst[tid] = 0u;
    uint4* d4 = reinterpret_cast<uint4*>(dst + head);
    for (int64_t e = tid; e < body; e += stride) d4[e] = make_uint4(0u, 0u, 0u, 0u);
    const int64_t done = head + body * 4;
    if (tid < n - done) dst[done + tid] = 0u;
}

inline unsigned span_blocks(int64_t elements) {  // 16 elements (four 16-byte accesses) per lane, at most 64 workgroups per span
    return (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div64(elements, (int64_t)SPAN_THREADS * 16), 1), 64);
}

}  // namespace
