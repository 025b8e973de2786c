// What the metric families share (metrics, stoi, loudness, iir, pitch, align, mcd, lpc, sdr, bands, coherence .hip): the fixed-order workgroup
// reductions and the LDS sort on the device, and on the host the scratch layout, the checks of a batch of clips and the staging of their lengths.  Each
// family's arithmetic, geometry and parameter checks are its own.
#pragma once

#include "../kernels.hpp"

#include <algorithm>

// ---- device: THE fixed tree over a workgroup's values.  A xor tree inside each wave, then the waves' results in wave order; every thread
// gets the result.  "summed in fp64 in a fixed order" of every family's bit guarantee is this function.  (over_frames in stoi.hip and
// wave_min_int in pitch.hip are other trees and stay where they are.) ---------------------------------------------------------------------
template <int THREADS>
__device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();  // the previous use of lds is over
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) s += lds[w];
    return s;
}

template <int THREADS>
__device__ __forceinline__ double block_max(double v, double* lds) {  // (a maximum does not depend on the order)
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = lds[0];
#pragma unroll
    for (int w = 1; w < THREADS / 64; ++w) s = fmax(s, lds[w]);
    return s;
}

// The fold of 64 interleaved partial sums, one a lane (lpc.hip, sdr.hip): s[l] += s[l + h], h = 32 .. 1; lane 0 holds the sum (a lane at or
// above h adds what it is handed and is not read again).
__device__ __forceinline__ double fold64(double v) {
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) v = v + __shfl_down(v, h, 64);
    return v;
}

// The ascending sort of n_pad fp64 values in LDS (a power of two; the caller pads with +inf) by a whole workgroup of THREADS (lpc.hip,
// bands.hip: the trimmed means): a bitonic network.  The sorted sequence of a set of numbers does not depend on how it was reached.  The
// values are in place behind a barrier of the caller's; ends with a barrier.
template <int THREADS>
__device__ __forceinline__ void lds_sort(double* buf, int n_pad) {
    for (int size = 2; size <= n_pad; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = threadIdx.x; i < (n_pad >> 1); i += THREADS) {
                const int lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const double x = buf[lo], y = buf[hi];
                if ((x > y) == up) buf[lo] = y, buf[hi] = x;
            }
            __syncthreads();
        }
    }
}

// ---- host: the caller's scratch ---------------------------------------------------------------------------------------------------------
inline int64_t align256(int64_t v) { return round_up64(v, 256); }

// Byte offsets into a family's scratch, walked by its *_scratch_bytes function and its launcher alike.  Every layout begins with the
// clips' lengths, [batch] int32 at offset 0 (where stage_clip_lengths puts them); `bytes` is the size so far.
struct ScratchPlan {
    int64_t bytes;
    explicit ScratchPlan(int32_t batch) : bytes(align256((int64_t)batch * 4)) {}
    int64_t take(int64_t n) {  // a region of n bytes, rounded up to 256: its offset
        const int64_t at = bytes;
        bytes += align256(n);
        return at;
    }
    int64_t last(int64_t n) {  // the same for a final region whose size is not rounded up
        const int64_t at = bytes;
        bytes += n;
        return at;
    }
};

// ---- host: a batch of clips [batch][max_samples] and their optional lengths; `what` is the prefix of the entry's messages -------------------
inline int check_clip_batch(const char* what, int32_t batch, int64_t max_samples) {
    L3AC_REQUIRE(batch > 0 && batch <= 65535, "%s: batch %d outside 1..65535", what, batch);
    L3AC_REQUIRE(max_samples > 0 && max_samples < ((int64_t)1 << 31), "%s: max_samples %lld outside 1..2^31 - 1", what, (long long)max_samples);
    return L3AC_OK;
}

inline int check_clip_lengths(const char* what, const int32_t* samples, int32_t batch, int64_t max_samples) {
    for (int i = 0; samples && i < batch; ++i)
        L3AC_REQUIRE(samples[i] >= 1 && samples[i] <= max_samples, "%s: samples[%d] = %d outside [1, %lld]", what, i, samples[i],
                     (long long)max_samples);
    return L3AC_OK;
}

// The scratch of a launch: 256-byte aligned, at least `need` bytes (what l3ac_<entry>_scratch_bytes returns; entry == nullptr: an entry
// without one, whose scratch holds the lengths alone), and the lengths uploaded to its start.  *lens: their device copy, nullptr without.
inline int stage_clip_lengths(hipStream_t s, const char* what, const char* entry, const int32_t* samples, int32_t batch, void* scratch,
                              int64_t scratch_bytes, int64_t need, int** lens) {
    L3AC_REQUIRE(scratch && ((uintptr_t)scratch & 255) == 0, "%s: scratch must be a 256-byte aligned device buffer", what);
    if (entry)
        L3AC_REQUIRE(scratch_bytes >= need, "%s: scratch of %lld bytes is below l3ac_%s_scratch_bytes = %lld", what, (long long)scratch_bytes, entry,
                     (long long)need);
    else
        L3AC_REQUIRE(scratch_bytes >= need, "%s: scratch of %lld bytes is below the %lld of the clips' lengths", what, (long long)scratch_bytes,
                     (long long)need);
    *lens = samples ? static_cast<int*>(scratch) : nullptr;
    if (*lens) L3AC_TRY(launch_ragged_upload(s, *lens, samples, batch));
    return L3AC_OK;
}

// The clips of an entry that takes no scratch: their lengths travel as kernel arguments, RaggedUpload::CAP clips a launch; without lengths
// one launch takes the whole batch.  `launch(blk)` returns a status.
template <typename Launch>
int for_each_length_group(const int32_t* lens, int32_t batch, Launch launch) {
    const int group = lens ? RaggedUpload::CAP : batch;
    for (int off = 0; off < batch; off += group) {
        RaggedUpload blk{};
        blk.offset = off;
        blk.n = std::min(group, batch - off);
        for (int i = 0; lens && i < blk.n; ++i) blk.vals[i] = lens[off + i];
        L3AC_TRY(launch(blk));
    }
    return L3AC_OK;
}
