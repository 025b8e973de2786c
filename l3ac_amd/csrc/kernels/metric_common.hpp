// What the metric families share (metrics, stoi, loudness, iir, pitch, align, mcd, lpc, sdr, bands, coherence .hip): the fixed-order workgroup
// reductions, the LDS sort and the trimmed and ordered means of the pair kernels (lpc, bands) on the device, and on the host the scratch layout, the checks
// of a batch of clips, the staging of their lengths and the frame scratch of a pair.  Each family's arithmetic, geometry and parameter checks are its own;
// the un-centred framing of lpc, bands, coherence and pitch lives in frame_groups.hpp, what the two spectral families share in spectral_frames.hpp.
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

__device__ __forceinline__ double clamp_to(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }  // (NaN stays NaN)

// ---- device: the pieces of a pair kernel (lpc.hip, bands.hip): one workgroup of THREADS holds a pair's frames in LDS ---------------------------
constexpr int PAIR_THREADS = 1024, PAIR_MAX_FRAMES = 16384;  // 16384 fp64 values are 128 KiB of the CU's 160 KiB of LDS
static_assert(PAIR_MAX_FRAMES * 8 + PAIR_MAX_FRAMES + 256 <= 160 * 1024, "a pair's values and flags live in one workgroup's LDS");

// The pair's frames: the clip's own, at most f_max and PAIR_MAX_FRAMES (the host checked both; the clamp bounds every index).
__device__ __forceinline__ int pair_frames(int64_t frames, int64_t f_max) { return (int)std::min(std::min(frames, f_max), (int64_t)PAIR_MAX_FRAMES); }

// The integer sum of v over the workgroup; every thread gets it.  Contains barriers, which also publish what the caller wrote to LDS before.
template <int THREADS>
__device__ __forceinline__ int block_count(int v) {
    __shared__ int wave_count[THREADS / 64];
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();  // the previous use of wave_count is over
    if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
    for (int w = 0; w < THREADS / 64; ++w) s += wave_count[w];
    return s;
}

// The mean of the `keep` smallest of the values value_of(f) of the frames f < frames with kept(f): they go to buf, +inf elsewhere up to the next
// power of two, lds_sort orders them and thread 0 adds the first `keep` in sorted order from +0 (the other threads' result means nothing).
// Whether the mean is defined is the caller's rule.  Ends with a barrier.
template <int THREADS, typename Value, typename Kept>
__device__ __forceinline__ double lds_trimmed_mean(double* buf, int frames, int keep, Value value_of, Kept kept) {
    int n_pad = 1;
    while (n_pad < frames) n_pad <<= 1;
    for (int f = threadIdx.x; f < n_pad; f += THREADS) buf[f] = (f < frames && kept(f)) ? value_of(f) : __builtin_huge_val();
    __syncthreads();
    lds_sort<THREADS>(buf, n_pad);
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int f = 0; f < keep; ++f) s = s + buf[f];
    __syncthreads();  // buf is read before the next use overwrites it
    return s / (double)keep;
}

// The sum of value_of(f) over the frames f < frames with counted(f), added by thread 0 in frame order from +0, over `count`; NaN where count
// is 0 (the other threads' result means nothing).  Ends with a barrier.
template <int THREADS, typename Value, typename Counted>
__device__ __forceinline__ double lds_ordered_mean(double* buf, int frames, int count, Value value_of, Counted counted) {
    for (int f = threadIdx.x; f < frames; f += THREADS) buf[f] = counted(f) ? value_of(f) : 0.0;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0)
        for (int f = 0; f < frames; ++f)
            if (counted(f)) s = s + buf[f];
    __syncthreads();  // buf is read before the next use overwrites it
    return count == 0 ? __builtin_nan("") : s / (double)count;
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

struct PairScratch {  // byte offsets into the caller's scratch, after the clips' lengths, and its size
    int64_t vals, flags, need;
};
// A pair's frames: at most the PAIR_MAX_FRAMES that one workgroup holds in LDS, then (vals != nullptr) the scratch regions of the frames'
// values [batch][f_max] of value_bytes each and of their flags [batch][f_max] int32.
inline int pair_frames_plan(const char* what, int32_t batch, int64_t f_max, int value_bytes, ScratchPlan& plan, int64_t* vals, int64_t* flags) {
    L3AC_REQUIRE(f_max <= PAIR_MAX_FRAMES, "%s: %lld frames are more than the %d of a pair", what, (long long)f_max, PAIR_MAX_FRAMES);
    if (vals) *vals = plan.take((int64_t)batch * f_max * value_bytes), *flags = plan.take((int64_t)batch * f_max * 4);
    return L3AC_OK;
}

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
