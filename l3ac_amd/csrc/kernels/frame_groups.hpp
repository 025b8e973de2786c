// The un-centred frames of lpc, bands, coherence and pitch .hip: frame t of a clip is its samples t hop .. t hop + n - 1, a
// clip of fewer than n samples has no frame, and a workgroup stages a group of g consecutive frames in LDS once: frame k of the group starts
// at k pitch, pitch = min(hop, n), so overlapping frames share their samples and the samples between frames further apart are never read.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

__host__ __device__ __forceinline__ int64_t uncentred_frames(int64_t samples, int n, int hop) { return samples < n ? 0 : 1 + (samples - n) / hop; }

// The base of a family's geometry.  n is the frame length (pitch.hip: its span); g is the family's own choice.
struct FrameGroups {
    int n, hop, pitch, g;
    void set_frames(int n_, int hop_) { n = n_, hop = hop_, pitch = hop_ < n_ ? hop_ : n_; }
    __host__ __device__ int64_t frames(int64_t samples) const { return uncentred_frames(samples, n, hop); }
    // the frames of the group that starts at frame t0 of a clip of `frames` frames
    __host__ __device__ int count(int64_t t0, int64_t frames) const { return t0 >= frames ? 0 : (frames - t0 < g ? (int)(frames - t0) : g); }
    __host__ __device__ int floats(int cnt) const { return (cnt - 1) * pitch + n; }  // the staged samples of cnt frames
    __host__ __device__ int span_max() const { return floats(g); }
    // sample k of the stage of group t0 is this sample of the clip; every one lies inside a frame of the group
    __host__ __device__ int64_t src(int64_t t0, int k) const { return hop <= n ? t0 * hop + k : (t0 + k / n) * hop + k % n; }
};

// The cnt frames of group t0 of the one or two sides (x1 == nullptr: one) into xs0 and xs1 [floats(cnt)]; the caller's barrier follows.
template <int THREADS>
__device__ __forceinline__ void stage_group(const FrameGroups& fg, int64_t t0, int cnt, const float* x0, const float* x1, float* xs0, float* xs1) {
    const int floats = fg.floats(cnt);
    for (int k = threadIdx.x; k < floats; k += THREADS) {
        const int64_t src = fg.src(t0, k);
        xs0[k] = x0[src];
        if (x1) xs1[k] = x1[src];
    }
}

// The window into win [n] (nullptr: rectangular); the caller's barrier follows.  (coherence.hip stages it once for the groups of a chunk.)
template <int THREADS>
__device__ __forceinline__ void stage_window(int n, const float* window, float* win) {
    for (int i = threadIdx.x; i < n; i += THREADS) win[i] = window ? window[i] : 1.f;
}
