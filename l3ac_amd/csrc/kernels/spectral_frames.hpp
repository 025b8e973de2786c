// What the two spectral families share beside the transform of fft_f64.hpp (bands.hip, coherence.hip): the limits and the
// geometry of a launch over un-centred frames, its LDS formula, and a band's run of non-zero weights.
#pragma once

#include "frame_groups.hpp"
#include "metric_common.hpp"

constexpr int SP_MIN_FRAME = 2, SP_MAX_FRAME = 2048;
constexpr int SP_MIN_FFT = 16, SP_MAX_FFT = 4096;
constexpr int SP_MIN_BANDS = 2, SP_MAX_BANDS = 64;

// A group is g consecutive frames of one clip; g and the waves of a frame are functions of n_fft alone: one wave a frame (four frames in
// step) and g = 16 up to n_fft = 256, the whole workgroup of four waves a frame above, with g = 8 up to 1024, 4 at 2048 and 2 at 4096.
struct SpectralGeom : FrameGroups {
    int n_fft, log2n, h, wpf;  // transform length and its logarithm, bins kept, waves of a frame
};

inline int check_n_fft(const char* what, int32_t n_fft) {
    L3AC_REQUIRE(n_fft >= SP_MIN_FFT && n_fft <= SP_MAX_FFT && (n_fft & (n_fft - 1)) == 0, "%s: n_fft %d is not a power of two in %d..%d", what, n_fft,
                 SP_MIN_FFT, SP_MAX_FFT);
    return L3AC_OK;
}

inline int spectral_geom(const char* what, int32_t frame, int32_t hop, int32_t n_fft, SpectralGeom* p) {
    L3AC_REQUIRE(frame >= SP_MIN_FRAME && frame <= SP_MAX_FRAME, "%s: frame %d outside %d..%d", what, frame, SP_MIN_FRAME, SP_MAX_FRAME);
    L3AC_REQUIRE(hop >= 1, "%s: hop %d must be at least 1", what, hop);
    L3AC_TRY(check_n_fft(what, n_fft));
    L3AC_REQUIRE(n_fft >= frame, "%s: n_fft %d is below the frame %d", what, n_fft, frame);
    p->set_frames(frame, hop);
    p->n_fft = n_fft, p->h = n_fft / 2;
    p->log2n = 0;
    while ((1 << p->log2n) < n_fft) ++p->log2n;
    p->wpf = n_fft <= 256 ? 1 : 4;
    p->g = n_fft <= 256 ? 16 : (n_fft <= 1024 ? 8 : (n_fft == 2048 ? 4 : 2));
    return L3AC_OK;
}

// The dynamic LDS of a launch: per team three arrays of n_fft doubles and the family's `team_extra` doubles, the family's `tail` bytes, the
// window and the group's samples of both sides.
constexpr int spectral_lds(int n_fft, int wpf, int g, int pitch, int n, int team_extra, int tail) {
    return (4 / wpf) * (3 * n_fft + team_extra) * 8 + tail + (n + 2 * ((g - 1) * pitch + n)) * 4;
}
// the largest launches: a hop at or above the frame, the longest frame the transform takes
template <int TEAM_EXTRA, int TAIL>
constexpr int spectral_lds_max() {
    constexpr int most = std::max(std::max(spectral_lds(4096, 4, 2, 2048, 2048, TEAM_EXTRA, TAIL), spectral_lds(2048, 4, 4, 2048, 2048, TEAM_EXTRA, TAIL)),
                                  std::max(spectral_lds(1024, 4, 8, 1024, 1024, TEAM_EXTRA, TAIL), spectral_lds(256, 1, 16, 256, 256, TEAM_EXTRA, TAIL)));
    static_assert(most <= 160 * 1024, "a group lives in one workgroup's LDS");
    return most;
}

// Thread i < nb: band i's non-zero weights of weights [nb][h] are [runs[2 i], runs[2 i + 1]); the caller's barrier follows.
__device__ __forceinline__ void band_runs(const double* weights, int nb, int h, int* runs) {
    const int i = threadIdx.x;
    if (!weights || i >= nb) return;
    const double* wrow = weights + (int64_t)i * h;
    int lo = h, hi = 0;
    for (int k = 0; k < h; ++k)
        if (wrow[k] != 0.0) lo = k < lo ? k : lo, hi = k + 1;
    runs[2 * i] = lo < hi ? lo : 0, runs[2 * i + 1] = hi;
}
