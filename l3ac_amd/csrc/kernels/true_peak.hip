// True peak of mono clips after ITU-R BS.1770-4 annex 2 / EBU Tech 3341: the largest magnitude of the clip oversampled L times, and its
// sample peak (include/l3ac_hip.h, "true peak").  No reference counterpart.
//
// The oversampler IS the library's sample-rate conversion fs -> L fs (kernels/resample.hip): up = L, down = 1, half_len = 10 L, K = 21
// taps a phase, and output m = L a + p (input position a, phase p) is
//   y[m] = sum_{t < 21} g_p[t] * x[a - 10 + t],   x zero before sample 0 and at and after the clip's own length n,
// evaluated as the fp32 fmaf chain over t = 0 .. 20 from +0, the chain of resample_poly_kernel (whose zero taps before and after add
// +0).  The taps come from resample_phase_taps, the design behind l3ac_resample_bank, and travel as kernel arguments (L x 21 floats, at
// most 336 bytes): no table, no upload, nothing to warm up before a capture.  The oversampled signal is never written: per clip the
// kernels read its 4 n bytes and write 16.
//   1. true_peak_tile_kernel<L>  grid (tiles of TP_TILE input positions, clips): the tile and its 10 + 10 halo staged once in LDS; a
//                                thread owns 4 consecutive positions, reads their 24-sample window as six quads and evaluates the 4 L
//                                chains; max |y| and max |x| over the workgroup -> tile_max[clip][tile][2] fp32
//   2. true_peak_clip_kernel     one workgroup per clip: the maxima of its own tiles -> stats = {max(peak, os), peak} as fp64
// A maximum does not depend on the order it is taken in: a clip's bits depend on its own samples alone, never on the batch, the row, the
// stride, the tiling or the scratch size.  No atomics.  fmaxf drops a NaN: non-finite samples leave their own clip's result unspecified and
// touch no other clip (every staged value belongs to the workgroup's own clip).
#include "metric_common.hpp"

#include <vector>

namespace {

constexpr int TP_K = 21;                  // taps per phase of an L-fold oversampler: ceil((20 L + 1) / L)
constexpr int TP_HALO = 10;               // inputs before and after a position that its outputs read
constexpr int TP_THREADS = 256;
constexpr int TP_PER_THREAD = 4;          // consecutive positions a thread, one ds_read_b128 apart
constexpr int TP_TILE = TP_THREADS * TP_PER_THREAD;  // chosen from the code (a quad per lane, 4 KiB of LDS), not from a measurement
constexpr int TP_WINDOW = TP_PER_THREAD + 2 * TP_HALO;  // 24 samples = 6 quads
constexpr int TP_LDS = TP_TILE + 2 * TP_HALO + 4;       // the last thread's sixth quad ends at TP_TILE + 23
constexpr int TP_MIN_RATE = 8000, TP_SPLIT_RATE = 96000, TP_MAX_RATE = 192000;

template <int L>
struct TpTaps {
    float g[L][TP_K];
};

int factor_of(int32_t fs) {
    L3AC_REQUIRE(fs >= TP_MIN_RATE && fs <= TP_MAX_RATE, "true_peak: sample_rate %d outside %d..%d", fs, TP_MIN_RATE, TP_MAX_RATE);
    return fs < TP_SPLIT_RATE ? 4 : 2;
}

struct TpGeom {
    int factor;
    int64_t tiles, tile_max, total_min;  // tiles of the longest clip; byte offset of tile_max [batch][tiles][2] fp32; the scratch
};

int tp_geom(int32_t batch, int64_t max_samples, int32_t sample_rate, TpGeom* g) {
    const int factor = factor_of(sample_rate);
    if (factor < 0) return factor;
    L3AC_TRY(check_clip_batch("true_peak", batch, max_samples));
    g->factor = factor;
    g->tiles = ceil_div64(max_samples, TP_TILE);
    ScratchPlan plan(batch);
    g->tile_max = plan.take((int64_t)batch * g->tiles * 2 * 4);
    g->total_min = plan.bytes;
    return L3AC_OK;
}

template <int L>
__global__ __launch_bounds__(TP_THREADS) void true_peak_tile_kernel(const float* __restrict__ audio, int64_t stride, int64_t max_samples,
                                                                  const int* __restrict__ lens, TpTaps<L> taps, int64_t tiles,
                                                                  float* __restrict__ tile_max) {
    __shared__ __attribute__((aligned(16))) float xs[TP_LDS];  // xs[i] = x[a0 - 10 + i]
    __shared__ double red[TP_THREADS / 64];
    const int b = blockIdx.y;
    const int64_t n = lens ? lens[b] : max_samples;
    const int64_t a0 = (int64_t)blockIdx.x * TP_TILE;
    if (a0 >= n) return;  // (the whole workgroup: the clip kernel reads the clip's own tiles only)
    const float* x = audio + (int64_t)b * stride;
    for (int i = threadIdx.x; i < TP_LDS; i += TP_THREADS) {
        const int64_t at = a0 - TP_HALO + i;
        xs[i] = (at >= 0 && at < n) ? x[at] : 0.f;
    }
    __syncthreads();
    float w[TP_WINDOW];
#pragma unroll
    for (int q = 0; q < TP_WINDOW / 4; ++q) {
        const float4 v = *reinterpret_cast<const float4*>(xs + TP_PER_THREAD * threadIdx.x + 4 * q);
        w[4 * q] = v.x, w[4 * q + 1] = v.y, w[4 * q + 2] = v.z, w[4 * q + 3] = v.w;
    }
    float os = 0.f, peak = 0.f;
#pragma unroll
    for (int j = 0; j < TP_PER_THREAD; ++j) {
        if (a0 + TP_PER_THREAD * threadIdx.x + j >= n) break;  // outputs L a + p exist for a < n only
        peak = fmaxf(peak, fabsf(w[TP_HALO + j]));
#pragma unroll
        for (int p = 0; p < L; ++p) {
            float acc = 0.f;
#pragma unroll
            for (int t = 0; t < TP_K; ++t) acc = fmaf(taps.g[p][t], w[j + t], acc);
            os = fmaxf(os, fabsf(acc));
        }
    }
    const double os_max = block_max<TP_THREADS>((double)os, red), peak_max = block_max<TP_THREADS>((double)peak, red);
    if (threadIdx.x == 0) {
        float* out = tile_max + ((int64_t)b * tiles + blockIdx.x) * 2;
        out[0] = (float)os_max, out[1] = (float)peak_max;  // (fp32 values widened and narrowed: exact)
    }
}

__global__ __launch_bounds__(TP_THREADS) void true_peak_clip_kernel(int64_t max_samples, const int* __restrict__ lens, int64_t tiles,
                                                                  const float* __restrict__ tile_max, double* __restrict__ stats) {
    __shared__ double red[TP_THREADS / 64];
    const int b = blockIdx.x;
    const int64_t n = lens ? lens[b] : max_samples;
    const int64_t own = (n + TP_TILE - 1) / TP_TILE;
    const float* m = tile_max + (int64_t)b * tiles * 2;
    double os = 0.0, peak = 0.0;
    for (int64_t t = threadIdx.x; t < own; t += TP_THREADS) os = fmax(os, (double)m[2 * t]), peak = fmax(peak, (double)m[2 * t + 1]);
    os = block_max<TP_THREADS>(os, red);
    peak = block_max<TP_THREADS>(peak, red);
    if (threadIdx.x == 0) stats[2 * (int64_t)b] = fmax(peak, os), stats[2 * (int64_t)b + 1] = peak;
}

template <int L>
int launch_tiles(hipStream_t s, const float* audio, int64_t stride, int32_t batch, int64_t max_samples, const int* lens, int32_t sample_rate,
                 int64_t tiles, float* tile_max) {
    ResamplePlan p;
    L3AC_TRY(resample_plan(sample_rate, L * sample_rate, &p));
    L3AC_REQUIRE(p.up == L && p.down == 1 && p.K == TP_K, "true_peak: internal: the %d-fold plan is up %d / down %d with %d taps", L, p.up, p.down, p.K);
    std::vector<float> host((size_t)L * TP_K);
    resample_phase_taps(p, host.data());
    TpTaps<L> taps;
    for (int ph = 0; ph < L; ++ph)
        for (int t = 0; t < TP_K; ++t) taps.g[ph][t] = host[(size_t)ph * TP_K + t];
    ProfScope prof(s, "true_peak_tile_kernel", 2.0 * L * TP_K * batch * (double)max_samples, 4.0 * batch * (double)max_samples);
    hipLaunchKernelGGL(true_peak_tile_kernel<L>, dim3((unsigned)tiles, (unsigned)batch), dim3(TP_THREADS), 0, s, audio, stride, max_samples, lens, taps,
                       tiles, tile_max);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

}  // namespace

extern "C" {

int32_t l3ac_true_peak_factor(int32_t sample_rate) { return factor_of(sample_rate); }

int32_t l3ac_true_peak_tile(void) { return TP_TILE; }

int64_t l3ac_true_peak_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sample_rate) {
    TpGeom g;
    L3AC_TRY(tp_geom(batch, max_samples, sample_rate, &g));
    return g.total_min;
}

int l3ac_true_peak(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, int32_t sample_rate,
                   double* stats, void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    TpGeom g;
    L3AC_TRY(tp_geom(batch, max_samples, sample_rate, &g));
    L3AC_REQUIRE(audio && stats, "true_peak: null buffer");
    L3AC_REQUIRE(batch == 1 || audio_stride >= max_samples, "true_peak: row stride %lld below max_samples %lld", (long long)audio_stride,
                 (long long)max_samples);
    L3AC_TRY(check_clip_lengths("true_peak", samples, batch, max_samples));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "true_peak", "true_peak", samples, batch, scratch, scratch_bytes, g.total_min, &lens));
    float* tile_max = reinterpret_cast<float*>(static_cast<char*>(scratch) + g.tile_max);
    if (g.factor == 4)
        L3AC_TRY(launch_tiles<4>(s, audio, audio_stride, batch, max_samples, lens, sample_rate, g.tiles, tile_max));
    else
        L3AC_TRY(launch_tiles<2>(s, audio, audio_stride, batch, max_samples, lens, sample_rate, g.tiles, tile_max));
    ProfScope prof(s, "true_peak_clip_kernel", 0.0, 8.0 * batch * (double)g.tiles);
    hipLaunchKernelGGL(true_peak_clip_kernel, dim3((unsigned)batch), dim3(TP_THREADS), 0, s, max_samples, lens, g.tiles, tile_max, stats);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

}  // extern "C"
