// YIN pitch tracking (de Cheveigne & Kawahara 2002, steps 1-5) of mono clips, and the pairwise F0 metrics (include/l3ac_hip.h, "pitch";
// DESIGN.md §3.15, which is normative).  No reference counterpart.
//
//   pitch_kernel          grid (runs of PT_GROUPS frame groups, batch), 4 waves.  A group is G consecutive frames of one clip (G = 8, halved
//                         until the group fits the LDS budget; a function of the parameters alone).  Per group:
//     stage               the group's samples, (G - 1) min(hop, span) + span floats (FrameGroups of frame_groups.hpp, which owns the
//                         framing; its frame length n is the span here), go to LDS once; the loads run along the row at any
//                         alignment and any hop, and the NEXT group's first PT_PRE x 256 samples are loaded into registers before the
//                         current group is worked on
//     difference          an item is (frame, 64 lags); the waves take the items in turn.  Lane l holds lag tau = 64 chunk + l: the read of
//                         x[j] is one LDS address for the whole wave (a broadcast), the reads of x[j + tau] are consecutive across the lanes
//                         (no bank conflict).  d(tau) = sum_j (x[j] - x[j + tau])^2 in fp32, direct form: one subtraction and one fmaf per
//                         term, term j into accumulator j % 4, d = (a0 + a1) + (a2 + a3): an order that depends on W alone
//     prefix              fp64 from here on.  One lane per frame: S(tau) = S(tau - 1) + d(tau), in the order of tau
//     cmnd                every thread: c(tau) = d(tau) tau / S(tau), exactly 1 for tau = 0 and where S(tau) = 0
//     pick                one wave per frame: the first tau below the threshold and the first argmin are minima over (value, index), which
//                         do not depend on the order they are taken in; the descent, the parabola and f0 by every lane alike
//   pitch_metrics_kernel  one workgroup per clip pair: the counts, and the sum of the squared cents over fixed strides and a fixed tree
//
// A frame's values depend on its own span samples only — never on the batch, the clip's row, the row stride, the scratch size, the frame's
// place in its group or what lies after the clip's length; no atomics; no device table, so a first call can be captured.  Non-finite samples
// make NaN values in the frames that read them; every index is bounded by the parameters, whatever the values.
//
// Contraction is off for this whole file: the one fused operation, the fmaf of the difference function, is spelled out.
#include "frame_groups.hpp"
#include "metric_common.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int PT_THREADS = 256;
constexpr int PT_WAVES = PT_THREADS / 64;
constexpr int PT_FRAMES = 8;           // frames of a group at most
constexpr int PT_GROUPS = 4;           // groups a workgroup walks: the next one's loads are in flight while the current one is worked on
constexpr int PT_PRE = 8;              // registers per thread of that prefetch: the first 2048 samples of a group
constexpr int PT_LDS_TARGET = 48 << 10;  // a group of more than one frame stays below this: three workgroups per CU
constexpr int PT_MAX_SPAN = 4000;      // one frame's samples, d row and c row: 4 span + 12 (T + 1) <= 16 span <= 64,000 bytes of LDS
constexpr int PT_MIN_RATE = 8000, PT_MAX_RATE = 192000;
constexpr int PM_THREADS = 256;

struct PitchGeom : FrameGroups {  // n: the span = w + t samples a frame reads
    int fs, tau_min, tau_max, t, w, lds_bytes;  // t = tau_max + 1: lags 0 .. t; dynamic LDS of the launch
    double threshold;
};

int lds_need(int g, int pitch, int span, int lags) { return (int)round_up64(((int64_t)(g - 1) * pitch + span) * 4, 8) + g * lags * 12; }

// window / hop: -1 selects the default (tau_max / fs / 100)
int pitch_geom(int32_t fs, double fmin, double fmax, int32_t window, int32_t hop, PitchGeom* p) {
    L3AC_REQUIRE(fs >= PT_MIN_RATE && fs <= PT_MAX_RATE, "pitch: sample_rate %d outside %d..%d", fs, PT_MIN_RATE, PT_MAX_RATE);
    L3AC_REQUIRE(fmin > 0.0 && fmin < fmax && std::isfinite(fmax), "pitch: fmin %g must be positive and below fmax %g", fmin, fmax);
    L3AC_REQUIRE(fmax <= fs / 4.0, "pitch: fmax %g above sample_rate / 4 = %g", fmax, fs / 4.0);
    L3AC_REQUIRE(fs / fmin <= 2.0 * PT_MAX_SPAN, "pitch: fmin %g too low for sample_rate %d: span above the cap of %d samples", fmin, fs, PT_MAX_SPAN);
    p->fs = fs;
    p->tau_min = (int)std::floor(fs / fmax);
    p->tau_max = (int)std::ceil(fs / fmin);
    L3AC_REQUIRE(p->tau_max > p->tau_min, "pitch: fmin %g and fmax %g leave no lag range at sample_rate %d (tau_min %d, tau_max %d)", fmin, fmax, fs,
                 p->tau_min, p->tau_max);
    p->t = p->tau_max + 1;
    L3AC_REQUIRE(hop >= 1 || hop == -1, "pitch: hop %d must be at least 1 (-1: sample_rate / 100)", hop);
    L3AC_REQUIRE(window >= 1 || window == -1, "pitch: window %d must be at least 1 (-1: tau_max)", window);
    p->w = window == -1 ? p->tau_max : window;
    L3AC_REQUIRE((int64_t)p->w + p->t <= PT_MAX_SPAN, "pitch: span = window + tau_max + 1 = %lld above the cap of %d samples", (long long)p->w + p->t,
                 PT_MAX_SPAN);
    p->set_frames(p->w + p->t, hop == -1 ? fs / 100 : hop);
    p->g = PT_FRAMES;
    while (p->g > 1 && lds_need(p->g, p->pitch, p->n, p->t + 1) > PT_LDS_TARGET) p->g >>= 1;
    p->lds_bytes = lds_need(p->g, p->pitch, p->n, p->t + 1);
    p->threshold = 0.0;
    return L3AC_OK;
}

__device__ __forceinline__ int wave_min_int(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- the tracker: grid (runs of PT_GROUPS groups, batch) ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(PT_THREADS) void pitch_kernel(const float* __restrict__ audio, int64_t stride, int64_t max_samples,
                                                         const int* __restrict__ lens, PitchGeom p, int64_t f_max, double* __restrict__ f0,
                                                         int* __restrict__ voiced, double* __restrict__ aper, double* __restrict__ cmnd,
                                                         int* __restrict__ frames_out) {
    extern __shared__ __attribute__((aligned(16))) double lds_raw[];
    const int lags = p.t + 1;
    double* cm = lds_raw;                                               // [g][lags]: S, then c
    float* dd = reinterpret_cast<float*>(cm + (int64_t)p.g * lags);    // [g][lags]
    float* xs = dd + (int64_t)p.g * lags;                               // [(g - 1) pitch + span]: frame k of the group starts at k pitch
    const int b = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t frames = p.frames(lens ? lens[b] : max_samples);
    const float* x = audio + (int64_t)b * stride;
    const double nan = __builtin_nan("");
    if (frames_out && blockIdx.x == 0 && tid == 0) frames_out[b] = (int)frames;

    const int64_t run0 = (int64_t)blockIdx.x * (PT_GROUPS * p.g);
    float pre[PT_PRE];
    auto fetch = [&](int64_t t0) {  // the first samples that frame group t0 stages
        const int cnt = p.count(t0, frames);
        const int floats = cnt ? p.floats(cnt) : 0;
#pragma unroll
        for (int i = 0; i < PT_PRE; ++i) {
            const int k = tid + i * PT_THREADS;
            pre[i] = k < floats ? x[p.src(t0, k)] : 0.f;
        }
    };
    fetch(run0);
    for (int gi = 0; gi < PT_GROUPS; ++gi) {
        const int64_t t0 = run0 + (int64_t)gi * p.g;
        if (t0 >= f_max) break;  // (the whole workgroup)
        const int cnt = p.count(t0, frames);
        // rows at and after the clip's own frames
        for (int k = cnt + wave; k < p.g && t0 + k < f_max; k += PT_WAVES) {
            const int64_t row = (int64_t)b * f_max + t0 + k;
            if (lane == 0) f0[row] = nan, voiced[row] = 0, aper[row] = nan;
            if (cmnd)
                for (int tau = lane; tau < lags; tau += 64) cmnd[row * lags + tau] = nan;
        }
        if (cnt == 0) continue;  // (the whole workgroup; no later group of this clip has a frame either)
        const int floats = p.floats(cnt);
        __syncthreads();  // the previous group's reads of xs, dd and cm are over
#pragma unroll
        for (int i = 0; i < PT_PRE; ++i) {
            const int k = tid + i * PT_THREADS;
            if (k < floats) xs[k] = pre[i];
        }
        for (int k = PT_PRE * PT_THREADS + tid; k < floats; k += PT_THREADS) xs[k] = x[p.src(t0, k)];
        __syncthreads();
        if (gi + 1 < PT_GROUPS && t0 + p.g < f_max) fetch(t0 + p.g);

        // the difference function
        const int chunks = (lags + 63) >> 6;
        for (int item = wave; item < cnt * chunks; item += PT_WAVES) {
            const int k = item / chunks, tau = (item - k * chunks) * 64 + lane;
            const float* lo = xs + k * p.pitch;
            const float* hi = lo + min(tau, p.t);  // (a lane past the last lag rereads it and stores nothing)
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
            int j = 0;
            for (; j + 4 <= p.w; j += 4) {
                const float d0 = lo[j] - hi[j], d1 = lo[j + 1] - hi[j + 1], d2 = lo[j + 2] - hi[j + 2], d3 = lo[j + 3] - hi[j + 3];
                a0 = fmaf(d0, d0, a0);
                a1 = fmaf(d1, d1, a1);
                a2 = fmaf(d2, d2, a2);
                a3 = fmaf(d3, d3, a3);
            }
            if (j < p.w) {
                const float d0 = lo[j] - hi[j];
                a0 = fmaf(d0, d0, a0);
            }
            if (j + 1 < p.w) {
                const float d1 = lo[j + 1] - hi[j + 1];
                a1 = fmaf(d1, d1, a1);
            }
            if (j + 2 < p.w) {
                const float d2 = lo[j + 2] - hi[j + 2];
                a2 = fmaf(d2, d2, a2);
            }
            if (tau <= p.t) dd[k * lags + tau] = (a0 + a1) + (a2 + a3);
        }
        __syncthreads();

        // S(tau), in the order of tau; one lane per frame
        if (tid < cnt) {
            const float* d = dd + tid * lags;
            double* s = cm + tid * lags;
            double acc = 0.0;
            s[0] = 0.0;
            for (int tau = 1; tau < lags; ++tau) {
                acc = acc + (double)d[tau];
                s[tau] = acc;
            }
        }
        __syncthreads();
        for (int i = tid; i < cnt * lags; i += PT_THREADS) {
            const int k = i / lags, tau = i - k * lags;
            const double s = cm[i];
            const double c = (tau == 0 || s == 0.0) ? 1.0 : ((double)dd[i] * (double)tau) / s;
            cm[i] = c;
            if (cmnd) cmnd[((int64_t)b * f_max + t0 + k) * lags + tau] = c;
        }
        __syncthreads();

        // the pick and the refinement; one wave per frame
        for (int k = wave; k < cnt; k += PT_WAVES) {
            const double* c = cm + k * lags;
            int first = 0x7fffffff;
            for (int tau = p.tau_min + lane; tau <= p.tau_max; tau += 64)
                if (c[tau] < p.threshold) {
                    first = tau;
                    break;
                }
            first = wave_min_int(first);
            int star, is_voiced;
            if (first != 0x7fffffff) {
                is_voiced = 1;
                star = first;
                while (star + 1 <= p.tau_max && c[star + 1] < c[star]) ++star;
            } else {  // the first argmin: the smallest value, among equals the smallest lag
                is_voiced = 0;
                double best = __builtin_huge_val();
                int at = 0x7fffffff;
                for (int tau = p.tau_min + lane; tau <= p.tau_max; tau += 64)
                    if (c[tau] < best) best = c[tau], at = tau;
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) {
                    const double ob = __shfl_xor(best, o, 64);
                    const int oa = __shfl_xor(at, o, 64);
                    if (ob < best || (ob == best && oa < at)) best = ob, at = oa;
                }
                star = at == 0x7fffffff ? p.tau_min : at;  // (nothing below +inf in the range)
            }
            if (lane == 0) {
                const double a = c[star - 1], m = c[star], e = c[star + 1];  // tau_min >= 4 and tau_max + 1 = t: inside the row
                const double den = (a - 2.0 * m) + e;
                double shift = 0.0;
                if (den > 0.0) {
                    const double sh = (0.5 * (a - e)) / den;
                    if (fabs(sh) <= 1.0) shift = sh;
                }
                const int64_t row = (int64_t)b * f_max + t0 + k;
                f0[row] = (double)p.fs / ((double)star + shift);
                voiced[row] = is_voiced;
                aper[row] = m;
            }
        }
    }
}

// ---- the pair metrics: one workgroup per clip; the clips' frame counts (at most RaggedUpload::CAP, clips lens.offset ...) are arguments ----------
__global__ __launch_bounds__(PM_THREADS) void pitch_metrics_kernel(const double* __restrict__ f0_ref, const int* __restrict__ v_ref,
                                                                 const double* __restrict__ f0_est, const int* __restrict__ v_est,
                                                                 int64_t max_frames, int has_lens, RaggedUpload lens, double* __restrict__ out,
                                                                 int* __restrict__ counts) {
    __shared__ double lds[PM_THREADS / 64];
    const int b = lens.offset + blockIdx.x;
    const int64_t frames = has_lens ? lens.vals[blockIdx.x] : max_frames;
    const int64_t row = (int64_t)b * max_frames;
    double n_ref = 0.0, n_est = 0.0, n_both = 0.0, n_flip = 0.0, n_gross = 0.0, sq = 0.0;  // (whole numbers below 2^31: exact in any order)
    for (int64_t f = threadIdx.x; f < frames; f += PM_THREADS) {
        const bool vr = v_ref[row + f] != 0, ve = v_est[row + f] != 0;
        n_ref += vr, n_est += ve, n_flip += vr != ve;
        if (vr && ve) {
            const double ratio = f0_est[row + f] / f0_ref[row + f];
            const double cents = 1200.0 * log2(ratio);
            n_both += 1.0;
            n_gross += fabs(ratio - 1.0) > 0.2;
            sq += cents * cents;
        }
    }
    n_ref = block_sum<PM_THREADS>(n_ref, lds);
    n_est = block_sum<PM_THREADS>(n_est, lds);
    n_both = block_sum<PM_THREADS>(n_both, lds);
    n_flip = block_sum<PM_THREADS>(n_flip, lds);
    n_gross = block_sum<PM_THREADS>(n_gross, lds);
    sq = block_sum<PM_THREADS>(sq, lds);
    if (threadIdx.x == 0) {
        const double total = (double)frames;  // (0 / 0 is NaN: no frame, or no frame voiced on both sides)
        out[4 * (int64_t)b] = sqrt(sq / n_both);
        out[4 * (int64_t)b + 1] = n_gross / n_both;
        out[4 * (int64_t)b + 2] = n_flip / total;
        out[4 * (int64_t)b + 3] = (n_flip + n_gross) / total;
        counts[4 * (int64_t)b] = (int)frames;
        counts[4 * (int64_t)b + 1] = (int)n_ref;
        counts[4 * (int64_t)b + 2] = (int)n_est;
        counts[4 * (int64_t)b + 3] = (int)n_both;
    }
}

}  // namespace

extern "C" {

int l3ac_pitch_lags(int32_t sample_rate, double fmin, double fmax, int32_t window, int32_t hop, int32_t* out) {
    PitchGeom p;
    L3AC_TRY(pitch_geom(sample_rate, fmin, fmax, window, hop, &p));
    L3AC_REQUIRE(out, "pitch_lags: null out");
    out[0] = p.tau_min, out[1] = p.tau_max, out[2] = p.w, out[3] = p.hop, out[4] = p.n;
    return L3AC_OK;
}

int64_t l3ac_pitch_frames(int64_t samples, int32_t sample_rate, double fmin, double fmax, int32_t window, int32_t hop) {
    PitchGeom p;
    L3AC_TRY(pitch_geom(sample_rate, fmin, fmax, window, hop, &p));
    L3AC_REQUIRE(samples >= 0, "pitch_frames: samples %lld must not be negative", (long long)samples);
    return p.frames(samples);
}

int64_t l3ac_pitch_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sample_rate, double fmin, double fmax, int32_t window, int32_t hop) {
    PitchGeom p;
    L3AC_TRY(pitch_geom(sample_rate, fmin, fmax, window, hop, &p));
    L3AC_TRY(check_clip_batch("pitch", batch, max_samples));
    return ScratchPlan(batch).bytes;  // the clips' lengths
}

int l3ac_pitch(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, int32_t sample_rate,
               double fmin, double fmax, int32_t window, int32_t hop, double threshold, double* f0, int32_t* voiced, double* aperiodicity,
               double* cmnd, int32_t* frames, void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    PitchGeom p;
    L3AC_TRY(pitch_geom(sample_rate, fmin, fmax, window, hop, &p));
    L3AC_REQUIRE(threshold > 0.0 && threshold < 1.0, "pitch: threshold %g outside (0, 1)", threshold);
    p.threshold = threshold;
    L3AC_TRY(check_clip_batch("pitch", batch, max_samples));
    const int64_t f_max = p.frames(max_samples);
    L3AC_REQUIRE(audio, "pitch: null audio");
    L3AC_REQUIRE(f_max == 0 || (f0 && voiced && aperiodicity), "pitch: null output buffer");
    L3AC_REQUIRE(batch == 1 || audio_stride >= max_samples, "pitch: row stride %lld below max_samples %lld", (long long)audio_stride,
                 (long long)max_samples);
    L3AC_TRY(check_clip_lengths("pitch", samples, batch, max_samples));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "pitch", "pitch", samples, batch, scratch, scratch_bytes, ScratchPlan(batch).bytes, &lens));
    // (no frame anywhere: one workgroup per clip still writes the frame counts)
    const int64_t runs = std::max<int64_t>(ceil_div64(f_max, (int64_t)PT_GROUPS * p.g), 1);
    const double terms = (double)batch * (double)f_max * p.w * (p.t + 1);
    ProfScope prof(s, "pitch_kernel", 3.0 * terms, 4.0 * batch * (double)max_samples);
    hipLaunchKernelGGL(pitch_kernel, dim3((unsigned)runs, (unsigned)batch), dim3(PT_THREADS), (size_t)p.lds_bytes, s, audio, audio_stride, max_samples,
                       lens, p, f_max, f0, voiced, aperiodicity, f_max > 0 ? cmnd : nullptr, frames);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

int l3ac_pitch_metrics(const double* f0_ref, const int32_t* voiced_ref, const double* f0_est, const int32_t* voiced_est, int32_t batch,
                       int64_t max_frames, const int32_t* frames, double* out, int32_t* counts, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    L3AC_REQUIRE(batch > 0 && batch <= 65535, "pitch_metrics: batch %d outside 1..65535", batch);
    L3AC_REQUIRE(max_frames >= 0 && max_frames < ((int64_t)1 << 31), "pitch_metrics: max_frames %lld outside 0..2^31 - 1", (long long)max_frames);
    L3AC_REQUIRE(out && counts, "pitch_metrics: null output buffer");
    L3AC_REQUIRE(max_frames == 0 || (f0_ref && voiced_ref && f0_est && voiced_est), "pitch_metrics: null track");
    for (int i = 0; frames && i < batch; ++i)
        L3AC_REQUIRE(frames[i] >= 0 && frames[i] <= max_frames, "pitch_metrics: frames[%d] = %d outside [0, %lld]", i, frames[i], (long long)max_frames);
    return for_each_length_group(frames, batch, [&](const RaggedUpload& blk) -> int {
        ProfScope prof(s, "pitch_metrics_kernel", 0.0, 24.0 * blk.n * (double)max_frames);
        hipLaunchKernelGGL(pitch_metrics_kernel, dim3((unsigned)blk.n), dim3(PM_THREADS), 0, s, f0_ref, voiced_ref, f0_est, voiced_est, max_frames,
                           frames ? 1 : 0, blk, out, counts);
        L3AC_LAUNCH_CHECK();
        return L3AC_OK;
    });
}

}  // extern "C"
