// Short-time linear prediction of mono clips and the spectral-envelope measures of speech-codec evaluation on top of it: log-likelihood
// ratio, Itakura-Saito distance, LPC cepstral distance and segmental SNR (include/l3ac_hip.h, "linear prediction"; DESIGN.md §3.18, which
// is normative).  No reference counterpart.
//
//   lpc_frame_kernel   grid (groups of frames, batch), 4 waves.  A group is G consecutive frames of one clip (G = 16, halved until the group
//                      fits the LDS budget; a function of the parameters alone).  The group's samples of the one or two sides, (G - 1)
//                      min(hop, N) + N floats a side, and the window go to LDS once (stage_group of frame_groups.hpp, which owns the
//                      framing); the frames overlap, so every sample is read from memory once per group and up to N / hop times from
//                      LDS.  Then one wave per frame, the four waves in step:
//     autocorrelation  fp64 from here on.  xw[i] = (double)x[i] (double)w[i], exact.  For each lag k lane l sums the terms i = l, l + 64, ...
//                      of xw[i] xw[i + k] in increasing i from +0, and the 64 partial sums are folded s[l] += s[l + h], h = 32 .. 1: the
//                      reads of a term are consecutive across the lanes (no bank conflict), the order depends on N and k alone.  The
//                      noise energy sum (xw_r[i] - xw_e[i])^2 takes the same order; the signal energy IS r_r[0].
//     recursion        lane 0: Levinson-Durbin of each side on its r[0..p] in LDS, in the stated order; a frame is valid iff r[0] > 0
//                      and every E_m > 0
//     forms            pairs only.  Lane i: the inner sums sum_j r[|i - j|] a[j] of the three quadratic forms in increasing j; lane 0: the
//                      outer sums in increasing i, the cepstra of 1 / A, the four values and their clamps
//   lpc_pair_kernel    one workgroup per pair, built on the pair pieces of metric_common.hpp: the frames' values of a measure go to LDS
//                      (+inf where the frame is not valid on both sides, and up to the next power of two), a bitonic sort orders them —
//                      the sorted sequence of a set of numbers does not depend on how it was reached — and lane 0 sums the first
//                      k = floor(trim V + 0.5) in that order (lds_trimmed_mean).  16384 fp64 values are 128 KiB of the CU's 160 KiB of
//                      LDS: this is what caps a pair at 16384 frames.  The segmental SNR is the sum of the counted frames' values in
//                      frame order over their count (lds_ordered_mean).
//
// A frame's values depend on its own N samples a side only — never on the batch, the clip's row, the row stride, the scratch size, the
// frame's place in its group or what lies after the clip's length, which is never read; no atomics.  Non-finite samples make unspecified
// values in the frames that read them, and in their pair's means; every index is bounded by the parameters, whatever the values.
//
// Contraction is off for this whole file: every product and sum rounds on its own, in the order DESIGN.md states.
#include "frame_groups.hpp"
#include "metric_common.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int LP_THREADS = 256;
constexpr int LP_WAVES = LP_THREADS / 64;
constexpr int LP_FRAMES = 16;            // frames of a group at most
constexpr int LP_MAX_ORDER = 32;
constexpr int LP_ROW = LP_MAX_ORDER + 1;  // r[0..p], a[0..p]
constexpr int LP_MAX_FRAME = 8192;
constexpr int LP_MIN_RATE = 8000, LP_MAX_RATE = 192000;
constexpr int LP_LDS_TARGET = 48 << 10;  // a group of more than one frame stays below this: three workgroups per CU
// a wave's rows of LP_ROW doubles in LDS: r, a, reflection and cepstrum of each side, a spare row, the three forms' inner sums
enum { W_R0 = 0, W_R1, W_A0, W_A1, W_K0, W_K1, W_C0, W_C1, W_TMP, W_Q0, W_Q1, W_Q2, W_ROWS };
constexpr int LP_WORK = W_ROWS * LP_ROW;  // doubles per wave
constexpr int LP_LDS_MAX = LP_WAVES * LP_WORK * 8 + 3 * LP_MAX_FRAME * 4;  // one frame of 8192 samples, two sides and the window
constexpr double LP_DB = 4.342944819032518;  // 10 / ln 10
static_assert(LP_LDS_MAX <= 160 * 1024, "a group lives in one workgroup's LDS");

struct LpcGeom : FrameGroups {
    int p, lds_bytes;  // order, dynamic LDS of the launch
};

struct LpcClamp {
    double trim, llr_max, is_max, cd_max;
};

int lds_need(int g, int pitch, int n) { return LP_WAVES * LP_WORK * 8 + n * 4 + 2 * ((g - 1) * pitch + n) * 4; }

int lpc_geom(int32_t fs, int32_t order, int32_t frame, int32_t hop, LpcGeom* p) {
    L3AC_REQUIRE(fs >= LP_MIN_RATE && fs <= LP_MAX_RATE, "lpc: sample_rate %d outside %d..%d", fs, LP_MIN_RATE, LP_MAX_RATE);
    L3AC_REQUIRE(order >= 1 && order <= LP_MAX_ORDER, "lpc: order %d outside 1..%d", order, LP_MAX_ORDER);
    L3AC_REQUIRE(frame > order && frame <= LP_MAX_FRAME, "lpc: frame %d outside order + 1 = %d .. %d", frame, order + 1, LP_MAX_FRAME);
    L3AC_REQUIRE(hop >= 1, "lpc: hop %d must be at least 1", hop);
    p->set_frames(frame, hop), p->p = order;
    p->g = LP_FRAMES;
    while (p->g > 1 && lds_need(p->g, p->pitch, frame) > LP_LDS_TARGET) p->g >>= 1;
    p->lds_bytes = lds_need(p->g, p->pitch, frame);
    return L3AC_OK;
}

// Levinson-Durbin on r[0..p] -> a[0..p], refl[0..p-1], *err = E_p; false where r[0] > 0 or an E_m > 0 fails (the arrays are then partial)
__device__ bool levinson(const double* r, double* a, double* tmp, double* refl, int p, double* err) {
    if (!(r[0] > 0.0)) return false;
    a[0] = 1.0;
    double e = r[0];
    for (int m = 1; m <= p; ++m) {
        double acc = r[m];
        for (int i = 1; i < m; ++i) acc = acc + a[i] * r[m - i];
        const double km = -acc / e;
        for (int i = 1; i < m; ++i) tmp[i] = a[i] + km * a[m - i];
        for (int i = 1; i < m; ++i) a[i] = tmp[i];
        a[m] = km;
        refl[m - 1] = km;
        e = e * (1.0 - km * km);
        if (!(e > 0.0)) return false;
    }
    *err = e;
    return true;
}

// cepstrum of 1 / A: c[1..p]
__device__ void cepstrum(const double* a, double* c, int p) {
    c[1] = -a[1];
    for (int m = 2; m <= p; ++m) {
        double s = 0.0;
        for (int k = 1; k < m; ++k) s = s + (((double)k / (double)m) * c[k]) * a[m - k];
        c[m] = -a[m] - s;
    }
}

// ---- the frames: grid (groups, batch).  est == nullptr: one side (l3ac_lpc), else a pair (l3ac_lpc_metrics) ----------------------------------
__global__ __launch_bounds__(LP_THREADS) void lpc_frame_kernel(const float* __restrict__ ref, int64_t ref_stride, const float* __restrict__ est,
                                                             int64_t est_stride, int64_t max_samples, const int* __restrict__ lens,
                                                             const float* __restrict__ window, LpcGeom p, LpcClamp cl, int64_t f_max,
                                                             double* __restrict__ out_a, double* __restrict__ out_k, double* __restrict__ out_e,
                                                             double* __restrict__ out_r, int* __restrict__ out_valid, int* __restrict__ frames_out,
                                                             double* __restrict__ vals, double* __restrict__ forms, int* __restrict__ flags) {
    extern __shared__ __attribute__((aligned(16))) double lds_raw[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y;
    const int n_frame = p.n, order = p.p, rows = order + 1;
    double* work = lds_raw + wave * LP_WORK;
    float* win = reinterpret_cast<float*>(lds_raw + LP_WAVES * LP_WORK);  // [n]
    float* xs0 = win + n_frame;                                           // [span_max]: frame k of the group starts at k pitch
    float* xs1 = xs0 + p.span_max();
    const bool pair = est != nullptr;
    const int64_t frames = p.frames(lens ? lens[b] : max_samples);
    const double nan = __builtin_nan("");
    if (frames_out && blockIdx.x == 0 && tid == 0) frames_out[b] = (int)frames;

    const int64_t t0 = (int64_t)blockIdx.x * p.g;
    if (t0 >= f_max) return;  // (the one workgroup of a batch without any frame)
    const int cnt = p.count(t0, frames);
    // rows at and after the clip's own frames
    for (int k = cnt + wave; k < p.g && t0 + k < f_max; k += LP_WAVES) {
        const int64_t row = (int64_t)b * f_max + t0 + k;
        if (!pair) {
            if (lane == 0) out_e[row] = nan, out_valid[row] = 0;
            if (lane < rows) out_a[row * rows + lane] = nan, out_r[row * rows + lane] = nan;
            if (lane < order) out_k[row * order + lane] = nan;
        } else {
            if (lane < 4) vals[row * 4 + lane] = nan;
            if (lane == 0) flags[row] = 0;
            if (forms && lane < 5) forms[row * 5 + lane] = nan;
        }
    }
    if (cnt == 0) return;  // (the whole workgroup)

    stage_group<LP_THREADS>(p, t0, cnt, ref + (int64_t)b * ref_stride, pair ? est + (int64_t)b * est_stride : nullptr, xs0, xs1);
    stage_window<LP_THREADS>(n_frame, window, win);
    __syncthreads();

    for (int k0 = 0; k0 < cnt; k0 += LP_WAVES) {  // the four waves in step: every barrier below is reached by all of them
        const int k = k0 + wave;
        const bool active = k < cnt;
        const int64_t row = (int64_t)b * f_max + t0 + k;
        const float* f0 = xs0 + (active ? k : 0) * p.pitch;
        const float* f1 = xs1 + (active ? k : 0) * p.pitch;
        for (int side = 0; side < (pair ? 2 : 1); ++side) {
            const float* x = side ? f1 : f0;
            for (int kk = 0; kk <= order; ++kk) {
                double s = 0.0;
                for (int i = lane; i + kk < n_frame; i += 64) {
                    const double u = (double)x[i] * (double)win[i], v = (double)x[i + kk] * (double)win[i + kk];
                    s = s + u * v;
                }
                s = fold64(s);
                if (lane == 0) work[(W_R0 + side) * LP_ROW + kk] = s;
            }
        }
        double noise = 0.0;
        if (pair) {
            for (int i = lane; i < n_frame; i += 64) {
                const double d = (double)f0[i] * (double)win[i] - (double)f1[i] * (double)win[i];
                noise = noise + d * d;
            }
            noise = fold64(noise);
        }
        __syncthreads();
        bool ok0 = false, ok1 = false;
        double e0 = nan, e1 = nan;
        if (lane == 0 && active) {
            ok0 = levinson(work + W_R0 * LP_ROW, work + W_A0 * LP_ROW, work + W_TMP * LP_ROW, work + W_K0 * LP_ROW, order, &e0);
            if (pair) ok1 = levinson(work + W_R1 * LP_ROW, work + W_A1 * LP_ROW, work + W_TMP * LP_ROW, work + W_K1 * LP_ROW, order, &e1);
        }
        ok0 = __shfl(ok0 ? 1 : 0, 0, 64) != 0;
        ok1 = __shfl(ok1 ? 1 : 0, 0, 64) != 0;
        __syncthreads();
        if (!pair) {
            if (active) {
                if (lane == 0) out_e[row] = ok0 ? e0 : nan, out_valid[row] = ok0 ? 1 : 0;
                if (lane < rows) {
                    out_r[row * rows + lane] = work[W_R0 * LP_ROW + lane];
                    out_a[row * rows + lane] = ok0 ? work[W_A0 * LP_ROW + lane] : nan;
                }
                if (lane < order) out_k[row * order + lane] = ok0 ? work[W_K0 * LP_ROW + lane] : nan;
            }
            __syncthreads();  // the rows are read before the next frame overwrites them
            continue;
        }
        const bool both = ok0 && ok1;
        if (active && both && lane < rows) {  // the inner sums of num = q(a_e, r_r), g_r = q(a_r, r_r), g_e = q(a_e, r_e)
            const double *r0 = work + W_R0 * LP_ROW, *r1 = work + W_R1 * LP_ROW, *a0 = work + W_A0 * LP_ROW, *a1 = work + W_A1 * LP_ROW;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0;
            for (int j = 0; j < rows; ++j) {
                const int d = lane > j ? lane - j : j - lane;
                s0 = s0 + r0[d] * a1[j];
                s1 = s1 + r0[d] * a0[j];
                s2 = s2 + r1[d] * a1[j];
            }
            work[W_Q0 * LP_ROW + lane] = s0, work[W_Q1 * LP_ROW + lane] = s1, work[W_Q2 * LP_ROW + lane] = s2;
        }
        __syncthreads();
        if (active && lane == 0) {
            const double sig = work[W_R0 * LP_ROW];
            double num = nan, g_r = nan, g_e = nan, llr = nan, is = nan, cd = nan, snr = nan;
            if (both) {
                const double *a0 = work + W_A0 * LP_ROW, *a1 = work + W_A1 * LP_ROW;
                double *c0 = work + W_C0 * LP_ROW, *c1 = work + W_C1 * LP_ROW;
                num = 0.0, g_r = 0.0, g_e = 0.0;
                for (int i = 0; i < rows; ++i) {
                    num = num + a1[i] * work[W_Q0 * LP_ROW + i];
                    g_r = g_r + a0[i] * work[W_Q1 * LP_ROW + i];
                    g_e = g_e + a1[i] * work[W_Q2 * LP_ROW + i];
                }
                const double ratio = num / g_r;
                llr = clamp_to(log(ratio), 0.0, cl.llr_max);
                is = clamp_to(((g_r / g_e) * ratio + log(g_e / g_r)) - 1.0, 0.0, cl.is_max);
                cepstrum(a0, c0, order);
                cepstrum(a1, c1, order);
                double sq = 0.0;
                for (int m = 1; m <= order; ++m) {
                    const double d = c0[m] - c1[m];
                    sq = sq + d * d;
                }
                cd = clamp_to(LP_DB * sqrt(2.0 * sq), 0.0, cl.cd_max);
            }
            const bool counted = sig > 0.0;
            if (counted) snr = noise == 0.0 ? 35.0 : clamp_to(10.0 * log10(sig / noise), -10.0, 35.0);
            vals[row * 4] = llr, vals[row * 4 + 1] = is, vals[row * 4 + 2] = cd, vals[row * 4 + 3] = snr;
            flags[row] = (both ? 1 : 0) | (counted ? 2 : 0);
            if (forms) forms[row * 5] = num, forms[row * 5 + 1] = g_r, forms[row * 5 + 2] = g_e, forms[row * 5 + 3] = sig, forms[row * 5 + 4] = noise;
        }
        __syncthreads();  // the rows are read before the next frame overwrites them
    }
}

// ---- the pair: one workgroup per pair -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PAIR_THREADS) void lpc_pair_kernel(const double* __restrict__ vals, const int* __restrict__ flags, int64_t f_max,
                                                            int64_t max_samples, const int* __restrict__ lens, LpcGeom p, LpcClamp cl,
                                                            double* __restrict__ out, int* __restrict__ counts) {
    __shared__ double buf[PAIR_MAX_FRAMES];
    __shared__ unsigned char fl[PAIR_MAX_FRAMES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int frames = pair_frames(p.frames(lens ? lens[b] : max_samples), f_max);
    const double* row = vals + (int64_t)b * f_max * 4;
    int both = 0;  // the frames valid on both sides in the low half, the frames counted for the segmental SNR in the high half: 16384 at most each
    for (int f = tid; f < frames; f += PAIR_THREADS) {
        const int g = flags[(int64_t)b * f_max + f];
        fl[f] = (unsigned char)g;
        both += (g & 1) + ((g & 2) << 15);
    }
    both = block_count<PAIR_THREADS>(both);
    const int v_lpc = both & 0xffff, v_snr = both >> 16;
    const int keep = (int)floor(cl.trim * (double)v_lpc + 0.5);
    const double nan = __builtin_nan("");
    for (int m = 0; m < 3; ++m) {  // the three envelope measures over the frames valid on both sides
        const double mean = lds_trimmed_mean<PAIR_THREADS>(buf, frames, keep, [&](int f) { return row[f * 4 + m]; }, [&](int f) { return fl[f] & 1; });
        if (tid == 0) out[(int64_t)b * 4 + m] = (v_lpc == 0 || keep == 0) ? nan : mean;
    }
    const double snr = lds_ordered_mean<PAIR_THREADS>(buf, frames, v_snr, [&](int f) { return row[f * 4 + 3]; }, [&](int f) { return fl[f] & 2; });
    if (tid == 0) {
        out[(int64_t)b * 4 + 3] = snr;
        counts[(int64_t)b * 3] = frames, counts[(int64_t)b * 3 + 1] = v_lpc, counts[(int64_t)b * 3 + 2] = v_snr;
    }
}

int configure_frame_kernel() {
    static PerDeviceOnce configured;
    return raise_dynamic_lds(configured, {{lpc_frame_kernel, LP_LDS_MAX}});
}

// the parameters checked, then the frames' four values [batch][F][4] fp64 and the frames' flags [batch][F] int32
int lpc_metrics_scratch(int32_t batch, int64_t max_samples, int32_t sample_rate, int32_t order, int32_t frame, int32_t hop, LpcGeom* p,
                        PairScratch* sc) {
    L3AC_TRY(lpc_geom(sample_rate, order, frame, hop, p));
    L3AC_TRY(check_clip_batch("lpc", batch, max_samples));
    ScratchPlan plan(batch);
    L3AC_TRY(pair_frames_plan("lpc_metrics", batch, p->frames(max_samples), 32, plan, &sc->vals, &sc->flags));
    sc->need = plan.bytes;
    return L3AC_OK;
}

}  // namespace

extern "C" {

int64_t l3ac_lpc_window(int32_t frame, float* out, int64_t cap) {
    L3AC_REQUIRE(frame >= 2 && frame <= LP_MAX_FRAME, "lpc_window: frame %d outside 2..%d", frame, LP_MAX_FRAME);
    if (!out || cap < frame) return frame;
    for (int i = 0; i < frame; ++i) out[i] = (float)(0.5 * (1.0 - std::cos(2.0 * M_PI * (double)(i + 1) / (double)(frame + 1))));
    return frame;
}

int l3ac_lpc_defaults(int32_t sample_rate, int32_t* out) {
    L3AC_REQUIRE(sample_rate >= LP_MIN_RATE && sample_rate <= LP_MAX_RATE, "lpc: sample_rate %d outside %d..%d", sample_rate, LP_MIN_RATE, LP_MAX_RATE);
    L3AC_REQUIRE(out, "lpc_defaults: null out");
    const int frame = (int)((30 * (int64_t)sample_rate + 500) / 1000);
    out[0] = sample_rate < 10000 ? 10 : 16, out[1] = frame, out[2] = frame / 4;
    return L3AC_OK;
}

int64_t l3ac_lpc_frames(int64_t samples, int32_t frame, int32_t hop) {
    L3AC_REQUIRE(samples >= 0, "lpc_frames: samples %lld must not be negative", (long long)samples);
    L3AC_REQUIRE(frame >= 2 && frame <= LP_MAX_FRAME, "lpc_frames: frame %d outside 2..%d", frame, LP_MAX_FRAME);
    L3AC_REQUIRE(hop >= 1, "lpc_frames: hop %d must be at least 1", hop);
    return uncentred_frames(samples, frame, hop);
}

int64_t l3ac_lpc_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sample_rate, int32_t order, int32_t frame, int32_t hop) {
    LpcGeom p;
    L3AC_TRY(lpc_geom(sample_rate, order, frame, hop, &p));
    L3AC_TRY(check_clip_batch("lpc", batch, max_samples));
    return ScratchPlan(batch).bytes;  // the clips' lengths
}

int l3ac_lpc(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, int32_t sample_rate, int32_t order,
             int32_t frame, int32_t hop, const float* window, double* a, double* reflection, double* error, double* autocorr, int32_t* valid,
             int32_t* frames, void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    LpcGeom p;
    L3AC_TRY(lpc_geom(sample_rate, order, frame, hop, &p));
    L3AC_TRY(check_clip_batch("lpc", batch, max_samples));
    const int64_t f_max = p.frames(max_samples);
    L3AC_REQUIRE(audio, "lpc: null audio");
    L3AC_REQUIRE(f_max == 0 || (a && reflection && error && autocorr && valid), "lpc: null output buffer");
    L3AC_REQUIRE(batch == 1 || audio_stride >= max_samples, "lpc: row stride %lld below max_samples %lld", (long long)audio_stride,
                 (long long)max_samples);
    L3AC_TRY(check_clip_lengths("lpc", samples, batch, max_samples));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "lpc", "lpc", samples, batch, scratch, scratch_bytes, ScratchPlan(batch).bytes, &lens));
    L3AC_TRY(configure_frame_kernel());
    // (no frame anywhere: one workgroup per clip still writes the frame counts)
    const int64_t groups = std::max<int64_t>(ceil_div64(f_max, p.g), 1);
    ProfScope prof(s, "lpc_frame_kernel", 2.0 * batch * (double)f_max * frame * (order + 1), 4.0 * batch * (double)max_samples);
    hipLaunchKernelGGL(lpc_frame_kernel, dim3((unsigned)groups, (unsigned)batch), dim3(LP_THREADS), (size_t)p.lds_bytes, s, audio, audio_stride,
                       (const float*)nullptr, (int64_t)0, max_samples, lens, window, p, LpcClamp{}, f_max, a, reflection, error, autocorr, valid, frames,
                       (double*)nullptr, (double*)nullptr, (int*)nullptr);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

int64_t l3ac_lpc_metrics_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sample_rate, int32_t order, int32_t frame, int32_t hop) {
    LpcGeom p;
    PairScratch sc;
    L3AC_TRY(lpc_metrics_scratch(batch, max_samples, sample_rate, order, frame, hop, &p, &sc));
    return sc.need;
}

int l3ac_lpc_metrics(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples,
                     const int32_t* samples, int32_t sample_rate, int32_t order, int32_t frame, int32_t hop, const float* window, double trim,
                     double llr_max, double is_max, double cd_max, double* out, int32_t* counts, double* frame_values, double* forms, void* scratch,
                     int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    LpcGeom p;
    PairScratch sc;
    L3AC_TRY(lpc_metrics_scratch(batch, max_samples, sample_rate, order, frame, hop, &p, &sc));
    L3AC_REQUIRE(trim > 0.0 && trim <= 1.0, "lpc_metrics: trim %g outside (0, 1]", trim);
    L3AC_REQUIRE(llr_max >= 0.0 && std::isfinite(llr_max), "lpc_metrics: llr_max %g must be finite and not negative", llr_max);
    L3AC_REQUIRE(is_max >= 0.0 && std::isfinite(is_max), "lpc_metrics: is_max %g must be finite and not negative", is_max);
    L3AC_REQUIRE(cd_max >= 0.0 && std::isfinite(cd_max), "lpc_metrics: cd_max %g must be finite and not negative", cd_max);
    L3AC_REQUIRE(ref && est, "lpc_metrics: null audio");
    L3AC_REQUIRE(out && counts, "lpc_metrics: null output buffer");
    L3AC_REQUIRE(batch == 1 || (ref_stride >= max_samples && est_stride >= max_samples), "lpc_metrics: row stride below max_samples %lld",
                 (long long)max_samples);
    L3AC_TRY(check_clip_lengths("lpc_metrics", samples, batch, max_samples));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "lpc_metrics", "lpc_metrics", samples, batch, scratch, scratch_bytes, sc.need, &lens));
    const int64_t f_max = p.frames(max_samples);
    char* base = static_cast<char*>(scratch);
    double* vals = frame_values ? frame_values : reinterpret_cast<double*>(base + sc.vals);
    int* flags = reinterpret_cast<int*>(base + sc.flags);
    const LpcClamp cl{trim, llr_max, is_max, cd_max};
    if (f_max > 0) {
        L3AC_TRY(configure_frame_kernel());
        ProfScope prof(s, "lpc_frame_kernel", 4.0 * batch * (double)f_max * frame * (order + 1), 8.0 * batch * (double)max_samples);
        hipLaunchKernelGGL(lpc_frame_kernel, dim3((unsigned)ceil_div64(f_max, p.g), (unsigned)batch), dim3(LP_THREADS), (size_t)p.lds_bytes, s, ref,
                           ref_stride, est, est_stride, max_samples, lens, window, p, cl, f_max, (double*)nullptr, (double*)nullptr, (double*)nullptr,
                           (double*)nullptr, (int*)nullptr, (int*)nullptr, vals, forms, flags);
        L3AC_LAUNCH_CHECK();
    }
    ProfScope prof(s, "lpc_pair_kernel", 0.0, 36.0 * batch * (double)f_max);
    hipLaunchKernelGGL(lpc_pair_kernel, dim3((unsigned)batch), dim3(PAIR_THREADS), 0, s, vals, flags, f_max, max_samples, lens, p, cl, out, counts);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

}  // extern "C"
