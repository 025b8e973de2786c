// Quality metrics on the device: STFT, log-mel spectrogram, log-mel distance, and MSE / SNR / SI-SDR (include/l3ac_hip.h, "quality
// metrics").  No reference counterpart: the reference's demo ends with ((x - y) ** 2).mean().
//
// STFT of torch.stft(x, n_fft, hop, n_fft, hann_window(n_fft), center=True, pad_mode="constant", onesided=True): frame f of a clip covers
// samples [f hop - n_fft/2, f hop + n_fft/2), zeros outside the clip, F(n) = 1 + n / hop frames.  The DFT is ONE product on the exact fp32
// matrix pipe (launch_gemm, no w_img): the clips are staged as rows of a scratch buffer — n_fft/2 zeros, the clip's own samples, zeros up
// to the row pitch P, a multiple of hop — and read as overlapping GEMM rows with lda = hop, so slot row g = clip * (P / hop) + f is frame f
// of that clip at base + g * hop, whatever the batch.  W is the window-folded basis [n_fft + 2][n_fft] (row 2k: w cos, row 2k + 1:
// -w sin, designed on the host in fp64, rounded once to fp32), and every output is launch_gemm's k-ordered fp32 chain: its bits do not
// depend on m, i.e. on the batch, the clip's row, or how many slot rows one product takes.  The slot rows after a clip's own F(n) frames
// (they run into the next clip's row) are computed with the rest of their panel and never stored anywhere.
// The slot rows are walked in groups that fit the spectrum scratch [G][n_fft + 4]; each group's spectra are consumed at once:
//   stft      metrics_scatter_kernel copies the valid rows into the caller's [batch][F][n_fft/2 + 1][2]
//   log_mel   metrics_mel_kernel: power, the triangular mel sum as one fmaf chain per filter over its run of bins (increasing k, from
//             +0), log10 of the value clamped at 1e-10
//   distance  the same kernel on both signals' spectra; |L_ref - L_est| in fp64, summed per frame in a fixed order (per lane over
//             filters lane, lane + 64, ..., then a xor tree) into frame_sum[clip][f]; metrics_mean_kernel sums a clip's frames in a
//             fixed order.  No atomics: nothing depends on the group size or on the batch.
// signal_metrics_kernel: one workgroup per clip, two fp64 passes with fixed per-thread strides and a fixed tree.
#include "metric_common.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr int MT_THREADS = 256;
constexpr int MT_MAX_MELS = 256;
constexpr int MT_MIN_GROUP = 128;  // slot rows per product at the minimum scratch: one GEMM row panel
constexpr int SM_THREADS = 1024;

struct MelGeom {
    int batch, n_fft, hop, bins, n_mels;
    int64_t max_samples, pitch, slots, frames;  // pitch P (floats) of a staged row, slots = P / hop, frames = F(max_samples)
    int64_t rows;                               // slot rows that hold a valid frame of some clip: (batch - 1) slots + frames
    int64_t spec_ld;                            // n_fft + 4: 16-byte rows
};

struct MelScratch {  // byte offsets into the caller's scratch, after the clips' lengths
    int64_t runs, frame_sum, stage, spec, total_min;
};

int mel_geom(int32_t batch, int64_t max_samples, int32_t n_fft, int32_t hop, int32_t n_mels, bool mels, MelGeom* g, MelScratch* sc) {
    L3AC_REQUIRE(n_fft >= 16 && n_fft <= 2048 && n_fft % 16 == 0, "metrics: n_fft %d must be a multiple of 16 in 16..2048", n_fft);
    L3AC_REQUIRE(hop >= 4 && hop <= n_fft && hop % 4 == 0, "metrics: hop %d must be a multiple of 4 in 4..n_fft (%d)", hop, n_fft);
    if (mels) L3AC_REQUIRE(n_mels >= 1 && n_mels <= MT_MAX_MELS, "metrics: n_mels %d outside 1..%d", n_mels, MT_MAX_MELS);
    L3AC_REQUIRE(batch > 0 && batch <= 65535 && max_samples > 0, "metrics: batch %d outside 1..65535 or no samples (%lld)", batch,
                 (long long)max_samples);
    L3AC_REQUIRE(max_samples < ((int64_t)1 << 31) - 4096, "metrics: clips of %lld samples are too long", (long long)max_samples);
    g->batch = batch;
    g->n_fft = n_fft;
    g->hop = hop;
    g->bins = n_fft / 2 + 1;
    g->n_mels = n_mels;
    g->max_samples = max_samples;
    g->frames = 1 + max_samples / hop;
    // the last frame of the longest clip starts at (max / hop) hop and reads n_fft floats of its own row
    g->pitch = (max_samples / hop) * hop + round_up64(n_fft, hop);
    g->slots = g->pitch / hop;
    g->rows = (int64_t)(batch - 1) * g->slots + g->frames;
    g->spec_ld = n_fft + 4;
    L3AC_REQUIRE(g->rows < ((int64_t)1 << 31), "metrics: %lld frame rows in one call (batch %d) exceed 2^31", (long long)g->rows, batch);
    ScratchPlan plan(batch);
    sc->runs = plan.take((int64_t)MT_MAX_MELS * 8);
    sc->frame_sum = plan.take((int64_t)batch * g->frames * 8);
    sc->stage = plan.take(2 * (int64_t)batch * g->pitch * 4);
    sc->spec = plan.last(2 * std::min<int64_t>(MT_MIN_GROUP, g->rows) * g->spec_ld * 4);
    sc->total_min = plan.bytes;
    return L3AC_OK;
}

// ---- staging: clip rows [batch][pitch] = n_fft/2 zeros ++ the clip's own samples ++ zeros ------------------------------------------
// grid (quads of a row / 256, batch, signals)
__global__ __launch_bounds__(MT_THREADS) void metrics_stage_kernel(const float* __restrict__ x0, int64_t stride0, const float* __restrict__ x1,
                                                                 int64_t stride1, const int* __restrict__ lens, float* __restrict__ stage,
                                                                 MelGeom g) {
    const int b = blockIdx.y;
    const float* x = (blockIdx.z ? x1 : x0) + (int64_t)b * (blockIdx.z ? stride1 : stride0);
    float* row = stage + ((int64_t)blockIdx.z * g.batch + b) * g.pitch;
    const int64_t n = lens ? lens[b] : g.max_samples;
    const int64_t half = g.n_fft / 2;
    const int64_t q = (int64_t)blockIdx.x * MT_THREADS + threadIdx.x;
    if (4 * q >= g.pitch) return;  // (pitch is a multiple of 4)
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t i = 4 * q + j - half;
        v[j] = (i >= 0 && i < n) ? x[i] : 0.f;
    }
    *reinterpret_cast<float4*>(row + 4 * q) = make_float4(v[0], v[1], v[2], v[3]);
}

// ---- each filter's run of bins [lo, hi): first to last non-zero weight (hi = lo = 0 for an empty filter) ---------------------------------
__global__ __launch_bounds__(MT_THREADS) void metrics_runs_kernel(const float* __restrict__ w, int n_mels, int bins, int2* __restrict__ runs) {
    const int m = blockIdx.x * MT_THREADS + threadIdx.x;
    if (m >= n_mels) return;
    int lo = 0, hi = 0;
    bool any = false;
    for (int k = 0; k < bins; ++k) {
        if (w[(int64_t)m * bins + k] != 0.f) {
            if (!any) lo = k;
            any = true;
            hi = k + 1;
        }
    }
    runs[m] = make_int2(lo, hi);
}

// whether slot row `row` is a frame of a clip, and which
__device__ __forceinline__ bool slot_frame(const MelGeom& g, const int* __restrict__ lens, int64_t row, int& clip, int& f) {
    clip = (int)((uint32_t)row / (uint32_t)g.slots);
    f = (int)((uint32_t)row % (uint32_t)g.slots);
    if (clip >= g.batch) return false;
    const int n = lens ? lens[clip] : (int)g.max_samples;
    return f < 1 + n / g.hop;
}

// ---- spectra of a group [grid][spec_ld] -> the caller's [batch][frames][bins][2]: valid rows only (the rest was zeroed) --------------------
__global__ __launch_bounds__(MT_THREADS) void metrics_scatter_kernel(const float* __restrict__ spec, int64_t row0, const int* __restrict__ lens,
                                                                   float* __restrict__ out, MelGeom g) {
    const int64_t row = row0 + blockIdx.x;
    int clip, f;
    if (!slot_frame(g, lens, row, clip, f)) return;
    const float* src = spec + (int64_t)blockIdx.x * g.spec_ld;
    float* dst = out + ((int64_t)clip * g.frames + f) * (2 * g.bins);
    for (int e = threadIdx.x; e < 2 * g.bins; e += MT_THREADS) dst[e] = src[e];
}

// ---- spectrum -> log-mel: one wave per slot row, four rows per workgroup ----------------------------------------------------------------
// The row's n_fft + 2 floats are read as 16-byte quads (two bins each) into the wave's own LDS strip as powers; lane l then owns filters
// l, l + 64, ..., each one fmaf chain over its run of bins.  out != null: the cells go to out[clip][f][n_mels]; else spec1 holds the second
// signal's spectra and the fp64 sum of |L0 - L1| over the frame's filters goes to frame_sum[clip][f].
constexpr int MEL_ROWS = 4;
constexpr int MEL_PMAX = 1028;  // bins <= 1025, rounded to quads

__device__ __forceinline__ float mel_cell(const float* __restrict__ p, const float* __restrict__ w, int2 run) {
    float acc = 0.f;
    for (int k = run.x; k < run.y; ++k) acc = fmaf(w[k], p[k], acc);
    // log10(max(M, 1e-10)): at or below the clamp the value is log10(1e-10) = -10 exactly
    return acc <= 1e-10f ? -10.f : log10f(acc);
}

__global__ __launch_bounds__(MT_THREADS) void metrics_mel_kernel(const float* __restrict__ spec0, const float* __restrict__ spec1, int64_t row0,
                                                               int count, const int* __restrict__ lens, const float* __restrict__ weights,
                                                               const int2* __restrict__ runs, float* __restrict__ out,
                                                               double* __restrict__ frame_sum, MelGeom g) {
    __shared__ __attribute__((aligned(16))) float pw[2][MEL_ROWS][MEL_PMAX];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = blockIdx.x * MEL_ROWS + wave;
    int clip = 0, f = 0;
    const bool valid = r < count && slot_frame(g, lens, row0 + r, clip, f);  // (wave-uniform)
    const int quads = (g.n_fft + 4) / 4;  // the row's n_fft + 2 floats and two of padding, never used
    const int n_sig = out ? 1 : 2;
    for (int s = 0; valid && s < n_sig; ++s) {
        const float4* src = reinterpret_cast<const float4*>((s ? spec1 : spec0) + (int64_t)r * g.spec_ld);
        for (int q = lane; q < quads; q += 64) {
            const float4 v = src[q];
            // re^2 + im^2, two roundings; one 8-byte LDS write per quad; bin 2q + 1 <= n_fft/2 + 1 < MEL_PMAX
            *reinterpret_cast<float2*>(&pw[s][wave][2 * q]) = make_float2(fmaf(v.x, v.x, v.y * v.y), fmaf(v.z, v.z, v.w * v.w));
        }
    }
    __syncthreads();
    if (!valid) return;
    double sum = 0.0;
    for (int m = lane; m < g.n_mels; m += 64) {
        const int2 run = runs[m];
        const float* w = weights + (int64_t)m * g.bins;
        const float l0 = mel_cell(pw[0][wave], w, run);
        if (out) {
            out[((int64_t)clip * g.frames + f) * g.n_mels + m] = l0;
        } else {
            const float l1 = mel_cell(pw[1][wave], w, run);
            sum += fabs((double)l0 - (double)l1);
        }
    }
    if (!out) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, 64);
        if (lane == 0) frame_sum[(int64_t)clip * g.frames + f] = sum;
    }
}

// ---- a clip's distance: the mean of its F(n) frame sums over F(n) n_mels cells; one workgroup per clip ------------------------------------
__global__ __launch_bounds__(MT_THREADS) void metrics_mean_kernel(const double* __restrict__ frame_sum, const int* __restrict__ lens,
                                                                double* __restrict__ out, MelGeom g) {
    __shared__ double lds[MT_THREADS / 64];
    const int b = blockIdx.x;
    const int n = lens ? lens[b] : (int)g.max_samples;
    const int frames = 1 + n / g.hop;
    double v = 0.0;
    for (int f = threadIdx.x; f < frames; f += MT_THREADS) v += frame_sum[(int64_t)b * g.frames + f];
    const double s = block_sum<MT_THREADS>(v, lds);
    if (threadIdx.x == 0) out[b] = s / ((double)frames * (double)g.n_mels);
}

// ---- mse, snr_db, si_sdr_db of a clip pair: one workgroup per clip, two fp64 passes ------------------------------------------------------
// pass 1: S_r, S_e, S_rr, S_re and D = sum (r - e)^2 (direct); mu = S / n, alpha = (S_re - S_r S_e / n) / (S_rr - S_r^2 / n).
// pass 2: V = sum (r - mu_r)^2 and E = sum ((e - mu_e) - alpha (r - mu_r))^2, both direct.  alpha minimises E, so its own rounding
//         (from the expanded pass-1 sums) enters E only squared.
__global__ __launch_bounds__(SM_THREADS) void signal_metrics_kernel(const float* __restrict__ ref, int64_t ref_stride, const float* __restrict__ est,
                                                                  int64_t est_stride, int64_t max_samples, const int* __restrict__ lens,
                                                                  double* __restrict__ out) {
    __shared__ double lds[SM_THREADS / 64];
    const int b = blockIdx.x;
    const float* r = ref + (int64_t)b * ref_stride;
    const float* e = est + (int64_t)b * est_stride;
    const int64_t n = lens ? lens[b] : max_samples;
    double sr = 0.0, se = 0.0, srr = 0.0, sre = 0.0, sd = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += SM_THREADS) {
        const double a = (double)r[i], c = (double)e[i], d = a - c;
        sr += a;
        se += c;
        srr += a * a;
        sre += a * c;
        sd += d * d;
    }
    sr = block_sum<SM_THREADS>(sr, lds);
    se = block_sum<SM_THREADS>(se, lds);
    srr = block_sum<SM_THREADS>(srr, lds);
    sre = block_sum<SM_THREADS>(sre, lds);
    sd = block_sum<SM_THREADS>(sd, lds);
    const double dn = (double)n;
    const double mu_r = sr / dn, mu_e = se / dn;
    const double alpha = (sre - sr * se / dn) / (srr - sr * sr / dn);
    double v = 0.0, res = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += SM_THREADS) {
        const double a = (double)r[i] - mu_r, c = (double)e[i] - mu_e;
        const double d = c - alpha * a;
        v += a * a;
        res += d * d;
    }
    v = block_sum<SM_THREADS>(v, lds);
    res = block_sum<SM_THREADS>(res, lds);
    if (threadIdx.x == 0) {
        out[3 * (int64_t)b] = sd / dn;
        out[3 * (int64_t)b + 1] = 10.0 * log10(srr / sd);
        out[3 * (int64_t)b + 2] = 10.0 * log10(alpha * alpha * v / res);
    }
}

enum MelMode { MODE_STFT, MODE_LOG_MEL, MODE_DISTANCE };

int run_mel(hipStream_t s, MelMode mode, const float* x0, int64_t stride0, const float* x1, int64_t stride1, int32_t batch, int64_t max_samples,
            const int32_t* samples, int32_t n_fft, int32_t hop, int32_t n_mels, const float* basis, const float* weights, void* out,
            void* scratch, int64_t scratch_bytes) {
    MelGeom g;
    MelScratch sc;
    L3AC_TRY(mel_geom(batch, max_samples, n_fft, hop, n_mels, mode != MODE_STFT, &g, &sc));
    const int n_sig = mode == MODE_DISTANCE ? 2 : 1;
    L3AC_REQUIRE(x0 && (n_sig == 1 || x1) && out, "metrics: null buffer");
    L3AC_REQUIRE(basis && (mode == MODE_STFT || weights), "metrics: null table (l3ac_stft_basis / l3ac_mel_weights, copied to the device)");
    L3AC_REQUIRE(((uintptr_t)basis & 15) == 0, "metrics: the basis must be 16-byte aligned");
    L3AC_REQUIRE(batch == 1 || (stride0 >= max_samples && (n_sig == 1 || stride1 >= max_samples)), "metrics: row stride below max_samples %lld",
                 (long long)max_samples);
    L3AC_TRY(check_clip_lengths("metrics", samples, batch, max_samples));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "metrics", "mel", samples, batch, scratch, scratch_bytes, sc.total_min, &lens));
    char* base = static_cast<char*>(scratch);
    int2* runs = reinterpret_cast<int2*>(base + sc.runs);
    double* frame_sum = reinterpret_cast<double*>(base + sc.frame_sum);
    float* stage = reinterpret_cast<float*>(base + sc.stage);
    float* spec = reinterpret_cast<float*>(base + sc.spec);
    // slot rows per product: what the scratch holds (per signal), never more than there are
    const int64_t group = std::min<int64_t>(g.rows, (scratch_bytes - sc.spec) / (n_sig * g.spec_ld * 4));
    float* spec1 = spec + group * g.spec_ld;

    if (mode == MODE_STFT)
        L3AC_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)batch * g.frames * g.bins * 2 * sizeof(float), s));
    if (mode == MODE_LOG_MEL)
        L3AC_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)batch * g.frames * n_mels * sizeof(float), s));
    {
        ProfScope prof(s, "metrics_stage_kernel", 0.0, 4.0 * n_sig * batch * (double)(max_samples + g.pitch));
        hipLaunchKernelGGL(metrics_stage_kernel, dim3((unsigned)ceil_div64(g.pitch / 4, MT_THREADS), (unsigned)batch, (unsigned)n_sig), dim3(MT_THREADS), 0,
                           s, x0, stride0, x1, stride1, lens, stage, g);
        L3AC_LAUNCH_CHECK();
    }
    if (mode != MODE_STFT) {
        hipLaunchKernelGGL(metrics_runs_kernel, dim3((unsigned)ceil_div64(n_mels, MT_THREADS)), dim3(MT_THREADS), 0, s, weights, n_mels, g.bins, runs);
        L3AC_LAUNCH_CHECK();
    }
    for (int64_t row0 = 0; row0 < g.rows; row0 += group) {
        const int64_t count = std::min(group, g.rows - row0);
        for (int sig = 0; sig < n_sig; ++sig) {
            GemmArgs ga;
            ga.a = stage + (int64_t)sig * batch * g.pitch + row0 * hop;  // row r of the product: frame row0 + r, n_fft floats from here + r hop
            ga.lda = hop;
            ga.w = basis;
            ga.ldw = n_fft;
            ga.c = sig ? spec1 : spec;
            ga.ldc = g.spec_ld;
            ga.m = count;
            ga.n = n_fft + 2;
            ga.k = n_fft;
            ga.epi = EPI_BIAS;
            L3AC_TRY(launch_gemm(s, ga));
        }
        if (mode == MODE_STFT) {
            ProfScope prof(s, "metrics_scatter_kernel", 0.0, 8.0 * count * (n_fft + 2));
            hipLaunchKernelGGL(metrics_scatter_kernel, dim3((unsigned)count), dim3(MT_THREADS), 0, s, spec, row0, lens, static_cast<float*>(out), g);
            L3AC_LAUNCH_CHECK();
        } else {
            ProfScope prof(s, "metrics_mel_kernel", 0.0, 4.0 * n_sig * count * (double)(n_fft + 2 + n_mels));
            hipLaunchKernelGGL(metrics_mel_kernel, dim3((unsigned)ceil_div64(count, MEL_ROWS)), dim3(MT_THREADS), 0, s, spec, spec1, row0, (int)count, lens,
                               weights, runs, mode == MODE_LOG_MEL ? static_cast<float*>(out) : nullptr, frame_sum, g);
            L3AC_LAUNCH_CHECK();
        }
    }
    if (mode == MODE_DISTANCE) {
        ProfScope prof(s, "metrics_mean_kernel", 0.0, 8.0 * batch * (double)g.frames);
        hipLaunchKernelGGL(metrics_mean_kernel, dim3((unsigned)batch), dim3(MT_THREADS), 0, s, frame_sum, lens, static_cast<double*>(out), g);
        L3AC_LAUNCH_CHECK();
    }
    return L3AC_OK;
}

}  // namespace

extern "C" {

int64_t l3ac_stft_frames(int64_t samples, int32_t hop) {
    L3AC_REQUIRE(samples >= 1 && hop >= 1, "stft_frames: samples %lld and hop %d must be positive", (long long)samples, hop);
    return 1 + samples / hop;
}

int64_t l3ac_stft_basis(int32_t n_fft, float* basis, int64_t cap) {
    L3AC_REQUIRE(n_fft >= 16 && n_fft <= 2048 && n_fft % 16 == 0, "metrics: n_fft %d must be a multiple of 16 in 16..2048", n_fft);
    const int64_t need = (int64_t)(n_fft + 2) * n_fft;
    if (!basis || cap < need) return need;
    const double step = 2.0 * M_PI / n_fft;
    for (int k = 0; k <= n_fft / 2; ++k) {
        for (int j = 0; j < n_fft; ++j) {
            const double w = 0.5 - 0.5 * std::cos(step * j);  // periodic Hann
            const double ang = step * (double)((j * k) % n_fft);  // the phase reduced in integers
            basis[(int64_t)(2 * k) * n_fft + j] = (float)(w * std::cos(ang));
            basis[(int64_t)(2 * k + 1) * n_fft + j] = (float)(-w * std::sin(ang));
        }
    }
    return need;
}

int64_t l3ac_mel_weights(int32_t sample_rate, int32_t n_fft, int32_t n_mels, float* w, int64_t cap) {
    L3AC_REQUIRE(sample_rate > 0, "metrics: sample_rate %d must be positive", sample_rate);
    L3AC_REQUIRE(n_fft >= 16 && n_fft <= 2048 && n_fft % 16 == 0, "metrics: n_fft %d must be a multiple of 16 in 16..2048", n_fft);
    L3AC_REQUIRE(n_mels >= 1 && n_mels <= MT_MAX_MELS, "metrics: n_mels %d outside 1..%d", n_mels, MT_MAX_MELS);
    const int bins = n_fft / 2 + 1;
    const int64_t need = (int64_t)n_mels * bins;
    if (!w || cap < need) return need;
    // HTK scale, no normalisation: n_mels + 2 points equally spaced in mel from 0 to sample_rate / 2
    const double mel_max = 2595.0 * std::log10(1.0 + 0.5 * sample_rate / 700.0);
    std::vector<double> p(n_mels + 2);
    for (int i = 0; i < n_mels + 2; ++i) p[i] = 700.0 * (std::pow(10.0, (mel_max * i / (n_mels + 1)) / 2595.0) - 1.0);
    for (int m = 0; m < n_mels; ++m) {
        for (int k = 0; k < bins; ++k) {
            const double f = (double)k * sample_rate / n_fft;
            const double up = (f - p[m]) / (p[m + 1] - p[m]), down = (p[m + 2] - f) / (p[m + 2] - p[m + 1]);
            w[(int64_t)m * bins + k] = (float)std::max(0.0, std::min(up, down));
        }
    }
    return need;
}

int64_t l3ac_mel_scratch_bytes(int32_t batch, int64_t max_samples, int32_t n_fft, int32_t hop, int32_t n_mels) {
    MelGeom g;
    MelScratch sc;
    L3AC_TRY(mel_geom(batch, max_samples, n_fft, hop, n_mels, true, &g, &sc));
    return sc.total_min;
}

int l3ac_stft(const float* audio, int32_t batch, int64_t max_samples, int64_t audio_stride, const int32_t* samples, int32_t n_fft, int32_t hop,
              const float* basis, float* spec, void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    return run_mel(s, MODE_STFT, audio, audio_stride, nullptr, 0, batch, max_samples, samples, n_fft, hop, 0, basis, nullptr, spec, scratch,
                   scratch_bytes);
}

int l3ac_log_mel(const float* audio, int32_t batch, int64_t max_samples, int64_t audio_stride, const int32_t* samples, int32_t n_fft, int32_t hop,
                 const float* basis, const float* weights, int32_t n_mels, float* out, void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    return run_mel(s, MODE_LOG_MEL, audio, audio_stride, nullptr, 0, batch, max_samples, samples, n_fft, hop, n_mels, basis, weights, out, scratch,
                   scratch_bytes);
}

int l3ac_mel_distance(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples,
                      const int32_t* samples, int32_t n_fft, int32_t hop, int32_t n_mels, const float* basis, const float* weights, double* out,
                      void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    return run_mel(s, MODE_DISTANCE, ref, ref_stride, est, est_stride, batch, max_samples, samples, n_fft, hop, n_mels, basis, weights, out, scratch,
                   scratch_bytes);
}

int l3ac_signal_metrics(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples,
                        const int32_t* samples, double* out, void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    L3AC_REQUIRE(ref && est && out, "signal_metrics: null buffer");
    L3AC_REQUIRE(batch > 0 && max_samples > 0, "signal_metrics: empty input (batch %d, samples %lld)", batch, (long long)max_samples);
    L3AC_REQUIRE(max_samples < ((int64_t)1 << 31), "signal_metrics: clips of %lld samples are too long", (long long)max_samples);
    L3AC_REQUIRE(batch == 1 || (ref_stride >= max_samples && est_stride >= max_samples), "signal_metrics: row stride below max_samples %lld",
                 (long long)max_samples);
    L3AC_TRY(check_clip_lengths("metrics", samples, batch, max_samples));  // (this one message has always said "metrics")
    int* lens = nullptr;
    if (samples) {  // the clips' lengths live in the scratch: batch int32
        L3AC_REQUIRE(scratch && ((uintptr_t)scratch & 3) == 0 && scratch_bytes >= (int64_t)batch * 4,
                     "signal_metrics: with per-clip lengths the scratch must hold batch (%d) int32", batch);
        lens = static_cast<int*>(scratch);
        L3AC_TRY(launch_ragged_upload(s, lens, samples, batch));
    }
    ProfScope prof(s, "signal_metrics_kernel", 16.0 * batch * (double)max_samples, 16.0 * batch * (double)max_samples);
    hipLaunchKernelGGL(signal_metrics_kernel, dim3((unsigned)batch), dim3(SM_THREADS), 0, s, ref, ref_stride, est, est_stride, max_samples, lens, out);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

}  // extern "C"
