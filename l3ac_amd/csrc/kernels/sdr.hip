// The SDR of BSS Eval for one source: the signal-to-distortion ratio of an estimate after any linear time-invariant distortion of up to L taps
// of the reference has been allowed (include/l3ac_hip.h, "BSS Eval SDR"; DESIGN.md §3.21, which is normative), and its two primitives on their
// own: the lag correlation of whole clips and the Toeplitz solve.  No reference counterpart.
//
//   sdr_corr_kernel      grid (groups of 16 lags, sides, batch), 4 waves, 4 lags a wave.  corr(u, v)[k] = sum_{t=0}^{n-1-k} u[t] v[t+k]: the clip
//                        goes through LDS in tiles of 2048 samples as fp32 — the u tile, and the v tile from the group's first lag on with 15
//                        more samples — lane l walks t = l mod 64, so consecutive lanes read consecutive addresses (no bank conflict), and a
//                        wave's four partial sums per lane stay in registers across the tiles.  fp64: the samples are converted first, so
//                        a product is exact; partial l takes its terms in increasing t from +0, then the fold s[l] += s[l + h], h = 32 .. 1.
//                        The order depends on n and k alone.  Side 0 of l3ac_sdr is corr(s, s), whose lag 0 takes the diagonal loading; side 1
//                        is corr(s, s^).
//   sdr_solve_kernel     one wave per pair: the Levinson recursion with a general right-hand side for G c = b, G[i][j] = r[|i - j|].  r, b,
//                        c and two copies of the predictor a sit in LDS (40 KiB at L = 1024).  Step m: lane l takes the terms i = i0 + l,
//                        i0 + l + 64, .. of both inner sums — they read the state of step m - 1 alone — in increasing i from +0, two folds,
//                        then every lane forms k_m, E_m, lambda and nu from the broadcast sums, and lane l writes a'[i] for its i and the
//                        c'[m - i] that a'[i] enters.  Two barriers a step, of one wave: they order its LDS traffic and wait for nobody.
//   sdr_residual_kernel  grid (segments of 4096 outputs, batch), 256 threads.  c as fp64 and s[4096 q - L + 1 .. 4096 q + 4096) as fp32 sit in
//                        LDS; thread i owns the outputs t = 4096 q + i + 256 j, j = 0 .. 15, in registers; per tap one broadcast read of
//                        c[k] and sixteen conflict-free reads of s.  y[t] from +0 in increasing k, e[t] = s^[t] - y[t]; the thread's y^2 and
//                        e^2 from +0 in increasing j, block_sum, two fp64 per segment.
//   sdr_final_kernel     one thread per pair: the segments' sums from +0 in increasing q, 10 log10(T / D), NaN for an invalid pair.
//
// A sample outside [0, n) is selected away, never multiplied by zero; validity selects between values; every index and loop bound comes from
// the parameters and the clips' lengths, never from a sample.  A pair's values depend on its own n samples a side only — not on the batch,
// the row, the strides or the scratch size; what lies at or after the clip's length is never read.  No atomics.
//
// Contraction is off for this whole file: every product and sum rounds on its own, in the order DESIGN.md states.
#include "metric_common.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int SD_MAX_TAPS = 1024;
constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / 64;
constexpr int SC_RUN = 4;                    // lags a wave holds in registers
constexpr int SC_GROUP = SC_WAVES * SC_RUN;  // lags of a workgroup
constexpr int SC_TILE = 2048;                // samples of a tile: a multiple of 64, so that lane l keeps t = l mod 64
constexpr int SR_THREADS = 256;
constexpr int SR_PER = 16;                   // outputs a thread owns
constexpr int SR_SEG = SR_THREADS * SR_PER;  // outputs of a segment

static_assert(SC_TILE % 64 == 0, "a tile keeps the lanes' residues");
static_assert(SR_SEG == 4096, "DESIGN.md states the segment");
static_assert(5 * SD_MAX_TAPS * 8 <= 64 * 1024, "the solve's state fits the LDS of a launch that asks for nothing");

__device__ __forceinline__ double lane0(double v) { return __shfl(v, 0, 64); }

// ---- correlation: out[(b sides + side) lags + k] -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_THREADS) void sdr_corr_kernel(const float* __restrict__ u, int64_t u_stride, const float* __restrict__ v0,
                                                            int64_t v0_stride, const float* __restrict__ v1, int64_t v1_stride, int64_t max_samples,
                                                            const int* __restrict__ lens, int lags, double load, double* __restrict__ out) {
    __shared__ float us[SC_TILE];
    __shared__ float vs[SC_TILE + SC_GROUP];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int side = blockIdx.y, b = blockIdx.z;
    const int kb = blockIdx.x * SC_GROUP;  // the group's first lag
    const int kw = kb + wave * SC_RUN;     // the wave's first lag
    const int64_t n = lens ? lens[b] : max_samples;
    const float* x = u + (int64_t)b * u_stride;
    const float* y = side ? v1 + (int64_t)b * v1_stride : v0 + (int64_t)b * v0_stride;
    double s[SC_RUN];
#pragma unroll
    for (int j = 0; j < SC_RUN; ++j) s[j] = 0.0;
    for (int64_t t0 = 0; t0 < n; t0 += SC_TILE) {  // (the bound is the clip's length)
        __syncthreads();                           // the previous tile has been read
        for (int i = tid; i < SC_TILE; i += SC_THREADS) us[i] = t0 + i < n ? x[t0 + i] : 0.f;
        for (int i = tid; i < SC_TILE + SC_GROUP; i += SC_THREADS) vs[i] = t0 + kb + i < n ? y[t0 + kb + i] : 0.f;
        __syncthreads();
        const int64_t left = n - t0;  // terms t0 + i with i + k < left are inside the clip
        const int count = left < SC_TILE ? (int)left : SC_TILE;
        for (int i = lane; i < count; i += 64) {
            const double a = (double)us[i];
#pragma unroll
            for (int j = 0; j < SC_RUN; ++j) {
                const double p = a * (double)vs[i + wave * SC_RUN + j];
                s[j] = i + kw + j < left ? s[j] + p : s[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < SC_RUN; ++j) {
        double r = fold64(s[j]);
        if (side == 0 && kw + j == 0 && load != 0.0) r = r * (1.0 + load);
        if (lane == 0 && kw + j < lags) out[((int64_t)b * gridDim.y + side) * lags + kw + j] = r;
    }
}

// ---- Toeplitz solve: one wave per pair.  r, b: rows `row` doubles apart; x [batch][len]; error `err_stride` doubles apart ------------------------
__global__ __launch_bounds__(64) void sdr_solve_kernel(const double* __restrict__ r_in, const double* __restrict__ b_in, int64_t row, int len,
                                                     double* __restrict__ x, double* __restrict__ error, int64_t err_stride, int* __restrict__ valid) {
    extern __shared__ __attribute__((aligned(16))) double sv[];
    double *r = sv, *rhs = sv + len, *c = sv + 2 * len, *a = sv + 3 * len, *a_new = sv + 4 * len;
    const int lane = threadIdx.x, pair = blockIdx.x;
    for (int i = lane; i < len; i += 64) {
        r[i] = r_in[(int64_t)pair * row + i];
        rhs[i] = b_in[(int64_t)pair * row + i];
        a[i] = a_new[i] = i == 0 ? 1.0 : 0.0;
        c[i] = 0.0;
    }
    __syncthreads();
    const double r0 = r[0];
    bool ok = r0 > 0.0;
    double e = r0;
    if (lane == 0) c[0] = rhs[0] / r0;
    __syncthreads();
    for (int m = 1; m < len; ++m) {
        double pa = 0.0, pc = 0.0;
        for (int i = 1 + lane; i < m; i += 64) pa = pa + a[i] * r[m - i];
        for (int i = lane; i < m; i += 64) pc = pc + c[i] * r[m - i];
        const double acc = r[m] + lane0(fold64(pa));
        const double km = -acc / e;
        e = e * (1.0 - km * km);
        ok = ok && e > 0.0;
        const double lam = rhs[m] - lane0(fold64(pc));
        const double nu = lam / e;
        __syncthreads();                           // every lane has read the c of step m - 1
        for (int i = 1 + lane; i <= m; i += 64) {  // a'[i], and c'[m - i] = c[m - i] + nu a'[i]
            const double an = i < m ? a[i] + km * a[m - i] : km;
            a_new[i] = an;
            c[m - i] = c[m - i] + nu * an;
        }
        if (lane == 0) c[m] = nu;
        __syncthreads();
        double* swap = a;
        a = a_new, a_new = swap;
    }
    const double nan = __builtin_nan("");
    for (int i = lane; i < len; i += 64) x[(int64_t)pair * len + i] = ok ? c[i] : nan;
    if (lane == 0) error[(int64_t)pair * err_stride] = ok ? e : nan, valid[pair] = ok ? 1 : 0;
}

// ---- residual: seg[(b segs + q) 2] = the segment's sum of y^2, of e^2 ---------------------------------------------------------------------------
__global__ __launch_bounds__(SR_THREADS) void sdr_residual_kernel(const float* __restrict__ ref, int64_t ref_stride, const float* __restrict__ est,
                                                                int64_t est_stride, int64_t max_samples, const int* __restrict__ lens,
                                                                const double* __restrict__ filter, int taps, int64_t segs, double* __restrict__ seg) {
    extern __shared__ __attribute__((aligned(16))) double sr[];
    __shared__ double red[SR_THREADS / 64];
    double* c = sr;                                      // [taps]
    float* xs = reinterpret_cast<float*>(sr + taps);  // [SR_SEG + taps - 1]: sample 4096 q - taps + 1 + i
    const int tid = threadIdx.x, b = blockIdx.y;
    const int64_t q = blockIdx.x;
    const int64_t n = lens ? lens[b] : max_samples;
    const int64_t outputs = n + taps - 1;
    if (q * SR_SEG >= outputs) return;  // (the whole workgroup: a segment past the clip's own)
    const float* x = ref + (int64_t)b * ref_stride;
    const float* z = est + (int64_t)b * est_stride;
    const int64_t first = q * SR_SEG - (taps - 1);
    for (int i = tid; i < taps; i += SR_THREADS) c[i] = filter[(int64_t)b * taps + i];
    for (int i = tid; i < SR_SEG + taps - 1; i += SR_THREADS) {
        const int64_t t = first + i;
        xs[i] = t >= 0 && t < n ? x[t] : 0.f;
    }
    __syncthreads();
    double y[SR_PER];
#pragma unroll
    for (int j = 0; j < SR_PER; ++j) y[j] = 0.0;
    for (int k = 0; k < taps; ++k) {
        const double ck = c[k];
        const int at = tid + (taps - 1) - k;  // the LDS index of sample t - k for j = 0
#pragma unroll
        for (int j = 0; j < SR_PER; ++j) {
            const int64_t t = first + at + SR_THREADS * j;  // t - k of the clip
            const double p = ck * (double)xs[at + SR_THREADS * j];
            y[j] = t >= 0 && t < n ? y[j] + p : y[j];
        }
    }
    double tt = 0.0, dd = 0.0;
#pragma unroll
    for (int j = 0; j < SR_PER; ++j) {
        const int64_t t = q * SR_SEG + tid + SR_THREADS * j;
        if (t < outputs) {
            const double e = (t < n ? (double)z[t] : 0.0) - y[j];
            tt = tt + y[j] * y[j];
            dd = dd + e * e;
        }
    }
    tt = block_sum<SR_THREADS>(tt, red);
    dd = block_sum<SR_THREADS>(dd, red);
    if (tid == 0) seg[((int64_t)b * segs + q) * 2] = tt, seg[((int64_t)b * segs + q) * 2 + 1] = dd;
}

// ---- the pair: out[b][0..2] = sdr_db, T, D; out[b][3] is the solve's E_{L-1} ---------------------------------------------------------------------
__global__ __launch_bounds__(64) void sdr_final_kernel(const double* __restrict__ seg, int64_t segs, int64_t max_samples, const int* __restrict__ lens,
                                                     int taps, const int* __restrict__ valid, int batch, double* __restrict__ out) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    const int64_t n = lens ? lens[b] : max_samples;
    int64_t own = (n + taps - 1 + SR_SEG - 1) / SR_SEG;
    own = own < segs ? own : segs;  // (the host sized segs for max_samples; the clamp bounds every index)
    double tt = 0.0, dd = 0.0;
    for (int64_t q = 0; q < own; ++q) tt = tt + seg[((int64_t)b * segs + q) * 2], dd = dd + seg[((int64_t)b * segs + q) * 2 + 1];
    const bool ok = valid[b] != 0;
    const double nan = __builtin_nan("");
    out[(int64_t)b * 4] = ok ? 10.0 * log10(tt / dd) : nan;
    out[(int64_t)b * 4 + 1] = ok ? tt : nan;
    out[(int64_t)b * 4 + 2] = ok ? dd : nan;
}

int check_taps(const char* what, const char* name, int32_t taps) {
    L3AC_REQUIRE(taps >= 1 && taps <= SD_MAX_TAPS, "%s: %s %d outside 1..%d", what, name, taps, SD_MAX_TAPS);
    return L3AC_OK;
}

// a batch of clips whose lagged or filtered extent stays an int32
int check_extent(const char* what, const char* name, int32_t batch, int64_t max_samples, int32_t taps) {
    L3AC_TRY(check_taps(what, name, taps));
    L3AC_TRY(check_clip_batch(what, batch, max_samples));
    L3AC_REQUIRE(max_samples + taps - 1 < ((int64_t)1 << 31), "%s: max_samples %lld + %s %d - 1 must stay below 2^31", what, (long long)max_samples, name,
                 taps);
    return L3AC_OK;
}

struct SdrScratch {  // byte offsets into the caller's scratch, after the clips' lengths
    int64_t corr, filter, seg, segs, need;
};

// the autocorrelation and cross-correlation [batch][2][L] fp64, the filter [batch][L] fp64, the segments' two sums [batch][S][2] fp64
int sdr_scratch(int32_t batch, int64_t max_samples, int32_t taps, SdrScratch* sc) {
    L3AC_TRY(check_extent("sdr", "filter_length", batch, max_samples, taps));
    ScratchPlan plan(batch);
    sc->segs = ceil_div64(max_samples + taps - 1, SR_SEG);
    sc->corr = plan.take((int64_t)batch * 2 * taps * 8);
    sc->filter = plan.take((int64_t)batch * taps * 8);
    sc->seg = plan.take((int64_t)batch * sc->segs * 16);
    sc->need = plan.bytes;
    return L3AC_OK;
}

void enqueue_corr(hipStream_t s, const float* u, int64_t u_stride, const float* v0, int64_t v0_stride, const float* v1, int64_t v1_stride, int32_t batch,
                  int64_t max_samples, const int* lens, int32_t lags, double load, double* out) {
    const int sides = v1 ? 2 : 1;
    ProfScope prof(s, "sdr_corr_kernel", 2.0 * sides * batch * (double)max_samples * lags, 4.0 * (sides + 1) * batch * (double)max_samples);
    hipLaunchKernelGGL(sdr_corr_kernel, dim3((unsigned)ceil_div64(lags, SC_GROUP), (unsigned)sides, (unsigned)batch), dim3(SC_THREADS), 0, s, u, u_stride,
                       v0, v0_stride, v1 ? v1 : v0, v1 ? v1_stride : v0_stride, max_samples, lens, lags, load, out);
}

void enqueue_solve(hipStream_t s, const double* r, const double* b, int64_t row, int32_t batch, int32_t len, double* x, double* error, int64_t err_stride,
                   int32_t* valid) {
    ProfScope prof(s, "sdr_solve_kernel", 4.0 * batch * (double)len * len, 24.0 * batch * (double)len);
    hipLaunchKernelGGL(sdr_solve_kernel, dim3((unsigned)batch), dim3(64), (size_t)5 * len * 8, s, r, b, row, len, x, error, err_stride, valid);
}

}  // namespace

extern "C" {

int64_t l3ac_correlate_scratch_bytes(int32_t batch, int64_t max_samples, int32_t lags) {
    L3AC_TRY(check_extent("correlate", "lags", batch, max_samples, lags));
    return ScratchPlan(batch).bytes;  // the clips' lengths
}

int l3ac_correlate(const float* u, int64_t u_stride, const float* v, int64_t v_stride, int32_t batch, int64_t max_samples, const int32_t* samples,
                   int32_t lags, double* out, void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    L3AC_TRY(check_extent("correlate", "lags", batch, max_samples, lags));
    L3AC_REQUIRE(u && v, "correlate: null audio");
    L3AC_REQUIRE(out, "correlate: null output buffer");
    L3AC_REQUIRE(batch == 1 || (u_stride >= max_samples && v_stride >= max_samples), "correlate: row stride below max_samples %lld",
                 (long long)max_samples);
    L3AC_TRY(check_clip_lengths("correlate", samples, batch, max_samples));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "correlate", "correlate", samples, batch, scratch, scratch_bytes, ScratchPlan(batch).bytes, &lens));
    enqueue_corr(s, u, u_stride, v, v_stride, nullptr, 0, batch, max_samples, lens, lags, 0.0, out);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

int64_t l3ac_toeplitz_solve_scratch_bytes(int32_t batch, int32_t length) {
    L3AC_TRY(check_taps("toeplitz_solve", "length", length));
    L3AC_REQUIRE(batch > 0 && batch <= 65535, "toeplitz_solve: batch %d outside 1..65535", batch);
    return ScratchPlan(batch).bytes;  // the first region of every layout; the solve keeps its state in LDS
}

int l3ac_toeplitz_solve(const double* r, const double* b, int32_t batch, int32_t length, double* x, double* error, int32_t* valid, void* scratch,
                        int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    L3AC_TRY(check_taps("toeplitz_solve", "length", length));
    L3AC_REQUIRE(batch > 0 && batch <= 65535, "toeplitz_solve: batch %d outside 1..65535", batch);
    L3AC_REQUIRE(r && b, "toeplitz_solve: null input");
    L3AC_REQUIRE(x && error && valid, "toeplitz_solve: null output buffer");
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "toeplitz_solve", "toeplitz_solve", nullptr, batch, scratch, scratch_bytes, ScratchPlan(batch).bytes, &lens));
    enqueue_solve(s, r, b, length, batch, length, x, error, 1, valid);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

int64_t l3ac_sdr_scratch_bytes(int32_t batch, int64_t max_samples, int32_t filter_length) {
    SdrScratch sc;
    L3AC_TRY(sdr_scratch(batch, max_samples, filter_length, &sc));
    return sc.need;
}

int l3ac_sdr(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples, const int32_t* samples,
             int32_t filter_length, double load, double* out, int32_t* valid, double* filter, double* corr, void* scratch, int64_t scratch_bytes,
             void* stream) {
    hipStream_t s = (hipStream_t)stream;
    SdrScratch sc;
    L3AC_TRY(sdr_scratch(batch, max_samples, filter_length, &sc));
    L3AC_REQUIRE(load >= 0.0 && std::isfinite(load), "sdr: load %g must be finite and not negative", load);
    L3AC_REQUIRE(ref && est, "sdr: null audio");
    L3AC_REQUIRE(out && valid, "sdr: null output buffer");
    L3AC_REQUIRE(batch == 1 || (ref_stride >= max_samples && est_stride >= max_samples), "sdr: row stride below max_samples %lld", (long long)max_samples);
    L3AC_TRY(check_clip_lengths("sdr", samples, batch, max_samples));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "sdr", "sdr", samples, batch, scratch, scratch_bytes, sc.need, &lens));
    char* base = static_cast<char*>(scratch);
    double* rb = corr ? corr : reinterpret_cast<double*>(base + sc.corr);
    double* c = filter ? filter : reinterpret_cast<double*>(base + sc.filter);
    double* seg = reinterpret_cast<double*>(base + sc.seg);
    const int taps = filter_length;
    enqueue_corr(s, ref, ref_stride, ref, ref_stride, est, est_stride, batch, max_samples, lens, taps, load, rb);
    L3AC_LAUNCH_CHECK();
    enqueue_solve(s, rb, rb + taps, 2 * (int64_t)taps, batch, taps, c, out + 3, 4, valid);
    L3AC_LAUNCH_CHECK();
    {
        ProfScope prof(s, "sdr_residual_kernel", 2.0 * batch * (double)(max_samples + taps) * taps, 8.0 * batch * (double)max_samples);
        hipLaunchKernelGGL(sdr_residual_kernel, dim3((unsigned)sc.segs, (unsigned)batch), dim3(SR_THREADS), (size_t)taps * 8 + (size_t)(SR_SEG + taps) * 4,
                           s, ref, ref_stride, est, est_stride, max_samples, lens, c, taps, sc.segs, seg);
        L3AC_LAUNCH_CHECK();
    }
    ProfScope prof(s, "sdr_final_kernel", 0.0, 16.0 * batch * (double)sc.segs);
    hipLaunchKernelGGL(sdr_final_kernel, dim3((unsigned)ceil_div64(batch, 64)), dim3(64), 0, s, seg, sc.segs, max_samples, lens, taps, valid, batch, out);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

}  // extern "C"
