// ITU-R BS.1770-4 integrated loudness of mono clips, and loudness normalisation (include/l3ac_hip.h, "loudness").  No
// reference counterpart.  Everything here is fp64; the fp32 samples convert exactly.
//
// K-weighting is two biquads in cascade (transposed direct form II), a linear recurrence with a 4-value state (s1, s2 of the shelf, s1, s2
// of the high-pass).  It runs in parallel over time with one step (100 ms, fs / 10 samples) as the segment:
//   1. loudness_pass_kernel<false>  every (clip, step) filters its samples from a ZERO state and writes its 4-value end state; the same
//                                   pass takes the step's max |x|
//   2. loudness_scan_kernel         one thread per clip walks the steps in order: start_{s+1} = M start_s + end_s, M the 4x4 matrix that
//                                   advances the cascade's state over one step of zero input (the response is linear: from a true start
//                                   state the end state is the zero-input part M start plus the zero-state part); start_s replaces end_s.
//                                   M and the running state are pairs of doubles (hi + lo), see pair.hpp
//   3. loudness_pass_kernel<true>   every (clip, step) reruns the recursion from its true start state and sums y^2 in sample order: e_s
//   4. loudness_gate_kernel         one workgroup per clip: z_j, l_j, the absolute and the relative gate, L, the sample peak, the counts
// The EBU R128 entries run phases 1 to 3 through the same host helper and read the step energies instead of phase 4:
//   loudness_series_kernel  the blocks of any window of 1 .. 600 steps: z_k, l_k, and a copy of the step energies
//   loudness_range_kernel   one workgroup per clip: EBU Tech 3342 loudness range on 3 s blocks, the short-term and momentary maxima
// The coefficients and M are designed on the host in fp64 (loudness_coeffs) and travel as kernel arguments: no device table, nothing to
// warm up before a capture.  A step's values depend on its own samples and on the steps before it in its own clip only — never on the
// batch, the clip's row, the row stride or the scratch size; no atomics; the sums of the gate kernel run over fixed strides and a fixed tree.
//
// One lane per step reads rows `step` floats apart, so a wave's 64 steps are staged through LDS 32 samples at a time: the loads run
// along the rows (128 contiguous bytes per half wave, any alignment, any step), the recursion reads its own row of the tile at an odd
// pitch (no bank conflicts), and the next round's loads are in flight while the current one is filtered.
//
// The product of a multiply must not be fused into the add that follows it differently in the two passes or on the host: contraction is
// off for this whole file, host code included (M is designed by the same recursion).
#include "metric_common.hpp"

#include <algorithm>
#include <cmath>
#include <limits>

#pragma clang fp contract(off)

#include "pair.hpp"

namespace {

constexpr int LD_STEPS = 64;              // steps per workgroup: one wave, one lane per step
constexpr int LD_CHUNK = 32;              // samples of every step staged per round
constexpr int LD_PITCH = LD_CHUNK + 1;    // odd: lane l reads bank (l + j) % 32
constexpr int LD_GATE_THREADS = 256;
constexpr int LD_GAIN_THREADS = 256;
constexpr int LD_MIN_RATE = 8000, LD_MAX_RATE = 192000;

struct LoudFilter {  // b0 b1 b2 a1 a2 of the two stages (a0 = 1), M row-major as hi + lo, the step in samples
    double c[2][5];
    double m[4][4], m_lo[4][4];
    int step;
};

struct LoudScratch {  // byte offsets into the caller's scratch, after the clips' lengths
    int64_t state, energy, step_max, total_min;
};

bool rate_ok(int32_t fs) { return fs % 10 == 0 && fs >= LD_MIN_RATE && fs <= LD_MAX_RATE; }

#define LD_REQUIRE_RATE(fs) \
    L3AC_REQUIRE(rate_ok(fs), "loudness: sample_rate %d must be a multiple of 10 in %d..%d", fs, LD_MIN_RATE, LD_MAX_RATE)

// one sample through one biquad, transposed direct form II: the order of scipy.signal.sosfilt
template <typename T>
__host__ __device__ __forceinline__ T biquad(const T (&c)[5], T x, T& s1, T& s2) {
    const T y = c[0] * x + s1;
    s1 = c[1] * x - c[3] * y + s2;
    s2 = c[2] * x - c[4] * y;
    return y;
}

// (Pair, pair_add, pair_mul: what the scan carries, pair.hpp)

int loud_geom(int32_t batch, int64_t max_samples, int32_t sample_rate, int64_t* s_max, LoudScratch* sc) {
    LD_REQUIRE_RATE(sample_rate);
    L3AC_TRY(check_clip_batch("loudness", batch, max_samples));
    *s_max = max_samples / (sample_rate / 10);
    ScratchPlan plan(batch);
    sc->state = plan.take((int64_t)batch * *s_max * 4 * 8);
    sc->energy = plan.take((int64_t)batch * *s_max * 8);
    sc->step_max = plan.take((int64_t)batch * *s_max * 4);
    sc->total_min = plan.bytes;
    return L3AC_OK;
}

// ---- phases 1 and 3: grid (groups of 64 steps, batch), one wave ----------------------------------------------------------------------
// ENERGY = false: from a zero state; writes state[clip][s][4] = the end state and step_max[clip][s].
// ENERGY = true:  from state[clip][s] (the scan's true start state); writes energy[clip][s] = sum y^2 in the order of the samples.
template <bool ENERGY>
__global__ __launch_bounds__(LD_STEPS) void loudness_pass_kernel(const float* __restrict__ audio, int64_t stride, int64_t max_samples,
                                                                const int* __restrict__ lens, LoudFilter f, int64_t s_max,
                                                                double* __restrict__ state, double* __restrict__ energy,
                                                                float* __restrict__ step_max) {
    __shared__ float tile[LD_STEPS * LD_PITCH];
    const int b = blockIdx.y;
    const int64_t n = lens ? lens[b] : max_samples;
    const int64_t steps = n / f.step;  // every sample of a whole step lies inside the clip: (s + 1) step <= n
    const int64_t s0 = (int64_t)blockIdx.x * LD_STEPS;
    if (s0 >= steps) return;  // (the whole workgroup)
    const float* x = audio + (int64_t)b * stride;
    const int lane = threadIdx.x;
    const int64_t s = s0 + lane;
    const bool active = s < steps;
    // round r of the loads: row 2 i + (lane >> 5) of the tile, column lane & 31, i = 0 .. 31
    const int col = lane & (LD_CHUNK - 1), half = lane >> 5;
    float pre[LD_CHUNK];
    auto fetch = [&](int c0) {
        const bool col_ok = c0 + col < f.step;
#pragma unroll
        for (int i = 0; i < LD_CHUNK; ++i) {
            const int64_t row = s0 + 2 * i + half;
            pre[i] = (col_ok && row < steps) ? x[row * f.step + c0 + col] : 0.f;
        }
    };
    double s1a = 0.0, s2a = 0.0, s1b = 0.0, s2b = 0.0, e = 0.0;
    float mx = 0.f;
    double* st = state + ((int64_t)b * s_max + s) * 4;
    if (ENERGY && active) s1a = st[0], s2a = st[1], s1b = st[2], s2b = st[3];
    fetch(0);
    for (int c0 = 0; c0 < f.step; c0 += LD_CHUNK) {
        __syncthreads();  // the previous round's reads are over
#pragma unroll
        for (int i = 0; i < LD_CHUNK; ++i) tile[(2 * i + half) * LD_PITCH + col] = pre[i];
        __syncthreads();
        if (c0 + LD_CHUNK < f.step) fetch(c0 + LD_CHUNK);
        const int count = min(LD_CHUNK, f.step - c0);
        for (int j = 0; j < count; ++j) {
            const float xf = tile[lane * LD_PITCH + j];
            const double y = biquad(f.c[1], biquad(f.c[0], (double)xf, s1a, s2a), s1b, s2b);
            if (ENERGY) e = e + y * y;
            else mx = fmaxf(mx, fabsf(xf));
        }
    }
    if (!active) return;
    if (ENERGY) {
        energy[(int64_t)b * s_max + s] = e;
    } else {
        st[0] = s1a, st[1] = s2a, st[2] = s1b, st[3] = s2b;
        step_max[(int64_t)b * s_max + s] = mx;
    }
}

// ---- phase 2: one thread per clip; state[clip][s] = the end state from zero -> the true start state -------------------------------------
__global__ __launch_bounds__(64) void loudness_scan_kernel(int batch, int64_t max_samples, const int* __restrict__ lens, LoudFilter f, int64_t s_max,
                                                         double* __restrict__ state) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= batch) return;
    const int64_t steps = (lens ? lens[b] : max_samples) / f.step;
    double* st = state + (int64_t)b * s_max * 4;
    Pair cur[4] = {};
    for (int64_t s = 0; s < steps; ++s, st += 4) {
        const double end[4] = {st[0], st[1], st[2], st[3]};
#pragma unroll
        for (int k = 0; k < 4; ++k) st[k] = cur[k].hi;  // the passes start from the pair rounded to fp64
        Pair nxt[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            Pair acc = pair_mul({f.m[k][0], f.m_lo[k][0]}, cur[0]);
#pragma unroll
            for (int i = 1; i < 4; ++i) acc = pair_add(acc, pair_mul({f.m[k][i], f.m_lo[k][i]}, cur[i]));
            nxt[k] = pair_add(acc, {end[k], 0.0});
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) cur[k] = nxt[k];
    }
}

// ---- phase 4: blocks, gates, L; one workgroup per clip ------------------------------------------------------------------------------------
__global__ __launch_bounds__(LD_GATE_THREADS) void loudness_gate_kernel(const float* __restrict__ audio, int64_t stride, int64_t max_samples,
                                                                      const int* __restrict__ lens, int step, int64_t s_max, int64_t j_max,
                                                                      const double* __restrict__ energy, const float* __restrict__ step_max,
                                                                      double* __restrict__ stats, int* __restrict__ counts,
                                                                      double* __restrict__ momentary) {
    __shared__ double lds[LD_GATE_THREADS / 64];
    const int b = blockIdx.x;
    const int64_t n = lens ? lens[b] : max_samples;
    const int64_t steps = n / step;
    const int64_t blocks = steps > 3 ? steps - 3 : 0;
    const double* e = energy + (int64_t)b * s_max;
    const double norm = 4.0 * (double)step;
    const double ninf = -__builtin_huge_val();
    auto mean_square = [&](int64_t j) { return (((e[j] + e[j + 1]) + e[j + 2]) + e[j + 3]) / norm; };
    auto lkfs = [&](double z) { return -0.691 + 10.0 * log10(z); };  // (-inf for z = 0)

    // the absolute gate; the l_j row on request
    double sum = 0.0, cnt = 0.0;
    for (int64_t j = threadIdx.x; j < blocks; j += LD_GATE_THREADS) {
        const double z = mean_square(j), l = lkfs(z);
        if (momentary) momentary[(int64_t)b * j_max + j] = l;
        if (l > -70.0) sum += z, cnt += 1.0;
    }
    if (momentary)
        for (int64_t j = blocks + threadIdx.x; j < j_max; j += LD_GATE_THREADS) momentary[(int64_t)b * j_max + j] = ninf;
    sum = block_sum<LD_GATE_THREADS>(sum, lds);
    cnt = block_sum<LD_GATE_THREADS>(cnt, lds);  // (whole numbers below 2^31: exact)
    // the relative gate, 10 LU below the loudness of the absolutely gated blocks (no such block: nothing passes)
    const double gamma = lkfs(sum / cnt) - 10.0;
    double sum2 = 0.0, cnt2 = 0.0;
    if (cnt > 0.0) {
        for (int64_t j = threadIdx.x; j < blocks; j += LD_GATE_THREADS) {
            const double z = mean_square(j), l = lkfs(z);
            if (l > -70.0 && l > gamma) sum2 += z, cnt2 += 1.0;
        }
    }
    sum2 = block_sum<LD_GATE_THREADS>(sum2, lds);
    cnt2 = block_sum<LD_GATE_THREADS>(cnt2, lds);

    // the sample peak over the clip's own n samples: the whole steps' maxima, then the samples after the last whole step
    double peak = 0.0;
    for (int64_t s = threadIdx.x; s < steps; s += LD_GATE_THREADS) peak = fmax(peak, (double)step_max[(int64_t)b * s_max + s]);
    const float* x = audio + (int64_t)b * stride;
    for (int64_t i = steps * step + threadIdx.x; i < n; i += LD_GATE_THREADS) peak = fmax(peak, (double)fabsf(x[i]));
    peak = block_max<LD_GATE_THREADS>(peak, lds);

    if (threadIdx.x == 0) {
        stats[2 * (int64_t)b] = cnt2 > 0.0 ? lkfs(sum2 / cnt2) : ninf;
        stats[2 * (int64_t)b + 1] = peak;
        counts[2 * (int64_t)b] = (int)blocks;
        counts[2 * (int64_t)b + 1] = (int)cnt2;
    }
}

// ---- stats [batch][2] (L, peak) -> gain [batch][2] (g_db, gain) -----------------------------------------------------------------------------
__global__ __launch_bounds__(LD_GAIN_THREADS) void loudness_gain_kernel(const double* __restrict__ stats, int batch, double target, double limit,
                                                                      int has_limit, double* __restrict__ gain) {
    const int b = blockIdx.x * LD_GAIN_THREADS + threadIdx.x;
    if (b >= batch) return;
    const double l = stats[2 * (int64_t)b], peak = stats[2 * (int64_t)b + 1];
    double g_db = target - l;
    if (has_limit && peak > 0.0) g_db = fmin(g_db, limit - 20.0 * log10(peak));
    if (l == -__builtin_huge_val()) g_db = 0.0;
    gain[2 * (int64_t)b] = g_db;
    gain[2 * (int64_t)b + 1] = pow(10.0, g_db / 20.0);
}

// ---- out = (float)((double)x gain), zeros at and after the clip's length; grid (quads of a row / 256, batch) ----------------------------
// The lengths of the launch's clips (at most RaggedUpload::CAP, clips lens.offset ...) are kernel arguments: the entry takes no scratch.
// VEC: both rows are 16-byte aligned (the host checked the pointers and the strides); the quad that straddles max_samples goes one by one.
template <bool VEC>
__global__ __launch_bounds__(LD_GAIN_THREADS) void apply_gain_kernel(const float* audio, int64_t stride, float* out, int64_t out_stride,
                                                                   int64_t max_samples, int has_lens, RaggedUpload lens,
                                                                   const double* __restrict__ gain, int64_t gain_stride) {
    const int b = lens.offset + blockIdx.y;
    const float* x = audio + (int64_t)b * stride;  // (out may be audio: every thread reads its own quad before it writes it)
    float* y = out + (int64_t)b * out_stride;
    const int64_t n = has_lens ? lens.vals[blockIdx.y] : max_samples;
    const double g = gain[(int64_t)b * gain_stride];
    const int64_t i0 = 4 * ((int64_t)blockIdx.x * LD_GAIN_THREADS + threadIdx.x);
    if (i0 >= max_samples) return;
    if (VEC && i0 + 4 <= max_samples) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i0 < n) v = *reinterpret_cast<const float4*>(x + i0);  // (a quad that starts inside the clip lies inside the row)
        v.x = i0 < n ? (float)((double)v.x * g) : 0.f;
        v.y = i0 + 1 < n ? (float)((double)v.y * g) : 0.f;
        v.z = i0 + 2 < n ? (float)((double)v.z * g) : 0.f;
        v.w = i0 + 3 < n ? (float)((double)v.w * g) : 0.f;
        *reinterpret_cast<float4*>(y + i0) = v;
        return;
    }
    for (int64_t i = i0; i < min(i0 + 4, max_samples); ++i) y[i] = i < n ? (float)((double)x[i] * g) : 0.f;
}

int filter_design(int32_t fs, LoudFilter* f) {
    LD_REQUIRE_RATE(fs);
    // De Man's parametrisation of the two K-weighting stages, evaluated at fs
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(M_PI * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        f->c[0][0] = (Vh + Vb * K / Q + K * K) / a0;
        f->c[0][1] = 2.0 * (K * K - Vh) / a0;
        f->c[0][2] = (Vh - Vb * K / Q + K * K) / a0;
        f->c[0][3] = 2.0 * (K * K - 1.0) / a0;
        f->c[0][4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(M_PI * f0 / fs);
        const double a0 = 1.0 + K / Q + K * K;
        f->c[1][0] = 1.0;
        f->c[1][1] = -2.0;
        f->c[1][2] = 1.0;
        f->c[1][3] = 2.0 * (K * K - 1.0) / a0;
        f->c[1][4] = (1.0 - K / Q + K * K) / a0;
    }
    f->step = fs / 10;
    // M: column k is where the unit state e_k is after one step of zero input, by the passes' own recursion on the fp64 coefficients,
    // run in the host's long double (64 mantissa bits on x86) and kept as hi + lo; where long double is double, lo is zero
    long double c[2][5];
    for (int s = 0; s < 2; ++s)
        for (int i = 0; i < 5; ++i) c[s][i] = f->c[s][i];
    for (int k = 0; k < 4; ++k) {
        long double st[4] = {0.0L, 0.0L, 0.0L, 0.0L};
        st[k] = 1.0L;
        for (int i = 0; i < f->step; ++i) biquad(c[1], biquad(c[0], 0.0L, st[0], st[1]), st[2], st[3]);
        for (int r = 0; r < 4; ++r) {
            f->m[r][k] = (double)st[r];
            f->m_lo[r][k] = (double)(st[r] - (long double)f->m[r][k]);
        }
    }
    return L3AC_OK;
}

// ---- phases 1 to 3 of every entry that needs the step energies: energy[clip][s] and step_max[clip][s] in the caller's scratch ----------------
struct LoudBuffers {
    double *state, *energy;
    float* step_max;
};

int launch_step_energies(hipStream_t s, const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int* lens,
                         const LoudFilter& f, int64_t s_max, const LoudScratch& sc, void* scratch, LoudBuffers* w) {
    char* base = static_cast<char*>(scratch);
    double* state = w->state = reinterpret_cast<double*>(base + sc.state);
    double* energy = w->energy = reinterpret_cast<double*>(base + sc.energy);
    float* step_max = w->step_max = reinterpret_cast<float*>(base + sc.step_max);
    if (s_max <= 0) return L3AC_OK;
    const dim3 grid((unsigned)ceil_div64(s_max, LD_STEPS), (unsigned)batch);
    const double flops = 22.0 * batch * (double)max_samples, bytes = 4.0 * batch * (double)max_samples;
    {
        ProfScope prof(s, "loudness_pass_kernel<state>", flops, bytes);
        hipLaunchKernelGGL(loudness_pass_kernel<false>, grid, dim3(LD_STEPS), 0, s, audio, audio_stride, max_samples, lens, f, s_max, state, energy,
                           step_max);
        L3AC_LAUNCH_CHECK();
    }
    {
        ProfScope prof(s, "loudness_scan_kernel", 32.0 * batch * (double)s_max, 64.0 * batch * (double)s_max);
        hipLaunchKernelGGL(loudness_scan_kernel, dim3((unsigned)ceil_div64(batch, 64)), dim3(64), 0, s, batch, max_samples, lens, f, s_max, state);
        L3AC_LAUNCH_CHECK();
    }
    {
        ProfScope prof(s, "loudness_pass_kernel<energy>", flops, bytes);
        hipLaunchKernelGGL(loudness_pass_kernel<true>, grid, dim3(LD_STEPS), 0, s, audio, audio_stride, max_samples, lens, f, s_max, state, energy,
                           step_max);
        L3AC_LAUNCH_CHECK();
    }
    return L3AC_OK;
}

// ---- EBU R128 on the step energies: the block series of any window, and the loudness range ---------------------------------
// A block of W steps that starts at step k: z_k = (((e_k + e_{k+1}) + ...) + e_{k+W-1}) / (W step), summed left to right (W = 4: the
// mean_square of loudness_gate_kernel bit for bit), l_k = -0.691 + 10 log10 z_k.  A clip of `steps` whole steps has max(steps - W + 1, 0).
constexpr int LD_SERIES_THREADS = 256;
constexpr int LD_MAX_WINDOW = 600;       // steps: 60 s
constexpr int LD_SHORT_STEPS = 30;       // the short-term window, 3 s
constexpr int LD_RANGE_THREADS = PAIR_THREADS;

__device__ __forceinline__ double block_mean_square(const double* __restrict__ e, int64_t k, int w, double norm) {
    double sum = e[k];
    for (int i = 1; i < w; ++i) sum = sum + e[k + i];
    return sum / norm;
}

__device__ __forceinline__ double lkfs_of(double z) { return -0.691 + 10.0 * log10(z); }  // (-inf for z = 0)

// grid (ceil(max(k_max, s_max) / 256), batch): lufs [batch][k_max] (-inf at and after the clip's own blocks), mean_square [batch][k_max] or
// null (0 there), energies [batch][s_max] or null (the step energies, 0 at and after the clip's own steps), blocks_out [batch] or null
__global__ __launch_bounds__(LD_SERIES_THREADS) void loudness_series_kernel(int64_t max_samples, const int* __restrict__ lens, int step, int window,
                                                                          int64_t s_max, int64_t k_max, const double* __restrict__ energy,
                                                                          double* __restrict__ lufs, double* __restrict__ mean_square,
                                                                          double* __restrict__ energies, int* __restrict__ blocks_out) {
    const int b = blockIdx.y;
    const int64_t steps = (lens ? lens[b] : max_samples) / step;
    const int64_t blocks = steps >= window ? steps - window + 1 : 0;
    const double* e = energy + (int64_t)b * s_max;
    const int64_t k = (int64_t)blockIdx.x * LD_SERIES_THREADS + threadIdx.x;
    if (k < k_max) {
        const double z = k < blocks ? block_mean_square(e, k, window, (double)window * (double)step) : 0.0;
        lufs[(int64_t)b * k_max + k] = k < blocks ? lkfs_of(z) : -__builtin_huge_val();
        if (mean_square) mean_square[(int64_t)b * k_max + k] = z;
    }
    if (energies && k < s_max) energies[(int64_t)b * s_max + k] = k < steps ? e[k] : 0.0;
    if (blocks_out && k == 0) blocks_out[b] = (int)blocks;
}

// One workgroup per clip, the clip's short-term z_k in LDS (at most PAIR_MAX_FRAMES of them: the host checked): EBU Tech 3342 on blocks of
// 3 s every 100 ms.  The gates decide on l values as loudness_gate_kernel does; the relative gate lies 20 LU below the absolutely gated level.
// The survivors' z, +inf elsewhere up to n_pad, are sorted ascending; the percentiles are picks, in integer arithmetic.
// stats [b][5] = lra, low, high, short_term_max, momentary_max; counts [b][3] = blocks, above the absolute gate, gated.
__global__ __launch_bounds__(LD_RANGE_THREADS) void loudness_range_kernel(int64_t max_samples, const int* __restrict__ lens, int step, int64_t s_max,
                                                                        int n_pad_max, const double* __restrict__ energy, double* __restrict__ stats,
                                                                        int* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) double range_z[];  // [n_pad_max]
    __shared__ double lds[LD_RANGE_THREADS / 64];
    const int b = blockIdx.x;
    const int64_t steps = (lens ? lens[b] : max_samples) / step;
    const int blocks = (int)std::min<int64_t>(steps >= LD_SHORT_STEPS ? steps - LD_SHORT_STEPS + 1 : 0, n_pad_max);  // (the clamp bounds every index)
    const int64_t blocks4 = steps > 3 ? steps - 3 : 0;
    const double* e = energy + (int64_t)b * s_max;
    const double ninf = -__builtin_huge_val();
    int n_pad = 1;
    while (n_pad < blocks) n_pad <<= 1;

    // the momentary maximum over the 400 ms blocks
    double mom = ninf;
    for (int64_t j = threadIdx.x; j < blocks4; j += LD_RANGE_THREADS) mom = fmax(mom, lkfs_of(block_mean_square(e, j, 4, 4.0 * (double)step)));
    mom = block_max<LD_RANGE_THREADS>(mom, lds);

    // the short-term blocks, their maximum, the absolute gate
    double st = ninf, sum = 0.0, cnt = 0.0;
    for (int k = threadIdx.x; k < blocks; k += LD_RANGE_THREADS) {
        const double z = block_mean_square(e, k, LD_SHORT_STEPS, (double)LD_SHORT_STEPS * (double)step), l = lkfs_of(z);
        range_z[k] = z;
        st = fmax(st, l);
        if (l > -70.0) sum += z, cnt += 1.0;
    }
    st = block_max<LD_RANGE_THREADS>(st, lds);
    sum = block_sum<LD_RANGE_THREADS>(sum, lds);
    cnt = block_sum<LD_RANGE_THREADS>(cnt, lds);  // (whole numbers below 2^31: exact)
    // the relative gate (no absolutely gated block: nothing passes); every thread rewrites the elements it wrote
    const double gamma = lkfs_of(sum / cnt) - 20.0;
    double kept = 0.0;
    for (int k = threadIdx.x; k < n_pad; k += LD_RANGE_THREADS) {
        double keep = __builtin_huge_val();
        if (k < blocks && cnt > 0.0) {
            const double z = range_z[k], l = lkfs_of(z);
            if (l > -70.0 && l > gamma) keep = z, kept += 1.0;
        }
        range_z[k] = keep;
    }
    kept = block_sum<LD_RANGE_THREADS>(kept, lds);  // (its barriers publish range_z)
    lds_sort<LD_RANGE_THREADS>(range_z, n_pad);
    if (threadIdx.x == 0) {
        const int g = (int)kept;
        double low = ninf, high = ninf, lra = 0.0;
        if (g > 0) {
            low = lkfs_of(range_z[((g - 1) * 10 + 50) / 100]);
            high = lkfs_of(range_z[((g - 1) * 95 + 50) / 100]);
            lra = high - low;
        }
        double* out = stats + 5 * (int64_t)b;
        out[0] = lra, out[1] = low, out[2] = high, out[3] = st, out[4] = mom;
        counts[3 * (int64_t)b] = blocks, counts[3 * (int64_t)b + 1] = (int)cnt, counts[3 * (int64_t)b + 2] = g;
    }
}

int configure_range_kernel() {
    static PerDeviceOnce configured;
    return raise_dynamic_lds(configured, {{loudness_range_kernel, PAIR_MAX_FRAMES * 8}});
}

// what the series and the range share with l3ac_loudness: the checks, the staged lengths, the design, phases 1 to 3
int step_energies_of(hipStream_t s, const char* what, const char* entry, const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples,
                     const int32_t* samples, int32_t sample_rate, void* scratch, int64_t scratch_bytes, int64_t s_max, const LoudScratch& sc,
                     LoudFilter* f, int** lens, LoudBuffers* w) {
    L3AC_TRY(stage_clip_lengths(s, what, entry, samples, batch, scratch, scratch_bytes, sc.total_min, lens));
    L3AC_TRY(filter_design(sample_rate, f));
    return launch_step_energies(s, audio, audio_stride, batch, max_samples, *lens, *f, s_max, sc, scratch, w);
}

}  // namespace

extern "C" {

int64_t l3ac_loudness_coeffs(int32_t sample_rate, double* out, int64_t cap) {
    LoudFilter f;
    L3AC_TRY(filter_design(sample_rate, &f));
    const int64_t need = 2 * 6 + 16;
    if (!out || cap < need) return need;
    for (int s = 0; s < 2; ++s) {
        double* row = out + 6 * s;
        row[0] = f.c[s][0], row[1] = f.c[s][1], row[2] = f.c[s][2], row[3] = 1.0, row[4] = f.c[s][3], row[5] = f.c[s][4];
    }
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) out[12 + 4 * r + k] = f.m[r][k];
    return need;
}

int64_t l3ac_loudness_blocks(int64_t samples, int32_t sample_rate) {
    LD_REQUIRE_RATE(sample_rate);
    L3AC_REQUIRE(samples >= 1, "loudness_blocks: samples %lld must be positive", (long long)samples);
    return std::max<int64_t>(samples / (sample_rate / 10) - 3, 0);
}

int64_t l3ac_loudness_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sample_rate) {
    int64_t s_max;
    LoudScratch sc;
    L3AC_TRY(loud_geom(batch, max_samples, sample_rate, &s_max, &sc));
    return sc.total_min;
}

int l3ac_loudness(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, int32_t sample_rate,
                  double* stats, int32_t* counts, double* momentary, void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    int64_t s_max;
    LoudScratch sc;
    L3AC_TRY(loud_geom(batch, max_samples, sample_rate, &s_max, &sc));
    L3AC_REQUIRE(audio && stats && counts, "loudness: null buffer");
    L3AC_REQUIRE(batch == 1 || audio_stride >= max_samples, "loudness: row stride %lld below max_samples %lld", (long long)audio_stride,
                 (long long)max_samples);
    L3AC_TRY(check_clip_lengths("loudness", samples, batch, max_samples));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "loudness", "loudness", samples, batch, scratch, scratch_bytes, sc.total_min, &lens));
    LoudFilter f;
    L3AC_TRY(filter_design(sample_rate, &f));
    LoudBuffers w;
    L3AC_TRY(launch_step_energies(s, audio, audio_stride, batch, max_samples, lens, f, s_max, sc, scratch, &w));
    double* energy = w.energy;
    float* step_max = w.step_max;
    const int64_t j_max = std::max<int64_t>(s_max - 3, 0);

    ProfScope prof(s, "loudness_gate_kernel", 0.0, 12.0 * batch * (double)s_max);
    hipLaunchKernelGGL(loudness_gate_kernel, dim3((unsigned)batch), dim3(LD_GATE_THREADS), 0, s, audio, audio_stride, max_samples, lens, f.step, s_max,
                       j_max, energy, step_max, stats, counts, j_max > 0 ? momentary : nullptr);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

int l3ac_loudness_gain(const double* stats, int32_t batch, double target_lufs, double peak_limit_db, double* gain, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    L3AC_REQUIRE(batch > 0 && batch <= 65535, "loudness_gain: batch %d outside 1..65535", batch);
    L3AC_REQUIRE(std::isfinite(target_lufs), "loudness_gain: target_lufs must be finite");
    L3AC_REQUIRE(stats && gain, "loudness_gain: null buffer");
    const bool has_limit = !std::isnan(peak_limit_db);
    ProfScope prof(s, "loudness_gain_kernel", 0.0, 32.0 * batch);
    hipLaunchKernelGGL(loudness_gain_kernel, dim3((unsigned)ceil_div64(batch, LD_GAIN_THREADS)), dim3(LD_GAIN_THREADS), 0, s, stats, batch, target_lufs,
                       has_limit ? peak_limit_db : 0.0, has_limit ? 1 : 0, gain);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

int l3ac_apply_gain(const float* audio, int64_t audio_stride, float* out, int64_t out_stride, int32_t batch, int64_t max_samples,
                    const int32_t* samples, const double* gain, int64_t gain_stride, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    L3AC_TRY(check_clip_batch("apply_gain", batch, max_samples));
    L3AC_REQUIRE(audio && out && gain, "apply_gain: null buffer");
    L3AC_REQUIRE(batch == 1 || (audio_stride >= max_samples && out_stride >= max_samples), "apply_gain: row stride below max_samples %lld",
                 (long long)max_samples);
    L3AC_REQUIRE(gain_stride >= 1, "apply_gain: gain_stride %lld must be positive", (long long)gain_stride);
    L3AC_TRY(check_clip_lengths("loudness", samples, batch, max_samples));  // (this one message has always said "loudness")
    const bool vec = (((uintptr_t)audio | (uintptr_t)out) & 15) == 0 && (batch == 1 || ((audio_stride | out_stride) & 3) == 0);
    return for_each_length_group(samples, batch, [&](const RaggedUpload& blk) -> int {
        const dim3 grid((unsigned)ceil_div64(ceil_div64(max_samples, 4), LD_GAIN_THREADS), (unsigned)blk.n);
        ProfScope prof(s, "apply_gain_kernel", 1.0 * blk.n * (double)max_samples, 8.0 * blk.n * (double)max_samples);
        if (vec)
            hipLaunchKernelGGL(apply_gain_kernel<true>, grid, dim3(LD_GAIN_THREADS), 0, s, audio, audio_stride, out, out_stride, max_samples,
                               samples ? 1 : 0, blk, gain, gain_stride);
        else
            hipLaunchKernelGGL(apply_gain_kernel<false>, grid, dim3(LD_GAIN_THREADS), 0, s, audio, audio_stride, out, out_stride, max_samples,
                               samples ? 1 : 0, blk, gain, gain_stride);
        L3AC_LAUNCH_CHECK();
        return L3AC_OK;
    });
}

int64_t l3ac_r128_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sample_rate) {
    int64_t s_max;
    LoudScratch sc;
    L3AC_TRY(loud_geom(batch, max_samples, sample_rate, &s_max, &sc));
    return sc.total_min;
}

int l3ac_r128_series(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, int32_t sample_rate,
                     int32_t window_steps, double* lufs, double* mean_square, double* energies, int32_t* blocks, void* scratch, int64_t scratch_bytes,
                     void* stream) {
    hipStream_t s = (hipStream_t)stream;
    int64_t s_max;
    LoudScratch sc;
    L3AC_TRY(loud_geom(batch, max_samples, sample_rate, &s_max, &sc));
    L3AC_REQUIRE(window_steps >= 1 && window_steps <= LD_MAX_WINDOW, "r128_series: window_steps %d outside 1..%d", window_steps, LD_MAX_WINDOW);
    const int64_t k_max = std::max<int64_t>(s_max - window_steps + 1, 0);
    L3AC_REQUIRE(audio && (lufs || k_max == 0), "r128_series: null buffer");
    L3AC_REQUIRE(batch == 1 || audio_stride >= max_samples, "r128_series: row stride %lld below max_samples %lld", (long long)audio_stride,
                 (long long)max_samples);
    L3AC_TRY(check_clip_lengths("r128_series", samples, batch, max_samples));
    LoudFilter f;
    int* lens;
    LoudBuffers w;
    L3AC_TRY(step_energies_of(s, "r128_series", "r128", audio, audio_stride, batch, max_samples, samples, sample_rate, scratch, scratch_bytes, s_max, sc,
                              &f, &lens, &w));
    const int64_t cells = std::max<int64_t>(std::max(k_max, energies ? s_max : 0), 1);  // (one workgroup a clip at least: the block counts)
    ProfScope prof(s, "loudness_series_kernel", 1.0 * window_steps * batch * (double)k_max, 24.0 * batch * (double)s_max);
    hipLaunchKernelGGL(loudness_series_kernel, dim3((unsigned)ceil_div64(cells, LD_SERIES_THREADS), (unsigned)batch), dim3(LD_SERIES_THREADS), 0, s,
                       max_samples, lens, f.step, window_steps, s_max, k_max, w.energy, lufs, k_max > 0 ? mean_square : nullptr,
                       s_max > 0 ? energies : nullptr, blocks);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

int l3ac_r128_range(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, int32_t sample_rate,
                    double* stats, int32_t* counts, void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    int64_t s_max;
    LoudScratch sc;
    L3AC_TRY(loud_geom(batch, max_samples, sample_rate, &s_max, &sc));
    L3AC_REQUIRE(audio && stats && counts, "r128_range: null buffer");
    L3AC_REQUIRE(batch == 1 || audio_stride >= max_samples, "r128_range: row stride %lld below max_samples %lld", (long long)audio_stride,
                 (long long)max_samples);
    L3AC_TRY(check_clip_lengths("r128_range", samples, batch, max_samples));
    // the short-term blocks of the longest clip live in one workgroup's LDS
    int64_t longest = samples ? 0 : max_samples;
    for (int i = 0; samples && i < batch; ++i) longest = std::max<int64_t>(longest, samples[i]);
    const int64_t k_most = std::max<int64_t>(longest / (sample_rate / 10) - LD_SHORT_STEPS + 1, 0);
    L3AC_REQUIRE(k_most <= PAIR_MAX_FRAMES, "r128_range: %lld short-term blocks are more than the %d of a clip", (long long)k_most, PAIR_MAX_FRAMES);
    int n_pad = 1;
    while (n_pad < k_most) n_pad <<= 1;
    LoudFilter f;
    int* lens;
    LoudBuffers w;
    L3AC_TRY(step_energies_of(s, "r128_range", "r128", audio, audio_stride, batch, max_samples, samples, sample_rate, scratch, scratch_bytes, s_max, sc,
                              &f, &lens, &w));
    L3AC_TRY(configure_range_kernel());
    ProfScope prof(s, "loudness_range_kernel", 34.0 * batch * (double)s_max, 8.0 * 34 * batch * (double)s_max);
    hipLaunchKernelGGL(loudness_range_kernel, dim3((unsigned)batch), dim3(LD_RANGE_THREADS), (size_t)n_pad * 8, s, max_samples, lens, f.step, s_max, n_pad,
                       w.energy, stats, counts);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

}  // extern "C"
