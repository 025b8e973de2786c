// Polyphase sample-rate conversion: scipy.signal.resample_poly with its defaults (include/l3ac_hip.h, "sample-rate
// conversion").
//
// For in_rate a and out_rate b: g = gcd(a, b), up = b / g, down = a / g, M = max(up, down), half_len = 10 M, prototype
// h = firwin(2 half_len + 1, 1 / M, window = ('kaiser', 5.0)) * up (designed here, on the host, in fp64), and
//   y[m] = sum_j h[j] * xu[m down + half_len - j],   xu[n] = x[n / up] when up | n and 0 <= n / up < n_in, else 0,
// for m < n_out = ceil(n_in up / down).  In polyphase form output m has phase p = (m down + half_len) mod up and newest input
// i = (m down + half_len) div up; with K = ceil((2 half_len + 1) / up) and s = i - (K - 1) (its oldest input),
//   y[m] = sum_{t < K} g_p[t] * x[s + t],   g_p[t] = h[p + (K - 1 - t) up]   (0 past the end of h).
//
// Kernel: the 64 lanes of a wave are 64 CLIPS, all computing the same output index m.  The phase, and with it every tap, is then
// the same across the wave: taps are scalar loads (SGPRs), and each lane reads its own clip's inputs from an LDS window
// [64 clips][pitch] at a wave-uniform column, four at a time (ds_read_b128, conflict-free: pitch = 4 mod 8).  A quad read needs a
// column that is a multiple of 4; the bank holds each phase four times, as (0 x v, g_p) for v = 0 .. 3, and an output whose s is
// v mod 4 reads from s - v with variant v.  Windows start at multiples of 4, so which variant an output uses depends on m alone.  A
// zero tap adds +0 to a sum that starts at +0 (or is nonzero): every output is the fp32 fmaf chain over t = 0 .. K-1 in that order,
// whatever the batch, the clip's position, the input stride or the launch geometry.
// A workgroup (4 waves) owns 64 clips x n_blk consecutive outputs (wave w: outputs w, w + 4, ...); long filters are walked in
// chunks of RS_TAP_CHUNK taps, each chunk restaging the window.  Outputs are staged through LDS and stored as coalesced rows.
#include "../kernels.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace {

constexpr int RS_CLIPS = 64;       // lanes = clips
constexpr int RS_MAX_OUT = 64;     // outputs per workgroup (per clip)
constexpr int RS_OUT_PER_WAVE = RS_MAX_OUT / 4;
constexpr int RS_TAP_CHUNK = 64;   // taps per staged window (multiple of 4)
constexpr int RS_SPAN = 112;       // max inputs between a workgroup's first and last output: keeps LDS <= 64 KiB
constexpr int RS_MAX_FACTOR = 1024;
constexpr int RS_MAX_PITCH = 184;  // >= RS_SPAN + 3 + RS_TAP_CHUNK, rounded up to 4 mod 8
constexpr int RS_STAGE_QUADS = (RS_CLIPS * RS_MAX_PITCH / 4 + 255) / 256;  // window quads per thread

struct RsGeom {
    int64_t n_in, n_out, x_stride, y_stride;
    int batch, up, down, half_len, K, KE;  // KE: row length of a bank entry (multiple of 4, >= K + 3)
    int n_blk_out, pitch, ys_pitch;
};

__global__ __launch_bounds__(256) void resample_poly_kernel(const float* __restrict__ x, const float* __restrict__ bank,
                                                            float* __restrict__ y, RsGeom g) {
    extern __shared__ float rs_lds[];
    float* xs = rs_lds;                         // [64][pitch]  input window of the current tap chunk
    float* ys = rs_lds + RS_CLIPS * g.pitch;    // [64][ys_pitch] results
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b0 = blockIdx.y * RS_CLIPS;
    const int64_t m0 = (int64_t)blockIdx.x * g.n_blk_out;
    const int n_blk = (int)min((int64_t)g.n_blk_out, g.n_out - m0);

    auto oldest = [&](int64_t m, int& phase) -> int64_t {  // s of output m, and its phase (wave-uniform: scalar arithmetic)
        const int64_t q = m * g.down + g.half_len;
        if (q <= 0x7fffffff) {  // the 32-bit division, far shorter than the 64-bit one
            const uint32_t q32 = (uint32_t)q, up = (uint32_t)g.up;
            phase = (int)(q32 % up);
            return (int64_t)(q32 / up) - (g.K - 1);
        }
        phase = (int)(q % g.up);
        return q / g.up - (g.K - 1);
    };
    // 16-B loads of the window when every row start is 16-B aligned (w0 is a multiple of 4 inputs)
    const bool vec = ((reinterpret_cast<uintptr_t>(x) & 15) == 0) && (g.x_stride % 4 == 0 || g.batch == 1);
    int ph;
    const int64_t w_base = oldest(m0, ph) & ~(int64_t)3;
    const int span = (int)((oldest(m0 + n_blk - 1, ph) & ~(int64_t)3) - w_base);

    float acc[RS_OUT_PER_WAVE];
#pragma unroll
    for (int j = 0; j < RS_OUT_PER_WAVE; ++j) acc[j] = 0.f;

    for (int t0 = 0; t0 < g.KE; t0 += RS_TAP_CHUNK) {
        const int tc = min(RS_TAP_CHUNK, g.KE - t0);
        const int wc = min(span + tc, g.pitch);  // == span + tc: the host sized pitch for the largest span
        if (t0) __syncthreads();                 // every wave is done with the previous chunk's window
        const int64_t w0 = w_base + t0;
        // the window as 64 rows x wq quads; every load of a thread issued before the first LDS write, so that their latencies overlap
        const int wq = (wc + 3) >> 2;  // 4 wq <= pitch: pitch is a multiple of 4 >= wc
        const int nq = RS_CLIPS * wq;
        float4 v[RS_STAGE_QUADS];
#pragma unroll
        for (int k = 0; k < RS_STAGE_QUADS; ++k) {
            const int e = threadIdx.x + 256 * k;
            v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e < nq) {
                const int r = e / wq, b = b0 + r;
                const int64_t i = w0 + 4 * (e - r * wq);
                const float* src = x + (int64_t)min(b, g.batch - 1) * g.x_stride;
                if (b < g.batch) {
                    if (vec && i >= 0 && i + 3 < g.n_in) {
                        v[k] = *reinterpret_cast<const float4*>(src + i);
                    } else {
                        if (i >= 0 && i < g.n_in) v[k].x = src[i];
                        if (i + 1 >= 0 && i + 1 < g.n_in) v[k].y = src[i + 1];
                        if (i + 2 >= 0 && i + 2 < g.n_in) v[k].z = src[i + 2];
                        if (i + 3 >= 0 && i + 3 < g.n_in) v[k].w = src[i + 3];
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < RS_STAGE_QUADS; ++k) {
            const int e = threadIdx.x + 256 * k;
            if (e < nq) {
                const int r = e / wq;
                *reinterpret_cast<float4*>(xs + r * g.pitch + 4 * (e - r * wq)) = v[k];
            }
        }
        __syncthreads();
        const float* xr = xs + lane * g.pitch;
#pragma unroll
        for (int j = 0; j < RS_OUT_PER_WAVE; ++j) {
            const int o = wave + 4 * j;
            if (o < n_blk) {
                int phase;
                const int64_t s = oldest(m0 + o, phase);
                const int col = (int)((s & ~(int64_t)3) - w_base);
                const float* gt = bank + (int64_t)(4 * phase + (int)(s & 3)) * g.KE + t0;
                const float* xp = xr + col;
                float a = acc[j];
#pragma unroll 4
                for (int t = 0; t < tc; t += 4) {
                    const float4 xv = *reinterpret_cast<const float4*>(xp + t);
                    a = fmaf(gt[t], xv.x, a);
                    a = fmaf(gt[t + 1], xv.y, a);
                    a = fmaf(gt[t + 2], xv.z, a);
                    a = fmaf(gt[t + 3], xv.w, a);
                }
                acc[j] = a;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < RS_OUT_PER_WAVE; ++j) {
        const int o = wave + 4 * j;
        if (o < n_blk) ys[lane * g.ys_pitch + o] = acc[j];
    }
    __syncthreads();
    for (int r = wave; r < RS_CLIPS && b0 + r < g.batch; r += 4)
        if (lane < n_blk) y[(int64_t)(b0 + r) * g.y_stride + m0 + lane] = ys[r * g.ys_pitch + lane];
}

double bessel_i0(double x) {  // power series; x <= 5 here, converged long before 60 terms
    double sum = 1.0, term = 1.0;
    const double q = 0.25 * x * x;
    for (int k = 1; k < 60; ++k) {
        term *= q / ((double)k * k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

}  // namespace

int resample_plan(int32_t in_rate, int32_t out_rate, ResamplePlan* p) {
    L3AC_REQUIRE(in_rate > 0 && out_rate > 0, "resample: rates must be positive (got %d -> %d)", in_rate, out_rate);
    const int64_t gc = std::gcd((int64_t)in_rate, (int64_t)out_rate);
    p->up = (int)(out_rate / gc);
    p->down = (int)(in_rate / gc);
    const int64_t M = std::max(p->up, p->down);
    L3AC_REQUIRE(M <= RS_MAX_FACTOR, "resample: %d -> %d reduces to up %d / down %d; max(up, down) must be <= %d", in_rate,
                 out_rate, p->up, p->down, RS_MAX_FACTOR);
    p->half_len = (int)(10 * M);
    p->K = (int)ceil_div64(2 * (int64_t)p->half_len + 1, p->up);
    p->KE = 4 * (int)ceil_div64(p->K + 3, 4);
    return L3AC_OK;
}

int64_t resample_length(const ResamplePlan& p, int64_t n_in) { return ceil_div64(n_in * p.up, p.down); }

int64_t resample_bank_floats(const ResamplePlan& p) { return p.up == p.down ? 0 : (int64_t)p.up * 4 * p.KE; }

void resample_phase_taps(const ResamplePlan& p, float* taps) {
    const int M = std::max(p.up, p.down);
    const int n = 2 * p.half_len + 1;
    // firwin(n, 1 / M, window=('kaiser', 5.0)), scipy's arithmetic: h = c sinc(c (k - alpha)) w[k], normalised to unit sum
    std::vector<double> h(n);
    const double c = 1.0 / M, alpha = 0.5 * (n - 1), beta = 5.0, i0b = bessel_i0(beta);
    double sum = 0.0;
    for (int k = 0; k < n; ++k) {
        const double m = k - alpha;
        const double arg = M_PI * (c * m);
        const double sinc = (m == 0.0) ? 1.0 : std::sin(arg) / arg;
        const double r = m / alpha;
        h[k] = c * sinc * (bessel_i0(beta * std::sqrt(1.0 - r * r)) / i0b);
        sum += h[k];
    }
    for (int k = 0; k < n; ++k) h[k] = h[k] / sum * p.up;
    for (int ph = 0; ph < p.up; ++ph)
        for (int t = 0; t < p.K; ++t) {
            const int64_t j = ph + (int64_t)(p.K - 1 - t) * p.up;
            taps[(int64_t)ph * p.K + t] = j < n ? (float)h[j] : 0.f;
        }
}

void resample_fill_bank(const ResamplePlan& p, float* bank) {
    std::vector<float> taps((size_t)p.up * p.K);
    resample_phase_taps(p, taps.data());
    // bank[phase][v][KE], v = 0 .. 3: v zeros, then g_p[0 .. K), zero-padded to KE
    for (int ph = 0; ph < p.up; ++ph) {
        float* rows = bank + (int64_t)ph * 4 * p.KE;
        for (int t = 0; t < 4 * p.KE; ++t) rows[t] = 0.f;
        for (int t = 0; t < p.K; ++t)
            for (int v = 0; v < 4; ++v) rows[v * p.KE + v + t] = taps[(size_t)ph * p.K + t];
    }
}

extern "C" {

int64_t l3ac_resample_length(int32_t in_rate, int32_t out_rate, int64_t n_in) {
    ResamplePlan p;
    L3AC_TRY(resample_plan(in_rate, out_rate, &p));
    L3AC_REQUIRE(n_in >= 0 && n_in <= (INT64_MAX / 1024), "resample: bad input length %lld", (long long)n_in);
    return resample_length(p, n_in);
}

int64_t l3ac_resample_bank(int32_t in_rate, int32_t out_rate, float* bank, int64_t cap) {
    ResamplePlan p;
    L3AC_TRY(resample_plan(in_rate, out_rate, &p));
    const int64_t need = resample_bank_floats(p);
    if (bank && need > 0 && cap >= need) resample_fill_bank(p, bank);
    return need;
}

int l3ac_resample(const float* x, int32_t batch, int64_t n_in, int64_t x_stride, int32_t in_rate, int32_t out_rate, const float* bank,
                  float* y, int64_t y_stride, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    ResamplePlan p;
    L3AC_TRY(resample_plan(in_rate, out_rate, &p));
    L3AC_REQUIRE(x && y, "resample: null buffer");
    L3AC_REQUIRE(batch > 0 && n_in > 0, "resample: empty input (batch %d, n_in %lld)", batch, (long long)n_in);
    L3AC_REQUIRE(x_stride >= n_in || batch == 1, "resample: input row stride %lld < n_in %lld", (long long)x_stride, (long long)n_in);
    const int64_t n_out = resample_length(p, n_in);
    L3AC_REQUIRE(y_stride >= n_out || batch == 1, "resample: output row stride %lld < n_out %lld", (long long)y_stride, (long long)n_out);
    if (p.up == p.down) {
        L3AC_HIP_CHECK(hipMemcpy2DAsync(y, (size_t)(batch > 1 ? y_stride : n_out) * 4, x, (size_t)(batch > 1 ? x_stride : n_in) * 4,
                                        (size_t)n_in * 4, (size_t)batch, hipMemcpyDeviceToDevice, s));
        return L3AC_OK;
    }
    L3AC_REQUIRE(bank, "resample: null filter bank (l3ac_resample_bank, copied to the device)");
    RsGeom g{};
    g.n_in = n_in;
    g.n_out = n_out;
    g.x_stride = x_stride;
    g.y_stride = y_stride;
    g.batch = batch;
    g.up = p.up;
    g.down = p.down;
    g.half_len = p.half_len;
    g.K = p.K;
    g.KE = p.KE;
    // outputs per workgroup: as many as keep the input span <= RS_SPAN (and <= RS_MAX_OUT)
    g.n_blk_out = (int)std::min<int64_t>(RS_MAX_OUT, (int64_t)RS_SPAN * p.up / p.down + 1);
    // span between the first and the last output's oldest input, each rounded down to a multiple of 4:
    // <= ceil((n_blk - 1) down / up) + 3
    const int64_t span_max = ceil_div64((int64_t)(g.n_blk_out - 1) * p.down, p.up) + 3;
    const int64_t cols = span_max + std::min(RS_TAP_CHUNK, p.KE);
    g.pitch = (int)(cols + ((4 - cols % 8) + 8) % 8);  // >= cols, == 4 mod 8: quad reads of 16 rows hit distinct bank slots
    g.ys_pitch = g.n_blk_out | 1;
    L3AC_REQUIRE(g.pitch <= RS_MAX_PITCH, "resample: internal window pitch %d > %d", g.pitch, RS_MAX_PITCH);
    const size_t lds = (size_t)RS_CLIPS * (g.pitch + g.ys_pitch) * sizeof(float);
    L3AC_REQUIRE(lds <= 65536, "resample: internal LDS budget exceeded (%zu B)", lds);
    const int64_t gx = ceil_div64(n_out, g.n_blk_out), gy = ceil_div64(batch, RS_CLIPS);
    L3AC_REQUIRE(gx <= 0x7fffffff, "resample: output too long (%lld samples)", (long long)n_out);
    ProfScope prof(s, "resample_poly_kernel", 2.0 * batch * n_out * p.K, 4.0 * batch * (n_in + n_out));
    hipLaunchKernelGGL(resample_poly_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), lds, s, x, bank, y, g);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

}  // extern "C"
