// Decoder "EnhanceBlock" front end and the output head.
//
// EnhanceBlock (reference l3ac/tconv/__init__.py:30-44): from CHANNEL 0 of x only, four trend branches
//   p_k = avg_pool(max_pool(|x0|, k), k), k in {1 (identity), 3, 5, 9}
//   -> weight-normed Conv1d(1 -> 1, k7, dilation k//2 + 1 = {1, 2, 3, 5}, pad 3*dil)
//   -> InstanceNorm1d(4, affine) over the frames of each clip -> plain Conv1d(4 -> C, 1) -> x + y * x.
// Here: `enhance_branches` writes the four raw branch signals yi [batch][frames][4]; `enhance_stats` centres them in place
// (yi - mean) and reduces them to 1/sqrt(var + 1e-5) per (clip, branch); the normalise + merge + gate is the SRC_GATE row kernel.
//
// Output head (l3ac/modules.py:192-194): weight-normed Conv1d(c -> 1, k7, pad 3) -> tanh on the snake-activated
// last feature map.
#include "../kernels.hpp"

namespace {

constexpr int TILE = 256;
constexpr int XH = 23;  // 3*5 (conv reach at dilation 5) + 4 (avg 9) + 4 (max 9)

// RAGGED (a ragged batch): clip b's pools and convs end at its own last frame rn[b] * rmult — x at and after
// it reads as 0, as do the pooled values there: the zero padding of the clip alone.  `frames` stays the batch's row count.
template <bool RAGGED>
__global__ __launch_bounds__(TILE) void enhance_branches_kernel(const EnhanceW w, const float* __restrict__ x,
                                                               int frames, int c, float* __restrict__ yi,
                                                               const int* __restrict__ rn, int rmult) {
    __shared__ float xs[TILE + 2 * XH];
    __shared__ float mbuf[TILE + 30 + 8];
    __shared__ float pbuf[TILE + 30];
    const int tid = threadIdx.x;
    const int b = blockIdx.y;
    const int t0 = blockIdx.x * TILE;
    const float* clip = x + (int64_t)b * frames * c;
    for (int i = tid; i < TILE + 2 * XH; i += TILE) {
        const int u = t0 - XH + i;
        xs[i] = (u >= 0 && u < (RAGGED ? rn[b] * rmult : frames)) ? clip[(int64_t)u * c] : 0.f;
    }
    __syncthreads();

    float out[4];
    // The seven taps are summed in fp64 and rounded once.  An fp32 fma chain from the bias rounds seven times at the bias's magnitude;
    // for a quiet channel 0 (1e-6: the taps are far below an ulp of the bias) that is most of what the InstanceNorm then multiplies
    // by 1/std = 316, and it left the gate 1.6 - 1.9 x less accurate than the fp32 oracle, whose conv adds the bias last
    // (tests/test_gpu_trend_front.py).  28 fp64 fmas per frame, next to a gather of channel 0 at a stride of c floats.
    {  // branch 0: identity pool, dilation 1
        double acc = (double)w.tb[0];
#pragma unroll
        for (int j = 0; j < 7; ++j) acc = fma((double)w.tw[j], (double)xs[XH + tid + j - 3], acc);
        out[0] = (float)acc;
    }
    const int pool_k[3] = {3, 5, 9};
#pragma unroll
    for (int br = 0; br < 3; ++br) {
        const int k = pool_k[br];
        const int hk = k >> 1;
        const int dil = hk + 1;  // pool_kernel // dilation_rate(2) + 1 (tconv/base.py:34)
        const int reach = 3 * dil;
        const int m_len = TILE + 2 * reach + 2 * hk;
        for (int i = tid; i < m_len; i += TILE) {
            const int v = t0 - reach - hk + i;
            float m = 0.f;
            if (v >= 0 && v < (RAGGED ? rn[b] * rmult : frames)) {
                const int base = v - hk - (t0 - XH);
                for (int s = 0; s < k; ++s) m = fmaxf(m, fabsf(xs[base + s]));
            }
            mbuf[i] = m;
        }
        __syncthreads();
        for (int i = tid; i < TILE + 2 * reach; i += TILE) {
            const int u = t0 - reach + i;
            float pv = 0.f;
            if (u >= 0 && u < (RAGGED ? rn[b] * rmult : frames)) {
                float sum = 0.f;
                for (int s = 0; s < k; ++s) {
                    const int v = u - hk + s;
                    if (v >= 0 && v < (RAGGED ? rn[b] * rmult : frames)) sum += mbuf[i + s];
                }
                pv = sum / (float)k;
            }
            pbuf[i] = pv;
        }
        __syncthreads();
        double acc = (double)w.tb[br + 1];
#pragma unroll
        for (int j = 0; j < 7; ++j) acc = fma((double)w.tw[(br + 1) * 7 + j], (double)pbuf[tid + j * dil], acc);
        out[br + 1] = (float)acc;
        __syncthreads();
    }
    const int t = t0 + tid;
    if (t < frames)
        *reinterpret_cast<float4*>(yi + ((int64_t)b * frames + t) * 4) = make_float4(out[0], out[1], out[2], out[3]);
}

// one block per clip: two-pass mean / biased variance over frames for the 4 branch channels (RAGGED: over the clip's own rn[b] * rmult
// frames, summed in the order of the clip alone; `batch_frames` is the batch's row count).
// The gate multiplies yi - mean by 1/std, up to 316 at a near-constant channel 0 (silence, DC, a square wave, a 1e-6 signal), so what
// is wrong in the mean comes out 316 x larger.  With an fp32 mean (ceil(T / 1024) + 22 additions, a product by the rounded 1 / T) the
// gate was 3 - 14 x less accurate there than the fp32 oracle, whose ATen instance_norm accumulates in fp64; and ANY mean stored in fp32
// is up to half an ulp off, which is still 3 % of yi - mean for a 1e-6 signal.  So: the sums run in fp64, and the second pass writes
// yi - mean back over yi, the difference taken in fp64 and rounded once; stats[0..3] (the mean the gate evaluators subtract) is 0.
// tests/test_gpu_trend_front.py holds the result to 1.5 x the oracle's rms error per input kind.
// The kernel is bound by its passes over yi (16 B per frame): the fp64 adds and the 2 x 24 shuffles are not on that path.
template <bool RAGGED>
__global__ __launch_bounds__(1024) void enhance_stats_kernel(float* __restrict__ yi, int batch_frames,
                                                            float* __restrict__ stats, const int* __restrict__ rn, int rmult) {
    __shared__ double part[16][4];
    __shared__ double bc[4];
    const int b = blockIdx.x;
    float4* src = reinterpret_cast<float4*>(yi) + (int64_t)b * batch_frames;
    const int frames = RAGGED ? rn[b] * rmult : batch_frames;  // >= 1: l3ac_decode_ragged refuses a clip without a token
    auto block_sum = [&](double (&v)[4]) {  // v <- the block's sums, the same bits in every thread; a fixed order of additions
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int m = 1; m < 64; m <<= 1) v[j] += __shfl_xor(v[j], m);
        __syncthreads();
        if ((threadIdx.x & 63) == 0)
            for (int j = 0; j < 4; ++j) part[threadIdx.x >> 6][j] = v[j];
        __syncthreads();
        if (threadIdx.x < 4) {
            double s = part[0][threadIdx.x];
            for (int i = 1; i < 16; ++i) s += part[i][threadIdx.x];
            bc[threadIdx.x] = s;
        }
        __syncthreads();
        for (int j = 0; j < 4; ++j) v[j] = bc[j];
    };
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = threadIdx.x; t < frames; t += 1024) {
        const float4 v = src[t];
        acc[0] += (double)v.x; acc[1] += (double)v.y; acc[2] += (double)v.z; acc[3] += (double)v.w;
    }
    block_sum(acc);
    const double mean[4] = {acc[0] / (double)frames, acc[1] / (double)frames, acc[2] / (double)frames, acc[3] / (double)frames};
    acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
    for (int t = threadIdx.x; t < frames; t += 1024) {
        const float4 v = src[t];
        const double dx = (double)v.x - mean[0], dy = (double)v.y - mean[1], dz = (double)v.z - mean[2], dw = (double)v.w - mean[3];
        acc[0] += dx * dx; acc[1] += dy * dy; acc[2] += dz * dz; acc[3] += dw * dw;
        src[t] = make_float4((float)dx, (float)dy, (float)dz, (float)dw);
    }
    block_sum(acc);
    if (threadIdx.x == 0) {
        float* o = stats + (int64_t)b * 8;
        o[0] = o[1] = o[2] = o[3] = 0.f;  // yi is centred
#pragma unroll
        for (int j = 0; j < 4; ++j) o[4 + j] = (float)(1.0 / sqrt(acc[j] / (double)frames + 1e-5));
    }
}

// head: x [batch][frames][c] (already snake-activated) -> audio [batch][frames]
__global__ __launch_bounds__(TILE) void head_kernel(const float* __restrict__ x, int frames, int c,
                                                   const float* __restrict__ w, const float* __restrict__ bias,
                                                   float* __restrict__ audio, const int pretanh) {
    const int b = blockIdx.y;
    const int t = blockIdx.x * TILE + threadIdx.x;
    if (t >= frames) return;
    const float* clip = x + (int64_t)b * frames * c;
    float acc = bias[0];
    for (int j = 0; j < 7; ++j) {
        const int ts = t + j - 3;
        if (ts < 0 || ts >= frames) continue;
        const float4* row = reinterpret_cast<const float4*>(clip + (int64_t)ts * c);
        const float4* wr = reinterpret_cast<const float4*>(w + j * c);
        for (int q = 0; q < (c >> 2); ++q) {
            const float4 xv = row[q];
            const float4 wv = wr[q];
            acc = fmaf(wv.x, xv.x, acc);
            acc = fmaf(wv.y, xv.y, acc);
            acc = fmaf(wv.z, xv.z, acc);
            acc = fmaf(wv.w, xv.w, acc);
        }
    }
    audio[(int64_t)b * frames + t] = pretanh ? acc : tanhf(acc);
}

}  // namespace

int launch_enhance_branches(hipStream_t s, const EnhanceW& w, const float* x, int batch, int frames, int c, float* yi, const RaggedClips* rc) {
    L3AC_REQUIRE(batch > 0 && batch <= 65535 && frames > 0, "enhance: bad shape");
    L3AC_REQUIRE(frames <= L3AC_MAX_CLIP_FRAMES, "enhance: %d frames per clip, the limit is 2^31 - 65536 (32-bit frame numbers)", frames);
    ProfScope prof(s, rc ? "enhance_branches_kernel<RAGGED>" : "enhance_branches_kernel", 2.0 * (28.0 + 34.0) * batch * frames,
                   4.0 * 5.0 * batch * frames);
    const dim3 grid((unsigned)ceil_div64(frames, TILE), (unsigned)batch);
    if (rc) hipLaunchKernelGGL(enhance_branches_kernel<true>, grid, dim3(TILE), 0, s, w, x, frames, c, yi, rc->n, rc->mult);
    else hipLaunchKernelGGL(enhance_branches_kernel<false>, grid, dim3(TILE), 0, s, w, x, frames, c, yi, nullptr, 1);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

int launch_enhance_stats(hipStream_t s, float* yi, int batch, int frames, float* stats, const RaggedClips* rc) {
    L3AC_REQUIRE(batch > 0 && frames > 0 && frames <= L3AC_MAX_CLIP_FRAMES, "enhance: bad shape, or more than 2^31 - 65536 frames per clip");
    ProfScope prof(s, rc ? "enhance_stats_kernel<RAGGED>" : "enhance_stats_kernel", 16.0 * batch * frames, 48.0 * batch * frames);
    if (rc) hipLaunchKernelGGL(enhance_stats_kernel<true>, dim3((unsigned)batch), dim3(1024), 0, s, yi, frames, stats, rc->n, rc->mult);
    else hipLaunchKernelGGL(enhance_stats_kernel<false>, dim3((unsigned)batch), dim3(1024), 0, s, yi, frames, stats, nullptr, 1);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

int launch_head(hipStream_t s, const float* x, int batch, int frames, int c, const float* w, const float* b,
                float* audio, bool pretanh) {
    L3AC_REQUIRE(c % 4 == 0 && batch <= 65535 && frames <= L3AC_MAX_CLIP_FRAMES, "head: bad shape, or more than 2^31 - 65536 frames per clip");
    ProfScope prof(s, "head_kernel", 14.0 * c * batch * frames, 4.0 * (c + 1.0) * batch * frames);
    hipLaunchKernelGGL(head_kernel, dim3((unsigned)ceil_div64(frames, TILE), (unsigned)batch), dim3(TILE), 0, s, x, frames, c,
                       w, b, audio, pretanh ? 1 : 0);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}
