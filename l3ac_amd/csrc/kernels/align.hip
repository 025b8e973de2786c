// Time alignment of clip pairs (include/l3ac_hip.h, "time alignment"; DESIGN.md §3.16, which is normative): the cross-correlation
// r(d) = sum_j ref[j] est[j + d], d = -L .. L, as a GEMM on the fp32 matrix pipe, the pick of the delay and the polarity, and the shift
// that puts a pair on common samples.  No reference counterpart.
//
//   xcorr_kernel        grid (segments of XC_S samples, blocks of XC_DIAGS lags, batch), 4 waves.  In segment g the clip's reference is
//                       the matrix A[a][k] = ref[g S + 32 k + a] (32 x 128) and the estimate B[k][c] = est[g S + 32 k + c - L]
//                       (128 x (32 + 2L)), out-of-range entries reading as 0 (a select, never a product with 0): entry (a, a + d + L) of
//                       A B is the segment's share of r(d) over the samples j = 32 k + a, so r_g(d) is the sum of a diagonal.
//     stage             the segment of ref and the XC_S + 32 XC_TILES - 32 samples of est that the block's columns read go to LDS once
//     product           a wave takes column tiles w, w + 4; per k pair a lane reads its A element once and one B element per tile
//                       (32 consecutive floats per k row: no bank conflict) and issues one v_mfma_f32_32x32x2_f32 per tile: an fp32
//                       fmaf chain over k = 0 .. 127 in the order of k, starting from 0
//     diagonals         the tiles go through LDS (over the staged samples); one lane per lag sums its diagonal in fp64 in the order
//                       of a and writes r_g(d) to scratch [clip][g][2L + 1].  A block owns XC_DIAGS = 32 (XC_TILES - 1) lags: their
//                       diagonals lie inside its own XC_TILES column tiles.  Segments at or past a clip's length are skipped here and
//                       in the pick alike.
//   xcorr_pick_kernel   one workgroup per clip: r(d) = sum_g r_g(d) in the order of g; the energies in signal_metrics_kernel's shape
//                       (exact fp64 squares, fixed strides, the fixed tree); the pick, a minimum over (-|r|, |d|, d), which does not
//                       depend on the order it is taken in; polarity, correlation and the parabolic refinement by one lane
//   align_apply_kernel  grid (blocks along the row, batch): the two rows shifted by the clip's lag, read from device memory; zeros after
//
// A clip's values depend on its own samples and L only — never on the batch, the clip's row, the row stride, the scratch size or what
// lies after the clip's length; no atomics; no device table, so a first call can be captured.  Non-finite samples make that clip's
// results unspecified; every index is bounded by the parameters, whatever the values.
//
// Contraction is off for this whole file: the only fused operations are those of the matrix instruction.
#include "metric_common.hpp"
#include "split_bf16.hpp"

#include <algorithm>

#pragma clang fp contract(off)

namespace {

constexpr int XC_THREADS = 256;
constexpr int XC_WAVES = XC_THREADS / 64;
constexpr int XC_S = 4096;                          // samples of a segment: 32 R
constexpr int XC_R = XC_S / 32;                     // k extent of a segment's product
constexpr int XC_TILES = 8;                         // 32-column tiles of a block: two per wave
constexpr int XC_COLS = 32 * XC_TILES;
constexpr int XC_DIAGS = XC_COLS - 32;              // lags of a block: the diagonal of its last lag ends in its last column
constexpr int XC_EST = XC_S + XC_COLS - 32;         // est samples a block reads: B[k][c], k < R, c < XC_COLS
constexpr int XC_MAX_LAG = 16384;
constexpr int PK_THREADS = 256;
constexpr int AP_THREADS = 256;

static_assert(32 * XC_COLS <= XC_S + XC_EST, "the block's 32 x XC_COLS result tile reuses the LDS of the staged samples");
static_assert(XC_TILES % XC_WAVES == 0 && XC_DIAGS <= XC_THREADS, "two tiles per wave, one lane per lag");


int64_t segments_of(int64_t n) { return ceil_div64(n, XC_S); }

// ---- the segments' diagonal sums: grid (segments, lag blocks, batch) ------------------------------------------------------------------------------
__global__ __launch_bounds__(XC_THREADS) void xcorr_kernel(const float* __restrict__ ref, int64_t ref_stride, const float* __restrict__ est,
                                                         int64_t est_stride, int64_t max_samples, const int* __restrict__ lens, int max_lag,
                                                         double* __restrict__ seg_sums) {
    __shared__ __attribute__((aligned(16))) float lds[XC_S + XC_EST];
    float* as = lds;         // [XC_S]: A[a][k] at 32 k + a
    float* bs = lds + XC_S;  // [XC_EST]: B[k][c] at 32 k + c, c local to the block
    const int b = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t n = lens ? lens[b] : max_samples;
    const int64_t seg0 = (int64_t)blockIdx.x * XC_S;
    if (seg0 >= n) return;  // (the whole workgroup: the pick reads the segments below ceil(n / S) only)
    const int lags = 2 * max_lag + 1;
    const int diag0 = blockIdx.y * XC_DIAGS;                      // the block's first lag index i = d + L, and its first column
    const int diags = min(XC_DIAGS, lags - diag0);                // (at least 1: the grid has ceil(lags / XC_DIAGS) blocks)
    const int tiles = (diags + 31 + 31) >> 5;                     // column tiles that the block's diagonals reach
    const float* r = ref + (int64_t)b * ref_stride;
    const float* e = est + (int64_t)b * est_stride;

    for (int i = tid; i < XC_S; i += XC_THREADS) {
        const int64_t j = seg0 + i;
        as[i] = j < n ? r[j] : 0.f;
    }
    const int64_t est0 = seg0 + diag0 - max_lag;  // sample of bs[0]
    for (int i = tid; i < XC_EST; i += XC_THREADS) {
        const int64_t j = est0 + i;
        bs[i] = (j >= 0 && j < n) ? e[j] : 0.f;
    }
    __syncthreads();

    // lane l holds A[l & 31][2 kp + (l >> 5)] and B[2 kp + (l >> 5)][l & 31]
    const int col = lane & 31, half = lane >> 5;
    const int t0 = wave, t1 = wave + XC_WAVES;
    f32x16_t acc0 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    f32x16_t acc1 = acc0;
    if (t0 < tiles) {  // (the whole wave)
        const float* ap = as + 32 * half + col;
        const float* bp = bs + 32 * half + col;
        if (t1 < tiles) {
#pragma unroll 4
            for (int kp = 0; kp < XC_R / 2; ++kp) {
                const float a = ap[64 * kp];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[64 * kp + 32 * t0], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[64 * kp + 32 * t1], acc1, 0, 0, 0);
            }
        } else {
#pragma unroll 4
            for (int kp = 0; kp < XC_R / 2; ++kp) acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[64 * kp], bp[64 * kp + 32 * t0], acc0, 0, 0, 0);
        }
    }
    __syncthreads();  // every read of the staged samples is over

    // C[a][c] at a XC_COLS + c: register i of a lane is row (i & 3) + 8 (i >> 2) + 4 (l >> 5), column l & 31 of its tile
    float* cs = lds;
    if (t0 < tiles) {
#pragma unroll
        for (int i = 0; i < 16; ++i) cs[((i & 3) + 8 * (i >> 2) + 4 * half) * XC_COLS + 32 * t0 + col] = acc0[i];
    }
    if (t1 < tiles) {
#pragma unroll
        for (int i = 0; i < 16; ++i) cs[((i & 3) + 8 * (i >> 2) + 4 * half) * XC_COLS + 32 * t1 + col] = acc1[i];
    }
    __syncthreads();
    if (tid < diags) {  // columns tid .. tid + 31 < 32 tiles
        double sum = 0.0;
#pragma unroll 8
        for (int a = 0; a < 32; ++a) sum = sum + (double)cs[a * XC_COLS + tid + a];
        seg_sums[((int64_t)b * gridDim.x + blockIdx.x) * lags + diag0 + tid] = sum;
    }
}

// whether lag index i with |r| = v comes before lag index j with |r| = w: the larger value, then the smaller |d|, then the smaller d
__device__ __forceinline__ bool pk_before(double v, int i, double w, int j, int max_lag) {
    if (v != w) return v > w;
    const int di = abs(i - max_lag), dj = abs(j - max_lag);
    return di != dj ? di < dj : i < j;
}

// ---- the pick: one workgroup per clip ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PK_THREADS) void xcorr_pick_kernel(const float* __restrict__ ref, int64_t ref_stride, const float* __restrict__ est,
                                                              int64_t est_stride, int64_t max_samples, const int* __restrict__ lens, int max_lag,
                                                              const double* __restrict__ seg_sums, int64_t seg_max, int* __restrict__ lag_out,
                                                              int* __restrict__ polarity_out, double* __restrict__ delay_out,
                                                              double* __restrict__ correlation_out, double* __restrict__ xcorr_out) {
    __shared__ double lds[PK_THREADS / 64];
    __shared__ double best_v[PK_THREADS / 64];
    __shared__ int best_i[PK_THREADS / 64];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t n = lens ? lens[b] : max_samples;
    const int lags = 2 * max_lag + 1;
    const int64_t segs = (n + XC_S - 1) / XC_S;
    const double* rows = seg_sums + (int64_t)b * seg_max * lags;
    auto r_of = [&](int i) {
        double sum = 0.0;
        for (int64_t g = 0; g < segs; ++g) sum = sum + rows[g * lags + i];
        return sum;
    };

    // the energies: exact squares, fixed strides, the fixed tree
    const float* r = ref + (int64_t)b * ref_stride;
    const float* e = est + (int64_t)b * est_stride;
    double e_ref = 0.0, e_est = 0.0;
    for (int64_t i = tid; i < n; i += PK_THREADS) {
        const double a = (double)r[i], c = (double)e[i];
        e_ref += a * a;
        e_est += c * c;
    }
    e_ref = block_sum<PK_THREADS>(e_ref, lds);
    e_est = block_sum<PK_THREADS>(e_est, lds);

    // the pick: (-1, lag 0) stands where no |r| compares (NaN rows), so the lag stays inside [-L, L]
    double v = -1.0;
    int at = max_lag;
    for (int i = tid; i < lags; i += PK_THREADS) {
        const double ri = r_of(i);
        if (xcorr_out) xcorr_out[(int64_t)b * lags + i] = ri;
        const double w = fabs(ri);
        if (pk_before(w, i, v, at, max_lag)) v = w, at = i;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double ov = __shfl_xor(v, o, 64);
        const int oa = __shfl_xor(at, o, 64);
        if (pk_before(ov, oa, v, at, max_lag)) v = ov, at = oa;
    }
    if ((tid & 63) == 0) best_v[tid >> 6] = v, best_i[tid >> 6] = at;
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < PK_THREADS / 64; ++w)
        if (pk_before(best_v[w], best_i[w], v, at, max_lag)) v = best_v[w], at = best_i[w];

    const double prod = e_ref * e_est;
    if (prod == 0.0) {
        lag_out[b] = 0, polarity_out[b] = 0, delay_out[b] = 0.0, correlation_out[b] = __builtin_nan("");
        return;
    }
    const double peak = r_of(at);
    const int pol = peak < 0.0 ? -1 : 1;
    double shift = 0.0;
    if (at > 0 && at < lags - 1) {
        const double s = (double)pol;
        const double a = s * r_of(at - 1), m = s * peak, c = s * r_of(at + 1);
        const double den = (a - 2.0 * m) + c;
        if (den < 0.0) shift = (0.5 * (a - c)) / den;
    }
    lag_out[b] = at - max_lag;
    polarity_out[b] = pol;
    delay_out[b] = (double)(at - max_lag) + shift;
    correlation_out[b] = peak / sqrt(prod);
}

// ---- the shift: grid (blocks along the row, batch) --------------------------------------------------------------------------------------
__global__ __launch_bounds__(AP_THREADS) void align_apply_kernel(const float* __restrict__ ref, int64_t ref_stride, const float* __restrict__ est,
                                                               int64_t est_stride, int64_t max_samples, const int* __restrict__ lens,
                                                               const int* __restrict__ lag, float* __restrict__ out_ref, int64_t out_ref_stride,
                                                               float* __restrict__ out_est, int64_t out_est_stride, int* __restrict__ out_samples) {
    const int b = blockIdx.y;
    const int64_t n = lens ? lens[b] : max_samples;
    const int64_t d = lag[b];
    const int64_t mag = d < 0 ? -d : d;
    const int64_t m = mag < n ? n - mag : 0;  // every read below is at j + |d| < n
    const int64_t from_ref = d < 0 ? mag : 0, from_est = d > 0 ? mag : 0;
    const float* r = ref + (int64_t)b * ref_stride;
    const float* e = est + (int64_t)b * est_stride;
    float* o_r = out_ref + (int64_t)b * out_ref_stride;
    float* o_e = out_est + (int64_t)b * out_est_stride;
    if (blockIdx.x == 0 && threadIdx.x == 0) out_samples[b] = (int)m;
    for (int64_t j = (int64_t)blockIdx.x * AP_THREADS + threadIdx.x; j < max_samples; j += (int64_t)gridDim.x * AP_THREADS) {
        o_r[j] = j < m ? r[j + from_ref] : 0.f;
        o_e[j] = j < m ? e[j + from_est] : 0.f;
    }
}

struct XcorrScratch {  // byte offsets into the caller's scratch, after the clips' lengths
    int64_t seg_sums, need;
};

// the parameters checked, then r_g(d) [batch][segments][2L + 1] fp64 (the last region: not rounded up)
int xcorr_scratch(int32_t batch, int64_t max_samples, int32_t max_lag, XcorrScratch* sc) {
    L3AC_REQUIRE(max_lag >= 0 && max_lag <= XC_MAX_LAG, "xcorr: max_lag %d outside 0..%d", max_lag, XC_MAX_LAG);
    L3AC_TRY(check_clip_batch("xcorr", batch, max_samples));
    ScratchPlan plan(batch);
    sc->seg_sums = plan.last((int64_t)batch * segments_of(max_samples) * (2 * (int64_t)max_lag + 1) * 8);
    sc->need = plan.bytes;
    return L3AC_OK;
}

}  // namespace

extern "C" {

int64_t l3ac_xcorr_scratch_bytes(int32_t batch, int64_t max_samples, int32_t max_lag) {
    XcorrScratch sc;
    L3AC_TRY(xcorr_scratch(batch, max_samples, max_lag, &sc));
    return sc.need;
}

int l3ac_xcorr(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples, const int32_t* samples,
               int32_t max_lag, int32_t* lag, int32_t* polarity, double* delay, double* correlation, double* xcorr, void* scratch,
               int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    XcorrScratch sc;
    L3AC_TRY(xcorr_scratch(batch, max_samples, max_lag, &sc));
    L3AC_REQUIRE(ref && est, "xcorr: null audio");
    L3AC_REQUIRE(lag && polarity && delay && correlation, "xcorr: null output buffer");
    L3AC_REQUIRE(batch == 1 || (ref_stride >= max_samples && est_stride >= max_samples), "xcorr: row stride below max_samples %lld",
                 (long long)max_samples);
    L3AC_TRY(check_clip_lengths("xcorr", samples, batch, max_samples));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "xcorr", "xcorr", samples, batch, scratch, scratch_bytes, sc.need, &lens));
    double* seg_sums = reinterpret_cast<double*>(static_cast<char*>(scratch) + sc.seg_sums);
    const int64_t segs = segments_of(max_samples);
    const int lags = 2 * max_lag + 1;
    const double terms = (double)batch * (double)max_samples * lags;
    {
        ProfScope prof(s, "xcorr_kernel", 2.0 * terms, 8.0 * batch * (double)max_samples);
        hipLaunchKernelGGL(xcorr_kernel, dim3((unsigned)segs, (unsigned)ceil_div64(lags, XC_DIAGS), (unsigned)batch), dim3(XC_THREADS), 0, s, ref,
                           ref_stride, est, est_stride, max_samples, lens, max_lag, seg_sums);
        L3AC_LAUNCH_CHECK();
    }
    ProfScope prof(s, "xcorr_pick_kernel", 4.0 * batch * (double)max_samples, 8.0 * batch * ((double)max_samples + (double)segs * lags));
    hipLaunchKernelGGL(xcorr_pick_kernel, dim3((unsigned)batch), dim3(PK_THREADS), 0, s, ref, ref_stride, est, est_stride, max_samples, lens, max_lag,
                       seg_sums, segs, lag, polarity, delay, correlation, xcorr);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

int l3ac_align_apply(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples,
                     const int32_t* samples, const int32_t* lag, float* out_ref, int64_t out_ref_stride, float* out_est, int64_t out_est_stride,
                     int32_t* out_samples, void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    L3AC_TRY(check_clip_batch("align_apply", batch, max_samples));
    L3AC_REQUIRE(ref && est, "align_apply: null audio");
    L3AC_REQUIRE(lag, "align_apply: null lag");
    L3AC_REQUIRE(out_ref && out_est && out_samples, "align_apply: null output buffer");
    L3AC_REQUIRE(batch == 1 || (ref_stride >= max_samples && est_stride >= max_samples && out_ref_stride >= max_samples && out_est_stride >= max_samples),
                 "align_apply: row stride below max_samples %lld", (long long)max_samples);
    L3AC_TRY(check_clip_lengths("align_apply", samples, batch, max_samples));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "align_apply", nullptr, samples, batch, scratch, scratch_bytes, ScratchPlan(batch).bytes, &lens));
    const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div64(max_samples, (int64_t)AP_THREADS * 4), 256);
    ProfScope prof(s, "align_apply_kernel", 0.0, 16.0 * batch * (double)max_samples);
    hipLaunchKernelGGL(align_apply_kernel, dim3(blocks, (unsigned)batch), dim3(AP_THREADS), 0, s, ref, ref_stride, est, est_stride, max_samples, lens,
                       lag, out_ref, out_ref_stride, out_est, out_est_stride, out_samples);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

}  // extern "C"
