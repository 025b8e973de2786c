// Mel-cepstral distortion along a dynamic-time-warping path (include/l3ac_hip.h, "mel-cepstral distortion"; DESIGN.md §3.17, which is
// normative): the cepstra of l3ac_log_mel's cells, a batched DTW over rows of fp32 features, and its backtrace.  No reference counterpart.
//
//   mfcc_dct_kernel   grid (blocks of cells, batch): l3ac_log_mel (metrics.hip: its staging, its product, its mel kernel — nothing of it is
//                     repeated here) writes the clips' cells [batch][F][n_mels] into the scratch; one lane per (frame, q) then runs
//                     c[f][q] = sum_m D[q][m] L[f][m] as ONE fp32 fmaf chain over m = 0 .. n_mels - 1 from +0: the chain launch_gemm
//                     gives without a w_img.  (launch_gemm itself takes k and lda in multiples of 4: n_mels = 255 would need a padded
//                     copy of the cells and of the table first; the chain is 40 to 256 terms per output and not worth two more passes.)
//                     Frames at or after a clip's own F(n) are written as exact zeros by a select.
//   dtw_kernel        one workgroup of DTW_THREADS per pair, walking the anti-diagonals d = i + j of the pair's Fa x Fb matrix.  Thread t
//                     owns rows t, t + DTW_THREADS, ...; the three live anti-diagonals (d, d - 1, d - 2), indexed by the row, are fp64
//                     in LDS: 3 x 4096 x 8 = 96 KiB of the CU's 160 — this is what caps a pair at 4096 frames a side.  Cell (i, j)
//                     reads its predecessors (i - 1, j - 1) = diag[d - 2][i - 1], (i - 1, j) = diag[d - 1][i - 1], (i, j - 1) =
//                     diag[d - 1][i] and writes diag[d][i]: the buffer written at step d is the one read as d - 2 one step earlier, so ONE
//                     barrier per anti-diagonal orders everything.  delta(i, j) is computed on the fly from the pair's rows, read
//                     through L2, in fp64 in the order of q.  One choice byte per cell (0: diagonal, 1: (i - 1, j), 2: (i, j - 1)) goes
//                     to the scratch [pair][Fa_max][Fb_max].  A choice is only ever taken among the predecessors inside the matrix and
//                     replaced on a strict <, so with NaN in the pair every stored choice still points inside the matrix.
//     backtrace       the tail of the same kernel: after a barrier lane 0 walks the stored choices from (Fa - 1, Fb - 1) to (0, 0) —
//                     once to count P, once more to write the path from (0, 0) forward when the caller wants it; the workgroup fills
//                     the rows after P with -1.
//     diagonal_only   delta(f, f) by the workgroup into LDS, summed by lane 0 in the order of f; P = F, the path is (f, f).
//
// A pair's bits depend on its own Fa + Fb rows only — never on the batch, the pair's row, the strides, the scratch size or what lies at or
// after its frame counts (masked by never being read); no atomics; the frame counts are kernel arguments and there is no device table
// on the DTW side, so a first call can be captured.
//
// Contraction is off for this whole file: the only fused operation is the fmaf that the cepstrum's chain is written in.
#include "metric_common.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int CEP_THREADS = 256;
constexpr int CEP_MAX_COEFFS = 64;
constexpr int CEP_MAX_MELS = 256;
constexpr int DTW_THREADS = 1024;
constexpr int DTW_MAX_FRAMES = 4096;  // three fp64 anti-diagonals of this many rows are 96 KiB of LDS
constexpr int DTW_MAX_DIM = 64;

static_assert(3 * DTW_MAX_FRAMES * 8 <= 160 * 1024, "the three anti-diagonals live in one workgroup's LDS");

// ---- cepstra: grid (blocks of (frame, q) cells, batch) ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(CEP_THREADS) void mfcc_dct_kernel(const float* __restrict__ cells, const float* __restrict__ dct,
                                                             const int* __restrict__ lens, float* __restrict__ out, int64_t frames,
                                                             int64_t max_samples, int hop, int n_mels, int n_out) {
    const int b = blockIdx.y;
    const int64_t e = (int64_t)blockIdx.x * CEP_THREADS + threadIdx.x;
    if (e >= frames * n_out) return;
    const int64_t f = e / n_out;
    const int q = (int)(e - f * n_out);
    const int64_t n = lens ? lens[b] : max_samples;
    float acc = 0.f;
    if (f < 1 + n / hop) {
        const float* l = cells + ((int64_t)b * frames + f) * n_mels;
        const float* d = dct + (int64_t)q * n_mels;
        for (int m = 0; m < n_mels; ++m) acc = fmaf(d[m], l[m], acc);
    }
    out[((int64_t)b * frames + f) * n_out + q] = acc;
}

// ---- DTW: one workgroup per pair -----------------------------------------------------------------------------------------------------------
// delta(i, j): difference, square and sum in fp64 in the order of q, then the square root
__device__ __forceinline__ double frame_delta(const float* __restrict__ x, const float* __restrict__ y, int dim) {
    double s = 0.0;
    for (int q = 0; q < dim; ++q) {
        const double d = (double)x[q] - (double)y[q];
        s = s + d * d;
    }
    return sqrt(s);
}

__global__ __launch_bounds__(DTW_THREADS) void dtw_kernel(const float* __restrict__ a, int64_t a_frame_stride, int64_t a_row_stride,
                                                        const float* __restrict__ b, int64_t b_frame_stride, int64_t b_row_stride, int dim,
                                                        int fa_max, int fb_max, const int* __restrict__ lens_a, const int* __restrict__ lens_b,
                                                        int diagonal_only, double* __restrict__ cost, int* __restrict__ path_len,
                                                        int* __restrict__ path, double* __restrict__ delta, unsigned char* __restrict__ choice) {
    __shared__ double diag[3][DTW_MAX_FRAMES];
    __shared__ int steps;
    const int p = blockIdx.x;
    const int tid = threadIdx.x;
    // (the host checked the counts; the clamp keeps every index inside the buffers whatever reaches the device)
    const int fa = min(max(lens_a ? lens_a[p] : fa_max, 1), fa_max);
    const int fb = min(max(lens_b ? lens_b[p] : fb_max, 1), fb_max);
    const float* xa = a + (int64_t)p * a_row_stride;
    const float* xb = b + (int64_t)p * b_row_stride;
    const int64_t cells = (int64_t)fa_max * fb_max;
    unsigned char* ch = choice + (int64_t)p * cells;
    double* dl = delta ? delta + (int64_t)p * cells : nullptr;
    const int path_rows = fa_max + fb_max - 1;
    int* pt = path ? path + (int64_t)p * path_rows * 2 : nullptr;

    if (diagonal_only) {  // (fa == fb: checked by the host; the smaller one bounds every read)
        const int fr = min(fa, fb);
        for (int f = tid; f < fr; f += DTW_THREADS) {
            const double v = frame_delta(xa + (int64_t)f * a_frame_stride, xb + (int64_t)f * b_frame_stride, dim);
            diag[0][f] = v;
            if (dl) dl[(int64_t)f * fb_max + f] = v;
            if (pt) pt[2 * f] = f, pt[2 * f + 1] = f;
        }
        __syncthreads();
        if (tid == 0) {
            double sum = diag[0][0];
            for (int f = 1; f < fr; ++f) sum = sum + diag[0][f];
            cost[p] = sum;
            path_len[p] = fr;
        }
        if (pt)
            for (int k = fr + tid; k < path_rows; k += DTW_THREADS) pt[2 * k] = -1, pt[2 * k + 1] = -1;
        return;
    }

    const int last = fa + fb - 2;
    for (int d = 0; d <= last; ++d) {
        double* cur = diag[d % 3];
        const double* p1 = diag[(d + 2) % 3];  // anti-diagonal d - 1
        const double* p2 = diag[(d + 1) % 3];  // anti-diagonal d - 2
        const int lo = max(0, d - fb + 1), hi = min(d, fa - 1);
        for (int i = tid; i <= hi; i += DTW_THREADS) {
            if (i < lo) continue;
            const int j = d - i;
            const double v = frame_delta(xa + (int64_t)i * a_frame_stride, xb + (int64_t)j * b_frame_stride, dim);
            if (dl) dl[(int64_t)i * fb_max + j] = v;
            double acc = v;
            unsigned char c = 0;  // (the origin's byte is never read)
            if (i > 0 && j > 0) {
                double best = p2[i - 1];
                const double up = p1[i - 1], left = p1[i];
                if (up < best) best = up, c = 1;
                if (left < best) best = left, c = 2;
                acc = v + best;
            } else if (i > 0) {
                acc = v + p1[i - 1];
                c = 1;
            } else if (j > 0) {
                acc = v + p1[i];
                c = 2;
            }
            cur[i] = acc;
            ch[(int64_t)i * fb_max + j] = c;
        }
        __syncthreads();  // diag[d] is complete; diag[d - 2] is free: the next step writes it
    }
    __threadfence();  // the choice bytes, for lane 0's walk
    __syncthreads();
    if (tid == 0) {
        cost[p] = diag[last % 3][fa - 1];
        // a stored choice never leaves the matrix (see above); the tests on i and j keep the walk inside it whatever the bytes hold
        auto step = [&](int& i, int& j) {
            const unsigned char c = ch[(int64_t)i * fb_max + j];
            if (c == 0 && i > 0 && j > 0) --i, --j;
            else if ((c == 1 && i > 0) || j == 0) --i;
            else --j;
        };
        int i = fa - 1, j = fb - 1, n = 1;
        while (i > 0 || j > 0) step(i, j), ++n;
        path_len[p] = n;
        steps = n;
        if (pt) {
            i = fa - 1, j = fb - 1;
            int k = n - 1;
            pt[2 * k] = i, pt[2 * k + 1] = j;
            while (i > 0 || j > 0) {
                step(i, j);
                --k;
                pt[2 * k] = i, pt[2 * k + 1] = j;
            }
        }
    }
    if (!pt) return;
    __syncthreads();
    for (int k = steps + tid; k < path_rows; k += DTW_THREADS) pt[2 * k] = -1, pt[2 * k + 1] = -1;
}

int cep_params(int32_t n_mels, int32_t n_coeffs) {
    L3AC_REQUIRE(n_mels >= 1 && n_mels <= CEP_MAX_MELS, "mfcc: n_mels %d outside 1..%d", n_mels, CEP_MAX_MELS);
    L3AC_REQUIRE(n_coeffs >= 1 && n_coeffs <= std::min(n_mels - 1, CEP_MAX_COEFFS), "mfcc: n_coeffs %d outside 1..min(n_mels - 1, %d) = %d", n_coeffs,
                 CEP_MAX_COEFFS, std::min(n_mels - 1, CEP_MAX_COEFFS));
    return L3AC_OK;
}

struct MfccScratch {  // byte offsets into the caller's scratch, after the clips' lengths
    int64_t cells, mel, need;
};

// the parameters checked, then the cells [batch][F][n_mels] and log_mel's own scratch (as large as it says: not rounded up)
int mfcc_scratch(int32_t batch, int64_t max_samples, int32_t n_fft, int32_t hop, int32_t n_mels, int32_t n_coeffs, MfccScratch* sc) {
    L3AC_TRY(cep_params(n_mels, n_coeffs));
    const int64_t mel = l3ac_mel_scratch_bytes(batch, max_samples, n_fft, hop, n_mels);
    if (mel < 0) return L3AC_EINVAL;
    ScratchPlan plan(batch);
    sc->cells = plan.take((int64_t)batch * (1 + max_samples / hop) * n_mels * 4);
    sc->mel = plan.last(mel);
    sc->need = plan.bytes;
    return L3AC_OK;
}

struct DtwScratch {  // byte offsets into the caller's scratch, after side a's frame counts
    int64_t lens_b, choice, need;
};

// the shape checked (frame counts, not samples), then side b's frame counts and one choice byte per cell [batch][Fa_max][Fb_max]
int dtw_scratch(int32_t batch, int32_t max_frames_a, int32_t max_frames_b, DtwScratch* sc) {
    L3AC_REQUIRE(batch > 0 && batch <= 65535, "dtw: batch %d outside 1..65535", batch);
    L3AC_REQUIRE(max_frames_a >= 1 && max_frames_a <= DTW_MAX_FRAMES, "dtw: max_frames_a %d outside 1..%d", max_frames_a, DTW_MAX_FRAMES);
    L3AC_REQUIRE(max_frames_b >= 1 && max_frames_b <= DTW_MAX_FRAMES, "dtw: max_frames_b %d outside 1..%d", max_frames_b, DTW_MAX_FRAMES);
    ScratchPlan plan(batch);
    sc->lens_b = plan.take((int64_t)batch * 4);
    sc->choice = plan.take((int64_t)batch * max_frames_a * max_frames_b);
    sc->need = plan.bytes;
    return L3AC_OK;
}

}  // namespace

extern "C" {

int64_t l3ac_dct_table(int32_t n_mels, int32_t n_coeffs, float* out, int64_t cap) {
    L3AC_TRY(cep_params(n_mels, n_coeffs));
    const int64_t need = (int64_t)(n_coeffs + 1) * n_mels;
    if (!out || cap < need) return need;
    const double m_d = (double)n_mels;
    for (int q = 0; q <= n_coeffs; ++q) {
        for (int m = 0; m < n_mels; ++m) {
            const int r = (q * (2 * m + 1)) % (4 * n_mels);  // the phase pi q (2m + 1) / (2M), reduced in integers
            out[(int64_t)q * n_mels + m] = q == 0 ? (float)std::sqrt(1.0 / m_d) : (float)(std::sqrt(2.0 / m_d) * std::cos(M_PI * (double)r / (2.0 * m_d)));
        }
    }
    return need;
}

int64_t l3ac_mfcc_scratch_bytes(int32_t batch, int64_t max_samples, int32_t n_fft, int32_t hop, int32_t n_mels, int32_t n_coeffs) {
    MfccScratch sc;
    L3AC_TRY(mfcc_scratch(batch, max_samples, n_fft, hop, n_mels, n_coeffs, &sc));
    return sc.need;
}

int l3ac_mfcc(const float* audio, int32_t batch, int64_t max_samples, int64_t audio_stride, const int32_t* samples, int32_t n_fft, int32_t hop,
              const float* basis, const float* weights, int32_t n_mels, const float* dct, int32_t n_coeffs, float* out, void* scratch,
              int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    MfccScratch sc;
    L3AC_TRY(mfcc_scratch(batch, max_samples, n_fft, hop, n_mels, n_coeffs, &sc));
    L3AC_REQUIRE(audio && out, "mfcc: null buffer");
    L3AC_REQUIRE(basis && weights && dct, "mfcc: null table (l3ac_stft_basis / l3ac_mel_weights / l3ac_dct_table, copied to the device)");
    L3AC_REQUIRE(batch == 1 || audio_stride >= max_samples, "mfcc: row stride below max_samples %lld", (long long)max_samples);
    L3AC_TRY(check_clip_lengths("mfcc", samples, batch, max_samples));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "mfcc", "mfcc", samples, batch, scratch, scratch_bytes, sc.need, &lens));
    const int64_t frames = 1 + max_samples / hop;
    char* base = static_cast<char*>(scratch);
    float* cells = reinterpret_cast<float*>(base + sc.cells);
    L3AC_TRY(l3ac_log_mel(audio, batch, max_samples, audio_stride, samples, n_fft, hop, basis, weights, n_mels, cells, base + sc.mel,
                          scratch_bytes - sc.mel, stream));
    const int n_out = n_coeffs + 1;
    ProfScope prof(s, "mfcc_dct_kernel", 2.0 * batch * (double)frames * n_out * n_mels, 4.0 * batch * (double)frames * (n_mels + n_out));
    hipLaunchKernelGGL(mfcc_dct_kernel, dim3((unsigned)ceil_div64(frames * n_out, CEP_THREADS), (unsigned)batch), dim3(CEP_THREADS), 0, s, cells, dct,
                       lens, out, frames, max_samples, hop, n_mels, n_out);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

int64_t l3ac_dtw_scratch_bytes(int32_t batch, int32_t max_frames_a, int32_t max_frames_b) {
    DtwScratch sc;
    L3AC_TRY(dtw_scratch(batch, max_frames_a, max_frames_b, &sc));
    return sc.need;
}

int l3ac_dtw(const float* a, int64_t a_frame_stride, int64_t a_row_stride, const float* b, int64_t b_frame_stride, int64_t b_row_stride, int32_t batch,
             int32_t dim, int32_t max_frames_a, int32_t max_frames_b, const int32_t* frames_a, const int32_t* frames_b, int32_t diagonal_only,
             double* cost, int32_t* path_len, int32_t* path, double* delta, void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    DtwScratch sc;
    L3AC_TRY(dtw_scratch(batch, max_frames_a, max_frames_b, &sc));
    L3AC_REQUIRE(dim >= 1 && dim <= DTW_MAX_DIM, "dtw: dim %d outside 1..%d", dim, DTW_MAX_DIM);
    L3AC_REQUIRE(a && b, "dtw: null features");
    L3AC_REQUIRE(cost && path_len, "dtw: null output buffer");
    L3AC_REQUIRE((max_frames_a == 1 || a_frame_stride >= dim) && (max_frames_b == 1 || b_frame_stride >= dim), "dtw: frame stride below dim %d", dim);
    L3AC_REQUIRE(batch == 1 || (a_row_stride >= (int64_t)(max_frames_a - 1) * a_frame_stride + dim &&
                                b_row_stride >= (int64_t)(max_frames_b - 1) * b_frame_stride + dim),
                 "dtw: row stride below the extent of a pair's frames ((max_frames - 1) frame_stride + dim)");
    L3AC_REQUIRE(a_frame_stride >= 0 && b_frame_stride >= 0 && a_row_stride >= 0 && b_row_stride >= 0, "dtw: negative stride");
    for (int i = 0; frames_a && i < batch; ++i)
        L3AC_REQUIRE(frames_a[i] >= 1 && frames_a[i] <= max_frames_a, "dtw: frames_a[%d] = %d outside [1, %d]", i, frames_a[i], max_frames_a);
    for (int i = 0; frames_b && i < batch; ++i)
        L3AC_REQUIRE(frames_b[i] >= 1 && frames_b[i] <= max_frames_b, "dtw: frames_b[%d] = %d outside [1, %d]", i, frames_b[i], max_frames_b);
    if (diagonal_only) {
        for (int i = 0; i < batch; ++i) {
            const int fa = frames_a ? frames_a[i] : max_frames_a, fb = frames_b ? frames_b[i] : max_frames_b;
            L3AC_REQUIRE(fa == fb, "dtw: diagonal_only needs equal frame counts, pair %d has %d and %d", i, fa, fb);
        }
    }
    int* lens_a;
    L3AC_TRY(stage_clip_lengths(s, "dtw", "dtw", frames_a, batch, scratch, scratch_bytes, sc.need, &lens_a));
    char* base = static_cast<char*>(scratch);
    int* lens_b = frames_b ? reinterpret_cast<int*>(base + sc.lens_b) : nullptr;
    if (lens_b) L3AC_TRY(launch_ragged_upload(s, lens_b, frames_b, batch));
    unsigned char* choice = reinterpret_cast<unsigned char*>(base + sc.choice);
    const double cells = (double)batch * max_frames_a * max_frames_b;
    ProfScope prof(s, "dtw_kernel", 3.0 * dim * cells, (8.0 * dim + 1.0) * cells);
    hipLaunchKernelGGL(dtw_kernel, dim3((unsigned)batch), dim3(DTW_THREADS), 0, s, a, a_frame_stride, a_row_stride, b, b_frame_stride, b_row_stride, dim,
                       max_frames_a, max_frames_b, lens_a, lens_b, diagonal_only ? 1 : 0, cost, path_len, path, delta, choice);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

}  // extern "C"
