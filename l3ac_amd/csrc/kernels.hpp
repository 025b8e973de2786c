// Launch API of the HIP kernels (one .hip file per kernel family under kernels/).
// All pointers are device pointers; activations are frame-major [batch][frame][channel].
#pragma once

#include "common.hpp"

// ------------------------------------------------------------------------------------------------
// fp32 MFMA GEMM:  c[m][n] = epilogue( sum_k A(m,k) * w[n][k] )
// ------------------------------------------------------------------------------------------------
enum GemmEpilogue : int {
    EPI_BIAS = 0,       // acc + bias[n]                               (bias may be null)
    EPI_BIAS_RES = 1,   // res[m][n] + (acc + bias[n])                 ConvUnit / LegacyUnit residual, attention/ff residual
    EPI_SNAKE = 2,      // snake(acc + bias[n], alpha[n])              LegacyUnit inner activation
    EPI_SNAKE_GRN = 3,  // s = snake(acc + bias); gamma*s + beta + s   ConvUnit pw_conv1 -> snake -> GRN (normaliser == 1)
    EPI_GEGLU = 4,      // value/gate column tiles interleaved: out[m][j] = v * gelu(g)   (FeedForward)
};

struct GemmArgs {
    // A operand.  taps == 1: plain rows, a[m * lda + k].  taps > 1: implicit 1-D convolution over the frames of
    // one clip: k = tap * cin + c reads a[(b*frames + t + (tap - taps/2) * dil) * lda + c], zero outside the clip.
    const float* a = nullptr;
    int64_t lda = 0;
    int taps = 1, dil = 1, cin = 0;
    int64_t frames = 0;
    // W operand [n][k] (row stride ldw), output c [m][ldc]
    const float* w = nullptr;
    int64_t ldw = 0;
    // optional pre-split bf16x3 image of w (gemm_split.hip); when set, enabled and the shape is eligible the product
    // runs on the bf16 matrix cores at fp32 accuracy, otherwise on the exact-fp32 MFMA kernel
    const unsigned char* w_img = nullptr;
    float* c = nullptr;
    int64_t ldc = 0;
    int64_t m = 0;
    int n = 0, k = 0;
    // epilogue
    int epi = EPI_BIAS;
    int w256 = 1;  // split route, batch rows (option "gemm_w256"): 0 no product, 1 the long-K light-epilogue ones, 2 every eligible
                   // shape on gemm_split_kernel_w256 (the same bits either way; in what was padding: the kernels' arguments keep their layout)
    const float* bias = nullptr;
    const float* res = nullptr;
    int64_t ldres = 0;
    const float* alpha = nullptr;      // snake alpha[n]
    const float* inv_alpha = nullptr;  // 1 / (alpha[n] + 1e-8)
    const float* gamma = nullptr;      // GRN
    const float* beta = nullptr;
    int n_out = 0;                     // EPI_GEGLU: number of valid output columns (ff inner)
    // optional EnhanceBlock gate applied to the A operand while it is staged (tconv/__init__.py:35-44, same arithmetic as
    // the SRC_GATE row kernel): a'(m, k) = a + (gate_b[k] + gate_w[k][:] . instnorm(yi[m][:])) * a.  Plain A, k % 16 == 0.
    const float* gate_yi = nullptr;     // branch signals [m][4], centred in place by enhance_stats_kernel
    const float* gate_stats = nullptr;  // [clip][8] = mean[4] (0: yi arrives centred; the subtraction that is left is exact), 1/std[4]
    const float* gate_in_w = nullptr;   // InstanceNorm affine [4]
    const float* gate_in_b = nullptr;
    const float* gate_w = nullptr;      // merge conv [k][4]
    const float* gate_b = nullptr;      // [k]
    int64_t gate_frames = 0;            // rows per clip
};
int launch_gemm(hipStream_t s, const GemmArgs& g);

// bf16x3 split-operand GEMM (kernels/gemm_split.hip)
#define L3AC_SPLIT_TILE_BYTES 24576  // one k tile (32) of one column block (128): 3 planes x 128 rows x 64 B
bool gemm_split_eligible(int n, int k);  // the route of a launch is its GemmArgs::w_img (null = exact fp32 MFMA kernel)
bool gemm_split_conv_ok(const struct GemmArgs& g);  // taps > 1 on the split route: cin % 32 == 0, plain frame-major rows
int64_t gemm_split_image_bytes(int n, int k);
void gemm_split_image_host(const float* w, int64_t ldw, int n, int k, unsigned char* img);  // img: host buffer
int launch_gemm_split_image(hipStream_t s, const float* w, int64_t ldw, int n, int k, unsigned char* img);  // device
int launch_gemm_split(hipStream_t s, const GemmArgs& g);
bool gemm_split_w256_ok(const GemmArgs& g);
int launch_gemm_split_w256(hipStream_t s, const GemmArgs& g);  // gemm_split_w256.hip: a batch's rows, n % 256 == 0, an even number of whole k tiles

// ------------------------------------------------------------------------------------------------
// row kernels: one output row = one frame (all channels), optional per-row normalisation
// ------------------------------------------------------------------------------------------------
enum RowSource : int {
    SRC_PLAIN = 0,    // y = x
    SRC_DWCONV7 = 1,  // depth-wise conv k7 pad 3 along frames (ConvUnit.dw_conv)
    SRC_LERP = 2,     // linear upsample x scale, align_corners=False (nn.Upsample)
    SRC_GATE = 3,     // EnhanceBlock: x + (merge(instnorm(yi))) * x
};
enum RowNorm : int {
    NORM_NONE = 0,
    NORM_LN = 1,  // F.layer_norm over channels: (x - mu) * rsqrt(var + eps) * w + b
    NORM_CN = 2,  // channel_norm channels_first: (x - mu) / sqrt(var + eps) * w + b
};
struct RowArgs {
    const float* x = nullptr;
    float* y = nullptr;
    int64_t batch = 0, frames_in = 0, frames_out = 0;
    int c = 0;
    int src = SRC_PLAIN, norm = NORM_NONE;
    const float* dw_w = nullptr;  // [7][c]
    const float* dw_b = nullptr;  // [c]
    int scale = 1;                // SRC_LERP
    const float* yi = nullptr;    // SRC_GATE: branch signals [batch][frames][4], centred in place by enhance_stats_kernel
    const float* stats = nullptr; // [batch][8] = mean[4] (0: yi arrives centred), invstd[4]
    const float* in_w = nullptr;  // InstanceNorm affine [4]
    const float* in_b = nullptr;
    const float* gate_w = nullptr;  // merge conv [c][4]
    const float* gate_b = nullptr;  // [c]
    const float* nw = nullptr;      // norm affine [c]
    const float* nb = nullptr;
    float eps = 0.f;
};
int launch_rows(hipStream_t s, const RowArgs& r);

// elementwise
int launch_snake(hipStream_t s, const float* x, float* y, int64_t rows, int c, const float* alpha,
                 const float* inv_alpha, int mode = 0);  // mode: see snake_kernel
int launch_geglu(hipStream_t s, const float* h, int64_t ldh, float* y, int64_t ldy, int64_t rows, int inner);
int launch_grn_sumsq(hipStream_t s, const float* h, int64_t batch, int64_t per_clip, float* sumsq);
int launch_grn_apply(hipStream_t s, float* h, int64_t batch, int64_t frames, int c, const float* sumsq,
                     const float* gamma, const float* beta, float* min_track = nullptr);  // min_track: running minimum of sumsq

// FirstBlock (tconv/__init__.py:8-27): audio [batch][samples] -> y [batch][frames][d0], frames >= samples (zero tail)
struct FirstBlockW {
    const float* tw;   // trend convs [5][4][7]
    const float* tb;   // [5][4]
    const float* w1;   // conv_1 [80][20]
    const float* b1;   // [80]
    const float* w2;   // conv_2 [d0][81]
    const float* b2;   // [d0]
    int d0;
};
// Per-clip bounds of a ragged batch (kernels/ragged.hip), device arrays: clip b has n[b] * mult of the
// launch's `frames` (and, for the first block, samples[b] of its `samples`); null = every clip has them all (the plain kernels)
struct RaggedClips {
    const int* n = nullptr;
    int mult = 1;
    const int* samples = nullptr;
};
int launch_first_block(hipStream_t s, const FirstBlockW& w, const float* audio, int64_t audio_stride, int batch,
                       int samples, int frames, float* y, const RaggedClips* rc = nullptr);

// EnhanceBlock helpers (tconv/__init__.py:30-44)
struct EnhanceW {
    const float* tw;  // trend convs [4][7]
    const float* tb;  // [4]
};
int launch_enhance_branches(hipStream_t s, const EnhanceW& w, const float* x, int batch, int frames, int c, float* yi,
                            const RaggedClips* rc = nullptr);
// (centres yi in place: stats = 0[4], 1/std[4])
int launch_enhance_stats(hipStream_t s, float* yi, int batch, int frames, float* stats, const RaggedClips* rc = nullptr);

// output head (modules.py:190-195 after the Snake1d): conv 24 -> 1 k7 pad 3, tanh
// pretanh (validation, l3ac_ctx_set_head_pretanh): store the conv result BEFORE the final tanh
int launch_head(hipStream_t s, const float* x, int batch, int frames, int c, const float* w /*[7][c]*/,
                const float* b, float* audio, bool pretanh = false);

// causal local attention, look-back one window (local_attention.LocalAttention); qkv [rows][3*heads*dh]
int launch_attention(hipStream_t s, const float* qkv, float* out, const float* bias_table /*[heads][2*window]*/,
                     int batch, int frames, int heads, int dh, int window);

// FSQ
struct FsqArgs {
    const float* x = nullptr;   // [n][feat] or null (latents is then the input)
    int64_t n = 0;
    int feat = 0, n_levels = 0;
    int levels[L3AC_MAX_LEVELS] = {0};
    const float* w_in = nullptr;
    const float* b_in = nullptr;
    const float* w_out = nullptr;
    const float* b_out = nullptr;
    const int32_t* idx_in = nullptr;  // decode path: indices are the input
    float* q_feature = nullptr;
    int32_t* indices = nullptr;
    float* level_indices = nullptr;
    float* latents = nullptr;
    bool act_in = false;              // x == idx_in == null and `latents` holds act = (tanh(lat) + 1) / 2 (vq/fsq.py:56)
    int* bad_count = nullptr;         // decode path: device counter of indices outside [0, codebook size) (they are clamped)
};
int launch_fsq(hipStream_t s, const FsqArgs& a);
// measurement aid: fsq_kernel's grid and access pattern (feat 128, 6 levels) with no arithmetic — its achievable HBM ceiling
int launch_fsq_copy_ceiling(hipStream_t s, const float* x, int64_t n, float* q, int32_t* idx, float* li, int blocks_per_cu = 0);
// token bit stream (kernels/bitpack.hip)
int launch_pack_indices(hipStream_t s, const int32_t* idx, int batch, int n_tok, int bits, uint32_t* out, int words_per_clip);
int launch_unpack_indices(hipStream_t s, const uint32_t* in, int batch, int n_tok, int bits, int words_per_clip, int32_t* idx);
// polyphase sample-rate conversion, scipy.signal.resample_poly's defaults (kernels/resample.hip)
struct ResamplePlan {
    int up, down;   // out_rate / gcd, in_rate / gcd
    int half_len;   // 10 max(up, down)
    int K, KE;      // taps per output; bank row length (even, >= K + 1)
};
int resample_plan(int32_t in_rate, int32_t out_rate, ResamplePlan* p);  // L3AC_EINVAL (message set) on unsupported rates
int64_t resample_length(const ResamplePlan& p, int64_t n_in);
int64_t resample_bank_floats(const ResamplePlan& p);                     // 0 when up == down (a copy needs no filter)
void resample_fill_bank(const ResamplePlan& p, float* bank);             // host: [up][2][KE] fp32, each tap rounded once from fp64
int launch_resample(hipStream_t s, const float* x, int batch, int64_t n_in, int64_t x_stride, int32_t in_rate, int32_t out_rate,
                    const float* bank, float* y, int64_t y_stride);
// ragged batches (kernels/ragged.hip): per-clip counts reach the device as kernel arguments, CAP values per launch
struct RaggedUpload {
    static constexpr int CAP = 248;
    int offset, n;
    int vals[CAP];
};
int launch_ragged_upload(hipStream_t s, int* dst, const int* host, int n);
// zero rows [n[b] * mult, n[b] * mult + width) of each clip of x [batch][frames][c] (clipped to frames)
int launch_ragged_mask(hipStream_t s, float* x, int batch, int frames, int c, const int* n, int mult, int width);
// row n[b] * mult of each clip = row n[b] * mult - 1 (where it is inside the clip's frames)
int launch_ragged_dup(hipStream_t s, float* x, int batch, int frames, int c, const int* n, int mult);
// compact clip k <-> batch clip perm[k0 + k] for k < count: `rows` rows of c floats; clip strides in floats
int launch_ragged_gather(hipStream_t s, const float* src, float* dst, const int* perm, int k0, int count, int rows, int c,
                         int64_t batch_clip, int64_t compact_clip, bool scatter);
// long recordings as chunk rows (kernels/chunk.hip): descriptors reach the device as kernel arguments, CAP per launch
struct ChunkBlock {
    static constexpr int CAP = 112;  // 3.5 KiB of the 4 KiB a launch's arguments may take
    l3ac_chunk_desc desc[CAP];
};
// HOST: the chunks of `batch` recordings (ChunkData's geometry); the count, or L3AC_EINVAL.  Fills `out` when non-null (cap >= count)
int64_t chunk_plan(const int64_t* frames, int batch, int64_t chunk_len, int64_t prefix_len, int round_to, l3ac_chunk_desc* out, int64_t cap);
// recordings [recs][src_stride][c] -> chunk rows [rows][dst_row_frames][c], 4-byte elements; `desc` is a host array
int launch_chunk_cut(hipStream_t s, const void* src, int recs, int64_t src_stride, int c, const l3ac_chunk_desc* desc, int count, void* dst,
                     int rows, int64_t dst_row_frames);
// chunk rows [rows][src_row_frames][c] -> recordings [recs][dst_stride][c], prefixes dropped, zeros from a recording's end to out_frames
int launch_chunk_merge(hipStream_t s, const void* src, int rows, int64_t src_row_frames, int c, const l3ac_chunk_desc* desc, int count,
                       void* dst, int recs, int64_t dst_stride, int64_t out_frames);
// streaming sessions (kernels/stream.hip): the state carried between pushes; descriptors as kernel arguments, CAP per launch
struct StreamBlock {
    static constexpr int CAP = 72;  // 3.4 KiB of the 4 KiB a launch's arguments may take
    l3ac_stream_desc desc[CAP];
};
// chunk row desc.row = state[slot][0 : held] ++ fresh[slot][off : off + take] ++ zeros(pad); `desc` is a host array
int launch_stream_gather(hipStream_t s, const void* state, int streams, int64_t state_frames, const void* fresh, int64_t fresh_frames,
                         int64_t fresh_stride, int c, const l3ac_stream_desc* desc, int count, void* rows, int n_rows, int64_t row_frames);
// state[slot][0 : keep] = the last keep of row desc.row's held + take own frames
int launch_stream_carry(hipStream_t s, const void* rows, int n_rows, int64_t row_frames, int c, const l3ac_stream_desc* desc, int count, void* state,
                        int streams, int64_t state_frames);
// state[slot][held : held + take] = fresh[slot][off : off + take]
int launch_stream_append(hipStream_t s, const void* fresh, int64_t fresh_frames, int64_t fresh_stride, int c, const l3ac_stream_desc* desc, int count,
                         void* state, int streams, int64_t state_frames);
// frames [prefix, held + take + pad) of row desc.row -> dst[slot][out ...], then `zero` zero frames
int launch_stream_emit(hipStream_t s, const void* rows, int n_rows, int64_t row_frames, int c, const l3ac_stream_desc* desc, int count, void* dst,
                       int streams, int64_t dst_stride, int64_t out_frames);
// streaming sample-rate conversion (kernels/resample_stream.hip): one launch per push computes every stream's outputs
// from state ++ new samples and writes its next state into the other state buffer; descriptors as kernel arguments, CAP per launch
struct ResampleStreamBlock {
    static constexpr int CAP = 128;  // 3 KiB of the 4 KiB a launch's arguments may take
    l3ac_resample_stream_desc desc[CAP];
};
int64_t resample_stream_state_floats(const ResamplePlan& p);  // K - 1 rounded up to a multiple of 4
int launch_resample_stream(hipStream_t s, const float* state_in, float* state_out, int streams, int64_t state_stride, const float* fresh,
                           int64_t fresh_frames, int64_t fresh_stride, int32_t in_rate, int32_t out_rate, const float* bank,
                           const l3ac_resample_stream_desc* desc, int count, float* out, int64_t out_frames, int64_t out_stride);
// streaming token wire format (kernels/bitpack_stream.hip): one launch per push packs / unpacks every stream's
// held bits ++ new tokens / bytes and writes its next pending bits into the other state buffer; descriptors as kernel arguments, CAP per launch
struct PackStreamBlock {
    static constexpr int CAP = 160;  // 3.1 KiB of the 4 KiB a launch's arguments may take
    l3ac_pack_stream_desc desc[CAP];
};
struct UnpackStreamBlock {
    static constexpr int CAP = 160;
    l3ac_unpack_stream_desc desc[CAP];
};
int64_t packed_bytes(int64_t n_tok, int bits);  // HOST: ceil(n_tok * bits / 8), L3AC_EINVAL for n_tok < 0 or bits outside 1..32
int launch_pack_stream(hipStream_t s, const uint32_t* state_in, uint32_t* state_out, int streams, const int32_t* fresh, int64_t fresh_tokens,
                       int64_t fresh_stride, int bits, const l3ac_pack_stream_desc* desc, int count, uint8_t* out, int64_t out_bytes,
                       int64_t out_stride);
int launch_unpack_stream(hipStream_t s, const uint32_t* state_in, uint32_t* state_out, int streams, const uint8_t* fresh, int64_t fresh_bytes,
                         int64_t fresh_stride, int bits, const l3ac_unpack_stream_desc* desc, int count, int32_t* out, int64_t out_tokens,
                         int64_t out_stride);
// quality metrics (kernels/metrics.hip): STFT as one exact-fp32 GEMM over staged clip rows, log-mel, log-mel
// distance and the time-domain metrics; `samples` is a host array (null: every clip has max_samples), handed over as kernel arguments
int64_t stft_frames(int64_t samples, int32_t hop);                          // HOST: 1 + samples / hop, L3AC_EINVAL for samples or hop < 1
int64_t stft_basis(int32_t n_fft, float* basis, int64_t cap);               // HOST: [n_fft + 2][n_fft] fp32, each entry rounded once from fp64
int64_t mel_weights(int32_t sample_rate, int32_t n_fft, int32_t n_mels, float* w, int64_t cap);  // HOST: [n_mels][n_fft / 2 + 1]
int64_t mel_scratch_bytes(int32_t batch, int64_t max_samples, int32_t n_fft, int32_t hop, int32_t n_mels);
int launch_stft(hipStream_t s, const float* audio, int32_t batch, int64_t max_samples, int64_t audio_stride, const int32_t* samples, int32_t n_fft,
                int32_t hop, const float* basis, float* spec, void* scratch, int64_t scratch_bytes);
int launch_log_mel(hipStream_t s, const float* audio, int32_t batch, int64_t max_samples, int64_t audio_stride, const int32_t* samples, int32_t n_fft,
                   int32_t hop, const float* basis, const float* weights, int32_t n_mels, float* out, void* scratch, int64_t scratch_bytes);
int launch_mel_distance(hipStream_t s, const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch,
                        int64_t max_samples, const int32_t* samples, int32_t n_fft, int32_t hop, int32_t n_mels, const float* basis,
                        const float* weights, double* out, void* scratch, int64_t scratch_bytes);
int launch_signal_metrics(hipStream_t s, const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch,
                          int64_t max_samples, const int32_t* samples, double* out, void* scratch, int64_t scratch_bytes);
// speech intelligibility (kernels/stoi.hip; include/l3ac_hip.h "speech intelligibility"): STOI and ESTOI of pairs at 10 kHz
int64_t stoi_frames(int64_t samples);               // HOST: A(samples), L3AC_EINVAL for samples < 1
int64_t stoi_basis(float* basis, int64_t cap);      // HOST: [514][256] fp32, each entry rounded once from fp64
int64_t stoi_window(float* w, int64_t cap);         // HOST: [256] fp32 = row 0 of the basis
int stoi_bands(int32_t* runs);                      // HOST: 15 x (lo, hi)
int64_t stoi_scratch_bytes(int32_t batch, int64_t max_samples);
int launch_stoi(hipStream_t s, const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples,
                const int32_t* samples, const float* basis, double* out, int32_t* frames_out, float* bands_out, void* scratch,
                int64_t scratch_bytes);
// loudness (kernels/loudness.hip; include/l3ac_hip.h "loudness"): BS.1770-4 integrated loudness of mono clips in fp64,
// the K-weighting recursion parallel over 100 ms steps (zero-state pass, per-clip scan of the 4-value state, energy pass), and the gain
int64_t loudness_coeffs(int32_t sample_rate, double* out, int64_t cap);     // HOST: [2][6] b0 b1 b2 a0 a1 a2, then M [4][4]
int64_t loudness_blocks(int64_t samples, int32_t sample_rate);              // HOST: J(samples)
int64_t loudness_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sample_rate);
int launch_loudness(hipStream_t s, const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples,
                    int32_t sample_rate, double* stats, int32_t* counts, double* momentary, void* scratch, int64_t scratch_bytes);
int launch_loudness_gain(hipStream_t s, const double* stats, int32_t batch, double target_lufs, double peak_limit_db, double* gain);
int launch_apply_gain(hipStream_t s, const float* audio, int64_t audio_stride, float* out, int64_t out_stride, int32_t batch, int64_t max_samples,
                      const int32_t* samples, const double* gain, int64_t gain_stride);
// pitch (kernels/pitch.hip; include/l3ac_hip.h "pitch"): YIN over groups of frames staged in LDS (fp32 difference
// function, one lane per lag; fp64 from the prefix on), and the pairwise F0 metrics; window / hop -1: the defaults
int pitch_lags(int32_t sample_rate, double fmin, double fmax, int32_t window, int32_t hop, int32_t* out);  // HOST: tau_min tau_max W hop span
int64_t pitch_frames(int64_t samples, int32_t sample_rate, double fmin, double fmax, int32_t window, int32_t hop);  // HOST: F(samples)
int64_t pitch_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sample_rate, double fmin, double fmax, int32_t window, int32_t hop);
int launch_pitch(hipStream_t s, const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples,
                 int32_t sample_rate, double fmin, double fmax, int32_t window, int32_t hop, double threshold, double* f0, int32_t* voiced,
                 double* aperiodicity, double* cmnd, int32_t* frames, void* scratch, int64_t scratch_bytes);
int launch_pitch_metrics(hipStream_t s, const double* f0_ref, const int32_t* voiced_ref, const double* f0_est, const int32_t* voiced_est, int32_t batch,
                         int64_t max_frames, const int32_t* frames, double* out, int32_t* counts);
// time alignment (kernels/align.hip; include/l3ac_hip.h "time alignment"): the cross-correlation of clip pairs over
// lags -max_lag .. max_lag as a GEMM on the fp32 matrix pipe with fp64 diagonal sums, the pick of lag / polarity / delay / correlation,
// and the shift by per-clip lags read from device memory
int64_t xcorr_scratch_bytes(int32_t batch, int64_t max_samples, int32_t max_lag);
int launch_xcorr(hipStream_t s, const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples,
                 const int32_t* samples, int32_t max_lag, int32_t* lag, int32_t* polarity, double* delay, double* correlation, double* xcorr,
                 void* scratch, int64_t scratch_bytes);
int launch_align_apply(hipStream_t s, const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples,
                       const int32_t* samples, const int32_t* lag, float* out_ref, int64_t out_ref_stride, float* out_est, int64_t out_est_stride,
                       int32_t* out_samples, void* scratch, int64_t scratch_bytes);
// mel-cepstral distortion (kernels/mcd.hip; include/l3ac_hip.h "mel-cepstral distortion"): the orthonormal DCT-II
// table (host), the cepstra of log_mel's cells as one fp32 fmaf chain per coefficient, and the batched DTW over rows of fp32 features
// (fp64 frame distances and accumulation, one workgroup per pair, the backtrace in the same kernel)
int64_t dct_table(int32_t n_mels, int32_t n_coeffs, float* out, int64_t cap);
int64_t mfcc_scratch_bytes(int32_t batch, int64_t max_samples, int32_t n_fft, int32_t hop, int32_t n_mels, int32_t n_coeffs);
int launch_mfcc(hipStream_t s, const float* audio, int32_t batch, int64_t max_samples, int64_t audio_stride, const int32_t* samples, int32_t n_fft,
                int32_t hop, const float* basis, const float* weights, int32_t n_mels, const float* dct, int32_t n_coeffs, float* out, void* scratch,
                int64_t scratch_bytes);
int64_t dtw_scratch_bytes(int32_t batch, int32_t max_frames_a, int32_t max_frames_b);
int launch_dtw(hipStream_t s, const float* a, int64_t a_frame_stride, int64_t a_row_stride, const float* b, int64_t b_frame_stride, int64_t b_row_stride,
               int32_t batch, int32_t dim, int32_t max_frames_a, int32_t max_frames_b, const int32_t* frames_a, const int32_t* frames_b,
               int32_t diagonal_only, double* cost, int32_t* path_len, int32_t* path, double* delta, void* scratch, int64_t scratch_bytes);
// linear prediction and the envelope measures (kernels/lpc.hip; include/l3ac_hip.h "linear prediction"): the window
// (host), the geometry (host), short-time autocorrelation + Levinson-Durbin of one side, and of a pair with the three quadratic forms, the
// cepstra, LLR / IS / CD / segmental SNR per frame and the sorted, trimmed means per pair (one workgroup per pair)
int64_t lpc_window(int32_t frame, float* out, int64_t cap);
int lpc_defaults(int32_t sample_rate, int32_t* out);
int64_t lpc_frames(int64_t samples, int32_t frame, int32_t hop);
int64_t lpc_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sample_rate, int32_t order, int32_t frame, int32_t hop);
int launch_lpc(hipStream_t s, const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples,
               int32_t sample_rate, int32_t order, int32_t frame, int32_t hop, const float* window, double* a, double* reflection, double* error,
               double* autocorr, int32_t* valid, int32_t* frames, void* scratch, int64_t scratch_bytes);
int64_t lpc_metrics_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sample_rate, int32_t order, int32_t frame, int32_t hop);
int launch_lpc_metrics(hipStream_t s, const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples,
                       const int32_t* samples, int32_t sample_rate, int32_t order, int32_t frame, int32_t hop, const float* window, double trim,
                       double llr_max, double is_max, double cd_max, double* out, int32_t* counts, double* frame_values, double* forms, void* scratch,
                       int64_t scratch_bytes);
// the SDR of BSS Eval and its primitives (kernels/sdr.hip; include/l3ac_hip.h "BSS Eval SDR"): the lag correlation of
// whole clips, the Toeplitz solve (Levinson with a general right-hand side, one wave per pair), and the two chained with the residual's
// energies and 10 log10(T / D)
int64_t correlate_scratch_bytes(int32_t batch, int64_t max_samples, int32_t lags);
int launch_correlate(hipStream_t s, const float* u, int64_t u_stride, const float* v, int64_t v_stride, int32_t batch, int64_t max_samples,
                     const int32_t* samples, int32_t lags, double* out, void* scratch, int64_t scratch_bytes);
int64_t toeplitz_solve_scratch_bytes(int32_t batch, int32_t length);
int launch_toeplitz_solve(hipStream_t s, const double* r, const double* b, int32_t batch, int32_t length, double* x, double* error, int32_t* valid,
                          void* scratch, int64_t scratch_bytes);
int64_t sdr_scratch_bytes(int32_t batch, int64_t max_samples, int32_t filter_length);
int launch_sdr(hipStream_t s, const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples,
               const int32_t* samples, int32_t filter_length, double load, double* out, int32_t* valid, double* filter, double* corr, void* scratch,
               int64_t scratch_bytes);
// explicit-codebook L2 argmin (kernels/fsq.hip): scratch = vq_argmin_scratch_bytes(n, k) bytes, caller-provided
size_t vq_argmin_scratch_bytes(int64_t n, int k, int form = 0);
// form: 0 automatic, 1 the direct-form scan wherever the screened form would run (the reference the screened form is tested against)
int launch_vq_argmin(hipStream_t s, const float* queries, int64_t n, const float* codebook, int k, int dim, void* scratch,
                     int32_t* out_idx, int form = 0);
