// Internal launch API of the codec's HIP kernels (one .hip file per kernel family under kernels/), and the helpers several families share.
// The context-free entries of include/l3ac_hip.h are not declared again here: that header is their one declaration.
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

// ------------------------------------------------------------------------------------------------
// The context-free entries (token packing, resampling, chunking, streaming, wire format, the metric families) have no declaration here:
// each l3ac_* function of include/l3ac_hip.h is defined once, in its family's file under kernels/, and that is what other families call.
// Below is only what several of those files share.
// ------------------------------------------------------------------------------------------------
// polyphase sample-rate conversion, scipy.signal.resample_poly's defaults (kernels/resample.hip, kernels/resample_stream.hip)
struct ResamplePlan {
    int up, down;   // out_rate / gcd, in_rate / gcd
    int half_len;   // 10 max(up, down)
    int K, KE;      // taps per output; bank row length (even, >= K + 1)
};
int resample_plan(int32_t in_rate, int32_t out_rate, ResamplePlan* p);  // L3AC_EINVAL (message set) on unsupported rates
int64_t resample_length(const ResamplePlan& p, int64_t n_in);
int64_t resample_bank_floats(const ResamplePlan& p);                     // 0 when up == down (a copy needs no filter)
void resample_phase_taps(const ResamplePlan& p, float* taps);            // host: THE filter design: g_p[t] as [up][K] fp32, each tap rounded once from fp64
void resample_fill_bank(const ResamplePlan& p, float* bank);             // host: [up][4][KE] fp32, the same taps laid out for resample_poly_kernel
int64_t resample_stream_state_floats(const ResamplePlan& p);             // a stream's carried inputs: K - 1 rounded up to a multiple of 4
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
// Descriptors of the chunk, stream, streaming-resample and wire-format calls are host values and reach the device as kernel arguments,
// CAP per launch: each block stays inside the 4 KiB that a launch's arguments may take
struct ChunkBlock {  // kernels/chunk.hip
    static constexpr int CAP = 112;  // 3.5 KiB
    l3ac_chunk_desc desc[CAP];
};
struct StreamBlock {  // kernels/stream.hip
    static constexpr int CAP = 72;  // 3.4 KiB
    l3ac_stream_desc desc[CAP];
};
struct ResampleStreamBlock {  // kernels/resample_stream.hip
    static constexpr int CAP = 128;  // 3 KiB
    l3ac_resample_stream_desc desc[CAP];
};
struct PackStreamBlock {  // kernels/bitpack_stream.hip
    static constexpr int CAP = 160;  // 3.1 KiB
    l3ac_pack_stream_desc desc[CAP];
};
struct UnpackStreamBlock {
    static constexpr int CAP = 160;
    l3ac_unpack_stream_desc desc[CAP];
};

// explicit-codebook L2 argmin (kernels/fsq.hip): scratch = vq_argmin_scratch_bytes(n, k) bytes, caller-provided
size_t vq_argmin_scratch_bytes(int64_t n, int k, int form = 0);
// form: 0 automatic, 1 the direct-form scan wherever the screened form would run (the reference the screened form is tested against)
int launch_vq_argmin(hipStream_t s, const float* queries, int64_t n, const float* codebook, int k, int dim, void* scratch,
                     int32_t* out_idx, int form = 0);
