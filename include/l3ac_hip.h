/*
 * l3ac_hip.h — C ABI of the MI355X-native L3AC encode -> quantize -> decode path (libl3ac_hip.so).
 *
 * The reference (zhai-lw/L3AC) is pure Python and exposes no FFI; its boundary for this path is the method
 * surface of l3ac/__init__.py.  Each entry point below names the reference interface it replaces:
 *
 *   l3ac_create / l3ac_destroy   <- l3ac.get_model + network.load_model   (l3ac/__init__.py:21-25, :104-106,
 *                                                                          l3ac/xtract/nn/module.py:43-54)
 *   l3ac_encode                  <- L3AC.encode_audio                      (l3ac/__init__.py:108-114)
 *   l3ac_decode                  <- L3AC.decode_audio                      (l3ac/__init__.py:116-121)
 *   l3ac_fsq_* / l3ac_vq_argmin  <- VQEmbed.forward / to_features          (l3ac/vq/__init__.py:20-30, vq/fsq.py:30-81)
 *   l3ac_op_*                    <- the individual blocks of modules.py / tconv / local_trans.py, exported so
 *                                   that every kernel can be parity-tested alone.
 *
 * Conventions
 *   - every function returns 0 on success, a negative L3AC_E* code otherwise; nothing throws across the ABI;
 *     l3ac_last_error() returns a human-readable message for the calling thread's last failure.
 *   - all data pointers are DEVICE pointers (e.g. torch tensor.data_ptr()), contiguous, 16-byte aligned,
 *     fp32 / int32.  Activations are frame-major: [batch][frame][channel], channel fastest.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); calls only enqueue
 *     work on it: no host synchronisation, and no allocation once l3ac_reserve() has sized the workspace,
 *     so a call sequence can be captured into a hipGraph.
 *   - one context per device; a context is not thread-safe (one host thread at a time).
 *   - a context owns ONE workspace that every encode / decode / op call reuses in place.  Calls may be issued on
 *     different streams: each call makes its stream wait for the completion event of the context's previous call
 *     when that ran on another stream, so pipelined callers (encode of batch n+1 on stream A, decode of batch n on
 *     stream B) are serialised on the device instead of corrupting each other.  Two exceptions, both the caller's
 *     to order: work captured into a hipGraph (no events are recorded or waited for during capture; keep a captured
 *     sequence on one stream) and replays of such a graph.  For true overlap use one context per stream.
 */
#ifndef L3AC_HIP_H
#define L3AC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define L3AC_ABI_VERSION 5
#define L3AC_MAX_STAGES 8
#define L3AC_MAX_LEVELS 8

enum {
    L3AC_OK = 0,
    L3AC_EINVAL = -1,    /* bad argument / unsupported geometry */
    L3AC_EWEIGHT = -2,   /* missing / mis-shaped weight tensor */
    L3AC_EHIP = -3,      /* HIP runtime error */
    L3AC_ENOMEM = -4,    /* workspace too small while stream capture forbids growing it */
    L3AC_ECOOP = -5,     /* an EARLIER call's cooperative transformer launch timed out: that call's outputs are invalid
                            (see l3ac_coop_timeout_count).  Reported once, by the first call ENTERED after the failure has been
                            counted — the failure word is read at enqueue time without synchronising, so on an asynchronous stream
                            that is one or more calls after the failing one; the message bounds the suspects.  Only a
                            synchronising check (l3ac_coop_timeout_pending / _count, validate=True in the Python surface) is
                            authoritative for the calls issued so far */
};

/* Network geometry: the [network_config] table of the reference's TOML files
 * (l3ac/codec.py:13-36, l3ac/en_codec.py:9-19). */
typedef struct l3ac_config {
    int32_t abi_version;                     /* = L3AC_ABI_VERSION */
    int32_t feature_dim;
    int32_t n_enc;                           /* len(encoder_dims) */
    int32_t enc_dims[L3AC_MAX_STAGES];
    int32_t enc_depths[L3AC_MAX_STAGES];
    int32_t compress_rates[L3AC_MAX_STAGES]; /* n_enc - 1 entries */
    int32_t n_dec;                           /* len(decoder_dims) */
    int32_t dec_dims[L3AC_MAX_STAGES];
    int32_t dec_depths[L3AC_MAX_STAGES];
    int32_t decode_rates[L3AC_MAX_STAGES];   /* n_dec - 1 entries */
    int32_t n_levels;
    int32_t levels[L3AC_MAX_LEVELS];         /* vq_config.levels */
    int32_t en_coder_depth;
    int32_t en_coder_window_size;
    int32_t en_coder_compress_rate;
    int32_t grn_exact;                       /* 0: GRN normaliser taken as exactly 1.0f (true for ||x|| >= 0.25);
                                                1: evaluate g / (g + eps) per clip (layers.py:112-115) */
} l3ac_config;

/* One named fp32 host tensor.  Names are the reference's state-dict keys prefixed with the module file name,
 * weight-norm already folded (".parametrizations.weight.original{0,1}" -> ".weight"), e.g.
 * "encoder.blocks.1.0.module.pw_conv1.weight". */
typedef struct l3ac_tensor {
    const char* name;
    const float* data;
    int64_t numel;
} l3ac_tensor;

typedef struct l3ac_ctx l3ac_ctx;

const char* l3ac_last_error(void);
int l3ac_abi_version(void);

int l3ac_create(const l3ac_config* cfg, const l3ac_tensor* tensors, int32_t n_tensors, int32_t device,
                l3ac_ctx** out);
void l3ac_destroy(l3ac_ctx* ctx);

/* Size the workspace for clips of up to `samples` samples in batches of up to `batch` (allocates; call it
 * before stream capture).  encode/decode grow the workspace themselves when not capturing. */
int l3ac_reserve(l3ac_ctx* ctx, int32_t batch, int32_t samples);
int64_t l3ac_workspace_bytes(const l3ac_ctx* ctx);
/* decode_audio(indices = ...) takes its indices from outside (a wire stream): values outside [0, codebook size) are counted
 * per context and clamped into range instead of being decomposed into wrapped level indices.  This call synchronises the
 * device, writes the count since the last reset to *out and optionally resets it. */
int l3ac_bad_index_count(l3ac_ctx* ctx, int32_t reset, int64_t* out);
/* The cooperative form of the transformer kernel (option "trans_coop", below; reference l3ac/local_trans.py:42-48 — which cannot
 * return silently wrong tokens) gives each clip of a small batch six workgroups that wait for each other's partial results.  If they
 * are ever not co-resident (another PROCESS filling the device, a CU mask, a debugger) an arrival poll expires after
 * "coop_timeout_ms" (default 250 ms; every workgroup then stops waiting, so the launch ends within about one time limit), the kernel
 * counts it in host-visible memory and the outputs of that call are INVALID.  The host is told in two ways:
 *   - an encode / decode / op call ENTERED after the failing launch has run returns L3AC_ECOOP (once) before doing anything.  The
 *     entry check reads host memory and does not synchronise: calls enqueued on an asynchronous stream before the failing launch
 *     ran are not stopped (they ran the cooperative form too and are suspect), and a program that ends first is never told.  The
 *     error text says how many calls were entered since the last synchronising check: the invalid call is one of them;
 *   - AUTHORITATIVE: l3ac_coop_timeout_pending / l3ac_coop_timeout_count synchronise the device first.  _count writes the number
 *     of expired polls since the last reset to *out and acts on them (the report is then considered delivered: no L3AC_ECOOP
 *     follows); _pending writes the number NOT yet acted on and leaves the state alone — read before and after a call it attributes
 *     a failure to that call without hiding an earlier one (what validate=True of the Python surface does).
 * Either way the context then leaves the cooperative form (trans_coop = 0: same bits, one workgroup per clip) and its arrival
 * counters are zeroed again, so the repeated call is correct.  Inside ONE process cooperative launches cannot starve each other:
 * every context claims the CUs its launches need in a per-device registry and a launch that does not fit runs in the
 * one-workgroup form.  Other processes sharing the device must set trans_coop = 0 (env L3AC_TRANS_COOP=0).
 * A hipGraph captured from a context must not be replayed concurrently with itself or with other work of the same context
 * (the slabs and counters are per context, like the workspace). */
int l3ac_coop_timeout_count(l3ac_ctx* ctx, int32_t reset, int64_t* out);
int l3ac_coop_timeout_pending(l3ac_ctx* ctx, int64_t* out);
/* CUs of `device` that live contexts of this process have claimed for cooperative launches (the registry above); -1 for a bad
 * ordinal.  No device call. */
int32_t l3ac_coop_claimed_cus(int32_t device);
/* Guard of the GRN fast path (layers.py:112-115; l3ac_config.grn_exact).  A context created with grn_exact = 1 evaluates
 * g / (g + 1e-8) per clip and keeps the smallest per-clip norm g = ||x||_2 any of its GRN layers has seen; this call
 * synchronises the device, writes that minimum to *out (+inf if no GRN has run) and optionally resets it.  The fast path
 * (grn_exact = 0) is exact whenever the reported minimum is >= 0.25. */
int l3ac_grn_min_norm(l3ac_ctx* ctx, int32_t reset, float* out);
int32_t l3ac_hop_length(const l3ac_ctx* ctx);

/* encode_audio: audio [batch][samples] (row stride `audio_stride` floats) is right-padded with zeros to a
 * multiple of hop_length (codec.py:79-84); n_tok = ceil(samples / hop).
 *   q_feature      [batch][n_tok][feature_dim] fp32
 *   indices        [batch][n_tok]              int32
 *   level_indices  [batch][n_tok][n_levels]    fp32   (may be NULL) */
int l3ac_encode(l3ac_ctx* ctx, const float* audio, int32_t batch, int32_t samples, int64_t audio_stride,
                float* q_feature, int32_t* indices, float* level_indices, void* stream);

/* decode_audio: from q_feature, or — when q_feature is NULL — from indices (vq/__init__.py:20-23).
 *   audio_out [batch][n_tok * hop_length] fp32, NOT trimmed (the caller slices, example.py:28). */
int l3ac_decode(l3ac_ctx* ctx, const float* q_feature, const int32_t* indices, int32_t batch, int32_t n_tok,
                float* audio_out, void* stream);

/* Ragged batches: clips of different lengths in one call.  Clip i's outputs are bit-identical to the
 * same call on that clip alone, and zero after its own tokens / samples; what lies after its own length in the inputs is never
 * read into its results, whatever it holds.  The per-clip lengths are HOST arrays of `batch` entries, read during the call (they
 * pick launch forms) and handed to the device as kernel arguments: the caller may overwrite them as soon as the call returns,
 * and a captured graph replays the lengths it was captured with.  No allocation once l3ac_reserve(batch, max_samples) has run.
 * Refused (L3AC_EINVAL) on a context created with grn_exact = 1: its per-clip GRN norm would include the padding.
 *
 * l3ac_encode_ragged: audio [batch][max_samples] (row stride audio_stride); samples[i] in [1, max_samples].
 *   q_feature / indices / level_indices as l3ac_encode with n_tok = ceil(max_samples / hop); clip i's first
 *   ceil(samples[i] / hop) tokens are those of l3ac_encode on its samples[i] samples alone, the rest are zero. */
int l3ac_encode_ragged(l3ac_ctx* ctx, const float* audio, int32_t batch, int32_t max_samples, int64_t audio_stride,
                       const int32_t* samples, float* q_feature, int32_t* indices, float* level_indices, void* stream);

/* l3ac_decode_ragged: q_feature [batch][max_tok][feature_dim] or (q_feature NULL) indices [batch][max_tok]; n_tok[i] in
 *   [1, max_tok] with n_tok[i] * en_coder_compress_rate >= 2.  audio_out [batch][max_tok * hop]: clip i's first n_tok[i] * hop
 *   samples are l3ac_decode of its first n_tok[i] tokens alone, the rest are zero.  Tokens after a clip's own never reach
 *   l3ac_bad_index_count. */
int l3ac_decode_ragged(l3ac_ctx* ctx, const float* q_feature, const int32_t* indices, int32_t batch, int32_t max_tok,
                       const int32_t* n_tok, float* audio_out, void* stream);

/* ---- quantiser kernels, context-free --------------------------------------------------------------- */

/* Fused FSQ (vq/__init__.py:25-30 + vq/fsq.py:30-68, eval): x [n][feat] -> q_feature [n][feat], indices [n],
 * level_indices [n][n_levels] (NULL to skip), latents [n][n_levels] (NULL to skip; test hook).
 * w_in [n_levels][feat], b_in [n_levels], w_out [feat][n_levels], b_out [feat] are device pointers.
 * With x == NULL the `latents` buffer is an INPUT (project_in skipped). */
int l3ac_fsq_forward(const float* x, int64_t n, int32_t feat, const int32_t* levels, int32_t n_levels,
                     const float* w_in, const float* b_in, const float* w_out, const float* b_out,
                     float* q_feature, int32_t* indices, float* level_indices, float* latents, void* stream);

/* The rounding half of the quantiser on its own: SuperFSQ.quantize_act_value (vq/fsq.py:56-65) ->
 * level_indices_to_indices (:67-68) -> inv_act (:21) -> project_out (vq/__init__.py:29).  act [n][n_levels] holds the
 * activation values in [0, 1], i.e. what tanh_act (vq/fsq_act.py:38-39) returns, so no transcendental sits between the
 * input and the rounding: exact k + 0.5 products and their one-ulp neighbours can be presented bit for bit. */
int l3ac_fsq_quantize_act(const float* act, int64_t n, int32_t feat, const int32_t* levels, int32_t n_levels,
                          const float* w_out, const float* b_out, float* q_feature, int32_t* indices,
                          float* level_indices, void* stream);

/* VQEmbed.to_features (vq/__init__.py:20-23): indices [n] -> q_feature [n][feat]. */
int l3ac_fsq_decode(const int32_t* indices, int64_t n, int32_t feat, const int32_t* levels, int32_t n_levels,
                    const float* w_out, const float* b_out, float* q_feature, void* stream);

/* Measurement aid (no reference counterpart): the quantiser kernel's grid and per-lane access pattern at feat = 128, 6 levels
 * — 512 B read, 512 + 4 + 24 B written per token — with no arithmetic: the HBM rate this access pattern can reach on the
 * box, printed beside the quantiser's own rate by bench.py (`fsq_kernel.copy_ceiling`). */
int l3ac_fsq_copy_ceiling(const float* x, int64_t n, float* q_feature, int32_t* indices, float* level_indices, void* stream);
/* The same copy at a given residency (workgroups per CU, 1 .. 8; 0 = as above: the quantiser kernel's own residency).  The copy kernel uses
 * no LDS and few registers, so its best rate is at a higher residency than the quantiser's: bench.py measures both and divides by the best. */
int l3ac_fsq_copy_ceiling_at(const float* x, int64_t n, float* q_feature, int32_t* indices, float* level_indices, int32_t blocks_per_cu,
                             void* stream);

/* Explicit-codebook nearest neighbour (the search FSQ is the closed form of):
 * queries [n][dim] (= tanh(latents)), codebook [k][dim] (= indices_to_codes(arange(k)), vq/fsq.py:80-81);
 * out_idx[i] = argmin_k ||q_i - c_k||^2, lowest k on exact ties.  dim <= 8.
 * The result is DEFINED by dist = sum_d (q_d - c_d)^2 accumulated with fmaf in dimension order and strict '<' over
 * increasing k.  A query for which no code compares below +inf (a NaN or Inf coordinate, or distances that all overflow)
 * gets index 0, as torch.argmin does on an all-NaN or all-inf row: out_idx is always an index into the codebook.
 * From 5 120 queries on the candidates are first screened on the fp32 matrix cores and then decided by
 * exactly that arithmetic (kernels/fsq.hip, "screened form"), so every size returns the same bits.
 * `scratch` is a caller-owned device buffer of at least l3ac_vq_argmin_scratch_bytes(n, k, form) bytes (partial minima of
 * the codebook slices, code norms, the list of queries that need the full direct-form search): the call allocates nothing
 * and can be captured into a hipGraph.  n < 2^31.
 * `form`: 0 = automatic; 1 = the direct-form scan wherever the screened form would run (the two are compared by
 * tests/test_gpu_blocks.py and timed side by side by tools/vq_argmin_bench.py).  An argument of the call, not library state:
 * nothing another thread does can change what a call — or a graph captured from it — computes. */
int64_t l3ac_vq_argmin_scratch_bytes(int64_t n, int32_t k, int32_t form);
int l3ac_vq_argmin(const float* queries, int64_t n, const float* codebook, int32_t k, int32_t dim, int32_t* out_idx,
                   void* scratch, int64_t scratch_bytes, int32_t form, void* stream);

/* ---- token wire format (no reference counterpart: the reference keeps int32 indices, vq/fsq.py:68) ---------------
 * Per clip, token t occupies bits [t*bits, (t+1)*bits) of a little-endian bit stream, zero-padded to whole 32-bit
 * words; bits = ceil(log2(codebook size)) (17 at 1kbps, 18 at 3kbps).
 *   indices [batch][n_tok] int32  <->  packed [batch][words_per_clip] uint32,  words_per_clip >= ceil(n_tok*bits/32). */
int l3ac_pack_indices(const int32_t* indices, int32_t batch, int32_t n_tok, int32_t bits, uint32_t* packed,
                      int32_t words_per_clip, void* stream);
int l3ac_unpack_indices(const uint32_t* packed, int32_t batch, int32_t n_tok, int32_t bits, int32_t words_per_clip,
                        int32_t* indices, void* stream);

/* ---- sample-rate conversion (the reference resamples on the CPU before encoding: example.py, librosa.resample) ---------
 * scipy.signal.resample_poly(x, up, down) with its defaults, for in_rate -> out_rate: g = gcd, up = out_rate / g,
 * down = in_rate / g, half_len = 10 max(up, down), prototype firwin(2 half_len + 1, 1 / max(up, down), window=('kaiser', 5.0)) * up
 * (designed on the host in fp64, each tap rounded once to fp32), zero padding at both ends, n_out = ceil(n_in up / down).
 * Supported: positive rates whose reduced max(up, down) <= 1024 (every standard rate from 8 to 192 kHz to and from 16 kHz);
 * anything else returns L3AC_EINVAL before any device work.  Context-free, like l3ac_pack_indices.
 *   l3ac_resample_length: n_out, or < 0 for unsupported rates / a negative n_in.
 *   l3ac_resample_bank:   HOST only: the polyphase bank's length in floats (0 when in_rate == out_rate), or < 0 for unsupported
 *                         rates; fills `bank` (host memory) when it is non-null and cap >= that length.  The caller copies it to
 *                         the device once per rate pair.
 *   l3ac_resample:        x [batch][x_stride] (first n_in samples of each row) -> y [batch][y_stride] (first n_out samples);
 *                         `bank` is the DEVICE copy of l3ac_resample_bank's output (unused when in_rate == out_rate: a copy).
 *                         fp32 fmaf chain per output in a fixed tap order: the bits of a clip do not depend on the batch, its
 *                         position in it, the strides or the launch geometry.  Enqueue only; capturable into a hipGraph. */
int64_t l3ac_resample_length(int32_t in_rate, int32_t out_rate, int64_t n_in);
int64_t l3ac_resample_bank(int32_t in_rate, int32_t out_rate, float* bank, int64_t cap);
int l3ac_resample(const float* x, int32_t batch, int64_t n_in, int64_t x_stride, int32_t in_rate, int32_t out_rate,
                  const float* bank, float* y, int64_t y_stride, void* stream);

/* ---- long recordings as chunk rows (reference: ChunkData, l3ac/codec.py:159-188) ----------------------
 * A recording of n frames is cut into chunks of chunk_len frames, each but the first preceded by the prefix_len frames before it:
 * chunk j covers [j * chunk_len - (j ? prefix_len : 0), min(n, (j + 1) * chunk_len)).  The chunks of a batch of recordings are the rows of
 * one ragged call (l3ac_encode_ragged / l3ac_decode_ragged); merging drops every chunk's prefix again.  Context-free, like
 * l3ac_pack_indices.  Frames hold `c` 4-byte elements (fp32 or int32: moved bit for bit, no arithmetic).
 *   l3ac_chunk_plan:  HOST only.  frames[i] >= 1 frames per recording, first rounded up to a multiple of round_to (audio: the hop, the
 *                     zero padding of codec.py:79-84; 1 otherwise); chunk_len > prefix_len >= 0.  Returns the number of chunks N, rows
 *                     numbered 0 .. N - 1 recording after recording, and fills desc_out when it is non-null (cap >= N); < 0
 *                     (L3AC_EINVAL, nothing written) on bad arguments or a cap that is too small.  The one place the geometry is computed.
 *   l3ac_chunk_cut:   src [recs][src_stride][c] -> dst [rows][dst_row_frames][c]: row desc.row gets frames [start, start + frames) of
 *                     recording desc.rec, its last desc.pad frames (the rounding) as zeros, never read.  Frames of a row after the
 *                     chunk's own are not written.
 *   l3ac_chunk_merge: src [rows][src_row_frames][c] -> dst [recs][dst_stride][c]: frames [prefix, frames) of row desc.row go to
 *                     [start + prefix, start + frames) of recording desc.rec; a recording's last chunk also zeroes its row from
 *                     start + frames to out_frames (<= dst_stride).  Called with a whole plan it writes every frame below out_frames
 *                     of every recording exactly once.
 * `desc` is a HOST array of `count` descriptors (any slice of a plan, in any order), checked against the shapes given before
 * anything is launched and handed to the device as kernel arguments, 112 per launch: the caller may change it as soon as the call
 * returns, a captured graph replays what it captured.  16-byte accesses where source and destination of a span are congruent
 * modulo 16 bytes (always for c % 4 == 0 with 16-byte aligned rows), dword accesses otherwise.  Enqueue only. */
typedef struct l3ac_chunk_desc {
    int32_t rec;     /* recording: row of the [recs][stride] layout */
    int32_t row;     /* row of the chunk layout */
    int64_t start;   /* the chunk's first frame in its recording, prefix included */
    int32_t frames;  /* frames of the chunk, prefix included */
    int32_t prefix;  /* of them, frames that belong to the previous chunk: prefix_len, 0 for a recording's first chunk */
    int32_t pad;     /* of them, frames at the end that exist only through rounding: cut writes zeros */
    int32_t last;    /* 1 for a recording's last chunk */
} l3ac_chunk_desc;
int64_t l3ac_chunk_plan(const int64_t* frames, int32_t batch, int64_t chunk_len, int64_t prefix_len, int32_t round_to,
                        l3ac_chunk_desc* desc_out, int64_t cap);
int l3ac_chunk_cut(const void* src, int32_t recs, int64_t src_stride, int32_t c, const l3ac_chunk_desc* desc, int32_t count,
                   void* dst, int32_t rows, int64_t dst_row_frames, void* stream);
int l3ac_chunk_merge(const void* src, int32_t rows, int64_t src_row_frames, int32_t c, const l3ac_chunk_desc* desc, int32_t count,
                     void* dst, int32_t recs, int64_t dst_stride, int64_t out_frames, void* stream);

/* ---- streaming sessions: the state carried between pushes ---------------------------------------------
 * S live streams are cut with a step of CL frames and a look-back of P frames: chunk k of a stream covers
 * [max(0, k * CL - P), (k + 1) * CL) and emits what lies at or after k * CL; P may be at or above CL, which l3ac_chunk_plan refuses.
 * A session keeps one state buffer [streams][state_frames][c] (state_frames >= P + CL): stream i's row holds, from frame 0, the
 * frames that can still be needed, its look-back followed directly by its pending frames.  How many they are is a host value.
 * A push of new frames fresh [streams][fresh_stride][c] (fresh_frames <= fresh_stride of them valid per row; may be null when no
 * descriptor takes any) runs in rounds, each stream completing at most one chunk per round:
 *   l3ac_stream_gather: row desc.row of rows [n_rows][row_frames][c] = state[slot][0 : held] ++ fresh[slot][off : off + take] ++
 *                       pad zero frames.  Frames of a row after these are not written.
 *   l3ac_stream_carry:  state[slot][0 : keep] = frames [held + take - keep, held + take) of row desc.row: the stream's next look-back,
 *                       read from the row just built because it overlaps what the state held (no kernel moves a span onto an
 *                       overlapping span of its own buffer).
 *   l3ac_stream_append: state[slot][held : held + take] = fresh[slot][off : off + take]: what a push leaves pending.
 *   l3ac_stream_emit:   rows [n_rows][row_frames][c] (a ragged call's output) -> dst [streams][dst_stride][c]: frames
 *                       [prefix, held + take + pad) of row desc.row go to dst[slot][out ...], followed by `zero` zero frames, all
 *                       below out_frames <= dst_stride.  A descriptor with held + take + pad == prefix writes zeros only.
 * Each call reads only the fields named for it.  Context-free, 4-byte elements moved bit for bit, like the chunk entries; `desc` is a
 * HOST array, checked against the shapes before anything is launched (bounds, and that no two descriptors write the same frame) and
 * handed to the device as kernel arguments, 72 per launch: graph-safe.  Enqueue only. */
typedef struct l3ac_stream_desc {
    int32_t slot;    /* stream: row of the state, of the new frames and of the output */
    int32_t row;     /* row of the rows layout */
    int32_t held;    /* frames taken from the front of the stream's state row */
    int32_t take;    /* new frames taken */
    int64_t off;     /* ... from this frame of the stream's row of new frames */
    int32_t pad;     /* zero frames at the row's end (a flushed last chunk rounded up to a whole hop) */
    int32_t keep;    /* carry: frames the stream keeps as its next look-back */
    int32_t prefix;  /* emit: leading frames of the row that are look-back, dropped */
    int32_t zero;    /* emit: zero frames written after the emitted ones */
    int64_t out;     /* emit: first frame written in the stream's output row */
} l3ac_stream_desc;
int l3ac_stream_gather(const void* state, int32_t streams, int64_t state_frames, const void* fresh, int64_t fresh_frames, int64_t fresh_stride,
                       int32_t c, const l3ac_stream_desc* desc, int32_t count, void* rows, int32_t n_rows, int64_t row_frames, void* stream);
int l3ac_stream_carry(const void* rows, int32_t n_rows, int64_t row_frames, int32_t c, const l3ac_stream_desc* desc, int32_t count, void* state,
                      int32_t streams, int64_t state_frames, void* stream);
int l3ac_stream_append(const void* fresh, int64_t fresh_frames, int64_t fresh_stride, int32_t c, const l3ac_stream_desc* desc, int32_t count,
                       void* state, int32_t streams, int64_t state_frames, void* stream);
int l3ac_stream_emit(const void* rows, int32_t n_rows, int64_t row_frames, int32_t c, const l3ac_stream_desc* desc, int32_t count, void* dst,
                     int32_t streams, int64_t dst_stride, int64_t out_frames, void* stream);

/* ---- streaming sample-rate conversion: packets in, l3ac_resample's bits out ---------------------------
 * S live streams at in_rate are converted to out_rate push by push.  With l3ac_resample's up, down, half_len and
 * K = ceil((2 half_len + 1) / up), output m of a stream reads its inputs i(m) - (K - 1) .. i(m), i(m) = (m down + half_len) div up, with the
 * taps of phase (m down + half_len) mod up.  A stream that has received N inputs and emitted E outputs keeps its last `held` inputs
 * (0 <= held <= K - 1) in its row of a state buffer [streams][state_stride], state_stride >= l3ac_resample_stream_state().  A push of n new
 * inputs makes N' = N + n and emits outputs [E, E'):
 *   not ended:  E' = max(0, ceil((N' up - half_len) / down))   exactly the outputs whose newest input exists: the output lags the input
 *                                                              by half_len / up input samples;
 *               held' = N' - max(0, i(E') - (K - 1))
 *   ended:      E' = ceil(N' up / down), held' = 0             inputs past the end count as zeros, as in l3ac_resample; the slot is fresh.
 * The device is told none of N, E: a descriptor carries q0 = E down + half_len - (N - held) up, which lies in [0, K up), so nothing handed
 * over grows with the age of a stream.  The stream's input is the virtual row state_in[slot][0 : held] ++ fresh[slot][0 : take] ++ zeros
 * (zeros before it as well), read in place; output j of the push has its newest input at row position (q0 + j down) div up.
 *   l3ac_resample_stream_state: HOST only: floats per state row, K - 1 rounded up to a multiple of 4; < 0 for unsupported rates.
 *   l3ac_resample_stream:       ONE launch per ResampleStreamBlock of descriptors (128): out[slot][0 : count] = the stream's outputs, zeros from
 *                               there to out_frames (<= out_stride; every element below out_frames of a described stream's row is written
 *                               once, rows without a descriptor are not touched), and state_out[slot][0 : keep] = the last `keep` frames of
 *                               state_in[slot][0 : held] ++ fresh[slot][0 : take].  state_in and state_out are two buffers that must not
 *                               overlap (a session alternates them; describe idle streams too, with keep = held, so that their state
 *                               follows); `bank` is the DEVICE copy of l3ac_resample_bank's output.  out may be null when out_frames is 0,
 *                               fresh when no descriptor takes any.  Equal rates: out[slot][0 : take] = fresh[slot][0 : take] bit for bit
 *                               (held, keep must be 0 and count == take; the state buffers and the bank are not used).
 * Bit guarantee: every output is the fp32 fmaf chain over t = 0 .. K - 1 in that order from +0, l3ac_resample's documented arithmetic;
 * for finite input, and however a stream's samples are split over pushes, the concatenation of what it emits equals l3ac_resample of the
 * whole stream bit for bit.  `desc` is a HOST array with at most one descriptor per stream, checked before anything is launched (stream
 * in range, held within the state row, take within the packet, count within the output row, keep <= held + take, q0 in [0, K up)) and
 * handed to the device as kernel arguments: graph-safe as far as the entry goes.  Enqueue only. */
typedef struct l3ac_resample_stream_desc {
    int32_t slot;    /* stream: row of the state buffers, of the new samples and of the output */
    int32_t held;    /* samples at the front of the stream's row of state_in */
    int32_t take;    /* new samples, from the front of the stream's row of `fresh` */
    int32_t count;   /* outputs this push emits */
    int32_t keep;    /* samples the stream holds afterwards: the last `keep` of held + take */
    int32_t q0;      /* E down + half_len - (N - held) up */
} l3ac_resample_stream_desc;
int64_t l3ac_resample_stream_state(int32_t in_rate, int32_t out_rate);
int l3ac_resample_stream(const float* state_in, float* state_out, int32_t streams, int64_t state_stride, const float* fresh, int64_t fresh_frames,
                         int64_t fresh_stride, int32_t in_rate, int32_t out_rate, const float* bank, const l3ac_resample_stream_desc* desc,
                         int32_t count, float* out, int64_t out_frames, int64_t out_stride, void* stream);

/* ---- quality metrics: STFT, log-mel, log-mel distance, MSE / SNR / SI-SDR ------------------------------
 * No reference counterpart: the reference's demo ends with ((sample_audio - generated_audio) ** 2).mean() on the host.
 * Spec (fp64): a clip of n >= 1 samples has F(n) = 1 + n / hop frames; frame f covers samples [f hop - n_fft/2, f hop + n_fft/2), zeros
 * outside [0, n); w[j] = 0.5 - 0.5 cos(2 pi j / n_fft) (periodic Hann); X[f][k] = sum_j w[j] x_f[j] exp(-2 pi i j k / n_fft), k = 0 .. n_fft/2:
 * torch.stft(x, n_fft, hop, n_fft, hann_window(n_fft), center=True, pad_mode="constant", onesided=True).  Mel weights: HTK scale
 * mel(f) = 2595 log10(1 + f / 700), no normalisation, n_mels + 2 points p equally spaced in mel from 0 to sample_rate / 2, triangles on the
 * bin frequencies f_k = k sample_rate / n_fft: W[m][k] = max(0, min((f_k - p_m) / (p_m+1 - p_m), (p_m+2 - f_k) / (p_m+2 - p_m+1))).
 * Log-mel: L[f][m] = log10(max(sum_k W[m][k] (re^2 + im^2), 1e-10)).  Distance of a pair at one scale: the mean of |L_ref - L_est| over
 * the clip's F(n) n_mels cells.  Time domain, per clip over its own n samples, in fp64: mse = sum (r - e)^2 / n,
 * snr_db = 10 log10(sum r^2 / sum (r - e)^2), si_sdr_db = 10 log10(a^2 sum (r - mu_r)^2 / sum ((e - mu_e) - a (r - mu_r))^2) with
 * a = cov(r, e) / var(r) (Le Roux et al., zero-mean form); a zero denominator gives +inf and 0 / 0 gives nan, as IEEE division does.
 * Supported: n_fft a multiple of 16 in 16..2048, hop a multiple of 4 in 4..n_fft, n_mels in 1..256, sample_rate > 0, batch <= 65535;
 * anything else returns L3AC_EINVAL (or a negative count) before any device work.  Context-free, like l3ac_resample.
 *   l3ac_stft_frames:       HOST only: F(samples) = 1 + samples / hop; < 0 for samples < 1 or hop < 1.
 *   l3ac_stft_basis:        HOST only: the window-folded DFT basis, (n_fft + 2) * n_fft floats as [n_fft + 2][n_fft]: row 2k holds
 *                           w[j] cos(2 pi (j k mod n_fft) / n_fft), row 2k + 1 holds -w[j] sin(...), designed in fp64 with the phase reduced in
 *                           integers, each entry rounded once to fp32.  Returns the length; fills `basis` (host memory) when it is non-null
 *                           and cap >= that length.  The caller copies it to the device once per n_fft (16-byte aligned there).
 *   l3ac_mel_weights:       HOST only: W as [n_mels][n_fft/2 + 1] floats, designed in fp64, each entry rounded once to fp32; same protocol.
 *                           The two fp32 tables are part of the spec: the bit guarantees below are stated on them.
 *   l3ac_mel_scratch_bytes: the minimum scratch of the three calls below for these shapes (n_mels is validated, the size does not depend
 *                           on it): the clips' lengths, both signals staged as zero-padded rows (2 batch (max_samples + 2 n_fft) floats at
 *                           most), one fp64 per frame, and the spectra of 128 frames of both signals.  < 0 for unsupported parameters.
 *   l3ac_stft:              audio [batch][audio_stride] -> spec [batch][F(max_samples)][n_fft/2 + 1][2] (re, im).  `samples`: HOST array of
 *                           batch lengths in 1..max_samples, or NULL (every clip has max_samples); samples at or after a clip's length are
 *                           never read into a result, and the rows of `spec` after a clip's own F(samples[i]) frames are zero.  `basis` is
 *                           the DEVICE copy of l3ac_stft_basis' output.  Every real and imaginary part is one exact-fp32 chain of fused
 *                           multiply-adds over j in the fixed k order of l3ac_gemm_f32 from +0.
 *   l3ac_log_mel:           the same arguments plus `weights` (the DEVICE copy of l3ac_mel_weights' output) -> out
 *                           [batch][F(max_samples)][n_mels], zero after a clip's own frames.  Power = fma(re, re, im im); each cell is one
 *                           fmaf chain over its filter's run of bins (first to last non-zero weight) in increasing k from +0, then
 *                           log10f, and exactly -10 when the sum is <= 1e-10f (every cell of an empty filter, every cell of silence).
 *   l3ac_mel_distance:      ref and est [batch][*_stride] with common lengths -> out [batch] fp64: per cell |L_ref - L_est| in fp64 from
 *                           the fp32 cells l3ac_log_mel computes, summed per frame and then per clip in a fixed order, divided by
 *                           F(samples[i]) n_mels.  No floating-point atomics.
 *   l3ac_signal_metrics:    ref and est as above -> out [batch][3] fp64 = mse, snr_db, si_sdr_db.  Samples converted exactly to fp64; one
 *                           workgroup per clip, two passes with fixed per-thread strides (1024) and a fixed tree: pass 1 the sums (the
 *                           means, a, and sum (r - e)^2 directly), pass 2 sum (r - mu_r)^2 and the residual energy directly, never by
 *                           expanding the square.  `scratch` holds the clips' lengths only: batch int32, unused (may be NULL) when
 *                           `samples` is NULL.
 * Bit guarantee: a clip's results do not depend on the batch it is in, on its row, on the row strides, or on the scratch size (a scratch
 * above the minimum lets one product take more frames; the frames that straddle two staged clips are computed and never stored).
 * `samples` is handed to the device as kernel arguments (248 per launch): graph-safe.  `scratch` is a caller-owned, 256-byte aligned
 * device buffer: the calls allocate nothing, do not synchronise, and can be captured into a hipGraph.  Enqueue only. */
int64_t l3ac_stft_frames(int64_t samples, int32_t hop);
int64_t l3ac_stft_basis(int32_t n_fft, float* basis, int64_t cap);
int64_t l3ac_mel_weights(int32_t sample_rate, int32_t n_fft, int32_t n_mels, float* w, int64_t cap);
int64_t l3ac_mel_scratch_bytes(int32_t batch, int64_t max_samples, int32_t n_fft, int32_t hop, int32_t n_mels);
int l3ac_stft(const float* audio, int32_t batch, int64_t max_samples, int64_t audio_stride, const int32_t* samples, int32_t n_fft, int32_t hop,
              const float* basis, float* spec, void* scratch, int64_t scratch_bytes, void* stream);
int l3ac_log_mel(const float* audio, int32_t batch, int64_t max_samples, int64_t audio_stride, const int32_t* samples, int32_t n_fft, int32_t hop,
                 const float* basis, const float* weights, int32_t n_mels, float* out, void* scratch, int64_t scratch_bytes, void* stream);
int l3ac_mel_distance(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples,
                      const int32_t* samples, int32_t n_fft, int32_t hop, int32_t n_mels, const float* basis, const float* weights, double* out,
                      void* scratch, int64_t scratch_bytes, void* stream);
int l3ac_signal_metrics(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples,
                        const int32_t* samples, double* out, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- speech intelligibility: STOI and ESTOI --------------------------------------------------------------
 * STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) of clip pairs AT 10 kHz, with the constants of the published implementations:
 * frames of 256 samples at hop 128 zero-padded to n_fft 512, 15 third-octave bands from 150 Hz, segments of 30 frames, clipping at
 * -15 dB, 40 dB of dynamic range, eps = 2^-52.  A clip of L samples has A(L) analysis frames: 0 for L <= 256, else
 * ceil((L - 256) / 128); frame f starts at 128 f < L - 256.  Spec (fp64, on the two fp32 tables below; DESIGN.md section 3.13 in full):
 * the reference's frame energies e_f = sum_j (w[j] x[128 f + j])^2 decide which frames stay, 20 log10(sqrt(e_f) + eps) > max_f(...) - 40,
 * the same frames in both signals; each signal is rebuilt from its K kept frames by overlap-add of w[j] x[128 f_q + j] (fp32 on the
 * device, at most two terms per sample in the order of q); the T = K - 1 spectra of the rebuilt signal are the basis applied to
 * s[128 t .. 128 t + 256); bands[t][i] = sqrt(sum of re^2 + im^2 over the band's run of bins) is an fp32 cell; every m = 30 .. T gives
 * one d_m from the 15 x 30 blocks of frames m - 30 .. m - 1 (STOI: rows scaled to the reference's norm, clipped at (1 + 10^(15/20)) x,
 * centred, normalised, sum x y' / 15;  ESTOI: rows, then columns centred and normalised, sum x y / 30), in fp64; the value is the mean
 * of the d_m.  T < 30: both values are exactly 1e-5 (the published implementations' convention) and frames_out tells.
 *   l3ac_stoi_frames:        HOST only: A(samples); < 0 for samples < 1.
 *   l3ac_stoi_window:        HOST only: w[j] = hanning(258)[1 + j], 256 floats, designed in fp64 and rounded once; the size-query protocol
 *                            of l3ac_stft_basis (returns the length; fills the buffer when it is non-null and cap >= that length).
 *   l3ac_stoi_basis:         HOST only: the window-folded basis [514][256]: row 2k = w[j] cos(2 pi (j k mod 512) / 512), row 2k + 1 =
 *                            -w[j] sin(...), k = 0 .. 256; same protocol.  Row 0 is the window.  The caller copies it to the device once.
 *   l3ac_stoi_bands:         HOST only: runs[2 i], runs[2 i + 1] = the bins [lo, hi) of band i = 0 .. 14 (30 ints): lo = the bin nearest to
 *                            150 * 2^((2 i - 1) / 6) Hz, hi = the bin nearest to 150 * 2^((2 i + 1) / 6) Hz, bin k at k * 10000 / 512 Hz.
 *   l3ac_stoi_scratch_bytes: the minimum scratch of l3ac_stoi for these shapes; < 0 for batch outside 1..65535 or clips too long.
 *   l3ac_stoi:               ref and est [batch][*_stride] at 10 kHz with common lengths (`samples`: HOST array of batch lengths in
 *                            1..max_samples, or NULL) -> out [batch][2] fp64 = stoi, estoi; frames_out [batch] int32 (device) = T;
 *                            bands_out (device, or NULL) [2][batch][A(max_samples) - 1][15] fp32: the reference's, then the estimate's
 *                            band cells, zero at and after a clip's own T frames.  `basis` is the DEVICE copy of l3ac_stoi_basis' output.
 *                            Every bad argument (batch 0 or above 65535, a length outside 1..max_samples, a row stride below
 *                            max_samples, a null buffer, a scratch below the minimum, clips too long) is L3AC_EINVAL before any device work.
 * Bit guarantee and calling convention: as the quality metrics above (a clip's results do not depend on the batch, its row, the strides
 * or the scratch size; no atomics; enqueue only, nothing allocated, no synchronisation, capturable). */
int64_t l3ac_stoi_frames(int64_t samples);
int64_t l3ac_stoi_basis(float* basis, int64_t cap);
int64_t l3ac_stoi_window(float* window, int64_t cap);
int l3ac_stoi_bands(int32_t* runs);
int64_t l3ac_stoi_scratch_bytes(int32_t batch, int64_t max_samples);
int l3ac_stoi(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples, const int32_t* samples,
              const float* basis, double* out, int32_t* frames_out, float* bands_out, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- loudness: BS.1770-4 integrated loudness and loudness normalisation ---------------------------------------
 * Integrated loudness of MONO clips (one channel of weight 1.0) after ITU-R BS.1770-4, in fp64 throughout: K-weighting (two biquads in
 * cascade, designed on the host by De Man's closed forms evaluated AT the sample rate, the choice pyloudnorm makes; at 48 kHz they are
 * the standard's table), blocks of 400 ms at 75 % overlap, the absolute gate at -70 LKFS and the relative gate 10 LU below the loudness
 * of the absolutely gated blocks.  A rate fs is supported iff fs % 10 == 0 and 8000 <= fs <= 192000; step = fs / 10.  A clip of n samples
 * has S = n / step whole steps and J(n) = max(S - 3, 0) blocks; samples at or after S step enter nothing but the peak.  The filter
 * starts from rest at sample 0.  L = -inf exactly when no block passes both gates (J = 0 and digital silence included).  The recursion
 * runs in parallel over the steps (a zero-state pass, a per-clip scan of the 4-value state, an energy pass).
 *   l3ac_loudness_coeffs:        HOST only: out[0..11] = the two stages' b0 b1 b2 a0 a1 a2 (a0 = 1), out[12..27] = M [4][4] row-major, the
 *                                matrix that advances the cascade's state (s1, s2 of stage 1, s1, s2 of stage 2; transposed direct form II)
 *                                over one step of zero input.  The size-query protocol of l3ac_stft_basis (returns 28; fills the buffer
 *                                when it is non-null and cap >= 28).  < 0 with a message for an unsupported rate.
 *   l3ac_loudness_blocks:        HOST only: J(samples); < 0 for samples < 1 or an unsupported rate.
 *   l3ac_loudness_scratch_bytes: the minimum scratch of l3ac_loudness for these shapes; < 0 for batch outside 1..65535, max_samples outside
 *                                1..2^31 - 1 or an unsupported rate.
 *   l3ac_loudness:               audio [batch][audio_stride] (`samples`: HOST array of batch lengths in 1..max_samples, or NULL) -> stats
 *                                [batch][2] fp64 = L in LKFS, the sample peak max |x| over the clip's own samples; counts [batch][2] int32 =
 *                                J, the blocks that pass both gates; momentary (device, or NULL) [batch][J(max_samples)] fp64 = the blocks'
 *                                loudness l_j, -inf at and after a clip's own J.  All outputs are device buffers.
 *   l3ac_loudness_gain:          stats [batch][2] (device, as written by l3ac_loudness) -> gain [batch][2] fp64 (device) = g_db, 10^(g_db/20):
 *                                g_db = target_lufs - L, with a peak_limit_db (NaN: none) and peak > 0 at most peak_limit_db -
 *                                20 log10(peak), and exactly 0 when L = -inf.  No host synchronisation.
 *   l3ac_apply_gain:             out[b][i] = (float)((double)audio[b][i] * gain[b * gain_stride]) for i below the clip's length, 0 from there
 *                                to max_samples.  out == audio is allowed.  16-byte accesses when both pointers are 16-byte aligned and
 *                                both strides multiples of 4 (the bits are the same either way).
 * Every bad argument (batch 0 or above 65535, a length outside 1..max_samples, a row stride below max_samples, a null buffer, a scratch
 * below the minimum, an unsupported rate, a non-finite target) is L3AC_EINVAL before any device work, with a message naming it.
 * Bit guarantee and calling convention: as the quality metrics above (a clip's results do not depend on the batch, its row, the strides
 * or the scratch size; no atomics; enqueue only, nothing allocated, no synchronisation, capturable).  There is no device table: the
 * coefficients and M travel as kernel arguments, so nothing needs a warm-up before a capture. */
int64_t l3ac_loudness_coeffs(int32_t sample_rate, double* out, int64_t cap);
int64_t l3ac_loudness_blocks(int64_t samples, int32_t sample_rate);
int64_t l3ac_loudness_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sample_rate);
int l3ac_loudness(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, int32_t sample_rate,
                  double* stats, int32_t* counts, double* momentary, void* scratch, int64_t scratch_bytes, void* stream);
int l3ac_loudness_gain(const double* stats, int32_t batch, double target_lufs, double peak_limit_db, double* gain, void* stream);
int l3ac_apply_gain(const float* audio, int64_t audio_stride, float* out, int64_t out_stride, int32_t batch, int64_t max_samples,
                    const int32_t* samples, const double* gain, int64_t gain_stride, void* stream);

/* ---- EBU R128: block loudness series, loudness range and true peak -------------------------------------------------
 * On the step energies e_s of the loudness meter above (the same rates, steps, filter and kernels): a block of W steps that starts at
 * step k has z_k = (((e_k + e_{k+1}) + ...) + e_{k+W-1}) / (W step), summed left to right (W = 4: the meter's own block, bit for bit), and
 * l_k = -0.691 + 10 log10 z_k.  A clip of S whole steps has K = max(S - W + 1, 0) such blocks, one every 100 ms.
 *   l3ac_r128_scratch_bytes: the minimum scratch of l3ac_r128_series and l3ac_r128_range (that of l3ac_loudness); the same refusals.
 *   l3ac_r128_series:        window_steps = W in 1..600 -> lufs [batch][K(max_samples)] fp64 = l_k, -inf at and after a clip's own K;
 *                            mean_square (or NULL) [batch][K(max_samples)] = z_k, 0 there; energies (or NULL) [batch][S(max_samples)] = e_s,
 *                            0 at and after a clip's own S; blocks (or NULL) [batch] int32 = the clip's own K.  lufs may be NULL only when
 *                            K(max_samples) = 0.
 *   l3ac_r128_range:         EBU Tech 3342 on the short-term blocks, W = 30 (3 s) every step (100 ms: 2.9 s of overlap, where Tech 3342 asks
 *                            for at least 2 s).  The gates decide on l as the meter's do: the absolute gate l_k > -70, the relative gate
 *                            l_k > G, G = -0.691 + 10 log10(mean of the absolutely gated z) - 20.  The g survivors' z are sorted ascending;
 *                            low = l of z[((g - 1) 10 + 50) / 100], high = l of z[((g - 1) 95 + 50) / 100] (integer division), lra = high -
 *                            low; g = 0: lra = 0 exactly, low = high = -inf.  stats [batch][5] fp64 = lra, low, high, the largest l_k
 *                            (short-term maximum), the largest l of the W = 4 blocks (momentary maximum), both -inf without a block;
 *                            counts [batch][3] int32 = K, the blocks above the absolute gate, g.  A clip of more than 16384 short-term
 *                            blocks (27 min) is refused before any device work.
 * True peak: the largest magnitude of the clip oversampled L times by l3ac_resample's own filter for fs -> L fs (21 taps a phase, the
 * same host design, the same fp32 fmaf chain per output: the bits of max |l3ac_resample(clip alone)|), L = 4 for 8000 <= fs < 96000,
 * L = 2 for 96000 <= fs <= 192000; samples before the clip and at and after its length are zero.
 *   l3ac_true_peak_factor:        HOST only: L; < 0 with a message for a rate outside 8000..192000.
 *   l3ac_true_peak_tile:          HOST only: the input positions one workgroup evaluates (no part of the bits).
 *   l3ac_true_peak_scratch_bytes: the minimum scratch of l3ac_true_peak; < 0 for batch outside 1..65535, max_samples outside 1..2^31 - 1
 *                                 or an unsupported rate.
 *   l3ac_true_peak:               stats [batch][2] fp64 (device) = max(peak, os), peak: os the oversampled maximum, peak = max |x|.
 * Every bad argument is L3AC_EINVAL before any device work, with a message naming it.  Bit guarantee and calling convention: as the
 * loudness meter's.  No device table: the taps travel as kernel arguments, so l3ac_true_peak can be captured as a process' first call.
 * Non-finite samples leave their own clip's results unspecified and no other clip's. */
int64_t l3ac_r128_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sample_rate);
int l3ac_r128_series(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, int32_t sample_rate,
                     int32_t window_steps, double* lufs, double* mean_square, double* energies, int32_t* blocks, void* scratch, int64_t scratch_bytes,
                     void* stream);
int l3ac_r128_range(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, int32_t sample_rate,
                    double* stats, int32_t* counts, void* scratch, int64_t scratch_bytes, void* stream);
int32_t l3ac_true_peak_factor(int32_t sample_rate);
int32_t l3ac_true_peak_tile(void);
int64_t l3ac_true_peak_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sample_rate);
int l3ac_true_peak(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, int32_t sample_rate,
                   double* stats, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- IIR filtering: scipy.signal.sosfilt one-shot and streaming, Butterworth designs -----------------------------
 * A cascade of 1 <= sections <= 8 second-order sections filters MONO clips, in fp64 throughout (the fp32 samples convert exactly).  `sos`
 * is a HOST array [sections][5] = b0 b1 b2 a1 a2 (a0 = 1: the caller has divided by it).  One sample through one section is one
 * transposed-direct-form-II step, y = b0 x + s1; s1 = b1 x - a1 y + s2; s2 = b2 x - a2 y, each product rounded before its sum (no
 * contraction): scipy's order.  The sections run in cascade; every clip starts from rest at its sample 0.  Every coefficient must be
 * finite and every section inside the stability triangle, |a2| < 1 and |a1| < 1 + a2 (first-order sections, b2 = a2 = 0, and the
 * identity 1 0 0 0 0 included).
 * The recursion runs in parallel over time in segments of SEG = l3ac_sosfilt_segment samples (256) anchored at sample 0, and SEG is
 * part of the definition of the bits: (A) every segment is filtered from a zero state and keeps its end state (2 sections values: s1, s2
 * of section 0, of section 1, ...); (B) per clip start_{s+1} = M start_s + end_s over the complete segments, where M advances the
 * cascade's state over SEG samples of zero input; M, the running state and the products are pairs of doubles hi + lo, the row of M
 * times the state summed in column order, then the end state added; (C) every segment is filtered again from hi(start_s), and that
 * is y.  M is designed on the device on every call, by the same step in pair arithmetic (coefficients as (c, 0)) on SEG zero samples
 * from each unit state: no table, no upload, nothing to warm up before a capture.
 *   l3ac_sosfilt_segment:       HOST only: SEG.
 *   l3ac_sosfilt_scratch_bytes: the minimum scratch of l3ac_sosfilt, and of l3ac_sosfilt_stream with batch = its descriptors and
 *                               max_samples = max(fresh_frames, 1); < 0 for batch outside 1..65535, max_samples outside 1..2^31 - 1 or
 *                               sections outside 1..8.
 *   l3ac_sosfilt:               audio [batch][audio_stride] fp32 (`samples`: HOST array of batch lengths in 1..max_samples, or NULL) -> out
 *                               [batch][out_stride], fp64 when out_f64 is non-zero, else fp32 = (float)y; zeros at and after a clip's length
 *                               up to max_samples.  out must not overlap audio.
 *   l3ac_sosfilt_matrix:        M of `sos` -> hi, lo: DEVICE buffers [2 sections][2 sections] fp64, row-major (the tests' view of it).
 *   l3ac_sosfilt_stream_state:  HOST only: doubles per state row, 8 sections; < 0 for sections outside 1..8.
 *   l3ac_sosfilt_stream:        one push of S live streams.  A stream at position p = s SEG + k carries in its row of a state buffer
 *                               [streams][state_stride] the start pair of its current segment (hi, then lo), its running true state and
 *                               its running zero-state state; k is the caller's.  A push continues both recursions of the stream's
 *                               current segment sample by sample, hands the completed segments' end states to the scan, and saves both
 *                               running states of the last, partial segment: out[slot][0 : take] = the filtered samples, zeros from there to
 *                               fresh_frames, and state_out[slot] = the stream's state afterwards (a stream that takes nothing is copied;
 *                               L3AC_SOS_END leaves the slot at rest: zeros; a descriptor with L3AC_SOS_FRESH starts from rest without
                               reading its state row, so a slot can be handed to a new stream at any time).  As many outputs as inputs, no latency, nothing to flush.  state_in and
 *                               state_out are two buffers that must not overlap (a session alternates them; a fresh buffer is zeros);
 *                               describe idle streams too, so that their state follows.  `desc` is a HOST array with at most one
 *                               descriptor per stream, handed to the device as kernel arguments.  out may be null when fresh_frames is 0.
 *                               However a stream is split over pushes and whatever the other streams do, the concatenation of its outputs
 *                               is l3ac_sosfilt of the whole stream bit for bit.
 *   l3ac_butter_sos:            HOST only: the bilinear Butterworth low-pass or high-pass of `order` 1..16 with pre-warping, in closed form,
 *                               K = tan(pi cutoff_hz / sample_rate): out [ceil(order / 2)][6] = b0 b1 b2 a0 a1 a2 with a0 = 1, scipy's
 *                               layout.  An odd order puts the first-order section first, b = (K, K, 0) / (1 + K) or (1, -1, 0) / (1 + K),
 *                               a = (1, (K - 1) / (K + 1), 0); pair k = 0 .. order / 2 - 1 follows with q = 2 sin(pi (2 k + 1) / (2 order)),
 *                               a0 = 1 + q K + K^2, a = (1, 2 (K^2 - 1) / a0, (1 - q K + K^2) / a0), b = (K^2, 2 K^2, K^2) / a0 or
 *                               (1, -2, 1) / a0.  The size-query protocol of l3ac_stft_basis; < 0 for an order outside 1..16 or a cutoff
 *                               outside (0, sample_rate / 2).
 * Every bad argument (sections outside 1..8, a non-finite coefficient, an unstable section, batch 0 or above 65535, a length outside
 * 1..max_samples, a row stride below max_samples, a null buffer, a scratch below the minimum, a descriptor out of range) is L3AC_EINVAL
 * before any device work, with a message naming it.  Bit guarantee and calling convention: as the quality metrics above (a clip's
 * output does not depend on the batch, its row, the strides or the scratch size; no atomics; enqueue only, nothing allocated, no
 * synchronisation; l3ac_sosfilt is capturable as the first call of a process). */
typedef struct l3ac_sosfilt_stream_desc {
    int32_t slot;    /* stream: row of the state buffers, of the new samples and of the output */
    int32_t k;       /* samples the stream's current segment has had: its position modulo SEG */
    int32_t take;    /* new samples, from the front of the stream's row of `fresh` */
    int32_t flags;   /* L3AC_SOS_END: the stream ends with this push, its slot is at rest afterwards; L3AC_SOS_FRESH: the stream begins
                        with this push (k = 0): nothing of state_in is read, whatever the slot held */
} l3ac_sosfilt_stream_desc;
enum { L3AC_SOS_END = 1, L3AC_SOS_FRESH = 2 };
int32_t l3ac_sosfilt_segment(void);
int64_t l3ac_sosfilt_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sections);
int l3ac_sosfilt(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, const double* sos,
                 int32_t sections, void* out, int64_t out_stride, int32_t out_f64, void* scratch, int64_t scratch_bytes, void* stream);
int l3ac_sosfilt_matrix(const double* sos, int32_t sections, double* hi, double* lo, void* stream);
int64_t l3ac_sosfilt_stream_state(int32_t sections);
int l3ac_sosfilt_stream(const double* state_in, double* state_out, int32_t streams, int64_t state_stride, const float* fresh, int64_t fresh_frames,
                        int64_t fresh_stride, const double* sos, int32_t sections, const l3ac_sosfilt_stream_desc* desc, int32_t count, void* out,
                        int64_t out_stride, int32_t out_f64, void* scratch, int64_t scratch_bytes, void* stream);
int64_t l3ac_butter_sos(int32_t order, double cutoff_hz, double sample_rate, int32_t highpass, double* out, int64_t cap);

/* ---- pitch: YIN F0 tracking and the pairwise F0 metrics (which states every formula) ------------------------------
 * A deterministic YIN tracker (de Cheveigne & Kawahara 2002, steps 1-5) of MONO clips.  Parameters: sample_rate fs, fmin, fmax, window W
 * (-1: tau_max), hop (-1: fs / 100), threshold.  tau_min = floor(fs / fmax), tau_max = ceil(fs / fmin), T = tau_max + 1, span = W + T.
 * Supported iff 8000 <= fs <= 192000, 0 < fmin < fmax <= fs / 4, tau_max > tau_min, hop >= 1, W >= 1, 0 < threshold < 1 and span <= 4000
 * (one frame's samples with its d and c rows in 64,000 bytes of LDS).  A clip of n samples has F(n) = 0 frames for n < span, else
 * 1 + (n - span) / hop; frame t reads samples [t hop, t hop + span) and nothing else (no padding, no centring).  The difference function
 * d(tau), tau = 0 .. T, is summed in fp32 in the direct form; the cumulative-mean-normalised c(tau), the pick, the parabolic refinement
 * and f0 = fs / (tau* + shift) are fp64.
 *   l3ac_pitch_lags:          HOST only: out[0..4] = tau_min, tau_max, W, hop, span, the defaults resolved.
 *   l3ac_pitch_frames:        HOST only: F(samples); < 0 for samples < 0 or unsupported parameters.
 *   l3ac_pitch_scratch_bytes: the minimum scratch of l3ac_pitch for these shapes; < 0 for batch outside 1..65535, max_samples outside
 *                             1..2^31 - 1 or unsupported parameters.
 *   l3ac_pitch:               audio [batch][audio_stride] (`samples`: HOST array of batch lengths in 1..max_samples, or NULL) -> f0
 *                             [batch][F(max_samples)] fp64 in Hz, voiced [batch][F(max_samples)] int32 (1: a lag fell below the threshold),
 *                             aperiodicity [batch][F(max_samples)] fp64 = c(tau*); rows at and after a clip's own F hold NaN / 0 / NaN.
 *                             cmnd (or NULL) [batch][F(max_samples)][T + 1] fp64 = c, NaN rows after a clip's own F.  frames (or NULL)
 *                             [batch] int32 = the clips' F.  All outputs are device buffers.
 *   l3ac_pitch_metrics:       two tracks of equal geometry, as written by l3ac_pitch, [batch][max_frames] each (`frames`: HOST array of
 *                             batch frame counts in 0..max_frames, or NULL) -> out [batch][4] fp64 = f0_rmse_cents, gpe, vde, ffe; counts
 *                             [batch][4] int32 = frames, voiced_ref, voiced_est, voiced_both.  A ratio whose denominator is 0 is NaN.
 * Every bad argument is L3AC_EINVAL before any device work, with a message naming it.  Bit guarantee and calling convention: as the
 * quality metrics above (a clip's results do not depend on the batch, its row, the stride, the scratch size or what lies after its
 * length; no atomics; enqueue only, nothing allocated, no synchronisation, capturable).  There is no device table: nothing needs a
 * warm-up before a capture.  Non-finite samples leave the frames that read them unspecified and disturb nothing else. */
int l3ac_pitch_lags(int32_t sample_rate, double fmin, double fmax, int32_t window, int32_t hop, int32_t* out);
int64_t l3ac_pitch_frames(int64_t samples, int32_t sample_rate, double fmin, double fmax, int32_t window, int32_t hop);
int64_t l3ac_pitch_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sample_rate, double fmin, double fmax, int32_t window, int32_t hop);
int l3ac_pitch(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, int32_t sample_rate,
               double fmin, double fmax, int32_t window, int32_t hop, double threshold, double* f0, int32_t* voiced, double* aperiodicity,
               double* cmnd, int32_t* frames, void* scratch, int64_t scratch_bytes, void* stream);
int l3ac_pitch_metrics(const double* f0_ref, const int32_t* voiced_ref, const double* f0_est, const int32_t* voiced_est, int32_t batch,
                       int64_t max_frames, const int32_t* frames, double* out, int32_t* counts, void* stream);

/* ---- time alignment: cross-correlation delay, polarity and shift of clip pairs (which states every formula) ------
 * A pair ref, est of fp32 rows with a common per-clip length n, and a lag range L = max_lag, 0 <= L <= 16384.  For d = -L .. L,
 * r(d) = sum_j ref[j] est[j + d] over the j with 0 <= j < n and 0 <= j + d < n (an empty overlap gives exactly 0): a positive d means the
 * estimate is late by d samples.  r is computed per segment of 4096 samples as a matrix product on the fp32 matrix pipe (an fp32 fmaf
 * chain over 128 terms in a fixed order) and from there in fp64 in a fixed order; the energies E_ref, E_est are fp64 sums of exact
 * squares.  lag d* maximises |r(d)| (ties: the smaller |d|, then the smaller d); polarity = -1 where r(d*) < 0, else +1; correlation =
 * r(d*) / sqrt(E_ref E_est); delay = d* + the vertex of the parabola through s r(d* - 1), s r(d*), s r(d* + 1), s = polarity, where
 * -L < d* < L and the parabola opens downwards, else d*.  E_ref E_est = 0 gives lag 0, polarity 0, delay 0 and correlation NaN.
 *   l3ac_xcorr_scratch_bytes: the minimum scratch of l3ac_xcorr for these shapes, 256 ceil(4 batch / 256) + 8 batch ceil(max_samples / 4096)
 *                             (2 max_lag + 1) bytes; < 0 for batch outside 1..65535, max_samples outside 1..2^31 - 1 or max_lag outside
 *                             0..16384.  With max_lag = 0 it covers l3ac_align_apply, which needs the first term only.
 *   l3ac_xcorr:               ref [batch][ref_stride], est [batch][est_stride] (`samples`: HOST array of batch lengths in 1..max_samples, or
 *                             NULL) -> lag [batch] int32, polarity [batch] int32, delay [batch] fp64, correlation [batch] fp64, and
 *                             xcorr (or NULL) [batch][2 max_lag + 1] fp64 = r(-L) .. r(L).  All outputs are device buffers.
 *   l3ac_align_apply:         lag [batch] int32 is a DEVICE buffer (any values).  With m = max(0, n - |d|): out_ref[j] = ref[j + max(0, -d)]
 *                             and out_est[j] = est[j + max(0, d)] for j < m, exact zeros for m <= j < max_samples; out_samples [batch]
 *                             int32 (device) = m.  The outputs must not overlap the inputs.  polarity is not applied.
 * Every bad argument is L3AC_EINVAL before any device work, with a message naming it.  Bit guarantee and calling convention: as the
 * quality metrics above (a clip's results do not depend on the batch, its row, the stride, the scratch size or what lies after its
 * length; no atomics; enqueue only, nothing allocated, no synchronisation, capturable).  There is no device table: nothing needs a
 * warm-up before a capture.  Non-finite samples inside a clip leave that clip's results unspecified (its lag stays inside [-L, L]) and
 * disturb nothing else. */
int64_t l3ac_xcorr_scratch_bytes(int32_t batch, int64_t max_samples, int32_t max_lag);
int l3ac_xcorr(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples, const int32_t* samples,
               int32_t max_lag, int32_t* lag, int32_t* polarity, double* delay, double* correlation, double* xcorr, void* scratch,
               int64_t scratch_bytes, void* stream);
int l3ac_align_apply(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples,
                     const int32_t* samples, const int32_t* lag, float* out_ref, int64_t out_ref_stride, float* out_est, int64_t out_est_stride,
                     int32_t* out_samples, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- mel-cepstral distortion along a dynamic-time-warping path (which states every formula) -----------------------
 * Cepstra: c[f][q] = sum_m D[q][m] L[f][m], q = 0 .. K = n_coeffs, where L are exactly the fp32 cells of l3ac_log_mel for the same
 * arguments (M = n_mels of them per frame) and D is the orthonormal DCT-II, D[0][m] = sqrt(1 / M), D[q][m] = sqrt(2 / M) cos(pi q (m + 1/2)
 * / M), designed in fp64 with the phase q (2m + 1) mod 4M reduced in integers and rounded once to fp32.  Each c[f][q] is one fp32 fmaf
 * chain over m = 0 .. M - 1 in increasing m from +0.  n_coeffs in 1..min(n_mels - 1, 64); the other parameters as l3ac_log_mel.
 * DTW: a pair of feature sequences a [Fa][dim], b [Fb][dim] (fp32; Fa, Fb in 1..4096, dim in 1..64).  delta(i, j) = sqrt(sum_q (a[i][q] -
 * b[j][q])^2) in fp64 from the fp32 values, difference, square and sum in the order of q, no contraction.  Dacc[0][0] = delta(0, 0),
 * Dacc[i][j] = delta(i, j) + min(Dacc[i-1][j-1], Dacc[i-1][j], Dacc[i][j-1]) over the predecessors inside the matrix, ties to the
 * diagonal, then to (i-1, j), then to (i, j-1): one fp64 addition per cell.  The path is the backtrace of these choices from (Fa-1, Fb-1),
 * reported from (0, 0) forward; its length P lies in max(Fa, Fb) .. Fa + Fb - 1; cost = Dacc[Fa-1][Fb-1], the sequential fp64 sum of
 * delta along the path.  With diagonal_only (every pair's Fa = Fb = F): cost = sum_f delta(f, f) in the order of f, P = F, the path
 * is (f, f).  The mel-cepstral distortion of a pair is 5 sqrt(2) cost / P dB on the cepstra q = 1 .. K (l3ac_amd/mcd.py).
 *   l3ac_dct_table:          HOST only: D as [n_coeffs + 1][n_mels] floats; same protocol as l3ac_mel_weights (returns the float count;
 *                            nothing is written when out is NULL or cap is below it; < 0 for unsupported parameters).
 *   l3ac_mfcc_scratch_bytes: the minimum scratch of l3ac_mfcc: 256 ceil(4 batch / 256) + 256 ceil(4 batch F(max_samples) n_mels / 256) +
 *                            l3ac_mel_scratch_bytes(batch, max_samples, n_fft, hop, n_mels); < 0 for unsupported parameters.
 *   l3ac_mfcc:               l3ac_log_mel's arguments, then `dct` (the DEVICE copy of l3ac_dct_table's output) and n_coeffs -> out
 *                            [batch][F(max_samples)][n_coeffs + 1] fp32 (device); the rows after a clip's own F(n) frames are zero.
 *                            A larger scratch lets log_mel take more frames per product; the bits do not depend on it.
 *   l3ac_dtw_scratch_bytes:  the minimum scratch of l3ac_dtw: 2 * 256 ceil(4 batch / 256) + 256 ceil(batch max_frames_a max_frames_b /
 *                            256) bytes (the two sides' frame counts, one choice byte per cell); < 0 for batch outside 1..65535 or a
 *                            max_frames outside 1..4096.
 *   l3ac_dtw:                a: pair p's frame i at a + p a_row_stride + i a_frame_stride, dim floats; b alike.  The strides count floats
 *                            (a_frame_stride >= dim, a_row_stride >= (max_frames_a - 1) a_frame_stride + dim), so a view that skips
 *                            a leading coefficient needs no copy.  frames_a, frames_b: HOST arrays of batch counts in 1..max_frames_a /
 *                            1..max_frames_b, or NULL (every pair has the maximum).  -> cost [batch] fp64, path_len [batch] int32, path
 *                            (or NULL) [batch][max_frames_a + max_frames_b - 1][2] int32 = (i, j) from (0, 0) forward, -1 after P, and
 *                            delta (or NULL; a test hook) [batch][max_frames_a][max_frames_b] fp64, of which the cells the call
 *                            evaluates are written (all Fa x Fb of a pair, with diagonal_only its diagonal) and nothing else.  All
 *                            outputs are device buffers.  diagonal_only with unequal counts in a pair is L3AC_EINVAL.
 * Every bad argument is L3AC_EINVAL before any device work, with a message naming it.  Bit guarantee and calling convention: as the
 * quality metrics above (a pair's results depend on its own frames only — not on the batch, its row, the strides, the scratch size or
 * what lies at or after its frame counts, which is never read; no atomics; enqueue only, nothing allocated, no synchronisation,
 * capturable).  l3ac_dtw has no device table: nothing needs a warm-up before a capture.  A non-finite feature inside a pair leaves that
 * pair's results unspecified (its path stays inside its matrix) and disturbs nothing else. */
int64_t l3ac_dct_table(int32_t n_mels, int32_t n_coeffs, float* out, int64_t cap);
int64_t l3ac_mfcc_scratch_bytes(int32_t batch, int64_t max_samples, int32_t n_fft, int32_t hop, int32_t n_mels, int32_t n_coeffs);
int l3ac_mfcc(const float* audio, int32_t batch, int64_t max_samples, int64_t audio_stride, const int32_t* samples, int32_t n_fft, int32_t hop,
              const float* basis, const float* weights, int32_t n_mels, const float* dct, int32_t n_coeffs, float* out, void* scratch,
              int64_t scratch_bytes, void* stream);
int64_t l3ac_dtw_scratch_bytes(int32_t batch, int32_t max_frames_a, int32_t max_frames_b);
int l3ac_dtw(const float* a, int64_t a_frame_stride, int64_t a_row_stride, const float* b, int64_t b_frame_stride, int64_t b_row_stride, int32_t batch,
             int32_t dim, int32_t max_frames_a, int32_t max_frames_b, const int32_t* frames_a, const int32_t* frames_b, int32_t diagonal_only,
             double* cost, int32_t* path_len, int32_t* path, double* delta, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- linear prediction and the spectral-envelope measures: LLR, Itakura-Saito, cepstral distance, segmental SNR (DESIGN.md section 3.18,
 * which states every formula and summation order) -------------------------------------------------------------------------------------------
 * Framing: sample_rate in 8000..192000 (it selects nothing but l3ac_lpc_defaults' values), order p in 1..32, frame N in p + 1..8192, hop >=
 * 1.  A clip of n samples has F(n) = 0 frames for n < N, else 1 + (n - N) / hop; frame t reads samples [t hop, t hop + N) and nothing else
 * (no padding, no centring).  xw[i] = (double)x[i] (double)w[i] with w the fp32 window: `window` is the DEVICE copy of l3ac_lpc_window's
 * output, w[i] = 0.5 (1 - cos(2 pi (i + 1) / (N + 1))) designed in fp64 and rounded once, or NULL for the rectangular window.
 * Per frame, all fp64 with contraction off: r[k] = sum_{i=0}^{N-1-k} xw[i] xw[i+k], k = 0..p, as 64 interleaved partial sums (partial l
 * takes the terms i = l mod 64 in increasing i from +0) folded s[l] += s[l+h] for h = 32, 16, .., 1.  Levinson-Durbin: a[0] = 1, E_0 = r[0];
 * for m = 1..p: acc = r[m] + sum_{i=1}^{m-1} a[i] r[m-i] in increasing i, k_m = -acc / E_{m-1}, a'[i] = a[i] + k_m a[m-i], a'[m] = k_m, E_m =
 * E_{m-1} (1 - k_m k_m).  A frame is valid iff r[0] > 0 and every E_m > 0.  q(a, r) = sum_i a[i] (sum_j r[|i-j|] a[j]), both sums from +0 in
 * increasing index.  Cepstrum of 1/A: c_1 = -a_1, c_m = -a_m - sum_{k=1}^{m-1} ((k / m) c_k) a_{m-k}, the sum from +0 in increasing k.
 * For a pair (reference r, estimate e; a frame needs both sides valid): num = q(a_e, r_r), g_r = q(a_r, r_r), g_e = q(a_e, r_e);
 * LLR = ln(num / g_r) clamped to [0, llr_max]; IS = ((g_r / g_e) (num / g_r) + ln(g_e / g_r)) - 1 clamped to [0, is_max]; CD = (10 / ln 10)
 * sqrt(2 sum_{m=1}^{p} (c_r[m] - c_e[m])^2) clamped to [0, cd_max].  Segmental SNR on the same windowed frames: sig = r_r[0], noise =
 * sum (xw_r[i] - xw_e[i])^2 in the autocorrelation's order; 10 log10(sig / noise) clamped to [-10, 35], 35 where noise == 0; a frame
 * counts iff sig > 0.  Per pair: seg_snr_db is the mean of the counted frames' values summed in frame order; for each of LLR, IS, CD the V
 * valid frames' values are sorted ascending, the first k = floor(trim V + 0.5) summed in that order from +0 and divided by k; V = 0 or k = 0
 * gives NaN.  A pair has at most 16384 frames.
 *   l3ac_lpc_window:                HOST only: w as `frame` floats; same protocol as l3ac_mel_weights (returns the float count; nothing is
 *                                   written when out is NULL or cap is below it; < 0 for frame outside 2..8192).
 *   l3ac_lpc_defaults:              HOST only: out[3] = order (10 below 10 kHz, else 16), frame ((30 fs + 500) / 1000), hop (frame / 4).
 *   l3ac_lpc_frames:                HOST only: F(samples); < 0 for samples < 0, frame outside 2..8192 or hop < 1.
 *   l3ac_lpc_scratch_bytes:         the minimum scratch of l3ac_lpc: 256 ceil(4 batch / 256) bytes; < 0 for unsupported parameters.
 *   l3ac_lpc:                       audio [batch] rows of max_samples floats, audio_stride floats apart; samples: HOST array of batch
 *                                   lengths in 1..max_samples, or NULL -> with F = F(max_samples): a [batch][F][p+1], reflection
 *                                   [batch][F][p], error [batch][F] (E_p), autocorr [batch][F][p+1] fp64, valid [batch][F] and frames
 *                                   [batch] (or NULL) int32, all device buffers.  Rows at and after a clip's own F(n) are NaN / 0; an
 *                                   invalid frame has a, reflection and error NaN and keeps its autocorr.
 *   l3ac_lpc_metrics_scratch_bytes: the minimum scratch of l3ac_lpc_metrics: 256 ceil(4 batch / 256) + 256 ceil(32 batch F / 256) + 256
 *                                   ceil(4 batch F / 256) bytes (the lengths, the frames' four values, the frames' flags); < 0 for
 *                                   unsupported parameters or F(max_samples) > 16384.
 *   l3ac_lpc_metrics:               ref, est as audio above; trim in (0, 1]; llr_max, is_max, cd_max finite and >= 0 -> out [batch][4]
 *                                   fp64 = llr, is_distance, cepstral_distance_db, seg_snr_db; counts [batch][3] int32 = frames, valid
 *                                   frames V, frames counted for the SNR; frame_values (or NULL) [batch][F][4] fp64 = the frames' clamped
 *                                   LLR, IS, CD, SNR, NaN where not counted; forms (or NULL; a test hook) [batch][F][5] fp64 = num, g_r, g_e,
 *                                   sig, noise (the first three NaN where a side is invalid).  All device buffers.
 * Every bad argument is L3AC_EINVAL before any device work, with a message naming it.  Bit guarantee and calling convention: as the
 * quality metrics above (a pair's results depend on its own samples only — not on the batch, its row, the strides, the scratch size or
 * what lies at or after its length, which is never read; no atomics; enqueue only, nothing allocated, no synchronisation, capturable).
 * Non-finite samples leave the frames that read them, and their pair's means, unspecified and disturb nothing else. */
int64_t l3ac_lpc_window(int32_t frame, float* out, int64_t cap);
int l3ac_lpc_defaults(int32_t sample_rate, int32_t* out);
int64_t l3ac_lpc_frames(int64_t samples, int32_t frame, int32_t hop);
int64_t l3ac_lpc_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sample_rate, int32_t order, int32_t frame, int32_t hop);
int l3ac_lpc(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, int32_t sample_rate, int32_t order,
             int32_t frame, int32_t hop, const float* window, double* a, double* reflection, double* error, double* autocorr, int32_t* valid,
             int32_t* frames, void* scratch, int64_t scratch_bytes, void* stream);
int64_t l3ac_lpc_metrics_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sample_rate, int32_t order, int32_t frame, int32_t hop);
int l3ac_lpc_metrics(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples,
                     const int32_t* samples, int32_t sample_rate, int32_t order, int32_t frame, int32_t hop, const float* window, double trim,
                     double llr_max, double is_max, double cd_max, double* out, int32_t* counts, double* frame_values, double* forms, void* scratch,
                     int64_t scratch_bytes, void* stream);

/* ---- BSS Eval SDR: the signal-to-distortion ratio after a fitted distortion filter of up to 1024 taps, with its two primitives, the lag
 * correlation of whole clips and the Toeplitz solve (which states every formula and summation order) ------------------
 * A pair: reference s and estimate s^, fp32, n >= 1 samples each; filter length L in 1..1024; diagonal loading load >= 0.  Everything is fp64
 * with contraction off; samples are converted first, so a product of two samples is exact; a sample outside [0, n) is selected away, never
 * multiplied by zero.
 * Correlation: corr(u, v)[k] = sum_{t=0}^{n-1-k} u[t] v[t+k], k = 0..L-1 (+0 for k >= n), as 64 interleaved partial sums (partial l takes the
 * terms t = l mod 64 in increasing t from +0) folded p[l] += p[l+h] for h = 32, 16, .., 1.  r = corr(s, s), b = corr(s, s^), then r[0] =
 * r[0] (1.0 + load), skipped for load == 0.
 * Toeplitz solve of G c = b, G[i][j] = r[|i-j|]: isum over i = i0..i1 is 64 partial sums by (i - i0) mod 64 in increasing i from +0 and the
 * same fold.  a[0] = 1, E_0 = r[0], c[0] = b[0] / r[0]; for m = 1..L-1: acc = r[m] + isum_{i=1}^{m-1} a[i] r[m-i], k_m = -acc / E_{m-1},
 * a'[i] = a[i] + k_m a[m-i] for i = 1..m-1, a'[m] = k_m, E_m = E_{m-1} (1 - k_m k_m); then lambda = b[m] - isum_{i=0}^{m-1} c[i] r[m-i], nu =
 * lambda / E_m, c'[i] = c[i] + nu a'[m-i] for i = 0..m-1, c'[m] = nu.  A pair is valid iff r[0] > 0 and every E_m > 0 (a NaN fails both).
 * Residual: y[t] = sum_{k=0}^{L-1} c[k] s[t-k] from +0 in increasing k over the k with 0 <= t-k < n, t = 0..n+L-2; e[t] = (t < n ? s^[t] :
 * 0) - y[t].  T = sum y^2 and D = sum e^2: the outputs in segments of 4096; in segment q thread i of 256 takes t = 4096 q + i + 256 j, j =
 * 0..15, those below n+L-1, in increasing j from +0; then a xor tree inside each wave of 64 and the four waves' results in wave order; then the
 * segments' sums from +0 in increasing q.  sdr_db = 10 log10(T / D) as IEEE has it: +inf for D == 0 < T, -inf for T == 0 < D, NaN for 0 / 0.
 * With one source BSS Eval's SIR is +inf and its SAR equals the SDR.
 *   l3ac_correlate_scratch_bytes:      the minimum scratch of l3ac_correlate: 256 ceil(4 batch / 256) bytes (the lengths); < 0 for lags
 *                                      outside 1..1024, a bad batch or max_samples, or max_samples + lags - 1 >= 2^31.
 *   l3ac_correlate:                    u, v [batch] rows of max_samples floats, u_stride / v_stride floats apart; samples: HOST array of
 *                                      batch lengths in 1..max_samples, or NULL -> out [batch][lags] fp64 = corr(u, v).
 *   l3ac_toeplitz_solve_scratch_bytes: 256 ceil(4 batch / 256) bytes (the first region of every layout; the solve keeps its state in LDS);
 *                                      < 0 for length outside 1..1024 or batch outside 1..65535.
 *   l3ac_toeplitz_solve:               r, b [batch][length] fp64 -> x [batch][length] fp64 (the c above), error [batch] fp64 = E_{length-1},
 *                                      valid [batch] int32.  An invalid system has x and error NaN.
 *   l3ac_sdr_scratch_bytes:            the minimum scratch of l3ac_sdr: 256 ceil(4 batch / 256) + 256 ceil(16 batch L / 256) + 256 ceil(8
 *                                      batch L / 256) + 256 ceil(16 batch S / 256) bytes, S = ceil((max_samples + L - 1) / 4096) (the
 *                                      lengths, r and b, the filter, the segments' two sums); < 0 as l3ac_correlate_scratch_bytes.
 *   l3ac_sdr:                          ref, est as u, v above; load finite and >= 0 -> out [batch][4] fp64 = sdr_db, T, D, E_{L-1}; valid
 *                                      [batch] int32; filter (or NULL) [batch][L] fp64 = c; corr (or NULL; a test hook) [batch][2][L] fp64 =
 *                                      r, b.  An invalid pair has out and filter NaN and keeps its r and b.
 * All but `samples` are device buffers.  Every bad argument is L3AC_EINVAL before any device work, with a message naming it.  Bit
 * guarantee and calling convention: as the quality metrics above (a pair's results depend on its own samples only — not on the batch, its
 * row, the strides, the scratch size or what lies at or after its length, which is never read; no atomics; enqueue only, nothing allocated,
 * no synchronisation).  No device table: all three are capturable as the first call.  Non-finite samples leave their own pair's results
 * unspecified and disturb nothing else: no address, bound or launch size comes from a sample value. */
int64_t l3ac_correlate_scratch_bytes(int32_t batch, int64_t max_samples, int32_t lags);
int l3ac_correlate(const float* u, int64_t u_stride, const float* v, int64_t v_stride, int32_t batch, int64_t max_samples, const int32_t* samples,
                   int32_t lags, double* out, void* scratch, int64_t scratch_bytes, void* stream);
int64_t l3ac_toeplitz_solve_scratch_bytes(int32_t batch, int32_t length);
int l3ac_toeplitz_solve(const double* r, const double* b, int32_t batch, int32_t length, double* x, double* error, int32_t* valid, void* scratch,
                        int64_t scratch_bytes, void* stream);
int64_t l3ac_sdr_scratch_bytes(int32_t batch, int64_t max_samples, int32_t filter_length);
int l3ac_sdr(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples, const int32_t* samples,
             int32_t filter_length, double load, double* out, int32_t* valid, double* filter, double* corr, void* scratch, int64_t scratch_bytes,
             void* stream);

/* ---- critical-band measures: the spectrum of un-centred frames, frequency-weighted segmental SNR, weighted spectral slope distance, log-
 * spectral distance (which states every formula and summation order) -------------------------------------------------
 * Framing as linear prediction above: frame N in 2..2048, hop >= 1, F(n) = l3ac_lpc_frames(n, N, hop); frame t reads samples [t hop, t hop +
 * N) of its own clip; xw[j] = (double)x[j] (double)w[j] with `window` the DEVICE copy of l3ac_lpc_window's output or NULL for the rectangular
 * window.  n_fft: a power of two in 16..4096, n_fft >= N; h = n_fft / 2.  Everything is fp64 with contraction off.
 * Twiddles T[m] = (cos 2 pi m / n_fft, -sin 2 pi m / n_fft), m = 0..h-1: `twiddles` is the DEVICE copy of l3ac_bands_twiddles' output and part
 * of the definition.  FFT: complex radix-2 decimation in time; z[bitrev(j)] = (xw[j], 0) for j < N, (0, 0) up to n_fft; for spans L = 2, 4, ..,
 * n_fft and j = 0..L/2-1, with w = T[j n_fft / L], a = z[i + j], b = z[i + j + L/2]: t_re = w_re b_re - w_im b_im, t_im = w_re b_im + w_im b_re
 * (four rounded products, one rounded subtraction or addition each), a' = a + t, b' = a - t.  Bins k = 0..h-1 are kept: P[k] = re re + im im,
 * A[k] = sqrt(P[k]) correctly rounded; S = sum_k A[k] as 64 interleaved partial sums (partial l takes k = l mod 64 in increasing k from +0)
 * folded s[l] += s[l+g] for g = 32, 16, .., 1.
 * Band filters: `weights` is the DEVICE copy of l3ac_band_weights' output, [bands][h] fp64, bands in 2..64; a band sum of v is sum_k W[i][k]
 * v[k] over the band's run of non-zero weights in increasing k from +0 (the product rounded, then the sum).
 * fwSegSNR of a frame: m[k] = A[k] / S (normalize = 1) or A[k]; M[i] the band sum of m on each side; d = Mr_i - Me_i, err_i = d d where that is
 * above 2^-52, else 2^-52; w_i = pow(Mr_i, gamma); snr_i = 10 log10((Mr_i Mr_i) / err_i); (sum_i w_i snr_i) / (sum_i w_i), both from +0 in
 * band order, clamped to [-10, 35]; the frame counts iff S > 0 on both sides.
 * WSS of a frame, per side: E[i] = the band sum of P where that is above 1e-10, else 1e-10; e[i] = 10 log10(E[i]); s[i] = e[i+1] - e[i], i =
 * 0..bands-2; "rising at i" is E[i+1] > E[i]; the nearest peak of i: rising: n = i, while n <= bands-2 and rising at n: n++, peak at n;
 * otherwise n = i, while n >= 0 and not rising at n: n--, peak at n + 1; emax = e[first i of the largest E]; W_side[i] = (20 / ((20 + emax)
 * - e[i])) (1 / ((1 + e[peak]) - e[i])).  W[i] = (W_r[i] + W_e[i]) / 2, d = s_r[i] - s_e[i]; the frame value is (sum_i W[i] (d d)) / (sum_i
 * W[i]), both from +0 in band order.
 * LSD of a frame: sqrt((sum_k (10 log10(max(Pr[k], 1e-10)) - 10 log10(max(Pe[k], 1e-10)))^2) / h), the sum as S's.
 * Per pair (at most 16384 frames): fw_seg_snr_db the mean of the counted frames' values summed in frame order, NaN for none; wss: all V = F
 * frames' values sorted ascending, the first k = floor(trim V + 0.5) summed in that order from +0 and divided by k, NaN for V = 0 or k = 0;
 * lsd_db the mean of all frames' values summed in frame order, NaN for none.
 *   l3ac_bands_default_fft:            HOST only: the smallest power of two >= max(2 frame, 16); < 0 for frame outside 2..2048.
 *   l3ac_bands_twiddles:               HOST only: T as n_fft doubles (re, im interleaved); same protocol as l3ac_mel_weights (returns the
 *                                      count; nothing is written when out is NULL or cap is below it).  T[0] = (1, 0), T[n_fft / 4] = (0, -1)
 *                                      exactly; the others are designed in long double on an angle mirrored into [0, pi / 4], rounded once.
 *   l3ac_bands_critical:               HOST only: the default table as 50 doubles: 25 centre frequencies, then 25 bandwidths, in Hz.
 *   l3ac_band_weights:                 HOST only: sample_rate in 8000..192000; centre_hz, bandwidth_hz: `bands` doubles each.  With f0 =
 *                                      centre / (fs / 2) h and bw = bandwidth / (fs / 2) h in fp64: W[i][k] = exp(-11 ((k - floor(f0)) / bw)^2 +
 *                                      ln(min_j bandwidth_j) - ln(bandwidth_i)) in long double, rounded once, and 0 where that is <=
 *                                      exp(-30 / (2 * 2.303)).  Same protocol (bands h doubles).  < 0 for a centre outside [0, fs / 2), a
 *                                      bandwidth that is not positive and finite, or a band without a non-zero weight.
 *   l3ac_frame_spectrum_scratch_bytes: the minimum scratch of l3ac_frame_spectrum and l3ac_band_energies: 256 ceil(4 batch / 256) bytes.
 *   l3ac_frame_spectrum:               audio [batch] rows of max_samples floats, audio_stride floats apart; samples: HOST array of batch
 *                                      lengths in 1..max_samples, or NULL -> with F = F(max_samples): spectrum [batch][F][h][2] fp64 (re, im);
 *                                      power, magnitude (or NULL) [batch][F][h] fp64 = P, A; magnitude_sum (or NULL) [batch][F] fp64 = S;
 *                                      frames (or NULL) [batch] int32.  Rows at and after a clip's own F(n) are NaN.
 *   l3ac_band_energies:                -> power, magnitude [batch][F][bands] fp64: the band sums of P (before the floor) and of A.
 *   l3ac_band_metrics_scratch_bytes:   the minimum scratch of l3ac_band_metrics: 256 ceil(4 batch / 256) + 256 ceil(24 batch F / 256) + 256
 *                                      ceil(4 batch F / 256) bytes (the lengths, the frames' three values, the frames' flags); < 0 for
 *                                      unsupported parameters or F(max_samples) > 16384.
 *   l3ac_band_metrics:                 ref, est as audio above; gamma finite, normalize 0 or 1, trim in (0, 1] -> out [batch][3] fp64 =
 *                                      fw_seg_snr_db, wss, lsd_db; counts [batch][2] int32 = frames, frames counted for the fwSegSNR;
 *                                      frame_values (or NULL) [batch][F][3] fp64, the fwSegSNR NaN where not counted; and the test hooks (or
 *                                      NULL): magnitude_sum [batch][F][2] = S of ref, est; band_power, band_magnitude [batch][F][2][bands]
 *                                      = the band sums of P (before the floor) and of m; peaks [batch][F][2][bands] int32 = the nearest
 *                                      peak's band of i = 0..bands-2, then the first band of the largest E.
 * All but `samples` are device buffers.  Every bad argument is L3AC_EINVAL before any device work, with a message naming it.  Bit guarantee
 * and calling convention: as the quality metrics above (a pair's results depend on its own samples only — not on the batch, its row, the
 * strides, the scratch size or what lies at or after its length, which is never read; no atomics; enqueue only, nothing allocated, no
 * synchronisation, capturable).  Non-finite samples leave the frames that read them, and their pair's means, unspecified and disturb
 * nothing else: no address, bound or loop count comes from a sample value. */
int32_t l3ac_bands_default_fft(int32_t frame);
int64_t l3ac_bands_twiddles(int32_t n_fft, double* out, int64_t cap);
int64_t l3ac_bands_critical(double* out, int64_t cap);
int64_t l3ac_band_weights(int32_t sample_rate, int32_t n_fft, int32_t bands, const double* centre_hz, const double* bandwidth_hz, double* out,
                          int64_t cap);
int64_t l3ac_frame_spectrum_scratch_bytes(int32_t batch, int64_t max_samples, int32_t frame, int32_t hop, int32_t n_fft);
int l3ac_frame_spectrum(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, int32_t frame,
                        int32_t hop, int32_t n_fft, const float* window, const double* twiddles, double* spectrum, double* power, double* magnitude,
                        double* magnitude_sum, int32_t* frames, void* scratch, int64_t scratch_bytes, void* stream);
int l3ac_band_energies(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, int32_t frame,
                       int32_t hop, int32_t n_fft, const float* window, const double* twiddles, const double* weights, int32_t bands, double* power,
                       double* magnitude, int32_t* frames, void* scratch, int64_t scratch_bytes, void* stream);
int64_t l3ac_band_metrics_scratch_bytes(int32_t batch, int64_t max_samples, int32_t frame, int32_t hop, int32_t n_fft, int32_t bands);
int l3ac_band_metrics(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples,
                      const int32_t* samples, int32_t frame, int32_t hop, int32_t n_fft, const float* window, const double* twiddles,
                      const double* weights, int32_t bands, double gamma, int32_t normalize, double trim, double* out, int32_t* counts,
                      double* frame_values, double* magnitude_sum, double* band_power, double* band_magnitude, int32_t* peaks, void* scratch,
                      int64_t scratch_bytes, void* stream);

/* ---- coherence: the magnitude-squared coherence per level class and the coherence speech intelligibility index CSII with its three-level
 * form I3 (Kates & Arehart 2005; DESIGN.md section 3.23, which states every formula and summation order) ------------------------------------
 * Framing, window, twiddles, transform and band filters as the critical-band measures above (frame N in 2..2048, hop >= 1, n_fft a power of
 * two in 16..4096 and >= N, all of them supported here; h = n_fft / 2; X, Y the kept bins of the reference's and the estimate's frame).
 * Everything is fp64 with contraction off.  A pair may have at most 16384 frames.
 * Level classes, decided on the reference: E_t = sum_j xw[j]^2 as 64 interleaved partials (partial l takes j = l mod 64 in increasing j from
 * +0) folded s[l] += s[l+g], g = 32..1; S = sum_t E_t the same way over t; M = S / F; class 0: E_t >= M, 1: E_t >= 0.1 M, 2: E_t >= 0.001 M,
 * 3: otherwise (each product rounded once); S == 0: every frame in class 3.
 * Sums per class c and bin k over the class's frames: Sxx = sum (Xr Xr + Xi Xi), Syy likewise, Sxy_re = sum (Xr Yr + Xi Yi), Sxy_im = sum (Xi
 * Yr - Xr Yi).  Order: a chunk is 4 G consecutive frames, G = 16 for n_fft <= 256, 8 up to 1024, 4 at 2048, 2 at 4096; the frames of a chunk
 * in increasing t from +0, then the chunks in increasing order from +0.  "All frames" = ((c0 + c1) + (c2 + c3)) per value.
 * g = min((Sxy_re^2 + Sxy_im^2) / (Sxx Syy), 1), 0 where Sxx Syy == 0.  msc and msc_levels hold NaN where the count is below 2.
 * Bands: N_i = sum_k W[i][k] (g_k Syy_k), D_i = sum_k W[i][k] ((1 - g_k) Syy_k) over the band's run of non-zero weights in increasing k from
 * +0; T_i = 0 if N_i == 0, 1 if D_i == 0 and N_i > 0, else (clamp(10 log10(N_i / D_i), -15, 15) + 15) / 30; the value of a row is (sum_i I_i
 * T_i) / (sum_i I_i), both from +0 in band order, NaN where the row's frame count is below 2.  i3 = (-3.47 + 1.84 low) + 9.99 mid;
 * intelligibility = 1 / (1 + exp(-i3)).
 *   l3ac_sii_bands:               HOST only: the critical-band table of ANSI S3.5-1997 as 63 doubles: 21 centre frequencies, 21 bandwidths
 *                                 (upper - lower edge), 21 importances; protocol of l3ac_bands_critical.
 *   l3ac_coherence_scratch_bytes: the minimum scratch of l3ac_coherence and l3ac_csii, each term rounded up to 256: 4 batch + 8 batch F + 4
 *                                 batch F + 20 batch + 128 batch h + 128 batch ceil(F / (4 G)) h bytes, F = F(max_samples); < 0 for
 *                                 unsupported parameters or F > 16384.
 *   l3ac_coherence:               ref, est, samples, window, twiddles as l3ac_band_metrics -> every output or NULL: msc [batch][h] over all
 *                                 frames; msc_levels [batch][4][h]; sums [batch][4][4][h] = per class Sxx, Syy, Sxy_re, Sxy_im; counts
 *                                 [batch][5] int32 = frames, then the frames of classes 0..3; frame_class [batch][F] int32, -1 at and after a
 *                                 clip's own frames; frame_energy [batch][F] fp64, NaN there.
 *   l3ac_csii:                    weights [bands][h] and importance [bands] (finite, positive) DEVICE tables, bands in 2..64 -> out
 *                                 [batch][6] fp64 = csii (all frames), csii_high, csii_mid, csii_low (classes 0, 1, 2), i3, intelligibility;
 *                                 counts as above; band_signal, band_distortion, band_value [batch][4][bands] = N, D, T of classes 0, 1, 2
 *                                 and, in row 3, of all frames (computed whatever the counts); sums as above; all but out may be NULL.
 * Bit guarantee, calling convention and non-finite samples as the critical-band measures above; fp64 buffers 8-byte aligned. */
int64_t l3ac_sii_bands(double* out, int64_t cap);
int64_t l3ac_coherence_scratch_bytes(int32_t batch, int64_t max_samples, int32_t frame, int32_t hop, int32_t n_fft);
int l3ac_coherence(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples,
                   const int32_t* samples, int32_t frame, int32_t hop, int32_t n_fft, const float* window, const double* twiddles, double* msc,
                   double* msc_levels, double* sums, int32_t* counts, int32_t* frame_class, double* frame_energy, void* scratch,
                   int64_t scratch_bytes, void* stream);
int l3ac_csii(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples, const int32_t* samples,
              int32_t frame, int32_t hop, int32_t n_fft, const float* window, const double* twiddles, const double* weights,
              const double* importance, int32_t bands, double* out, int32_t* counts, double* band_signal, double* band_distortion,
              double* band_value, double* sums, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- streaming token wire format: ragged packing and byte sessions -------------------------------------
 * The format of the rectangular calls above, stated per byte: token t of a stream occupies bits [t*bits, (t+1)*bits) of a little-endian bit
 * stream, byte k of the stream is bits [8k, 8k+8), and a stream of n tokens is ceil(n*bits/8) bytes, its last byte zero-padded: exactly the
 * first ceil(n*bits/8) bytes of the row that the rectangular pack call writes for the same tokens (the rest of that row is zero).  Bits of an
 * index above `bits` are dropped.  bits in 1..32.
 * S live streams are packed / unpacked push by push; a stream's carried state is ONE uint32 in its slot of a state buffer [streams]:
 *   packing:    the `held` bits (0..7, the low bits of state_in[slot]) that have not filled a byte yet.  The stream's input is the virtual bit
 *               string  held bits ++ `take` tokens from the front of fresh[slot] (int32 [streams][fresh_stride]),  T = held + take*bits bits.
 *               not ended: count = T div 8 bytes, keep = T mod 8;     ended: count = ceil(T / 8), keep = 0 and the slot is fresh.
 *   unpacking:  the `held` bits (0..bits-1) that have not completed a token yet, followed by `take` bytes from the front of fresh[slot]
 *               (uint8 [streams][fresh_stride], any byte alignment), T = held + 8*take bits.
 *               not ended: count = T div bits tokens, keep = T mod bits;     ended: keep = 0, the slot is fresh, and count tokens are emitted
 *               with 0 <= T - count*bits < max(bits, 8): the bits dropped are a stream's byte padding (for bits >= 8: count = T div bits).
 * Neither the tokens nor the bytes a stream has seen reach the device: nothing in a descriptor grows with the age of a stream.
 *   l3ac_packed_bytes:   HOST only: ceil(n_tok*bits/8), or < 0 for n_tok < 0 or bits outside 1..32.
 *   l3ac_pack_stream:    ONE launch per 160 descriptors: out[slot][0 : count] (uint8 [streams][out_stride], out_stride a multiple of 4, rows
 *                        4-byte aligned) = the first count bytes of the virtual bit string, zeros from there to out_bytes (<= out_stride; every
 *                        byte below out_bytes of a described stream's row is written once, rows without a descriptor are not touched), and
 *                        state_out[slot] = the string's last `keep` bits.  Tokens at or after `take` are never read.
 *   l3ac_unpack_stream:  the mirror: out[slot][0 : count] (int32 [streams][out_stride]) = the tokens, zeros from there to out_tokens, and
 *                        state_out[slot] = the last `keep` bits.  Bytes at or after `take` are never read.
 * state_in and state_out are two buffers that must not overlap (a session alternates them; describe idle streams too, with take = 0 and
 * keep = held, so that their state follows).  They may be null when every held and keep is 0, fresh when no descriptor takes any, out when
 * the output size is 0.  `desc` is a HOST array with at most one descriptor per stream, checked before anything is launched (stream in range,
 * held in range, take within the packet, count within the output row, count and keep one of the two forms above) and handed to the device
 * as kernel arguments: graph-safe as far as the entry goes.  Integer and byte work, exact by construction.  Enqueue only. */
typedef struct l3ac_pack_stream_desc {
    int32_t slot;    /* stream: row of the new tokens and of the output, element of the state buffers */
    int32_t held;    /* pending bits in state_in[slot]: 0..7 */
    int32_t take;    /* new tokens, from the front of the stream's row of `fresh` */
    int32_t count;   /* bytes this push emits */
    int32_t keep;    /* pending bits afterwards, written to state_out[slot] */
} l3ac_pack_stream_desc;
typedef struct l3ac_unpack_stream_desc {
    int32_t slot;    /* stream: row of the new bytes and of the output, element of the state buffers */
    int32_t held;    /* pending bits in state_in[slot]: 0..bits-1 */
    int32_t take;    /* new bytes, from the front of the stream's row of `fresh` */
    int32_t count;   /* tokens this push emits */
    int32_t keep;    /* pending bits afterwards, written to state_out[slot] */
} l3ac_unpack_stream_desc;
int64_t l3ac_packed_bytes(int64_t n_tok, int32_t bits);
int l3ac_pack_stream(const uint32_t* state_in, uint32_t* state_out, int32_t streams, const int32_t* fresh, int64_t fresh_tokens,
                     int64_t fresh_stride, int32_t bits, const l3ac_pack_stream_desc* desc, int32_t count, uint8_t* out, int64_t out_bytes,
                     int64_t out_stride, void* stream);
int l3ac_unpack_stream(const uint32_t* state_in, uint32_t* state_out, int32_t streams, const uint8_t* fresh, int64_t fresh_bytes,
                       int64_t fresh_stride, int32_t bits, const l3ac_unpack_stream_desc* desc, int32_t count, int32_t* out, int64_t out_tokens,
                       int64_t out_stride, void* stream);

/* ---- single blocks of a context's network, for per-kernel parity tests ------------------------------ */
/* `block` is the reference state-dict prefix of the block inside its module file, e.g. "encoder.blocks.1.0.module".
 * Shapes: x / y are [batch][frames][channels] frame-major.
 *
 * Size limits (DESIGN.md section 3.20.1 lists every 32-bit quantity of the codec kernels with its bound).  A tensor may hold 2^31
 * elements and more: row, clip and byte offsets are 64-bit, and the row kernels switch to a 64-bit instantiation.  What is bounded, for
 * these entries and for l3ac_encode / l3ac_decode alike — a call past a limit is refused with L3AC_EINVAL before any launch, and by
 * these entries before the context's workspace is sized for it:
 *   batch <= 65535 (grid dimension of the per-clip kernels);
 *   frames <= L3AC_MAX_CLIP_FRAMES (frame numbers inside a clip are 32-bit, with a tile and a halo added) and batch * frames <
 *     L3AC_MAX_ROWS (tile numbers are 32-bit; the kernels' own launchers ask tiles < 2^31 - 65536);
 *   rows = batch * frames < 2^31 wherever a convolution is evaluated as a GEMM (conv_k3, the unfused LegacyUnit, the gated up conv);
 *   conv_unit_ring_kernel (C = 48 by default, C = 24 under "narrow_ring" = 2): frames * C < L3AC_MAX_RING_CLIP_ELEMS — it keeps
 *     offsets INSIDE a clip in 32 bits;
 *   an up layer in either form (the row kernel's linear upsampling, up_fused_kernel): frames * scale <= L3AC_MAX_LERP_FRAMES_OUT —
 *     the source position is computed in fp32 as ATen does; past 2^23 output frames per clip it is no longer within half a frame of
 *     the exact one: the row kernel can then read the row after the clip's last, the fused kernel take the wrong neighbour frame. */
#define L3AC_MAX_CLIP_FRAMES 2147418112      /* 2^31 - 65536 */
#define L3AC_MAX_ROWS 17179869184LL          /* 2^34 */
#define L3AC_MAX_RING_CLIP_ELEMS 536870912   /* 2^29 */
#define L3AC_MAX_LERP_FRAMES_OUT 8388608     /* 2^23 */
int l3ac_op_first_block(l3ac_ctx* ctx, const float* audio, int32_t batch, int32_t samples, float* y, void* stream);
/* The stem as l3ac_encode runs it: audio [batch] rows of `samples` valid floats, `audio_stride` floats apart (>= samples; what lies
 * between the rows is not read), -> y [batch][frames][d0] with frames >= samples > 0: frames samples .. frames - 1 are the zero
 * right-padding of Codec.preprocess (codec.py:79-84), folded into the load.  Anything else is refused (L3AC_EINVAL) before a launch.
 * l3ac_op_first_block(audio, batch, samples) = l3ac_op_first_block_at(audio, batch, samples, samples, samples). */
int l3ac_op_first_block_at(l3ac_ctx* ctx, const float* audio, int32_t batch, int32_t samples, int64_t audio_stride, int32_t frames,
                           float* y, void* stream);
int l3ac_op_conv_unit(l3ac_ctx* ctx, const char* block, const float* x, int32_t batch, int32_t frames, float* y,
                      void* stream);
int l3ac_op_down_layer(l3ac_ctx* ctx, const char* block, const float* x, int32_t batch, int32_t frames, float* y,
                       void* stream);
int l3ac_op_conv_k3(l3ac_ctx* ctx, const char* block, const float* x, int32_t batch, int32_t frames, float* y,
                    void* stream);
int l3ac_op_enhance(l3ac_ctx* ctx, const char* block, const float* x, int32_t batch, int32_t frames, float* y,
                    void* stream);
int l3ac_op_up_layer(l3ac_ctx* ctx, const char* block, const float* x, int32_t batch, int32_t frames, float* y,
                     void* stream);
/* EnhanceBlock + up layer as the decoder pipeline runs them (the gate is applied to the 1x1 conv's A operand while it is
 * staged, tconv/__init__.py:35-44 + modules.py:160-164): y [batch][frames * scale][cout] */
int l3ac_op_enhance_up(l3ac_ctx* ctx, const char* enhance_block, const char* up_block, const float* x, int32_t batch,
                       int32_t frames, float* y, void* stream);
int l3ac_op_last_block(l3ac_ctx* ctx, const float* x, int32_t batch, int32_t frames, float* audio, void* stream);
/* The output stage's parts as l3ac_op_last_block runs them: LegacyUnit `unit` (0, 1, 2 = dilation 1, 3, 9: modules.py order),
 * x -> y [batch][frames][c] (x must not alias y); the head, x [batch][frames][c] -> audio [batch][frames] (honours
 * l3ac_ctx_set_head_pretanh).  l3ac_op_last_block(x) = op_head(op_legacy_unit(2, op_legacy_unit(1, op_legacy_unit(0, x)))). */
int l3ac_op_legacy_unit(l3ac_ctx* ctx, int32_t unit, const float* x, int32_t batch, int32_t frames, float* y, void* stream);
int l3ac_op_head(l3ac_ctx* ctx, const float* x, int32_t batch, int32_t frames, float* audio, void* stream);
int l3ac_op_local_trans(l3ac_ctx* ctx, const char* block, const float* x, int32_t batch, int32_t frames, float* y,
                        void* stream);
/* whole sub-modules */
int l3ac_op_encoder(l3ac_ctx* ctx, const float* audio, int32_t batch, int32_t samples, float* feature, void* stream);
int l3ac_op_en_encoder(l3ac_ctx* ctx, const float* feature, int32_t batch, int32_t frames, float* tokens, void* stream);
int l3ac_op_en_decoder(l3ac_ctx* ctx, const float* tokens, int32_t batch, int32_t n_tok, float* feature, void* stream);
int l3ac_op_decoder(l3ac_ctx* ctx, const float* feature, int32_t batch, int32_t frames, float* audio, void* stream);

/* snake activation on its own (layers.py:29-33): y = x + (alpha + 1e-8)^-1 * sin(alpha * x)^2 for x [rows][c], alpha [c]
 * (device pointers).  mode bit 0: evaluate the two-elements-per-lane form the GEMM epilogues and the fused units use;
 * mode bit 1: y = sin(x)^2 alone (the kernels' own sine; alpha is not used); mode 4: y = gelu(x), the exact (erf) GELU as the
 * kernels evaluate it (tconv/__init__.py:13, the transformer's GEGLU; alpha is not used).
 * A test entry (it synchronises and allocates): the pipeline applies snake inside its GEMM / unit kernels. */
int l3ac_op_snake(const float* x, float* y, int64_t rows, int32_t c, const float* alpha, int32_t mode, void* stream);
/* Validation switch of ONE context: while enabled its output head (modules.py:192-194) stores the Conv1d(c -> 1, k7) result
 * BEFORE the final tanh, so that decoder parity can be checked where tanh's saturation does not hide it.  Like every
 * call on a context, not to be issued while another thread uses (or captures a graph on) the same context. */
int l3ac_ctx_set_head_pretanh(l3ac_ctx* ctx, int32_t enable);

/* ---- per-launch profile (measurement aid; reference has no counterpart) -------------------------------
 * Between l3ac_profile_begin() and l3ac_profile_end() every kernel launched by the calling thread is bracketed
 * by HIP events on its own stream.  l3ac_profile_end() synchronises, aggregates per kernel name (launch count,
 * summed device time, summed algorithmic FLOPs and bytes) and writes at most `cap` entries. */
typedef struct l3ac_profile_entry {
    char name[64];
    int32_t launches;
    int32_t reserved;
    double ms_total;
    double flops;   /* algorithmic floating-point operations of those launches */
    double bytes;   /* algorithmic HBM bytes of those launches */
} l3ac_profile_entry;
int l3ac_profile_begin(void);
int l3ac_profile_end(l3ac_profile_entry* out, int32_t cap, int32_t* n_out);

/* Generic fp32 MFMA GEMM used by every channel contraction: c[m][n] = a[m][:] . w[n][:] + bias[n].
 * a [m][k] (row stride lda), w [n][k], k % 4 == 0.  Exported for the kernel micro-benchmark and tests. */
int l3ac_gemm_f32(const float* a, int64_t lda, const float* w, const float* bias, float* c, int64_t ldc,
                  int64_t m, int32_t n, int32_t k, void* stream);

/* ---- fp32 products on the bf16 matrix cores ("bf16x3" operand splitting; kernels/gemm_split.hip) -----------------
 * Every fp32 operand is split exactly into three bf16 planes (3 x 8 significant bits = the 24-bit significand) and the
 * product is the six plane products of order <= 2, accumulated in fp32: error vs fp64 no larger than the fp32 fmaf
 * chain's (tests/test_gpu_blocks.py::test_gemm_split_accuracy), at 2.67x fewer matrix-core cycles.  The network's large
 * channel contractions use it by default.  The route is a property of the CONTEXT: l3ac_ctx_set_gemm_split(ctx, 0)
 * routes every later product of that context through the exact v_mfma_f32_32x32x2_f32 kernel instead (option "gemm_split"
 * below: a context starts on the split route unless L3AC_GEMM_SPLIT=0 is in the environment when it is created); other contexts,
 * and graphs already captured from this one, are not affected.
 * (reference counterpart: none — torch.nn.functional.linear / conv1d on fp32 tensors.) */
/* The split itself, on the HOST (no GPU needed; this is what builds the weight images): planes [3][n] bf16 bit patterns with
 * x[i] == bf16(planes[0][i]) + bf16(planes[1][i]) + bf16(planes[2][i]) exactly for every finite fp32 x[i]
 * (tests/test_host.py::test_bf16x3_split_is_exact). */
void l3ac_split3_host(const float* x, int64_t n, uint16_t* planes);
int l3ac_ctx_set_gemm_split(l3ac_ctx* ctx, int32_t enable);
/* Route options of ONE context by name.  Every option has a default; where an environment variable is named, its value (read with
 * atoi when the context is CREATED) replaces the default.  Both the environment and l3ac_ctx_set_option go through one rule: a 0/1
 * switch takes value != 0, any other option is clamped into its range; a retired value is refused with L3AC_EINVAL.
 * "gemm_split" (default 1, L3AC_GEMM_SPLIT) and "head_pretanh" (default 0): the setters above.  "narrow_ring" (0..2) — which
 * fused kernel takes the ConvUnits with C <= 48 on the split route: 0 = conv_unit_split_kernel (32 frames per wave) everywhere,
 * 1 (default) = conv_unit_ring_kernel (16 frames per wave, weights resident in / streamed through LDS) at the width where it is the
 * faster one (C = 48), 2 = wherever it exists (C = 24 too).  Both evaluate the same operations; their results agree to rounding.
 * "trans_coop" (default 1, L3AC_TRANS_COOP): batches of at most 32 clips — a streaming chunk is one — run every LocalTrans stack in the
 * cooperative form of trans_stack_kernel (six co-resident workgroups per clip exchanging partial tiles through global memory); 0 keeps one
 * workgroup per clip.  Both forms return the same bits.  The cooperative form's six workgroups per clip wait for each other: they need
 * six CUs per clip (claimed per context in a process-wide registry; a launch that does not fit runs in the one-workgroup form);
 * failure reporting: l3ac_coop_timeout_count above.  "coop_timeout_ms" (default 250, 1..20000): the time limit of an arrival poll.
 * "coop_release_claim" (any value): returns the CUs this context has claimed for cooperative launches to the per-device registry (a claim
 * otherwise only grows until the context is destroyed); not while a graph captured from the context may still replay a cooperative launch.
 * "coop_test_fault" (test hook, default 0): j + 1 makes workgroup j of every clip withhold its first arrival.
 * "down_fused" (default 2, L3AC_DOWN_FUSED, 0..2): the encoder down layers 24 -> 48 and 48 -> 96 (Conv1d(k = stride) + ChannelNorm) in one
 * kernel instead of an fp32-MFMA GEMM + row kernel.  2: down_exact_kernel — the arithmetic of those two kernels bit for bit, on both GEMM
 * routes; 0: the two kernels.  1 was retired and is refused.
 * "gemm_w256" (default 1, L3AC_GEMM_W256, 0..2): which bf16x3 batch products take the 256-column kernel gemm_split_kernel_w256: 0 none,
 * 1 the long-K light-epilogue ones, 2 every eligible shape.  The same bits either way.
 * "unit_chunk_mb" (default 192, L3AC_UNIT_CHUNK_MB, 0..65536): the C = 512 ConvUnits (GEMM form) run over groups of clips whose hidden
 * tensor is about this many MB (0: the whole batch at once).  The same bits either way.
 * "wide_sliced" (default 1, 0..2): the wide ConvUnits (C = 96 .. 256) of few frames — up to 256 tiles of 16, a streaming chunk — as two
 * launches over frame tiles x channel slices instead of the fused kernel whose waves own their frames end to end; 0 never, 2 wherever
 * the form exists.  The same bits either way.
 * "unit_counter" (default 1, L3AC_UNIT_COUNTER, 0..3): batch kernels that keep two workgroups per CU resident (the C = 96 ConvUnits,
 * the LegacyUnits) hand their units of work out by a device counter instead of equal static shares (the workgroup dispatched first is
 * served first by every SIMD and would finish its share early); 0: static shares; 2 / 3 (measurement): only the ConvUnits / only the
 * LegacyUnits.  Which workgroup computes a tile does not enter its arithmetic: the same bits either way.
 * Unknown names return L3AC_EINVAL.  l3ac_ctx_get_option writes the value an option holds now (all but coop_release_claim and
 * coop_test_fault). */
int l3ac_ctx_set_option(l3ac_ctx* ctx, const char* name, int32_t value);
int l3ac_ctx_get_option(const l3ac_ctx* ctx, const char* name, int32_t* out);
int32_t l3ac_ctx_get_gemm_split(const l3ac_ctx* ctx);
/* Weight image for l3ac_gemm_split_f32: w [n][k] fp32 -> `image` (device, l3ac_gemm_split_image_bytes(n, k) bytes;
 * 0 = shape not eligible: needs n >= 192, k >= 32, k % 8 == 0). */
int64_t l3ac_gemm_split_image_bytes(int32_t n, int32_t k);
int l3ac_gemm_split_image(const float* w, int32_t n, int32_t k, void* image, void* stream);
/* c[m][n] = a[m][:] . w[n][:] + bias[n] with w given as its split image (a [m][k] fp32, row stride lda); the 256-column kernel takes
 * the products option "gemm_w256" of a new context would send there.  _at: that choice given as w256 (0..2; test entry). */
int l3ac_gemm_split_f32(const float* a, int64_t lda, const void* image, const float* bias, float* c, int64_t ldc,
                        int64_t m, int32_t n, int32_t k, void* stream);
int l3ac_gemm_split_f32_at(const float* a, int64_t lda, const void* image, const float* bias, float* c, int64_t ldc,
                           int64_t m, int32_t n, int32_t k, int32_t w256, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* L3AC_HIP_H */
