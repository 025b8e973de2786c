// Long recordings as chunk rows (l3ac_chunk_plan / l3ac_chunk_cut / l3ac_chunk_merge).
//
// A recording of n frames is cut the way the reference's ChunkData cuts it (l3ac/codec.py:159-188): chunk j covers frames
// [j * chunk_len - (j ? prefix_len : 0), min(n, (j + 1) * chunk_len)).  The chunks of a whole batch of recordings become the rows of
// ONE ragged call (section 3.7); these kernels move the data between the two layouts:
//   chunk_cut_kernel     recordings [B][stride][c] -> chunk rows [N][row_frames][c]; the frames a recording gains when its length is
//                        rounded up (audio: to a hop multiple, Network.preprocess) are written as zeros
//   chunk_merge_kernel   chunk rows -> recordings [B][stride][c]: every chunk but a recording's first drops its prefix; the last chunk
//                        of a recording also zeroes the recording's row from its end to out_frames
// Elements are 4 bytes and are moved as integers: int32 tokens and fp32 samples / features share the kernels, no floating-point
// instruction touches them.  c = 1 for samples and tokens, c = feature_dim or n_levels for per-token vectors.
//
// Access width.  Chunk starts are multiples of the hop (270 samples at 1kbps) and prefixes are dropped, so source and destination of a
// span are in general only 4-byte aligned RELATIVE to each other.  Where they are 16 bytes apart modulo 16 (always when c % 4 == 0
// and the row strides are multiples of 4 elements) a span is a scalar head up to the destination's next 16-byte boundary, a body of
// 16-byte loads and stores, and a scalar tail; otherwise every lane moves one dword per step, which is still one fully coalesced
// 256-byte access per wave.  The choice is uniform over a workgroup (one chunk per blockIdx.y).
//
// The chunk descriptors are host values and reach the device as KERNEL ARGUMENTS, ChunkBlock::CAP per launch (the way RaggedUpload
// carries the lengths of a ragged call): the caller's array may change after the call, a captured graph replays what it captured,
// and no workspace or staging buffer is involved.
#include <algorithm>

#include "../kernels.hpp"
#include "span_copy.hpp"

namespace {

constexpr int THREADS = SPAN_THREADS;

// grid (span blocks, chunks of this block of descriptors)
__global__ __launch_bounds__(THREADS) void chunk_cut_kernel(const uint32_t* __restrict__ src, int64_t src_stride, int c,
                                                           uint32_t* __restrict__ dst, int64_t dst_row_frames, const ChunkBlock blk) {
    const l3ac_chunk_desc d = blk.desc[blockIdx.y];
    const int64_t tid = (int64_t)blockIdx.x * THREADS + threadIdx.x, stride = (int64_t)gridDim.x * THREADS;
    const int64_t own = (int64_t)(d.frames - d.pad) * c;
    uint32_t* row = dst + (int64_t)d.row * dst_row_frames * c;
    copy_span(row, src + ((int64_t)d.rec * src_stride + d.start) * c, own, tid, stride);
    if (d.pad > 0) zero_span(row + own, (int64_t)d.pad * c, tid, stride);
}

__global__ __launch_bounds__(THREADS) void chunk_merge_kernel(const uint32_t* __restrict__ src, int64_t src_row_frames, int c,
                                                             uint32_t* __restrict__ dst, int64_t dst_stride, int64_t out_frames,
                                                             const ChunkBlock blk) {
    const l3ac_chunk_desc d = blk.desc[blockIdx.y];
    const int64_t tid = (int64_t)blockIdx.x * THREADS + threadIdx.x, stride = (int64_t)gridDim.x * THREADS;
    uint32_t* rec = dst + (int64_t)d.rec * dst_stride * c;
    copy_span(rec + (d.start + d.prefix) * c, src + ((int64_t)d.row * src_row_frames + d.prefix) * c, (int64_t)(d.frames - d.prefix) * c,
              tid, stride);
    const int64_t end = d.start + d.frames;
    if (d.last && end < out_frames) zero_span(rec + end * c, (out_frames - end) * c, tid, stride);
}

int check_descs(const char* who, const l3ac_chunk_desc* desc, int count, int recs, int64_t rec_frames, int rows, int64_t row_frames) {
    L3AC_REQUIRE(desc && count > 0, "%s: no descriptors", who);
    for (int i = 0; i < count; ++i) {
        const l3ac_chunk_desc& d = desc[i];
        L3AC_REQUIRE(d.rec >= 0 && d.rec < recs && d.row >= 0 && d.row < rows, "%s: descriptor %d: recording %d of %d, row %d of %d", who,
                     i, d.rec, recs, d.row, rows);
        L3AC_REQUIRE(d.start >= 0 && d.frames >= 1 && d.frames <= row_frames && d.prefix >= 0 && d.prefix < d.frames && d.pad >= 0 &&
                         d.pad <= d.frames,
                     "%s: descriptor %d: start %lld, %d frames (prefix %d, zero tail %d) for rows of %lld frames", who, i,
                     (long long)d.start, d.frames, d.prefix, d.pad, (long long)row_frames);
        L3AC_REQUIRE(d.start + d.frames <= rec_frames, "%s: descriptor %d ends at frame %lld of a recording row of %lld", who, i,
                     (long long)(d.start + d.frames), (long long)rec_frames);
    }
    return L3AC_OK;
}

}  // namespace

extern "C" {

int64_t l3ac_chunk_plan(const int64_t* frames, int32_t batch, int64_t chunk_len, int64_t prefix_len, int32_t round_to,
                        l3ac_chunk_desc* desc_out, int64_t cap) {
    L3AC_REQUIRE(frames && batch > 0, "chunk_plan: no recordings");
    L3AC_REQUIRE(prefix_len >= 0 && chunk_len > prefix_len, "chunk_plan: chunk_len (%lld) must exceed prefix_len (%lld >= 0)",
                 (long long)chunk_len, (long long)prefix_len);
    L3AC_REQUIRE(round_to >= 1, "chunk_plan: round_to = %d", round_to);
    L3AC_REQUIRE(chunk_len + prefix_len <= INT32_MAX - round_to, "chunk_plan: a chunk row of %lld frames does not fit 32 bits",
                 (long long)(chunk_len + prefix_len));
    int64_t total = 0;
    for (int b = 0; b < batch; ++b) {
        L3AC_REQUIRE(frames[b] >= 1 && frames[b] <= (INT64_MAX >> 12), "chunk_plan: frames[%d] = %lld", b, (long long)frames[b]);
        total += ceil_div64(round_up64(frames[b], round_to), chunk_len);
    }
    L3AC_REQUIRE(total <= INT32_MAX, "chunk_plan: %lld chunks", (long long)total);
    if (!desc_out) return total;
    L3AC_REQUIRE(cap >= total, "chunk_plan: %lld chunks but room for %lld descriptors", (long long)total, (long long)cap);
    int64_t row = 0;
    for (int b = 0; b < batch; ++b) {
        const int64_t n = round_up64(frames[b], round_to);
        for (int64_t i = 0; i < n; i += chunk_len, ++row) {
            l3ac_chunk_desc& d = desc_out[row];
            const int64_t start = i == 0 ? 0 : i - prefix_len;
            const int64_t stop = std::min(n, i + chunk_len);
            d.rec = b;
            d.row = (int32_t)row;
            d.start = start;
            d.frames = (int32_t)(stop - start);
            d.prefix = (int32_t)(i - start);
            d.pad = (int32_t)std::max<int64_t>(stop - std::max(frames[b], start), 0);  // (rounding adds < round_to <= a chunk's own frames)
            d.last = stop == n;
        }
    }
    return total;
}

int l3ac_chunk_cut(const void* src, int32_t recs, int64_t src_stride, int32_t c, const l3ac_chunk_desc* desc, int32_t count, void* dst,
                   int32_t rows, int64_t dst_row_frames, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    L3AC_REQUIRE(src && dst && recs > 0 && rows > 0 && c >= 1 && src_stride >= 1 && dst_row_frames >= 1, "chunk_cut: bad arguments");
    L3AC_REQUIRE((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 4 == 0, "chunk_cut: buffers must be 4-byte aligned");
    L3AC_TRY(check_descs("chunk_cut", desc, count, recs, INT64_MAX, rows, dst_row_frames));
    for (int i = 0; i < count; ++i)  // what is READ ends inside the source row; the zero tail is written only
        L3AC_REQUIRE(desc[i].start + desc[i].frames - desc[i].pad <= src_stride, "chunk_cut: descriptor %d reads to frame %lld of a row of %lld",
                     i, (long long)(desc[i].start + desc[i].frames - desc[i].pad), (long long)src_stride);
    for (int off = 0; off < count; off += ChunkBlock::CAP) {
        ChunkBlock blk{};
        const int n = std::min(count - off, (int)ChunkBlock::CAP);
        int64_t longest = 0, moved = 0;
        for (int i = 0; i < n; ++i) {
            blk.desc[i] = desc[off + i];
            longest = std::max<int64_t>(longest, blk.desc[i].frames);
            moved += blk.desc[i].frames;
        }
        ProfScope prof(s, "chunk_cut_kernel", 0.0, 8.0 * (double)moved * c);
        hipLaunchKernelGGL(chunk_cut_kernel, dim3(span_blocks(longest * c), (unsigned)n), dim3(THREADS), 0, s,
                           static_cast<const uint32_t*>(src), src_stride, c, static_cast<uint32_t*>(dst), dst_row_frames, blk);
        L3AC_LAUNCH_CHECK();
    }
    return L3AC_OK;
}

int l3ac_chunk_merge(const void* src, int32_t rows, int64_t src_row_frames, int32_t c, const l3ac_chunk_desc* desc, int32_t count, void* dst,
                     int32_t recs, int64_t dst_stride, int64_t out_frames, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    L3AC_REQUIRE(src && dst && recs > 0 && rows > 0 && c >= 1 && src_row_frames >= 1, "chunk_merge: bad arguments");
    L3AC_REQUIRE(out_frames >= 1 && out_frames <= dst_stride, "chunk_merge: out_frames %lld for rows of %lld", (long long)out_frames,
                 (long long)dst_stride);
    L3AC_REQUIRE((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) % 4 == 0, "chunk_merge: buffers must be 4-byte aligned");
    L3AC_TRY(check_descs("chunk_merge", desc, count, recs, out_frames, rows, src_row_frames));
    for (int off = 0; off < count; off += ChunkBlock::CAP) {
        ChunkBlock blk{};
        const int n = std::min(count - off, (int)ChunkBlock::CAP);
        int64_t longest = 0, moved = 0, zeroed = 0;
        for (int i = 0; i < n; ++i) {
            const l3ac_chunk_desc& d = blk.desc[i] = desc[off + i];
            const int64_t tail = d.last ? out_frames - (d.start + d.frames) : 0;
            longest = std::max<int64_t>(longest, std::max<int64_t>(d.frames - d.prefix, tail));
            moved += d.frames - d.prefix;
            zeroed += tail;
        }
        ProfScope prof(s, "chunk_merge_kernel", 0.0, (8.0 * (double)moved + 4.0 * (double)zeroed) * c);
        hipLaunchKernelGGL(chunk_merge_kernel, dim3(span_blocks(longest * c), (unsigned)n), dim3(THREADS), 0, s,
                           static_cast<const uint32_t*>(src), src_row_frames, c, static_cast<uint32_t*>(dst), dst_stride, out_frames, blk);
        L3AC_LAUNCH_CHECK();
    }
    return L3AC_OK;
}

}  // extern "C"
