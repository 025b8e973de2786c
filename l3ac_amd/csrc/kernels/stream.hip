// Streaming sessions: the state carried between pushes (l3ac_stream_gather / _carry / _append / _emit).
//
// A session of S live streams keeps ONE state buffer [S][state_frames][c]: stream i's row holds, from frame 0 on, the last `held` frames of
// the stream that can still be needed — its look-back followed directly by the frames that have not completed a chunk yet.  They are one
// contiguous piece of the stream, so there is no ring and nothing wraps.  `held` and the split are host values, like the lengths of a
// ragged call.  A push hands in [S][fresh_stride][c] new frames and runs in rounds in which every stream completes at most one chunk:
//   stream_gather_kernel   chunk row = state[slot][0 : held] ++ fresh[slot][off : off + take] ++ zeros(pad), into a rows tensor of its own
//                          (the rows of a ragged call, as chunk_cut_kernel builds them from whole recordings)
//   stream_carry_kernel    the next state, FROM THE ROW JUST BUILT: state[slot][0 : keep] = row[own - keep : own], own = held + take.  The
//                          kept frames overlap the frames the state held before (keep > own - held whenever the look-back is at least a
//                          step): moving them inside the state buffer would move a span onto an overlapping span, which no kernel here does
//   stream_append_kernel   after the last round: state[slot][held : held + take] = fresh[slot][off : off + take], what is left of the push
//   stream_emit_kernel     rows of a ragged call's output -> the push's output [S][out_frames][c]: frames [prefix, frames) of a row go to
//                          [out, out + frames - prefix) of stream slot's row, followed by `zero` zero frames (the stream's last chunk of the
//                          push fills its row up to out_frames; a stream that emits nothing has a descriptor of zeros alone).  The shape of
//                          chunk_merge_kernel, whose descriptor checks (start >= 0: the prefix lies INSIDE the recording row) do not admit a
//                          look-back longer than what a stream has emitted so far in the push
// The spans move through copy_span / zero_span (span_copy.hpp): 32-bit integers, 16-byte accesses where source and destination are congruent
// modulo 16 bytes, dwords otherwise, uniform per workgroup (one descriptor per blockIdx.y).  Every frame of a row and every live frame of the
// state is written by exactly one lane of one launch; the host checks refuse descriptors whose destinations overlap.
//
// The descriptors are host values and reach the device as KERNEL ARGUMENTS, StreamBlock::CAP per launch, the ChunkBlock way: no staging
// buffer, the caller's array may change after the call, a captured graph replays what it captured.
#include <algorithm>
#include <vector>

#include "../kernels.hpp"
#include "span_copy.hpp"

namespace {

constexpr int THREADS = SPAN_THREADS;

#define STREAM_LANE() \
    const l3ac_stream_desc d = blk.desc[blockIdx.y]; \
    const int64_t tid = (int64_t)blockIdx.x * THREADS + threadIdx.x, stride = (int64_t)gridDim.x * THREADS

// grid (span blocks, descriptors of this block)
__global__ __launch_bounds__(THREADS) void stream_gather_kernel(const uint32_t* __restrict__ state, int64_t state_frames,
                                                               const uint32_t* __restrict__ fresh, int64_t fresh_stride, int c,
                                                               uint32_t* __restrict__ rows, int64_t row_frames, const StreamBlock blk) {
    STREAM_LANE();
    uint32_t* row = rows + (int64_t)d.row * row_frames * c;
    const int64_t held = (int64_t)d.held * c, take = (int64_t)d.take * c;
    if (held > 0) copy_span(row, state + (int64_t)d.slot * state_frames * c, held, tid, stride);
    if (take > 0) copy_span(row + held, fresh + ((int64_t)d.slot * fresh_stride + d.off) * c, take, tid, stride);
    if (d.pad > 0) zero_span(row + held + take, (int64_t)d.pad * c, tid, stride);
}

__global__ __launch_bounds__(THREADS) void stream_carry_kernel(const uint32_t* __restrict__ rows, int64_t row_frames, int c,
                                                              uint32_t* __restrict__ state, int64_t state_frames, const StreamBlock blk) {
    STREAM_LANE();
    const int64_t own = (int64_t)d.held + d.take;
    copy_span(state + (int64_t)d.slot * state_frames * c, rows + ((int64_t)d.row * row_frames + own - d.keep) * c, (int64_t)d.keep * c, tid, stride);
}

__global__ __launch_bounds__(THREADS) void stream_append_kernel(const uint32_t* __restrict__ fresh, int64_t fresh_stride, int c,
                                                               uint32_t* __restrict__ state, int64_t state_frames, const StreamBlock blk) {
    STREAM_LANE();
    copy_span(state + ((int64_t)d.slot * state_frames + d.held) * c, fresh + ((int64_t)d.slot * fresh_stride + d.off) * c, (int64_t)d.take * c, tid,
              stride);
}

__global__ __launch_bounds__(THREADS) void stream_emit_kernel(const uint32_t* __restrict__ rows, int64_t row_frames, int c,
                                                             uint32_t* __restrict__ dst, int64_t dst_stride, const StreamBlock blk) {
    STREAM_LANE();
    const int64_t n = (int64_t)d.held + d.take + d.pad - d.prefix;
    uint32_t* out = dst + ((int64_t)d.slot * dst_stride + d.out) * c;
    if (n > 0) copy_span(out, rows + ((int64_t)d.row * row_frames + d.prefix) * c, n * c, tid, stride);
    if (d.zero > 0) zero_span(out + n * c, (int64_t)d.zero * c, tid, stride);
}

#undef STREAM_LANE

struct Piece {  // frames [begin, end) of row `key` of a destination
    int64_t key, begin, end;
};

// no two descriptors of a call write the same frame
int check_disjoint(const char* who, std::vector<Piece>& pieces) {
    std::sort(pieces.begin(), pieces.end(), [](const Piece& a, const Piece& b) { return a.key != b.key ? a.key < b.key : a.begin < b.begin; });
    for (size_t i = 1; i < pieces.size(); ++i)
        L3AC_REQUIRE(pieces[i].key != pieces[i - 1].key || pieces[i].begin >= pieces[i - 1].end || pieces[i].begin == pieces[i].end ||
                         pieces[i - 1].begin == pieces[i - 1].end,
                     "%s: two descriptors write frames [%lld, %lld) and [%lld, %lld) of destination row %lld", who,
                     (long long)pieces[i - 1].begin, (long long)pieces[i - 1].end, (long long)pieces[i].begin, (long long)pieces[i].end,
                     (long long)pieces[i].key);
    return L3AC_OK;
}

bool apart(const void* a, int64_t a_elements, const void* b, int64_t b_elements) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 + (uintptr_t)a_elements * 4 <= b0 || b0 + (uintptr_t)b_elements * 4 <= a0;
}

int check_common(const char* who, const l3ac_stream_desc* desc, int count, int streams, int c) {
    L3AC_REQUIRE(desc && count > 0, "%s: no descriptors", who);
    L3AC_REQUIRE(streams > 0 && c >= 1, "%s: %d streams of %d-element frames", who, streams, c);
    for (int i = 0; i < count; ++i) {
        const l3ac_stream_desc& d = desc[i];
        L3AC_REQUIRE(d.slot >= 0 && d.slot < streams, "%s: descriptor %d: stream %d of %d", who, i, d.slot, streams);
        L3AC_REQUIRE(d.held >= 0 && d.take >= 0 && d.pad >= 0 && d.keep >= 0 && d.prefix >= 0 && d.zero >= 0 && d.off >= 0 && d.out >= 0 &&
                         (int64_t)d.held + d.take + d.pad <= INT32_MAX,
                     "%s: descriptor %d: held %d, take %d at %lld, zero tail %d, keep %d, prefix %d, zeros %d, out %lld", who, i, d.held, d.take,
                     (long long)d.off, d.pad, d.keep, d.prefix, d.zero, (long long)d.out);
    }
    return L3AC_OK;
}

template <class Launch>
int launch_blocks(const l3ac_stream_desc* desc, int count, int c, int64_t (*span)(const l3ac_stream_desc&), Launch&& launch) {
    for (int off = 0; off < count; off += StreamBlock::CAP) {
        StreamBlock blk{};
        const int n = std::min(count - off, (int)StreamBlock::CAP);
        int64_t longest = 0, moved = 0;
        for (int i = 0; i < n; ++i) {
            blk.desc[i] = desc[off + i];
            longest = std::max(longest, span(blk.desc[i]));
            moved += span(blk.desc[i]);
        }
        L3AC_TRY(launch(blk, dim3(span_blocks(longest * c), (unsigned)n), moved));
    }
    return L3AC_OK;
}

}  // namespace

extern "C" {

int l3ac_stream_gather(const void* state, int32_t streams, int64_t state_frames, const void* fresh, int64_t fresh_frames, int64_t fresh_stride,
                       int32_t c, const l3ac_stream_desc* desc, int32_t count, void* rows, int32_t n_rows, int64_t row_frames, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    L3AC_TRY(check_common("stream_gather", desc, count, streams, c));
    L3AC_REQUIRE(state && rows && state_frames >= 1 && n_rows > 0 && row_frames >= 1 && fresh_frames >= 0 && fresh_stride >= 1,
                 "stream_gather: bad arguments");
    L3AC_REQUIRE((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(fresh) | reinterpret_cast<uintptr_t>(rows)) % 4 == 0,
                 "stream_gather: buffers must be 4-byte aligned");
    L3AC_REQUIRE(apart(state, (int64_t)streams * state_frames * c, rows, (int64_t)n_rows * row_frames * c), "stream_gather: rows overlap the state");
    std::vector<Piece> pieces;
    for (int i = 0; i < count; ++i) {
        const l3ac_stream_desc& d = desc[i];
        const int64_t frames = (int64_t)d.held + d.take + d.pad;
        L3AC_REQUIRE(d.row >= 0 && d.row < n_rows && frames >= 1 && frames <= row_frames, "stream_gather: descriptor %d: row %d of %d, %lld frames for rows of %lld",
                     i, d.row, n_rows, (long long)frames, (long long)row_frames);
        L3AC_REQUIRE(d.held <= state_frames, "stream_gather: descriptor %d takes %d frames of a state row of %lld", i, d.held, (long long)state_frames);
        L3AC_REQUIRE(d.take == 0 || (fresh && d.off + d.take <= fresh_frames), "stream_gather: descriptor %d reads new frames [%lld, %lld) of %lld", i,
                     (long long)d.off, (long long)(d.off + d.take), (long long)fresh_frames);
        pieces.push_back({d.row, 0, frames});
    }
    L3AC_TRY(check_disjoint("stream_gather", pieces));
    return launch_blocks(desc, count, c, [](const l3ac_stream_desc& d) { return (int64_t)d.held + d.take + d.pad; },
                         [&](const StreamBlock& blk, dim3 grid, int64_t moved) -> int {
                             ProfScope prof(s, "stream_gather_kernel", 0.0, 8.0 * (double)moved * c);
                             hipLaunchKernelGGL(stream_gather_kernel, grid, dim3(THREADS), 0, s, static_cast<const uint32_t*>(state), state_frames,
                                                static_cast<const uint32_t*>(fresh), fresh_stride, c, static_cast<uint32_t*>(rows), row_frames, blk);
                             L3AC_LAUNCH_CHECK();
                             return L3AC_OK;
                         });
}

int l3ac_stream_carry(const void* rows, int32_t n_rows, int64_t row_frames, int32_t c, const l3ac_stream_desc* desc, int32_t count, void* state,
                      int32_t streams, int64_t state_frames, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    L3AC_TRY(check_common("stream_carry", desc, count, streams, c));
    L3AC_REQUIRE(state && rows && state_frames >= 1 && n_rows > 0 && row_frames >= 1, "stream_carry: bad arguments");
    L3AC_REQUIRE((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(rows)) % 4 == 0, "stream_carry: buffers must be 4-byte aligned");
    L3AC_REQUIRE(apart(state, (int64_t)streams * state_frames * c, rows, (int64_t)n_rows * row_frames * c), "stream_carry: rows overlap the state");
    std::vector<Piece> pieces;
    for (int i = 0; i < count; ++i) {
        const l3ac_stream_desc& d = desc[i];
        const int64_t own = (int64_t)d.held + d.take;
        L3AC_REQUIRE(d.row >= 0 && d.row < n_rows && own <= row_frames, "stream_carry: descriptor %d: row %d of %d, %lld frames for rows of %lld", i, d.row,
                     n_rows, (long long)own, (long long)row_frames);
        L3AC_REQUIRE(d.keep <= own && d.keep <= state_frames, "stream_carry: descriptor %d keeps %d of %lld frames in a state row of %lld", i, d.keep,
                     (long long)own, (long long)state_frames);
        pieces.push_back({d.slot, 0, d.keep});
    }
    L3AC_TRY(check_disjoint("stream_carry", pieces));
    return launch_blocks(desc, count, c, [](const l3ac_stream_desc& d) { return (int64_t)d.keep; },
                         [&](const StreamBlock& blk, dim3 grid, int64_t moved) -> int {
                             ProfScope prof(s, "stream_carry_kernel", 0.0, 8.0 * (double)moved * c);
                             hipLaunchKernelGGL(stream_carry_kernel, grid, dim3(THREADS), 0, s, static_cast<const uint32_t*>(rows), row_frames, c,
                                                static_cast<uint32_t*>(state), state_frames, blk);
                             L3AC_LAUNCH_CHECK();
                             return L3AC_OK;
                         });
}

int l3ac_stream_append(const void* fresh, int64_t fresh_frames, int64_t fresh_stride, int32_t c, const l3ac_stream_desc* desc, int32_t count,
                       void* state, int32_t streams, int64_t state_frames, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    L3AC_TRY(check_common("stream_append", desc, count, streams, c));
    L3AC_REQUIRE(state && state_frames >= 1 && fresh_frames >= 0 && fresh_stride >= 1, "stream_append: bad arguments");
    L3AC_REQUIRE((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(fresh)) % 4 == 0, "stream_append: buffers must be 4-byte aligned");
    std::vector<Piece> pieces;
    for (int i = 0; i < count; ++i) {
        const l3ac_stream_desc& d = desc[i];
        L3AC_REQUIRE((int64_t)d.held + d.take <= state_frames, "stream_append: descriptor %d: %d + %d frames in a state row of %lld", i, d.held, d.take,
                     (long long)state_frames);
        L3AC_REQUIRE(d.take == 0 || (fresh && d.off + d.take <= fresh_frames), "stream_append: descriptor %d reads new frames [%lld, %lld) of %lld", i,
                     (long long)d.off, (long long)(d.off + d.take), (long long)fresh_frames);
        pieces.push_back({d.slot, d.held, (int64_t)d.held + d.take});
    }
    L3AC_TRY(check_disjoint("stream_append", pieces));
    return launch_blocks(desc, count, c, [](const l3ac_stream_desc& d) { return (int64_t)d.take; },
                         [&](const StreamBlock& blk, dim3 grid, int64_t moved) -> int {
                             ProfScope prof(s, "stream_append_kernel", 0.0, 8.0 * (double)moved * c);
                             hipLaunchKernelGGL(stream_append_kernel, grid, dim3(THREADS), 0, s, static_cast<const uint32_t*>(fresh), fresh_stride, c,
                                                static_cast<uint32_t*>(state), state_frames, blk);
                             L3AC_LAUNCH_CHECK();
                             return L3AC_OK;
                         });
}

int l3ac_stream_emit(const void* rows, int32_t n_rows, int64_t row_frames, int32_t c, const l3ac_stream_desc* desc, int32_t count, void* dst,
                     int32_t streams, int64_t dst_stride, int64_t out_frames, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    L3AC_TRY(check_common("stream_emit", desc, count, streams, c));
    L3AC_REQUIRE(rows && dst && n_rows > 0 && row_frames >= 1, "stream_emit: bad arguments");
    L3AC_REQUIRE(out_frames >= 1 && out_frames <= dst_stride, "stream_emit: out_frames %lld for rows of %lld", (long long)out_frames, (long long)dst_stride);
    L3AC_REQUIRE((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(dst)) % 4 == 0, "stream_emit: buffers must be 4-byte aligned");
    L3AC_REQUIRE(apart(dst, (int64_t)streams * dst_stride * c, rows, (int64_t)n_rows * row_frames * c), "stream_emit: rows overlap the output");
    std::vector<Piece> pieces;
    for (int i = 0; i < count; ++i) {
        const l3ac_stream_desc& d = desc[i];
        const int64_t frames = (int64_t)d.held + d.take + d.pad;
        L3AC_REQUIRE(d.prefix <= frames && frames <= row_frames && (frames == d.prefix || (d.row >= 0 && d.row < n_rows)),
                     "stream_emit: descriptor %d: row %d of %d, %lld frames (prefix %d) for rows of %lld", i, d.row, n_rows, (long long)frames, d.prefix,
                     (long long)row_frames);
        L3AC_REQUIRE(d.out + (frames - d.prefix) + d.zero <= out_frames, "stream_emit: descriptor %d writes to frame %lld of %lld", i,
                     (long long)(d.out + (frames - d.prefix) + d.zero), (long long)out_frames);
        pieces.push_back({d.slot, d.out, d.out + (frames - d.prefix) + d.zero});
    }
    L3AC_TRY(check_disjoint("stream_emit", pieces));
    return launch_blocks(desc, count, c, [](const l3ac_stream_desc& d) { return std::max<int64_t>((int64_t)d.held + d.take + d.pad - d.prefix, d.zero); },
                         [&](const StreamBlock& blk, dim3 grid, int64_t moved) -> int {
                             ProfScope prof(s, "stream_emit_kernel", 0.0, 8.0 * (double)moved * c);
                             hipLaunchKernelGGL(stream_emit_kernel, grid, dim3(THREADS), 0, s, static_cast<const uint32_t*>(rows), row_frames, c,
                                                static_cast<uint32_t*>(dst), dst_stride, blk);
                             L3AC_LAUNCH_CHECK();
                             return L3AC_OK;
                         });
}

}  // extern "C"
