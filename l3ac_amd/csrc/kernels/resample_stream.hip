// Streaming sample-rate conversion: packets in, l3ac_resample's bits out (l3ac_resample_stream).
//
// Geometry (resample.hip's, per stream): output m reads inputs i(m) - (K - 1) .. i(m), i(m) = (m down + half_len) div up, with the taps of
// phase (m down + half_len) mod up.  A stream that has received N inputs and emitted E outputs keeps its last `held` inputs in its state row.
// A push hands in `take` new inputs; the stream's input is the VIRTUAL row
//   state_in[slot][0 : held] ++ fresh[slot][0 : take] ++ zeros,        zeros before position 0 as well,
// whose position 0 is input N - held of the stream.  Output E + j of the push has q = q0 + j down, q0 = E down + half_len - (N - held) up:
// its newest input sits at row position q div up, its phase is q mod up (the origin moved by a whole number of inputs).  Neither N nor E
// reaches the device: nothing in a descriptor grows with the age of a stream.
//
// Kernel: one workgroup = one stream (blockIdx.y: its descriptor) x n_blk <= 256 consecutive outputs; LANES ARE OUTPUTS, so every lane has
// its own phase and its own window offset.  The inputs the block needs for a chunk of RSS_TAPS taps are read by row position from their two
// sources into LDS (no row tensor is gathered first); each lane then runs the fp32 fmaf chain over t = 0 .. K-1 in that order from +0 with
// variant 0 of its phase's bank row (the unshifted taps): resample_poly_kernel's chain without its zero taps, which are no-ops on finite
// inputs.  For up == 1 there is one phase and the tap pointer is wave-uniform (scalar loads); otherwise taps are per-lane reads of the
// bank (at most a few hundred KiB per rate pair: L2-resident).  n_blk is chosen so that the inputs between a block's first and last
// output stay within RSS_SPAN; long filters are walked in tap chunks in ascending t, restaging the window.
// Every output element of a stream's row below out_frames is written exactly once: the stream's `count` outputs, then zeros.
// The same launch writes the stream's NEXT state, the last `keep` inputs of state ++ fresh, into the session's OTHER state buffer (the span
// overlaps the one it is read from; no kernel moves a span onto an overlapping span of its own buffer), idle streams included.
// Equal rates: a copy of the packet (copy_span: bit for bit, -0.0 stays -0.0; fmaf(1, -0, +0) would not keep it), no state.
//
// Descriptors are host values passed as kernel arguments, ResampleStreamBlock::CAP per launch, the StreamBlock way.
#include <algorithm>
#include <vector>

#include "../kernels.hpp"
#include "span_copy.hpp"

namespace {

constexpr int RSS_THREADS = SPAN_THREADS;  // one output per lane
constexpr int RSS_SPAN = 2048;             // most inputs between the newest inputs of a block's first and last output
constexpr int RSS_TAPS = 64;               // taps per staged window, resample_poly_kernel's chunk
constexpr int RSS_WIN = RSS_SPAN + RSS_TAPS;

struct RssGeom {
    int64_t state_stride, fresh_stride, out_stride, out_frames;
    int up, down, K, KE, n_blk;
};

template <bool ONE_PHASE>
__global__ __launch_bounds__(RSS_THREADS) void resample_stream_kernel(const float* __restrict__ state_in, float* __restrict__ state_out,
                                                                      const float* __restrict__ fresh, const float* __restrict__ bank,
                                                                      float* __restrict__ out, const RssGeom g, const ResampleStreamBlock blk) {
    __shared__ float xs[RSS_WIN];
    const l3ac_resample_stream_desc d = blk.desc[blockIdx.y];
    const float* sin = state_in + (int64_t)d.slot * g.state_stride;
    const float* nw = fresh + (int64_t)d.slot * g.fresh_stride;  // (not dereferenced when take == 0)
    const int own = d.held + d.take;

    // the next state: row positions [own - keep, own), by all the workgroups of this stream
    if (d.keep > 0) {
        const int64_t tid = (int64_t)blockIdx.x * RSS_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * RSS_THREADS;
        uint32_t* dst = reinterpret_cast<uint32_t*>(state_out + (int64_t)d.slot * g.state_stride);
        const int start = own - d.keep;
        const int from_state = max(0, min(d.keep, d.held - start));
        if (from_state > 0) copy_span(dst, reinterpret_cast<const uint32_t*>(sin + start), from_state, tid, stride);
        if (d.keep > from_state)
            copy_span(dst + from_state, reinterpret_cast<const uint32_t*>(nw + (start + from_state - d.held)), d.keep - from_state, tid, stride);
    }

    const int64_t j0 = (int64_t)blockIdx.x * g.n_blk;
    if (j0 >= g.out_frames) return;  // a push that emits nothing: the state alone
    const int nb = (int)min((int64_t)g.n_blk, g.out_frames - j0);
    const int live = (int)max((int64_t)0, min((int64_t)nb, (int64_t)d.count - j0));  // outputs of this block the stream emits; zeros after
    float acc = 0.f;
    if (live > 0) {  // uniform over the workgroup
        const int64_t qb = (int64_t)d.q0 + j0 * g.down;
        const int64_t ib = qb / g.up;
        const int rb = (int)(qb - ib * g.up);
        const int o = min((int)threadIdx.x, live - 1);  // lanes without an output shadow the last one: their reads stay inside the window
        const int v = rb + o * g.down;                  // < up + 255 down
        const int di = v / g.up;                        // this lane's newest input, relative to the block's first output's
        const int phase = ONE_PHASE ? 0 : v - di * g.up;
        const int span = (rb + (live - 1) * g.down) / g.up;  // <= RSS_SPAN by the choice of n_blk
        const int64_t base = ib - (g.K - 1);                 // row position of the first output's oldest input
        const float* taps = bank + (int64_t)4 * phase * g.KE;
        for (int t0 = 0; t0 < g.K; t0 += RSS_TAPS) {
            const int tc = min(RSS_TAPS, g.K - t0);
            const int wlen = span + tc;  // <= RSS_WIN
            if (t0) __syncthreads();     // every lane is done with the previous chunk's window
            for (int e = threadIdx.x; e < wlen; e += RSS_THREADS) {
                const int64_t r = base + t0 + e;
                float x = 0.f;  // before the stream's first sample, after its end
                if (r >= 0) {
                    if (r < d.held) x = sin[r];
                    else if (r < own) x = nw[r - d.held];
                }
                xs[e] = x;
            }
            __syncthreads();
            const float* xp = xs + di;
            const float* gp = taps + t0;
#pragma unroll 4
            for (int t = 0; t < tc; ++t) acc = fmaf(gp[t], xp[t], acc);
        }
    }
    if ((int)threadIdx.x < nb) out[(int64_t)d.slot * g.out_stride + j0 + threadIdx.x] = (int)threadIdx.x < live ? acc : 0.f;
}

// equal rates: out[slot][0 : take] = fresh[slot][0 : take], zeros up to out_frames
__global__ __launch_bounds__(RSS_THREADS) void resample_stream_copy_kernel(const uint32_t* __restrict__ fresh, int64_t fresh_stride,
                                                                           uint32_t* __restrict__ out, int64_t out_stride, int64_t out_frames,
                                                                           const ResampleStreamBlock blk) {
    const l3ac_resample_stream_desc d = blk.desc[blockIdx.y];
    const int64_t tid = (int64_t)blockIdx.x * RSS_THREADS + threadIdx.x, stride = (int64_t)gridDim.x * RSS_THREADS;
    uint32_t* row = out + (int64_t)d.slot * out_stride;
    if (d.take > 0) copy_span(row, fresh + (int64_t)d.slot * fresh_stride, d.take, tid, stride);
    if (out_frames > d.take) zero_span(row + d.take, out_frames - d.take, tid, stride);
}

bool rss_apart(const void* a, int64_t a_elements, const void* b, int64_t b_elements) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return !a || !b || a0 + (uintptr_t)a_elements * 4 <= b0 || b0 + (uintptr_t)b_elements * 4 <= a0;
}

}  // namespace

int64_t resample_stream_state_floats(const ResamplePlan& p) { return 4 * ceil_div64(p.K - 1, 4); }

extern "C" {

int64_t l3ac_resample_stream_state(int32_t in_rate, int32_t out_rate) {
    ResamplePlan p;
    L3AC_TRY(resample_plan(in_rate, out_rate, &p));
    return resample_stream_state_floats(p);
}

int l3ac_resample_stream(const float* state_in, float* state_out, int32_t streams, int64_t state_stride, const float* fresh, int64_t fresh_frames,
                         int64_t fresh_stride, int32_t in_rate, int32_t out_rate, const float* bank, const l3ac_resample_stream_desc* desc,
                         int32_t count, float* out, int64_t out_frames, int64_t out_stride, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    ResamplePlan p;
    L3AC_TRY(resample_plan(in_rate, out_rate, &p));
    const bool copy = p.up == p.down;
    L3AC_REQUIRE(desc && count > 0, "resample_stream: no descriptors");
    L3AC_REQUIRE(streams > 0 && state_stride >= 0 && fresh_frames >= 0 && fresh_stride >= fresh_frames && fresh_stride >= 1,
                 "resample_stream: %d streams, state rows of %lld, %lld new frames in rows of %lld", streams, (long long)state_stride,
                 (long long)fresh_frames, (long long)fresh_stride);
    L3AC_REQUIRE(out_frames >= 0 && out_frames <= INT32_MAX && out_stride >= out_frames && out_stride >= 1 && (out || out_frames == 0),
                 "resample_stream: out_frames %lld for output rows of %lld", (long long)out_frames, (long long)out_stride);
    L3AC_REQUIRE(copy || (state_in && state_out && bank), "resample_stream: null state buffer or filter bank");
    const int64_t n_state = (int64_t)streams * state_stride, n_fresh = (int64_t)streams * fresh_stride, n_out = (int64_t)streams * out_stride;
    L3AC_REQUIRE(copy || rss_apart(state_in, n_state, state_out, n_state), "resample_stream: the two state buffers overlap");
    L3AC_REQUIRE(rss_apart(out, n_out, fresh, n_fresh) && (copy || (rss_apart(out, n_out, state_in, n_state) && rss_apart(out, n_out, state_out, n_state) &&
                                                                    rss_apart(fresh, n_fresh, state_out, n_state))),
                 "resample_stream: the output or the next state overlaps an input");
    L3AC_REQUIRE((reinterpret_cast<uintptr_t>(state_in) | reinterpret_cast<uintptr_t>(state_out) | reinterpret_cast<uintptr_t>(fresh) |
                  reinterpret_cast<uintptr_t>(out)) % 4 == 0, "resample_stream: buffers must be 4-byte aligned");
    const int64_t q_end = (int64_t)p.K * p.up;
    std::vector<int> slots;
    bool moves = false;
    for (int i = 0; i < count; ++i) {
        const l3ac_resample_stream_desc& d = desc[i];
        L3AC_REQUIRE(d.slot >= 0 && d.slot < streams, "resample_stream: descriptor %d: stream %d of %d", i, d.slot, streams);
        L3AC_REQUIRE(d.held >= 0 && d.held <= state_stride, "resample_stream: descriptor %d holds %d frames of a state row of %lld", i, d.held,
                     (long long)state_stride);
        L3AC_REQUIRE(d.take >= 0 && d.take <= fresh_frames && (d.take == 0 || fresh), "resample_stream: descriptor %d takes %d of %lld new frames", i,
                     d.take, (long long)fresh_frames);
        L3AC_REQUIRE(d.count >= 0 && d.count <= out_frames, "resample_stream: descriptor %d emits %d frames into rows of %lld", i, d.count,
                     (long long)out_frames);
        L3AC_REQUIRE(d.keep >= 0 && d.keep <= state_stride && (int64_t)d.keep <= (int64_t)d.held + d.take,
                     "resample_stream: descriptor %d keeps %d of %d + %d frames in a state row of %lld", i, d.keep, d.held, d.take, (long long)state_stride);
        L3AC_REQUIRE(d.q0 >= 0 && d.q0 < q_end, "resample_stream: descriptor %d: origin %d outside [0, %lld)", i, d.q0, (long long)q_end);
        L3AC_REQUIRE(!copy || (d.held == 0 && d.keep == 0 && d.count == d.take),
                     "resample_stream: descriptor %d: equal rates pass %d frames through, not %d (held %d, keep %d)", i, d.take, d.count, d.held, d.keep);
        slots.push_back(d.slot);
        moves = moves || d.keep > 0;
    }
    std::sort(slots.begin(), slots.end());
    L3AC_REQUIRE(std::adjacent_find(slots.begin(), slots.end()) == slots.end(), "resample_stream: two descriptors for one stream");
    if (out_frames == 0 && !moves) return L3AC_OK;  // nothing to emit, nothing to keep
    RssGeom g{};
    g.state_stride = state_stride;
    g.fresh_stride = fresh_stride;
    g.out_stride = out_stride;
    g.out_frames = out_frames;
    g.up = p.up;
    g.down = p.down;
    g.K = p.K;
    g.KE = p.KE;
    g.n_blk = (int)std::min<int64_t>(RSS_THREADS, (int64_t)RSS_SPAN * p.up / p.down + 1);
    for (int off = 0; off < count; off += ResampleStreamBlock::CAP) {
        ResampleStreamBlock blk{};
        const int n = std::min(count - off, (int)ResampleStreamBlock::CAP);
        double emitted = 0.0, moved = 0.0;
        for (int i = 0; i < n; ++i) {
            blk.desc[i] = desc[off + i];
            emitted += blk.desc[i].count;
            moved += blk.desc[i].take + blk.desc[i].keep;
        }
        if (copy) {
            if (out_frames == 0) continue;
            ProfScope prof(s, "resample_stream_copy_kernel", 0.0, 4.0 * ((double)n * out_frames + moved));
            hipLaunchKernelGGL(resample_stream_copy_kernel, dim3(span_blocks(out_frames), (unsigned)n), dim3(RSS_THREADS), 0, s,
                               reinterpret_cast<const uint32_t*>(fresh), fresh_stride, reinterpret_cast<uint32_t*>(out), out_stride, out_frames, blk);
            L3AC_LAUNCH_CHECK();
            continue;
        }
        const dim3 grid((unsigned)std::max<int64_t>(ceil_div64(out_frames, g.n_blk), 1), (unsigned)n);
        ProfScope prof(s, "resample_stream_kernel", 2.0 * emitted * p.K, 4.0 * ((double)n * out_frames + moved));
        if (p.up == 1)
            hipLaunchKernelGGL((resample_stream_kernel<true>), grid, dim3(RSS_THREADS), 0, s, state_in, state_out, fresh, bank, out, g, blk);
        else
            hipLaunchKernelGGL((resample_stream_kernel<false>), grid, dim3(RSS_THREADS), 0, s, state_in, state_out, fresh, bank, out, g, blk);
        L3AC_LAUNCH_CHECK();
    }
    return L3AC_OK;
}

}  // extern "C"
