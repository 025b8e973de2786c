// Recursive (IIR) filtering of batches of mono clips: scipy.signal.sosfilt, one-shot and streaming, and the Butterworth designs
// (include/l3ac_hip.h, "IIR filtering").  No reference counterpart.  Everything here is fp64; the fp32 samples convert
// exactly.
//
// A cascade of N <= 8 second-order sections (transposed direct form II, the order of biquad() in loudness.hip and of scipy) is a linear
// recurrence with a 2N-value state (s1, s2 of section 0, s1, s2 of section 1, ...).  It runs in parallel over time in fixed segments of
// IIR_SEG samples anchored at the clip's (or the stream's) sample 0, in the three phases of loudness.hip:
//   0. sos_matrix_kernel        M, the 2N x 2N matrix that advances the cascade's state over IIR_SEG samples of zero input: lane k runs
//                               the cascade on IIR_SEG zero samples from the unit state e_k in pair arithmetic (pair.hpp) and writes
//                               column k as hi + lo into the call's scratch.  On every call: no table, no upload, nothing to warm up
//   A. sos_pass_kernel<.,false> every (row, segment) lane filters its samples from a ZERO state and writes its 2N-value end state
//   B. sos_scan_kernel          one wave per row, lane r holding row r of M: start_{s+1} = M start_s + end_s over the row's COMPLETE
//                               segments, M, the running state and the products as pairs; hi(start_s) replaces end_s
//   C. sos_pass_kernel<.,true>  every lane reruns the recursion from hi(start_s) and writes y (fp64 or (float)y), zeros at and after
//                               the row's length
// A row is a clip (l3ac_sosfilt: it starts from rest) or a stream's share of one push (l3ac_sosfilt_stream).  A stream at position
// s IIR_SEG + k carries [start pair hi 2N | lo 2N | running true state 2N | running zero-state state 2N] and the host integer k: the
// lane of the push's first segment skips the k samples it has had and continues BOTH recursions from the carried values (k == 0: from
// hi(start) and from zero, as any lane), the scan starts from the carried pair, and the lane of the push's last segment saves both
// running states.  A descriptor flagged fresh (a stream's first push, whatever its slot held before) reads nothing of state_in: it starts
// from rest, as a clip does.  Every sample therefore goes through the same operations in the same order however the stream is cut: the
// concatenation of a stream's outputs is l3ac_sosfilt of the whole stream bit for bit.  One kernel family serves both entries.
//
// A row's values depend on its own samples only, never on the batch, the row's position, the strides or the scratch size; no atomics.
// One lane per segment reads rows IIR_SEG floats apart, so a wave's 64 segments are staged through LDS 32 samples at a time at an odd
// pitch, as loudness_pass_kernel stages its loads, and y leaves through a second tile the same way: loads and stores both run along the
// rows.  Contraction is off for this whole file, host code included.
#include "metric_common.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

#include "pair.hpp"

namespace {

constexpr int IIR_SEG = 256;            // samples per segment: part of the definition of the bits
constexpr int IIR_MAX_SECTIONS = 8;
constexpr int IIR_LANES = 64;           // segments per workgroup: one wave, one lane per segment
constexpr int IIR_CHUNK = 32;           // samples of every segment staged per round
constexpr int IIR_PITCH = IIR_CHUNK + 1;  // odd: lane l reads bank (l + j) % 32
constexpr int IIR_MAX_ORDER = 16;

struct SosCoef {  // b0 b1 b2 a1 a2 of every section (a0 = 1)
    double c[IIR_MAX_SECTIONS][5];
};

struct SosRows {  // what every kernel is told about the launch's rows
    const int* lens;         // [rows] lengths of the clips, or null: max_samples each (one-shot)
    const int* desc;         // [rows][4] slot, k, take, flags of l3ac_sosfilt_stream_desc, or null: one-shot, row i is clip i from rest
    const double* state_in;  // [streams][state_stride], or null: every row starts from rest
    double* state_out;       // the other state buffer, or null
    int64_t state_stride, max_samples, segs_max;
    double* ends;            // [rows][segs_max][2N]: phase A's end states, then phase B's start states
    const double* m;         // M hi [2N][2N], then M lo [2N][2N], row-major
};

struct SosScratch {  // byte offsets into the caller's scratch, after the clips' lengths
    int64_t desc, m, ends, total_min, segs_max;
};

struct SosJob {
    int64_t slot, n;  // the row of audio, out and the state buffers; the samples of this call
    int k, end;       // samples the first segment has had before this call; the stream ends with it
    int fresh;        // the row starts from rest: nothing of state_in is read
};

__device__ __forceinline__ SosJob sos_job(const SosRows& r, int i) {
    if (r.desc) {
        const int flags = r.desc[4 * i + 3];
        return {r.desc[4 * i], r.desc[4 * i + 2], r.desc[4 * i + 1], flags & L3AC_SOS_END, (flags & L3AC_SOS_FRESH) || !r.state_in};
    }
    return {i, r.lens ? (int64_t)r.lens[i] : r.max_samples, 0, 0, 1};
}

// one sample through one section: biquad() of loudness.hip
__device__ __forceinline__ double sos_step(const double (&c)[5], double x, double& s1, double& s2) {
    const double y = c[0] * x + s1;
    s1 = c[1] * x - c[3] * y + s2;
    s2 = c[2] * x - c[4] * y;
    return y;
}

__device__ __forceinline__ Pair pair_sub(Pair a, Pair b) { return pair_add(a, {-b.hi, -b.lo}); }

// the same step on pairs, the coefficients as (c, 0): what designs M
__device__ __forceinline__ Pair sos_step_pair(const double (&c)[5], Pair x, Pair& s1, Pair& s2) {
    const Pair y = pair_add(pair_mul({c[0], 0.0}, x), s1);
    s1 = pair_add(pair_sub(pair_mul({c[1], 0.0}, x), pair_mul({c[3], 0.0}, y)), s2);
    s2 = pair_sub(pair_mul({c[2], 0.0}, x), pair_mul({c[4], 0.0}, y));
    return y;
}

// ---- phase 0: M; one workgroup, lane k = column k ------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(IIR_LANES) void sos_matrix_kernel(SosCoef f, double* __restrict__ m_hi, double* __restrict__ m_lo) {
    constexpr int NS = 2 * N;
    const int k = threadIdx.x;
    if (k >= NS) return;
    Pair st[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) st[i] = {i == k ? 1.0 : 0.0, 0.0};
    for (int t = 0; t < IIR_SEG; ++t) {
        Pair v = {0.0, 0.0};
#pragma unroll
        for (int sec = 0; sec < N; ++sec) v = sos_step_pair(f.c[sec], v, st[2 * sec], st[2 * sec + 1]);
    }
#pragma unroll
    for (int r = 0; r < NS; ++r) m_hi[r * NS + k] = st[r].hi, m_lo[r * NS + k] = st[r].lo;
}

// ---- phases A and C: grid (groups of 64 segments, rows), one wave ----------------------------------------------------------------------
// Segment s of a row covers the call's samples [s IIR_SEG - k, (s + 1) IIR_SEG - k) that lie in [0, n).
// OUT = false: from a zero state (segment 0 of a stream with k > 0: from the carried zero-state state); writes ends[row][s].
// OUT = true:  from ends[row][s], the scan's start state (segment 0 with k > 0: from the carried true state); writes y, and zeros from n
//              to max_samples.  The lane of the row's last segment writes its running state into state_out.
template <int N, bool OUT, bool F64>
__global__ __launch_bounds__(IIR_LANES) void sos_pass_kernel(const float* __restrict__ audio, int64_t stride, SosCoef f, SosRows r,
                                                            void* __restrict__ out, int64_t out_stride) {
    constexpr int NS = 2 * N;
    __shared__ float tin[IIR_LANES * IIR_PITCH];
    __shared__ double tout[OUT ? IIR_LANES * IIR_PITCH : 1];
    const SosJob job = sos_job(r, blockIdx.y);
    const int64_t s0 = (int64_t)blockIdx.x * IIR_LANES;
    const int64_t g0 = s0 * IIR_SEG - job.k;  // the call's index of the group's first sample (negative in a stream's first segment)
    const int lane = threadIdx.x;
    const int col = lane & (IIR_CHUNK - 1), half = lane >> 5;  // a round of loads or stores: row 2 i + half of a tile, column col
    const float* x = audio + job.slot * stride;
    const bool live = g0 < job.n;  // (the whole workgroup)
    if (!OUT && !live) return;

    auto store = [&](int c0, bool filtered) {  // the group's columns c0 .. c0 + 31 of y, along the rows
#pragma unroll
        for (int i = 0; i < IIR_CHUNK; ++i) {
            const int row = 2 * i + half;
            const int64_t idx = g0 + (int64_t)row * IIR_SEG + c0 + col;
            if (idx < 0 || idx >= r.max_samples) continue;
            const double v = filtered && idx < job.n ? tout[OUT ? row * IIR_PITCH + col : 0] : 0.0;
            if (F64) static_cast<double*>(out)[job.slot * out_stride + idx] = v;
            else static_cast<float*>(out)[job.slot * out_stride + idx] = (float)v;
        }
    };
    if (OUT && !live) {  // past the row's length: zeros
        for (int c0 = 0; c0 < IIR_SEG; c0 += IIR_CHUNK) store(c0, false);
        return;
    }

    const int64_t seg = s0 + lane;
    const int64_t base = seg * IIR_SEG - job.k;                                                // the call's index of the segment's sample 0
    const int first = (int)std::min<int64_t>(IIR_SEG, std::max<int64_t>(0, -base));             // the segment's samples of this call:
    const int last = (int)std::min<int64_t>(IIR_SEG, std::max<int64_t>(0, job.n - base));       // columns first .. last - 1
    const bool active = first < last;
    const int64_t n_seg = (job.k + job.n + IIR_SEG - 1) / IIR_SEG;
    double* e = r.ends + ((int64_t)blockIdx.y * r.segs_max + seg) * NS;  // (an active lane's segment is below segs_max)
    double st[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) st[i] = 0.0;
    if (active) {
        if (seg == 0 && job.k > 0 && !job.fresh) {
            const double* c = r.state_in + job.slot * r.state_stride + (OUT ? 2 : 3) * NS;
#pragma unroll
            for (int i = 0; i < NS; ++i) st[i] = c[i];
        } else if (OUT) {
#pragma unroll
            for (int i = 0; i < NS; ++i) st[i] = e[i];
        }
    }

    float pre[IIR_CHUNK];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int i = 0; i < IIR_CHUNK; ++i) {
            const int64_t idx = g0 + (int64_t)(2 * i + half) * IIR_SEG + c0 + col;
            pre[i] = (idx >= 0 && idx < job.n) ? x[idx] : 0.f;
        }
    };
    fetch(0);
    for (int c0 = 0; c0 < IIR_SEG; c0 += IIR_CHUNK) {
        __syncthreads();  // the previous round's reads of both tiles are over
#pragma unroll
        for (int i = 0; i < IIR_CHUNK; ++i) tin[(2 * i + half) * IIR_PITCH + col] = pre[i];
        __syncthreads();
        if (c0 + IIR_CHUNK < IIR_SEG) fetch(c0 + IIR_CHUNK);
        for (int j = 0; j < IIR_CHUNK; ++j) {
            if (c0 + j < first || c0 + j >= last) continue;
            double v = (double)tin[lane * IIR_PITCH + j];
#pragma unroll
            for (int sec = 0; sec < N; ++sec) v = sos_step(f.c[sec], v, st[2 * sec], st[2 * sec + 1]);
            if (OUT) tout[lane * IIR_PITCH + j] = v;
        }
        if (OUT) {
            __syncthreads();
            store(c0, true);
        }
    }
    if (!active) return;
    if (!OUT) {
#pragma unroll
        for (int i = 0; i < NS; ++i) e[i] = st[i];
    }
    if (r.state_out && seg == n_seg - 1) {
        double* c = r.state_out + job.slot * r.state_stride + (OUT ? 2 : 3) * NS;
#pragma unroll
        for (int i = 0; i < NS; ++i) c[i] = job.end ? 0.0 : st[i];
    }
}

// ---- phase B: one wave per row, lane r = row r of M; ends[row][s] = the end state from zero -> the start state ---------------------------
template <int N>
__global__ __launch_bounds__(IIR_LANES) void sos_scan_kernel(SosRows r) {
    constexpr int NS = 2 * N;
    const SosJob job = sos_job(r, blockIdx.x);
    const int lane = threadIdx.x;
    const int row = min(lane, NS - 1);  // (the lanes past 2N shadow the last row for the broadcasts; they load no end state and write nothing)
    const int64_t pos = job.k + job.n;
    const int64_t n_seg = (pos + IIR_SEG - 1) / IIR_SEG, n_whole = pos / IIR_SEG;  // segments touched; of them complete after this call
    Pair m[NS];
#pragma unroll
    for (int i = 0; i < NS; ++i) m[i] = {r.m[row * NS + i], r.m[NS * NS + row * NS + i]};
    const double* sin = job.fresh ? nullptr : r.state_in + job.slot * r.state_stride;
    Pair cur = {0.0, 0.0};
    if (sin) cur = {sin[row], sin[NS + row]};
    double* e = r.ends + (int64_t)blockIdx.x * r.segs_max * NS + row;
    for (int64_t s = 0; s < n_seg; ++s, e += NS) {
        const bool whole = s < n_whole;  // (only the last segment may be incomplete: its lane wrote no end state when the call brought it nothing)
        const double end = whole && lane < NS ? *e : 0.0;
        if (lane < NS) *e = cur.hi;  // the passes start from the pair rounded to fp64
        if (!whole) break;
        Pair acc = pair_mul(m[0], {__shfl(cur.hi, 0, 64), __shfl(cur.lo, 0, 64)});
#pragma unroll
        for (int i = 1; i < NS; ++i) acc = pair_add(acc, pair_mul(m[i], {__shfl(cur.hi, i, 64), __shfl(cur.lo, i, 64)}));
        cur = pair_add(acc, {end, 0.0});
    }
    if (!r.state_out || lane >= NS) return;
    double* so = r.state_out + job.slot * r.state_stride;
    so[lane] = job.end ? 0.0 : cur.hi;
    so[NS + lane] = job.end ? 0.0 : cur.lo;
    if (job.n == 0) {  // no lane of the passes ran: the running states follow as they are
        so[2 * NS + lane] = job.end || !sin ? 0.0 : sin[2 * NS + lane];
        so[3 * NS + lane] = job.end || !sin ? 0.0 : sin[3 * NS + lane];
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
// the cascade as the kernels take it, refused unless every section is finite and inside the stability triangle (an unstable cascade
// overflows M)
int sos_coef(const char* what, const double* sos, int32_t sections, SosCoef* f) {
    L3AC_REQUIRE(sections >= 1 && sections <= IIR_MAX_SECTIONS, "%s: sections %d outside 1..%d", what, sections, IIR_MAX_SECTIONS);
    L3AC_REQUIRE(sos, "%s: null sos", what);
    *f = SosCoef{};
    for (int s = 0; s < sections; ++s) {
        const double* c = sos + 5 * s;
        for (int i = 0; i < 5; ++i) {
            L3AC_REQUIRE(std::isfinite(c[i]), "%s: section %d has a non-finite coefficient", what, s);
            f->c[s][i] = c[i];
        }
        L3AC_REQUIRE(std::fabs(c[4]) < 1.0 && std::fabs(c[3]) < 1.0 + c[4],
                     "%s: section %d (a1 = %.17g, a2 = %.17g) is not stable: it needs |a2| < 1 and |a1| < 1 + a2", what, s, c[3], c[4]);
    }
    return L3AC_OK;
}

int sos_geom(const char* what, int32_t rows, int64_t max_samples, int32_t sections, SosScratch* sc) {
    L3AC_REQUIRE(sections >= 1 && sections <= IIR_MAX_SECTIONS, "%s: sections %d outside 1..%d", what, sections, IIR_MAX_SECTIONS);
    L3AC_TRY(check_clip_batch(what, rows, max_samples));
    const int64_t ns = 2 * sections;
    sc->segs_max = ceil_div64(max_samples + IIR_SEG - 1, IIR_SEG);  // a stream's first segment may begin IIR_SEG - 1 samples before the call
    ScratchPlan plan(rows);
    sc->desc = plan.take((int64_t)rows * 16);
    sc->m = plan.take(2 * ns * ns * 8);
    sc->ends = plan.take((int64_t)rows * sc->segs_max * ns * 8);
    sc->total_min = plan.bytes;
    return L3AC_OK;
}

template <int N>
int sos_matrix_n(hipStream_t s, const SosCoef& f, double* hi, double* lo) {
    ProfScope prof(s, "sos_matrix_kernel", 0.0, 0.0);
    hipLaunchKernelGGL(sos_matrix_kernel<N>, dim3(1), dim3(IIR_LANES), 0, s, f, hi, lo);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

// M, then the three phases over `rows` rows of at most max_samples samples (0: a push that brings nothing, the scan alone)
template <int N>
int sos_run_n(hipStream_t s, const float* audio, int64_t stride, int32_t rows, const SosCoef& f, SosRows r, void* out, int64_t out_stride, bool f64) {
    constexpr int NS = 2 * N;
    const bool passes = r.max_samples > 0;
    double* m = const_cast<double*>(r.m);
    if (passes) L3AC_TRY(sos_matrix_n<N>(s, f, m, m + NS * NS));
    const dim3 grid((unsigned)ceil_div64(r.segs_max, IIR_LANES), (unsigned)rows);
    const double flops = 9.0 * N * rows * (double)r.max_samples, bytes = 4.0 * rows * (double)r.max_samples;
    if (passes) {
        ProfScope prof(s, "sos_pass_kernel<state>", flops, bytes);
        hipLaunchKernelGGL((sos_pass_kernel<N, false, false>), grid, dim3(IIR_LANES), 0, s, audio, stride, f, r, out, out_stride);
        L3AC_LAUNCH_CHECK();
    }
    {
        ProfScope prof(s, "sos_scan_kernel", 22.0 * NS * NS * rows * (double)r.segs_max, 16.0 * NS * rows * (double)r.segs_max);
        hipLaunchKernelGGL(sos_scan_kernel<N>, dim3((unsigned)rows), dim3(IIR_LANES), 0, s, r);
        L3AC_LAUNCH_CHECK();
    }
    if (passes) {
        ProfScope prof(s, "sos_pass_kernel<output>", flops, bytes * (f64 ? 3.0 : 2.0));
        if (f64) hipLaunchKernelGGL((sos_pass_kernel<N, true, true>), grid, dim3(IIR_LANES), 0, s, audio, stride, f, r, out, out_stride);
        else hipLaunchKernelGGL((sos_pass_kernel<N, true, false>), grid, dim3(IIR_LANES), 0, s, audio, stride, f, r, out, out_stride);
        L3AC_LAUNCH_CHECK();
    }
    return L3AC_OK;
}

#define IIR_DISPATCH(sections, call)            \
    switch (sections) {                         \
        case 1: return call(1);                 \
        case 2: return call(2);                 \
        case 3: return call(3);                 \
        case 4: return call(4);                 \
        case 5: return call(5);                 \
        case 6: return call(6);                 \
        case 7: return call(7);                 \
        default: return call(8);                \
    }

int sos_run(hipStream_t s, const float* audio, int64_t stride, int32_t rows, const SosCoef& f, int32_t sections, const SosRows& r, void* out,
            int64_t out_stride, bool f64) {
#define IIR_RUN(n) sos_run_n<n>(s, audio, stride, rows, f, r, out, out_stride, f64)
    IIR_DISPATCH(sections, IIR_RUN)
#undef IIR_RUN
}

int sos_matrix(hipStream_t s, const SosCoef& f, int32_t sections, double* hi, double* lo) {
#define IIR_MATRIX(n) sos_matrix_n<n>(s, f, hi, lo)
    IIR_DISPATCH(sections, IIR_MATRIX)
#undef IIR_MATRIX
}

bool iir_apart(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return !a || !b || a0 + (uintptr_t)a_bytes <= b0 || b0 + (uintptr_t)b_bytes <= a0;
}

}  // namespace

extern "C" {

int32_t l3ac_sosfilt_segment(void) { return IIR_SEG; }

int64_t l3ac_sosfilt_scratch_bytes(int32_t batch, int64_t max_samples, int32_t sections) {
    SosScratch sc;
    L3AC_TRY(sos_geom("sosfilt", batch, max_samples, sections, &sc));
    return sc.total_min;
}

int l3ac_sosfilt(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, const double* sos,
                 int32_t sections, void* out, int64_t out_stride, int32_t out_f64, void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    SosCoef f;
    L3AC_TRY(sos_coef("sosfilt", sos, sections, &f));
    SosScratch sc;
    L3AC_TRY(sos_geom("sosfilt", batch, max_samples, sections, &sc));
    L3AC_REQUIRE(audio && out, "sosfilt: null buffer");
    L3AC_REQUIRE(batch == 1 || (audio_stride >= max_samples && out_stride >= max_samples), "sosfilt: row stride below max_samples %lld",
                 (long long)max_samples);
    L3AC_TRY(check_clip_lengths("sosfilt", samples, batch, max_samples));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "sosfilt", "sosfilt", samples, batch, scratch, scratch_bytes, sc.total_min, &lens));
    char* base = static_cast<char*>(scratch);
    SosRows r{};
    r.lens = lens;
    r.max_samples = max_samples;
    r.segs_max = sc.segs_max;
    r.ends = reinterpret_cast<double*>(base + sc.ends);
    r.m = reinterpret_cast<const double*>(base + sc.m);
    return sos_run(s, audio, audio_stride, batch, f, sections, r, out, out_stride, out_f64 != 0);
}

int l3ac_sosfilt_matrix(const double* sos, int32_t sections, double* hi, double* lo, void* stream) {
    SosCoef f;
    L3AC_TRY(sos_coef("sosfilt_matrix", sos, sections, &f));
    L3AC_REQUIRE(hi && lo, "sosfilt_matrix: null buffer");
    return sos_matrix((hipStream_t)stream, f, sections, hi, lo);
}

int64_t l3ac_sosfilt_stream_state(int32_t sections) {
    L3AC_REQUIRE(sections >= 1 && sections <= IIR_MAX_SECTIONS, "sosfilt_stream_state: sections %d outside 1..%d", sections, IIR_MAX_SECTIONS);
    return 8 * (int64_t)sections;
}

int l3ac_sosfilt_stream(const double* state_in, double* state_out, int32_t streams, int64_t state_stride, const float* fresh, int64_t fresh_frames,
                        int64_t fresh_stride, const double* sos, int32_t sections, const l3ac_sosfilt_stream_desc* desc, int32_t count, void* out,
                        int64_t out_stride, int32_t out_f64, void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    SosCoef f;
    L3AC_TRY(sos_coef("sosfilt_stream", sos, sections, &f));
    L3AC_REQUIRE(desc && count > 0, "sosfilt_stream: no descriptors");
    L3AC_REQUIRE(streams > 0 && streams <= 65535 && count <= streams, "sosfilt_stream: %d descriptors for %d streams (1..65535)", count, streams);
    L3AC_REQUIRE(fresh_frames >= 0 && fresh_frames < ((int64_t)1 << 31), "sosfilt_stream: %lld new frames outside 0..2^31 - 1", (long long)fresh_frames);
    L3AC_REQUIRE(state_stride >= 8 * (int64_t)sections, "sosfilt_stream: state rows of %lld are below l3ac_sosfilt_stream_state = %d",
                 (long long)state_stride, 8 * sections);
    L3AC_REQUIRE(streams == 1 || (fresh_stride >= fresh_frames && out_stride >= fresh_frames),
                 "sosfilt_stream: row stride below the %lld new frames", (long long)fresh_frames);
    L3AC_REQUIRE(state_in && state_out, "sosfilt_stream: null state buffer");
    L3AC_REQUIRE(fresh_frames == 0 || (fresh && out), "sosfilt_stream: null buffer");
    const int64_t state_bytes = (int64_t)streams * state_stride * 8;
    L3AC_REQUIRE(iir_apart(state_in, state_bytes, state_out, state_bytes), "sosfilt_stream: the two state buffers overlap");
    std::vector<int> slots;
    for (int i = 0; i < count; ++i) {
        const l3ac_sosfilt_stream_desc& d = desc[i];
        L3AC_REQUIRE(d.slot >= 0 && d.slot < streams, "sosfilt_stream: descriptor %d: stream %d of %d", i, d.slot, streams);
        L3AC_REQUIRE(d.k >= 0 && d.k < IIR_SEG, "sosfilt_stream: descriptor %d: position %d outside [0, %d)", i, d.k, IIR_SEG);
        L3AC_REQUIRE(d.take >= 0 && d.take <= fresh_frames, "sosfilt_stream: descriptor %d takes %d of %lld new frames", i, d.take,
                     (long long)fresh_frames);
        L3AC_REQUIRE((d.flags & ~(L3AC_SOS_END | L3AC_SOS_FRESH)) == 0, "sosfilt_stream: descriptor %d: flags %d hold an unknown bit", i, d.flags);
        L3AC_REQUIRE(!(d.flags & L3AC_SOS_FRESH) || d.k == 0, "sosfilt_stream: descriptor %d: a fresh stream at position %d", i, d.k);
        slots.push_back(d.slot);
    }
    std::sort(slots.begin(), slots.end());
    L3AC_REQUIRE(std::adjacent_find(slots.begin(), slots.end()) == slots.end(), "sosfilt_stream: two descriptors for one stream");
    SosScratch sc;
    L3AC_TRY(sos_geom("sosfilt_stream", count, std::max<int64_t>(fresh_frames, 1), sections, &sc));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "sosfilt_stream", "sosfilt", nullptr, count, scratch, scratch_bytes, sc.total_min, &lens));
    char* base = static_cast<char*>(scratch);
    static_assert(sizeof(l3ac_sosfilt_stream_desc) == 16, "the descriptors are uploaded as four ints each");
    L3AC_TRY(launch_ragged_upload(s, reinterpret_cast<int*>(base + sc.desc), reinterpret_cast<const int*>(desc), 4 * count));
    SosRows r{};
    r.desc = reinterpret_cast<const int*>(base + sc.desc);
    r.state_in = state_in;
    r.state_out = state_out;
    r.state_stride = state_stride;
    r.max_samples = fresh_frames;
    r.segs_max = sc.segs_max;
    r.ends = reinterpret_cast<double*>(base + sc.ends);
    r.m = reinterpret_cast<const double*>(base + sc.m);
    return sos_run(s, fresh, fresh_stride, count, f, sections, r, out, out_stride, out_f64 != 0);
}

int64_t l3ac_butter_sos(int32_t order, double cutoff_hz, double sample_rate, int32_t highpass, double* out, int64_t cap) {
    L3AC_REQUIRE(order >= 1 && order <= IIR_MAX_ORDER, "butter_sos: order %d outside 1..%d", order, IIR_MAX_ORDER);
    L3AC_REQUIRE(std::isfinite(sample_rate) && sample_rate > 0.0, "butter_sos: sample_rate must be positive and finite");
    L3AC_REQUIRE(std::isfinite(cutoff_hz) && cutoff_hz > 0.0 && cutoff_hz < 0.5 * sample_rate,
                 "butter_sos: cutoff %.17g Hz outside (0, sample_rate / 2 = %.17g)", cutoff_hz, 0.5 * sample_rate);
    const int64_t sections = (order + 1) / 2, need = 6 * sections;
    if (!out || cap < need) return need;
    const double K = std::tan(M_PI * cutoff_hz / sample_rate);
    double* row = out;
    if (order % 2) {  // the first-order section first
        const double a0 = 1.0 + K;
        row[0] = (highpass ? 1.0 : K) / a0;
        row[1] = (highpass ? -1.0 : K) / a0;
        row[2] = 0.0;
        row[3] = 1.0;
        row[4] = (K - 1.0) / (K + 1.0);
        row[5] = 0.0;
        row += 6;
    }
    for (int k = 0; k < order / 2; ++k, row += 6) {
        const double q = 2.0 * std::sin(M_PI * (2 * k + 1) / (2.0 * order));
        const double a0 = 1.0 + q * K + K * K;
        row[0] = (highpass ? 1.0 : K * K) / a0;
        row[1] = (highpass ? -2.0 : 2.0 * K * K) / a0;
        row[2] = (highpass ? 1.0 : K * K) / a0;
        row[3] = 1.0;
        row[4] = 2.0 * (K * K - 1.0) / a0;
        row[5] = (1.0 - q * K + K * K) / a0;
    }
    return need;
}

}  // extern "C"
