// The magnitude-squared coherence of a pair of clips over the un-centred frames of lpc, per level class of the reference's frames, and the
// coherence speech intelligibility index built on it (include/l3ac_hip.h, "coherence"; DESIGN.md §3.23, which is normative).  No reference
// counterpart.  Four kernels, all fp64:
//
//   coh_energy_kernel  grid (frames / 4, batch), one wave a frame: E_t = sum_j (x_j w_j)^2 of the reference as 64 interleaved partials (j mod
//                      64) folded with fold64.
//   coh_class_kernel   one wave a pair: S = sum_t E_t (frame t in partial t mod 64, fold64), M = S / F, the class of every frame (0: E >= M,
//                      1: E >= 0.1 M, 2: E >= 0.001 M, 3: below; all 3 where S == 0) and the four counts.
//   coh_chunk_kernel   grid (chunks, batch), 4 waves.  A chunk is four groups of G consecutive frames of one pair, with G and the waves of a
//                      frame those of SpectralGeom (spectral_frames.hpp, shared with bands.hip: one wave a frame and G = 16 up to n_fft =
//                      256, the workgroup a frame above, G = 8 up to 1024, 4 at 2048, 2 at 4096).  A group's samples of both sides go to
//                      LDS once (stage_group of frame_groups.hpp, which owns the framing), the window once per chunk.  Per frame the two transforms of fft_f64.hpp, then per kept bin k the four products Pxx = Xr Xr + Xi Xi, Pyy,
//                      Cre = Xr Yr + Xi Yi, Cim = Xi Yr - Xr Yi through LDS; the thread that owns bin k adds them to its registers of the
//                      frame's class, the frames of the chunk in order.  The chunk's sums [4 classes][4][h] go to the scratch.
//   coh_finish_kernel  one workgroup a pair: the chunks in order; "all frames" = ((c0 + c1) + (c2 + c3)); g = min((Cre^2 + Cim^2) / (Sxx Syy),
//                      1), 0 where Sxx Syy == 0; with band weights, lane i the chains N_i, D_i of band i over its run of non-zero weights
//                      (band_runs) and T_i, thread 0 the class value in band order; then I3 and the intelligibility.
//
// A pair's values depend on its own samples only — never on the batch, the pair's row, the row strides, the scratch size, the grid or what
// lies at or after the clip's length, which is never read; no atomics.  Non-finite samples make unspecified values in their own pair only:
// every index and every loop is bounded by the parameters, whatever the values (a NaN energy compares false and lands in class 3).
//
// Contraction is off for this whole file: every product and sum rounds on its own, in the order DESIGN.md states.
#include "fft_f64.hpp"
#include "spectral_frames.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int CO_THREADS = 256;
constexpr int CO_GROUPS = 4;          // groups of a chunk
constexpr int CO_MAX_CHUNK = 64;
constexpr int CO_CLASSES = 4;
constexpr int CO_TABLE_BANDS = 21;

struct CohGeom : SpectralGeom {
    int chunk, bpt, lds_bytes;  // frames of a chunk, bins a thread, dynamic LDS of the launch
};

// a team's three arrays hold re, im and the first side's bins, after the products the four products; then the chunk's classes
constexpr int CO_LDS_MAX = spectral_lds_max<0, CO_MAX_CHUNK * 4>();

int coh_geom(const char* what, int32_t frame, int32_t hop, int32_t n_fft, CohGeom* p) {
    L3AC_TRY(spectral_geom(what, frame, hop, n_fft, p));
    p->chunk = CO_GROUPS * p->g;
    p->bpt = std::max(p->h / CO_THREADS, 1);
    p->lds_bytes = spectral_lds(n_fft, p->wpf, p->g, p->pitch, frame, 0, CO_MAX_CHUNK * 4);
    return L3AC_OK;
}

struct CohIo {
    const float* ref;
    int64_t ref_stride;
    const float* est;
    int64_t est_stride;
    int64_t max_samples;
    const int* lens;
    const float* window;
    const double* tw;          // [n_fft / 2][2]
    const double* weights;     // [bands][h] or nullptr: no band mapping
    const double* importance;  // [bands]
    int bands;
    int64_t f_max, chunks_max;
    double* energy;  // [batch][F]: NaN at and after a clip's own frames
    int* cls;        // [batch][F]
    int* cls_out;    // [batch][F] or nullptr: -1 at and after a clip's own frames
    int* counts;     // [batch][5]: frames, then the classes' frames
    double* part;    // [batch][chunks_max][4][4][h]
    double* sums;    // [batch][4][4][h]: per class Sxx, Syy, Sxy_re, Sxy_im
    // every output below may be nullptr
    double* msc;         // [batch][h]
    double* msc_levels;  // [batch][4][h]
    double* band_n;      // [batch][4][bands]: classes 0..2, then all frames
    double* band_d;
    double* band_t;
    double* out;  // [batch][6]: csii, high, mid, low, i3, intelligibility
};

__device__ __forceinline__ int64_t clip_frames(const CohIo& io, const CohGeom& p, int b) {
    const int64_t f = p.frames(io.lens ? io.lens[b] : io.max_samples);
    return f < io.f_max ? f : io.f_max;  // (the host checked the lengths; the clamp bounds every index)
}

// ---- the frame energies of the reference: grid (ceil(F / 4), batch), one wave a frame --------------------------------------------------------
__global__ __launch_bounds__(CO_THREADS) void coh_energy_kernel(CohIo io, CohGeom p) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * (CO_THREADS / 64) + (threadIdx.x >> 6);
    if (t >= io.f_max) return;  // (the whole wave)
    const int64_t frames = clip_frames(io, p, b);
    if (t >= frames) {
        if (lane == 0) io.energy[(int64_t)b * io.f_max + t] = __builtin_nan("");
        return;
    }
    const float* x = io.ref + (int64_t)b * io.ref_stride + t * p.hop;
    double s = 0.0;
    for (int j = lane; j < p.n; j += 64) {
        const double v = (double)x[j] * (io.window ? (double)io.window[j] : 1.0);
        s = s + v * v;
    }
    s = fold64(s);
    if (lane == 0) io.energy[(int64_t)b * io.f_max + t] = s;
}

// ---- the level classes: one wave a pair --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void coh_class_kernel(CohIo io, CohGeom p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int frames = (int)clip_frames(io, p, b);
    const double* e = io.energy + (int64_t)b * io.f_max;
    double s = 0.0;
    for (int t = lane; t < frames; t += 64) s = s + e[t];
    s = __shfl(fold64(s), 0, 64);
    const double mean = s / (double)frames;
    const double mid = 0.1 * mean, low = 0.001 * mean;
    int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
    for (int t = lane; t < (int)io.f_max; t += 64) {
        int c = -1;
        if (t < frames) {
            const double v = e[t];
            c = s == 0.0 ? 3 : (v >= mean ? 0 : (v >= mid ? 1 : (v >= low ? 2 : 3)));
            n0 += c == 0, n1 += c == 1, n2 += c == 2, n3 += c == 3;
        }
        io.cls[(int64_t)b * io.f_max + t] = c;
        if (io.cls_out) io.cls_out[(int64_t)b * io.f_max + t] = c;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        n0 += __shfl_xor(n0, o, 64), n1 += __shfl_xor(n1, o, 64), n2 += __shfl_xor(n2, o, 64), n3 += __shfl_xor(n3, o, 64);
    }
    if (lane == 0) {
        int* c = io.counts + (int64_t)b * 5;
        c[0] = frames, c[1] = n0, c[2] = n1, c[3] = n2, c[4] = n3;
    }
}

// ---- the cross-spectral sums of a chunk: grid (chunks, batch) ------------------------------------------------------------------------------
template <int BPT>
__global__ __launch_bounds__(CO_THREADS) void coh_chunk_kernel(CohIo io, CohGeom p) {
    extern __shared__ __attribute__((aligned(16))) double lds_raw[];
    const int tid = threadIdx.x;
    const int ts = 64 * p.wpf, teams = CO_THREADS / ts, team = tid / ts, tl = tid % ts;
    const int b = blockIdx.y;
    const int n_frame = p.n, nf = p.n_fft, h = p.h;
    double* zre = lds_raw + team * 3 * nf;  // [nf] each
    double* zim = zre + nf;
    double* q0 = zim + nf;                                          // the first side's re [h], im [h]
    int* cls_s = reinterpret_cast<int*>(lds_raw + teams * 3 * nf);  // [CO_MAX_CHUNK]
    float* win = reinterpret_cast<float*>(cls_s + CO_MAX_CHUNK);    // [n]
    float* xs0 = win + n_frame;                                     // [span_max]: frame k of the group starts at k pitch
    float* xs1 = xs0 + p.span_max();
    const int64_t frames = clip_frames(io, p, b);
    const int64_t c0 = (int64_t)blockIdx.x * p.chunk;
    if (c0 >= frames) return;  // (the whole workgroup: the finish reads the clip's own chunks only)

    double acc[BPT][CO_CLASSES][4];
#pragma unroll
    for (int i = 0; i < BPT; ++i)
#pragma unroll
        for (int c = 0; c < CO_CLASSES; ++c) acc[i][c][0] = acc[i][c][1] = acc[i][c][2] = acc[i][c][3] = 0.0;

    for (int i = tid; i < p.chunk; i += CO_THREADS) {
        const int c = c0 + i < frames ? io.cls[(int64_t)b * io.f_max + c0 + i] : 3;
        cls_s[i] = c < 0 ? 0 : (c > 3 ? 3 : c);
    }
    stage_window<CO_THREADS>(n_frame, io.window, win);

    for (int sg = 0; sg < CO_GROUPS; ++sg) {
        const int64_t t0 = c0 + (int64_t)sg * p.g;
        if (t0 >= frames) break;  // (uniform)
        const int cnt = p.count(t0, frames);
        // (the previous group's frames are done with the stage: their last step ended with a barrier)
        stage_group<CO_THREADS>(p, t0, cnt, io.ref + (int64_t)b * io.ref_stride, io.est + (int64_t)b * io.est_stride, xs0, xs1);
        __syncthreads();

        for (int k0 = 0; k0 < cnt; k0 += teams) {  // the teams in step: every barrier below is reached by all of them
            const int k = k0 + team;
            const bool active = k < cnt;
            for (int side = 0; side < 2; ++side) {
                const float* x = (side ? xs1 : xs0) + (active ? k : 0) * p.pitch;
                fft_f64_load(zre, zim, x, win, n_frame, nf, p.log2n, tl, ts);
                fft_f64_passes(zre, zim, io.tw, nf, p.log2n, tl, ts);
                if (side == 0) {
                    for (int kk = tl; kk < h; kk += ts) q0[kk] = zre[swz(kk)], q0[h + kk] = zim[swz(kk)];
                    __syncthreads();  // (the second side's load overwrites re and im)
                }
            }
            // the four products of bin kk: Pxx, Pyy to the first side's array, Cre, Cim to the upper halves of re and im, which the bins
            // at and above Nyquist have left (the elements below h stay below h under swz: h is below 32 or a multiple of 32)
            for (int kk = tl; kk < h; kk += ts) {
                const double xr = q0[kk], xi = q0[h + kk], yr = zre[swz(kk)], yi = zim[swz(kk)];
                q0[kk] = xr * xr + xi * xi;
                q0[h + kk] = yr * yr + yi * yi;
                zre[h + kk] = xr * yr + xi * yi;
                zim[h + kk] = xi * yr - xr * yi;
            }
            __syncthreads();
            // the owner of a bin adds the step's frames in order
            for (int j = 0; j < teams && k0 + j < cnt; ++j) {
                const double* z = lds_raw + j * 3 * nf;
                const int c = cls_s[(int)(t0 - c0) + k0 + j];
#pragma unroll
                for (int i = 0; i < BPT; ++i) {
                    const int kk = tid + i * CO_THREADS;
                    if (kk < h) {
                        const double v0 = z[2 * nf + kk], v1 = z[2 * nf + h + kk], v2 = z[h + kk], v3 = z[nf + h + kk];
#pragma unroll
                        for (int cc = 0; cc < CO_CLASSES; ++cc)
                            if (c == cc) {
                                acc[i][cc][0] = acc[i][cc][0] + v0, acc[i][cc][1] = acc[i][cc][1] + v1;
                                acc[i][cc][2] = acc[i][cc][2] + v2, acc[i][cc][3] = acc[i][cc][3] + v3;
                            }
                    }
                }
            }
            __syncthreads();  // the products are read before the next frame overwrites them
        }
    }
    double* out = io.part + ((int64_t)b * io.chunks_max + blockIdx.x) * 16 * h;
#pragma unroll
    for (int i = 0; i < BPT; ++i) {
        const int kk = tid + i * CO_THREADS;
        if (kk < h) {
#pragma unroll
            for (int c = 0; c < CO_CLASSES; ++c)
#pragma unroll
                for (int v = 0; v < 4; ++v) out[(c * 4 + v) * h + kk] = acc[i][c][v];
        }
    }
}

// ---- the pair: one workgroup a pair ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(CO_THREADS) void coh_finish_kernel(CohIo io, CohGeom p) {
    __shared__ double sig[SP_MAX_FFT / 2], dis[SP_MAX_FFT / 2];  // g Syy and (1 - g) Syy of the row in hand
    __shared__ double tv[SP_MAX_BANDS], vals[4];
    __shared__ int runs[2 * SP_MAX_BANDS];  // band i's non-zero weights are [lo, hi)
    const int b = blockIdx.x, tid = threadIdx.x, h = p.h, nb = io.bands;
    const int* counts = io.counts + (int64_t)b * 5;
    const int frames = counts[0];
    const int chunks = (frames + p.chunk - 1) / p.chunk;
    const double nan = __builtin_nan("");
    double* sums = io.sums + (int64_t)b * 16 * h;
    const double* part = io.part + (int64_t)b * io.chunks_max * 16 * h;
    for (int k = tid; k < h; k += CO_THREADS)
        for (int cv = 0; cv < 16; ++cv) {
            double s = 0.0;
            for (int c = 0; c < chunks; ++c) s = s + part[((int64_t)c * 16 + cv) * h + k];
            sums[cv * h + k] = s;
        }
    band_runs(io.weights, nb, h, runs);
    __syncthreads();

    for (int r = 0; r < 5; ++r) {  // the classes 0..3, then all frames
        const int count = r < 4 ? counts[1 + r] : frames;
        for (int k = tid; k < h; k += CO_THREADS) {  // (the thread that wrote sums[..][k] reads it)
            double v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q)
                v[q] = r < 4 ? sums[(r * 4 + q) * h + k]
                             : ((sums[q * h + k] + sums[(4 + q) * h + k]) + (sums[(8 + q) * h + k] + sums[(12 + q) * h + k]));
            const double den = v[0] * v[1];
            const double ratio = (v[2] * v[2] + v[3] * v[3]) / den;
            const double g = den == 0.0 ? 0.0 : (ratio > 1.0 ? 1.0 : ratio);
            double* dst = r < 4 ? (io.msc_levels ? io.msc_levels + ((int64_t)b * 4 + r) * h : nullptr) : (io.msc ? io.msc + (int64_t)b * h : nullptr);
            if (dst) dst[k] = count < 2 ? nan : g;
            sig[k] = g * v[1], dis[k] = (1.0 - g) * v[1];
        }
        __syncthreads();
        if (!io.weights || r == 3) continue;  // (uniform; the next row's writes come after its own barrier below or this one)
        const int row = r < 3 ? r : 3;
        if (tid < nb) {
            const double* wrow = io.weights + (int64_t)tid * h;
            const int lo = runs[2 * tid], hi = runs[2 * tid + 1];
            double n_i = 0.0, d_i = 0.0;
            for (int k = lo; k < hi; ++k) n_i = n_i + wrow[k] * sig[k], d_i = d_i + wrow[k] * dis[k];
            double t_i;
            if (n_i == 0.0) {
                t_i = 0.0;
            } else if (d_i == 0.0 && n_i > 0.0) {
                t_i = 1.0;
            } else {
                t_i = (clamp_to(10.0 * log10(n_i / d_i), -15.0, 15.0) + 15.0) / 30.0;
            }
            tv[tid] = t_i;
            const int64_t at = ((int64_t)b * 4 + row) * nb + tid;
            if (io.band_n) io.band_n[at] = n_i;
            if (io.band_d) io.band_d[at] = d_i;
            if (io.band_t) io.band_t[at] = t_i;
        }
        __syncthreads();
        if (tid == 0) {
            double num = 0.0, den = 0.0;
            for (int i = 0; i < nb; ++i) num = num + io.importance[i] * tv[i], den = den + io.importance[i];
            vals[row] = count < 2 ? nan : num / den;
        }
        __syncthreads();  // sig, dis and tv are read before the next row overwrites them
    }
    if (io.out && io.weights && tid == 0) {
        const double i3 = (-3.47 + 1.84 * vals[2]) + 9.99 * vals[1];
        double* o = io.out + (int64_t)b * 6;
        o[0] = vals[3], o[1] = vals[0], o[2] = vals[1], o[3] = vals[2], o[4] = i3, o[5] = 1.0 / (1.0 + exp(-i3));
    }
}

template <int BPT>
int launch_chunks(hipStream_t s, const CohIo& io, const CohGeom& p, int32_t batch) {
    static PerDeviceOnce configured;
    L3AC_TRY(raise_dynamic_lds(configured, {{coh_chunk_kernel<BPT>, CO_LDS_MAX}}));
    ProfScope prof(s, "coh_chunk_kernel", 2.0 * batch * (double)io.f_max * 5.0 * p.n_fft * p.log2n, 8.0 * batch * (double)io.max_samples);
    hipLaunchKernelGGL(coh_chunk_kernel<BPT>, dim3((unsigned)io.chunks_max, (unsigned)batch), dim3(CO_THREADS), (size_t)p.lds_bytes, s, io, p);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

struct CohScratch {  // byte offsets into the caller's scratch, after the clips' lengths
    int64_t energy, cls, counts, sums, part, need;
};

// the parameters checked, then the frames' energies [batch][F] fp64 and classes [batch][F] int32, the counts [batch][5] int32, the class
// sums [batch][16][h] fp64 and the chunks' sums [batch][ceil(F / chunk)][16][h] fp64
int coh_scratch(const char* what, int32_t batch, int64_t max_samples, int32_t frame, int32_t hop, int32_t n_fft, CohGeom* p, CohScratch* sc) {
    L3AC_TRY(coh_geom(what, frame, hop, n_fft, p));
    L3AC_TRY(check_clip_batch(what, batch, max_samples));
    const int64_t f_max = p->frames(max_samples);
    ScratchPlan plan(batch);
    L3AC_TRY(pair_frames_plan(what, batch, f_max, 0, plan, nullptr, nullptr));  // (the check alone: a pair's frames are capped as band_metrics')
    sc->energy = plan.take((int64_t)batch * f_max * 8);
    sc->cls = plan.take((int64_t)batch * f_max * 4);
    sc->counts = plan.take((int64_t)batch * 5 * 4);
    sc->sums = plan.take((int64_t)batch * 16 * p->h * 8);
    sc->part = plan.take((int64_t)batch * ceil_div64(f_max, p->chunk) * 16 * p->h * 8);
    sc->need = plan.bytes;
    return L3AC_OK;
}

// the checks the two entries share, then the four launches; io holds the entry's own outputs and tables
int coh_run(const char* what, hipStream_t s, CohIo io, const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch,
            int64_t max_samples, const int32_t* samples, int32_t frame, int32_t hop, int32_t n_fft, const float* window, const double* twiddles,
            double* sums, int32_t* counts, int32_t* frame_class, double* frame_energy, void* scratch, int64_t scratch_bytes) {
    CohGeom p;
    CohScratch sc;
    L3AC_TRY(coh_scratch(what, batch, max_samples, frame, hop, n_fft, &p, &sc));
    L3AC_REQUIRE(ref && est, "%s: null audio", what);
    L3AC_REQUIRE(twiddles, "%s: null twiddles", what);
    L3AC_REQUIRE(((uintptr_t)ref & 3) == 0 && ((uintptr_t)est & 3) == 0 && ((uintptr_t)window & 3) == 0, "%s: audio and window must be 4-byte aligned",
                 what);
    L3AC_REQUIRE(((uintptr_t)twiddles & 7) == 0 && ((uintptr_t)io.weights & 7) == 0 && ((uintptr_t)io.importance & 7) == 0 &&
                     ((uintptr_t)sums & 7) == 0 && ((uintptr_t)frame_energy & 7) == 0 && ((uintptr_t)io.msc & 7) == 0 &&
                     ((uintptr_t)io.msc_levels & 7) == 0 && ((uintptr_t)io.band_n & 7) == 0 && ((uintptr_t)io.band_d & 7) == 0 &&
                     ((uintptr_t)io.band_t & 7) == 0 && ((uintptr_t)io.out & 7) == 0,
                 "%s: fp64 buffers must be 8-byte aligned", what);
    L3AC_REQUIRE(((uintptr_t)counts & 3) == 0 && ((uintptr_t)frame_class & 3) == 0, "%s: int32 buffers must be 4-byte aligned", what);
    L3AC_REQUIRE(batch == 1 || (ref_stride >= max_samples && est_stride >= max_samples), "%s: row stride below max_samples %lld", what,
                 (long long)max_samples);
    L3AC_TRY(check_clip_lengths(what, samples, batch, max_samples));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, what, "coherence", samples, batch, scratch, scratch_bytes, sc.need, &lens));
    char* base = static_cast<char*>(scratch);
    io.ref = ref, io.ref_stride = ref_stride, io.est = est, io.est_stride = est_stride, io.max_samples = max_samples, io.lens = lens;
    io.window = window, io.tw = twiddles;
    io.f_max = p.frames(max_samples),io.chunks_max = ceil_div64(io.f_max, p.chunk);
    io.energy = frame_energy ? frame_energy : reinterpret_cast<double*>(base + sc.energy);
    io.cls = reinterpret_cast<int*>(base + sc.cls), io.cls_out = frame_class;
    io.counts = counts ? counts : reinterpret_cast<int*>(base + sc.counts);
    io.sums = sums ? sums : reinterpret_cast<double*>(base + sc.sums);
    io.part = reinterpret_cast<double*>(base + sc.part);
    if (io.f_max > 0) {
        ProfScope prof(s, "coh_energy_kernel", 3.0 * batch * (double)io.f_max * p.n, 4.0 * batch * (double)io.max_samples);
        hipLaunchKernelGGL(coh_energy_kernel, dim3((unsigned)ceil_div64(io.f_max, CO_THREADS / 64), (unsigned)batch), dim3(CO_THREADS), 0, s, io, p);
        L3AC_LAUNCH_CHECK();
    }
    {
        ProfScope prof(s, "coh_class_kernel", 0.0, 12.0 * batch * (double)io.f_max);
        hipLaunchKernelGGL(coh_class_kernel, dim3((unsigned)batch), dim3(64), 0, s, io, p);
        L3AC_LAUNCH_CHECK();
    }
    if (io.f_max > 0) {
        switch (p.bpt) {
            case 1: L3AC_TRY(launch_chunks<1>(s, io, p, batch)); break;
            case 2: L3AC_TRY(launch_chunks<2>(s, io, p, batch)); break;
            case 4: L3AC_TRY(launch_chunks<4>(s, io, p, batch)); break;
            default: L3AC_TRY(launch_chunks<8>(s, io, p, batch)); break;
        }
    }
    ProfScope prof(s, "coh_finish_kernel", 0.0, 128.0 * batch * (double)(io.chunks_max + 1) * p.h);
    hipLaunchKernelGGL(coh_finish_kernel, dim3((unsigned)batch), dim3(CO_THREADS), 0, s, io, p);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

// the critical-band procedure of ANSI S3.5-1997: centre frequencies, lower band edges (the last entry: the last upper edge) and the band
// importance function
const double SII_CENTRE[CO_TABLE_BANDS] = {150.0,  250.0,  350.0,  450.0,  570.0,  700.0,  840.0,  1000.0, 1170.0, 1370.0, 1600.0,
                                           1850.0, 2150.0, 2500.0, 2900.0, 3400.0, 4000.0, 4800.0, 5800.0, 7000.0, 8500.0};
const double SII_EDGE[CO_TABLE_BANDS + 1] = {100.0,  200.0,  300.0,  400.0,  510.0,  630.0,  770.0,  920.0,  1080.0, 1270.0, 1480.0,
                                             1720.0, 2000.0, 2320.0, 2700.0, 3150.0, 3700.0, 4400.0, 5300.0, 6400.0, 7700.0, 9500.0};
const double SII_IMPORTANCE[CO_TABLE_BANDS] = {0.0103, 0.0261, 0.0419, 0.0577, 0.0577, 0.0577, 0.0577, 0.0577, 0.0577, 0.0577, 0.0577,
                                               0.0577, 0.0577, 0.0577, 0.0577, 0.0577, 0.0577, 0.0460, 0.0343, 0.0226, 0.0110};

}  // namespace

extern "C" {

int64_t l3ac_sii_bands(double* out, int64_t cap) {
    if (!out || cap < 3 * CO_TABLE_BANDS) return 3 * CO_TABLE_BANDS;
    for (int i = 0; i < CO_TABLE_BANDS; ++i) {
        out[i] = SII_CENTRE[i], out[CO_TABLE_BANDS + i] = SII_EDGE[i + 1] - SII_EDGE[i], out[2 * CO_TABLE_BANDS + i] = SII_IMPORTANCE[i];
    }
    return 3 * CO_TABLE_BANDS;
}

int64_t l3ac_coherence_scratch_bytes(int32_t batch, int64_t max_samples, int32_t frame, int32_t hop, int32_t n_fft) {
    CohGeom p;
    CohScratch sc;
    L3AC_TRY(coh_scratch("coherence", batch, max_samples, frame, hop, n_fft, &p, &sc));
    return sc.need;
}

int l3ac_coherence(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples,
                   const int32_t* samples, int32_t frame, int32_t hop, int32_t n_fft, const float* window, const double* twiddles, double* msc,
                   double* msc_levels, double* sums, int32_t* counts, int32_t* frame_class, double* frame_energy, void* scratch,
                   int64_t scratch_bytes, void* stream) {
    CohIo io{};
    io.msc = msc, io.msc_levels = msc_levels;
    return coh_run("coherence", (hipStream_t)stream, io, ref, ref_stride, est, est_stride, batch, max_samples, samples, frame, hop, n_fft, window,
                   twiddles, sums, counts, frame_class, frame_energy, scratch, scratch_bytes);
}

int l3ac_csii(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples, const int32_t* samples,
              int32_t frame, int32_t hop, int32_t n_fft, const float* window, const double* twiddles, const double* weights,
              const double* importance, int32_t bands, double* out, int32_t* counts, double* band_signal, double* band_distortion,
              double* band_value, double* sums, void* scratch, int64_t scratch_bytes, void* stream) {
    L3AC_REQUIRE(bands >= SP_MIN_BANDS && bands <= SP_MAX_BANDS, "csii: %d bands outside %d..%d", bands, SP_MIN_BANDS, SP_MAX_BANDS);
    L3AC_REQUIRE(weights && importance, "csii: null weights or importance");
    L3AC_REQUIRE(out, "csii: null output buffer");
    CohIo io{};
    io.weights = weights, io.importance = importance, io.bands = bands;
    io.band_n = band_signal, io.band_d = band_distortion, io.band_t = band_value, io.out = out;
    return coh_run("csii", (hipStream_t)stream, io, ref, ref_stride, est, est_stride, batch, max_samples, samples, frame, hop, n_fft, window, twiddles,
                   sums, counts, nullptr, nullptr, scratch, scratch_bytes);
}

}  // extern "C"
