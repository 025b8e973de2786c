// Speech intelligibility on the device: STOI (Taal et al. 2011) and ESTOI (Jensen & Taal 2016) of clip pairs at 10 kHz
// (include/l3ac_hip.h, "speech intelligibility").  No reference counterpart.
//
// A clip of L samples has F = A(L) analysis frames of 256 samples at hop 128 (frame f starts at 128 f < L - 256).  The chain, per call:
//   stoi_energy_kernel   one wave per analysis frame of the REFERENCE: v_f = 20 log10(sqrt(sum_j (w[j] x[128 f + j])^2) + eps) in fp64
//   stoi_select_kernel   one workgroup per clip: max_f v_f, then the frames with v_f > max - 40 in passes of 256 frames, a ballot scan
//                        inside each wave, the waves' counts through LDS and a carried offset: the kept-frame list f_0 < f_1 < ... and
//                        K.  No atomics, nothing global.  K lives on the device only.
//   stoi_ola_kernel      both signals rebuilt from the kept frames by overlap-add, straight into staged rows [2][batch][pitch]: sample
//                        i gathers its at most two terms w[j] x[128 f_q + j] (q = i / 128 - 1, then q = i / 128), zero at or after
//                        128 (K - 1) + 256.  pitch = 128 (A(max) + 1) is sized for K = F.
//   launch_gemm          the spectra: the staged rows read as overlapping GEMM rows (lda = 128, k = 256) against the window-folded
//                        basis [514][256], exactly as metrics.hip does; slot row g = clip * (pitch / 128) + t is frame t of that clip.
//                        Slot rows at or after a clip's T = K - 1 frames hold finite values and are never consumed.
//   stoi_bands_kernel    one wave per slot row: power fma(re, re, im im), one fp32 sum per third-octave band over its run of bins in
//                        increasing k from +0, the square root correctly rounded -> bands [2][batch][A(max) - 1][16], zero for t >= T.
//   stoi_segment_kernel  one wave per (clip, m): the two 15 x 30 blocks of frames m - 30 .. m - 1 in registers (lane = frame, 15 bands
//                        per lane), both d_m in fp64: sums over frames are xor trees, sums over bands run in the lane.
//   stoi_mean_kernel     one workgroup per clip: the d_m summed in a fixed order; the sentinel 1e-5 when T < 30.
// Nothing depends on the batch, the clip's row, the row strides or the group of slot rows one product takes.
#include "metric_common.hpp"

#include <algorithm>
#include <cmath>

// the spec's arithmetic is written out operation by operation: a fused multiply-add only where fma() / fmaf() says so
#pragma clang fp contract(off)

namespace {

constexpr int ST_THREADS = 256;
constexpr int ST_FRAME = 256, ST_HOP = 128, ST_NFFT = 512, ST_BANDS = 15, ST_SEG = 30;
constexpr int ST_BASIS_ROWS = ST_NFFT + 2;  // 514: re and im of bins 0 .. 256
constexpr int ST_SPEC_LD = ST_NFFT + 4;     // 516: 16-byte rows
constexpr int ST_MIN_GROUP = 128;           // slot rows per product at the minimum scratch: one GEMM row panel
constexpr int ST_BAND_LD = 16;              // 15 cells padded to a 64-byte row
constexpr double ST_EPS = 2.220446049250313e-16;  // 2^-52
constexpr double ST_RANGE_DB = 40.0;
constexpr double ST_SENTINEL = 1e-5;

struct StoiGeom {
    int batch;
    int f_max, t_max, seg_max;  // A(max_samples); spectral frames A(max) - 1 and segments t_max - 29 of a clip that keeps every frame
    int64_t max_samples;
    int64_t pitch, slots, rows;  // staged row (floats), pitch / 128, slot rows that hold a spectral frame of some clip
};

struct StoiScratch {  // byte offsets into the caller's scratch, after the clips' lengths
    int64_t runs, kcount, level, kept, stage, bands, dseg, spec, total_min;
};

__host__ __device__ inline int64_t st_frames(int64_t n) { return n <= ST_FRAME ? 0 : (n - ST_FRAME + ST_HOP - 1) / ST_HOP; }

int stoi_geom(int32_t batch, int64_t max_samples, StoiGeom* g, StoiScratch* sc) {
    L3AC_REQUIRE(batch > 0 && batch <= 65535 && max_samples > 0, "stoi: batch %d outside 1..65535 or no samples (%lld)", batch,
                 (long long)max_samples);
    L3AC_REQUIRE(max_samples < ((int64_t)1 << 31) - 4096, "stoi: clips of %lld samples are too long", (long long)max_samples);
    g->batch = batch;
    g->max_samples = max_samples;
    g->f_max = (int)st_frames(max_samples);
    g->t_max = std::max(g->f_max - 1, 0);
    g->seg_max = std::max(g->t_max - (ST_SEG - 1), 0);
    // K kept frames rebuild 128 (K - 1) + 256 samples; K <= f_max
    g->pitch = (int64_t)ST_HOP * (std::max(g->f_max, 1) + 1);
    g->slots = g->pitch / ST_HOP;
    g->rows = g->t_max ? (int64_t)(batch - 1) * g->slots + g->t_max : 0;
    L3AC_REQUIRE(g->rows < ((int64_t)1 << 31), "stoi: %lld frame rows in one call (batch %d) exceed 2^31", (long long)g->rows, batch);
    ScratchPlan plan(batch);
    sc->runs = plan.take(2 * ST_BANDS * 4);
    sc->kcount = plan.take((int64_t)batch * 4);
    sc->level = plan.take((int64_t)batch * g->f_max * 8);
    sc->kept = plan.take((int64_t)batch * g->f_max * 4);
    sc->stage = plan.take(2 * (int64_t)batch * g->pitch * 4);
    sc->bands = plan.take(2 * (int64_t)batch * g->t_max * ST_BAND_LD * 4);
    sc->dseg = plan.take((int64_t)batch * g->seg_max * 2 * 8);
    sc->spec = plan.last(2 * std::min<int64_t>(ST_MIN_GROUP, g->rows) * ST_SPEC_LD * 4);
    sc->total_min = plan.bytes;
    return L3AC_OK;
}

__device__ __forceinline__ int64_t clip_len(const int* __restrict__ lens, int b, const StoiGeom& g) { return lens ? lens[b] : g.max_samples; }

// ---- reference frame levels: grid (frames / 4, batch), one wave per analysis frame, four samples per lane ---------------------------------
__global__ __launch_bounds__(ST_THREADS) void stoi_energy_kernel(const float* __restrict__ ref, int64_t ref_stride, const int* __restrict__ lens,
                                                               const float* __restrict__ window, double* __restrict__ level, StoiGeom g) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.y;
    const int f = __builtin_amdgcn_readfirstlane(blockIdx.x * (ST_THREADS / 64) + (threadIdx.x >> 6));
    if (f >= st_frames(clip_len(lens, b, g))) return;  // (wave-uniform)
    const float* x = ref + (int64_t)b * ref_stride + (int64_t)f * ST_HOP + 4 * lane;  // 128 f + 255 < L: the clip's own samples
    const float4 w = *reinterpret_cast<const float4*>(window + 4 * lane);
    const float wj[4] = {w.x, w.y, w.z, w.w};
    double e = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double p = (double)wj[j] * (double)x[j];  // exact: 24 x 24 bits
        e = fma(p, p, e);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) e += __shfl_xor(e, o, 64);
    if (lane == 0) level[(int64_t)b * g.f_max + f] = 20.0 * log10(sqrt(e) + ST_EPS);
}

// ---- which frames stay: one workgroup per clip ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ST_THREADS) void stoi_select_kernel(const double* __restrict__ level, const int* __restrict__ lens, int* __restrict__ kept,
                                                               int* __restrict__ kcount, int* __restrict__ frames_out, StoiGeom g) {
    __shared__ double wmax[ST_THREADS / 64];
    __shared__ int wcnt[ST_THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.x;
    const int frames = (int)st_frames(clip_len(lens, b, g));
    const double* v = level + (int64_t)b * g.f_max;
    int* list = kept + (int64_t)b * g.f_max;
    double mx = -INFINITY;  // (a maximum does not depend on the order it is taken in)
    for (int f = threadIdx.x; f < frames; f += ST_THREADS) mx = fmax(mx, v[f]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    if (lane == 0) wmax[wave] = mx;
    __syncthreads();
    mx = fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3]));
    const double threshold = mx - ST_RANGE_DB;
    int base = 0;  // frames kept before this pass
    for (int f0 = 0; f0 < frames; f0 += ST_THREADS) {
        const int f = f0 + threadIdx.x;
        const bool keep = f < frames && v[f] > threshold;
        const unsigned long long mask = __ballot(keep);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        __syncthreads();  // the previous pass has read wcnt
        if (lane == 0) wcnt[wave] = __popcll(mask);
        __syncthreads();
        int off = base, total = 0;
#pragma unroll
        for (int w = 0; w < ST_THREADS / 64; ++w) {
            if (w < wave) off += wcnt[w];
            total += wcnt[w];
        }
        if (keep) list[off + before] = f;  // off + before < kept so far <= frames <= f_max
        base += total;
    }
    if (threadIdx.x == 0) {
        kcount[b] = base;
        frames_out[b] = base > 0 ? base - 1 : 0;
    }
}

// ---- overlap-add of the kept frames into staged rows: grid (quads of a row / 256, batch, 2) -----------------------------------------------
__global__ __launch_bounds__(ST_THREADS) void stoi_ola_kernel(const float* __restrict__ x0, int64_t stride0, const float* __restrict__ x1, int64_t stride1,
                                                            const float* __restrict__ window, const int* __restrict__ kept,
                                                            const int* __restrict__ kcount, float* __restrict__ stage, StoiGeom g) {
    const int b = blockIdx.y;
    const int64_t q4 = (int64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (4 * q4 >= g.pitch) return;  // (pitch is a multiple of 128)
    const float* x = (blockIdx.z ? x1 : x0) + (int64_t)b * (blockIdx.z ? stride1 : stride0);
    const int* list = kept + (int64_t)b * g.f_max;
    const int k = kcount[b];
    const int64_t i0 = 4 * q4;
    const int q = (int)(i0 / ST_HOP), j = (int)(i0 % ST_HOP);  // the quad lies inside one hop
    // sample 128 q + j: frame q - 1 at offset j + 128 first, then frame q at offset j; K frames cover [0, 128 (K + 1))
    const bool first = q >= 1 && q - 1 < k, second = q < k;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (first) {
        const float* src = x + (int64_t)list[q - 1] * ST_HOP + ST_HOP + j;
        const float4 w = *reinterpret_cast<const float4*>(window + ST_HOP + j);
        v[0] = w.x * src[0];
        v[1] = w.y * src[1];
        v[2] = w.z * src[2];
        v[3] = w.w * src[3];
    }
    if (second) {
        const float* src = x + (int64_t)list[q] * ST_HOP + j;
        const float4 w = *reinterpret_cast<const float4*>(window + j);
        v[0] = v[0] + w.x * src[0];
        v[1] = v[1] + w.y * src[1];
        v[2] = v[2] + w.z * src[2];
        v[3] = v[3] + w.w * src[3];
    }
    *reinterpret_cast<float4*>(stage + ((int64_t)blockIdx.z * g.batch + b) * g.pitch + i0) = make_float4(v[0], v[1], v[2], v[3]);
}

// ---- spectra of a group -> third-octave bands: one wave per slot row, four rows per workgroup -----------------------------------------------
constexpr int SB_ROWS = 4;
constexpr int SB_PMAX = 260;  // bins 0 .. 256 and the padding of the 516-float row

__global__ __launch_bounds__(ST_THREADS) void stoi_bands_kernel(const float* __restrict__ spec0, const float* __restrict__ spec1, int64_t row0, int count,
                                                              const int* __restrict__ kcount, const int* __restrict__ runs,
                                                              float* __restrict__ bands, float* __restrict__ bands_out, StoiGeom g) {
    __shared__ __attribute__((aligned(16))) float pw[2][SB_ROWS][SB_PMAX];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = blockIdx.x * SB_ROWS + wave;
    const int64_t row = row0 + r;
    const int clip = (int)((uint32_t)row / (uint32_t)g.slots);
    const int t = (int)((uint32_t)row % (uint32_t)g.slots);
    const bool cell = r < count && clip < g.batch && t < g.t_max;  // a row of the output (wave-uniform)
    const bool valid = cell && t < kcount[clip] - 1;               // and one of the clip's own T frames
    if (valid) {
        for (int s = 0; s < 2; ++s) {
            const float4* src = reinterpret_cast<const float4*>((s ? spec1 : spec0) + (int64_t)r * ST_SPEC_LD);
            for (int q = lane; q < ST_SPEC_LD / 4; q += 64) {
                const float4 v = src[q];  // two bins; the last quad's second half is the row's padding, never used
                *reinterpret_cast<float2*>(&pw[s][wave][2 * q]) = make_float2(fmaf(v.x, v.x, v.y * v.y), fmaf(v.z, v.z, v.w * v.w));
            }
        }
    }
    __syncthreads();
    if (!cell || lane >= 2 * ST_BAND_LD) return;
    const int sig = lane >> 4, band = lane & 15;
    float val = 0.f;
    if (valid && band < ST_BANDS) {
        const int lo = runs[band], hi = runs[ST_BANDS + band];
        float acc = 0.f;
        for (int k = lo; k < hi; ++k) acc = acc + pw[sig][wave][k];
        val = (float)sqrt((double)acc);  // the fp64 root rounded to fp32 is the correctly rounded fp32 root (53 >= 2 * 24 + 2)
    }
    const int64_t at = ((int64_t)sig * g.batch + clip) * g.t_max + t;
    bands[at * ST_BAND_LD + band] = val;
    if (bands_out && band < ST_BANDS) bands_out[at * ST_BANDS + band] = val;
}

// ---- d_m of both measures: grid (segments / 4, batch), one wave per (clip, m) -----------------------------------------------------------------
// lane & 31 = frame n of the segment (30 and 31 hold zeros; the upper half of the wave repeats the lower one), 15 bands per lane.
__device__ __forceinline__ double over_frames(double v) {
#pragma unroll
    for (int o = 16; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ void load_bands(const float* __restrict__ p, double* v) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 c = reinterpret_cast<const float4*>(p)[q];
        v[4 * q] = c.x;
        v[4 * q + 1] = c.y;
        v[4 * q + 2] = c.z;
        if (q < 3) v[4 * q + 3] = c.w;
    }
}

__global__ __launch_bounds__(ST_THREADS) void stoi_segment_kernel(const float* __restrict__ bands, const int* __restrict__ kcount, double* __restrict__ dseg,
                                                                double clip_gain, StoiGeom g) {
    const int lane = threadIdx.x & 63;
    const int clip = blockIdx.y;
    const int seg = __builtin_amdgcn_readfirstlane(blockIdx.x * (ST_THREADS / 64) + (threadIdx.x >> 6));
    const int t_clip = kcount[clip] - 1;
    if (seg >= t_clip - (ST_SEG - 1)) return;  // (wave-uniform; no barrier below)
    const int n = lane & 31;
    const bool act = n < ST_SEG;
    double x[ST_BANDS], y[ST_BANDS];
#pragma unroll
    for (int i = 0; i < ST_BANDS; ++i) x[i] = y[i] = 0.0;
    if (act) {  // frame seg + n <= T - 1
        load_bands(bands + (((int64_t)clip) * g.t_max + seg + n) * ST_BAND_LD, x);
        load_bands(bands + (((int64_t)g.batch + clip) * g.t_max + seg + n) * ST_BAND_LD, y);
    }
    double dot = 0.0;
#pragma unroll
    for (int i = 0; i < ST_BANDS; ++i) {
        const double nx = sqrt(over_frames(x[i] * x[i])), ny = sqrt(over_frames(y[i] * y[i]));
        const double yp = fmin(nx / (ny + ST_EPS) * y[i], clip_gain * x[i]);
        const double mx = over_frames(x[i]) / ST_SEG, my = over_frames(y[i]) / ST_SEG, mp = over_frames(yp) / ST_SEG;
        const double xc = act ? x[i] - mx : 0.0, yc = act ? y[i] - my : 0.0, pc = act ? yp - mp : 0.0;
        const double xn = xc / (sqrt(over_frames(xc * xc)) + ST_EPS);
        const double pn = pc / (sqrt(over_frames(pc * pc)) + ST_EPS);
        dot += xn * pn;
        x[i] = xn;  // the row-normalised blocks: ESTOI's first step
        y[i] = yc / (sqrt(over_frames(yc * yc)) + ST_EPS);
    }
    const double d_stoi = over_frames(dot) / ST_BANDS;
    // ESTOI: each column (this lane's frame over the 15 bands) centred and normalised
    double sx = 0.0, sy = 0.0;
#pragma unroll
    for (int i = 0; i < ST_BANDS; ++i) {
        sx += x[i];
        sy += y[i];
    }
    sx /= ST_BANDS;
    sy /= ST_BANDS;
    double qx = 0.0, qy = 0.0;
#pragma unroll
    for (int i = 0; i < ST_BANDS; ++i) {
        x[i] -= sx;
        y[i] -= sy;
        qx += x[i] * x[i];
        qy += y[i] * y[i];
    }
    qx = sqrt(qx) + ST_EPS;
    qy = sqrt(qy) + ST_EPS;
    double col = 0.0;
#pragma unroll
    for (int i = 0; i < ST_BANDS; ++i) col += (x[i] / qx) * (y[i] / qy);
    const double d_estoi = over_frames(col) / ST_SEG;  // (lanes 30 and 31 hold zero columns)
    if (lane == 0) {
        double* d = dseg + ((int64_t)clip * g.seg_max + seg) * 2;
        d[0] = d_stoi;
        d[1] = d_estoi;
    }
}

// ---- a clip's values: the mean of its T - 29 segments, or the sentinel; one workgroup per clip -----------------------------------------------
__global__ __launch_bounds__(ST_THREADS) void stoi_mean_kernel(const double* __restrict__ dseg, const int* __restrict__ kcount, double* __restrict__ out,
                                                             StoiGeom g) {
    __shared__ double lds[ST_THREADS / 64];
    const int b = blockIdx.x;
    const int segs = kcount[b] - 1 - (ST_SEG - 1);  // (block-uniform)
    double a = 0.0, c = 0.0;
    for (int m = threadIdx.x; m < segs; m += ST_THREADS) {
        a += dseg[((int64_t)b * g.seg_max + m) * 2];
        c += dseg[((int64_t)b * g.seg_max + m) * 2 + 1];
    }
    a = block_sum<ST_THREADS>(a, lds);
    c = block_sum<ST_THREADS>(c, lds);
    if (threadIdx.x == 0) {
        out[2 * (int64_t)b] = segs >= 1 ? a / (double)segs : ST_SENTINEL;
        out[2 * (int64_t)b + 1] = segs >= 1 ? c / (double)segs : ST_SENTINEL;
    }
}

double hann258(int j) { return 0.5 - 0.5 * std::cos(2.0 * M_PI * (double)(j + 1) / 257.0); }  // hanning(258)[1 + j]

}  // namespace

extern "C" {

int64_t l3ac_stoi_frames(int64_t samples) {
    L3AC_REQUIRE(samples >= 1, "stoi_frames: samples %lld must be positive", (long long)samples);
    return st_frames(samples);
}

int64_t l3ac_stoi_window(float* window, int64_t cap) {
    if (!window || cap < ST_FRAME) return ST_FRAME;
    for (int j = 0; j < ST_FRAME; ++j) window[j] = (float)hann258(j);
    return ST_FRAME;
}

int64_t l3ac_stoi_basis(float* basis, int64_t cap) {
    const int64_t need = (int64_t)ST_BASIS_ROWS * ST_FRAME;
    if (!basis || cap < need) return need;
    const double step = 2.0 * M_PI / ST_NFFT;
    for (int k = 0; k <= ST_NFFT / 2; ++k) {
        for (int j = 0; j < ST_FRAME; ++j) {
            const double w = hann258(j);  // (row 0, w cos(0) rounded once, is the fp32 window itself: the kernels read it there)
            const double ang = step * (double)((j * k) % ST_NFFT);  // the phase reduced in integers
            basis[(int64_t)(2 * k) * ST_FRAME + j] = (float)(w * std::cos(ang));
            basis[(int64_t)(2 * k + 1) * ST_FRAME + j] = (float)(-w * std::sin(ang));
        }
    }
    return need;
}

int l3ac_stoi_bands(int32_t* runs) {
    L3AC_REQUIRE(runs, "stoi_bands: null buffer");
    auto nearest = [](double f) {  // the first bin whose frequency is nearest to f
        int best = 0;
        double err = INFINITY;
        for (int k = 0; k <= ST_NFFT / 2; ++k) {
            const double d = (double)k * 10000.0 / ST_NFFT - f;
            if (d * d < err) {
                err = d * d;
                best = k;
            }
        }
        return best;
    };
    for (int i = 0; i < ST_BANDS; ++i) {
        runs[2 * i] = nearest(150.0 * std::pow(2.0, (2 * i - 1) / 6.0));
        runs[2 * i + 1] = nearest(150.0 * std::pow(2.0, (2 * i + 1) / 6.0));
    }
    return L3AC_OK;
}

int64_t l3ac_stoi_scratch_bytes(int32_t batch, int64_t max_samples) {
    StoiGeom g;
    StoiScratch sc;
    L3AC_TRY(stoi_geom(batch, max_samples, &g, &sc));
    return sc.total_min;
}

int l3ac_stoi(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples, const int32_t* samples,
              const float* basis, double* out, int32_t* frames_out, float* bands_out, void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    StoiGeom g;
    StoiScratch sc;
    L3AC_TRY(stoi_geom(batch, max_samples, &g, &sc));
    L3AC_REQUIRE(ref && est && out && frames_out, "stoi: null buffer");
    L3AC_REQUIRE(basis && ((uintptr_t)basis & 15) == 0, "stoi: the basis (l3ac_stoi_basis, copied to the device) must be a 16-byte aligned buffer");
    L3AC_REQUIRE(batch == 1 || (ref_stride >= max_samples && est_stride >= max_samples), "stoi: row stride below max_samples %lld",
                 (long long)max_samples);
    L3AC_TRY(check_clip_lengths("stoi", samples, batch, max_samples));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "stoi", "stoi", samples, batch, scratch, scratch_bytes, sc.total_min, &lens));
    char* base = static_cast<char*>(scratch);
    int* runs = reinterpret_cast<int*>(base + sc.runs);
    int* kcount = reinterpret_cast<int*>(base + sc.kcount);
    double* level = reinterpret_cast<double*>(base + sc.level);
    int* kept = reinterpret_cast<int*>(base + sc.kept);
    float* stage = reinterpret_cast<float*>(base + sc.stage);
    float* bands = reinterpret_cast<float*>(base + sc.bands);
    double* dseg = reinterpret_cast<double*>(base + sc.dseg);
    float* spec = reinterpret_cast<float*>(base + sc.spec);
    const float* window = basis;  // row 0: w[j] cos(0)

    if (g.f_max > 0) {
        ProfScope prof(s, "stoi_energy_kernel", 0.0, 4.0 * batch * (double)max_samples);
        hipLaunchKernelGGL(stoi_energy_kernel, dim3((unsigned)ceil_div64(g.f_max, ST_THREADS / 64), (unsigned)batch), dim3(ST_THREADS), 0, s, ref, ref_stride,
                           lens, window, level, g);
        L3AC_LAUNCH_CHECK();
    }
    {
        ProfScope prof(s, "stoi_select_kernel", 0.0, 20.0 * batch * (double)g.f_max);
        hipLaunchKernelGGL(stoi_select_kernel, dim3((unsigned)batch), dim3(ST_THREADS), 0, s, level, lens, kept, kcount, frames_out, g);
        L3AC_LAUNCH_CHECK();
    }
    if (g.t_max > 0) {
        int32_t host_runs[2 * ST_BANDS], lo_hi[2 * ST_BANDS];
        L3AC_TRY(l3ac_stoi_bands(host_runs));
        for (int i = 0; i < ST_BANDS; ++i) {  // the kernel reads [lo of every band][hi of every band]
            lo_hi[i] = host_runs[2 * i];
            lo_hi[ST_BANDS + i] = host_runs[2 * i + 1];
        }
        L3AC_TRY(launch_ragged_upload(s, runs, lo_hi, 2 * ST_BANDS));
        {
            ProfScope prof(s, "stoi_ola_kernel", 0.0, 16.0 * batch * (double)g.pitch);
            hipLaunchKernelGGL(stoi_ola_kernel, dim3((unsigned)ceil_div64(g.pitch / 4, ST_THREADS), (unsigned)batch, 2u), dim3(ST_THREADS), 0, s, ref,
                               ref_stride, est, est_stride, window, kept, kcount, stage, g);
            L3AC_LAUNCH_CHECK();
        }
        // slot rows per product: what the scratch holds (per signal), never more than there are
        const int64_t group = std::min<int64_t>(g.rows, (scratch_bytes - sc.spec) / (2 * (int64_t)ST_SPEC_LD * 4));
        float* spec1 = spec + group * ST_SPEC_LD;
        for (int64_t row0 = 0; row0 < g.rows; row0 += group) {
            const int64_t count = std::min(group, g.rows - row0);
            for (int sig = 0; sig < 2; ++sig) {
                GemmArgs ga;
                ga.a = stage + (int64_t)sig * batch * g.pitch + row0 * ST_HOP;  // row r of the product: 256 floats from here + 128 r
                ga.lda = ST_HOP;
                ga.w = basis;
                ga.ldw = ST_FRAME;
                ga.c = sig ? spec1 : spec;
                ga.ldc = ST_SPEC_LD;
                ga.m = count;
                ga.n = ST_BASIS_ROWS;
                ga.k = ST_FRAME;
                ga.epi = EPI_BIAS;
                L3AC_TRY(launch_gemm(s, ga));
            }
            ProfScope prof(s, "stoi_bands_kernel", 0.0, 8.0 * count * (double)(ST_SPEC_LD + ST_BAND_LD));
            hipLaunchKernelGGL(stoi_bands_kernel, dim3((unsigned)ceil_div64(count, SB_ROWS)), dim3(ST_THREADS), 0, s, spec, spec1, row0, (int)count, kcount, runs,
                               bands, bands_out, g);
            L3AC_LAUNCH_CHECK();
        }
    }
    if (g.seg_max > 0) {
        ProfScope prof(s, "stoi_segment_kernel", 0.0, 8.0 * batch * (double)g.seg_max * ST_SEG * ST_BAND_LD);
        hipLaunchKernelGGL(stoi_segment_kernel, dim3((unsigned)ceil_div64(g.seg_max, ST_THREADS / 64), (unsigned)batch), dim3(ST_THREADS), 0, s, bands, kcount,
                           dseg, 1.0 + std::pow(10.0, 15.0 / 20.0), g);
        L3AC_LAUNCH_CHECK();
    }
    {
        ProfScope prof(s, "stoi_mean_kernel", 0.0, 16.0 * batch * (double)g.seg_max);
        hipLaunchKernelGGL(stoi_mean_kernel, dim3((unsigned)batch), dim3(ST_THREADS), 0, s, dseg, kcount, out, g);
        L3AC_LAUNCH_CHECK();
    }
    return L3AC_OK;
}

}  // extern "C"
