// The short-time spectrum of un-centred frames and the critical-band measures of speech-codec evaluation on top of it: the frequency-
// weighted segmental SNR, the weighted spectral slope distance and the log-spectral distance (include/l3ac_hip.h, "critical-band
// measures"; DESIGN.md §3.22, which is normative).  No reference counterpart.
//
//   bands_frame_kernel  grid (groups of frames, batch), 4 waves.  A group is G consecutive frames of one clip; G and the waves of a frame
//                       are functions of n_fft alone: one wave a frame (four frames in step) and G = 16 up to n_fft = 256, the whole
//                       workgroup a frame above, with G = 8 up to 1024, 4 at 2048 and 2 at 4096 (SpectralGeom of spectral_frames.hpp,
//                       which coherence.hip shares).  The group's samples of the one or two sides and the window go to LDS once
//                       (stage_group of frame_groups.hpp, which owns the framing).  Then per frame and side, all fp64:
//     FFT               complex radix-2 decimation in time on two LDS arrays (re, im) of n_fft doubles: the bit-reversed load of xw[j] =
//                       (double)x[j] (double)w[j], then log2(n_fft) passes of n_fft / 2 butterflies with a barrier between them.  Every
//                       output is one fixed expression tree: which thread takes which butterfly changes no bit.  Element i lives at
//                       i ^ (i & 32 ? 31 : 0): the 32 lanes of an LDS read group then meet 32 different 8-byte banks in every pass (the
//                       passes with a half-span below 32 would otherwise put lanes l and l + 16 on one bank).  The network lives in
//                       fft_f64.hpp, which coherence.hip shares.
//     bins              k < n_fft / 2: P = re re + im im, A = sqrt(P) (correctly rounded), into the arrays' upper halves, which the bins
//                       at and above Nyquist have left; the first side of a pair moves to a third array.
//     sums              the team's first wave: S = sum A as 64 interleaved partials folded with fold64; lane i the band sums of band i,
//                       one chain over the band's run of non-zero weights (band_runs, once per workgroup)
//     measures          pairs only, the first wave: lane i the terms of band i (the peak walks are bounded by `bands`), lane 0 the sums
//                       in band order; the log-spectral distance as 64 interleaved partials
//   bands_pair_kernel   one workgroup per pair, built on the pair pieces of metric_common.hpp like lpc_pair_kernel: the frames' WSS values
//                       sorted in LDS and the lowest k summed in that order (lds_trimmed_mean), the two other measures summed in frame
//                       order (lds_ordered_mean); the LDS caps a pair at 16384 frames.
//
// A frame's values depend on its own N samples a side only — never on the batch, the clip's row, the row stride, the scratch size, the
// frame's place in its group or what lies after the clip's length, which is never read; no atomics.  Non-finite samples make unspecified
// values in the frames that read them, and in their pair's means; every index and every loop is bounded by the parameters, whatever the
// values.
//
// Contraction is off for this whole file: every product and sum rounds on its own, in the order DESIGN.md states.
#include "fft_f64.hpp"
#include "spectral_frames.hpp"

#include <algorithm>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int BD_THREADS = 256;
constexpr int BD_MIN_RATE = 8000, BD_MAX_RATE = 192000;
constexpr int BD_TABLE_BANDS = 25;
// a team's small rows of doubles in LDS: the two sums S, then rows of 64: the band sums M and E of each side, E clamped and in dB of each
// side, and four rows of terms
enum { SM_S = 0, SM_M = 8, SM_P = SM_M + 128, SM_EC = SM_P + 128, SM_DB = SM_EC + 128, SM_T0 = SM_DB + 128, SM_T1 = SM_T0 + 64, SM_T2 = SM_T1 + 64,
       SM_T3 = SM_T2 + 64, BD_SMALL = SM_T3 + 64 };

constexpr double BD_FLOOR = 1e-10;    // of a band energy and of a bin's power before the logarithm
constexpr double BD_ERR_FLOOR = 0x1p-52;

struct BandsGeom : SpectralGeom {
    int bands, lds_bytes;  // bands (0: none), dynamic LDS of the launch
};

// a team's small rows beside its three arrays, then the bands' runs [64][2] int32
constexpr int BD_LDS_MAX = spectral_lds_max<BD_SMALL, 128 * 4>();

int bands_geom(int32_t frame, int32_t hop, int32_t n_fft, int32_t bands, BandsGeom* p) {
    L3AC_TRY(spectral_geom("bands", frame, hop, n_fft, p));
    L3AC_REQUIRE(bands == 0 || (bands >= SP_MIN_BANDS && bands <= SP_MAX_BANDS), "bands: %d bands outside %d..%d", bands, SP_MIN_BANDS, SP_MAX_BANDS);
    p->bands = bands;
    p->lds_bytes = spectral_lds(n_fft, p->wpf, p->g, p->pitch, frame, BD_SMALL, 128 * 4);
    return L3AC_OK;
}

struct BandsIo {
    const float* ref;
    int64_t ref_stride;
    const float* est;  // nullptr: one side
    int64_t est_stride;
    int64_t max_samples;
    const int* lens;
    const float* window;
    const double* tw;       // [n_fft / 2][2]
    const double* weights;  // [bands][h] or nullptr
    int64_t f_max;
    double gamma;
    int normalize;
    // every output may be nullptr
    double* spectrum;   // [batch][F][h][2], one side
    double* power;      // [batch][F][h], one side
    double* magnitude;  // [batch][F][h], one side
    double* mag_sum;    // [batch][F][sides]
    double* band_p;     // [batch][F][sides][bands]: the band sums of P, before the floor
    double* band_m;     // [batch][F][sides][bands]: the band sums of m
    int* peaks;         // [batch][F][2][bands]: the nearest peak of slope i = 0 .. bands - 2, then the first maximum
    double* vals;       // [batch][F][3]: fwSegSNR, WSS, LSD
    int* flags;         // [batch][F]: counted for the fwSegSNR
    int* frames_out;    // [batch]
};

// ---- the frames: grid (groups, batch) ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BD_THREADS) void bands_frame_kernel(BandsIo io, BandsGeom p) {
    extern __shared__ __attribute__((aligned(16))) double lds_raw[];
    const int tid = threadIdx.x;
    const int ts = 64 * p.wpf, teams = BD_THREADS / ts, team = tid / ts, tl = tid % ts;
    const int b = blockIdx.y;
    const int n_frame = p.n, nf = p.n_fft, h = p.h, nb = p.bands;
    const bool pair = io.est != nullptr;
    const int sides = pair ? 2 : 1;
    double* zre = lds_raw + team * (3 * nf + BD_SMALL);  // [nf] each; after the bins the upper halves hold P and A
    double* zim = zre + nf;
    double* q0 = zim + nf;  // P [h], A [h] of a pair's first side
    double* sm = q0 + nf;   // [BD_SMALL]
    int* runs = reinterpret_cast<int*>(lds_raw + teams * (3 * nf + BD_SMALL));  // [64][2]: band i's non-zero weights are [lo, hi)
    float* win = reinterpret_cast<float*>(runs + 128);                           // [n]
    float* xs0 = win + n_frame;                                                  // [span_max]: frame k of the group starts at k pitch
    float* xs1 = xs0 + p.span_max();
    const int64_t frames = p.frames(io.lens ? io.lens[b] : io.max_samples);
    const int64_t f_max = io.f_max;
    const double nan = __builtin_nan("");
    if (io.frames_out && blockIdx.x == 0 && tid == 0) io.frames_out[b] = (int)frames;

    const int64_t t0 = (int64_t)blockIdx.x * p.g;
    if (t0 >= f_max) return;  // (the one workgroup of a batch without any frame)
    const int cnt = p.count(t0, frames);
    // rows at and after the clip's own frames
    for (int k = cnt + team; k < p.g && t0 + k < f_max; k += teams) {
        const int64_t row = (int64_t)b * f_max + t0 + k;
        for (int i = tl; i < 2 * h; i += ts) {
            if (io.spectrum) io.spectrum[row * 2 * h + i] = nan;
            if (i < h && io.power) io.power[row * h + i] = nan;
            if (i < h && io.magnitude) io.magnitude[row * h + i] = nan;
        }
        for (int i = tl; i < sides * nb; i += ts) {
            if (io.band_p) io.band_p[row * sides * nb + i] = nan;
            if (io.band_m) io.band_m[row * sides * nb + i] = nan;
            if (io.peaks) io.peaks[row * 2 * nb + i] = -1;
        }
        if (tl < sides && io.mag_sum) io.mag_sum[row * sides + tl] = nan;
        if (tl < 3 && io.vals) io.vals[row * 3 + tl] = nan;
        if (tl == 0 && io.flags) io.flags[row] = 0;
    }
    if (cnt == 0) return;  // (the whole workgroup)

    stage_group<BD_THREADS>(p, t0, cnt, io.ref + (int64_t)b * io.ref_stride, pair ? io.est + (int64_t)b * io.est_stride : nullptr, xs0, xs1);
    stage_window<BD_THREADS>(n_frame, io.window, win);
    band_runs(io.weights, nb, h, runs);
    __syncthreads();

    for (int k0 = 0; k0 < cnt; k0 += teams) {  // the teams in step: every barrier below is reached by all of them
        const int k = k0 + team;
        const bool active = k < cnt;
        const int64_t row = (int64_t)b * f_max + t0 + k;
        for (int side = 0; side < sides; ++side) {
            const float* x = (side ? xs1 : xs0) + (active ? k : 0) * p.pitch;
            fft_f64_load(zre, zim, x, win, n_frame, nf, p.log2n, tl, ts);
            fft_f64_passes(zre, zim, io.tw, nf, p.log2n, tl, ts);
            double* pw = (pair && side == 0) ? q0 : zre + h;
            double* mg = (pair && side == 0) ? q0 + h : zim + h;
            for (int kk = tl; kk < h; kk += ts) {  // (the elements below h stay below h under swz: h is below 32 or a multiple of 32)
                const double re = zre[swz(kk)], im = zim[swz(kk)];
                const double pk = re * re + im * im;
                const double ak = __dsqrt_rn(pk);
                pw[kk] = pk, mg[kk] = ak;
                if (active) {
                    if (io.spectrum) io.spectrum[(row * h + kk) * 2] = re, io.spectrum[(row * h + kk) * 2 + 1] = im;
                    if (io.power) io.power[row * h + kk] = pk;
                    if (io.magnitude) io.magnitude[row * h + kk] = ak;
                }
            }
            __syncthreads();
            if (tl < 64) {
                double s_mag = 0.0;
                for (int kk = tl; kk < h; kk += 64) s_mag = s_mag + mg[kk];
                s_mag = __shfl(fold64(s_mag), 0, 64);
                if (tl == 0) sm[SM_S + side] = s_mag;
                if (tl == 0 && active && io.mag_sum) io.mag_sum[row * sides + side] = s_mag;
                if (io.weights && tl < nb) {
                    const double* wrow = io.weights + (int64_t)tl * h;
                    const int lo = runs[2 * tl], hi = runs[2 * tl + 1];
                    double acc_m = 0.0, acc_p = 0.0;
                    for (int kk = lo; kk < hi; ++kk) {
                        const double w = wrow[kk];
                        const double m = io.normalize ? mg[kk] / s_mag : mg[kk];
                        acc_m = acc_m + w * m;
                        acc_p = acc_p + w * pw[kk];
                    }
                    sm[SM_M + side * 64 + tl] = acc_m, sm[SM_P + side * 64 + tl] = acc_p;
                    if (active && io.band_m) io.band_m[(row * sides + side) * nb + tl] = acc_m;
                    if (active && io.band_p) io.band_p[(row * sides + side) * nb + tl] = acc_p;
                }
            }
            // (the next side's load writes the elements below h of re and im only after this barrier; P, A and sm stay)
            __syncthreads();
        }
        if (!pair || !io.weights) continue;  // (uniform)

        // ---- the measures of the pair: the team's first wave, P and A of side 0 in q0, of side 1 in the upper halves of re and im
        if (tl < nb) {
            const double m_r = sm[SM_M + tl], m_e = sm[SM_M + 64 + tl];
            const double d = m_r - m_e, dd = d * d;
            const double err = dd > BD_ERR_FLOOR ? dd : BD_ERR_FLOOR;
            const double w = pow(m_r, io.gamma);
            const double snr = 10.0 * log10((m_r * m_r) / err);
            sm[SM_T0 + tl] = w, sm[SM_T1 + tl] = w * snr;
            for (int side = 0; side < 2; ++side) {
                const double e_raw = sm[SM_P + side * 64 + tl];
                const double e_c = e_raw > BD_FLOOR ? e_raw : BD_FLOOR;
                sm[SM_EC + side * 64 + tl] = e_c, sm[SM_DB + side * 64 + tl] = 10.0 * log10(e_c);
            }
        }
        __syncthreads();
        double lsd = 0.0;
        if (tl < 64) {
            double w_side[2] = {0.0, 0.0}, slope[2] = {0.0, 0.0};
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const double* ec = sm + SM_EC + side * 64;
                const double* db = sm + SM_DB + side * 64;
                int am = 0;
                for (int i = 1; i < nb; ++i)
                    if (ec[i] > ec[am]) am = i;
                if (tl < nb - 1) {
                    int at;
                    if (ec[tl + 1] > ec[tl]) {
                        int m = tl;
                        while (m <= nb - 2 && ec[m + 1] > ec[m]) ++m;
                        at = m;
                    } else {
                        int m = tl;
                        while (m >= 0 && !(ec[m + 1] > ec[m])) --m;
                        at = m + 1;
                    }
                    const double e_i = db[tl];
                    w_side[side] = (20.0 / ((20.0 + db[am]) - e_i)) * (1.0 / ((1.0 + db[at]) - e_i));
                    slope[side] = db[tl + 1] - e_i;
                    if (active && io.peaks) io.peaks[(row * 2 + side) * nb + tl] = at;
                }
                if (tl == nb - 1 && active && io.peaks) io.peaks[(row * 2 + side) * nb + tl] = am;
            }
            if (tl < nb - 1) {
                const double w = (w_side[0] + w_side[1]) / 2.0, d = slope[0] - slope[1];
                sm[SM_T2 + tl] = w, sm[SM_T3 + tl] = w * (d * d);
            }
            const double* p_r = q0;
            const double* p_e = zre + h;
            for (int kk = tl; kk < h; kk += 64) {
                const double a = p_r[kk] > BD_FLOOR ? p_r[kk] : BD_FLOOR, c = p_e[kk] > BD_FLOOR ? p_e[kk] : BD_FLOOR;
                const double d = 10.0 * log10(a) - 10.0 * log10(c);
                lsd = lsd + d * d;
            }
            lsd = fold64(lsd);
        }
        __syncthreads();
        if (tl == 0 && active) {
            double num = 0.0, den = 0.0;
            for (int i = 0; i < nb; ++i) num = num + sm[SM_T1 + i], den = den + sm[SM_T0 + i];
            const double fw = clamp_to(num / den, -10.0, 35.0);
            double w_num = 0.0, w_den = 0.0;
            for (int i = 0; i < nb - 1; ++i) w_num = w_num + sm[SM_T3 + i], w_den = w_den + sm[SM_T2 + i];
            const bool counted = sm[SM_S] > 0.0 && sm[SM_S + 1] > 0.0;
            io.vals[row * 3] = counted ? fw : nan;
            io.vals[row * 3 + 1] = w_num / w_den;
            io.vals[row * 3 + 2] = __dsqrt_rn(lsd / (double)h);
            io.flags[row] = counted ? 1 : 0;
        }
        __syncthreads();  // the rows are read before the next frame overwrites them
    }
}

// ---- the pair: one workgroup per pair -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PAIR_THREADS) void bands_pair_kernel(const double* __restrict__ vals, const int* __restrict__ flags, int64_t f_max,
                                                              int64_t max_samples, const int* __restrict__ lens, BandsGeom p, double trim,
                                                              double* __restrict__ out, int* __restrict__ counts) {
    __shared__ double buf[PAIR_MAX_FRAMES];
    __shared__ unsigned char fl[PAIR_MAX_FRAMES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int frames = pair_frames(p.frames(lens ? lens[b] : max_samples), f_max);
    const double* row = vals + (int64_t)b * f_max * 3;
    int v_snr = 0;
    for (int f = tid; f < frames; f += PAIR_THREADS) {
        const int g = flags[(int64_t)b * f_max + f];
        fl[f] = (unsigned char)g;
        v_snr += g & 1;
    }
    v_snr = block_count<PAIR_THREADS>(v_snr);
    const int keep = (int)floor(trim * (double)frames + 0.5);
    const double wss = lds_trimmed_mean<PAIR_THREADS>(buf, frames, keep, [&](int f) { return row[f * 3 + 1]; }, [](int) { return true; });
    if (tid == 0) out[(int64_t)b * 3 + 1] = (frames == 0 || keep == 0) ? __builtin_nan("") : wss;
    for (int m = 0; m < 3; m += 2) {  // the fwSegSNR over its counted frames, the LSD over all, in frame order
        const double mean = lds_ordered_mean<PAIR_THREADS>(buf, frames, m == 0 ? v_snr : frames, [&](int f) { return row[f * 3 + m]; },
                                                         [&](int f) { return m == 2 || (fl[f] & 1); });
        if (tid == 0) out[(int64_t)b * 3 + m] = mean;
    }
    if (tid == 0) counts[(int64_t)b * 2] = frames, counts[(int64_t)b * 2 + 1] = v_snr;
}

int configure_frame_kernel() {
    static PerDeviceOnce configured;
    return raise_dynamic_lds(configured, {{bands_frame_kernel, BD_LDS_MAX}});
}

// the parameters checked, then (metrics) the frames' three values [batch][F][3] fp64 and the frames' flags [batch][F] int32
int bands_scratch(const char* what, bool metrics, int32_t batch, int64_t max_samples, int32_t frame, int32_t hop, int32_t n_fft, int32_t bands,
                  BandsGeom* p, PairScratch* sc) {
    L3AC_TRY(bands_geom(frame, hop, n_fft, bands, p));
    L3AC_TRY(check_clip_batch(what, batch, max_samples));
    ScratchPlan plan(batch);
    sc->vals = sc->flags = 0;
    if (metrics) {
        L3AC_REQUIRE(bands != 0, "%s: %d bands outside %d..%d", what, bands, SP_MIN_BANDS, SP_MAX_BANDS);
        L3AC_TRY(pair_frames_plan(what, batch, p->frames(max_samples), 24, plan, &sc->vals, &sc->flags));
    }
    sc->need = plan.bytes;
    return L3AC_OK;
}

int launch_frames(hipStream_t s, const BandsIo& io, const BandsGeom& p, int32_t batch, bool always) {
    if (io.f_max == 0 && !always) return L3AC_OK;
    L3AC_TRY(configure_frame_kernel());
    // (no frame anywhere: one workgroup per clip still writes the frame counts)
    const int64_t groups = std::max<int64_t>(ceil_div64(io.f_max, p.g), 1);
    const double sides = io.est ? 2.0 : 1.0;
    ProfScope prof(s, "bands_frame_kernel", sides * batch * (double)io.f_max * 5.0 * p.n_fft * p.log2n, sides * 4.0 * batch * (double)io.max_samples);
    hipLaunchKernelGGL(bands_frame_kernel, dim3((unsigned)groups, (unsigned)batch), dim3(BD_THREADS), (size_t)p.lds_bytes, s, io, p);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

// the 25 critical bands of the published measures: centre frequencies and bandwidths in Hz
const double BD_CENTRE[BD_TABLE_BANDS] = {50.0,    120.0,   190.0,   260.0,   330.0,   400.0,   470.0,   540.0,   617.372, 703.378, 798.717, 904.128, 1020.38,
                                          1148.30, 1288.72, 1442.54, 1610.70, 1794.16, 1993.93, 2211.08, 2446.71, 2701.97, 2978.04, 3276.17, 3597.63};
const double BD_WIDTH[BD_TABLE_BANDS] = {70.0,    70.0,    70.0,    70.0,    70.0,    70.0,    70.0,    77.3724, 86.0056, 95.3398, 105.411, 116.256, 127.914,
                                         140.423, 153.823, 168.154, 183.457, 199.776, 217.153, 235.631, 255.255, 276.072, 298.126, 321.465, 346.136};

}  // namespace

extern "C" {

int32_t l3ac_bands_default_fft(int32_t frame) {
    L3AC_REQUIRE(frame >= SP_MIN_FRAME && frame <= SP_MAX_FRAME, "bands: frame %d outside %d..%d", frame, SP_MIN_FRAME, SP_MAX_FRAME);
    int32_t n_fft = SP_MIN_FFT;
    while (n_fft < 2 * frame) n_fft <<= 1;
    return n_fft;
}

int64_t l3ac_bands_twiddles(int32_t n_fft, double* out, int64_t cap) {
    L3AC_TRY(check_n_fft("bands", n_fft));
    if (!out || cap < n_fft) return n_fft;
    const long double two_pi = 2.0L * acosl(-1.0L);
    const int half = n_fft / 2, quarter = n_fft / 4, eighth = n_fft / 8;
    for (int m = 0; m < half; ++m) {
        // the angle 2 pi m / n_fft lies in [0, pi): mirrored into [0, pi / 2] and then into [0, pi / 4]
        const int m1 = m > quarter ? half - m : m;
        const bool swap = m1 > eighth;
        const int m2 = swap ? quarter - m1 : m1;
        const long double a = two_pi * (long double)m2 / (long double)n_fft;
        long double c = swap ? sinl(a) : cosl(a), sn = swap ? cosl(a) : sinl(a);
        if (m > quarter) c = -c;
        out[2 * m] = (double)c, out[2 * m + 1] = (double)-sn;
    }
    out[0] = 1.0, out[1] = 0.0;
    out[2 * quarter] = 0.0, out[2 * quarter + 1] = -1.0;
    return n_fft;
}

int64_t l3ac_bands_critical(double* out, int64_t cap) {
    if (!out || cap < 2 * BD_TABLE_BANDS) return 2 * BD_TABLE_BANDS;
    for (int i = 0; i < BD_TABLE_BANDS; ++i) out[i] = BD_CENTRE[i], out[BD_TABLE_BANDS + i] = BD_WIDTH[i];
    return 2 * BD_TABLE_BANDS;
}

int64_t l3ac_band_weights(int32_t sample_rate, int32_t n_fft, int32_t bands, const double* centre_hz, const double* bandwidth_hz, double* out,
                          int64_t cap) {
    L3AC_REQUIRE(sample_rate >= BD_MIN_RATE && sample_rate <= BD_MAX_RATE, "band_weights: sample_rate %d outside %d..%d", sample_rate, BD_MIN_RATE,
                 BD_MAX_RATE);
    L3AC_TRY(check_n_fft("band_weights", n_fft));
    L3AC_REQUIRE(bands >= SP_MIN_BANDS && bands <= SP_MAX_BANDS, "band_weights: %d bands outside %d..%d", bands, SP_MIN_BANDS, SP_MAX_BANDS);
    L3AC_REQUIRE(centre_hz && bandwidth_hz, "band_weights: null centre_hz or bandwidth_hz");
    const int h = n_fft / 2;
    const double nyquist = sample_rate / 2.0;
    double narrowest = bandwidth_hz[0];
    for (int i = 0; i < bands; ++i) {
        L3AC_REQUIRE(centre_hz[i] >= 0.0 && centre_hz[i] < nyquist, "band_weights: centre_hz[%d] = %g outside [0, %g)", i, centre_hz[i], nyquist);
        L3AC_REQUIRE(bandwidth_hz[i] > 0.0 && std::isfinite(bandwidth_hz[i]), "band_weights: bandwidth_hz[%d] = %g must be positive and finite", i,
                     bandwidth_hz[i]);
        narrowest = std::min(narrowest, bandwidth_hz[i]);
    }
    const int64_t count = (int64_t)bands * h;
    const bool fill = out && cap >= count;
    const double threshold = (double)expl(-30.0L / (2.0L * 2.303L));
    for (int i = 0; i < bands; ++i) {
        const double f0 = centre_hz[i] / nyquist * (double)h, bw = bandwidth_hz[i] / nyquist * (double)h;
        const long double at = (long double)std::floor(f0), gain = logl((long double)narrowest) - logl((long double)bandwidth_hz[i]);
        bool any = false;
        for (int k = 0; k < h; ++k) {
            const long double x = ((long double)k - at) / (long double)bw;
            double w = (double)expl(-11.0L * (x * x) + gain);
            if (w <= threshold) w = 0.0;
            any = any || w != 0.0;
            if (fill) out[(int64_t)i * h + k] = w;
        }
        L3AC_REQUIRE(any, "band_weights: band %d (centre %g Hz, bandwidth %g Hz) has no non-zero weight", i, centre_hz[i], bandwidth_hz[i]);
    }
    return count;
}

int64_t l3ac_frame_spectrum_scratch_bytes(int32_t batch, int64_t max_samples, int32_t frame, int32_t hop, int32_t n_fft) {
    BandsGeom p;
    PairScratch sc;
    L3AC_TRY(bands_scratch("frame_spectrum", false, batch, max_samples, frame, hop, n_fft, 0, &p, &sc));
    return sc.need;  // the clips' lengths
}

int l3ac_frame_spectrum(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, int32_t frame,
                        int32_t hop, int32_t n_fft, const float* window, const double* twiddles, double* spectrum, double* power, double* magnitude,
                        double* magnitude_sum, int32_t* frames, void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    BandsGeom p;
    PairScratch sc;
    L3AC_TRY(bands_scratch("frame_spectrum", false, batch, max_samples, frame, hop, n_fft, 0, &p, &sc));
    const int64_t f_max = p.frames(max_samples);
    L3AC_REQUIRE(audio, "frame_spectrum: null audio");
    L3AC_REQUIRE(twiddles, "frame_spectrum: null twiddles");
    L3AC_REQUIRE(f_max == 0 || spectrum, "frame_spectrum: null output buffer");
    L3AC_REQUIRE(batch == 1 || audio_stride >= max_samples, "frame_spectrum: row stride %lld below max_samples %lld", (long long)audio_stride,
                 (long long)max_samples);
    L3AC_TRY(check_clip_lengths("frame_spectrum", samples, batch, max_samples));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "frame_spectrum", "frame_spectrum", samples, batch, scratch, scratch_bytes, sc.need, &lens));
    BandsIo io{};
    io.ref = audio, io.ref_stride = audio_stride, io.max_samples = max_samples, io.lens = lens, io.window = window, io.tw = twiddles, io.f_max = f_max;
    io.spectrum = spectrum, io.power = power, io.magnitude = magnitude, io.mag_sum = magnitude_sum, io.frames_out = frames;
    return launch_frames(s, io, p, batch, true);
}

int l3ac_band_energies(const float* audio, int64_t audio_stride, int32_t batch, int64_t max_samples, const int32_t* samples, int32_t frame,
                       int32_t hop, int32_t n_fft, const float* window, const double* twiddles, const double* weights, int32_t bands, double* power,
                       double* magnitude, int32_t* frames, void* scratch, int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    BandsGeom p;
    PairScratch sc;
    L3AC_REQUIRE(bands != 0, "band_energies: %d bands outside %d..%d", bands, SP_MIN_BANDS, SP_MAX_BANDS);
    L3AC_TRY(bands_scratch("band_energies", false, batch, max_samples, frame, hop, n_fft, bands, &p, &sc));
    const int64_t f_max = p.frames(max_samples);
    L3AC_REQUIRE(audio, "band_energies: null audio");
    L3AC_REQUIRE(twiddles && weights, "band_energies: null twiddles or weights");
    L3AC_REQUIRE(f_max == 0 || (power && magnitude), "band_energies: null output buffer");
    L3AC_REQUIRE(batch == 1 || audio_stride >= max_samples, "band_energies: row stride %lld below max_samples %lld", (long long)audio_stride,
                 (long long)max_samples);
    L3AC_TRY(check_clip_lengths("band_energies", samples, batch, max_samples));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "band_energies", "frame_spectrum", samples, batch, scratch, scratch_bytes, sc.need, &lens));
    BandsIo io{};
    io.ref = audio, io.ref_stride = audio_stride, io.max_samples = max_samples, io.lens = lens, io.window = window, io.tw = twiddles, io.f_max = f_max;
    io.weights = weights, io.band_p = power, io.band_m = magnitude, io.frames_out = frames;
    return launch_frames(s, io, p, batch, true);
}

int64_t l3ac_band_metrics_scratch_bytes(int32_t batch, int64_t max_samples, int32_t frame, int32_t hop, int32_t n_fft, int32_t bands) {
    BandsGeom p;
    PairScratch sc;
    L3AC_TRY(bands_scratch("band_metrics", true, batch, max_samples, frame, hop, n_fft, bands, &p, &sc));
    return sc.need;
}

int l3ac_band_metrics(const float* ref, int64_t ref_stride, const float* est, int64_t est_stride, int32_t batch, int64_t max_samples,
                      const int32_t* samples, int32_t frame, int32_t hop, int32_t n_fft, const float* window, const double* twiddles,
                      const double* weights, int32_t bands, double gamma, int32_t normalize, double trim, double* out, int32_t* counts,
                      double* frame_values, double* magnitude_sum, double* band_power, double* band_magnitude, int32_t* peaks, void* scratch,
                      int64_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    BandsGeom p;
    PairScratch sc;
    L3AC_TRY(bands_scratch("band_metrics", true, batch, max_samples, frame, hop, n_fft, bands, &p, &sc));
    L3AC_REQUIRE(std::isfinite(gamma), "band_metrics: gamma %g must be finite", gamma);
    L3AC_REQUIRE(normalize == 0 || normalize == 1, "band_metrics: normalize %d must be 0 or 1", normalize);
    L3AC_REQUIRE(trim > 0.0 && trim <= 1.0, "band_metrics: trim %g outside (0, 1]", trim);
    L3AC_REQUIRE(ref && est, "band_metrics: null audio");
    L3AC_REQUIRE(twiddles && weights, "band_metrics: null twiddles or weights");
    L3AC_REQUIRE(out && counts, "band_metrics: null output buffer");
    L3AC_REQUIRE(batch == 1 || (ref_stride >= max_samples && est_stride >= max_samples), "band_metrics: row stride below max_samples %lld",
                 (long long)max_samples);
    L3AC_TRY(check_clip_lengths("band_metrics", samples, batch, max_samples));
    int* lens;
    L3AC_TRY(stage_clip_lengths(s, "band_metrics", "band_metrics", samples, batch, scratch, scratch_bytes, sc.need, &lens));
    const int64_t f_max = p.frames(max_samples);
    char* base = static_cast<char*>(scratch);
    double* vals = frame_values ? frame_values : reinterpret_cast<double*>(base + sc.vals);
    int* flags = reinterpret_cast<int*>(base + sc.flags);
    BandsIo io{};
    io.ref = ref, io.ref_stride = ref_stride, io.est = est, io.est_stride = est_stride, io.max_samples = max_samples, io.lens = lens;
    io.window = window, io.tw = twiddles, io.weights = weights, io.f_max = f_max, io.gamma = gamma, io.normalize = normalize;
    io.mag_sum = magnitude_sum, io.band_p = band_power, io.band_m = band_magnitude, io.peaks = peaks, io.vals = vals, io.flags = flags;
    L3AC_TRY(launch_frames(s, io, p, batch, false));
    ProfScope prof(s, "bands_pair_kernel", 0.0, 28.0 * batch * (double)f_max);
    hipLaunchKernelGGL(bands_pair_kernel, dim3((unsigned)batch), dim3(PAIR_THREADS), 0, s, vals, flags, f_max, max_samples, lens, p, trim, out, counts);
    L3AC_LAUNCH_CHECK();
    return L3AC_OK;
}

}  // extern "C"
