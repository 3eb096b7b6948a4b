// kernels_notch.hpp -- narrowband (CW) interference in complex64 samples (include/gypsum_hip.h, "notch"): complex amplitudes of
// tones per block (gyp_iq_tones_dev: spectrum scan, frequency refinement), their removal per millisecond (gyp_notch_iq_dev, the
// ingest's in-place pass between whatever produced a block and the level) and the host arithmetic around the two (gyp_tones_find,
// gyp_tone_refine).
//
// Phase.  Both kernels take the down-converter's mixer (ddc_mixer, kernels_resample.hpp): theta(i) = 2 pi ((f i) mod fs) / fs with
// i the absolute sample index and f a whole number of Hz carried as f mod fs in [0, fs).  (f i) mod fs comes off in integers -- a
// lane reduces its first index mod fs once (f, i mod fs < 2^31: the product stays below 2^62) and then steps by (f T) mod fs for
// its stride of T samples -- so the float32 pair (cos theta, -sin theta) is a pure function of (f, i), within 2^-22 of exact at
// any index: blocks, windows, seeks and launch shapes see the same bits.
//
// Measurement.  Thread t of the workgroup owns samples n = t, t + T, ... of the item's row and adds, in that order and in float64,
//     re += w[n] * (x_re c - x_im s)      im += w[n] * (x_re s + x_im c)        with (c, s) = (cos theta, -sin theta) in float32
// (each float32 x float32 product is exact in float64; the difference / sum, the window product and the accumulation are one
// rounding each: contraction is off; rectangular rows skip the window product).  The T partial sums are reduced by a fixed tree --
// lane l takes lane l + 32, 16, 8, 4, 2, 1 of its wavefront, then thread 0 adds the wavefronts' sums in order through LDS -- and
// thread 0 divides by the window's sum.  Rows are read 8 bytes per sample whatever their alignment.  No atomics: a record is a
// pure function of its samples, its first index and its frequency, the same bits for every call shape, window and grid size.
//
// Removal (iq_notch_kernel).  One kNotchThreads-thread workgroup per (stream, millisecond) over the widen kernel's persistent grid.
// For the stream's tones t = 0 .. K-1 in list order:
//     A_t  = the rectangular measurement above over the millisecond's N samples of the residual y_(t-1) (y_(-1) = x), as float64,
//            then a_t = ((float)Re A_t, (float)Im A_t)
//     y_t  = y_(t-1) - a_t e^(+j theta_t) in float32:   p_re = a_re c - a_im s'    p_im = a_re s' + a_im c     (s' = sin theta = -s)
//                                                      y_re = y_re - p_re         y_im = y_im - p_im
//            (four products, one difference, one sum and two subtractions: one float32 rounding each)
// The subtraction of tone t-1 and the measurement of tone t share one pass over the residual.  A thread reads and writes its own
// samples only, so the residual may live anywhere: in LDS where the millisecond fits 128 KiB (N <= 16384), else in the output
// buffer, re-read from L2.  Arithmetic per sample and reduction order are the same in both forms: the same bits (a test compares
// them through gyp_debug_set "notch_no_lds").  out may be in; an empty tone list copies the input bits.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

struct ToneMix {
    int64_t fs;        // < 2^31
    double q_scale;    // 4 / fs
    double y_scale;    // 1 / (2 fs)
};

// (f i) mod fs for a lane whose first absolute index is i (>= 0), and its step for a stride of T samples.
__device__ __forceinline__ int64_t tone_phase0(int64_t f, int64_t i, int64_t fs) { return f * (i % fs) % fs; }
__device__ __forceinline__ int64_t tone_step(int64_t f, int64_t T, int64_t fs) { return f * (T % fs) % fs; }

// One sample's term of the measurement: x e^(-j theta), float64 over the float32 mixer value m = (cos theta, -sin theta).
__device__ __forceinline__ void tone_term(float2 x, float2 m, double& tr, double& ti) {
#pragma clang fp contract(off)
    const double r = (double)x.x, i = (double)x.y, c = (double)m.x, s = (double)m.y;
    const double rc = r * c, is = i * s, rs = r * s, ic = i * c;
    tr = rc - is;
    ti = rs + ic;
}

// The fixed tree over a workgroup of W wavefronts: in-wave, then thread 0 adds the wavefronts' sums in order.  Thread 0 returns
// the sums; the others return garbage.  The caller keeps a __syncthreads between two uses of s_re / s_im.
template <int W>
__device__ __forceinline__ void tone_reduce(double& re, double& im, double* s_re, double* s_im) {
#pragma clang fp contract(off)
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        re += __shfl_down(re, off, 64);
        im += __shfl_down(im, off, 64);
    }
    if (lane == 0) {
        s_re[wave] = re;
        s_im[wave] = im;
    }
    __syncthreads();
    if (t == 0) {
        re = s_re[0];
        im = s_im[0];
#pragma unroll
        for (int w = 1; w < W; ++w) {
            re += s_re[w];
            im += s_im[w];
        }
    }
}

// One workgroup per (stream, block, frequency) item, frequency fastest (neighbouring workgroups read the same block).
// freqs: f mod fs per frequency.  window: GYP_WINDOW_RECT or GYP_WINDOW_HANN, w[n] = sin^2(pi (n + 1) / (B + 1)) in float64, whose
// sum over the block is (B + 1) / 2.
__global__ __launch_bounds__(256) void iq_tones_kernel(const float2* __restrict__ iq, int64_t stream_stride, int64_t first_index,
                                                       int32_t n_blocks, int32_t B, const int64_t* __restrict__ freqs, int32_t n_freq,
                                                       ToneMix mix, int32_t window, int64_t n_items, gyp_tone_rec* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double s_re[4], s_im[4];
    const int t = (int)threadIdx.x;
    const int64_t per_stream = (int64_t)n_blocks * n_freq;
    const double w_arg = 1.0 / (double)(B + 1);
    const double w_sum = window == GYP_WINDOW_HANN ? (double)(B + 1) * 0.5 : (double)B;
    for (int64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const int64_t s = it / per_stream, rem = it - s * per_stream;
        const int64_t b = rem / n_freq, k = rem - b * n_freq;
        const float2* row = iq + s * stream_stride + b * B;
        const int64_t f = freqs[k];
        int64_t r = tone_phase0(f, first_index + b * B + t, mix.fs);
        const int64_t step = tone_step(f, 256, mix.fs);
        double re = 0.0, im = 0.0;
        for (int32_t n = t; n < B; n += 256) {
            const float2 m = ddc_mixer(r, mix.fs, mix.q_scale, mix.y_scale);
            double tr, ti;
            tone_term(row[n], m, tr, ti);
            if (window == GYP_WINDOW_HANN) {
                const double sw = sinpi((double)(n + 1) * w_arg);
                const double w = sw * sw;
                tr = w * tr;
                ti = w * ti;
            }
            re += tr;
            im += ti;
            r += step;
            if (r >= mix.fs) r -= mix.fs;
        }
        tone_reduce<4>(re, im, s_re, s_im);
        if (t == 0) {
            gyp_tone_rec rec;
            rec.re = re / w_sum;
            rec.im = im / w_sum;
            out[it] = rec;
        }
        __syncthreads();   // the next item's partial sums reuse the LDS words
    }
}

// The tone lists of up to kNotchStreams streams travel as a kernel argument (f mod fs each): no device table, nothing to wait for.
constexpr int kNotchStreams = 8;
constexpr int kNotchThreads = 1024;
constexpr int32_t kNotchLdsSamples = 16384;   // 128 KiB of float2: every rate up to 16.368 Msps; 49.104 Msps re-reads from L2
struct NotchArgs {
    int32_t count[kNotchStreams];
    int64_t f[kNotchStreams][GYP_NOTCH_MAX_TONES];
};

template <bool LDS>
__global__ __launch_bounds__(kNotchThreads) void iq_notch_kernel(const float2* in, float2* out, int64_t stream_stride, int64_t first_index,
                                                                 int32_t n_ms, int32_t n, int64_t n_items, ToneMix mix, NotchArgs tones) {
#pragma clang fp contract(off)
    extern __shared__ float2 notch_xs[];   // LDS: the millisecond's residual (n samples)
    constexpr int W = kNotchThreads / 64;
    __shared__ double s_re[W], s_im[W];
    __shared__ float2 s_a;
    const int t = (int)threadIdx.x;
    for (int64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const int64_t s = it / n_ms, ms = it - s * n_ms;
        const float2* src = in + s * stream_stride + ms * n;
        float2* dst = out + s * stream_stride + ms * n;
        const int32_t K = tones.count[s];
        const int64_t i0 = first_index + ms * n + t;
        float2 a = make_float2(0.f, 0.f);
        int64_t f_prev = 0;
        for (int32_t tt = 0; tt <= K; ++tt) {   // pass tt: subtract tone tt - 1, measure tone tt
            const int64_t f_cur = tt < K ? tones.f[s][tt] : 0;
            int64_t rp = tone_phase0(f_prev, i0, mix.fs), rc = tone_phase0(f_cur, i0, mix.fs);
            const int64_t sp = tone_step(f_prev, kNotchThreads, mix.fs), sc = tone_step(f_cur, kNotchThreads, mix.fs);
            double re = 0.0, im = 0.0;
            for (int32_t k = t; k < n; k += kNotchThreads) {
                float2 x = tt == 0 ? src[k] : (LDS ? notch_xs[k] : dst[k]);
                if (tt > 0) {
                    const float2 m = ddc_mixer(rp, mix.fs, mix.q_scale, mix.y_scale);
                    const float c = m.x, s1 = -m.y;   // e^(+j theta)
                    const float ac = a.x * c, bs = a.y * s1, as = a.x * s1, bc = a.y * c;
                    const float p_re = ac - bs, p_im = as + bc;
                    x.x = x.x - p_re;
                    x.y = x.y - p_im;
                    rp += sp;
                    if (rp >= mix.fs) rp -= mix.fs;
                }
                if (LDS && tt < K) notch_xs[k] = x;
                else dst[k] = x;
                if (tt < K) {
                    const float2 m = ddc_mixer(rc, mix.fs, mix.q_scale, mix.y_scale);
                    double tr, ti;
                    tone_term(x, m, tr, ti);
                    re += tr;
                    im += ti;
                    rc += sc;
                    if (rc >= mix.fs) rc -= mix.fs;
                }
            }
            if (tt < K) {
                tone_reduce<W>(re, im, s_re, s_im);
                if (t == 0) s_a = make_float2((float)(re / (double)n), (float)(im / (double)n));
                __syncthreads();
                a = s_a;
                f_prev = f_cur;
            }
        }
        __syncthreads();   // s_a and the partial sums are reused by the next item
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
constexpr int64_t kNotchMinSeparationHz = 4000;

// GYP_E_BAD_ARG's reason, or nullptr if the list can be removed at fs_hz.
static const char* notch_check(const int64_t* freqs, int32_t count, int64_t fs_hz) {
    if (count < 0 || count > GYP_NOTCH_MAX_TONES) return "a stream takes between 0 and 8 tones";
    if (count > 0 && !freqs) return "the tone list is NULL";
    for (int32_t i = 0; i < count; ++i) {
        const int64_t f = freqs[i];
        if (f <= -fs_hz || f >= fs_hz || 2 * (f < 0 ? -f : f) >= fs_hz) return "every tone must satisfy |f| < fs / 2";
        for (int32_t j = 0; j < i; ++j) {
            const int64_t d = f - freqs[j];
            if ((d < 0 ? -d : d) < kNotchMinSeparationHz)
                return "tones of one stream must be at least 4000 Hz apart (over one millisecond closer tones are far from orthogonal)";
        }
    }
    return nullptr;
}

static inline int64_t tone_mod(int64_t f, int64_t fs) { return ((f % fs) + fs) % fs; }

// gyp_tones_find's selection (the header states the rules).  The number of bins written, or -1 with *why set.
static int32_t tones_find(const double* power, int32_t n_freq, double threshold_over_median, int32_t min_separation_bins, int32_t max_tones,
                          int32_t* out_bins, const char** why, double* median_out = nullptr) {
    for (int32_t k = 0; k < n_freq; ++k)
        if (!(power[k] >= 0.0) || !std::isfinite(power[k])) {
            *why = "every power must be finite and >= 0";
            return -1;
        }
    std::vector<double> sorted(power, power + n_freq);
    std::sort(sorted.begin(), sorted.end());
    const double median = n_freq % 2 ? sorted[(size_t)n_freq / 2] : (sorted[(size_t)n_freq / 2 - 1] + sorted[(size_t)n_freq / 2]) / 2.0;
    if (median_out) *median_out = median;
    const double bar = threshold_over_median * median;
    std::vector<int32_t> cand;
    for (int32_t k = 0; k < n_freq; ++k) {
        if (!(power[k] >= bar) || !(power[k] > 0.0)) continue;
        if (k > 0 && !(power[k] > power[k - 1])) continue;            // a plateau's lowest bin is its maximum
        if (k + 1 < n_freq && !(power[k] >= power[k + 1])) continue;
        cand.push_back(k);
    }
    std::stable_sort(cand.begin(), cand.end(), [&](int32_t a, int32_t b) { return power[a] > power[b]; });   // ties: the lowest bin first
    int32_t n_out = 0;
    for (const int32_t k : cand) {
        if (n_out >= max_tones) break;
        bool apart = true;
        for (int32_t j = 0; j < n_out; ++j) {
            const int32_t d = k - out_bins[j];
            if ((d < 0 ? -d : d) < min_separation_bins) apart = false;
        }
        if (apart) out_bins[n_out++] = k;
    }
    return n_out;
}

// gyp_tone_refine's arithmetic (the header states the order): float64, one rounding per operation.
static double tone_refine(const gyp_tone_rec* rec, int32_t n_blocks, double block_seconds) {
#pragma clang fp contract(off)
    double s_re = 0.0, s_im = 0.0;
    for (int32_t b = 0; b + 1 < n_blocks; ++b) {
        const double p = rec[b + 1].re * rec[b].re, q = rec[b + 1].im * rec[b].im;
        const double u = rec[b + 1].im * rec[b].re, v = rec[b + 1].re * rec[b].im;
        const double cr = p + q, ci = u - v;
        s_re += cr;
        s_im += ci;
    }
    const double angle = std::atan2(s_im, s_re);
    const double turn = 6.283185307179586 * block_seconds;
    return angle / turn;
}

// The scan of gyp_ingest_find_tones: grid point k of -kScanHalf .. kScanHalf is round(k fs / 2048) Hz, |f| <= 0.45 fs.
constexpr int32_t kScanDiv = 2048, kScanHalf = 921, kScanBlock = 1024, kScanFine = 64;
static inline int64_t scan_freq(int32_t k, int64_t fs) {
    const int64_t a = ((int64_t)(k < 0 ? -k : k) * fs + kScanDiv / 2) / kScanDiv;
    return k < 0 ? -a : a;
}
// Upper bound of the Hann window's leakage, in power relative to the tone's peak, at a distance of d grid points (two grid points
// are one bin 1/T of the 1024-sample block): |W(x)| / |W(0)| = |sinc(x)| / |1 - x^2| <= 1 / (pi x (x^2 - 1)) for x = d / 2 >= 2;
// inside the main lobe (x < 2) the bound is 1.
static inline double scan_leakage(int32_t d) {
    const double x = 0.5 * (double)(d < 0 ? -d : d);
    if (x < 2.0) return 1.0;
    const double a = 1.0 / (3.141592653589793 * x * (x * x - 1.0));
    return a * a;
}
