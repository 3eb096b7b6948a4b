// kernels_resample.hpp -- rational-rate resampler: interleaved I,Q words at fs_in -> complex64 at the stream format's fs_out
// (gyp_resample_iq_dev, gyp_ingest_open_resampled), and the digital down-converter in front of the same filter: real words at an
// intermediate frequency -> complex baseband (gyp_ddc_iq_dev, gyp_ingest_open_ddc).  The contracts are written down in
// include/gypsum_hip.h ("resampler", "down-converter").
//
// Both rates are whole kHz.  With g = gcd(N_in, N_out), L = N_out / g and M = N_in / g the phase pattern repeats every L outputs
// and M inputs: output n = P*L + p (period P, phase p) sits at input instant P*M + p*M/L, i.e. at the integer base
// P*M + off(p), off(p) = floor(p*M / L), with fraction mu = (p*M mod L) / L.  Millisecond m holds periods m*g .. m*g+g-1.
//
// A workgroup owns one tile of one stream: periods [P0, P1) x phases [pa, pb).  It stages the tile's input span, widened to
// float2, in LDS; then each lane holds one phase's T taps in registers and produces that phase's output in every period of the
// tile, so the taps are read once per tile instead of once per output, and neighbouring lanes read neighbouring LDS samples and
// write neighbouring outputs.  Every output is the same chain of fmaf over its T taps in tap order whatever the tile, the
// window or the launch, so blocks, windowed calls and seeks give bit-identical samples.
//
// The staging step is a compile-time policy: StageIQ widens an I,Q word pair to float2; StageReal widens one real word and
// multiplies it by the mixer exp(-j 2 pi ((if_hz * i) mod fs_in) / fs_in) of its absolute input index i, a pure function of i
// (exact integer phase, no accumulator), so the bit-identity argument above carries over unchanged.
//
// Packed recordings (1-, 2- or 4-bit words, include/gypsum_hip.h "packed recordings") stage through StageIQPacked / StageRealPacked:
// a sample's code comes out of its one byte at its bit offset and its value is a table entry levels[code] * scale, the same single
// float32 multiply as (float)word * scale.  After the staging step nothing differs, so packed and int8 words holding the same levels
// give the same bits.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "resample_plan.hpp"   // the host side's ratio, tiling and mixer constants

// One cached design: the ratio of its rates (n_in, n_out, g, L, M) and the taps in the kernel's layout, [T][L] with column p =
// phase p's taps (design row p*M mod L).
struct ResampleDesign : gyp::ResampleRatio {
    int64_t fs_in = 0, fs_out = 0;
    int32_t taps = 0;
    bool real = false;   // the down-converter's (real words at an IF); the cache key includes it
    float* d_taps = nullptr;
};

// taps: 0 -> 32; otherwise one of 16, 24, 32, 48, 64.  Returns 0 if not allowed.
static inline int32_t resample_taps(int32_t taps) {
    if (taps == 0) return 32;
    return (taps == 16 || taps == 24 || taps == 32 || taps == 48 || taps == 64) ? taps : 0;
}

// Rates the resampler accepts: whole kHz, 0.5 <= fs_out / fs_in <= 2, fs_in != fs_out.
static inline bool resample_rates_ok(int64_t fs_in, int64_t fs_out) {
    if (fs_in <= 0 || fs_out <= 0 || fs_in % 1000 || fs_out % 1000 || fs_in == fs_out) return false;
    return 2 * fs_out >= fs_in && fs_out <= 2 * fs_in;
}

// Down-converter taps: 0 -> the smallest of 32, 48, 64, 96, 128 with T * fs_out >= 16 * fs_in (the filter spans >= 16 outputs);
// otherwise one of those five.  Returns 0 if not allowed (or if 0 cannot be resolved, which ddc_rates_ok rules out).
static inline int32_t ddc_taps(int32_t taps, int64_t fs_in, int64_t fs_out) {
    static const int32_t kTaps[] = {32, 48, 64, 96, 128};
    for (int32_t t : kTaps)
        if (taps == t || (taps == 0 && t * fs_out >= 16 * fs_in)) return t;
    return 0;
}

// Rates and IF the down-converter accepts, in integers: whole kHz, fs_in < 2^31 Hz, 8 fs_out >= fs_in, 20 |if| >= 9 fs_out (the
// mirror band at -2 if clears the +-0.45 fs_out passband), 20 |if| + 9 fs_out <= 10 fs_in (the band lies below the real Nyquist).
static inline bool ddc_rates_ok(int64_t fs_in, int64_t fs_out, int64_t if_hz) {
    if (fs_in <= 0 || fs_out <= 0 || fs_in % 1000 || fs_out % 1000 || fs_in > INT32_MAX || fs_out > fs_in) return false;
    if (if_hz < -fs_in || if_hz > fs_in) return false;   // keeps 20 |if| in range; the last rule refuses these anyway
    const int64_t a = if_hz < 0 ? -if_hz : if_hz;
    return 8 * fs_out >= fs_in && 20 * a >= 9 * fs_out && 20 * a + 9 * fs_out <= 10 * fs_in;
}

static double resample_i0(double x) {   // modified Bessel function of the first kind, order 0 (power series; x <= 8 here)
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

// The L x T design, phase-major (row = mu * L), in float64, then rounded to float32.
//   h_mu[j] = c(j - mu) / sum_j' c(j' - mu),  j = -T/2+1 .. T/2
//   c(t) = fc * sinc(fc * t) * I0(beta * sqrt(1 - (t / (T/2))^2)) / I0(beta),  fc = 0.9 * min(fs_in, fs_out) / fs_in,  beta = 8
static void resample_design_rows(int64_t fs_in, int64_t fs_out, int32_t T, int32_t L, float* table) {
    const double kPi = 3.14159265358979323846;
    const double rho = 0.9, beta = 8.0;
    const double fc = rho * (double)std::min(fs_in, fs_out) / (double)fs_in;
    const double i0b = resample_i0(beta);
    const double half = 0.5 * T;
    std::vector<double> c((size_t)T);
    for (int32_t row = 0; row < L; ++row) {
        const double mu = (double)row / (double)L;
        double sum = 0.0;
        for (int32_t k = 0; k < T; ++k) {
            const double t = (double)(k - T / 2 + 1) - mu;
            const double a = fc * t;
            const double sinc = a == 0.0 ? 1.0 : std::sin(kPi * a) / (kPi * a);
            const double r = t / half;
            const double w = resample_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
            c[(size_t)k] = fc * sinc * w;
            sum += c[(size_t)k];
        }
        for (int32_t k = 0; k < T; ++k) table[(size_t)row * T + k] = (float)(c[(size_t)k] / sum);
    }
}

template <class W>
__device__ __forceinline__ float2 resample_load(const W* __restrict__ s, float scale) {
    return make_float2((float)s[0] * scale, (float)s[1] * scale);
}

// exp(-j 2 pi r / fs) for 0 <= r < fs, in float32 within 2^-22 of the exact value.  The nearest quarter turn k = rint(4 r / fs)
// comes off exactly in integers (e = 4 r - k fs, |e| <= fs / 2), so sincospif sees |y| = |e| / (2 fs) <= 1/4 with an argument
// error of at most half a float32 ulp there (2^-27: pi 2^-27 rad), and its own error is about an ulp of values below 1
// (2^-24); the quarter turn is an exact swap and sign change.  A function of r alone: the same r gives the same bits.
__device__ __forceinline__ float2 ddc_mixer(int64_t r, int64_t fs, double q_scale, double y_scale) {
    const int64_t k = (int64_t)rint((double)r * q_scale);
    const float y = (float)((double)(4 * r - k * fs) * y_scale);
    float s, c;
    sincospif(y, &s, &c);                   // theta = pi/2 k + pi y
    const int q = (int)(k & 3);
    const float ct = q == 0 ? c : q == 1 ? -s : q == 2 ? -c : s;
    const float st = q == 0 ? s : q == 1 ? c : q == 2 ? -s : -c;
    return make_float2(ct, -st);
}

// Staging policies of resample_kernel: xs[k] = the filter input at absolute index s0 + k (zero outside [0, ...) and outside the
// buffer's raw_n samples, which start at index raw_first).
// Each policy is its W-independent parameter block plus the staging loop for word type W.
struct StageIQParams {
    float scale;
};
struct StageRealParams {
    float scale;
    int64_t fs;        // fs_in (< 2^31)
    int64_t f;         // if_hz mod fs, in [0, fs)
    double q_scale;    // 4 / fs
    double y_scale;    // 1 / (2 fs)
};

template <class W>
struct StageIQ : StageIQParams {   // interleaved I,Q words: (I, Q) * scale
    using Word = W;
    using Params = StageIQParams;
    static constexpr int kWords = 2;   // words per sample
    static constexpr bool kReal = false;   // the down-converter's tap counts (resample_launch_taps)
    static constexpr bool kSplitPeriods = false;   // lanes split the tile's periods too (see resample_kernel)
    __device__ __forceinline__ void stage(float2* xs, const W* __restrict__ src, int64_t s0, int32_t span, int64_t raw_first,
                                          int64_t raw_n) const {
        for (int32_t k = threadIdx.x; k < span; k += blockDim.x) {
            const int64_t idx = s0 + k;
            const int64_t rel = idx - raw_first;
            xs[k] = (idx >= 0 && rel >= 0 && rel < raw_n) ? resample_load(src + 2 * rel, scale) : make_float2(0.f, 0.f);
        }
    }
};

template <class W>
struct StageReal : StageRealParams {   // real words at an IF: word * scale * exp(-j 2 pi ((if_hz * i) mod fs) / fs)
    using Word = W;
    using Params = StageRealParams;
    static constexpr int kWords = 1;
    static constexpr bool kReal = true;
    static constexpr bool kSplitPeriods = true;
    __device__ __forceinline__ void stage(float2* xs, const W* __restrict__ src, int64_t s0, int32_t span, int64_t raw_first,
                                          int64_t raw_n) const {
        // r = (f * i) mod fs, exactly: one 64-bit reduction of this lane's first index, then steps of blockDim samples in
        // integers below 2^32 (f, r, step < fs < 2^31)
        int64_t i = (s0 + (int64_t)threadIdx.x) % fs;
        if (i < 0) i += fs;
        int64_t r = f * i % fs;
        const int64_t step = f * (int64_t)blockDim.x % fs;
        for (int32_t k = threadIdx.x; k < span; k += blockDim.x) {
            const int64_t idx = s0 + k;
            const int64_t rel = idx - raw_first;
            const float x = (idx >= 0 && rel >= 0 && rel < raw_n) ? (float)src[rel] * scale : 0.f;
            const float2 m = ddc_mixer(r, fs, q_scale, y_scale);
            xs[k] = make_float2(x * m.x, x * m.y);
            r += step;
            if (r >= fs) r -= fs;
        }
    }
};

// --- packed words -------------------------------------------------------------------------------------------------------------
// The levels a packing gives its codes, before scale (entries >= 2^bits unused).  The kernels read them from a 16-float table in
// device memory (cached on the context): passed by value in the kernel arguments, the same 16 floats made the scheduler double
// resample_kernel's registers at T = 16 and 24 (6 -> 3 waves per SIMD).
struct PackedLevels {
    float v[16];
};

// levels[c] * scale into an LDS table, one lane per entry: the lookup of a code is then one LDS read, never a dynamically
// indexed register array (scratch).  The caller syncs before reading the table.
template <int BITS>
__device__ __forceinline__ void packed_table(float* tab, const float* __restrict__ levels, float scale) {
    if (threadIdx.x < (1u << BITS)) tab[threadIdx.x] = levels[threadIdx.x] * scale;
}

// The code of the word `slot` bits into byte `b` (slot a multiple of BITS below 8), in the packing's bit order.
template <int BITS>
__device__ __forceinline__ uint32_t packed_code(uint32_t b, uint32_t slot, bool msb_first) {
    const uint32_t sh = msb_first ? 8u - BITS - slot : slot;
    return (b >> sh) & ((1u << BITS) - 1u);
}

struct StagePackedParams {
    const float* levels; // 16 floats in device memory
    float scale;
    int32_t order;       // GYP_PACK_MSB_FIRST / GYP_PACK_LSB_FIRST
    int32_t bit0;        // bit offset of the buffer's sample 0 in its first byte
};
struct StageRealPackedParams : StagePackedParams {
    int64_t fs;          // as StageRealParams
    int64_t f;
    double q_scale;
    double y_scale;
};

template <int BITS>
struct StageIQPacked : StagePackedParams {   // I,Q words packed BITS to a word: (levels[cI], levels[cQ]) * scale
    using Word = uint8_t;
    using Params = StagePackedParams;
    static constexpr int kWords = 1;   // strides count bytes
    static constexpr bool kReal = false;
    static constexpr bool kSplitPeriods = false;
    __device__ __forceinline__ void stage(float2* xs, const uint8_t* __restrict__ src, int64_t s0, int32_t span, int64_t raw_first,
                                          int64_t raw_n) const {
        __shared__ float tab[16];
        packed_table<BITS>(tab, levels, scale);
        __syncthreads();
        const bool msb = order == GYP_PACK_MSB_FIRST;
        for (int32_t k = threadIdx.x; k < span; k += blockDim.x) {
            const int64_t idx = s0 + k;
            const int64_t rel = idx - raw_first;
            float2 x = make_float2(0.f, 0.f);
            if (idx >= 0 && rel >= 0 && rel < raw_n) {
                const int64_t pos = bit0 + rel * (2 * BITS);   // a sample's 2 BITS bits never straddle a byte
                const uint32_t b = src[pos >> 3], slot = (uint32_t)(pos & 7);
                x = make_float2(tab[packed_code<BITS>(b, slot, msb)], tab[packed_code<BITS>(b, slot + BITS, msb)]);
            }
            xs[k] = x;
        }
    }
};

template <int BITS>
struct StageRealPacked : StageRealPackedParams {   // real words packed BITS to a word, mixed down as StageReal does
    using Word = uint8_t;
    using Params = StageRealPackedParams;
    static constexpr int kWords = 1;
    static constexpr bool kReal = true;
    static constexpr bool kSplitPeriods = true;
    __device__ __forceinline__ void stage(float2* xs, const uint8_t* __restrict__ src, int64_t s0, int32_t span, int64_t raw_first,
                                          int64_t raw_n) const {
        __shared__ float tab[16];
        packed_table<BITS>(tab, levels, scale);
        __syncthreads();
        const bool msb = order == GYP_PACK_MSB_FIRST;
        int64_t i = (s0 + (int64_t)threadIdx.x) % fs;   // the mixer index exactly as StageReal steps it
        if (i < 0) i += fs;
        int64_t r = f * i % fs;
        const int64_t step = f * (int64_t)blockDim.x % fs;
        for (int32_t k = threadIdx.x; k < span; k += blockDim.x) {
            const int64_t idx = s0 + k;
            const int64_t rel = idx - raw_first;
            float x = 0.f;
            if (idx >= 0 && rel >= 0 && rel < raw_n) {
                const int64_t pos = bit0 + rel * BITS;
                x = tab[packed_code<BITS>(src[pos >> 3], (uint32_t)(pos & 7), msb)];
            }
            const float2 m = ddc_mixer(r, fs, q_scale, y_scale);
            xs[k] = make_float2(x * m.x, x * m.y);
            r += step;
            if (r >= fs) r -= fs;
        }
    }
};

// grid: x = period tiles * phase chunks (chunk fastest), y = streams; dynamic LDS: the largest tile span in float2.
template <class S, int T>
__global__ __launch_bounds__(256) void resample_kernel(const typename S::Word* __restrict__ raw, int64_t in_stride, int64_t raw_first,
                                                       int64_t raw_n, S stage, const float* __restrict__ taps, int32_t L, int32_t M,
                                                       int64_t p_first, int64_t n_periods, int32_t np_tile, int32_t pc_tile,
                                                       int32_t n_pchunks, float2* __restrict__ out, int64_t out_stride) {
    extern __shared__ float2 xs[];
    const int64_t stream = blockIdx.y;
    const int32_t chunk = (int32_t)(blockIdx.x % (uint32_t)n_pchunks);
    const int64_t ptile = blockIdx.x / (uint32_t)n_pchunks;
    const int64_t P0 = p_first + ptile * np_tile;
    const int64_t P1 = P0 + np_tile < p_first + n_periods ? P0 + np_tile : p_first + n_periods;
    const int32_t pa = chunk * pc_tile;
    const int32_t pb = pa + pc_tile < L ? pa + pc_tile : L;
    const int64_t off_a = (int64_t)pa * M / L;
    const int64_t off_b = (int64_t)(pb - 1) * M / L;
    // input samples s0 .. s0+span-1: from tap -T/2+1 of (P0, pa) to tap T/2 of (P1-1, pb-1)
    const int64_t s0 = P0 * M + off_a - (T / 2 - 1);
    const int32_t span = (int32_t)((P1 - 1 - P0) * M + off_b - off_a + T);
    stage.stage(xs, raw + stream * in_stride * S::kWords, s0, span, raw_first, raw_n);
    __syncthreads();
    float2* dst = out + stream * out_stride;
    // Lanes over (phase, group of four periods).  StageIQ: one lane per phase, every period of the tile.  StageReal also splits
    // the periods when the tile has fewer phases than lanes, as its ratios often do (L = 1 at 16.368 -> 4.092, 3 at
    // 38.192 -> 8.184): lane (p, grp) takes the quads grp, grp + n_grp, ...  Which lane computes an output changes, its chain not.
    int32_t lane = threadIdx.x, grp = 0, n_grp = 1;
    uint32_t lanes = 0;
    if constexpr (S::kSplitPeriods) {
        const int32_t nph = pb - pa;
        if (nph < (int32_t)blockDim.x) {
            n_grp = (int32_t)blockDim.x / nph;
            grp = (int32_t)threadIdx.x / nph;
            lane = grp < n_grp ? (int32_t)threadIdx.x % nph : nph;   // the blockDim % nph lanes left over idle
            lanes = (uint32_t)nph;
        } else {
            lanes = blockDim.x;
        }
    }
    for (int32_t p = pa + lane; p < pb; p += S::kSplitPeriods ? lanes : blockDim.x) {
        float h[T];
#pragma unroll
        for (int j = 0; j < T; ++j) h[j] = taps[(size_t)j * L + p];
        const int32_t base = (int32_t)((int64_t)p * M / L - off_a);
        int64_t P = P0 + 4 * grp;
        // four periods at a time (independent chains), then the rest; the per-output chain is the same either way
        for (; P + 4 <= P1; P += 4 * n_grp) {
            const float2* x0 = xs + (int32_t)(P - P0) * M + base;
            float re[4] = {0.f, 0.f, 0.f, 0.f}, im[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < T; ++j) {
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float2 x = x0[q * M + j];
                    re[q] = __builtin_fmaf(h[j], x.x, re[q]);
                    im[q] = __builtin_fmaf(h[j], x.y, im[q]);
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) dst[(P + q - p_first) * L + p] = make_float2(re[q], im[q]);
        }
        for (; P < P1; ++P) {
            const float2* x0 = xs + (int32_t)(P - P0) * M + base;
            float re = 0.f, im = 0.f;
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const float2 x = x0[j];
                re = __builtin_fmaf(h[j], x.x, re);
                im = __builtin_fmaf(h[j], x.y, im);
            }
            dst[(P - p_first) * L + p] = make_float2(re, im);
        }
    }
}
