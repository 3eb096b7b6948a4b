// kernels_resample.hpp -- rational-rate resampler: interleaved I,Q words at fs_in -> complex64 at the stream format's fs_out
// (gyp_resample_iq_dev, gyp_ingest_open_resampled; the contract is written down in include/gypsum_hip.h).
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
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

// One cached design: the taps in the kernel's layout, [T][L] with column p = phase p's taps (design row p*M mod L).
struct ResampleDesign {
    int64_t fs_in = 0, fs_out = 0;
    int32_t taps = 0;
    int32_t n_in = 0, n_out = 0, g = 0, L = 0, M = 0;
    float* d_taps = nullptr;
};

static inline int64_t resample_gcd(int64_t a, int64_t b) {
    while (b) {
        const int64_t t = a % b;
        a = b;
        b = t;
    }
    return a;
}

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

// grid: x = period tiles * phase chunks (chunk fastest), y = streams; dynamic LDS: the largest tile span in float2.
template <class W, int T>
__global__ __launch_bounds__(256) void resample_kernel(const W* __restrict__ raw, int64_t in_stride, int64_t raw_first, int64_t raw_n,
                                                       float scale, const float* __restrict__ taps, int32_t L, int32_t M,
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
    const W* src = raw + stream * in_stride * 2;
    for (int32_t k = threadIdx.x; k < span; k += blockDim.x) {
        const int64_t idx = s0 + k;
        const int64_t rel = idx - raw_first;
        xs[k] = (idx >= 0 && rel >= 0 && rel < raw_n) ? resample_load(src + 2 * rel, scale) : make_float2(0.f, 0.f);
    }
    __syncthreads();
    float2* dst = out + stream * out_stride;
    for (int32_t p = pa + (int32_t)threadIdx.x; p < pb; p += blockDim.x) {
        float h[T];
#pragma unroll
        for (int j = 0; j < T; ++j) h[j] = taps[(size_t)j * L + p];
        const int32_t base = (int32_t)((int64_t)p * M / L - off_a);
        int64_t P = P0;
        // four periods at a time (independent chains), then the rest; the per-output chain is the same either way
        for (; P + 4 <= P1; P += 4) {
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
