// kernels_level.hpp -- signal conditioning of complex64 samples (include/gypsum_hip.h, "level"): per-millisecond DC / power /
// peak / clipping statistics (gyp_iq_stats_dev), the level's application y = (x - dc) * gain (gyp_condition_iq_dev, the ingest's
// in-place pass behind whatever produced a block) and the host arithmetic between the two (gyp_iq_level_from_stats).
//
// Both kernels read 8 bytes per sample once and are HBM-bound; like the widen kernel they walk a persistent grid of at most
// n_cus * widen_wg_per_cu workgroups, because on the upload stream they run beside the trackers.
//
// Statistics.  One 256-thread workgroup per (stream, millisecond) item.  Thread t owns the sample pairs p = t, t + 256, ... of the
// item's row (samples 2p and 2p + 1, counted from the row's first sample; the last pair of an odd row holds one sample) and adds
// them to its three float64 accumulators in that order.  A row that starts on a 16-byte boundary is read as float4 per pair, any
// other row as two float2: which thread adds which sample, and in which order, does not depend on the row's address.  The 256
// partial sums are reduced by a fixed tree -- lane l takes lane l + 32, 16, 8, 4, 2, 1 of its wavefront, then thread 0 adds the
// four wavefronts' sums in order through LDS -- and thread 0 writes the record.  No atomics: a record is a pure function of its
// millisecond's samples, the same bits for every call shape, window and grid size.  Contraction is off, so every product and
// every sum is one float64 rounding; for integer-valued samples with |v| < 2^15 every partial sum is an exact integer below 2^53.
#pragma once

#include <cmath>
#include <cstdint>

__device__ __forceinline__ void level_add(float re, float im, float clip, double& sre, double& sim, double& ssq, float& mx, int32_t& nc) {
#pragma clang fp contract(off)
    const double r = (double)re, i = (double)im;
    sre += r;
    sim += i;
    ssq += r * r;
    ssq += i * i;
    const float ar = fabsf(re), ai = fabsf(im);
    mx = fmaxf(mx, fmaxf(ar, ai));
    nc += (ar >= clip ? 1 : 0) + (ai >= clip ? 1 : 0);
}

__global__ __launch_bounds__(256) void iq_stats_kernel(const float* __restrict__ iq, int64_t stream_stride, int32_t n_ms, int32_t n,
                                                       int64_t n_items, float clip_level, gyp_iq_stats* __restrict__ out) {
    __shared__ double s_re[4], s_im[4], s_sq[4];
    __shared__ float s_mx[4];
    __shared__ int32_t s_nc[4];
    const float clip = clip_level > 0.0f ? clip_level : INFINITY;   // no component reaches it: n_clip stays 0
    const int32_t n_pairs = (n + 1) / 2;
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const int64_t s = it / n_ms, m = it - s * n_ms;
        const float* row = iq + 2 * (s * stream_stride + m * n);
        const bool vec4 = ((uintptr_t)row & 15u) == 0;   // uniform over the workgroup
        double sre = 0.0, sim = 0.0, ssq = 0.0;
        float mx = 0.0f;
        int32_t nc = 0;
        if (vec4) {
#pragma unroll 4
            for (int32_t p = t; p < n_pairs; p += 256) {
                if (2 * p + 1 < n) {
                    const float4 v = reinterpret_cast<const float4*>(row)[p];
                    level_add(v.x, v.y, clip, sre, sim, ssq, mx, nc);
                    level_add(v.z, v.w, clip, sre, sim, ssq, mx, nc);
                } else {
                    const float2 v = reinterpret_cast<const float2*>(row)[2 * p];
                    level_add(v.x, v.y, clip, sre, sim, ssq, mx, nc);
                }
            }
        } else {
#pragma unroll 4
            for (int32_t p = t; p < n_pairs; p += 256) {
                const float2 a = reinterpret_cast<const float2*>(row)[2 * p];
                level_add(a.x, a.y, clip, sre, sim, ssq, mx, nc);
                if (2 * p + 1 < n) {
                    const float2 b = reinterpret_cast<const float2*>(row)[2 * p + 1];
                    level_add(b.x, b.y, clip, sre, sim, ssq, mx, nc);
                }
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            sre += __shfl_down(sre, off, 64);
            sim += __shfl_down(sim, off, 64);
            ssq += __shfl_down(ssq, off, 64);
            mx = fmaxf(mx, __shfl_down(mx, off, 64));
            nc += __shfl_down(nc, off, 64);
        }
        if (lane == 0) {
            s_re[wave] = sre;
            s_im[wave] = sim;
            s_sq[wave] = ssq;
            s_mx[wave] = mx;
            s_nc[wave] = nc;
        }
        __syncthreads();
        if (t == 0) {
            gyp_iq_stats r;
            r.sum_re = ((s_re[0] + s_re[1]) + s_re[2]) + s_re[3];
            r.sum_im = ((s_im[0] + s_im[1]) + s_im[2]) + s_im[3];
            r.sum_sq = ((s_sq[0] + s_sq[1]) + s_sq[2]) + s_sq[3];
            r.max_abs = fmaxf(fmaxf(s_mx[0], s_mx[1]), fmaxf(s_mx[2], s_mx[3]));
            r.n_clip = s_nc[0] + s_nc[1] + s_nc[2] + s_nc[3];
            out[it] = r;
        }
        __syncthreads();   // the next item's partial sums reuse the LDS words
    }
}

// The levels of up to kLevelStreams streams travel as a kernel argument: no device table, nothing to wait for.
constexpr int kLevelStreams = 8;
struct LevelArgs {
    gyp_iq_level v[kLevelStreams];
};

// Stream blockIdx.y of this launch: y = (x - dc) * gain per component, a float32 subtraction and then a float32 multiplication.
// A thread reads what it writes and nothing else, so out may be in.  vec4: every row of both buffers starts 16-byte aligned.
__global__ __launch_bounds__(256) void iq_condition_kernel(const float* in, float* out, int64_t stream_stride, int64_t n_samples,
                                                           LevelArgs levels, int32_t vec4) {
#pragma clang fp contract(off)
    const gyp_iq_level lv = levels.v[blockIdx.y];
    const float* src = in + 2 * (int64_t)blockIdx.y * stream_stride;
    float* dst = out + 2 * (int64_t)blockIdx.y * stream_stride;
    const int64_t first = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    if (vec4) {
        const int64_t n_pairs = n_samples / 2;
        for (int64_t p = first; p < n_pairs; p += stride) {
            const float4 v = reinterpret_cast<const float4*>(src)[p];
            reinterpret_cast<float4*>(dst)[p] = make_float4((v.x - lv.dc_re) * lv.gain, (v.y - lv.dc_im) * lv.gain,
                                                            (v.z - lv.dc_re) * lv.gain, (v.w - lv.dc_im) * lv.gain);
        }
        if ((n_samples & 1) && first == 0) {
            const float2 v = reinterpret_cast<const float2*>(src)[n_samples - 1];
            reinterpret_cast<float2*>(dst)[n_samples - 1] = make_float2((v.x - lv.dc_re) * lv.gain, (v.y - lv.dc_im) * lv.gain);
        }
    } else {
        for (int64_t i = first; i < n_samples; i += stride) {
            const float2 v = reinterpret_cast<const float2*>(src)[i];
            reinterpret_cast<float2*>(dst)[i] = make_float2((v.x - lv.dc_re) * lv.gain, (v.y - lv.dc_im) * lv.gain);
        }
    }
}

// GYP_E_BAD_ARG's reason, or nullptr if the level can be applied.
static const char* level_check(const gyp_iq_level* l) {
    if (!std::isfinite(l->dc_re) || !std::isfinite(l->dc_im)) return "level.dc_re / dc_im must be finite";
    if (!(l->gain > 0.0f) || !std::isfinite(l->gain)) return "level.gain must be positive and finite";
    if (l->reserved != 0) return "level.reserved must be 0";
    return nullptr;
}

// The mean of n_ms milliseconds of samples_per_ms samples from their records, as gyp_iq_level_from_stats and gyp_ingest_find_pulses
// take it: the sums added in index order, then divided by the count, in float64 with one rounding per operation.
struct IqMean { double re, im; };
static IqMean mean_from_stats(const gyp_iq_stats* stats, int32_t n_ms, int32_t samples_per_ms) {
#pragma clang fp contract(off)
    double S_re = 0.0, S_im = 0.0;
    for (int32_t i = 0; i < n_ms; ++i) {
        S_re += stats[i].sum_re;
        S_im += stats[i].sum_im;
    }
    const double M = (double)n_ms * samples_per_ms;
    return IqMean{S_re / M, S_im / M};
}

// gyp_iq_level_from_stats' arithmetic (the header states the order): float64, one rounding per operation -- contraction is off,
// or the compiler would fuse a + b and P - q with the products in front of them.  nullptr, or GYP_E_BAD_ARG's reason.
static const char* level_from_stats(const gyp_iq_stats* stats, int32_t n_ms, int32_t samples_per_ms, int32_t remove_dc, double target_rms,
                                    gyp_iq_level* level_out, double* measured_out4) {
#pragma clang fp contract(off)
    double S_sq = 0.0;
    int64_t C = 0;
    for (int32_t i = 0; i < n_ms; ++i) {
        S_sq += stats[i].sum_sq;
        C += stats[i].n_clip;
    }
    const double M = (double)n_ms * samples_per_ms;
    const IqMean mean = mean_from_stats(stats, n_ms, samples_per_ms);
    const double m_re = mean.re, m_im = mean.im, P = S_sq / M;
    const double d_re = remove_dc ? m_re : 0.0, d_im = remove_dc ? m_im : 0.0;
    const double a = d_re * d_re;
    const double b = d_im * d_im;
    const double q = a + b;
    const double V = P - q;
    if (!(V > 0.0) || !std::isfinite(V)) return "the recording's power about the offset is not positive and finite (a constant recording has none to scale)";
    const double rms = std::sqrt(V);
    const double g = target_rms / rms;
    const gyp_iq_level level = {(float)d_re, (float)d_im, (float)g, 0};
    if (level_check(&level)) return "the level does not fit float32 (offset not finite, or gain zero or not finite)";
    *level_out = level;
    if (measured_out4) {
        measured_out4[0] = m_re;
        measured_out4[1] = m_im;
        measured_out4[2] = rms;
        measured_out4[3] = (double)C / (2.0 * M);
    }
    return nullptr;
}
