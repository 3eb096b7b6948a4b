// kernels_blank.hpp -- pulsed (wideband) interference in complex64 samples (include/gypsum_hip.h, "blanker"): samples whose power
// about a centre reaches a threshold are replaced by the centre together with `guard` neighbours on either side, per millisecond
// (gyp_blank_iq_dev, the ingest's in-place pass between whatever produced a block and the notches); a histogram of that power in
// eighth-octave bins (gyp_iq_power_hist_dev) and the host arithmetic that turns it into a threshold (gyp_blank_from_hist).
//
// Both kernels read 8 bytes per sample once; like the widen kernel they walk a persistent grid of at most n_cus * widen_wg_per_cu
// workgroups, because on the upload stream they run beside the trackers.  On that grid the histogram runs at a copy's rate and the
// blanker, whose two passes per item do not overlap, at about half of it (profiles/blank_kernels.txt).
//
// Power.  dx = re - center_re, dy = im - center_im, a = dx dx, b = dy dy, p = a + b, all float32, one rounding each (contraction
// is off).  A sample is a hit iff p >= threshold * threshold (one float32 product); a NaN p compares false.
//
// Blanking (iq_blank_kernel).  One 256-thread workgroup per (stream, millisecond) item.
//   pass 1  wavefront w takes the chunks c = w, w + 4, ... of the millisecond.  A row that starts on 8 bytes only is read as one
//           float2 per lane (chunk = 64 samples, lane l holds sample 64 c + l) and __ballot of the hit predicate IS hit word c.  A
//           row on 16 bytes is read as one float4 per lane (chunk = 128 samples, lane l holds 128 c + 2 l and the one behind it);
//           the ballots of the even and of the odd samples are interleaved bit by bit into hit words 2 c and 2 c + 1 (on the
//           scalar unit: a ballot is wave-uniform).  Lane 0 stores the words to LDS: ceil(N / 64) words, bit i & 63 of word i >> 6
//           is sample i; bits at and beyond N are zero.
//   barrier
//   pass 2  sample i is blanked iff a bit of [i - guard, i + guard] is set.  With guard <= 64 that range lies in the sample's own
//           word and its two neighbours; which bits of each it covers depends on i & 63 and the guard only, so a lane makes its
//           three masks once and a sample costs three LDS words (the same address over the wavefront: a broadcast), three ANDs and
//           a test.  Words before the first and behind the last read as zero, which is the intersection with [0, N): nothing
//           crosses a millisecond's edge.  __ballot of the blanked predicate is the dilated word; its popcount goes to the item's
//           count through an integer LDS atomic.  The samples come from the registers pass 1 left them in (the first kBlankKeep
//           chunks of each wavefront) or are read again (from L2; a lane re-reads and writes its own samples only).
// In place only blanked samples are stored: the stage costs one read of the block and a few percent of a write.  Out of place
// every sample is stored.  The result is a pure function of the millisecond's samples and the blanker: the same bits for every
// call shape, window, grid size and row alignment.  No floating-point atomics.
//
// Histogram (iq_power_hist_kernel).  Workgroup (x, s) of a launch walks stream s with the persistent grid's stride, counts
// bin = (bits of p without the sign) >> 20 in 2048 LDS words with integer atomics and adds its non-zero bins to the stream's
// global histogram with integer atomics: counts are integers, so the result does not depend on the order.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

constexpr int kBlankThreads = 256;
constexpr int kBlankWaves = kBlankThreads / 64;
constexpr int kBlankKeep = 16;                  // chunks per wavefront kept in registers: 4096 samples by float2, 8192 by float4
constexpr int32_t kBlankMaxSamples = 65536;     // per millisecond: 1024 hit words, 8 KiB of LDS
constexpr int32_t kBlankMaxGuard = 64;

// The blankers / centres of up to kBlankStreams streams travel as a kernel argument: no device table, nothing to wait for.
constexpr int kBlankStreams = 8;
struct BlankArgs {
    gyp_blanker v[kBlankStreams];
};
struct HistArgs {
    float2 c[kBlankStreams];
};

__device__ __forceinline__ float blank_power(float re, float im, float c_re, float c_im) {
#pragma clang fp contract(off)
    const float dx = re - c_re, dy = im - c_im;
    const float a = dx * dx, b = dy * dy;
    return a + b;
}

// Bit k of x to bit 2 k.
__device__ __forceinline__ uint64_t blank_spread(uint32_t x) {
    uint64_t v = x;
    v = (v | (v << 16)) & 0x0000ffff0000ffffull;
    v = (v | (v << 8)) & 0x00ff00ff00ff00ffull;
    v = (v | (v << 4)) & 0x0f0f0f0f0f0f0f0full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & 0x5555555555555555ull;
    return v;
}

// The bits of [b - g, b + g] that fall into the word before the one that holds bit b (0 <= b < 64), into that word and into the
// word behind it, 0 <= g <= 64.
struct BlankMasks {
    uint64_t prev, cur, next;
};
__device__ __forceinline__ BlankMasks blank_masks(int b, int g) {
    BlankMasks m;
    const int lo = b - g > 0 ? b - g : 0, hi = b + g < 63 ? b + g : 63;
    m.cur = (~0ull << lo) & (~0ull >> (63 - hi));
    m.prev = b < g ? ~0ull << (64 + b - g) : 0ull;          // bits 64 + b - g .. 63
    m.next = b + g >= 64 ? ~0ull >> (127 - b - g) : 0ull;   // bits 0 .. b + g - 64
    return m;
}
__device__ __forceinline__ bool blank_test(const BlankMasks& m, uint64_t prev, uint64_t cur, uint64_t next) {
    return ((prev & m.prev) | (cur & m.cur) | (next & m.next)) != 0ull;
}

// VEC4: this item's rows of both buffers start on 16 bytes.  STORE_ALL: out of place.
template <bool VEC4, bool STORE_ALL>
__device__ __forceinline__ void blank_item(const float2* src, float2* dst, int32_t n, const gyp_blanker bl, uint64_t* s_hits, int32_t* s_count) {
#pragma clang fp contract(off)
    constexpr int kPer = VEC4 ? 2 : 1;              // samples per lane and chunk
    constexpr int kChunk = 64 * kPer;
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int32_t n_chunks = (n + kChunk - 1) / kChunk, n_words = (n + 63) >> 6;
    const float t2 = bl.threshold * bl.threshold;
    const float2 centre = make_float2(bl.center_re, bl.center_im);
    float4 keep[kBlankKeep];   // (.xy only by float2)

    auto load = [&](int32_t c) -> float4 {
        const int32_t i = c * kChunk + kPer * lane;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (VEC4 && i + 1 < n) v = *reinterpret_cast<const float4*>(src + i);
        else if (i < n) {
            const float2 a = src[i];
            v.x = a.x, v.y = a.y;
        }
        return v;
    };
    auto hits = [&](int32_t c, const float4& v) {
        const int32_t i = c * kChunk + kPer * lane;
        const bool h0 = i < n && blank_power(v.x, v.y, centre.x, centre.y) >= t2;
        const uint64_t b0 = __ballot(h0);
        if (VEC4) {
            const bool h1 = i + 1 < n && blank_power(v.z, v.w, centre.x, centre.y) >= t2;
            const uint64_t b1 = __ballot(h1);
            if (lane == 0) {
                s_hits[2 * c] = blank_spread((uint32_t)b0) | (blank_spread((uint32_t)b1) << 1);
                if (2 * c + 1 < n_words) s_hits[2 * c + 1] = blank_spread((uint32_t)(b0 >> 32)) | (blank_spread((uint32_t)(b1 >> 32)) << 1);
            }
        } else if (lane == 0) {
            s_hits[c] = b0;
        }
    };

    // pass 1
#pragma unroll
    for (int k = 0; k < kBlankKeep; ++k) {
        const int32_t c = k * kBlankWaves + wave;   // wave-uniform
        if (c < n_chunks) {
            keep[k] = load(c);
            hits(c, keep[k]);
        }
    }
    for (int32_t c = kBlankKeep * kBlankWaves + wave; c < n_chunks; c += kBlankWaves) hits(c, load(c));
    if (t == 0) *s_count = 0;
    __syncthreads();

    // pass 2: a lane's samples sit at the same bits of their words in every chunk
    const int bit0 = (kPer * lane) & 63;
    const BlankMasks m0 = blank_masks(bit0, bl.guard), m1 = blank_masks(VEC4 ? bit0 + 1 : bit0, bl.guard);
    int32_t count = 0;
    auto finish = [&](int32_t c, const float4& v) {
        const int32_t i = c * kChunk + kPer * lane;
        const int32_t w = (c * kChunk >> 6) + (VEC4 ? lane >> 5 : 0);   // the word of this lane's samples
        uint64_t prev = 0ull, cur = 0ull, next = 0ull;
        if (w < n_words) {
            cur = s_hits[w];
            if (w > 0) prev = s_hits[w - 1];
            if (w + 1 < n_words) next = s_hits[w + 1];
        }
        const bool k0 = i < n && blank_test(m0, prev, cur, next);
        const bool k1 = VEC4 && i + 1 < n && blank_test(m1, prev, cur, next);
        count += __popcll(__ballot(k0));
        if (VEC4) count += __popcll(__ballot(k1));
        if (STORE_ALL) {
            if (VEC4 && i + 1 < n)
                *reinterpret_cast<float4*>(dst + i) = make_float4(k0 ? centre.x : v.x, k0 ? centre.y : v.y, k1 ? centre.x : v.z, k1 ? centre.y : v.w);
            else if (i < n) dst[i] = k0 ? centre : make_float2(v.x, v.y);
        } else {
            if (VEC4 && k0 && k1) *reinterpret_cast<float4*>(dst + i) = make_float4(centre.x, centre.y, centre.x, centre.y);
            else {
                if (k0) dst[i] = centre;
                if (k1) dst[i + 1] = centre;
            }
        }
    };
#pragma unroll
    for (int k = 0; k < kBlankKeep; ++k) {
        const int32_t c = k * kBlankWaves + wave;
        if (c < n_chunks) finish(c, keep[k]);
    }
    for (int32_t c = kBlankKeep * kBlankWaves + wave; c < n_chunks; c += kBlankWaves) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (STORE_ALL) v = load(c);   // (in place nothing but the centre is written: no second read at all)
        finish(c, v);
    }
    if (lane == 0 && count) atomicAdd(s_count, count);   // (the count is wave-uniform)
}

// counts may be null.  in may be out (then STORE_ALL is false and only blanked samples are written).
template <bool STORE_ALL>
__global__ __launch_bounds__(kBlankThreads) void iq_blank_kernel(const float2* in, float2* out, int64_t stream_stride, int32_t n_ms, int32_t n,
                                                                 int64_t n_items, BlankArgs blankers, int32_t* counts) {
    __shared__ uint64_t s_hits[kBlankMaxSamples / 64];
    __shared__ int32_t s_count;
    for (int64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const int64_t s = it / n_ms, ms = it - s * n_ms;
        const float2* src = in + s * stream_stride + ms * n;
        float2* dst = out + s * stream_stride + ms * n;
        const bool vec4 = (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0;   // uniform over the workgroup
        if (vec4) blank_item<true, STORE_ALL>(src, dst, n, blankers.v[s], s_hits, &s_count);
        else blank_item<false, STORE_ALL>(src, dst, n, blankers.v[s], s_hits, &s_count);
        __syncthreads();   // every wavefront's count is in; the next item reuses the hit words
        if (threadIdx.x == 0 && counts) counts[it] = s_count;
    }
}

// Workgroup (x, s): stream s of this launch.  hist: this launch's first stream's 2048 words, zeroed by the caller.
__global__ __launch_bounds__(256) void iq_power_hist_kernel(const float2* __restrict__ iq, int64_t stream_stride, int64_t n_samples, HistArgs centres,
                                                            uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_hist[GYP_POWER_HIST_BINS];
    const int t = (int)threadIdx.x;
    for (int b = t; b < GYP_POWER_HIST_BINS; b += 256) s_hist[b] = 0u;
    __syncthreads();
    const float2 c = centres.c[blockIdx.y];
    const float2* row = iq + (int64_t)blockIdx.y * stream_stride;
    auto add = [&](float re, float im) { atomicAdd(&s_hist[(__float_as_uint(blank_power(re, im, c.x, c.y)) & 0x7fffffffu) >> 20], 1u); };
    // the order does not matter to integer counts: a row on 8 bytes only gives up its first sample, and the rest is on 16
    const int64_t head = ((uintptr_t)row & 15u) && n_samples > 0 ? 1 : 0;
    if (head && blockIdx.x == 0 && t == 0) add(row[0].x, row[0].y);
    const float4* body = reinterpret_cast<const float4*>(row + head);
    const int64_t n_pairs = (n_samples - head) / 2;
    const int64_t first = (int64_t)blockIdx.x * 256 + t, stride = (int64_t)gridDim.x * 256;
#pragma unroll 4
    for (int64_t p = first; p < n_pairs; p += stride) {
        const float4 v = body[p];
        add(v.x, v.y);
        add(v.z, v.w);
    }
    if (head + 2 * n_pairs < n_samples && blockIdx.x == 0 && t == 1) add(row[n_samples - 1].x, row[n_samples - 1].y);
    __syncthreads();
    uint32_t* out = hist + (int64_t)blockIdx.y * GYP_POWER_HIST_BINS;
    for (int b = t; b < GYP_POWER_HIST_BINS; b += 256)
        if (s_hist[b]) atomicAdd(&out[b], s_hist[b]);
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
// GYP_E_BAD_ARG's reason, or nullptr if the blanker can be applied.
static const char* blanker_check(const gyp_blanker* b) {
    if (!std::isfinite(b->center_re) || !std::isfinite(b->center_im)) return "blanker.center_re / center_im must be finite";
    if (!(b->threshold > 0.0f) || !std::isfinite(b->threshold)) return "blanker.threshold must be positive and finite";
    if (b->guard < 0 || b->guard > kBlankMaxGuard) return "blanker.guard must lie in 0 .. 64";
    return nullptr;
}

// The lower edge of bin k (0 .. 2048): the float whose bits are k << 20 (bin 2040's is +inf).
static inline double blank_bin_edge(int32_t k) {
    const uint32_t bits = (uint32_t)k << 20;
    float f;
    std::memcpy(&f, &bits, sizeof f);
    return (double)f;
}

// The median of a power histogram and t = sqrt(threshold_over_median * median), the arithmetic gyp_blank_from_hist and
// gyp_excise_from_hist share (the header states the order): float64, one rounding per operation.  nullptr, or GYP_E_BAD_ARG's reason.
static const char* hist_median_threshold(const uint32_t* hist, double threshold_over_median, double* median_out, double* t_out) {
#pragma clang fp contract(off)
    constexpr int32_t kFinite = 2040;   // bins of finite p
    double M = 0.0;
    for (int32_t k = 0; k < kFinite; ++k) M += (double)hist[k];
    if (!(M > 0.0)) return "the histogram holds no sample of finite power";
    const double r = M / 2.0;
    double before = 0.0;
    int32_t k = 0;
    for (; k < kFinite; ++k) {
        if (before + (double)hist[k] >= r) break;
        before += (double)hist[k];
    }
    if (k == kFinite) return "the histogram holds no sample of finite power";   // (unreachable: the last cumulative count is M >= r)
    const double lo = blank_bin_edge(k), width = blank_bin_edge(k + 1) - lo;
    const double part = (r - before) / (double)hist[k];
    const double step = part * width;
    const double median = lo + step;
    if (!(median > 0.0)) return "the median power is not positive";
    const double scaled = threshold_over_median * median;
    *median_out = median;
    *t_out = std::sqrt(scaled);
    return nullptr;
}

// gyp_blank_from_hist behind its argument checks.  nullptr, or GYP_E_BAD_ARG's reason.
static const char* blank_from_hist(const uint32_t* hist, float center_re, float center_im, double threshold_over_median, int32_t guard,
                                   gyp_blanker* blanker_out, double* measured_out2) {
    double median = 0.0, t = 0.0;
    if (const char* why = hist_median_threshold(hist, threshold_over_median, &median, &t)) return why;
    const gyp_blanker b = {center_re, center_im, (float)t, guard};
    if (blanker_check(&b)) return "the blanker does not fit float32 (centre not finite, or threshold zero or not finite)";
    *blanker_out = b;
    if (measured_out2) {
        measured_out2[0] = median;
        measured_out2[1] = t;
    }
    return nullptr;
}
