// kernels_excise.hpp -- narrowband and swept interference in complex64 samples (include/gypsum_hip.h, "excisor"): per millisecond,
// half-overlapped 256-point transforms behind a periodic Hann window; the bins whose power reaches a threshold, and `guard` bins on
// either side round the ring of 256, are excised: what they held is transformed back and subtracted from the samples
// (gyp_excise_iq_dev, the ingest's in-place pass between the blanker and the notches); a histogram of the bins' power in
// eighth-octave bins (gyp_iq_spectrum_hist_dev) and the host arithmetic that turns it into a threshold (gyp_excise_from_hist).
//
// Frames.  A millisecond of n samples is nh = ceil(n / 128) hops of 128 samples; frame f = 0 .. nh covers hops f - 1 and f (the hop
// before the first and the one behind the last are zeros, and so is what lies behind sample n - 1 in the last hop).  Hop j is the
// upper half of frame j and the lower half of frame j + 1, and y = x - (e_j[upper] + e_(j+1)[lower]) with e_f the inverse transform
// of frame f's excised bins over 256; a frame without an excised bin is not transformed back and contributes nothing, and a hop
// whose two frames both have none is, in place, not written.
//
// Transform.  One wavefront owns a frame: 256 points, four per lane, radix 4, decimation in frequency, float32.  Lane l enters with
// points l + 64 q (q = 0 .. 3) and leaves with bins rev(l) + 64 k, rev = l's three base-4 digits reversed.  The three exchanges
// between the four stages go through a 2 KiB LDS tile that belongs to the wavefront (LDS operations of one wavefront execute in
// order: no barrier, only wave_lds_fence for the compiler).  The nine twiddles a lane needs are the same for every frame: it makes
// them once per launch in float64 (sincospi) and keeps the float32 roundings in registers, as it does its four window values
// w[k] = (float)sin^2(pi k / 256).  Nearest roundings of exact values carry no common bias in |w|.  The inverse is the same
// transform on the conjugate, conjugated and divided by 256 (exact), with one exchange in front and one behind to bring bins and
// samples back to the order lanes hold hops in.
//
// Decision.  p = re re + im im in float32 (no contraction); a hit iff p >= threshold threshold; __ballot of the four hit
// predicates is four words in lane order, a bit permutation (rev is two delta swaps of a 64-bit word) makes them the 256-bit hit
// word in bin order, and the guard's dilation is rotations of that word on the scalar unit.  A NaN anywhere in a frame makes every
// p of the frame NaN: nothing is hit.
//
// In place.  Wavefront w of an item owns a run of neighbouring frames f0 .. f1 - 1 and stores hops f0 .. f1 - 1.  Hop f1 - 1 also
// needs frame f1's lower half: the wavefront walks frame f1 too (its owner does the same arithmetic on the same bits and reports
// its mask and count; one frame more per run, three per item, and the runs are cut so that every wavefront walks as many).  So a wavefront reads hops f0 - 1 .. f1 and stores f0 .. f1 - 1:
// hop f0 - 1 is stored by the run before and hop f1 by the run behind.  THE HAZARD'S RESOLUTION: every wavefront loads these two
// boundary hops into registers in a prologue, then the workgroup passes a barrier, and only then is anything stored.  Inside its
// run a wavefront loads hop f + 1 (into registers, one frame ahead) before it stores hop f - 1, and never reads a hop again.
// The result is a pure function of the millisecond's samples and the excisor: the same bits for every call shape, window, grid
// size and row alignment.  Rows are read and written 8 bytes per lane, 512 contiguous bytes per wavefront and access, whatever the
// row's alignment.  No floating-point atomics.
//
// Histogram (iq_spectrum_hist_kernel).  The same transform of the frames that lie entirely inside their millisecond (f >= 1 and
// 128 f + 128 <= n), bin = (bits of p without the sign) >> 20 counted in 2048 LDS words with integer atomics; a workgroup adds
// its non-zero bins to the stream's global histogram, with integer atomics, when the next item belongs to another stream.
#pragma once

#include <cmath>
#include <cstdint>

constexpr int kExciseThreads = 256;
constexpr int kExciseWaves = kExciseThreads / 64;
constexpr int32_t kExciseHop = GYP_EXCISE_FRAME / 2;
constexpr int32_t kExciseMaxSamples = 65536;   // per millisecond
constexpr int32_t kExciseMaxGuard = 8;
static_assert(GYP_EXCISE_FRAME == 256, "the transform is 256 points: four radix-4 stages, four points per lane");

// The excisors of up to kExciseStreams streams travel as a kernel argument: no device table, nothing to wait for.
constexpr int kExciseStreams = 8;
struct ExciseArgs {
    gyp_excisor v[kExciseStreams];
};

__host__ __device__ inline int32_t excise_frames(int32_t n) { return (n + kExciseHop - 1) / kExciseHop + 1; }   // == ceil((n + 128) / 128)

// What a lane keeps for every frame.
struct ExciseLane {
    float2 tw[3][3];   // stage s = 0 .. 2, output k = 1 .. 3: exp(-2 pi i j k / 256), j = l, 4 (l & 15), 16 (l & 3)
    float win[4];      // w[l + 64 q]
    int rev;           // this lane leaves the transform with bins rev + 64 k
};
__device__ __forceinline__ float2 excise_twiddle(int j) {
    double s, c;
    sincospi(-(double)(j & 255) / 128.0, &s, &c);
    return make_float2((float)c, (float)s);
}
__device__ __forceinline__ ExciseLane excise_lane(int lane) {
    ExciseLane c;
#pragma unroll
    for (int k = 1; k <= 3; ++k) {
        c.tw[0][k - 1] = excise_twiddle(lane * k);
        c.tw[1][k - 1] = excise_twiddle(4 * (lane & 15) * k);
        c.tw[2][k - 1] = excise_twiddle(16 * (lane & 3) * k);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const double s = sinpi((double)(lane + 64 * q) / 256.0);
        c.win[q] = (float)(s * s);
    }
    c.rev = (lane >> 4) | (lane & 12) | ((lane & 3) << 4);
    return c;
}

// v <- the four outputs of a radix-4 butterfly (forward: W4 = -i), outputs 1 .. 3 times tw[0 .. 2].
template <bool TWIDDLE>
__device__ __forceinline__ void excise_butterfly(float2 (&v)[4], const float2 (&tw)[3]) {
#pragma clang fp contract(off)
    const float2 a = make_float2(v[0].x + v[2].x, v[0].y + v[2].y), b = make_float2(v[0].x - v[2].x, v[0].y - v[2].y);
    const float2 c = make_float2(v[1].x + v[3].x, v[1].y + v[3].y), d = make_float2(v[1].x - v[3].x, v[1].y - v[3].y);
    float2 y[4];
    y[0] = make_float2(a.x + c.x, a.y + c.y);
    y[1] = make_float2(b.x + d.y, b.y - d.x);
    y[2] = make_float2(a.x - c.x, a.y - c.y);
    y[3] = make_float2(b.x - d.y, b.y + d.x);
    v[0] = y[0];
#pragma unroll
    for (int k = 1; k < 4; ++k)
        v[k] = TWIDDLE ? make_float2(y[k].x * tw[k - 1].x - y[k].y * tw[k - 1].y, y[k].x * tw[k - 1].y + y[k].y * tw[k - 1].x) : y[k];
}

// Every lane stores v[k] at wr(k) of its wavefront's tile, then loads v[k] from rd(k).
template <class Wr, class Rd>
__device__ __forceinline__ void excise_exchange(float2* tile, float2 (&v)[4], Wr wr, Rd rd) {
    gyp::wave_lds_fence();   // (the reads of the exchange before are through)
#pragma unroll
    for (int k = 0; k < 4; ++k) tile[wr(k)] = v[k];
    gyp::wave_lds_fence();
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = tile[rd(k)];
}

// Points lane + 64 q in, bins c.rev + 64 k out.
__device__ __forceinline__ void excise_fft256(float2 (&v)[4], float2* tile, const ExciseLane& c, int lane) {
    excise_butterfly<true>(v, c.tw[0]);
    excise_exchange(tile, v, [&](int k) { return 64 * k + lane; }, [&](int q) { return 64 * (lane >> 4) + (lane & 15) + 16 * q; });
    excise_butterfly<true>(v, c.tw[1]);
    excise_exchange(tile, v, [&](int k) { return 64 * (lane >> 4) + 16 * k + (lane & 15); }, [&](int q) { return 16 * (lane >> 2) + (lane & 3) + 4 * q; });
    excise_butterfly<true>(v, c.tw[2]);
    excise_exchange(tile, v, [&](int k) { return 16 * (lane >> 2) + 4 * k + (lane & 3); }, [&](int q) { return 4 * lane + q; });
    excise_butterfly<false>(v, c.tw[2]);
}
// Bins c.rev + 64 k (or positions in that order) in, lane + 64 q out.
__device__ __forceinline__ void excise_to_natural(float2 (&v)[4], float2* tile, const ExciseLane& c, int lane) {
    excise_exchange(tile, v, [&](int k) { return c.rev + 64 * k; }, [&](int q) { return lane + 64 * q; });
}

// Bit l of x to bit rev(l): index bits 0 <-> 4 and 1 <-> 5.
__device__ __forceinline__ uint64_t excise_rev_bits(uint64_t x) {
    uint64_t t = ((x >> 15) ^ x) & 0x0000aaaa0000aaaaull;
    x ^= t | (t << 15);
    t = ((x >> 30) ^ x) & 0x00000000ccccccccull;
    x ^= t | (t << 30);
    return x;
}

struct ExciseBits {
    uint64_t w[4];   // bit k & 63 of word k >> 6 is bin k
};
// Every bin within g of a set one, round the ring of 256.  0 <= g <= 8.
__device__ __forceinline__ ExciseBits excise_dilate(const ExciseBits& h, int g) {
    ExciseBits d = h;
    for (int s = 1; s <= g; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i)
            d.w[i] |= (h.w[i] << s) | (h.w[(i + 3) & 3] >> (64 - s)) | (h.w[i] >> s) | (h.w[(i + 1) & 3] << (64 - s));
    return d;
}

// The first frame of wavefront w's run (w = kExciseWaves: nf).  Every run but the last walks one frame more than it owns, so the
// nf + 3 frames walked are spread evenly and the last run owns one more than it would otherwise: 17 frames are 4, 4, 4, 5 owned and
// 5 walked by each.  Below 8 frames: ceil(nf / 4) each while they last.
__device__ __forceinline__ int32_t excise_run_start(int32_t nf, int w) {
    if (nf < 2 * kExciseWaves) return min(w * ((nf + kExciseWaves - 1) / kExciseWaves), nf);
    const int32_t walked = nf + kExciseWaves - 1, q = walked / kExciseWaves, r = walked % kExciseWaves;
    return w == kExciseWaves ? nf : w * (q - 1) + min(w, r);
}

// Hop j of the row: lane l takes samples 128 j + l and 128 j + l + 64; zeros outside 0 .. n - 1.
__device__ __forceinline__ void excise_load_hop(const float2* src, int32_t n, int32_t j, int lane, float2 (&h)[2]) {
    const int32_t i = j * kExciseHop + lane;
    h[0] = j >= 0 && i < n ? src[i] : make_float2(0.f, 0.f);
    h[1] = j >= 0 && i + 64 < n ? src[i + 64] : make_float2(0.f, 0.f);
}

// The frame of hops lo and hi, windowed and transformed: v = its bins, and the power of each.
__device__ __forceinline__ void excise_analyse(const float2 (&lo)[2], const float2 (&hi)[2], float2* tile, const ExciseLane& c, int lane,
                                               float2 (&v)[4], float (&p)[4]) {
#pragma clang fp contract(off)
    v[0] = make_float2(lo[0].x * c.win[0], lo[0].y * c.win[0]);
    v[1] = make_float2(lo[1].x * c.win[1], lo[1].y * c.win[1]);
    v[2] = make_float2(hi[0].x * c.win[2], hi[0].y * c.win[2]);
    v[3] = make_float2(hi[1].x * c.win[3], hi[1].y * c.win[3]);
    excise_fft256(v, tile, c, lane);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float a = v[k].x * v[k].x, b = v[k].y * v[k].y;
        p[k] = a + b;
    }
}

// STORE_ALL: out of place.  masks: this item's 4 words per frame, or null.
template <bool STORE_ALL>
__device__ __forceinline__ void excise_item(const float2* src, float2* dst, int32_t n, const gyp_excisor ex, float2* tile, const ExciseLane& c,
                                            uint64_t* masks, int32_t* s_count) {
#pragma clang fp contract(off)
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int32_t nf = excise_frames(n);
    const int32_t f0 = excise_run_start(nf, wave), f1 = excise_run_start(nf, wave + 1);   // this wavefront's frames (wave-uniform)
    const int32_t f_end = f1 < nf ? f1 + 1 : f1;                      // walked: the run and the first frame behind it
    const float t2 = ex.threshold * ex.threshold;

    // prologue: the hops another run stores, before anyone stores
    float2 lo[2], hi[2], last[2], nxt[2];
    excise_load_hop(src, n, f0 - 1, lane, lo);
    excise_load_hop(src, n, f1, lane, last);
    if (t == 0) *s_count = 0;
    __syncthreads();

    int32_t count = 0;
    if (f0 < f1) {
        float2 up[2] = {make_float2(0.f, 0.f), make_float2(0.f, 0.f)};   // the frame before's correction of its upper half
        bool up_any = false;
        excise_load_hop(src, n, f0, lane, hi);
        for (int32_t f = f0; f < f_end; ++f) {
            if (f + 1 == f1) nxt[0] = last[0], nxt[1] = last[1];
            else if (f + 1 < f_end) excise_load_hop(src, n, f + 1, lane, nxt);
            float2 v[4];
            float p[4];
            excise_analyse(lo, hi, tile, c, lane, v, p);
            ExciseBits cut;   // first the hits in lane order, then (where there are any) the excised bins in bin order
#pragma unroll
            for (int k = 0; k < 4; ++k) cut.w[k] = __ballot(p[k] >= t2);
            const bool any_hit = (cut.w[0] | cut.w[1] | cut.w[2] | cut.w[3]) != 0ull;
            if (any_hit) {
#pragma unroll
                for (int k = 0; k < 4; ++k) cut.w[k] = excise_rev_bits(cut.w[k]);
                cut = excise_dilate(cut, ex.guard);
            }
            if (f < f1) {   // the owner reports
                count += __popcll(cut.w[0]) + __popcll(cut.w[1]) + __popcll(cut.w[2]) + __popcll(cut.w[3]);
                if (masks && lane < 4) masks[(int64_t)f * 4 + lane] = lane == 0 ? cut.w[0] : lane == 1 ? cut.w[1] : lane == 2 ? cut.w[2] : cut.w[3];
            }
            if (any_hit) {
                // what the excised bins held, back in the samples' order: e = conj(FFT(conj(E))) / 256
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool on = (cut.w[k] >> c.rev) & 1ull;
                    v[k] = on ? make_float2(v[k].x, -v[k].y) : make_float2(0.f, 0.f);
                }
                excise_to_natural(v, tile, c, lane);
                excise_fft256(v, tile, c, lane);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = make_float2(v[k].x * (1.0f / 256.0f), -v[k].y * (1.0f / 256.0f));
                excise_to_natural(v, tile, c, lane);
            }
            // hop f - 1 has both its frames now (the first hop walked belongs to the run before)
            if (f > f0 && (STORE_ALL || up_any || any_hit)) {
                const int32_t i = (f - 1) * kExciseHop + lane;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    float2 y = lo[h];
                    if (up_any || any_hit) {
                        const float2 corr = up_any && any_hit ? make_float2(up[h].x + v[h].x, up[h].y + v[h].y) : up_any ? up[h] : v[h];
                        y = make_float2(lo[h].x - corr.x, lo[h].y - corr.y);
                    }
                    if (i + 64 * h < n) dst[i + 64 * h] = y;
                }
            }
            up[0] = v[2], up[1] = v[3], up_any = any_hit;
            lo[0] = hi[0], lo[1] = hi[1];
            hi[0] = nxt[0], hi[1] = nxt[1];
        }
    }
    if (lane == 0 && count) atomicAdd(s_count, count);   // (the count is wave-uniform)
}

// counts and masks may be null.  in may be out (then STORE_ALL is false and only corrected hops are written).
template <bool STORE_ALL>
__global__ __launch_bounds__(kExciseThreads) void iq_excise_kernel(const float2* in, float2* out, int64_t stream_stride, int32_t n_ms, int32_t n,
                                                                   int64_t n_items, ExciseArgs excisors, int32_t* counts, uint64_t* masks) {
    __shared__ float2 s_tile[kExciseWaves][GYP_EXCISE_FRAME];
    __shared__ int32_t s_count;
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const ExciseLane c = excise_lane(lane);
    const int64_t nf = excise_frames(n);
    for (int64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const int64_t s = it / n_ms, ms = it - s * n_ms;
        const float2* src = in + s * stream_stride + ms * n;
        float2* dst = out + s * stream_stride + ms * n;
        excise_item<STORE_ALL>(src, dst, n, excisors.v[s], s_tile[wave], c, masks ? masks + it * nf * 4 : nullptr, &s_count);
        __syncthreads();   // every wavefront's count is in
        if (threadIdx.x == 0 && counts) counts[it] = s_count;
    }
}

// One workgroup per (stream, millisecond) item.  hist: n_streams x 2048 words, zeroed by the caller.  n >= 256.
__global__ __launch_bounds__(kExciseThreads) void iq_spectrum_hist_kernel(const float2* __restrict__ iq, int64_t stream_stride, int32_t n_ms, int32_t n,
                                                                          int64_t n_items, uint32_t* __restrict__ hist) {
    __shared__ float2 s_tile[kExciseWaves][GYP_EXCISE_FRAME];
    __shared__ uint32_t s_hist[GYP_POWER_HIST_BINS];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const ExciseLane c = excise_lane(lane);
    for (int b = t; b < GYP_POWER_HIST_BINS; b += kExciseThreads) s_hist[b] = 0u;
    __syncthreads();
    // the frames inside the millisecond are 1 .. n_full; this wavefront's run of them
    const int32_t n_full = n / kExciseHop - 1, run = (n_full + kExciseWaves - 1) / kExciseWaves;
    const int32_t f0 = min(1 + wave * run, n_full + 1), f1 = min(f0 + run, n_full + 1);
    for (int64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        const int64_t s = it / n_ms, ms = it - s * n_ms;
        const float2* src = iq + s * stream_stride + ms * n;
        float2 lo[2], hi[2];
        excise_load_hop(src, n, f0 - 1, lane, lo);
        for (int32_t f = f0; f < f1; ++f) {
            excise_load_hop(src, n, f, lane, hi);
            float2 v[4];
            float p[4];
            excise_analyse(lo, hi, s_tile[wave], c, lane, v, p);
#pragma unroll
            for (int k = 0; k < 4; ++k) atomicAdd(&s_hist[(__float_as_uint(p[k]) & 0x7fffffffu) >> 20], 1u);
            lo[0] = hi[0], lo[1] = hi[1];
        }
        const int64_t it_next = it + gridDim.x;
        if (it_next >= n_items || it_next / n_ms != s) {   // uniform over the workgroup
            __syncthreads();
            uint32_t* out = hist + s * GYP_POWER_HIST_BINS;
            for (int b = t; b < GYP_POWER_HIST_BINS; b += kExciseThreads)
                if (s_hist[b]) {
                    atomicAdd(&out[b], s_hist[b]);
                    s_hist[b] = 0u;
                }
            __syncthreads();
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------
// GYP_E_BAD_ARG's reason, or nullptr if the excisor can be applied.
static const char* excisor_check(const gyp_excisor* e) {
    if (!(e->threshold > 0.0f) || !std::isfinite(e->threshold)) return "excisor.threshold must be positive and finite";
    if (e->guard < 0 || e->guard > kExciseMaxGuard) return "excisor.guard must lie in 0 .. 8";
    if (e->reserved[0] != 0 || e->reserved[1] != 0) return "excisor.reserved must be 0";
    return nullptr;
}

// gyp_excise_from_hist's arithmetic: the blanker's median and threshold (hist_median_threshold, kernels_blank.hpp).  nullptr, or
// GYP_E_BAD_ARG's reason.
static const char* excise_from_hist(const uint32_t* hist, double threshold_over_median, int32_t guard, gyp_excisor* excisor_out,
                                    double* measured_out2) {
    double median = 0.0, t = 0.0;
    if (const char* why = hist_median_threshold(hist, threshold_over_median, &median, &t)) return why;
    const gyp_excisor e = {(float)t, guard, {0, 0}};
    if (excisor_check(&e)) return "the excisor does not fit float32 (threshold zero or not finite)";
    *excisor_out = e;
    if (measured_out2) {
        measured_out2[0] = median;
        measured_out2[1] = t;
    }
    return nullptr;
}
