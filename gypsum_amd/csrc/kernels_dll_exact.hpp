// kernels_dll_exact.hpp -- the code loop re-integrated exactly behind the block tracking kernels.
// A part of kernels.hpp (which lists every kernel); the parts build on each other in the order kernels.hpp includes them.
#pragma once
#include "kernels_track_block.hpp"

namespace gyp {

// ---------------------------------------------------------------------------------------------------------
// The code loop, exactly.  Both block tracking kernels advance their code phase on a PROVISIONAL discriminator (float32
// taps).  The code loop is a side chain -- nothing else of the tracker reads it -- so its exact trajectory is formed
// afterwards from the hand-over records (SpecIn: the Doppler, carrier phase and code phase each millisecond ran with):
//   dll_exact_wave_kernel / dll_exact_block_kernel   tracker.py:297 in float64 for every (channel, millisecond) at the lag the
//                       tracking kernel used: raw float32 samples x float64 carrier, float64 sums; all of them in parallel;
//   dll_scan_kernel     one workgroup per channel, the milliseconds in order: tracker.py:298-303 from those values.  Where
//                       its int(self.phase) differs from the provisional one (the two accumulators straddle an integer: about
//                       once per 1e6 channel-ms, for a few milliseconds each time) the millisecond's sums are formed on the
//                       spot for the right lag (a "repair" step) and the record's code phase / peak offset corrected.
// The exact state travels in DllExact from sub-block to sub-block and is written back into the channel state by the last scan
// of a call, so the next call -- and its provisional loop -- starts from it.
// ---------------------------------------------------------------------------------------------------------
struct DllExactParams {
    const cf* iq;
    int64_t stream_stride;
    int32_t n_ms, ms_begin, ms_end;
    const double* start_time;
    const ChanState* states;
    int32_t n_chan;
    const SpecIn* spec;
    double* disc_out;          // [n_chan][n_ms]
    const float* chipf;        // CodeTables::chipf
    double inv_fs;
    const int32_t* only_if;    // optional: only channels with only_if[ch] != 0 (the re-run of failed speculations) ...
    const int32_t* from_sub;   // ... and of those only the milliseconds from sub-block from_sub[ch] on (SubLayout)
    SubLayout sub;
    const int32_t* trk_round;  // round protocol (SpecCtl): channel ch's milliseconds are sub-block trk_round[ch] (-1: none); null: [ms_begin, ms_end)
};

// acc * w + x  (complex): one Horner step of sum_i x_i w^i
__device__ __forceinline__ double2 horner64(double2 acc, double2 w, double2 x) {
    return make_double2(fma(acc.x, w.x, fma(-acc.y, w.y, x.x)), fma(acc.x, w.y, fma(acc.y, w.x, x.y)));
}
__device__ __forceinline__ double2 cvt64(cf x) { return make_double2((double)x.x, (double)x.y); }
__device__ __forceinline__ double2 cvt64(double2 x) { return x; }   // (samples staged in LDS are converted already)
// One wavefront per (channel, millisecond), any K <= 8.  With s = K q + r the samples are taken in REPLICA-aligned windows:
// "virtual chip" m (m = -1 .. 1022) is the K samples n = K m + r + i, i < K -- exactly the samples that meet replica chip
// j = (m - q) mod 1023 at lag s -- so no window is split between two code chips and nothing in the arithmetic depends on r
// (it only moves the load address by r samples; the vector loads are 8-byte aligned).  The circular block is cut at its ends:
// window -1 holds the first r samples (its i < K - r fall before the block: zero), window 1022 the last K - r; both meet
// replica chip (1022 - q) mod 1023, and the carrier of sample n is exp(-2 pi i (u0 + du n)) for either.  1024 windows = 64
// lanes x 16: lane l owns m = l + 64 c - 1 (consecutive lanes read consecutive 8K-byte pieces).  Per window
//     h = sum_i x_i rho^i  (Horner, rho = exp(-2 pi i du)),   P += chip[j] h,
//     E += (chip[j] - chip[j+1]) x_{K-1}  (lag s-1 sees the next replica chip at a window's last sample),
//     L += (chip[j-1] - chip[j]) x_0      (lag s+1 the previous one at its first);
// windows are folded last one first with the window-stride rotation S = rho^(64 K) (Horner again: acc = acc S + term), the
// lane's anchor carrier (times rho^(K-1) for E) is applied once at the end, six DPP reductions finish the unit.  No LDS, no
// barrier; ~46 float64 operations + 19 converts per window.
// dll_exact_shared_kernel folds the same windows out of LDS: there is ONE copy of the window arithmetic, so the two agree bit for bit.
struct ExactChips { float cm1, c0, cp1; };           // replica chips j - 1, j, j + 1 of a window
__device__ __forceinline__ ExactChips exact_window_chips(const float* chipf, int m, int q) {
    int j = m - q;
    j = j < 0 ? j + kChips : j;                      // (m - q) mod 1023 for m >= 0; m = -1 -> (1022 - q) mod 1023 (q <= 1022)
    j = j < 0 ? j + kChips : j;
    const float* cp = chipf + j + kChips;
    return ExactChips{cp[-1], cp[0], cp[1]};
}
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Walign-mismatch"   // two samples in one 16-byte load at any sample offset: 8-byte alignment is intended
typedef float4 __attribute__((aligned(8))) float4_a8;
__device__ __forceinline__ float4 load_pair_a8(const cf* src, int pair = 0) { return reinterpret_cast<const float4_a8*>(src)[pair]; }
#pragma clang diagnostic pop
template <int K, bool EDGE>
__device__ __forceinline__ ExactChips exact_window_load(const cf* __restrict__ block, int m, int r, int q, const float* __restrict__ chipf, cf (&x)[K]) {
    constexpr int N = K * kChips;
    const int n0 = K * m + r;                        // first sample of the window; [n0, n0 + K) leaves [0, N) only at m = -1 / 1022
    if constexpr (EDGE) {
#pragma unroll
        for (int i = 0; i < K; ++i) {
            const int n = n0 + i;
            const cf v = block[min(max(n, 0), N - 1)];
            const bool in = n >= 0 && n < N;
            x[i] = make_float2(in ? v.x : 0.f, in ? v.y : 0.f);
        }
    } else {
        const cf* src = block + n0;
#pragma unroll
        for (int i = 0; i + 1 < K; i += 2) {
            const float4 v = load_pair_a8(src + i);
            x[i] = make_float2(v.x, v.y);
            x[i + 1] = make_float2(v.z, v.w);
        }
        if (K & 1) x[K - 1] = src[K - 1];
    }
    return exact_window_chips(chipf, m, q);
}
template <int K, typename S>   // S: cf (converted where the Horner chain uses it) or double2
__device__ __forceinline__ void exact_window_fold(const S (&x)[K], const ExactChips& c, double2 rho, double2 step, double2& sp, double2& se, double2& sl) {
    const double dj = (double)c.c0, gl = (double)(c.cm1 - c.c0), ge = (double)(c.c0 - c.cp1);
    double2 h = cvt64(x[K - 1]);
#pragma unroll
    for (int i = K - 2; i >= 0; --i) h = horner64(h, rho, cvt64(x[i]));
    const double2 xe = cvt64(x[K - 1]), xl = cvt64(x[0]);
    sp = horner64(sp, step, make_double2(dj * h.x, dj * h.y));
    se = horner64(se, step, make_double2(ge * xe.x, ge * xe.y));
    sl = horner64(sl, step, make_double2(gl * xl.x, gl * xl.y));
}
template <int K, bool EDGE>
__device__ __forceinline__ void exact_window(const cf* __restrict__ block, int m, int r, int q, const float* __restrict__ chipf,
                                             double2 rho, double2 step, double2& sp, double2& se, double2& sl) {
    cf x[K];
    const ExactChips c = exact_window_load<K, EDGE>(block, m, r, q, chipf, x);
    exact_window_fold<K>(x, c, rho, step, sp, se, sl);
}
template <int K>
__device__ __forceinline__ double2 cpow_km1(double2 w) {   // w^(K-1), K <= 8
    double2 r = make_double2(1.0, 0.0);
#pragma unroll
    for (int i = 0; i < K - 1; ++i) r = cmul64(r, w);
    return r;
}
// What the windows of one (channel, millisecond) are summed with: the carrier (du cycles per sample, u0 at the block's first
// sample), the lag K q + r and the satellite's code.
struct ExactUnit {
    double du, u0;
    int q, r;
    const float* chipf;
};
template <int K>
__device__ __forceinline__ ExactUnit exact_unit(const DllExactParams& p, const SpecIn& in, int sat, int ms) {
    ExactUnit u;
    u.chipf = p.chipf + (sat - 1) * 2048;
    u.du = in.doppler * p.inv_fs;
    u.u0 = carrier_cycles(in.doppler, p.start_time[ms], in.carrier_phase);
    const int sN = __builtin_amdgcn_readfirstlane(mod_n(in.code_phase, K * kChips));
    u.q = sN / K; u.r = sN % K;
    return u;
}
// A lane's three window sums -> the unit's discriminator: the lane's anchor carrier (times rho^(K-1) for E), the wavefront's sums, the
// store.  n_anchor = K (lane - 1) + r, the first sample of the lane's first window: the kernel forms it, next to the same expression
// of that window's load (formed here, the compiler no longer sees the two as one and the wave kernel takes more registers).
template <int K>
__device__ __forceinline__ void exact_unit_store(double2 sp, double2 se, double2 sl, const ExactUnit& u, int lane, int n_anchor, double* out) {
    const double2 rho_a = carrier64(u.du);
    const double2 anchor = carrier64(u.u0 + u.du * (double)n_anchor);
    const double2 pp = cmul64(sp, anchor), ee = cmul64(cmul64(se, cpow_km1<K>(rho_a)), anchor), ll = cmul64(sl, anchor);
    double acc[6] = {pp.x, pp.y, ee.x, ee.y, ll.x, ll.y};
#pragma unroll
    for (int v = 0; v < 6; ++v) acc[v] = wave_sum_last(acc[v]);
    if (lane == 63) *out = dll_discriminator_exact(acc);
}
// Unit u of a launch -> its (channel, millisecond); false: not this round's or not part of the re-run.  Uniform over the unit's threads.
__device__ __forceinline__ bool exact_unit_decode(const DllExactParams& p, int u, int& ch, int& ms) {
    if (!unit_decode(p, u, ch, ms)) return false;
    if (p.only_if && !p.only_if[ch]) return false;
    if (p.from_sub && ms < p.sub.begin(p.from_sub[ch])) return false;
    return true;
}
// The windows are loaded where they are folded, two at a time by unrolling; a fifth wavefront per SIMD covers the waits.  Requesting
// a window one or two ahead of its fold was measured and rejected (10.3 against 8.2 ms, profiles/r04_exact_ab.txt; commit ffb6ef5
// is the last one that carried that code).
template <int K>
__global__ __launch_bounds__(256, 4) void dll_exact_wave_kernel(DllExactParams p) {
    static_assert(K <= 8, "a window's samples in registers");
    constexpr int N = K * kChips;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int n_units = p.n_chan * unit_span(p);
    const int n_groups = (n_units + 3) >> 2;
    for (int g = blockIdx.x; g < n_groups; g += gridDim.x) {
        // four consecutive units per workgroup, consecutive groups inside an XCD's slice: the channels of a stream-ms (shared IQ) meet in one L2
        const int u = ((n_groups & 7) ? g : xcd_contiguous(g, n_groups)) * 4 + wave;
        if (u >= n_units) continue;
        int ch, ms;
        if (!exact_unit_decode(p, u, ch, ms)) continue;           // wave-uniform
        const int64_t at = (int64_t)ch * p.n_ms + ms;
        const SpecIn in = p.spec[at];
        if (in.key == kSpecKeyLost) continue;                     // wave-uniform: the tracker never processed it
        const ChanState* st = p.states + ch;
        const int sat = __builtin_amdgcn_readfirstlane(st->sat_id), stream = __builtin_amdgcn_readfirstlane(st->stream);
        const cf* block = p.iq + (int64_t)stream * p.stream_stride + (int64_t)ms * N;
        const ExactUnit x = exact_unit<K>(p, in, sat, ms);
        double2 sp = make_double2(0.0, 0.0), se = sp, sl = sp;
        const double2 rho = carrier64(x.du), step = carrier64(x.du * (double)(K * 64));
        exact_window<K, true>(block, lane + 64 * 15 - 1, x.r, x.q, x.chipf, rho, step, sp, se, sl);     // holds window 1022 (lane 63)
#pragma unroll 2
        for (int c = 14; c >= 1; --c) exact_window<K, false>(block, lane + 64 * c - 1, x.r, x.q, x.chipf, rho, step, sp, se, sl);
        exact_window<K, true>(block, lane - 1, x.r, x.q, x.chipf, rho, step, sp, se, sl);               // holds window -1 (lane 0)
        exact_unit_store<K>(sp, se, sl, x, lane, K * (lane - 1) + x.r, p.disc_out + at);
    }
}
// ---- the same sums with a stream's millisecond staged once for all its channels (throughput path) -----------------------------
// dll_exact_wave_kernel lets every channel fetch and convert its stream's samples itself: twelve channels of a stream read the
// same 8K-sample millisecond twelve times, at a 8K-byte lane stride, and convert it float32 -> float64 twelve times.  Here the work
// item is a (channel group, millisecond): a group is up to kExactSharedConsumers channels of ONE stream (exact_group_kernel builds
// the table from the device's channel states -- gyp_bank_reset_dev rewrites ChanState::stream on the device, no host copy is
// trusted).  One 16-wavefront workgroup per CU:
//   producers (4 wavefronts)  hold the NEXT item's millisecond as raw float32 in registers, requested in lane order (16 bytes per
//                             lane, 1 KiB per load) while the consumers sum, and convert + store it into LDS between the two barriers;
//   consumers (12 wavefronts) one channel each: dll_exact_wave_kernel's arithmetic on float64 samples out of LDS -- the same operands
//                             in the same order, so the same bits.
// LDS layout: sample n (n = -K .. N + K - 1, K zeros on either side of the block: the cut windows -1 and 1022 become ordinary ones, a
// zero adds what the predicated load added) lives at 16-byte unit (n + K) + (n + K) / K, i.e. 16 bytes of padding behind every K
// samples.  Lanes read windows m = lane + 64 c - 1 at a lane stride of K + 1 units (K = 8: 144 B = 36 banks, sixteen lanes on sixteen
// different 4-bank groups) whatever r = s mod K is.  (N + 2K) / K * (K + 1) units: 147 600 bytes at K = 8, one workgroup per CU.
constexpr int kExactSharedConsumers = 12;
constexpr int kExactSharedProducers = 4;
constexpr int kExactSharedThreads = 64 * (kExactSharedConsumers + kExactSharedProducers);
constexpr int kExactGroupMaxChan = 16384;   // exact_group_kernel keeps every channel's stream index in LDS
struct ExactGroup {
    int32_t stream, n;                      // n channels (1 .. kExactSharedConsumers) of this stream, ascending
    int32_t ch[kExactSharedConsumers];
    int32_t pad[2];
};
static_assert(sizeof(ExactGroup) == 64, "ExactGroup");
template <int K>
constexpr int exact_shared_lds_units() { return (K * kChips + 2 * K) / K * (K + 1); }
template <int K>
constexpr size_t exact_shared_lds_bytes() { return (size_t)exact_shared_lds_units<K>() * sizeof(double2); }

// Channel c leads a group if the number of channels before it on its stream is a multiple of kExactSharedConsumers; it then collects
// the following channels of that stream.  One thread per channel; any channel order, any number of channels per stream.  *n_groups
// is zeroed by the host in front of the launch.  (Group ORDER depends on the atomic's arrival order; the sums do not.)
__global__ __launch_bounds__(256) void exact_group_kernel(const ChanState* __restrict__ states, int32_t n_chan, ExactGroup* __restrict__ groups,
                                                          int32_t* __restrict__ n_groups) {
    __shared__ int32_t s_stream[kExactGroupMaxChan];
    for (int i = threadIdx.x; i < n_chan; i += blockDim.x) s_stream[i] = states[i].stream;
    __syncthreads();
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_chan) return;
    const int s = s_stream[c];
    int before = 0;
    for (int i = 0; i < c; ++i) before += s_stream[i] == s ? 1 : 0;
    if (before % kExactSharedConsumers) return;
    ExactGroup g;
    g.stream = s; g.n = 1; g.ch[0] = c; g.pad[0] = g.pad[1] = 0;
#pragma unroll
    for (int k = 1; k < kExactSharedConsumers; ++k) g.ch[k] = -1;
    for (int i = c + 1; i < n_chan && g.n < kExactSharedConsumers; ++i) {
        if (s_stream[i] != s) continue;
#pragma unroll
        for (int k = 1; k < kExactSharedConsumers; ++k)      // (static indices: the record stays in registers)
            if (k == g.n) g.ch[k] = i;
        ++g.n;
    }
    groups[atomicAdd(n_groups, 1)] = g;
}

struct DllExactSharedParams {
    DllExactParams x;              // only_if / from_sub / trk_round are null on this path
    const ExactGroup* groups;
    const int32_t* n_groups;
};
// Workgroup b walks items [n_items b / grid, n_items (b + 1) / grid) of (group, millisecond), milliseconds innermost: consecutive
// milliseconds of a stream stay on one CU.  The two roles run separate loops with the same two barriers per item (wave-uniform
// branch), so that the producers' 64 sample registers are not live in the consumers' loop.
template <int K>
__global__ __launch_bounds__(kExactSharedThreads) void dll_exact_shared_kernel(DllExactSharedParams ps) {
    static_assert(K <= 8, "a window's samples in registers");
    constexpr int N = K * kChips;
    static_assert(K % 2 == 0, "the producers fetch sample pairs");
    constexpr int PT = 64 * kExactSharedProducers;       // producer threads
    constexpr int PAIRS = N / 2;                         // 16-byte sample pairs of a millisecond
    constexpr int LOADS = (PAIRS + PT - 1) / PT;         // pairs per producer lane
    extern __shared__ double2 s_x[];
    const DllExactParams& p = ps.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int span = p.ms_end - p.ms_begin;
    const int64_t n_items = (int64_t)__builtin_amdgcn_readfirstlane(ps.n_groups[0]) * span;
    const int64_t lo = n_items * blockIdx.x / gridDim.x, hi = n_items * (blockIdx.x + 1) / gridDim.x;
    if (lo >= hi) return;
    if (threadIdx.x < 2 * K) {                            // the zero halos, once
        const int np = threadIdx.x < K ? (int)threadIdx.x : N + (int)threadIdx.x;   // n + K of samples -K .. -1 and N .. N + K - 1
        s_x[np + np / K] = make_double2(0.0, 0.0);
    }
    if (wave >= kExactSharedConsumers) {
        const int pt = lane + 64 * (wave - kExactSharedConsumers);
        float4 hold[LOADS];                               // pair t = pt + PT j: samples 2t, 2t + 1 (lane order: 1 KiB per wavefront and load)
        auto request = [&](int64_t item) {
            const int g = (int)(item / span), ms = p.ms_begin + (int)(item % span);
            const int stream = __builtin_amdgcn_readfirstlane(ps.groups[g].stream);
            const cf* block = p.iq + (int64_t)stream * p.stream_stride + (int64_t)ms * N;
#pragma unroll
            for (int j = 0; j < LOADS; ++j) {
                const int t = pt + PT * j;
                if (PT * j + PT <= PAIRS) hold[j] = load_pair_a8(block, t);
                else hold[j] = t < PAIRS ? load_pair_a8(block, t) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        };
        request(lo);
        for (int64_t item = lo; item < hi; ++item) {
#pragma unroll
            for (int j = 0; j < LOADS; ++j) {
                const int t = pt + PT * j, np = 2 * t + K;   // (np and K even: both samples in front of the same padding)
                if (PT * j + PT <= PAIRS || t < PAIRS) {
                    s_x[np + np / K] = make_double2((double)hold[j].x, (double)hold[j].y);
                    s_x[np + np / K + 1] = make_double2((double)hold[j].z, (double)hold[j].w);
                }
            }
            __syncthreads();                              // the millisecond is staged
            if (item + 1 < hi) request(item + 1);
            __syncthreads();                              // the consumers are done with it
        }
        return;
    }
    const double2* win0 = s_x + (K + 1) * lane;           // window m = lane - 1 at r = 0
    for (int64_t item = lo; item < hi; ++item) {
        __syncthreads();                                  // the millisecond is staged
        const int g = (int)(item / span), ms = p.ms_begin + (int)(item % span);
        const ExactGroup* grp = ps.groups + g;
        const int ch = wave < __builtin_amdgcn_readfirstlane(grp->n) ? __builtin_amdgcn_readfirstlane(grp->ch[wave]) : -1;
        if (ch >= 0) {                                    // wave-uniform
            const int64_t at = (int64_t)ch * p.n_ms + ms;
            const SpecIn in = p.spec[at];
            if (in.key != kSpecKeyLost) {                 // wave-uniform
                const ExactUnit u = exact_unit<K>(p, in, __builtin_amdgcn_readfirstlane(p.states[ch].sat_id), ms);
                int off[K];                               // sample i of a window: r + i units on, one more behind the padding
#pragma unroll
                for (int i = 0; i < K; ++i) off[i] = u.r + i + (u.r + i >= K ? 1 : 0);
                double2 sp = make_double2(0.0, 0.0), se = sp, sl = sp;
                const double2 rho = carrier64(u.du), step = carrier64(u.du * (double)(K * 64));
#pragma unroll 2
                for (int c = 15; c >= 0; --c) {
                    const double2* w = win0 + (K + 1) * 64 * c;
                    double2 x[K];
#pragma unroll
                    for (int i = 0; i < K; ++i) x[i] = w[off[i]];
                    exact_window_fold<K>(x, exact_window_chips(u.chipf, lane + 64 * c - 1, u.q), rho, step, sp, se, sl);
                }
                exact_unit_store<K>(sp, se, sl, u, lane, K * (lane - 1) + u.r, p.disc_out + at);
            }
        }
        __syncthreads();                                  // done with the millisecond
    }
}
// The first NV of the exact sums of one millisecond at lag `lag`, by a whole workgroup of T threads walking the block
// (exact_epl_generic), with the carrier the millisecond ran with (`in`): the wavefronts' sums meet in `part` and, behind a barrier,
// thread 0 alone runs use(ex) on their sum.  (A callable, not an array handed back: an array filled under `tid == 0` and read by the
// caller cost both kernels some 40 registers.)  The two users add the wavefronts in different associations and each keeps its own,
// they are not the same bits: PAIRS (p0 + p1) + (p2 + p3), else ((p0 + p1) + p2) + p3.  GUARD: a barrier in front of the hand-over,
// for a caller that has none between thread 0's reads of `part` and the next call.
template <int K, int T, int NV, bool PAIRS, bool GUARD, typename ParamsT, typename UseT>
__device__ __forceinline__ void workgroup_exact_sums(const cf* block, const ParamsT& p, const SpecIn& in, int ms, int lag,
                                                     const float* chipf, int tid, double (*part)[6], UseT use) {
    static_assert(!PAIRS || T == 256, "four wavefronts");
    const double du = in.doppler * p.inv_fs;
    const double u0 = carrier_cycles(in.doppler, p.start_time[ms], in.carrier_phase);
    double acc[6];
    exact_epl_generic<K, T>(block, u0, du, lag, chipf, tid, acc);
#pragma unroll
    for (int v = 0; v < NV; ++v) acc[v] = wave_sum_last(acc[v]);
    if (GUARD) __syncthreads();
    if ((tid & 63) == 63) {
#pragma unroll
        for (int v = 0; v < NV; ++v) part[tid >> 6][v] = acc[v];
    }
    __syncthreads();
    if (tid == 0) {
        double ex[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            if (PAIRS) {
                ex[v] = (part[0][v] + part[1][v]) + (part[2][v] + part[3][v]);
            } else {
                double t = part[0][v];
#pragma unroll
                for (int w = 1; w < T / 64; ++w) t += part[w][v];
                ex[v] = t;
            }
        }
        use(ex);
    }
}
// Rates above 8 samples per chip (16.368 ... 49.104 Msps): one 256-thread workgroup per unit walks the block (exact_epl_generic).
template <int K>
__global__ __launch_bounds__(256) void dll_exact_block_kernel(DllExactParams p) {
    constexpr int N = K * kChips;
    __shared__ double part[4][6];
    const int tid = threadIdx.x;
    const int n_units = p.n_chan * unit_span(p);
    for (int v = blockIdx.x; v < n_units; v += gridDim.x) {
        int ch, ms;
        if (!exact_unit_decode(p, (n_units & 7) ? v : xcd_contiguous(v, n_units), ch, ms)) continue;   // uniform
        const int64_t at = (int64_t)ch * p.n_ms + ms;
        const SpecIn in = p.spec[at];
        if (in.key == kSpecKeyLost) continue;                     // uniform
        const ChanState* st = p.states + ch;
        const cf* block = p.iq + (int64_t)st->stream * p.stream_stride + (int64_t)ms * N;
        workgroup_exact_sums<K, 256, 6, true, true>(block, p, in, ms, mod_n(in.code_phase, N), p.chipf + (st->sat_id - 1) * 2048, tid, part,
                                                    [&](const double (&ex)[6]) { p.disc_out[at] = dll_discriminator_exact(ex); });
    }
}

struct DllScanParams {
    const cf* iq;
    int64_t stream_stride;
    int32_t n_ms, ms_begin, ms_end;
    const double* start_time;
    ChanState* states;
    const ChanState* ckpt;     // the states before the call, or null: the tracking kernel left them in `exact` (throughput path)
    int32_t n_chan;
    const SpecIn* spec;
    const double* disc;
    gyp_track_rec* rec_out;
    DllExact* exact;
    const int32_t* bad;        // optional per-channel flags of failed speculations ...
    int32_t only_bad;          // ... 0: flagged channels are left alone (the re-run gives them everything); 1: ONLY flagged ones (after it)
    const int32_t* from_sub;   // only_bad: the re-run started at sub-block from_sub[ch] (SubLayout)
    SubLayout sub;
    DllExact* hist_out;        // optional: the loop's state at the end of this launch's range is also left here (the next sub-block's checkpoint)
    const float* chipf;
    double inv_fs, dll_gain, dll_modulus, n_samples;
    int32_t first, final;
    int32_t* prof_delta;       // optional [n_chan][prof_depth], zeroed by the host: (exact - provisional) code phase of a repaired
    int32_t prof_from, prof_depth;   // millisecond, for the rows of TrackBlockParams::prof_tail
    // The pseudosymbol is sign(Re peak) (tracker.py:316): a float32 peak whose real part is within symbol_tau of zero relative to
    // its modulus (an unlocked channel rotating through +-90 degrees) cannot decide it by itself.  For those milliseconds the
    // coherent prompt value at the arg-max lag is formed in float64 here, like a repair step, and the record's pseudosymbol
    // rewritten.  (This removes the millisecond's own float32 rounding, ~1e-6 relative.  What it cannot remove is the carrier
    // loop's accumulated float32 difference from the reference's state -- the loop runs on float32 peaks -- which in a channel that
    // never locks can reach 1e-4 rad: one pseudosymbol in 3.6 M channel-ms at 4.092 Msps, profiles/r03_surveys.txt.)
    float symbol_tau;
    // round protocol (SpecCtl): channel ch scans sub-block trk_round[ch] (-1: nothing) from the loop state hist[sub][ch]
    // (sub == 0: the channel's checkpoint ckpt[ch]) and leaves hist[sub + 1][ch]; `first` / `final` / ms_begin / ms_end are not used
    const int32_t* trk_round;
    DllExact* hist;
};
constexpr int kScanThreads = 256;
constexpr int kScanChunk = 512;     // milliseconds staged in LDS at a time
constexpr int kSpecKeyRepaired = -3;
// The satellite's +-1 code (twice over) into LDS, by the whole workgroup: once per launch, at the first millisecond whose sums it forms.
__device__ __forceinline__ void scan_stage_code(float* s_chipf, const float* chipf, int tid) {
    for (int k = tid; k < 2048; k += kScanThreads) s_chipf[k] = chipf[k];
    __syncthreads();
}
template <int K>
__global__ __launch_bounds__(kScanThreads) void dll_scan_kernel(DllScanParams p) {
    constexpr int N = K * kChips;
    // One chunk of the channel's hand-over data in LDS: loaded and written back by all threads (coalesced), walked by wavefront 0
    // alone (every lane the same values: broadcast reads, no cross-lane traffic) -- the serial loop never touches global memory.
    __shared__ double s_disc[kScanChunk];   // in: tracker.py:297 at the provisional lag; out: at the lag the exact loop ran with
    __shared__ int s_cpin[kScanChunk];      // provisional code phase of the millisecond
    __shared__ int s_cpout[kScanChunk];     // exact code phase after the update (the record's)
    __shared__ int s_key[kScanChunk];       // SpecIn::key; kSpecKeyRepaired once the millisecond has been repaired
    __shared__ double part[kScanThreads / 64][6];
    __shared__ float s_chipf[2048];         // this satellite's +-1 code twice over (scan_stage_code)
    __shared__ double s_a;
    __shared__ int s_s, s_pos, s_repairs;
    __shared__ int s_nund;
    __shared__ short s_und[kScanChunk];     // milliseconds of the chunk whose float32 peak cannot decide the pseudosymbol
    bool have_code = false;
    const int ch = blockIdx.x, tid = threadIdx.x;
    if (ch >= p.n_chan) return;
    if (p.bad && (p.bad[ch] != 0) != (p.only_bad != 0)) return;
    const ChanState* st = p.states + ch;
    int range_lo = p.ms_begin, range_hi = p.ms_end, sub_here = -1;
    if (p.trk_round) {   // uniform
        sub_here = p.trk_round[ch];
        if (sub_here < 0) return;
        range_lo = p.sub.begin(sub_here);
        range_hi = p.sub.end(sub_here, p.n_ms);
    }
    if (tid == 0) {
        if (p.trk_round) {
            if (sub_here == 0) { s_a = p.ckpt[ch].dll_phase; s_s = p.ckpt[ch].code_phase; s_repairs = 0; }
            else { const DllExact x = p.hist[(size_t)sub_here * p.n_chan + ch]; s_a = x.dll; s_s = x.code_phase; s_repairs = x.repairs; }
        } else if (p.first && p.ckpt) { s_a = p.ckpt[ch].dll_phase; s_s = p.ckpt[ch].code_phase; s_repairs = 0; }
        else { const DllExact x = p.exact[ch]; s_a = x.dll; s_s = x.code_phase; s_repairs = p.first ? 0 : x.repairs; }
    }
    const float* chipf = p.chipf + (st->sat_id - 1) * 2048;
    const cf* stream = p.iq + (int64_t)st->stream * p.stream_stride;
    const int64_t row = (int64_t)ch * p.n_ms;
    const int ms_first = (p.only_bad && p.from_sub) ? max(p.ms_begin, p.sub.begin(min(p.from_sub[ch], p.sub.sub_of(p.n_ms - 1)))) : range_lo;
    for (int c0 = ms_first; c0 < range_hi; c0 += kScanChunk) {
        const int len = min(kScanChunk, range_hi - c0);
        for (int i = tid; i < len; i += kScanThreads) {
            const SpecIn* in = p.spec + row + c0 + i;
            const int key = in->key;
            s_key[i] = key;
            s_cpin[i] = in->code_phase;
            s_disc[i] = key == kSpecKeyLost ? 0.0 : p.disc[row + c0 + i];
        }
        if (tid == 0) { s_pos = 0; s_nund = 0; }
        __syncthreads();
        if (p.rec_out) {
            for (int i = tid; i < len; i += kScanThreads) {
                const gyp_track_rec* r = p.rec_out + row + c0 + i;
                const float pr = r->peak_re, pi = r->peak_im;
                if (s_key[i] != kSpecKeyLost && r->status != 2 && fabsf(pr) <= p.symbol_tau * __builtin_amdgcn_sqrtf(fmaf(pr, pr, pi * pi)))
                    s_und[atomicAdd(&s_nund, 1)] = (short)i;
            }
            __syncthreads();
            const int n_und = s_nund;
            for (int u = 0; u < n_und; ++u) {   // uniform; rare (test hook GYP_SYMBOL_TAU = 10: every millisecond)
                const int ms = c0 + s_und[u];
                const SpecIn in = p.spec[row + ms];
                if (!have_code) { scan_stage_code(s_chipf, chipf, tid); have_code = true; }   // uniform
                int lag = mod_n(in.code_phase, N) + p.rec_out[row + ms].peak_offset;   // (before any repair moves the offset: same lag)
                lag = lag >= N ? lag - N : lag;
                workgroup_exact_sums<K, kScanThreads, 1, false, false>(   // (Re of the coherent prompt value is all the pseudosymbol needs)
                    stream + (int64_t)ms * N, p, in, ms, lag, s_chipf, tid, part,
                    [&](const double (&re)[1]) { p.rec_out[row + ms].pseudosymbol = re[0] > 0.0 ? 1 : (re[0] < 0.0 ? -1 : 0); });
                __syncthreads();
            }
        }
        while (true) {   // uniform: every thread sees the same s_pos
            if (tid < 64) {   // wavefront 0 walks until the chunk ends or a millisecond needs its sums formed again
                // Every lane carries the same values.  The common case -- processed, lags agree, accumulator in its usual range -- is
                // straight-line vector code behind ONE scalar branch per millisecond (each vector-to-scalar hand-over costs the
                // pipeline's depth), with the next millisecond's hand-over values already requested from LDS.
                double a = s_a;
                int s = s_s, i = __builtin_amdgcn_readfirstlane(s_pos);   // (i: scalar loop control)
                bool stop = false;
                int key_n = 0, cp_n = 0;
                double d_n = 0.0;
                if (i < len) { key_n = s_key[i]; cp_n = s_cpin[i]; d_n = s_disc[i]; }
                while (i < len && !stop) {   // uniform
                    const int key = key_n, cp = cp_n;
                    const double d = d_n;
                    if (i + 1 < len) { key_n = s_key[i + 1]; cp_n = s_cpin[i + 1]; d_n = s_disc[i + 1]; }
                    const double dll = __dadd_rn(a, __dmul_rn(d, p.dll_gain));   // tracker.py:298: product and sum rounded separately, as Python does
                    const double whole = trunc(dll);
                    // (bitwise, not short-circuit: one predicate, no branch per clause)
                    const int usual = (int)(key != kSpecKeyLost) & ((int)(key == kSpecKeyRepaired) | (int)(s == cp)) &
                                      (int)(fabs(whole) < 2147483648.0) & (int)(dll > -p.dll_modulus) & (int)(dll < 2.0 * p.dll_modulus);
                    if (__builtin_amdgcn_readfirstlane(usual)) {
                        double r = dll >= p.dll_modulus ? dll - p.dll_modulus : dll;   // pymod_uniform's fast range
                        r += (r != 0.0 && r < 0.0) ? p.dll_modulus : 0.0;
                        r += r < 0.0 ? p.dll_modulus : 0.0;
                        a = r;
                        s = (int)whole;
                        if (tid == 0) s_cpout[i] = s;
                        ++i;
                        continue;
                    }
                    if (uniform(key == kSpecKeyLost)) {                   // not processed: the loop state stands (the status-2 record carries it)
                        if (tid == 0) s_cpout[i] = s;
                        ++i;
                        continue;
                    }
                    if (uniform(key != kSpecKeyRepaired && s != cp)) { stop = true; break; }
                    double r = pymod_uniform(dll, p.dll_modulus);         // the accumulator outside its usual range
                    r += r < 0.0 ? p.dll_modulus : 0.0;
                    a = r;
                    s = uniform(fabs(whole) < 2147483648.0) ? (int)whole : code_phase_beyond_int32(whole, p.n_samples);
                    if (tid == 0) s_cpout[i] = s;
                    ++i;
                }
                if (tid == 0) { s_a = a; s_s = s; s_pos = i; }
            }
            __syncthreads();
            const int pos = s_pos;
            if (pos >= len) break;
            {   // repair: this millisecond's float64 sums for the lag the exact loop is at
                const int ms = c0 + pos;
                const SpecIn in = p.spec[row + ms];
                if (!have_code) { scan_stage_code(s_chipf, chipf, tid); have_code = true; }   // uniform
                workgroup_exact_sums<K, kScanThreads, 6, false, false>(stream + (int64_t)ms * N, p, in, ms, mod_n(s_s, N), s_chipf, tid, part, [&](const double (&ex)[6]) {
                    s_disc[pos] = dll_discriminator_exact(ex);
                    s_key[pos] = kSpecKeyRepaired;
                    if (p.rec_out) {   // the arg-max LAG stands; its index in the profile of the PRN rolled by s moves with s
                        gyp_track_rec* rec = p.rec_out + row + ms;
                        int lag = rec->peak_offset + mod_n(in.code_phase, N);
                        lag = lag >= N ? lag - N : lag;
                        const int k2 = lag - mod_n(s_s, N);
                        rec->peak_offset = k2 < 0 ? k2 + N : k2;
                    }
                    if (p.prof_delta && ms >= p.prof_from)
                        p.prof_delta[(int64_t)ch * p.prof_depth + (ms - p.prof_from)] = mod_n(s_s, N) - mod_n(in.code_phase, N);
                    ++s_repairs;
                });
                __syncthreads();
            }
        }
        // write-back: the record's discriminator and code phase
        if (p.rec_out) {
            for (int i = tid; i < len; i += kScanThreads) {
                gyp_track_rec* rec = p.rec_out + row + c0 + i;
                rec->code_phase = s_cpout[i];
                if (s_key[i] != kSpecKeyLost) rec->discriminator = (float)s_disc[i];
            }
        }
        __syncthreads();   // the arrays are reused by the next chunk
    }
    if (tid == 0) {
        DllExact x; x.dll = s_a; x.code_phase = s_s; x.repairs = s_repairs;
        if (p.trk_round) {
            p.hist[(size_t)(sub_here + 1) * p.n_chan + ch] = x;   // (spec_finalize_kernel writes the state back when the block has held)
        } else {
            p.exact[ch] = x;
            if (p.hist_out) p.hist_out[ch] = x;
            if (p.final) { p.states[ch].dll_phase = s_a; p.states[ch].code_phase = s_s; }
        }
    }
}

}  // namespace gyp
