// kernels_weak.hpp -- the weak bank's tracking kernel (include/gypsum_hip.h, "weak-signal tracking"; the shared arithmetic is
// weak_plan.hpp's).  A part of kernels.hpp.
//
// weak_track_kernel: one workgroup of kWeakWaves wavefronts per channel, channels in bank order in the grid (through xcd_contiguous, so
// that the channels of a stream share an L2 as the 1-ms tracker's do).  A channel is serial only where its loop closes, so the call's
// milliseconds go through in chunks of at most 20 between which the state is final:
//   plan    thread 0 writes one WeakMsPlan per millisecond of the chunk into LDS -- in TRACK the rest of the current period (all share
//           the period-start u0 / c0 and differ in their first sample index), in SYNC / WAIT up to 20 one-millisecond periods whose
//           open-loop NCO states it steps through itself (they depend on no sum); a chunk never crosses the end of SYNC, the bit edge
//           or the end of the call;
//   sums    wavefront w takes the chunk's milliseconds w, w + kWeakWaves, ...: lane l walks samples l, l + 64, ... in increasing order
//           with six float64 accumulators (minus, prompt, plus: the float32 products widened -- float32 accumulators put a noise-free
//           16.368 Msps millisecond at 1.01 of the 1e-4 bar, a bias of adding equal terms to a growing sum), the lanes are reduced in
//           float64 by the fixed tree in which lane l takes lane l + 32, 16, 8, 4, 2, 1, and lane 0 rounds the six sums to float32
//           once, leaves them in LDS and writes the millisecond's record.  Which wavefront
//           takes a millisecond does not enter its arithmetic: the sums are a function of the plan entry and the samples alone;
//   fold    thread 0 walks the chunk in order: SYNC prompts go to the bank's prompt row, TRACK sums into the period's float64 sums,
//           and a period that is complete closes the loops (weak_close_period) and writes its record;
//   edge    when the last SYNC prompt is in, the workgroup copies the prompt row into LDS, lanes 0..19 of wavefront 0 each take one
//           offset's energy (weak_bit_energy) and thread 0 picks (weak_bit_pick).
// The satellite's 1023 chips sit in LDS as +-1.0f: neighbouring lanes read the same or the next chip, so the reads broadcast.
// No atomics; barriers only between the four steps.  Contraction is off in everything the header fixes an order for.
//
// What bounds it: per sample one float64 multiply-add pair and range reduction for the carrier phase, the float32 sine/cosine
// polynomial (carrier_from_cycles_fast, ~25 instructions), one 64-bit multiply and three shift / remainder chains for the chip
// indices, three LDS reads and six float64 adds -- about a hundred vector instructions for 8 bytes fetched, so the kernel is bound
// by vector issue, not by memory: every channel of a stream re-reads the stream's samples through L2.
#pragma once

#include "weak_plan.hpp"

namespace gyp {

constexpr int kWeakWaves = 10;                 // 20 milliseconds of a period = 2 per wavefront
constexpr int kWeakThreads = kWeakWaves * 64;

struct WeakMsPlan {
    double u_base, du;     // cycles at sample index 0 of the period; cycles per sample
    int64_t c_base, r;     // 2^-40 chips at sample index 0 of the period; per sample
    int32_t k_first;       // index in the period of the millisecond's first sample
    int16_t pos;
    int8_t phase, pad;
};

struct WeakTrackParams {
    WeakChan* states;              // [n_chan]
    float2* sync_prompts;          // [n_chan][sync_ms]
    const float* iq;               // stream s at iq + 2 * s * stream_stride
    int64_t stream_stride;
    const uint8_t* chips;          // [32][1023] in {0, 1}
    gyp_weak_ms_rec* ms_out;       // [n_chan][n_ms] or NULL
    gyp_weak_period_rec* period_out;   // [n_chan][n_ms / 20 + 1] or NULL
    int32_t* n_periods_out;        // [n_chan] or NULL
    gyp_weak_params prm;
    double fs;
    int64_t first_ms;
    int32_t n, n_ms, n_chan;
};

__device__ __forceinline__ int weak_chip_of(int64_t v) {
    int t = (int)(v >> 40) % kChips;
    return t < 0 ? t + kChips : t;
}

// The three sums of one millisecond (all 64 lanes; the result is lane 0's).
__device__ __forceinline__ void weak_ms_sums(const float2* __restrict__ x, int32_t n, const WeakMsPlan& pl, int64_t d, const float* chips_pm, int lane,
                                             cf& minus, cf& prompt, cf& plus) {
#pragma clang fp contract(off)
    double mr = 0.0, mi = 0.0, pr = 0.0, pi = 0.0, lr = 0.0, li = 0.0;
    for (int32_t i = lane; i < n; i += 64) {
        const int32_t k = pl.k_first + i;
        const double step = pl.du * (double)k;
        const cf car = carrier_from_cycles_fast(pl.u_base + step);
        const cf w = cmul(x[i], car);
        const int64_t at = pl.c_base + (int64_t)k * pl.r;
        const float sm = chips_pm[weak_chip_of(at - d)], sp = chips_pm[weak_chip_of(at)], sl = chips_pm[weak_chip_of(at + d)];
        mr += (double)(sm * w.x); mi += (double)(sm * w.y);
        pr += (double)(sp * w.x); pi += (double)(sp * w.y);
        lr += (double)(sl * w.x); li += (double)(sl * w.y);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mr += __shfl_down(mr, off); mi += __shfl_down(mi, off);
        pr += __shfl_down(pr, off); pi += __shfl_down(pi, off);
        lr += __shfl_down(lr, off); li += __shfl_down(li, off);
    }
    minus = make_float2((float)mr, (float)mi); prompt = make_float2((float)pr, (float)pi); plus = make_float2((float)lr, (float)li);
}

__device__ __forceinline__ gyp_weak_ms_rec weak_lost_rec() {
    gyp_weak_ms_rec r{};
    r.status = 2;
    return r;
}

__global__ __launch_bounds__(kWeakThreads) void weak_track_kernel(WeakTrackParams p) {
    __shared__ float chips_pm[kChips + 1];
    __shared__ WeakChan st;
    __shared__ WeakMsPlan plan[kWeakPeriodMs];
    __shared__ float2 sums[kWeakPeriodMs][3];
    __shared__ float2 sync_lds[kWeakSyncMax];
    __shared__ double energies[kWeakPeriodMs];
    __shared__ int32_t chunk, edge_now;

    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int chan = xcd_contiguous((int)blockIdx.x, p.n_chan);
    if (chan >= p.n_chan) return;
    const int32_t max_periods = p.n_ms / kWeakPeriodMs + 1;
    gyp_weak_ms_rec* const ms_row = p.ms_out ? p.ms_out + (int64_t)chan * p.n_ms : nullptr;
    gyp_weak_period_rec* const period_row = p.period_out ? p.period_out + (int64_t)chan * max_periods : nullptr;
    float2* const sync_row = p.sync_prompts + (int64_t)chan * p.prm.sync_ms;

    if (tid == 0) st = p.states[chan];
    __syncthreads();
    {
        const uint8_t* c = p.chips + (size_t)(st.sat_id - 1) * kChips;
        for (int i = tid; i < kChips; i += kWeakThreads) chips_pm[i] = c[i] ? 1.0f : -1.0f;
    }
    const float2* const x0 = reinterpret_cast<const float2*>(p.iq) + (int64_t)st.stream * p.stream_stride;
    __syncthreads();

    int32_t m = 0, n_periods = 0;   // n_periods: thread 0's
    while (m < p.n_ms) {
        if (st.status != 0) {       // lost or dropped (uniform: read from LDS behind a barrier)
            if (ms_row)
                for (int32_t i = m + tid; i < p.n_ms; i += kWeakThreads) ms_row[i] = weak_lost_rec();
            break;
        }
        if (tid == 0) {             // ---- plan
            const int64_t ma = p.first_ms + m;
            if (st.phase == kWeakWait && ma % kWeakPeriodMs == st.edge) { st.phase = kWeakTrack; st.pos = 0; }
            const double du = st.f / p.fs;
            const int64_t r = weak_code_rate(st.f, p.n);
            int32_t c = p.n_ms - m;
            if (st.phase == kWeakTrack) {
                if (c > kWeakPeriodMs - st.pos) c = kWeakPeriodMs - st.pos;
                if (st.pos == 0) st.period_first = ma;
                for (int32_t j = 0; j < c; ++j)
                    plan[j] = WeakMsPlan{st.u0, du, st.c0, r, (st.pos + j) * p.n, (int16_t)(st.pos + j), (int8_t)kWeakTrack, 0};
            } else {
                if (c > kWeakPeriodMs) c = kWeakPeriodMs;
                if (st.phase == kWeakSync) {
                    if (c > p.prm.sync_ms - st.sync_count) c = p.prm.sync_ms - st.sync_count;
                } else {
                    const int32_t to_edge = (int32_t)((((int64_t)st.edge - ma) % kWeakPeriodMs + kWeakPeriodMs) % kWeakPeriodMs);   // > 0 here
                    if (c > to_edge) c = to_edge;
                }
                for (int32_t j = 0; j < c; ++j) {
                    plan[j] = WeakMsPlan{st.u0, du, st.c0, r, 0, 0, (int8_t)st.phase, 0};
                    weak_advance(&st.u0, &st.c0, st.f, p.fs, p.n, r);
                }
            }
            chunk = c;
            edge_now = 0;
        }
        __syncthreads();
        const int32_t c = chunk;
        for (int32_t j = wave; j < c; j += kWeakWaves) {   // ---- sums
            cf mi, pr, pl;
            weak_ms_sums(x0 + (int64_t)(m + j) * p.n, p.n, plan[j], p.prm.spacing, chips_pm, lane, mi, pr, pl);
            if (lane == 0) {
                sums[j][0] = mi; sums[j][1] = pr; sums[j][2] = pl;
                if (ms_row) {
                    gyp_weak_ms_rec rec{};
                    rec.minus_re = mi.x; rec.minus_im = mi.y; rec.prompt_re = pr.x; rec.prompt_im = pr.y; rec.plus_re = pl.x; rec.plus_im = pl.y;
                    rec.pos = plan[j].pos; rec.phase = plan[j].phase;
                    ms_row[m + j] = rec;
                }
            }
        }
        __syncthreads();
        if (tid == 0) {             // ---- fold
            for (int32_t j = 0; j < c; ++j) {
                if (st.phase == kWeakSync) {
                    sync_row[st.sync_count++] = sums[j][1];
                    if (st.sync_count == p.prm.sync_ms) edge_now = 1;   // the chunk ends here
                } else if (st.phase == kWeakTrack) {
                    weak_fold_ms(&st, sums[j][0].x, sums[j][0].y, sums[j][1].x, sums[j][1].y, sums[j][2].x, sums[j][2].y);
                    if (++st.pos == kWeakPeriodMs) {
                        gyp_weak_period_rec rec;
                        weak_close_period(&st, p.prm, p.fs, p.n, &rec);
                        if (period_row && n_periods < max_periods) period_row[n_periods] = rec;
                        ++n_periods;
                    }
                }
            }
        }
        __syncthreads();
        if (edge_now) {             // ---- edge (uniform)
            for (int32_t i = tid; i < p.prm.sync_ms; i += kWeakThreads) sync_lds[i] = sync_row[i];
            __syncthreads();
            if (tid < kWeakPeriodMs) energies[tid] = weak_bit_energy(reinterpret_cast<const float*>(sync_lds), p.prm.sync_ms, st.sync_start, tid);
            __syncthreads();
            if (tid == 0) { st.edge = weak_bit_pick(energies); st.phase = kWeakWait; }
            __syncthreads();
        }
        m += c;
    }
    if (tid == 0) {
        p.states[chan] = st;
        if (p.n_periods_out) p.n_periods_out[chan] = n_periods < max_periods ? n_periods : max_periods;
    }
}

}  // namespace gyp
