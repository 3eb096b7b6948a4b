// kernels_refine.hpp -- the weak-signal hand-over (include/gypsum_hip.h, "weak-signal hand-over"; the shared arithmetic is
// refine_plan.hpp's and weak_plan.hpp's).  A part of kernels.hpp.
//
// Three launches per call, none with an atomic:
//   weak_refine_plan_kernel      one thread per candidate steps u0 and c0 through the n_ms open-loop milliseconds with weak_advance, as
//                                thread 0 of weak_track_kernel does in SYNC, and writes one WeakMsPlan per (candidate, millisecond): the
//                                states are the bank's whichever workgroup later takes a millisecond.
//   weak_refine_sums_kernel      the hot path: one wavefront per (candidate, millisecond), grid-wide.  A workgroup of kRefineWaves
//                                wavefronts takes a run of kRefineWaves milliseconds of one candidate (one each) and loads the
//                                satellite's chips into LDS once.  weak_prompt_sum is weak_ms_sums without the minus and plus lags: the
//                                same loop order, products, float64 lane accumulators, reduction tree and single rounding, so the
//                                prompt is the bank's SYNC prompt bit for bit.  256 threads and 4 KiB of LDS: the candidates of a
//                                three-satellite hand-over over 220 ms are 165 workgroups, one per CU, where the bank's shape is three.
//   weak_refine_estimate_kernel  one workgroup per candidate: the prompts into LDS (at most 16 KiB), the squared pre-sums beside them
//                                (at most 32 KiB), threads take bins j and walk g in order (every lane reads the same s_g: a broadcast),
//                                thread 0 picks, interpolates and forms Y*, all threads derotate the prompts in LDS, lanes 0..19 take
//                                the twenty bit-edge energies as weak_track_kernel's edge step does, thread 0 writes the record.  The
//                                power row (up to 4097 float64) lives in device memory: with it the kernel would not fit 64 KiB of LDS.
#pragma once

#include "kernels_weak.hpp"
#include "refine_plan.hpp"

namespace gyp {

constexpr int kRefineWaves = 4;                   // wavefronts, and milliseconds, per workgroup of the sums kernel
constexpr int kRefineThreads = kRefineWaves * 64;
constexpr int kRefineEstThreads = 256;

// A candidate as the host uploads it: the start-up state of a weak bank's channel (weak_fresh_chan) and what the record repeats.
struct WeakRefineCand {
    int32_t stream, sat_id, code_phase, pad;
    double f, u0, carrier_phase;
    int64_t c0;
};

struct WeakRefineArgs {
    const WeakRefineCand* cands;   // [n_cand]
    WeakMsPlan* plans;             // [n_cand][n_ms]
    float2* prompts;               // [n_cand][n_ms]
    double* power;                 // [n_cand][n_bins]
    const float* iq;               // stream s at iq + 2 * s * stream_stride
    int64_t stream_stride;
    const uint8_t* chips;          // [32][1023] in {0, 1}
    gyp_weak_refined* out;         // [n_cand]
    gyp_weak_refine_params prm;
    double fs;
    int64_t first_ms;
    int32_t n, n_ms, n_cand;
};

__global__ __launch_bounds__(64) void weak_refine_plan_kernel(WeakRefineArgs p) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= p.n_cand) return;
    const WeakRefineCand c = p.cands[i];
    double u0 = c.u0;
    int64_t c0 = c.c0;
    const double du = c.f / p.fs;
    const int64_t r = weak_code_rate(c.f, p.n);
    WeakMsPlan* const row = p.plans + (int64_t)i * p.n_ms;
    for (int32_t m = 0; m < p.n_ms; ++m) {
        row[m] = WeakMsPlan{u0, du, c0, r, 0, 0, (int8_t)kWeakSync, 0};
        weak_advance(&u0, &c0, c.f, p.fs, p.n, r);
    }
}

// The prompt sum of one millisecond (all 64 lanes; the result is lane 0's): weak_ms_sums' prompt, bit for bit.
__device__ __forceinline__ cf weak_prompt_sum(const float2* __restrict__ x, int32_t n, const WeakMsPlan& pl, const float* chips_pm, int lane) {
#pragma clang fp contract(off)
    double pr = 0.0, pi = 0.0;
    for (int32_t i = lane; i < n; i += 64) {
        const int32_t k = pl.k_first + i;
        const double step = pl.du * (double)k;
        const cf car = carrier_from_cycles_fast(pl.u_base + step);
        const cf w = cmul(x[i], car);
        const int64_t at = pl.c_base + (int64_t)k * pl.r;
        const float sp = chips_pm[weak_chip_of(at)];
        pr += (double)(sp * w.x); pi += (double)(sp * w.y);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        pr += __shfl_down(pr, off); pi += __shfl_down(pi, off);
    }
    return make_float2((float)pr, (float)pi);
}

// grid: n_cand x ceil(n_ms / kRefineWaves), candidate-major
__global__ __launch_bounds__(kRefineThreads) void weak_refine_sums_kernel(WeakRefineArgs p) {
    __shared__ float chips_pm[kChips + 1];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int runs = (p.n_ms + kRefineWaves - 1) / kRefineWaves;
    const int cand = (int)(blockIdx.x / (unsigned)runs), run = (int)(blockIdx.x % (unsigned)runs);
    const WeakRefineCand c = p.cands[cand];
    {
        const uint8_t* code = p.chips + (size_t)(c.sat_id - 1) * kChips;
        for (int i = tid; i < kChips; i += kRefineThreads) chips_pm[i] = code[i] ? 1.0f : -1.0f;
    }
    __syncthreads();
    const int32_t m = run * kRefineWaves + wave;
    if (m >= p.n_ms) return;                     // (no barrier follows)
    const float2* const x = reinterpret_cast<const float2*>(p.iq) + (int64_t)c.stream * p.stream_stride + (int64_t)m * p.n;
    const WeakMsPlan pl = p.plans[(int64_t)cand * p.n_ms + m];
    const cf prompt = weak_prompt_sum(x, p.n, pl, chips_pm, lane);
    if (lane == 0) p.prompts[(int64_t)cand * p.n_ms + m] = prompt;
}

// grid: n_cand
__global__ __launch_bounds__(kRefineEstThreads) void weak_refine_estimate_kernel(WeakRefineArgs p) {
    __shared__ float2 pr_lds[kRefineMaxMs];
    __shared__ double s_lds[2 * kRefineMaxMs];
    __shared__ double energies[kWeakPeriodMs];
    __shared__ RefinePick pick;
    __shared__ double ystar[2];

    const int tid = (int)threadIdx.x;
    const int cand = (int)blockIdx.x;
    const RefineShape sh = refine_shape(p.prm, p.n_ms);
    const float2* const row = p.prompts + (int64_t)cand * p.n_ms;
    double* const P = p.power + (int64_t)cand * sh.n_bins;

    for (int32_t m = tid; m < p.n_ms; m += kRefineEstThreads) pr_lds[m] = row[m];
    __syncthreads();
    for (int32_t g = tid; g < sh.G; g += kRefineEstThreads)
        refine_group_square(reinterpret_cast<const float*>(pr_lds), g, sh.L, &s_lds[2 * g], &s_lds[2 * g + 1]);
    __syncthreads();
    for (int32_t j = tid; j < sh.n_bins; j += kRefineEstThreads) P[j] = refine_bin_power(s_lds, sh, j);
    __threadfence_block();                       // the workgroup's own writes to P, visible to thread 0 behind the barrier
    __syncthreads();
    if (tid == 0) {
        pick = refine_pick(P, sh);
        refine_sum_at(s_lds, sh.G, sh.L, pick.delta_hz, &ystar[0], &ystar[1]);
    }
    __syncthreads();
    const double delta = pick.delta_hz;
    for (int32_t m = tid; m < p.n_ms; m += kRefineEstThreads) {
        float2 v = pr_lds[m];
        refine_derotate(v.x, v.y, delta, m, &v.x, &v.y);
        pr_lds[m] = v;
    }
    __syncthreads();
    if (tid < kWeakPeriodMs) energies[tid] = weak_bit_energy(reinterpret_cast<const float*>(pr_lds), p.n_ms, p.first_ms, tid);
    __syncthreads();
    if (tid == 0) {
        const WeakRefineCand c = p.cands[cand];
        gyp_weak_refined o{};
        o.stream = c.stream; o.sat_id = c.sat_id; o.code_phase = c.code_phase;
        o.doppler_hz = c.f + pick.delta_hz;
        o.edge = weak_bit_pick(energies);
        o.edge_ratio = refine_edge_ratio(energies, o.edge);
        o.carrier_phase = refine_carrier_phase(c.carrier_phase, ystar[0], ystar[1]);
        o.delta_hz = pick.delta_hz; o.peak_to_mean = pick.peak_to_mean;
        o.bin = pick.bin; o.status = pick.status;
        p.out[cand] = o;
    }
}

}  // namespace gyp
