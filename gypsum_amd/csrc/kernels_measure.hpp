// kernels_measure.hpp -- the weak-signal measurement (include/gypsum_hip.h, "weak-signal measurement"; the shared arithmetic is
// measure_plan.hpp's and weak_plan.hpp's).  A part of kernels.hpp.
//
// Three launches per pass, none with an atomic, none with a host round trip in between:
//   weak_measure_plan_kernel   one thread per candidate steps u0 and c0 through the n_ms open-loop milliseconds with weak_advance, as
//                              weak_refine_plan_kernel does, but from the c0 that the device holds: the first pass copies the
//                              candidate's start into the call's state row, a later pass reads what the fold kernel left there.
//   weak_measure_sums_kernel   the hot path: one wavefront per (candidate, millisecond), grid-wide; a workgroup of kMeasureWaves
//                              wavefronts takes a run of as many milliseconds of one candidate and loads the satellite's chips into LDS
//                              once (4 KiB, 256 threads: the shape of weak_refine_sums_kernel).  weak_ms_sums_w is weak_ms_sums with a
//                              seventh float64 accumulator for W = sum |x|^2: the same loop order, products, lane accumulators,
//                              reduction tree and single rounding, so the six sums are the bank's bit for bit
//                              (tests/test_gpu_weak_measure.py holds it to that).  Like the bank's it is bound by vector issue (about
//                              a hundred vector instructions for the 8 bytes of a sample), not by memory or LDS; the float64 work is
//                              seven adds and a multiply-add pair per sample, well under the carrier's and the chip indices' share.
//   weak_measure_fold_kernel   one workgroup per candidate: thread g takes group g (at most 100: measure_group, 20 records and 20 W_m
//                              from global memory, four float64 into LDS), thread 0 adds the groups in order, forms the envelopes and
//                              the correction (measure_close), writes the next pass's c0 and, after the last pass, the record.  The
//                              order is fixed, so a candidate's record is the same bits alone or among others.
#pragma once

#include "kernels_weak.hpp"
#include "measure_plan.hpp"

namespace gyp {

constexpr int kMeasureWaves = 4;                  // wavefronts, and milliseconds, per workgroup of the sums kernel
constexpr int kMeasureThreads = kMeasureWaves * 64;
constexpr int kMeasureFoldThreads = 128;          // >= kMeasureMaxGroups

// A candidate as the host uploads it: the start-up state of a weak bank's channel (weak_fresh_chan) and what the record repeats.
struct WeakMeasureCand {
    int32_t stream, sat_id, edge, pad;
    double f, u0, carrier_phase;
    int64_t c0;
};

// What a candidate carries from pass to pass, device resident.
struct WeakMeasureState {
    int64_t c0;
    double delta;
    int32_t status, pad;
};

// One pass's rows of per-millisecond values: candidate c's row begins at base + (c * stride + row) * n_ms.
template <typename T>
struct WeakMeasureRows {
    T* base;
    int32_t stride, row;
    __host__ __device__ T* of(int cand, int32_t n_ms) const { return base + ((int64_t)cand * stride + row) * n_ms; }
};

struct WeakMeasureArgs {
    const WeakMeasureCand* cands;  // [n_cand]
    WeakMeasureState* states;      // [n_cand]
    WeakMsPlan* plans;             // [n_cand][n_ms]
    WeakMeasureRows<gyp_weak_ms_rec> sums;   // this pass's
    WeakMeasureRows<double> w;
    gyp_weak_measure_fold* folds;  // [n_cand][passes] or NULL
    const float* iq;               // stream s at iq + 2 * s * stream_stride
    int64_t stream_stride;
    const uint8_t* chips;          // [32][1023] in {0, 1}
    gyp_weak_measured* out;        // [n_cand]
    int64_t spacing;
    double fs;
    int64_t first_ms;
    int32_t n, n_ms, n_cand;
    int32_t pass, passes;          // this launch's pass, 0-based
};

__global__ __launch_bounds__(64) void weak_measure_plan_kernel(WeakMeasureArgs p) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= p.n_cand) return;
    const WeakMeasureCand c = p.cands[i];
    if (p.pass == 0) p.states[i] = WeakMeasureState{c.c0, 0.0, 0, 0};
    double u0 = c.u0;
    int64_t c0 = p.pass == 0 ? c.c0 : p.states[i].c0;
    const double du = c.f / p.fs;
    const int64_t r = weak_code_rate(c.f, p.n);
    WeakMsPlan* const row = p.plans + (int64_t)i * p.n_ms;
    for (int32_t m = 0; m < p.n_ms; ++m) {
        row[m] = WeakMsPlan{u0, du, c0, r, 0, 0, (int8_t)kWeakSync, 0};
        weak_advance(&u0, &c0, c.f, p.fs, p.n, r);
    }
}

// weak_ms_sums with W = sum |x|^2 beside it (all 64 lanes; the results are lane 0's).
__device__ __forceinline__ void weak_ms_sums_w(const float2* __restrict__ x, int32_t n, const WeakMsPlan& pl, int64_t d, const float* chips_pm, int lane,
                                               cf& minus, cf& prompt, cf& plus, double& w_out) {
#pragma clang fp contract(off)
    double mr = 0.0, mi = 0.0, pr = 0.0, pi = 0.0, lr = 0.0, li = 0.0, ww = 0.0;
    for (int32_t i = lane; i < n; i += 64) {
        const int32_t k = pl.k_first + i;
        const double step = pl.du * (double)k;
        const cf car = carrier_from_cycles_fast(pl.u_base + step);
        const float2 xi = x[i];
        const cf w = cmul(xi, car);
        const int64_t at = pl.c_base + (int64_t)k * pl.r;
        const float sm = chips_pm[weak_chip_of(at - d)], sp = chips_pm[weak_chip_of(at)], sl = chips_pm[weak_chip_of(at + d)];
        mr += (double)(sm * w.x); mi += (double)(sm * w.y);
        pr += (double)(sp * w.x); pi += (double)(sp * w.y);
        lr += (double)(sl * w.x); li += (double)(sl * w.y);
        const double xr = (double)xi.x, xm = (double)xi.y;
        const double a = xr * xr, b = xm * xm;
        ww += a + b;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        mr += __shfl_down(mr, off); mi += __shfl_down(mi, off);
        pr += __shfl_down(pr, off); pi += __shfl_down(pi, off);
        lr += __shfl_down(lr, off); li += __shfl_down(li, off);
        ww += __shfl_down(ww, off);
    }
    minus = make_float2((float)mr, (float)mi); prompt = make_float2((float)pr, (float)pi); plus = make_float2((float)lr, (float)li);
    w_out = ww;
}

// grid: n_cand x ceil(n_ms / kMeasureWaves), candidate-major
__global__ __launch_bounds__(kMeasureThreads) void weak_measure_sums_kernel(WeakMeasureArgs p) {
    __shared__ float chips_pm[kChips + 1];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int runs = (p.n_ms + kMeasureWaves - 1) / kMeasureWaves;
    const int cand = (int)(blockIdx.x / (unsigned)runs), run = (int)(blockIdx.x % (unsigned)runs);
    const WeakMeasureCand c = p.cands[cand];
    {
        const uint8_t* code = p.chips + (size_t)(c.sat_id - 1) * kChips;
        for (int i = tid; i < kChips; i += kMeasureThreads) chips_pm[i] = code[i] ? 1.0f : -1.0f;
    }
    __syncthreads();
    const int32_t m = run * kMeasureWaves + wave;
    if (m >= p.n_ms) return;                     // (no barrier follows)
    const float2* const x = reinterpret_cast<const float2*>(p.iq) + (int64_t)c.stream * p.stream_stride + (int64_t)m * p.n;
    const WeakMsPlan pl = p.plans[(int64_t)cand * p.n_ms + m];
    cf mi, pr, ls;
    double w;
    weak_ms_sums_w(x, p.n, pl, p.spacing, chips_pm, lane, mi, pr, ls, w);
    if (lane == 0) {
        gyp_weak_ms_rec rec{};
        rec.minus_re = mi.x; rec.minus_im = mi.y; rec.prompt_re = pr.x; rec.prompt_im = pr.y; rec.plus_re = ls.x; rec.plus_im = ls.y;
        rec.pos = 0; rec.phase = (int8_t)kWeakSync;
        p.sums.of(cand, p.n_ms)[m] = rec;
        p.w.of(cand, p.n_ms)[m] = w;
    }
}

// grid: n_cand
__global__ __launch_bounds__(kMeasureFoldThreads) void weak_measure_fold_kernel(WeakMeasureArgs p) {
    __shared__ double ge[4 * kMeasureFoldThreads];
    const int tid = (int)threadIdx.x;
    const int cand = (int)blockIdx.x;
    const WeakMeasureCand c = p.cands[cand];
    const int32_t head = measure_first_head(p.first_ms, c.edge), n_groups = measure_groups(p.n_ms, p.first_ms, c.edge);
    if (tid < n_groups) measure_group(p.sums.of(cand, p.n_ms), p.w.of(cand, p.n_ms), head + tid * kWeakPeriodMs, &ge[4 * tid]);
    __syncthreads();
    if (tid != 0) return;
    WeakMeasureState st = p.states[cand];
    const gyp_weak_measure_fold f = measure_close(ge, n_groups, p.spacing, st.c0);
    {
#pragma clang fp contract(off)
        st.c0 = f.c0; st.delta = st.delta + f.dd; st.status |= f.status;
    }
    p.states[cand] = st;
    if (p.folds) p.folds[(int64_t)cand * p.passes + p.pass] = f;
    if (p.pass + 1 < p.passes) return;
    gyp_weak_measured o{};
    o.stream = c.stream; o.sat_id = c.sat_id;
    o.doppler_hz = c.f; o.carrier_phase = c.carrier_phase;
    o.c0 = st.c0;
    o.code_phase_samples = measure_code_phase_samples(st.c0, p.n);
    o.delta_chips = st.delta; o.dd_last = f.dd; o.cn0_dbhz = f.cn0_dbhz;
    o.edge = c.edge; o.n_groups = n_groups; o.status = st.status;
    p.out[cand] = o;
}

}  // namespace gyp
