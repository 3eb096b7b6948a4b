// refine_plan.hpp -- the arithmetic of the weak-signal hand-over (include/gypsum_hip.h, "weak-signal hand-over") that the host and
// the device must agree on, written once: what a request is refused for, the shape of the periodogram, the squared pre-sums, one
// bin's sum, the pick with its interpolation and quality figure, the carrier phase, the derotation in front of the bit-edge energies
// (weak_plan.hpp's, unchanged) and the edge ratio.  Plain C++17 and pure functions over plain arrays: no HIP call, no context
// (tests/weak_refine_model.py restates them).  Compiled for the device as well when a HIP compiler reads this file: weak_refine_estimate_kernel
// spreads the same functions over a workgroup, refine_estimate below walks them on one thread.  Everything is float64 and contraction
// is off; the sine and cosine are the platform's (libm on the host, the device library on the GPU), which is why the two sides agree
// to a tolerance and not bit for bit.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "../../include/gypsum_hip.h"
#include "weak_plan.hpp"

namespace gyp {

constexpr int32_t kRefineMinMs = 40, kRefineMaxMs = 2000;
constexpr int32_t kRefineMinGroups = 8, kRefineMaxBins = 4097;

inline gyp_weak_refine_params refine_params_default() {
    gyp_weak_refine_params p{};
    p.span_hz = 20.0; p.step_hz = 0.5; p.presum_ms = 4; p.reserved = 0;
    return p;
}

// L, G, J and the guard of the quality figure for a checked request.
struct RefineShape {
    int32_t n_ms, L, G, J, n_bins, guard;
    double step_hz;
};

GYP_WEAK_HD inline RefineShape refine_shape(const gyp_weak_refine_params& p, int32_t n_ms) {
#pragma clang fp contract(off)
    RefineShape s{};
    s.n_ms = n_ms; s.L = p.presum_ms; s.G = n_ms / p.presum_ms;
    s.J = (int32_t)floor(p.span_hz / p.step_hz);
    s.n_bins = 2 * s.J + 1;
    const double width = (double)n_ms * p.step_hz;
    s.guard = (int32_t)ceil(1000.0 / width);
    s.step_hz = p.step_hz;
    return s;
}

// Why a request is refused (nullptr: it is not), in the header's order.
inline const char* refine_refusal(const gyp_weak_refine_params& p, int32_t n_ms, int64_t first_ms) {
    if (!(p.span_hz > 0.0 && p.span_hz <= 100.0)) return "span_hz must be in (0, 100]";
    if (!(p.step_hz >= 0.01 && p.step_hz <= p.span_hz)) return "step_hz must be in [0.01, span_hz]";
    const int32_t L = p.presum_ms;
    if (!(L == 1 || L == 2 || L == 4 || L == 5 || L == 10 || L == 20)) return "presum_ms must be one of 1, 2, 4, 5, 10, 20";
    if (p.span_hz >= 250.0 / (double)L) return "span_hz must be below 250 / presum_ms";
    if (floor(p.span_hz / p.step_hz) > (double)((kRefineMaxBins - 1) / 2)) return "more than 4097 bins";
    if (n_ms < kRefineMinMs || n_ms > kRefineMaxMs) return "n_ms must be 40..2000";
    if (n_ms / L < kRefineMinGroups) return "fewer than 8 groups of presum_ms milliseconds";
    if (first_ms < 0) return "first_ms is negative";
    return nullptr;
}

// (cos, sin)(-2 pi c) for a phase of c cycles, reduced to [-1/2, 1/2] first.
GYP_WEAK_HD inline void refine_rotor(double cycles, double* wr, double* wi) {
#pragma clang fp contract(off)
    const double c = cycles - rint(cycles);
    const double a = -6.283185307179586476925 * c;
    *wr = cos(a); *wi = sin(a);
}

// s_g = q_g^2 with q_g the sum, in order, of the L prompts of group g widened.
GYP_WEAK_HD inline void refine_group_square(const float* prompts, int32_t g, int32_t L, double* re, double* im) {
#pragma clang fp contract(off)
    const float* p = prompts + 2 * (size_t)g * L;
    double qr = 0.0, qi = 0.0;
    for (int32_t i = 0; i < L; ++i) {
        qr += (double)p[2 * i];
        qi += (double)p[2 * i + 1];
    }
    const double a = qr * qr;
    const double b = qi * qi;
    *re = a - b;
    const double c = 2.0 * qr;
    *im = c * qi;
}

// t_g in seconds: the middle of group g.
GYP_WEAK_HD inline double refine_group_time(int32_t g, int32_t L) {
#pragma clang fp contract(off)
    const double first = (double)(g * L);
    const double half = 0.5 * (double)L;
    return (first + half) / 1000.0;
}

// Y(f) = sum over g, in increasing g, of s_g exp(-2 pi i 2 f t_g); s: G interleaved re,im pairs.
GYP_WEAK_HD inline void refine_sum_at(const double* s, int32_t G, int32_t L, double f_hz, double* yr, double* yi) {
#pragma clang fp contract(off)
    double ar = 0.0, ai = 0.0;
    const double f2 = 2.0 * f_hz;
    for (int32_t g = 0; g < G; ++g) {
        double wr, wi;
        refine_rotor(f2 * refine_group_time(g, L), &wr, &wi);
        const double sr = s[2 * g], si = s[2 * g + 1];
        const double rr = sr * wr;
        const double ii = si * wi;
        const double ri = sr * wi;
        const double ir = si * wr;
        ar += rr - ii;
        ai += ri + ir;
    }
    *yr = ar; *yi = ai;
}

// P_j, j = -J..J at index j + J.
GYP_WEAK_HD inline double refine_bin_power(const double* s, const RefineShape& sh, int32_t index) {
#pragma clang fp contract(off)
    double yr, yi;
    const double f = (double)(index - sh.J) * sh.step_hz;
    refine_sum_at(s, sh.G, sh.L, f, &yr, &yi);
    const double a = yr * yr;
    const double b = yi * yi;
    return a + b;
}

struct RefinePick {
    int32_t bin, status;
    double delta_hz, peak_to_mean;
};

// The arg-max (the lowest index on a tie), the parabola through it and its neighbours, and P[k] over the mean of the bins more than
// `guard` away.  A row without a positive value has no peak: the centre bin, delta 0, NaN and status 1.
GYP_WEAK_HD inline RefinePick refine_pick(const double* P, const RefineShape& sh) {
#pragma clang fp contract(off)
    RefinePick out{};
    int32_t k = 0;
    for (int32_t j = 1; j < sh.n_bins; ++j)
        if (P[j] > P[k]) k = j;
    if (!(P[k] > 0.0)) {
        out.bin = sh.J; out.status = 1; out.delta_hz = 0.0;
        out.peak_to_mean = std::numeric_limits<double>::quiet_NaN();
        return out;
    }
    double d = 0.0;
    const bool at_end = k == 0 || k == sh.n_bins - 1;
    if (!at_end) {
        const double twice = 2.0 * P[k];
        const double den = P[k - 1] - twice + P[k + 1];
        if (den < 0.0) {
            const double num = 0.5 * (P[k - 1] - P[k + 1]);
            d = num / den;
            if (d > 0.5) d = 0.5;
            if (d < -0.5) d = -0.5;
        }
    }
    out.bin = k; out.status = at_end ? 1 : 0;
    out.delta_hz = ((double)(k - sh.J) + d) * sh.step_hz;
    double sum = 0.0;
    int32_t count = 0;
    for (int32_t j = 0; j < sh.n_bins; ++j) {
        const int32_t away = j > k ? j - k : k - j;
        if (away > sh.guard) { sum += P[j]; ++count; }
    }
    out.peak_to_mean = count ? P[k] / (sum / (double)count) : std::numeric_limits<double>::quiet_NaN();
    return out;
}

// x wrapped to (-pi, pi].
GYP_WEAK_HD inline double refine_wrap_phase(double x) {
#pragma clang fp contract(off)
    const double pi = 3.14159265358979323846, two_pi = 6.283185307179586476925;
    const double turns = ceil((x - pi) / two_pi);
    return x - two_pi * turns;
}

// carrier_phase + angle(Y*) / 2, wrapped: right modulo pi.
GYP_WEAK_HD inline double refine_carrier_phase(double carrier_phase, double yr, double yi) {
#pragma clang fp contract(off)
    const double half = 0.5 * atan2(yi, yr);
    return refine_wrap_phase(carrier_phase + half);
}

// p'_m = p_m exp(-2 pi i delta (m + 0.5) / 1000), each part rounded to float32 once.
GYP_WEAK_HD inline void refine_derotate(float re, float im, double delta_hz, int32_t m, float* out_re, float* out_im) {
#pragma clang fp contract(off)
    double wr, wi;
    const double t = ((double)m + 0.5) / 1000.0;
    refine_rotor(delta_hz * t, &wr, &wi);
    const double pr = (double)re, pi = (double)im;
    const double rr = pr * wr;
    const double ii = pi * wi;
    const double ri = pr * wi;
    const double ir = pi * wr;
    *out_re = (float)(rr - ii);
    *out_im = (float)(ri + ir);
}

// The largest of the twenty energies over the second largest (en[best] is the largest; NaN when both are 0).
GYP_WEAK_HD inline double refine_edge_ratio(const double* en, int32_t best) {
    int32_t second = best == 0 ? 1 : 0;
    for (int32_t o = 0; o < kWeakPeriodMs; ++o)
        if (o != best && en[o] > en[second]) second = o;
    return en[best] / en[second];
}

// Steps 2-7 on one thread.  f0 and phase0 are the candidate's Doppler and carrier phase (0 for gyp_weak_refine_estimate); stream, sat_id
// and code_phase of *out are the caller's.
inline void refine_estimate(const float* prompts, int32_t n_ms, int64_t first_ms, const gyp_weak_refine_params& prm, double f0, double phase0,
                            gyp_weak_refined* out) {
    const RefineShape sh = refine_shape(prm, n_ms);
    std::vector<double> s(2 * (size_t)sh.G), P((size_t)sh.n_bins);
    for (int32_t g = 0; g < sh.G; ++g) refine_group_square(prompts, g, sh.L, &s[2 * g], &s[2 * g + 1]);
    for (int32_t j = 0; j < sh.n_bins; ++j) P[j] = refine_bin_power(s.data(), sh, j);
    const RefinePick pick = refine_pick(P.data(), sh);
    double yr, yi;
    refine_sum_at(s.data(), sh.G, sh.L, pick.delta_hz, &yr, &yi);
    std::vector<float> rot(2 * (size_t)n_ms);
    for (int32_t m = 0; m < n_ms; ++m) refine_derotate(prompts[2 * m], prompts[2 * m + 1], pick.delta_hz, m, &rot[2 * m], &rot[2 * m + 1]);
    double en[kWeakPeriodMs];
    for (int o = 0; o < kWeakPeriodMs; ++o) en[o] = weak_bit_energy(rot.data(), n_ms, first_ms, o);
    out->edge = weak_bit_pick(en);
    out->edge_ratio = refine_edge_ratio(en, out->edge);
    out->doppler_hz = f0 + pick.delta_hz;
    out->carrier_phase = refine_carrier_phase(phase0, yr, yi);
    out->delta_hz = pick.delta_hz; out->peak_to_mean = pick.peak_to_mean;
    out->bin = pick.bin; out->status = pick.status;
}

}  // namespace gyp
