// measure_plan.hpp -- the arithmetic of the weak-signal measurement (include/gypsum_hip.h, "weak-signal measurement") that the host
// and the device must agree on, written once: what a request is refused for, the groups of 20 milliseconds at a bit edge, one group's
// four float64 sums, their fold into the envelopes, the correction of c0, the C/N0, the code phase in samples and the state a weak bank
// takes.  Plain C++17 and pure functions over plain arrays: no HIP call, no context (tests/weak_measure_model.py restates them).
// Compiled for the device as well when a HIP compiler reads this file: weak_measure_fold_kernel spreads measure_group over a workgroup
// and closes the pass with measure_close on one thread, measure_estimate below walks both on one thread.  Everything is float64 and
// contraction is off; + - x / and sqrt are correctly rounded on both sides, so the correction agrees bit for bit; log10 is the
// platform's, so the C/N0 agrees to a tolerance.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

#include "../../include/gypsum_hip.h"
#include "weak_plan.hpp"

namespace gyp {

constexpr int32_t kMeasureMinMs = 40, kMeasureMaxMs = 2000;
constexpr int32_t kMeasureMaxGroups = kMeasureMaxMs / kWeakPeriodMs;
constexpr int32_t kMeasureMaxPasses = 4;
constexpr int64_t kMeasureMinSpacing = (int64_t)1 << 36, kMeasureMaxSpacing = (int64_t)1 << 39;

inline gyp_weak_measure_params measure_params_default() {
    gyp_weak_measure_params p{};
    p.spacing = kWeakOne / 2; p.passes = 2; p.reserved = 0;
    return p;
}

// The first group's head as an index into the buffer, and the number of whole groups behind it (gyp_weak_bit_sync's groups for o = edge).
GYP_WEAK_HD inline int32_t measure_first_head(int64_t first_ms, int32_t edge) {
    return (int32_t)((((int64_t)edge - first_ms) % kWeakPeriodMs + kWeakPeriodMs) % kWeakPeriodMs);
}
GYP_WEAK_HD inline int32_t measure_groups(int32_t n_ms, int64_t first_ms, int32_t edge) {
    const int32_t left = n_ms - measure_first_head(first_ms, edge);
    return left < kWeakPeriodMs ? 0 : left / kWeakPeriodMs;
}

// Why a request is refused (nullptr: it is not), in the header's order; the candidates come after (measure_cand_refusal).
inline const char* measure_spacing_refusal(int64_t spacing) {
    return spacing < kMeasureMinSpacing || spacing > kMeasureMaxSpacing ? "spacing must be 2^36 .. 2^39" : nullptr;
}
inline const char* measure_refusal(const gyp_weak_measure_params& p, int32_t n_ms, int64_t first_ms) {
    if (const char* why = measure_spacing_refusal(p.spacing)) return why;
    if (p.passes < 1 || p.passes > kMeasureMaxPasses) return "passes must be 1..4";
    if (n_ms < kMeasureMinMs || n_ms > kMeasureMaxMs) return "n_ms must be 40..2000";
    if (first_ms < 0) return "first_ms is negative";
    return nullptr;
}
inline const char* measure_edge_refusal(int32_t edge, int32_t n_ms, int64_t first_ms) {
    if (edge < 0 || edge >= kWeakPeriodMs) return "an edge is outside 0..19";
    if (measure_groups(n_ms, first_ms, edge) < 1) return "no whole group of 20 milliseconds at an edge";
    return nullptr;
}
inline const char* measure_cand_refusal(const gyp_weak_refined& r, int32_t n, int32_t n_ms, int64_t first_ms) {
    if (const char* why = weak_init_refusal(gyp_chan_init{r.stream, r.sat_id, r.doppler_hz, r.carrier_phase, r.code_phase, 0})) return why;
    if (r.code_phase < 0 || r.code_phase >= n) return "a code phase is outside [0, N)";
    return measure_edge_refusal(r.edge, n_ms, first_ms);
}

// One group's sums: e[0..2] = |sum of the 20 widened minus / prompt / plus|^2, e[3] = the sum of its 20 W_m.  sums: the buffer's
// records, w: its W_m, head: the group's first millisecond as an index into both.
GYP_WEAK_HD inline void measure_group(const gyp_weak_ms_rec* sums, const double* w, int32_t head, double* e) {
#pragma clang fp contract(off)
    double mr = 0.0, mi = 0.0, pr = 0.0, pi = 0.0, lr = 0.0, li = 0.0, ws = 0.0;
    for (int32_t j = 0; j < kWeakPeriodMs; ++j) {
        const gyp_weak_ms_rec& s = sums[head + j];
        mr += (double)s.minus_re; mi += (double)s.minus_im;
        pr += (double)s.prompt_re; pi += (double)s.prompt_im;
        lr += (double)s.plus_re; li += (double)s.plus_im;
        ws += w[head + j];
    }
    const double ma = mr * mr, mb = mi * mi;
    const double pa = pr * pr, pb = pi * pi;
    const double la = lr * lr, lb = li * li;
    e[0] = ma + mb; e[1] = pa + pb; e[2] = la + lb; e[3] = ws;
}

// 10 log10(((E0 - Wn) / Wn) / 0.020), NaN when E0 <= Wn or Wn is 0 (or either is NaN).
GYP_WEAK_HD inline double measure_cn0(double e_prompt, double wn) {
#pragma clang fp contract(off)
    if (!(wn > 0.0) || !(e_prompt > wn)) return std::numeric_limits<double>::quiet_NaN();
    const double snr = (e_prompt - wn) / wn;
    return 10.0 * log10(snr / 0.020);
}

GYP_WEAK_HD inline double measure_envelope(double e, double wn) {
#pragma clang fp contract(off)
    const double over = e - wn;
    return sqrt(over > 0.0 ? over : 0.0);
}

// Steps 3 (the sums over the groups, in increasing h) and 4 from the groups' sums ge[n_groups][4].
GYP_WEAK_HD inline gyp_weak_measure_fold measure_close(const double* ge, int32_t n_groups, int64_t spacing, int64_t c0) {
#pragma clang fp contract(off)
    gyp_weak_measure_fold o{};
    double em = 0.0, ep = 0.0, el = 0.0, wn = 0.0;
    for (int32_t g = 0; g < n_groups; ++g) {
        em += ge[4 * g]; ep += ge[4 * g + 1]; el += ge[4 * g + 2]; wn += ge[4 * g + 3];
    }
    const double a_minus = measure_envelope(em, wn), a_plus = measure_envelope(el, wn);
    const double sum = a_plus + a_minus;
    double dd = 0.0;
    if (sum > 0.0) {
        const double d = (double)spacing / (double)kWeakOne;
        const double gain = 1.0 - d;
        const double diff = a_plus - a_minus;
        dd = gain * diff / sum;
    } else {
        o.status = 1;
    }
    o.e_minus = em; o.e_prompt = ep; o.e_plus = el; o.wn = wn;
    o.dd = dd;
    o.cn0_dbhz = measure_cn0(ep, wn);
    o.c0 = weak_mod_code(c0 + (int64_t)llround(dd * (double)kWeakOne));
    o.n_groups = n_groups;
    return o;
}

// 0.5 - K (c0 / 2^40), + N when negative, 0 where that rounds to N: the inverse of weak_fresh_chan's c0.
GYP_WEAK_HD inline double measure_code_phase_samples(int64_t c0, int32_t n) {
#pragma clang fp contract(off)
    const double k = (double)(n / 1023);
    const double chips = (double)c0 / (double)kWeakOne;
    double cp = 0.5 - k * chips;
    if (cp < 0.0) cp += (double)n;
    if (!(cp < (double)n)) cp = 0.0;
    return cp;
}

// Steps 3-4 on one thread (gyp_weak_measure_estimate); the request is checked.
inline gyp_weak_measure_fold measure_estimate(const gyp_weak_ms_rec* sums, const double* w, int32_t n_ms, int64_t first_ms, int32_t edge,
                                              int64_t spacing, int64_t c0) {
    double ge[4 * kMeasureMaxGroups];
    const int32_t head = measure_first_head(first_ms, edge), n_groups = measure_groups(n_ms, first_ms, edge);
    for (int32_t g = 0; g < n_groups; ++g) measure_group(sums, w, head + g * kWeakPeriodMs, &ge[4 * g]);
    return measure_close(ge, n_groups, spacing, c0);
}

// The state gyp_weak_bank_set_state takes, ms_ahead milliseconds behind the buffer's first (gyp_weak_measured_state); checked.
inline gyp_weak_state measure_state(const gyp_weak_measured& rec, double fs, int32_t n, int32_t ms_ahead) {
    const WeakChan s = weak_fresh_chan(gyp_chan_init{rec.stream, rec.sat_id, rec.doppler_hz, rec.carrier_phase, 0, 0}, n, 0);
    double u0 = s.u0;
    int64_t c0 = rec.c0;
    const int64_t r = weak_code_rate(s.f, n);
    for (int32_t m = 0; m < ms_ahead; ++m) weak_advance(&u0, &c0, s.f, fs, n, r);
    gyp_weak_state o{};
    o.f = o.f_int = s.f; o.u0 = u0; o.c0 = c0;
    o.phase = kWeakWait; o.edge = rec.edge;
    return o;
}

}  // namespace gyp
