// weak_plan.hpp -- the arithmetic of a weak bank (include/gypsum_hip.h, "weak-signal tracking") that the host and the device
// must agree on, written once: what a request is refused for, a channel's start-up from an acquisition result, the code rate and
// the NCO advances, the bit-edge energies (gyp_weak_bit_sync; weak_track_kernel picks the edge with the same functions) and the
// loop update at the end of a 20-ms period.  Plain C++17 and pure functions over plain structs: no HIP call, no context
// (tests/weak_track_model.py restates them).  Compiled for the device as well when a HIP compiler reads this file.  Contraction is
// off wherever the header promises an order.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/gypsum_hip.h"
#include "hybrid_plan.hpp"

#if defined(__HIPCC__)
#define GYP_WEAK_HD __host__ __device__
#else
#define GYP_WEAK_HD
#endif

namespace gyp {

constexpr int64_t kWeakOne = (int64_t)1 << 40;          // one chip
constexpr int64_t kWeakCodeMod = 1023 * kWeakOne;
constexpr double kWeakL1Hz = kL1Hz;                     // (hybrid_plan.hpp: the search and the loops scale code Doppler by the same number)
constexpr int kWeakPeriodMs = 20, kWeakMuWindow = 25;
constexpr int kWeakSyncMin = 40, kWeakSyncMax = 2000;
constexpr int kWeakSync = 0, kWeakWait = 1, kWeakTrack = 2;   // gyp_weak_state::phase
constexpr int kWeakMaxMs = 65535;

// A channel's whole state, device resident ([n_chan] in the bank).  f, u0, c0 are those of the current period's start (of the next
// millisecond in the open-loop phases).
struct WeakChan {
    int32_t stream, sat_id;
    int32_t status, phase, edge, pos, n_periods, sync_count;
    int64_t sync_start, period_first;
    double f, f_int, u0;
    int64_t c0;
    double s_i, s_q, m_re, m_im, p_re, p_im, wbp;   // the current period's float64 sums so far: prompt, minus, plus, sum |prompt|^2
    double mu[kWeakMuWindow];                        // ring: period k's mu at k % 25
    double mu_mean;
};

inline gyp_weak_params weak_params_default() {
    gyp_weak_params p{};
    p.period_ms = kWeakPeriodMs; p.sync_ms = 400; p.spacing = kWeakOne / 2;
    p.pll_bw_hz = 8.0; p.dll_bw_hz = 1.0; p.lose_mu = 2.5; p.reserved = 0.0;
    return p;
}

// Why a parameter set is refused (nullptr: it is not).
inline const char* weak_params_refusal(const gyp_weak_params& p) {
    if (p.period_ms != kWeakPeriodMs) return "period_ms must be 20";
    if (p.sync_ms < kWeakSyncMin || p.sync_ms > kWeakSyncMax) return "sync_ms must be 40..2000";
    if (p.spacing < 1 || p.spacing > kWeakOne) return "spacing must be 1 .. 2^40";
    if (!(p.pll_bw_hz > 0.0 && p.pll_bw_hz <= 50.0)) return "pll_bw_hz must be in (0, 50]";
    if (!(p.dll_bw_hz > 0.0 && p.dll_bw_hz <= 10.0)) return "dll_bw_hz must be in (0, 10]";
    if (!(p.lose_mu >= 0.0 && p.lose_mu <= 20.0)) return "lose_mu must be in [0, 20]";
    return nullptr;
}
inline const char* weak_init_refusal(const gyp_chan_init& in) {
    if (in.stream < 0) return "a stream index is negative";
    if (in.sat_id < 1 || in.sat_id > 32) return "satellite id out of range";
    if (!std::isfinite(in.doppler_hz)) return "a Doppler is not finite";
    if (!std::isfinite(in.carrier_phase)) return "a carrier phase is not finite";
    return nullptr;
}

GYP_WEAK_HD inline double weak_frac(double x) { return x - floor(x); }

// r = llround((1023 / N) (1 + f / 1575.42e6) 2^40), products left to right, one rounding each.
GYP_WEAK_HD inline int64_t weak_code_rate(double f, int32_t n) {
#pragma clang fp contract(off)
    const double a = 1023.0 / (double)n;
    const double q = f / kWeakL1Hz;
    const double b = 1.0 + q;
    const double ab = a * b;
    return (int64_t)llround(ab * (double)kWeakOne);
}

GYP_WEAK_HD inline int64_t weak_mod_code(int64_t c) {
    c %= kWeakCodeMod;
    return c < 0 ? c + kWeakCodeMod : c;
}

// u0 and c0 after `samples` samples at (f, r).
GYP_WEAK_HD inline void weak_advance(double* u0, int64_t* c0, double f, double fs, int64_t samples, int64_t r) {
#pragma clang fp contract(off)
    const double du = f / fs;
    const double step = du * (double)samples;
    *u0 = weak_frac(*u0 + step);
    *c0 = weak_mod_code(*c0 + samples * r);
}

// Fresh state from an acquisition result, in SYNC from millisecond `cursor`.
inline WeakChan weak_fresh_chan(const gyp_chan_init& in, int32_t n, int64_t cursor) {
    WeakChan s{};
    s.stream = in.stream; s.sat_id = in.sat_id;
    s.phase = kWeakSync; s.edge = -1;
    s.sync_start = cursor;
    s.f = s.f_int = in.doppler_hz;
    s.u0 = weak_frac(in.carrier_phase / (2.0 * 3.14159265358979323846));
    if (!(s.u0 < 1.0)) s.u0 = 0.0;                      // frac of a tiny negative rounds to 1: the header's start-up rule says 0 then
    const double k = (double)(n / 1023);
    s.c0 = weak_mod_code((int64_t)llround((0.5 - (double)in.code_phase) / k * (double)kWeakOne));
    return s;
}

// en[o] of gyp_weak_bit_sync: prompts are interleaved re,im float32 pairs, prompt of millisecond first_ms + i at i.
GYP_WEAK_HD inline double weak_bit_energy(const float* prompts, int32_t n_ms, int64_t first_ms, int32_t o) {
#pragma clang fp contract(off)
    int64_t h = first_ms + (((int64_t)o - first_ms) % 20 + 20) % 20;
    double acc = 0.0;
    int32_t groups = 0;
    for (; h + 20 <= first_ms + n_ms; h += 20) {
        const float* g = prompts + 2 * (h - first_ms);
        double re = 0.0, im = 0.0;
        for (int j = 0; j < 20; ++j) {
            re += (double)g[2 * j];
            im += (double)g[2 * j + 1];
        }
        const double a = re * re;
        const double b = im * im;
        acc += a + b;
        ++groups;
    }
    return groups ? acc / (double)groups : 0.0;
}
// The edge: the largest energy, the lowest offset on a tie.
GYP_WEAK_HD inline int32_t weak_bit_pick(const double* en) {
    int32_t best = 0;
    for (int32_t o = 1; o < 20; ++o)
        if (en[o] > en[best]) best = o;
    return best;
}

// One millisecond's float32 sums into the period's float64 sums.
GYP_WEAK_HD inline void weak_fold_ms(WeakChan* s, float m_re, float m_im, float p_re, float p_im, float l_re, float l_im) {
#pragma clang fp contract(off)
    const double pr = (double)p_re, pi = (double)p_im;
    s->s_i += pr; s->s_q += pi;
    s->m_re += (double)m_re; s->m_im += (double)m_im;
    s->p_re += (double)l_re; s->p_im += (double)l_im;
    const double a = pr * pr;
    const double b = pi * pi;
    s->wbp += a + b;
}

// The end of a TRACK period: the record, the NCO advances with the period's f, the loop updates, the loss test.  s->pos is 20.
GYP_WEAK_HD inline void weak_close_period(WeakChan* s, const gyp_weak_params& p, double fs, int32_t n, gyp_weak_period_rec* out) {
#pragma clang fp contract(off)
    const double two_pi = 6.283185307179586476925;
    const double T = (double)p.period_ms / 1000.0;
    const double i = s->s_i, q = s->s_q;
    const double e_minus = sqrt(s->m_re * s->m_re + s->m_im * s->m_im), e_plus = sqrt(s->p_re * s->p_re + s->p_im * s->p_im);
    const double nbp = i * i + q * q;
    const double mu = s->wbp > 0.0 ? nbp / s->wbp : 0.0;
    const double dphi = i != 0.0 ? atan(q / i) : 0.0;
    const double e_sum = e_plus + e_minus;
    const double dd = e_sum != 0.0 ? 0.5 * (e_plus - e_minus) / e_sum : 0.0;
    gyp_weak_period_rec rec{};
    rec.first_ms = s->period_first; rec.f = s->f; rec.u0 = s->u0; rec.c0 = s->c0;
    rec.i = i; rec.q = q; rec.mu = mu; rec.dphi = dphi; rec.dd = dd;
    rec.bit = i >= 0.0 ? 1 : -1;
    weak_advance(&s->u0, &s->c0, s->f, fs, (int64_t)p.period_ms * n, weak_code_rate(s->f, n));
    const double wn = p.pll_bw_hz / 0.53;
    const double kp = 1.414 * wn, ki = wn * wn;
    s->f_int = s->f_int + ki * dphi * T / two_pi;
    s->f = s->f_int + kp * dphi / two_pi;
    s->c0 = weak_mod_code(s->c0 + (int64_t)llround(4.0 * p.dll_bw_hz * dd * T * (double)kWeakOne));
    s->mu[s->n_periods % kWeakMuWindow] = mu;
    s->n_periods += 1;
    s->pos = 0;
    s->s_i = s->s_q = s->m_re = s->m_im = s->p_re = s->p_im = s->wbp = 0.0;
    s->mu_mean = 0.0;
    if (s->n_periods >= kWeakMuWindow) {
        double sum = 0.0;
        for (int k = 0; k < kWeakMuWindow; ++k) sum += s->mu[(s->n_periods + k) % kWeakMuWindow];   // oldest first
        s->mu_mean = sum / (double)kWeakMuWindow;
        if (s->mu_mean < p.lose_mu) { s->status = 2; rec.status = 1; }
    }
    rec.mu_mean = s->mu_mean;
    if (out) *out = rec;
}

}  // namespace gyp
