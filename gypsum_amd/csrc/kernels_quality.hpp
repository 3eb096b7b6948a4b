// kernels_quality.hpp -- signal quality of tracked channels (include/gypsum_hip.h, "signal quality"): per (channel, window) sums of
// a block's gyp_track_rec records (gyp_track_quality_dev), from which the host arithmetic below derives C/N0 by two estimators, a
// carrier-lock indicator and the share of locked milliseconds (gyp_quality_from_sums).
//
// One 64-lane wavefront per (channel, window) item, four items per 256-thread workgroup over a flat grid (grid-strided where the
// items outnumber it); no LDS, no barrier, no atomics.  A lane reads 12 bytes of each 56-byte record it owns: the prompt peak (8
// bytes at offset 0) and the word at offset 48 that holds the bytes `locked` (49) and `status` (50).  The records come straight out
// of the tracking kernels and are L2-warm behind them.
//
// Records.  Lane l owns records l, l + 64, ... of the window and adds the used ones (status != 2) to its accumulators in that
// order.  Groups.  For a channel with bit offset b >= 0 the window's groups are the runs of 20 records starting at call-relative
// index b + 20 g (g >= 0) that lie inside the window whole, numbered from the window's first; lane l owns groups l, l + 64, ... and
// walks each one's 20 records in order.  Both sets of partial sums are reduced by the fixed tree of kernels_level.hpp -- lane l
// takes lane l + 32, 16, 8, 4, 2, 1 -- and lane 0 writes the record.  Contraction is off: every product, sum and quotient is one
// float64 rounding, so a record is a pure function of its window's records and of b mod 20 relative to the window.
#pragma once

#include <cmath>
#include <cstdint>

// The bit offsets of up to kQualityChans channels travel as a kernel argument (-1 .. 19 fits a byte): no device table, nothing to
// wait for.
constexpr int kQualityChans = 1024;
struct QualityArgs {
    int8_t bit_offset[kQualityChans];
};

constexpr int kGroupMs = 20;   // pseudosymbols per navigation bit

struct QualityPeak {
    float re, im;
    bool used, locked;
};

__device__ __forceinline__ QualityPeak quality_load(const gyp_track_rec* r) {
    const float2 pk = *reinterpret_cast<const float2*>(r);                                   // peak_re, peak_im
    const uint32_t flags = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(r) + 48);   // pseudosymbol, locked, status, nudged
    return QualityPeak{pk.x, pk.y, ((flags >> 16) & 0xffu) != 2u, ((flags >> 8) & 0xffu) != 0u};
}

__global__ __launch_bounds__(256) void track_quality_kernel(const gyp_track_rec* __restrict__ recs, int64_t chan_stride, int32_t n_ms,
                                                            int32_t window_ms, int32_t n_win, int64_t n_items, QualityArgs args,
                                                            gyp_quality_sums* __restrict__ out) {
#pragma clang fp contract(off)
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    for (int64_t it = (int64_t)blockIdx.x * 4 + wave; it < n_items; it += (int64_t)gridDim.x * 4) {
        const int32_t c = (int32_t)(it / n_win), w = (int32_t)(it - (int64_t)c * n_win);
        const gyp_track_rec* row = recs + (int64_t)c * chan_stride;
        const int32_t r0 = w * window_ms;   // < n_ms: w < n_win = ceil(n_ms / window_ms)
        const int32_t r1 = (int64_t)r0 + window_ms < n_ms ? r0 + window_ms : n_ms;
        int32_t n_used = 0, n_locked = 0, n_groups = 0;
        double s2 = 0.0, s4 = 0.0, snp = 0.0, spl = 0.0;
        for (int32_t r = r0 + lane; r < r1; r += 64) {
            const QualityPeak p = quality_load(row + r);
            if (p.used) {
                const double re = (double)p.re, im = (double)p.im;
                const double a = re * re;
                const double b = im * im;
                const double p2 = a + b;
                s2 += p2;
                s4 += p2 * p2;
                n_used += 1;
                n_locked += p.locked ? 1 : 0;
            }
        }
        const int32_t b = args.bit_offset[c];
        if (b >= 0) {
            // the window's first group starts at the first b + 20 g >= r0; groups that end beyond r1 belong to no window
            const int32_t g0 = r0 <= b ? 0 : (r0 - b + kGroupMs - 1) / kGroupMs;
            const int64_t first = (int64_t)b + (int64_t)kGroupMs * g0;
            const int32_t n_g = first + kGroupMs <= r1 ? (int32_t)((r1 - first) / kGroupMs) : 0;
            for (int32_t j = lane; j < n_g; j += 64) {
                const gyp_track_rec* g = row + first + (int64_t)kGroupMs * j;
                double si = 0.0, sq = 0.0, wbp = 0.0;
                bool all_used = true;
#pragma unroll 4
                for (int k = 0; k < kGroupMs; ++k) {
                    const QualityPeak p = quality_load(g + k);
                    const double re = (double)p.re, im = (double)p.im;
                    const double a = re * re;
                    const double bb = im * im;
                    si += re;
                    sq += im;
                    wbp += a + bb;
                    all_used = all_used && p.used;
                }
                const double ii = si * si;
                const double qq = sq * sq;
                const double nbp = ii + qq;
                const double nbd = ii - qq;
                if (all_used && wbp > 0.0 && nbp > 0.0) {
                    snp += nbp / wbp;
                    spl += nbd / nbp;
                    n_groups += 1;
                }
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            s2 += __shfl_down(s2, off, 64);
            s4 += __shfl_down(s4, off, 64);
            snp += __shfl_down(snp, off, 64);
            spl += __shfl_down(spl, off, 64);
            n_used += __shfl_down(n_used, off, 64);
            n_locked += __shfl_down(n_locked, off, 64);
            n_groups += __shfl_down(n_groups, off, 64);
        }
        if (lane == 0) {
            gyp_quality_sums r;
            r.n_used = n_used;
            r.n_locked = n_locked;
            r.n_groups = n_groups;
            r.reserved = 0;
            r.sum_p2 = s2;
            r.sum_p4 = s4;
            r.sum_np = snp;
            r.sum_pl = spl;
            out[it] = r;
        }
    }
}

// gyp_quality_from_sums' arithmetic (the header states the order): float64, one rounding per operation, contraction off -- or the
// compiler would fuse t - M4 and M2 - Pd with what stands in front of them.  An estimate that is not defined is NaN.
static void quality_from_sums(const gyp_quality_sums* sums, int32_t n, gyp_quality* out) {
#pragma clang fp contract(off)
    int64_t n_used = 0, n_locked = 0, n_groups = 0;
    double S2 = 0.0, S4 = 0.0, Snp = 0.0, Spl = 0.0;
    for (int32_t i = 0; i < n; ++i) {
        n_used += sums[i].n_used;
        n_locked += sums[i].n_locked;
        n_groups += sums[i].n_groups;
        S2 += sums[i].sum_p2;
        S4 += sums[i].sum_p4;
        Snp += sums[i].sum_np;
        Spl += sums[i].sum_pl;
    }
    const double nan = std::nan("");
    gyp_quality q = {nan, nan, nan, nan, (int32_t)n_used, (int32_t)n_groups};
    if (n_used >= 2) {
        const double nn = (double)n_used;
        const double M2 = S2 / nn, M4 = S4 / nn;
        const double a = M2 * M2;
        const double t = a + a;
        const double d = t - M4;
        if (d > 0.0) {
            const double Pd = std::sqrt(d);
            const double Pn = M2 - Pd;
            if (Pn > 0.0) {
                const double snr = Pd / Pn;
                const double x = snr * 1000.0;
                q.cn0_m2m4_dbhz = 10.0 * std::log10(x);
            }
        }
    }
    if (n_groups >= 1) {
        const double G = (double)n_groups;
        const double mu = Snp / G;
        if (mu > 1.0 && mu < 20.0) {
            const double num = mu - 1.0;
            const double den = 20.0 - mu;
            const double snr = num / den;
            const double x = snr * 1000.0;
            q.cn0_nwpr_dbhz = 10.0 * std::log10(x);
        }
        q.phase_lock = Spl / G;
    }
    if (n_used >= 1) q.locked_share = (double)n_locked / (double)n_used;
    *out = q;
}
