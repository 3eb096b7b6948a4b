// hybrid_plan.hpp -- what a hybrid coherent/non-coherent search (gyp_correlate_grid_hybrid_dev, gyp_acquire_weak_dev) runs for a
// shape: whether the request is one the kernels take, the sets of blocks, the cell chunks whose profile + power scratch fits the
// budget, and the two pieces of float64 arithmetic the host and the device must agree on bit for bit: a block's code-Doppler shift
// (gyp_hybrid_shift) and the detection statistic of a set (gyp_hybrid_stats; hybrid_reduce_kernel picks the reported set with it).
// Plain C++17 and pure functions: no HIP call, no context (tests/hybrid_model.py restates them).  The two arithmetic pieces are
// compiled for the device as well when a HIP compiler reads this file.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define GYP_HYB_HD __host__ __device__
#else
#define GYP_HYB_HD
#endif

namespace gyp {

constexpr int kHybAlternate = 1, kHybCodeDoppler = 2;   // GYP_HYB_ALTERNATE, GYP_HYB_CODE_DOPPLER
constexpr int kHybFlagMask = kHybAlternate | kHybCodeDoppler;
constexpr double kL1Hz = 1575420000.0;                  // carrier cycles per second: code Doppler = carrier Doppler / (kL1Hz / 1.023e6) chips/s
constexpr int kHybMaxCoherentMs = 20;                   // one data bit
constexpr int kHybScratchMbMin = 16, kHybScratchMbMax = 65536, kHybScratchMbDefault = 1024;

// Samples by which the correlation peak of block `block` (of coherent_ms milliseconds, n samples each) has moved EARLIER than in
// block 0 at carrier Doppler doppler_hz: a positive Doppler shortens the code period by the factor 1 / (1 + f / kL1Hz), so after
// block * coherent_ms * n samples the code is ahead by that many times f / kL1Hz.  One product and one quotient, each rounded once,
// then round half away from zero.
GYP_HYB_HD inline int32_t hybrid_shift(int32_t n, int32_t coherent_ms, int32_t block, double doppler_hz, int32_t flags) {
#pragma clang fp contract(off)
    if (!(flags & kHybCodeDoppler)) return 0;
    const double elapsed = (double)((int64_t)block * coherent_ms * n);
    const double num = elapsed * doppler_hz;
    const double q = num / kL1Hz;
    if (!(q > -2147483000.0 && q < 2147483000.0)) return 0;   // (not a Doppler: the entry points refuse non-finite bins)
    return (int32_t)llround(q);
}

// z = (peak - mean_off) / std_off of one set's statistics, population variance; NaN where it is not defined (no lag away from the
// peak, or a variance that is not positive).  float64, one rounding per operation.
GYP_HYB_HD inline double hybrid_z(float peak, int32_t n_off, double sum_off, double sumsq_off) {
#pragma clang fp contract(off)
    if (n_off <= 0) return NAN;
    const double nn = (double)n_off;
    const double mean = sum_off / nn;
    const double m2 = sumsq_off / nn;
    const double mm = mean * mean;
    const double var = m2 - mm;
    if (!(var > 0.0)) return NAN;
    const double sd = sqrt(var);
    const double d = (double)peak - mean;
    return d / sd;
}

// The reported set: the one with the larger z; set 0 on a tie, or when either z is NaN.
GYP_HYB_HD inline int hybrid_pick_set(double z0, double z1) { return z1 > z0 ? 1 : 0; }

struct HybShape { int n; int64_t n_cells; int coherent_ms, n_blocks, flags; };   // samples per millisecond; the grid; the search
struct HybPlan {
    bool fits;             // false: refused before anything is reserved or launched, every other member is 0
    int n_sets;            // 2 with kHybAlternate (even blocks, odd blocks), else 1
    int chunk_cells;       // cells per chunk: each holds a float2 profile row and n_sets float power rows in the scratch
    int n_chunks;          // gyp_debug_get "last_hybrid_chunks"
    size_t profile, power; // elements of Scratch::hyb_profile (float2) and hyb_power (float) for one chunk
    int acc_x;             // hybrid_accumulate_kernel: blocks of 256 lags per cell (grid.x), cells in grid.y
};

// Why a request is refused (nullptr: it is not).  The order is the header's.
inline const char* hybrid_refusal(int coherent_ms, int n_blocks, int flags) {
    if (coherent_ms < 1 || coherent_ms > kHybMaxCoherentMs) return "coherent_ms must be 1..20";
    if (n_blocks < 1) return "n_blocks must be at least 1";
    if ((int64_t)n_blocks * coherent_ms > 65535) return "n_blocks * coherent_ms must be at most 65535";
    if (flags & ~kHybFlagMask) return "unknown flag bits";
    if ((flags & kHybAlternate) && n_blocks < 2) return "GYP_HYB_ALTERNATE needs at least 2 blocks";
    return nullptr;
}

inline HybPlan hybrid_plan(const HybShape& s, int scratch_mb) {
    HybPlan pl{};
    if (hybrid_refusal(s.coherent_ms, s.n_blocks, s.flags) || s.n_cells < 1 || s.n_cells > INT32_MAX || s.n < 1) return pl;
    pl.fits = true;
    pl.n_sets = (s.flags & kHybAlternate) ? 2 : 1;
    const size_t cell_bytes = (size_t)s.n * (8 + 4 * (size_t)pl.n_sets);
    const size_t budget = (size_t)scratch_mb << 20;
    // at least one cell per chunk whatever the budget (a cell at 49.104 Msps takes 0.8 MB: far below the smallest budget);
    // at most 65535 cells, the accumulate kernel's grid.y
    const int64_t room = std::max<int64_t>(1, (int64_t)(budget / cell_bytes));
    pl.chunk_cells = (int)std::min<int64_t>({s.n_cells, room, 65535});
    pl.n_chunks = (int)((s.n_cells + pl.chunk_cells - 1) / pl.chunk_cells);
    pl.profile = (size_t)pl.chunk_cells * s.n;
    pl.power = pl.profile * pl.n_sets;
    pl.acc_x = (s.n + 255) / 256;
    return pl;
}

// blocks of set k (blocks_used of a record whose reported set is k)
GYP_HYB_HD inline int hybrid_blocks_in_set(int n_blocks, int n_sets, int set) {
    if (n_sets != 2) return set == 0 ? n_blocks : 0;
    return set == 0 ? (n_blocks + 1) / 2 : n_blocks / 2;
}

// The coarse level of gyp_acquire_weak: bins center - spread + i * (500 / T) while < center + spread (float64, i counted up: no
// running sum).  Returns how many; bin i is hybrid_coarse_bin(...).
inline double hybrid_coarse_bin(double center, double spread, int coherent_ms, int i) { return center - spread + (double)i * (500.0 / coherent_ms); }
inline int hybrid_coarse_bins(double center, double spread, int coherent_ms) {
    int n = 0;
    while (n < 1000000 && hybrid_coarse_bin(center, spread, coherent_ms, n) < center + spread) ++n;
    return n;
}
// The fine level: best + j * step for |j * step| <= 250 / T, j = -J .. J: 2 J + 1 bins (0 when step <= 0: no fine level).
inline int hybrid_fine_half(double step, int coherent_ms) {
    if (!(step > 0.0)) return -1;
    int j = 0;
    while (j < 500000 && (double)(j + 1) * step <= 250.0 / coherent_ms) ++j;
    return j;
}

}  // namespace gyp
