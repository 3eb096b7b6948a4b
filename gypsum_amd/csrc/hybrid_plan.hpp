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

// gyp_acquire_weak_dev's search for a shape: the two levels' bins, the offsets of their cell tables in Scratch::hyb_level_cells,
// what it reserves, and hybrid_run's plan for the larger level (reserved once, up front: a buffer that grew between the levels
// would wait for the stream).
constexpr int kWeakMaxSats = 32, kWeakMaxLevelBins = 4096;
struct WeakSearchShape { int n; int n_streams, n_sats, coherent_ms, n_blocks, flags; double center_hz, spread_hz, fine_step_hz; };
struct WeakSearchPlan {
    const char* refusal;               // nullptr: runs; else why not, in the order the entry point has always refused, and every other member is 0
    int n_coarse, fine_half, n_fine;   // fine_half -1, n_fine 0: no fine level
    int64_t n_states;                  // (stream, satellite) pairs
    size_t coarse_cells, fine_cells;   // cell-table offsets: level 0 at 0, level 1 at coarse_cells, the final cells at coarse_cells + fine_cells
    size_t level_cells, records;       // elements of hyb_level_cells and of hyb_records
    HybPlan run;
};
inline WeakSearchPlan weak_search_plan(const WeakSearchShape& s, int scratch_mb) {
    const auto refused = [](const char* why) { WeakSearchPlan r{}; r.refusal = why; return r; };
    if (const char* why = hybrid_refusal(s.coherent_ms, s.n_blocks, s.flags)) return refused(why);
    if (s.n_sats > kWeakMaxSats) return refused("at most 32 satellites per call");
    if (!std::isfinite(s.center_hz) || !std::isfinite(s.spread_hz) || !std::isfinite(s.fine_step_hz) || !(s.spread_hz > 0.0))
        return refused("center, spread and fine step must be finite and the spread positive");
    WeakSearchPlan pl{};
    pl.n_coarse = hybrid_coarse_bins(s.center_hz, s.spread_hz, s.coherent_ms);
    pl.fine_half = hybrid_fine_half(s.fine_step_hz, s.coherent_ms);
    pl.n_fine = pl.fine_half >= 0 ? 2 * pl.fine_half + 1 : 0;
    if (pl.n_coarse < 1 || pl.n_coarse > kWeakMaxLevelBins || pl.n_fine > kWeakMaxLevelBins) return refused("a level must have between 1 and 4096 Doppler bins");
    pl.n_states = (int64_t)s.n_streams * s.n_sats;
    if (pl.n_states * std::max(pl.n_coarse, pl.n_fine) > INT32_MAX) return refused("more than 2^31 - 1 cells");
    const size_t states = (size_t)pl.n_states;
    pl.coarse_cells = states * pl.n_coarse;
    pl.fine_cells = states * pl.n_fine;
    pl.level_cells = pl.coarse_cells + pl.fine_cells + states;
    pl.records = std::max(pl.coarse_cells, pl.fine_cells);
    pl.run = hybrid_plan(HybShape{s.n, (int64_t)pl.records, s.coherent_ms, s.n_blocks, s.flags}, scratch_mb);
    return pl;
}

}  // namespace gyp
