// acq_plan.hpp -- what a search (gyp_acquire_dev, gyp_search_level_dev) runs for a shape: whether it fits the kernels' 32-bit cell
// indices and grids, how many levels, how many of them through the shared-forward kernels and with room for how many units, the
// elements of every acq_* scratch buffer, the grids of the bookkeeping launches, and the parts a multi-stream scan goes through in.
// Plain C++17 and a pure function of the shape, the search, three gyp_params and the A/B switches: no HIP call, no context
// (tests/acq_plan_model.py restates it; tests/test_host_sanitizers.py sweeps one against the other).  Include after kernels.hpp:
// kMaxBins, kSpecUnitMs and cf are the kernels' own.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace gyp {

struct AcqShape { int k, n, n_streams, n_sats, n_ms; };                 // samples per chip and per millisecond; the search
struct AcqSearch { double center0, spread0; bool single_level; };       // first level; one level (gyp_search_level_dev) or down to acq_min_spread_hz
struct AcqLevels { double initial_spread_hz, min_spread_hz, bins_per_spread; };   // gyp_params::acq_initial_spread_hz, acq_min_spread_hz, acq_bins_per_spread
struct AcqSwitches { bool no_pipe, no_acq_shared_fwd, no_acq_split, is_helper; int acq_lanes; };   // gyp_debug_set names; a helper context
constexpr int kMaxAcqLanes = 4;
struct AcqPlan {
    bool fits;                   // false: the search is refused before anything is reserved or launched, and every other member is 0
    int n_states, n_cells;       // (stream, satellite) pairs; kMaxBins cells each
    int n_levels;                // levels the search runs (gyp_debug_get "last_acq_levels")
    int shared_levels;           // the first of them, through the shared-forward kernels ("last_acq_shared_levels")
    double bins_per_spread;      // acq_plan_kernel's bins of a level
    int max_units;               // room of the spectra buffer, in (stream, bin) units; 0: nothing is shared
    size_t states, cells, out, refined, partial64, profiles, spectra;   // elements of Scratch::acq_* and of partial64 (acq_book_layout and acq_units_layout take n_cells and max_units)
    int tpb, nblk;               // one thread per state: init, plan, reduce, finish (and refine-sum's 64 states per block)
    int refine_x, refine_y;      // acq_refine_kernel: candidate slots x milliseconds
    int exact_z;                 // acq_exact_profile_kernel's z and acq_exact_decide_kernel's grid: blocks that walk the states
    int lanes;                   // parts of a scan ("last_acq_lanes": those actually used) ...
    int lane_first[kMaxAcqLanes], lane_streams[kMaxAcqLanes];   // ... and each part's first stream and streams
};

static_assert(sizeof(cf) == 8, "the room for shared-forward units is counted in complex64 spectra");

inline AcqPlan acq_plan(const AcqShape& s, const AcqSearch& q, const AcqLevels& lv, const AcqSwitches& sw) {
    AcqPlan pl{};
    // cells are indexed in int32 on the device, and the refine kernel's grid has a row of blocks per millisecond
    const int64_t n_states = (int64_t)s.n_streams * s.n_sats;
    if (n_states * kMaxBins > INT32_MAX || s.n_ms > 65535) return pl;
    pl.fits = true;
    pl.n_states = (int)n_states;
    pl.n_cells = pl.n_states * kMaxBins;
    pl.bins_per_spread = lv.bins_per_spread;
    const size_t n_cells = (size_t)pl.n_cells;
    // Shared forward transforms (K == 8, the pipelined path): the first three levels of a scan put every satellite of a stream on the
    // same Doppler bins -- range(-7000, 7000, 700) for all at level 1, multiples of 350 and 175 Hz at levels 2 and 3 -- so the
    // wipe-off and the 8 forward transforms of a (stream, bin) unit are run once (corr_cells_pipe_kernel MODE 1) and read back by
    // each of its satellites (MODE 2).  From level 4 on every satellite has a grid of its own: no unit to speak of.  The spectra
    // take 128 KiB per unit-millisecond: room for 3 * kMaxBins units per stream (level 3 needs ~70 at most), capped at 1 GiB; units
    // beyond the room stay on the unshared kernel.  (min(1 GiB, units x unit_bytes) / unit_bytes, without the product.)
    if (s.k == 8 && !sw.no_pipe && !sw.no_acq_shared_fwd) {
        const size_t unit_bytes = (size_t)s.n_ms * kSpecUnitMs * sizeof(cf);
        pl.max_units = (int)std::min({n_cells, ((size_t)1 << 30) / unit_bytes, (size_t)s.n_streams * 3 * kMaxBins});
    }
    // acquisition.py:81,89: halve the spread down to the smallest one, or stay at the one level asked for (levels 1-3 of a scan share)
    for (double spread = q.spread0; q.single_level ? spread == q.spread0 : spread >= lv.min_spread_hz; spread /= 2.0) {
        if (pl.max_units > 0 && spread * 4.0 >= lv.initial_spread_hz) ++pl.shared_levels;
        ++pl.n_levels;
    }
    pl.states = (size_t)pl.n_states;
    pl.cells = pl.out = pl.refined = n_cells;
    pl.partial64 = n_cells * (size_t)s.n_ms;                      // per-ms magnitudes of the candidates
    pl.profiles = (size_t)pl.n_states * 2 * s.n;                  // float64 profile rows of the (rare) cross-level near-ties
    pl.spectra = (size_t)pl.max_units * s.n_ms * kSpecUnitMs;
    pl.tpb = 64;
    pl.nblk = (pl.n_states + pl.tpb - 1) / pl.tpb;
    // normally one or two candidates per (stream, satellite): 2 n_states slots x n_ms blocks, strided beyond that
    pl.refine_x = (int)std::min<int64_t>(pl.n_cells, 2 * n_states);
    pl.refine_y = s.n_ms;
    // (pending pairs are rare -- about one acquisition in a hundred: a short z grid whose blocks walk the states)
    pl.exact_z = std::min(pl.n_states, 32);
    // A scan is ten levels of one big correlation launch each plus eight small bookkeeping launches (the tie-breaks, the reductions:
    // ~3 ms of a 13-stream scan during which the chip is almost empty, profiles/r03y_acq_timeline.txt) and the big launches end in
    // a ragged last round of workgroups.  Streams are searched independently of each other, so a scan of several streams goes
    // through in parts on several HIP streams -- the others on helper contexts of their own (own scratch and tables): one part's
    // big launch fills the chip while another part is in its small ones.  Same results bit for bit.  At least two streams per part,
    // the remaining streams spread evenly over the remaining parts.
    pl.lanes = sw.is_helper || sw.no_acq_split ? 1 : std::max(1, std::min({sw.acq_lanes, s.n_streams / 2, kMaxAcqLanes}));
    for (int i = 0, s0 = 0; i < pl.lanes; ++i) {
        pl.lane_first[i] = s0;
        s0 += pl.lane_streams[i] = (s.n_streams - s0) / (pl.lanes - i);
    }
    return pl;
}

}  // namespace gyp
