// grid_plan.hpp -- which cells kernel a flat search grid (gyp_correlate_grid_dev) takes, with how many satellites per wavefront and
// branch runs, the scratch it needs and the size of its persistent grid.  Plain C++17 and a pure function of the shape and the A/B
// switches: no HIP types, no context (tests/grid_plan_model.py restates it; tests/test_host_sanitizers.py sweeps one against the other).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace gyp {

struct GridShape { int k, n_cus; int64_t n_units; int n_sats, n_blk; };   // n_units = streams x bins; n_blk = 1 (coherent) or n_ms
struct GridSwitches { bool no_pipe, no_shared_fwd, no_grid_fused, no_grid_parts; int fused_waves; };   // gyp_debug_set names
struct GridPlan {
    int path;         // 1 fused, 2 shared forward, 3 one wavefront per cell, 4 workgroup per cell (gyp_debug_get "last_grid_path")
    bool pipe;        // path 3: grid_cells_wave_pipe_kernel, else grid_cells_wave_kernel
    int waves;        // wavefronts per workgroup of paths 1 and 2
    int gs, parts;    // path 2: satellites per wavefront, runs a unit's K branches are cut into
    bool wide_fold;   // K > 8: wipe + boxcar instead of grid_fold_kernel
    size_t folded_bytes, z_bytes, partial_bytes;   // scratch: folded rows, wiped-off samples of the wide fold, partial statistics
    int wgrid;        // workgroups of the cells launch
};

constexpr size_t kGridCfBytes = 8, kGridPartialBytes = 24;   // sizeof(cf), sizeof(GridPartial): gypsum_hip.hip asserts both
constexpr int kGridChips = 1023;

inline GridPlan grid_plan(const GridShape& s, const GridSwitches& sw) {
    GridPlan pl{};
    const int k = s.k;
    const int64_t n_cells = s.n_units * s.n_sats;
    // workgroups of per_wg items each, `most` at the most
    const auto groups_of = [](int64_t items, int per_wg, int most) { return (int)std::max<int64_t>(1, std::min<int64_t>((items + per_wg - 1) / per_wg, most)); };
    pl.waves = sw.fused_waves == 8 ? 8 : 12;
    pl.gs = pl.parts = 1;
    pl.wide_fold = k > 8;
    // enough units to fill the chip's 2048 wavefront slots twice over, at most 32 satellites, at most 8 samples per chip: the fold is
    // fused into the cells kernel, one wavefront per (stream, bin) unit loops every satellite (no folded rows in HBM)
    if (k <= 8 && s.n_blk == 1 && s.n_sats >= 4 && s.n_sats <= 32 && s.n_units >= (int64_t)s.n_cus * 16 && !sw.no_pipe && !sw.no_shared_fwd &&
        !sw.no_grid_fused) {
        pl.path = 1;
        pl.wgrid = groups_of(s.n_units, pl.waves, s.n_cus);
        return pl;
    }
    pl.folded_bytes = (size_t)s.n_units * s.n_blk * k * 1024 * kGridCfBytes;
    if (pl.wide_fold) pl.z_bytes = (size_t)s.n_units * s.n_blk * (k * kGridChips) * kGridCfBytes;
    // Satellites per wavefront: more of them share a forward transform (1 + gs transforms per gs cells) but make fewer, longer work
    // items -- on a chip the grid does not fill (config 5 on one GPU, anything strong-scaled) the rounds decide.  A chip the items do
    // not fill also runs a last round that is partly empty: a unit's K branches are cut into `parts` runs -- the forward transforms
    // stay shared -- so that the rounds are shorter and the last one costs less (grid_merge_parts_kernel merges the partial statistics).
    // Group size and runs are chosen TOGETHER: cost = (1 + gs) transforms x (K / parts) branches per item x rounds of the chip's
    // wavefront slots, with up to 32 satellites per wavefront and runs down to one branch (chosen one after the other, with gs <= 8 and
    // at most 16 runs, config 5 ran 19 rounds x 4 branches x 9 = 684 transform times; together 19 x 1 x 33 = 627).
    const double slots = s.n_cus * (pl.waves == 8 ? 8.0 : 12.0);
    double cost = 2.0 * k * std::ceil((double)s.n_units * s.n_sats / slots);   // one wavefront per cell: fwd + inv per branch
    for (int gs = 2; gs <= 32; gs *= 2) {
        if (gs / 2 >= s.n_sats) break;
        const double groups = (double)s.n_units * ((s.n_sats + gs - 1) / gs);
        for (int pp = 1; pp <= k; ++pp) {
            if (k % pp || (pp > 1 && sw.no_grid_parts)) continue;
            const double t = (1.0 + gs) * (k / pp) * std::ceil(groups * pp / slots) + (pp > 1 ? 0.25 * (1.0 + gs) : 0.0);   // (+: a merge launch)
            if (t < cost * (pp > 1 ? 0.97 : 1.0)) { cost = t; pl.gs = gs; pl.parts = pp; }
        }
    }
    if (s.n_blk == 1 && pl.gs > 1 && !sw.no_pipe && !sw.no_shared_fwd) {   // one wavefront per (unit, gs satellites, run of branches)
        pl.path = 2;
        if (pl.parts > 1) pl.partial_bytes = (size_t)n_cells * pl.parts * kGridPartialBytes;
        pl.wgrid = groups_of(s.n_units * ((s.n_sats + pl.gs - 1) / pl.gs) * pl.parts, pl.waves, s.n_cus);
        return pl;
    }
    pl.gs = pl.parts = 1;
    if (s.n_blk == 1 && k % 2 == 0 && !sw.no_pipe) {   // one wavefront per cell, 256 VGPRs, next row prefetched
        pl.path = 3;
        pl.pipe = true;
        pl.wgrid = groups_of(n_cells, 8, s.n_cus);
    } else if (s.n_blk == 1 && k <= 8) {   // one wavefront per cell, no barriers
        pl.path = 3;
        pl.wgrid = groups_of(n_cells, 8, s.n_cus * 2);
    } else {   // a workgroup per cell; wavefronts a CU hosts for this rate, in workgroups: k > 8 ? 1 : 16 / k
        pl.path = 4;
        pl.wgrid = (int)std::max<int64_t>(1, std::min<int64_t>(n_cells, (int64_t)s.n_cus * (k > 8 ? 1 : 16 / k)) & ~(int64_t)7);
    }
    return pl;
}

}  // namespace gyp
