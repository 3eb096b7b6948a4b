// resample_plan.hpp -- what the sample path in front of the correlators (resampler, down-converter, packed stages) launches for a
// shape: the ratio of the two rates, resample_kernel's tiling of the output (grid, LDS, whether it fits), and the mixer's constants.
// Plain C++17 and pure functions of their arguments: no HIP type, no context (tests/resample_plan_model.py restates them;
// tests/test_host_sanitizers.py sweeps one against the other and checks that no tile's span exceeds the LDS reserved for it).
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>

namespace gyp {

// Both rates are whole kHz.  With g = gcd(N_in, N_out) the phase pattern repeats every L = N_out / g outputs and M = N_in / g
// inputs (kernels_resample.hpp); millisecond m holds periods m*g .. m*g+g-1.
struct ResampleRatio { int32_t n_in = 0, n_out = 0, g = 0, L = 0, M = 0; };
inline ResampleRatio resample_ratio(int64_t fs_in, int64_t fs_out) {
    ResampleRatio r;
    r.n_in = (int32_t)(fs_in / 1000);
    r.n_out = (int32_t)(fs_out / 1000);
    r.g = std::gcd(r.n_in, r.n_out);
    r.L = r.n_out / r.g;
    r.M = r.n_in / r.g;
    return r;
}

// resample_kernel's launch for output milliseconds first_ms .. first_ms+n_ms-1 (n_ms >= 1) of n_streams streams: grid
// (n_tiles, n_streams), lds_samples float2 of dynamic LDS, and the kernel's arguments of the same names.  A tile is np_tile periods x
// pc_tile phases; tiles are numbered period tile by period tile, the n_pchunks phase chunks of one fastest.
struct ResampleTiling {
    bool fits;             // false: the launch is refused (grid.x beyond int32 or grid.y beyond 65535) and every other member is 0
    int64_t n_tiles;
    int64_t lds_samples;   // at least the span the kernel stages for any tile
    int64_t p_first, n_periods;
    int32_t np_tile, pc_tile, n_pchunks;
};

// tile_samples is the LDS budget of one tile in input samples (gyp_debug_set "resample_tile_samples"; the packed stages pass 8
// less: their 16-entry level table takes 64 bytes of LDS beside the tile, so five workgroups still fit a CU).  The tile's shape
// does not change an output's bits.
inline ResampleTiling resample_tiling(const ResampleRatio& r, int32_t taps, int32_t n_streams, int64_t first_ms, int32_t n_ms, int32_t tile_samples) {
    ResampleTiling t{};
    const int64_t n_periods = (int64_t)n_ms * r.g;
    const int32_t T = taps, TS = tile_samples;
    int32_t np_tile = 1, pc_tile = r.L, n_pchunks = 1;
    int64_t lds_samples;
    if (r.M + T - 1 <= TS) {      // whole periods: as many as fit (a period's last phase reaches M - 1 + T samples from its first)
        np_tile = (int32_t)std::min<int64_t>(std::max(1, (TS - T + 1) / r.M), n_periods);
        lds_samples = (int64_t)np_tile * r.M + T - 1;
    } else {                      // one period, its phases in chunks whose span fits: pc phases reach less than (pc - 1) M / L + 1 + T samples
        pc_tile = (int32_t)std::max<int64_t>(1, (int64_t)(TS - T - 1) * r.L / r.M);
        n_pchunks = (r.L + pc_tile - 1) / pc_tile;
        lds_samples = std::max(TS, T);   // (a budget below T, which no caller can ask for: one phase alone still stages its T taps)
    }
    const int64_t n_tiles = (n_periods + np_tile - 1) / np_tile * n_pchunks;
    if (n_tiles > INT32_MAX || n_streams > 65535) return t;
    return ResampleTiling{true, n_tiles, lds_samples, first_ms * r.g, n_periods, np_tile, pc_tile, n_pchunks};
}

// The constants of the mixer exp(-j 2 pi ((f_hz * i) mod fs) / fs) the kernels evaluate (ddc_mixer, the tone kernels): the
// frequency reduced into [0, fs) and the two scales of the quarter-turn reduction, 4 / fs and 1 / (2 fs).
struct MixerParams { int64_t fs, f; double q_scale, y_scale; };
inline MixerParams mixer_params(int64_t fs, int64_t f_hz) { return MixerParams{fs, (f_hz % fs + fs) % fs, 4.0 / (double)fs, 0.5 / (double)fs}; }

}  // namespace gyp
