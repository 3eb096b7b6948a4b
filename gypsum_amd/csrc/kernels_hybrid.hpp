// kernels_hybrid.hpp -- hybrid coherent/non-coherent search (include/gypsum_hip.h, "weak-signal acquisition"): what joins the
// coherent profiles corr_cells_kernel writes, one block of coherent_ms milliseconds at a time, into a detection record per cell.
// A part of kernels.hpp (which lists every kernel).
//
//   hybrid_grid_cells_kernel   the gyp_cell_desc table of a flat grid (stream x satellite x bin, bins fastest).
//   hybrid_accumulate_kernel   P_k[l] (+)= |C_b[(l - delta_b) mod N]|^2 for one block b of every cell of a chunk: thread l of a cell
//                              reads one float2 of the block's profile row at the rotated index -- two contiguous runs around the wrap,
//                              so a wavefront's 512 bytes stay coalesced -- and adds re^2 + im^2 (float32, one rounding per operation)
//                              to the power row of the block's set.  The first block of a set stores: no memset pass.  HBM-bound:
//                              8 bytes read + 4 read + 4 written per lag and block.
//   hybrid_reduce_kernel       one 256-thread workgroup per cell, its sets one after the other.  Pass 1: thread t walks lags t,
//                              t + 256, ... keeping (largest value, lowest index); lane l takes lane l + 32, 16, 8, 4, 2, 1 of its
//                              wavefront, the four wavefronts meet in LDS.  Pass 2, over the lags more than a chip from that arg-max
//                              (circular distance): the same for the second peak, and float64 sum / sum of squares in that fixed order
//                              -- thread-strided partials, the wavefront tree, then ((w0 + w1) + w2) + w3.  Thread 0 forms z of each
//                              set (hybrid_z, the host's own function), picks the set and writes the record.  No atomics: a record is
//                              a pure function of its cell's power rows.
//   hybrid_coarse_cells_kernel / hybrid_select_kernel / hybrid_finish_kernel   gyp_acquire_weak_dev's bookkeeping, one thread per
//                              (stream, satellite): the coarse level's cell table; the best bin of a level by z (float64, hybrid_z;
//                              the lowest bin wins a tie, NaN never wins) and from it the next level's cell table or the final cell
//                              (tap at the code phase); the carrier phase from that cell's tap into the result.
// Every table and record is written by plain vector stores of the thread that owns it.
#pragma once
#include "hybrid_plan.hpp"
#include "kernels_common.hpp"

namespace gyp {

__global__ __launch_bounds__(256) void hybrid_grid_cells_kernel(const int32_t* __restrict__ sat_ids, const double* __restrict__ doppler,
                                                                int32_t n_sats, int32_t n_bins, int32_t n_cells, gyp_cell_desc* __restrict__ cells) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_cells) return;
    const int32_t bin = (int32_t)(c % n_bins);
    const int64_t row = c / n_bins;
    gyp_cell_desc d;
    d.stream = (int32_t)(row / n_sats);
    d.sat_id = sat_ids[row % n_sats];
    d.doppler_hz = doppler[bin];
    d.tap_index = -1;
    d.reserved = 0;
    cells[c] = d;
}

struct HybAccParams {
    const float2* profile;        // [chunk cells][n] the block's coherent profiles
    float* power;                 // [chunk cells][n_sets][n]
    const gyp_cell_desc* cells;   // the chunk's cells (their Doppler gives the shift)
    int32_t n, coherent_ms, block, flags, n_sets;
};

__global__ __launch_bounds__(256) void hybrid_accumulate_kernel(HybAccParams p) {
#pragma clang fp contract(off)
    const int32_t l = (int32_t)blockIdx.x * 256 + (int32_t)threadIdx.x;
    if (l >= p.n) return;
    const int64_t cell = blockIdx.y;
    const int32_t delta = hybrid_shift(p.n, p.coherent_ms, p.block, p.cells[cell].doppler_hz, p.flags);   // uniform over the workgroup
    int32_t dm = delta % p.n;   // (l - delta) mod n with dm in [0, n)
    if (dm < 0) dm += p.n;
    const int32_t src = l >= dm ? l - dm : l - dm + p.n;
    const float2 c = p.profile[cell * p.n + src];
    const float a = c.x * c.x;
    const float b = c.y * c.y;
    const float pw = a + b;
    const int32_t set = p.n_sets == 2 ? (p.block & 1) : 0;
    float* row = p.power + (cell * p.n_sets + set) * p.n;
    row[l] = p.block < p.n_sets ? pw : row[l] + pw;
}

struct HybPair { float v; int32_t i; };
// the better of two (value, index) pairs: the larger value, the lower index among equal values
__device__ __forceinline__ HybPair hyb_better(HybPair a, HybPair b) { return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a; }
__device__ __forceinline__ HybPair hyb_wave_best(HybPair x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        HybPair o;
        o.v = __shfl_down(x.v, off, 64);
        o.i = __shfl_down(x.i, off, 64);
        x = hyb_better(x, o);
    }
    return x;
}

struct HybSetStats { float peak, second; int32_t argmax, second_argmax, n_off; double sum_off, sumsq_off; };

__global__ __launch_bounds__(256) void hybrid_reduce_kernel(const float* __restrict__ power, int32_t n, int32_t n_sets, int32_t n_blocks,
                                                            gyp_hybrid_cell* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ HybPair s_best[4];
    __shared__ double s_sum[4], s_sq[4];
    __shared__ int32_t s_cnt[4];
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t cell = blockIdx.x;
    const int32_t spc = n / kChips;
    const HybPair none = {-1.0f, 0x7fffffff};   // below every power; a row of NaN keeps it
    HybSetStats st[2];
    for (int32_t set = 0; set < n_sets; ++set) {
        const float* row = power + (cell * n_sets + set) * n;
        HybPair best = none;
        for (int32_t l = t; l < n; l += 256) best = hyb_better(best, HybPair{row[l], l});
        best = hyb_wave_best(best);
        if (lane == 0) s_best[wave] = best;
        __syncthreads();
        const HybPair pk = hyb_better(hyb_better(hyb_better(s_best[0], s_best[1]), s_best[2]), s_best[3]);
        __syncthreads();
        HybPair sec = none;
        double sum = 0.0, sq = 0.0;
        int32_t cnt = 0;
        for (int32_t l = t; l < n; l += 256) {
            int32_t d = l > pk.i ? l - pk.i : pk.i - l;
            d = d < n - d ? d : n - d;
            if (d > spc) {
                const float v = row[l];
                const double v64 = (double)v;
                sec = hyb_better(sec, HybPair{v, l});
                sum += v64;
                sq += v64 * v64;
                cnt += 1;
            }
        }
        sec = hyb_wave_best(sec);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            sum += __shfl_down(sum, off, 64);
            sq += __shfl_down(sq, off, 64);
            cnt += __shfl_down(cnt, off, 64);
        }
        if (lane == 0) { s_best[wave] = sec; s_sum[wave] = sum; s_sq[wave] = sq; s_cnt[wave] = cnt; }
        __syncthreads();
        if (t == 0) {
            const HybPair s2 = hyb_better(hyb_better(hyb_better(s_best[0], s_best[1]), s_best[2]), s_best[3]);
            HybSetStats& r = st[set];
            r.peak = pk.v;
            r.argmax = pk.i;
            r.n_off = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
            r.second = r.n_off > 0 ? s2.v : 0.0f;
            r.second_argmax = r.n_off > 0 ? s2.i : -1;
            r.sum_off = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
            r.sumsq_off = ((s_sq[0] + s_sq[1]) + s_sq[2]) + s_sq[3];
        }
        __syncthreads();   // the next set's partial results reuse the LDS words
    }
    if (t == 0) {
        int32_t set = 0;
        if (n_sets == 2)
            set = hybrid_pick_set(hybrid_z(st[0].peak, st[0].n_off, st[0].sum_off, st[0].sumsq_off),
                                  hybrid_z(st[1].peak, st[1].n_off, st[1].sum_off, st[1].sumsq_off));
        const HybSetStats& r = st[set];
        gyp_hybrid_cell o;
        o.peak = r.peak;
        o.argmax = r.argmax;
        o.second = r.second;
        o.second_argmax = r.second_argmax;
        o.n_off = r.n_off;
        o.set = set;
        o.sum_off = r.sum_off;
        o.sumsq_off = r.sumsq_off;
        o.blocks_used = hybrid_blocks_in_set(n_blocks, n_sets, set);
        o.reserved = 0;
        out[cell] = o;
    }
}

// ---------------------------------------------------------------------------------------------------------
// gyp_acquire_weak_dev: the two levels' bookkeeping, one thread per (stream, satellite) state
// ---------------------------------------------------------------------------------------------------------
struct HybSatIds { int32_t v[32]; };   // travels as a kernel argument: no device table, nothing to wait for

__global__ __launch_bounds__(64) void hybrid_coarse_cells_kernel(HybSatIds ids, int32_t n_sats, int32_t n_states, int32_t n_bins, double center,
                                                                 double spread, int32_t coherent_ms, gyp_cell_desc* __restrict__ cells) {
#pragma clang fp contract(off)
    const int32_t s = (int32_t)blockIdx.x * 64 + (int32_t)threadIdx.x;
    if (s >= n_states) return;
    const double lo = center - spread, step = 500.0 / coherent_ms;
    for (int32_t i = 0; i < n_bins; ++i) {
        gyp_cell_desc d;
        d.stream = s / n_sats;
        d.sat_id = ids.v[s % n_sats];
        const double off = (double)i * step;
        d.doppler_hz = lo + off;
        d.tap_index = -1;
        d.reserved = 0;
        cells[(int64_t)s * n_bins + i] = d;
    }
}

struct HybSelectParams {
    const gyp_hybrid_cell* recs;   // [n_states][n_bins] this level's records ...
    const gyp_cell_desc* cells;    // ... and cells
    int32_t n_states, n_bins;
    int32_t next_half;             // >= 0: write the next level's cells, best + j * next_step for j = -next_half .. next_half; < 0: this level is the last
    double next_step;
    gyp_cell_desc* next_cells;     // [n_states][2 next_half + 1], or the final cells [n_states] (tap at the code phase)
    gyp_weak_result* out;          // the last level only
};

__global__ __launch_bounds__(64) void hybrid_select_kernel(HybSelectParams p) {
#pragma clang fp contract(off)
    const int32_t s = (int32_t)blockIdx.x * 64 + (int32_t)threadIdx.x;
    if (s >= p.n_states) return;
    const gyp_hybrid_cell* row = p.recs + (int64_t)s * p.n_bins;
    int32_t best = 0;
    double best_z = hybrid_z(row[0].peak, row[0].n_off, row[0].sum_off, row[0].sumsq_off);
    for (int32_t i = 1; i < p.n_bins; ++i) {
        const double z = hybrid_z(row[i].peak, row[i].n_off, row[i].sum_off, row[i].sumsq_off);
        if (z > best_z || (best_z != best_z && z == z)) { best = i; best_z = z; }
    }
    const gyp_cell_desc bc = p.cells[(int64_t)s * p.n_bins + best];
    if (p.next_half >= 0) {
        const int32_t nb = 2 * p.next_half + 1;
        for (int32_t i = 0; i < nb; ++i) {
            gyp_cell_desc d = bc;
            const double off = (double)(i - p.next_half) * p.next_step;
            d.doppler_hz = bc.doppler_hz + off;
            p.next_cells[(int64_t)s * nb + i] = d;
        }
        return;
    }
    const gyp_hybrid_cell r = row[best];
    gyp_cell_desc d = bc;
    d.tap_index = r.argmax;
    p.next_cells[s] = d;
    gyp_weak_result o;
    o.stream = bc.stream;
    o.sat_id = bc.sat_id;
    o.doppler_hz = bc.doppler_hz;
    o.code_phase = r.argmax;
    o.reserved0 = 0;
    o.carrier_phase = 0.0;   // hybrid_finish_kernel
    o.z = best_z;
    o.peak_ratio = (double)r.peak / (double)r.second;
    o.set = r.set;
    o.reserved = 0;
    p.out[s] = o;
}

// carrier_phase = angle(C_0[code_phase]) from the tap of the final cell's block 0
__global__ __launch_bounds__(64) void hybrid_finish_kernel(const gyp_cell* __restrict__ taps, int32_t n_states, gyp_weak_result* __restrict__ out) {
    const int32_t s = (int32_t)blockIdx.x * 64 + (int32_t)threadIdx.x;
    if (s >= n_states) return;
    out[s].carrier_phase = atan2((double)taps[s].tap_im, (double)taps[s].tap_re);
}

}  // namespace gyp
