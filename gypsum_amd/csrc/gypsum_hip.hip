// gypsum_hip.hip -- C ABI of libgypsum_hip.so (see include/gypsum_hip.h).  gfx950 / ROCm only.
//
// Host side: context, PRN code generation (integer LFSRs), float64 construction of the per-satellite
// frequency-domain replicas and FFT twiddle tables, device buffers, kernel launches.
#include <hip/hip_runtime.h>

#include <cmath>
#include <complex>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <new>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/gypsum_hip.h"
#include "kernels.hpp"
#include "bit_integrator.hpp"
#include "grid_plan.hpp"
#include "track_plan.hpp"
#include "acq_plan.hpp"
#include "cond_plan.hpp"
#include "dev_mem.hpp"

using namespace gyp;

// ---------------------------------------------------------------------------------------------------------
// PRN codes (gps_ca_prn_codes.py:100-250): 10-stage G1/G2 registers as bit masks, stage i = bit i-1
// ---------------------------------------------------------------------------------------------------------
static const uint8_t kG2Taps[32][2] = {
    {2, 6}, {3, 7}, {4, 8}, {5, 9}, {1, 9}, {2, 10}, {1, 8}, {2, 9}, {3, 10}, {2, 3}, {3, 4}, {5, 6}, {6, 7}, {7, 8},
    {8, 9}, {9, 10}, {1, 4}, {2, 5}, {3, 6}, {4, 7}, {5, 8}, {6, 9}, {1, 3}, {4, 6}, {5, 7}, {6, 8}, {7, 9}, {8, 10},
    {1, 6}, {2, 7}, {3, 8}, {4, 9}};
static const uint16_t kFirstTenChipsOctal[32] = {
    01440, 01620, 01710, 01744, 01133, 01455, 01131, 01454, 01626, 01504, 01642, 01750, 01764, 01772, 01775, 01776,
    01156, 01467, 01633, 01715, 01746, 01763, 01063, 01706, 01743, 01761, 01770, 01774, 01127, 01453, 01625, 01712};

static inline unsigned stage(unsigned reg, int i) { return (reg >> (i - 1)) & 1u; }

static int make_prn_chips(uint8_t* out /*32*1023*/) {
    unsigned g1 = 0x3FF, g2 = 0x3FF;
    for (int c = 0; c < kChips; ++c) {
        const unsigned o1 = stage(g1, 10);
        for (int sv = 0; sv < 32; ++sv) out[sv * kChips + c] = (uint8_t)(o1 ^ stage(g2, kG2Taps[sv][0]) ^ stage(g2, kG2Taps[sv][1]));
        const unsigned fb1 = stage(g1, 3) ^ stage(g1, 10);
        const unsigned fb2 = stage(g2, 2) ^ stage(g2, 3) ^ stage(g2, 6) ^ stage(g2, 8) ^ stage(g2, 9) ^ stage(g2, 10);
        g1 = ((g1 << 1) & 0x3FF) | fb1;
        g2 = ((g2 << 1) & 0x3FF) | fb2;
    }
    for (int sv = 0; sv < 32; ++sv) {
        unsigned head = 0;
        for (int c = 0; c < 10; ++c) head = (head << 1) | out[sv * kChips + c];
        if (head != kFirstTenChipsOctal[sv]) return GYP_E_BAD_ARG;
    }
    return GYP_OK;
}

// ---------------------------------------------------------------------------------------------------------
// float64 host FFT (radix-2, in place) for the replica spectra
// ---------------------------------------------------------------------------------------------------------
typedef std::complex<double> cd;
static void host_fft(std::vector<cd>& a) {
    const size_t n = a.size();
    for (size_t i = 1, j = 0; i < n; ++i) {
        size_t bit = n >> 1;
        for (; j & bit; bit >>= 1) j ^= bit;
        j ^= bit;
        if (i < j) std::swap(a[i], a[j]);
    }
    for (size_t len = 2; len <= n; len <<= 1) {
        const double ang = -2.0 * M_PI / (double)len;
        for (size_t i = 0; i < n; i += len)
            for (size_t k = 0; k < len / 2; ++k) {
                const cd w(std::cos(ang * (double)k), std::sin(ang * (double)k));
                const cd u = a[i + k], v = a[i + k + len / 2] * w;
                a[i + k] = u + v;
                a[i + k + len / 2] = u - v;
            }
    }
}

// conj(FFT2048(periodic +-1 code)) / 2048 in the kernel's [physical reg][lane] layout:
// physical register i of lane (h, l) holds bin f = 2*(l + 32*bitrev5(i)) + h.
static void make_replica_lane_layout(const uint8_t* chips, float* out /*32*64*2*/) {
    std::vector<cd> pp(2048, cd(0.0, 0.0));
    for (int m = 0; m < kChips; ++m) pp[m] = chips[m] ? 1.0 : -1.0;
    for (int j = 1; j < kChips; ++j) pp[2048 - j] = chips[kChips - j] ? 1.0 : -1.0;
    host_fft(pp);
    for (int i = 0; i < 32; ++i)
        for (int lane = 0; lane < 64; ++lane) {
            const int l = lane & 31, h = lane >> 5;
            const int f = 2 * (l + 32 * bitrev5(i)) + h;
            const cd v = std::conj(pp[f]) / 2048.0;
            out[(i * 64 + lane) * 2 + 0] = (float)v.real();
            out[(i * 64 + lane) * 2 + 1] = (float)v.imag();
        }
}

// ---------------------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------------------
// samples per chip (multiples of 1.023 MHz) the kernels are instantiated for
#ifndef GYP_FOR_EACH_RATE   // a development build may pass a shorter list (-D'GYP_FOR_EACH_RATE(X)=X(2) X(8)'): fewer instantiations
#define GYP_FOR_EACH_RATE(X) X(1) X(2) X(3) X(4) X(5) X(6) X(8) X(10) X(12) X(16) X(20) X(48)
#endif
static bool rate_supported(int k) {
    switch (k) {
#define X(K) case K:
        GYP_FOR_EACH_RATE(X)
#undef X
        return true;
    }
    return false;
}

static thread_local std::string g_create_error;

// Device buffers of the entry points on a context, one per role.  Each is reserved (Slack::grow) and used within one call, on the
// context's stream; nothing is kept in them between calls.  A helper context (gyp_acquire_dev) has a set of its own.
// Staging of the host-buffer entry points; only the wrappers that take host pointers use these, never a *_dev function (the wrappers
// that upload samples alone and return one array go through staged_call):
//   stage_iq       samples: gyp_correlate_cells, gyp_correlate_grid, gyp_search_level, gyp_acquire, gyp_track_step, gyp_track_block, gyp_weak_track_block
//   stage_in       descriptors: gyp_correlate_cells (gyp_cell_desc), gyp_track_step (gyp_chan_in)
//   stage_out      results: gyp_correlate_cells, gyp_correlate_grid (gyp_cell), gyp_search_level, gyp_acquire (gyp_acq_result), gyp_track_step (gyp_chan_out), gyp_track_block (gyp_track_rec)
//   weak_stage     results: gyp_weak_track_block (the call's millisecond records, period records and period counts, back to back; its
//                  samples go through stage_iq like every host form's)
//   stage_profile  optional profile rows: gyp_correlate_cells, gyp_track_step
//   stage_times    start times: gyp_track_step (per stream), gyp_track_block (per millisecond)
//   quality_recs, quality_sums   tracking records in, sums out: gyp_track_quality (roles of its own: its input is the kind of record
//                  stage_out holds for gyp_track_block)
// Working buffers of the *_dev functions; no wrapper uses these:
//   sat_ids, doppler          satellite ids and Doppler bins: gyp_correlate_grid_dev, gyp_grid_best_bins_refined_dev
//   folded, z, grid_partial   gyp_correlate_grid_dev: folded rows, the wide rates' wiped-off samples, partial results of branch runs
//   refine_list               gyp_grid_best_bins_refined_dev (refine_list_layout)
//   partial64                 float64 per-millisecond sums: gyp_grid_best_bins_refined_dev, acquire_search
//   acq_*                     acquire_search (gyp_acquire_dev, gyp_search_level_dev), sized by its AcqPlan and reserved in acq_reserve: search states, cell table, cell outputs, refined sums, float64 profiles, acq_book_layout, acq_units_layout, shared-forward spectra
//   synth_scene, bench_sink   gyp_synth_iq_dev, gyp_debug_fft_bench
//   hyb_sat_ids, hyb_doppler, hyb_grid_cells   gyp_correlate_grid_hybrid_dev: satellite ids, Doppler bins and the cell table made of them
//   hyb_cell_out, hyb_profile, hyb_power   hybrid_run (behind both hybrid entry points), sized by its HybPlan and reserved in hybrid_reserve
//                             alone: per chunk of cells the gyp_cell records the cells kernel must write somewhere, a block's coherent
//                             profiles, the sets' power rows
//   hyb_level_cells, hyb_records, hyb_taps   gyp_acquire_weak_dev, sized by its WeakSearchPlan: the cell tables of the coarse level, the
//                             fine level and the final cells (back to back), the larger level's records (weak_level), the final
//                             cells' gyp_cell records (their taps)
//   wref_cands, wref_plans, wref_prompts, wref_power   gyp_weak_refine_dev: the candidates' start-up states, one WeakMsPlan per (candidate,
//                             millisecond), the prompts when the caller takes none, the power rows of the periodograms
//   wmeas_cands, wmeas_states, wmeas_plans, wmeas_sums, wmeas_w   gyp_weak_measure_dev: the candidates' start-up states, what each carries
//                             from pass to pass (c0, the corrections' sum, the status), one WeakMsPlan per (candidate, millisecond),
//                             and one pass's sums and W_m when the caller takes none
// Members with more than one user, and why no call path holds two of them: the stage_* members serve one wrapper at a time and no
// wrapper calls another (the hybrid wrappers gyp_correlate_grid_hybrid and gyp_acquire_weak use stage_iq and stage_out like the
// others); of gyp_correlate_grid_dev, gyp_grid_best_bins_refined_dev (sat_ids, doppler) and acquire_search (partial64)
// none calls another, and what acquire_search calls (launch_cells, launch_cells_shared, gyp_correlate_cells_dev) uses no member.
// hybrid_run serves one of gyp_correlate_grid_hybrid_dev and gyp_acquire_weak_dev at a time, neither calls the other, and its
// launch_cells uses no member; the hyb_* members have no user outside the hybrid entry points.  The wref_* members have no user but
// gyp_weak_refine_dev, which calls no entry point; its wrapper gyp_weak_refine stages through stage_iq and stage_out (the records, then
// the prompts, back to back) like the others.  The wmeas_* members have no user but gyp_weak_measure_dev, which calls no entry point;
// its wrapper gyp_weak_measure goes through staged_call (the records, then the sums, the W_m and the folds it was asked for, back to back).
struct Scratch {
    DevBuf<int32_t> hyb_sat_ids;
    DevBuf<double> hyb_doppler;
    DevBuf<gyp_cell_desc> hyb_grid_cells, hyb_level_cells;
    DevBuf<gyp_cell> hyb_cell_out, hyb_taps;
    DevBuf<cf> hyb_profile;
    DevBuf<float> hyb_power;
    DevBuf<gyp_hybrid_cell> hyb_records;
    DevBuf<WeakRefineCand> wref_cands;
    DevBuf<WeakMsPlan> wref_plans;
    DevBuf<float2> wref_prompts;
    DevBuf<double> wref_power;
    DevBuf<WeakMeasureCand> wmeas_cands;
    DevBuf<WeakMeasureState> wmeas_states;
    DevBuf<WeakMsPlan> wmeas_plans;
    DevBuf<gyp_weak_ms_rec> wmeas_sums;
    DevBuf<double> wmeas_w;
    DevBuf<float> stage_iq, stage_profile, bench_sink;
    DevBuf<uint8_t> stage_in, stage_out, weak_stage, refine_list, acq_book, acq_units;
    DevBuf<double> stage_times, doppler, partial64, acq_refined, acq_profiles;
    DevBuf<int32_t> sat_ids;
    DevBuf<cf> folded, z, acq_spectra;
    DevBuf<GridPartial> grid_partial;
    DevBuf<AcqSearchState> acq_states;
    DevBuf<gyp_cell_desc> acq_cells;
    DevBuf<gyp_cell> acq_out;
    DevBuf<gyp_synth_sat> synth_scene;
    DevBuf<gyp_track_rec> quality_recs;
    DevBuf<gyp_quality_sums> quality_sums;
};

// The tables of the 32 C/A codes on the device (gyp_set_stream_format builds them whole, or not at all)
struct CodeBufs {
    DevBuf<cf> replicas, tw;    // [32][32][64]; tw1024[1024] ++ tw2048[1024] ++ ones[1024]
    DevBuf<uint8_t> chips;      // [32][1023]: synthetic generator, float64 tie-breaks
    DevBuf<uint16_t> ones, trans;   // [32][512]: positions of each code's 512 ones (float64 strength tie-break); [32][kMaxTrans]: chip transitions (float64 early/late boundary sums)
    DevBuf<int32_t> ntrans;     // [32]
    DevBuf<float> chipf;        // [32][2048]: +-1.0f codes, twice over (window correlations of the speculative tracker)
};

struct gyp_ctx {
    int device = 0;
    Stream own_stream;         // (declared before everything used on it: destroyed last)
    hipStream_t stream = nullptr;
    Event ev0, ev1;
    int n_cus = 256;
    int n_xcd = 8;             // hipDeviceAttributeNumberOfXccs (workgroup b is dispatched to XCD b % n_xcd)
    // A/B switches and test hooks: gyp_debug_set / gyp_debug_get by the names in kDebugSwitches below
    bool no_pipe = false;      // A/B switch back to the two-workgroups-per-CU cells kernel
    int widen_wg_per_cu = 2;      // workgroups per CU of the persistent grid of the kernels on the upload stream (1..8; cond_plan.hpp: persistent_cap)
    int resample_tile = 4096;     // "resample_tile_samples": LDS budget of one resample_kernel tile, in input samples (32 KiB: five
                                  // workgroups per CU); same output for any value
    std::vector<std::pair<ResampleDesign, DevBuf<float>>> resample_designs;   // gyp_resample_iq_dev / gyp_ingest_open_resampled: one per (fs_in, fs_out, taps), with the owner of its d_taps
    std::vector<std::pair<PackedLevels, DevBuf<float>>> packed_levels;   // packed recordings: each level table met, in device memory
    bool notch_no_lds = false;    // A/B switch: iq_notch_kernel keeps the residual in the output buffer at every rate (same bits)
    DevBuf<int64_t> tone_freqs;   // gyp_iq_tones_dev: the call's frequencies (f mod fs) in device memory
    int track_chunk_ms = 250;     // the throughput tracking kernel's launch length (0: whole blocks; r03-r05: 500)
    float symbol_tau = 1e-4f;     // |Re peak| / |peak| below which the pseudosymbol is decided in float64 (test hook: 10 = always)
    bool no_shared_fwd = false;   // A/B switch: flat grids transform every cell's rows themselves again
    bool no_acq_shared_fwd = false;   // A/B switch: acquisition levels transform every cell's rows themselves again
    int cells_cu_reserve = 0;     // CUs the correlation-cell launches leave free (see launch_cells)
    int last_grid_refined_rows = 0;   // gyp_debug_get("last_grid_refined_rows"): rows the last gyp_grid_best_bins_refined_dev call decided in float64
    DevBuf<int32_t> acq_witness;        // [kAcqWitnessInts] gyp_debug_get("last_acq_units" / "last_acq_shared_cells" / "last_acq_unshared_cells", and "..._l<k>" per level): what the levels of
                                        // the last search on this context did (acq_init_kernel zeroes, the compact kernels add; read on request only)
    AcqPlan last_acq_plan{};            // of that search (a split scan's: the whole scan's); gyp_debug_get("last_acq_levels" / "last_acq_shared_levels" / "last_acq_lanes") read it.  lanes: the
                                        // parts it actually went through in -- this context and the first lanes - 1 helpers (0 none yet)
    GridPlan last_grid_plan{};    // of the last gyp_correlate_grid* call; gyp_debug_get("last_grid_path") reads its path (1 fused, 2 shared forward, 3 one wavefront per cell, 4 workgroup per cell)
    int grid_fused_waves = 12;    // 12 (default) or 8 wavefronts per workgroup of the fused flat-grid kernel (A/B)
    bool no_grid_fused = false;   // A/B switch: flat grids go through grid_fold_kernel + folded rows in HBM (r05) instead of the fused kernel
    bool no_grid_parts = false;   // A/B switch: flat-grid work items take whole units (no branch runs + merge)
    int hybrid_scratch_mb = kHybScratchMbDefault;   // "hybrid_scratch_mb": budget of hybrid_run's profile + power scratch (same records for any value)
    HybPlan last_hybrid_plan{};   // of the last hybrid_run; gyp_debug_get("last_hybrid_chunks") reads its n_chunks
    std::string err;
    // stream format
    int64_t fs = 0;
    int32_t n = 0;
    int k = 0;
    CodeBufs codes;
    // RCCL communicator (gyp_comm_init); the library is dlopen'ed on first use, libgypsum_hip does not link against it
    void* comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    gyp_params params;
    int spec_sub_ms = 0;         // target length of a speculative block's sub-blocks (a failed verification costs one); 0 = by rate (spec_sub_ms_for, track_plan.hpp)
    bool spec_redo = true;       // 0 = A/B switch back to re-running a failed speculation on the throughput kernel
    int prof_wave = 0;           // which wavefront of workgroup 0 stamps gyp_debug_track_profile's counters
    bool no_exact_shared = false;   // A/B switch: the throughput path's exact sums fetch and convert the samples per channel again (dll_exact_wave_kernel)
    int last_exact_path = 0;     // gyp_debug_get("last_exact_path"): the exact-sums kernel of the last plain throughput call (0 none yet, 1 dll_exact_wave_kernel, 2 dll_exact_shared_kernel, 3 dll_exact_block_kernel)
    TrackPlan last_track_plan{};   // of the last gyp_track_block_dev call; gyp_debug_get("last_track_flow") reads its flow (0 none yet, 1 throughput kernel, 2 speculative with the re-run at the end, 3 round protocol)
    bool no_spec = false;        // A/B switch: lightly loaded banks use the throughput kernel too
    bool track_finish_all = false;   // A/B switch: every wavefront of the throughput tracking kernel merges the millisecond's profile again (same bits)
    int spec_fail_at = -1;       // (test hook): channel 0's verification is made to fail at that millisecond of a block
    bool spec_debug = false;     // per-ms window dump of the speculative tracker (gyp_debug_spec_read)
    double dll_prov_bias = 0.0;  // (test hook): added to the speculative kernel's PROVISIONAL discriminator, so
                                 // that dll_scan_kernel's repair path runs; results must not depend on it
    DevBuf<long long> prof;      // gyp_debug_track_profile: per-phase cycle counters of track_block workgroup 0
    Event ev_order;              // gyp_wait_for(waiter, this): recorded on this context's stream
    gyp_ctx* helper[kMaxAcqLanes - 1] = {};   // gyp_acquire_dev: the other parts of a multi-stream scan run here (own stream, scratch, tables)
    int acq_lanes = 2;
    bool is_helper = false;
    bool no_acq_split = false;       // A/B switch
    // gyp_debug_track_timing: HIP events around the three launches of the throughput tracking path (tracking kernel, exact sums, scan)
    bool time_track = false;
    bool track_timed = false;   // the events below have been recorded since timing was switched on (the speculative path records none)
    int track_launches = 0;     // launches of the tracking kernel behind the last timed call
    Event ev_track[4];
    Scratch scratch;
};

// Every switch of gyp_debug_set / gyp_debug_get: name, range, integral or not, whether the helper contexts of a multi-stream scan run
// under the caller's value (acquire_helper), getter, setter.  The read-only "last_*" values are in debug_read_only.
struct DebugSwitch { const char* name; double lo, hi; bool integral, inherited; double (*get)(const gyp_ctx&); void (*set)(gyp_ctx&, double); };
#define GYP_SWITCH(NAME, FIELD, LO, HI, INTEGRAL, INHERITED) \
    {NAME, LO, HI, INTEGRAL, INHERITED, [](const gyp_ctx& c) { return (double)c.FIELD; }, [](gyp_ctx& c, double v) { c.FIELD = static_cast<decltype(c.FIELD)>(v); }}
static const DebugSwitch kDebugSwitches[] = {
    GYP_SWITCH("no_pipe", no_pipe, 0, 1, true, true),
    GYP_SWITCH("no_shared_fwd", no_shared_fwd, 0, 1, true, true),
    GYP_SWITCH("no_acq_shared_fwd", no_acq_shared_fwd, 0, 1, true, true),
    GYP_SWITCH("no_acq_split", no_acq_split, 0, 1, true, false),
    GYP_SWITCH("no_spec", no_spec, 0, 1, true, true),
    GYP_SWITCH("spec_debug", spec_debug, 0, 1, true, false),
    GYP_SWITCH("acq_lanes", acq_lanes, 1, kMaxAcqLanes, true, false),
    GYP_SWITCH("track_chunk_ms", track_chunk_ms, 0, 1e6, true, true),   // (and not 1..19: gyp_debug_set)
    GYP_SWITCH("widen_wg_per_cu", widen_wg_per_cu, 1, 8, true, false),
    GYP_SWITCH("symbol_tau", symbol_tau, 0, 100, false, true),
    GYP_SWITCH("dll_prov_bias", dll_prov_bias, -1e6, 1e6, false, false),
    GYP_SWITCH("spec_fail_at", spec_fail_at, -1, 2147483647.0, true, false),
    GYP_SWITCH("spec_redo", spec_redo, 0, 1, true, false),
    GYP_SWITCH("spec_sub_ms", spec_sub_ms, 0, 2000, true, false),
    GYP_SWITCH("no_exact_shared", no_exact_shared, 0, 1, true, false),
    GYP_SWITCH("prof_wave", prof_wave, 0, 7, true, false),
    GYP_SWITCH("no_grid_parts", no_grid_parts, 0, 1, true, false),
    GYP_SWITCH("no_grid_fused", no_grid_fused, 0, 1, true, false),
    GYP_SWITCH("grid_fused_waves", grid_fused_waves, 8, 12, true, false),   // (8 or 12: gyp_debug_set)
    GYP_SWITCH("cells_cu_reserve", cells_cu_reserve, 0, 128, true, true),
    GYP_SWITCH("resample_tile_samples", resample_tile, 1024, 8192, true, false),
    GYP_SWITCH("notch_no_lds", notch_no_lds, 0, 1, true, false),
    GYP_SWITCH("track_finish_all", track_finish_all, 0, 1, true, true),
    GYP_SWITCH("hybrid_scratch_mb", hybrid_scratch_mb, kHybScratchMbMin, kHybScratchMbMax, true, false),
};
#undef GYP_SWITCH

// What the 1-ms bank and the weak bank share on the host (bank_create, bank_put_state, bank_covers below); each has its `states` besides.
struct BankBase {
    gyp_ctx* ctx = nullptr;
    int n_chan = 0;
    int64_t fs = 0;              // the stream format the bank was created under
    int n = 0;
    std::vector<int32_t> stream_of;   // host copy of each channel's stream index
};
struct gyp_bank : BankBase {
    Stream verify_stream;       // (declared before everything used on it: destroyed last)
    Event ev_spec, ev_verify, ev_vring[3];
    DevBuf<ChanState> states;
    // speculative block tracking: state checkpoint, per-(channel, ms) hand-over records, failed-verification flags
    DevBuf<ChanState> ckpt;      // [sub-blocks][n_chan]: as many sub-blocks as the longest layout so far (18 KB per channel and sub-block)
    DevBuf<SpecIn> spec;         // [n_chan][n_ms]
    DevBuf<double> disc;         // [n_chan][n_ms] exact discriminators from the verify pass (dll_scan_kernel's input)
    DevBuf<DllExact> dllx;       // [n_chan] the exactly re-integrated code loop between sub-blocks
    DevBuf<ExactGroup> groups;   // [n_chan] + one int32 counter behind them: dll_exact_shared_kernel's channel groups (exact_group_kernel, every call)
    int last_n_ms = 0;           // row length of spec / disc in the last throughput call (gyp_debug_disc_read)
    DevBuf<int32_t> bad, bad_from;   // per channel: verification failed; the first verify sub-block that failed
    DevBuf<DllExact> hist;       // [sub-blocks + 1][n_chan] the exact code loop at the sub-block starts
    // round protocol of the speculative tracker (SpecCtl, kernels_track_block.hpp)
    DevBuf<SpecCtl> ctl;         // [n_chan]
    DevBuf<int32_t> trk, fail;   // [rounds][n_chan]
    DevBuf<int32_t> redo_stats;  // [4] of the last block: sub-blocks, rounds, sub-block re-dos, channels finished by the transform kernel
    DevBuf<float> dbg;           // GYP_SPEC_DEBUG: per-ms window dump of the last block
    // gyp_bank_keep_profiles: the last call's trailing prompt profiles (tracker.py:154,308-309)
    DevBuf<float> prof_tail;     // [n_chan][prof_depth][n]
    DevBuf<int32_t> prof_delta;  // [n_chan][prof_depth] exact - provisional code phase (repaired milliseconds only)
    int prof_depth = 0;
    int prof_rows = 0;               // rows valid after the last gyp_track_block(_dev)
};

// RCCL, resolved at run time (see the multi-GPU section of the C ABI below)
namespace {
struct RcclId { char b[128]; };   // ncclUniqueId, passed by value
struct RcclApi {
    typedef RcclId Id;
    void* lib = nullptr;
    int (*GetUniqueId)(void*) = nullptr;
    int (*CommInitRank)(void**, int, RcclId, int) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    std::string err;
};
RcclApi g_rccl;
bool rccl_load() {
    if (g_rccl.lib) return true;
    const char* names[] = {"librccl.so", "librccl.so.1"};
    void* h = nullptr;
    // First choice: the librccl that sits next to the HIP runtime THIS library is bound to.  A process may hold two ROCm
    // stacks (PyTorch ships its own libamdhip64 / libhsa-runtime64 / librccl): an RCCL from the other stack talks to an
    // HSA runtime nobody initialised (ncclCommInitRank: "no ROCm-capable device is detected").
    Dl_info info;
    // GYP_RCCL_LIB=<path or soname>: use exactly this library (a deployment with its own RCCL build); nothing else is tried
    const char* forced = std::getenv("GYP_RCCL_LIB");
    if (forced && *forced) {
        h = dlopen(forced, RTLD_NOW | RTLD_GLOBAL);
        if (!h) {
            const char* why = dlerror();
            g_rccl.err = std::string("librccl not found: GYP_RCCL_LIB=") + forced + ": " + (why ? why : "no loader message");
            return false;
        }
    } else if (dladdr(reinterpret_cast<void*>(&hipStreamSynchronize), &info) && info.dli_fname) {
        std::string dir(info.dli_fname);
        const size_t slash = dir.rfind('/');
        if (slash != std::string::npos) {
            dir.resize(slash + 1);
            for (const char* n : {"librccl.so.1", "librccl.so"}) if (!h) h = dlopen((dir + n).c_str(), RTLD_NOW | RTLD_GLOBAL);
        }
    }
    for (const char* n : names) if (!h) h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);      // else a copy already in the process, if any
    for (const char* n : {"librccl.so.1", "librccl.so"}) if (!h) h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
        const char* why = dlerror();   // (one call: dlerror() clears the message it returns)
        g_rccl.err = std::string("librccl not found: ") + (why ? why : "no loader message");
        return false;
    }
    g_rccl.GetUniqueId = reinterpret_cast<decltype(g_rccl.GetUniqueId)>(dlsym(h, "ncclGetUniqueId"));
    g_rccl.CommInitRank = reinterpret_cast<decltype(g_rccl.CommInitRank)>(dlsym(h, "ncclCommInitRank"));
    g_rccl.AllGather = reinterpret_cast<decltype(g_rccl.AllGather)>(dlsym(h, "ncclAllGather"));
    g_rccl.CommDestroy = reinterpret_cast<decltype(g_rccl.CommDestroy)>(dlsym(h, "ncclCommDestroy"));
    g_rccl.GetErrorString = reinterpret_cast<decltype(g_rccl.GetErrorString)>(dlsym(h, "ncclGetErrorString"));
    if (!g_rccl.GetUniqueId || !g_rccl.CommInitRank || !g_rccl.AllGather || !g_rccl.CommDestroy) {
        g_rccl.err = "librccl lacks ncclGetUniqueId / ncclCommInitRank / ncclAllGather / ncclCommDestroy";
        return false;
    }
    g_rccl.lib = h;
    return true;
}
std::string rccl_msg(const char* what, int rc) {
    return std::string(what) + ": " + (g_rccl.GetErrorString ? g_rccl.GetErrorString(rc) : "RCCL error") + " (" + std::to_string(rc) + ")";
}
}  // namespace

static int fail(gyp_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    else g_create_error = msg;
    return code;
}
static int refuse(gyp_ctx* ctx, const char* who, const std::string& why) { return fail(ctx, GYP_E_BAD_ARG, std::string(who) + ": " + why); }
#define HIP_TRY(ctx, call)                                                                                   \
    do {                                                                                                     \
        hipError_t e_ = (call);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return fail(ctx, GYP_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_));                  \
    } while (0)

static const char* const kNoFormat = "gyp_set_stream_format has not been called";
static int need_format(gyp_ctx* ctx) { return ctx->k ? GYP_OK : fail(ctx, GYP_E_NO_FORMAT, kNoFormat); }
static int check_sat_ids(gyp_ctx* ctx, const int32_t* ids, int n) {
    for (int i = 0; i < n; ++i) if (ids[i] < 1 || ids[i] > 32) return fail(ctx, GYP_E_BAD_ARG, "satellite id out of range");
    return GYP_OK;
}
// n_streams * n_ms milliseconds of complex64 samples, in floats
static size_t iq_floats(const gyp_ctx* ctx, int64_t n_streams, int64_t n_ms) { return (size_t)n_streams * n_ms * ctx->n * 2; }
static const uint8_t* as_bytes(const void* p) { return static_cast<const uint8_t*>(p); }
// The tail of a host-buffer entry point: the staged results (and profile rows) copied back; returns when they have arrived.
static int stage_back(gyp_ctx* ctx, void* out_host, size_t out_bytes, float* profile_host = nullptr, size_t n_prof = 0) {
    if (out_host) HIP_TRY(ctx, hipMemcpyAsync(out_host, ctx->scratch.stage_out.get(), out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (profile_host) HIP_TRY(ctx, hipMemcpyAsync(profile_host, ctx->scratch.stage_profile.get(), n_prof * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GYP_OK;
}
// A host form that uploads only samples and returns one array: the results' staging reserved, the samples uploaded,
// `call(iq_dev, stream_stride_samples, out_dev)` -- the _dev form -- and the results copied back.  The wrapper's own checks come first.
template <typename F>
static int staged_call(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, int32_t n_ms, void* out_host, size_t out_bytes, F&& call) {
    Scratch& sc = ctx->scratch;
    HIP_TRY(ctx, sc.stage_out.reserve(out_bytes, Slack::grow, ctx->stream));
    HIP_TRY(ctx, upload(sc.stage_iq, iq_host, iq_floats(ctx, n_streams, n_ms), ctx->stream));
    if (const int rc = call(sc.stage_iq.get(), (int64_t)n_ms * ctx->n, sc.stage_out.get())) return rc;
    return stage_back(ctx, out_host, out_bytes);
}
// A bank (gyp_bank, gyp_weak_bank) from its validated host states: made, its base filled, the states reserved, `rest(bank)` for what
// the kind has besides, the states copied; deleted again if any of that fails.
template <class Bank, class State, class F>
static int bank_create(gyp_ctx* ctx, const char* who, const std::vector<State>& init, Bank** out, F&& rest) {
    Bank* b = new Bank();
    b->ctx = ctx; b->n_chan = (int)init.size(); b->fs = ctx->fs; b->n = ctx->n;
    for (const State& s : init) b->stream_of.push_back(s.stream);
    hipError_t e = b->states.reserve(init.size(), Slack::exact);
    if (e == hipSuccess) e = rest(*b);
    if (e == hipSuccess) e = hipMemcpy(b->states.get(), init.data(), init.size() * sizeof(State), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        delete b;
        return fail(ctx, GYP_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
    }
    *out = b;
    return GYP_OK;
}
// One channel's state put into a bank, behind everything enqueued on the context's stream
template <class Bank, class State>
static int bank_put_state(Bank* bank, int32_t index, const State& s) {
    gyp_ctx* ctx = bank->ctx;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(bank->states.get() + index, &s, sizeof(State), hipMemcpyHostToDevice));
    bank->stream_of[index] = s.stream;
    return GYP_OK;
}
// The host forms of block tracking: every channel's stream is among the n_streams passed
static int bank_covers(const BankBase& bank, const char* who, int32_t n_streams) {
    for (int c = 0; c < bank.n_chan; ++c)
        if (bank.stream_of[c] >= n_streams)
            return refuse(bank.ctx, who, "channel " + std::to_string(c) + " reads stream " + std::to_string(bank.stream_of[c]) + " but only " +
                                             std::to_string(n_streams) + " were passed");
    return GYP_OK;
}
// A channel's state at the start of tracking: the acquisition's values, fresh loop state and histories
static ChanState fresh_chan_state(const gyp_chan_init& in) {
    ChanState s;
    std::memset(&s, 0, sizeof(s));
    s.stream = in.stream; s.sat_id = in.sat_id; s.doppler = in.doppler_hz; s.carrier_phase = in.carrier_phase;
    s.code_phase = in.code_phase; s.dll_phase = (double)in.code_phase;  // tracker.py:224
    return s;
}

extern "C" {

int gyp_version(void) { return GYP_VERSION; }

void gyp_params_default(gyp_params* p) {
    if (!p) return;
    p->acq_initial_spread_hz = 7000.0; p->acq_min_spread_hz = 10.0; p->acq_bins_per_spread = 10.0;
    p->dll_gain = 0.002; p->dll_phase_modulus = 2046.0;
    p->pll_bandwidth_locked_hz = 3.0; p->pll_bandwidth_unlocked_hz = 6.0;
    p->lock_error_variance_max = 900.0; p->lock_i_variance_max = 2.0; p->lock_rotation_max_deg = 6.0;
    p->watchdog_period_s = 6.0; p->watchdog_drop_below = 0.2; p->watchdog_nudge_below = 0.93; p->watchdog_nudge_hz = 5.0;
    p->spec_confidence_kappa = 20.0;
    p->acq_reuse_level_records = 1.0;
}

int gyp_set_params(gyp_ctx* ctx, const gyp_params* p) {
    if (!ctx || !p) return GYP_E_BAD_ARG;
    if (!(p->acq_initial_spread_hz > 0) || !(p->acq_min_spread_hz > 0) || !(p->acq_bins_per_spread >= 1) || !(p->dll_phase_modulus > 0) ||
        !(p->pll_bandwidth_locked_hz > 0) || !(p->pll_bandwidth_unlocked_hz > 0) || !(p->lock_error_variance_max > 0) ||
        !(p->lock_i_variance_max > 0) || !(p->lock_rotation_max_deg > 0 && p->lock_rotation_max_deg < 90) || !(p->watchdog_period_s > 0) ||
        !(p->spec_confidence_kappa >= 0) || !std::isfinite(p->dll_gain) ||
        !(p->acq_reuse_level_records == 0.0 || p->acq_reuse_level_records == 1.0))
        return fail(ctx, GYP_E_BAD_ARG, "gyp_set_params: value out of range");
    for (double s = p->acq_initial_spread_hz; s >= p->acq_min_spread_hz; s /= 2.0) {   // every level must fit the cell table
        const int step = (int)(s / p->acq_bins_per_spread);
        if (step < 1) return fail(ctx, GYP_E_BAD_ARG, "gyp_set_params: a search level would have a zero Doppler step");
        // centres are integers (0, then a bin of the level above): int(c + s) - int(c - s) <= floor(2 s) + 1
        const int span = (int)std::floor(2.0 * s) + 1;
        if ((span + step - 1) / step > kMaxBins) return fail(ctx, GYP_E_BAD_ARG, "gyp_set_params: a search level would exceed 28 Doppler bins");
    }
    ctx->params = *p;
    return GYP_OK;
}

int gyp_get_params(gyp_ctx* ctx, gyp_params* out) {
    if (!ctx || !out) return GYP_E_BAD_ARG;
    *out = ctx->params;
    return GYP_OK;
}

const char* gyp_last_error(const gyp_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int gyp_create(int device_ordinal, gyp_ctx** out) {
    if (!out) return fail(nullptr, GYP_E_BAD_ARG, "gyp_create: out is NULL");
    *out = nullptr;
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0)
        return fail(nullptr, GYP_E_NO_DEVICE, std::string("no HIP device available (") + hipGetErrorString(e) +
                                                  "); libgypsum_hip has no CPU fallback");
    if (device_ordinal < 0 || device_ordinal >= n_dev) return fail(nullptr, GYP_E_BAD_ARG, "device ordinal out of range");
    HIP_TRY(nullptr, hipSetDevice(device_ordinal));
    hipDeviceProp_t prop;
    HIP_TRY(nullptr, hipGetDeviceProperties(&prop, device_ordinal));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, GYP_E_NO_DEVICE, std::string("libgypsum_hip is built for gfx950 only, found ") + prop.gcnArchName);
    gyp_ctx* ctx = new gyp_ctx();
    ctx->device = device_ordinal;
    ctx->n_cus = prop.multiProcessorCount;
    {
        int xccs = 0;
        if (hipDeviceGetAttribute(&xccs, hipDeviceAttributeNumberOfXccs, device_ordinal) == hipSuccess && xccs > 0) ctx->n_xcd = xccs;
    }
    // (no GYP_* environment variable is read here or anywhere else in the library except GYP_RCCL_LIB, a deployment's library path:
    // the A/B switches and test hooks below are set through gyp_debug_set by whoever wants them)
    gyp_params_default(&ctx->params);
    if (ctx->own_stream.create(hipStreamNonBlocking) != hipSuccess || ctx->ev0.create(hipEventDefault) != hipSuccess || ctx->ev1.create(hipEventDefault) != hipSuccess) {
        delete ctx;
        return fail(nullptr, GYP_E_HIP, "stream/event creation failed");
    }
    ctx->stream = ctx->own_stream.get();
    if (ctx->acq_witness.reserve(kAcqWitnessInts, Slack::exact) != hipSuccess || hipMemset(ctx->acq_witness.get(), 0, kAcqWitnessInts * sizeof(int32_t)) != hipSuccess) {
        gyp_destroy(ctx);
        return fail(nullptr, GYP_E_HIP, "gyp_create: no device memory for the acquisition counters");
    }
    *out = ctx;
    return GYP_OK;
}

void gyp_destroy(gyp_ctx* ctx) {
    if (!ctx) return;
    for (auto& h : ctx->helper) if (h) { gyp_destroy(h); h = nullptr; }
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(ctx->comm);
    delete ctx;   // the members release what they hold: buffers and events first, the stream last
}

int gyp_device_name(gyp_ctx* ctx, char* out, int cap) {
    if (!ctx || !out || cap <= 0) return GYP_E_BAD_ARG;
    hipDeviceProp_t prop;
    HIP_TRY(ctx, hipGetDeviceProperties(&prop, ctx->device));
    std::snprintf(out, (size_t)cap, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return GYP_OK;
}

int gyp_set_stream(gyp_ctx* ctx, void* hip_stream) {
    if (!ctx) return GYP_E_BAD_ARG;
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream.get();
    return GYP_OK;
}

int gyp_sync(gyp_ctx* ctx) {
    if (!ctx) return GYP_E_BAD_ARG;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GYP_OK;
}

int gyp_wait_for(gyp_ctx* ctx, gyp_ctx* other) {
    if (!ctx || !other) return GYP_E_BAD_ARG;
    if (ctx == other) return GYP_OK;
    HIP_TRY(ctx, other->ev_order.create(hipEventDisableTiming));
    HIP_TRY(ctx, hipEventRecord(other->ev_order.get(), other->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, other->ev_order.get(), 0));
    return GYP_OK;
}

int gyp_timer_start(gyp_ctx* ctx) {
    if (!ctx) return GYP_E_BAD_ARG;
    HIP_TRY(ctx, hipEventRecord(ctx->ev0.get(), ctx->stream));
    return GYP_OK;
}

int gyp_timer_stop(gyp_ctx* ctx, float* elapsed_ms) {
    if (!ctx || !elapsed_ms) return GYP_E_BAD_ARG;
    HIP_TRY(ctx, hipEventRecord(ctx->ev1.get(), ctx->stream));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev1.get()));
    HIP_TRY(ctx, hipEventElapsedTime(elapsed_ms, ctx->ev0.get(), ctx->ev1.get()));
    return GYP_OK;
}

int gyp_prn_chips(uint8_t* out_32x1023) {
    if (!out_32x1023) return GYP_E_BAD_ARG;
    return make_prn_chips(out_32x1023);
}

int gyp_prn_spectrum_lane_layout(int sat_id, float* out_32x64x2) {
    if (sat_id < 1 || sat_id > 32 || !out_32x64x2) return GYP_E_BAD_ARG;
    std::vector<uint8_t> chips(32 * kChips);
    const int rc = make_prn_chips(chips.data());
    if (rc != GYP_OK) return rc;
    make_replica_lane_layout(chips.data() + (sat_id - 1) * kChips, out_32x64x2);
    return GYP_OK;
}

int gyp_set_stream_format(gyp_ctx* ctx, int64_t fs_hz, int32_t samples_per_ms) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (fs_hz <= 0 || samples_per_ms <= 0 || fs_hz / 1000 != samples_per_ms || fs_hz % 1000 != 0)
        return fail(ctx, GYP_E_BAD_RATE, "samples_per_ms must equal fs_hz / 1000");
    if (samples_per_ms % kChips != 0)
        return fail(ctx, GYP_E_BAD_RATE, "sample rate must be an integer multiple of 1.023 MHz (the replica is np.repeat(chips, N // 1023))");
    const int k = samples_per_ms / kChips;
    if (!rate_supported(k))
        return fail(ctx, GYP_E_BAD_RATE, "supported multiples of 1.023 MHz: 1, 2, 3, 4, 5, 6, 8, 10, 12, 16, 20, 48");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->codes.replicas.get()) {   // built into a local: the context gets the tables whole or, after a failure, not at all (the next call tries again)
        CodeBufs t;
        std::vector<uint8_t> chips(32 * kChips);
        if (make_prn_chips(chips.data()) != GYP_OK) return fail(ctx, GYP_E_BAD_ARG, "PRN self-check against IS-GPS-200 markers failed");
        std::vector<float> rep(32 * 32 * 64 * 2);
        for (int sv = 0; sv < 32; ++sv) make_replica_lane_layout(chips.data() + sv * kChips, rep.data() + (size_t)sv * 32 * 64 * 2);
        std::vector<float> tw(3072 * 2);   // tw1024, tw2048, 1024 ones (the even half-wave's radix-2 "twiddle", wave_fft_fwd)
        for (int n = 0; n < 1024; ++n) { tw[(2048 + n) * 2 + 0] = 1.0f; tw[(2048 + n) * 2 + 1] = 0.0f; }
        for (int g = 0; g < 32; ++g)
            for (int n = 0; n < 32; ++n) {
                const double a = -2.0 * M_PI * (double)(g * n) / 1024.0;
                tw[(g * 32 + n) * 2 + 0] = (float)std::cos(a);
                tw[(g * 32 + n) * 2 + 1] = (float)std::sin(a);
            }
        for (int n = 0; n < 1024; ++n) {
            const double a = -2.0 * M_PI * (double)n / 2048.0;
            tw[(1024 + n) * 2 + 0] = (float)std::cos(a);
            tw[(1024 + n) * 2 + 1] = (float)std::sin(a);
        }
        std::vector<uint16_t> ones(32 * 512);   // every C/A code has exactly 512 ones (balanced Gold codes)
        for (int sv = 0; sv < 32; ++sv) {
            int k1 = 0;
            for (int m = 0; m < kChips; ++m)
                if (chips[(size_t)sv * kChips + m] && k1 < 512) ones[(size_t)sv * 512 + k1++] = (uint16_t)m;
            if (k1 != 512) return fail(ctx, GYP_E_BAD_ARG, "a generated C/A code does not have 512 ones");
        }
        // chip transitions m (chip[m-1] != chip[m], indices mod 1023) with the sign of chip[m-1] - chip[m] as +-1 codes,
        // and the +-1 codes themselves laid out twice so that chip[(j - q) mod 1023] is chipf[j - q + 1023]
        std::vector<uint16_t> trans((size_t)32 * kMaxTrans, 0);
        std::vector<int32_t> ntrans(32, 0);
        std::vector<float> chipf((size_t)32 * 2048);
        for (int sv = 0; sv < 32; ++sv) {
            const uint8_t* c = chips.data() + (size_t)sv * kChips;
            int nt = 0;
            for (int m = 0; m < kChips; ++m) {
                const int prev = c[(m + kChips - 1) % kChips], cur = c[m];
                if (prev != cur) trans[(size_t)sv * kMaxTrans + nt++] = (uint16_t)(m | (prev < cur ? 0x8000 : 0));
            }
            ntrans[sv] = nt;
            for (int i = 0; i < 2048; ++i) chipf[(size_t)sv * 2048 + i] = c[i % kChips] ? 1.0f : -1.0f;
        }
        const auto put = [&](auto& buf, const auto& host, size_t count) -> hipError_t {   // (count in the buffer's elements)
            const hipError_t e = buf.reserve(count, Slack::exact);
            return e != hipSuccess ? e : hipMemcpy(buf.get(), host.data(), host.size() * sizeof(host[0]), hipMemcpyHostToDevice);
        };
        HIP_TRY(ctx, put(t.replicas, rep, rep.size() / 2));
        HIP_TRY(ctx, put(t.tw, tw, tw.size() / 2));
        HIP_TRY(ctx, put(t.chips, chips, chips.size()));
        HIP_TRY(ctx, put(t.ones, ones, ones.size()));
        HIP_TRY(ctx, put(t.trans, trans, trans.size()));
        HIP_TRY(ctx, put(t.ntrans, ntrans, ntrans.size()));
        HIP_TRY(ctx, put(t.chipf, chipf, chipf.size()));
        ctx->codes = std::move(t);
    }
    ctx->fs = fs_hz;
    ctx->n = samples_per_ms;
    ctx->k = k;
    return GYP_OK;
}

int gyp_malloc(gyp_ctx* ctx, uint64_t bytes, void** dptr) {
    if (!ctx || !dptr) return GYP_E_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 1);
    if (e != hipSuccess) return fail(ctx, GYP_E_NOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
    return GYP_OK;
}

int gyp_free(gyp_ctx* ctx, void* dptr) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (dptr) HIP_TRY(ctx, hipFree(dptr));
    return GYP_OK;
}

int gyp_memcpy_h2d(gyp_ctx* ctx, void* dst_dev, const void* src_host, uint64_t bytes) {
    if (!ctx || (!dst_dev && bytes) || (!src_host && bytes)) return GYP_E_BAD_ARG;
    HIP_TRY(ctx, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    return GYP_OK;
}

int gyp_memcpy_d2h(gyp_ctx* ctx, void* dst_host, const void* src_dev, uint64_t bytes) {
    if (!ctx || (!dst_host && bytes) || (!src_dev && bytes)) return GYP_E_BAD_ARG;
    HIP_TRY(ctx, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GYP_OK;
}

int gyp_memcpy_d2h_async(gyp_ctx* ctx, void* dst_host, const void* src_dev, uint64_t bytes) {
    if (!ctx || (!dst_host && bytes) || (!src_dev && bytes)) return GYP_E_BAD_ARG;
    HIP_TRY(ctx, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return GYP_OK;
}

double gyp_cell_strength(const gyp_cell* c, int32_t samples_per_ms) {
    const double pk = (double)c->peak;
    return pk / ((c->sum - (double)c->n_max * pk) / (double)(samples_per_ms - c->n_max));
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// launches
// ---------------------------------------------------------------------------------------------------------
// wavefronts a CU hosts for this rate (LDS tiles and VGPR budgets are sized for it), in workgroups
static int blocks_per_cu(int k) { return k > 8 ? 1 : 16 / k; }
static int threads_for(int k) { return 64 * largest_divisor_up_to_8(k); }

// a launch with `lds` bytes of dynamic LDS (above 64 KB a kernel has to be given leave first)
template <typename KernelT, typename... Args>
static int launch_dyn(gyp_ctx* ctx, KernelT kernel, dim3 grid, dim3 threads, size_t lds, hipStream_t stream, const Args&... args) {
    HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, grid, threads, lds, stream, args...);
    HIP_TRY(ctx, hipGetLastError());
    return GYP_OK;
}
template <typename KernelT, typename ParamsT>
static int launch_k(gyp_ctx* ctx, KernelT kernel, int k, int grid, const ParamsT& p, size_t lds, hipStream_t stream) {
    return launch_dyn(ctx, kernel, dim3(grid), dim3(threads_for(k)), lds, stream, p);
}
template <typename KernelT, typename ParamsT>
static int launch_k(gyp_ctx* ctx, KernelT kernel, int k, int grid, const ParamsT& p, size_t lds) {   // on the context's stream
    return launch_k(ctx, kernel, k, grid, p, lds, ctx->stream);
}

// The stream's samples per chip as a compile-time constant: f(std::integral_constant<int, K>) of the rate set by gyp_set_stream_format
template <typename F>
static int for_rate(gyp_ctx* ctx, F&& f) {
    switch (ctx->k) {
#define X(K) case K: return f(std::integral_constant<int, K>{});
        GYP_FOR_EACH_RATE(X)
#undef X
    }
    return fail(ctx, GYP_E_NO_FORMAT, kNoFormat);
}
// a run-time flag as a compile-time one: f(std::true_type) or f(std::false_type)
template <typename F>
static auto for_flag(bool flag, F&& f) { return flag ? f(std::true_type{}) : f(std::false_type{}); }
// behind a plain launch: what the runtime made of it
static int launched(gyp_ctx* ctx) {
    HIP_TRY(ctx, hipGetLastError());
    return GYP_OK;
}
// The workgroups a launch on the upload stream may take beside the trackers (cond_plan.hpp says why it is capped)
static int64_t persistent_cap(const gyp_ctx* ctx) { return gyp::persistent_cap(ctx->n_cus, ctx->widen_wg_per_cu); }
// `count` elements from device memory to the host on the context's stream, which is then synchronised: they are there on return
template <typename T>
static int fetch(gyp_ctx* ctx, T* host, const T* dev, size_t count) {
    HIP_TRY(ctx, hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GYP_OK;
}
template <typename T>
static int fetch(gyp_ctx* ctx, std::vector<T>& host, const T* dev) { return fetch(ctx, host.data(), dev, host.size()); }

static int launch_cells(gyp_ctx* ctx, const CellsParams& p, int integration) {
    // gyp_debug_set "cells_cu_reserve" n: the correlation-cell launches of this context (acquisition levels, gyp_correlate_cells) size
    // their persistent grids for n fewer CUs.  A receiver's scan context sets it: the scan's workgroups take a whole CU each (155 KB of
    // LDS) and hold it for the length of the launch, so a tracking round of the bank -- one 97-148 KB workgroup per channel, launched
    // every few hundred microseconds -- otherwise waits for one of them to drain; with 16 CUs (two per XCD: workgroup b runs on XCD
    // b % 8) never taken by the scan the trackers always find room.  The cells are walked grid-stride: same results.
    const int cus = std::max(ctx->n_xcd, ctx->n_cus - ctx->cells_cu_reserve);
    const int grid = std::max(1, std::min(p.n_cells, cus * blocks_per_cu(ctx->k)) & ~7);
    const bool coh = integration == GYP_COHERENT;
    if (!coh && ctx->k == 8 && !ctx->no_pipe) {   // one pipelined workgroup per CU (256 VGPRs, double-buffered LDS)
        const int grid1 = std::max(1, std::min(p.n_cells, cus) & ~7);
        return p.prof ? launch_k(ctx, corr_cells_pipe_kernel<8, true>, 8, grid1, p, lds_bytes_pipe<8>())
                      : launch_k(ctx, corr_cells_pipe_kernel<8, false>, 8, grid1, p, lds_bytes_pipe<8>());
    }
    return for_rate(ctx, [&](auto rate) {
        constexpr int K = decltype(rate)::value;
        return for_flag(coh, [&](auto c) { return launch_k(ctx, corr_cells_kernel<K, decltype(c)::value>, K, grid, p, lds_bytes<K>()); });
    });
}

// A level's shared forward transforms (acquire_search): MODE 1 over the units, then MODE 2 over their cells.  Both walk device-side work
// lists with a persistent grid of one workgroup per CU, like the unshared pipelined launch.
static int launch_cells_shared(gyp_ctx* ctx, const CellsParams& p_units, const CellsParams& p_cells) {
    const int cus = std::max(ctx->n_xcd, ctx->n_cus - ctx->cells_cu_reserve);
    const int grid1 = std::max(1, std::min(p_cells.n_cells, cus) & ~7);
    int rc = launch_k(ctx, corr_cells_pipe_kernel<8, false, 1>, 8, grid1, p_units, lds_bytes_pipe<8>());
    if (rc) return rc;
    return launch_k(ctx, corr_cells_pipe_kernel<8, false, 2>, 8, grid1, p_cells, lds_bytes_pipe<8>());
}

static int launch_track_step(gyp_ctx* ctx, const TrackStepParams& p) {
    const int grid = std::max(1, std::min(p.n_chan, ctx->n_cus * blocks_per_cu(ctx->k)) & ~7);
    return for_rate(ctx, [&](auto rate) {
        constexpr int K = decltype(rate)::value;
        return launch_k(ctx, track_step_kernel<K>, K, grid, p, lds_bytes<K>());
    });
}

template <bool PROF>
static int launch_track_block_t(gyp_ctx* ctx, const TrackBlockParams& p_in, int mode) {
    const int grid = p_in.n_chan;
    TrackBlockParams p = p_in;
    // gyp_debug_set "prof_wave" names a wavefront of workgroup 0: kernels with fewer wavefronts (K = 2 has two, K = 4 four in MODE 0) would
    // leave gyp_debug_track_profile's counters stale -- the last wavefront the launch has stamps them instead
    p.prof_wave = std::min(p.prof_wave, (mode == 2 ? 512 : threads_for(ctx->k)) / 64 - 1);
    if (mode == 2) {   // 512 threads whatever the rate (launch_k's block size follows its rate argument: 8 -> 512)
        if (ctx->k == 2) return launch_k(ctx, track_block_kernel<2, PROF, 2>, 8, grid, p, lds_bytes_spec<2>());
        if (ctx->k == 16) return launch_k(ctx, track_block_kernel<16, PROF, 2>, 8, grid, p, lds_bytes_spec<16>());
        return launch_k(ctx, track_block_kernel<8, PROF, 2>, 8, grid, p, lds_bytes_spec<8>());
    }
    return for_rate(ctx, [&](auto rate) {
        constexpr int K = decltype(rate)::value;
        return launch_k(ctx, track_block_kernel<K, PROF, 0>, K, grid, p, lds_bytes<K>());
    });
}
// mode 0: throughput kernel; 2: latency form + speculation (at most one workgroup per CU)
static int launch_track_block(gyp_ctx* ctx, const TrackBlockParams& p, int mode) {
    // (the instrumented instantiation also carries the optional profile rows: the fast one stays free of both)
    return (p.prof || p.prof_tail) ? launch_track_block_t<true>(ctx, p, mode) : launch_track_block_t<false>(ctx, p, mode);
}
static int launch_track_verify(gyp_ctx* ctx, const TrackVerifyParams& p, hipStream_t stream) {
    const int n_units = p.n_chan * (p.trk_round ? p.sub.longest : p.ms_end - p.ms_begin);
    int grid = std::max(8, std::min(n_units, ctx->n_cus * blocks_per_cu(ctx->k)) & ~7);
    if (p.trk_round) {
        // Round protocol: this launch runs beside the NEXT round's tracking launch, whose workgroups (one per channel, 97 KB of LDS)
        // fit no CU that already holds one of these (78 KB): a verify launch that fills the chip first makes the tracking launch wait
        // for it to drain, every round (0.3 us per ms-step of a 12-channel bank).  One workgroup per CU on all but the CUs the channels
        // need (workgroup b goes to XCD b % 8; inside an XCD the dispatcher fills the emptiest CU first) leaves those CUs empty.
        // (K = 2: the same with 46 KB / 8 x 212 registers against up to eight 2-wavefront verify workgroups per CU.)
        const int X = ctx->n_xcd, per_xcd = ctx->n_cus / X, need = (p.n_chan + X - 1) / X + 1;
        grid = X * std::max(4, per_xcd - need);
        grid = std::max(X, std::min(grid, n_units / X * X));
    }
    if (ctx->k == 2) return launch_k(ctx, track_verify_kernel<2>, 2, grid, p, lds_bytes<2>(), stream);
    if (ctx->k == 16) return launch_k(ctx, track_verify_kernel<16>, 16, grid, p, lds_bytes<16>(), stream);
    return launch_k(ctx, track_verify_kernel<8>, 8, grid, p, lds_bytes<8>(), stream);
}

// tracker.py:297 in float64 for every (channel, millisecond) of [ms_begin, ms_end), then the code loop re-integrated from it
template <int K>
static void launch_dll_exact_k(const gyp_ctx* ctx, const DllExactParams& p, int n_units, hipStream_t stream) {
    if constexpr (K <= 8) {
        const int grid = std::max(1, std::min((n_units + 3) / 4, ctx->n_cus * 8));
        hipLaunchKernelGGL(dll_exact_wave_kernel<K>, dim3(grid), dim3(256), 0, stream, p);
    } else {
        const int grid = std::max(1, std::min(n_units, ctx->n_cus * 8));
        hipLaunchKernelGGL(dll_exact_block_kernel<K>, dim3(grid), dim3(256), 0, stream, p);
    }
}
static int launch_dll_exact(gyp_ctx* ctx, const DllExactParams& p, hipStream_t stream) {
    // (round protocol: a round holds at most one sub-block per channel -- the kernels walk n_chan * round_length() units -- so the grid is
    // sized by the longest sub-block like launch_track_verify's, not by the whole block)
    const int n_units = p.n_chan * (p.trk_round ? p.sub.longest : p.ms_end - p.ms_begin);
    if (n_units <= 0) return GYP_OK;
    return for_rate(ctx, [&](auto rate) -> int {
        launch_dll_exact_k<decltype(rate)::value>(ctx, p, n_units, stream);
        HIP_TRY(ctx, hipGetLastError());
        return GYP_OK;
    });
}
// The same sums for the plain throughput call at 8 samples per chip: the channels are grouped by stream on the device, then one
// workgroup per CU stages each (group, millisecond) once for all the group's channels (dll_exact_shared_kernel).
static int launch_dll_exact_shared(gyp_ctx* ctx, const DllExactParams& p, ExactGroup* groups, hipStream_t stream) {
    if (p.n_chan <= 0 || p.ms_end <= p.ms_begin) return GYP_OK;
    int32_t* n_groups = reinterpret_cast<int32_t*>(groups + p.n_chan);
    HIP_TRY(ctx, hipMemsetAsync(n_groups, 0, sizeof(int32_t), stream));
    hipLaunchKernelGGL(exact_group_kernel, dim3((p.n_chan + 255) / 256), dim3(256), 0, stream, p.states, p.n_chan, groups, n_groups);
    DllExactSharedParams s;
    s.x = p; s.groups = groups; s.n_groups = n_groups;
    return launch_dyn(ctx, dll_exact_shared_kernel<8>, dim3(ctx->n_cus), dim3(kExactSharedThreads), exact_shared_lds_bytes<8>(), stream, s);
}
static int launch_dll_scan(gyp_ctx* ctx, const DllScanParams& p, hipStream_t stream) {
    return for_rate(ctx, [&](auto rate) -> int {
        hipLaunchKernelGGL(dll_scan_kernel<decltype(rate)::value>, dim3((unsigned)p.n_chan), dim3(kScanThreads), 0, stream, p);
        HIP_TRY(ctx, hipGetLastError());
        return GYP_OK;
    });
}

extern "C" {

// ---------------------------------------------------------------- correlation cells ----------------------
}   // extern "C"
// order_dev / n_active_dev: optional work list of the acquisition driver (see CellsParams)
static CellsParams cells_params(gyp_ctx* ctx, const float* iq_dev, int64_t stream_stride_samples, int32_t n_ms, const gyp_cell_desc* cells_dev,
                                int32_t n_cells, gyp_cell* out_dev, float* profile_out_dev, const int32_t* order_dev, const int32_t* n_active_dev) {
    CellsParams p;
    p.iq = reinterpret_cast<const cf*>(iq_dev);
    p.stream_stride = stream_stride_samples;
    p.n_ms = n_ms;
    p.cells = cells_dev;
    p.n_cells = n_cells;
    p.out = out_dev;
    p.profile_out = profile_out_dev;
    p.replica_table = ctx->codes.replicas.get();
    p.tw_tables = ctx->codes.tw.get();
    p.inv_fs = 1.0 / (double)ctx->fs;
    p.prof = ctx->prof.get();
    p.prof_wave = std::min(ctx->prof_wave, 7);
    p.order = order_dev;
    p.n_active = n_active_dev;
    p.spectra = nullptr;
    p.unit_of = nullptr;
    return p;
}
extern "C" {
int gyp_correlate_cells_dev(gyp_ctx* ctx, const float* iq_dev, int64_t stream_stride_samples, int32_t n_ms,
                            const gyp_cell_desc* cells_dev, int32_t n_cells, int32_t integration,
                            gyp_cell* out_dev, float* profile_out_dev) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    if (!iq_dev || !cells_dev || !out_dev || n_ms < 0 || n_cells < 0 || (integration != GYP_COHERENT && integration != GYP_NON_COHERENT))
        return fail(ctx, GYP_E_BAD_ARG, "gyp_correlate_cells_dev: bad argument");
    if (n_cells == 0) return GYP_OK;
    return launch_cells(ctx, cells_params(ctx, iq_dev, stream_stride_samples, n_ms, cells_dev, n_cells, out_dev, profile_out_dev, nullptr, nullptr), integration);
}

int gyp_correlate_cells(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, int32_t n_ms,
                        const gyp_cell_desc* cells_host, int32_t n_cells, int32_t integration,
                        gyp_cell* out_host, float* profile_out_host) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    if (!iq_host || !cells_host || !out_host || n_streams <= 0 || n_ms < 0 || n_cells < 0)
        return fail(ctx, GYP_E_BAD_ARG, "gyp_correlate_cells: bad argument");
    for (int i = 0; i < n_cells; ++i)
        if (cells_host[i].stream < 0 || cells_host[i].stream >= n_streams || cells_host[i].sat_id < 1 || cells_host[i].sat_id > 32 ||
            cells_host[i].tap_index >= ctx->n)
            return fail(ctx, GYP_E_BAD_ARG, "gyp_correlate_cells: cell descriptor out of range");
    if (n_cells == 0) return GYP_OK;
    Scratch& sc = ctx->scratch;
    const size_t n_iq = iq_floats(ctx, n_streams, n_ms), out_bytes = (size_t)n_cells * sizeof(gyp_cell);
    const size_t n_prof = profile_out_host ? (size_t)n_cells * ctx->n * (integration == GYP_COHERENT ? 2 : 1) : 0;
    HIP_TRY(ctx, sc.stage_out.reserve(out_bytes, Slack::grow, ctx->stream));
    HIP_TRY(ctx, sc.stage_profile.reserve(n_prof, Slack::grow, ctx->stream));
    HIP_TRY(ctx, upload(sc.stage_iq, iq_host, n_iq, ctx->stream, n_iq ? 0 : 2));
    HIP_TRY(ctx, upload(sc.stage_in, as_bytes(cells_host), (size_t)n_cells * sizeof(gyp_cell_desc), ctx->stream));
    if (const int rc = gyp_correlate_cells_dev(ctx, sc.stage_iq.get(), (int64_t)n_ms * ctx->n, n_ms, (const gyp_cell_desc*)sc.stage_in.get(), n_cells,
                                               integration, (gyp_cell*)sc.stage_out.get(), profile_out_host ? sc.stage_profile.get() : nullptr))
        return rc;
    return stage_back(ctx, out_host, out_bytes, profile_out_host, n_prof);
}

// ---------------------------------------------------------------- flat search grid -----------------------
}   // extern "C"
// The three scratch buffers that hold several arrays: one layout each, giving the size on a null base and the pointers on the buffer.
static size_t refine_list_layout(void* base, size_t n_rows, size_t n_cells, GridRefineParams* p) {   // Scratch::refine_list
    Carve c(base);
    p->n_cand = c.take<int32_t>(4);            // [0] candidates, [1] pending rows
    p->pend_rows = c.take<int32_t>(n_rows); p->pend_first = c.take<int32_t>(n_rows);
    p->cand = c.take<int32_t>(n_cells);
    return c.bytes();
}
struct AcqBook {        // acquire_search's bookkeeping (Scratch::acq_book)
    gyp_cell* prev_out;                       // the previous level's records
    int32_t *reuse, *order, *cand;            // reuse map, the level's work list, the tie-break's candidate list
    int32_t* pend;                            // = reuse: the reuse map is consumed by acq_reuse_kernel before acq_reduce_kernel fills this with the pending states
    int32_t *n_active, *n_cand, *n_pend;      // their lengths; candidates of the tie-break in n_cand[0], pending cross-level pairs in n_cand[1] = n_pend[0]
    size_t bytes;
};
static AcqBook acq_book_layout(void* base, size_t n_cells) {
    Carve c(base);
    AcqBook b;
    b.prev_out = c.take<gyp_cell>(n_cells);
    b.pend = b.reuse = c.take<int32_t>(n_cells); b.order = c.take<int32_t>(n_cells); b.cand = c.take<int32_t>(n_cells);
    b.n_active = c.take<int32_t>(1); b.n_cand = c.take<int32_t>(1); b.n_pend = c.take<int32_t>(1);   // three counters at the start of a 64-byte tail
    c.take<int32_t>(13);
    b.bytes = c.bytes();
    return b;
}
static size_t acq_units_layout(void* base, size_t max_units, size_t n_cells, AcqUnits* u) {   // Scratch::acq_units
    Carve c(base);
    u->unit_cell = c.take<int32_t>(max_units);
    u->sh_cell = c.take<int32_t>(n_cells); u->sh_unit = c.take<int32_t>(n_cells);
    u->counts = c.take<int32_t>(4);
    return c.bytes();
}

static_assert(sizeof(cf) == kGridCfBytes && sizeof(GridPartial) == kGridPartialBytes && kChips == kGridChips, "grid_plan.hpp sizes the scratch by these");
// 12 or 8 wavefronts per workgroup ("grid_fused_waves") as a compile-time constant
template <typename F>
static int for_waves(int waves, F&& f) { return waves == 8 ? f(std::integral_constant<int, 8>{}) : f(std::integral_constant<int, 12>{}); }

// The launches of a planned flat grid (grid_plan.hpp): the fold stage, unless it is fused into the cells kernel, then the cells kernel
template <int K>
static int launch_grid(gyp_ctx* ctx, const GridParams& p, const GridPlan& pl, bool coh) {
    hipStream_t stream = ctx->stream;
    const int n_units = p.n_streams * p.n_bins, n_cells = n_units * p.n_sats, n_blk = coh ? 1 : p.n_ms;
    const dim3 wgrid(pl.wgrid);
    const size_t lds_units = 2 * kTablesBytes + (size_t)pl.waves * kXchWaveBytes + (size_t)pl.waves * 32 * sizeof(SatStat);   // paths 1 and 2
    if constexpr (K <= 8) {
        if (pl.path == 1)
            return for_waves(pl.waves, [&](auto w) {
                constexpr int W = decltype(w)::value;
                return for_flag(coh, [&](auto c) {
                    return launch_dyn(ctx, grid_cells_wave_fused_kernel<K, decltype(c)::value, W>, wgrid, dim3(64 * W), lds_units, stream, p);
                });
            });
    }
    if constexpr (K > 8) {   // wide rates: coalesced wipe-off into z, then the K-sample boxcar out of LDS tiles
        cf* zbuf = ctx->scratch.z.get();
        const dim3 zgrid((unsigned)((K * kChips + 255) / 256), (unsigned)n_blk, (unsigned)n_units);
        for_flag(coh, [&](auto c) { hipLaunchKernelGGL((grid_wipe_kernel<K, decltype(c)::value>), zgrid, dim3(256), 0, stream, p, zbuf); });
        HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(grid_boxcar_kernel<K>, dim3(8, (unsigned)n_blk, (unsigned)n_units), dim3(128), 0, stream, p, (const cf*)zbuf, n_blk);
    } else {
        const dim3 fgrid((unsigned)n_units, (unsigned)n_blk, (unsigned)Geom<K>::R);
        for_flag(coh, [&](auto c) { hipLaunchKernelGGL((grid_fold_kernel<K, decltype(c)::value>), fgrid, dim3(threads_for(K)), 0, stream, p); });
    }
    HIP_TRY(ctx, hipGetLastError());
    if (pl.path == 2) {   // one wavefront per (unit, gs satellites, run of branches); runs are merged afterwards
        const int rc = for_waves(pl.waves, [&](auto w) {
            constexpr int W = decltype(w)::value;
            return launch_dyn(ctx, grid_cells_wave_shared_kernel<K, 32, W>, wgrid, dim3(64 * W), lds_units, stream, p, pl.gs);
        });
        if (rc || pl.parts == 1) return rc;
        hipLaunchKernelGGL(grid_merge_parts_kernel, dim3((n_cells + 255) / 256), dim3(256), 0, stream, p, n_cells);
        HIP_TRY(ctx, hipGetLastError());
        return GYP_OK;
    }
    if (pl.path == 4)   // a workgroup per cell
        return for_flag(coh, [&](auto c) { return launch_k(ctx, grid_cells_kernel<K, decltype(c)::value>, K, pl.wgrid, p, lds_bytes<K>()); });
    if constexpr (K % 2 == 0) {   // path 3: one wavefront per cell, with the next row prefetched or without barriers
        if (pl.pipe) return launch_dyn(ctx, grid_cells_wave_pipe_kernel<K>, wgrid, dim3(512), 2 * kTablesBytes + 8 * kXchWaveBytes, stream, p);
    }
    if constexpr (K <= 8) {
        if (!pl.pipe) return launch_dyn(ctx, grid_cells_wave_kernel<K>, wgrid, dim3(512), kTablesBytes + 8 * kXchWaveBytes, stream, p);
    }
    return fail(ctx, GYP_E_BAD_ARG, "flat grid: the plan names a kernel this rate does not have");
}
extern "C" {

int gyp_correlate_grid_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t n_ms,
                           const int32_t* sat_ids_host, int32_t n_sats, const double* doppler_hz_host, int32_t n_bins,
                           int32_t integration, gyp_cell* out_dev) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    if (!iq_dev || !sat_ids_host || !doppler_hz_host || !out_dev || n_streams <= 0 || n_ms <= 0 || n_sats <= 0 || n_bins <= 0 ||
        (integration != GYP_COHERENT && integration != GYP_NON_COHERENT))
        return fail(ctx, GYP_E_BAD_ARG, "gyp_correlate_grid_dev: bad argument");
    if (const int rc = check_sat_ids(ctx, sat_ids_host, n_sats)) return rc;
    const bool coh = integration == GYP_COHERENT;
    const int n_blk = coh ? 1 : n_ms;
    const int64_t n_units = (int64_t)n_streams * n_bins;
    if (n_units > 2147483647LL / 2 || n_blk > 65535) return fail(ctx, GYP_E_BAD_ARG, "gyp_correlate_grid_dev: grid too large");
    const GridPlan pl = grid_plan(GridShape{ctx->k, ctx->n_cus, n_units, n_sats, n_blk},
                                  GridSwitches{ctx->no_pipe, ctx->no_shared_fwd, ctx->no_grid_fused, ctx->no_grid_parts, ctx->grid_fused_waves});
    Scratch& sc = ctx->scratch;
    HIP_TRY(ctx, sc.folded.reserve(pl.folded_bytes / sizeof(cf), Slack::grow, ctx->stream));
    HIP_TRY(ctx, sc.z.reserve(pl.z_bytes / sizeof(cf), Slack::grow, ctx->stream));
    HIP_TRY(ctx, sc.grid_partial.reserve(pl.partial_bytes / sizeof(GridPartial), Slack::grow, ctx->stream));
    HIP_TRY(ctx, upload(sc.sat_ids, sat_ids_host, (size_t)n_sats, ctx->stream, 16));
    HIP_TRY(ctx, upload(sc.doppler, doppler_hz_host, (size_t)n_bins, ctx->stream, 8));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the host arrays may be temporaries
    GridParams p;
    p.iq = reinterpret_cast<const cf*>(iq_dev);
    p.stream_stride = stream_stride_samples;
    p.n_ms = n_ms; p.n_streams = n_streams; p.n_sats = n_sats; p.n_bins = n_bins;
    p.sat_ids = sc.sat_ids.get();
    p.doppler = sc.doppler.get();
    p.folded = sc.folded.get();
    p.out = out_dev;
    p.replica_table = ctx->codes.replicas.get();
    p.tw_tables = ctx->codes.tw.get();
    p.inv_fs = 1.0 / (double)ctx->fs;
    p.parts = pl.parts;
    p.partial = pl.partial_bytes ? sc.grid_partial.get() : nullptr;
    if (const int rc = for_rate(ctx, [&](auto rate) { return launch_grid<decltype(rate)::value>(ctx, p, pl, coh); })) return rc;
    ctx->last_grid_plan = pl;
    return GYP_OK;
}

int gyp_correlate_grid(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, int32_t n_ms, const int32_t* sat_ids_host,
                       int32_t n_sats, const double* doppler_hz_host, int32_t n_bins, int32_t integration, gyp_cell* out_host) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    if (!iq_host || !out_host || n_streams <= 0 || n_ms <= 0 || n_sats <= 0 || n_bins <= 0)
        return fail(ctx, GYP_E_BAD_ARG, "gyp_correlate_grid: bad argument");
    return staged_call(ctx, iq_host, n_streams, n_ms, out_host, (size_t)n_streams * n_sats * n_bins * sizeof(gyp_cell), [&](const float* iq_dev, int64_t stride, void* out_dev) {
        return gyp_correlate_grid_dev(ctx, iq_dev, n_streams, stride, n_ms, sat_ids_host, n_sats, doppler_hz_host, n_bins, integration, (gyp_cell*)out_dev);
    });
}

int gyp_grid_best_bins_dev(gyp_ctx* ctx, const gyp_cell* cells_dev, int32_t n_rows, int32_t n_bins, gyp_best_bin* out_dev) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    if (!cells_dev || !out_dev || n_rows < 0 || n_bins <= 0) return fail(ctx, GYP_E_BAD_ARG, "gyp_grid_best_bins_dev: bad argument");
    if (n_rows == 0) return GYP_OK;
    hipLaunchKernelGGL(grid_best_bin_kernel, dim3((n_rows + 255) / 256), dim3(256), 0, ctx->stream, cells_dev, n_rows, n_bins, ctx->n, out_dev);
    HIP_TRY(ctx, hipGetLastError());
    return GYP_OK;
}

int gyp_grid_best_bins_refined_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t n_ms,
                                   const int32_t* sat_ids_host, int32_t n_sats, const double* doppler_hz_host, int32_t n_bins, int32_t integration,
                                   const gyp_cell* cells_dev, gyp_best_bin* out_dev) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    if (!iq_dev || !sat_ids_host || !doppler_hz_host || !cells_dev || !out_dev || n_streams <= 0 || n_ms <= 0 || n_sats <= 0 || n_bins <= 0 ||
        (integration != GYP_COHERENT && integration != GYP_NON_COHERENT))
        return fail(ctx, GYP_E_BAD_ARG, "gyp_grid_best_bins_refined_dev: bad argument");
    if (const int rc = check_sat_ids(ctx, sat_ids_host, n_sats)) return rc;
    const int64_t n_rows = (int64_t)n_streams * n_sats, n_cells = n_rows * n_bins;
    if (n_cells > 2147483647LL / 2) return fail(ctx, GYP_E_BAD_ARG, "gyp_grid_best_bins_refined_dev: grid too large");
    Scratch& sc = ctx->scratch;
    GridRefineParams p;
    HIP_TRY(ctx, sc.refine_list.reserve(refine_list_layout(nullptr, (size_t)n_rows, (size_t)n_cells, &p), Slack::grow, ctx->stream));
    HIP_TRY(ctx, upload(sc.sat_ids, sat_ids_host, (size_t)n_sats, ctx->stream, 16));
    HIP_TRY(ctx, upload(sc.doppler, doppler_hz_host, (size_t)n_bins, ctx->stream, 8));
    p.iq = reinterpret_cast<const cf*>(iq_dev);
    p.stream_stride = stream_stride_samples;
    p.n_ms = n_ms; p.n_per_ms = ctx->n; p.k = ctx->k; p.n_sats = n_sats; p.n_bins = n_bins; p.n_rows = (int32_t)n_rows;
    p.coherent = integration == GYP_COHERENT ? 1 : 0;
    p.sat_ids = sc.sat_ids.get();
    p.doppler = sc.doppler.get();
    p.cells = cells_dev; p.out = out_dev; p.chips = ctx->codes.chips.get(); p.inv_fs = 1.0 / (double)ctx->fs;
    refine_list_layout(sc.refine_list.get(), (size_t)n_rows, (size_t)n_cells, &p);
    HIP_TRY(ctx, hipMemsetAsync(p.n_cand, 0, 4 * sizeof(int32_t), ctx->stream));
    p.partial = nullptr;
    hipLaunchKernelGGL(grid_best_bin_select_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    // how many candidates there are decides the size of the per-millisecond sums: one small read-back (the host arrays above are
    // temporaries of the caller anyway: the entry point synchronises like gyp_correlate_grid_dev)
    int32_t counts[2] = {0, 0};
    if (const int rc = fetch(ctx, counts, p.n_cand, 2)) return rc;
    ctx->last_grid_refined_rows = counts[1];
    if (counts[0] == 0) return GYP_OK;
    HIP_TRY(ctx, sc.partial64.reserve((size_t)counts[0] * n_ms * 2, Slack::grow, ctx->stream));
    p.partial = sc.partial64.get();
    hipLaunchKernelGGL(grid_refine_kernel, dim3((unsigned)std::min(counts[0], 65535), (unsigned)n_ms), dim3(256), 0, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(grid_best_bin_decide_kernel, dim3((unsigned)std::min((counts[1] + 63) / 64, 1024)), dim3(64), 0, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    return GYP_OK;
}

// ---------------------------------------------------------------- acquisition ----------------------------
// acquisition.py:70-152 from (center, spread) down to min_spread -- or exactly one level -- for every (stream, satellite).
// The host path is plan -> parameter set -> begin / level / finish: acq_plan (acq_plan.hpp) says what the search runs and how large its
// scratch is, acq_param_set builds every kernel's parameters once, and each step is the list of its launches.

// The arguments of one search: a call's own, or one part of a split scan (its streams of the caller's buffers, from stream_base on)
struct AcqCall { const float* iq_dev; int32_t n_streams; int64_t stream_stride; int32_t n_ms; const int32_t* sat_ids_host; int32_t n_sats; gyp_acq_result* out_dev; int stream_base; };
// ... checked and planned, for both entry points and for each part of a scan.  split: a scan that may go through in parts (gyp_acquire_dev);
// a part, a single level and a helper's search are planned whole
static int plan_search(gyp_ctx* ctx, const AcqCall& c, const AcqSearch& q, bool split, AcqPlan* pl) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    if (!c.iq_dev || !c.sat_ids_host || !c.out_dev || c.n_streams <= 0 || c.n_sats <= 0 || c.n_ms <= 0)
        return fail(ctx, GYP_E_BAD_ARG, "gyp_acquire_dev / gyp_search_level_dev: bad argument");
    if (const int rc = check_sat_ids(ctx, c.sat_ids_host, c.n_sats)) return rc;
    if (c.n_sats > 32) return fail(ctx, GYP_E_BAD_ARG, "at most 32 satellites per search");
    *pl = acq_plan(AcqShape{ctx->k, ctx->n, c.n_streams, c.n_sats, c.n_ms}, q,
                   AcqLevels{ctx->params.acq_initial_spread_hz, ctx->params.acq_min_spread_hz, ctx->params.acq_bins_per_spread},
                   AcqSwitches{ctx->no_pipe, ctx->no_acq_shared_fwd, ctx->no_acq_split || !split, ctx->is_helper, ctx->acq_lanes});
    if (!pl->fits) return fail(ctx, GYP_E_BAD_ARG, "gyp_acquire_dev / gyp_search_level_dev: search too large (at most 65535 ms, and 2^31 - 1 cells at 28 per stream and satellite)");
    return GYP_OK;
}
static int acq_reserve(gyp_ctx* ctx, const AcqPlan& pl) {
    Scratch& sc = ctx->scratch;
    HIP_TRY(ctx, sc.acq_states.reserve(pl.states, Slack::grow, ctx->stream));
    HIP_TRY(ctx, sc.acq_cells.reserve(pl.cells, Slack::grow, ctx->stream));
    HIP_TRY(ctx, sc.acq_out.reserve(pl.out, Slack::grow, ctx->stream));
    HIP_TRY(ctx, sc.acq_refined.reserve(pl.refined, Slack::grow, ctx->stream));
    HIP_TRY(ctx, sc.acq_book.reserve(acq_book_layout(nullptr, pl.cells).bytes, Slack::grow, ctx->stream));
    HIP_TRY(ctx, sc.partial64.reserve(pl.partial64, Slack::grow, ctx->stream));
    HIP_TRY(ctx, sc.acq_profiles.reserve(pl.profiles, Slack::grow, ctx->stream));   // written whole by acq_exact_profile_kernel
    if (pl.max_units > 0) {
        AcqUnits sized;
        HIP_TRY(ctx, sc.acq_spectra.reserve(pl.spectra, Slack::grow, ctx->stream));
        HIP_TRY(ctx, sc.acq_units.reserve(acq_units_layout(nullptr, (size_t)pl.max_units, pl.cells, &sized), Slack::grow, ctx->stream));
    }
    return GYP_OK;
}

// Every kernel's parameters of one search, built once from the context, the plan and the reserved scratch: no level changes any of them
struct AcqParamSet {
    AcqSearchState* states; gyp_cell_desc* cells; gyp_cell* out; double* refined;   // Scratch::acq_states, acq_cells, acq_out, acq_refined
    int cells_per_stream;
    AcqBook book;
    AcqUnits units;
    CellsParams cells_units, cells_shared, cells_listed;   // MODE 1 over the units, MODE 2 over their cells; the level's work list
    RefineParams refine;
    ExactParams exact;
};
static AcqParamSet acq_param_set(gyp_ctx* ctx, const AcqCall& c, const AcqPlan& pl) {
    Scratch& sc = ctx->scratch;
    AcqParamSet s{};
    s.states = sc.acq_states.get(); s.cells = sc.acq_cells.get(); s.out = sc.acq_out.get(); s.refined = sc.acq_refined.get();
    s.cells_per_stream = c.n_sats * kMaxBins;
    s.book = acq_book_layout(sc.acq_book.get(), pl.cells);
    s.cells_listed = cells_params(ctx, c.iq_dev, c.stream_stride, c.n_ms, s.cells, pl.n_cells, s.out, nullptr, s.book.order, s.book.n_active);
    s.units.max_units = pl.max_units;
    if (pl.max_units > 0) {
        acq_units_layout(sc.acq_units.get(), (size_t)pl.max_units, pl.cells, &s.units);
        s.cells_units = s.cells_listed;
        s.cells_units.order = s.units.unit_cell; s.cells_units.n_active = s.units.counts; s.cells_units.prof = nullptr; s.cells_units.spectra = sc.acq_spectra.get();
        s.cells_shared = s.cells_units;
        s.cells_shared.order = s.units.sh_cell; s.cells_shared.n_active = s.units.counts + 1; s.cells_shared.unit_of = s.units.sh_unit;
    }
    RefineParams& rp = s.refine;
    rp.iq = reinterpret_cast<const cf*>(c.iq_dev); rp.stream_stride = c.stream_stride; rp.n_ms = c.n_ms; rp.n_per_ms = ctx->n; rp.k = ctx->k;
    rp.states = s.states; rp.cells = s.cells; rp.out = s.out; rp.refined = s.refined;
    rp.chips = ctx->codes.chips.get(); rp.inv_fs = 1.0 / (double)ctx->fs;
    rp.cand = s.book.cand; rp.n_cand = s.book.n_cand; rp.partial = sc.partial64.get();
    ExactParams& ep = s.exact;   // cross-level near-ties in strength: float64 profiles for the (few) pending pairs, else immediate exits
    ep.iq = rp.iq; ep.stream_stride = c.stream_stride; ep.n_ms = c.n_ms; ep.n_per_ms = ctx->n; ep.k = ctx->k; ep.n_states = pl.n_states;
    ep.states = s.states; ep.ones = ctx->codes.ones.get(); ep.inv_fs = rp.inv_fs; ep.profiles = sc.acq_profiles.get();
    ep.pend = s.book.pend; ep.n_pend = s.book.n_pend;
    return s;
}

static void acq_begin(gyp_ctx* ctx, const AcqCall& c, const AcqSearch& q, const AcqParamSet& s, const AcqPlan& pl) {
    AcqSatList sl;
    for (int i = 0; i < 32; ++i) sl.id[i] = i < c.n_sats ? c.sat_ids_host[i] : 0;
    hipLaunchKernelGGL(acq_init_kernel, dim3(pl.nblk), dim3(pl.tpb), 0, ctx->stream, s.states, pl.n_states, c.n_sats, sl, q.center0, q.spread0,
                       ctx->acq_witness.get());   // acquisition.py:78-79
}
static int acq_level(gyp_ctx* ctx, const AcqParamSet& s, const AcqPlan& pl, int level) {
    const dim3 per_state(pl.nblk), tpb(pl.tpb);
    const AcqBook& b = s.book;
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(acq_plan_kernel, per_state, tpb, 0, st, s.states, pl.n_states, s.cells, b.reuse, pl.bins_per_spread,
                       ctx->params.acq_reuse_level_records != 0.0 ? 1 : 0);
    if (level < pl.shared_levels) {
        hipLaunchKernelGGL(acq_compact_units_kernel, dim3(1), dim3(1024), 0, st, (const gyp_cell_desc*)s.cells, pl.n_cells, s.cells_per_stream,
                           b.order, b.n_active, b.n_cand, s.units, ctx->acq_witness.get(), level);
        if (const int rc = launch_cells_shared(ctx, s.cells_units, s.cells_shared)) return rc;
    } else {
        hipLaunchKernelGGL(acq_compact_kernel, dim3(1), dim3(1024), 0, st, (const gyp_cell_desc*)s.cells, pl.n_cells, b.order, b.n_active, b.n_cand,
                           ctx->acq_witness.get(), level);
    }
    if (const int rc = launch_cells(ctx, s.cells_listed, GYP_NON_COHERENT)) return rc;
    hipLaunchKernelGGL(acq_reuse_kernel, dim3((unsigned)pl.n_states), dim3(64), 0, st, (const int32_t*)b.reuse, s.out, b.prev_out,
                       (const AcqSearchState*)s.states, s.refined, b.cand, b.n_cand, pl.n_states);
    hipLaunchKernelGGL(acq_refine_kernel, dim3((unsigned)pl.refine_x, (unsigned)pl.refine_y), dim3(256), 0, st, s.refine);
    hipLaunchKernelGGL(acq_refine_sum_kernel, per_state, dim3(64), 0, st, s.refine);
    hipLaunchKernelGGL(acq_reduce_kernel, per_state, tpb, 0, st, s.states, pl.n_states, s.out, s.refined, ctx->n, b.pend, b.n_pend);
    hipLaunchKernelGGL(acq_exact_profile_kernel, dim3((unsigned)(ctx->k * kExactSplit), 2, (unsigned)pl.exact_z), dim3(1024), 0, st, s.exact);
    hipLaunchKernelGGL(acq_exact_decide_kernel, dim3((unsigned)pl.exact_z), dim3(256), 0, st, s.exact);
    return GYP_OK;
}
// The coherent pass over every state's best bin (acquisition.py:91-152) -- a single level reports its bin as it is
static int acq_finish(gyp_ctx* ctx, const AcqCall& c, const AcqSearch& q, const AcqParamSet& s, const AcqPlan& pl) {
    const gyp_cell* coherent = nullptr;
    if (!q.single_level) {
        hipLaunchKernelGGL(acq_plan_coherent_kernel, dim3(pl.nblk), dim3(pl.tpb), 0, ctx->stream, s.states, pl.n_states, s.cells);
        if (const int rc = gyp_correlate_cells_dev(ctx, c.iq_dev, c.stream_stride, c.n_ms, s.cells, pl.n_states, GYP_COHERENT, s.out, nullptr)) return rc;
        coherent = s.out;
    }
    hipLaunchKernelGGL(acq_finish_kernel, dim3(pl.nblk), dim3(pl.tpb), 0, ctx->stream, s.states, pl.n_states, coherent, c.out_dev, c.stream_base);
    HIP_TRY(ctx, hipGetLastError());
    return GYP_OK;
}

static int acquire_search(gyp_ctx* ctx, const AcqCall& c, const AcqSearch& q) {
    AcqPlan pl;
    if (const int rc = plan_search(ctx, c, q, false, &pl)) return rc;
    ctx->last_acq_plan = pl;
    if (const int rc = acq_reserve(ctx, pl)) return rc;
    const AcqParamSet set = acq_param_set(ctx, c, pl);
    acq_begin(ctx, c, q, set, pl);
    for (int level = 0; level < pl.n_levels; ++level)
        if (const int rc = acq_level(ctx, set, pl, level)) return rc;
    return acq_finish(ctx, c, q, set, pl);
}

// The other parts of a multi-stream scan (AcqPlan::lanes) run on helper contexts of their own
static gyp_ctx* acquire_helper(gyp_ctx* ctx, int which) {
    if (!ctx->helper[which]) {
        gyp_ctx* h = nullptr;
        if (gyp_create(ctx->device, &h) != GYP_OK) return nullptr;
        h->is_helper = true;
        ctx->helper[which] = h;
    }
    gyp_ctx* h = ctx->helper[which];
    if (h->fs != ctx->fs || h->n != ctx->n)
        if (gyp_set_stream_format(h, ctx->fs, ctx->n) != GYP_OK) return nullptr;
    h->params = ctx->params;
    // the helper runs under the caller's switches (it never read an environment of its own)
    for (const DebugSwitch& k : kDebugSwitches)
        if (k.inherited) k.set(*h, k.get(*ctx));
    return h;
}

int gyp_acquire_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples,
                    int32_t n_ms, const int32_t* sat_ids_host, int32_t n_sats, gyp_acq_result* out_dev) {
    const AcqCall call{iq_dev, n_streams, stream_stride_samples, n_ms, sat_ids_host, n_sats, out_dev, 0};
    const AcqSearch scan{0.0, ctx ? ctx->params.acq_initial_spread_hz : 0.0, false};
    AcqPlan pl;
    if (const int rc = plan_search(ctx, call, scan, true, &pl)) return rc;
    gyp_ctx* lane_ctx[kMaxAcqLanes] = {ctx};
    for (int i = 1; i < pl.lanes; ++i)
        if (!(lane_ctx[i] = acquire_helper(ctx, i - 1))) pl.lanes = 1;   // no helper: the whole scan on this context
    if (pl.lanes == 1) return acquire_search(ctx, call, scan);
    int rc = GYP_OK;
    std::string why;
    // (a failure of gyp_wait_for(helper, ctx) leaves its text in the helper: everything is reported through the caller's context)
    for (int i = 1; i < pl.lanes && !rc; ++i)
        if ((rc = gyp_wait_for(lane_ctx[i], ctx))) why = "gyp_acquire_dev: ordering a helper stream behind the caller's: " + lane_ctx[i]->err;   // the samples may still be on their way on this context's stream
    int enqueued = 0;
    for (int i = 0; i < pl.lanes && !rc; ++i) {
        const int s0 = pl.lane_first[i];
        gyp_ctx* c = lane_ctx[i];
        rc = acquire_search(c, AcqCall{iq_dev + (int64_t)s0 * stream_stride_samples * 2, pl.lane_streams[i], stream_stride_samples, n_ms, sat_ids_host, n_sats,
                                       out_dev + (size_t)s0 * n_sats, s0}, scan);
        if (rc) why = c == ctx ? ctx->err : std::string("part of the scan on a helper stream: ") + c->err;
        enqueued = i + 1;   // (a part that failed half way may have launches in flight too)
    }
    ctx->last_acq_plan = pl;   // the scan's, with the parts it went through in (this context's own part has left its plan here)
    // Join every helper that may have work in flight -- ALSO on failure: the caller is entitled to free or overwrite iq_dev /
    // out_dev as soon as its own stream has passed this point, error or not.
    for (int i = 1; i < std::max(enqueued, rc ? pl.lanes : 0); ++i) {
        const int rj = gyp_wait_for(ctx, lane_ctx[i]);            // whatever follows on this context's stream sees every part
        if (rj && !rc) { rc = rj; why = "gyp_acquire_dev: joining a helper stream: " + ctx->err; }
        if (rj) (void)hipStreamSynchronize(lane_ctx[i]->stream);  // the event path failed: wait for the helper on the host instead
    }
    return rc ? fail(ctx, rc, why) : GYP_OK;
}

int gyp_search_level_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t n_ms,
                         const int32_t* sat_ids_host, int32_t n_sats, double center_hz, double spread_hz, gyp_acq_result* out_dev) {
    if (!ctx) return GYP_E_BAD_ARG;
    const int step = (int)(spread_hz / ctx->params.acq_bins_per_spread);
    if (!(spread_hz > 0) || step < 1 || ((int)(center_hz + spread_hz) - (int)(center_hz - spread_hz) + step - 1) / step > kMaxBins)
        return fail(ctx, GYP_E_BAD_ARG, "gyp_search_level_dev: the level must have between 1 and 28 Doppler bins");
    return acquire_search(ctx, AcqCall{iq_dev, n_streams, stream_stride_samples, n_ms, sat_ids_host, n_sats, out_dev, 0}, AcqSearch{center_hz, spread_hz, true});
}

// What gyp_search_level and gyp_acquire refuse themselves
static int search_check(gyp_ctx* ctx, const char* who, const float* iq_host, int32_t n_streams, int32_t n_ms, int32_t n_sats, const gyp_acq_result* out_host) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    if (!iq_host || !out_host || n_streams <= 0 || n_ms <= 0 || n_sats <= 0) return fail(ctx, GYP_E_BAD_ARG, std::string(who) + ": bad argument");
    return GYP_OK;
}

int gyp_search_level(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, int32_t n_ms, const int32_t* sat_ids_host,
                     int32_t n_sats, double center_hz, double spread_hz, gyp_acq_result* out_host) {
    if (const int rc = search_check(ctx, "gyp_search_level", iq_host, n_streams, n_ms, n_sats, out_host)) return rc;
    return staged_call(ctx, iq_host, n_streams, n_ms, out_host, (size_t)n_streams * n_sats * sizeof(gyp_acq_result), [&](const float* iq_dev, int64_t stride, void* out_dev) {
        return gyp_search_level_dev(ctx, iq_dev, n_streams, stride, n_ms, sat_ids_host, n_sats, center_hz, spread_hz, (gyp_acq_result*)out_dev);
    });
}

int gyp_acquire(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, int32_t n_ms, const int32_t* sat_ids_host,
                int32_t n_sats, gyp_acq_result* out_host) {
    if (const int rc = search_check(ctx, "gyp_acquire", iq_host, n_streams, n_ms, n_sats, out_host)) return rc;
    return staged_call(ctx, iq_host, n_streams, n_ms, out_host, (size_t)n_streams * n_sats * sizeof(gyp_acq_result), [&](const float* iq_dev, int64_t stride, void* out_dev) {
        return gyp_acquire_dev(ctx, iq_dev, n_streams, stride, n_ms, sat_ids_host, n_sats, (gyp_acq_result*)out_dev);
    });
}

// ---------------------------------------------------------------- weak-signal acquisition -----------------
}   // extern "C"
// What both hybrid entry points refuse (hybrid_plan.hpp: hybrid_refusal), before anything is reserved or launched.
static int hybrid_check(gyp_ctx* ctx, const char* who, const void* iq, const void* out, int32_t n_streams, int64_t stream_stride_samples,
                        int32_t coherent_ms, int32_t n_blocks, int32_t flags, const int32_t* sat_ids_host, int32_t n_sats) {
    if (!iq || !out || !sat_ids_host || n_streams <= 0 || n_sats <= 0 || stream_stride_samples < 0) return refuse(ctx, who, "bad argument");
    if (const char* why = hybrid_refusal(coherent_ms, n_blocks, flags)) return refuse(ctx, who, why);
    return check_sat_ids(ctx, sat_ids_host, n_sats);
}

// hybrid_run's scratch for a plan: the one place hyb_cell_out, hyb_profile and hyb_power are reserved.
static int hybrid_reserve(gyp_ctx* ctx, const HybPlan& pl) {
    Scratch& sc = ctx->scratch;
    HIP_TRY(ctx, sc.hyb_cell_out.reserve((size_t)pl.chunk_cells, Slack::grow, ctx->stream));
    HIP_TRY(ctx, sc.hyb_profile.reserve(pl.profile, Slack::grow, ctx->stream));
    HIP_TRY(ctx, sc.hyb_power.reserve(pl.power, Slack::grow, ctx->stream));
    return GYP_OK;
}

// The records of n_cells cells (device table) into out_dev: the cells go through in chunks that fit the scratch budget; per chunk
// every block's coherent profiles (the cells launch, unchanged, given the block as its whole buffer) are added into the power rows
// of the block's set, in increasing block order, then reduced.  Enqueues only; the scratch is reserved before the first launch.
static int hybrid_run(gyp_ctx* ctx, const float* iq_dev, int64_t stream_stride_samples, int32_t coherent_ms, int32_t n_blocks, int32_t flags,
                      const gyp_cell_desc* cells_dev, int64_t n_cells, gyp_hybrid_cell* out_dev) {
    const HybPlan pl = hybrid_plan(HybShape{ctx->n, n_cells, coherent_ms, n_blocks, flags}, ctx->hybrid_scratch_mb);
    if (!pl.fits) return fail(ctx, GYP_E_BAD_ARG, "hybrid search: the request does not fit (more than 2^31 - 1 cells?)");
    if (const int rc = hybrid_reserve(ctx, pl)) return rc;
    Scratch& sc = ctx->scratch;
    for (int64_t c0 = 0; c0 < n_cells; c0 += pl.chunk_cells) {
        const int32_t nc = (int32_t)std::min<int64_t>(pl.chunk_cells, n_cells - c0);
        HybAccParams a;
        a.profile = sc.hyb_profile.get();
        a.power = sc.hyb_power.get();
        a.cells = cells_dev + c0;
        a.n = ctx->n; a.coherent_ms = coherent_ms; a.flags = flags; a.n_sets = pl.n_sets;
        for (int32_t b = 0; b < n_blocks; ++b) {
            const float* block = iq_dev + (int64_t)b * coherent_ms * ctx->n * 2;
            if (const int rc = launch_cells(ctx, cells_params(ctx, block, stream_stride_samples, coherent_ms, cells_dev + c0, nc, sc.hyb_cell_out.get(),
                                                              reinterpret_cast<float*>(sc.hyb_profile.get()), nullptr, nullptr), GYP_COHERENT))
                return rc;
            a.block = b;
            hipLaunchKernelGGL(hybrid_accumulate_kernel, dim3((unsigned)pl.acc_x, (unsigned)nc), dim3(256), 0, ctx->stream, a);
            if (const int rc = launched(ctx)) return rc;
        }
        hipLaunchKernelGGL(hybrid_reduce_kernel, dim3((unsigned)nc), dim3(256), 0, ctx->stream, (const float*)sc.hyb_power.get(), ctx->n, pl.n_sets,
                           n_blocks, out_dev + c0);
        if (const int rc = launched(ctx)) return rc;
    }
    ctx->last_hybrid_plan = pl;
    return GYP_OK;
}
extern "C" {

int gyp_hybrid_stats(const gyp_hybrid_cell* c, double* z_out, double* peak_ratio_out) {
    if (!c) return fail(nullptr, GYP_E_BAD_ARG, "gyp_hybrid_stats: NULL record");
    if (z_out) *z_out = hybrid_z(c->peak, c->n_off, c->sum_off, c->sumsq_off);
    if (peak_ratio_out) *peak_ratio_out = (double)c->peak / (double)c->second;
    return GYP_OK;
}

int gyp_hybrid_shift(int32_t n, int32_t coherent_ms, int32_t block, double doppler_hz, int32_t flags) {
    return hybrid_shift(n, coherent_ms, block, doppler_hz, flags);
}

int gyp_correlate_grid_hybrid_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t coherent_ms,
                                  int32_t n_blocks, int32_t flags, const int32_t* sat_ids_host, int32_t n_sats, const double* doppler_hz_host,
                                  int32_t n_bins, gyp_hybrid_cell* out_dev) {
    static const char* const who = "gyp_correlate_grid_hybrid_dev";
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    if (!doppler_hz_host || n_bins <= 0) return refuse(ctx, who, "bad argument");
    if (const int rc = hybrid_check(ctx, who, iq_dev, out_dev, n_streams, stream_stride_samples, coherent_ms, n_blocks, flags, sat_ids_host, n_sats)) return rc;
    for (int i = 0; i < n_bins; ++i)
        if (!std::isfinite(doppler_hz_host[i])) return refuse(ctx, who, "a Doppler bin is not finite");
    const int64_t n_cells = (int64_t)n_streams * n_sats * n_bins;
    if (n_cells > INT32_MAX) return refuse(ctx, who, "more than 2^31 - 1 cells");
    Scratch& sc = ctx->scratch;
    HIP_TRY(ctx, sc.hyb_grid_cells.reserve((size_t)n_cells, Slack::grow, ctx->stream));
    HIP_TRY(ctx, upload(sc.hyb_sat_ids, sat_ids_host, (size_t)n_sats, ctx->stream));
    HIP_TRY(ctx, upload(sc.hyb_doppler, doppler_hz_host, (size_t)n_bins, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the host arrays may be temporaries
    hipLaunchKernelGGL(hybrid_grid_cells_kernel, dim3((unsigned)((n_cells + 255) / 256)), dim3(256), 0, ctx->stream, (const int32_t*)sc.hyb_sat_ids.get(),
                       (const double*)sc.hyb_doppler.get(), n_sats, n_bins, (int32_t)n_cells, sc.hyb_grid_cells.get());
    if (const int rc = launched(ctx)) return rc;
    return hybrid_run(ctx, iq_dev, stream_stride_samples, coherent_ms, n_blocks, flags, sc.hyb_grid_cells.get(), n_cells, out_dev);
}

int gyp_correlate_grid_hybrid(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, int32_t coherent_ms, int32_t n_blocks, int32_t flags,
                              const int32_t* sat_ids_host, int32_t n_sats, const double* doppler_hz_host, int32_t n_bins,
                              gyp_hybrid_cell* out_host) {
    static const char* const who = "gyp_correlate_grid_hybrid";
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    if (!doppler_hz_host || n_bins <= 0) return refuse(ctx, who, "bad argument");
    if (const int rc = hybrid_check(ctx, who, iq_host, out_host, n_streams, 0, coherent_ms, n_blocks, flags, sat_ids_host, n_sats)) return rc;
    const int64_t n_cells = (int64_t)n_streams * n_sats * n_bins;
    if (n_cells > INT32_MAX) return refuse(ctx, who, "more than 2^31 - 1 cells");
    return staged_call(ctx, iq_host, n_streams, n_blocks * coherent_ms, out_host, (size_t)n_cells * sizeof(gyp_hybrid_cell), [&](const float* iq_dev, int64_t stride, void* out_dev) {
        return gyp_correlate_grid_hybrid_dev(ctx, iq_dev, n_streams, stride, coherent_ms, n_blocks, flags, sat_ids_host, n_sats, doppler_hz_host, n_bins, (gyp_hybrid_cell*)out_dev);
    });
}

}   // extern "C"
// One level of gyp_acquire_weak_dev (0 coarse, 1 fine): hybrid_run over the level's cells, then the select kernel, which writes the next
// level's cells around each state's best bin -- behind the last level the final cells and the results.  The one place HybSelectParams is filled.
struct WeakCall { const float* iq; int64_t stride; int32_t coherent_ms, n_blocks, flags; double fine_step_hz; gyp_weak_result* out; };
static int weak_level(gyp_ctx* ctx, const WeakCall& c, const WeakSearchPlan& pl, int level) {
    Scratch& sc = ctx->scratch;
    gyp_cell_desc* const cells = sc.hyb_level_cells.get() + (level ? pl.coarse_cells : 0);
    const bool last = level == 1 || pl.fine_half < 0;
    if (const int rc = hybrid_run(ctx, c.iq, c.stride, c.coherent_ms, c.n_blocks, c.flags, cells, (int64_t)(level ? pl.fine_cells : pl.coarse_cells), sc.hyb_records.get()))
        return rc;
    HybSelectParams sp;
    sp.recs = sc.hyb_records.get();
    sp.cells = cells;
    sp.n_states = (int32_t)pl.n_states; sp.n_bins = level ? pl.n_fine : pl.n_coarse;
    sp.next_half = last ? -1 : pl.fine_half; sp.next_step = c.fine_step_hz;
    sp.next_cells = sc.hyb_level_cells.get() + pl.coarse_cells + (last ? pl.fine_cells : 0);
    sp.out = c.out;
    hipLaunchKernelGGL(hybrid_select_kernel, dim3((unsigned)((pl.n_states + 63) / 64)), dim3(64), 0, ctx->stream, sp);
    return launched(ctx);
}
extern "C" {

int gyp_acquire_weak_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t coherent_ms,
                         int32_t n_blocks, int32_t flags, double center_hz, double spread_hz, double fine_step_hz,
                         const int32_t* sat_ids_host, int32_t n_sats, gyp_weak_result* out_dev) {
    static const char* const who = "gyp_acquire_weak_dev";
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    if (const int rc = hybrid_check(ctx, who, iq_dev, out_dev, n_streams, stream_stride_samples, coherent_ms, n_blocks, flags, sat_ids_host, n_sats)) return rc;
    const WeakSearchPlan pl = weak_search_plan(WeakSearchShape{ctx->n, n_streams, n_sats, coherent_ms, n_blocks, flags, center_hz, spread_hz, fine_step_hz}, ctx->hybrid_scratch_mb);
    if (pl.refusal) return refuse(ctx, who, pl.refusal);
    Scratch& sc = ctx->scratch;
    const size_t states = (size_t)pl.n_states;
    HIP_TRY(ctx, sc.hyb_level_cells.reserve(pl.level_cells, Slack::grow, ctx->stream));
    HIP_TRY(ctx, sc.hyb_records.reserve(pl.records, Slack::grow, ctx->stream));
    HIP_TRY(ctx, sc.hyb_taps.reserve(states, Slack::grow, ctx->stream));
    if (const int rc = hybrid_reserve(ctx, pl.run)) return rc;
    const dim3 sgrid((unsigned)((pl.n_states + 63) / 64));
    HybSatIds ids{};
    for (int i = 0; i < n_sats; ++i) ids.v[i] = sat_ids_host[i];
    hipLaunchKernelGGL(hybrid_coarse_cells_kernel, sgrid, dim3(64), 0, ctx->stream, ids, n_sats, (int32_t)pl.n_states, pl.n_coarse, center_hz, spread_hz, coherent_ms,
                       sc.hyb_level_cells.get());
    if (const int rc = launched(ctx)) return rc;
    const WeakCall call{iq_dev, stream_stride_samples, coherent_ms, n_blocks, flags, fine_step_hz, out_dev};
    for (int level = 0; level < (pl.fine_half >= 0 ? 2 : 1); ++level)
        if (const int rc = weak_level(ctx, call, pl, level)) return rc;
    // the coherent pass of the final bin over block 0, for the carrier phase at the code phase (the tap)
    if (const int rc = launch_cells(ctx, cells_params(ctx, iq_dev, stream_stride_samples, coherent_ms, sc.hyb_level_cells.get() + pl.coarse_cells + pl.fine_cells, (int32_t)pl.n_states,
                                                      sc.hyb_taps.get(), nullptr, nullptr, nullptr), GYP_COHERENT))
        return rc;
    hipLaunchKernelGGL(hybrid_finish_kernel, sgrid, dim3(64), 0, ctx->stream, (const gyp_cell*)sc.hyb_taps.get(), (int32_t)pl.n_states, out_dev);
    return launched(ctx);
}

int gyp_acquire_weak(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, int32_t coherent_ms, int32_t n_blocks, int32_t flags,
                     double center_hz, double spread_hz, double fine_step_hz, const int32_t* sat_ids_host, int32_t n_sats,
                     gyp_weak_result* out_host) {
    static const char* const who = "gyp_acquire_weak";
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    if (const int rc = hybrid_check(ctx, who, iq_host, out_host, n_streams, 0, coherent_ms, n_blocks, flags, sat_ids_host, n_sats)) return rc;
    return staged_call(ctx, iq_host, n_streams, n_blocks * coherent_ms, out_host, (size_t)n_streams * n_sats * sizeof(gyp_weak_result), [&](const float* iq_dev, int64_t stride, void* out_dev) {
        return gyp_acquire_weak_dev(ctx, iq_dev, n_streams, stride, coherent_ms, n_blocks, flags, center_hz, spread_hz, fine_step_hz, sat_ids_host, n_sats, (gyp_weak_result*)out_dev);
    });
}

// ---------------------------------------------------------------- tracking: explicit millisecond ----------
int gyp_track_step_dev(gyp_ctx* ctx, const float* iq_dev, int64_t stream_stride_samples, const double* start_time_dev,
                       const gyp_chan_in* chans_dev, int32_t n_chan, gyp_chan_out* out_dev, float* profile_out_dev) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    if (!iq_dev || !start_time_dev || !chans_dev || !out_dev || n_chan < 0) return fail(ctx, GYP_E_BAD_ARG, "gyp_track_step_dev: bad argument");
    if (n_chan == 0) return GYP_OK;
    TrackStepParams p;
    p.iq = reinterpret_cast<const cf*>(iq_dev);
    p.stream_stride = stream_stride_samples;
    p.start_time = start_time_dev;
    p.chans = chans_dev;
    p.n_chan = n_chan;
    p.out = out_dev;
    p.profile_out = profile_out_dev;
    p.replica_table = ctx->codes.replicas.get();
    p.tw_tables = ctx->codes.tw.get();
    p.inv_fs = 1.0 / (double)ctx->fs;
    p.trans = ctx->codes.trans.get();
    p.n_trans = ctx->codes.ntrans.get();
    p.chipf = ctx->codes.chipf.get();
    return launch_track_step(ctx, p);
}

int gyp_track_step(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, const double* start_time_host,
                   const gyp_chan_in* chans_host, int32_t n_chan, gyp_chan_out* out_host, float* profile_out_host) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    if (!iq_host || !start_time_host || !chans_host || !out_host || n_streams <= 0 || n_chan < 0)
        return fail(ctx, GYP_E_BAD_ARG, "gyp_track_step: bad argument");
    for (int i = 0; i < n_chan; ++i)
        if (chans_host[i].stream < 0 || chans_host[i].stream >= n_streams || chans_host[i].sat_id < 1 || chans_host[i].sat_id > 32)
            return fail(ctx, GYP_E_BAD_ARG, "gyp_track_step: channel descriptor out of range");
    if (n_chan == 0) return GYP_OK;
    Scratch& sc = ctx->scratch;
    const size_t out_bytes = (size_t)n_chan * sizeof(gyp_chan_out), n_prof = profile_out_host ? (size_t)n_chan * ctx->n : 0;
    HIP_TRY(ctx, sc.stage_out.reserve(out_bytes, Slack::grow, ctx->stream));
    HIP_TRY(ctx, sc.stage_profile.reserve(n_prof, Slack::grow, ctx->stream));
    HIP_TRY(ctx, upload(sc.stage_iq, iq_host, iq_floats(ctx, n_streams, 1), ctx->stream));
    HIP_TRY(ctx, upload(sc.stage_in, as_bytes(chans_host), (size_t)n_chan * sizeof(gyp_chan_in), ctx->stream));
    HIP_TRY(ctx, upload(sc.stage_times, start_time_host, (size_t)n_streams, ctx->stream));
    if (const int rc = gyp_track_step_dev(ctx, sc.stage_iq.get(), ctx->n, sc.stage_times.get(), (const gyp_chan_in*)sc.stage_in.get(), n_chan,
                                          (gyp_chan_out*)sc.stage_out.get(), profile_out_host ? sc.stage_profile.get() : nullptr))
        return rc;
    return stage_back(ctx, out_host, out_bytes, profile_out_host, n_prof);
}

// ---------------------------------------------------------------- tracking: device-resident loops --------
int gyp_bank_create(gyp_ctx* ctx, const gyp_chan_init* chans_host, int32_t n_chan, gyp_bank** out) {
    if (!ctx || !out) return GYP_E_BAD_ARG;
    *out = nullptr;
    if (const int rc = need_format(ctx)) return rc;
    if (!chans_host || n_chan <= 0) return fail(ctx, GYP_E_BAD_ARG, "gyp_bank_create: bad argument");
    std::vector<ChanState> init((size_t)n_chan);
    for (int i = 0; i < n_chan; ++i) {
        if (chans_host[i].stream < 0 || chans_host[i].sat_id < 1 || chans_host[i].sat_id > 32)
            return fail(ctx, GYP_E_BAD_ARG, "gyp_bank_create: channel descriptor out of range");
        init[i] = fresh_chan_state(chans_host[i]);
    }
    return bank_create(ctx, "gyp_bank_create", init, out, [](gyp_bank&) { return hipSuccess; });
}

void gyp_bank_destroy(gyp_bank* bank) {
    if (!bank) return;
    (void)hipStreamSynchronize(bank->ctx->stream);
    if (bank->verify_stream.get()) (void)hipStreamSynchronize(bank->verify_stream.get());
    delete bank;   // the members release what they hold: buffers and events first, the verify stream last
}

int gyp_bank_size(const gyp_bank* bank) { return bank ? bank->n_chan : GYP_E_BAD_ARG; }

int gyp_bank_set_channel(gyp_bank* bank, int32_t index, const gyp_chan_init* in) {
    if (!bank) return GYP_E_BAD_ARG;
    gyp_ctx* ctx = bank->ctx;
    if (!in || index < 0 || index >= bank->n_chan || in->stream < 0 || in->sat_id < 1 || in->sat_id > 32)
        return fail(ctx, GYP_E_BAD_ARG, "gyp_bank_set_channel: bad argument");
    return bank_put_state(bank, index, fresh_chan_state(*in));
}

int gyp_bank_drop_channel(gyp_bank* bank, int32_t index) {
    if (!bank) return GYP_E_BAD_ARG;
    gyp_ctx* ctx = bank->ctx;
    if (index < 0 || index >= bank->n_chan) return fail(ctx, GYP_E_BAD_ARG, "gyp_bank_drop_channel: index out of range");
    const int32_t one = 1;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(reinterpret_cast<char*>(bank->states.get() + index) + offsetof(ChanState, lost), &one, sizeof(one),
                           hipMemcpyHostToDevice));
    return GYP_OK;
}

// Block tracking (gyp_track_block_dev): track_plan says what the call runs, track_param_set builds every kernel's parameters once, and
// the flow states per launch only what differs (span_of, round_of, rerun_of).
// Buffers of the exact code loop (hand-over records, float64 discriminators, the loop's state), any tracking path.
static int ensure_dll_buffers(gyp_bank* bank, size_t n_rec) {
    gyp_ctx* ctx = bank->ctx;
    const hipStream_t s0 = ctx->stream, s1 = bank->verify_stream.get();
    HIP_TRY(ctx, bank->dllx.reserve((size_t)bank->n_chan, Slack::exact, s0, s1));
    HIP_TRY(ctx, bank->groups.reserve((size_t)bank->n_chan + 1, Slack::exact, s0, s1));
    HIP_TRY(ctx, bank->spec.reserve(n_rec, Slack::exact, s0, s1));
    HIP_TRY(ctx, bank->disc.reserve(n_rec, Slack::exact, s0, s1));
    return GYP_OK;
}

// The parameters of the four kernels behind a gyp_track_block_dev call (tracking, verification, exact sums, scan).
struct TrackParamSet { TrackBlockParams trk; TrackVerifyParams ver; DllExactParams sums; DllScanParams scan; };
// The channels the throughput kernel re-runs behind a speculative block: their flags, the checkpoints, each one's first sub-block, the exact code loop at the sub-block starts, the sub-blocks.
struct TrackRerun { const int32_t* bad; const ChanState* ckpt; const int32_t* bad_from; const DllExact* hist; SubLayout sub; };

// The set as launches over the whole block, every channel, need it (a plain throughput call's).  The bank's buffers have been reserved.
static TrackParamSet track_param_set(gyp_bank* bank, const TrackPlan& plan, const float* iq_dev, int64_t stream_stride_samples, int32_t n_ms,
                                     const double* start_time_dev, gyp_track_rec* rec_out_dev) {
    gyp_ctx* ctx = bank->ctx;
    TrackParamSet s{};   // (what is not set below is null / 0: no work list, no checkpoints, no rounds, no kept profiles)
    const auto block = [&](auto& x) -> auto& {   // the fields all four have
        x.iq = reinterpret_cast<const cf*>(iq_dev); x.stream_stride = stream_stride_samples; x.n_ms = n_ms; x.ms_begin = 0; x.ms_end = n_ms;
        x.start_time = start_time_dev; x.states = bank->states.get(); x.n_chan = bank->n_chan; x.inv_fs = 1.0 / (double)ctx->fs;
        x.sub = SubLayout::none();
        return x;
    };
    TrackBlockParams& p = block(s.trk);
    p.rec_out = rec_out_dev; p.replica_table = ctx->codes.replicas.get(); p.tw_tables = ctx->codes.tw.get(); p.fs = (double)ctx->fs;
    p.prof = ctx->prof.get(); p.prof_wave = ctx->prof_wave; p.finish_all = ctx->track_finish_all ? 1 : 0;
    p.codes = CodeTables{ctx->codes.trans.get(), ctx->codes.ntrans.get(), ctx->codes.chipf.get()};
    const gyp_params& g = ctx->params;
    // tracker.py:227-244: alpha = 4 zeta B dt, beta = 4 B^2 dt with zeta = 1/sqrt(2), dt = 1/fs, in the reference's order
    const double dt = 1.0 / (double)ctx->fs, bl = g.pll_bandwidth_locked_hz, bu = g.pll_bandwidth_unlocked_hz;
    p.lp = LoopParams{g.dll_gain, g.dll_phase_modulus, 4.0 * (1.0 / std::sqrt(2.0)) * bl * dt, 4.0 * (bl * bl) * dt,
                      4.0 * (1.0 / std::sqrt(2.0)) * bu * dt, 4.0 * (bu * bu) * dt,
                      g.lock_error_variance_max, g.lock_i_variance_max, g.lock_rotation_max_deg,
                      std::tan(g.lock_rotation_max_deg * M_PI / 180.0),
                      g.watchdog_period_s, g.watchdog_drop_below, g.watchdog_nudge_below, g.watchdog_nudge_hz, (double)ctx->n};
    p.spec_out = bank->spec.get(); p.spec_kappa = plan.spec_kappa; p.prov_bias = ctx->dll_prov_bias;
    p.exact0 = plan.flow == 1 ? bank->dllx.get() : nullptr;   // the throughput kernel leaves the code loop's state before the block here for dll_scan_kernel
    p.dbg = plan.flow != 1 && ctx->spec_debug ? bank->dbg.get() : nullptr;
    if (bank->prof_depth > 0) { p.prof_tail = bank->prof_tail.get(); p.prof_from = n_ms - bank->prof_rows; p.prof_depth = bank->prof_depth; }
    TrackVerifyParams& v = block(s.ver);
    v.spec = bank->spec.get(); v.rec_out = rec_out_dev; v.sub_index = 0; v.force_fail_ms = ctx->spec_fail_at;
    v.replica_table = ctx->codes.replicas.get(); v.tw_tables = ctx->codes.tw.get(); v.tie_tol = 4e-6f;
    DllExactParams& x = block(s.sums);
    x.spec = bank->spec.get(); x.disc_out = bank->disc.get(); x.chipf = ctx->codes.chipf.get();
    DllScanParams& d = block(s.scan);
    d.spec = bank->spec.get(); d.disc = bank->disc.get(); d.rec_out = rec_out_dev; d.exact = bank->dllx.get(); d.only_bad = 0;
    d.chipf = ctx->codes.chipf.get(); d.dll_gain = p.lp.dll_gain; d.dll_modulus = p.lp.dll_modulus; d.n_samples = p.lp.n_samples;
    d.first = 1; d.final = 1; d.symbol_tau = ctx->symbol_tau;
    d.prof_delta = p.prof_tail ? bank->prof_delta.get() : nullptr; d.prof_from = p.prof_from; d.prof_depth = p.prof_depth;
    return s;
}
// The launches cover [b, e) of every channel: sub-block j of flow 2, whose verification flags the channels that fail it and whose scan
// starts from the checkpoints -- or a chunk of the throughput kernel, which uses the tracking part alone.
static TrackParamSet span_of(const TrackParamSet& base, const gyp_bank* bank, int j, int b, int e) {
    TrackParamSet s = base;
    s.trk.ms_begin = s.ver.ms_begin = s.sums.ms_begin = s.scan.ms_begin = b;
    s.trk.ms_end = s.ver.ms_end = s.sums.ms_end = s.scan.ms_end = e;
    if (b > 0) s.trk.exact0 = nullptr;          // the code loop's state before the BLOCK is what dll_scan_kernel starts from
    s.scan.bad = s.ver.bad = bank->bad.get(); s.ver.bad_from = bank->bad_from.get(); s.ver.sub_index = j;
    s.scan.ckpt = bank->ckpt.get(); s.scan.first = b == 0 ? 1 : 0; s.scan.final = e == s.trk.n_ms ? 1 : 0;
    s.scan.hist_out = bank->hist.get() && e < s.trk.n_ms ? bank->hist.get() + (size_t)(j + 1) * bank->n_chan : nullptr;
    return s;
}
// Round R of the round protocol: every channel takes its own next sub-block (row R of the round tables; the spans are not used).
static TrackParamSet round_of(const TrackParamSet& base, const gyp_bank* bank, const TrackPlan& plan, int R) {
    TrackParamSet s = base;
    s.trk.ctl = bank->ctl.get(); s.trk.trk = bank->trk.get(); s.trk.fail = bank->fail.get(); s.trk.ckpt = bank->ckpt.get();
    s.trk.n_sub = plan.layout.n; s.trk.round = R; s.trk.exact_hist = bank->hist.get();
    s.trk.sub = s.ver.sub = s.sums.sub = s.scan.sub = plan.layout;
    s.ver.trk_round = s.sums.trk_round = s.scan.trk_round = bank->trk.get() + (size_t)R * bank->n_chan;
    s.ver.fail_round = bank->fail.get() + (size_t)R * bank->n_chan;
    s.scan.ckpt = bank->ckpt.get(); s.scan.hist = bank->hist.get(); s.scan.first = 0; s.scan.final = 0;
    return s;
}
// The re-run of the channels whose speculation failed verification: only they run, each from the checkpoint of the sub-block in which
// that happened, and the scan takes ONLY them.
static TrackParamSet rerun_of(const TrackParamSet& base, const gyp_bank* bank, const TrackRerun& r) {
    TrackParamSet s = base;
    s.trk.exact0 = bank->dllx.get(); s.trk.dbg = nullptr;
    s.trk.only_if = s.sums.only_if = s.scan.bad = r.bad; s.scan.only_bad = 1;
    s.trk.restore_from = r.ckpt; s.trk.exact_hist = r.hist;
    s.trk.from_sub = s.sums.from_sub = s.scan.from_sub = r.bad_from;
    s.trk.sub = s.sums.sub = s.scan.sub = r.sub;
    return s;
}

// The throughput tracking kernel with its code loop re-integrated exactly behind it (same stream).  rerun: behind a speculative
// block, for the channels whose speculation failed verification; null for a plain call.
static int track_block_throughput(gyp_bank* bank, const TrackParamSet& base, const TrackPlan& plan, const TrackRerun* rerun = nullptr) {
    gyp_ctx* ctx = bank->ctx;
    const TrackParamSet s = rerun ? rerun_of(base, bank, *rerun) : base;
    const int n_ms = s.trk.n_ms;
    int rc;
    const bool timed = ctx->time_track && !rerun;
    if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev_track[0].get(), ctx->stream));
    ctx->track_launches = plan.launches;
    for (int b0 = 0; b0 < n_ms; b0 += plan.chunk_ms)   // a launch boundary is a rendezvous of a stream's channels (track_plan)
        if ((rc = launch_track_block(ctx, span_of(s, bank, 0, b0, std::min(n_ms, b0 + plan.chunk_ms)).trk, 0))) return rc;
    if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev_track[1].get(), ctx->stream));
    bank->last_n_ms = n_ms;
    if ((rc = plan.exact_path == 2 ? launch_dll_exact_shared(ctx, s.sums, bank->groups.get(), ctx->stream) : launch_dll_exact(ctx, s.sums, ctx->stream))) return rc;
    if (!rerun) ctx->last_exact_path = plan.exact_path;
    if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev_track[2].get(), ctx->stream));
    if ((rc = launch_dll_scan(ctx, s.scan, ctx->stream))) return rc;
    if (timed) { HIP_TRY(ctx, hipEventRecord(ctx->ev_track[3].get(), ctx->stream)); ctx->track_timed = true; }
    return GYP_OK;
}

// Speculative block tracking (track_plan.hpp; everything is enqueued, nothing synchronises with the host).
//   flow 2, r03 form: every sub-block's verification trails its tracking on the verify stream; channels that failed one are re-run from
//   that sub-block's checkpoint by the TRANSFORM kernel afterwards.
//   flow 3, the round protocol (SpecCtl, kernels_track_block.hpp): round R's tracking launch on the context's stream, its verify /
//   exact-sums / scan launches on the verify stream behind it, launch R + 2 waiting for the verify kernels of round R.
// The prologue: the buffers, the tables of the flow cleared, gyp_debug_spec_redo_read's counters set.
static int spec_begin(gyp_bank* bank, const TrackPlan& plan, int n_ms) {
    gyp_ctx* ctx = bank->ctx;
    const size_t n_chan = (size_t)bank->n_chan, n_rec = n_chan * n_ms;
    const int n_sub = plan.layout.n, rounds = plan.rounds;
    // each resource under its own check: a HIP failure part way through leaves what exists in place for the retry
    HIP_TRY(ctx, bank->verify_stream.create(hipStreamNonBlocking));
    const hipStream_t s0 = ctx->stream, s1 = bank->verify_stream.get();
    HIP_TRY(ctx, bank->bad.reserve(n_chan, Slack::exact, s0, s1));
    HIP_TRY(ctx, bank->bad_from.reserve(n_chan, Slack::exact, s0, s1));
    HIP_TRY(ctx, bank->ctl.reserve(n_chan, Slack::exact, s0, s1));
    if (!bank->redo_stats.get()) {
        HIP_TRY(ctx, bank->redo_stats.reserve(4, Slack::exact));
        HIP_TRY(ctx, hipMemset(bank->redo_stats.get(), 0, 4 * sizeof(int32_t)));
    }
    HIP_TRY(ctx, bank->ev_spec.create(hipEventDisableTiming));
    HIP_TRY(ctx, bank->ev_verify.create(hipEventDisableTiming));
    for (Event& e : bank->ev_vring) HIP_TRY(ctx, e.create(hipEventDisableTiming));
    // state checkpoints and code-loop history: as many sub-blocks as this block uses; the round tables: as many rounds
    HIP_TRY(ctx, bank->ckpt.reserve((size_t)n_sub * n_chan, Slack::exact, s0, s1));
    HIP_TRY(ctx, bank->hist.reserve((size_t)(n_sub + 1) * n_chan, Slack::exact, s0, s1));
    HIP_TRY(ctx, bank->trk.reserve((size_t)rounds * n_chan, Slack::exact, s0, s1));
    HIP_TRY(ctx, bank->fail.reserve((size_t)rounds * n_chan, Slack::exact, s0, s1));
    if (const int rc = ensure_dll_buffers(bank, n_rec)) return rc;
    if (plan.flow == 2) {
        HIP_TRY(ctx, hipMemsetAsync(bank->bad.get(), 0, n_chan * sizeof(int32_t), ctx->stream));
        HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)bank->bad_from.get(), 0x7fffffff, n_chan, ctx->stream));
    } else {
        HIP_TRY(ctx, hipMemsetAsync(bank->ctl.get(), 0, n_chan * sizeof(SpecCtl), ctx->stream));   // cursor 0, nothing forced (rb_round 0 only ever matters for R = 1, which consults nothing)
        HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)bank->fail.get(), 0x7fffffff, (size_t)rounds * n_chan, ctx->stream));
        HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)bank->trk.get(), 0xffffffff, (size_t)rounds * n_chan, ctx->stream));
    }
    hipLaunchKernelGGL(set4_kernel, dim3(1), dim3(1), 0, ctx->stream, bank->redo_stats.get(), n_sub, plan.flow == 3 ? rounds : n_sub, 0, 0);
    if (ctx->spec_debug) HIP_TRY(ctx, bank->dbg.reserve(n_rec * 20, Slack::exact, ctx->stream));
    return GYP_OK;
}
// One step: the tracking launch on the context's stream; its verification, exact sums and scan behind it on the verify stream.
static int spec_step(gyp_bank* bank, const TrackParamSet& s) {
    gyp_ctx* ctx = bank->ctx;
    const hipStream_t vs = bank->verify_stream.get();
    int rc;
    if ((rc = launch_track_block(ctx, s.trk, 2))) return rc;
    HIP_TRY(ctx, hipEventRecord(bank->ev_spec.get(), ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(vs, bank->ev_spec.get(), 0));
    if ((rc = launch_track_verify(ctx, s.ver, vs))) return rc;
    if ((rc = launch_dll_exact(ctx, s.sums, vs))) return rc;
    return launch_dll_scan(ctx, s.scan, vs);
}

// An error between the first launch on the verify stream and the join leaves work enqueued there that reads the caller's IQ and writes
// the bank's buffers: it is waited out before the error reaches the caller (who may free either).
struct VerifyStreamGuard {
    gyp_bank* bank;
    bool armed = true;
    ~VerifyStreamGuard() {
        if (!armed) return;
        (void)hipStreamSynchronize(bank->verify_stream.get());
        (void)hipStreamSynchronize(bank->ctx->stream);
    }
};

static int track_block_speculative(gyp_bank* bank, const TrackParamSet& base, const TrackPlan& plan) {
    gyp_ctx* ctx = bank->ctx;
    const SubLayout& lay = plan.layout;
    const hipStream_t vs = bank->verify_stream.get();
    int rc;
    VerifyStreamGuard join_on_error{bank};
    if (plan.flow == 2) {
        for (int j = 0; j < lay.n; ++j) {
            HIP_TRY(ctx, hipMemcpyAsync(bank->ckpt.get() + (size_t)j * bank->n_chan, bank->states.get(), (size_t)bank->n_chan * sizeof(ChanState),
                                        hipMemcpyDeviceToDevice, ctx->stream));
            if ((rc = spec_step(bank, span_of(base, bank, j, lay.begin(j), lay.end(j, base.trk.n_ms))))) return rc;
        }
    } else {
        for (int R = 0; R < plan.rounds; ++R) {
            if (R >= 2) HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, bank->ev_vring[(R - 2) % 3].get(), 0));   // round R - 2's reports are in
            if ((rc = spec_step(bank, round_of(base, bank, plan, R)))) return rc;
            HIP_TRY(ctx, hipEventRecord(bank->ev_vring[R % 3].get(), vs));
        }
    }
    // the epilogue: the context's stream joins the verify stream, and the throughput kernel takes the channels the speculation did not finish
    HIP_TRY(ctx, hipEventRecord(bank->ev_verify.get(), vs));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, bank->ev_verify.get(), 0));
    join_on_error.armed = false;
    if (plan.flow == 2) {
        // gyp_debug_spec_redo_read's out4[3]: how many channels the transform kernel finishes (the round protocol's spec_finalize_kernel counts its own)
        hipLaunchKernelGGL(count_nonzero_kernel, dim3(1), dim3(64), 0, ctx->stream, bank->bad.get(), bank->n_chan, bank->redo_stats.get() + 3);
    } else {
        SpecFinalizeParams f;
        f.ctl = bank->ctl.get(); f.trk = bank->trk.get(); f.fail = bank->fail.get(); f.states = bank->states.get(); f.ckpt = bank->ckpt.get(); f.hist = bank->hist.get();
        f.exact = bank->dllx.get(); f.bad = bank->bad.get(); f.bad_from = bank->bad_from.get(); f.stats = bank->redo_stats.get();
        f.n_chan = bank->n_chan; f.n_sub = lay.n; f.rounds = plan.rounds;
        hipLaunchKernelGGL(spec_finalize_kernel, dim3((unsigned)bank->n_chan), dim3(256), 0, ctx->stream, f);
        HIP_TRY(ctx, hipGetLastError());
    }
    // flow 2: channels whose window maximum was not the global one somewhere (any count is handled), from the checkpoint of the sub-block in which that
    // happened; flow 3: channels the rounds did not finish (out of forced-transform slots or of rounds), from their last good checkpoint
    const TrackRerun rerun{bank->bad.get(), bank->ckpt.get(), bank->bad_from.get(), bank->hist.get(), lay};
    return track_block_throughput(bank, base, plan, &rerun);
}

int gyp_track_block_dev(gyp_bank* bank, const float* iq_dev, int64_t stream_stride_samples, int32_t n_ms,
                        const double* start_time_dev, gyp_track_rec* rec_out_dev) {
    if (!bank) return GYP_E_BAD_ARG;
    gyp_ctx* ctx = bank->ctx;
    if (!iq_dev || !start_time_dev || n_ms < 0) return fail(ctx, GYP_E_BAD_ARG, "gyp_track_block_dev: bad argument");
    if (bank->fs != ctx->fs || bank->n != ctx->n)
        return fail(ctx, GYP_E_BAD_ARG, "gyp_track_block: the bank was created for " + std::to_string(bank->fs) + " Hz / " + std::to_string(bank->n) +
                                            " samples per ms, the context is now set to " + std::to_string(ctx->fs) + " / " + std::to_string(ctx->n));
    if (n_ms == 0) return GYP_OK;
    const TrackPlan plan = ctx->last_track_plan = track_plan(TrackShape{ctx->k, ctx->n, ctx->n_cus, bank->n_chan, n_ms, bank->prof_depth > 0},
                                      TrackSwitches{ctx->no_pipe, ctx->no_spec, ctx->spec_redo, ctx->spec_sub_ms, ctx->track_chunk_ms, ctx->no_exact_shared, ctx->params.spec_confidence_kappa});
    if (bank->prof_depth > 0) {
        bank->prof_rows = std::min(bank->prof_depth, (int)n_ms);
        HIP_TRY(ctx, hipMemsetAsync(bank->prof_delta.get(), 0, (size_t)bank->n_chan * bank->prof_depth * sizeof(int32_t), ctx->stream));
    }
    if (const int rc = plan.flow == 1 ? ensure_dll_buffers(bank, (size_t)bank->n_chan * n_ms) : spec_begin(bank, plan, n_ms)) return rc;
    const TrackParamSet set = track_param_set(bank, plan, iq_dev, stream_stride_samples, n_ms, start_time_dev, rec_out_dev);
    return plan.flow == 1 ? track_block_throughput(bank, set, plan) : track_block_speculative(bank, set, plan);
}

int gyp_bank_keep_profiles(gyp_bank* bank, int32_t depth) {
    if (!bank) return GYP_E_BAD_ARG;
    gyp_ctx* ctx = bank->ctx;
    if (depth < 0 || depth > 4096) return fail(ctx, GYP_E_BAD_ARG, "gyp_bank_keep_profiles: depth must be in 0..4096");
    if (depth == bank->prof_depth) return GYP_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, bank->prof_tail.reset());
    HIP_TRY(ctx, bank->prof_delta.reset());
    bank->prof_depth = 0; bank->prof_rows = 0;
    if (depth == 0) return GYP_OK;
    const size_t rows = (size_t)bank->n_chan * depth;
    if (bank->prof_tail.reserve(rows * bank->n, Slack::exact) != hipSuccess) {
        (void)hipGetLastError();
        return fail(ctx, GYP_E_NOMEM, "gyp_bank_keep_profiles: " + std::to_string(rows * bank->n * sizeof(float)) + " bytes of profile rows do not fit");
    }
    HIP_TRY(ctx, bank->prof_delta.reserve(rows, Slack::exact));
    bank->prof_depth = depth;
    return GYP_OK;
}

int gyp_bank_read_profiles(gyp_bank* bank, int32_t channel, float* out, int32_t* n_rows_out) {
    if (!bank || !n_rows_out) return GYP_E_BAD_ARG;
    gyp_ctx* ctx = bank->ctx;
    if (channel < 0 || channel >= bank->n_chan) return fail(ctx, GYP_E_BAD_ARG, "gyp_bank_read_profiles: no such channel");
    *n_rows_out = bank->prof_rows;
    if (!out || bank->prof_rows == 0) return GYP_OK;
    const int n = bank->n, rows = bank->prof_rows;
    std::vector<float> raw((size_t)rows * n);
    std::vector<int32_t> delta(rows);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(raw.data(), bank->prof_tail.get() + (size_t)channel * bank->prof_depth * n, raw.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(delta.data(), bank->prof_delta.get() + (size_t)channel * bank->prof_depth, rows * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int r = 0; r < rows; ++r) {
        // the row is roll(c0, -s_provisional); the reference's is roll(c0, -s_exact): out[k] = row[(k + s_exact - s_provisional) mod n]
        const int d = ((delta[r] % n) + n) % n;
        const float* row = raw.data() + (size_t)r * n;
        std::memcpy(out + (size_t)r * n, row + d, (size_t)(n - d) * sizeof(float));
        if (d) std::memcpy(out + (size_t)r * n + (n - d), row, (size_t)d * sizeof(float));
    }
    return GYP_OK;
}

int gyp_track_block(gyp_bank* bank, const float* iq_host, int32_t n_streams, int32_t n_ms, const double* start_time_host,
                    gyp_track_rec* rec_out_host) {
    if (!bank) return GYP_E_BAD_ARG;
    gyp_ctx* ctx = bank->ctx;
    if (!iq_host || !start_time_host || n_streams <= 0 || n_ms < 0) return fail(ctx, GYP_E_BAD_ARG, "gyp_track_block: bad argument");
    if (const int rc = bank_covers(*bank, "gyp_track_block", n_streams)) return rc;
    if (n_ms == 0) return GYP_OK;
    Scratch& sc = ctx->scratch;
    const size_t rec_bytes = rec_out_host ? (size_t)bank->n_chan * n_ms * sizeof(gyp_track_rec) : 0;
    HIP_TRY(ctx, sc.stage_out.reserve(rec_bytes, Slack::grow, ctx->stream));
    HIP_TRY(ctx, upload(sc.stage_iq, iq_host, iq_floats(ctx, n_streams, n_ms), ctx->stream));
    HIP_TRY(ctx, upload(sc.stage_times, start_time_host, (size_t)n_ms, ctx->stream));
    if (const int rc = gyp_track_block_dev(bank, sc.stage_iq.get(), (int64_t)n_ms * ctx->n, n_ms, sc.stage_times.get(),
                                           rec_out_host ? (gyp_track_rec*)sc.stage_out.get() : nullptr))
        return rc;
    return stage_back(ctx, rec_out_host, rec_bytes);
}

// ---------------------------------------------------------------- weak-signal tracking ---------------------
}   // extern "C"
// A weak bank: the channels' states and the SYNC prompt rows, device resident; the cursor and the parameters on the host.
struct gyp_weak_bank : BankBase {
    int64_t cursor = 0;          // absolute index of the next millisecond
    gyp_weak_params prm{};
    DevBuf<WeakChan> states;         // [n_chan]
    DevBuf<float2> sync_prompts;     // [n_chan][sync_ms]
};
static int weak_get_chan(gyp_weak_bank* bank, int32_t index, WeakChan* s) {
    gyp_ctx* ctx = bank->ctx;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(s, bank->states.get() + index, sizeof(WeakChan), hipMemcpyDeviceToHost));
    return GYP_OK;
}
// What both forms of gyp_weak_track_block refuse, before anything runs.
static int weak_track_check(gyp_weak_bank* bank, const char* who, const void* iq, int64_t first_ms, int32_t n_ms) {
    gyp_ctx* ctx = bank->ctx;
    if (!iq) return refuse(ctx, who, "bad argument");
    if (n_ms < 1 || n_ms > kWeakMaxMs) return refuse(ctx, who, "n_ms must be 1..65535");
    if (ctx->fs != bank->fs || ctx->n != bank->n) return refuse(ctx, who, "the context's stream format is not the one the bank was created under");
    if (first_ms != bank->cursor)
        return refuse(ctx, who, "first_ms " + std::to_string(first_ms) + " is not the bank's cursor " + std::to_string(bank->cursor));
    return GYP_OK;
}
extern "C" {

void gyp_weak_params_default(gyp_weak_params* out) {
    if (out) *out = weak_params_default();
}

int gyp_weak_bit_sync(const float* prompts, int32_t n_ms, int64_t first_ms, double* energies_out20, int32_t* offset_out) {
    if (!prompts || n_ms < kWeakPeriodMs || first_ms < 0) return fail(nullptr, GYP_E_BAD_ARG, "gyp_weak_bit_sync: bad argument");
    double en[kWeakPeriodMs];
    for (int o = 0; o < kWeakPeriodMs; ++o) en[o] = weak_bit_energy(prompts, n_ms, first_ms, o);
    if (energies_out20) std::memcpy(energies_out20, en, sizeof(en));
    if (offset_out) *offset_out = weak_bit_pick(en);
    return GYP_OK;
}

int gyp_weak_bank_create(gyp_ctx* ctx, const gyp_chan_init* chans_host, int32_t n_chan, const gyp_weak_params* params, int64_t first_ms,
                         gyp_weak_bank** out) {
    static const char* const who = "gyp_weak_bank_create";
    if (!ctx || !out) return GYP_E_BAD_ARG;
    *out = nullptr;
    if (const int rc = need_format(ctx)) return rc;
    if (!chans_host || n_chan < 1 || first_ms < 0) return refuse(ctx, who, "bad argument");
    const gyp_weak_params prm = params ? *params : weak_params_default();
    if (const char* why = weak_params_refusal(prm)) return refuse(ctx, who, why);
    std::vector<WeakChan> init((size_t)n_chan);
    for (int i = 0; i < n_chan; ++i) {
        if (const char* why = weak_init_refusal(chans_host[i])) return refuse(ctx, who, why);
        init[i] = weak_fresh_chan(chans_host[i], ctx->n, first_ms);
    }
    return bank_create(ctx, who, init, out, [&](gyp_weak_bank& b) {
        b.cursor = first_ms; b.prm = prm;
        return b.sync_prompts.reserve(init.size() * (size_t)prm.sync_ms, Slack::exact);
    });
}

void gyp_weak_bank_destroy(gyp_weak_bank* bank) {
    if (!bank) return;
    (void)hipStreamSynchronize(bank->ctx->stream);
    delete bank;
}

int gyp_weak_bank_size(const gyp_weak_bank* bank) { return bank ? bank->n_chan : GYP_E_BAD_ARG; }

int gyp_weak_bank_set_channel(gyp_weak_bank* bank, int32_t index, const gyp_chan_init* in) {
    static const char* const who = "gyp_weak_bank_set_channel";
    if (!bank) return GYP_E_BAD_ARG;
    if (!in || index < 0 || index >= bank->n_chan) return refuse(bank->ctx, who, "bad argument");
    if (const char* why = weak_init_refusal(*in)) return refuse(bank->ctx, who, why);
    return bank_put_state(bank, index, weak_fresh_chan(*in, bank->n, bank->cursor));
}

int gyp_weak_bank_drop_channel(gyp_weak_bank* bank, int32_t index) {
    if (!bank) return GYP_E_BAD_ARG;
    if (index < 0 || index >= bank->n_chan) return refuse(bank->ctx, "gyp_weak_bank_drop_channel", "index out of range");
    WeakChan s;
    if (const int rc = weak_get_chan(bank, index, &s)) return rc;
    s.status = 2;
    return bank_put_state(bank, index, s);
}

int gyp_weak_bank_get_state(gyp_weak_bank* bank, gyp_weak_state* out_host, int64_t* cursor_out) {
    if (!bank) return GYP_E_BAD_ARG;
    gyp_ctx* ctx = bank->ctx;
    if (cursor_out) *cursor_out = bank->cursor;
    if (!out_host) return GYP_OK;
    std::vector<WeakChan> s((size_t)bank->n_chan);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(s.data(), bank->states.get(), s.size() * sizeof(WeakChan), hipMemcpyDeviceToHost));
    for (int i = 0; i < bank->n_chan; ++i) {
        gyp_weak_state o{};
        o.f = s[i].f; o.f_int = s[i].f_int; o.u0 = s[i].u0; o.c0 = s[i].c0;
        o.phase = s[i].phase; o.edge = s[i].edge; o.status = s[i].status; o.pos = s[i].pos; o.n_periods = s[i].n_periods;
        o.mu_mean = s[i].mu_mean;
        out_host[i] = o;
    }
    return GYP_OK;
}

int gyp_weak_bank_set_state(gyp_weak_bank* bank, int32_t index, const gyp_weak_state* in) {
    static const char* const who = "gyp_weak_bank_set_state";
    if (!bank) return GYP_E_BAD_ARG;
    gyp_ctx* ctx = bank->ctx;
    if (!in || index < 0 || index >= bank->n_chan) return refuse(ctx, who, "bad argument");
    if (!std::isfinite(in->f) || !std::isfinite(in->f_int) || !(in->u0 >= 0.0 && in->u0 < 1.0) || in->c0 < 0 || in->c0 >= kWeakCodeMod ||
        in->edge < 0 || in->edge >= kWeakPeriodMs)
        return refuse(ctx, who, "state out of range");
    WeakChan s;
    if (const int rc = weak_get_chan(bank, index, &s)) return rc;
    WeakChan t{};
    t.stream = s.stream; t.sat_id = s.sat_id;
    t.phase = kWeakWait; t.edge = in->edge; t.sync_start = bank->cursor;
    t.f = in->f; t.f_int = in->f_int; t.u0 = in->u0; t.c0 = in->c0;
    return bank_put_state(bank, index, t);
}

int gyp_weak_track_block_dev(gyp_weak_bank* bank, const float* iq_dev, int64_t stream_stride_samples, int64_t first_ms, int32_t n_ms,
                             gyp_weak_ms_rec* ms_out_dev, gyp_weak_period_rec* period_out_dev, int32_t* n_periods_out_dev) {
    static const char* const who = "gyp_weak_track_block_dev";
    if (!bank) return GYP_E_BAD_ARG;
    gyp_ctx* ctx = bank->ctx;
    if (const int rc = weak_track_check(bank, who, iq_dev, first_ms, n_ms)) return rc;
    if (stream_stride_samples < (int64_t)n_ms * bank->n) return refuse(ctx, who, "the stream stride is below n_ms * N");
    WeakTrackParams p{};
    p.states = bank->states.get(); p.sync_prompts = bank->sync_prompts.get();
    p.iq = iq_dev; p.stream_stride = stream_stride_samples; p.chips = ctx->codes.chips.get();
    p.ms_out = ms_out_dev; p.period_out = period_out_dev; p.n_periods_out = n_periods_out_dev;
    p.prm = bank->prm; p.fs = (double)bank->fs; p.first_ms = first_ms;
    p.n = bank->n; p.n_ms = n_ms; p.n_chan = bank->n_chan;
    hipLaunchKernelGGL(weak_track_kernel, dim3((unsigned)bank->n_chan), dim3(kWeakThreads), 0, ctx->stream, p);
    if (const int rc = launched(ctx)) return rc;
    bank->cursor += n_ms;
    return GYP_OK;
}

int gyp_weak_track_block(gyp_weak_bank* bank, const float* iq_host, int32_t n_streams, int64_t first_ms, int32_t n_ms,
                         gyp_weak_ms_rec* ms_out_host, gyp_weak_period_rec* period_out_host, int32_t* n_periods_out_host) {
    static const char* const who = "gyp_weak_track_block";
    if (!bank) return GYP_E_BAD_ARG;
    gyp_ctx* ctx = bank->ctx;
    if (n_streams < 1) return refuse(ctx, who, "bad argument");
    if (const int rc = weak_track_check(bank, who, iq_host, first_ms, n_ms)) return rc;
    if (const int rc = bank_covers(*bank, who, n_streams)) return rc;
    Scratch& sc = ctx->scratch;
    const size_t nc = (size_t)bank->n_chan, max_periods = (size_t)n_ms / kWeakPeriodMs + 1;
    const size_t ms_bytes = nc * n_ms * sizeof(gyp_weak_ms_rec), per_bytes = nc * max_periods * sizeof(gyp_weak_period_rec), cnt_bytes = nc * sizeof(int32_t);
    HIP_TRY(ctx, sc.weak_stage.reserve(ms_bytes + per_bytes + cnt_bytes, Slack::grow, ctx->stream));
    HIP_TRY(ctx, upload(sc.stage_iq, iq_host, iq_floats(ctx, n_streams, n_ms), ctx->stream));
    uint8_t* const base = sc.weak_stage.get();
    if (const int rc = gyp_weak_track_block_dev(bank, sc.stage_iq.get(), (int64_t)n_ms * ctx->n, first_ms, n_ms, (gyp_weak_ms_rec*)base,
                                                (gyp_weak_period_rec*)(base + ms_bytes), (int32_t*)(base + ms_bytes + per_bytes)))
        return rc;
    if (ms_out_host) HIP_TRY(ctx, hipMemcpyAsync(ms_out_host, base, ms_bytes, hipMemcpyDeviceToHost, ctx->stream));
    // the period rows and their counts in one copy; only the records written go on to the caller (the rest of each row stays as it was)
    std::vector<uint8_t> staged(period_out_host || n_periods_out_host ? per_bytes + cnt_bytes : 0);
    if (!staged.empty()) HIP_TRY(ctx, hipMemcpyAsync(staged.data(), base + ms_bytes, staged.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (staged.empty()) return GYP_OK;
    const int32_t* const cnt = reinterpret_cast<const int32_t*>(staged.data() + per_bytes);
    if (n_periods_out_host) std::memcpy(n_periods_out_host, cnt, cnt_bytes);
    if (period_out_host)
        for (size_t c = 0; c < nc; ++c)
            if (cnt[c] > 0)
                std::memcpy(period_out_host + c * max_periods, staged.data() + c * max_periods * sizeof(gyp_weak_period_rec),
                            (size_t)cnt[c] * sizeof(gyp_weak_period_rec));
    return GYP_OK;
}

// ---------------------------------------------------------------- weak-signal hand-over --------------------
void gyp_weak_refine_params_default(gyp_weak_refine_params* out) {
    if (out) *out = refine_params_default();
}

int gyp_weak_refine_estimate(const float* prompts, int32_t n_ms, int64_t first_ms, const gyp_weak_refine_params* params, gyp_weak_refined* out) {
    static const char* const who = "gyp_weak_refine_estimate";
    if (!prompts || !out) return refuse(nullptr, who, "bad argument");
    const gyp_weak_refine_params prm = params ? *params : refine_params_default();
    if (const char* why = refine_refusal(prm, n_ms, first_ms)) return refuse(nullptr, who, why);
    gyp_weak_refined r{};
    refine_estimate(prompts, n_ms, first_ms, prm, 0.0, 0.0, &r);
    *out = r;
    return GYP_OK;
}

}   // extern "C"
// What both forms of gyp_weak_refine refuse, before anything runs (stride < 0: the host form, which has none).
static int weak_refine_check(gyp_ctx* ctx, const char* who, const void* iq, const void* out, int32_t n_streams, int64_t stream_stride_samples,
                             int64_t first_ms, int32_t n_ms, const gyp_weak_result* results, int32_t n_results, const gyp_weak_refine_params& prm) {
    if (!iq || !out || !results || n_streams < 1 || n_results < 1) return refuse(ctx, who, "bad argument");
    if (const char* why = refine_refusal(prm, n_ms, first_ms)) return refuse(ctx, who, why);
    if (stream_stride_samples >= 0 && stream_stride_samples < (int64_t)n_ms * ctx->n) return refuse(ctx, who, "the stream stride is below n_ms * N");
    if ((int64_t)n_results * ((n_ms + kRefineWaves - 1) / kRefineWaves) > INT32_MAX) return refuse(ctx, who, "more than 2^31 - 1 workgroups");
    for (int32_t i = 0; i < n_results; ++i) {
        const gyp_weak_result& r = results[i];
        const gyp_chan_init in{r.stream, r.sat_id, r.doppler_hz, r.carrier_phase, r.code_phase, 0};
        if (const char* why = weak_init_refusal(in)) return refuse(ctx, who, why);
        if (r.stream >= n_streams)
            return refuse(ctx, who, "result " + std::to_string(i) + " reads stream " + std::to_string(r.stream) + " but only " + std::to_string(n_streams) + " were passed");
        if (r.code_phase < 0 || r.code_phase >= ctx->n) return refuse(ctx, who, "a code phase is outside [0, N)");
    }
    return GYP_OK;
}
extern "C" {

int gyp_weak_refine_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int64_t first_ms, int32_t n_ms,
                        const gyp_weak_result* results_host, int32_t n_results, const gyp_weak_refine_params* params,
                        gyp_weak_refined* out_dev, float* prompts_out_dev) {
    static const char* const who = "gyp_weak_refine_dev";
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    const gyp_weak_refine_params prm = params ? *params : refine_params_default();
    if (stream_stride_samples < 0) return refuse(ctx, who, "bad argument");
    if (const int rc = weak_refine_check(ctx, who, iq_dev, out_dev, n_streams, stream_stride_samples, first_ms, n_ms, results_host, n_results, prm)) return rc;
    const RefineShape sh = refine_shape(prm, n_ms);
    std::vector<WeakRefineCand> cands((size_t)n_results);
    for (int32_t i = 0; i < n_results; ++i) {
        const gyp_weak_result& r = results_host[i];
        const WeakChan s = weak_fresh_chan(gyp_chan_init{r.stream, r.sat_id, r.doppler_hz, r.carrier_phase, r.code_phase, 0}, ctx->n, first_ms);
        cands[i] = WeakRefineCand{r.stream, r.sat_id, r.code_phase, 0, s.f, s.u0, r.carrier_phase, s.c0};
    }
    Scratch& sc = ctx->scratch;
    const size_t rows = (size_t)n_results * (size_t)n_ms;
    HIP_TRY(ctx, sc.wref_plans.reserve(rows, Slack::grow, ctx->stream));
    if (!prompts_out_dev) HIP_TRY(ctx, sc.wref_prompts.reserve(rows, Slack::grow, ctx->stream));
    HIP_TRY(ctx, sc.wref_power.reserve((size_t)n_results * (size_t)sh.n_bins, Slack::grow, ctx->stream));
    HIP_TRY(ctx, upload(sc.wref_cands, cands.data(), cands.size(), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the candidates are a temporary
    WeakRefineArgs p{};
    p.cands = sc.wref_cands.get(); p.plans = sc.wref_plans.get();
    p.prompts = prompts_out_dev ? reinterpret_cast<float2*>(prompts_out_dev) : sc.wref_prompts.get();
    p.power = sc.wref_power.get();
    p.iq = iq_dev; p.stream_stride = stream_stride_samples; p.chips = ctx->codes.chips.get();
    p.out = out_dev; p.prm = prm; p.fs = (double)ctx->fs; p.first_ms = first_ms;
    p.n = ctx->n; p.n_ms = n_ms; p.n_cand = n_results;
    hipLaunchKernelGGL(weak_refine_plan_kernel, dim3((unsigned)((n_results + 63) / 64)), dim3(64), 0, ctx->stream, p);
    if (const int rc = launched(ctx)) return rc;
    const unsigned runs = (unsigned)((n_ms + kRefineWaves - 1) / kRefineWaves);
    hipLaunchKernelGGL(weak_refine_sums_kernel, dim3((unsigned)n_results * runs), dim3(kRefineThreads), 0, ctx->stream, p);
    if (const int rc = launched(ctx)) return rc;
    hipLaunchKernelGGL(weak_refine_estimate_kernel, dim3((unsigned)n_results), dim3(kRefineEstThreads), 0, ctx->stream, p);
    return launched(ctx);
}

int gyp_weak_refine(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, int64_t first_ms, int32_t n_ms,
                    const gyp_weak_result* results_host, int32_t n_results, const gyp_weak_refine_params* params,
                    gyp_weak_refined* out_host, float* prompts_out_host) {
    static const char* const who = "gyp_weak_refine";
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    const gyp_weak_refine_params prm = params ? *params : refine_params_default();
    if (const int rc = weak_refine_check(ctx, who, iq_host, out_host, n_streams, -1, first_ms, n_ms, results_host, n_results, prm)) return rc;
    Scratch& sc = ctx->scratch;
    const size_t rec_bytes = (size_t)n_results * sizeof(gyp_weak_refined), prompt_bytes = (size_t)n_results * (size_t)n_ms * sizeof(float2);
    HIP_TRY(ctx, sc.stage_out.reserve(rec_bytes + prompt_bytes, Slack::grow, ctx->stream));
    HIP_TRY(ctx, upload(sc.stage_iq, iq_host, iq_floats(ctx, n_streams, n_ms), ctx->stream));
    uint8_t* const base = sc.stage_out.get();
    if (const int rc = gyp_weak_refine_dev(ctx, sc.stage_iq.get(), n_streams, (int64_t)n_ms * ctx->n, first_ms, n_ms, results_host, n_results, &prm,
                                           (gyp_weak_refined*)base, (float*)(base + rec_bytes)))
        return rc;
    if (prompts_out_host) HIP_TRY(ctx, hipMemcpyAsync(prompts_out_host, base + rec_bytes, prompt_bytes, hipMemcpyDeviceToHost, ctx->stream));
    return stage_back(ctx, out_host, rec_bytes);
}

// ---------------------------------------------------------------- weak-signal measurement ------------------
void gyp_weak_measure_params_default(gyp_weak_measure_params* out) {
    if (out) *out = measure_params_default();
}

int gyp_weak_measure_estimate(const gyp_weak_ms_rec* sums, const double* w, int32_t n_ms, int64_t first_ms, int32_t edge, int64_t spacing,
                              int64_t c0, gyp_weak_measure_fold* out) {
    static const char* const who = "gyp_weak_measure_estimate";
    if (!sums || !w || !out) return refuse(nullptr, who, "bad argument");
    gyp_weak_measure_params prm = measure_params_default();
    prm.spacing = spacing;
    if (const char* why = measure_refusal(prm, n_ms, first_ms)) return refuse(nullptr, who, why);
    if (const char* why = measure_edge_refusal(edge, n_ms, first_ms)) return refuse(nullptr, who, why);
    if (c0 < 0 || c0 >= kWeakCodeMod) return refuse(nullptr, who, "c0 is outside [0, 1023 * 2^40)");
    *out = measure_estimate(sums, w, n_ms, first_ms, edge, spacing, c0);
    return GYP_OK;
}

int gyp_weak_measured_state(const gyp_weak_measured* rec, int64_t fs, int32_t samples_per_ms, int32_t ms_ahead, gyp_weak_state* out) {
    static const char* const who = "gyp_weak_measured_state";
    if (!rec || !out) return refuse(nullptr, who, "bad argument");
    if (fs < 1) return refuse(nullptr, who, "fs must be positive");
    if (samples_per_ms < 1023 || samples_per_ms % 1023 != 0) return refuse(nullptr, who, "N must be a positive multiple of 1023");
    if (ms_ahead < 0 || ms_ahead > kWeakMaxMs) return refuse(nullptr, who, "ms_ahead must be 0..65535");
    if (!std::isfinite(rec->doppler_hz)) return refuse(nullptr, who, "a Doppler is not finite");
    if (!std::isfinite(rec->carrier_phase)) return refuse(nullptr, who, "a carrier phase is not finite");
    if (rec->c0 < 0 || rec->c0 >= kWeakCodeMod) return refuse(nullptr, who, "c0 is outside [0, 1023 * 2^40)");
    if (rec->edge < 0 || rec->edge >= kWeakPeriodMs) return refuse(nullptr, who, "an edge is outside 0..19");
    *out = measure_state(*rec, (double)fs, samples_per_ms, ms_ahead);
    return GYP_OK;
}

}   // extern "C"
// What both forms of gyp_weak_measure refuse, before anything runs (stride < 0: the host form, which has none).
static int weak_measure_check(gyp_ctx* ctx, const char* who, const void* iq, const void* out, int32_t n_streams, int64_t stream_stride_samples,
                              int64_t first_ms, int32_t n_ms, const gyp_weak_refined* refined, int32_t n_results, const gyp_weak_measure_params& prm) {
    if (!iq || !out || !refined || n_streams < 1 || n_results < 1) return refuse(ctx, who, "bad argument");
    if (const char* why = measure_refusal(prm, n_ms, first_ms)) return refuse(ctx, who, why);
    if (stream_stride_samples >= 0 && stream_stride_samples < (int64_t)n_ms * ctx->n) return refuse(ctx, who, "the stream stride is below n_ms * N");
    if ((int64_t)n_results * ((n_ms + kMeasureWaves - 1) / kMeasureWaves) > INT32_MAX) return refuse(ctx, who, "more than 2^31 - 1 workgroups");
    for (int32_t i = 0; i < n_results; ++i) {
        const gyp_weak_refined& r = refined[i];
        if (const char* why = measure_cand_refusal(r, ctx->n, n_ms, first_ms)) return refuse(ctx, who, why);
        if (r.stream >= n_streams)
            return refuse(ctx, who, "candidate " + std::to_string(i) + " reads stream " + std::to_string(r.stream) + " but only " + std::to_string(n_streams) + " were passed");
    }
    return GYP_OK;
}
// Where a pass's rows of sums (or W_m) go: the caller's array is [candidate][pass][n_ms], the scratch [candidate][n_ms].
template <typename T>
static WeakMeasureRows<T> weak_measure_rows(T* callers, T* scratch, int32_t passes, int32_t pass) {
    return callers ? WeakMeasureRows<T>{callers, passes, pass} : WeakMeasureRows<T>{scratch, 1, 0};
}
extern "C" {

int gyp_weak_measure_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int64_t first_ms, int32_t n_ms,
                         const gyp_weak_refined* refined_host, int32_t n_results, const gyp_weak_measure_params* params,
                         gyp_weak_measured* out_dev, gyp_weak_ms_rec* sums_out_dev, double* w_out_dev, gyp_weak_measure_fold* folds_out_dev) {
    static const char* const who = "gyp_weak_measure_dev";
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    const gyp_weak_measure_params prm = params ? *params : measure_params_default();
    if (stream_stride_samples < 0) return refuse(ctx, who, "bad argument");
    if (const int rc = weak_measure_check(ctx, who, iq_dev, out_dev, n_streams, stream_stride_samples, first_ms, n_ms, refined_host, n_results, prm)) return rc;
    std::vector<WeakMeasureCand> cands((size_t)n_results);
    for (int32_t i = 0; i < n_results; ++i) {
        const gyp_weak_refined& r = refined_host[i];
        const WeakChan s = weak_fresh_chan(gyp_chan_init{r.stream, r.sat_id, r.doppler_hz, r.carrier_phase, r.code_phase, 0}, ctx->n, first_ms);
        cands[i] = WeakMeasureCand{r.stream, r.sat_id, r.edge, 0, s.f, s.u0, r.carrier_phase, s.c0};
    }
    Scratch& sc = ctx->scratch;
    const size_t rows = (size_t)n_results * (size_t)n_ms;
    HIP_TRY(ctx, sc.wmeas_plans.reserve(rows, Slack::grow, ctx->stream));
    HIP_TRY(ctx, sc.wmeas_states.reserve((size_t)n_results, Slack::grow, ctx->stream));
    if (!sums_out_dev) HIP_TRY(ctx, sc.wmeas_sums.reserve(rows, Slack::grow, ctx->stream));
    if (!w_out_dev) HIP_TRY(ctx, sc.wmeas_w.reserve(rows, Slack::grow, ctx->stream));
    HIP_TRY(ctx, upload(sc.wmeas_cands, cands.data(), cands.size(), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // the candidates are a temporary
    WeakMeasureArgs p{};
    p.cands = sc.wmeas_cands.get(); p.states = sc.wmeas_states.get(); p.plans = sc.wmeas_plans.get();
    p.folds = folds_out_dev;
    p.iq = iq_dev; p.stream_stride = stream_stride_samples; p.chips = ctx->codes.chips.get();
    p.out = out_dev; p.spacing = prm.spacing; p.fs = (double)ctx->fs; p.first_ms = first_ms;
    p.n = ctx->n; p.n_ms = n_ms; p.n_cand = n_results; p.passes = prm.passes;
    const unsigned runs = (unsigned)((n_ms + kMeasureWaves - 1) / kMeasureWaves);
    for (int32_t pass = 0; pass < prm.passes; ++pass) {
        p.pass = pass;
        // the sums and the W_m each go to the caller's row of this pass, or to the one scratch row a candidate has
        p.sums = weak_measure_rows(sums_out_dev, sc.wmeas_sums.get(), prm.passes, pass);
        p.w = weak_measure_rows(w_out_dev, sc.wmeas_w.get(), prm.passes, pass);
        hipLaunchKernelGGL(weak_measure_plan_kernel, dim3((unsigned)((n_results + 63) / 64)), dim3(64), 0, ctx->stream, p);
        if (const int rc = launched(ctx)) return rc;
        hipLaunchKernelGGL(weak_measure_sums_kernel, dim3((unsigned)n_results * runs), dim3(kMeasureThreads), 0, ctx->stream, p);
        if (const int rc = launched(ctx)) return rc;
        hipLaunchKernelGGL(weak_measure_fold_kernel, dim3((unsigned)n_results), dim3(kMeasureFoldThreads), 0, ctx->stream, p);
        if (const int rc = launched(ctx)) return rc;
    }
    return GYP_OK;
}

int gyp_weak_measure(gyp_ctx* ctx, const float* iq_host, int32_t n_streams, int64_t first_ms, int32_t n_ms,
                     const gyp_weak_refined* refined_host, int32_t n_results, const gyp_weak_measure_params* params,
                     gyp_weak_measured* out_host, gyp_weak_ms_rec* sums_out_host, double* w_out_host, gyp_weak_measure_fold* folds_out_host) {
    static const char* const who = "gyp_weak_measure";
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    const gyp_weak_measure_params prm = params ? *params : measure_params_default();
    if (const int rc = weak_measure_check(ctx, who, iq_host, out_host, n_streams, -1, first_ms, n_ms, refined_host, n_results, prm)) return rc;
    // the staged results: the records, then what was asked for of the sums, the W_m and the folds, back to back (all multiples of 8 bytes)
    const size_t rows = (size_t)n_results * (size_t)prm.passes * (size_t)n_ms;
    const size_t rec_bytes = (size_t)n_results * sizeof(gyp_weak_measured), sums_bytes = sums_out_host ? rows * sizeof(gyp_weak_ms_rec) : 0;
    const size_t w_bytes = w_out_host ? rows * sizeof(double) : 0, fold_bytes = folds_out_host ? (size_t)n_results * prm.passes * sizeof(gyp_weak_measure_fold) : 0;
    std::vector<uint8_t> staged(rec_bytes + sums_bytes + w_bytes + fold_bytes);
    const int rc = staged_call(ctx, iq_host, n_streams, n_ms, staged.data(), staged.size(), [&](const float* iq_dev, int64_t stride, void* out_dev) {
        uint8_t* const base = static_cast<uint8_t*>(out_dev);
        return gyp_weak_measure_dev(ctx, iq_dev, n_streams, stride, first_ms, n_ms, refined_host, n_results, &prm, (gyp_weak_measured*)base,
                                    sums_bytes ? (gyp_weak_ms_rec*)(base + rec_bytes) : nullptr, w_bytes ? (double*)(base + rec_bytes + sums_bytes) : nullptr,
                                    fold_bytes ? (gyp_weak_measure_fold*)(base + rec_bytes + sums_bytes + w_bytes) : nullptr);
    });
    if (rc) return rc;
    std::memcpy(out_host, staged.data(), rec_bytes);
    if (sums_bytes) std::memcpy(sums_out_host, staged.data() + rec_bytes, sums_bytes);
    if (w_bytes) std::memcpy(w_out_host, staged.data() + rec_bytes + sums_bytes, w_bytes);
    if (fold_bytes) std::memcpy(folds_out_host, staged.data() + rec_bytes + sums_bytes + w_bytes, fold_bytes);
    return GYP_OK;
}

// ---------------------------------------------------------------- multi-GPU: one all-gather over RCCL ------
// the only exchange of the path is one all-gather of fixed-size result records per batch.  RCCL is
// resolved at run time (dlopen of the librccl the process already has, e.g. torch's, else the system one), so the
// library loads -- and every single-GPU entry point works -- on hosts without it.

int gyp_comm_unique_id(void* out_128_bytes) {
    if (!out_128_bytes) return GYP_E_BAD_ARG;
    if (!rccl_load()) return fail(nullptr, GYP_E_COMM, g_rccl.err);
    const int rc = g_rccl.GetUniqueId(out_128_bytes);
    if (rc != 0) return fail(nullptr, GYP_E_COMM, rccl_msg("ncclGetUniqueId", rc));
    return GYP_OK;
}

int gyp_comm_init(gyp_ctx* ctx, int32_t rank, int32_t world, const void* unique_id_128_bytes) {
    if (!ctx || world < 1 || rank < 0 || rank >= world) return ctx ? fail(ctx, GYP_E_BAD_ARG, "gyp_comm_init: bad rank / world") : GYP_E_BAD_ARG;
    if (ctx->comm) return fail(ctx, GYP_E_BAD_ARG, "gyp_comm_init: the context already has a communicator");
    if (!unique_id_128_bytes) {
        if (world != 1) return fail(ctx, GYP_E_BAD_ARG, "gyp_comm_init: a unique id is required for world > 1");
        ctx->comm_rank = 0; ctx->comm_world = 1;      // single process, no RCCL: gyp_allgather_dev is a device copy
        return GYP_OK;
    }
    if (!rccl_load()) return fail(ctx, GYP_E_COMM, g_rccl.err);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    RcclApi::Id id;
    std::memcpy(id.b, unique_id_128_bytes, sizeof(id.b));
    void* comm = nullptr;
    const int rc = g_rccl.CommInitRank(&comm, world, id, rank);
    if (rc != 0) return fail(ctx, GYP_E_COMM, rccl_msg("ncclCommInitRank", rc));
    ctx->comm = comm; ctx->comm_rank = rank; ctx->comm_world = world;
    return GYP_OK;
}

int gyp_comm_destroy(gyp_ctx* ctx) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (ctx->comm) {
        (void)hipStreamSynchronize(ctx->stream);
        const int rc = g_rccl.CommDestroy(ctx->comm);
        ctx->comm = nullptr;
        if (rc != 0) return fail(ctx, GYP_E_COMM, rccl_msg("ncclCommDestroy", rc));
    }
    ctx->comm_rank = 0; ctx->comm_world = 1;
    return GYP_OK;
}

int gyp_comm_info(gyp_ctx* ctx, int32_t* rank, int32_t* world, int32_t* uses_rccl) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (rank) *rank = ctx->comm_rank;
    if (world) *world = ctx->comm_world;
    if (uses_rccl) *uses_rccl = ctx->comm ? 1 : 0;
    return GYP_OK;
}

int gyp_allgather_dev(gyp_ctx* ctx, const void* send_dev, void* recv_dev, uint64_t bytes_per_rank) {
    if (!ctx || (!send_dev && bytes_per_rank) || (!recv_dev && bytes_per_rank)) return ctx ? fail(ctx, GYP_E_BAD_ARG, "gyp_allgather_dev: bad argument") : GYP_E_BAD_ARG;
    if (bytes_per_rank == 0) return GYP_OK;
    if (!ctx->comm) {
        if (ctx->comm_world != 1) return fail(ctx, GYP_E_COMM, "gyp_allgather_dev: no communicator");
        if (send_dev != recv_dev)
            HIP_TRY(ctx, hipMemcpyAsync(recv_dev, send_dev, bytes_per_rank, hipMemcpyDeviceToDevice, ctx->stream));
        return GYP_OK;
    }
    // enqueued on the context's stream, behind the kernels that produce the records: no host synchronisation
    const int rc = g_rccl.AllGather(send_dev, recv_dev, (size_t)bytes_per_rank, /* ncclInt8 */ 0, ctx->comm, ctx->stream);
    if (rc != 0) return fail(ctx, GYP_E_COMM, rccl_msg("ncclAllGather", rc));
    return GYP_OK;
}

// ---------------------------------------------------------------- host staging helpers -----------------------
int gyp_host_alloc(gyp_ctx* ctx, uint64_t bytes, void** out) {
    if (!ctx || !out) return GYP_E_BAD_ARG;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) return fail(ctx, GYP_E_NOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    return GYP_OK;
}

int gyp_host_free(gyp_ctx* ctx, void* p) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (p) HIP_TRY(ctx, hipHostFree(p));
    return GYP_OK;
}

int gyp_debug_spec_read(gyp_bank* bank, float* out, int32_t n_floats, int32_t* bad_out) {
    if (!bank) return GYP_E_BAD_ARG;
    gyp_ctx* ctx = bank->ctx;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (out && bank->dbg.get()) HIP_TRY(ctx, hipMemcpy(out, bank->dbg.get(), std::min((size_t)n_floats, bank->dbg.capacity()) * sizeof(float), hipMemcpyDeviceToHost));
    if (bad_out && bank->bad.get()) HIP_TRY(ctx, hipMemcpy(bad_out, bank->bad.get(), (size_t)bank->n_chan * sizeof(int32_t), hipMemcpyDeviceToHost));
    return GYP_OK;
}

int gyp_debug_spec_layout(int32_t n_ms, int32_t* starts_out) { return gyp_debug_spec_layout_for(n_ms, 500, starts_out); }
int gyp_debug_spec_layout_for(int32_t n_ms, int32_t sub_ms, int32_t* starts_out) {
    if (n_ms <= 0 || sub_ms < 100 || sub_ms > 2000 || !starts_out) return GYP_E_BAD_ARG;
    const SubLayout l = spec_layout(n_ms, sub_ms);
    for (int i = 0; i <= l.n; ++i) starts_out[i] = l.start[i];
    return l.n;
}

int gyp_debug_spec_redo_read(gyp_bank* bank, int32_t* out4) {
    if (!bank || !out4) return GYP_E_BAD_ARG;
    gyp_ctx* ctx = bank->ctx;
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    if (!bank->redo_stats.get()) return GYP_OK;   // the bank has not tracked a block on the speculative path
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(out4, bank->redo_stats.get(), 4 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return GYP_OK;
}

int gyp_debug_dll_read(gyp_bank* bank, int32_t* repairs_out) {
    if (!bank || !repairs_out) return GYP_E_BAD_ARG;
    gyp_ctx* ctx = bank->ctx;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<DllExact> x((size_t)bank->n_chan);
    for (int i = 0; i < bank->n_chan; ++i) repairs_out[i] = 0;
    if (!bank->dllx.get()) return GYP_OK;          // the bank has not tracked a block yet
    HIP_TRY(ctx, hipMemcpy(x.data(), bank->dllx.get(), x.size() * sizeof(DllExact), hipMemcpyDeviceToHost));
    for (int i = 0; i < bank->n_chan; ++i) repairs_out[i] = x[i].repairs;
    return GYP_OK;
}

int gyp_debug_disc_read(gyp_bank* bank, int32_t n_ms, double* disc_out) {
    if (!bank) return GYP_E_BAD_ARG;
    gyp_ctx* ctx = bank->ctx;
    if (!disc_out || n_ms <= 0 || n_ms != bank->last_n_ms || !bank->disc.get() || !bank->spec.get())
        return fail(ctx, GYP_E_BAD_ARG, "gyp_debug_disc_read: n_ms must be the length of the bank's last block on the throughput path");
    const size_t n_rec = (size_t)bank->n_chan * n_ms;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<SpecIn> spec(n_rec);
    HIP_TRY(ctx, hipMemcpy(disc_out, bank->disc.get(), n_rec * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(spec.data(), bank->spec.get(), n_rec * sizeof(SpecIn), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n_rec; ++i)
        if (spec[i].key == kSpecKeyLost) disc_out[i] = 0.0;   // not processed: the pass wrote nothing there
    return GYP_OK;
}

int gyp_bank_reset_dev(gyp_bank* bank, const gyp_chan_init* inits_dev) {
    if (!bank) return GYP_E_BAD_ARG;
    gyp_ctx* ctx = bank->ctx;
    if (!inits_dev) return fail(ctx, GYP_E_BAD_ARG, "gyp_bank_reset_dev: bad argument");
    hipLaunchKernelGGL(bank_reset_kernel, dim3((bank->n_chan + 63) / 64), dim3(64), 0, ctx->stream, bank->states.get(), inits_dev, bank->n_chan);
    HIP_TRY(ctx, hipGetLastError());
    return GYP_OK;
}

int gyp_bank_get_state(gyp_bank* bank, double* doppler_hz, double* carrier_phase, int32_t* code_phase, int32_t* lost) {
    if (!bank) return GYP_E_BAD_ARG;
    gyp_ctx* ctx = bank->ctx;
    std::vector<ChanState> host((size_t)bank->n_chan);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(host.data(), bank->states.get(), host.size() * sizeof(ChanState), hipMemcpyDeviceToHost));
    for (int i = 0; i < bank->n_chan; ++i) {
        if (doppler_hz) doppler_hz[i] = host[i].doppler;
        if (carrier_phase) carrier_phase[i] = host[i].carrier_phase;
        if (code_phase) code_phase[i] = host[i].code_phase;
        if (lost) lost[i] = host[i].lost;
    }
    return GYP_OK;
}

// ---------------------------------------------------------------- synthetic IQ ----------------------------
int gyp_synth_iq_dev(gyp_ctx* ctx, float* out_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t n_ms,
                     const gyp_synth_sat* sats_host, int32_t n_sats, float noise_sigma, uint64_t seed) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    if (!out_dev || !sats_host || n_streams <= 0 || n_ms <= 0 || n_ms > 65535 || n_sats < 0)
        return fail(ctx, GYP_E_BAD_ARG, "gyp_synth_iq_dev: bad argument (n_ms must be 1..65535)");
    for (int i = 0; i < n_streams * n_sats; ++i)
        if (sats_host[i].sat_id < 1 || sats_host[i].sat_id > 32 || sats_host[i].code_phase < 0 || sats_host[i].code_phase >= ctx->n)
            return fail(ctx, GYP_E_BAD_ARG, "gyp_synth_iq_dev: satellite descriptor out of range");
    const size_t n_scene = (size_t)n_streams * n_sats;
    HIP_TRY(ctx, upload(ctx->scratch.synth_scene, sats_host, n_scene, ctx->stream, n_scene ? 0 : 1));
    SynthParams p;
    p.out = reinterpret_cast<cf*>(out_dev);
    p.stream_stride = stream_stride_samples;
    p.n_ms = n_ms;
    p.n_per_ms = ctx->n;
    p.k = ctx->k;
    p.n_sats = n_sats;
    p.sats = ctx->scratch.synth_scene.get();
    p.chips = ctx->codes.chips.get();
    p.sigma = noise_sigma;
    p.seed = seed;
    p.inv_fs = 1.0 / (double)ctx->fs;
    hipLaunchKernelGGL(synth_iq_kernel, dim3((ctx->n + 255) / 256, n_ms, n_streams), dim3(256), 0, ctx->stream, p);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // sats_host may be a temporary
    return GYP_OK;
}

// A/B switches and test hooks of a context, by name.  The library reads no environment variable for them (a stray variable in
// a deployment must not change the speed path): whoever wants one says so through this call.  Values are range-checked (kDebugSwitches).

// The values gyp_debug_get reads and nobody sets (what the last call of its kind did): GYP_OK, GYP_E_HIP, or GYP_E_BAD_ARG if `name` is none.
static int debug_read_only(gyp_ctx* ctx, const char* name, double* out) {
    auto is = [&](const char* n) { return std::strcmp(name, n) == 0; };
    if (is("last_grid_refined_rows")) { *out = (double)ctx->last_grid_refined_rows; return GYP_OK; }
    if (is("last_grid_path")) { *out = (double)ctx->last_grid_plan.path; return GYP_OK; }
    if (is("last_track_flow")) { *out = (double)ctx->last_track_plan.flow; return GYP_OK; }
    if (is("last_exact_path")) { *out = (double)ctx->last_exact_path; return GYP_OK; }
    if (is("last_acq_lanes")) { *out = (double)ctx->last_acq_plan.lanes; return GYP_OK; }
    if (is("last_acq_levels")) { *out = (double)ctx->last_acq_plan.n_levels; return GYP_OK; }
    if (is("last_acq_shared_levels")) { *out = (double)ctx->last_acq_plan.shared_levels; return GYP_OK; }
    if (is("last_hybrid_chunks")) { *out = (double)ctx->last_hybrid_plan.n_chunks; return GYP_OK; }
    for (int w = 0; w < 3; ++w) {
        // "last_acq_units" etc.: summed over the levels of the last search; with "_l<k>" appended: its level k alone (1 .. kAcqWitnessLevels)
        static const char* const kWitness[3] = {"last_acq_units", "last_acq_shared_cells", "last_acq_unshared_cells"};
        const size_t len = std::strlen(kWitness[w]);
        if (std::strncmp(name, kWitness[w], len) != 0) continue;
        int at = w;
        if (name[len] != 0) {
            char* end = nullptr;
            const long k = name[len] == '_' && name[len + 1] == 'l' && name[len + 2] >= '1' && name[len + 2] <= '9' ? std::strtol(name + len + 2, &end, 10) : 0;
            if (k < 1 || k > kAcqWitnessLevels || !end || *end != 0) continue;
            at = 3 * (int)k + w;
        }
        // the one place the counters are waited for and copied: this context's part of the last search plus the helpers' parts
        long long total = 0;
        for (int i = 0; i < ctx->last_acq_plan.lanes; ++i) {
            gyp_ctx* c = i == 0 ? ctx : ctx->helper[i - 1];
            if (!c || !c->acq_witness.get()) continue;
            int32_t v = 0;
            if (hipStreamSynchronize(c->stream) != hipSuccess) return GYP_E_HIP;
            if (hipMemcpy(&v, c->acq_witness.get() + at, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess) return GYP_E_HIP;
            total += v;
        }
        *out = (double)total;
        return GYP_OK;
    }
    return GYP_E_BAD_ARG;
}
static const DebugSwitch* debug_switch(const char* name) {
    for (const DebugSwitch& k : kDebugSwitches)
        if (std::strcmp(name, k.name) == 0) return &k;
    return nullptr;
}
int gyp_debug_set(gyp_ctx* ctx, const char* name, double value) {
    if (!ctx || !name) return GYP_E_BAD_ARG;
    const DebugSwitch* k = debug_switch(name);
    if (!k) return fail(ctx, GYP_E_BAD_ARG, std::string("gyp_debug_set: no such switch: ") + name);
    if (!std::isfinite(value) || value < k->lo || value > k->hi || (k->integral && value != std::floor(value)))
        return fail(ctx, GYP_E_BAD_ARG, std::string("gyp_debug_set: ") + name + " must be " + (k->integral ? "an integer " : "") + "in [" +
                                            std::to_string(k->lo) + ", " + std::to_string(k->hi) + "]");
    if (std::strcmp(name, "track_chunk_ms") == 0 && value != 0.0 && value < 20.0)
        return fail(ctx, GYP_E_BAD_ARG, "gyp_debug_set: track_chunk_ms must be 0 (whole blocks) or at least 20");
    if (std::strcmp(name, "grid_fused_waves") == 0 && value != 8.0 && value != 12.0)
        return fail(ctx, GYP_E_BAD_ARG, "gyp_debug_set: grid_fused_waves must be 8 or 12");
    k->set(*ctx, value);
    return GYP_OK;
}
int gyp_debug_get(gyp_ctx* ctx, const char* name, double* out) {
    if (!ctx || !name || !out) return GYP_E_BAD_ARG;
    if (const DebugSwitch* k = debug_switch(name)) { *out = k->get(*ctx); return GYP_OK; }
    const int rc = debug_read_only(ctx, name, out);
    if (rc == GYP_E_HIP) return fail(ctx, rc, std::string("gyp_debug_get: reading the device counters of ") + name + " failed");
    if (rc != GYP_OK) return fail(ctx, GYP_E_BAD_ARG, std::string("gyp_debug_get: no such switch: ") + name);
    return GYP_OK;
}

int gyp_debug_track_profile(gyp_ctx* ctx, int enable, long long* out8) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (enable && !ctx->prof.get()) {
        HIP_TRY(ctx, ctx->prof.reserve(16, Slack::exact));
        HIP_TRY(ctx, hipMemset(ctx->prof.get(), 0, 16 * sizeof(long long)));
    }
    if (out8 && ctx->prof.get()) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, hipMemcpy(out8, ctx->prof.get(), 16 * sizeof(long long), hipMemcpyDeviceToHost));
    }
    if (!enable) HIP_TRY(ctx, ctx->prof.reset());
    return GYP_OK;
}

int gyp_debug_track_timing(gyp_ctx* ctx, int enable, float* out4) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (enable)
        for (Event& e : ctx->ev_track) HIP_TRY(ctx, e.create(hipEventDefault));
    if (out4) {
        out4[0] = out4[1] = out4[2] = out4[3] = 0.0f;   // (a bank on the speculative path: no per-kernel split, zeros)
        if (ctx->time_track && ctx->track_timed) {
            HIP_TRY(ctx, hipEventSynchronize(ctx->ev_track[3].get()));
            for (int i = 0; i < 3; ++i) HIP_TRY(ctx, hipEventElapsedTime(out4 + i, ctx->ev_track[i].get(), ctx->ev_track[i + 1].get()));
            out4[3] = (float)ctx->track_launches;
        }
    }
    if (out4 || !enable || !ctx->time_track) ctx->track_timed = false;   // a reading belongs to the one call before it
    ctx->time_track = enable != 0;
    return GYP_OK;
}

int gyp_debug_fft_bench(gyp_ctx* ctx, int waves_per_wg, int wgs, int iters, float* ms_out) {
    if (!ctx || !ms_out) return GYP_E_BAD_ARG;
    if (const int rc = need_format(ctx)) return rc;
    HIP_TRY(ctx, ctx->scratch.bench_sink.reserve((size_t)wgs * 1024, Slack::grow, ctx->stream));
    float* sink = ctx->scratch.bench_sink.get();
    for (int rep = 0; rep < 2; ++rep) {
        HIP_TRY(ctx, hipEventRecord(ctx->ev0.get(), ctx->stream));
        const auto bench = [&](auto w) {
            constexpr int W = decltype(w)::value;
            return launch_dyn(ctx, fft_bench_kernel<W>, dim3(wgs), dim3(64 * W), lds_bytes<W>(), ctx->stream, ctx->codes.tw.get(), ctx->codes.replicas.get(), iters, sink);
        };
        int rc;
        switch (waves_per_wg) {
            case 1: rc = bench(std::integral_constant<int, 1>{}); break;
            case 2: rc = bench(std::integral_constant<int, 2>{}); break;
            case 4: rc = bench(std::integral_constant<int, 4>{}); break;
            case 8: rc = bench(std::integral_constant<int, 8>{}); break;
            default: return fail(ctx, GYP_E_BAD_ARG, "waves_per_wg must be 1, 2, 4 or 8");
        }
        if (rc) return rc;
        HIP_TRY(ctx, hipEventRecord(ctx->ev1.get(), ctx->stream));
        HIP_TRY(ctx, hipEventSynchronize(ctx->ev1.get()));
        HIP_TRY(ctx, hipEventElapsedTime(ms_out, ctx->ev0.get(), ctx->ev1.get()));
    }
    return GYP_OK;
}

int gyp_synth_nav_bit(uint64_t seed, int32_t stream, int32_t sat_id, int32_t nav_bit_offset_ms, int64_t ms) {
    return synth_nav_bit(seed, stream, sat_id, nav_bit_offset_ms, ms);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// navigation bits (host only)
// ---------------------------------------------------------------------------------------------------------
struct gyp_bits {
    std::vector<gyp_bits_impl::Channel> chans;
    std::deque<gyp_bit_event> fifo;
};

static int bits_take(gyp_bits* b, gyp_bit_event* out, int32_t cap, int32_t* n_out) {
    int32_t n = 0;
    if (out)
        while (n < cap && !b->fifo.empty()) {
            out[n++] = b->fifo.front();
            b->fifo.pop_front();
        }
    if (n_out) *n_out = n;
    return GYP_OK;
}

extern "C" {

int gyp_bits_create(int32_t n_channels, gyp_bits** out) {
    if (!out) return fail(nullptr, GYP_E_BAD_ARG, "gyp_bits_create: out is NULL");
    *out = nullptr;
    if (n_channels <= 0) return fail(nullptr, GYP_E_BAD_ARG, "gyp_bits_create: n_channels must be positive");
    gyp_bits* b = new (std::nothrow) gyp_bits();
    if (!b) return fail(nullptr, GYP_E_NOMEM, "gyp_bits_create: out of memory");
    b->chans.resize(n_channels);
    *out = b;
    return GYP_OK;
}

void gyp_bits_destroy(gyp_bits* bits) { delete bits; }

int gyp_bits_reset(gyp_bits* bits, int32_t channel) {
    if (!bits) return fail(nullptr, GYP_E_BAD_ARG, "gyp_bits_reset: bits is NULL");
    if (channel < -1 || channel >= (int32_t)bits->chans.size())
        return fail(nullptr, GYP_E_BAD_ARG, "gyp_bits_reset: channel out of range");
    for (int32_t c = 0; c < (int32_t)bits->chans.size(); ++c)
        if (channel < 0 || c == channel) bits->chans[c].reset();
    return GYP_OK;
}

int gyp_bits_push(gyp_bits* bits, int32_t channel, int32_t n, const double* receiver_timestamp,
                  const double* start_of_pseudosymbol, const double* end_of_pseudosymbol,
                  const int8_t* pseudosymbol, int32_t* cursor_at_emit_out, gyp_bit_event* events_out,
                  int32_t capacity, int32_t* n_events_out) {
    if (n_events_out) *n_events_out = 0;
    if (!bits) return fail(nullptr, GYP_E_BAD_ARG, "gyp_bits_push: bits is NULL");
    if (channel < 0 || channel >= (int32_t)bits->chans.size())
        return fail(nullptr, GYP_E_BAD_ARG, "gyp_bits_push: channel out of range");
    if (n < 0 || capacity < 0 || (n > 0 && (!receiver_timestamp || !start_of_pseudosymbol || !end_of_pseudosymbol || !pseudosymbol)))
        return fail(nullptr, GYP_E_BAD_ARG, "gyp_bits_push: bad arguments");
    for (int32_t i = 0; i < n; ++i)   // NavigationBitPseudosymbol.from_val raises KeyError on anything else
        if (pseudosymbol[i] != 1 && pseudosymbol[i] != -1)
            return fail(nullptr, GYP_E_BAD_ARG, "gyp_bits_push: pseudosymbol " + std::to_string(i) + " is not -1/+1");
    gyp_bits_impl::Channel& ch = bits->chans[channel];
    auto sink = [&](const gyp_bits_impl::BitOut& o) {
        bits->fifo.push_back(gyp_bit_event{o.start, o.end, channel, o.bit});
    };
    for (int32_t i = 0; i < n; ++i) {
        const int64_t at = ch.process(receiver_timestamp[i],
                                      gyp_bits_impl::Symbol{start_of_pseudosymbol[i], end_of_pseudosymbol[i], pseudosymbol[i]}, sink);
        if (cursor_at_emit_out) cursor_at_emit_out[i] = (int32_t)at;
    }
    return bits_take(bits, events_out, capacity, n_events_out);
}

int gyp_bits_push_block(gyp_bits* bits, const gyp_track_rec* recs_host, int32_t n_chan, int32_t n_ms,
                        const double* start_time, const double* end_time, gyp_bit_event* events_out,
                        int32_t capacity, int32_t* n_events_out) {
    if (n_events_out) *n_events_out = 0;
    if (!bits) return fail(nullptr, GYP_E_BAD_ARG, "gyp_bits_push_block: bits is NULL");
    if (n_chan < 0 || n_chan > (int32_t)bits->chans.size() || n_ms < 0 || capacity < 0)
        return fail(nullptr, GYP_E_BAD_ARG, "gyp_bits_push_block: bad sizes");
    if (n_chan * (int64_t)n_ms > 0 && (!recs_host || !start_time || !end_time))
        return fail(nullptr, GYP_E_BAD_ARG, "gyp_bits_push_block: NULL input");
    std::vector<int32_t> live_ms(n_chan, n_ms);   // first ms with status != 0, per channel
    for (int32_t c = 0; c < n_chan; ++c)
        for (int32_t t = 0; t < n_ms; ++t) {
            const gyp_track_rec& r = recs_host[(size_t)c * n_ms + t];
            if (r.status != 0) { live_ms[c] = t; break; }
            if (r.pseudosymbol != 1 && r.pseudosymbol != -1)
                return fail(nullptr, GYP_E_BAD_ARG, "gyp_bits_push_block: channel " + std::to_string(c) + " ms " +
                                                        std::to_string(t) + ": pseudosymbol is not -1/+1");
        }
    for (int32_t t = 0; t < n_ms; ++t)
        for (int32_t c = 0; c < n_chan; ++c) {
            if (t >= live_ms[c]) continue;
            const gyp_track_rec& r = recs_host[(size_t)c * n_ms + t];
            // tracker.py:319-326: the pseudosymbol's edges are the chunk's plus the code-phase delay
            const double delay = (static_cast<double>(r.code_phase) / 2046.0) * 0.001;
            bits->chans[c].process(start_time[t], gyp_bits_impl::Symbol{start_time[t] + delay, end_time[t] + delay, r.pseudosymbol},
                                   [&](const gyp_bits_impl::BitOut& o) {
                                       bits->fifo.push_back(gyp_bit_event{o.start, o.end, c, o.bit});
                                   });
        }
    return bits_take(bits, events_out, capacity, n_events_out);
}

int gyp_bits_drain(gyp_bits* bits, gyp_bit_event* events_out, int32_t capacity, int32_t* n_events_out) {
    if (n_events_out) *n_events_out = 0;
    if (!bits || capacity < 0) return fail(nullptr, GYP_E_BAD_ARG, "gyp_bits_drain: bad arguments");
    return bits_take(bits, events_out, capacity, n_events_out);
}

int gyp_bits_get_state(const gyp_bits* bits, int32_t channel, gyp_bits_state* out) {
    if (!bits || !out) return fail(nullptr, GYP_E_BAD_ARG, "gyp_bits_get_state: NULL argument");
    if (channel < 0 || channel >= (int32_t)bits->chans.size())
        return fail(nullptr, GYP_E_BAD_ARG, "gyp_bits_get_state: channel out of range");
    const gyp_bits_impl::Channel& ch = bits->chans[channel];
    std::memset(out, 0, sizeof(*out));
    out->determined_bit_phase = ch.determined_bit_phase;
    out->previous_bit_phase_decision = ch.previous_bit_phase_decision;
    out->sequential_unknown_bit_value_counter = ch.sequential_unknown;
    out->queued_pseudosymbols = (int32_t)ch.queue.size();
    out->pseudosymbol_cursor_within_queue = ch.cursor;
    out->slide = ch.slide;
    out->failed_bit_count = ch.failed_bit_count;
    out->emitted_bit_count = ch.emitted_bit_count;
    out->processed_pseudosymbol_count = ch.processed;
    out->last_emitted_bits_len = ch.bits_len;
    for (int i = 0; i < ch.bits_len; ++i)
        out->last_emitted_bits[i] = ch.bits[(ch.bits_head + i) % gyp_bits_impl::kBitHistory];
    return GYP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// IQ ingest
// ---------------------------------------------------------------------------------------------------------
#include "ingest.hpp"

// ---------------------------------------------------------------------------------------------------------
// Resampler (kernels_resample.hpp): fs_in recordings -> the stream format
// ---------------------------------------------------------------------------------------------------------
// The design for (fs_in, the context's rate, T, input kind), built and uploaded on first use.  A copy: the context owns d_taps' memory.
static int resample_cached_design(gyp_ctx* ctx, int64_t fs_in, int32_t T, bool real, ResampleDesign* out) {
    for (const auto& cached : ctx->resample_designs)
        if (const ResampleDesign& d = cached.first; d.fs_in == fs_in && d.fs_out == ctx->fs && d.taps == T && d.real == real) {
            *out = d;
            return GYP_OK;
        }
    ResampleDesign d;
    static_cast<ResampleRatio&>(d) = resample_ratio(fs_in, ctx->fs);
    d.fs_in = fs_in;
    d.fs_out = ctx->fs;
    d.taps = T;
    d.real = real;
    std::vector<float> rows((size_t)d.L * T), cols((size_t)d.L * T);
    resample_design_rows(fs_in, ctx->fs, T, d.L, rows.data());
    for (int32_t p = 0; p < d.L; ++p) {   // the kernel's layout: column p holds phase p's taps (design row p*M mod L)
        const int64_t row = (int64_t)p * d.M % d.L;
        for (int32_t j = 0; j < T; ++j) cols[(size_t)j * d.L + p] = rows[(size_t)row * T + j];
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf<float> taps;
    HIP_TRY(ctx, upload(taps, cols.data(), cols.size(), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // `cols` is a temporary
    d.d_taps = taps.get();
    ctx->resample_designs.emplace_back(d, std::move(taps));
    *out = d;
    return GYP_OK;
}

static const char* const kResampleTapsRule = ": taps must be 0 (32), 16, 24, 32, 48 or 64";
static const char* const kDdcTapsRule = ": taps must be 0 (auto), 32, 48, 64, 96 or 128";
static const char* const kDdcRateRule = ": rates must be whole kHz with fs_in < 2^31 Hz and 8 fs_out >= fs_in, and the IF must satisfy "
                                        "20 |if| >= 9 fs_out and 20 |if| + 9 fs_out <= 10 fs_in";

// The design that takes fs_in recordings to the context's rate: the resampler's (I,Q words), or with `real` the down-converter's
// (real words at if_hz).  Refuses in this order: no stream format, the tap count, the rates.
static int filter_design(gyp_ctx* ctx, int64_t fs_in, bool real, int64_t if_hz, int32_t taps, ResampleDesign* out, const char* who) {
    if (!ctx->fs) return fail(ctx, GYP_E_NO_FORMAT, std::string(who) + ": " + kNoFormat);
    if (real ? taps && !ddc_taps(taps, 0, 0) : !resample_taps(taps))
        return fail(ctx, GYP_E_BAD_ARG, std::string(who) + (real ? kDdcTapsRule : kResampleTapsRule));
    if (real ? !ddc_rates_ok(fs_in, ctx->fs, if_hz) : !resample_rates_ok(fs_in, ctx->fs))
        return fail(ctx, GYP_E_BAD_RATE, std::string(who) + (real ? kDdcRateRule : ": fs_in must be a positive multiple of 1000 Hz, differ from the "
                                                                                   "stream format's rate and lie within a factor 2 of it"));
    return resample_cached_design(ctx, fs_in, real ? ddc_taps(taps, fs_in, ctx->fs) : resample_taps(taps), real, out);
}

// One call of the sample path, by name: the words, the window of them the caller holds, the scale, the output window.
struct RawWindow {
    const void* raw;        // stream 0's words
    int64_t stride;         // between streams: in SAMPLES for word formats, in BYTES for packed ones
    int64_t first, n;       // the buffer holds input samples first .. first+n-1 (the unpacker: samples 0 .. n-1); zeros outside
    int32_t bit0;           // packed words: the buffer's sample 0 starts bit0 bits into its first byte; else 0
};
struct OutWindow {
    float* iq;              // stream 0's complex64 samples
    int64_t stride;         // between streams, in samples
    int64_t first_ms;       // output milliseconds first_ms .. first_ms+n_ms-1 (the unpacker: in.n samples) ...
    int32_t n_ms, n_streams;   // ... of n_streams streams
};
struct SampleRequest {
    int32_t fmt;            // GYP_FMT_* words, unless ...
    const PackedFormat* pk; // ... set: packed words of this format
    int64_t if_hz;          // real words (the design's kind says so) are mixed down from it; I,Q words: 0
    float scale;
    RawWindow in;
    OutWindow out;
};

template <class S, int TT>
static void resample_launch_one(hipStream_t stream, const ResampleDesign& d, const SampleRequest& rq, const ResampleTiling& tl,
                                const typename S::Params& prm) {
    S stage;
    static_cast<typename S::Params&>(stage) = prm;
    const dim3 grid((unsigned)tl.n_tiles, (unsigned)rq.out.n_streams);
    hipLaunchKernelGGL((resample_kernel<S, TT>), grid, dim3(256), (size_t)tl.lds_samples * sizeof(float2), stream, (const typename S::Word*)rq.in.raw,
                       rq.in.stride, rq.in.first, rq.in.n, stage, d.d_taps, d.L, d.M, tl.p_first, tl.n_periods, tl.np_tile, tl.pc_tile,
                       tl.n_pchunks, (float2*)rq.out.iq, rq.out.stride);
}

// The tap counts each policy is instantiated for: the resampler's 16..64, the down-converter's 32..128.
template <class S, class... A>
static void resample_launch_taps(int32_t T, const A&... a) {
    if constexpr (!S::kReal) {
        switch (T) {
            case 16: resample_launch_one<S, 16>(a...); break;
            case 24: resample_launch_one<S, 24>(a...); break;
            case 32: resample_launch_one<S, 32>(a...); break;
            case 48: resample_launch_one<S, 48>(a...); break;
            default: resample_launch_one<S, 64>(a...); break;
        }
    } else {
        switch (T) {
            case 32: resample_launch_one<S, 32>(a...); break;
            case 48: resample_launch_one<S, 48>(a...); break;
            case 64: resample_launch_one<S, 64>(a...); break;
            case 96: resample_launch_one<S, 96>(a...); break;
            default: resample_launch_one<S, 128>(a...); break;
        }
    }
}

template <template <class> class Stage, class... A>
static void resample_launch_fmt(int32_t fmt, int32_t T, const A&... a) {
    switch (fmt) {
        case GYP_FMT_F32: resample_launch_taps<Stage<float>>(T, a...); break;
        case GYP_FMT_I8: resample_launch_taps<Stage<int8_t>>(T, a...); break;
        case GYP_FMT_U8: resample_launch_taps<Stage<uint8_t>>(T, a...); break;
        default: resample_launch_taps<Stage<int16_t>>(T, a...); break;
    }
}

template <template <int> class Stage, class... A>
static void resample_launch_bits(int32_t bits, int32_t T, const A&... a) {
    switch (bits) {
        case 1: resample_launch_taps<Stage<1>>(T, a...); break;
        case 2: resample_launch_taps<Stage<2>>(T, a...); break;
        default: resample_launch_taps<Stage<4>>(T, a...); break;
    }
}

// The packing's level table in device memory: uploaded on first use and cached on the context (which frees it), like a design.
static int packed_levels_dev(gyp_ctx* ctx, const PackedFormat& pk, const float** out) {
    for (const auto& l : ctx->packed_levels)
        if (std::memcmp(l.first.v, pk.levels.v, sizeof(pk.levels.v)) == 0) {
            *out = l.second.get();
            return GYP_OK;
        }
    DevBuf<float> d;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, upload(d, pk.levels.v, 16, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // `pk` may be the caller's temporary
    *out = d.get();
    ctx->packed_levels.emplace_back(pk.levels, std::move(d));
    return GYP_OK;
}

// Enqueue resample_kernel on `stream` for a request that has passed resample_check (n_ms >= 1).  The staging policy follows the
// words (rq.pk, rq.fmt) and the design's kind, which matches the packing's: a real design stages real words mixed down from if_hz.
static int resample_launch(gyp_ctx* ctx, hipStream_t stream, const ResampleDesign& d, const SampleRequest& rq) {
    const ResampleTiling tl = resample_tiling(d, d.taps, rq.out.n_streams, rq.out.first_ms, rq.out.n_ms, ctx->resample_tile - (rq.pk ? 8 : 0));
    if (!tl.fits) return fail(ctx, GYP_E_BAD_ARG, "gyp_resample: launch too large (split it)");
    const MixerParams mix = mixer_params(d.fs_in, rq.if_hz);
    if (!rq.pk) {
        if (d.real) resample_launch_fmt<StageReal>(rq.fmt, d.taps, stream, d, rq, tl, StageRealParams{rq.scale, mix.fs, mix.f, mix.q_scale, mix.y_scale});
        else resample_launch_fmt<StageIQ>(rq.fmt, d.taps, stream, d, rq, tl, StageIQParams{rq.scale});
    } else {
        const float* levels = nullptr;
        if (const int rc = packed_levels_dev(ctx, *rq.pk, &levels)) return rc;
        const StagePackedParams words{levels, rq.scale, rq.pk->order, rq.in.bit0};
        if (d.real) resample_launch_bits<StageRealPacked>(rq.pk->bits, d.taps, stream, d, rq, tl, StageRealPackedParams{words, mix.fs, mix.f, mix.q_scale, mix.y_scale});
        else resample_launch_bits<StageIQPacked>(rq.pk->bits, d.taps, stream, d, rq, tl, words);
    }
    HIP_TRY(ctx, hipGetLastError());
    return GYP_OK;
}

// Enqueue ingest_unpack_kernel on `stream` (packed I,Q words at their own rate): the request's in.n samples of every stream.
static int unpack_launch(gyp_ctx* ctx, hipStream_t stream, const SampleRequest& rq) {
    const PackedFormat& pk = *rq.pk;
    const UnpackPlan pl = unpack_plan(persistent_cap(ctx), (uintptr_t)rq.out.iq, rq.out.stride, pk.bits, rq.in.n, rq.out.n_streams);
    const float* levels = nullptr;
    if (const int rc = packed_levels_dev(ctx, pk, &levels)) return rc;
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(pl.grid), dim3(256), 0, stream, (const uint8_t*)rq.in.raw, rq.in.stride, rq.in.bit0, rq.in.n, rq.out.n_streams,
                           levels, rq.scale, pk.order, (float2*)rq.out.iq, rq.out.stride, pl.vec4);
    };
    switch (pk.bits) {
        case 1: launch(ingest_unpack_kernel<1>); break;
        case 2: launch(ingest_unpack_kernel<2>); break;
        default: launch(ingest_unpack_kernel<4>); break;
    }
    HIP_TRY(ctx, hipGetLastError());
    return GYP_OK;
}

// A packed buffer holds bit0 + n * B bits per stream, bit0 a sample edge below 8 (the unpacker's entry asks this too).
static bool packed_window_ok(const PackedFormat& pk, const RawWindow& in) {
    const int64_t B = pk.sample_bits();
    if (in.bit0 < 0 || in.bit0 >= 8 || in.bit0 % B || in.n < 0 || in.stride < 0) return false;
    if (in.n > (INT64_MAX - 8) / B / 2 || in.stride > INT64_MAX / 16) return false;
    return in.stride * 8 >= in.bit0 + in.n * B;
}

// GYP_E_BAD_ARG's reason, or nullptr if the request can be launched with design d (n_ms == 0: there is nothing to launch).
static const char* resample_check(const ResampleDesign& d, const SampleRequest& rq) {
    const RawWindow& in = rq.in;
    const bool rest_ok = rq.out.n_streams >= 1 && rq.out.n_ms >= 0 && rq.out.first_ms >= 0 && rq.out.stride >= (int64_t)rq.out.n_ms * d.n_out &&
                         std::isfinite(rq.scale) && (in.n <= 0 || in.raw) && (rq.out.n_ms <= 0 || rq.out.iq);
    if (!rq.pk)
        return rest_ok && in.n >= 0 && in.stride >= in.n ? nullptr
                                                         : "bad arguments (n_streams >= 1, n_ms >= 0, first_ms >= 0, in_stride >= raw_n_samples >= 0, "
                                                           "out_stride >= n_ms * N_out, finite scale, non-NULL buffers)";
    return rest_ok && packed_window_ok(*rq.pk, in) ? nullptr
                                                   : "bad arguments (n_streams >= 1, n_ms >= 0, first_ms >= 0, raw_n_samples >= 0, 0 <= bit0 < 8 a multiple of "
                                                     "the sample's bits, 8 in_stride_bytes >= bit0 + raw_n_samples * sample bits, out_stride >= n_ms * N_out, "
                                                     "finite scale, non-NULL buffers)";
}

// The three resampling device entries behind their own first checks: the design, the argument check, the launch on the context's stream.
static int resample_dev(gyp_ctx* ctx, const char* who, int64_t fs_in_hz, bool real, int32_t taps, const SampleRequest& rq) {
    ResampleDesign d;
    if (const int rc = filter_design(ctx, fs_in_hz, real, rq.if_hz, taps, &d, who)) return rc;
    if (const char* why = resample_check(d, rq)) return fail(ctx, GYP_E_BAD_ARG, std::string(who) + ": " + why);
    if (rq.out.n_ms == 0) return GYP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return resample_launch(ctx, ctx->stream, d, rq);
}

extern "C" {

int gyp_resample_design(int64_t fs_in_hz, int64_t fs_out_hz, int32_t taps, float* table_out, int32_t* n_phases_out) {
    const int32_t T = resample_taps(taps);
    if (!T) return fail(nullptr, GYP_E_BAD_ARG, std::string("gyp_resample_design") + kResampleTapsRule);
    if (!resample_rates_ok(fs_in_hz, fs_out_hz))
        return fail(nullptr, GYP_E_BAD_RATE, "gyp_resample_design: rates must be positive multiples of 1000 Hz, differ, and lie within a factor 2");
    const int32_t L = resample_ratio(fs_in_hz, fs_out_hz).L;
    if (n_phases_out) *n_phases_out = L;
    if (table_out) resample_design_rows(fs_in_hz, fs_out_hz, T, L, table_out);
    return GYP_OK;
}

int gyp_resample_iq_dev(gyp_ctx* ctx, int32_t fmt, const void* raw_dev, int32_t n_streams, int64_t in_stride_samples,
                        int64_t raw_first_sample, int64_t raw_n_samples, float scale, int64_t fs_in_hz, int32_t taps, int64_t first_ms,
                        int32_t n_ms, int64_t out_stride_samples, float* out_dev) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (!ingest_word_bytes(fmt)) return fail(ctx, GYP_E_BAD_ARG, "gyp_resample_iq_dev: fmt must be one of GYP_FMT_*");
    SampleRequest rq{};
    rq.fmt = fmt, rq.scale = scale;
    rq.in = RawWindow{raw_dev, in_stride_samples, raw_first_sample, raw_n_samples, 0};
    rq.out = OutWindow{out_dev, out_stride_samples, first_ms, n_ms, n_streams};
    return resample_dev(ctx, "gyp_resample_iq_dev", fs_in_hz, false, taps, rq);
}

int gyp_ddc_design(int64_t fs_in_hz, int64_t fs_out_hz, int64_t if_hz, int32_t taps, float* table_out, int32_t* n_phases_out,
                   int32_t* taps_out) {
    if (taps && !ddc_taps(taps, 0, 0)) return fail(nullptr, GYP_E_BAD_ARG, std::string("gyp_ddc_design") + kDdcTapsRule);
    if (!ddc_rates_ok(fs_in_hz, fs_out_hz, if_hz)) return fail(nullptr, GYP_E_BAD_RATE, std::string("gyp_ddc_design") + kDdcRateRule);
    const int32_t T = ddc_taps(taps, fs_in_hz, fs_out_hz);
    const int32_t L = resample_ratio(fs_in_hz, fs_out_hz).L;
    if (n_phases_out) *n_phases_out = L;
    if (taps_out) *taps_out = T;
    if (table_out) resample_design_rows(fs_in_hz, fs_out_hz, T, L, table_out);
    return GYP_OK;
}

int gyp_ddc_iq_dev(gyp_ctx* ctx, int32_t fmt, const void* raw_dev, int32_t n_streams, int64_t in_stride_samples, int64_t raw_first_sample,
                   int64_t raw_n_samples, float scale, int64_t fs_in_hz, int64_t if_hz, int32_t taps, int64_t first_ms, int32_t n_ms,
                   int64_t out_stride_samples, float* out_dev) {
    if (!ctx) return GYP_E_BAD_ARG;
    if (!ingest_word_bytes(fmt)) return fail(ctx, GYP_E_BAD_ARG, "gyp_ddc_iq_dev: fmt must be one of GYP_FMT_*");
    SampleRequest rq{};
    rq.fmt = fmt, rq.if_hz = if_hz, rq.scale = scale;
    rq.in = RawWindow{raw_dev, in_stride_samples, raw_first_sample, raw_n_samples, 0};
    rq.out = OutWindow{out_dev, out_stride_samples, first_ms, n_ms, n_streams};
    return resample_dev(ctx, "gyp_ddc_iq_dev", fs_in_hz, true, taps, rq);
}

int gyp_packed_span(const gyp_packing* packing, int32_t samples_per_ms, int64_t file_bytes, int64_t first_sample, int64_t n_samples,
                    int64_t* in_first_out, int64_t* in_n_out, int64_t* first_byte_out, int32_t* bit0_out, int64_t* n_bytes_out,
                    int64_t* file_samples_out, int64_t* total_ms_out) {
    PackedFormat pk;
    if (const char* why = packing_check(packing, &pk)) return fail(nullptr, GYP_E_BAD_ARG, std::string("gyp_packed_span: ") + why);
    if (samples_per_ms < 1 || file_bytes < 0 || file_bytes > ((int64_t)1 << 58) || n_samples < 0 || n_samples > ((int64_t)1 << 61) ||
        first_sample < -((int64_t)1 << 61) || first_sample > ((int64_t)1 << 61))
        return fail(nullptr, GYP_E_BAD_ARG, "gyp_packed_span: bad arguments (samples_per_ms >= 1, 0 <= file_bytes < 2^58, 0 <= n_samples <= 2^61, "
                                            "|first_sample| <= 2^61)");
    const int64_t file_samples = file_bytes * 8 / pk.sample_bits();
    const PackedSpan sp = packed_span(pk.sample_bits(), file_samples, first_sample, n_samples);
    if (in_first_out) *in_first_out = sp.in_first;
    if (in_n_out) *in_n_out = sp.in_n;
    if (first_byte_out) *first_byte_out = sp.first_byte;
    if (bit0_out) *bit0_out = sp.bit0;
    if (n_bytes_out) *n_bytes_out = sp.n_bytes;
    if (file_samples_out) *file_samples_out = file_samples;
    if (total_ms_out) *total_ms_out = file_samples > 0 ? (file_samples - 1) / samples_per_ms : 0;
    return GYP_OK;
}

int gyp_unpack_iq_dev(gyp_ctx* ctx, const gyp_packing* packing, const void* raw_dev, int32_t n_streams, int64_t in_stride_bytes,
                      int32_t bit0, int64_t n_samples, float scale, int64_t out_stride_samples, float* out_dev) {
    if (!ctx) return GYP_E_BAD_ARG;
    PackedFormat pk;
    if (const char* why = packing_check(packing, &pk)) return fail(ctx, GYP_E_BAD_ARG, std::string("gyp_unpack_iq_dev: ") + why);
    if (pk.real) return fail(ctx, GYP_E_BAD_ARG, "gyp_unpack_iq_dev: real words are down-converted (gyp_resample_packed_dev), not unpacked");
    SampleRequest rq{};
    rq.pk = &pk, rq.scale = scale;
    rq.in = RawWindow{raw_dev, in_stride_bytes, 0, n_samples, bit0};
    rq.out = OutWindow{out_dev, out_stride_samples, 0, 0, n_streams};
    if (n_streams < 1 || n_streams > 65535 || !packed_window_ok(pk, rq.in) || out_stride_samples < n_samples || !std::isfinite(scale) ||
        (n_samples > 0 && (!raw_dev || !out_dev)))
        return fail(ctx, GYP_E_BAD_ARG, "gyp_unpack_iq_dev: bad arguments (1 <= n_streams <= 65535, n_samples >= 0, 0 <= bit0 < 8 a multiple "
                                        "of the sample's bits, 8 in_stride_bytes >= bit0 + n_samples * sample bits, out_stride >= n_samples, "
                                        "finite scale, non-NULL buffers)");
    if (n_samples == 0) return GYP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return unpack_launch(ctx, ctx->stream, rq);
}

int gyp_resample_packed_dev(gyp_ctx* ctx, const gyp_packing* packing, const void* raw_dev, int32_t n_streams, int64_t in_stride_bytes,
                            int32_t bit0, int64_t raw_first_sample, int64_t raw_n_samples, float scale, int64_t fs_in_hz, int64_t if_hz,
                            int32_t taps, int64_t first_ms, int32_t n_ms, int64_t out_stride_samples, float* out_dev) {
    if (!ctx) return GYP_E_BAD_ARG;
    const char* who = "gyp_resample_packed_dev";
    PackedFormat pk;
    if (const char* why = packing_check(packing, &pk)) return fail(ctx, GYP_E_BAD_ARG, std::string(who) + ": " + why);
    if (pk.real != (if_hz != 0))
        return fail(ctx, GYP_E_BAD_ARG, std::string(who) + ": real words need if_hz != 0, I,Q words if_hz = 0");
    SampleRequest rq{};
    rq.pk = &pk, rq.if_hz = if_hz, rq.scale = scale;
    rq.in = RawWindow{raw_dev, in_stride_bytes, raw_first_sample, raw_n_samples, bit0};
    rq.out = OutWindow{out_dev, out_stride_samples, first_ms, n_ms, n_streams};
    return resample_dev(ctx, who, fs_in_hz, pk.real, taps, rq);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// Level (kernels_level.hpp): per-millisecond statistics, y = (x - dc) * gain
// ---------------------------------------------------------------------------------------------------------
// One call of a conditioning stage, by name.  A stage that only measures leaves `out` null; the level and histogram stages take a
// count of samples in place of n_ms x n.
struct IqWindow {
    const float* in;        // stream 0's complex64 samples
    float* out;             // where a stage that writes samples puts them (may be `in`); strided like `in`
    int32_t n_streams;
    int64_t stride;         // between streams, in samples
    int32_t n_ms, n;        // n_ms milliseconds of n samples
    int64_t first_index;    // the absolute index of the window's first sample: the phase reference of the tone stages
    hipStream_t stream;
    IqWindow(const float* in_, float* out_, int32_t n_streams_, int64_t stride_, int32_t n_ms_, int32_t n_, int64_t first_index_, hipStream_t stream_)
        : in(in_), out(out_), n_streams(n_streams_), stride(stride_), n_ms(n_ms_), n(n_), first_index(first_index_), stream(stream_) {}
    const float2* src(int32_t s0) const { return reinterpret_cast<const float2*>(in) + s0 * stride; }   // stream s0's row
    float2* dst(int32_t s0) const { return reinterpret_cast<float2*>(out) + s0 * stride; }
};

// The launches of a plan in order: launch(chunk) fills the chunk's argument struct and enqueues it.  The first error ends the walk.
template <class Launch>
static int for_each_chunk(const StagePlan& pl, Launch&& launch) {
    for (int32_t i = 0; i < pl.n_chunks; ++i)
        if (const int rc = launch(stage_chunk(pl, i))) return rc;
    return GYP_OK;
}
// The refusals' common forms: "<who>: <why>", and rows of `extent` samples that would overlap at this stride
static bool rows_overlap(int32_t n_streams, int64_t stride, int64_t extent) { return n_streams > 1 && stride < extent; }
// The window of the stand-alone blanker, excisor and spectrum histogram, whose refusals read alike but for min_ms, lo and hi
static int window_check(gyp_ctx* ctx, const char* who, const IqWindow& w, int32_t min_ms, int32_t lo, int32_t hi) {
    if (w.n_streams < 1 || w.n_ms < min_ms || w.n < lo || w.n > hi || rows_overlap(w.n_streams, w.stride, (int64_t)w.n_ms * w.n))
        return refuse(ctx, who, "bad arguments (n_streams >= 1, n_ms >= " + std::to_string(min_ms) + ", " + std::to_string(lo) +
                                " <= samples_per_ms <= " + std::to_string(hi) + ", stream_stride_samples >= n_ms * samples_per_ms)");
    return GYP_OK;
}

// Enqueue iq_stats_kernel: one record per (stream, millisecond) of the window into `out`.
static int stats_launch(gyp_ctx* ctx, const IqWindow& w, float clip_level, gyp_iq_stats* out) {
    const StageChunk c = stage_chunk(stats_plan(persistent_cap(ctx), w.n_streams, w.n_ms), 0);
    hipLaunchKernelGGL(iq_stats_kernel, dim3(c.grid_x), dim3(256), 0, w.stream, w.in, w.stride, w.n_ms, w.n, c.items, clip_level, out);
    return launched(ctx);
}

// Enqueue iq_condition_kernel over the first n_samples samples of every stream; unused slots of a launch's levels repeat its last one.
static int condition_launch(gyp_ctx* ctx, const IqWindow& w, int64_t n_samples, const gyp_iq_level* levels) {
    const StagePlan pl = condition_plan(persistent_cap(ctx), kLevelStreams, (uintptr_t)w.in, (uintptr_t)w.out, w.n_streams, w.stride, n_samples);
    return for_each_chunk(pl, [&](const StageChunk& c) {
        LevelArgs a{};
        for (int32_t i = 0; i < kLevelStreams; ++i) a.v[i] = levels[c.s0 + std::min(i, c.ns - 1)];
        hipLaunchKernelGGL(iq_condition_kernel, dim3(c.grid_x, c.grid_y), dim3(256), 0, w.stream, w.in + 2 * c.s0 * w.stride,
                           w.out + 2 * c.s0 * w.stride, w.stride, n_samples, a, pl.vec4);
        return launched(ctx);
    });
}

extern "C" {

int gyp_iq_stats_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t n_ms,
                     int32_t samples_per_ms, float clip_level, gyp_iq_stats* out_dev) {
    const char* who = "gyp_iq_stats_dev";
    if (!ctx) return refuse(nullptr, who, "ctx is NULL");
    if (!iq_dev || !out_dev) return refuse(ctx, who, "iq_dev and out_dev must not be NULL");
    if (n_streams < 1 || n_ms < 1 || samples_per_ms < 1) return refuse(ctx, who, "n_streams, n_ms and samples_per_ms must be >= 1");
    if (rows_overlap(n_streams, stream_stride_samples, (int64_t)n_ms * samples_per_ms))
        return refuse(ctx, who, "stream_stride_samples must be >= n_ms * samples_per_ms");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return stats_launch(ctx, IqWindow(iq_dev, nullptr, n_streams, stream_stride_samples, n_ms, samples_per_ms, 0, ctx->stream), clip_level, out_dev);
}

int gyp_condition_iq_dev(gyp_ctx* ctx, const float* in_dev, float* out_dev, int32_t n_streams, int64_t stream_stride_samples,
                         int64_t n_samples, const gyp_iq_level* levels_host) {
    const char* who = "gyp_condition_iq_dev";
    if (!ctx) return refuse(nullptr, who, "ctx is NULL");
    if (!in_dev || !out_dev || !levels_host) return refuse(ctx, who, "in_dev, out_dev and levels_host must not be NULL");
    if (n_streams < 1 || n_samples < 0 || rows_overlap(n_streams, stream_stride_samples, n_samples))
        return refuse(ctx, who, "bad arguments (n_streams >= 1, n_samples >= 0, stream_stride_samples >= n_samples)");
    for (int32_t s = 0; s < n_streams; ++s)
        if (const char* why = level_check(&levels_host[s])) return refuse(ctx, who, why);
    if (n_samples == 0) return GYP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return condition_launch(ctx, IqWindow(in_dev, out_dev, n_streams, stream_stride_samples, 0, 0, 0, ctx->stream), n_samples, levels_host);
}

int gyp_iq_level_from_stats(const gyp_iq_stats* stats, int32_t n_ms, int32_t samples_per_ms, int32_t remove_dc, double target_rms,
                            gyp_iq_level* level_out, double* measured_out4) {
    if (!stats || !level_out) return fail(nullptr, GYP_E_BAD_ARG, "gyp_iq_level_from_stats: stats and level_out must not be NULL");
    if (n_ms < 1 || samples_per_ms < 1) return fail(nullptr, GYP_E_BAD_ARG, "gyp_iq_level_from_stats: n_ms and samples_per_ms must be >= 1");
    if (!(target_rms > 0.0) || !std::isfinite(target_rms))
        return fail(nullptr, GYP_E_BAD_ARG, "gyp_iq_level_from_stats: target_rms must be positive and finite");
    if (const char* why = level_from_stats(stats, n_ms, samples_per_ms, remove_dc, target_rms, level_out, measured_out4))
        return fail(nullptr, GYP_E_BAD_ARG, std::string("gyp_iq_level_from_stats: ") + why);
    return GYP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// Notch (kernels_notch.hpp): complex amplitudes of tones per block, their per-millisecond projection out of the samples
// ---------------------------------------------------------------------------------------------------------
static bool tone_rate_ok(int64_t fs_hz) { return fs_hz >= 1000 && fs_hz < ((int64_t)1 << 31); }
static ToneMix tone_mix(int64_t fs_hz) {
    const MixerParams m = mixer_params(fs_hz, 0);
    return ToneMix{m.fs, m.q_scale, m.y_scale};
}

// Enqueue iq_tones_kernel for the n_freq frequencies the context's table holds (tones_upload_freqs): one record per (stream, block,
// frequency) of the window, whose n_ms x n are blocks x samples here, into `out`.
static int tones_launch(gyp_ctx* ctx, const IqWindow& w, int64_t fs_hz, int32_t n_freq, int32_t window, gyp_tone_rec* out) {
    const StageChunk c = stage_chunk(tones_plan(ctx->n_cus, w.n_streams, w.n_ms, n_freq), 0);
    hipLaunchKernelGGL(iq_tones_kernel, dim3(c.grid_x), dim3(256), 0, w.stream, w.src(0), w.stride, w.first_index, w.n_ms, w.n,
                       ctx->tone_freqs.get(), n_freq, tone_mix(fs_hz), window, c.items, out);
    return launched(ctx);
}

// The call's frequencies as f mod fs in the context's table.  Waits for the copy: the host array is the caller's.
static int tones_upload_freqs(gyp_ctx* ctx, const int64_t* freqs_hz, int32_t n_freq, int64_t fs_hz) {
    std::vector<int64_t> r((size_t)n_freq);
    for (int32_t k = 0; k < n_freq; ++k) r[(size_t)k] = tone_mod(freqs_hz[k], fs_hz);
    HIP_TRY(ctx, upload(ctx->tone_freqs, r.data(), r.size(), ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return GYP_OK;
}

// Enqueue iq_notch_kernel for tone lists that have passed notch_check; unused slots of a launch's lists stay empty.
static int notch_launch(gyp_ctx* ctx, const IqWindow& w, int64_t fs_hz, const gyp_notch_tones* tones) {
    const StagePlan pl = notch_plan(persistent_cap(ctx), kNotchStreams, w.n_streams, w.n_ms, w.n, kNotchLdsSamples, ctx->notch_no_lds);
    return for_each_chunk(pl, [&](const StageChunk& c) {
        NotchArgs a{};
        for (int32_t i = 0; i < c.ns; ++i) {
            a.count[i] = tones[c.s0 + i].count;
            for (int32_t k = 0; k < a.count[i]; ++k) a.f[i][k] = tone_mod(tones[c.s0 + i].freq_hz[k], fs_hz);
        }
        return for_flag(pl.lds_bytes > 0, [&](auto lds) {
            return launch_dyn(ctx, iq_notch_kernel<decltype(lds)::value>, dim3(c.grid_x), dim3(kNotchThreads), (size_t)pl.lds_bytes, w.stream,
                              w.src(c.s0), w.dst(c.s0), w.stride, w.first_index, w.n_ms, w.n, c.items, tone_mix(fs_hz), a);
        });
    });
}

extern "C" {

int gyp_iq_tones_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int64_t first_sample_index,
                     int32_t n_blocks, int32_t block_samples, int64_t fs_hz, const int64_t* freqs_hz_host, int32_t n_freq, int32_t window,
                     gyp_tone_rec* out_dev) {
    const char* who = "gyp_iq_tones_dev";
    if (!ctx) return refuse(nullptr, who, "ctx is NULL");
    if (!iq_dev || !out_dev || !freqs_hz_host) return refuse(ctx, who, "iq_dev, freqs_hz_host and out_dev must not be NULL");
    if (n_streams < 1 || n_blocks < 1 || block_samples < 1 || n_freq < 1 || first_sample_index < 0)
        return refuse(ctx, who, "n_streams, n_blocks, block_samples and n_freq must be >= 1, first_sample_index >= 0");
    if (rows_overlap(n_streams, stream_stride_samples, (int64_t)n_blocks * block_samples))
        return refuse(ctx, who, "stream_stride_samples must be >= n_blocks * block_samples");
    if (!tone_rate_ok(fs_hz)) return refuse(ctx, who, "fs_hz must lie in [1000, 2^31)");
    if (window != GYP_WINDOW_RECT && window != GYP_WINDOW_HANN) return refuse(ctx, who, "window must be GYP_WINDOW_RECT or GYP_WINDOW_HANN");
    for (int32_t k = 0; k < n_freq; ++k) {
        const int64_t f = freqs_hz_host[k];
        if (f <= -fs_hz || f >= fs_hz || 2 * (f < 0 ? -f : f) >= fs_hz) return refuse(ctx, who, "every frequency must satisfy |f| < fs / 2");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (const int rc = tones_upload_freqs(ctx, freqs_hz_host, n_freq, fs_hz)) return rc;
    const IqWindow w(iq_dev, nullptr, n_streams, stream_stride_samples, n_blocks, block_samples, first_sample_index, ctx->stream);
    return tones_launch(ctx, w, fs_hz, n_freq, window, out_dev);
}

int gyp_notch_iq_dev(gyp_ctx* ctx, const float* in_dev, float* out_dev, int32_t n_streams, int64_t stream_stride_samples,
                     int64_t first_sample_index, int32_t n_ms, int32_t samples_per_ms, int64_t fs_hz, const gyp_notch_tones* tones_host) {
    const char* who = "gyp_notch_iq_dev";
    if (!ctx) return refuse(nullptr, who, "ctx is NULL");
    if (!in_dev || !out_dev || !tones_host) return refuse(ctx, who, "in_dev, out_dev and tones_host must not be NULL");
    if (n_streams < 1 || n_ms < 0 || samples_per_ms < 1 || first_sample_index < 0 ||
        rows_overlap(n_streams, stream_stride_samples, (int64_t)n_ms * samples_per_ms))
        return refuse(ctx, who, "bad arguments (n_streams >= 1, n_ms >= 0, samples_per_ms >= 1, first_sample_index >= 0, "
                                "stream_stride_samples >= n_ms * samples_per_ms)");
    if (!tone_rate_ok(fs_hz)) return refuse(ctx, who, "fs_hz must lie in [1000, 2^31)");
    for (int32_t s = 0; s < n_streams; ++s) {
        if (tones_host[s].reserved != 0) return refuse(ctx, who, "tones.reserved must be 0");
        if (const char* why = notch_check(tones_host[s].freq_hz, tones_host[s].count, fs_hz)) return refuse(ctx, who, why);
    }
    if (n_ms == 0) return GYP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const IqWindow w(in_dev, out_dev, n_streams, stream_stride_samples, n_ms, samples_per_ms, first_sample_index, ctx->stream);
    return notch_launch(ctx, w, fs_hz, tones_host);
}

int gyp_tones_find(const double* power, int32_t n_freq, double freq_step_hz, double threshold_over_median, int32_t min_separation_bins,
                   int32_t max_tones, int32_t* out_bins) {
    if (!power || (!out_bins && max_tones > 0)) return fail(nullptr, GYP_E_BAD_ARG, "gyp_tones_find: power and out_bins must not be NULL");
    if (n_freq < 1 || min_separation_bins < 1 || max_tones < 0)
        return fail(nullptr, GYP_E_BAD_ARG, "gyp_tones_find: n_freq and min_separation_bins must be >= 1, max_tones >= 0");
    if (!(freq_step_hz > 0.0) || !std::isfinite(freq_step_hz) || !(threshold_over_median > 0.0) || !std::isfinite(threshold_over_median))
        return fail(nullptr, GYP_E_BAD_ARG, "gyp_tones_find: freq_step_hz and threshold_over_median must be positive and finite");
    const char* why = nullptr;
    const int32_t n = tones_find(power, n_freq, threshold_over_median, min_separation_bins, max_tones, out_bins, &why);
    if (n < 0) return fail(nullptr, GYP_E_BAD_ARG, std::string("gyp_tones_find: ") + why);
    return n;
}

int gyp_tone_refine(const gyp_tone_rec* records, int32_t n_blocks, double block_seconds, double* delta_hz_out) {
    if (!records || !delta_hz_out) return fail(nullptr, GYP_E_BAD_ARG, "gyp_tone_refine: records and delta_hz_out must not be NULL");
    if (n_blocks < 2) return fail(nullptr, GYP_E_BAD_ARG, "gyp_tone_refine: n_blocks must be >= 2");
    if (!(block_seconds > 0.0) || !std::isfinite(block_seconds))
        return fail(nullptr, GYP_E_BAD_ARG, "gyp_tone_refine: block_seconds must be positive and finite");
    *delta_hz_out = tone_refine(records, n_blocks, block_seconds);
    return GYP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// Signal quality (kernels_quality.hpp): per (channel, window) sums of tracking records, the figures derived from them
// ---------------------------------------------------------------------------------------------------------
// GYP_E_BAD_ARG's reason, or nullptr if the call can be launched.
static const char* quality_check(const void* recs, int32_t n_chan, int64_t chan_stride_recs, int32_t n_ms, int32_t window_ms,
                                 const int32_t* bit_offset, const void* out) {
    if (!recs || !out) return "the records and the output must not be NULL";
    if (n_chan < 1 || n_ms < 1 || window_ms < 1) return "n_chan, n_ms and window_ms must be >= 1";
    if (n_chan > 1 && chan_stride_recs < n_ms) return "chan_stride_recs must be >= n_ms";
    if (bit_offset)
        for (int32_t c = 0; c < n_chan; ++c)
            if (bit_offset[c] < -1 || bit_offset[c] >= kGroupMs) return "every bit offset must lie in -1 .. 19";
    return nullptr;
}

// Enqueue track_quality_kernel on the context's stream for arguments that have passed quality_check; unused slots of a launch's
// bit offsets, and every slot without offsets, are -1.
static int quality_launch(gyp_ctx* ctx, const gyp_track_rec* recs, int32_t n_chan, int64_t stride, int32_t n_ms, int32_t window_ms,
                          const int32_t* bit_offset, gyp_quality_sums* out) {
    const StagePlan pl = quality_plan(ctx->n_cus, kQualityChans, n_chan, n_ms, window_ms);
    const int32_t n_win = (int32_t)pl.per_stream;
    return for_each_chunk(pl, [&](const StageChunk& c) {
        QualityArgs a;
        for (int32_t i = 0; i < kQualityChans; ++i) a.bit_offset[i] = (int8_t)(bit_offset && i < c.ns ? bit_offset[c.s0 + i] : -1);
        hipLaunchKernelGGL(track_quality_kernel, dim3(c.grid_x), dim3(256), 0, ctx->stream, recs + (int64_t)c.s0 * stride, stride, n_ms,
                           window_ms, n_win, c.items, a, out + (int64_t)c.s0 * n_win);
        return launched(ctx);
    });
}

extern "C" {

int gyp_track_quality_dev(gyp_ctx* ctx, const gyp_track_rec* recs_dev, int32_t n_chan, int64_t chan_stride_recs, int32_t n_ms,
                          int32_t window_ms, const int32_t* bit_offset_host, gyp_quality_sums* out_dev) {
    const char* who = "gyp_track_quality_dev";
    if (!ctx) return refuse(nullptr, who, "ctx is NULL");
    if (const char* why = quality_check(recs_dev, n_chan, chan_stride_recs, n_ms, window_ms, bit_offset_host, out_dev)) return refuse(ctx, who, why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return quality_launch(ctx, recs_dev, n_chan, chan_stride_recs, n_ms, window_ms, bit_offset_host, out_dev);
}

int gyp_track_quality(gyp_ctx* ctx, const gyp_track_rec* recs_host, int32_t n_chan, int64_t chan_stride_recs, int32_t n_ms,
                      int32_t window_ms, const int32_t* bit_offset_host, gyp_quality_sums* out_host) {
    const char* who = "gyp_track_quality";
    if (!ctx) return refuse(nullptr, who, "ctx is NULL");
    if (const char* why = quality_check(recs_host, n_chan, chan_stride_recs, n_ms, window_ms, bit_offset_host, out_host)) return refuse(ctx, who, why);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Scratch& sc = ctx->scratch;
    const size_t n_recs = (size_t)(n_chan - 1) * (size_t)chan_stride_recs + (size_t)n_ms;
    const size_t n_out = (size_t)n_chan * (size_t)quality_windows(n_ms, window_ms);
    HIP_TRY(ctx, upload(sc.quality_recs, recs_host, n_recs, ctx->stream));
    HIP_TRY(ctx, sc.quality_sums.reserve(n_out, Slack::grow, ctx->stream));
    if (const int rc = quality_launch(ctx, sc.quality_recs.get(), n_chan, chan_stride_recs, n_ms, window_ms, bit_offset_host, sc.quality_sums.get()))
        return rc;
    return fetch(ctx, out_host, sc.quality_sums.get(), n_out);
}

int gyp_quality_from_sums(const gyp_quality_sums* sums, int32_t n, gyp_quality* out) {
    if (!sums || !out) return fail(nullptr, GYP_E_BAD_ARG, "gyp_quality_from_sums: sums and out must not be NULL");
    if (n < 1) return fail(nullptr, GYP_E_BAD_ARG, "gyp_quality_from_sums: n must be >= 1");
    quality_from_sums(sums, n, out);
    return GYP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// Blanker (kernels_blank.hpp): per-millisecond pulse blanking, the power histogram its threshold comes from
// ---------------------------------------------------------------------------------------------------------
// Enqueue iq_blank_kernel for blankers that have passed blanker_check; unused slots of a launch's blankers repeat its last one.
// counts (may be null): one int32 per (stream, millisecond).  In place only the blanked samples are stored.
static int blank_launch(gyp_ctx* ctx, const IqWindow& w, const gyp_blanker* blankers, int32_t* counts) {
    const StagePlan pl = blank_plan(persistent_cap(ctx), kBlankStreams, w.n_streams, w.n_ms);
    return for_each_chunk(pl, [&](const StageChunk& c) {
        BlankArgs a{};
        for (int32_t i = 0; i < kBlankStreams; ++i) a.v[i] = blankers[c.s0 + std::min(i, c.ns - 1)];
        int32_t* cnt = counts ? counts + (int64_t)c.s0 * w.n_ms : nullptr;
        for_flag(w.in == w.out, [&](auto in_place) {   // the kernel's flag is `copy`
            hipLaunchKernelGGL(iq_blank_kernel<!decltype(in_place)::value>, dim3(c.grid_x), dim3(kBlankThreads), 0, w.stream, w.src(c.s0), w.dst(c.s0),
                               w.stride, w.n_ms, w.n, c.items, a, cnt);
        });
        return launched(ctx);
    });
}

// Zero the histograms and enqueue iq_power_hist_kernel over the first n_samples samples of every stream.  centres: 2 floats per
// stream, or null for 0; unused slots of a launch's centres stay zero.
static int hist_launch(gyp_ctx* ctx, const IqWindow& w, int64_t n_samples, const float* centres, uint32_t* hist) {
    HIP_TRY(ctx, hipMemsetAsync(hist, 0, (size_t)w.n_streams * GYP_POWER_HIST_BINS * sizeof(uint32_t), w.stream));
    return for_each_chunk(hist_plan(persistent_cap(ctx), kBlankStreams, w.n_streams, n_samples), [&](const StageChunk& c) {
        HistArgs a{};
        for (int32_t i = 0; i < c.ns; ++i) a.c[i] = centres ? make_float2(centres[2 * (c.s0 + i)], centres[2 * (c.s0 + i) + 1]) : make_float2(0.f, 0.f);
        hipLaunchKernelGGL(iq_power_hist_kernel, dim3(c.grid_x, c.grid_y), dim3(256), 0, w.stream, w.src(c.s0), w.stride, n_samples, a,
                           hist + (int64_t)c.s0 * GYP_POWER_HIST_BINS);
        return launched(ctx);
    });
}

extern "C" {

int gyp_blank_iq_dev(gyp_ctx* ctx, const float* in_dev, float* out_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t n_ms,
                     int32_t samples_per_ms, const gyp_blanker* blankers_host, int32_t* counts_out_dev) {
    const char* who = "gyp_blank_iq_dev";
    if (!ctx) return refuse(nullptr, who, "ctx is NULL");
    if (!in_dev || !out_dev || !blankers_host) return refuse(ctx, who, "in_dev, out_dev and blankers_host must not be NULL");
    const IqWindow w(in_dev, out_dev, n_streams, stream_stride_samples, n_ms, samples_per_ms, 0, ctx->stream);
    if (const int rc = window_check(ctx, who, w, 0, 1, kBlankMaxSamples)) return rc;
    for (int32_t s = 0; s < n_streams; ++s)
        if (const char* why = blanker_check(&blankers_host[s])) return refuse(ctx, who, why);
    if (n_ms == 0) return GYP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return blank_launch(ctx, w, blankers_host, counts_out_dev);
}

int gyp_iq_power_hist_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int64_t n_samples,
                          const float* centers_host, uint32_t* hist_out_dev) {
    const char* who = "gyp_iq_power_hist_dev";
    if (!ctx) return refuse(nullptr, who, "ctx is NULL");
    if (!iq_dev || !hist_out_dev) return refuse(ctx, who, "iq_dev and hist_out_dev must not be NULL");
    if (n_streams < 1 || n_samples < 1 || rows_overlap(n_streams, stream_stride_samples, n_samples))
        return refuse(ctx, who, "bad arguments (n_streams >= 1, n_samples >= 1, stream_stride_samples >= n_samples)");
    if (centers_host)
        for (int32_t i = 0; i < 2 * n_streams; ++i)
            if (!std::isfinite(centers_host[i])) return refuse(ctx, who, "every centre must be finite");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return hist_launch(ctx, IqWindow(iq_dev, nullptr, n_streams, stream_stride_samples, 0, 0, 0, ctx->stream), n_samples, centers_host, hist_out_dev);
}

int gyp_blank_from_hist(const uint32_t* hist, float center_re, float center_im, double threshold_over_median, int32_t guard,
                        gyp_blanker* blanker_out, double* measured_out2) {
    if (!hist || !blanker_out) return fail(nullptr, GYP_E_BAD_ARG, "gyp_blank_from_hist: hist and blanker_out must not be NULL");
    if (!(threshold_over_median > 0.0) || !std::isfinite(threshold_over_median))
        return fail(nullptr, GYP_E_BAD_ARG, "gyp_blank_from_hist: threshold_over_median must be positive and finite");
    if (!std::isfinite(center_re) || !std::isfinite(center_im)) return fail(nullptr, GYP_E_BAD_ARG, "gyp_blank_from_hist: the centre must be finite");
    if (guard < 0 || guard > kBlankMaxGuard) return fail(nullptr, GYP_E_BAD_ARG, "gyp_blank_from_hist: guard must lie in 0 .. 64");
    if (const char* why = blank_from_hist(hist, center_re, center_im, threshold_over_median, guard, blanker_out, measured_out2))
        return fail(nullptr, GYP_E_BAD_ARG, std::string("gyp_blank_from_hist: ") + why);
    return GYP_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------
// Excisor (kernels_excise.hpp): per-millisecond excision of spectral bins, the bin-power histogram its threshold comes from
// ---------------------------------------------------------------------------------------------------------
// Enqueue iq_excise_kernel for excisors that have passed excisor_check; unused slots of a launch's excisors repeat its last one.
// counts (may be null): one int32 per (stream, millisecond); masks (may be null): four words per (stream, millisecond, frame).
static int excise_launch(gyp_ctx* ctx, const IqWindow& w, const gyp_excisor* excisors, int32_t* counts, uint64_t* masks) {
    const StagePlan pl = excise_plan(persistent_cap(ctx), kExciseStreams, w.n_streams, w.n_ms);
    return for_each_chunk(pl, [&](const StageChunk& c) {
        ExciseArgs a{};
        for (int32_t i = 0; i < kExciseStreams; ++i) a.v[i] = excisors[c.s0 + std::min(i, c.ns - 1)];
        int32_t* cnt = counts ? counts + (int64_t)c.s0 * w.n_ms : nullptr;
        uint64_t* msk = masks ? masks + (int64_t)c.s0 * w.n_ms * excise_frames(w.n) * 4 : nullptr;
        for_flag(w.in == w.out, [&](auto in_place) {   // the kernel's flag is `copy`
            hipLaunchKernelGGL(iq_excise_kernel<!decltype(in_place)::value>, dim3(c.grid_x), dim3(kExciseThreads), 0, w.stream, w.src(c.s0),
                               w.dst(c.s0), w.stride, w.n_ms, w.n, c.items, a, cnt, msk);
        });
        return launched(ctx);
    });
}

// Zero the histograms and enqueue iq_spectrum_hist_kernel over the window: every stream in one launch.
static int spectrum_hist_launch(gyp_ctx* ctx, const IqWindow& w, uint32_t* hist) {
    HIP_TRY(ctx, hipMemsetAsync(hist, 0, (size_t)w.n_streams * GYP_POWER_HIST_BINS * sizeof(uint32_t), w.stream));
    const StageChunk c = stage_chunk(excise_plan(persistent_cap(ctx), w.n_streams, w.n_streams, w.n_ms), 0);
    hipLaunchKernelGGL(iq_spectrum_hist_kernel, dim3(c.grid_x), dim3(kExciseThreads), 0, w.stream, w.src(0), w.stride, w.n_ms, w.n, c.items, hist);
    return launched(ctx);
}

extern "C" {

int gyp_excise_iq_dev(gyp_ctx* ctx, const float* in_dev, float* out_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t n_ms,
                      int32_t samples_per_ms, const gyp_excisor* excisors_host, int32_t* counts_out_dev, uint64_t* masks_out_dev) {
    const char* who = "gyp_excise_iq_dev";
    if (!ctx) return refuse(nullptr, who, "ctx is NULL");
    if (!in_dev || !out_dev || !excisors_host) return refuse(ctx, who, "in_dev, out_dev and excisors_host must not be NULL");
    const IqWindow w(in_dev, out_dev, n_streams, stream_stride_samples, n_ms, samples_per_ms, 0, ctx->stream);
    if (const int rc = window_check(ctx, who, w, 0, 1, kExciseMaxSamples)) return rc;
    for (int32_t s = 0; s < n_streams; ++s)
        if (const char* why = excisor_check(&excisors_host[s])) return refuse(ctx, who, why);
    if (n_ms == 0) return GYP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return excise_launch(ctx, w, excisors_host, counts_out_dev, masks_out_dev);
}

int gyp_iq_spectrum_hist_dev(gyp_ctx* ctx, const float* iq_dev, int32_t n_streams, int64_t stream_stride_samples, int32_t n_ms,
                             int32_t samples_per_ms, uint32_t* hist_out_dev) {
    const char* who = "gyp_iq_spectrum_hist_dev";
    if (!ctx) return refuse(nullptr, who, "ctx is NULL");
    if (!iq_dev || !hist_out_dev) return refuse(ctx, who, "iq_dev and hist_out_dev must not be NULL");
    const IqWindow w(iq_dev, nullptr, n_streams, stream_stride_samples, n_ms, samples_per_ms, 0, ctx->stream);
    if (const int rc = window_check(ctx, who, w, 1, GYP_EXCISE_FRAME, kExciseMaxSamples)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return spectrum_hist_launch(ctx, w, hist_out_dev);
}

int gyp_excise_from_hist(const uint32_t* hist, double threshold_over_median, int32_t guard, gyp_excisor* excisor_out, double* measured_out2) {
    if (!hist || !excisor_out) return fail(nullptr, GYP_E_BAD_ARG, "gyp_excise_from_hist: hist and excisor_out must not be NULL");
    if (!(threshold_over_median > 0.0) || !std::isfinite(threshold_over_median))
        return fail(nullptr, GYP_E_BAD_ARG, "gyp_excise_from_hist: threshold_over_median must be positive and finite");
    if (guard < 0 || guard > kExciseMaxGuard) return fail(nullptr, GYP_E_BAD_ARG, "gyp_excise_from_hist: guard must lie in 0 .. 8");
    if (const char* why = excise_from_hist(hist, threshold_over_median, guard, excisor_out, measured_out2))
        return fail(nullptr, GYP_E_BAD_ARG, std::string("gyp_excise_from_hist: ") + why);
    return GYP_OK;
}

}  // extern "C"

static void ingest_free(gyp_ingest* g) {
    ingest_stop_reader(g);
    if (g->ctx) {
        (void)hipSetDevice(g->ctx->device);
        if (g->copy_stream.get()) (void)hipStreamSynchronize(g->copy_stream.get());
    }
    if (g->fd >= 0) close(g->fd);
    delete g;   // the members release what they hold: the rings and events first, the copy stream last
}

// Enqueue ingest_widen_kernel on `stream`: n_words int8, uint8 or int16 words (fmt) -> float32 * scale
static void widen_launch(const gyp_ctx* ctx, hipStream_t stream, int32_t fmt, const void* raw, size_t n_words, float scale, float* out) {
    const dim3 grid(grid_widen(n_words, persistent_cap(ctx)));
    switch (fmt) {
        case kFmtI8: hipLaunchKernelGGL(ingest_widen_kernel<int8_t>, grid, dim3(256), 0, stream, (const int8_t*)raw, out, n_words, scale); break;
        case kFmtU8: hipLaunchKernelGGL(ingest_widen_kernel<uint8_t>, grid, dim3(256), 0, stream, (const uint8_t*)raw, out, n_words, scale); break;
        default: hipLaunchKernelGGL(ingest_widen_kernel<int16_t>, grid, dim3(256), 0, stream, (const int16_t*)raw, out, n_words, scale); break;
    }
}

// One stream of n_ms milliseconds from millisecond first_ms of the handle's output at `in`, as a stage on `stream` takes it
static IqWindow ingest_window(const gyp_ingest* g, const float* in, float* out, int32_t n_ms, int64_t first_ms, hipStream_t stream) {
    return IqWindow(in, out, 1, 0, n_ms, g->src.n, first_ms * g->src.n, stream);
}

// The stages that are on condition device slot d's block in place on the copy stream, behind whatever produced it, in the chain's
// order.  (A counting stage is only on once its counts are made: ingest_counts_made.)
static int ingest_condition(gyp_ingest* g, int d, int64_t first_ms, int32_t n_ms) {
    const Conditioning& cond = g->cond;
    float* iq = g->dev_iq[d].get();
    const IqWindow w = ingest_window(g, iq, iq, n_ms, first_ms, g->copy_stream.get());
    for (const Stage s : kChain) {
        SlotCounts* counts = g->counts_of(s);
        if (counts) counts->mark(d, cond.on(s));
        if (!cond.on(s)) continue;
        const int rc = s == Stage::blanker   ? blank_launch(g->ctx, w, &cond.blanker, counts->dev[d].get())
                       : s == Stage::excisor ? excise_launch(g->ctx, w, &cond.excisor, counts->dev[d].get(), nullptr)
                       : s == Stage::notches ? notch_launch(g->ctx, w, g->fs, &cond.notches)
                                             : condition_launch(g->ctx, w, (int64_t)n_ms * w.n, &cond.level);
        if (rc) return rc;
    }
    return GYP_OK;
}

// The producer of a block, on the copy stream: file-width words in `raw` (the span's slot) -> complex64 in the output slot `iq`.
static int ingest_produce(gyp_ingest* g, const IngestSpan& sp, const gyp_ingest::Upload& u, const void* raw, float* iq) {
    gyp_ctx* ctx = g->ctx;
    const IngestSource& src = g->src;
    const hipStream_t copy = g->copy_stream.get();
    const int64_t out_n = (int64_t)u.n_ms * src.n;
    if (src.kind == SourceKind::plain) {
        if (src.fmt == kFmtF32) return GYP_OK;   // uploaded as it is
        widen_launch(ctx, copy, src.fmt, raw, (size_t)out_n * 2, g->scale, iq);
        HIP_TRY(ctx, hipGetLastError());
        return GYP_OK;
    }
    SampleRequest rq{};
    rq.fmt = src.fmt, rq.pk = src.packed() ? &src.pk : nullptr, rq.if_hz = src.if_hz, rq.scale = g->scale;
    // word formats: the whole window, zero-padded (the buffer's sample 0 is input sample s0).  Packed words: the window's part inside
    // the file (sample 0 is input sample in_first); a block at the output rate lies inside it whole (in_n == out_n)
    rq.in = src.packed() ? RawWindow{raw, sp.n_bytes, sp.in_first, sp.in_n, sp.bit0} : RawWindow{raw, sp.count, sp.s0, sp.count, 0};
    rq.out = OutWindow{iq, out_n, u.first_ms, u.n_ms, 1};
    return src.filtered() ? resample_launch(ctx, copy, src.rs, rq) : unpack_launch(ctx, copy, rq);
}

// Enqueue the upload (+ widening) of the reader's next block on the copy stream.  Returns 1 if a block was
// enqueued, 0 if none is available (end of data, or not yet read and !wait), negative on error.
static int ingest_enqueue_upload(gyp_ingest* g, gyp_ingest::Upload* u, bool wait) {
    gyp_ctx* ctx = g->ctx;
    const IngestSource& src = g->src;
    const hipStream_t copy = g->copy_stream.get();
    // keep fewer than `depth` host slots tied up in uploads: retire the oldest first
    while ((int)g->in_flight.size() >= src.depth - 1) {
        const gyp_ingest::Upload& f = g->in_flight.front();
        HIP_TRY(ctx, hipEventSynchronize(g->uploaded[f.block % src.depth].get()));
        ingest_release(g, f.block + 1);
        g->in_flight.pop_front();
    }
    int slot;
    if (!ingest_take(g, &slot, &u->first_ms, &u->n_ms, wait)) {
        if (g->io_errno) return fail(ctx, GYP_E_IO, std::string("gyp_ingest: read failed: ") + std::strerror(g->io_errno));
        return 0;
    }
    u->host_slot = slot;
    u->block = g->taken - 1;
    const int d = (int)(u->block % src.depth);
    // the device slot may hold an older block: everything the consumer has enqueued so far drains first (that is
    // the kernels of block k-1 when block k+1 is uploaded ahead, so the upload still overlaps block k's kernels)
    HIP_TRY(ctx, hipEventRecord(g->consumer_mark.get(), ctx->stream));
    HIP_TRY(ctx, hipStreamWaitEvent(copy, g->consumer_mark.get(), 0));
    float* iq = g->dev_iq[d].get();
    // the slot as the reader filled it, in file width (float32 at the output rate lands in the output slot directly); the host slot
    // is free again as soon as the copy is through, so `uploaded` stands directly behind it, ahead of the producer
    void* raw = src.raw_block_bytes ? (void*)g->dev_raw[d].get() : (void*)iq;
    const IngestSpan sp = ingest_span(src, g->file_samples, u->first_ms, u->n_ms);
    if (sp.slot_bytes()) HIP_TRY(ctx, hipMemcpyAsync(raw, g->host[slot], (size_t)sp.slot_bytes(), hipMemcpyHostToDevice, copy));
    HIP_TRY(ctx, hipEventRecord(g->uploaded[d].get(), copy));
    if (const int rc = ingest_produce(g, sp, *u, raw, iq)) return rc;
    if (const int lrc = ingest_condition(g, d, u->first_ms, u->n_ms)) return lrc;
    HIP_TRY(ctx, hipEventRecord(g->ready[d].get(), copy));
    g->in_flight.push_back(*u);
    ++g->dev_blocks;
    return 1;
}

// Python's round(x, 6) for the magnitudes a cursor/fs takes: correctly rounded decimal -> nearest double.
static double round6(double x) {
    char buf[64];
    std::snprintf(buf, sizeof buf, "%.6f", x);
    return std::strtod(buf, nullptr);
}

// Makes the handle of a described source: opens and measures the file, allocates the rings, starts the reader.  `who` is the entry
// point's name in the out-of-memory message.
static int ingest_finish_open(gyp_ctx* ctx, const IngestSource& src, int64_t fs, const char* path, gyp_ingest** out, const std::string& who) {
    gyp_ingest* g = new (std::nothrow) gyp_ingest(ctx, fs, src);
    if (!g) return fail(ctx, GYP_E_NOMEM, who + ": out of memory");
    if (const int e = ingest_open_file(g, path)) {
        ingest_free(g);
        return fail(ctx, GYP_E_IO, std::string("gyp_ingest_open: ") + path + ": " + std::strerror(e));
    }
    const int32_t depth = src.depth;
    const size_t block_bytes = src.host_block_bytes;
    g->host_mem.resize(depth);
    auto setup = [&]() -> int {
        if (!ctx) {
            for (int i = 0; i < depth; ++i) {
                void* m = nullptr;
                if (posix_memalign(&m, 4096, block_bytes)) return fail(ctx, GYP_E_NOMEM, "gyp_ingest_open: out of memory");
                g->host[i] = g->host_mem[i].adopt(m);
            }
            return GYP_OK;
        }
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        g->locality = device_locality(ctx->device);
        {
            ScopedAffinity on_the_gpus_node(g->locality);   // pinned pages land on the node of the thread that allocates them
            for (int i = 0; i < depth; ++i) {
                HIP_TRY(ctx, g->host_mem[i].alloc(block_bytes));
                g->host[i] = g->host_mem[i].get();
                std::memset(g->host[i], 0, block_bytes);     // first touch, still on that node
            }
        }
        HIP_TRY(ctx, g->copy_stream.create(hipStreamNonBlocking));
        g->dev_raw.resize(depth);
        g->dev_iq.resize(depth);
        g->uploaded.resize(depth);
        g->ready.resize(depth);
        for (int i = 0; i < depth; ++i) {
            HIP_TRY(ctx, g->blanked.ensure(i + 1, src.block_ms));   // (slot by slot, beside the slot's other buffers)
            HIP_TRY(ctx, g->dev_raw[i].reserve(src.raw_block_bytes, Slack::exact));
            HIP_TRY(ctx, g->dev_iq[i].reserve((size_t)src.block_ms * src.n * 2, Slack::exact));
            HIP_TRY(ctx, g->uploaded[i].create(hipEventDisableTiming));
            HIP_TRY(ctx, g->ready[i].create(hipEventDisableTiming));
        }
        HIP_TRY(ctx, g->consumer_mark.create(hipEventDisableTiming));
        return GYP_OK;
    };
    if (const int rc = setup()) {
        ingest_free(g);
        return rc;
    }
    ingest_start_reader(g, 0);
    *out = g;
    return GYP_OK;
}

// gyp_ingest_open_resampled (I,Q words) and gyp_ingest_open_ddc (real words at an IF): one handle type, the same reader, halo,
// ring and upload stream; `real` changes the bytes per sample and the kernel's staging policy.
static int ingest_open_filtered(gyp_ctx* ctx, const char* path, int32_t fmt, int64_t fs_in_hz, bool real, int64_t if_hz, int32_t taps,
                                int32_t block_ms, int32_t depth, gyp_ingest** out, const char* who) {
    if (!out) return fail(ctx, GYP_E_BAD_ARG, std::string(who) + ": out is NULL");
    *out = nullptr;
    if (!ctx) return fail(nullptr, GYP_E_BAD_ARG, std::string(who) + ": a context is required");
    const int wb = ingest_word_bytes(fmt);
    if (!path || !wb || block_ms < 1 || depth < 3 || depth > 64)
        return fail(ctx, GYP_E_BAD_ARG, std::string(who) + ": bad arguments (format, block_ms >= 1, 3 <= depth <= 64)");
    ResampleDesign d;
    if (const int rc = filter_design(ctx, fs_in_hz, real, if_hz, taps, &d, who)) return rc;
    return ingest_finish_open(ctx, ingest_describe(fmt, nullptr, d, if_hz, block_ms, depth), d.fs_out, path, out, who);
}

// The measurement of one stage over the handle's own device blocks of [first_ms, first_ms + n_ms): that stage and the ones behind it
// are put aside, so the blocks are what the stage would be given (Conditioning::upstream_of).  per_block(iq_dev, ms done, ms to take) is
// called for the blocks in order; after(next) does what follows the walk (downloads, host arithmetic, further launches on the context's
// stream) and may write the conditioning to install into `next`, which starts as the one found.  Then, whatever happened and in
// this order: the error text is saved (the seek overwrites ctx->err), the context's stream is synchronised (nothing may still read
// a block or a temporary), release() lets the caller's temporaries go, the conditioning becomes `next` on success and what it was
// otherwise, the cursor goes back to where it was, and the first error is reported with its own message.
template <class PerBlock, class After, class Release>
static int ingest_measure_range(gyp_ingest* g, int64_t first_ms, int32_t n_ms, Stage measured, const char* who, PerBlock per_block,
                                After after, Release release) {
    gyp_ctx* ctx = g->ctx;
    const Conditioning before = g->cond;
    const int64_t back_to = g->consumer_ms;
    Conditioning next = before;
    g->cond = before.upstream_of(measured);
    auto measure = [&]() -> int {
        if (const int rc = gyp_ingest_seek(g, first_ms)) return rc;
        for (int32_t done = 0; done < n_ms;) {
            const float* iq = nullptr;
            int64_t first = 0;
            int32_t count = 0;
            if (const int rc = gyp_ingest_next_dev(g, &iq, &first, &count)) return rc;
            if (count == 0 || first != first_ms + done) return fail(ctx, GYP_E_IO, std::string(who) + ": the recording ended inside the range");
            const int32_t take = std::min(count, n_ms - done);
            if (const int rc = per_block(iq, done, take)) return rc;
            done += take;
        }
        return after(next);
    };
    const int rc = measure();
    const std::string why = ctx->err;
    (void)hipStreamSynchronize(ctx->stream);
    release();
    g->cond = rc == GYP_OK ? next : before;
    const int rc_back = gyp_ingest_seek(g, back_to);
    return rc ? fail(ctx, rc, why) : rc_back;
}

// What the entry points that need the handle's device side open with: `what` says, in the refusal, why this one needs it.
static int ingest_device_handle(const gyp_ingest* g, const char* who, const char* what, gyp_ctx** ctx) {
    if (!g) return refuse(nullptr, who, "handle is NULL");
    if (!g->ctx) return refuse(nullptr, who, std::string("the handle was opened without a context (") + what + ")");
    *ctx = g->ctx;
    return GYP_OK;
}
// A measurement's range: whole milliseconds inside the recording, at most max_ms of them.
static int ingest_range_check(const gyp_ingest* g, const char* who, int64_t first_ms, int32_t n_ms, int32_t max_ms) {
    if (n_ms < 1 || n_ms > max_ms || first_ms < 0 || first_ms > g->total_ms - n_ms)
        return refuse(g->ctx, who, "[first_ms, first_ms + n_ms) must lie in [0, total_ms), 1 <= n_ms <= " + std::to_string(max_ms));
    return GYP_OK;
}
// A changed conditioning applies from the next block handed out: what was uploaded ahead carries the old one, so it is dropped and
// read again.
static int ingest_recondition(gyp_ingest* g) { return gyp_ingest_seek(g, g->consumer_ms); }

// The range of a measurement that wants it in one buffer (gyp_ingest_find_pulses, _find_excisor, _find_tones): the buffer, the copy
// of each block into it, the window over it on the context's stream, and the measurement itself.
struct GatheredRange {
    gyp_ingest* g;
    int64_t first_ms;
    int32_t n_ms;
    DevBuf<float> iq;   // the range's samples
    int64_t total() const { return (int64_t)n_ms * g->src.n; }
    hipError_t reserve() { return iq.reserve((size_t)total() * 2, Slack::exact); }
    IqWindow window() const { return ingest_window(g, iq.get(), nullptr, n_ms, first_ms, g->ctx->stream); }
    // ingest_measure_range of `measured`, gathering every block; what is released is the buffer, then the caller's temporaries
    template <class After, class Release>
    int measure(Stage measured, const char* who, After after, Release release_rest) {
        const size_t n = (size_t)g->src.n;
        return ingest_measure_range(
            g, first_ms, n_ms, measured, who,
            [&](const float* block, int32_t done, int32_t take) -> int {
                HIP_TRY(g->ctx, hipMemcpyAsync(iq.get() + 2 * (size_t)done * n, block, (size_t)take * n * 2 * sizeof(float), hipMemcpyDeviceToDevice, g->ctx->stream));
                return GYP_OK;
            },
            after, [&] { (void)iq.reset(), release_rest(); });
    }
};

// What the record-valued stages (level, blanker, excisor) have in common: the switch and the record in a Conditioning, and why
// their entry points need the handle's device side.  A stage that is switched off by its setter holds Conditioning{}'s record.
template <class T>
struct StageRecord { Stage stage; const char* applies; bool Conditioning::*on; T Conditioning::*rec; };
static const StageRecord<gyp_iq_level> kLevelRecord{Stage::level, "a level applies to device blocks", &Conditioning::level_on, &Conditioning::level};
static const StageRecord<gyp_blanker> kBlankerRecord{Stage::blanker, "a blanker applies to device blocks", &Conditioning::blank_on, &Conditioning::blanker};
static const StageRecord<gyp_excisor> kExcisorRecord{Stage::excisor, "an excisor applies to device blocks", &Conditioning::excise_on, &Conditioning::excisor};

// A counting stage's counts are made before it is first switched on, set or found: the blanker's at open, the excisor's here, so
// that a handle that never gets an excisor allocates nothing for it.
static int ingest_counts_made(gyp_ingest* g, Stage s) {
    SlotCounts* counts = g->counts_of(s);
    if (!counts || (int32_t)counts->dev.size() >= g->src.depth) return GYP_OK;
    HIP_TRY(g->ctx, hipSetDevice(g->ctx->device));
    HIP_TRY(g->ctx, counts->ensure(g->src.depth, g->src.block_ms));
    return GYP_OK;
}
// The limits of the two stages whose threshold is put a factor above a histogram's median; `why`, or the rate's refusal
struct HistStage { int32_t max_guard, max_samples; const char* too_wide; };
static const HistStage kBlankHist{kBlankMaxGuard, kBlankMaxSamples, "the blanker takes at most 65536 samples per millisecond"};
static const HistStage kExciseHist{kExciseMaxGuard, kExciseMaxSamples, "the excisor takes at most 65536 samples per millisecond"};
static const char* hist_stage_check(const char* why, const gyp_ingest* g, const HistStage& hs) {
    return why ? why : g->src.n > hs.max_samples ? hs.too_wide : nullptr;
}

// gyp_ingest_set_* and gyp_ingest_get_* of these stages: check() is why the stage does not take the record given, or nullptr
template <class T, class Check>
static int ingest_set_record(gyp_ingest* g, const char* who, const StageRecord<T>& st, const T* value, Check check) {
    gyp_ctx* ctx;
    if (const int rc = ingest_device_handle(g, who, st.applies, &ctx)) return rc;
    if (value) {
        if (const char* why = check()) return refuse(ctx, who, why);
        if (const int rc = ingest_counts_made(g, st.stage)) return rc;
    }
    g->cond.*st.on = value != nullptr;
    g->cond.*st.rec = value ? *value : Conditioning{}.*st.rec;
    return ingest_recondition(g);
}
template <class T>
static int ingest_get_record(const gyp_ingest* g, const char* who, const StageRecord<T>& st, T* out, int32_t* enabled_out) {
    gyp_ctx* ctx;
    if (const int rc = ingest_device_handle(g, who, st.applies, &ctx)) return rc;
    if (out) *out = g->cond.*st.rec;
    if (enabled_out) *enabled_out = g->cond.*st.on ? 1 : 0;
    return GYP_OK;
}

// gyp_ingest_last_blanked / _last_excised: the stage's counts of the block most recently handed out
template <class T>
static int ingest_last_counts(gyp_ingest* g, const char* who, const StageRecord<T>& st, int32_t* counts_out, int32_t cap, int32_t* n_ms_out) {
    gyp_ctx* ctx;
    if (const int rc = ingest_device_handle(g, who, st.applies, &ctx)) return rc;
    if (!n_ms_out || cap < 0 || (cap > 0 && !counts_out)) return refuse(ctx, who, "n_ms_out is NULL, or cap > 0 without counts_out");
    *n_ms_out = g->last_n_ms;
    const int32_t take = std::min(cap, g->last_n_ms);
    if (take <= 0 || g->last_slot < 0) return GYP_OK;
    const int d = g->last_slot;
    const SlotCounts& counts = *g->counts_of(st.stage);
    if (!counts.passed(d)) {
        std::fill(counts_out, counts_out + take, 0);
        return GYP_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, g->counts_stream.create(hipStreamNonBlocking));
    HIP_TRY(ctx, hipEventSynchronize(g->ready[d].get()));   // that block's chain only: not what was uploaded ahead
    HIP_TRY(ctx, hipMemcpyAsync(counts_out, counts.dev[d].get(), (size_t)take * sizeof(int32_t), hipMemcpyDeviceToHost, g->counts_stream.get()));
    HIP_TRY(ctx, hipStreamSynchronize(g->counts_stream.get()));
    return GYP_OK;
}

// gyp_ingest_find_pulses and gyp_ingest_find_excisor open alike, but for a HistStage's limits ...
static int hist_find_check(const gyp_ingest* g, const char* who, const HistStage& hs, int64_t first_ms, int32_t n_ms, double factor, int32_t guard,
                           gyp_ctx** ctx) {
    if (const int rc = ingest_device_handle(g, who, "the histogram is taken on the device", ctx)) return rc;
    if (const int rc = ingest_range_check(g, who, first_ms, n_ms, 1000)) return rc;
    if (!(factor > 0.0) || !std::isfinite(factor) || guard < 0 || guard > hs.max_guard)
        return refuse(*ctx, who, "threshold_over_median must be positive and finite, 0 <= guard <= " + std::to_string(hs.max_guard));
    const char* why = hist_stage_check(nullptr, g, hs);
    return why ? refuse(*ctx, who, why) : GYP_OK;
}
// ... and end alike over their gathered range: launch(window, hist_dev) enqueues the histogram, from_hist(hist, &found) derives the
// stage's record from it (nullptr, or the refusal's reason); the record is installed if asked and copied out.
template <class T, class Launch, class FromHist, class Release>
static int hist_find(GatheredRange& range, const char* who, const StageRecord<T>& st, int32_t install, T* out, Launch launch, FromHist from_hist,
                     Release release_rest) {
    gyp_ctx* ctx = range.g->ctx;
    DevBuf<uint32_t> hist_dev;
    HIP_TRY(ctx, hist_dev.reserve(GYP_POWER_HIST_BINS, Slack::exact));
    T found{};
    const int rc = range.measure(
        st.stage, who,
        [&](Conditioning& next) -> int {
            std::vector<uint32_t> hist(GYP_POWER_HIST_BINS);
            if (const int rc = launch(range.window(), hist_dev.get())) return rc;
            if (const int rc = fetch(ctx, hist, hist_dev.get())) return rc;
            if (const char* why = from_hist(hist.data(), &found)) return refuse(ctx, who, why);
            if (install) next.*st.on = true, next.*st.rec = found;
            return GYP_OK;
        },
        [&] { release_rest(), (void)hist_dev.reset(); });
    if (rc == GYP_OK && out) *out = found;
    return rc;
}

// gyp_ingest_find_tones over the gathered range: what is searched, the device buffers, the records last measured, what was found.
struct ToneSearch {
    GatheredRange range;
    double threshold;
    int32_t max_tones;
    DevBuf<gyp_tone_rec> recs_dev;
    std::vector<gyp_tone_rec> recs;   // block-major
    std::vector<int64_t> found;
    std::vector<double> found_db;
    int32_t n_scan() const { return (int32_t)(range.total() / kScanBlock); }
    int32_t n_fine() const { return (int32_t)(range.total() / kScanFine); }
};
constexpr int32_t kScanGrid = 2 * kScanHalf + 1;

// records of `freqs` over n_blocks blocks of block_samples samples of the gathered range, block-major, in ts.recs
static int tone_measure(ToneSearch& ts, const std::vector<int64_t>& freqs, int32_t n_blocks, int32_t block_samples, int32_t window) {
    gyp_ctx* ctx = ts.range.g->ctx;
    if (const int rc = tones_upload_freqs(ctx, freqs.data(), (int32_t)freqs.size(), ts.range.g->fs)) return rc;
    IqWindow w = ts.range.window();   // as n_blocks blocks of block_samples samples
    w.n_ms = n_blocks, w.n = block_samples;
    if (const int rc = tones_launch(ctx, w, ts.range.g->fs, (int32_t)freqs.size(), window, ts.recs_dev.get())) return rc;
    ts.recs.resize((size_t)n_blocks * freqs.size());
    return fetch(ctx, ts.recs, ts.recs_dev.get());
}
// one refinement step of every tone found: the phase slope over blocks of block_samples samples, rounded to whole Hz
static int tone_refine_found(ToneSearch& ts, int32_t n_blocks, int32_t block_samples, int32_t window) {
    const int64_t fs = ts.range.g->fs;
    std::vector<int64_t>& found = ts.found;
    if (const int rc = tone_measure(ts, found, n_blocks, block_samples, window)) return rc;
    std::vector<gyp_tone_rec> col((size_t)n_blocks);
    for (size_t t = 0; t < found.size(); ++t) {
        for (int32_t b = 0; b < n_blocks; ++b) col[(size_t)b] = ts.recs[(size_t)b * found.size() + t];
        const double delta = tone_refine(col.data(), n_blocks, (double)block_samples / (double)fs);
        const int64_t f = found[t] + (int64_t)std::llrint(delta);
        if (2 * (f < 0 ? -f : f) < fs) found[t] = f;
    }
    return GYP_OK;
}
// the scan, and its candidates without the offset at 0 Hz and without what the window leaks from it and from stronger tones
static int tone_scan(ToneSearch& ts) {
    gyp_ctx* ctx = ts.range.g->ctx;
    const int64_t fs = ts.range.g->fs;
    const int32_t n_scan = ts.n_scan();
    std::vector<int64_t> grid((size_t)kScanGrid);
    for (int32_t k = 0; k < kScanGrid; ++k) grid[(size_t)k] = scan_freq(k - kScanHalf, fs);
    if (const int rc = tone_measure(ts, grid, n_scan, kScanBlock, GYP_WINDOW_HANN)) return rc;
    std::vector<double> power((size_t)kScanGrid, 0.0);
    for (int32_t b = 0; b < n_scan; ++b)
        for (int32_t k = 0; k < kScanGrid; ++k) {
            const gyp_tone_rec& r = ts.recs[(size_t)b * kScanGrid + k];
            power[(size_t)k] += r.re * r.re + r.im * r.im;
        }
    for (double& p : power) p /= (double)n_scan;
    constexpr int32_t kMaxCand = 256;
    int32_t cand[kMaxCand];
    const char* why = nullptr;
    double median = 0.0;
    const int32_t min_sep = (int32_t)((kNotchMinSeparationHz * kScanDiv + fs - 1) / fs) + 2;
    const int32_t n_cand = tones_find(power.data(), kScanGrid, ts.threshold, min_sep, kMaxCand, cand, &why, &median);
    if (n_cand < 0) return fail(ctx, GYP_E_BAD_ARG, std::string("gyp_ingest_find_tones: the scan's spectrum: ") + why);
    std::vector<int32_t> kept;
    for (int32_t c = 0; c < n_cand && (int32_t)kept.size() < ts.max_tones; ++c) {
        const int32_t k = cand[c];
        if (std::abs(k - kScanHalf) < 4) continue;
        bool leak = power[(size_t)k] <= 4.0 * power[(size_t)kScanHalf] * scan_leakage(k - kScanHalf);
        for (const int32_t j : kept) leak = leak || power[(size_t)k] <= 4.0 * power[(size_t)j] * scan_leakage(k - j);
        if (!leak) kept.push_back(k);
    }
    for (const int32_t k : kept) {
        ts.found.push_back(grid[(size_t)k]);
        ts.found_db.push_back(10.0 * std::log10(power[(size_t)k] / median));
    }
    return GYP_OK;
}
// scan, then refine what was found: over the short blocks, and over whole milliseconds where there are two
static int tone_search(ToneSearch& ts) {
    if (const int rc = tone_scan(ts)) return rc;
    if (ts.found.empty()) return GYP_OK;
    // (Hann on the short blocks: behind a rectangular window of 64 samples an offset-binary file's offset or a stronger tone
    // leaks into a weak tone's records at -30 dB and below and bends its phase slope)
    if (const int rc = tone_refine_found(ts, ts.n_fine(), kScanFine, GYP_WINDOW_HANN)) return rc;
    if (ts.range.n_ms >= 2)
        if (const int rc = tone_refine_found(ts, ts.range.n_ms, ts.range.g->src.n, GYP_WINDOW_RECT)) return rc;
    return notch_check(ts.found.data(), (int32_t)ts.found.size(), ts.range.g->fs)
               ? fail(ts.range.g->ctx, GYP_E_BAD_ARG, "gyp_ingest_find_tones: two refined tones lie closer than 4000 Hz")
               : GYP_OK;
}

extern "C" {

int gyp_ingest_open(gyp_ctx* ctx, const char* path, int32_t fmt, int64_t fs_hz, int32_t n, int32_t block_ms,
                    int32_t depth, gyp_ingest** out) {
    if (!out) return fail(ctx, GYP_E_BAD_ARG, "gyp_ingest_open: out is NULL");
    *out = nullptr;
    const int wb = ingest_word_bytes(fmt);
    if (!path || !wb || fs_hz <= 0 || n <= 0 || block_ms < 1 || depth < 3 || depth > 64)
        return fail(ctx, GYP_E_BAD_ARG, "gyp_ingest_open: bad arguments (format, fs, n, block_ms >= 1, 3 <= depth <= 64)");
    if ((int64_t)n != fs_hz / 1000)   // antenna_sample_provider.py:135
        return fail(ctx, GYP_E_BAD_RATE, "gyp_ingest_open: n must be fs // 1000");
    return ingest_finish_open(ctx, ingest_describe(fmt, nullptr, ingest_unfiltered(n), 0, block_ms, depth), fs_hz, path, out, "gyp_ingest_open");
}

int gyp_ingest_open_resampled(gyp_ctx* ctx, const char* path, int32_t fmt, int64_t fs_in_hz, int32_t taps, int32_t block_ms,
                              int32_t depth, gyp_ingest** out) {
    return ingest_open_filtered(ctx, path, fmt, fs_in_hz, false, 0, taps, block_ms, depth, out, "gyp_ingest_open_resampled");
}

int gyp_ingest_open_ddc(gyp_ctx* ctx, const char* path, int32_t fmt, int64_t fs_in_hz, int64_t if_hz, int32_t taps, int32_t block_ms,
                        int32_t depth, gyp_ingest** out) {
    return ingest_open_filtered(ctx, path, fmt, fs_in_hz, true, if_hz, taps, block_ms, depth, out, "gyp_ingest_open_ddc");
}

int gyp_ingest_open_packed(gyp_ctx* ctx, const char* path, const gyp_packing* packing, int64_t fs_in_hz, int64_t if_hz, int32_t taps,
                           int32_t block_ms, int32_t depth, gyp_ingest** out) {
    const char* who = "gyp_ingest_open_packed";
    if (!out) return fail(ctx, GYP_E_BAD_ARG, std::string(who) + ": out is NULL");
    *out = nullptr;
    if (!ctx) return fail(nullptr, GYP_E_BAD_ARG, std::string(who) + ": a context is required");
    PackedFormat pk;
    if (const char* why = packing_check(packing, &pk)) return fail(ctx, GYP_E_BAD_ARG, std::string(who) + ": " + why);
    if (pk.real != (if_hz != 0)) return fail(ctx, GYP_E_BAD_ARG, std::string(who) + ": real words need if_hz != 0, I,Q words if_hz = 0");
    if (!path || block_ms < 1 || depth < 3 || depth > 64)
        return fail(ctx, GYP_E_BAD_ARG, std::string(who) + ": bad arguments (path, block_ms >= 1, 3 <= depth <= 64)");
    if (!ctx->fs) return fail(ctx, GYP_E_NO_FORMAT, std::string(who) + ": " + kNoFormat);
    const bool native = !pk.real && fs_in_hz == ctx->fs;
    const float* levels = nullptr;   // uploaded now, not on the copy stream's first block
    if (const int rc = packed_levels_dev(ctx, pk, &levels)) return rc;
    ResampleDesign d = ingest_unfiltered((int32_t)(ctx->fs / 1000));
    if (!native)
        if (const int rc = filter_design(ctx, fs_in_hz, pk.real, if_hz, taps, &d, who)) return rc;
    return ingest_finish_open(ctx, ingest_describe(0, &pk, d, if_hz, block_ms, depth), ctx->fs, path, out, who);
}

int gyp_device_locality(gyp_ctx* ctx, int32_t* numa_node_out, char* cpulist_out, int32_t cap) {
    if (!ctx) return GYP_E_BAD_ARG;
    const HostLocality loc = device_locality(ctx->device);
    if (numa_node_out) *numa_node_out = loc.numa_node;
    if (cpulist_out && cap > 0) {
        // a list that does not fit is cut at a comma, never in the middle of a range (a truncated "128-1" would bind to the wrong CPUs)
        std::string text = loc.cpulist;
        if ((int)text.size() >= cap) {
            const size_t cut = text.rfind(',', (size_t)cap - 1);
            text = cut == std::string::npos ? std::string() : text.substr(0, cut);
        }
        std::snprintf(cpulist_out, (size_t)cap, "%s", text.c_str());
    }
    return GYP_OK;
}

void gyp_ingest_close(gyp_ingest* ing) {
    if (ing) ingest_free(ing);
}

int64_t gyp_ingest_total_ms(const gyp_ingest* ing) { return ing ? ing->total_ms : 0; }

int gyp_ingest_set_scale(gyp_ingest* g, float scale) {
    if (!g) return fail(nullptr, GYP_E_BAD_ARG, "gyp_ingest_set_scale: handle is NULL");
    if (!(scale > 0.0f) || !std::isfinite(scale)) return fail(g->ctx, GYP_E_BAD_ARG, "gyp_ingest_set_scale: scale must be positive and finite");
    if (!g->src.packed() && g->src.fmt == kFmtF32) return fail(g->ctx, GYP_E_BAD_ARG, "gyp_ingest_set_scale: float32 recordings are uploaded as they are");
    g->scale = scale;
    return GYP_OK;
}

int gyp_ingest_seek(gyp_ingest* g, int64_t ms) {
    if (!g) return fail(nullptr, GYP_E_BAD_ARG, "gyp_ingest_seek: handle is NULL");
    if (ms < 0 || ms > g->total_ms) return fail(g->ctx, GYP_E_BAD_ARG, "gyp_ingest_seek: millisecond out of range");
    ingest_stop_reader(g);
    if (g->ctx) {
        HIP_TRY(g->ctx, hipStreamSynchronize(g->copy_stream.get()));
        g->in_flight.clear();
        g->have_ahead = false;
        g->last_slot = -1;   // (ingest_last_counts: the slots are about to be refilled)
        g->last_n_ms = 0;
    }
    ingest_start_reader(g, ms);
    g->consumer_ms = ms;
    return GYP_OK;
}

int gyp_ingest_next_host(gyp_ingest* g, const void** raw_out, int64_t* first_ms_out, int32_t* n_ms_out) {
    if (!g || !raw_out || !first_ms_out || !n_ms_out) return fail(g ? g->ctx : nullptr, GYP_E_BAD_ARG, "gyp_ingest_next_host: NULL argument");
    *raw_out = nullptr;
    *n_ms_out = 0;
    if (g->src.filtered()) return fail(g->ctx, GYP_E_BAD_ARG, "gyp_ingest_next_host: a resampled handle has no host blocks (gyp_ingest_next_dev)");
    if (g->src.packed()) return fail(g->ctx, GYP_E_BAD_ARG, "gyp_ingest_next_host: a packed handle has no host blocks (gyp_ingest_next_dev)");
    static const struct { Stage stage; const char* is_on; } kAsked[] = {   // in the order this call has always asked, not the chain's
        {Stage::level, "a level is on"}, {Stage::notches, "notches are on"}, {Stage::blanker, "a blanker is on"}, {Stage::excisor, "an excisor is on"}};
    for (const auto& a : kAsked)
        if (g->cond.on(a.stage))
            return fail(g->ctx, GYP_E_BAD_ARG, std::string("gyp_ingest_next_host: ") + a.is_on + ", and host blocks are raw file words (gyp_ingest_next_dev)");
    if (g->ctx && (!g->in_flight.empty() || g->have_ahead))
        return fail(g->ctx, GYP_E_BAD_ARG, "gyp_ingest_next_host: device blocks are in flight on this handle; seek first");
    ingest_release(g, g->taken);   // the block handed out by the previous call may be overwritten now
    int slot;
    if (!ingest_take(g, &slot, first_ms_out, n_ms_out, true)) {
        *n_ms_out = 0;
        if (g->io_errno) return fail(g->ctx, GYP_E_IO, std::string("gyp_ingest: read failed: ") + std::strerror(g->io_errno));
        return GYP_OK;
    }
    *raw_out = g->host[slot];
    g->consumer_ms = *first_ms_out + *n_ms_out;
    return GYP_OK;
}

int gyp_ingest_next_dev(gyp_ingest* g, const float** iq_dev_out, int64_t* first_ms_out, int32_t* n_ms_out) {
    if (!g || !iq_dev_out || !first_ms_out || !n_ms_out) return fail(g ? g->ctx : nullptr, GYP_E_BAD_ARG, "gyp_ingest_next_dev: NULL argument");
    *iq_dev_out = nullptr;
    *n_ms_out = 0;
    gyp_ctx* ctx = g->ctx;
    if (!ctx) return fail(nullptr, GYP_E_NO_DEVICE, "gyp_ingest_next_dev: the handle was opened without a context");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    gyp_ingest::Upload cur{};
    if (g->have_ahead) {
        cur = g->ahead;
        g->have_ahead = false;
    } else {
        const int rc = ingest_enqueue_upload(g, &cur, true);
        if (rc < 0) return rc;
        if (rc == 0) return GYP_OK;   // end of data
    }
    // start the next block's upload now if the reader already has it: it then overlaps this block's kernels
    const int rc = ingest_enqueue_upload(g, &g->ahead, false);
    if (rc < 0) return rc;
    g->have_ahead = rc == 1;
    const int d = (int)(cur.block % g->src.depth);
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, g->ready[d].get(), 0));
    // hand back host slots whose upload has finished
    while (!g->in_flight.empty() && hipEventQuery(g->uploaded[g->in_flight.front().block % g->src.depth].get()) == hipSuccess) {
        ingest_release(g, g->in_flight.front().block + 1);
        g->in_flight.pop_front();
    }
    *iq_dev_out = g->dev_iq[d].get();
    *first_ms_out = cur.first_ms;
    *n_ms_out = cur.n_ms;
    g->consumer_ms = cur.first_ms + cur.n_ms;
    g->last_slot = d;
    g->last_n_ms = cur.n_ms;
    return GYP_OK;
}

int gyp_widen_iq_dev(gyp_ctx* ctx, int32_t fmt, const void* raw_dev, uint64_t n_words, float scale, float* out_dev) {
    if (!ctx || !raw_dev || !out_dev) return ctx ? fail(ctx, GYP_E_BAD_ARG, "gyp_widen_iq_dev: bad argument") : GYP_E_BAD_ARG;
    if (n_words == 0) return GYP_OK;
    if (fmt != GYP_FMT_I8 && fmt != GYP_FMT_U8 && fmt != GYP_FMT_I16)
        return fail(ctx, GYP_E_BAD_ARG, "gyp_widen_iq_dev: fmt must be GYP_FMT_I8, GYP_FMT_U8 or GYP_FMT_I16");
    widen_launch(ctx, ctx->stream, fmt, raw_dev, (size_t)n_words, scale, out_dev);
    HIP_TRY(ctx, hipGetLastError());
    return GYP_OK;
}

int gyp_ingest_set_level(gyp_ingest* g, const gyp_iq_level* level) {
    return ingest_set_record(g, "gyp_ingest_set_level", kLevelRecord, level, [&] { return level_check(level); });
}

int gyp_ingest_get_level(const gyp_ingest* g, gyp_iq_level* out, int32_t* enabled_out) {
    return ingest_get_record(g, "gyp_ingest_get_level", kLevelRecord, out, enabled_out);
}

int gyp_ingest_calibrate(gyp_ingest* g, int64_t first_ms, int32_t n_ms, int32_t remove_dc, double target_rms, float clip_level,
                         gyp_iq_level* level_out, double* measured_out4) {
    const char* who = "gyp_ingest_calibrate";
    gyp_ctx* ctx;
    if (const int rc = ingest_device_handle(g, who, "the statistics are taken on the device", &ctx)) return rc;
    if (const int rc = ingest_range_check(g, who, first_ms, n_ms, 10000)) return rc;
    if (!(target_rms > 0.0) || !std::isfinite(target_rms)) return refuse(ctx, who, "target_rms must be positive and finite");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevBuf<gyp_iq_stats> stats_dev;
    HIP_TRY(ctx, stats_dev.reserve((size_t)n_ms, Slack::exact));
    gyp_iq_stats* d_stats = stats_dev.get();
    std::vector<gyp_iq_stats> stats((size_t)n_ms);
    gyp_iq_level level{};
    // the level is put aside: the blocks measured are the handle's output without it (blanker, excisor and notches stay)
    const int rc = ingest_measure_range(
        g, first_ms, n_ms, Stage::level, who,
        [&](const float* iq, int32_t done, int32_t take) {
            return stats_launch(ctx, ingest_window(g, iq, nullptr, take, 0, ctx->stream), clip_level, d_stats + done);
        },
        [&](Conditioning& next) -> int {
            if (const int rc = fetch(ctx, stats, d_stats)) return rc;
            if (const char* why = level_from_stats(stats.data(), n_ms, g->src.n, remove_dc, target_rms, &level, measured_out4))
                return refuse(ctx, who, why);
            next.level_on = true;
            next.level = level;
            return GYP_OK;
        },
        [&] { (void)stats_dev.reset(); });
    if (rc) return rc;
    if (level_out) *level_out = level;
    return GYP_OK;
}

int gyp_ingest_set_notches(gyp_ingest* g, const int64_t* freqs_hz, int32_t n) {
    const char* who = "gyp_ingest_set_notches";
    gyp_ctx* ctx;
    if (const int rc = ingest_device_handle(g, who, "notches apply to device blocks", &ctx)) return rc;
    if (!freqs_hz) n = 0;
    if (const char* why = notch_check(freqs_hz, n, g->fs)) return refuse(ctx, who, why);
    gyp_notch_tones t{};
    t.count = n;
    for (int32_t i = 0; i < n; ++i) t.freq_hz[i] = freqs_hz[i];
    g->cond.notches = t;
    return ingest_recondition(g);
}

int gyp_ingest_get_notches(const gyp_ingest* g, int64_t* freqs_out8, int32_t* n_out) {
    gyp_ctx* ctx;
    if (const int rc = ingest_device_handle(g, "gyp_ingest_get_notches", "notches apply to device blocks", &ctx)) return rc;
    if (freqs_out8)
        for (int32_t i = 0; i < g->cond.notches.count; ++i) freqs_out8[i] = g->cond.notches.freq_hz[i];
    if (n_out) *n_out = g->cond.notches.count;
    return GYP_OK;
}

int gyp_ingest_find_tones(gyp_ingest* g, int64_t first_ms, int32_t n_ms, double threshold, int32_t max_tones, int32_t install,
                          int64_t* freqs_out, double* power_db_out, int32_t* n_out) {
    const char* who = "gyp_ingest_find_tones";
    gyp_ctx* ctx;
    if (const int rc = ingest_device_handle(g, who, "the scan runs on the device", &ctx)) return rc;
    if (!n_out) return refuse(ctx, who, "n_out is NULL");
    *n_out = 0;
    if (const int rc = ingest_range_check(g, who, first_ms, n_ms, 1000)) return rc;
    if (!(threshold > 0.0) || !std::isfinite(threshold) || max_tones < 1 || max_tones > GYP_NOTCH_MAX_TONES)
        return refuse(ctx, who, "threshold must be positive and finite, 1 <= max_tones <= 8");
    ToneSearch ts{{g, first_ms, n_ms}, threshold, max_tones};
    if (!tone_rate_ok(g->fs) || ts.range.total() < kScanBlock)
        return refuse(ctx, who, "the range must hold at least 1024 samples at a rate in [1000, 2^31) Hz");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, ts.range.reserve());
    HIP_TRY(ctx, ts.recs_dev.reserve(std::max<size_t>((size_t)ts.n_scan() * kScanGrid, (size_t)ts.n_fine() * GYP_NOTCH_MAX_TONES), Slack::exact));
    // the blocks gathered are the producer's output behind the blanker and the excisor, where they are on: no notches, no level
    if (const int rc = ts.range.measure(
            Stage::notches, who,
            [&](Conditioning& next) -> int {
                if (const int rc = tone_search(ts)) return rc;
                if (install) {
                    next.notches = gyp_notch_tones{};
                    next.notches.count = (int32_t)ts.found.size();
                    for (size_t t = 0; t < ts.found.size(); ++t) next.notches.freq_hz[t] = ts.found[t];
                }
                return GYP_OK;
            },
            [&] { (void)ts.recs_dev.reset(); }))
        return rc;
    for (size_t t = 0; t < ts.found.size(); ++t) {
        if (freqs_out) freqs_out[t] = ts.found[t];
        if (power_db_out) power_db_out[t] = ts.found_db[t];
    }
    *n_out = (int32_t)ts.found.size();
    return GYP_OK;
}

int gyp_ingest_set_blanker(gyp_ingest* g, const gyp_blanker* blanker) {
    return ingest_set_record(g, "gyp_ingest_set_blanker", kBlankerRecord, blanker,
                             [&] { return hist_stage_check(blanker_check(blanker), g, kBlankHist); });
}

int gyp_ingest_get_blanker(const gyp_ingest* g, gyp_blanker* out, int32_t* enabled_out) {
    return ingest_get_record(g, "gyp_ingest_get_blanker", kBlankerRecord, out, enabled_out);
}

int gyp_ingest_find_pulses(gyp_ingest* g, int64_t first_ms, int32_t n_ms, int32_t remove_dc, double threshold_over_median, int32_t guard,
                           int32_t install, gyp_blanker* blanker_out, double* measured_out2) {
    const char* who = "gyp_ingest_find_pulses";
    gyp_ctx* ctx;
    if (const int rc = hist_find_check(g, who, kBlankHist, first_ms, n_ms, threshold_over_median, guard, &ctx)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    GatheredRange range{g, first_ms, n_ms};
    DevBuf<gyp_iq_stats> stats_dev;
    HIP_TRY(ctx, range.reserve());
    HIP_TRY(ctx, stats_dev.reserve((size_t)n_ms, Slack::exact));
    float centre[2] = {0.0f, 0.0f};
    // the blocks gathered are the producer's output: no blanker, no excisor, no notches, no level
    return hist_find(
        range, who, kBlankerRecord, install, blanker_out,
        [&](const IqWindow& w, uint32_t* hist_dev) -> int {   // about the range's mean, where asked
            if (remove_dc) {
                std::vector<gyp_iq_stats> stats((size_t)n_ms);
                if (const int rc = stats_launch(ctx, w, 0.0f, stats_dev.get())) return rc;
                if (const int rc = fetch(ctx, stats, stats_dev.get())) return rc;
                const IqMean mean = mean_from_stats(stats.data(), n_ms, w.n);
                centre[0] = (float)mean.re;
                centre[1] = (float)mean.im;
                if (!std::isfinite(centre[0]) || !std::isfinite(centre[1])) return refuse(ctx, who, "the range's mean is not finite");
            }
            return hist_launch(ctx, w, range.total(), centre, hist_dev);
        },
        [&](const uint32_t* hist, gyp_blanker* found) {
            return blank_from_hist(hist, centre[0], centre[1], threshold_over_median, guard, found, measured_out2);
        },
        [&] { (void)stats_dev.reset(); });
}

int gyp_ingest_last_blanked(gyp_ingest* g, int32_t* counts_out, int32_t cap, int32_t* n_ms_out) {
    return ingest_last_counts(g, "gyp_ingest_last_blanked", kBlankerRecord, counts_out, cap, n_ms_out);
}

int gyp_ingest_set_excisor(gyp_ingest* g, const gyp_excisor* excisor) {
    return ingest_set_record(g, "gyp_ingest_set_excisor", kExcisorRecord, excisor,
                             [&] { return hist_stage_check(excisor_check(excisor), g, kExciseHist); });
}

int gyp_ingest_get_excisor(const gyp_ingest* g, gyp_excisor* out, int32_t* enabled_out) {
    return ingest_get_record(g, "gyp_ingest_get_excisor", kExcisorRecord, out, enabled_out);
}

int gyp_ingest_find_excisor(gyp_ingest* g, int64_t first_ms, int32_t n_ms, double threshold_over_median, int32_t guard, int32_t install,
                            gyp_excisor* excisor_out, double* measured_out2) {
    const char* who = "gyp_ingest_find_excisor";
    gyp_ctx* ctx;
    if (const int rc = hist_find_check(g, who, kExciseHist, first_ms, n_ms, threshold_over_median, guard, &ctx)) return rc;
    if (g->src.n < GYP_EXCISE_FRAME) return refuse(ctx, who, "the histogram needs at least 256 samples per millisecond");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (install)
        if (const int rc = ingest_counts_made(g, Stage::excisor)) return rc;
    GatheredRange range{g, first_ms, n_ms};
    HIP_TRY(ctx, range.reserve());
    // the blocks gathered are the producer's output behind the blanker, where one is on: no excisor, no notches, no level
    return hist_find(
        range, who, kExcisorRecord, install, excisor_out,
        [&](const IqWindow& w, uint32_t* hist_dev) { return spectrum_hist_launch(ctx, w, hist_dev); },
        [&](const uint32_t* hist, gyp_excisor* found) { return excise_from_hist(hist, threshold_over_median, guard, found, measured_out2); }, [] {});
}

int gyp_ingest_last_excised(gyp_ingest* g, int32_t* counts_out, int32_t cap, int32_t* n_ms_out) {
    return ingest_last_counts(g, "gyp_ingest_last_excised", kExcisorRecord, counts_out, cap, n_ms_out);
}

int gyp_ingest_times(const gyp_ingest* g, int64_t first_ms, int32_t n_ms, double* start_out, double* end_out) {
    if (!g || n_ms < 0 || first_ms < 0 || (n_ms > 0 && (!start_out || !end_out)))
        return fail(g ? g->ctx : nullptr, GYP_E_BAD_ARG, "gyp_ingest_times: bad arguments");
    for (int32_t i = 0; i < n_ms; ++i) {
        const int64_t cursor = (first_ms + i) * g->src.n;
        start_out[i] = round6((double)cursor / (double)g->fs);
        end_out[i] = round6((double)(cursor + g->src.n) / (double)g->fs);
    }
    return GYP_OK;
}

}  // extern "C"
