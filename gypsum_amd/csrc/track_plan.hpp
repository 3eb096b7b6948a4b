// track_plan.hpp -- what a gyp_track_block_dev call runs for a bank and a block: which flow, the sub-blocks and rounds of a speculative
// block, the throughput kernel's launches, the exact-sums kernel, the confidence threshold.  Plain C++17 and a pure function of the shape
// and the A/B switches: no HIP call, no context, no bank (tests/track_plan_model.py restates it; tests/test_host_sanitizers.py sweeps one
// against the other).  Include after kernels.hpp: SubLayout, kMaxSubBlocks and kExactGroupMaxChan are the kernels' own.
#pragma once
#include <algorithm>
#include <cmath>

namespace gyp {

struct TrackShape { int k, n, n_cus, n_chan, n_ms; bool keep_profiles; };   // samples per chip and per millisecond; the bank; the block; gyp_bank_keep_profiles depth > 0
struct TrackSwitches { bool no_pipe, no_spec, spec_redo; int spec_sub_ms, track_chunk_ms; bool no_exact_shared; double spec_confidence_kappa; };   // gyp_debug_set names; gyp_params
struct TrackPlan {
    int flow;          // 1 throughput kernel, 2 speculative with the re-run at the end (r03 form), 3 speculative under the round protocol (gyp_debug_get "last_track_flow")
    SubLayout layout;  // sub-blocks of a speculative block (none() in flow 1)
    int rounds;        // flow 3: tracking launches; flow 2: 1 (the round tables keep one row); flow 1: 0
    int chunk_ms, launches;   // the throughput kernel's launch length and launches (a speculative block's re-run of failed channels: one, whole)
    int exact_path;    // the exact-sums kernel beside the throughput kernel: 1 dll_exact_wave_kernel, 2 dll_exact_shared_kernel, 3 dll_exact_block_kernel
    float spec_kappa;  // TrackBlockParams::spec_kappa of every launch of the call
};

// Sub-blocks of a speculative block: the last sub-block's verification trails the tracking, and a failed verification costs a
// sub-block (more, shorter ones for long blocks); each round re-reads the channel state and the tables (~20 us).
constexpr int kMaxSub = 20;
inline int spec_sub_ms_for(int k, int spec_sub_ms) { return spec_sub_ms >= 100 ? spec_sub_ms : (k == 2 ? 167 : 500); }   // gyp_debug_set "spec_sub_ms": 0 (and 1..99) = by rate
// ... and their lengths: equal ones, except that a block of sub-blocks of >= 160 ms ends with three shrinking ones (0.56, 0.34 and
// 0.20 of the usual length) in place of its last one (SubLayout: only the last sub-block's verification is not hidden behind tracking;
// each piece is ~0.6 of the one before because round R waits for the verification of round R - 2, which takes about half as long
// as the tracking of the same milliseconds at 16.368 Msps and a third at 8.184).
inline SubLayout spec_layout(int n_ms, int sub_ms) {   // sub_ms: target sub-block length
    const int cap = sub_ms == 500 ? kMaxSub : kMaxSubBlocks - 2;   // (a layout ends with two more, shrinking, sub-blocks: SubLayout holds 32)
    const int n_sub = n_ms >= 2048 ? std::min(cap, std::max(4, n_ms / sub_ms)) : (n_ms >= 256 ? 4 : 1);
    SubLayout l = SubLayout::none();
    const int len = (n_ms + n_sub - 1) / n_sub;
    int at = 0;
    auto push = [&](int piece) {
        if (piece <= 0 || at >= n_ms || l.n >= kMaxSubBlocks) return;
        piece = std::min(piece, n_ms - at);
        l.start[l.n++] = at;
        l.longest = std::max(l.longest, piece);
        at += piece;
    };
    if (n_sub > 1 && len >= 160) {
        const int t1 = (56 * len + 99) / 100, t2 = (34 * len + 99) / 100, t3 = std::max(32, len / 5);
        const int body = n_ms - (t1 + t2 + t3), piece = (body + n_sub - 2) / (n_sub - 1);
        for (int j = 0; j < n_sub - 1; ++j) push(piece);
        push(t1); push(t2);
        push(n_ms - at);
    } else {
        for (int j = 0; j < n_sub; ++j) push(len);
    }
    for (int i = l.n; i <= kMaxSubBlocks; ++i) l.start[i] = n_ms;
    return l;
}

// The rounds couple the tracking launches to the verify launches two rounds back, so the verify kernels must keep up beside the
// tracking -- on the CUs the channels leave free, one workgroup per CU (launch_track_verify).  That holds for a receiver's bank
// (12 channels: verify 0.4 ms per 500-ms round against 2 ms of tracking) and up to about two streams; beyond, the verify launches
// become the bottleneck (tools/mid_bank_probe.sh: 48 channels 5.5 against 4.7 ms per 1000 ms, 252 channels 109 against 16), and
// those banks keep r03's flow, in which nothing waits for the verification until the end of the block.
constexpr int kMaxRoundProtocolChannels = 24;

inline TrackPlan track_plan(const TrackShape& s, const TrackSwitches& sw) {
    TrackPlan pl{};
    pl.spec_kappa = (float)sw.spec_confidence_kappa;
    const bool light = (s.k == 8 || s.k == 2 || s.k == 16) && s.n_chan <= s.n_cus && !sw.no_pipe;   // one workgroup per CU anyway
    // (profiles kept: the transform kernel forms every millisecond's full profile anyway)
    if (s.keep_profiles || !light || sw.no_spec) {
        pl.flow = 1;
        // The channels of a stream are independent workgroups that read the same samples; nothing keeps them within an L2's worth
        // (~11 ms of an XCD's resident streams) of each other, and over a 1000-ms launch they drift apart: FETCH_SIZE per
        // millisecond is 1.24x the algorithmic bytes for launches of <= 250 ms and 2.6x for 1000 ms (profiles/r03_drift.txt).  A
        // launch boundary is a rendezvous: long blocks go through in chunks (the loop state travels in ChanState anyway, and a block
        // gives the same records however it is cut).  r03-r05: 500 ms (1.3-1.5x).  How far the workgroups of a stream drift depends on
        // their relative pace, and with the staging instructions of r06's gain correction 500-ms launches counted 2.0x at an unchanged
        // kernel time (profiles/r06_experiments.txt item 9).  r06: 250 ms (the default of "track_chunk_ms") -- 1.29x, the same 58.6 ms
        // of tracking kernels per 1536-channel x 1000-ms step (125 ms: 1.23x), resident throughput unchanged; the price is a host-fed
        // pipeline's overlap -- the chip drains at every boundary and the upload stream's widen kernel takes it whole: int8-fed
        // 0.960 -> 0.938 of the resident rate (profiles/r06zf_chunk_sweep.txt, r06zf_chunk_legs.txt).
        pl.chunk_ms = sw.track_chunk_ms <= 0 ? s.n_ms : sw.track_chunk_ms;
        // at 8 samples per chip the channels are grouped by stream and each (group, millisecond) is staged once (dll_exact_shared_kernel)
        pl.exact_path = s.k == 8 && !sw.no_exact_shared && s.n_chan <= kExactGroupMaxChan ? 2 : (s.k <= 8 ? 1 : 3);
    } else {
        pl.layout = spec_layout(s.n_ms, spec_sub_ms_for(s.k, sw.spec_sub_ms));
        const int n_sub = pl.layout.n;
        // r03 form: blocks of one sub-block, gyp_debug_set "spec_redo" 0, banks beyond the round protocol's reach
        pl.flow = n_sub == 1 || !sw.spec_redo || s.n_chan > kMaxRoundProtocolChannels ? 2 : 3;
        // a re-do costs its channel two rounds: room for three of them behind the last sub-block, then the transform kernel takes over
        pl.rounds = pl.flow == 3 ? n_sub + 2 + (n_sub >= 8 ? 6 : 2) : 1;
        pl.chunk_ms = s.n_ms;   // the re-run of failed channels: one launch, the per-channel exact sums
        pl.exact_path = s.k <= 8 ? 1 : 3;
        // gyp_params::spec_confidence_kappa is quoted for 8184 lags: the chance that some noise lag beats a peak of kappa x the sample
        // energy is (number of lags) x exp(-kappa), so a rate with fewer lags reaches the same risk at a lower threshold (2.046 Msps:
        // 20 -> 18.6, which moves ~5 % of its milliseconds from the in-kernel transform path to the fast path; 16.368 Msps: 20.7)
        // r06, 2.046 Msps only: a further -5 (20 -> 13.6) together with sub-blocks of ~167 ms instead of ~500 (spec_sub_ms_for).  At two
        // samples per chip a millisecond that fails the test runs its transforms on TWO of the workgroup's eight wavefronts (~15 us against
        // 2.9 on the fast path), and a verification that fails costs its channel one short sub-block: measured on five scenes / seeds at
        // a N = 18..41, sigma = 6 a (tools/kappa_sweep.py, profiles/r06_experiments.txt item 2): 180-205 x -> 217-245 x real time, SURVEY d2's
        // cfg2 scene 316 -> 320 x.  8.184 / 16.368 Msps: no difference within the noise of the measurement, left alone.
        const double kappa_rate = std::log((double)s.n / 8184.0) + (s.k == 2 ? -5.0 : 0.0);
        pl.spec_kappa = (float)std::max(0.0, sw.spec_confidence_kappa + (sw.spec_confidence_kappa > 0.0 ? kappa_rate : 0.0));
    }
    pl.launches = (s.n_ms + pl.chunk_ms - 1) / pl.chunk_ms;
    return pl;
}

}  // namespace gyp
