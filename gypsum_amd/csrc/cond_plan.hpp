// cond_plan.hpp -- what the conditioning stages behind the sample path launch for a shape: the statistics, level, tone, notch,
// blanker, excisor, histogram and quality kernels, and the widen and unpack kernels whose persistent grid they share.  A call of n streams
// (channels) is cut into launches of at most k, because a launch's per-stream parameters travel by value in a kernel argument; a
// plan says how many launches, which streams each takes, its grid, its dynamic LDS and whether rows are accessed 16 bytes at a time.
// Plain C++17 and pure functions of their arguments: no HIP type, no context, addresses as uintptr_t
// (tests/cond_plan_model.py restates them; tests/test_host_sanitizers.py sweeps one against the other).
#pragma once
#include <algorithm>
#include <cstdint>

namespace gyp {

// The persistent grid.  These kernels read 8 bytes per sample once and are HBM-bound; on the upload stream they run BESIDE the
// previous block's tracking kernels.  With 8 workgroups per CU the widen kernel took the chip at every launch boundary of the
// trackers; 2 per CU (gyp_debug_set "widen_wg_per_cu", 1..8) leave them their slots -- int8-fed / resident 0.934-0.942 ->
// 0.949-0.953 (profiles/r06zi / r06zj_widen_grid.txt).  Every conditioning stage on that stream walks a grid of at most this many
// workgroups, whatever the call's size; the output's bits do not depend on it.
inline int64_t persistent_cap(int n_cus, int wg_per_cu) { return (int64_t)n_cus * wg_per_cu; }

// The three shapes of a capped grid.  Item counts are 64-bit and narrowed to int only here.
// One workgroup per item (a (stream, millisecond), a (stream, block, frequency)): items >= 1.
inline int grid_per_item(int64_t items, int64_t cap) { return (int)std::min<int64_t>(items, cap); }
// grid (x, ns): ns streams side by side share the cap, each row of v elements walked by x workgroups of 256 threads; at least 1.
inline int grid_per_row(int64_t v, int64_t cap, int32_t ns) {
    return (int)std::max<int64_t>(1, std::min<int64_t>((v + 255) / 256, std::max<int64_t>(1, cap / ns)));
}
// The widen kernel: 16 words per thread, and one workgroup more for the words behind the last whole 16.
inline unsigned grid_widen(uint64_t n_words, int64_t cap) { return (unsigned)std::min<uint64_t>((n_words / 16 + 255) / 256 + 1, (uint64_t)cap); }

enum class GridRule : int32_t {
    per_item,   // grid_per_item over ns * per_stream items
    per_row,    // grid_per_row over one row of per_stream elements, grid.y = ns
    per_quad,   // four items per workgroup (one wavefront each): min(ceil(items / 4), cap)
};

// One stage's call.  Chunk i takes streams i * k .. and is launched as stage_chunk(plan, i) says.
struct StagePlan {
    int32_t n, k;         // n streams (channels) in launches of at most k
    int32_t n_chunks;
    GridRule rule;
    int64_t per_stream;   // per_item / per_quad: one stream's items; per_row: one row's elements (vec4: float4s, else float2s)
    int64_t cap;          // workgroups one launch may take
    int64_t lds_bytes;    // dynamic LDS of every launch
    int32_t vec4;         // rows are read and written 16 bytes at a time (every row starts 16-byte aligned)
};
struct StageChunk {
    int32_t s0, ns;       // the launch's streams: s0 .. s0 + ns - 1
    int grid_x, grid_y;
    int64_t items;        // what grid_x is spread over: the launch's items, or one row's elements
};

inline StagePlan stage_plan(int32_t n, int32_t k, GridRule rule, int64_t per_stream, int64_t cap) {
    return StagePlan{n, k, (int32_t)(((int64_t)n + k - 1) / k), rule, per_stream, cap, 0, 0};
}
inline StageChunk stage_chunk(const StagePlan& p, int32_t i) {
    const int32_t s0 = i * p.k, ns = std::min<int32_t>(p.k, p.n - s0);
    if (p.rule == GridRule::per_row) return StageChunk{s0, ns, grid_per_row(p.per_stream, p.cap, ns), ns, p.per_stream};
    const int64_t items = (int64_t)ns * p.per_stream;
    return StageChunk{s0, ns, p.rule == GridRule::per_quad ? grid_per_item((items + 3) / 4, p.cap) : grid_per_item(items, p.cap), 1, items};
}

inline bool aligned16(uintptr_t a) { return (a & 15u) == 0; }

// iq_stats_kernel: one workgroup per (stream, millisecond) over the persistent grid, every stream in one launch.
inline StagePlan stats_plan(int64_t cap, int32_t n_streams, int32_t n_ms) { return stage_plan(n_streams, n_streams, GridRule::per_item, n_ms, cap); }

// iq_condition_kernel, k streams per launch; the launches of a call share the persistent grid's workgroups among their streams.
// 16-byte accesses when both base addresses are 16-byte aligned and every row starts 16-byte aligned if the first one does
// (one stream, or an even stride); a row is then (n_samples + 1) / 2 float4s.
inline StagePlan condition_plan(int64_t cap, int32_t k, uintptr_t in, uintptr_t out, int32_t n_streams, int64_t stride, int64_t n_samples) {
    const bool rows16 = n_streams == 1 || stride % 2 == 0;
    const int32_t vec4 = aligned16(in | out) && rows16;
    StagePlan p = stage_plan(n_streams, k, GridRule::per_row, vec4 ? (n_samples + 1) / 2 : n_samples, cap);
    p.vec4 = vec4;
    return p;
}

// iq_notch_kernel, k streams per launch: one workgroup per (stream, millisecond).  A millisecond of at most lds_samples samples
// keeps its residual in LDS (n float2); a longer one, or any with gyp_debug_set "notch_no_lds", in the output buffer.
inline StagePlan notch_plan(int64_t cap, int32_t k, int32_t n_streams, int32_t n_ms, int32_t n, int32_t lds_samples, bool no_lds) {
    StagePlan p = stage_plan(n_streams, k, GridRule::per_item, n_ms, cap);
    p.lds_bytes = n <= lds_samples && !no_lds ? (int64_t)n * 8 : 0;
    return p;
}

// iq_blank_kernel, k streams per launch: one workgroup per (stream, millisecond).
inline StagePlan blank_plan(int64_t cap, int32_t k, int32_t n_streams, int32_t n_ms) { return stage_plan(n_streams, k, GridRule::per_item, n_ms, cap); }

// iq_excise_kernel (k streams per launch) and iq_spectrum_hist_kernel (k = n_streams): one workgroup per (stream, millisecond).
inline StagePlan excise_plan(int64_t cap, int32_t k, int32_t n_streams, int32_t n_ms) { return stage_plan(n_streams, k, GridRule::per_item, n_ms, cap); }

// iq_power_hist_kernel, k streams per launch, sharing the persistent grid like the condition kernel: a thread takes two samples.
inline StagePlan hist_plan(int64_t cap, int32_t k, int32_t n_streams, int64_t n_samples) { return stage_plan(n_streams, k, GridRule::per_row, n_samples / 2, cap); }

// iq_tones_kernel (on the context's stream, never beside the trackers): one workgroup per (stream, block, frequency), 8 per CU.
inline StagePlan tones_plan(int n_cus, int32_t n_streams, int32_t n_blocks, int32_t n_freq) {
    return stage_plan(n_streams, n_streams, GridRule::per_item, (int64_t)n_blocks * n_freq, (int64_t)n_cus * 8);
}

// track_quality_kernel, k channels per launch: one wavefront per (channel, window of window_ms records), 64 workgroups per CU.
inline int32_t quality_windows(int32_t n_ms, int32_t window_ms) { return (int32_t)(((int64_t)n_ms + window_ms - 1) / window_ms); }
inline StagePlan quality_plan(int n_cus, int32_t k, int32_t n_chan, int32_t n_ms, int32_t window_ms) {
    return stage_plan(n_chan, k, GridRule::per_quad, quality_windows(n_ms, window_ms), (int64_t)n_cus * 64);
}

// ingest_unpack_kernel: a thread takes one 64-bit word of 64 / bits samples; 16-byte stores when the output's base is aligned and
// the stride is even (every row then starts 16-byte aligned).
struct UnpackPlan { int grid; int32_t vec4; int64_t items; };
inline UnpackPlan unpack_plan(int64_t cap, uintptr_t out, int64_t out_stride, int32_t bits, int64_t n_samples, int32_t n_streams) {
    const int64_t per_word = 64 / bits;
    const int64_t items = (n_samples + per_word - 1) / per_word * n_streams;
    return UnpackPlan{(int)std::max<int64_t>(1, std::min<int64_t>((items + 255) / 256, cap)), aligned16(out) && out_stride % 2 == 0, items};
}

}  // namespace gyp
