// Stand-alone driver for the host code of libgypsum_hip under ASan + UBSan or TSan (tests/test_host_sanitizers.py builds and runs it).
//
//     prog <scenario> <in_dir> <out_dir>
//
// One translation unit with the product: it includes gypsum_hip.hip itself, so the extern "C" entry points AND the static helpers
// behind them are compiled with this program's sanitizer flags.  Inputs are little-endian binary files the pytest side wrote, results
// are raw arrays it compares with numpy models or with the uninstrumented library.  No context is ever made and no entry point is given
// a non-NULL one: nothing here initialises the GPU.
#include "../../gypsum_amd/csrc/gypsum_hip.hip"

#include <fstream>
#include <iterator>

#ifndef __has_feature
#define __has_feature(x) 0
#endif

namespace drv {

static std::string g_in, g_out;

[[noreturn]] static void die(const std::string& what) {
    std::fprintf(stderr, "driver: %s\n", what.c_str());
    std::exit(2);
}
#define REQUIRE(cond)                                                                        \
    do {                                                                                     \
        if (!(cond)) drv::die(std::string(__FILE__) + ":" + std::to_string(__LINE__) + ": " #cond); \
    } while (0)

static std::vector<uint8_t> read_bytes(const std::string& name) {
    std::ifstream f(g_in + "/" + name, std::ios::binary);
    if (!f) die("cannot read " + name);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}
template <class T>
static std::vector<T> read_array(const std::string& name) {
    const std::vector<uint8_t> b = read_bytes(name);
    REQUIRE(b.size() % sizeof(T) == 0);
    std::vector<T> v(b.size() / sizeof(T));
    if (!b.empty()) std::memcpy(v.data(), b.data(), b.size());
    return v;
}
static std::string in_path(const std::string& name) { return g_in + "/" + name; }

// An output file under <out_dir>; everything is appended raw.
struct Out {
    FILE* f;
    explicit Out(const std::string& name) : f(std::fopen((g_out + "/" + name).c_str(), "wb")) {
        if (!f) die("cannot write " + name);
    }
    ~Out() { std::fclose(f); }
    Out(const Out&) = delete;
    void bytes(const void* p, size_t n) {
        if (n && std::fwrite(p, 1, n, f) != n) die("short write");
    }
    template <class T>
    void put(const T& v) { bytes(&v, sizeof(T)); }
    void i64(int64_t v) { put(v); }
    void line(const std::string& s) {
        bytes(s.data(), s.size());
        bytes("\n", 1);
    }
};

// The log of blocks a reader handed out: rows (tag, first_ms, n_ms, n_bytes) in <name>.i64 and the bytes back to back in <name>.bin.
struct BlockLog {
    Out meta, data;
    explicit BlockLog(const std::string& name) : meta(name + ".i64"), data(name + ".bin") {}
    void block(int64_t tag, int64_t first, int64_t n_ms, const void* p, size_t n) {
        meta.i64(tag);
        meta.i64(first);
        meta.i64(n_ms);
        meta.i64((int64_t)n);
        data.bytes(p, n);
    }
};

static const int kWordBytes[4] = {4, 1, 2, 1};   // by GYP_FMT_*

// One gyp_ingest_next_host call; logs the block (n_ms 0: a row without bytes).  Returns n_ms, or the error code.
static int next_host(gyp_ingest* g, int fmt, int n, BlockLog& log, int64_t tag) {
    const void* raw = nullptr;
    int64_t first = -1;
    int32_t n_ms = -1;
    const int rc = gyp_ingest_next_host(g, &raw, &first, &n_ms);
    if (rc != GYP_OK) return rc;
    if (n_ms == 0) {
        REQUIRE(raw == nullptr);
        log.block(tag, -1, 0, nullptr, 0);
        return 0;
    }
    log.block(tag, first, n_ms, raw, (size_t)n_ms * n * 2 * kWordBytes[fmt]);
    return n_ms;
}

// --------------------------------------------------------------------------------------------------------- ingest-host
// cases.i64 rows: file index, fmt, n, block_ms, depth, middle millisecond.  times.i64 rows: fs, first_ms.
static void ingest_host() {
    const std::vector<int64_t> cases = read_array<int64_t>("cases.i64");
    BlockLog log("blocks");
    Out info("info.i64");
    for (size_t c = 0; c * 6 < cases.size(); ++c) {
        const int64_t* k = &cases[c * 6];
        const int fmt = (int)k[1], n = (int)k[2];
        const std::string path = in_path("f" + std::to_string(k[0]) + "_" + std::to_string(fmt) + ".bin");
        gyp_ingest* g = nullptr;
        REQUIRE(gyp_ingest_open(nullptr, path.c_str(), fmt, (int64_t)n * 1000, n, (int32_t)k[3], (int32_t)k[4], &g) == GYP_OK && g);
        const int64_t total = gyp_ingest_total_ms(g);
        info.i64(total);
        const int64_t tag = (int64_t)c * 4;
        while (next_host(g, fmt, n, log, tag) > 0) {}
        REQUIRE(next_host(g, fmt, n, log, tag + 1) == 0);   // past the end, twice
        REQUIRE(next_host(g, fmt, n, log, tag + 1) == 0);
        REQUIRE(gyp_ingest_seek(g, total) == GYP_OK);
        REQUIRE(next_host(g, fmt, n, log, tag + 2) == 0);
        REQUIRE(gyp_ingest_seek(g, k[5]) == GYP_OK);
        next_host(g, fmt, n, log, tag + 3);
        info.i64(gyp_ingest_seek(g, -1));
        info.i64(gyp_ingest_seek(g, total + 1));
        next_host(g, fmt, n, log, tag + 3);   // a refused seek leaves the reader where it was
        const float inf = std::numeric_limits<float>::infinity();
        for (float s : {0.0f, -1.0f, inf, std::numeric_limits<float>::quiet_NaN(), 0.01f}) info.i64(gyp_ingest_set_scale(g, s));
        gyp_ingest_close(g);
    }
    info.i64(gyp_ingest_set_scale(nullptr, 1.0f));
    info.i64(gyp_ingest_seek(nullptr, 0));
    info.i64(gyp_ingest_total_ms(nullptr));
    gyp_ingest_close(nullptr);
    {   // the refusals of open
        gyp_ingest* g = nullptr;
        const std::string path = in_path("f0_0.bin");
        info.i64(gyp_ingest_open(nullptr, in_path("missing").c_str(), 0, 2046000, 2046, 1, 3, &g));
        info.i64(gyp_ingest_open(nullptr, path.c_str(), 0, 2046000, 2046, 1, 2, &g));
        info.i64(gyp_ingest_open(nullptr, path.c_str(), 0, 2046000, 2046, 1, 65, &g));
        info.i64(gyp_ingest_open(nullptr, path.c_str(), 0, 2046000, 2046, 0, 3, &g));
        info.i64(gyp_ingest_open(nullptr, path.c_str(), 4, 2046000, 2046, 1, 3, &g));
        info.i64(gyp_ingest_open(nullptr, path.c_str(), 0, 2046000, 2047, 1, 3, &g));
        info.i64(gyp_ingest_open(nullptr, path.c_str(), 0, 2046000, 2046, 1, 3, nullptr));
        REQUIRE(g == nullptr);
    }
    const std::vector<int64_t> times = read_array<int64_t>("times.i64");
    Out t("times.f64");
    for (size_t i = 0; i * 2 < times.size(); ++i) {
        const int64_t fs = times[2 * i], first = times[2 * i + 1];
        gyp_ingest* g = nullptr;
        REQUIRE(gyp_ingest_open(nullptr, in_path("f2_0.bin").c_str(), 0, fs, (int32_t)(fs / 1000), 1, 3, &g) == GYP_OK);
        double* start = (double*)std::malloc(40 * sizeof(double));   // exact sizes: one element too many is a report
        double* end = (double*)std::malloc(40 * sizeof(double));
        REQUIRE(gyp_ingest_times(g, first, 40, start, end) == GYP_OK);
        t.bytes(start, 40 * sizeof(double));
        t.bytes(end, 40 * sizeof(double));
        REQUIRE(gyp_ingest_times(g, -1, 1, start, end) == GYP_E_BAD_ARG && gyp_ingest_times(g, 0, -1, start, end) == GYP_E_BAD_ARG &&
                gyp_ingest_times(g, 0, 1, nullptr, end) == GYP_E_BAD_ARG && gyp_ingest_times(g, 0, 0, nullptr, nullptr) == GYP_OK);
        std::free(start);
        std::free(end);
        gyp_ingest_close(g);
    }
}

// --------------------------------------------------------------------------------------------------------- ingest-races
// The reader has filled its ring and waits for a slot (same translation unit: the counters are read under the handle's mutex).
static void wait_ring_full(gyp_ingest* g) {
    for (;;) {
        {
            std::lock_guard<std::mutex> lk(g->mu);
            if (g->eof || g->produced - g->released >= g->src.depth) return;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
}

// rec.bin: float32 recording at 2.046 Msps (a few hundred ms).  seeks.i64: the milliseconds of the alternating seek / next calls.
static void ingest_races() {
    const int n = 2046, fmt = 0;
    const std::string path = in_path("rec.bin");
    BlockLog log("blocks");
    Out info("info.i64");
    auto open = [&](int block_ms, int depth) {
        gyp_ingest* g = nullptr;
        REQUIRE(gyp_ingest_open(nullptr, path.c_str(), fmt, 2046000, n, block_ms, depth, &g) == GYP_OK && g);
        return g;
    };
    for (int i = 0; i < 50; ++i) gyp_ingest_close(open(1 + i % 7, 3 + i % 5));   // close directly after open
    for (int i = 0; i < 20; ++i) {                                               // close while the reader waits on a full ring
        gyp_ingest* g = open(1 + i % 3, 3);
        wait_ring_full(g);
        gyp_ingest_close(g);
    }
    {   // seek while the reader is reading a large block, and while it waits
        gyp_ingest* g = open(200, 3);
        const int64_t total = gyp_ingest_total_ms(g);
        for (int i = 0; i < 60; ++i) {
            REQUIRE(gyp_ingest_seek(g, (i * 37) % (total + 1)) == GYP_OK);   // the reader was started a moment ago: it is inside pread
            if (i % 3 == 0) REQUIRE(next_host(g, fmt, n, log, 1) >= 0);
            if (i % 10 == 9) wait_ring_full(g);
        }
        gyp_ingest_close(g);
    }
    {
        gyp_ingest* g = open(4, 3);
        for (int64_t ms : read_array<int64_t>("seeks.i64")) {
            REQUIRE(gyp_ingest_seek(g, ms) == GYP_OK);
            REQUIRE(next_host(g, fmt, n, log, 2) >= 0);
        }
        gyp_ingest_close(g);
    }
    {   // close at end of data
        gyp_ingest* g = open(16, 64);
        while (next_host(g, fmt, n, log, 3) > 0) {}
        gyp_ingest_close(g);
    }
    {   // the file shrinks after open: the blocks read before stay good, the next one is GYP_E_IO
        const std::string victim = in_path("shrinks.bin");
        gyp_ingest* g = nullptr;
        REQUIRE(gyp_ingest_open(nullptr, victim.c_str(), fmt, 2046000, n, 2, 3, &g) == GYP_OK && g);
        wait_ring_full(g);   // blocks 0..2 = milliseconds 0..5 are in the ring
        const int fd = ::open(victim.c_str(), O_WRONLY);
        REQUIRE(fd >= 0 && ftruncate(fd, (off_t)6 * n * 8 + 24) == 0);
        ::close(fd);
        int rc = 0;
        for (int i = 0; i < 3; ++i) REQUIRE((rc = next_host(g, fmt, n, log, 4)) == 2);
        rc = next_host(g, fmt, n, log, 4);   // block 3 starts beyond the new end: pread returns 0
        info.i64(rc);
        Out("shrinks_error.txt").line(gyp_last_error(nullptr));
        info.i64(next_host(g, fmt, n, log, 4));   // the error stays
        REQUIRE(gyp_ingest_seek(g, 0) == GYP_OK);   // and a seek clears it
        REQUIRE(next_host(g, fmt, n, log, 5) == 2);
        gyp_ingest_close(g);
    }
    {   // two handles, two consumer threads, each with its own gyp_last_error(NULL)
        std::string msg[2];
        auto body = [&](int who) {
            BlockLog mine("thread" + std::to_string(who));
            gyp_ingest* g = open(who ? 3 : 5, who ? 3 : 8);
            const int64_t total = gyp_ingest_total_ms(g);
            for (int round = 0; round < 3; ++round) {
                while (next_host(g, fmt, n, mine, 6 + who) > 0) {}
                REQUIRE(gyp_ingest_seek(g, (total / 3) * round) == GYP_OK);
            }
            const int rc = who ? gyp_ingest_set_scale(g, -1.0f) : gyp_ingest_seek(g, total + 1);
            REQUIRE(rc == GYP_E_BAD_ARG);
            std::this_thread::sleep_for(std::chrono::milliseconds(5));   // (the other thread fails in the meantime)
            msg[who] = gyp_last_error(nullptr);
            gyp_ingest_close(g);
        };
        std::thread a(body, 0), b(body, 1);
        a.join();
        b.join();
        Out m("thread_errors.txt");
        m.line(msg[0]);
        m.line(msg[1]);
    }
}

// --------------------------------------------------------------------------------------------------------- bits
// plan.i64 rows: stream index, symbols per push, event capacity, reset mode (0 none, 1 gyp_bits_reset(channel) in mid-stream, 2 channel -1).
// Stream k: s<k>.sym (int8), s<k>.start / s<k>.end (float64).  Then the block path on recs.bin (channel-major gyp_track_rec).
static void put_state(gyp_bits* b, int32_t ch, Out& states) {
    gyp_bits_state* st = (gyp_bits_state*)std::malloc(sizeof(gyp_bits_state));
    REQUIRE(gyp_bits_get_state(b, ch, st) == GYP_OK);
    states.bytes(st, sizeof(*st));
    std::free(st);
}
static void bits() {
    const std::vector<int64_t> plan = read_array<int64_t>("plan.i64");
    Out events("events.bin"), cursors("cursors.i32"), states("states.bin"), counts("counts.i32");
    for (size_t r = 0; r * 4 < plan.size(); ++r) {
        const int64_t* k = &plan[r * 4];
        const std::string s = "s" + std::to_string(k[0]);
        const std::vector<int8_t> sym = read_array<int8_t>(s + ".sym");
        const std::vector<double> start = read_array<double>(s + ".start"), end = read_array<double>(s + ".end");
        const int32_t push = (int32_t)k[1], cap = (int32_t)k[2], channel = 1;
        gyp_bits* b = nullptr;
        REQUIRE(gyp_bits_create(3, &b) == GYP_OK && b);
        const size_t total = sym.size(), mid = total / 2;
        bool reset_done = k[3] == 0;
        for (size_t at = 0; at < total; at += (size_t)push) {
            const int32_t n = (int32_t)std::min<size_t>((size_t)push, total - at);
            if (!reset_done && at >= mid) {
                REQUIRE(gyp_bits_reset(b, k[3] == 2 ? -1 : channel) == GYP_OK);
                reset_done = true;
            }
            // exact-size copies on the heap: a read or write one element out is a report
            double* ts = (double*)std::malloc(n * sizeof(double));
            double* te = (double*)std::malloc(n * sizeof(double));
            int8_t* v = (int8_t*)std::malloc((size_t)n);
            int32_t* cur = (int32_t*)std::malloc(n * sizeof(int32_t));
            gyp_bit_event* ev = cap ? (gyp_bit_event*)std::malloc((size_t)cap * sizeof(gyp_bit_event)) : nullptr;
            std::memcpy(ts, &start[at], n * sizeof(double));
            std::memcpy(te, &end[at], n * sizeof(double));
            std::memcpy(v, &sym[at], (size_t)n);
            int32_t n_ev = -1;
            REQUIRE(gyp_bits_push(b, channel, n, ts, ts, te, v, cur, ev, cap, &n_ev) == GYP_OK);
            REQUIRE(n_ev >= 0 && n_ev <= cap);
            counts.put(n_ev);
            events.bytes(ev, (size_t)n_ev * sizeof(gyp_bit_event));
            cursors.bytes(cur, n * sizeof(int32_t));
            put_state(b, channel, states);
            std::free(ts);
            std::free(te);
            std::free(v);
            std::free(cur);
            std::free(ev);
        }
        for (;;) {   // what the pushes left in the FIFO
            gyp_bit_event* ev = (gyp_bit_event*)std::malloc(5 * sizeof(gyp_bit_event));
            int32_t n_ev = -1;
            REQUIRE(gyp_bits_drain(b, ev, 5, &n_ev) == GYP_OK);
            counts.put(n_ev);
            events.bytes(ev, (size_t)n_ev * sizeof(gyp_bit_event));
            std::free(ev);
            if (n_ev == 0) break;
        }
        put_state(b, 0, states);   // an untouched channel
        gyp_bits_destroy(b);
    }
    // the block path: cuts.i64 = the millisecond cuts, recs.bin holds a status-1 record
    const std::vector<int64_t> cuts = read_array<int64_t>("cuts.i64");
    const std::vector<uint8_t> recs = read_bytes("recs.bin");
    const std::vector<double> start = read_array<double>("block.start"), end = read_array<double>("block.end");
    const int32_t n_ms = (int32_t)start.size();
    REQUIRE(n_ms > 0 && recs.size() % ((size_t)n_ms * sizeof(gyp_track_rec)) == 0);
    const int32_t n_chan = (int32_t)(recs.size() / ((size_t)n_ms * sizeof(gyp_track_rec)));
    gyp_bits* b = nullptr;
    REQUIRE(gyp_bits_create(n_chan, &b) == GYP_OK);
    Out bev("block_events.bin"), bstates("block_states.bin"), bcounts("block_counts.i32");
    for (size_t i = 0; i + 1 < cuts.size(); ++i) {
        const int32_t a = (int32_t)cuts[i], len = (int32_t)(cuts[i + 1] - cuts[i]);
        gyp_track_rec* part = (gyp_track_rec*)std::malloc((size_t)n_chan * len * sizeof(gyp_track_rec));
        for (int32_t c = 0; c < n_chan; ++c)
            std::memcpy(part + (size_t)c * len, recs.data() + ((size_t)c * n_ms + a) * sizeof(gyp_track_rec), (size_t)len * sizeof(gyp_track_rec));
        double* ts = (double*)std::malloc(len * sizeof(double));
        double* te = (double*)std::malloc(len * sizeof(double));
        std::memcpy(ts, &start[a], len * sizeof(double));
        std::memcpy(te, &end[a], len * sizeof(double));
        const int32_t cap = i % 2 ? 3 : 1000;
        gyp_bit_event* ev = (gyp_bit_event*)std::malloc((size_t)cap * sizeof(gyp_bit_event));
        int32_t n_ev = -1;
        REQUIRE(gyp_bits_push_block(b, part, n_chan, len, ts, te, ev, cap, &n_ev) == GYP_OK);
        bcounts.put(n_ev);
        bev.bytes(ev, (size_t)n_ev * sizeof(gyp_bit_event));
        for (int32_t c = 0; c < n_chan; ++c) put_state(b, c, bstates);
        std::free(part);
        std::free(ts);
        std::free(te);
        std::free(ev);
    }
    Out rc("refusals.i64");
    int32_t n_ev = 0;
    gyp_bits_state st;
    gyp_bits* refused = nullptr;
    rc.i64(gyp_bits_create(0, &refused));
    rc.i64(gyp_bits_create(-1, &refused));
    rc.i64(gyp_bits_create(1, nullptr));
    REQUIRE(refused == nullptr);
    rc.i64(gyp_bits_reset(b, n_chan));
    rc.i64(gyp_bits_reset(nullptr, 0));
    rc.i64(gyp_bits_push(b, n_chan, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &n_ev));
    rc.i64(gyp_bits_push(b, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &n_ev));
    rc.i64(gyp_bits_push(nullptr, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, &n_ev));
    rc.i64(gyp_bits_push_block(b, nullptr, n_chan + 1, 1, nullptr, nullptr, nullptr, 0, &n_ev));
    rc.i64(gyp_bits_push_block(b, nullptr, 1, 1, nullptr, nullptr, nullptr, 0, &n_ev));
    rc.i64(gyp_bits_drain(b, nullptr, -1, &n_ev));
    rc.i64(gyp_bits_get_state(b, -1, &st));
    rc.i64(gyp_bits_get_state(b, 0, nullptr));
    gyp_bits_destroy(b);
    gyp_bits_destroy(nullptr);
}

// --------------------------------------------------------------------------------------------------------- spans
// cases.i64 rows: bits, real, order, samples_per_ms, file_bytes, first_sample, n_samples, file_samples if the static helper is to be
// called too (the contract's arithmetic stays inside int64), else -1.
static void spans() {
    const std::vector<int64_t> cases = read_array<int64_t>("cases.i64");
    Out pub("public.i64"), stat("static.i64");
    for (size_t c = 0; c * 8 < cases.size(); ++c) {
        const int64_t* k = &cases[c * 8];
        gyp_packing p{};
        p.bits = (int32_t)k[0];
        p.real = (int32_t)k[1];
        p.order = (int32_t)k[2];
        for (int i = 0; i < 16; ++i) p.levels[i] = (float)i - 7.5f;
        int64_t* o = (int64_t*)std::malloc(6 * sizeof(int64_t));
        int32_t* bit0 = (int32_t*)std::malloc(sizeof(int32_t));
        for (int i = 0; i < 6; ++i) o[i] = -777;
        *bit0 = -777;
        const int rc = gyp_packed_span(&p, (int32_t)k[3], k[4], k[5], k[6], &o[0], &o[1], &o[2], bit0, &o[3], &o[4], &o[5]);
        REQUIRE(gyp_packed_span(&p, (int32_t)k[3], k[4], k[5], k[6], nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == rc);
        pub.i64(rc);
        for (int i = 0; i < 6; ++i) pub.i64(o[i]);
        pub.i64(*bit0);
        std::free(o);
        std::free(bit0);
        PackedSpan sp;
        if (k[7] >= 0) sp = packed_span(k[0] * (k[1] ? 1 : 2), k[7], k[5], k[6]);
        stat.i64(sp.in_first);
        stat.i64(sp.in_n);
        stat.i64(sp.first_byte);
        stat.i64(sp.n_bytes);
        stat.i64(sp.bit0);
    }
}

// --------------------------------------------------------------------------------------------------------- designs
// cases.i64 rows: kind (0 resampler, 1 down-converter), fs_in, fs_out, if_hz, taps.
static void designs() {
    const std::vector<int64_t> cases = read_array<int64_t>("cases.i64");
    Out meta("meta.i64"), tables("tables.f32");
    for (size_t c = 0; c * 5 < cases.size(); ++c) {
        const int64_t* k = &cases[c * 5];
        int32_t L = -1, T = -1;
        const int rc = k[0] ? gyp_ddc_design(k[1], k[2], k[3], (int32_t)k[4], nullptr, &L, &T) : gyp_resample_design(k[1], k[2], (int32_t)k[4], nullptr, &L);
        if (!k[0] && rc == GYP_OK) T = resample_taps((int32_t)k[4]);
        meta.i64(rc);
        meta.i64(L);
        meta.i64(T);
        if (rc != GYP_OK) {
            REQUIRE(L == -1 && T == -1);
            continue;
        }
        float* table = (float*)std::malloc((size_t)L * T * sizeof(float));   // exactly L x T: ASan sees a one-element overrun
        int32_t L2 = -1, T2 = -1;
        const int rc2 = k[0] ? gyp_ddc_design(k[1], k[2], k[3], (int32_t)k[4], table, &L2, &T2) : gyp_resample_design(k[1], k[2], (int32_t)k[4], table, &L2);
        REQUIRE(rc2 == GYP_OK && L2 == L && (!k[0] || T2 == T));
        REQUIRE((k[0] ? gyp_ddc_design(k[1], k[2], k[3], (int32_t)k[4], nullptr, nullptr, nullptr) : gyp_resample_design(k[1], k[2], (int32_t)k[4], nullptr, nullptr)) == GYP_OK);
        tables.bytes(table, (size_t)L * T * sizeof(float));
        std::free(table);
    }
}

// --------------------------------------------------------------------------------------------------------- misc
static void misc() {
    {
        uint8_t* chips = (uint8_t*)std::malloc(32 * 1023);
        REQUIRE(gyp_prn_chips(chips) == GYP_OK && gyp_prn_chips(nullptr) == GYP_E_BAD_ARG);
        Out("prn_chips.u8").bytes(chips, 32 * 1023);
        std::free(chips);
        Out lanes("lanes.f32"), rc("lanes_rc.i64");
        for (int sat : {1, 32, 0, 33}) {
            float* t = (float*)std::malloc(32 * 64 * 2 * sizeof(float));
            const int r = gyp_prn_spectrum_lane_layout(sat, t);
            rc.i64(r);
            if (r == GYP_OK) lanes.bytes(t, 32 * 64 * 2 * sizeof(float));
            std::free(t);
        }
        rc.i64(gyp_prn_spectrum_lane_layout(1, nullptr));
    }
    {   // cells.bin: gyp_cell records; cells_n.i32: samples_per_ms of each
        const std::vector<uint8_t> cells = read_bytes("cells.bin");
        const std::vector<int32_t> n = read_array<int32_t>("cells_n.i32");
        REQUIRE(cells.size() == n.size() * sizeof(gyp_cell));
        Out s("strength.f64");
        for (size_t i = 0; i < n.size(); ++i) {
            gyp_cell* c = (gyp_cell*)std::malloc(sizeof(gyp_cell));
            std::memcpy(c, cells.data() + i * sizeof(gyp_cell), sizeof(gyp_cell));
            s.put(gyp_cell_strength(c, n[i]));
            std::free(c);
        }
    }
    {   // nav.i64 rows: seed, stream, sat, offset, ms
        const std::vector<int64_t> nav = read_array<int64_t>("nav.i64");
        Out o("nav_bits.i64");
        for (size_t i = 0; i * 5 < nav.size(); ++i)
            o.i64(gyp_synth_nav_bit((uint64_t)nav[5 * i], (int32_t)nav[5 * i + 1], (int32_t)nav[5 * i + 2], (int32_t)nav[5 * i + 3], nav[5 * i + 4]));
    }
    {
        gyp_params* p = (gyp_params*)std::malloc(sizeof(gyp_params));
        gyp_params_default(p);
        gyp_params_default(nullptr);
        Out("params.f64").bytes(p, sizeof(*p));
        std::free(p);
    }
    {   // layout.i64: n_ms values then, after a -1, sub_ms values; every pair into a 33-int heap buffer
        const std::vector<int64_t> in = read_array<int64_t>("layout.i64");
        const size_t cut = std::find(in.begin(), in.end(), (int64_t)-1) - in.begin();
        Out o("layout.i32");
        for (size_t s = cut + 1; s < in.size(); ++s)
            for (size_t i = 0; i < cut; ++i) {
                int32_t* starts = (int32_t*)std::malloc(33 * sizeof(int32_t));
                for (int j = 0; j < 33; ++j) starts[j] = -777;
                o.put((int32_t)gyp_debug_spec_layout_for((int32_t)in[i], (int32_t)in[s], starts));
                o.bytes(starts, 33 * sizeof(int32_t));
                if (in[s] == 500) {
                    int32_t* again = (int32_t*)std::malloc(33 * sizeof(int32_t));
                    for (int j = 0; j < 33; ++j) again[j] = -777;
                    (void)gyp_debug_spec_layout((int32_t)in[i], again);
                    REQUIRE(std::memcmp(starts, again, 33 * sizeof(int32_t)) == 0);
                    std::free(again);
                }
                std::free(starts);
            }
        int32_t one[33];
        REQUIRE(gyp_debug_spec_layout_for(0, 500, one) == GYP_E_BAD_ARG && gyp_debug_spec_layout_for(-5, 500, one) == GYP_E_BAD_ARG &&
                gyp_debug_spec_layout_for(100, 500, nullptr) == GYP_E_BAD_ARG);
    }
    {   // every entry point that needs a context, a bank or a handle refuses NULL and writes nothing
        Out o("null_rc.i64");
        uint8_t* buf = (uint8_t*)std::malloc(256);
        std::memset(buf, 0x5a, 256);
        void* vp = nullptr;
        gyp_bank* bank = nullptr;
        gyp_ingest* ing = nullptr;
        gyp_packing pk{};
        pk.bits = 2;
        int32_t sat = 1;
        double dop = 0.0;
        float* f = (float*)buf;
        gyp_ctx* none = nullptr;
        gyp_bank* nobank = nullptr;
        const int rcs[] = {
            gyp_set_params(none, (gyp_params*)buf), gyp_get_params(none, (gyp_params*)buf), gyp_device_name(none, (char*)buf, 256), gyp_set_stream(none, nullptr),
            gyp_sync(none), gyp_wait_for(none, none), gyp_timer_start(none), gyp_timer_stop(none, f), gyp_set_stream_format(none, 2046000, 2046),
            gyp_malloc(none, 16, &vp), gyp_free(none, buf), gyp_memcpy_h2d(none, buf, buf, 16), gyp_memcpy_d2h(none, buf, buf, 16),
            gyp_memcpy_d2h_async(none, buf, buf, 16),
            gyp_correlate_cells_dev(none, f, 2046, 1, (gyp_cell_desc*)buf, 1, 0, (gyp_cell*)buf, nullptr),
            gyp_correlate_cells(none, f, 1, 1, (gyp_cell_desc*)buf, 1, 0, (gyp_cell*)buf, nullptr),
            gyp_correlate_grid_dev(none, f, 1, 2046, 1, &sat, 1, &dop, 1, 0, (gyp_cell*)buf),
            gyp_correlate_grid(none, f, 1, 1, &sat, 1, &dop, 1, 0, (gyp_cell*)buf),
            gyp_grid_best_bins_dev(none, (gyp_cell*)buf, 1, 1, (gyp_best_bin*)buf),
            gyp_grid_best_bins_refined_dev(none, f, 1, 2046, 1, &sat, 1, &dop, 1, 0, (gyp_cell*)buf, (gyp_best_bin*)buf),
            gyp_acquire_dev(none, f, 1, 2046, 1, &sat, 1, (gyp_acq_result*)buf), gyp_acquire(none, f, 1, 1, &sat, 1, (gyp_acq_result*)buf),
            gyp_search_level_dev(none, f, 1, 2046, 1, &sat, 1, 0.0, 7000.0, (gyp_acq_result*)buf),
            gyp_search_level(none, f, 1, 1, &sat, 1, 0.0, 7000.0, (gyp_acq_result*)buf),
            gyp_track_step_dev(none, f, 2046, &dop, (gyp_chan_in*)buf, 1, (gyp_chan_out*)buf, nullptr),
            gyp_track_step(none, f, 1, &dop, (gyp_chan_in*)buf, 1, (gyp_chan_out*)buf, nullptr),
            gyp_bank_create(none, (gyp_chan_init*)buf, 1, &bank), gyp_bank_size(nobank), gyp_bank_set_channel(nobank, 0, (gyp_chan_init*)buf),
            gyp_bank_drop_channel(nobank, 0), gyp_track_block_dev(nobank, f, 2046, 1, &dop, (gyp_track_rec*)buf),
            gyp_track_block(nobank, f, 1, 1, &dop, (gyp_track_rec*)buf), gyp_bank_keep_profiles(nobank, 1),
            gyp_bank_read_profiles(nobank, 0, f, &sat), gyp_bank_reset_dev(nobank, (gyp_chan_init*)buf),
            gyp_bank_get_state(nobank, &dop, &dop, &sat, &sat), gyp_comm_init(none, 0, 1, nullptr), gyp_comm_destroy(none),
            gyp_comm_info(none, &sat, &sat, &sat), gyp_allgather_dev(none, buf, buf, 16), gyp_host_alloc(none, 16, &vp), gyp_host_free(none, buf),
            gyp_widen_iq_dev(none, GYP_FMT_I8, buf, 16, 1.0f, f), gyp_synth_iq_dev(none, f, 1, 2046, 1, (gyp_synth_sat*)buf, 1, 0.0f, 1),
            gyp_debug_set(none, "no_pipe", 1.0), gyp_debug_get(none, "no_pipe", &dop), gyp_debug_track_profile(none, 1, (long long*)buf),
            gyp_debug_track_timing(none, 1, f), gyp_debug_fft_bench(none, 4, 1, 1, f), gyp_debug_spec_read(nobank, f, 20, &sat),
            gyp_debug_spec_redo_read(nobank, &sat), gyp_debug_dll_read(nobank, &sat), gyp_debug_disc_read(nobank, 1, &dop),
            gyp_resample_iq_dev(none, GYP_FMT_I8, buf, 1, 16, 0, 16, 1.0f, 2048000, 32, 0, 1, 2046, f),
            gyp_ddc_iq_dev(none, GYP_FMT_I8, buf, 1, 16, 0, 16, 1.0f, 16368000, 4092000, 64, 0, 1, 4092, f),
            gyp_unpack_iq_dev(none, &pk, buf, 1, 16, 0, 16, 1.0f, 16, f),
            gyp_resample_packed_dev(none, &pk, buf, 1, 16, 0, 0, 16, 1.0f, 2048000, 0, 32, 0, 1, 2046, f),
            gyp_ingest_open_resampled(none, in_path("cells.bin").c_str(), GYP_FMT_I8, 2048000, 32, 1, 3, &ing),
            gyp_ingest_open_ddc(none, in_path("cells.bin").c_str(), GYP_FMT_I8, 16368000, 4092000, 64, 1, 3, &ing),
            gyp_ingest_open_packed(none, in_path("cells.bin").c_str(), &pk, 2048000, 0, 32, 1, 3, &ing),
            gyp_device_locality(none, &sat, (char*)buf, 256), gyp_ingest_next_dev(nullptr, (const float**)&vp, (int64_t*)buf, &sat),
            gyp_ingest_next_host(nullptr, (const void**)&vp, (int64_t*)buf, &sat),
        };
        for (int rc : rcs) o.i64(rc);
        gyp_destroy(nullptr);
        gyp_bank_destroy(nullptr);
        bool untouched = vp == nullptr && bank == nullptr && ing == nullptr && sat == 1 && dop == 0.0;
        for (int i = 0; i < 256; ++i) untouched = untouched && buf[i] == 0x5a;
        o.i64(untouched ? 1 : 0);
        std::free(buf);
    }
}

// --------------------------------------------------------------------------------------------------------- halo-readers
// Handles of all four kinds without a context, described, measured and sized by the product (ingest_describe, ingest_open_file,
// ingest_span); ring slots of exactly host_block_bytes; the product's reader thread and take / release protocol.
// cases.i64 rows: packed (0/1), fmt or bits, real, order, n_in, taps (0: not filtered), block_ms, depth, file index, restart millisecond.
// spans.i64 rows, one per block handed out: s0, count, in_first, in_n, first_byte, bit0, n_bytes, pad_lo, pad_hi.
static void halo_readers() {
    const std::vector<int64_t> cases = read_array<int64_t>("cases.i64");
    BlockLog log("blocks");
    Out info("info.i64"), spans("spans.i64");
    for (size_t c = 0; c * 10 < cases.size(); ++c) {
        const int64_t* k = &cases[c * 10];
        ResampleDesign d;
        d.taps = (int32_t)k[5];
        d.real = k[2] != 0;
        d.n_in = d.n_out = (int32_t)k[4];
        PackedFormat pk;
        pk.bits = (int32_t)k[1];
        pk.real = d.real;
        pk.order = (int32_t)k[3];
        gyp_ingest* g = new gyp_ingest(nullptr, 0, ingest_describe(k[0] ? 0 : (int32_t)k[1], k[0] ? &pk : nullptr, d, 0, (int32_t)k[6], (int32_t)k[7]));
        const IngestSource& src = g->src;
        REQUIRE(ingest_open_file(g, in_path("h" + std::to_string(k[8]) + ".bin").c_str()) == 0);
        info.i64(g->total_ms);
        info.i64(g->file_samples);
        info.i64((int64_t)src.host_block_bytes);
        for (auto& p : g->host) REQUIRE((p = (uint8_t*)std::malloc(src.host_block_bytes)) != nullptr);   // no rounding up
        auto consume = [&](int64_t tag) {
            for (;;) {
                ingest_release(g, g->taken);
                int slot = -1;
                int64_t first = -1;
                int32_t n_ms = -1;
                if (!ingest_take(g, &slot, &first, &n_ms, true)) break;
                const IngestSpan sp = ingest_span(src, g->file_samples, first, n_ms);
                for (int64_t v : {sp.s0, sp.count, sp.in_first, sp.in_n, sp.first_byte, (int64_t)sp.bit0, sp.n_bytes, sp.pad_lo, sp.pad_hi}) spans.i64(v);
                REQUIRE((size_t)sp.slot_bytes() <= src.host_block_bytes);
                log.block(tag, first, n_ms, g->host[slot], (size_t)sp.slot_bytes());
            }
            REQUIRE(g->io_errno == 0);
        };
        ingest_start_reader(g, 0);
        consume((int64_t)c * 2);
        ingest_stop_reader(g);
        if (k[9] <= g->total_ms) {
            ingest_start_reader(g, k[9]);
            consume((int64_t)c * 2 + 1);
            ingest_stop_reader(g);
        }
        for (auto p : g->host) std::free(p);
        ingest_free(g);
    }
}

// --------------------------------------------------------------------------------------------------------- small-parsers
static void small_parsers() {
    {   // cpulists.bin: strings, each closed by a NUL
        const std::vector<uint8_t> all = read_bytes("cpulists.bin");
        Out o("cpusets.bin");
        for (size_t at = 0; at < all.size();) {
            const std::string text((const char*)&all[at]);
            at += text.size() + 1;
            cpu_set_t* set = (cpu_set_t*)std::malloc(sizeof(cpu_set_t));
            const bool any = parse_cpulist(text, set);
            o.put((uint8_t)any);
            for (int cpu = 0; cpu < CPU_SETSIZE; ++cpu) o.put((uint8_t)(CPU_ISSET(cpu, set) ? 1 : 0));
            std::free(set);
        }
        o.put((int32_t)CPU_SETSIZE);
    }
    {
        Out o("small_files.bin");
        for (const char* name : {"missing", "empty", "big2000", "trailing"}) {
            const std::string s = read_small_file(in_path(name));
            o.put((int64_t)s.size());
            o.bytes(s.data(), s.size());
        }
    }
    {
        Out o("round6.f64");
        for (double x : read_array<double>("round6.f64")) o.put(round6(x));
    }
    {   // packings.bin: gyp_packing records; the refusal's text, or "ok"
        const std::vector<uint8_t> all = read_bytes("packings.bin");
        Out o("packings.txt");
        for (size_t at = 0; at + sizeof(gyp_packing) <= all.size(); at += sizeof(gyp_packing)) {
            gyp_packing* p = (gyp_packing*)std::malloc(sizeof(gyp_packing));
            std::memcpy(p, &all[at], sizeof(gyp_packing));
            PackedFormat f;
            const char* why = packing_check(p, &f);
            REQUIRE(packing_check(p, nullptr) == why);
            o.line(why ? why : "ok " + std::to_string(f.bits) + " " + std::to_string((int)f.real) + " " + std::to_string(f.order) + " " + std::to_string(f.sample_bits()));
            std::free(p);
        }
        o.line(packing_check(nullptr, nullptr));
    }
}

// --------------------------------------------------------------------------------------------------------- grid-plan
// shapes.i64 rows: k, n_cus, n_units, n_sats, n_blk, switches (bit 0 no_pipe, 1 no_shared_fwd, 2 no_grid_fused, 3 no_grid_parts), fused_waves.
// plans.i64 rows: GridPlan's members in their order.
static void grid_plans() {
    const std::vector<int64_t> shapes = read_array<int64_t>("shapes.i64");
    REQUIRE(shapes.size() % 7 == 0);
    std::vector<int64_t> plans;
    plans.reserve(shapes.size() / 7 * 10);
    for (size_t r = 0; r * 7 < shapes.size(); ++r) {
        const int64_t* s = &shapes[r * 7];
        const GridPlan pl = grid_plan(GridShape{(int)s[0], (int)s[1], s[2], (int)s[3], (int)s[4]},
                                      GridSwitches{(s[5] & 1) != 0, (s[5] & 2) != 0, (s[5] & 4) != 0, (s[5] & 8) != 0, (int)s[6]});
        for (int64_t v : {(int64_t)pl.path, (int64_t)pl.pipe, (int64_t)pl.waves, (int64_t)pl.gs, (int64_t)pl.parts, (int64_t)pl.wide_fold, (int64_t)pl.wgrid,
                          (int64_t)pl.folded_bytes, (int64_t)pl.z_bytes, (int64_t)pl.partial_bytes})
            plans.push_back(v);
    }
    Out("plans.i64").bytes(plans.data(), plans.size() * sizeof(int64_t));
}

// --------------------------------------------------------------------------------------------------------- track-plan
// shapes.i64 rows: k, n, n_cus, n_chan, n_ms, keep_profiles, switches (bit 0 no_pipe, 1 no_spec, 2 spec_redo, 3 no_exact_shared), spec_sub_ms,
// track_chunk_ms, spec_confidence_kappa.  plans.i64 rows: flow, rounds, chunk_ms, launches, exact_path, the bits of spec_kappa, the layout's n,
// longest and all of start[].
static void track_plans() {
    const std::vector<int64_t> shapes = read_array<int64_t>("shapes.i64");
    REQUIRE(shapes.size() % 10 == 0);
    std::vector<int64_t> plans;
    plans.reserve(shapes.size() / 10 * (9 + kMaxSubBlocks));
    for (size_t r = 0; r * 10 < shapes.size(); ++r) {
        const int64_t* s = &shapes[r * 10];
        const TrackPlan pl = track_plan(TrackShape{(int)s[0], (int)s[1], (int)s[2], (int)s[3], (int)s[4], s[5] != 0},
                                        TrackSwitches{(s[6] & 1) != 0, (s[6] & 2) != 0, (s[6] & 4) != 0, (int)s[7], (int)s[8], (s[6] & 8) != 0, (double)s[9]});
        uint32_t kappa_bits;
        std::memcpy(&kappa_bits, &pl.spec_kappa, sizeof(kappa_bits));
        for (int64_t v : {(int64_t)pl.flow, (int64_t)pl.rounds, (int64_t)pl.chunk_ms, (int64_t)pl.launches, (int64_t)pl.exact_path, (int64_t)kappa_bits,
                          (int64_t)pl.layout.n, (int64_t)pl.layout.longest})
            plans.push_back(v);
        for (int32_t v : pl.layout.start) plans.push_back(v);
    }
    Out("plans.i64").bytes(plans.data(), plans.size() * sizeof(int64_t));
}

// --------------------------------------------------------------------------------------------------------- acq-plan
// shapes.i64 rows: k, n, n_streams, n_sats, n_ms, switches (bit 0 no_pipe, 1 no_acq_shared_fwd, 2 no_acq_split, 3 is_helper), acq_lanes, single_level,
// then the bits of four float64: spread0, acq_initial_spread_hz, acq_min_spread_hz, acq_bins_per_spread.  plans.i64 rows: AcqPlan's members in
// their order (bins_per_spread as its bits).
static void acq_plans() {
    const std::vector<int64_t> shapes = read_array<int64_t>("shapes.i64");
    REQUIRE(shapes.size() % 12 == 0);
    std::vector<int64_t> plans;
    plans.reserve(shapes.size() / 12 * (20 + 2 * kMaxAcqLanes));
    for (size_t r = 0; r * 12 < shapes.size(); ++r) {
        const int64_t* s = &shapes[r * 12];
        double real[4];
        std::memcpy(real, s + 8, sizeof(real));
        const AcqPlan pl = acq_plan(AcqShape{(int)s[0], (int)s[1], (int)s[2], (int)s[3], (int)s[4]}, AcqSearch{0.0, real[0], s[7] != 0}, AcqLevels{real[1], real[2], real[3]},
                                    AcqSwitches{(s[5] & 1) != 0, (s[5] & 2) != 0, (s[5] & 4) != 0, (s[5] & 8) != 0, (int)s[6]});
        int64_t bins_bits;
        std::memcpy(&bins_bits, &pl.bins_per_spread, sizeof(bins_bits));
        for (int64_t v : {(int64_t)pl.fits, (int64_t)pl.n_states, (int64_t)pl.n_cells, (int64_t)pl.n_levels, (int64_t)pl.shared_levels, bins_bits, (int64_t)pl.max_units,
                          (int64_t)pl.states, (int64_t)pl.cells, (int64_t)pl.out, (int64_t)pl.refined, (int64_t)pl.partial64, (int64_t)pl.profiles, (int64_t)pl.spectra,
                          (int64_t)pl.tpb, (int64_t)pl.nblk, (int64_t)pl.refine_x, (int64_t)pl.refine_y, (int64_t)pl.exact_z, (int64_t)pl.lanes})
            plans.push_back(v);
        for (int v : pl.lane_first) plans.push_back(v);
        for (int v : pl.lane_streams) plans.push_back(v);
    }
    Out("plans.i64").bytes(plans.data(), plans.size() * sizeof(int64_t));
}

// --------------------------------------------------------------------------------------------------------- resample-plan
// shapes.i64 rows: fs_in, fs_out (Hz), taps, n_streams, first_ms, n_ms, tile_samples.  plans.i64 rows: ResampleRatio's members, then
// ResampleTiling's, in their order.  mixers.i64 rows: fs, f_hz -> mixed.i64 rows: MixerParams' members (the two scales as their bits).
static void resample_plans() {
    const std::vector<int64_t> shapes = read_array<int64_t>("shapes.i64");
    REQUIRE(shapes.size() % 7 == 0);
    std::vector<int64_t> plans;
    plans.reserve(shapes.size() / 7 * 13);
    for (size_t r = 0; r * 7 < shapes.size(); ++r) {
        const int64_t* s = &shapes[r * 7];
        const ResampleRatio q = resample_ratio(s[0], s[1]);
        const ResampleTiling t = resample_tiling(q, (int32_t)s[2], (int32_t)s[3], s[4], (int32_t)s[5], (int32_t)s[6]);
        for (int64_t v : {(int64_t)q.n_in, (int64_t)q.n_out, (int64_t)q.g, (int64_t)q.L, (int64_t)q.M, (int64_t)t.fits, t.n_tiles, t.lds_samples, t.p_first,
                          t.n_periods, (int64_t)t.np_tile, (int64_t)t.pc_tile, (int64_t)t.n_pchunks})
            plans.push_back(v);
    }
    Out("plans.i64").bytes(plans.data(), plans.size() * sizeof(int64_t));
    const std::vector<int64_t> mixers = read_array<int64_t>("mixers.i64");
    Out mixed("mixed.i64");
    for (size_t r = 0; r * 2 < mixers.size(); ++r) {
        const MixerParams m = mixer_params(mixers[2 * r], mixers[2 * r + 1]);
        const ToneMix tone = tone_mix(m.fs);   // the tone kernels' constants come from the same function
        REQUIRE(tone.fs == m.fs && tone.q_scale == m.q_scale && tone.y_scale == m.y_scale);
        int64_t bits[2];
        std::memcpy(&bits[0], &m.q_scale, 8);
        std::memcpy(&bits[1], &m.y_scale, 8);
        for (int64_t v : {m.fs, m.f, bits[0], bits[1]}) mixed.i64(v);
    }
}

// --------------------------------------------------------------------------------------------------------- cond-plan
// shapes.i64 rows: stage, n_cus, wg_per_cu, n, a, b, stride, in_addr, out_addr, flag (tests/cond_plan_model.py says what a and b are
// per stage).  plans.i64 rows: the plan, its first and last launch, and over all launches the sum and the largest of their stream
// counts, how many start where the one before ended, and the smallest and largest grid.x.
static void cond_plans() {
    const std::vector<int64_t> shapes = read_array<int64_t>("shapes.i64");
    REQUIRE(shapes.size() % 10 == 0);
    std::vector<int64_t> plans;
    plans.reserve(shapes.size() / 10 * 20);
    for (size_t r = 0; r * 10 < shapes.size(); ++r) {
        const int64_t* s = &shapes[r * 10];
        const int n_cus = (int)s[1];
        const int32_t n = (int32_t)s[3];
        const int64_t cap = persistent_cap(n_cus, (int)s[2]), a = s[4], b = s[5], stride = s[6];
        const uintptr_t in = (uintptr_t)s[7], out = (uintptr_t)s[8];
        if (s[0] == 7 || s[0] == 8) {   // the two single launches outside the stream loop
            const UnpackPlan u = s[0] == 8 ? unpack_plan(cap, out, stride, (int32_t)b, a, n) : UnpackPlan{(int)grid_widen((uint64_t)a, cap), 0, 0};
            for (int64_t v : {(int64_t)1, (int64_t)u.vec4, (int64_t)0, (int64_t)0, cap, (int64_t)0, (int64_t)0, (int64_t)u.grid, (int64_t)0, u.items}) plans.push_back(v);
            plans.insert(plans.end(), 10, 0);
            continue;
        }
        StagePlan p{};
        switch (s[0]) {
            case 0: p = stats_plan(cap, n, (int32_t)a); break;
            case 1: p = condition_plan(cap, kLevelStreams, in, out, n, stride, a); break;
            case 2: p = notch_plan(cap, kNotchStreams, n, (int32_t)a, (int32_t)b, kNotchLdsSamples, s[9] != 0); break;
            case 3: p = blank_plan(cap, kBlankStreams, n, (int32_t)a); break;
            case 4: p = hist_plan(cap, kBlankStreams, n, a); break;
            case 5: p = tones_plan(n_cus, n, (int32_t)a, (int32_t)b); break;
            case 6: p = quality_plan(n_cus, kQualityChans, n, (int32_t)a, (int32_t)b); break;
            case 9: p = excise_plan(cap, kExciseStreams, n, (int32_t)a); break;    // excise_launch's chunks
            case 10: p = excise_plan(cap, n, n, (int32_t)a); break;                // spectrum_hist_launch's one launch
            default: die("cond-plan: unknown stage");
        }
        REQUIRE(p.n_chunks >= 1);
        const StageChunk first = stage_chunk(p, 0), last = stage_chunk(p, p.n_chunks - 1);
        int64_t sum_ns = 0, max_ns = 0, in_order = 0, min_gx = INT64_MAX, max_gx = 0;
        for (int32_t i = 0; i < p.n_chunks; ++i) {
            const StageChunk c = stage_chunk(p, i);
            in_order += c.s0 == sum_ns && c.ns >= 1;
            sum_ns += c.ns;
            max_ns = std::max<int64_t>(max_ns, c.ns);
            min_gx = std::min<int64_t>(min_gx, c.grid_x);
            max_gx = std::max<int64_t>(max_gx, c.grid_x);
        }
        for (int64_t v : {(int64_t)p.n_chunks, (int64_t)p.vec4, p.lds_bytes, p.per_stream, p.cap, (int64_t)first.s0, (int64_t)first.ns, (int64_t)first.grid_x,
                          (int64_t)first.grid_y, first.items, (int64_t)last.s0, (int64_t)last.ns, (int64_t)last.grid_x, (int64_t)last.grid_y, last.items, sum_ns,
                          max_ns, in_order, min_gx, max_gx})
            plans.push_back(v);
    }
    Out("plans.i64").bytes(plans.data(), plans.size() * sizeof(int64_t));
}

// --------------------------------------------------------------------------------------------------------- cond-chain
// Conditioning::upstream_of for every combination of stages on and off and every stage measured.  chain.i64 rows: the combination
// (bit i: stage i of the chain is on), the stage, the conditioning before and after as cond_row lays it out.  A stage that is off
// holds values of its own too (a measurement had switched it off), except the notches, whose list is their switch.
static void cond_row(const Conditioning& c, std::vector<int64_t>& row) {
    auto bits = [](float f) { uint32_t u; std::memcpy(&u, &f, 4); return (int64_t)u; };
    for (int64_t v : {(int64_t)c.blank_on, bits(c.blanker.center_re), bits(c.blanker.center_im), bits(c.blanker.threshold), (int64_t)c.blanker.guard,
                      (int64_t)c.excise_on, bits(c.excisor.threshold), (int64_t)c.excisor.guard, (int64_t)c.excisor.reserved[0], (int64_t)c.excisor.reserved[1],
                      (int64_t)c.notches.count, (int64_t)c.notches.reserved})
        row.push_back(v);
    for (int64_t f : c.notches.freq_hz) row.push_back(f);
    for (int64_t v : {(int64_t)c.level_on, bits(c.level.dc_re), bits(c.level.dc_im), bits(c.level.gain), (int64_t)c.level.reserved}) row.push_back(v);
}
static void cond_chain() {
    std::vector<int64_t> rows;
    for (int combo = 0; combo < 16; ++combo)
        for (const Stage s : kChain) {
            Conditioning c;
            c.blank_on = combo & 1, c.blanker = gyp_blanker{1.5f + combo, -2.5f, 30.0f, 4};
            c.excise_on = (combo & 2) != 0, c.excisor = gyp_excisor{100.0f + combo, 1, {0, 0}};
            if (combo & 4) {
                c.notches.count = 3;
                for (int i = 0; i < 3; ++i) c.notches.freq_hz[i] = -403000 + 5000 * i + combo;
            }
            c.level_on = (combo & 8) != 0, c.level = gyp_iq_level{0.25f, -0.5f, 0.03125f * (1 + combo), 0};
            REQUIRE(c.on(Stage::blanker) == c.blank_on && c.on(Stage::excisor) == c.excise_on && c.on(Stage::notches) == ((combo & 4) != 0) &&
                    c.on(Stage::level) == c.level_on);
            rows.push_back(combo);
            rows.push_back((int64_t)s);
            cond_row(c, rows);
            cond_row(c.upstream_of(s), rows);
        }
    Out("chain.i64").bytes(rows.data(), rows.size() * sizeof(int64_t));
}

// --------------------------------------------------------------------------------------------------------- dev-mem
// The owners of dev_mem.hpp on a host without a device (every allocation fails), the scratch layouts, the table of debug switches on a
// context that lives on the stack.  No kernel is launched and no context is made through gyp_create.
template <class T>
static int64_t offset_of(const T* p, const void* base) { return (int64_t)((const uint8_t*)p - (const uint8_t*)base); }
static void dev_mem() {
    {
        DevBuf<float> a;
        REQUIRE(a.reserve(0, Slack::grow) == hipSuccess && a.get() == nullptr && a.capacity() == 0);   // enough already: nothing is asked of HIP
        REQUIRE(a.reserve(100, Slack::grow) != hipSuccess);
        REQUIRE(a.get() == nullptr && a.capacity() == 0);
        REQUIRE(a.reserve(7, Slack::exact, (hipStream_t) nullptr, (hipStream_t) nullptr) != hipSuccess);   // again, after the failure
        REQUIRE(a.get() == nullptr && a.capacity() == 0);
        DevBuf<float> b(std::move(a));
        DevBuf<float> c;
        c = std::move(b);
        REQUIRE(a.get() == nullptr && b.get() == nullptr && c.get() == nullptr && c.capacity() == 0);
        float* host = (float*)std::malloc(4 * sizeof(float));
        REQUIRE(upload(c, host, 4, nullptr) != hipSuccess && c.get() == nullptr && c.capacity() == 0);
        std::free(host);
        REQUIRE(c.release() == nullptr && c.reset() == hipSuccess);
        std::vector<DevBuf<uint8_t>> ring(3);
        for (auto& r : ring) REQUIRE(r.reserve(4096, Slack::exact) != hipSuccess && r.get() == nullptr);
        ring.resize(40);   // moved
        Event e;
        Stream s;
        if (e.create(hipEventDisableTiming) != hipSuccess) REQUIRE(e.get() == nullptr);
        if (s.create(hipStreamNonBlocking) != hipSuccess) REQUIRE(s.get() == nullptr);
        Event e2(std::move(e));
        Stream s2(std::move(s));
        REQUIRE(e.get() == nullptr && s.get() == nullptr);
        PinnedBuf p;
        p.adopt(std::malloc(100));
        REQUIRE(p.get() != nullptr);
        std::memset(p.get(), 1, 100);
        PinnedBuf q(std::move(p));
        REQUIRE(p.get() == nullptr && q.get()[99] == 1);
        PinnedBuf pinned;
        if (pinned.alloc(64) != hipSuccess) REQUIRE(pinned.get() == nullptr);
    }
    {   // layouts.i64: n_cells, n_rows, max_units.  carve.i64: per layout the offsets of its arrays in their order, then its size
        const std::vector<int64_t> in = read_array<int64_t>("layouts.i64");
        REQUIRE(in.size() == 3);
        const size_t n_cells = (size_t)in[0], n_rows = (size_t)in[1], max_units = (size_t)in[2];
        Out o("carve.i64");
        void* base = nullptr;
        REQUIRE(posix_memalign(&base, 256, 1 << 20) == 0);
        const AcqBook b0 = acq_book_layout(nullptr, n_cells), b = acq_book_layout(base, n_cells);
        REQUIRE(b0.prev_out == nullptr && b0.n_pend == nullptr && b0.bytes == b.bytes);
        REQUIRE(b.bytes == n_cells * (sizeof(gyp_cell) + 3 * sizeof(int32_t)) + 64);   // the size this buffer was always given
        REQUIRE((uint8_t*)(b.prev_out + n_cells) <= (uint8_t*)b.reuse && b.reuse + n_cells <= b.order && b.order + n_cells <= b.cand &&
                b.cand + n_cells <= b.n_active && b.n_active + 1 <= b.n_cand && b.n_cand + 1 <= b.n_pend && (uint8_t*)(b.n_pend + 1) <= (uint8_t*)base + b.bytes);
        for (int64_t v : {offset_of(b.prev_out, base), offset_of(b.reuse, base), offset_of(b.order, base), offset_of(b.cand, base),
                          offset_of(b.n_active, base), offset_of(b.n_cand, base), offset_of(b.n_pend, base), (int64_t)b.bytes})
            o.i64(v);
        const size_t n_grid = n_rows * 7;   // a refine call's cells: rows x bins
        GridRefineParams r{}, r0{};
        const size_t rb = refine_list_layout(base, n_rows, n_grid, &r);
        REQUIRE(refine_list_layout(nullptr, n_rows, n_grid, &r0) == rb && r0.cand == nullptr && rb == (n_grid + 2 * n_rows + 4) * sizeof(int32_t));
        REQUIRE(r.n_cand + 4 <= r.pend_rows && r.pend_rows + n_rows <= r.pend_first && r.pend_first + n_rows <= r.cand &&
                (uint8_t*)(r.cand + n_grid) <= (uint8_t*)base + rb);
        for (int64_t v : {offset_of(r.n_cand, base), offset_of(r.pend_rows, base), offset_of(r.pend_first, base), offset_of(r.cand, base), (int64_t)rb}) o.i64(v);
        AcqUnits u{}, u0{};
        const size_t ub = acq_units_layout(base, max_units, n_cells, &u);
        REQUIRE(acq_units_layout(nullptr, max_units, n_cells, &u0) == ub && u0.unit_cell == nullptr && ub == (max_units + 2 * n_cells + 4) * sizeof(int32_t));
        REQUIRE(u.unit_cell + max_units <= u.sh_cell && u.sh_cell + n_cells <= u.sh_unit && u.sh_unit + n_cells <= u.counts &&
                (uint8_t*)(u.counts + 4) <= (uint8_t*)base + ub);
        for (int64_t v : {offset_of(u.unit_cell, base), offset_of(u.sh_cell, base), offset_of(u.sh_unit, base), offset_of(u.counts, base), (int64_t)ub}) o.i64(v);
        std::free(base);
    }
    {   // switches.txt: name, lo, hi, integral, inherited, default of every row
        Out o("switches.txt");
        gyp_ctx ctx;
        for (const DebugSwitch& k : kDebugSwitches) {
            size_t same = 0;
            for (const DebugSwitch& other : kDebugSwitches) same += std::strcmp(k.name, other.name) == 0;
            REQUIRE(same == 1);
            double def = -777.0, got = -777.0;
            REQUIRE(gyp_debug_get(&ctx, k.name, &def) == GYP_OK && k.lo <= def && def <= k.hi);
            o.line(std::string(k.name) + " " + std::to_string(k.lo) + " " + std::to_string(k.hi) + " " + std::to_string((int)k.integral) + " " +
                   std::to_string((int)k.inherited) + " " + std::to_string(def));
            for (double v : {k.hi, k.lo}) {   // set, then get
                REQUIRE(gyp_debug_set(&ctx, k.name, v) == GYP_OK && gyp_debug_get(&ctx, k.name, &got) == GYP_OK && got == v);
            }
            const double inf = std::numeric_limits<double>::infinity();
            for (double v : {k.lo - 1.0, k.hi + 1.0, inf, -inf, std::numeric_limits<double>::quiet_NaN(), k.integral ? k.lo + 0.5 : inf}) {   // refused: the field stays
                REQUIRE(gyp_debug_set(&ctx, k.name, v) == GYP_E_BAD_ARG && gyp_debug_get(&ctx, k.name, &got) == GYP_OK && got == k.lo);
                REQUIRE(std::string(gyp_last_error(&ctx)).find(std::string("gyp_debug_set: ") + k.name + " must be ") == 0);
            }
            REQUIRE(gyp_debug_set(&ctx, k.name, def) == GYP_OK);
        }
        double got = 0.0;   // the two extra rules
        REQUIRE(gyp_debug_set(&ctx, "track_chunk_ms", 19.0) == GYP_E_BAD_ARG && gyp_debug_set(&ctx, "track_chunk_ms", 20.0) == GYP_OK &&
                gyp_debug_get(&ctx, "track_chunk_ms", &got) == GYP_OK && got == 20.0);
        REQUIRE(gyp_debug_set(&ctx, "grid_fused_waves", 10.0) == GYP_E_BAD_ARG && gyp_debug_get(&ctx, "grid_fused_waves", &got) == GYP_OK && got == 12.0);
        REQUIRE(gyp_debug_set(&ctx, "no_such_switch", 1.0) == GYP_E_BAD_ARG && gyp_debug_set(&ctx, "last_grid_path", 1.0) == GYP_E_BAD_ARG);
        REQUIRE(gyp_debug_get(&ctx, "last_grid_path", &got) == GYP_OK && got == 0.0 && gyp_debug_get(&ctx, "last_exact_path", &got) == GYP_OK &&
                gyp_debug_get(&ctx, "no_such_switch", &got) == GYP_E_BAD_ARG);
        REQUIRE(gyp_debug_set(&ctx, "last_track_flow", 1.0) == GYP_E_BAD_ARG && gyp_debug_get(&ctx, "last_track_flow", &got) == GYP_OK && got == 0.0);
        for (const char* name : {"last_acq_lanes", "last_acq_levels", "last_acq_shared_levels"})
            REQUIRE(gyp_debug_set(&ctx, name, 1.0) == GYP_E_BAD_ARG && gyp_debug_get(&ctx, name, &got) == GYP_OK && got == 0.0);
    }
    {   // a search that does not fit is refused before anything is planned into the context, reserved or launched (gyp_create's parameters and a
        // stream format by hand: no tables)
        gyp_ctx ctx;
        gyp_params_default(&ctx.params);
        ctx.fs = 8184000; ctx.n = 8184; ctx.k = 8;
        float iq = 0.0f;
        gyp_acq_result res{};
        const std::vector<int32_t> sats(33, 1);
        auto too_large = [&](int rc) { return rc == GYP_E_BAD_ARG && std::string(gyp_last_error(&ctx)).find("search too large") != std::string::npos && ctx.last_acq_plan.lanes == 0; };
        REQUIRE(too_large(gyp_acquire_dev(&ctx, &iq, 1, 8184, 65536, sats.data(), 1, &res)));
        REQUIRE(too_large(gyp_search_level_dev(&ctx, &iq, 1, 8184, 65536, sats.data(), 1, 0.0, 7000.0, &res)));
        REQUIRE(too_large(gyp_acquire_dev(&ctx, &iq, 2739138, 8184, 10, sats.data(), 28, &res)));
        REQUIRE(too_large(gyp_search_level_dev(&ctx, &iq, 2739138, 8184, 10, sats.data(), 28, 0.0, 7000.0, &res)));
        REQUIRE(gyp_acquire_dev(&ctx, &iq, 1, 8184, 0, sats.data(), 1, &res) == GYP_E_BAD_ARG && std::string(gyp_last_error(&ctx)) == "gyp_acquire_dev / gyp_search_level_dev: bad argument");
        REQUIRE(gyp_acquire_dev(&ctx, &iq, 8, 8184, 10, sats.data(), 33, &res) == GYP_E_BAD_ARG && ctx.helper[0] == nullptr);   // refused before a helper is made
    }
}

// --------------------------------------------------------------------------------------------------------- hybrid-plan
// plans.i64 rows in: n, n_cells, scratch_mb, flags, coherent_ms, n_blocks -> out: HybPlan's members in their order.  bins.f64 rows in:
// coherent_ms, center, spread, step -> bins.i64 out: hybrid_coarse_bins, hybrid_fine_half, the bits of the first and of the last coarse
// bin.  shifts.f64 rows in: n, coherent_ms, block, doppler, flags -> shifts.i64.  zs.f64 rows in: peak, n_off, sum_off, sumsq_off ->
// zs.f64 out.  searches.f64 rows in: n, n_streams, n_sats, coherent_ms, n_blocks, flags, center, spread, step, scratch_mb ->
// searches.i64 out: WeakSearchPlan's members and its run plan's; searches.txt: the refusal, or "ok".
static void put_plan(std::vector<int64_t>& o, const HybPlan& pl) {
    for (int64_t v : {(int64_t)pl.fits, (int64_t)pl.n_sets, (int64_t)pl.chunk_cells, (int64_t)pl.n_chunks, (int64_t)pl.profile, (int64_t)pl.power, (int64_t)pl.acc_x}) o.push_back(v);
}
static void hybrid_plans() {
    std::vector<int64_t> o;
    const std::vector<int64_t> shapes = read_array<int64_t>("plans.i64");
    REQUIRE(shapes.size() % 6 == 0);
    for (size_t r = 0; r * 6 < shapes.size(); ++r) {
        const int64_t* s = &shapes[r * 6];
        put_plan(o, hybrid_plan(HybShape{(int)s[0], s[1], (int)s[4], (int)s[5], (int)s[3]}, (int)s[2]));
    }
    Out("plans.i64").bytes(o.data(), o.size() * sizeof(int64_t));
    o.clear();
    const std::vector<double> bins = read_array<double>("bins.f64");
    for (size_t r = 0; r * 4 < bins.size(); ++r) {
        const double* b = &bins[r * 4];
        const int T = (int)b[0], n = hybrid_coarse_bins(b[1], b[2], T);
        const double first = hybrid_coarse_bin(b[1], b[2], T, 0), last = hybrid_coarse_bin(b[1], b[2], T, std::max(n - 1, 0));
        int64_t bits[2];
        std::memcpy(&bits[0], &first, 8);
        std::memcpy(&bits[1], &last, 8);
        for (int64_t v : {(int64_t)n, (int64_t)hybrid_fine_half(b[3], T), bits[0], bits[1]}) o.push_back(v);
    }
    Out("bins.i64").bytes(o.data(), o.size() * sizeof(int64_t));
    o.clear();
    const std::vector<double> shifts = read_array<double>("shifts.f64");
    for (size_t r = 0; r * 5 < shifts.size(); ++r) {
        const double* s = &shifts[r * 5];
        o.push_back(hybrid_shift((int32_t)s[0], (int32_t)s[1], (int32_t)s[2], s[3], (int32_t)s[4]));
        REQUIRE(gyp_hybrid_shift((int32_t)s[0], (int32_t)s[1], (int32_t)s[2], s[3], (int32_t)s[4]) == o.back());
    }
    Out("shifts.i64").bytes(o.data(), o.size() * sizeof(int64_t));
    o.clear();
    const std::vector<double> zs = read_array<double>("zs.f64");
    Out z_out("zs.f64");
    for (size_t r = 0; r * 4 < zs.size(); ++r) {
        gyp_hybrid_cell* c = (gyp_hybrid_cell*)std::calloc(1, sizeof(gyp_hybrid_cell));
        c->peak = (float)zs[r * 4]; c->n_off = (int32_t)zs[r * 4 + 1]; c->sum_off = zs[r * 4 + 2]; c->sumsq_off = zs[r * 4 + 3];
        double z = -777.0;
        REQUIRE(gyp_hybrid_stats(c, &z, nullptr) == GYP_OK);
        z_out.put(z);
        z_out.put((double)hybrid_pick_set(zs[r * 4 + 2], zs[r * 4 + 3]));   // (any two numbers of the row: the NaNs and the ties are among them)
        std::free(c);
    }
    const std::vector<double> searches = read_array<double>("searches.f64");
    Out why("searches.txt");
    for (size_t r = 0; r * 10 < searches.size(); ++r) {
        const double* s = &searches[r * 10];
        const WeakSearchPlan pl = weak_search_plan(WeakSearchShape{(int)s[0], (int)s[1], (int)s[2], (int)s[3], (int)s[4], (int)s[5], s[6], s[7], s[8]}, (int)s[9]);
        why.line(pl.refusal ? pl.refusal : "ok");
        for (int64_t v : {(int64_t)pl.n_coarse, (int64_t)pl.fine_half, (int64_t)pl.n_fine, pl.n_states, (int64_t)pl.coarse_cells, (int64_t)pl.fine_cells, (int64_t)pl.level_cells,
                          (int64_t)pl.records})
            o.push_back(v);
        put_plan(o, pl.run);
    }
    Out("searches.i64").bytes(o.data(), o.size() * sizeof(int64_t));
    {   // the plan's refusals reach the caller before anything is planned into the context, reserved or launched (a stream format by hand: no tables)
        gyp_ctx ctx;
        ctx.fs = 2046000; ctx.n = 2046; ctx.k = 2;
        float iq = 0.0f;
        gyp_weak_result res{};
        const std::vector<int32_t> sats(33, 1);
        auto refused = [&](int rc, const char* text) { return rc == GYP_E_BAD_ARG && std::string(gyp_last_error(&ctx)) == text && !ctx.last_hybrid_plan.fits && ctx.last_hybrid_plan.n_chunks == 0; };
        REQUIRE(refused(gyp_acquire_weak_dev(&ctx, &iq, 1, 2046, 1, 1, 0, 0.0, 1024250.0, 0.0, sats.data(), 1, &res), "gyp_acquire_weak_dev: a level must have between 1 and 4096 Doppler bins"));
        REQUIRE(refused(gyp_acquire_weak_dev(&ctx, &iq, 16385, 2046, 1, 1, 0, 0.0, 1024000.0, 0.0, sats.data(), 32, &res), "gyp_acquire_weak_dev: more than 2^31 - 1 cells"));
        REQUIRE(refused(gyp_acquire_weak_dev(&ctx, &iq, 1, 2046, 1, 1, 0, 0.0, 500.0, 0.0, sats.data(), 33, &res), "gyp_acquire_weak_dev: at most 32 satellites per call"));
        REQUIRE(refused(gyp_acquire_weak_dev(&ctx, &iq, 1, 2046, 1, 1, 0, 0.0, 0.0, 0.0, sats.data(), 1, &res), "gyp_acquire_weak_dev: center, spread and fine step must be finite and the spread positive"));
    }
}

// --------------------------------------------------------------------------------------------------------- weak-plan
// params.bin: gyp_weak_params records; inits.bin: gyp_chan_init records -> refusals.txt: a line each ("ok" where it is taken).
// fresh.i64 rows: n, cursor, then inits_fresh.bin's record of the same index -> fresh.bin: WeakChan records.  rates.f64 rows: f, n ->
// rates.i64.  advances.f64 rows: u0, f, fs and advances.i64 rows: c0, samples, r -> advanced.f64 (u0) and advanced.i64 (c0, and
// weak_mod_code of the row's c0).  sync.f32: rows of 40 prompts (re, im), sync.i64: the first_ms values -> sync.f64: per row and first_ms
// 20 energies and the pick.  loop.f32 rows: 26 x 20 milliseconds of m_re, m_im, p_re, p_im, l_re, l_im; loop.f64: f, u0, fs, pll_bw_hz, dll_bw_hz, lose_mu;
// loop.i64: c0, n, period_first -> periods.bin: 26 gyp_weak_period_rec records, chan.bin: the final WeakChan.
static void weak_plans() {
    {
        Out o("refusals.txt");
        const std::vector<uint8_t> prm = read_bytes("params.bin"), inits = read_bytes("inits.bin");
        for (size_t at = 0; at + sizeof(gyp_weak_params) <= prm.size(); at += sizeof(gyp_weak_params)) {
            gyp_weak_params* p = (gyp_weak_params*)std::malloc(sizeof(gyp_weak_params));
            std::memcpy(p, &prm[at], sizeof(*p));
            const char* why = weak_params_refusal(*p);
            o.line(why ? why : "ok");
            std::free(p);
        }
        for (size_t at = 0; at + sizeof(gyp_chan_init) <= inits.size(); at += sizeof(gyp_chan_init)) {
            gyp_chan_init* in = (gyp_chan_init*)std::malloc(sizeof(gyp_chan_init));
            std::memcpy(in, &inits[at], sizeof(*in));
            const char* why = weak_init_refusal(*in);
            o.line(why ? why : "ok");
            std::free(in);
        }
        const gyp_weak_params def = weak_params_default();
        REQUIRE(weak_params_refusal(def) == nullptr);
        Out("default.bin").put(def);
    }
    {
        const std::vector<int64_t> rows = read_array<int64_t>("fresh.i64");
        const std::vector<uint8_t> inits = read_bytes("inits_fresh.bin");
        REQUIRE(inits.size() == rows.size() / 2 * sizeof(gyp_chan_init));
        Out o("fresh.bin");
        for (size_t r = 0; r * 2 < rows.size(); ++r) {
            gyp_chan_init in;
            std::memcpy(&in, &inits[r * sizeof(in)], sizeof(in));
            o.put(weak_fresh_chan(in, (int32_t)rows[2 * r], rows[2 * r + 1]));
        }
    }
    {
        const std::vector<double> rates = read_array<double>("rates.f64"), adv = read_array<double>("advances.f64");
        const std::vector<int64_t> adv_i = read_array<int64_t>("advances.i64");
        Out ro("rates.i64"), af("advanced.f64"), ai("advanced.i64");
        for (size_t r = 0; r * 2 < rates.size(); ++r) ro.i64(weak_code_rate(rates[2 * r], (int32_t)rates[2 * r + 1]));
        REQUIRE(adv.size() == adv_i.size());
        for (size_t r = 0; r * 3 < adv.size(); ++r) {
            double u0 = adv[3 * r];
            int64_t c0 = weak_mod_code(adv_i[3 * r]);
            ai.i64(c0);
            weak_advance(&u0, &c0, adv[3 * r + 1], adv[3 * r + 2], adv_i[3 * r + 1], adv_i[3 * r + 2]);
            af.put(u0);
            ai.i64(c0);
        }
    }
    {
        const std::vector<float> prompts = read_array<float>("sync.f32");
        const std::vector<int64_t> firsts = read_array<int64_t>("sync.i64");
        const int32_t n_ms = 40;
        REQUIRE(prompts.size() % (2 * n_ms) == 0);
        float* p = (float*)std::malloc(2 * n_ms * sizeof(float));   // exactly n_ms prompts: a read one past is a report
        Out o("sync.f64");
        for (size_t row = 0; row * 2 * n_ms < prompts.size(); ++row) {
            std::memcpy(p, &prompts[row * 2 * n_ms], 2 * n_ms * sizeof(float));
            for (int64_t first : firsts) {
                double en[kWeakPeriodMs], api[kWeakPeriodMs];
                int32_t pick = -1;
                for (int k = 0; k < kWeakPeriodMs; ++k) o.put(en[k] = weak_bit_energy(p, n_ms, first, k));
                o.put((double)weak_bit_pick(en));
                REQUIRE(gyp_weak_bit_sync(p, n_ms, first, api, &pick) == GYP_OK && std::memcmp(api, en, sizeof(en)) == 0 && pick == weak_bit_pick(en));
            }
        }
        std::free(p);
    }
    {
        const std::vector<float> ms = read_array<float>("loop.f32");
        const std::vector<double> d = read_array<double>("loop.f64");
        const std::vector<int64_t> k = read_array<int64_t>("loop.i64");
        REQUIRE(ms.size() % (6 * kWeakPeriodMs) == 0 && d.size() == 6 && k.size() == 3);
        gyp_weak_params prm = weak_params_default();
        prm.pll_bw_hz = d[3]; prm.dll_bw_hz = d[4]; prm.lose_mu = d[5];
        WeakChan* s = (WeakChan*)std::calloc(1, sizeof(WeakChan));
        s->phase = kWeakTrack; s->f = s->f_int = d[0]; s->u0 = d[1]; s->c0 = k[0];
        Out periods("periods.bin");
        for (size_t period = 0; period * 6 * kWeakPeriodMs < ms.size(); ++period) {
            s->period_first = k[2] + (int64_t)period * kWeakPeriodMs;
            for (int i = 0; i < kWeakPeriodMs; ++i) {
                const float* m = &ms[(period * kWeakPeriodMs + i) * 6];
                weak_fold_ms(s, m[0], m[1], m[2], m[3], m[4], m[5]);
                s->pos += 1;
            }
            gyp_weak_period_rec rec;
            weak_close_period(s, prm, d[2], (int32_t)k[1], &rec);
            periods.put(rec);
        }
        Out("chan.bin").bytes(s, sizeof(WeakChan));
        std::free(s);
    }
}

}  // namespace drv

int main(int argc, char** argv) {
    if (argc != 4) drv::die("usage: prog <scenario> <in_dir> <out_dir>");
    std::string san;
#if __has_feature(address_sanitizer)
    san += " address";
#endif
#if __has_feature(thread_sanitizer)
    san += " thread";
#endif
#ifdef GYP_DRIVER_UBSAN
    san += " undefined";
#endif
    std::printf("sanitizers:%s\n", san.c_str());
    drv::g_in = argv[2];
    drv::g_out = argv[3];
    const std::pair<const char*, void (*)()> table[] = {
        {"ingest-host", drv::ingest_host}, {"ingest-races", drv::ingest_races}, {"bits", drv::bits}, {"spans", drv::spans},
        {"designs", drv::designs}, {"misc", drv::misc}, {"halo-readers", drv::halo_readers}, {"small-parsers", drv::small_parsers},
        {"grid-plan", drv::grid_plans}, {"track-plan", drv::track_plans}, {"acq-plan", drv::acq_plans}, {"resample-plan", drv::resample_plans},
        {"cond-plan", drv::cond_plans}, {"cond-chain", drv::cond_chain}, {"dev-mem", drv::dev_mem}, {"hybrid-plan", drv::hybrid_plans},
        {"weak-plan", drv::weak_plans},
    };
    for (const auto& s : table)
        if (std::string(argv[1]) == s.first) {
            s.second();
            std::fflush(stdout);
            return 0;
        }
    drv::die(std::string("unknown scenario ") + argv[1]);
}
