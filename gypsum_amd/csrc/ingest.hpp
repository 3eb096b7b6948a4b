// IQ ingest: recording file -> host ring (pinned) -> async H2D -> complex64 in HBM.
//
// The reference opens the file and np.fromfile()s 2N words for every millisecond
// (antenna_sample_provider.py:98-123).  Here one reader thread preads whole blocks of milliseconds into a ring of
// pinned buffers, the consumer's call enqueues the upload of the *next* block on a copy stream while the kernels of
// the current block run, and integer sample formats (RTL-SDR / HackRF raw int8, int16) cross PCIe in their file
// width and are widened to float32 pairs by a kernel on the device.  Values are exactly what
// `words[0::2] + 1j*words[1::2]` holds for the same dtype (no offset; no scaling unless gyp_ingest_set_scale asks).
#pragma once

#include <fcntl.h>
#include <pthread.h>
#include <sched.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <mutex>
#include <thread>

enum : int32_t { kFmtF32 = 0, kFmtI8 = 1, kFmtI16 = 2, kFmtU8 = 3 };

// ---------------------------------------------------------------------------------------------------------
// Host locality (SURVEY section 8 e: one process per GPU on an 8-GPU node).  A rank's reader thread and its pinned ring belong on
// the NUMA node its GPU hangs off: across the socket interconnect a pinned H2D stream loses bandwidth and eight ranks' rings
// would all land on the node the launcher happened to start on.  The GPU's node comes from sysfs (PCI bus id -> numa_node), the
// node's CPUs from /sys/devices/system/node/nodeN/cpulist; a host without that information (containers, single-node boxes
// reporting -1) is left alone.
// ---------------------------------------------------------------------------------------------------------
struct HostLocality {
    int numa_node = -1;
    std::string cpulist;       // as sysfs prints it, e.g. "0-31,128-159"
    cpu_set_t cpus;
    bool have_cpus = false;
};
static bool parse_cpulist(const std::string& text, cpu_set_t* set) {
    CPU_ZERO(set);
    int count = 0;
    const char* p = text.c_str();
    while (*p) {
        char* end = nullptr;
        const long a = std::strtol(p, &end, 10);
        if (end == p || a < 0) break;
        long b = a;
        p = end;
        if (*p == '-') {
            b = std::strtol(p + 1, &end, 10);
            if (end == p + 1 || b < a) break;
            p = end;
        }
        for (long c = a; c <= b && c < CPU_SETSIZE; ++c) { CPU_SET((int)c, set); ++count; }
        if (*p == ',') ++p;
        else break;
    }
    return count > 0;
}
static std::string read_small_file(const std::string& path) {
    std::string out;
    if (FILE* f = std::fopen(path.c_str(), "r")) {
        char buf[512];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof(buf), f)) > 0) out.append(buf, n);   // (a many-core host's cpulist can exceed one buffer)
        std::fclose(f);
        while (!out.empty() && (out.back() == '\n' || out.back() == ' ')) out.pop_back();
    }
    return out;
}
static HostLocality device_locality(int device) {
    HostLocality loc;
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int)sizeof(bus), device) != hipSuccess) return loc;
    for (char* c = bus; *c; ++c) *c = (char)std::tolower((unsigned char)*c);   // sysfs spells bus ids in lower case
    const std::string node = read_small_file(std::string("/sys/bus/pci/devices/") + bus + "/numa_node");
    if (node.empty()) return loc;
    loc.numa_node = std::atoi(node.c_str());
    if (loc.numa_node < 0) return loc;
    loc.cpulist = read_small_file("/sys/devices/system/node/node" + std::to_string(loc.numa_node) + "/cpulist");
    loc.have_cpus = parse_cpulist(loc.cpulist, &loc.cpus);
    return loc;
}
// While alive, the calling thread runs on the given CPUs (pinned pages are allocated on the node of the thread that asks for them).
struct ScopedAffinity {
    cpu_set_t saved;
    bool active = false;
    explicit ScopedAffinity(const HostLocality& loc) {
        if (!loc.have_cpus) return;
        if (pthread_getaffinity_np(pthread_self(), sizeof(saved), &saved) != 0) return;
        active = pthread_setaffinity_np(pthread_self(), sizeof(loc.cpus), &loc.cpus) == 0;
    }
    ~ScopedAffinity() {
        if (active) (void)pthread_setaffinity_np(pthread_self(), sizeof(saved), &saved);
    }
};

static inline int ingest_word_bytes(int32_t fmt) {
    switch (fmt) {
        case kFmtF32: return 4;
        case kFmtI16: return 2;
        case kFmtI8:
        case kFmtU8: return 1;
        default: return 0;
    }
}

// 16 input bytes per lane per iteration: coalesced dwordx4 loads, 64-256 B of contiguous float stores per lane.
template <class T>
__global__ __launch_bounds__(256) void ingest_widen_kernel(const T* __restrict__ raw, float* __restrict__ out, size_t n_words, float scale) {
    constexpr int kPer = 16 / sizeof(T);
    const size_t n_vec = n_words / kPer;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t v = (size_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_vec; v += stride) {
        const uint4 w = reinterpret_cast<const uint4*>(raw)[v];
        T e[kPer];
        __builtin_memcpy(e, &w, 16);
        float4* o = reinterpret_cast<float4*>(out + v * kPer);
#pragma unroll
        for (int i = 0; i < kPer / 4; ++i)
            o[i] = make_float4((float)e[4 * i] * scale, (float)e[4 * i + 1] * scale, (float)e[4 * i + 2] * scale, (float)e[4 * i + 3] * scale);
    }
    if (blockIdx.x == 0)   // tail (block sizes are multiples of 2N words, so this is at most 15 words)
        for (size_t i = n_vec * kPer + threadIdx.x; i < n_words; i += blockDim.x) out[i] = (float)raw[i] * scale;
}

// Packed I,Q words -> complex64 (gyp_unpack_iq_dev; the packed ingest at the context's rate).  The widen kernel's shape: a
// persistent grid, 16 aligned input bytes per lane per iteration, contiguous float stores.  Item (stream s, vector v) writes
// samples v*kS .. v*kS+kS-1 of stream s, whose 128 bits start e0 = 8 * (stream base mod 16) + bit0 bits into aligned block v:
// the lane loads blocks v and v+1 (v+1 only if those bits reach into it and it holds bytes of the stream), turns an MSB-first
// packing into a little-endian bit string and shifts it down by e0 (a select on e0 / 32, then v_alignbit), so word j of the
// item sits at bits [j*BITS, (j+1)*BITS).  An aligned block that holds any byte of the stream lies in that byte's page, so no
// load can fault beyond the buffer.  Values are levels[code] * scale from an LDS table: no dynamically indexed registers.
template <int BITS>
__device__ __forceinline__ uint32_t packed_lsb_first(uint32_t x) {   // reverse the order of the BITS-bit fields within each byte
    if (BITS == 1) x = ((x & 0x55555555u) << 1) | ((x >> 1) & 0x55555555u);
    if (BITS <= 2) x = ((x & 0x33333333u) << 2) | ((x >> 2) & 0x33333333u);
    return ((x & 0x0f0f0f0fu) << 4) | ((x >> 4) & 0x0f0f0f0fu);
}

template <int BITS>
__global__ __launch_bounds__(256) void ingest_unpack_kernel(const uint8_t* __restrict__ raw, int64_t in_stride, int32_t bit0,
                                                            int64_t n_samples, int32_t n_streams, const float* __restrict__ levels, float scale,
                                                            int32_t order, float2* __restrict__ out, int64_t out_stride, int32_t vec4) {
    __shared__ float tab[16];
    packed_table<BITS>(tab, levels, scale);
    __syncthreads();
    constexpr int kS = 64 / BITS;                 // samples per 16 bytes (2 BITS bits each)
    constexpr uint32_t kMask = (1u << BITS) - 1u;
    const bool msb = order == GYP_PACK_MSB_FIRST;
    const int64_t n_vec = (n_samples + kS - 1) / kS;
    const int64_t n_bytes = (bit0 + n_samples * (2 * BITS) + 7) >> 3;   // of each stream, from its base
    const int64_t n_items = n_vec * n_streams;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < n_items; it += stride) {
        const int64_t s = it / n_vec, v = it - s * n_vec;
        const uint8_t* base = raw + s * in_stride;
        const uint32_t a = (uint32_t)((uintptr_t)base & 15u);
        const uint4* blk = reinterpret_cast<const uint4*>(base - a);
        const uint32_t e0 = a * 8u + (uint32_t)bit0;   // 0 .. 127
        const uint4 w0 = blk[v];                       // holds the stream's byte (e0 + 128 v) / 8
        const uint4 w1 = (e0 != 0 && 16 * (v + 1) < a + n_bytes) ? blk[v + 1] : make_uint4(0u, 0u, 0u, 0u);
        uint32_t d[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
        if (msb) {
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = packed_lsb_first<BITS>(d[k]);
        }
        const uint32_t q = e0 >> 5, r = e0 & 31u;
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t lo = q == 0 ? d[k] : q == 1 ? d[k + 1] : q == 2 ? d[k + 2] : d[k + 3];
            const uint32_t hi = q == 0 ? d[k + 1] : q == 1 ? d[k + 2] : q == 2 ? d[k + 3] : d[k + 4];
            w[k] = __builtin_amdgcn_alignbit(hi, lo, r);
        }
        const int64_t n0 = v * kS;
        float2* o = out + s * out_stride + n0;
#define GYP_WORD(j) tab[(w[((j) * BITS) >> 5] >> (((j) * BITS) & 31)) & kMask]
        if (vec4 && n0 + kS <= n_samples) {
#pragma unroll
            for (int i = 0; i < kS / 2; ++i)
                reinterpret_cast<float4*>(o)[i] = make_float4(GYP_WORD(4 * i), GYP_WORD(4 * i + 1), GYP_WORD(4 * i + 2), GYP_WORD(4 * i + 3));
        } else {
#pragma unroll
            for (int i = 0; i < kS; ++i)
                if (n0 + i < n_samples) o[i] = make_float2(GYP_WORD(2 * i), GYP_WORD(2 * i + 1));
        }
#undef GYP_WORD
    }
}

// A validated packing as the kernels take it.
struct PackedFormat {
    int32_t bits = 0, order = 0;
    bool real = false;
    PackedLevels levels{};
    int64_t sample_bits() const { return (int64_t)bits * (real ? 1 : 2); }
};
// GYP_E_BAD_ARG's reason, or nullptr if the packing is valid (then *out holds it).
static const char* packing_check(const gyp_packing* p, PackedFormat* out) {
    if (!p) return "packing is NULL";
    if (p->bits != 1 && p->bits != 2 && p->bits != 4) return "packing.bits must be 1, 2 or 4";
    if (p->real != 0 && p->real != 1) return "packing.real must be 0 or 1";
    if (p->order != GYP_PACK_MSB_FIRST && p->order != GYP_PACK_LSB_FIRST) return "packing.order must be GYP_PACK_MSB_FIRST or GYP_PACK_LSB_FIRST";
    if (p->reserved != 0) return "packing.reserved must be 0";
    PackedFormat f;
    f.bits = p->bits;
    f.order = p->order;
    f.real = p->real == 1;
    for (int c = 0; c < (1 << p->bits); ++c) {
        if (!std::isfinite(p->levels[c])) return "packing.levels[c] must be finite for every code c < 2^bits";
        f.levels.v[c] = p->levels[c];
    }
    if (out) *out = f;
    return nullptr;
}

// Where samples first .. first+n-1 lie in a packed file of file_samples samples of B bits: the part inside the file and the bytes
// that cover it (all zero if none).  gyp_packed_span is this function; the ingest reads exactly these bytes.
struct PackedSpan {
    int64_t in_first = 0, in_n = 0, first_byte = 0, n_bytes = 0;
    int32_t bit0 = 0;
};
static PackedSpan packed_span(int64_t B, int64_t file_samples, int64_t first, int64_t n) {
    PackedSpan sp;
    const int64_t a = std::max<int64_t>(first, 0), b = std::min<int64_t>(first + n, file_samples);
    if (b <= a) return sp;
    sp.in_first = a;
    sp.in_n = b - a;
    sp.first_byte = a * B / 8;
    sp.bit0 = (int32_t)(a * B % 8);
    sp.n_bytes = (b * B + 7) / 8 - sp.first_byte;
    return sp;
}

// ---------------------------------------------------------------------------------------------------------
// The handle.  Everything below is host code without a HIP call: what the file holds, where a block's samples lie in it, how many
// milliseconds it has, the reader thread and the take / release protocol.  What launches or copies is in gypsum_hip.hip.
// ---------------------------------------------------------------------------------------------------------
// What the file holds and how the device turns it into the stream format:
//   plain            I,Q words at the output rate, widened (float32: uploaded as they are)              gyp_ingest_open
//   filtered         I,Q or real words at another rate, resampled / down-converted from if_hz           gyp_ingest_open_resampled / _ddc
//   packed_native    packed I,Q words at the output rate, unpacked                                      gyp_ingest_open_packed
//   packed_filtered  packed I,Q or real words at another rate, resampled / down-converted               gyp_ingest_open_packed
enum class SourceKind : int32_t { plain, filtered, packed_native, packed_filtered };

// One handle's source, built by ingest_describe at open and never written afterwards: the reader thread reads it without the lock.
// A block of output milliseconds [first, first + n_ms) needs input samples first*in_n - halo_lo .. (first+n_ms)*in_n + halo_hi - 1
// (ingest_span); an unfiltered source has in_n == n and no halo.
struct IngestSource {
    SourceKind kind = SourceKind::plain;
    int32_t fmt = kFmtF32;    // the words of plain and filtered sources
    PackedFormat pk{};        // the words of packed sources
    bool real = false;        // one real word per sample, mixed down from if_hz (the mixer index is the file index)
    int64_t if_hz = 0;
    ResampleDesign rs{};      // filtered sources
    int32_t n = 0, in_n = 0;  // samples per millisecond of the output and of the file
    int32_t halo_lo = 0, halo_hi = 0;
    int64_t sample_bits = 0;  // one input sample in the file
    int32_t block_ms = 0, depth = 0;
    size_t host_block_bytes = 0, raw_block_bytes = 0;   // one ring slot on the host / of file-width words on the device (0: none)
    bool packed() const { return kind == SourceKind::packed_native || kind == SourceKind::packed_filtered; }
    bool filtered() const { return kind == SourceKind::filtered || kind == SourceKind::packed_filtered; }
};

// A block's input samples [s0, s0 + count), their part inside the file with the bytes that cover it (PackedSpan; a width that is a
// multiple of 8 has bit0 == 0), and what a ring slot holds for it: pad_lo zero bytes, the n_bytes of the file, pad_hi zero bytes.
// Word formats pad to the whole window (the kernel indexes from s0); packed blocks are the file's bytes as they are (the kernel
// is given in_first and bit0).
struct IngestSpan : PackedSpan {
    int64_t s0 = 0, count = 0, pad_lo = 0, pad_hi = 0;
    int64_t slot_bytes() const { return pad_lo + n_bytes + pad_hi; }
};
static IngestSpan ingest_span(const IngestSource& s, int64_t file_samples, int64_t first_ms, int32_t n_ms) {
    IngestSpan sp;
    sp.s0 = first_ms * s.in_n - s.halo_lo;
    sp.count = (int64_t)n_ms * s.in_n + s.halo_lo + s.halo_hi;
    static_cast<PackedSpan&>(sp) = packed_span(s.sample_bits, file_samples, sp.s0, sp.count);
    if (!s.packed()) {
        const int64_t sample_bytes = s.sample_bits / 8;
        sp.pad_lo = (sp.in_n ? sp.in_first - sp.s0 : sp.count) * sample_bytes;
        sp.pad_hi = sp.count * sample_bytes - sp.pad_lo - sp.n_bytes;
    }
    return sp;
}

// The source of a file of `fmt` words (pk null) or of `pk` packed words, filtered by design d (taps, n_in, n_out, real) or, with
// d.taps == 0, at the output rate already (n_in == n_out).  A filter of T taps reaches T/2 - 1 samples back and T/2 ahead.
// A ring slot holds the largest block: block_ms milliseconds with the halo, for packed words at any bit0, plus one byte.
static IngestSource ingest_describe(int32_t fmt, const PackedFormat* pk, const ResampleDesign& d, int64_t if_hz, int32_t block_ms, int32_t depth) {
    IngestSource s;
    const bool filtered = d.taps > 0;
    s.kind = pk ? (filtered ? SourceKind::packed_filtered : SourceKind::packed_native) : (filtered ? SourceKind::filtered : SourceKind::plain);
    s.fmt = fmt;
    if (pk) s.pk = *pk;
    s.real = d.real;
    s.if_hz = if_hz;
    s.rs = d;
    s.n = d.n_out;
    s.in_n = d.n_in;
    if (filtered) {
        s.halo_lo = d.taps / 2 - 1;
        s.halo_hi = d.taps / 2;
    }
    s.sample_bits = pk ? pk->sample_bits() : (int64_t)8 * ingest_word_bytes(fmt) * (d.real ? 1 : 2);
    s.block_ms = block_ms;
    s.depth = depth;
    s.host_block_bytes = (size_t)((ingest_span(s, 0, 0, block_ms).count * s.sample_bits + 7) / 8 + (pk ? 1 : 0));
    // (float32 at the output rate lands in the output slot directly: no device slot of raw words)
    s.raw_block_bytes = s.kind == SourceKind::plain && fmt == kFmtF32 ? 0 : s.host_block_bytes;
    return s;
}
// The design of a source that is not filtered: n samples per millisecond in and out.
static ResampleDesign ingest_unfiltered(int32_t n) {
    ResampleDesign d;
    d.n_in = d.n_out = n;
    return d;
}

// A file's whole samples, and the milliseconds the reference provider delivers from it before NoMoreSamplesError: it stops one
// word short of the end, so word formats count (bytes - 1) / millisecond bytes; packed files count in samples (gyp_packed_span).
struct IngestExtent {
    int64_t total_ms = 0, file_samples = 0;
};
static IngestExtent ingest_extent(const IngestSource& s, int64_t file_bytes) {
    IngestExtent e;
    e.file_samples = file_bytes * 8 / s.sample_bits;
    if (s.packed()) e.total_ms = e.file_samples > 0 ? (e.file_samples - 1) / s.in_n : 0;
    else e.total_ms = file_bytes > 0 ? (file_bytes - 1) / (s.in_n * s.sample_bits / 8) : 0;
    return e;
}

// The conditioning chain: what is applied in place to every device block behind its producer, on the copy stream, in this order.
// It is written here only: ingest_condition walks it, and a measurement sees what is in front of its stage (Conditioning::upstream_of).
enum class Stage : int32_t { blanker, excisor, notches, level };
constexpr Stage kChain[] = {Stage::blanker, Stage::excisor, Stage::notches, Stage::level};
// The stages' switches and values.  One value, so that a measurement can put it aside and back whole (ingest_measure_range); a
// stage that is off holds what it is initialised with here, or what it held when a measurement switched it off.
struct Conditioning {
    bool level_on = false;     // gyp_ingest_set_level / gyp_ingest_calibrate
    gyp_iq_level level{0.0f, 0.0f, 1.0f, 0};
    gyp_notch_tones notches{};   // gyp_ingest_set_notches / gyp_ingest_find_tones
    bool blank_on = false;     // gyp_ingest_set_blanker / gyp_ingest_find_pulses
    gyp_blanker blanker{0.0f, 0.0f, 1.0f, 0};
    bool excise_on = false;    // gyp_ingest_set_excisor / gyp_ingest_find_excisor
    gyp_excisor excisor{1.0f, 0, {0, 0}};
    bool on(Stage s) const {
        return s == Stage::blanker ? blank_on : s == Stage::excisor ? excise_on : s == Stage::notches ? notches.count > 0 : level_on;
    }
    // The conditioning of the blocks the measurement of stage s sees: s and everything behind it off.  What is switched off keeps
    // its values, except the notches, whose list is their switch.
    Conditioning upstream_of(Stage s) const {
        Conditioning c = *this;
        for (const Stage t : kChain) {
            if (t < s) continue;
            if (t == Stage::notches) c.notches = gyp_notch_tones{};
            else (t == Stage::blanker ? c.blank_on : t == Stage::excisor ? c.excise_on : c.level_on) = false;
        }
        return c;
    }
};

// What gyp_ingest_last_blanked and _last_excised read: a counting stage's count per millisecond of the block in each device slot.
struct SlotCounts {
    std::vector<DevBuf<int32_t>> dev;   // per slot: block_ms words
    std::vector<uint8_t> went;          // per slot: the block in it went through the stage
    // Slots [what there is, depth) of block_ms words each: nothing where they exist.  After a failure the slots made so far stay.
    hipError_t ensure(int32_t depth, int32_t block_ms) {
        while ((int32_t)dev.size() < depth) {
            DevBuf<int32_t> slot;
            if (const hipError_t e = slot.reserve((size_t)block_ms, Slack::exact)) return e;
            dev.push_back(std::move(slot));
            went.push_back(0);
        }
        return hipSuccess;
    }
    void mark(int d, bool through) { if (d < (int)went.size()) went[d] = through ? 1 : 0; }
    bool passed(int d) const { return d < (int)went.size() && went[d]; }
};

struct gyp_ingest {
    gyp_ingest(gyp_ctx* c, int64_t fs_hz, const IngestSource& s) : ctx(c), fs(fs_hz), src(s) {}
    gyp_ctx* const ctx;       // null: host-only (no pinned memory, no device ring)
    const int64_t fs;         // the output rate
    const IngestSource src;
    int fd = -1;
    float scale = 1.0f;       // integer and packed words only: sample = word * scale (1 = the reference's raw values)
    int64_t total_ms = 0, file_samples = 0;   // ingest_extent of the file as it was at open
    HostLocality locality;    // the GPU's NUMA node: the pinned ring is allocated there and the reader thread runs there
    Conditioning cond;
    int64_t consumer_ms = 0;        // where the next block handed out starts (set_level and calibrate seek back to it)

    // host ring, filled by the reader thread
    std::vector<uint8_t*> host;
    std::vector<PinnedBuf> host_mem;   // owns what `host` points to (empty where the caller supplied and frees the blocks)
    std::vector<int64_t> host_first;
    std::vector<int32_t> host_ms;
    std::thread reader;
    std::mutex mu;
    std::condition_variable cv;
    int64_t cursor_ms = 0;          // next millisecond the reader will read
    int64_t produced = 0, taken = 0, released = 0;   // block counters: read / handed to the consumer / slot reusable
    bool eof = false, stop = false;
    int io_errno = 0;

    // device ring
    Stream copy_stream;              // (declared before everything used on it: destroyed last)
    std::vector<DevBuf<uint8_t>> dev_raw;   // file-width words (unused for float32: the upload lands in dev_iq directly)
    std::vector<DevBuf<float>> dev_iq;
    SlotCounts blanked;              // the blanker's counts, made at open
    SlotCounts excised;              // the excisor's, made when the handle first gets an excisor: one that never does allocates nothing
    SlotCounts* counts_of(Stage s) { return s == Stage::blanker ? &blanked : s == Stage::excisor ? &excised : nullptr; }
    Stream counts_stream;            // ingest_last_counts' download (made by its first call: it must not wait for anything else)
    int last_slot = -1;              // the device slot of the block most recently handed out (-1: none since open / seek)
    int32_t last_n_ms = 0;
    std::vector<Event> uploaded, ready;
    Event consumer_mark;
    struct Upload {
        int64_t block, first_ms;
        int32_t n_ms;
        int host_slot;
    };
    std::deque<Upload> in_flight;    // uploads enqueued whose host slot is not yet released
    bool have_ahead = false;         // the next block's upload is already enqueued
    Upload ahead{};
    int64_t dev_blocks = 0;          // uploads enqueued so far (device slot = index % depth)
};

// Opens the file, measures it and sizes the (still empty) host ring's tables.  0 or an errno.
static int ingest_open_file(gyp_ingest* g, const char* path) {
    g->fd = open(path, O_RDONLY | O_CLOEXEC);
    struct stat st;
    if (g->fd < 0 || fstat(g->fd, &st) != 0) return errno;
    const IngestExtent e = ingest_extent(g->src, (int64_t)st.st_size);
    g->total_ms = e.total_ms;
    g->file_samples = e.file_samples;
    (void)posix_fadvise(g->fd, 0, 0, POSIX_FADV_SEQUENTIAL);
    g->host.assign(g->src.depth, nullptr);
    g->host_first.assign(g->src.depth, 0);
    g->host_ms.assign(g->src.depth, 0);
    return 0;
}

// pread until `want` bytes from file offset `at` are in: 0, or an errno (EIO: the file shrank under us).
static int pread_fully(int fd, uint8_t* buf, size_t want, size_t at) {
    for (size_t got = 0; got < want;) {
        const ssize_t r = pread(fd, buf + got, want - got, (off_t)(at + got));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return r < 0 ? errno : EIO;
        got += (size_t)r;
    }
    return 0;
}

static void ingest_reader_main(gyp_ingest* g) {
    const int32_t depth = g->src.depth;
    for (;;) {
        int slot;
        int64_t first;
        int32_t n_ms;
        {
            std::unique_lock<std::mutex> lk(g->mu);
            g->cv.wait(lk, [&] { return g->stop || (!g->eof && g->produced - g->released < depth); });
            if (g->stop) return;
            first = g->cursor_ms;
            n_ms = (int32_t)std::min<int64_t>(g->src.block_ms, g->total_ms - first);
            if (n_ms <= 0) {
                g->eof = true;
                g->cv.notify_all();
                continue;
            }
            slot = (int)(g->produced % depth);
        }
        // the slot's content, whatever the kind: zeros where the span says, then the file's bytes
        uint8_t* buf = g->host[slot];
        const IngestSpan sp = ingest_span(g->src, g->file_samples, first, n_ms);
        std::memset(buf, 0, (size_t)sp.pad_lo);
        std::memset(buf + sp.pad_lo + sp.n_bytes, 0, (size_t)sp.pad_hi);
        const int err = pread_fully(g->fd, buf + sp.pad_lo, (size_t)sp.n_bytes, (size_t)sp.first_byte);
        std::lock_guard<std::mutex> lk(g->mu);
        if (err) {
            g->io_errno = err;
            g->eof = true;
        } else {
            g->host_first[slot] = first;
            g->host_ms[slot] = n_ms;
            g->cursor_ms = first + n_ms;
            ++g->produced;
        }
        g->cv.notify_all();
    }
}

static void ingest_stop_reader(gyp_ingest* g) {
    if (!g->reader.joinable()) return;
    {
        std::lock_guard<std::mutex> lk(g->mu);
        g->stop = true;
    }
    g->cv.notify_all();
    g->reader.join();
    g->stop = false;
}

static void ingest_start_reader(gyp_ingest* g, int64_t at_ms) {
    g->cursor_ms = at_ms;
    g->produced = g->taken = g->released = 0;
    g->eof = false;
    g->io_errno = 0;
    g->reader = std::thread(ingest_reader_main, g);
    if (g->locality.have_cpus)   // (best effort: a cpuset that forbids those CPUs leaves the thread where it is)
        (void)pthread_setaffinity_np(g->reader.native_handle(), sizeof(g->locality.cpus), &g->locality.cpus);
}

// Blocks until the reader has a block; returns false at end of data (or on an I/O error, see io_errno).
static bool ingest_take(gyp_ingest* g, int* slot, int64_t* first, int32_t* n_ms, bool wait) {
    std::unique_lock<std::mutex> lk(g->mu);
    if (wait) g->cv.wait(lk, [&] { return g->produced > g->taken || g->eof; });
    if (g->produced <= g->taken) return false;
    *slot = (int)(g->taken % g->src.depth);
    *first = g->host_first[*slot];
    *n_ms = g->host_ms[*slot];
    ++g->taken;
    return true;
}

static void ingest_release(gyp_ingest* g, int64_t up_to_block /* exclusive */) {
    std::lock_guard<std::mutex> lk(g->mu);
    if (up_to_block > g->released) g->released = up_to_block;
    g->cv.notify_all();
}

