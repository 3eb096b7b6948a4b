// dev_mem.hpp -- move-only owners of what the host side holds: device memory, host blocks, events, streams.  Host code only.
// A destructor releases what its object holds and does nothing when it is empty, so a context, a bank or an ingest handle is torn
// down by `delete`.  Members go in reverse order of declaration: declare a stream BEFORE the buffers and events used on it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <utility>

namespace gyp {

// How DevBuf::reserve sizes a new allocation: exactly what was asked for (a bank's buffers), or with room to grow, bytes +
// bytes / 4 + 4096 (the scratch of the entry points, whose shapes change from call to call).
enum class Slack { exact, grow };

template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : cap_(o.cap_), p_(o.release()) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { (void)reset(); cap_ = o.cap_; p_ = o.release(); }
        return *this;
    }
    ~DevBuf() { (void)reset(); }
    T* get() const { return p_; }
    T* release() { cap_ = 0; return std::exchange(p_, nullptr); }
    size_t capacity() const { return cap_; }   // in elements; 0 when empty
    hipError_t reset() { return p_ ? hipFree(release()) : hipSuccess; }
    // Room for `count` elements.  No HIP call when the capacity suffices; else whatever may still use the old memory on `streams`
    // is waited for, the old memory is freed and new memory allocated (contents are not kept).  After a failure the object is empty.
    template <typename... Streams>
    hipError_t reserve(size_t count, Slack slack, Streams... streams) {
        if (cap_ >= count) return hipSuccess;
        if (p_) {
            const hipStream_t used[sizeof...(Streams) + 1] = {streams...};   // (a stream not created yet is null: nothing ran on it)
            hipError_t e = hipSuccess;
            for (size_t i = 0; i < sizeof...(Streams); ++i)
                if (used[i] && e == hipSuccess) e = hipStreamSynchronize(used[i]);
            const hipError_t ef = reset();
            if (e != hipSuccess || ef != hipSuccess) return e != hipSuccess ? e : ef;
        }
        const size_t bytes = count * sizeof(T), room = slack == Slack::grow ? bytes + bytes / 4 + 4096 : bytes;
        const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p_), room);
        if (e != hipSuccess) p_ = nullptr;
        else cap_ = room / sizeof(T);
        return e;
    }
private:
    size_t cap_ = 0;
    T* p_ = nullptr;
};

// Room for `count` + `pad` elements (Slack::grow), then the copy of host[0 .. count) enqueued on `stream`, which is also the stream
// the buffer's earlier contents were used on.  The host array must stay valid until the stream has passed the copy.
template <typename T>
hipError_t upload(DevBuf<T>& buf, const T* host, size_t count, hipStream_t stream, size_t pad = 0) {
    const hipError_t e = buf.reserve(count + pad, Slack::grow, stream);
    return e != hipSuccess ? e : hipMemcpyAsync(buf.get(), host, count * sizeof(T), hipMemcpyHostToDevice, stream);
}

// Typed, aligned sub-arrays of one allocation, handed out in the order asked for.  A layout is a function that take()s its arrays
// from a Carve: run on a null base it yields the size to allocate (bytes()), run on the buffer the pointers -- one list for both.
class Carve {
public:
    explicit Carve(void* base) : base_(static_cast<uint8_t*>(base)) {}
    template <typename T>
    T* take(size_t count) {
        at_ = (at_ + alignof(T) - 1) / alignof(T) * alignof(T);
        T* p = base_ ? reinterpret_cast<T*>(base_ + at_) : nullptr;
        at_ += count * sizeof(T);
        return p;
    }
    size_t bytes() const { return at_; }
private:
    uint8_t* base_;
    size_t at_ = 0;
};

// A HIP event or stream: create(flags) makes it once (later calls do nothing), the destructor destroys it.
template <typename H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H)>
class Handle {
public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    ~Handle() { if (h_) (void)Destroy(h_); }
    hipError_t create(unsigned flags) { return h_ ? hipSuccess : Create(&h_, flags); }
    H get() const { return h_; }
private:
    H h_ = nullptr;
};
using Event = Handle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;

// A block of host memory: pinned (hipHostMalloc), or, for a user without a device, memory of the C library (freed with free()).
class PinnedBuf {
public:
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), pinned_(o.pinned_) {}
    ~PinnedBuf() { pinned_ ? (void)hipHostFree(p_) : std::free(p_); }
    hipError_t alloc(size_t bytes) {   // (an empty object's)
        const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p_), bytes, hipHostMallocDefault);
        if (e != hipSuccess) p_ = nullptr;
        pinned_ = p_ != nullptr;
        return e;
    }
    uint8_t* adopt(void* from_malloc) { return p_ = static_cast<uint8_t*>(from_malloc); }   // (an empty object's)
    uint8_t* get() const { return p_; }
private:
    uint8_t* p_ = nullptr;
    bool pinned_ = false;
};

}  // namespace gyp
