// rph_buffers.h -- the library's host-side plumbing (included through rph_internal.h): status macros, growable device and pinned
// buffers, context scratch shared by caller streams, and the host thread pool.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <thread>
#include <vector>

#include "../../include/rupphash.h"

void rph_set_error(const char *fmt, ...);

#define RPH_HIP_CHECK(expr)                                                                  \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            rph_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return e_ == hipErrorOutOfMemory ? RPH_ERR_OOM : RPH_ERR_HIP;                    \
        }                                                                                    \
    } while (0)

#define RPH_TRY(expr)                  \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != RPH_OK) return rc_; \
    } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// Sections of one buffer, one behind the other: add(bytes, align) places the next section at the first multiple of `align` behind the
// last one and returns its offset; end() is where the last section ends
class Layout {
  public:
    size_t add(size_t bytes, size_t align = 1)
    {
        const size_t off = align_up(end_, align);
        end_ = off + bytes;
        return off;
    }
    size_t end() const { return end_; }

  private:
    size_t end_ = 0;
};

// reserve() argument: the caller has already synchronised every stream whose work uses the buffer
struct Synced {};
constexpr Synced synced{};

// Device (DevBuf) or pinned host (PinnedBuf) memory, move-only, freed by its destructor.  Kernels may write pinned memory directly.
template <bool Pinned>
class Buffer {
  public:
    Buffer() = default;
    Buffer(Buffer &&o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
    Buffer &operator=(Buffer &&o) noexcept
    {
        if (this != &o) {
            reset();
            std::swap(p_, o.p_);
            std::swap(cap_, o.cap_);
        }
        return *this;
    }
    ~Buffer() { reset(); }

    uint8_t *data() const { return p_; }
    template <class T>
    T *as() const
    {
        return reinterpret_cast<T *>(p_);
    }
    size_t capacity() const { return cap_; }

    void reset()  // nothing in flight may use the buffer any more
    {
        if (p_) (void)(Pinned ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
    }
    // a new buffer of `bytes` (at least 1) in place of the old one
    int alloc(size_t bytes)
    {
        reset();
        bytes = std::max<size_t>(bytes, 1);
        RPH_HIP_CHECK(Pinned ? hipHostMalloc((void **)&p_, bytes) : hipMalloc((void **)&p_, bytes));
        cap_ = bytes;
        return RPH_OK;
    }
    // capacity() >= need afterwards.  A buffer that grows gets `bytes` (>= need: the caller's slack); the old one, if any, is freed once
    // `user`, the stream whose work uses it, has been synchronised -- or at once with `synced`.
    int reserve(size_t need, size_t bytes, hipStream_t user)
    {
        if (cap_ >= need) return RPH_OK;
        if (p_) RPH_HIP_CHECK(hipStreamSynchronize(user));
        return alloc(bytes);
    }
    int reserve(size_t need, size_t bytes, Synced) { return cap_ >= need ? RPH_OK : alloc(bytes); }
    int reserve(size_t need, hipStream_t user) { return reserve(need, need, user); }
    int reserve(size_t need, Synced s) { return reserve(need, need, s); }

  private:
    uint8_t *p_ = nullptr;
    size_t cap_ = 0;
};
using DevBuf = Buffer<false>;
using PinnedBuf = Buffer<true>;

// Device scratch owned by the context and shared by every caller stream.  Each use is acquire(stream, ...), the launches, publish(stream),
// all under ctx->mu.  acquire makes `stream` wait for the event of the last user when that user ran on another stream; publish records the
// event on `stream`.  Since every user publishes, the last event comes after the last user's work, and that user was itself ordered
// behind the one before it: the event covers all earlier users.  Growing frees the old buffer after hipDeviceSynchronize, because kernels
// of any stream may still use it.
class SharedScratch {
  public:
    SharedScratch() = default;
    SharedScratch(const SharedScratch &) = delete;
    SharedScratch &operator=(const SharedScratch &) = delete;
    ~SharedScratch()
    {
        if (done_) (void)hipEventDestroy(done_);
    }

    uint8_t *data() const { return buf_.data(); }
    template <class T>
    T *as() const
    {
        return buf_.as<T>();
    }
    size_t capacity() const { return buf_.capacity(); }

    int acquire(hipStream_t stream, size_t need, size_t bytes)  // bytes >= need: the caller's slack when the scratch grows
    {
        if (buf_.capacity() < need) {
            RPH_HIP_CHECK(hipDeviceSynchronize());
            RPH_TRY(buf_.alloc(bytes));
        }
        if (!done_) RPH_HIP_CHECK(hipEventCreateWithFlags(&done_, hipEventDisableTiming));
        if (used_ && last_ != stream) RPH_HIP_CHECK(hipStreamWaitEvent(stream, done_, 0));
        return RPH_OK;
    }
    int acquire(hipStream_t stream, size_t need) { return acquire(stream, need, need); }
    int publish(hipStream_t stream)
    {
        RPH_HIP_CHECK(hipEventRecord(done_, stream));
        last_ = stream;
        used_ = true;
        return RPH_OK;
    }
    void forget_stream(hipStream_t stream)  // `stream` has been synchronised and is going away: nothing left to order behind
    {
        if (last_ == stream) used_ = false;
    }

  private:
    DevBuf buf_;
    hipEvent_t done_ = nullptr;
    hipStream_t last_ = nullptr;
    bool used_ = false;
};

// One use of a context's shared scratch on `s`, under ctx->mu: published on every way out of the scope, an error's included, so that
// the next user on another stream is ordered behind whatever this one had enqueued.  done() is the ordinary end and reports.
struct ScratchUse {
    SharedScratch &scratch;
    hipStream_t s;
    bool held = false;
    int acquire(size_t need, size_t bytes)
    {
        RPH_TRY(scratch.acquire(s, need, bytes));
        held = true;
        return RPH_OK;
    }
    int done()
    {
        held = false;
        return scratch.publish(s);
    }
    ~ScratchUse()
    {
        if (held) (void)scratch.publish(s);
    }
};

// Declared behind the host variables that asynchronous copies write and the buffers that kernels in flight use: on every way out of the
// scope, an error's included, the stream is through with them before they go.  On the ordinary way out the stream is already idle.
struct StreamDrain {
    hipStream_t s;
    ~StreamDrain() { (void)hipStreamSynchronize(s); }
};

// Host threads when the caller does not say: what this process may actually use (its affinity mask, and the cgroup CPU quota a
// container runs under -- hardware_concurrency() reports the machine's 256 threads inside a 16-CPU container); rph_api.cpp
unsigned rph_host_threads();

// body(i) for every i in [first, last) on up to `threads` threads (the caller's one among them)
template <class F>
void parallel_for(size_t first, size_t last, unsigned threads, F &&body)
{
    std::atomic<size_t> next{first};
    auto work = [&]() {
        for (;;) {
            const size_t i = next.fetch_add(1);
            if (i >= last) return;
            body(i);
        }
    };
    const unsigned nt = (unsigned)std::min<size_t>(std::max(1u, threads), last > first ? last - first : 1);
    if (nt <= 1) {
        work();
        return;
    }
    std::vector<std::thread> th;
    for (unsigned t = 0; t + 1 < nt; t++) th.emplace_back(work);
    work();
    for (auto &t : th) t.join();
}
