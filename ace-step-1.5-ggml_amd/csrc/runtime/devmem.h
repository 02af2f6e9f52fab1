// Device memory of the runtime, and the one table built on it.  Four owners, each freeing what it holds in its
// destructor (none may have static storage duration: a hipFree after the HIP runtime has shut down must stay
// impossible):
//   DevBuf     a workspace that only grows (engines, ABI staging);
//   DevMem     a fixed-size allocation for one scope (self-tests, the generate entry's staging);
//   DevArena   every allocation of a loaded model, freed together;
//   RopeTable  the NEOX cos / sin table every engine reads, on two DevBufs.
// Only hipMalloc / hipFree / hipMemset / hipMemcpy / hipDeviceSynchronize / hipStreamSynchronize are called here.
#pragma once

#include <cmath>
#include <utility>
#include <vector>

#include "../common.h"

namespace acemi {

// A device allocation that only grows; moved, not copied.
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;  // allocated (rounded up to 256)
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), bytes(std::exchange(o.bytes, 0)) {}
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            bytes = std::exchange(o.bytes, 0);
        }
        return *this;
    }
    ~DevBuf() { release(); }
    void release() noexcept {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    // At least `need` bytes (0 counts as 16).  Growing drops the contents: the new allocation is zero-filled.
    void ensure(size_t need) {
        if (need == 0) need = 16;
        if (bytes >= need) return;
        if (p) {
            ACEMI_HIP(hipDeviceSynchronize());
            ACEMI_HIP(hipFree(p));
            p = nullptr;
            bytes = 0;
        }
        const size_t alloc = (need + 255) & ~size_t(255);
        ACEMI_HIP(hipMalloc(&p, alloc));
        ACEMI_HIP(hipMemset(p, 0, alloc));
        // hipMemset runs on the legacy null stream, which does not order against the library's
        // non-blocking streams: finish it before any kernel can write the new buffer
        ACEMI_HIP(hipDeviceSynchronize());
        bytes = alloc;
    }
    template <typename T>
    T* as() const {
        return static_cast<T*>(p);
    }
};
inline void ensure(DevBuf& b, size_t bytes) { b.ensure(bytes); }

// A device allocation of fixed size (at least 16 bytes) for one scope, filled from `host` when that is not null.
struct DevMem {
    void* p = nullptr;
    explicit DevMem(size_t bytes) { ACEMI_HIP(hipMalloc(&p, bytes < 16 ? 16 : bytes)); }
    DevMem(const void* host, size_t bytes) : DevMem(bytes) {
        if (host && bytes) {
            const hipError_t e = hipMemcpy(p, host, bytes, hipMemcpyHostToDevice);
            if (e != hipSuccess) {  // no destructor runs for a constructor that throws
                (void)hipFree(p);
                ACEMI_HIP(e);
            }
        }
    }
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() {
        if (p) (void)hipFree(p);
    }
    template <typename T>
    T* as() const {
        return static_cast<T*>(p);
    }
    void to_host(void* host, size_t bytes) const { ACEMI_HIP(hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost)); }
};

// The device allocations of a loaded model.
class DevArena {
   public:
    DevArena() = default;
    DevArena(const DevArena&) = delete;
    DevArena& operator=(const DevArena&) = delete;
    ~DevArena() {
        for (const Item& a : items_) (void)hipFree(a.p);
    }
    void* alloc(size_t bytes) {
        void* d = nullptr;
        ACEMI_HIP(hipMalloc(&d, bytes));
        items_.push_back(Item{d, bytes});
        bytes_ += bytes;
        return d;
    }
    template <typename T>
    T* upload(const void* host, size_t bytes) {
        void* d = alloc(bytes);
        ACEMI_HIP(hipMemcpy(d, host, bytes, hipMemcpyHostToDevice));
        ACEMI_HIP(hipDeviceSynchronize());  // null-stream copy: done before any stream reads it
        return static_cast<T*>(d);
    }
    // Frees the allocation made before the last one; the last one takes its place (a loader that replaces an
    // upload by an image computed from it).
    void drop_before_last() {
        ACEMI_CHECK(items_.size() >= 2, "arena: nothing to replace");
        Item& old = items_[items_.size() - 2];
        (void)hipFree(old.p);
        bytes_ -= old.bytes;
        old = items_.back();
        items_.pop_back();
    }
    size_t bytes() const { return bytes_; }

   private:
    struct Item {
        void* p;
        size_t bytes;
    };
    std::vector<Item> items_;
    size_t bytes_ = 0;
};

// NEOX RoPE table with the reference's own float arithmetic: ggml_rope_cache_init runs
// theta = p; theta *= theta_scale per pair, theta_scale = powf(base, -2/n_dims), cos/sinf on the CPU
// (acestep_dit_model.cpp:1205-1210).  Computed on the host, rows [n][head_dim / 2] of cos and of sin.
class RopeTable {
   public:
    // Positions 0..n-1.  Row p does not depend on n, so a longer table is a valid prefix for every shorter request:
    // rebuilt only when n exceeds the rows held, or head_dim or theta changed.
    void ensure(int n, int head_dim, float rope_theta, hipStream_t s) {
        if (n <= n_ && head_dim == head_dim_ && rope_theta == theta_) return;
        const int half = head_dim / 2;
        const float theta_scale = powf(rope_theta, -2.0f / (float)head_dim);
        std::vector<float> cs((size_t)n * half), sn((size_t)n * half);
        for (int p = 0; p < n; ++p) {
            float theta = (float)p;
            for (int i = 0; i < half; ++i) {
                cs[(size_t)p * half + i] = (float)std::cos((double)theta);  // correctly rounded cosf / sinf
                sn[(size_t)p * half + i] = (float)std::sin((double)theta);
                theta *= theta_scale;
            }
        }
        // a forward still queued on `s` (a non-blocking stream) may read the old table: drain it first
        ACEMI_HIP(hipStreamSynchronize(s));
        n_ = 0;
        cos_.ensure(cs.size() * 4);
        sin_.ensure(sn.size() * 4);
        ACEMI_HIP(hipMemcpy(cos_.p, cs.data(), cs.size() * 4, hipMemcpyHostToDevice));
        ACEMI_HIP(hipMemcpy(sin_.p, sn.data(), sn.size() * 4, hipMemcpyHostToDevice));
        ACEMI_HIP(hipDeviceSynchronize());  // null-stream copy: done before any stream reads it
        n_ = n;
        head_dim_ = head_dim;
        theta_ = rope_theta;
    }
    const float* cos() const { return cos_.as<float>(); }
    const float* sin() const { return sin_.as<float>(); }
    int rows() const { return n_; }

   private:
    DevBuf cos_, sin_;
    int n_ = 0, head_dim_ = 0;
    float theta_ = 0.f;
};

}  // namespace acemi
