/*
 * device_buffer.h -- the one owner of device memory (DESIGN "Who owns device memory"). Host C++ only: the HIP runtime API and the
 * standard library, nothing of the kernels.
 *
 * A DevBuf frees what it holds when it goes away, so a struct of buffers needs no list of them. It knows nothing about growth: every
 * caller sizes its own allocation (ensure, ensure_keep, the stream slots) and calls alloc with the result.
 * No DevBuf may have static storage duration: its destructor would run after the HIP runtime has shut down.
 */
#pragma once

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstddef>
#include <cstdint>

/* buffers and bytes held by all DevBufs of the process (paffy_hip_device_buffers) */
inline std::atomic<int64_t> devbuf_held_buffers{0}, devbuf_held_bytes{0};

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;

    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) {
        o.p = nullptr;
        o.cap = 0;
    }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) {
            (void)release();
            p = o.p;
            cap = o.cap;
            o.p = nullptr;
            o.cap = 0;
        }
        return *this;
    }
    ~DevBuf() { (void)release(); }

    /* frees what the buffer holds; the buffer is empty afterwards whatever hipFree answered */
    hipError_t release() {
        hipError_t e = hipSuccess;
        if (p) {
            e = hipFree(p);
            devbuf_held_buffers.fetch_sub(1, std::memory_order_relaxed);
            devbuf_held_bytes.fetch_sub((int64_t)cap, std::memory_order_relaxed);
        }
        p = nullptr;
        cap = 0;
        return e;
    }
    /* exactly `bytes`, after releasing what was held; on failure the buffer is empty */
    hipError_t alloc(size_t bytes) {
        hipError_t e = release();
        if (e != hipSuccess) return e;
        e = hipMalloc(&p, bytes);
        if (e != hipSuccess || !p) {
            p = nullptr;
            return e;
        }
        cap = bytes;
        devbuf_held_buffers.fetch_add(1, std::memory_order_relaxed);
        devbuf_held_bytes.fetch_add((int64_t)cap, std::memory_order_relaxed);
        return hipSuccess;
    }
};
