/*
 * device_buffer_check.cpp -- paffy_amd/csrc/device_buffer.h on the host, without the HIP runtime: hipMalloc, hipFree and hipGetLastError are
 * this file's own (malloc / free with a tally; allocations above `fail_above` bytes fail), so AddressSanitizer sees every buffer the type
 * loses or frees twice. Built and run by tests/test_device_buffer_host.py:
 *   g++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I$ROCM/include -fsanitize=address,undefined -Ipaffy_amd/csrc tests/host/device_buffer_check.cpp
 * Exit status 0: every check held and nothing is left allocated.
 */
#include "device_buffer.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <type_traits>
#include <utility>
#include <vector>

static std::map<void *, size_t> live; /* the stand-in runtime's allocations */
static size_t fail_above = ~(size_t)0;
static int n_malloc = 0, n_free = 0, n_last_error = 0;
static hipError_t sticky = hipSuccess;

extern "C" hipError_t hipMalloc(void **ptr, size_t size) {
    n_malloc++;
    if (size > fail_above) {
        *ptr = reinterpret_cast<void *>(0x1); /* a failing call may leave anything behind: the type must not keep it */
        return sticky = hipErrorOutOfMemory;
    }
    *ptr = malloc(size ? size : 1);
    live[*ptr] = size;
    return hipSuccess;
}
extern "C" hipError_t hipFree(void *ptr) {
    n_free++;
    if (!ptr) return hipSuccess;
    if (!live.count(ptr)) {
        fprintf(stderr, "hipFree of %p, which is not allocated\n", ptr);
        abort();
    }
    live.erase(ptr);
    free(ptr);
    return hipSuccess;
}
extern "C" hipError_t hipGetLastError(void) {
    n_last_error++;
    const hipError_t e = sticky;
    sticky = hipSuccess;
    return e;
}

static int failures = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
            failures++;                                                      \
        }                                                                    \
    } while (0)

static size_t live_bytes() {
    size_t n = 0;
    for (const auto &kv : live) n += kv.second;
    return n;
}
/* the stand-in's tally and the library's two counters agree on `buffers` buffers of `bytes` bytes */
static bool held(size_t buffers, size_t bytes) {
    return live.size() == buffers && live_bytes() == bytes && devbuf_held_buffers.load() == (int64_t)buffers && devbuf_held_bytes.load() == (int64_t)bytes;
}

/* the library's growth policy (ensure in paffy_hip.hip), restated: free first, the size with slack, then the exact size */
static hipError_t ensure_like(DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return hipSuccess;
    hipError_t e = b.release();
    if (e != hipSuccess) return e;
    if (b.alloc(bytes + bytes / 2 + 256) != hipSuccess) {
        (void)hipGetLastError();
        return b.alloc(bytes);
    }
    return hipSuccess;
}

struct Entry { /* a kept index: a key and the buffers it owns */
    int key = 0;
    DevBuf a, b;
};

/* the stream-slot motion: the buffer goes to `kept` where that is empty, otherwise it stays with `from` and goes when that does */
static void hand_over(DevBuf &kept, DevBuf &from) {
    if (!kept.p) kept = std::move(from);
}

int main() {
    static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "DevBuf must not be copied");
    static_assert(std::is_nothrow_move_constructible<DevBuf>::value && std::is_nothrow_move_assignable<DevBuf>::value, "DevBuf must move, and a vector must use the move");

    { /* alloc, re-alloc, release */
        DevBuf b;
        CHECK(b.p == nullptr && b.cap == 0 && held(0, 0));
        CHECK(b.release() == hipSuccess && n_free == 0); /* nothing held: no call */
        CHECK(b.alloc(100) == hipSuccess && b.p && b.cap == 100 && held(1, 100));
        memset(b.p, 0x5a, b.cap);
        CHECK(b.alloc(300) == hipSuccess && b.cap == 300 && held(1, 300) && n_free == 1); /* released first */
        memset(b.p, 0x5a, b.cap);
        CHECK(b.release() == hipSuccess && b.p == nullptr && b.cap == 0 && held(0, 0));
        CHECK(b.alloc(8) == hipSuccess && held(1, 8));
    } /* the destructor */
    CHECK(held(0, 0));

    { /* move construction and move assignment: the source is empty, the target's old buffer is released */
        DevBuf a, b;
        CHECK(a.alloc(10) == hipSuccess && b.alloc(20) == hipSuccess && held(2, 30));
        void *pa = a.p;
        DevBuf c(std::move(a));
        CHECK(c.p == pa && c.cap == 10 && a.p == nullptr && a.cap == 0 && held(2, 30));
        b = std::move(c);
        CHECK(b.p == pa && b.cap == 10 && c.p == nullptr && c.cap == 0 && held(1, 10));
        DevBuf &same = b; /* self-move */
        b = std::move(same);
        CHECK(b.p == pa && b.cap == 10 && held(1, 10));
        b = DevBuf(); /* what `F.dev = {}` does to every member */
        CHECK(b.p == nullptr && held(0, 0));
    }
    CHECK(held(0, 0));

    { /* std::swap (seqload_host.h, dedupe_parts_kernel.h) */
        DevBuf a, b, empty;
        CHECK(a.alloc(16) == hipSuccess && b.alloc(32) == hipSuccess);
        void *pa = a.p, *pb = b.p;
        std::swap(a, b);
        CHECK(a.p == pb && a.cap == 32 && b.p == pa && b.cap == 16 && held(2, 48));
        std::swap(a, empty);
        CHECK(a.p == nullptr && a.cap == 0 && empty.p == pb && empty.cap == 32 && held(2, 48));
        std::swap(b, b);
        CHECK(b.p == pa && held(2, 48));
    }
    CHECK(held(0, 0));

    { /* the kept-index motion: entries move between two vectors, with an erase in between and reallocation of both */
        std::vector<Entry> kept, pool;
        for (int k = 0; k < 9; k++) {
            Entry e;
            e.key = k;
            CHECK(e.a.alloc(64 + (size_t)k) == hipSuccess && e.b.alloc(8) == hipSuccess);
            kept.push_back(std::move(e));
        }
        CHECK(held(18, 9 * 72 + 36));
        for (int key : {4, 0, 8}) { /* index_drop */
            for (size_t i = 0; i < kept.size(); i++)
                if (kept[i].key == key) {
                    pool.push_back(std::move(kept[i]));
                    kept.erase(kept.begin() + (long)i);
                    break;
                }
        }
        CHECK(kept.size() == 6 && pool.size() == 3 && held(18, 9 * 72 + 36));
        for (const Entry &e : kept) CHECK(e.a.p && e.a.cap == 64 + (size_t)e.key && e.b.cap == 8);
        { /* index_keep: one back out of the pool, grown, kept again */
            Entry e;
            e = std::move(pool.back());
            pool.pop_back();
            CHECK(e.key == 8 && e.a.cap == 72 && held(18, 9 * 72 + 36));
            e.key = 11;
            CHECK(ensure_like(e.a, 1000) == hipSuccess && e.a.cap == 1000 + 500 + 256 && ensure_like(e.b, 8) == hipSuccess && e.b.cap == 8);
            kept.push_back(std::move(e));
        }
        CHECK(kept.size() == 7 && pool.size() == 2 && held(18, 9 * 72 + 36 - 72 + 1756));
        pool.clear(); /* entries that go take their buffers along */
        CHECK(held(14, 9 * 72 + 36 - 72 + 1756 - (64 + 8) - (68 + 8)));
    }
    CHECK(held(0, 0));

    { /* the stream-slot motion: to a new owner where that has room, otherwise dropped with the old one */
        DevBuf kept[2];
        CHECK(kept[1].alloc(50) == hipSuccess);
        void *occupied = kept[1].p;
        {
            DevBuf slot_in, slot_out;
            CHECK(slot_in.alloc(40) == hipSuccess && slot_out.alloc(60) == hipSuccess && held(3, 150));
            void *pin = slot_in.p;
            hand_over(kept[0], slot_in);
            hand_over(kept[1], slot_out);
            CHECK(kept[0].p == pin && kept[0].cap == 40 && slot_in.p == nullptr && kept[1].p == occupied && slot_out.p && held(3, 150));
        }
        CHECK(held(2, 90));
        DevBuf taken = std::move(kept[0]); /* the next stream takes it again */
        CHECK(taken.cap == 40 && kept[0].p == nullptr && held(2, 90));
    }
    CHECK(held(0, 0));

    { /* a failed allocation leaves the buffer empty; the growth policy then takes the exact size */
        DevBuf b;
        CHECK(b.alloc(100) == hipSuccess);
        fail_above = 1000;
        CHECK(b.alloc(2000) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0 && held(0, 0));
        CHECK(hipGetLastError() == hipErrorOutOfMemory && hipGetLastError() == hipSuccess);
        const int calls = n_malloc, cleared = n_last_error;
        CHECK(ensure_like(b, 900) == hipSuccess && b.cap == 900 && held(1, 900)); /* 900 + 450 + 256 fails, 900 fits */
        CHECK(n_malloc == calls + 2 && n_last_error == cleared + 1 && hipGetLastError() == hipSuccess);
        CHECK(ensure_like(b, 800) == hipSuccess && b.cap == 900 && n_malloc == calls + 2); /* fits: nothing happens */
        CHECK(ensure_like(b, 1001) == hipErrorOutOfMemory && b.p == nullptr && b.cap == 0 && held(0, 0)); /* neither size fits */
        (void)hipGetLastError();
        fail_above = ~(size_t)0;
        CHECK(ensure_like(b, 1001) == hipSuccess && b.cap == 1001 + 500 + 256 && held(1, 1757));
    }
    CHECK(held(0, 0));
    CHECK(n_malloc > 0 && n_free > 0);

    if (failures) {
        fprintf(stderr, "device_buffer_check: %d check(s) failed\n", failures);
        return 1;
    }
    printf("device_buffer_check: ok (%d allocations, %d frees)\n", n_malloc, n_free);
    return 0;
}
