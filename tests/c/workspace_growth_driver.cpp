// A workspace growth that the runtime refuses leaves an owner that no later call can mistake for a larger one: the buffer is
// empty (or untouched) and the layout size of the R1CS scratch does not advance, so a following small request allocates again
// instead of passing a stale gate.  2^50 bytes are refused at once by every device and by the runtime without one.  Nothing here
// launches a kernel.  Built by tests/test_workspace_growth.py and linked against the library; prints "ok".
#include <cstdio>
#include <cstdlib>

#include "lsr_prove_common.hpp"

#define CHECK(cond)                                                           \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                     \
        }                                                                     \
    } while (0)

static constexpr size_t kHugeBytes = size_t(1) << 50;

template <class F>
static bool throws(F&& f) {
    try {
        f();
    } catch (const lsr::HipFailure&) {
        return true;
    }
    return false;
}

// p lies inside a live device allocation
static bool live(const void* p) {
    hipPointerAttribute_t attr{};
    const bool ok = hipPointerGetAttributes(&attr, p) == hipSuccess && attr.type == hipMemoryTypeDevice;
    (void)hipGetLastError();
    return ok;
}

int main() {
    const bool gpu = lsr::visible_device_count() > 0;
    if (gpu) CHECK(hipSetDevice(0) == hipSuccess);

    // DeviceBuffer::reserve
    lsr::DeviceBuffer<uint64_t> b;
    if (gpu) {
        b.reserve(1024);
        CHECK(b.ptr && b.count == 1024 && live(b.ptr));
    }
    uint64_t* const old_ptr = b.ptr;
    const size_t old_count = b.count;
    CHECK(throws([&] { b.reserve(kHugeBytes / sizeof(uint64_t)); }));
    CHECK((b.ptr == nullptr && b.count == 0) || (b.ptr == old_ptr && b.count == old_count));
    if (gpu) {
        b.reserve(512);
        CHECK(b.ptr && b.count >= 512 && live(b.ptr) && live(b.ptr + 511));
    }

    // R1csScratch: its chunk is the layout of `small` and `io`
    lsr::R1csScratch ws;
    if (gpu) {
        ws.grow(4, 2);
        CHECK(ws.chunk == 4 && ws.small.ptr);
        ws.stage(100);
        CHECK(ws.io.ptr && ws.io_status.ptr);
    }
    const size_t old_chunk = ws.chunk;
    CHECK(throws([&] { ws.grow(kHugeBytes / 8 / 25, 2); }));
    CHECK(ws.chunk == old_chunk);
    CHECK((ws.small.ptr == nullptr) == (ws.small.count == 0));
    if (gpu) {
        ws.grow(2, 1);
        CHECK(ws.small.ptr && ws.chunk >= 2);
        const lsr::R1csSlots v = ws.slots();
        for (const uint64_t* p : {v.keys, v.alphas, v.betas, v.hash_a, v.hash_b, v.ev, v.blinding, v.publics}) CHECK(live(p));
        CHECK(v.publics + ws.chunk * std::max<size_t>(1, ws.publics) <= ws.small.ptr + ws.small.count);
        ws.stage(100);
        CHECK(ws.io.count >= ws.chunk * (ws.row_words + 13 + 8) && ws.io_status.count >= ws.chunk && live(ws.io.ptr));
    }
    std::printf("ok (%s)\n", gpu ? "device" : "no device");
    return 0;
}
