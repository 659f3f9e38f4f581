// The host call path shared by the ring operations (lsr_ring_mul.hip, lsr_ring_dot.hip, lsr_ring_fold.hip, lsr_ring_matvec.hip,
// lsr_ring_gadget.hip, lsr_ring_galois.hip, lsr_ring_sample.hip, lsr_ring_challenge.hip, lsr_ring_pack.hip, lsr_ring_norm.hip,
// lsr_ring_scalar.hip, lsr_ring_gram.hip, lsr_ring_quadform.hip, and the ring combination of lsr_commit.hip; the operations on a ring
// handle under any modulus reach it through lsr_ring_mod_call.hpp, which holds the handle's own bracket): the dispatch from a context to a kernel instantiation, the
// bracket that keeps the context's workspaces safe across streams and threads, the argument checks the entry points
// have in common and the one loop that stages host buffers through bounded device chunks (host_staged; its arithmetic:
// lsr_staging_plan.hpp).  The dispatch helpers (for_tile_log, for_rank, for_top_bits, for_bool, for_flavour) also serve the commitment
// pipelines of lsr_commit.hip.  Host code only.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <initializer_list>
#include <stdexcept>
#include <type_traits>

#include "lsr_ntt_kernels.hpp"
#include "lsr_runtime.hpp"
#include "lsr_staging_plan.hpp"

namespace lsr {

// f(std::integral_constant<int, LT>{}) for LT = lt in [LO, HI]; any other lt goes to HI.  <1, 12>: every tile size; <9, 12>: the
// middle pass of a two-pass transform (mid_tile_log).
template <int LO, int HI, class F>
void for_tile_log(int lt, F&& f) {
    if constexpr (LO < HI) {
        if (lt == LO) f(std::integral_constant<int, LO>{});
        else for_tile_log<LO + 1, HI>(lt, f);
    } else {
        f(std::integral_constant<int, HI>{});
    }
}

// f(std::integral_constant<int, K>{}) for the module rank K = k in 1 .. 4; any other k goes to 4 (a caller with a generic form for
// larger ranks takes it first)
template <class F>
void for_rank(uint32_t k, F&& f) {
    for_tile_log<1, 4>(static_cast<int>(k), f);
}

// f(std::integral_constant<int, R>{}) for the R = 4 (n = 2^16) or 5 (n = 2^17) index bits of a top round
template <class F>
void for_top_bits(int r, F&& f) {
    if (r == 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 5>{});
}

// f(std::true_type{}) or f(std::false_type{}): a run-time switch as a template argument
template <class F>
void for_bool(bool on, F&& f) {
    if (on) f(std::true_type{});
    else f(std::false_type{});
}

// f(A{}) for the arithmetic flavour A of the context's kernels
template <class F>
decltype(auto) for_flavour(const NttContext& c, F&& f) {
    if (c.gold) return f(ArithGold{});
    if (c.use_f64) return f(ArithF64{});
    return f(ArithU64{});
}

// n > 4096: the tile size of the middle pass, the low log n - 4 (n = 2^17: - 5) bits of a two-pass transform
inline int mid_tile_log(const NttContext& c) { return c.logn - std::max(c.logn - kTileLog, 4); }

// what a capturing call says when the workspace it needs was never allocated (also the Gram workspace of a ring handle, lsr_ring_mod_call.hpp)
constexpr const char* kWorkspaceBeforeCapture =
    "this call needs the context's workspace, which the first such call allocates: make one eager (uncaptured) "
    "call on this context before capturing";

// The bracket of one ring call on the device (caller validated the arguments): under ring_mutex, `workspace` allocated at
// `workspace_words` by the first call that needs it, the launches of `enqueue` on `s` behind the context's previous ring call, and
// ring_event recorded behind them for the next one.  A capturing stream: no brackets (lsr_runtime.hpp, stream_is_capturing).
template <class Enqueue>
void ring_call(const NttContext& c, DeviceBuffer<uint64_t>& workspace, size_t workspace_words, bool needs_workspace, hipStream_t s,
               Enqueue&& enqueue) {
    std::lock_guard<std::mutex> lock(c.ring_mutex);
    const bool capturing = stream_is_capturing(s);
    if (needs_workspace && !workspace.ptr) {
        // the workspace is allocated once and never resized, so a graph captured after one eager call keeps valid pointers; an
        // allocation inside the capture would not be part of the graph
        if (capturing)
            throw std::runtime_error(kWorkspaceBeforeCapture);
        workspace.allocate(workspace_words);
    }
    if (!capturing) c.ring_event.wait(s);
    enqueue();
    LSR_HIP(hipGetLastError());
    if (!capturing) c.ring_event.record(s);
}

inline void require_device() {
    if (visible_device_count() <= 0) throw std::runtime_error("no HIP device visible — this library has no CPU fallback");
}

// [out, out + out_bytes) and [in, in + in_bytes) share memory
inline bool ranges_overlap(const void* out, size_t out_bytes, const void* in, size_t in_bytes) {
    const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + out_bytes;
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), i1 = i0 + in_bytes;
    return o0 < i1 && i0 < o1;
}
// `message` when they do
inline void require_apart(const void* out, size_t out_bytes, const void* in, size_t in_bytes, const char* message) {
    if (ranges_overlap(out, out_bytes, in, in_bytes)) throw std::runtime_error(message);
}

// the middle pass of a fused ring operation assumes ONE strided round on either side
inline void refuse_above_two_pass(const NttContext& c, const char* message) {
    if (c.logn > kTwoPassMaxLog2) throw std::runtime_error(message);
}

// bytes of device memory one host-pointer call stages at a time: LAMBDA_SNARK_STAGING_MIB (a positive integer, read once per
// process; a test and tuning knob as LAMBDA_SNARK_NTT_CHUNK_MIB is), 256 MiB when unset or unparsable
inline size_t staging_bytes() {
    static const size_t bytes = [] {
        if (const char* e = std::getenv("LAMBDA_SNARK_STAGING_MIB")) {
            const long v = std::atol(e);
            if (v > 0) return static_cast<size_t>(v) << 20;
        }
        return static_cast<size_t>(256) << 20;
    }();
    return bytes;
}

// the items of a call that fit the staging bound at `words_per_item` staged words each: at least 1, at most `count`
inline size_t staging_chunk(size_t count, size_t words_per_item) {
    return std::max<size_t>(1, std::min<size_t>(count, (staging_bytes() / 8) / words_per_item));
}

// what `run` sees of one chunk: items [first, first + now) of the call, the device buffer of each lane in the order the lanes were
// declared (an absent lane: NULL), and group_first, the group the group lanes' buffers start at
constexpr size_t kStagedMaxLanes = 5;
struct StagedChunk {
    size_t first, now, group_first;
    void* buffer[kStagedMaxLanes];
    template <class T>
    T* lane(size_t i) const { return static_cast<T*>(buffer[i]); }
};

// The host buffers of a call of `count` items through bounded device chunks of `chunk` items on the context's work stream (DESIGN.md
// §5c; the lanes and their arithmetic: lsr_staging_plan.hpp).  Per chunk, in stream order: the uploads, `run(chunk, s)`, which
// enqueues the device work of the chunk's items and nothing else, the downloads, one synchronisation.  The group lanes of a call
// share one `components`.
template <class Run>
void host_staged(const NttContext& c, size_t count, size_t chunk, std::initializer_list<StagedLane> lanes, Run&& run) {
    if (lanes.size() > kStagedMaxLanes) throw std::logic_error("host_staged: more lanes than kStagedMaxLanes");
    DeviceGuard guard(c.device);
    DeviceBuffer<unsigned char> device[kStagedMaxLanes];
    StagedChunk k{};
    size_t components = 0;
    for (size_t i = 0; i < lanes.size(); ++i) {
        const StagedLane& l = lanes.begin()[i];
        device[i].allocate(staged_allocation(l, count, chunk));
        k.buffer[i] = device[i].ptr;
        if (l.components) components = l.components;
    }
    std::lock_guard<std::mutex> lock(c.staging_mutex);   // serialises use of work_stream(c)
    hipStream_t s = work_stream(c);
    for (k.first = 0; k.first < count; k.first += chunk) {
        k.now = std::min(chunk, count - k.first);
        k.group_first = components ? staged_group_first(k.first, components) : 0;
        for (size_t i = 0; i < lanes.size(); ++i) {
            const StagedLane& l = lanes.begin()[i];
            const StagedCopy copy = staged_copy(l, k.first, k.now);
            if (staged_uploads(l, k.first))
                LSR_HIP(hipMemcpyAsync(device[i].ptr, static_cast<const unsigned char*>(l.up) + copy.host_offset, copy.bytes, hipMemcpyHostToDevice, s));
        }
        run(k, s);
        for (size_t i = 0; i < lanes.size(); ++i) {
            const StagedLane& l = lanes.begin()[i];
            const StagedCopy copy = staged_copy(l, k.first, k.now);
            if (l.down && l.extent != 0)
                LSR_HIP(hipMemcpyAsync(static_cast<unsigned char*>(l.down) + copy.host_offset, device[i].ptr, copy.bytes, hipMemcpyDeviceToHost, s));
        }
        LSR_HIP(hipStreamSynchronize(s));
    }
}

// one operand up, one result down: `in_words` words go up and `out_words` words come back per item, `run(d_out, d_in, now, s)`
// enqueues the work of `now` items
template <class Run>
void host_staged(const NttContext& c, uint64_t* out, const uint64_t* in, size_t count, size_t out_words, size_t in_words, Run&& run) {
    host_staged(c, count, staging_chunk(count, in_words + out_words), {staged_items(in, nullptr, in_words * 8), staged_items(nullptr, out, out_words * 8)},
                [&](const StagedChunk& k, hipStream_t s) { run(k.lane<uint64_t>(1), k.lane<const uint64_t>(0), k.now, s); });
}

// The host buffers of a ring inner product c_j = sum_i f(a_{j,i}) b_{j,i} ([batch][terms][n] against [b_rows][terms][n]) through
// bounded device chunks on the context's work stream: whole outputs while one output's terms fit the staging bound, else one output
// at a time with its terms in groups (the accumulator stays on the device between groups).
// `run(d_c, d_a, d_b, now, group, b_rows, s, first, last)` enqueues the device call of `now` outputs over `group` terms; first / last:
// the group starts / finishes the sums.
template <class Run>
void host_staged_dot(const NttContext& c, uint64_t* out, const uint64_t* a, const uint64_t* b, size_t batch, size_t terms, size_t b_rows, Run&& run) {
    DeviceGuard guard(c.device);
    const size_t n = c.degree;
    const bool shared_b = b_rows == 1 && batch > 1;
    const size_t bound = std::max<size_t>(1, staging_bytes() / (n * 8));          // polynomials per staged operand
    const size_t group_max = std::min(terms, bound), chunk = group_max == terms ? std::max<size_t>(1, std::min(batch, bound / terms)) : 1;
    DeviceBuffer<uint64_t> da(chunk * group_max * n), db((shared_b ? 1 : chunk) * group_max * n), dc(chunk * n);
    std::lock_guard<std::mutex> lock(c.staging_mutex);   // serialises use of work_stream(c)
    hipStream_t s = work_stream(c);
    for (size_t j0 = 0; j0 < batch; j0 += chunk) {
        const size_t now = std::min(chunk, batch - j0);
        for (size_t i0 = 0; i0 < terms; i0 += group_max) {
            const size_t group = std::min(group_max, terms - i0), off = (j0 * terms + i0) * n;
            LSR_HIP(hipMemcpyAsync(da.ptr, a + off, now * group * n * 8, hipMemcpyHostToDevice, s));
            if (!shared_b) LSR_HIP(hipMemcpyAsync(db.ptr, b + off, now * group * n * 8, hipMemcpyHostToDevice, s));
            else if (j0 == 0 || group != terms) LSR_HIP(hipMemcpyAsync(db.ptr, b + i0 * n, group * n * 8, hipMemcpyHostToDevice, s));
            run(dc.ptr, da.ptr, db.ptr, now, group, shared_b ? 1 : now, s, i0 == 0, i0 + group == terms);
        }
        LSR_HIP(hipMemcpyAsync(out + j0 * n, dc.ptr, now * n * 8, hipMemcpyDeviceToHost, s));
        LSR_HIP(hipStreamSynchronize(s));
    }
}

}  // namespace lsr
