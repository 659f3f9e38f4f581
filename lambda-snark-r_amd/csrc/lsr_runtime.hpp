// Host runtime shared by the C-ABI translation units: error reporting, device guards, contexts.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "lsr_arith.hpp"
#include "lsr_host_math.hpp"

namespace lsr {

void set_last_error(const std::string& msg);
const char* last_error_cstr();

struct HipFailure : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define LSR_HIP(expr)                                                                                         \
    do {                                                                                                      \
        hipError_t lsr_e_ = (expr);                                                                           \
        if (lsr_e_ != hipSuccess)                                                                             \
            throw ::lsr::HipFailure(std::string(#expr) + ": " + hipGetErrorString(lsr_e_));                  \
    } while (0)

// The C-ABI error boundary: runs `body`; an exception becomes -1, lsr_last_error "<where>: <what>" and a line on stderr.
template <class F>
int abi_guarded(const char* where, F&& body) noexcept {
    try {
        body();
        return 0;
    } catch (const std::exception& e) {
        set_last_error(std::string(where) + ": " + e.what());
        std::fprintf(stderr, "lambda_snark_core: %s failed: %s\n", where, e.what());
        return -1;
    } catch (...) {
        set_last_error(std::string(where) + ": unknown exception");
        return -1;
    }
}

// An argument refusal at the C-ABI: -1 and lsr_last_error "<where>: <why>" (nothing on stderr).
inline int abi_refuse(const char* where, const std::string& why) {
    set_last_error(std::string(where) + ": " + why);
    return -1;
}

// Device selection that does not leak into the caller's thread state (Rust wrappers are Send, not
// Sync: the calling thread may change between calls — SURVEY.md §8(b) "Threading").
class DeviceGuard {
public:
    explicit DeviceGuard(int device);
    ~DeviceGuard();
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;

private:
    int previous_ = -1;
    bool switched_ = false;
};

int default_device();          // LAMBDA_SNARK_DEVICE, else LOCAL_RANK, else 0; -1 (+ message) when that index is not a visible device
int visible_device_count();    // 0 if the runtime cannot see a GPU
// the device a handle is created on: `device`, or default_device() for a negative one; -1 (+ lsr_last_error "<where>: ...") when
// there is none.  announce: also say on stderr that no device is visible
int resolve_device(const char* where, int device, bool announce);

// The owners below release what they hold in their destructors (which never throw) and cannot be copied.  A buffer's `count` is the
// only record of its capacity: ptr != nullptr <=> count > 0, also after a failed allocation (the buffer is then empty).
template <class T>
struct DeviceBuffer {
    T* ptr = nullptr;
    size_t count = 0;
    DeviceBuffer() = default;
    explicit DeviceBuffer(size_t n) { allocate(n); }
    ~DeviceBuffer() { release(); }
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    void allocate(size_t n) {
        release();
        if (!n) return;
        void* p = nullptr;
        LSR_HIP(hipMalloc(&p, n * sizeof(T)));
        ptr = static_cast<T*>(p);
        count = n;
    }
    void reserve(size_t n) {   // grows only
        if (count < n) allocate(n);
    }
    void release() noexcept {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        count = 0;
    }
    void upload(const std::vector<T>& host) {
        allocate(host.size());
        if (!host.empty()) LSR_HIP(hipMemcpy(ptr, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice));
    }
    void wipe() noexcept {     // zeroes the contents (a secret); synchronous on the null stream
        if (ptr) (void)hipMemset(ptr, 0, count * sizeof(T));
    }
};

// page-locked host memory; flags: hipHostMallocPortable (any device of the node may DMA into it) or hipHostMallocDefault
template <class T>
struct PinnedBuffer {
    T* ptr = nullptr;
    size_t count = 0;
    explicit PinnedBuffer(unsigned flags) : flags_(flags) {}
    ~PinnedBuffer() { release(); }
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    void allocate(size_t n) {
        release();
        if (!n) return;
        void* p = nullptr;
        LSR_HIP(hipHostMalloc(&p, n * sizeof(T), flags_));
        ptr = static_cast<T*>(p);
        count = n;
    }
    void reserve(size_t n) {   // grows only
        if (count < n) allocate(n);
    }
    void release() noexcept {
        if (ptr) (void)hipHostFree(ptr);
        ptr = nullptr;
        count = 0;
    }
    void wipe() noexcept {     // zeroes the contents (a secret)
        volatile T* v = ptr;
        for (size_t i = 0; i < count; ++i) v[i] = 0;
    }

private:
    unsigned flags_;
};

// An event without timing, created by its first record(); sync() and wait() do nothing before that.
class Event {
public:
    Event() = default;
    ~Event() {
        if (ev_) (void)hipEventDestroy(ev_);
    }
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    void record(hipStream_t s) {
        if (!ev_) LSR_HIP(hipEventCreateWithFlags(&ev_, hipEventDisableTiming));
        LSR_HIP(hipEventRecord(ev_, s));
    }
    void sync() const {        // the host waits for the last record
        if (ev_) LSR_HIP(hipEventSynchronize(ev_));
    }
    void wait(hipStream_t s) const {   // `s` waits for the last record
        if (ev_) LSR_HIP(hipStreamWaitEvent(s, ev_, 0));
    }

private:
    hipEvent_t ev_ = nullptr;
};

// One stream: the owner creates it into `handle` where it is needed (with the flags and priority of that place).
struct Stream {
    hipStream_t handle = nullptr;
    Stream() = default;
    ~Stream() {
        if (handle) (void)hipStreamDestroy(handle);
    }
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    operator hipStream_t() const { return handle; }
};

// the deleter of a handle owned by another handle: its destroy function
template <class T, void (*Destroy)(T*)>
struct HandleDeleter {
    void operator()(T* p) const noexcept { Destroy(p); }
};

}  // namespace lsr

// The opaque C-ABI handle (reference: struct NttContext, cpp-core/src/ntt.cpp:21-26).
struct NttContext {
    // modulus and degree stay the first two fields: the refusals of lsr_ntt_ring_challenge_batch read nothing else of a context, and
    // tests/test_ring_challenge_abi.py checks their order on a handle that holds only these
    uint64_t modulus = 0;
    uint32_t degree = 0;
    // the coefficient context of a ring handle under any modulus (lsr_ring_mod_coeff_context): no twiddle tables, so
    // the coefficient-wise calls run on it and every call that transforms refuses it first (refuse_coeff_context below)
    bool coeff = false;
    int logn = 0;
    int device = 0;
    bool use_f64 = false;
    int handoff_bytes = 8;   // bytes per residue of the private intermediate between the two passes of run_ntt (n > 4096): 8, or 6 when the
                             // FP64 flavour's hand-off words fit 48 bits (lsr_ntt.hip handoff_is_packed)
    bool gold = false;       // modulus = NTT_MODULUS (2^64 - 2^32 + 1): ArithGold kernels
    bool cyclic = false;     // cyclic twiddle tables (prover path) instead of negacyclic; psi then holds omega
    uint64_t psi = 0;
    lsr::ModParams mod{};
    // stage-order twiddles on the device; only the flavour in use is populated
    lsr::DeviceBuffer<double> fwd_f64, inv_f64;
    lsr::DeviceBuffer<lsr::ShoupOperand> fwd_u64, inv_u64;
    lsr::DeviceBuffer<uint64_t> fwd_gold, inv_gold;
    uint64_t n_inv_gold = 0, w_last_scaled_gold = 0;
    double n_inv_f64 = 0, w_last_scaled_f64 = 0;
    lsr::ShoupOperand n_inv_u64{}, w_last_scaled_u64{};
    // staging for the single-polynomial host-pointer entry points
    mutable std::mutex staging_mutex;
    mutable lsr::DeviceBuffer<uint64_t> staging;   // 3 n words
    // the context's own stream for the host-pointer entry points — created on first use (lsr::work_stream): device-API callers
    // bring their stream, and every stream a process opens competes for the runtime's few hardware queues
    mutable std::mutex stream_mutex;
    mutable lsr::Stream stream;
    // workspace of lsr_ntt_ring_mul_batch(_device) (lsr_ring_mul.hip): allocated by the first call that needs it at a size fixed by n
    // alone, never resized (a graph captured after one eager call stays valid), freed with the context.  ring_mutex serialises the
    // calls on the host; ring_event (recorded at the end of every call outside capture) orders each call behind the previous one
    // on the device, whatever streams they were issued on.
    mutable std::mutex ring_mutex;
    mutable lsr::DeviceBuffer<uint64_t> ring_scratch;
    mutable lsr::Event ring_event;
    // workspace of lsr_ntt_ring_dot_batch(_device) (lsr_ring_dot.hip), under the same rules and the same mutex and event: a buffer of
    // its own, because neither workspace is ever resized and the two calls need different sizes
    mutable lsr::DeviceBuffer<uint64_t> ring_dot_scratch;
    // n > 4096 route of lsr_ntt_ring_matvec_batch(_device) (lsr_ring_matvec.hip): one dense chunk of ring_dot outputs on its way to
    // the strided rows of y.  Allocated by the first lsr_ntt_ring_matrix_create(_device) on the context at a size fixed by n alone,
    // never resized.  ring_matvec_mutex is held for a whole call (taken before ring_mutex, never the other way round); the call
    // records ring_event after its last copy out of the buffer, so the next ring call starts behind it.
    mutable std::mutex ring_matvec_mutex;
    mutable lsr::DeviceBuffer<uint64_t> ring_matvec_scratch;
    // the cosine table of the fixed-point operator norm (lsr_ring_challenge.hip, n <= 4096): 2 n words, built on the host and uploaded
    // by lsr_ntt_ring_opnorm_prepare or by the first call that needs it, never resized, freed with the context
    mutable std::mutex opnorm_mutex;
    mutable lsr::DeviceBuffer<int32_t> opnorm_table;
};

namespace lsr {

// q, 2 q, the doubles and floor(2^128 / q) for any q >= 2, prime or not (mulmod_barrett128 and mod64_barrett use nothing else of q)
inline ModParams make_mod_params(uint64_t q, int logn) {
    ModParams p{};
    p.q = q;
    p.two_q = 2 * q;
    p.qd = static_cast<double>(q);
    p.inv_qd = 1.0 / p.qd;
    u128 ratio = ~static_cast<u128>(0) / q;             // floor((2^128 - 1) / q): one short of floor(2^128 / q) exactly when q | 2^128
    if ((q & (q - 1)) == 0) ratio += 1;
    p.barrett_hi = static_cast<uint64_t>(ratio >> 64);
    p.barrett_lo = static_cast<uint64_t>(ratio);
    p.logn = logn;
    return p;
}

NttContext* create_ntt_context(uint64_t q, uint32_t n, int device);
// the negacyclic context of (q, n) without twiddle tables that a ring handle lends out (lsr_ring_mod_coeff_context): any q >= 2 and any
// n = 2^logn the handle admits; psi = 0, the 8-byte hand-off, the flavour of lsr_set_arith_mode.  `where` names the entry point
NttContext* create_coeff_context(const char* where, uint64_t q, uint32_t n, int logn, int device);
// The refusal every entry point that transforms makes first after its context's own NULL check: true, with lsr_last_error "<where>:
// ... coefficient context ...", when ctx is a coefficient context.  An entry lsr_ntt_ring_X whose product the handle computes itself
// is pointed to lsr_ring_mod_X.
inline bool refuse_coeff_context(const char* where, const NttContext* ctx) {
    if (!ctx || !ctx->coeff) return false;
    static const char* const kOnHandle[] = {"mul_batch", "dot_batch", "dot_galois_batch", "fold_batch", "gram_batch", "gram_sym2_batch",
                                            "matrix_create", "matrix_create_seeded"};
    const std::string name(where), prefix("lsr_ntt_ring_"), device("_device");
    std::string instead;
    if (name.compare(0, prefix.size(), prefix) == 0) {
        std::string rest = name.substr(prefix.size());
        const bool dev = rest.size() > device.size() && rest.compare(rest.size() - device.size(), device.size(), device) == 0;
        if (dev) rest.resize(rest.size() - device.size());
        for (const char* k : kOnHandle)
            if (rest == k) instead = std::string(": use lsr_ring_mod_") + rest + (dev ? "_device" : "") + " on the handle";
    }
    set_last_error(name + ": the context is the coefficient context of a ring handle (lsr_ring_mod_coeff_context), which has no twiddle tables and "
                          "serves the coefficient-wise calls only" + instead);
    return true;
}
// cyclic transform over F_q with the given primitive n-th root (0 = the reference's root for NTT_MODULUS)
// large: the ceiling is 2^22 instead of 2^17 (lsr_cyclic_ntt_context_create_large; above 2^17 only q = NTT_MODULUS); `where` names
// the entry point in lsr_last_error
NttContext* create_cyclic_ntt_context(uint64_t q, uint32_t n, uint64_t omega, int device, bool large = false,
                                      const char* where = "lsr_cyclic_ntt_context_create");
void destroy_ntt_context(NttContext* ctx);
using NttContextPtr = std::unique_ptr<NttContext, HandleDeleter<NttContext, destroy_ntt_context>>;
hipStream_t work_stream(const NttContext& ctx);
// asynchronous launches on `stream`, data resident on ctx->device
// add_on_inverse (optional): canonical residues [batch][n] added to the outputs of an inverse transform in its final
// store (the commitment's fused blinding add)
// pre_mul_on_inverse (optional, NTT_MODULUS contexts): residues [n] in Montgomery form (prover_montgomery); input word i of
// every polynomial of an inverse transform is multiplied by entry i as it is read
// forward_source (optional): a forward transform reads its operands from there ([batch][n], canonical) and writes d_data
void launch_ntt(const NttContext& ctx, uint64_t* d_data, size_t batch, bool inverse, hipStream_t stream,
                const uint64_t* add_on_inverse = nullptr, const uint64_t* pre_mul_on_inverse = nullptr,
                const uint64_t* forward_source = nullptr);
// only the strided top-bits round of an n > 4096 FP64-flavour transform: forward reads canonical `src`, writes raw elements
// to `dst` (may alias); inverse turns raw elements into canonical residues (+ optional canonical `add`), in place
// forward transform (Goldilocks, n <= 4096) with elementwise work fused into the read-in: mode 1 = multiply by x1 first (src may be
// NULL = in place), mode 2 = test x1 * x2 == operand and mark failing instances in bad[index >> log n]
bool ntt_forward_can_fuse(const NttContext& ctx);
void launch_ntt_forward_fused(const NttContext& ctx, uint64_t* d_data, size_t batch, hipStream_t stream, const uint64_t* src, int mode, const uint64_t* x1,
                              const uint64_t* x2, uint32_t* bad);
// true while `stream` records into a HIP graph: events recorded there belong to the capture (they cannot be waited for on the
// host), so the per-object ordering brackets stand aside — a captured call sequence is ordered by the capture itself, and the
// caller orders graph launches against other work on the same object
bool stream_is_capturing(hipStream_t stream);
// `words` 64-bit words at `dst` set to zero by a KERNEL on `stream` (device-API paths that may be captured into a HIP graph: a
// captured hipMemsetAsync cleared the verdict state on the first replay only — tools/graph_probe.py, profiles/README.md)
void zero_words_async(uint64_t* dst, size_t words, hipStream_t stream);
void launch_ntt_forward_finish(const NttContext& ctx, const uint64_t* d_data, size_t batch, hipStream_t stream, const uint64_t* x1,
                               const uint64_t* chat, const uint64_t* untwist, uint64_t half_m_inv, uint64_t* quotient, uint32_t* top);
void launch_top_round_forward(const NttContext& ctx, uint64_t* d_dst, const uint64_t* d_src, size_t polys, hipStream_t stream);
void launch_top_round_inverse(const NttContext& ctx, uint64_t* d_data, size_t polys, hipStream_t stream, const uint64_t* add);
// the same round with the added residues sampled in the pass (CDT Gaussian per polynomial, lsr_sampler.hpp) instead of read
struct BlindSampler;
void launch_top_round_inverse_sampled(const NttContext& ctx, uint64_t* d_data, size_t polys, hipStream_t stream, const BlindSampler& sampler);
// split sampling (sampler.side != NULL in both calls): the forward round of a chunk also samples the first half of the rows of the
// residues its inverse round will add, into sampler.side ([polys][n / 2^r][2^r / 16] words, int8 per sample)
void launch_top_round_forward_sampling(const NttContext& ctx, uint64_t* d_dst, const uint64_t* d_src, size_t polys, hipStream_t stream,
                                       const BlindSampler& sampler);
// the strided top-bits round of an n > 4096 transform in the context's flavour: forward reads canonical `src`, writes raw elements
// to `d` (may alias); inverse turns raw elements into canonical residues, in place
void launch_strided_round(const NttContext& ctx, uint64_t* d, const uint64_t* src, size_t polys, bool inverse, hipStream_t stream);
// bytes of one chunk of a two-pass transform: the array written by one pass stays in the Infinity Cache for the next
size_t ntt_chunk_bytes();
void launch_pointwise(const NttContext& ctx, uint64_t* d_out, const uint64_t* d_a, const uint64_t* d_b, size_t count,
                      hipStream_t stream);
// out[b][i] = in[b][bitrev_logn(i)] (out != in)
void launch_bit_reverse(uint64_t* d_out, const uint64_t* d_in, int logn, size_t batch, hipStream_t stream);
int arith_mode();

}  // namespace lsr
