/*
 * lambda_snark/batch.h — ADDITIVE entry points (not in the reference): batched and device-resident
 * forms of the hot path, seeded/deterministic variants, and introspection.
 *
 * Why they exist: the reference C-ABI moves ONE polynomial through host pointers per call
 * (cpp-core/include/lambda_snark/ntt.h:55-92, commitment.h:58-63); a GPU cannot reach the headline
 * metric (batched degree-2^16 NTTs/s, commits/s) through that, so SURVEY.md §8(b) asks for batched
 * twins.  Every symbol here is `lsr_`-prefixed or `*_batch`-suffixed; the reference symbols keep their
 * exact semantics.  All are extern "C", plain pointers and sizes; `stream` is a hipStream_t passed as
 * void* (NULL = the default stream of the context's device).
 */
#pragma once

#include "lambda_snark/commitment.h"
#include "lambda_snark/ntt.h"
#include "lambda_snark/types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- runtime ---------------- */
/* number of visible HIP devices (0 when there is no GPU / no driver) */
int lsr_device_count(void) LSR_NOEXCEPT;
/* last error message of the calling thread ("" if none) */
const char* lsr_last_error(void) LSR_NOEXCEPT;
/* library / kernel-variant description, e.g. "lambda_snark_core hip gfx950 r3 (...)" */
const char* lsr_version(void) LSR_NOEXCEPT;

/* ---------------- NTT: contexts on a chosen device ---------------- */
/* like ntt_context_create, on HIP device `device` (-1 = LAMBDA_SNARK_DEVICE env, else LOCAL_RANK, else 0; an index that is
 * not a visible device is an error — NULL and a message — never wrapped around onto another rank's GPU) */
NttContext* lsr_ntt_context_create_on(uint64_t q, uint32_t n, int device) LSR_NOEXCEPT;
int      lsr_ntt_context_device(const NttContext* ctx) LSR_NOEXCEPT;
uint64_t lsr_ntt_context_root(const NttContext* ctx) LSR_NOEXCEPT;   /* psi */
/* 1 if the context computes with the exact FP64-FMA Barrett kernels (q < 2^45), 0 for u64 Shoup */
int      lsr_ntt_context_uses_f64(const NttContext* ctx) LSR_NOEXCEPT;
/* bytes per residue of the private intermediate between the two passes of an n > 4096 transform: 6 when the FP64 kernels' hand-off words
 * fit 48 bits (q < 2^47 / 4.5 for n <= 65536, q < 2^47 / 5.375 for n = 131072) and the context was not created under
 * LAMBDA_SNARK_NTT_HANDOFF=8, else 8 (also for n <= 4096, where there is no hand-off).  Results are the same words either way for
 * inputs in [0, q), which every transform entry point requires.  The library does not check them: words >= q, which the 8-byte path
 * happened to carry exactly up to 2^50, wrap at 48 bits on the 6-byte path and give wrong results without an error. */
int      lsr_ntt_handoff_bytes(const NttContext* ctx) LSR_NOEXCEPT;
/* force the arithmetic flavour of FUTURE contexts: 0 auto, 1 u64 Shoup always (testing) */
void     lsr_set_arith_mode(int mode) LSR_NOEXCEPT;

/* ---------------- NTT: batched, host buffers ([batch][n] contiguous) ---------------- */
int ntt_forward_batch(const NttContext* ctx, uint64_t* polys, size_t batch) LSR_NOEXCEPT;
int ntt_inverse_batch(const NttContext* ctx, uint64_t* polys, size_t batch) LSR_NOEXCEPT;
/* result/a/b are [batch][n]; returns 0 / -1 (unlike the void single-poly form) */
int ntt_mul_pointwise_batch(const NttContext* ctx, uint64_t* result, const uint64_t* a, const uint64_t* b,
                            size_t batch) LSR_NOEXCEPT;

/* ---------------- NTT: batched, device-resident, asynchronous on `stream` ---------------- */
int lsr_ntt_forward_batch_device(const NttContext* ctx, uint64_t* d_polys, size_t batch, void* stream) LSR_NOEXCEPT;
int lsr_ntt_inverse_batch_device(const NttContext* ctx, uint64_t* d_polys, size_t batch, void* stream) LSR_NOEXCEPT;
int lsr_ntt_mul_pointwise_device(const NttContext* ctx, uint64_t* d_result, const uint64_t* d_a,
                                 const uint64_t* d_b, size_t count, void* stream) LSR_NOEXCEPT;

/* ---------------- NTT: batched ring multiply ---------------- */
/* c_j = a_j * b_j in the ring of the context: Z_q[X]/(X^n + 1) for ntt_context_create / lsr_ntt_context_create_on contexts,
 * Z_q[X]/(X^n - 1) for lsr_cyclic_ntt_context_create contexts.  Natural coefficient order in and out, inputs in [0,q),
 * outputs canonical.  a, c: [batch][n]; b: [b_rows][n] with b_rows == batch (one b per product) or b_rows == 1 (the same b
 * for every product).  c may alias a or b exactly (partial overlap: undefined).  batch == 0: no-op, 0.  0 / -1.
 * NULL context or buffer, b_rows not in {1, batch}, no visible device: -1 and lsr_last_error, before any device work.
 * One fused pass per product at n <= 4096; four passes per chunk of the batch above.
 *
 * lsr_ntt_ring_mul_batch: host buffers, staged through bounded device chunks; returns when c is complete.
 * lsr_ntt_ring_mul_batch_device: device buffers on the context's device, asynchronous on `stream` (enqueues only).
 *
 * Workspace, ordering and graph capture.  n > 4096, and b_rows == 1 with batch > 1, use a workspace owned by the context.  Its
 * size depends on n alone; the first call that needs it allocates it, it is never resized and is freed by ntt_context_free.
 *   - Calls on one context are ordered: each call's work starts on the device after the previous call's work has finished, whatever
 *     streams they were issued on (an event recorded by every call).  Calls may come from several host threads.
 *   - Capture into a HIP graph (stream capture on `stream`): allowed once the workspace exists, i.e. after one eager call of a kind that
 *     needs it.  A call that would have to allocate it while `stream` is capturing returns -1.  A captured call is not bracketed by
 *     the ordering event: the caller orders graph launches against other ring multiplies on the same context.
 *   - ntt_context_free and lsr_ntt_ring_mul_batch wait for ring multiplies still pending on the context. */
int lsr_ntt_ring_mul_batch(const NttContext* ctx, uint64_t* c, const uint64_t* a, const uint64_t* b,
                           size_t batch, size_t b_rows) LSR_NOEXCEPT;
int lsr_ntt_ring_mul_batch_device(const NttContext* ctx, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b,
                                  size_t batch, size_t b_rows, void* stream) LSR_NOEXCEPT;

/* ---------------- NTT: batched ring inner product ---------------- */
/* c_j = sum_{i < terms} a_{j,i} * b_{j,i} in the ring of the context (as lsr_ntt_ring_mul_batch: X^n + 1 on negacyclic contexts,
 * X^n - 1 on cyclic ones): a row of A s, <b, r>, a long product split into blocks.  Natural coefficient order in and out, inputs
 * in [0,q), outputs canonical.  a: [batch][terms][n]; b: [b_rows][terms][n] with b_rows == batch (one vector b per output) or
 * b_rows == 1 (the same vector b for every output); c: [batch][n].  terms == 1 gives lsr_ntt_ring_mul_batch's output word for word.
 * The products are summed in registers and the inverse transform runs once per output: one fused pass at n <= 4096 (16 terms + 8
 * bytes of memory traffic per output residue, 8 terms + 8 with a shared b), three passes per chunk above.
 *
 * Refusals (-1 and lsr_last_error, before any device work), in this order: NULL context or buffer; b_rows not in {1, batch};
 * terms == 0.  Then batch == 0 is a no-op that returns 0.  Then: a context above n = 131072; terms above LSR_RING_DOT_MAX_TERMS
 * (the terms of one output tile are addressed through one 32-bit buffer range); c overlapping a or b in address range (the output
 * has another shape than the operands: there is no aliasing form); no visible device.
 *
 * lsr_ntt_ring_dot_batch: host buffers, staged through bounded device chunks; returns when c is complete.
 * lsr_ntt_ring_dot_batch_device: device buffers on the context's device, asynchronous on `stream` (enqueues only).
 *
 * Workspace, ordering and graph capture: the contract of lsr_ntt_ring_mul_batch above.  n > 4096, and b_rows == 1 with batch > 1, use
 * a workspace owned by the context whose size depends on n alone (never on batch or terms: the batch and, where they do not fit, the
 * terms are taken in chunks); the first eager call that needs it allocates it, it is never resized, a capturing call that would have
 * to allocate it returns -1.  Calls on one context are ordered by the same event as its ring multiplies, so the two kinds are
 * ordered against each other too; ntt_context_free waits for pending work.
 *
 * FP64-flavour contexts (q < 2^45) re-centre the running sum every LSR_RING_DOT_F64_RECENTRE_PERIOD products, which keeps it an
 * exact integer in a double for any number of terms. */
#define LSR_RING_DOT_MAX_TERMS 65536
#define LSR_RING_DOT_F64_RECENTRE_PERIOD 32
int lsr_ntt_ring_dot_batch(const NttContext* ctx, uint64_t* c, const uint64_t* a, const uint64_t* b,
                           size_t batch, size_t terms, size_t b_rows) LSR_NOEXCEPT;
int lsr_ntt_ring_dot_batch_device(const NttContext* ctx, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b,
                                  size_t batch, size_t terms, size_t b_rows, void* stream) LSR_NOEXCEPT;

/* ---------------- NTT: batched ring matrix-vector product with a resident matrix ---------------- */
/* y_j = M x_j over the ring of the context (as lsr_ntt_ring_mul_batch: X^n + 1 on negacyclic contexts, X^n - 1 on cyclic ones):
 * y[j][r] = sum_{c < cols} M[r][c] * x[j][c] — a module-SIS / Ajtai commitment, a fold of many rows by a matrix of ring-valued
 * challenges.  m: [rows][cols][n]; x: [batch][cols][n]; y: [batch][rows][n].  Natural coefficient order in and out; m and x under
 * the operand contract of lsr_ntt_ring_dot_batch's b and a (inputs in [0,q)); outputs canonical, equal word for word to
 * lsr_ntt_ring_dot_batch(ctx, ., x, M[r], batch, cols, 1) row by row.
 *
 * The matrix handle.  lsr_ntt_ring_matrix_create(_device) copies M to the context's device and keeps it there in the form the
 * product reads: at n <= 4096 the forward transform of every entry, computed once; above, M as given.  The handle owns that copy:
 * the caller's buffer may be changed or freed once lsr_ntt_ring_matrix_create returns (host pointer m) — for
 * lsr_ntt_ring_matrix_create_device (device pointer d_m, asynchronous on `stream`) once the work enqueued on `stream` up to that
 * point is done; products on any stream start behind it.  The handle is immutable after creation: products on one matrix may be
 * issued from several threads and on several streams.  The context must outlive the matrix: free every matrix of a context
 * (lsr_ntt_ring_matrix_free, NULL-safe, waits for products still reading the matrix) before ntt_context_free.
 * lsr_ntt_ring_matrix_rows / _cols: the dimensions; _row_block: the number of rows one workgroup of the n <= 4096 kernel keeps in
 * registers (a property of the context's arithmetic flavour; 1 above n = 4096) — all three 0 on NULL.
 *
 * Limits: rows in [1, LSR_RING_MATVEC_MAX_ROWS], cols in [1, LSR_RING_DOT_MAX_TERMS] (the x words and the y words of one tile are
 * each addressed through one 32-bit buffer range, which these two caps keep below 2^31 bytes: every cols within the cap goes through
 * one launch, there are no column groups), rows * cols * n * 8 <= LSR_RING_MATVEC_MAX_MATRIX_BYTES (the device copy; the kernel
 * addresses M one polynomial at a time from a 64-bit pointer).
 *
 * Refusals of create (NULL and lsr_last_error, before any device work), in this order: NULL ctx or m; rows == 0; cols == 0; rows
 * above LSR_RING_MATVEC_MAX_ROWS; cols above LSR_RING_DOT_MAX_TERMS; rows * cols * 16 above LSR_RING_MATVEC_MAX_MATRIX_BYTES (over
 * the cap at any n) — all of these without reading the context; then a context above n = 131072 (as lsr_ntt_ring_dot_batch);
 * rows * cols * n * 8 above the cap; no visible device.
 * Refusals of the product (-1 and lsr_last_error, before any device work): NULL mat, y or x.  Then batch == 0 is a no-op that
 * returns 0.  Then: y overlapping x in address range; no visible device.
 *
 * lsr_ntt_ring_matvec_batch: host buffers, staged through bounded device chunks; returns when y is complete.
 * lsr_ntt_ring_matvec_batch_device: device buffers on the context's device, asynchronous on `stream` (enqueues only).
 *
 * n <= 4096: one launch per call, no workspace, no ordering against other calls beyond the streams' own.  n > 4096: one ring inner
 * product per row and chunk of the batch plus a strided copy, through lsr_ntt_ring_dot_batch_device's workspace and a dense chunk
 * the first create on the context allocates (sizes fixed by n alone); ordering and graph capture are lsr_ntt_ring_dot_batch's — same
 * mutex, same event, one eager product before capturing. */
#define LSR_RING_MATVEC_MAX_ROWS 32768
#define LSR_RING_MATVEC_MAX_MATRIX_BYTES 1073741824
typedef struct LsrRingMatrix LsrRingMatrix;
LsrRingMatrix* lsr_ntt_ring_matrix_create(const NttContext* ctx, const uint64_t* m, size_t rows, size_t cols) LSR_NOEXCEPT;
LsrRingMatrix* lsr_ntt_ring_matrix_create_device(const NttContext* ctx, const uint64_t* d_m, size_t rows, size_t cols,
                                                 void* stream) LSR_NOEXCEPT;
void lsr_ntt_ring_matrix_free(LsrRingMatrix* mat) LSR_NOEXCEPT;
size_t lsr_ntt_ring_matrix_rows(const LsrRingMatrix* mat) LSR_NOEXCEPT;
size_t lsr_ntt_ring_matrix_cols(const LsrRingMatrix* mat) LSR_NOEXCEPT;
size_t lsr_ntt_ring_matrix_row_block(const LsrRingMatrix* mat) LSR_NOEXCEPT;
int lsr_ntt_ring_matvec_batch(const LsrRingMatrix* mat, uint64_t* y, const uint64_t* x, size_t batch) LSR_NOEXCEPT;
int lsr_ntt_ring_matvec_batch_device(const LsrRingMatrix* mat, uint64_t* d_y, const uint64_t* d_x, size_t batch,
                                     void* stream) LSR_NOEXCEPT;

/* ---------------- NTT: gadget decomposition, norm check and the fused product y = M G^-1(x) ---------------- */
/* An Ajtai commitment y = M x binds only when x is short.  These calls write arbitrary ring elements in small balanced digits, check
 * that an opened vector is short, and commit to the digits without materialising them.
 *
 * Parameters: b = base_log2, B = 2^b, D = digits, off = (B/2) (B^D - 1) / (B - 1) — B/2 in every digit position.
 * (b, D) is ADMISSIBLE for q when 2 <= b <= 32, D >= 1, b D <= 64; B/2 <= floor(q/2) (every digit is its own centred representative);
 * floor((q - 1)/2) <= off; floor(q/2) <= B^D - 1 - off.
 * lsr_ring_gadget_min_digits(q, base_log2): the smallest admissible D, 0 when there is none (e.g. every b for q = 2^64 - 2^32 + 1,
 * so cyclic Goldilocks contexts are refused by the rule itself).  Host only, no device needed.
 *
 * Digits.  For x in [0, q): v = x if x <= floor(q/2), else x - q; u = v + off, so 0 <= u < B^D <= 2^64 and wrapping 64-bit arithmetic
 * is exact.  Digit d is z_d = ((u >> b d) & (B - 1)) - B/2 in [-B/2, B/2 - 1], stored as the canonical residue (z_d, or q + z_d when
 * negative); sum_d z_d B^d = v exactly.  There is no carry chain: digit d is a function of the word and d alone.
 * G^-1 of a vector x [batch][xcols][n] is [batch][xcols D][n] with column c D + d = digit d of x[.][c], coefficient by coefficient.
 *
 * lsr_ntt_ring_decompose_batch(_device): x [count][n] in [0, q) -> out [count][digits][n].  Every ring degree and arithmetic flavour a
 *   context has; no workspace, so a device call can be captured into a HIP graph from the first call.  out must not overlap x.
 * lsr_ntt_ring_recompose_batch(_device): out[j] = sum_d B^d z[j][d] mod q for ANY canonical z [count][digits][n], short or not — the
 *   gadget product G z.  Needs only 2 <= b <= 32, D >= 1, b (D - 1) <= 64, not admissibility.  out must not overlap z.
 * lsr_ntt_ring_linf_batch(_device): linf[j] = max over the n coefficients of |centred x[j]|, x [count][n]; UINT64_MAX when some word of
 *   element j is >= q (a verifier passes untrusted data: the case is defined, and the other elements are unaffected).  The exact l2
 *   norm, which does not fit 64 bits, is lsr_ntt_ring_l2sq_batch below ("norms and projections of ring vectors").
 * lsr_ntt_ring_matvec_gadget_batch(_device): x [batch][xcols][n] with xcols * digits == lsr_ntt_ring_matrix_cols(mat) ->
 *   y [batch][rows][n] = lsr_ntt_ring_matvec_batch(mat, G^-1(x)) word for word.  n <= 4096: one launch, no workspace (the digits are
 *   extracted as the tile kernel loads x).  n > 4096 is refused: there lsr_ntt_ring_matvec_batch is itself a composed route, so
 *   decompose into a temporary and call it.
 * The plain forms take host buffers, staged through bounded device chunks, and return when the output is complete; the _device forms
 * take device buffers on the context's device and are asynchronous on `stream` (enqueue only).
 *
 * Refusals (-1 and lsr_last_error naming the entry point, before any device work), in this order: (1) NULL handle or buffer; (2) the
 * rules that do not read the context: b outside [2, 32], D == 0, b D > 64 (recompose: b (D - 1) > 64); (3) decompose and the fused
 * product: (b, D) not admissible for the context's q; (4) fused product: cols % digits != 0.  (5) Then count == 0 / batch == 0 is a
 * no-op that returns 0.  Then (6) the output overlapping the operand in address range; (7) fused product: n above 4096; (8) no
 * visible device. */
uint64_t lsr_ring_gadget_min_digits(uint64_t q, unsigned base_log2) LSR_NOEXCEPT;
int lsr_ntt_ring_decompose_batch(const NttContext* ctx, uint64_t* out, const uint64_t* x, size_t count, unsigned base_log2,
                                 size_t digits) LSR_NOEXCEPT;
int lsr_ntt_ring_decompose_batch_device(const NttContext* ctx, uint64_t* d_out, const uint64_t* d_x, size_t count, unsigned base_log2,
                                        size_t digits, void* stream) LSR_NOEXCEPT;
int lsr_ntt_ring_recompose_batch(const NttContext* ctx, uint64_t* out, const uint64_t* z, size_t count, unsigned base_log2,
                                 size_t digits) LSR_NOEXCEPT;
int lsr_ntt_ring_recompose_batch_device(const NttContext* ctx, uint64_t* d_out, const uint64_t* d_z, size_t count, unsigned base_log2,
                                        size_t digits, void* stream) LSR_NOEXCEPT;
int lsr_ntt_ring_linf_batch(const NttContext* ctx, const uint64_t* x, size_t count, uint64_t* linf) LSR_NOEXCEPT;
int lsr_ntt_ring_linf_batch_device(const NttContext* ctx, const uint64_t* d_x, size_t count, uint64_t* d_linf, void* stream) LSR_NOEXCEPT;
int lsr_ntt_ring_matvec_gadget_batch(const LsrRingMatrix* mat, uint64_t* y, const uint64_t* x, size_t batch, unsigned base_log2,
                                     size_t digits) LSR_NOEXCEPT;
int lsr_ntt_ring_matvec_gadget_batch_device(const LsrRingMatrix* mat, uint64_t* d_y, const uint64_t* d_x, size_t batch,
                                            unsigned base_log2, size_t digits, void* stream) LSR_NOEXCEPT;

/* ---------------- NTT: seeded ring sampling on the device and seed-expanded ring matrices ---------------- */
/* Exact sampling of ring elements from ChaCha20 streams: the public matrix of an Ajtai commitment from a
 * seed, short masking vectors and ternary secrets, and ring-valued challenges keyed by transcript digests that never leave the
 * device.  Integer code that reads only q and n of the context: every context (negacyclic, cyclic, large cyclic) and every
 * arithmetic flavour is served by one path.  out: [count][n], canonical residues, natural coefficient order.
 *
 * Streams.  A stream is (256-bit key, domain, 64-bit index).  Its 64-bit word w is ChaCha20 block w / 8 (the 32-bit block
 * counter), 32-bit words 2 (w % 8) (low half) and 2 (w % 8) + 1 (high half); the nonce is {domain, index_lo, index_hi}.  A key is
 * four little-endian 64-bit words; the 32 bytes of a SHA3 digest, in their own byte order, are a valid key.
 * Element e < count uses key keys[4 (e / components) ..] and stream index index_base + (e % components): ceil(count / components)
 * keys are read, the last group may be ragged.
 *
 * The one rejection primitive draw(m; w_0, w_1, ...; U) for m >= 2: L = bitlen(m - 1), F = floor(U / L); the candidates of a word
 * are its F low fields (w >> f L) & (2^L - 1), f = 0 .. F-1; words are scanned in order and fields in order within a word; the
 * result is the first candidate below m.  After LSR_RING_SAMPLE_MAX_WORDS words without an accepted candidate the result is field
 * 0 of the last word reduced mod m (probability at most 2^-64; defined so that the function is total).  m = 1 gives 0 and consumes
 * nothing.
 *
 * Kinds.
 *   LSR_RING_SAMPLE_UNIFORM (param must be 0): coefficient i = draw(q; word a n + i for a = 0, 1, ...; U = 64) — exactly uniform
 *     on [0, q).
 *   LSR_RING_SAMPLE_BOUNDED (param beta, 1 <= beta <= (q - 1) / 2): r = draw(2 beta + 1; the same words; U = 64), v = r - beta,
 *     stored as the canonical residue (v, or q + v) — exactly uniform on [-beta, beta].
 *   LSR_RING_SAMPLE_BALL (param kappa, 1 <= kappa <= n): exactly kappa coefficients +-1, the rest 0, uniform over that set
 *     (Dilithium's SampleInBall).  c = 0; for s = 0 .. kappa-1: i = n - kappa + s, j = draw(i + 1; word a kappa + s for a = 0, 1,
 *     ...; U = 63); c[i] = c[j]; then c[j] = (bit 63 of word s) ? q - 1 : 1.
 * All word indices stay below 2^28, so the block counter never wraps.
 * Sampling is NOT constant-time: the pattern of rejections depends on the stream.  Rejected candidates are independent of the
 * accepted values (each candidate is a fresh field of the stream), so the timing reveals nothing about the values drawn.
 *
 * lsr_ring_sample_key_from_seed: the key {seed_lo, seed_hi, "LSR1", "STRM", 0, 0, 0, 0} of a raw 64-bit seed (reproducible test
 *   streams, as lsr_sample_gaussian_seeded; only as secret as the seed).  Host only.
 * lsr_ntt_ring_sample_batch: host buffers (out and keys), staged through bounded device chunks; complete on return.
 * lsr_ntt_ring_sample_batch_device: d_out and d_keys are device memory on the context's device (d_keys 8-byte aligned; it may be
 *   the d_hashes32 of lsr_fs_challenge_batch_device); enqueues only, allocates nothing, can be captured into a HIP graph from the
 *   first call.
 * Refusals (-1 and lsr_last_error naming the entry point, before any device work), in this order: (1) NULL context, buffer or
 * keys; (2) an unknown kind, components == 0; (3) the rules that read the context: UNIFORM with param != 0, BOUNDED with beta == 0
 * or beta > (q - 1) / 2, BALL with kappa == 0 or kappa > n.  (4) Then count == 0 is a no-op that returns 0.  Then (5) index_base +
 * components overflowing 64 bits; no visible device.
 *
 * lsr_ntt_ring_matrix_create_seeded: the matrix whose entry M[r][c] is the UNIFORM element with stream index index_base + r cols +
 *   c under the one key, sampled straight into the handle's buffer on the device and, at n <= 4096, transformed in place: the
 *   matrix never crosses PCIe and never exists on the host.  Complete on return.  The handle is indistinguishable from
 *   lsr_ntt_ring_matrix_create_device of the sampled words.  Limits and refusal order of lsr_ntt_ring_matrix_create with key in the
 *   place of m; index_base + rows cols overflowing 64 bits is refused just before the visible-device check. */
#define LSR_RING_SAMPLE_UNIFORM 0
#define LSR_RING_SAMPLE_BOUNDED 1
#define LSR_RING_SAMPLE_BALL 2
#define LSR_RING_SAMPLE_MAX_WORDS 64
void lsr_ring_sample_key_from_seed(uint64_t seed, uint64_t key[4]) LSR_NOEXCEPT;
int lsr_ntt_ring_sample_batch(const NttContext* ctx, uint64_t* out, size_t count, int kind, uint64_t param, const uint64_t* keys,
                              size_t components, uint32_t domain, uint64_t index_base) LSR_NOEXCEPT;
int lsr_ntt_ring_sample_batch_device(const NttContext* ctx, uint64_t* d_out, size_t count, int kind, uint64_t param,
                                     const uint64_t* d_keys, size_t components, uint32_t domain, uint64_t index_base,
                                     void* stream) LSR_NOEXCEPT;
LsrRingMatrix* lsr_ntt_ring_matrix_create_seeded(const NttContext* ctx, const uint64_t key[4], uint32_t domain, uint64_t index_base,
                                                 size_t rows, size_t cols) LSR_NOEXCEPT;

/* ---------------- NTT: batched fold of ring vectors by ring-valued challenges ---------------- */
/* out[j][c] = sum_{i < terms} p[j][i] * v[j term_stride + i][c] in the ring of the context (as lsr_ntt_ring_mul_batch: X^n + 1 on
 * negacyclic contexts, X^n - 1 on cyclic ones): the folded witness z_j = sum_i c_{j,i} x_{j,i} of a folding or Sigma protocol over
 * Ajtai commitments, and — applied to the commitments — the folded commitment.
 * v: [vectors][width][n] with vectors = (outputs - 1) term_stride + terms; p: [outputs][terms][n]; out: [outputs][width][n].  Words
 * are canonical ([0,q) in, canonical out) in natural coefficient order, as lsr_ntt_ring_dot_batch; a challenge's -1 is q - 1, which is
 * what LSR_RING_SAMPLE_BALL writes.  term_stride as lsr_lwe_ring_combine_rows_device: 0 — every output folds the same `terms`
 * vectors; terms — disjoint groups; any other value is allowed (overlapping or spaced groups).
 * out[j][c] equals lsr_ntt_ring_dot_batch on the gathered operands a[(j,c)][i] = v[j term_stride + i][c], b[(j,c)][i] = p[j][i]
 * word for word, in every arithmetic flavour and at every n from 2 to 131072.  The transform of a challenge is shared by the `width`
 * components it multiplies: one fused pass at n <= 4096 behind one transform of the challenges, three passes per chunk above.
 *
 * Limits: terms <= LSR_RING_DOT_MAX_TERMS, width <= LSR_RING_FOLD_MAX_WIDTH.
 * Refusals (-1 and lsr_last_error naming the entry point, before any device work), in this order: (1) NULL context or buffer;
 * (2) terms == 0.  (3) Then outputs == 0 or width == 0 is a no-op that returns 0 (as batch == 0 of lsr_ntt_ring_dot_batch).  Then
 * (4) terms above LSR_RING_DOT_MAX_TERMS; (5) width above LSR_RING_FOLD_MAX_WIDTH; (6) a size that overflows size_t: vectors,
 * vectors * width, outputs * terms, outputs * width, or one of the last three times 16 bytes (a polynomial of the smallest ring) —
 * all of these without reading the context.  Then (7) a context above n = 131072; (8) the byte size of v, p or out overflowing
 * size_t at the context's n; (9) out overlapping v, then p, in address range (there is no aliasing form); (10) no visible device.
 *
 * lsr_ntt_ring_fold_batch: host buffers, staged through bounded device chunks; returns when out is complete.
 * lsr_ntt_ring_fold_batch_device: device buffers on the context's device, asynchronous on `stream` (enqueues only).
 *
 * Workspace, ordering and graph capture: the contract of lsr_ntt_ring_dot_batch above, and its workspace — no other.  Every call
 * uses it (its size depends on n alone; outputs, components and terms that do not fit are taken in chunks and groups); the first
 * eager ring inner product or fold on the context allocates it, a capturing call that would have to allocate it returns -1: make one
 * eager call first.  Calls are ordered by the context's ring event against each other and against the ring multiplies and inner
 * products of the context.  FP64-flavour contexts re-centre the running sum every LSR_RING_DOT_F64_RECENTRE_PERIOD products. */
#define LSR_RING_FOLD_MAX_WIDTH 65536
int lsr_ntt_ring_fold_batch(const NttContext* ctx, uint64_t* out, const uint64_t* v, const uint64_t* p,
                            size_t outputs, size_t terms, size_t term_stride, size_t width) LSR_NOEXCEPT;
int lsr_ntt_ring_fold_batch_device(const NttContext* ctx, uint64_t* d_out, const uint64_t* d_v, const uint64_t* d_p,
                                   size_t outputs, size_t terms, size_t term_stride, size_t width, void* stream) LSR_NOEXCEPT;

/* ---------------- NTT: Galois automorphisms of ring elements and the twisted ring inner product ---------------- */
/* sigma_g: X -> X^g in the ring of the context.  With n the context's degree, N = 2 n on negacyclic contexts
 * (X^n + 1) and N = n on cyclic ones (X^n - 1); a Galois element is an odd g with 1 <= g < N.  sigma_g(sum_i x_i X^i) =
 * sum_i x_i X^(i g) reduced in the ring; with h = g^-1 mod N, on canonical words in natural coefficient order:
 *   negacyclic: s = (j h) mod 2 n;  out[j] = x[s] if s < n, else q - x[s - n] (0 where x[s - n] is 0);
 *   cyclic:     out[j] = x[(j h) mod n].
 * g = N - 1 is the conjugation: the constant coefficient of sigma_{N-1}(a) b is the inner product of the coefficient vectors of a and
 * b mod q.  sigma_g sigma_h = sigma_{g h mod N}.  The output for a word >= q is unspecified (arithmetic on the word: it never faults).
 *
 * lsr_ntt_ring_automorphism_batch(_device): out[e] = sigma_g(x[e]), e < count, buffers [count][n].  Served on every context the
 * library creates and at every n (large cyclic contexts up to 2^22 included): it runs no transform, needs no workspace and takes
 * no part in the context's ring ordering — the device form is asynchronous in plain stream order (as
 * lsr_ntt_ring_decompose_batch_device) and capturable with no warm-up call.
 * lsr_ntt_ring_dot_galois_batch(_device): c_j = sum_{i < terms} sigma_g(a_{j,i}) b_{j,i}, shapes and b_rows of lsr_ntt_ring_dot_batch.
 * c equals lsr_ntt_ring_dot_batch applied to the materialised sigma_g(a) word for word, in every arithmetic flavour; g = 1 equals
 * lsr_ntt_ring_dot_batch.  The permutation and the sign are applied where the fused kernel reads a: sigma_g(a) never exists in
 * memory.  Served at n <= 4096 only (as lsr_ntt_ring_matvec_gadget_batch); above, compose the two calls.  Workspace, ordering event
 * and graph capture: the contract of lsr_ntt_ring_dot_batch, and its workspace (a shared b needs it: one eager ring inner product
 * on the context before a capture).
 * g is passed by value and validated on the host: the device forms enqueue only.
 *
 * Refusals (-1 and lsr_last_error naming the entry point, before any device work), in this order: (1) NULL context or buffer;
 * (2) inner product only: b_rows not 1 or batch, then terms == 0; (3) g even (both rings: read without the context).  (4) Then
 * count == 0 or batch == 0 is a no-op that returns 0.  (5) A size that overflows size_t: batch * terms, b_rows * terms, or a
 * polynomial count times 16 bytes (a polynomial of the smallest ring) — all of these without reading the context.  Then (6) g >= N;
 * the byte size of a buffer overflowing size_t at the context's n; inner product only: n above 4096, terms above
 * LSR_RING_DOT_MAX_TERMS; the output overlapping an input in address range (there is no in-place form); no visible device.
 *
 * The host forms stage through bounded device chunks and return when the output is complete. */
int lsr_ntt_ring_automorphism_batch(const NttContext* ctx, uint64_t* out, const uint64_t* x, size_t count, uint64_t g) LSR_NOEXCEPT;
int lsr_ntt_ring_automorphism_batch_device(const NttContext* ctx, uint64_t* d_out, const uint64_t* d_x, size_t count, uint64_t g,
                                           void* stream) LSR_NOEXCEPT;
int lsr_ntt_ring_dot_galois_batch(const NttContext* ctx, uint64_t* c, const uint64_t* a, const uint64_t* b,
                                  size_t batch, size_t terms, size_t b_rows, uint64_t g) LSR_NOEXCEPT;
int lsr_ntt_ring_dot_galois_batch_device(const NttContext* ctx, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b,
                                         size_t batch, size_t terms, size_t b_rows, uint64_t g, void* stream) LSR_NOEXCEPT;

/* ---------------- NTT: norms and projections of ring vectors ---------------- */
/* The relation a LaBRADOR / Greyhound-style argument proves is |s|_2 <= B, and it proves it through the Johnson-Lindenstrauss
 * projection p = Pi s in Z^256 of the witness.  Integer code that reads only q and n of the context, as the
 * sampling calls: every context and arithmetic flavour is served by one path.
 * A vector is `width` ring elements, [width][n] canonical words; its flattened position is pos = c n + k and len = width n.
 * centred(v) = v if v <= floor(q/2), else v - q, as lsr_ntt_ring_linf_batch.
 *
 * lsr_ntt_ring_l2sq_batch(_device): x [count][width][n] -> out [count][2], the low word then the high word of sum_pos centred(x)^2
 *   as an unsigned 128-bit integer.  Both words are UINT64_MAX when a word of the vector is >= q or the sum is 2^128 - 1 or more
 *   (whatever the order of summation: the terms are non-negative and a partial sum that overflows is remembered); the other vectors
 *   of the batch are unaffected.  No workspace, plain stream order, capturable from the first call.
 *
 * lsr_ntt_ring_project_batch(_device): x [count][width][n] -> out [count][LSR_RING_PROJECT_ROWS] int64 and status [count] int32.
 *   Vector j uses key keys[4 (j / components) ..]; row r of its matrix is the stream (key, domain, index_base + 256 (j % components)
 *   + r) of "seeded ring sampling" above, ceil(count / components) keys are read.  Entry pi[r][pos] = (f & 1) - (f >> 1) with
 *   f = (word[pos / 32] >> 2 (pos % 32)) & 3 of that stream: 0, +1, -1, 0 for f = 0 .. 3, so +-1 with probability 1/4 each.
 *   out[j][r] = sum_pos pi[r][pos] centred(x[j][pos]), an exact int64 stored as its two's-complement word.
 *   status[j]: 1 — done; -1 — a word of the vector is >= q; 0 — some |centred| is above `bound` (and no word is >= q).  For a status
 *   other than 1 all 256 outputs of that vector are 0; the other vectors are unaffected.
 *   bound is the caller's l-infinity bound: len bound <= 2^63 - 1 is what makes the 64-bit sum exact.
 *   The matrix is generated from the streams inside the kernel that applies it and never exists in memory.  The device form
 *   enqueues three launches (the outputs zeroed and the status set to 1; the slices of the vectors added into the outputs by 64-bit
 *   integer atomics — wrapping adds, the same word in any order; the outputs of a refused vector cleared) and allocates nothing:
 *   capturable from the first call.  out and status are written by all three, so nothing else may touch them in between.
 * lsr_ntt_ring_project_matrix_batch(_device): rows rows_first .. rows_first + rows - 1 of the matrix of ONE (key, index_base) — the
 *   matrix of a vector with j % components = 0 — as ring elements: out [rows][width][n] with words 0, 1, q - 1.  Coefficient 0 of
 *   lsr_ntt_ring_dot_galois_batch(row r, s, conjugation) is then p_r mod q, which is how a verifier proves p_r.  (A separate entry,
 *   not a kind of lsr_ntt_ring_sample_batch: a row spans `width` elements.)  key: four words, host memory for the plain form and
 *   device memory for the _device form.
 * The plain forms take host buffers, staged through bounded device chunks of whole vectors (rows), and return when the output is
 * complete; the _device forms take device buffers on the context's device and are asynchronous on `stream`.
 *
 * Refusals (-1 and lsr_last_error naming the entry point, before any device work), in this order: (1) NULL context, buffer, keys or
 * status; (2) components == 0, then bound == 0; rows_first + rows above 256.  (3) Then count == 0, width == 0 or rows == 0 is a no-op
 * that returns 0.  (4) A size that overflows size_t without reading the context: count * width (rows * width), that times 16 bytes,
 * count * 256 * 8.  Then (5) the rules that read the context: bound above floor(q/2), len above 2^32 (the positions a stream's block
 * counter reaches), len * bound above 2^63 - 1; index_base + 256 components (matrix: index_base + 256) overflowing 64 bits; the
 * byte size of a buffer overflowing size_t at the context's n; out (then status) overlapping x in address range; no visible
 * device.
 *
 * lsr_ntt_ring_project_adjoint_batch(_device): the adjoint Pi^T w of the projection, as ring vectors — the
 *   step that turns the 256 constraints on p into ring constraints: with weights w in Z_q^256, the constant coefficient of
 *   <sigma_{-1}(Pi^T w), s> is <w, p> mod q.  weights [groups][sets][256] canonical words, groups = ceil(count / components): all
 *   vectors of one key group (the witness vectors of one proof) share their weights.  Vector j < count has the matrix of
 *   lsr_ntt_ring_project_batch exactly: key keys[4 (j / components) ..], row r the stream (key, domain, index_base +
 *   256 (j % components) + r), entry pi[r][pos] from the 2-bit field as above; ceil(count / components) key groups are read.
 *   out [count][sets][width][n] canonical words.  conjugate == 0: out[j][k][pos] = sum_r weights[j / components][k][r] pi_j[r][pos]
 *   mod q.  conjugate == 1: every ring element of that result is replaced by its image under sigma_g, g = N - 1 (N = 2n on
 *   negacyclic contexts, N = n on cyclic ones) — word for word what lsr_ntt_ring_automorphism_batch returns for that g.
 *   status[j]: 1 — done; -1 — a weight word of the vector's group (any set) is >= q: then all sets * width * n outputs of that vector
 *   are 0; the other vectors are unaffected.  Exact integer arithmetic for every modulus a context admits (plain 64-bit sums below
 *   q = 2^55, a reduction per step above).  1 <= sets <= LSR_RING_PROJECT_ADJOINT_MAX_SETS.
 *   The device form is one kernel that writes every output word and the status itself (more than 2^30 workgroups: several
 *   launches): no init pass, no atomics, nothing allocated, no workspace, no part in the context's ring ordering; plain stream order,
 *   capturable from the first call.  The plain form stages whole vectors through bounded device chunks, each with its own key and
 *   weight groups.
 *   Refusals, in this order: (1) NULL context, out, status, weights or keys; (2) components == 0, then sets == 0 or sets above
 *   LSR_RING_PROJECT_ADJOINT_MAX_SETS, then conjugate other than 0 or 1.  (3) Then count == 0 or width == 0 is a no-op that returns 0.
 *   (4) A size that overflows size_t without reading the context: count * sets, that times width, that times 16 bytes.  Then (5) the
 *   rules that read the context: len above 2^32; index_base + 256 components overflowing 64 bits; the byte size of a buffer
 *   overflowing size_t at the context's n; out (then status) overlapping weights in address range; no visible device. */
#define LSR_RING_PROJECT_ROWS 256
#define LSR_RING_PROJECT_ADJOINT_MAX_SETS 16
int lsr_ntt_ring_l2sq_batch(const NttContext* ctx, const uint64_t* x, size_t count, size_t width, uint64_t* out) LSR_NOEXCEPT;
int lsr_ntt_ring_l2sq_batch_device(const NttContext* ctx, const uint64_t* d_x, size_t count, size_t width, uint64_t* d_out,
                                   void* stream) LSR_NOEXCEPT;
int lsr_ntt_ring_project_batch(const NttContext* ctx, int64_t* out, int32_t* status, const uint64_t* x, size_t count, size_t width,
                               uint64_t bound, const uint64_t* keys, size_t components, uint32_t domain,
                               uint64_t index_base) LSR_NOEXCEPT;
int lsr_ntt_ring_project_batch_device(const NttContext* ctx, int64_t* d_out, int32_t* d_status, const uint64_t* d_x, size_t count,
                                      size_t width, uint64_t bound, const uint64_t* d_keys, size_t components, uint32_t domain,
                                      uint64_t index_base, void* stream) LSR_NOEXCEPT;
int lsr_ntt_ring_project_matrix_batch(const NttContext* ctx, uint64_t* out, size_t rows_first, size_t rows, size_t width,
                                      const uint64_t* key, uint32_t domain, uint64_t index_base) LSR_NOEXCEPT;
int lsr_ntt_ring_project_matrix_batch_device(const NttContext* ctx, uint64_t* d_out, size_t rows_first, size_t rows, size_t width,
                                             const uint64_t* d_key, uint32_t domain, uint64_t index_base,
                                             void* stream) LSR_NOEXCEPT;
int lsr_ntt_ring_project_adjoint_batch(const NttContext* ctx, uint64_t* out, int32_t* status, const uint64_t* weights, size_t count,
                                       size_t sets, size_t width, int conjugate, const uint64_t* keys, size_t components,
                                       uint32_t domain, uint64_t index_base) LSR_NOEXCEPT;
int lsr_ntt_ring_project_adjoint_batch_device(const NttContext* ctx, uint64_t* d_out, int32_t* d_status, const uint64_t* d_weights,
                                              size_t count, size_t sets, size_t width, int conjugate, const uint64_t* d_keys,
                                              size_t components, uint32_t domain, uint64_t index_base,
                                              void* stream) LSR_NOEXCEPT;

/* ---------------- NTT: scalar-weighted aggregation of ring vectors ---------------- */
/* lsr_ntt_ring_scalar_combine_batch(_device): sums of ring vectors weighted by SCALARS of Z_q, plus an addend —
 * the step of a LaBRADOR / Greyhound-style argument that collapses the L constraint families with constant-term conditions by
 * scalars psi^(k) in Z_q^L and adds the back-projection: phi''^(k)_i = sum_l psi^(k)_l phi'^(l)_i + (Pi^T w^(k))_i.  A scalar acts
 * coefficient-wise, so no transform runs: out[sets x len] = weights[sets x terms] v[terms x len] mod q per vector, v read once for
 * all sets.  A vector is `width` ring elements, [width][n] canonical words, pos = c n + k and len = width n, as above.
 *   v: [vectors][width][n] with vectors = (count - 1) term_stride + terms.  term_stride as lsr_ntt_ring_fold_batch: 0 — every output
 *     sums the same `terms` vectors; terms — disjoint groups; any other value is allowed.
 *   weights: [groups][sets][terms] canonical words, groups = ceil(count / components): the vectors of one group (one proof) share
 *     their weights, the convention of lsr_ntt_ring_project_adjoint_batch.
 *   addend: NULL, or [count][sets][width][n].
 *   out: [count][sets][width][n] canonical words,
 *     out[j][k][pos] = (addend ? addend[j][k][pos] : 0) + sum_{i < terms} weights[j / components][k][i] v[j term_stride + i][pos] mod q.
 *   addend may be EXACTLY out (the in-place form: what follows lsr_ntt_ring_project_adjoint_batch with conjugate = 1, whose output
 *     layout this is); any other overlap is refused.
 *   status[j]: 1 — done; -1 — a weight word of the vector's group (any set) is >= q: then all sets * len outputs of that vector are
 *     0, in place included, and the other vectors are unaffected (the adjoint's rule).
 *   Words of v and addend are canonical by contract, as in lsr_ntt_ring_fold_batch: a word >= q gives an unspecified result and never
 *   faults.  The result is the exact integer residue, so it does not depend on the arithmetic flavour.  Served on every context the
 *   library creates — negacyclic FP64 and 64-bit flavours, the 60-bit prime, Goldilocks cyclic contexts, those above n = 131072
 *   included: the call reads only q, the flavour's reduction constants and n, and no twiddle table.
 * Limits: 1 <= sets <= LSR_RING_SCALAR_COMBINE_MAX_SETS, 1 <= terms <= LSR_RING_DOT_MAX_TERMS, len <= 2^32.
 * Refusals (-1 and lsr_last_error naming the entry point, before any device work), in this order: (1) NULL ctx, out, status, v or
 * weights; (2) components == 0, then sets == 0 or above LSR_RING_SCALAR_COMBINE_MAX_SETS, then terms == 0 or above
 * LSR_RING_DOT_MAX_TERMS.  (3) Then count == 0 or width == 0 is a no-op that returns 0.  (4) A size that overflows size_t without
 * reading the context: vectors, vectors * width, count * sets, count * sets * width, groups * sets * terms, or one of these times 16
 * bytes.  Then (5) the rules that read the context: len above 2^32; the byte size of a buffer overflowing size_t at the context's n;
 * out overlapping v, then weights, then status, then an addend that is neither NULL nor equal to out; no visible device.
 *
 * The device form is one kernel that writes every output word and the status itself (more than 2^30 workgroups: several launches):
 * no init pass, no atomics, no workspace, nothing allocated, no part in the context's ring ordering; plain stream order, capturable
 * from the first call.  A workgroup owns LSR_RING_SCALAR_COMBINE_TILE positions of one vector, two per lane with 16-byte accesses,
 * when v, out and addend are 16-byte aligned (half as many, one per lane, when one of them is not) and stages the weights
 * LSR_RING_SCALAR_COMBINE_STAGE terms at a time; FP64-flavour contexts re-centre the running sums every
 * LSR_RING_DOT_F64_RECENTRE_PERIOD products.
 * The plain form takes host buffers and returns when out and status are complete: whole outputs go through bounded device chunks,
 * each with its weight groups (term_stride == 0: v goes up once); an output whose terms exceed the bound takes them in groups, the
 * in-place addend carrying the running sum from one group to the next. */
#define LSR_RING_SCALAR_COMBINE_MAX_SETS 16
#define LSR_RING_SCALAR_COMBINE_TILE 512
#define LSR_RING_SCALAR_COMBINE_STAGE 128
int lsr_ntt_ring_scalar_combine_batch(const NttContext* ctx, uint64_t* out, int32_t* status, const uint64_t* v, const uint64_t* weights,
                                      const uint64_t* addend, size_t count, size_t sets, size_t terms, size_t term_stride, size_t width,
                                      size_t components) LSR_NOEXCEPT;
int lsr_ntt_ring_scalar_combine_batch_device(const NttContext* ctx, uint64_t* d_out, int32_t* d_status, const uint64_t* d_v,
                                             const uint64_t* d_weights, const uint64_t* d_addend, size_t count, size_t sets,
                                             size_t terms, size_t term_stride, size_t width, size_t components,
                                             void* stream) LSR_NOEXCEPT;

/* ---------------- NTT: batched ring Gram matrices G = A B^T ---------------- */
/* Every pairwise ring inner product of the vectors of one family with the vectors of another, or of one family with itself — the
 * "garbage" polynomials g_il = <s_i, s_l> and h_il = <phi_i, s_l> + <phi_l, s_i> of a LaBRADOR / Greyhound style argument (DESIGN.md
 * section 5j).  The ring is the context's (X^n + 1 on negacyclic contexts, X^n - 1 on cyclic ones); words are canonical ([0,q) in,
 * canonical out) in natural coefficient order.  a: [batch][ra][width][n], b: [batch][rb][width][n]; a family is one index j < batch.
 *   Cross form (b != NULL): g is [batch][ra][rb][n], g[j][i][l] = sum_{c < width} a[j][i][c] * b[j][l][c].  b may be the pointer a
 *     (the full square matrix of one family; with rb == ra it is transformed once).
 *   Symmetric form (b == NULL): rb must equal ra =: r; only i <= l is computed and stored, g is [batch][r (r + 1) / 2][n] and the
 *     pair (i, l) is polynomial i r - i (i - 1) / 2 + (l - i) of its family.
 * Every output equals lsr_ntt_ring_dot_batch(ctx, ., a[j][i], b[j][l], 1, width, 1) word for word, in every arithmetic flavour and
 * at every n from 2 to 131072 (all arithmetic is exact).  Each of the (ra + rb) width operand polynomials of a family is transformed
 * once and each output inverse-transformed once; between them runs a register-blocked pointwise product over E x E outputs per
 * workgroup.  lsr_ntt_ring_gram_block: that edge E for the context's flavour (0 on NULL), as lsr_ntt_ring_matrix_row_block.
 *
 * Limits: ra, rb <= LSR_RING_GRAM_MAX_VECTORS, width <= LSR_RING_DOT_MAX_TERMS, one family's operands ((ra + rb) width n 8 bytes;
 * symmetric form: ra for ra + rb) and one family's outputs each <= LSR_RING_GRAM_MAX_FAMILY_BYTES.
 * Refusals (-1 and lsr_last_error naming the entry point, before any device work), in this order: (1) NULL ctx, g or a; (2) ra == 0,
 * width == 0, or b != NULL and rb == 0; (3) b == NULL and rb != ra; (4) ra or rb above LSR_RING_GRAM_MAX_VECTORS, width above
 * LSR_RING_DOT_MAX_TERMS; (5) a size that overflows size_t: batch ra width, batch rb width, the output count, or one of them times
 * 16 bytes (a polynomial of the smallest ring) — all of these without reading the context.  Then batch == 0 is a no-op that returns
 * 0.  Then (6) a context above n = 131072; (7) a family above LSR_RING_GRAM_MAX_FAMILY_BYTES; (8) more vectors in a family (ra + rb;
 * symmetric: ra) than the workspace holds polynomials — the message names LAMBDA_SNARK_NTT_CHUNK_MIB, which sizes it; (9) g
 * overlapping a, then b, in address range; (10) no visible device.
 *
 * lsr_ntt_ring_gram_batch: host buffers, whole families staged through bounded device chunks; returns when g is complete.
 * lsr_ntt_ring_gram_batch_device: device buffers on the context's device, asynchronous on `stream` (enqueues only).  a and b are
 * never written.
 *
 * Workspace, ordering and graph capture: the contract of lsr_ntt_ring_dot_batch above, and its workspace — no other.  Every call
 * uses it (its size depends on n alone): families that fit are taken in chunks of whole families, a family that does not fit in
 * groups of columns, the running sums waiting in g as canonical evaluation-domain words between groups.  The first eager ring inner
 * product, fold or Gram call on the context allocates it; a capturing call that would have to allocate it returns -1: make one eager
 * call first.  FP64-flavour contexts re-centre the running sums every LSR_RING_DOT_F64_RECENTRE_PERIOD columns. */
#define LSR_RING_GRAM_MAX_VECTORS 64
#define LSR_RING_GRAM_MAX_FAMILY_BYTES 1073741824
int lsr_ntt_ring_gram_batch(const NttContext* ctx, uint64_t* g, const uint64_t* a, const uint64_t* b, size_t batch, size_t ra, size_t rb,
                            size_t width) LSR_NOEXCEPT;
int lsr_ntt_ring_gram_batch_device(const NttContext* ctx, uint64_t* d_g, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t ra,
                                   size_t rb, size_t width, void* stream) LSR_NOEXCEPT;
size_t lsr_ntt_ring_gram_block(const NttContext* ctx) LSR_NOEXCEPT;

/* ---------------- NTT: the symmetrised packed Gram matrix and ring quadratic forms ---------------- */
/* The two pieces that close a LaBRADOR / Greyhound style verifier's equations <z, z> = sum g_il c_i c_l and sum_i <phi_i, z> c_i =
 * sum h_il c_i c_l on the device.  Ring, word and order conventions: the Gram call's above.
 *
 * lsr_ntt_ring_gram_sym2_batch(_device): a and b are [batch][r][width][n], both non-NULL (b may be the pointer a); h is
 * [batch][r (r + 1) / 2][n] in the packed order of the symmetric Gram form, with
 *   h[j][(i, l)] = <a_i, b_l> + <a_l, b_i> for i < l,   h[j][(i, i)] = <a_i, b_i> (once).
 * Every off-diagonal word equals (lsr_ntt_ring_dot_batch(a_i, b_l) + lsr_ntt_ring_dot_batch(a_l, b_i)) mod q and every diagonal word
 * lsr_ntt_ring_dot_batch(a_i, b_i), in every flavour.  Plan, limits, workspace, ordering and capture contract: lsr_ntt_ring_gram_batch's
 * cross form with ra = rb = r (one third mode of its kernel: a block pair adds both products into one accumulator).  Refusals: those of
 * lsr_ntt_ring_gram_batch in its order with ra = rb = r, (1) including a NULL b.
 *
 * lsr_ntt_ring_quadform_batch(_device): g is [batch][r (r + 1) / 2][n] in the same packed order, c is [c_rows][r][n] with c_rows ==
 * batch (challenges per family) or c_rows == 1 (one set for every family), out is [batch][n]:
 *   out[j] = sum_i g[j][(i, i)] c_i c_i + offdiag * sum_{i < l} g[j][(i, l)] c_i c_l.
 * offdiag is a scalar word below q: 2 for a g that stores each off-diagonal entry once (the symmetric Gram form), 1 for an h that
 * already holds both cross terms (the sym2 form); any other canonical word is allowed.  Every output word equals the composed route
 * (lsr_ntt_ring_mul_batch per pair, a scaling by offdiag mod q, lsr_ntt_ring_dot_batch with terms = r (r + 1) / 2) in every flavour
 * and at every n from 2 to 131072: all arithmetic is exact.  r + r (r + 1) / 2 forward transforms (a shared c: once per call) and one
 * inverse per family; between them a pointwise kernel evaluates the form row by row of the triangle, the rows split into slices
 * balanced by pairs whose partial sums are added in a fixed order (no atomics).
 * Refusals (-1 and lsr_last_error naming the entry point, before any device work), in this order: (1) NULL ctx, out, g or c; (2) r
 * == 0; (3) c_rows neither 1 nor batch; (4) r above LSR_RING_GRAM_MAX_VECTORS; (5) a size that overflows size_t: batch r (r + 1) / 2,
 * c_rows r, or one of them times 16 bytes — all of these without reading the context.  Then batch == 0 is a no-op that returns 0.
 * Then (6) a context above n = 131072; (7) offdiag >= q; (8) one family's g above LSR_RING_GRAM_MAX_FAMILY_BYTES; (9) r + 2
 * polynomials (the transformed c of one family, one of g, one partial sum) not fitting the workspace — the message names
 * LAMBDA_SNARK_NTT_CHUNK_MIB, which sizes it; (10) out overlapping g, then c, in address range; (11) no visible device.
 * The host form stages whole families through bounded device chunks (a shared c goes up once) and returns when out is complete; the
 * _device form takes device buffers on the context's device and only enqueues on `stream`.  g and c are never written.
 * Workspace, ordering and graph capture: the contract of lsr_ntt_ring_dot_batch above, and its workspace — no other.  A family
 * whose transforms do not fit it is taken in groups of consecutive packed pairs with the transformed c resident, the running sum
 * waiting in out as canonical evaluation-domain words between groups. */
int lsr_ntt_ring_gram_sym2_batch(const NttContext* ctx, uint64_t* h, const uint64_t* a, const uint64_t* b, size_t batch, size_t r,
                                 size_t width) LSR_NOEXCEPT;
int lsr_ntt_ring_gram_sym2_batch_device(const NttContext* ctx, uint64_t* d_h, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t r,
                                        size_t width, void* stream) LSR_NOEXCEPT;
int lsr_ntt_ring_quadform_batch(const NttContext* ctx, uint64_t* out, const uint64_t* g, const uint64_t* c, size_t batch, size_t r,
                                size_t c_rows, uint64_t offdiag) LSR_NOEXCEPT;
int lsr_ntt_ring_quadform_batch_device(const NttContext* ctx, uint64_t* d_out, const uint64_t* d_g, const uint64_t* d_c, size_t batch,
                                       size_t r, size_t c_rows, uint64_t offdiag, void* stream) LSR_NOEXCEPT;

/* ---------------- NTT: operator-norm-bounded ring challenges ---------------- */
/* The challenges of a LaBRADOR/Greyhound-style argument, drawn on the device: elements with kappa1
 * coefficients +-1 and kappa2 coefficients +-2 whose operator norm — the largest |c(zeta)| over the complex roots zeta of the ring's
 * modulus polynomial — is at most T, which is what makes ||c s|| <= T ||s|| hold.  Integer code that reads q, n and the ring of the
 * context: every arithmetic flavour, negacyclic and cyclic contexts, n <= LSR_RING_OPNORM_MAX_DEGREE.
 *
 * The fixed-point operator norm.  A float comparison against T is not reproducible between a device, a model and a verifier on
 * another machine, so the norm is an integer function.  Table: C[j] = round(2^30 cos(pi j / n)), 0 <= j < 2n, int32 (no entry is
 * within 2.6e-4 of a rounding tie for any power of two n <= 4096: double-precision cos of any honest libm reproduces it).  For an
 * element with centred coefficients c_i and an exponent e: Re_e = sum_i c_i C[(i e) mod 2n], Im_e = sum_i c_i C[(i e - n/2) mod 2n];
 *   N(c) = max over e in E of Re_e^2 + Im_e^2, an unsigned 128-bit integer in units of 2^-60;
 *   E = {2k + 1 : 0 <= k < n/2} on a negacyclic context, {2k : 0 <= k <= n/2} on a cyclic one: one representative per conjugate
 *   pair of the ring's complex embeddings.
 * "||c||_op <= T" MEANS N(c) <= T^2 2^60.  sqrt(N(c)) / 2^30 differs from the true operator norm by at most sqrt(2) ||c||_1 2^-31
 * (every table entry is off by at most 1/2, in Re and in Im), which is below n max|c_i| 2^-30.5.
 *
 * lsr_ring_opnorm_table: the table of degree n into out[2n].  Host only, no device needed.  -1 for a NULL out or an n that is not a
 *   power of two in [2, LSR_RING_OPNORM_MAX_DEGREE].
 * lsr_ntt_ring_opnorm_batch(_device): x [count][n] canonical residues, out [count][2]: N(c) as low word, high word (the layout of
 *   lsr_ntt_ring_l2sq_batch).  An element's output is all ones (both words) if it holds a word >= q or a centred coefficient above
 *   2^15 in magnitude: that bound keeps every Re and Im inside int64 (2^12 2^15 2^30 = 2^57), the products are 32 x 32 + 64
 *   multiply-adds.  Refusals (-1 and lsr_last_error naming the entry point, before any device work), in this order: (1) NULL
 *   context or buffer; (2) a context with n above LSR_RING_OPNORM_MAX_DEGREE.  (3) Then count == 0 is a no-op that returns 0.  Then
 *   (4) a size that overflows size_t; out overlapping x; no visible device.
 * lsr_ntt_ring_opnorm_prepare: builds the table on the host, uploads it once and caches it in the context (2n words, freed with
 *   it).  lsr_ntt_ring_opnorm_batch(_device), and lsr_ntt_ring_challenge_batch(_device) with opnorm_bound != 0, do this themselves
 *   on first use, SYNCHRONOUSLY (an allocation and a blocking copy, refused on a capturing stream).  After it the _device forms
 *   enqueue one kernel and allocate nothing: they can be captured into a HIP graph.  Refuses NULL, n above the limit, no device.
 *
 * lsr_ntt_ring_challenge_batch(_device): out [count][n] canonical residues (1, 2, q - 1, q - 2 and 0), tries int32 [count].
 * Keys, components, domain, index_base and streams exactly as "seeded ring sampling" above: element e uses key
 * keys[4 (e / components) ..] and stream index index_base + (e % components); device-resident SHA3 digests are valid keys.
 *   Candidate of attempt t = 0, 1, ...: LSR_RING_SAMPLE_BALL's inside-out shuffle with kappa = kappa1 + kappa2 steps, read from
 *     the element's stream at word offset t LSR_RING_CHALLENGE_ATTEMPT_WORDS.  c = 0; for s = 0 .. kappa-1: i = n - kappa + s,
 *     j = draw(i + 1; word t 2^18 + a kappa + s for a = 0, 1, ...; U = 63); c[i] = c[j]; then c[j] = +-(s < kappa2 ? 2 : 1), minus
 *     when bit 63 of word t 2^18 + s is set.  Uniform over the elements with exactly kappa1 coefficients +-1 and kappa2
 *     coefficients +-2.  With kappa <= n <= 4096 an attempt's word indices stay below 2^18 past its offset, and with max_tries <=
 *     LSR_RING_CHALLENGE_MAX_TRIES all word indices stay below 2^28.
 *   Acceptance.  opnorm_bound == 0: attempt 0 is taken, tries[e] = 1; with kappa2 == 0 the output is word for word
 *     LSR_RING_SAMPLE_BALL with kappa = kappa1.  Otherwise (T = opnorm_bound): the first attempt t < max_tries with N(c) <=
 *     T^2 2^60 is written and tries[e] = t + 1.
 *   No attempt passes: the element is written as zeros and tries[e] = 0 — the caller re-keys.  At LaBRADOR's parameters (n = 64,
 *     kappa1 = 31, kappa2 = 10, T = 15) a candidate passes with probability about 0.177 (20 000 samples of the model), so
 *     max_tries = 256 fails with probability about 0.823^256, about 2^-72.
 * Like the sampling above this is NOT constant-time, and need not be: challenges are public.
 * Refusals (-1 and lsr_last_error naming the entry point, before any device work), in this order: (1) NULL context, buffer, tries
 * or keys; (2) components == 0; (3) kappa1 + kappa2 == 0 or above n; (4) kappa2 > 0 with q < 5; (5) max_tries == 0 or above
 * LSR_RING_CHALLENGE_MAX_TRIES; (6) opnorm_bound >= 2^32; (7) a context with n above LSR_RING_OPNORM_MAX_DEGREE.  (8) Then
 * count == 0 is a no-op that returns 0.  Then (9) index_base + components overflowing 64 bits; no visible device. */
#define LSR_RING_OPNORM_MAX_DEGREE 4096
#define LSR_RING_CHALLENGE_ATTEMPT_WORDS 262144
#define LSR_RING_CHALLENGE_MAX_TRIES 1024
int lsr_ring_opnorm_table(uint32_t n, int32_t* out) LSR_NOEXCEPT;
int lsr_ntt_ring_opnorm_prepare(const NttContext* ctx) LSR_NOEXCEPT;
int lsr_ntt_ring_opnorm_batch(const NttContext* ctx, const uint64_t* x, size_t count, uint64_t* out) LSR_NOEXCEPT;
int lsr_ntt_ring_opnorm_batch_device(const NttContext* ctx, const uint64_t* d_x, size_t count, uint64_t* d_out, void* stream) LSR_NOEXCEPT;
int lsr_ntt_ring_challenge_batch(const NttContext* ctx, uint64_t* out, int32_t* tries, size_t count, uint32_t kappa1, uint32_t kappa2,
                                 uint64_t opnorm_bound, uint32_t max_tries, const uint64_t* keys, size_t components, uint32_t domain,
                                 uint64_t index_base) LSR_NOEXCEPT;
int lsr_ntt_ring_challenge_batch_device(const NttContext* ctx, uint64_t* d_out, int32_t* d_tries, size_t count, uint32_t kappa1,
                                        uint32_t kappa2, uint64_t opnorm_bound, uint32_t max_tries, const uint64_t* d_keys,
                                        size_t components, uint32_t domain, uint64_t index_base, void* stream) LSR_NOEXCEPT;

/* ---------------- NTT: bit-packed ring elements ---------------- */
/* lsr_ntt_ring_pack_batch(_device), lsr_ntt_ring_unpack_batch(_device): the bytes of a proof message from short ring elements and
 * back — base-2^b digits of lsr_ntt_ring_decompose_batch (whose range [-B/2, B/2 - 1] is exactly that of a
 * b-bit two's-complement field), folded witnesses with a known l-infinity bound, ternary and BALL elements (2 bits), uniform
 * elements (bitlen(q - 1) bits) — instead of one 64-bit word per coefficient.
 *
 * An element is n coefficients x[0..n) of a context (canonical residues, natural order).
 * `bits` lies in [1, 63]; `mode` is one of two new macros.
 *
 * - `LSR_RING_PACK_CENTRED` (0):
 *   - v = x if x <= (q-1)/2, else x - q, which is `ring_linf`'s centring.
 *   - v is *in range* iff -2^(bits-1) <= v <= 2^(bits-1) - 1.
 *   - The field is v mod 2^bits, in two's complement.
 * - `LSR_RING_PACK_RESIDUE` (1):
 *   - x is in range iff x < 2^bits.
 *   - The field is the low `bits` bits of x.
 * - Stream:
 *   - Bit b of field i is bit i*bits + b of the element's bit stream.
 *   - Stream bit t is bit t mod 64 of word floor(t/64).
 *   - An element occupies W = ceil(n*bits/64) words; `size_t lsr_ring_pack_words(uint32_t n, unsigned bits)` returns W on the host,
 *     and 0 for bits outside [1, 63].
 *   - Bits from n*bits upward in the last word are zero. That can only happen at n < 64; for n >= 64 the packed elements are
 *     contiguous with no padding.
 * - **pack**: x [count][n] -> out [count][W], status [count] (int32).
 *   - status = -1 if some word of the element is >= q. This outranks everything, as in `ring_project`.
 *   - status = 0 if none is >= q but some coefficient is out of range.
 *   - status = 1 otherwise.
 *   - Whatever the status, every field is the low `bits` bits of v (CENTRED) or of x (RESIDUE); for a word >= q it is the low bits
 *     of the word itself.
 *   - The output is therefore defined for every input, an element spread over many workgroups needs no second pass, and other
 *     elements are unaffected.
 * - **unpack**: in [count][W] -> out [count][n], status [count].
 *   - CENTRED: sign-extend the field to v. It is valid iff |v| <= (q-1)/2, and the word is v or q + v.
 *   - RESIDUE: the field f is valid iff f < q, and the word is f.
 *   - An invalid field writes the word 0 and makes the status 0.
 *   - A non-zero padding bit makes the status 0. Otherwise the status is 1.
 *   - A status-1 decode is the unique preimage: pack(unpack(w)) = w and unpack(pack(x)) = x with both statuses 1. This uniqueness
 *     is what a Fiat-Shamir verifier needs.
 *   - Every word of `out` is below q, whatever came in.
 * - `unsigned lsr_ring_pack_min_bits(uint64_t q, int mode, uint64_t bound)`, host only.
 *   - CENTRED: it returns the smallest number of bits whose range holds every |v| <= bound, which is bitlen(bound) + 1 for
 *     bound >= 1.
 *   - RESIDUE: it returns bitlen(bound).
 *   - It returns 0 if that exceeds 63, or if bound is 0 or above (q-1)/2 (CENTRED) or q-1 (RESIDUE).
 *
 * The calls read only q and n of a context, like lsr_ntt_ring_sample_batch and lsr_ntt_ring_l2sq_batch: one integer code path
 * serves negacyclic and cyclic contexts, every arithmetic flavour and every ring degree (2 .. 2^22), 64-bit moduli included (the
 * centring compares are unsigned).
 * Refusals (-1 and lsr_last_error naming the entry point, before any device work), in this order: (1) NULL context, buffer or
 * status; (2) unknown mode, or bits outside [1, 63].  (3) Then count == 0 is a no-op that returns 0.  Then (4) count * n or
 * count * W (or their bytes) overflowing size_t; the output overlapping the input, the output overlapping status, status overlapping
 * the input; a word buffer that is not 8-byte aligned or a status that is not 4-byte aligned; (5) no visible device.  (1), (2) and
 * the overflow check read nothing of the context but its degree.
 *
 * The _device forms only enqueue kernels, in plain stream order: no workspace, nothing allocated, no event, no part in the
 * context's ring ordering; they can be captured into a HIP graph from the first call.  Pack at n >= 64: a workgroup owns a tile of
 * LSR_RING_PACK_TILE coefficients (two per lane with 16-byte loads) when x is 16-byte aligned, half as many (one per lane) when it
 * is not; the tile's fields are staged in LDS and leave as coalesced 8-byte stores of whole output words.  Unpack at n >= 64 stages
 * the tile's stream words in LDS and stores two words per lane (16 bytes) when out is 16-byte aligned.  Where an element spans several workgroups (n above the tile) a kernel first sets
 * the statuses to 1 and the workgroups lower them with atomicMin; smaller elements get their status written directly.
 * The plain forms take host buffers and return when out and status are complete: whole elements go through bounded device chunks
 * on the context's work stream; pack uploads words and downloads only packed words and statuses, unpack is the reverse. */
#define LSR_RING_PACK_CENTRED 0
#define LSR_RING_PACK_RESIDUE 1
#define LSR_RING_PACK_TILE 512
size_t lsr_ring_pack_words(uint32_t n, unsigned bits) LSR_NOEXCEPT;
unsigned lsr_ring_pack_min_bits(uint64_t q, int mode, uint64_t bound) LSR_NOEXCEPT;
int lsr_ntt_ring_pack_batch(const NttContext* ctx, uint64_t* out, int32_t* status, const uint64_t* x, size_t count, int mode,
                            unsigned bits) LSR_NOEXCEPT;
int lsr_ntt_ring_pack_batch_device(const NttContext* ctx, uint64_t* d_out, int32_t* d_status, const uint64_t* d_x, size_t count, int mode,
                                   unsigned bits, void* stream) LSR_NOEXCEPT;
int lsr_ntt_ring_unpack_batch(const NttContext* ctx, uint64_t* out, int32_t* status, const uint64_t* in, size_t count, int mode,
                              unsigned bits) LSR_NOEXCEPT;
int lsr_ntt_ring_unpack_batch_device(const NttContext* ctx, uint64_t* d_out, int32_t* d_status, const uint64_t* d_in, size_t count,
                                     int mode, unsigned bits, void* stream) LSR_NOEXCEPT;

/* ---------------- NTT: ring products under any modulus (two NTT primes and CRT) ---------------- */
/* An NttContext exists only for a prime q = 1 (mod 2n).  An LsrRingMod is "the ring Z_q[X]/(X^n + 1)" for ANY q >= 2 — a prime
 * = 5 (mod 8), Kyber's 3329 at n = 256, a power of two — as long as the products fit the two primes below.
 *
 * - Primes: p1, p2 are the two 44-bit NTT primes of an RNS commitment context of the same n (lsr_rns_commit_moduli): p1 the default
 *   commitment modulus for n, p2 the largest 44-bit prime = 1 (mod 2n) other than p1; both in (2^43, 2^44), P = p1 p2.
 *   lsr_ring_mod_primes(n, primes) reports them on the host (0, or -1 when n is no power of two in [2, 131072]).  The handle owns
 *   one ordinary negacyclic context per prime; lsr_ring_mod_prime_context(h, i), i in {0, 1}, lends it (NULL otherwise; never free it).
 * - Centred representative (the toolkit's convention): for x in [0, q), v = x if x <= floor(q/2), else x - q.  With h = floor(q/2),
 *   |v| <= h.
 * - Capacity: max_terms = floor(((P - 1)/2) / (n h^2)) (128-bit host arithmetic, saturated at SIZE_MAX).  A sum of `terms`
 *   products of ring elements has coefficients of magnitude at most terms n h^2, so up to max_terms it is recovered exactly from its
 *   residues mod P.  lsr_ring_mod_capacity(q, n) computes it without a device; lsr_ring_mod_max_terms(h) reads it (0 on NULL).
 * - Admissible (q, n): q >= 2, n a power of two in [2, 131072], the two primes exist, max_terms >= 1 (capacity returns 0 otherwise).
 *   Then h < 2^43 < p_i: the residue of v mod p_i is v, or v + p_i for a negative v.  lsr_ring_mod_create refuses everything else
 *   (NULL and lsr_last_error naming the rule).  lsr_ring_mod_free is NULL-safe and waits for the handle's pending work.
 *
 * The two streaming kernels, at every n the handle admits, device buffers, asynchronous on `stream`:
 * - lsr_ring_mod_lift_batch_device(h, i, d_out, d_x, count): words mod q (count words: any number of polynomials) -> canonical
 *   residues mod p_i of their centred representatives.  d_out may be d_x itself.
 * - lsr_ring_mod_reduce_batch_device(h, d_out, d_r0, d_r1, count, accumulate): for residues r0 < p1, r1 < p2, X is the unique
 *   integer in [-(P-1)/2, (P-1)/2] with those residues; the output is X mod q in [0, q), or with accumulate != 0 that value added
 *   mod q to the word d_out holds (which is below q).  d_out may be d_r0 or d_r1 itself.
 * Both are one pass with 16-byte accesses per lane where every buffer is 16-byte aligned (8-byte ones otherwise), use no workspace,
 * take no part in any ordering and can be captured into a HIP graph from the first call.  Refusals, in this order: NULL handle or
 * buffer; (lift) i outside {0, 1}; then count == 0 is a no-op that returns 0; then count * 8 overflowing size_t, a buffer that is
 * not 8-byte aligned, an output that overlaps an operand without being it; no visible device.
 *
 * Composition.  Together with lsr_ring_mod_prime_context these two calls put every bilinear call of the toolkit under q at EVERY n
 * the handle admits: lift the operands for prime 0 and for prime 1, run the call on each prime's context, reduce the two results.
 * That covers lsr_ntt_ring_mul_batch, lsr_ntt_ring_dot_batch, lsr_ntt_ring_fold_batch, lsr_ntt_ring_matvec_batch,
 * lsr_ntt_ring_gram_batch, lsr_ntt_ring_gram_sym2_batch and lsr_ntt_ring_dot_galois_batch.  The caller keeps ONE bound: the number of
 * products summed per output must not exceed max_terms (a gram_sym2 entry sums two).  Longer sums are split by the caller and the
 * parts reduced with `accumulate`.  At n <= 4096 each of these has a fused call on the handle (mul, dot and dot_galois here; matvec,
 * gram and fold in the sections below) and the composed route is only the way above 4096.  The calls that are not bilinear — sampling,
 * norms, projections, automorphisms, digits, packing — need no primes at all: they run on the handle's coefficient context, below.
 *
 * The fused calls, n <= 4096:
 *   c_j = a_j b_j (mul) and c_j = sum_{i < terms} a_{j,i} b_{j,i} (dot) in Z_q[X]/(X^n + 1), canonical; inputs in [0, q).
 * Shapes, b_rows in {1, batch} and the host-staged plain forms are those of lsr_ntt_ring_mul_batch and lsr_ntt_ring_dot_batch; mul's c
 * may alias a or b exactly, dot's c may not overlap an operand.  One launch per prime of a tile kernel that centres and re-bases
 * the operands as it loads them — the lifted operands never exist in memory — then one reduce launch.  A shared b (b_rows == 1,
 * batch > 1) is lifted and transformed once per prime.  terms above max_terms are taken in groups of at most max_terms, each reduced
 * with accumulate: exactness never depends on the caller knowing the capacity.
 * Refusals (-1 and lsr_last_error, before any device work), in this order: NULL handle or buffer; b_rows not in {1, batch}; (dot)
 * terms == 0.  Then batch == 0 is a no-op that returns 0.  Then: n above 4096 (the message names the composed route above); terms
 * above LSR_RING_DOT_MAX_TERMS; sizes overflowing size_t; c overlapping an operand; no visible device.
 * Workspace, ordering and graph capture: the workspace belongs to the handle, its size depends on n alone and lsr_ring_mod_create
 * allocates it, so the _device forms capture into a HIP graph from the first call.  The batch is taken in chunks.  Calls on one
 * handle are ordered by an event of the handle's own (as a context's ring calls are); a captured call is not bracketed.
 *
 * The twisted inner product, n <= 4096:
 *   lsr_ring_mod_dot_galois_batch(h, c, a, b, batch, terms, b_rows, g):  c_j = sum_{i < terms} sigma_g(a_{j,i}) b_{j,i} in
 *   Z_q[X]/(X^n + 1), canonical, sigma_g: X -> X^g for odd g < 2n.  Every output equals lsr_ring_mod_dot_batch on the materialised
 *   sigma_g(a) word for word; g = 1 is lsr_ring_mod_dot_batch.  With g = 2n - 1 coefficient 0 of c_j is <a_j, b_j> mod q, the inner
 *   product of the coefficient vectors.  The tile kernel of dot fetches the words of a through the permutation before it lifts them;
 *   sigma_g only permutes and negates centred coefficients, so the capacity is max_terms unchanged and the terms go in the same groups.
 *   Shapes, b_rows, the host-staged form, workspace, ordering and graph capture are those of lsr_ring_mod_dot_batch.  Refusals, in this
 *   order: NULL handle or buffer; b_rows not in {1, batch}; terms == 0; g even.  Then batch == 0 is a no-op that returns 0.  Then:
 *   g >= 2n; n above 4096 (the message names the composed route: lift, lsr_ntt_ring_dot_galois_batch_device on each prime context,
 *   reduce); terms above LSR_RING_DOT_MAX_TERMS; sizes overflowing size_t; c overlapping an operand; no visible device.
 *
 * The coefficient context:
 *   lsr_ring_mod_coeff_context(h) lends an NttContext of (q, n) that is negacyclic and has NO twiddle tables (NULL on a NULL handle).
 *   The handle creates it in lsr_ring_mod_create and frees it with itself: never free it (ntt_context_free on it does nothing).  Its
 *   flavour follows lsr_set_arith_mode like any context's (every admissible q is below 2^45: FP64 by default).
 *   Accessors: lsr_ntt_context_device the device, lsr_ntt_context_root 0, lsr_ntt_context_uses_f64 the flavour, lsr_ntt_handoff_bytes 8,
 *   lsr_ntt_context_is_cyclic 0.
 *   SERVED on it, host and _device forms, signatures and contracts unchanged, exact for every admissible q (even, 2, 3, the largest
 *   the handle admits), centred by the convention above: lsr_ntt_ring_sample_batch, lsr_ntt_ring_challenge_batch,
 *   lsr_ntt_ring_opnorm_batch, lsr_ntt_ring_opnorm_prepare, lsr_ntt_ring_pack_batch, lsr_ntt_ring_unpack_batch,
 *   lsr_ntt_ring_decompose_batch, lsr_ntt_ring_recompose_batch, lsr_ntt_ring_linf_batch, lsr_ntt_ring_automorphism_batch,
 *   lsr_ntt_ring_l2sq_batch, lsr_ntt_ring_project_batch, lsr_ntt_ring_project_matrix_batch, lsr_ntt_ring_project_adjoint_batch,
 *   lsr_ntt_ring_scalar_combine_batch, and the word-by-word products mod q ntt_mul_pointwise, ntt_mul_pointwise_batch,
 *   lsr_ntt_mul_pointwise_device (they run no transform).
 *   REFUSED on it: every other function that takes an NttContext (or an array of them) — ntt_forward, ntt_inverse, ntt_forward_batch,
 *   ntt_inverse_batch, lsr_ntt_forward_batch_device, lsr_ntt_inverse_batch_device, lsr_ntt_forward_batch_sharded,
 *   lsr_ntt_inverse_batch_sharded, lsr_cyclic_ntt_forward_batch, lsr_cyclic_ntt_inverse_batch, lsr_ntt_ring_matrix_create_seeded,
 *   lsr_ntt_ring_gram_block, and with their _device forms lsr_ntt_ring_mul_batch, lsr_ntt_ring_dot_batch, lsr_ntt_ring_fold_batch,
 *   lsr_ntt_ring_dot_galois_batch, lsr_ntt_ring_matrix_create, lsr_ntt_ring_gram_batch, lsr_ntt_ring_gram_sym2_batch,
 *   lsr_ntt_ring_quadform_batch.  Each returns -1, NULL or 0 according to its type; lsr_last_error names the
 *   entry point, contains "coefficient context" and names the lsr_ring_mod_* call to use where one exists.  The refusal is the first
 *   check after the context's own NULL check: it precedes every look at a buffer (a sharded call looks at its `shards` contexts). */
typedef struct LsrRingMod LsrRingMod;
LsrRingMod* lsr_ring_mod_create(uint64_t q, uint32_t n, int device) LSR_NOEXCEPT;
void lsr_ring_mod_free(LsrRingMod* h) LSR_NOEXCEPT;
uint64_t lsr_ring_mod_modulus(const LsrRingMod* h) LSR_NOEXCEPT;
const NttContext* lsr_ring_mod_prime_context(const LsrRingMod* h, int i) LSR_NOEXCEPT;
size_t lsr_ring_mod_max_terms(const LsrRingMod* h) LSR_NOEXCEPT;
const NttContext* lsr_ring_mod_coeff_context(const LsrRingMod* h) LSR_NOEXCEPT;
int lsr_ring_mod_primes(uint32_t n, uint64_t primes[2]) LSR_NOEXCEPT;
size_t lsr_ring_mod_capacity(uint64_t q, uint32_t n) LSR_NOEXCEPT;
int lsr_ring_mod_lift_batch_device(const LsrRingMod* h, int i, uint64_t* d_out, const uint64_t* d_x, size_t count, void* stream) LSR_NOEXCEPT;
int lsr_ring_mod_reduce_batch_device(const LsrRingMod* h, uint64_t* d_out, const uint64_t* d_r0, const uint64_t* d_r1, size_t count,
                                     int accumulate, void* stream) LSR_NOEXCEPT;
int lsr_ring_mod_mul_batch(const LsrRingMod* h, uint64_t* c, const uint64_t* a, const uint64_t* b, size_t batch, size_t b_rows) LSR_NOEXCEPT;
int lsr_ring_mod_mul_batch_device(const LsrRingMod* h, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t b_rows,
                                  void* stream) LSR_NOEXCEPT;
int lsr_ring_mod_dot_batch(const LsrRingMod* h, uint64_t* c, const uint64_t* a, const uint64_t* b, size_t batch, size_t terms,
                           size_t b_rows) LSR_NOEXCEPT;
int lsr_ring_mod_dot_batch_device(const LsrRingMod* h, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t batch, size_t terms,
                                  size_t b_rows, void* stream) LSR_NOEXCEPT;
int lsr_ring_mod_dot_galois_batch(const LsrRingMod* h, uint64_t* c, const uint64_t* a, const uint64_t* b, size_t batch, size_t terms,
                                  size_t b_rows, uint64_t g) LSR_NOEXCEPT;
int lsr_ring_mod_dot_galois_batch_device(const LsrRingMod* h, uint64_t* d_c, const uint64_t* d_a, const uint64_t* d_b, size_t batch,
                                         size_t terms, size_t b_rows, uint64_t g, void* stream) LSR_NOEXCEPT;

/* ---------------- NTT: resident matrices under any modulus (y = M x and y = M G^-1(x) on a ring handle) ---------------- */
/* The module product with a public matrix — an Ajtai commitment t = A s, Kyber's A s, a commitment to the digits of a long witness —
 * in Z_q[X]/(X^n + 1) for the q of an LsrRingMod, n <= 4096.  Every output is exact and canonical in [0, q).
 *
 * Capacity with a short operand (host only):
 *   lsr_ring_mod_capacity_bounded(q, n, bound) = floor(((P - 1)/2) / (n floor(q/2) bound))
 * counts the negacyclic products of one operand of centred magnitude <= floor(q/2) and one of magnitude <= bound that one sum may
 * hold.  128-bit host arithmetic, saturated at SIZE_MAX as lsr_ring_mod_capacity; 0 for bound == 0, for bound > floor(q/2) and
 * wherever lsr_ring_mod_capacity(q, n) is 0; lsr_ring_mod_capacity_bounded(q, n, floor(q/2)) == lsr_ring_mod_capacity(q, n).
 *
 * The matrix.  m is [rows][cols][n], words in [0, q).  The handle keeps two device copies: for each prime the forward transform (the
 * order the context's transform writes) of the lifted entries.  Lifetime and ownership are lsr_ntt_ring_matrix_create's: create
 * copies (the host form is complete on return, the device form enqueues on `stream` and later calls on other streams start behind
 * it), the matrix is immutable, the handle h must outlive it, lsr_ring_mod_matrix_free is NULL-safe and waits for the matrix's ready
 * event and for the handle's pending work; _rows, _cols and _row_block return 0 on NULL (_row_block: the rows of M one workgroup
 * keeps in registers, that of the prime contexts' kernels).
 * lsr_ring_mod_matrix_create_seeded: entry M[r][c] is the UNIFORM element of lsr_ntt_ring_sample_batch's definition with modulus q,
 * one key and stream index index_base + r cols + c, sampled on the device; the handle is indistinguishable from _create_device of
 * those words.  Complete on return.
 * Limits: rows in [1, LSR_RING_MATVEC_MAX_ROWS], cols in [1, LSR_RING_DOT_MAX_TERMS], rows cols n 8 <= LSR_RING_MATVEC_MAX_MATRIX_BYTES
 * per prime.
 * Refusals of create (NULL and lsr_last_error naming the entry point, before any device work), in this order: NULL h or m / key;
 * rows == 0; cols == 0; rows above its cap; cols above its cap; rows cols 16 above the byte cap; n above 4096 (the message names
 * the composed route: lift M per prime, lsr_ntt_ring_matrix_create_device on lsr_ring_mod_prime_context, lift x, two
 * lsr_ntt_ring_matvec_batch_device, reduce, with the columns in groups of max_terms); rows cols n 8 above the byte cap; (seeded)
 * index_base + rows cols overflowing 64 bits; no visible device.
 *
 * The products.
 *   lsr_ring_mod_matvec_batch:        x [batch][cols][n], y [batch][rows][n]:  y[j][r] = sum_c M[r][c] x[j][c] in R_q — word for word
 *                                     lsr_ring_mod_dot_batch(h, ., x, M[r], batch, cols, 1) row by row.
 *   lsr_ring_mod_matvec_gadget_batch: x [batch][xcols][n] with xcols digits == cols:  y = M G^-1(x), G^-1 as defined under "gadget
 *                                     decomposition" above, taken against q: the centred word against floor(q/2), the offset off, digit
 *                                     z_d in [-B/2, B/2 - 1], matrix column xc digits + d <- digit d of x[.][xc].  Word for word the
 *                                     plain product on the decomposed vector, which never exists in memory.  (b, D) must be admissible
 *                                     for q by the rule stated there; lsr_ring_gadget_min_digits(q, b) answers it for any q.
 * Grouping rule: matrix columns are taken in groups, each reduced into y with accumulate from the second on — at most max_terms
 * columns per group for the plain product, at most lsr_ring_mod_capacity_bounded(q, n, B/2) for the gadget product (a digit's
 * magnitude is at most B/2); a gadget group may end between two digits of one column of x.  Exactness never depends on the caller
 * knowing either capacity.
 * Refusals of the products (-1 and lsr_last_error, before any device work), in this order: NULL mat or buffer; (gadget) base_log2
 * outside [2, 32], digits == 0 or base_log2 digits > 64; (gadget) (b, D) not admissible for q; (gadget) cols % digits != 0.  Then
 * batch == 0 is a no-op that returns 0.  Then: y overlapping x in address range; no visible device.
 * The plain forms take host buffers through bounded device chunks on the first prime context's work stream and return when y is
 * complete; the _device forms enqueue only.  Workspace, ordering and graph capture are the fused products': no allocation after
 * create (the per-prime sums go to the handle's workspace in chunks of whole vectors or, where rows n exceeds 2^22 words, of one
 * vector and a range of rows), calls on one handle are ordered by the handle's event, a captured call is not bracketed and the
 * _device forms capture into a HIP graph from the first call.
 *
 * The bounded product: the plain product with a bound on x that the device VERIFIES — the commitment t = A s
 * and the verifier's A z, whose operand is short by construction.
 *   lsr_ring_mod_matvec_bounded_batch: x [batch][cols][n], y [batch][rows][n], status [batch] (int32), never NULL.
 * bound_x is the l-infinity bound the caller asserts on the centred representatives of x; 0 states none, which is floor(q/2): then
 * only -1 can occur and the call is the plain product with a canonicity check.  status is written for every vector, with the values
 * and the precedence of the Gram and fold calls below:
 *    1   every one of the cols n words of x[j] was below q and within the bound: y[j] equals lsr_ring_mod_matvec_batch on the same
 *        operands word for word, canonical in [0, q);
 *    0   some word's centred magnitude exceeded the bound;
 *   -1   some word was >= q (-1 wins over 0).
 * For a status 0 or -1 EVERY word of y[j] is 0; the other vectors of the batch are unaffected.
 * Grouping rule: matrix columns are taken in groups of at most lsr_ring_mod_capacity_bounded(q, n, bound_x) (0 -> floor(q/2), which
 * gives max_terms), every group after the first reduced into y with accumulate: q = 2^40 + 15 at n = 64 takes 258 columns in 37
 * groups unbounded and in one with x declared within 128.  Exactness never depends on the caller knowing the capacity — the bound is
 * verified, not promised.  A violation found in a later group still leaves y[j] all zero.
 * Refusals (-1 and lsr_last_error naming the entry point, before any device work), in this order: (1) NULL mat, y, status or x;
 * (2) bound_x above floor(q/2).  (3) Then batch == 0 is a no-op that returns 0.  Then (4) y overlapping x; (5) status overlapping
 * x, then y, in address range; (6) no visible device.
 * Range: n <= 4096, as the matrix handle itself.
 * Workspace, ordering and graph capture are the plain product's: the per-vector flag words are the 4096 32-bit words behind the
 * handle's workspace, which lsr_ring_mod_create allocates, so they exist before lsr_ring_mod_matrix_create returns; a chunk of
 * whole vectors is capped at 4096 vectors by them.  The _device form allocates nothing, is ordered by the handle's mutex and event
 * and captures into a HIP graph from the first call; the plain form takes host buffers through bounded device chunks, status staged
 * alongside y, and returns when both are complete.
 * The bounded inner product with a per-output b is lsr_ring_mod_fold_batch at width = 1, term_stride = terms (out[j] = sum_i
 * p[j][i] v[j terms + i]); lsr_ring_mod_dot_batch takes no bound. */
typedef struct LsrRingModMatrix LsrRingModMatrix;
size_t lsr_ring_mod_capacity_bounded(uint64_t q, uint32_t n, uint64_t bound) LSR_NOEXCEPT;
LsrRingModMatrix* lsr_ring_mod_matrix_create(const LsrRingMod* h, const uint64_t* m, size_t rows, size_t cols) LSR_NOEXCEPT;
LsrRingModMatrix* lsr_ring_mod_matrix_create_device(const LsrRingMod* h, const uint64_t* d_m, size_t rows, size_t cols, void* stream) LSR_NOEXCEPT;
LsrRingModMatrix* lsr_ring_mod_matrix_create_seeded(const LsrRingMod* h, const uint64_t key[4], uint32_t domain, uint64_t index_base, size_t rows,
                                                    size_t cols) LSR_NOEXCEPT;
void lsr_ring_mod_matrix_free(LsrRingModMatrix* mat) LSR_NOEXCEPT;
size_t lsr_ring_mod_matrix_rows(const LsrRingModMatrix* mat) LSR_NOEXCEPT;
size_t lsr_ring_mod_matrix_cols(const LsrRingModMatrix* mat) LSR_NOEXCEPT;
size_t lsr_ring_mod_matrix_row_block(const LsrRingModMatrix* mat) LSR_NOEXCEPT;
int lsr_ring_mod_matvec_batch(const LsrRingModMatrix* mat, uint64_t* y, const uint64_t* x, size_t batch) LSR_NOEXCEPT;
int lsr_ring_mod_matvec_batch_device(const LsrRingModMatrix* mat, uint64_t* d_y, const uint64_t* d_x, size_t batch, void* stream) LSR_NOEXCEPT;
int lsr_ring_mod_matvec_gadget_batch(const LsrRingModMatrix* mat, uint64_t* y, const uint64_t* x, size_t batch, unsigned base_log2,
                                     size_t digits) LSR_NOEXCEPT;
int lsr_ring_mod_matvec_gadget_batch_device(const LsrRingModMatrix* mat, uint64_t* d_y, const uint64_t* d_x, size_t batch, unsigned base_log2,
                                            size_t digits, void* stream) LSR_NOEXCEPT;
int lsr_ring_mod_matvec_bounded_batch(const LsrRingModMatrix* mat, uint64_t* y, int32_t* status, const uint64_t* x, size_t batch,
                                      uint64_t bound_x) LSR_NOEXCEPT;
int lsr_ring_mod_matvec_bounded_batch_device(const LsrRingModMatrix* mat, uint64_t* d_y, int32_t* d_status, const uint64_t* d_x, size_t batch,
                                             uint64_t bound_x, void* stream) LSR_NOEXCEPT;

/* ---------------- NTT: Gram matrices under any modulus (bounded ring vectors on a ring handle) ---------------- */
/* The garbage polynomials of a lattice argument — g_il = <s_i, s_l>, h_il = <phi_i, s_l> + <phi_l, s_i> — in Z_q[X]/(X^n + 1) for the
 * q of an LsrRingMod, at every n the handle admits.  Shapes, packed layouts, limits and the three forms are those of
 * lsr_ntt_ring_gram_batch and lsr_ntt_ring_gram_sym2_batch: a [batch][ra][width][n], b [batch][rb][width][n], g [batch][ra][rb][n]
 * (cross); b == NULL: the packed upper triangle of a with itself, g [batch][r (r + 1) / 2][n] (symmetric, rb == ra); sym2: the
 * symmetrised packed form of two families.  Limits: LSR_RING_GRAM_MAX_VECTORS, LSR_RING_DOT_MAX_TERMS, LSR_RING_GRAM_MAX_FAMILY_BYTES.
 * The ring is negacyclic.  Every operand polynomial is lifted and transformed once per prime.
 *
 * Definition.  Every output word equals lsr_ring_mod_dot_batch on (a[j][i], b[j][l]) pair by pair — for sym2 the sum of two such
 * results mod q — canonical in [0, q); inputs in [0, q).
 *
 * Capacity with two short operands (host only):
 *   lsr_ring_mod_capacity_product(q, n, bound_a, bound_b) = floor(((P - 1)/2) / (n bound_a bound_b))
 * counts the negacyclic products of an operand of centred magnitude <= bound_a and one of magnitude <= bound_b that one sum may hold.
 * 128-bit host arithmetic, saturated at SIZE_MAX; 0 when a bound is 0, when a bound is above floor(q/2) and wherever
 * lsr_ring_mod_capacity(q, n) is 0.  With h = floor(q/2): capacity_product(q, n, h, bound) == lsr_ring_mod_capacity_bounded(q, n, bound)
 * and capacity_product(q, n, h, h) == lsr_ring_mod_capacity(q, n).
 *
 * Bounds.  bound_a and bound_b are the l-infinity bounds the caller asserts on the centred representatives of a and of b; 0 states
 * none, which is floor(q/2).  The symmetric form (b == NULL) does not read bound_b and holds a against bound_a twice.  In the cross
 * form with b == a the same words are held against both bounds.  The device VERIFIES the bounds:
 * status is [batch] (int32), never NULL, and written for every family:
 *    1   every operand word of family j was below q and within its bound: the family's outputs are exact;
 *    0   some word's centred magnitude exceeded its bound;
 *   -1   some word was >= q (-1 wins over 0).
 * For a status 0 or -1 EVERY output word of that family is 0; the other families of the batch are unaffected.  With both bounds none
 * only -1 can occur.
 *
 * Grouping rule: columns are taken in groups of at most capacity_product(q, n, bound_a, bound_b) (the symmetric form: bound_a twice;
 * sym2: half of it, rounded down — an entry sums two products per column), every group after the first reduced into g with
 * accumulate.  Exactness never depends on the caller knowing a capacity.
 *
 * Refusals (-1 and lsr_last_error, before any device work), in this order: NULL handle, g, status, a (sym2: or b); ra, width (b: rb)
 * == 0; b == NULL with rb != ra; ra or rb above LSR_RING_GRAM_MAX_VECTORS; width above LSR_RING_DOT_MAX_TERMS; sizes overflowing
 * size_t; a bound above floor(q/2) (bound_b only where b is read).  Then batch == 0 is a no-op that returns 0.  Then: one family's
 * operands or outputs above LSR_RING_GRAM_MAX_FAMILY_BYTES; a family that does not fit the workspace even one column at a time
 * (vectors + outputs polynomials per prime); sym2 where capacity_product is below 2 (the message names the cross form; q =
 * 8246337208321 at n = 8 is such a ring); g or status overlapping an operand or each other; no visible device.
 *
 * Workspace, ordering and graph capture.  The workspace belongs to the handle: per prime max(2^23, LAMBDA_SNARK_NTT_CHUNK_MIB 2^20 / 32)
 * 64-bit words — 2^23 words, 64 MiB, at the default chunk size of 256 MiB; a function of the process-wide chunk size alone — and
 * 2^15 words of per-family flags behind the two halves.  A chunk of whole families holds, per prime, the families' lifted operands,
 * and their outputs ((vectors width + outputs) n words a family); a family that does not fit, or whose width exceeds the capacity, is
 * taken alone in column groups.  The first eager Gram call or lsr_ring_mod_gram_prepare(h) allocates it; it is never resized and
 * lsr_ring_mod_free releases it; lsr_ring_mod_create allocates nothing for it.  A _device call on a capturing stream that finds it
 * missing is refused (the message asks for one eager call first) and leaves the handle usable; after _prepare the _device forms
 * capture into a HIP graph from the first call.  Calls on one handle are ordered by the handle's mutex and event; a captured call is
 * not bracketed.  The plain forms take host buffers through bounded device chunks of whole families on the first prime context's
 * work stream and return when g and status are complete; the _device forms enqueue only. */
size_t lsr_ring_mod_capacity_product(uint64_t q, uint32_t n, uint64_t bound_a, uint64_t bound_b) LSR_NOEXCEPT;
int lsr_ring_mod_gram_prepare(const LsrRingMod* h) LSR_NOEXCEPT;
int lsr_ring_mod_gram_batch(const LsrRingMod* h, uint64_t* g, int32_t* status, const uint64_t* a, const uint64_t* b, size_t batch, size_t ra,
                            size_t rb, size_t width, uint64_t bound_a, uint64_t bound_b) LSR_NOEXCEPT;
int lsr_ring_mod_gram_batch_device(const LsrRingMod* h, uint64_t* d_g, int32_t* d_status, const uint64_t* d_a, const uint64_t* d_b, size_t batch,
                                   size_t ra, size_t rb, size_t width, uint64_t bound_a, uint64_t bound_b, void* stream) LSR_NOEXCEPT;
int lsr_ring_mod_gram_sym2_batch(const LsrRingMod* h, uint64_t* out, int32_t* status, const uint64_t* a, const uint64_t* b, size_t batch, size_t r,
                                 size_t width, uint64_t bound_a, uint64_t bound_b) LSR_NOEXCEPT;
int lsr_ring_mod_gram_sym2_batch_device(const LsrRingMod* h, uint64_t* d_out, int32_t* d_status, const uint64_t* d_a, const uint64_t* d_b,
                                        size_t batch, size_t r, size_t width, uint64_t bound_a, uint64_t bound_b, void* stream) LSR_NOEXCEPT;

/* ---------------- NTT: fold under any modulus (ring vectors by ring-valued challenges on a ring handle) ---------------- */
/* The fold z_j = sum_i c_{j,i} s_{j term_stride + i} of a lattice argument — the prover's fold of the witness, the verifier's fold of
 * the commitments — in Z_q[X]/(X^n + 1) for the q of an LsrRingMod, n <= 4096:
 *   out[j][c] = sum_{i < terms} p[j][i] * v[j term_stride + i][c].
 * Shapes, layouts and term_stride (0, terms, or anything else) are those of lsr_ntt_ring_fold_batch: v [vectors][width][n] with
 * vectors = (outputs - 1) term_stride + terms, p [outputs][terms][n], out [outputs][width][n].  The ring is negacyclic.
 *
 * Definition.  Every output polynomial out[j][c] equals lsr_ring_mod_dot_batch on the gathered operands a_i = v[j term_stride + i][c],
 * b_i = p[j][i], word for word: canonical in [0, q); inputs in [0, q); a challenge's -1 is q - 1.
 * Limits: terms <= LSR_RING_DOT_MAX_TERMS, width <= LSR_RING_FOLD_MAX_WIDTH.
 *
 * Bounds and status: those of the Gram matrices above.  bound_v and bound_p are the l-infinity bounds the caller asserts on the
 * centred representatives of v and of p; 0 states none, which is floor(q/2).  The device VERIFIES them: status is [outputs] (int32),
 * never NULL, and written for every output:
 *    1   every word output j reads — the terms width n words of its term vectors and the terms n words of p[j] — was below q and
 *        within its bound: out[j] is exact;
 *    0   some such word's centred magnitude exceeded its bound;
 *   -1   some such word was >= q (-1 wins over 0).
 * For a status 0 or -1 EVERY word of out[j] is 0; the other outputs are unaffected.  With term_stride == 0 every output reads the same
 * vectors, so a bad word in v gates every output, while a bad word in p[j] gates output j alone.
 *
 * Grouping rule: terms are taken in groups of at most lsr_ring_mod_capacity_product(q, n, bound_v, bound_p) (0 -> floor(q/2)), every
 * group after the first reduced into out with accumulate.  Exactness never depends on the caller knowing a capacity: q = 2^40 + 15 at
 * n = 64 carries 7 unbounded products and 2199021131876 with the challenges declared within 2.  A violation found in a later group
 * still leaves out[j] all zero.
 *
 * Range: n <= 4096, as lsr_ring_mod_dot_batch.  Above it the call is refused and the message names the composed route: lift v and p
 * per prime, lsr_ntt_ring_fold_batch_device on lsr_ring_mod_prime_context(h, i), reduce, the terms in groups of max_terms.
 *
 * Refusals (-1 and lsr_last_error naming the entry point, before any device work), in this order: (1) NULL handle, out, status, v or
 * p; (2) terms == 0.  (3) Then outputs == 0 or width == 0 is a no-op that returns 0.  Then (4) terms above LSR_RING_DOT_MAX_TERMS;
 * (5) width above LSR_RING_FOLD_MAX_WIDTH; (6) a size that overflows size_t, as lsr_ntt_ring_fold_batch lists them; (7) a bound above
 * floor(q/2); (8) n above 4096; (9) the byte size of v, p or out overflowing size_t at the handle's n; (10) out overlapping v, then
 * p, status overlapping v, p, then out, in address range; (11) no visible device.
 *
 * Workspace, ordering and graph capture.  The workspace is the handle's own, the one of the fused products with the per-output flag
 * words behind it: its size depends on n alone and lsr_ring_mod_create allocates it — there is no _prepare — so the _device form
 * enqueues only and captures into a HIP graph from the first call, without a hidden allocation.  Per prime it holds 2^22 words of
 * sums and min(4096, 2^21 / n) challenge transforms: outputs are taken in chunks of whole outputs that fit both (an output of more
 * than 2^22 / n components alone, its components in chunks).  Calls on one handle are ordered by the handle's mutex and event; a
 * captured call is not bracketed.  The plain form takes host buffers through bounded device chunks on the first prime context's work
 * stream — whole outputs together with the span of vectors they read, each operand within LAMBDA_SNARK_STAGING_MIB where one output's
 * is (a shared v, term_stride == 0, goes up once) — and returns when out and status are complete. */
int lsr_ring_mod_fold_batch(const LsrRingMod* h, uint64_t* out, int32_t* status, const uint64_t* v, const uint64_t* p, size_t outputs, size_t terms,
                            size_t term_stride, size_t width, uint64_t bound_v, uint64_t bound_p) LSR_NOEXCEPT;
int lsr_ring_mod_fold_batch_device(const LsrRingMod* h, uint64_t* d_out, int32_t* d_status, const uint64_t* d_v, const uint64_t* d_p, size_t outputs,
                                   size_t terms, size_t term_stride, size_t width, uint64_t bound_v, uint64_t bound_p, void* stream) LSR_NOEXCEPT;

/* ---------------- NTT: quadratic forms under any modulus (a packed Gram triangle in ring-valued challenges on a ring handle) -------- */
/* The verifier's closing equations of a lattice argument — <z, z> = sum g_il c_i c_l and sum_i <phi_i, z> c_i = sum h_il c_i c_l — in
 * Z_q[X]/(X^n + 1) for the q of an LsrRingMod, at every n the handle admits.  This is the call to take where
 * lsr_ntt_ring_quadform_batch is refused on the handle's coefficient context.  Shapes are those of lsr_ntt_ring_quadform_batch: g
 * [batch][r (r + 1) / 2][n] in the packed order lsr_ring_mod_gram_batch (b == NULL) and lsr_ring_mod_gram_sym2_batch write, c
 * [c_rows][r][n] with c_rows == batch or 1 (one set of challenges for every family), out [batch][n], status [batch].  The ring is
 * negacyclic.  Limits: r <= LSR_RING_GRAM_MAX_VECTORS, one family's g <= LSR_RING_GRAM_MAX_FAMILY_BYTES.
 *
 * Definition.  out[j] = sum_i g[j][(i,i)] c_i c_i + offdiag * sum_{i < l} g[j][(i,l)] c_i c_l in Z_q[X]/(X^n + 1): canonical in
 * [0, q), exact, and independent of the kernel flavour and of how the call slices, groups and chunks its work; inputs in [0, q).
 * Word for word it is lsr_ring_mod_mul_batch on every pair (c_i, c_l), the off-diagonal products scaled by offdiag mod q, and
 * lsr_ring_mod_dot_batch of the r (r + 1) / 2 products against g[j].  offdiag is a word below q — 2 for a lsr_ring_mod_gram_batch(s),
 * 1 for a lsr_ring_mod_gram_sym2_batch(phi, s) — and acts through its centred representative w: the kernels multiply by the residues
 * of w mod p1 and mod p2.  g and c are never written.
 *
 * Capacity of a cubic sum (host only).  The form is CUBIC in its operands, so neither max_terms nor lsr_ring_mod_capacity_product,
 * which count bilinear products, cover it:
 *   lsr_ring_mod_capacity_quadform(q, n, bound_g, bound_c) = floor(((P - 1)/2) / (n^2 bound_g bound_c^2))
 * counts the triple negacyclic products g c c' of operands of centred magnitude |g| <= bound_g and |c|, |c'| <= bound_c that one sum
 * may hold.  A bound of 0 states none, which is floor(q/2); 0 for a bound above floor(q/2) and wherever lsr_ring_mod_capacity(q, n) is
 * 0; saturated at SIZE_MAX.  (The divisor can exceed 128 bits: (P - 1)/2 is divided by n, n, bound_g, bound_c, bound_c in turn.)
 * q = 4294967197 at n = 64 carries 0 such products of unbounded operands and 4398042366208 with the challenges declared within 2.
 *
 * Bounds and status: those of the Gram matrices above.  bound_g and bound_c are the l-infinity bounds the caller asserts on the
 * centred representatives of g and of c; 0 states none.  The device VERIFIES them: status is [batch] (int32), never NULL, and written
 * for every family:
 *    1   every word family j reads — its g[j] and the c it takes — was below q and within its bound: out[j] is exact;
 *    0   some such word's centred magnitude exceeded its bound;
 *   -1   some such word was >= q (-1 wins over 0).
 * For a status 0 or -1 EVERY word of out[j] is 0.  With c_rows == 1 every family reads the same c, so a bad word in c gates every
 * family, while a bad word in g[j] gates family j alone.
 *
 * Grouping rule: with W = max(1, |w|), the packed pairs are taken in runs of the packed order of at most
 * floor(lsr_ring_mod_capacity_quadform(q, n, bound_g, bound_c) / W) pairs (the workspace may cut the runs shorter); every group goes
 * all the way to out — inverse transform, CRT, reduction mod q — and every group after the first is added to out mod q.  A violation
 * found in a later group still leaves out[j] all zero.  Where not even one pair fits — unbounded challenges at any modulus of 32 bits
 * or more, an offdiag such as (q + 1)/2 at a large q — the call is refused before any device work; the message names bound_c and the
 * route that always works because it reduces mod q between the two products: lsr_ring_mod_mul_batch per pair, a scaling by offdiag,
 * lsr_ring_mod_dot_batch.
 *
 * Refusals (-1 and lsr_last_error naming the entry point, before any device work), in this order: (1) NULL h, out, status, g or c;
 * (2) r == 0; (3) c_rows neither 1 nor batch; (4) r above LSR_RING_GRAM_MAX_VECTORS; (5) a size that overflows size_t, as
 * lsr_ntt_ring_quadform_batch lists them; (6) offdiag >= q; (7) a bound above floor(q/2).  (8) Then batch == 0 is a no-op that returns
 * 0.  Then (9) one family's g above LSR_RING_GRAM_MAX_FAMILY_BYTES; (10) the capacity refusal above; (11) r + 3 polynomials per prime
 * (the transformed c of one family, one of g, one partial sum, one sum) not fitting the workspace — the message names
 * LAMBDA_SNARK_NTT_CHUNK_MIB, which sizes it (at the present limits no call reaches this one: a prime's half holds at least 64
 * polynomials at n = 131072, and a family of r >= 62 there is above LSR_RING_GRAM_MAX_FAMILY_BYTES); (12) out overlapping g, then c, status overlapping g, c, then out, in address range;
 * (13) no visible device; (14) a capturing stream with the workspace not yet allocated (the message asks for one eager call first;
 * the handle stays usable).
 *
 * Workspace, ordering and graph capture: the Gram matrices' — the handle's Gram workspace and its flag words, allocated by the first
 * eager Gram or quadratic-form call or by lsr_ring_mod_gram_prepare(h), never resized; there is no workspace of this call's own.  A chunk
 * of whole families holds, per prime, the transformed c (r polynomials a family, or r once when shared: a shared c is lifted, checked
 * and transformed once per call), a group of transformed g, the slices' partial sums and one sum a family.  After _prepare the _device
 * form captures into a HIP graph from the first call (one chain of kernels).  Calls on one handle are ordered by the handle's mutex
 * and event; a captured call is not bracketed.  The plain form takes host buffers through bounded device chunks of whole families on
 * the first prime context's work stream (a shared c goes up once) and returns when out and status are complete; the _device form
 * enqueues only. */
size_t lsr_ring_mod_capacity_quadform(uint64_t q, uint32_t n, uint64_t bound_g, uint64_t bound_c) LSR_NOEXCEPT;
int lsr_ring_mod_quadform_batch(const LsrRingMod* h, uint64_t* out, int32_t* status, const uint64_t* g, const uint64_t* c, size_t batch, size_t r,
                                size_t c_rows, uint64_t offdiag, uint64_t bound_g, uint64_t bound_c) LSR_NOEXCEPT;
int lsr_ring_mod_quadform_batch_device(const LsrRingMod* h, uint64_t* d_out, int32_t* d_status, const uint64_t* d_g, const uint64_t* d_c, size_t batch,
                                       size_t r, size_t c_rows, uint64_t offdiag, uint64_t bound_g, uint64_t bound_c, void* stream) LSR_NOEXCEPT;

/* ---------------- NTT: responses under any modulus (z = y + sum c s with a verified abort on a ring handle) ---------------- */
/* The masked response of a Fiat-Shamir-with-aborts protocol — z = y + c s, accepted only where its l-infinity norm stays within
 * gamma - beta and thrown away otherwise — in Z_q[X]/(X^n + 1) for the q of an LsrRingMod, n <= 4096:
 *   z[j][c] = y[j][c] + sum_{i < terms} p[j][i] * v[j term_stride + i][c].
 * Shapes, layouts, term_stride rules and limits are those of lsr_ring_mod_fold_batch above: v [vectors][width][n], p
 * [outputs][terms][n], out [outputs][width][n], status [outputs]; y is [outputs][width][n] of canonical words, or NULL for no mask.
 *
 * Definition.  Let f be what lsr_ring_mod_fold_batch writes for the same v, p, term_stride, bound_v and bound_p.  Then
 * z[j] = (f[j] + y[j]) mod q word for word, and the status of output j, [outputs] (int32), never NULL and written for every output, is
 *   -1   some word output j reads — those of the fold and the width n words of y[j] — was >= q;
 *    0   some such word's centred magnitude exceeded bound_v, bound_p or bound_y;
 *    2   LSR_RING_RESPOND_REJECTED: the inputs were fine, but the centred magnitude of some word of z[j] exceeds bound_z.  This is
 *        the abort: the caller restarts that instance;
 *    1   accepted: out[j] = z[j].
 * -1 wins over 0, 0 wins over 2, 2 wins over 1.  For every status other than 1 EVERY word of out[j] is 0 when the call completes;
 * the other outputs are unaffected.  That holds too where the offending word is met in a later group of terms or a later chunk of
 * components.  (The handle's workspace still holds the residues of the product until the next call on the handle: the promise is
 * about out.)
 *
 * Bounds: l-infinity bounds on centred representatives, inclusive; 0 for any of them states none, which is floor(q/2), so
 * bound_z == 0 never rejects.  With y == NULL and bound_z == 0 the call equals lsr_ring_mod_fold_batch word for word, status
 * included.  The norm held against bound_z is that of the representative of z centred mod q, in (-q/2, q/2]: it is the norm of the
 * INTEGER y + sum c s whenever bound_y + terms n bound_v bound_p < q/2, and a caller that needs the integer norm declares bounds
 * that say so.
 *
 * In place: y may be exactly out (sample the mask into the output buffer, then respond).  Any other overlap of out with y, v or p,
 * and any overlap of status with anything, is refused.
 *
 * Grouping rule: the fold's — terms in groups of at most lsr_ring_mod_capacity_product(q, n, bound_v, bound_p), y added once, with
 * the first group, and the norm judged on the finished sum alone.
 *
 * Range: n <= 4096.  Above it the call is refused and the message names the composed route: the fold's composed route, then an add
 * mod q and lsr_ntt_ring_linf_batch_device on lsr_ring_mod_coeff_context(h).
 *
 * Refusals (-1 and lsr_last_error naming the entry point, before any device work; they read only q and n of the handle), in the
 * fold's order: (1) NULL handle, out, status, v or p; (2) terms == 0.  (3) Then outputs == 0 or width == 0 is a no-op that returns 0.
 * Then (4) terms above LSR_RING_DOT_MAX_TERMS; (5) width above LSR_RING_FOLD_MAX_WIDTH; (6) a size that overflows size_t; (7) a NULL y
 * with bound_y != 0, then any of the four bounds above floor(q/2) — the message names all four; (8) n above 4096; (9) the byte size
 * of v, p or out overflowing size_t at the handle's n; (10) out overlapping y (unless y == out), v, then p, status overlapping y, v,
 * p, then out, in address range; (11) no visible device.
 *
 * Workspace, ordering and graph capture: the fold's.  The handle's own workspace and flag words, nothing allocated, there is no
 * _prepare; the _device form enqueues only and captures into a HIP graph as the first call on a fresh handle; calls on one handle are
 * ordered by its mutex and event, and a captured call is not bracketed.  The plain form takes host buffers through bounded device
 * chunks of whole outputs within LAMBDA_SNARK_STAGING_MIB, y as one more staged operand (or with out, where it is out), and returns
 * when out and status are complete. */
#define LSR_RING_RESPOND_REJECTED 2
int lsr_ring_mod_respond_batch(const LsrRingMod* h, uint64_t* out, int32_t* status, const uint64_t* y, const uint64_t* v, const uint64_t* p,
                               size_t outputs, size_t terms, size_t term_stride, size_t width, uint64_t bound_y, uint64_t bound_v,
                               uint64_t bound_p, uint64_t bound_z) LSR_NOEXCEPT;
int lsr_ring_mod_respond_batch_device(const LsrRingMod* h, uint64_t* d_out, int32_t* d_status, const uint64_t* d_y, const uint64_t* d_v,
                                      const uint64_t* d_p, size_t outputs, size_t terms, size_t term_stride, size_t width, uint64_t bound_y,
                                      uint64_t bound_v, uint64_t bound_p, uint64_t bound_z, void* stream) LSR_NOEXCEPT;

/* ---------------- Gaussian sampler: seeded / device ---------------- */
/* sample i of object (seed, domain, index) uses ChaCha20 stream word i (low bit: sign; upper 63 bits: the uniform
 * value compared with the CDT table at 63-bit precision);
 * output = two's-complement int64 like sample_gaussian. Host buffer. */
int lsr_sample_gaussian_seeded(uint64_t* output, size_t len, double sigma, uint64_t seed, uint32_t domain,
                               uint64_t index) LSR_NOEXCEPT;
/* CDT table exactly as cpp-core/src/utils.cpp:26-75 (host long double); returns entry count or 0 */
size_t lsr_gaussian_cdf(double sigma, uint64_t* cdf, size_t cap) LSR_NOEXCEPT;

/* ---------------- commitment: seeded contexts, batches, the metric workload ---------------- */
/* lwe_context_create with an explicit key seed and device (-1 = default).  key_seed != 0: every key of the context is
 * derived from it — reproducible contexts for tests and for replicating ONE context on several devices; such a context is
 * only as secret as the 64-bit seed.  key_seed == 0: 256-bit OS entropy, exactly lwe_context_create. */
LweContext* lsr_lwe_context_create_seeded(const PublicParams* params, uint64_t key_seed, int device) LSR_NOEXCEPT;
/* The modulus to put into PublicParams.modulus for a context whose lwe_linear_combine has the reference's range
 * (commitment.cpp:88-96,247-266: any coefficient below the plaintext modulus): the largest 60-bit prime = 1 (mod 2 ring_degree).
 * A default context (any modulus no transform can use: 2^44 + 1, 12289 ...) commits under a 44-bit prime on the FP64 kernels and
 * refuses combinations whose centred coefficients sum beyond ~800 (noise budget); under the 60-bit prime the bound is ~2^25 and
 * the u64 Harvey/Shoup kernels run (about 1.5x the time per transform).  0 for an unsupported ring_degree. */
uint64_t lsr_lwe_wide_modulus(uint32_t ring_degree) LSR_NOEXCEPT;
/* Two-prime RNS context: the reference's lwe_linear_combine range (any coefficient below t, over any realistic number of terms) on
 * the FP64 kernels.  The context commits under Q = q1 q2 (about 2^88) and keeps every commitment as its residues mod q1 and q2:
 *   q1 = what a default context picks for ring_degree (17592169062401 up to 4096, else the largest 44-bit prime = 1 mod 2n),
 *   q2 = the largest 44-bit prime = 1 (mod 2 ring_degree) other than q1;  t = lsr_plain_modulus(ring_degree), unchanged.
 * params->modulus is IGNORED (as a default context ignores a modulus no transform can use).  Keys, context id and the per-commitment
 * stream keys are derived exactly as by lsr_lwe_context_create_seeded (key_seed == 0: one draw of OS entropy); r, e1, e2 of a
 * commitment are sampled once and are the same integers under both primes:
 *   u_i = INTT_qi(A_i^T NTT_qi(r)) + e1,   v_i = INTT_qi(<b_i, NTT_qi(r)>) + e2 + (round(Q (m mod t) / t) mod q_i).
 * Wire row (lsr_lwe_commitment_words = 6 + 2 (k + 1) n words): data[0] = payload bytes, then "LSRR0001", n | k<<32, q1, q2, t,
 * u_1[k][n], v_1[n], u_2[k][n], v_2[n].  A single-prime context answers -1 to such a row and an RNS context -1 to a single-prime row.
 * Opening: x_i = v_i - <s, u_i> mod q_i, x = CRT(x_1, x_2) in [0, Q), slot = floor((t x + Q/2) / Q) mod t, compared with the claimed
 * words as given.  lwe_linear_combine enforces sum |c_i| (noise_unit + 1) < Q / 2t (c_i centred mod t), a bound of about 2^67.
 * Served: lwe_commit, lwe_commit_batch, lsr_lwe_commit_batch_flat(_device), lsr_lwe_commit_keys(_device), lsr_lwe_commit_rows_device,
 * lwe_verify_opening(_batch), lsr_lwe_verify_opening_batch_flat, lsr_lwe_verify_rows_device, lwe_linear_combine, the free calls and
 * the size / rank getters; lsr_lwe_modulus returns q1; lsr_lwe_pipeline "rns-tile" (ring_degree 4096, rank <= 4, sigma <= ~6.9: one
 * launch per batch, one workgroup per commitment or opening) or "rns-general".  Refused with -1 / NULL and a message in lsr_last_error:
 * lsr_mlwe_matvec_batch_device, lsr_lwe_sample_blinding_device, lsr_lwe_public_matrix, lsr_lwe_ntt_context,
 * lsr_lwe_context_replicate, every *_sharded call, and the provers / lsr_simple_verify_batch* when handed such a context.
 * NULL (message in lsr_last_error) for any (ring_degree, module_rank, sigma) a default context refuses, and without a device. */
LweContext* lsr_lwe_context_create_rns(const PublicParams* params, uint64_t key_seed, int device) LSR_NOEXCEPT;
/* out = {q1, q2} of an RNS context, 0; -1 on any other context */
int lsr_lwe_rns_moduli(const LweContext* ctx, uint64_t out[2]) LSR_NOEXCEPT;
/* the same pair from the ring degree alone (host only, no device needed); -1 for an unsupported ring_degree */
int lsr_rns_commit_moduli(uint32_t ring_degree, uint64_t out[2]) LSR_NOEXCEPT;
uint64_t lsr_lwe_modulus(const LweContext* ctx) LSR_NOEXCEPT;         /* internal q actually used */
uint64_t lsr_lwe_plain_modulus(const LweContext* ctx) LSR_NOEXCEPT;   /* t */
uint32_t lsr_lwe_ring_degree(const LweContext* ctx) LSR_NOEXCEPT;
uint32_t lsr_lwe_module_rank(const LweContext* ctx) LSR_NOEXCEPT;
size_t   lsr_lwe_commitment_words(const LweContext* ctx) LSR_NOEXCEPT; /* LweCommitment.len */
const NttContext* lsr_lwe_ntt_context(const LweContext* ctx) LSR_NOEXCEPT;
/* copy the public matrix A_hat ([k][k][n], NTT domain) to a host buffer */
int lsr_lwe_public_matrix(const LweContext* ctx, uint64_t* a_hat) LSR_NOEXCEPT;

/* `batch` commitments in one device pass.  messages = [batch][msg_len]; seeds[batch] (0 = fresh; semantics of lwe_commit);
 * out[batch] receives commitments to be freed with lwe_commitment_free.  0 / -1. */
int lwe_commit_batch(LweContext* ctx, const uint64_t* messages, size_t msg_len, size_t batch,
                     const uint64_t* seeds, LweCommitment** out) LSR_NOEXCEPT;

/* The same `batch` commitments written back to back into ONE caller-owned host array
 * out_words[batch][lsr_lwe_commitment_words(ctx)] — row i holds exactly the words lwe_commit_batch would put in
 * out[i]->data (data[0] = payload byte length, commitment.cpp:44-60) — with no per-commitment allocation: the rows are
 * assembled on the device and come back in one copy.  0 / -1. */
int lsr_lwe_commit_batch_flat(LweContext* ctx, const uint64_t* messages, size_t msg_len, size_t batch,
                              const uint64_t* seeds, uint64_t* out_words) LSR_NOEXCEPT;
/* The same with the rows left in DEVICE memory d_out_words[batch][lsr_lwe_commitment_words(ctx)] on the context's device
 * (messages and seeds are still host arrays); returns after the rows are complete.  For chaining with
 * lsr_fs_challenge_batch_device before the rows travel to the host. */
int lsr_lwe_commit_batch_flat_device(LweContext* ctx, const uint64_t* messages, size_t msg_len, size_t batch,
                                     const uint64_t* seeds, uint64_t* d_out_words) LSR_NOEXCEPT;

/* Whole commitments without a byte of host traffic (round 3): the batched, device-resident form of lwe_commit
 * (cpp-core/src/commitment.cpp:138-164, contract cpp-core/include/lambda_snark/commitment.h:43-63) and of lwe_verify_opening
 * (commitment.cpp:200-232, commitment.h:80-99).  lsr_lwe_commit_keys derives, on the host, the per-commitment
 * 256-bit stream keys exactly as lwe_commit does (seed != 0: PRF of seed, context id and embedded message; seed == 0: fresh OS
 * entropy) into out_keys[batch][4]; lsr_lwe_commit_rows_device then turns DEVICE arrays d_keys[batch][4] and
 * d_messages[batch][msg_len] into the wire rows d_rows[batch][lsr_lwe_commitment_words(ctx)] — word for word what
 * lsr_lwe_commit_batch_flat returns for the same keys — asynchronously on `stream`.  Contexts with ring_degree 4096 (FP64
 * flavour, rank <= 4, sigma <= ~6.9) run it as ONE launch with one workgroup per commitment: r, e1, e2 are sampled in the
 * lanes, transformed and multiplied in LDS, and only the finished row is written; ring_degree 2^16 / 2^17 sample inside the
 * strided transform rounds (three launches per chunk).  lsr_lwe_pipeline names the path a context takes: "tile", "fused",
 * "fused-matvec" (only the matrix-vector workload is fused), "general"; "rns-tile" / "rns-general" on an RNS context.
 * Calls on one context are ordered one behind the other (each waits for the previous call's last kernel), whatever streams the
 * caller passes; the synchronous entry points of the same context (lwe_commit, lwe_verify_opening, lwe_linear_combine, the batch
 * and sharded calls) and lwe_context_free wait for a pending asynchronous call before they touch the context's workspaces.
 * Results are ready when `stream` has drained.  0 / -1.
 * lsr_lwe_commit_keys_device derives the same keys ON THE DEVICE from device-resident messages (seeds: a HOST array, every seed
 * non-zero — seed 0 means fresh OS entropy, which only the host call can serve: -1), asynchronously on `stream`: the host
 * derivation hashes every embedded message word (about 10 us per full-length message at n = 4096 on one core), which for long
 * messages costs several times what the commitments themselves take on the GPU. */
int lsr_lwe_commit_keys(const LweContext* ctx, const uint64_t* messages, size_t msg_len, size_t batch, const uint64_t* seeds,
                        uint64_t* out_keys) LSR_NOEXCEPT;
int lsr_lwe_commit_keys_device(LweContext* ctx, const uint64_t* d_messages, size_t msg_len, size_t batch, const uint64_t* seeds,
                               uint64_t* d_keys, void* stream) LSR_NOEXCEPT;
int lsr_lwe_commit_rows_device(LweContext* ctx, const uint64_t* d_messages, size_t msg_len, size_t batch,
                               const uint64_t* d_keys, uint64_t* d_rows, void* stream) LSR_NOEXCEPT;
/* `count` openings of device-resident rows against device-resident claimed messages (1 <= msg_len <= ring_degree):
 * d_results[i] = 1 / 0 / -1 with the meaning of lwe_verify_opening.  Asynchronous on `stream`.  0 / -1. */
int lsr_lwe_verify_rows_device(const LweContext* ctx, const uint64_t* d_rows, const uint64_t* d_messages, size_t msg_len,
                               size_t count, int* d_results, void* stream) LSR_NOEXCEPT;
const char* lsr_lwe_pipeline(const LweContext* ctx) LSR_NOEXCEPT;

/* ---------------- commitment: decoding rows, with the measured noise ----------------
 * What a row opens to, and how much decoding headroom it has left — for callers that fold rows with lwe_linear_combine and would
 * otherwise recompute the expected message on the side, and for combinations of already combined rows, whose depth the budget
 * check of lwe_linear_combine cannot see (it assumes fresh inputs; the wire row carries no weight).
 * Definitions.  x_i = the i-th coefficient of v - <s, u> mod q (RNS context: the CRT lift of the two residues into [0, Q); read
 * Q for q below).  With h = floor(q/2):
 *   N_i   = t x_i + h = s_i q + rem_i,   0 <= rem_i < q,   s_i in [0, t]
 *   slot  = (s_i == t ? 0 : s_i)                    bit for bit the value lwe_verify_opening compares with the claimed word
 *   rho_i = |rem_i - h| = |t x_i - s_i q| <= h      t times the distance of x_i from the nearest plaintext lattice point, exact
 *   noise_bits = bitlen(max_i rho_i) over ALL ring_degree coefficients (0 when the maximum is 0)
 * A row stops decoding to its message when noise_bits reaches lsr_lwe_noise_capacity_bits = bitlen(h); the headroom of a row is
 * the capacity minus its noise_bits.  Scaling a row by 2^e adds e to its noise_bits.  Fresh commitments at ring_degree 4096, rank 2,
 * sigma 3.19 measure 32 or 33 bits, of a capacity of 43 (default context) or 87 (RNS context).
 *
 * lsr_lwe_decode_rows_device: d_messages[count][slots] = the first `slots` decoded plaintext slots of each device-resident row
 * (1 <= slots <= ring_degree); d_status[count] = 1 (well-formed, decoded) or -1 (wrong header for this context, a residue word >=
 * its modulus, a row of the other kind of context — the screening of lsr_lwe_verify_rows_device): messages and noise of such a row
 * are unspecified, its neighbours are unaffected.  d_noise_bits (may be NULL) [count].  Without it only the first `slots`
 * coefficients of a row are divided; with it all ring_degree are.  Asynchronous on `stream`; ordering behind other calls on the
 * context, workspaces and graph capture exactly as lsr_lwe_verify_rows_device.  Every pipeline lsr_lwe_pipeline names is served.
 * lsr_lwe_decode_batch_flat: the same for host rows words[count][lsr_lwe_commitment_words], staged in the chunks the flat verify uses;
 * returns when the outputs are complete.
 * lsr_lwe_decode: one LweCommitment; returns the status (1 / -1).
 * NULL context or buffer (noise_bits excepted), slots == 0 or > ring_degree: -1 and a message in lsr_last_error, before any device
 * work (without a device there is no context to pass).  count == 0: no-op, 0.  Otherwise 0 / -1.
 * Decoding reveals the message by design; nothing here is meant to be constant-time. */
int lsr_lwe_decode_rows_device(const LweContext* ctx, const uint64_t* d_rows, size_t count, size_t slots,
                               uint64_t* d_messages, int* d_status, uint32_t* d_noise_bits, void* stream) LSR_NOEXCEPT;
int lsr_lwe_decode_batch_flat(const LweContext* ctx, const uint64_t* words, size_t count, size_t slots,
                              uint64_t* messages, int* status, uint32_t* noise_bits) LSR_NOEXCEPT;
int lsr_lwe_decode(const LweContext* ctx, const LweCommitment* cm, uint64_t* message, size_t slots, uint32_t* noise_bits) LSR_NOEXCEPT;
/* bit length of floor(q/2) (RNS: floor(Q/2)); 0 for a NULL context */
uint32_t lsr_lwe_noise_capacity_bits(const LweContext* ctx) LSR_NOEXCEPT;

/* ---------------- commitment: batched linear combination of device-resident rows ----------------
 * lwe_linear_combine for a whole batch, without a host round trip.  With W = lsr_lwe_commitment_words(ctx), output j < outputs is
 *   out_j = sum_{i < terms} c'_{j,i} * row[j * term_stride + i]
 * over the (k + 1) n body residues mod q (RNS context: over both residue blocks, each under its own prime), where c'_{j,i} is the
 * centred representative of d_coeffs[j * terms + i] mod t: a value in (t/2, t) acts as c - t, exactly as in lwe_linear_combine.
 * d_rows holds (outputs - 1) * term_stride + terms rows of W words and is only read.  term_stride = 0 combines one shared set of
 * terms with `outputs` coefficient vectors; term_stride = terms folds disjoint consecutive groups; any other stride is allowed.
 * d_out_rows[outputs][W] must not overlap d_rows.  d_coeffs[outputs][terms] is DEVICE memory (d_alphas of
 * lsr_fs_challenge_batch_device can be passed as it is); coefficients are any 64-bit words, reduced mod t as given.
 * An output row with status 1 is word for word the `data` lwe_linear_combine returns for the same terms and coefficients (header
 * and canonical body residues).
 * d_status[j] =  1  combined;
 *                0  refused for the noise budget: sum_i |c'_{j,i}| exceeds the largest integer weight the comparison of
 *                   lwe_linear_combine accepts on this context (weight (noise_unit + 1) < Delta / 2 in double; RNS: < Q / 2t in long
 *                   double), computed once per call on the host and compared with the kernel's exact integer sum — the decision of
 *                   lwe_linear_combine for that coefficient vector;
 *               -1  some term row of this output is not a canonical row of this context (wrong header, a row of the other kind of
 *                   context, a body residue >= its modulus — the screening of lsr_lwe_verify_rows_device), whatever its coefficient.
 * Rows with status 0 or -1 are unspecified; their neighbours are unaffected.
 * Asynchronous on `stream`; uses no workspace of the context and allocates nothing, so a call can be captured into a HIP graph from
 * the first call on (the status is written by a kernel).  Ordered behind other asynchronous calls on the context exactly as
 * lsr_lwe_verify_rows_device, and waited for by the synchronous entry points.  Every kind of context is served (FP64, u64, RNS).
 * lsr_lwe_combine_batch_flat: the same for host arrays, staged in the bounded chunks the flat verify uses (the terms of one output
 * are never split); returns when the outputs are complete.
 * NULL context or buffer, terms == 0, terms >= 2^32, outputs >= 2^31, a term_stride whose row count overflows: -1 and a message
 * naming the entry point in lsr_last_error, before any device work.  outputs == 0: no-op, 0.  Otherwise 0 / -1.
 * The FP64 kernel canonicalises its accumulators every LSR_COMBINE_TERMS terms; a workgroup serves LSR_COMBINE_OUTPUTS outputs. */
#define LSR_COMBINE_TERMS 32
#define LSR_COMBINE_OUTPUTS 8
int lsr_lwe_combine_rows_device(const LweContext* ctx, const uint64_t* d_rows, size_t terms, size_t term_stride,
                                const uint64_t* d_coeffs, size_t outputs, uint64_t* d_out_rows, int* d_status, void* stream) LSR_NOEXCEPT;
int lsr_lwe_combine_batch_flat(const LweContext* ctx, const uint64_t* rows, size_t terms, size_t term_stride,
                               const uint64_t* coeffs, size_t outputs, uint64_t* out_rows, int* status) LSR_NOEXCEPT;

/* ---------------- commitment: ring-element linear combination of device-resident rows ----------------
 * Folding rows with ring-valued challenges.  With W = lsr_lwe_commitment_words(ctx) and n the ring degree, output j < outputs is
 *   out_j = sum_{i < terms} p'_{j,i}(X) * row[j * term_stride + i]
 * component by component over the k + 1 body polynomials in Z_q[X]/(X^n + 1) (RNS context: over both residue blocks, each under its
 * own prime, with the same integer polynomial p').  d_polys[outputs][terms][n] is DEVICE memory, natural coefficient order; every
 * word is any 64-bit value, reduced mod t as given and centred: c <= (t - 1)/2 acts as c, otherwise as c - t (the rule of
 * lsr_lwe_combine_rows_device per coefficient).  d_rows is only read; term_stride means what it means for
 * lsr_lwe_combine_rows_device (0: shared terms; terms: disjoint groups; anything else allowed).  d_out_rows[outputs][W] must not
 * overlap d_rows or d_polys.  Output rows carry the context's header and canonical body residues.
 * d_status[j] =  1  combined.  The row opens to sum_i p'_{j,i} m_i mod (X^n + 1, t), m_i = the n decoded slots of the term rows;
 *                0  weight_j = sum_i sum_x |p'_{j,i,x}| (an exact integer below 2^52) exceeds lsr_lwe_combine_max_weight(ctx), the
 *                   weight the scalar combine compares against: |(p e)_x| <= ||p||_1 ||e||_inf, and the rounding of round(q m / t)
 *                   adds at most ||p||_1 / 2 (the "+ 1" of noise_unit + 1);
 *               -1  some term row of this output is not a canonical row of this context (the screening of
 *                   lsr_lwe_verify_rows_device).
 * Rows with status 0 or -1 are unspecified; their neighbours are unaffected.  When every polynomial of a call is constant, the call
 * gives the rows and statuses of lsr_lwe_combine_rows_device for the same constants, word for word.
 * Asynchronous on `stream`, ordered behind other asynchronous calls on the context exactly as lsr_lwe_verify_rows_device; the
 * synchronous entry points and lwe_context_free wait for it.  The call needs a workspace for the transformed polynomials, owned by
 * the context: its size depends on (n, k, kind of context) and the process-wide chunk size only, the first eager call that needs it
 * allocates it, and it is never resized.  A CAPTURING call (HIP graph) that would have to allocate the workspace returns -1: make
 * one eager call on the context first (n > 4096: that call also allocates the ring inner product's workspace).  Outputs, and terms
 * where they do not fit, are taken in chunks; between groups of terms the re-centred raw accumulator waits in the output row.
 * lsr_lwe_ring_combine_batch_flat: the same for host arrays, staged in the bounded chunks lsr_lwe_combine_batch_flat uses (the terms
 * of one output go up whole and are split on the device only, in the group form above); returns when the outputs are complete.
 * Every kind of context is served (FP64, u64 wide modulus, RNS; every ring degree a context accepts).
 * NULL context or buffer, terms == 0, terms > LSR_RING_COMBINE_MAX_TERMS, outputs >= 2^31, a row count that overflows, an output
 * overlapping an input: -1 and a message naming the entry point in lsr_last_error, before any device work.  outputs == 0: no-op, 0.
 * lsr_lwe_combine_max_weight: the largest weight either combine accepts on this context; 0 for NULL. */
#define LSR_RING_COMBINE_MAX_TERMS 65536
int lsr_lwe_ring_combine_rows_device(const LweContext* ctx, const uint64_t* d_rows, size_t terms, size_t term_stride,
                                     const uint64_t* d_polys, size_t outputs, uint64_t* d_out_rows, int* d_status, void* stream) LSR_NOEXCEPT;
int lsr_lwe_ring_combine_batch_flat(const LweContext* ctx, const uint64_t* rows, size_t terms, size_t term_stride,
                                    const uint64_t* polys, size_t outputs, uint64_t* out_rows, int* status) LSR_NOEXCEPT;
uint64_t lsr_lwe_combine_max_weight(const LweContext* ctx) LSR_NOEXCEPT;

/* `count` openings in one device pass.  messages = [count][msg_len]; results[i] = 1 / 0 / -1 with the meaning of
 * lwe_verify_opening (cpp-core/src/commitment.cpp:200-232) for (commitments[i], messages[i]); NULL entries => -1.
 * Returns 0, or -1 if the call itself failed. */
int lwe_verify_opening_batch(const LweContext* ctx, const LweCommitment* const* commitments, const uint64_t* messages,
                             size_t msg_len, size_t count, int* results) LSR_NOEXCEPT;
/* The same for `count` commitments stored back to back (rows of lsr_lwe_commit_batch_flat): words[count][lsr_lwe_commitment_words]. */
int lsr_lwe_verify_opening_batch_flat(const LweContext* ctx, const uint64_t* words, const uint64_t* messages,
                                      size_t msg_len, size_t count, int* results) LSR_NOEXCEPT;

/* The Module-LWE matrix–vector workload of BASELINE config 3, device-resident:
 *   u_j = INTT( A_hat^T . NTT(r_j) ) + e1_j   for j < batch;   r, e1, u are [batch][k][n] in [0,q).
 * d_e1 != NULL: the blinding residues are read from it (seeds may be NULL).
 * d_e1 == NULL: e1 is sampled on the device, component i of vector j from the raw-seed stream (seeds[j], domain 5, i)
 *               (key = {seed, "LSR1", "STRM"}: a reproducible workload stream, not a commitment's message-bound key);
 *               `seeds` is then a HOST array of `batch` seeds and the call returns after the work has finished.
 * d_r: contexts that qualify for the fused pipeline (FP64 flavour, n = 2^16 or 2^17, rank <= 4) only read it; otherwise it
 * is overwritten with NTT(r) — treat its contents as unspecified after the call.  0 / -1. */
int lsr_mlwe_matvec_batch_device(const LweContext* ctx, uint64_t* d_r, const uint64_t* d_e1, uint64_t* d_u,
                                 size_t batch, const uint64_t* seeds, void* stream) LSR_NOEXCEPT;

/* Field elements wider than the plaintext modulus t (about 2^20).  lwe_commit embeds every message word mod t — the
 * reference's BatchEncoder takes out-of-range words unchecked and lwe_verify_opening compares the decoded slots with the
 * message words as given (cpp-core/src/commitment.cpp:152,223-226), so there, as here, a word >= t is bound only through
 * its residue and never opens.  A caller that needs a 44- or 64-bit coefficient bound in full commits to its LIMBS:
 * limbs[i * limbs_per_word + l] = (words[i] >> (l * limb_bits)) & (2^limb_bits - 1), e.g. limb_bits = 16, limbs_per_word = 4
 * (64-bit words) or limb_bits = 15, limbs_per_word = 3 (44-bit field); every limb is < t, the message grows by the factor
 * limbs_per_word (<= ring_degree slots in all) and opens word for word.  Returns the number of limbs (count *
 * limbs_per_word; also when `words` or `limbs` is NULL, for sizing), 0 on invalid limb parameters.  Host only. */
size_t lsr_words_to_limbs(const uint64_t* words, size_t count, unsigned limb_bits, unsigned limbs_per_word,
                          uint64_t* limbs) LSR_NOEXCEPT;

/* The blinding residues alone: d_e1[batch][k][n] in [0,q), component i of vector j from the seeded CDT stream
 * (seeds[j], domain 5, i) — exactly what lsr_mlwe_matvec_batch_device samples when d_e1 == NULL.  `seeds` is a HOST
 * array; the call returns after the samples are complete.  0 / -1. */
int lsr_lwe_sample_blinding_device(const LweContext* ctx, uint64_t* d_e1, size_t batch, const uint64_t* seeds,
                                   void* stream) LSR_NOEXCEPT;

/* Synthetic inputs of SURVEY.md section 8(d): d_out[objects][len], element i of object o = the (i+1)-th output of
 * splitmix64 seeded with seed_base + o, reduced mod q (q = 0: the raw 64-bit word).  Asynchronous on `stream`, launched on
 * the calling thread's current HIP device.  0 / -1. */
int lsr_fill_splitmix_device(uint64_t* d_out, size_t objects, size_t len, uint64_t seed_base, uint64_t q,
                             void* stream) LSR_NOEXCEPT;

/* ---------------- several devices of one node inside ONE call (BASELINE config 4) ----------------
 * Independent polynomials / commitments: the batch is cut into `shards` contiguous slices (lsr_shard_bounds: sizes differ
 * by at most one, earlier shards take the extra), shard g is driven by ctxs[g] on ITS device from its own host thread and
 * stream, and every slice of the result is copied device -> host straight into its place in the caller's single array
 * (allocate it with lsr_host_alloc_pinned for full PCIe speed).  No collective, no device-to-device traffic; the shared
 * resource is host PCIe / DRAM bandwidth.  The reference has no counterpart (single-threaded CPU library; its only
 * concurrency statement is `unsafe impl Send`, rust-api/lambda-snark/src/context.rs:76).  The contexts of a call must be
 * distinct objects; several may live on the same device (that is how a one-GPU box exercises this path). */
void  lsr_shard_bounds(size_t batch, int shards, int index, size_t* first, size_t* count) LSR_NOEXCEPT;
void* lsr_host_alloc_pinned(size_t bytes) LSR_NOEXCEPT;     /* NULL on failure */
void  lsr_host_free_pinned(void* p) LSR_NOEXCEPT;
/* the same commitment context (same keys: same A_hat, s, b_hat, context id) on another device; commitments made by either
 * replica verify and combine under the other.  NULL on failure. */
LweContext* lsr_lwe_context_replicate(const LweContext* ctx, int device) LSR_NOEXCEPT;
/* ntt_forward_batch / ntt_inverse_batch over `shards` contexts of the same (q, n): polys is ONE host array [batch][n] */
int lsr_ntt_forward_batch_sharded(const NttContext* const* ctxs, int shards, uint64_t* polys, size_t batch) LSR_NOEXCEPT;
int lsr_ntt_inverse_batch_sharded(const NttContext* const* ctxs, int shards, uint64_t* polys, size_t batch) LSR_NOEXCEPT;
/* lsr_lwe_commit_batch_flat over replicas of one context: host messages [batch][msg_len], seeds [batch] (or NULL), rows
 * written to out_words[batch][lsr_lwe_commitment_words] — bit-identical to the one-device call. */
int lsr_lwe_commit_batch_flat_sharded(LweContext* const* ctxs, int shards, const uint64_t* messages, size_t msg_len,
                                      size_t batch, const uint64_t* seeds, uint64_t* out_words) LSR_NOEXCEPT;
/* The config-4 workload: u_j = INTT(A_hat^T NTT(r_j)) + e1_j with DEVICE-resident inputs per shard and a HOST gather.
 * d_r[g], d_e1[g]: arrays on ctxs[g]'s device holding rows [first_g, first_g + count_g) of the batch ([count_g][k][n]);
 * host_u: one array [batch][k][n].  Each shard works through its slice in pieces: the device -> host copy of one piece runs on
 * a copy stream under the kernels of the next, so a shard takes about max(kernels, gather) plus one piece, not their sum.
 * seconds (optional, 2 doubles): over the shards, [0] the longest kernel time of a slice, [1] the longest wall time until a
 * slice's last byte is in host memory.  _stats: the same two figures for every shard, per_shard[shards][2].  0 / -1. */
int lsr_mlwe_matvec_batch_sharded(LweContext* const* ctxs, int shards, uint64_t* const* d_r, const uint64_t* const* d_e1,
                                  size_t batch, uint64_t* host_u, double* seconds) LSR_NOEXCEPT;
int lsr_mlwe_matvec_batch_sharded_stats(LweContext* const* ctxs, int shards, uint64_t* const* d_r,
                                        const uint64_t* const* d_e1, size_t batch, uint64_t* host_u,
                                        double* per_shard) LSR_NOEXCEPT;

/* ---------------- Fiat–Shamir consumer of the commitment words (host, no GPU needed) ---------------- */
/* The transcript of rust-api/lambda-snark/src/challenge.rs:102-134: SHA3-256 over "LAMBDA-SNARK-R-FS-v1", the
 * public inputs and ALL commitment words (each length-prefixed, little-endian); alpha = LE64(h[0..8]) mod modulus.
 * hash32 may be NULL.  0 / -1. */
int lsr_fs_challenge(const uint64_t* public_inputs, size_t n_inputs, const LweCommitment* commitment, uint64_t modulus,
                     uint64_t* alpha, uint8_t* hash32) LSR_NOEXCEPT;
/* `count` transcripts at once: commitments as rows words[count][words_per_commitment] (lsr_lwe_commit_batch_flat), public
 * inputs [count][n_inputs]; alphas[count], hashes32 (optional) [count][32].  SHA3 is sequential inside a transcript and
 * independent across them: a pool of `threads` host threads (0 = up to 16) shares the rows.  0 / -1. */
int lsr_fs_challenge_batch_flat(const uint64_t* public_inputs, size_t n_inputs, const uint64_t* words,
                                size_t words_per_commitment, size_t count, uint64_t modulus, uint64_t* alphas,
                                uint8_t* hashes32, unsigned threads) LSR_NOEXCEPT;
/* alpha_i = derive(public_inputs_i, row_i), then beta_i = derive([alpha_i], row_i) — the pair every R1CS prover and verifier needs
 * (lib.rs:761-768) — with both transcripts of a row hashed by the same pool thread.  betas [count] is required; hashes_alpha32 and
 * hashes_beta32 (optional) [count][32].  Equal to two lsr_fs_challenge_batch_flat calls.  0 / -1. */
int lsr_fs_challenge_chain_batch_flat(const uint64_t* public_inputs, size_t n_inputs, const uint64_t* words,
                                      size_t words_per_commitment, size_t count, uint64_t modulus, uint64_t* alphas,
                                      uint64_t* betas, uint8_t* hashes_alpha32, uint8_t* hashes_beta32, unsigned threads) LSR_NOEXCEPT;
/* The same on device-resident arrays (8-byte aligned), asynchronous on `stream`: d_words [count][words_per_commitment] (e.g. from
 * lsr_lwe_commit_batch_flat_device), d_public_inputs [count][n_inputs] (may be a previous call's d_alphas with n_inputs = 1),
 * d_alphas [count], d_hashes32 (optional) [count][32].  One kernel launch on the calling thread's current HIP device (where the
 * arrays must live): no allocation, no host synchronisation, capturable into a HIP graph.  Two kernels compute the same words:
 * LANE gives every transcript one lane (a launch costs one transcript's time, flat up to 65 536 of them); WAVE gives it half a
 * wavefront (several times faster for the batches the provers see).  This call picks by lsr_fs_transcript_path.  0 / -1. */
int lsr_fs_challenge_batch_device(const uint64_t* d_public_inputs, size_t n_inputs, const uint64_t* d_words,
                                  size_t words_per_commitment, size_t count, uint64_t modulus, uint64_t* d_alphas,
                                  uint8_t* d_hashes32, void* stream) LSR_NOEXCEPT;
enum { LSR_FS_PATH_AUTO = 0, LSR_FS_PATH_LANE = 1, LSR_FS_PATH_WAVE = 2 };
/* lsr_fs_challenge_batch_device with the kernel chosen by the caller (an unknown `path` is -1). */
int lsr_fs_challenge_batch_device_on(int path, const uint64_t* d_public_inputs, size_t n_inputs, const uint64_t* d_words,
                                     size_t words_per_commitment, size_t count, uint64_t modulus, uint64_t* d_alphas,
                                     uint8_t* d_hashes32, void* stream) LSR_NOEXCEPT;
/* The chained pair on the device: d_alphas and d_betas [count] are both written, the digests are optional.  WAVE is ONE launch
 * (the half-wavefront that found alpha goes on to hash [alpha] || row); LANE is the two launches a caller would chain. */
int lsr_fs_challenge_chain_batch_device(int path, const uint64_t* d_public_inputs, size_t n_inputs, const uint64_t* d_words,
                                        size_t words_per_commitment, size_t count, uint64_t modulus, uint64_t* d_alphas,
                                        uint64_t* d_betas, uint8_t* d_hashes_alpha32, uint8_t* d_hashes_beta32, void* stream) LSR_NOEXCEPT;
/* What AUTO picks for `count` transcripts of `words_per_commitment` words: LSR_FS_PATH_LANE or LSR_FS_PATH_WAVE (host only). */
int lsr_fs_transcript_path(size_t count, size_t words_per_commitment) LSR_NOEXCEPT;

/* ---------------- host-only number theory (usable without a GPU) ---------------- */
uint64_t lsr_minimal_primitive_root(uint64_t q, uint32_t n) LSR_NOEXCEPT;   /* 0 if none */
uint64_t lsr_select_commit_modulus(uint64_t requested_q, uint32_t n) LSR_NOEXCEPT;
uint64_t lsr_plain_modulus(uint32_t n) LSR_NOEXCEPT;                        /* SEAL Batching(n,20) */

#ifdef __cplusplus
}
#endif
