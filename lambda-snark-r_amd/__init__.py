"""Host-side mirror of the reference's safe wrappers over the lambda-snark-sys C-ABI.

The reference's host language is Rust (absent from this image), so the wrappers that sit above the
C-ABI are mirrored here in Python with the same names, argument meaning and error behaviour:

* ``LweContext``  <-> rust-api/lambda-snark/src/context.rs:14-76   (``LweContext::new`` -> ``lwe_context_create``)
* ``Commitment``  <-> rust-api/lambda-snark/src/commitment.rs:31-121 (``new``, ``clone``, ``linear_combine``, ``as_bytes``)
* ``LweContext.combine_rows_device`` / ``LweContext.combine_rows`` <-> ``Commitment::linear_combine`` (commitment.rs:48-84) for a
  batch of device-resident (or host) wire rows: ``lsr_lwe_combine_rows_device`` / ``lsr_lwe_combine_batch_flat``
* ``verify_opening_with_context`` <-> rust-api/lambda-snark/src/opening.rs:160-222
* ``NttContext``  <-> the ``ntt_*`` symbols (only exercised by cpp-core/tests/test_ntt.cpp in the reference)
* ``CyclicNtt`` / ``QuotientPlan`` <-> rust-api/lambda-snark/src/ntt.rs:117-233 and r1cs.rs:474-506 (prover path)
* ``SimpleProver`` / ``verify_simple_batch`` <-> prove_simple, prove_zk, simulate_proof and verify_simple (lib.rs:465-681, 1269-1285)

All arithmetic happens in liblambda_snark_core.so (HIP, gfx950).  Nothing here computes; there is no
CPU fallback.  (The directory name has a hyphen; load it through ``__graft_entry__.load_package()``.)
"""
import ctypes
import weakref

import numpy as np

from . import _abi
from ._abi import PROFILE_RING_B, PROFILE_SCALAR_A, LweCommitment, LweOpening, PublicParams

__all__ = [
    "NttContext", "LweContext", "Commitment", "Params", "CoreError", "verify_opening_with_context",
    "sample_gaussian", "verify_openings_batch", "verify_openings_words", "PublicParams", "PROFILE_RING_B", "PROFILE_SCALAR_A",
    "CyclicNtt", "QuotientPlan", "R1csProver", "compute_root_of_unity", "NTT_MODULUS", "NTT_PRIMITIVE_ROOT",
    "RING_DOT_F64_RECENTRE_PERIOD", "RING_DOT_MAX_TERMS", "RING_FOLD_MAX_WIDTH", "RING_MATVEC_MAX_ROWS", "RING_MATVEC_MAX_MATRIX_BYTES", "RingMatrix", "ring_gadget_min_digits", "RING_SAMPLE_UNIFORM", "RING_SAMPLE_BOUNDED", "RING_SAMPLE_BALL", "RING_SAMPLE_MAX_WORDS", "ring_sample_key", "RING_OPNORM_MAX_DEGREE", "RING_CHALLENGE_ATTEMPT_WORDS", "RING_CHALLENGE_MAX_TRIES", "ring_opnorm_table", "RING_PACK_CENTRED", "RING_PACK_RESIDUE", "ring_pack_words", "ring_pack_min_bits", "RING_PROJECT_ROWS", "RING_PROJECT_ADJOINT_MAX_SETS", "RING_SCALAR_COMBINE_MAX_SETS", "RING_GRAM_MAX_VECTORS", "ring_gram_index", "RingMod", "ring_mod_primes", "ring_mod_capacity", "ring_mod_capacity_bounded", "ring_mod_capacity_product", "ring_mod_capacity_quadform", "RING_RESPOND_REJECTED", "RingModMatrix", "SimpleProver", "chacha20rng_keys", "random_blinding", "random_blinding_device", "verify_simple_batch", "verify_simple_batch_device",
]


class CoreError(RuntimeError):
    """Mirror of lambda_snark_core::Error::{FfiError, CommitmentFailed, InvalidDimensions}."""


def _u64_array(values, name="array"):
    arr = np.ascontiguousarray(values, dtype=np.uint64)
    if arr.ndim == 0:
        raise ValueError(f"{name} must be an array")
    return arr


def _ring_mul(lib, handle, n, a, b):
    """c = a * b in the context's ring (host arrays): a is [n] or [batch, n]; b is [n] (one b for every product) or [batch, n]."""
    a2 = np.ascontiguousarray(_u64_array(a).reshape(-1, n))
    b2 = np.ascontiguousarray(_u64_array(b).reshape(-1, n))
    batch, b_rows = a2.shape[0], b2.shape[0]
    out = np.empty_like(a2)
    if lib.lsr_ntt_ring_mul_batch(handle, out.ctypes.data, a2.ctypes.data, b2.ctypes.data, batch, b_rows) != 0:
        raise CoreError("lsr_ntt_ring_mul_batch failed: " + _abi.last_error())
    return out.reshape(np.shape(a)) if np.ndim(a) == 1 else out


def _ring_mul_device(lib, handle, d_c, d_a, d_b, batch, b_rows, stream):
    if lib.lsr_ntt_ring_mul_batch_device(handle, d_c, d_a, d_b, batch, b_rows, stream) != 0:
        raise CoreError("lsr_ntt_ring_mul_batch_device failed: " + _abi.last_error())


# FP64-flavour contexts re-centre the running sum of a ring inner product after this many products (batch.h
# LSR_RING_DOT_F64_RECENTRE_PERIOD); the largest number of terms is LSR_RING_DOT_MAX_TERMS
RING_DOT_F64_RECENTRE_PERIOD = 32
RING_DOT_MAX_TERMS = 65536
# the largest width of a ring fold (batch.h LSR_RING_FOLD_MAX_WIDTH)
RING_FOLD_MAX_WIDTH = 65536


def _ring_dot(lib, handle, n, a, b):
    """c = sum_i a_i * b_i in the context's ring (host arrays): a is [terms, n] (one output) or [batch, terms, n]; b is [terms, n] (one
    vector b for every output) or [batch, terms, n].  Returns [n] for a 2-d a, else [batch, n]."""
    a_in = _u64_array(a)
    if a_in.ndim < 2 or a_in.shape[-1] != n:
        raise ValueError("a must be [terms, n] or [batch, terms, n]")
    terms = a_in.shape[-2]
    if terms == 0:
        raise ValueError("terms must be at least 1")
    a3 = np.ascontiguousarray(a_in.reshape(-1, terms, n))
    b3 = np.ascontiguousarray(_u64_array(b).reshape(-1, terms, n))
    batch, b_rows = a3.shape[0], b3.shape[0]
    out = np.empty((batch, n), dtype=np.uint64)
    if lib.lsr_ntt_ring_dot_batch(handle, out.ctypes.data, a3.ctypes.data, b3.ctypes.data, batch, terms, b_rows) != 0:
        raise CoreError("lsr_ntt_ring_dot_batch failed: " + _abi.last_error())
    return out[0] if a_in.ndim == 2 else out


def _ring_dot_device(lib, handle, d_c, d_a, d_b, batch, terms, b_rows, stream):
    if lib.lsr_ntt_ring_dot_batch_device(handle, d_c, d_a, d_b, batch, terms, b_rows, stream) != 0:
        raise CoreError("lsr_ntt_ring_dot_batch_device failed: " + _abi.last_error())


# batch.h LSR_RING_MATVEC_MAX_ROWS / LSR_RING_MATVEC_MAX_MATRIX_BYTES: the caps on a RingMatrix (cols is capped by RING_DOT_MAX_TERMS)
RING_MATVEC_MAX_ROWS = 32768
RING_MATVEC_MAX_MATRIX_BYTES = 1 << 30


class RingMatrix:
    """A rows x cols matrix of ring elements resident on a context's device (``LsrRingMatrix*``, batch.h): ``matvec`` computes
    y_j = M x_j in the context's ring.  Made by ``NttContext.ring_matrix`` / ``CyclicNtt.ring_matrix`` (host array) or
    ``ring_matrix_device`` (device pointer).  Holds a reference to its context, which must stay open for every ``matvec``; ``close()`` itself does not read the context,
    so closing (or collecting) the matrix after its context is safe."""

    def __init__(self, ctx, handle):
        self._ctx, self._lib, self._h, self.n = ctx, ctx._lib, handle, ctx.n

    @property
    def handle(self):
        return self._h

    @property
    def rows(self):
        return self._lib.lsr_ntt_ring_matrix_rows(self._h)

    @property
    def cols(self):
        return self._lib.lsr_ntt_ring_matrix_cols(self._h)

    @property
    def row_block(self):
        """Rows of M one workgroup of the n <= 4096 kernel keeps in registers (1 above n = 4096)."""
        return self._lib.lsr_ntt_ring_matrix_row_block(self._h)

    def matvec(self, x):
        """x is [cols, n] (one vector, returns [rows, n]) or [batch, cols, n] (returns [batch, rows, n]); numpy in and out."""
        x_in = _u64_array(x)
        if x_in.ndim not in (2, 3) or x_in.shape[-2:] != (self.cols, self.n):
            raise ValueError("x must be [cols, n] or [batch, cols, n]")
        x3 = np.ascontiguousarray(x_in.reshape(-1, self.cols, self.n))
        out = np.empty((x3.shape[0], self.rows, self.n), dtype=np.uint64)
        if self._lib.lsr_ntt_ring_matvec_batch(self._h, out.ctypes.data, x3.ctypes.data, x3.shape[0]) != 0:
            raise CoreError("lsr_ntt_ring_matvec_batch failed: " + _abi.last_error())
        return out[0] if x_in.ndim == 2 else out

    def matvec_device(self, d_y, d_x, batch, stream=0):
        """Device buffers: y [batch][rows][n], x [batch][cols][n], asynchronous on `stream`."""
        if self._lib.lsr_ntt_ring_matvec_batch_device(self._h, d_y, d_x, batch, stream) != 0:
            raise CoreError("lsr_ntt_ring_matvec_batch_device failed: " + _abi.last_error())

    def matvec_gadget(self, x, base_log2, digits):
        """y = M G^-1(x) without the decomposed vector (n <= 4096): x is [xcols, n] or [batch, xcols, n] with xcols * digits == cols;
        equal to ``matvec(ctx.ring_decompose(x, base_log2, digits))`` word for word."""
        x_in = _u64_array(x)
        if x_in.ndim not in (2, 3) or x_in.shape[-1] != self.n or x_in.shape[-2] * int(digits) != self.cols:
            raise ValueError("x must be [xcols, n] or [batch, xcols, n] with xcols * digits == cols")
        x3 = np.ascontiguousarray(x_in.reshape(-1, x_in.shape[-2], self.n))
        out = np.empty((x3.shape[0], self.rows, self.n), dtype=np.uint64)
        if self._lib.lsr_ntt_ring_matvec_gadget_batch(self._h, out.ctypes.data, x3.ctypes.data, x3.shape[0], base_log2, digits) != 0:
            raise CoreError("lsr_ntt_ring_matvec_gadget_batch failed: " + _abi.last_error())
        return out[0] if x_in.ndim == 2 else out

    def matvec_gadget_device(self, d_y, d_x, batch, base_log2, digits, stream=0):
        """Device buffers: y [batch][rows][n], x [batch][cols / digits][n], asynchronous on `stream`."""
        if self._lib.lsr_ntt_ring_matvec_gadget_batch_device(self._h, d_y, d_x, batch, base_log2, digits, stream) != 0:
            raise CoreError("lsr_ntt_ring_matvec_gadget_batch_device failed: " + _abi.last_error())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.lsr_ntt_ring_matrix_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _ring_matrix(ctx, m):
    m_in = _u64_array(m)
    if m_in.ndim != 3 or m_in.shape[-1] != ctx.n:
        raise ValueError("m must be [rows, cols, n]")
    m3 = np.ascontiguousarray(m_in)
    handle = ctx._lib.lsr_ntt_ring_matrix_create(ctx._h, m3.ctypes.data, m3.shape[0], m3.shape[1])
    if not handle:
        raise CoreError("lsr_ntt_ring_matrix_create failed: " + _abi.last_error())
    return RingMatrix(ctx, handle)


def _ring_matrix_device(ctx, d_m, rows, cols, stream):
    handle = ctx._lib.lsr_ntt_ring_matrix_create_device(ctx._h, d_m, rows, cols, stream)
    if not handle:
        raise CoreError("lsr_ntt_ring_matrix_create_device failed: " + _abi.last_error())
    return RingMatrix(ctx, handle)


def ring_gadget_min_digits(q, base_log2):
    """The smallest admissible digit count of the balanced base-2^base_log2 decomposition under q (batch.h), 0 when there is none.
    Host only."""
    return _abi.lib().lsr_ring_gadget_min_digits(int(q), int(base_log2))


def _check(rc, name):
    if rc != 0:
        raise CoreError(name + " failed: " + _abi.last_error())


class _RingGadget:
    """Gadget decomposition on a context (``NttContext`` and ``CyclicNtt``; batch.h "gadget decomposition")."""

    def ring_decompose(self, x, base_log2, digits):
        """x [n] or [count, n] in [0, q) -> its balanced base-2^base_log2 digits [digits, n] or [count, digits, n], canonical residues."""
        x_in = _u64_array(x)
        if x_in.ndim not in (1, 2) or x_in.shape[-1] != self.n:
            raise ValueError("x must be [n] or [count, n]")
        x2 = np.ascontiguousarray(x_in.reshape(-1, self.n))
        out = np.empty((x2.shape[0], int(digits), self.n), dtype=np.uint64)
        _check(self._lib.lsr_ntt_ring_decompose_batch(self._h, out.ctypes.data, x2.ctypes.data, x2.shape[0], base_log2, digits),
               "lsr_ntt_ring_decompose_batch")
        return out[0] if x_in.ndim == 1 else out

    def ring_decompose_device(self, d_out, d_x, count, base_log2, digits, stream=0):
        """Device buffers: out [count][digits][n], x [count][n], asynchronous on `stream`."""
        _check(self._lib.lsr_ntt_ring_decompose_batch_device(self._h, d_out, d_x, count, base_log2, digits, stream),
               "lsr_ntt_ring_decompose_batch_device")

    def ring_recompose(self, z, base_log2):
        """z [digits, n] or [count, digits, n], any canonical residues -> sum_d 2^(base_log2 d) z[d] mod q, [n] or [count, n]."""
        z_in = _u64_array(z)
        if z_in.ndim not in (2, 3) or z_in.shape[-1] != self.n:
            raise ValueError("z must be [digits, n] or [count, digits, n]")
        digits = z_in.shape[-2]
        z3 = np.ascontiguousarray(z_in.reshape(-1, digits, self.n))
        out = np.empty((z3.shape[0], self.n), dtype=np.uint64)
        _check(self._lib.lsr_ntt_ring_recompose_batch(self._h, out.ctypes.data, z3.ctypes.data, z3.shape[0], base_log2, digits),
               "lsr_ntt_ring_recompose_batch")
        return out[0] if z_in.ndim == 2 else out

    def ring_recompose_device(self, d_out, d_z, count, base_log2, digits, stream=0):
        """Device buffers: out [count][n], z [count][digits][n], asynchronous on `stream`."""
        _check(self._lib.lsr_ntt_ring_recompose_batch_device(self._h, d_out, d_z, count, base_log2, digits, stream),
               "lsr_ntt_ring_recompose_batch_device")

    def ring_linf(self, x):
        """max |centred coefficient| of every element of x [..., n] (shape x.shape[:-1]); 2^64 - 1 for an element with a word >= q."""
        x_in = _u64_array(x)
        if x_in.shape[-1] != self.n:
            raise ValueError("x must be [..., n]")
        x2 = np.ascontiguousarray(x_in.reshape(-1, self.n))
        out = np.empty(x2.shape[0], dtype=np.uint64)
        _check(self._lib.lsr_ntt_ring_linf_batch(self._h, x2.ctypes.data, x2.shape[0], out.ctypes.data), "lsr_ntt_ring_linf_batch")
        return out.reshape(x_in.shape[:-1])

    def ring_linf_device(self, d_x, count, d_linf, stream=0):
        """Device buffers: x [count][n], linf [count], asynchronous on `stream`."""
        _check(self._lib.lsr_ntt_ring_linf_batch_device(self._h, d_x, count, d_linf, stream), "lsr_ntt_ring_linf_batch_device")


# batch.h LSR_RING_SAMPLE_*: the kinds of ring_sample and the attempt cap of its rejection primitive
RING_SAMPLE_UNIFORM, RING_SAMPLE_BOUNDED, RING_SAMPLE_BALL = 0, 1, 2
RING_SAMPLE_MAX_WORDS = 64


def ring_sample_key(seed):
    """The 256-bit stream key {seed_lo, seed_hi, "LSR1", "STRM", 0, 0, 0, 0} of a raw 64-bit seed as four uint64 words (batch.h
    lsr_ring_sample_key_from_seed): reproducible test streams, only as secret as the seed.  Host only."""
    key = np.zeros(4, dtype=np.uint64)
    _abi.lib().lsr_ring_sample_key_from_seed(int(seed), key.ctypes.data)
    return key


def _ring_keys(keys):
    """Keys as [groups, 4] uint64 words: a uint64 array of 4 words per key, or bytes / a uint8 array of 32 bytes per key (a digest)."""
    if isinstance(keys, (bytes, bytearray)):
        keys = np.frombuffer(bytes(keys), dtype=np.uint8)
    arr = np.asarray(keys)
    if arr.dtype == np.uint8:
        if arr.size == 0 or arr.size % 32:
            raise ValueError("byte keys must be 32 bytes each")
        return np.ascontiguousarray(arr).reshape(-1, 32).view("<u8")
    arr = _u64_array(keys, "keys")
    if arr.size == 0 or arr.size % 4:
        raise ValueError("keys must be four 64-bit words each")
    return np.ascontiguousarray(arr.reshape(-1, 4))


class _RingSample:
    """Seeded ring sampling on a context (``NttContext`` and ``CyclicNtt``; batch.h "seeded ring sampling")."""

    def ring_sample(self, count, kind, param, keys, components=None, domain=16, index_base=0):
        """[count, n] canonical ring elements of `kind` (RING_SAMPLE_UNIFORM with param 0, _BOUNDED with param beta, _BALL with param
        kappa).  Element e uses key e // components and stream index index_base + e % components; keys is [groups, 4] uint64 (or 32
        bytes per key) with groups >= ceil(count / components).  components=None spreads the elements evenly over the keys given:
        ceil(count / groups) — one key: all elements under it; count keys: one element each."""
        k2 = _ring_keys(keys)
        count = int(count)
        if components is None:
            components = max(1, -(-count // k2.shape[0]))
        components = int(components)
        if components > 0 and k2.shape[0] < -(-count // components):
            raise ValueError("keys must hold ceil(count / components) keys")
        out = np.empty((count, self.n), dtype=np.uint64)
        _check(self._lib.lsr_ntt_ring_sample_batch(self._h, out.ctypes.data, count, kind, param, k2.ctypes.data, components, domain, index_base),
               "lsr_ntt_ring_sample_batch")
        return out

    def ring_sample_device(self, d_out, count, kind, param, d_keys, components, domain=16, index_base=0, stream=0):
        """Device buffers: out [count][n]; d_keys [ceil(count / components)][4] words (8-byte aligned; transcript digests are valid
        keys).  Asynchronous on `stream`; enqueues only."""
        _check(self._lib.lsr_ntt_ring_sample_batch_device(self._h, d_out, count, kind, param, d_keys, components, domain, index_base, stream),
               "lsr_ntt_ring_sample_batch_device")

    def ring_matrix_seeded(self, key, rows, cols, domain=16, index_base=0):
        """The RingMatrix whose entry [r][c] is the UNIFORM element of stream index index_base + r cols + c under `key` (four uint64
        words or 32 bytes), sampled on the device: equal to ring_matrix(ring_sample(rows cols, RING_SAMPLE_UNIFORM, 0, key))."""
        k2 = _ring_keys(key)
        if k2.shape[0] != 1:
            raise ValueError("key must be one 256-bit key")
        handle = self._lib.lsr_ntt_ring_matrix_create_seeded(self._h, k2.ctypes.data, domain, index_base, rows, cols)
        if not handle:
            raise CoreError("lsr_ntt_ring_matrix_create_seeded failed: " + _abi.last_error())
        return RingMatrix(self, handle)


# batch.h LSR_RING_OPNORM_MAX_DEGREE, LSR_RING_CHALLENGE_*: the largest ring degree of the operator norm, the stream words set aside for
# one attempt of a challenge and the cap on max_tries
RING_OPNORM_MAX_DEGREE = 4096
RING_CHALLENGE_ATTEMPT_WORDS = 1 << 18
RING_CHALLENGE_MAX_TRIES = 1024


def ring_opnorm_table(n):
    """C[j] = round(2^30 cos(pi j / n)), 0 <= j < 2n, as int32 (batch.h lsr_ring_opnorm_table): the table of the fixed-point operator
    norm of a ring of degree n, a power of two in [2, RING_OPNORM_MAX_DEGREE].  Host only."""
    n = int(n)
    if not 0 <= n < 1 << 32:
        raise ValueError("n must fit 32 bits")
    out = np.zeros(2 * n if n <= RING_OPNORM_MAX_DEGREE else 1, dtype=np.int32)
    _check(_abi.lib().lsr_ring_opnorm_table(n, out.ctypes.data), "lsr_ring_opnorm_table")
    return out


class _RingChallenge:
    """The fixed-point operator norm and operator-norm-bounded challenges on a context (``NttContext`` and ``CyclicNtt``; batch.h
    "operator-norm-bounded ring challenges").  N(c) is an integer in units of 2^-60; "norm <= T" means N(c) <= T^2 2^60."""

    def ring_opnorm_prepare(self):
        """Builds the context's cosine table and makes it resident on the device (once): behind it ring_opnorm_device and
        ring_challenge_device enqueue only and can be captured into a graph."""
        _check(self._lib.lsr_ntt_ring_opnorm_prepare(self._h), "lsr_ntt_ring_opnorm_prepare")

    def ring_opnorm(self, x):
        """N(c) of every element of x [..., n] as Python ints (an object array of shape x.shape[:-1]; an int for one element);
        2^128 - 1 for an element with a word >= q or a centred coefficient above 2^15 in magnitude."""
        x_in = _u64_array(x, "x")
        if x_in.shape[-1] != self.n:
            raise ValueError("x must be [n] or [..., n]")
        x2 = np.ascontiguousarray(x_in.reshape(-1, self.n))
        out = np.empty((x2.shape[0], 2), dtype=np.uint64)
        _check(self._lib.lsr_ntt_ring_opnorm_batch(self._h, x2.ctypes.data, x2.shape[0], out.ctypes.data), "lsr_ntt_ring_opnorm_batch")
        values = [int(lo) | (int(hi) << 64) for lo, hi in out.tolist()]
        if x_in.ndim == 1:
            return values[0]
        res = np.empty(len(values), dtype=object)
        res[:] = values
        return res.reshape(x_in.shape[:-1])

    def ring_opnorm_device(self, d_x, count, d_out, stream=0):
        """Device buffers: x [count][n], out [count][2] (low word, high word).  Asynchronous on `stream`; the first call on a context
        without ring_opnorm_prepare uploads the table synchronously."""
        _check(self._lib.lsr_ntt_ring_opnorm_batch_device(self._h, d_x, count, d_out, stream), "lsr_ntt_ring_opnorm_batch_device")

    def ring_challenge(self, count, kappa1, kappa2, opnorm_bound, keys, components=None, max_tries=256, domain=16, index_base=0):
        """(out, tries): out [count, n] challenges with kappa1 coefficients +-1 and kappa2 coefficients +-2, tries int32 [count].
        opnorm_bound T > 0: element e is its first candidate with N(c) <= T^2 2^60 and tries[e] the attempts that took (zeros and 0
        when max_tries candidates failed: re-key); T = 0: the first candidate, tries 1 (kappa2 = 0: RING_SAMPLE_BALL).  Keys,
        components, domain and index_base as ring_sample."""
        k2 = _ring_keys(keys)
        count = int(count)
        if components is None:
            components = max(1, -(-count // k2.shape[0]))
        components = int(components)
        if components > 0 and k2.shape[0] < -(-count // components):
            raise ValueError("keys must hold ceil(count / components) keys")
        out = np.empty((count, self.n), dtype=np.uint64)
        tries = np.empty(count, dtype=np.int32)
        _check(self._lib.lsr_ntt_ring_challenge_batch(self._h, out.ctypes.data, tries.ctypes.data, count, kappa1, kappa2, int(opnorm_bound), max_tries,
                                                      k2.ctypes.data, components, domain, index_base), "lsr_ntt_ring_challenge_batch")
        return out, tries

    def ring_challenge_device(self, d_out, d_tries, count, kappa1, kappa2, opnorm_bound, d_keys, components, max_tries=256, domain=16,
                              index_base=0, stream=0):
        """Device buffers: out [count][n], tries int32 [count]; d_keys [ceil(count / components)][4] words (8-byte aligned; transcript
        digests are valid keys).  Asynchronous on `stream`; with opnorm_bound != 0 the first call on a context without
        ring_opnorm_prepare uploads the table synchronously."""
        _check(self._lib.lsr_ntt_ring_challenge_batch_device(self._h, d_out, d_tries, count, kappa1, kappa2, int(opnorm_bound), max_tries, d_keys,
                                                             components, domain, index_base, stream), "lsr_ntt_ring_challenge_batch_device")


# batch.h LSR_RING_PACK_*: the field of a coefficient is its centred value in two's complement, or the residue itself
RING_PACK_CENTRED, RING_PACK_RESIDUE = 0, 1


def ring_pack_words(n, bits):
    """W = ceil(n bits / 64), the words of one packed element (batch.h lsr_ring_pack_words); 0 for bits outside [1, 63].  Host only."""
    if not 0 <= int(bits) < 2**32:
        return 0
    return _abi.lib().lsr_ring_pack_words(int(n), int(bits))


def ring_pack_min_bits(q, mode, bound):
    """The fewest bits whose range holds every |v| <= bound (RING_PACK_CENTRED) or every x <= bound (RING_PACK_RESIDUE) under q
    (batch.h lsr_ring_pack_min_bits); 0 when there are none.  Host only."""
    return _abi.lib().lsr_ring_pack_min_bits(int(q), int(mode), int(bound))


class _RingPack:
    """Bit-packed encoding and decoding of short ring elements on a context (``NttContext`` and ``CyclicNtt``; batch.h "bit-packed
    ring elements")."""

    def ring_pack(self, x, bits, mode=RING_PACK_CENTRED):
        """x [n] or [count, n] canonical words -> (words uint64 [W] or [count, W], status int32 [] or [count]) with W =
        ring_pack_words(n, bits).  status 1: every coefficient in range; 0: one is not (its field is truncated); -1: a word >= q."""
        x_in = _u64_array(x, "x")
        if x_in.ndim not in (1, 2) or x_in.shape[-1] != self.n:
            raise ValueError("x must be [n] or [count, n]")
        x2 = np.ascontiguousarray(x_in.reshape(-1, self.n))
        out = np.zeros((x2.shape[0], ring_pack_words(self.n, bits)), dtype=np.uint64)
        status = np.zeros(x2.shape[0], dtype=np.int32)
        _check(self._lib.lsr_ntt_ring_pack_batch(self._h, out.ctypes.data, status.ctypes.data, x2.ctypes.data, x2.shape[0], int(mode), int(bits)),
               "lsr_ntt_ring_pack_batch")
        return (out[0], status[0]) if x_in.ndim == 1 else (out, status)

    def ring_pack_device(self, d_out, d_status, d_x, count, bits, mode=RING_PACK_CENTRED, stream=0):
        """Device buffers: out [count][W], status int32 [count], x [count][n]; 8-byte aligned.  Asynchronous on `stream`; enqueues
        only, allocates nothing."""
        _check(self._lib.lsr_ntt_ring_pack_batch_device(self._h, d_out, d_status, d_x, count, int(mode), int(bits), stream),
               "lsr_ntt_ring_pack_batch_device")

    def ring_unpack(self, words, bits, mode=RING_PACK_CENTRED):
        """words [W] or [count, W] -> (x uint64 [n] or [count, n], status int32 [] or [count]).  status 1: the canonical encoding of x;
        0: an invalid field (its word is 0) or a non-zero padding bit — CHECK IT before the data is used."""
        w_in = _u64_array(words, "words")
        wpe = ring_pack_words(self.n, bits)
        if w_in.ndim not in (1, 2) or (wpe and w_in.shape[-1] != wpe):
            raise ValueError("words must be [W] or [count, W] with W = ring_pack_words(n, bits)")
        w2 = np.ascontiguousarray(w_in.reshape(w_in.shape[0] if w_in.ndim == 2 else 1, -1))
        out = np.zeros((w2.shape[0], self.n), dtype=np.uint64)
        status = np.zeros(w2.shape[0], dtype=np.int32)
        _check(self._lib.lsr_ntt_ring_unpack_batch(self._h, out.ctypes.data, status.ctypes.data, w2.ctypes.data, w2.shape[0], int(mode), int(bits)),
               "lsr_ntt_ring_unpack_batch")
        return (out[0], status[0]) if w_in.ndim == 1 else (out, status)

    def ring_unpack_device(self, d_out, d_status, d_in, count, bits, mode=RING_PACK_CENTRED, stream=0):
        """Device buffers: out [count][n], status int32 [count], in [count][W]; 8-byte aligned.  Asynchronous on `stream`; enqueues
        only, allocates nothing."""
        _check(self._lib.lsr_ntt_ring_unpack_batch_device(self._h, d_out, d_status, d_in, count, int(mode), int(bits), stream),
               "lsr_ntt_ring_unpack_batch_device")


class _RingFold:
    """Fold of ring vectors by ring-valued challenges on a context (``NttContext`` and ``CyclicNtt``; batch.h)."""

    def ring_fold(self, v, p, term_stride=0):
        """out[j][c] = sum_i p[j][i] * v[j term_stride + i][c] in the context's ring (host arrays): v is [vectors, width, n], p is
        [outputs, terms, n] (or [terms, n]: one output) with vectors >= (outputs - 1) term_stride + terms.  Returns
        [outputs, width, n] ([width, n] for a 2-d p)."""
        n = self.n
        v_in, p_in = _u64_array(v, "v"), _u64_array(p, "p")
        if v_in.ndim != 3 or v_in.shape[-1] != n:
            raise ValueError("v must be [vectors, width, n]")
        if p_in.ndim not in (2, 3) or p_in.shape[-1] != n:
            raise ValueError("p must be [terms, n] or [outputs, terms, n]")
        terms, term_stride = p_in.shape[-2], int(term_stride)
        if terms == 0:
            raise ValueError("terms must be at least 1")
        v3, p3 = np.ascontiguousarray(v_in), np.ascontiguousarray(p_in.reshape(-1, terms, n))
        outputs, width = p3.shape[0], v3.shape[1]
        if term_stride < 0 or (outputs and v3.shape[0] < (outputs - 1) * term_stride + terms):
            raise ValueError("v must hold (outputs - 1) * term_stride + terms vectors")
        out = np.empty((outputs, width, n), dtype=np.uint64)
        _check(self._lib.lsr_ntt_ring_fold_batch(self._h, out.ctypes.data, v3.ctypes.data, p3.ctypes.data, outputs, terms, term_stride, width),
               "lsr_ntt_ring_fold_batch")
        return out[0] if p_in.ndim == 2 else out

    def ring_fold_device(self, d_out, d_v, d_p, outputs, terms, term_stride, width, stream=0):
        """Device buffers: out [outputs][width][n], v [(outputs - 1) term_stride + terms][width][n], p [outputs][terms][n].
        Asynchronous on `stream`; enqueues only."""
        _check(self._lib.lsr_ntt_ring_fold_batch_device(self._h, d_out, d_v, d_p, outputs, terms, term_stride, width, stream),
               "lsr_ntt_ring_fold_batch_device")


class _RingGalois:
    """Galois automorphisms sigma_g: X -> X^g on a context (``NttContext``: N = 2 n, ``CyclicNtt``: N = n; g odd, 1 <= g < N; batch.h
    "Galois automorphisms")."""

    _GALOIS_ORDER_PER_N = 2   # N / n: X has order 2 n modulo X^n + 1

    @property
    def galois_conjugation(self):
        """N - 1, the element of the conjugation X -> X^-1: coefficient 0 of ring_dot_galois(a, b, N - 1) is <a, b> mod q."""
        return self._GALOIS_ORDER_PER_N * self.n - 1

    def ring_automorphism(self, x, g):
        """sigma_g of every element of x [n] or [..., n] (canonical words in, canonical words out; same shape)."""
        x_in = _u64_array(x)
        if x_in.shape[-1] != self.n:
            raise ValueError("x must be [n] or [..., n]")
        x2 = np.ascontiguousarray(x_in.reshape(-1, self.n))
        out = np.empty_like(x2)
        _check(self._lib.lsr_ntt_ring_automorphism_batch(self._h, out.ctypes.data, x2.ctypes.data, x2.shape[0], int(g)),
               "lsr_ntt_ring_automorphism_batch")
        return out.reshape(x_in.shape)

    def ring_automorphism_device(self, d_out, d_x, count, g, stream=0):
        """Device buffers: out and x [count][n], out apart from x.  Asynchronous on `stream` in plain stream order; enqueues only."""
        _check(self._lib.lsr_ntt_ring_automorphism_batch_device(self._h, d_out, d_x, count, int(g), stream),
               "lsr_ntt_ring_automorphism_batch_device")

    def ring_dot_galois(self, a, b, g):
        """c = sum_i sigma_g(a_i) * b_i in the context's ring, equal to ring_dot(ring_automorphism(a, g), b) word for word (n <= 4096);
        shapes as ring_dot."""
        n = self.n
        a_in = _u64_array(a)
        if a_in.ndim < 2 or a_in.shape[-1] != n:
            raise ValueError("a must be [terms, n] or [batch, terms, n]")
        terms = a_in.shape[-2]
        if terms == 0:
            raise ValueError("terms must be at least 1")
        a3 = np.ascontiguousarray(a_in.reshape(-1, terms, n))
        b3 = np.ascontiguousarray(_u64_array(b).reshape(-1, terms, n))
        batch, b_rows = a3.shape[0], b3.shape[0]
        out = np.empty((batch, n), dtype=np.uint64)
        _check(self._lib.lsr_ntt_ring_dot_galois_batch(self._h, out.ctypes.data, a3.ctypes.data, b3.ctypes.data, batch, terms, b_rows, int(g)),
               "lsr_ntt_ring_dot_galois_batch")
        return out[0] if a_in.ndim == 2 else out

    def ring_dot_galois_device(self, d_c, d_a, d_b, batch, terms, b_rows, g, stream=0):
        """Device buffers, shapes as ring_dot_device.  Asynchronous on `stream`; enqueues only."""
        _check(self._lib.lsr_ntt_ring_dot_galois_batch_device(self._h, d_c, d_a, d_b, batch, terms, b_rows, int(g), stream),
               "lsr_ntt_ring_dot_galois_batch_device")


# batch.h LSR_RING_PROJECT_ROWS: the rows of the Johnson-Lindenstrauss projection
RING_PROJECT_ROWS = 256
# batch.h LSR_RING_PROJECT_ADJOINT_MAX_SETS: the most weight sets of one ring_project_adjoint call
RING_PROJECT_ADJOINT_MAX_SETS = 16


class _RingNorm:
    """Exact l2 norms and seeded Johnson-Lindenstrauss projections of ring vectors on a context (``NttContext`` and ``CyclicNtt``;
    batch.h "norms and projections of ring vectors").  A vector is [width, n] canonical words."""

    def _ring_vectors(self, x):
        x_in = _u64_array(x, "x")
        if x_in.ndim < 2 or x_in.shape[-1] != self.n:
            raise ValueError("x must be [width, n] or [..., width, n]")
        width = x_in.shape[-2]
        return x_in, np.ascontiguousarray(x_in.reshape(-1, width, self.n)), width

    def ring_l2sq(self, x):
        """sum of the squared centred coefficients of every vector of x [..., width, n], exact, as Python ints (an object array of
        shape x.shape[:-2]; an int for one vector); 2^128 - 1 for a vector with a word >= q or a sum that does not fit below it."""
        x_in, x3, width = self._ring_vectors(x)
        out = np.empty((x3.shape[0], 2), dtype=np.uint64)
        _check(self._lib.lsr_ntt_ring_l2sq_batch(self._h, x3.ctypes.data, x3.shape[0], width, out.ctypes.data), "lsr_ntt_ring_l2sq_batch")
        values = [int(lo) | (int(hi) << 64) for lo, hi in out.tolist()]
        if x_in.ndim == 2:
            return values[0]
        res = np.empty(len(values), dtype=object)
        res[:] = values
        return res.reshape(x_in.shape[:-2])

    def ring_l2sq_device(self, d_x, count, width, d_out, stream=0):
        """Device buffers: x [count][width][n], out [count][2] (low word, high word).  Asynchronous on `stream`; enqueues only."""
        _check(self._lib.lsr_ntt_ring_l2sq_batch_device(self._h, d_x, count, width, d_out, stream), "lsr_ntt_ring_l2sq_batch_device")

    def ring_project(self, x, bound, keys, components=None, domain=17, index_base=0):
        """(p, status) for x [count, width, n] (or [width, n]: one vector): p int64 [count, 256] with p[j][r] = <pi_r, centred x[j]>
        over the integers, status int32 [count] (1 done; 0 some |coefficient| above bound; -1 a word >= q; p[j] is 0 unless 1).
        Vector j uses key j // components and the streams index_base + 256 (j % components) + r; keys as ring_sample;
        components=None spreads the vectors evenly over the keys given."""
        x_in, x3, width = self._ring_vectors(x)
        k2 = _ring_keys(keys)
        count = x3.shape[0]
        if components is None:
            components = max(1, -(-count // k2.shape[0]))
        components = int(components)
        if components > 0 and k2.shape[0] < -(-count // components):
            raise ValueError("keys must hold ceil(count / components) keys")
        out = np.empty((count, RING_PROJECT_ROWS), dtype=np.int64)
        status = np.empty(count, dtype=np.int32)
        _check(self._lib.lsr_ntt_ring_project_batch(self._h, out.ctypes.data, status.ctypes.data, x3.ctypes.data, count, width, int(bound),
                                                    k2.ctypes.data, components, domain, index_base), "lsr_ntt_ring_project_batch")
        return (out[0], status[0]) if x_in.ndim == 2 else (out, status)

    def ring_project_device(self, d_out, d_status, d_x, count, width, bound, d_keys, components, domain=17, index_base=0, stream=0):
        """Device buffers: out [count][256] int64, status [count] int32, x [count][width][n], d_keys [ceil(count / components)][4]
        words.  Asynchronous on `stream`; enqueues only and allocates nothing."""
        _check(self._lib.lsr_ntt_ring_project_batch_device(self._h, d_out, d_status, d_x, count, width, int(bound), d_keys, components, domain,
                                                           index_base, stream), "lsr_ntt_ring_project_batch_device")

    def ring_project_matrix(self, key, width, rows_first=0, rows=RING_PROJECT_ROWS, domain=17, index_base=0):
        """Rows rows_first .. rows_first + rows - 1 of the projection matrix of (key, index_base) as ring elements [rows, width, n]
        with words 0, 1, q - 1: coefficient 0 of ring_dot_galois(row r, s, galois_conjugation) is p_r mod q."""
        k2 = _ring_keys(key)
        if k2.shape[0] != 1:
            raise ValueError("key must be one 256-bit key")
        out = np.empty((int(rows), int(width), self.n), dtype=np.uint64)
        _check(self._lib.lsr_ntt_ring_project_matrix_batch(self._h, out.ctypes.data, rows_first, rows, width, k2.ctypes.data, domain, index_base),
               "lsr_ntt_ring_project_matrix_batch")
        return out

    def ring_project_matrix_device(self, d_out, rows_first, rows, width, d_key, domain=17, index_base=0, stream=0):
        """Device buffers: out [rows][width][n], d_key four words.  Asynchronous on `stream`; enqueues only."""
        _check(self._lib.lsr_ntt_ring_project_matrix_batch_device(self._h, d_out, rows_first, rows, width, d_key, domain, index_base, stream),
               "lsr_ntt_ring_project_matrix_batch_device")

    def ring_project_adjoint(self, weights, width, count, keys, components=None, conjugate=False, domain=17, index_base=0):
        """(out, status) = the adjoint Pi^T w of ring_project: weights [groups, sets, 256] canonical words (or
        [sets, 256]: one group), groups = ceil(count / components) -> out uint64 [count, sets, width, n] with out[j][k][pos] =
        sum_r weights[j // components][k][r] pi_j[r][pos] mod q, pi_j the matrix ring_project uses for vector j; conjugate: every
        element under sigma_{N-1} (ring_automorphism with g = galois_conjugation).  status int32 [count]: 1, or -1 (out[j] all 0)
        when a weight of the vector's group is >= q.  components=None spreads the vectors evenly over the keys given."""
        w = _u64_array(weights, "weights")
        if w.ndim == 2:
            w = w[None]
        if w.ndim != 3 or w.shape[2] != RING_PROJECT_ROWS:
            raise ValueError("weights must be [groups, sets, 256] or [sets, 256]")
        k2 = _ring_keys(keys)
        count, width = int(count), int(width)
        if components is None:
            components = max(1, -(-count // k2.shape[0]))
        components = int(components)
        groups = -(-count // components) if components > 0 else 0
        if k2.shape[0] < groups or w.shape[0] < groups:
            raise ValueError("keys and weights must hold ceil(count / components) groups")
        sets = w.shape[1]
        out = np.empty((count, sets, width, self.n), dtype=np.uint64)
        status = np.empty(count, dtype=np.int32)
        _check(self._lib.lsr_ntt_ring_project_adjoint_batch(self._h, out.ctypes.data, status.ctypes.data, w.ctypes.data, count, sets, width,
                                                            int(bool(conjugate)), k2.ctypes.data, components, domain, index_base),
               "lsr_ntt_ring_project_adjoint_batch")
        return out, status

    def ring_project_adjoint_device(self, d_out, d_status, d_weights, count, sets, width, conjugate, d_keys, components, domain=17, index_base=0,
                                    stream=0):
        """Device buffers: out [count][sets][width][n], status [count] int32, weights [ceil(count / components)][sets][256], d_keys
        [ceil(count / components)][4] words.  Asynchronous on `stream`; one kernel, allocates nothing."""
        _check(self._lib.lsr_ntt_ring_project_adjoint_batch_device(self._h, d_out, d_status, d_weights, count, sets, width, int(conjugate), d_keys,
                                                                   components, domain, index_base, stream),
               "lsr_ntt_ring_project_adjoint_batch_device")


# batch.h LSR_RING_SCALAR_COMBINE_MAX_SETS: the most weight sets of one ring_scalar_combine call
RING_SCALAR_COMBINE_MAX_SETS = 16


class _RingScalar:
    """Scalar-weighted aggregation of ring vectors with an addend on a context (``NttContext`` and ``CyclicNtt``; batch.h
    "scalar-weighted aggregation of ring vectors").  A vector is [width, n] canonical words."""

    def ring_scalar_combine(self, v, weights, count, term_stride=0, components=None, addend=None):
        """(out, status): out uint64 [count, sets, width, n] with out[j][k] = addend[j][k] + sum_i weights[j // components][k][i] *
        v[j term_stride + i] mod q, the weights SCALARS of Z_q.  v is [vectors, width, n] with vectors >= (count - 1) term_stride +
        terms; weights [groups, sets, terms] canonical words (or [sets, terms]: one group), groups = ceil(count / components);
        addend None or [count, sets, width, n].  status int32 [count]: 1, or -1 (out[j] all 0) when a weight of the vector's group
        is >= q.  components=None spreads the vectors evenly over the weight groups given."""
        n = self.n
        v_in, w = _u64_array(v, "v"), _u64_array(weights, "weights")
        if v_in.ndim != 3 or v_in.shape[-1] != n:
            raise ValueError("v must be [vectors, width, n]")
        if w.ndim == 2:
            w = w[None]
        if w.ndim != 3:
            raise ValueError("weights must be [groups, sets, terms] or [sets, terms]")
        v3, w3 = np.ascontiguousarray(v_in), np.ascontiguousarray(w)
        count, term_stride, width = int(count), int(term_stride), v3.shape[1]
        sets, terms = w3.shape[1], w3.shape[2]
        if components is None:
            components = max(1, -(-count // max(1, w3.shape[0])))
        components = int(components)
        if components > 0 and w3.shape[0] < -(-count // components):
            raise ValueError("weights must hold ceil(count / components) groups")
        if count < 0 or term_stride < 0 or (count and v3.shape[0] < (count - 1) * term_stride + terms):
            raise ValueError("v must hold (count - 1) * term_stride + terms vectors")
        a4 = None
        if addend is not None:
            a4 = np.ascontiguousarray(_u64_array(addend, "addend"))
            if a4.shape != (count, sets, width, n):
                raise ValueError("addend must be [count, sets, width, n]")
        out = np.empty((count, sets, width, n), dtype=np.uint64)
        status = np.empty(count, dtype=np.int32)
        _check(self._lib.lsr_ntt_ring_scalar_combine_batch(self._h, out.ctypes.data, status.ctypes.data, v3.ctypes.data, w3.ctypes.data,
                                                           None if a4 is None else a4.ctypes.data, count, sets, terms, term_stride, width, components),
               "lsr_ntt_ring_scalar_combine_batch")
        return out, status

    def ring_scalar_combine_device(self, d_out, d_status, d_v, d_weights, d_addend, count, sets, terms, term_stride, width, components, stream=0):
        """Device buffers: out [count][sets][width][n], status [count] int32, v [(count - 1) term_stride + terms][width][n], weights
        [ceil(count / components)][sets][terms]; d_addend 0 or None, a buffer laid out as out, or d_out itself (in place).
        Asynchronous on `stream`; one kernel, allocates nothing."""
        _check(self._lib.lsr_ntt_ring_scalar_combine_batch_device(self._h, d_out, d_status, d_v, d_weights, d_addend or None, count, sets, terms,
                                                                  term_stride, width, components, stream),
               "lsr_ntt_ring_scalar_combine_batch_device")


# the most vectors of one family of a ring Gram matrix (batch.h LSR_RING_GRAM_MAX_VECTORS)
RING_GRAM_MAX_VECTORS = 64
# the status of a response whose inputs were fine and whose norm was not (batch.h LSR_RING_RESPOND_REJECTED)
RING_RESPOND_REJECTED = 2


def ring_gram_index(r, i, l):
    """The polynomial of the pair (i, l), i <= l < r, in the packed upper triangle a symmetric ring_gram returns."""
    r, i, l = int(r), int(i), int(l)
    if not 0 <= i <= l < r:
        raise ValueError("ring_gram_index takes 0 <= i <= l < r")
    return i * r - i * (i - 1) // 2 + (l - i)


class _RingGram:
    """Ring Gram matrices G = A B^T of families of ring vectors on a context (``NttContext`` and ``CyclicNtt``; batch.h "batched ring
    Gram matrices")."""

    @property
    def ring_gram_block(self):
        """The edge E of the register block of the Gram kernel in this context's arithmetic flavour."""
        return int(self._lib.lsr_ntt_ring_gram_block(self._h))

    def ring_gram(self, a, b=None):
        """g[j][i][l] = sum_c a[j][i][c] * b[j][l][c] in the context's ring (host arrays): a is [batch, ra, width, n], b is
        [batch, rb, width, n]; returns [batch, ra, rb, n].  b=None: the family with itself, only i <= l, returned packed as
        [batch, ra (ra + 1) / 2, n] (ring_gram_index).  3-d operands ([ra, width, n]) are a batch of one, and so is the result."""
        n = self.n
        a_in = _u64_array(a, "a")
        if a_in.ndim not in (3, 4) or a_in.shape[-1] != n:
            raise ValueError("a must be [ra, width, n] or [batch, ra, width, n]")
        ra, width = a_in.shape[-3], a_in.shape[-2]
        a4 = np.ascontiguousarray(a_in.reshape(-1, ra, width, n))
        batch = a4.shape[0]
        if b is None:
            out = np.empty((batch, ra * (ra + 1) // 2, n), dtype=np.uint64)
            _check(self._lib.lsr_ntt_ring_gram_batch(self._h, out.ctypes.data, a4.ctypes.data, None, batch, ra, ra, width), "lsr_ntt_ring_gram_batch")
            return out[0] if a_in.ndim == 3 else out
        b_in = a_in if b is a else _u64_array(b, "b")
        if b_in.ndim != a_in.ndim or b_in.shape[-1] != n or b_in.shape[-2] != width:
            raise ValueError("b must be [rb, width, n] or [batch, rb, width, n], with the width and the rank of a")
        rb = b_in.shape[-3]
        b4 = a4 if b_in is a_in else np.ascontiguousarray(b_in.reshape(-1, rb, width, n))
        if b4.shape[0] != batch:
            raise ValueError("a and b must hold the same number of families")
        out = np.empty((batch, ra, rb, n), dtype=np.uint64)
        _check(self._lib.lsr_ntt_ring_gram_batch(self._h, out.ctypes.data, a4.ctypes.data, b4.ctypes.data, batch, ra, rb, width), "lsr_ntt_ring_gram_batch")
        return out[0] if a_in.ndim == 3 else out

    def ring_gram_device(self, d_g, d_a, d_b, batch, ra, rb, width, stream=0):
        """Device buffers: a [batch][ra][width][n], b [batch][rb][width][n], g [batch][ra][rb][n]; d_b of 0 or None: the symmetric
        form, g [batch][ra (ra + 1) / 2][n].  Asynchronous on `stream`; enqueues only."""
        _check(self._lib.lsr_ntt_ring_gram_batch_device(self._h, d_g, d_a, d_b or None, batch, ra, rb, width, stream), "lsr_ntt_ring_gram_batch_device")

    def ring_gram_sym2(self, a, b):
        """The symmetrised packed Gram matrix of two families (host arrays): a and b are [batch, r, width, n] (b may be
        a itself); returns h [batch, r (r + 1) / 2, n] (ring_gram_index) with h[j][(i, l)] = <a_i, b_l> + <a_l, b_i> for i < l and
        h[j][(i, i)] = <a_i, b_i>.  3-d operands ([r, width, n]) are a batch of one, and so is the result."""
        n = self.n
        a_in = _u64_array(a, "a")
        b_in = a_in if b is a else _u64_array(b, "b")
        if a_in.ndim not in (3, 4) or a_in.shape[-1] != n:
            raise ValueError("a must be [r, width, n] or [batch, r, width, n]")
        if b_in.shape != a_in.shape:
            raise ValueError("b must have the shape of a")
        r, width = a_in.shape[-3], a_in.shape[-2]
        a4 = np.ascontiguousarray(a_in.reshape(-1, r, width, n))
        b4 = a4 if b_in is a_in else np.ascontiguousarray(b_in.reshape(-1, r, width, n))
        batch = a4.shape[0]
        out = np.empty((batch, r * (r + 1) // 2, n), dtype=np.uint64)
        _check(self._lib.lsr_ntt_ring_gram_sym2_batch(self._h, out.ctypes.data, a4.ctypes.data, b4.ctypes.data, batch, r, width), "lsr_ntt_ring_gram_sym2_batch")
        return out[0] if a_in.ndim == 3 else out

    def ring_gram_sym2_device(self, d_h, d_a, d_b, batch, r, width, stream=0):
        """Device buffers: a and b [batch][r][width][n] (d_b may be d_a), h [batch][r (r + 1) / 2][n].  Asynchronous on `stream`; enqueues
        only."""
        _check(self._lib.lsr_ntt_ring_gram_sym2_batch_device(self._h, d_h, d_a, d_b or None, batch, r, width, stream), "lsr_ntt_ring_gram_sym2_batch_device")

    def ring_quadform(self, g, c, offdiag=2):
        """out[j] = sum_i g[j][(i, i)] c_i c_i + offdiag * sum_{i < l} g[j][(i, l)] c_i c_l in the context's ring (host arrays, DESIGN.md
        §5m): g is [batch, r (r + 1) / 2, n] in the packed order of a symmetric ring_gram (ring_gram_index), c is [batch, r, n], or
        [r, n]: one set of challenges shared by every family; returns [batch, n].  offdiag: a word below q — 2 for a ring_gram(s), 1
        for a ring_gram_sym2(phi, s).  A 2-d g is a batch of one, and so is the result."""
        n = self.n
        g_in, c_in = _u64_array(g, "g"), _u64_array(c, "c")
        if g_in.ndim not in (2, 3) or g_in.shape[-1] != n:
            raise ValueError("g must be [pairs, n] or [batch, pairs, n]")
        if c_in.ndim not in (2, 3) or c_in.shape[-1] != n:
            raise ValueError("c must be [r, n] or [batch, r, n]")
        r, pairs = c_in.shape[-2], g_in.shape[-2]
        if pairs != r * (r + 1) // 2:
            raise ValueError("g must hold r (r + 1) / 2 polynomials per family for the r polynomials of c")
        g3 = np.ascontiguousarray(g_in.reshape(-1, pairs, n))
        c3 = np.ascontiguousarray(c_in.reshape(-1, r, n))
        batch, c_rows = g3.shape[0], (1 if c_in.ndim == 2 else c3.shape[0])
        if c_rows not in (1, batch):
            raise ValueError("c must hold one set of challenges ([r, n]) or one per family of g")
        out = np.empty((batch, n), dtype=np.uint64)
        _check(self._lib.lsr_ntt_ring_quadform_batch(self._h, out.ctypes.data, g3.ctypes.data, c3.ctypes.data, batch, r, c_rows, int(offdiag)),
               "lsr_ntt_ring_quadform_batch")
        return out[0] if g_in.ndim == 2 else out

    def ring_quadform_device(self, d_out, d_g, d_c, batch, r, c_rows, offdiag=2, stream=0):
        """Device buffers: g [batch][r (r + 1) / 2][n], c [c_rows][r][n] with c_rows 1 or batch, out [batch][n].  Asynchronous on
        `stream`; enqueues only."""
        _check(self._lib.lsr_ntt_ring_quadform_batch_device(self._h, d_out, d_g, d_c, batch, r, c_rows, int(offdiag), stream),
               "lsr_ntt_ring_quadform_batch_device")


class NttContext(_RingGadget, _RingSample, _RingChallenge, _RingPack, _RingFold, _RingGalois, _RingNorm, _RingScalar, _RingGram):
    """RAII handle over ``NttContext*`` (cpp-core/include/lambda_snark/ntt.h:25-41)."""

    def __init__(self, q, n, device=-1):
        self._lib = _abi.lib()
        self.q, self.n = int(q), int(n)
        self._h = self._lib.lsr_ntt_context_create_on(self.q, self.n, device) if device >= 0 else self._lib.ntt_context_create(self.q, self.n)
        if not self._h:
            raise CoreError(f"ntt_context_create({q}, {n}) returned NULL: {_abi.last_error()}")

    @property
    def handle(self):
        return self._h

    @property
    def root(self):
        return self._lib.lsr_ntt_context_root(self._h)

    @property
    def uses_f64(self):
        return bool(self._lib.lsr_ntt_context_uses_f64(self._h))

    @property
    def handoff_bytes(self):
        """Bytes per residue of the intermediate between the two passes of an n > 4096 transform (6 or 8; batch.h)."""
        return self._lib.lsr_ntt_handoff_bytes(self._h)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ntt_context_free(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # --- reference single-polynomial entry points (host buffers, in place) ---
    def forward(self, coeffs):
        a = _u64_array(coeffs).copy()
        if self._lib.ntt_forward(self._h, a.ctypes.data, a.size) != 0:
            raise CoreError("ntt_forward failed")
        return a

    def inverse(self, evals):
        a = _u64_array(evals).copy()
        if self._lib.ntt_inverse(self._h, a.ctypes.data, a.size) != 0:
            raise CoreError("ntt_inverse failed")
        return a

    def mul_pointwise(self, a, b):
        a, b = _u64_array(a), _u64_array(b)
        out = np.zeros_like(a)
        self._lib.ntt_mul_pointwise(self._h, out.ctypes.data, a.ctypes.data, b.ctypes.data, a.size)
        return out

    # --- batched host entry points ([batch][n]) ---
    def forward_batch(self, polys):
        a = _u64_array(polys).copy().reshape(-1, self.n)
        if self._lib.ntt_forward_batch(self._h, a.ctypes.data, a.shape[0]) != 0:
            raise CoreError("ntt_forward_batch failed: " + _abi.last_error())
        return a

    def inverse_batch(self, polys):
        a = _u64_array(polys).copy().reshape(-1, self.n)
        if self._lib.ntt_inverse_batch(self._h, a.ctypes.data, a.shape[0]) != 0:
            raise CoreError("ntt_inverse_batch failed: " + _abi.last_error())
        return a

    # --- device-resident entry points (raw device pointers, e.g. torch.Tensor.data_ptr()) ---
    def forward_device(self, dptr, batch, stream=0):
        if self._lib.lsr_ntt_forward_batch_device(self._h, dptr, batch, stream) != 0:
            raise CoreError("lsr_ntt_forward_batch_device failed: " + _abi.last_error())

    def inverse_device(self, dptr, batch, stream=0):
        if self._lib.lsr_ntt_inverse_batch_device(self._h, dptr, batch, stream) != 0:
            raise CoreError("lsr_ntt_inverse_batch_device failed: " + _abi.last_error())

    def mul_pointwise_device(self, dres, da, db, count, stream=0):
        if self._lib.lsr_ntt_mul_pointwise_device(self._h, dres, da, db, count, stream) != 0:
            raise CoreError("lsr_ntt_mul_pointwise_device failed: " + _abi.last_error())

    # --- ring multiply in Z_q[X]/(X^n + 1) ---
    def ring_mul(self, a, b):
        """a * b mod (X^n + 1, q): a is [n] or [batch, n], b is [n] (shared by every product) or [batch, n]; numpy in and out."""
        return _ring_mul(self._lib, self._h, self.n, a, b)

    def ring_mul_device(self, d_c, d_a, d_b, batch, b_rows, stream=0):
        """Device buffers [batch][n] (b: [b_rows][n], b_rows 1 or batch), asynchronous on `stream`."""
        _ring_mul_device(self._lib, self._h, d_c, d_a, d_b, batch, b_rows, stream)

    # --- ring inner product in Z_q[X]/(X^n + 1) ---
    def ring_dot(self, a, b):
        """sum_i a_i * b_i mod (X^n + 1, q): a is [terms, n] or [batch, terms, n], b is [terms, n] (shared by every output) or
        [batch, terms, n]; numpy in and out ([n] or [batch, n])."""
        return _ring_dot(self._lib, self._h, self.n, a, b)

    def ring_dot_device(self, d_c, d_a, d_b, batch, terms, b_rows, stream=0):
        """Device buffers: c [batch][n], a [batch][terms][n], b [b_rows][terms][n] (b_rows 1 or batch), asynchronous on `stream`."""
        _ring_dot_device(self._lib, self._h, d_c, d_a, d_b, batch, terms, b_rows, stream)

    # --- ring matrix-vector product y = M x with a matrix resident on the device ---
    def ring_matrix(self, m):
        """A RingMatrix of m [rows, cols, n] (host array; copied and, at n <= 4096, transformed once)."""
        return _ring_matrix(self, m)

    def ring_matrix_device(self, d_m, rows, cols, stream=0):
        """A RingMatrix of the device buffer d_m [rows][cols][n], asynchronous on `stream`."""
        return _ring_matrix_device(self, d_m, rows, cols, stream)


def ring_mod_primes(n):
    """``lsr_ring_mod_primes``: the two 44-bit NTT primes (p1, p2) a RingMod of ring degree n computes under (host only)."""
    out = (ctypes.c_uint64 * 2)()
    if _abi.lib().lsr_ring_mod_primes(int(n), out) != 0:
        raise ValueError("unsupported ring degree")
    return int(out[0]), int(out[1])


def ring_mod_capacity(q, n):
    """``lsr_ring_mod_capacity``: how many products mod q, degree n, one sum may hold (max_terms); 0 when (q, n) is not admissible
    (host only)."""
    if not (0 <= int(q) < 2**64 and 0 <= int(n) < 2**32):
        return 0
    return int(_abi.lib().lsr_ring_mod_capacity(int(q), int(n)))


def ring_mod_capacity_bounded(q, n, bound):
    """``lsr_ring_mod_capacity_bounded``: how many products of an element mod q with an element of centred magnitude <= bound, degree n,
    one sum may hold; 0 for bound == 0, bound > q // 2 or an inadmissible (q, n) (host only)."""
    if not (0 <= int(q) < 2**64 and 0 <= int(n) < 2**32 and 0 <= int(bound) < 2**64):
        return 0
    return int(_abi.lib().lsr_ring_mod_capacity_bounded(int(q), int(n), int(bound)))


def ring_mod_capacity_product(q, n, bound_a, bound_b):
    """``lsr_ring_mod_capacity_product``: how many products of an element of centred magnitude <= bound_a with one of magnitude
    <= bound_b, degree n, one sum mod q may hold; 0 for a bound of 0 or above q // 2 or an inadmissible (q, n) (host only)."""
    if not (0 <= int(q) < 2**64 and 0 <= int(n) < 2**32 and 0 <= int(bound_a) < 2**64 and 0 <= int(bound_b) < 2**64):
        return 0
    return int(_abi.lib().lsr_ring_mod_capacity_product(int(q), int(n), int(bound_a), int(bound_b)))


def ring_mod_capacity_quadform(q, n, bound_g, bound_c):
    """``lsr_ring_mod_capacity_quadform``: how many triple products g c c' of an element of centred magnitude <= bound_g with two of
    magnitude <= bound_c, degree n, one sum mod q may hold (a bound of 0: none, q // 2); 0 for a bound above q // 2 or an inadmissible
    (q, n) (host only)."""
    if not (0 <= int(q) < 2**64 and 0 <= int(n) < 2**32 and 0 <= int(bound_g) < 2**64 and 0 <= int(bound_c) < 2**64):
        return 0
    return int(_abi.lib().lsr_ring_mod_capacity_quadform(int(q), int(n), int(bound_g), int(bound_c)))


class RingModMatrix:
    """A rows x cols matrix over Z_q[X]/(X^n + 1) resident on a RingMod's device (``LsrRingModMatrix*``, batch.h "resident matrices
    under any modulus").  Made by ``RingMod.matrix`` (host array), ``matrix_device`` (device pointer) or
    ``matrix_seeded``.  Its RingMod must stay open for every call; closing the RingMod closes its matrices first."""

    def __init__(self, ring, handle):
        self._ring, self._lib, self._h, self.n = ring, ring._lib, handle, ring.n
        ring._matrices.add(self)
        ring._matrix_handles.add(handle)

    @property
    def handle(self):
        return self._h

    @property
    def rows(self):
        return self._lib.lsr_ring_mod_matrix_rows(self._h)

    @property
    def cols(self):
        return self._lib.lsr_ring_mod_matrix_cols(self._h)

    @property
    def row_block(self):
        """Rows of M one workgroup of the kernel keeps in registers."""
        return self._lib.lsr_ring_mod_matrix_row_block(self._h)

    def matvec(self, x):
        """y = M x mod (X^n + 1, q): x is [cols, n] (returns [rows, n]) or [batch, cols, n] (returns [batch, rows, n]); numpy in and out."""
        x_in = _u64_array(x)
        if x_in.ndim not in (2, 3) or x_in.shape[-2:] != (self.cols, self.n):
            raise ValueError("x must be [cols, n] or [batch, cols, n]")
        x3 = np.ascontiguousarray(x_in.reshape(-1, self.cols, self.n))
        out = np.empty((x3.shape[0], self.rows, self.n), dtype=np.uint64)
        _check(self._lib.lsr_ring_mod_matvec_batch(self._h, out.ctypes.data, x3.ctypes.data, x3.shape[0]), "lsr_ring_mod_matvec_batch")
        return out[0] if x_in.ndim == 2 else out

    def matvec_device(self, d_y, d_x, batch, stream=0):
        """Device buffers: y [batch][rows][n], x [batch][cols][n], asynchronous on `stream`."""
        _check(self._lib.lsr_ring_mod_matvec_batch_device(self._h, d_y, d_x, batch, stream), "lsr_ring_mod_matvec_batch_device")

    def matvec_gadget(self, x, base_log2, digits):
        """y = M G^-1(x) with the digits taken against q and never stored: x is [xcols, n] or [batch, xcols, n], xcols * digits == cols."""
        x_in = _u64_array(x)
        if x_in.ndim not in (2, 3) or x_in.shape[-1] != self.n or x_in.shape[-2] * int(digits) != self.cols:
            raise ValueError("x must be [xcols, n] or [batch, xcols, n] with xcols * digits == cols")
        x3 = np.ascontiguousarray(x_in.reshape(-1, x_in.shape[-2], self.n))
        out = np.empty((x3.shape[0], self.rows, self.n), dtype=np.uint64)
        _check(self._lib.lsr_ring_mod_matvec_gadget_batch(self._h, out.ctypes.data, x3.ctypes.data, x3.shape[0], base_log2, digits),
               "lsr_ring_mod_matvec_gadget_batch")
        return out[0] if x_in.ndim == 2 else out

    def matvec_gadget_device(self, d_y, d_x, batch, base_log2, digits, stream=0):
        """Device buffers: y [batch][rows][n], x [batch][cols / digits][n], asynchronous on `stream`."""
        _check(self._lib.lsr_ring_mod_matvec_gadget_batch_device(self._h, d_y, d_x, batch, base_log2, digits, stream),
               "lsr_ring_mod_matvec_gadget_batch_device")

    def matvec_bounded(self, x, bound_x=0):
        """y = M x with the bound on x verified on the device: x is [cols, n] or [batch, cols, n].  Returns
        (y [batch, rows, n], status [batch]) — ([rows, n], status) for a 2-d x.  bound_x: the l-infinity bound asserted on the centred
        words of x (0: none); status[j] is 1 where every word of x[j] kept it (y[j] is ``matvec``'s), 0 where one exceeded the bound,
        -1 where one was >= q — then every word of y[j] is 0."""
        x_in = _u64_array(x)
        if x_in.ndim not in (2, 3) or x_in.shape[-2:] != (self.cols, self.n):
            raise ValueError("x must be [cols, n] or [batch, cols, n]")
        if not 0 <= int(bound_x) < 2**64:
            raise ValueError("bound_x must be a 64-bit word")
        x3 = np.ascontiguousarray(x_in.reshape(-1, self.cols, self.n))
        out = np.empty((x3.shape[0], self.rows, self.n), dtype=np.uint64)
        status = np.empty(x3.shape[0], dtype=np.int32)
        _check(self._lib.lsr_ring_mod_matvec_bounded_batch(self._h, out.ctypes.data, status.ctypes.data, x3.ctypes.data, x3.shape[0], int(bound_x)),
               "lsr_ring_mod_matvec_bounded_batch")
        return (out[0], status[0]) if x_in.ndim == 2 else (out, status)

    def matvec_bounded_device(self, d_y, d_status, d_x, batch, bound_x=0, stream=0):
        """Device buffers: y [batch][rows][n], status [batch] int32, x [batch][cols][n].  Asynchronous on `stream`; enqueues only."""
        _check(self._lib.lsr_ring_mod_matvec_bounded_batch_device(self._h, d_y, d_status, d_x, batch, int(bound_x), stream),
               "lsr_ring_mod_matvec_bounded_batch_device")

    def close(self):
        handle = getattr(self, "_h", None)
        if handle:
            self._h = None
            self._ring._matrices.discard(self)
            # lsr_ring_mod_matrix_free reads the RingMod's handle.  A RingMod closed first has freed this matrix itself and emptied
            # the set (RingMod.close): then there is nothing left to free, and the handle must not be touched.
            if handle in self._ring._matrix_handles:
                self._ring._matrix_handles.discard(handle)
                self._lib.lsr_ring_mod_matrix_free(handle)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class _BorrowedNttContext(NttContext):
    """A context a RingMod lends (a prime context or the coefficient context): every member of NttContext, owned by the RingMod
    (close() only lets go)."""

    def __init__(self, owner, handle, q, n):   # pylint: disable=super-init-not-called
        self._lib, self._h, self._owner = owner._lib, handle, owner
        self.q, self.n = int(q), int(n)

    def close(self):
        self._h = self._owner = None

    __del__ = close


class RingMod:
    """RAII handle over ``LsrRingMod*``: the ring Z_q[X]/(X^n + 1) for any modulus q >= 2 through two NTT primes and CRT (batch.h
    "ring products under any modulus")."""

    def __init__(self, q, n, device=-1):
        self._lib = _abi.lib()
        self.q, self.n = int(q), int(n)
        if not (0 <= self.q < 2**64 and 0 <= self.n < 2**32):
            raise CoreError(f"lsr_ring_mod_create({q}, {n}): out of range")
        self._h = self._lib.lsr_ring_mod_create(self.q, self.n, device)
        if not self._h:
            raise CoreError(f"lsr_ring_mod_create({q}, {n}) returned NULL: {_abi.last_error()}")
        self._primes = ring_mod_primes(self.n)
        self._contexts = [None, None, None]      # prime 0, prime 1, the coefficient context
        self._matrices = weakref.WeakSet()
        # the native handles of the matrices still to be freed.  The WeakSet alone does not find them all: when a RingMod and its
        # matrices are collected as cyclic garbage (the frames of a traceback hold both), the weak references are cleared before any
        # finalizer runs, and the RingMod's may run first.
        self._matrix_handles = set()

    @property
    def handle(self):
        return self._h

    @property
    def primes(self):
        return self._primes

    @property
    def max_terms(self):
        return int(self._lib.lsr_ring_mod_max_terms(self._h))

    def prime_context(self, i):
        """The handle's negacyclic NttContext of prime i (0 or 1), borrowed: valid until this RingMod is closed."""
        if i not in (0, 1):
            raise ValueError("the prime index must be 0 or 1")
        if self._contexts[i] is None:
            self._contexts[i] = _BorrowedNttContext(self, self._lib.lsr_ring_mod_prime_context(self._h, i), self._primes[i], self.n)
        return self._contexts[i]

    def coeff_context(self):
        """The handle's NttContext of (q, n) itself, without twiddle tables, borrowed like the prime contexts: the coefficient-wise
        members (ring_sample, ring_challenge, ring_opnorm, ring_pack, ring_unpack, ring_decompose, ring_recompose, ring_linf,
        ring_automorphism, ring_l2sq, ring_project, ring_project_matrix, ring_project_adjoint, ring_scalar_combine, mul_pointwise) work
        on it under any q; every member that transforms raises CoreError naming the RingMod call to use."""
        if self._contexts[2] is None:
            self._contexts[2] = _BorrowedNttContext(self, self._lib.lsr_ring_mod_coeff_context(self._h), self.q, self.n)
        return self._contexts[2]

    def close(self):
        if getattr(self, "_h", None):
            for mat in list(getattr(self, "_matrices", ())):   # a matrix must not outlive its handle
                mat.close()
            handles = getattr(self, "_matrix_handles", set())
            while handles:                                     # matrices the WeakSet no longer names (see __init__): freed here,
                self._lib.lsr_ring_mod_matrix_free(handles.pop())   # and their close() finds the set empty
            for ctx in self._contexts:
                if ctx is not None:
                    ctx.close()
            self._lib.lsr_ring_mod_free(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def matrix(self, m):
        """The resident RingModMatrix of the host array m [rows, cols, n], words in [0, q); complete on return."""
        m_in = _u64_array(m)
        if m_in.ndim != 3 or m_in.shape[-1] != self.n:
            raise ValueError("m must be [rows, cols, n]")
        m3 = np.ascontiguousarray(m_in)
        handle = self._lib.lsr_ring_mod_matrix_create(self._h, m3.ctypes.data, m3.shape[0], m3.shape[1])
        if not handle:
            raise CoreError("lsr_ring_mod_matrix_create failed: " + _abi.last_error())
        return RingModMatrix(self, handle)

    def matrix_device(self, d_m, rows, cols, stream=0):
        """The same from a device buffer [rows][cols][n], enqueued on `stream`; d_m is copied and may be reused behind the stream."""
        handle = self._lib.lsr_ring_mod_matrix_create_device(self._h, d_m, rows, cols, stream)
        if not handle:
            raise CoreError("lsr_ring_mod_matrix_create_device failed: " + _abi.last_error())
        return RingModMatrix(self, handle)

    def matrix_seeded(self, key, domain, index_base, rows, cols):
        """The RingModMatrix whose entry [r][c] is the UNIFORM element mod q of stream index index_base + r cols + c under `key` (four
        uint64 words or 32 bytes), sampled on the device."""
        k2 = _ring_keys(key)
        if k2.shape[0] != 1:
            raise ValueError("key must be one 256-bit key")
        handle = self._lib.lsr_ring_mod_matrix_create_seeded(self._h, k2.ctypes.data, domain, index_base, rows, cols)
        if not handle:
            raise CoreError("lsr_ring_mod_matrix_create_seeded failed: " + _abi.last_error())
        return RingModMatrix(self, handle)

    def lift_device(self, i, d_out, d_x, count, stream=0):
        """d_out[e] = the residue mod prime i of the centred representative of d_x[e], e < count words; d_out may be d_x."""
        _check(self._lib.lsr_ring_mod_lift_batch_device(self._h, i, d_out, d_x, count, stream), "lsr_ring_mod_lift_batch_device")

    def reduce_device(self, d_out, d_r0, d_r1, count, accumulate=False, stream=0):
        """d_out[e] = (or, accumulate: += mod q) the word mod q of the centred integer with residues d_r0[e] mod p1, d_r1[e] mod p2."""
        _check(self._lib.lsr_ring_mod_reduce_batch_device(self._h, d_out, d_r0, d_r1, count, int(bool(accumulate)), stream),
               "lsr_ring_mod_reduce_batch_device")

    def mul(self, a, b):
        """a * b mod (X^n + 1, q): a is [n] or [batch, n], b is [n] (shared by every product) or [batch, n]; numpy in and out."""
        a2 = np.ascontiguousarray(_u64_array(a).reshape(-1, self.n))
        b2 = np.ascontiguousarray(_u64_array(b).reshape(-1, self.n))
        out = np.empty_like(a2)
        _check(self._lib.lsr_ring_mod_mul_batch(self._h, out.ctypes.data, a2.ctypes.data, b2.ctypes.data, a2.shape[0], b2.shape[0]), "lsr_ring_mod_mul_batch")
        return out.reshape(np.shape(a)) if np.ndim(a) == 1 else out

    def mul_device(self, d_c, d_a, d_b, batch, b_rows, stream=0):
        """Device buffers [batch][n] (b: [b_rows][n], b_rows 1 or batch), asynchronous on `stream`."""
        _check(self._lib.lsr_ring_mod_mul_batch_device(self._h, d_c, d_a, d_b, batch, b_rows, stream), "lsr_ring_mod_mul_batch_device")

    def dot(self, a, b):
        """sum_i a_i * b_i mod (X^n + 1, q): a is [terms, n] or [batch, terms, n], b is [terms, n] (shared by every output) or
        [batch, terms, n]; numpy in and out ([n] or [batch, n])."""
        a_in = _u64_array(a)
        if a_in.ndim < 2 or a_in.shape[-1] != self.n:
            raise ValueError("a must be [terms, n] or [batch, terms, n]")
        terms = a_in.shape[-2]
        if terms == 0:
            raise ValueError("terms must be at least 1")
        a3 = np.ascontiguousarray(a_in.reshape(-1, terms, self.n))
        b3 = np.ascontiguousarray(_u64_array(b).reshape(-1, terms, self.n))
        out = np.empty((a3.shape[0], self.n), dtype=np.uint64)
        _check(self._lib.lsr_ring_mod_dot_batch(self._h, out.ctypes.data, a3.ctypes.data, b3.ctypes.data, a3.shape[0], terms, b3.shape[0]),
               "lsr_ring_mod_dot_batch")
        return out[0] if a_in.ndim == 2 else out

    def dot_device(self, d_c, d_a, d_b, batch, terms, b_rows, stream=0):
        """Device buffers: c [batch][n], a [batch][terms][n], b [b_rows][terms][n] (b_rows 1 or batch), asynchronous on `stream`."""
        _check(self._lib.lsr_ring_mod_dot_batch_device(self._h, d_c, d_a, d_b, batch, terms, b_rows, stream), "lsr_ring_mod_dot_batch_device")

    def ring_dot_galois(self, a, b, g):
        """sum_i sigma_g(a_i) * b_i mod (X^n + 1, q), sigma_g: X -> X^g for odd g < 2n (n <= 4096): equal to dot on the materialised
        sigma_g(a) word for word; shapes as dot.  With g = 2n - 1, coefficient 0 is the inner product of the coefficient vectors."""
        a_in = _u64_array(a)
        if a_in.ndim < 2 or a_in.shape[-1] != self.n:
            raise ValueError("a must be [terms, n] or [batch, terms, n]")
        terms = a_in.shape[-2]
        if terms == 0:
            raise ValueError("terms must be at least 1")
        a3 = np.ascontiguousarray(a_in.reshape(-1, terms, self.n))
        b3 = np.ascontiguousarray(_u64_array(b).reshape(-1, terms, self.n))
        out = np.empty((a3.shape[0], self.n), dtype=np.uint64)
        _check(self._lib.lsr_ring_mod_dot_galois_batch(self._h, out.ctypes.data, a3.ctypes.data, b3.ctypes.data, a3.shape[0], terms, b3.shape[0], int(g)),
               "lsr_ring_mod_dot_galois_batch")
        return out[0] if a_in.ndim == 2 else out

    def ring_dot_galois_device(self, d_c, d_a, d_b, batch, terms, b_rows, g, stream=0):
        """Device buffers, shapes as dot_device.  Asynchronous on `stream`; enqueues only."""
        _check(self._lib.lsr_ring_mod_dot_galois_batch_device(self._h, d_c, d_a, d_b, batch, terms, b_rows, int(g), stream),
               "lsr_ring_mod_dot_galois_batch_device")

    def gram_prepare(self):
        """``lsr_ring_mod_gram_prepare``: allocates the Gram workspace, so that ``gram_device`` captures into a graph from the first call."""
        _check(self._lib.lsr_ring_mod_gram_prepare(self._h), "lsr_ring_mod_gram_prepare")

    def _gram_operands(self, a, b, same_shape):
        n = self.n
        a_in = _u64_array(a, "a")
        if a_in.ndim not in (3, 4) or a_in.shape[-1] != n:
            raise ValueError("a must be [ra, width, n] or [batch, ra, width, n]")
        a4 = np.ascontiguousarray(a_in.reshape(-1, a_in.shape[-3], a_in.shape[-2], n))
        if b is None:
            return a_in, a4, None
        b_in = a_in if b is a else _u64_array(b, "b")
        if b_in.ndim != a_in.ndim or b_in.shape[-1] != n or b_in.shape[-2] != a_in.shape[-2] or (same_shape and b_in.shape != a_in.shape):
            raise ValueError("b must have the shape of a" if same_shape else "b must be [rb, width, n] or [batch, rb, width, n], with the width and the rank of a")
        b4 = a4 if b_in is a_in else np.ascontiguousarray(b_in.reshape(-1, b_in.shape[-3], b_in.shape[-2], n))
        if b4.shape[0] != a4.shape[0]:
            raise ValueError("a and b must hold the same number of families")
        return a_in, a4, b4

    def gram(self, a, b=None, bound_a=0, bound_b=0):
        """g[j][i][l] = sum_c a[j][i][c] * b[j][l][c] mod (X^n + 1, q) (host arrays): a is [batch, ra, width, n], b is
        [batch, rb, width, n]; returns (g [batch, ra, rb, n], status [batch]).  b=None: the family with itself, only i <= l, packed as
        [batch, ra (ra + 1) / 2, n] (ring_gram_index).  bound_a, bound_b: the l-infinity bounds asserted on the centred operands (0:
        none); status[j] is 1 where family j kept them (exact outputs), 0 where a word exceeded its bound, -1 where a word was >= q —
        then every output word of the family is 0.  3-d operands are a batch of one, and so are the results."""
        a_in, a4, b4 = self._gram_operands(a, b, False)
        batch, ra, width = a4.shape[:3]
        rb = ra if b4 is None else b4.shape[1]
        out = np.empty((batch, ra * (ra + 1) // 2, self.n) if b4 is None else (batch, ra, rb, self.n), dtype=np.uint64)
        status = np.empty(batch, dtype=np.int32)
        _check(self._lib.lsr_ring_mod_gram_batch(self._h, out.ctypes.data, status.ctypes.data, a4.ctypes.data, None if b4 is None else b4.ctypes.data, batch,
                                                 ra, rb, width, int(bound_a), int(bound_b)), "lsr_ring_mod_gram_batch")
        return (out[0], status[0]) if a_in.ndim == 3 else (out, status)

    def gram_device(self, d_g, d_status, d_a, d_b, batch, ra, rb, width, bound_a=0, bound_b=0, stream=0):
        """Device buffers: a [batch][ra][width][n], b [batch][rb][width][n], g [batch][ra][rb][n], status [batch] int32; d_b of 0 or
        None: the symmetric form, g [batch][ra (ra + 1) / 2][n].  Asynchronous on `stream`; enqueues only."""
        _check(self._lib.lsr_ring_mod_gram_batch_device(self._h, d_g, d_status, d_a, d_b or None, batch, ra, rb, width, int(bound_a), int(bound_b), stream),
               "lsr_ring_mod_gram_batch_device")

    def gram_sym2(self, a, b, bound_a=0, bound_b=0):
        """The symmetrised packed Gram matrix of two families mod (X^n + 1, q) (host arrays): a and b are [batch, r, width, n]; returns
        (h [batch, r (r + 1) / 2, n], status [batch]) with h[j][(i, l)] = <a_i, b_l> + <a_l, b_i> for i < l and <a_i, b_i> on the
        diagonal (ring_gram_index); bounds and status as ``gram``."""
        if b is None:
            raise ValueError("gram_sym2 takes two families")
        a_in, a4, b4 = self._gram_operands(a, b, True)
        batch, r, width = a4.shape[:3]
        out = np.empty((batch, r * (r + 1) // 2, self.n), dtype=np.uint64)
        status = np.empty(batch, dtype=np.int32)
        _check(self._lib.lsr_ring_mod_gram_sym2_batch(self._h, out.ctypes.data, status.ctypes.data, a4.ctypes.data, b4.ctypes.data, batch, r, width,
                                                      int(bound_a), int(bound_b)), "lsr_ring_mod_gram_sym2_batch")
        return (out[0], status[0]) if a_in.ndim == 3 else (out, status)

    def gram_sym2_device(self, d_h, d_status, d_a, d_b, batch, r, width, bound_a=0, bound_b=0, stream=0):
        """Device buffers: a and b [batch][r][width][n] (d_b may be d_a), h [batch][r (r + 1) / 2][n], status [batch] int32.
        Asynchronous on `stream`; enqueues only."""
        _check(self._lib.lsr_ring_mod_gram_sym2_batch_device(self._h, d_h, d_status, d_a, d_b or None, batch, r, width, int(bound_a), int(bound_b), stream),
               "lsr_ring_mod_gram_sym2_batch_device")

    def fold(self, v, p, term_stride=0, bound_v=0, bound_p=0):
        """out[j][c] = sum_i p[j][i] * v[j term_stride + i][c] mod (X^n + 1, q) (host arrays, n <= 4096): v is [vectors, width, n], p is
        [outputs, terms, n] (or [terms, n]: one output) with vectors >= (outputs - 1) term_stride + terms, as ``NttContext.ring_fold``.
        Returns (out [outputs, width, n], status [outputs]) — ([width, n], status) for a 2-d p.  bound_v, bound_p: the l-infinity
        bounds asserted on the centred words of v and p (0: none); status[j] is 1 where every word output j reads kept them (exact
        output), 0 where one exceeded its bound, -1 where one was >= q — then every word of out[j] is 0."""
        n = self.n
        v_in, p_in = _u64_array(v, "v"), _u64_array(p, "p")
        if v_in.ndim != 3 or v_in.shape[-1] != n:
            raise ValueError("v must be [vectors, width, n]")
        if p_in.ndim not in (2, 3) or p_in.shape[-1] != n:
            raise ValueError("p must be [terms, n] or [outputs, terms, n]")
        terms, term_stride = p_in.shape[-2], int(term_stride)
        if terms == 0:
            raise ValueError("terms must be at least 1")
        v3, p3 = np.ascontiguousarray(v_in), np.ascontiguousarray(p_in.reshape(-1, terms, n))
        outputs, width = p3.shape[0], v3.shape[1]
        if term_stride < 0 or (outputs and v3.shape[0] < (outputs - 1) * term_stride + terms):
            raise ValueError("v must hold (outputs - 1) * term_stride + terms vectors")
        out = np.empty((outputs, width, n), dtype=np.uint64)
        status = np.empty(outputs, dtype=np.int32)
        _check(self._lib.lsr_ring_mod_fold_batch(self._h, out.ctypes.data, status.ctypes.data, v3.ctypes.data, p3.ctypes.data, outputs, terms, term_stride,
                                                 width, int(bound_v), int(bound_p)), "lsr_ring_mod_fold_batch")
        return (out[0], status[0]) if p_in.ndim == 2 else (out, status)

    def fold_device(self, d_out, d_status, d_v, d_p, outputs, terms, term_stride, width, bound_v=0, bound_p=0, stream=0):
        """Device buffers: out [outputs][width][n], status [outputs] int32, v [(outputs - 1) term_stride + terms][width][n],
        p [outputs][terms][n].  Asynchronous on `stream`; enqueues only."""
        _check(self._lib.lsr_ring_mod_fold_batch_device(self._h, d_out, d_status, d_v, d_p, outputs, terms, term_stride, width, int(bound_v), int(bound_p),
                                                        stream), "lsr_ring_mod_fold_batch_device")

    def respond(self, v, p, y=None, term_stride=0, bound_y=0, bound_v=0, bound_p=0, bound_z=0):
        """The masked response z[j] = y[j] + sum_i p[j][i] * v[j term_stride + i] mod (X^n + 1, q) with its abort (host arrays,
        n <= 4096): v and p as ``fold`` takes them, y [outputs, width, n] ([width, n] for a 2-d p) or None for no mask.
        Returns (out [outputs, width, n], status [outputs]) — ([width, n], status) for a 2-d p.  The bounds are l-infinity bounds on
        centred words (0: none).  status[j] is 1 where out[j] = z[j] was accepted; 2 (RING_RESPOND_REJECTED) where the inputs were
        fine but a word of z[j] exceeded bound_z; 0 where a word of v, p or y exceeded its bound; -1 where one was >= q.  For every
        status other than 1 every word of out[j] is 0."""
        n = self.n
        v_in, p_in = _u64_array(v, "v"), _u64_array(p, "p")
        if v_in.ndim != 3 or v_in.shape[-1] != n:
            raise ValueError("v must be [vectors, width, n]")
        if p_in.ndim not in (2, 3) or p_in.shape[-1] != n:
            raise ValueError("p must be [terms, n] or [outputs, terms, n]")
        terms, term_stride = p_in.shape[-2], int(term_stride)
        if terms == 0:
            raise ValueError("terms must be at least 1")
        v3, p3 = np.ascontiguousarray(v_in), np.ascontiguousarray(p_in.reshape(-1, terms, n))
        outputs, width = p3.shape[0], v3.shape[1]
        if term_stride < 0 or (outputs and v3.shape[0] < (outputs - 1) * term_stride + terms):
            raise ValueError("v must hold (outputs - 1) * term_stride + terms vectors")
        y3 = None
        if y is not None:
            y3 = np.ascontiguousarray(_u64_array(y, "y"))
            if y3.shape != ((width, n) if p_in.ndim == 2 else (outputs, width, n)):
                raise ValueError("y must be [outputs, width, n] ([width, n] for a 2-d p)")
        out = np.empty((outputs, width, n), dtype=np.uint64)
        status = np.empty(outputs, dtype=np.int32)
        _check(self._lib.lsr_ring_mod_respond_batch(self._h, out.ctypes.data, status.ctypes.data, None if y3 is None else y3.ctypes.data, v3.ctypes.data,
                                                    p3.ctypes.data, outputs, terms, term_stride, width, int(bound_y), int(bound_v), int(bound_p),
                                                    int(bound_z)), "lsr_ring_mod_respond_batch")
        return (out[0], status[0]) if p_in.ndim == 2 else (out, status)

    def respond_device(self, d_out, d_status, d_y, d_v, d_p, outputs, terms, term_stride, width, bound_y=0, bound_v=0, bound_p=0, bound_z=0, stream=0):
        """Device buffers: out [outputs][width][n], status [outputs] int32, y as out (0: no mask; d_out itself: in place), v and p
        as ``fold_device`` takes them.  Asynchronous on `stream`; enqueues only."""
        _check(self._lib.lsr_ring_mod_respond_batch_device(self._h, d_out, d_status, d_y or None, d_v, d_p, outputs, terms, term_stride, width, int(bound_y),
                                                           int(bound_v), int(bound_p), int(bound_z), stream), "lsr_ring_mod_respond_batch_device")

    def quadform(self, g, c, offdiag=2, bound_g=0, bound_c=0):
        """out[j] = sum_i g[j][(i, i)] c_i c_i + offdiag * sum_{i < l} g[j][(i, l)] c_i c_l mod (X^n + 1, q) (host arrays, DESIGN.md
        §5u): g is [batch, r (r + 1) / 2, n] in the packed order of ``gram(s)`` and ``gram_sym2`` (ring_gram_index), c is [batch, r, n],
        or [r, n]: one set of challenges shared by every family.  Returns (out [batch, n], status [batch]) — ([n], status) for a 2-d g.
        offdiag: a word below q — 2 for a gram(s), 1 for a gram_sym2(phi, s).  bound_g, bound_c: the l-infinity bounds asserted on the
        centred words of g and c (0: none); status[j] is 1 where every word family j reads kept them (exact output), 0 where one
        exceeded its bound, -1 where one was >= q — then every word of out[j] is 0."""
        n = self.n
        g_in, c_in = _u64_array(g, "g"), _u64_array(c, "c")
        if g_in.ndim not in (2, 3) or g_in.shape[-1] != n:
            raise ValueError("g must be [pairs, n] or [batch, pairs, n]")
        if c_in.ndim not in (2, 3) or c_in.shape[-1] != n:
            raise ValueError("c must be [r, n] or [batch, r, n]")
        r, pairs = c_in.shape[-2], g_in.shape[-2]
        if pairs != r * (r + 1) // 2:
            raise ValueError("g must hold r (r + 1) / 2 polynomials per family for the r polynomials of c")
        g3 = np.ascontiguousarray(g_in.reshape(-1, pairs, n))
        c3 = np.ascontiguousarray(c_in.reshape(-1, r, n))
        batch, c_rows = g3.shape[0], (1 if c_in.ndim == 2 else c3.shape[0])
        if c_rows not in (1, batch):
            raise ValueError("c must hold one set of challenges ([r, n]) or one per family of g")
        out = np.empty((batch, n), dtype=np.uint64)
        status = np.empty(batch, dtype=np.int32)
        _check(self._lib.lsr_ring_mod_quadform_batch(self._h, out.ctypes.data, status.ctypes.data, g3.ctypes.data, c3.ctypes.data, batch, r, c_rows,
                                                     int(offdiag), int(bound_g), int(bound_c)), "lsr_ring_mod_quadform_batch")
        return (out[0], status[0]) if g_in.ndim == 2 else (out, status)

    def quadform_device(self, d_out, d_status, d_g, d_c, batch, r, c_rows, offdiag=2, bound_g=0, bound_c=0, stream=0):
        """Device buffers: g [batch][r (r + 1) / 2][n], c [c_rows][r][n] with c_rows 1 or batch, out [batch][n], status [batch] int32.
        Asynchronous on `stream`; enqueues only."""
        _check(self._lib.lsr_ring_mod_quadform_batch_device(self._h, d_out, d_status, d_g, d_c, batch, r, c_rows, int(offdiag), int(bound_g), int(bound_c),
                                                            stream), "lsr_ring_mod_quadform_batch_device")



class Params:
    """Mirror of lambda_snark_core::Params (rust-api/lambda-snark-core/src/lib.rs:136-196), RingB profile."""

    def __init__(self, security_level=128, q=17592186044417, n=4096, k=2, sigma=3.19, profile=PROFILE_RING_B):
        self.security_level, self.q, self.n, self.k, self.sigma, self.profile = security_level, q, n, k, sigma, profile

    def to_ffi(self):
        # context.rs:18-42: ScalarA is sent as ring_degree = 1, module_rank = 1
        if self.profile == PROFILE_SCALAR_A:
            return PublicParams(PROFILE_SCALAR_A, self.security_level, self.q, 1, 1, self.sigma)
        return PublicParams(PROFILE_RING_B, self.security_level, self.q, self.n, self.k, self.sigma)


class LweContext:
    """Mirror of lambda_snark::LweContext (context.rs:14-76)."""

    def __init__(self, params, key_seed=None, device=-1):
        self._lib = _abi.lib()
        self.params = params
        ffi = params.to_ffi()
        if key_seed is None and device < 0:
            self._h = self._lib.lwe_context_create(ctypes.byref(ffi))
        else:
            self._h = self._lib.lsr_lwe_context_create_seeded(ctypes.byref(ffi), int(key_seed or 0), device)
        if not self._h:
            raise CoreError("FfiError: lwe_context_create returned NULL")   # context.rs:46-48

    @classmethod
    def create_rns(cls, params, key_seed=None, device=-1):
        """``lsr_lwe_context_create_rns``: a two-prime RNS context (``params.q`` is ignored) whose ``linear_combine`` takes any
        coefficient below the plaintext modulus, as the reference does; commitments and openings go through the same wrappers."""
        self = object.__new__(cls)
        self._lib, self.params = _abi.lib(), params
        ffi = params.to_ffi()
        self._h = self._lib.lsr_lwe_context_create_rns(ctypes.byref(ffi), int(key_seed or 0), device)
        if not self._h:
            raise CoreError("FfiError: lsr_lwe_context_create_rns returned NULL: " + _abi.last_error())
        return self

    def rns_moduli(self):
        """``lsr_lwe_rns_moduli``: (q1, q2) of an RNS context, None on any other context."""
        out = (ctypes.c_uint64 * 2)()
        if self._lib.lsr_lwe_rns_moduli(self._h, out) != 0:
            return None
        return int(out[0]), int(out[1])

    @property
    def handle(self):
        return self._h

    def modulus(self):
        """context.rs:90 returns params.q; the ring modulus actually used is ``commit_modulus``."""
        return self.params.q

    @property
    def commit_modulus(self):
        return self._lib.lsr_lwe_modulus(self._h)

    @property
    def plain_modulus(self):
        return self._lib.lsr_lwe_plain_modulus(self._h)

    @property
    def ring_degree(self):
        return self._lib.lsr_lwe_ring_degree(self._h)

    @property
    def module_rank(self):
        return self._lib.lsr_lwe_module_rank(self._h)

    @property
    def pipeline(self):
        """``lsr_lwe_pipeline``: which kernels this context's commitments and openings run on ("tile", "fused", "fused-matvec", "general")."""
        return self._lib.lsr_lwe_pipeline(self._h).decode()

    @property
    def commitment_words(self):
        return self._lib.lsr_lwe_commitment_words(self._h)

    def commit_keys(self, messages, seeds):
        """``lsr_lwe_commit_keys``: the per-commitment 256-bit stream keys exactly as ``lwe_commit`` derives them (seed 0: fresh entropy),
        [batch][4] uint64 — the input of the device-resident ``lsr_lwe_commit_rows_device``."""
        messages = np.ascontiguousarray(messages, dtype=np.uint64)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        if messages.ndim != 2 or messages.shape[0] != seeds.size:
            raise ValueError("messages must be [batch][msg_len] with one seed per row")
        keys = np.zeros((seeds.size, 4), dtype=np.uint64)
        rc = self._lib.lsr_lwe_commit_keys(self._h, messages.ctypes.data if messages.size else None, messages.shape[1], seeds.size, seeds.ctypes.data,
                                           keys.ctypes.data)
        if rc != 0:
            raise CoreError("lsr_lwe_commit_keys failed: " + _abi.last_error())
        return keys

    def commit_keys_device(self, d_messages, msg_len, seeds, d_keys, stream):
        """``lsr_lwe_commit_keys_device``: the same keys derived on the device from device-resident messages (seeds: host array, all
        non-zero), asynchronous on `stream`."""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        if self._lib.lsr_lwe_commit_keys_device(self._h, d_messages, msg_len, seeds.size, seeds.ctypes.data, d_keys, stream) != 0:
            raise CoreError("lsr_lwe_commit_keys_device failed: " + _abi.last_error())

    def commit_rows_device(self, d_messages, msg_len, batch, d_keys, d_rows, stream):
        """``lsr_lwe_commit_rows_device``: device pointers (ints) in, wire rows out, asynchronous on `stream`."""
        if self._lib.lsr_lwe_commit_rows_device(self._h, d_messages, msg_len, batch, d_keys, d_rows, stream) != 0:
            raise CoreError("CommitmentFailed: " + _abi.last_error())

    def verify_rows_device(self, d_rows, d_messages, msg_len, count, d_results, stream):
        """``lsr_lwe_verify_rows_device``: int32 verdicts (1 / 0 / -1 as ``lwe_verify_opening``) per row, asynchronous on `stream`."""
        if self._lib.lsr_lwe_verify_rows_device(self._h, d_rows, d_messages, msg_len, count, d_results, stream) != 0:
            raise CoreError("VerificationFailed: " + _abi.last_error())

    @property
    def noise_capacity_bits(self):
        """``lsr_lwe_noise_capacity_bits``: a row stops decoding to its message when its ``noise_bits`` reaches this."""
        return self._lib.lsr_lwe_noise_capacity_bits(self._h)

    def decode_rows_device(self, d_rows, count, slots, d_messages, d_status, d_noise_bits, stream):
        """``lsr_lwe_decode_rows_device``: device pointers (ints) in; the first `slots` plaintext slots of every row, int32 status
        (1 / -1) and, unless `d_noise_bits` is None, uint32 noise bit lengths out; asynchronous on `stream`."""
        if self._lib.lsr_lwe_decode_rows_device(self._h, d_rows, count, slots, d_messages, d_status, d_noise_bits, stream) != 0:
            raise CoreError("DecodeFailed: " + _abi.last_error())

    def decode_rows(self, rows, slots=None, noise=False):
        """``lsr_lwe_decode_batch_flat``: rows [count][words] (host) -> (messages [count][slots], status [count]) and, with `noise`,
        noise_bits [count]; `slots` defaults to the ring degree."""
        rows = _u64_array(rows, "rows")
        if rows.ndim != 2 or rows.shape[1] != self.commitment_words:
            raise ValueError("rows must be [count][commitment_words]")
        slots = self.ring_degree if slots is None else int(slots)
        count = rows.shape[0]
        messages = np.zeros((count, max(slots, 0)), dtype=np.uint64)
        status = np.zeros(count, dtype=np.int32)
        bits = np.zeros(count, dtype=np.uint32)
        if self._lib.lsr_lwe_decode_batch_flat(self._h, rows.ctypes.data, count, slots, messages.ctypes.data, status.ctypes.data,
                                               bits.ctypes.data if noise else None) != 0:
            raise CoreError("DecodeFailed: " + _abi.last_error())
        return (messages, status, bits) if noise else (messages, status)

    def combine_rows_device(self, d_rows, terms, d_coeffs, outputs, d_out_rows, d_status, term_stride=0, stream=None):
        """``lsr_lwe_combine_rows_device``: device pointers (ints) in; out_j = sum_i c'_{j,i} row[j * term_stride + i] for j < outputs
        and int32 status (1 combined / 0 over the noise budget / -1 a malformed term row) out; asynchronous on `stream`."""
        if self._lib.lsr_lwe_combine_rows_device(self._h, d_rows, terms, term_stride, d_coeffs, outputs, d_out_rows, d_status, stream) != 0:
            raise CoreError("CombineFailed: " + _abi.last_error())

    def combine_rows(self, rows, coeffs, term_stride=0):
        """``lsr_lwe_combine_batch_flat``: rows [(outputs - 1) * term_stride + terms][words] and coeffs [outputs][terms] (host) ->
        (out_rows [outputs][words], status [outputs])."""
        rows = _u64_array(rows, "rows")
        coeffs = _u64_array(coeffs, "coeffs")
        if rows.ndim != 2 or rows.shape[1] != self.commitment_words:
            raise ValueError("rows must be [count][commitment_words]")
        if coeffs.ndim != 2:
            raise ValueError("coeffs must be [outputs][terms]")
        outputs, terms = coeffs.shape
        if outputs and rows.shape[0] != (outputs - 1) * int(term_stride) + terms:
            raise ValueError("rows must hold (outputs - 1) * term_stride + terms rows")
        out = np.zeros((outputs, rows.shape[1]), dtype=np.uint64)
        status = np.zeros(outputs, dtype=np.int32)
        if self._lib.lsr_lwe_combine_batch_flat(self._h, rows.ctypes.data, terms, int(term_stride), coeffs.ctypes.data, outputs, out.ctypes.data,
                                                status.ctypes.data) != 0:
            raise CoreError("CombineFailed: " + _abi.last_error())
        return out, status

    @property
    def combine_max_weight(self):
        """``lsr_lwe_combine_max_weight``: the largest weight (sum of |c'|, for ring elements over every coefficient) that
        ``combine_rows`` and ``ring_combine_rows`` accept on this context."""
        return self._lib.lsr_lwe_combine_max_weight(self._h)

    def ring_combine_rows_device(self, d_rows, terms, d_polys, outputs, d_out_rows, d_status, term_stride=0, stream=None):
        """``lsr_lwe_ring_combine_rows_device``: device pointers (ints) in; out_j = sum_i p'_{j,i}(X) row[j * term_stride + i] in
        Z_q[X]/(X^n + 1) for j < outputs, d_polys = [outputs][terms][n] coefficient words (reduced mod t and centred), and int32 status
        (1 combined / 0 over the noise budget / -1 a malformed term row) out; asynchronous on `stream`."""
        if self._lib.lsr_lwe_ring_combine_rows_device(self._h, d_rows, terms, term_stride, d_polys, outputs, d_out_rows, d_status, stream) != 0:
            raise CoreError("RingCombineFailed: " + _abi.last_error())

    def ring_combine_rows(self, rows, polys, term_stride=0):
        """``lsr_lwe_ring_combine_batch_flat``: rows [(outputs - 1) * term_stride + terms][words] and polys [outputs][terms][n] (host) ->
        (out_rows [outputs][words], status [outputs])."""
        rows = _u64_array(rows, "rows")
        polys = _u64_array(polys, "polys")
        if rows.ndim != 2 or rows.shape[1] != self.commitment_words:
            raise ValueError("rows must be [count][commitment_words]")
        if polys.ndim != 3 or polys.shape[2] != self.ring_degree:
            raise ValueError("polys must be [outputs][terms][ring_degree]")
        outputs, terms = polys.shape[:2]
        if outputs and rows.shape[0] != (outputs - 1) * int(term_stride) + terms:
            raise ValueError("rows must hold (outputs - 1) * term_stride + terms rows")
        out = np.zeros((outputs, rows.shape[1]), dtype=np.uint64)
        status = np.zeros(outputs, dtype=np.int32)
        if self._lib.lsr_lwe_ring_combine_batch_flat(self._h, rows.ctypes.data, terms, int(term_stride), polys.ctypes.data, outputs, out.ctypes.data,
                                                     status.ctypes.data) != 0:
            raise CoreError("RingCombineFailed: " + _abi.last_error())
        return out, status

    def public_matrix(self):
        k, n = self.module_rank, self.ring_degree
        a = np.zeros((k, k, n), dtype=np.uint64)
        if self._lib.lsr_lwe_public_matrix(self._h, a.ctypes.data) != 0:
            raise CoreError("lsr_lwe_public_matrix failed")
        return a

    def replicate(self, device=-1):
        """``lsr_lwe_context_replicate``: the same context (same keys) on another device, for sharded runs."""
        twin = object.__new__(LweContext)
        twin._lib, twin.params = self._lib, self.params
        twin._h = self._lib.lsr_lwe_context_replicate(self._h, device)
        if not twin._h:
            raise CoreError("FfiError: lsr_lwe_context_replicate returned NULL")
        return twin

    def close(self):
        if getattr(self, "_h", None):
            self._lib.lwe_context_free(self._h)
            self._h = None

    __del__ = close


class PinnedArray:
    """A uint64 host array in page-locked memory (``lsr_host_alloc_pinned``): the single gather target of a sharded call."""

    def __init__(self, shape):
        self._lib = _abi.lib()
        self.shape = tuple(int(x) for x in shape)
        count = int(np.prod(self.shape))
        self._p = self._lib.lsr_host_alloc_pinned(max(count, 1) * 8)
        if not self._p:
            raise MemoryError("lsr_host_alloc_pinned failed")
        self.array = np.ctypeslib.as_array(ctypes.cast(self._p, ctypes.POINTER(ctypes.c_uint64)), shape=(count,)).reshape(self.shape)

    @property
    def ptr(self):
        return self._p

    def close(self):
        if getattr(self, "_p", None):
            self.array = None
            self._lib.lsr_host_free_pinned(self._p)
            self._p = None

    __del__ = close


def shard_bounds(batch, shards, index):
    """``lsr_shard_bounds`` -> (first, count) of shard `index`."""
    first, count = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _abi.lib().lsr_shard_bounds(batch, shards, index, ctypes.byref(first), ctypes.byref(count))
    return first.value, count.value


def _handles(ctxs):
    return (ctypes.c_void_p * len(ctxs))(*[c.handle for c in ctxs])


def sharded_ntt(ctxs, polys, inverse=False):
    """``lsr_ntt_forward_batch_sharded`` / ``_inverse_``: `polys` is ONE host array [batch][n], transformed in place."""
    lib = _abi.lib()
    fn = lib.lsr_ntt_inverse_batch_sharded if inverse else lib.lsr_ntt_forward_batch_sharded
    if fn(_handles(ctxs), len(ctxs), polys.ctypes.data, polys.shape[0]) != 0:
        raise CoreError("sharded transform failed: " + _abi.last_error())
    return polys


def sharded_commit_words(ctxs, messages, seeds, out=None):
    """``lsr_lwe_commit_batch_flat_sharded``: rows [batch][words] written into `out` (a host array, e.g. ``PinnedArray.array``)."""
    lib = _abi.lib()
    msgs = _u64_array(messages, "messages")
    sd = _u64_array(seeds, "seeds")
    if out is None:
        out = np.zeros((msgs.shape[0], lib.lsr_lwe_commitment_words(ctxs[0].handle)), dtype=np.uint64)
    if lib.lsr_lwe_commit_batch_flat_sharded(_handles(ctxs), len(ctxs), msgs.ctypes.data, msgs.shape[1], msgs.shape[0], sd.ctypes.data, out.ctypes.data) != 0:
        raise CoreError("CommitmentFailed: " + _abi.last_error())
    return out


def sharded_matvec(ctxs, d_r_ptrs, d_e1_ptrs, batch, host_u):
    """``lsr_mlwe_matvec_batch_sharded``: device-resident inputs per shard, gather into the host array `host_u`;
    returns (longest kernel time of a shard's slice, longest wall time until a slice is in host memory), seconds."""
    lib = _abi.lib()
    r = (ctypes.c_void_p * len(ctxs))(*d_r_ptrs)
    e = (ctypes.c_void_p * len(ctxs))(*d_e1_ptrs)
    seconds = (ctypes.c_double * 2)()
    if lib.lsr_mlwe_matvec_batch_sharded(_handles(ctxs), len(ctxs), r, e, batch, host_u.ctypes.data, seconds) != 0:
        raise CoreError("sharded matvec failed: " + _abi.last_error())
    return seconds[0], seconds[1]


def sharded_matvec_stats(ctxs, d_r_ptrs, d_e1_ptrs, batch, host_u):
    """``lsr_mlwe_matvec_batch_sharded_stats``: the same call, returning [(kernel seconds, wall seconds until gathered)] per shard."""
    lib = _abi.lib()
    r = (ctypes.c_void_p * len(ctxs))(*d_r_ptrs)
    e = (ctypes.c_void_p * len(ctxs))(*d_e1_ptrs)
    stats = (ctypes.c_double * (2 * len(ctxs)))()
    if lib.lsr_mlwe_matvec_batch_sharded_stats(_handles(ctxs), len(ctxs), r, e, batch, host_u.ctypes.data, stats) != 0:
        raise CoreError("sharded matvec failed: " + _abi.last_error())
    return [(stats[2 * g], stats[2 * g + 1]) for g in range(len(ctxs))]


class Commitment:
    """Mirror of lambda_snark::Commitment (commitment.rs:31-121)."""

    def __init__(self, ctx, message=None, seed=0, _raw=None):
        self._lib = _abi.lib()
        self._ctx = ctx
        if _raw is not None:
            self._p = _raw
            return
        # commitment.rs:33-36: every coefficient is reduced mod ctx.modulus() before the call
        if isinstance(message, np.ndarray) and message.dtype == np.uint64 and message.ndim == 1:    # (a 2^22-word quotient: no Python loop)
            msg = np.ascontiguousarray(message % np.uint64(ctx.modulus()))
        else:
            msg = np.array([int(m) % ctx.modulus() for m in message], dtype=np.uint64)
        self._p = self._lib.lwe_commit(ctx.handle, msg.ctypes.data, msg.size, int(seed))
        if not self._p:
            raise CoreError("CommitmentFailed")   # commitment.rs:40-42

    @classmethod
    def batch(cls, ctx, messages, seeds):
        """``lwe_commit_batch``: messages [batch][msg_len], seeds [batch]."""
        lib = _abi.lib()
        msgs = np.ascontiguousarray(messages, dtype=np.uint64)
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        out = (ctypes.POINTER(LweCommitment) * msgs.shape[0])()
        if lib.lwe_commit_batch(ctx.handle, msgs.ctypes.data, msgs.shape[1], msgs.shape[0], seeds.ctypes.data, out) != 0:
            raise CoreError("CommitmentFailed: " + _abi.last_error())
        return [cls(ctx, _raw=out[i]) for i in range(msgs.shape[0])]

    @staticmethod
    def batch_words(ctx, messages, seeds):
        """``lsr_lwe_commit_batch_flat``: the same commitments as ``batch`` as one [batch][words] array (no per-commitment
        allocation)."""
        lib = _abi.lib()
        msgs = _u64_array(messages, "messages")
        if msgs.ndim != 2:
            raise ValueError("messages must be [batch][msg_len]")
        sd = _u64_array(seeds, "seeds")
        out = np.zeros((msgs.shape[0], lib.lsr_lwe_commitment_words(ctx.handle)), dtype=np.uint64)
        if lib.lsr_lwe_commit_batch_flat(ctx.handle, msgs.ctypes.data, msgs.shape[1], msgs.shape[0], sd.ctypes.data, out.ctypes.data) != 0:
            raise CoreError("CommitmentFailed: " + _abi.last_error())
        return out

    def clone(self):
        p = self._lib.lwe_commitment_clone(self._p)
        if not p:
            raise CoreError("lwe_commitment_clone returned NULL")   # commitment.rs:22-24 panics
        return Commitment(self._ctx, _raw=p)

    @staticmethod
    def linear_combine(ctx, commitments, coeffs):
        """commitment.rs:60-84 (coefficients reduced mod ctx.modulus() first, :66-69)."""
        if len(commitments) == 0:
            raise ValueError("no commitments provided")                     # commitment.rs:66-68
        if len(commitments) != len(coeffs):
            raise ValueError("commitments/coeffs length mismatch")          # commitment.rs:70-74
        lib = _abi.lib()
        arr = (ctypes.POINTER(LweCommitment) * len(commitments))(*[c._p if c is not None else None for c in commitments])
        cf = np.array([int(c) % ctx.modulus() for c in coeffs], dtype=np.uint64)
        p = lib.lwe_linear_combine(ctx.handle, arr, cf.ctypes.data, len(commitments))
        if not p:
            raise CoreError("CommitmentFailed")   # commitment.rs:80-82
        return Commitment(ctx, _raw=p)

    def decode(self, ctx, slots=None, noise=False):
        """``lsr_lwe_decode``: the first `slots` plaintext slots this commitment opens to under `ctx` (default: all of them), with
        `noise` also its noise bit length; raises when the commitment is not a canonical row of `ctx`."""
        slots = ctx.ring_degree if slots is None else int(slots)
        message = np.zeros(max(slots, 1), dtype=np.uint64)
        bits = ctypes.c_uint32(0)
        if self._lib.lsr_lwe_decode(ctx.handle, self._p, message.ctypes.data, slots, ctypes.byref(bits) if noise else None) != 1:
            raise CoreError("DecodeFailed: " + _abi.last_error())
        message = message[:slots]
        return (message, int(bits.value)) if noise else message

    def as_words(self):
        """commitment.rs:88-93: the flat u64 words (hashed word-by-word by the Fiat–Shamir transcript)."""
        c = self._p.contents
        return np.ctypeslib.as_array(c.data, shape=(c.len,)).copy()

    def as_bytes(self):
        return self.as_words().tobytes()

    def serialize(self):
        """The bincode form of the Rust type (commitment.rs:112-121, pinned by tests/serialization.rs:128-153): a u64
        element count followed by the words, little endian.  There is no deserialisation (it needs an LweContext)."""
        words = self.as_words()
        return int(words.size).to_bytes(8, "little") + words.astype("<u8").tobytes()

    def __len__(self):
        return self._p.contents.len

    def free(self):
        if getattr(self, "_p", None):
            self._lib.lwe_commitment_free(self._p)
            self._p = None

    __del__ = free


def rns_commit_moduli(ring_degree):
    """``lsr_rns_commit_moduli``: the (q1, q2) an RNS context of this ring degree commits under (host only)."""
    out = (ctypes.c_uint64 * 2)()
    if _abi.lib().lsr_rns_commit_moduli(int(ring_degree), out) != 0:
        raise ValueError("unsupported ring degree")
    return int(out[0]), int(out[1])


def wide_modulus(ring_degree):
    """``lsr_lwe_wide_modulus``: the 60-bit NTT prime to pass as ``Params.q`` for reference-range linear combinations."""
    return int(_abi.lib().lsr_lwe_wide_modulus(int(ring_degree)))


def words_to_limbs(words, limb_bits=16, limbs_per_word=4):
    """``lsr_words_to_limbs``: little-endian limbs of field elements wider than the plaintext modulus, so that a commitment
    binds them in full (a message word >= t is embedded mod t and never opens — commitment.cpp:152,223-226)."""
    lib = _abi.lib()
    w = _u64_array(words, "words").ravel()
    out = np.zeros(w.size * limbs_per_word, dtype=np.uint64)
    if lib.lsr_words_to_limbs(w.ctypes.data, w.size, limb_bits, limbs_per_word, out.ctypes.data) != out.size:
        raise ValueError("invalid limb parameters")
    return out


def verify_opening_with_context(ctx, commitment, message, randomness=None):
    """opening.rs:160-222 -> ``lwe_verify_opening``; returns True/False, raises on -1."""
    lib = _abi.lib()
    msg = np.array([int(m) % ctx.modulus() for m in message], dtype=np.uint64)   # opening.rs:198-201
    rnd = np.zeros(1, dtype=np.uint64) if randomness is None else _u64_array(randomness)
    opening = LweOpening(rnd.ctypes.data_as(_abi.u64p), rnd.size)
    rc = lib.lwe_verify_opening(ctx.handle, commitment._p, msg.ctypes.data, msg.size, ctypes.byref(opening))
    if rc < 0:
        raise CoreError("lwe_verify_opening returned -1")
    return rc == 1


def verify_openings_batch(ctx, commitments, messages):
    """``lwe_verify_opening_batch``: messages [count][msg_len] (reduced mod ctx.modulus() like opening.rs:198-201);
    returns a list of 1 / 0 / -1."""
    lib = _abi.lib()
    msgs = np.ascontiguousarray([[int(m) % ctx.modulus() for m in row] for row in messages], dtype=np.uint64)
    arr = (ctypes.POINTER(LweCommitment) * len(commitments))(*[c._p if c is not None else None for c in commitments])
    out = np.zeros(len(commitments), dtype=np.int32)
    if lib.lwe_verify_opening_batch(ctx.handle, arr, msgs.ctypes.data, msgs.shape[1] if msgs.ndim == 2 else 0, len(commitments), out.ctypes.data) != 0:
        raise CoreError("lwe_verify_opening_batch failed: " + _abi.last_error())
    return [int(x) for x in out]


def verify_openings_words(ctx, words, messages):
    """``lsr_lwe_verify_opening_batch_flat``: commitments as rows of one array (``Commitment.batch_words``)."""
    lib = _abi.lib()
    rows = _u64_array(words, "words")
    msgs = _u64_array(messages, "messages")
    count = rows.shape[0] if rows.ndim == 2 else 0
    out = np.zeros(count, dtype=np.int32)
    if count and lib.lsr_lwe_verify_opening_batch_flat(ctx.handle, rows.ctypes.data, msgs.ctypes.data, msgs.shape[1] if msgs.ndim == 2 else 0, count,
                                                       out.ctypes.data) != 0:
        raise CoreError("lsr_lwe_verify_opening_batch_flat failed: " + _abi.last_error())
    return [int(x) for x in out]


def sample_gaussian(length, sigma, seed=None, domain=16, index=0):
    """``sample_gaussian`` (utils.h:27) or its seeded twin; returns int64 samples."""
    lib = _abi.lib()
    out = np.zeros(length, dtype=np.uint64)
    if seed is None:
        rc = lib.sample_gaussian(out.ctypes.data, length, float(sigma))
    else:
        rc = lib.lsr_sample_gaussian_seeded(out.ctypes.data, length, float(sigma), int(seed), int(domain), int(index))
    if rc != 0:
        raise CoreError("sample_gaussian failed")
    return out.view(np.int64)


# ---- prover-side polynomial path (include/lambda_snark/prover.h) -------------------------------------------------
NTT_MODULUS = 18446744069414584321          # rust-api/lambda-snark-core/src/lib.rs:58
NTT_PRIMITIVE_ROOT = 1753635133440165772    # lib.rs:78


def compute_root_of_unity(n, modulus=NTT_MODULUS, primitive_root=NTT_PRIMITIVE_ROOT):
    """rust-api/lambda-snark/src/ntt.rs:226-233 (host integer arithmetic only)."""
    if n <= 0 or n & (n - 1) or n > 1 << 32:
        raise ValueError("n must be power of 2, n <= 2^32")
    return pow(primitive_root, (1 << 32) // n, modulus)


MAX_TWO_PASS_SIZE = 1 << 17   # above it the *_large constructors (prover.h): n, m up to 2^lsr_prover_max_log2_size() = 2^22


def prover_max_log2_size():
    """``lsr_prover_max_log2_size``: log2 of the largest cyclic transform / constraint count (22)."""
    return int(_abi.lib().lsr_prover_max_log2_size())


class CyclicNtt(_RingGadget, _RingSample, _RingChallenge, _RingPack, _RingFold, _RingGalois, _RingNorm, _RingScalar, _RingGram):
    """The transform pair of rust-api/lambda-snark/src/ntt.rs: ``forward(coeffs)`` = ``ntt_forward(coeffs, modulus, omega)``
    (natural order in and out), ``inverse(evals)`` = ``ntt_inverse``.  One handle per (modulus, n, omega).  n above 2^17 (up to 2^22,
    NTT_MODULUS only) goes through ``lsr_cyclic_ntt_context_create_large``."""

    _GALOIS_ORDER_PER_N = 1   # X has order n modulo X^n - 1

    def __init__(self, n, modulus=NTT_MODULUS, omega=0, device=-1):
        self._lib = _abi.lib()
        self.n, self.modulus = int(n), int(modulus)
        name = "lsr_cyclic_ntt_context_create_large" if self.n > MAX_TWO_PASS_SIZE else "lsr_cyclic_ntt_context_create"
        self._h = getattr(self._lib, name)(self.modulus, self.n, int(omega), device)
        if not self._h:
            raise CoreError(f"{name}({modulus}, {n}) returned NULL: {_abi.last_error()}")

    @property
    def handle(self):
        return self._h

    @property
    def omega(self):
        return self._lib.lsr_ntt_context_root(self._h)

    def _run(self, fn, values):
        arr = _u64_array(values).copy()
        if arr.size % self.n:
            raise ValueError("length must be a multiple of n")
        if fn(self._h, arr.ctypes.data, arr.size // self.n) != 0:
            raise CoreError("cyclic NTT failed: " + _abi.last_error())
        return arr

    def forward(self, coeffs):
        return self._run(self._lib.lsr_cyclic_ntt_forward_batch, coeffs)

    def inverse(self, evals):
        return self._run(self._lib.lsr_cyclic_ntt_inverse_batch, evals)

    def ring_mul(self, a, b):
        """Cyclic convolution a * b mod (X^n - 1, modulus); shapes as NttContext.ring_mul."""
        return _ring_mul(self._lib, self._h, self.n, a, b)

    def ring_mul_device(self, d_c, d_a, d_b, batch, b_rows, stream=0):
        _ring_mul_device(self._lib, self._h, d_c, d_a, d_b, batch, b_rows, stream)

    def ring_dot(self, a, b):
        """Sum of cyclic convolutions sum_i a_i * b_i mod (X^n - 1, modulus); shapes as NttContext.ring_dot."""
        return _ring_dot(self._lib, self._h, self.n, a, b)

    def ring_dot_device(self, d_c, d_a, d_b, batch, terms, b_rows, stream=0):
        _ring_dot_device(self._lib, self._h, d_c, d_a, d_b, batch, terms, b_rows, stream)

    def ring_matrix(self, m):
        """A RingMatrix of m [rows, cols, n] over Z_q[X]/(X^n - 1); as NttContext.ring_matrix."""
        return _ring_matrix(self, m)

    def ring_matrix_device(self, d_m, rows, cols, stream=0):
        return _ring_matrix_device(self, d_m, rows, cols, stream)

    def close(self):
        if self._h:
            self._lib.ntt_context_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class QuotientPlan:
    """Steps 3-6 of ``R1CS::compute_quotient_poly`` (rust-api/lambda-snark/src/r1cs.rs:474-506) on the NTT path
    (``should_use_ntt``: m a power of two, modulus NTT_MODULUS), for batches of independent instances."""

    def __init__(self, m, device=-1):
        self._lib = _abi.lib()
        self.m = int(m)
        name = "lsr_quotient_plan_create_large" if self.m > MAX_TWO_PASS_SIZE else "lsr_quotient_plan_create"
        self._h = getattr(self._lib, name)(self.m, device)
        if not self._h:
            raise CoreError(f"{name}({m}) returned NULL: {_abi.last_error()}")

    @property
    def handle(self):
        return self._h

    def quotient_batch(self, a_evals, b_evals, c_evals):
        """-> (coefficients [batch][m], lengths [batch]); length 0 marks the reference's Err (remainder non-zero)."""
        a, b, c = (_u64_array(v) for v in (a_evals, b_evals, c_evals))
        if not (a.size == b.size == c.size) or a.size % self.m:
            raise ValueError("a, b, c must hold the same number of m-word instances")
        batch = a.size // self.m
        quot = np.zeros((batch, self.m), dtype=np.uint64)
        lens = np.zeros(batch, dtype=np.uint32)
        if batch and self._lib.lsr_quotient_batch(self._h, a.ctypes.data, b.ctypes.data, c.ctypes.data, batch, quot.ctypes.data, lens.ctypes.data) != 0:
            raise CoreError("lsr_quotient_batch failed: " + _abi.last_error())
        return quot, lens

    def compute_quotient_poly(self, a_evals, b_evals, c_evals):
        """One instance, with the reference's return convention: the trimmed coefficient list, or CoreError."""
        quot, lens = self.quotient_batch(a_evals, b_evals, c_evals)
        if lens[0] == 0:
            raise CoreError("Polynomial division by Z_H: remainder non-zero (witness invalid)")   # r1cs.rs:1050-1054
        return quot[0, :lens[0]].copy()

    def quotient_device(self, da, db, dc, batch, dquot, dlen, stream=0):
        if self._lib.lsr_quotient_batch_device(self._h, da, db, dc, batch, dquot, dlen, stream) != 0:
            raise CoreError("lsr_quotient_batch_device failed: " + _abi.last_error())

    def close(self):
        if self._h:
            self._lib.lsr_quotient_plan_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SPARSE_ENTRY_DTYPE = np.dtype([("row", "<u4"), ("col", "<u4"), ("value", "<u8")])   # r1cs.h SparseEntry, 16 bytes


class R1csProver:
    """``R1CS`` restricted to what the prover's hot loop needs (rust-api/lambda-snark/src/r1cs.rs:88-137, 296-304, 474-506):
    the three matrices on the device, ``compute_constraint_evals`` and ``compute_quotient_poly`` for batches of witnesses.
    ``a``, ``b``, ``c`` are lists of ``(row, col, value)`` entries of m x n matrices.  ``modulus=None`` is NTT_MODULUS with m = 2^k
    (``lsr_r1cs_prover_create``); any other modulus, or NTT_MODULUS with m not a power of two, takes the Lagrange path
    (``lsr_r1cs_prover_create_mod``: odd q >= 3, 1 <= m <= 8192).  On the NTT path m goes up to 2^22; a matrix may
    then also be a numpy array of dtype ``SPARSE_ENTRY_DTYPE`` (the FFI's coordinate entries), which is handed over without a copy."""

    def __init__(self, m, n, a, b, c, device=-1, modulus=None):
        self._lib = _abi.lib()
        self.m, self.n = int(m), int(n)
        keep, mats = [], []
        for entries in (a, b, c):
            if isinstance(entries, np.ndarray) and entries.dtype == SPARSE_ENTRY_DTYPE:
                arr = np.ascontiguousarray(entries if len(entries) else np.zeros(1, dtype=SPARSE_ENTRY_DTYPE))
                keep.append(arr)
                mats.append(_abi.SparseMatrix(ctypes.cast(arr.ctypes.data, ctypes.POINTER(_abi.SparseEntry)), len(entries), self.m, self.n))
                continue
            arr = (_abi.SparseEntry * max(1, len(entries)))()
            for i, (row, col, value) in enumerate(entries):
                arr[i] = _abi.SparseEntry(int(row), int(col), int(value))
            keep.append(arr)
            mats.append(_abi.SparseMatrix(ctypes.cast(arr, ctypes.POINTER(_abi.SparseEntry)), len(entries), self.m, self.n))
        if modulus is None:
            self._h = self._lib.lsr_r1cs_prover_create(ctypes.byref(mats[0]), ctypes.byref(mats[1]), ctypes.byref(mats[2]), device)
            if not self._h:
                raise CoreError(f"lsr_r1cs_prover_create(m={m}, n={n}) returned NULL: {_abi.last_error()}")
        else:
            self._h = self._lib.lsr_r1cs_prover_create_mod(ctypes.byref(mats[0]), ctypes.byref(mats[1]), ctypes.byref(mats[2]), int(modulus), device)
            if not self._h:
                raise CoreError(f"lsr_r1cs_prover_create_mod(m={m}, n={n}, modulus={modulus}) returned NULL: {_abi.last_error()}")
        self.modulus = int(self._lib.lsr_r1cs_prover_modulus(self._h))
        self.uses_ntt = bool(self._lib.lsr_r1cs_prover_uses_ntt(self._h))

    def _witnesses(self, witnesses):
        w = _u64_array(witnesses)
        if w.size % self.n:
            raise ValueError("Witness length must equal n")      # r1cs.rs:297
        return w, w.size // self.n

    def compute_constraint_evals(self, witnesses):
        w, batch = self._witnesses(witnesses)
        out = [np.zeros((batch, self.m), dtype=np.uint64) for _ in range(3)]
        if batch and self._lib.lsr_r1cs_constraint_evals_batch(self._h, w.ctypes.data, batch, *(o.ctypes.data for o in out)) != 0:
            raise CoreError("lsr_r1cs_constraint_evals_batch failed: " + _abi.last_error())
        return tuple(out)

    def interpolate_batch(self, witnesses):
        """Lagrange-path provers: the interpolated A_z, B_z, C_z (lagrange_interpolate) -> three [batch][m] coefficient arrays."""
        w, batch = self._witnesses(witnesses)
        out = [np.zeros((batch, self.m), dtype=np.uint64) for _ in range(3)]
        if batch and self._lib.lsr_r1cs_interpolate_batch(self._h, w.ctypes.data, batch, *(o.ctypes.data for o in out)) != 0:
            raise CoreError("lsr_r1cs_interpolate_batch failed: " + _abi.last_error())
        return tuple(out)

    def quotient_batch(self, witnesses):
        w, batch = self._witnesses(witnesses)
        quot = np.zeros((batch, self.m), dtype=np.uint64)
        lens = np.zeros(batch, dtype=np.uint32)
        if batch and self._lib.lsr_r1cs_quotient_batch(self._h, w.ctypes.data, batch, quot.ctypes.data, lens.ctypes.data) != 0:
            raise CoreError("lsr_r1cs_quotient_batch failed: " + _abi.last_error())
        return quot, lens

    def prove_batch(self, ctx, witnesses, seeds, n_public, commit_modulus, blinding=None):
        """``prove_r1cs`` (blinding None) or ``prove_r1cs_zk`` (lib.rs:747-809, 877-980) for a batch of witnesses, NTT path.
        -> (rows [batch][ctx.commitment_words], proofs [batch][PROOF_WORDS], hashes [batch][2][32] uint8, status [batch]); status 0 marks
        a witness that does not satisfy the R1CS.  commit_modulus is Rust's ``LweContext::modulus()`` (``ctx.modulus()``)."""
        w, batch = self._witnesses(witnesses)
        seeds = _u64_array(seeds)
        if seeds.size != batch:
            raise ValueError("one seed per witness")
        blind = None if blinding is None else _u64_array(blinding)
        if blind is not None and blind.size != batch:
            raise ValueError("one blinding factor per witness")
        rows = np.zeros((batch, ctx.commitment_words), dtype=np.uint64)
        proofs = np.zeros((batch, PROOF_WORDS), dtype=np.uint64)
        hashes = np.zeros((batch, 2, 32), dtype=np.uint8)
        status = np.zeros(batch, dtype=np.uint32)
        if batch and self._lib.lsr_r1cs_prove_batch(self._h, ctx.handle, int(commit_modulus), w.ctypes.data, batch, int(n_public), seeds.ctypes.data,
                                                    None if blind is None else blind.ctypes.data, rows.ctypes.data, proofs.ctypes.data,
                                                    hashes.ctypes.data, status.ctypes.data) != 0:
            raise CoreError("lsr_r1cs_prove_batch failed: " + _abi.last_error())
        return rows, proofs, hashes, status

    def prove_batch_device(self, ctx, d_witnesses, batch, seeds, n_public, commit_modulus, d_rows, d_proofs, d_hashes, d_status, d_blinding=None,
                           stream=0):
        """``lsr_r1cs_prove_batch_device``: device pointers (ints, e.g. torch.Tensor.data_ptr()) in and out, host seeds (all non-zero),
        asynchronous on `stream`."""
        seeds = _u64_array(seeds)
        if seeds.size != batch:
            raise ValueError("one seed per witness")
        if self._lib.lsr_r1cs_prove_batch_device(self._h, ctx.handle, int(commit_modulus), d_witnesses, batch, int(n_public), seeds.ctypes.data,
                                                 d_blinding, d_rows, d_proofs, d_hashes, d_status, stream) != 0:
            raise CoreError("lsr_r1cs_prove_batch_device failed: " + _abi.last_error())

    def compute_quotient_poly(self, witness):
        quot, lens = self.quotient_batch(witness)
        if lens[0] == 0:
            raise CoreError("Witness does not satisfy R1CS constraints")          # r1cs.rs:477-480
        return quot[0, :lens[0]].copy()

    def close(self):
        if self._h:
            self._lib.lsr_r1cs_prover_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


PROOF_WORDS = 13
PROOF_FIELDS = ("alpha", "beta", "q_alpha", "q_beta", "a_z_alpha", "b_z_alpha", "c_z_alpha", "a_z_beta", "b_z_beta", "c_z_beta", "opening_alpha",
                "opening_beta", "blinding_factor")   # prover.h LSR_PROOF_*: ProofR1CS / ProofR1csZk field order


def verify_r1cs_batch(m, publics, rows, proofs, zk=False, modulus=None):
    """``verify_r1cs`` / ``verify_r1cs_zk`` (lib.rs:1016-1095, 1142-1215) for a batch, on the host (no GPU needed): -> int32 [batch] of 1 / 0.
    publics [batch][n_public], rows [batch][words], proofs [batch][PROOF_WORDS].  ``modulus=None``: NTT_MODULUS, m = 2^k
    (``lsr_r1cs_verify_batch``); else ``lsr_r1cs_verify_batch_mod``."""
    proofs = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, PROOF_WORDS)
    batch = proofs.shape[0]
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(batch, -1)
    publics = np.ascontiguousarray(publics, dtype=np.uint64).reshape(batch, -1)
    results = np.zeros(batch, dtype=np.int32)
    if modulus is not None:
        if batch and _abi.lib().lsr_r1cs_verify_batch_mod(int(m), int(modulus), publics.ctypes.data if publics.size else None, publics.shape[1],
                                                          rows.ctypes.data, rows.shape[1], proofs.ctypes.data, batch, 1 if zk else 0,
                                                          results.ctypes.data) != 0:
            raise CoreError("lsr_r1cs_verify_batch_mod failed: " + _abi.last_error())
        return results
    if batch and _abi.lib().lsr_r1cs_verify_batch(int(m), publics.ctypes.data if publics.size else None, publics.shape[1], rows.ctypes.data, rows.shape[1],
                                                  proofs.ctypes.data, batch, 1 if zk else 0, results.ctypes.data) != 0:
        raise CoreError("lsr_r1cs_verify_batch failed: " + _abi.last_error())
    return results


def verify_r1cs_batch_device(m, d_publics, n_public, d_rows, words_per_row, d_proofs, batch, d_results, zk=False, stream=0, modulus=None):
    """``lsr_r1cs_verify_batch_device``: device pointers, int32 results, asynchronous on `stream`.  ``modulus`` not None:
    ``lsr_r1cs_verify_batch_mod_device``."""
    if modulus is not None:
        if _abi.lib().lsr_r1cs_verify_batch_mod_device(int(m), int(modulus), d_publics, n_public, d_rows, words_per_row, d_proofs, batch, 1 if zk else 0,
                                                       d_results, stream) != 0:
            raise CoreError("lsr_r1cs_verify_batch_mod_device failed: " + _abi.last_error())
        return
    if _abi.lib().lsr_r1cs_verify_batch_device(int(m), d_publics, n_public, d_rows, words_per_row, d_proofs, batch, 1 if zk else 0, d_results, stream) != 0:
        raise CoreError("lsr_r1cs_verify_batch_device failed: " + _abi.last_error())


def prover_eval_batch_device(d_coeffs, length, batch, d_points, points_per_poly, d_values, stream=0):
    """``lsr_prover_eval_batch_device``: eval_poly (r1cs.rs:362-373) over NTT_MODULUS, values[i][k] = coeffs[i](points[i][k])."""
    if _abi.lib().lsr_prover_eval_batch_device(d_coeffs, length, batch, d_points, points_per_poly, d_values, stream) != 0:
        raise CoreError("lsr_prover_eval_batch_device failed: " + _abi.last_error())


# ---- the witness-polynomial proofs: prove_simple / prove_zk / simulate_proof / verify_simple (lib.rs:465-681, 1269-1285) ----------
SIMPLE_PROOF_WORDS = 3
SIMPLE_PROOF_FIELDS = ("alpha", "evaluation", "seed")   # prover.h LSR_SIMPLE_*: the challenge, Opening.evaluation, Opening.witness[0]
SIMPLE_MODES = {"plain": 0, "zk": 1, "simulate": 2}      # prove_simple, prove_zk, simulate_proof


def _simple_mode(mode):
    if mode not in SIMPLE_MODES:
        raise ValueError(f"mode must be one of {sorted(SIMPLE_MODES)}")
    return SIMPLE_MODES[mode]


def chacha20rng_keys(seeds):
    """``lsr_chacha20rng_keys_from_u64``: ``ChaCha20Rng::seed_from_u64`` keys, [count][4] uint64 (no GPU needed)."""
    seeds = _u64_array(seeds, "seeds").ravel()
    keys = np.zeros((seeds.size, 4), dtype=np.uint64)
    if seeds.size and _abi.lib().lsr_chacha20rng_keys_from_u64(seeds.ctypes.data, seeds.size, keys.ctypes.data) != 0:
        raise CoreError("lsr_chacha20rng_keys_from_u64 failed: " + _abi.last_error())
    return keys


def random_blinding(keys, length, modulus):
    """``lsr_random_blinding``: ``Polynomial::random_blinding(length - 1, modulus, .)`` per key (polynomial.rs:176-187) on the host,
    -> [batch][length] uint64."""
    keys = _u64_array(keys, "keys").reshape(-1, 4)
    out = np.zeros((keys.shape[0], int(length)), dtype=np.uint64)
    if _abi.lib().lsr_random_blinding(keys.ctypes.data, keys.shape[0], int(length), int(modulus), out.ctypes.data if out.size else None) != 0:
        raise CoreError("lsr_random_blinding failed: " + _abi.last_error())
    return out


def random_blinding_device(d_keys, batch, length, modulus, d_out, stream=0):
    """``lsr_random_blinding_device``: device pointers, asynchronous on `stream`."""
    if _abi.lib().lsr_random_blinding_device(d_keys, batch, int(length), int(modulus), d_out, stream) != 0:
        raise CoreError("lsr_random_blinding_device failed: " + _abi.last_error())


class SimpleProver:
    """``prove_simple`` / ``prove_zk`` / ``simulate_proof`` (lib.rs:465-491, 551-585, 657-681) for batches of one length over an odd
    field modulus q (``lsr_simple_prover_create``)."""

    def __init__(self, modulus, device=-1):
        self._lib = _abi.lib()
        self._h = self._lib.lsr_simple_prover_create(int(modulus), device)
        if not self._h:
            raise CoreError(f"lsr_simple_prover_create(modulus={modulus}) returned NULL: {_abi.last_error()}")
        self.modulus = int(self._lib.lsr_simple_prover_modulus(self._h))

    def prove_batch(self, ctx, witnesses, publics, seeds, commit_modulus, mode="plain", blinding_keys=None, length=None):
        """-> (rows [batch][ctx.commitment_words], coeffs [batch][length] (f' mod q = Opening.witness[1..]), proofs
        [batch][SIMPLE_PROOF_WORDS], hashes [batch][32] uint8).  witnesses [batch][length] (None for "simulate", which then needs
        ``length``); publics [batch][n_public]; seeds [batch] (0 = fresh entropy); blinding_keys [batch][4] (``chacha20rng_keys`` of the
        blinding / sim seeds; None = fresh entropy); commit_modulus is Rust's ``LweContext::modulus()`` (``ctx.modulus()``)."""
        m = _simple_mode(mode)
        seeds = _u64_array(seeds, "seeds").ravel()
        batch = seeds.size
        if witnesses is None:
            if m != SIMPLE_MODES["simulate"] or length is None:
                raise ValueError("witnesses are needed unless mode='simulate' with a length")
            w, length = None, int(length)
        else:
            w = _u64_array(witnesses, "witnesses").reshape(batch, -1)
            length = w.shape[1]
        pub = np.ascontiguousarray(publics, dtype=np.uint64).reshape(batch, -1)
        keys = None if blinding_keys is None else _u64_array(blinding_keys, "blinding_keys").reshape(batch, 4)
        rows = np.zeros((batch, ctx.commitment_words), dtype=np.uint64)
        coeffs = np.zeros((batch, length), dtype=np.uint64)
        proofs = np.zeros((batch, SIMPLE_PROOF_WORDS), dtype=np.uint64)
        hashes = np.zeros((batch, 32), dtype=np.uint8)
        if self._lib.lsr_simple_prove_batch(self._h, ctx.handle, int(commit_modulus), m, None if w is None else w.ctypes.data, length, batch,
                                            pub.ctypes.data if pub.size else None, pub.shape[1], seeds.ctypes.data,
                                            None if keys is None else keys.ctypes.data, rows.ctypes.data, coeffs.ctypes.data if coeffs.size else None,
                                            proofs.ctypes.data, hashes.ctypes.data) != 0:
            raise CoreError("lsr_simple_prove_batch failed: " + _abi.last_error())
        return rows, coeffs, proofs, hashes

    def prove_batch_device(self, ctx, d_witnesses, length, batch, d_publics, n_public, seeds, commit_modulus, d_rows, d_coeffs, d_proofs, d_hashes=None,
                           mode="plain", d_blinding_keys=None, stream=0):
        """``lsr_simple_prove_batch_device``: device pointers (ints) in and out, host seeds (all non-zero), asynchronous on `stream`."""
        seeds = _u64_array(seeds, "seeds").ravel()
        if seeds.size != batch:
            raise ValueError("one seed per proof")
        if self._lib.lsr_simple_prove_batch_device(self._h, ctx.handle, int(commit_modulus), _simple_mode(mode), d_witnesses, int(length), batch, d_publics,
                                                   int(n_public), seeds.ctypes.data, d_blinding_keys, d_rows, d_coeffs, d_proofs, d_hashes, stream) != 0:
            raise CoreError("lsr_simple_prove_batch_device failed: " + _abi.last_error())

    def close(self):
        if self._h:
            self._lib.lsr_simple_prover_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def verify_simple_batch(modulus, publics, rows, proofs, coeffs, ctx=None, commit_modulus=None):
    """``verify_simple`` (lib.rs:1269-1285) for a batch on the host -> int32 [batch] of 1 / 0; no GPU needed without ``ctx``.  With ``ctx``
    the binding check of ``verify_opening_with_context`` (opening.rs:160-222) is added (commit_modulus defaults to ``ctx.modulus()``)."""
    proofs = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, SIMPLE_PROOF_WORDS)
    batch = proofs.shape[0]
    rows = np.ascontiguousarray(rows, dtype=np.uint64).reshape(batch, -1)
    publics = np.ascontiguousarray(publics, dtype=np.uint64).reshape(batch, -1)
    coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(batch, -1)
    results = np.zeros(batch, dtype=np.int32)
    cm = 0 if ctx is None else int(ctx.modulus() if commit_modulus is None else commit_modulus)
    if batch and _abi.lib().lsr_simple_verify_batch(int(modulus), publics.ctypes.data if publics.size else None, publics.shape[1], rows.ctypes.data,
                                                    rows.shape[1], proofs.ctypes.data, coeffs.ctypes.data if coeffs.size else None, coeffs.shape[1],
                                                    batch, None if ctx is None else ctx.handle, cm, results.ctypes.data) != 0:
        raise CoreError("lsr_simple_verify_batch failed: " + _abi.last_error())
    return results


def verify_simple_batch_device(modulus, d_publics, n_public, d_rows, words_per_row, d_proofs, d_coeffs, length, batch, d_results, ctx=None,
                               commit_modulus=None, stream=0):
    """``lsr_simple_verify_batch_device``: device pointers, int32 results, asynchronous on `stream`."""
    cm = 0 if ctx is None else int(ctx.modulus() if commit_modulus is None else commit_modulus)
    if _abi.lib().lsr_simple_verify_batch_device(int(modulus), d_publics, int(n_public), d_rows, words_per_row, d_proofs, d_coeffs, int(length), batch,
                                                 None if ctx is None else ctx.handle, cm, d_results, stream) != 0:
        raise CoreError("lsr_simple_verify_batch_device failed: " + _abi.last_error())
