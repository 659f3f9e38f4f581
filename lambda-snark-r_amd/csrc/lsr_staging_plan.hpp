// The arithmetic of the host staging loop (host_staged, lsr_ring_call.hpp): which bytes of a host buffer a chunk of
// items moves, which groups it needs, and how large the device buffers are.  Includes no HIP header, so that
// tools/staging_plan_check.cpp sweeps it on a CPU.
#pragma once
#include <algorithm>
#include <cstddef>

namespace lsr {

// One buffer of a staged call: `up` (or NULL) goes to the device before the chunk's work, `down` (or NULL) comes back after it; both:
// an in-place buffer.  extent == 0: an absent lane, with no device buffer and no copies.
//   An item lane (components == 0) holds `extent` bytes per item, `stride` bytes apart: stride == extent is a plain per-item buffer,
// stride < extent a span of overlapping windows (the vectors a fold reads at term_stride < terms), stride == 0 one operand that every
// item shares, which goes up once.
//   A group lane (components != 0) holds `extent` bytes per group of `components` consecutive items (keys, weights); a chunk brings
// the groups its items belong to.
struct StagedLane {
    const void* up;
    void* down;
    size_t stride, extent, components;
};

inline StagedLane staged_items(const void* up, void* down, size_t stride, size_t extent) { return {up, down, stride, extent, 0}; }
inline StagedLane staged_items(const void* up, void* down, size_t bytes) { return {up, down, bytes, bytes, 0}; }
inline StagedLane staged_groups(const void* up, size_t group_bytes, size_t components) { return {up, nullptr, group_bytes, group_bytes, components}; }

// the bytes `items` >= 1 consecutive items of an item lane span
inline size_t staged_span(const StagedLane& l, size_t items) { return (items - 1) * l.stride + l.extent; }

// the group of the first item of a chunk: the device buffer of a group lane starts there
inline size_t staged_group_first(size_t j0, size_t components) { return j0 / components; }

// bytes of the lane's device buffer in a call of `count` items taken `chunk` at a time.  A chunk touches at most chunk / components
// + 2 groups: whole ones and a partial one at either end.
inline size_t staged_allocation(const StagedLane& l, size_t count, size_t chunk) {
    if (l.extent == 0) return 0;
    if (l.components == 0) return staged_span(l, chunk);
    return std::min((count - 1) / l.components + 1, chunk / l.components + 2) * l.extent;
}

// the copy of items [j0, j0 + now): `bytes` at `host_offset` of the host buffer, to or from the start of the device buffer
struct StagedCopy {
    size_t host_offset, bytes;
};
inline StagedCopy staged_copy(const StagedLane& l, size_t j0, size_t now) {
    if (l.components == 0) return {j0 * l.stride, staged_span(l, now)};
    const size_t g0 = staged_group_first(j0, l.components), g1 = (j0 + now - 1) / l.components;
    return {g0 * l.extent, (g1 - g0 + 1) * l.extent};
}

// whether the chunk at j0 uploads the lane: a shared operand goes up with the first chunk alone
inline bool staged_uploads(const StagedLane& l, size_t j0) { return l.up && l.extent != 0 && (l.components != 0 || l.stride != 0 || j0 == 0); }

}  // namespace lsr
