// Stand-alone host check of the staging loop's arithmetic (lsr_staging_plan.hpp), meant to be built with
// -fsanitize=address,undefined and run on a CPU:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -Ilambda-snark-r_amd/csrc tools/staging_plan_check.cpp -o staging_plan_check \
//       && ./staging_plan_check
// It walks the chunks exactly as host_staged (lsr_ring_call.hpp) does, over every count and chunk in 1 .. 40, components in 1 .. 45,
// stride in {0, 1, 3} and extent in max(stride, 1) .. stride + 4, and asserts that (a) the chunks tile [0, count); (b) every copy
// of an item lane lies inside the host buffer of (count - 1) stride + extent bytes and inside the device buffer; (c) every item of a
// chunk finds its group inside the range the chunk uploaded, and that range inside the device buffer and the host's
// ceil(count / components) groups; (d) a stride == 0 lane goes up exactly once.
#include <cstddef>
#include <cstdio>

#include "lsr_staging_plan.hpp"

#define CHECK(cond)                                                                                                                    \
    do {                                                                                                                               \
        if (!(cond)) {                                                                                                                 \
            std::fprintf(stderr, "FAILED %s at count = %zu, chunk = %zu, j0 = %zu, components = %zu, stride = %zu, extent = %zu\n", #cond, \
                         count, chunk, j0, components, stride, extent);                                                                \
            return 1;                                                                                                                  \
        }                                                                                                                              \
    } while (0)

int main() {
    static const char host[1] = {};
    size_t plans = 0, copies = 0;
    for (size_t count = 1; count <= 40; ++count)
        for (size_t chunk = 1; chunk <= 40; ++chunk) {
            size_t components = 0, stride = 0, extent = 0, j0 = 0;
            // (a) the loop of host_staged
            size_t covered = 0;
            for (j0 = 0; j0 < count; j0 += chunk) {
                const size_t now = std::min(chunk, count - j0);
                CHECK(j0 == covered && now >= 1 && now <= chunk);
                covered += now;
            }
            CHECK(covered == count);
            // (b), (d) item lanes
            for (size_t si = 0; si < 3; ++si) {
                stride = si == 0 ? 0 : (si == 1 ? 1 : 3);
                for (extent = std::max<size_t>(stride, 1); extent <= stride + 4; ++extent) {
                    const lsr::StagedLane lane = lsr::staged_items(host, nullptr, stride, extent);
                    const size_t host_bytes = (count - 1) * stride + extent, device_bytes = lsr::staged_allocation(lane, count, chunk);
                    size_t uploads = 0;
                    for (j0 = 0; j0 < count; j0 += chunk) {
                        const size_t now = std::min(chunk, count - j0);
                        const lsr::StagedCopy copy = lsr::staged_copy(lane, j0, now);
                        CHECK(copy.bytes >= 1 && copy.bytes <= device_bytes);
                        CHECK(copy.host_offset + copy.bytes <= host_bytes);
                        // item j of the chunk sits at (j - j0) stride of the device buffer
                        CHECK((now - 1) * stride + extent <= copy.bytes);
                        uploads += lsr::staged_uploads(lane, j0);
                        ++copies;
                    }
                    if (stride == 0) CHECK(uploads == 1);
                    else CHECK(uploads == (count + chunk - 1) / chunk);
                    ++plans;
                }
            }
            // (c) group lanes
            stride = extent = 5;
            for (components = 1; components <= 45; ++components) {
                const lsr::StagedLane lane = lsr::staged_groups(host, extent, components);
                const size_t host_groups = (count + components - 1) / components, device_bytes = lsr::staged_allocation(lane, count, chunk);
                CHECK(device_bytes <= (chunk / components + 2) * extent);
                for (j0 = 0; j0 < count; j0 += chunk) {
                    const size_t now = std::min(chunk, count - j0), group_first = lsr::staged_group_first(j0, components);
                    const lsr::StagedCopy copy = lsr::staged_copy(lane, j0, now);
                    CHECK(lsr::staged_uploads(lane, j0));
                    CHECK(copy.host_offset == group_first * extent && copy.bytes % extent == 0 && copy.bytes >= extent);
                    CHECK(copy.bytes <= device_bytes);
                    CHECK(copy.host_offset + copy.bytes <= host_groups * extent);
                    for (size_t j = j0; j < j0 + now; ++j) CHECK(j / components >= group_first && (j / components - group_first + 1) * extent <= copy.bytes);
                    ++copies;
                }
                ++plans;
            }
        }
    std::printf("staging plan: %zu lane plans, %zu chunk copies: ok\n", plans, copies);
    return 0;
}
