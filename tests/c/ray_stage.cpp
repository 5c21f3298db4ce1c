// ray_stage.cpp -- rt::stage_layout (raytracercpp_amd/csrc/ray_stage.hpp, included alone and compiled as plain
// C++) over the array lists of the three host ray queries (renderer.cpp trace_rays, wide_query,
// trace_ray_colors) at n = 0, 1, 3, 255, 2^28 and 2^30: every offset a multiple of 16, the slots disjoint and in
// the list's order, the total the last slot's end rounded up, and every figure equal to the same sum taken in
// 128 bits (nothing wraps in 64: the shaded list takes 50 B per ray, 53.7 GB at 2^30).
// Prints "ok <layouts> <checks>".
#include <cstdio>
#include <cstdlib>

#include "../../raytracercpp_amd/csrc/ray_stage.hpp"

using rt::StageArray;
typedef unsigned __int128 u128;

static long checks = 0;
#define CHECK(c)                                                                      \
    do {                                                                              \
        checks++;                                                                     \
        if (!(c)) {                                                                   \
            std::printf("FAILED %s (list %d, n %llu, array %d)\n", #c, li, (unsigned long long)n, k); \
            std::exit(1);                                                             \
        }                                                                             \
    } while (0)

int main()
{
    static char host[16];   // (the layout reads no host pointer)
    const unsigned once = rt::STAGE_UP | rt::STAGE_DOWN | rt::STAGE_ONCE;
    // bytes per ray, in the order the renderer lists them: origins, directions, then the outputs
    const StageArray trace_rays[] = {rt::stage_in(host, 12), rt::stage_in(host, 12), rt::stage_out(host, 4),
                                     rt::stage_out(host, 4), rt::stage_out(host, 4), rt::stage_out(host, 4),
                                     rt::stage_out(host, 1)};
    const StageArray wide_query[] = {rt::stage_in(host, 12),  rt::stage_in(host, 12),  rt::stage_out(host, 12),
                                     rt::stage_out(host, 12), rt::stage_out(host, 4),  rt::stage_out(host, 4),
                                     rt::stage_out(host, 4),  rt::stage_out(host, 4),  rt::stage_out(host, 4),
                                     rt::stage_out(host, 1)};
    const StageArray trace_ray[] = {rt::stage_in(host, 12), rt::stage_in(host, 12), rt::stage_out(host, 16),
                                    rt::stage_out(host, 4), rt::stage_out(host, 4), rt::stage_out(host, 1),
                                    rt::stage_out(host, 1), {host, 16, once}};
    struct {
        const StageArray* a;
        int count;
    } const lists[] = {{trace_rays, 7}, {wide_query, 10}, {trace_ray, 8}};
    const uint64_t ns[] = {0, 1, 3, 255, 1ull << 28, 1ull << 30};
    int layouts = 0;
    for (int li = 0; li < 3; li++)
        for (uint64_t n : ns) {
            const StageArray* a = lists[li].a;
            const int count = lists[li].count;
            const rt::StageLayout L = rt::stage_layout(a, count, n);
            u128 end = 0;   // the previous slot's end, in 128 bits
            int k;
            for (k = 0; k < count; k++) {
                const u128 bytes = (u128)a[k].elem * ((a[k].flags & rt::STAGE_ONCE) ? 1 : n);
                const u128 off = (end + 15) / 16 * 16;
                CHECK(L.off[k] % 16 == 0);
                CHECK((u128)L.off[k] >= end);     // disjoint from the slots before it, and after them
                CHECK((u128)L.off[k] == off);     // ... with no gap but the rounding, and no wrap
                CHECK((u128)L.bytes[k] == bytes);
                end = off + bytes;
            }
            k = count - 1;
            CHECK((u128)L.total == (end + 15) / 16 * 16);
            CHECK(L.total == (L.off[k] + L.bytes[k] + 15) / 16 * 16);
            CHECK(L.total % 16 == 0 && (L.total >> 40) == 0);
            layouts++;
        }
    // every per-ray size times 2^30 is a multiple of 16: no rounding there, 50 B per ray and the counts
    {
        const int li = 2, k = 7;
        const uint64_t n = 1ull << 30;
        CHECK(rt::stage_layout(trace_ray, 8, n).total == 50 * n + 16);
        CHECK(rt::stage_layout(trace_ray, 8, 0).total == 16);   // the counts alone
        CHECK(rt::stage_layout(trace_rays, 7, 3).total == 48 + 48 + 4 * 16 + 16);
    }
    std::printf("ok %d %ld\n", layouts, checks);
    return 0;
}
