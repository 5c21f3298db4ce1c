// vis_slots.cpp -- rt::vis_pick_slot (raytracercpp_amd/csrc/vis_slots.hpp, included alone and compiled as plain
// C++) driven the way Renderer::visibility_device drives it, over 4,000 launches on 1 to 20 streams in random order:
// the slot is in range and within the caller's arrays, a stream that has a slot gets that slot, a new stream takes an
// unused slot while there is one, and after that the slot whose last launch is the oldest (a model kept beside it:
// the streams by their last launch); no two slots ever hold one stream.
// Prints "ok <launches> <checks>".
#include <cstdio>
#include <cstdlib>

#include "../../raytracercpp_amd/csrc/vis_slots.hpp"

static long checks = 0;
#define CHECK(c)                                                       \
    do {                                                               \
        checks++;                                                      \
        if (!(c)) {                                                    \
            std::printf("FAILED %s (launch %d, stream %d)\n", #c, launch, s); \
            std::exit(1);                                              \
        }                                                              \
    } while (0)

int main()
{
    constexpr int CAP = rt::VIS_SLOTS, NSTREAMS = 20;
    int launches = 0;
    uint32_t rng = 12345u;
    for (int round = 0; round < 4; round++) {
        // (exactly 'count' entries are valid, as in the renderer: the arrays are sized to it, so that a read past
        // count is a heap overflow the sanitizer reports)
        int count = 0;
        uintptr_t* streams = new uintptr_t[1];
        uint64_t* used = new uint64_t[1];
        uint64_t uses = 0;
        uint64_t last[NSTREAMS] = {};   // the model: each stream's last launch (0: none, or its slot was taken)
        const int nstreams = round == 0 ? 1 : round == 1 ? CAP : round == 2 ? CAP + 1 : NSTREAMS;
        for (int launch = 0; launch < 1000; launch++, launches++) {
            rng = rng * 1664525u + 1013904223u;
            const int s = (int)((rng >> 8) % (uint32_t)nstreams);
            // (stream 0 is the null stream: the handle 0 is a stream like any other)
            const uintptr_t h = s == 0 ? 0 : (uintptr_t)0x1000 * (uintptr_t)s;
            const rt::VisPick p = rt::vis_pick_slot(streams, used, count, CAP, h);
            CHECK(p.slot >= 0 && p.slot < CAP && p.slot <= count);
            CHECK(!(p.fresh && p.recycled));
            int holder = -1;
            for (int i = 0; i < count; i++)
                if (streams[i] == h) holder = i;
            if (holder >= 0) {
                CHECK(p.slot == holder && !p.fresh && !p.recycled && last[s] == used[holder]);
            } else if (count < CAP) {
                CHECK(p.fresh && p.slot == count && last[s] == 0);
                uintptr_t* ns = new uintptr_t[count + 1];
                uint64_t* nu = new uint64_t[count + 1];
                for (int i = 0; i < count; i++) {
                    ns[i] = streams[i];
                    nu[i] = used[i];
                }
                delete[] streams;
                delete[] used;
                streams = ns;
                used = nu;
                count++;
            } else {
                CHECK(p.recycled && p.slot < count && last[s] == 0);
                for (int i = 0; i < count; i++)
                    CHECK(used[p.slot] <= used[i]);
                for (int k = 0; k < NSTREAMS; k++)   // the stream that held the slot has none now
                    if (last[k] == used[p.slot]) last[k] = 0;
            }
            streams[p.slot] = h;
            used[p.slot] = ++uses;
            last[s] = uses;
            for (int i = 0; i < count; i++)
                for (int j = i + 1; j < count; j++)
                    CHECK(streams[i] != streams[j] && used[i] != used[j]);
        }
        delete[] streams;
        delete[] used;
    }
    std::printf("ok %d %ld\n", launches, checks);
    return 0;
}
