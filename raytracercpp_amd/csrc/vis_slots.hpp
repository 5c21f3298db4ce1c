// vis_slots.hpp -- which per-stream slot a visibility launch takes (renderer.cpp visibility_device): the slot of
// the launching stream, else a slot not yet in use, else the least recently used one, which the caller recycles
// once that slot's last launch is done.  Plain C++ (no HIP): tests/c/vis_slots.cpp includes it alone.
#pragma once

#include <stdint.h>

namespace rt {

constexpr int VIS_SLOTS = 8;   // streams with visibility launches in flight at a time (as BAND_SLOTS)

struct VisPick {
    int slot;        // the slot the launch takes
    bool fresh;      // never used before: its fence is to be created (count grows by one)
    bool recycled;   // another stream's: wait for its last launch, then it is this stream's
};

// streams[i] / used[i] for i < count <= cap: the slots' streams (as integers) and the value of the use counter at
// their last launch (distinct, growing with every launch).
inline VisPick vis_pick_slot(const uintptr_t* streams, const uint64_t* used, int count, int cap, uintptr_t stream)
{
    for (int i = 0; i < count; i++)
        if (streams[i] == stream)
            return {i, false, false};
    if (count < cap)
        return {count, true, false};
    int lru = 0;
    for (int i = 1; i < cap; i++)
        if (used[i] < used[lru])
            lru = i;
    return {lru, false, true};
}

}  // namespace rt
