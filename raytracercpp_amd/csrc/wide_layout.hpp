// wide_layout.hpp -- where the arrays lie inside the device-resident wide BVH's packed buffers (renderer.hpp
// WideDev, the risk buffer), as functions of the tree's node count nn and triangle-record count nt.  Every
// reader and writer of these buffers takes its offsets from here.  No HIP call: host programs include it.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace rt {

// WideDev::b_tmp, what wide_gather_kernel reads: slot[nt] (int32), then leaf_of_slot[nt] (uint32)
constexpr size_t wide_tmp_slot_off(size_t, size_t) { return 0; }
constexpr size_t wide_tmp_leaf_of_slot_off(size_t, size_t nt) { return nt * 4; }
constexpr size_t wide_tmp_bytes(size_t, size_t nt) { return nt * 8; }

// WideDev::b_links, the grazing-risk walk's (WBvh::tri_leaf, parent): tri_leaf[nt], then parent[nn] (uint32)
constexpr size_t wide_links_tri_leaf_off(size_t, size_t) { return 0; }
constexpr size_t wide_links_parent_off(size_t, size_t nt) { return nt * 4; }
constexpr size_t wide_links_bytes(size_t nn, size_t nt) { return (nt + nn) * 4; }

// The risk buffer (KParams::wrisk): per node 8 packed words (8 B), then the walk's 8 keys (4 B) and 8 boxes
// (6 floats) for all nodes, then the two risk caps (KParams::risk_cap) in a tail of their own.
constexpr size_t WRISK_ENTRIES = 8;   // per node: one per child (W_WIDTH)
constexpr size_t wide_risk_words_off(size_t) { return 0; }
constexpr size_t wide_risk_keys_off(size_t nn) { return nn * WRISK_ENTRIES * 8; }
constexpr size_t wide_risk_boxes_off(size_t nn) { return wide_risk_keys_off(nn) + nn * WRISK_ENTRIES * 4; }
constexpr size_t wide_risk_caps_off(size_t nn) { return wide_risk_boxes_off(nn) + nn * WRISK_ENTRIES * 24; }
constexpr size_t wide_risk_bytes(size_t nn) { return wide_risk_caps_off(nn) + 64; }

// the risk buffer's arrays for a tree of nn nodes (entries: of words, keys and boxes each)
struct WRiskView {
    unsigned long long* words;
    uint32_t* keys;
    float* boxes;
    uint32_t* caps;
    size_t entries;
};

inline WRiskView wide_risk_view(void* base, size_t nn)
{
    char* b = static_cast<char*>(base);
    return {reinterpret_cast<unsigned long long*>(b + wide_risk_words_off(nn)),
            reinterpret_cast<uint32_t*>(b + wide_risk_keys_off(nn)), reinterpret_cast<float*>(b + wide_risk_boxes_off(nn)),
            reinterpret_cast<uint32_t*>(b + wide_risk_caps_off(nn)), nn * WRISK_ENTRIES};
}

}  // namespace rt
