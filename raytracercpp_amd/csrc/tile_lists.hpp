// tile_lists.hpp -- the tile lists of a frame launch: which of the launch's 8 x 8 tiles the
// tile mask (wbvh.hpp wbvh_mask_rect) leaves to trace ('covered') and which it answers
// ('clear'), in ascending tile index.  The predicate is the plain frame kernel's own (kernels.hip
// ray_trace_kernel: the lanes on the image, and the __ballot over their blocks' mask bits), written once for
// the host and the device, as wbvh.hpp's; kernels.hip tile_class_kernel / tile_list_kernel build the lists,
// tile_lists_host the same on the host.
#pragma once

#include <stdint.h>

#include <vector>

#include "rt_math.hpp"

namespace rt {

// A launch's rows and tiles (KParams' fields of the same names) and the camera's mask words.
struct TileLayout {
    int32_t rw, rh;            // the internal image
    int32_t local_rows;        // rows of the launch's local buffers
    int32_t band_rows;         // internal rows per band
    int32_t rank, nranks;      // interleaved bands (band_map == nullptr)
    int32_t tiles_x, tiles_y;  // 8 x 8 tiles over (rw, local_rows)
    const int32_t* band_map;   // a band list: local band -> global band (nullptr: interleaved)
    const uint32_t* mask;      // block (px >> 3, py >> 3) at bit (px >> 3) & 31 of word (py >> 3) mask_wpr + (px >> 8)
    int32_t mask_wpr;
};

enum TileClass { TILE_OFF = 0, TILE_CLEAR = 1, TILE_COVERED = 2 };

// the global internal row of a launch-local row (kernels.hip global_row)
RT_HD int tl_global_row(const TileLayout& L, int lr)
{
    if (L.nranks == 1)
        return lr;
    const int band = lr / L.band_rows;
    const int g = L.band_map ? L.band_map[band] : band * L.nranks + L.rank;
    return g * L.band_rows + (lr - band * L.band_rows);
}

// One lane of a tile, as the frame kernel sees it (lane = 8 * row + column): TILE_OFF when its pixel is not on
// the image, else its block's mask bit (TILE_COVERED: set).
RT_HD int tile_lane_class(const TileLayout& L, int tile, int lane)
{
    const int tx = tile % L.tiles_x, ty = tile / L.tiles_x;
    const int px = tx * 8 + (lane & 7);
    const int lr = ty * 8 + (lane >> 3);
    const int py = lr < L.local_rows ? tl_global_row(L, lr) : L.rh;
    if (px >= L.rw || py >= L.rh)
        return TILE_OFF;
    const uint32_t mw = L.mask[(size_t)(py >> 3) * (size_t)L.mask_wpr + (size_t)(px >> 8)];
    return (mw >> ((px >> 3) & 31)) & 1u ? TILE_COVERED : TILE_CLEAR;
}

// The tile: TILE_OFF when no lane is on the image, TILE_COVERED when an on-image lane's bit is set, else
// TILE_CLEAR.  A tile's eight columns share px >> 3 and column 0 is on the image when any is, so the rows'
// first lanes decide (a tile's rows may lie in several bands, and so in several block rows of the mask).
RT_HD int tile_class(const TileLayout& L, int tile)
{
    int c = TILE_OFF;
    for (int row = 0; row < 8; row++) {
        const int k = tile_lane_class(L, tile, 8 * row);
        c = k > c ? k : c;
    }
    return c;
}

// The queue's shard s of TILE_SHARDS owns covered[r0, r1): n s / 8 .. n (s + 1) / 8, a contiguous run in
// row-major order (a band of the image with an eighth of the covered tiles).
RT_HD void tile_shard_range(int n, int s, int shards, int& r0, int& r1)
{
    r0 = (int)((long long)n * s / shards);
    r1 = (int)((long long)n * (s + 1) / shards);
}

// The lists' buffer, in 4-byte words: [0] covered tiles, [1] clear tiles, [2..3] unused; covered[ntiles] at
// TL_HEAD, clear[ntiles] behind it; then per 64 tiles two 64-bit words of tile_class_kernel (bit i: tile 64 k + i
// is covered / is clear), the scan's input.
constexpr int TL_HEAD = 4;
RT_HD size_t tile_lists_class_word(int ntiles) { return (size_t)TL_HEAD + 2 * (size_t)ntiles; }
RT_HD size_t tile_lists_words(int ntiles) { return tile_lists_class_word(ntiles) + 4 * (((size_t)ntiles + 63) / 64); }

// The lists on the host (L.mask: host memory).
inline void tile_lists_host(const TileLayout& L, std::vector<int32_t>& covered, std::vector<int32_t>& clear)
{
    covered.clear();
    clear.clear();
    const int ntiles = L.tiles_x * L.tiles_y;
    for (int t = 0; t < ntiles; t++) {
        const int c = tile_class(L, t);
        if (c == TILE_COVERED)
            covered.push_back(t);
        else if (c == TILE_CLEAR)
            clear.push_back(t);
    }
}

}  // namespace rt
