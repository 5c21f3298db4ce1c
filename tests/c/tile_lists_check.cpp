// tile_lists_check.cpp -- the tile lists (raytracercpp_amd/csrc/tile_lists.hpp) on the host, for
// tests/test_tile_lists.py: over random and structured masks, image sizes and band layouts, the lists of
// tile_lists_host against the frame kernel's predicate evaluated lane by lane (pixel by pixel), and the queue's
// shard ranges over 'covered'.  No GPU and no library: the header alone.  Prints one line per case group and
// "OK"; exit status 1 on the first violation.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../../raytracercpp_amd/csrc/tile_lists.hpp"

using namespace rt;

static uint32_t g_rng = 12345u;
static uint32_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 17;
    g_rng ^= g_rng << 5;
    return g_rng;
}

static int g_fail = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            printf("FAIL %s: ", #cond);        \
            printf(__VA_ARGS__);               \
            printf("\n");                      \
            g_fail++;                          \
            return;                            \
        }                                      \
    } while (0)

enum MaskKind { ALL_CLEAR, ALL_SET, ONE_BIT, DISC, RANDOM_HALF, RANDOM_SPARSE, NKINDS };

static std::vector<uint32_t> make_mask(int kind, int bw, int bh, int wpr)
{
    std::vector<uint32_t> w((size_t)bh * wpr, 0u);
    auto set = [&](int bx, int by) { w[(size_t)by * wpr + (bx >> 5)] |= 1u << (bx & 31); };
    const int ox = (int)(rnd() % (uint32_t)bw), oy = (int)(rnd() % (uint32_t)bh);
    for (int by = 0; by < bh; by++)
        for (int bx = 0; bx < bw; bx++) {
            bool on = false;
            switch (kind) {
            case ALL_CLEAR: break;
            case ALL_SET: on = true; break;
            case ONE_BIT: on = bx == ox && by == oy; break;
            case DISC: on = (bx - bw / 2) * (bx - bw / 2) + (by - bh / 2) * (by - bh / 2) <= (bh / 3) * (bh / 3); break;
            case RANDOM_HALF: on = rnd() & 1u; break;
            default: on = rnd() % 11u == 0; break;
            }
            if (on)
                set(bx, by);
        }
    return w;
}

static void check_shards(int n)
{
    int prev = 0;
    for (int s = 0; s < 8; s++) {
        int r0, r1;
        tile_shard_range(n, s, 8, r0, r1);
        CHECK(r0 == prev && r1 >= r0, "n %d shard %d: [%d, %d) after %d", n, s, r0, r1, prev);
        CHECK(r1 - r0 <= (n + 7) / 8, "n %d shard %d: %d entries", n, s, r1 - r0);
        prev = r1;
    }
    CHECK(prev == n, "n %d: the shards end at %d", n, prev);
}

static void check_case(const TileLayout& L, const char* what, long long& ncov, long long& nclr)
{
    std::vector<int32_t> covered, clear;
    tile_lists_host(L, covered, clear);
    const int ntiles = L.tiles_x * L.tiles_y;
    CHECK(std::is_sorted(covered.begin(), covered.end()) &&
              std::adjacent_find(covered.begin(), covered.end()) == covered.end(),
          "%s: covered is not strictly ascending", what);
    CHECK(std::is_sorted(clear.begin(), clear.end()) && std::adjacent_find(clear.begin(), clear.end()) == clear.end(),
          "%s: clear is not strictly ascending", what);
    std::vector<char> in_cov(ntiles, 0), in_clr(ntiles, 0);
    for (int32_t t : covered) {
        CHECK(t >= 0 && t < ntiles, "%s: covered tile %d", what, t);
        in_cov[t] = 1;
    }
    for (int32_t t : clear) {
        CHECK(t >= 0 && t < ntiles, "%s: clear tile %d", what, t);
        in_clr[t] = 1;
    }
    for (int t = 0; t < ntiles; t++) {
        // the frame kernel: the lanes on the image, and the ballot over their blocks' bits -- lane by lane
        bool on_image = false, any_bit = false;
        for (int lane = 0; lane < 64; lane++) {
            const int tx = t % L.tiles_x, ty = t / L.tiles_x;
            const int px = tx * 8 + (lane & 7), lr = ty * 8 + (lane >> 3);
            int py = L.rh;
            if (lr < L.local_rows) {
                if (L.nranks == 1)
                    py = lr;
                else {
                    const int band = lr / L.band_rows;
                    const int g = L.band_map ? L.band_map[band] : band * L.nranks + L.rank;
                    py = g * L.band_rows + (lr - band * L.band_rows);
                }
            }
            if (px >= L.rw || py >= L.rh)
                continue;
            on_image = true;
            any_bit |= (L.mask[(size_t)(py >> 3) * L.mask_wpr + (px >> 8)] >> ((px >> 3) & 31)) & 1u;
        }
        CHECK(!(in_cov[t] && in_clr[t]), "%s: tile %d is in both lists", what, t);
        CHECK((in_cov[t] || in_clr[t]) == on_image, "%s: tile %d on the image %d, listed %d", what, t, (int)on_image,
              in_cov[t] || in_clr[t]);
        CHECK(!on_image || (bool)in_cov[t] == any_bit, "%s: tile %d covered %d, a lane's bit set %d", what, t, in_cov[t],
              (int)any_bit);
    }
    check_shards((int)covered.size());
    // every entry of covered belongs to exactly one shard's range
    std::vector<int> owner(covered.size(), 0);
    for (int s = 0; s < 8; s++) {
        int r0, r1;
        tile_shard_range((int)covered.size(), s, 8, r0, r1);
        for (int i = r0; i < r1; i++)
            owner[i]++;
    }
    CHECK(std::all_of(owner.begin(), owner.end(), [](int c) { return c == 1; }), "%s: a covered entry outside one shard", what);
    ncov += (long long)covered.size();
    nclr += (long long)clear.size();
}

int main()
{
    const int sizes[3][2] = {{64, 32}, {96, 96}, {128, 72}};
    int ncases = 0;
    for (const auto& sz : sizes) {
        const int rw = sz[0], rh = sz[1];
        const int bw = (rw + 7) / 8, bh = (rh + 7) / 8, wpr = (bw + 31) / 32;
        for (int kind = 0; kind < NKINDS; kind++) {
            long long ncov = 0, nclr = 0;
            for (int rep = 0; rep < (kind >= ONE_BIT ? 3 : 1); rep++) {
                const std::vector<uint32_t> mask = make_mask(kind, bw, bh, wpr);
                // the whole frame (rt_ray_trace), then band rows 8 and 3 at 1 and 3 ranks, then a permuted band list
                std::vector<TileLayout> layouts;
                std::vector<std::vector<int32_t>> maps;
                layouts.push_back(TileLayout{rw, rh, rh, rh, 0, 1, (rw + 7) / 8, (rh + 7) / 8, nullptr, mask.data(), wpr});
                for (int br : {8, 3}) {
                    const int nb = (rh + br - 1) / br;
                    for (int nranks : {1, 3})
                        for (int rank = 0; rank < nranks; rank++) {
                            const int mine = (nb - rank + nranks - 1) / nranks;
                            const int lrows = mine * br;
                            layouts.push_back(TileLayout{rw, rh, lrows, br, rank, nranks, (rw + 7) / 8, (lrows + 7) / 8, nullptr,
                                                         mask.data(), wpr});
                        }
                    // a band list: a random subset of the bands in a random order (nranks 2: the list's layout)
                    std::vector<int32_t> perm(nb);
                    std::iota(perm.begin(), perm.end(), 0);
                    for (int i = nb - 1; i > 0; i--)
                        std::swap(perm[i], perm[rnd() % (uint32_t)(i + 1)]);
                    perm.resize(std::max(1, nb * 2 / 3));
                    maps.push_back(perm);
                }
                for (size_t m = 0; m < maps.size(); m++) {
                    const int br = m == 0 ? 8 : 3;
                    const int lrows = (int)maps[m].size() * br;
                    layouts.push_back(TileLayout{rw, rh, lrows, br, 0, 2, (rw + 7) / 8, (lrows + 7) / 8, maps[m].data(),
                                                 mask.data(), wpr});
                }
                for (const TileLayout& L : layouts) {
                    char what[160];
                    snprintf(what, sizeof what, "%dx%d mask %d rows %d rank %d/%d%s", rw, rh, kind, L.band_rows, L.rank,
                             L.nranks, L.band_map ? " list" : "");
                    check_case(L, what, ncov, nclr);
                    ncases++;
                    if (g_fail)
                        return 1;
                    if (kind == ALL_CLEAR && ncov != 0) {
                        printf("FAIL %s: covered tiles under an all-clear mask\n", what);
                        return 1;
                    }
                }
                if (kind == ALL_SET && nclr != 0) {
                    printf("FAIL %dx%d: clear tiles under an all-set mask\n", rw, rh);
                    return 1;
                }
            }
            printf("%dx%d mask kind %d: covered %lld, clear %lld tiles over the layouts\n", rw, rh, kind, ncov, nclr);
        }
    }
    for (int n = 0; n <= 70; n++) {   // the shard ranges alone: n < 8, n = 0, and beyond
        check_shards(n);
        if (g_fail)
            return 1;
    }
    check_shards(129600);
    check_shards(2147483640);
    if (g_fail)
        return 1;
    printf("OK %d cases\n", ncases);
    return 0;
}
