// The host quick-tree builder on its own (wbvh.cpp build_wbvh_quick over wbvh_quick.hpp), for a run under
// the host sanitizers and for comparing two source trees' output: builds the octree and the quick tree of
// a pile of 500 copies of one triangle (runs trees three deep), a 5,000-triangle random soup and a UV
// sphere with pole slivers, checks each with check_wbvh, and prints one FNV-1a digest per input over the
// nodes, slot maps and links.  Link it with librt_mi355x.so (tests/test_wbvh_quick_digest.py) or compile it
// with octree.cpp and wbvh.cpp; prints "ok" when every tree has 0 violations.
#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../../raytracercpp_amd/csrc/wbvh.hpp"

using namespace rt;

static uint64_t digest(const WBvh& w)
{
    uint64_t h = 1469598103934665603ull;
    auto mix = [&h](const void* p, size_t len) {
        const unsigned char* b = static_cast<const unsigned char*>(p);
        for (size_t i = 0; i < len; i++) {
            h ^= b[i];
            h *= 1099511628211ull;
        }
    };
    mix(w.nodes.data(), w.nodes.size() * sizeof(WNode));
    mix(w.slot.data(), w.slot.size() * 4);
    mix(w.leaf_of_slot.data(), w.leaf_of_slot.size() * 4);
    mix(w.tri_leaf.data(), w.tri_leaf.size() * 4);
    mix(w.parent.data(), w.parent.size() * 4);
    return h;
}

static int run(const char* name, const std::vector<float>& tri, int depth, int leaf)
{
    FlatOctree f;
    build_flat_octree(tri.data(), (int64_t)tri.size() / 9, depth, leaf, f);
    WBvh w;
    build_wbvh_quick(f, w, true);
    const int64_t v = check_wbvh(f, w);
    std::printf("%s depth %d leaf %d: nodes %lld leaves %lld wide depth %lld digest %016llx violations %lld\n", name, depth,
                leaf, (long long)w.stats.nodes, (long long)w.stats.leaves, (long long)w.stats.depth,
                (unsigned long long)digest(w), (long long)v);
    return v == 0 ? 0 : 1;
}

int main()
{
    int bad = 0;
    std::vector<float> pile;
    for (int k = 0; k < 500; k++) {
        const float v[9] = {0.1f, 0.2f, -3.0f, 1.1f, 0.3f, -3.2f, 0.4f, 1.5f, -2.9f};
        pile.insert(pile.end(), v, v + 9);
    }
    bad += run("pile500", pile, 12, 40);
    bad += run("pile500", pile, 3, 1);
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> U(-1.0f, 1.0f);
    std::vector<float> soup;
    for (int k = 0; k < 5000; k++) {
        const float c[3] = {3 * U(rng), 3 * U(rng), -6 + 2 * U(rng)};
        float v[9];
        for (int j = 0; j < 9; j++) v[j] = c[j % 3] + 0.3f * U(rng);
        if (k % 50 == 0)   // zero-area and zero-normal records among them
            for (int j = 3; j < 9; j++) v[j] = k % 100 == 0 ? v[j % 3] : v[j % 3] + (j < 6 ? 0.1f : 0.2f);
        soup.insert(soup.end(), v, v + 9);
    }
    bad += run("soup5000", soup, 12, 40);
    bad += run("soup5000", soup, 12, 4);
    bad += run("soup5000", soup, 0, 40);
    std::vector<float> sph;
    const int nu = 96, nv = 48;
    auto P = [&](int i, int j, float* o) {
        const double th = M_PI * j / nv, ph = 2 * M_PI * (i % nu) / nu;
        o[0] = (float)(1.2 * std::sin(th) * std::cos(ph));
        o[1] = (float)(1.2 * std::cos(th));
        o[2] = (float)(1.2 * std::sin(th) * std::sin(ph) - 3.0);
    };
    for (int i = 0; i < nu; i++)
        for (int j = 0; j < nv; j++) {
            float a[3], b[3], c[3], d[3];
            P(i, j, a), P(i + 1, j, b), P(i + 1, j + 1, c), P(i, j + 1, d);
            for (float* v : {a, b, c, a, c, d})
                sph.insert(sph.end(), v, v + 3);
        }
    bad += run("sphere", sph, 12, 40);
    bad += run("sphere", sph, 6, 2);
    std::printf(bad ? "FAIL\n" : "ok\n");
    return bad ? 1 : 0;
}
