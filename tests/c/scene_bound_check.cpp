// The scene bound (wbvh.hpp wbvh_scene_bound / scene_bound_rejects) against the query it
// shortcuts, on the host (tests/scene_bound_tool.py; librt_mi355x.so's own octree and wide-BVH build): rays
// from cam; the bound as renderer.cpp prepare_risk computes it from the wide BVH's root (scale_override > 0:
// shrunk about its centre by that factor).  Every ray runs the unmodified host query with the camera's risk
// words; a ray the bound rejects runs it without them as well, and is a violation unless both end as W_MISS
// after at most one node visit.
//   scene_bound_check <in> <out>
//   in:  int64 n, nrays; int32 max_depth, leaf_max_obj_count; float scale_override, cam[3]; float tri9[n][9];
//        float dir[nrays][3]
//   out: int64 {violations, rays rejected, rays the full query answers as misses, bound valid}; float bound[6]
//        (lo x y z, hi x y z); int32 rejected[nrays]
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "../../raytracercpp_amd/csrc/wbvh.hpp"

using namespace rt;

static int fail(const char* what)
{
    fprintf(stderr, "scene_bound_check: %s\n", what);
    return 1;
}

int main(int argc, char** argv)
{
    if (argc != 3)
        return fail("usage: scene_bound_check <in> <out>");
    FILE* fi = fopen(argv[1], "rb");
    if (!fi)
        return fail("cannot open the input");
    int64_t n = 0, nrays = 0;
    int32_t max_depth = 0, leaf_max_obj_count = 0;
    float scale_override = 0.0f, cam[3] = {0, 0, 0};
    bool ok = fread(&n, 8, 1, fi) == 1 && fread(&nrays, 8, 1, fi) == 1 && fread(&max_depth, 4, 1, fi) == 1 &&
              fread(&leaf_max_obj_count, 4, 1, fi) == 1 && fread(&scale_override, 4, 1, fi) == 1 && fread(cam, 4, 3, fi) == 3 &&
              n > 0 && nrays >= 0;
    std::vector<float> tri, dirs;
    if (ok) {
        tri.resize((size_t)n * 9);
        dirs.resize((size_t)nrays * 3);
        ok = fread(tri.data(), 4, tri.size(), fi) == tri.size() && fread(dirs.data(), 4, dirs.size(), fi) == dirs.size();
    }
    fclose(fi);
    if (!ok)
        return fail("bad input");
    const float* tri9 = tri.data();
    const float* dir = dirs.data();
    std::vector<int32_t> rej_out((size_t)nrays, 0);
    int32_t* rejected = rej_out.data();
    float bound[6];
    int64_t out[4];
    FlatOctree f;
    WBvh w;
    build_flat_octree(tri9, n, max_depth, leaf_max_obj_count, f);
    build_wbvh(f, w);
    if (f.nodes.empty() || w.nodes.empty())
        return fail("no wide BVH");
    float S = 0.0f;
    for (int a = 0; a < 3; a++)
        S = std::max(S, std::max(std::fabs(f.nodes[0].dn[a]), std::fabs(f.nodes[0].df[a])));
    // (a scale outside the query's gate: the frames run no wide query; the bound is invalid and the
    // rays below are not queried)
    const bool usable = S > 0x1p-20f && S < 0x1p20f;
    const WSceneBound B =
        wbvh_scene_bound(w.nodes[0], cam, nullptr, S, W_QS_CLOSEST, scale_override > 0.0f ? (double)scale_override : 1.0);
    for (int a = 0; a < 3; a++) {
        bound[a] = B.lo[a];
        bound[3 + a] = B.hi[a];
    }
    std::vector<uint64_t> risk;
    const bool cam_finite = std::isfinite(cam[0]) && std::isfinite(cam[1]) && std::isfinite(cam[2]);
    if (usable && cam_finite) {
        const float lo[3] = {f.nodes[0].dn[0], f.nodes[0].dn[1], f.nodes[0].dn[2]};
        const float hi[3] = {f.nodes[0].df[0], f.nodes[0].df[1], f.nodes[0].df[2]};
        const float zero[3] = {0, 0, 0};
        const WRiskArgs RA = wbvh_risk_args(lo, hi, S, cam, zero, W_QS_CLOSEST, W_QS_SHADOW);
        risk.assign(w.nodes.size() * 8, wrisk_pack(INFINITY, 0));
        std::vector<float> lbox(6 * w.tris.size());
        for (size_t k = 0; k < w.tris.size(); k++) {
            const GNode& L = f.nodes[w.leaf_of_k[k]];
            for (int a = 0; a < 3; a++) {
                lbox[6 * k + a] = L.dn[a];
                lbox[6 * k + 3 + a] = L.df[a];
            }
        }
        wbvh_risk_host(w, lbox, RA, 0, risk);
    }
    std::atomic<int64_t> nrej{0}, nviol{0}, nmiss{0};
    const v3 o = mk(cam[0], cam[1], cam[2]);
    const float om = std::max(std::fabs(o.x), std::max(std::fabs(o.y), std::fabs(o.z)));
    const float m = 0x1p-16f * (om + S);
    auto body = [&](int64_t b, int64_t e) {
        WStackArr<W_DEEP_STACK> stk;
        for (int64_t i = b; i < e; i++) {
            const v3 d = mk(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]);
            const bool rej = B.valid && scene_bound_rejects(B.lo, B.hi, o, d);
            rejected[i] = rej ? 1 : 0;
            nrej += rej;
            if (!usable)
                continue;
            bool viol = false;
            for (int pass = 0; pass < (rej ? 2 : 1); pass++) {
                WHit h;
                uint32_t wk[4] = {0, 0, 0, 0};
                const uint64_t* rk = pass == 0 && !risk.empty() ? risk.data() : nullptr;
                const int st = wbvh_closest(w.nodes.data(), w.tris.data(), o, d, m, stk, h, wk, INFINITY, true,
                                                W_QS_CLOSEST, rk, 0, 0.0f);
                if (pass == 0 && st == W_MISS)
                    ++nmiss;
                viol |= rej && (st != W_MISS || wk[0] > 1u);
            }
            nviol += viol;
        }
    };
    unsigned hc = std::max(1u, std::min(std::thread::hardware_concurrency(), 16u));
    std::vector<std::thread> th;
    int64_t chunk = (nrays + hc - 1) / hc;
    for (unsigned k = 0; k < hc; k++) {
        int64_t b = (int64_t)k * chunk, e = std::min(nrays, b + chunk);
        if (b < e)
            th.emplace_back(body, b, e);
    }
    for (auto& x : th)
        x.join();
    out[0] = nviol.load();
    out[1] = nrej.load();
    out[2] = nmiss.load();
    out[3] = B.valid;
    FILE* fo = fopen(argv[2], "wb");
    if (!fo)
        return fail("cannot open the output");
    ok = fwrite(out, 8, 4, fo) == 4 && fwrite(bound, 4, 6, fo) == 6 && fwrite(rejected, 4, rej_out.size(), fo) == rej_out.size();
    fclose(fo);
    return ok ? 0 : fail("short write");
}
