// The tile mask (wbvh.hpp wbvh_cut_host / wbvh_mask_cam / wbvh_mask_host) against the query
// it shortcuts, on the host (tests/tile_mask_tool.py; librt_mi355x.so's own octree and wide-BVH build).  The
// cut and the mask are computed as renderer.cpp prepare_mask does; every pixel-centre ray of the image, its
// direction by kernels.hip camera_dir's float arithmetic (restated below for the affine case, the only one
// with a mask) and moved by 'nudge' ulps per component, runs the unmodified host query with the camera's
// risk words; the rays of a block whose bit is clear run it without them as well.  A ray of a clear block
// that does not end as W_MISS, or tests a triangle, is a violation.
//   tile_mask_check <in> <out>
//   in:  int64 n; int32 max_depth, leaf_max_obj_count, rw, rh, quick, budget, nudge, proj_mode, c2w_affine, guard_set;
//        float scale_override, guard_override, proj_w, cam[3], proj_inv[16], c2w[16]; float tri9[n][9]
//   out: int64 {violations, mask valid, cut entries, blocks per row, block rows, scene bound valid};
//        uint8 per block (row-major): bit 0 covered (the mask's bit), bit 1 some ray of the block does not end
//        as a miss without a triangle test, bit 2 the scene bound rejects every ray of the block
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
    fprintf(stderr, "tile_mask_check: %s\n", what);
    return 1;
}

struct Cam {
    float proj_inv[16], c2w[16], proj_w, pos[3];
    int32_t proj_mode, rw, rh;
};

// kernels.hip camera_dir with proj_mode != 0 and c2w_affine, the same float expressions in the same order
static v3 camera_dir(const Cam& P, int px, int py)
{
    const float y_world = ((float)py + 0.5f) / P.rh * 2 - 1;
    const float x_world = ((float)px + 0.5f) / P.rw * 2 - 1;
    const float* m = P.proj_inv;
    const float x = x_world, y = y_world, z = -1.0f;
    const float xt = m[0] * x + m[1] * y + m[2] * z + m[3];
    const float yt = m[4] * x + m[5] * y + m[6] * z + m[7];
    const float zt = m[8] * x + m[9] * y + m[10] * z + m[11];
    const float w = P.proj_w;
    const v3 vs = P.proj_mode == 1 ? mk(xt, yt, zt) : mk(xt * w, yt * w, zt * w);
    const float* c = P.c2w;
    const v3 ws = mk(c[0] * vs.x + c[1] * vs.y + c[2] * vs.z + c[3], c[4] * vs.x + c[5] * vs.y + c[6] * vs.z + c[7],
                     c[8] * vs.x + c[9] * vs.y + c[10] * vs.z + c[11]);
    return normalize(ws - mk(P.pos[0], P.pos[1], P.pos[2]));
}

static float nudged(float v, int k)
{
    for (int i = 0; i < (k < 0 ? -k : k); i++)
        v = std::nextafter(v, k > 0 ? INFINITY : -INFINITY);
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 3)
        return fail("usage: tile_mask_check <in> <out>");
    FILE* fi = fopen(argv[1], "rb");
    if (!fi)
        return fail("cannot open the input");
    int64_t n = 0;
    int32_t iv[10];
    float fv[3];
    Cam P{};
    bool ok = fread(&n, 8, 1, fi) == 1 && fread(iv, 4, 10, fi) == 10 && fread(fv, 4, 3, fi) == 3 && fread(P.pos, 4, 3, fi) == 3 &&
              fread(P.proj_inv, 4, 16, fi) == 16 && fread(P.c2w, 4, 16, fi) == 16 && n > 0;
    std::vector<float> tri;
    if (ok) {
        tri.resize((size_t)n * 9);
        ok = fread(tri.data(), 4, tri.size(), fi) == tri.size();
    }
    fclose(fi);
    const int max_depth = iv[0], leaf = iv[1], quick = iv[4], budget = iv[5], nudge = iv[6], c2w_affine = iv[8], guard_set = iv[9];
    P.rw = iv[2];
    P.rh = iv[3];
    P.proj_mode = iv[7];
    P.proj_w = fv[2];
    if (!ok || P.rw <= 0 || P.rh <= 0 || P.rw > 4096 || P.rh > 4096)
        return fail("bad input");
    const double scale = fv[0] > 0.0f ? (double)fv[0] : 1.0, guard = fv[1];

    FlatOctree f;
    WBvh w;
    build_flat_octree(tri.data(), n, max_depth, leaf, f);
    if (quick)
        build_wbvh_quick(f, w);
    else
        build_wbvh(f, w);
    if (f.nodes.empty() || w.nodes.empty())
        return fail("no wide BVH");
    float S = 0.0f;
    for (int a = 0; a < 3; a++)
        S = std::max(S, std::max(std::fabs(f.nodes[0].dn[a]), std::fabs(f.nodes[0].df[a])));
    const bool usable = S > 0x1p-20f && S < 0x1p20f;   // (outside: the frames run no wide query)
    std::vector<uint32_t> cut, words;
    wbvh_cut_host(w.nodes.data(), (int64_t)w.nodes.size(), budget, W_CUT_DEPTH, W_QS_CLOSEST, cut);
    WMaskCam C = wbvh_mask_cam(P.proj_inv, P.c2w, P.proj_mode, P.proj_w, c2w_affine, P.pos, nullptr, S, W_QS_CLOSEST, P.rw, P.rh,
                               guard_set ? &guard : nullptr, scale);
    const int bw = (P.rw + 7) / 8, bh = (P.rh + 7) / 8;
    // a mask that holds a whole-image entry is what the frames get as well; "valid" here: the camera has a
    // mask and some block is clear
    bool valid = C.valid && usable && P.proj_mode != 0 && c2w_affine;
    if (valid)
        wbvh_mask_host(w.nodes.data(), (int64_t)w.nodes.size(), w.parent.data(), cut, C, words);
    std::vector<uint8_t> blocks((size_t)bw * bh, 1);
    bool any_clear = false;
    if (valid)
        for (int by = 0; by < bh; by++)
            for (int bx = 0; bx < bw; bx++) {
                const bool cov = (words[(size_t)by * C.wpr + (bx >> 5)] >> (bx & 31)) & 1u;
                blocks[(size_t)by * bw + bx] = cov ? 1 : 0;
                any_clear |= !cov;
            }
    valid = valid && any_clear;
    const WSceneBound B = wbvh_scene_bound(w.nodes[0], P.pos, nullptr, S, W_QS_CLOSEST);

    std::vector<uint64_t> risk;
    if (usable && std::isfinite(P.pos[0]) && std::isfinite(P.pos[1]) && std::isfinite(P.pos[2])) {
        const float lo[3] = {f.nodes[0].dn[0], f.nodes[0].dn[1], f.nodes[0].dn[2]};
        const float hi[3] = {f.nodes[0].df[0], f.nodes[0].df[1], f.nodes[0].df[2]};
        const float zero[3] = {0, 0, 0};
        const WRiskArgs RA = wbvh_risk_args(lo, hi, S, P.pos, zero, W_QS_CLOSEST, W_QS_SHADOW);
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
    std::atomic<int64_t> nviol{0};
    std::vector<std::atomic<uint8_t>> flags((size_t)bw * bh);
    for (auto& x : flags)
        x = 0;
    const v3 o = mk(P.pos[0], P.pos[1], P.pos[2]);
    const float om = std::max(std::fabs(o.x), std::max(std::fabs(o.y), std::fabs(o.z)));
    const float m = 0x1p-16f * (om + S);
    auto body = [&](int y0, int y1) {
        WStackArr<W_DEEP_STACK> stk;
        for (int py = y0; py < y1; py++)
            for (int px = 0; px < P.rw; px++) {
                v3 d = camera_dir(P, px, py);
                d = mk(nudged(d.x, nudge), nudged(d.y, -nudge), nudged(d.z, (px + py) & 1 ? nudge : -nudge));
                const size_t b = (size_t)(py >> 3) * bw + (px >> 3);
                const bool clear = !(blocks[b] & 1);
                if (!(B.valid && scene_bound_rejects(B.lo, B.hi, o, d)))
                    flags[b] |= 4;   // (bit 2 is inverted below)
                if (!usable)
                    continue;
                for (int pass = 0; pass < (clear ? 2 : 1); pass++) {
                    WHit h;
                    uint32_t wk[4] = {0, 0, 0, 0};
                    const uint64_t* rk = pass == 0 && !risk.empty() ? risk.data() : nullptr;
                    const int st = wbvh_closest(w.nodes.data(), w.tris.data(), o, d, m, stk, h, wk, INFINITY, true, W_QS_CLOSEST,
                                                rk, 0, 0.0f);
                    if (st != W_MISS || wk[1] > 0u) {
                        flags[b] |= 2;
                        if (clear)
                            ++nviol;
                    }
                }
            }
    };
    const int hc = (int)std::max(1u, std::min(std::thread::hardware_concurrency(), 16u));
    std::vector<std::thread> th;
    const int chunk = (P.rh + hc - 1) / hc;
    for (int k = 0; k < hc; k++) {
        const int y0 = k * chunk, y1 = std::min((int)P.rh, y0 + chunk);
        if (y0 < y1)
            th.emplace_back(body, y0, y1);
    }
    for (auto& x : th)
        x.join();
    for (size_t b = 0; b < blocks.size(); b++)
        blocks[b] = (uint8_t)((blocks[b] & 1) | (flags[b] & 2) | ((flags[b] & 4) ? 0 : 4));
    const int64_t out[6] = {nviol.load(), valid ? 1 : 0, (int64_t)cut.size(), bw, bh, B.valid};
    FILE* fo = fopen(argv[2], "wb");
    if (!fo)
        return fail("cannot open the output");
    ok = fwrite(out, 8, 6, fo) == 6 && fwrite(blocks.data(), 1, blocks.size(), fo) == blocks.size();
    fclose(fo);
    return ok ? 0 : fail("short write");
}
