// Entry nodes (wbvh.hpp wbvh_entry_block / wbvh_entry_host and wbvh_closest's start set) against
// the query from the root, on the host (tests/tile_starts_tool.py; librt_mi355x.so's own octree and wide-BVH
// build).  The cut, the mask and the entry sets are computed as renderer.cpp prepare_mask does; every
// pixel-centre ray of the image, its direction by kernels.hip camera_dir's float arithmetic (the affine case)
// moved by 'nudge' ulps per component, runs the unmodified host query from the root and then from its block's
// entry set, both with the camera's risk words and the certificate (kdop_certifies).  The program writes both
// answers of every ray; the test applies the fallback (the oracle's BVH::intersect for what is not certified)
// and compares them.
//   tile_starts_check <in> <out>
//   in:  int64 n; int32 max_depth, leaf_max_obj_count, rw, rh, quick, budget, nudge, proj_mode, c2w_affine, K, fan,
//        hook; float proj_w, cam[3], proj_inv[16], c2w[16]; float tri9[n][9]
//        hook 1 (the checker's teeth): every entry set loses a covering node -- a set of two or more links its
//        first, a set of one link N becomes N's covering children but the first
//   out: int64 {structural violations, mask valid, blocks per row, block rows, blocks below the root, rays certified
//        from the root but not from the entry set, rays certified by both with different records, blocks with a link
//        whose covering children include a leaf}; uint32 sets[block rows][blocks per row][4]; per ray (row-major):
//        int32 status[2], id[2]; float t[2], u[2], v[2] (0: from the root, 1: from the entry set); float d[3]
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../raytracercpp_amd/csrc/wbvh.hpp"

using namespace rt;

static int fail(const char* what)
{
    fprintf(stderr, "tile_starts_check: %s\n", what);
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

struct RayOut {
    int32_t status[2], id[2];
    float t[2], u[2], v[2];
    float d[3];
};

int main(int argc, char** argv)
{
    if (argc != 3)
        return fail("usage: tile_starts_check <in> <out>");
    FILE* fi = fopen(argv[1], "rb");
    if (!fi)
        return fail("cannot open the input");
    int64_t n = 0;
    int32_t iv[12];
    Cam P{};
    bool ok = fread(&n, 8, 1, fi) == 1 && fread(iv, 4, 12, fi) == 12 && fread(&P.proj_w, 4, 1, fi) == 1 &&
              fread(P.pos, 4, 3, fi) == 3 && fread(P.proj_inv, 4, 16, fi) == 16 && fread(P.c2w, 4, 16, fi) == 16 && n > 0;
    std::vector<float> tri;
    if (ok) {
        tri.resize((size_t)n * 9);
        ok = fread(tri.data(), 4, tri.size(), fi) == tri.size();
    }
    fclose(fi);
    const int max_depth = iv[0], leaf = iv[1], quick = iv[4], budget = iv[5], nudge = iv[6], c2w_affine = iv[8], K = iv[9],
              fan = iv[10], hook = iv[11];
    P.rw = iv[2];
    P.rh = iv[3];
    P.proj_mode = iv[7];
    if (!ok || P.rw <= 0 || P.rh <= 0 || P.rw > 4096 || P.rh > 4096)
        return fail("bad input");

    FlatOctree f;
    WBvh w;
    build_flat_octree(tri.data(), n, max_depth, leaf, f);
    if (quick)
        build_wbvh_quick(f, w);
    else
        build_wbvh(f, w);
    if (f.nodes.empty() || w.nodes.empty())
        return fail("no wide BVH");
    const int64_t nn = (int64_t)w.nodes.size();
    float S = 0.0f;
    for (int a = 0; a < 3; a++)
        S = std::max(S, std::max(std::fabs(f.nodes[0].dn[a]), std::fabs(f.nodes[0].df[a])));
    const bool usable = S > 0x1p-20f && S < 0x1p20f;   // (outside: the frames run no wide query)
    const WMaskCam C = wbvh_mask_cam(P.proj_inv, P.c2w, P.proj_mode, P.proj_w, c2w_affine, P.pos, nullptr, S, W_QS_CLOSEST, P.rw, P.rh);
    const int bw = (P.rw + 7) / 8, bh = (P.rh + 7) / 8;
    const bool valid = C.valid && usable && P.proj_mode != 0 && c2w_affine;
    std::vector<uint32_t> cut, words, sets((size_t)bw * bh * W_ENTRY_MAX, W_EMPTY);
    for (size_t b = 0; b < (size_t)bw * bh; b++)
        sets[b * W_ENTRY_MAX] = 0u;
    if (valid) {
        wbvh_cut_host(w.nodes.data(), nn, budget, W_CUT_DEPTH, W_QS_CLOSEST, cut);
        wbvh_mask_host(w.nodes.data(), nn, w.parent.data(), cut, C, words);
        wbvh_entry_host(w.nodes.data(), nn, C, words.data(), K, fan, W_CUT_DEPTH, sets);
    }
    // structure: links packed to the front, inner nodes of the tree, at most K of them; a clear block at the root
    int64_t nstruct = 0, nbelow = 0, nleafpar = 0;
    auto covering = [&](uint32_t node, int bx, int by, uint32_t ch[W_WIDTH]) {
        int cnt = 0;
        for (int j = 0; j < W_WIDTH; j++)
            if (w.nodes[node].child[j] != W_EMPTY && wbvh_rect_holds(wbvh_mask_rect(w.nodes[node], j, C), bx, by))
                ch[cnt++] = w.nodes[node].child[j];
        return cnt;
    };
    for (int by = 0; by < bh; by++)
        for (int bx = 0; bx < bw; bx++) {
            uint32_t* s = &sets[((size_t)by * bw + bx) * W_ENTRY_MAX];
            int nl = 0;
            bool gap = false, leafpar = false;
            for (int i = 0; i < W_ENTRY_MAX; i++) {
                if (s[i] == W_EMPTY) {
                    gap = true;
                    continue;
                }
                nl++;
                if (gap || (s[i] & W_LEAF) || (int64_t)s[i] >= nn)
                    nstruct++;
                else if (valid) {
                    uint32_t ch[W_WIDTH];
                    const int cnt = covering(s[i], bx, by, ch);
                    for (int k = 0; k < cnt; k++)
                        leafpar |= (ch[k] & W_LEAF) != 0;
                }
            }
            if (nl == 0 || nl > K)
                nstruct++;
            const bool cov = valid && ((words[(size_t)by * C.wpr + (bx >> 5)] >> (bx & 31)) & 1u);
            if (s[0] != 0u) {
                nbelow++;
                if (!cov)
                    nstruct++;
            }
            nleafpar += leafpar;
            if (hook == 1 && s[0] != 0u) {
                if (nl >= 2) {
                    for (int i = 0; i + 1 < W_ENTRY_MAX; i++)
                        s[i] = s[i + 1];
                    s[W_ENTRY_MAX - 1] = W_EMPTY;
                } else {
                    uint32_t ch[W_WIDTH];
                    const int cnt = covering(s[0], bx, by, ch);
                    if (cnt >= 2) {
                        for (int i = 0; i < W_ENTRY_MAX; i++)
                            s[i] = i + 1 < cnt ? ch[i + 1] : W_EMPTY;
                    }
                }
            }
        }

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
    std::vector<RayOut> rays((size_t)P.rw * P.rh);
    std::atomic<int64_t> nextra{0}, ndiffer{0};
    const v3 o = mk(P.pos[0], P.pos[1], P.pos[2]);
    const float om = std::max(std::fabs(o.x), std::max(std::fabs(o.y), std::fabs(o.z)));
    const float m = 0x1p-16f * (om + S);
    auto body = [&](int y0, int y1) {
        WStackArr<W_DEEP_STACK> stk;
        for (int py = y0; py < y1; py++)
            for (int px = 0; px < P.rw; px++) {
                v3 d = camera_dir(P, px, py);
                d = mk(nudged(d.x, nudge), nudged(d.y, -nudge), nudged(d.z, (px + py) & 1 ? nudge : -nudge));
                RayOut& R = rays[(size_t)py * P.rw + px];
                R.d[0] = d.x;
                R.d[1] = d.y;
                R.d[2] = d.z;
                const uint32_t* start = &sets[((size_t)(py >> 3) * bw + (px >> 3)) * W_ENTRY_MAX];
                for (int pass = 0; pass < 2; pass++) {
                    R.status[pass] = W_UNCERT;
                    R.id[pass] = -1;
                    R.t[pass] = -1.0f;
                    R.u[pass] = 1.0f;
                    R.v[pass] = 0.0f;
                    if (!usable)
                        continue;
                    WHit h;
                    const uint64_t* rk = risk.empty() ? nullptr : risk.data();
                    int st = wbvh_closest(w.nodes.data(), w.tris.data(), o, d, m, stk, h, nullptr, INFINITY, true, W_QS_CLOSEST,
                                          rk, 0, 0.0f, 0u, (WNoFeed*)nullptr, false, pass ? start : nullptr);
                    if (st == W_DEEP)
                        st = W_UNCERT;
                    if (st == W_HIT) {
                        const int32_t slot = w.slot[(size_t)h.k];
                        if (kdop_certifies(f.nodes[w.leaf_of_slot[(size_t)slot]], o, d, h.t)) {
                            R.id[pass] = f.tri_id[(size_t)slot];
                            R.t[pass] = h.t;
                            R.u[pass] = h.u;
                            R.v[pass] = h.v;
                        } else
                            st = W_UNCERT;
                    }
                    R.status[pass] = st;
                }
                if (R.status[0] != W_UNCERT && R.status[1] == W_UNCERT)
                    ++nextra;
                if (R.status[0] != W_UNCERT && R.status[1] != W_UNCERT &&
                    (R.status[0] != R.status[1] || R.id[0] != R.id[1] || std::memcmp(&R.t[0], &R.t[1], 4) ||
                     std::memcmp(&R.u[0], &R.u[1], 4) || std::memcmp(&R.v[0], &R.v[1], 4)))
                    ++ndiffer;
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
    const int64_t out[8] = {nstruct, valid ? 1 : 0, bw, bh, nbelow, nextra.load(), ndiffer.load(), nleafpar};
    FILE* fo = fopen(argv[2], "wb");
    if (!fo)
        return fail("cannot open the output");
    ok = fwrite(out, 8, 8, fo) == 8 && fwrite(sets.data(), 4, sets.size(), fo) == sets.size() &&
         fwrite(rays.data(), sizeof(RayOut), rays.size(), fo) == rays.size();
    fclose(fo);
    return ok ? 0 : fail("short write");
}
