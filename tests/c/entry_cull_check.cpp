// The entry search's back-face test (wbvh.hpp wbvh_entry_backfacing / wbvh_entry_cover) against
// the per-ray cone test of wbvh_closest, on the host (tests/entry_cull_tool.py; librt_mi355x.so's own octree and
// wide-BVH build).  The cut, the mask and the entry sets are computed as renderer.cpp prepare_mask does.  Then, per
// covered block, every node that can be reached from the root through covering inner children (a superset of the
// nodes the search examines under any policy) is examined, and for every child the block's test drops, each of the
// block's pixel rays -- its direction by kernels.hip camera_dir's float arithmetic (the affine case) moved by 'nudge'
// ulps per component -- must skip that child by the query's own float inequality, a > c cstep.
//   entry_cull_check <in> <out>
//   in:  int64 n; int32 max_depth, leaf_max_obj_count, rw, rh, quick, budget, nudge, proj_mode, c2w_affine, K, fan,
//        cull; float proj_w, cam[3], proj_inv[16], c2w[16]; float tri9[n][9]
//        cull: WMaskCam::cull (0: off, 1: the four corners, 2 (the checker's teeth): the block's centre alone)
//   out: int64 {mask valid, blocks per row, block rows, covered blocks, blocks below the root, nodes examined,
//        children dropped, violations (ray, dropped child) pairs, children of the tree with a cone, structural
//        violations}; uint32 sets[block rows][blocks per row][4]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raytracercpp_amd/csrc/wbvh.hpp"

using namespace rt;

static int fail(const char* what)
{
    fprintf(stderr, "entry_cull_check: %s\n", what);
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

// wbvh_closest's cone test of child j of N for direction d: the same float expressions (setup's dl and cstep)
static bool ray_skips(const WNode& N, int j, v3 d)
{
    const float dl = sqrtf(d.x * d.x + d.y * d.y + d.z * d.z) * (1.0f + 0x1p-20f);
    const float cstep = dl * W_CONE_STEP;
    const uint32_t nrj = N.nrm[j];
    const float nx = (float)(int8_t)(nrj & 0xffu), ny = (float)(int8_t)((nrj >> 8) & 0xffu), nz = (float)(int8_t)((nrj >> 16) & 0xffu);
    const float a = nx * d.x + ny * d.y + nz * d.z;
    return a > (float)(nrj >> 24) * cstep;
}

int main(int argc, char** argv)
{
    if (argc != 3)
        return fail("usage: entry_cull_check <in> <out>");
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
              fan = iv[10], cull = iv[11];
    P.rw = iv[2];
    P.rh = iv[3];
    P.proj_mode = iv[7];
    if (!ok || P.rw <= 0 || P.rh <= 0 || P.rw > 4096 || P.rh > 4096 || cull < 0 || cull > 2)
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
    WMaskCam C = wbvh_mask_cam(P.proj_inv, P.c2w, P.proj_mode, P.proj_w, c2w_affine, P.pos, nullptr, S, W_QS_CLOSEST, P.rw, P.rh);
    C.cull = cull;
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
    int64_t ncones = 0;
    for (const WNode& N : w.nodes)
        for (int j = 0; j < W_WIDTH; j++)
            ncones += N.child[j] != W_EMPTY && (N.nrm[j] >> 24) != 255u;

    int64_t ncov = 0, nbelow = 0, nexam = 0, ndrop = 0, nviol = 0, nstruct = 0;
    std::vector<uint32_t> todo;
    std::vector<int> tdepth;
    for (int by = 0; by < bh && valid; by++)
        for (int bx = 0; bx < bw; bx++) {
            const uint32_t* s = &sets[((size_t)by * bw + bx) * W_ENTRY_MAX];
            const bool cov = (words[(size_t)by * C.wpr + (bx >> 5)] >> (bx & 31)) & 1u;
            bool gap = false;
            for (int i = 0; i < W_ENTRY_MAX; i++) {
                gap |= s[i] == W_EMPTY;
                if (s[i] != W_EMPTY && (gap || (s[i] & W_LEAF) || (int64_t)s[i] >= nn))
                    nstruct++;
            }
            if (s[0] == W_EMPTY || (!cov && s[0] != 0u))
                nstruct++;
            if (!cov)
                continue;
            ncov++;
            nbelow += s[0] != 0u;
            v3 dir[64];
            int nd = 0;
            for (int y = 8 * by; y < 8 * by + 8 && y < P.rh; y++)
                for (int x = 8 * bx; x < 8 * bx + 8 && x < P.rw; x++) {
                    const v3 d = camera_dir(P, x, y);
                    dir[nd++] = mk(nudged(d.x, nudge), nudged(d.y, -nudge), nudged(d.z, (x + y) & 1 ? nudge : -nudge));
                }
            todo.assign(1, 0u);
            tdepth.assign(1, 0);
            while (!todo.empty()) {
                const uint32_t node = todo.back();
                const int depth = tdepth.back();
                todo.pop_back();
                tdepth.pop_back();
                const WNode& N = w.nodes[node];
                nexam++;
                for (int j = 0; j < W_WIDTH; j++)
                    if (N.child[j] != W_EMPTY && wbvh_entry_backfacing(N, j, C, bx, by)) {
                        ndrop++;
                        for (int i = 0; i < nd; i++)
                            nviol += !ray_skips(N, j, dir[i]);
                    }
                uint32_t ch[W_WIDTH];
                bool inner;
                const int cnt = wbvh_entry_cover(N, nn, C, bx, by, ch, inner);
                for (int k = 0; k < cnt && depth + 1 < W_CUT_DEPTH; k++)
                    if (!(ch[k] & W_LEAF) && (int64_t)ch[k] < nn) {
                        todo.push_back(ch[k]);
                        tdepth.push_back(depth + 1);
                    }
            }
        }
    const int64_t out[10] = {valid ? 1 : 0, bw, bh, ncov, nbelow, nexam, ndrop, nviol, ncones, nstruct};
    FILE* fo = fopen(argv[2], "wb");
    if (!fo)
        return fail("cannot open the output");
    ok = fwrite(out, 8, 10, fo) == 10 && fwrite(sets.data(), 4, sets.size(), fo) == sets.size();
    fclose(fo);
    return ok ? 0 : fail("short write");
}
