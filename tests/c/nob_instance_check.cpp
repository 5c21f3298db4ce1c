// The wide query's instance without case (b) (wbvh.hpp wbvh_closest<.., NOB = true>) against the
// general instance, on the host (tests/nob_instance_tool.py; librt_mi355x.so's own octree, wide-BVH, risk-word and
// origin-cone builds).  Camera rays: every pixel centre of a rw x rh image, its direction by kernels.hip camera_dir's
// float arithmetic, with the camera's risk words and cap (kernels.hip wide_closest).  Shadow rays: from every
// certified camera hit towards the light, with the light's words, its cap and the origin cones (kernels.hip
// is_shadowed / wide_shadow).  The queries of a ray must agree in status, triangle, the bits of t, u and v, the
// reasons word and the work counters (nodes, triangles, loop iterations):
//   A  the frame kernels' general instance (LAZY: risk words loaded only where !nob) with nob as computed;
//   B  every ray: the general instance as every other caller runs it (the words loaded for every ray with risk
//      keys); where nob holds also the same with nob true and no risk words at all (a nob ray reads none);
//   C  where nob holds: the NOB instance.
// mode 1 (the checker's teeth): the rays whose nob does NOT hold go through C as well; rays whose answers or
// counters then differ from A's are counted (teeth_differ), and the comparison above still runs.
//   nob_instance_check <in> <out>
//   in:  int64 n; int32 max_depth, leaf_max_obj_count, rw, rh, quick, mode, proj_mode, c2w_affine, ocone_dim, no_cap;
//        float proj_w, cam[3], light[3], proj_inv[16], c2w[16]; float tri9[n][9]
//   out: int64[24] (the names in tests/nob_instance_tool.py KEYS); uint8 nob[rh][rw] of the camera rays
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../raytracercpp_amd/csrc/ocone.hpp"
#include "../../raytracercpp_amd/csrc/wbvh.hpp"

using namespace rt;

static int fail(const char* what)
{
    fprintf(stderr, "nob_instance_check: %s\n", what);
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

// one query's answer and work
struct Ans {
    int32_t st, k;
    uint32_t t, u, v, why, nn, nt, steps;
};
static bool same(const Ans& a, const Ans& b)
{
    return a.st == b.st && a.k == b.k && a.t == b.t && a.u == b.u && a.v == b.v && a.why == b.why && a.nn == b.nn &&
           a.nt == b.nt && a.steps == b.steps;
}
static uint32_t bits(float x)
{
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}

// what every query of one kind shares
struct Kind {
    const WBvh* w;
    float hi;
    bool ties;
    float QS;
    const uint64_t* rk;
    int rsel;
    float rsub;
};
template <bool NOB, bool LAZY = false>
static Ans query(const Kind& K, v3 o, v3 d, float m, bool nob, bool words)
{
    WStackLocal stk;
    WHit h;
    uint32_t wk[4] = {0, 0, 0, 0};
    Ans a;
    a.st = wbvh_closest<WStackLocal, 1, WNoFeed, NOB, LAZY>(K.w->nodes.data(), K.w->tris.data(), o, d, m, stk, h, wk, K.hi, K.ties,
                                                      K.QS, words ? K.rk : nullptr, K.rsel, K.rsub, 0u, (WNoFeed*)nullptr, nob);
    a.k = h.k;
    a.t = bits(h.t);
    a.u = bits(h.u);
    a.v = bits(h.v);
    a.why = wk[2];
    a.nn = wk[0];
    a.nt = wk[1];
    a.steps = wk[3];
    return a;
}

// out[base ..]: rays, nob rays, rays with a mismatch in B, nob rays with a mismatch in C, node visits, node visits of nob rays, teeth rays, teeth differ
struct Tally {
    int64_t rays = 0, nob = 0, bad_b = 0, bad_c = 0, visits = 0, visits_nob = 0, teeth = 0, teeth_differ = 0;
};
// A, B and C of one ray; returns A
static Ans check_ray(const Kind& K, v3 o, v3 d, float m, bool nob, bool teeth, Tally& T)
{
    const Ans A = query<false, true>(K, o, d, m, nob, true);
    T.rays++;
    T.visits += A.nn;
    bool bad_b = !same(A, query<false>(K, o, d, m, nob, true));
    if (nob) {
        T.nob++;
        T.visits_nob += A.nn;
        bad_b |= !same(A, query<false>(K, o, d, m, true, false));
        T.bad_c += !same(A, query<true>(K, o, d, m, true, true));
    } else if (teeth) {
        T.teeth++;
        T.teeth_differ += !same(A, query<true>(K, o, d, m, true, true));
    }
    T.bad_b += bad_b;
    return A;
}

int main(int argc, char** argv)
{
    if (argc != 3)
        return fail("usage: nob_instance_check <in> <out>");
    FILE* fi = fopen(argv[1], "rb");
    if (!fi)
        return fail("cannot open the input");
    int64_t n = 0;
    int32_t iv[10];
    Cam P{};
    float light[3];
    bool ok = fread(&n, 8, 1, fi) == 1 && fread(iv, 4, 10, fi) == 10 && fread(&P.proj_w, 4, 1, fi) == 1 &&
              fread(P.pos, 4, 3, fi) == 3 && fread(light, 4, 3, fi) == 3 && fread(P.proj_inv, 4, 16, fi) == 16 &&
              fread(P.c2w, 4, 16, fi) == 16 && n > 0 && n < (1 << 24);
    std::vector<float> tri;
    if (ok) {
        tri.resize((size_t)n * 9);
        ok = fread(tri.data(), 4, tri.size(), fi) == tri.size();
    }
    fclose(fi);
    const int max_depth = iv[0], leaf = iv[1], quick = iv[4], mode = iv[5], c2w_affine = iv[7], ocone_dim = iv[8], no_cap = iv[9];
    P.rw = iv[2];
    P.rh = iv[3];
    P.proj_mode = iv[6];
    if (!ok || P.rw <= 0 || P.rh <= 0 || P.rw > 4096 || P.rh > 4096 || P.proj_mode == 0 || !c2w_affine || ocone_dim < 0 ||
        ocone_dim > 256)
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
    float S = 0.0f;
    for (int a = 0; a < 3; a++)
        S = std::max(S, std::max(std::fabs(f.nodes[0].dn[a]), std::fabs(f.nodes[0].df[a])));
    if (!(S > 0x1p-20f && S < 0x1p20f))
        return fail("the scene's scale is outside the wide query's gate");

    // the risk words and caps of the camera and the light (capi.cpp rt_wbvh_query_ex, renderer.cpp prepare_risk)
    const float lo[3] = {f.nodes[0].dn[0], f.nodes[0].dn[1], f.nodes[0].dn[2]};
    const float hi[3] = {f.nodes[0].df[0], f.nodes[0].df[1], f.nodes[0].df[2]};
    const WRiskArgs RA = wbvh_risk_args(lo, hi, S, P.pos, light, W_QS_CLOSEST, W_QS_SHADOW);
    std::vector<uint64_t> risk(w.nodes.size() * 8, wrisk_pack(INFINITY, 0));
    std::vector<float> lbox(6 * w.tris.size());
    for (size_t k = 0; k < w.tris.size(); k++) {
        const GNode& L = f.nodes[w.leaf_of_k[k]];
        for (int a = 0; a < 3; a++) {
            lbox[6 * k + a] = L.dn[a];
            lbox[6 * k + 3 + a] = L.df[a];
        }
    }
    wbvh_risk_host(w, lbox, RA, 0, risk);
    wbvh_risk_host(w, lbox, RA, 1, risk);
    float cap[2] = {-1.0f, -1.0f};   // (no cap: never skips)
    float cap_dir[2][3] = {};
    int64_t at_risk[2] = {0, 0};
    for (int sel = 0; sel < 2; sel++) {
        if (!RA.on[sel])
            continue;
        const float* X = sel == 0 ? P.pos : light;
        double v[3], l = 0;
        for (int a = 0; a < 3; a++) {
            v[a] = 0.5 * ((double)lo[a] + (double)hi[a]) - (double)X[a];
            l += v[a] * v[a];
        }
        l = std::sqrt(l);
        for (int a = 0; a < 3; a++)
            cap_dir[sel][a] = l > 0 && l < INFINITY ? (float)(v[a] / l) : (a == 0 ? 1.0f : 0.0f);
        const double c[3] = {cap_dir[sel][0], cap_dir[sel][1], cap_dir[sel][2]};
        float sm = INFINITY;
        for (const GTri& t : w.tris)
            if (wbvh_risk_key(t, RA.p[sel][0], RA.p[sel][1], RA.p[sel][2], RA.G[sel], RA.nu[sel], RA.slack[sel], RA.QS[sel]) <
                INFINITY) {
                sm = std::min(sm, risk_cap_tri(t, c));
                at_risk[sel]++;
            }
        if (!no_cap)
            cap[sel] = sm;
    }
    // the origin cones (renderer.cpp start_accel's build)
    OConeGrid ocg;
    OConeView ocv{};
    if (ocone_dim > 0) {
        build_origin_cones(w, S, W_QS_CLOSEST, 0.0102 + 0x1p-16 * S, ocone_dim, 80.0 * 3.14159265358979 / 180.0, 0, ocg);
        if (!ocg.cells.empty()) {
            ocv.cells = ocg.cells.data();
            for (int a = 0; a < 3; a++) {
                ocv.lo[a] = ocg.lo[a];
                ocv.dim[a] = ocg.dim[a];
            }
            ocv.ih = ocg.ih;
        }
    }

    const bool teeth = mode == 1;
    Tally TC, TS;
    std::vector<uint8_t> nobmap((size_t)P.rw * P.rh, 0);
    const int bw = (P.rw + 7) / 8, bh = (P.rh + 7) / 8;
    std::vector<int32_t> tile_rays((size_t)bw * bh, 0), tile_nob((size_t)bw * bh, 0);
    const v3 cam = mk(P.pos[0], P.pos[1], P.pos[2]), lp = mk(light[0], light[1], light[2]);
    const uint64_t* crk = RA.on[0] ? risk.data() : nullptr;
    for (int py = 0; py < P.rh; py++)
        for (int px = 0; px < P.rw; px++) {
            const v3 d = camera_dir(P, px, py);
            if (!(d.x == d.x && d.y == d.y && d.z == d.z))
                continue;
            // kernels.hip wide_closest
            const Kind KC{&w, INFINITY, true, W_QS_CLOSEST, crk, 0, 0.0f};
            const bool nob = crk && cap[0] >= 0.0f && risk_cap_skip(cap[0], cap_dir[0], d, W_QS_CLOSEST);
            const float m = 0x1p-16f * (std::max(std::fabs(cam.x), std::max(std::fabs(cam.y), std::fabs(cam.z))) + S);
            const Ans A = check_ray(KC, cam, d, m, nob, teeth, TC);
            nobmap[(size_t)py * P.rw + px] = nob;
            const size_t b = (size_t)(py >> 3) * bw + (px >> 3);
            tile_rays[b]++;
            tile_nob[b] += nob;
            if (A.st != W_HIT)
                continue;
            // kernels.hip is_shadowed / wide_shadow from the hit point, its normal the record's, turned to the camera
            float t;
            memcpy(&t, &A.t, 4);
            const GTri& T = w.tris[(size_t)A.k];
            v3 nrm = mk(T.n[0], T.n[1], T.n[2]);
            if (!(length2(nrm) > 0.0f))
                continue;
            nrm = normalize(nrm);
            if (dot(nrm, d) > 0.0f)
                nrm = nrm * -1.0f;
            const v3 p = cam + d * t;
            const v3 so = p + nrm * 1.0e-4f, sd = normalize(lp - p);
            if (!(sd.x == sd.x && sd.y == sd.y && sd.z == sd.z))
                continue;
            const float nl = std::fabs(nrm.x) + std::fabs(nrm.y) + std::fabs(nrm.z);
            const float sm = 0x1p-16f * (std::max(std::fabs(so.x), std::max(std::fabs(so.y), std::fabs(so.z))) + S);
            const float shi = (std::sqrt(length2(p - lp)) + 1.0e-4f * nl) * (1.0f + 0x1p-10f) + sm;
            const bool lightk = RA.on[1] && shi <= RA.ray_G && nl <= RA.ray_nl;
            const Kind KS{&w, shi, false, W_QS_SHADOW, lightk ? risk.data() : nullptr, 1,
                          lightk ? wrisk_sub(W_QS_SHADOW, shi, RA.ray_nu) : 0.0f};
            const bool snob = ocone_skip(ocv, so, sd, W_QS_SHADOW) ||
                              (lightk && cap[1] >= 0.0f && risk_cap_skip(cap[1], cap_dir[1], sd, W_QS_SHADOW));
            check_ray(KS, so, sd, sm, snob, teeth, TS);
        }
    int64_t tiles = 0, tiles_nob = 0;
    for (size_t b = 0; b < tile_rays.size(); b++)
        if (tile_rays[b] > 0) {
            tiles++;
            tiles_nob += tile_nob[b] == tile_rays[b];
        }
    const int64_t out[24] = {TC.rays, TC.nob, TC.bad_b, TC.bad_c, TC.visits, TC.visits_nob, TC.teeth, TC.teeth_differ,
                             TS.rays, TS.nob, TS.bad_b, TS.bad_c, TS.visits, TS.visits_nob, TS.teeth, TS.teeth_differ,
                             tiles, tiles_nob, cap[0] >= 0.0f, cap[1] >= 0.0f, at_risk[0], at_risk[1],
                             (int64_t)w.nodes.size(), ocv.cells != nullptr};
    FILE* fo = fopen(argv[2], "wb");
    if (!fo)
        return fail("cannot open the output");
    ok = fwrite(out, 8, 24, fo) == 24 && fwrite(nobmap.data(), 1, nobmap.size(), fo) == nobmap.size();
    fclose(fo);
    return ok ? 0 : fail("short write");
}
