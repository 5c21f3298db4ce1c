// wbvh.hpp -- a 4-wide SAH bounding-volume hierarchy over the octree's triangle records,
// used to find primary-ray hits fast, and the certificate that makes its answer the
// reference's.
//
// The reference's BVH::intersect (tp2/projets/bvh.h:212-287) returns the closest hit
// among the triangles of the octree leaves it visits, folded in its visit order.  The
// wide BVH below finds the minimum-t hit t* over ALL triangles (its boxes contain every
// point Moller-Trumbore can report as a hit; the kernel widens them by a margin far above
// the rounding of the test).  That is the reference's record when
//   (1) t* is finite and > 0, no other triangle hits at exactly t*, and no tested hit is NaN;
//   (2) the octree leaf L holding t*'s triangle passes the reference's own k-DOP test
//       (BoundingVolume::intersect, bvh.h:79-105, the same IEEE arithmetic) with t_near <= t*.
// Every ancestor's slabs contain L's (min / max over more triangles), and rounding is
// monotone, so each ancestor's computed t_near is <= L's and its t_far >= L's: every node
// on the path passes and none is skipped by the early-out (bvh.h:270: that needs an
// earlier record t_A < t_near <= t*, and t* is the minimum).  The reference therefore
// tests t*'s triangle and its record ends at t* with the same (t, u, v), and every node on
// the path returns true.  A query the certificate does not cover (ties, t* <= 0 or
// infinite, a NaN hit, a traversal stack overflow, (2) failing) is re-traced by the exact
// octree traversal.  With no hit at all, the reference finds none either and returns false
// with a fresh record.
//
// Layout (HBM): WNode 128 B (struct WNode below), the four children's boxes quantised to 8 bits
// per plane against the node's own frame (Ylitie et al.'s compressed wide nodes, 4-wide):
//   float4 0: origin x, y, z (the node box's low corner) and the three scale exponents
//             (byte a = biased exponent of the power-of-two step s_a along axis a);
//   float4 1: q_lo x[4], q_lo y[4], q_lo z[4], q_hi x[4] (one byte per child);
//   float4 2: q_hi y[4], q_hi z[4], the slab scale and offset;
//   float4 3 / 4: the slab normals and cones / the slab ranges;
//   float4 5: the four child links:
//     inner child:  node index (bit 31 clear);
//     leaf child:   W_LEAF | first << 3 | (count - 1), triangles first .. first + count - 1
//                   of the wide BVH's own triangle order (count <= 8);
//     no child:     W_EMPTY.
//   float4 6 / 7: the conditioning bytes of the sound child test (ext, ext2).
// Child box = [origin + q_lo s, origin + q_hi s] with q_lo rounded down and q_hi up, so
// it holds the float box exactly (checked in double by check_wbvh).
// Triangles: GTri records (octree.hpp) copied in leaf order, plus slot[] = the octree GTri
// slot of each, and leaf_of_slot[] = the flattened octree leaf node holding each slot.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "octree.hpp"

namespace rt {

constexpr uint32_t W_LEAF = 0x80000000u;
constexpr uint32_t W_EMPTY = 0xFFFFFFFFu;
constexpr int W_MAX_LEAF = 8;
#ifndef W_STACK_N
#define W_STACK_N 16
#endif
constexpr int W_STACK = W_STACK_N;   // traversal stack entries per lane (a child dropped by a full stack
                                     // whose key is at most the final best hit: the query is not certified)
constexpr int W_WIDTH = 4;    // children per node

// the grazing split QS of the wide query's child test per query kind (wbvh_closest, wbvh_risk_key):
// (a)'s reach grows as 1 / QS (wq_reach: its D term is 10.87u D / QS), the risk set of case (b) as QS.
// r05, with the correlated reach (tools/visit_probe.py, host wide-node visits per C4 ray, every 8th
// tile row): camera 2^-8 / 2^-10 / 2^-12 / 2^-14: 5.71 / 5.15 / 4.83 / 52 (at 2^-14 the pole slivers'
// s q falls below the bound's 5.86u: no reach); shadow 2^-11 / 2^-12 / 2^-13 / 2^-14: 7.72 / 7.06 /
// 8.61 / 8.55.  On the GPU (three scenes, so that the choice is not the headline sphere's alone,
// profiles/r05/qs_scenes.log): camera 2^-10 is ahead of 2^-8 on C4 (+7.8%), hair1m (+5%) and robot
// (+1%); 2^-12 is ahead on C4 only (hair1m -6%, robot -4%)
#ifndef W_QS_CLOSEST
#define W_QS_CLOSEST 0x1p-10f
#endif
#ifndef W_QS_SHADOW
#define W_QS_SHADOW 0x1p-12f
#endif

#ifndef W_SMIN_FLOOR
#define W_SMIN_FLOOR 0.0f   // (diagnostic builds: a floor on the children's smin, to price the slivers' widening)
#endif

#ifndef W_STEP_HOOK
#define W_STEP_HOOK(cur, leaf)   // diagnostic builds (kernels.hip): per-step wave statistics
#endif
#ifndef W_NOB_HOOK
#define W_NOB_HOOK(nob)   // diagnostic builds (kernels.hip): the node steps whose lanes all skip case (b)
#endif

// Case (b) of wbvh_closest for rays that skip it (nob):
//   0: the risk words are loaded for every ray with risk keys, and every query runs the general instance;
//   1: in the frame kernels' queries (wbvh_closest<.., LAZY = true>, kernels.hip wide_run's NOBF) the risk words
//      are loaded only by the lanes that can read them (risk keys and !nob);
//   2: 1, and a wave of those queries whose active lanes all have nob runs the instance compiled without
//      case (b) (wbvh_closest<.., NOB = true>).
#ifndef W_NOB_FAST
#define W_NOB_FAST 2
#endif

// cone threshold step: c in 0..254 encodes c * 224 / 254 >= |N| (|N| <= 127 sqrt 3 < 220), so 255
// can never pass.  W_CONE_EPS: the triangles' minimum cos(normal, d) the build guarantees
constexpr float W_CONE_STEP = 224.0f / 254.0f;
constexpr double W_CONE_EPS = 1e-4;

struct alignas(16) WNode {
    float ox, oy, oz;
    uint32_t exps;        // byte a: biased exponent (127 + k) of the step 2^k along axis a
    uint8_t qlo[3][W_WIDTH];    // [axis][child]
    uint8_t qhi[3][W_WIDTH];
    // Orientation slab of child j: every vertex v below it has
    //   slo + q0 s  <=  N_j . (v - origin)  <=  slo + q1 s,
    // N_j = nrm bytes 0..2 as signed 8-bit integers (the subtree's area-weighted normal,
    // quantised to [-127, 127]), q0 / q1 the low / high 16 bits of slab[j].  A curved patch is thin
    // along its mean normal, so a ray that grazes the surface misses most patches' slabs
    // although it crosses their boxes (silhouette rays).
    // Backface cone of child j: nrm byte 3 = c, 255 = none.  Every triangle
    // below j that Moller-Trumbore could ever hit faces away from a ray whose direction d has
    //   N_j . d  >  c * W_CONE_STEP * |d|
    // (the test rejects it on Mdet <= 0 before anything else), so such a ray skips j.
    float s, slo;
    uint32_t nrm[W_WIDTH];
    uint32_t slab[W_WIDTH];
    uint32_t child[W_WIDTH];
    // Conditioning of child j's triangles (the grazing-sound query), one byte each,
    // as 8-bit minifloats (wn_code / wn_decode):
    //   ext[j]  byte 0: smin, a lower bound on sin(alpha) (alpha: the triangle's angle at a);
    //           byte 1: s2, a lower bound on sin(alpha' / 2), alpha' = min(alpha, pi - alpha);
    //           byte 2: sth, an upper bound on sin(angle(N_j, n)) over the triangles' exact normals;
    //           byte 3: lmax, an upper bound on their edges |ab|, |ac|;
    //   ext2[j] byte 0: rho, how far the k-DOP boxes of the octree leaves holding them reach past
    //           the child's box (0 when the child holds whole octree leaves); bytes 1-3 unused.
    uint32_t ext[W_WIDTH];
    uint32_t ext2[W_WIDTH];
};
static_assert(sizeof(WNode) == 128, "WNode size");
// word offsets inside a node (the kernel loads it as 16-B rows and picks words)
constexpr int WN_QLO = 4;                           // qlo[a] starts at word WN_QLO + a * W_WIDTH / 4
constexpr int WN_QHI = 4 + 3 * W_WIDTH / 4;         // qhi[a] at WN_QHI + a * W_WIDTH / 4
constexpr int WN_SS = 4 + 6 * W_WIDTH / 4;          // s, slo
constexpr int WN_NRM = ((4 + 6 * W_WIDTH / 4 + 2 + 3) / 4) * 4;
constexpr int WN_SLAB = WN_NRM + W_WIDTH;
constexpr int WN_CHILD = WN_SLAB + W_WIDTH;
constexpr int WN_EXT = WN_CHILD + W_WIDTH;
constexpr int WN_EXT2 = WN_EXT + W_WIDTH;
constexpr int WN_ROWS = (int)(sizeof(WNode) / 16);

// The conditioning bytes: value(k) = float with bits (k << 20) + base for k > 0 (three mantissa
// bits, an octave per 8 codes); k = 0 is 0.  Unit quantities (sines) use WQ_UNIT (k = 255 is
// 1.0), lengths WQ_LEN (2^-16 .. 2^16; k = 255 stands for "no bound", infinity).
constexpr uint32_t WQ_UNIT = 0x3F800000u - (255u << 20);
constexpr uint32_t WQ_LEN = 111u << 23;
RT_HD float wq_val(uint32_t k, uint32_t base)
{
    return k == 0u ? 0.0f : __builtin_bit_cast(float, (k << 20) + base);
}
RT_HD float wq_len(uint32_t k)
{
    return k == 255u ? INFINITY : wq_val(k, WQ_LEN);
}
// code k read as if k = 0 stood for the smallest nonzero value (2^-19 x the top value for WQ_UNIT,
// 2^-16 for WQ_LEN): a larger upper bound, or, for a lower bound used only as a divisor whose tiny
// values already mean "no bound" (the query's smin, s2), the same decision as 0
RT_HD float wq_val_nz(uint32_t k, uint32_t base)
{
    return __builtin_bit_cast(float, (k << 20) + base);
}

struct WStats {
    int64_t nodes = 0, leaves = 0, tris = 0, max_leaf = 0, depth = 0;
    float sah = 0.0f;   // SAH cost of the binary tree (traversal 1, triangle 1), for diagnostics
};

struct WBvh {
    std::vector<WNode> nodes;          // nodes[0] = root (empty when there are no triangles)
    std::vector<GTri> tris;            // octree records in leaf order
    std::vector<int32_t> slot;         // wide-BVH triangle -> octree GTri slot
    std::vector<uint32_t> leaf_of_slot;   // octree GTri slot -> flattened octree leaf node
    std::vector<uint32_t> leaf_of_k;      // wide-BVH triangle -> flattened octree leaf node (= leaf_of_slot[slot])
    // the grazing-risk walk (wbvh_risk_tri): wide-BVH triangle -> its leaf child (node << 2 | slot),
    // node -> its parent's child entry (parent << 2 | slot; W_EMPTY for the root)
    std::vector<uint32_t> tri_leaf, parent;
    WStats stats;
};

// A lower bound on sin(angle at a) of the record's edges ab, ac (floats) from the exact cross
// product: the double products of floats are exact, each difference rounds once (2^-53 of the
// larger term), so |ab x ac| >= |cross_double| - 2^-51 |ab| |ac|.  1 for a zero cross product
// of non-zero edges is not claimed: 0 then (never skipped by the query's margins).
// (host and device: the quick tree's builders, wbvh_quick.hpp)
RT_HD double sin_at_a_lb(const GTri& t)
{
    const double x0 = t.ab[0], x1 = t.ab[1], x2 = t.ab[2], y0 = t.ac[0], y1 = t.ac[1], y2 = t.ac[2];
    const double c0 = x1 * y2 - x2 * y1, c1 = x2 * y0 - x0 * y2, c2 = x0 * y1 - x1 * y0;
    const double ab = sqrt(x0 * x0 + x1 * x1 + x2 * x2), ac = sqrt(y0 * y0 + y1 * y1 + y2 * y2);
    const double lam = ab * ac;
    if (!(lam > 0x1p-100) || !(lam < 0x1p100))
        return 0.0;
    const double c = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
    const double v = (c - 0x1p-50 * lam) / lam * (1 - 1e-12);
    return 0.0 < v ? v : 0.0;   // (std::max(0.0, v))
}

// sin of the triangle's angle at a (Moller-Trumbore's vertex) as a float rounded down, from the
// exact cross product of the record's edges (sin_at_a_lb; the stored normal's own rounding could
// make |n| / (|ab| |ac|) overestimate it); 1 for n = 0 (never hit: Mdet = 0); 0 where the
// rounding analysis of DESIGN.md 5.6 does not apply (|n| outside [2^-60, 2^60], |ab| |ac|
// outside (2^-100, 2^100)).  Host only (kernels.hip leaf_missed's margin).
inline float sin_at_a_f(const GTri& t)
{
    const double n = std::sqrt((double)t.n[0] * t.n[0] + (double)t.n[1] * t.n[1] + (double)t.n[2] * t.n[2]);
    if (n == 0)
        return 1.0f;
    if (!(n >= 0x1p-60 && n <= 0x1p60))
        return 0.0f;
    const double sl = sin_at_a_lb(t);
    const float f = (float)sl;
    return (double)f > sl ? std::nextafter(f, 0.0f) : f;
}

// Binned-SAH binary build over the octree's triangle records, collapsed to 4-wide nodes
// (RT_BUILD_THREADS threads, as the octree build).  Boxes are the records' vertices a,
// a + ab, a + ac rounded outward to float.
void build_wbvh(const FlatOctree& oct, WBvh& out);
// The quick tree (r05, wbvh.cpp): the octree's own hierarchy as the wide BVH, O(n) to build, for the
// frames right after a geometry change while the SAH tree builds; RT_WBVH_QUICK=1 makes
// build_wbvh build it instead.
// tris = false: WBvh::tris left empty (the renderer gathers the records on the device; wbvh_fill_tris
// makes the host copy when a host check needs it).
void build_wbvh_quick(const FlatOctree& oct, WBvh& out, bool tris = true);
void wbvh_fill_tris(const FlatOctree& oct, WBvh& w);

// Structural check (CPU tests): every octree slot exactly once, each child box holds its
// subtree's boxes / its triangles' vertices, leaf sizes within W_MAX_LEAF, leaf_of_slot
// consistent with the octree.  Returns the number of violations.
int64_t check_wbvh(const FlatOctree& oct, const WBvh& w);

// ---------------------------------------------------------------------------------
// Traversal (host and device).  One query: the closest Moller-Trumbore hit over the
// wide BVH, then the certificate against the octree.

// Triangle::intersect, triangle.cpp:25-91 (backface culling), on a GTri record: the
// same expressions in the same order as the reference (and kernels.hip tri_test_rec).
RT_HD bool mt_record(const GTri& T, v3 o, v3 d, float& t_out, float& u_out, float& v_out)
{
    v3 a = mk(T.a[0], T.a[1], T.a[2]);
    v3 ab = mk(T.ab[0], T.ab[1], T.ab[2]);
    v3 ac = mk(T.ac[0], T.ac[1], T.ac[2]);
    v3 n = mk(T.n[0], T.n[1], T.n[2]);
    v3 OA = o - a;
    v3 nd = -d;
    v3 m = cross(nd, OA);
    float Mdet = dot(n, nd);
    if (Mdet <= 0)
        return false;
    float inv = 1 / Mdet;
    float u = dot(m, ac) * inv;
    if (u < 0 || u > 1)
        return false;
    float v = dot(m, -ab) * inv;
    if (v < 0 || u + v > 1)
        return false;
    float t = dot(n, OA) * inv;
    t_out = t;
    u_out = u;
    v_out = v;
    return !(t < 0);
}

RT_HD GTri load_gtri(const GTri* p)
{
    const float4* q = reinterpret_cast<const float4*>(p);
    float4 a = ldg(q), b = ldg(q + 1), c = ldg(q + 2);
    GTri g;
    g.a[0] = a.x; g.a[1] = a.y; g.a[2] = a.z;
    g.ab[0] = a.w; g.ab[1] = b.x; g.ab[2] = b.y;
    g.ac[0] = b.z; g.ac[1] = b.w; g.ac[2] = c.x;
    g.n[0] = c.y; g.n[1] = c.z; g.n[2] = c.w;
    return g;
}

RT_HD GNode load_gnode(const GNode* p)
{
    const float4* q = reinterpret_cast<const float4*>(p);
    float4 a = ldg(q), b = ldg(q + 1), c = ldg(q + 2), d = ldg(q + 3);
    GNode g;
    g.dn[0] = a.x; g.dn[1] = a.y; g.dn[2] = a.z; g.dn[3] = a.w;
    g.dn[4] = b.x; g.dn[5] = b.y; g.dn[6] = b.z;
    g.df[0] = b.w; g.df[1] = c.x; g.df[2] = c.y; g.df[3] = c.z; g.df[4] = c.w;
    g.df[5] = d.x; g.df[6] = d.y;
    g.a = __builtin_bit_cast(uint32_t, d.z);
    g.b = __builtin_bit_cast(uint32_t, d.w);
    return g;
}

// sqrt within 1 ulp on the device (the hardware instruction), correctly rounded on the host; callers
// round up by far more than 1 ulp where they need an upper bound
RT_HD float fast_sqrt(float a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sqrtf(a);
#else
    return std::sqrt(a);
#endif
}

RT_HD float fast_rcp(float a)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_rcpf(a);
#elif defined(RT_TEST_RCP_HOOK)
    return RT_TEST_RCP_HOOK(a);   // tests/c/kdop_fast.cpp: a reciprocal a few ulps off
#else
    // host emulation: the correctly rounded reciprocal (the device's is within 1 ulp of it;
    // both stay inside the slab margin)
    return 1.0f / a;
#endif
}

// BoundingVolume::intersect (bvh.h:79-105) with the ray's plane products as
// OctreeNode::intersect computes them (bvh.h:216-223), branch-free as kernels.hip
// vol_test: returns pass && t_near <= t.
// Case (b)'s bound on the origin's distance from a triangle's plane: with q = |cos(n,
// d)| < QS, s = sin(alpha) (the angle at a), s2 = sin(alpha' / 2), L >= the edges, D >= |o - a| and u =
// 2^-24, a hit Moller-Trumbore reports (u', v' in [0, 1]; triangle.cpp:25-91) puts the origin within
//   H0 = 1.01 [QS (2L + D) + u (24.2 L + 48 D) / s + u (30 L + 12 D + 24 D / s) / s2]
// of the plane: for q s >= 24u the exact line-plane point P0 has barycentrics within 1 + (12.1u + 24u
// D / |e|) / (q s) of [0, 1] (numerator and Mdet rounding), so |P0 - a| <= 2L + u (24.2 L + 48 D) / (q s),
// and the distance is q |P0 - o| <= q (|P0 - a| + D); below, Mdet < 30u |ab||ac||d| bounds both
// barycentric numerators U = -alpha d.n - gamma d.(n x ac), V = -beta d.n + gamma d.(n x ab), and the
// larger of |d.(n x ab)| / |ab|, |d.(n x ac)| / |ac| is at least s2 |d|.  Device: the hardware
// reciprocal (1 ulp), inside the 1.01.
RT_HD float wq_h0(float QS, float L, float D, float s, float s2)
{
    constexpr float U = 0x1p-24f;
    const float is = fast_rcp(s), is2 = fast_rcp(s2);
    const float a = __builtin_fmaf(QS, 2.0f * L + D, U * __builtin_fmaf(24.2f, L, 48.0f * D) * is);
    return 1.01f * __builtin_fmaf(U * __builtin_fmaf(30.0f, L, __builtin_fmaf(24.0f, D * is, 12.0f * D)), is2, a);
}

RT_HD bool kdop_certifies_exact(const GNode& nd, v3 o, v3 d, float t)
{
    float t_near = -INFINITY, t_far = INFINITY;
#pragma unroll
    for (int i = 0; i < NPLANES; i++) {
        v3 n = mk(PLANE_N[i][0], PLANE_N[i][1], PLANE_N[i][2]);
        float den = dot(n, d);
        float num = dot(n, o);
        if (den == 0.0f)
            num = __builtin_nanf("");   // skipped plane (bvh.h:86-87): NaN quotients are ignored
        float d0 = (nd.dn[i] - num) / den;
        float d1 = (nd.df[i] - num) / den;
        t_near = fmaxf(t_near, fminf(d0, d1));
        t_far = fminf(t_far, fmaxf(d0, d1));
    }
    return !(t_far < t_near) && t_near <= t;
}

// The same decision, first from quotients through the hardware reciprocal (1 ulp): each is
// within 2^-21 of the correctly rounded one (relative), a max / min of them within 2^-21 of its
// exact counterpart's magnitude, so a comparison won by more than 2^-19 (|t_near| + |t_far| + |t|)
// is the exact comparison's.  Closer calls, a denominator below 2^-100 (reciprocal range) and
// infinite bounds take the correctly rounded divisions.  The numerators are the reference's.
RT_HD bool kdop_certifies(const GNode& nd, v3 o, v3 d, float t)
{
    float t_near = -INFINITY, t_far = INFINITY;
    bool tiny = false;
#pragma unroll
    for (int i = 0; i < NPLANES; i++) {
        v3 n = mk(PLANE_N[i][0], PLANE_N[i][1], PLANE_N[i][2]);
        float den = dot(n, d);
        float num = dot(n, o);
        if (den == 0.0f)
            num = __builtin_nanf("");
        tiny |= den != 0.0f && !(fabsf(den) >= 0x1p-100f);
        const float r = fast_rcp(den);
        float d0 = (nd.dn[i] - num) * r;
        float d1 = (nd.df[i] - num) * r;
        t_near = fmaxf(t_near, fminf(d0, d1));
        t_far = fminf(t_far, fmaxf(d0, d1));
    }
    const float e = (fabsf(t_near) + fabsf(t_far) + fabsf(t)) * 0x1p-19f;
    if (!tiny && fabsf(t_near) < INFINITY && fabsf(t_far) < INFINITY && e < INFINITY) {
        if (t_far - t_near > e && t - t_near > e)
            return true;
        if (t_near - t_far > e || t_near - t > e)
            return false;
    }
    return kdop_certifies_exact(nd, o, d, t);
}

RT_HD uint32_t fbits(float f) { return __builtin_bit_cast(uint32_t, f); }
RT_HD float bitsf(uint32_t u) { return __builtin_bit_cast(float, u); }

// Grazing risk of a triangle for a point X ("risk keys"): INFINITY when no ray of the
// kind X stands for can make the triangle report a hit in case (b) of wbvh_closest (|cos(n, d)| = q <
// QS); otherwise a key K >= 0 such that every hit it reports in case (b) has
//   t' >= (K - QS hi - nu) / (QS |d|)      (camera: t' >= K / (QS |d|)).
// Case (b) puts the ray's origin o within H0(D = |o - a|) of the triangle's plane (wq_h0; s2 =
// sin(alpha' / 2) as the build's ext byte 1, L = the longer edge).  And with s = sin(alpha)
// and u = 2^-24, Moller-Trumbore's float quantities (triangle.cpp:25-91; stored normal n within
// 2.83u |ab||ac| of the exact one) satisfy |Mdet| <= (q + 6u/s) |n~||d| and |n . OA| >= |n~| (dist(o) -
// cN |o - a|), cN = (6/s + 1.2)u, so a reported t' >= (dist(o) - cN |o - a|) / ((QS + 6u/s) |d|) (1 - 2.01u).
//   camera (G = 0, nu = 0): the rays start at X itself: K = (dist(X) - cN |X - a|) / f, f = 1 + 6u/(s QS);
//   light: the rays start at o with |X - o| <= hi <= G and their lines pass within nu of X, so
//          dist(o) >= dist(X) - QS hi - nu and |o - a| <= |X - a| + G: K = (dist(X) - cN (|X - a| + G)) / f;
//          X lies within H0(|X - a| + G) + QS G + nu of the plane when it is at risk at all.
// slack >= the query's box margin m for those rays.  In double from the record's float edges (the
// products exact, each difference rounded once); the key is rounded down to float (0 when negative).
// A degenerate record (no s2 bound) is always at risk with key 0, one whose stored normal is zero
// never (Mdet = 0: never a hit).
RT_HD float wbvh_risk_key(const GTri& t, double px, double py, double pz, double G, double nu, double slack, double QS)
{
    if (t.n[0] == 0.0f && t.n[1] == 0.0f && t.n[2] == 0.0f)
        return INFINITY;
    const double x0 = t.ab[0], x1 = t.ab[1], x2 = t.ab[2], y0 = t.ac[0], y1 = t.ac[1], y2 = t.ac[2];
    const double c0 = x1 * y2 - x2 * y1, c1 = x2 * y0 - x0 * y2, c2 = x0 * y1 - x1 * y0;
    const double la = sqrt(x0 * x0 + x1 * x1 + x2 * x2), lc = sqrt(y0 * y0 + y1 * y1 + y2 * y2);
    const double cl = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
    if (!(la * lc > 0x1p-100) || !(cl > 0x1p-50 * la * lc))
        return 0.0f;

    const double ca = fabs(x0 * y0 + x1 * y1 + x2 * y2) / (la * lc);
    const double s2 = sqrt(fmax(0.0, (1.0 - fmin(1.0, ca + 1e-12)) / 2.0)) * (1 - 1e-9);
    const double sa = cl / (la * lc) * (1 - 1e-9);
    if (!(s2 > 0.0) || !(sa > 0.0))
        return 0.0f;
    const double ax = px - (double)t.a[0], ay = py - (double)t.a[1], az = pz - (double)t.a[2];
    const double Da = sqrt(ax * ax + ay * ay + az * az);
    const double dist = fabs(c0 * ax + c1 * ay + c2 * az) / cl;
    const double L = fmax(la, lc) * (1 + 1e-12);
    const double sa0 = cl / (la * lc);
    const double Dx = Da + G + slack, u = 0x1p-24;
    const double H0 = 1.01 * (QS * (2 * L + Dx) + u * (24.2 * L + 48 * Dx) / sa0 + u * (30 * L + 12 * Dx + 24 * Dx / sa0) / s2);
    const double rhs = (H0 + QS * G + nu) * (1 + 1e-6);
    if (dist > rhs)
        return INFINITY;
    if (!(dist <= rhs))
        return 0.0f;   // NaN
    const double cN = (6.0 / sa + 1.2) * 0x1p-24 * 1.01;
    const double K = (dist * (1 - 1e-9) - cN * (Da + G + slack)) / (1.0 + 6.0 * 0x1p-24 / (sa * QS)) * (1 - 1e-6);
    if (!(K > 0.0))
        return 0.0f;
    const float f = (float)K;
    return (double)f > K ? nextafterf(f, 0.0f) : f;
}

// Case (a)'s reach (r05, DESIGN.md 5.6 "The correlated bound"): how far a point Moller-Trumbore reports
// (triangle.cpp:25-91) can lie from its triangle T = (a, a + ab, a + ac), and from T's plane.  With u =
// 2^-24, N = ab x ac, s = |N| / (|ab| |ac|), q = cos(N, -d), L >= |ab|, |ac|, D >= |o - x| for every x of T,
// the computed m, Mdet, U = m.ac, V = -m.ab, T = n.OA carry errors dm, eM, eu, ev, eT (|n - N| <= 2.83u
// |ab||ac|, |dm| <= 3.84u |d| |o - a|, |eM| <= 3.01u |n||d|, |eu| <= 3.01u |m||ac|, |ev| <= 3.01u |m||ab|,
// |eT| <= 4.02u |n| |o - a|).  For P' = a + u' ab + v' ac (in T: u', v' were accepted) and p' = o + t' d,
// the identities U ab + V ac = m x N and (o - a) x d = M give
//   Mdet (p' - P') = -(n - N) x M + eM (o - a) + eT d - dm x N - eu ab - ev ac   (+ the final roundings),
// where |M| = |d| h, h = dist(a, line) <= L + |p' - P'|, and Mdet >= |d||N| G, G = q - 3.01u - 2.84u / s.
// So the D terms come with 1 / G only and 1 / s meets only L (the former bound had D / (q s)):
//   E = |p' - P'| <= [8.85u (L + E) / (s G) + 10.87u D / G + 43u^2 D / (s G) + 2.011u (D + E + L)]
// and, by Binet-Cauchy on Mdet (p' - a).N, the distance of p' from T's plane
//   eta <= [2.83u (L + E) / (s G) + (3.01 (D + E) + 4.02 D) u kq + 2.011u (D + E)] / (1 - 3.02u / G - 9u^2 / (s G))
// with kq = (1 + 2.83u / (s G))(1 + 5.85u / (s G)) >= (|n| / |N|)(q / G).  tests/c/wq_lemma.cpp checks both
// on 10^7 accepted hits (largest |p' - P'| / E 0.33, eta ratio 0.47).  Inputs: lower bounds smin <= s, qa
// <= q; G >= qa - 5.85u / smin.  wq_reach: E (INFINITY: no bound); wq_eta: eta.  Float evaluation: every
// constant is rounded up, every step a product or sum of non-negative terms (relative error a few u,
// inside the final 2^-16).
struct WReach {
    float E, isG, iG;   // the reach, >= 1 / (s G), >= 1 / G
};
RT_HD WReach wq_reach(float qa, float smin, float L, float D)
{
    constexpr float U = 0x1p-24f;
    WReach r;
    const float X = __builtin_fmaf(smin, qa, -5.86f * U);   // <= s G (one rounding)
    r.isG = X > 0.0f ? fast_rcp(X) * (1.0f + 0x1p-18f) : INFINITY;
    r.iG = smin * r.isG * (1.0f + 0x1p-20f);
    const float beta = __builtin_fmaf(8.86f * U, r.isG, 2.012f * U);
    // 1 / (1 - beta) <= 1 + 2 beta for beta <= 1/2
    const float num = U * __builtin_fmaf(8.86f, L * r.isG, __builtin_fmaf(10.88f, D * r.iG, __builtin_fmaf(43.1f * U, D * r.isG,
                                                                                                       2.012f * (D + L))));
    r.E = !(beta <= 0.5f) ? INFINITY : num * __builtin_fmaf(2.0f, beta, 1.0f) * (1.0f + 0x1p-16f);
    return r;
}
// The same error split into a lateral part and a part along d: p' - P' = lat + par, par parallel to d.
// Only the terms eT d, the d-component of eM (o - a) (o - a = (P' - a) + (p' - P') - t' d) and the final
// rounding of t' lie along d; so P' + lat, a point of the line, lies within Rlat of T (the line crosses
// the box widened by Rlat) and p' lies within Rpar of it along the line:
//   Rlat <= 8.85u (L + E) / (s G) + 3.01u kn (L + E) / G + 3.84u D / G + 23.2u^2 D / (s G) + 2.012u L,
//   Rpar <= (4.02 D + 3.01 (D + E)) u kn / G + 2.011u (D + E),   kn = 1 + 2.83u / (s G) >= |n| / |N|.
// The D / q term of the lateral reach is 3.84u D / G against 10.87u D / G for E (tests/c/wq_lemma.cpp:
// largest lat / Rlat 0.38).
RT_HD void wq_split(const WReach& r, float L, float D, float& Rlat, float& Rpar)
{
    constexpr float U = 0x1p-24f;
    const float E = r.E;
    const float kn = __builtin_fmaf(2.84f * U, r.isG, 1.0f);
    const float LE = (L + E) * (1.0f + 0x1p-22f);
    Rlat = U * __builtin_fmaf(8.86f * LE, r.isG,
                              __builtin_fmaf(__builtin_fmaf(3.03f * LE, kn, 3.85f * D), r.iG,
                                             __builtin_fmaf(23.3f * U * D, r.isG, 2.013f * L))) * (1.0f + 0x1p-16f);
    Rpar = U * __builtin_fmaf(__builtin_fmaf(4.03f, D, 3.02f * (D + E)) * kn, r.iG, 2.012f * (D + E)) * (1.0f + 0x1p-16f);
}

RT_HD float wq_eta(const WReach& r, float L, float D)
{
    constexpr float U = 0x1p-24f;
    const float E = r.E;
    const float kq = __builtin_fmaf(2.84f * U, r.isG, 1.0f) * __builtin_fmaf(5.86f * U, r.isG, 1.0f);
    const float x = __builtin_fmaf(3.03f * U, r.iG, 9.1f * U * U * r.isG);   // <= 0.17 when E is finite
    const float n2 = U * __builtin_fmaf(2.85f * (L + E), r.isG,
                                        __builtin_fmaf(__builtin_fmaf(3.02f, D + E, 4.03f * D), kq, 2.012f * (D + E)));
    return n2 * __builtin_fmaf(2.0f, x, 1.0f) * (1.0f + 0x1p-16f);
}

// The closed-form reach of a well-conditioned child (W_FAST_REACH, DESIGN.md 5.6 "Closed-form reach"): at
// fixed qa and smin, E, Rlat, Rpar and eta above are linear in (L, D) (E's numerator is, its factor is a
// constant, and the others are linear in L, D and E), and every term falls as qa or smin grows.  So for qa
// >= W_FAST_Q and smin >= W_FAST_S each is at most its value at that corner:
//   E <= u (143.9 L + 45.6 D), Rlat <= u (156.1 L + 15.42 D), Rpar <= u (0.00013 L + 30.25 D),
//   eta <= u (45.65 L + 9.08 D)                                            (W_FAST_Q = W_FAST_S = 1/4),
// the float functions' values at (L, D) = (1, 0) and (0, 1) (143.778, 45.534; 155.898, 15.4008; 0.000121,
// 30.2129; 45.6016, 9.06235) rounded up by 2^-10 or more, which covers the float evaluation of either
// side.  tests/c/wq_fast_bound.cpp compares them with the functions over every smin code from the
// threshold up, every finite L code, qa from W_FAST_Q to 1 and D over 2^-20 .. 2^20.  The child's smin
// byte is compared raw (the code is monotone); qlb, not qa, is compared, so QS plays no part.
// Off by default: with it the plain frame kernel spills 5 VGPRs at its 168 against 2 without.
#ifndef W_FAST_REACH
#define W_FAST_REACH 0
#endif
#define W_FAST_Q 0.25f
#define W_FAST_S 0.25f
// the smallest smin code whose value is >= W_FAST_S (wq_val: an octave per 8 codes, 255 = 1)
constexpr uint32_t W_FAST_S_CODE = ((__builtin_bit_cast(uint32_t, W_FAST_S) - WQ_UNIT) + 0xFFFFFu) >> 20;
static_assert(W_FAST_S_CODE == 239u, "the closed form's constants are those of smin = 1/4");
// e: the child's ext word (smin code in byte 0, L code in byte 3)
RT_HD bool wq_fast_ok(float qlb, uint32_t e)
{
    return W_FAST_REACH && qlb >= W_FAST_Q && (e & 0xffu) >= W_FAST_S_CODE && (e >> 24) != 255u;
}
RT_HD void wq_fast(float L, float D, float& E, float& Rlat, float& Rpar)
{
    const float UL = 0x1p-24f * L, UD = 0x1p-24f * D;
    E = __builtin_fmaf(143.9f, UL, 45.6f * UD);
    Rlat = __builtin_fmaf(156.1f, UL, 15.42f * UD);
    Rpar = __builtin_fmaf(0.00013f, UL, 30.25f * UD);
}
RT_HD float wq_fast_eta(float L, float D)
{
    return __builtin_fmaf(45.65f * 0x1p-24f, L, 9.08f * 0x1p-24f * D);
}

// The scene bound (DESIGN.md 5.6 "The scene bound"): a box such that a camera ray whose LINE misses it
// enters no child of the root, so its query ends after the root step as W_MISS; such a ray is answered
// W_MISS without loading a node (kernels.hip wide_closest).  The box is the union U of the root's non-empty
// children's decoded boxes [origin + q_lo step, origin + q_hi step], widened per axis by W >= every
// widening the root step applies to a child's box for a ray from cam:
//   (a) Rb + dtp |d_axis| <= m + Rlat + Rpar (1 + 2^-16) (wbvh_closest: the box widened by Rb = m + Rlat,
//       then tmin -= dtp, tmax += dtp with dtp = Rpar idl, idl <= (1 + 2^-17) / |d| <= (1 + 2^-16) /
//       |d_axis|), Rlat / Rpar from wq_reach / wq_split at qa = QS: the query's qa = max(qlb, QS) and
//       every term falls as qa grows; D = the query's Dn for cam (a per-child D is smaller);
//   (b) without risk words, the child's box widened by m + rho; with them, its at-risk box widened by m +
//       rho: the octree leaves it covers lie within rho of the child's box (ext2; check_wbvh), and its
//       bytes are rounded outward by less than a step (wrisk_qbox), so it lies within rho + step of the
//       child's box: 2 rho + step + m in all.  Case (b) accepts any t: hence the line test, not the ray's.
// (The root's whole frame [origin, origin + 255 step] would serve as well, but its power-of-two step makes
// it up to twice the scene: from the C4 camera it fills the view, and nothing would be rejected.)
// The slab and the cone only remove children.  The reach functions are the query's own float code (the
// device's reciprocal and square root differ from the host's by 1 ulp); the sum is taken in double, 1/8 m
// and a relative 2^-19 cover the two roundings of each plane's t on either side (each a relative 2^-24
// of |origin - o| + W over |d_axis|, against m = 2^-16 (max|o| + S)), and the planes are rounded outward
// to float.  valid = 0 (nothing is rejected): a child with no finite reach (L code 255, beta > 1/2, X <=
// 0) or rho, a scale outside the query's gate, a non-finite frame, camera or light (wbvh_risk_args then
// marks every child at risk over its whole frame).  scale (tests): the box shrunk about its centre.
struct WSceneBound {
    float lo[3], hi[3];
    int32_t valid;
};

// What the bound needs of a node N and the camera, once per (node, camera): N's frame and steps, the query's
// margin m and its Dn for cam over N's frame (case (a)'s D).  valid = 0: the gates above failed.  Nothing in
// the bound's derivation is particular to the root: a ray from cam that reaches N enters child j only if its
// line crosses j's decoded box widened by W_j(N, cam) (wbvh_child_reach).
struct WBoundCtx {
    float m, D, smax;
    float org[3], st[3];
    int32_t valid;
};

RT_HD WBoundCtx wbvh_bound_ctx(const WNode& N, const float cam[3], bool light_finite, float S)
{
    WBoundCtx C{};
    const float om = fmaxf(fabsf(cam[0]), fmaxf(fabsf(cam[1]), fabsf(cam[2])));
    if (!(om < 0x1p26f) || !(S > 0x1p-20f && S < 0x1p20f) || !light_finite)
        return C;
    C.m = 0x1p-16f * (om + S);   // kernels.hip wide_margin
    C.org[0] = N.ox;
    C.org[1] = N.oy;
    C.org[2] = N.oz;
    float f2 = 0.0f;
    for (int a = 0; a < 3; a++) {
        C.st[a] = __builtin_bit_cast(float, ((N.exps >> (8 * a)) & 0xffu) << 23);
        C.smax = fmaxf(C.smax, C.st[a]);
        const float Da = C.org[a] - cam[a];
        const float f = fmaxf(fabsf(Da), fabsf(__builtin_fmaf(255.0f, C.st[a], Da)));
        f2 = a == 0 ? f * f : f2 + f * f;   // (fx fx + fy fy) + fz fz, as the query's Dn
    }
    const float Dn = sqrtf(f2) * (1.0f + 0x1p-16f) + C.m;
    if (!(Dn < 0x1p28f))
        return C;   // (a NaN or infinite frame as well)
    C.D = Dn * (1.0f + 0x1p-20f);
    C.valid = 1;
    return C;
}

// W_j(N, cam) before the margin terms (+ 1.125 m, relative 2^-19): the larger of case (a)'s Rlat + Rpar (1 +
// 2^-16) at qa = QS and case (b)'s 2 rho + step; < 0: child j has no finite reach or rho
RT_HD double wbvh_child_reach(const WNode& N, int j, const WBoundCtx& C, float QS)
{
    const uint32_t e = N.ext[j];
    if ((e >> 24) == 255u)
        return -1.0;
    const float smin = fmaxf(wq_val_nz(e & 0xffu, WQ_UNIT), W_SMIN_FLOOR);
    const float L = wq_val_nz(e >> 24, WQ_LEN);
    const WReach wr = wq_reach(QS, smin, L, C.D);
    float Rlat, Rpar;
    wq_split(wr, L, C.D, Rlat, Rpar);
    const float rho = wq_len(N.ext2[j] & 0xffu);
    if (!(wr.E < INFINITY) || !(Rlat < INFINITY) || !(Rpar < INFINITY) || !(rho < INFINITY))
        return -1.0;
    return fmax((double)Rlat + (double)Rpar * (1.0 + 0x1p-16), 2.0 * (double)rho + (double)C.smax);
}

inline WSceneBound wbvh_scene_bound(const WNode& root, const float cam[3], const float* light, float S, float QS,
                                    double scale = 1.0)
{
    WSceneBound B{};
    const WBoundCtx C = wbvh_bound_ctx(
        root, cam, !light || (std::isfinite(light[0]) && std::isfinite(light[1]) && std::isfinite(light[2])), S);
    if (!C.valid)
        return B;
    const float m = C.m;
    const float* org = C.org;
    const float* st = C.st;
    double W = 0.0;
    int qlo[3] = {255, 255, 255}, qhi[3] = {0, 0, 0};
    bool any = false;
    for (int j = 0; j < W_WIDTH; j++) {
        if (root.child[j] == W_EMPTY)
            continue;
        any = true;
        const double Wj = wbvh_child_reach(root, j, C, QS);
        if (Wj < 0.0)
            return B;
        W = std::max(W, Wj);
        for (int a = 0; a < 3; a++) {
            qlo[a] = std::min(qlo[a], (int)root.qlo[a][j]);
            qhi[a] = std::max(qhi[a], (int)root.qhi[a][j]);
        }
    }
    if (!any)
        return B;
    W = (W + 1.125 * (double)m) * (1.0 + 0x1p-19);
    for (int a = 0; a < 3; a++) {
        const double l = (double)org[a] + qlo[a] * (double)st[a] - W, h = (double)org[a] + qhi[a] * (double)st[a] + W;
        const double c = 0.5 * (l + h), r = 0.5 * (h - l) * scale;
        const double lo = c - r, hi = c + r;
        if (!(std::fabs(lo) < 0x1p27) || !(std::fabs(hi) < 0x1p27) || !(lo <= hi))
            return B;
        B.lo[a] = (float)lo;
        if ((double)B.lo[a] > lo)
            B.lo[a] = std::nextafter(B.lo[a], -INFINITY);
        B.hi[a] = (float)hi;
        if ((double)B.hi[a] < hi)
            B.hi[a] = std::nextafter(B.hi[a], INFINITY);
    }
    B.valid = 1;
    return B;
}

// The per-ray test: true when the line o + t d misses the box [lo, hi], by the slab arithmetic of
// wbvh_closest's box() (the same reciprocals, DMIN clamp and SL slack; o, lo and hi are finite and below
// 2^27, wbvh_scene_bound).  A direction with a NaN or infinite component, or shorter than 2^-50 (the
// query's idl then exceeds the bound's 1 / |d_axis|), is never rejected.
RT_HD bool scene_bound_rejects(const float lo[3], const float hi[3], v3 o, v3 d)
{
    const float DMIN = 0x1p-100f;
    constexpr float SL = 0x1p-20f;
    const float dd = d.x * d.x + d.y * d.y + d.z * d.z;
    if (!(dd >= 0x1p-100f && dd < INFINITY))
        return false;
    const float ix = 1.0f / (fabsf(d.x) < DMIN ? copysignf(DMIN, d.x) : d.x);
    const float iy = 1.0f / (fabsf(d.y) < DMIN ? copysignf(DMIN, d.y) : d.y);
    const float iz = 1.0f / (fabsf(d.z) < DMIN ? copysignf(DMIN, d.z) : d.z);
    const float x0 = (lo[0] - o.x) * ix, x1 = (hi[0] - o.x) * ix;
    const float y0 = (lo[1] - o.y) * iy, y1 = (hi[1] - o.y) * iy;
    const float z0 = (lo[2] - o.z) * iz, z1 = (hi[2] - o.z) * iz;
    const float tmin = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fminf(z0, z1));
    const float tmax = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1));
    return tmin > __builtin_fmaf(fabsf(tmax), SL, tmax);
}

// ---------------------------------------------------------------------------------
// The tile mask: the scene bound taken a few levels down the tree and applied per 8 x 8
// block of the image, once per camera.
//
// The cut: entries (node << 2 | child slot) such that every root-to-leaf path crosses exactly one.  It
// starts as the root's non-empty children and is expanded level by level: an entry whose child is an
// inner node M is replaced by M's non-empty children when each of them has a finite reach and rho by the
// tree alone (wbvh_cut_child_ok; what the camera adds, Dn's gate and an overflow, is met in
// wbvh_mask_rect: such an entry covers the whole image).  A level is expanded as a whole, and only while
// the cut stays within its budget and the depth limit.
constexpr int W_CUT_MAX = 1 << 16;   // the largest budget (the cut's buffers)
#ifndef W_CUT_BUDGET
#define W_CUT_BUDGET 4096
#endif
#ifndef W_CUT_DEPTH
#define W_CUT_DEPTH 12
#endif

RT_HD bool wbvh_cut_child_ok(const WNode& M, int k, float QS)
{
    const uint32_t e = M.ext[k];
    if ((e >> 24) == 255u || (M.ext2[k] & 0xffu) == 255u)
        return false;
    const float smin = fmaxf(wq_val_nz(e & 0xffu, WQ_UNIT), W_SMIN_FLOOR);
    const WReach wr = wq_reach(QS, smin, wq_val_nz(e >> 24, WQ_LEN), 0.0f);
    return wr.E < INFINITY;
}

// The entries that replace 'entry' in the next level: itself (returns 1, out[0] = entry), or the non-empty
// children of the inner node its child link names (returns their number)
RT_HD int wbvh_cut_expand(const WNode* nodes, int64_t nnodes, uint32_t entry, float QS, uint32_t out[W_WIDTH])
{
    out[0] = entry;
    const uint32_t c = nodes[entry >> 2].child[entry & 3u];
    if ((c & W_LEAF) || (int64_t)c >= nnodes || c >= (1u << 30))
        return 1;   // (a leaf; W_EMPTY has the leaf bit)
    const WNode& M = nodes[c];
    int n = 0;
    uint32_t tmp[W_WIDTH];
    for (int k = 0; k < W_WIDTH; k++) {
        if (M.child[k] == W_EMPTY)
            continue;
        if (!wbvh_cut_child_ok(M, k, QS))
            return 1;
        tmp[n++] = (c << 2) | (uint32_t)k;
    }
    if (n == 0)
        return 1;
    for (int k = 0; k < n; k++)
        out[k] = tmp[k];
    return n;
}

// The cut on the host (the device's: kernels.hip wide_cut_kernel, the same levels, in any order)
inline void wbvh_cut_host(const WNode* nodes, int64_t nnodes, int budget, int max_depth, float QS, std::vector<uint32_t>& cut)
{
    cut.clear();
    if (nnodes <= 0)
        return;
    budget = std::min(budget, W_CUT_MAX);
    for (int j = 0; j < W_WIDTH; j++)
        if (nodes[0].child[j] != W_EMPTY)
            cut.push_back((uint32_t)j);
    std::vector<uint32_t> next;
    for (int depth = 1; depth < max_depth; depth++) {
        next.clear();
        bool grew = false;
        for (uint32_t en : cut) {
            uint32_t out[W_WIDTH];
            const int n = wbvh_cut_expand(nodes, nnodes, en, QS, out);
            grew |= !(n == 1 && out[0] == en);
            next.insert(next.end(), out, out + n);
        }
        if (!grew || (int64_t)next.size() > budget)
            break;
        cut.swap(next);
    }
}

// The camera as the mask sees it.  With KParams::proj_mode != 0 and c2w_affine the direction of pixel (x,
// y) before normalisation (kernels.hip camera_dir) is affine in (x, y): dir = M (x, y, 1).  Minv is M's
// inverse (double), so a point P has (a, b, s) = Minv (P - cam) and lies on the line of pixel (a / s, b /
// s), for s of either sign (the bound's test is the line's).  guard (pixels) covers the float rounding
// of camera_dir against the exact map and the mask's own rounding (wbvh_mask_cam).  scale (tests): each
// cut box shrunk about its centre.  cull: the entry search's back-face test (wbvh_entry_backfacing; 0: off,
// 1: on, 2 (tests, unsound): the block's centre alone).
struct WMaskCam {
    double Minv[9];
    double M[9];
    double guard, scale;
    float cam[3];
    float S, QS;
    int32_t rw, rh;         // the internal image
    int32_t bw, bh, wpr;    // 8 x 8 blocks, 32-bit words per block row: block (bx, by) is bit bx & 31 of word by wpr + (bx >> 5)
    int32_t light_finite;
    int32_t valid;
    int32_t cull;
    int32_t pad;            // (no padding bytes: renderer.cpp prepare_mask compares cameras with memcmp)
};

// valid = 0 (no mask): a general projection or camera matrix, non-finite values, a singular M, or a camera
// whose float rounding the one-pixel guard does not cover.  camera_dir's float evaluation (x_world within
// 3u, each matrix row a sum of four products, the subtraction of cam, the normalisation's division; u =
// 2^-24) puts component r of the direction within 22u T_r of the exact affine map's, T_r the sum of the
// absolute terms of row r of both transforms plus |cam_r| (13u for the maps and the subtraction, u for
// the division, 8u for a direction moved by up to 4 ulps); as a vector E <= 2^-18 max T.  A direction
// d + e maps to Minv d + Minv e = (x, y, 1) + (da, db, ds) with |da| <= |row a| E ..., so the pixel moves by at
// most (|da| + rw |ds|) / (1 - |ds|) <= 2 (|da| + rw |ds|) for |ds| <= 1/2.  The guard is one pixel plus four
// times that bound (the mask's own arithmetic is in double: its rounding is far below); no mask when the
// bound exceeds one pixel.  guard_override (tests): a guard to use instead, may be negative.
inline WMaskCam wbvh_mask_cam(const float proj_inv[16], const float c2w[16], int proj_mode, float proj_w, int c2w_affine,
                              const float cam[3], const float* light, float S, float QS, int rw, int rh,
                              const double* guard_override = nullptr, double scale = 1.0)
{
    WMaskCam C{};
    C.rw = rw;
    C.rh = rh;
    C.bw = (rw + 7) / 8;
    C.bh = (rh + 7) / 8;
    C.wpr = (C.bw + 31) / 32;
    C.S = S;
    C.QS = QS;
    C.scale = scale;
    C.light_finite = !light || (std::isfinite(light[0]) && std::isfinite(light[1]) && std::isfinite(light[2]));
    if (proj_mode == 0 || !c2w_affine || rw <= 0 || rh <= 0 || rw > (1 << 20) || rh > (1 << 20) || !C.light_finite)
        return C;
    const double pw = proj_mode == 1 ? 1.0 : (double)proj_w;
    const double ax = 2.0 / rw, bx = 1.0 / rw - 1.0, ay = 2.0 / rh, by = 1.0 / rh - 1.0;
    double M[9], T = 0.0, Tv[3];
    for (int r = 0; r < 3; r++) {
        const float* p = proj_inv + 4 * r;
        Tv[r] = std::fabs(pw) * (std::fabs((double)p[0]) + std::fabs((double)p[1]) + std::fabs((double)p[2]) + std::fabs((double)p[3]));
    }
    double vs[3][3];   // view-space direction: column of x, of y, constant
    for (int r = 0; r < 3; r++) {
        const float* p = proj_inv + 4 * r;
        vs[r][0] = pw * (double)p[0] * ax;
        vs[r][1] = pw * (double)p[1] * ay;
        vs[r][2] = pw * ((double)p[0] * bx + (double)p[1] * by - (double)p[2] + (double)p[3]);
    }
    for (int r = 0; r < 3; r++) {
        const float* c = c2w + 4 * r;
        double Tw = std::fabs((double)c[3]) + std::fabs((double)cam[r]);
        for (int k = 0; k < 3; k++) {
            Tw += std::fabs((double)c[k]) * Tv[k];
            M[3 * r + k] = (double)c[0] * vs[0][k] + (double)c[1] * vs[1][k] + (double)c[2] * vs[2][k];
        }
        M[3 * r + 2] += (double)c[3] - (double)cam[r];
        T = std::max(T, Tw);
        C.cam[r] = cam[r];
    }
    const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
    const double det = M[0] * c00 + M[1] * c01 + M[2] * c02;
    if (!std::isfinite(det) || !std::isfinite(T) || det == 0.0)
        return C;
    const double id = 1.0 / det;
    C.Minv[0] = c00 * id;
    C.Minv[1] = (M[2] * M[7] - M[1] * M[8]) * id;
    C.Minv[2] = (M[1] * M[5] - M[2] * M[4]) * id;
    C.Minv[3] = c01 * id;
    C.Minv[4] = (M[0] * M[8] - M[2] * M[6]) * id;
    C.Minv[5] = (M[2] * M[3] - M[0] * M[5]) * id;
    C.Minv[6] = c02 * id;
    C.Minv[7] = (M[1] * M[6] - M[0] * M[7]) * id;
    C.Minv[8] = (M[0] * M[4] - M[1] * M[3]) * id;
    double rn[3], res = 0.0;
    for (int r = 0; r < 3; r++) {
        rn[r] = std::sqrt(C.Minv[3 * r] * C.Minv[3 * r] + C.Minv[3 * r + 1] * C.Minv[3 * r + 1] + C.Minv[3 * r + 2] * C.Minv[3 * r + 2]);
        // (the inverse checked against M: a badly conditioned M has no mask)
        for (int k = 0; k < 3; k++) {
            const double x = C.Minv[3 * r] * M[k] + C.Minv[3 * r + 1] * M[3 + k] + C.Minv[3 * r + 2] * M[6 + k];
            res = std::max(res, std::fabs(x - (r == k ? 1.0 : 0.0)));
        }
    }
    const double E = 0x1p-18 * T;
    const double ds = rn[2] * E;
    const double shift = 2.0 * (std::max(rn[0], rn[1]) * E + std::max(rw, rh) * ds);
    if (!(res < 1e-9) || !(ds <= 0.5) || !(shift <= 1.0))
        return C;
    for (int i = 0; i < 9; i++)
        C.M[i] = M[i];
    C.guard = guard_override ? *guard_override : 1.0 + 4.0 * shift;
    C.cull = 1;
    C.valid = 1;
    return C;
}

// KParams::proj_mode / proj_w of an inverse projection, as renderer.cpp fill_params derives them (host tools)
inline void wbvh_proj_shortcut(const float m[16], int& mode, float& w)
{
    mode = 0;
    w = 1.0f;
    bool fin = true;
    for (int i = 0; i < 16; i++)
        fin = fin && std::isfinite(m[i]);
    if (fin && m[12] == 0.0f && m[13] == 0.0f && m[14] != 0.0f) {
        volatile float mz = m[14] * -1.0f;   // (volatile: evaluated as the kernel does, in float)
        const float wt = mz + m[15];
        if (std::isfinite(wt) && wt != 0.0f) {
            mode = wt == 1.0f ? 1 : 2;
            w = 1.0f / wt;
        }
    }
}

// The blocks a cut entry may touch: [x0, x1] x [y0, y1] inclusive (empty: x0 > x1); an entry whose widened
// box has no projection (a corner on either side of, or near, the camera's plane s = 0; no finite W; a
// failed gate) covers every block.
struct WMaskRect {
    int32_t x0, y0, x1, y1;
};

RT_HD WMaskRect wbvh_mask_rect(const WNode& N, int j, const WMaskCam& C)
{
    const WMaskRect all = {0, 0, C.bw - 1, C.bh - 1};
    const WBoundCtx B = wbvh_bound_ctx(N, C.cam, C.light_finite != 0, C.S);
    if (!B.valid)
        return all;
    double W = wbvh_child_reach(N, j, B, C.QS);
    if (W < 0.0)
        return all;
    W = (W + 1.125 * (double)B.m) * (1.0 + 0x1p-19);
    double lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        const double l = (double)B.org[a] + (double)N.qlo[a][j] * (double)B.st[a] - W;
        const double h = (double)B.org[a] + (double)N.qhi[a][j] * (double)B.st[a] + W;
        const double c = 0.5 * (l + h), r = 0.5 * (h - l) * C.scale;
        lo[a] = c - r - (double)C.cam[a];
        hi[a] = c + r - (double)C.cam[a];
        if (!(fabs(lo[a]) < 0x1p27) || !(fabs(hi[a]) < 0x1p27) || !(lo[a] <= hi[a]))
            return all;
    }
    double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY, smin = INFINITY, smax = -INFINITY;
    for (int c = 0; c < 8; c++) {
        const double px = (c & 1) ? hi[0] : lo[0], py = (c & 2) ? hi[1] : lo[1], pz = (c & 4) ? hi[2] : lo[2];
        const double a = C.Minv[0] * px + C.Minv[1] * py + C.Minv[2] * pz;
        const double b = C.Minv[3] * px + C.Minv[4] * py + C.Minv[5] * pz;
        const double s = C.Minv[6] * px + C.Minv[7] * py + C.Minv[8] * pz;
        smin = fmin(smin, s);
        smax = fmax(smax, s);
        const double x = a / s, y = b / s;
        xmin = fmin(xmin, x);
        xmax = fmax(xmax, x);
        ymin = fmin(ymin, y);
        ymax = fmax(ymax, y);
    }
    // every s of one sign and clear of zero (s is linear: it then keeps that sign over the whole box, whose
    // projection is the convex hull of the corners')
    const double sa = fmax(fabs(smin), fabs(smax));
    if (!(smin * smax > 0.0) || !(fmin(fabs(smin), fabs(smax)) > 0x1p-20 * sa) || !(sa < INFINITY))
        return all;
    xmin -= C.guard;
    xmax += C.guard;
    ymin -= C.guard;
    ymax += C.guard;
    if (!(xmin <= xmax) || !(ymin <= ymax))
        return WMaskRect{1, 1, 0, 0};   // (a negative guard, tests; NaN cannot occur: every s is clear of zero)
    if (xmax < 0.0 || ymax < 0.0 || xmin > (double)(C.rw - 1) || ymin > (double)(C.rh - 1))
        return WMaskRect{1, 1, 0, 0};
    WMaskRect R;
    R.x0 = (int32_t)floor(fmax(xmin, 0.0)) >> 3;
    R.y0 = (int32_t)floor(fmax(ymin, 0.0)) >> 3;
    R.x1 = (int32_t)ceil(fmin(xmax, (double)(C.rw - 1))) >> 3;
    R.y1 = (int32_t)ceil(fmin(ymax, (double)(C.rh - 1))) >> 3;
    return R;
}

// A cut entry's blocks: a ray that reaches the entry's node N has entered N at its parent, and the parent at
// its own, so its pixel lies in every ancestor entry's rectangle as well: the intersection along the chain
// (parent: WBvh::parent, node -> its parent's entry, W_EMPTY for the root; nullptr: the entry's own
// rectangle).  A deep child's W may exceed its ancestors' (its rho is that of the octree leaves it shares
// with its siblings), so the chain is what makes a finer cut never worse than a coarser one.
RT_HD WMaskRect wbvh_mask_entry(const WNode* nodes, int64_t nnodes, const uint32_t* parent, uint32_t entry, const WMaskCam& C)
{
    WMaskRect R = wbvh_mask_rect(nodes[entry >> 2], (int)(entry & 3u), C);
    uint32_t n = entry >> 2;
    for (int up = 0; parent && up < 64 && R.x0 <= R.x1 && R.y0 <= R.y1; up++) {
        const uint32_t p = parent[n];
        if (p == W_EMPTY || (int64_t)(p >> 2) >= nnodes)
            break;
        const WMaskRect Q = wbvh_mask_rect(nodes[p >> 2], (int)(p & 3u), C);
        R.x0 = R.x0 > Q.x0 ? R.x0 : Q.x0;
        R.y0 = R.y0 > Q.y0 ? R.y0 : Q.y0;
        R.x1 = R.x1 < Q.x1 ? R.x1 : Q.x1;
        R.y1 = R.y1 < Q.y1 ? R.y1 : Q.y1;
        n = p >> 2;
    }
    if (R.x0 > R.x1 || R.y0 > R.y1)
        return WMaskRect{1, 1, 0, 0};
    return R;
}

// The bits of rect R in word w of a block row (wbvh_mask_rect's layout)
RT_HD uint32_t wbvh_mask_word(const WMaskRect& R, int w)
{
    const int b0 = R.x0 - 32 * w, b1 = R.x1 - 32 * w;
    if (b1 < 0 || b0 > 31)
        return 0u;
    const uint32_t lo = b0 <= 0 ? 0xFFFFFFFFu : 0xFFFFFFFFu << b0;
    const uint32_t hi = b1 >= 31 ? 0xFFFFFFFFu : 0xFFFFFFFFu >> (31 - b1);
    return lo & hi;
}

// The mask on the host (the device's: kernels.hip wide_mask_kernel): words[bh wpr], a set bit = the block
// may hold a ray that enters the cut
inline void wbvh_mask_host(const WNode* nodes, int64_t nnodes, const uint32_t* parent, const std::vector<uint32_t>& cut,
                           const WMaskCam& C, std::vector<uint32_t>& words)
{
    words.assign((size_t)C.bh * C.wpr, 0u);
    for (uint32_t en : cut) {
        const WMaskRect R = wbvh_mask_entry(nodes, nnodes, parent, en, C);
        for (int y = R.y0; y <= R.y1 && R.x0 <= R.x1; y++)
            for (int w = R.x0 >> 5; w <= R.x1 >> 5; w++)
                words[(size_t)y * C.wpr + w] |= wbvh_mask_word(R, w);
    }
}

// ---------------------------------------------------------------------------------
// Entry nodes: where the camera rays of an 8 x 8 block can go, found once per camera.  A
// camera ray enters child j of node N only if its pixel lies in wbvh_mask_rect(N, j, C) (5.12), so the rays
// of block b that reach N go on into c(N) = the non-empty children whose rectangle holds b and that do not
// face away from every ray of b (wbvh_entry_backfacing), and nowhere else.
// Top-down from the root, a frontier node N is replaced by the child nodes of c(N) while every member of
// c(N) is an inner node (no triangle is ever tested above the frontier), |c(N)| <= fan, the frontier stays
// within K nodes and below max_depth; a node with an empty c(N) is dropped.  The block's primary queries
// start at the frontier's nodes instead of the root (wbvh_closest's start set).  The links are ordered by the
// distance of the node's frame from the camera, nearest first (the order does not change the answer: the
// near subtree sets the best hit before the far one is visited); unused slots hold W_EMPTY; an empty result
// is stored as the root {0, W_EMPTY, ...}.
constexpr int W_ENTRY_MAX = 4;   // links per block (one uint4)
#ifndef W_ENTRY_K
#define W_ENTRY_K 4
#endif
#ifndef W_ENTRY_FAN
// (tools/visit_probe.py, profiles/entry_cull/host_probe_*.log: with the back-face test K 4, fan 4 saves the most on
// sphere1m, hair1m and robot1080)
#define W_ENTRY_FAN 4
#endif
// the fan of the search without the back-face test (RT_ENTRY_CULL=0: the sets as they were before it, for A/B runs;
// profiles/entry_nodes/host_probe.log: fan 3 saved the most there)
constexpr int W_ENTRY_FAN_UNCULLED = 3;
inline int wbvh_entry_fan(const WMaskCam& C)   // the renderer's fan for camera C
{
    return C.cull ? W_ENTRY_FAN : W_ENTRY_FAN_UNCULLED;
}

struct WEntrySet {
    uint32_t link[W_ENTRY_MAX];
};

RT_HD bool wbvh_rect_holds(const WMaskRect& R, int bx, int by)
{
    return bx >= R.x0 && bx <= R.x1 && by >= R.y0 && by <= R.y1;
}

// squared distance of cam from node N's frame [origin, origin + 255 step] (the links' order)
RT_HD double wbvh_entry_dist(const WNode& N, const float cam[3])
{
    const double org[3] = {N.ox, N.oy, N.oz};
    double s = 0.0;
    for (int a = 0; a < 3; a++) {
        const double st = (double)__builtin_bit_cast(float, ((N.exps >> (8 * a)) & 0xffu) << 23);
        const double lo = org[a], hi = org[a] + 255.0 * st, c = (double)cam[a];
        const double g = c < lo ? lo - c : (c > hi ? c - hi : 0.0);
        s += g * g;
    }
    return s == s ? s : INFINITY;
}

// The block's back-face test (C.cull): child j of N is dropped from c(N) when every camera ray of block (bx, by)
// skips it at N by wbvh_closest's cone test, a > c cstep in float (WNode: every triangle below j faces away
// from such a ray).  A pixel's direction before normalisation is d = M (x, y, 1), and camera_dir's float
// direction is a positive multiple of M (x', y', 1) with (x', y') within C.guard of the pixel (wbvh_mask_cam: the
// third coordinate stays above 1/2).  f(d) = N_j . d - k |d| with k >= 0 is concave and positively homogeneous, so
// over the rays of the rectangle [8 bx - guard, 8 bx + 7 + guard] x [8 by - guard, 8 by + 7 + guard] it is
// smallest at one of the four corners: f > 0 there gives f > 0 for every float direction of the block.  The
// margin in k = c W_CONE_STEP (1 + 2^-12) + 2^-10 makes that imply the ray's own float decision: its a is
// a sum of three float products, within 3 u |N_j| |d| <= 3 2^-24 220 |d| < 4e-5 |d| of N_j . d; its threshold
// c cstep is at most c W_CONE_STEP |d| (1 + 2^-20)(1 + 2^-22)(1 + u)^3 <= c W_CONE_STEP |d| (1 + 2^-18) (setup:
// the square root and the dot within 2^-22, rounded up by 2^-20, two more products).  2^-10 is 25 times the
// first, 2^-12 sixty-four times the second, and together they cost at most 0.056 of a code's step of 0.88.
// Evaluated in double without a square root or a division (a > 0 and a^2 > k^2 |d|^2; double's rounding,
// 1e-15 relative, is far inside the margin), so the host and the device decide alike.  Code 255: no cone.
constexpr double W_CULL_REL = 0x1p-12, W_CULL_ABS = 0x1p-10;

RT_HD bool wbvh_entry_backfacing(const WNode& N, int j, const WMaskCam& C, int bx, int by)
{
    const uint32_t nr = N.nrm[j];
    if (C.cull == 0 || (nr >> 24) == 255u)
        return false;
    const double n[3] = {(double)(int8_t)(nr & 0xffu), (double)(int8_t)((nr >> 8) & 0xffu), (double)(int8_t)((nr >> 16) & 0xffu)};
    const double k = (double)(nr >> 24) * (double)W_CONE_STEP * (1.0 + W_CULL_REL) + W_CULL_ABS;
    const double x0 = 8.0 * bx - C.guard, x1 = 8.0 * bx + 7.0 + C.guard;
    const double y0 = 8.0 * by - C.guard, y1 = 8.0 * by + 7.0 + C.guard;
    const int corners = C.cull == 2 ? 1 : 4;
    for (int q = 0; q < corners; q++) {
        const double x = C.cull == 2 ? 0.5 * (x0 + x1) : ((q & 1) ? x1 : x0);
        const double y = C.cull == 2 ? 0.5 * (y0 + y1) : ((q & 2) ? y1 : y0);
        const double dx = C.M[0] * x + C.M[1] * y + C.M[2];
        const double dy = C.M[3] * x + C.M[4] * y + C.M[5];
        const double dz = C.M[6] * x + C.M[7] * y + C.M[8];
        const double a = n[0] * dx + n[1] * dy + n[2] * dz;
        if (!(a > 0.0 && a * a > k * k * (dx * dx + dy * dy + dz * dz)))
            return false;
    }
    return true;
}

// c(N) for block (bx, by): the non-empty children of N that face some ray of the block (the four dot products
// first: they are cheaper than the rectangle's sixteen divisions) and whose rectangle holds it.  inner: every
// one of them is an inner node of the tree
RT_HD int wbvh_entry_cover(const WNode& N, int64_t nnodes, const WMaskCam& C, int bx, int by, uint32_t ch[W_WIDTH], bool& inner)
{
    int cnt = 0;
    inner = true;
    for (int j = 0; j < W_WIDTH; j++) {
        const uint32_t c = N.child[j];
        if (c == W_EMPTY || wbvh_entry_backfacing(N, j, C, bx, by) || !wbvh_rect_holds(wbvh_mask_rect(N, j, C), bx, by))
            continue;
        inner = inner && !(c & W_LEAF) && (int64_t)c < nnodes;
        ch[cnt++] = c;
    }
    return cnt;
}

RT_HD WEntrySet wbvh_entry_block(const WNode* nodes, int64_t nnodes, const WMaskCam& C, int bx, int by, int K, int fan,
                                 int max_depth)
{
    WEntrySet S;
    for (int i = 0; i < W_ENTRY_MAX; i++)
        S.link[i] = W_EMPTY;
    S.link[0] = 0u;
    if (nnodes <= 0 || !C.valid)
        return S;
    K = K < 1 ? 1 : (K > W_ENTRY_MAX ? W_ENTRY_MAX : K);
    uint32_t fn[W_ENTRY_MAX];
    int fd[W_ENTRY_MAX];
    bool fin[W_ENTRY_MAX];
    int n = 1;
    fn[0] = 0u;
    fd[0] = 0;
    fin[0] = false;
    for (;;) {
        // the shallowest node still open (the first of them): the budget goes to the levels in turn
        int i = n;
        for (int k = 0; k < n; k++)
            if (!fin[k] && (i == n || fd[k] < fd[i]))
                i = k;
        if (i == n)
            break;
        const WNode& N = nodes[fn[i]];
        uint32_t ch[W_WIDTH];
        bool inner;
        const int cnt = wbvh_entry_cover(N, nnodes, C, bx, by, ch, inner);
        if (cnt == 0) {   // no ray of the block goes below N
            for (int k = i + 1; k < n; k++) {
                fn[k - 1] = fn[k];
                fd[k - 1] = fd[k];
                fin[k - 1] = fin[k];
            }
            n--;
            continue;
        }
        if (!inner || cnt > fan || n - 1 + cnt > K || fd[i] + 1 >= max_depth) {
            fin[i] = true;
            continue;
        }
        fn[i] = ch[0];
        fd[i]++;
        for (int k = 1; k < cnt; k++) {
            fn[n] = ch[k];
            fd[n] = fd[i];
            fin[n] = false;
            n++;
        }
    }
    if (n == 0)
        return S;   // (the root: its query ends after one step)
    double key[W_ENTRY_MAX];
    for (int i = 0; i < n; i++)
        key[i] = wbvh_entry_dist(nodes[fn[i]], C.cam);
    for (int i = 1; i < n; i++)   // nearest first; equal distances by node index
        for (int k = i; k > 0 && (key[k] < key[k - 1] || (key[k] == key[k - 1] && fn[k] < fn[k - 1])); k--) {
            const double tk = key[k];
            key[k] = key[k - 1];
            key[k - 1] = tk;
            const uint32_t tf = fn[k];
            fn[k] = fn[k - 1];
            fn[k - 1] = tf;
        }
    for (int i = 0; i < n; i++)
        S.link[i] = fn[i];
    return S;
}

// The entry sets on the host (the device's: kernels.hip wide_entry_kernel): W_ENTRY_MAX words per block,
// row-major over the mask's block grid; a block whose mask bit is clear (words: wbvh_mask_host's; nullptr:
// every block is covered) keeps the root
inline void wbvh_entry_host(const WNode* nodes, int64_t nnodes, const WMaskCam& C, const uint32_t* words, int K, int fan,
                            int max_depth, std::vector<uint32_t>& out)
{
    out.assign((size_t)C.bw * C.bh * W_ENTRY_MAX, W_EMPTY);
    for (int by = 0; by < C.bh; by++)
        for (int bx = 0; bx < C.bw; bx++) {
            uint32_t* o = &out[((size_t)by * C.bw + bx) * W_ENTRY_MAX];
            o[0] = 0u;
            if (words && !((words[(size_t)by * C.wpr + (bx >> 5)] >> (bx & 31)) & 1u))
                continue;
            const WEntrySet S = wbvh_entry_block(nodes, nnodes, C, bx, by, K, fan, max_depth);
            for (int i = 0; i < W_ENTRY_MAX; i++)
                o[i] = S.link[i];
        }
}

// A frame's two risk points (kernels.hip wide_risk_kernel): sel 0 the camera (rays start at it), sel
// 1 the light (shadow rays: o = p + 1e-4 n, d = normalize(light - p), renderer.cpp:340-402, for hit
// points p in the scene box [lo, hi]).  The shadow rays that may use the light's keys are the ones
// whose segment bound hi (kernels.hip is_shadowed, >= |light - o|) is <= ray_G and whose normal has
// |n|_1 <= ray_nl: their lines pass within nu = 1.001e-4 ray_nl + 16u G of the light (the offset
// and normalize's rounding; ray_nu: nu rounded up).  slack >= the query's margin m for the kind's
// origins.
struct WRiskArgs {
    double p[2][3];
    double G[2], nu[2], slack[2], QS[2];
    int32_t on[2];
    float ray_G, ray_nl, ray_nu;
};

inline WRiskArgs wbvh_risk_args(const float lo[3], const float hi[3], float S, const float cam[3], const float light[3],
                                float qs_cam, float qs_light)
{
    WRiskArgs A{};
    double cm = 0, lm = 0, gc = 0;
    for (int a = 0; a < 3; a++) {
        A.p[0][a] = cam[a];
        A.p[1][a] = light[a];
        cm = std::max(cm, std::fabs((double)cam[a]));
        lm = std::max(lm, std::fabs((double)light[a]));
    }
    for (int c = 0; c < 8; c++) {
        double g = 0;
        for (int a = 0; a < 3; a++) {
            const double x = ((c >> a) & 1) ? hi[a] : lo[a];
            g += (x - light[a]) * (x - light[a]);
        }
        gc = std::max(gc, std::sqrt(g));
    }
    A.ray_nl = 2.0f;
    const double G = 1.01 * (gc + 1e-4 * A.ray_nl) + 0x1p-10 * (S + lm);
    A.ray_G = std::nextafter((float)G, 0.0f);
    A.G[0] = 0.0;
    A.nu[0] = 0.0;
    A.slack[0] = 1.01 * 0x1p-16 * (cm + S);
    A.QS[0] = qs_cam;
    A.G[1] = G;
    A.nu[1] = 1.001e-4 * A.ray_nl + 16.0 * 0x1p-24 * G;
    A.ray_nu = std::nextafter((float)(A.nu[1] * (1 + 1e-6)), INFINITY);
    A.slack[1] = 1.01 * 0x1p-16 * (lm + G + S);
    A.QS[1] = qs_light;
    const bool fin = std::isfinite(cm) && std::isfinite(lm) && std::isfinite(G);
    A.on[0] = A.on[1] = fin ? 1 : 0;
    return A;
}

// The risk cap of a frame's point X (camera or light): s <= |cos(N, c)| for the exact normal N of every
// triangle at risk for X's rays (wbvh_risk_key < INFINITY), c a unit direction (from X towards the scene).
// A ray of X's kind at angle g to the line of c has, for each of them, |cos(N, d)| >= s cos g - sqrt(1 -
// s^2) sin g (N = a c + b e with |a| >= s, e normal to c): when that is >= QS (plus a margin over the float
// evaluation) none of them is in case (b) for the ray, and the others cannot report there (their key is
// INFINITY), so the query skips case (b).  For a convex object seen from X the at-risk triangles are its
// silhouette, whose normals are all at 90 degrees + the silhouette's angle from the direction to its
// centre: every ray into the silhouette's interior skips.
RT_HD bool risk_cap_skip(float s, const float c[3], v3 d, float QS)
{
    const float dl = sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
    const float cg = fabsf(c[0] * d.x + c[1] * d.y + c[2] * d.z) / dl;
    const float x = c[1] * d.z - c[2] * d.y, y = c[2] * d.x - c[0] * d.z, z = c[0] * d.y - c[1] * d.x;
    const float sg = sqrtf(x * x + y * y + z * z) / dl;
    return s * cg - sqrtf(fmaxf(0.0f, 1.0f - s * s)) * sg >= QS + 0x1p-14f;
}
// A triangle's lower bound on |cos(N, c)| (risk_cap_skip), in double from the record's float edges; 0 for
// a degenerate record (no normal: it counts as at risk for every ray)
RT_HD float risk_cap_tri(const GTri& t, const double c[3])
{
    const double x0 = t.ab[0], x1 = t.ab[1], x2 = t.ab[2], y0 = t.ac[0], y1 = t.ac[1], y2 = t.ac[2];
    const double c0 = x1 * y2 - x2 * y1, c1 = x2 * y0 - x0 * y2, c2 = x0 * y1 - x1 * y0;
    const double la = sqrt(x0 * x0 + x1 * x1 + x2 * x2), lc = sqrt(y0 * y0 + y1 * y1 + y2 * y2);
    const double cl = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
    if (!(la * lc > 0x1p-100) || !(cl > 0x1p-50 * la * lc) || !(cl < INFINITY))
        return 0.0f;
    const double v = fabs(c0 * c[0] + c1 * c[1] + c2 * c[2]) / cl - 1e-9;
    if (!(v > 0.0))
        return 0.0f;
    const float f = (float)v;
    return (double)f > v ? nextafterf(f, 0.0f) : f;
}

// rsub of wbvh_closest for a shadow ray with |light - o| <= h (rounded up)
RT_HD float wrisk_sub(float QS, float h, float nu)
{
    return __builtin_fmaf(QS, h, nu) * (1.0f + 0x1p-20f);
}

// The per-point risk words of the wide BVH, one 64-bit word per child (risk[(2 node + sel) 4 + j]):
// bits 0-47 = the box of the octree leaves holding its at-risk triangles (the reference tests such a
// triangle only where the line crosses its leaf's k-DOP, inside that box), quantised like the child
// boxes against the node's frame (6 bytes: lo x y z, hi x y z; lo rounded down, hi up, clamped to the
// frame: the box lies within rho of the child's, so the decoded box widened by rho holds it), bits
// 48-63 = the smallest key (wbvh_risk_key) of them as a bfloat16 rounded down (INFINITY: none at risk).
RT_HD uint64_t wrisk_pack(float K, uint64_t box48)
{
    return ((uint64_t)(fbits(K) >> 16) << 48) | (box48 & 0xFFFFFFFFFFFFull);
}
RT_HD float wrisk_key(uint64_t w)
{
    return bitsf((uint32_t)(w >> 48) << 16);
}
// the 6 bytes of a float box [lo, hi] against a node's frame (origin, power-of-two steps)
RT_HD uint64_t wrisk_qbox(const WNode& nd, const float lo[3], const float hi[3])
{
    const double org[3] = {nd.ox, nd.oy, nd.oz};
    uint64_t q = 0;
    for (int a = 0; a < 3; a++) {
        const double st = ldexp(1.0, (int)((nd.exps >> (8 * a)) & 0xffu) - 127);
        const double l = floor(((double)lo[a] - org[a]) / st), h = ceil(((double)hi[a] - org[a]) / st);
        const uint64_t ql = (uint64_t)fmin(255.0, fmax(0.0, l)), qh = (uint64_t)fmin(255.0, fmax(0.0, h));
        q |= ql << (8 * a);
        q |= qh << (8 * (a + 3));
    }
    return q;
}

// Host version of kernels.hip wide_risk_kernel (tests, rt_wbvh_query_ex): a triangle's key and its
// octree leaf's axis box go up its leaf entry's parent chain (minimum, union), stopping where both are
// already there (aggregates over subtrees: what an entry holds its ancestors hold too).  leaf_box:
// per wide-BVH triangle, its octree leaf's axis box (lo xyz, hi xyz).
inline void wbvh_risk_host(const WBvh& w, const std::vector<float>& leaf_box, const WRiskArgs& A, int sel,
                           std::vector<uint64_t>& risk)
{
    risk.resize(w.nodes.size() * 8, wrisk_pack(INFINITY, 0));
    const size_t ne = w.nodes.size() * 4;
    std::vector<float> K(ne, INFINITY), B(ne * 6);
    for (size_t i = 0; i < ne; i++)
        for (int a = 0; a < 3; a++) {
            B[6 * i + a] = INFINITY;
            B[6 * i + 3 + a] = -INFINITY;
        }
    if (!A.on[sel]) {   // no bound: every child at risk, key 0, its whole frame
        for (size_t v = 0; v < w.nodes.size(); v++)
            for (int j = 0; j < 4; j++)
                risk[(2 * v + sel) * 4 + j] = wrisk_pack(0.0f, 0xFFFFFF000000ull);
        return;
    }
    for (size_t k = 0; k < w.tris.size(); k++) {
        const float Kt = wbvh_risk_key(w.tris[k], A.p[sel][0], A.p[sel][1], A.p[sel][2], A.G[sel], A.nu[sel],
                                       A.slack[sel], A.QS[sel]);
        if (!(Kt < INFINITY))
            continue;
        const float* lb = &leaf_box[6 * k];
        uint32_t e = w.tri_leaf[k];
        while (e != W_EMPTY) {
            const size_t i = (size_t)(e >> 2) * 4 + (e & 3u);
            float* b = &B[6 * i];
            const bool has = K[i] <= Kt && b[0] <= lb[0] && b[1] <= lb[1] && b[2] <= lb[2] && b[3] >= lb[3] &&
                             b[4] >= lb[4] && b[5] >= lb[5];
            if (has)
                break;
            K[i] = std::min(K[i], Kt);
            for (int a = 0; a < 3; a++) {
                b[a] = std::min(b[a], lb[a]);
                b[3 + a] = std::max(b[3 + a], lb[3 + a]);
            }
            e = w.parent[e >> 2];
        }
    }
    for (size_t v = 0; v < w.nodes.size(); v++)
        for (int j = 0; j < 4; j++) {
            const size_t i = v * 4 + j;
            risk[(2 * v + sel) * 4 + j] = K[i] < INFINITY ? wrisk_pack(K[i], wrisk_qbox(w.nodes[v], &B[6 * i], &B[6 * i + 3]))
                                                          : wrisk_pack(INFINITY, 0);
        }
}

// Checks a frame's risk words of point sel (host or GPU-computed) against the tree (CPU tests,
// rt_risk_words): for every triangle with a finite key (wbvh_risk_key), every entry on its leaf's
// parent chain must hold a key <= it and an at-risk box that, widened by the entry's rho, holds the
// triangle's octree leaf (what wbvh_closest's case (b) relies on).  Returns the number of violations.
int64_t check_risk_words(const FlatOctree& oct, const WBvh& w, const WRiskArgs& A, int sel, const uint64_t* risk);

// W_DEEP: not certified only because the stack overflowed (callers may retry with a deeper stack)
// W_LONG: stopped after max_steps loop iterations (the caller defers the query to a later pass)
enum WStatus : int { W_MISS = 0, W_HIT = 1, W_UNCERT = 2, W_DEEP = 3, W_LONG = 4 };
constexpr int W_DEEP_STACK = 64;   // the retry's stack (private memory, kernels.hip wide_closest_deep)

struct WHit {
    float t, u, v;
    int32_t k;   // wide-BVH triangle index (W_HIT)
};

// A lane's traversal stack: entry (child link, entry t); CAP entries.
template <int N>
struct WStackArr {
    static constexpr int CAP = N;
    uint2 e[N];
    RT_HD void put(int i, uint2 v) { e[i] = v; }
    RT_HD uint2 get(int i) const { return e[i]; }
};
using WStackLocal = WStackArr<W_STACK>;   // host

// A lane group: G adjacent lanes of a wave (lanes g0 .. g0 + G - 1, g0 a multiple of G) trace one ray
// together (wbvh_closest<Stack, G>, kernels.hip trace_split_part and refl_trace_long_kernel).  Device only; on the host
// (G = 1) these are the identity.
template <int G>
RT_HD uint32_t wg_lane()
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __lane_id() & (uint32_t)(G - 1);
#else
    return 0u;
#endif
}
// the group's lanes where p holds (bit i: group lane i)
template <int G>
RT_HD uint32_t wg_bits(bool p)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)(__ballot(p) >> (__lane_id() & ~(uint32_t)(G - 1))) & ((1u << G) - 1u);
#else
    return p ? 1u : 0u;
#endif
}
#if defined(__HIP_DEVICE_COMPILE__)
// a 32-bit value from the lane the DPP quad permutation names (within each group of 4 lanes; all active)
template <int PERM>
__device__ __forceinline__ uint32_t wg_quad(uint32_t x)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, PERM, 0xF, 0xF, false);
}
#endif
template <int G>
RT_HD float wg_min(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (G <= 4) {   // DPP quad permutations (lane ^ 1, lane ^ 2), no LDS round trip
        x = fminf(x, __uint_as_float(wg_quad<0xB1>(__float_as_uint(x))));
        if (G == 4)
            x = fminf(x, __uint_as_float(wg_quad<0x4E>(__float_as_uint(x))));
    } else {
        for (int m = 1; m < G; m <<= 1)
            x = fminf(x, __shfl_xor(x, m));
    }
#endif
    return x;
}
// x of group lane i (i may differ per lane)
template <int G, class T>
RT_HD T wg_read(T x, int i)
{
    static_assert(sizeof(T) == 4, "32-bit values");
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (G <= 4) {   // the group's G values by DPP quad broadcasts, then a select
        uint32_t u;
        __builtin_memcpy(&u, &x, 4);
        uint32_t r;
        if (G == 4) {   // quad lane 0 / 1 / 2 / 3 to every lane of the quad
            const uint32_t b0 = wg_quad<0x00>(u), b1 = wg_quad<0x55>(u), b2 = wg_quad<0xAA>(u), b3 = wg_quad<0xFF>(u);
            r = i == 0 ? b0 : i == 1 ? b1 : i == 2 ? b2 : b3;
        } else {        // pairs: (0, 0, 2, 2) and (1, 1, 3, 3)
            const uint32_t b0 = wg_quad<0xA0>(u), b1 = wg_quad<0xF5>(u);
            r = i == 0 ? b0 : b1;
        }
        T y;
        __builtin_memcpy(&y, &r, 4);
        return y;
    } else {
        return __shfl(x, (int)(__lane_id() & ~(uint32_t)(G - 1)) + i);
    }
#else
    (void)i;
    return x;
#endif
}

// Closest hit over the wide BVH for the ray (o, d) among hits with t <= hi.  m: box margin
// (2^-16 (max|o| + scene scale), the leaf-slab margin of kernels.hip leaf_missed).
// Returns W_MISS (no triangle reports a hit at t <= hi), W_HIT (h = the minimum-t hit, finite
// and > 0, unique when ties: still to be certified by kdop_certifies on its octree leaf) or
// W_UNCERT (W_DEEP when only the stack overflowed).  Shadow queries (hi = the segment end of kernels.hip is_shadowed, ties false) read
// only the record's t.  work (optional, 4 entries): {nodes, triangles} added, [2] = the reasons
// a query is not certified, [3] = loop iterations added.
//
// The query is sound for every ray: a child is skipped only when no triangle
// below it can REPORT a hit (Moller-Trumbore's rounded t, u, v; triangle.cpp:25-91) that the
// reference could record at t <= the best hit so far.  With q = |cos(n, d)| of a triangle, s =
// sin(alpha), u = 2^-24 and D >= |o - a| (the node frame's farthest corner):
//   (a) every reported point p' lies within R = wq_reach's E of its triangle (r05: D / q and L / (q s)
//       terms, L the longest edge) and within eta (wq_eta) of its plane,
//       which is tilted by theta from the child's slab normal: the child's box widened by R and
//       its slab widened by eta + R sin(theta) hold p' (q is bounded below by the cone: q >=
//       cos(phi) - sin(theta) (1 + sin(theta)), phi the angle between N and -d);
//   (b) for the triangles with q < QS that bound is not used: their reported points can lie
//       anywhere on their plane, but the origin is then within H0 (wq_h0) of
//       that plane (the barycentric numerators must be small), and the reference tests such a
//       triangle only where the line crosses its octree leaf's k-DOP (inside the child box
//       widened by rho).  A child passing both is entered, keyed by its risk key's t bound (0
//       without risk keys).
// Robustly back-facing children (the cone) report nothing and are skipped as before.
// nob: no triangle with q < QS can report a hit for this ray (ocone.hpp ocone_skip, the origin cones),
// so case (b) is skipped (with or without risk words).  Such a ray reads no risk word: LAZY (compile time, with
// W_NOB_FAST; the frame kernels' queries, kernels.hip wide_run) loads them only on the lanes with risk keys and !nob
// (the others take zeros, which no path of theirs reads); without LAZY every lane with risk keys loads them.
// NOB (compile time): the caller promises that nob is true on every lane.  The instance is the same text
// without the risk words, rkj / kbl, both case (b) branches, their ext2 word, dchild and wq_h0: with nob true
// the general instance enters neither branch and reads rw[] nowhere else, so the two take the same decisions,
// keys, order and answers, and count the same work, visit for visit (tests/c/nob_instance_check.cpp).
// risk (optional): the risk words of the ray's kind rsel (wrisk_pack / wbvh_risk_host / kernels.hip
// wide_risk_kernel): a child whose key is INFINITY holds no triangle that can report a hit in case (b)
// for this ray; its (b) triangles lie in octree leaves inside its at-risk box (so the line must cross
// that box, widened by rho), and none of their reports has t' below (key - rsub) / (QS |d|), so (b) is
// skipped for it when that exceeds the best hit.  rsub: 0 for the camera (rsel 0); for the light (rsel 1), at least
// QS h + nu with h >= |light - o| and nu the frame's (WRiskArgs::ray_nu; wrisk_sub).  The caller
// guarantees the ray is of that kind.
//
// G > 1 (device, Stack = kernels.hip WStackLds, max_steps 0): the G lanes of a lane group (wg_lane)
// hold the same ray and walk its tree together.  Group lane 0 starts at the root, the others idle; after
// every step the group shares its best hit bound (best_s, the minimum over the group), and each idle lane
// takes the bottom entry of a busy lane's stack (the stack is then a ring [bot, sp): pushes and pops at
// sp, steals at bot; the i-th idle lane in lane order takes from the i-th lane with entries).  Every
// child pushed is visited by one lane or skipped because its key exceeds the group's best (never below
// the final best: skipped soundly), so the group's lanes together test every triangle the G = 1 query
// would need; the answer (minimum over the lanes' records, a tie when two lanes hold it or one lane saw
// two) is the same on every lane of the group.
// start (optional, one query per call): the nodes the walk starts at instead of the root: a
// caller passes a set that every child the root query would enter for this ray lies below, with only inner
// nodes above it; nullptr: the root.
// No lane refill (the default): one query per call.
struct WNoFeed {
    static constexpr bool on = false;
    bool busy = false;
    bool drained = true;   // (wave-uniform) the feed has no query left to hand out
    int threshold = 64;
    template <class H> RT_HD void finish(int, H&, v3, v3) {}
    RT_HD bool fetch(bool, v3&, v3&, float&, bool&) { return false; }
};

template <class Stack, int G = 1, class Feed = WNoFeed, bool NOB = false, bool LAZY = false>
RT_HD int wbvh_closest(const WNode* nodes, const GTri* tris, v3 o, v3 d, float m, Stack& stk, WHit& h,
                       uint32_t* work = nullptr, float hi = INFINITY, bool ties = true, float QS = 0x1p-8f,
                       const uint64_t* risk = nullptr, int rsel = 0, float rsub = 0.0f, uint32_t max_steps = 0,
                       Feed* feed = nullptr, bool nob = false, const uint32_t* start = nullptr)
{
    static_assert(G == 1 || ((G & (G - 1)) == 0 && G <= 8 && (Stack::CAP & (Stack::CAP - 1)) == 0),
                  "a lane group: a power of two up to 8 lanes, a ring stack of 2^k entries");
    // Feed::on (device, one lane per query): lane refill.  The wave stays in the loop; a lane whose query
    // ended waits, and when at least feed->threshold lanes (or every lane) wait, each hands its query's
    // status and record to feed->finish and takes the next ray from feed->fetch (o, d, m and nob; hi, ties,
    // QS, the risk words, rsel and rsub are the same for every query of the feed).  The per-query work is the
    // one-query
    // call's: the same state, reset per query, the same steps.  Returns W_MISS once the feed is drained.
    constexpr bool FEED = Feed::on;
    static_assert(!FEED || G == 1, "lane refill: one lane per query");
    static_assert(!FEED || !NOB, "lane refill: nob comes with each ray (Feed::fetch)");
    // the stack index of entry i (a ring in a lane group)
    auto slot = [](int i) { return G > 1 ? (i & (Stack::CAP - 1)) : i; };
    h.t = INFINITY;
    h.u = 1.0f;
    h.v = 0.0f;
    h.k = -1;
    // slab parameters: t = (lo - (o + M)) / d and (hi - (o - M)) / d over the box widened by M.
    // A direction component below 2^-100 in magnitude (or 0) is treated as +-2^-100: the
    // slab's t range then exceeds 2^70 m / |d| on the far side, far beyond the scene's, so
    // it constrains only as much as the true one does (the margin covers the origin's side).
    const float DMIN = 0x1p-100f;
    constexpr float SL = 0x1p-20f;   // relative slack over the rounding of a slab parameter (<= 3 ulp)
    constexpr float NLH = 127.9f;    // |N| of a quantised slab normal: 127 +- sqrt(3) / 2 (wbvh.cpp quantise)
    float ix, iy, iz, aix, aiy, aiz, dl, cstep, idl, icp, iqd;
    bool nx_lo, ny_lo, nz_lo;
    auto setup = [&]() {
        ix = 1.0f / (fabsf(d.x) < DMIN ? copysignf(DMIN, d.x) : d.x);
        iy = 1.0f / (fabsf(d.y) < DMIN ? copysignf(DMIN, d.y) : d.y);
        iz = 1.0f / (fabsf(d.z) < DMIN ? copysignf(DMIN, d.z) : d.z);
        // per axis, the byte row of the entry (near) planes: q_lo where the direction is positive,
        // q_hi where it is negative; the near plane is widened by -M sign(d), the far one by +M sign(d)
        nx_lo = !(ix < 0.0f);
        ny_lo = !(iy < 0.0f);
        nz_lo = !(iz < 0.0f);
        aix = fabsf(ix);
        aiy = fabsf(iy);
        aiz = fabsf(iz);
        // |d| rounded up (sqrt and dot within 2^-22), times the cone step: threshold = c * cstep
        dl = sqrtf(d.x * d.x + d.y * d.y + d.z * d.z) * (1.0f + 0x1p-20f);
        cstep = dl * W_CONE_STEP;
        // 1 / |d| rounded up (|d| rounded down, the hardware reciprocal within 1 ulp)
        idl = fast_rcp(sqrtf(d.x * d.x + d.y * d.y + d.z * d.z) * (1.0f - 0x1p-20f)) * (1.0f + 0x1p-18f);
        icp = (1.0f - 0x1p-18f) / (NLH * dl);   // cos(angle(N, -d)) >= -a icp
        iqd = (1.0f - 0x1p-20f) / (QS * dl);    // a risk key's t bound: key / (QS |d|)
    };
    setup();
    float best_s = hi + fabsf(hi) * SL;   // h.t (or hi) plus slack: a child entered at or below it may hold a hit
    bool tie = false, nanhit = false, infhit = false;
    float dropped = INFINITY;   // the smallest key of the children a full stack could not take
    int sp = 0, bot = 0;        // the stack's entries [bot, sp) (bot > 0: entries taken by the group)
    uint32_t cur = FEED || (G > 1 && wg_lane<G>() != 0) ? W_EMPTY : 0u;   // root node (FEED: no query yet)
    if (!FEED && start && cur != W_EMPTY) {
        // the start set (wbvh_entry_block, W_ENTRY_MAX links, W_EMPTY in unused slots; G > 1: group lane 0
        // holds it): the first link is visited now, the others wait on the stack with key 0 (never culled),
        // the second on top
        cur = start[0];
        for (int i = W_ENTRY_MAX - 1; i >= 1; i--)
            if (start[i] != W_EMPTY)
                stk.put(slot(sp++), make_uint2(start[i], 0u));
    }
    uint32_t nn = 0, nt = 0;
    uint32_t steps = 0;   // loop iterations (node or leaf visits)
    // the status of the lane's query once its loop is over (G = 1; the tail below for every G)
    auto status = [&]() -> int {
        const bool ovf = dropped < INFINITY && dropped <= best_s;
        if (nanhit)
            return W_UNCERT;
        if (h.k < 0) {
            if (infhit)
                return W_UNCERT;
            if (ovf)
                return W_DEEP;
            h.t = -1.0f;   // HitInfo() (hitInfo.h:8-24): t = -1, u = 1, v = 0
            return W_MISS;
        }
        if ((ties && tie) || !(h.t > 0.0f && h.t < INFINITY))
            return W_UNCERT;
        return ovf ? W_DEEP : W_HIT;
    };
    // FEED: at the loop's head, with the wave together; false once the feed is drained and no lane runs
    (void)status;
    auto refill = [&]() -> bool {
        if constexpr (FEED) {
#if defined(__HIP_DEVICE_COMPILE__)
            const bool idle_lane = cur == W_EMPTY;
            const uint64_t idle = __ballot(idle_lane);
            if (idle != 0ull && (idle == __ballot(1) || __popcll(idle) >= feed->threshold)) {
                if (idle_lane && feed->busy)
                    feed->finish(status(), h, o, d);
                if (feed->fetch(idle_lane, o, d, m, nob)) {   // (wave-uniform call; true for the lanes given a ray)
                    setup();
                    h.t = INFINITY;
                    h.u = 1.0f;
                    h.v = 0.0f;
                    h.k = -1;
                    best_s = hi + fabsf(hi) * SL;
                    tie = nanhit = infhit = false;
                    dropped = INFINITY;
                    sp = bot = 0;
                    cur = 0u;
                }
                return __ballot(cur != W_EMPTY) != 0ull || !feed->drained;
            }
#endif
        }
        return true;
    };
    while (FEED ? refill() : (G > 1 ? wg_bits<G>(cur != W_EMPTY) != 0u : cur != W_EMPTY)) {
        if constexpr (FEED) {
            if (cur == W_EMPTY)
                continue;   // (waits for the refill)
        }
        ++steps;
        if (max_steps && steps > max_steps)
            return W_LONG;
        // ---- inner nodes: test the four child boxes, go to the nearest, push the others ----
        // if-if: every lane takes one step (inner node or leaf) per iteration
        if (!(cur & W_LEAF)) {
            nn++;
            W_STEP_HOOK(cur, 0);
            W_NOB_HOOK(NOB || nob);
            const uint4* p = reinterpret_cast<const uint4*>(nodes + cur);
            constexpr int NR = WN_ROWS;
            uint4 Rw[NR];
#pragma unroll
            for (int i = 0; i < NR; i++)
                Rw[i] = ldg(p + i);
            // word i of the node (compile-time i)
            auto wd = [&](int i) -> uint32_t {
                const uint4 r = Rw[i >> 2];
                return (i & 3) == 0 ? r.x : (i & 3) == 1 ? r.y : (i & 3) == 2 ? r.z : r.w;
            };
            const float ss = bitsf(wd(WN_SS)), slo = bitsf(wd(WN_SS + 1));
            const uint32_t ex = wd(3);
            const float stx = bitsf((ex & 0xffu) << 23), sty = bitsf(((ex >> 8) & 0xffu) << 23),
                        stz = bitsf(((ex >> 16) & 0xffu) << 23);
            // t of a plane origin + q s (widened by M) = q (s / d) + (origin - o -+ M) / d
            const float sx = stx * ix, sy = sty * iy, sz = stz * iz;
            const float Dx = bitsf(wd(0)) - o.x, Dy = bitsf(wd(1)) - o.y, Dz = bitsf(wd(2)) - o.z;
            const float bx = Dx * ix, by = Dy * iy, bz = Dz * iz;
            // per axis, the byte rows of the entry (near) and exit (far) planes: q_lo where the direction
            // is positive, q_hi where it is negative (one select per node and row)
            constexpr int QW = W_WIDTH / 4;   // words per axis row of quantised planes
            uint32_t nwx[QW], fwx[QW], nwy[QW], fwy[QW], nwz[QW], fwz[QW];
#pragma unroll
            for (int jw = 0; jw < QW; jw++) {
                const uint32_t lx = wd(WN_QLO + 0 * QW + jw), hx = wd(WN_QHI + 0 * QW + jw);
                const uint32_t ly = wd(WN_QLO + 1 * QW + jw), hy = wd(WN_QHI + 1 * QW + jw);
                const uint32_t lz = wd(WN_QLO + 2 * QW + jw), hz = wd(WN_QHI + 2 * QW + jw);
                nwx[jw] = nx_lo ? lx : hx;
                fwx[jw] = nx_lo ? hx : lx;
                nwy[jw] = ny_lo ? ly : hy;
                fwy[jw] = ny_lo ? hy : ly;
                nwz[jw] = nz_lo ? lz : hz;
                fwz[jw] = nz_lo ? hz : lz;
            }
            // D: o to the farthest corner of the node's frame [origin, origin + 255 step]
            float Dn;
            {
                const float fx = fmaxf(fabsf(Dx), fabsf(__builtin_fmaf(255.0f, stx, Dx)));
                const float fy = fmaxf(fabsf(Dy), fabsf(__builtin_fmaf(255.0f, sty, Dy)));
                const float fz = fmaxf(fabsf(Dz), fabsf(__builtin_fmaf(255.0f, stz, Dz)));
                Dn = fast_sqrt(fx * fx + fy * fy + fz * fz) * (1.0f + 0x1p-16f) + m;
            }
            // the children's risk words for this ray's kind (wrisk_pack): key and at-risk box, for the lanes
            // whose case (b) can read them (a wave with no such lane skips the loads and their addresses)
            [[maybe_unused]] uint32_t rw[2 * W_WIDTH];
            if constexpr (NOB)
                ;   // (no case (b): nothing reads them)
            else if (LAZY && W_NOB_FAST ? risk && !nob : risk != nullptr) {
                const uint4* rp = reinterpret_cast<const uint4*>(risk + (2 * (size_t)cur + rsel) * W_WIDTH);
                const uint4 r0 = ldg(rp), r1 = ldg(rp + 1);
                rw[0] = r0.x; rw[1] = r0.y; rw[2] = r0.z; rw[3] = r0.w;
                rw[4] = r1.x; rw[5] = r1.y; rw[6] = r1.z; rw[7] = r1.w;
            } else {
#pragma unroll
                for (int i = 0; i < 2 * W_WIDTH; i++)
                    rw[i] = 0u;   // key 0 (unused: the full test runs)
            }
            float key[W_WIDTH];
            uint32_t ref[W_WIDTH];
            float pri[W_WIDTH];   // visiting order (key: the cull bound kept on the stack)
#pragma unroll
            for (int j = 0; j < W_WIDTH; j++) {
                const int sh = 8 * (j & 3), jw = j >> 2;
                const uint32_t chj = wd(WN_CHILD + j);
                ref[j] = chj;
                key[j] = INFINITY;
                pri[j] = INFINITY;
                const uint32_t nrj = wd(WN_NRM + j);
                const float nx = (float)(int8_t)(nrj & 0xffu), ny = (float)(int8_t)((nrj >> 8) & 0xffu),
                            nz = (float)(int8_t)((nrj >> 16) & 0xffu);
                const float a = nx * d.x + ny * d.y + nz * d.z;
                // every triangle below faces away when a exceeds the cone threshold (rounding of
                // a and of the threshold: < 1e-4 |d|, inside the build's 0.01 |d|): none reports a hit
                if (chj != W_EMPTY && !(a > (float)(nrj >> 24) * cstep)) {
                    const uint32_t e = wd(WN_EXT + j);
                    const float smin = fmaxf(wq_val_nz(e & 0xffu, WQ_UNIT), W_SMIN_FLOOR);
                    const float sth = wq_val_nz((e >> 16) & 0xffu, WQ_UNIT);
                    const float L = (e >> 24) == 255u ? INFINITY : wq_val_nz(e >> 24, WQ_LEN);
                    const float qlb = __builtin_fmaf(-sth, 1.0f + sth, -a * icp) - 0x1p-20f;
                    const float qa = fmaxf(qlb, QS);
                    const float qnx = (float)((nwx[jw] >> sh) & 0xffu), qfx = (float)((fwx[jw] >> sh) & 0xffu);
                    const float qny = (float)((nwy[jw] >> sh) & 0xffu), qfy = (float)((fwy[jw] >> sh) & 0xffu);
                    const float qnz = (float)((nwz[jw] >> sh) & 0xffu), qfz = (float)((fwz[jw] >> sh) & 0xffu);
                    // D for case (b): o to the farthest corner of child j's box (it holds the child's
                    // vertices; Dn's frame can be several times larger, and near the origin (b) is priced
                    // by D sin(theta)).  Case (a) keeps the node frame's Dn (sound either way)
                    [[maybe_unused]] auto dchild = [&]() -> float {
                        const float fx = fmaxf(fabsf(__builtin_fmaf(qnx, stx, Dx)), fabsf(__builtin_fmaf(qfx, stx, Dx)));
                        const float fy = fmaxf(fabsf(__builtin_fmaf(qny, sty, Dy)), fabsf(__builtin_fmaf(qfy, sty, Dy)));
                        const float fz = fmaxf(fabsf(__builtin_fmaf(qnz, stz, Dz)), fabsf(__builtin_fmaf(qfz, stz, Dz)));
                        return fast_sqrt(fx * fx + fy * fy + fz * fz) * (1.0f + 0x1p-16f) + m;
                    };
                    // (a): the box widened by R, the slab by eta + R sin(theta) (wq_reach: the correlated bound of
                    // Moller-Trumbore's reports, D = Dn)
                    const float Da = Dn;
                    // (a well-conditioned child seen at cos >= W_FAST_Q: the bounds' closed form, wq_fast)
                    const bool fastr = wq_fast_ok(qlb, e);
                    WReach wr;
                    // the box test: the line crosses the box widened by the lateral reach, and a report lies
                    // within Rpar of that crossing along the line (wq_split)
                    float E, Rlat, Rpar;
                    if (fastr)
                        wq_fast(L, Da, E, Rlat, Rpar);
                    else {
                        wr = wq_reach(qa, smin, L, Da);
                        E = wr.E;
                        wq_split(wr, L, Da, Rlat, Rpar);
                    }
                    const float R = E + m;
                    const float Rb = Rlat + m;
                    const float dtp = Rpar * idl;
                    // the entry / exit planes' t of this child's box widened by M:
                    // q (s / d) + (origin - o) / d -+ M / |d| per axis
                    auto box = [&](float M, float& tmin, float& tmax) {
                        const float tnx = __builtin_fmaf(-M, aix, __builtin_fmaf(qnx, sx, bx));
                        const float tny = __builtin_fmaf(-M, aiy, __builtin_fmaf(qny, sy, by));
                        const float tnz = __builtin_fmaf(-M, aiz, __builtin_fmaf(qnz, sz, bz));
                        const float tfx = __builtin_fmaf(M, aix, __builtin_fmaf(qfx, sx, bx));
                        const float tfy = __builtin_fmaf(M, aiy, __builtin_fmaf(qfy, sy, by));
                        const float tfz = __builtin_fmaf(M, aiz, __builtin_fmaf(qfz, sz, bz));
                        tmin = fmaxf(fmaxf(tnx, tny), tnz);
                        tmax = fminf(fminf(tfx, tfy), tfz);
                    };
                    const uint32_t sbj = wd(WN_SLAB + j);
                    const float C0 = __builtin_fmaf((float)(sbj & 0xffffu), ss, slo);
                    const float C1 = __builtin_fmaf((float)(sbj >> 16), ss, slo);
                    const float b = nx * Dx + ny * Dy + nz * Dz;   // N . (origin - o)
                    float tmin, tmax;
                    box(Rb, tmin, tmax);
                    tmin -= dtp;
                    tmax += dtp;
                    // enter when max(tmin, 0) <= min(tmax (1 + SL), best_s); a NaN tmin (every
                    // slab NaN) enters too.  The key orders the children; misses get INFINITY.
                    bool ok = fmaxf(tmin, 0.0f) <= fminf(__builtin_fmaf(fabsf(tmax), SL, tmax), best_s);
                    // the slab only narrows the box's interval: skipped when no lane's box passes
                    if (ok && R < INFINITY) {
                        // N . (o + t d - origin) in [C0, C1] widened by w: t between
                        // (C0 - w + b) / a and (C1 + w + b) / a
                        const float eta = fastr ? wq_fast_eta(L, Da) : wq_eta(wr, L, Da);
                        const float w = NLH * __builtin_fmaf(R, sth, eta) * (1.0f + 0x1p-16f) + 384.0f * m;
                        // the hardware reciprocal (1 ulp): its error moves the slab's t by a relative
                        // 2^-23, a distance far inside the margin over the scene
                        const float ia = fast_rcp(a);
                        const float s0 = (C0 - w + b) * ia, s1 = (C1 + w + b) * ia;
                        tmin = fmaxf(tmin, fminf(s0, s1));
                        tmax = fminf(tmax, fmaxf(s0, s1));
                        ok = fmaxf(tmin, 0.0f) <= fminf(__builtin_fmaf(fabsf(tmax), SL, tmax), best_s);
                    }
                    if (ok)
                        key[j] = fminf(fmaxf(tmin, 0.0f), 3.0e38f);
                    // (b): triangles that may lie nearly parallel to d (q < QS), none of whose reports
                    // precedes kbl (the risk key): the line must cross the octree leaves holding them
                    // (the child box widened by rho, any t), and the origin must lie within H0
                    // (wq_h0) of a triangle's plane, so within H0 + D sin(theta)
                    // of the child's slab (D = dchild() >= |o - a|)
                    if constexpr (!NOB) {
                        const float rkj = bitsf(rw[2 * j + 1] & 0xFFFF0000u);   // wrisk_key
                        const float kbl = (rkj - rsub) * iqd;
                        if (!risk && !nob && qlb < QS) {
                            // no risk words (reflection rays, rt_trace_ray):
                            // the child box widened by m + rho (any t) and the origin within H0 + D sin(theta) of
                            // the slab; keyed 0 (no risk key bounds the reports' t)
                            float umin, umax;
                            const uint32_t e2 = wd(WN_EXT2 + j);
                            box(m + wq_len(e2 & 0xffu), umin, umax);
                            bool okb = !(umin > __builtin_fmaf(fabsf(umax), SL, umax));
                            if (okb) {
                                const float s2 = wq_val_nz((e >> 8) & 0xffu, WQ_UNIT);
                                const float Dc = dchild();
                                const float H0 = wq_h0(QS, L, Dc, smin, s2);
                                const float w = NLH * (H0 + __builtin_fmaf(Dc, sth, m)) * (1.0f + 0x1p-16f) + 384.0f * m;
                                okb = !(-b < C0 - w || -b > C1 + w);
                            }
                            if (okb)
                                key[j] = 0.0f;
                        } else if (risk && !nob && qlb < QS && rkj < INFINITY && !(kbl > best_s)) {
                            const uint32_t e2 = wd(WN_EXT2 + j);
                            // the at-risk octree leaves' box widened by m + rho (any t)
                            const float Mb = m + wq_len(e2 & 0xffu);
                            const uint32_t r0 = rw[2 * j], r1 = rw[2 * j + 1];   // lo x y z, hi x y z bytes
                            const float blx = (float)(r0 & 0xffu), bly = (float)((r0 >> 8) & 0xffu),
                                        blz = (float)((r0 >> 16) & 0xffu), bhx = (float)(r0 >> 24),
                                        bhy = (float)(r1 & 0xffu), bhz = (float)((r1 >> 8) & 0xffu);
                            const float umin = fmaxf(fmaxf(__builtin_fmaf(-Mb, aix, __builtin_fmaf(nx_lo ? blx : bhx, sx, bx)),
                                                           __builtin_fmaf(-Mb, aiy, __builtin_fmaf(ny_lo ? bly : bhy, sy, by))),
                                                     __builtin_fmaf(-Mb, aiz, __builtin_fmaf(nz_lo ? blz : bhz, sz, bz)));
                            const float umax = fminf(fminf(__builtin_fmaf(Mb, aix, __builtin_fmaf(nx_lo ? bhx : blx, sx, bx)),
                                                           __builtin_fmaf(Mb, aiy, __builtin_fmaf(ny_lo ? bhy : bly, sy, by))),
                                                     __builtin_fmaf(Mb, aiz, __builtin_fmaf(nz_lo ? bhz : blz, sz, bz)));
                            bool okb = !(umin > __builtin_fmaf(fabsf(umax), SL, umax));
                            if (okb) {
                                const float s2 = wq_val_nz((e >> 8) & 0xffu, WQ_UNIT);
                                const float Dc = dchild();
                                const float H0 = wq_h0(QS, L, Dc, smin, s2);
                                const float w = NLH * (H0 + __builtin_fmaf(Dc, sth, m)) * (1.0f + 0x1p-16f) + 384.0f * m;
                                okb = !(-b < C0 - w || -b > C1 + w);   // N . (o - origin) = -b
                            }
                            if (okb)
                                key[j] = fminf(key[j], fminf(fmaxf(kbl, 0.0f), 3.0e38f));
                        }
                    }
                    // visit order: the entry t of the child's unwidened box (not below the key).  A child
                    // holding ill-conditioned triangles (UV-sphere pole slivers) has a box widened by a
                    // large R whose entry t precedes the actual hit; ordered by that key the query walked
                    // such subtrees first, with no best hit to cull them yet (grazing C4 rays: 144 of 156
                    // entered children before the hit).  The order does not change the answer.
                    if (key[j] < INFINITY)
                        pri[j] = fmaxf(key[j], fmaxf(fmaxf(__builtin_fmaf(qnx, sx, bx), __builtin_fmaf(qny, sy, by)),
                                                     __builtin_fmaf(qnz, sz, bz)));
                }
#if defined(__HIP_DEVICE_COMPILE__)
                // one child at a time: the scheduler would interleave the children's
                // temporaries (VALU latency is hidden by the other waves anyway)
                __builtin_amdgcn_sched_barrier(0);
#endif
            }
            // sort the (pri, key, ref) triples ascending by pri: misses (INFINITY) go last
#define W_CSWAP(a, b)                                                              \
    if (pri[b] < pri[a]) {                                                         \
        float tp = pri[a]; pri[a] = pri[b]; pri[b] = tp;                           \
        float tk = key[a]; key[a] = key[b]; key[b] = tk;                           \
        uint32_t tr = ref[a]; ref[a] = ref[b]; ref[b] = tr;                        \
    }
            W_CSWAP(0, 1) W_CSWAP(2, 3) W_CSWAP(0, 2) W_CSWAP(1, 3) W_CSWAP(1, 2)
#undef W_CSWAP
            if (key[0] < INFINITY) {
                cur = ref[0];
#pragma unroll
                for (int j = W_WIDTH - 1; j >= 1; j--)
                    if (key[j] < INFINITY) {
                        if (sp - bot < Stack::CAP)
                            stk.put(slot(sp++), make_uint2(ref[j], fbits(key[j])));
                        else {
                            // full: the entry with the largest key goes (the new child or one on the
                            // stack, which it replaces); the query stays certified if the dropped key
                            // exceeds the final best hit
                            int im = -1;
                            float km = key[j];
                            for (int i = 0; i < Stack::CAP; i++) {
                                const float ki = bitsf(stk.get(i).y);
                                if (ki > km) {
                                    km = ki;
                                    im = i;
                                }
                            }
                            if (im >= 0)
                                stk.put(im, make_uint2(ref[j], fbits(key[j])));
                            dropped = fminf(dropped, km);
                        }
                    }
            } else {
                cur = W_EMPTY;
                while (sp > bot) {
                    uint2 e = stk.get(slot(--sp));
                    if (bitsf(e.y) <= best_s) {
                        cur = e.x;
                        break;
                    }
                }
            }
        }
        else if (G == 1 || cur != W_EMPTY) {   // (an idle lane of a group: no step)
        // ---- a leaf: its triangles, closest hit kept; equal t from another triangle is a tie ----
        W_STEP_HOOK(cur, 1);
        const uint32_t first = (cur >> 3) & 0x0FFFFFFFu, cnt = (cur & 7u) + 1u;
        const uint32_t kend = first + cnt;
        // the leaf's triangles in order (loading two records at a time was measured slower)
        auto fold = [&](const GTri& T, uint32_t k) {
            nt++;
            float t, u, v;
            if (mt_record(T, o, d, t, u, v)) {
                if (t != t)
                    nanhit = true;
                else if (!(t <= hi))
                    ;   // beyond the segment
                else if (t == INFINITY)
                    infhit = true;   // overflowed t: only matters when no finite hit exists
                else if (t < h.t) {
                    h.t = t;
                    h.u = u;
                    h.v = v;
                    h.k = (int32_t)k;
                    tie = false;
                    best_s = t + fabsf(t) * SL;
                } else if (t == h.t)
                    tie = true;
            }
        };
        for (uint32_t k = first; k < kend; k++)
            fold(load_gtri(tris + k), k);
        cur = W_EMPTY;
        while (sp > bot) {
            uint2 e = stk.get(slot(--sp));
            if (bitsf(e.y) <= best_s) {
                cur = e.x;
                break;
            }
        }
        }
        if constexpr (G > 1) {
            // the group's best bound, then the idle lanes take work: the i-th idle lane the bottom
            // (oldest: the largest subtree) entry of the i-th lane holding entries
            best_s = wg_min<G>(best_s);
            const uint32_t idle = wg_bits<G>(cur == W_EMPTY), busy = wg_bits<G>(sp > bot);
            if (idle && busy) {
                const uint32_t gl = wg_lane<G>(), below = (1u << gl) - 1u;
                int src = -1;
                if (cur == W_EMPTY) {
                    uint32_t b = busy;
                    for (int r = __builtin_popcount(idle & below); r > 0 && b; r--)
                        b &= b - 1u;
                    src = b ? __builtin_ctz(b) : -1;
                }
                const int sbot = wg_read<G>(bot, src >= 0 ? src : (int)gl);
                if (sp > bot && __builtin_popcount(busy & below) < __builtin_popcount(idle))
                    bot++;   // (the taker reads the entry below before any later push can reuse its slot)
                if (src >= 0) {
                    const uint2 e = stk.get_lane(src - (int)gl, slot(sbot));
                    if (bitsf(e.y) <= best_s)
                        cur = e.x;
                }
            }
        }
    }
    if constexpr (G > 1) {
        // the group's answer: the least t over its lanes' records; a tie when two lanes hold it (each
        // triangle is tested by one lane at most) or the lane holding it saw two
        const float T = wg_min<G>(h.t);
        const uint32_t at = wg_bits<G>(h.k >= 0 && h.t == T);
        const int w = at ? __builtin_ctz(at) : 0;
        tie = __builtin_popcount(at) > 1 || wg_bits<G>(h.k >= 0 && h.t == T && tie) != 0u;
        h.t = wg_read<G>(h.t, w);
        h.u = wg_read<G>(h.u, w);
        h.v = wg_read<G>(h.v, w);
        h.k = wg_read<G>(h.k, w);
        nanhit = wg_bits<G>(nanhit) != 0u;
        infhit = wg_bits<G>(infhit) != 0u;
        dropped = wg_min<G>(dropped);
        best_s = wg_min<G>(best_s);
    }
    // a dropped child matters only if it could hold a hit at t <= the final best (a pop would have
    // skipped it otherwise)
    const bool overflow = dropped < INFINITY && dropped <= best_s;
    if (work) {
        work[0] += nn;
        work[1] += nt;
        work[3] += steps;
        // why a query is not certified (diagnostics): 1 stack overflow, 2 NaN hit,
        // 4 only overflowed hits, 8 tie, 16 minimum t not in (0, inf)
        work[2] = (overflow ? 1u : 0u) | (nanhit ? 2u : 0u) | (h.k < 0 && infhit ? 4u : 0u) |
                  (h.k >= 0 && ties && tie ? 8u : 0u) | (h.k >= 0 && !(h.t > 0.0f && h.t < INFINITY) ? 16u : 0u);
    }
    if constexpr (FEED)
        return W_MISS;   // (every query went to feed->finish)
    if (nanhit)
        return W_UNCERT;
    if (h.k < 0) {
        if (infhit)
            return W_UNCERT;
        if (overflow)
            return W_DEEP;
        h.t = -1.0f;   // HitInfo() (hitInfo.h:8-24): t = -1, u = 1, v = 0
        return W_MISS;
    }
    if ((ties && tie) || !(h.t > 0.0f && h.t < INFINITY))
        return W_UNCERT;
    return overflow ? W_DEEP : W_HIT;
}

}  // namespace rt
