// wbvh_quick.hpp -- the per-node arithmetic of the quick wide BVH (wbvh.hpp build_wbvh_quick, DESIGN.md
// 5.9), one set of expressions for the host builder (wbvh.cpp) and the device builder
// (wbvh_quick_gpu.hip).  Everything is built with -ffp-contract=off; the double products of floats are
// exact, IEEE division and sqrt are correctly rounded on both sides, and floor / ceil / lround / frexp /
// ldexp / nextafter are exact, so with the same operation order the two builders produce the same bytes
// wherever no transcendental (acos, cos, sin: the cone code and sth) is involved.
#pragma once

#include "wbvh.hpp"

namespace rt {
namespace quick {

// std::min / std::max's rule (the first operand on a tie or a NaN), host and device
template <class T>
RT_HD T qmin(T a, T b)
{
    return b < a ? b : a;
}
template <class T>
RT_HD T qmax(T a, T b)
{
    return a < b ? b : a;
}

struct Box {
    float lo[3], hi[3];
};

RT_HD Box empty_box() { return Box{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}}; }
RT_HD void grow(Box& b, const Box& o)
{
    for (int a = 0; a < 3; a++) {
        b.lo[a] = qmin(b.lo[a], o.lo[a]);
        b.hi[a] = qmax(b.hi[a], o.hi[a]);
    }
}

// float lower / upper bound of a double
RT_HD float down(double x)
{
    float f = (float)x;
    return (double)f > x ? nextafterf(f, -INFINITY) : f;
}
RT_HD float up(double x)
{
    float f = (float)x;
    return (double)f < x ? nextafterf(f, INFINITY) : f;
}

// the box of a record's vertices a, a + ab, a + ac (exact sums in double, rounded outward)
RT_HD Box tri_box(const GTri& g)
{
    Box b;
    for (int c = 0; c < 3; c++) {
        double a = g.a[c], p = a + (double)g.ab[c], q = a + (double)g.ac[c];
        b.lo[c] = down(qmin(a, qmin(p, q)));
        b.hi[c] = up(qmax(a, qmax(p, q)));
    }
    return b;
}

// The conditioning bytes (wbvh.hpp wq_val): the largest code whose value is <= x (a lower
// bound on a sine in [0, 1]), and the smallest code whose value is >= x (an upper bound; for
// lengths 255 = no bound).
RT_HD uint32_t wq_code_lb(double x)
{
    if (!(x > 0))
        return 0u;
    if (x >= 1)
        return 255u;
    float f = (float)x;
    if ((double)f > x)
        f = nextafterf(f, 0.0f);
    const uint32_t bits = fbits(f);
    if (bits < WQ_UNIT + (1u << 20))
        return 0u;
    const uint32_t k = (bits - WQ_UNIT) >> 20;
    return k > 255u ? 255u : k;
}

RT_HD uint32_t wq_code_ub(double x, uint32_t base)
{
    if (!(x > 0))
        return x == 0 ? 0u : 255u;   // (NaN: no bound)
    float f = (float)x;
    if ((double)f < x)
        f = nextafterf(f, INFINITY);
    const uint32_t bits = fbits(f);
    if (bits <= base + (1u << 20))
        return 1u;
    const uint32_t k = (bits - base + (1u << 20) - 1u) >> 20;
    if (base == WQ_UNIT)
        return k > 255u ? 255u : k;
    return k > 254u ? 255u : k;
}

// the decoded box of child j (double, exact)
RT_HD Box decode(const WNode& w, int j, double lo[3], double hi[3])
{
    const float org[3] = {w.ox, w.oy, w.oz};
    Box b;
    for (int a = 0; a < 3; a++) {
        const double st = ldexp(1.0, (int)((w.exps >> (8 * a)) & 0xffu) - 127);
        lo[a] = org[a] + w.qlo[a][j] * st;
        hi[a] = org[a] + w.qhi[a][j] * st;
        b.lo[a] = down(lo[a]);
        b.hi[a] = up(hi[a]);
    }
    return b;
}

// A child of a quick-tree node while it is built: a run of triangles, or a node below
struct QChild {
    Box box;
    uint32_t link = W_EMPTY;   // W_LEAF | first << 3 | (count - 1), or a node index
    double ns[3] = {0, 0, 0};  // sum of the stored normals (the slab normal's direction)
    int nq[3] = {1, 0, 0};     // the quantised slab normal (quantise's rule)
    double slo = INFINITY, shi = -INFINITY;   // range of nq . v over the triangles' vertices (absolute)
    double tc = 0, ts = 0;     // half-angles between nq and the stored normals / the exact normals below
    bool nocone = false, nosth = false;
    double smin = 1.0, s2 = 1.0, lmax = 0.0;
    int32_t leaf = -1;         // a run of an octree leaf's triangles: that leaf (rho against its axis box)
};

RT_HD void q_normal(QChild& c)
{
    const double len = sqrt(c.ns[0] * c.ns[0] + c.ns[1] * c.ns[1] + c.ns[2] * c.ns[2]);
    for (int a = 0; a < 3; a++)
        c.nq[a] = len > 0 ? (int)lround(127.0 * c.ns[a] / len) : (a == 0 ? 1 : 0);
    if (c.nq[0] == 0 && c.nq[1] == 0 && c.nq[2] == 0)
        c.nq[0] = 1;
}

RT_HD double q_len(const int* q) { return sqrt((double)q[0] * q[0] + (double)q[1] * q[1] + (double)q[2] * q[2]); }

// angle between two quantised normals, rounded up (acos near 1 turns the cosine's rounding, ~1e-16,
// into ~1.5e-8 of angle: 1e-7 of slack)
RT_HD double q_angle(const int* a, const int* b)
{
    const double c = ((double)a[0] * b[0] + (double)a[1] * b[1] + (double)a[2] * b[2]) / (q_len(a) * q_len(b));
    return acos(qmax(-1.0, qmin(1.0, c))) + 1e-7;
}

// a run of triangles [first, first + cnt) of the wide order (record i: t[map[i]]): everything from the
// triangles themselves
RT_HD void q_from_tris(QChild& c, const GTri* t, const int32_t* map, int32_t first, int32_t cnt)
{
    c.box = empty_box();
    for (int a = 0; a < 3; a++)
        c.ns[a] = 0;
    for (int32_t i = first; i < first + cnt; i++) {
        const GTri& T = t[map[i]];
        grow(c.box, tri_box(T));
        for (int a = 0; a < 3; a++)
            c.ns[a] += (double)T.n[a];
    }
    q_normal(c);
    const double n0 = c.nq[0], n1 = c.nq[1], n2 = c.nq[2], NL = q_len(c.nq);
    double cmin = 1.0, smn = 1.0;   // stored normals (cone), exact normals (sth)
    for (int32_t i = first; i < first + cnt; i++) {
        const GTri& T = t[map[i]];
        const double a0 = T.a[0], a1 = T.a[1], a2 = T.a[2];
        const double s0 = n0 * a0 + n1 * a1 + n2 * a2;
        const double s1 = n0 * (a0 + (double)T.ab[0]) + n1 * (a1 + (double)T.ab[1]) + n2 * (a2 + (double)T.ab[2]);
        const double sv = n0 * (a0 + (double)T.ac[0]) + n1 * (a1 + (double)T.ac[1]) + n2 * (a2 + (double)T.ac[2]);
        c.slo = qmin(c.slo, qmin(s0, qmin(s1, sv)));
        c.shi = qmax(c.shi, qmax(s0, qmax(s1, sv)));
        const double m0 = T.n[0], m1 = T.n[1], m2 = T.n[2];
        const double mlen = sqrt(m0 * m0 + m1 * m1 + m2 * m2);
        if (mlen == 0)
            continue;   // Mdet = 0: never a hit (no cone, no conditioning bound needed)
        if (!(mlen > 1e-30 && mlen < 1e27))
            c.nocone = true;
        else
            cmin = qmin(cmin, (m0 * n0 + m1 * n1 + m2 * n2) / (mlen * NL));
        const double x0 = T.ab[0], x1 = T.ab[1], x2 = T.ab[2], y0 = T.ac[0], y1 = T.ac[1], y2 = T.ac[2];
        const double c0 = x1 * y2 - x2 * y1, c1 = x2 * y0 - x0 * y2, c2 = x0 * y1 - x1 * y0;
        const double la = sqrt(x0 * x0 + x1 * x1 + x2 * x2), lc = sqrt(y0 * y0 + y1 * y1 + y2 * y2);
        const double cl = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
        c.lmax = qmax(c.lmax, qmax(la, lc) * (1 + 1e-12));
        c.smin = qmin(c.smin, sin_at_a_lb(T));
        if (!(la * lc > 0x1p-100) || !(cl > 0x1p-50 * la * lc)) {
            c.s2 = 0.0;
            c.nosth = true;
            continue;
        }
        const double ca = fabs(x0 * y0 + x1 * y1 + x2 * y2) / (la * lc);
        c.s2 = qmin(c.s2, sqrt(qmax(0.0, (1.0 - qmin(1.0, ca + 1e-12)) / 2.0)) * (1 - 1e-9));
        smn = qmin(smn, (c0 * n0 + c1 * n1 + c2 * n2) / (cl * NL) - 1e-12);
    }
    c.tc = acos(qmax(-1.0, qmin(1.0, cmin))) + 1e-7;
    c.ts = acos(qmax(-1.0, qmin(1.0, smn))) + 1e-7;
}

// an upper child from its children (and the octree node's axis box, which it holds)
RT_HD void q_combine(QChild& p, const QChild* ch, int nc, const Box* extra)
{
    p.box = empty_box();
    if (extra)
        p.box = *extra;
    for (int a = 0; a < 3; a++)
        p.ns[a] = 0;
    p.nocone = p.nosth = false;
    p.smin = p.s2 = 1.0;
    p.lmax = 0.0;
    for (int i = 0; i < nc; i++) {
        grow(p.box, ch[i].box);
        for (int a = 0; a < 3; a++)
            p.ns[a] += ch[i].ns[a];
        p.nocone |= ch[i].nocone;
        p.nosth |= ch[i].nosth;
        p.smin = qmin(p.smin, ch[i].smin);
        p.s2 = qmin(p.s2, ch[i].s2);
        p.lmax = qmax(p.lmax, ch[i].lmax);
    }
    q_normal(p);
    p.tc = p.ts = 0;
    for (int i = 0; i < nc; i++) {
        const double d = q_angle(p.nq, ch[i].nq);
        p.tc = qmax(p.tc, d + ch[i].tc);
        p.ts = qmax(p.ts, d + ch[i].ts);
    }
    // the slab: the range of nq . v over the box's corners (the box holds every vertex below)
    p.slo = INFINITY;
    p.shi = -INFINITY;
    for (int k = 0; k < 8; k++) {
        const double v0 = (k & 1) ? p.box.hi[0] : p.box.lo[0], v1 = (k & 2) ? p.box.hi[1] : p.box.lo[1],
                     v2 = (k & 4) ? p.box.hi[2] : p.box.lo[2];
        const double sv = p.nq[0] * v0 + p.nq[1] * v1 + p.nq[2] * v2;
        p.slo = qmin(p.slo, sv);
        p.shi = qmax(p.shi, sv);
    }
    p.leaf = -1;
}

// the node's boxes (quantise's rule), then per child the slab (absolute range shifted to the node's
// origin, widened by the rounding of that shift), the cone code, the conditioning bytes and rho
// (onodes: the flattened octree's nodes, for a leaf run's reach past its octree leaf's axis box)
RT_HD WNode q_node(const QChild* ch, int nc, const GNode* onodes)
{
    WNode w = {};
    Box nb = empty_box();
    for (int j = 0; j < nc; j++)
        grow(nb, ch[j].box);
    const float org[3] = {nb.lo[0], nb.lo[1], nb.lo[2]};
    w.ox = org[0];
    w.oy = org[1];
    w.oz = org[2];
    for (int a = 0; a < 3; a++) {
        const double ext = (double)nb.hi[a] - (double)org[a];
        int k = -100;
        if (ext > 0) {
            int e;
            frexp(ext / 255.0, &e);
            k = qmax(-100, qmin(127, e - 1));
            while (k < 127 && ldexp(255.0, k) < ext)
                k++;
        }
        w.exps |= (uint32_t)(127 + k) << (8 * a);
        const double st = ldexp(1.0, k);
        for (int j = 0; j < nc; j++) {
            const double lo = floor(((double)ch[j].box.lo[a] - org[a]) / st);
            const double hi = ceil(((double)ch[j].box.hi[a] - org[a]) / st);
            w.qlo[a][j] = (uint8_t)qmax(0.0, qmin(255.0, lo));
            w.qhi[a][j] = (uint8_t)qmax(0.0, qmin(255.0, hi));
        }
    }
    for (int j = 0; j < W_WIDTH; j++)
        w.child[j] = j < nc ? ch[j].link : W_EMPTY;
    double lo[W_WIDTH], hi[W_WIDTH], lo_all = INFINITY, hi_all = -INFINITY;
    for (int j = 0; j < nc; j++) {
        const double sh = (double)ch[j].nq[0] * org[0] + (double)ch[j].nq[1] * org[1] + (double)ch[j].nq[2] * org[2];
        // |rounding| of the absolute sums and of the shift: a few ulps of the largest magnitude
        const double slack = 0x1p-48 * (fabs(ch[j].slo) + fabs(ch[j].shi) + fabs(sh) +
                                        128.0 * (fabs((double)org[0]) + fabs((double)org[1]) + fabs((double)org[2])));
        lo[j] = ch[j].slo - sh - slack;
        hi[j] = ch[j].shi - sh + slack;
        lo_all = qmin(lo_all, lo[j]);
        hi_all = qmax(hi_all, hi[j]);
    }
    const float slo = down(lo_all);
    const double ext = hi_all - (double)slo;
    int k = -100;
    if (ext > 0) {
        int e;
        frexp(ext / 65535.0, &e);
        k = qmax(-100, qmin(127, e - 1));
        while (k < 127 && ldexp(65535.0, k) < ext)
            k++;
    }
    const double st = ldexp(1.0, k);
    w.s = (float)st;
    w.slo = slo;
    for (int j = 0; j < nc; j++) {
        const QChild& c = ch[j];
        // the cone code (cone_code's rule) from the half-angle
        int code = 255;
        const double NL = q_len(c.nq);
        const double psi = acos(W_CONE_EPS) - c.tc - 1e-9;
        if (!c.nocone && psi > 0) {
            const double cd = ceil((cos(psi) * NL + 0.01) / ((double)W_CONE_STEP * (1 - 1e-9)));
            code = cd <= 254 ? (int)cd : 255;
        }
        w.nrm[j] = (uint32_t)(uint8_t)(int8_t)c.nq[0] | ((uint32_t)(uint8_t)(int8_t)c.nq[1] << 8) |
                   ((uint32_t)(uint8_t)(int8_t)c.nq[2] << 16) | ((uint32_t)code << 24);
        double q0 = floor((lo[j] - (double)slo) / st), q1 = ceil((hi[j] - (double)slo) / st);
        q0 = qmax(0.0, qmin(65535.0, q0));
        q1 = qmax(0.0, qmin(65535.0, q1));
        w.slab[j] = (uint32_t)q0 | ((uint32_t)q1 << 16);
        const double sth = c.nosth || c.ts >= 3.14159265358979323846 / 2 ? 1.0 : qmin(1.0, sin(c.ts) + 1e-12);
        w.ext[j] = wq_code_lb(c.smin) | (wq_code_lb(c.s2) << 8) | (wq_code_ub(sth, WQ_UNIT) << 16) |
                   (wq_code_ub(c.lmax, WQ_LEN) << 24);
        double rho = 0.0;
        if (c.leaf >= 0) {
            double dlo[3], dhi[3];
            decode(w, j, dlo, dhi);
            const GNode& L = onodes[(size_t)c.leaf];
            for (int a = 0; a < 3; a++)
                rho = qmax(rho, qmax(dlo[a] - (double)L.dn[a], (double)L.df[a] - dhi[a]));
        }
        w.ext2[j] = wq_code_ub(rho, WQ_LEN);
    }
    return w;
}

// The 4-ary tree over an octree leaf's m runs of W_MAX_LEAF triangles (build_wbvh_quick's 'runs'): a
// node splits its runs over up to four children as evenly as possible (child p takes runs [m p / parts,
// m (p + 1) / parts)), a child of one run is a leaf child, a larger one a node.  Its node count R(m) in
// closed form: R(m) = 1 for m <= 4, m - 3 for m <= 8, else 1 + (m mod 4) R(m / 4 + 1) + (4 - m mod 4)
// R(m / 4); R(m) and R(m + 1) follow from R(m / 4) and R(m / 4 + 1) alone, one step per base-4 digit.
RT_HD uint32_t q_runs_nodes(uint32_t m)
{
    int K = 0;
    while ((m >> (2 * K)) > 8u)
        K++;
    const uint32_t x0 = m >> (2 * K);   // <= 8
    // R(x0) and R(x0 + 1): R(9) = 1 + R(3) + 3 R(2) = 5
    uint32_t r0 = x0 <= 4u ? 1u : x0 - 3u, r1 = x0 + 1u <= 4u ? 1u : (x0 + 1u <= 8u ? x0 - 2u : 5u);
    for (int k = K - 1; k >= 0; k--) {
        const uint32_t x = m >> (2 * k), y = x + 1u;   // r0 = R(x / 4), r1 = R(x / 4 + 1)
        const uint32_t n0 = 1u + (x & 3u) * r1 + (4u - (x & 3u)) * r0;
        const uint32_t n1 = (y & 3u) == 0u ? 1u + 4u * r1 : 1u + (y & 3u) * r1 + (4u - (y & 3u)) * r0;
        r0 = n0;
        r1 = n1;
    }
    return r0;
}

}  // namespace quick
}  // namespace rt
