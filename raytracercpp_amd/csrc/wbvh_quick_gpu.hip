// wbvh_quick_gpu.hip -- see wbvh_quick_gpu.hpp.  build_wbvh_quick (wbvh.cpp) plans the tree by a
// depth-first recursion over the octree; here the same numbering comes from subtree sizes:
//   sizes     bottom-up over the octree's levels: each octree node's wide-node count W and triangle
//             count T (a leaf of <= 8 triangles: 0 nodes; a larger one: its runs tree, q_runs_nodes; an
//             inner node: itself, its 0 / 1 / 2 group nodes and its children's)
//   plan      top-down: an inner node writes its wide node's plan and its group nodes' and hands each
//             child its wide index (after the earlier siblings' subtrees), first triangle and depth; a
//             leaf writes its triangles' slots in the wide order and, when large, its runs tree
//   geometry  the wide nodes deepest first, one lane per node: the host's per-node expressions
//             (wbvh_quick.hpp q_from_tris / q_node / q_combine), the aggregates kept per node
//   links     tri_leaf / parent from the nodes' child words
// The octree is in level order (OctreeDevInfo::level_base), so every level is one launch; a pass reads
// only what earlier launches wrote, no block waits for another, and the host reads two small totals
// back (the node count after 'sizes', the nodes per depth after 'plan').  Integer atomics only
// (counts, maxima, list positions: the tree's bytes do not depend on their order).
#include "wbvh_quick_gpu.hpp"

#include "wbvh_quick.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>

namespace rt {

using namespace quick;

namespace {

constexpr int BLOCK = 256;
constexpr int GEOM_BLOCK = 64;
constexpr int RUNS_STACK = 16;   // a runs tree over n <= 2^26 triangles is at most 12 deep

// a wide node's children: a run of triangles (b > 0: first a, count b, of octree leaf 'leaf') or a node (a)
struct QPlan {
    int32_t a[W_WIDTH], b[W_WIDTH], leaf[W_WIDTH];
    int32_t nc;
    int32_t oct;       // the octree node whose axis box the node's entry in its parent holds (-1: none)
    int32_t runleaf;   // a node over runs of octree leaf L's triangles: L
    int32_t depth;
};

struct Sub {   // the per-octree-node arrays (WQuickGpuScratch::sub)
    uint32_t *W, *T;
    int32_t *I, *F, *D;
};

__global__ __launch_bounds__(BLOCK) void wq_sizes_kernel(const GNode* __restrict__ nodes, int base, int count, int nn,
                                                         Sub s)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= count)
        return;
    const int u = base + i;
    const GNode g = load_gnode(nodes + u);
    uint32_t w, t;
    if (g.b & LEAF_BIT) {
        t = g.b & ~LEAF_BIT;
        // (the root leaf is a node over its runs even with one run)
        w = (t <= (uint32_t)W_MAX_LEAF && u != 0) ? 0u : q_runs_nodes((t + W_MAX_LEAF - 1) / W_MAX_LEAF);
    } else {
        const uint32_t cn = g.b < 8u ? g.b : 8u;
        w = 1u + (cn <= (uint32_t)W_WIDTH ? 0u : (cn <= 7u ? 1u : 2u));
        t = 0;
        for (uint32_t k = 0; k < cn; k++) {
            const uint32_t c = g.a + k;
            if (c < (uint32_t)nn) {
                w += s.W[c];
                t += s.T[c];
            }
        }
    }
    s.W[u] = w;
    s.T[u] = t;
}

struct PlanOut {
    QPlan* plans;
    int np;
    int32_t* slot;            // wide order -> octree slot
    uint32_t* leaf_of_slot;   // octree slot -> octree leaf
    int nt;
    WQuickDevInfo* info;
};

__device__ inline void note_plan(const PlanOut& o, int depth)
{
    if (depth >= 0 && depth < WQ_GPU_MAX_DEPTH)
        atomicAdd(&o.info->depth_count[depth], 1);
    atomicMax(&o.info->max_depth, depth);
}

// build_wbvh_quick's 'inner', 'entry' and 'runs' for the octree nodes of one level
__global__ __launch_bounds__(BLOCK) void wq_plan_kernel(const GNode* __restrict__ nodes, int base, int count, int nn,
                                                        Sub s, PlanOut o)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= count)
        return;
    const int u = base + i;
    if (u == 0) {
        s.I[0] = 0;
        s.F[0] = 0;
        s.D[0] = 0;
    }
    const GNode g = load_gnode(nodes + u);
    const int me = s.I[u], dep = s.D[u];
    int leaves = 0, maxleaf = 0;
    if (g.b & LEAF_BIT) {
        const int cnt = (int)(g.b & ~LEAF_BIT), first = s.F[u];
        for (int k = 0; k < cnt; k++) {
            if (first + k < o.nt)
                o.slot[first + k] = (int32_t)g.a + k;
            if (g.a + (uint32_t)k < (uint32_t)o.nt)
                o.leaf_of_slot[g.a + (uint32_t)k] = (uint32_t)u;
        }
        if (cnt <= W_MAX_LEAF && u != 0)
            return;   // a leaf child of its parent's node (counted there)
        // the runs tree, depth first (the host's recursion with an explicit stack)
        struct Frame {
            int first, cnt, me, p, r0;
        } st[RUNS_STACK];
        int sp = 0, next = me + 1;
        st[0] = Frame{first, cnt, me, 0, 0};
        if (me >= 0 && me < o.np) {
            o.plans[me].oct = u;
            o.plans[me].runleaf = u;
            o.plans[me].depth = dep;
            note_plan(o, dep);
        }
        while (sp >= 0) {
            Frame& f = st[sp];
            const int nr = (f.cnt + W_MAX_LEAF - 1) / W_MAX_LEAF;
            const int parts = nr < W_WIDTH ? nr : W_WIDTH;
            if (f.p >= parts) {
                if (f.me >= 0 && f.me < o.np)
                    o.plans[f.me].nc = parts;
                sp--;
                continue;
            }
            const int r1 = (int)((long long)nr * (f.p + 1) / parts);
            const int fr = f.first + f.r0 * W_MAX_LEAF;
            const int c = (f.cnt < r1 * W_MAX_LEAF ? f.cnt : r1 * W_MAX_LEAF) - f.r0 * W_MAX_LEAF;
            const int j = f.p, node = f.me;
            const bool one = r1 - f.r0 == 1;
            f.p++;
            f.r0 = r1;
            const bool ok = node >= 0 && node < o.np;
            if (one) {
                if (ok) {
                    o.plans[node].a[j] = fr;
                    o.plans[node].b[j] = c;
                    o.plans[node].leaf[j] = u;
                }
                leaves++;
                maxleaf = maxleaf > c ? maxleaf : c;
            } else {
                const int child = next++;
                if (ok) {
                    o.plans[node].a[j] = child;
                    o.plans[node].b[j] = 0;
                    o.plans[node].leaf[j] = -1;
                }
                if (sp + 1 >= RUNS_STACK)
                    break;   // (never: the depth bound above)
                if (child >= 0 && child < o.np) {
                    o.plans[child].oct = -1;
                    o.plans[child].runleaf = u;
                    o.plans[child].depth = dep + sp + 1;
                    note_plan(o, dep + sp + 1);
                }
                st[++sp] = Frame{fr, c, child, 0, 0};
            }
        }
    } else {
        const int c0 = (int)g.a, cn = (int)(g.b < 8u ? g.b : 8u);
        QPlan P;
        P.nc = 0;
        P.oct = u;
        P.runleaf = -1;
        P.depth = dep;
        for (int j = 0; j < W_WIDTH; j++) {
            P.a[j] = P.b[j] = 0;
            P.leaf[j] = -1;
        }
        int idx = me + 1, tri = s.F[u];
        // octree node c as child j of plan Q at depth qd
        auto entry = [&](int c, QPlan& Q, int j, int qd) {
            if (c < 0 || c >= nn)
                return;
            const uint32_t cb = nodes[c].b;
            const int cnt = (int)(cb & ~LEAF_BIT);
            s.F[c] = tri;
            if ((cb & LEAF_BIT) && cnt <= W_MAX_LEAF) {
                Q.a[j] = tri;
                Q.b[j] = cnt;
                Q.leaf[j] = c;
                s.I[c] = -1;
                s.D[c] = qd;
                leaves++;
                maxleaf = maxleaf > cnt ? maxleaf : cnt;
            } else {
                Q.a[j] = idx;
                Q.b[j] = 0;
                Q.leaf[j] = -1;
                s.I[c] = idx;
                s.D[c] = qd + 1;
            }
            idx += (int)s.W[c];
            tri += (int)s.T[c];
        };
        // 1-4 direct; 5-7: 3 direct + 1 group; 8: 2 direct + 2 groups of 3
        const int direct = cn <= W_WIDTH ? cn : (cn <= 7 ? 3 : 2);
        for (int k = 0; k < direct; k++)
            entry(c0 + k, P, P.nc++, dep);
        int rest = cn - direct, at = c0 + direct;
        const int groups = rest == 0 ? 0 : (cn <= 7 ? 1 : 2);
        for (int gi = 0; gi < groups; gi++) {
            const int gs = gi == groups - 1 ? rest : (rest + 1) / 2;
            const int gnode = idx++;
            QPlan G;
            G.nc = 0;
            G.oct = -1;
            G.runleaf = -1;
            G.depth = dep + 1;
            for (int j = 0; j < W_WIDTH; j++) {
                G.a[j] = G.b[j] = 0;
                G.leaf[j] = -1;
            }
            for (int k = 0; k < gs && k < W_WIDTH; k++)
                entry(at + k, G, G.nc++, dep + 1);
            if (gnode >= 0 && gnode < o.np) {
                o.plans[gnode] = G;
                note_plan(o, dep + 1);
            }
            const int j = P.nc++;
            P.a[j] = gnode;
            P.b[j] = 0;
            P.leaf[j] = -1;
            at += gs;
            rest -= gs;
        }
        if (me >= 0 && me < o.np) {
            o.plans[me] = P;
            note_plan(o, dep);
        }
    }
    if (leaves) {
        atomicAdd(&o.info->leaves, leaves);
        atomicMax(&o.info->max_leaf, maxleaf);
    }
}

// one thread: the depth lists' first positions
__global__ void wq_offsets_kernel(WQuickDevInfo* info)
{
    int at = 0;
    for (int d = 0; d < WQ_GPU_MAX_DEPTH; d++) {
        info->cursor[d] = at;
        at += info->depth_count[d];
    }
}

__global__ __launch_bounds__(BLOCK) void wq_bucket_kernel(const QPlan* __restrict__ plans, int np, int32_t* list,
                                                          WQuickDevInfo* info)
{
    const int w = blockIdx.x * BLOCK + threadIdx.x;
    if (w >= np)
        return;
    const int d = plans[w].depth;
    if (d < 0 || d >= WQ_GPU_MAX_DEPTH)
        return;
    const int at = atomicAdd(&info->cursor[d], 1);
    if (at >= 0 && at < np)
        list[at] = w;
}

// one lane per wide node of a depth: build_wbvh_quick's geometry loop
__global__ __launch_bounds__(GEOM_BLOCK) void wq_geom_kernel(const QPlan* __restrict__ plans, const int32_t* __restrict__ list,
                                                             int count, int np, const GNode* __restrict__ onodes,
                                                             const GTri* __restrict__ tris, const int32_t* __restrict__ slot,
                                                             WNode* wnodes, QChild* agg)
{
    const int q = blockIdx.x * GEOM_BLOCK + threadIdx.x;
    if (q >= count)
        return;
    const int w = list[q];
    if (w < 0 || w >= np)
        return;
    const QPlan P = plans[w];
    const int nc = P.nc < 0 ? 0 : (P.nc > W_WIDTH ? W_WIDTH : P.nc);
    QChild ch[W_WIDTH];
    for (int j = 0; j < nc; j++) {
        if (P.b[j] > 0) {
            q_from_tris(ch[j], tris, slot, P.a[j], P.b[j]);
            ch[j].link = W_LEAF | ((uint32_t)P.a[j] << 3) | (uint32_t)(P.b[j] - 1);
            ch[j].leaf = P.leaf[j];
        } else {
            const int c = P.a[j] >= 0 && P.a[j] < np ? P.a[j] : w;   // (always in range: the plan's own indices)
            ch[j] = agg[c];
            ch[j].link = (uint32_t)P.a[j];
        }
    }
    wnodes[w] = q_node(ch, nc, onodes);
    // the node's entry in its parent holds the axis boxes of the octree leaves below (wbvh.cpp)
    Box ax = empty_box();
    auto axis = [&](int32_t u) {
        const GNode& g = onodes[u];
        Box b;
        for (int a = 0; a < 3; a++) {
            b.lo[a] = g.dn[a];
            b.hi[a] = g.df[a];
        }
        grow(ax, b);
    };
    if (P.oct >= 0)
        axis(P.oct);
    for (int j = 0; j < nc; j++)
        if (P.b[j] > 0 && P.leaf[j] >= 0)
            axis(P.leaf[j]);
    QChild me;
    q_combine(me, ch, nc, &ax);
    me.leaf = P.runleaf;
    me.link = W_EMPTY;
    agg[w] = me;
}

__global__ __launch_bounds__(BLOCK) void wq_links_kernel(const WNode* __restrict__ wnodes, int np, int nt,
                                                         uint32_t* tri_leaf, uint32_t* parent)
{
    const int w = blockIdx.x * BLOCK + threadIdx.x;
    if (w >= np)
        return;
    if (w == 0)
        parent[0] = W_EMPTY;
    for (int j = 0; j < W_WIDTH; j++) {
        const uint32_t c = wnodes[w].child[j];
        const uint32_t e = (uint32_t)w << 2 | (uint32_t)j;
        if (c == W_EMPTY)
            continue;
        if (c & W_LEAF) {
            const uint32_t first = (c >> 3) & 0x0FFFFFFFu, cnt = (c & 7u) + 1u;
            for (uint32_t k = first; k < first + cnt; k++)
                if (k < (uint32_t)nt)
                    tri_leaf[k] = e;
        } else if (c < (uint32_t)np)
            parent[c] = e;
    }
}

unsigned blocks(int64_t n, int per_block = BLOCK) { return (unsigned)((n + per_block - 1) / per_block); }

}  // namespace

WQuickGpuScratch::~WQuickGpuScratch()
{
    if (pinned)
        (void)hipHostFree(pinned);
}

bool wbvh_quick_device_supported(int64_t n, int max_depth)
{
    return octree_device_supported(n, max_depth) && n < ((int64_t)1 << 28);
}

int build_wbvh_quick_device(WQuickGpuScratch& S, const GNode* d_nodes, const GTri* d_tris, const OctreeDevInfo& oi,
                            DevBuf& wnodes, DevBuf& tmp, DevBuf& links, int64_t stats[5], hipStream_t stream,
                            hipError_t* err)
{
    *err = hipSuccess;
    for (int k = 0; k < 5; k++) stats[k] = 0;
    const int64_t nn64 = oi.nodes, nt64 = oi.tris;
    const int levels = oi.levels;
    if (nn64 == 0 || nt64 == 0)
        return OCT_GPU_OK;   // the empty tree: nothing to launch
    if (nn64 < 0 || nn64 > (1ll << 26) || nt64 < 0 || nt64 > OCT_GPU_MAX_TRIS || levels < 1 ||
        levels > OCT_GPU_MAX_DEPTH + 1 || oi.level_base[0] != 0 || oi.level_base[levels] != nn64)
        return OCT_GPU_UNSUPPORTED;
    for (int d = 0; d < levels; d++)
        if (oi.level_base[d + 1] < oi.level_base[d])
            return OCT_GPU_UNSUPPORTED;
    const int nn = (int)nn64, nt = (int)nt64;
    hipError_t e = hipSuccess;
#define WQ_CK(x)                       \
    do {                               \
        if ((e = (x)) != hipSuccess) { \
            *err = e;                  \
            return OCT_GPU_HIP;        \
        }                              \
    } while (0)
#define WQ_LAUNCHED() WQ_CK(hipGetLastError())

    // RT_BUILD_PROFILE: the passes' times on stderr (the stream is drained after each pass)
    const bool prof = std::getenv("RT_BUILD_PROFILE") != nullptr;
    auto tick = std::chrono::steady_clock::now();
    auto phase = [&](const char* what) {
        if (!prof)
            return hipSuccess;
        const hipError_t pe = hipStreamSynchronize(stream);
        auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[wbvh quick gpu] %-10s %8.3f ms\n", what, std::chrono::duration<double, std::milli>(now - tick).count());
        tick = now;
        return pe;
    };
    if (!S.pinned)
        WQ_CK(hipHostMalloc(&S.pinned, sizeof(WQuickDevInfo), hipHostMallocDefault));
    WQ_CK(S.sub.reserve((size_t)nn * 20));
    WQ_CK(S.info.reserve(sizeof(WQuickDevInfo)));
    Sub sub;
    sub.W = S.sub.as<uint32_t>();
    sub.T = sub.W + nn;
    sub.I = reinterpret_cast<int32_t*>(sub.T + nn);
    sub.F = sub.I + nn;
    sub.D = sub.F + nn;
    WQuickDevInfo* d_info = S.info.as<WQuickDevInfo>();
    WQ_CK(hipMemsetAsync(d_info, 0, sizeof(WQuickDevInfo), stream));
    // sizes, deepest level first
    for (int d = levels - 1; d >= 0; d--) {
        const int base = oi.level_base[d], count = oi.level_base[d + 1] - base;
        if (count <= 0)
            continue;
        wq_sizes_kernel<<<blocks(count), BLOCK, 0, stream>>>(d_nodes, base, count, nn, sub);
        WQ_LAUNCHED();
    }
    uint32_t* pin = static_cast<uint32_t*>(S.pinned);
    WQ_CK(hipMemcpyAsync(pin, sub.W, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    WQ_CK(hipMemcpyAsync(pin + 1, sub.T, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    WQ_CK(hipStreamSynchronize(stream));   // the first readback: the tree's node count
    WQ_CK(phase("sizes"));
    const int64_t np64 = pin[0];
    if (pin[1] != (uint32_t)nt || np64 < 1 || np64 > 2 * nt64 + 2)
        return OCT_GPU_UNSUPPORTED;   // (never: every slot lies in one leaf, and a node has a run or two nodes below)
    const int np = (int)np64;
    WQ_CK(S.plans.reserve((size_t)np * sizeof(QPlan)));
    WQ_CK(S.agg.reserve((size_t)np * sizeof(QChild)));
    WQ_CK(S.list.reserve((size_t)np * 4));
    WQ_CK(wnodes.reserve((size_t)np * sizeof(WNode)));
    // the arrays inside tmp and links (wide_layout.hpp)
    const size_t lnn = (size_t)np, lnt = (size_t)nt;
    WQ_CK(tmp.reserve(wide_tmp_bytes(lnn, lnt)));
    WQ_CK(links.reserve(wide_links_bytes(lnn, lnt)));
    uint32_t* const tri_leaf = reinterpret_cast<uint32_t*>(links.as<char>() + wide_links_tri_leaf_off(lnn, lnt));
    uint32_t* const parent = reinterpret_cast<uint32_t*>(links.as<char>() + wide_links_parent_off(lnn, lnt));
    PlanOut po;
    po.plans = S.plans.as<QPlan>();
    po.np = np;
    po.slot = reinterpret_cast<int32_t*>(tmp.as<char>() + wide_tmp_slot_off(lnn, lnt));
    po.leaf_of_slot = reinterpret_cast<uint32_t*>(tmp.as<char>() + wide_tmp_leaf_of_slot_off(lnn, lnt));
    po.nt = nt;
    po.info = d_info;
    // plans, top level first
    for (int d = 0; d < levels; d++) {
        const int base = oi.level_base[d], count = oi.level_base[d + 1] - base;
        if (count <= 0)
            continue;
        wq_plan_kernel<<<blocks(count), BLOCK, 0, stream>>>(d_nodes, base, count, nn, sub, po);
        WQ_LAUNCHED();
    }
    wq_offsets_kernel<<<1, 1, 0, stream>>>(d_info);
    WQ_LAUNCHED();
    WQuickDevInfo* hi = static_cast<WQuickDevInfo*>(S.pinned);
    WQ_CK(hipMemcpyAsync(hi, d_info, sizeof(WQuickDevInfo), hipMemcpyDeviceToHost, stream));
    WQ_CK(hipStreamSynchronize(stream));   // the second readback: the nodes per depth
    WQ_CK(phase("plan"));
    if (hi->max_depth < 0 || hi->max_depth >= WQ_GPU_MAX_DEPTH)
        return OCT_GPU_UNSUPPORTED;
    int64_t total = 0;
    int32_t off[WQ_GPU_MAX_DEPTH], cnt[WQ_GPU_MAX_DEPTH];
    for (int d = 0; d < WQ_GPU_MAX_DEPTH; d++) {
        off[d] = hi->cursor[d];
        cnt[d] = hi->depth_count[d];
        if (cnt[d] < 0 || off[d] != total) {
            *err = hipErrorUnknown;
            return OCT_GPU_HIP;
        }
        total += cnt[d];
    }
    if (total != np) {   // (never: every wide node was planned once)
        *err = hipErrorUnknown;
        return OCT_GPU_HIP;
    }
    const int maxd = hi->max_depth;
    stats[0] = np;
    stats[1] = hi->leaves;
    stats[2] = nt;
    stats[3] = hi->max_leaf;
    stats[4] = maxd + 1;
    wq_bucket_kernel<<<blocks(np), BLOCK, 0, stream>>>(po.plans, np, S.list.as<int32_t>(), d_info);
    WQ_LAUNCHED();
    // geometry, deepest nodes first
    for (int d = maxd; d >= 0; d--) {
        if (cnt[d] <= 0)
            continue;
        wq_geom_kernel<<<blocks(cnt[d], GEOM_BLOCK), GEOM_BLOCK, 0, stream>>>(
            po.plans, S.list.as<int32_t>() + off[d], cnt[d], np, d_nodes, d_tris, po.slot, wnodes.as<WNode>(),
            S.agg.as<QChild>());
        WQ_LAUNCHED();
    }
    WQ_CK(phase("geometry"));
    wq_links_kernel<<<blocks(np), BLOCK, 0, stream>>>(wnodes.as<WNode>(), np, nt, tri_leaf, parent);
    WQ_LAUNCHED();
    WQ_CK(hipStreamSynchronize(stream));
    WQ_CK(phase("links"));
#undef WQ_CK
#undef WQ_LAUNCHED
    return OCT_GPU_OK;
}

}  // namespace rt
