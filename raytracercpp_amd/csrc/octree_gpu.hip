// octree_gpu.hip -- see octree_gpu.hpp.  octree.cpp states the build's closed form: a node at depth d
// holding c triangles is inner iff c > leaf and d != max_depth, each child gets its parent's
// triangles in insertion order, and the flatten is level order with empty leaves dropped.  Here every
// level is one pass over the items still above a leaf:
//   classify  a node is inner / kept / leaf from its count; one exclusive scan gives each node its
//             rank among the level's inner nodes (its 8 children in the next level), its flat index
//             and its leaves' first triangle slot (level order: the serial flatten's BFS sequence)
//   leaf      one wave per leaf folds the triangles' k-DOP slabs in slot order and writes the
//             GTri / tri_id records
//   route     an item's key in the next level: 8 x the parent's inner rank + octant (c > centre)
//   sort      a stable radix sort on that key: triangles keep their insertion order inside a node
//   children  the next level's nodes: create_children's boxes, their ranges by binary search
// and the inner volumes are folded bottom-up over each node's kept children in octant order.
// Every float expression is the host's (rt_math.hpp, -ffp-contract=off); smin / smax keep the first
// operand on a tie and are associative, so the ordered wave reduction below gives the serial fold's
// bytes, signed zeros included.  No float atomics, no cross-block waits: the host reads two counts
// back per level (inner nodes, items left) and sizes the next level's launches with them.
#include "octree_gpu.hpp"

#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>

namespace rt {

namespace {

constexpr int BLOCK = 256;
constexpr int WAVE = 64;

struct DNode {   // OctreeNode::_min / _max and its items [begin, end) of the level's item arrays
    int32_t begin, end;
    float mn[3], mx[3];
};

struct S3 {
    int32_t inner, kept, ltris;
};
struct S3Sum {
    __host__ __device__ S3 operator()(const S3& a, const S3& b) const
    {
        return S3{a.inner + b.inner, a.kept + b.kept, a.ltris + b.ltris};
    }
};

struct Box {
    float v[6];   // min xyz, max xyz
};

__device__ inline Box box_join(const Box& a, const Box& b)
{
    Box r;
    for (int k = 0; k < 3; k++) {
        r.v[k] = smin(a.v[k], b.v[k]);
        r.v[3 + k] = smax(a.v[3 + k], b.v[3 + k]);
    }
    return r;
}

// the block's boxes joined (any order: the root box's zero signs never reach the output)
__device__ inline Box block_box(Box b, Box* lds)
{
    lds[threadIdx.x] = b;
    __syncthreads();
    for (int s = BLOCK / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            lds[threadIdx.x] = box_join(lds[threadIdx.x], lds[threadIdx.x + s]);
        __syncthreads();
    }
    return lds[0];
}

__device__ inline Box empty_box()
{
    return Box{{INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY}};
}

// prep_triangles (octree.cpp): Triangle::bbox_centroid and the root box's partial per block
__global__ __launch_bounds__(BLOCK) void oct_prep_kernel(const float* __restrict__ tri9, int n, float* cx, float* cy,
                                                         float* cz, int32_t* tid, uint32_t* key, Box* partial)
{
    __shared__ Box lds[BLOCK];
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    Box b = empty_box();
    if (t < n) {
        const float* p = tri9 + 9 * (size_t)t;
        v3 v[3];
        for (int k = 0; k < 3; k++) v[k] = mk(p[3 * k], p[3 * k + 1], p[3 * k + 2]);
        v3 lo = mk(smin(v[0].x, smin(v[1].x, v[2].x)), smin(v[0].y, smin(v[1].y, v[2].y)),
                   smin(v[0].z, smin(v[1].z, v[2].z)));
        v3 hi = mk(smax(v[0].x, smax(v[1].x, v[2].x)), smax(v[0].y, smax(v[1].y, v[2].y)),
                   smax(v[0].z, smax(v[1].z, v[2].z)));
        float kk = 1.f / 2;   // Point / float, vec.cpp:56-60
        v3 c = kk * (lo + hi);
        cx[t] = c.x;
        cy[t] = c.y;
        cz[t] = c.z;
        tid[t] = t;
        key[t] = 0;   // every item starts in the root
        b = Box{{lo.x, lo.y, lo.z, hi.x, hi.y, hi.z}};
    }
    b = block_box(b, lds);
    if (threadIdx.x == 0)
        partial[blockIdx.x] = b;
}

// one block: the root node and the zeroed totals
__global__ __launch_bounds__(BLOCK) void oct_root_kernel(const Box* partial, int nblocks, int n, DNode* root,
                                                         OctreeDevInfo* info)
{
    __shared__ Box lds[BLOCK];
    Box b = empty_box();
    for (int j = threadIdx.x; j < nblocks; j += BLOCK) b = box_join(b, partial[j]);
    b = block_box(b, lds);
    if (threadIdx.x == 0) {
        DNode r;
        r.begin = 0;
        r.end = n;
        for (int k = 0; k < 3; k++) {
            r.mn[k] = b.v[k];
            r.mx[k] = b.v[3 + k];
        }
        *root = r;
        for (int k = 0; k < 6; k++) info->stats[k] = 0;
        info->levels = 0;
        info->ordered_slabs = 1;
        info->nodes = info->tris = 0;
        for (int k = 0; k < OCT_GPU_MAX_DEPTH + 3; k++) info->level_base[k] = info->slot_base[k] = 0;
        info->next[0] = info->next[1] = 0;
        info->max_leaf = 0;
    }
}

// OctreeNode::insert's split rule in closed form (octree.cpp build_flat_octree)
__global__ __launch_bounds__(BLOCK) void oct_classify_kernel(const DNode* nodes, int N, int d, int max_depth,
                                                             unsigned long long lim, S3* flags, OctreeDevInfo* info)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= N)
        return;
    const int cnt = nodes[i].end - nodes[i].begin;
    const bool leaf = !((unsigned long long)(long long)cnt > lim && d != max_depth);
    S3 f;
    f.inner = leaf ? 0 : 1;
    f.kept = (leaf && cnt == 0) ? 0 : 1;
    f.ltris = leaf ? cnt : 0;
    flags[i] = f;
    if (leaf && cnt > 0)
        atomicMax(&info->max_leaf, cnt);   // (an integer maximum: the same in any order)
}

// one thread: the level's totals into the running ones
__global__ void oct_level_kernel(const S3* flags, const S3* ranks, int N, int m, int d, OctreeDevInfo* info)
{
    const S3 tot = S3Sum()(ranks[N - 1], flags[N - 1]);
    info->next[0] = tot.inner;
    info->next[1] = m - tot.ltris;
    info->level_base[d + 1] = info->level_base[d] + tot.kept;
    info->slot_base[d + 1] = info->slot_base[d] + tot.ltris;
    info->stats[0] += tot.inner;
    info->stats[1] += N - tot.inner;
    info->stats[2] += N - tot.kept;
    info->stats[4] = d;
    if (tot.kept > 0)
        info->levels = d + 1;
}

// an inner node's a / b words, by its group of 8 children once they are classified
__global__ __launch_bounds__(BLOCK) void oct_link_kernel(const S3* flags, const S3* ranks, int ngroups, int d,
                                                         const int32_t* parent_flat, const OctreeDevInfo* info,
                                                         GNode* out)
{
    const int g = blockIdx.x * BLOCK + threadIdx.x;
    if (g >= ngroups)
        return;
    int first = -1;
    uint32_t k = 0;
    for (int o = 0; o < 8; o++) {
        const int i = 8 * g + o;
        if (flags[i].kept) {
            if (first < 0)
                first = info->level_base[d] + ranks[i].kept;
            k++;
        }
    }
    GNode& p = out[parent_flat[g]];
    p.a = (uint32_t)first;
    p.b = k;
}

// One wave per node.  A kept leaf: compute_volume's fold over its triangles in slot order
// (BoundingVolume::triangle_volume per triangle), make_gtri and the slot map.  An inner node:
// its children's group tables.
__global__ __launch_bounds__(BLOCK) void oct_leaf_kernel(const DNode* nodes, const S3* flags, const S3* ranks, int N,
                                                         int d, const float* __restrict__ tri9, const int32_t* tid,
                                                         const OctreeDevInfo* info, GNode* out, GTri* tris,
                                                         int32_t* tri_id, int32_t* inner_node, int32_t* parent_flat)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int i = blockIdx.x * (BLOCK / WAVE) + (threadIdx.x / WAVE);
    if (i >= N)
        return;
    const S3 f = flags[i], r = ranks[i];
    if (!f.kept)
        return;
    const int flat = info->level_base[d] + r.kept;
    if (f.inner) {
        if (lane == 0) {
            inner_node[r.inner] = i;
            parent_flat[r.inner] = flat;
        }
        return;
    }
    const int begin = nodes[i].begin, cnt = nodes[i].end - nodes[i].begin;
    const int s0 = info->slot_base[d] + r.ltris;
    float dn[NPLANES], df[NPLANES];
    for (int p = 0; p < NPLANES; p++) {
        dn[p] = INFINITY;
        df[p] = -INFINITY;
    }
    for (int k0 = 0; k0 < cnt; k0 += WAVE) {
        const int k = k0 + lane;
        float tn[NPLANES], tf[NPLANES];
        for (int p = 0; p < NPLANES; p++) {
            tn[p] = INFINITY;
            tf[p] = -INFINITY;
        }
        if (k < cnt) {
            const int t = tid[begin + k];
            const float* q = tri9 + 9 * (size_t)t;
            v3 v[3];
            for (int j = 0; j < 3; j++) v[j] = mk(q[3 * j], q[3 * j + 1], q[3 * j + 2]);
            for (int p = 0; p < NPLANES; p++) {
                const v3 pn = mk(PLANE_N[p][0], PLANE_N[p][1], PLANE_N[p][2]);
                for (int j = 0; j < 3; j++) {
                    float dist = dot(pn, v[j]);
                    tn[p] = smin(tn[p], dist);
                    tf[p] = smax(tf[p], dist);
                }
            }
            // make_gtri (octree.cpp)
            v3 ab = v[1] - v[0];
            v3 ac = v[2] - v[0];
            v3 nn = cross(v[1] - v[0], v[2] - v[0]);
            GTri gt;
            gt.a[0] = v[0].x; gt.a[1] = v[0].y; gt.a[2] = v[0].z;
            gt.ab[0] = ab.x; gt.ab[1] = ab.y; gt.ab[2] = ab.z;
            gt.ac[0] = ac.x; gt.ac[1] = ac.y; gt.ac[2] = ac.z;
            gt.n[0] = nn.x; gt.n[1] = nn.y; gt.n[2] = nn.z;
            tris[s0 + k] = gt;
            tri_id[s0 + k] = t;
        }
        // ordered tree reduction: lane l joins [l, l + off) with [l + off, l + 2 off), the lower
        // slots as the first operand; lanes past the leaf's end hold the fold's identity
        for (int off = 1; off < WAVE; off <<= 1)
            for (int p = 0; p < NPLANES; p++) {
                float on = __shfl_down(tn[p], off, WAVE), of = __shfl_down(tf[p], off, WAVE);
                if (lane + off < WAVE) {
                    tn[p] = smin(tn[p], on);
                    tf[p] = smax(tf[p], of);
                }
            }
        for (int p = 0; p < NPLANES; p++) {
            dn[p] = smin(dn[p], tn[p]);
            df[p] = smax(df[p], tf[p]);
        }
    }
    if (lane == 0) {
        GNode g;
        for (int p = 0; p < NPLANES; p++) {
            g.dn[p] = dn[p];
            g.df[p] = df[p];
        }
        g.a = (uint32_t)s0;
        g.b = LEAF_BIT | (uint32_t)cnt;
        out[flat] = g;
    }
}

// insert_to_children (bvh.h:195-210): the octant of the bbox centroid against the cell centre
__global__ __launch_bounds__(BLOCK) void oct_route_kernel(const DNode* nodes, const S3* flags, const S3* ranks, int m,
                                                          int ninner, const float* cx, const float* cy,
                                                          const float* cz, const uint32_t* key, uint32_t* key_out,
                                                          int32_t* pos)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= m)
        return;
    const uint32_t node = key[i];
    uint32_t k = 8u * (uint32_t)ninner;   // in a leaf: sorted behind every item that moves on
    if (flags[node].inner) {
        const DNode nd = nodes[node];
        float ccx = (nd.mn[0] + nd.mx[0]) / 2;
        float ccy = (nd.mn[1] + nd.mx[1]) / 2;
        float ccz = (nd.mn[2] + nd.mx[2]) / 2;
        int oct = 0;
        if (cx[i] > ccx) oct += 1;
        if (cy[i] > ccy) oct += 2;
        if (cz[i] > ccz) oct += 4;
        k = 8u * (uint32_t)ranks[node].inner + (uint32_t)oct;
    }
    key_out[i] = k;
    pos[i] = i;
}

__global__ __launch_bounds__(BLOCK) void oct_gather_kernel(const int32_t* pos, int m, const float* cx, const float* cy,
                                                           const float* cz, const int32_t* tid, float* ox, float* oy,
                                                           float* oz, int32_t* otid)
{
    const int j = blockIdx.x * BLOCK + threadIdx.x;
    if (j >= m)
        return;
    const int s = pos[j];
    ox[j] = cx[s];
    oy[j] = cy[s];
    oz[j] = cz[s];
    otid[j] = tid[s];
}

__device__ inline int lower_bound_key(const uint32_t* key, int m, uint32_t c)
{
    int lo = 0, hi = m;
    for (int it = 0; it < 32 && lo < hi; it++) {
        const int mid = lo + (hi - lo) / 2;
        if (key[mid] < c)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// OctreeNode::create_children, bvh.h:153-167 (children 2 / 4 / 6 from _min + Point(...)), and the
// child's items: the sorted keys equal to its index
__global__ __launch_bounds__(BLOCK) void oct_children_kernel(const DNode* nodes, const int32_t* inner_node, int nchild,
                                                             const uint32_t* key, int m, DNode* next)
{
    const int c = blockIdx.x * BLOCK + threadIdx.x;
    if (c >= nchild)
        return;
    const DNode nd = nodes[inner_node[c >> 3]];
    const int o = c & 7;
    v3 mn = mk(nd.mn[0], nd.mn[1], nd.mn[2]), mx = mk(nd.mx[0], nd.mx[1], nd.mx[2]);
    float cx = (mn.x + mx.x) / 2;
    float cy = (mn.y + mx.y) / 2;
    float cz = (mn.z + mx.z) / 2;
    v3 lo, hi;
    switch (o) {
    case 0: lo = mn;                   hi = mk(cx, cy, cz);       break;
    case 1: lo = mk(cx, mn.y, mn.z);   hi = mk(mx.x, cy, cz);     break;
    case 2: lo = mn + mk(0, cy, 0);    hi = mk(cx, mx.y, cz);     break;
    case 3: lo = mk(cx, cy, mn.z);     hi = mk(mx.x, mx.y, cz);   break;
    case 4: lo = mn + mk(0, 0, cz);    hi = mk(cx, cy, mx.z);     break;
    case 5: lo = mk(cx, mn.y, cz);     hi = mk(mx.x, cy, mx.z);   break;
    case 6: lo = mn + mk(0, cy, cz);   hi = mk(cx, mx.y, mx.z);   break;
    default: lo = mk(cx, cy, cz);      hi = mk(mx.x, mx.y, mx.z); break;
    }
    DNode ch;
    ch.begin = lower_bound_key(key, m, (uint32_t)c);
    ch.end = lower_bound_key(key, m, (uint32_t)c + 1u);
    ch.mn[0] = lo.x; ch.mn[1] = lo.y; ch.mn[2] = lo.z;
    ch.mx[0] = hi.x; ch.mx[1] = hi.y; ch.mx[2] = hi.z;
    next[c] = ch;
}

// compute_volume (bvh.h:141-151) of a level's inner nodes: the fold over the kept children in
// octant order (an empty child's +inf / -inf never changes the fold).  16 lanes per node, one
// per slab distance.
__global__ __launch_bounds__(BLOCK) void oct_inner_kernel(GNode* out, int d, int bound, const OctreeDevInfo* info)
{
    const int t = blockIdx.x * BLOCK + threadIdx.x;
    const int i = t >> 4, j = t & 15;
    if (i >= bound || i >= info->level_base[d + 1] - info->level_base[d] || j >= 2 * NPLANES)
        return;
    GNode& g = out[info->level_base[d] + i];
    if (g.b & LEAF_BIT)
        return;
    const uint32_t nk = g.b < 8u ? g.b : 8u;
    const bool nearp = j < NPLANES;
    float acc = nearp ? INFINITY : -INFINITY;
    for (uint32_t k = 0; k < nk; k++) {
        const float v = reinterpret_cast<const float*>(&out[g.a + k])[j];
        acc = nearp ? smin(acc, v) : smax(acc, v);
    }
    reinterpret_cast<float*>(&g)[j] = acc;
}

// finish_checks (octree.cpp) and the last totals
__global__ __launch_bounds__(BLOCK) void oct_check_kernel(const GNode* out, int bound, int levels_built,
                                                          OctreeDevInfo* info)
{
    const int f = blockIdx.x * BLOCK + threadIdx.x;
    const int nn = info->level_base[levels_built];
    if (f == 0) {
        info->nodes = nn;
        info->tris = info->slot_base[levels_built];
        info->stats[3] = info->max_leaf;
        info->stats[5] = 1 + 8 * info->stats[0];
    }
    if (f >= bound || f >= nn)
        return;
    bool ok = true;
    for (int p = 0; p < NPLANES; p++)
        if (!(out[f].dn[p] <= out[f].df[p]))
            ok = false;
    if (!ok)
        info->ordered_slabs = 0;   // (every writer stores the same value)
}

unsigned blocks(int64_t n, int per_block = BLOCK) { return (unsigned)((n + per_block - 1) / per_block); }

// grows b to 'need' bytes keeping its first 'keep' bytes (work queued on 'stream' may still write them)
hipError_t grow_keep(DevBuf& b, size_t need, size_t keep, hipStream_t stream)
{
    if (b.p && need <= b.bytes)
        return hipSuccess;
    DevBuf nb;
    hipError_t e = nb.reserve(std::max(need, 2 * b.bytes));
    if (e == hipSuccess && keep && b.p)
        e = hipMemcpyAsync(nb.p, b.p, keep, hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess)
        e = hipStreamSynchronize(stream);
    if (e == hipSuccess)
        b.swap(nb);
    return e;
}

}  // namespace

OctreeGpuScratch::~OctreeGpuScratch()
{
    if (pinned)
        (void)hipHostFree(pinned);
}

bool octree_device_supported(int64_t n, int max_depth)
{
    return n >= 0 && n <= OCT_GPU_MAX_TRIS && max_depth >= 0 && max_depth <= OCT_GPU_MAX_DEPTH;
}

int build_flat_octree_device(OctreeGpuScratch& S, const float* d_tri9, int64_t n64, int max_depth,
                             int leaf_max_obj_count, DevBuf& nodes, DevBuf& tris, DevBuf& tri_id,
                             OctreeDevInfo* d_info, OctreeDevInfo* h_info, hipStream_t stream, hipError_t* err)
{
    *err = hipSuccess;
    if (!octree_device_supported(n64, max_depth))
        return OCT_GPU_UNSUPPORTED;
    *h_info = OctreeDevInfo();
    h_info->ordered_slabs = 1;
    if (n64 == 0)
        return OCT_GPU_OK;   // the empty tree: nothing to launch
    const int n = (int)n64;
    const unsigned long long lim = (unsigned long long)(size_t)(long)leaf_max_obj_count;   // bvh.h:181
    hipError_t e = hipSuccess;
#define OCT_CK(x)                 \
    do {                          \
        if ((e = (x)) != hipSuccess) { \
            *err = e;             \
            return OCT_GPU_HIP;   \
        }                         \
    } while (0)
#define OCT_LAUNCHED() OCT_CK(hipGetLastError())

    if (!S.pinned)
        OCT_CK(hipHostMalloc(&S.pinned, 2 * sizeof(int32_t), hipHostMallocDefault));
    for (int k = 0; k < 2; k++) {
        OCT_CK(S.cx[k].reserve((size_t)n * 4));
        OCT_CK(S.cy[k].reserve((size_t)n * 4));
        OCT_CK(S.cz[k].reserve((size_t)n * 4));
        OCT_CK(S.tid[k].reserve((size_t)n * 4));
        OCT_CK(S.key[k].reserve((size_t)n * 4));
        OCT_CK(S.pos[k].reserve((size_t)n * 4));
    }
    OCT_CK(tris.reserve((size_t)n * sizeof(GTri)));
    OCT_CK(tri_id.reserve((size_t)n * 4));
    const unsigned pb = blocks(n);
    OCT_CK(S.partial.reserve((size_t)pb * sizeof(Box)));
    OCT_CK(S.lnodes[0].reserve(sizeof(DNode)));

    int cur = 0;    // the item arrays and keys of the current level
    int ln = 0;     // its nodes
    oct_prep_kernel<<<pb, BLOCK, 0, stream>>>(d_tri9, n, S.cx[0].as<float>(), S.cy[0].as<float>(), S.cz[0].as<float>(),
                                              S.tid[0].as<int32_t>(), S.key[0].as<uint32_t>(), S.partial.as<Box>());
    OCT_LAUNCHED();
    oct_root_kernel<<<1, BLOCK, 0, stream>>>(S.partial.as<Box>(), (int)pb, n, S.lnodes[0].as<DNode>(), d_info);
    OCT_LAUNCHED();

    int64_t N = 1;          // nodes of the level
    int m = n;              // items in them
    int64_t bound = 0;      // flat nodes of the levels above: at most their nodes
    int level_nodes[OCT_GPU_MAX_DEPTH + 2];
    int levels_built = 0;
    for (int d = 0; d <= max_depth; d++) {
        if (bound + N > (1ll << 26))   // (flat indices and launch sizes stay in 32 bits; the caller builds on the host)
            return OCT_GPU_UNSUPPORTED;
        // the level keeps at most its N nodes
        OCT_CK(grow_keep(nodes, (size_t)(bound + N) * sizeof(GNode), (size_t)bound * sizeof(GNode), stream));
        OCT_CK(S.flags.reserve((size_t)N * sizeof(S3)));
        OCT_CK(S.ranks.reserve((size_t)N * sizeof(S3)));
        OCT_CK(S.inner_node.reserve((size_t)N * 4));
        OCT_CK(S.parent_flat[d & 1].reserve((size_t)N * 4));
        const DNode* lv = S.lnodes[ln].as<DNode>();
        S3* flags = S.flags.as<S3>();
        S3* ranks = S.ranks.as<S3>();
        oct_classify_kernel<<<blocks(N), BLOCK, 0, stream>>>(lv, (int)N, d, max_depth, lim, flags, d_info);
        OCT_LAUNCHED();
        size_t tb = 0;
        OCT_CK(hipcub::DeviceScan::ExclusiveScan(nullptr, tb, flags, ranks, S3Sum(), S3{0, 0, 0}, (int)N, stream));
        OCT_CK(S.tmp.reserve(tb));
        OCT_CK(hipcub::DeviceScan::ExclusiveScan(S.tmp.p, tb, flags, ranks, S3Sum(), S3{0, 0, 0}, (int)N, stream));
        oct_level_kernel<<<1, 1, 0, stream>>>(flags, ranks, (int)N, m, d, d_info);
        OCT_LAUNCHED();
        OCT_CK(hipMemcpyAsync(S.pinned, d_info->next, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        if (d > 0) {
            oct_link_kernel<<<blocks(N / 8), BLOCK, 0, stream>>>(flags, ranks, (int)(N / 8), d,
                                                                 S.parent_flat[(d - 1) & 1].as<int32_t>(), d_info,
                                                                 nodes.as<GNode>());
            OCT_LAUNCHED();
        }
        oct_leaf_kernel<<<blocks(N, BLOCK / WAVE), BLOCK, 0, stream>>>(
            lv, flags, ranks, (int)N, d, d_tri9, S.tid[cur].as<int32_t>(), d_info, nodes.as<GNode>(), tris.as<GTri>(),
            tri_id.as<int32_t>(), S.inner_node.as<int32_t>(), S.parent_flat[d & 1].as<int32_t>());
        OCT_LAUNCHED();
        OCT_CK(hipStreamSynchronize(stream));   // the level's one readback
        const int ninner = static_cast<const int32_t*>(S.pinned)[0];
        const int mnext = static_cast<const int32_t*>(S.pinned)[1];
        level_nodes[d] = (int)N;
        levels_built = d + 1;
        bound += N;
        if (ninner <= 0)
            break;
        if (ninner > N || mnext <= 0 || mnext > m || d == max_depth) {   // (never: the counts are sums over this level)
            *err = hipErrorUnknown;
            return OCT_GPU_HIP;
        }
        const int64_t nchild = 8ll * ninner;
        oct_route_kernel<<<blocks(m), BLOCK, 0, stream>>>(lv, flags, ranks, m, ninner, S.cx[cur].as<float>(),
                                                          S.cy[cur].as<float>(), S.cz[cur].as<float>(),
                                                          S.key[cur].as<uint32_t>(), S.key[cur ^ 1].as<uint32_t>(),
                                                          S.pos[0].as<int32_t>());
        OCT_LAUNCHED();
        int bits = 1;
        while ((nchild >> bits) != 0) bits++;   // keys 0 .. nchild
        // stable: a node's items keep their order (key[cur] is free: the sorted keys go there)
        OCT_CK(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, S.key[cur ^ 1].as<uint32_t>(), S.key[cur].as<uint32_t>(),
                                                  S.pos[0].as<int32_t>(), S.pos[1].as<int32_t>(), m, 0, bits, stream));
        OCT_CK(S.tmp.reserve(tb));
        OCT_CK(hipcub::DeviceRadixSort::SortPairs(S.tmp.p, tb, S.key[cur ^ 1].as<uint32_t>(), S.key[cur].as<uint32_t>(),
                                                  S.pos[0].as<int32_t>(), S.pos[1].as<int32_t>(), m, 0, bits, stream));
        oct_gather_kernel<<<blocks(mnext), BLOCK, 0, stream>>>(
            S.pos[1].as<int32_t>(), mnext, S.cx[cur].as<float>(), S.cy[cur].as<float>(), S.cz[cur].as<float>(),
            S.tid[cur].as<int32_t>(), S.cx[cur ^ 1].as<float>(), S.cy[cur ^ 1].as<float>(), S.cz[cur ^ 1].as<float>(),
            S.tid[cur ^ 1].as<int32_t>());
        OCT_LAUNCHED();
        OCT_CK(S.lnodes[ln ^ 1].reserve((size_t)nchild * sizeof(DNode)));
        oct_children_kernel<<<blocks(nchild), BLOCK, 0, stream>>>(lv, S.inner_node.as<int32_t>(), (int)nchild,
                                                                  S.key[cur].as<uint32_t>(), mnext,
                                                                  S.lnodes[ln ^ 1].as<DNode>());
        OCT_LAUNCHED();
        // the sorted keys are in key[cur]; the gathered items in the other arrays: move the keys over
        // by exchanging the two key buffers, so that index cur ^ 1 holds the whole next level
        S.key[0].swap(S.key[1]);
        cur ^= 1;
        ln ^= 1;
        N = nchild;
        m = mnext;
    }
    // the inner volumes, bottom-up (the deepest level holds leaves only)
    for (int d = levels_built - 2; d >= 0; d--) {
        oct_inner_kernel<<<blocks(16ll * level_nodes[d]), BLOCK, 0, stream>>>(nodes.as<GNode>(), d, level_nodes[d],
                                                                              d_info);
        OCT_LAUNCHED();
    }
    oct_check_kernel<<<blocks(bound), BLOCK, 0, stream>>>(nodes.as<GNode>(), (int)bound, levels_built, d_info);
    OCT_LAUNCHED();
    OCT_CK(hipMemcpyAsync(h_info, d_info, sizeof(OctreeDevInfo), hipMemcpyDeviceToHost, stream));
    OCT_CK(hipStreamSynchronize(stream));
#undef OCT_CK
#undef OCT_LAUNCHED
    return OCT_GPU_OK;
}

}  // namespace rt
