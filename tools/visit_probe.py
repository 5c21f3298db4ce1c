"""Host probe of the wide query's work on a frame's rays (rt_wbvh_query_ex, no GPU): wide-node visits
per primary ray (the camera's risk words) and per shadow ray (the light's), their tail, and the
costliest 8x8 tiles' longest rays.  With RT_LIB_PATH pointing at a variant build (tools/variants.py
build ...) the same rays price a variant of the child test.
    python tools/visit_probe.py [config] [tile_row_stride]
Rays: every tile_row_stride-th row of 8x8 tiles (all 8 rows of each), so tile maxima are exact.
Then (RT_PROBE_ENTRY=0: not) the same primary rays started at their blocks' entry sets, per
policy, without and with the search's back-face test (cull 0 / 1): visits per hit and per miss ray, the sets' sizes
and depths, what closed the links (a covering leaf child / more covering children than fan / the depth cap / the
budget K), and the queries whose status differs from the root query's (profiles/entry_cull/host_probe_*.log)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

from raytracercpp_amd import _lib, scenes
from tools.wbvh_probe import camera_rays


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "sphere1m"
    tstride = int(sys.argv[2]) if len(sys.argv) > 2 else 8
    sc, st = scenes.CONFIGS[name]()
    rw, rh = st.render_size()
    o, d = camera_rays(sc, st, 1)
    rows = np.concatenate([np.arange(ty * 8, min(ty * 8 + 8, rh)) for ty in range(0, (rh + 7) // 8, tstride)])
    sel = (rows[:, None] * rw + np.arange(rw)[None, :]).ravel()
    o, d = o[sel], d[sel]
    nodes = np.zeros(len(o), np.int32)
    st_, ids, t, u, v, stats, ms, oo, do = _lib.wbvh_query(sc.tri, o, d, st.bvh_max_depth, st.bvh_leaf_object_count,
                                                            cam=sc.cam_pos, rays_out=True, ray_nodes=nodes)
    assert stats["violations"] == 0, stats
    # shadow rays of the certified hits (is_shadowed: hit point, geometric normal)
    hit = st_ == 1
    T = sc.tri[ids[hit]].reshape(-1, 3, 3)
    p = (o[hit] + d[hit] * t[hit][:, None]).astype(np.float32)
    n = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    lit = ((sc.light[None] - p) * n).sum(1) > 0
    snodes = np.zeros(int(lit.sum()), np.int32)
    _lib.wbvh_query(sc.tri, p[lit], n[lit], st.bvh_max_depth, st.bvh_leaf_object_count, cam=sc.cam_pos,
                    light=sc.light, shadow_rays=True, ray_nodes=snodes)
    q = np.percentile(nodes, [50, 90, 99, 99.9, 100])
    print(f"{name}: {len(o)} primary rays ({len(rows)} rows): {nodes.mean():.3f} node visits/ray; "
          f"p50/p90/p99/p99.9/max {q[0]:.0f}/{q[1]:.0f}/{q[2]:.0f}/{q[3]:.0f}/{q[4]:.0f}; "
          f"not certified {int((st_ == 2).sum())}")
    qs = np.percentile(snodes, [50, 90, 99, 99.9, 100]) if len(snodes) else [0] * 5
    print(f"  {len(snodes)} shadow rays: {snodes.mean() if len(snodes) else 0:.3f} node visits/ray; "
          f"p50/p90/p99/p99.9/max {qs[0]:.0f}/{qs[1]:.0f}/{qs[2]:.0f}/{qs[3]:.0f}/{qs[4]:.0f}")
    # per tile: the longest primary ray (the wave's iterations are at least that)
    tx = rw // 8
    tile = (np.repeat(np.arange(len(rows)) // 8, rw) * tx + np.tile(np.arange(rw) // 8, len(rows)))
    tmax = np.zeros(tile.max() + 1, np.int64)
    np.maximum.at(tmax, tile, nodes)
    top = np.sort(tmax)[::-1]
    print(f"  tiles: {len(tmax)}; longest-ray visits, top 10: {top[:10].tolist()}; tiles over 100: {int((tmax > 100).sum())},"
          f" over 200: {int((tmax > 200).sum())}")
    print(f"  hit rays {nodes[hit].mean():.3f} visits/ray, misses {nodes[~hit].mean():.3f}; mean over tiles of the "
          f"longest ray {tmax.mean():.3f} (the waves' iterations: {tmax.mean() / max(nodes.mean(), 1e-9):.2f}x the mean ray)")
    if os.environ.get("RT_PROBE_ENTRY", "1") != "0":
        entry_table(name, sc, st, o, d, rows, rw, rh, st_, nodes)


def entry_table(name, sc, st, o, d, rows, rw, rh, st_root, n_root):
    """The same rays started at their blocks' entry sets, per policy (K nodes per block, a
    frontier node expanded while at most 'fan' of its children cover the block)."""
    pix = np.stack([np.tile(np.arange(rw), len(rows)), np.repeat(rows, rw)], 1).astype(np.int32)
    hit = st_root == 1
    blk = (pix[:, 1] >> 3) * ((rw + 7) // 8) + (pix[:, 0] >> 3)
    print(f"  entry sets ({name}, {len(o)} rays; from the root: {n_root[hit].mean():.3f} visits per hit ray, "
          f"{n_root[~hit].mean():.3f} per miss ray)")
    print("  K fan cull | hit ray  miss ray  all rays | saved/hit | status differs | covered blocks: links 1/2/3/4, at the "
          "root | closed by leaf/fan/depth/K | link depth 1..12")
    for k, fan, cull in [(k, fan, c) for k, fan in ((1, 1), (2, 2), (4, 1), (4, 2), (4, 3), (4, 4)) for c in (0, 1)]:
        nodes = np.zeros(len(o), np.int32)
        e = dict(proj_inv=sc.proj_inv, cam_to_world=sc.cam_to_world, rw=rw, rh=rh, pixel=pix, k=k, fan=fan, no_cull=1 - cull)
        s2 = _lib.wbvh_query(sc.tri, o, d, st.bvh_max_depth, st.bvh_leaf_object_count, cam=sc.cam_pos, ray_nodes=nodes,
                             entry=e)[0]
        assert e["has_mask"], "the camera has no mask"
        sets = e["sets"].reshape(-1, 4)
        # the covered blocks among the probed rows: those whose set is not the bare root, or that hold a hit
        probed = np.unique(blk)
        ps = sets[probed]
        nl = (ps != 0xFFFFFFFF).sum(1)
        root = (ps[:, 0] == 0)
        cov = ~root | np.isin(probed, np.unique(blk[hit]))
        sizes = [int(((nl == i) & ~root & cov).sum()) for i in (1, 2, 3, 4)]
        ch = e["close_hist"]
        print(f"  {k} {fan}   {cull}    | {nodes[hit].mean():7.3f}  {nodes[~hit].mean():7.3f}  {nodes.mean():7.3f}  | "
              f"{n_root[hit].mean() - nodes[hit].mean():6.3f}    | {int((s2 != st_root).sum()):6d}         | "
              f"{sizes[0]}/{sizes[1]}/{sizes[2]}/{sizes[3]}, {int((root & cov).sum())} | {ch[0]}/{ch[1]}/{ch[2]}/{ch[3]} | "
              f"{e['depth_hist'][1:13]}")


if __name__ == "__main__":
    main()
