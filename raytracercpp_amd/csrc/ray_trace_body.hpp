// ray_trace_body.hpp -- the body of kernels.hip's frame kernels, included once in ray_trace_kernel<REFL, PLAIN, OCT>
// (LIST = false) and once in ray_trace_list_kernel (LIST = true), inside the kernel's braces: REFL, PLAIN, OCT and
// LIST are constants of the including kernel, P_arg its parameter.  Not a header to include anywhere else.
    // The kernel reads its parameters where the kernel received them, through a pointer
    // the compiler cannot hoist out of the tile loop: each field is loaded (scalar cache) where
    // a tile uses it instead of ~100 of them being held in registers across the loop, which
    // spilled (register budget).
    auto kp = __builtin_amdgcn_kernarg_segment_ptr();
    const KParams& P = *reinterpret_cast<const KParams*>((const void*)kp);
    uint2* lv = lane_stack();
    int lane = threadIdx.x & 63;
    unsigned nshadow = 0, nrefl = 0;
    tile_queue_init();
#if RT_PHASE_TIME
    if (PLAIN && lane == 0) {
        for (int k = 0; k < PH_PHASES; k++)
            g_phase[threadIdx.x >> 6][k] = 0;
        g_phase[threadIdx.x >> 6][PH_PHASES] = __builtin_amdgcn_s_memtime();
    }
#endif
    for (;;) {
        auto kpl = kp;
        asm volatile("" : "+s"(kpl));   // (the loop's loads depend on it: not hoisted)
        const KParams& P = *reinterpret_cast<const KParams*>((const void*)kpl);
        const v3 cam = mk(P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]);
        if (PLAIN && !REFL && !OCT && P.heavy_group == SPLIT_G &&
            !__builtin_amdgcn_readfirstlane(__hip_atomic_load(&g_bq.split_done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))) {
            // the split tiles' parts first (trace_split_part)
            int t = 0;
            if (lane == 0)
                t = atomicAdd(P.heavy_ctr + 2, 1);
            t = __builtin_amdgcn_readfirstlane(t);
            if (t < P.split_parts * min(ldg(P.heavy_ctr + 3), P.tiles_x * P.tiles_y / 16)) {
                trace_split_part<SPLIT_G>(P, lv, t, lane, nshadow);
                continue;
            }
            if (lane == 0)
                __hip_atomic_store(&g_bq.split_done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        const int tq = tile_queue_next<LIST>(P);
        if (PLAIN) PH_MARK(6);
        if (tq < 0)
            break;
        const int tile = tq & 0x0fffffff;
        if (P.heavy_list)
            set_wave_prio(tq >> 28);
        const uint64_t tile_t0 = __builtin_amdgcn_s_memtime();
        int tx, ty;
        tile_xy(P, tile, tx, ty);
        int px = tx * 8 + (lane & 7);
        int lr = ty * 8 + (lane >> 3);
        int py = lr < P.local_rows ? global_row(P, lr) : P.rh;
        if (PLAIN) PH_MARK(0);
        if (px >= P.rw || py >= P.rh) {
            if (P.tile_cost && lane == 0)
                P.tile_cost[tile] = 0u;
            continue;
        }
        if (PLAIN && !REFL && !OCT && P.tile_mask) {
            // the tile mask: no ray of a block whose bit is clear enters the cut, so each
            // is a certified miss; a tile whose lanes' blocks are all clear is the background's
            const uint32_t mw = ldg(P.tile_mask + (size_t)(py >> 3) * (size_t)P.mask_wpr + (size_t)(px >> 8));
            if (!__ballot((mw >> ((px >> 3) & 31)) & 1u)) {
                fill_masked_tile(P, lr, px);
                if (P.tile_cost)
                    tile_cost_store(P, tile, tile_t0, lane);
                PH_MARK(7);
                continue;
            }
        }
        // ray generation, renderer.cpp:1086-1098
        const v3 rd = camera_dir(P, px, py, cam);
        if (PLAIN) PH_MARK(1);

        uint32_t rng = REFL ? pixel_seed((uint32_t)(py * P.rw + px), P.rng_seed) : 0u;
        PixelOut po = trace_pixel<REFL, PLAIN, 1, OCT>(P, cam, rd, lv, rng, nshadow, nrefl,
                                                        PLAIN && !REFL && !OCT ? tile_start_index(P, px, py) : -1);
        size_t o = (size_t)lr * P.rw + px;
        if (P.argb) P.argb[o] = color_to_argb(po.color);
        if (!REFL && P.ds_out) downscale_tile(P, lane, lr, px, color_to_argb(po.color));
        if (P.rgba) P.rgba[o] = make_float4(po.color.r, po.color.g, po.color.b, po.alpha);
        if (P.hit_id) P.hit_id[o] = po.found ? po.src : -1;
        if (P.hit_t) P.hit_t[o] = po.fin.t;
        if (P.shadow) P.shadow[o] = (uint8_t)(po.found && po.shadowed);
        if (!PLAIN && P.zbuf) write_ssao_buffers(P, o, po.found, cam, rd, po.fin);
        if (PLAIN) PH_MARK(5);
        if (P.tile_cost)   // the tile's shader cycles (heavy-first order of the next launch)
            tile_cost_store(P, tile, tile_t0, lane);
    }
    if (LIST && P.list_off) {
        // the queue ran over the covered tiles alone: the clear ones, now (at the exit: the heavy tiles started
        // with the frame, and the frame's tail has idle waves)
        fill_clear_tiles(P);
        PH_MARK(7);
    }
    tile_stats_flush(P, lane);
#if RT_PHASE_TIME
    if (PLAIN) {
        PH_MARK(0);   // the final (empty) dequeues
        const int wid = (int)(blockIdx.x * WAVES_PER_BLOCK + (threadIdx.x >> 6));
        if (P.dbg && lane == 0 && wid < DBG_WAVES)
            for (int k = 0; k < PH_PHASES; k++)
                P.dbg[DBG_WORDS * wid + k] = g_phase[threadIdx.x >> 6][k];
    }
#endif
    if (nshadow) atomicAdd(&P.counters[0], (unsigned long long)nshadow);
    if (nrefl) atomicAdd(&P.counters[1], (unsigned long long)nrefl);
