// rbs_call.h -- one likelihood call on one device: the occlusion coefficients, the launches of the rectangles, raster, copy and
// shared-plane kernels, the shared trail's policy, and enqueue_loglikes, which strings them together.  Also the small helpers that
// the call is the first to need and plane housekeeping and create_impl use after it: host_propagate, exact_background, exact_stride,
// kExactTau (stamped planes) and tiles_upper_bound.
// Not a header to include elsewhere: a section of rbsensor_capi.hip's translation unit, included there once, behind rbs_handle.h
// and the frame section (it calls can_borrow, stage_borrowed, wait_for_upload, obs_frame, ...).
namespace {

// alpha/beta of the occlusion process over n frames (affine form of SURVEY A.5), rounded
// once to float -- the same rule as oracle orc_eager_coeffs().
void occlusion_coeffs(const rbs_handle* h, int n_frames, float* alpha, float* beta)
{
    const double c = h->p_oo - h->p_ov;
    const double a = std::exp(((double)n_frames * h->delta_time) * std::log(c));
    const double g = (1.0 - h->p_oo) * (a - 1.0) / (c - 1.0);
    *alpha = (float)a;
    *beta = (float)((1.0 - a) - g);
}

// OcclusionModel propagate as the oracle evaluates it (oracle orc_propagate): the same expressions, the same libm.
double host_propagate(const rbs_handle* h, double occ, double dt)
{
    const double c = h->p_oo - h->p_ov;
    const double pow_c = std::exp(dt * std::log(c));
    const double new_visible = pow_c * (1.0 - occ) + (1.0 - h->p_oo) * (pow_c - 1.0) / (c - 1.0);
    return 1.0 - new_visible;
}
// Stamped planes: the prior of a never-covered pixel `frames` frames after rbs_reset (the oracle's slot of initial values, stamp 0).
float exact_background(const rbs_handle* h, long frames)
{
    return (float)host_propagate(h, (double)(float)h->init_occ, (double)frames * h->delta_time);
}
// Floats per slot of `px` pixels: the values, then the ages (two per float), rounded to whole float4s.
size_t exact_stride(size_t px) { return (px + (px + 1) / 2 + 3) & ~(size_t)3; }
constexpr double kExactTau = 0x1p-40;   // c^(age_max dt) <= this: what a pixel declared background can still differ by

// Most work items any rectangle inside the frame can split into (sizes the partial-sum buffer).
size_t tiles_upper_bound(int cols, int rows, int max_w, int cap_px)
{
    size_t worst = 1;
    for (int rw = 16; rw <= ((cols + 15) & ~15); rw += 16) {
        const rbs::TileGrid g = rbs::tile_grid(rw, rows, max_w, cap_px);
        worst = std::max(worst, (size_t)g.nx * g.ny);
    }
    return worst;
}

// The rectangles kernel of a call over P.n particles, one of its three launches (enqueue_loglikes and the test build's probe,
// rbsensor_probes.hip, launch it through here).  frame_src: a device frame handed over right before the call -- its ingest
// (keep: the copy to keep, or null; aux: its per-pixel terms, or null) rides on the same launch, aux_blocks blocks behind the
// particles'; else deltas: the poses are composed from P.deltas_src first.
void launch_prep(const DevParams& P, int* d_rects, int update, bool deltas, const float* frame_src, double* aux, float* pbg, float* keep,
                 hipStream_t s)
{
    constexpr int ptb = 64 * rbs::kPrepPerBlock;
    const unsigned prep_blocks = (unsigned)((P.n + rbs::kPrepPerBlock - 1) / rbs::kPrepPerBlock);
    if (frame_src) {
        const int aux_blocks = (aux || keep) ? (P.npx + ptb - 1) / ptb : 0;
        hipLaunchKernelGGL(rbs::rbs_frame_prep_kernel, dim3((unsigned)aux_blocks + prep_blocks), dim3(ptb), 0, s, P, d_rects, update, frame_src,
                           aux, pbg, keep, aux_blocks);
    } else if (deltas) {
        hipLaunchKernelGGL(rbs::rbs_prep_deltas_kernel, dim3(prep_blocks), dim3(ptb), 0, s, P, d_rects, update);
    } else {
        hipLaunchKernelGGL(rbs::rbs_prep_kernel, dim3(prep_blocks), dim3(ptb), 0, s, P, d_rects, update);
    }
}

// The instantiations of the raster kernel: updating or read-only call, likelihood precision,
// whole planes or slabs, and the same eight again for object models with a body of many clusters.
void launch_raster(const rbs_handle* h, bool update, dim3 grid, dim3 block, size_t smem, hipStream_t s, const DevParams& P)
{
    const bool slab = h->slab_px != 0, many = h->many_clusters, stp = P.bgp_src != nullptr;   // (template arguments S, M, T; U: update)
    if (h->exact && !h->many_clusters && h->n_bodies == 1 && !P.groups) {   // stamped planes, one body
        with_flags([&](auto U, auto S, auto T) { hipLaunchKernelGGL((rbs::rbs_raster_kernel_exact_one_f64<U(), S(), T()>), grid, block, smem, s, P); },
                   update, slab, stp);
        return;
    }
    if (h->exact) {   // stamped planes (binary64): updating or not, whole planes or slabs, many clusters, shared background plane
        with_flags([&](auto U, auto S, auto M, auto T) { hipLaunchKernelGGL((rbs::rbs_raster_kernel_exact_f64<U(), S(), M(), T()>), grid, block, smem, s, P); },
                   update, slab, many, stp);
        return;
    }
    if (P.bgp_src && h->precision == RBS_PRECISION_F32) {   // the shared background plane, float32 likelihood
        with_flags([&](auto U, auto S, auto M) { hipLaunchKernelGGL((rbs::rbs_raster_kernel_stp_f32<U(), S(), M()>), grid, block, smem, s, P); },
                   update, slab, many);
        return;
    }
    if (P.bgp_src) {   // the shared background plane (binary64)
        with_flags([&](auto U, auto S, auto M) { hipLaunchKernelGGL((rbs::rbs_raster_kernel_stp_f64<U(), S(), M()>), grid, block, smem, s, P); },
                   update, slab, many);
        return;
    }
    if (!h->many_clusters && h->precision == RBS_PRECISION_F64 && h->n_bodies == 1 && !P.groups) {
        with_flags([&](auto U, auto S) { hipLaunchKernelGGL((rbs::rbs_raster_kernel_one_f64<U(), S()>), grid, block, smem, s, P); }, update, slab);
        return;
    }
    with_flags([&](auto M, auto U, auto F32, auto S) {   // (many clusters x precision: four names, one pair of arguments)
        if constexpr (M() && F32()) hipLaunchKernelGGL((rbs::rbs_raster_kernel_many_f32<U(), S()>), grid, block, smem, s, P);
        else if constexpr (M()) hipLaunchKernelGGL((rbs::rbs_raster_kernel_many_f64<U(), S()>), grid, block, smem, s, P);
        else if constexpr (F32()) hipLaunchKernelGGL((rbs::rbs_raster_kernel_f32<U(), S()>), grid, block, smem, s, P);
        else hipLaunchKernelGGL((rbs::rbs_raster_kernel_f64<U(), S()>), grid, block, smem, s, P);
    }, many, update, h->precision == RBS_PRECISION_F32, slab);
}

// The shared plane's own step on stream s: bgp[1 - cur] = step(bgp[cur]), re-based first on local slot `rebase` of the planes
// (occ, win, reg) -- its owner's, wherever they live -- or (-2) reset to the scalar level.
int32_t launch_bgp_step(rbs_handle* h, const DevParams& P, const float* occ, const int4* win, const int4* reg, int rebase, hipStream_t s)
{
    if (h->exact)
        hipLaunchKernelGGL(rbs::rbs_bgp_step_exact_kernel, dim3((unsigned)((h->npx + 255) / 256)), dim3(256), 0, s, h->d_bgp[h->cur], h->d_bgp[1 - h->cur],
                           occ, win, reg, P.plane_stride, P.plane_px, rebase, h->rows, h->cols, P.elapsed2, P.bg_new);
    else
        hipLaunchKernelGGL(rbs::rbs_bgp_step_kernel, dim3((unsigned)((h->npx + 255) / 256)), dim3(256), 0, s, h->d_bgp[h->cur], h->d_bgp[1 - h->cur],
                           occ, win, reg, P.plane_stride, rebase, h->rows, h->cols, P.alpha, P.beta, P.bg_new);
    RBS_HIP(h, hipGetLastError());
    return RBS_OK;
}

// The shared trail's policy (rbs_handle::stp), one decision per call: `o` owns the state -- a handle of its own, or the GROUP for
// all its shards.  Returns this call's directive: rebase >= 0 (re-base on that slot's plane; entering: the shared plane starts as
// the scalar level first), -2 (back to the scalar background), -1 (nothing).
rbs_handle::StpNow stp_decide(rbs_handle* o, bool update, double area_frac)
{
    rbs_handle::StpNow d;
    const long since = o->calls - o->stp_last_rebase;
    if (update && o->stp && area_frac > o->wide_enter && since >= 16 && since < o->stp_every) {
        // re-basing did not help: the windows are still most of the frame a sample or two later -- the particles share no
        // ancestor (a synthetic permutation of parents; a filter that never resamples).  Back to the scalar background and
        // the whole-plane machinery that serves such windows best: this call re-measures every child against the scalar
        // level over the bounding box of the shared plane's own values.
        d.rebase = -2;
    } else if (update && !o->stp && area_frac > o->stp_enter && o->calls > 0 && o->calls >= o->stp_block_until) {
        d.entering = true;
        d.rebase = 0;
        o->stp = true;
    } else if (update && o->stp && area_frac > o->stp_enter && since >= o->stp_every) {
        d.rebase = 0;
    }
    if (o->stp && d.rebase >= 0) { o->stp_last_rebase = o->calls; o->stp_rebases += 1; }
    return d;
}

int32_t enqueue_loglikes(rbs_handle* h, const double* d_poses, const int* d_indices, int n,
                         bool update, double* d_out, hipStream_t s, const double* host_poses = nullptr, const double* host_deltas = nullptr)
{
    h->quiet = false;
    // a borrowed frame (rbs_set_observation_borrowed) is staged BETWEEN the two kernels of the split launch, while the
    // geometry kernel -- which needs no frame -- runs; a handle that cannot launch that way stages it here and now
    if (!(can_borrow(h) && s == h->stream))
        if (int32_t rc = stage_borrowed(h)) return rc;
    DevParams P = h->base;
    occlusion_coeffs(h, h->pending_frames, &P.alpha, &P.beta);
    P.bg_old = h->background;
    P.bg_new = std::fmaf(P.alpha, h->background, P.beta);
    P.exact = h->exact ? 1 : 0;
    P.plane_px = h->slab_px ? h->slab_px : h->npx;
    if (h->exact) {   // stamped planes: nothing is stepped; a never-covered pixel's prior comes from the model clock
        const unsigned e = (unsigned)std::min(h->pending_frames, 0xffff);
        P.elapsed2 = e | (e << 16);
        P.age_max = h->age_max;
        P.ptab = h->d_ptab;
        P.bg_new = exact_background(h, h->update_clock + h->pending_frames);
        P.bg_old = P.bg_new;
    }
    P.windowed = h->windowed ? 1 : 0;
    P.rect_align = h->windowed ? rbs::kRectAlignWindowed : rbs::kRectAlign;
    P.win_src = h->d_win[h->cur];
    P.win_dst = h->d_win[1 - h->cur];
    P.win_used = h->d_win_used;
    P.frame = obs_frame(h);
    P.aux = obs_aux(h);
    P.pbg = h->d_pbg;
    P.occ_src = h->d_occ[h->cur];
    P.occ_dst = h->d_occ[1 - h->cur];
    P.poses = d_poses;
    P.poses_src = host_poses;   // pinned host memory the rectangles kernel pulls the poses from (into d_poses)
    P.deltas_src = host_deltas; // ... or composes them from (rbs_loglikes_deltas)
    P.indices = d_indices;
    P.slots = h->max_particles;
    P.n_dev = 1;
    P.shard_cap = h->max_particles;
    P.slab_px = h->slab_px;
    P.plane_stride = (int)h->plane_stride;
    P.reg_src = h->d_reg[h->cur];
    P.reg_dst = h->d_reg[1 - h->cur];
    P.err = h->d_err;
    if (h->group) {   // the planes and windows of every shard of the group: parents are global slots
        rbs_handle* g = h->group;
        P.n_dev = (int)g->shards.size();
        P.shard_cap = g->shard_cap;
        P.slots = P.n_dev * g->shard_cap;
        for (int k = 0; k < P.n_dev; ++k) {
            P.occ_src_dev[k] = g->snap_occ[k];
            P.win_src_dev[k] = g->snap_win[k];
            P.reg_src_dev[k] = g->snap_reg[k];
        }
    }
    if (h->peer_world > 1) {   // the same table, the other devices being other PROCESSES' handles (every rank flips its buffers in step)
        P.n_dev = h->peer_world;
        P.shard_cap = h->max_particles;
        P.slots = h->peer_world * h->max_particles;
        for (int k = 0; k < P.n_dev; ++k) {
            P.occ_src_dev[k] = k == h->peer_rank ? h->d_occ[h->cur] : h->peer_occ[k][h->cur];
            P.win_src_dev[k] = k == h->peer_rank ? h->d_win[h->cur] : h->peer_win[k][h->cur];
            P.reg_src_dev[k] = k == h->peer_rank ? h->d_reg[h->cur] : h->peer_reg[k][h->cur];
        }
    }
    P.out = d_out;
    P.n = n;
    const int slot = (int)(h->calls % rbs_handle::kRing);          // ev_join
    const bool timed = h->timing_every <= 1 || h->calls < 4 || h->calls % h->timing_every == 0;   // and the first few, so short sessions have a warm sample
    const int tslot = (int)(h->timed_calls % rbs_handle::kRing);    // timing events
    if (timed) h->ring_update[tslot] = update;
    // tile limits: as large as the LDS tile allows (a particle's rectangle is then usually ONE
    // work item, whatever its aspect); with fewer particles than persistent blocks the pixel
    // budget is divided so that a rectangle splits into about blocks/n row bands
    if (h->windowed && update && h->area_pending && hipEventQuery(h->ev_area) == hipSuccess) {
        const double frac = (double)*h->h_area / ((double)h->area_n * (double)h->npx);   // sampled a few calls ago
        h->area_frac = frac;
        if (frac > h->wide_enter && !h->slab_px && !h->exact) h->wide = true;   // (slabs: regions that large do not fit anyway; stamped planes: the windowed copy serves every size)
        else if (frac < h->wide_leave) h->wide = false;
        h->area_pending = false;
    }
    // shared trail: enter once the windows have grown, re-base while they stay large (see rbs_handle::stp)
    int rebase = -1;          // >= 0: re-base on that (global) slot's plane; -2: back to the scalar background
    bool stp_leaving = false;
    P.bgp_src = nullptr; P.bgp_dst = nullptr; P.rebase_box = nullptr;
    rbs_handle* const so = h->group ? h->group : h;   // who owns the shared trail's state: the group for all its shards
    if (h->windowed && so->stp_allowed) {
        rbs_handle::StpNow d;
        if (h->group) {
            d = so->stp_now;                               // (decided once for every shard: group_begin_call)
        } else if (h->peer_world > 1 || h->ipc_exported || h->stp_request != -1) {   // the caller's directive (rbs_shared_trail_rebase): attached ranks always
            if (update && h->stp_request != -1) {
                if (h->stp_request >= 0) {
                    d.rebase = h->stp_request;
                    d.entering = !h->stp;
                    h->stp_last_rebase = h->calls;
                    h->stp_rebases += 1;
                } else if (h->stp) {
                    d.rebase = -2;
                }
                h->stp_request = -1;
            }
        } else {
            d = stp_decide(h, update, h->area_frac);
        }
        rebase = d.rebase;
        stp_leaving = rebase == -2;
        if (d.entering || (h->group && so->stp && !h->stp && !stp_leaving)) {   // this device's copy of the shared plane: the scalar level everywhere
            for (int k = 0; k < 2; ++k)
                if (!h->d_bgp[k]) RBS_HIP(h, hipMalloc(&h->d_bgp[k], sizeof(float) * (h->exact ? exact_stride((size_t)h->npx) : (size_t)h->npx)));
            if (!h->d_bgp_box) RBS_HIP(h, hipMalloc(&h->d_bgp_box, sizeof(int4)));
            hipLaunchKernelGGL(rbs::rbs_fill_kernel, dim3(256), dim3(256), 0, s, h->d_bgp[h->cur], (size_t)h->npx, h->background);
            RBS_HIP(h, hipGetLastError());
            if (h->exact)   // (every pixel background: ages 0xffff)
                RBS_HIP(h, hipMemsetAsync(h->d_bgp[h->cur] + h->npx, 0xff, sizeof(unsigned short) * (size_t)h->npx, s));
            h->stp = true;
            h->wide = false;
        }
        if (stp_leaving && h->stp) {
            hipLaunchKernelGGL(rbs::rbs_set_window_kernel, dim3(1), dim3(64), 0, s, h->d_bgp_box, 1, make_int4(h->cols, h->rows, 0, 0));
            if (h->exact)
                hipLaunchKernelGGL(rbs::rbs_bbox_age_kernel, dim3((unsigned)((h->npx + 255) / 256)), dim3(256), 0, s, h->d_bgp[h->cur], h->rows, h->cols,
                                   (unsigned)h->age_max, reinterpret_cast<int*>(h->d_bgp_box));
            else
            hipLaunchKernelGGL(rbs::rbs_bbox_kernel, dim3((unsigned)((h->npx + 255) / 256)), dim3(256), 0, s, h->d_bgp[h->cur], h->rows, h->cols,
                               h->background, reinterpret_cast<int*>(h->d_bgp_box));
            RBS_HIP(h, hipGetLastError());
        }
        if (h->stp) {
            P.bgp_src = h->d_bgp[h->cur];
            P.bgp_dst = h->d_bgp[1 - h->cur];
            h->wide = false;   // (the whole-plane machinery knows the scalar background only)
            if (rebase >= 0) h->area_frac = 0.0;   // (judged again from the next sample)
        } else {
            rebase = -1; stp_leaving = false;
        }
    }
    // the whole-plane layout always runs two raster blocks per CU and can afford the larger LDS
    // tile (fewer rectangles split into two work items).  Windowed planes keep ONE tile size
    // whatever the number of blocks of a call: the split decides the order in which a
    // particle's partial sums are added, and the switch between the modes depends on when an
    // asynchronous read-back lands -- results must not.
    const bool f64 = h->precision == RBS_PRECISION_F64;   // (its math tables take a little of the LDS tile)
    // (round 5, C4 slice: the 16 384-px tile with two blocks per CU -- 6 work items per particle instead of 10 -- 7.62 ms against 6.32 with
    // three blocks and the small tile; two blocks with the small tile 8.16: the larger tile is worth 7 %, the third wave per SIMD 25 %)
    P.tile_px = !h->windowed && h->raster_blocks <= 2 * h->cu_count ? (f64 ? rbs::kTilePxBigF64 : rbs::kTilePxBig)
                                                                     : (h->exact ? rbs::kTilePxExact : f64 ? rbs::kTilePxF64 : rbs::kTilePx);
    // split launch: binary64 likelihood on windowed planes (the tile size is the handle's for its whole life, like the
    // monolith's: the split of a rectangle into items decides the order in which a particle's partial sums are added)
    const bool have_borrowed = h->fr.next.borrowed();
    bool split = (h->split || have_borrowed) && f64 && h->windowed;   // (the same tile, the same items, the same bits either way)
    if (split && !h->exact && !(!h->windowed && h->raster_blocks <= 2 * h->cu_count)) P.tile_px = rbs::kDepthTilePx;   // (= kTilePxF64 already; stamped planes: their own, smaller)
    P.tile_w = 256;
    P.tile_h = std::max(4, P.tile_px / 256 / std::max(1, h->smalln_target / std::max(1, n)));
    const size_t tiles_max = tiles_upper_bound(h->cols, h->rows, P.tile_w, std::min(P.tile_w * P.tile_h, P.tile_px));
    const size_t need = (size_t)n * tiles_max * (h->d_groups[0] ? rbs::kMaxGroups : 1);
    if (need > h->partial_cap) {
        RBS_HIP(h, hipStreamSynchronize(s));
        RBS_HIP(h, hipStreamSynchronize(h->copy_stream));
        (void)hipFree(h->d_partial);
        (void)hipFree(h->d_item_particle);
        h->d_partial = nullptr;
        h->d_item_particle = nullptr;
        h->partial_cap = 0;
        RBS_HIP(h, hipMalloc(&h->d_partial, sizeof(double) * need));
        RBS_HIP(h, hipMalloc(&h->d_item_particle, sizeof(int) * need));
        h->partial_cap = need;
    }
    if (split) {
        // the hand-over buffer: one tile per work item, sized for the WORST case (every rectangle the whole frame: 36 tiles per
        // particle at 640x480) so that no item can ever lie beyond it -- 2.7 GB at 2 000 particles.  Where that exceeds
        // kDepthBudget (20 000 particles) the call is launched as ONE kernel instead (a borrowed frame is staged first).
        // RBS_SPLIT_ITEMS_PER_PARTICLE (tooling / tests): a buffer of n x that many tiles (+ 1 024); an item beyond it is
        // contained (its particle's log-likelihood is NaN), never a wild access.
        constexpr size_t kDepthBudget = (size_t)8 << 30;
        const char* pe = std::getenv("RBS_SPLIT_ITEMS_PER_PARTICLE");
        const size_t want = pe ? std::min(need, (size_t)n * (size_t)std::max(1, std::atoi(pe)) + 1024) : need;
        const size_t bytes = sizeof(unsigned) * (size_t)rbs::kDepthTilePx * want;
        //  the buffer must also FIT: no more than half of what the device has free once the old buffer is returned --
        // the planes of max_particles, other handles and the caller's own allocations live there too -- and an allocation that
        // fails all the same takes the one-kernel launch instead of failing the call
        bool fits = bytes <= kDepthBudget;
        if (fits && want > h->depth_items) {
            size_t free_b = 0, total_b = 0;
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
                const size_t mine = sizeof(unsigned) * (size_t)rbs::kDepthTilePx * h->depth_items;
                fits = bytes <= (free_b + mine) / 2;
            } else {
                (void)hipGetLastError();
            }
        }
        if (want > h->depth_items && fits) {
            RBS_HIP(h, hipStreamSynchronize(s));
            (void)hipFree(h->d_depth);
            h->d_depth = nullptr;
            h->depth_items = 0;
            if (hipMalloc(&h->d_depth, bytes) == hipSuccess) {
                h->depth_items = want;
            } else {
                (void)hipGetLastError();
                h->d_depth = nullptr;
                fits = false;
            }
        }
        if (want > h->depth_items && !fits) {   // one kernel (a borrowed frame is staged first: nothing of this call is enqueued yet)
            split = false;
            if (have_borrowed) {
                if (int32_t rc = stage_borrowed(h)) return rc;
                P.frame = obs_frame(h);
                P.aux = obs_aux(h);
            }
        }
    }
    if (split) {
        P.depth = h->d_depth;
        P.depth_items = (int)std::min<size_t>(h->depth_items, 0x7fffffff);
        P.ctrb_this = h->d_ctr + 4 + (int)(h->calls & 1);
        P.ctrb_next = h->d_ctr + 4 + (int)((h->calls + 1) & 1);
    }
    int* const d_rects = h->d_rects[h->calls & 1];
    P.rects = d_rects;
    P.groups = h->d_groups[h->calls & 1];
    P.strips = update && h->windowed && !h->copy_walk ? h->d_strips[h->calls & 1] : nullptr;
    P.parents = h->d_parents[h->calls & 1];
    P.item_range = h->d_item_range;
    P.item_particle = h->d_item_particle;
    P.ctr_this = h->d_ctr + 2 * (int)(h->calls & 1);
    P.ctr_next = h->d_ctr + 2 * (int)((h->calls + 1) & 1);
    P.done = h->d_done;
    P.partial = h->d_partial;
#ifdef RBS_PHASE_TIMING
    if (!h->d_phase) { RBS_HIP(h, hipMalloc(&h->d_phase, 256)); RBS_HIP(h, hipMemset(h->d_phase, 0, 256)); }
    P.phase = h->d_phase;
#endif
    if (timed) RBS_HIP(h, hipEventRecord(h->ev_start[tslot], s));
    const dim3 block(rbs::kBlock);
    // dense planes: prep + scan read only the poses and run ahead of the previous call's copy
    // kernel (which reads the other rectangle buffer); windowed planes: prep reads the windows
    // that copy kernel is still growing, so the join comes first (that copy is short)
    if (h->windowed && h->join_pending >= 0) {
        RBS_HIP(h, hipStreamWaitEvent(s, h->ev_join[h->join_pending], 0));
        h->join_pending = -1;
    }
    // the plane the shared plane is re-based on: GLOBAL slot `rebase`, wherever it lives (a shard / an attached rank reads it from its owner)
    const float* rb_occ = P.occ_src; const int4* rb_win = P.win_src; const int4* rb_reg = h->slab_px ? P.reg_src : (const int4*)nullptr;
    int rb_local = rebase;
    if (rebase >= 0 && P.n_dev > 1) {
        const int owner = rebase / P.shard_cap;
        rb_local = rebase - owner * P.shard_cap;
        rb_occ = P.occ_src_dev[owner]; rb_win = P.win_src_dev[owner]; rb_reg = h->slab_px ? P.reg_src_dev[owner] : (const int4*)nullptr;
    }
    if (P.bgp_src) P.rebase_box = rebase >= 0 ? rb_win + rb_local : rebase == -2 ? h->d_bgp_box : nullptr;
    if (P.bgp_src && update)   // the shared plane's own step (and re-basing): reads the current planes, complete after the join above
        if (int32_t rc = launch_bgp_step(h, P, rb_occ, rb_win, rb_reg, rebase >= 0 ? rb_local : rebase, s)) return rc;
    bool sample_area = false;
    if (h->windowed && update) {
        sample_area = timed && !h->area_pending;
        if (sample_area) RBS_HIP(h, hipMemsetAsync(h->d_area, 0, sizeof(unsigned long long), s));
    }
    P.area_sum = sample_area ? h->d_area : nullptr;
    const bool wide = h->windowed && update && h->wide;
    // wide windows: two raster blocks per CU leave the streaming copy its registers
    const bool mid = h->windowed && update && !wide && h->area_frac > h->mid_enter;
    // the windowed copy done by the raster kernel's own blocks (rbs_raster_kernel_wcopy_*: one body, one rectangle, scalar
    // background, whole planes, one device): the call is then prep + raster on this stream -- no fork, no second queue, no join
    const bool fused = h->fused_copy && update && h->windowed && !wide && !mid && !split && !h->exact && !h->slab_px && !P.bgp_src &&
                       !P.groups && h->n_bodies == 1 && !h->many_clusters && !h->group && h->peer_world <= 1 && !h->ipc_exported;
    if (timed && fused) h->ring_update[tslot] = false;   // (no copy kernel to time: timing_summary's copy_kernel_ms is 0)
    if (const float* df = take_device_frame(h, s)) {   // a device frame pending on this stream rides on the rectangles kernel
        launch_prep(P, d_rects, update ? 1 : 0, false, df, h->d_aux, h->d_pbg, df == h->d_frame ? (float*)nullptr : h->d_frame, s);
    } else {
        if (int32_t rc = flush_device_frame(h, s)) return rc;
        launch_prep(P, d_rects, update ? 1 : 0, host_deltas, nullptr, nullptr, nullptr, nullptr, s);
    }
    RBS_HIP(h, hipGetLastError());
    if (sample_area) {
        RBS_HIP(h, hipMemcpyAsync(h->h_area, h->d_area, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        RBS_HIP(h, hipEventRecord(h->ev_area, s));
        h->area_pending = true;
        h->area_n = (n + 7) / 8;    // (the rectangles kernel adds every 8th particle's region)
    }
    if (update && !fused) {
        // fork: the copy kernel runs on the handle's second stream, concurrently with the
        // persistent raster kernel; it needs this call's rectangles only
        RBS_HIP(h, hipEventRecord(h->ev_fork, s));
        // (the windowed copy kernel itself is launched BEHIND the raster kernel's launch, below: its one-wave blocks
        // (32 VGPRs) run beside the persistent raster blocks (3 x 160 VGPRs per SIMD) whichever of the two reaches the
        // device first, and the three runtime calls it takes -- 10-15 us of host time -- are then not in front of the
        // raster kernel when the host is what the device waits for: a tracker frame by frame, the host-pointer calls)
        if (!(h->windowed && !wide)) RBS_HIP(h, hipStreamWaitEvent(h->copy_stream, h->ev_fork, 0));
    }
    // deferred join: the raster kernel reads planes the previous updating call's copy kernel
    // may still be writing; everything before this point overlapped with that copy's tail
    if (h->join_pending >= 0) {
        RBS_HIP(h, hipStreamWaitEvent(s, h->ev_join[h->join_pending], 0));
        h->join_pending = -1;
    }
    if (h->windowed && update && !wide && !mid && !fused && h->timed_calls > h->balance_seen && h->raster_blocks == 3 * h->cu_count) {
        const int last = (int)((h->timed_calls - 1) % rbs_handle::kRing);
        if (h->ring_update[last] && hipEventQuery(h->ev_raster_stop[last]) == hipSuccess && hipEventQuery(h->ev_copy_stop[last]) == hipSuccess) {
            float r_ms = 0.f, c_ms = 0.f;
            if (hipEventElapsedTime(&r_ms, h->ev_raster_start[last], h->ev_raster_stop[last]) == hipSuccess &&
                hipEventElapsedTime(&c_ms, h->ev_copy_start[last], h->ev_copy_stop[last]) == hipSuccess && r_ms > 0.f) {
                const int step = std::max(1, h->cu_count / 8), lo = 5 * h->cu_count / 2;
                int cur = h->balance_blocks ? h->balance_blocks : h->raster_blocks;
                if (c_ms > 1.04f * r_ms) cur = std::max(lo, cur - step);
                else if (c_ms < 0.92f * r_ms) cur = std::min(h->raster_blocks, cur + step);
                h->balance_blocks = cur;
            } else {
                (void)hipGetLastError();
            }
            h->balance_seen = h->timed_calls;
        }
    }
    const int full_grid = h->balance_blocks && h->windowed && update && !fused ? h->balance_blocks : h->raster_blocks;
    const dim3 rgrid((unsigned)(wide || mid ? std::min(h->raster_blocks, 2 * h->cu_count) : full_grid));
    // a host frame that is read where it was uploaded: only now does the stream wait for the upload
    // (split launch: the geometry kernel needs no frame -- the wait sits between the two kernels, and a host frame
    // travels while the depth tiles are rasterized)
    if (!split) if (int32_t rc = wait_for_upload(h, s)) return rc;
    // the windowed copy kernel (one-wave blocks beside the persistent kernels, on the handle's second stream).  A call that stages a
    // borrowed frame between its two kernels launches it BEFORE the staging: it then runs beside the geometry kernel instead of
    // beside the likelihood kernel the caller is waiting for (plugin step +0.7 %, tests/cpp/host_bench --plugin)
    bool window_copy_launched = false;
    auto launch_window_copy = [&]() -> int32_t {
        RBS_HIP(h, hipStreamWaitEvent(h->copy_stream, h->ev_fork, 0));
        if (timed) RBS_HIP(h, hipEventRecord(h->ev_copy_start[tslot], h->copy_stream));
        const int ny = std::min(n, 32768);
        // one body: only the cells outside its rectangle are enumerated (1); several bodies: the strip list the rectangles kernel
        // made (2: round 6); RBS_COPY_WALK=1: the walk over the whole region (0)
        const int strips = !P.groups ? 1 : (P.strips ? 2 : 0);
        const dim3 wg((unsigned)(strips == 1 ? h->win_chunks_single : h->win_chunks), (unsigned)ny, (unsigned)((n + ny - 1) / ny));
        with_flags([&](auto E, auto S, auto B) {
            if (strips == 2) hipLaunchKernelGGL((rbs::rbs_copy_window_kernel<S(), 2, B(), E()>), wg, dim3(64), 0, h->copy_stream, P);
            else if (strips == 1) hipLaunchKernelGGL((rbs::rbs_copy_window_kernel<S(), 1, B(), E()>), wg, dim3(64), 0, h->copy_stream, P);
            else hipLaunchKernelGGL((rbs::rbs_copy_window_kernel<S(), 0, B(), E()>), wg, dim3(64), 0, h->copy_stream, P);
        }, h->exact, h->slab_px != 0, P.bgp_src != nullptr);
        RBS_HIP(h, hipGetLastError());
        if (timed) RBS_HIP(h, hipEventRecord(h->ev_copy_stop[tslot], h->copy_stream));
        RBS_HIP(h, hipEventRecord(h->ev_join[slot], h->copy_stream));
        window_copy_launched = true;
        return RBS_OK;
    };
    if (timed) RBS_HIP(h, hipEventRecord(h->ev_raster_start[tslot], s));
    if (split) {
        const bool two = wide || mid;   // (wide windows: fewer blocks, so that the streaming copy keeps its registers)
        const dim3 dgrid((unsigned)(two ? std::min(h->depth_blocks, 2 * h->cu_count) : h->depth_blocks));
        const dim3 egrid((unsigned)(two ? std::min(h->eval_blocks, 3 * h->cu_count) : h->eval_blocks));
        const size_t dsm = rbs::smem_bytes_depth(P.tile_px, h->many_clusters), esm = rbs::smem_bytes(0, true, false, h->exact);
        with_flags([&](auto M) { hipLaunchKernelGGL((rbs::rbs_depth_kernel<M()>), dgrid, block, dsm, s, P); }, h->many_clusters);
        RBS_HIP(h, hipGetLastError());
        if (have_borrowed && update && h->windowed && !wide)
            if (int32_t rc = launch_window_copy()) return rc;
        if (have_borrowed) {   // the host converts and sends the caller's frame while the depth tiles are rasterized
            if (int32_t rc = stage_borrowed(h)) {
                // half a call is enqueued (rectangles + geometry kernel: the work-item counters of this parity are spent, no plane
                // has been written): every later call is refused until rbs_reset re-establishes a known state
                h->poisoned = true;
                h->poison_msg = h->err;
                return rc;
            }
            P.frame = obs_frame(h);
            P.aux = obs_aux(h);
        }
        if (int32_t rc = wait_for_upload(h, s)) return rc;
        with_flags([&](auto U, auto S, auto T, auto E) { hipLaunchKernelGGL((rbs::rbs_eval_kernel<U(), S(), T(), E()>), egrid, block, esm, s, P); },
                   update, h->slab_px != 0, P.bgp_src != nullptr, h->exact);
        RBS_HIP(h, hipGetLastError());
    }
    if (update) {
        const size_t rsm = rbs::smem_bytes(P.tile_px, f64, h->many_clusters, h->exact);
        if (fused && f64) hipLaunchKernelGGL(rbs::rbs_raster_kernel_wcopy_one_f64, rgrid, block, rsm, s, P);
        else if (fused) hipLaunchKernelGGL(rbs::rbs_raster_kernel_wcopy_f32, rgrid, block, rsm, s, P);
        else if (!split) launch_raster(h, true, rgrid, block, rsm, s, P);
        RBS_HIP(h, hipGetLastError());
        if (timed) RBS_HIP(h, hipEventRecord(h->ev_raster_stop[tslot], s));
        if (timed && (!h->windowed || wide)) RBS_HIP(h, hipEventRecord(h->ev_copy_start[tslot], h->copy_stream));
        if (fused) {
            // (done: the raster kernel wrote the particles' cells outside their rectangles)
        } else if (h->windowed && !wide) {
            if (!window_copy_launched) if (int32_t rc = launch_window_copy()) return rc;
        } else if (wide) {
            const int W4 = P.cols >> 2;
            const int nseg = (W4 + 63) / 64;
            const int ny = std::min(n, 32768);
            const dim3 rg((unsigned)(((P.rows + 1) / 2) * nseg), (unsigned)ny, (unsigned)((n + ny - 1) / ny));
            const int nblk = ((P.rows + 1) / 2) * nseg;
            if (!h->d_wide_flags)
                RBS_HIP(h, hipMalloc(&h->d_wide_flags, (size_t)h->max_particles * nblk));
            P.wide_flags = h->d_wide_flags;
            hipLaunchKernelGGL((rbs::rbs_copy_rows_kernel<2, true>), rg, dim3(64), 0, h->copy_stream, P, nseg);
            hipLaunchKernelGGL(rbs::rbs_wide_window_kernel, dim3((unsigned)n), dim3(64), 0, h->copy_stream, P, nseg, nblk);
        } else if ((P.cols & 3) == 0) {   // two rows per one-wave block: a wave moves 1 KB of a row
            const int W4 = P.cols >> 2;
            const int nseg = (W4 + 63) / 64;
            const int ny = std::min(n, 32768);
            const dim3 rg((unsigned)(((P.rows + 1) / 2) * nseg), (unsigned)ny, (unsigned)((n + ny - 1) / ny));
            hipLaunchKernelGGL((rbs::rbs_copy_rows_kernel<2, false>), rg, dim3(64), 0, h->copy_stream, P, nseg);
        } else {
            const dim3 cgrid((unsigned)std::min<long>((long)h->copy_blocks, (long)n * P.bands));
            hipLaunchKernelGGL((rbs::rbs_copy_kernel<1>), cgrid, block, 0, h->copy_stream, P);
        }
        RBS_HIP(h, hipGetLastError());
        if (!h->windowed || wide) {
            if (timed) RBS_HIP(h, hipEventRecord(h->ev_copy_stop[tslot], h->copy_stream));
            RBS_HIP(h, hipEventRecord(h->ev_join[slot], h->copy_stream));
        }
    } else {
        if (!split) launch_raster(h, false, rgrid, block, rbs::smem_bytes(P.tile_px, f64, h->many_clusters, h->exact), s, P);
        RBS_HIP(h, hipGetLastError());
        if (timed) RBS_HIP(h, hipEventRecord(h->ev_raster_stop[tslot], s));
    }
    if (timed) { RBS_HIP(h, hipEventRecord(h->ev_stop[tslot], s)); h->timed_calls += 1; }
    if (h->fr.cur >= 0 && s != h->stream) {
        // the staging image is released on the handle's stream: keep that stream behind its readers
        RBS_HIP(h, hipEventRecord(h->ev_reader, s));
        RBS_HIP(h, hipStreamWaitEvent(h->stream, h->ev_reader, 0));
    }
    if (stp_leaving) {   // from the next call on the planes are measured against the scalar background again
        h->stp = false;
        h->stp_block_until = h->calls + 4000;
        h->area_frac = 1.0;   // (what the last sample said: the next calls take the whole-plane machinery at once)
        h->wide = !h->slab_px && !h->exact;
    }
    if (update && !fused) h->join_pending = slot;   // joined lazily: by the next call, or by drain()
    if (h->group) {
        // other shards read this shard's planes: one event that covers both streams of this call
        if (h->join_pending >= 0) {
            RBS_HIP(h, hipStreamWaitEvent(s, h->ev_join[h->join_pending], 0));
            h->join_pending = -1;
        }
        RBS_HIP(h, hipEventRecord(h->ev_done, s));
    }
    h->calls += 1;
    if (update) {
        h->cur = 1 - h->cur;
        h->update_clock += h->pending_frames;
        h->pending_frames = 0;
        h->background = P.bg_new;
    }
    return RBS_OK;
}

}  // namespace
