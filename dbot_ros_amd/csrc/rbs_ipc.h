// rbs_ipc.h -- one process per GPU, host side: planes exported and attached over HIP IPC (rbs_ipc_export, rbs_ipc_attach), windows
// staged from the other ranks' planes (rbs_stage_windows), resampling across ranks (rbs_peer_resample; kernels: rbsensor_peers.hip).
// Not a header to include elsewhere: a section of rbsensor_capi.hip's translation unit, included there once INSIDE its extern "C"
// block of sensor entry points (these are four of them).

// ---- one process per GPU: the handles of the other ranks, mapped (include/rbsensor_mi355x.h) ----
namespace {
struct IpcBlob {
    uint32_t magic;
    int32_t device, max_particles, rows, cols, slab_px, windowed, cur, exact;
    int64_t plane_stride;
    hipIpcMemHandle_t mem[6];   // occ[0], occ[1], win[0], win[1], reg[0], reg[1] (reg: slabs only)
};
static_assert(sizeof(IpcBlob) <= RBS_IPC_BLOB_BYTES, "RBS_IPC_BLOB_BYTES");
constexpr uint32_t kIpcMagic = 0x52425331u;
}

int32_t rbs_ipc_export(rbs_handle* h, void* blob_out)
{
    if (!h || !blob_out) return RBS_ERR_INVALID_ARGUMENT;
    if (!h->shards.empty()) return fail(h, RBS_ERR_UNSUPPORTED, "ipc_export: a handle over several devices already shares its planes in-process");
    RBS_HIP(h, hipSetDevice(h->device));
    if (h->stp) return fail(h, RBS_ERR_UNSUPPORTED, "ipc_export: the handle already stores its planes against a shared background plane of its own "
                                                    "(windows grew past the shared-trail threshold): rbs_reset first, then export");
    h->ipc_exported = true;   // (other ranks read these planes in place: from now on the shared trail is entered / re-based / left only when the
                              //  caller says so, on every rank alike -- rbs_shared_trail_rebase)
    if (int32_t rc = drain(h, true)) return rc;
    std::memset(blob_out, 0, RBS_IPC_BLOB_BYTES);
    IpcBlob b{};
    b.magic = kIpcMagic;
    b.device = h->device; b.max_particles = h->max_particles; b.rows = h->rows; b.cols = h->cols;
    b.slab_px = h->slab_px; b.windowed = h->windowed ? 1 : 0; b.cur = h->cur; b.plane_stride = (int64_t)h->plane_stride; b.exact = h->exact ? 1 : 0;
    void* bufs[6] = {h->d_occ[0], h->d_occ[1], h->d_win[0], h->d_win[1], h->d_reg[0], h->d_reg[1]};
    for (int k = 0; k < 6; ++k)
        if (bufs[k]) RBS_HIP(h, hipIpcGetMemHandle(&b.mem[k], bufs[k]));
    std::memcpy(blob_out, &b, sizeof(b));
    return RBS_OK;
}

int32_t rbs_ipc_attach(rbs_handle* h, int32_t rank, int32_t world, const void* blobs)
{
    if (!h || !blobs) return RBS_ERR_INVALID_ARGUMENT;
    if (!h->shards.empty()) return fail(h, RBS_ERR_UNSUPPORTED, "ipc_attach: a handle over several devices already shares its planes in-process");
    if (world < 1 || world > rbs::kMaxDevices || rank < 0 || rank >= world)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("ipc_attach: rank %d of %d (at most %d ranks)", rank, world, rbs::kMaxDevices));
    if (h->peer_world > 1) return fail(h, RBS_ERR_INVALID_ARGUMENT, "ipc_attach: already attached");
    if (h->stp) return fail(h, RBS_ERR_UNSUPPORTED, "ipc_attach: the handle stores its planes against a shared background plane already: rbs_reset first");
#ifdef RBS_TEST_HOOKS   // (librbsensor_mi355x_hooks.so only) RBS_TEST_ATTACH_HANG=1: the call never returns -- what hipIpcOpenMemHandle was
                        // seen to do for some buffer sizes; tests/test_gpu_fullsize.py checks that bench.py --gpus N still prints its line
    if (const char* e = std::getenv("RBS_TEST_ATTACH_HANG"))
        if (std::atoi(e) != 0) for (;;) ::usleep(1000000);
#endif
    if ((long)world * h->max_particles > 0x7fffffffL) return fail(h, RBS_ERR_INVALID_ARGUMENT, "ipc_attach: too many global slots");
    RBS_HIP(h, hipSetDevice(h->device));
    if (int32_t rc = drain(h, true)) return rc;
    const unsigned char* raw = static_cast<const unsigned char*>(blobs);
    for (int k = 0; k < world; ++k) {
        IpcBlob b;
        std::memcpy(&b, raw + (size_t)k * RBS_IPC_BLOB_BYTES, sizeof(b));
        if (b.magic != kIpcMagic) return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("ipc_attach: blob %d is not an rbs_ipc_export", k));
        if (b.max_particles != h->max_particles || b.rows != h->rows || b.cols != h->cols || b.slab_px != h->slab_px ||
            b.windowed != (h->windowed ? 1 : 0) || b.plane_stride != (int64_t)h->plane_stride || b.cur != h->cur || b.exact != (h->exact ? 1 : 0))
            return fail(h, RBS_ERR_INVALID_ARGUMENT,
                        fmt("ipc_attach: rank %d's handle differs (max_particles %d, %d x %d, slab %d px, %s planes, buffer %d) from this one "
                            "(%d, %d x %d, %d, %s, %d): every rank must create the same handle and be at the same point of its call sequence",
                            k, b.max_particles, b.cols, b.rows, b.slab_px, b.windowed ? "windowed" : "whole", b.cur, h->max_particles, h->cols,
                            h->rows, h->slab_px, h->windowed ? "windowed" : "whole", h->cur));
        if (k == rank) continue;
        if (b.device != h->device) {   // another GPU of the node: read over xGMI
            int can = 0;
            RBS_HIP(h, hipDeviceCanAccessPeer(&can, h->device, b.device));
            if (!can) return fail(h, RBS_ERR_UNSUPPORTED, fmt("ipc_attach: device %d cannot access device %d's memory (peer access)", h->device, b.device));
            const hipError_t e = hipDeviceEnablePeerAccess(b.device, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
                (void)hipGetLastError();
                return fail(h, RBS_ERR_HIP, fmt("hipDeviceEnablePeerAccess(%d -> %d): %s", h->device, b.device, hipGetErrorString(e)));
            }
            (void)hipGetLastError();
        }
        for (int m = 0; m < 6; ++m) {
            if (m >= 4 && !h->slab_px) break;
            void* p = nullptr;
            const hipError_t e = hipIpcOpenMemHandle(&p, b.mem[m], hipIpcMemLazyEnablePeerAccess);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                return fail(h, RBS_ERR_HIP, fmt("hipIpcOpenMemHandle(rank %d, buffer %d): %s", k, m, hipGetErrorString(e)));
            }
            h->peer_mapped[k][m] = p;
        }
        for (int c = 0; c < 2; ++c) {
            h->peer_occ[k][c] = static_cast<const float*>(h->peer_mapped[k][c]);
            h->peer_win[k][c] = static_cast<const int4*>(h->peer_mapped[k][2 + c]);
            h->peer_reg[k][c] = static_cast<const int4*>(h->peer_mapped[k][4 + c]);
        }
    }
    h->peer_world = world;
    h->peer_rank = rank;
    return RBS_OK;
}

int32_t rbs_stage_windows(rbs_handle* h, const int32_t* d_src_global, const int32_t* d_dst_local, int32_t n, void* stream)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!h->shards.empty()) return fail(h, RBS_ERR_UNSUPPORTED, "stage_windows: a handle over several devices reads every parent in place");
    if (!h->windowed || (h->cols & 3))
        return fail(h, RBS_ERR_UNSUPPORTED, "stage_windows: windowed planes only (state_layout dense moves whole planes: rbs_export/import_plane)");
    if (n < 0 || n > h->max_particles || (n > 0 && (!d_src_global || !d_dst_local)))
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("stage_windows: n = %d outside 0..%d, or a null pointer", n, h->max_particles));
    if (n == 0) return RBS_OK;
    RBS_HIP(h, hipSetDevice(h->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    if (h->join_pending >= 0) RBS_HIP(h, hipStreamWaitEvent(s, h->ev_join[h->join_pending], 0));
    DevParams P = h->base;
    P.slots = h->max_particles; P.n_dev = 1; P.shard_cap = h->max_particles;
    P.slab_px = h->slab_px; P.plane_stride = (int)h->plane_stride;
    P.exact = h->exact ? 1 : 0; P.plane_px = h->slab_px ? h->slab_px : h->npx;
    P.occ_src = h->d_occ[h->cur]; P.win_src = h->d_win[h->cur]; P.reg_src = h->d_reg[h->cur];
    if (h->peer_world > 1) {
        P.n_dev = h->peer_world;
        P.slots = h->peer_world * h->max_particles;
        for (int k = 0; k < P.n_dev; ++k) {
            P.occ_src_dev[k] = k == h->peer_rank ? h->d_occ[h->cur] : h->peer_occ[k][h->cur];
            P.win_src_dev[k] = k == h->peer_rank ? h->d_win[h->cur] : h->peer_win[k][h->cur];
            P.reg_src_dev[k] = k == h->peer_rank ? h->d_reg[h->cur] : h->peer_reg[k][h->cur];
        }
    }
    hipLaunchKernelGGL(rbs::rbs_stage_kernel, dim3((unsigned)n, 4), dim3(256), 0, s, P, d_src_global, d_dst_local, h->d_occ[h->cur],
                       h->d_win[h->cur], h->d_reg[h->cur]);
    RBS_HIP(h, hipGetLastError());
    return RBS_OK;
}

int32_t rbs_peer_resample(rbs_handle* h, const double* d_loglik_all, const double* d_uniforms_sorted, int32_t n_total, int32_t n_local,
                          int32_t rank, int32_t min_share, double temperature, int32_t* d_parent_idx, int32_t* d_stage_src,
                          int32_t* d_stage_dst, int32_t* d_parents_local, int64_t* d_counts, void* stream)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!h->shards.empty()) return fail(h, RBS_ERR_UNSUPPORTED, "peer_resample: a handle over several devices resamples inside rbs_tracker_*");
    if (n_local <= 0 || n_total < n_local || n_total % n_local != 0 || rank < 0 || rank >= n_total / n_local)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("peer_resample: n_total = %d is not world x n_local = %d with rank %d inside it", n_total, n_local, rank));
    if (2 * (long)n_local > (long)h->max_particles)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("peer_resample: n_local = %d needs max_particles >= %d (own slots + staging slots), have %d",
                                                      n_local, 2 * n_local, h->max_particles));
    if (h->peer_world > 1 && (h->peer_world != n_total / n_local || h->peer_rank != rank))
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("peer_resample: rank %d of %d, but the handle is attached as rank %d of %d", rank, n_total / n_local,
                                                      h->peer_rank, h->peer_world));
    if (!d_loglik_all || !d_uniforms_sorted || !d_parent_idx || !d_stage_src || !d_stage_dst || !d_counts)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "peer_resample: null pointer");
    if (!(temperature > 0.0) || min_share < 1) return fail(h, RBS_ERR_INVALID_ARGUMENT, "peer_resample: temperature must be > 0, min_share >= 1");
    RBS_HIP(h, hipSetDevice(h->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    const int tiles = (n_total + rbp::kTile - 1) / rbp::kTile;
    if (tiles > rbp::kMaxTiles) return fail(h, RBS_ERR_UNSUPPORTED, fmt("peer_resample: n_total = %d exceeds %d particles", n_total, rbp::kMaxTiles * rbp::kTile));
    const size_t need = sizeof(double) * ((size_t)n_total + 2 * (size_t)tiles + 1) + 2 * sizeof(int) * (size_t)n_local;
    if (need > h->peer_scratch_bytes) {   // (first call, or a larger job: the only synchronising path)
        RBS_HIP(h, hipStreamSynchronize(s));
        (void)hipFree(h->d_peer_scratch);
        h->d_peer_scratch = nullptr;
        h->peer_scratch_bytes = 0;
        RBS_HIP(h, hipMalloc(&h->d_peer_scratch, need));
        h->peer_scratch_bytes = need;
    }
    rbp::PeerPlan Q;
    Q.ll_all = d_loglik_all; Q.uniforms = d_uniforms_sorted;
    Q.N = n_total; Q.n = n_local; Q.rank = rank; Q.cap = h->max_particles; Q.min_share = min_share;
    Q.temperature = temperature;
    Q.cdf = static_cast<double*>(h->d_peer_scratch);
    Q.tile_max = Q.cdf + n_total;
    Q.tile_total = Q.tile_max + tiles;
    Q.max_all = Q.tile_total + tiles;
    Q.mine = reinterpret_cast<int*>(Q.max_all + 1);
    Q.aux = Q.mine + n_local;
    Q.parent_idx = d_parent_idx; Q.stage_src = d_stage_src; Q.stage_dst = d_stage_dst;
    Q.parents_local = d_parents_local;
    Q.counts = reinterpret_cast<long long*>(d_counts);
    h->peer_last = Q;
    h->peer_last_stream = s;
    h->peer_last_max = tiles > rbp::kOwnMaxTiles;
    // (every launch is checked where it is made: a refused launch must name its kernel, not surface at the last one -- VERDICT r4 #7)
    if (tiles > rbp::kOwnMaxTiles) {
        hipLaunchKernelGGL(rbp::peer_max_kernel, dim3(tiles), dim3(rbp::kThreads), 0, s, Q);
        RBS_HIP(h, hipGetLastError());
    }
    hipLaunchKernelGGL(rbp::peer_weights_kernel, dim3(tiles), dim3(rbp::kThreads), 0, s, Q);
    RBS_HIP(h, hipGetLastError());
    hipLaunchKernelGGL(rbp::peer_search_kernel, dim3((unsigned)((n_local + rbp::kThreads - 1) / rbp::kThreads)), dim3(rbp::kThreads), 0, s, Q);
    RBS_HIP(h, hipGetLastError());
    hipLaunchKernelGGL(rbp::peer_resample_kernel, dim3(1), dim3(rbp::kThreads), 0, s, Q);
    RBS_HIP(h, hipGetLastError());
    return RBS_OK;
}
