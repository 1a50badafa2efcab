// rbs_handle.h -- what every part of the C-API's host side shares: the handle (struct rbs_handle), RCCL's entry points, the error
// helpers and macros (fmt, fail, RBS_HIP, RBS_REFUSE_POISONED), upload, and with_flags, which picks a kernel's instantiation.
// Part of rbsensor_capi.hip's translation unit (included from there, after the kernels).
#pragma once

using rbs::DevParams;

static_assert(sizeof(rbs_config) == 216 && offsetof(rbs_config, state_slab_px) == 208 && offsetof(rbs_config, likelihood_precision) == 184 &&
                  offsetof(rbs_config, device_ids) == 200,
              "rbs_config layout (ABI 2) is mirrored by dbot_ros_amd/_capi.py and tests/test_capi_cpu.py");

#ifndef RBS_TRACKER_SPLIT_MAX_DEFAULT
#define RBS_TRACKER_SPLIT_MAX_DEFAULT 5000   // (measured, tests/cpp/host_bench --tracker: frame by frame +12-16 % at 1 000-2 000 particles, +6-10 % at 4 000, nothing from 6 000 up)
#endif

struct rbs_handle {
    int device = 0;
    int rows = 0, cols = 0, npx = 0;
    int max_particles = 0;
    int n_bodies = 0;
    DevParams base{};           // static part of the kernel parameters
    double p_ov = 0, p_oo = 0, init_occ = 0, delta_time = 0;
    double* d_soup = nullptr;
    float* d_frame = nullptr;
    double* d_aux = nullptr;    // per-frame-pixel model terms, [npx][4] (precision F64), of a frame ingested from device memory
    double* d_aux_slot[2] = {nullptr, nullptr};   // ... of the host frame uploaded into d_fin[k] (computed on the upload stream)
    float* d_pbg = nullptr;
    float* d_occ[2] = {nullptr, nullptr};
    int cur = 0;
    int pending_frames = 0;     // set_observation calls since the last updating loglikes
    double* d_poses = nullptr;
    int* d_indices = nullptr;
    int* d_rects[2] = {nullptr, nullptr};  // [max_particles][4], alternating per call: the previous
                                // call's copy kernel may still be reading its rectangles
    rbs::Groups* d_groups[2] = {nullptr, nullptr};   // [max_particles] per-group rectangles (several bodies), alternating like d_rects
    rbs::Strips* d_strips[2] = {nullptr, nullptr};   // [max_particles] the copy kernel's cells outside the groups' rectangles (windowed planes), alternating alike
    int tracker_split_max = RBS_TRACKER_SPLIT_MAX_DEFAULT;   // rbs_tracker_*: see RBS_OPT_TRACKER_SPLIT_MAX
    bool copy_walk = false;                          // RBS_COPY_WALK=1 (tooling / A-B): several bodies take the walk over the whole region instead
    int* d_parents[2] = {nullptr, nullptr};   // [max_particles] snapshot of the caller's indices, alternating like d_rects
    int4* d_win[2] = {nullptr, nullptr};   // [max_particles] window of each plane, per buffer
    int4* d_win_used = nullptr; // [max_particles] region the copy kernel writes this call
    // window-sized slabs (rbs_config.state_slab_px): a slot holds slab_px floats and the stored region
    // of its plane; 0 = whole planes
    int slab_px = 0;
    size_t plane_stride = 0;    // floats per slot: npx or slab_px
    int4* d_reg[2] = {nullptr, nullptr};   // [max_particles] stored region of each plane, per buffer
    int* d_err = nullptr;       // [2] device: [0] a region did not fit its slab, [1] the largest region asked for so far (px)
    int* h_err = nullptr;       // pinned copy, fetched with the log-likelihoods ([2], [3]: the flags as they were BEFORE the call)
    bool slab_auto = false;     // the slab size is the library's choice (rbs_config.state_slab_px == 0 with many particles)
    bool slab_probed = false;   // ... and has been checked against a first call's regions (rbs_loglikes_device, probe_auto_slabs)
    int* d_bbox = nullptr;      // [4] scratch of rbs_import_plane / rbs_set_occlusion
    bool windowed = true;       // planes valid inside their window only (state_layout dense: whole plane)
    bool many_clusters = false; // a body of more than 256 clusters: the rbs_raster_kernel_many_* instantiations (shared cluster cull)
    // windowed planes whose windows have grown to a large part of the frame are served like whole
    // planes (streaming copy kernel beside two raster blocks per CU); the stored area is sampled
    // on the device every timing_every-th updating call and read back without blocking
    unsigned char* d_wide_flags = nullptr;   // [max_particles][copy blocks per plane], allocated on first use
    unsigned long long* d_area = nullptr;
    unsigned long long* h_area = nullptr;   // pinned
    hipEvent_t ev_area = nullptr;
    bool area_pending = false;
    int area_n = 0;
    bool wide = false;
    double area_frac = 0.0;     // last sampled stored-window area / frame area
    static constexpr double mid_enter = 0.15;    // above it: two raster blocks per CU, so the windowed copy runs beside them
    // Raster / copy balance: the windowed copy kernel runs beside the persistent raster blocks and
    // a call ends when the later of the two does.  When the copy kernel outlasts the raster kernel
    // (several bodies far apart: one window spans them and the copy fills the gaps) the next calls
    // run a few raster blocks fewer, and take them back when the raster kernel is the later one
    // again.  Decided from the kernel timers of the last timed call; the results do not depend on
    // the number of blocks.
    int balance_blocks = 0;     // current grid of the raster kernel (0: raster_blocks)
    long balance_seen = 0;      // timed_calls the rule has looked at
    double wide_enter = 0.50, wide_leave = 0.35;   // measured: the streaming copy wins from about half the frame
    int cu_count = 256;
    int smalln_target = 768;    // few particles: aim at about this many work items per call
    static constexpr int win_chunks = 8;         // row chunks (blocks) per particle of the windowed copy kernel (several bodies: it walks the whole window)
    static constexpr int win_chunks_single = 2;  // ... one body: it enumerates only the cells outside the rectangle, a tenth of the window
    int upload_chunks = 2;      // pieces a caller's host frame is staged and sent in (RBS_UPLOAD_CHUNKS) ...
    bool quiet = false;         // ... while nothing long of this handle's is running on the device (set by the entry points that
                                // wait for results, cleared by every launch): behind a running raster kernel the second piece's
                                // hand-over waits for that kernel (measured: pipelined tracker 3 750 -> 1 880 frames/s)
    bool async_outstanding = false;   // rbs_loglikes_device calls since the last rbs_synchronize (possibly on the caller's streams)
    float background = 0.f;     // never-covered occlusion level of the current buffer
    int2* d_item_range = nullptr;   // [max_particles] work items of each particle
    int* d_item_particle = nullptr; // [partial_cap] owner of each work item
    int* d_ctr = nullptr;           // [4] work-item counters of even / odd calls (+ [2] the split launch's likelihood-kernel tickets)
    // Split launch (round 5): geometry kernel -> depth tiles in memory -> likelihood kernel, each with its own occupancy
    // (rbsensor_kernels.hip, rbs_depth_kernel / rbs_eval_kernel).  rbs_config has no field for it: RBS_SPLIT in the
    // environment at rbs_create (tooling / A-B), otherwise the library's choice below.
    // Shared trail (round 5): a plane equals a handle-wide background PLANE outside its window instead of a scalar level.  A
    // pixel stays in a window ~730 frames after the object left it, and every child inherits that trail from its parent: with
    // resampling the particles soon share it from a common ancestor, and it was stored, read and stepped once per PARTICLE per
    // frame (a sweeping object: windows of 85 % of the frame, 2.2 M particle-likelihoods/s where the headline has 10.5).  Once
    // the sampled window area exceeds stp_enter the handle switches: the shared plane starts as the scalar background everywhere
    // and is RE-BASED on one particle's plane (inside that plane's window its values), every child of that call is re-measured
    // against it (its window shrinks to where it really differs), and so again every stp_every updating calls while windows
    // are large.  Values are unchanged bit for bit (the plane steps with the same float operations as any stored value); only
    // what is stored changes.  Single-device handles (whole planes or slabs), binary64 likelihood; RBS_SHARED_TRAIL=0 disables.
    bool stp = false, stp_allowed = true;
    float* d_bgp[2] = {nullptr, nullptr};   // [npx] the shared plane of either buffer (indexed like d_occ: by `cur`)
    double stp_enter = 0.10;
    int stp_every = 32;
    long stp_last_rebase = -1000000;
    long stp_rebases = 0;
    long stp_block_until = 0;               // re-basing did not shrink the windows (particles that share no ancestor): not again before this call
    // Round 6: the shared trail on handles whose planes OTHERS read in place.  The planes of every shard of a group (every rank of
    // an attached job) are stored against ONE shared plane, of which every device keeps its own identical copy: it starts as the
    // scalar level everywhere, steps with the same operations on every device, and is re-based by all of them in the SAME call on
    // the SAME global slot (a shard reads that slot's plane from its owner, in place) -- so "outside its window" means the same
    // values whichever device asks.  A group takes ONE decision per call for all its shards (group_begin_call, from the largest
    // window fraction any shard has sampled); attached ranks are told by their caller (rbs_shared_trail_rebase: the same call on
    // every rank before the same step), who has the collective to agree on it.
    struct StpNow { int rebase = -1; bool entering = false; } stp_now;   // group: this call's directive to the shards
    bool stp_leave_pending = false;         // group: the call in flight leaves the shared trail (the group's own state follows at the next call)
    int stp_request = -1;                   // rbs_shared_trail_rebase: >= 0 re-base on that GLOBAL slot at the next updating call (entering if need be), -2: leave
    bool ipc_exported = false;              // other processes may map this handle's planes (rbs_ipc_export): it no longer switches on its own
    int4* d_bgp_box = nullptr;              // [1] bounding box of the shared plane's values that differ from the scalar background
    bool split = false;
    unsigned* d_depth = nullptr;    // [depth_items][kDepthTilePx]
    size_t depth_items = 0;
    int depth_blocks = 0, eval_blocks = 0;   // the two persistent grids
    int* d_done = nullptr;      // [max_particles] finished work items per particle
    double* d_partial = nullptr; // [partial_cap] per-item partial sums
    unsigned long long* d_phase = nullptr;  // RBS_PHASE_TIMING builds
    size_t partial_cap = 0;
    float* d_cluster_sphere = nullptr;
    float* d_cluster_cone = nullptr;
    double* d_cluster_vtx = nullptr;   // [clusters][3][64] unique vertices of each cluster (vertex sharing)
    int* d_cluster_nv = nullptr;       // [clusters]
    unsigned* d_tri_local = nullptr;   // [n_tri] positions of a triangle's vertices in its cluster's list
    float* d_vtx = nullptr;         // [sum of vertex counts][4] float32 vertices (screen rectangles)
    float* d_tri_plane = nullptr;   // [n_tri][4] model-space plane of each triangle (float32 pre-cull)
    int precision = RBS_PRECISION_F64;
    // Stamped planes (rbs_config.occlusion_mode = RBS_OCC_REFERENCE; DevParams::exact): a slot is plane_px floats + plane_px
    // 16-bit ages, plane_stride floats in all.
    bool fused_copy = true;         // windowed copy inside the raster kernel where it applies (RBS_FUSED_COPY=0, tooling / A-B: the side-stream kernel)
    bool exact = false;
    int age_max = 0;            // ages beyond it are background
    double* d_ptab = nullptr;   // [age_max + 1][2] the propagation table
    std::vector<double> ptab;   // ... its host copy
    long update_clock = 0;      // frames between rbs_reset and the last updating call: the planes' epoch
    float* d_tmp_plane = nullptr;   // [npx] scratch of the plane hooks (the shared plane's effective values)
    float* d_render = nullptr;
    // pinned staging of the host-pointer API: poses | indices in one block (one H2D copy), the
    // log-likelihoods in another, and the event the caller waits on (the out copy alone -- the
    // planes' copy kernel on the second stream is joined by the next call, as in the device API)
    unsigned char* h_in = nullptr;
    double* h_out = nullptr;
    unsigned char* d_in = nullptr;     // device image of h_in
    unsigned char* h_in_dev = nullptr; // h_in / h_out as the device addresses them (kernels read / write them in place)
    double* h_out_dev = nullptr;
    size_t in_idx_off = 0;             // byte offset of the indices inside h_in / d_in
    hipEvent_t ev_out = nullptr;
    float* h_frames[2] = {nullptr, nullptr};   // pinned frame staging, alternating
    float* h_frames_dev[2] = {nullptr, nullptr};   // ... as the device addresses them
    static constexpr size_t frame_pull_bytes = 128 * 1024;   // frames up to this size are read from the staging buffer by a kernel
    hipEvent_t ev_frame[2] = {nullptr, nullptr};   // the upload out of h_frames[k] into d_fin[k] has finished
    // Host frames travel on their own stream into one of two device staging buffers, and the launch
    // stream only waits for the upload where it ingests the frame: a frame handed over while the
    // previous frame's kernels are still running (rbs_tracker_submit) is uploaded beside them.
    hipStream_t up_stream = nullptr;
    float* d_fin[2] = {nullptr, nullptr};
    hipEvent_t ev_used[2] = {nullptr, nullptr};    // the readers of d_fin[k] have been enqueued up to here
    hipEvent_t ev_reader = nullptr;                // orders the handle's stream after a reader on a caller's stream
    // The observation and the frame on its way to becoming it (only the frame section of this file touches them).  A host
    // frame needs no ingest on the launch stream (F64: its per-pixel terms are computed behind the copy, into d_aux_slot[k]):
    // the staging image d_fin[cur] IS the observation, and only the raster kernel waits for its upload.  cur = -1: d_frame,
    // where a device frame is ingested.  `next` holds at most ONE frame -- every hand-over stages, ingests or abandons the one
    // before it: a borrowed host frame or a device frame whose ingest rides on the next loglikes on `stream` (both counted by
    // the model clock), or a frame uploaded AHEAD into staging image `slot`, waiting beside the observation.
    struct NextFrame {
        enum Kind { NONE, BORROWED_F64, BORROWED_F32, DEVICE, AHEAD } kind = NONE;
        const void* src = nullptr;      // BORROWED_*, DEVICE
        hipStream_t stream = nullptr;   // DEVICE
        int slot = -1;                  // AHEAD
        bool borrowed() const { return kind == BORROWED_F64 || kind == BORROWED_F32; }
    };
    struct FrameState {
        int cur = -1;             // staging image that is the observation, -1: d_frame
        int stage = 0;            // pinned image (h_frames) the next host frame is staged in
        bool acquired = false;    // rbs_acquire_frame_buffer without its rbs_commit_frame_buffer yet
        NextFrame next;
    } fr;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;   // the copy kernel runs here, beside the raster kernel
    hipEvent_t ev_fork = nullptr;
    static constexpr int copy_blocks = 1 << 30;  // cap on the copy grid (one block per (particle, band) below it)
    int raster_blocks = 768;    // persistent raster grid: 3 per CU
    // timing ring: HIP events around the whole call (on the launch stream) and around the copy
    // kernel (on the copy stream) for the last kRing loglikes calls
    static constexpr int kRing = 256;
    hipEvent_t ev_start[kRing] = {}, ev_stop[kRing] = {}, ev_copy_start[kRing] = {}, ev_join[kRing] = {};
    hipEvent_t ev_raster_start[kRing] = {}, ev_raster_stop[kRing] = {}, ev_copy_stop[kRing] = {};
    bool ring_update[kRing] = {};
    // every event is a packet the stream must retire between two kernels: only every
    // timing_every-th call carries the timing events (ring slots count TIMED calls); ev_join, which
    // orders later work after the copy kernel, is recorded on every updating call
    int timing_every = 8;
    long timed_calls = 0;
    long calls = 0;
    int join_pending = -1;      // ring slot whose copy kernel later work on the planes must wait for
    std::string err;
    // A call that failed half-way through a fan-out (some shards enqueued, others not) or between a
    // tracker's buffer swaps leaves the handle's double buffers out of step: every later call is
    // refused with this message until rbs_reset (rbs_tracker_initialize) re-establishes a known state.
    bool poisoned = false;
    std::string poison_msg;
    // test hook, builds with -DRBS_TEST_HOOKS only (tests/test_gpu_multidevice.py): RBS_TEST_FAULT="<shard>:<call>" read at rbs_create makes
    // the group's <call>-th rbs_loglikes fail on shard <shard> after the shards before it were enqueued
    int fault_shard = -1;
    long fault_call = -1, group_calls = 0;
    // ---- several devices in one handle (rbs_config.n_devices > 1) ----
    // A GROUP handle owns one single-device handle ("shard") per device; global slot g lives on
    // shard g / shard_cap.  Every call is fanned out to the shards by the calling thread; a
    // shard's kernels read parents that live on other shards in place (peer access).
    std::vector<rbs_handle*> shards;   // group: its shards
    rbs_handle* group = nullptr;       // shard: its group
    int shard_index = 0;
    int shard_cap = 0;                 // global slots per device
    hipEvent_t ev_done = nullptr;      // shard: its last loglikes call has finished, planes included
    struct Rccl* rccl = nullptr;       // group: communicators for the log-likelihood all-gather (device tracker)
    // ---- particle sharding across PROCESSES (rbs_ipc_attach): the other ranks' plane buffers, window and
    // region tables mapped into this process; rank r owns global slots [r * max_particles, ...)
    int peer_world = 0, peer_rank = 0;
    const float* peer_occ[rbs::kMaxDevices][2] = {};
    const int4* peer_win[rbs::kMaxDevices][2] = {};
    const int4* peer_reg[rbs::kMaxDevices][2] = {};
    void* peer_mapped[rbs::kMaxDevices][6] = {};    // what hipIpcCloseMemHandle gets back
    void* d_peer_scratch = nullptr;                 // rbs_peer_resample: cdf [N] + 2 x [tiles] + 1 doubles + 2 x [n] ints
    size_t peer_scratch_bytes = 0;
    rbp::PeerPlan peer_last{};                      // ... its last call: the job and its views of the scratch block, the stream it went
    hipStream_t peer_last_stream = nullptr;         //   to, whether peer_max_kernel ran (N = 0: no call yet; read by the test build's
    bool peer_last_max = false;                     //   rbs_test_peer_scratch alone)
    const float* snap_occ[rbs::kMaxDevices] = {};   // group: every shard's CURRENT planes / windows as of the start
    const int4* snap_win[rbs::kMaxDevices] = {};    //   of the call being fanned out (shards flip buffers one by one)
    const int4* snap_reg[rbs::kMaxDevices] = {};
    // ---- the object finder (rbsensor_find.hip) builds its scoring handles from the sensor's creation parameters
    rbs_config cfg{};                               // as passed to rbs_create; its pointers point into the copies below
    std::vector<double> cfg_vertices;
    std::vector<int32_t> cfg_vertex_counts, cfg_triangles, cfg_triangle_counts;
    int occ_slots = 0;          // occlusion slots allocated: 0 = max_particles; a finder's scoring handle keeps slot 0 only
                                // (it is only ever called with update = 0 and every index 0)
    // ---- the pose assessor (rbsensor_assess.hip): its planes, records and staging, allocated by the first rbs_assess_poses
    struct rbs_assess_state* assess = nullptr;
    // ---- the occlusion map (rbsensor_occmap.hip): its buffers, allocated by the first rbs_occlusion_mean / rbs_occlusion_bodies /
    // rbs_tracker_set_occlusion_map
    struct rbs_occmap_state* occmap = nullptr;
    // ---- the object map (rbsensor_objmap.hip): its buffers, allocated by the first rbs_object_map / rbs_object_segment /
    // rbs_tracker_set_object_map
    struct rbs_objmap_state* objmap = nullptr;
    // ---- the posterior modes (rbs_modes_api.h): its buffers, allocated by the first rbs_pose_modes
    struct rbs_modes_state* modes = nullptr;
    // ---- the pose refiner (rbs_refine_api.h): its planes, partial sums and staging, allocated by the first rbs_refine_poses
    struct rbs_refine_state* refine = nullptr;
    long frames_handed = 0;     // frames handed over since rbs_create (rbs_object_segment refuses a handle that never saw one)
};

// RCCL, bound at run time (dlopen): a single-device handle never needs it, and a process that
// already carries torch's copy of the library keeps exactly one.
struct Rccl {
    void* lib = nullptr;
    typedef void* comm_t;
    int (*CommInitAll)(comm_t*, int, const int*) = nullptr;
    int (*CommDestroy)(comm_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, comm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    std::vector<comm_t> comms;
};

namespace {

thread_local std::string g_create_error;

std::string fmt(const char* f, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, f);
    vsnprintf(buf, sizeof buf, f, ap);
    va_end(ap);
    return buf;
}

#define RBS_HIP(h, call)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            (void)hipGetLastError(); /* HIP's last error is sticky: it must not fail a later call */ \
            (h)->err = fmt("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__,   \
                           __LINE__);                                                         \
            return e_ == hipErrorOutOfMemory ? RBS_ERR_OUT_OF_MEMORY : RBS_ERR_HIP;           \
        }                                                                                     \
    } while (0)

int32_t fail(rbs_handle* h, int32_t code, const std::string& msg)
{
    h->err = msg;
    return code;
}

// One host array to a new device allocation of at least min_count elements.
template <class T>
int32_t upload(rbs_handle* h, T** dst, const std::vector<T>& src, size_t min_count = 0)
{
    RBS_HIP(h, hipMalloc(dst, sizeof(T) * std::max(src.size(), min_count)));
    RBS_HIP(h, hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
    return RBS_OK;
}

static_assert(rbs::kMeshMaxBodies == rbs::kMaxBodies, "rbs_mesh.h keeps its own copy of the kernels' body limit");
static_assert(rbs::kMeshOk == RBS_OK && rbs::kMeshInvalidArgument == RBS_ERR_INVALID_ARGUMENT, "rbs_mesh.h returns the C-ABI's codes");
#define RBS_REFUSE_POISONED(h)                                                                \
    do {                                                                                      \
        if ((h)->poisoned)                                                                    \
            return fail(h, RBS_ERR_HIP, "the handle is in an undefined state after a failed call (" + (h)->poison_msg + \
                                            "): call rbs_reset / rbs_tracker_initialize");    \
    } while (0)

// Run-time booleans to the template arguments of a kernel: with_flags(f, a, b, ...) calls f(A, B, ...) with std::true_type /
// std::false_type for each flag, in the order given, and returns what f returns.  In the generic lambda f, A() is a constant
// expression: f names the kernel once, as kernel<A(), B(), ...>, and every combination is instantiated (false before true, the
// first flag the slowest: the order of a case table keyed with the first flag as its highest bit).
template <class F>
auto with_flags(F&& f) { return f(); }
template <class F, class... R>
auto with_flags(F&& f, bool b, R... rest)
{
    if (!b) return with_flags([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
    return with_flags([&](auto... c) { return f(std::true_type{}, c...); }, rest...);
}

}  // namespace
