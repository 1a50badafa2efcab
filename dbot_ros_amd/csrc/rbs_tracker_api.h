// rbs_tracker_api.h -- the device tracker's host side: struct rbs_tracker, tfail / RBT_HIP / talloc, the launch_* helpers of the
// kernels in rbsensor_tracker.hip, tracker_create_one, group_tracker_track, tracker_submit_impl and the rbs_tracker_* entry points.
// Not a header to include elsewhere: a section of rbsensor_capi.hip's translation unit, included there once after the extern "C"
// block of sensor entry points (rbsensor_probes.hip, in the hooks library, uses the launch_* helpers).

struct rbs_tracker {
    const double* frame64 = nullptr;   // rbs_tracker_submit_f64: this submit's frame as doubles (tracker_submit_impl reads it instead of `frame`)
    std::vector<float> frame_tmp;      // ... converted here where a float frame is needed (a sensor over several devices)
    rbs_handle* s = nullptr;
    rbt::TrackerDev T{};
    std::vector<void*> allocs;
    double* d_normals = nullptr;   // staging for host-supplied randomness
    double* d_uniforms = nullptr;
    std::string err;
    // a sensor over several devices: one replica (all particle states + the filter's kernels) per
    // shard; `s` is then the group handle and T is unused
    std::vector<rbs_tracker*> reps;
    // pipelining (rbs_tracker_submit / rbs_tracker_result): up to two frames in flight; per slot the
    // host-supplied randomness (pinned staging + its device image) and the frame's result (pinned)
    double* h_normals[2] = {nullptr, nullptr};
    double* h_uniforms[2] = {nullptr, nullptr};
    double* d_normals2[2] = {nullptr, nullptr};
    double* d_uniforms2[2] = {nullptr, nullptr};
    double* h_state[2] = {nullptr, nullptr};
    int* h_flags[2] = {nullptr, nullptr};
    int* h_serr[2] = {nullptr, nullptr};
    hipEvent_t ev_res[2] = {nullptr, nullptr};
    double* h_state_dev[2] = {nullptr, nullptr};   // h_state / h_flags as the device addresses them
    int* h_flags_dev[2] = {nullptr, nullptr};
    int32_t res_rc[2] = {0, 0};       // (a handle over several devices runs submit synchronously)
    int res_seq[2] = {0, 0};          // the frame number the kernel that finishes slot k's frame stores into h_flags[k][2]
    long submitted = 0, collected = 0;
    bool recentre_pending = false;    // T.part_old still holds the particles before the last frame's re-centring
    bool poisoned = false;            // a frame failed half-way (buffers partly swapped): rbs_tracker_initialize first
    // the posterior report (rbs_tracker_set_posterior, rbsensor_posterior.hip): off by default.  Per in-flight frame a pinned
    // slot the frame's last kernels write ([1 + D + D D] doubles, then 4 ints) and the event recorded behind them;
    // rbs_tracker_result copies the slot into `post` / `post_i`, so the slot is free for the next-but-one submit.
    bool post_on = false, post_valid = false, post_ready = false;   // post_ready: every buffer and event below exists
    rbt::PostDev P{};
    double* h_post[2] = {nullptr, nullptr};
    double* h_post_dev[2] = {nullptr, nullptr};
    hipEvent_t ev_post[2] = {nullptr, nullptr};
    hipEvent_t ev_post0[2] = {nullptr, nullptr};   // in front of the report's first launch: its device time (rbs_tracker_posterior_ms)
    float post_ms = 0.f;
    std::vector<double> post;
    int32_t post_i[4] = {0, 0, 0, 0};
    // the posterior modes (rbs_tracker_set_modes, rbsensor_modes.hip): off by default, on the posterior report's pattern.  Per
    // in-flight frame a pinned slot of n_objects rbs_body_modes the frame's last kernel writes and the event recorded behind it;
    // rbs_tracker_result copies the slot into `modes`.  M: the parameters and the report's own device buffers.
    bool modes_on = false, modes_valid = false, modes_ready = false;   // modes_ready: every buffer and event below exists
    rbt::ModesDev M{};
    double* modes_work = nullptr;   // modes_doubles(n, bodies)
    int* modes_sel = nullptr;       // modes_ints(bodies)
    rbs_body_modes* h_modes[2] = {nullptr, nullptr};
    rbs_body_modes* h_modes_dev[2] = {nullptr, nullptr};
    hipEvent_t ev_modes[2] = {nullptr, nullptr};
    hipEvent_t ev_modes0[2] = {nullptr, nullptr};   // in front of the report's first launch: its device time (rbs_tracker_modes_ms)
    int modes_seq[2] = {0, 0};
    float modes_ms = 0.f;
    int32_t modes_frame = 0;
    std::vector<rbs_body_modes> modes;
    // the occlusion map (rbs_tracker_set_occlusion_map, rbsensor_occmap.hip): off by default.  Per in-flight frame a pinned
    // image the frame's last kernel writes and the event recorded behind it; rbs_tracker_result copies it into `map`.
    bool map_on = false, map_valid = false, map_ready = false;   // map_ready: every buffer and event below exists
    float* h_map[2] = {nullptr, nullptr};
    float* h_map_dev[2] = {nullptr, nullptr};
    hipEvent_t ev_map[2] = {nullptr, nullptr};
    hipEvent_t ev_map0[2] = {nullptr, nullptr};   // in front of the map's first launch: its device time (rbs_tracker_occlusion_map_ms)
    int map_seq[2] = {0, 0};                      // the frame number of the map in image k
    float map_ms = 0.f;
    int32_t map_frame = 0;
    std::vector<float> map;
    // the object map (rbs_tracker_set_object_map, rbsensor_objmap.hip): off by default, on the occlusion map's pattern.  An image
    // is [n_objects + 2][npx] floats: cover, depth, var.
    bool obj_on = false, obj_valid = false, obj_ready = false;
    float* h_obj[2] = {nullptr, nullptr};
    float* h_obj_dev[2] = {nullptr, nullptr};
    hipEvent_t ev_obj[2] = {nullptr, nullptr};
    hipEvent_t ev_obj0[2] = {nullptr, nullptr};
    int obj_seq[2] = {0, 0};
    float obj_ms = 0.f;
    int32_t obj_frame = 0;
    std::vector<float> obj;
};

namespace {
int32_t tfail(rbs_tracker* t, int32_t code, const std::string& msg) { t->err = msg; t->s->err = msg; return code; }

#define RBT_HIP(t, call)                                                                       \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            (void)hipGetLastError();                                                           \
            return tfail(t, e_ == hipErrorOutOfMemory ? RBS_ERR_OUT_OF_MEMORY : RBS_ERR_HIP,   \
                         fmt("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__)); \
        }                                                                                      \
    } while (0)

template <typename X>
int32_t talloc(rbs_tracker* t, X** p, size_t count)
{
    RBT_HIP(t, hipMalloc(p, sizeof(X) * (count ? count : 1)));
    t->allocs.push_back(*p);
    return RBS_OK;
}
}  // namespace

namespace {
// The filter step's weights and the tracker's mean: single-block kernels for few particles (the
// launch chain is what counts there), grid kernels from kMultiBlockFrom particles on.
void launch_weights(const rbt::TrackerDev& T, int updated, hipStream_t s)
{
    if (T.n < rbt::kMultiBlockFrom) {
        hipLaunchKernelGGL(rbt::weights_kernel, dim3(1), dim3(1024), 0, s, T, updated);
        return;
    }
    const int blocks = (T.n + rbt::kChunk - 1) / rbt::kChunk;
    hipLaunchKernelGGL(rbt::weights_w1_kernel, dim3((unsigned)blocks), dim3(1024), 0, s, T, updated);
    hipLaunchKernelGGL(rbt::weights_w2_kernel, dim3((unsigned)blocks), dim3(1024), 0, s, T);
    hipLaunchKernelGGL(rbt::weights_w3_kernel, dim3(1), dim3(64), 0, s, T, blocks);
    hipLaunchKernelGGL(rbt::weights_w4_kernel, dim3((unsigned)blocks), dim3(1024), 0, s, T);
}
void launch_mean(const rbt::TrackerDev& T, hipStream_t s)
{
    if (T.n < rbt::kMultiBlockFrom) {
        hipLaunchKernelGGL(rbt::mean_kernel, dim3(1), dim3(1024), 0, s, T);
        return;
    }
    const int blocks = (T.n + rbt::kChunk - 1) / rbt::kChunk;
    hipLaunchKernelGGL(rbt::mean_m1_kernel, dim3((unsigned)blocks), dim3(1024), 0, s, T);
    hipLaunchKernelGGL(rbt::mean_m2_kernel, dim3((unsigned)blocks), dim3(1024), 0, s, T);
    hipLaunchKernelGGL(rbt::mean_m3_kernel, dim3(1), dim3(64), 0, s, T, blocks);
}
// The other steps of a frame, each with its launch geometry in one place: rbs_tracker_submit, the
// tracker over several devices and the test build's filter probe (rbsensor_probes.hip) launch them
// through these.
inline dim3 per_particle_grid(const rbt::TrackerDev& T) { return dim3((unsigned)((T.n + 255) / 256)); }
void launch_propagate(const rbt::TrackerDev& T, int b, int recentre, hipStream_t s)
{
    hipLaunchKernelGGL(rbt::propagate_kernel, per_particle_grid(T), dim3(256), 0, s, T, b, recentre);
}
void launch_resample_gather(const rbt::TrackerDev& T, int b, hipStream_t s)
{
    hipLaunchKernelGGL(rbt::resample_gather_kernel, dim3((unsigned)T.n), dim3(64), 0, s, T, b);
}
void launch_gather(const rbt::TrackerDev& T, hipStream_t s)
{
    hipLaunchKernelGGL(rbt::gather_kernel, dim3((unsigned)T.n), dim3(64), 0, s, T);
}
void launch_filter_tail(const rbt::TrackerDev& T, int b, int updated, hipStream_t s)
{
    hipLaunchKernelGGL(rbt::filter_tail_kernel, dim3(1), dim3(1024), 0, s, T, b, updated);
}
void launch_filter_step(const rbt::TrackerDev& T, int b, int updated, int last, hipStream_t s)
{
    hipLaunchKernelGGL(rbt::filter_step_kernel, dim3(1), dim3(1024), 0, s, T, b, updated, last);
}
void launch_recentre(const rbt::TrackerDev& T, double* particles, hipStream_t s)
{
    hipLaunchKernelGGL(rbt::recentre_kernel, per_particle_grid(T), dim3(256), 0, s, T, particles);
}
// The posterior report of the population in `particles` (the frame's last launches; recentred: 0 = the re-centring is
// pending and T.mean holds what it needs -- one launch in front re-centres a copy of the poses): one block below
// kMultiBlockFrom particles, five grid launches from there on.
void launch_posterior(const rbt::TrackerDev& T, const rbt::PostDev& P, const double* particles, int recentred, hipStream_t s)
{
    if (!recentred) hipLaunchKernelGGL(rbt::rbs_post_recentre_kernel, per_particle_grid(T), dim3(256), 0, s, T, P, particles);
    if (T.n < rbt::kMultiBlockFrom) {
        hipLaunchKernelGGL(rbt::rbs_post_kernel, dim3(1), dim3(1024), 0, s, T, P, particles, recentred);
        return;
    }
    const unsigned blocks = (unsigned)rbt::post_blocks(T.n), G = (unsigned)(T.D / 6);
    hipLaunchKernelGGL(rbt::rbs_post_max_kernel, dim3(blocks), dim3(1024), 0, s, T, P);
    hipLaunchKernelGGL(rbt::rbs_post_sums_kernel, dim3(blocks), dim3(1024), 0, s, T, P, particles, recentred);
    hipLaunchKernelGGL(rbt::rbs_post_mean_kernel, dim3(1), dim3(1024), 0, s, T, P, (int)blocks);
    hipLaunchKernelGGL(rbt::rbs_post_cov_kernel, dim3(blocks, G * (G + 1)), dim3(1024), 0, s, T, P, particles, recentred);
    hipLaunchKernelGGL(rbt::rbs_post_cov_fold_kernel, dim3(1), dim3(1024), 0, s, T, P, (int)blocks);
}
// after a sampling block's gather: the gathered arrays are the block's result
void swap_gathered(rbt::TrackerDev& T)
{
    std::swap(T.part_old, T.part_old2);
    std::swap(T.part_new, T.part_new2);
    std::swap(T.noise, T.noise2);
    std::swap(T.ll, T.ll2);
    std::swap(T.idx, T.idx2);
}

// One device's tracker state.  cap > 0: the sensor is a shard of a group with `cap` slots per device.
int32_t tracker_create_one(rbs_handle* sensor, const rbs_tracker_params* p, int n_dev, int cap, rbs_tracker** out)
{
    RBS_HIP(sensor, hipSetDevice(sensor->device));
    rbs_tracker* t = new (std::nothrow) rbs_tracker;
    if (!t) return fail(sensor, RBS_ERR_OUT_OF_MEMORY, "tracker_create: out of host memory");
    t->s = sensor;
    rbt::TrackerDev& T = t->T;
    T.n = p->n_particles;
    T.parts = sensor->n_bodies;
    T.D = T.parts * rbt::kBody;
    for (int k = 0; k < 3; ++k) { T.sigma[k] = p->linear_sigma[k]; T.sigma[3 + k] = p->angular_sigma[k]; }
    T.vf = p->velocity_factor;
    T.max_kl = p->max_kl_divergence;
    const size_t n = (size_t)T.n, D = (size_t)T.D, P6 = (size_t)T.parts * 6;
    int32_t rc = RBS_OK;
    if ((rc = talloc(t, &T.part_old, n * D)) || (rc = talloc(t, &T.part_new, n * D)) ||
        (rc = talloc(t, &T.part_old2, n * D)) || (rc = talloc(t, &T.part_new2, n * D)) ||
        (rc = talloc(t, &T.noise, n * P6)) || (rc = talloc(t, &T.noise2, n * P6)) ||
        (rc = talloc(t, &T.logw, n)) || (rc = talloc(t, &T.ll, n)) || (rc = talloc(t, &T.ll2, n)) ||
        (rc = talloc(t, &T.ll_new, n)) || (rc = talloc(t, &T.idx, n)) || (rc = talloc(t, &T.idx2, n)) ||
        (rc = talloc(t, &T.parents, n)) || (rc = talloc(t, &T.cdf, n)) || (rc = talloc(t, &T.deflt, D)) ||
        (rc = talloc(t, &T.mean, D + (size_t)T.parts * 9)) || (rc = talloc(t, &T.poses, n * (size_t)T.parts * 12)) ||
        (rc = talloc(t, &T.flag, 2)) || (rc = talloc(t, &T.red, (size_t)rbt::kRedBlocks * (3 + D))) ||
        (rc = talloc(t, &t->d_normals, n * P6)) ||
        (rc = talloc(t, &t->d_uniforms, n * (size_t)T.parts)) ||
        (cap > 0 && ((rc = talloc(t, &T.layout, n)) || (rc = talloc(t, &T.ll_sorted, (size_t)n_dev * cap)) ||
                     (rc = talloc(t, &T.poses_sorted, (size_t)cap * T.parts * 12)) || (rc = talloc(t, &T.idx_sorted, (size_t)cap))))) {
        rbs_tracker_destroy(t);
        return rc;
    }
    if (hipMemsetAsync(T.deflt, 0, sizeof(double) * D, sensor->stream) != hipSuccess) {
        (void)hipGetLastError();
        rbs_tracker_destroy(t);
        return fail(sensor, RBS_ERR_HIP, "tracker_create: hipMemsetAsync failed");
    }
    t->d_normals2[0] = t->d_normals;
    t->d_uniforms2[0] = t->d_uniforms;
    if ((rc = talloc(t, &t->d_normals2[1], n * P6)) || (rc = talloc(t, &t->d_uniforms2[1], n * (size_t)T.parts))) {
        rbs_tracker_destroy(t);
        return rc;
    }
    for (int k = 0; k < 2; ++k) {
        if (hipHostMalloc(&t->h_normals[k], sizeof(double) * n * P6, hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc(&t->h_uniforms[k], sizeof(double) * n * T.parts, hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc(&t->h_state[k], sizeof(double) * D, hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc(&t->h_flags[k], sizeof(int) * 4, hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc(&t->h_serr[k], 2 * sizeof(int), hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&t->ev_res[k], hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            rbs_tracker_destroy(t);
            return fail(sensor, RBS_ERR_OUT_OF_MEMORY, "tracker_create: pinned host memory");
        }
        t->h_serr[k][0] = t->h_serr[k][1] = 0;
        t->h_flags[k][2] = 0;
        if (hipHostGetDevicePointer(reinterpret_cast<void**>(&t->h_state_dev[k]), t->h_state[k], 0) != hipSuccess ||
            hipHostGetDevicePointer(reinterpret_cast<void**>(&t->h_flags_dev[k]), t->h_flags[k], 0) != hipSuccess) {
            (void)hipGetLastError();
            rbs_tracker_destroy(t);
            return fail(sensor, RBS_ERR_HIP, "tracker_create: hipHostGetDevicePointer failed");
        }
    }
    *out = t;
    return RBS_OK;
}
}  // namespace

extern "C" {

int32_t rbs_tracker_create(rbs_handle* sensor, const rbs_tracker_params* p, rbs_tracker** out)
{
    if (!sensor || !out) return RBS_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    const int total = sensor->shards.empty() ? sensor->max_particles : (int)sensor->shards.size() * sensor->shard_cap;
    if (!p || p->n_particles <= 0 || p->n_particles > total)
        return fail(sensor, RBS_ERR_INVALID_ARGUMENT, "tracker_create: n_particles outside 1..max_particles");
    if (p->n_particles > rbt::kRedBlocks * rbt::kChunk)
        return fail(sensor, RBS_ERR_INVALID_ARGUMENT, fmt("tracker_create: at most %d particles", rbt::kRedBlocks * rbt::kChunk));
    if (sensor->shards.empty()) return tracker_create_one(sensor, p, 1, 0, out);
    rbs_tracker* g = new (std::nothrow) rbs_tracker;
    if (!g) return fail(sensor, RBS_ERR_OUT_OF_MEMORY, "tracker_create: out of host memory");
    g->s = sensor;
    for (rbs_handle* sh : sensor->shards) {
        rbs_tracker* r = nullptr;
        if (int32_t rc = tracker_create_one(sh, p, (int)sensor->shards.size(), sensor->shard_cap, &r)) {
            sensor->err = sh->err;
            rbs_tracker_destroy(g);
            return rc;
        }
        g->reps.push_back(r);
    }
    *out = g;
    return RBS_OK;
}

void rbs_tracker_destroy(rbs_tracker* t)
{
    if (!t) return;
    if (!t->reps.empty() || !t->s->shards.empty()) {
        for (rbs_tracker* r : t->reps) rbs_tracker_destroy(r);
        delete t;
        return;
    }
    (void)hipSetDevice(t->s->device);
    (void)hipStreamSynchronize(t->s->stream);
    for (void* p : t->allocs) (void)hipFree(p);
    for (int k = 0; k < 2; ++k) {
        if (t->h_normals[k]) (void)hipHostFree(t->h_normals[k]);
        if (t->h_uniforms[k]) (void)hipHostFree(t->h_uniforms[k]);
        if (t->h_state[k]) (void)hipHostFree(t->h_state[k]);
        if (t->h_flags[k]) (void)hipHostFree(t->h_flags[k]);
        if (t->h_serr[k]) (void)hipHostFree(t->h_serr[k]);
        if (t->ev_res[k]) (void)hipEventDestroy(t->ev_res[k]);
        if (t->h_post[k]) (void)hipHostFree(t->h_post[k]);
        if (t->ev_post[k]) (void)hipEventDestroy(t->ev_post[k]);
        if (t->ev_post0[k]) (void)hipEventDestroy(t->ev_post0[k]);
        if (t->h_modes[k]) (void)hipHostFree(t->h_modes[k]);
        if (t->ev_modes[k]) (void)hipEventDestroy(t->ev_modes[k]);
        if (t->ev_modes0[k]) (void)hipEventDestroy(t->ev_modes0[k]);
        if (t->h_map[k]) (void)hipHostFree(t->h_map[k]);
        if (t->ev_map[k]) (void)hipEventDestroy(t->ev_map[k]);
        if (t->ev_map0[k]) (void)hipEventDestroy(t->ev_map0[k]);
        if (t->h_obj[k]) (void)hipHostFree(t->h_obj[k]);
        if (t->ev_obj[k]) (void)hipEventDestroy(t->ev_obj[k]);
        if (t->ev_obj0[k]) (void)hipEventDestroy(t->ev_obj0[k]);
    }
    delete t;
}

int32_t rbs_tracker_initialize(rbs_tracker* t, const double* default_state)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (!default_state) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_initialize: null state");
    t->submitted = t->collected = 0;
    t->recentre_pending = false;
    t->poisoned = false;
    t->post_valid = false;
    t->modes_valid = false;
    t->map_valid = false;
    t->obj_valid = false;
    if (!t->reps.empty()) {
        for (rbs_tracker* r : t->reps)
            if (int32_t rc = rbs_tracker_initialize(r, default_state)) { t->s->err = r->s->err; return rc; }
        for (rbs_handle* sh : t->s->shards) {   // the shards' resets left their streams idle: a clean slate for the group's ordering
            RBT_HIP(t, hipSetDevice(sh->device));
            RBT_HIP(t, hipEventRecord(sh->ev_done, sh->stream));
        }
        t->s->poisoned = false;
        frame_abandon(t->s);
        return RBS_OK;
    }
    rbt::TrackerDev& T = t->T;
    RBT_HIP(t, hipSetDevice(t->s->device));
    if (int32_t rc = rbs_reset(t->s)) return rc;
    hipStream_t s = t->s->stream;
    RBT_HIP(t, hipMemcpyAsync(T.deflt, default_state, sizeof(double) * T.D, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(rbt::init_kernel, dim3((unsigned)((T.n + 255) / 256)), dim3(256), 0, s, T);
    RBT_HIP(t, hipGetLastError());
    RBT_HIP(t, hipStreamSynchronize(s));
    T.frame = 0;
    for (int k = 0; k < 2; ++k) { t->h_flags[k][2] = 0; t->res_seq[k] = 0; }   // frame numbers start over
    if (t->s->slab_px && !t->s->group) {
        // Window-sized slabs: a tracker frame that overflows cannot be repeated, so the slabs are sized
        // BEFORE the first frame -- one updating probe call of a single particle at the default pose
        // measures the object's screen rectangle, the housekeeping enlarges the slabs to hold it with
        // room to move, and the sensor is reset again.  From there on the regions grow a few pixels
        // per frame and the housekeeping at every frame's result keeps ahead of them.
        rbs_handle* h = t->s;
        hipLaunchKernelGGL(rbt::default_pose_kernel, dim3(1), dim3(64), 0, s, T);
        RBT_HIP(t, hipGetLastError());
        if (int32_t rc = enqueue_loglikes(h, T.poses, T.idx, 1, true, T.ll_new, s)) return rc;
        if (int32_t rc = drain(h, true)) return rc;
        RBT_HIP(t, hipMemcpy(h->h_err, h->d_err, 2 * sizeof(int), hipMemcpyDeviceToHost));
        if (int32_t rc = slab_housekeeping(h)) return rc;
        if (int32_t rc = rbs_reset(h)) return rc;
    }
    return RBS_OK;
}

}  // extern "C" (group_tracker_track below needs C++ linkage)

namespace {
// One frame on a sensor over several devices.  Every device runs the whole filter on all the
// particle states (identical inputs, identical code); the sensor call alone is sharded: device k
// evaluates the particles laid out at slots [k cap, (k+1) cap) (layout_kernel), and the
// log-likelihoods are exchanged with ONE all-gather per sampling block (RCCL over xGMI).
int32_t group_tracker_track(rbs_tracker* t, const float* frame, const double* normals, const double* uniforms,
                            uint64_t seed, double* out_state, int32_t* out_resamplings)
{
    rbs_handle* g = t->s;
    const int nd = (int)g->shards.size(), cap = g->shard_cap;
    if (frame)
        if (int32_t rc = rbs_set_observation_f32(g, frame, (size_t)g->npx)) return rc;
    std::vector<hipStream_t> streams(nd);
    std::vector<double*> llbufs(nd);
    for (int k = 0; k < nd; ++k) {
        rbs_tracker* r = t->reps[k];
        rbt::TrackerDev& T = r->T;
        rbs_handle* h = r->s;
        streams[k] = h->stream;
        llbufs[k] = T.ll_sorted;
        RBT_HIP(t, hipSetDevice(h->device));
        const size_t n = (size_t)T.n;
        T.normals = nullptr;
        T.uniforms = nullptr;
        if (normals) {
            RBT_HIP(t, hipMemcpyAsync(r->d_normals, normals, sizeof(double) * n * T.parts * 6, hipMemcpyHostToDevice, h->stream));
            T.normals = r->d_normals;
        }
        if (uniforms) {
            RBT_HIP(t, hipMemcpyAsync(r->d_uniforms, uniforms, sizeof(double) * n * T.parts, hipMemcpyHostToDevice, h->stream));
            T.uniforms = r->d_uniforms;
        }
        T.seed = seed;
    }
    const int parts = t->reps[0]->T.parts, n = t->reps[0]->T.n;
    const dim3 g256((unsigned)((n + 255) / 256)), b256(256);
    for (int b = 0; b < parts; ++b) {
        const bool last = b == parts - 1;
        for (int k = 0; k < nd; ++k) {
            rbs_tracker* r = t->reps[k];
            RBT_HIP(t, hipSetDevice(r->s->device));
            launch_propagate(r->T, b, 0, streams[k]);
            hipLaunchKernelGGL(rbt::layout_kernel, dim3(1), dim3(1024), 0, streams[k], r->T, nd, cap);
            const int lo = std::min(n, k * cap), cnt = std::min(n, (k + 1) * cap) - lo;
            if (cnt > 0)
                hipLaunchKernelGGL(rbt::shard_gather_kernel, dim3((unsigned)((cnt + 255) / 256)), b256, 0, streams[k], r->T, lo, cnt);
            RBT_HIP(t, hipGetLastError());
        }
        if (int32_t rc = group_begin_call(g, nullptr, last)) return rc;
        for (int k = 0; k < nd; ++k) {
            rbs_tracker* r = t->reps[k];
            rbs_handle* h = r->s;
            RBT_HIP(t, hipSetDevice(h->device));
            const int lo = std::min(n, k * cap), cnt = std::min(n, (k + 1) * cap) - lo;
            if (cnt > 0) {
                if (int32_t rc = enqueue_loglikes(h, r->T.poses_sorted, r->T.idx_sorted, cnt, last, r->T.ll_sorted + lo, h->stream))
                    return gfail(g, h, rc);
            } else {
                if (int32_t rc = advance_empty(h, last)) return gfail(g, h, rc);
                RBT_HIP(t, hipEventRecord(h->ev_done, h->stream));
            }
        }
        if (int32_t rc = group_allgather(g, llbufs.data(), (size_t)cap, streams.data())) return rc;
        for (int k = 0; k < nd; ++k) {
            rbs_tracker* r = t->reps[k];
            rbt::TrackerDev& T = r->T;
            RBT_HIP(t, hipSetDevice(r->s->device));
            hipStream_t s = streams[k];
            hipLaunchKernelGGL(rbt::shard_scatter_kernel, g256, b256, 0, s, T, last ? 1 : 0);
            launch_weights(T, 0, s);
            hipLaunchKernelGGL(rbt::resample_kernel, g256, b256, 0, s, T, b);
            launch_gather(T, s);
            RBT_HIP(t, hipGetLastError());
            swap_gathered(T);
        }
    }
    int flags[2] = {0, 0};
    for (int k = 0; k < nd; ++k) {
        rbs_tracker* r = t->reps[k];
        rbt::TrackerDev& T = r->T;
        RBT_HIP(t, hipSetDevice(r->s->device));
        launch_mean(T, streams[k]);
        launch_recentre(T, T.part_new, streams[k]);
        RBT_HIP(t, hipGetLastError());
        std::swap(T.part_old, T.part_new);   // this frame's particles are the next frame's old ones
        if (k == 0) {
            RBT_HIP(t, hipMemcpyAsync(out_state, T.deflt, sizeof(double) * T.D, hipMemcpyDeviceToHost, streams[k]));
            RBT_HIP(t, hipMemcpyAsync(flags, T.flag, sizeof(flags), hipMemcpyDeviceToHost, streams[k]));
        }
        T.frame += 1;
    }
    for (int k = 0; k < nd; ++k) {   // the host frame / randomness buffers may be reused after this call
        RBT_HIP(t, hipSetDevice(t->reps[k]->s->device));
        RBT_HIP(t, hipStreamSynchronize(streams[k]));
    }
    if (out_resamplings) *out_resamplings = flags[1];
    int32_t slab_rc = RBS_OK;
    for (rbs_handle* sh : g->shards) {   // slabs: a region that did not fit, on any shard
        if (!sh->slab_px) break;
        RBT_HIP(t, hipSetDevice(sh->device));
        RBT_HIP(t, hipMemcpy(sh->h_err, sh->d_err, 2 * sizeof(int), hipMemcpyDeviceToHost));
        if (slab_rc == RBS_OK && check_slab_error(sh) != RBS_OK) slab_rc = gfail(g, sh, RBS_ERR_OUT_OF_MEMORY);
    }
    const std::string msg = g->err;
    if (int32_t rc = group_grow_slabs(g, nullptr)) return rc;   // (every stream is idle here: enlarge before a region fills a slab)
    if (slab_rc) g->err = msg;
    return slab_rc;
}
}  // namespace

extern "C" {

// The body of rbs_tracker_submit; a failure in here happens after some of the frame's work was
// enqueued and some of the tracker's buffers were swapped.
static int32_t tracker_submit_impl(rbs_tracker* t, const float* frame, const double* normals, const double* uniforms, uint64_t seed)
{
    if (t->submitted - t->collected >= 2)
        return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_submit: two frames are in flight already (call rbs_tracker_result)");
    const int slot = (int)(t->submitted & 1);
    const double* frame64 = t->frame64;
    t->frame64 = nullptr;
    if (frame64 && !t->reps.empty()) {   // (the sharded form uploads float frames: converted once here)
        t->frame_tmp.resize((size_t)t->reps[0]->s->npx);
        convert_f64_f32(t->frame_tmp.data(), frame64, t->frame_tmp.size());
        frame = t->frame_tmp.data();
        frame64 = nullptr;
    }
    if (!t->reps.empty()) {   // several devices: the frame runs to completion here, its result waits in the slot
        rbs_tracker* r0 = t->reps[0];
        t->res_rc[slot] = group_tracker_track(t, frame, normals, uniforms, seed, r0->h_state[slot], &r0->h_flags[slot][1]);
        t->submitted += 1;
        return t->res_rc[slot];
    }
    rbt::TrackerDev& T = t->T;
    rbs_handle* h = t->s;
    const BorrowedFrameGuard borrowed_guard{h};   // (the caller's frame is the caller's again when this returns, whatever happened)
    RBT_HIP(t, hipSetDevice(h->device));
    if ((frame || frame64) && h->npx <= 0) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_submit: bad sensor");
    hipStream_t s = h->stream;
    const size_t n = (size_t)T.n;
    T.normals = nullptr;
    T.uniforms = nullptr;
    // host-supplied randomness goes through pinned staging: the caller's buffers are free on return
    if (normals) {
        std::memcpy(t->h_normals[slot], normals, sizeof(double) * n * T.parts * 6);
        RBT_HIP(t, hipMemcpyAsync(t->d_normals2[slot], t->h_normals[slot], sizeof(double) * n * T.parts * 6, hipMemcpyHostToDevice, s));
        T.normals = t->d_normals2[slot];
    }
    if (uniforms) {
        std::memcpy(t->h_uniforms[slot], uniforms, sizeof(double) * n * T.parts);
        RBT_HIP(t, hipMemcpyAsync(t->d_uniforms2[slot], t->h_uniforms[slot], sizeof(double) * n * T.parts, hipMemcpyHostToDevice, s));
        T.uniforms = t->d_uniforms2[slot];
    }
    T.seed = seed;
    T.host_state = t->h_state_dev[slot];
    T.host_flags = t->h_flags_dev[slot];
    const char* nf = std::getenv("RBS_TRACKER_FUSED");
    const bool fused = T.n <= rbt::kFusedFilterMax && !(nf && std::atoi(nf) == 0);
    static const bool tail_on = [] { const char* e = std::getenv("RBS_TRACKER_TAIL"); return !(e && std::atoi(e) == 0); }();
    const bool tail = !fused && tail_on && T.n < rbt::kMultiBlockFrom;   // (RBS_TRACKER_TAIL=0: the three separate launches, A/B)
    for (int b = 0; b < T.parts; ++b) {
        const bool last = b == T.parts - 1;
        // (the transition fused into the sensor's rectangles kernel -- one launch less -- measured no
        // gain: 3 987 against 3 976 frames/s at 2 000 particles)
        launch_propagate(T, b, b == 0 && t->recentre_pending ? 1 : 0, s);
        if (b == 0) t->recentre_pending = false;
        RBT_HIP(t, hipGetLastError());
        // the frame is handed over AFTER the first transition launch: the transition (and the
        // sensor's rectangles kernel behind it) do not depend on it, and run while the host copies
        // the frame into pinned memory and the copy engine uploads it
        if (b == 0 && (frame || frame64)) {
            // Few particles: the frame's own journey (staging copy, transfer, model terms: ~80 us) is most of a frame, and the sensor's
            // GEOMETRY kernel does not need it -- the frame is handed to the sensor as a borrowed one and staged by enqueue_loglikes
            // between the two kernels of the split launch (inside this call: the caller's buffer is free on return as before).  Above
            // kTrackerSplitMax evaluations the one-kernel launch's shorter kernel time wins (RBS_TRACKER_SPLIT_MAX, 0: never).
            const int split_max = h->tracker_split_max;
            const bool idle = t->submitted == t->collected;   // (a frame already in flight -- look-ahead -- hides the journey by itself, and the one-kernel launch is the shorter)
            if (idle && T.n * T.parts <= split_max && can_borrow(h)) {
                if (int32_t rc = frame_begin(h)) return rc;
                if (int32_t rc = frame_ready(h, h->stream)) return rc;
                hand_over_borrowed(h, frame, frame64);   // (doubles, as dbot hands images over: converted while they are staged)
            } else if (int32_t rc = frame64 ? rbs_set_observation(h, frame64, (size_t)h->npx) : rbs_set_observation_f32(h, frame, (size_t)h->npx)) return rc;
        }
        if (int32_t rc = enqueue_loglikes(h, T.poses, T.idx, T.n, last, T.ll_new, s)) return rc;
        if (fused) {
            launch_filter_step(T, b, last ? 1 : 0, last ? 1 : 0, s);
        } else if (tail && last) {
            // the estimate first (one launch, the result event right behind it), the gather after
            launch_filter_tail(T, b, 1, s);
            RBT_HIP(t, hipGetLastError());
            if (h->slab_px) RBT_HIP(t, hipMemcpyAsync(t->h_serr[slot], h->d_err, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
            RBT_HIP(t, hipEventRecord(t->ev_res[slot], s));
            launch_gather(T, s);
        } else {
            launch_weights(T, last ? 1 : 0, s);
            launch_resample_gather(T, b, s);
        }
        RBT_HIP(t, hipGetLastError());
        swap_gathered(T);
    }
    bool recentred = fused;   // (filter_step_kernel re-centres behind its mean)
    if (!fused) {
        // (re-centring inside the single mean block was tried: its two rounds of rotations per thread
        // on one CU take longer than the separate launch, 25 us against 16.5 + 5)
        if (!tail) launch_mean(T, s);
        // the re-centring itself rides in the next frame's first transition launch (the thread that
        // moves particle i re-centres it first); rbs_tracker_get applies it on demand
        static const bool now = [] { const char* e = std::getenv("RBS_TRACKER_RECENTRE_NOW"); return e && std::atoi(e) != 0; }();
        if (now) launch_recentre(T, T.part_new, s);
        else t->recentre_pending = true;
        recentred = now;
    }
    RBT_HIP(t, hipGetLastError());
    if (t->post_on) {
        // the report of the population this frame leaves in T.part_new (named here, before the swap below renames it), behind
        // the frame's last kernel -- in the tail route behind the gather -- and an event of its own: the estimate's sequence
        // number and ev_res do not wait for it
        rbt::PostDev P = t->P;
        P.out = t->h_post_dev[slot];
        P.out_i = reinterpret_cast<int*>(P.out + rbt::post_out_doubles(T.D));
        RBT_HIP(t, hipEventRecord(t->ev_post0[slot], s));
        launch_posterior(T, P, T.part_new, recentred ? 1 : 0, s);
        RBT_HIP(t, hipGetLastError());
        RBT_HIP(t, hipEventRecord(t->ev_post[slot], s));
    }
    if (t->modes_on) {
        // the modes of the same population (T.part_new, T.logw), behind the posterior report's launches where that is on, with a
        // slot and an event of their own
        rbt::ModesDev M = t->M;
        M.out = t->h_modes_dev[slot];
        RBT_HIP(t, hipEventRecord(t->ev_modes0[slot], s));
        rbt::launch_modes(M, T, T.part_new, T.D, rbt::kBody, T.logw, recentred ? 0 : 1, s);
        RBT_HIP(t, hipGetLastError());
        RBT_HIP(t, hipEventRecord(t->ev_modes[slot], s));
        t->modes_seq[slot] = (int)(T.frame + 1);
    }
    if (t->map_on) {
        // the occlusion map of the population this frame leaves behind (T.logw, T.idx: what rbs_tracker_get returns) over the
        // planes the frame's last updating call wrote, behind everything else of the frame and with an event of its own
        RBT_HIP(t, hipEventRecord(t->ev_map0[slot], s));
        if (int32_t rc = occmap::enqueue(h, T.idx, T.logw, T.n, t->h_map_dev[slot])) { t->err = h->err; return rc; }
        RBT_HIP(t, hipEventRecord(t->ev_map[slot], s));
        t->map_seq[slot] = (int)(T.frame + 1);
    }
    if (t->obj_on) {
        // the object map of the same population over the poses the frame's last sampling block evaluated: member i is a copy of
        // particle T.idx[i] of that block (gather_one: idx2[j] = idx[parent], idx being the identity behind the last block's
        // weights), and row s of T.poses holds every body's pose slot s was evaluated with (propagate_body writes all of them
        // in every block).  The next frame's transition overwrites T.poses behind these launches in stream order.
        RBT_HIP(t, hipEventRecord(t->ev_obj0[slot], s));
        if (int32_t rc = objmap::enqueue(h, T.poses, T.n, T.idx, T.logw, T.n, t->h_obj_dev[slot])) { t->err = h->err; return rc; }
        RBT_HIP(t, hipEventRecord(t->ev_obj[slot], s));
        t->obj_seq[slot] = (int)(T.frame + 1);
    }
    std::swap(T.part_old, T.part_new);   // this frame's particles are the next frame's old ones
    // (the estimate and the flags were stored into h_state[slot] / h_flags[slot] by the kernel that
    // finished them: no copies behind the last kernel)
    if (!tail) {
        if (h->slab_px) RBT_HIP(t, hipMemcpyAsync(t->h_serr[slot], h->d_err, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
        RBT_HIP(t, hipEventRecord(t->ev_res[slot], s));
    }
    t->res_seq[slot] = (int)(T.frame + 1);
    T.frame += 1;
    t->res_rc[slot] = RBS_OK;
    t->submitted += 1;
    return RBS_OK;
}

int32_t rbs_tracker_submit(rbs_tracker* t, const float* frame, const double* normals, const double* uniforms, uint64_t seed)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (t->poisoned || t->s->poisoned)
        return tfail(t, RBS_ERR_HIP, "tracker_submit: an earlier frame failed half-way (" + (t->s->poisoned ? t->s->poison_msg : t->err) +
                                         "): call rbs_tracker_initialize");
    const long before = t->submitted;
    const int32_t rc = tracker_submit_impl(t, frame, normals, uniforms, seed);
    if (rc != RBS_OK && !(rc == RBS_ERR_INVALID_ARGUMENT && t->submitted == before)) {
        // drain what was enqueued and refuse further frames: the particle buffers are out of step
        const std::string why = t->err.empty() ? t->s->err : t->err;
        if (t->reps.empty()) { (void)hipSetDevice(t->s->device); (void)hipStreamSynchronize(t->s->stream); (void)hipStreamSynchronize(t->s->copy_stream); }
        else for (rbs_tracker* r : t->reps) { (void)hipSetDevice(r->s->device); (void)hipStreamSynchronize(r->s->stream); (void)hipStreamSynchronize(r->s->copy_stream); }
        (void)hipGetLastError();
        t->poisoned = true;
        t->err = why;
        t->s->err = why;
    }
    return rc;
}

int32_t rbs_tracker_result(rbs_tracker* t, double* out_state, int32_t* out_resamplings)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (!out_state) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_result: null output");
    if (t->collected >= t->submitted) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_result: no frame in flight");
    const int slot = (int)(t->collected & 1);
    t->collected += 1;
    rbs_tracker* r = t->reps.empty() ? t : t->reps[0];
    const int D = r->T.D;
    if (t->reps.empty()) {
        RBT_HIP(t, hipSetDevice(t->s->device));
        // The kernel that finishes the frame stores the estimate into pinned (host-coherent) memory and
        // the frame's number behind it with a system-scope release: spin on that number -- the signalling
        // of the kernel's completion and the wake-up behind it cost several microseconds more.  The
        // event is the fall-back (and the only way with slabs, whose error word arrives by a copy).
        bool seen = false;
        if (!t->s->slab_px && t->res_seq[slot] > 0) {
            volatile int* seq = t->h_flags[slot] + 2;
            for (long it = 0; it < 4000000 && !seen; ++it) {
                seen = __atomic_load_n(seq, __ATOMIC_ACQUIRE) == t->res_seq[slot];
                if (!seen && (it & 255) == 255 && hipEventQuery(t->ev_res[slot]) == hipSuccess) break;
                if (!seen) __builtin_ia32_pause();
            }
        }
        if (!seen) RBT_HIP(t, hipEventSynchronize(t->ev_res[slot]));
        if (t->post_on) {   // the report is finished behind the estimate: wait for it and take it out of the slot
            RBT_HIP(t, hipEventSynchronize(t->ev_post[slot]));
            const size_t nd = rbt::post_out_doubles(D);
            std::memcpy(t->post.data(), t->h_post[slot], sizeof(double) * nd);
            std::memcpy(t->post_i, t->h_post[slot] + nd, sizeof(t->post_i));
            if (hipEventElapsedTime(&t->post_ms, t->ev_post0[slot], t->ev_post[slot]) != hipSuccess) { (void)hipGetLastError(); t->post_ms = 0.f; }
            t->post_valid = true;
        }
        if (t->modes_on) {   // likewise the modes
            RBT_HIP(t, hipEventSynchronize(t->ev_modes[slot]));
            std::memcpy(t->modes.data(), t->h_modes[slot], sizeof(rbs_body_modes) * t->modes.size());
            t->modes_frame = t->modes_seq[slot];
            if (hipEventElapsedTime(&t->modes_ms, t->ev_modes0[slot], t->ev_modes[slot]) != hipSuccess) { (void)hipGetLastError(); t->modes_ms = 0.f; }
            t->modes_valid = true;
        }
        if (t->map_on) {   // likewise the map, finished last
            RBT_HIP(t, hipEventSynchronize(t->ev_map[slot]));
            std::memcpy(t->map.data(), t->h_map[slot], sizeof(float) * t->map.size());
            t->map_frame = t->map_seq[slot];
            if (hipEventElapsedTime(&t->map_ms, t->ev_map0[slot], t->ev_map[slot]) != hipSuccess) { (void)hipGetLastError(); t->map_ms = 0.f; }
            t->map_valid = true;
        }
        if (t->obj_on) {   // ... and the object map behind it
            RBT_HIP(t, hipEventSynchronize(t->ev_obj[slot]));
            std::memcpy(t->obj.data(), t->h_obj[slot], sizeof(float) * t->obj.size());
            t->obj_frame = t->obj_seq[slot];
            if (hipEventElapsedTime(&t->obj_ms, t->ev_obj0[slot], t->ev_obj[slot]) != hipSuccess) { (void)hipGetLastError(); t->obj_ms = 0.f; }
            t->obj_valid = true;
        }
    }
    std::memcpy(out_state, r->h_state[slot], sizeof(double) * D);
    if (out_resamplings) *out_resamplings = r->h_flags[slot][1];
    if (!t->reps.empty()) return t->res_rc[slot];
    if (t->submitted == t->collected) t->s->quiet = !t->s->async_outstanding;   // frame by frame: the next frame may travel in pieces
    if (t->s->slab_px) {
        // the frame has run: a region that did not fit cannot be repaired here (the filter has resampled
        // on the contained particle's NaN) and is an error -- but the slabs are enlarged BEFORE that,
        // whenever the largest region asked for has filled three quarters of one, at a frame boundary
        // with nothing in flight (regions move a few pixels per frame)
        rbs_handle* h = t->s;
        h->h_err[0] = t->h_serr[slot][0];
        h->h_err[1] = t->h_serr[slot][1];
        const int32_t rc = check_slab_error(h);
        const std::string msg = h->err;
        if (t->submitted == t->collected)
            if (int32_t rc2 = slab_housekeeping(h)) return rc2;
        if (rc) { h->err = msg; t->err = msg; t->poisoned = true; }
        return rc;
    }
    return RBS_OK;
}

int32_t rbs_tracker_submit_f64(rbs_tracker* t, const double* frame, const double* normals, const double* uniforms, uint64_t seed)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    t->frame64 = frame;
    const int32_t rc = rbs_tracker_submit(t, nullptr, normals, uniforms, seed);
    t->frame64 = nullptr;
    return rc;
}

int32_t rbs_tracker_track_f64(rbs_tracker* t, const double* frame, const double* normals, const double* uniforms, uint64_t seed,
                              double* out_state, int32_t* out_resamplings)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    t->frame64 = frame;
    const int32_t rc = rbs_tracker_track(t, nullptr, normals, uniforms, seed, out_state, out_resamplings);
    t->frame64 = nullptr;
    return rc;
}

int32_t rbs_tracker_track(rbs_tracker* t, const float* frame, const double* normals,
                          const double* uniforms, uint64_t seed, double* out_state,
                          int32_t* out_resamplings)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (!out_state) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_track: null output");
    if (t->submitted != t->collected)
        return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_track: frames submitted with rbs_tracker_submit are still in flight");
    if (int32_t rc = rbs_tracker_submit(t, frame, normals, uniforms, seed)) {
        if (t->submitted != t->collected) t->collected = t->submitted;   // (a group's frame that failed: nothing to collect)
        return rc;
    }
    return rbs_tracker_result(t, out_state, out_resamplings);
}

int32_t rbs_tracker_get(rbs_tracker* t, double* particles, double* log_weights, int32_t* indices)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (!t->reps.empty()) {
        for (rbs_tracker* r : t->reps) { RBT_HIP(t, hipSetDevice(r->s->device)); RBT_HIP(t, hipStreamSynchronize(r->s->stream)); }
        return rbs_tracker_get(t->reps[0], particles, log_weights, indices);
    }
    rbt::TrackerDev& T = t->T;
    RBT_HIP(t, hipSetDevice(t->s->device));
    if (t->recentre_pending) {   // (deferred into the next frame's transition launch: apply it now)
        launch_recentre(T, T.part_old, t->s->stream);
        RBT_HIP(t, hipGetLastError());
        t->recentre_pending = false;
    }
    RBT_HIP(t, hipStreamSynchronize(t->s->stream));
    if (particles) RBT_HIP(t, hipMemcpy(particles, T.part_old, sizeof(double) * (size_t)T.n * T.D, hipMemcpyDeviceToHost));
    if (log_weights) RBT_HIP(t, hipMemcpy(log_weights, T.logw, sizeof(double) * (size_t)T.n, hipMemcpyDeviceToHost));
    if (indices) RBT_HIP(t, hipMemcpy(indices, T.idx, sizeof(int) * (size_t)T.n, hipMemcpyDeviceToHost));
    return RBS_OK;
}

int32_t rbs_tracker_set_posterior(rbs_tracker* t, int32_t enable)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (!t->reps.empty() || !t->s->shards.empty())
        return tfail(t, RBS_ERR_UNSUPPORTED, "tracker_set_posterior: single-device trackers only");
    if (t->submitted != t->collected)
        return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_set_posterior: frames are in flight (call rbs_tracker_result)");
    rbt::TrackerDev& T = t->T;
    if (enable && !t->post_ready) {
        // every buffer is made once, each only where an earlier attempt that failed half-way has not left it; the report is
        // switched on only when all of them exist
        RBT_HIP(t, hipSetDevice(t->s->device));
        const size_t nd = rbt::post_out_doubles(T.D);
        if (!t->P.pose) if (int32_t rc = talloc(t, &t->P.pose, (size_t)T.n * T.parts * 6)) return rc;
        if (!t->P.e) if (int32_t rc = talloc(t, &t->P.e, (size_t)T.n)) return rc;
        if (T.n >= rbt::kMultiBlockFrom) {
            if (!t->P.partials) if (int32_t rc = talloc(t, &t->P.partials, rbt::post_partials_doubles(T.n, T.D))) return rc;
            if (!t->P.bitmap) if (int32_t rc = talloc(t, &t->P.bitmap, (size_t)(T.n + 31) / 32)) return rc;
        }
        t->post.assign(nd, 0.0);
        for (int k = 0; k < 2; ++k) {
            if (!t->h_post[k]) RBT_HIP(t, hipHostMalloc(&t->h_post[k], sizeof(double) * nd + 4 * sizeof(int), hipHostMallocDefault));
            if (!t->h_post_dev[k]) RBT_HIP(t, hipHostGetDevicePointer(reinterpret_cast<void**>(&t->h_post_dev[k]), t->h_post[k], 0));
            if (!t->ev_post[k]) RBT_HIP(t, hipEventCreate(&t->ev_post[k]));
            if (!t->ev_post0[k]) RBT_HIP(t, hipEventCreate(&t->ev_post0[k]));
        }
        t->post_ready = true;
    }
    t->post_on = enable != 0;
    t->post_valid = false;
    return RBS_OK;
}

int32_t rbs_tracker_posterior(rbs_tracker* t, rbs_tracker_posterior_info* info, double* mean, double* cov)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (t->poisoned || t->s->poisoned)
        return tfail(t, RBS_ERR_HIP, "tracker_posterior: an earlier frame failed half-way (" + (t->s->poisoned ? t->s->poison_msg : t->err) +
                                         "): call rbs_tracker_initialize");
    if (!t->post_on) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_posterior: the report is off (rbs_tracker_set_posterior)");
    if (!t->post_valid) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_posterior: no frame has been handed out since rbs_tracker_initialize");
    const size_t D = (size_t)t->T.D;
    if (info) {
        info->n = t->post_i[0];
        info->survivors = t->post_i[1];
        info->resampled = t->post_i[2];
        info->frame = t->post_i[3];
        info->ess = t->post[0];
    }
    if (mean) std::memcpy(mean, t->post.data() + 1, sizeof(double) * D);
    if (cov) std::memcpy(cov, t->post.data() + 1 + D, sizeof(double) * D * D);
    return RBS_OK;
}

int32_t rbs_tracker_posterior_ms(rbs_tracker* t, float* ms)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (!ms) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_posterior_ms: null output");
    if (!t->post_on || !t->post_valid) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_posterior_ms: no report has been handed out");
    *ms = t->post_ms;
    return RBS_OK;
}

int32_t rbs_tracker_set_modes(rbs_tracker* t, const rbs_modes_params* params)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (!t->reps.empty() || !t->s->shards.empty())
        return tfail(t, RBS_ERR_UNSUPPORTED, "tracker_set_modes: single-device trackers only");
    if (t->submitted != t->collected)
        return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_set_modes: frames are in flight (call rbs_tracker_result)");
    if (params)
        if (const char* why = modes::refuse_params(params)) return tfail(t, RBS_ERR_INVALID_ARGUMENT, fmt("tracker_set_modes: %s", why));
    rbt::TrackerDev& T = t->T;
    if (params && T.n > rbt::kModesMaxN) return tfail(t, RBS_ERR_UNSUPPORTED, fmt("tracker_set_modes: at most %d particles", rbt::kModesMaxN));
    if (params && !t->modes_ready) {
        // every buffer is made once, each only where an earlier attempt that failed half-way has not left it; the report is
        // switched on only when all of them exist
        RBT_HIP(t, hipSetDevice(t->s->device));
        if (!t->modes_work) if (int32_t rc = talloc(t, &t->modes_work, rbt::modes_doubles(T.n, T.parts))) return rc;
        if (!t->modes_sel) if (int32_t rc = talloc(t, &t->modes_sel, rbt::modes_ints(T.parts))) return rc;
        t->M.n = T.n;
        t->M.parts = T.parts;
        rbt::modes_carve(t->M, t->modes_work, t->modes_sel);
        t->modes.assign((size_t)T.parts, rbs_body_modes{});
        for (int k = 0; k < 2; ++k) {
            if (!t->h_modes[k]) RBT_HIP(t, hipHostMalloc(&t->h_modes[k], sizeof(rbs_body_modes) * (size_t)T.parts, hipHostMallocDefault));
            if (!t->h_modes_dev[k]) RBT_HIP(t, hipHostGetDevicePointer(reinterpret_cast<void**>(&t->h_modes_dev[k]), t->h_modes[k], 0));
            if (!t->ev_modes[k]) RBT_HIP(t, hipEventCreate(&t->ev_modes[k]));
            if (!t->ev_modes0[k]) RBT_HIP(t, hipEventCreate(&t->ev_modes0[k]));
        }
        t->modes_ready = true;
    }
    if (params) modes::fill(t->M, T.n, T.parts, *params);
    t->modes_on = params != nullptr;
    t->modes_valid = false;
    return RBS_OK;
}

int32_t rbs_tracker_modes(rbs_tracker* t, int32_t* frame, rbs_body_modes* out)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (t->poisoned || t->s->poisoned)
        return tfail(t, RBS_ERR_HIP, "tracker_modes: an earlier frame failed half-way (" + (t->s->poisoned ? t->s->poison_msg : t->err) +
                                         "): call rbs_tracker_initialize");
    if (!t->modes_on) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_modes: the report is off (rbs_tracker_set_modes)");
    if (!t->modes_valid) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_modes: no frame has been handed out since rbs_tracker_initialize");
    if (frame) *frame = t->modes_frame;
    if (out) std::memcpy(out, t->modes.data(), sizeof(rbs_body_modes) * t->modes.size());
    return RBS_OK;
}

int32_t rbs_tracker_modes_ms(rbs_tracker* t, float* ms)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (!ms) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_modes_ms: null output");
    if (!t->modes_on || !t->modes_valid) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_modes_ms: no report has been handed out");
    *ms = t->modes_ms;
    return RBS_OK;
}

int32_t rbs_tracker_set_occlusion_map(rbs_tracker* t, int32_t enable)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (!t->reps.empty() || !t->s->shards.empty())
        return tfail(t, RBS_ERR_UNSUPPORTED, "tracker_set_occlusion_map: single-device trackers only");
    if (t->submitted != t->collected)
        return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_set_occlusion_map: frames are in flight (call rbs_tracker_result)");
    if (enable && !t->map_ready) {
        // every buffer is made once, each only where an earlier attempt that failed half-way has not left it; the map is
        // switched on only when all of them exist
        rbs_handle* h = t->s;
        if (h->group || h->peer_world > 1) return tfail(t, RBS_ERR_UNSUPPORTED, "tracker_set_occlusion_map: single-device trackers only");
        RBT_HIP(t, hipSetDevice(h->device));
        if (int32_t rc = occmap::ensure(h, t->T.n)) { t->err = h->err; return rc; }
        t->map.assign((size_t)h->npx, 0.f);
        for (int k = 0; k < 2; ++k) {
            if (!t->h_map[k]) RBT_HIP(t, hipHostMalloc(&t->h_map[k], sizeof(float) * (size_t)h->npx, hipHostMallocDefault));
            if (!t->h_map_dev[k]) RBT_HIP(t, hipHostGetDevicePointer(reinterpret_cast<void**>(&t->h_map_dev[k]), t->h_map[k], 0));
            if (!t->ev_map[k]) RBT_HIP(t, hipEventCreate(&t->ev_map[k]));
            if (!t->ev_map0[k]) RBT_HIP(t, hipEventCreate(&t->ev_map0[k]));
        }
        t->map_ready = true;
    }
    t->map_on = enable != 0;
    t->map_valid = false;
    return RBS_OK;
}

int32_t rbs_tracker_occlusion_map(rbs_tracker* t, int32_t* frame, float* out)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (t->poisoned || t->s->poisoned)
        return tfail(t, RBS_ERR_HIP, "tracker_occlusion_map: an earlier frame failed half-way (" + (t->s->poisoned ? t->s->poison_msg : t->err) +
                                         "): call rbs_tracker_initialize");
    if (!t->map_on) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_occlusion_map: the map is off (rbs_tracker_set_occlusion_map)");
    if (!t->map_valid) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_occlusion_map: no frame has been handed out since rbs_tracker_initialize");
    if (frame) *frame = t->map_frame;
    if (out) std::memcpy(out, t->map.data(), sizeof(float) * t->map.size());
    return RBS_OK;
}

int32_t rbs_tracker_occlusion_map_ms(rbs_tracker* t, float* ms)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (!ms) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_occlusion_map_ms: null output");
    if (!t->map_on || !t->map_valid) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_occlusion_map_ms: no map has been handed out");
    *ms = t->map_ms;
    return RBS_OK;
}

int32_t rbs_tracker_set_object_map(rbs_tracker* t, int32_t enable)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (!t->reps.empty() || !t->s->shards.empty())
        return tfail(t, RBS_ERR_UNSUPPORTED, "tracker_set_object_map: single-device trackers only");
    if (t->submitted != t->collected)
        return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_set_object_map: frames are in flight (call rbs_tracker_result)");
    if (enable && !t->obj_ready) {
        // every buffer is made once, each only where an earlier attempt that failed half-way has not left it; the map is
        // switched on only when all of them exist
        rbs_handle* h = t->s;
        if (const char* why = objmap::refuse_handle(h)) return tfail(t, RBS_ERR_UNSUPPORTED, fmt("tracker_set_object_map: %s", why));
        RBT_HIP(t, hipSetDevice(h->device));
        if (int32_t rc = objmap::ensure(h, t->T.n, t->T.n)) { t->err = h->err; return rc; }
        const size_t floats = (size_t)(h->n_bodies + 2) * (size_t)h->npx;
        t->obj.assign(floats, 0.f);
        for (int k = 0; k < 2; ++k) {
            if (!t->h_obj[k]) RBT_HIP(t, hipHostMalloc(&t->h_obj[k], sizeof(float) * floats, hipHostMallocDefault));
            if (!t->h_obj_dev[k]) RBT_HIP(t, hipHostGetDevicePointer(reinterpret_cast<void**>(&t->h_obj_dev[k]), t->h_obj[k], 0));
            if (!t->ev_obj[k]) RBT_HIP(t, hipEventCreate(&t->ev_obj[k]));
            if (!t->ev_obj0[k]) RBT_HIP(t, hipEventCreate(&t->ev_obj0[k]));
        }
        t->obj_ready = true;
    }
    t->obj_on = enable != 0;
    t->obj_valid = false;
    return RBS_OK;
}

int32_t rbs_tracker_object_map(rbs_tracker* t, int32_t* frame, float* cover, float* depth, float* var)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (t->poisoned || t->s->poisoned)
        return tfail(t, RBS_ERR_HIP, "tracker_object_map: an earlier frame failed half-way (" + (t->s->poisoned ? t->s->poison_msg : t->err) +
                                         "): call rbs_tracker_initialize");
    if (!t->obj_on) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_object_map: the map is off (rbs_tracker_set_object_map)");
    if (!t->obj_valid) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_object_map: no frame has been handed out since rbs_tracker_initialize");
    const size_t npx = (size_t)t->s->npx, B = (size_t)t->s->n_bodies;
    if (frame) *frame = t->obj_frame;
    if (cover) std::memcpy(cover, t->obj.data(), sizeof(float) * B * npx);
    if (depth) std::memcpy(depth, t->obj.data() + B * npx, sizeof(float) * npx);
    if (var) std::memcpy(var, t->obj.data() + (B + 1) * npx, sizeof(float) * npx);
    return RBS_OK;
}

int32_t rbs_tracker_object_map_ms(rbs_tracker* t, float* ms)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (!ms) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_object_map_ms: null output");
    if (!t->obj_on || !t->obj_valid) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_object_map_ms: no map has been handed out");
    *ms = t->obj_ms;
    return RBS_OK;
}

int32_t rbs_tracker_poses(rbs_tracker* t, double* out)
{
    if (!t) return RBS_ERR_INVALID_ARGUMENT;
    if (!out) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_poses: null output");
    if (!t->reps.empty() || !t->s->shards.empty())
        return tfail(t, RBS_ERR_UNSUPPORTED, "tracker_poses: single-device trackers only");
    if (t->poisoned || t->s->poisoned)
        return tfail(t, RBS_ERR_HIP, "tracker_poses: an earlier frame failed half-way (" + (t->s->poisoned ? t->s->poison_msg : t->err) +
                                         "): call rbs_tracker_initialize");
    // (no snapshot is kept: a frame in flight has overwritten, or is overwriting, the rows the last result's population points at)
    if (t->submitted != t->collected)
        return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_poses: frames are in flight (call rbs_tracker_result)");
    rbt::TrackerDev& T = t->T;
    if (T.frame < 1) return tfail(t, RBS_ERR_INVALID_ARGUMENT, "tracker_poses: no frame has been tracked since rbs_tracker_initialize");
    RBT_HIP(t, hipSetDevice(t->s->device));
    RBT_HIP(t, hipStreamSynchronize(t->s->stream));
    const size_t w = (size_t)T.parts * 12;
    std::vector<double> rows((size_t)T.n * w);
    std::vector<int> idx((size_t)T.n);
    RBT_HIP(t, hipMemcpy(rows.data(), T.poses, sizeof(double) * rows.size(), hipMemcpyDeviceToHost));
    RBT_HIP(t, hipMemcpy(idx.data(), T.idx, sizeof(int) * idx.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < (size_t)T.n; ++i) std::memcpy(out + i * w, rows.data() + (size_t)idx[i] * w, sizeof(double) * w);
    return RBS_OK;
}

}  // extern "C"
