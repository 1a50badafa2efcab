// rbs_modes_api.h -- the posterior modes' host side on a sensor handle (kernels: rbsensor_modes.hip): the parameter checks, the
// handle's own buffers and the stateless entry point rbs_pose_modes.  The device tracker's report (rbs_tracker_set_modes ..)
// lives with the tracker in rbs_tracker_api.h.  Not a header to include elsewhere: a section of rbsensor_capi.hip's translation unit.

static_assert(sizeof(rbs_modes_params) == 32 && offsetof(rbs_modes_params, k_max) == 24, "rbs_modes_params layout is mirrored by dbot_ros_amd/_capi.py");
static_assert(sizeof(rbs_mode) == 80 && offsetof(rbs_mode, density) == 8 && offsetof(rbs_mode, delta) == 32, "rbs_mode layout is mirrored by dbot_ros_amd/_capi.py");
static_assert(sizeof(rbs_body_modes) == 8 + 80 * RBS_MODES_MAX && offsetof(rbs_body_modes, mode) == 8, "rbs_body_modes layout is mirrored by dbot_ros_amd/_capi.py");

// What a sensor owns once rbs_pose_modes has been asked of it: allocated at first use, grow-only, freed by rbs_destroy.
struct rbs_modes_state {
    int cap_n = 0;
    size_t cap_work = 0;
    double* d_in = nullptr;        // [cap_n][bodies][6] the caller's deltas
    double* d_lw = nullptr;        // [cap_n]
    double* d_work = nullptr;      // [cap_work] >= modes_doubles(n, bodies) of every n asked so far (NOT monotonic in n: the j-split's
                                   // part count drops where the part length grows, 16 parts at 1 024 particles and 5 at 1 025)
    int* d_sel = nullptr;          // modes_ints(bodies)
    rbs_body_modes* d_out = nullptr;   // [bodies]
};

namespace {
namespace modes {

// nullptr, or what is wrong with the parameters
const char* refuse_params(const rbs_modes_params* p)
{
    if (!p) return "null parameters";
    if (!(p->h_t > 0.0) || !std::isfinite(p->h_t)) return "h_t must be positive";
    if (!(p->h_r > 0.0 && p->h_r <= 1.0)) return "h_r must lie in (0, 1]";
    if (!(p->separation >= 1.0) || !std::isfinite(p->separation)) return "separation must be at least 1";
    if (p->k_max < 1 || p->k_max > RBS_MODES_MAX) return "k_max outside 1..8";
    return nullptr;
}

void fill(rbt::ModesDev& M, int n, int parts, const rbs_modes_params& p)
{
    M.n = n;
    M.parts = parts;
    M.k_max = p.k_max;
    M.h_t = p.h_t;
    M.c4 = 4.0 / (p.h_r * p.h_r);
    M.sep2 = p.separation * p.separation;
}

int32_t ensure(rbs_handle* h, int n)
{
    if (!h->modes) {
        h->modes = new (std::nothrow) rbs_modes_state;
        if (!h->modes) return fail(h, RBS_ERR_OUT_OF_MEMORY, "pose_modes: out of host memory");
    }
    rbs_modes_state* o = h->modes;
    const int B = h->n_bodies;
    if (!o->d_sel) RBS_HIP(h, hipMalloc(&o->d_sel, sizeof(int) * rbt::modes_ints(B)));
    if (!o->d_out) RBS_HIP(h, hipMalloc(&o->d_out, sizeof(rbs_body_modes) * (size_t)B));
    if (n > o->cap_n) {
        RBS_HIP(h, hipStreamSynchronize(h->stream));
        (void)hipFree(o->d_in); (void)hipFree(o->d_lw);
        o->d_in = nullptr; o->d_lw = nullptr;
        o->cap_n = 0;
        RBS_HIP(h, hipMalloc(&o->d_in, sizeof(double) * (size_t)n * B * 6));
        RBS_HIP(h, hipMalloc(&o->d_lw, sizeof(double) * (size_t)n));
        o->cap_n = n;
    }
    const size_t need = rbt::modes_doubles(n, B);
    if (need > o->cap_work) {
        RBS_HIP(h, hipStreamSynchronize(h->stream));
        (void)hipFree(o->d_work);
        o->d_work = nullptr;
        o->cap_work = 0;
        RBS_HIP(h, hipMalloc(&o->d_work, sizeof(double) * need));
        o->cap_work = need;
    }
    return RBS_OK;
}

}  // namespace modes

// rbs_destroy (the handle's device is current and its streams are idle).
void modes_release(rbs_handle* h)
{
    rbs_modes_state* o = h->modes;
    if (!o) return;
    (void)hipFree(o->d_in);
    (void)hipFree(o->d_lw);
    (void)hipFree(o->d_work);
    (void)hipFree(o->d_sel);
    (void)hipFree(o->d_out);
    delete o;
    h->modes = nullptr;
}

}  // namespace

extern "C" {

void rbs_modes_default_params(rbs_modes_params* p)
{
    if (!p) return;
    // starting values, unmeasured: a few transition sigmas wide, not tuned on data
    p->h_t = 0.02;
    p->h_r = 0.2;
    p->separation = 2.0;
    p->k_max = 4;
    p->reserved = 0;
}

int32_t rbs_pose_modes(rbs_handle* h, const double* deltas, const double* log_weights, int32_t n, const rbs_modes_params* params,
                       rbs_body_modes* out)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!deltas || !log_weights || !out) return fail(h, RBS_ERR_INVALID_ARGUMENT, "pose_modes: null pointer");
    if (const char* why = modes::refuse_params(params)) return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("pose_modes: %s", why));
    if (n < 1) return fail(h, RBS_ERR_INVALID_ARGUMENT, "pose_modes: n < 1");
    if (!h->shards.empty() || h->group || h->peer_world > 1) return fail(h, RBS_ERR_UNSUPPORTED, "pose_modes: single-device handles only");
    if (n > h->max_particles) return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("pose_modes: n %d above max_particles %d", n, h->max_particles));
    if (n > rbt::kModesMaxN) return fail(h, RBS_ERR_UNSUPPORTED, fmt("pose_modes: at most %d particles", rbt::kModesMaxN));
    const int B = h->n_bodies;
    bool any = false;
    for (int i = 0; i < n; ++i) {
        const double w = log_weights[i];
        if (std::isfinite(w)) any = true;
        else if (!(std::isinf(w) && w < 0.0)) return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("pose_modes: log-weight %d is neither finite nor -inf", i));
    }
    if (!any) return fail(h, RBS_ERR_INVALID_ARGUMENT, "pose_modes: every log-weight is -inf");
    for (size_t k = 0; k < (size_t)n * B * 6; ++k)
        if (!std::isfinite(deltas[k])) return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("pose_modes: delta entry %zu is not finite", k));
    RBS_REFUSE_POISONED(h);
    RBS_HIP(h, hipSetDevice(h->device));
    if (int32_t rc = modes::ensure(h, n)) return rc;
    rbs_modes_state* o = h->modes;
    hipStream_t s = h->stream;
    RBS_HIP(h, hipStreamSynchronize(s));   // (the two buffers written next have no reader left)
    RBS_HIP(h, hipMemcpy(o->d_in, deltas, sizeof(double) * (size_t)n * B * 6, hipMemcpyHostToDevice));
    RBS_HIP(h, hipMemcpy(o->d_lw, log_weights, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    rbt::ModesDev M{};
    modes::fill(M, n, B, *params);
    rbt::modes_carve(M, o->d_work, o->d_sel);
    M.out = o->d_out;
    rbt::launch_modes(M, rbt::TrackerDev{}, o->d_in, B * 6, 6, o->d_lw, 0, s);
    RBS_HIP(h, hipGetLastError());
    RBS_HIP(h, hipStreamSynchronize(s));
    RBS_HIP(h, hipMemcpy(out, o->d_out, sizeof(rbs_body_modes) * (size_t)B, hipMemcpyDeviceToHost));
    return RBS_OK;
}

}  // extern "C"
