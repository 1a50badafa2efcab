// rbs_refine_api.h -- the pose refiner's host side on a sensor handle (kernels: rbsensor_refine.hip): the parameter checks, the
// handle's own buffers and the entry points rbs_refine_*.  Not a header to include elsewhere: a section of
// rbsensor_capi.hip's translation unit, included behind rbsensor_refine.hip (release calls refine_release).

static_assert(sizeof(rbs_refine_params) == 64 && offsetof(rbs_refine_params, min_pixels) == 56, "rbs_refine_params layout is mirrored by dbot_ros_amd/_capi.py");
static_assert(sizeof(rbs_refine_body) == 32 && offsetof(rbs_refine_body, rms_first) == 16, "rbs_refine_body layout is mirrored by dbot_ros_amd/_capi.py and the solve kernel");
static_assert(sizeof(rbs_refine_history) == 376 && offsetof(rbs_refine_history, sums) == 96 && offsetof(rbs_refine_history, count) == 368,
              "rbs_refine_history layout is mirrored by dbot_ros_amd/_capi.py and the solve kernel");
static_assert(rbs::kRefineMaxPlanes == rbs::kAssessMaxPlanes, "the refiner's limits are the assessor's");

// What a sensor owns once it has refined: allocated at first use, grow-only, freed by rbs_destroy.
struct rbs_refine_state {
    int cap = 0;                    // planes the buffers hold
    float* d_planes = nullptr;      // [cap][npx]
    int4* d_rects = nullptr;        // [cap]
    double* d_partial = nullptr;    // [cap][kRefineParts][kRefineSums]
    int* d_pcount = nullptr;        // [cap][kRefineParts]
    int* d_frozen = nullptr;        // [kRefineMaxPlanes]
    unsigned char* d_out = nullptr; // poses [kRefineMaxPlanes][12] | records [kRefineMaxPlanes] | history [RBS_REFINE_MAX_ITERS][kRefineMaxPlanes]:
                                    // what the call's one copy brings back (the history packed [iters][planes])
    float* d_frame = nullptr;       // [npx] a caller's frame
    unsigned char* h_pin = nullptr; // pinned: frame [npx] floats | the image of d_out
    hipEvent_t ev[3 * RBS_REFINE_MAX_ITERS + 1] = {};
    float ms[3] = {0.f, 0.f, 0.f};  // render, accumulate, solve: summed over the iterations
    int n = 0, iters = 0;           // poses and iterations of the last call (0: none yet)
};

namespace {
namespace refine {

constexpr size_t kRecOff = sizeof(double) * 12 * rbs::kRefineMaxPlanes;
constexpr size_t kHistOff = kRecOff + sizeof(rbs_refine_body) * rbs::kRefineMaxPlanes;
constexpr size_t kOutBytes = kHistOff + sizeof(rbs_refine_history) * RBS_REFINE_MAX_ITERS * rbs::kRefineMaxPlanes;

const char* check_params(const rbs_refine_params* p)
{
    if (!(p->gate_sigmas > 0.0) || !std::isfinite(p->gate_sigmas)) return "refine: gate_sigmas must be finite and > 0";
    if (!(p->huber_sigmas > 0.0) || !std::isfinite(p->huber_sigmas)) return "refine: huber_sigmas must be finite and > 0";
    if (!(p->damping >= 0.0) || !std::isfinite(p->damping)) return "refine: damping must be finite and >= 0";
    if (!(p->max_rotation > 0.0) || !std::isfinite(p->max_rotation)) return "refine: max_rotation must be finite and > 0";
    if (!(p->max_translation > 0.0) || !std::isfinite(p->max_translation)) return "refine: max_translation must be finite and > 0";
    if (!(p->eps_rotation >= 0.0) || !std::isfinite(p->eps_rotation)) return "refine: eps_rotation must be finite and >= 0";
    if (!(p->eps_translation >= 0.0) || !std::isfinite(p->eps_translation)) return "refine: eps_translation must be finite and >= 0";
    if (p->min_pixels < 1) return "refine: min_pixels must be >= 1";
    if (p->iters < 1 || p->iters > RBS_REFINE_MAX_ITERS) return "refine: iters outside 1..32";
    return nullptr;
}

size_t pin_out_off(const rbs_handle* h) { return (sizeof(float) * (size_t)h->npx + 15) & ~(size_t)15; }

int32_t ensure(rbs_handle* h, int planes)
{
    if (!h->refine) {
        h->refine = new (std::nothrow) rbs_refine_state;
        if (!h->refine) return fail(h, RBS_ERR_OUT_OF_MEMORY, "refine: out of host memory");
    }
    rbs_refine_state* a = h->refine;
    // (each on its own: a call that failed half way leaves what it got, and the next one asks for the rest)
    if (!a->h_pin) RBS_HIP(h, hipHostMalloc(&a->h_pin, pin_out_off(h) + kOutBytes, hipHostMallocDefault));
    if (!a->d_frame) RBS_HIP(h, hipMalloc(&a->d_frame, sizeof(float) * (size_t)h->npx));
    if (!a->d_out) RBS_HIP(h, hipMalloc(&a->d_out, kOutBytes));
    if (!a->d_frozen) RBS_HIP(h, hipMalloc(&a->d_frozen, sizeof(int) * rbs::kRefineMaxPlanes));
    for (hipEvent_t& e : a->ev)
        if (!e) RBS_HIP(h, hipEventCreate(&e));
    if (planes > a->cap) {   // (grow-only; the stream is idle of this state's readers: every call ends synchronised)
        RBS_HIP(h, hipStreamSynchronize(h->stream));
        (void)hipFree(a->d_planes); (void)hipFree(a->d_rects); (void)hipFree(a->d_partial); (void)hipFree(a->d_pcount);
        a->d_planes = nullptr; a->d_rects = nullptr; a->d_partial = nullptr; a->d_pcount = nullptr;
        a->cap = 0;
        a->n = 0;
        RBS_HIP(h, hipMalloc(&a->d_planes, sizeof(float) * (size_t)planes * h->npx));
        RBS_HIP(h, hipMalloc(&a->d_rects, sizeof(int4) * (size_t)planes));
        RBS_HIP(h, hipMalloc(&a->d_partial, sizeof(double) * rbs::kRefineSums * rbs::kRefineParts * (size_t)planes));
        RBS_HIP(h, hipMalloc(&a->d_pcount, sizeof(int) * rbs::kRefineParts * (size_t)planes));
        a->cap = planes;
    }
    return RBS_OK;
}

}  // namespace refine

// rbs_destroy (the handle's device is current and its streams are idle).
void refine_release(rbs_handle* h)
{
    rbs_refine_state* a = h->refine;
    if (!a) return;
    (void)hipFree(a->d_planes);
    (void)hipFree(a->d_rects);
    (void)hipFree(a->d_partial);
    (void)hipFree(a->d_pcount);
    (void)hipFree(a->d_frozen);
    (void)hipFree(a->d_out);
    (void)hipFree(a->d_frame);
    if (a->h_pin) (void)hipHostFree(a->h_pin);
    for (hipEvent_t e : a->ev)
        if (e) (void)hipEventDestroy(e);
    delete a;
    h->refine = nullptr;
}

}  // namespace

extern "C" {

void rbs_refine_default_params(rbs_refine_params* p)
{
    if (!p) return;
    // starting values, unmeasured: none was tuned on data
    p->gate_sigmas = 10.0;
    p->huber_sigmas = 3.0;
    p->damping = 1e-3;
    p->max_rotation = 0.2;
    p->max_translation = 0.02;
    p->eps_rotation = 1e-3;
    p->eps_translation = 1e-4;
    p->min_pixels = 16;
    p->iters = 10;
}

int32_t rbs_refine_check_params(const rbs_refine_params* params)
{
    return params && refine::check_params(params) ? RBS_ERR_INVALID_ARGUMENT : RBS_OK;
}

int32_t rbs_refine_poses(rbs_handle* h, const rbs_refine_params* params, const float* frame, const double* poses_in, int32_t n,
                         double* poses_out, rbs_refine_body* records_out)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!poses_in || !poses_out) return fail(h, RBS_ERR_INVALID_ARGUMENT, "refine_poses: null pointer");
    if (n < 1) return fail(h, RBS_ERR_INVALID_ARGUMENT, "refine_poses: n < 1");
    rbs_refine_params p;
    if (params) p = *params; else rbs_refine_default_params(&p);
    if (const char* bad = refine::check_params(&p)) return fail(h, RBS_ERR_INVALID_ARGUMENT, bad);
    if (!h->shards.empty() || h->group || h->peer_world > 1)
        return fail(h, RBS_ERR_UNSUPPORTED, "refine_poses: single-device handles only");
    const int B = h->n_bodies;
    if ((long)n * B > rbs::kRefineMaxPlanes)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("refine_poses: n x n_objects = %ld exceeds %d", (long)n * B, rbs::kRefineMaxPlanes));
    const int planes = n * B;
    for (size_t i = 0; i < (size_t)planes * 12; ++i)
        if (!std::isfinite(poses_in[i])) return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("refine_poses: pose entry %zu is not finite", i));
    RBS_REFUSE_POISONED(h);
    RBS_HIP(h, hipSetDevice(h->device));
    if (int32_t rc = refine::ensure(h, planes)) return rc;
    rbs_refine_state* a = h->refine;
    hipStream_t s = h->stream;
    const size_t npx = (size_t)h->npx;
    const float* d_frame;
    if (frame) {
        std::memcpy(a->h_pin, frame, sizeof(float) * npx);
        RBS_HIP(h, hipMemcpyAsync(a->d_frame, a->h_pin, sizeof(float) * npx, hipMemcpyHostToDevice, s));
        d_frame = a->d_frame;
    } else {   // the sensor's current observation, as rbs_assess_poses reads it
        if (int32_t rc = make_current(h, s)) return rc;
        d_frame = obs_frame(h);
    }
    unsigned char* h_out = a->h_pin + refine::pin_out_off(h);
    double* d_poses = reinterpret_cast<double*>(a->d_out);
    rbs_refine_body* d_rec = reinterpret_cast<rbs_refine_body*>(a->d_out + refine::kRecOff);
    rbs_refine_history* d_hist = reinterpret_cast<rbs_refine_history*>(a->d_out + refine::kHistOff);
    const size_t hist_bytes = sizeof(rbs_refine_history) * (size_t)p.iters * planes;
    a->n = 0;
    std::memcpy(h_out, poses_in, sizeof(double) * 12 * (size_t)planes);
    RBS_HIP(h, hipMemcpyAsync(d_poses, h_out, sizeof(double) * 12 * (size_t)planes, hipMemcpyHostToDevice, s));
    RBS_HIP(h, hipMemsetAsync(d_rec, 0, sizeof(rbs_refine_body) * (size_t)planes, s));
    RBS_HIP(h, hipMemsetAsync(a->d_frozen, 0, sizeof(int) * (size_t)planes, s));
    rbs::RefineArgs A{};
    A.S = rbs::PlaneSet{a->d_planes, a->d_rects, h->cols, h->npx, B};
    A.frame = d_frame;
    A.rows = h->rows;
    A.fx = h->base.fx; A.fy = h->base.fy; A.cx = h->base.cx; A.cy = h->base.cy;
    A.ms = h->base.ms; A.sf = h->base.sf;
    A.gate = p.gate_sigmas; A.huber = p.huber_sigmas; A.damping = p.damping;
    A.max_rot = p.max_rotation; A.max_trans = p.max_translation;
    A.eps_rot = p.eps_rotation; A.eps_trans = p.eps_translation;
    A.min_pixels = p.min_pixels;
    A.poses = d_poses;
    A.partial = a->d_partial;
    A.pcount = a->d_pcount;
    A.frozen = a->d_frozen;
    A.rec = d_rec;
    A.hist = d_hist;
    RBS_HIP(h, hipEventRecord(a->ev[0], s));
    for (int it = 0; it < p.iters; ++it) {
        A.it = it;
        rbs::launch_pose_planes(s, h->base, d_poses, n, true, a->d_planes, a->d_rects, nullptr);
        RBS_HIP(h, hipGetLastError());
        RBS_HIP(h, hipEventRecord(a->ev[3 * it + 1], s));
        hipLaunchKernelGGL(rbs::rbs_refine_accumulate_kernel, dim3((unsigned)planes, rbs::kRefineParts), dim3(256), 0, s, A);
        RBS_HIP(h, hipGetLastError());
        RBS_HIP(h, hipEventRecord(a->ev[3 * it + 2], s));
        hipLaunchKernelGGL(rbs::rbs_refine_solve_kernel, dim3((unsigned)planes), dim3(64), 0, s, A);
        RBS_HIP(h, hipGetLastError());
        RBS_HIP(h, hipEventRecord(a->ev[3 * it + 3], s));
    }
    RBS_HIP(h, hipMemcpyAsync(h_out, a->d_out, refine::kHistOff + hist_bytes, hipMemcpyDeviceToHost, s));
    RBS_HIP(h, hipStreamSynchronize(s));
    a->ms[0] = a->ms[1] = a->ms[2] = 0.f;
    for (int e = 0; e < 3 * p.iters; ++e) {
        float ms = 0.f;
        RBS_HIP(h, hipEventElapsedTime(&ms, a->ev[e], a->ev[e + 1]));
        a->ms[e % 3] += ms;
    }
    std::memcpy(poses_out, h_out, sizeof(double) * 12 * (size_t)planes);
    if (records_out) std::memcpy(records_out, h_out + refine::kRecOff, sizeof(rbs_refine_body) * (size_t)planes);
    a->n = n;
    a->iters = p.iters;
    return RBS_OK;
}

int32_t rbs_refine_get_history(rbs_handle* h, int32_t k, int32_t b, int32_t iteration, rbs_refine_history* out)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    const rbs_refine_state* a = h->refine;
    if (!out || !a || a->n < 1 || k < 0 || k >= a->n || b < 0 || b >= h->n_bodies || iteration < 0 || iteration >= a->iters)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "refine_get_history: no poses refined yet, a bad index or a null pointer");
    // (the last call's copy is still in the pinned buffer: every call ends synchronised)
    const rbs_refine_history* hist = reinterpret_cast<const rbs_refine_history*>(a->h_pin + refine::pin_out_off(h) + refine::kHistOff);
    *out = hist[(size_t)iteration * a->n * h->n_bodies + (size_t)k * h->n_bodies + b];
    return RBS_OK;
}

int32_t rbs_refine_kernel_ms(rbs_handle* h, float* out3)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!out3 || !h->refine || h->refine->n < 1) return fail(h, RBS_ERR_INVALID_ARGUMENT, "refine_kernel_ms: no poses refined yet or a null pointer");
    for (int k = 0; k < 3; ++k) out3[k] = h->refine->ms[k];
    return RBS_OK;
}

}  // extern "C"
