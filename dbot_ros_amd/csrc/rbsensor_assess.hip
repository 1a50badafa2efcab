// rbsensor_assess.hip -- poses judged against one depth frame (rbs_assess_*, include/rbsensor_mi355x.h; the rule:
// DESIGN.md Appendix J).  Included by rbsensor_capi.hip ahead of create_impl, behind rbs_pose_planes.h: it uses the handle,
// its observation and the shared planes, and sensor release calls assess_release.
//
// Per call, on the sensor's stream:
//   rbs_planes_render_kernel<true>  (rbs_pose_planes.h) one plane per (pose, body): body b alone in its own screen
//                             rectangle, so the minimum over the bodies is bit-identical to rbs_render_depth.
//   rbs_assess_count_kernel   a fixed grid per pose over the union of its bodies' rectangles: owner and class per pixel
//                             (planes_owner, planes_class), integer counts in LDS, one integer global add per block and
//                             counter.
// Integer sums do not depend on their order: the same inputs give the same counts, run after run.  The verdict is
// taken on the host from the counts (assess::verdict_of, also rbs_assess_verdict).
// rbs_contour_poses (rbsensor_contour.hip) is the same call with one more kernel behind the count kernel, on the same
// planes: assess::run below serves both entry points.
namespace rbs {

constexpr int kAssessMaxPlanes = 64;      // n x n_objects of one call
constexpr int kAssessCountBlocks = 32;    // blocks per pose of the count kernel
constexpr int kAssessFields = 8;          // int32 per record (rbs_assess_body)

struct AssessArgs {
    PlaneSet S;               // the n x B planes of the call
    const float* frame;
    double sigmas, ms, sf;    // tau = sigmas (ms + sf d d)
    int* rec;                 // [n x B][kAssessFields], zeroed: rendered, valid, support, in_front, behind
};

// Owner and class of every pixel of pose blockIdx.y's rectangle (the union of its bodies').
__global__ __launch_bounds__(256) void rbs_assess_count_kernel(const AssessArgs A)
{
    __shared__ int s_cnt[kMaxBodies * 5];
    __shared__ int4 s_rect[kMaxBodies];
    const PlaneSet& S = A.S;
    const int tid = threadIdx.x, k = blockIdx.y, B = S.B;
    for (int e = tid; e < B * 5; e += 256) s_cnt[e] = 0;
    if (tid < B) s_rect[tid] = S.rects[k * B + tid];
    __syncthreads();
    const int4 u = planes_union_rect(S, s_rect, 0xffffffffu);
    const int x0 = u.x, y0 = u.y, x1 = u.z, y1 = u.w;
    if (x1 > x0) {
        const int w = x1 - x0, total = w * (y1 - y0);
        const float* planes = S.planes + (size_t)k * B * S.npx;
        for (int p = blockIdx.x * 256 + tid; p < total; p += gridDim.x * 256) {
            const int ly = p / w, x = x0 + (p - ly * w), y = y0 + ly;
            const int i = y * S.cols + x;
            float best;
            const int owner = planes_owner(S, planes, s_rect, 0xffffffffu, x, y, i, best);
            if (owner < 0) continue;
            const float yv = A.frame[i];
            int* c = s_cnt + owner * 5;
            atomicAdd(c + 0, 1);
            if (!(fabsf(yv) < INFINITY)) continue;   // no reading (NaN fails the comparison too)
            atomicAdd(c + 1, 1);
            atomicAdd(c + 2 + planes_class(yv, best, A.sigmas, A.ms, A.sf), 1);   // support, in_front, behind
        }
    }
    __syncthreads();
    for (int e = tid; e < B * 5; e += 256) {
        const int v = s_cnt[e];
        if (v) atomicAdd(A.rec + (size_t)(k * B + e / 5) * kAssessFields + e % 5, v);
    }
}

}  // namespace rbs

static_assert(sizeof(rbs_assess_body) == 32 && sizeof(rbs_assess_body) == sizeof(int32_t) * rbs::kAssessFields &&
                  offsetof(rbs_assess_body, verdict) == 20,
              "rbs_assess_body layout is mirrored by dbot_ros_amd/_capi.py, the count kernel and tests/test_assess_cpu.py");
static_assert(sizeof(rbs_assess_params) == 32, "rbs_assess_params layout is mirrored by dbot_ros_amd/_capi.py");

// What a sensor owns once it has assessed: allocated at first use, grow-only, freed by rbs_destroy.
struct rbs_assess_state {
    int cap = 0;                    // planes the buffers hold
    float* d_planes = nullptr;      // [cap][npx]
    int4* d_rects = nullptr;        // [cap]
    int* d_rec = nullptr;           // [cap][8]
    int* d_crec = nullptr;          // [cap][8] the contour rule's records (rbsensor_contour.hip)
    double* d_poses = nullptr;      // [cap][12]
    float* d_frame = nullptr;       // [npx] a caller's frame
    unsigned char* h_pin = nullptr; // pinned: frame [npx] floats | poses [kAssessMaxPlanes][12] | records [kAssessMaxPlanes] | contour records [kAssessMaxPlanes]
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    float ms[3] = {0.f, 0.f, 0.f};   // render, count, contour
    int n = 0;                      // poses of the last call (0: none yet)
    bool contour = false;           // the last call was an rbs_contour_poses
};

namespace {

// rbsensor_contour.hip: the rim kernel behind the count kernel, on the planes and rectangles of A, into rec (zeroed).
int32_t contour_enqueue(rbs_handle* h, const rbs::AssessArgs& A, int n, int radius, int* rec);

namespace assess {

const char* check_params(const rbs_assess_params* p)
{
    if (!(p->sigmas > 0.0) || !std::isfinite(p->sigmas)) return "assess: sigmas must be finite and > 0";
    if (!(p->min_support_fraction >= 0.0 && p->min_support_fraction <= 1.0)) return "assess: min_support_fraction must lie in [0, 1]";
    if (!(p->min_visible_fraction >= 0.0 && p->min_visible_fraction <= 1.0)) return "assess: min_visible_fraction must lie in [0, 1]";
    if (p->min_pixels < 1) return "assess: min_pixels must be >= 1";
    return nullptr;
}

int32_t verdict_of(const rbs_assess_params& p, const rbs_assess_body& c)
{
    const int32_t u = c.support + c.behind;
    if (c.rendered < p.min_pixels) return RBS_ASSESS_OUT_OF_VIEW;
    if ((double)u < p.min_visible_fraction * (double)c.rendered) return RBS_ASSESS_OCCLUDED;
    if ((double)c.support >= p.min_support_fraction * (double)u) return RBS_ASSESS_SUPPORTED;
    return RBS_ASSESS_LOST;
}

size_t pin_poses_off(const rbs_handle* h) { return (sizeof(float) * (size_t)h->npx + 15) & ~(size_t)15; }
size_t pin_rec_off(const rbs_handle* h) { return pin_poses_off(h) + sizeof(double) * 12 * rbs::kAssessMaxPlanes; }
size_t pin_crec_off(const rbs_handle* h) { return pin_rec_off(h) + sizeof(rbs_assess_body) * rbs::kAssessMaxPlanes; }

int32_t ensure(rbs_handle* h, int planes)
{
    if (!h->assess) {
        h->assess = new (std::nothrow) rbs_assess_state;
        if (!h->assess) return fail(h, RBS_ERR_OUT_OF_MEMORY, "assess: out of host memory");
    }
    rbs_assess_state* a = h->assess;
    if (!a->h_pin) {
        RBS_HIP(h, hipHostMalloc(&a->h_pin, pin_crec_off(h) + sizeof(rbs_contour_body) * rbs::kAssessMaxPlanes, hipHostMallocDefault));
        RBS_HIP(h, hipMalloc(&a->d_frame, sizeof(float) * (size_t)h->npx));
        for (hipEvent_t& e : a->ev) RBS_HIP(h, hipEventCreate(&e));
    }
    if (planes > a->cap) {   // (grow-only; the stream is idle of this state's readers: every call ends synchronised)
        RBS_HIP(h, hipStreamSynchronize(h->stream));
        (void)hipFree(a->d_planes); (void)hipFree(a->d_rects); (void)hipFree(a->d_rec); (void)hipFree(a->d_crec); (void)hipFree(a->d_poses);
        a->d_planes = nullptr; a->d_rects = nullptr; a->d_rec = nullptr; a->d_crec = nullptr; a->d_poses = nullptr;
        a->cap = 0;
        a->n = 0;
        RBS_HIP(h, hipMalloc(&a->d_planes, sizeof(float) * (size_t)planes * h->npx));
        RBS_HIP(h, hipMalloc(&a->d_rects, sizeof(int4) * (size_t)planes));
        RBS_HIP(h, hipMalloc(&a->d_rec, sizeof(int) * rbs::kAssessFields * (size_t)planes));
        RBS_HIP(h, hipMalloc(&a->d_crec, sizeof(int) * rbs::kAssessFields * (size_t)planes));
        RBS_HIP(h, hipMalloc(&a->d_poses, sizeof(double) * 12 * (size_t)planes));
        a->cap = planes;
    }
    return RBS_OK;
}

// The assessor's planes are now those of n poses (0: of none, while they are being drawn), what rbs_assess_get_plane and
// the *_kernel_ms calls answer from; contour: an rbs_contour_poses drew them.  rbs_occlusion_bodies draws into them too.
void planes_hold(rbs_assess_state* a, int n, bool contour)
{
    a->n = n;
    a->contour = contour;
}

// rbs_assess_poses (contour == nullptr: its two kernels and nothing else) and rbs_contour_poses (contour: checked by the
// caller; one more kernel and one more copy; out_contour gets the counts, its caller takes the verdicts).  `who` names
// the entry point in the messages.  out may be NULL.
int32_t run(rbs_handle* h, const char* who, const rbs_assess_params* params, const rbs_contour_params* contour, const float* frame,
            const double* poses, int32_t n, rbs_assess_body* out, rbs_contour_body* out_contour)
{
    if (!poses) return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("%s: null pointer", who));
    if (n < 1) return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("%s: n < 1", who));
    rbs_assess_params p;
    if (params) p = *params; else rbs_assess_default_params(&p);
    if (const char* bad = check_params(&p)) return fail(h, RBS_ERR_INVALID_ARGUMENT, bad);
    if (!h->shards.empty() || h->group || h->peer_world > 1)
        return fail(h, RBS_ERR_UNSUPPORTED, fmt("%s: single-device handles only", who));
    const int B = h->n_bodies;
    if ((long)n * B > rbs::kAssessMaxPlanes)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("%s: n x n_objects = %ld exceeds %d", who, (long)n * B, rbs::kAssessMaxPlanes));
    const int planes = n * B;
    for (size_t i = 0; i < (size_t)planes * 12; ++i)
        if (!std::isfinite(poses[i])) return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("%s: pose entry %zu is not finite", who, i));
    RBS_REFUSE_POISONED(h);
    RBS_HIP(h, hipSetDevice(h->device));
    if (int32_t rc = ensure(h, planes)) return rc;
    rbs_assess_state* a = h->assess;
    hipStream_t s = h->stream;
    const size_t npx = (size_t)h->npx;
    const float* d_frame;
    if (frame) {
        std::memcpy(a->h_pin, frame, sizeof(float) * npx);
        RBS_HIP(h, hipMemcpyAsync(a->d_frame, a->h_pin, sizeof(float) * npx, hipMemcpyHostToDevice, s));
        d_frame = a->d_frame;
    } else {   // the sensor's current observation, as rbs_get_observation reads it (the kernels below run behind the sensor's queued work)
        if (int32_t rc = make_current(h, s)) return rc;
        d_frame = obs_frame(h);
    }
    double* h_poses = reinterpret_cast<double*>(a->h_pin + pin_poses_off(h));
    rbs_assess_body* h_rec = reinterpret_cast<rbs_assess_body*>(a->h_pin + pin_rec_off(h));
    rbs_contour_body* h_crec = reinterpret_cast<rbs_contour_body*>(a->h_pin + pin_crec_off(h));
    std::memcpy(h_poses, poses, sizeof(double) * 12 * (size_t)planes);
    RBS_HIP(h, hipMemcpyAsync(a->d_poses, h_poses, sizeof(double) * 12 * (size_t)planes, hipMemcpyHostToDevice, s));
    RBS_HIP(h, hipMemsetAsync(a->d_rec, 0, sizeof(int) * rbs::kAssessFields * (size_t)planes, s));
    if (contour) RBS_HIP(h, hipMemsetAsync(a->d_crec, 0, sizeof(int) * rbs::kAssessFields * (size_t)planes, s));
    planes_hold(a, 0, false);
    RBS_HIP(h, hipEventRecord(a->ev[0], s));
    rbs::launch_pose_planes(s, h->base, a->d_poses, n, true, a->d_planes, a->d_rects, nullptr);
    RBS_HIP(h, hipGetLastError());
    RBS_HIP(h, hipEventRecord(a->ev[1], s));
    rbs::AssessArgs A{};
    A.S = rbs::PlaneSet{a->d_planes, a->d_rects, h->cols, h->npx, B};
    A.frame = d_frame;
    A.sigmas = p.sigmas;
    A.ms = h->base.ms;
    A.sf = h->base.sf;
    A.rec = a->d_rec;
    hipLaunchKernelGGL(rbs::rbs_assess_count_kernel, dim3(rbs::kAssessCountBlocks, (unsigned)n), dim3(256), 0, s, A);
    RBS_HIP(h, hipGetLastError());
    RBS_HIP(h, hipEventRecord(a->ev[2], s));
    if (contour) {
        if (int32_t rc = contour_enqueue(h, A, n, contour->radius, a->d_crec)) return rc;
        RBS_HIP(h, hipEventRecord(a->ev[3], s));
        RBS_HIP(h, hipMemcpyAsync(h_crec, a->d_crec, sizeof(rbs_contour_body) * (size_t)planes, hipMemcpyDeviceToHost, s));
    }
    RBS_HIP(h, hipMemcpyAsync(h_rec, a->d_rec, sizeof(rbs_assess_body) * (size_t)planes, hipMemcpyDeviceToHost, s));
    RBS_HIP(h, hipStreamSynchronize(s));
    for (int k = 0; k < (contour ? 3 : 2); ++k) RBS_HIP(h, hipEventElapsedTime(&a->ms[k], a->ev[k], a->ev[k + 1]));
    for (int i = 0; out && i < planes; ++i) {
        out[i] = h_rec[i];
        out[i].verdict = verdict_of(p, out[i]);
        out[i].reserved[0] = out[i].reserved[1] = 0;
    }
    for (int i = 0; out_contour && i < planes; ++i) out_contour[i] = h_crec[i];
    planes_hold(a, n, contour != nullptr);
    return RBS_OK;
}

}  // namespace assess

// rbs_destroy (the handle's device is current and its streams are idle).
void assess_release(rbs_handle* h)
{
    rbs_assess_state* a = h->assess;
    if (!a) return;
    (void)hipFree(a->d_planes);
    (void)hipFree(a->d_rects);
    (void)hipFree(a->d_rec);
    (void)hipFree(a->d_crec);
    (void)hipFree(a->d_poses);
    (void)hipFree(a->d_frame);
    if (a->h_pin) (void)hipHostFree(a->h_pin);
    for (hipEvent_t e : a->ev)
        if (e) (void)hipEventDestroy(e);
    delete a;
    h->assess = nullptr;
}

}  // namespace

extern "C" {

void rbs_assess_default_params(rbs_assess_params* p)
{
    if (!p) return;
    p->sigmas = 3.0;
    p->min_support_fraction = 0.5;
    p->min_visible_fraction = 0.25;
    p->min_pixels = 16;
    p->reserved = 0;
}

int32_t rbs_assess_verdict(const rbs_assess_params* params, const rbs_assess_body* body, int32_t* verdict)
{
    if (!body || !verdict) return RBS_ERR_INVALID_ARGUMENT;
    rbs_assess_params p;
    if (params) p = *params; else rbs_assess_default_params(&p);
    if (assess::check_params(&p)) return RBS_ERR_INVALID_ARGUMENT;
    *verdict = assess::verdict_of(p, *body);
    return RBS_OK;
}

int32_t rbs_assess_poses(rbs_handle* h, const rbs_assess_params* params, const float* frame, const double* poses, int32_t n,
                         rbs_assess_body* out)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!out) return fail(h, RBS_ERR_INVALID_ARGUMENT, "assess_poses: null pointer");
    return assess::run(h, "assess_poses", params, nullptr, frame, poses, n, out, nullptr);
}

int32_t rbs_assess_get_plane(rbs_handle* h, int32_t k, int32_t b, float* out)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    const rbs_assess_state* a = h->assess;
    if (!out || !a || a->n < 1 || k < 0 || k >= a->n || b < 0 || b >= h->n_bodies)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "assess_get_plane: no poses assessed yet, a bad index or a null pointer");
    RBS_HIP(h, hipSetDevice(h->device));
    RBS_HIP(h, hipStreamSynchronize(h->stream));
    const size_t kb = (size_t)k * h->n_bodies + b;
    int4 r;
    RBS_HIP(h, hipMemcpy(&r, a->d_rects + kb, sizeof(int4), hipMemcpyDeviceToHost));
    RBS_HIP(h, hipMemcpy(out, a->d_planes + kb * h->npx, sizeof(float) * h->npx, hipMemcpyDeviceToHost));
    for (int row = 0; row < h->rows; ++row)   // the plane is valid inside its rectangle only
        for (int col = 0; col < h->cols; ++col)
            if (!(col >= r.x && col < r.z && row >= r.y && row < r.w)) out[(size_t)row * h->cols + col] = INFINITY;
    return RBS_OK;
}

int32_t rbs_assess_kernel_ms(rbs_handle* h, float* out2)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!out2 || !h->assess || h->assess->n < 1) return fail(h, RBS_ERR_INVALID_ARGUMENT, "assess_kernel_ms: no poses assessed yet or a null pointer");
    out2[0] = h->assess->ms[0];
    out2[1] = h->assess->ms[1];
    return RBS_OK;
}

}  // extern "C"
