// rbsensor_find_scene.hip -- the scene finder (rbs_find_scene_*, include/rbsensor_mi355x.h): every body of a
// model of several from one depth frame.  Included at the end of rbsensor_find.hip's part of the translation unit: it owns one
// per-part finder (find_create_part) per body and a B-body scoring handle (make_scorer), so every score is the sensor's.
//
// Per scene find, on the B-body scoring handle's stream, for each searched body in S1's order:
//   rbs_planes_render_kernel<true>  (rbs_pose_planes.h, as the assessor's) the B bodies' planes at the poses so far, into the
//                              scene finder's own buffers
//   rbs_finds_residual_kernel  the residual frame: the union of the placed bodies' rectangles grown by the radius, in tiles of
//                              32 x 32 pixels; a tile and its halo are staged in LDS once as (support, depth) and every thread
//                              tests its pixels against the (2r + 1)^2 staged neighbours; pixels outside the grown union are
//                              copied through.  One writer per pixel: no atomics.
//   (find_run)                 the body's own finder on the residual frame (rbsensor_find.hip)
// then the joint polish:
//   rbs_finds_children_kernel  a round's children [children][B][12]: body c perturbed by step 6's code, the others copied
//   (rbs_loglikes_device)      their B-body scores on the original frame
//   rbs_finds_select_kernel    the best child (step 6's tie rule) becomes X
// Every order is fixed: the same frame gives the same bits.
// (Named rbs_finds_*: the rbs_find_*_kernel names are a closed list, tests/test_finder_cpu.py.)
#include <chrono>

namespace rbf {

constexpr int kResBlocks = 64;                                  // the residual kernel's grid
constexpr int kResTile = 32;                                    // interior pixels per tile side
constexpr int kResMaxRadius = 8;
constexpr int kResStage = kResTile + 2 * kResMaxRadius;         // 48: the staged side at the largest radius
constexpr int kResPerThread = kResTile * kResTile / 256;        // interior pixels of a thread
constexpr unsigned kResNaN = 0x7FC00000u;                       // an explained pixel
constexpr int kSceneMaxSweeps = 8, kSceneMaxChildren = 1024;

struct ResidualArgs {
    rbs::PlaneSet S;          // [B] planes of one pose
    const unsigned* frame;    // the frame's bits
    unsigned* out;            // the residual frame's bits
    int rows, radius;
    unsigned placed;          // bit b: body b is placed
    double sigmas, ms, sf;    // tau = sigmas (ms + sf d d)
};

// neither in front nor behind: the assess rule's support test
__device__ inline bool res_agrees(const ResidualArgs& A, float y, float depth)
{
    return rbs::planes_class(y, depth, A.sigmas, A.ms, A.sf) == rbs::kPlaneSupport;
}

__global__ __launch_bounds__(256) void rbs_finds_residual_kernel(const ResidualArgs A)
{
    __shared__ float s_depth[kResStage * kResStage];            // depth(j) of a staged pixel (its owner's plane)
    __shared__ unsigned char s_support[kResStage * kResStage];  // 1: j is a support pixel
    __shared__ int4 s_rect[rbs::kMaxBodies];
    const rbs::PlaneSet& PS = A.S;
    const int tid = threadIdx.x, B = PS.B, r = A.radius, cols = PS.cols, rows = A.rows;
    const int S = kResTile + 2 * r;                             // staged side
    if (tid < B) s_rect[tid] = PS.rects[tid];
    __syncthreads();
    const int4 u = rbs::planes_union_rect(PS, s_rect, A.placed);
    int x0 = u.x, y0 = u.y, x1 = u.z, y1 = u.w;
    const bool any = x1 > x0;                                   // (block-uniform)
    if (any) { x0 = max(x0 - r, 0); y0 = max(y0 - r, 0); x1 = min(x1 + r, cols); y1 = min(y1 + r, rows); }
    // outside the grown union: the frame's bits
    for (int p = blockIdx.x * 256 + tid; p < PS.npx; p += gridDim.x * 256) {
        const int y = p / cols, x = p - y * cols;
        if (any && x >= x0 && x < x1 && y >= y0 && y < y1) continue;
        A.out[p] = A.frame[p];
    }
    if (!any) return;
    const int nx = (x1 - x0 + kResTile - 1) / kResTile, ny = (y1 - y0 + kResTile - 1) / kResTile;
    for (int t = blockIdx.x; t < nx * ny; t += gridDim.x) {
        const int ty = t / nx;
        const int tx0 = x0 + (t - ty * nx) * kResTile, ty0 = y0 + ty * kResTile;
        __syncthreads();                                        // the last tile's readers are through
        for (int p = tid; p < S * S; p += 256) {
            const int sy = p / S, x = tx0 - r + (p - sy * S), y = ty0 - r + sy;
            float best = INFINITY;
            bool support = false;
            if (x >= 0 && x < cols && y >= 0 && y < rows) {
                const int i = y * cols + x;
                (void)rbs::planes_owner(PS, PS.planes, s_rect, A.placed, x, y, i, best);   // the placed bodies' nearest depth
                if (best < INFINITY) {
                    const float yv = __uint_as_float(A.frame[i]);
                    support = fabsf(yv) < INFINITY && res_agrees(A, yv, best);   // (NaN fails the first comparison)
                }
            }
            s_depth[p] = best;
            s_support[p] = support ? 1 : 0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kResPerThread; ++q) {
            const int p = tid + q * 256, iy = p / kResTile, ix = p - iy * kResTile;
            const int x = tx0 + ix, y = ty0 + iy;
            if (x >= x1 || y >= y1) continue;
            const int i = y * cols + x;
            const unsigned bits = A.frame[i];
            const float yv = __uint_as_float(bits);
            bool explained = s_support[(iy + r) * S + ix + r] != 0;           // rule (a)
            if (!explained && fabsf(yv) < INFINITY) {                          // rule (b): staged rows iy .. iy + 2r, columns ix .. ix + 2r
                for (int dy = 0; dy <= 2 * r && !explained; ++dy)
                    for (int dx = 0; dx <= 2 * r; ++dx) {
                        const int j = (iy + dy) * S + ix + dx;
                        if (s_support[j] && res_agrees(A, yv, s_depth[j])) { explained = true; break; }
                    }
            }
            A.out[i] = explained ? kResNaN : bits;
        }
    }
}

// One thread per (child, body) of polish round `round`: out [children][B][12] from X [B][12]; body c of child j > 0 by step 6's
// perturbation with the counter's round word 0x10000 + round.
__global__ __launch_bounds__(256) void rbs_finds_children_kernel(const double* __restrict__ X, int B, int c, int children, int round,
                                                                 unsigned long long seed, double st, double sa, double* __restrict__ out)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= children * B) return;
    const int j = g / B, b = g - j * B;
    const double* P = X + (size_t)b * 12;
    double* o = out + (size_t)g * 12;
    if (j == 0 || b != c) {
#pragma unroll
        for (int e = 0; e < 12; ++e) o[e] = P[e];
        return;
    }
    double nz[6];
    child_normals(seed, 0x10000 + round, c, j, nz);
    perturb_pose(P, nz, st, sa, o);
}

// One wave: the best child (ties: lowest j; NaN never beats a number; all NaN: child 0) becomes X [B][12]; *score, *best.
__global__ __launch_bounds__(64) void rbs_finds_select_kernel(const double* __restrict__ child, const double* __restrict__ child_score,
                                                              int children, int B, double* __restrict__ X, double* __restrict__ score,
                                                              int* __restrict__ best_out)
{
    int best = 0;
    double bs = child_score[0];
    for (int j = 1; j < children; ++j) {                        // (every lane the same walk: no exchange needed)
        const double s = child_score[j];
        if (s > bs || (bs != bs && s == s)) { bs = s; best = j; }
    }
    const double* P = child + (size_t)best * 12 * B;
    for (int e = threadIdx.x; e < 12 * B; e += 64) X[e] = P[e];
    if (threadIdx.x == 0) { *score = bs; *best_out = best; }
}

}  // namespace rbf

static_assert(sizeof(rbs_find_scene_params) == 48 && offsetof(rbs_find_scene_params, polish_sigma_translation) == 24,
              "rbs_find_scene_params layout is mirrored by dbot_ros_amd/_capi.py");
static_assert(rbf::kResMaxRadius == rbs::kContourMaxRadius, "the residual kernel stages its halo as the contour kernel does");

struct rbs_find_scene {
    rbs_handle* s = nullptr;              // the sensor (borrowed)
    rbs_find_params fp{};
    rbs_find_scene_params sp{};
    int B = 0;
    rbs_find* body[rbs::kMaxBodies] = {}; // part b's finder
    rbs_handle* joint = nullptr;          // the B-body scoring handle (max_particles = polish_children, one occlusion slot)
    hipStream_t st = nullptr;             // = joint->stream
    double e[rbs::kMaxBodies] = {};       // S1's e_b
    int rounds_cap = 0;                   // polish_sweeps * B
    float* h_frame = nullptr;             // pinned staging of the frame
    double* h_X = nullptr;                // pinned [B][12] + the joint score
    float* d_frame = nullptr;             // [npx]
    float* d_planes = nullptr;            // [B][npx]
    int4* d_rects = nullptr;              // [B]
    float* d_resid = nullptr;             // [B][npx] the residual frame each searched body was found on
    double* d_X = nullptr;                // [B][12]
    double* d_child = nullptr;            // [max(1, rounds_cap)][children][B][12]
    double* d_child_score = nullptr;      // [max(1, rounds_cap)][children]
    double* d_joint = nullptr;            // [1]
    int* d_best = nullptr;                // [max(1, rounds_cap)]
    int* d_zero = nullptr;                // [children] parent indices: all 0
    hipEvent_t ev[3] = {};
    // the last scene find
    bool have = false;
    int order[rbs::kMaxBodies] = {};
    int ns = 0;
    uint32_t searched = 0;
    int rounds_run = -1;                  // polish rounds of the last find (-1: the polish was skipped)
    float ms_body[rbs::kMaxBodies] = {};
    float ms[4] = {};                     // render, residual, polish, whole
    std::string err;
};

namespace {

int32_t sfail(rbs_find_scene* f, int32_t code, const std::string& msg) { f->err = msg; return code; }

const char* scene_check(const rbs_find_scene_params* p)
{
    if (!(p->explain_sigmas > 0.0) || !std::isfinite(p->explain_sigmas)) return "find_scene: explain_sigmas must be finite and > 0";
    if (p->explain_radius < 0 || p->explain_radius > rbf::kResMaxRadius) return "find_scene: explain_radius outside 0..8";
    if (p->polish_sweeps < 0 || p->polish_sweeps > rbf::kSceneMaxSweeps) return "find_scene: polish_sweeps outside 0..8";
    if (p->polish_children < 1 || p->polish_children > rbf::kSceneMaxChildren) return "find_scene: polish_children outside 1..1024";
    if (!(p->polish_sigma_translation >= 0.0) || !std::isfinite(p->polish_sigma_translation) || !(p->polish_sigma_angle >= 0.0) ||
        !std::isfinite(p->polish_sigma_angle))
        return "find_scene: polish_sigma_translation and polish_sigma_angle must be finite and >= 0";
    if (!(p->polish_decay > 0.0) || !(p->polish_decay <= 1.0)) return "find_scene: polish_decay outside (0, 1]";
    return nullptr;
}

// the planes of the B bodies at d_X and the residual frame of the bodies in `placed`, into out; ms[0], ms[1] += the two kernels
int32_t scene_residual(rbs_find_scene* f, uint32_t placed, float* out)
{
    rbs_handle* j = f->joint;
    hipStream_t st = f->st;
    RBF_HIP(f, hipEventRecord(f->ev[0], st));
    rbs::launch_pose_planes(st, j->base, f->d_X, 1, true, f->d_planes, f->d_rects, nullptr);   // (j->base.n_bodies == f->B)
    RBF_HIP(f, hipGetLastError());
    RBF_HIP(f, hipEventRecord(f->ev[1], st));
    rbf::ResidualArgs A{};
    A.S = rbs::PlaneSet{f->d_planes, f->d_rects, j->cols, j->npx, f->B};
    A.frame = reinterpret_cast<const unsigned*>(f->d_frame);
    A.out = reinterpret_cast<unsigned*>(out);
    A.rows = j->rows;
    A.radius = f->sp.explain_radius;
    A.placed = placed;
    A.sigmas = f->sp.explain_sigmas;
    A.ms = j->base.ms;
    A.sf = j->base.sf;
    hipLaunchKernelGGL(rbf::rbs_finds_residual_kernel, dim3(rbf::kResBlocks), dim3(256), 0, st, A);
    RBF_HIP(f, hipGetLastError());
    RBF_HIP(f, hipEventRecord(f->ev[2], st));
    RBF_HIP(f, hipStreamSynchronize(st));
    float a = 0.f, b = 0.f;
    (void)hipEventElapsedTime(&a, f->ev[0], f->ev[1]);
    (void)hipEventElapsedTime(&b, f->ev[1], f->ev[2]);
    f->ms[0] += a;
    f->ms[1] += b;
    return RBS_OK;
}

}  // namespace

extern "C" {

void rbs_find_scene_default_params(rbs_find_scene_params* p)
{
    if (!p) return;
    p->explain_sigmas = 3.0;
    p->explain_radius = 2;
    p->polish_sweeps = 2;
    p->polish_children = 64;
    p->reserved = 0;
    p->polish_sigma_translation = 0.005;
    p->polish_sigma_angle = 5.0 * M_PI / 180.0;
    p->polish_decay = 0.6;
}

const char* rbs_find_scene_last_error(const rbs_find_scene* f) { return f ? f->err.c_str() : "null scene finder"; }

void rbs_find_scene_destroy(rbs_find_scene* f)
{
    if (!f) return;
    for (rbs_find*& b : f->body)
        if (b) { rbs_find_destroy(b); b = nullptr; }
    if (f->joint) (void)hipSetDevice(f->joint->device);
    if (f->st) (void)hipStreamSynchronize(f->st);
    for (void* q : {(void*)f->d_frame, (void*)f->d_planes, (void*)f->d_rects, (void*)f->d_resid, (void*)f->d_X, (void*)f->d_child,
                    (void*)f->d_child_score, (void*)f->d_joint, (void*)f->d_best, (void*)f->d_zero})
        if (q) (void)hipFree(q);
    if (f->h_frame) (void)hipHostFree(f->h_frame);
    if (f->h_X) (void)hipHostFree(f->h_X);
    for (hipEvent_t& e : f->ev)
        if (e) (void)hipEventDestroy(e);
    if (f->joint) release(f->joint);
    delete f;
}

int32_t rbs_find_scene_create(rbs_handle* sensor, const rbs_find_params* find_params, const rbs_find_scene_params* scene_params,
                              rbs_find_scene** out)
{
    if (out) *out = nullptr;
    rbs_find_scene_params sp;
    if (scene_params) sp = *scene_params; else rbs_find_scene_default_params(&sp);
    const char* bad = !find_params ? "find_scene_create: find_params is NULL" : !out ? "find_scene_create: out is NULL" : find_check(find_params);
    if (!bad) bad = scene_check(&sp);
    if (!bad && !sensor) bad = "find_scene_create: sensor is NULL";
    if (bad) {
        if (sensor) sensor->err = bad; else g_create_error = bad;
        return RBS_ERR_INVALID_ARGUMENT;
    }
    if (!sensor->shards.empty() || sensor->group || sensor->peer_world > 1)
        return fail(sensor, RBS_ERR_UNSUPPORTED, "find_scene_create: the scene finder runs on single-device handles only");
    rbs_find_scene* f = new (std::nothrow) rbs_find_scene;
    if (!f) return fail(sensor, RBS_ERR_OUT_OF_MEMORY, "find_scene_create: out of host memory");
    f->s = sensor;
    f->fp = *find_params;
    f->sp = sp;
    f->B = sensor->n_bodies;
    auto bail = [&](int32_t rc) { sensor->err = f->err; rbs_find_scene_destroy(f); return rc; };
    const int B = f->B, rows = sensor->rows, cols = sensor->cols;
    const size_t npx = (size_t)rows * cols;
    for (int b = 0; b < B; ++b) {
        size_t v0, t0;
        part_offsets(sensor, b, &v0, &t0);
        f->e[b] = mean_vertex_distance(sensor->cfg_vertices.data() + 3 * v0, (size_t)sensor->cfg_vertex_counts[b]);
        if (int32_t rc = find_create_part(sensor, find_params, b, &f->body[b])) { f->err = sensor->err; return bail(rc); }
    }
    if (int32_t rc = make_scorer(sensor, -1, &f->err, rows, cols, sensor->cfg.K, sp.polish_children, &f->joint)) return bail(rc);
    f->st = f->joint->stream;
    f->rounds_cap = sp.polish_sweeps * B;
    const size_t R = (size_t)std::max(1, f->rounds_cap), nc = (size_t)sp.polish_children;
    if (hipSetDevice(sensor->device) != hipSuccess ||
        hipHostMalloc(&f->h_frame, sizeof(float) * npx, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(&f->h_X, sizeof(double) * (12 * (size_t)B + 1), hipHostMallocDefault) != hipSuccess ||
        hipMalloc(&f->d_frame, sizeof(float) * npx) != hipSuccess ||
        hipMalloc(&f->d_planes, sizeof(float) * npx * B) != hipSuccess ||
        hipMalloc(&f->d_rects, sizeof(int4) * B) != hipSuccess ||
        hipMalloc(&f->d_resid, sizeof(float) * npx * B) != hipSuccess ||
        hipMalloc(&f->d_X, sizeof(double) * 12 * B) != hipSuccess ||
        hipMalloc(&f->d_child, sizeof(double) * 12 * B * nc * R) != hipSuccess ||
        hipMalloc(&f->d_child_score, sizeof(double) * nc * R) != hipSuccess ||
        hipMalloc(&f->d_joint, sizeof(double)) != hipSuccess ||
        hipMalloc(&f->d_best, sizeof(int) * R) != hipSuccess ||
        hipMalloc(&f->d_zero, sizeof(int) * nc) != hipSuccess ||
        hipMemset(f->d_zero, 0, sizeof(int) * nc) != hipSuccess) {
        (void)hipGetLastError();
        f->err = "find_scene_create: device or pinned memory";
        return bail(RBS_ERR_OUT_OF_MEMORY);
    }
    for (hipEvent_t& e : f->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            (void)hipGetLastError();
            f->err = "find_scene_create: events";
            return bail(RBS_ERR_HIP);
        }
    *out = f;
    return RBS_OK;
}

int32_t rbs_find_scene_set_foreground(rbs_find_scene* f, const rbs_find_foreground* g)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (g && g->enabled != 0)
        if (const char* bad = foreground_check(g)) return sfail(f, RBS_ERR_INVALID_ARGUMENT, bad);   // (before any body's setting changes)
    for (int b = 0; b < f->B; ++b)
        if (int32_t rc = rbs_find_set_foreground(f->body[b], g)) return sfail(f, rc, f->body[b]->err);
    return RBS_OK;
}

int32_t rbs_find_scene_set_refinement(rbs_find_scene* f, const rbs_find_refinement* g)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (g && g->enabled != 0)
        if (const char* bad = refinement_check(g, f->fp.children)) return sfail(f, RBS_ERR_INVALID_ARGUMENT, bad);
    for (int b = 0; b < f->B; ++b)
        if (int32_t rc = rbs_find_set_refinement(f->body[b], g)) return sfail(f, rc, f->body[b]->err);
    return RBS_OK;
}

int32_t rbs_find_scene_set_gate(rbs_find_scene* f, const rbs_find_gate* g)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (g && g->enabled != 0)
        if (const char* bad = gate_check(g)) return sfail(f, RBS_ERR_INVALID_ARGUMENT, std::string("find gate: ") + bad);
    for (int b = 0; b < f->B; ++b)
        if (int32_t rc = rbs_find_set_gate(f->body[b], g)) return sfail(f, rc, f->body[b]->err);
    return RBS_OK;
}

int32_t rbs_find_scene_run(rbs_find_scene* f, const float* frame, uint32_t search_mask, const double* given_poses, double* out_poses,
                           double* out_scores, uint32_t* found_mask, double* joint_score)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    const int B = f->B;
    const uint32_t all = B >= 32 ? 0xFFFFFFFFu : (1u << B) - 1u;
    if (!found_mask || !joint_score) return sfail(f, RBS_ERR_INVALID_ARGUMENT, "find_scene_run: a null found_mask / joint_score");
    if (search_mask == 0 || (search_mask & ~all)) return sfail(f, RBS_ERR_INVALID_ARGUMENT, "find_scene_run: search_mask is 0 or names a body >= n_objects");
    if (search_mask != all && !given_poses) return sfail(f, RBS_ERR_INVALID_ARGUMENT, "find_scene_run: given_poses is NULL while a body is not searched");
    for (int b = 0; b < B; ++b)
        if (!(search_mask >> b & 1u))
            for (int e = 0; e < 12; ++e)
                if (!std::isfinite(given_poses[12 * b + e]))
                    return sfail(f, RBS_ERR_INVALID_ARGUMENT, fmt("find_scene_run: given pose of body %d is not finite", b));
    const auto wall0 = std::chrono::steady_clock::now();
    rbs_handle* s = f->s;
    const size_t npx = (size_t)s->npx;
    RBF_HIP(f, hipSetDevice(s->device));
    if (frame) {
        std::memcpy(f->h_frame, frame, sizeof(float) * npx);
    } else {   // the sensor's current observation, as rbs_find_run reads it
        if (int32_t rc = rbs_get_observation(s, f->h_frame)) return sfail(f, rc, "find_scene_run: sensor: " + s->err);
    }
    f->have = false;
    f->rounds_run = -1;
    f->searched = search_mask;
    for (float& m : f->ms) m = 0.f;
    for (float& m : f->ms_body) m = 0.f;
    // S1: the searched bodies by e_b descending, ties to the lower b
    f->ns = 0;
    for (int b = 0; b < B; ++b)
        if (search_mask >> b & 1u) f->order[f->ns++] = b;
    std::stable_sort(f->order, f->order + f->ns, [&](int a, int b) { return f->e[a] > f->e[b]; });
    hipStream_t st = f->st;
    RBF_HIP(f, hipMemcpyAsync(f->d_frame, f->h_frame, sizeof(float) * npx, hipMemcpyHostToDevice, st));
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<double> X(12 * (size_t)B, nan), score(B, nan);
    uint32_t placed = all & ~search_mask, posed = placed, found = 0;
    for (int b = 0; b < B; ++b)
        if (placed >> b & 1u) std::memcpy(&X[12 * (size_t)b], given_poses + 12 * b, sizeof(double) * 12);
    for (int i = 0; i < f->ns; ++i) {
        const int b = f->order[i];
        float* resid = f->d_resid + (size_t)b * npx;
        if (placed) {   // S2 (a body not placed is rendered where it does no harm and is masked out)
            for (int c = 0; c < B; ++c) {
                double* d = f->h_X + 12 * c;
                if (placed >> c & 1u) { std::memcpy(d, &X[12 * (size_t)c], sizeof(double) * 12); continue; }
                for (int e = 0; e < 12; ++e) d[e] = e == 0 || e == 4 || e == 8 || e == 11 ? 1.0 : 0.0;
            }
            RBF_HIP(f, hipMemcpyAsync(f->d_X, f->h_X, sizeof(double) * 12 * B, hipMemcpyHostToDevice, st));
            if (int32_t rc = scene_residual(f, placed, resid)) return rc;
        } else {
            RBF_HIP(f, hipMemcpyAsync(resid, f->d_frame, sizeof(float) * npx, hipMemcpyDeviceToDevice, st));
            RBF_HIP(f, hipStreamSynchronize(st));
        }
        // S3
        double pose[12], sc = nan;
        int32_t n = 0, fnd = 0;
        rbs_find* fb = f->body[b];
        if (int32_t rc = find_run(fb, nullptr, resid, 1, pose, &sc, &n, &fnd)) return sfail(f, rc, fmt("find_scene_run: body %d: ", b) + fb->err);
        f->ms_body[b] = fb->ms[4];
        if (n < 1) continue;
        std::memcpy(&X[12 * (size_t)b], pose, sizeof(pose));
        score[b] = sc;
        posed |= 1u << b;
        if (fnd) { placed |= 1u << b; found |= 1u << b; }
    }
    // S4
    double joint = nan;
    if (posed == all) {
        rbs_handle* j = f->joint;
        RBF_RC(f, j, rbs_reset(j));
        RBF_RC(f, j, rbs_set_observation_device(j, f->d_frame, st));
        std::memcpy(f->h_X, X.data(), sizeof(double) * 12 * B);
        RBF_HIP(f, hipEventRecord(f->ev[0], st));
        RBF_HIP(f, hipMemcpyAsync(f->d_X, f->h_X, sizeof(double) * 12 * B, hipMemcpyHostToDevice, st));
        const int nc = f->sp.polish_children, rounds = f->sp.polish_sweeps * f->ns;
        double st_w = f->sp.polish_sigma_translation, sa_w = f->sp.polish_sigma_angle;
        for (int r = 0; r < rounds; ++r) {
            if (r > 0 && r % f->ns == 0) { st_w *= f->sp.polish_decay; sa_w *= f->sp.polish_decay; }
            double* cp = f->d_child + (size_t)r * 12 * B * nc;
            double* cs = f->d_child_score + (size_t)r * nc;
            hipLaunchKernelGGL(rbf::rbs_finds_children_kernel, dim3((unsigned)((nc * B + 255) / 256)), dim3(256), 0, st, f->d_X, B,
                               f->order[r % f->ns], nc, r, (unsigned long long)f->fp.seed, st_w, sa_w, cp);
            RBF_HIP(f, hipGetLastError());
            RBF_RC(f, j, rbs_loglikes_device(j, cp, f->d_zero, nc, 0, cs, st));
            hipLaunchKernelGGL(rbf::rbs_finds_select_kernel, dim3(1), dim3(64), 0, st, cp, cs, nc, B, f->d_X, f->d_joint, f->d_best + r);
            RBF_HIP(f, hipGetLastError());
        }
        if (rounds == 0) {   // no polish: X is scored once
            RBF_HIP(f, hipMemcpyAsync(f->d_child, f->d_X, sizeof(double) * 12 * B, hipMemcpyDeviceToDevice, st));
            RBF_RC(f, j, rbs_loglikes_device(j, f->d_child, f->d_zero, 1, 0, f->d_child_score, st));
            hipLaunchKernelGGL(rbf::rbs_finds_select_kernel, dim3(1), dim3(64), 0, st, f->d_child, f->d_child_score, 1, B, f->d_X, f->d_joint,
                               f->d_best);
            RBF_HIP(f, hipGetLastError());
        }
        RBF_HIP(f, hipMemcpyAsync(f->h_X, f->d_X, sizeof(double) * 12 * B, hipMemcpyDeviceToHost, st));
        RBF_HIP(f, hipMemcpyAsync(f->h_X + 12 * B, f->d_joint, sizeof(double), hipMemcpyDeviceToHost, st));
        RBF_HIP(f, hipEventRecord(f->ev[1], st));
        RBF_HIP(f, hipStreamSynchronize(st));
        (void)hipEventElapsedTime(&f->ms[2], f->ev[0], f->ev[1]);
        std::memcpy(X.data(), f->h_X, sizeof(double) * 12 * B);
        joint = f->h_X[12 * B];
        f->rounds_run = rounds;
    }
    f->ms[3] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    f->have = true;
    if (out_poses) std::memcpy(out_poses, X.data(), sizeof(double) * 12 * B);
    if (out_scores) std::memcpy(out_scores, score.data(), sizeof(double) * B);
    *found_mask = found;
    *joint_score = joint;
    return RBS_OK;
}

int32_t rbs_find_scene_get_order(rbs_find_scene* f, int32_t* order, int32_t* n, double* e)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (!n || !f->have) return sfail(f, RBS_ERR_INVALID_ARGUMENT, "find_scene_get_order: no scene find yet, or a null pointer");
    *n = f->ns;
    for (int i = 0; order && i < f->ns; ++i) order[i] = f->order[i];
    for (int b = 0; e && b < f->B; ++b) e[b] = f->e[b];
    return RBS_OK;
}

int32_t rbs_find_scene_get_residual(rbs_find_scene* f, int32_t body, float* out)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (!out || !f->have || body < 0 || body >= f->B || !(f->searched >> body & 1u))
        return sfail(f, RBS_ERR_INVALID_ARGUMENT, "find_scene_get_residual: no scene find yet, a body that was not searched, or a null pointer");
    RBF_HIP(f, hipSetDevice(f->s->device));
    RBF_HIP(f, hipMemcpy(out, f->d_resid + (size_t)body * f->s->npx, sizeof(float) * (size_t)f->s->npx, hipMemcpyDeviceToHost));
    return RBS_OK;
}

rbs_find* rbs_find_scene_body_finder(rbs_find_scene* f, int32_t body)
{
    return f && body >= 0 && body < f->B ? f->body[body] : nullptr;
}

int32_t rbs_find_scene_get_polish(rbs_find_scene* f, int32_t round, double* poses, double* scores, int32_t* n, int32_t* best)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (!n) return sfail(f, RBS_ERR_INVALID_ARGUMENT, "find_scene_get_polish: n is NULL");
    if (!f->have || f->rounds_run < 0) return sfail(f, RBS_ERR_INVALID_ARGUMENT, "find_scene_get_polish: no scene find with a polish yet");
    if (round < 0 || round >= std::max(1, f->rounds_run)) return sfail(f, RBS_ERR_INVALID_ARGUMENT, "find_scene_get_polish: round outside the last polish");
    const size_t nc = f->rounds_run == 0 ? 1 : (size_t)f->sp.polish_children, B = (size_t)f->B;
    const size_t slot = (size_t)f->sp.polish_children;
    *n = (int32_t)nc;
    RBF_HIP(f, hipSetDevice(f->s->device));
    if (poses) RBF_HIP(f, hipMemcpy(poses, f->d_child + (size_t)round * 12 * B * slot, sizeof(double) * 12 * B * nc, hipMemcpyDeviceToHost));
    if (scores) RBF_HIP(f, hipMemcpy(scores, f->d_child_score + (size_t)round * slot, sizeof(double) * nc, hipMemcpyDeviceToHost));
    if (best) RBF_HIP(f, hipMemcpy(best, f->d_best + round, sizeof(int), hipMemcpyDeviceToHost));
    return RBS_OK;
}

int32_t rbs_find_scene_stage_ms(rbs_find_scene* f, float* per_body, float* out4)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (!out4 || !f->have) return sfail(f, RBS_ERR_INVALID_ARGUMENT, "find_scene_stage_ms: no scene find yet, or a null pointer");
    for (int b = 0; per_body && b < f->B; ++b) per_body[b] = f->ms_body[b];
    for (int i = 0; i < 4; ++i) out4[i] = f->ms[i];
    return RBS_OK;
}

}  // extern "C"
