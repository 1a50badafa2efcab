// rbsensor_contour.hip -- the silhouette of a pose judged against the frame (rbs_contour_*, include/rbsensor_mi355x.h;
// the rule: DESIGN.md Appendix J, "The contour rule").  Included by rbsensor_capi.hip behind rbsensor_assess.hip: the
// planes (rbs_planes_render_kernel<true>, rbs_pose_planes.h), rectangles, frame and buffers are the assessor's
// (rbs_assess_state), and rbs_contour_poses is assess::run with one more kernel behind the count kernel:
//   rbs_contour_count_kernel  a fixed grid per pose over the union of its bodies' rectangles grown by `radius`, in tiles
//                             of 32 x 32 pixels.  A tile and its halo are staged in LDS once as (owner, depth), composed
//                             from the B planes by the owner rule the count kernel uses (planes_owner); per body present in the staged tile a
//                             horizontal and then a vertical running maximum over (owner == b ? depth : -inf) gives the
//                             anchor of every interior pixel (a window maximum is separable); uncovered interior pixels
//                             with an anchor are the body's rim and are classed against the frame.  Integer counts in
//                             LDS, one integer global add per block and non-zero counter.
// Integer sums and a float maximum do not depend on their order: the same inputs give the same records, run after run.
namespace rbs {

constexpr int kContourBlocks = 32;        // blocks per pose
constexpr int kContourTile = 32;          // interior pixels per tile side
constexpr int kContourMaxRadius = 8;
constexpr int kContourStage = kContourTile + 2 * kContourMaxRadius;   // 48: the staged side at the largest radius
constexpr int kContourPerThread = kContourTile * kContourTile / 256;  // interior pixels of a thread

struct ContourArgs {
    AssessArgs A;             // planes, rects, frame, noise model; A.rec is not used
    int rows, radius;
    int* rec;                 // [n x B][kAssessFields], zeroed: rim, valid, flush, in_front, beyond
};

__global__ __launch_bounds__(256) void rbs_contour_count_kernel(const ContourArgs C)
{
    __shared__ float s_depth[kContourStage * kContourStage];        // depth(j) of a staged pixel (its owner's plane)
    __shared__ signed char s_owner[kContourStage * kContourStage];  // owner(j), -1: uncovered or outside the image
    __shared__ float s_row[kContourStage * kContourTile];           // one body's horizontal maxima [staged row][interior column]
    __shared__ int s_cnt[kMaxBodies * 5];
    __shared__ int4 s_rect[kMaxBodies];
    __shared__ unsigned s_present;                                  // bodies that own a staged pixel of this tile
    const AssessArgs& A = C.A;
    const PlaneSet& PS = A.S;
    const int tid = threadIdx.x, k = blockIdx.y, B = PS.B, r = C.radius, cols = PS.cols, rows = C.rows;
    const int S = kContourTile + 2 * r;                             // staged side
    for (int e = tid; e < B * 5; e += 256) s_cnt[e] = 0;
    if (tid < B) s_rect[tid] = PS.rects[k * B + tid];
    __syncthreads();
    const int4 u = planes_union_rect(PS, s_rect, 0xffffffffu);
    int x0 = u.x, y0 = u.y, x1 = u.z, y1 = u.w;
    if (x1 > x0) {                                                  // (block-uniform)
        x0 = max(x0 - r, 0); y0 = max(y0 - r, 0); x1 = min(x1 + r, cols); y1 = min(y1 + r, rows);
        const int nx = (x1 - x0 + kContourTile - 1) / kContourTile, ny = (y1 - y0 + kContourTile - 1) / kContourTile;
        const float* planes = PS.planes + (size_t)k * B * PS.npx;
        for (int t = blockIdx.x; t < nx * ny; t += gridDim.x) {
            const int ty = t / nx;
            const int tx0 = x0 + (t - ty * nx) * kContourTile, ty0 = y0 + ty * kContourTile;
            __syncthreads();                                        // the last tile's readers are through
            if (tid == 0) s_present = 0u;
            __syncthreads();
            unsigned mine = 0u;
            for (int p = tid; p < S * S; p += 256) {
                const int sy = p / S, x = tx0 - r + (p - sy * S), y = ty0 - r + sy;
                float best = INFINITY;
                int owner = -1;
                if (x >= 0 && x < cols && y >= 0 && y < rows) owner = planes_owner(PS, planes, s_rect, 0xffffffffu, x, y, y * cols + x, best);
                s_owner[p] = (signed char)owner;
                s_depth[p] = best;
                if (owner >= 0) mine |= 1u << owner;
            }
            if (mine) atomicOr(&s_present, mine);
            float yv[kContourPerThread];                            // the frame at this thread's interior pixels
            bool open[kContourPerThread];                           // inside the region and uncovered
#pragma unroll
            for (int q = 0; q < kContourPerThread; ++q) {
                const int p = tid + q * 256, iy = p / kContourTile, ix = p - iy * kContourTile;
                const int x = tx0 + ix, y = ty0 + iy;
                open[q] = x < x1 && y < y1;
                yv[q] = open[q] ? A.frame[y * cols + x] : 0.f;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < kContourPerThread; ++q) {
                const int p = tid + q * 256, iy = p / kContourTile, ix = p - iy * kContourTile;
                open[q] = open[q] && s_owner[(iy + r) * S + ix + r] < 0;
            }
            const unsigned present = s_present;
            for (int b = 0; b < B; ++b) {
                if (!(present >> b & 1u)) continue;                 // (block-uniform)
                for (int p = tid; p < S * kContourTile; p += 256) { // horizontal: the window of interior column ix is staged columns ix .. ix + 2r
                    const int sy = p / kContourTile, ix = p - sy * kContourTile;
                    float m = -INFINITY;
                    for (int dx = 0; dx <= 2 * r; ++dx) {
                        const int j = sy * S + ix + dx;
                        if (s_owner[j] == b) m = fmaxf(m, s_depth[j]);
                    }
                    s_row[p] = m;
                }
                __syncthreads();
                int rim = 0, flush = 0, front = 0, beyond = 0;
#pragma unroll
                for (int q = 0; q < kContourPerThread; ++q) {       // vertical: staged rows iy .. iy + 2r
                    if (!open[q]) continue;
                    const int p = tid + q * 256, iy = p / kContourTile, ix = p - iy * kContourTile;
                    float a = -INFINITY;
                    for (int dy = 0; dy <= 2 * r; ++dy) a = fmaxf(a, s_row[(iy + dy) * kContourTile + ix]);
                    if (!(a > -INFINITY)) continue;                 // no pixel of b in the window
                    ++rim;
                    if (!(fabsf(yv[q]) < INFINITY)) continue;       // no reading (NaN fails the comparison too)
                    const int cls = planes_class(yv[q], a, A.sigmas, A.ms, A.sf);
                    if (cls == kPlaneInFront) ++front; else if (cls == kPlaneBehind) ++beyond; else ++flush;
                }
                int* c = s_cnt + b * 5;
                if (rim) atomicAdd(c + 0, rim);
                if (flush + front + beyond) atomicAdd(c + 1, flush + front + beyond);
                if (flush) atomicAdd(c + 2, flush);
                if (front) atomicAdd(c + 3, front);
                if (beyond) atomicAdd(c + 4, beyond);
                __syncthreads();                                    // s_row is the next body's
            }
        }
    }
    __syncthreads();
    for (int e = tid; e < B * 5; e += 256) {
        const int v = s_cnt[e];
        if (v) atomicAdd(C.rec + (size_t)(k * B + e / 5) * kAssessFields + e % 5, v);
    }
}

}  // namespace rbs

static_assert(sizeof(rbs_contour_body) == 32 && sizeof(rbs_contour_body) == sizeof(int32_t) * rbs::kAssessFields &&
                  offsetof(rbs_contour_body, verdict) == 20,
              "rbs_contour_body layout is mirrored by dbot_ros_amd/_capi.py, the contour kernel and tests/test_contour_cpu.py");
static_assert(sizeof(rbs_contour_params) == 32 && offsetof(rbs_contour_params, min_valid_fraction) == 8 &&
                  offsetof(rbs_contour_params, min_flush_fraction) == 24,
              "rbs_contour_params layout is mirrored by dbot_ros_amd/_capi.py");
static_assert(rbs::kMaxBodies <= 32, "a body is a bit of s_present and a signed char of s_owner");

namespace {
namespace contour {

const char* check_params(const rbs_contour_params* p)
{
    if (p->radius < 1 || p->radius > rbs::kContourMaxRadius) return "contour: radius must lie in 1 .. 8";
    if (p->min_rim_pixels < 1) return "contour: min_rim_pixels must be >= 1";
    if (!(p->min_valid_fraction >= 0.0 && p->min_valid_fraction <= 1.0)) return "contour: min_valid_fraction must lie in [0, 1]";
    if (!(p->min_contour_fraction >= 0.0 && p->min_contour_fraction <= 1.0)) return "contour: min_contour_fraction must lie in [0, 1]";
    if (!(p->min_flush_fraction >= 0.0 && p->min_flush_fraction <= 1.0)) return "contour: min_flush_fraction must lie in [0, 1]";
    return nullptr;
}

int32_t verdict_of(const rbs_contour_params& p, const rbs_contour_body& c)
{
    if (c.rim < p.min_rim_pixels) return RBS_CONTOUR_NO_RIM;
    if (c.valid == 0 || (double)c.valid < p.min_valid_fraction * (double)c.rim) return RBS_CONTOUR_UNDECIDED;
    if ((double)c.beyond >= p.min_contour_fraction * (double)c.valid) return RBS_CONTOUR_PRESENT;
    if ((double)c.flush >= p.min_flush_fraction * (double)c.valid) return RBS_CONTOUR_ABSENT;
    return RBS_CONTOUR_UNDECIDED;
}

}  // namespace contour

// assess::run, behind the count kernel on the sensor's stream.
int32_t contour_enqueue(rbs_handle* h, const rbs::AssessArgs& A, int n, int radius, int* rec)
{
    rbs::ContourArgs C{};
    C.A = A;
    C.rows = h->rows;
    C.radius = radius;
    C.rec = rec;
    hipLaunchKernelGGL(rbs::rbs_contour_count_kernel, dim3(rbs::kContourBlocks, (unsigned)n), dim3(256), 0, h->stream, C);
    RBS_HIP(h, hipGetLastError());
    return RBS_OK;
}

}  // namespace

extern "C" {

void rbs_contour_default_params(rbs_contour_params* p)
{
    if (!p) return;
    p->radius = 2;
    p->min_rim_pixels = 16;
    p->min_valid_fraction = 0.5;
    p->min_contour_fraction = 0.3;
    p->min_flush_fraction = 0.5;
}

int32_t rbs_contour_verdict(const rbs_contour_params* params, const rbs_contour_body* body, int32_t* verdict)
{
    if (!body || !verdict) return RBS_ERR_INVALID_ARGUMENT;
    rbs_contour_params p;
    if (params) p = *params; else rbs_contour_default_params(&p);
    if (contour::check_params(&p)) return RBS_ERR_INVALID_ARGUMENT;
    *verdict = contour::verdict_of(p, *body);
    return RBS_OK;
}

int32_t rbs_contour_poses(rbs_handle* h, const rbs_assess_params* params, const rbs_contour_params* cparams, const float* frame,
                          const double* poses, int32_t n, rbs_assess_body* out_assess, rbs_contour_body* out_contour)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!out_contour) return fail(h, RBS_ERR_INVALID_ARGUMENT, "contour_poses: null pointer");
    rbs_contour_params c;
    if (cparams) c = *cparams; else rbs_contour_default_params(&c);
    if (const char* bad = contour::check_params(&c)) return fail(h, RBS_ERR_INVALID_ARGUMENT, bad);
    if (int32_t rc = assess::run(h, "contour_poses", params, &c, frame, poses, n, out_assess, out_contour)) return rc;
    const int planes = n * h->n_bodies;
    for (int i = 0; i < planes; ++i) {
        out_contour[i].verdict = contour::verdict_of(c, out_contour[i]);
        out_contour[i].reserved[0] = out_contour[i].reserved[1] = 0;
    }
    return RBS_OK;
}

int32_t rbs_contour_kernel_ms(rbs_handle* h, float* out3)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!out3 || !h->assess || h->assess->n < 1 || !h->assess->contour)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "contour_kernel_ms: the last assessment was not a contour_poses, or a null pointer");
    for (int k = 0; k < 3; ++k) out3[k] = h->assess->ms[k];
    return RBS_OK;
}

}  // extern "C"
