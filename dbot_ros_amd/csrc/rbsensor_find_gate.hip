// rbsensor_find_gate.hip -- the finder's opt-in silhouette gate (rbs_find_set_gate, include/rbsensor_mi355x.h steps 4b, 5
// and 7; DESIGN.md Appendix F, "Step 4b").  Included at the end of rbsensor_find.hip, ahead of the scene finder.
//
// With the gate on, a find has these launches more, on the finder's stream:
//   rbs_findc_evidence_kernel  one block per pose: the pose's screen rectangle grown by `radius` is walked in tiles of
//                              (64 - 2 radius)^2 interior pixels; a tile and its halo are rendered by raster_window into the
//                              LDS depth tile (no depth plane goes to global memory), a horizontal and then a vertical running
//                              maximum over the covered depths gives every uncovered interior pixel its anchor, and every
//                              thread classes its interior pixels against the frame: covered ones into the assess classes,
//                              uncovered ones with an anchor into the rim classes.  Ten integer counts in LDS; thread 0 writes
//                              them and the class.  One writer per pose: no global atomics, no float atomics.
//                              Step 4b: the coarse handle's DevParams, behind each scoring call on the same `batch` poses.
//                              Step 7: the full handle's DevParams on the S final survivors.
//   rbs_findc_mask_kernel      the gated order of step 5 is the chunked top-k run twice: the scores with every hypothesis
//   rbs_findc_merge_kernel     outside class c made NaN, c = 0 and then c = 1; the merge puts class 1's best behind class 0's
//                              numbers.  Both passes are rbs_find_topk_kernel's total order: the result is exact.
//   rbs_findc_order_kernel     one wave: step 7's order, the survivors' records and classes gathered in it.
// Integer counts and a float maximum do not depend on their order: the same frame gives the same records, run after run.
namespace rbf {

constexpr int kEvSide = 64;                        // the staged side: interior + 2 radius
constexpr int kEvStagePx = kEvSide * kEvSide;
constexpr int kEvFields = 10;                      // rendered, valid, support, in_front, behind | rim, valid, flush, in_front, beyond
constexpr int kEvMaxRadius = 8;                    // (the contour rule's)
constexpr size_t kEvRasterBytes = rbs::smem_bytes(kEvStagePx, false);
constexpr size_t kEvSmemBytes = kEvRasterBytes + sizeof(float) * kEvStagePx + 16 * sizeof(int);
static_assert(kEvRasterBytes % 16 == 0 && kEvSmemBytes <= 64 * 1024, "the evidence kernel's dynamic LDS: aligned, and within the default limit");
static_assert(kEvSide - 2 * kEvMaxRadius >= 16, "a tile keeps an interior at the largest radius");

struct EvArgs {
    const double* poses;      // [n][12]
    const float* frame;       // at the resolution of the DevParams
    int n, radius;
    double sigmas;            // tau = sigmas (ms + sf d d)
    int min_pixels, min_rim_pixels;
    double min_support_fraction, min_visible_fraction, min_valid_fraction, min_contour_fraction, min_flush_fraction;
    int* rec;                 // [n][kEvFields]
    int* cls;                 // [n]
};

// assess::verdict_of == SUPPORTED and contour::verdict_of == PRESENT, the same binary64 comparisons: class 0, else 1
__device__ __host__ inline int ev_class(const EvArgs& E, const int* c)
{
    const int rendered = c[0], support = c[2], behind = c[4], u = support + behind;
    bool supported = false;
    if (rendered < E.min_pixels) supported = false;
    else if ((double)u < E.min_visible_fraction * (double)rendered) supported = false;
    else supported = (double)support >= E.min_support_fraction * (double)u;
    const int rim = c[5], valid = c[6], beyond = c[9];
    bool present = false;
    if (rim < E.min_rim_pixels) present = false;
    else if (valid == 0 || (double)valid < E.min_valid_fraction * (double)rim) present = false;
    else present = (double)beyond >= E.min_contour_fraction * (double)valid;
    return supported && present ? 0 : 1;
}

// x, as far as the compiler can tell, differs from lane to lane: it and what is computed from it stay in vector registers
template <class T> __device__ inline void in_vgprs(T& x) { asm volatile("" : "+v"(x)); }

__global__ __launch_bounds__(rbs::kBlock) void rbs_findc_evidence_kernel(const rbs::DevParams P0, const EvArgs E)
{
    // raster_window holds the pose, the camera and the mesh's tables in scalar registers, more of them than a wave has: every
    // kernel that renders through it spills some into vector lanes (4 .. 44 SGPRs).  This kernel is far from its vector budget,
    // so what the rasterizer reads of P and the pose is declared per-lane here: 184 VGPRs, two waves per SIMD, nothing spilled.
    rbs::DevParams P = P0;
    in_vgprs(P.fx); in_vgprs(P.fy); in_vgprs(P.cx); in_vgprs(P.cy);
    in_vgprs(P.soup); in_vgprs(P.tri_plane); in_vgprs(P.tri_local); in_vgprs(P.cluster_sphere); in_vgprs(P.cluster_cone);
    in_vgprs(P.cluster_nv); in_vgprs(P.cluster_vtx);
    in_vgprs(P.sphere[0][0]); in_vgprs(P.sphere[0][1]); in_vgprs(P.sphere[0][2]); in_vgprs(P.sphere[0][3]);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const rbs::Smem m = rbs::carve(smem, kEvStagePx, false);
    float* s_row = reinterpret_cast<float*>(smem + kEvRasterBytes);   // horizontal maxima [staged row][interior column]
    int* s_cnt = reinterpret_cast<int*>(s_row + kEvStagePx);          // [kEvFields]
    const int tid = threadIdx.x, k = blockIdx.x, rad = E.radius, cols = P.cols, rows = P.rows;
    int lane_zero = 0;
    in_vgprs(lane_zero);
    const double* pose = E.poses + (size_t)k * 12 + lane_zero;
    int* s_geo = s_cnt + kEvFields;                                   // [6] the grown rectangle, tiles per row, tiles
    if (tid < kEvFields) s_cnt[tid] = 0;
    const rbs::Rect r = rbs::bodies_rect(P, pose, 0, 1);             // (every wave: the same rectangle)
    if (tid == 0) {
        const int gx0 = max(r.x0 - rad, 0), gy0 = max(r.y0 - rad, 0), gx1 = min(r.x1 + rad, cols), gy1 = min(r.y1 + rad, rows);
        const int T = kEvSide - 2 * rad;
        const int nx = (gx1 - gx0 + T - 1) / T, ny = (gy1 - gy0 + T - 1) / T;
        s_geo[0] = gx0; s_geo[1] = gy0; s_geo[2] = gx1; s_geo[3] = gy1; s_geo[4] = nx;
        s_geo[5] = r.x1 > r.x0 ? nx * ny : 0;
    }
    __syncthreads();
    // A tile's geometry is read from LDS ahead of the render and again behind it: nothing of it is held across raster_window.
    const int ntiles = __builtin_amdgcn_readfirstlane(s_geo[5]);
    {
        for (int t = 0; t < ntiles; ++t) {
            int ix0, iy0, ix1, iy1, sx0, sy0, sx1, sy1;
            auto tile_geo = [&]() {
                const int T = kEvSide - 2 * rad;                     // interior side
                const int gx0 = __builtin_amdgcn_readfirstlane(s_geo[0]), gy0 = __builtin_amdgcn_readfirstlane(s_geo[1]);
                const int gx1 = __builtin_amdgcn_readfirstlane(s_geo[2]), gy1 = __builtin_amdgcn_readfirstlane(s_geo[3]);
                const int nx = __builtin_amdgcn_readfirstlane(s_geo[4]);
                const int ty = t / nx;
                ix0 = gx0 + (t - ty * nx) * T; iy0 = gy0 + ty * T;
                ix1 = min(ix0 + T, gx1); iy1 = min(iy0 + T, gy1);
                sx0 = max(ix0 - rad, 0); sy0 = max(iy0 - rad, 0); sx1 = min(ix1 + rad, cols); sy1 = min(iy1 + rad, rows);
            };
            tile_geo();
            // the tile and its halo, culled as rbs_planes_render_kernel's; on return the tile is complete and synchronised
            rbs::raster_window<false, true>(P, pose, sx0, sy0, sx1, sy1, true, m.tile, m.big, m.nbig,
                                            m.evalq + (tid >> 6) * rbs::kQPlanes * rbs::kEvalQueue, 1u);
            tile_geo();
            const int sw = sx1 - sx0, sh = sy1 - sy0, iw = ix1 - ix0, ih = iy1 - iy0;
            for (int p = tid; p < sh * iw; p += rbs::kBlock) {       // horizontal: columns x - rad .. x + rad of the staged row
                const int sy = p / iw, x = ix0 + (p - sy * iw);
                const int a0 = max(x - rad, sx0) - sx0, a1 = min(x + rad, sx1 - 1) - sx0;
                const unsigned* row = m.tile + sy * sw;
                float mx = -INFINITY;
                for (int a = a0; a <= a1; ++a) {
                    const unsigned bits = row[a];
                    if (bits != rbs::kInfBits) mx = fmaxf(mx, __uint_as_float(bits));
                }
                s_row[p] = mx;
            }
            __syncthreads();
            int cnt[kEvFields];                                      // (wave-uniform: every count is a ballot's population)
#pragma unroll
            for (int e = 0; e < kEvFields; ++e) cnt[e] = 0;
            for (int p0 = 0; p0 < ih * iw; p0 += rbs::kBlock) {      // (a uniform trip count: the ballots below see every lane)
                const int p = p0 + tid;
                const bool in = p < ih * iw;
                bool covered = false, rim = false, reading = false, front = false, back = false;
                if (in) {
                    const int ly = p / iw, lx = p - ly * iw;
                    const int x = ix0 + lx, y = iy0 + ly;
                    const unsigned bits = m.tile[(y - sy0) * sw + (x - sx0)];
                    const float yv = E.frame[(size_t)y * cols + x];
                    float dep = __uint_as_float(bits);
                    covered = bits != rbs::kInfBits;                 // covered: the assess classes
                    if (!covered) {                                  // uncovered: the rim, when the window holds a covered pixel
                        const int b0 = max(y - rad, sy0) - sy0, b1 = min(y + rad, sy1 - 1) - sy0;
                        float a = -INFINITY;
                        for (int b = b0; b <= b1; ++b) a = fmaxf(a, s_row[b * iw + lx]);
                        rim = a > -INFINITY;
                        dep = a;
                    }
                    reading = (covered || rim) && fabsf(yv) < INFINITY;   // (NaN fails the comparison too)
                    const double d = (double)dep;
                    const double g = (double)yv - d;
                    const double tau = E.sigmas * (P.ms + P.sf * (d * d));
                    front = reading && g < -tau;
                    back = reading && !front && g > tau;
                }
                const bool mid = reading && !front && !back;
                cnt[0] += __popcll(__ballot(covered));
                cnt[1] += __popcll(__ballot(covered && reading));
                cnt[2] += __popcll(__ballot(covered && mid));
                cnt[3] += __popcll(__ballot(covered && front));
                cnt[4] += __popcll(__ballot(covered && back));
                cnt[5] += __popcll(__ballot(rim));
                cnt[6] += __popcll(__ballot(rim && reading));
                cnt[7] += __popcll(__ballot(rim && mid));
                cnt[8] += __popcll(__ballot(rim && front));
                cnt[9] += __popcll(__ballot(rim && back));
            }
            if ((tid & 63) == 0) {                                   // (s_cnt was zeroed ahead of the first tile's barriers)
#pragma unroll
                for (int e = 0; e < kEvFields; ++e)
                    if (cnt[e]) atomicAdd(s_cnt + e, cnt[e]);
            }
            __syncthreads();                                         // the tile and s_row are the next tile's
        }
    }
    __syncthreads();
    if (tid == 0) {
        int c[kEvFields];
#pragma unroll
        for (int e = 0; e < kEvFields; ++e) {
            c[e] = s_cnt[e];
            E.rec[(size_t)k * kEvFields + e] = c[e];
        }
        E.cls[k] = ev_class(E, c);
    }
}

// out [n] := score where the hypothesis is of class `want`, NaN elsewhere
__global__ __launch_bounds__(256) void rbs_findc_mask_kernel(const double* __restrict__ score, const int* __restrict__ cls, int want, long n,
                                                             double* __restrict__ out)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = cls[i] == want ? score[i] : __builtin_nan("");
}

// One block.  cand [nc]: class 0's best in order (its numbers first: NaN sorts last); fill [nc]: class 1's.  cand's entries
// behind its n0 numbers := fill [0 .. nc - n0).
__global__ __launch_bounds__(kMaxCandidates) void rbs_findc_merge_kernel(double* __restrict__ cand_s, long long* __restrict__ cand_i,
                                                                         const double* __restrict__ fill_s,
                                                                         const long long* __restrict__ fill_i, int nc)
{
    const int i = threadIdx.x;
    const bool number = i < nc && cand_s[i] == cand_s[i];
    const int n0 = __syncthreads_count(number);
    if (i >= n0 && i < nc) {
        cand_s[i] = fill_s[i - n0];
        cand_i[i] = fill_i[i - n0];
    }
}

// a before b in step 7's order: a number before NaN, then the lower class, the larger score, the smaller index
__device__ inline bool gate_before(double sa, int ca, int ia, double sb, int cb, int ib)
{
    const bool na = sa != sa, nb = sb != sb;
    if (na != nb) return nb;
    if (!na && ca != cb) return ca < cb;
    if (!na && sa != sb) return sa > sb;
    return ia < ib;
}

// One wave.  Survivor k's rank is the number of survivors before it; order [rank] := k, and its record and class go there too.
__global__ __launch_bounds__(64) void rbs_findc_order_kernel(const double* __restrict__ score, const int* __restrict__ cls,
                                                             const int* __restrict__ rec, int S, long long* __restrict__ order,
                                                             int* __restrict__ out_cls, int* __restrict__ out_rec)
{
    const int k = threadIdx.x;
    if (k >= S) return;
    const double s = score[k];
    const int c = cls[k];
    int rank = 0;
    for (int j = 0; j < S; ++j)
        if (j != k && gate_before(score[j], cls[j], j, s, c, k)) ++rank;
    order[rank] = k;
    out_cls[rank] = c;
    for (int e = 0; e < kEvFields; ++e) out_rec[rank * kEvFields + e] = rec[k * kEvFields + e];
}

// the evidence of n poses [n][12] against `frame`, through handle h's geometry (h->base) at its resolution
inline void launch_evidence(hipStream_t st, const rbs_handle* h, const rbs_find_gate& g, const float* frame, const double* poses, int n,
                            int* rec, int* cls)
{
    rbs::DevParams P = h->base;
    P.poses = poses;
    P.n = n;
    EvArgs E{};
    E.poses = poses;
    E.frame = frame;
    E.n = n;
    E.radius = g.radius;
    E.sigmas = g.sigmas;
    E.min_pixels = g.min_pixels;
    E.min_rim_pixels = g.min_rim_pixels;
    E.min_support_fraction = g.min_support_fraction;
    E.min_visible_fraction = g.min_visible_fraction;
    E.min_valid_fraction = g.min_valid_fraction;
    E.min_contour_fraction = g.min_contour_fraction;
    E.min_flush_fraction = g.min_flush_fraction;
    E.rec = rec;
    E.cls = cls;
    hipLaunchKernelGGL(rbs_findc_evidence_kernel, dim3((unsigned)n), dim3(rbs::kBlock), kEvSmemBytes, st, P, E);
}

inline void launch_gate_mask(hipStream_t st, const double* score, const int* cls, int want, long n, double* out)
{
    hipLaunchKernelGGL(rbs_findc_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, score, cls, want, n, out);
}

inline void launch_gate_merge(hipStream_t st, double* cand_s, long long* cand_i, const double* fill_s, const long long* fill_i, int nc)
{
    hipLaunchKernelGGL(rbs_findc_merge_kernel, dim3(1), dim3(kMaxCandidates), 0, st, cand_s, cand_i, fill_s, fill_i, nc);
}

inline void launch_gate_order(hipStream_t st, const double* score, const int* cls, const int* rec, int S, long long* order, int* out_cls,
                              int* out_rec)
{
    hipLaunchKernelGGL(rbs_findc_order_kernel, dim3(1), dim3(64), 0, st, score, cls, rec, S, order, out_cls, out_rec);
}

}  // namespace rbf

static_assert(sizeof(rbs_find_gate) == 72 && offsetof(rbs_find_gate, sigmas) == 24 && offsetof(rbs_find_gate, min_flush_fraction) == 64,
              "rbs_find_gate layout is mirrored by dbot_ros_amd/_capi.py");

// What a finder owns once the gate has been switched on: allocated then, freed by rbs_find_destroy.
struct rbs_find_gate_state {
    int* d_rec = nullptr;          // [max_seeds * n_rotations][10] step 4b's records, by hypothesis
    int* d_cls = nullptr;          // [max_seeds * n_rotations]
    double* d_masked = nullptr;    // [max_seeds * n_rotations] one class's scores, the others NaN
    int* d_srec = nullptr;         // [S][10] step 7's records by survivor, then [S][10] in the result's order
    int* d_scls = nullptr;         // [S] and [S] likewise
    std::vector<hipEvent_t> ev;    // a pair per batch of step 4b, then step 7's pair
};

namespace {

const char* gate_check(const rbs_find_gate* g)
{
    rbs_assess_params a;
    a.sigmas = g->sigmas;
    a.min_support_fraction = g->min_support_fraction;
    a.min_visible_fraction = g->min_visible_fraction;
    a.min_pixels = g->min_pixels;
    a.reserved = 0;
    if (const char* bad = assess::check_params(&a)) return bad;
    rbs_contour_params c;
    c.radius = g->radius;
    c.min_rim_pixels = g->min_rim_pixels;
    c.min_valid_fraction = g->min_valid_fraction;
    c.min_contour_fraction = g->min_contour_fraction;
    c.min_flush_fraction = g->min_flush_fraction;
    return contour::check_params(&c);
}

void gate_release(rbs_find* f)
{
    rbs_find_gate_state* g = f->gs;
    if (!g) return;
    for (void* q : {(void*)g->d_rec, (void*)g->d_cls, (void*)g->d_masked, (void*)g->d_srec, (void*)g->d_scls})
        if (q) (void)hipFree(q);
    for (hipEvent_t e : g->ev)
        if (e) (void)hipEventDestroy(e);
    delete g;
    f->gs = nullptr;
}

// events [first, first + count) exist
int32_t gate_events(rbs_find* f, size_t upto)
{
    rbs_find_gate_state* g = f->gs;
    while (g->ev.size() < upto) {
        hipEvent_t e = nullptr;
        RBF_HIP(f, hipEventCreate(&e));
        g->ev.push_back(e);
    }
    return RBS_OK;
}

// step 4b behind the scoring call of hypotheses [h0, h0 + nb): their poses lie in f->d_hyp.  batch_no: the call's number
int32_t gate_coarse(rbs_find* f, long h0, int nb, int batch_no)
{
    rbs_find_gate_state* g = f->gs;
    if (int32_t rc = gate_events(f, 2 * (size_t)batch_no + 2)) return rc;
    RBF_HIP(f, hipEventRecord(g->ev[2 * batch_no], f->st));
    rbf::launch_evidence(f->st, f->coarse, f->gt, f->d_coarse, f->d_hyp, nb, g->d_rec + (size_t)h0 * rbf::kEvFields, g->d_cls + h0);
    RBF_HIP(f, hipGetLastError());
    RBF_HIP(f, hipEventRecord(g->ev[2 * batch_no + 1], f->st));
    return RBS_OK;
}

// step 5's candidates in the gated order: d_cand_score / d_cand_idx [nc]
int32_t gate_select(rbs_find* f, int nc)
{
    rbs_find_gate_state* g = f->gs;
    hipStream_t st = f->st;
    const double* ts;
    const long long* ti;
    rbf::launch_gate_mask(st, f->d_score, g->d_cls, 0, f->n_hyp, g->d_masked);
    RBF_HIP(f, hipGetLastError());
    if (int32_t rc = find_topk(f, g->d_masked, nullptr, f->n_hyp, nc, &ts, &ti)) return rc;
    RBF_HIP(f, hipMemcpyAsync(f->d_cand_score, ts, sizeof(double) * nc, hipMemcpyDeviceToDevice, st));
    RBF_HIP(f, hipMemcpyAsync(f->d_cand_idx, ti, sizeof(long long) * nc, hipMemcpyDeviceToDevice, st));
    rbf::launch_gate_mask(st, f->d_score, g->d_cls, 1, f->n_hyp, g->d_masked);
    RBF_HIP(f, hipGetLastError());
    if (int32_t rc = find_topk(f, g->d_masked, nullptr, f->n_hyp, nc, &ts, &ti)) return rc;
    rbf::launch_gate_merge(st, f->d_cand_score, f->d_cand_idx, ts, ti, nc);
    RBF_HIP(f, hipGetLastError());
    return RBS_OK;
}

// step 7: the S survivors' evidence at the sensor's resolution and their order: d_final_idx [S]
int32_t gate_result(rbs_find* f, int S, int batches)
{
    rbs_find_gate_state* g = f->gs;
    hipStream_t st = f->st;
    const int nS = f->p.n_survivors;
    if (int32_t rc = gate_events(f, 2 * (size_t)batches + 2)) return rc;
    RBF_HIP(f, hipEventRecord(g->ev[2 * batches], st));
    rbf::launch_evidence(st, f->full, f->gt, f->d_full, f->d_surv, S, g->d_srec, g->d_scls);
    RBF_HIP(f, hipGetLastError());
    RBF_HIP(f, hipEventRecord(g->ev[2 * batches + 1], st));
    rbf::launch_gate_order(st, f->d_surv_score, g->d_scls, g->d_srec, S, f->d_final_idx, g->d_scls + nS, g->d_srec + (size_t)nS * rbf::kEvFields);
    RBF_HIP(f, hipGetLastError());
    return RBS_OK;
}

// after the find's last synchronisation: the two times
void gate_times(rbs_find* f, int batches, bool with_result)
{
    rbs_find_gate_state* g = f->gs;
    f->gms[0] = f->gms[1] = 0.f;
    for (int b = 0; b < batches; ++b) {
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, g->ev[2 * b], g->ev[2 * b + 1]);
        f->gms[0] += ms;
    }
    if (with_result) (void)hipEventElapsedTime(&f->gms[1], g->ev[2 * batches], g->ev[2 * batches + 1]);
}

// the class of pose 0 of the result (the find is synchronised)
int32_t gate_first_class(rbs_find* f, int* c0)
{
    RBF_HIP(f, hipMemcpy(c0, f->gs->d_scls + f->p.n_survivors, sizeof(int), hipMemcpyDeviceToHost));
    return RBS_OK;
}

}  // namespace

extern "C" {

void rbs_find_default_gate(rbs_find_gate* g)
{
    if (!g) return;
    rbs_assess_params a;
    rbs_contour_params c;
    rbs_assess_default_params(&a);
    rbs_contour_default_params(&c);
    g->enabled = 1;
    g->require_confirmed = 0;
    g->radius = c.radius;
    g->min_rim_pixels = c.min_rim_pixels;
    g->min_pixels = a.min_pixels;
    g->sigmas = a.sigmas;
    g->min_support_fraction = a.min_support_fraction;
    g->min_visible_fraction = a.min_visible_fraction;
    g->min_valid_fraction = c.min_valid_fraction;
    g->min_contour_fraction = c.min_contour_fraction;
    g->min_flush_fraction = c.min_flush_fraction;
}

int32_t rbs_find_set_gate(rbs_find* f, const rbs_find_gate* g)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (!g || g->enabled == 0) {
        f->gt.enabled = 0;
        return RBS_OK;
    }
    if (const char* bad = gate_check(g)) return ffail(f, RBS_ERR_INVALID_ARGUMENT, std::string("find gate: ") + bad);
    RBF_HIP(f, hipSetDevice(f->s->device));
    if (!f->gs) {
        rbs_find_gate_state* s = new (std::nothrow) rbs_find_gate_state;
        if (!s) return ffail(f, RBS_ERR_OUT_OF_MEMORY, "find_set_gate: out of host memory");
        const size_t H = (size_t)f->p.max_seeds * (size_t)f->p.n_rotations, S = (size_t)f->p.n_survivors;
        f->gs = s;
        if (hipMalloc(&s->d_rec, sizeof(int) * rbf::kEvFields * H) != hipSuccess || hipMalloc(&s->d_cls, sizeof(int) * H) != hipSuccess ||
            hipMalloc(&s->d_masked, sizeof(double) * H) != hipSuccess ||
            hipMalloc(&s->d_srec, sizeof(int) * rbf::kEvFields * 2 * S) != hipSuccess ||
            hipMalloc(&s->d_scls, sizeof(int) * 2 * S) != hipSuccess) {
            (void)hipGetLastError();
            gate_release(f);
            return ffail(f, RBS_ERR_OUT_OF_MEMORY, "find_set_gate: device memory");
        }
    }
    f->gt = *g;
    f->gt.enabled = 1;
    f->gt.require_confirmed = g->require_confirmed != 0;
    return RBS_OK;
}

int32_t rbs_find_get_evidence(rbs_find* f, int32_t stage, int32_t* records, int32_t* classes, int64_t* n)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (!n) return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_get_evidence: n is NULL");
    if (!f->have || !f->gt_ran) return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_get_evidence: no find with the gate yet");
    const rbs_find_gate_state* g = f->gs;
    RBF_HIP(f, hipSetDevice(f->s->device));
    const int S = f->n_surv, nS = f->p.n_survivors;
    const long long* d_idx = nullptr;
    long m = 0;
    switch (stage) {
        case RBS_FIND_COARSE:
            *n = f->n_hyp;
            if (records && f->n_hyp) RBF_HIP(f, hipMemcpy(records, g->d_rec, sizeof(int) * rbf::kEvFields * (size_t)f->n_hyp, hipMemcpyDeviceToHost));
            if (classes && f->n_hyp) RBF_HIP(f, hipMemcpy(classes, g->d_cls, sizeof(int) * (size_t)f->n_hyp, hipMemcpyDeviceToHost));
            return RBS_OK;
        case RBS_FIND_CANDIDATES: d_idx = f->d_cand_idx; m = f->n_cand; break;
        case RBS_FIND_SURVIVORS: d_idx = f->d_surv0_idx; m = S; break;
        case RBS_FIND_RESULT:
            *n = S;
            if (records && S) RBF_HIP(f, hipMemcpy(records, g->d_srec + (size_t)nS * rbf::kEvFields, sizeof(int) * rbf::kEvFields * (size_t)S, hipMemcpyDeviceToHost));
            if (classes && S) RBF_HIP(f, hipMemcpy(classes, g->d_scls + nS, sizeof(int) * (size_t)S, hipMemcpyDeviceToHost));
            return RBS_OK;
        default:
            return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_get_evidence: the stage is not COARSE, CANDIDATES, SURVIVORS or RESULT");
    }
    *n = m;   // step 4b's records of the stage's hypotheses, in the stage's order
    if (m == 0 || (!records && !classes)) return RBS_OK;
    std::vector<long long> idx((size_t)m);
    RBF_HIP(f, hipMemcpy(idx.data(), d_idx, sizeof(long long) * (size_t)m, hipMemcpyDeviceToHost));
    for (long i = 0; i < m; ++i) {
        if (records) RBF_HIP(f, hipMemcpy(records + (size_t)i * rbf::kEvFields, g->d_rec + (size_t)idx[i] * rbf::kEvFields, sizeof(int) * rbf::kEvFields, hipMemcpyDeviceToHost));
        if (classes) RBF_HIP(f, hipMemcpy(classes + i, g->d_cls + idx[i], sizeof(int), hipMemcpyDeviceToHost));
    }
    return RBS_OK;
}

int32_t rbs_find_gate_ms(rbs_find* f, float* out2)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (!out2 || !f->have || !f->gt_ran) return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_gate_ms: no find with the gate yet, or a null pointer");
    out2[0] = f->gms[0];
    out2[1] = f->gms[1];
    return RBS_OK;
}

}  // extern "C"
