// rbsensor_gauss.hip -- the robust Gaussian tracker (rbs_gauss_*, include/rbsensor_mi355x.h; the arithmetic:
// DESIGN.md Appendix G).  Included at the end of rbsensor_capi.hip: it uses the handle, its frame staging
// and the rasterizer of rbsensor_kernels.hip.
//
// Per frame, on the sensor's stream:
//   rbs_gauss_render_kernel   one block row per distinct sigma pose (1 + 12 B of them), the pose's screen
//                             rectangle cut into 64 x 64 tiles dealt to the row's blocks; every tile goes
//                             through raster_window exactly as rbs_render_kernel's (depths bit-identical to
//                             the oracle's orc_render).  Plane k is valid inside rect k only.
//   rbs_gauss_moments_kernel  per pixel of the union rectangle with a finite observation: y_hat, P, h, R, the
//                             robust body weight b and pi = b / R; a block stages 256 pixels' (pi, residual, h)
//                             in LDS and thread e accumulates entry e of {Lambda - I (upper triangle), eta} over
//                             them in pixel order.  Fixed grid -> per-block partials.
//   rbs_gauss_reduce_kernel   entry e summed over the partials in block order.
// Every sum has a fixed order: the same inputs give the same bits, run after run.  The host does the D x D
// algebra in binary64 (D = 12 B <= 36) with one synchronisation per frame.
namespace rbs {

constexpr int kGaussMaxBodies = 3;        // 6B(6B+1)/2 + 6B <= 256 entries: one per thread of the moments block
constexpr int kGaussBlocks = 256;         // moments grid: fixed, so the reduction order is too
constexpr int kGaussTileW = 64, kGaussTilePx = 4096;   // render tiles: small, so that a pose's rectangle spreads over blocks
constexpr int kGaussRenderSplit = 32;     // blocks per sigma pose (tiles beyond it: strided)

__global__ __launch_bounds__(kBlock) void rbs_gauss_render_kernel(const DevParams P, float* __restrict__ planes, int4* __restrict__ rects)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Smem m = carve(smem, P.tile_px, false);
    const int k = blockIdx.x;
    const double* pose = P.poses + (size_t)k * 12 * P.n_bodies;
    const Rect r = particle_rect(P, pose);
    if (blockIdx.y == 0 && threadIdx.x == 0) rects[k] = make_int4(r.x0, r.y0, r.x1, r.y1);
    if (r.x1 <= r.x0) return;
    const TileGrid tg = tile_grid(r.x1 - r.x0, r.y1 - r.y0, P.tile_w, min(P.tile_w * P.tile_h, P.tile_px));
    const int nx = (r.x1 - r.x0 + tg.tw - 1) / tg.tw, ny = (r.y1 - r.y0 + tg.th - 1) / tg.th;
    float* out = planes + (size_t)k * P.npx;
    for (int t = blockIdx.y; t < nx * ny; t += gridDim.y) {
        const int ty = t / nx;
        const int wx0 = r.x0 + (t - ty * nx) * tg.tw, wy0 = r.y0 + ty * tg.th;
        const int wx1 = min(r.x1, wx0 + tg.tw), wy1 = min(r.y1, wy0 + tg.th);
        const int tw = wx1 - wx0, npx = tw * (wy1 - wy0);
        raster_window(P, pose, wx0, wy0, wx1, wy1, true, m.tile, m.big, m.nbig,
                      m.evalq + (threadIdx.x >> 6) * kQPlanes * kEvalQueue, 0xffffffffu);
        for (int p = threadIdx.x; p < npx; p += kBlock) {
            const int lr = p / tw;
            out[(size_t)(wy0 + lr) * P.cols + wx0 + (p - lr * tw)] = __uint_as_float(m.tile[p]);
        }
        __syncthreads();
    }
}

struct GaussArgs {
    const float* planes;      // [nd][npx], plane k valid inside rects[k]
    const int4* rects;        // [nd]
    const float* frame;       // the observation
    int cols, npx;
    double wm0, wc0, w;       // unscented weights: centre (mean, covariance), every other point
    double inv2sqrtc;         // 1 / (2 sqrt(c))
    double bg_depth, fg2, bg2;
    int robust;               // tail_weight > 0
    double log_tail;          // log(w u) - log(1 - w), u = 1 / (tail_max - tail_min)
    double tail_min, tail_max;
    double* partials;         // [gridDim.x][NE]
};

template <int NB>
__global__ __launch_bounds__(256) void rbs_gauss_moments_kernel(const GaussArgs A)
{
    constexpr int NP = 6 * NB, ND = 1 + 2 * NP, NL = NP * (NP + 1) / 2, NE = NL + NP;
    static_assert(NE <= 256, "one Lambda / eta entry per thread");
    constexpr int kRow = 257;                 // (padded: the threads of a wave read different rows at one pixel)
    __shared__ double s_h[NP * kRow];
    __shared__ double s_pi[256], s_r[256];
    __shared__ int4 s_rect[ND];
    const int tid = threadIdx.x;
    if (tid < ND) s_rect[tid] = A.rects[tid];
    __syncthreads();
    int ux0 = 1 << 30, uy0 = 1 << 30, ux1 = 0, uy1 = 0;
    for (int k = 0; k < ND; ++k) {
        const int4 r = s_rect[k];
        if (r.z <= r.x || r.w <= r.y) continue;
        ux0 = min(ux0, r.x); uy0 = min(uy0, r.y); ux1 = max(ux1, r.z); uy1 = max(uy1, r.w);
    }
    const int uw = max(0, ux1 - ux0), n_u = uw * max(0, uy1 - uy0);
    // this thread's entry: (a, b), a <= b, of the upper triangle, or eta_a
    int ea = 0, eb = -1;
    if (tid < NL) {
        int rem = tid;
        while (rem >= NP - ea) { rem -= NP - ea; ++ea; }
        eb = ea + rem;
    } else if (tid < NE) {
        ea = tid - NL;
    }
    double acc = 0.0;
    constexpr double kExtra = 2.0 * NP;       // the velocity columns' 2 x 6B sigma points: copies of the centre
    for (int base = blockIdx.x * 256; base < n_u; base += gridDim.x * 256) {
        const int q = base + tid;
        double pi = 0.0, res = 0.0, h[NP];
#pragma unroll
        for (int j = 0; j < NP; ++j) h[j] = 0.0;
        if (q < n_u) {
            const int row = uy0 + q / uw, col = ux0 + q % uw;
            const int i = row * A.cols + col;
            const float yf = A.frame[i];
            if (isfinite(yf)) {
                double m[ND];
                bool cov[ND];
#pragma unroll
                for (int k = 0; k < ND; ++k) {
                    const int4 r = s_rect[k];
                    const float d = (col >= r.x && col < r.z && row >= r.y && row < r.w) ? A.planes[(size_t)k * A.npx + i] : INFINITY;
                    cov[k] = d < INFINITY;
                    m[k] = cov[k] ? (double)d : A.bg_depth;
                }
                double sm = 0.0, ss = 0.0;
#pragma unroll
                for (int k = 1; k < ND; ++k) { sm += m[k]; ss += cov[k] ? A.fg2 : A.bg2; }
                const double s0 = cov[0] ? A.fg2 : A.bg2;
                const double yhat = A.wm0 * m[0] + A.w * (sm + kExtra * m[0]);
                double sq = 0.0;
#pragma unroll
                for (int k = 1; k < ND; ++k) sq += (m[k] - yhat) * (m[k] - yhat);
                const double d0 = m[0] - yhat;
                double Pv = A.wc0 * (d0 * d0) + A.w * (sq + kExtra * (d0 * d0)) + (A.wm0 * s0 + A.w * (ss + kExtra * s0));
                Pv = fmax(Pv, A.fg2);
                double hh = 0.0;
#pragma unroll
                for (int j = 0; j < NP; ++j) { h[j] = (m[1 + 2 * j] - m[2 + 2 * j]) * A.inv2sqrtc; hh += h[j] * h[j]; }
                const double R = fmax(Pv - hh, A.fg2);
                const double y = (double)yf;
                res = y - yhat;
                double b = 1.0;
                if (A.robust && y >= A.tail_min && y <= A.tail_max) {
                    const double lg = -0.5 * log(6.283185307179586 * Pv) - 0.5 * (res * res) / Pv;
                    b = 1.0 / (1.0 + exp(A.log_tail - lg));   // (exp overflows to inf: b = 0)
                }
                pi = b / R;
            }
        }
        s_pi[tid] = pi;
        s_r[tid] = res;
#pragma unroll
        for (int j = 0; j < NP; ++j) s_h[j * kRow + tid] = h[j];
        __syncthreads();
        if (tid < NE) {
            const double* ha = s_h + ea * kRow;
            const double* hb = eb >= 0 ? s_h + eb * kRow : s_r;
            for (int p = 0; p < 256; ++p) acc += (s_pi[p] * ha[p]) * hb[p];
        }
        __syncthreads();
    }
    if (tid < NE) A.partials[(size_t)blockIdx.x * NE + tid] = acc;
}

__global__ __launch_bounds__(256) void rbs_gauss_reduce_kernel(const double* __restrict__ partials, int nblocks, int ne, double* __restrict__ out)
{
    const int e = threadIdx.x;
    if (e >= ne) return;
    // kU loads in flight, then added in block order (one dependent load per trip measured 0.064 ms: its latency x 256)
    constexpr int kU = 32;
    double s = 0.0;
    for (int b0 = 0; b0 < nblocks; b0 += kU) {
        double v[kU];
#pragma unroll
        for (int u = 0; u < kU; ++u) v[u] = b0 + u < nblocks ? partials[(size_t)(b0 + u) * ne + e] : 0.0;
#pragma unroll
        for (int u = 0; u < kU; ++u)
            if (b0 + u < nblocks) s += v[u];
    }
    out[e] = s;
}

}  // namespace rbs

struct rbs_gauss {
    rbs_handle* s = nullptr;
    rbs_gauss_params p{};
    int B = 0, D = 0, NP = 0, nd = 0, NE = 0;
    double c = 0, sqrtc = 0, wm0 = 0, wc0 = 0, w = 0;
    bool initialized = false, tracked = false;
    std::vector<double> z, mu, cov;                      // belief: default state, mean delta, covariance (state order)
    std::vector<double> z_prior, mu_prior, cov_prior;    // the last frame's prior
    std::vector<double> sigma;                           // [nd][B][12] the last frame's sigma poses
    std::vector<int> perm;                               // state index -> pose-first index
    float* d_planes = nullptr;
    int4* d_rects = nullptr;
    double* d_poses = nullptr;
    double* d_partials = nullptr;
    double* d_out = nullptr;
    double* h_poses = nullptr;                           // pinned
    double* h_out = nullptr;                             // pinned
    hipEvent_t ev[4] = {};
    float ms[3] = {};
};

namespace {
namespace gauss {

// pose.py's rotvec_to_matrix (angle-axis through the unit quaternion)
void rotvec_to_matrix(const double* rv, double* R)
{
    const double angle = std::sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
    const double k = angle < 1e-9 ? 0.5 - angle * angle / 48.0 : std::sin(0.5 * angle) / angle;
    const double w = std::cos(0.5 * angle), x = rv[0] * k, y = rv[1] * k, z = rv[2] * k;
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// pose.py's matrix_to_rotvec (atan2 form; the axis from the symmetric part near pi)
void matrix_to_rotvec(const double* R, double* rv)
{
    const double s[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
    const double sn = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
    const double cs = 0.5 * (R[0] + R[4] + R[8] - 1.0);
    const double angle = std::atan2(sn, cs);
    if (sn > 1e-8) { for (int i = 0; i < 3; ++i) rv[i] = s[i] * (angle / sn); return; }
    if (cs > 0.0) { for (int i = 0; i < 3; ++i) rv[i] = s[i]; return; }
    double d[3];
    int im = 0;
    for (int i = 0; i < 3; ++i) {
        d[i] = std::sqrt(std::max((R[4 * i] + 1.0) * 0.5, 0.0));
        if (d[i] > d[im]) im = i;
    }
    double axis[3];
    for (int i = 0; i < 3; ++i) axis[i] = (R[3 * i + im] + (i == im ? 1.0 : 0.0)) / (2.0 * d[im]);
    const double n = std::sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
    for (int i = 0; i < 3; ++i) rv[i] = axis[i] / n * angle;
}

void matmul3(const double* A, const double* B, double* C)
{
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}

// Lower Cholesky factor of the symmetric n x n A (its lower triangle is read); false: not positive definite.
bool cholesky(const double* A, double* L, int n)
{
    std::fill(L, L + (size_t)n * n, 0.0);
    for (int j = 0; j < n; ++j) {
        double d = A[(size_t)j * n + j];
        for (int k = 0; k < j; ++k) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
        if (!(d > 0.0) || !std::isfinite(d)) return false;
        const double ljj = std::sqrt(d);
        L[(size_t)j * n + j] = ljj;
        for (int i = j + 1; i < n; ++i) {
            double v = A[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) v -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
            L[(size_t)i * n + j] = v / ljj;
        }
    }
    return true;
}

// x := (L L^T)^-1 x
void chol_solve(const double* L, int n, double* x)
{
    for (int i = 0; i < n; ++i) {
        double v = x[i];
        for (int k = 0; k < i; ++k) v -= L[(size_t)i * n + k] * x[k];
        x[i] = v / L[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double v = x[i];
        for (int k = i + 1; k < n; ++k) v -= L[(size_t)k * n + i] * x[k];
        x[i] = v / L[(size_t)i * n + i];
    }
}

void symmetrize(double* A, int n)
{
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j) {
            const double v = 0.5 * (A[(size_t)i * n + j] + A[(size_t)j * n + i]);
            A[(size_t)i * n + j] = A[(size_t)j * n + i] = v;
        }
}

int32_t gfail(rbs_gauss* g, int32_t rc, const std::string& msg) { return fail(g->s, rc, msg); }

const char* check_params(const rbs_gauss_params* p)
{
    for (int i = 0; i < 3; ++i)
        if (!(p->linear_sigma[i] >= 0.0) || !(p->angular_sigma[i] >= 0.0) || !std::isfinite(p->linear_sigma[i]) ||
            !std::isfinite(p->angular_sigma[i]))
            return "gauss_create: object_transition sigmas must be finite and >= 0";
    if (!std::isfinite(p->velocity_factor)) return "gauss_create: velocity_factor must be finite";
    if (!(p->ut_alpha > 0.0) || !std::isfinite(p->ut_alpha)) return "gauss_create: unscented_transform/alpha must be > 0";
    if (!(p->fg_noise_std > 0.0) || !std::isfinite(p->fg_noise_std)) return "gauss_create: fg_noise_std must be > 0";
    if (!(p->bg_noise_std >= 0.0) || !std::isfinite(p->bg_noise_std) || !std::isfinite(p->bg_depth))
        return "gauss_create: bg_depth must be finite and bg_noise_std >= 0";
    if (!(p->tail_weight >= 0.0 && p->tail_weight < 1.0)) return "gauss_create: tail_weight must lie in [0, 1)";
    if (!std::isfinite(p->uniform_tail_min) || !std::isfinite(p->uniform_tail_max) || !(p->uniform_tail_max > p->uniform_tail_min))
        return "gauss_create: uniform_tail_max must exceed uniform_tail_min";
    return nullptr;
}

// One frame: predict, sigma poses, the three kernels, the update in the whitened space, re-centring.
int32_t track_impl(rbs_gauss* g, const float* f32, const double* f64, double* out_state, double* out_cov)
{
    rbs_handle* h = g->s;
    if (!out_state) return gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_track: out_state is NULL");
    if (!g->initialized) return gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_track: rbs_gauss_initialize first");
    if (!h->shards.empty() || h->group || h->peer_world > 1)
        return gfail(g, RBS_ERR_UNSUPPORTED, "gauss_track: single-device handles only");
    RBS_REFUSE_POISONED(h);
    RBS_HIP(h, hipSetDevice(h->device));
    const size_t npx = (size_t)h->npx;
    if (f32) { if (int32_t rc = rbs_set_observation_f32(h, f32, npx)) return rc; }
    else if (f64) { if (int32_t rc = rbs_set_observation(h, f64, npx)) return rc; }
    if (int32_t rc = stage_borrowed(h)) return rc;
    if (int32_t rc = flush_lazy_frame(h, h->stream)) return rc;
    if (h->frame_wait >= 0) RBS_HIP(h, hipStreamWaitEvent(h->stream, h->ev_frame[h->frame_wait], 0));
    h->quiet = false;

    const int B = g->B, D = g->D, NP = g->NP, nd = g->nd;
    // ---- predict (state order): per body pose' = pose + vf vel, vel' = vf vel; Q = [[S, S], [S, S]]
    const double vf = g->p.velocity_factor;
    std::vector<double> A((size_t)D * D, 0.0), Q((size_t)D * D, 0.0);
    for (int b = 0; b < B; ++b)
        for (int d = 0; d < 6; ++d) {
            const int ip = 12 * b + d, iv = ip + 6;
            A[(size_t)ip * D + ip] = 1.0;
            A[(size_t)ip * D + iv] = vf;
            A[(size_t)iv * D + iv] = vf;
            const double sg = d < 3 ? g->p.linear_sigma[d] : g->p.angular_sigma[d - 3];
            Q[(size_t)ip * D + ip] = Q[(size_t)ip * D + iv] = Q[(size_t)iv * D + ip] = Q[(size_t)iv * D + iv] = sg * sg;
        }
    std::vector<double> mum(D, 0.0), AS((size_t)D * D, 0.0), Sm((size_t)D * D, 0.0);
    for (int i = 0; i < D; ++i)
        for (int k = 0; k < D; ++k) mum[i] += A[(size_t)i * D + k] * g->mu[k];
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) {
            double v = 0.0;
            for (int k = 0; k < D; ++k) v += A[(size_t)i * D + k] * g->cov[(size_t)k * D + j];
            AS[(size_t)i * D + j] = v;
        }
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) {
            double v = 0.0;
            for (int k = 0; k < D; ++k) v += AS[(size_t)i * D + k] * A[(size_t)j * D + k];
            Sm[(size_t)i * D + j] = v + Q[(size_t)i * D + j];
        }
    symmetrize(Sm.data(), D);
    g->z_prior = g->z;
    g->mu_prior = mum;
    g->cov_prior = Sm;
    // ---- sigma points in pose-first order
    std::vector<double> mpf(D), Spf((size_t)D * D), L((size_t)D * D);
    for (int i = 0; i < D; ++i) {
        mpf[g->perm[i]] = mum[i];
        for (int j = 0; j < D; ++j) Spf[(size_t)g->perm[i] * D + g->perm[j]] = Sm[(size_t)i * D + j];
    }
    if (!cholesky(Spf.data(), L.data(), D))
        return gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_track: the predicted covariance is not positive definite");
    double Rz[rbs::kGaussMaxBodies][9];
    for (int b = 0; b < B; ++b) rotvec_to_matrix(g->z.data() + 12 * b + 3, Rz[b]);
    for (int k = 0; k < nd; ++k) {
        const int j = (k - 1) / 2;
        const double sc = k == 0 ? 0.0 : ((k - 1) % 2 == 0 ? g->sqrtc : -g->sqrtc);
        for (int b = 0; b < B; ++b) {
            double x[6], Rd[9];
            for (int d = 0; d < 6; ++d) x[d] = mpf[6 * b + d] + (k == 0 ? 0.0 : sc * L[(size_t)(6 * b + d) * D + j]);
            rotvec_to_matrix(x + 3, Rd);
            double* out = g->sigma.data() + ((size_t)k * B + b) * 12;
            matmul3(Rd, Rz[b], out);
            for (int d = 0; d < 3; ++d) out[9 + d] = g->z[12 * b + d] + x[d];
        }
    }
    std::memcpy(g->h_poses, g->sigma.data(), sizeof(double) * g->sigma.size());
    // ---- device: render, moments, reduction
    hipStream_t s = h->stream;
    RBS_HIP(h, hipMemcpyAsync(g->d_poses, g->h_poses, sizeof(double) * g->sigma.size(), hipMemcpyHostToDevice, s));
    DevParams P = h->base;
    P.poses = g->d_poses;
    P.n = nd;
    P.tile_w = rbs::kGaussTileW;
    P.tile_px = rbs::kGaussTilePx;
    P.tile_h = rbs::kGaussTilePx / rbs::kGaussTileW;
    RBS_HIP(h, hipEventRecord(g->ev[0], s));
    hipLaunchKernelGGL(rbs::rbs_gauss_render_kernel, dim3((unsigned)nd, rbs::kGaussRenderSplit), dim3(rbs::kBlock),
                       rbs::smem_bytes(rbs::kGaussTilePx, false), s, P, g->d_planes, g->d_rects);
    RBS_HIP(h, hipGetLastError());
    RBS_HIP(h, hipEventRecord(g->ev[1], s));
    rbs::GaussArgs G{};
    G.planes = g->d_planes;
    G.rects = g->d_rects;
    G.frame = h->cur_frame;
    G.cols = h->cols;
    G.npx = h->npx;
    G.wm0 = g->wm0; G.wc0 = g->wc0; G.w = g->w;
    G.inv2sqrtc = 1.0 / (2.0 * g->sqrtc);
    G.bg_depth = g->p.bg_depth;
    G.fg2 = g->p.fg_noise_std * g->p.fg_noise_std;
    G.bg2 = g->p.bg_noise_std * g->p.bg_noise_std;
    G.robust = g->p.tail_weight > 0.0;
    G.log_tail = std::log(g->p.tail_weight / (g->p.uniform_tail_max - g->p.uniform_tail_min)) - std::log(1.0 - g->p.tail_weight);
    G.tail_min = g->p.uniform_tail_min;
    G.tail_max = g->p.uniform_tail_max;
    G.partials = g->d_partials;
    switch (B) {
    case 1: hipLaunchKernelGGL(rbs::rbs_gauss_moments_kernel<1>, dim3(rbs::kGaussBlocks), dim3(256), 0, s, G); break;
    case 2: hipLaunchKernelGGL(rbs::rbs_gauss_moments_kernel<2>, dim3(rbs::kGaussBlocks), dim3(256), 0, s, G); break;
    default: hipLaunchKernelGGL(rbs::rbs_gauss_moments_kernel<3>, dim3(rbs::kGaussBlocks), dim3(256), 0, s, G); break;
    }
    RBS_HIP(h, hipGetLastError());
    RBS_HIP(h, hipEventRecord(g->ev[2], s));
    hipLaunchKernelGGL(rbs::rbs_gauss_reduce_kernel, dim3(1), dim3(256), 0, s, (const double*)g->d_partials, rbs::kGaussBlocks, g->NE, g->d_out);
    RBS_HIP(h, hipGetLastError());
    RBS_HIP(h, hipEventRecord(g->ev[3], s));
    RBS_HIP(h, hipMemcpyAsync(g->h_out, g->d_out, sizeof(double) * g->NE, hipMemcpyDeviceToHost, s));
    RBS_HIP(h, hipStreamSynchronize(s));
    h->quiet = true;
    for (int k = 0; k < 3; ++k) RBS_HIP(h, hipEventElapsedTime(&g->ms[k], g->ev[k], g->ev[k + 1]));
    g->tracked = true;
    // ---- update in the whitened space: Lambda = I + sum pi h h^T (pose block), eta = sum pi h r
    std::vector<double> Lam((size_t)NP * NP), M((size_t)NP * NP), zeta(NP), Linv((size_t)NP * NP);
    int e = 0;
    for (int a = 0; a < NP; ++a)
        for (int b = a; b < NP; ++b, ++e) Lam[(size_t)a * NP + b] = Lam[(size_t)b * NP + a] = g->h_out[e] + (a == b ? 1.0 : 0.0);
    for (int a = 0; a < NP; ++a) zeta[a] = g->h_out[e + a];
    if (!cholesky(Lam.data(), M.data(), NP))
        return gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_track: the information matrix is not finite (the frame?)");
    chol_solve(M.data(), NP, zeta.data());
    for (int col = 0; col < NP; ++col) {
        std::vector<double> x(NP, 0.0);
        x[col] = 1.0;
        chol_solve(M.data(), NP, x.data());
        for (int r = 0; r < NP; ++r) Linv[(size_t)r * NP + col] = x[r];
    }
    std::vector<double> mup(mpf), T((size_t)D * D, 0.0), Spp((size_t)D * D, 0.0);
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < NP; ++j) mup[i] += L[(size_t)i * D + j] * zeta[j];
    for (int i = 0; i < D; ++i)   // T = L blockdiag(Lambda^-1, I)
        for (int j = 0; j < D; ++j) {
            if (j >= NP) { T[(size_t)i * D + j] = L[(size_t)i * D + j]; continue; }
            double v = 0.0;
            for (int k = 0; k < NP; ++k) v += L[(size_t)i * D + k] * Linv[(size_t)k * NP + j];
            T[(size_t)i * D + j] = v;
        }
    for (int i = 0; i < D; ++i)
        for (int j = 0; j < D; ++j) {
            double v = 0.0;
            for (int k = 0; k < D; ++k) v += T[(size_t)i * D + k] * L[(size_t)j * D + k];
            Spp[(size_t)i * D + j] = v;
        }
    symmetrize(Spp.data(), D);
    for (int i = 0; i < D; ++i) {
        g->mu[i] = mup[g->perm[i]];
        for (int j = 0; j < D; ++j) g->cov[(size_t)i * D + j] = Spp[(size_t)g->perm[i] * D + g->perm[j]];
    }
    // ---- re-centre: the mean's pose folds into z (ParticleTracker.track's rule), z's velocities := the mean's
    for (int b = 0; b < B; ++b) {
        double* zb = g->z.data() + 12 * b;
        double* mb = g->mu.data() + 12 * b;
        double Rm[9], Rn[9];
        rotvec_to_matrix(mb + 3, Rm);
        matmul3(Rm, Rz[b], Rn);
        for (int d = 0; d < 3; ++d) zb[d] += mb[d];
        matrix_to_rotvec(Rn, zb + 3);
        for (int d = 6; d < 12; ++d) zb[d] = mb[d];
        for (int d = 0; d < 6; ++d) mb[d] = 0.0;
    }
    std::memcpy(out_state, g->z.data(), sizeof(double) * D);
    if (out_cov) std::memcpy(out_cov, g->cov.data(), sizeof(double) * D * D);
    return RBS_OK;
}

}  // namespace gauss
}  // namespace

extern "C" {

void rbs_gauss_destroy(rbs_gauss* g)
{
    if (!g) return;
    (void)hipSetDevice(g->s->device);
    (void)hipStreamSynchronize(g->s->stream);
    for (void* p : {(void*)g->d_planes, (void*)g->d_rects, (void*)g->d_poses, (void*)g->d_partials, (void*)g->d_out})
        if (p) (void)hipFree(p);
    if (g->h_poses) (void)hipHostFree(g->h_poses);
    if (g->h_out) (void)hipHostFree(g->h_out);
    for (hipEvent_t& e : g->ev)
        if (e) (void)hipEventDestroy(e);
    delete g;
}

int32_t rbs_gauss_create(rbs_handle* sensor, const rbs_gauss_params* p, rbs_gauss** out)
{
    if (out) *out = nullptr;
    const char* bad = !p ? "gauss_create: params is NULL" : !out ? "gauss_create: out is NULL" : gauss::check_params(p);
    if (!bad && !sensor) bad = "gauss_create: sensor is NULL";
    if (bad) {
        if (sensor) sensor->err = bad; else g_create_error = bad;
        return RBS_ERR_INVALID_ARGUMENT;
    }
    if (!sensor->shards.empty() || sensor->group || sensor->peer_world > 1)
        return fail(sensor, RBS_ERR_UNSUPPORTED, "gauss_create: the Gaussian tracker runs on single-device handles only");
    if (sensor->n_bodies > rbs::kGaussMaxBodies)
        return fail(sensor, RBS_ERR_UNSUPPORTED, fmt("gauss_create: at most %d objects", rbs::kGaussMaxBodies));
    rbs_gauss* g = new (std::nothrow) rbs_gauss;
    if (!g) return fail(sensor, RBS_ERR_OUT_OF_MEMORY, "gauss_create: out of host memory");
    g->s = sensor;
    g->p = *p;
    g->B = sensor->n_bodies;
    g->D = 12 * g->B;
    g->NP = 6 * g->B;
    g->nd = 1 + 2 * g->NP;
    g->NE = g->NP * (g->NP + 1) / 2 + g->NP;
    const double a2 = p->ut_alpha * p->ut_alpha;
    g->c = a2 * g->D;
    g->sqrtc = std::sqrt(g->c);
    g->wm0 = 1.0 - 1.0 / a2;
    g->wc0 = g->wm0 + 1.0 - a2 + 2.0;
    g->w = 1.0 / (2.0 * g->c);
    g->z.assign(g->D, 0.0);
    g->mu.assign(g->D, 0.0);
    g->cov.assign((size_t)g->D * g->D, 0.0);
    g->sigma.assign((size_t)g->nd * g->B * 12, 0.0);
    g->perm.resize(g->D);
    for (int b = 0; b < g->B; ++b)
        for (int d = 0; d < 12; ++d) g->perm[12 * b + d] = d < 6 ? 6 * b + d : g->NP + 6 * b + (d - 6);
    rbs_handle* h = sensor;
    auto cleanup = [&](int32_t rc) { rbs_gauss_destroy(g); return rc; };
    if (hipSetDevice(h->device) != hipSuccess ||
        hipMalloc(&g->d_planes, sizeof(float) * (size_t)g->nd * h->npx) != hipSuccess ||
        hipMalloc(&g->d_rects, sizeof(int4) * g->nd) != hipSuccess ||
        hipMalloc(&g->d_poses, sizeof(double) * g->sigma.size()) != hipSuccess ||
        hipMalloc(&g->d_partials, sizeof(double) * (size_t)rbs::kGaussBlocks * g->NE) != hipSuccess ||
        hipMalloc(&g->d_out, sizeof(double) * g->NE) != hipSuccess ||
        hipHostMalloc(&g->h_poses, sizeof(double) * g->sigma.size(), hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(&g->h_out, sizeof(double) * g->NE, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        fail(h, RBS_ERR_OUT_OF_MEMORY, "gauss_create: device or pinned memory");
        return cleanup(RBS_ERR_OUT_OF_MEMORY);
    }
    for (hipEvent_t& e : g->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            (void)hipGetLastError();
            fail(h, RBS_ERR_HIP, "gauss_create: hipEventCreate failed");
            return cleanup(RBS_ERR_HIP);
        }
    *out = g;
    return RBS_OK;
}

int32_t rbs_gauss_initialize(rbs_gauss* g, const double* default_state, const double* cov0)
{
    if (!g) return RBS_ERR_INVALID_ARGUMENT;
    if (!default_state) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_initialize: null state");
    const int D = g->D;
    std::vector<double> c((size_t)D * D, 0.0), Lc((size_t)D * D);
    if (cov0) {
        std::memcpy(c.data(), cov0, sizeof(double) * c.size());
        gauss::symmetrize(c.data(), D);
    } else {
        for (int b = 0; b < g->B; ++b)
            for (int d = 0; d < 12; ++d) {
                const double sg = (d % 6) < 3 ? g->p.linear_sigma[d % 3] : g->p.angular_sigma[d % 3];
                c[(size_t)(12 * b + d) * D + 12 * b + d] = sg * sg;
            }
    }
    for (int i = 0; i < D; ++i)
        if (!std::isfinite(default_state[i])) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_initialize: state not finite");
    g->z.assign(default_state, default_state + D);
    g->mu.assign(D, 0.0);
    g->cov = c;
    g->initialized = true;
    g->tracked = false;
    return RBS_OK;
}

int32_t rbs_gauss_track(rbs_gauss* g, const float* frame, double* out_state, double* out_cov)
{
    if (!g) return RBS_ERR_INVALID_ARGUMENT;
    return gauss::track_impl(g, frame, nullptr, out_state, out_cov);
}

int32_t rbs_gauss_track_f64(rbs_gauss* g, const double* frame, double* out_state, double* out_cov)
{
    if (!g) return RBS_ERR_INVALID_ARGUMENT;
    return gauss::track_impl(g, nullptr, frame, out_state, out_cov);
}

int32_t rbs_gauss_get_prior(rbs_gauss* g, double* default_state, double* mean, double* cov)
{
    if (!g) return RBS_ERR_INVALID_ARGUMENT;
    if (!g->tracked) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_get_prior: no frame tracked yet");
    if (default_state) std::memcpy(default_state, g->z_prior.data(), sizeof(double) * g->D);
    if (mean) std::memcpy(mean, g->mu_prior.data(), sizeof(double) * g->D);
    if (cov) std::memcpy(cov, g->cov_prior.data(), sizeof(double) * g->D * g->D);
    return RBS_OK;
}

int32_t rbs_gauss_get_sigma_poses(rbs_gauss* g, double* out, int32_t* n)
{
    if (!g) return RBS_ERR_INVALID_ARGUMENT;
    if (n) *n = g->nd;
    if (!out) return RBS_OK;
    if (!g->tracked) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_get_sigma_poses: no frame tracked yet");
    std::memcpy(out, g->sigma.data(), sizeof(double) * g->sigma.size());
    return RBS_OK;
}

int32_t rbs_gauss_get_render(rbs_gauss* g, int32_t k, float* out)
{
    if (!g) return RBS_ERR_INVALID_ARGUMENT;
    rbs_handle* h = g->s;
    if (!out || k < 0 || k >= g->nd) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_get_render: bad index or null pointer");
    if (!g->tracked) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_get_render: no frame tracked yet");
    RBS_HIP(h, hipSetDevice(h->device));
    RBS_HIP(h, hipStreamSynchronize(h->stream));
    int4 r;
    RBS_HIP(h, hipMemcpy(&r, g->d_rects + k, sizeof(int4), hipMemcpyDeviceToHost));
    RBS_HIP(h, hipMemcpy(out, g->d_planes + (size_t)k * h->npx, sizeof(float) * h->npx, hipMemcpyDeviceToHost));
    for (int row = 0; row < h->rows; ++row)   // the plane is valid inside its rectangle only
        for (int col = 0; col < h->cols; ++col)
            if (!(col >= r.x && col < r.z && row >= r.y && row < r.w)) out[(size_t)row * h->cols + col] = INFINITY;
    return RBS_OK;
}

int32_t rbs_gauss_get_moments(rbs_gauss* g, double* out, int32_t* n)
{
    if (!g) return RBS_ERR_INVALID_ARGUMENT;
    if (!out || !n) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_get_moments: null pointer");
    if (!g->tracked) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_get_moments: no frame tracked yet");
    *n = g->NE;
    std::memcpy(out, g->h_out, sizeof(double) * g->NE);   // (track_impl synchronised before it read them)
    return RBS_OK;
}

int32_t rbs_gauss_kernel_ms(rbs_gauss* g, float* out3)
{
    if (!g) return RBS_ERR_INVALID_ARGUMENT;
    if (!out3) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_kernel_ms: null pointer");
    if (!g->tracked) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_kernel_ms: no frame tracked yet");
    for (int k = 0; k < 3; ++k) out3[k] = g->ms[k];
    return RBS_OK;
}

}  // extern "C"
