// rbsensor_gauss.hip -- the robust Gaussian tracker (rbs_gauss_*, include/rbsensor_mi355x.h; the arithmetic:
// DESIGN.md Appendix G).  Included at the end of rbsensor_capi.hip: it uses the handle, its frame staging
// and the rasterizer of rbsensor_kernels.hip.
//
// Per frame, on the sensor's stream:
//   rbs_planes_render_kernel<false>  (rbs_pose_planes.h) one plane per distinct sigma pose (1 + 12 B of them):
//                             all bodies, z-min, in the pose's screen rectangle; depths bit-identical to the
//                             oracle's orc_render.  Plane k is valid inside rect k only.
//   rbs_gauss_moments_kernel  per pixel of the union rectangle with a finite observation: y_hat, P, h, R, the
//                             robust body weight b and pi = b / R; a block stages 256 pixels' (pi, residual, h)
//                             in LDS and thread e accumulates entry e of {Lambda - I (upper triangle), eta} over
//                             them in pixel order.  Fixed grid -> per-block partials.
//   rbs_gauss_reduce_kernel   entry e summed over the partials in block order.
// Every sum has a fixed order: the same inputs give the same bits, run after run.  rbs_gauss_track does the D x D
// algebra on the host in binary64 (D = 12 B <= 36) with one synchronisation per frame; rbs_gauss_submit / _result run
// it on the device instead (rbs_gauss_predict_kernel before the render, rbs_gauss_reduce_update_kernel in place of
// the reduction), in the host's operation order, with up to two frames in flight.
namespace rbs {

constexpr int kGaussMaxBodies = 3;        // 6B(6B+1)/2 + 6B <= 256 entries: one per thread of the moments block
constexpr int kGaussBlocks = 256;         // moments grid: fixed, so the reduction order is too

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
    const int* err;           // rbs_gauss_submit's error word (nullptr: rbs_gauss_track)
};

template <int NB>
__global__ __launch_bounds__(256) void rbs_gauss_moments_kernel(const GaussArgs A)
{
    constexpr int NP = 6 * NB, ND = 1 + 2 * NP, NL = NP * (NP + 1) / 2, NE = NL + NP;
    static_assert(NE <= 256, "one Lambda / eta entry per thread");
    if (A.err && *A.err) return;
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

// ---- rbs_gauss_submit: the whole frame on the device.  The belief stays in device memory between frames; the host's
// binary64 algebra of track_impl is restated below in ITS operation order (dot products in ascending k from 0.0, the
// left-looking Cholesky, the same solves), so that with -ffp-contract=off and correctly rounded sqrt / division the
// prior and its factor are bit-identical to the host's; only device sin / cos / atan2 may differ in the last ulp.
constexpr int kGaussMaxD = 12 * kGaussMaxBodies, kGaussMaxNP = 6 * kGaussMaxBodies;

enum GaussError : int { kGaussOk = 0, kGaussNotPD = 1, kGaussInfoNotFinite = 2 };

struct GaussDev {
    int B, D, NP, nd;
    double vf;                // velocity_factor
    double sg[6];             // linear xyz, angular xyz sigmas
    double sqrtc;
    double* bel;              // the belief: z [D] | mu [D] | Sigma [D][D], state order
    double* prior;            // the frame's prior, same layout
    double* L;                // [D][D] Cholesky factor of the prior covariance, pose-first order
    double* mpf;              // [D] the prior mean, pose-first order
    double* poses;            // [nd][B][12] the sigma poses the render kernel reads
    int* err;                 // GaussError of the first frame that failed (sticky until rbs_gauss_initialize)
    const double* partials;   // [nblocks][ne] the moments kernel's
    int nblocks, ne;
    double* out;              // [ne] the reduced entries (rbs_gauss_get_moments)
    double* host;             // pinned result block of the frame's slot: z [D] | mu [D] | Sigma [D][D]
    int* host_word;           // pinned: [0] status (GaussError), [1] the frame's sequence number
    int seq;
};

// state index -> pose-first index (rbs_gauss.perm)
__device__ inline int gauss_perm(int i, int NP)
{
    const int b = i / 12, d = i - 12 * b;
    return d < 6 ? 6 * b + d : NP + 6 * b + (d - 6);
}

// Lower Cholesky factor of the symmetric n x n A (n <= 64) into L (zero above the diagonal), one row per thread of the
// block's first wave: element (i, j) is v = A[i][j], v -= L[i][k] L[j][k] for ascending k < j, then v / L[j][j] -- the
// host's cholesky() exactly.  false (uniform): not positive definite.
__device__ inline bool gauss_cholesky(const double* A, double* L, int n, double* s_col)
{
    const int t = threadIdx.x;
    for (int e = t; e < n * n; e += blockDim.x) L[e] = 0.0;
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        double v = 0.0;
        if (t >= j && t < n) {
            v = A[t * n + j];
#pragma unroll 8
            for (int k = 0; k < j; ++k) v -= L[t * n + k] * L[j * n + k];
            s_col[t] = v;
        }
        __syncthreads();
        const double d = s_col[j];
        if (!(d > 0.0) || !isfinite(d)) return false;
        const double ljj = sqrt(d);
        if (t == j) L[j * n + j] = ljj;
        else if (t > j && t < n) L[t * n + j] = v / ljj;
        __syncthreads();
    }
    return true;
}

// One workgroup (one wave): predict, symmetrise, permute, factor, sigma poses.
__global__ __launch_bounds__(64) void rbs_gauss_predict_kernel(const GaussDev G)
{
    __shared__ double s_S[kGaussMaxD * kGaussMaxD];   // Sigma^- (state order)
    __shared__ double s_W[kGaussMaxD * kGaussMaxD];   // A Sigma, then Sigma^- in pose-first order
    __shared__ double s_L[kGaussMaxD * kGaussMaxD];
    __shared__ double s_m[kGaussMaxD], s_col[kGaussMaxD], s_Rz[kGaussMaxBodies][9];
    __shared__ int s_bad;
    const int t = threadIdx.x, D = G.D, NP = G.NP, B = G.B;
    if (*G.err) return;                       // an earlier frame failed: this one reports the same (rbs_gauss_result)
    const double* z = G.bel;
    const double* mu = G.bel + D;
    const double* cov = G.bel + 2 * D;
    if (t == 0) s_bad = 0;
    __syncthreads();
    // (a non-finite belief: the host's products 0 x inf give NaN and its factorisation fails -- the same outcome, up front)
    for (int e = t; e < D * D; e += 64)
        if (!isfinite(cov[e])) s_bad = 1;
    __syncthreads();
    if (s_bad) {
        if (t == 0) *G.err = kGaussNotPD;
        return;
    }
    // mu^- = A mu, A Sigma, (A Sigma) A^T + Q.  A's row i: pose index i -> 1 at i, vf at i + 6; velocity index i -> vf at i.
    // The host sums over every k from 0.0; the terms left out here are 0 x (finite) = +-0, which change no bit of such a sum.
    for (int i = t; i < D; i += 64) {
        const bool pose = i % 12 < 6;
        const double v = pose ? (0.0 + 1.0 * mu[i]) + G.vf * mu[i + 6] : 0.0 + G.vf * mu[i];
        s_m[i] = v;
        G.prior[D + i] = v;
        G.prior[i] = z[i];
    }
    for (int e = t; e < D * D; e += 64) {
        const int i = e / D, j = e - i * D;
        s_W[e] = i % 12 < 6 ? (0.0 + 1.0 * cov[i * D + j]) + G.vf * cov[(i + 6) * D + j] : 0.0 + G.vf * cov[i * D + j];
    }
    __syncthreads();
    for (int e = t; e < D * D; e += 64) {
        const int i = e / D, j = e - i * D;
        const double v = j % 12 < 6 ? (0.0 + s_W[i * D + j] * 1.0) + s_W[i * D + j + 6] * G.vf : 0.0 + s_W[i * D + j] * G.vf;
        // Q = [[S, S], [S, S]] per body and per axis
        const int di = i % 12, dj = j % 12;
        const double sg = G.sg[di % 6];
        s_S[e] = v + ((i / 12 == j / 12 && di % 6 == dj % 6) ? sg * sg : 0.0);
    }
    __syncthreads();
    for (int e = t; e < D * D; e += 64) {     // symmetrise: each pair (i > j) belongs to one thread
        const int i = e / D, j = e - i * D;
        if (j < i) {
            const double v = 0.5 * (s_S[i * D + j] + s_S[j * D + i]);
            s_S[i * D + j] = s_S[j * D + i] = v;
        }
    }
    __syncthreads();
    for (int e = t; e < D * D; e += 64) {
        const int i = e / D, j = e - i * D;
        G.prior[2 * D + e] = s_S[e];
        s_W[gauss_perm(i, NP) * D + gauss_perm(j, NP)] = s_S[e];
    }
    for (int i = t; i < D; i += 64) G.mpf[gauss_perm(i, NP)] = s_m[i];
    if (t < B) rbd::rotvec_to_matrix(z + 12 * t + 3, s_Rz[t]);
    __syncthreads();
    if (!gauss_cholesky(s_W, s_L, D, s_col)) {
        if (t == 0) *G.err = kGaussNotPD;
        return;
    }
    for (int e = t; e < D * D; e += 64) G.L[e] = s_L[e];
    // the mean again in pose-first order (the global copy above is the update kernel's)
    for (int i = t; i < D; i += 64) s_col[gauss_perm(i, NP)] = s_m[i];
    __syncthreads();
    bool bad = false;
    for (int q = t; q < G.nd * B; q += 64) {
        const int k = q / B, b = q - k * B;
        const int j = (k - 1) / 2;
        const double sc = k == 0 ? 0.0 : ((k - 1) % 2 == 0 ? G.sqrtc : -G.sqrtc);
        double x[6], Rd[9];
#pragma unroll
        for (int d = 0; d < 6; ++d) x[d] = s_col[6 * b + d] + (k == 0 ? 0.0 : sc * s_L[(6 * b + d) * D + j]);
        rbd::rotvec_to_matrix(x + 3, Rd);
        double o[12];
        rbd::matmul3(Rd, s_Rz[b], o);
#pragma unroll
        for (int d = 0; d < 3; ++d) o[9 + d] = z[12 * b + d] + x[d];
        double* out = G.poses + (size_t)q * 12;
#pragma unroll
        for (int d = 0; d < 12; ++d) {
            out[d] = o[d];
            bad |= !isfinite(o[d]);
        }
    }
    if (bad) s_bad = 1;                       // (NaN poses never reach the rasterizer)
    __syncthreads();
    if (s_bad && t == 0) *G.err = kGaussNotPD;
}

// The frame's result block, then its number behind it with a system-scope release (rbt::publish_result's pattern).
__device__ inline void gauss_publish(const GaussDev& G, int status)
{
    if (threadIdx.x == 0) G.host_word[0] = status;
    __threadfence_block();
    __syncthreads();
    if (threadIdx.x == 0) __hip_atomic_store(G.host_word + 1, G.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// One block of 256: the fixed-order reduction (rbs_gauss_reduce_kernel's), then the update in the whitened space, the
// covariance, the re-centring, in track_impl's order; the new belief goes to device memory and to the slot's result block.
__global__ __launch_bounds__(256) void rbs_gauss_reduce_update_kernel(const GaussDev G)
{
    __shared__ double s_L[kGaussMaxD * kGaussMaxD], s_T[kGaussMaxD * kGaussMaxD], s_S[kGaussMaxD * kGaussMaxD];
    __shared__ double s_lam[kGaussMaxNP * kGaussMaxNP], s_M[kGaussMaxNP * kGaussMaxNP];
    __shared__ double s_x[(kGaussMaxNP + 1) * kGaussMaxNP];   // column c < NP: Lambda^-1 e_c; column NP: zeta
    __shared__ double s_e[256], s_col[kGaussMaxD], s_mup[kGaussMaxD];
    __shared__ double s_mu[kGaussMaxD];
    const int t = threadIdx.x, D = G.D, NP = G.NP, B = G.B;
    const int err = *G.err;
    if (err) {                                // (uniform) the frame failed before: report it, leave the belief
        gauss_publish(G, err);
        return;
    }
    if (t < G.ne) {                           // rbs_gauss_reduce_kernel's sum, bit for bit
        constexpr int kU = 32;
        double s = 0.0;
        for (int b0 = 0; b0 < G.nblocks; b0 += kU) {
            double v[kU];
#pragma unroll
            for (int u = 0; u < kU; ++u) v[u] = b0 + u < G.nblocks ? G.partials[(size_t)(b0 + u) * G.ne + t] : 0.0;
#pragma unroll
            for (int u = 0; u < kU; ++u)
                if (b0 + u < G.nblocks) s += v[u];
        }
        G.out[t] = s;
        s_e[t] = s;
    }
    for (int e = t; e < D * D; e += 256) s_L[e] = G.L[e];
    __syncthreads();
    // Lambda = I + sum pi h h^T (upper triangle, row-major, then eta), zeta = eta
    const int NL = NP * (NP + 1) / 2;
    if (t < NL) {
        int a = 0, rem = t;
        while (rem >= NP - a) { rem -= NP - a; ++a; }
        const int b = a + rem;
        s_lam[a * NP + b] = s_lam[b * NP + a] = s_e[t] + (a == b ? 1.0 : 0.0);
    } else if (t < NL + NP) {
        s_x[NP * NP + (t - NL)] = s_e[t];
    }
    for (int e = t; e < NP * NP; e += 256) s_x[e] = (e / NP == e % NP) ? 1.0 : 0.0;
    __syncthreads();
    if (!gauss_cholesky(s_lam, s_M, NP, s_col)) {
        if (t == 0) *G.err = kGaussInfoNotFinite;
        gauss_publish(G, kGaussInfoNotFinite);
        return;
    }
    if (t <= NP) {                            // chol_solve: column t of Lambda^-1 (t < NP), zeta (t = NP)
        double* x = s_x + t * NP;
        for (int i = 0; i < NP; ++i) {
            double v = x[i];
#pragma unroll 6
            for (int k = 0; k < i; ++k) v -= s_M[i * NP + k] * x[k];
            x[i] = v / s_M[i * NP + i];
        }
        for (int i = NP - 1; i >= 0; --i) {
            double v = x[i];
#pragma unroll 6
            for (int k = i + 1; k < NP; ++k) v -= s_M[k * NP + i] * x[k];
            x[i] = v / s_M[i * NP + i];
        }
    }
    __syncthreads();
    const double* zeta = s_x + NP * NP;
    for (int i = t; i < D; i += 256) {        // mu+ = mpf + L[:, :NP] zeta
        double v = G.mpf[i];
#pragma unroll 6
        for (int j = 0; j < NP; ++j) v += s_L[i * D + j] * zeta[j];
        s_mup[i] = v;
    }
    for (int e = t; e < D * D; e += 256) {    // T = L blockdiag(Lambda^-1, I); Lambda^-1[k][j] = column j's entry k
        const int i = e / D, j = e - i * D;
        if (j >= NP) { s_T[e] = s_L[e]; continue; }
        double v = 0.0;
#pragma unroll 6
        for (int k = 0; k < NP; ++k) v += s_L[i * D + k] * s_x[j * NP + k];
        s_T[e] = v;
    }
    __syncthreads();
    for (int e = t; e < D * D; e += 256) {    // Sigma+ = T L^T
        const int i = e / D, j = e - i * D;
        double v = 0.0;
#pragma unroll 12
        for (int k = 0; k < D; ++k) v += s_T[i * D + k] * s_L[j * D + k];
        s_S[e] = v;
    }
    __syncthreads();
    for (int e = t; e < D * D; e += 256) {
        const int i = e / D, j = e - i * D;
        if (j < i) {
            const double v = 0.5 * (s_S[i * D + j] + s_S[j * D + i]);
            s_S[i * D + j] = s_S[j * D + i] = v;
        }
    }
    __syncthreads();
    double* z = G.bel;
    for (int e = t; e < D * D; e += 256) {    // back to state order
        const int i = e / D, j = e - i * D;
        const double v = s_S[gauss_perm(i, NP) * D + gauss_perm(j, NP)];
        G.bel[2 * D + e] = v;
        G.host[2 * D + e] = v;
    }
    for (int i = t; i < D; i += 256) s_mu[i] = s_mup[gauss_perm(i, NP)];
    __syncthreads();
    if (t < B) {                              // re-centre: the mean's pose folds into z, z's velocities := the mean's
        double* zb = z + 12 * t;
        double* mb = s_mu + 12 * t;
        double Rz[9], Rm[9], Rn[9], zn[12];
        rbd::rotvec_to_matrix(zb + 3, Rz);
        rbd::rotvec_to_matrix(mb + 3, Rm);
        rbd::matmul3(Rm, Rz, Rn);
        for (int d = 0; d < 3; ++d) zn[d] = zb[d] + mb[d];
        rbd::matrix_to_rotvec(Rn, zn + 3);
        for (int d = 6; d < 12; ++d) zn[d] = mb[d];
        for (int d = 0; d < 6; ++d) mb[d] = 0.0;
        for (int d = 0; d < 12; ++d) {
            zb[d] = zn[d];
            G.host[12 * t + d] = zn[d];
        }
    }
    __syncthreads();
    for (int i = t; i < D; i += 256) {
        G.bel[D + i] = s_mu[i];
        G.host[D + i] = s_mu[i];
    }
    gauss_publish(G, kGaussOk);
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
    // rbs_gauss_submit / rbs_gauss_result: the belief, the last frame's prior, its factor and the permuted mean live
    // on the device; each frame's estimate lands in its slot's pinned result block
    double* d_bel = nullptr;                             // z [D] | mu [D] | Sigma [D][D]
    double* d_prior = nullptr;                           // the same layout: the last frame's prior
    double* d_L = nullptr;                               // [D][D]
    double* d_mpf = nullptr;                             // [D]
    int* d_err = nullptr;                                // rbs::GaussError, sticky until rbs_gauss_initialize
    double* h_bel = nullptr;                             // pinned: the host belief on its way up
    double* h_res[2] = {};                               // pinned result blocks: z | mu | Sigma
    double* h_res_dev[2] = {};
    int* h_word[2] = {};                                 // pinned: [0] status, [1] sequence number
    int* h_word_dev[2] = {};
    hipEvent_t ev_res[2] = {};
    long submitted = 0, collected = 0;
    int seq = 0, res_seq[2] = {};
    bool host_newer = true;                              // the host's belief is newer than the device's (initialize, track)
    bool dev_last = false;                               // the last completed frame ran on the device
    bool failed = false;                                 // a submitted frame failed: no frames until rbs_gauss_initialize
    std::string fail_msg;
    const double* submit64 = nullptr;                    // rbs_gauss_submit_f64's frame, on its way through rbs_gauss_submit
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

// The moments kernel's arguments (the frame: the sensor's observation, made current).
rbs::GaussArgs moments_args(rbs_gauss* g)
{
    rbs_handle* h = g->s;
    rbs::GaussArgs G{};
    G.planes = g->d_planes;
    G.rects = g->d_rects;
    G.frame = obs_frame(h);
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
    return G;
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
    if (int32_t rc = make_current(h, h->stream)) return rc;
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
    RBS_HIP(h, hipEventRecord(g->ev[0], s));
    rbs::launch_pose_planes(s, h->base, g->d_poses, nd, false, g->d_planes, g->d_rects, nullptr);
    RBS_HIP(h, hipGetLastError());
    RBS_HIP(h, hipEventRecord(g->ev[1], s));
    const rbs::GaussArgs G = moments_args(g);
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

// The device path's launch parameters.
rbs::GaussDev dev_args(rbs_gauss* g, int slot)
{
    rbs::GaussDev G{};
    G.B = g->B; G.D = g->D; G.NP = g->NP; G.nd = g->nd;
    G.vf = g->p.velocity_factor;
    for (int d = 0; d < 3; ++d) { G.sg[d] = g->p.linear_sigma[d]; G.sg[3 + d] = g->p.angular_sigma[d]; }
    G.sqrtc = g->sqrtc;
    G.bel = g->d_bel;
    G.prior = g->d_prior;
    G.L = g->d_L;
    G.mpf = g->d_mpf;
    G.poses = g->d_poses;
    G.err = g->d_err;
    G.partials = g->d_partials;
    G.nblocks = rbs::kGaussBlocks;
    G.ne = g->NE;
    G.out = g->d_out;
    G.host = g->h_res_dev[slot];
    G.host_word = g->h_word_dev[slot];
    return G;
}

// One frame enqueued: predict + sigma poses, render, moments, reduction + update, on the sensor's stream.
// *enqueued: something of this frame reached the device.
int32_t submit_impl(rbs_gauss* g, const float* f32, const double* f64, bool* enqueued)
{
    rbs_handle* h = g->s;
    if (!g->initialized) return gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_submit: rbs_gauss_initialize first");
    if (!h->shards.empty() || h->group || h->peer_world > 1)
        return gfail(g, RBS_ERR_UNSUPPORTED, "gauss_submit: single-device handles only");
    if (g->submitted - g->collected >= 2)
        return gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_submit: two frames are in flight already (call rbs_gauss_result)");
    RBS_REFUSE_POISONED(h);
    RBS_HIP(h, hipSetDevice(h->device));
    const size_t npx = (size_t)h->npx;
    const BorrowedFrameGuard borrowed_guard{h};
    const bool behind = g->submitted > g->collected;
    // a frame staged on a caller's stream (rbs_set_observation_device) is copied into the handle's buffer there: after the
    // frame in flight has read that buffer
    if (behind) if (int32_t rc = device_frame_after_readers(h)) return rc;
    if (f32) { if (int32_t rc = rbs_set_observation_f32(h, f32, npx)) return rc; }
    else if (f64) { if (int32_t rc = rbs_set_observation(h, f64, npx)) return rc; }
    if (int32_t rc = make_current(h, h->stream)) return rc;
    h->quiet = false;
    *enqueued = true;
    hipStream_t s = h->stream;
    const int D = g->D;
    if (g->host_newer) {   // after initialize or track: the host's belief goes up first
        std::memcpy(g->h_bel, g->z.data(), sizeof(double) * D);
        std::memcpy(g->h_bel + D, g->mu.data(), sizeof(double) * D);
        std::memcpy(g->h_bel + 2 * D, g->cov.data(), sizeof(double) * D * D);
        RBS_HIP(h, hipMemcpyAsync(g->d_bel, g->h_bel, sizeof(double) * (2 * D + (size_t)D * D), hipMemcpyHostToDevice, s));
        g->host_newer = false;
    }
    const int slot = (int)(g->submitted & 1);
    rbs::GaussDev G = dev_args(g, slot);
    G.seq = g->seq + 1;
    hipLaunchKernelGGL(rbs::rbs_gauss_predict_kernel, dim3(1), dim3(64), 0, s, G);
    RBS_HIP(h, hipGetLastError());
    RBS_HIP(h, hipEventRecord(g->ev[0], s));
    rbs::launch_pose_planes(s, h->base, g->d_poses, g->nd, false, g->d_planes, g->d_rects, g->d_err);
    RBS_HIP(h, hipGetLastError());
    RBS_HIP(h, hipEventRecord(g->ev[1], s));
    rbs::GaussArgs A = moments_args(g);
    A.err = g->d_err;
    switch (g->B) {
    case 1: hipLaunchKernelGGL(rbs::rbs_gauss_moments_kernel<1>, dim3(rbs::kGaussBlocks), dim3(256), 0, s, A); break;
    case 2: hipLaunchKernelGGL(rbs::rbs_gauss_moments_kernel<2>, dim3(rbs::kGaussBlocks), dim3(256), 0, s, A); break;
    default: hipLaunchKernelGGL(rbs::rbs_gauss_moments_kernel<3>, dim3(rbs::kGaussBlocks), dim3(256), 0, s, A); break;
    }
    RBS_HIP(h, hipGetLastError());
    // the frame's staging image has been read: frame N + 2's upload into it waits for this, not for the frame's result
    if (int32_t rc = frame_read_done(h, s)) return rc;
    RBS_HIP(h, hipEventRecord(g->ev[2], s));
    hipLaunchKernelGGL(rbs::rbs_gauss_reduce_update_kernel, dim3(1), dim3(256), 0, s, G);
    RBS_HIP(h, hipGetLastError());
    RBS_HIP(h, hipEventRecord(g->ev[3], s));
    RBS_HIP(h, hipEventRecord(g->ev_res[slot], s));
    g->seq += 1;
    g->res_seq[slot] = g->seq;
    g->submitted += 1;
    return RBS_OK;
}

// The last completed frame ran on the device: its prior, sigma poses, moments and kernel times into the host copies
// (the inspection functions read those), nothing in flight.
int32_t pull_inspection(rbs_gauss* g)
{
    rbs_handle* h = g->s;
    const int D = g->D;
    RBS_HIP(h, hipSetDevice(h->device));
    RBS_HIP(h, hipStreamSynchronize(h->stream));
    std::vector<double> pr(2 * D + (size_t)D * D);
    RBS_HIP(h, hipMemcpy(pr.data(), g->d_prior, sizeof(double) * pr.size(), hipMemcpyDeviceToHost));
    g->z_prior.assign(pr.begin(), pr.begin() + D);
    g->mu_prior.assign(pr.begin() + D, pr.begin() + 2 * D);
    g->cov_prior.assign(pr.begin() + 2 * D, pr.end());
    RBS_HIP(h, hipMemcpy(g->sigma.data(), g->d_poses, sizeof(double) * g->sigma.size(), hipMemcpyDeviceToHost));
    RBS_HIP(h, hipMemcpy(g->h_out, g->d_out, sizeof(double) * g->NE, hipMemcpyDeviceToHost));
    for (int k = 0; k < 3; ++k) RBS_HIP(h, hipEventElapsedTime(&g->ms[k], g->ev[k], g->ev[k + 1]));
    g->dev_last = false;
    return RBS_OK;
}

// rbs_gauss_track: at a frame boundary, on a tracker whose submitted frames have not failed.
int32_t track_gate(rbs_gauss* g)
{
    if (g->submitted != g->collected)
        return gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_track: frames submitted with rbs_gauss_submit are still in flight (call rbs_gauss_result)");
    if (g->failed)
        return gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_track: a submitted frame failed (" + g->fail_msg + "): call rbs_gauss_initialize");
    if (g->dev_last) return pull_inspection(g);   // (track_impl keeps the host copies the inspection functions read)
    return RBS_OK;
}

// Inspection and rbs_gauss_track need a frame boundary with nothing in flight.
int32_t refuse_in_flight(rbs_gauss* g, const char* what)
{
    if (g->submitted != g->collected)
        return gfail(g, RBS_ERR_INVALID_ARGUMENT, std::string(what) + ": frames submitted with rbs_gauss_submit are still in flight");
    if (g->dev_last) return pull_inspection(g);
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
    for (void* p : {(void*)g->d_planes, (void*)g->d_rects, (void*)g->d_poses, (void*)g->d_partials, (void*)g->d_out, (void*)g->d_bel,
                    (void*)g->d_prior, (void*)g->d_L, (void*)g->d_mpf, (void*)g->d_err})
        if (p) (void)hipFree(p);
    for (void* p : {(void*)g->h_poses, (void*)g->h_out, (void*)g->h_bel, (void*)g->h_res[0], (void*)g->h_res[1], (void*)g->h_word[0],
                    (void*)g->h_word[1]})
        if (p) (void)hipHostFree(p);
    for (hipEvent_t& e : g->ev)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t& e : g->ev_res)
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
    const size_t nbel = 2 * (size_t)g->D + (size_t)g->D * g->D;
    if (hipMalloc(&g->d_bel, sizeof(double) * nbel) != hipSuccess || hipMalloc(&g->d_prior, sizeof(double) * nbel) != hipSuccess ||
        hipMalloc(&g->d_L, sizeof(double) * g->D * g->D) != hipSuccess || hipMalloc(&g->d_mpf, sizeof(double) * g->D) != hipSuccess ||
        hipMalloc(&g->d_err, sizeof(int)) != hipSuccess || hipMemset(g->d_err, 0, sizeof(int)) != hipSuccess ||
        hipHostMalloc(&g->h_bel, sizeof(double) * nbel, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        fail(h, RBS_ERR_OUT_OF_MEMORY, "gauss_create: device or pinned memory");
        return cleanup(RBS_ERR_OUT_OF_MEMORY);
    }
    for (int k = 0; k < 2; ++k)
        if (hipHostMalloc(&g->h_res[k], sizeof(double) * nbel, hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc(&g->h_word[k], 2 * sizeof(int), hipHostMallocDefault) != hipSuccess ||
            hipHostGetDevicePointer(reinterpret_cast<void**>(&g->h_res_dev[k]), g->h_res[k], 0) != hipSuccess ||
            hipHostGetDevicePointer(reinterpret_cast<void**>(&g->h_word_dev[k]), g->h_word[k], 0) != hipSuccess) {
        (void)hipGetLastError();
        fail(h, RBS_ERR_OUT_OF_MEMORY, "gauss_create: device or pinned memory");
        return cleanup(RBS_ERR_OUT_OF_MEMORY);
    }
    for (int k = 0; k < 2; ++k) g->h_word[k][0] = g->h_word[k][1] = 0;
    for (hipEvent_t& e : g->ev_res)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            fail(h, RBS_ERR_HIP, "gauss_create: hipEventCreate failed");
            return cleanup(RBS_ERR_HIP);
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
    rbs_handle* h = g->s;
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
    // frames still in flight are dropped; a failed frame's error word is cleared, stream-ordered before the next frame
    RBS_HIP(h, hipSetDevice(h->device));
    if (g->submitted != g->collected) {
        RBS_HIP(h, hipStreamSynchronize(h->stream));
        g->collected = g->submitted;
    }
    RBS_HIP(h, hipMemsetAsync(g->d_err, 0, sizeof(int), h->stream));
    g->z.assign(default_state, default_state + D);
    g->mu.assign(D, 0.0);
    g->cov = c;
    g->initialized = true;
    g->tracked = false;
    g->host_newer = true;
    g->dev_last = false;
    g->failed = false;
    return RBS_OK;
}

int32_t rbs_gauss_track(rbs_gauss* g, const float* frame, double* out_state, double* out_cov)
{
    if (!g) return RBS_ERR_INVALID_ARGUMENT;
    if (int32_t rc = gauss::track_gate(g)) return rc;
    const int32_t rc = gauss::track_impl(g, frame, nullptr, out_state, out_cov);
    if (rc == RBS_OK) g->host_newer = true;
    return rc;
}

int32_t rbs_gauss_track_f64(rbs_gauss* g, const double* frame, double* out_state, double* out_cov)
{
    if (!g) return RBS_ERR_INVALID_ARGUMENT;
    if (int32_t rc = gauss::track_gate(g)) return rc;
    const int32_t rc = gauss::track_impl(g, nullptr, frame, out_state, out_cov);
    if (rc == RBS_OK) g->host_newer = true;
    return rc;
}

int32_t rbs_gauss_get_prior(rbs_gauss* g, double* default_state, double* mean, double* cov)
{
    if (!g) return RBS_ERR_INVALID_ARGUMENT;
    if (int32_t rc = gauss::refuse_in_flight(g, "gauss_get_prior")) return rc;
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
    if (int32_t rc = gauss::refuse_in_flight(g, "gauss_get_sigma_poses")) return rc;
    if (!g->tracked) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_get_sigma_poses: no frame tracked yet");
    std::memcpy(out, g->sigma.data(), sizeof(double) * g->sigma.size());
    return RBS_OK;
}

int32_t rbs_gauss_get_render(rbs_gauss* g, int32_t k, float* out)
{
    if (!g) return RBS_ERR_INVALID_ARGUMENT;
    rbs_handle* h = g->s;
    if (!out || k < 0 || k >= g->nd) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_get_render: bad index or null pointer");
    if (int32_t rc = gauss::refuse_in_flight(g, "gauss_get_render")) return rc;
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
    if (int32_t rc = gauss::refuse_in_flight(g, "gauss_get_moments")) return rc;
    if (!g->tracked) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_get_moments: no frame tracked yet");
    *n = g->NE;
    std::memcpy(out, g->h_out, sizeof(double) * g->NE);   // (track_impl synchronised before it read them; pull_inspection copied them)
    return RBS_OK;
}

int32_t rbs_gauss_kernel_ms(rbs_gauss* g, float* out3)
{
    if (!g) return RBS_ERR_INVALID_ARGUMENT;
    if (!out3) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_kernel_ms: null pointer");
    if (int32_t rc = gauss::refuse_in_flight(g, "gauss_kernel_ms")) return rc;
    if (!g->tracked) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_kernel_ms: no frame tracked yet");
    for (int k = 0; k < 3; ++k) out3[k] = g->ms[k];
    return RBS_OK;
}


int32_t rbs_gauss_submit(rbs_gauss* g, const float* frame)
{
    if (!g) return RBS_ERR_INVALID_ARGUMENT;
    if (g->failed) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_submit: a submitted frame failed (" + g->fail_msg + "): call rbs_gauss_initialize");
    bool enqueued = false;
    const int32_t rc = gauss::submit_impl(g, g->submit64 ? nullptr : frame, g->submit64, &enqueued);
    g->submit64 = nullptr;
    if (rc != RBS_OK && (enqueued || (rc != RBS_ERR_INVALID_ARGUMENT && rc != RBS_ERR_UNSUPPORTED))) {
        // drain what was enqueued and refuse further frames: the device belief is out of step with the frames
        rbs_handle* h = g->s;
        const std::string why = h->err;
        (void)hipSetDevice(h->device);
        (void)hipStreamSynchronize(h->stream);
        (void)hipStreamSynchronize(h->up_stream);
        (void)hipGetLastError();
        g->failed = true;
        g->fail_msg = why;
        h->err = why;
    }
    return rc;
}

int32_t rbs_gauss_submit_f64(rbs_gauss* g, const double* frame)
{
    if (!g) return RBS_ERR_INVALID_ARGUMENT;
    if (!frame) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_submit_f64: null frame");
    g->submit64 = frame;
    const int32_t rc = rbs_gauss_submit(g, nullptr);
    g->submit64 = nullptr;
    return rc;
}

int32_t rbs_gauss_result(rbs_gauss* g, double* out_state, double* out_cov)
{
    if (!g) return RBS_ERR_INVALID_ARGUMENT;
    if (!out_state) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_result: out_state is NULL");
    if (g->collected >= g->submitted) return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, "gauss_result: no frame in flight");
    rbs_handle* h = g->s;
    const int slot = (int)(g->collected & 1);
    g->collected += 1;
    RBS_HIP(h, hipSetDevice(h->device));
    // The reduce + update kernel stores the result block into pinned memory and the frame's number behind it with a
    // system-scope release: spin on the number (rbs_tracker_result's rule), the event is the fall-back.
    bool seen = false;
    volatile int* seq = g->h_word[slot] + 1;
    for (long it = 0; it < 4000000 && !seen; ++it) {
        seen = __atomic_load_n(seq, __ATOMIC_ACQUIRE) == g->res_seq[slot];
        if (!seen && (it & 255) == 255 && hipEventQuery(g->ev_res[slot]) == hipSuccess) break;
        if (!seen) __builtin_ia32_pause();
    }
    if (!seen) RBS_HIP(h, hipEventSynchronize(g->ev_res[slot]));
    if (g->submitted == g->collected) h->quiet = !h->async_outstanding;
    const int status = __atomic_load_n(g->h_word[slot], __ATOMIC_ACQUIRE);
    if (status != rbs::kGaussOk) {
        const char* why = status == rbs::kGaussNotPD ? "gauss_result: the predicted covariance is not positive definite"
                                                     : "gauss_result: the information matrix is not finite (the frame?)";
        g->failed = true;
        g->fail_msg = why;
        return gauss::gfail(g, RBS_ERR_INVALID_ARGUMENT, why);
    }
    const int D = g->D;
    const double* r = g->h_res[slot];
    g->z.assign(r, r + D);
    g->mu.assign(r + D, r + 2 * D);
    g->cov.assign(r + 2 * D, r + 2 * D + (size_t)D * D);
    g->tracked = true;
    g->dev_last = true;
    std::memcpy(out_state, r, sizeof(double) * D);
    if (out_cov) std::memcpy(out_cov, r + 2 * D, sizeof(double) * D * D);
    return RBS_OK;
}

}  // extern "C"
