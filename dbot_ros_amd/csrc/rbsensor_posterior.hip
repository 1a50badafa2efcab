// rbsensor_posterior.hip -- the particle tracker's posterior report (include/rbsensor_mi355x.h, "Posterior report"): weighted
// mean, covariance, effective sample size and the number of occlusion planes alive, of the population a frame leaves behind,
// reduced on the device behind the frame's own kernels.  Opt-in (rbs_tracker_set_posterior); with it off nothing here is launched.
//
// The population: x_i = particle i's deltas as rbs_tracker_get would return them after the frame -- re-centred.  The kernels
// are launched LAST in a frame's chain and are told whether the re-centring has happened (filter_step_kernel,
// RBS_TRACKER_RECENTRE_NOW=1) or is pending (T.mean / RmT hold what recentre_body needs).  Pending, a launch in front
// (rbs_post_recentre_kernel, one thread per particle) takes a REGISTER copy of every body's six pose components, applies
// recentre_body -- the function recentre_kernel calls, so the same bits -- and keeps the result in PostDev::pose, a buffer
// of the report's own ([n][bodies][6]); the passes behind read the pose from there and the velocities from the particles.
// (recentre_body alone takes 114 registers: re-centring again inside every accumulation loop, with the accumulators live
// across it, does not fit the 128 registers of a 1 024-thread block and spilled 25 to 148 of them.)  Nothing of the filter's
// is written: the kernels read part, logw, idx, mean, flag and write PostDev's buffers only.
//
// Rule (two passes, binary64, -ffp-contract=off):  m = max lw,  e_i = exp(lw_i - m),  S = sum e_i,  Q = sum e_i^2,
//   ess = S^2 / Q,   mean[c] = (sum e_i x_i[c]) / S,   cov[a][b] = (sum (e_i (x_i[a] - mean[a])) (x_i[b] - mean[b])) / S  for a <= b,
// mirrored into b > a.  survivors = distinct values among idx_i (a bitmap of n bits: integer OR and popcount, order-free).
// At least one log-weight is finite (the filter's own weights need the same): with every lw_i = -inf, m = -inf, every e_i
// and with them mean, cov and ess are NaN -- outside the contract, as in the numpy twin.
//
// Tiling.  D = 12 per body reaches 36 at three bodies: 666 upper-triangle entries do not fit a thread.  The components are
// cut into column groups of six -- a body's pose (position, rotation vector) and its velocities -- and row groups of three,
// and the upper triangle is walked in tiles of 3 x 6 components (row group ra against column groups gb >= ra / 2): 18
// accumulators per thread, the nine values of a particle re-read per tile (L2).  D / 6 = G: G (G + 1) tiles -- 6 for one
// body, 42 for three.  (6 x 6 tiles: the 36 accumulators, a particle's twelve values and the block reduction do not fit the
// 128 registers of a 1 024-thread block -- 18 to 50 spilled.)  The compiler's report (lib/resource_usage.txt) shows no
// scratch and no spilled register for every kernel here, which tests/test_tracker_posterior_cpu.py asserts.
//
// Order of every sum: fixed by n alone.  Single-block form (n < kMultiBlockFrom, one launch): w = min(16, ceil(n / 256))
// waves are at work, thread t < 64 w takes particles t, t + 64 w, ...; then block_sum's shuffle tree and its order over the
// sixteen waves (mean_body's pattern; the idle waves' zeros included).  Grid form (five
// launches over kChunk-particle chunks): thread t of chunk c takes c kChunk + t + 1024 k, k < 4 (mean_m2_kernel's pattern);
// the per-chunk partials are folded by one block in chunk order.  No floating-point atomics: two runs, frame by frame or
// with look-ahead, give the same bits; the two forms differ from each other in the last bits as mean_kernel and
// mean_m1..m3 do.
#pragma once

namespace rbt {

constexpr int kPostAcc = 18;                     // a tile: 3 x 6 components of the upper triangle
constexpr int kPostMaxD = rbs::kMaxBodies * kBody;

struct PostDev {
    // the tracker's own allocation, grid form only (post_partials_doubles): per chunk the maximum, S, Q, sum e x [D] and the
    // upper triangle's sums [D (D + 1) / 2]; then the head: S, mean [D]
    double* partials;
    unsigned* bitmap;      // [(n + 31) / 32], grid form only
    double* pose;          // [n][bodies][6]: the re-centred pose components while the filter's own re-centring is pending
    double* e;             // [n]: exp(lw_i - m), stored by the first pass (an exp inside the tile loops, the accumulators live, spilled)
    double* out;           // [1 + D + D D]: ess, mean, cov row-major (pinned host memory as the device addresses it, or device memory)
    int* out_i;            // [4]: n, survivors, resampled, frame
};

inline int post_blocks(int n) { return (n + kChunk - 1) / kChunk; }
inline size_t post_tri(int D) { return (size_t)D * (D + 1) / 2; }
inline size_t post_partials_doubles(int n, int D) { return (size_t)post_blocks(n) * (3 + D + post_tri(D)) + 1 + D; }
inline size_t post_out_doubles(int D) { return 1 + (size_t)D + (size_t)D * D; }

// where the grid form keeps what
struct PostLayout {
    double *mx, *se, *sq, *sx, *tri, *head;
    int tri_n;
};
__host__ __device__ inline PostLayout post_layout(const PostDev& P, int blocks, int D)
{
    PostLayout L;
    L.tri_n = D * (D + 1) / 2;
    L.mx = P.partials;
    L.se = L.mx + blocks;
    L.sq = L.se + blocks;
    L.sx = L.sq + blocks;
    L.tri = L.sx + (size_t)blocks * D;
    L.head = L.tri + (size_t)blocks * L.tri_n;
    return L;
}

// pending: every body's six pose components of particle i, re-centred on a register copy, into P.pose
__device__ inline void post_recentre_copy(const TrackerDev& T, const PostDev& P, const double* __restrict__ part, int i)
{
    for (int b = 0; b < T.parts; ++b) {
        double x[6];
        const double* p = part + (size_t)i * T.D + b * kBody;
#pragma unroll
        for (int k = 0; k < 6; ++k) x[k] = p[k];
        recentre_body(T, x, b);
        double* out = P.pose + ((size_t)i * T.parts + b) * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) out[k] = x[k];
    }
}

// Pending only, in front of either form: one thread per particle, launched with 256 as recentre_kernel is (recentre_body
// takes 114 registers; inside a 1 024-thread kernel, whose budget is 128, it spilled)
__global__ __launch_bounds__(256) void rbs_post_recentre_kernel(const TrackerDev T, const PostDev P, const double* __restrict__ part)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < T.n) post_recentre_copy(T, P, part, i);
}

// components [6 g, 6 g + 6) of particle i, re-centred: even groups are a body's pose
__device__ inline void post_load6(const TrackerDev& T, const PostDev& P, const double* __restrict__ part, int i, int g, bool pending, double* x)
{
    const double* p = pending && !(g & 1) ? P.pose + ((size_t)i * T.parts + (g >> 1)) * 6 : part + (size_t)i * T.D + g * 6;
#pragma unroll
    for (int k = 0; k < 6; ++k) x[k] = p[k];
}

// K values per thread summed over the block, each exactly as block_sum sums one (shuffle tree, then the sixteen waves in
// order): thread c < K returns the sum of a[c].  Blocks of 1 024 threads.  Waves from `waves` on hold zeros only (they took
// no particle) and skip the tree -- the sum of zeros is the zero they hold: the same bits, and 12 K cross-lane moves per
// wave less through the one LDS pipe the sixteen waves share (measured: that pipe, not the particles, is the kernel's time).
template <int K>
__device__ inline double post_block_sums(double* a, double (*shb)[kPostAcc], int waves = 16)
{
    if ((int)(threadIdx.x >> 6) < waves)
#pragma unroll
        for (int c = 0; c < K; ++c)
            for (int off = 32; off > 0; off >>= 1) a[c] += __shfl_down(a[c], off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int c = 0; c < K; ++c) shb[threadIdx.x >> 6][c] = a[c];
    __syncthreads();
    double sum = 0.0;
    if ((int)threadIdx.x < K)
        for (int w = 0; w < 16; ++w) sum += shb[w][threadIdx.x];
    return sum;
}

// components [3 r, 3 r + 3) likewise: a body's position, rotation vector, linear or angular velocity
__device__ inline void post_load3(const TrackerDev& T, const PostDev& P, const double* __restrict__ part, int i, int r, bool pending, double* x)
{
    const int body = r >> 2, q = r & 3;
    const double* p = pending && q < 2 ? P.pose + ((size_t)i * T.parts + body) * 6 + 3 * q : part + (size_t)i * T.D + 3 * r;
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = p[k];
}

// One particle's terms of tile (ra, gb): rows [3 ra, 3 ra + 3), columns [6 gb, 6 gb + 6).
__device__ inline void post_tile_terms(const TrackerDev& T, const PostDev& P, const double* __restrict__ part, int i, int ra, int gb,
                                       bool pending, double e, const double* mean, double* acc)
{
    double xa[3], xb[6];
    post_load3(T, P, part, i, ra, pending, xa);
    post_load6(T, P, part, i, gb, pending, xb);
    double eda[3], db[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) eda[k] = e * (xa[k] - mean[3 * ra + k]);
#pragma unroll
    for (int k = 0; k < 6; ++k) db[k] = xb[k] - mean[6 * gb + k];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 6; ++b) acc[6 * a + b] += eda[a] * db[b];
}

// tiles of the upper triangle in the order they are walked: row group ra ascending, column groups gb = ra / 2 .. G - 1
__host__ __device__ inline int post_tiles(int D) { const int G = D / 6; return G * (G + 1); }
__device__ inline void post_tile_of(int D, int t, int& ra, int& gb)
{
    const int G = D / 6;
    ra = 0;
    while (t >= G - (ra >> 1)) { t -= G - (ra >> 1); ra += 1; }
    gb = (ra >> 1) + t;
}

// ------------------------------------------------------------------ single-block form
__global__ __launch_bounds__(1024) void rbs_post_kernel(const TrackerDev T, const PostDev P, const double* __restrict__ part, int recentred)
{
    __shared__ double sh[16];
    __shared__ double shb[16][kPostAcc];
    __shared__ double sh_mean[kPostMaxD];
    __shared__ unsigned bm[kMultiBlockFrom / 32];
    __shared__ int sh_cnt;
    const int n = T.n, D = T.D, tid = threadIdx.x;
    const bool pending = recentred == 0;
    // Particles go to the first `waves` waves, four a lane until all sixteen are at work (a function of n alone): thread
    // t < 64 waves takes t, t + 64 waves, ...  The other waves hold zeros and skip the reductions' shuffle trees.
    const int waves = min(16, max(1, (n + 255) / 256)), stride = 64 * waves;
    const int first = tid < stride ? tid : n;
    double m = -INFINITY;
    for (int i = first; i < n; i += stride) m = fmax(m, T.logw[i]);
    m = rbd::block_max(m, sh);
    double s = 0.0, q = 0.0;
    for (int i = first; i < n; i += stride) {   // (a thread reads back below only the e_i it stored here)
        const double e = exp(T.logw[i] - m);
        P.e[i] = e;
        s += e;
        q += e * e;
    }
    const double S = rbd::block_sum(s, sh);
    const double Q = rbd::block_sum(q, sh);
    // survivors: a bitmap of n bits in LDS (slot values are < n; anything else is not a slot and is not counted)
    for (int w = tid; w < kMultiBlockFrom / 32; w += 1024) bm[w] = 0u;
    if (tid == 0) sh_cnt = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 1024) {
        const int v = T.idx[i];
        if ((unsigned)v < (unsigned)n) atomicOr(&bm[v >> 5], 1u << (v & 31));
    }
    __syncthreads();
    int cnt = 0;
    for (int w = tid; w < kMultiBlockFrom / 32; w += 1024) cnt += __popc(bm[w]);
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if ((tid & 63) == 0) atomicAdd(&sh_cnt, cnt);
    // first pass: the mean, six components at a time
    for (int g = 0; g < D / 6; ++g) {
        double a[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) a[c] = 0.0;
        for (int i = first; i < n; i += stride) {
            const double e = P.e[i];
            double x[6];
            post_load6(T, P, part, i, g, pending, x);
#pragma unroll
            for (int c = 0; c < 6; ++c) a[c] += e * x[c];
        }
        const double sum = post_block_sums<6>(a, shb, waves);
        if (tid < 6) sh_mean[6 * g + tid] = sum / S;
    }
    __syncthreads();
    if (tid == 0) {
        P.out[0] = S * S / Q;
        P.out_i[0] = n;
        P.out_i[1] = sh_cnt;
        P.out_i[2] = T.flag[0];
        P.out_i[3] = (int)(T.frame + 1);
    }
    for (int c = tid; c < D; c += 1024) P.out[1 + c] = sh_mean[c];
    // second pass: central moments, tile by tile
    double* cov = P.out + 1 + D;
    const int tiles = post_tiles(D);
    for (int t = 0; t < tiles; ++t) {
        int ra, gb;
        post_tile_of(D, t, ra, gb);
        double acc[kPostAcc];
#pragma unroll
        for (int c = 0; c < kPostAcc; ++c) acc[c] = 0.0;
        for (int i = first; i < n; i += stride) post_tile_terms(T, P, part, i, ra, gb, pending, P.e[i], sh_mean, acc);
        const double sum = post_block_sums<kPostAcc>(acc, shb, waves);
        if (tid < kPostAcc) {
            const int a = 3 * ra + tid / 6, b = 6 * gb + tid % 6;
            if (a <= b) {
                const double v = sum / S;
                cov[(size_t)a * D + b] = v;
                cov[(size_t)b * D + a] = v;
            }
        }
    }
}

// ------------------------------------------------------------------ grid form: chunks of kChunk particles
// g1: per-chunk maximum of the log-weights; the chunk's words of the bitmap are cleared for g2
__global__ __launch_bounds__(1024) void rbs_post_max_kernel(const TrackerDev T, const PostDev P)
{
    __shared__ double sh[16];
    const PostLayout L = post_layout(P, (int)gridDim.x, T.D);
    double m = -INFINITY;
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * kChunk + k * 1024 + (int)threadIdx.x;
        if (i < T.n) m = fmax(m, T.logw[i]);
    }
    m = rbd::block_max(m, sh);
    if (threadIdx.x == 0) L.mx[blockIdx.x] = m;
    const int words = (T.n + 31) / 32, w = blockIdx.x * (kChunk / 32) + (int)threadIdx.x;
    if ((int)threadIdx.x < kChunk / 32 && w < words) P.bitmap[w] = 0u;
}

// g2: per chunk S, Q and sum e x; the slot bitmap
__global__ __launch_bounds__(1024) void rbs_post_sums_kernel(const TrackerDev T, const PostDev P, const double* __restrict__ part, int recentred)
{
    __shared__ double sh[16];
    __shared__ double shb[16][kPostAcc];
    const PostLayout L = post_layout(P, (int)gridDim.x, T.D);
    const bool pending = recentred == 0;
    double m = -INFINITY;
    for (int b = threadIdx.x; b < (int)gridDim.x; b += 1024) m = fmax(m, L.mx[b]);
    m = rbd::block_max(m, sh);
    double e[4], se = 0.0, sq = 0.0;
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * kChunk + k * 1024 + (int)threadIdx.x;
        e[k] = i < T.n ? exp(T.logw[i] - m) : 0.0;
        if (i < T.n) P.e[i] = e[k];
        se += e[k];
        sq += e[k] * e[k];
        if (i < T.n) {
            const int v = T.idx[i];
            // (after a resampling thousands of particles name the same few slots: an atomic each serialised on those words,
            //  0.24 ms at 20 000 particles; a bit that is seen set needs none)
            if ((unsigned)v < (unsigned)T.n &&
                !(__hip_atomic_load(P.bitmap + (v >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & (1u << (v & 31))))
                atomicOr(P.bitmap + (v >> 5), 1u << (v & 31));
        }
    }
    se = rbd::block_sum(se, sh);
    sq = rbd::block_sum(sq, sh);
    if (threadIdx.x == 0) { L.se[blockIdx.x] = se; L.sq[blockIdx.x] = sq; }
    for (int g = 0; g < T.D / 6; ++g) {
        double a[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) a[c] = 0.0;
        for (int k = 0; k < 4; ++k) {
            const int i = blockIdx.x * kChunk + k * 1024 + (int)threadIdx.x;
            if (i < T.n) {
                double x[6];
                post_load6(T, P, part, i, g, pending, x);
#pragma unroll
                for (int c = 0; c < 6; ++c) a[c] += e[k] * x[c];
            }
        }
        const double sum = post_block_sums<6>(a, shb);
        if ((int)threadIdx.x < 6) L.sx[(size_t)blockIdx.x * T.D + 6 * g + threadIdx.x] = sum;
    }
}

// g3 (one block): S, Q and the mean in chunk order; ess; survivors = popcount of the bitmap; the integers
__global__ __launch_bounds__(1024) void rbs_post_mean_kernel(const TrackerDev T, const PostDev P, int blocks)
{
    __shared__ int sh_cnt;
    const PostLayout L = post_layout(P, blocks, T.D);
    const int tid = threadIdx.x;
    if (tid == 0) sh_cnt = 0;
    __syncthreads();
    double S = 0.0, Q = 0.0;      // (the threads that divide by S sum it, each in chunk order; thread 0 also Q)
    if (tid < T.D)
        for (int b = 0; b < blocks; ++b) S += L.se[b];
    if (tid == 0)
        for (int b = 0; b < blocks; ++b) Q += L.sq[b];
    for (int c = tid; c < T.D; c += 1024) {
        double sum = 0.0;
        for (int b = 0; b < blocks; ++b) sum += L.sx[(size_t)b * T.D + c];
        const double mu = sum / S;
        L.head[1 + c] = mu;
        P.out[1 + c] = mu;
    }
    int cnt = 0;
    const int words = (T.n + 31) / 32;
    for (int w = tid; w < words; w += 1024) cnt += __popc(P.bitmap[w]);
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if ((tid & 63) == 0) atomicAdd(&sh_cnt, cnt);
    __syncthreads();
    if (tid == 0) {
        L.head[0] = S;
        P.out[0] = S * S / Q;
        P.out_i[0] = T.n;
        P.out_i[1] = sh_cnt;
        P.out_i[2] = T.flag[0];
        P.out_i[3] = (int)(T.frame + 1);
    }
}

// g4: grid (chunks, tiles): a chunk's sums of one tile of the upper triangle
__global__ __launch_bounds__(1024) void rbs_post_cov_kernel(const TrackerDev T, const PostDev P, const double* __restrict__ part, int recentred)
{
    __shared__ double shb[16][kPostAcc];
    __shared__ double sh_mean[kPostMaxD];
    const PostLayout L = post_layout(P, (int)gridDim.x, T.D);
    const int D = T.D, tid = threadIdx.x;
    const bool pending = recentred == 0;
    for (int c = tid; c < D; c += 1024) sh_mean[c] = L.head[1 + c];
    __syncthreads();
    int ra, gb;
    post_tile_of(D, (int)blockIdx.y, ra, gb);
    double acc[kPostAcc];
#pragma unroll
    for (int c = 0; c < kPostAcc; ++c) acc[c] = 0.0;
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * kChunk + k * 1024 + tid;
        if (i < T.n) post_tile_terms(T, P, part, i, ra, gb, pending, P.e[i], sh_mean, acc);
    }
    const double sum = post_block_sums<kPostAcc>(acc, shb);
    if (tid < kPostAcc) {
        const int a = 3 * ra + tid / 6, b = 6 * gb + tid % 6;
        if (a <= b) L.tri[(size_t)blockIdx.x * L.tri_n + (size_t)a * D - (size_t)a * (a - 1) / 2 + (b - a)] = sum;
    }
}

// g5 (one block): every entry of the upper triangle summed in chunk order, divided by S, mirrored
__global__ __launch_bounds__(1024) void rbs_post_cov_fold_kernel(const TrackerDev T, const PostDev P, int blocks)
{
    const PostLayout L = post_layout(P, blocks, T.D);
    const int D = T.D;
    const double S = L.head[0];
    double* cov = P.out + 1 + D;
    for (int t = threadIdx.x; t < L.tri_n; t += 1024) {
        int a = 0, r = t;
        while (r >= D - a) { r -= D - a; a += 1; }
        const int b = a + r;
        double sum = 0.0;
        for (int k = 0; k < blocks; ++k) sum += L.tri[(size_t)k * L.tri_n + t];
        const double v = sum / S;
        cov[(size_t)a * D + b] = v;
        cov[(size_t)b * D + a] = v;
    }
}

}  // namespace rbt
