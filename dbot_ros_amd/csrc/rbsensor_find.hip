// rbsensor_find.hip -- the object finder (rbs_find_*, include/rbsensor_mi355x.h).  Included at the
// end of rbsensor_capi.hip: it scores through handles of its own made from the sensor's configuration
// (rbs_handle::cfg), so every score comes from the sensor's raster kernels.
//
// Per find, on the coarse scoring handle's stream:
//   rbs_find_subsample_kernel   every f-th pixel of every f-th row of the frame already on the device
//   (rbs_findfg_*_kernel)       opt-in step 1b (rbs_find_set_foreground): the dominant inverse-depth plane of the coarse frame
//                               from three-point trials, and the seeding frame -- the coarse frame with every pixel that is not
//                               strictly in front of that plane NaN.  The seed kernel then reads the seeding frame.
//   rbs_find_seed_kernel        one block: valid seed-grid pixels compacted in row-major order, then thinned
//   rbs_find_hyp_kernel         hypothesis h -> pose (Super-Fibonacci rotation, seed translation), binary64
//   (rbs_loglikes_device)       coarse scores, `batch` hypotheses per launch
//   rbs_find_topk_kernel        per 2 048-item chunk: bitonic sort in LDS, the best k written; repeated until one chunk
//   rbs_find_nms_kernel         one wave: greedy suppression in candidate order
//   rbs_find_children_kernel    a round's children (Philox4x32-10 normals), then (rbs_loglikes_device) their scores
//   rbs_find_select_kernel      each survivor keeps its best child
//   (rbs_findr_*_kernel)        opt-in step 6b (rbs_find_set_refinement) in place of step 6's fixed schedule: every survivor
//                               carries a 6 x 6 search covariance; its children are drawn through the covariance's factor and
//                               the covariance is re-estimated from the round's best children, all on the device
//   (rbs_findc_*_kernel)        opt-in gate (rbs_find_set_gate; rbsensor_find_gate.hip): every hypothesis' assess and contour
//                               evidence behind its coarse score (step 4b), the confirmed ones first in steps 5 and 7
// Every order is fixed: the same frame gives the same bits, whatever `batch`.
#include <climits>

namespace rbf {

constexpr int kTopC = 2048;        // items per top-k chunk (LDS: 16 bytes each; > kMaxCandidates, so every pass at least halves the items)
constexpr int kTopThreads = 1024;
constexpr int kMaxCandidates = 1024;
constexpr int kMaxSurvivors = 64;  // one wave's lanes in the suppression
constexpr int kSeedThreads = 1024;
constexpr double kPsi = 1.533751168755204288118041;   // psi^4 = psi + 4 (Alexa 2022)
constexpr double kTwoPi = 6.283185307179586;

struct HypParams {
    const double* seeds;   // [n_seeds][4] (u, v, d, pixel)
    int n_rot;
    double fx, fy, cx, cy; // coarse K
    double offset;
};

// (x, y, z, w) unit quaternion of Super-Fibonacci point i of n, as a row-major rotation matrix
__device__ __host__ inline void sf_rotation(long i, int n, double* R)
{
    const double s = (double)i + 0.5;
    const double t = s / (double)n;
    const double r = sqrt(t), Rr = sqrt(1.0 - t);
    const double a = kTwoPi * s / 1.4142135623730951, b = kTwoPi * s / kPsi;
    const double x = r * sin(a), y = r * cos(a), z = Rr * sin(b), w = Rr * cos(b);
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z);       R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);       R[7] = 2.0 * (y * z + w * x);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

__device__ inline void hyp_pose(const HypParams& H, long h, double* __restrict__ out)
{
    const long s = h / H.n_rot;
    const int r = (int)(h - s * H.n_rot);
    sf_rotation(r, H.n_rot, out);
    const double u = H.seeds[4 * s], v = H.seeds[4 * s + 1], d = H.seeds[4 * s + 2];
    const double x = (u - H.cx) / H.fx, y = (v - H.cy) / H.fy;
    const double nrm = sqrt(x * x + y * y + 1.0);
    out[9] = d * x + H.offset * (x / nrm);
    out[10] = d * y + H.offset * (y / nrm);
    out[11] = d + H.offset * (1.0 / nrm);
}

__global__ __launch_bounds__(256) void rbs_find_subsample_kernel(const float* __restrict__ src, int src_cols, float* __restrict__ dst,
                                                                 int rows, int cols, int f)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= rows * cols) return;
    const int r = p / cols, c = p - r * cols;
    dst[p] = src[(size_t)r * f * src_cols + (size_t)c * f];
}

// One block.  cells: [ceil(rows/s) * ceil(cols/s)] scratch of compacted pixel indices; info[0] := kept, info[1] := valid.
__global__ __launch_bounds__(kSeedThreads) void rbs_find_seed_kernel(const float* __restrict__ frame, int rows, int cols, int stride,
                                                                     double dmin, double dmax, int max_seeds, int* __restrict__ cells,
                                                                     double* __restrict__ seeds, int* __restrict__ info)
{
    __shared__ int wave_sum[kSeedThreads / 64];
    __shared__ int base;
    const int gr = (rows + stride - 1) / stride, gc = (cols + stride - 1) / stride, ncell = gr * gc;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) base = 0;
    __syncthreads();
    for (int c0 = 0; c0 < ncell; c0 += kSeedThreads) {
        const int c = c0 + (int)threadIdx.x;
        int px = -1;
        if (c < ncell) {
            const int i = c / gc, j = c - i * gc;
            const int p = i * stride * cols + j * stride;
            const double d = (double)frame[p];
            if (d >= dmin && d <= dmax) px = p;   // (NaN and inf fail one of the two)
        }
        const unsigned long long m = __ballot(px >= 0);
        const int before = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_sum[wv] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wv; ++w) off += wave_sum[w];
        if (px >= 0) cells[off + before] = px;
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
            for (int w = 0; w < kSeedThreads / 64; ++w) tot += wave_sum[w];
            base += tot;
        }
        __syncthreads();
    }
    const int n = base;
    const int step = n > max_seeds ? (n + max_seeds - 1) / max_seeds : 1;
    const int kept = (n + step - 1) / step;
    for (int i = threadIdx.x; i < kept; i += kSeedThreads) {
        const int p = cells[(size_t)i * step];
        const int v = p / cols, u = p - v * cols;
        seeds[4 * i] = (double)u;
        seeds[4 * i + 1] = (double)v;
        seeds[4 * i + 2] = (double)frame[p];
        seeds[4 * i + 3] = (double)p;
    }
    if (threadIdx.x == 0) { info[0] = kept; info[1] = n; }
}

__global__ __launch_bounds__(256) void rbs_find_hyp_kernel(const HypParams H, long h0, int n, double* __restrict__ poses)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double p[12];
    hyp_pose(H, h0 + i, p);
#pragma unroll
    for (int k = 0; k < 12; ++k) poses[(size_t)i * 12 + k] = p[k];
}

// gather: poses of the listed hypotheses
__global__ __launch_bounds__(256) void rbs_find_gather_kernel(const HypParams H, const long long* __restrict__ idx, int n,
                                                              double* __restrict__ poses)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double p[12];
    hyp_pose(H, idx[i], p);
#pragma unroll
    for (int k = 0; k < 12; ++k) poses[(size_t)i * 12 + k] = p[k];
}

// a before b: larger score first, NaN last, then smaller index
__device__ inline bool before(double sa, long long ia, double sb, long long ib)
{
    const bool na = sa != sa, nb = sb != sb;
    if (na != nb) return nb;
    if (!na && sa != sb) return sa > sb;
    return ia < ib;
}

// Block b sorts items [b C, (b+1) C) of (score, idx) -- idx == nullptr: the item's own position -- and writes
// its best k to out[b k ...].  Padding: (NaN, LLONG_MAX), which sorts after everything.
__global__ __launch_bounds__(kTopThreads) void rbs_find_topk_kernel(const double* __restrict__ score, const long long* __restrict__ idx,
                                                                    long n, int k, double* __restrict__ out_score,
                                                                    long long* __restrict__ out_idx)
{
    __shared__ double ss[kTopC];
    __shared__ long long si[kTopC];
    const long b0 = (long)blockIdx.x * kTopC;
    for (int i = threadIdx.x; i < kTopC; i += kTopThreads) {
        const long g = b0 + i;
        ss[i] = g < n ? score[g] : __builtin_nan("");
        si[i] = g < n ? (idx ? idx[g] : (long long)g) : LLONG_MAX;
    }
    __syncthreads();
    for (int size = 2; size <= kTopC; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int p = threadIdx.x; p < kTopC / 2; p += kTopThreads) {
                const int i = 2 * stride * (p / stride) + (p % stride), j = i + stride;
                const bool up = (i & size) == 0;
                const bool sw = up ? before(ss[j], si[j], ss[i], si[i]) : before(ss[i], si[i], ss[j], si[j]);
                if (sw) {
                    const double t = ss[i]; ss[i] = ss[j]; ss[j] = t;
                    const long long u = si[i]; si[i] = si[j]; si[j] = u;
                }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < k; i += kTopThreads) {
        out_score[(size_t)blockIdx.x * k + i] = ss[i];
        out_idx[(size_t)blockIdx.x * k + i] = si[i];
    }
}

// One wave.  Candidates [n] in order (poses [n][12]); kept: their positions, at most max_keep; out[0] := count.
__global__ __launch_bounds__(64) void rbs_find_nms_kernel(const double* __restrict__ poses, const double* __restrict__ score, int n,
                                                          double t2, double trace_min, int max_keep, int* __restrict__ kept,
                                                          int* __restrict__ count)
{
    __shared__ int keep_pos[kMaxSurvivors];
    const int lane = threadIdx.x;
    int nk = 0;
    for (int c = 0; c < n && nk < max_keep; ++c) {
        if (score[c] != score[c]) break;   // (NaN sorts last: nothing after it is a candidate)
        const double* P = poses + (size_t)c * 12;
        bool near = false;
        if (lane < nk) {
            const double* Q = poses + (size_t)keep_pos[lane] * 12;
            const double dx = P[9] - Q[9], dy = P[10] - Q[10], dz = P[11] - Q[11];
            const double d2 = dx * dx + dy * dy + dz * dz;
            double tr = P[0] * Q[0];
            for (int e = 1; e < 9; ++e) tr = tr + P[e] * Q[e];
            near = d2 <= t2 && tr >= trace_min;
        }
        const bool drop = __ballot(near) != 0ull;
        if (!drop) {
            if (lane == 0) keep_pos[nk] = c;
            __syncthreads();
            ++nk;
        }
    }
    for (int i = lane; i < nk; i += 64) kept[i] = keep_pos[i];
    if (lane == 0) *count = nk;
}

// the six standard normals of child j of survivor k in round `round`: Box-Muller pairs of three Philox blocks
__device__ inline void child_normals(unsigned long long seed, int round, int k, int j, double* nz)
{
#pragma unroll
    for (int pr = 0; pr < 3; ++pr) {
        const uint4 r = rbd::philox(seed, ((unsigned long long)(unsigned)round << 32) | (unsigned)k, ((unsigned long long)(unsigned)j << 2) | pr);
        const double u1 = 1.0 - rbd::u01(r.x, r.y), u2 = rbd::u01(r.z, r.w);
        const double rad = sqrt(-2.0 * log(u1));
        nz[2 * pr] = rad * cos(kTwoPi * u2);
        nz[2 * pr + 1] = rad * sin(kTwoPi * u2);
    }
}

// step 6's perturbation of the pose P by the six normals nz: o := R(sa nz[0..2]) R | t + st nz[3..5]
__device__ inline void perturb_pose(const double* __restrict__ P, const double* nz, double st, double sa, double* __restrict__ o)
{
    const double v[3] = {sa * nz[0], sa * nz[1], sa * nz[2]};
    double A[9];
    rbd::rotvec_to_matrix(v, A);
    rbd::matmul3(A, P, o);
    o[9] = P[9] + st * nz[3];
    o[10] = P[10] + st * nz[4];
    o[11] = P[11] + st * nz[5];
}

// One thread per child of round r: [S][children][12].
__global__ __launch_bounds__(256) void rbs_find_children_kernel(const double* __restrict__ surv, int S, int children, int round,
                                                                unsigned long long seed, double st, double sa,
                                                                double* __restrict__ out)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= S * children) return;
    const int k = g / children, j = g - k * children;
    const double* P = surv + (size_t)k * 12;
    double* o = out + (size_t)g * 12;
    if (j == 0) {
#pragma unroll
        for (int e = 0; e < 12; ++e) o[e] = P[e];
        return;
    }
    double nz[6];
    child_normals(seed, round, k, j, nz);
    perturb_pose(P, nz, st, sa, o);
}

// One thread per survivor: its best child (ties: lowest j; NaN never beats a number) becomes the survivor.  All children NaN:
// child 0 -- the survivor itself -- with a NaN score; the final sort then puts it last (include/rbsensor_mi355x.h, step 6).
__global__ __launch_bounds__(64) void rbs_find_select_kernel(const double* __restrict__ child, const double* __restrict__ child_score,
                                                             int S, int children, double* __restrict__ surv, double* __restrict__ surv_score)
{
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= S) return;
    int best = 0;
    double bs = child_score[(size_t)k * children];
    for (int j = 1; j < children; ++j) {
        const double s = child_score[(size_t)k * children + j];
        if (s > bs || (bs != bs && s == s)) { bs = s; best = j; }
    }
    const double* P = child + ((size_t)k * children + best) * 12;
#pragma unroll
    for (int e = 0; e < 12; ++e) surv[(size_t)k * 12 + e] = P[e];
    surv_score[k] = bs;
}

// survivors in the order of the final sort: poses and scores gathered by position
__global__ __launch_bounds__(64) void rbs_find_order_kernel(const double* __restrict__ surv, const double* __restrict__ surv_score,
                                                            const long long* __restrict__ order, int S, double* __restrict__ out_pose,
                                                            double* __restrict__ out_score)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= S) return;
    const long long k = order[i];
#pragma unroll
    for (int e = 0; e < 12; ++e) out_pose[(size_t)i * 12 + e] = surv[(size_t)k * 12 + e];
    out_score[i] = surv_score[k];
}

// candidates -> survivors: the kept positions' poses, scores and hypothesis indices
__global__ __launch_bounds__(64) void rbs_find_keep_kernel(const double* __restrict__ cand_pose, const double* __restrict__ cand_score,
                                                           const long long* __restrict__ cand_idx, const int* __restrict__ kept,
                                                           const int* __restrict__ count, double* __restrict__ surv,
                                                           double* __restrict__ surv_coarse, long long* __restrict__ surv_idx)
{
    const int i = threadIdx.x;
    if (i >= *count) return;
    const int c = kept[i];
#pragma unroll
    for (int e = 0; e < 12; ++e) surv[(size_t)i * 12 + e] = cand_pose[(size_t)c * 12 + e];
    surv_coarse[i] = cand_score[c];
    surv_idx[i] = cand_idx[c];
}

// ---------------------------------------------------------------------------- step 1b: the foreground (opt-in)
// The dominant plane of the coarse frame in inverse depth, 1 / z = a u + b v + c, and the seeding frame.  Binary64, only
// + - * / and comparisons in the order of include/rbsensor_mi355x.h (step 1b), so tests/find_fg_twin.py makes every decision
// bit for bit.  The chosen plane is a trial's three-point plane: there is no least-squares refit.
// (Named rbs_findfg_*: the rbs_find_*_kernel names are a closed list, tests/test_finder_cpu.py.)
constexpr int kFgThreads = 256;
constexpr int kFgMaxTrials = 4096;
constexpr int kFgRecord = 8;       // accepted, a, b, c, count, n_valid, trial, (pixels masked: the host's)

struct FgModel {
    double dmin, dmax;             // valid: dmin <= d <= dmax (the seed kernel's test)
    double ms, sf;                 // sigma(z) = ms + sf (z z)
};

__device__ inline bool fg_valid(const FgModel& M, double d) { return d >= M.dmin && d <= M.dmax; }
__device__ inline double fg_sigma(const FgModel& M, double z) { return M.ms + M.sf * (z * z); }

// One thread per trial t: three pixels from Philox4x32-10 (key = seed, counter words (t, 0, 0, 0xFFFFFFFF): the refinement's
// word 3 is a round <= 64), planes [t][4] := (a, b, c, void); a void trial is (0, 0, 0, 1).
__global__ __launch_bounds__(kFgThreads) void rbs_findfg_trials_kernel(const float* __restrict__ frame, int npx, int cols, const FgModel M,
                                                                       unsigned long long seed, int trials, double* __restrict__ planes)
{
    const int t = blockIdx.x * kFgThreads + threadIdx.x;
    if (t >= trials) return;
    const uint4 r = rbd::philox(seed, 0xFFFFFFFF00000000ull, (unsigned long long)(unsigned)t);
    const unsigned word[3] = {r.x, r.y, r.z};
    double u[3], v[3], d[3];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = (int)(((unsigned long long)word[k] * (unsigned long long)npx) >> 32);   // < npx
        const int row = i / cols;
        u[k] = (double)(i - row * cols);
        v[k] = (double)row;
        d[k] = (double)frame[i];
        ok = ok && fg_valid(M, d[k]);
    }
    const double D = (u[1] - u[0]) * (v[2] - v[0]) - (u[2] - u[0]) * (v[1] - v[0]);
    double a = 0.0, b = 0.0, c = 0.0;
    ok = ok && D != 0.0;
    if (ok) {
        const double q0 = 1.0 / d[0], q1 = 1.0 / d[1], q2 = 1.0 / d[2];
        a = ((q1 - q0) * (v[2] - v[0]) - (q2 - q0) * (v[1] - v[0])) / D;
        b = ((u[1] - u[0]) * (q2 - q0) - (u[2] - u[0]) * (q1 - q0)) / D;
        c = (q0 - a * u[0]) - b * v[0];
    }
    double* o = planes + 4 * (size_t)t;
    o[0] = a; o[1] = b; o[2] = c; o[3] = ok ? 0.0 : 1.0;
}

// One block per trial, pixels strided over the block: counts[t] := the valid pixels within rs sigma of trial t's plane (-1: a
// void trial).  Block `trials` counts the valid pixels: counts[trials] := n_valid.  Integer sums: exact in any order.
__global__ __launch_bounds__(kFgThreads) void rbs_findfg_count_kernel(const float* __restrict__ frame, int npx, int cols, const FgModel M,
                                                                      const double* __restrict__ planes, int trials, double rs,
                                                                      int* __restrict__ counts)
{
    __shared__ int wave_sum[kFgThreads / 64];
    const int t = blockIdx.x;
    const bool all = t == trials;
    double a = 0.0, b = 0.0, c = 0.0;
    if (!all) {
        if (planes[4 * (size_t)t + 3] != 0.0) {
            if (threadIdx.x == 0) counts[t] = -1;
            return;
        }
        a = planes[4 * (size_t)t]; b = planes[4 * (size_t)t + 1]; c = planes[4 * (size_t)t + 2];
    }
    int mine = 0;   // (lane 0 of each wave carries the wave's sum)
    for (int p0 = 0; p0 < npx; p0 += kFgThreads) {
        const int p = p0 + (int)threadIdx.x;
        bool in = false;
        if (p < npx) {
            const double d = (double)frame[p];
            in = fg_valid(M, d);
            if (in && !all) {
                const int row = p / cols;
                const double w = (a * (double)(p - row * cols) + b * (double)row) + c;
                in = w > 0.0;
                if (in) {
                    const double z = 1.0 / w;
                    in = fabs(d - z) <= rs * fg_sigma(M, z);
                }
            }
        }
        mine += __popcll(__ballot(in));
    }
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int w = 0; w < kFgThreads / 64; ++w) tot += wave_sum[w];
        counts[t] = tot;
    }
}

// One wave: the highest count, ties to the lowest trial; accepted when count >= 3 and count >= min_fraction n_valid.
// rec [kFgRecord] := accepted, a, b, c, count, n_valid, trial, 0.
__global__ __launch_bounds__(64) void rbs_findfg_best_kernel(const double* __restrict__ planes, const int* __restrict__ counts, int trials,
                                                             double min_fraction, double* __restrict__ rec)
{
    __shared__ int best_c[64], best_t[64];
    const int lane = threadIdx.x;
    int bc = INT_MIN, bt = INT_MAX;
    for (int t = lane; t < trials; t += 64) {   // (ascending t: a later equal count never replaces)
        const int c = counts[t];
        if (c > bc) { bc = c; bt = t; }
    }
    best_c[lane] = bc;
    best_t[lane] = bt;
    __syncthreads();
    if (lane != 0) return;
    for (int l = 1; l < 64; ++l)
        if (best_c[l] > bc || (best_c[l] == bc && best_t[l] < bt)) { bc = best_c[l]; bt = best_t[l]; }
    const int n_valid = counts[trials];
    const bool accepted = bc >= 3 && (double)bc >= min_fraction * (double)n_valid;
    rec[0] = accepted ? 1.0 : 0.0;
    rec[1] = planes[4 * (size_t)bt];
    rec[2] = planes[4 * (size_t)bt + 1];
    rec[3] = planes[4 * (size_t)bt + 2];
    rec[4] = (double)bc;
    rec[5] = (double)n_valid;
    rec[6] = (double)bt;
    rec[7] = 0.0;
}

// One thread per coarse pixel: the seeding frame.  A pixel keeps its depth (its bits) when the plane is not accepted, or the
// plane is behind the camera there (w <= 0), or the pixel is strictly in front: z - d > mask_sigmas sigma(z); else NaN.
__global__ __launch_bounds__(kFgThreads) void rbs_findfg_mask_kernel(const float* __restrict__ frame, int npx, int cols, const FgModel M,
                                                                     const double* __restrict__ rec, double mask_sigmas,
                                                                     float* __restrict__ out)
{
    const int p = blockIdx.x * kFgThreads + threadIdx.x;
    if (p >= npx) return;
    const float f = frame[p];
    bool keep = rec[0] == 0.0;
    if (!keep) {
        const int row = p / cols;
        const double w = (rec[1] * (double)(p - row * cols) + rec[2] * (double)row) + rec[3];
        keep = w <= 0.0;
        if (!keep) {
            const double z = 1.0 / w;
            keep = z - (double)f > mask_sigmas * fg_sigma(M, z);
        }
    }
    out[p] = keep ? f : __builtin_nanf("");
}

// ---------------------------------------------------------------------------- step 6b: the adaptive refinement (opt-in)
// Every survivor carries a symmetric 6 x 6 covariance C over (rotation vector, translation) and its lower factor L.  A round's
// children are d = L n around the survivor; after the round C is re-estimated from the perturbations of the round's best children
// (a cross-entropy step) and factored again.  Binary64; apart from the normals and the rotation of step 6 only + - * / and sqrt,
// in the order of include/rbsensor_mi355x.h (step 6b), so tests/find_refine_twin.py reproduces every covariance bit for bit
// from the device's own perturbations.  (Named rbs_findr_*: the rbs_find_*_kernel names are a closed list.)
constexpr int kRefMaxElite = 64;

struct RefineRule {
    int elite;
    double mix, shrink, jitter;
};

// Lane 0 of a wave: sL [36] := the lower Cholesky factor of sC [36] by rows (the upper part 0); a pivot that is not > 0 or not
// finite: sL := diag(sqrt(max(C_ii, jitter))), max(x, y) = x > y ? x : y.  sC and sL in LDS.
__device__ inline void factor6(const double* sC, double jitter, double* sL)
{
    double L[6][6];
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) L[i][j] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            double s = sC[6 * i + j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
            if (j == i) {
                ok = ok && s > 0.0 && s <= 1.7976931348623157e308;
                L[i][i] = sqrt(s);
            } else {
                L[i][j] = s / L[j][j];
            }
        }
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            double v = L[i][j];
            if (!ok) {
                const double c = sC[6 * i + i];
                v = i == j ? sqrt(c > jitter ? c : jitter) : 0.0;
            }
            sL[6 * i + j] = v;
        }
}

// One wave per survivor: cov [S][36] := diag(sa^2 x 3, st^2 x 3), fac [S][36] := its factor.
__global__ __launch_bounds__(64) void rbs_findr_init_kernel(double sa, double st, double jitter, double* __restrict__ cov,
                                                            double* __restrict__ fac)
{
    __shared__ double sC[36], sL[36];
    const int k = blockIdx.x, lane = threadIdx.x;
    if (lane < 36) {
        const int a = lane / 6, b = lane - 6 * a;
        const double v = a != b ? 0.0 : a < 3 ? sa * sa : st * st;
        sC[lane] = v;
        cov[(size_t)k * 36 + lane] = v;
    }
    __syncthreads();
    if (lane == 0) factor6(sC, jitter, sL);
    __syncthreads();
    if (lane < 36) fac[(size_t)k * 36 + lane] = sL[lane];
}

// One thread per child of round r through the survivors' factors fac [S][36]: out [S][children][12] and the perturbations
// dd [S][children][6] (child 0: the survivor, d = 0).  d_a = sum over b <= a, ascending, of L_ab n_b; n: step 6's normals.
__global__ __launch_bounds__(256) void rbs_findr_children_kernel(const double* __restrict__ surv, const double* __restrict__ fac, int S,
                                                                 int children, int round, unsigned long long seed,
                                                                 double* __restrict__ out, double* __restrict__ dd)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= S * children) return;
    const int k = g / children, j = g - k * children;
    const double* P = surv + (size_t)k * 12;
    double* o = out + (size_t)g * 12;
    double* od = dd + (size_t)g * 6;
    if (j == 0) {
#pragma unroll
        for (int e = 0; e < 12; ++e) o[e] = P[e];
#pragma unroll
        for (int e = 0; e < 6; ++e) od[e] = 0.0;
        return;
    }
    double nz[6], d[6];
    child_normals(seed, round, k, j, nz);
    const double* L = fac + (size_t)k * 36;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double s = L[6 * a] * nz[0];
#pragma unroll
        for (int b = 1; b <= a; ++b) s = s + L[6 * a + b] * nz[b];
        d[a] = s;
        od[a] = s;
    }
    double A[9];
    rbd::rotvec_to_matrix(d, A);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            o[3 * r + c] = A[3 * r] * P[c] + A[3 * r + 1] * P[3 + c] + A[3 * r + 2] * P[6 + c];
    o[9] = P[9] + d[3];
    o[10] = P[10] + d[4];
    o[11] = P[11] + d[5];
}

// One wave per survivor k, after the round's scores.  Lane l holds children l, l + 64, ...  The elite is taken one at a time in
// step 5's order (score descending, j ascending, NaN never): every lane's best child that comes after the last one taken, then a
// butterfly over the lanes; it ends early when no child with a number is left (m of them).  Lane 6 a + b sums M_ab = d_a d_b in
// that order, then C_ab := shrink ((1 - mix) C_ab + mix (M_ab / m)) (+ jitter on the diagonal); m == 0: C unchanged.
// cov_out [S][36] := C (cov_in may be cov_out), fac [S][36] := its factor.
__global__ __launch_bounds__(64) void rbs_findr_update_kernel(const double* __restrict__ child_score, const double* __restrict__ dd,
                                                              int children, const RefineRule U, const double* cov_in,
                                                              double* cov_out, double* __restrict__ fac)
{
    __shared__ double sC[36], sL[36];
    const int k = blockIdx.x, lane = threadIdx.x;
    const double* score = child_score + (size_t)k * children;
    const double* D = dd + (size_t)k * children * 6;
    const int a = lane < 36 ? lane / 6 : 0, b = lane < 36 ? lane - 6 * a : 0;
    double acc = 0.0;
    double ps = 0.0;
    int pj = -1, m = 0;
    for (int e = 0; e < U.elite; ++e) {
        double bs = __builtin_nan("");
        int bj = INT_MAX;                             // (NaN, INT_MAX): after every child
        for (int j = lane; j < children; j += 64) {   // (ascending j: of equal scores the first stays)
            const double s = score[j];
            if (s != s) continue;
            if (e > 0 && !before(ps, pj, s, j)) continue;
            if (before(s, j, bs, bj)) { bs = s; bj = j; }
        }
#pragma unroll
        for (int w = 1; w < 64; w <<= 1) {
            const double os = __shfl_xor(bs, w, 64);
            const int oj = __shfl_xor(bj, w, 64);
            if (before(os, oj, bs, bj)) { bs = os; bj = oj; }
        }
        if (bj == INT_MAX) break;   // (the same in every lane: no child with a number is left)
        if (lane < 36) acc = acc + D[(size_t)bj * 6 + a] * D[(size_t)bj * 6 + b];
        ps = bs;
        pj = bj;
        ++m;
    }
    if (lane < 36) {
        double c = cov_in[(size_t)k * 36 + lane];
        if (m > 0) {
            const double Mab = acc / (double)m;
            c = U.shrink * ((1.0 - U.mix) * c + U.mix * Mab);
            if (a == b) c = c + U.jitter;
        }
        sC[lane] = c;
        cov_out[(size_t)k * 36 + lane] = c;
    }
    __syncthreads();
    if (lane == 0) factor6(sC, U.jitter, sL);
    __syncthreads();
    if (lane < 36) fac[(size_t)k * 36 + lane] = sL[lane];
}

// ---------------------------------------------------------------------------- launches
// One helper per launch of a find: a stream and raw device pointers, nothing of an rbs_find.  rbs_find_run and
// rbs_find_get_stage launch through these, and so do the probes of the test build (rbsensor_probes.hip).

// the suppression's two thresholds from the parameters: |t - t'|^2 <= t2 and trace(R^T R') >= trace_min
inline void nms_thresholds(double nms_translation, double nms_angle, double* t2, double* trace_min)
{
    *t2 = nms_translation * nms_translation;
    *trace_min = 1.0 + 2.0 * std::cos(nms_angle);
}

// cells of the seed grid: the size of the seed kernel's `cells` scratch
inline size_t seed_cells(int rows, int cols, int stride)
{
    return (size_t)((rows + stride - 1) / stride) * (size_t)((cols + stride - 1) / stride);
}

// items a top-k of n items to k needs in each of its two ping-pong buffers (the first pass's output)
inline size_t topk_items(long n, int k) { return (size_t)((n + kTopC - 1) / kTopC) * (size_t)k; }

inline void launch_subsample(hipStream_t st, const float* src, int src_cols, float* dst, int rows, int cols, int f)
{
    const int cpx = rows * cols;
    hipLaunchKernelGGL(rbs_find_subsample_kernel, dim3((unsigned)((cpx + 255) / 256)), dim3(256), 0, st, src, src_cols, dst, rows, cols, f);
}

inline void launch_seeds(hipStream_t st, const float* frame, int rows, int cols, int stride, double dmin, double dmax, int max_seeds,
                         int* cells, double* seeds, int* info)
{
    hipLaunchKernelGGL(rbs_find_seed_kernel, dim3(1), dim3(kSeedThreads), 0, st, frame, rows, cols, stride, dmin, dmax, max_seeds, cells,
                       seeds, info);
}

inline void launch_hyp(hipStream_t st, const HypParams& H, long h0, int n, double* poses)
{
    hipLaunchKernelGGL(rbs_find_hyp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, H, h0, n, poses);
}

inline void launch_gather(hipStream_t st, const HypParams& H, const long long* idx, int n, double* poses)
{
    hipLaunchKernelGGL(rbs_find_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, H, idx, n, poses);
}

// The best k of (score, idx) [n] -- idx == nullptr: positions -- in passes of kTopC-item chunks until one chunk is left;
// tk_s / tk_i: the ping-pong buffers, topk_items(n, k) items each.  *out_s / *out_i: where the k results lie.
inline hipError_t launch_topk(hipStream_t st, const double* score, const long long* idx, long n, int k, double* const tk_s[2],
                              long long* const tk_i[2], const double** out_s, const long long** out_i)
{
    int buf = 0;
    while (true) {
        const long blocks = (n + kTopC - 1) / kTopC;
        hipLaunchKernelGGL(rbs_find_topk_kernel, dim3((unsigned)blocks), dim3(kTopThreads), 0, st, score, idx, n, k, tk_s[buf], tk_i[buf]);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        score = tk_s[buf];
        idx = tk_i[buf];
        buf ^= 1;
        n = blocks * k;
        if (blocks == 1) break;
    }
    *out_s = score;
    *out_i = idx;
    return hipSuccess;
}

// the suppression over candidates [n] in order, then the kept ones' poses, scores and indices gathered; count: [1]
inline void launch_nms_keep(hipStream_t st, const double* cand_pose, const double* cand_score, const long long* cand_idx, int n, double t2,
                            double trace_min, int max_keep, int* kept, int* count, double* surv, double* surv_score, long long* surv_idx)
{
    hipLaunchKernelGGL(rbs_find_nms_kernel, dim3(1), dim3(64), 0, st, cand_pose, cand_score, n, t2, trace_min, max_keep, kept, count);
    hipLaunchKernelGGL(rbs_find_keep_kernel, dim3(1), dim3(64), 0, st, cand_pose, cand_score, cand_idx, kept, count, surv, surv_score, surv_idx);
}

inline void launch_children(hipStream_t st, const double* surv, int S, int children, int round, unsigned long long seed, double sigma_t,
                            double sigma_a, double* out)
{
    const int nch = S * children;
    hipLaunchKernelGGL(rbs_find_children_kernel, dim3((unsigned)((nch + 255) / 256)), dim3(256), 0, st, surv, S, children, round, seed,
                       sigma_t, sigma_a, out);
}

inline void launch_select(hipStream_t st, const double* child, const double* child_score, int S, int children, double* surv, double* surv_score)
{
    hipLaunchKernelGGL(rbs_find_select_kernel, dim3((unsigned)((S + 63) / 64)), dim3(64), 0, st, child, child_score, S, children, surv, surv_score);
}

inline void launch_order(hipStream_t st, const double* surv, const double* surv_score, const long long* order, int S, double* out_pose,
                         double* out_score)
{
    hipLaunchKernelGGL(rbs_find_order_kernel, dim3(1), dim3(64), 0, st, surv, surv_score, order, S, out_pose, out_score);
}

// step 1b: planes [trials][4]
inline void launch_plane_trials(hipStream_t st, const float* frame, int rows, int cols, const FgModel& M, unsigned long long seed, int trials,
                                double* planes)
{
    hipLaunchKernelGGL(rbs_findfg_trials_kernel, dim3((unsigned)((trials + kFgThreads - 1) / kFgThreads)), dim3(kFgThreads), 0, st, frame,
                       rows * cols, cols, M, seed, trials, planes);
}

// counts [trials + 1]: every trial's inliers, then the valid pixels.  trials == 0: the valid pixels alone (planes unused)
inline void launch_plane_count(hipStream_t st, const float* frame, int rows, int cols, const FgModel& M, const double* planes, int trials,
                               double ransac_sigmas, int* counts)
{
    hipLaunchKernelGGL(rbs_findfg_count_kernel, dim3((unsigned)(trials + 1)), dim3(kFgThreads), 0, st, frame, rows * cols, cols, M, planes,
                       trials, ransac_sigmas, counts);
}

// rec [kFgRecord]
inline void launch_plane_best(hipStream_t st, const double* planes, const int* counts, int trials, double min_fraction, double* rec)
{
    hipLaunchKernelGGL(rbs_findfg_best_kernel, dim3(1), dim3(64), 0, st, planes, counts, trials, min_fraction, rec);
}

// out [rows * cols]: the seeding frame
inline void launch_mask(hipStream_t st, const float* frame, int rows, int cols, const FgModel& M, const double* rec, double mask_sigmas,
                        float* out)
{
    const int npx = rows * cols;
    hipLaunchKernelGGL(rbs_findfg_mask_kernel, dim3((unsigned)((npx + kFgThreads - 1) / kFgThreads)), dim3(kFgThreads), 0, st, frame, npx,
                       cols, M, rec, mask_sigmas, out);
}

// step 6b: cov [S][36], fac [S][36]
inline void launch_refine_init(hipStream_t st, int S, double sigma_a, double sigma_t, double jitter, double* cov, double* fac)
{
    hipLaunchKernelGGL(rbs_findr_init_kernel, dim3((unsigned)S), dim3(64), 0, st, sigma_a, sigma_t, jitter, cov, fac);
}

// out [S * children][12], dd [S * children][6]
inline void launch_refine_children(hipStream_t st, const double* surv, const double* fac, int S, int children, int round,
                                   unsigned long long seed, double* out, double* dd)
{
    const int nch = S * children;
    hipLaunchKernelGGL(rbs_findr_children_kernel, dim3((unsigned)((nch + 255) / 256)), dim3(256), 0, st, surv, fac, S, children, round, seed,
                       out, dd);
}

// child_score [S * children], dd [S * children][6], cov_in [S][36] -> cov_out [S][36] (may be cov_in), fac [S][36]
inline void launch_refine_update(hipStream_t st, const double* child_score, const double* dd, int S, int children, const RefineRule& U,
                                 const double* cov_in, double* cov_out, double* fac)
{
    hipLaunchKernelGGL(rbs_findr_update_kernel, dim3((unsigned)S), dim3(64), 0, st, child_score, dd, children, U, cov_in, cov_out, fac);
}

}  // namespace rbf

struct rbs_find_gate_state;          // rbsensor_find_gate.hip

struct rbs_find {
    rbs_handle* s = nullptr;          // the sensor (borrowed)
    int part = -1;                    // >= 0: the finder of that part of a sensor of several (rbsensor_find_scene.hip); -1: the sensor's one object
    rbs_find_params p{};
    rbs_handle* coarse = nullptr;     // scoring handles: coarse resolution (max_particles = batch) and the sensor's
    rbs_handle* full = nullptr;       //   (max_particles = n_survivors * children); one occlusion slot each
    int f = 1, crows = 0, ccols = 0;
    double cK[9] = {};
    double offset = 0.0;
    double t2 = 0.0, trace_min = 0.0;   // the suppression's thresholds (rbf::nms_thresholds)
    hipStream_t st = nullptr;         // = coarse->stream: every kernel of a find
    float* d_full = nullptr;          // [rows*cols] the frame
    float* d_coarse = nullptr;        // [crows*ccols]
    float* h_frame = nullptr;         // pinned staging of a host frame
    int* d_cells = nullptr;           // seed-grid compaction
    double* d_seeds = nullptr;        // [max_seeds][4]
    int* d_info = nullptr;            // [2] kept, valid  (+ [2] suppression count, [3] valid pixels of the seeding frame),
    int* h_info = nullptr;            //   then step 1b's record, kFgRecord doubles (info_bytes in all); h_info: pinned
    // step 1b (rbs_find_set_foreground): allocated when first switched on
    rbs_find_foreground fg{};         // the setting of the next find
    float* d_seedframe = nullptr;     // [crows*ccols] the seeding frame
    double* d_planes = nullptr;       // [fg_cap][4]
    int* d_counts = nullptr;          // [fg_cap + 1]
    int fg_cap = 0;
    // step 6b (rbs_find_set_refinement): allocated when first switched on
    rbs_find_refinement rf{};         // the setting of the next find
    double* d_cov = nullptr;          // [rounds + 1][S][36] the covariances entering each round, then the final ones
    double* d_fac = nullptr;          // [S][36] the current factors
    double* d_dd = nullptr;           // [rounds][S*children][6] the children's perturbations
    // the gate (rbs_find_set_gate): allocated when first switched on
    rbs_find_gate gt{};               // the setting of the next find
    rbs_find_gate_state* gs = nullptr;
    double* d_hyp = nullptr;          // [batch][12]
    int* d_zero = nullptr;            // [max(batch, S*children)] parent indices: all 0
    double* d_score = nullptr;        // [max_seeds * n_rotations] coarse scores
    double* d_tk_s[2] = {};           // top-k ping-pong
    long long* d_tk_i[2] = {};
    size_t tk_cap = 0;
    double* d_cand_pose = nullptr;    // [n_candidates][12]
    double* d_cand_score = nullptr;
    long long* d_cand_idx = nullptr;
    int* d_kept = nullptr;
    double* d_surv = nullptr;         // [S][12] current survivors
    double* d_surv_score = nullptr;   // [S]
    double* d_surv0 = nullptr;        // [S][12] after the suppression (coarse)
    double* d_surv0_score = nullptr;
    long long* d_surv0_idx = nullptr;
    double* d_child = nullptr;        // [rounds][S*children][12]
    double* d_child_score = nullptr;  // [rounds][S*children]
    double* d_final = nullptr;        // [S][12]
    double* d_final_score = nullptr;
    long long* d_final_idx = nullptr;
    hipEvent_t ev[5] = {};
    // the last find
    bool have = false;
    bool fg_ran = false;              // with step 1b
    bool rf_ran = false;              // with step 6b
    bool gt_ran = false;              // with the gate
    float gms[2] = {};                // the evidence kernel's ms: step 4b, step 7
    double plane[rbf::kFgRecord] = {};
    int n_seeds = 0, n_valid = 0, n_cand = 0, n_surv = 0;
    long n_hyp = 0;
    float ms[5] = {};
    std::string err;
};

namespace {

int32_t ffail(rbs_find* f, int32_t code, const std::string& msg) { f->err = msg; return code; }

#define RBF_HIP(f, call)                                                                                          \
    do {                                                                                                          \
        hipError_t e_ = (call);                                                                                   \
        if (e_ != hipSuccess) {                                                                                   \
            (void)hipGetLastError();                                                                              \
            (f)->err = fmt("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__);            \
            return e_ == hipErrorOutOfMemory ? RBS_ERR_OUT_OF_MEMORY : RBS_ERR_HIP;                               \
        }                                                                                                         \
    } while (0)
#define RBF_RC(f, h, call)                                                                                        \
    do {                                                                                                          \
        const int32_t rc_ = (call);                                                                               \
        if (rc_ != RBS_OK) { (f)->err = std::string("scoring handle: ") + (h)->err; return rc_; }                 \
    } while (0)

constexpr size_t info_bytes = sizeof(int) * 4 + sizeof(double) * rbf::kFgRecord;

const char* foreground_check(const rbs_find_foreground* g)
{
    if (g->plane_trials < 1 || g->plane_trials > rbf::kFgMaxTrials) return "find: plane_trials outside 1..4096";
    if (!(g->ransac_sigmas >= 0.0) || !std::isfinite(g->ransac_sigmas) || !(g->mask_sigmas >= 0.0) || !std::isfinite(g->mask_sigmas))
        return "find: ransac_sigmas and mask_sigmas must be finite and >= 0";
    if (!(g->min_inlier_fraction >= 0.0) || !(g->min_inlier_fraction <= 1.0)) return "find: min_inlier_fraction outside [0, 1]";
    return nullptr;
}

const char* refinement_check(const rbs_find_refinement* g, int children)
{
    if (g->elite < 1 || g->elite > rbf::kRefMaxElite || g->elite > children) return "find: elite outside 1..min(64, children)";
    if (!(g->mix >= 0.0) || !(g->mix <= 1.0)) return "find: mix outside [0, 1]";
    if (!(g->shrink > 0.0) || !(g->shrink <= 1.0)) return "find: shrink outside (0, 1]";
    if (!(g->jitter >= 0.0) || !std::isfinite(g->jitter)) return "find: jitter must be finite and >= 0";
    return nullptr;
}

rbf::FgModel fg_model(const rbs_find* f)
{
    return rbf::FgModel{f->p.min_depth, f->p.max_depth, f->s->cfg.model_sigma, f->s->cfg.sigma_factor};
}

const char* find_check(const rbs_find_params* p)
{
    if (!(p->coarse_downsampling == 0 || p->coarse_downsampling == 1 || p->coarse_downsampling == 2 || p->coarse_downsampling == 4))
        return "find: coarse_downsampling must be 0, 1, 2 or 4";
    if (p->seed_stride < 1 || p->seed_stride > 4096) return "find: seed_stride outside 1..4096";
    if (!(p->min_depth > 0.0) || !(p->max_depth >= p->min_depth) || !std::isfinite(p->max_depth)) return "find: need 0 < min_depth <= max_depth < inf";
    if (!(p->depth_offset < 0.0 || (p->depth_offset >= 0.0 && std::isfinite(p->depth_offset)))) return "find: depth_offset must be finite (< 0: the default)";
    if (p->max_seeds < 1 || p->max_seeds > (1 << 20)) return "find: max_seeds outside 1..2^20";
    if (p->n_rotations < 1 || p->n_rotations > (1 << 20)) return "find: n_rotations outside 1..2^20";
    if ((long long)p->max_seeds * p->n_rotations > (1LL << 31) - 1) return "find: max_seeds * n_rotations above 2^31 - 1";
    if (p->n_candidates < 1 || p->n_candidates > rbf::kMaxCandidates) return "find: n_candidates outside 1..1024";
    if (p->n_survivors < 1 || p->n_survivors > rbf::kMaxSurvivors || p->n_survivors > p->n_candidates)
        return "find: n_survivors outside 1..min(64, n_candidates)";
    if (!(p->nms_translation >= 0.0) || !std::isfinite(p->nms_translation) || !(p->nms_angle >= 0.0) || !std::isfinite(p->nms_angle))
        return "find: nms_translation and nms_angle must be finite and >= 0";
    if (p->rounds < 0 || p->rounds > 64) return "find: rounds outside 0..64";
    if (p->children < 1 || p->children > 4096) return "find: children outside 1..4096";
    if (!(p->sigma_translation >= 0.0) || !std::isfinite(p->sigma_translation) || !(p->sigma_angle >= 0.0) || !std::isfinite(p->sigma_angle))
        return "find: sigma_translation and sigma_angle must be finite and >= 0";
    if (!(p->decay > 0.0) || !(p->decay <= 1.0)) return "find: decay outside (0, 1]";
    if (p->batch < 1 || p->batch > (1 << 20)) return "find: batch outside 1..2^20";
    if (p->min_score != p->min_score) return "find: min_score is NaN";
    return nullptr;
}

// where part b's vertices and triangles begin in the sensor's concatenated arrays (elements, not coordinates)
void part_offsets(const rbs_handle* s, int b, size_t* v0, size_t* t0)
{
    *v0 = *t0 = 0;
    for (int i = 0; i < b; ++i) { *v0 += (size_t)s->cfg_vertex_counts[i]; *t0 += (size_t)s->cfg_triangle_counts[i]; }
}

// a scoring handle: the sensor's configuration at (rows, cols, K), one occlusion slot, whole planes; part >= 0: the one-body
// model made of that part of the sensor's
int32_t make_scorer(const rbs_handle* s, int part, std::string* err, int rows, int cols, const double* K, int max_particles, rbs_handle** out)
{
    rbs_config c = s->cfg;
    if (part >= 0) {
        size_t v0, t0;
        part_offsets(s, part, &v0, &t0);
        c.n_objects = 1;
        c.vertices = s->cfg_vertices.data() + 3 * v0;
        c.vertex_counts = s->cfg_vertex_counts.data() + part;
        c.triangles = s->cfg_triangles.data() + 3 * t0;
        c.triangle_counts = s->cfg_triangle_counts.data() + part;
    }
    c.rows = rows;
    c.cols = cols;
    for (int i = 0; i < 9; ++i) c.K[i] = K[i];
    c.max_particles = max_particles;
    c.n_devices = 0;
    c.device_ids = nullptr;
    c.state_slab_px = RBS_SLAB_WHOLE_PLANES;
    rbs_handle* h = new (std::nothrow) rbs_handle;
    if (!h) { *err = "find_create: out of host memory"; return RBS_ERR_OUT_OF_MEMORY; }
    h->occ_slots = 1;
    int32_t rc;
    try {
        rc = create_impl(&c, h);
    } catch (const std::exception& e) {
        h->err = e.what();
        rc = RBS_ERR_OUT_OF_MEMORY;
    }
    if (rc != RBS_OK) {
        *err = "find_create: scoring handle: " + h->err;
        release(h);
        return rc;
    }
    h->smalln_target = 1;   // one tile split whatever the call's size (that of calls of >= 2 x CUs poses)
    *out = h;
    return RBS_OK;
}

int32_t find_topk(rbs_find* f, const double* score, const long long* idx, long n, int k, const double** out_s, const long long** out_i)
{
    RBF_HIP(f, rbf::launch_topk(f->st, score, idx, n, k, f->d_tk_s, f->d_tk_i, out_s, out_i));
    return RBS_OK;
}

rbf::HypParams hyp_params(const rbs_find* f)
{
    rbf::HypParams H;
    H.seeds = f->d_seeds;
    H.n_rot = f->p.n_rotations;
    H.fx = f->cK[0]; H.fy = f->cK[4]; H.cx = f->cK[2]; H.cy = f->cK[5];
    H.offset = f->offset;
    return H;
}

// the mean distance of n vertices from their mean: the default depth_offset
double mean_vertex_distance(const double* V, size_t nv)
{
    double c[3] = {0.0, 0.0, 0.0};
    for (size_t i = 0; i < nv; ++i)
        for (int k = 0; k < 3; ++k) c[k] += V[3 * i + k];
    for (int k = 0; k < 3; ++k) c[k] /= (double)nv;
    double m = 0.0;
    for (size_t i = 0; i < nv; ++i) {
        const double dx = V[3 * i] - c[0], dy = V[3 * i + 1] - c[1], dz = V[3 * i + 2] - c[2];
        m += std::sqrt(dx * dx + dy * dy + dz * dz);
    }
    return m / (double)nv;
}

int32_t find_create_part(rbs_handle* sensor, const rbs_find_params* p, int part, rbs_find** out);
int32_t find_run(rbs_find* f, const float* frame, const float* d_frame, int32_t k, double* poses, double* scores, int32_t* n_out, int32_t* found);
// rbsensor_find_gate.hip: the gate's part of a find, and its release
int32_t gate_coarse(rbs_find* f, long h0, int nb, int batch_no);
int32_t gate_select(rbs_find* f, int nc);
int32_t gate_result(rbs_find* f, int S, int batches);
void gate_times(rbs_find* f, int batches, bool with_result);
int32_t gate_first_class(rbs_find* f, int* c0);
void gate_release(rbs_find* f);

}  // namespace

extern "C" {

void rbs_find_default_params(rbs_find_params* p)
{
    if (!p) return;
    p->coarse_downsampling = 0;
    p->seed_stride = 4;
    p->min_depth = 0.2;
    p->max_depth = 3.0;
    p->depth_offset = -1.0;
    p->max_seeds = 1024;
    p->n_rotations = 1024;
    p->n_candidates = 512;
    p->nms_translation = 0.02;
    p->nms_angle = 30.0 * M_PI / 180.0;
    p->n_survivors = 32;
    p->rounds = 8;
    p->children = 64;
    p->sigma_translation = 0.01;
    p->sigma_angle = 10.0 * M_PI / 180.0;
    p->decay = 0.6;
    p->batch = 65536;
    p->seed = 0;
    p->min_score = -INFINITY;
}

const char* rbs_find_last_error(const rbs_find* f) { return f ? f->err.c_str() : "null finder"; }

void rbs_find_destroy(rbs_find* f)
{
    if (!f) return;
    if (f->coarse) (void)hipSetDevice(f->coarse->device);
    if (f->st) (void)hipStreamSynchronize(f->st);
    for (void* q : {(void*)f->d_full, (void*)f->d_coarse, (void*)f->d_cells, (void*)f->d_seeds, (void*)f->d_info, (void*)f->d_hyp,
                    (void*)f->d_zero, (void*)f->d_score, (void*)f->d_tk_s[0], (void*)f->d_tk_s[1], (void*)f->d_tk_i[0],
                    (void*)f->d_tk_i[1], (void*)f->d_cand_pose, (void*)f->d_cand_score, (void*)f->d_cand_idx, (void*)f->d_kept,
                    (void*)f->d_surv, (void*)f->d_surv_score, (void*)f->d_surv0, (void*)f->d_surv0_score, (void*)f->d_surv0_idx,
                    (void*)f->d_child, (void*)f->d_child_score, (void*)f->d_final, (void*)f->d_final_score, (void*)f->d_final_idx,
                    (void*)f->d_seedframe, (void*)f->d_planes, (void*)f->d_counts, (void*)f->d_cov, (void*)f->d_fac, (void*)f->d_dd})
        if (q) (void)hipFree(q);
    gate_release(f);
    if (f->h_frame) (void)hipHostFree(f->h_frame);
    if (f->h_info) (void)hipHostFree(f->h_info);
    for (hipEvent_t& e : f->ev)
        if (e) (void)hipEventDestroy(e);
    if (f->coarse) release(f->coarse);
    if (f->full) release(f->full);
    delete f;
}

int32_t rbs_find_create(rbs_handle* sensor, const rbs_find_params* p, rbs_find** out)
{
    if (out) *out = nullptr;
    const char* bad = !p ? "find_create: params is NULL" : !out ? "find_create: out is NULL" : find_check(p);
    if (!bad && !sensor) bad = "find_create: sensor is NULL";
    if (bad) {
        if (sensor) sensor->err = bad; else g_create_error = bad;
        return RBS_ERR_INVALID_ARGUMENT;
    }
    if (!sensor->shards.empty() || sensor->group || sensor->peer_world > 1)
        return fail(sensor, RBS_ERR_UNSUPPORTED, "find_create: the finder runs on single-device handles only");
    if (sensor->n_bodies != 1)
        return fail(sensor, RBS_ERR_UNSUPPORTED, "find_create: the finder searches for one object (n_objects = 1)");
    return find_create_part(sensor, p, -1, out);
}

}  // extern "C"

namespace {

// rbs_find_create behind its checks; part >= 0: the finder of that part of the sensor's model alone (a scene finder's)
int32_t find_create_part(rbs_handle* sensor, const rbs_find_params* p, int part, rbs_find** out)
{
    rbs_find* f = new (std::nothrow) rbs_find;
    if (!f) return fail(sensor, RBS_ERR_OUT_OF_MEMORY, "find_create: out of host memory");
    f->s = sensor;
    f->part = part;
    f->p = *p;
    auto bail = [&](int32_t rc) { sensor->err = f->err; rbs_find_destroy(f); return rc; };
    const int rows = sensor->rows, cols = sensor->cols;
    f->f = p->coarse_downsampling;
    if (f->f == 0) f->f = cols / 4 >= 160 ? 4 : cols / 2 >= 160 ? 2 : 1;
    f->crows = rows / f->f;
    f->ccols = cols / f->f;
    if (f->crows < 1 || f->ccols < 1) { f->err = "find_create: the coarse frame would be empty"; return bail(RBS_ERR_INVALID_ARGUMENT); }
    for (int i = 0; i < 9; ++i) f->cK[i] = sensor->cfg.K[i];
    for (int i = 0; i < 6; ++i) f->cK[i] /= (double)f->f;
    {   // depth offset: mean distance of the vertices from their mean
        size_t v0 = 0, t0 = 0;
        if (part >= 0) part_offsets(sensor, part, &v0, &t0);
        const size_t nv = part >= 0 ? (size_t)sensor->cfg_vertex_counts[part] : sensor->cfg_vertices.size() / 3;
        f->offset = p->depth_offset < 0.0 ? mean_vertex_distance(sensor->cfg_vertices.data() + 3 * v0, nv) : p->depth_offset;
    }
    rbf::nms_thresholds(p->nms_translation, p->nms_angle, &f->t2, &f->trace_min);
    const int S = p->n_survivors, nch = S * p->children;
    if (int32_t rc = make_scorer(sensor, part, &f->err, f->crows, f->ccols, f->cK, p->batch, &f->coarse)) return bail(rc);
    if (int32_t rc = make_scorer(sensor, part, &f->err, rows, cols, sensor->cfg.K, nch, &f->full)) return bail(rc);
    f->st = f->coarse->stream;
    const long H = (long)p->max_seeds * p->n_rotations;
    f->tk_cap = rbf::topk_items(H, p->n_candidates) + rbf::kTopC;
    const size_t R = (size_t)std::max(1, p->rounds);
    if (hipSetDevice(sensor->device) != hipSuccess ||
        hipMalloc(&f->d_full, sizeof(float) * (size_t)rows * cols) != hipSuccess ||
        hipMalloc(&f->d_coarse, sizeof(float) * (size_t)f->crows * f->ccols) != hipSuccess ||
        hipHostMalloc(&f->h_frame, sizeof(float) * (size_t)rows * cols, hipHostMallocDefault) != hipSuccess ||
        hipMalloc(&f->d_cells, sizeof(int) * rbf::seed_cells(f->crows, f->ccols, p->seed_stride)) != hipSuccess ||
        hipMalloc(&f->d_seeds, sizeof(double) * 4 * (size_t)p->max_seeds) != hipSuccess ||
        hipMalloc(&f->d_info, info_bytes) != hipSuccess ||
        hipHostMalloc(&f->h_info, info_bytes, hipHostMallocDefault) != hipSuccess ||
        hipMalloc(&f->d_hyp, sizeof(double) * 12 * (size_t)p->batch) != hipSuccess ||
        hipMalloc(&f->d_zero, sizeof(int) * (size_t)std::max(p->batch, nch)) != hipSuccess ||
        hipMemset(f->d_zero, 0, sizeof(int) * (size_t)std::max(p->batch, nch)) != hipSuccess ||
        hipMalloc(&f->d_score, sizeof(double) * (size_t)H) != hipSuccess ||
        hipMalloc(&f->d_tk_s[0], sizeof(double) * f->tk_cap) != hipSuccess ||
        hipMalloc(&f->d_tk_s[1], sizeof(double) * f->tk_cap) != hipSuccess ||
        hipMalloc(&f->d_tk_i[0], sizeof(long long) * f->tk_cap) != hipSuccess ||
        hipMalloc(&f->d_tk_i[1], sizeof(long long) * f->tk_cap) != hipSuccess ||
        hipMalloc(&f->d_cand_pose, sizeof(double) * 12 * (size_t)p->n_candidates) != hipSuccess ||
        hipMalloc(&f->d_cand_score, sizeof(double) * (size_t)p->n_candidates) != hipSuccess ||
        hipMalloc(&f->d_cand_idx, sizeof(long long) * (size_t)p->n_candidates) != hipSuccess ||
        hipMalloc(&f->d_kept, sizeof(int) * rbf::kMaxSurvivors) != hipSuccess ||
        hipMalloc(&f->d_surv, sizeof(double) * 12 * S) != hipSuccess ||
        hipMalloc(&f->d_surv_score, sizeof(double) * S) != hipSuccess ||
        hipMalloc(&f->d_surv0, sizeof(double) * 12 * S) != hipSuccess ||
        hipMalloc(&f->d_surv0_score, sizeof(double) * S) != hipSuccess ||
        hipMalloc(&f->d_surv0_idx, sizeof(long long) * S) != hipSuccess ||
        hipMalloc(&f->d_child, sizeof(double) * 12 * (size_t)nch * R) != hipSuccess ||
        hipMalloc(&f->d_child_score, sizeof(double) * (size_t)nch * R) != hipSuccess ||
        hipMalloc(&f->d_final, sizeof(double) * 12 * S) != hipSuccess ||
        hipMalloc(&f->d_final_score, sizeof(double) * S) != hipSuccess ||
        hipMalloc(&f->d_final_idx, sizeof(long long) * S) != hipSuccess) {
        (void)hipGetLastError();
        f->err = "find_create: device or pinned memory";
        return bail(RBS_ERR_OUT_OF_MEMORY);
    }
    for (hipEvent_t& e : f->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            (void)hipGetLastError();
            f->err = "find_create: events";
            return bail(RBS_ERR_HIP);
        }
    *out = f;
    return RBS_OK;
}

// rbs_find_run; d_frame != nullptr: the frame lies on the device already (its writers finished) and `frame` is not read
int32_t find_run(rbs_find* f, const float* frame, const float* d_frame, int32_t k, double* poses, double* scores, int32_t* n_out, int32_t* found)
{
    if (k < 0 || !n_out || !found) return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_run: k < 0 or a null n_out / found");
    *n_out = 0;
    *found = 0;
    f->have = false;
    rbs_handle* s = f->s;
    const rbs_find_params& p = f->p;
    const size_t npx = (size_t)s->npx;
    RBF_HIP(f, hipSetDevice(s->device));
    if (d_frame) {   // copied below, device to device
    } else if (frame) {
        std::memcpy(f->h_frame, frame, sizeof(float) * npx);
    } else {   // the sensor's current observation, as rbs_get_observation reads it (waits for the sensor's queued work)
        if (int32_t rc = rbs_get_observation(s, f->h_frame)) return ffail(f, rc, "find_run: sensor: " + s->err);
    }
    // fresh scoring state: the first frame after rbs_reset, every index 0
    RBF_RC(f, f->coarse, rbs_reset(f->coarse));
    RBF_RC(f, f->full, rbs_reset(f->full));
    hipStream_t st = f->st;
    RBF_HIP(f, hipEventRecord(f->ev[0], st));
    if (d_frame) RBF_HIP(f, hipMemcpyAsync(f->d_full, d_frame, sizeof(float) * npx, hipMemcpyDeviceToDevice, st));
    else RBF_HIP(f, hipMemcpyAsync(f->d_full, f->h_frame, sizeof(float) * npx, hipMemcpyHostToDevice, st));
    rbf::launch_subsample(st, f->d_full, s->cols, f->d_coarse, f->crows, f->ccols, f->f);
    const bool fg = f->fg.enabled != 0;
    double* d_rec = reinterpret_cast<double*>(f->d_info + 4);
    if (fg) {   // step 1b: the seeds come from what stands in front of the dominant plane (scoring keeps the whole frames)
        const rbf::FgModel M = fg_model(f);
        const int T = f->fg.plane_trials;
        rbf::launch_plane_trials(st, f->d_coarse, f->crows, f->ccols, M, (unsigned long long)p.seed, T, f->d_planes);
        rbf::launch_plane_count(st, f->d_coarse, f->crows, f->ccols, M, f->d_planes, T, f->fg.ransac_sigmas, f->d_counts);
        rbf::launch_plane_best(st, f->d_planes, f->d_counts, T, f->fg.min_inlier_fraction, d_rec);
        rbf::launch_mask(st, f->d_coarse, f->crows, f->ccols, M, d_rec, f->fg.mask_sigmas, f->d_seedframe);
        rbf::launch_plane_count(st, f->d_seedframe, f->crows, f->ccols, M, nullptr, 0, 0.0, f->d_info + 3);
    }
    rbf::launch_seeds(st, fg ? f->d_seedframe : f->d_coarse, f->crows, f->ccols, p.seed_stride, p.min_depth, p.max_depth, p.max_seeds,
                      f->d_cells, f->d_seeds, f->d_info);
    RBF_HIP(f, hipGetLastError());
    RBF_RC(f, f->coarse, rbs_set_observation_device(f->coarse, f->d_coarse, st));
    RBF_RC(f, f->full, rbs_set_observation_device(f->full, f->d_full, st));
    RBF_HIP(f, hipMemcpyAsync(f->h_info, f->d_info, fg ? info_bytes : 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    RBF_HIP(f, hipEventRecord(f->ev[1], st));
    RBF_HIP(f, hipStreamSynchronize(st));
    f->n_seeds = f->h_info[0];
    f->n_valid = f->h_info[1];
    f->fg_ran = fg;
    f->rf_ran = false;
    const bool gate = f->gt.enabled != 0;
    f->gt_ran = gate;
    f->gms[0] = f->gms[1] = 0.f;
    for (double& v : f->plane) v = 0.0;
    if (fg) {
        std::memcpy(f->plane, f->h_info + 4, sizeof(f->plane));
        f->plane[7] = f->plane[5] - (double)f->h_info[3];   // valid coarse pixels that the seeding frame no longer has
    }
    f->n_hyp = (long)f->n_seeds * p.n_rotations;
    f->n_cand = f->n_surv = 0;
    for (float& m : f->ms) m = 0.f;
    if (f->n_seeds == 0) {
        (void)hipEventElapsedTime(&f->ms[0], f->ev[0], f->ev[1]);
        f->ms[4] = f->ms[0];
        f->have = true;
        return RBS_OK;
    }
    // coarse scores, `batch` hypotheses per launch
    const rbf::HypParams HP = hyp_params(f);
    int batches = 0;
    for (long h0 = 0; h0 < f->n_hyp; h0 += p.batch, ++batches) {
        const int nb = (int)std::min<long>(p.batch, f->n_hyp - h0);
        rbf::launch_hyp(st, HP, h0, nb, f->d_hyp);
        RBF_HIP(f, hipGetLastError());
        RBF_RC(f, f->coarse, rbs_loglikes_device(f->coarse, f->d_hyp, f->d_zero, nb, 0, f->d_score + h0, st));
        if (gate)   // step 4b: the same poses' evidence
            if (int32_t rc = gate_coarse(f, h0, nb, batches)) return rc;
    }
    RBF_HIP(f, hipEventRecord(f->ev[2], st));
    // selection: top n_candidates, then the suppression
    const int nc = (int)std::min<long>(p.n_candidates, f->n_hyp);
    const double* ts;
    const long long* ti;
    if (gate) {   // the confirmed hypotheses first
        if (int32_t rc = gate_select(f, nc)) return rc;
    } else {
        if (int32_t rc = find_topk(f, f->d_score, nullptr, f->n_hyp, nc, &ts, &ti)) return rc;
        RBF_HIP(f, hipMemcpyAsync(f->d_cand_score, ts, sizeof(double) * nc, hipMemcpyDeviceToDevice, st));
        RBF_HIP(f, hipMemcpyAsync(f->d_cand_idx, ti, sizeof(long long) * nc, hipMemcpyDeviceToDevice, st));
    }
    rbf::launch_gather(st, HP, f->d_cand_idx, nc, f->d_cand_pose);
    rbf::launch_nms_keep(st, f->d_cand_pose, f->d_cand_score, f->d_cand_idx, nc, f->t2, f->trace_min, p.n_survivors, f->d_kept,
                         f->d_info + 2, f->d_surv0, f->d_surv0_score, f->d_surv0_idx);
    RBF_HIP(f, hipGetLastError());
    RBF_HIP(f, hipMemcpyAsync(f->h_info + 2, f->d_info + 2, sizeof(int), hipMemcpyDeviceToHost, st));
    RBF_HIP(f, hipEventRecord(f->ev[3], st));
    RBF_HIP(f, hipStreamSynchronize(st));
    // candidates: those of a number (NaN sorts last)
    {
        std::vector<double> cs(nc);
        RBF_HIP(f, hipMemcpy(cs.data(), f->d_cand_score, sizeof(double) * nc, hipMemcpyDeviceToHost));
        int m = 0;
        while (m < nc && cs[m] == cs[m]) ++m;
        f->n_cand = m;
    }
    const int S = f->h_info[2];
    f->n_surv = S;
    if (S > 0) {
        RBF_HIP(f, hipMemcpyAsync(f->d_surv, f->d_surv0, sizeof(double) * 12 * S, hipMemcpyDeviceToDevice, st));
        // refinement at the sensor's resolution
        const int nch = S * p.children;
        double st_r = p.sigma_translation, sa_r = p.sigma_angle;
        const bool rf = f->rf.enabled != 0;
        const rbf::RefineRule U{f->rf.elite, f->rf.mix, f->rf.shrink, f->rf.jitter};
        const size_t cov_stride = 36 * (size_t)p.n_survivors;   // (a round's covariances: a slot of n_survivors, S of them used)
        if (rf) rbf::launch_refine_init(st, S, sa_r, st_r, U.jitter, f->d_cov, f->d_fac);
        for (int r = 0; r < p.rounds; ++r) {
            double* cp = f->d_child + (size_t)r * 12 * S * p.children;
            double* cs = f->d_child_score + (size_t)r * S * p.children;
            double* dd = rf ? f->d_dd + (size_t)r * 6 * S * p.children : nullptr;
            if (rf) rbf::launch_refine_children(st, f->d_surv, f->d_fac, S, p.children, r, (unsigned long long)p.seed, cp, dd);
            else rbf::launch_children(st, f->d_surv, S, p.children, r, (unsigned long long)p.seed, st_r, sa_r, cp);
            RBF_HIP(f, hipGetLastError());
            RBF_RC(f, f->full, rbs_loglikes_device(f->full, cp, f->d_zero, nch, 0, cs, st));
            rbf::launch_select(st, cp, cs, S, p.children, f->d_surv, f->d_surv_score);
            if (rf)   // step 6b: the covariances entering round r + 1 and their factors
                rbf::launch_refine_update(st, cs, dd, S, p.children, U, f->d_cov + (size_t)r * cov_stride, f->d_cov + (size_t)(r + 1) * cov_stride,
                                          f->d_fac);
            RBF_HIP(f, hipGetLastError());
            st_r *= p.decay;
            sa_r *= p.decay;
        }
        if (p.rounds == 0) {   // no refinement: the survivors are scored once at the sensor's resolution
            RBF_RC(f, f->full, rbs_loglikes_device(f->full, f->d_surv, f->d_zero, S, 0, f->d_surv_score, st));
        }
        if (gate) {   // step 7's evidence, and the confirmed survivors first
            if (int32_t rc = gate_result(f, S, batches)) return rc;
        } else {
            const double* fs;
            const long long* fi;
            if (int32_t rc = find_topk(f, f->d_surv_score, nullptr, S, S, &fs, &fi)) return rc;
            RBF_HIP(f, hipMemcpyAsync(f->d_final_idx, fi, sizeof(long long) * S, hipMemcpyDeviceToDevice, st));
        }
        rbf::launch_order(st, f->d_surv, f->d_surv_score, f->d_final_idx, S, f->d_final, f->d_final_score);
        RBF_HIP(f, hipGetLastError());
    }
    f->rf_ran = S > 0 && f->rf.enabled != 0;
    RBF_HIP(f, hipEventRecord(f->ev[4], st));
    RBF_HIP(f, hipStreamSynchronize(st));
    (void)hipEventElapsedTime(&f->ms[0], f->ev[0], f->ev[1]);
    (void)hipEventElapsedTime(&f->ms[1], f->ev[1], f->ev[2]);
    (void)hipEventElapsedTime(&f->ms[2], f->ev[2], f->ev[3]);
    (void)hipEventElapsedTime(&f->ms[3], f->ev[3], f->ev[4]);
    (void)hipEventElapsedTime(&f->ms[4], f->ev[0], f->ev[4]);
    if (gate) gate_times(f, batches, S > 0);
    f->have = true;
    const int K = std::min(k, S);
    if (S > 0) {
        double best = 0.0;
        RBF_HIP(f, hipMemcpy(&best, f->d_final_score, sizeof(double), hipMemcpyDeviceToHost));
        *found = best >= p.min_score ? 1 : 0;
        if (gate && f->gt.require_confirmed) {   // pose 0 must be confirmed too
            int c0 = 1;
            if (int32_t rc = gate_first_class(f, &c0)) return rc;
            if (c0 != 0) *found = 0;
        }
    }
    if (K > 0 && poses) RBF_HIP(f, hipMemcpy(poses, f->d_final, sizeof(double) * 12 * K, hipMemcpyDeviceToHost));
    if (K > 0 && scores) RBF_HIP(f, hipMemcpy(scores, f->d_final_score, sizeof(double) * K, hipMemcpyDeviceToHost));
    *n_out = K;
    return RBS_OK;
}

}  // namespace

extern "C" {

int32_t rbs_find_run(rbs_find* f, const float* frame, int32_t k, double* poses, double* scores, int32_t* n_out, int32_t* found)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    return find_run(f, frame, nullptr, k, poses, scores, n_out, found);
}

int32_t rbs_find_get_stage(rbs_find* f, int32_t stage, int32_t round, double* poses, double* scores, int64_t* indices, int64_t* n,
                           double* info)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (!n) return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_get_stage: n is NULL");
    if (!f->have) return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_get_stage: no find yet");
    RBF_HIP(f, hipSetDevice(f->s->device));
    if (info) {
        info[0] = f->crows; info[1] = f->ccols; info[2] = f->f; info[3] = (double)f->n_hyp; info[4] = f->n_valid; info[5] = f->offset;
    }
    const int S = f->n_surv, nch = S * f->p.children;
    auto fetch = [&](const void* d, void* hst, size_t bytes) -> int32_t {
        if (hst && bytes) RBF_HIP(f, hipMemcpy(hst, d, bytes, hipMemcpyDeviceToHost));
        return RBS_OK;
    };
    auto iota = [&](long m) { if (indices) for (long i = 0; i < m; ++i) indices[i] = i; };
    switch (stage) {
        case RBS_FIND_SEEDS:
            *n = f->n_seeds;
            iota(f->n_seeds);
            return fetch(f->d_seeds, poses, sizeof(double) * 4 * f->n_seeds);
        case RBS_FIND_COARSE: {
            *n = f->n_hyp;
            iota(f->n_hyp);
            if (int32_t rc = fetch(f->d_score, scores, sizeof(double) * f->n_hyp)) return rc;
            if (poses) {
                const rbf::HypParams HP = hyp_params(f);
                for (long h0 = 0; h0 < f->n_hyp; h0 += f->p.batch) {
                    const int nb = (int)std::min<long>(f->p.batch, f->n_hyp - h0);
                    rbf::launch_hyp(f->st, HP, h0, nb, f->d_hyp);
                    RBF_HIP(f, hipGetLastError());
                    RBF_HIP(f, hipMemcpyAsync(poses + (size_t)h0 * 12, f->d_hyp, sizeof(double) * 12 * nb, hipMemcpyDeviceToHost, f->st));
                }
                RBF_HIP(f, hipStreamSynchronize(f->st));
            }
            return RBS_OK;
        }
        case RBS_FIND_CANDIDATES: {
            *n = f->n_cand;
            if (int32_t rc = fetch(f->d_cand_pose, poses, sizeof(double) * 12 * f->n_cand)) return rc;
            if (int32_t rc = fetch(f->d_cand_score, scores, sizeof(double) * f->n_cand)) return rc;
            return fetch(f->d_cand_idx, indices, sizeof(long long) * f->n_cand);
        }
        case RBS_FIND_SURVIVORS: {
            *n = S;
            if (int32_t rc = fetch(f->d_surv0, poses, sizeof(double) * 12 * S)) return rc;
            if (int32_t rc = fetch(f->d_surv0_score, scores, sizeof(double) * S)) return rc;
            return fetch(f->d_surv0_idx, indices, sizeof(long long) * S);
        }
        case RBS_FIND_CHILDREN: {
            if (round < 0 || round >= f->p.rounds) return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_get_stage: round outside 0..rounds-1");
            *n = nch;
            iota(nch);
            if (int32_t rc = fetch(f->d_child + (size_t)round * 12 * nch, poses, sizeof(double) * 12 * nch)) return rc;
            return fetch(f->d_child_score + (size_t)round * nch, scores, sizeof(double) * nch);
        }
        case RBS_FIND_RESULT: {
            *n = S;
            if (int32_t rc = fetch(f->d_final, poses, sizeof(double) * 12 * S)) return rc;
            if (int32_t rc = fetch(f->d_final_score, scores, sizeof(double) * S)) return rc;
            return fetch(f->d_final_idx, indices, sizeof(long long) * S);
        }
        default:
            return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_get_stage: bad stage");
    }
}

void rbs_find_default_foreground(rbs_find_foreground* g)
{
    if (!g) return;
    g->enabled = 1;
    g->plane_trials = 256;
    g->ransac_sigmas = 2.0;
    g->mask_sigmas = 5.0;
    g->min_inlier_fraction = 0.2;
}

int32_t rbs_find_set_foreground(rbs_find* f, const rbs_find_foreground* g)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (!g || g->enabled == 0) {
        f->fg.enabled = 0;
        return RBS_OK;
    }
    if (const char* bad = foreground_check(g)) return ffail(f, RBS_ERR_INVALID_ARGUMENT, bad);
    RBF_HIP(f, hipSetDevice(f->s->device));
    if (!f->d_seedframe) RBF_HIP(f, hipMalloc(&f->d_seedframe, sizeof(float) * (size_t)f->crows * f->ccols));
    if (g->plane_trials > f->fg_cap) {   // (the old arrays may still be read by a find's kernels: none is in flight after rbs_find_run)
        double* planes = nullptr;
        int* counts = nullptr;
        hipError_t e = hipMalloc(&planes, sizeof(double) * 4 * (size_t)g->plane_trials);
        if (e == hipSuccess) e = hipMalloc(&counts, sizeof(int) * ((size_t)g->plane_trials + 1));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (planes) (void)hipFree(planes);
            return ffail(f, RBS_ERR_OUT_OF_MEMORY, "find_set_foreground: device memory");
        }
        RBF_HIP(f, hipStreamSynchronize(f->st));
        if (f->d_planes) (void)hipFree(f->d_planes);
        if (f->d_counts) (void)hipFree(f->d_counts);
        f->d_planes = planes;
        f->d_counts = counts;
        f->fg_cap = g->plane_trials;
    }
    f->fg = *g;
    f->fg.enabled = 1;
    return RBS_OK;
}

int32_t rbs_find_get_plane(rbs_find* f, double* out8)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (!out8 || !f->have) return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_get_plane: no find yet, or a null pointer");
    for (int i = 0; i < rbf::kFgRecord; ++i) out8[i] = f->plane[i];
    return RBS_OK;
}

int32_t rbs_find_get_seed_frame(rbs_find* f, float* out, int64_t* n)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (!n) return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_get_seed_frame: n is NULL");
    if (!f->have) return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_get_seed_frame: no find yet");
    *n = (int64_t)f->crows * f->ccols;
    if (!out) return RBS_OK;
    RBF_HIP(f, hipSetDevice(f->s->device));
    RBF_HIP(f, hipMemcpy(out, f->fg_ran ? f->d_seedframe : f->d_coarse, sizeof(float) * (size_t)*n, hipMemcpyDeviceToHost));
    return RBS_OK;
}

void rbs_find_default_refinement(rbs_find_refinement* g)
{
    if (!g) return;
    g->enabled = 1;
    g->elite = 8;
    g->mix = 0.5;
    g->shrink = 1.0;
    g->jitter = 1e-10;
}

int32_t rbs_find_set_refinement(rbs_find* f, const rbs_find_refinement* g)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (!g || g->enabled == 0) {
        f->rf.enabled = 0;
        return RBS_OK;
    }
    if (const char* bad = refinement_check(g, f->p.children)) return ffail(f, RBS_ERR_INVALID_ARGUMENT, bad);
    RBF_HIP(f, hipSetDevice(f->s->device));
    if (!f->d_cov) {
        const size_t S = (size_t)f->p.n_survivors, R = (size_t)f->p.rounds;
        double *cov = nullptr, *fac = nullptr, *dd = nullptr;
        hipError_t e = hipMalloc(&cov, sizeof(double) * 36 * S * (R + 1));
        if (e == hipSuccess) e = hipMalloc(&fac, sizeof(double) * 36 * S);
        if (e == hipSuccess) e = hipMalloc(&dd, sizeof(double) * 6 * S * (size_t)f->p.children * std::max<size_t>(1, R));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (cov) (void)hipFree(cov);
            if (fac) (void)hipFree(fac);
            return ffail(f, RBS_ERR_OUT_OF_MEMORY, "find_set_refinement: device memory");
        }
        f->d_cov = cov;
        f->d_fac = fac;
        f->d_dd = dd;
    }
    f->rf = *g;
    f->rf.enabled = 1;
    return RBS_OK;
}

int32_t rbs_find_get_covariance(rbs_find* f, int32_t round, double* cov, int64_t* n)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (!n) return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_get_covariance: n is NULL");
    if (!f->have || !f->rf_ran) return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_get_covariance: no find with step 6b yet");
    if (round < 0 || round > f->p.rounds) return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_get_covariance: round outside 0..rounds");
    *n = f->n_surv;
    if (!cov || f->n_surv == 0) return RBS_OK;
    RBF_HIP(f, hipSetDevice(f->s->device));
    RBF_HIP(f, hipMemcpy(cov, f->d_cov + (size_t)round * 36 * (size_t)f->p.n_survivors, sizeof(double) * 36 * (size_t)f->n_surv,
                         hipMemcpyDeviceToHost));
    return RBS_OK;
}

int32_t rbs_find_get_perturbations(rbs_find* f, int32_t round, double* d, int64_t* n)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (!n) return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_get_perturbations: n is NULL");
    if (!f->have || !f->rf_ran) return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_get_perturbations: no find with step 6b yet");
    if (round < 0 || round >= f->p.rounds) return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_get_perturbations: round outside 0..rounds-1");
    const size_t nch = (size_t)f->n_surv * (size_t)f->p.children;
    *n = (int64_t)nch;
    if (!d || nch == 0) return RBS_OK;
    RBF_HIP(f, hipSetDevice(f->s->device));
    RBF_HIP(f, hipMemcpy(d, f->d_dd + (size_t)round * 6 * nch, sizeof(double) * 6 * nch, hipMemcpyDeviceToHost));
    return RBS_OK;
}

int32_t rbs_find_stage_ms(rbs_find* f, float* out5)
{
    if (!f) return RBS_ERR_INVALID_ARGUMENT;
    if (!out5 || !f->have) return ffail(f, RBS_ERR_INVALID_ARGUMENT, "find_stage_ms: no find yet, or a null pointer");
    for (int i = 0; i < 5; ++i) out5[i] = f->ms[i];
    return RBS_OK;
}

}  // extern "C"

// The gate (rbs_find_set_gate, rbs_find_get_evidence): the rbs_findc_* kernels and what find_run calls of them.
#include "rbsensor_find_gate.hip"

// The scene finder (rbs_find_scene_*): the bodies of a model of several, over per-part finders of the above.
#include "rbsensor_find_scene.hip"
