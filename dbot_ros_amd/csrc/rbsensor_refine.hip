// rbsensor_refine.hip -- poses refined against one depth frame: the two kernels of rbs_refine_poses (the rule, operation by
// operation: include/rbsensor_mi355x.h "Poses refined against one depth frame"; host side:
// rbs_refine_api.h).  Included by rbsensor_capi.hip behind rbs_pose_planes.h: the planes, their rectangles and the owner of
// a pixel are the assess rule's.
//
// Per iteration, on the sensor's stream:
//   rbs_planes_render_kernel<true>   (rbs_pose_planes.h) one plane per (pose, body) from the device pose buffer.
//   rbs_refine_accumulate_kernel     grid (plane, part): the usable pixels of the body's rectangle, 28 binary64 sums and a
//                                    count per thread in registers, the wave's shuffle tree, the block's waves in ascending
//                                    order through LDS, one partial per block.
//   rbs_refine_solve_kernel          one wave per (pose, body): the parts folded in ascending order, the damped normal
//                                    equations by Cholesky, the clamp, the convergence test, the new pose into the pose buffer
//                                    the next iteration's render reads, one history record.
// No floating-point atomics and no order that depends on scheduling: the same inputs give the same bits.
namespace rbs {

constexpr int kRefineMaxPlanes = 64;     // n x n_objects of one call
constexpr int kRefineParts = 16;         // blocks per plane of the accumulate kernel, at most
constexpr int kRefinePartPx = 1024;      // pixels of a rectangle per part before another part is opened
constexpr int kRefineSums = 28;          // H upper (21), g (6), q

struct RefineArgs {
    PlaneSet S;               // the n x B planes of this iteration
    const float* frame;
    int rows;
    double fx, fy, cx, cy, ms, sf;
    double gate, huber, damping, max_rot, max_trans, eps_rot, eps_trans;
    int min_pixels;
    int it;                   // this iteration
    double* poses;            // [n x B][12]: read by the render, rewritten by the solve
    double* partial;          // [n x B][kRefineParts][kRefineSums]
    int* pcount;              // [n x B][kRefineParts]
    int* frozen;              // [n x B]
    rbs_refine_body* rec;     // [n x B]
    rbs_refine_history* hist; // [iters][n x B]
};

// The parts of a rectangle of `total` pixels: a rule of the rectangle alone.
__host__ __device__ inline int refine_parts(int total)
{
    const int p = (total + kRefinePartPx - 1) / kRefinePartPx;
    return p < kRefineParts ? p : kRefineParts;
}

// Body b owns pixel (x, y) of the image: its depth there.
__device__ inline bool refine_owned(const PlaneSet& S, const float* __restrict__ planes, const int4* s_rect, int b, int x, int y, double& D)
{
    float best;
    if (planes_owner(S, planes, s_rect, 0xffffffffu, x, y, y * S.cols + x, best) != b) return false;
    D = (double)best;
    return true;
}

__global__ __launch_bounds__(256) void rbs_refine_accumulate_kernel(const RefineArgs A)
{
    __shared__ int4 s_rect[kMaxBodies];
    __shared__ double s_sum[4][kRefineSums];
    __shared__ int s_cnt[4];
    const PlaneSet& S = A.S;
    const int tid = threadIdx.x, kb = blockIdx.x, part = blockIdx.y, B = S.B;
    const int k = kb / B, b = kb - k * B;
    if (A.frozen[kb]) return;
    if (tid < B) s_rect[tid] = S.rects[k * B + tid];
    __syncthreads();
    const int4 rc = s_rect[b];
    const int w = rc.z - rc.x, total = w > 0 ? w * (rc.w - rc.y) : 0;
    const int P = refine_parts(total);
    if (part >= P) return;
    const float* planes = S.planes + (size_t)k * B * S.npx;
    const double t0 = A.poses[kb * 12 + 9], t1 = A.poses[kb * 12 + 10], t2 = A.poses[kb * 12 + 11];
    double acc[kRefineSums];
#pragma unroll
    for (int j = 0; j < kRefineSums; ++j) acc[j] = 0.0;
    int cnt = 0;
    for (int p = part * 256 + tid; p < total; p += P * 256) {
        const int ly = p / w, x = rc.x + (p - ly * w), y = rc.y + ly;
        if (x < 1 || x > S.cols - 2 || y < 1 || y > A.rows - 2) continue;
        double D, Dl, Dr, Du, Dd;
        if (!refine_owned(S, planes, s_rect, b, x, y, D)) continue;
        const float yv = A.frame[y * S.cols + x];
        if (!(fabsf(yv) < INFINITY)) continue;
        const double e = (double)yv - D;
        const double sigma = A.ms + A.sf * (D * D);
        const double ae = fabs(e);
        if (!(ae <= A.gate * sigma)) continue;
        if (!refine_owned(S, planes, s_rect, b, x - 1, y, Dl) || !refine_owned(S, planes, s_rect, b, x + 1, y, Dr) ||
            !refine_owned(S, planes, s_rect, b, x, y - 1, Du) || !refine_owned(S, planes, s_rect, b, x, y + 1, Dd))
            continue;
        const double rx = ((double)x - A.cx) / A.fx, ry = ((double)y - A.cy) / A.fy;
        const double rxl = ((double)(x - 1) - A.cx) / A.fx, rxr = ((double)(x + 1) - A.cx) / A.fx;
        const double ryu = ((double)(y - 1) - A.cy) / A.fy, ryd = ((double)(y + 1) - A.cy) / A.fy;
        const double m0 = D * rx, m1 = D * ry, m2 = D;
        const double a0 = Dr * rxr - Dl * rxl, a1 = Dr * ry - Dl * ry, a2 = Dr - Dl;
        const double c0 = Dd * rx - Du * rx, c1 = Dd * ryd - Du * ryu, c2 = Dd - Du;
        double N0 = a1 * c2 - a2 * c1, N1 = a2 * c0 - a0 * c2, N2 = a0 * c1 - a1 * c0;
        if ((N0 * m0 + N1 * m1) + N2 * m2 > 0.0) { N0 = -N0; N1 = -N1; N2 = -N2; }
        const double s = sqrt((N0 * N0 + N1 * N1) + N2 * N2);
        if (!(s > 0.0)) continue;
        const double n0 = N0 / s, n1 = N1 / s, n2 = N2 / s;
        const double hs = A.huber * sigma;
        const double hw = ae <= hs ? 1.0 : hs / ae;
        const double wt = hw / (sigma * sigma);
        const double r = e * ((n0 * rx + n1 * ry) + n2);
        const double q0 = m0 - t0, q1 = m1 - t1, q2 = m2 - t2;
        double J[6];
        J[0] = q1 * n2 - q2 * n1; J[1] = q2 * n0 - q0 * n2; J[2] = q0 * n1 - q1 * n0;
        J[3] = n0; J[4] = n1; J[5] = n2;
        int o = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const double wj = wt * J[i];
#pragma unroll
            for (int j = i; j < 6; ++j) acc[o++] += wj * J[j];
            acc[21 + i] += wj * r;
        }
        acc[27] += (wt * r) * r;
        ++cnt;
    }
    // the wave's shuffle tree, then the waves in ascending order
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int j = 0; j < kRefineSums; ++j) {
        double v = acc[j];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) s_sum[wave][j] = v;
    }
    for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off, 64);
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    const size_t slot = (size_t)kb * kRefineParts + part;
    if (tid < kRefineSums) A.partial[slot * kRefineSums + tid] = ((s_sum[0][tid] + s_sum[1][tid]) + s_sum[2][tid]) + s_sum[3][tid];
    if (tid == kRefineSums) A.pcount[slot] = ((s_cnt[0] + s_cnt[1]) + s_cnt[2]) + s_cnt[3];
}

// The damped normal equations of one body: delta = (H + damping diag H)^-1 g by lower Cholesky, by rows.  S: the 28 sums.
// false: a pivot that is not > 0 or not finite.
__device__ inline bool refine_solve6(const double* S, double damping, double* delta)
{
    double L[6][6];
    int o = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) L[j][i] = S[o++];      // the lower triangle holds A
    for (int i = 0; i < 6; ++i) L[i][i] = L[i][i] + damping * L[i][i];
    for (int i = 0; i < 6; ++i) {
        for (int j = 0; j <= i; ++j) {
            double s = L[i][j];
            for (int c = 0; c < j; ++c) s -= L[i][c] * L[j][c];
            if (j < i) { L[i][j] = s / L[j][j]; continue; }
            if (!(s > 0.0) || !(s < INFINITY)) return false;
            L[i][i] = sqrt(s);
        }
    }
    double yv[6];
    for (int i = 0; i < 6; ++i) {
        double s = S[21 + i];
        for (int c = 0; c < i; ++c) s -= L[i][c] * yv[c];
        yv[i] = s / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double s = yv[i];
        for (int c = i + 1; c < 6; ++c) s -= L[c][i] * delta[c];
        delta[i] = s / L[i][i];
    }
    return true;
}

// v (3 values) scaled down to length `limit` if it is longer; its length afterwards as the rule reads it.
__device__ inline double refine_clamp3(double* v, double limit)
{
    const double len = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    if (!(len > limit)) return len;
    const double f = limit / len;
    v[0] *= f; v[1] *= f; v[2] *= f;
    return limit;
}

__global__ __launch_bounds__(64) void rbs_refine_solve_kernel(const RefineArgs A)
{
    __shared__ double s_sum[kRefineSums];
    __shared__ int s_cnt;
    const int lane = threadIdx.x, kb = blockIdx.x, B = A.S.B;
    rbs_refine_history* H = A.hist + (size_t)A.it * gridDim.x + kb;
    double* pose = A.poses + (size_t)kb * 12;
    if (lane < 12) H->pose[lane] = pose[lane];
    if (A.frozen[kb]) {
        if (lane < kRefineSums) H->sums[lane] = 0.0;
        if (lane < 6) H->delta[lane] = 0.0;
        if (lane == 0) { H->count = 0; H->status = RBS_REFINE_FROZEN; }
        return;
    }
    const int4 rc = A.S.rects[kb];
    const int w = rc.z - rc.x, total = w > 0 ? w * (rc.w - rc.y) : 0;
    const int P = refine_parts(total);
    (void)B;
    if (lane < kRefineSums) {
        double s = 0.0;
        for (int p = 0; p < P; ++p) s += A.partial[((size_t)kb * kRefineParts + p) * kRefineSums + lane];
        s_sum[lane] = s;
        H->sums[lane] = s;
    }
    if (lane == kRefineSums) {
        int c = 0;
        for (int p = 0; p < P; ++p) c += A.pcount[(size_t)kb * kRefineParts + p];
        s_cnt = c;
    }
    __syncthreads();
    if (lane != 0) return;
    const int count = s_cnt;
    double delta[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int status;
    if (count < A.min_pixels) {
        status = RBS_REFINE_TOO_FEW_PIXELS;
    } else if (!refine_solve6(s_sum, A.damping, delta)) {
        status = RBS_REFINE_DEGENERATE;
        for (int i = 0; i < 6; ++i) delta[i] = 0.0;
        A.frozen[kb] = 1;
    } else {
        const double lo = refine_clamp3(delta, A.max_rot), lv = refine_clamp3(delta + 3, A.max_trans);
        double Rd[9], Rn[9];
        rbd::rotvec_to_matrix(delta, Rd);
        rbd::matmul3(Rd, pose, Rn);
        for (int i = 0; i < 9; ++i) pose[i] = Rn[i];
        for (int i = 0; i < 3; ++i) pose[9 + i] = pose[9 + i] + delta[3 + i];
        status = RBS_REFINE_MAX_ITERATIONS;
        if (lo < A.eps_rot && lv < A.eps_trans) {
            status = RBS_REFINE_CONVERGED;
            A.frozen[kb] = 1;
        }
    }
    for (int i = 0; i < 6; ++i) H->delta[i] = delta[i];
    H->count = count;
    H->status = status;
    rbs_refine_body* R = A.rec + kb;
    const double rms = count > 0 ? sqrt(s_sum[27] / (double)count) : 0.0;
    if (A.it == 0) { R->count_first = count; R->rms_first = rms; }
    R->count_last = count;
    R->rms_last = rms;
    R->iterations = A.it + 1;
    R->status = status;
}

}  // namespace rbs
