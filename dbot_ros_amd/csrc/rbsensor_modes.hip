// rbsensor_modes.hip -- the particle tracker's posterior modes (include/rbsensor_mi355x.h, "Posterior modes"): is the cloud one
// hump or several, and where are they -- an all-pairs weighted kernel density over the particles, its maxima picked greedily
// with suppression, every particle assigned to its nearest maximum, and each maximum's core averaged into a pose.  Opt-in
// (rbs_tracker_set_modes) or stateless on host arrays (rbs_pose_modes); with it off nothing here is launched.  The kernels
// read the particles and the log-weights and write ModesDev's buffers only.
//
// Rule (binary64, -ffp-contract=off), per body b, bodies independent:
//   m = max lw, e_i = exp(lw_i - m), S = sum e_i;  p_i the position delta, q_i the unit quaternion of the rotation-vector delta;
//   d2(i, j) = |p_i - p_j|^2 / h_t^2 + 4 (1 - (q_i . q_j)^2) / h_r^2
//   rho_i    = (1 / S) sum_j e_j max(0, 1 - d2(i, j))
//   k_max rounds: seed = the candidate (e_i > 0, not suppressed) of largest rho, lowest index on a tie; every i with
//   d2(i, seed) < separation^2 is suppressed.  Every e_i > 0 belongs to the seed of smallest d2 (the earlier on a tie); a mode's
//   core is its members with d2 < 1; mass, core mass, the core's weighted mean position and mean quaternion (signs aligned
//   with the seed's) -> rotation vector with angle in [0, pi].
//
// Launches (six, on one stream):
//   rbs_modes_max_kernel     chunks of kChunk particles: the chunk's maximum log-weight
//   rbs_modes_pack_kernel    one thread per particle (256 a block, as recentre_kernel -- recentre_body's registers): m folded from
//                            the chunk maxima, e_i, and per body a 64-byte record  p / h_t (3), q (4), e.  Where the filter's
//                            re-centring is pending the pose is re-centred on a REGISTER copy by recentre_body -- the function
//                            recentre_kernel calls, so the same bits; the particles are never written.  The block's sum of e
//                            (block_sum) is its partial of S.
//   rbs_modes_density_kernel the n^2 pass.  One thread owns one i; the j's stream through LDS in tiles of 64 records which every
//                            lane reads at the same address (a broadcast); a thread accumulates in ascending j.  n / 256 blocks
//                            cannot fill the machine, so the j range is cut into parts of modes_part_len(n) records -- 64 up to
//                            1 024 particles, 256 up to 4 096, 1 024 above: a function of n alone -- one block per (i-block,
//                            part, body); the partials are folded in part order by the next kernel.
//   rbs_modes_select_kernel  one block per body: S (the pack blocks' partials in block order), rho_i, then k_max rounds of argmax
//                            with index tie-break and suppression.
//   rbs_modes_assign_kernel  chunks x bodies: nearest seed per particle, then per mode nine sums -- e of the members, e of the
//                            core, e p (3) and e sign q (4) over the core -- reduced exactly as block_sum reduces one value
//                            (post_block_sums' pattern), one partial per chunk.
//   rbs_modes_finish_kernel  the chunks' partials folded in chunk order; masses, the mean pose; the report.
// Order of every sum: fixed by n (and k_max) alone.  No floating-point atomics: two runs, frame by frame or with look-ahead,
// give the same bits.  The compiler's report (lib/resource_usage.txt) shows no scratch and no spilled register for every kernel
// here, which tests/test_tracker_modes_cpu.py asserts.
#pragma once

#include "../../include/rbsensor_mi355x.h"

namespace rbt {

constexpr int kModesMax = RBS_MODES_MAX;
constexpr int kModesTile = 64;          // records of a tile in LDS (4 KB)
constexpr int kModesRec = 8;            // doubles of a record: p / h_t (3), q (4), e
constexpr int kModesSums = 9;           // per mode and chunk: member e, core e, core e p (3), core e sign q (4)
// e_i below this counts as 0 (the header's rule): 289 orders below the heaviest particle is no belief, and with 62 binary orders of
// room above the smallest normal number the products e p and e q of the core sums stay normal -- a subnormal weight has lost
// the bits the sums' error bounds count on (a mode of such particles had its core mass right to seven digits only)
constexpr double kModesEMin = 0x1p-960;
constexpr int kModesMaxN = 65536;       // the n^2 pass: refused above (64 parts of 1 024 at most)

__host__ __device__ inline int modes_part_len(int n) { return n <= 1024 ? 64 : n <= 4096 ? 256 : 1024; }
__host__ __device__ inline int modes_split(int n) { return (n + modes_part_len(n) - 1) / modes_part_len(n); }
__host__ __device__ inline int modes_chunks(int n) { return (n + kChunk - 1) / kChunk; }
__host__ __device__ inline int modes_pack_blocks(int n) { return (n + 255) / 256; }

struct ModesDev {
    int n, parts, k_max;
    double h_t, c4, sep2;           // h_t, 4 / h_r^2, separation^2
    double* mx;          // [chunks] chunk maxima of the log-weights
    double* se;          // [pack blocks] partials of S
    double* rec;         // [parts][n][8]
    double* rho_part;    // [parts][split][n]
    double* rho;         // [parts][n]: rho_i; the selection's working copy (-1: no candidate)
    double* sel_d;       // [parts][1 + kModesMax]: S, the seeds' densities
    int* sel_i;          // [parts][1 + kModesMax]: n_modes, the seeds
    double* partials;    // [parts][chunks][kModesMax][kModesSums]
    rbs_body_modes* out; // [parts] (pinned host memory as the device addresses it, or device memory)
};

// what one population needs, in doubles (mx .. partials, in that order) and ints
inline size_t modes_doubles(int n, int parts)
{
    return (size_t)modes_chunks(n) + modes_pack_blocks(n) + (size_t)parts * n * kModesRec + (size_t)parts * modes_split(n) * n + (size_t)parts * n +
           (size_t)parts * (1 + kModesMax) + (size_t)parts * modes_chunks(n) * kModesMax * kModesSums;
}
inline size_t modes_ints(int parts) { return (size_t)parts * (1 + kModesMax); }
inline void modes_carve(ModesDev& M, double* d, int* i)
{
    const int n = M.n, parts = M.parts;
    M.mx = d;                d += modes_chunks(n);
    M.se = d;                d += modes_pack_blocks(n);
    M.rec = d;               d += (size_t)parts * n * kModesRec;
    M.rho_part = d;          d += (size_t)parts * modes_split(n) * n;
    M.rho = d;               d += (size_t)parts * n;
    M.sel_d = d;             d += (size_t)parts * (1 + kModesMax);
    M.partials = d;
    M.sel_i = i;
}

// d2 of two records; symmetric in its arguments bit for bit
__device__ inline double modes_d2(const double* __restrict__ a, const double* __restrict__ b, double c4)
{
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    const double c = a[3] * b[3] + a[4] * b[4] + a[5] * b[5] + a[6] * b[6];
    return (dx * dx + dy * dy + dz * dz) + c4 * (1.0 - c * c);
}

__global__ __launch_bounds__(1024) void rbs_modes_max_kernel(const ModesDev M, const double* __restrict__ logw)
{
    __shared__ double sh[16];
    double m = -INFINITY;
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * kChunk + k * 1024 + (int)threadIdx.x;
        if (i < M.n) m = fmax(m, logw[i]);
    }
    m = rbd::block_max(m, sh);
    if (threadIdx.x == 0) M.mx[blockIdx.x] = m;
}

// src: particle i's body b has its six pose components at src[i stride + b bstride]; pending: re-centre them first (T.mean)
__global__ __launch_bounds__(256) void rbs_modes_pack_kernel(const ModesDev M, const TrackerDev T, const double* __restrict__ src, int stride,
                                                             int bstride, const double* __restrict__ logw, int pending)
{
    __shared__ double sh[4];
    const int i = blockIdx.x * 256 + (int)threadIdx.x;
    double m = -INFINITY;
    for (int c = 0; c < modes_chunks(M.n); ++c) m = fmax(m, M.mx[c]);
    double e = 0.0;
    if (i < M.n) {
        e = exp(logw[i] - m);
        if (e < kModesEMin) e = 0.0;
        for (int b = 0; b < M.parts; ++b) {
            double x[6];
            const double* p = src + (size_t)i * stride + (size_t)b * bstride;
#pragma unroll
            for (int k = 0; k < 6; ++k) x[k] = p[k];
            if (pending) recentre_body(T, x, b);
            const double angle = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
            const double half = 0.5 * angle;
            const double k = angle < 1e-9 ? 0.5 - angle * angle / 48.0 : sin(half) / angle;   // (rbd::rotvec_to_matrix's quaternion)
            double* r = M.rec + ((size_t)b * M.n + i) * kModesRec;
            r[0] = x[0] / M.h_t; r[1] = x[1] / M.h_t; r[2] = x[2] / M.h_t;
            r[3] = cos(half); r[4] = x[3] * k; r[5] = x[4] * k; r[6] = x[5] * k;
            r[7] = e;
        }
    }
    const double s = rbd::block_sum(e, sh);
    if (threadIdx.x == 0) M.se[blockIdx.x] = s;
}

// grid (i-blocks of 256, parts of the j range, bodies)
__global__ __launch_bounds__(256) void rbs_modes_density_kernel(const ModesDev M)
{
    __shared__ double tile[kModesTile * kModesRec];
    const int n = M.n, b = blockIdx.z, tid = threadIdx.x;
    const int i = blockIdx.x * 256 + tid;
    const double* __restrict__ rec = M.rec + (size_t)b * n * kModesRec;
    const int len = modes_part_len(n), j_lo = blockIdx.y * len, j_hi = min(n, j_lo + len);
    double a[kModesRec - 1];
    {
        const double* r = rec + (size_t)min(i, n - 1) * kModesRec;
#pragma unroll
        for (int k = 0; k < kModesRec - 1; ++k) a[k] = r[k];
    }
    const double c4 = M.c4;
    double acc = 0.0;
    for (int j0 = j_lo; j0 < j_hi; j0 += kModesTile) {
        const int cnt = min(kModesTile, j_hi - j0);
        __syncthreads();
        // 64 records = 512 doubles, two a thread
        for (int w = tid; w < cnt * kModesRec; w += 256) tile[w] = rec[(size_t)j0 * kModesRec + w];
        __syncthreads();
        for (int jj = 0; jj < cnt; ++jj) {
            const double* t = tile + jj * kModesRec;
            const double k = 1.0 - modes_d2(a, t, c4);
            acc += t[7] * fmax(0.0, k);
        }
    }
    if (i < n) M.rho_part[((size_t)b * gridDim.y + blockIdx.y) * n + i] = acc;
}

// argmax with the lowest index on a tie, over the block; every thread gets the result.  shv / shi: one per wave.
__device__ inline void modes_block_argmax(double& v, int& idx, double* shv, int* shi)
{
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(v, off, 64);
        const int oi = __shfl_down(idx, off, 64);
        if (ov > v || (ov == v && oi < idx)) { v = ov; idx = oi; }
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { shv[threadIdx.x >> 6] = v; shi[threadIdx.x >> 6] = idx; }
    __syncthreads();
    v = shv[0]; idx = shi[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
        if (shv[w] > v || (shv[w] == v && shi[w] < idx)) { v = shv[w]; idx = shi[w]; }
}

// one block per body
__global__ __launch_bounds__(1024) void rbs_modes_select_kernel(const ModesDev M)
{
    __shared__ double shv[16];
    __shared__ int shi[16];
    __shared__ double seed_rec[kModesRec];
    __shared__ double sh_S;
    const int n = M.n, b = blockIdx.x, tid = threadIdx.x;
    const int split = modes_split(n);
    const double* __restrict__ rec = M.rec + (size_t)b * n * kModesRec;
    double* __restrict__ rho = M.rho + (size_t)b * n;
    if (tid == 0) {
        double S = 0.0;
        for (int k = 0; k < modes_pack_blocks(n); ++k) S += M.se[k];
        sh_S = S;
    }
    __syncthreads();
    const double S = sh_S;
    for (int i = tid; i < n; i += 1024) {
        double sum = 0.0;
        for (int s = 0; s < split; ++s) sum += M.rho_part[((size_t)b * split + s) * n + i];
        rho[i] = rec[(size_t)i * kModesRec + 7] > 0.0 ? sum / S : -1.0;
    }
    int found = 0;
    for (int round = 0; round < M.k_max; ++round) {
        double v = -1.0;
        int idx = n;
        for (int i = tid; i < n; i += 1024)
            if (rho[i] > v) { v = rho[i]; idx = i; }      // (ascending i: the lowest index of the thread's largest)
        modes_block_argmax(v, idx, shv, shi);
        if (!(v >= 0.0)) break;                           // no candidate left (uniform over the block)
        if (tid < kModesRec) seed_rec[tid] = rec[(size_t)idx * kModesRec + tid];
        if (tid == 0) {
            M.sel_i[b * (1 + kModesMax) + 1 + round] = idx;
            M.sel_d[b * (1 + kModesMax) + 1 + round] = v;
        }
        __syncthreads();
        for (int i = tid; i < n; i += 1024)
            if (rho[i] >= 0.0 && modes_d2(rec + (size_t)i * kModesRec, seed_rec, M.c4) < M.sep2) rho[i] = -1.0;
        found = round + 1;
        __syncthreads();
    }
    if (tid == 0) {
        M.sel_i[b * (1 + kModesMax)] = found;
        M.sel_d[b * (1 + kModesMax)] = S;
    }
}

// grid (chunks, bodies): thread t of chunk c takes c kChunk + t + 1024 k, k < 4 (mean_m2_kernel's pattern)
__global__ __launch_bounds__(1024) void rbs_modes_assign_kernel(const ModesDev M)
{
    __shared__ double shb[16][kPostAcc];
    __shared__ double seeds[kModesMax * kModesRec];
    const int n = M.n, b = blockIdx.y, tid = threadIdx.x;
    const double* __restrict__ rec = M.rec + (size_t)b * n * kModesRec;
    const int K = M.sel_i[b * (1 + kModesMax)];
    if (tid < K * kModesRec) seeds[tid] = rec[(size_t)M.sel_i[b * (1 + kModesMax) + 1 + tid / kModesRec] * kModesRec + tid % kModesRec];
    __syncthreads();
    // per particle: its mode, +16 inside the core, +32 where the quaternion's sign is turned; -1: no member (e = 0, or past n)
    int tag[4];
    for (int k = 0; k < 4; ++k) {
        const int i = blockIdx.x * kChunk + k * 1024 + tid;
        tag[k] = -1;
        if (i < n && rec[(size_t)i * kModesRec + 7] > 0.0) {
            double best = INFINITY;
            int at = 0;
            for (int mode = 0; mode < K; ++mode) {
                const double d2 = modes_d2(rec + (size_t)i * kModesRec, seeds + mode * kModesRec, M.c4);
                if (d2 < best) { best = d2; at = mode; }
            }
            const double* r = rec + (size_t)i * kModesRec;
            const double* s = seeds + at * kModesRec;
            const double c = r[3] * s[3] + r[4] * s[4] + r[5] * s[5] + r[6] * s[6];
            tag[k] = at + (best < 1.0 ? 16 : 0) + (c < 0.0 ? 32 : 0);
        }
    }
    for (int mode = 0; mode < K; ++mode) {
        double a[kModesSums];
#pragma unroll
        for (int c = 0; c < kModesSums; ++c) a[c] = 0.0;
        for (int k = 0; k < 4; ++k) {
            if (tag[k] < 0 || (tag[k] & 15) != mode) continue;
            const double* r = rec + ((size_t)blockIdx.x * kChunk + k * 1024 + tid) * kModesRec;
            const double e = r[7];
            a[0] += e;
            if (tag[k] & 16) {
                const double es = tag[k] & 32 ? -e : e;
                a[1] += e;
                a[2] += e * r[0]; a[3] += e * r[1]; a[4] += e * r[2];
                a[5] += es * r[3]; a[6] += es * r[4]; a[7] += es * r[5]; a[8] += es * r[6];
            }
        }
        const double sum = post_block_sums<kModesSums>(a, shb);
        if (tid < kModesSums) M.partials[(((size_t)b * gridDim.x + blockIdx.x) * kModesMax + mode) * kModesSums + tid] = sum;
        __syncthreads();
    }
}

// one block per body, one thread per mode: the chunks' partials in chunk order; the report
__global__ __launch_bounds__(64) void rbs_modes_finish_kernel(const ModesDev M)
{
    const int b = blockIdx.x, mode = threadIdx.x, chunks = modes_chunks(M.n);
    const int K = M.sel_i[b * (1 + kModesMax)];
    rbs_body_modes* out = M.out + b;
    if (mode == 0) { out->n_modes = K; out->reserved = 0; }
    if (mode >= kModesMax) return;
    rbs_mode* o = out->mode + mode;
    if (mode >= K) {
        o->seed = -1; o->reserved = 0;
        o->density = o->mass = o->core_mass = 0.0;
        for (int k = 0; k < 6; ++k) o->delta[k] = 0.0;
        return;
    }
    const double S = M.sel_d[b * (1 + kModesMax)];
    double a[kModesSums];
    for (int c = 0; c < kModesSums; ++c) {
        double sum = 0.0;
        for (int k = 0; k < chunks; ++k) sum += M.partials[(((size_t)b * chunks + k) * kModesMax + mode) * kModesSums + c];
        a[c] = sum;
    }
    o->seed = M.sel_i[b * (1 + kModesMax) + 1 + mode];
    o->reserved = 0;
    o->density = M.sel_d[b * (1 + kModesMax) + 1 + mode];
    o->mass = a[0] / S;
    o->core_mass = a[1] / S;
    for (int k = 0; k < 3; ++k) o->delta[k] = a[2 + k] / a[1] * M.h_t;
    // the mean quaternion -- divided by the core's sum of e first: its components are then of order 1 whatever the weights' scale
    // (the squares of a sum of weights of 1e-158 underflow) -- normalised, w >= 0 -> rotation vector with angle in [0, pi]
    const double mw = a[5] / a[1], mx = a[6] / a[1], my = a[7] / a[1], mz = a[8] / a[1];
    const double qn = sqrt(mw * mw + mx * mx + my * my + mz * mz);
    double w = mw / qn, x = mx / qn, y = my / qn, z = mz / qn;
    if (w < 0.0) { w = -w; x = -x; y = -y; z = -z; }
    const double vn = sqrt(x * x + y * y + z * z);
    const double scale = vn > 0.0 ? 2.0 * atan2(vn, w) / vn : 0.0;
    o->delta[3] = x * scale; o->delta[4] = y * scale; o->delta[5] = z * scale;
}

// The six launches.  src / stride / bstride / pending: rbs_modes_pack_kernel.
inline void launch_modes(const ModesDev& M, const TrackerDev& T, const double* src, int stride, int bstride, const double* logw, int pending,
                         hipStream_t s)
{
    const unsigned chunks = (unsigned)modes_chunks(M.n), parts = (unsigned)M.parts;
    hipLaunchKernelGGL(rbs_modes_max_kernel, dim3(chunks), dim3(1024), 0, s, M, logw);
    hipLaunchKernelGGL(rbs_modes_pack_kernel, dim3((unsigned)modes_pack_blocks(M.n)), dim3(256), 0, s, M, T, src, stride, bstride, logw, pending);
    hipLaunchKernelGGL(rbs_modes_density_kernel, dim3((unsigned)modes_pack_blocks(M.n), (unsigned)modes_split(M.n), parts), dim3(256), 0, s, M);
    hipLaunchKernelGGL(rbs_modes_select_kernel, dim3(parts), dim3(1024), 0, s, M);
    hipLaunchKernelGGL(rbs_modes_assign_kernel, dim3(chunks, parts), dim3(1024), 0, s, M);
    hipLaunchKernelGGL(rbs_modes_finish_kernel, dim3(parts), dim3(64), 0, s, M);
}

}  // namespace rbt
