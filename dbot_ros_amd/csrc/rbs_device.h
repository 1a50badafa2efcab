// rbs_device.h -- device helpers that belong to no one module: rotations, the counter-based random numbers and the two
// block reductions.  Included at the top of rbsensor_kernels.hip, so every file of the translation unit behind it sees them.
// Each exists once: the sensor's pose composition, the particle tracker, its posterior report, the occlusion map, the
// Gaussian tracker and the finder all call these, and their results are compared bit for bit against the oracle and the numpy
// twins (binary64, fixed operation order, -ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace rbd {

// ------------------------------------------------------------------ rotations
// rotation vector -> row-major matrix through the unit quaternion; same formula as
// dbot_ros_amd/pose.py rotvec_to_matrix.
__device__ inline void rotvec_to_matrix(const double* rv, double* R)
{
    const double angle = sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2]);
    const double half = 0.5 * angle;
    const double k = angle < 1e-9 ? 0.5 - angle * angle / 48.0 : sin(half) / angle;
    const double w = cos(half), x = rv[0] * k, y = rv[1] * k, z = rv[2] * k;
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z); R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y); R[7] = 2.0 * (y * z + w * x); R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// matrix -> rotation vector, atan2 form (dbot_ros_amd/tracker.py _rotvecs / pose.py matrix_to_rotvec)
__device__ inline void matrix_to_rotvec(const double* R, double* rv)
{
    const double sx = 0.5 * (R[7] - R[5]), sy = 0.5 * (R[2] - R[6]), sz = 0.5 * (R[3] - R[1]);
    const double sn = sqrt(sx * sx + sy * sy + sz * sz);
    const double cs = 0.5 * ((R[0] + R[4] + R[8]) - 1.0);
    const double ang = atan2(sn, cs);
    if (sn > 1e-8 || cs > 0.0) {
        const double k = sn > 1e-8 ? ang / sn : 1.0;
        rv[0] = sx * k; rv[1] = sy * k; rv[2] = sz * k;
        return;
    }
    // angle ~ pi: the antisymmetric part vanishes, the axis comes from the symmetric part
    // (column i of R + e_i is parallel to the axis; i = the largest diagonal entry), as in
    // dbot_ros_amd/pose.py matrix_to_rotvec
    double d[3];
    for (int k = 0; k < 3; ++k) d[k] = sqrt(fmax((R[4 * k] + 1.0) * 0.5, 0.0));
    const int i = d[0] >= d[1] ? (d[0] >= d[2] ? 0 : 2) : (d[1] >= d[2] ? 1 : 2);
    double a[3];
    for (int k = 0; k < 3; ++k) a[k] = (R[3 * k + i] + (k == i ? 1.0 : 0.0)) / (2.0 * d[i]);
    const double an = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    for (int k = 0; k < 3; ++k) rv[k] = a[k] / an * ang;
}

__device__ inline void matmul3(const double* A, const double* B, double* C)
{
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c)
            C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}

// ------------------------------------------------------------------ random numbers
// Philox4x32-10 counter-based generator: (seed, frame, stream, index) -> 4 x 32 random bits.
__device__ inline uint4 philox(unsigned long long seed, unsigned long long ctr_hi, unsigned long long ctr_lo)
{
    unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    unsigned c0 = (unsigned)ctr_lo, c1 = (unsigned)(ctr_lo >> 32), c2 = (unsigned)ctr_hi, c3 = (unsigned)(ctr_hi >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return make_uint4(c0, c1, c2, c3);
}
__device__ inline double u01(unsigned hi, unsigned lo)   // 53-bit uniform in [0,1)
{
    return (double)((((unsigned long long)hi << 32) | lo) >> 11) * (1.0 / 9007199254740992.0);
}

// ------------------------------------------------------------------ block reductions
// Every thread gets the result: the shuffle tree of each wave, then the waves in ascending order.  sh: one double per wave.
__device__ inline double block_sum(double v, double* sh)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    double s = 0.0;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) s += sh[k];
    return s;
}
__device__ inline double block_max(double v, double* sh)
{
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[w] = v;
    __syncthreads();
    double s = -INFINITY;
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) s = fmax(s, sh[k]);
    return s;
}

}  // namespace rbd
