// rbs_pose_planes.h -- a set of poses drawn as depth planes, and the rule for reading such planes back.  Included by
// rbsensor_capi.hip behind rbsensor_kernels.hip (the rasterizer) and rbs_handle.h, ahead of rbsensor_assess.hip.  The
// assessor, the contour rule, the occlusion map's per-body summary, the scene finder's residual frame, the Gaussian tracker
// and the inspection hook rbs_render_depth all draw and read through this file, so that their depths and owners agree bit
// for bit by construction.
//
//   rbs_planes_render_kernel<PER_BODY>  one block row per plane; the plane's screen rectangle is cut into tiles (geometry
//                             from P) dealt to the row's blocks, tiles beyond gridDim.y strided.  Every tile goes through
//                             raster_window, culled as the raster kernel culls, so the depths are bit-identical to the
//                             oracle's orc_render.  PER_BODY: plane (k, b) = body b of pose k alone, in its own rectangle
//                             (body mask 1 << b); the minimum over b equals the plane of the whole pose.  Otherwise plane k =
//                             every body of pose k (z-min) in the pose's rectangle.  A plane is valid inside its rectangle only.
//   PlaneSet                  such planes as a reader addresses them, with the union rectangle, the owner rule and the
//                             agreement class.
#pragma once

namespace rbs {

constexpr int kPlaneTileW = 64, kPlaneTilePx = 4096;   // render tiles: small, so that a plane's rectangle spreads over blocks
constexpr int kPlaneRenderSplit = 32;                  // blocks per plane (tiles beyond it: strided)

// rects (nullable): rects[plane] := the plane's rectangle.  err (nullable): a device error word; non-zero: nothing is drawn
// (rbs_gauss_submit: the frame's prior failed).
template <bool PER_BODY>
__global__ __launch_bounds__(kBlock) void rbs_planes_render_kernel(const DevParams P, float* __restrict__ planes, int4* __restrict__ rects,
                                                                   const int* __restrict__ err)
{
    if (err && *err) return;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const Smem m = carve(smem, P.tile_px, false);
    const int kb = blockIdx.x;                // the plane: (pose, body) or pose
    const int k = PER_BODY ? kb / P.n_bodies : kb, b = kb - k * P.n_bodies;
    const double* pose = P.poses + (size_t)k * 12 * P.n_bodies;
    const Rect r = PER_BODY ? bodies_rect(P, pose, b, b + 1) : particle_rect(P, pose);
    const unsigned mask = PER_BODY ? 1u << b : 0xffffffffu;
    if (rects && blockIdx.y == 0 && threadIdx.x == 0) rects[kb] = make_int4(r.x0, r.y0, r.x1, r.y1);
    if (r.x1 <= r.x0) return;
    const TileGrid tg = tile_grid(r.x1 - r.x0, r.y1 - r.y0, P.tile_w, min(P.tile_w * P.tile_h, P.tile_px));
    const int nx = (r.x1 - r.x0 + tg.tw - 1) / tg.tw, ny = (r.y1 - r.y0 + tg.th - 1) / tg.th;
    float* out = planes + (size_t)kb * P.npx;
    for (int t = blockIdx.y; t < nx * ny; t += gridDim.y) {
        const int ty = t / nx;
        const int wx0 = r.x0 + (t - ty * nx) * tg.tw, wy0 = r.y0 + ty * tg.th;
        const int wx1 = min(r.x1, wx0 + tg.tw), wy1 = min(r.y1, wy0 + tg.th);
        const int tw = wx1 - wx0, npx = tw * (wy1 - wy0);
        raster_window(P, pose, wx0, wy0, wx1, wy1, true, m.tile, m.big, m.nbig,
                      m.evalq + (threadIdx.x >> 6) * kQPlanes * kEvalQueue, mask);
        for (int p = threadIdx.x; p < npx; p += kBlock) {
            const int lr = p / tw;
            out[(size_t)(wy0 + lr) * P.cols + wx0 + (p - lr * tw)] = __uint_as_float(m.tile[p]);
        }
        __syncthreads();
    }
}

// The n poses at d_poses ([n][n_bodies][12]) as planes on stream s, with the sensor's geometry `base` (a handle's base
// parameters): n x n_bodies planes (per_body) or n.  The caller checks hipGetLastError.
inline void launch_pose_planes(hipStream_t s, const DevParams& base, const double* d_poses, int n, bool per_body, float* planes,
                               int4* rects, const int* err)
{
    DevParams P = base;
    P.poses = d_poses;
    P.n = n;
    P.tile_w = kPlaneTileW;
    P.tile_px = kPlaneTilePx;
    P.tile_h = kPlaneTilePx / kPlaneTileW;
    const dim3 grid((unsigned)(per_body ? n * base.n_bodies : n), kPlaneRenderSplit);
    if (per_body)
        hipLaunchKernelGGL(rbs_planes_render_kernel<true>, grid, dim3(kBlock), smem_bytes(kPlaneTilePx, false), s, P, planes, rects, err);
    else
        hipLaunchKernelGGL(rbs_planes_render_kernel<false>, grid, dim3(kBlock), smem_bytes(kPlaneTilePx, false), s, P, planes, rects, err);
}

// rbs_create: the dynamic LDS both instantiations may ask for (rbs_render_depth's big tile is the largest).
inline hipError_t pose_planes_configure()
{
    for (const void* f : {reinterpret_cast<const void*>(&rbs_planes_render_kernel<true>), reinterpret_cast<const void*>(&rbs_planes_render_kernel<false>)})
        if (hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem_bytes(kTilePxBig, false))) return e;
    return hipSuccess;
}

// Per-body planes as a reader addresses them.
struct PlaneSet {
    const float* planes;      // [n x B][npx], plane (k, b) valid inside rects[k B + b]
    const int4* rects;        // [n x B]
    int cols, npx, B;
};

// The union of the rectangles (s_rect: one pose's B, staged by the caller) of the bodies in `mask` (x1 <= x0: none of them
// holds a pixel).
__device__ inline int4 planes_union_rect(const PlaneSet& S, const int4* s_rect, unsigned mask)
{
    int x0 = S.cols, y0 = S.npx, x1 = 0, y1 = 0;
    for (int b = 0; b < S.B; ++b) {
        const int4 r = s_rect[b];
        if (r.z <= r.x || !(mask >> b & 1u)) continue;   // (the mask last: see planes_owner)
        x0 = min(x0, r.x); y0 = min(y0, r.y); x1 = max(x1, r.z); y1 = max(y1, r.w);
    }
    return make_int4(x0, y0, x1, y1);
}
// The owner rule: the body of `mask` whose plane is nearest at pixel (x, y) = i among those whose rectangle holds it, a tie
// with the lowest body; -1 where no plane has a surface.  planes: the pose's B planes; best: the owner's depth.
__device__ inline int planes_owner(const PlaneSet& S, const float* __restrict__ planes, const int4* s_rect, unsigned mask, int x, int y, int i,
                                   float& best)
{
    best = INFINITY;
    int owner = -1;
    for (int b = 0; b < S.B; ++b) {     // ascending: a tie stays with the lowest body
        const int4 r = s_rect[b];       // a plane is valid inside its rectangle only
        // (the mask is tested last: tested first, the all-ones callers' loops came out in another shape than without a mask --
        // two VGPRs more in the count kernel, one in the occlusion map's -- although the test folds away)
        if (x < r.x || x >= r.z || y < r.y || y >= r.w || !(mask >> b & 1u)) continue;
        const float d = planes[(size_t)b * S.npx + i];
        if (d < best) { best = d; owner = b; }
    }
    return owner;
}
// The agreement class of a reading y against a plane's depth: tau = sigmas (ms + sf d d), r = y - d in binary64.
enum PlaneClass : int { kPlaneSupport = 0, kPlaneInFront = 1, kPlaneBehind = 2 };
__device__ inline int planes_class(float y, float depth, double sigmas, double ms, double sf)
{
    const double d = (double)depth;
    const double r = (double)y - d;
    const double tau = sigmas * (ms + sf * (d * d));
    return r < -tau ? kPlaneInFront : r > tau ? kPlaneBehind : kPlaneSupport;
}

}  // namespace rbs
