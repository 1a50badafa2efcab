// rbsensor_objmap.hip -- the posterior's object map (include/rbsensor_mi355x.h, "Object map"): per pixel
// and body the probability that a weighted particle population sees that body there, the posterior mean and variance of the
// rendered depth, and the segmentation of the staged observation against such a map.  Included by rbsensor_capi.hip behind
// rbsensor_occmap.hip: it uses that file's weight kernels as they are (rbs_occmap_weights_kernel, rbs_occmap_slots_kernel), the
// rasterizer's raster_window and bodies_rect (rbsensor_kernels.hip) and the owner rule planes_owner (rbs_pose_planes.h).
// rbs_destroy calls objmap_release, the device tracker (rbs_tracker_api.h) calls objmap::enqueue at the end of a frame.
//
// The rule.  Members i < n with pose index k_i < m and log-weight lw_i;  e_i, S, W_k as the occlusion map forms them.  A pose
// is live when W_k > 0.  d_{k,b}(p): body b of pose k alone, drawn as rbs_planes_render_kernel<true> draws it; o_k(p), d_k(p):
// planes_owner over the pose's B planes.  In binary64, -ffp-contract=off, every output float rounded once:
//   c_b(p) = sum_k W_k [o_k(p) = b],  a(p) = c_0 + c_1 + ... (ascending b),  s1 = sum_k W_k d_k,  s2 = sum_k W_k (d_k d_k)
//   cover[b][p] = (float)(c_b / S),  depth[p] = (float)(s1 / a),  var[p] = (float)max(0, s2 / a - (s1 / a)(s1 / a));
//   a = 0:  depth = +inf, var = 0.
// Nothing is written but this file's own buffers.
//
// Launches (one stream, in this order):
//   rbs_occmap_weights_kernel, rbs_occmap_slots_kernel   e_i, S, W_k (rbsensor_occmap.hip; a "slot" there is a pose here).
//   rbs_objmap_rects_kernel     one wave per (pose, body): bodies_rect of a live pose's body, the empty rectangle otherwise.
//   rbs_objmap_live_kernel      one block: the live poses in ascending k (an integer scan) and the union U of their bodies'
//                               rectangles (integer min / max).
//   rbs_objmap_render_kernel    grid: tiles of U x groups.  U is cut from its corner into tiles of kObjTileW x (tile_px / kObjTileW)
//                               pixels, tile_px = objmap_tile_px(B); the live list into G = objmap_groups(...) contiguous
//                               parts.  A block owns one tile and one part.  Per entry: the bodies whose rectangle meets the
//                               tile (block-uniform test) are drawn by raster_window, body mask 1 << b, over the WHOLE tile into
//                               the body's own LDS plane -- one pitch for every body, so planes_owner reads them as it reads
//                               planes in memory; a depth is a function of its pixel alone (every sample is tested against every
//                               triangle the cull keeps, and the cull keeps whatever may touch the window), so it is the plane
//                               kernel's bit for bit however U is cut.  Then every thread adds, for the pixels it owns
//                               (p = thread, thread + 256, ...), W_k / W_k d / W_k d d into B + 2 binary64 accumulators per
//                               pixel in LDS: ascending list order.  The block writes its partials once.
//   rbs_objmap_fold_kernel      per pixel of the frame: inside U the G partials in group order, the divisions, one rounding;
//                               outside U (or with no live pose) 0, +inf, 0.
// LDS of a render block: the rasterizer's scratch (smem_bytes(0)), B planes of tile_px floats, (B + 2) tile_px doubles:
// 74 800 bytes at B = 4 and 66 608 at B = 8 -- two blocks per CU in every case (static_assert below).
// The accumulators live in LDS: held in registers across raster_window (176 VGPRs in the plane kernel) they would spill.
//
// Segmentation (rbs_object_segment): rbs_objmap_segment_kernel labels every pixel and counts per block of 256 pixels;
// rbs_objmap_scan_kernel turns the block counts into offsets (one block, an integer scan); rbs_objmap_points_kernel writes the
// labelled pixels in ascending pixel index.  Per-body counts are integer atomics: order-free.
#pragma once

namespace rbs {

constexpr int kObjMaxBodies = 8;        // rbs_object_map: n_objects above it is RBS_ERR_UNSUPPORTED
constexpr int kObjTileW = 32;           // a render tile is kObjTileW x (tile_px / kObjTileW)
constexpr int kObjMaxGroups = 32;       // G <= this
constexpr int kObjPerGroup = 8;         // ... and no part of the live list shorter than this while G > 1
constexpr size_t kObjPartialDoubles = (size_t)4 << 20;   // 32 MiB of partial sums, or one group's worth where that is larger

__host__ __device__ constexpr int objmap_tile_px(int B) { return B <= 4 ? 1024 : 512; }
// The partial sums of one group over `tiles` tiles.
__host__ __device__ constexpr size_t objmap_group_doubles(int tiles, int B) { return (size_t)tiles * objmap_tile_px(B) * (B + 2); }
// G: a fixed function of the live count, the tiles of U and n_objects (cap: the doubles the partial buffer holds).
__host__ __device__ inline int objmap_groups(int live, int tiles, int B, size_t cap)
{
    int g = (live + kObjPerGroup - 1) / kObjPerGroup;
    if (g > kObjMaxGroups) g = kObjMaxGroups;
    const size_t fit = cap / objmap_group_doubles(tiles < 1 ? 1 : tiles, B);
    if ((size_t)g > fit) g = (int)fit;
    return g < 1 ? 1 : g;
}
__host__ __device__ constexpr int objmap_tiles(int w, int h, int B)
{
    return ((w + kObjTileW - 1) / kObjTileW) * ((h + objmap_tile_px(B) / kObjTileW - 1) / (objmap_tile_px(B) / kObjTileW));
}
constexpr size_t objmap_smem_bytes(int B)
{
    return smem_bytes(0, false) + sizeof(float) * (size_t)B * objmap_tile_px(B) + sizeof(double) * (size_t)(B + 2) * objmap_tile_px(B);
}
static_assert(smem_bytes(0, false) % 16 == 0, "the planes and the accumulators behind the rasterizer's scratch stay aligned");
static_assert(2 * ((objmap_smem_bytes(4) + 1279) / 1280 * 1280) <= 160 * 1024 && 2 * ((objmap_smem_bytes(kObjMaxBodies) + 1279) / 1280 * 1280) <= 160 * 1024,
              "two render blocks per CU: LDS is granted in 1 280-byte steps");

struct ObjArgs {
    const double* W;        // [m] per-pose weights
    int4* rects;            // [m][B] per-body rectangles (live poses; the empty rectangle otherwise)
    int* live;              // [m] the live poses, ascending
    int* head_i;            // live count, U (x0, y0, x1, y1)
    const double* head_d;   // m = max lw, S
    double* part;           // [G][tiles][B + 2][tile_px]
    size_t cap;             // doubles `part` holds
    float* cover;           // [B][npx]
    float* depth;           // [npx]
    float* var;             // [npx]
};

__global__ __launch_bounds__(256) void rbs_objmap_rects_kernel(const DevParams P, const ObjArgs A)
{
    const int kb = blockIdx.x * 4 + (threadIdx.x >> 6);   // (wave-uniform from here on: bodies_rect is a whole wave's work)
    if (kb >= P.n * P.n_bodies) return;
    const int k = kb / P.n_bodies, b = kb - k * P.n_bodies;
    int4 r = make_int4(0, 0, 0, 0);
    if (A.W[k] > 0.0) {
        const Rect q = bodies_rect(P, P.poses + (size_t)k * 12 * P.n_bodies, b, b + 1);
        r = make_int4(q.x0, q.y0, q.x1, q.y1);
    }
    if ((threadIdx.x & 63) == 0) A.rects[kb] = r;
}

__global__ __launch_bounds__(1024) void rbs_objmap_live_kernel(const DevParams P, const ObjArgs A)
{
    __shared__ int s_wave[16];
    __shared__ int s_u[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, B = P.n_bodies;
    if (tid == 0) { s_u[0] = P.cols; s_u[1] = P.rows; s_u[2] = 0; s_u[3] = 0; }
    const int per = (P.n + 1023) / 1024;
    const int k0 = min(P.n, tid * per), k1 = min(P.n, k0 + per);
    int cnt = 0;
    for (int k = k0; k < k1; ++k) cnt += A.W[k] > 0.0 ? 1 : 0;
    // exclusive scan of cnt over the block: integers, any order gives the same offsets
    int inc = cnt;
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(inc, off, 64);
        if (lane >= off) inc += v;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int at = inc - cnt, total = 0;
    for (int w = 0; w < 16; ++w) {
        if (w < wave) at += s_wave[w];
        total += s_wave[w];
    }
    for (int k = k0; k < k1; ++k) {
        if (!(A.W[k] > 0.0)) continue;
        A.live[at++] = k;
        for (int b = 0; b < B; ++b) {
            const int4 r = A.rects[k * B + b];
            if (r.z <= r.x || r.w <= r.y) continue;
            atomicMin(&s_u[0], r.x); atomicMin(&s_u[1], r.y);
            atomicMax(&s_u[2], r.z); atomicMax(&s_u[3], r.w);
        }
    }
    __syncthreads();
    if (tid == 0) {
        A.head_i[0] = total;
        A.head_i[1] = s_u[0]; A.head_i[2] = s_u[1];
        A.head_i[3] = min(s_u[2], P.cols); A.head_i[4] = min(s_u[3], P.rows);
    }
}

// What a block of the render or fold kernel knows of the launch: live count, U, its tiling, G.
struct ObjGrid { int L, x0, y0, x1, y1, nx, ny, th, G; };
__device__ inline ObjGrid objmap_grid(const ObjArgs& A, int B)
{
    ObjGrid g;
    g.L = A.head_i[0];
    g.x0 = A.head_i[1]; g.y0 = A.head_i[2]; g.x1 = A.head_i[3]; g.y1 = A.head_i[4];
    g.th = objmap_tile_px(B) / kObjTileW;
    const bool any = g.L > 0 && g.x1 > g.x0 && g.y1 > g.y0;
    g.nx = any ? (g.x1 - g.x0 + kObjTileW - 1) / kObjTileW : 0;
    g.ny = any ? (g.y1 - g.y0 + g.th - 1) / g.th : 0;
    g.G = objmap_groups(g.L, g.nx * g.ny, B, A.cap);
    return g;
}

__global__ __launch_bounds__(kBlock) void rbs_objmap_render_kernel(const DevParams P, const ObjArgs A)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int4 s_rect[kObjMaxBodies];
    const int B = P.n_bodies, T = objmap_tile_px(B), tid = threadIdx.x;
    const ObjGrid g = objmap_grid(A, B);
    const int t = blockIdx.x, grp = blockIdx.y;
    // (the whole block takes this exit or none of it does)
    if (t >= g.nx * g.ny || grp >= g.G) return;
    const Smem m = carve(smem, 0, false);
    float* planes = reinterpret_cast<float*>(smem + smem_bytes(0, false));   // [B][T]
    double* acc = reinterpret_cast<double*>(planes + (size_t)B * T);         // [B + 2][T]
    const int ty = t / g.nx;
    const int wx0 = g.x0 + (t - ty * g.nx) * kObjTileW, wy0 = g.y0 + ty * g.th;
    const int wx1 = min(g.x1, wx0 + kObjTileW), wy1 = min(g.y1, wy0 + g.th);
    const int tw = wx1 - wx0, npx = tw * (wy1 - wy0);
    for (int a = 0; a < B + 2; ++a)
        for (int p = tid; p < npx; p += kBlock) acc[a * T + p] = 0.0;   // (a thread's own pixels: no barrier between this and its sums)
    const PlaneSet S{planes, s_rect, tw, T, B};
    const int j0 = (int)((long)g.L * grp / g.G), j1 = (int)((long)g.L * (grp + 1) / g.G);
    for (int j = j0; j < j1; ++j) {
        const int k = A.live[j];
        __syncthreads();   // (the last entry's owner pass is over: its rectangles and planes may go)
        if (tid < B) s_rect[tid] = A.rects[k * B + tid];
        __syncthreads();
        unsigned meet = 0u;
        for (int b = 0; b < B; ++b) {
            const int4 r = s_rect[b];
            if (r.z > wx0 && r.x < wx1 && r.w > wy0 && r.y < wy1) meet |= 1u << b;
        }
        if (!meet) continue;
        const double* pose = P.poses + (size_t)k * 12 * B;
        for (int b = 0; b < B; ++b)
            if (meet >> b & 1u)
                raster_window(P, pose, wx0, wy0, wx1, wy1, true, reinterpret_cast<unsigned*>(planes + (size_t)b * T), m.big, m.nbig,
                              m.evalq + (tid >> 6) * kQPlanes * kEvalQueue, 1u << b);
        const double w = A.W[k];
        for (int p = tid; p < npx; p += kBlock) {
            const int ly = p / tw;
            float best;
            // (a body that was not drawn has no pixel of this tile in its rectangle: the owner rule never reads its plane)
            const int owner = planes_owner(S, planes, s_rect, 0xffffffffu, wx0 + (p - ly * tw), wy0 + ly, p, best);
            if (owner < 0) continue;
            const double d = (double)best;
            acc[owner * T + p] += w;
            acc[B * T + p] += w * d;
            acc[(B + 1) * T + p] += w * (d * d);
        }
    }
    double* out = A.part + ((size_t)grp * (g.nx * g.ny) + t) * (size_t)(B + 2) * T;
    for (int a = 0; a < B + 2; ++a)
        for (int p = tid; p < npx; p += kBlock) out[a * T + p] = acc[a * T + p];
}

__global__ __launch_bounds__(256) void rbs_objmap_fold_kernel(const DevParams P, const ObjArgs A)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P.npx) return;
    const int B = P.n_bodies, T = objmap_tile_px(B);
    const ObjGrid g = objmap_grid(A, B);
    const int y = i / P.cols, x = i - y * P.cols;
    if (g.nx == 0 || x < g.x0 || x >= g.x1 || y < g.y0 || y >= g.y1) {
        for (int b = 0; b < B; ++b) A.cover[(size_t)b * P.npx + i] = 0.f;
        A.depth[i] = INFINITY;
        A.var[i] = 0.f;
        return;
    }
    const int tx = (x - g.x0) / kObjTileW, ty = (y - g.y0) / g.th;
    const int wx0 = g.x0 + tx * kObjTileW, tw = min(g.x1, wx0 + kObjTileW) - wx0;
    const int p = (y - g.y0 - ty * g.th) * tw + (x - wx0);
    const size_t tile_stride = (size_t)(B + 2) * T, group_stride = (size_t)(g.nx * g.ny) * tile_stride;
    const double* src = A.part + (size_t)(ty * g.nx + tx) * tile_stride + p;
    const double S = A.head_d[1];
    double a = 0.0;
    for (int b = 0; b < B; ++b) {
        double c = src[(size_t)b * T];
        for (int q = 1; q < g.G; ++q) c += src[q * group_stride + (size_t)b * T];
        A.cover[(size_t)b * P.npx + i] = (float)(c / S);
        a += c;
    }
    double s1 = src[(size_t)B * T], s2 = src[(size_t)(B + 1) * T];
    for (int q = 1; q < g.G; ++q) { s1 += src[q * group_stride + (size_t)B * T]; s2 += src[q * group_stride + (size_t)(B + 1) * T]; }
    if (a > 0.0) {
        const double mu = s1 / a;
        A.depth[i] = (float)mu;
        A.var[i] = (float)fmax(0.0, s2 / a - mu * mu);
    } else {
        A.depth[i] = INFINITY;
        A.var[i] = 0.f;
    }
}

// ---- segmentation --------------------------------------------------------------------------------------------------------------
struct ObjSegArgs {
    const float* cover; const float* depth; const float* var;   // the maps
    const float* y;                                             // the observation
    double min_cover, sigmas, depth_sigmas, ms, sf;
    double fx, fy, cx, cy;
    int B, cols, npx, capacity;
    int* labels;      // [npx]
    int* block_cnt;   // [blocks + 1]: labelled pixels per block of 256; after the scan, the offsets and the total
    int* counts;      // [B], zeroed
    int* pixel;       // [capacity]
    float* xyz;       // [capacity][3]
};

__device__ inline int objmap_label(const ObjSegArgs& A, int i)
{
    int best = 0;
    float c = A.cover[i];
    for (int b = 1; b < A.B; ++b) {     // ascending, strictly greater: a tie stays with the lowest body
        const float cb = A.cover[(size_t)b * A.npx + i];
        if (cb > c) { c = cb; best = b; }
    }
    const float yv = A.y[i];
    if (!((double)c >= A.min_cover) || !(fabsf(yv) < INFINITY)) return -1;
    const double D = (double)A.depth[i];
    if (!(D < INFINITY)) return -1;     // no surface (min_cover = 0 lets such a pixel come this far)
    const double tau = A.sigmas * (A.ms + A.sf * (D * D));
    const double ex = fmax(0.0, fabs((double)yv - D) - tau);
    return ex * ex <= (A.depth_sigmas * A.depth_sigmas) * (double)A.var[i] ? best : -1;
}

__global__ __launch_bounds__(256) void rbs_objmap_segment_kernel(const ObjSegArgs A)
{
    __shared__ int s_cnt[4];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int label = i < A.npx ? objmap_label(A, i) : -1;
    if (i < A.npx) A.labels[i] = label;
    if (label >= 0) atomicAdd(A.counts + label, 1);
    const unsigned long long mask = __ballot(label >= 0);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(mask);
    __syncthreads();
    if (threadIdx.x == 0) A.block_cnt[blockIdx.x] = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
}

// block_cnt[0 .. blocks) -> exclusive offsets, block_cnt[blocks] = the total.
__global__ __launch_bounds__(1024) void rbs_objmap_scan_kernel(int* __restrict__ block_cnt, int blocks)
{
    __shared__ int s_wave[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (blocks + 1023) / 1024;
    const int b0 = min(blocks, tid * per), b1 = min(blocks, b0 + per);
    int cnt = 0;
    for (int b = b0; b < b1; ++b) cnt += block_cnt[b];
    int inc = cnt;
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(inc, off, 64);
        if (lane >= off) inc += v;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int at = inc - cnt, total = 0;
    for (int w = 0; w < 16; ++w) {
        if (w < wave) at += s_wave[w];
        total += s_wave[w];
    }
    for (int b = b0; b < b1; ++b) {
        const int c = block_cnt[b];
        block_cnt[b] = at;
        at += c;
    }
    if (tid == 0) block_cnt[blocks] = total;
}

__global__ __launch_bounds__(256) void rbs_objmap_points_kernel(const ObjSegArgs A)
{
    __shared__ int s_cnt[4];
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool on = i < A.npx && A.labels[i] >= 0;
    const unsigned long long mask = __ballot(on);
    if (lane == 0) s_cnt[wave] = __popcll(mask);
    __syncthreads();
    if (!on) return;
    int c = A.block_cnt[blockIdx.x] + __popcll(mask & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) c += s_cnt[w];
    if (c >= A.capacity) return;
    const int y = i / A.cols, x = i - y * A.cols;
    const float z = A.y[i];
    A.pixel[c] = i;
    A.xyz[3 * (size_t)c] = (float)(((double)x - A.cx) / A.fx * (double)z);
    A.xyz[3 * (size_t)c + 1] = (float)(((double)y - A.cy) / A.fy * (double)z);
    A.xyz[3 * (size_t)c + 2] = z;
}

// rbs_create: the render kernel's dynamic LDS (beside pose_planes_configure).
inline hipError_t objmap_configure()
{
    return hipFuncSetAttribute(reinterpret_cast<const void*>(&rbs_objmap_render_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)objmap_smem_bytes(4));
}

}  // namespace rbs

static_assert(rbs::objmap_smem_bytes(4) >= rbs::objmap_smem_bytes(rbs::kObjMaxBodies) && rbs::objmap_smem_bytes(4) >= rbs::objmap_smem_bytes(5),
              "objmap_configure asks for the largest block");

// What a sensor owns once an object map has been asked of it: allocated at first use, grow-only, freed by rbs_destroy.
struct rbs_objmap_state {
    int cap_n = 0, cap_m = 0;       // members / poses the buffers below hold
    int* d_idx = nullptr;           // [cap_n] a caller's pose indices (rbs_object_map)
    double* d_lw = nullptr;         // [cap_n] ... and log-weights
    double* d_e = nullptr;          // [cap_n]
    double* d_poses = nullptr;      // [cap_m][B][12] a caller's poses
    double* d_W = nullptr;          // [cap_m]
    int4* d_rects = nullptr;        // [cap_m][B]
    int* d_live = nullptr;          // [cap_m]
    int* d_head_i = nullptr;        // [8]
    double* d_head_d = nullptr;     // [2]
    double* d_part = nullptr;       // [part_cap]
    size_t part_cap = 0;
    float* d_maps = nullptr;        // [B + 2][npx]: cover, depth, var -- rbs_object_map's, and what rbs_object_segment reads
    int* d_seg = nullptr;           // labels [npx], block counts [blocks + 1], counts [B], pixel [npx]
    float* d_xyz = nullptr;         // [npx][3]
    hipEvent_t ev[2] = {nullptr, nullptr};
    float ms = 0.f;
    bool have = false;              // an rbs_object_map has run: d_maps holds its maps
    int32_t info[8] = {};           // of that call: live, U, tiles, G
};

namespace {
namespace objmap {

int seg_blocks(const rbs_handle* h) { return (h->npx + 255) / 256; }

// The doubles of partial sums a handle keeps: G = kObjMaxGroups over the whole frame, but no more than kObjPartialDoubles --
// and never less than one group over the whole frame.
size_t part_doubles(const rbs_handle* h)
{
    const size_t one = rbs::objmap_group_doubles(rbs::objmap_tiles(h->cols, h->rows, h->n_bodies), h->n_bodies);
    return std::max(one, std::min(one * rbs::kObjMaxGroups, rbs::kObjPartialDoubles));
}

// Buffers for n members over m poses (grow-only; a growth waits for the stream: its readers may be queued there).
int32_t ensure(rbs_handle* h, int n, int m)
{
    if (!h->objmap) {
        h->objmap = new (std::nothrow) rbs_objmap_state;
        if (!h->objmap) return fail(h, RBS_ERR_OUT_OF_MEMORY, "object map: out of host memory");
    }
    rbs_objmap_state* o = h->objmap;
    const size_t npx = (size_t)h->npx, B = (size_t)h->n_bodies;
    if (!o->d_head_i) RBS_HIP(h, hipMalloc(&o->d_head_i, sizeof(int) * 8));
    if (!o->d_head_d) RBS_HIP(h, hipMalloc(&o->d_head_d, sizeof(double) * 2));
    if (!o->d_part) {
        RBS_HIP(h, hipMalloc(&o->d_part, sizeof(double) * part_doubles(h)));
        o->part_cap = part_doubles(h);
    }
    if (!o->d_maps) RBS_HIP(h, hipMalloc(&o->d_maps, sizeof(float) * (B + 2) * npx));
    if (!o->d_seg) RBS_HIP(h, hipMalloc(&o->d_seg, sizeof(int) * (2 * npx + (size_t)seg_blocks(h) + 1 + B)));
    if (!o->d_xyz) RBS_HIP(h, hipMalloc(&o->d_xyz, sizeof(float) * 3 * npx));
    for (hipEvent_t& e : o->ev)
        if (!e) RBS_HIP(h, hipEventCreate(&e));
    if (n > o->cap_n) {
        RBS_HIP(h, hipStreamSynchronize(h->stream));
        (void)hipFree(o->d_idx); (void)hipFree(o->d_lw); (void)hipFree(o->d_e);
        o->d_idx = nullptr; o->d_lw = nullptr; o->d_e = nullptr;
        o->cap_n = 0;
        RBS_HIP(h, hipMalloc(&o->d_idx, sizeof(int) * (size_t)n));
        RBS_HIP(h, hipMalloc(&o->d_lw, sizeof(double) * (size_t)n));
        RBS_HIP(h, hipMalloc(&o->d_e, sizeof(double) * (size_t)n));
        o->cap_n = n;
    }
    if (m > o->cap_m) {
        RBS_HIP(h, hipStreamSynchronize(h->stream));
        (void)hipFree(o->d_poses); (void)hipFree(o->d_W); (void)hipFree(o->d_rects); (void)hipFree(o->d_live);
        o->d_poses = nullptr; o->d_W = nullptr; o->d_rects = nullptr; o->d_live = nullptr;
        o->cap_m = 0;
        RBS_HIP(h, hipMalloc(&o->d_poses, sizeof(double) * 12 * B * (size_t)m));
        RBS_HIP(h, hipMalloc(&o->d_W, sizeof(double) * (size_t)m));
        RBS_HIP(h, hipMalloc(&o->d_rects, sizeof(int4) * B * (size_t)m));
        RBS_HIP(h, hipMalloc(&o->d_live, sizeof(int) * (size_t)m));
        o->cap_m = m;
    }
    return RBS_OK;
}

// The map of the population (d_idx, d_lw -- nullptr: uniform --, n) over the m poses at d_poses into maps ([B + 2][npx] floats as
// the device addresses them: cover, depth, var), on the handle's stream.  The buffers exist (ensure).  Reads the poses and the
// mesh; writes this state's buffers and `maps` only.
int32_t enqueue(rbs_handle* h, const double* d_poses, int m, const int* d_idx, const double* d_lw, int n, float* maps)
{
    rbs_objmap_state* o = h->objmap;
    hipStream_t s = h->stream;
    const int B = h->n_bodies;
    DevParams P = h->base;
    P.poses = d_poses;
    P.n = m;
    P.tile_w = rbs::kObjTileW;
    P.tile_px = rbs::objmap_tile_px(B);
    P.tile_h = P.tile_px / P.tile_w;
    rbs::ObjArgs A{};
    A.W = o->d_W;
    A.rects = o->d_rects;
    A.live = o->d_live;
    A.head_i = o->d_head_i;
    A.head_d = o->d_head_d;
    A.part = o->d_part;
    A.cap = o->part_cap;
    A.cover = maps;
    A.depth = maps + (size_t)B * h->npx;
    A.var = A.depth + h->npx;
    hipLaunchKernelGGL(rbs::rbs_occmap_weights_kernel, dim3(1), dim3(1024), 0, s, d_lw, n, o->d_e, o->d_head_d);
    hipLaunchKernelGGL(rbs::rbs_occmap_slots_kernel, dim3((unsigned)((m + 63) / 64)), dim3(64), 0, s, d_idx, (const double*)o->d_e, n, m, o->d_W);
    hipLaunchKernelGGL(rbs::rbs_objmap_rects_kernel, dim3((unsigned)((m * B + 3) / 4)), dim3(256), 0, s, P, A);
    hipLaunchKernelGGL(rbs::rbs_objmap_live_kernel, dim3(1), dim3(1024), 0, s, P, A);
    const int tiles = rbs::objmap_tiles(h->cols, h->rows, B);
    const int groups = rbs::objmap_groups(m, 1, B, o->part_cap);   // (the most any live count <= m and any U can ask for)
    hipLaunchKernelGGL(rbs::rbs_objmap_render_kernel, dim3((unsigned)tiles, (unsigned)groups), dim3(rbs::kBlock), rbs::objmap_smem_bytes(B), s, P, A);
    hipLaunchKernelGGL(rbs::rbs_objmap_fold_kernel, dim3((unsigned)((h->npx + 255) / 256)), dim3(256), 0, s, P, A);
    RBS_HIP(h, hipGetLastError());
    return RBS_OK;
}

const char* refuse_handle(const rbs_handle* h)
{
    if (!h->shards.empty() || h->group || h->peer_world > 1) return "single-device handles only";
    if (h->n_bodies > rbs::kObjMaxBodies) return "n_objects above 8";
    return nullptr;
}

}  // namespace objmap

// rbs_destroy (the handle's device is current and its streams are idle).
void objmap_release(rbs_handle* h)
{
    rbs_objmap_state* o = h->objmap;
    if (!o) return;
    (void)hipFree(o->d_idx); (void)hipFree(o->d_lw); (void)hipFree(o->d_e);
    (void)hipFree(o->d_poses); (void)hipFree(o->d_W); (void)hipFree(o->d_rects); (void)hipFree(o->d_live);
    (void)hipFree(o->d_head_i); (void)hipFree(o->d_head_d); (void)hipFree(o->d_part);
    (void)hipFree(o->d_maps); (void)hipFree(o->d_seg); (void)hipFree(o->d_xyz);
    for (hipEvent_t e : o->ev)
        if (e) (void)hipEventDestroy(e);
    delete o;
    h->objmap = nullptr;
}

}  // namespace

extern "C" {

int32_t rbs_object_map(rbs_handle* h, const double* poses, int32_t n_poses, const int32_t* members, const double* log_weights, int32_t n,
                       float* cover, float* depth, float* var)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!poses) return fail(h, RBS_ERR_INVALID_ARGUMENT, "object_map: null pointer");
    if (n_poses < 1 || n < 1) return fail(h, RBS_ERR_INVALID_ARGUMENT, "object_map: n < 1");
    if (!members && n != n_poses) return fail(h, RBS_ERR_INVALID_ARGUMENT, "object_map: without members n must equal n_poses");
    if (const char* why = objmap::refuse_handle(h)) return fail(h, RBS_ERR_UNSUPPORTED, fmt("object_map: %s", why));
    for (int i = 0; members && i < n; ++i)
        if (members[i] < 0 || members[i] >= n_poses) return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("object_map: bad pose index %d (member %d)", members[i], i));
    if (log_weights) {
        bool any = false;
        for (int i = 0; i < n; ++i) {
            const double w = log_weights[i];
            if (std::isfinite(w)) any = true;
            else if (!(std::isinf(w) && w < 0.0))
                return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("object_map: log-weight %d is neither finite nor -inf", i));
        }
        if (!any) return fail(h, RBS_ERR_INVALID_ARGUMENT, "object_map: every log-weight is -inf");
    }
    const size_t B = (size_t)h->n_bodies, npx = (size_t)h->npx;
    for (size_t i = 0; i < (size_t)n_poses * B * 12; ++i)
        if (!std::isfinite(poses[i])) return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("object_map: pose entry %zu is not finite", i));
    RBS_REFUSE_POISONED(h);
    RBS_HIP(h, hipSetDevice(h->device));
    if (int32_t rc = objmap::ensure(h, n, n_poses)) return rc;
    rbs_objmap_state* o = h->objmap;
    hipStream_t s = h->stream;
    RBS_HIP(h, hipStreamSynchronize(s));   // (the buffers written next have no reader left)
    if (members) RBS_HIP(h, hipMemcpy(o->d_idx, members, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    else {
        std::vector<int> id((size_t)n);
        for (int i = 0; i < n; ++i) id[(size_t)i] = i;
        RBS_HIP(h, hipMemcpy(o->d_idx, id.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    }
    if (log_weights) RBS_HIP(h, hipMemcpy(o->d_lw, log_weights, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    RBS_HIP(h, hipMemcpy(o->d_poses, poses, sizeof(double) * 12 * B * (size_t)n_poses, hipMemcpyHostToDevice));
    o->have = false;
    RBS_HIP(h, hipEventRecord(o->ev[0], s));
    if (int32_t rc = objmap::enqueue(h, o->d_poses, n_poses, o->d_idx, log_weights ? o->d_lw : nullptr, n, o->d_maps)) return rc;
    RBS_HIP(h, hipEventRecord(o->ev[1], s));
    RBS_HIP(h, hipStreamSynchronize(s));
    if (cover) RBS_HIP(h, hipMemcpy(cover, o->d_maps, sizeof(float) * B * npx, hipMemcpyDeviceToHost));
    if (depth) RBS_HIP(h, hipMemcpy(depth, o->d_maps + B * npx, sizeof(float) * npx, hipMemcpyDeviceToHost));
    if (var) RBS_HIP(h, hipMemcpy(var, o->d_maps + (B + 1) * npx, sizeof(float) * npx, hipMemcpyDeviceToHost));
    int head[5];
    RBS_HIP(h, hipMemcpy(head, o->d_head_i, sizeof(head), hipMemcpyDeviceToHost));
    RBS_HIP(h, hipEventElapsedTime(&o->ms, o->ev[0], o->ev[1]));
    const bool any = head[0] > 0 && head[3] > head[1] && head[4] > head[2];
    const int tiles = any ? rbs::objmap_tiles(head[3] - head[1], head[4] - head[2], (int)B) : 0;
    for (int k = 0; k < 5; ++k) o->info[k] = head[k];
    o->info[5] = tiles;
    o->info[6] = rbs::objmap_groups(head[0], tiles, (int)B, o->part_cap);
    o->info[7] = rbs::objmap_tile_px((int)B);
    o->have = true;
    return RBS_OK;
}

int32_t rbs_object_map_ms(rbs_handle* h, float* ms)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!ms || !h->objmap || !h->objmap->have) return fail(h, RBS_ERR_INVALID_ARGUMENT, "object_map_ms: no map computed yet or a null pointer");
    *ms = h->objmap->ms;
    return RBS_OK;
}

int32_t rbs_object_map_info(rbs_handle* h, int32_t* out8)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!out8 || !h->objmap || !h->objmap->have) return fail(h, RBS_ERR_INVALID_ARGUMENT, "object_map_info: no map computed yet or a null pointer");
    for (int k = 0; k < 8; ++k) out8[k] = h->objmap->info[k];
    return RBS_OK;
}

void rbs_object_segment_default_params(rbs_object_segment_params* p)
{
    if (!p) return;
    rbs_assess_params a;
    rbs_assess_default_params(&a);
    p->min_cover = 0.5;
    p->sigmas = a.sigmas;
    p->depth_sigmas = 3.0;
    p->reserved = 0.0;
}

int32_t rbs_object_segment(rbs_handle* h, const rbs_object_segment_params* params, const float* cover, const float* depth, const float* var,
                           int32_t* labels, int32_t* counts, int32_t* pixel, float* xyz, int32_t capacity, int32_t* n_points)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    rbs_object_segment_params p;
    if (params) p = *params; else rbs_object_segment_default_params(&p);
    if (!(p.min_cover >= 0.0 && p.min_cover <= 1.0) || !(p.sigmas > 0.0) || !std::isfinite(p.sigmas) || !(p.depth_sigmas >= 0.0) || !std::isfinite(p.depth_sigmas))
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "object_segment: min_cover must lie in [0, 1], sigmas be finite and > 0, depth_sigmas finite and >= 0");
    if (capacity < 0 || (capacity > 0 && (!pixel || !xyz))) return fail(h, RBS_ERR_INVALID_ARGUMENT, "object_segment: capacity without its outputs");
    if (cover && (!depth || !var)) return fail(h, RBS_ERR_INVALID_ARGUMENT, "object_segment: cover without depth and var");
    if (const char* why = objmap::refuse_handle(h)) return fail(h, RBS_ERR_UNSUPPORTED, fmt("object_segment: %s", why));
    if (h->frames_handed == 0) return fail(h, RBS_ERR_INVALID_ARGUMENT, "object_segment: no observation has been staged");
    if (!cover && !(h->objmap && h->objmap->have)) return fail(h, RBS_ERR_INVALID_ARGUMENT, "object_segment: no rbs_object_map has run on this handle");
    RBS_REFUSE_POISONED(h);
    RBS_HIP(h, hipSetDevice(h->device));
    if (int32_t rc = objmap::ensure(h, 1, 1)) return rc;
    rbs_objmap_state* o = h->objmap;
    hipStream_t s = h->stream;
    const size_t B = (size_t)h->n_bodies, npx = (size_t)h->npx;
    if (int32_t rc = make_current(h, s)) return rc;   // the observation as rbs_get_observation reads it
    RBS_HIP(h, hipStreamSynchronize(s));
    if (cover) {
        RBS_HIP(h, hipMemcpy(o->d_maps, cover, sizeof(float) * B * npx, hipMemcpyHostToDevice));
        RBS_HIP(h, hipMemcpy(o->d_maps + B * npx, depth, sizeof(float) * npx, hipMemcpyHostToDevice));
        RBS_HIP(h, hipMemcpy(o->d_maps + (B + 1) * npx, var, sizeof(float) * npx, hipMemcpyHostToDevice));
        o->have = false;   // (rbs_object_map_ms / _info speak of maps that are no longer there)
    }
    const int blocks = objmap::seg_blocks(h);
    rbs::ObjSegArgs A{};
    A.cover = o->d_maps; A.depth = o->d_maps + B * npx; A.var = o->d_maps + (B + 1) * npx;
    A.y = obs_frame(h);
    A.min_cover = p.min_cover; A.sigmas = p.sigmas; A.depth_sigmas = p.depth_sigmas;
    A.ms = h->base.ms; A.sf = h->base.sf;
    A.fx = h->base.fx; A.fy = h->base.fy; A.cx = h->base.cx; A.cy = h->base.cy;
    A.B = (int)B; A.cols = h->cols; A.npx = h->npx;
    A.capacity = (int)std::min((size_t)capacity, npx);
    A.labels = o->d_seg;
    A.block_cnt = o->d_seg + npx;
    A.counts = A.block_cnt + blocks + 1;
    A.pixel = A.counts + B;
    A.xyz = o->d_xyz;
    RBS_HIP(h, hipMemsetAsync(A.counts, 0, sizeof(int) * B, s));
    hipLaunchKernelGGL(rbs::rbs_objmap_segment_kernel, dim3((unsigned)blocks), dim3(256), 0, s, A);
    hipLaunchKernelGGL(rbs::rbs_objmap_scan_kernel, dim3(1), dim3(1024), 0, s, A.block_cnt, blocks);
    hipLaunchKernelGGL(rbs::rbs_objmap_points_kernel, dim3((unsigned)blocks), dim3(256), 0, s, A);
    RBS_HIP(h, hipGetLastError());
    RBS_HIP(h, hipStreamSynchronize(s));
    int total = 0;
    RBS_HIP(h, hipMemcpy(&total, A.block_cnt + blocks, sizeof(int), hipMemcpyDeviceToHost));
    if (labels) RBS_HIP(h, hipMemcpy(labels, A.labels, sizeof(int) * npx, hipMemcpyDeviceToHost));
    if (counts) RBS_HIP(h, hipMemcpy(counts, A.counts, sizeof(int) * B, hipMemcpyDeviceToHost));
    const size_t take = (size_t)std::min(total, A.capacity);
    if (take) {
        RBS_HIP(h, hipMemcpy(pixel, A.pixel, sizeof(int) * take, hipMemcpyDeviceToHost));
        RBS_HIP(h, hipMemcpy(xyz, A.xyz, sizeof(float) * 3 * take, hipMemcpyDeviceToHost));
    }
    if (n_points) *n_points = total;
    return RBS_OK;
}

}  // extern "C"
