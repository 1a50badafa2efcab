// rbsensor_occmap.hip -- the posterior's occlusion map (include/rbsensor_mi355x.h, "Occlusion map"): the
// weighted mean over a particle population of the occlusion planes its members point at, reduced on the device from the planes
// as they are stored, and a per-body summary of such a map at given poses.  Included by rbsensor_capi.hip behind
// rbsensor_contour.hip: it uses the handle, the planes' storage (rbs_planes.h) and the assessor's planes (rbsensor_assess.hip);
// rbs_destroy calls occmap_release, the device tracker (rbs_tracker_api.h) calls occmap::enqueue at the end of a frame.
//
// The rule.  Members i < n with slot idx_i and log-weight lw_i (lw == nullptr: all equal):  m = max lw,  e_i = exp(lw_i - m),
// S = sum e_i,  W_s = sum over {i : idx_i = s} of e_i,  M(p) = (float)((sum over live s of W_s (double)v_s(p)) / S)  where
// v_s(p) is the float rbs_get_occlusion(h, s, .) hands out at p and a slot is live when W_s > 0.  binary64, -ffp-contract=off.
//
// The read rule stands once: occ_background (a pixel outside a slot's window: the scalar level, or the shared plane's pixel)
// and occ_slot_value (inside: the stored float, on slabs addressed through the stored region; stamped planes: exact_prior of
// the stored value and age, as rbs_expand_exact_kernel forms it).  Nothing is written but this file's own buffers: no slot is
// made dense, no window, region, clock or plane changes.
//
// Launches (one stream, in this order):
//   rbs_occmap_weights_kernel   one block: m (a maximum: order-free), e_i stored, S.  Thread t takes members t, t + 1024, ...
//                               in ascending order; then block_sum's shuffle tree and its order over the sixteen waves.
//   rbs_occmap_slots_kernel     one thread per slot: idx and e staged through LDS in chunks of 256 members, every thread walks
//                               the chunk in ascending i and adds the e_i of its own slot -- W_s is summed in ascending i.
//   rbs_occmap_compact_kernel   one block: the live slots in ascending order with their window, where their first stored float
//                               is and their row pitch (an integer scan), and the union rectangle U of the non-empty live
//                               windows (integer min / max).
//   rbs_occmap_kernel           one block of four waves per 64 consecutive pixels of a row.  The live list is cut into four
//                               contiguous parts, one per wave, all over the same 64 pixels: with U of some 10^4 pixels one
//                               wave per 64 pixels alone would leave most CUs idle.  A wave stages its part's descriptors in
//                               LDS 64 at a time and reads them back wave-uniformly (first lane -> scalar registers), so the
//                               window's test in y is a scalar branch and the loads of a row coalesce.  Each wave sums its
//                               part in list order; the four partials go to LDS and are folded in part order by the first
//                               wave, which divides by S and rounds to float once.  Pixels outside U get the background.
// Every order above is fixed by n, idx and the windows; there is no floating-point atomic: two runs give the same bits.
// A population that never resampled has n live slots: the same kernels, only longer lists.
//
// rbs_occmap_bodies_kernel: the assessor's planes and owner rule (rbs_planes_render_kernel<true>, planes_owner:
// rbs_pose_planes.h) over a map instead of a depth frame: integer counts and a 32.32 fixed-point sum, order-free.
#pragma once

namespace rbs {

constexpr int kOccParts = 4;       // waves of a map block = parts the live list is cut into
constexpr int kOccChunk = 256;     // members staged per step of the slots kernel

// The planes of the current buffer as the kernels address them.
struct OccView {
    const float* occ;       // slot s starts at occ + s * plane_stride
    size_t plane_stride;
    const int4* win;        // [slots] windows; nullptr: dense planes (every window is the frame)
    const int4* reg;        // [slots] stored regions of slabs; nullptr: whole planes
    const float* bgp;       // the shared trail's plane (stamped: [npx] values, then [npx] 16-bit ages); nullptr: the scalar level
    float bg;
    int rows, cols, npx, slots;
    int exact, plane_px;    // stamped planes: a slot's ages start plane_px floats behind its values
};
// A live slot: its window, geo = (x, y of its first stored float, row pitch, slot), its weight.
struct OccLive {
    int4 win, geo;
    double w, pad;
};
static_assert(sizeof(OccLive) == 48, "three 16-byte pieces, staged piecewise");

// ---- the read rule -------------------------------------------------------------------------------------------------------------
// The value of every plane at (x, y) outside its window.  (P: ptab, age_max and bg_new = the scalar level, for exact_prior.)
__device__ inline float occ_background(const OccView& V, const DevParams& P, int x, int y)
{
    const int i = y * V.cols + x;
    if (!V.exact) return V.bgp ? V.bgp[i] : V.bg;
    // (two calls, not one on selected operands: the compiler turned the selection into a choice between two ADDRESSES, one of
    // them a copy of V.bg in scratch memory)
    if (V.bgp) return exact_prior(P, V.bgp[i], (int)reinterpret_cast<const unsigned short*>(V.bgp + V.npx)[i]);
    return exact_prior(P, V.bg, 0xffff);
}
// The value of the slot stored at `base` with window w and geometry g at (x, y); bgv = occ_background(x, y).
__device__ inline float occ_slot_value(const OccView& V, const DevParams& P, const float* __restrict__ base, int4 w, int4 g, int x, int y, float bgv)
{
    if (!(x >= w.x && x < w.z && y >= w.y && y < w.w)) return bgv;
    const size_t at = (size_t)(y - g.y) * g.z + (x - g.x);
    const float v = base[at];
    if (!V.exact) return v;
    return exact_prior(P, v, (int)reinterpret_cast<const unsigned short*>(base + V.plane_px)[at]);
}

// ---- weights -------------------------------------------------------------------------------------------------------------------
// head_d: m, S
__global__ __launch_bounds__(1024) void rbs_occmap_weights_kernel(const double* __restrict__ lw, int n, double* __restrict__ e, double* __restrict__ head_d)
{
    __shared__ double sh[16];
    const int tid = threadIdx.x;
    double m = lw ? -INFINITY : 0.0;
    if (lw) for (int i = tid; i < n; i += 1024) m = fmax(m, lw[i]);
    m = rbd::block_max(m, sh);
    double s = 0.0;
    for (int i = tid; i < n; i += 1024) {
        const double ei = lw ? exp(lw[i] - m) : 1.0;
        e[i] = ei;
        s += ei;
    }
    const double S = rbd::block_sum(s, sh);
    if (tid == 0) { head_d[0] = m; head_d[1] = S; }
}

__global__ __launch_bounds__(64) void rbs_occmap_slots_kernel(const int* __restrict__ idx, const double* __restrict__ e, int n, int slots, double* __restrict__ W)
{
    __shared__ int s_idx[kOccChunk];
    __shared__ double s_e[kOccChunk];
    const int s = blockIdx.x * 64 + threadIdx.x;
    double w = 0.0;
    for (int c = 0; c < n; c += kOccChunk) {
        const int cnt = min(kOccChunk, n - c);
        for (int j = threadIdx.x; j < cnt; j += 64) { s_idx[j] = idx[c + j]; s_e[j] = e[c + j]; }
        __syncthreads();
        // (no branch: a member of another slot adds +0.0, which leaves w as it is bit for bit, and the LDS reads of eight
        // members are in flight together -- one wave per block has nothing else to hide their latency behind.  Measured at
        // 2 000 slots x 2 000 members: 145 us with the branch, 108 us in this form)
#pragma unroll 8
        for (int j = 0; j < cnt; ++j) w += s_idx[j] == s ? s_e[j] : 0.0;
        __syncthreads();
    }
    if (s < slots) W[s] = w;
}

// head_i: live, U (x0, y0, x1, y1)
__global__ __launch_bounds__(1024) void rbs_occmap_compact_kernel(const OccView V, const double* __restrict__ W, OccLive* __restrict__ live, int* __restrict__ head_i)
{
    __shared__ int s_wave[16];
    __shared__ int s_u[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { s_u[0] = V.cols; s_u[1] = V.rows; s_u[2] = 0; s_u[3] = 0; }
    const int per = (V.slots + 1023) / 1024;
    const int s0 = min(V.slots, tid * per), s1 = min(V.slots, s0 + per);
    int cnt = 0;
    for (int s = s0; s < s1; ++s) cnt += W[s] > 0.0 ? 1 : 0;
    // exclusive scan of cnt over the block: integers, any order gives the same offsets
    int inc = cnt;
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(inc, off, 64);
        if (lane >= off) inc += v;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    int at = inc - cnt, total = 0;
    for (int k = 0; k < 16; ++k) {
        if (k < wave) at += s_wave[k];
        total += s_wave[k];
    }
    for (int s = s0; s < s1; ++s) {
        const double w = W[s];
        if (!(w > 0.0)) continue;
        int wx0 = 0, wy0 = 0, wx1 = V.cols, wy1 = V.rows;   // dense planes: the frame
        if (V.win) { const int4 r = V.win[s]; wx0 = r.x; wy0 = r.y; wx1 = r.z; wy1 = r.w; }
        const bool empty = wx1 <= wx0 || wy1 <= wy0;
        if (empty) { wx0 = V.cols; wy0 = V.rows; wx1 = 0; wy1 = 0; }
        int gx = 0, gy = 0, pitch = V.cols;
        if (V.reg && !empty) { const int4 r = V.reg[s]; gx = r.x; gy = r.y; pitch = r.z - r.x; }
        OccLive* d = live + at++;
        d->win = make_int4(wx0, wy0, wx1, wy1);
        d->geo = make_int4(gx, gy, pitch, s);
        d->w = w;
        d->pad = 0.0;
        if (!empty) {
            atomicMin(&s_u[0], wx0); atomicMin(&s_u[1], wy0);
            atomicMax(&s_u[2], wx1); atomicMax(&s_u[3], wy1);
        }
    }
    __syncthreads();
    if (tid == 0) {
        head_i[0] = total;
        head_i[1] = s_u[0]; head_i[2] = s_u[1];
        head_i[3] = min(s_u[2], V.cols); head_i[4] = min(s_u[3], V.rows);
    }
}

// ---- the map -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kOccParts) void rbs_occmap_kernel(const OccView V, const DevParams P, const OccLive* __restrict__ live,
                                                                     const int* __restrict__ head_i, const double* __restrict__ head_d,
                                                                     float* __restrict__ out)
{
    __shared__ int4 s_win[kOccParts][64];
    __shared__ int4 s_geo[kOccParts][64];
    __shared__ double s_w[kOccParts][64];
    __shared__ double s_part[kOccParts][64];
    const int lane = threadIdx.x & 63, part = threadIdx.x >> 6;
    const int tx0 = (int)blockIdx.x * 64, x = tx0 + lane, y = (int)blockIdx.y;
    const bool inb = x < V.cols;
    const float bgv = inb ? occ_background(V, P, x, y) : 0.f;
    const int L = head_i[0];
    const int4 U = make_int4(head_i[1], head_i[2], head_i[3], head_i[4]);
    // (the whole block takes this exit or none of it does)
    if (L < 1 || y < U.y || y >= U.w || tx0 >= U.z || tx0 + 64 <= U.x) {
        if (part == 0 && inb) out[(size_t)y * V.cols + x] = bgv;
        return;
    }
    const int p0 = (int)((long)L * part / kOccParts), p1 = (int)((long)L * (part + 1) / kOccParts);
    const int batches = ((L + kOccParts - 1) / kOccParts + 63) / 64;   // of the longest part: every wave takes every barrier
    double acc = 0.0;
    for (int b = 0; b < batches; ++b) {
        const int j0 = p0 + b * 64;
        if (j0 + lane < p1) {
            const OccLive* d = live + j0 + lane;
            s_win[part][lane] = d->win;
            s_geo[part][lane] = d->geo;
            s_w[part][lane] = d->w;
        }
        __syncthreads();
        const int cnt = max(0, min(64, p1 - j0));
        for (int k = 0; k < cnt; ++k) {
            const int4 wv = s_win[part][k], gv = s_geo[part][k];
            const int4 w = make_int4(__builtin_amdgcn_readfirstlane(wv.x), __builtin_amdgcn_readfirstlane(wv.y),
                                     __builtin_amdgcn_readfirstlane(wv.z), __builtin_amdgcn_readfirstlane(wv.w));
            float v = bgv;
            if (y >= w.y && y < w.w) {   // (the same for the whole wave; occ_slot_value tests x)
                const int4 g = make_int4(__builtin_amdgcn_readfirstlane(gv.x), __builtin_amdgcn_readfirstlane(gv.y),
                                         __builtin_amdgcn_readfirstlane(gv.z), __builtin_amdgcn_readfirstlane(gv.w));
                if (inb) v = occ_slot_value(V, P, V.occ + (size_t)g.w * V.plane_stride, w, g, x, y, bgv);
            }
            acc += s_w[part][k] * (double)v;
        }
        __syncthreads();
    }
    s_part[part][lane] = acc;
    __syncthreads();
    if (part != 0 || !inb) return;
    double total = s_part[0][lane];
    for (int p = 1; p < kOccParts; ++p) total += s_part[p][lane];
    const bool in_u = x >= U.x && x < U.z;
    out[(size_t)y * V.cols + x] = in_u ? (float)(total / head_d[1]) : bgv;
}

// ---- per-body summary of a map -------------------------------------------------------------------------------------------------
struct OccBodiesArgs {
    PlaneSet S;               // the assessor's n x B planes
    const float* map;         // [npx]
    double threshold;
    rbs_occlusion_body* rec;  // [n x B], zeroed
};

// Every pixel of pose blockIdx.y's rectangle with rbs_assess_count_kernel's walk and owner rule (planes_union_rect,
// planes_owner: rbs_pose_planes.h).
__global__ __launch_bounds__(256) void rbs_occmap_bodies_kernel(const OccBodiesArgs A)
{
    __shared__ int s_cnt[kMaxBodies * 2];
    __shared__ unsigned long long s_sum[kMaxBodies];
    __shared__ int4 s_rect[kMaxBodies];
    const PlaneSet& S = A.S;
    const int tid = threadIdx.x, k = blockIdx.y, B = S.B;
    for (int e = tid; e < B * 2; e += 256) s_cnt[e] = 0;
    if (tid < B) { s_sum[tid] = 0ull; s_rect[tid] = S.rects[k * B + tid]; }
    __syncthreads();
    const int4 u = planes_union_rect(S, s_rect, 0xffffffffu);
    const int x0 = u.x, y0 = u.y, x1 = u.z, y1 = u.w;
    if (x1 > x0) {
        const int w = x1 - x0, total = w * (y1 - y0);
        const float* planes = S.planes + (size_t)k * B * S.npx;
        for (int p = blockIdx.x * 256 + tid; p < total; p += gridDim.x * 256) {
            const int ly = p / w, x = x0 + (p - ly * w), y = y0 + ly;
            const int i = y * S.cols + x;
            float best;
            const int owner = planes_owner(S, planes, s_rect, 0xffffffffu, x, y, i, best);
            if (owner < 0) continue;
            const double mv = (double)A.map[i];
            atomicAdd(s_cnt + owner * 2, 1);
            if (mv > A.threshold) atomicAdd(s_cnt + owner * 2 + 1, 1);
            atomicAdd(s_sum + owner, (unsigned long long)(mv * 4294967296.0));
        }
    }
    __syncthreads();
    for (int b = tid; b < B; b += 256) {
        rbs_occlusion_body* r = A.rec + (size_t)k * B + b;
        if (s_cnt[2 * b]) atomicAdd(&r->rendered, s_cnt[2 * b]);
        if (s_cnt[2 * b + 1]) atomicAdd(&r->occluded, s_cnt[2 * b + 1]);
        if (s_sum[b]) atomicAdd(reinterpret_cast<unsigned long long*>(&r->sum_q32), s_sum[b]);
    }
}

}  // namespace rbs

static_assert(sizeof(rbs_occlusion_body) == 32 && offsetof(rbs_occlusion_body, sum_q32) == 8 && offsetof(rbs_occlusion_body, reserved) == 16,
              "rbs_occlusion_body layout is mirrored by dbot_ros_amd/_capi.py and tests/test_occlusion_map_cpu.py");

// What a sensor owns once a map has been asked of it: allocated at first use, grow-only, freed by rbs_destroy.
struct rbs_occmap_state {
    int cap_n = 0;                  // members the per-member buffers hold
    int* d_idx = nullptr;           // [cap_n] a caller's slots (rbs_occlusion_mean)
    double* d_lw = nullptr;         // [cap_n] ... and log-weights
    double* d_e = nullptr;          // [cap_n]
    double* d_W = nullptr;          // [slots]
    rbs::OccLive* d_live = nullptr; // [slots]
    int* d_head_i = nullptr;        // [8]
    double* d_head_d = nullptr;     // [2]
    float* d_out = nullptr;         // [npx] rbs_occlusion_mean's map; rbs_occlusion_bodies' map
    rbs_occlusion_body* d_brec = nullptr;   // [kAssessMaxPlanes]
    hipEvent_t ev[2] = {nullptr, nullptr};
    float ms = 0.f;
    bool have = false;              // an rbs_occlusion_mean has run
};

namespace {
namespace occmap {

int slots_of(const rbs_handle* h) { return h->occ_slots > 0 ? h->occ_slots : h->max_particles; }

// Buffers for a population of n members (grow-only; a growth waits for the stream: its readers may be queued there).
int32_t ensure(rbs_handle* h, int n)
{
    if (!h->occmap) {
        h->occmap = new (std::nothrow) rbs_occmap_state;
        if (!h->occmap) return fail(h, RBS_ERR_OUT_OF_MEMORY, "occlusion map: out of host memory");
    }
    rbs_occmap_state* o = h->occmap;
    const size_t slots = (size_t)slots_of(h);
    if (!o->d_W) RBS_HIP(h, hipMalloc(&o->d_W, sizeof(double) * slots));
    if (!o->d_live) RBS_HIP(h, hipMalloc(&o->d_live, sizeof(rbs::OccLive) * slots));
    if (!o->d_head_i) RBS_HIP(h, hipMalloc(&o->d_head_i, sizeof(int) * 8));
    if (!o->d_head_d) RBS_HIP(h, hipMalloc(&o->d_head_d, sizeof(double) * 2));
    if (!o->d_out) RBS_HIP(h, hipMalloc(&o->d_out, sizeof(float) * (size_t)h->npx));
    if (!o->d_brec) RBS_HIP(h, hipMalloc(&o->d_brec, sizeof(rbs_occlusion_body) * rbs::kAssessMaxPlanes));
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
    return RBS_OK;
}

// The map of the population (d_idx, d_lw -- nullptr: uniform --, n) over the CURRENT planes into `out` (npx floats as the device
// addresses them), on the handle's stream.  The buffers exist (ensure).  The launches are ordered behind the plane writes of the
// last updating call -- the copy stream's join, taken here as drain takes it -- and, being on the handle's stream, in front of
// every later call's writes: the copy stream forks from this stream inside that call.
int32_t enqueue(rbs_handle* h, const int* d_idx, const double* d_lw, int n, float* out)
{
    rbs_occmap_state* o = h->occmap;
    hipStream_t s = h->stream;
    if (h->join_pending >= 0) {
        RBS_HIP(h, hipStreamWaitEvent(s, h->ev_join[h->join_pending], 0));
        h->join_pending = -1;
    }
    rbs::OccView V{};
    V.occ = h->d_occ[h->cur];
    V.plane_stride = h->plane_stride;
    V.win = h->windowed ? h->d_win[h->cur] : nullptr;
    V.reg = h->slab_px ? h->d_reg[h->cur] : nullptr;
    V.bgp = shared_plane(h);
    V.bg = h->background;
    V.rows = h->rows; V.cols = h->cols; V.npx = h->npx;
    V.slots = slots_of(h);
    V.exact = h->exact ? 1 : 0;
    V.plane_px = h->slab_px ? h->slab_px : h->npx;
    DevParams P = h->base;
    P.ptab = h->d_ptab;
    P.age_max = h->age_max;
    P.bg_new = h->background;
    hipLaunchKernelGGL(rbs::rbs_occmap_weights_kernel, dim3(1), dim3(1024), 0, s, d_lw, n, o->d_e, o->d_head_d);
    hipLaunchKernelGGL(rbs::rbs_occmap_slots_kernel, dim3((unsigned)((V.slots + 63) / 64)), dim3(64), 0, s, d_idx, (const double*)o->d_e, n, V.slots, o->d_W);
    hipLaunchKernelGGL(rbs::rbs_occmap_compact_kernel, dim3(1), dim3(1024), 0, s, V, (const double*)o->d_W, o->d_live, o->d_head_i);
    hipLaunchKernelGGL(rbs::rbs_occmap_kernel, dim3((unsigned)((h->cols + 63) / 64), (unsigned)h->rows), dim3(64 * rbs::kOccParts), 0, s, V, P,
                       (const rbs::OccLive*)o->d_live, (const int*)o->d_head_i, (const double*)o->d_head_d, out);
    RBS_HIP(h, hipGetLastError());
    return RBS_OK;
}

const char* single_device_only(const rbs_handle* h)
{
    return !h->shards.empty() || h->group || h->peer_world > 1 ? "single-device handles only" : nullptr;
}

}  // namespace occmap

// rbs_destroy (the handle's device is current and its streams are idle).
void occmap_release(rbs_handle* h)
{
    rbs_occmap_state* o = h->occmap;
    if (!o) return;
    (void)hipFree(o->d_idx);
    (void)hipFree(o->d_lw);
    (void)hipFree(o->d_e);
    (void)hipFree(o->d_W);
    (void)hipFree(o->d_live);
    (void)hipFree(o->d_head_i);
    (void)hipFree(o->d_head_d);
    (void)hipFree(o->d_out);
    (void)hipFree(o->d_brec);
    for (hipEvent_t e : o->ev)
        if (e) (void)hipEventDestroy(e);
    delete o;
    h->occmap = nullptr;
}

}  // namespace

extern "C" {

int32_t rbs_occlusion_mean(rbs_handle* h, const int32_t* slots, const double* log_weights, int32_t n, float* out)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!slots || !out) return fail(h, RBS_ERR_INVALID_ARGUMENT, "occlusion_mean: null pointer");
    if (n < 1) return fail(h, RBS_ERR_INVALID_ARGUMENT, "occlusion_mean: n < 1");
    if (const char* why = occmap::single_device_only(h)) return fail(h, RBS_ERR_UNSUPPORTED, fmt("occlusion_mean: %s", why));
    const int nslots = occmap::slots_of(h);
    for (int i = 0; i < n; ++i)
        if (slots[i] < 0 || slots[i] >= nslots) return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("occlusion_mean: bad slot %d (member %d)", slots[i], i));
    if (log_weights) {
        bool any = false;
        for (int i = 0; i < n; ++i) {
            const double w = log_weights[i];
            if (std::isfinite(w)) any = true;
            else if (!(std::isinf(w) && w < 0.0))
                return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("occlusion_mean: log-weight %d is neither finite nor -inf", i));
        }
        if (!any) return fail(h, RBS_ERR_INVALID_ARGUMENT, "occlusion_mean: every log-weight is -inf");
    }
    RBS_REFUSE_POISONED(h);
    RBS_HIP(h, hipSetDevice(h->device));
    if (int32_t rc = drain(h, true)) return rc;
    if (int32_t rc = occmap::ensure(h, n)) return rc;
    rbs_occmap_state* o = h->occmap;
    RBS_HIP(h, hipMemcpy(o->d_idx, slots, sizeof(int) * (size_t)n, hipMemcpyHostToDevice));
    if (log_weights) RBS_HIP(h, hipMemcpy(o->d_lw, log_weights, sizeof(double) * (size_t)n, hipMemcpyHostToDevice));
    o->have = false;
    RBS_HIP(h, hipEventRecord(o->ev[0], h->stream));
    if (int32_t rc = occmap::enqueue(h, o->d_idx, log_weights ? o->d_lw : nullptr, n, o->d_out)) return rc;
    RBS_HIP(h, hipEventRecord(o->ev[1], h->stream));
    RBS_HIP(h, hipStreamSynchronize(h->stream));
    RBS_HIP(h, hipMemcpy(out, o->d_out, sizeof(float) * (size_t)h->npx, hipMemcpyDeviceToHost));
    RBS_HIP(h, hipEventElapsedTime(&o->ms, o->ev[0], o->ev[1]));
    o->have = true;
    return RBS_OK;
}

int32_t rbs_occlusion_mean_ms(rbs_handle* h, float* ms)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!ms || !h->occmap || !h->occmap->have) return fail(h, RBS_ERR_INVALID_ARGUMENT, "occlusion_mean_ms: no map computed yet or a null pointer");
    *ms = h->occmap->ms;
    return RBS_OK;
}

int32_t rbs_occlusion_bodies(rbs_handle* h, const float* map, const double* poses, int32_t n, double threshold, rbs_occlusion_body* out)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!map || !poses || !out) return fail(h, RBS_ERR_INVALID_ARGUMENT, "occlusion_bodies: null pointer");
    if (n < 1) return fail(h, RBS_ERR_INVALID_ARGUMENT, "occlusion_bodies: n < 1");
    if (!(threshold >= 0.0 && threshold <= 1.0)) return fail(h, RBS_ERR_INVALID_ARGUMENT, "occlusion_bodies: threshold must lie in [0, 1]");
    if (const char* why = occmap::single_device_only(h)) return fail(h, RBS_ERR_UNSUPPORTED, fmt("occlusion_bodies: %s", why));
    const int B = h->n_bodies;
    if ((long)n * B > rbs::kAssessMaxPlanes)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("occlusion_bodies: n x n_objects = %ld exceeds %d", (long)n * B, rbs::kAssessMaxPlanes));
    const int planes = n * B;
    for (size_t i = 0; i < (size_t)planes * 12; ++i)
        if (!std::isfinite(poses[i])) return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("occlusion_bodies: pose entry %zu is not finite", i));
    for (size_t i = 0; i < (size_t)h->npx; ++i)
        if (!(map[i] >= 0.f && map[i] <= 1.f)) return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("occlusion_bodies: map value %zu is not in [0, 1]", i));
    RBS_REFUSE_POISONED(h);
    RBS_HIP(h, hipSetDevice(h->device));
    if (int32_t rc = assess::ensure(h, planes)) return rc;
    if (int32_t rc = occmap::ensure(h, 1)) return rc;
    rbs_assess_state* a = h->assess;
    rbs_occmap_state* o = h->occmap;
    hipStream_t s = h->stream;
    // the assessor's planes and rectangles at these poses
    RBS_HIP(h, hipStreamSynchronize(s));   // (the two buffers written next have no reader left)
    RBS_HIP(h, hipMemcpy(a->d_poses, poses, sizeof(double) * 12 * (size_t)planes, hipMemcpyHostToDevice));
    RBS_HIP(h, hipMemcpy(o->d_out, map, sizeof(float) * (size_t)h->npx, hipMemcpyHostToDevice));
    RBS_HIP(h, hipMemsetAsync(o->d_brec, 0, sizeof(rbs_occlusion_body) * (size_t)planes, s));
    assess::planes_hold(a, 0, false);
    rbs::launch_pose_planes(s, h->base, a->d_poses, n, true, a->d_planes, a->d_rects, nullptr);
    RBS_HIP(h, hipGetLastError());
    rbs::OccBodiesArgs A{};
    A.S = rbs::PlaneSet{a->d_planes, a->d_rects, h->cols, h->npx, B};
    A.map = o->d_out;
    A.threshold = threshold;
    A.rec = o->d_brec;
    hipLaunchKernelGGL(rbs::rbs_occmap_bodies_kernel, dim3(rbs::kAssessCountBlocks, (unsigned)n), dim3(256), 0, s, A);
    RBS_HIP(h, hipGetLastError());
    RBS_HIP(h, hipStreamSynchronize(s));
    RBS_HIP(h, hipMemcpy(out, o->d_brec, sizeof(rbs_occlusion_body) * (size_t)planes, hipMemcpyDeviceToHost));
    // (the planes of these poses are what rbs_assess_get_plane hands out now, as after an rbs_assess_poses; the assessor's kernel
    // times -- rbs_assess_kernel_ms -- stay those of its own last call: no event of its is recorded here)
    assess::planes_hold(a, n, false);
    return RBS_OK;
}

}  // extern "C"
