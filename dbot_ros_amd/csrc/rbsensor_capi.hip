// rbsensor_capi.hip -- host side of librbsensor_mi355x.so: the C-ABI declared in
// include/rbsensor_mi355x.h over the kernels in rbsensor_kernels.hip.
//
// Device-resident state per handle (sizes at 640x480, N slots):
//   soup      9 * n_tri doubles, SoA triangle soup                     (368 KB @5 120 tris)
//   frame     rows*cols float, current observation                     (1.2 MB)
//   occ[2]    2 * N * rows*cols float, double-buffered occlusion planes (2.46 MB * N)
//   win[2]    2 * N int4 + one float: a plane is explicit inside its window, the background elsewhere
//   poses / indices / out   per-call staging for the host-pointer API
// There is no CPU path in this library.
//
// One translation unit.  Most of the host side has files of its own, included below where they are needed:
//   rbs_handle.h       struct rbs_handle, Rccl, fmt / fail / upload, RBS_HIP, RBS_REFUSE_POISONED, with_flags
//   rbs_frames.h       frame ingest: obs_frame, convert_f64_f32*, BorrowedFrameGuard, upload_frame, hand_over_*, make_current, frame_abandon
//   rbs_call.h         the likelihood call: occlusion_coeffs, launch_prep, launch_raster, launch_bgp_step, stp_decide, enqueue_loglikes
//   rbs_device.h       (through rbsensor_kernels.hip) generic device helpers: rotations, Philox, block_sum / block_max
//   rbs_pose_planes.h  poses drawn as depth planes: rbs_planes_render_kernel, launch_pose_planes, PlaneSet and its owner rule
//   rbs_planes.h       the occlusion planes' storage: materialize, slab_expand / exact_expand, store_plane, fit_or_grow, grow_slabs, drain
//   rbs_planes_api.h   the slot entry points: rbs_get_occlusion .. rbs_import_window, rbs_stream_join, rbs_get_window
//   rbs_ipc.h          IpcBlob, rbs_ipc_export, rbs_ipc_attach, rbs_stage_windows, rbs_peer_resample
//   rbs_modes_api.h    the posterior modes on a sensor handle: rbs_modes_default_params, rbs_pose_modes
//   rbs_tracker_api.h  the device tracker's host side: struct rbs_tracker, launch_*, rbs_tracker_*
// This file itself: release / create_impl, several devices, and the remaining extern "C" sensor entry points.
#include "rbsensor_kernels.hip"
#include "rbsensor_tracker.hip"
#include "rbsensor_posterior.hip"
#include "rbsensor_modes.hip"
#include "rbsensor_peers.hip"
#include "rbs_mesh.h"

#include "../../include/rbsensor_mi355x.h"

#include <dlfcn.h>
#include <unistd.h>

#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <array>
#include <map>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "rbs_handle.h"

// Frame ingest: obs_frame .. frame_abandon.
#include "rbs_frames.h"

#include "rbs_call.h"

// The occlusion planes' storage: materialize, slabs, stamped planes, grow_slabs, drain.
#include "rbs_planes.h"

// Poses drawn as depth planes and the rule for reading them back: the render kernel, its launch, PlaneSet (create_impl sets its LDS limit).
#include "rbs_pose_planes.h"

// The pose assessor (rbs_assess_*): its kernels and host side (release calls into it).
#include "rbsensor_assess.hip"
// The contour rule beside it (rbs_contour_*): one more kernel on the assessor's planes.
#include "rbsensor_contour.hip"
// The occlusion map (rbs_occlusion_*): the population's mean plane read from the planes as stored, and its per-body summary.
#include "rbsensor_occmap.hip"
// The object map (rbs_object_*): per pixel and body what a population sees, the mean and variance of its depth, the segmentation.
#include "rbsensor_objmap.hip"
// The posterior modes (rbs_pose_modes): the handle's buffers and the stateless entry point; kernels in rbsensor_modes.hip.
#include "rbs_modes_api.h"
// The pose refiner (rbs_refine_*): projective point-to-plane Gauss-Newton on the assess rule's planes; kernels, then the host side.
#include "rbsensor_refine.hip"
#include "rbs_refine_api.h"

namespace {

int copy_bands_for(int rows, int cols)
{
    // ~3840 float4 (60 KB) per copy block; an EVEN band count keeps 1+bands odd so raster
    // blocks (block index = particle*(1+bands)) rotate over all 8 XCDs.
    const long n4 = ((long)rows * cols + 3) / 4;
    long b = (n4 + 3839) / 3840;
    if (b < 2) b = 2;
    if (b & 1) ++b;
    if (b > rows) b = (rows & 1) ? rows + 1 : rows;
    return (int)b;
}

void release(rbs_handle* h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->copy_stream) (void)hipStreamSynchronize(h->copy_stream);
    for (auto& rank_bufs : h->peer_mapped)
        for (void*& p : rank_bufs)
            if (p) { (void)hipIpcCloseMemHandle(p); p = nullptr; }
    (void)hipFree(h->d_soup);
    (void)hipFree(h->d_frame);
    (void)hipFree(h->d_aux);
    (void)hipFree(h->d_aux_slot[0]);
    (void)hipFree(h->d_aux_slot[1]);
    (void)hipFree(h->d_pbg);
    (void)hipFree(h->d_occ[0]);
    (void)hipFree(h->d_occ[1]);
    (void)hipFree(h->d_poses);
    (void)hipFree(h->d_indices);
    (void)hipFree(h->d_rects[0]);
    (void)hipFree(h->d_rects[1]);
    (void)hipFree(h->d_groups[0]);
    (void)hipFree(h->d_groups[1]);
    (void)hipFree(h->d_strips[0]);
    (void)hipFree(h->d_strips[1]);
    (void)hipFree(h->d_parents[0]);
    (void)hipFree(h->d_parents[1]);
    (void)hipFree(h->d_win[0]);
    (void)hipFree(h->d_win[1]);
    (void)hipFree(h->d_win_used);
    (void)hipFree(h->d_reg[0]);
    (void)hipFree(h->d_reg[1]);
    (void)hipFree(h->d_err);
    (void)hipFree(h->d_bbox);
    (void)hipFree(h->d_peer_scratch);
    if (h->h_err) (void)hipHostFree(h->h_err);
    (void)hipFree(h->d_item_range);
    (void)hipFree(h->d_item_particle);
    (void)hipFree(h->d_ctr);
    (void)hipFree(h->d_depth);
    (void)hipFree(h->d_bgp[0]);
    (void)hipFree(h->d_bgp[1]);
    (void)hipFree(h->d_bgp_box);
    (void)hipFree(h->d_ptab);
    (void)hipFree(h->d_tmp_plane);
    (void)hipFree(h->d_area);
    (void)hipFree(h->d_wide_flags);
    if (h->h_area) (void)hipHostFree(h->h_area);
    if (h->ev_area) (void)hipEventDestroy(h->ev_area);
    (void)hipFree(h->d_done);
    (void)hipFree(h->d_partial);
    (void)hipFree(h->d_cluster_sphere);
    (void)hipFree(h->d_cluster_cone);
    (void)hipFree(h->d_cluster_vtx);
    (void)hipFree(h->d_cluster_nv);
    (void)hipFree(h->d_tri_local);
    (void)hipFree(h->d_tri_plane);
    (void)hipFree(h->d_vtx);
    (void)hipFree(h->d_render);
    assess_release(h);
    occmap_release(h);
    objmap_release(h);
    modes_release(h);
    refine_release(h);
    if (h->up_stream) (void)hipStreamSynchronize(h->up_stream);
    for (int k = 0; k < 2; ++k) {
        if (h->h_frames[k]) (void)hipHostFree(h->h_frames[k]);
        if (h->ev_frame[k]) (void)hipEventDestroy(h->ev_frame[k]);
        if (h->ev_used[k]) (void)hipEventDestroy(h->ev_used[k]);
        if (k == 0 && h->ev_reader) (void)hipEventDestroy(h->ev_reader);
        (void)hipFree(h->d_fin[k]);
    }
    if (h->up_stream) (void)hipStreamDestroy(h->up_stream);
    if (h->h_in) (void)hipHostFree(h->h_in);
    if (h->h_out) (void)hipHostFree(h->h_out);
    (void)hipFree(h->d_in);
    if (h->ev_out) (void)hipEventDestroy(h->ev_out);
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    for (int i = 0; i < rbs_handle::kRing; ++i) {
        if (h->ev_start[i]) (void)hipEventDestroy(h->ev_start[i]);
        if (h->ev_stop[i]) (void)hipEventDestroy(h->ev_stop[i]);
        if (h->ev_copy_start[i]) (void)hipEventDestroy(h->ev_copy_start[i]);
        if (h->ev_join[i]) (void)hipEventDestroy(h->ev_join[i]);
        if (h->ev_raster_start[i]) (void)hipEventDestroy(h->ev_raster_start[i]);
        if (h->ev_raster_stop[i]) (void)hipEventDestroy(h->ev_raster_stop[i]);
        if (h->ev_copy_stop[i]) (void)hipEventDestroy(h->ev_copy_stop[i]);
    }
    if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

int32_t create_impl(const rbs_config* cfg, rbs_handle* h)
{
    if (cfg->abi_version != RBS_ABI_VERSION)
        return fail(h, RBS_ERR_INVALID_ARGUMENT,
                    fmt("abi_version %d, library is %d", cfg->abi_version, RBS_ABI_VERSION));
    if (cfg->rows <= 0 || cfg->cols <= 0 || cfg->cols > 8192 || cfg->rows > 8192)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("bad resolution %dx%d", cfg->cols, cfg->rows));
    if (cfg->max_particles <= 0)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "max_particles must be positive");
    if (cfg->n_objects <= 0 || cfg->n_objects > rbs::kMaxBodies)
        return fail(h, RBS_ERR_INVALID_ARGUMENT,
                    fmt("n_objects %d outside 1..%d", cfg->n_objects, rbs::kMaxBodies));
    if (!cfg->vertices || !cfg->vertex_counts || !cfg->triangles || !cfg->triangle_counts)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "null mesh pointer");
    const double* K = cfg->K;
    if (!(K[0] > 0.0) || !(K[4] > 0.0) || K[1] != 0.0 || K[3] != 0.0 || K[6] != 0.0 ||
        K[7] != 0.0 || K[8] != 1.0)
        return fail(h, RBS_ERR_UNSUPPORTED,
                    "camera matrix must be [fx 0 cx; 0 fy cy; 0 0 1] with fx, fy > 0");
    const double c = cfg->p_occluded_occluded - cfg->p_occluded_visible;
    if (!(c > 0.0) || !(c < 1.0))
        return fail(h, RBS_ERR_INVALID_ARGUMENT,
                    "need 0 < p_occluded_occluded - p_occluded_visible < 1");
    if (!(cfg->delta_time > 0.0)) return fail(h, RBS_ERR_INVALID_ARGUMENT, "delta_time must be > 0");
    // the pixel model: a density needs a positive noise level and a mixture weight in [0, 1) (with
    // these the per-pixel arithmetic never meets a NaN of its own making: sigma > 0 for every finite o)
    if (!(cfg->model_sigma > 0.0) || !(cfg->sigma_factor >= 0.0) || !std::isfinite(cfg->model_sigma) || !std::isfinite(cfg->sigma_factor))
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "need kinect.model_sigma > 0 and kinect.sigma_factor >= 0");
    // tail_weight: the reference hands the ROS parameter through unchecked, 0 included, so 0 <= tw < 1 is
    // accepted.  The library's erfc / exp are accurate in ABSOLUTE terms (1e-16), which is all the mixture can see next to
    // tw / max_depth -- with tw = 0 the far tails would be priced by that floor instead of the decaying value --
    // so a weight below kTailWeightFloor is EVALUATED as kTailWeightFloor (tw / max_depth = 1.7e-10: the tables' 1e-16 is
    // then 6e-7 relative in the deepest tail, far inside the 1e-5 bar; a log-likelihood that the exact tw = 0 model
    // drives to -inf becomes a large finite negative number instead).  Stated in the header and INTEGRATION.md.
    if (!(cfg->tail_weight >= 0.0) || !(cfg->tail_weight < 1.0))
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "need 0 <= kinect.tail_weight < 1");
    if (!(cfg->initial_occlusion_prob >= 0.0) || !(cfg->initial_occlusion_prob <= 1.0))
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "need 0 <= occlusion.initial_occlusion_prob <= 1");

    (void)hipGetLastError();   // a stale error left by somebody else on this thread is not ours
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(h, RBS_ERR_NO_DEVICE,
                    "no HIP device visible: librbsensor_mi355x has no CPU path");
    if (cfg->device_id < 0 || cfg->device_id >= ndev)
        return fail(h, RBS_ERR_NO_DEVICE, fmt("device_id %d of %d", cfg->device_id, ndev));
    h->device = cfg->device_id;
    RBS_HIP(h, hipSetDevice(h->device));

    h->rows = cfg->rows;
    h->cols = cfg->cols;
    h->npx = cfg->rows * cfg->cols;
    h->max_particles = cfg->max_particles;
    h->n_bodies = cfg->n_objects;
    h->p_ov = cfg->p_occluded_visible;
    h->p_oo = cfg->p_occluded_occluded;
    h->init_occ = cfg->initial_occlusion_prob;
    h->delta_time = cfg->delta_time;
    switch (cfg->likelihood_precision) {
        case RBS_PRECISION_DEFAULT:
            // the caller leaves it open: the library's default (F64, the reference CPU model's arithmetic),
            // unless the environment names one (tooling: A/B runs of an unchanged caller); a precision
            // the caller names is never overridden
            h->precision = RBS_PRECISION_LIBRARY_DEFAULT;
            if (const char* m = std::getenv("RBS_PRECISION")) {
                if (!std::strcmp(m, "f64")) h->precision = RBS_PRECISION_F64;
                else if (!std::strcmp(m, "f32")) h->precision = RBS_PRECISION_F32;
            }
            break;
        case RBS_PRECISION_F64: case RBS_PRECISION_F32: h->precision = cfg->likelihood_precision; break;
        default: return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("likelihood_precision %d", cfg->likelihood_precision));
    }
    if (cfg->state_layout < RBS_STATE_DEFAULT || cfg->state_layout > RBS_STATE_DENSE)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("state_layout %d", cfg->state_layout));
    if (cfg->state_slab_px < RBS_SLAB_WHOLE_PLANES)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("state_slab_px %d", cfg->state_slab_px));
    if (cfg->occlusion_mode < RBS_OCC_DEFAULT || cfg->occlusion_mode > RBS_OCC_REFERENCE)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("occlusion_mode %d", cfg->occlusion_mode));

    DevParams& B = h->base;
    B.rows = h->rows; B.cols = h->cols; B.npx = h->npx;
    B.n_bodies = h->n_bodies;
    B.fx = K[0]; B.fy = K[4]; B.cx = K[2]; B.cy = K[5];
    B.tw = std::max(cfg->tail_weight, RBS_TAIL_WEIGHT_FLOOR); B.ms = cfg->model_sigma; B.sf = cfg->sigma_factor;
    B.lambda = -std::log(0.5) / rbs::kHalfLifeDepth;
    B.cv0 = (1.0 - B.tw) / std::sqrt(M_PI);
    B.bands = copy_bands_for(h->rows, h->cols);
    B.band_rows = (h->rows + B.bands - 1) / B.bands;

    // the meshes -> what the raster kernels read (rbs_mesh.h: host only, checked on a CPU by tests/test_mesh_prep_cpu.py)
    rbs::PreparedMesh mesh;
    {
        const rbs::MeshInput in = {cfg->n_objects, cfg->vertices, cfg->vertex_counts, cfg->triangles, cfg->triangle_counts};
        std::string why;
        if (const int rc = rbs::prepare_mesh(in, /*allow_cull=*/true, &mesh, &why)) return fail(h, rc, why);
        std::copy(std::begin(mesh.tri_begin), std::end(mesh.tri_begin), B.tri_begin);
        std::copy(std::begin(mesh.tri_end), std::end(mesh.tri_end), B.tri_end);
        std::copy(std::begin(mesh.vtx_begin), std::end(mesh.vtx_begin), B.vtx_begin);
        for (int b = 0; b < h->n_bodies; ++b) {
            B.body_cull[b] = mesh.body_cull[b];
            std::copy(mesh.sphere[b], mesh.sphere[b] + 4, B.sphere[b]);
        }
        B.n_tri = (int)mesh.n_alloc;
    }
    {   // (the object finder re-creates this configuration at other resolutions: keep it with copies of the mesh)
        size_t nv = 0, nt = 0;
        for (int b = 0; b < cfg->n_objects; ++b) { nv += (size_t)cfg->vertex_counts[b]; nt += (size_t)cfg->triangle_counts[b]; }
        h->cfg = *cfg;
        h->cfg_vertices.assign(cfg->vertices, cfg->vertices + 3 * nv);
        h->cfg_vertex_counts.assign(cfg->vertex_counts, cfg->vertex_counts + cfg->n_objects);
        h->cfg_triangles.assign(cfg->triangles, cfg->triangles + 3 * nt);
        h->cfg_triangle_counts.assign(cfg->triangle_counts, cfg->triangle_counts + cfg->n_objects);
        h->cfg.vertices = h->cfg_vertices.data();
        h->cfg.vertex_counts = h->cfg_vertex_counts.data();
        h->cfg.triangles = h->cfg_triangles.data();
        h->cfg.triangle_counts = h->cfg_triangle_counts.data();
        h->cfg.n_devices = 0;
        h->cfg.device_ids = nullptr;
    }
    h->many_clusters |= mesh.max_clusters > 64 * (rbs::kBlock / 64);   // (more steps of 64 clusters than the block has waves)
    if (const char* e = std::getenv("RBS_SHARED_CULL")) h->many_clusters = std::atoi(e) != 0;   // (A/B: the other set of kernels)

    const size_t plane = (size_t)h->npx * sizeof(float);
    RBS_HIP(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    RBS_HIP(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    RBS_HIP(h, hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    for (int i = 0; i < rbs_handle::kRing; ++i) {
        RBS_HIP(h, hipEventCreate(&h->ev_start[i]));
        RBS_HIP(h, hipEventCreate(&h->ev_stop[i]));
        RBS_HIP(h, hipEventCreate(&h->ev_copy_start[i]));
        RBS_HIP(h, hipEventCreate(&h->ev_join[i]));
        RBS_HIP(h, hipEventCreate(&h->ev_raster_start[i]));
        RBS_HIP(h, hipEventCreate(&h->ev_raster_stop[i]));
        RBS_HIP(h, hipEventCreate(&h->ev_copy_stop[i]));
    }
    {
        hipDeviceProp_t prop;
        RBS_HIP(h, hipGetDeviceProperties(&prop, h->device));
        h->cu_count = std::max(1, prop.multiProcessorCount);
        h->raster_blocks = 3 * h->cu_count;
        // tuning overrides (defaults are the measured best on MI355X)
        if (const char* m = std::getenv("RBS_RASTER_BLOCKS")) h->raster_blocks = std::max(1, std::atoi(m));
        if (const char* m = std::getenv("RBS_SHARED_TRAIL")) h->stp_allowed = std::atoi(m) != 0;
        if (const char* m = std::getenv("RBS_FUSED_COPY")) h->fused_copy = std::atoi(m) != 0;
        if (const char* m = std::getenv("RBS_TRACKER_SPLIT_MAX")) h->tracker_split_max = std::atoi(m);
        if (const char* m = std::getenv("RBS_STP_ENTER")) h->stp_enter = std::atof(m);
        if (const char* m = std::getenv("RBS_STP_EVERY")) h->stp_every = std::max(1, std::atoi(m));
        if (const char* m = std::getenv("RBS_SPLIT")) h->split = std::atoi(m) != 0;
        h->depth_blocks = RBS_DEPTH_MINWAVES * h->cu_count;
        h->eval_blocks = RBS_EVAL_MINWAVES * h->cu_count;
        // the layout is the caller's choice (rbs_config.state_layout); the environment is consulted
        // only when the caller leaves it open (tools comparing both layouts of an unchanged caller)
        if (cfg->state_layout == RBS_STATE_DENSE) h->windowed = false;
        else if (cfg->state_layout == RBS_STATE_DEFAULT)
            if (const char* m = std::getenv("RBS_STATE")) h->windowed = std::strcmp(m, "dense") != 0;
        h->smalln_target = 2 * std::max(1, prop.multiProcessorCount);   // measured best at 64..500 particles
        if (const char* m = std::getenv("RBS_WIDE_ENTER")) { h->wide_enter = std::atof(m); h->wide_leave = h->wide_enter * 0.67; }
        if (const char* m = std::getenv("RBS_TIMING_EVERY")) h->timing_every = std::max(1, std::atoi(m));
        if (const char* m = std::getenv("RBS_UPLOAD_CHUNKS")) h->upload_chunks = std::min(16, std::max(1, std::atoi(m)));
        if (h->cols & 3) h->windowed = false;   // windows move whole float4s
        h->base.rect_align = h->windowed ? rbs::kRectAlignWindowed : rbs::kRectAlign;
        // whole planes: the big copy kernel must run BESIDE the raster kernel, and three raster
        // blocks per CU hold 504 of a SIMD's 512 VGPRs -- two leave room for the copy waves
        if (!h->windowed && !std::getenv("RBS_RASTER_BLOCKS")) h->raster_blocks = 2 * std::max(1, prop.multiProcessorCount);
    }
    if (int32_t rc = upload(h, &h->d_soup, mesh.soup)) return rc;
    B.soup = h->d_soup;
    RBS_HIP(h, hipMalloc(&h->d_frame, plane));
    if (h->precision == RBS_PRECISION_F64) {   // F32 derives the per-pixel terms from the observation on the fly
        RBS_HIP(h, hipMalloc(&h->d_aux, sizeof(double) * rbs::AUX_PLANES * (size_t)h->npx));
        RBS_HIP(h, hipMalloc(&h->d_aux_slot[0], sizeof(double) * rbs::AUX_PLANES * (size_t)h->npx));
        RBS_HIP(h, hipMalloc(&h->d_aux_slot[1], sizeof(double) * rbs::AUX_PLANES * (size_t)h->npx));
        RBS_HIP(h, hipMalloc(&h->d_pbg, plane));
    }
    RBS_HIP(h, hipMalloc(&h->d_render, plane));
    {   // the occlusion bookkeeping: the caller's choice; left open, the library's (tooling: RBS_OCC=reference|device in the
        // environment replaces DEFAULT only, never a mode the caller named)
        int mode = cfg->occlusion_mode;
        // (a pixel's age must fit 16 bits: c^(65 534 delta_time) <= 2^-40, i.e. the process forgets within the counter's range -- with the
        // reference's constants after 1 628 frames; a process that nearly never forgets, c = p_oo - p_ov above ~0.987 at 30 frames/s, cannot
        // be kept exactly this way)
        const bool ages_fit = std::exp((65534.0 * h->delta_time) * std::log(h->p_oo - h->p_ov)) <= kExactTau;
        const bool can = h->precision == RBS_PRECISION_F64 && h->windowed && ages_fit;
        if (mode == RBS_OCC_REFERENCE && h->precision == RBS_PRECISION_F64 && h->windowed && !ages_fit)
            return fail(h, RBS_ERR_UNSUPPORTED, fmt("occlusion_mode REFERENCE keeps a 16-bit age per pixel: with p_occluded_occluded - p_occluded_visible = %.6g and "
                                                    "delta_time = %.6g a value has not decayed to 2^-40 of itself after 65 534 frames", h->p_oo - h->p_ov, h->delta_time));
        if (mode == RBS_OCC_DEFAULT) {
            mode = RBS_OCC_LIBRARY_DEFAULT;
            if (const char* m = std::getenv("RBS_OCC")) mode = !std::strcmp(m, "reference") ? RBS_OCC_REFERENCE : !std::strcmp(m, "device") ? RBS_OCC_DEVICE_RULE : mode;
            if (mode == RBS_OCC_REFERENCE && !can) mode = RBS_OCC_DEVICE_RULE;
        } else if (mode == RBS_OCC_REFERENCE && !can) {
            return fail(h, RBS_ERR_UNSUPPORTED, "occlusion_mode REFERENCE needs the binary64 likelihood (likelihood_precision F64) and the windowed "
                                                "state layout (cols a multiple of 4)");
        }
        h->exact = mode == RBS_OCC_REFERENCE;
    }
    if (h->exact) {
        // the propagation table: entry a = the two terms of oracle orc_propagate that depend on the elapsed time a * delta_time alone
        const double cc = h->p_oo - h->p_ov, lc = std::log(cc);
        int K = 0;
        while (K < 65534 && std::exp(((double)K * h->delta_time) * lc) > kExactTau) ++K;
        h->age_max = K;
        h->ptab.resize(2 * (size_t)(K + 1));
        for (int a = 0; a <= K; ++a) {
            const double dt = (double)a * h->delta_time;
            const double pow_c = std::exp(dt * lc);
            h->ptab[2 * a] = pow_c;
            h->ptab[2 * a + 1] = (1.0 - h->p_oo) * (pow_c - 1.0) / (cc - 1.0);
        }
        RBS_HIP(h, hipMalloc(&h->d_ptab, sizeof(double) * h->ptab.size()));
        RBS_HIP(h, hipMemcpy(h->d_ptab, h->ptab.data(), sizeof(double) * h->ptab.size(), hipMemcpyHostToDevice));
        RBS_HIP(h, hipMalloc(&h->d_tmp_plane, plane));
    }
    // slabs apply to windowed planes only; a slab as large as a plane is a plane
    h->slab_px = 0;
    if (h->windowed && cfg->state_slab_px > 0 && cfg->state_slab_px < h->npx)
        h->slab_px = std::max(1024, (cfg->state_slab_px + 3) & ~3);
    else if (h->windowed && cfg->state_slab_px == 0 && h->max_particles > 8192 && (h->cols & 3) == 0 && h->npx / 8 >= 4096) {
        // many particles, nothing asked for: an eighth of a plane per slot (8x the particles in the same
        // memory, the same numbers); the slabs grow when a region comes close to filling one
        h->slab_px = (h->npx / 8 + 3) & ~3;
        h->slab_auto = true;
    }
    if (h->slab_px >= h->npx) h->slab_px = 0;
    h->plane_stride = h->slab_px ? (size_t)h->slab_px : (size_t)h->npx;
    if (h->exact) h->plane_stride = exact_stride(h->plane_stride);   // (the slots' ages follow their values)
    const size_t occ_slots = h->occ_slots > 0 ? (size_t)h->occ_slots : (size_t)h->max_particles;
    RBS_HIP(h, hipMalloc(&h->d_occ[0], occ_alloc_bytes(sizeof(float) * h->plane_stride * occ_slots)));
    RBS_HIP(h, hipMalloc(&h->d_occ[1], occ_alloc_bytes(sizeof(float) * h->plane_stride * occ_slots)));
    RBS_HIP(h, hipMalloc(&h->d_err, 2 * sizeof(int)));
    RBS_HIP(h, hipMemset(h->d_err, 0, 2 * sizeof(int)));
    RBS_HIP(h, hipHostMalloc(&h->h_err, 4 * sizeof(int), hipHostMallocDefault));
    h->h_err[0] = h->h_err[1] = h->h_err[2] = h->h_err[3] = 0;
    RBS_HIP(h, hipMalloc(&h->d_bbox, sizeof(int) * 4));
    if (h->slab_px) {
        RBS_HIP(h, hipMalloc(&h->d_reg[0], sizeof(int4) * (size_t)h->max_particles));
        RBS_HIP(h, hipMalloc(&h->d_reg[1], sizeof(int4) * (size_t)h->max_particles));
    }
    RBS_HIP(h, hipMalloc(&h->d_poses, sizeof(double) * 12 * h->n_bodies * (size_t)h->max_particles));
    RBS_HIP(h, hipMalloc(&h->d_indices, sizeof(int) * (size_t)h->max_particles));
    RBS_HIP(h, hipMalloc(&h->d_rects[0], sizeof(int) * 4 * (size_t)h->max_particles));
    RBS_HIP(h, hipMalloc(&h->d_rects[1], sizeof(int) * 4 * (size_t)h->max_particles));
    if (h->n_bodies > 1) {
        RBS_HIP(h, hipMalloc(&h->d_groups[0], sizeof(rbs::Groups) * (size_t)h->max_particles));
        RBS_HIP(h, hipMalloc(&h->d_groups[1], sizeof(rbs::Groups) * (size_t)h->max_particles));
        if (const char* e = std::getenv("RBS_COPY_WALK")) h->copy_walk = std::atoi(e) != 0;
        if (h->windowed)
            for (int k = 0; k < 2; ++k) RBS_HIP(h, hipMalloc(&h->d_strips[k], sizeof(rbs::Strips) * (size_t)h->max_particles));
    }
    RBS_HIP(h, hipMalloc(&h->d_parents[0], sizeof(int) * (size_t)h->max_particles));
    RBS_HIP(h, hipMalloc(&h->d_parents[1], sizeof(int) * (size_t)h->max_particles));
    RBS_HIP(h, hipMalloc(&h->d_win[0], sizeof(int4) * (size_t)h->max_particles));
    RBS_HIP(h, hipMalloc(&h->d_win[1], sizeof(int4) * (size_t)h->max_particles));
    RBS_HIP(h, hipMalloc(&h->d_win_used, sizeof(int4) * (size_t)h->max_particles));
    RBS_HIP(h, hipMalloc(&h->d_item_range, sizeof(int2) * (size_t)h->max_particles));
    RBS_HIP(h, hipMalloc(&h->d_area, sizeof(unsigned long long)));
    RBS_HIP(h, hipHostMalloc(&h->h_area, sizeof(unsigned long long), hipHostMallocDefault));
    RBS_HIP(h, hipEventCreateWithFlags(&h->ev_area, hipEventDisableTiming));
    RBS_HIP(h, hipMalloc(&h->d_ctr, sizeof(int) * 8));
    RBS_HIP(h, hipMemset(h->d_ctr, 0, sizeof(int) * 8));
    RBS_HIP(h, hipMalloc(&h->d_done, sizeof(int) * (size_t)h->max_particles));
    if (int32_t rc = upload(h, &h->d_cluster_sphere, mesh.cluster_sphere)) return rc;
    B.cluster_sphere = h->d_cluster_sphere;
    if (int32_t rc = upload(h, &h->d_cluster_cone, mesh.cluster_cone)) return rc;
    B.cluster_cone = h->d_cluster_cone;
    if (int32_t rc = upload(h, &h->d_cluster_vtx, mesh.cluster_vtx)) return rc;
    B.cluster_vtx = h->d_cluster_vtx;
    if (int32_t rc = upload(h, &h->d_cluster_nv, mesh.cluster_nv)) return rc;
    B.cluster_nv = h->d_cluster_nv;
    if (int32_t rc = upload(h, &h->d_tri_local, mesh.tri_local)) return rc;
    B.tri_local = h->d_tri_local;
    if (int32_t rc = upload(h, &h->d_tri_plane, mesh.tri_plane)) return rc;
    B.tri_plane = reinterpret_cast<const rbs::floatx4*>(h->d_tri_plane);
    if (int32_t rc = upload(h, &h->d_vtx, mesh.vtx, 4)) return rc;   // float32 copy of the vertices, per body (screen rectangles)
    B.vtx = reinterpret_cast<const rbs::floatx4*>(h->d_vtx);
    RBS_HIP(h, hipStreamCreateWithFlags(&h->up_stream, hipStreamNonBlocking));
    for (int k = 0; k < 2; ++k) {
        RBS_HIP(h, hipHostMalloc(&h->h_frames[k], plane, hipHostMallocPortable));   // (every device of a group uploads from shard 0's)
        if (hipHostGetDevicePointer((void**)&h->h_frames_dev[k], h->h_frames[k], 0) != hipSuccess) { (void)hipGetLastError(); h->h_frames_dev[k] = nullptr; }
        RBS_HIP(h, hipEventCreateWithFlags(&h->ev_frame[k], hipEventDisableTiming));
        RBS_HIP(h, hipEventCreateWithFlags(&h->ev_used[k], hipEventDisableTiming));
        if (k == 0) RBS_HIP(h, hipEventCreateWithFlags(&h->ev_reader, hipEventDisableTiming));
        RBS_HIP(h, hipMalloc(&h->d_fin[k], plane));
    }
    {
        const size_t pose_bytes = sizeof(double) * 12 * h->n_bodies * (size_t)h->max_particles;
        h->in_idx_off = pose_bytes;
        const size_t in_bytes = pose_bytes + sizeof(int) * (size_t)h->max_particles;
        RBS_HIP(h, hipHostMalloc(&h->h_in, in_bytes, hipHostMallocDefault));
        RBS_HIP(h, hipHostMalloc(&h->h_out, sizeof(double) * (size_t)h->max_particles, hipHostMallocDefault));
        RBS_HIP(h, hipHostGetDevicePointer(reinterpret_cast<void**>(&h->h_in_dev), h->h_in, 0));
        RBS_HIP(h, hipHostGetDevicePointer(reinterpret_cast<void**>(&h->h_out_dev), h->h_out, 0));
        RBS_HIP(h, hipMalloc(&h->d_in, in_bytes));
        RBS_HIP(h, hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming));
    }

    // the raster / render kernels carve the LDS depth tile from dynamic shared memory
    {
        // (every instantiation of these families: launch_raster's flags, counted through)
        const void* kernels[5 * 4 + 16];
        constexpr int cap = (int)(sizeof kernels / sizeof *kernels);
        int n_kernels = 0;
        auto add = [&](auto* kernel) { if (n_kernels < cap) kernels[n_kernels] = reinterpret_cast<const void*>(kernel); ++n_kernels; };
        for (int k = 0; k < 4; ++k)
            with_flags([&](auto U, auto S) {
                add(&rbs::rbs_raster_kernel_f64<U(), S()>); add(&rbs::rbs_raster_kernel_f32<U(), S()>);
                add(&rbs::rbs_raster_kernel_many_f64<U(), S()>); add(&rbs::rbs_raster_kernel_many_f32<U(), S()>);
                add(&rbs::rbs_raster_kernel_one_f64<U(), S()>);
            }, bool(k & 2), bool(k & 1));
        for (int k = 0; k < 16 && h->exact; ++k)
            with_flags([&](auto U, auto S, auto M, auto T) { add(&rbs::rbs_raster_kernel_exact_f64<U(), S(), M(), T()>); },
                       bool(k & 8), bool(k & 4), bool(k & 2), bool(k & 1));
        if (n_kernels > cap)   // (a family added above without enlarging the list: every rbs_create fails, so no test can miss it)
            return fail(h, RBS_ERR_UNSUPPORTED, fmt("create: %d kernels need the larger dynamic-LDS limit, the list holds %d", n_kernels, cap));
        for (int k = 0; k < n_kernels; ++k)
            RBS_HIP(h, hipFuncSetAttribute(kernels[k], hipFuncAttributeMaxDynamicSharedMemorySize, (int)rbs::smem_bytes(rbs::kTilePxBig, false, true)));
    }
    RBS_HIP(h, rbs::pose_planes_configure());
    RBS_HIP(h, rbs::objmap_configure());

    {   // per-item partial sums: sized for the default tiling so no call ever allocates
        const size_t gmul = h->d_groups[0] ? rbs::kMaxGroups : 1;   // every group of bodies tiles its own rectangle
        size_t need = gmul * (size_t)h->max_particles * tiles_upper_bound(h->cols, h->rows, 256, h->exact ? rbs::kTilePxExact : h->split ? rbs::kDepthTilePx : rbs::kTilePx);
        for (int nn = 1; nn < std::min(h->max_particles, h->raster_blocks); nn *= 2) {
            const int th = std::max(4, rbs::kTilePx / 256 / std::max(1, std::max(h->smalln_target, h->raster_blocks) / nn));
            need = std::max(need, gmul * (size_t)std::min(2 * nn, h->max_particles) * tiles_upper_bound(h->cols, h->rows, 256, 256 * th));
        }
        RBS_HIP(h, hipMalloc(&h->d_partial, sizeof(double) * need));
        RBS_HIP(h, hipMalloc(&h->d_item_particle, sizeof(int) * need));
        h->partial_cap = need;
    }
    // HIP creates a stream's hardware queue at its first submission: do that now, not inside the
    // first updating call
    hipLaunchKernelGGL(rbs::rbs_fill_kernel, dim3(1), dim3(64), 0, h->copy_stream, h->d_render, (size_t)1, 0.f);
    RBS_HIP(h, hipGetLastError());
    RBS_HIP(h, hipEventRecord(h->ev_fork, h->copy_stream));
    RBS_HIP(h, hipStreamSynchronize(h->copy_stream));
    // no observation yet: every pixel "no reading"
    for (int p = 0; p < h->npx; ++p) staging(h)[p] = NAN;
    if (int32_t rc = upload_frame(h, staging(h))) return rc;
    return rbs_reset(h);
}


// ----------------------------------------------------------------------------- several devices
// Copy a shard's error message up to the group handle the caller holds.
int32_t gfail(rbs_handle* g, rbs_handle* shard, int32_t rc)
{
    g->err = fmt("device %d: %s", shard->device, shard->err.c_str());
    return rc;
}

// A failure after part of a call was enqueued: wait for everything that was enqueued (nothing may
// still be writing when the caller reacts), and refuse further calls until rbs_reset.
int32_t poison(rbs_handle* h, int32_t rc)
{
    const std::string why = h->err;
    std::vector<rbs_handle*> all(h->shards.begin(), h->shards.end());
    if (all.empty()) all.push_back(h);
    for (rbs_handle* sh : all) {
        (void)hipSetDevice(sh->device);
        if (sh->stream) (void)hipStreamSynchronize(sh->stream);
        if (sh->copy_stream) (void)hipStreamSynchronize(sh->copy_stream);
        if (sh->up_stream) (void)hipStreamSynchronize(sh->up_stream);
    }
    (void)hipGetLastError();
    h->poisoned = true;
    h->poison_msg = why;
    h->err = why;
    return rc;
}

// Every shard orders its next call after EVERY shard's previous one: a call reads parents from
// the other shards' current planes (complete only when their previous updating call is) and
// overwrites the buffer the other shards' previous call was still reading.  All waits are
// issued before any shard enqueues (an event waited on is the one last recorded).
int32_t group_begin_call(rbs_handle* g, hipStream_t const* streams, bool update)
{
    const int nd = (int)g->shards.size();
    // the shared trail: ONE decision for every shard of this call (rbs_handle::stp_now), from the largest window fraction any
    // shard has sampled so far
    if (g->stp_leave_pending) {   // the previous call left the shared trail
        g->stp = false;
        g->stp_block_until = g->calls + 4000;
        g->stp_leave_pending = false;
    }
    g->stp_now = rbs_handle::StpNow();
    if (g->windowed && g->stp_allowed) {
        double frac = 0.0;
        for (rbs_handle* h : g->shards) frac = std::max(frac, h->area_frac);
        g->stp_now = stp_decide(g, update, frac);
        if (g->stp_now.rebase >= 0) for (rbs_handle* h : g->shards) h->area_frac = 0.0;
        if (g->stp_now.rebase == -2) { g->stp_leave_pending = true; for (rbs_handle* h : g->shards) h->area_frac = 1.0; }
    }
    g->calls += 1;
    for (int k = 0; k < nd; ++k) {
        g->snap_occ[k] = g->shards[k]->d_occ[g->shards[k]->cur];
        g->snap_win[k] = g->shards[k]->d_win[g->shards[k]->cur];
        g->snap_reg[k] = g->shards[k]->d_reg[g->shards[k]->cur];
    }
    for (int a = 0; a < nd; ++a) {
        rbs_handle* A = g->shards[a];
        RBS_HIP(g, hipSetDevice(A->device));
        for (int b = 0; b < nd; ++b)
            if (b != a) RBS_HIP(g, hipStreamWaitEvent(streams ? streams[a] : A->stream, g->shards[b]->ev_done, 0));
    }
    return RBS_OK;
}

// A shard that evaluates no particle in an updating call still moves its state on with the group -- its copy of the shared
// plane included (entering, stepping, re-basing, leaving: every device's copy stays the same plane).
int32_t advance_empty(rbs_handle* h, bool update)
{
    if (!update) return RBS_OK;
    float alpha, beta;
    occlusion_coeffs(h, h->pending_frames, &alpha, &beta);
    const float bg_new = h->exact ? exact_background(h, h->update_clock + h->pending_frames) : std::fmaf(alpha, h->background, beta);
    rbs_handle* g = h->group;
    if (g && h->windowed && g->stp_allowed) {
        const rbs_handle::StpNow d = g->stp_now;
        if (d.entering || (g->stp && !h->stp && d.rebase != -2)) {
            for (int k = 0; k < 2; ++k)
                if (!h->d_bgp[k]) RBS_HIP(h, hipMalloc(&h->d_bgp[k], sizeof(float) * (h->exact ? exact_stride((size_t)h->npx) : (size_t)h->npx)));
            if (!h->d_bgp_box) RBS_HIP(h, hipMalloc(&h->d_bgp_box, sizeof(int4)));
            hipLaunchKernelGGL(rbs::rbs_fill_kernel, dim3(256), dim3(256), 0, h->stream, h->d_bgp[h->cur], (size_t)h->npx, h->background);
            RBS_HIP(h, hipGetLastError());
            if (h->exact) RBS_HIP(h, hipMemsetAsync(h->d_bgp[h->cur] + h->npx, 0xff, sizeof(unsigned short) * (size_t)h->npx, h->stream));
            h->stp = true;
            h->wide = false;
        }
        if (h->stp) {
            DevParams P = h->base;
            P.alpha = alpha; P.beta = beta; P.bg_new = bg_new;
            P.plane_stride = (int)h->plane_stride;
            P.plane_px = h->slab_px ? h->slab_px : h->npx;
            const unsigned e = (unsigned)std::min(h->pending_frames, 0xffff);
            P.elapsed2 = e | (e << 16);
            int rb = d.rebase;
            const float* occ = nullptr; const int4* win = nullptr; const int4* reg = nullptr;
            if (rb >= 0) {
                const int owner = rb / g->shard_cap;
                occ = g->snap_occ[owner]; win = g->snap_win[owner]; reg = h->slab_px ? g->snap_reg[owner] : (const int4*)nullptr;
                rb -= owner * g->shard_cap;
            }
            if (int32_t rc = launch_bgp_step(h, P, occ, win, reg, rb, h->stream)) return rc;
            if (d.rebase == -2) { h->stp = false; h->area_frac = 1.0; }
        }
    }
    h->background = bg_new;
    h->cur = 1 - h->cur;
    h->update_clock += h->pending_frames;
    h->pending_frames = 0;
    // (h->calls stays: it selects the work-item counters, and a raster kernel zeroes the counters of
    // the call that FOLLOWS it -- a skipped call must not change which pair is next)
    return RBS_OK;
}

int32_t group_load_rccl(rbs_handle* g, const std::vector<int>& devs)
{
    Rccl* r = new Rccl;
    g->rccl = r;
    // a copy the process has loaded already (PyTorch ships its own librccl) before a second one from the ROCm tree
    for (const char* name : {"librccl.so.1", "librccl.so"}) {
        r->lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL | RTLD_NOLOAD);
        if (r->lib) break;
    }
    for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
        if (r->lib) break;
        r->lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
    }
    if (!r->lib) return fail(g, RBS_ERR_UNSUPPORTED, fmt("several devices need RCCL: dlopen(librccl.so.1) failed: %s", dlerror()));
    r->CommInitAll = reinterpret_cast<decltype(r->CommInitAll)>(dlsym(r->lib, "ncclCommInitAll"));
    r->CommDestroy = reinterpret_cast<decltype(r->CommDestroy)>(dlsym(r->lib, "ncclCommDestroy"));
    r->GroupStart = reinterpret_cast<decltype(r->GroupStart)>(dlsym(r->lib, "ncclGroupStart"));
    r->GroupEnd = reinterpret_cast<decltype(r->GroupEnd)>(dlsym(r->lib, "ncclGroupEnd"));
    r->AllGather = reinterpret_cast<decltype(r->AllGather)>(dlsym(r->lib, "ncclAllGather"));
    r->GetErrorString = reinterpret_cast<decltype(r->GetErrorString)>(dlsym(r->lib, "ncclGetErrorString"));
    if (!r->CommInitAll || !r->CommDestroy || !r->GroupStart || !r->GroupEnd || !r->AllGather || !r->GetErrorString)
        return fail(g, RBS_ERR_UNSUPPORTED, "librccl lacks an ncclCommInitAll / ncclAllGather / ncclGroup* symbol");
    r->comms.assign(devs.size(), nullptr);
    const int rc = r->CommInitAll(r->comms.data(), (int)devs.size(), devs.data());
    if (rc != 0) {
        const std::string msg = fmt("ncclCommInitAll over %zu devices failed: %s", devs.size(), r->GetErrorString(rc));
        r->comms.clear();
        return fail(g, RBS_ERR_HIP, msg);
    }
    return RBS_OK;
}

// Every shard gets every shard's `count` doubles: buf[k * count .. ) of shard k's buffer is what
// shard k produced.  RCCL all-gather over xGMI when the devices are distinct (the exchange of the
// log-likelihoods before resampling); plain device-to-device copies when a device appears twice
// in the handle (RCCL refuses that: functional tests on a one-GPU box).
int32_t group_allgather(rbs_handle* g, double* const* bufs, size_t count, hipStream_t const* streams)
{
    const int nd = (int)g->shards.size();
    if (g->rccl && !g->rccl->comms.empty()) {
        Rccl* r = g->rccl;
        int rc = r->GroupStart();
        for (int k = 0; k < nd && rc == 0; ++k)
            rc = r->AllGather(bufs[k] + (size_t)k * count, bufs[k], count, /*ncclDouble*/ 8, r->comms[k], streams[k]);
        const int rc2 = r->GroupEnd();
        if (rc != 0 || rc2 != 0) return fail(g, RBS_ERR_HIP, fmt("ncclAllGather failed: %s", r->GetErrorString(rc ? rc : rc2)));
        return RBS_OK;
    }
    // one event per producer, then every consumer copies every other shard's piece on its own stream
    for (int k = 0; k < nd; ++k) {
        RBS_HIP(g, hipSetDevice(g->shards[k]->device));
        RBS_HIP(g, hipEventRecord(g->shards[k]->ev_fork, streams[k]));
    }
    for (int a = 0; a < nd; ++a) {
        RBS_HIP(g, hipSetDevice(g->shards[a]->device));
        for (int b = 0; b < nd; ++b) {
            if (b == a) continue;
            RBS_HIP(g, hipStreamWaitEvent(streams[a], g->shards[b]->ev_fork, 0));
            RBS_HIP(g, hipMemcpyPeerAsync(bufs[a] + (size_t)b * count, g->shards[a]->device, bufs[b] + (size_t)b * count,
                                          g->shards[b]->device, sizeof(double) * count, streams[a]));
        }
    }
    return RBS_OK;
}

int32_t create_group(const rbs_config* cfg, rbs_handle* g)
{
    const int nd = cfg->n_devices;
    if (nd > rbs::kMaxDevices) return fail(g, RBS_ERR_INVALID_ARGUMENT, fmt("n_devices %d > %d", nd, rbs::kMaxDevices));
    if (!cfg->device_ids) return fail(g, RBS_ERR_INVALID_ARGUMENT, "n_devices > 1 but device_ids is NULL");
    if (cfg->max_particles <= 0) return fail(g, RBS_ERR_INVALID_ARGUMENT, "max_particles must be positive");
    g->max_particles = cfg->max_particles;
    g->shard_cap = (cfg->max_particles + nd - 1) / nd;
    g->rows = cfg->rows; g->cols = cfg->cols; g->npx = cfg->rows * cfg->cols;
    g->n_bodies = cfg->n_objects;
    g->device = cfg->device_ids[0];
    std::vector<int> devs(cfg->device_ids, cfg->device_ids + nd);
    bool distinct = true;
    for (int a = 0; a < nd; ++a)
        for (int b = a + 1; b < nd; ++b)
            if (devs[a] == devs[b]) distinct = false;
    for (int k = 0; k < nd; ++k) {
        rbs_config sub = *cfg;
        sub.device_id = devs[k];
        sub.n_devices = 0;
        sub.device_ids = nullptr;
        sub.max_particles = g->shard_cap;
        rbs_handle* sh = new (std::nothrow) rbs_handle;
        if (!sh) return fail(g, RBS_ERR_OUT_OF_MEMORY, "out of host memory");
        g->shards.push_back(sh);
        sh->group = g;
        sh->shard_index = k;
        sh->shard_cap = g->shard_cap;
        if (int32_t rc = create_impl(&sub, sh)) return gfail(g, sh, rc);
        RBS_HIP(g, hipEventCreateWithFlags(&sh->ev_done, hipEventDisableTiming));
        RBS_HIP(g, hipEventRecord(sh->ev_done, sh->stream));
    }
    g->windowed = g->shards[0]->windowed;
    g->precision = g->shards[0]->precision;
    g->stp_allowed = g->shards[0]->stp_allowed;      // (the shared trail's policy is the group's: one decision per call for every shard)
    g->stp_enter = g->shards[0]->stp_enter;
    g->stp_every = g->shards[0]->stp_every;
    g->wide_enter = g->shards[0]->wide_enter;
#ifdef RBS_TEST_HOOKS   // (librbsensor_mi355x_hooks.so, `make hooks`: the release library carries no fault injection -- ADVICE r3)
    if (const char* f = std::getenv("RBS_TEST_FAULT")) {
        int a = -1; long c = -1;
        if (std::sscanf(f, "%d:%ld", &a, &c) == 2) { g->fault_shard = a; g->fault_call = c; }
    }
#endif
    // parents on another device are read in place
    for (int a = 0; a < nd; ++a) {
        RBS_HIP(g, hipSetDevice(devs[a]));
        for (int b = 0; b < nd; ++b) {
            if (devs[a] == devs[b]) continue;
            int can = 0;
            RBS_HIP(g, hipDeviceCanAccessPeer(&can, devs[a], devs[b]));
            if (!can) return fail(g, RBS_ERR_UNSUPPORTED, fmt("device %d cannot access device %d's memory (peer access)", devs[a], devs[b]));
            const hipError_t e = hipDeviceEnablePeerAccess(devs[b], 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
                (void)hipGetLastError();
                return fail(g, RBS_ERR_HIP, fmt("hipDeviceEnablePeerAccess(%d -> %d): %s", devs[a], devs[b], hipGetErrorString(e)));
            }
            (void)hipGetLastError();
        }
    }
    bool want_rccl = distinct;
#ifdef RBS_TEST_HOOKS   // (hooks library only) RBS_TEST_FORCE_RCCL=1: take the RCCL branch on a one-GPU box too -- ncclCommInitAll refuses a
                        // device that appears twice, which is the failure the fall-back below exists for
    if (const char* e = std::getenv("RBS_TEST_FORCE_RCCL")) want_rccl = want_rccl || std::atoi(e) != 0;
#endif
    if (want_rccl) {
        if (int32_t rc = group_load_rccl(g, devs)) {
            // First contact with a node must not end at the communicator: the exchange is n doubles per block, and the devices can
            // read each other (checked above) -- the peer-copy form of group_allgather does the same job.  RBS_REQUIRE_RCCL=1: fatal.
            const char* req = std::getenv("RBS_REQUIRE_RCCL");
            if (req && std::atoi(req) != 0) return rc;
            std::fprintf(stderr, "[rbsensor_mi355x] RCCL is not used for this handle (%s): log-likelihoods are exchanged by peer copies\n", g->err.c_str());
            if (g->rccl) {
                for (auto c : g->rccl->comms)
                    if (c) (void)g->rccl->CommDestroy(c);
                delete g->rccl;
                g->rccl = nullptr;
            }
            g->err.clear();
        }
    }
    return RBS_OK;
}

void release_group(rbs_handle* g)
{
    if (g->rccl) {
        for (auto c : g->rccl->comms)
            if (c) (void)g->rccl->CommDestroy(c);
        // the library stays loaded: other handles (or torch) may be using it
        delete g->rccl;
        g->rccl = nullptr;
    }
    for (rbs_handle* sh : g->shards) {
        if (sh->ev_done) { (void)hipSetDevice(sh->device); (void)hipStreamSynchronize(sh->stream); (void)hipEventDestroy(sh->ev_done); sh->ev_done = nullptr; }
        release(sh);
    }
    g->shards.clear();
    delete g;
}

// The host-pointer call on one device: poses and parent slots are staged in pinned memory, and
// -- no copy engine involved -- the rectangles kernel pulls them from there over PCIe (writing the
// device copy of the poses the raster kernel reads) and the raster kernel stores the
// log-likelihoods straight into the pinned result buffer.  A separate H2D copy of 200 KB queued
// behind the frame's upload on the same engine, and each copy <-> kernel hand-over costs ~10 us:
// together 30 us of a 300 us step.
// rbs_loglikes_deltas: state deltas + default poses instead of absolute poses (packed on the way into pinned memory,
// composed on the device by the rectangles kernel, rbs_prep_deltas_kernel).
struct DeltaArgs { const double* deltas; const double* deflt; int stride; };

int32_t host_call(rbs_handle* h, const double* poses, const int32_t* indices, int n, bool update, const DeltaArgs* da = nullptr)
{
    const size_t pose_bytes = sizeof(double) * 12 * h->n_bodies * (size_t)n;
    // slabs: the overflow flag as it stands BEFORE this call -- set, it belongs to an asynchronous call
    // that has not been reported yet
    if (h->slab_px) RBS_HIP(h, hipMemcpyAsync(h->h_err + 2, h->d_err, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    if (da) {
        // [n][bodies][6] deltas, then [bodies][6] default poses: half the bytes of the absolute poses they stand for
        // (they fit the staging block sized for those: (n + 1) * 6 <= max_particles * 12)
        const int B = h->n_bodies;
        double* st = reinterpret_cast<double*>(h->h_in);
        const size_t nb = (size_t)n * B;
        if (da->deltas == st) {}   // (rbs_deltas_buffer: the caller gathered straight into the staging block)
        else if (da->stride == 6) std::memcpy(st, da->deltas, sizeof(double) * 6 * nb);
        else for (size_t k = 0; k < nb; ++k) std::memcpy(st + 6 * k, da->deltas + (size_t)da->stride * k, sizeof(double) * 6);
        for (int b = 0; b < B; ++b) std::memcpy(st + 6 * nb + 6 * b, da->deflt + (size_t)da->stride * b, sizeof(double) * 6);
        std::memcpy(h->h_in + h->in_idx_off, indices, sizeof(int) * (size_t)n);
        // (the rectangles kernel composes: the wave that owns a particle reads its 48 bytes per body from here)
        if (int32_t rc = flush_device_frame(h, h->stream)) return rc;   // (a pending device frame: its ingest has no deltas variant)
        if (int32_t rc = enqueue_loglikes(h, reinterpret_cast<const double*>(h->d_in),
                                          reinterpret_cast<const int*>(h->h_in_dev + h->in_idx_off), n, update,
                                          reinterpret_cast<double*>(h->h_out_dev), h->stream, nullptr,
                                          reinterpret_cast<const double*>(h->h_in_dev)))
            return rc;
        if (h->slab_px) RBS_HIP(h, hipMemcpyAsync(h->h_err, h->d_err, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        RBS_HIP(h, hipEventRecord(h->ev_out, h->stream));
        return RBS_OK;
    }
    std::memcpy(h->h_in, poses, pose_bytes);
    std::memcpy(h->h_in + h->in_idx_off, indices, sizeof(int) * (size_t)n);
    if (int32_t rc = enqueue_loglikes(h, reinterpret_cast<const double*>(h->d_in),
                                      reinterpret_cast<const int*>(h->h_in_dev + h->in_idx_off), n, update,
                                      reinterpret_cast<double*>(h->h_out_dev), h->stream,
                                      reinterpret_cast<const double*>(h->h_in_dev)))
        return rc;
    if (h->slab_px) RBS_HIP(h, hipMemcpyAsync(h->h_err, h->d_err, 2 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    RBS_HIP(h, hipEventRecord(h->ev_out, h->stream));
    return RBS_OK;
}

// Slabs of a group: every shard keeps the SAME slab size (a shard addresses its neighbours' planes
// with its own stride).  before != nullptr: a call overflowed -- take it back on every shard first.
// Otherwise housekeeping: enlarge when the largest region asked for on any shard has filled three
// quarters of a slab.  Drains every shard when it acts.
int32_t group_grow_slabs(rbs_handle* g, const std::vector<CallState>* before)
{
    rbs_handle* s0 = g->shards[0];
    if (!s0->slab_px) return RBS_OK;
    int need = 0;
    bool overflowed = false;
    for (rbs_handle* h : g->shards) { need = std::max(need, h->h_err[1]); overflowed = overflowed || h->h_err[0] != 0; }
    if (!before && !overflowed) {   // housekeeping: act (and drain every shard) only when the slabs will really be reallocated
        const int would = (int)std::min<long>(s0->npx, ((long)slab_for(s0, need) + 1023) & ~1023L);
        if ((long)need * 4 <= (long)s0->slab_px * 3 || would <= s0->slab_px) return RBS_OK;
    }
    for (size_t k = 0; k < g->shards.size(); ++k) {
        rbs_handle* h = g->shards[k];
        RBS_HIP(g, hipSetDevice(h->device));
        if (int32_t rc = drain(h, true)) return gfail(g, h, rc);
        if (before) restore_call_state(h, (*before)[k]);
    }
    const int target = slab_for(s0, need);
    for (rbs_handle* h : g->shards) {
        RBS_HIP(g, hipSetDevice(h->device));
        if (int32_t rc = grow_slabs(h, target)) return gfail(g, h, rc);
        if (h->h_err[0]) {
            RBS_HIP(g, hipMemsetAsync(h->d_err, 0, sizeof(int), h->stream));
            h->h_err[0] = 0;
        }
        RBS_HIP(g, hipStreamSynchronize(h->stream));
        RBS_HIP(g, hipEventRecord(h->ev_done, h->stream));
    }
    return RBS_OK;
}

// rbs_loglikes on a group: particle i is evaluated by shard i / shard_cap and (update) written
// to global slot i; `indices` are global parent slots.
int32_t group_loglikes(rbs_handle* g, const double* poses, int32_t* indices, int32_t n, int32_t update, double* out, const DeltaArgs* da = nullptr)
{
    const int nd = (int)g->shards.size();
    const int cap = g->shard_cap;
    for (int32_t i = 0; i < n; ++i)
        if (indices[i] < 0 || indices[i] >= nd * cap)
            return fail(g, RBS_ERR_INVALID_ARGUMENT, fmt("loglikes: indices[%d] = %d outside 0..%d", i, indices[i], nd * cap - 1));
    std::vector<CallState> before;
    for (rbs_handle* h : g->shards) before.push_back(save_call_state(h));
    const CallState gbefore = save_call_state(g);      // (the shared trail's state is the group's)
    const bool gleave = g->stp_leave_pending;
    const size_t stride = (size_t)12 * g->n_bodies;
    bool stale_overflow = false;
    for (int attempt = 0; attempt < 2; ++attempt) {
        // from here on a failure leaves some shards advanced and others not: the group is poisoned
        if (int32_t rc = group_begin_call(g, nullptr, update != 0)) return poison(g, rc);
        for (int k = 0; k < nd; ++k) {
            rbs_handle* h = g->shards[k];
            const int lo = std::min(n, k * cap), cnt = std::min(n, (k + 1) * cap) - lo;
            if (hipSetDevice(h->device) != hipSuccess) return poison(g, fail(g, RBS_ERR_HIP, fmt("hipSetDevice(%d) failed", h->device)));
            if (cnt <= 0) {
                if (int32_t rc = advance_empty(h, update != 0)) return poison(g, gfail(g, h, rc));
                if (hipEventRecord(h->ev_done, h->stream) != hipSuccess) return poison(g, fail(g, RBS_ERR_HIP, "hipEventRecord failed"));
                continue;
            }
#ifdef RBS_TEST_HOOKS
            if (k == g->fault_shard && g->group_calls == g->fault_call) {   // (test hook)
                g->group_calls += 1;
                return poison(g, gfail(g, h, fail(h, RBS_ERR_HIP, "injected fault (RBS_TEST_FAULT)")));
            }
#endif
            DeltaArgs dk = {nullptr, nullptr, 0};
            if (da) dk = DeltaArgs{da->deltas + (size_t)da->stride * g->n_bodies * (size_t)lo, da->deflt, da->stride};
            if (int32_t rc = host_call(h, da ? nullptr : poses + stride * (size_t)lo, indices + lo, cnt, update != 0, da ? &dk : nullptr))
                return poison(g, gfail(g, h, rc));
        }
        g->group_calls += 1;
        bool overflow = false;
        for (int k = 0; k < nd; ++k) {
            rbs_handle* h = g->shards[k];
            const int lo = std::min(n, k * cap), cnt = std::min(n, (k + 1) * cap) - lo;
            if (cnt <= 0) continue;
            if (hipSetDevice(h->device) != hipSuccess || hipEventSynchronize(h->ev_out) != hipSuccess)
                return poison(g, fail(g, RBS_ERR_HIP, fmt("device %d: waiting for the log-likelihoods failed", h->device)));
            std::memcpy(out + lo, h->h_out, sizeof(double) * (size_t)cnt);
            overflow = overflow || (h->slab_px && h->h_err[0]);
            // the flag as it stood BEFORE this call (host_call fetches it): set, it belongs to an asynchronous call whose
            // results were NaN and which has not been reported yet -- repaired below like this call's own, but REPORTED
            if (attempt == 0 && h->slab_px && h->h_err[2]) stale_overflow = true;
        }
        if (!overflow) break;
        if (attempt == 1) return gfail(g, g->shards[0], check_slab_error(g->shards[0]));
        // a region did not fit its slab on some shard: the whole call is taken back on every shard
        // (the planes it read are intact), every shard's slabs are enlarged alike -- a shard reads
        // its neighbours' planes with its own stride -- and the call runs again
        if (int32_t rc = group_grow_slabs(g, &before)) return poison(g, rc);
        restore_call_state(g, gbefore);
        g->stp_leave_pending = gleave;
    }
    if (update)
        for (int32_t i = 0; i < n; ++i) indices[i] = i;
    if (int32_t rc = group_grow_slabs(g, nullptr)) return rc;   // (housekeeping: enlarge before a region fills a slab)
    if (stale_overflow) {   // this call's numbers are good; an earlier asynchronous call's were not (single-device path: the same, once)
        rbs_handle* s0 = g->shards[0];
        s0->h_err[0] = 1;
        const int32_t rc = check_slab_error(s0);
        s0->h_err[0] = 0;
        return gfail(g, s0, rc);
    }
    return RBS_OK;
}

// rbs_set_observation_device on a group: `d_depth` lives on the handle's FIRST device; every shard
// ingests it from there (its ingest kernel reads the 1.2 MB over xGMI, peer access) once the work
// enqueued on the caller's stream so far -- whatever produced the frame -- has run.
int32_t group_set_observation_device(rbs_handle* g, const float* d_depth, hipStream_t stream)
{
    rbs_handle* s0 = g->shards[0];
    RBS_HIP(g, hipSetDevice(s0->device));
    hipStream_t cs = stream ? stream : s0->stream;
    RBS_HIP(g, hipEventRecord(s0->ev_reader, cs));
    for (size_t k = 0; k < g->shards.size(); ++k) {
        rbs_handle* h = g->shards[k];
        if (hipSetDevice(h->device) != hipSuccess) return poison(g, fail(g, RBS_ERR_HIP, fmt("hipSetDevice(%d) failed", h->device)));
        if (int32_t rc = flush_device_frame(h, h->stream)) return k == 0 ? gfail(g, h, rc) : poison(g, gfail(g, h, rc));
        if (int32_t rc = hand_over_device(h, d_depth, h->stream)) return k == 0 ? gfail(g, h, rc) : poison(g, gfail(g, h, rc));
        if (hipStreamWaitEvent(h->stream, s0->ev_reader, 0) != hipSuccess) return poison(g, fail(g, RBS_ERR_HIP, "hipStreamWaitEvent failed"));
    }
    return RBS_OK;
}

// rbs_loglikes_device on a group: poses / parent slots / results are arrays on the handle's FIRST
// device in global particle order; shard k evaluates particles [k cap, (k+1) cap) on its own stream
// -- its rectangles kernel pulls its slice of the poses and parent slots over xGMI (the route the
// host-pointer call uses for pinned memory), its raster kernel stores its log-likelihoods into the
// caller's array in place -- after the work enqueued on the caller's stream so far, and the caller's
// stream is ordered after every shard: d_out is complete in `stream` order, nothing synchronises
// with the host.
int32_t group_loglikes_device(rbs_handle* g, const double* d_poses, const int32_t* d_indices, int32_t n, int32_t update,
                              double* d_out, hipStream_t stream)
{
    const int nd = (int)g->shards.size(), cap = g->shard_cap;
    rbs_handle* s0 = g->shards[0];
    RBS_HIP(g, hipSetDevice(s0->device));
    hipStream_t cs = stream ? stream : s0->stream;
    RBS_HIP(g, hipEventRecord(s0->ev_reader, cs));           // the producers of poses / indices on the caller's stream
    for (int k = 0; k < nd; ++k) {
        RBS_HIP(g, hipSetDevice(g->shards[k]->device));
        RBS_HIP(g, hipStreamWaitEvent(g->shards[k]->stream, s0->ev_reader, 0));
    }
    // from here on a failure leaves some shards advanced and others not: the group is poisoned
    if (int32_t rc = group_begin_call(g, nullptr, update != 0)) return poison(g, rc);
    const size_t stride = (size_t)12 * g->n_bodies;
    for (int k = 0; k < nd; ++k) {
        rbs_handle* h = g->shards[k];
        const int lo = std::min(n, k * cap), cnt = std::min(n, (k + 1) * cap) - lo;
        if (hipSetDevice(h->device) != hipSuccess) return poison(g, fail(g, RBS_ERR_HIP, fmt("hipSetDevice(%d) failed", h->device)));
        if (cnt <= 0) {
            if (int32_t rc = advance_empty(h, update != 0)) return poison(g, gfail(g, h, rc));
            if (hipEventRecord(h->ev_done, h->stream) != hipSuccess) return poison(g, fail(g, RBS_ERR_HIP, "hipEventRecord failed"));
            continue;
        }
        if (int32_t rc = enqueue_loglikes(h, reinterpret_cast<const double*>(h->d_in), d_indices + lo, cnt, update != 0, d_out + lo,
                                          h->stream, d_poses + stride * (size_t)lo))
            return poison(g, gfail(g, h, rc));
    }
    if (hipSetDevice(s0->device) != hipSuccess) return poison(g, fail(g, RBS_ERR_HIP, "hipSetDevice failed"));
    for (int k = 0; k < nd; ++k)
        if (hipStreamWaitEvent(cs, g->shards[k]->ev_done, 0) != hipSuccess) return poison(g, fail(g, RBS_ERR_HIP, "hipStreamWaitEvent failed"));
    return RBS_OK;
}

// Route a global slot to its shard.
rbs_handle* shard_of(rbs_handle* g, int32_t slot, int32_t* local)
{
    const int k = slot / g->shard_cap;
    *local = slot - k * g->shard_cap;
    return g->shards[k];
}
#define RBS_GROUP_SLOT(h, slot, call)                                                         \
    do {                                                                                      \
        if (!(h)->shards.empty()) {                                                           \
            if ((slot) < 0 || (slot) >= (int)(h)->shards.size() * (h)->shard_cap)             \
                return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("bad slot %d", (int)(slot)));    \
            int32_t l_;                                                                       \
            rbs_handle* sh_ = shard_of(h, slot, &l_);                                         \
            const int32_t rc_ = call;                                                         \
            return rc_ ? gfail(h, sh_, rc_) : RBS_OK;                                         \
        }                                                                                     \
    } while (0)
#define RBS_GROUP_ALL(h, call)                                                                \
    do {                                                                                      \
        if (!(h)->shards.empty()) {                                                           \
            for (rbs_handle* sh_ : (h)->shards) {                                             \
                const int32_t rc_ = call;                                                     \
                if (rc_) return gfail(h, sh_, rc_);                                           \
            }                                                                                 \
            return RBS_OK;                                                                    \
        }                                                                                     \
    } while (0)
// A call that changes every shard's state: a failure on the first shard (argument errors land
// there) changed nothing; one on a later shard leaves the shards out of step -> poisoned.
#define RBS_GROUP_ALL_MUT(h, call)                                                            \
    do {                                                                                      \
        if (!(h)->shards.empty()) {                                                           \
            for (size_t k_ = 0; k_ < (h)->shards.size(); ++k_) {                              \
                rbs_handle* sh_ = (h)->shards[k_];                                            \
                const int32_t rc_ = call;                                                     \
                if (rc_) return k_ == 0 ? gfail(h, sh_, rc_) : poison(h, gfail(h, sh_, rc_)); \
            }                                                                                 \
            return RBS_OK;                                                                    \
        }                                                                                     \
    } while (0)
#define RBS_GROUP_FIRST(h, call)                                                              \
    do {                                                                                      \
        if (!(h)->shards.empty()) {                                                           \
            rbs_handle* sh_ = (h)->shards[0];                                                 \
            const int32_t rc_ = call;                                                         \
            return rc_ ? gfail(h, sh_, rc_) : RBS_OK;                                         \
        }                                                                                     \
    } while (0)

}  // namespace

extern "C" {

int32_t rbs_abi_version(void) { return RBS_ABI_VERSION; }

int32_t rbs_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* rbs_last_error(const rbs_handle* h)
{
    return h ? h->err.c_str() : g_create_error.c_str();
}

int32_t rbs_create(const rbs_config* cfg, rbs_handle** out)
{
    if (!out) { g_create_error = "rbs_create: out is NULL"; return RBS_ERR_INVALID_ARGUMENT; }
    *out = nullptr;
    if (!cfg) { g_create_error = "rbs_create: cfg is NULL"; return RBS_ERR_INVALID_ARGUMENT; }
    rbs_handle* h = new (std::nothrow) rbs_handle;
    if (!h) { g_create_error = "rbs_create: out of host memory"; return RBS_ERR_OUT_OF_MEMORY; }
    int32_t rc;
    const bool group = cfg->n_devices > 1 || (cfg->n_devices == 1 && cfg->device_ids && std::getenv("RBS_GROUP_SINGLE"));
    try {
        rc = group ? (cfg->abi_version != RBS_ABI_VERSION
                          ? fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("abi_version %d, library is %d", cfg->abi_version, RBS_ABI_VERSION))
                          : create_group(cfg, h))
                   : create_impl(cfg, h);
    } catch (const std::exception& e) {
        h->err = std::string("rbs_create: ") + e.what();
        rc = RBS_ERR_OUT_OF_MEMORY;
    }
    if (rc != RBS_OK) {
        g_create_error = h->err;
        if (group) release_group(h); else release(h);
        return rc;
    }
    *out = h;
    return RBS_OK;
}

void rbs_destroy(rbs_handle* h)
{
    if (h && !h->shards.empty()) release_group(h);
    else release(h);
}

int32_t rbs_reset(rbs_handle* h)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!h->shards.empty()) {
        for (rbs_handle* sh_ : h->shards)
            if (int32_t rc_ = rbs_reset(sh_)) return gfail(h, sh_, rc_);
        for (rbs_handle* sh_ : h->shards) {   // idle streams: a clean slate for the group's call ordering
            RBS_HIP(h, hipSetDevice(sh_->device));
            RBS_HIP(h, hipEventRecord(sh_->ev_done, sh_->stream));
        }
        h->poisoned = false;
        frame_abandon(h);
        h->stp = false;
        h->stp_leave_pending = false;
        h->stp_now = rbs_handle::StpNow();
        h->stp_last_rebase = -1000000;
        h->stp_block_until = 0;
        h->calls = 0;
        return RBS_OK;
    }
    RBS_HIP(h, hipSetDevice(h->device));
    if (int32_t rc = drain(h, true)) return rc;   // no copy kernel may still be writing planes
    // (a call that failed between its kernels may have left the work-item counters of either parity
    // in use: both pairs start from zero again)
    RBS_HIP(h, hipMemsetAsync(h->d_ctr, 0, 8 * sizeof(int), h->stream));
    h->poisoned = false;
    frame_abandon(h);
    h->stp = false;            // (every plane is all background again: the scalar says it all)
    h->stp_request = -1;
    h->stp_last_rebase = -1000000;
    h->stp_block_until = 0;
    h->area_frac = 0.0;
    h->cur = 0;
    h->pending_frames = 0;
    h->update_clock = 0;
    h->background = (float)h->init_occ;
    {   // windowed: every plane is all background (empty window); dense: full windows for ever
        const int4 w0 = h->windowed ? make_int4(h->cols, h->rows, 0, 0) : make_int4(0, 0, h->cols, h->rows);
        const unsigned g = (unsigned)((h->max_particles + 255) / 256);
        for (int b = 0; b < 2; ++b)
            hipLaunchKernelGGL(rbs::rbs_set_window_kernel, dim3(g), dim3(256), 0, h->stream, h->d_win[b],
                               h->max_particles, w0);
    }
    if (h->slab_px) {
        const unsigned g = (unsigned)((h->max_particles + 255) / 256);
        for (int b = 0; b < 2; ++b)
            hipLaunchKernelGGL(rbs::rbs_set_window_kernel, dim3(g), dim3(256), 0, h->stream, h->d_reg[b],
                               h->max_particles, make_int4(h->cols, h->rows, 0, 0));
    }
    RBS_HIP(h, hipMemsetAsync(h->d_err, 0, 2 * sizeof(int), h->stream));
    h->h_err[0] = h->h_err[1] = 0;
    const size_t n = h->plane_stride * (h->occ_slots > 0 ? (size_t)h->occ_slots : (size_t)h->max_particles);
    hipLaunchKernelGGL(rbs::rbs_fill_kernel, dim3(2048), dim3(256), 0, h->stream, h->d_occ[0], n,
                       (float)h->init_occ);
    // the second buffer too: touches every page now instead of inside the first updating call
    hipLaunchKernelGGL(rbs::rbs_fill_kernel, dim3(2048), dim3(256), 0, h->stream, h->d_occ[1], n,
                       (float)h->init_occ);
    RBS_HIP(h, hipGetLastError());
    if (int32_t rc = drain(h, true)) return rc;
    return RBS_OK;
}

// rbs_set_observation / _f32 (`what`: the entry point's name in its messages): the caller's host frame, copied now.
static int32_t set_host_frame(rbs_handle* h, const float* f32, const double* f64, size_t n, const char* what)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (int32_t rc = frame_begin(h)) return rc;
    RBS_GROUP_ALL_MUT(h, set_host_frame(sh_, f32, f64, n, what));
    if ((!f32 && !f64) || n != (size_t)h->npx)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("%s: expected %d pixels, got %zu", what, h->npx, n));
    if (int32_t rc = frame_ready(h, h->stream)) return rc;
    return hand_over_host(h, f32, f64);
}

// rbs_set_observation_borrowed / _f32: handles that cannot stage between two kernels (several devices; float32 likelihood;
// whole planes) copy at once.
static int32_t set_borrowed_frame(rbs_handle* h, const float* f32, const double* f64, size_t n, const char* what)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!can_borrow(h)) return set_host_frame(h, f32, f64, n, f64 ? "set_observation" : "set_observation_f32");
    if (int32_t rc = frame_begin(h)) return rc;
    if ((!f32 && !f64) || n != (size_t)h->npx)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("%s: expected %d pixels, got %zu", what, h->npx, n));
    if (int32_t rc = frame_ready(h, h->stream)) return rc;
    hand_over_borrowed(h, f32, f64);
    return RBS_OK;
}

int32_t rbs_set_observation(rbs_handle* h, const double* depth, size_t n)
{
    return set_host_frame(h, nullptr, depth, n, "set_observation");   // (converted and sent piece by piece)
}
int32_t rbs_set_observation_f32(rbs_handle* h, const float* depth, size_t n)
{
    return set_host_frame(h, depth, nullptr, n, "set_observation_f32");
}
int32_t rbs_set_observation_borrowed(rbs_handle* h, const double* depth, size_t n)
{
    return set_borrowed_frame(h, nullptr, depth, n, "set_observation_borrowed");
}
int32_t rbs_set_observation_borrowed_f32(rbs_handle* h, const float* depth, size_t n)
{
    return set_borrowed_frame(h, depth, nullptr, n, "set_observation_borrowed_f32");
}

int32_t rbs_acquire_frame_buffer(rbs_handle* h, float** buf)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!buf) return fail(h, RBS_ERR_INVALID_ARGUMENT, "acquire_frame_buffer: null pointer");
    RBS_REFUSE_POISONED(h);
    if (h->fr.acquired)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "acquire_frame_buffer: the buffer handed out last has not been committed (rbs_commit_frame_buffer)");
    return acquire_staging(h, buf);
}

int32_t rbs_commit_frame_buffer(rbs_handle* h)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_REFUSE_POISONED(h);
    // a commit uploads the buffer the matching acquire handed out: without one (or after another
    // rbs_set_observation* call took the acquire's place) there is nothing defined to upload, and the
    // upload would land in the image the kernels in flight are reading
    if (!h->fr.acquired)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "commit_frame_buffer: no buffer acquired (rbs_acquire_frame_buffer comes first, once per frame)");
    if (int32_t rc = frame_begin(h)) return rc;
    if (!h->shards.empty()) {
        const float* src = staging(h->shards[0]);
        for (rbs_handle* sh : h->shards) {
            if (int32_t rc = frame_ready(sh, sh->stream)) return poison(h, gfail(h, sh, rc));
            if (int32_t rc = hand_over_pinned(sh, src)) return poison(h, gfail(h, sh, rc));
        }
        return RBS_OK;
    }
    if (int32_t rc = frame_ready(h, h->stream)) return rc;
    return hand_over_pinned(h, staging(h));
}

int32_t rbs_set_observation_native_f32(rbs_handle* h, const float* native, int32_t width,
                                       int32_t height, int32_t f)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (int32_t rc = frame_begin(h)) return rc;
    RBS_GROUP_ALL_MUT(h, rbs_set_observation_native_f32(sh_, native, width, height, f));
    if (!native || f <= 0 || width <= 0 || height <= 0 || height / f != h->rows || width / f != h->cols)
        return fail(h, RBS_ERR_INVALID_ARGUMENT,
                    fmt("set_observation_native: %dx%d / %d does not give the evaluated %dx%d", width,
                        height, f, h->cols, h->rows));
    if (f == 1) return rbs_set_observation_f32(h, native, (size_t)h->npx);
    if (int32_t rc = frame_ready(h, h->stream)) return rc;
    return hand_over_native(h, native, width, f);
}

int32_t rbs_set_observation_device(rbs_handle* h, const float* d_depth, void* stream)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (int32_t rc = frame_begin(h)) return rc;
    if (!d_depth) return fail(h, RBS_ERR_INVALID_ARGUMENT, "set_observation_device: null pointer");
    if (!h->shards.empty()) return group_set_observation_device(h, d_depth, static_cast<hipStream_t>(stream));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    // the ingest kernel (copy into the handle's buffer + per-pixel model terms) is not launched
    // here: it shares a launch with the next rbs_loglikes* call's rectangles kernel when that
    // call comes on the same stream, and is launched on `s` by whatever needs the frame otherwise
    if (int32_t rc = frame_ready(h, s)) return rc;   // (an earlier frame nobody evaluated)
    return hand_over_device(h, d_depth, s);
}

int32_t rbs_get_observation(rbs_handle* h, float* out)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_GROUP_FIRST(h, rbs_get_observation(sh_, out));
    if (!out) return fail(h, RBS_ERR_INVALID_ARGUMENT, "get_observation: null pointer");
    RBS_HIP(h, hipSetDevice(h->device));
    if (int32_t rc = make_current(h, h->stream)) return rc;
    RBS_HIP(h, hipStreamSynchronize(h->stream));
    RBS_HIP(h, hipMemcpy(out, obs_frame(h), sizeof(float) * h->npx, hipMemcpyDeviceToHost));
    return RBS_OK;
}

int32_t rbs_deltas_buffer(rbs_handle* h, double** buf)
{
    if (!h || !buf) return RBS_ERR_INVALID_ARGUMENT;
    if (!h->shards.empty()) return fail(h, RBS_ERR_UNSUPPORTED, "deltas_buffer: single-device handles");
    *buf = reinterpret_cast<double*>(h->h_in);
    return RBS_OK;
}

int32_t rbs_get_poses(rbs_handle* h, double* out, int32_t n)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!h->shards.empty()) return fail(h, RBS_ERR_UNSUPPORTED, "get_poses: single-device handles");
    if (!out || n < 0 || n > h->max_particles) return fail(h, RBS_ERR_INVALID_ARGUMENT, "get_poses: bad arguments");
    RBS_HIP(h, hipSetDevice(h->device));
    RBS_HIP(h, hipStreamSynchronize(h->stream));
    RBS_HIP(h, hipMemcpy(out, h->d_in, sizeof(double) * 12 * h->n_bodies * (size_t)n, hipMemcpyDeviceToHost));
    return RBS_OK;
}

int32_t rbs_set_observation_prefetched(rbs_handle* h)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_REFUSE_POISONED(h);
    if (h->fr.next.kind != NextFrame::AHEAD)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "set_observation_prefetched: no frame was uploaded ahead (rbs_loglikes_prefetch), or another frame has been set since");
    if (int32_t rc = frame_begin(h)) return rc;
    if (int32_t rc = frame_ready(h, h->stream)) return rc;
    return hand_over_ahead(h);
}

static int32_t loglikes_impl(rbs_handle* h, const double* poses, int32_t* indices, int32_t n, int32_t update, double* out_loglik,
                             const float* next_depth, const DeltaArgs* da = nullptr)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    const BorrowedFrameGuard borrowed_guard{h};   // (a frame borrowed for this call is not the library's any longer once it returns)
    RBS_REFUSE_POISONED(h);
    if (n < 0 || n > h->max_particles)
        return fail(h, RBS_ERR_INVALID_ARGUMENT,
                    fmt("loglikes: n = %d outside 0..max_particles = %d", n, h->max_particles));
    if (n == 0) return RBS_OK;
    if (!poses || !indices || !out_loglik)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "loglikes: null pointer");
    if (!h->shards.empty()) return group_loglikes(h, poses, indices, n, update, out_loglik, da);
    const int32_t slots_total = h->peer_world > 1 ? h->peer_world * h->max_particles : h->max_particles;   // (attached: parents are global slots)
    for (int32_t i = 0; i < n; ++i)
        if (indices[i] < 0 || indices[i] >= slots_total)
            return fail(h, RBS_ERR_INVALID_ARGUMENT,
                        fmt("loglikes: indices[%d] = %d outside 0..%d", i, indices[i],
                            slots_total - 1));
    RBS_HIP(h, hipSetDevice(h->device));
    // the call waits for the log-likelihoods only -- the occlusion planes are finished by the second
    // stream and joined by the next call
    const CallState before = save_call_state(h);
    if (next_depth) {   // refused before anything is enqueued: the planes, the indices and the staging images stay as they are
        if (int32_t rc = stage_borrowed(h)) return rc;   // (a borrowed frame and a look-ahead frame: the borrowed one is staged first)
        if (int32_t rc = prefetch_check(h)) return rc;
    }
    if (int32_t rc = host_call(h, poses, indices, n, update != 0, da)) return rc;
    // the next frame travels while this call's kernels run; should the upload itself fail (a runtime error), the
    // likelihood call is still completed -- results copied, indices rewritten -- and the error reported after it
    const int32_t prefetch_rc = next_depth ? prefetch_frame(h, next_depth) : RBS_OK;
    RBS_HIP(h, hipEventSynchronize(h->ev_out));
    const bool stale_overflow = h->slab_px && h->h_err[2] != 0;   // of an earlier asynchronous call: reported below, once
    if (h->slab_px && h->h_err[0]) {
        // a region did not fit its slab: the planes this call read are intact (double buffer), so the
        // call is taken back, the slabs are enlarged to hold the largest region asked for, and the
        // call runs again -- the caller sees the numbers of whole planes, later
        if (int32_t rc = drain(h, true)) return rc;
        restore_call_state(h, before);
        if (int32_t rc = slab_housekeeping(h)) return rc;
        if (int32_t rc = host_call(h, poses, indices, n, update != 0, da)) return rc;
        RBS_HIP(h, hipEventSynchronize(h->ev_out));
        if (h->h_err[0]) return check_slab_error(h);   // (cannot happen: a region is never larger than the frame)
    }
    std::memcpy(out_loglik, h->h_out, sizeof(double) * (size_t)n);
    if (update) {
        const int32_t first = h->peer_world > 1 ? h->peer_rank * h->max_particles : 0;
        for (int32_t i = 0; i < n; ++i) indices[i] = first + i;
    }
    if (int32_t rc = slab_housekeeping(h)) return rc;
    h->quiet = !h->async_outstanding;   // (everything on the handle's stream has run; the copy kernel's last blocks are short)
    if (stale_overflow) {   // this call's results are good; an earlier rbs_loglikes_device's were not
        h->h_err[0] = 1;
        const int32_t rc = check_slab_error(h);
        h->h_err[0] = 0;
        return rc;
    }
    return prefetch_rc;   // (its message is rbs_last_error's: nothing above overwrote it on the way here)
}

int32_t rbs_loglikes_device(rbs_handle* h, const double* d_poses, const int32_t* d_indices,
                            int32_t n, int32_t update, double* d_out_loglik, void* stream)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_REFUSE_POISONED(h);
    if (n < 0 || n > h->max_particles)
        return fail(h, RBS_ERR_INVALID_ARGUMENT,
                    fmt("loglikes_device: n = %d outside 0..max_particles = %d", n, h->max_particles));
    if (n == 0) return RBS_OK;
    if (!d_poses || !d_indices || !d_out_loglik)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "loglikes_device: null pointer");
    if (!h->shards.empty()) return group_loglikes_device(h, d_poses, d_indices, n, update, d_out_loglik, static_cast<hipStream_t>(stream));
    RBS_HIP(h, hipSetDevice(h->device));
    hipStream_t s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    if (int32_t rc = stage_borrowed(h)) return rc;   // (only the host-pointer calls stage a borrowed frame behind their own kernels)
    if (h->slab_auto && !h->slab_probed && update && h->peer_world <= 1) {
        // slabs the LIBRARY chose (state_slab_px = 0, more than 8 192 particles): an asynchronous call cannot be taken
        // back, so the first one is preceded by a look at the regions it will store -- one small kernel and ONE host
        // synchronisation in the handle's lifetime -- and the slabs are enlarged first if they would be three
        // quarters full (a default-config handle must not answer its first call with NaNs)
        h->slab_probed = true;
        DevParams P = h->base;
        P.poses = d_poses; P.indices = d_indices; P.n = n;
        P.slots = h->max_particles; P.n_dev = 1; P.shard_cap = h->max_particles;
        P.win_src = h->d_win[h->cur];
        P.rect_align = h->windowed ? rbs::kRectAlignWindowed : rbs::kRectAlign;
        if (int32_t rc = drain(h, false)) return rc;
        int* d_max = h->d_err + 1;   // (the sticky maximum the rectangles kernel keeps: the probe only raises it early)
        hipLaunchKernelGGL(rbs::rbs_region_probe_kernel, dim3((unsigned)((n + rbs::kPrepPerBlock - 1) / rbs::kPrepPerBlock)),
                           dim3(64 * rbs::kPrepPerBlock), 0, s, P, d_max);
        RBS_HIP(h, hipGetLastError());
        RBS_HIP(h, hipMemcpyAsync(h->h_err, h->d_err, 2 * sizeof(int), hipMemcpyDeviceToHost, s));
        RBS_HIP(h, hipStreamSynchronize(s));
        if (int32_t rc = slab_housekeeping(h)) return rc;
    }
    h->async_outstanding = true;
    return enqueue_loglikes(h, d_poses, d_indices, n, update != 0, d_out_loglik, s);
}

int32_t rbs_loglikes(rbs_handle* h, const double* poses, int32_t* indices, int32_t n,
                     int32_t update, double* out_loglik)
{
    return loglikes_impl(h, poses, indices, n, update, out_loglik, nullptr);
}

int32_t rbs_loglikes_deltas(rbs_handle* h, const double* deltas, const double* default_poses, int32_t body_stride,
                            int32_t* indices, int32_t n, int32_t update, double* out_loglik)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (body_stride < 6) return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("loglikes_deltas: body_stride = %d, need >= 6 (position, rotation vector)", body_stride));
    if (n > 0 && (!deltas || !default_poses)) return fail(h, RBS_ERR_INVALID_ARGUMENT, "loglikes_deltas: null pointer");
    const DeltaArgs da = {deltas, default_poses, body_stride};
    return loglikes_impl(h, deltas, indices, n, update, out_loglik, nullptr, &da);
}

int32_t rbs_loglikes_prefetch(rbs_handle* h, const double* poses, int32_t* indices, int32_t n, int32_t update, double* out_loglik,
                              const float* next_depth, size_t next_n)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!h->shards.empty()) return fail(h, RBS_ERR_UNSUPPORTED, "loglikes_prefetch: single-device handles (a handle over several devices: rbs_acquire/commit_frame_buffer)");
    if (!next_depth || next_n != (size_t)h->npx)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("loglikes_prefetch: expected a next frame of %d pixels, got %zu", h->npx, next_n));
    if (n <= 0) return fail(h, RBS_ERR_INVALID_ARGUMENT, "loglikes_prefetch: n must be positive");
    return loglikes_impl(h, poses, indices, n, update, out_loglik, next_depth);
}

int32_t rbs_synchronize(rbs_handle* h)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!h->shards.empty()) {
        int32_t first = RBS_OK;
        for (rbs_handle* sh_ : h->shards) {
            RBS_HIP(h, hipSetDevice(sh_->device));
            if (int32_t rc = drain(sh_, true)) return gfail(h, sh_, rc);
            if (sh_->slab_px) RBS_HIP(h, hipMemcpy(sh_->h_err, sh_->d_err, 2 * sizeof(int), hipMemcpyDeviceToHost));
            if (first == RBS_OK && check_slab_error(sh_) != RBS_OK) first = gfail(h, sh_, RBS_ERR_OUT_OF_MEMORY);
        }
        if (int32_t rc = group_grow_slabs(h, nullptr)) return rc;
        return first;
    }
    RBS_HIP(h, hipSetDevice(h->device));
    if (int32_t rc = stage_borrowed(h)) return rc;   // (the caller's frame is released when this returns)
    if (int32_t rc = drain(h, true)) return rc;
    if (h->slab_px) RBS_HIP(h, hipMemcpy(h->h_err, h->d_err, 2 * sizeof(int), hipMemcpyDeviceToHost));
    // an asynchronous call whose region did not fit is reported here, ONCE; the slabs are enlarged
    // either way so that the calls that follow fit
    const int32_t rc = check_slab_error(h);
    const std::string msg = h->err;
    if (int32_t rc2 = slab_housekeeping(h)) return rc2;
    if (rc) h->err = msg;
    h->async_outstanding = false;
    h->quiet = true;
    return rc;
}

// the occlusion planes' slot entry points: rbs_get_occlusion .. rbs_import_window, rbs_stream_join, rbs_get_window
#include "rbs_planes_api.h"

// one process per GPU: rbs_ipc_export, rbs_ipc_attach, rbs_stage_windows, rbs_peer_resample
#include "rbs_ipc.h"

int32_t rbs_render_depth(rbs_handle* h, const double* pose, float* out)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_GROUP_FIRST(h, rbs_render_depth(sh_, pose, out));
    if (!pose || !out) return fail(h, RBS_ERR_INVALID_ARGUMENT, "render_depth: null pointer");
    RBS_HIP(h, hipSetDevice(h->device));
    RBS_HIP(h, hipMemcpyAsync(h->d_poses, pose, sizeof(double) * 12 * h->n_bodies,
                              hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(rbs::rbs_fill_kernel, dim3(256), dim3(256), 0, h->stream, h->d_render,
                       (size_t)h->npx, INFINITY);
    DevParams P = h->base;
    P.poses = h->d_poses;
    P.n = 1;
    P.tile_w = 256;
    P.tile_px = rbs::kTilePxBig;
    P.tile_h = P.tile_px / 256;
    // (one block, the raster kernel's big tile: not launch_pose_planes' geometry)
    hipLaunchKernelGGL(rbs::rbs_planes_render_kernel<false>, dim3(1), dim3(rbs::kBlock), rbs::smem_bytes(P.tile_px, false),
                       h->stream, P, h->d_render, (int4*)nullptr, (const int*)nullptr);
    RBS_HIP(h, hipGetLastError());
    RBS_HIP(h, hipMemcpyAsync(out, h->d_render, sizeof(float) * h->npx, hipMemcpyDeviceToHost,
                              h->stream));
    RBS_HIP(h, hipStreamSynchronize(h->stream));
    return RBS_OK;
}

#ifdef RBS_PHASE_TIMING
int32_t rbs_debug_phase_cycles(rbs_handle* h, unsigned long long* out8)
{
    if (!h || !h->d_phase) return RBS_ERR_INVALID_ARGUMENT;
    RBS_HIP(h, hipDeviceSynchronize());
    RBS_HIP(h, hipMemcpy(out8, h->d_phase, 256, hipMemcpyDeviceToHost));   // 16 cycle counters + 16 event counters
    RBS_HIP(h, hipMemset(h->d_phase, 0, 256));
    return RBS_OK;
}
#endif

int32_t rbs_last_kernel_ms(rbs_handle* h, float* ms)
{
    float copy_ms = 0.f;
    int32_t used = 0;
    return rbs_timing_summary(h, 1, ms, &copy_ms, &used);
}

int32_t rbs_timing_summary(rbs_handle* h, int32_t last_n, float* call_ms, float* copy_kernel_ms,
                           int32_t* n_used)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_GROUP_FIRST(h, rbs_timing_summary(sh_, last_n, call_ms, copy_kernel_ms, n_used));
    if (!call_ms || !copy_kernel_ms || !n_used || last_n <= 0)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "timing_summary: bad argument");
    if (h->calls == 0) return fail(h, RBS_ERR_INVALID_ARGUMENT, "timing_summary: no loglikes launched yet");
    RBS_HIP(h, hipSetDevice(h->device));
    // the timed calls among the last last_n calls (at least the most recent timed one)
    const long n = std::max<long>(1, std::min<long>({((long)last_n + h->timing_every - 1) / h->timing_every,
                                                      h->timed_calls, (long)rbs_handle::kRing}));
    double tot = 0.0, cpy = 0.0;
    int n_copy = 0;
    for (long k = 0; k < n; ++k) {
        const int slot = (int)((h->timed_calls - 1 - k) % rbs_handle::kRing);
        float ms = 0.f;
        RBS_HIP(h, hipEventSynchronize(h->ev_stop[slot]));
        RBS_HIP(h, hipEventElapsedTime(&ms, h->ev_start[slot], h->ev_stop[slot]));
        tot += ms;
        if (h->ring_update[slot]) {
            RBS_HIP(h, hipEventSynchronize(h->ev_copy_stop[slot]));
            RBS_HIP(h, hipEventElapsedTime(&ms, h->ev_copy_start[slot], h->ev_copy_stop[slot]));
            cpy += ms;
            ++n_copy;
        }
    }
    *call_ms = (float)(tot / (double)n);
    *copy_kernel_ms = n_copy ? (float)(cpy / n_copy) : 0.f;
    *n_used = (int32_t)n;
    return RBS_OK;
}

int32_t rbs_set_timing_every(rbs_handle* h, int32_t every)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_GROUP_ALL(h, rbs_set_timing_every(sh_, every));
    if (every < 1) return fail(h, RBS_ERR_INVALID_ARGUMENT, "set_timing_every: every must be >= 1");
    h->timing_every = every;
    return RBS_OK;
}

int32_t rbs_raster_kernel_ms(rbs_handle* h, int32_t last_n, float* raster_kernel_ms)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_GROUP_FIRST(h, rbs_raster_kernel_ms(sh_, last_n, raster_kernel_ms));
    if (!raster_kernel_ms || last_n <= 0) return fail(h, RBS_ERR_INVALID_ARGUMENT, "raster_kernel_ms: bad argument");
    if (h->calls == 0) return fail(h, RBS_ERR_INVALID_ARGUMENT, "raster_kernel_ms: no loglikes launched yet");
    RBS_HIP(h, hipSetDevice(h->device));
    const long n = std::max<long>(1, std::min<long>({((long)last_n + h->timing_every - 1) / h->timing_every,
                                                      h->timed_calls, (long)rbs_handle::kRing}));
    double tot = 0.0;
    for (long k = 0; k < n; ++k) {
        const int slot = (int)((h->timed_calls - 1 - k) % rbs_handle::kRing);
        float ms = 0.f;
        RBS_HIP(h, hipEventSynchronize(h->ev_raster_stop[slot]));
        RBS_HIP(h, hipEventElapsedTime(&ms, h->ev_raster_start[slot], h->ev_raster_stop[slot]));
        tot += ms;
    }
    *raster_kernel_ms = (float)(tot / (double)n);
    return RBS_OK;
}

int32_t rbs_set_option(rbs_handle* h, int32_t option, double value)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(value)) return fail(h, RBS_ERR_INVALID_ARGUMENT, "set_option: the value is not finite");
    std::vector<rbs_handle*> all(h->shards.begin(), h->shards.end());
    all.push_back(h);      // (a group keeps the shared trail's policy itself; its shards the rest)
    for (rbs_handle* x : all) {
        switch (option) {
            case RBS_OPT_SHARED_TRAIL: x->stp_allowed = value != 0.0; break;
            case RBS_OPT_SHARED_TRAIL_ENTER:
                if (!(value > 0.0 && value <= 1.0)) return fail(h, RBS_ERR_INVALID_ARGUMENT, "set_option: RBS_OPT_SHARED_TRAIL_ENTER must be in (0, 1]");
                x->stp_enter = value; break;
            case RBS_OPT_SHARED_TRAIL_EVERY:
                if (!(value >= 1.0)) return fail(h, RBS_ERR_INVALID_ARGUMENT, "set_option: RBS_OPT_SHARED_TRAIL_EVERY must be >= 1");
                x->stp_every = (int)value; break;
            case RBS_OPT_TRACKER_SPLIT_MAX:
                if (!(value >= 0.0)) return fail(h, RBS_ERR_INVALID_ARGUMENT, "set_option: RBS_OPT_TRACKER_SPLIT_MAX must be >= 0");
                x->tracker_split_max = (int)std::min(value, 2e9); break;
            case RBS_OPT_TIMING_EVERY:
                if (!(value >= 1.0)) return fail(h, RBS_ERR_INVALID_ARGUMENT, "set_option: RBS_OPT_TIMING_EVERY must be >= 1");
                x->timing_every = (int)std::min(value, 1e9); break;
            default: return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("set_option: unknown option %d", option));
        }
    }
    return RBS_OK;
}

int32_t rbs_window_fraction(rbs_handle* h, double* out)
{
    if (!h || !out) return RBS_ERR_INVALID_ARGUMENT;
    double f = h->area_frac;
    for (rbs_handle* sh : h->shards) f = std::max(f, sh->area_frac);
    *out = f;
    return RBS_OK;
}

int32_t rbs_shared_trail_rebase(rbs_handle* h, int32_t global_slot)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!h->shards.empty()) return fail(h, RBS_ERR_UNSUPPORTED, "shared_trail_rebase: a handle over several devices decides for its shards itself");
    if (!h->windowed) return fail(h, RBS_ERR_UNSUPPORTED, "shared_trail_rebase: windowed planes only");
    const int slots = std::max(1, h->peer_world) * h->max_particles;
    if (global_slot != -2 && (global_slot < 0 || global_slot >= slots))
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("shared_trail_rebase: slot %d outside 0..%d (or -2: leave)", global_slot, slots - 1));
    h->stp_request = global_slot;
    return RBS_OK;
}

int32_t rbs_shared_trail_state(rbs_handle* h, int32_t* active, int32_t* rebases)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    // (a handle over several devices: the group's own state -- one decision for all shards)
    if (active) *active = h->stp ? 1 : 0;
    if (rebases) *rebases = (int32_t)h->stp_rebases;
    return RBS_OK;
}

int32_t rbs_get_background(rbs_handle* h, float* out)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_GROUP_FIRST(h, rbs_get_background(sh_, out));
    if (!out) return fail(h, RBS_ERR_INVALID_ARGUMENT, "get_background: null pointer");
    *out = h->background;
    return RBS_OK;
}

}  // extern "C"

// The device tracker's host side (rbs_tracker_*).
#include "rbs_tracker_api.h"

// The robust Gaussian tracker (rbs_gauss_*): its kernels and host side.
#include "rbsensor_gauss.hip"
#include "rbsensor_find.hip"

#ifdef RBS_TEST_HOOKS   // (librbsensor_mi355x_hooks.so only) rbs_test_*: the per-pixel likelihood's inline functions, value by value (tests/test_gpu_pixel_math.py)
#include "rbsensor_probes.hip"
#endif
