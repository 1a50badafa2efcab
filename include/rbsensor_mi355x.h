/*
 * rbsensor_mi355x.h -- C-ABI of librbsensor_mi355x.so, the MI355X (gfx950) implementation of
 * dbot's Rao-Blackwellised depth-image observation model (RbSensor), i.e. the likelihood
 * evaluator that dbot_ros's particle tracker drives once per sampling block per frame.
 *
 * Drop-in boundary: each entry point replaces one virtual of the sensor object that
 * dbot::RbSensorBuilder<State>::build() returns.  The reference only names that object
 * through its builder, so the citations are the reference's own construction / call sites
 * (R: = bayesian-object-tracking/dbot_ros):
 *
 *   rbs_create            <- RbSensorBuilder<State>(object_model, camera_data, params)
 *                            R:source/dbot_ros/tracker/particle_tracker_node.cpp:164-203
 *                            R:source/dbot_ros/tracker/object_tracker_service_node.cpp:136-175
 *   rbs_reset             <- RbSensor::reset(), via tracker->initialize(...)
 *                            R:source/dbot_ros/tracker/particle_tracker_node.cpp:252
 *   rbs_set_observation   <- RbSensor::set_observation(image), via tracker_->track(image)
 *                            R:source/dbot_ros/object_tracker_ros.hpp:44-49
 *                            (layout R:source/dbot_ros/util/ros_interface.h:152-168)
 *   rbs_loglikes          <- RbSensor::loglikes(deltas, indices, update), once per sampling
 *                            block inside tracker_->track R:source/dbot_ros/object_tracker_ros.hpp:49
 *   rbs_destroy           <- ~RbSensor (tracker torn down per service session,
 *                            R:source/dbot_ros/tracker/object_tracker_service_node.cpp:233-238)
 *
 * Conventions: 0 = success, negative = error (message via rbs_last_error); the caller owns
 * every pointer it passes, the library copies what it keeps; a handle is driven by one
 * thread at a time but may be created/destroyed repeatedly from any thread; no exception
 * crosses this boundary.  There is NO CPU fallback: without a usable gfx950 device
 * rbs_create fails with RBS_ERR_NO_DEVICE.
 */
#ifndef RBSENSOR_MI355X_H
#define RBSENSOR_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RBS_ABI_VERSION 2

enum {
    RBS_OK = 0,
    RBS_ERR_INVALID_ARGUMENT = -1,
    RBS_ERR_NO_DEVICE = -2,
    RBS_ERR_OUT_OF_MEMORY = -3,
    RBS_ERR_HIP = -4,
    RBS_ERR_UNSUPPORTED = -5
};

/* rbs_config.likelihood_precision: the arithmetic of the per-pixel Kinect likelihood (exp / erf /
 * log and the mixture algebra).  Coverage and depth do not depend on it (binary64 geometry, float
 * depth), nor does the occlusion process' time step; the per-particle sum is binary64 in both.
 *   F64  (the library default) binary64 with the reference CPU path's float rounding points
 *        (SURVEY A.4): agrees with the device-rule (EAGER) oracle to ~1e-15 -- its resampling
 *        (parent) indices are reproduced one for one at 20 000 particles -- and with the
 *        reference-semantics (LAZY: per-pixel time stamps, double propagation) oracle to ~1e-8 at
 *        640x480 and <= 5e-7 at 80x60, relative to max(1, |ll|): inside BASELINE.json north_star's
 *        1e-5 for EVERY particle of C1 on every frame of a 30-frame resampled sequence.  Parent
 *        indices against the LAZY oracle, same uniforms and history (measured,
 *        tests/test_gpu_reference_semantics.py): 0 of 60 000 children over 30 resamplings at 2 000
 *        particles / 640x480; 16 of 600 000 children over 30 resamplings at 20 000 particles /
 *        80x60 (0-5 per resampling), every one of them a uniform within 1e-7 of a step of the
 *        cumulative weights that drew the neighbouring parent.  Stored planes differ from the LAZY
 *        model's "as of now" values by <= 1.2e-6 after 30 frames (the 2^-18 snap bounds it).
 *   F32  OPT-IN.  float32 likelihood on the exp2 / log2 / rcp units, per-pixel terms derived from
 *        the observation on the fly.  It does NOT meet north_star's bar for every particle and does
 *        NOT reproduce parent indices at large particle counts: against the reference-semantics
 *        oracle it is within 1e-5 relative only for particles whose sum is well conditioned
 *        (|ll| >= 0.1 of the sum of the magnitudes of the per-pixel terms); for all particles the
 *        bound is 1e-6 of that sum of magnitudes, i.e. float32-level agreement, ~5e-4 absolute on
 *        log-likelihoods of magnitude 1e4.  The occlusion POSTERIOR (carried state) is computed in
 *        float32 as well: stored planes differ from the oracle's by up to 2e-6.
 * DEFAULT = RBS_PRECISION_LIBRARY_DEFAULT.  (Tooling only: RBS_PRECISION=f64|f32 in the environment
 * replaces DEFAULT; it never overrides a precision the caller named.) */
enum { RBS_PRECISION_DEFAULT = 0, RBS_PRECISION_F64 = 1, RBS_PRECISION_F32 = 2 };
#define RBS_PRECISION_LIBRARY_DEFAULT RBS_PRECISION_F64
/* rbs_config.state_layout: how occlusion planes are stored ("occlusion state layout" below).
 * DEFAULT = windowed (RBS_STATE=dense in the environment overrides DEFAULT only: tooling). */
enum { RBS_STATE_DEFAULT = 0, RBS_STATE_WINDOWED = 1, RBS_STATE_DENSE = 2 };
/* rbs_config.state_slab_px: see the field. */
#define RBS_SLAB_WHOLE_PLANES (-1)
/* rbs_config.occlusion_mode: how the occlusion process (OcclusionModel propagate, constants at
 * R:source/dbot_ros/tracker/particle_tracker_node.cpp:176-189) is carried between frames.
 *   REFERENCE   the reference CPU model's own bookkeeping: a pixel keeps the float posterior it was last UPDATED to and the
 *               time of that update, and its prior at a later call is propagate(value, elapsed time) evaluated in binary64
 *               and rounded once -- the oracle's mode LAZY, whose operations the device performs in the oracle's order, so
 *               priors are bit-identical and log-likelihoods agree to the last digits of the transcendentals (~1e-13
 *               relative; tests/test_gpu_exact_occlusion.py).  Storage: per pixel of a window the float and a 16-bit AGE
 *               (frames since the update, counted against the slot's epoch = the last updating call): 6 bytes instead of
 *               4; nothing is stepped between frames -- the copy kernel copies, ages advance by packed saturating adds.
 *               A pixel whose age exceeds the frame count at which (p_oo - p_ov)^(age * delta_time) <= 2^-40 (1 628
 *               frames with the defaults) is the background again: its value differs from a never-covered pixel's by
 *               less than that.  That count must fit the age: parameters with which a value has not decayed so far
 *               within 65 534 frames (p_oo - p_ov above ~0.987 at 30 frames/s) are RBS_ERR_UNSUPPORTED in this mode.
 *               Binary64 likelihood and the windowed layout only (RBS_ERR_UNSUPPORTED otherwise); every layout option
 *               of the windowed form works (slabs, several devices, attached ranks, the shared trail).
 *   DEVICE_RULE the float-stepped rule (oracle mode EAGER): every stored value advanced by one float FMA per updating
 *               call and snapped onto the background within 2^-18 of it.  Within ~1e-8 of REFERENCE (relative, typical);
 *               of 30 720 particle-frames one was 1.3e-5 away, and 16 of 600 000 resampled children drew a neighbouring
 *               parent at 20 000 particles (both gone with REFERENCE).  All precisions and layouts.
 * The hooks below that hand out or take whole planes (rbs_get/set_occlusion, rbs_export/import_plane/_window) deal in
 * EFFECTIVE values as of the last updating call in both modes; in REFERENCE mode a plane handed in is taken "as of now"
 * (ages 0), the rule of the oracle's set_occlusion.  rbs_occlusion_*device_ptr are RBS_ERR_UNSUPPORTED in REFERENCE mode
 * (a slot is not a float plane).  DEFAULT = RBS_OCC_LIBRARY_DEFAULT. */
enum { RBS_OCC_DEFAULT = 0, RBS_OCC_DEVICE_RULE = 1, RBS_OCC_REFERENCE = 2 };
#define RBS_OCC_LIBRARY_DEFAULT RBS_OCC_DEVICE_RULE

typedef struct rbs_handle rbs_handle;

/* kinect.tail_weight = 0 is accepted, as the reference accepts it (it passes the ROS parameter through
 * unchecked, R:source/dbot_ros/tracker/particle_tracker_node.cpp:183-184), but evaluated as this floor: the
 * library's binary64 erfc / exp are accurate to 1e-16 ABSOLUTE, which is exact next to tw / max_depth for any
 * tw >= 1e-9 and would not be in a mixture without a tail.  Observable difference: pixels the exact tw = 0
 * model prices at log(0) = -inf contribute log(1.7e-10 / p_bg) ~ -22 each instead. */
#define RBS_TAIL_WEIGHT_FLOOR 1e-9

typedef struct rbs_config {
    int32_t abi_version;            /* RBS_ABI_VERSION                                        */
    int32_t device_id;              /* HIP device ordinal                                      */
    int32_t rows, cols;             /* evaluated resolution (after down-sampling)             */
    double K[9];                    /* row-major 3x3 intrinsics, top two rows already divided
                                       by the down-sampling factor
                                       (R:source/dbot_ros/util/ros_camera_data_provider.cpp:72);
                                       zero skew, K[8] == 1                                    */
    int32_t max_particles;          /* occlusion slots to allocate (>= any n passed later)    */
    int32_t n_objects;              /* rigid bodies = meshes (object/meshes)                   */
    const double* vertices;         /* concatenated xyz per object, sum(vertex_counts)*3      */
    const int32_t* vertex_counts;   /* [n_objects]                                             */
    const int32_t* triangles;       /* concatenated vertex-index triples, local to each object*/
    const int32_t* triangle_counts; /* [n_objects]                                             */
    /* RbSensorBuilder<State>::Parameters, R:...particle_tracker_node.cpp:176-189 */
    double p_occluded_visible;
    double p_occluded_occluded;
    double initial_occlusion_prob;
    double tail_weight;             /* 0 <= tw < 1; below RBS_TAIL_WEIGHT_FLOOR it is evaluated AS the floor (see above) */
    double model_sigma;
    double sigma_factor;
    double delta_time;
    /* --- ABI version 2 --- */
    int32_t likelihood_precision;   /* RBS_PRECISION_*                                         */
    int32_t state_layout;           /* RBS_STATE_*                                             */
    /* Particle sharding over several devices of one node inside ONE handle (the reference's
     * tracker node is one process, R:source/dbot_ros/tracker/particle_tracker_node.cpp:277-284):
     * n_devices <= 1 -> device_id alone.  n_devices > 1 -> device_ids[n_devices] HIP ordinals;
     * max_particles is the TOTAL over all devices.  See "several devices" below. */
    int32_t n_devices;
    const int32_t* device_ids;
    /* Window-sized slabs for the occlusion state (windowed layout only).  A slot then holds
     * state_slab_px floats instead of a whole plane (rows*cols floats: 2 x 1.2 MB per particle at
     * 640x480, of which a tracked object's window touches ~3 %) and stores only the region an updating
     * call writes, bbox(parent's window, the particle's screen rectangle).  The numbers are those of
     * whole planes.
     *   0   the library's choice: whole planes up to 8 192 particles (per device), slabs of
     *       rows*cols/8 floats above (8x the particles in the same memory);
     *   >0  slabs of that many floats;   RBS_SLAB_WHOLE_PLANES (-1)  whole planes whatever the count.
     * Slabs GROW: at every synchronising call the library enlarges them once the largest region any
     * particle has asked for fills three quarters of a slab, and a synchronous rbs_loglikes whose
     * region does not fit all the same is taken back, the slabs enlarged, and run again -- the caller
     * sees the numbers of whole planes (state memory grows towards that of whole planes in the
     * worst case; enlarging needs the new buffers beside the old ones for a moment and fails with
     * RBS_ERR_OUT_OF_MEMORY if they do not fit).  Only a call that has already RETURNED cannot be
     * repaired -- rbs_loglikes_device, a frame of rbs_tracker_*: a region that outgrows its slab by
     * more than a quarter within one such call is contained (log-likelihood NaN, plane reset to the
     * background) and reported once, by the next synchronising call / that frame's result; the slabs
     * have been enlarged when that call returns.  rbs_tracker_initialize sizes the slabs for the object
     * at its default pose with a probe call, so a tracker does not start on slabs that are too small;
     * slabs the LIBRARY chose (0) are checked the same way in front of a handle's first updating
     * rbs_loglikes_device (one small kernel, one host synchronisation, once).  Planes handed in from
     * outside (rbs_set_occlusion, rbs_import_plane / _window) enlarge the slabs when they do not fit.
     * With slabs -- chosen by the caller or by the library -- two hooks are RBS_ERR_UNSUPPORTED, because a slot
     * is not a plane any more: rbs_occlusion_device_ptr and rbs_occlusion_next_device_ptr (use
     * rbs_export_plane / rbs_export_window); RBS_SLAB_WHOLE_PLANES keeps them.  The shards of a handle over
     * several devices and ranks attached with rbs_ipc_attach keep ONE slab size among them: a group grows all its
     * shards together (synchronous calls), attached ranks do not grow. */
    int32_t state_slab_px;
    int32_t occlusion_mode;         /* RBS_OCC_* (this field was reserved0 = 0 = DEFAULT before round 6: same layout, same ABI version) */
} rbs_config;

int32_t rbs_abi_version(void);
int32_t rbs_device_count(void);

int32_t rbs_create(const rbs_config* cfg, rbs_handle** out);
void rbs_destroy(rbs_handle* h);
/* Message of the last error on this handle; h == NULL gives the calling thread's last
 * rbs_create failure. Never NULL. */
const char* rbs_last_error(const rbs_handle* h);

int32_t rbs_reset(rbs_handle* h);

/* depth[n], n == rows*cols, row-major (row*cols+col), metres, NaN/inf = no reading. */
int32_t rbs_set_observation(rbs_handle* h, const double* depth, size_t n);
/* Same, from the float32 pixels the camera driver delivers (skips the double round trip). */
int32_t rbs_set_observation_f32(rbs_handle* h, const float* depth, size_t n);
/* rbs_set_observation WITHOUT the copy at call time (round 5): the library BORROWS `depth` -- it must stay valid and
 * unchanged until the next rbs_loglikes / rbs_loglikes_deltas / rbs_loglikes_prefetch or rbs_synchronize on the handle has
 * RETURNED (any other entry point that needs the observation stages it first as well; a later rbs_set_observation* or
 * rbs_reset simply drops it).  That next likelihood call launches its rectangles kernel and its GEOMETRY kernel -- which
 * need no frame -- first, converts (double -> float) and sends the frame while they run, and only then launches the
 * likelihood kernel: the two-kernel form of the raster launch (same work items, same summation order, same bits as the
 * one-kernel launch), so the frame's journey, 60-100 us of a synchronous 300 us step, hides behind the geometry.
 * This is what the dbot binding calls: inside tracker_->track(image) (R:source/dbot_ros/object_tracker_ros.hpp:49) the
 * image outlives the filter's set_observation / loglikes pair.  The occlusion clock advances at this call, as for
 * rbs_set_observation.  Handles over several devices, precision F32 and whole-plane handles copy at once (= rbs_set_observation).
 * "Returned" includes returned with an error: a likelihood call that is refused (bad indices, ...) or fails before it staged
 * the frame copies it on its way out -- the frame is the observation from then on, the buffer the caller's again.
 * MEMORY: the two-kernel launch hands its depth tiles from the first kernel to the second through device memory, one tile (44 KB)
 * per work item, allocated at the first such call for the worst case the call's particle count allows (every rectangle the whole
 * frame: 36 tiles per particle at 640x480 -- 2.7 GB at 2 000 particles; rbs_tracker_*_f64 below 5 000 evaluations likewise).  The
 * library takes it only if it is at most 8 GB AND at most half of the device's free memory; otherwise, or if the allocation fails,
 * the call is launched as one kernel with the frame staged first (= rbs_set_observation), same results. */
int32_t rbs_set_observation_borrowed(rbs_handle* h, const double* depth, size_t n);
int32_t rbs_set_observation_borrowed_f32(rbs_handle* h, const float* depth, size_t n);   /* the same for the driver's float pixels */

/* Frame ingest straight from the camera driver: `native` is the full-resolution
 * float32 image (width x height, metres, NaN = no reading); the evaluated image is its
 * sub-sampling by the reference's rule, eval(row, col) = native(row*f, col*f) with
 * rows = height/f, cols = width/f (ri::to_eigen_vector, R:source/dbot_ros/util/ros_interface.h:152-168),
 * applied while the frame is staged into pinned memory: ONE host pass over the rows*cols values the
 * sensor evaluates (19 KB of a 1.2 MB frame at the reference's default factor 8) and a transfer of
 * that size -- in place of the reference's three host copies of the whole frame
 * (R:source/dbot_ros/object_tracker_ros.hpp:82,119, ros_interface.h:156-165). */
int32_t rbs_set_observation_native_f32(rbs_handle* h, const float* native, int32_t width,
                                       int32_t height, int32_t downsampling_factor);
/* The same from DEVICE memory on the handle's device (float[rows*cols], evaluated resolution):
 * for frames that are already on the GPU (a driver / preprocessing stage there, or a caller
 * replaying a resident sequence).  Ordered on `stream` (NULL = the handle's own stream), no
 * host synchronisation.  The ingest kernel is launched by the next rbs_* call that needs the
 * frame (it shares a launch with the next rbs_loglikes_device on the same stream): the caller
 * keeps `d_depth` alive and unchanged until that call's work has run. */
int32_t rbs_set_observation_device(rbs_handle* h, const float* d_depth, void* stream);
/* Zero-copy hand-over of a host frame: rbs_acquire_frame_buffer gives the handle's pinned staging
 * buffer for the NEXT frame (float[rows*cols], evaluated resolution, valid until the matching
 * commit); the caller writes the frame straight into it -- the conversion loop of
 * ri::to_eigen_vector (R:source/dbot_ros/util/ros_interface.h:152-168) can target it -- and
 * rbs_commit_frame_buffer is then rbs_set_observation_f32 without the 1.2 MB host copy.  Two
 * buffers alternate: acquiring waits for the upload that used the buffer two frames ago. */
int32_t rbs_acquire_frame_buffer(rbs_handle* h, float** buf);
int32_t rbs_commit_frame_buffer(rbs_handle* h);
/* Current evaluated observation -> host float[rows*cols] (inspection). */
int32_t rbs_get_observation(rbs_handle* h, float* out);

/* poses:   [n][n_objects][12] doubles, R (row-major 3x3) then t: absolute camera-frame pose
 *          of each body (delta composed with the default pose by the caller).
 * indices: [n] in: occlusion slot each particle inherits from; out (update != 0): identity.
 * update:  non-zero -> write the posterior occlusion of particle i into slot i.
 * out_loglik: [n] doubles.  Host pointers; synchronous: the call returns when the log-likelihoods
 * are in out_loglik (the caller's buffers are staged through pinned memory that the kernels read
 * and write in place -- no copy-engine transfer besides the frame's); the occlusion planes of an
 * updating call are finished in the background and joined by the next call on the handle. */
int32_t rbs_loglikes(rbs_handle* h, const double* poses, int32_t* indices, int32_t n,
                     int32_t update, double* out_loglik);

/* rbs_loglikes with the NEXT frame travelling behind it (a recorded dataset, or a driver that is a frame ahead:
 * the reference's tracker takes its frames from a mailbox, R:source/dbot_ros/object_tracker_ros.hpp:69-84, :44-49).
 * Same call, same results; between launching its kernels and waiting for them the library stages next_depth
 * (float32 metres, rows*cols, the layout of rbs_set_observation_f32) into its other pinned image and sends it on
 * the upload stream, the per-pixel model terms behind it -- the 1.2 MB copy and transfer of a 640x480 frame pass
 * while the raster kernel runs.  The current observation is unchanged.  rbs_set_observation_prefetched then makes
 * that frame the observation at no cost (one frame per call, as rbs_set_observation_f32 does: the model clock
 * advances by delta_time); any other rbs_set_observation* in between abandons it.  One frame may be waiting at a time: a second
 * rbs_loglikes_prefetch with a next frame before the first has been installed (or abandoned) is RBS_ERR_INVALID_ARGUMENT -- a caller
 * with several sampling blocks per frame hands the next frame to ONE of them and calls rbs_loglikes for the others.
 * Single-device handles. */
int32_t rbs_loglikes_prefetch(rbs_handle* h, const double* poses, int32_t* indices, int32_t n, int32_t update,
                              double* out_loglik, const float* next_depth, size_t next_n);
int32_t rbs_set_observation_prefetched(rbs_handle* h);

/* Device-pointer variant: poses/indices/out_loglik are device memory on the handle's device,
 * work is enqueued on `stream` (a hipStream_t, NULL = the handle's own stream) and the call
 * returns without synchronising.  indices is read-only and read in `stream` order only (the
 * first kernel snapshots it for the library's second stream): the caller may overwrite it by work
 * enqueued on `stream` right after the call.  With update != 0 the caller must treat the slot
 * map as identity afterwards.  d_out_loglik is complete in `stream` order.  The
 * occlusion planes an updating call writes are finished by a second, internal stream: every
 * later rbs_* call on the handle orders itself after them (so back-to-back calls pipeline), and
 * rbs_synchronize / rbs_occlusion_*_device_ptr / any host-pointer entry point waits for them. */
int32_t rbs_loglikes_device(rbs_handle* h, const double* d_poses, const int32_t* d_indices,
                            int32_t n, int32_t update, double* d_out_loglik, void* stream);

/* RbSensor::loglikes(deltas, indices, update) WITH THE ARGUMENTS THE FILTER PASSES (round 5): the particles' state
 * DELTAS around the sensor's default ("integrated") poses, not absolute poses -- what dbot's filter hands the
 * sensor inside tracker_->track(image) (R:source/dbot_ros/object_tracker_ros.hpp:49; the State of
 * R:source/dbot_ros/object_tracker_ros.h:40-41, read per body through component(i) as at .hpp:54-60).  The
 * composition of SURVEY A.1,
 *     R = R(delta rotation vector) R(default rotation vector),   t = t(delta) + t(default),
 * rotation vector -> matrix through the unit quaternion, runs on the device inside the rectangles kernel (the wave that owns a
 * particle composes its poses first; the operations and their order are oracle/tracker_oracle.c's orc_compose_poses; sin / cos /
 * sqrt are the device library's, so a composed entry may differ from a host libm composition in its last bit:
 * rbs_get_poses returns exactly what was evaluated).  On the host it costs two sin / cos / sqrt and a 3x3 product
 * per particle and body -- 0.25 ms at 2 000 particles, more than the device step.
 *   deltas         [n][n_objects][body_stride] doubles; of each body's body_stride (>= 6) values the first six are
 *                  read: position (3), rotation ("Euler") vector (3).  body_stride = 12 takes an array of dbot
 *                  FreeFloatingRigidBodiesState storage as it is (position, rotation vector, velocities).
 *   default_poses  [n_objects][body_stride], same layout: the sensor's integrated_poses().
 * Everything else -- indices in / out, update, out_loglik, errors, slabs -- as rbs_loglikes.  Single-device handles
 * and handles over several devices. */
int32_t rbs_loglikes_deltas(rbs_handle* h, const double* deltas, const double* default_poses, int32_t body_stride,
                            int32_t* indices, int32_t n, int32_t update, double* out_loglik);
/* The pinned staging block rbs_loglikes_deltas reads the deltas from, for callers whose particles are separate vectors (dbot's
 * StateArray: one Eigen vector per particle) and who must gather them anyway: gather position + rotation vector of every body, six
 * doubles each, particle-major ([n][n_objects][6], n <= max_particles) straight into *buf and pass *buf itself as `deltas` with
 * body_stride = 6 -- rbs_loglikes_deltas then skips its own staging copy.  The block is the handle's; valid until rbs_destroy; its
 * contents are consumed by the call.  Single-device handles. */
int32_t rbs_deltas_buffer(rbs_handle* h, double** buf);
/* Test / inspection hook: the absolute poses ([n][n_objects][12] doubles: R row-major, t) the handle's LAST
 * host-pointer likelihood call evaluated -- for rbs_loglikes the caller's own, for rbs_loglikes_deltas the
 * device's compositions.  Synchronises.  Single-device handles. */
int32_t rbs_get_poses(rbs_handle* h, double* out, int32_t n);

/* Block until everything enqueued on the handle's own stream has finished. */
int32_t rbs_synchronize(rbs_handle* h);

/* --- several devices in one handle --------------------------------------------------------
 * rbs_config.n_devices > 1 (the reference's tracker node is ONE process,
 * R:source/dbot_ros/tracker/particle_tracker_node.cpp:277-284): the handle shards the particles over
 * device_ids[].  Occlusion slots are GLOBAL, 0 .. n_devices * cap - 1 with
 * cap = ceil(max_particles / n_devices); slot g lives on device_ids[g / cap].  rbs_loglikes
 * evaluates particle i on the device that owns slot i (an updating call writes slot i there);
 * indices[i] may name a plane on any device -- a remote parent's window is read in place over
 * xGMI (peer access), nothing migrates.  rbs_set_observation* upload the frame to every device.
 * rbs_tracker_* on such a handle runs the filter replicated on every device, shards the sensor
 * call by a parent-affine layout and exchanges the log-likelihoods with one RCCL all-gather per
 * sampling block (librccl is bound with dlopen when such a handle is created).  The zero-copy
 * entry points work on such a handle too: rbs_set_observation_device takes a frame in the memory of
 * the FIRST device (device_ids[0]) and every device ingests it from there over xGMI;
 * rbs_loglikes_device takes poses / parent slots / results as arrays on the first device in global
 * particle order -- device k pulls its slice [k cap, (k+1) cap) and stores its log-likelihoods in
 * place (peer access) -- with `stream` a stream of the first device (NULL = the library's): the
 * devices start after the work enqueued on it so far, and it is ordered after all of them, so
 * d_out_loglik is complete in `stream` order without a host synchronisation; slot-addressed hooks (rbs_get/set_occlusion, rbs_get_window,
 * rbs_export/import_plane, rbs_occlusion_*device_ptr) take global slots and act on the owning
 * device; rbs_render_depth, rbs_get_observation, the timing queries answer for device_ids[0].
 * An ordinal may repeat in device_ids (several shards on one GPU: functional tests). */

/* --- occlusion state layout -------------------------------------------------------------
 * A slot's plane is stored as a WINDOW (a pixel rectangle) plus the handle-wide background
 * level: outside its window a plane equals the value a never-covered pixel has reached
 * (initial_occlusion_prob stepped by the occlusion process at every updating call).  An
 * updating call writes only bbox(parent's window, the particle's screen rectangle) and
 * re-tightens the child's window to the values that still differ from the background; the
 * process snaps a value within 2^-18 of the background onto it, so a window follows the object
 * instead of growing for ever.  The numbers are those of whole planes (oracle mode EAGER);
 * only the bytes moved change.  rbs_config.state_layout = RBS_STATE_DENSE keeps whole
 * planes (every updating call then copies every plane in full).  Every entry point below
 * hands out / accepts whole planes in either layout. */
/* --- inspection hooks (tests, state migration between devices) --- */
/* Window (x0, y0, x1, y1) of a slot's current plane; (cols, rows, 0, 0) = empty (all
 * background); (0, 0, cols, rows) always with state_layout dense. */
int32_t rbs_get_window(rbs_handle* h, int32_t slot, int32_t out[4]);
/* Never-covered occlusion level of the current planes. */
/* Shared trail (round 5).  With a scalar background a pixel stays in a window until its value has relaxed to within 2^-18 of
 * that level, ~730 frames after the object left it, and every child inherits the whole trail from its parent: an object that
 * moves across the image leaves windows of most of the frame, stored, read and stepped once per particle per frame.  Once the
 * sampled window area exceeds a tenth of the frame, a handle on windowed planes (whole planes or slabs; either likelihood precision,
 * round 6) stores its planes against a handle-wide background PLANE instead: the plane is re-based on one particle's plane and every child is
 * re-measured against it, so that what the particles share from a common ancestor is stored once (after a resampling that is
 * nearly all of it).  Stored VALUES do not change by a bit -- the shared plane steps with the float operations of any stored
 * value -- and every entry point sees whole planes as before (rbs_get_occlusion, rbs_export_window: the slot is made dense first).
 * RBS_SHARED_TRAIL=0 in the environment disables it; handles over several devices and attached ranks: see rbs_shared_trail_rebase below.
 * Inspection: *active = the handle has switched, *rebases = how often it re-based so far. */
int32_t rbs_shared_trail_state(rbs_handle* h, int32_t* active, int32_t* rebases);
/* Round 6: the shared trail where OTHERS read a handle's planes in place.  A handle over several devices (rbs_config.n_devices) takes
 * ONE decision per call for all its shards -- every device keeps its own, identical copy of the shared plane, stepped alike and
 * re-based in the same call on the same global slot, whose plane the other devices read from its owner -- and needs nothing from the
 * caller.  Handles of one process per GPU (rbs_ipc_export / rbs_ipc_attach) cannot agree among themselves: the CALLER, who owns the
 * collective, tells every rank before the SAME updating call -- rbs_shared_trail_rebase(h, global_slot): at the next updating call the
 * handle enters the shared-trail representation if it has not yet and re-bases its shared plane on that global slot's plane (any
 * rank's; read in place); global_slot = -2: it returns to the scalar background at that call.  Same slot, same call, every rank --
 * dbot_ros_amd/dist.py PeerShardedStep does it (shared_trail=True: every 32 steps while any rank's windows exceed a tenth of the
 * frame, agreed by one all-reduce of a flag).  On a handle of its own the call forces a re-basing on one of its slots (tests).
 * Values are unchanged by a bit, as for a single handle; an exported handle never switches by itself. */
int32_t rbs_shared_trail_rebase(rbs_handle* h, int32_t global_slot);
/* Behaviour switches a caller may need, as an API (round 6; the environment variables of the same meaning are tooling and are read
 * once at rbs_create -- INTEGRATION.md section 6 lists them).  Values take effect from the next call on; results never depend on them
 * (they choose what is stored and how a call is launched).
 *   RBS_OPT_SHARED_TRAIL        0 / 1   may the handle store its planes against a shared background plane (default 1; a handle that
 *                                       has already switched stays so until rbs_reset)
 *   RBS_OPT_SHARED_TRAIL_ENTER  (0, 1]  sampled window fraction of the frame above which it switches / keeps re-basing (default 0.10)
 *   RBS_OPT_SHARED_TRAIL_EVERY  >= 1    updating calls between re-basings while windows stay large (default 32)
 *   RBS_OPT_TRACKER_SPLIT_MAX   >= 0    rbs_tracker_*: evaluations per frame up to which a frame handed over frame by frame travels
 *                                       behind the geometry kernel (two-kernel launch; default 5 000, 0 = never)
 *   RBS_OPT_TIMING_EVERY        >= 1    = rbs_set_timing_every
 * A handle over several devices applies them to all its shards. */
enum { RBS_OPT_SHARED_TRAIL = 1, RBS_OPT_SHARED_TRAIL_ENTER = 2, RBS_OPT_SHARED_TRAIL_EVERY = 3, RBS_OPT_TRACKER_SPLIT_MAX = 4, RBS_OPT_TIMING_EVERY = 5 };
int32_t rbs_set_option(rbs_handle* h, int32_t option, double value);
/* The window area the handle sampled last (mean over its particles of the region an updating call stored, as a fraction of the
 * frame; sampled every 8th updating call, read back without blocking): what the shared trail's policy looks at. */
int32_t rbs_window_fraction(rbs_handle* h, double* out);
int32_t rbs_get_background(rbs_handle* h, float* out);
/* Stored occlusion plane of a slot -> host float[rows*cols]. */
int32_t rbs_get_occlusion(rbs_handle* h, int32_t slot, float* out);
/* Overwrite a slot's plane from host float[rows*cols]. */
int32_t rbs_set_occlusion(rbs_handle* h, int32_t slot, const float* plane);
/* Device address of a slot's current plane, made whole first (valid until the next updating call). */
int32_t rbs_occlusion_device_ptr(rbs_handle* h, int32_t slot, void** out);
/* Device address of slot's plane in the buffer the NEXT updating call will write. */
int32_t rbs_occlusion_next_device_ptr(rbs_handle* h, int32_t slot, void** out);
/* Device-to-device copy of a slot's plane to / from caller-owned device memory (float[rows*cols]
 * on the handle's device), enqueued on `stream` (NULL = the handle's stream) after the planes of
 * the last updating call are complete: the migration path between GPUs (a torch.distributed /
 * RCCL send or recv of the caller's buffer), without staging through the host. */
int32_t rbs_export_plane(rbs_handle* h, int32_t slot, void* d_dst, void* stream);
int32_t rbs_import_plane(rbs_handle* h, int32_t slot, const void* d_src, void* stream);
/* The same transport, WINDOW-SIZED (round 4): a plane is its window plus the background level, so what
 * has to travel is the window's rectangle and its w x h values (about 3 % of a plane), not rows*cols
 * floats.  rbs_export_window: rect_out = (x0, y0, x1, y1) of the slot's window -- (cols, rows, 0, 0) when
 * the plane is all background -- and its values packed row-major, width x1 - x0, into d_payload
 * (device memory of the handle's device, capacity_floats floats; too small: RBS_ERR_INVALID_ARGUMENT
 * with nothing copied, rect_out still valid so the caller can size the buffer).  Waits for the
 * rectangle (one 16-byte read-back); the payload copy is enqueued on `stream`.
 * rbs_import_window: the slot's plane becomes "background everywhere, these values inside rect"
 * (x0 and x1 multiples of 4, inside the frame); a slab that is too small for rect is ENLARGED first, as
 * behind rbs_import_plane (one drain of the handle; every rank grows its slabs on its own schedule, so a
 * window from a rank that has grown must not be refused by one that has not) -- only the shards of a
 * multi-device handle and handles attached to other ranks (rbs_ipc_attach), whose slabs are addressed with
 * a fixed stride from outside, fail with RBS_ERR_OUT_OF_MEMORY.  Both layouts, whole planes and slabs.
 * Used by dbot_ros_amd/dist.py (one process per GPU) to migrate a parent's plane to the rank its
 * surplus children were placed on: an RCCL send / recv of rect + payload. */
int32_t rbs_export_window(rbs_handle* h, int32_t slot, int32_t rect_out[4], void* d_payload, size_t capacity_floats, void* stream);
int32_t rbs_import_window(rbs_handle* h, int32_t slot, const int32_t rect[4], const void* d_payload, void* stream);
/* `stream` waits (on the device, no host synchronisation) until the planes of the handle's last
 * updating call are complete, the side stream's copy kernel included: what a caller enqueues on
 * `stream` afterwards -- e.g. the collective that tells the other ranks "my step is done" -- is
 * ordered after them. */
int32_t rbs_stream_join(rbs_handle* h, void* stream);

/* --- particle sharding ACROSS PROCESSES: one process per GPU (torch.distributed / RCCL) ------------
 * SURVEY 8(e)'s partitioning with one handle per rank: rank r owns global slots
 * [r * max_particles, (r + 1) * max_particles).  After rbs_ipc_attach the parent indices of
 * rbs_loglikes / rbs_loglikes_device are GLOBAL slots: a parent that lives in another rank's handle
 * is read IN PLACE over xGMI -- its window's ~3 % of a plane, once -- through that rank's buffers
 * mapped into this process (hipIpcGetMemHandle / hipIpcOpenMemHandle), exactly as the shards of a
 * multi-device handle read each other (rbs_config.n_devices).  No plane ever migrates; the only
 * collective of a filter step is the all-gather of the log-likelihoods.
 *   rbs_ipc_export   this handle's description (RBS_IPC_BLOB_BYTES bytes): memory handles of its two
 *                    plane buffers, window and region tables, its device and geometry.  Single-device
 *                    handles only; synchronises.
 *   rbs_ipc_attach   blobs = world x RBS_IPC_BLOB_BYTES, rank-major, every rank's export (exchanged by
 *                    the caller: an all-gather of bytes); rank = this handle's.  All handles must have
 *                    the same geometry, layout, max_particles and slab size.  Afterwards children are
 *                    still written to LOCAL slots 0..n-1 (global rank * max_particles + i); an updating
 *                    rbs_loglikes returns indices[i] = rank * max_particles + i.
 * ORDERING is the caller's: every rank performs the same sequence of rbs_reset / updating calls, and a
 * rank may start step k+1 only when every rank has finished step k (it reads their planes and
 * overwrites the buffer they were reading) -- enqueue rbs_stream_join and then the step's all-gather
 * on the stream the next call is enqueued on (bench.py --gpus N, dbot_ros_amd/dist.py PeerShardedStep).
 * Slabs do not grow once attached (the other ranks address them with a fixed stride): a region that
 * does not fit is an error; size state_slab_px for the scene. */
#define RBS_IPC_BLOB_BYTES 512
int32_t rbs_ipc_export(rbs_handle* h, void* blob_out);
int32_t rbs_ipc_attach(rbs_handle* h, int32_t rank, int32_t world, const void* blobs);
/* Parents that SEVERAL of this rank's children share are better pulled once than read in place by every
 * child: for i in [0, n) with d_dst_local[i] >= 0, the plane of global slot d_src_global[i] (any rank's)
 * is copied -- its window only -- into local slot d_dst_local[i] of the current buffer, on `stream`, no
 * host synchronisation (entries with d_dst_local[i] < 0 are skipped, so the arrays can have a fixed
 * length).  The caller keeps local slots for this (max_particles > the particles it evaluates) and names
 * the staged copy -- global slot rank * max_particles + d_dst_local[i] -- as the children's parent.
 * Both arrays in device memory.  Works on an unattached handle as well (src = local slots). */
int32_t rbs_stage_windows(rbs_handle* h, const int32_t* d_src_global, const int32_t* d_dst_local, int32_t n, void* stream);
/* The resampling half of the filter step across processes in one call: three or four launches on `stream` (two or three over
 * the chip for the cdf and the children's parents, one block for the plan), no host synchronisation after the first call, which
 * allocates scratch: what dbot_ros_amd/dist.py global_resample + plan_shard
 * compute with ~45 tensor kernels.  d_loglik_all [n_total = world * n_local]: the all-gathered
 * log-likelihoods, rank-major.  d_uniforms_sorted [n_total]: the step's uniforms in [0, 1), identical on
 * every rank and ASCENDING -- multinomial resampling (parent = upper_bound(cumulative normalised
 * weights, u); weights exp((ll - max) / temperature), temperature 1 = the filter's own) draws exchangeable
 * children, and u -> parent is monotone, so sorted uniforms give the children sorted by parent: child g of
 * the job is evaluated by rank g / n_local, and in that order the children of rank r's particles are one
 * contiguous run that mostly coincides with rank r's slots.  A NaN log-likelihood (a contained particle)
 * weighs nothing.  Outputs, all in device memory, [n_local] each unless noted:
 *   d_parent_idx     the GLOBAL slot local child k inherits from -- owner * max_particles + local slot --
 *                    or, for a parent on another rank that at least min_share of this rank's children
 *                    share, the local staging slot rank * max_particles + n_local + j
 *   d_stage_src/dst  the arguments of rbs_stage_windows(h, src, dst, n_local, stream), which the caller
 *                    enqueues next: entry k pulls global slot src[k] into local slot dst[k] iff dst[k] >= 0
 *   d_parents_local  (may be null) each local child's parent as an index into d_loglik_all
 *   d_counts [4]     int64, ACCUMULATED: children with a parent on another rank, of them served from
 *                    staging, windows staged, distinct parents among this rank's children
 * The handle needs max_particles >= 2 * n_local (own slots + staging slots); an attached handle must be
 * rank `rank` of n_total / n_local.  Deterministic: every rank derives the same parents bit for bit.
 * Replaces nothing in the reference (its filter is one process: R:source/dbot_ros/tracker/
 * particle_tracker_node.cpp:277-284); it is the step north_star's "RCCL all-reduce of log-weights before
 * resampling" leaves to each rank. */
int32_t rbs_peer_resample(rbs_handle* h, const double* d_loglik_all, const double* d_uniforms_sorted, int32_t n_total, int32_t n_local,
                          int32_t rank, int32_t min_share, double temperature, int32_t* d_parent_idx, int32_t* d_stage_src,
                          int32_t* d_stage_dst, int32_t* d_parents_local, int64_t* d_counts, void* stream);

/* Rasterize one pose [n_objects][12] -> host float[rows*cols], +inf where uncovered. */
int32_t rbs_render_depth(rbs_handle* h, const double* pose, float* out);
/* Device time in milliseconds of the most recent rbs_loglikes* call (HIP events recorded on the
 * launch stream around its kernels); blocks until it finished. */
int32_t rbs_last_kernel_ms(rbs_handle* h, float* ms);
/* Averages over the timed calls among the last last_n rbs_loglikes* calls (the library brackets
 * every 8th call with HIP events -- rbs_set_timing_every changes that -- and keeps the last 256
 * timed calls), from events recorded on the streams the kernels
 * run on: call_ms = the launch-stream part of a call
 * (frame terms + rectangles kernel, raster kernel); copy_kernel_ms = the copy kernel alone on its own
 * stream (updating calls only, 0 if none).  Blocks until those calls finished. */
int32_t rbs_timing_summary(rbs_handle* h, int32_t last_n, float* call_ms, float* copy_kernel_ms,
                           int32_t* n_used);
/* Bracket every `every`-th rbs_loglikes* call with timing events from now on (default 8; the
 * library keeps the last 256 timed calls).  bench.py's kernel-timing pass uses 2. */
int32_t rbs_set_timing_every(rbs_handle* h, int32_t every);
/* Same window of calls: the raster kernel alone (HIP events around it on the launch stream). */
int32_t rbs_raster_kernel_ms(rbs_handle* h, int32_t last_n, float* raster_kernel_ms);

/* ------------------------------------------------------------------------------------------
 * Device-side tracker (the callers either side of the hot path): the object
 * state transition, the RBC particle-filter step (weights, KL test, multinomial resampling)
 * and the tracker's weighted mean, run on the sensor's device around rbs_loglikes_device with
 * one host synchronisation per frame.  Replaces, for use_gpu trackers,
 *   dbot::ObjectTransitionBuilder<State>  R:source/dbot_ros/tracker/particle_tracker_node.cpp:138-159
 *   dbot::ParticleTrackerBuilder<Tracker> R:source/dbot_ros/tracker/particle_tracker_node.cpp:208-218
 *   tracker->initialize / tracker_->track R:...particle_tracker_node.cpp:252,
 *                                         R:source/dbot_ros/object_tracker_ros.hpp:49
 * States are in MODEL coordinates (pose of the centred mesh frame); the host mirrors do the
 * center_object_frame conversion and the moving average. */
typedef struct rbs_tracker rbs_tracker;

typedef struct rbs_tracker_params {
    double linear_sigma[3];      /* object_transition/linear_sigma_{x,y,z}  */
    double angular_sigma[3];     /* object_transition/angular_sigma_{x,y,z} */
    double velocity_factor;      /* object_transition/velocity_factor       */
    double max_kl_divergence;    /* particle_filter/max_kl_divergence       */
    int32_t n_particles;         /* evaluation_count / #objects; <= the sensor's max_particles */
} rbs_tracker_params;

/* The tracker borrows `sensor` (must outlive it) and drives it on the sensor's own stream. */
int32_t rbs_tracker_create(rbs_handle* sensor, const rbs_tracker_params* params, rbs_tracker** out);
void rbs_tracker_destroy(rbs_tracker* t);
/* default_state: [n_objects*12] = per body position, rotation vector, linear + angular velocity.
 * Particles := zero deltas, weights := uniform, sensor reset. */
int32_t rbs_tracker_initialize(rbs_tracker* t, const double* default_state);
/* One frame.  frame: float32[rows*cols] evaluated-resolution depth (NULL: the caller has
 * already called an rbs_set_observation* variant for this frame).  normals: [n_objects][n][6]
 * standard normals, uniforms: [n_objects][n] in [0,1) -- host-supplied randomness (reproducible,
 * used by the parity tests); either may be NULL to draw on the device (Philox4x32-10 keyed by
 * `seed` and the frame counter).  Outputs: the updated default state [n_objects*12] and the
 * number of resamplings so far. */
int32_t rbs_tracker_track(rbs_tracker* t, const float* frame, const double* normals,
                          const double* uniforms, uint64_t seed, double* out_state,
                          int32_t* out_resamplings);
/* The same frame in two halves, for callers that have the NEXT frame before they need this frame's
 * estimate (dataset replay, a camera that outruns the consumer): rbs_tracker_submit enqueues a
 * frame's work and returns at once -- the caller's frame / normals / uniforms buffers are free on
 * return -- and rbs_tracker_result waits for the OLDEST submitted frame and hands out its state.
 * Up to two frames may be in flight: the second frame's host copy and upload run beside the first
 * frame's kernels (host frames travel on their own stream).  rbs_tracker_track == submit + result.
 * Frames are processed strictly in order; the numbers are those of rbs_tracker_track. */
int32_t rbs_tracker_submit(rbs_tracker* t, const float* frame, const double* normals,
                           const double* uniforms, uint64_t seed);
int32_t rbs_tracker_result(rbs_tracker* t, double* out_state, int32_t* out_resamplings);
/* The same two with the image as dbot's tracker receives it -- rows*cols DOUBLES (Obsrv of R:source/dbot_ros/object_tracker_ros.h:40-41,
 * filled by ri::to_eigen_vector, R:source/dbot_ros/util/ros_interface.h:152-168): converted to float while it is staged (AVX2), and, frame
 * by frame with at most 5 000 evaluations, staged BEHIND the sensor's geometry kernel like any borrowed frame (the buffer is free on return). */
int32_t rbs_tracker_track_f64(rbs_tracker* t, const double* frame, const double* normals, const double* uniforms, uint64_t seed,
                              double* out_state, int32_t* out_resamplings);
int32_t rbs_tracker_submit_f64(rbs_tracker* t, const double* frame, const double* normals, const double* uniforms, uint64_t seed);
/* Inspection: particle deltas [n][n_objects*12], log-weights [n], occlusion slot map [n]
 * (any pointer may be NULL). */
int32_t rbs_tracker_get(rbs_tracker* t, double* particles, double* log_weights, int32_t* indices);

/* Posterior report (opt-in): what the filter knows about its own estimate, reduced on the device at the end of every
 * frame -- the spread a consumer fuses or gates with (a PoseWithCovariance), and the health of the sample.
 *
 * The rule.  At the end of a frame, after the last sampling block's resampling and gather, the tracker holds n particles:
 * x_i in R^D, D = 12 n_objects, the RE-CENTRED deltas -- exactly what rbs_tracker_get returns after that frame (pose
 * components relative to the frame's estimate, velocities as they are) -- their log-weights lw_i and the occlusion slot
 * map idx_i.  With m = max lw, e_i = exp(lw_i - m), S = sum e_i (lw_i = -inf: e_i = 0, the particle contributes nothing; at
 * least one lw_i is finite, as the filter's own weights require -- with all of them -inf the moments and ess are NaN):
 *   mean[c]   = (sum e_i x_i[c]) / S
 *   cov[a][b] = (sum e_i (x_i[a] - mean[a]) (x_i[b] - mean[b])) / S      two passes: the mean first, then central moments
 *               (raw moments minus mean mean^T cancel on the velocities); the upper triangle is computed and mirrored,
 *               so the matrix is symmetric bit for bit
 *   ess       = S^2 / sum e_i^2
 *   survivors = the number of distinct values among idx_i: distinct occlusion planes alive, i.e. distinct parents of the
 *               last block's resampling; n when that block did not resample
 *   resampled = the last block's resampling decision;  n;  frame = frames tracked since rbs_tracker_initialize (1, 2, ...)
 * Every sum is taken in binary64 in a fixed order that depends on n only (no floating-point atomics): two runs give the
 * same bits, and so do frame by frame and look-ahead.  Below 8 192 particles one block reduces, from there on a grid with
 * per-block partials folded in block order; the two forms may differ from each other in the last bits.
 * Convention.  Components per body: position (3), rotation vector (3), linear velocity (3), angular velocity (3), bodies in
 * order.  Pose rows and columns need no conversion for the MODEL frame: translation deltas add in the camera frame, rotation
 * deltas multiply from the left, R = R(delta) R(default) -- a left perturbation in camera axes.  (The host mirrors convert
 * to the published pose of a centred mesh.)
 *
 * rbs_tracker_set_posterior: enable != 0 switches the report on (allocating its buffers the first time), 0 off.  Off --
 * the default -- a frame enqueues exactly what it did before the report existed.  Frames in flight:
 * RBS_ERR_INVALID_ARGUMENT; a tracker over several devices: RBS_ERR_UNSUPPORTED.  The filter itself is not touched: estimates
 * and particles are bit for bit those of a tracker with the report off.
 * rbs_tracker_posterior: the report of the frame most recently handed out by rbs_tracker_result / rbs_tracker_track*
 * (with look-ahead: of frame k after result(k), while k + 1 is in flight).  mean [D], cov [D][D] row-major; info, mean, cov
 * may each be NULL.  RBS_ERR_INVALID_ARGUMENT while the report is off, before the first frame, and after
 * rbs_tracker_initialize until the next result; a poisoned tracker's error otherwise. */
typedef struct rbs_tracker_posterior_info {
    int32_t n;            /* particles */
    int32_t survivors;    /* distinct occlusion slots among the particles */
    int32_t resampled;    /* 1: the frame's last sampling block resampled */
    int32_t frame;        /* frames tracked since rbs_tracker_initialize */
    double ess;           /* effective sample size, 1 .. n */
} rbs_tracker_posterior_info;
int32_t rbs_tracker_set_posterior(rbs_tracker* t, int32_t enable);
int32_t rbs_tracker_posterior(rbs_tracker* t, rbs_tracker_posterior_info* info, double* mean, double* cov);
/* Device time of that report's kernels, first launch to last (HIP events on the tracker's stream), in milliseconds.
 * RBS_ERR_INVALID_ARGUMENT wherever rbs_tracker_posterior has no report. */
int32_t rbs_tracker_posterior_ms(rbs_tracker* t, float* ms);

/* Posterior modes (opt-in): is the posterior one hump or several, and where are they -- the question a particle filter can
 * answer and a mean with a covariance cannot.  A box seen from one side, a re-find, an occluder: the cloud splits, its mean is a
 * pose in neither hump, and its covariance says nothing of where to look.  The modes are found on the device by an all-pairs
 * weighted kernel density over the particles (n^2 pair terms per body).
 *
 * The rule.  Inputs are the posterior report's: the RE-CENTRED deltas x_i rbs_tracker_get returns after the frame and the
 * log-weights lw_i;  m = max lw,  e_i = exp(lw_i - m), and e_i = 0 where that is below 2^-960 (lw_i = -inf, or 289 orders
 * of magnitude below the heaviest particle: no belief, and binary64 products of such a weight would be subnormal and lose
 * the bits the sums' error bounds count on),  S = sum e_i.  Bodies are treated independently
 * (the filter samples them in blocks of their own, and joint modes in 6 n_objects dimensions are too sparse for a few thousand
 * particles).  For a body: p_i the particle's position delta, r_i its rotation-vector delta,
 *   q_i = (cos(|r_i| / 2), sin(|r_i| / 2) r_i / |r_i|)   the unit quaternion, (1, 0, 0, 0) at r_i = 0
 *   d2(i, j) = |p_i - p_j|^2 / h_t^2  +  4 (1 - (q_i . q_j)^2) / h_r^2
 *              (4 (1 - c^2) = 4 sin^2(theta / 2) of the relative rotation angle theta: theta^2 to second order, blind to the
 *              sign of a quaternion, the same for r and its equivalent beyond pi)
 *   rho_i    = (1 / S) sum_j e_j max(0, 1 - d2(i, j))     compact support: no exp in the pair loop
 * Selection, at most k_max rounds: the candidates are the particles with e_i > 0 that are not suppressed; the seed s_k is the
 * candidate of largest rho, the lowest index on a tie; then every i with d2(i, s_k) < separation^2 is suppressed; the rounds
 * stop when no candidate is left.  Assignment: every particle with e_i > 0 belongs to the seed of smallest d2, the earlier
 * mode on a tie.  mass_k = (sum of e over the members) / S: the masses sum to 1.  The mode's CORE is its members with
 * d2(i, s_k) < 1, core_mass_k their share; the mode's position delta is the e-weighted mean of the core's p_i, its rotation the
 * normalised e-weighted sum of sign(q_i . q_s) q_i over the core (h_r <= 1 keeps |q_i . q_s| > 0.86 there) turned back into a
 * rotation vector with angle in [0, pi].
 * Every sum is taken in binary64 in a fixed order that depends on n and the parameters only (no floating-point atomics): two
 * runs give the same bits, and so do frame by frame and look-ahead.
 *
 * Parameters: h_t > 0 (metres), 0 < h_r <= 1 (radians), separation >= 1, 1 <= k_max <= RBS_MODES_MAX.
 * rbs_modes_default_params fills the starting values -- 0.02 m, 0.2 rad, 2, 4 -- which are UNMEASURED: chosen from the scale
 * of the transition noise, not tuned on data.
 * At most 65 536 particles (the pair pass is n^2): RBS_ERR_UNSUPPORTED above. */
#define RBS_MODES_MAX 8
typedef struct rbs_modes_params {
    double h_t;           /* translation bandwidth, metres */
    double h_r;           /* rotation bandwidth, radians */
    double separation;    /* suppression radius in bandwidths */
    int32_t k_max;        /* most modes returned per body */
    int32_t reserved;     /* 0 */
} rbs_modes_params;
typedef struct rbs_mode {
    int32_t seed;         /* the particle the mode was seeded at (-1: unused entry) */
    int32_t reserved;
    double density;       /* rho at the seed */
    double mass;          /* share of the belief assigned to the mode */
    double core_mass;     /* ... within one bandwidth of the seed */
    double delta[6];      /* the core's mean pose: position delta, rotation-vector delta (re-centred, as rbs_tracker_get's) */
} rbs_mode;
typedef struct rbs_body_modes {
    int32_t n_modes;      /* 1 .. k_max */
    int32_t reserved;
    rbs_mode mode[RBS_MODES_MAX];   /* in selection order; entries from n_modes on are unused */
} rbs_body_modes;
void rbs_modes_default_params(rbs_modes_params* p);
/* Stateless, on host arrays (the host-side filter, tests): deltas [n][n_objects][6] (position, rotation vector per body),
 * log_weights [n] (finite or -inf, at least one finite), out [n_objects].  Synchronous.  RBS_ERR_INVALID_ARGUMENT: n < 1, n above
 * the sensor's max_particles, parameters out of range, a null pointer, a log-weight that is NaN or +inf, all of them -inf, a
 * delta that is not finite; RBS_ERR_UNSUPPORTED: a handle over several devices, n > 65 536. */
int32_t rbs_pose_modes(rbs_handle* h, const double* deltas, const double* log_weights, int32_t n, const rbs_modes_params* params,
                       rbs_body_modes* out);
/* The device tracker's report, on the pattern of the posterior report: params != NULL switches it on with these parameters
 * (allocating its buffers the first time), NULL off.  Off -- the default -- a frame enqueues exactly what it did before the
 * report existed; on, its kernels are launched behind the frame's chain (behind the posterior report's when that is on too; the
 * two are independent and neither needs the other) into a pinned slot per in-flight frame, with an event of its own.  Frames in
 * flight: RBS_ERR_INVALID_ARGUMENT; a tracker over several devices or of more than 65 536 particles: RBS_ERR_UNSUPPORTED.  The
 * filter itself is not touched: estimates and particles are bit for bit those of a tracker with the report off.
 * rbs_tracker_modes: the report of the frame most recently handed out by rbs_tracker_result / rbs_tracker_track* (with
 * look-ahead: of frame k after result(k), while k + 1 is in flight); out [n_objects]; frame (may be NULL): frames tracked since
 * rbs_tracker_initialize.  RBS_ERR_INVALID_ARGUMENT while the report is off, before the first frame, and after
 * rbs_tracker_initialize until the next result; a poisoned tracker's error otherwise.
 * rbs_tracker_modes_ms: device time of that report's kernels, first launch to last, in milliseconds. */
int32_t rbs_tracker_set_modes(rbs_tracker* t, const rbs_modes_params* params);
int32_t rbs_tracker_modes(rbs_tracker* t, int32_t* frame, rbs_body_modes* out);
int32_t rbs_tracker_modes_ms(rbs_tracker* t, float* ms);

/* ------------------------------------------------------------------------------------------
 * Robust Gaussian tracker (the reference's second tracker, R:source/dbot_ros/tracker/gaussian_tracker_node.cpp):
 * an unscented-transform Gaussian filter over the object state with pixels as conditionally independent
 * sensors and a per-pixel robust body weight -- DESIGN.md Appendix G states the arithmetic.  On the
 * sensor's device: the 1 + 12 n_objects distinct sigma poses are rendered (the particle path's binary64
 * rasterizer, depths bit-identical to the oracle's) and the per-pixel moments reduced in a fixed order
 * (deterministic: no floating-point atomics); on the host, in binary64: predict, Cholesky, sigma poses,
 * the 6 n_objects x 6 n_objects solve and the re-centring -- one host synchronisation per frame.
 * States are in MODEL coordinates like rbs_tracker_*; D = 12 n_objects.
 * Limits: n_objects <= 3; single-device handles only (several devices or an attached rank:
 * RBS_ERR_UNSUPPORTED).  A sensor handle drives ONE tracker at a time -- particle or Gaussian -- since
 * both set its observation. */
typedef struct rbs_gauss rbs_gauss;

typedef struct rbs_gauss_params {
    double linear_sigma[3];      /* gaussian_filter/object_transition/linear_sigma_{x,y,z}  (>= 0) */
    double angular_sigma[3];     /* gaussian_filter/object_transition/angular_sigma_{x,y,z} (>= 0) */
    double velocity_factor;      /* gaussian_filter/object_transition/velocity_factor */
    double ut_alpha;             /* gaussian_filter/unscented_transform/alpha (> 0; beta = 2, kappa = 0) */
    double fg_noise_std;         /* gaussian_filter/observation/fg_noise_std (> 0) */
    double bg_depth;             /* gaussian_filter/observation/bg_depth */
    double bg_noise_std;         /* gaussian_filter/observation/bg_noise_std (>= 0) */
    double tail_weight;          /* gaussian_filter/observation/tail_weight, in [0, 1) */
    double uniform_tail_min;     /* gaussian_filter/observation/uniform_tail_{min,max}: max > min */
    double uniform_tail_max;
} rbs_gauss_params;

/* The tracker borrows `sensor` (must outlive it) and runs on the sensor's own stream.  Invalid
 * parameters: RBS_ERR_INVALID_ARGUMENT (message via rbs_last_error(NULL) when sensor is NULL). */
int32_t rbs_gauss_create(rbs_handle* sensor, const rbs_gauss_params* params, rbs_gauss** out);
void rbs_gauss_destroy(rbs_gauss* g);
/* default_state [D]: the default pose z (velocities as given); mean delta := 0; covariance := cov0
 * [D][D] (symmetric positive definite), or NULL: per body diag(lin^2, ang^2, lin^2, ang^2). */
int32_t rbs_gauss_initialize(rbs_gauss* g, const double* default_state, const double* cov0);
/* One frame.  frame: float32[rows*cols] (NULL: already set through an rbs_set_observation* call).
 * out_state [D]: the re-centred default state (pose, and the mean's velocities); out_cov [D][D] or NULL. */
int32_t rbs_gauss_track(rbs_gauss* g, const float* frame, double* out_state, double* out_cov);
/* The same with rows*cols DOUBLES (dbot's Obsrv): rounded to float while staged, as rbs_set_observation. */
int32_t rbs_gauss_track_f64(rbs_gauss* g, const double* frame, double* out_state, double* out_cov);
/* Inspection, for the parity tests: the last frame's default state z [D], predicted mean [D] and
 * covariance [D][D] (any pointer may be NULL) ... */
int32_t rbs_gauss_get_prior(rbs_gauss* g, double* default_state, double* mean, double* cov);
/* ... its distinct sigma poses [n][n_objects][12] (R row-major | t), n = 1 + 12 n_objects: the centre,
 * then + and - of every pose column of the Cholesky factor (pose-first order) ... */
int32_t rbs_gauss_get_sigma_poses(rbs_gauss* g, double* out, int32_t* n);
/* ... the depth image of sigma pose k (+inf where nothing is covered) ... */
int32_t rbs_gauss_get_render(rbs_gauss* g, int32_t k, float* out);
/* ... the reduced moments exactly as the host read them: out [NE], NE = 6B(6B+1)/2 + 6B (B = n_objects), the
 * upper triangle of Lambda - I row-major (a <= b), then eta; *n := NE.  RBS_ERR_INVALID_ARGUMENT before the
 * first frame or for a NULL pointer ... */
int32_t rbs_gauss_get_moments(rbs_gauss* g, double* out, int32_t* n);
/* ... and its device time in ms: [0] render, [1] moments, [2] reduction (HIP events); a frame of
 * rbs_gauss_submit: [2] is the reduction + update kernel.  These five describe the last COMPLETED
 * frame, whichever path ran it, and return RBS_ERR_INVALID_ARGUMENT while frames are in flight. */
int32_t rbs_gauss_kernel_ms(rbs_gauss* g, float* out3);

/* The same frame in two halves, with the whole filter step on the device (predict, Cholesky and sigma
 * poses in one kernel, the update and re-centring in another; the belief stays in device memory):
 * rbs_gauss_submit enqueues one frame and returns at once (the caller's buffer is free on return);
 * rbs_gauss_result hands out the estimates in submission order, as rbs_gauss_track would have
 * (out_cov may be NULL).  At most two frames in flight; a third submit, a result with nothing in
 * flight, and rbs_gauss_track or inspection while frames are in flight: RBS_ERR_INVALID_ARGUMENT.
 * A frame whose algebra fails returns from rbs_gauss_result with rbs_gauss_track's code and message
 * for that condition, as does a frame in flight behind it; a failure half-way through submit drains
 * the stream.  Either way the tracker refuses frames until rbs_gauss_initialize (which also drops
 * frames still in flight).  At a frame boundary rbs_gauss_track and submit / result interleave: the
 * belief carries over both ways. */
int32_t rbs_gauss_submit(rbs_gauss* g, const float* frame);   /* NULL: a frame staged by rbs_set_observation* */
int32_t rbs_gauss_submit_f64(rbs_gauss* g, const double* frame);
int32_t rbs_gauss_result(rbs_gauss* g, double* out_state, double* out_cov);

/* ---------------------------------------------------------------------------------------------------------
 * Object finder: the object's initial pose from one depth frame, without a prior.  The reference answers a
 * request with auto_detect set by calling an external FindObject service and starting the tracker at the pose
 * it returns (R:source/dbot_ros/tracker/object_tracker_controller_service_node.cpp:143-167, "controller" below);
 * rbs_find_run is that service's search, on the device.
 *
 * The score of a pose is the log-likelihood rbs_loglikes(update = 0) gives it on a freshly reset handle of the
 * sensor's configuration: the first frame after rbs_reset, every index 0 -- what a tracker started at that pose
 * sees on its first frame -- in a call of at least 2 x (compute units) poses (512 on an MI355X): the finder scores
 * through the sensor's own raster kernels (same precision, occlusion mode, layout) on handles of its own, whose tile
 * split is fixed to that of such calls.  A smaller rbs_loglikes call splits a rectangle into more pieces and sums in
 * another order, so re-scoring one returned pose in a call of one pose agrees to rounding, not bit for bit; pad such
 * a call (repeat the pose) for the same bits.  Every stage is deterministic and none depends on `batch`.
 *
 *   1 coarse frame  the frame sub-sampled by f = coarse_downsampling (every f-th pixel of every f-th row, as
 *                   ri::to_eigen_vector; K's top two rows divided by f); 0: the largest of {1, 2, 4} that leaves
 *                   >= 160 columns.
 *   1b foreground   opt-in (rbs_find_set_foreground; off by default): the dominant plane of the coarse frame is found and
 *                   the seeds of step 2 are taken from a SEEDING FRAME, the coarse frame with every pixel that is not
 *                   strictly in front of that plane set to NaN.  Scoring (steps 4, 6) still reads the whole frames.  All
 *                   of it is binary64 with + - * / and comparisons only, in the order written, on the device.  (u, v) a
 *                   coarse pixel's column and row, d its depth, valid: min_depth <= d <= max_depth (step 2's test),
 *                   sigma(z) = model_sigma + sigma_factor (z z) of the sensor's rbs_config, npx the coarse pixels.
 *                   Trial t < plane_trials draws pixels i_k = (uint64(word_k) npx) >> 32, k = 0, 1, 2, from the words of
 *                   Philox4x32-10 (key = seed, counter words (t, 0, 0, 0xFFFFFFFF): step 6's last word is a round <= 64).
 *                   D = (u1 - u0)(v2 - v0) - (u2 - u0)(v1 - v0).  A trial is void when a pixel is not valid or D == 0;
 *                   else, q_k = 1 / d_k, its plane in inverse depth is a = ((q1 - q0)(v2 - v0) - (q2 - q0)(v1 - v0)) / D,
 *                   b = ((u1 - u0)(q2 - q0) - (u2 - u0)(q1 - q0)) / D, c = (q0 - a u0) - b v0.  Its count: the valid coarse
 *                   pixels (all, not the seed grid) with w = (a u + b v) + c > 0 and, z = 1 / w,
 *                   |d - z| <= ransac_sigmas sigma(z); a void trial counts -1.  The highest count wins, ties to the lowest
 *                   t; the plane is accepted when count >= 3 and count >= min_inlier_fraction n_valid.  The chosen plane
 *                   IS that trial's three-point plane: there is no least-squares refit.  A pixel of the seeding frame
 *                   keeps its depth when no plane is accepted, or w <= 0, or z - d > mask_sigmas sigma(z); every other
 *                   pixel is NaN.  *info[4] of rbs_find_get_stage then counts the seed pixels of the seeding frame.
 *   2 seeds         coarse pixels (u, v) = (j s, i s), s = seed_stride, whose depth d is finite and inside
 *                   [min_depth, max_depth], in row-major order; n of them are thinned to every step-th,
 *                   step = ceil(n / max_seeds).  Seed -> t = d K^-1 (u, v, 1) + depth_offset r, r the unit
 *                   vector along K^-1 (u, v, 1) (coarse K); depth_offset < 0: the mean distance of the mesh's
 *                   vertices from their mean.
 *   3 rotations     a Super-Fibonacci spiral of n_rotations unit quaternions (Alexa, CVPR 2022): for
 *                   i < N, s = i + 1/2, r = sqrt(s / N), R = sqrt(1 - s / N), a = 2 pi s / sqrt(2),
 *                   b = 2 pi s / 1.533751168755204288118041, q = (x, y, z, w) = (r sin a, r cos a, R sin b,
 *                   R cos b).  Hypothesis h = seed * n_rotations + rotation, generated on the device in binary64.
 *   4 coarse scores every hypothesis at the coarse resolution, `batch` at a time.
 *   4b evidence     opt-in (rbs_find_set_gate; off by default), the silhouette gate.  For every hypothesis h, against the
 *                   coarse frame (the frame step 4 scores on, not the seeding frame): the assess record (rendered, valid,
 *                   support, in_front, behind) and the contour record (rim, valid, flush, in_front, beyond) of its pose, by
 *                   exactly the definitions of rbs_assess_poses / rbs_contour_poses for a one-body model: the render culls as
 *                   rbs_render_depth's, tau = sigmas x (model_sigma + sigma_factor x (d x d)) in binary64, the anchor is the
 *                   maximum over the Chebyshev window of `radius`.  The verdicts are taken on the device with the binary64
 *                   comparisons of rbs_assess_verdict and rbs_contour_verdict, and the class c(h) is 0 when they are
 *                   RBS_ASSESS_SUPPORTED and RBS_CONTOUR_PRESENT (the pose is CONFIRMED), else 1.  With the gate on:
 *                   step 5's candidates are the n_candidates first hypotheses in the order (c ascending, score descending,
 *                   h ascending), NaN never -- the chunked top-k run twice, over class 0 with every other score NaN and then
 *                   over class 1 to fill up, which is exact -- and the suppression, unchanged, runs in that order.  In step 7
 *                   the sorted survivors get the same evidence at the sensor's resolution against the frame the find was
 *                   given (in a scene find: the residual frame), the output order is (c ascending, score descending, survivor
 *                   index ascending) with the NaN scores last in survivor order as before, and with require_confirmed set
 *                   found = 1 only when pose 0 has c = 0 and its score >= min_score; with it clear, found keeps its meaning
 *                   and is applied to pose 0 of the new order.
 *   5 selection     the n_candidates best in the order (score descending, hypothesis ascending), NaN never;
 *                   then a greedy non-maximum suppression in that order: a candidate is dropped when a kept one
 *                   has |t - t'|^2 <= nms_translation^2 AND trace(R^T R') >= 1 + 2 cos(nms_angle); at most
 *                   n_survivors are kept.
 *   6 refinement    `rounds` rounds at the sensor's resolution; survivor k has `children` children per round r:
 *                   child 0 is the survivor, child j > 0 is R = R(sa_r n) R_k, t = t_k + st_r n' with
 *                   st_r = sigma_translation decay^r, sa_r = sigma_angle decay^r, R(v) the rotation by the
 *                   vector v, and (n, n') six standard normals: Box-Muller pairs p = 0, 1, 2 of Philox4x32-10
 *                   (key = seed, counter = (j << 2 | p, round << 32 | k)), u1 = 1 - u01(x, y), u2 = u01(z, w),
 *                   n_2p = sqrt(-2 log u1) cos(2 pi u2), n_2p+1 = ... sin(...).  A survivor keeps its best child,
 *                   ties to the lowest j, NaN never beats a number, so its score never goes down.  A survivor whose
 *                   children ALL score NaN (child 0, itself, included) stays as it is, with a NaN score.  The survivors
 *                   are then sorted in step 5's order (by survivor index on ties); none is dropped here: those with a
 *                   NaN score come last, in survivor order, so poses [i] may carry scores [i] = NaN at the end, and
 *                   found is 0 when even the best score is NaN.
 *   6b adaptive     opt-in (rbs_find_set_refinement; off by default), in place of step 6's fixed schedule.  Everything is
 *      refinement   binary64 in the order written; apart from step 6's normals and R(v) the only operations are + - * / and
 *                   sqrt.  Survivor k carries a symmetric 6 x 6 covariance C_k over (rotation vector (3), translation (3)),
 *                   at the start diag(sa^2, sa^2, sa^2, st^2, st^2, st^2), sa = sigma_angle, st = sigma_translation; `decay`
 *                   is not read.  Round r: L_k is the lower Cholesky factor of C_k by rows -- for i = 0..5, j = 0..i:
 *                   s = C_ij, then s = s - L_ik L_jk for k = 0..j-1 ascending; L_ii = sqrt(s), L_ij = s / L_jj -- and when a
 *                   pivot s is not > 0 or not finite, L_k := diag(sqrt(max(C_ii, jitter))), max(x, y) = x > y ? x : y.
 *                   Child 0 is the survivor; child j > 0 has d = L_k n, d_a = L_a0 n_0 + L_a1 n_1 + ... + L_aa n_a summed in
 *                   that order, n step 6's six normals from the same Philox counters, and R = R(d_0..2) R_k,
 *                   t = t_k + d_3..5.  Scoring and keeping the best child are exactly step 6's: a survivor's score never
 *                   goes down.  Then the update: the elite is the `elite` best children of the round in step 5's order
 *                   (score descending, j ascending, NaN never); fewer children with a number: those m; m = 0: C_k stays.
 *                   M_ab = (sum of d_a d_b over the elite, in elite order, from 0; child 0 has d = 0) / m, and
 *                   C_ab <- shrink ((1 - mix) C_ab + mix M_ab), + jitter where a = b.  Steps 5 and 7 and the final sort are
 *                   unchanged.  The covariances never leave the device between rounds.
 *   7 output        the k <= n_survivors best poses [k][12] (R row-major | t, the sensor's mesh frame) and their
 *                   scores; found = (best score >= min_score).  A frame without a valid seed: RBS_OK, found = 0,
 *                   *n_out = 0.
 *
 * Memory: per finder about the frame at two resolutions with their per-pixel terms, the mesh, and `batch` poses
 * and scores (two scoring handles whose occlusion state is ONE plane each); the sensor's max_particles does not
 * limit it.  Limits: one object and a single-device handle (RBS_ERR_UNSUPPORTED otherwise); bad parameters:
 * RBS_ERR_INVALID_ARGUMENT.
 *
 * A find does not touch the sensor's state: observation, clock, occlusion planes, windows and any tracker over it
 * are left as they were, so a tracker can re-detect mid-sequence.  With frame == NULL the find reads the sensor's
 * current observation as rbs_get_observation does: it WAITS for the work queued on the sensor, a frame a tracker
 * has in flight (rbs_tracker_submit / rbs_gauss_submit) included, and leaves that frame's result unchanged.  With
 * a frame given it reads nothing of the sensor.  A finder is driven by one thread at a time and must be destroyed
 * before its sensor. */
typedef struct rbs_find rbs_find;

typedef struct rbs_find_params {
    int32_t coarse_downsampling;   /* f: 0 = the library's choice (above); else 1, 2 or 4                          */
    int32_t seed_stride;           /* 4                                                                             */
    double min_depth, max_depth;   /* 0.2, 3.0 (metres)                                                             */
    double depth_offset;           /* -1: mean vertex distance from the mesh's centre                               */
    int32_t max_seeds;             /* 1 024                                                                         */
    int32_t n_rotations;           /* 1 024                                                                         */
    int32_t n_candidates;          /* 512 (<= 1 024)                                                                */
    double nms_translation;        /* 0.02 (metres)                                                                 */
    double nms_angle;              /* 30 degrees, in radians                                                        */
    int32_t n_survivors;           /* 32 (<= 64, <= n_candidates)                                                   */
    int32_t rounds;                /* 8 (0 .. 64)                                                                   */
    int32_t children;              /* 64 (>= 1)                                                                     */
    double sigma_translation;      /* 0.01 (metres)                                                                 */
    double sigma_angle;            /* 10 degrees, in radians                                                        */
    double decay;                  /* 0.6, in (0, 1]                                                                */
    int32_t batch;                 /* 65 536 hypotheses scored per launch                                           */
    uint64_t seed;                 /* Philox key of the refinement                                                  */
    double min_score;              /* -inf: a find reports the best pose whatever its score                         */
} rbs_find_params;

/* The defaults above, stated once. */
void rbs_find_default_params(rbs_find_params* p);
/* controller:143-167 -- the finder over the sensor's mesh, camera, parameters and device. */
int32_t rbs_find_create(rbs_handle* sensor, const rbs_find_params* p, rbs_find** out);
void rbs_find_destroy(rbs_find* f);
/* controller:143-167 -- one find.  frame: rows*cols floats at the sensor's resolution (NULL: the sensor's current
 * observation); k: room for k poses; poses [k][12] and scores [k] (either may be NULL); *n_out := min(k, survivors);
 * *found := best score >= min_score (0 when there is no pose). */
int32_t rbs_find_run(rbs_find* f, const float* frame, int32_t k, double* poses, double* scores, int32_t* n_out,
                     int32_t* found);
/* controller:143-167 -- inspection of the last find, for the tests: one stage's exact outputs.  Stage
 *   RBS_FIND_SEEDS       poses [n][4] = (u, v, depth, coarse pixel index); scores unused; indices = seed number
 *   RBS_FIND_COARSE      every hypothesis: poses [n][12], coarse scores, indices = h
 *   RBS_FIND_CANDIDATES  the selection's order: poses, coarse scores, hypothesis indices
 *   RBS_FIND_SURVIVORS   after the suppression, in that order: poses, coarse scores, hypothesis indices
 *   RBS_FIND_CHILDREN    round `round`: poses [n_survivors][children][12], full-resolution scores, k * children + j
 *   RBS_FIND_RESULT      the sorted survivors: poses, full-resolution scores, survivor index k
 * Any pointer may be NULL; *n := the stage's count (call with NULL buffers to size them).  Before the first find
 * or for a bad stage / round: RBS_ERR_INVALID_ARGUMENT.  Also *info (may be NULL) [6] := coarse rows, cols,
 * f, hypotheses, valid seed pixels before thinning, depth_offset. */
enum { RBS_FIND_SEEDS = 0, RBS_FIND_COARSE = 1, RBS_FIND_CANDIDATES = 2, RBS_FIND_SURVIVORS = 3, RBS_FIND_CHILDREN = 4,
       RBS_FIND_RESULT = 5 };
int32_t rbs_find_get_stage(rbs_find* f, int32_t stage, int32_t round, double* poses, double* scores, int64_t* indices,
                           int64_t* n, double* info);
/* Device time of the last find's stages in ms (HIP events): [0] frame + seeds (step 1b included), [1] coarse scoring, [2] selection
 * (top-k + suppression), [3] refinement (step 6 or 6b), [4] the whole find. */
int32_t rbs_find_stage_ms(rbs_find* f, float* out5);
/* Step 1b, the foreground.  Memory: one coarse frame and plane_trials records of 36 bytes, allocated when the stage is
 * first switched on. */
typedef struct rbs_find_foreground {
    int32_t enabled;               /* 0: the stage is off (a new finder)                                            */
    int32_t plane_trials;          /* 256 (1 .. 4 096)                                                              */
    double ransac_sigmas;          /* 2: a trial's inliers lie within this many sigma(z) of its plane               */
    double mask_sigmas;            /* 5: a seed pixel stands more than this many sigma(z) in front of the plane     */
    double min_inlier_fraction;    /* 0.2 of the valid coarse pixels, in [0, 1]                                     */
} rbs_find_foreground;
/* The defaults above with enabled = 1, stated once. */
void rbs_find_default_foreground(rbs_find_foreground* g);
/* The setting of the finds from the next rbs_find_run on.  NULL or enabled == 0: the stage is off, and a find is bit for
 * bit that of a finder never configured.  Bad values: RBS_ERR_INVALID_ARGUMENT, and the previous setting stays. */
int32_t rbs_find_set_foreground(rbs_find* f, const rbs_find_foreground* g);
/* The last find's plane: out [8] := accepted (0 / 1), a, b, c, count, valid coarse pixels, trial, valid coarse pixels
 * masked.  The stage off: all 0.  No trial with a plane: count -1, trial 0, a = b = c = 0. */
int32_t rbs_find_get_plane(rbs_find* f, double* out8);
/* The last find's seeding frame (the stage off: the coarse frame): *n := coarse rows * cols; out (may be NULL) [*n]. */
int32_t rbs_find_get_seed_frame(rbs_find* f, float* out, int64_t* n);
/* Step 6b, the adaptive refinement.  Memory, allocated when the stage is first switched on: per survivor 36 doubles for
 * each of the rounds + 1 covariances kept for rbs_find_get_covariance and 36 for the current factor, and 6 doubles per child
 * and round for the perturbations d. */
typedef struct rbs_find_refinement {
    int32_t enabled;               /* 0: the stage is off (a new finder)                                            */
    int32_t elite;                 /* 8 (1 .. 64, <= children)                                                      */
    double mix;                    /* 0.5, in [0, 1]: the weight of the elite's second moment                       */
    double shrink;                 /* 1, in (0, 1]                                                                  */
    double jitter;                 /* 1e-10 (>= 0, finite): added to the diagonal after every update                */
} rbs_find_refinement;
/* The defaults above with enabled = 1, stated once. */
void rbs_find_default_refinement(rbs_find_refinement* g);
/* The setting of the finds from the next rbs_find_run on.  NULL or enabled == 0: the stage is off, and a find is bit for
 * bit that of a finder never configured.  Bad values: RBS_ERR_INVALID_ARGUMENT, and the previous setting stays. */
int32_t rbs_find_set_refinement(rbs_find* f, const rbs_find_refinement* g);
/* The last find's covariances entering round `round` (0 .. rounds; round == rounds: the final ones): *n := survivors,
 * cov (may be NULL) [*n][36] row-major.  The last find ran without the stage: RBS_ERR_INVALID_ARGUMENT. */
int32_t rbs_find_get_covariance(rbs_find* f, int32_t round, double* cov, int64_t* n);
/* The perturbations d of round `round`'s children (0 .. rounds - 1), for the tests: *n := survivors * children,
 * d (may be NULL) [*n][6], in RBS_FIND_CHILDREN's order. */
int32_t rbs_find_get_perturbations(rbs_find* f, int32_t round, double* d, int64_t* n);
/* Step 4b, the silhouette gate, and what it changes in steps 5 and 7.  The fields are rbs_assess_params' and
 * rbs_contour_params', with the same limits.  Memory, allocated when the stage is first switched on: 44 bytes per hypothesis
 * (max_seeds x n_rotations of them: ten int32 counts and the class, written batch by batch and kept for
 * rbs_find_get_evidence), 8 bytes per hypothesis for the gated order's masked scores, and 88 per survivor. */
typedef struct rbs_find_gate {
    int32_t enabled;               /* 0: the stage is off (a new finder)                                            */
    int32_t require_confirmed;     /* 0; 1: found also needs pose 0 to be confirmed                                 */
    int32_t radius;                /* 2 (1 .. 8): rbs_contour_params.radius                                         */
    int32_t min_rim_pixels;        /* 16                                                                            */
    int32_t min_pixels;            /* 16: rbs_assess_params.min_pixels                                              */
    double sigmas;                 /* 3                                                                             */
    double min_support_fraction;   /* 0.5                                                                           */
    double min_visible_fraction;   /* 0.25                                                                          */
    double min_valid_fraction;     /* 0.5                                                                           */
    double min_contour_fraction;   /* 0.3                                                                           */
    double min_flush_fraction;     /* 0.5 (not read by the class; checked as rbs_contour_params')                   */
} rbs_find_gate;
/* The two rules' defaults with enabled = 1 and require_confirmed = 0, stated once. */
void rbs_find_default_gate(rbs_find_gate* g);
/* The setting of the finds from the next rbs_find_run on.  NULL or enabled == 0: the stage is off, and a find is bit for
 * bit that of a finder never configured, launch for launch.  Bad values: RBS_ERR_INVALID_ARGUMENT, and the previous setting
 * stays. */
int32_t rbs_find_set_gate(rbs_find* f, const rbs_find_gate* g);
/* The last find's evidence, each in that stage's order: RBS_FIND_COARSE (every hypothesis), RBS_FIND_CANDIDATES and
 * RBS_FIND_SURVIVORS (step 4b's records of those hypotheses) and RBS_FIND_RESULT (step 7's records).  *n := the stage's
 * count; records (may be NULL) [*n][10] := rendered, valid, support, in_front, behind, rim, valid, flush, in_front, beyond;
 * classes (may be NULL) [*n].  The last find ran without the gate, or another stage: RBS_ERR_INVALID_ARGUMENT. */
int32_t rbs_find_get_evidence(rbs_find* f, int32_t stage, int32_t* records, int32_t* classes, int64_t* n);
/* Device time of the last find's evidence kernel in ms: step 4b's launches (they run behind the scoring calls, inside
 * rbs_find_stage_ms [1]) and step 7's (inside [3]). */
int32_t rbs_find_gate_ms(rbs_find* f, float* out2);
/* Message of the last error on this finder. Never NULL. */
const char* rbs_find_last_error(const rbs_find* f);

/* ---------------------------------------------------------------------------------------------------------
 * The scene finder: every body of a model of several from one depth frame (rbsensor_find_scene.hip; DESIGN.md
 * Appendix K).  An object beside rbs_find, which keeps its one-object limit.  It places the bodies named in a `search`
 * mask of a sensor of B bodies (1 <= B <= 16), given the poses of the others: greedily, body by body, each on a RESIDUAL
 * FRAME from which what the bodies placed so far explain is taken out, and at the end all together under the B-body
 * likelihood.  Everything below is binary64 with + - x / and comparisons and the finder's own steps, in the order written;
 * tests/scene_find_twin.py restates it in numpy and takes every decision bit for bit.
 *   S1 order     e_b = the mean distance of part b's vertices from their mean (rbs_find_create's depth_offset default, in
 *                that order of operations).  The searched bodies are taken by e_b descending, ties to the lower b.
 *   S2 residual  for the body about to be searched.  PLACED bodies are the given ones (not in `search`) and every searched
 *                body already handled whose find returned a pose with `found` set.  d_c, for the placed bodies c, are the
 *                assess rule's planes (the body rendered alone, +inf where it covers nothing); the owner of a pixel is the
 *                nearest placed body, ties to the lowest; an owned pixel j with a finite reading y_j is SUPPORT by the
 *                assess rule's test: d = d_owner(j), r = (double)y_j - (double)d,
 *                tau = explain_sigmas x (model_sigma + sigma_factor x (d x d)), neither r < -tau nor r > tau.
 *                Pixel i is EXPLAINED when (a) it is support, or (b) y_i is finite and some support pixel j of the
 *                Chebyshev window |x_i - x_j| <= explain_radius, |y_i - y_j| <= explain_radius (clipped to the image) has
 *                neither r < -tau nor r > tau with r = (double)y_i - (double)d(j) and tau from d(j).  (b) is an OR over j:
 *                it does not depend on an order; explain_radius = 0 leaves (a).  residual(i) is the float quiet NaN
 *                0x7FC00000 where i is explained and frame(i) bit for bit elsewhere, the frame's own NaNs included.  No
 *                placed body: the residual is the frame.
 *   S3 a body    rbs_find_run's steps 1-7 (with 1b / 6b as set on the scene finder) with the scene finder's
 *                rbs_find_params, the same seed for every body, for the one-body model made of part b -- every other
 *                rbs_config field the sensor's -- on the residual frame, for seeding and for scoring at both resolutions.
 *                The likelihood skips a NaN reading: a hypothesis laid on an explained blob scores about 0, one on the
 *                body's own blob its full support.  The body's pose is the best survivor, found_b is rbs_find_run's
 *                `found`.  A body without a pose or without `found` is not placed.
 *   S4 polish    only when every body of the model has a pose (else it is skipped and the joint score is NaN).  X is the
 *                B poses; the ns searched bodies are polished in S1's order.  Round r = 0 .. polish_sweeps x ns - 1 moves
 *                body c = order[r mod ns] in sweep w = r div ns with st = polish_sigma_translation x polish_decay^w,
 *                sa = polish_sigma_angle x polish_decay^w (repeated multiplication, as step 6).  Child 0 is X; child j > 0
 *                is X with body c's (R, t) replaced by step 6's perturbation R(sa n) R, t + st n', the six normals step 6's
 *                Box-Muller pairs of Philox4x32-10 with key = seed and counter (j << 2 | p, (0x10000 + r) << 32 | c):
 *                disjoint from step 6 (its round <= 64) and from step 1b (last word 0xFFFFFFFF).  All polish_children
 *                children are scored on the ORIGINAL frame by a B-body scoring handle: rbs_loglikes(update = 0) on a
 *                freshly reset handle of the sensor's configuration at its resolution, one occlusion slot, the finder's
 *                fixed tile split.  X becomes the best child, ties to the lowest j, NaN never beats a number: the joint
 *                score never goes down.  The joint score is the final X's; polish_sweeps = 0: X is scored once.
 *   output       poses [B][12] (given bodies bit for bit; a searched body without a pose: NaN), per-body scores [B] (S3's
 *                residual-frame score; NaN for given bodies and bodies without a pose), the found mask, the joint score.
 *
 * explain_sigmas = 3 is the assessor's reading of the sensor's own noise model.  explain_radius and the four polish
 * figures are starting values that nobody has measured against data (policy, like Appendix J's): DESIGN.md Appendix K.
 *
 * A scene find does not touch the sensor's state, and frame == NULL reads the sensor's observation as rbs_find_run does.
 * It owns one per-part finder per body and the B-body scoring handle (memory: B times a finder's, one frame per body for
 * the residuals, B planes).  Limits: single-device handles (RBS_ERR_UNSUPPORTED otherwise).  RBS_ERR_INVALID_ARGUMENT,
 * with the last find's results kept: search_mask 0 or with bits >= B, given_poses == NULL while a body is not searched,
 * a given pose that is not finite, bad parameters.  Driven by one thread at a time; destroyed before its sensor. */
typedef struct rbs_find_scene rbs_find_scene;

typedef struct rbs_find_scene_params {   /* 48 bytes */
    double explain_sigmas;             /* 3 (finite, > 0)                                                            */
    int32_t explain_radius;            /* 2 pixels (0 .. 8) (policy, unmeasured)                                     */
    int32_t polish_sweeps;             /* 2 (0 .. 8) (policy, unmeasured)                                            */
    int32_t polish_children;           /* 64 (1 .. 1 024) (policy, unmeasured)                                       */
    int32_t reserved;                  /* 0                                                                          */
    double polish_sigma_translation;   /* 0.005 (metres; finite, >= 0) (policy, unmeasured)                          */
    double polish_sigma_angle;         /* 5 degrees, in radians (finite, >= 0) (policy, unmeasured)                  */
    double polish_decay;               /* 0.6, in (0, 1] (policy, unmeasured)                                        */
} rbs_find_scene_params;

/* The defaults above, stated once. */
void rbs_find_scene_default_params(rbs_find_scene_params* p);
/* The scene finder over the sensor's model, camera, parameters and device.  find_params: every body's find (S3);
 * scene_params: NULL = the defaults. */
int32_t rbs_find_scene_create(rbs_handle* sensor, const rbs_find_params* find_params, const rbs_find_scene_params* scene_params,
                              rbs_find_scene** out);
void rbs_find_scene_destroy(rbs_find_scene* f);
/* Steps 1b / 6b of every body's find, as rbs_find_set_foreground / rbs_find_set_refinement. */
int32_t rbs_find_scene_set_foreground(rbs_find_scene* f, const rbs_find_foreground* g);
int32_t rbs_find_scene_set_refinement(rbs_find_scene* f, const rbs_find_refinement* g);
/* The gate of every body's find, as rbs_find_set_gate.  With require_confirmed, S3 leaves a body without a confirmed pose
 * unplaced: its bit is clear in found_mask and the bodies after it do not explain its pixels away. */
int32_t rbs_find_scene_set_gate(rbs_find_scene* f, const rbs_find_gate* g);
/* One scene find.  frame: rows*cols floats (NULL: the sensor's current observation); search_mask: bit b = body b is
 * searched; given_poses [B][12] (read for the bodies not searched; may be NULL when all are searched); out_poses [B][12],
 * out_scores [B] (either may be NULL); *found_mask: bit b = searched body b has a pose with `found`; *joint_score. */
int32_t rbs_find_scene_run(rbs_find_scene* f, const float* frame, uint32_t search_mask, const double* given_poses,
                           double* out_poses, double* out_scores, uint32_t* found_mask, double* joint_score);
/* Inspection of the last scene find, for the tests.  get_order: order [*n] := the searched bodies in S1's order, e [B]
 * (may be NULL) := every body's e_b.  get_residual: out [rows*cols] := the residual frame searched body `body` was found on.
 * body_finder: body b's finder, borrowed (NULL for a bad b): rbs_find_get_stage, _get_plane, _get_seed_frame,
 * _get_covariance, _get_perturbations and _stage_ms read that body's last find; it must not be run or destroyed.
 * get_polish: round `round`'s children poses [*n][B][12] and joint scores [*n] (either may be NULL), *best := the child
 * taken; polish_sweeps = 0: round 0 is X alone, *n = 1.  A polish that was skipped, a bad round or body, no scene find
 * yet: RBS_ERR_INVALID_ARGUMENT. */
int32_t rbs_find_scene_get_order(rbs_find_scene* f, int32_t* order, int32_t* n, double* e);
int32_t rbs_find_scene_get_residual(rbs_find_scene* f, int32_t body, float* out);
rbs_find* rbs_find_scene_body_finder(rbs_find_scene* f, int32_t body);
int32_t rbs_find_scene_get_polish(rbs_find_scene* f, int32_t round, double* poses, double* scores, int32_t* n, int32_t* best);
/* Time of the last scene find in ms: per_body [B] (may be NULL) := each searched body's whole find (its device time, 0 for
 * given bodies); out4 := the render kernel and the residual kernel (device time, summed over the searched bodies), the
 * polish (device time), the whole scene find (host wall time, uploads and synchronisations included). */
int32_t rbs_find_scene_stage_ms(rbs_find_scene* f, float* per_body, float* out4);
/* Message of the last error on this scene finder. Never NULL. */
const char* rbs_find_scene_last_error(const rbs_find_scene* f);

/* ---------------------------------------------------------------------------------------------------------
 * Poses judged against one depth frame (rbsensor_assess.hip).
 *
 * The reference leaves this judgement to a person: its controller shows the found pose in rviz and waits for a click
 * between FindObject and RunObjectTracker (object_tracker_controller_service_node.cpp:180-195), and nothing tells a
 * tracker that it has lost its object.  rbs_assess_poses counts, per pose and body, the pixels where the frame agrees
 * with the rendered body, and names a verdict.  Everything below is binary64 with + - x and comparisons and integer
 * counts: the same inputs give the same records on every run, and a numpy restatement takes every decision bit for bit.
 *
 * A call takes n absolute poses [n][n_objects][12] (R row-major | t, as for rbs_render_depth) and one frame.  For each pose:
 *   planes    d_b(i) is the depth of body b rendered alone (the rasterizer of rbs_render_depth with that body only,
 *             culled alike); uncovered pixels are +inf.  min over b of d_b equals rbs_render_depth of the pose bit for bit.
 *   owner     body b owns pixel i when d_b(i) is finite, d_b(i) < d_c(i) for every c < b and d_b(i) <= d_c(i) for every
 *             c > b: the nearest body, ties to the lowest.
 *   class     of an owned pixel, with y the frame's float, d = d_b(i), r = (double)y - (double)d and
 *             tau = sigmas x (model_sigma + sigma_factor x (d x d)) from the sensor's rbs_config (the finder's step 1b
 *             sigma(z)):  y not finite: no reading;  r < -tau: in_front;  r > tau: behind (the sensor sees through the
 *             place where the body should be);  otherwise: support.
 *   record    per (pose, body): rendered = owned pixels, valid = those with a finite y, support, in_front, behind.
 *   verdict   with u = support + behind:
 *               1. rendered < min_pixels                                     RBS_ASSESS_OUT_OF_VIEW
 *               2. (double)u < min_visible_fraction x (double)rendered        RBS_ASSESS_OCCLUDED (undecided)
 *               3. (double)support >= min_support_fraction x (double)u        RBS_ASSESS_SUPPORTED
 *               4. otherwise                                                  RBS_ASSESS_LOST
 *
 * The blind spot: something that stands NEARER than the pose says looks the same whether it is an occluder or the object
 * itself.  A pose pushed 2 cm back from the truth reads in_front on most pixels and hence OCCLUDED, not LOST; `behind` is
 * the decisive evidence, and only a pose that leaves the sensor looking through the body is called LOST.
 *
 * A call does not touch the sensor's state: poses staged by other calls, rbs_render_depth's image, the observation, the
 * clock, the occlusion planes and their windows are left as they were.  It runs on the sensor's stream into buffers of
 * its own (n x n_objects planes of rows x cols floats, allocated by the first call, grown when a later call needs more,
 * freed by rbs_destroy) and ends with one copy of n x n_objects records and one synchronisation.  With frame == NULL it
 * reads the sensor's current observation as rbs_get_observation does: it WAITS for the work queued on the sensor.  With
 * a frame given it reads nothing of the sensor.  Limits: n >= 1, n x n_objects <= 64, every pose entry finite
 * (checked on the host before any launch), single-device handles (RBS_ERR_UNSUPPORTED otherwise). */
enum { RBS_ASSESS_OUT_OF_VIEW = 0, RBS_ASSESS_OCCLUDED = 1, RBS_ASSESS_SUPPORTED = 2, RBS_ASSESS_LOST = 3 };

typedef struct rbs_assess_params {
    double sigmas;                 /* 3: a correct pixel lies within 3 sigma(z) of the sensor's own noise model with
                                      probability 0.997; finite, > 0                                                */
    double min_support_fraction;   /* 0.5 of u, in [0, 1] (policy: DESIGN.md Appendix J)                            */
    double min_visible_fraction;   /* 0.25 of rendered, in [0, 1] (policy)                                          */
    int32_t min_pixels;            /* 16 (>= 1) (policy)                                                            */
    int32_t reserved;              /* 0                                                                             */
} rbs_assess_params;

typedef struct rbs_assess_body {   /* 32 bytes */
    int32_t rendered, valid, support, in_front, behind;
    int32_t verdict;               /* RBS_ASSESS_*                                                                  */
    int32_t reserved[2];           /* 0                                                                             */
} rbs_assess_body;

/* The defaults above, stated once. */
void rbs_assess_default_params(rbs_assess_params* p);
/* controller:180-195 -- n poses judged against one frame.  params: NULL = the defaults; frame: rows*cols floats (NULL:
 * the sensor's current observation); poses [n][n_objects][12]; out [n][n_objects]. */
int32_t rbs_assess_poses(rbs_handle* h, const rbs_assess_params* params, const float* frame, const double* poses, int32_t n,
                         rbs_assess_body* out);
/* The verdict of one record's counts (rule above): host only, no device.  params: NULL = the defaults. */
int32_t rbs_assess_verdict(const rbs_assess_params* params, const rbs_assess_body* body, int32_t* verdict);
/* Inspection, for the tests: d_b of pose k of the last call, rows*cols floats, +inf outside the body's rectangle.  Before
 * the first call or for a bad k or b: RBS_ERR_INVALID_ARGUMENT. */
int32_t rbs_assess_get_plane(rbs_handle* h, int32_t k, int32_t b, float* out);
/* Device time of the last call's kernels in ms (HIP events): [0] render, [1] count. */
int32_t rbs_assess_kernel_ms(rbs_handle* h, float* out2);

/* ---------------------------------------------------------------------------------------------------------
 * The silhouette of a pose judged against the frame (rbsensor_contour.hip; DESIGN.md Appendix J, "The contour rule").
 *
 * The assess rule above sees depth agreement INSIDE the rendered body and nothing else: a pose whose visible face lies in
 * a surface of the scene (a wall, a table) reads RBS_ASSESS_SUPPORTED.  The contour rule is an opt-in second rule beside
 * it.  It looks at the pixels just OUTSIDE the rendered body: around an object the scene falls away behind the
 * silhouette; around a pose that lies in a wall the wall goes on.  Inputs per pose are the planes d_b of the assess rule
 * and the frame y; owner(i) and depth(i) = d_owner(i)(i) are those of the assess rule; a pixel is covered when it has an
 * owner.  Everything is binary64 + - x, comparisons, a float maximum and integer counts, as above.
 *   rim       an uncovered pixel i inside the image (no body of the pose owns it) is a rim pixel of body b when some
 *             pixel j owned by b lies in the Chebyshev window |x_i - x_j| <= radius, |y_i - y_j| <= radius, clipped to
 *             the image.  A pixel may be a rim pixel of several bodies and counts in each one's record.
 *   anchor    a_b(i) = the maximum of depth(j) over those j, as a float: the farthest point of the body's surface beside
 *             the pixel (the conservative choice; a maximum does not depend on order).
 *   class     of a rim pixel with a finite y, with g = (double)y - (double)a and
 *             tau = sigmas x (model_sigma + sigma_factor x (a x a)), sigmas the assess parameter:
 *             g < -tau: in_front (an occluder, or nothing to learn);  g > tau: beyond (the scene falls away behind the
 *             silhouette);  otherwise: flush (the surface the pose lies in continues past its silhouette).
 *   record    per (pose, body): rim, valid (finite y), flush, in_front, beyond; valid = flush + in_front + beyond.
 *   verdict   on the host from the counts, in this order:
 *               1. rim < min_rim_pixels                                                      RBS_CONTOUR_NO_RIM
 *               2. valid == 0 or (double)valid < min_valid_fraction x (double)rim            RBS_CONTOUR_UNDECIDED
 *               3. (double)beyond >= min_contour_fraction x (double)valid                    RBS_CONTOUR_PRESENT
 *               4. (double)flush >= min_flush_fraction x (double)valid                       RBS_CONTOUR_ABSENT
 *               5. otherwise                                                                 RBS_CONTOUR_UNDECIDED
 *
 * rbs_contour_poses is rbs_assess_poses plus one more kernel on the same planes: one call, one frame upload, one
 * synchronisation.  out_assess (may be NULL) equals rbs_assess_poses' output for the same arguments field for field;
 * limits, frame == NULL and "touches nothing of the sensor" are rbs_assess_poses'; rbs_assess_get_plane works after it. */
enum { RBS_CONTOUR_NO_RIM = 0, RBS_CONTOUR_UNDECIDED = 1, RBS_CONTOUR_PRESENT = 2, RBS_CONTOUR_ABSENT = 3 };

typedef struct rbs_contour_params {   /* 32 bytes */
    int32_t radius;                /* 2 pixels (1 .. 8): half the window's side                                     */
    int32_t min_rim_pixels;        /* 16 (>= 1) (policy: DESIGN.md Appendix J)                                      */
    double min_valid_fraction;     /* 0.5 of rim, in [0, 1] (policy)                                                */
    double min_contour_fraction;   /* 0.3 of valid, in [0, 1] (policy)                                              */
    double min_flush_fraction;     /* 0.5 of valid, in [0, 1] (policy)                                              */
} rbs_contour_params;

typedef struct rbs_contour_body {   /* 32 bytes */
    int32_t rim, valid, flush, in_front, beyond;
    int32_t verdict;               /* RBS_CONTOUR_*                                                                 */
    int32_t reserved[2];           /* 0                                                                             */
} rbs_contour_body;

/* The defaults above, stated once. */
void rbs_contour_default_params(rbs_contour_params* p);
/* n poses judged by both rules against one frame.  params, contour: NULL = the defaults; frame, poses, n: as for
 * rbs_assess_poses; out_assess [n][n_objects] or NULL; out_contour [n][n_objects].  Bad parameters are refused before
 * any launch. */
int32_t rbs_contour_poses(rbs_handle* h, const rbs_assess_params* params, const rbs_contour_params* contour, const float* frame,
                          const double* poses, int32_t n, rbs_assess_body* out_assess, rbs_contour_body* out_contour);
/* The verdict of one record's counts (rule above): host only, no device.  params: NULL = the defaults. */
int32_t rbs_contour_verdict(const rbs_contour_params* params, const rbs_contour_body* body, int32_t* verdict);
/* Device time of the last rbs_contour_poses' kernels in ms (HIP events): [0] render, [1] count, [2] contour.  When the
 * handle's last assessment was not an rbs_contour_poses: RBS_ERR_INVALID_ARGUMENT. */
int32_t rbs_contour_kernel_ms(rbs_handle* h, float* out3);

/* ---------------------------------------------------------------------------------------------------------
 * Occlusion map (csrc/rbsensor_occmap.hip): what a particle population believes is occluded -- the
 * weighted mean of the occlusion planes its members point at, reduced on the device from the planes as they are stored.
 * It is the quantity the assessor's blind spot (above, "The blind spot") asks for: a single frame cannot tell an occluder
 * from the object, the filter's belief, integrated over the frames, can.
 *
 * The rule.  Population: n members; member i has an occlusion slot idx_i and a log-weight lw_i.  At least one lw_i is
 * finite; lw_i = -inf contributes nothing.  With m = max lw:
 *   e_i = exp(lw_i - m)   (the device library's exp, as in the posterior report),    S = sum e_i,
 *   W_s = sum over { i : idx_i = s } of e_i.
 * Value of a slot at a pixel: v_s(p) is exactly the float rbs_get_occlusion(h, s, .) hands out at p, in every layout --
 *   inside the slot's window the stored float (slabs: addressed through the stored region); occlusion_mode REFERENCE: the
 *   effective value exact_prior(value, age) as of the slot's epoch, an age beyond age_max being the background;
 *   outside the window the scalar background, or the shared trail's plane pixel while the trail is active (REFERENCE: its
 *   effective value);  dense planes: the stored float.
 * Map:  M(p) = (float)((sum over s of W_s (double)v_s(p)) / S) -- the sum in binary64, one rounding to float; no contraction
 * into fused operations.  Every sum (W_s, S, the per-pixel sum) is taken in an order fixed by n, idx and the windows alone:
 * W_s over ascending i; S per thread t of 1 024 over i = t, t + 1 024, ..., then a fixed tree; per pixel the slots with
 * W_s > 0 in ascending s, cut into four contiguous parts that are summed one by one and folded in part order.  No
 * floating-point atomics: two runs give the same bits, and so do a tracker frame by frame and with look-ahead.  Outside every
 * live window M(p) is the background value bit for bit.
 * Nothing of the sensor is touched: values, windows, regions, the shared plane, clocks, staged poses, rbs_render_depth's
 * image and the observation stay as they were.  In particular no slot is made dense, as rbs_get_occlusion makes it on float
 * windowed planes: the planes are read in place.
 *
 * rbs_occlusion_mean: host pointers, synchronous.  slots [n] in [0, max_particles), repeats allowed; log_weights [n], NULL =
 * uniform weights; out [rows*cols].  RBS_ERR_INVALID_ARGUMENT: a null pointer, n < 1, a slot out of range, a log-weight that
 * is NaN or +inf, every log-weight -inf.  A handle over several devices or attached to other ranks: RBS_ERR_UNSUPPORTED.  A
 * poisoned handle: its own error.  The call's buffers are allocated at first use, grow only, and are freed by rbs_destroy. */
int32_t rbs_occlusion_mean(rbs_handle* h, const int32_t* slots, const double* log_weights, int32_t n, float* out);
/* Device time of the last rbs_occlusion_mean's kernels, first launch to last (HIP events), in milliseconds.
 * RBS_ERR_INVALID_ARGUMENT before the first map. */
int32_t rbs_occlusion_mean_ms(rbs_handle* h, float* ms);

/* The device tracker's occlusion map (opt-in), on the pattern of the posterior report: with it on, every frame ends with the
 * map of the population rbs_tracker_get returns after that frame (log_weights, indices), its kernels launched last in the
 * frame's chain -- behind the posterior report's when that is on too; the two are independent -- into a pinned buffer per
 * frame in flight.
 * rbs_tracker_set_occlusion_map: enable != 0 switches the map on (allocating its buffers the first time), 0 off.  Off -- the
 * default -- a frame enqueues exactly what it did before the map existed.  Frames in flight: RBS_ERR_INVALID_ARGUMENT; a
 * tracker over several devices: RBS_ERR_UNSUPPORTED.  The filter is not touched: estimates and particles are bit for bit those
 * of a tracker with the map off.
 * rbs_tracker_occlusion_map: the map of the frame most recently handed out by rbs_tracker_result / rbs_tracker_track* (with
 * look-ahead: of frame k after result(k), while k + 1 is in flight).  frame: frames tracked since rbs_tracker_initialize
 * (1, 2, ...); out [rows*cols]; either may be NULL.  RBS_ERR_INVALID_ARGUMENT while the map is off, before the first frame,
 * and after rbs_tracker_initialize until the next result; a poisoned tracker's error comes first.
 * rbs_tracker_occlusion_map_ms: device time of that map's kernels; RBS_ERR_INVALID_ARGUMENT wherever there is no map. */
int32_t rbs_tracker_set_occlusion_map(rbs_tracker* t, int32_t enable);
int32_t rbs_tracker_occlusion_map(rbs_tracker* t, int32_t* frame, float* out);
int32_t rbs_tracker_occlusion_map_ms(rbs_tracker* t, float* ms);

/* A map summarised per body at given poses: which share of each body the map calls occluded.  poses [n][n_objects][12] as
 * for rbs_assess_poses, n x n_objects <= 64; planes and the owner of a pixel are exactly the assessor's (Pose assessment
 * above: the nearest of the bodies' own depth planes, a tie with the lowest body).  Per pixel p owned by body b:
 *   rendered += 1;   occluded += ((double)M(p) > threshold);   sum_q32 += (uint64)((double)M(p) 2^32), truncated.
 * Integer sums: order-free.  The mean occlusion of a body is sum_q32 / 2^32 / rendered.
 * map [rows*cols] host floats, each finite and in [0, 1]; threshold in [0, 1]; out [n][n_objects].  Checked on the host
 * before any launch: RBS_ERR_INVALID_ARGUMENT.  Single-device handles only (RBS_ERR_UNSUPPORTED).  The sensor's state is not
 * touched; the assessor's last-call inspection state (rbs_assess_get_plane) is what an rbs_assess_poses at these poses
 * leaves, except that rbs_assess_kernel_ms keeps the times of the assessor's own last call (zeros when there was none).  On a
 * handle over several devices RBS_ERR_UNSUPPORTED comes before a poisoned handle's error, here and in rbs_occlusion_mean. */
typedef struct rbs_occlusion_body {   /* 32 bytes */
    int32_t rendered;       /* pixels the body owns */
    int32_t occluded;       /* ... of them with M > threshold */
    int64_t sum_q32;        /* sum over them of floor(M 2^32) */
    int32_t reserved[4];    /* 0 */
} rbs_occlusion_body;
int32_t rbs_occlusion_bodies(rbs_handle* h, const float* map, const double* poses, int32_t n, double threshold, rbs_occlusion_body* out);

/* ---------------------------------------------------------------------------------------------------------
 * Object map (csrc/rbsensor_objmap.hip): which pixels a weighted particle population sees the object
 * at, and at what depth -- per pixel and body the probability that the body is what the camera sees there, and the
 * posterior mean and variance of the rendered depth -- reduced on the device without a plane per member; and the
 * segmentation of the staged observation against such a map.
 *
 * Population.  n members; member i has a pose index k_i into poses[m][n_objects][12] (row-major R, then t, as for
 * rbs_assess_poses) and a log-weight lw_i.  e_i, S, m = max lw and the treatment of -inf are exactly the occlusion map's
 * (above), and so is W_k = sum over { i : k_i = k } of e_i in ascending i (the same kernels).  A pose is live when W_k > 0.
 * Planes and owner.  d_{k,b}(p): body b of pose k alone, the depth rbs_assess_get_plane hands out inside the body's
 * rectangle, +inf where there is no surface.  o_k(p), d_k(p): the assessor's owner rule -- the nearest body, a tie with the
 * lowest, -1: none.
 * Outputs (binary64, no contraction into fused operations, every output float rounded once):
 *   c_b(p) = sum_k W_k [o_k(p) = b]     a(p) = c_0(p) + c_1(p) + ...  (ascending b)   = sum_k W_k [o_k(p) >= 0]
 *   s1(p) = sum_k W_k d_k(p)            s2(p) = sum_k W_k (d_k(p) d_k(p))               (over the k with o_k(p) >= 0)
 *   cover[b][p] = (float)(c_b / S)   depth[p] = (float)(s1 / a)   var[p] = (float)max(0, s2 / a - (s1 / a)(s1 / a))
 *   a = 0:  depth[p] = +inf (rbs_render_depth's "no surface"),  var[p] = 0.
 * Order.  U = the union of the live poses' body rectangles, cut from its corner into tiles of 32 x 32 pixels (n_objects <= 4)
 * or 32 x 16 (5 .. 8).  The live poses in ascending k are cut into G contiguous parts, part g = [L g / G, L (g + 1) / G) of
 * the L live poses, with
 *   G = max(1, min(32, ceil(L / 8), floor(C / (tiles(U) tile_px (n_objects + 2)))))
 * C being the doubles of partial sums the handle keeps (below).  Every sum above is taken per part in ascending k and the
 * parts are added in ascending g: the order is fixed by n, the indices and the poses' rectangles alone.  No floating-point
 * atomics: two runs give the same bits, and so do a tracker frame by frame and with look-ahead.  A pixel no live pose covers
 * reads 0, +inf, 0 bit for bit.
 * Nothing of the sensor is written: planes, windows, clocks, staged poses, the observation and the assessor's inspection
 * state stay as they were.
 * Limits.  n_objects <= 8 (more: RBS_ERR_UNSUPPORTED).  Device memory, allocated at first use, grow-only, freed by
 * rbs_destroy: per member 20 bytes, per pose 16 n_objects + 12 + 96 n_objects (its rectangles, list entry, weight and the
 * caller's pose), the maps (n_objects + 2) x 4 bytes per pixel, the segmentation's 20 bytes per pixel, and the partial sums:
 * C = max(one part over the whole frame, min(32 parts over the whole frame, 4 Mi doubles = 32 MiB)), one part over the whole
 * frame being tiles(frame) tile_px (n_objects + 2) doubles -- 7.4 MB at 640 x 480 and one body.  Nothing grows with
 * n x rows x cols.
 *
 * rbs_object_map: host pointers, synchronous.  poses [n_poses][n_objects][12]; members [n] in [0, n_poses), repeats allowed,
 * NULL = the identity (then n must equal n_poses); log_weights [n], NULL = uniform; cover [n_objects][rows*cols], depth and
 * var [rows*cols], each may be NULL.  Refusals, in this order: a null poses pointer, n or n_poses < 1 (or n != n_poses
 * without members): RBS_ERR_INVALID_ARGUMENT; a handle over several devices or attached to other ranks, then
 * n_objects > 8: RBS_ERR_UNSUPPORTED; a pose index out of range, a log-weight that is NaN or +inf, every log-weight -inf, a
 * pose entry that is not finite: RBS_ERR_INVALID_ARGUMENT; a poisoned handle: its own error.
 * rbs_object_map_ms: device time of the last rbs_object_map's kernels, first launch to last (HIP events), in ms.
 * rbs_object_map_info: of the last rbs_object_map: [0] live poses L, [1..4] U (x0, y0, x1, y1), [5] tiles(U), [6] G,
 * [7] tile_px.  Both: RBS_ERR_INVALID_ARGUMENT before the first map, and after an rbs_object_segment with host maps has
 * replaced that map's images on the device. */
int32_t rbs_object_map(rbs_handle* h, const double* poses, int32_t n_poses, const int32_t* members, const double* log_weights, int32_t n,
                       float* cover, float* depth, float* var);
int32_t rbs_object_map_ms(rbs_handle* h, float* ms);
int32_t rbs_object_map_info(rbs_handle* h, int32_t* out8);

/* Segmentation of the staged observation y against a map.  With D = depth[p], tau = sigmas (model_sigma + sigma_factor D D)
 * (the assessor's tau, from the handle's Kinect parameters), all in binary64:
 *   b* = argmax_b cover[b][p], a tie with the lowest b;
 *   label[p] = b*  when  cover[b*][p] >= min_cover  and  y(p) is finite  and  D is finite (there is a surface)  and
 *                        max(0, |y - D| - tau)^2 <= depth_sigmas^2 var[p];         -1 otherwise.
 * No square root is taken: the labels are an exact function of the float maps.  counts[b] = pixels labelled b.  The
 * labelled pixels in ascending pixel index c = 0, 1, ...: pixel[c] = y * cols + x, xyz[c] = (X, Y, Z) in camera
 * coordinates on integer sample coordinates,  Z = y(p),  X = (float)(((double)x - cx) / fx * (double)Z),  Y likewise.
 * An integer scan, no atomics: order and values are exact.
 * cover / depth / var: host maps as rbs_object_map returns them; cover == NULL: the maps of the last rbs_object_map on this
 * handle, still on the device (RBS_ERR_INVALID_ARGUMENT when there are none, or when a call with host maps has replaced
 * them).  labels [rows*cols], counts [n_objects], pixel [capacity], xyz [capacity][3]; labels, counts and n_points may be
 * NULL, pixel and xyz when capacity == 0.  *n_points is always the full count; when it exceeds capacity the first `capacity`
 * points are written, nothing past them, and the call still returns RBS_OK -- compare *n_points with capacity.
 * Refusals, in this order: bad parameters (min_cover outside [0, 1], sigmas not finite and > 0, depth_sigmas not finite
 * and >= 0), capacity < 0 or > 0 without its outputs, cover without depth and var: RBS_ERR_INVALID_ARGUMENT; several devices,
 * n_objects > 8: RBS_ERR_UNSUPPORTED; no observation handed to the handle since rbs_create, cover == NULL without maps on the
 * device: RBS_ERR_INVALID_ARGUMENT; a poisoned handle: its own error. */
typedef struct rbs_object_segment_params {   /* 32 bytes */
    double min_cover;       /* 0.5 */
    double sigmas;          /* rbs_assess_default_params' sigmas */
    double depth_sigmas;    /* 3 */
    double reserved;        /* 0 */
} rbs_object_segment_params;
void rbs_object_segment_default_params(rbs_object_segment_params* p);
int32_t rbs_object_segment(rbs_handle* h, const rbs_object_segment_params* params, const float* cover, const float* depth, const float* var,
                           int32_t* labels, int32_t* counts, int32_t* pixel, float* xyz, int32_t capacity, int32_t* n_points);

/* The device tracker's object map (opt-in), point for point on the pattern of rbs_tracker_set_occlusion_map: with it on,
 * every frame ends with the object map of the population rbs_tracker_get returns after that frame, over the poses
 * rbs_tracker_poses returns, its kernels launched last in the frame's chain -- behind the posterior report's and the
 * occlusion map's when those are on; the three are independent -- into a pinned buffer per frame in flight.
 * rbs_tracker_set_object_map: enable != 0 switches it on (allocating its buffers the first time), 0 off.  Off -- the
 * default -- a frame enqueues exactly what it did before.  Refusals in this order: a tracker over several devices:
 * RBS_ERR_UNSUPPORTED; frames in flight: RBS_ERR_INVALID_ARGUMENT; n_objects > 8: RBS_ERR_UNSUPPORTED.  The filter is not
 * touched: estimates and particles are bit for bit those of a tracker with the map off.
 * rbs_tracker_object_map: the maps of the frame most recently handed out by rbs_tracker_result / rbs_tracker_track*; frame
 * and every output may be NULL.  A poisoned tracker's error first; then RBS_ERR_INVALID_ARGUMENT while the map is off, before
 * the first frame, and after rbs_tracker_initialize until the next result.
 * rbs_tracker_object_map_ms: device time of that map's kernels; RBS_ERR_INVALID_ARGUMENT wherever there is no map.
 * rbs_tracker_poses: out [n][n_objects][12], the absolute pose of every member of the population rbs_tracker_get returns:
 * member i's pose is the one the frame's last sampling block evaluated for its parent.  No snapshot is kept -- the next
 * frame's transition overwrites those rows -- so the call refuses where rbs_tracker_get would hand out another frame's
 * population: RBS_ERR_INVALID_ARGUMENT with frames in flight, and before the first frame; several devices:
 * RBS_ERR_UNSUPPORTED. */
int32_t rbs_tracker_set_object_map(rbs_tracker* t, int32_t enable);
int32_t rbs_tracker_object_map(rbs_tracker* t, int32_t* frame, float* cover, float* depth, float* var);
int32_t rbs_tracker_object_map_ms(rbs_tracker* t, float* ms);
int32_t rbs_tracker_poses(rbs_tracker* t, double* out);

/* ---------------------------------------------------------------------------------------------------------
 * Poses refined against one depth frame (rbsensor_refine.hip, rbs_refine_api.h).
 *
 * Between "a pose that is roughly right" (the finder's, a tracker's mean) and "the pose on the surface the frame shows"
 * stands a local, deterministic step: projective point-to-plane ICP, solved as damped Gauss-Newton.  Everything below is
 * binary64 with + - x / sqrt and comparisons in the order written (no contraction), sums in a fixed order and integer
 * counts; the only library functions are the sin and cos of rbd::rotvec_to_matrix.  A numpy restatement
 * (tests/refine_twin.py) takes every decision bit for bit.
 *
 * A call takes n absolute poses [n][n_objects][12] (R row-major | t, as for rbs_assess_poses), one frame and an iteration
 * count.  One iteration, for pose k (cx, cy, fx, fy: the camera matrix; ms, sf: model_sigma, sigma_factor of rbs_config):
 *   1. planes   d_b(j) of every body b of the pose and its rectangle: the assess rule's planes (body b rendered alone);
 *               owner(j) and its depth: the assess rule's owner.
 *   2. usable   pixel i = (x, y) is usable for body b when 1 <= x <= cols - 2 and 1 <= y <= rows - 2; b owns i and its
 *               four neighbours (x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1); the frame's y_i is finite; and
 *               |e| <= gate_sigmas x sigma with D = (double)d_b(i), e = (double)y_i - D, sigma = ms + sf x (D x D).
 *   3. points   rx(x) = ((double)x - cx) / fx, ry(y) = ((double)y - cy) / fy, the ray rho = (rx, ry, 1); the model point of
 *               pixel j is m(j) = (D_j x rx_j, D_j x ry_j, D_j).  a = m(x + 1, y) - m(x - 1, y), c = m(x, y + 1) - m(x, y - 1),
 *               N = a cross c = (a1 c2 - a2 c1, a2 c0 - a0 c2, a0 c1 - a1 c0).  If (N0 m0 + N1 m1) + N2 m2 > 0 at m = m(i),
 *               N = -N (decided on the un-normalised N: the normal faces the camera; (a cross c) . m equals
 *               D (D_r + D_l) (D_d + D_u) / (fx fy) up to rounding, so on rendered planes the flip is always taken, and as
 *               every term below holds n twice it changes no bit of any sum).  s = sqrt((N0 N0 + N1 N1) + N2 N2);
 *               a pixel with !(s > 0) is skipped; n = N / s, component by component.
 *   4. terms    h = 1 if |e| <= huber_sigmas x sigma, else (huber_sigmas x sigma) / |e|;  w = h / (sigma x sigma);
 *               r = e x ((n0 rx + n1 ry) + n2): n . (p - m(i)) for the observed point p = y_i rho on the same ray;
 *               q = m(i) - t_b;  J = (q cross n ; n) = (q1 n2 - q2 n1, q2 n0 - q0 n2, q0 n1 - q1 n0, n0, n1, n2): rotation first.
 *   5. sums     over the usable pixels of (k, b), 28 of them in this order: the 21 upper entries of H = sum (w J_a) J_b
 *               row by row ((0,0) (0,1) .. (0,5) (1,1) .. (5,5)), g_a = sum (w J_a) r, q = sum (w r) r; and the integer
 *               count.  The rectangle's pixels in row-major order p = 0, 1, .. are dealt to P parts of 256 threads: thread
 *               t of part j adds p = 256 j + t, + 256 P, + 512 P, .. in ascending order; P = min(16, ceil(pixels / 1024)), a
 *               rule of the rectangle alone.  A part's 256 sums fold per wave by the shuffle tree (offsets 32, 16, .. 1),
 *               then over the four waves in ascending order; the parts fold in ascending order.  No floating-point atomics:
 *               the same inputs give the same bits on every run and in every batch.
 *   6. solve    count < min_pixels: RBS_REFINE_TOO_FEW_PIXELS, the body does not move in this iteration and is evaluated
 *               again in the next one (ownership may change as other bodies move).  Otherwise A = H, A_aa = H_aa +
 *               damping x H_aa; lower Cholesky by rows (L_ab = (A_ab - sum_{c<b} L_ac L_bc) / L_bb, the pivot p = A_aa - sum
 *               L_ac L_ac, L_aa = sqrt(p)); a pivot that is not > 0 or not finite: RBS_REFINE_DEGENERATE, the body does not
 *               move and is frozen.  y_a = (g_a - sum_{c<a} L_ac y_c) / L_aa ascending, delta_a = (y_a - sum_{c>a} L_ca
 *               delta_c) / L_aa descending, sums ascending in c; delta = (omega, v).  |omega| = sqrt((o0 o0 + o1 o1) + o2 o2)
 *               > max_rotation: omega = omega x (max_rotation / |omega|); v likewise with max_translation.
 *               R <- rbd::rotvec_to_matrix(omega) R (matmul3), t <- t + v.  When the clamped |omega| < eps_rotation and
 *               |v| < eps_translation the update is still applied, and the body is RBS_REFINE_CONVERGED and frozen.  A frozen
 *               body is still rendered, for the owner rule.
 *   7. after `iters` iterations an unfrozen body is RBS_REFINE_MAX_ITERATIONS when its last iteration moved it, and
 *      RBS_REFINE_TOO_FEW_PIXELS when its last iteration had too few pixels.
 * Bodies of one pose are solved independently within an iteration, each from the planes of the poses that entered it.
 *
 * The record per (pose, body): status, the iterations evaluated (a frozen body: up to and including the one that froze
 * it), and count and rms = sqrt(q / count) (0 when count is 0) of the first and of the last evaluated iteration.
 *
 * A call does not touch the sensor's state (as rbs_assess_poses), nor the assessor's planes: it runs on the sensor's
 * stream into buffers of its own (n x n_objects planes, allocated by the first call, grow-only, freed by rbs_destroy).
 * All iterations are enqueued without a host round trip -- a frozen body skips by a device flag -- and the call ends
 * with one copy and one synchronisation.  frame == NULL: the sensor's current observation, with rbs_assess_poses' wait.
 * Limits: n >= 1, n x n_objects <= 64, every pose entry finite, the parameters within their ranges (all checked on the
 * host before any launch), single-device handles (RBS_ERR_UNSUPPORTED otherwise).
 *
 * Every default below is an unmeasured starting value: none was tuned on data (DESIGN.md Appendix Q says what was
 * measured with them). */
enum { RBS_REFINE_MAX_ITERATIONS = 0, RBS_REFINE_CONVERGED = 1, RBS_REFINE_TOO_FEW_PIXELS = 2, RBS_REFINE_DEGENERATE = 3,
       RBS_REFINE_FROZEN = 4 /* history only: the body was frozen before this iteration */ };
#define RBS_REFINE_MAX_ITERS 32

typedef struct rbs_refine_params {   /* 64 bytes */
    double gate_sigmas;       /* 10 (finite, > 0): unmeasured starting value                                        */
    double huber_sigmas;      /* 3 (finite, > 0): unmeasured starting value                                         */
    double damping;           /* 1e-3 (finite, >= 0; 0: plain Gauss-Newton): unmeasured starting value              */
    double max_rotation;      /* 0.2 rad per iteration (finite, > 0): unmeasured starting value                     */
    double max_translation;   /* 0.02 m per iteration (finite, > 0): unmeasured starting value                      */
    double eps_rotation;      /* 1e-3 rad (finite, >= 0): unmeasured starting value                                 */
    double eps_translation;   /* 1e-4 m (finite, >= 0): unmeasured starting value                                   */
    int32_t min_pixels;       /* 16 (>= 1): unmeasured starting value                                               */
    int32_t iters;            /* 10 (1 .. RBS_REFINE_MAX_ITERS): unmeasured starting value                          */
} rbs_refine_params;

typedef struct rbs_refine_body {   /* 32 bytes */
    int32_t status;                /* RBS_REFINE_MAX_ITERATIONS .. RBS_REFINE_DEGENERATE                            */
    int32_t iterations;            /* iterations evaluated                                                          */
    int32_t count_first, count_last;   /* usable pixels of the first / last evaluated iteration                     */
    double rms_first, rms_last;    /* sqrt(q / count) of those (whitened: in sigmas)                                */
} rbs_refine_body;

typedef struct rbs_refine_history {   /* 376 bytes: one iteration of one (pose, body) */
    double pose[12];               /* the pose that entered the iteration                                           */
    double sums[28];               /* H upper (21), g (6), q; zeros for RBS_REFINE_FROZEN                           */
    double delta[6];               /* (omega, v) applied, after the clamp; zeros when the body did not move         */
    int32_t count;
    int32_t status;                /* of this iteration: RBS_REFINE_MAX_ITERATIONS = moved and not converged        */
} rbs_refine_history;

/* The defaults above, stated once. */
void rbs_refine_default_params(rbs_refine_params* p);
/* RBS_OK when rbs_refine_poses would accept the parameters, RBS_ERR_INVALID_ARGUMENT otherwise (NULL: the defaults, RBS_OK):
 * host only, no device. */
int32_t rbs_refine_check_params(const rbs_refine_params* params);
/* n poses refined against one frame.  params: NULL = the defaults; frame: rows*cols floats (NULL: the sensor's current
 * observation); poses_in, poses_out [n][n_objects][12] (may be the same array); records_out [n][n_objects] or NULL. */
int32_t rbs_refine_poses(rbs_handle* h, const rbs_refine_params* params, const float* frame, const double* poses_in, int32_t n,
                         double* poses_out, rbs_refine_body* records_out);
/* Inspection: iteration `iteration` of body b of pose k of the last call.  Before the first call, or for a bad index:
 * RBS_ERR_INVALID_ARGUMENT. */
int32_t rbs_refine_get_history(rbs_handle* h, int32_t k, int32_t b, int32_t iteration, rbs_refine_history* out);
/* Device time of the last call's kernels in ms (HIP events), summed over its iterations: [0] render, [1] accumulate,
 * [2] solve. */
int32_t rbs_refine_kernel_ms(rbs_handle* h, float* out3);

#ifdef __cplusplus
}
#endif
#endif
