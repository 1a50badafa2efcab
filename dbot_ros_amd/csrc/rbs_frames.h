// rbs_frames.h -- frame ingest (rbs_handle::fr): what the kernels read (obs_frame / obs_aux), the double -> float staging
// (convert_f64_f32*), borrowed frames (BorrowedFrameGuard, stage_borrowed), device frames, upload_frame / prefetch_frame, the
// hand-over (frame_begin, frame_ready, hand_over_*), make_current, frame_abandon.
// Not a header to include elsewhere: a section of rbsensor_capi.hip's translation unit, included there once before rbs_call.h.
#if defined(__x86_64__)
#include <immintrin.h>   // (the frame's double -> float staging: AVX2 / AVX-512 where the host has them; other hosts take the scalar loop)
#endif

namespace {

// ----------------------------------------------------------------------------- the frame section (rbs_handle::fr)
// A hand-over: frame_begin, the entry point's own checks, frame_ready, one hand_over_*.  A reader: make_current (or, in
// enqueue_loglikes, its pieces), then obs_frame / obs_aux.
using NextFrame = rbs_handle::NextFrame;

// What the kernels read: the staging image of slot fr.cur (F64: with its model terms), or d_frame / d_aux.
const float* obs_frame(const rbs_handle* h) { return h->fr.cur >= 0 ? h->d_fin[h->fr.cur] : h->d_frame; }
const double* obs_aux(const rbs_handle* h) { return h->fr.cur >= 0 ? h->d_aux_slot[h->fr.cur] : h->d_aux; }
float* staging(const rbs_handle* h) { return h->h_frames[h->fr.stage]; }

// Can borrow: only a handle that stages a frame between the two kernels of the split launch takes one without copying it at
// once (one device, binary64 likelihood, windowed planes).
bool can_borrow(const rbs_handle* h)
{
    return h->shards.empty() && !h->group && h->precision == RBS_PRECISION_F64 && h->windowed;
}

// The pending device frame if its ingest is to run on stream s, taken: the caller launches that ingest (enqueue_loglikes: on
// the rectangles kernel's launch).  nullptr otherwise.
const float* take_device_frame(rbs_handle* h, hipStream_t s)
{
    if (h->fr.next.kind != NextFrame::DEVICE || h->fr.next.stream != s) return nullptr;
    const float* f = static_cast<const float*>(h->fr.next.src);
    h->fr.next = {};
    return f;
}

// Launch the ingest of a device frame left pending, on the stream it was given for; `then` (if not that stream) is ordered
// after it.
int32_t flush_device_frame(rbs_handle* h, hipStream_t then)
{
    if (h->fr.next.kind != NextFrame::DEVICE) return RBS_OK;
    const hipStream_t fs = h->fr.next.stream;
    const float* f = take_device_frame(h, fs);
    const size_t n = (size_t)h->npx;
    // (precision F32 keeps no per-pixel terms: a frame already in the handle's buffer needs nothing)
    if (h->d_aux || f != h->d_frame)
    hipLaunchKernelGGL(rbs::frame_aux_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, fs,
                       f, h->d_aux, h->d_pbg, h->npx, h->base.tw, h->base.ms, h->base.sf,
                       h->base.lambda, f == h->d_frame ? (float*)nullptr : h->d_frame);
    RBS_HIP(h, hipGetLastError());
    if (then != fs) {
        RBS_HIP(h, hipEventRecord(h->ev_fork, fs));
        RBS_HIP(h, hipStreamWaitEvent(then, h->ev_fork, 0));
    }
    return RBS_OK;
}

// A device frame pending on a caller's stream is ingested there, into d_frame: that stream first waits for the readers
// enqueued on the handle's stream so far.
int32_t device_frame_after_readers(rbs_handle* h)
{
    if (h->fr.next.kind != NextFrame::DEVICE || h->fr.next.stream == h->stream) return RBS_OK;
    RBS_HIP(h, hipEventRecord(h->ev_reader, h->stream));
    RBS_HIP(h, hipStreamWaitEvent(h->fr.next.stream, h->ev_reader, 0));
    return RBS_OK;
}

// Read done: frame N + 2's upload into the observation's staging image waits for the readers enqueued on s so far.
int32_t frame_read_done(rbs_handle* h, hipStream_t s)
{
    if (h->fr.cur >= 0) RBS_HIP(h, hipEventRecord(h->ev_used[h->fr.cur], s));
    return RBS_OK;
}

// Stream s waits for the upload of the observation's staging image (nothing to wait for on d_frame).
int32_t wait_for_upload(rbs_handle* h, hipStream_t s)
{
    if (h->fr.cur >= 0) RBS_HIP(h, hipStreamWaitEvent(s, h->ev_frame[h->fr.cur], 0));
    return RBS_OK;
}

// The staging image that served as the observation stops doing so (a new frame is coming): it may
// be overwritten once everything launched so far has run.
int32_t release_frame_slot(rbs_handle* h)
{
    if (int32_t rc = frame_read_done(h, h->stream)) return rc;
    h->fr.cur = -1;
    return RBS_OK;
}

// H2D of a frame staged in pinned host memory (`src`, normally staging(h)) on the upload stream into
// the device staging buffer of the current slot, which then IS the observation; the raster kernel
// waits for the upload (wait_for_upload).
// `pageable`: the caller's own frame, still to be staged into `src` (= staging(h)) -- staged and sent
// in h->upload_chunks pieces, so that the copy engine carries one piece while the host copies the next
// (a 640x480 frame: 41 us of memcpy + 29 us of transfer one after the other, ~20 us less interleaved).
// dbot hands the image over as a vector of DOUBLES (R:source/dbot_ros/util/ros_interface.h:152-168): double -> float while
// staging.  The scalar loop converts 2 values per instruction on a baseline x86-64 build; AVX2 (every host this library
// meets; checked at run time) does 4 per instruction and halves the time of a 640x480 frame.
#if defined(__x86_64__)
__attribute__((target("avx2"))) static void convert_f64_f32_avx2(float* __restrict__ dst, const double* __restrict__ src, size_t n)
{
    size_t p = 0;
    for (; p + 8 <= n; p += 8) {
        const __m128 a = _mm256_cvtpd_ps(_mm256_loadu_pd(src + p)), b = _mm256_cvtpd_ps(_mm256_loadu_pd(src + p + 4));
        _mm256_storeu_ps(dst + p, _mm256_set_m128(b, a));
    }
    for (; p < n; ++p) dst[p] = (float)src[p];
}
// AVX-512 hosts: 8 values per instruction and streaming stores (the staging image is read next by the copy engine, not by
// this core: no line of it needs to be fetched to be overwritten) -- 42 us against 50 per 640x480 frame out of L3 (EPYC 9575F,
// tools/dbg/convert_bench.cpp); the plugin path gains ~1 %
__attribute__((target("avx512f"))) static void convert_f64_f32_avx512(float* __restrict__ dst, const double* __restrict__ src, size_t n)
{
    size_t p = 0;
    for (; p + 16 <= n; p += 16) {
        const __m256 a = _mm512_cvtpd_ps(_mm512_loadu_pd(src + p)), b = _mm512_cvtpd_ps(_mm512_loadu_pd(src + p + 8));
        _mm512_stream_ps(dst + p, _mm512_castpd_ps(_mm512_insertf64x4(_mm512_castpd256_pd512(_mm256_castps_pd(a)), _mm256_castps_pd(b), 1)));
    }
    _mm_sfence();
    for (; p < n; ++p) dst[p] = (float)src[p];
}
#endif
static void convert_f64_f32(float* __restrict__ dst, const double* __restrict__ src, size_t n)
{
#if defined(__x86_64__)
    static const bool avx512 = __builtin_cpu_supports("avx512f") && !std::getenv("RBS_NO_AVX512");
    if (avx512 && (reinterpret_cast<uintptr_t>(dst) & 63) == 0) return convert_f64_f32_avx512(dst, src, n);
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2) return convert_f64_f32_avx2(dst, src, n);
#endif
    for (size_t p = 0; p < n; ++p) dst[p] = (float)src[p];
}

// Precision F64: the per-pixel model terms of the frame in d_fin[k], computed right behind its copy, on the upload stream,
// into the slot's own table -- the launch stream does not wait for the frame until the raster kernel needs it, so a caller's
// transition and the rectangles kernel run while the frame is still travelling (a tracker frame: 35 us of 400).
int32_t slot_aux(rbs_handle* h, int k)
{
    if (!h->d_aux) return RBS_OK;
    hipLaunchKernelGGL(rbs::frame_aux_kernel, dim3((unsigned)((h->npx + 255) / 256)), dim3(256), 0, h->up_stream,
                       h->d_fin[k], h->d_aux_slot[k], h->d_pbg, h->npx, h->base.tw, h->base.ms, h->base.sf, h->base.lambda, (float*)nullptr);
    RBS_HIP(h, hipGetLastError());
    return RBS_OK;
}

int32_t upload_frame(rbs_handle* h, const float* src, const float* pageable = nullptr, const double* pageable_f64 = nullptr)
{
    const int k = h->fr.stage;
    const size_t n = (size_t)h->npx;
    h->fr.next = {};   // (a frame uploaded ahead, or borrowed and never evaluated, is abandoned; a device frame: flushed first)
    // (the two staging images alternate, so k is never the image that serves as the observation --
    // should it be, its readers are recorded first: the wait below must not be on a stale event)
    if (k == h->fr.cur)
        if (int32_t rc = release_frame_slot(h)) return rc;
    RBS_HIP(h, hipStreamWaitEvent(h->up_stream, h->ev_used[k], 0));   // d_fin[k]: its readers were enqueued two frames ago
    // A SMALL frame (the reference's default operating point is 80x60: 19 KB) is not worth a transfer: a copy-engine
    // job costs ~11 us before it moves a byte and ~9 more until a kernel behind it starts.  The kernel that computes
    // the frame's model terms reads it where the host staged it (this handle's pinned buffer, over PCIe) and leaves
    // the observation in d_fin[k] as it goes (precision F32: that copy is all it does).
    const bool pull = n * sizeof(float) <= h->frame_pull_bytes && h->h_frames_dev[k] &&
                      (pageable || pageable_f64 || src == h->h_frames[k]);
    if (pageable || pageable_f64) {
        float* stage = h->h_frames[k];
        // (a frame of doubles takes the host ~4x as long to stage as a frame of floats: twice the pieces)
        const size_t want = (size_t)h->upload_chunks * (pageable_f64 && h->upload_chunks > 1 ? 2 : 1);
        const int pieces = h->quiet ? (int)std::max<size_t>(1, std::min<size_t>(want, n / 16384)) : 1;
        const size_t per = ((n + pieces - 1) / pieces + 1023) / 1024 * 1024;
        for (size_t off = 0; off < n; off += per) {
            const size_t len = std::min(per, n - off);
            if (pageable) std::memcpy(stage + off, pageable + off, len * sizeof(float));
            else convert_f64_f32(stage + off, pageable_f64 + off, len);   // dbot hands a vector of doubles
            if (!pull) RBS_HIP(h, hipMemcpyAsync(h->d_fin[k] + off, stage + off, len * sizeof(float), hipMemcpyHostToDevice, h->up_stream));
        }
    } else if (!pull) {
        RBS_HIP(h, hipMemcpyAsync(h->d_fin[k], src, n * sizeof(float), hipMemcpyHostToDevice, h->up_stream));
    }
    if (pull) {
        hipLaunchKernelGGL(rbs::frame_aux_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->up_stream,
                           h->h_frames_dev[k], h->d_aux ? h->d_aux_slot[k] : (double*)nullptr, h->d_pbg, h->npx, h->base.tw,
                           h->base.ms, h->base.sf, h->base.lambda, h->d_fin[k]);
        RBS_HIP(h, hipGetLastError());
    } else if (int32_t rc = slot_aux(h, k)) {
        return rc;
    }
    RBS_HIP(h, hipEventRecord(h->ev_frame[k], h->up_stream));
    if (int32_t rc = release_frame_slot(h)) return rc;
    h->fr.cur = k;   // (and, F64, its slot's table the model terms) until the next frame replaces it
    return RBS_OK;
}

// The pinned frame buffer the next host frame is staged in: the other one of the two, once the
// upload that last used it has finished (two frames ago: in practice never a wait).
int32_t next_frame_staging(rbs_handle* h)
{
    h->fr.stage ^= 1;
    RBS_HIP(h, hipEventSynchronize(h->ev_frame[h->fr.stage]));
    return RBS_OK;
}

// rbs_set_observation_borrowed's frame becomes the observation now: staged (double -> float) into pinned memory and sent.
int32_t stage_borrowed(rbs_handle* h)
{
    const NextFrame b = h->fr.next;
    if (!b.borrowed()) return RBS_OK;
    h->fr.next = {};
    if (int32_t rc = next_frame_staging(h)) return rc;
    if (b.kind == NextFrame::BORROWED_F64) return upload_frame(h, staging(h), nullptr, static_cast<const double*>(b.src));
    return upload_frame(h, staging(h), static_cast<const float*>(b.src));
}

// A borrowed frame is the caller's memory until the likelihood call behind it RETURNS -- however it returns.  A call that is
// refused or fails before its kernels staged the frame must not leave the pointer behind for a later call to read: on the way
// out the frame is copied after all (it becomes the observation, as rbs_set_observation would have made it), or dropped where
// the handle takes no more work.
struct BorrowedFrameGuard {
    rbs_handle* h;
    ~BorrowedFrameGuard()
    {
        if (!h->fr.next.borrowed()) return;
        if (h->poisoned || hipSetDevice(h->device) != hipSuccess) { h->fr.next = {}; return; }
        const std::string keep = h->err;      // (the message of the failure that brought us here stays rbs_last_error's)
        const int32_t rc = stage_borrowed(h);   // (whatever it returns, the frame is no longer the handle's)
        if (rc == RBS_OK) h->err = keep;
    }
};

// The NEXT frame, uploaded while the current one is still the observation (rbs_loglikes_prefetch: called between
// the launch of a call's kernels and the wait for its results, so the host's staging copy and the transfer pass
// behind the raster kernel): staged into the other pinned image, sent on the upload stream, its model terms
// (precision F64) computed behind it -- everything upload_frame does except making it the observation.
// What rbs_loglikes_prefetch needs, checked BEFORE the call's kernels are enqueued (a prefetch that failed
// behind an updating call left the caller with a failed call whose planes had already flipped).
int32_t prefetch_check(rbs_handle* h)
{
    if (h->fr.next.kind == NextFrame::AHEAD)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "loglikes_prefetch: the frame uploaded ahead by the previous rbs_loglikes_prefetch has not been "
                                                 "installed yet (rbs_set_observation_prefetched)");
    if ((h->fr.stage ^ 1) == h->fr.cur)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, "loglikes_prefetch: the staging image the next frame would use is the current observation "
                                                 "(the staging images did not alternate)");
    return RBS_OK;
}

int32_t prefetch_frame(rbs_handle* h, const float* depth)
{
    if (int32_t rc = prefetch_check(h)) return rc;   // (before the staging image is switched: a refused call changes nothing)
    if (int32_t rc = next_frame_staging(h)) return rc;
    const int k = h->fr.stage;
    const size_t n = (size_t)h->npx;
    RBS_HIP(h, hipStreamWaitEvent(h->up_stream, h->ev_used[k], 0));   // d_fin[k]: its readers were enqueued two frames ago
    std::memcpy(h->h_frames[k], depth, n * sizeof(float));
    RBS_HIP(h, hipMemcpyAsync(h->d_fin[k], h->h_frames[k], n * sizeof(float), hipMemcpyHostToDevice, h->up_stream));
    if (int32_t rc = slot_aux(h, k)) return rc;
    RBS_HIP(h, hipEventRecord(h->ev_frame[k], h->up_stream));
    h->fr.next = {NextFrame::AHEAD, nullptr, nullptr, k};
    return RBS_OK;
}


// Make current: the observation complete in stream s's order -- a borrowed frame staged, a device frame ingested, the upload
// of a host frame waited for.
int32_t make_current(rbs_handle* h, hipStream_t s)
{
    if (int32_t rc = stage_borrowed(h)) return rc;
    if (int32_t rc = flush_device_frame(h, s)) return rc;
    return wait_for_upload(h, s);
}

// Begin, the prologue of every hand-over: a handle left undefined by a failed call is refused, and a buffer acquired but never
// committed is abandoned.  Then, once the entry point has checked its frame, frame_ready: on the handle's device, a device
// frame handed over before and never evaluated is ingested (its clock tick stays counted), ordered before stream s.
int32_t frame_begin(rbs_handle* h)
{
    RBS_REFUSE_POISONED(h);
    h->fr.acquired = false;
    return RBS_OK;
}
int32_t frame_ready(rbs_handle* h, hipStream_t s)
{
    RBS_HIP(h, hipSetDevice(h->device));
    return flush_device_frame(h, s);
}

// Hand over: the frame becomes the observation -- a borrowed or device frame at the next call that needs it -- whatever waited
// in fr.next is abandoned, and the model clock advances one frame.
// ... the caller's host frame (floats or doubles), copied now
int32_t hand_over_host(rbs_handle* h, const float* f32, const double* f64)
{
    if (int32_t rc = next_frame_staging(h)) return rc;
    if (int32_t rc = upload_frame(h, staging(h), f32, f64)) return rc;   // (staged and sent piece by piece)
    h->pending_frames += 1;
    h->frames_handed += 1;
    return RBS_OK;
}
// ... a frame in pinned memory: the committed buffer (a group's: shard 0's, sent to every shard)
int32_t hand_over_pinned(rbs_handle* h, const float* src)
{
    if (int32_t rc = upload_frame(h, src)) return rc;
    h->pending_frames += 1;
    h->frames_handed += 1;
    return RBS_OK;
}
// ... the driver's full-resolution frame, sub-sampled by f.
// The reference's rule (R:source/dbot_ros/util/ros_interface.h:152-168): evaluated(r, c) =
// native(r f, c f) -- applied while the frame is staged, so that only the rows*cols values the
// sensor evaluates are copied and sent (1/f^2 of the driver's frame: 19 KB of 1.2 MB at the
// reference's default factor 8) and the frame then travels like any other host frame.
int32_t hand_over_native(rbs_handle* h, const float* native, int width, int f)
{
    if (int32_t rc = next_frame_staging(h)) return rc;
    for (int r = 0; r < h->rows; ++r) {
        const float* src = native + (size_t)r * f * width;
        float* dst = staging(h) + (size_t)r * h->cols;
        for (int c = 0; c < h->cols; ++c) dst[c] = src[(size_t)c * f];
    }
    return hand_over_pinned(h, staging(h));
}
// ... the caller's host frame, borrowed (can_borrow): a borrowed frame nobody evaluated is simply replaced
void hand_over_borrowed(rbs_handle* h, const float* f32, const double* f64)
{
    h->fr.next = f64 ? NextFrame{NextFrame::BORROWED_F64, f64} : NextFrame{NextFrame::BORROWED_F32, f32};
    h->pending_frames += 1;
    h->frames_handed += 1;
}
// ... a frame in device memory, ingested on stream s by whatever needs it first
int32_t hand_over_device(rbs_handle* h, const float* d_depth, hipStream_t s)
{
    if (int32_t rc = release_frame_slot(h)) return rc;
    h->fr.next = {NextFrame::DEVICE, d_depth, s};
    h->pending_frames += 1;
    h->frames_handed += 1;
    return RBS_OK;
}
// ... the frame uploaded ahead (fr.next is AHEAD)
int32_t hand_over_ahead(rbs_handle* h)
{
    const int k = h->fr.next.slot;
    h->fr.next = {};
    if (int32_t rc = release_frame_slot(h)) return rc;   // the readers of the frame it replaces are on the launch stream by now
    h->fr.cur = k;
    h->pending_frames += 1;
    h->frames_handed += 1;
    return RBS_OK;
}

// The pinned image the caller writes the next frame into (rbs_acquire_frame_buffer).  One image (shard 0's) feeds every device
// of a group: it is free once every shard's upload of the frame before last has finished.
int32_t acquire_staging(rbs_handle* h, float** buf)
{
    rbs_handle* const s0 = h->shards.empty() ? h : h->shards[0];
    const int k = s0->fr.stage ^ 1;
    for (size_t i = 0; i < std::max<size_t>(1, h->shards.size()); ++i) {
        rbs_handle* sh = h->shards.empty() ? h : h->shards[i];
        RBS_HIP(h, hipSetDevice(sh->device));
        sh->fr.stage = k;
        RBS_HIP(h, hipEventSynchronize(sh->ev_frame[k]));
    }
    *buf = staging(s0);
    h->fr.acquired = true;
    return RBS_OK;
}

// rbs_reset: an acquired buffer, a borrowed frame and a frame uploaded ahead belong to the session that ended (a device frame
// has been ingested by the drain before).
void frame_abandon(rbs_handle* h)
{
    h->fr.acquired = false;
    h->fr.next = {};
}

}  // namespace
