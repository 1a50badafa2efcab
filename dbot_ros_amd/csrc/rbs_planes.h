// rbs_planes.h -- the occlusion planes' storage, host side: a slot as a whole plane and back for every layout (dense planes, windowed
// planes, slabs, stamped planes, each with or without the shared trail), the slabs' growth and housekeeping, drain.  Each rule of
// the layouts stands here once; the entry points that read or write a slot are in rbs_planes_api.h.
// Not a header to include elsewhere: a section of rbsensor_capi.hip's translation unit, included there once after rbs_call.h
// (create_impl and the group code need it).
namespace {

int32_t drain(rbs_handle* h, bool host_sync);
int32_t grow_slabs(rbs_handle* h, int new_slab);

// Where a slot's plane (or slab) starts in the current buffer.
float* slot_base(const rbs_handle* h, int slot) { return h->d_occ[h->cur] + (size_t)slot * h->plane_stride; }
// The shared trail's background plane while it is active; nullptr: the background is the scalar level.
const float* shared_plane(const rbs_handle* h) { return h->stp ? (const float*)h->d_bgp[h->cur] : nullptr; }
dim3 px_grid(long px) { return dim3((unsigned)((px + 255) / 256)); }

// table[slot] = rect on stream s (table: d_win[cur], or d_reg[cur] -- a slab's stored region).
int32_t set_window(rbs_handle* h, int4* table, int slot, int4 rect, hipStream_t s)
{
    hipLaunchKernelGGL(rbs::rbs_set_window_kernel, dim3(1), dim3(64), 0, s, table + slot, 1, rect);
    RBS_HIP(h, hipGetLastError());
    return RBS_OK;
}
// "This slot's window is the whole frame."
int4 window_full(const rbs_handle* h) { return make_int4(0, 0, h->cols, h->rows); }

// w x rows floats between two pitched images on stream s (pitches in floats; a packed payload's pitch is w).
int32_t copy_window(rbs_handle* h, float* dst, size_t dst_pitch, const float* src, size_t src_pitch, int w, int rows, hipStream_t s)
{
    RBS_HIP(h, hipMemcpy2DAsync(dst, sizeof(float) * dst_pitch, src, sizeof(float) * src_pitch, sizeof(float) * (size_t)w, (size_t)rows,
                                hipMemcpyDeviceToDevice, s));
    return RBS_OK;
}

// Windowed planes: make slot's current plane dense in place (background outside its window) and
// mark its window full, on stream s.  Dense planes: nothing to do.
int32_t materialize(rbs_handle* h, int slot, hipStream_t s)
{
    if (!h->windowed) return RBS_OK;
    if (h->exact) return fail(h, RBS_ERR_UNSUPPORTED, "a slot of stamped planes (occlusion_mode REFERENCE) is not a float plane: use rbs_export_plane / rbs_get_occlusion");
    if (h->slab_px) return fail(h, RBS_ERR_UNSUPPORTED, "a slab cannot be made dense in place (state_slab_px)");
    hipLaunchKernelGGL(rbs::rbs_materialize_kernel, px_grid(h->npx), dim3(256), 0, s, slot_base(h, slot), h->d_win[h->cur] + slot, h->rows, h->cols,
                       h->background, shared_plane(h));
    RBS_HIP(h, hipGetLastError());
    return set_window(h, h->d_win[h->cur], slot, window_full(h), s);
}

// Slabs: a slot's plane as a whole plane in `d_full` (device, npx floats), on stream s.
int32_t slab_expand(rbs_handle* h, int slot, float* d_full, hipStream_t s)
{
    hipLaunchKernelGGL(rbs::rbs_expand_kernel, px_grid(h->npx), dim3(256), 0, s, slot_base(h, slot), h->d_reg[h->cur] + slot, h->d_win[h->cur] + slot,
                       h->rows, h->cols, h->background, d_full, shared_plane(h));
    RBS_HIP(h, hipGetLastError());
    return RBS_OK;
}

// Slab size that holds a region of `need` px with room to move.
// (1.5 x: a slab enlarged for `need` is at most two thirds full, below the three quarters that trigger the next
// enlargement -- with 1.25 x the trigger stayed true after growing and every synchronising call drained the handle: ADVICE r3)
int slab_for(const rbs_handle* h, int need) { return (int)std::min<long>(h->npx, (long)need + need / 2 + 1024); }

// Slabs: `px` values handed in from outside fit a slot, or the slabs grow until they do: as they grow for a region a call asks for
// (every rank enlarges its slabs on its own schedule: ADVICE r4) -- on a handle of its own; the shards of a group and
// attached ranks must keep one size among them.  `what` / `what_grown`: the noun phrase of the refusal before / after growing.
// The buffers are replaced: a pointer into them taken before is stale afterwards.
int32_t fit_or_grow(rbs_handle* h, long px, hipStream_t s, const std::string& what, const std::string& what_grown)
{
    if (px <= (long)h->slab_px) return RBS_OK;
    if (h->group || h->peer_world > 1)
        return fail(h, RBS_ERR_OUT_OF_MEMORY, fmt("%s does not fit a slab of %d px (state_slab_px)", what.c_str(), h->slab_px));
    if (int32_t rc = drain(h, true)) return rc;
    RBS_HIP(h, hipStreamSynchronize(s));   // (earlier imports on the caller's stream wrote into the buffers about to be replaced;
                                           //  store_plane has synchronised s for its box already: nothing to wait for there)
    if (int32_t rc = grow_slabs(h, slab_for(h, (int)std::min<long>(px, h->npx)))) return rc;
    if (px > (long)h->slab_px)
        return fail(h, RBS_ERR_OUT_OF_MEMORY, fmt("%s does not fit a slab of %d px (state_slab_px)", what_grown.c_str(), h->slab_px));
    return RBS_OK;
}

// Stamped planes (occlusion_mode REFERENCE): the hooks' two conversions.  A slot -> its plane of EFFECTIVE values as of the
// epoch (device, npx floats); slot < 0: the shared background plane itself.
int32_t exact_expand(rbs_handle* h, int slot, float* d_full, hipStream_t s)
{
    DevParams P = h->base;
    P.ptab = h->d_ptab;
    P.age_max = h->age_max;
    hipLaunchKernelGGL(rbs::rbs_expand_exact_kernel, px_grid(h->npx), dim3(256), 0, s, slot >= 0 ? (const float*)slot_base(h, slot) : (const float*)nullptr,
                       h->slab_px ? h->slab_px : h->npx,
                       slot >= 0 && h->slab_px ? (const int4*)(h->d_reg[h->cur] + slot) : (const int4*)nullptr,
                       slot >= 0 ? (const int4*)(h->d_win[h->cur] + slot) : (const int4*)nullptr, h->rows, h->cols, h->background,
                       shared_plane(h), P, d_full);
    RBS_HIP(h, hipGetLastError());
    return RBS_OK;
}

// A whole plane handed in from outside (device, npx floats) -> a slot of slabs or stamped planes: its window -- on slabs its stored
// region too -- becomes the float4-aligned bounding box of the values that differ from the background.  Stamped planes take the
// values as EFFECTIVE ones with age 0 ("as of now", the rule of the oracle's set_occlusion).  Synchronises s (the box is needed
// on the host: a slab must fit it).
int32_t store_plane(rbs_handle* h, int slot, const float* d_full, hipStream_t s)
{
    const bool slab = h->slab_px != 0;
    const float* bgref = shared_plane(h);   // "the background" per pixel: nullptr (the scalar level), or the shared plane's values
    if (h->exact && h->stp) {               // ... of a stamped shared plane: what its pixels are worth now, not what they hold
        if (int32_t rc = exact_expand(h, -1, h->d_tmp_plane, s)) return rc;
        bgref = h->d_tmp_plane;
    }
    const int init[4] = {h->cols, h->rows, 0, 0};
    RBS_HIP(h, hipMemcpyAsync(h->d_bbox, init, sizeof(init), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(rbs::rbs_bbox_kernel, px_grid(h->npx), dim3(256), 0, s, d_full, h->rows, h->cols, h->background, h->d_bbox, bgref);
    RBS_HIP(h, hipGetLastError());
    int box[4];
    RBS_HIP(h, hipMemcpyAsync(box, h->d_bbox, sizeof(box), hipMemcpyDeviceToHost, s));
    RBS_HIP(h, hipStreamSynchronize(s));
    int4 r = make_int4(box[0], box[1], std::min(box[2], h->cols), box[3]);
    if (r.z <= r.x || r.w <= r.y) r = make_int4(h->cols, h->rows, 0, 0);   // all background
    const long area = r.z > r.x ? (long)(r.z - r.x) * (r.w - r.y) : 0;
    // (whole stamped planes: the box is only the window -- nothing to fit, no stored region)
    if (slab)
        if (int32_t rc = fit_or_grow(h, area, s, fmt("a plane whose values differ from the background over %ld px", area), fmt("a plane of %ld px", area))) return rc;
    if (area > 0) {
        if (h->exact)
            hipLaunchKernelGGL(rbs::rbs_pack_exact_kernel, px_grid(area), dim3(256), 0, s, d_full, bgref, h->background, r, h->cols,
                               slab ? r.x : 0, slab ? r.y : 0, slab ? r.z - r.x : h->cols, slot_base(h, slot), slab ? h->slab_px : h->npx);
        else
            hipLaunchKernelGGL(rbs::rbs_pack_kernel, px_grid(area), dim3(256), 0, s, d_full, r, h->cols, slot_base(h, slot));
        RBS_HIP(h, hipGetLastError());
    }
    if (int32_t rc = set_window(h, h->d_win[h->cur], slot, r, s)) return rc;
    if (slab) if (int32_t rc = set_window(h, h->d_reg[h->cur], slot, r, s)) return rc;
    if (h->exact) RBS_HIP(h, hipStreamSynchronize(s));   // (stamped planes are stored when this returns; float slabs when s gets there)
    return RBS_OK;
}

// The sender's plane is its scalar background outside `r` and the packed payload inside (r empty: no payload): written out whole
// into d_plane (npx floats) on stream s.
int32_t fill_and_paste(rbs_handle* h, float* d_plane, int4 r, const float* d_payload, hipStream_t s)
{
    hipLaunchKernelGGL(rbs::rbs_fill_kernel, dim3(256), dim3(256), 0, s, d_plane, (size_t)h->npx, h->background);
    RBS_HIP(h, hipGetLastError());
    if (r.z <= r.x) return RBS_OK;
    return copy_window(h, d_plane + (size_t)r.y * h->cols + r.x, (size_t)h->cols, d_payload, (size_t)(r.z - r.x), r.z - r.x, r.w - r.y, s);
}

// "A region did not fit its slab" (h_err[0], fetched by the synchronising entry points): the message
// of the calls that cannot repair it themselves (asynchronous calls, the device tracker).
int32_t check_slab_error(rbs_handle* h)
{
    if (!h->slab_px || !h->h_err[0]) return RBS_OK;
    return fail(h, RBS_ERR_OUT_OF_MEMORY,
                fmt("a particle's occlusion window (with its screen rectangle) exceeded the slab of %d px "
                    "(rbs_config.state_slab_px) in a call that had already returned: its log-likelihood is NaN and its "
                    "plane was reset to the background; the slabs have been enlarged for the calls that follow", h->slab_px));
}

// Bytes to ask hipMalloc for when `bytes` are needed for a plane buffer.  A buffer whose size has bit 31 set
// (2-4 GiB, 6-8 GiB, ...) cannot be imported by another process on ROCm 7.2: hipIpcOpenMemHandle never
// returns (measured, tools/dbg/ipc_attach_notorch.py: 13 900 x 38 400 px opens at once, 14 500 x 38 400 hangs,
// 30 000 x 38 400 opens, 50 000 x 38 400 hangs).  Such sizes are rounded up to the next multiple of 4 GiB.
size_t occ_alloc_bytes(size_t bytes)
{
    return (bytes & 0x80000000ull) ? ((bytes >> 32) + 1) << 32 : bytes;
}

// Every slot gets `new_slab` floats (> the current size).  A slot stores its region row-major from
// its first float, so the planes move with one strided copy; the regions' tables stay as they are.
// Only the CURRENT buffer holds state (the other one is written from scratch by the next updating
// call).  The caller has drained the handle.
int32_t grow_slabs(rbs_handle* h, int new_slab)
{
    new_slab = std::min(h->npx, (new_slab + 1023) & ~1023);
    if (new_slab <= h->slab_px) return RBS_OK;
    if (h->peer_world > 1)   // the other ranks address these slabs with a fixed stride through their mappings
        return h->h_err[0] ? fail(h, RBS_ERR_OUT_OF_MEMORY,
                                  fmt("a region of %d px does not fit the slab of %d px, and slabs cannot grow once the handle is "
                                      "attached to other ranks (rbs_ipc_attach): create the handles with a larger state_slab_px",
                                      h->h_err[1], h->slab_px))
                           : RBS_OK;
    float* nb[2] = {nullptr, nullptr};
    const size_t new_stride = h->exact ? exact_stride((size_t)new_slab) : (size_t)new_slab;
    const size_t bytes = sizeof(float) * new_stride * h->max_particles;
    for (int k = 0; k < 2; ++k)
        if (hipMalloc(&nb[k], occ_alloc_bytes(bytes)) != hipSuccess) {
            (void)hipGetLastError();
            (void)hipFree(nb[0]);
            return fail(h, RBS_ERR_OUT_OF_MEMORY, fmt("enlarging the occlusion slabs from %d to %d px per slot needs 2 x %zu bytes more", h->slab_px, new_slab, bytes));
        }
    RBS_HIP(h, hipMemcpy2DAsync(nb[h->cur], sizeof(float) * new_stride, h->d_occ[h->cur], sizeof(float) * h->plane_stride,
                                sizeof(float) * (size_t)h->slab_px, (size_t)h->max_particles, hipMemcpyDeviceToDevice, h->stream));
    if (h->exact)   // ... and the slots' ages, which follow the values of a slot
        RBS_HIP(h, hipMemcpy2DAsync(nb[h->cur] + new_slab, sizeof(float) * new_stride, h->d_occ[h->cur] + h->slab_px, sizeof(float) * h->plane_stride,
                                    sizeof(unsigned short) * (size_t)h->slab_px, (size_t)h->max_particles, hipMemcpyDeviceToDevice, h->stream));
    RBS_HIP(h, hipStreamSynchronize(h->stream));
    (void)hipFree(h->d_occ[0]);
    (void)hipFree(h->d_occ[1]);
    h->d_occ[0] = nb[0];
    h->d_occ[1] = nb[1];
    h->slab_px = new_slab;
    h->plane_stride = new_stride;
    return RBS_OK;
}

// What a call must put back to be run again: an updating call only flips the buffers and moves the
// background level on -- the planes it read are intact.
// What a call that is taken back (a region did not fit its slab) must find as it was.  The shared trail's mode belongs to it:
// the planes the repeated call reads are measured against whatever background -- shared plane or scalar -- the FIRST attempt
// found, and an attempt that left the shared trail (or entered it, or re-based) has already switched the handle's view.
struct CallState { int cur; int pending_frames; float background; bool stp; long stp_last_rebase, stp_rebases, stp_block_until; double area_frac; bool wide; long update_clock; };
CallState save_call_state(const rbs_handle* h)
{
    return {h->cur, h->pending_frames, h->background, h->stp, h->stp_last_rebase, h->stp_rebases, h->stp_block_until, h->area_frac, h->wide, h->update_clock};
}
void restore_call_state(rbs_handle* h, const CallState& c)
{
    h->cur = c.cur; h->pending_frames = c.pending_frames; h->background = c.background; h->update_clock = c.update_clock;
    h->stp = c.stp; h->stp_last_rebase = c.stp_last_rebase; h->stp_rebases = c.stp_rebases; h->stp_block_until = c.stp_block_until;
    h->area_frac = c.area_frac; h->wide = c.wide;
}

// After a synchronising call on an idle handle: enlarge the slabs BEFORE a region fills one (the
// regions move a few pixels per frame; three quarters full is the trigger).  Clears the flag.
int32_t slab_housekeeping(rbs_handle* h)
{
    if (!h->slab_px) return RBS_OK;
    const bool overflowed = h->h_err[0] != 0;
    // drain (a host synchronisation of both streams) only when the slabs will really be reallocated: h_err[1] is a
    // sticky maximum, and a slab that is already the whole frame, or large enough for it, has nothing to gain
    const int target = (int)std::min<long>(h->npx, ((long)slab_for(h, h->h_err[1]) + 1023) & ~1023L);
    const bool grow = (long)h->h_err[1] * 4 > (long)h->slab_px * 3 && target > h->slab_px && h->peer_world <= 1;
    if (overflowed || grow) {
        if (int32_t rc = drain(h, true)) return rc;
        if (int32_t rc = grow_slabs(h, slab_for(h, h->h_err[1]))) return rc;
    }
    if (overflowed) {
        RBS_HIP(h, hipMemsetAsync(h->d_err, 0, sizeof(int), h->stream));   // (the flag; the maximum stays)
        h->h_err[0] = 0;
    }
    return RBS_OK;
}

// Make stream `s` (and the host, if sync) see the planes of the last updating call complete.
int32_t drain(rbs_handle* h, bool host_sync)
{
    if (int32_t rc = flush_device_frame(h, h->stream)) return rc;
    if (h->join_pending >= 0) {
        RBS_HIP(h, hipStreamWaitEvent(h->stream, h->ev_join[h->join_pending], 0));
        if (host_sync) RBS_HIP(h, hipEventSynchronize(h->ev_join[h->join_pending]));
        h->join_pending = -1;
    }
    if (host_sync) {
        RBS_HIP(h, hipStreamSynchronize(h->stream));
        RBS_HIP(h, hipStreamSynchronize(h->copy_stream));
    }
    return RBS_OK;
}

}  // namespace
