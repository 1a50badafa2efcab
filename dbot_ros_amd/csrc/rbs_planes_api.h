// rbs_planes_api.h -- the entry points that read or write one slot's occlusion plane: rbs_get_occlusion, rbs_set_occlusion,
// rbs_occlusion_device_ptr, rbs_occlusion_next_device_ptr, rbs_export_plane, rbs_import_plane, rbs_stream_join, rbs_export_window,
// rbs_import_window, rbs_get_window -- over the storage rules of rbs_planes.h.
// Not a header to include elsewhere: a section of rbsensor_capi.hip's translation unit, included there once INSIDE its extern "C"
// block of sensor entry points, after the group code.  Every slot entry point opens the same way: the null handle; RBS_GROUP_SLOT
// (a group routes the global slot to its shard and returns: "bad slot %d" from its own range check, a shard's failure through
// gfail as "device %d: ..."); then, on a handle of its own, one of the two prologues below.

// `stream` (null: the handle's own) sees the planes of the last updating call complete, side stream included.
static int32_t join_stream(rbs_handle* h, void* stream, hipStream_t* s)
{
    *s = stream ? static_cast<hipStream_t>(stream) : h->stream;
    if (h->join_pending >= 0) RBS_HIP(h, hipStreamWaitEvent(*s, h->ev_join[h->join_pending], 0));
    return RBS_OK;
}

// The prologue of the entry points that work on the handle's stream: the slot and the pointer the call cannot do without, the
// device.  Draining is the caller's, after the refusals it wants to win over it.
static int32_t slot_enter(rbs_handle* h, const char* name, int slot, const void* required)
{
    if (slot < 0 || slot >= h->max_particles || !required)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("%s: bad slot %d", name, slot));
    RBS_HIP(h, hipSetDevice(h->device));
    return RBS_OK;
}
// ... and of those that work on the caller's stream, which waits for a pending join: nothing drains, nothing blocks.
static int32_t slot_enter_on(rbs_handle* h, const char* name, int slot, const void* required, void* stream, hipStream_t* s)
{
    if (int32_t rc = slot_enter(h, name, slot, required)) return rc;
    return join_stream(h, stream, s);
}

// A slot's window as the host needs it for the window-sized transport (one 16-byte read-back).
static int32_t window_of(rbs_handle* h, int slot, hipStream_t s, int box[4])
{
    if (!h->windowed) { box[0] = 0; box[1] = 0; box[2] = h->cols; box[3] = h->rows; return RBS_OK; }
    RBS_HIP(h, hipMemcpyAsync(box, h->d_win[h->cur] + slot, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    RBS_HIP(h, hipStreamSynchronize(s));
    if (box[2] <= box[0] || box[3] <= box[1]) { box[0] = h->cols; box[1] = h->rows; box[2] = 0; box[3] = 0; }
    return RBS_OK;
}

int32_t rbs_get_occlusion(rbs_handle* h, int32_t slot, float* out)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_GROUP_SLOT(h, slot, rbs_get_occlusion(sh_, l_, out));
    if (int32_t rc = slot_enter(h, "get_occlusion", slot, out)) return rc;
    if (int32_t rc = drain(h, true)) return rc;
    const float* src = h->d_render;   // slabs, stamped planes: assembled beside the slots; whole float planes: made dense in place
    if (h->slab_px || h->exact) {
        if (int32_t rc = h->exact ? exact_expand(h, slot, h->d_render, h->stream) : slab_expand(h, slot, h->d_render, h->stream)) return rc;
    } else {
        if (int32_t rc = materialize(h, slot, h->stream)) return rc;
        src = slot_base(h, slot);
    }
    RBS_HIP(h, hipStreamSynchronize(h->stream));
    RBS_HIP(h, hipMemcpy(out, src, sizeof(float) * h->npx, hipMemcpyDeviceToHost));
    return RBS_OK;
}

int32_t rbs_set_occlusion(rbs_handle* h, int32_t slot, const float* plane)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_GROUP_SLOT(h, slot, rbs_set_occlusion(sh_, l_, plane));
    if (int32_t rc = slot_enter(h, "set_occlusion", slot, plane)) return rc;
    if (int32_t rc = drain(h, true)) return rc;
    if (h->slab_px || h->exact) {
        RBS_HIP(h, hipMemcpy(h->d_render, plane, sizeof(float) * h->npx, hipMemcpyHostToDevice));
        return store_plane(h, slot, h->d_render, h->stream);
    }
    RBS_HIP(h, hipMemcpy(slot_base(h, slot), plane, sizeof(float) * h->npx, hipMemcpyHostToDevice));
    if (h->windowed) {   // the whole plane is explicit now; the next updating call tightens it again
        if (int32_t rc = set_window(h, h->d_win[h->cur], slot, window_full(h), h->stream)) return rc;
        RBS_HIP(h, hipStreamSynchronize(h->stream));   // (a host call: done when it returns -- rbs_import_plane does not wait)
    }
    return RBS_OK;
}

int32_t rbs_occlusion_device_ptr(rbs_handle* h, int32_t slot, void** out)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_GROUP_SLOT(h, slot, rbs_occlusion_device_ptr(sh_, l_, out));
    if (int32_t rc = slot_enter(h, "occlusion_device_ptr", slot, out)) return rc;
    // (the order of the refusals: stamped planes here, before draining; slabs in materialize, after it)
    if (h->exact) return fail(h, RBS_ERR_UNSUPPORTED, "occlusion_device_ptr: a slot of stamped planes (occlusion_mode REFERENCE) is not a float plane");
    if (int32_t rc = drain(h, true)) return rc;   // planes complete before the caller touches them
    if (int32_t rc = materialize(h, slot, h->stream)) return rc;   // and dense, whatever the caller does next
    RBS_HIP(h, hipStreamSynchronize(h->stream));
    *out = slot_base(h, slot);
    return RBS_OK;
}

int32_t rbs_occlusion_next_device_ptr(rbs_handle* h, int32_t slot, void** out)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_GROUP_SLOT(h, slot, rbs_occlusion_next_device_ptr(sh_, l_, out));
    if (int32_t rc = slot_enter(h, "occlusion_next_device_ptr", slot, out)) return rc;
    // (the order of the refusals: slabs, then stamped planes, then the drain)
    if (h->slab_px) return fail(h, RBS_ERR_UNSUPPORTED, "occlusion_next_device_ptr: slots are slabs, not planes (state_slab_px)");
    if (h->exact) return fail(h, RBS_ERR_UNSUPPORTED, "occlusion_next_device_ptr: a slot of stamped planes (occlusion_mode REFERENCE) is not a float plane");
    if (int32_t rc = drain(h, true)) return rc;   // planes complete before the caller touches them
    *out = h->d_occ[1 - h->cur] + (size_t)slot * h->npx;
    return RBS_OK;
}

int32_t rbs_export_plane(rbs_handle* h, int32_t slot, void* d_dst, void* stream)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_GROUP_SLOT(h, slot, rbs_export_plane(sh_, l_, d_dst, stream));
    hipStream_t s;
    if (int32_t rc = slot_enter_on(h, "export_plane", slot, d_dst, stream, &s)) return rc;
    if (h->exact) return exact_expand(h, slot, static_cast<float*>(d_dst), s);
    if (h->slab_px) return slab_expand(h, slot, static_cast<float*>(d_dst), s);
    if (int32_t rc = materialize(h, slot, s)) return rc;
    RBS_HIP(h, hipMemcpyAsync(d_dst, slot_base(h, slot), sizeof(float) * h->npx, hipMemcpyDeviceToDevice, s));
    return RBS_OK;
}

int32_t rbs_import_plane(rbs_handle* h, int32_t slot, const void* d_src, void* stream)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_GROUP_SLOT(h, slot, rbs_import_plane(sh_, l_, d_src, stream));
    hipStream_t s;
    if (int32_t rc = slot_enter_on(h, "import_plane", slot, d_src, stream, &s)) return rc;
    if (h->exact || h->slab_px) return store_plane(h, slot, static_cast<const float*>(d_src), s);   // (synchronises: the box must fit)
    RBS_HIP(h, hipMemcpyAsync(slot_base(h, slot), d_src, sizeof(float) * h->npx, hipMemcpyDeviceToDevice, s));
    if (h->windowed) return set_window(h, h->d_win[h->cur], slot, window_full(h), s);   // (asynchronous: rbs_set_occlusion waits here)
    return RBS_OK;
}

int32_t rbs_stream_join(rbs_handle* h, void* stream)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    if (!h->shards.empty()) {
        for (rbs_handle* sh_ : h->shards)
            if (int32_t rc = rbs_stream_join(sh_, stream)) return gfail(h, sh_, rc);
        return RBS_OK;
    }
    RBS_HIP(h, hipSetDevice(h->device));
    hipStream_t s;
    return join_stream(h, stream, &s);
}

int32_t rbs_export_window(rbs_handle* h, int32_t slot, int32_t rect_out[4], void* d_payload, size_t capacity_floats, void* stream)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_GROUP_SLOT(h, slot, rbs_export_window(sh_, l_, rect_out, d_payload, capacity_floats, stream));
    hipStream_t s;
    if (int32_t rc = slot_enter_on(h, "export_window", slot, rect_out, stream, &s)) return rc;
    int box[4] = {0, 0, h->cols, h->rows};
    const float* src;   // where the window is cut from
    if (h->exact) {
        // stamped planes travel as EFFECTIVE values (what the receiver's rbs_import_window takes "as of now"): the slot's plane is
        // assembled beside the slots and its window cut out of it (shared trail: the whole plane, as below -- reported without
        // reading the window back, which would synchronise)
        if (int32_t rc = exact_expand(h, slot, h->d_render, s)) return rc;
        if (!h->stp) if (int32_t rc = window_of(h, slot, s, box)) return rc;
        src = h->d_render;
    } else if (h->stp && h->slab_px) {
        // (shared trail: outside its window the plane is the handle's background PLANE, which the receiver does not have -- a slab
        // cannot be made dense in place: the whole plane is assembled beside it and travels from there)
        for (int k = 0; k < 4; ++k) rect_out[k] = box[k];
        if ((size_t)h->npx > capacity_floats || !d_payload)
            return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("export_window: the plane of slot %d travels whole (%d values), the buffer holds %zu", slot, h->npx, capacity_floats));
        return slab_expand(h, slot, static_cast<float*>(d_payload), s);
    } else {
        // (shared trail, whole planes: the slot is made dense first and travels whole)
        if (h->stp) if (int32_t rc = materialize(h, slot, s)) return rc;
        if (int32_t rc = window_of(h, slot, s, box)) return rc;
        src = slot_base(h, slot);
    }
    for (int k = 0; k < 4; ++k) rect_out[k] = box[k];
    const int w = box[2] - box[0], hh = box[3] - box[1];
    if (w <= 0 || hh <= 0) return RBS_OK;   // all background: nothing to carry
    if ((size_t)w * (size_t)hh > capacity_floats || !d_payload)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("export_window: the window of slot %d holds %d x %d values, the buffer %zu", slot, w, hh, capacity_floats));
    // where the window's first value is stored, and the stored row length: a frame's, or the stored region's of a slab
    int reg[4] = {0, 0, h->cols, h->rows};
    if (h->slab_px && !h->exact) {
        RBS_HIP(h, hipMemcpyAsync(reg, h->d_reg[h->cur] + slot, sizeof(reg), hipMemcpyDeviceToHost, s));
        RBS_HIP(h, hipStreamSynchronize(s));
    }
    const size_t pitch = (size_t)(reg[2] - reg[0]);
    return copy_window(h, static_cast<float*>(d_payload), (size_t)w, src + (size_t)(box[1] - reg[1]) * pitch + (size_t)(box[0] - reg[0]), pitch, w, hh, s);
}

int32_t rbs_import_window(rbs_handle* h, int32_t slot, const int32_t rect[4], const void* d_payload, void* stream)
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_GROUP_SLOT(h, slot, rbs_import_window(sh_, l_, rect, d_payload, stream));
    hipStream_t s;
    if (int32_t rc = slot_enter_on(h, "import_window", slot, rect, stream, &s)) return rc;
    int4 r = make_int4(rect[0], rect[1], rect[2], rect[3]);
    const bool empty = r.z <= r.x || r.w <= r.y;
    if (empty) r = make_int4(h->cols, h->rows, 0, 0);
    else if (r.x < 0 || r.y < 0 || r.z > h->cols || r.w > h->rows || (h->windowed && ((r.x | r.z) & 3)) || !d_payload)
        return fail(h, RBS_ERR_INVALID_ARGUMENT, fmt("import_window: bad rectangle (%d, %d, %d, %d)", rect[0], rect[1], rect[2], rect[3]));
    const int w = r.z - r.x, hh = r.w - r.y;
    const float* payload = static_cast<const float*>(d_payload);
    if ((h->stp && h->slab_px) || h->exact) {
        // the sender's plane = its scalar background outside rect: assembled whole beside the slabs, stored like any plane handed in
        if (int32_t rc = fill_and_paste(h, h->d_render, r, payload, s)) return rc;
        return store_plane(h, slot, h->d_render, s);
    }
    if (!h->windowed || h->stp) {
        // whole planes without windows (or a handle whose implicit background is a plane of its own): the sender's scalar
        // background has to be written out
        if (int32_t rc = fill_and_paste(h, slot_base(h, slot), r, payload, s)) return rc;
        return h->stp ? set_window(h, h->d_win[h->cur], slot, window_full(h), s) : RBS_OK;
    }
    if (h->slab_px) {
        // a window handed in from a handle whose slabs have already grown: the slabs grow here as they do behind rbs_import_plane /
        // rbs_set_occlusion (the slot's address is taken afterwards)
        if (!empty) {
            const std::string what = fmt("import_window: a window of %d x %d values", w, hh);
            if (int32_t rc = fit_or_grow(h, (long)w * hh, s, what, what)) return rc;
            // the slot's stored region becomes the window itself, packed
            RBS_HIP(h, hipMemcpyAsync(slot_base(h, slot), payload, sizeof(float) * (size_t)w * (size_t)hh, hipMemcpyDeviceToDevice, s));
        }
        if (int32_t rc = set_window(h, h->d_reg[h->cur], slot, r, s)) return rc;
    } else if (!empty) {
        if (int32_t rc = copy_window(h, slot_base(h, slot) + (size_t)r.y * h->cols + r.x, (size_t)h->cols, payload, (size_t)w, w, hh, s)) return rc;
    }
    return set_window(h, h->d_win[h->cur], slot, r, s);
}

int32_t rbs_get_window(rbs_handle* h, int32_t slot, int32_t out[4])
{
    if (!h) return RBS_ERR_INVALID_ARGUMENT;
    RBS_GROUP_SLOT(h, slot, rbs_get_window(sh_, l_, out));
    if (int32_t rc = slot_enter(h, "get_window", slot, out)) return rc;
    if (int32_t rc = drain(h, true)) return rc;
    RBS_HIP(h, hipMemcpy(out, h->d_win[h->cur] + slot, sizeof(int32_t) * 4, hipMemcpyDeviceToHost));
    return RBS_OK;
}
