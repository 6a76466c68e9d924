// The image atlas: resizing it, host uploads through pinned staging blocks and device-to-atlas copies, all on the upload stream.
#include <cstring>
#include <map>
#include <utility>

#include "ctx.h"

using namespace vk;

namespace {

// waits for the atlas uploads still in flight (before the atlas is freed / resized / the context goes away)
int sync_uploads(vello_hip_ctx *c) {
    if (c->upload_stream) HIP_TRY(c, hipStreamSynchronize(c->upload_stream));
    // (a block that carries a lane's instance table is released by its own event: the lane's stream is not waited for here)
    for (auto &st : c->staging)
        if (st.busy && hipEventQuery(st.done) == hipSuccess) st.busy = false;
    return 0;
}

// the upload stream and its events (created on first use)
int ensure_upload_stream(vello_hip_ctx *c) {
    if (c->upload_stream) return 0;
    HIP_TRY(c, hipStreamCreateWithFlags(&c->upload_stream, hipStreamNonBlocking));
    HIP_TRY(c, hipEventCreateWithFlags(&c->atlas_ready, hipEventDisableTiming));
    HIP_TRY(c, hipEventCreateWithFlags(&c->lane_mark, hipEventDisableTiming));
    return 0;
}

// frames already enqueued may sample the texels an upload replaces: it runs behind all of them
int upload_behind_frames(vello_hip_ctx *c) {
    for (auto &l : c->lanes) {
        if (!l.stream || !l.used) continue;
        HIP_TRY(c, hipEventRecord(c->lane_mark, l.stream));
        HIP_TRY(c, hipStreamWaitEvent(c->upload_stream, c->lane_mark, 0));
    }
    return 0;
}

}  // namespace

namespace vk {

// a pinned block of >= bytes that no DMA is reading
int acquire_staging(vello_hip_ctx *c, size_t bytes, Staging *&out) {
    size_t held = 0;
    for (auto &st : c->staging) {
        if (st.busy && hipEventQuery(st.done) == hipSuccess) st.busy = false;
        held += st.size;
    }
    for (auto &st : c->staging)
        if (!st.busy && st.size >= bytes) {
            out = &st;
            return 0;
        }
    if (held > ((size_t)256 << 20)) {  // bound the pinned memory: drain and start over
        int r = sync_uploads(c);
        if (r) return r;
        if ((r = sync_all(c))) return r;  // (instance tables are copied on the lanes' streams)
        c->staging.clear();
    }
    Staging st;
    st.size = bytes < ((size_t)1 << 16) ? ((size_t)1 << 16) : bytes;
    HIP_TRY(c, hipHostMalloc(&st.host, st.size, hipHostMallocDefault));
    HIP_TRY(c, hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
    c->staging.push_back(std::move(st));
    out = &c->staging.back();
    return 0;
}

}  // namespace vk

extern "C" {

int vello_hip_resize_image_atlas(vello_hip_ctx *c, uint32_t width, uint32_t height) {
    if (!c || width > 0xffffu || height > 0xffffu) return VELLO_HIP_E_INVALID;  // DrawImage packs xy / extents in 16 bits
    HIP_TRY(c, hipSetDevice(c->device));
    int r = sync_all(c);
    if (r) return r;
    if ((r = sync_uploads(c))) return r;
    c->atlas_w = c->atlas_h = 0;
    if (width == 0 || height == 0) return VELLO_HIP_OK;
    size_t bytes = (size_t)width * height * 4u;
    if ((r = ensure(c, c->atlas, bytes))) return r;
    // Every writer of the atlas is ordered on the upload stream: hipMemset on the null stream is asynchronous to the host
    // for device memory and the (non-blocking) upload stream does not synchronise with it, so a clear issued there could
    // land AFTER the uploads that follow this call.  Frames wait for `atlas_ready` like they do after an upload.
    if ((r = ensure_upload_stream(c))) return r;
    HIP_TRY(c, hipMemsetAsync(c->atlas.ptr, 0, bytes, c->upload_stream));
    HIP_TRY(c, hipEventRecord(c->atlas_ready, c->upload_stream));
    c->atlas_epoch += 1u;
    c->atlas_w = width;
    c->atlas_h = height;
    return VELLO_HIP_OK;
}

int vello_hip_write_image(vello_hip_ctx *c, uint32_t x, uint32_t y, uint32_t width, uint32_t height, const uint8_t *rgba8,
                          size_t stride) {
    if (!c || !rgba8) return VELLO_HIP_E_INVALID;
    if ((uint64_t)x + width > c->atlas_w || (uint64_t)y + height > c->atlas_h) {
        c->last_error = "write_image outside the atlas";
        return VELLO_HIP_E_INVALID;
    }
    if (width == 0 || height == 0) return VELLO_HIP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    if (stride == 0) stride = (size_t)width * 4u;
    int r = ensure_upload_stream(c);
    if (r) return r;
    // the caller owns the pixels only for the duration of the call: into pinned memory now, DMA later
    const size_t row_bytes = (size_t)width * 4u;
    Staging *st = nullptr;
    if ((r = acquire_staging(c, row_bytes * height, st))) return r;
    for (uint32_t row = 0; row < height; row++) std::memcpy((char *)st->host + row * row_bytes, rgba8 + row * stride, row_bytes);
    if ((r = upload_behind_frames(c))) return r;
    HIP_TRY(c, hipMemcpy2DAsync((char *)c->atlas.ptr + ((size_t)y * c->atlas_w + x) * 4u, (size_t)c->atlas_w * 4u, st->host, row_bytes,
                                row_bytes, height, hipMemcpyHostToDevice, c->upload_stream));
    HIP_TRY(c, hipEventRecord(st->done, c->upload_stream));
    st->busy = true;
    // ... and every frame enqueued from here on runs behind it (prepare_frame)
    HIP_TRY(c, hipEventRecord(c->atlas_ready, c->upload_stream));
    c->atlas_epoch += 1u;
    return VELLO_HIP_OK;
}

int vello_hip_copy_images_device(vello_hip_ctx *c, const vello_hip_image_copy *copies, uint32_t n, void *src_stream) {
    if (!c) return VELLO_HIP_E_INVALID;
    if (n > 0u && !copies) {
        c->last_error = "copy_images_device: copies is NULL";
        return VELLO_HIP_E_INVALID;
    }
    // every rectangle is checked before anything is enqueued
    uint64_t total = 0;
    uint32_t m = 0;
#ifndef VELLO_SIMT_EMU
    std::map<uint64_t, uint64_t> checked;  // allocations found to be device memory of this device: base -> end
#endif
    for (uint32_t i = 0; i < n; i++) {
        const vello_hip_image_copy &cp = copies[i];
        if (cp.width == 0u || cp.height == 0u) continue;
        const std::string which = "copy_images_device: rectangle " + std::to_string(i);
        if ((uint64_t)cp.x + cp.width > c->atlas_w || (uint64_t)cp.y + cp.height > c->atlas_h) {
            c->last_error = which + " outside the atlas";
            return VELLO_HIP_E_INVALID;
        }
        const uint64_t stride = cp.src_stride ? cp.src_stride : (uint64_t)cp.width * 4u;
        if (cp.src == 0u || ((cp.src | stride) & 3u) != 0u) {
            c->last_error = which + (cp.src ? ": source address or row stride not a multiple of 4" : ": null source");
            return VELLO_HIP_E_INVALID;
        }
#ifndef VELLO_SIMT_EMU
        // every byte the rectangle reads lies in ONE allocation in device memory of this context's device (peer sources are not
        // taken); one runtime query per allocation, not per rectangle: a thousand sprites carved from one tensor cost one
        const uint64_t last = cp.src + (uint64_t)(cp.height - 1u) * stride + (uint64_t)cp.width * 4u - 1u;
        auto known = checked.upper_bound(cp.src);
        if (known == checked.begin() || (--known, last >= known->second)) {
            hipDeviceptr_t base = nullptr;
            size_t size = 0;
            hipPointerAttribute_t attr{};
            hipError_t e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)(uintptr_t)cp.src);
            if (e == hipSuccess) e = hipPointerGetAttributes(&attr, base);
            (void)hipGetLastError();  // a host address is an error here: do not leave it for the caller's next launch check
            const uint64_t b = (uint64_t)(uintptr_t)base;
            if (e != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != c->device || last >= b + size) {
                c->last_error = which + (e == hipSuccess && last >= b + size ? ": source rows run past the end of their allocation"
                                                                              : ": source is not device memory of device " + std::to_string(c->device));
                return VELLO_HIP_E_INVALID;
            }
            checked[b] = b + size;
        }
#endif
        total += (uint64_t)cp.width * cp.height;
        m++;
    }
    if (m == 0u) return VELLO_HIP_OK;
    if (total > ((uint64_t)1 << 40)) {  // (k_atlas_copy's grid is a 32-bit count of 4 096-texel chunks)
        c->last_error = "copy_images_device: more than 2^40 texels in one batch";
        return VELLO_HIP_E_INVALID;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    int r = ensure_upload_stream(c);
    if (r) return r;
    const size_t table_bytes = (size_t)m * sizeof(AtlasCopyDesc);
    Staging *st = nullptr;
    if ((r = acquire_staging(c, table_bytes, st))) return r;
    // (ensure() replaces a table too small with hipFree + hipMalloc; hipFree waits for the copies still reading the old one)
    if ((r = ensure(c, c->copy_descs, table_bytes))) return r;
    AtlasCopyDesc *table = (AtlasCopyDesc *)st->host;
    uint64_t first = 0;
    for (uint32_t i = 0, k = 0; i < n; i++) {
        const vello_hip_image_copy &cp = copies[i];
        if (cp.width == 0u || cp.height == 0u) continue;
        table[k++] = AtlasCopyDesc{cp.src, cp.src_stride ? cp.src_stride : (uint64_t)cp.width * 4u, (uint64_t)cp.y * c->atlas_w + cp.x, first,
                                   cp.width, cp.height};
        first += (uint64_t)cp.width * cp.height;
    }
    // behind the frames already enqueued, as write_image ...
    if ((r = upload_behind_frames(c))) return r;
    // ... and behind the caller's work that produced the sources
    if (src_stream) {
        HIP_TRY(c, hipEventRecord(c->lane_mark, (hipStream_t)src_stream));
        HIP_TRY(c, hipStreamWaitEvent(c->upload_stream, c->lane_mark, 0));
    }
    HIP_TRY(c, hipMemcpyAsync(c->copy_descs.ptr, st->host, table_bytes, hipMemcpyHostToDevice, c->upload_stream));
    HIP_TRY(c, hipEventRecord(st->done, c->upload_stream));
    st->busy = true;
    launch_atlas_copy((const AtlasCopyDesc *)c->copy_descs.ptr, m, total, (uint32_t *)c->atlas.ptr, c->atlas_w, c->upload_stream);
    HIP_TRY(c, hipGetLastError());
    // every frame enqueued from here on runs behind the copy (prepare_frame), and so does the caller's later work on src_stream
    HIP_TRY(c, hipEventRecord(c->atlas_ready, c->upload_stream));
    c->atlas_epoch += 1u;
    if (src_stream) HIP_TRY(c, hipStreamWaitEvent((hipStream_t)src_stream, c->atlas_ready, 0));
    return VELLO_HIP_OK;
}

}  // extern "C"
