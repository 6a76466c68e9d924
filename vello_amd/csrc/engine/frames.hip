// Frames: from render parameters to the launch sequence of one frame on one lane, and the entry points that render and wait.
#include <cstdio>
#include <cstring>

#include "ctx.h"

using namespace vk;

namespace {

// RenderConfig::new + BufferSizes::new, vello_encoding/src/config.rs:168-196, :363-435
int configure(vello_hip_ctx *c, const SceneSlot &sc, const vello_hip_render_params *p, Config &cfg) {
    if (!p || p->width == 0 || p->height == 0 || p->aa > VELLO_HIP_AA_MSAA16) {
        c->last_error = "invalid render params";
        return VELLO_HIP_E_INVALID;
    }
    if (((c->aa_mask >> p->aa) & 1u) == 0u) {
        // render.rs:566-568, :593-598: "shaders not configured to support AA mode"
        c->last_error = "AA mode was not enabled in vello_hip_create(aa_mask)";
        return VELLO_HIP_E_INVALID;
    }
    if (p->width > 0xffffu * TILE_WIDTH || p->height > 0xffffu * TILE_HEIGHT) {
        c->last_error = "target larger than 65535 tiles in one dimension";  // coarse packs tile coordinates in 16 bits
        return VELLO_HIP_E_INVALID;
    }
    std::memset(&cfg, 0, sizeof cfg);
    cfg.width_in_tiles = align_up(p->width, TILE_WIDTH) / TILE_WIDTH;
    cfg.height_in_tiles = align_up(p->height, TILE_HEIGHT) / TILE_HEIGHT;
    cfg.target_width = p->width;
    cfg.target_height = p->height;
    cfg.base_color = p->base_color;
    std::memcpy(&cfg.layout, &sc.layout, sizeof(Layout));
    uint32_t bin_data = c->caps.bin_data;
    if (bin_data <= sc.layout.bin_data_start) {
        c->last_error = "bin_data capacity smaller than the scene's info words";
        return VELLO_HIP_E_INVALID;
    }
    cfg.lines_size = c->caps.lines;
    cfg.binning_size = bin_data - sc.layout.bin_data_start;
    cfg.tiles_size = c->caps.tiles;
    cfg.seg_counts_size = c->caps.seg_counts;
    cfg.segments_size = c->caps.segments;
    cfg.blend_size = c->caps.blend_spill;
    cfg.ptcl_size = c->caps.ptcl;
    uint64_t initial_ptcl = (uint64_t)cfg.width_in_tiles * cfg.height_in_tiles * PTCL_INITIAL_ALLOC;
    if (initial_ptcl + PTCL_INCREMENT > cfg.ptcl_size) {
        c->last_error = "ptcl capacity smaller than the fixed per-tile allocation";
        return VELLO_HIP_E_INVALID;
    }
    return 0;
}

// R of a frame of these parameters enqueued now: the context's damage rectangle cut to the target (off: the whole target)
PixelRect damage_of(const vello_hip_ctx *c, const vello_hip_render_params *p) {
    if (!c->has_damage) return PixelRect{0u, 0u, p->width, p->height};
    const auto cut = [](uint32_t v, uint32_t hi) { return v < hi ? v : hi; };
    return PixelRect{cut(c->damage[0], p->width), cut(c->damage[1], p->height), cut(c->damage[2], p->width), cut(c->damage[3], p->height)};
}

// k_front's grid-barrier counter (Lane::front_sync) only ever grows, and the host keeps its value: a launch's barriers wait for
// sync_base + k * (its workgroups).  The two must never drift apart: if a launch is rejected the device never adds, if a
// barrier's spin bound trips the workgroups stop waiting -- either way the counter goes back to zero on the lane's stream, behind
// whatever was enqueued, and the host's copy with it.
void reset_front_sync(Lane &l, hipStream_t st) {
    if (l.front_sync.ptr) (void)hipMemsetAsync(l.front_sync.ptr, 0, 256, st);
    l.front_sync_value = 0u;
}
// After a k_front launch: the host's copy of the counter advances only once the launch was accepted.
int front_accepted(vello_hip_ctx *c, Lane &l, hipStream_t st, uint32_t add) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        reset_front_sync(l, st);
        c->last_error = std::string("k_front launch: ") + hipGetErrorString(e);
        return VELLO_HIP_E_HIP;
    }
    l.front_sync_value += add;
    c->fused_launches++;
    return 0;
}

// What a finished frame (one that did not fail, and whose flatten ran to its end) teaches about the scene it rendered
void learn_from_frame(SceneSlot &sc, const Control &ctl, const Lane &l) {
    sc.stroke_lines = (int64_t)ctl.heavy_count[2];
    sc.heavy_curves = (int64_t)ctl.heavy_count[0];
    sc.heavy_strokes = (int64_t)ctl.heavy_count[1];
    sc.soup_lines = (int64_t)ctl.bump.lines;
    // (a damaged frame cut only its window's tiles into slices: its count says nothing about the whole frame, and must not turn
    // "unknown" into a small number that costs the next whole frame its slice blocks)
    if (l.slices_on && !l.frame_damaged && (int64_t)ctl.slice_items > sc.slice_demand) sc.slice_demand = (int64_t)ctl.slice_items;
}

// bump.failed of ONE lane's latest frame -> error code.  Failures are per frame: vello_hip_render judges the lane that
// rendered its frame, vello_hip_sync the lanes of the current rotation, and vello_hip_grow_pools voids the frames that
// overflowed the old pools (l.used) -- so a retry on another lane is not failed by the lane that overflowed.
int check_lane(vello_hip_ctx *c, Lane &l) {
    if (!l.used || !l.zero_region.ptr) return VELLO_HIP_OK;
    Control ctl;
    HIP_TRY(c, hipMemcpy(&ctl, l.zero_region.ptr, sizeof ctl, hipMemcpyDeviceToHost));
    vello_hip_bump b;
    std::memcpy(&b, &ctl.bump, sizeof b);
    if (b.failed == 0u) {
        SceneSlot &sc = slot_of(c, l);
        if (l.flatten_ran && l.frame_generation == sc.generation) learn_from_frame(sc, ctl, l);  // (flatten ran to its end)
        return VELLO_HIP_OK;
    }
    if ((b.failed & FAILED_SCENE) != 0u) {
        c->last_error = "the path tag stream needs more path data, transforms or styles than the scene buffer holds";
        return VELLO_HIP_E_INVALID;
    }
    if ((b.failed & FAILED_INTERNAL) != 0u) {
        // a spin bound tripped (lookback.h, k_front's barrier): not a pool overflow -- growing pools would not help.  The lane is idle
        // here (the caller waited for it): its barrier counter starts over.
        reset_front_sync(l, l.stream);
        (void)hipStreamSynchronize(l.stream);
        c->last_error = "an engine-internal wait gave up (bump.failed bit 31): the frame is discarded";
        return VELLO_HIP_E_INTERNAL;
    }
    char msg[160];
    std::snprintf(msg, sizeof msg, "bump.failed=0x%x (lines %u, binning %u, tile %u, seg_counts %u, segments %u, ptcl %u)", b.failed,
                  b.lines, b.binning, b.tile, b.seg_counts, b.segments, b.ptcl);
    c->last_error = msg;
    return VELLO_HIP_E_CAPACITY;
}

}  // namespace

namespace vk {

// Where entry 0 of lane l's copy of the transform words lies, in words from the scene's start (SceneSlot::view_at; six words into
// the copy: slot -1 comes first).  VELLO_HIP_E_INVALID for a scene so large that the copy is out of a u32 offset's reach.  The entry
// points that rotate the lanes ask before they rotate, so that a refused frame leaves the rotation where it was.
int view_base(vello_hip_ctx *c, const SceneSlot &sc, const Lane &l, uint32_t &base) {
    const size_t set = l.which == LaneScene::Own ? 0u : (size_t)(&l - c->lanes.data());
    const uint64_t at = (uint64_t)sc.view_at + (uint64_t)set * sc.view_set_words + 6u;
    if (set >= sc.view_sets || at + sc.view_set_words > 0xffffffffull) {
        c->last_error = "the scene is too large for a view transform (its transform words must lie within 2^32 words of its start)";
        return VELLO_HIP_E_INVALID;
    }
    base = (uint32_t)at;
    return 0;
}

// Where lane l's copy of the retained list's draw-data words lies, in words from the scene's start (SceneSlot::dd_at): what a
// painted retained frame reads in the stream's place.  VELLO_HIP_E_INVALID for a list so large that the copies are out of a u32
// offset's reach (it was given none); asked before the rotation moves, as view_base is.
int paint_base(vello_hip_ctx *c, const SceneSlot &sc, const Lane &l, uint32_t &base) {
    const size_t set = (size_t)(&l - c->lanes.data());
    const uint64_t at = (uint64_t)sc.dd_at + (uint64_t)set * sc.dd_set_words;
    if (set >= sc.dd_sets || at + sc.dd_set_words > 0xffffffffull) {
        c->last_error = "the retained list is too large for per-frame paints (its bytes and copies must lie within 2^32 words of its start)";
        return VELLO_HIP_E_INVALID;
    }
    base = (uint32_t)at;
    return 0;
}

// Where lane l's copy of the shared scene's path-data words lies, in words from the scene's start (SceneSlot::pd_at): what a morphed
// frame reads in the stream's place.  VELLO_HIP_E_INVALID while the slot has no room for the copies (ensure_morph_room makes it).
int morph_base(vello_hip_ctx *c, const SceneSlot &sc, const Lane &l, uint32_t &base) {
    const size_t set = (size_t)(&l - c->lanes.data());
    const uint64_t at = (uint64_t)sc.pd_at + (uint64_t)set * sc.pd_set_words;
    if (set >= sc.pd_sets || at + sc.pd_set_words > 0xffffffffull) {
        c->last_error = "the scene has no room for per-frame path data (its bytes and copies must lie within 2^32 words of its start)";
        return VELLO_HIP_E_INVALID;
    }
    base = (uint32_t)at;
    return 0;
}

// Where entry 0 of lane l's copy of the style words lies, in words from the scene's start (SceneSlot::st_at; two words into the
// copy: slot -1 comes first): what a frame with a stroke scale reads in the stream's place.  VELLO_HIP_E_INVALID for a scene so
// large that the copy is out of a u32 offset's reach; asked before the rotation moves, as view_base is.
int style_base(vello_hip_ctx *c, const SceneSlot &sc, const Lane &l, uint32_t &base) {
    const size_t set = l.which == LaneScene::Own ? 0u : (size_t)(&l - c->lanes.data());
    const uint64_t at = (uint64_t)sc.st_at + (uint64_t)set * sc.st_set_words + 2u;
    if (set >= sc.st_sets || at + sc.st_set_words > 0xffffffffull) {
        c->last_error = "the scene is too large for a stroke scale (its bytes and copies must lie within 2^32 words of its start)";
        return VELLO_HIP_E_INVALID;
    }
    base = (uint32_t)at;
    return 0;
}

// The target contract of include/vello_hip.h (at vello_hip_render_resident).  fine stores dwords at output + y * stride and takes the
// stride as a u32: a device target that is not 4-aligned, rows that overlap or a stride of 2^32 and more would corrupt silently.
// Every entry point that takes a target asks before it uploads, rotates or enqueues anything.
int check_target(vello_hip_ctx *c, const vello_hip_render_params *p, const void *out, size_t out_stride, bool device) {
    if (!out || !p) return VELLO_HIP_OK;
    const uint64_t row = (uint64_t)p->width * 4u;
    const char *why = nullptr;
    if (out_stride != 0u && out_stride < row) why = "out_stride is below width * 4";
    else if (device && (uint64_t)row_stride(p, out_stride) > 0xffffffffull) why = "the row stride of a device target must be below 2^32";
    else if (device && (out_stride & 3u) != 0u) why = "out_stride of a device target is not a multiple of 4";
    else if (device && (reinterpret_cast<uintptr_t>(out) & 3u) != 0u) why = "the address of a device target is not a multiple of 4";
    if (!why) return VELLO_HIP_OK;
    c->last_error = std::string("target refused: ") + why;
    return VELLO_HIP_E_INVALID;
}

// The enqueue-time rules of vello_hip_set_base_image for a frame of these parameters and this device target (null: the lane's internal
// target, which is no caller's memory).  Asked before the frame's entry point uploads, rotates or enqueues anything; nothing to ask
// without an image.  The allocation is asked about once per setting and extent (vello_hip_ctx::base_checked).
int check_base_image(vello_hip_ctx *c, const vello_hip_render_params *p, const void *out, size_t out_stride) {
    if (!c->base_image || !p || p->width == 0u || p->height == 0u) return VELLO_HIP_OK;
    const auto refuse = [&](const std::string &why) {
        c->last_error = "base image refused: " + why;
        return VELLO_HIP_E_INVALID;
    };
    const uint64_t row = (uint64_t)p->width * 4u;
    const uint64_t stride = c->base_stride ? (uint64_t)c->base_stride : row;
    if (stride < row) return refuse("its stride is below width * 4 of the frame");
    const uint64_t bytes = (uint64_t)(p->height - 1u) * stride + row;
    if (bytes > c->base_checked) {
        if (const char *why = not_device_memory(c, c->base_image, (size_t)bytes)) return refuse(std::string("its address ") + why);
        c->base_checked = bytes;
    }
    if (out) {
        // in place -- the image IS the target: same address, same effective stride -- or apart; nothing in between: a pixel's word
        // must not be another pixel's output
        const uint64_t ostride = (uint64_t)row_stride(p, out_stride);
        const uint64_t a0 = (uint64_t)reinterpret_cast<uintptr_t>(c->base_image), a1 = a0 + bytes;
        const uint64_t b0 = (uint64_t)reinterpret_cast<uintptr_t>(out), b1 = b0 + (uint64_t)(p->height - 1u) * ostride + row;
        if (a0 < b1 && b0 < a1 && !(a0 == b0 && stride == ostride))
            return refuse("its bytes overlap the target's without being the target (same address and stride)");
    }
    return VELLO_HIP_OK;
}

int prepare_frame(vello_hip_ctx *c, Lane &l, const vello_hip_render_params *p, void *out_device, size_t out_stride, Frame &f,
                  bool upload_cfg) {
    const SceneSlot &sc = slot_of(c, l);
    if (!sc.resident) {
        c->last_error = "no scene uploaded";
        return VELLO_HIP_E_INVALID;
    }
    int r;
    if (c->auto_grow && p && p->width && p->height) {
        // robust mode: a target with more tiles than the PTCL pool's fixed 64 words per tile (config.rs:408 sizes it for
        // ~1 Mpx) grows the pool instead of failing; the info words of the scene likewise must fit bin_data
        uint64_t tiles_xy = (uint64_t)(align_up(p->width, TILE_WIDTH) / TILE_WIDTH) * (align_up(p->height, TILE_HEIGHT) / TILE_HEIGHT);
        uint64_t need_ptcl = tiles_xy * PTCL_INITIAL_ALLOC + 64u * PTCL_INCREMENT;
        uint64_t need_bin = (uint64_t)sc.layout.bin_data_start + (1u << 16);
        if (need_ptcl > c->caps.ptcl || need_bin > c->caps.bin_data) {
            if (need_ptcl > 0xffff0000ull || need_bin > 0xffff0000ull) {
                c->last_error = "target / scene too large for 32-bit pool offsets";
                return VELLO_HIP_E_INVALID;
            }
            if ((r = sync_all(c))) return r;
            vello_hip_capacities d = c->caps;
            if (need_ptcl > d.ptcl) d.ptcl = (uint32_t)(need_ptcl + need_ptcl / 4u);
            if (need_bin > d.bin_data) d.bin_data = (uint32_t)(need_bin + need_bin / 4u);
            if ((r = commit_caps(c, d))) return r;
        }
    }
    r = configure(c, sc, p, f.cfg);
    if (r) return r;
    c->cfg = f.cfg;
    c->have_cfg = true;
    // size-dependent buffers
    uint32_t wb = (f.cfg.width_in_tiles + 15u) / 16u, hb = (f.cfg.height_in_tiles + 15u) / 16u;
    uint32_t aligned_n_bins = align_up(wb * hb, 256u);
    uint32_t binning_wgs = (sc.layout.n_draw_objects + DRAW_WG - 1u) / DRAW_WG;
    if ((r = ensure(c, l.buf[VELLO_HIP_BUF_BIN_HEADERS], (size_t)(binning_wgs * aligned_n_bins + 1u) * sizeof(BinHeader)))) return r;
    if (!out_device && (r = ensure(c, l.buf[VELLO_HIP_BUF_OUTPUT], (size_t)p->width * p->height * 4u))) return r;
    if ((r = ensure(c, l.tile_order, (size_t)f.cfg.width_in_tiles * f.cfg.height_in_tiles * FINE_WORK_BUCKETS * 4u))) return r;
    // fine launches one (at once exiting) workgroup per slice item it MIGHT be given in front of the tiles' workgroups:
    // as many as the scene asked for in an earlier frame (+ 1/8), a quarter of the tiles while that is unknown.  Coarse
    // cuts a tile into slices only if its items fit (the rest are rendered unsliced), so any number is correct.
    const uint32_t n_tiles_target = f.cfg.width_in_tiles * f.cfg.height_in_tiles;
    if ((r = ensure(c, l.slice_items, (size_t)n_tiles_target * sizeof(SliceItem)))) return r;
    if ((r = ensure(c, l.slice_counters, (size_t)n_tiles_target * 4u))) return r;
    {
        uint64_t want = sc.slice_demand < 0 ? n_tiles_target / 4u : (uint64_t)sc.slice_demand + (uint64_t)sc.slice_demand / 8u + 16u;
        if (want < 64u) want = 64u;
        f.slice_cap = want > n_tiles_target ? n_tiles_target : (uint32_t)want;
    }
    // kernels take the ConfigUniform by value (kernarg); the device copy only serves the test seam
    if (upload_cfg) {
        HIP_TRY(c, hipMemcpy(c->config.ptr, &f.cfg, sizeof(Config), hipMemcpyHostToDevice));
        c->cfg_unsent = false;
    }
    f.n_tag_words = sc.n_tag_words;
    f.n_scene_words = (uint32_t)(sc.scene_len / 4u);
    f.aa = p->aa;
    f.scene = (const uint32_t *)sc.scene.ptr;
    f.has_view = c->has_view;
    f.view = c->view;
    f.xf_base = sc.layout.transform_base;
    // a frame of the retained list reads its lane's copy whether a view is set or not; its poses are the lane's (the entry point
    // has set them; vello_hip_run_stages picks its own)
    f.retained = &sc == &c->retained;
    if ((f.has_view || f.retained) && (r = view_base(c, sc, l, f.xf_base))) return r;
    f.xf_owner = f.retained ? (const uint32_t *)c->retained_owner.ptr : nullptr;
    f.pose_words = f.retained ? (l.pose_src ? l.pose_src : (const uint32_t *)c->retained_rest.ptr) : nullptr;
    f.n_instances = f.retained ? c->retained_n : 0u;
    f.pose_stream = f.retained ? l.pose_stream : nullptr;
    f.pose_mark = c->pose_mark;
    f.pose_check = f.retained && l.pose_check;
    // its draw-data words: the retained stream's -- or, a painted frame's (the entry point has set the lane's paint source) and a
    // vello_hip_run_stages' after one (the lane's copy holds that frame's words), the lane's copy
    f.dd_base = sc.layout.draw_data_base;
    f.dd_map = nullptr;
    f.paint_words = nullptr;
    f.paint_check = false;
    if (f.retained && (l.paint_src || l.painted_generation == sc.generation)) {
        if ((r = paint_base(c, sc, l, f.dd_base))) return r;
        f.dd_map = (const uint32_t *)c->retained_ddmap.ptr;
        f.paint_words = l.paint_src;
        f.paint_check = l.paint_src && l.paint_check;
    }
    // its path-data words: the scene's own -- or, a morphed frame's (the entry point has set the lane's sources) and a
    // vello_hip_run_stages' after one (the lane's copy holds that frame's words), the lane's copy
    f.pd_base = sc.layout.path_data_base;
    f.pd_a = f.pd_b = nullptr;
    f.pd_mode = PATH_BLEND_COPY_A;
    f.pd_t = 0.0f;
    f.pd_stream = nullptr;
    if (&sc == &c->shared && (l.pd_a || (l.morphed_generation == sc.generation && sc.pd_sets != 0u))) {
        if ((r = morph_base(c, sc, l, f.pd_base))) return r;
        f.pd_a = l.pd_a;
        f.pd_b = l.pd_b;
        f.pd_mode = l.pd_mode;
        f.pd_t = l.pd_t;
        f.pd_stream = l.pd_stream;
    }
    // its style words: the scene's own -- or, with a stroke scale, the lane's copy, which k_style_widths fills at the head of the
    // frame (a scene without a style entry keeps its own stream: nothing would fill the copy, and no tag reads a style word)
    f.has_stroke = c->has_stroke;
    f.stroke_scale = c->stroke_scale;
    f.stroke_min = c->stroke_min;
    f.st_base = sc.layout.style_base;
    if (f.has_stroke) {
        uint32_t at;
        if ((r = style_base(c, sc, l, at))) return r;
        if ((f.n_scene_words - sc.layout.style_base) / STYLE_SIZE_IN_WORDS != 0u) f.st_base = at;
        // Rule 4 of the contract says what VELLO_HIP_BUF_CONFIG shows behind such a frame: the scene's own layout.  An entry point that
        // enqueues without the blocking copy (vello_hip_render_resident among them, which marks nothing on its own) would leave
        // the device copy as an earlier frame or no frame left it, so the frame's Config is marked for sending when the buffer
        // is next read or written, as the composed, retained and morphed entry points mark theirs.  (f.cfg never carries st_base.)
        if (!upload_cfg) c->cfg_unsent = true;
    }
    f.control = (Control *)l.zero_region.ptr;
    f.zero_bytes = (uint32_t)sc.zero_bytes;
    f.front_sync = (uint32_t *)l.front_sync.ptr;
    f.pathtag_state = (unsigned long long *)((char *)l.zero_region.ptr + sizeof(Control));
    f.draw_state = f.pathtag_state + (size_t)sc.n_pathtag_parts * 10u;
    f.tag_monoids = (TagMonoid *)l.buf[VELLO_HIP_BUF_TAG_MONOIDS].ptr;
    // a frame of the shared scene with an index (built by its upload; VELLO_HIP_DEBUG_NO_SCENE_INDEX: today's per-frame path): the
    // scan's output and flatten's two stroke lists are the index's, read by every lane
    const SceneIndex &ix = sc.index;
    f.indexed = &sc == &c->shared && ix.valid && (c->debug_flags & VELLO_HIP_DEBUG_NO_SCENE_INDEX) == 0u;
    f.index_bboxes = f.indexed ? (const PathBbox *)ix.bboxes.ptr : nullptr;
    f.index_lists = f.indexed ? (const uint32_t *)ix.lists.ptr : nullptr;
    f.index_n_fill = f.indexed ? ix.n_fill : 0u;
    f.index_n_strokes = f.indexed ? ix.n_strokes : 0u;
    f.index_n_lines = f.indexed ? ix.n_lines : 0u;
    f.index_failed = f.indexed ? ix.failed : 0u;
    if (f.indexed) f.tag_monoids = (TagMonoid *)ix.monoids.ptr;
    l.frame_indexed = f.indexed;
    f.path_bboxes = (PathBbox *)l.buf[VELLO_HIP_BUF_PATH_BBOXES].ptr;
    f.lines = (LineSoup *)l.buf[VELLO_HIP_BUF_LINES].ptr;
    f.draw_monoids = (DrawMonoid *)l.buf[VELLO_HIP_BUF_DRAW_MONOIDS].ptr;
    f.info_bin_data = (uint32_t *)l.buf[VELLO_HIP_BUF_INFO_BIN_DATA].ptr;
    f.clip_inp = (Clip *)l.buf[VELLO_HIP_BUF_CLIP_INP].ptr;
    f.clip_bboxes = (Bbox4 *)l.buf[VELLO_HIP_BUF_CLIP_BBOXES].ptr;
    f.draw_bboxes = (Bbox4 *)l.buf[VELLO_HIP_BUF_DRAW_BBOXES].ptr;
    f.bin_headers = (BinHeader *)l.buf[VELLO_HIP_BUF_BIN_HEADERS].ptr;
    f.paths = (Path *)l.buf[VELLO_HIP_BUF_PATHS].ptr;
    f.tiles = (Tile *)l.buf[VELLO_HIP_BUF_TILES].ptr;
    f.seg_counts = (SegmentCount *)l.buf[VELLO_HIP_BUF_SEG_COUNTS].ptr;
    f.segments = (Segment *)l.buf[VELLO_HIP_BUF_SEGMENTS].ptr;
    f.ptcl = (uint32_t *)l.buf[VELLO_HIP_BUF_PTCL].ptr;
    f.blend_spill = (uint32_t *)l.buf[VELLO_HIP_BUF_BLEND_SPILL].ptr;
    f.clip_stack = (uint32_t *)l.clip_stack.ptr;
    f.coarse_el = (CoarseEl *)l.coarse_el.ptr;
    f.tile_bits = (uint32_t *)l.tile_bits.ptr;
    f.tile_order = (uint32_t *)l.tile_order.ptr;
    f.slice_items = (SliceItem *)l.slice_items.ptr;
    f.slice_counters = (uint32_t *)l.slice_counters.ptr;
    f.cov = (uint32_t *)l.cov.ptr;
    f.cov_cap = cov_cap_words(c->caps, c->aa_mask);
    f.slice_fills = f.slice_min_fills = 0u;
    l.slices_on = p->aa != 0u;
    if (p->aa != 0u) {
        const bool forced = (c->debug_flags & VELLO_HIP_DEBUG_FINE_SLICES) != 0u;
        const bool alone = c->n_active == 1u;
        f.slice_fills = forced ? FINE_SLICE_FILLS_FORCED : (alone ? FINE_SLICE_FILLS : FINE_SLICE_FILLS_IN_FLIGHT);
        f.slice_min_fills = forced ? FINE_SLICE_MIN_FILLS_FORCED : (alone ? FINE_SLICE_MIN_FILLS : FINE_SLICE_MIN_FILLS_IN_FLIGHT);
    }
    f.heavy_list = (uint32_t *)l.heavy_list.ptr;
    f.arc_items = (uint32_t *)l.arc_items.ptr;
    f.output = out_device ? (uint8_t *)out_device : (uint8_t *)l.buf[VELLO_HIP_BUF_OUTPUT].ptr;
    f.out_stride = row_stride(p, out_device ? out_stride : 0u);
    const SceneSlot &rs = sc.composed ? c->shared : sc;  // (a composed scene's draw data holds the library's ramp ids)
    f.ramps = rs.n_ramps ? (const uint32_t *)rs.ramps.ptr : nullptr;
    f.n_ramps = rs.n_ramps;
    f.brushes = sc.brushes || c->force_brushes;
    f.no_cull = (c->debug_flags & VELLO_HIP_DEBUG_NO_CULL) != 0u;
    f.viewport_cull = c->viewport_cull;
    // the damage rectangle, cut to THIS frame's target (off: the whole target)
    f.damage = damage_of(c, p);
    f.damaged = f.damage.x0 != 0u || f.damage.y0 != 0u || f.damage.x1 != p->width || f.damage.y1 != p->height;
    l.frame_damaged = f.damaged;
    // the base image (off: none); the entry point has asked check_base_image
    f.base_image = c->base_image;
    f.base_stride = (uint32_t)(c->base_stride ? c->base_stride : (size_t)p->width * 4u);
    f.base_stream = c->base_image ? c->base_stream : nullptr;
    f.base_event = f.base_stream ? c->base_ready : nullptr;
    f.base_mark = c->base_mark;
    f.sequential_clip = (c->debug_flags & VELLO_HIP_DEBUG_SEQ_CLIP) != 0u;
    f.stroke_kernel_min_lines = (c->debug_flags & VELLO_HIP_DEBUG_STROKE_KERNEL) != 0u ? 0u : FLATTEN_STROKE_KERNEL_MIN_LINES;
    f.path_count_small = sc.soup_lines >= 0 && sc.soup_lines < PATH_COUNT_SMALL_MAX_LINES;
    f.flatten_side_by_side = c->n_active == 1u;
    f.launch_stroke_kernel = sc.stroke_lines < 0 || (uint64_t)sc.stroke_lines >= f.stroke_kernel_min_lines;
    // Which kernels take flatten's heavy list (flatten_walk.inc).  The wave-cooperative walk pays where a lane alone would loop
    // long: a list short enough for a wave per entry (<= 4 096: the tiger's 2 300 curves, a circle's four), or one that is mostly
    // stroked curves (mmark: two offset curves a walk, a dozen lines a turn); the road map's blobs, joins and caps are 10 % faster
    // with every lane on its own and the fp64 routines inline.  Known from a finished frame of the scene; before there is one, by
    // the scene's size.
    {
        bool coop = flatten_n_seg_max(sc.layout, sc.n_tag_words) <= 16384u;
        if (sc.heavy_curves >= 0 && sc.stroke_lines >= 0) {
            const uint64_t nc = (uint64_t)sc.heavy_curves, ns = (uint64_t)sc.heavy_strokes;
            const uint64_t nl = (uint64_t)sc.stroke_lines < f.stroke_kernel_min_lines ? (uint64_t)sc.stroke_lines : 0u;
            const uint64_t n_heavy = nc + ns + nl;
            coop = n_heavy <= 4096u || ns * 2u > n_heavy + nc * 2u;
        }
        if (c->debug_flags & VELLO_HIP_DEBUG_FLATTEN_COOP) coop = true;
        if (c->debug_flags & VELLO_HIP_DEBUG_FLATTEN_ALONE) coop = false;
        f.flatten_coop = coop;
    }
    l.frame_generation = sc.generation;
    l.frame_cfg = f.cfg;
    f.atlas = c->atlas_w ? (const uint32_t *)c->atlas.ptr : nullptr;
    f.atlas_w = c->atlas_w;
    f.atlas_h = c->atlas_h;
    f.mask_lut8 = (const uint32_t *)c->mask8.ptr;
    f.mask_lut16 = (const uint32_t *)c->mask16.ptr;
    if (l.atlas_epoch_seen != c->atlas_epoch) {  // atlas uploads enqueued since this lane's last frame come first
        HIP_TRY(c, hipStreamWaitEvent(l.stream, c->atlas_ready, 0));
        l.atlas_epoch_seen = c->atlas_epoch;
    }
    l.used = true;
    return 0;
}

int run_stage_range(vello_hip_ctx *c, Lane &l, const Frame &f_in, int first, int last) {
    hipStream_t st = l.stream;
    // coarse decides which tiles are cut into slices from the number of slice blocks fine is going to launch: a FINE that
    // runs in a later call than its COARSE (vello_hip_run_stages) launches with the number COARSE was given, whatever
    // the scene's demand is known to be by then
    Frame f = f_in;
    if (first > VELLO_HIP_STAGE_COARSE) {
        if (last >= VELLO_HIP_STAGE_FINE && l.slice_fills_coarse != f.slice_fills) {
            // (coarse's sliced tiles are not in the work buckets: an area-AA fine would never render them)
            c->last_error = "vello_hip_run_stages: fine's AA mode must be of the same kind (area / MSAA) as the one coarse ran with";
            return VELLO_HIP_E_INVALID;
        }
        f.slice_cap = l.slice_cap_coarse;
    } else if (last >= VELLO_HIP_STAGE_COARSE) {
        l.slice_cap_coarse = f.slice_cap;
        l.slice_fills_coarse = f.slice_fills;
    }
    // Small scenes: consecutive stages as one launch (k_front, flatten.hip) -- A: [zero fill | pathtag scan | flatten's light pass
    // + draw scan], B: [binning | tile_alloc]; a scene of a few dozen segments: everything up to tile_alloc.  Not for a stage that
    // is being timed on its own.
    bool fuse_a = false, fuse_b = false, fuse_all = false;
    // Any scene: binning and tile_alloc as one launch (binning.hip k_binning_tile_alloc) when the range holds both and neither is
    // timed on its own
    const bool pair_b = (c->debug_flags & VELLO_HIP_DEBUG_NO_FUSION) == 0u && first <= VELLO_HIP_STAGE_BINNING && last >= VELLO_HIP_STAGE_TILE_ALLOC &&
                        (c->prof_mask & ((1u << VELLO_HIP_STAGE_BINNING) | (1u << VELLO_HIP_STAGE_TILE_ALLOC))) == 0u;
    if ((c->debug_flags & VELLO_HIP_DEBUG_NO_FUSION) == 0u && f.n_tag_words * 4u <= FRONT_MAX_TAGS &&
        f.cfg.layout.n_draw_objects <= FRONT_MAX_DRAW_OBJECTS && f.cfg.layout.n_paths <= FRONT_MAX_DRAW_OBJECTS) {
        const uint32_t pm = c->prof_mask;
        const uint32_t mask_a = (1u << VELLO_HIP_STAGE_PATHTAG_SCAN) | (1u << VELLO_HIP_STAGE_FLATTEN) | (1u << VELLO_HIP_STAGE_DRAW_SCAN);
        const uint32_t mask_b = (1u << VELLO_HIP_STAGE_BINNING) | (1u << VELLO_HIP_STAGE_TILE_ALLOC);
        fuse_a = first == VELLO_HIP_STAGE_PATHTAG_SCAN && last >= VELLO_HIP_STAGE_FLATTEN && (pm & mask_a) == 0u;
        fuse_b = first <= VELLO_HIP_STAGE_BINNING && last >= VELLO_HIP_STAGE_TILE_ALLOC && (pm & mask_b) == 0u;
        // (the heavy list aboard: the kernels of the cooperative walk, no stroke workgroups -- not when a debug flag asks for others)
        fuse_all = fuse_a && fuse_b && (pm & (1u << VELLO_HIP_STAGE_CLIP)) == 0u && f.cfg.layout.n_clips == 0u &&
                   flatten_n_seg_max(f) <= FRONT_TINY_SEGMENTS && f.flatten_coop && f.stroke_kernel_min_lines != 0u;
    }
    // a frame with a view: its transform words first (outside every stage's events), when the range holds a stage that reads them
    if (f.has_view && !f.retained && first <= VELLO_HIP_STAGE_DRAW_SCAN && last >= VELLO_HIP_STAGE_FLATTEN) {
        launch_view_transforms(f, st);
        HIP_TRY(c, hipGetLastError());
    }
    // A frame of the retained list: k_instance_transforms in that kernel's place, view or no view.  Where the poses are the caller's
    // device memory (pose_check; such a frame begins with the pathtag scan) the frame's zero fill comes first, here instead of in
    // that stage, so that the kernel can raise FAILED_SCENE over a pose that is not finite: behind the fill, ahead of the scan
    // (`zeroed`: the stage then neither clears nor has k_front clear).  Poses the host has tested keep the stage's own fill.
    // A painted frame: k_instance_paints beside it, which fills the lane's copy of the draw-data words the draw stage and coarse
    // read; device paints (paint_check) are tested by that kernel the way device poses are, behind the same early zero fill.
    bool zeroed = false;
    if (f.retained && (f.pose_words || f.paint_words) && first <= VELLO_HIP_STAGE_DRAW_SCAN && last >= VELLO_HIP_STAGE_FLATTEN) {
        if ((f.pose_check || f.paint_check) && first == VELLO_HIP_STAGE_PATHTAG_SCAN) {
            HIP_TRY(c, hipMemsetAsync(l.zero_region.ptr, 0, slot_of(c, l).zero_bytes, st));
            zeroed = true;
        }
        if (f.pose_words) {
            launch_instance_transforms(f, zeroed && f.pose_check, st);
            HIP_TRY(c, hipGetLastError());
            l.posed_generation = c->retained.generation;
        }
        if (f.paint_words) {
            launch_instance_paints(f, zeroed && f.paint_check, st);
            HIP_TRY(c, hipGetLastError());
        }
        if (f.pose_stream) {  // the caller's stream may overwrite poses and paints once these kernels have read them
            HIP_TRY(c, hipEventRecord(f.pose_mark, st));
            HIP_TRY(c, hipStreamWaitEvent(f.pose_stream, f.pose_mark, 0));
        }
    }
    // A morphed frame: its path-data words first, beside the view's transform words, when the range holds the stage that reads them;
    // the caller's stream may overwrite its device source once the kernel has read it
    if (f.pd_a && first <= VELLO_HIP_STAGE_FLATTEN && last >= VELLO_HIP_STAGE_FLATTEN) {
        launch_path_blend(f, st);
        HIP_TRY(c, hipGetLastError());
        if (f.pd_stream) {
            HIP_TRY(c, hipEventRecord(f.pose_mark, st));
            HIP_TRY(c, hipStreamWaitEvent(f.pd_stream, f.pose_mark, 0));
        }
    }
    // A frame with a stroke scale: its style words first, beside the view's transform words, when the range holds the stage that
    // reads widths.  (For a composed frame this sits behind k_compose_scene on the lane's stream: the kernel reads the composed
    // style stream; the retained list's is resident.)
    if (styled(f) && first <= VELLO_HIP_STAGE_FLATTEN && last >= VELLO_HIP_STAGE_FLATTEN) {
        launch_style_widths(f, st);
        HIP_TRY(c, hipGetLastError());
    }
    const uint32_t front_zero = zeroed ? 0u : FRONT_ZERO;
    for (int s = first; s <= last; s++) {
        bool prof = ((c->prof_mask >> s) & 1u) != 0u;
        uint32_t front_add = 0u;  // what a k_front launch of this stage adds to the lane's barrier counter (0: one workgroup)
        bool front_launched = false;
        Lane::EvPair ev{s, nullptr, nullptr, {nullptr, nullptr}};
        if (prof) {
            ev.a = get_event(c);
            ev.b = get_event(c);
            if (s == VELLO_HIP_STAGE_FLATTEN || s == VELLO_HIP_STAGE_COARSE) ev.mid[0] = get_event(c);
            if (s == VELLO_HIP_STAGE_FLATTEN) ev.mid[1] = get_event(c);
            HIP_TRY(c, hipEventRecord(ev.a, st));
        }
        switch (s) {
        case VELLO_HIP_STAGE_PATHTAG_SCAN:
            // render.rs:313 clears `bump`; the same memset resets both look-back states and tickets
            l.flatten_ran = false;
            if (fuse_all) {
                front_add = launch_front(f, st, front_zero | FRONT_PATHTAG | FRONT_LIGHT | FRONT_HEAVY | FRONT_BINNING | FRONT_TILE_ALLOC, true, l.front_sync_value);
                front_launched = true;
                break;
            }
            if (fuse_a) break;  // (with FLATTEN's first launch)
            if (f.indexed) {  // (never a frame that was `zeroed`: those are the retained list's)
                launch_frame_begin(f, st);
                break;
            }
            if (!zeroed) HIP_TRY(c, hipMemsetAsync(l.zero_region.ptr, 0, slot_of(c, l).zero_bytes, st));
            launch_pathtag_scan(f, st);
            break;
        case VELLO_HIP_STAGE_FLATTEN:
            l.flatten_ran = true;
            if (fuse_all) break;
            // (a range that goes on to DRAW_SCAN: that stage's workgroups ride in flatten's first launch)
            if (fuse_a) {
                // (k_front's barrier counter advances on the host only once the launch was accepted: ADVICE r5)
                const uint32_t add = launch_front(f, st, front_zero | FRONT_PATHTAG | FRONT_LIGHT, last >= VELLO_HIP_STAGE_DRAW_SCAN, l.front_sync_value);
                if (int r = front_accepted(c, l, st, add)) return r;
            }
            launch_flatten(f, st, prof ? ev.mid : nullptr, last >= VELLO_HIP_STAGE_DRAW_SCAN, fuse_a);
            break;
        case VELLO_HIP_STAGE_DRAW_SCAN:
            if (first > VELLO_HIP_STAGE_FLATTEN) launch_draw_scan(f, st);  // (else: done beside k_flatten_light)
            break;
        case VELLO_HIP_STAGE_CLIP: launch_clip(f, st); break;
        case VELLO_HIP_STAGE_BINNING:
            if (fuse_all) break;
            if (fuse_b) {
                if (f.cfg.layout.n_draw_objects != 0u || f.cfg.layout.n_paths != 0u) {
                    front_add = launch_front(f, st, FRONT_BINNING | FRONT_TILE_ALLOC, false, l.front_sync_value);
                    front_launched = true;
                }
            } else if (pair_b) {
                launch_binning_tile_alloc(f, st);
            } else {
                launch_binning(f, st);
            }
            break;
        case VELLO_HIP_STAGE_TILE_ALLOC:
            if (!fuse_all && !fuse_b && !pair_b) launch_tile_alloc(f, st);
            break;
        case VELLO_HIP_STAGE_PATH_COUNT: launch_path_count(f, st); break;
        case VELLO_HIP_STAGE_BACKDROP: launch_backdrop(f, st); break;
        case VELLO_HIP_STAGE_COARSE: launch_coarse(f, st, prof ? ev.mid : nullptr); break;
        case VELLO_HIP_STAGE_PATH_TILING: launch_path_tiling(f, st); break;
        case VELLO_HIP_STAGE_FINE:
            // A frame over a base image that a caller's stream writes: fine, the only reader, waits for the stream as it stood when
            // the image was set, and the stream for fine -- what it enqueues from here on may overwrite the image.
            if (f.base_event) HIP_TRY(c, hipStreamWaitEvent(st, f.base_event, 0));
            launch_fine(f, st);
            if (f.base_stream) {
                HIP_TRY(c, hipGetLastError());
                HIP_TRY(c, hipEventRecord(f.base_mark, st));
                HIP_TRY(c, hipStreamWaitEvent(f.base_stream, f.base_mark, 0));
            }
            break;
        default: return VELLO_HIP_E_INVALID;
        }
        if (front_launched) {
            if (int r = front_accepted(c, l, st, front_add)) return r;
        } else {
            HIP_TRY(c, hipGetLastError());
        }
        if (prof) {
            HIP_TRY(c, hipEventRecord(ev.b, st));
            l.events.push_back(ev);
        }
    }
    return 0;
}

}  // namespace vk

extern "C" {

// The pipelined form of vello_hip_render for animations: every frame brings its own scene.  The scene goes into
// the private slot of the next lane of the rotation (only THAT lane's previous frame is waited for), the frame is
// enqueued, and the call returns; other lanes keep rendering while the next scene crosses PCIe.
int vello_hip_render_frame(vello_hip_ctx *c, const uint8_t *scene, size_t scene_len, const vello_hip_layout *layout,
                           const vello_hip_render_params *params, const uint32_t *ramps, uint32_t n_ramps, void *out_device,
                           size_t out_stride) {
    if (!c || !params) return VELLO_HIP_E_INVALID;
    if (int tr = check_target(c, params, out_device, out_stride, true)) return tr;
    const auto set_up = [&](Lane &l, bool &) -> int {
        HIP_TRY(c, hipStreamSynchronize(l.stream));
        if (int r = load_slot(c, l.own, l.stream, scene, scene_len, layout, ramps, n_ramps)) return r;
        l.which = LaneScene::Own;
        return 0;
    };
    return enter_frame(c, params, out_device, out_stride, true, VELLO_HIP_STAGE_FINE, set_up, no_step, no_step);
}

int vello_hip_render_resident(vello_hip_ctx *c, const vello_hip_render_params *params, void *out_device, size_t out_stride) {
    if (!c) return VELLO_HIP_E_INVALID;
    if (int r = check_target(c, params, out_device, out_stride, true)) return r;
    const auto set_up = [&](Lane &l, bool &new_scene) -> int {
        new_scene = l.which != LaneScene::Shared;
        if (!new_scene) return 0;
        // the lane last rendered a scene of its own or the retained list: resident frames always show the scene of
        // vello_hip_upload_scene, whichever lane the rotation has reached
        if (!c->shared.resident) {
            c->last_error = "no scene uploaded (vello_hip_render_frame scenes are private to their frame)";
            return VELLO_HIP_E_INVALID;
        }
        HIP_TRY(c, hipStreamSynchronize(l.stream));
        l.which = LaneScene::Shared;
        return 0;
    };
    int last = VELLO_HIP_STAGE_FINE;
    if (const uint32_t ls = (c->debug_flags >> VELLO_HIP_DEBUG_LAST_STAGE_SHIFT) & 15u) last = (int)ls - 1 < last ? (int)ls - 1 : last;  // (measurement seam)
    // (the lane's copy of the path-data words, if a morphed frame left one, is not this frame's: it shows the scene's own points)
    Lane &lane = c->lanes[c->next_lane % c->n_active];
    const uint64_t morphed_was = lane.morphed_generation;
    lane.morphed_generation = 0u;
    const int r = enter_frame(c, params, out_device, out_stride, true, last, set_up, no_step, no_step);
    if (r) lane.morphed_generation = morphed_was;  // (refused: the lane's latest frame is still the one before)
    return r;
}

// A frame of the resident scene whose path-data words are blend(A, B, t).  Everything that can refuse the frame is asked before the
// lane is taken; what the host does per frame does not depend on the scene's size.  The blend's case (rule 2 of the contract) is
// picked here: the kernel is told to copy one stream or to mix two.
int vello_hip_render_resident_morphed(vello_hip_ctx *c, uint32_t src_a, uint32_t src_b, float t, const uint32_t *device_words, void *src_stream,
                                      const vello_hip_render_params *params, void *out_device, size_t out_stride) {
    if (!c) return VELLO_HIP_E_INVALID;
    auto refuse = [&](const std::string &why) {
        c->last_error = "render_resident_morphed: " + why;
        return VELLO_HIP_E_INVALID;
    };
    if (!params) return refuse("params is NULL");
    if (!c->shared.resident) return refuse("no scene uploaded");
    const SceneSlot &sc = c->shared;
    const uint32_t n = sc.layout.draw_tag_base - sc.layout.path_data_base;
    bool names_device = false;
    for (const uint32_t src : {src_a, src_b}) {
        if (src == VELLO_HIP_PATH_DATA_DEVICE) names_device = true;
        else if (src != VELLO_HIP_PATH_DATA_SCENE && src >= c->n_keys)
            return refuse("source " + std::to_string(src) + " of " + std::to_string(c->n_keys) + " keyframes (vello_hip_upload_path_keyframes)");
    }
    if (!names_device && device_words) return refuse("device_words goes with a VELLO_HIP_PATH_DATA_DEVICE source");
    if (!names_device && src_stream) return refuse("src_stream goes with a VELLO_HIP_PATH_DATA_DEVICE source");
    if (!(t - t == 0.0f)) return refuse("t is not finite");
    if (names_device) {
        if (!device_words) return refuse("VELLO_HIP_PATH_DATA_DEVICE without device_words");
        if ((reinterpret_cast<uintptr_t>(device_words) & 3u) != 0u) return refuse("the address of device_words is not a multiple of 4");
        if (n != 0u)
            if (const char *why = not_device_memory(c, device_words, (size_t)n * 4u)) return refuse(std::string("device_words ") + why);
    }
    const uint32_t mode = src_a == src_b || t == 0.0f ? PATH_BLEND_COPY_A : t == 1.0f ? PATH_BLEND_COPY_B : PATH_BLEND_MIX;
    if (mode == PATH_BLEND_MIX && sc.i16_segments)
        return refuse("the scene holds an i16 segment tag: its path data cannot be blended as floats (t = 0, t = 1 and equal sources are legal)");
    int r;
    if ((r = check_target(c, params, out_device, out_stride, true))) return r;
    {
        Config probe;  // (what prepare_frame would refuse, asked before anything changes)
        if ((r = configure(c, sc, params, probe))) return r;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    // the room for the lanes' copies: made once per resident scene (here, unless the keyframes' upload has made it)
    if ((r = ensure_morph_room(c))) return r;
    Lane &lane = c->lanes[c->next_lane % c->n_active];  // (the lane enter_frame takes)
    {
        uint32_t probe;
        if ((r = morph_base(c, sc, lane, probe))) return r;
    }
    if (src_stream && !c->pose_mark) HIP_TRY(c, hipEventCreateWithFlags(&c->pose_mark, hipEventDisableTiming));
    const auto source = [&](uint32_t src) -> const uint32_t * {
        if (src == VELLO_HIP_PATH_DATA_DEVICE) return device_words;
        if (src == VELLO_HIP_PATH_DATA_SCENE) return (const uint32_t *)sc.scene.ptr + sc.layout.path_data_base;
        return (const uint32_t *)c->keyframes.ptr + (size_t)src * c->key_stride;
    };
    const uint64_t morphed_was = lane.morphed_generation;
    const auto set_up = [&](Lane &l, bool &new_scene) -> int {
        new_scene = l.which != LaneScene::Shared;
        if (!new_scene) return 0;
        HIP_TRY(c, hipStreamSynchronize(l.stream));
        l.which = LaneScene::Shared;
        return 0;
    };
    const auto staged = [&](Lane &l) -> int {
        l.pd_a = source(src_a);
        l.pd_b = source(src_b);
        l.pd_mode = mode;
        l.pd_t = t;
        l.pd_stream = (hipStream_t)src_stream;
        l.morphed_generation = sc.generation;
        return 0;
    };
    bool entered = false;
    const auto enqueue = [&](Lane &l) -> int {
        entered = true;
        c->cfg_unsent = true;  // (VELLO_HIP_BUF_CONFIG gets the Config -- the scene's own layout -- when it is next read or written)
        if (src_stream) {  // behind what the caller's stream has been given so far
            HIP_TRY(c, hipEventRecord(c->pose_mark, (hipStream_t)src_stream));
            HIP_TRY(c, hipStreamWaitEvent(l.stream, c->pose_mark, 0));
        }
        return 0;
    };
    r = enter_frame(c, params, out_device, out_stride, false, VELLO_HIP_STAGE_FINE, set_up, staged, enqueue);
    // the sources belonged to this frame, enqueued or refused: the lane keeps neither the caller's memory nor the caller's stream
    lane.pd_a = lane.pd_b = nullptr;
    lane.pd_stream = nullptr;
    if (!entered) lane.morphed_generation = morphed_was;  // (refused: the lane's latest frame is still the one before)
    return r;
}

// A frame of the retained instance list under this frame's poses and paints.  Everything that can refuse the frame is asked before
// the lane is taken; what the host does per frame does not depend on the list's length unless poses or paints are the host's own.
// Without paints this is vello_hip_render_retained as it was: the same checks, the same copies, the same launches.
int vello_hip_render_retained_painted(vello_hip_ctx *c, const float *transforms, int transforms_is_device, const vello_hip_paint *paints,
                                      int paints_is_device, void *src_stream, const vello_hip_render_params *params, void *out_device,
                                      size_t out_stride) {
    if (!c || !params) return VELLO_HIP_E_INVALID;
    auto refuse = [&](const std::string &why) {
        c->last_error = "render_retained: " + why;
        return VELLO_HIP_E_INVALID;
    };
    if (!c->have_retained || !c->retained.resident) return refuse("no retained instance list (vello_hip_retain_instances)");
    const uint32_t n = c->retained_n;
    const size_t pose_bytes = (size_t)n * 24u, paint_bytes = (size_t)n * sizeof(vello_hip_paint);
    const bool device = transforms != nullptr && transforms_is_device != 0;
    const bool paints_device = paints != nullptr && paints_is_device != 0;
    if (paints && !c->have_masks)
        return refuse("the fragments' draw_data ranges add up to 2^32 words or more: the library takes no paints");
    if (src_stream && !device && !paints_device) return refuse("src_stream goes with poses or paints in device memory");
    if (transforms && !device)
        for (uint32_t i = 0; i < n; i++)
            for (int k = 0; k < 6; k++) {
                const float v = transforms[(size_t)i * 6u + k];
                if (!(v - v == 0.0f)) return refuse("instance " + std::to_string(i) + ": the pose has an entry that is not finite");
            }
    if (paints && !paints_device)
        for (uint32_t i = 0; i < n; i++)
            if (paints[i].flags != VELLO_HIP_PAINT_KEEP && paints[i].flags != VELLO_HIP_PAINT_SOLID)
                return refuse("instance " + std::to_string(i) + ": paint flags " + std::to_string(paints[i].flags) + " (VELLO_HIP_PAINT_KEEP or _SOLID)");
    // a source in device memory: 4-byte aligned, and -- GPU builds -- every byte the kernel reads lies in one allocation in device
    // memory of this context's device (vello_hip_copy_images_device)
    const auto check_device = [&](const void *ptr, size_t bytes, const char *what) -> int {
        if ((reinterpret_cast<uintptr_t>(ptr) & 3u) != 0u) return refuse(std::string("the address of device ") + what + " is not a multiple of 4");
#ifndef VELLO_SIMT_EMU
        if (n != 0u) {
            hipDeviceptr_t base = nullptr;
            size_t size = 0;
            hipPointerAttribute_t attr{};
            hipError_t e = hipMemGetAddressRange(&base, &size, (hipDeviceptr_t) const_cast<void *>(ptr));
            if (e == hipSuccess) e = hipPointerGetAttributes(&attr, base);
            (void)hipGetLastError();  // a host address is an error here: do not leave it for the next launch check
            if (e != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != c->device)
                return refuse(std::string("the ") + what + " are not device memory of device " + std::to_string(c->device));
            if ((uint64_t)(uintptr_t)ptr + bytes > (uint64_t)(uintptr_t)base + size)
                return refuse(std::string("the ") + what + " run past the end of their allocation");
        }
#else
        (void)bytes;
#endif
        return 0;
    };
    int r;
    if (device && (r = check_device(transforms, pose_bytes, "poses"))) return r;
    if (paints_device && (r = check_device(paints, paint_bytes, "paints"))) return r;
    if ((r = check_target(c, params, out_device, out_stride, true))) return r;
    {
        Config probe;  // (what prepare_frame would refuse, asked before the lane changes its scene)
        if ((r = configure(c, c->retained, params, probe))) return r;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    Lane &lane = c->lanes[c->next_lane % c->n_active];  // (the lane enter_frame takes)
    if (paints) {
        uint32_t probe;  // (likewise: the lane's copy of the draw-data words must be within reach)
        if ((r = paint_base(c, c->retained, lane, probe))) return r;
    }
    if (src_stream && !c->pose_mark) HIP_TRY(c, hipEventCreateWithFlags(&c->pose_mark, hipEventDisableTiming));
    // host sources cross in ONE pinned block: the poses, then the paints
    const size_t host_pose_bytes = transforms && !device ? pose_bytes : 0u, host_paint_bytes = paints && !paints_device ? paint_bytes : 0u;
    Staging *st = nullptr;
    const uint64_t painted_was = lane.painted_generation;
    const auto set_up = [&](Lane &l, bool &new_scene) -> int {
        new_scene = l.which != LaneScene::Retained;  // (else: sized when the list was retained, or by the lane's earlier frame of it)
        if (!new_scene) return 0;
        HIP_TRY(c, hipStreamSynchronize(l.stream));
        l.which = LaneScene::Retained;
        return 0;
    };
    const auto staged = [&](Lane &l) -> int {
        const bool host_poses = transforms && !device, host_paints = paints && !paints_device;
        if (host_poses || host_paints)
            if (int sr = acquire_staging(c, host_pose_bytes + host_paint_bytes, st)) return sr;
        if (host_poses)
            if (int sr = ensure(c, l.poses, pose_bytes)) return sr;
        if (host_paints)
            if (int sr = ensure(c, l.paints, paint_bytes)) return sr;
        l.pose_src = !transforms ? nullptr : device ? reinterpret_cast<const uint32_t *>(transforms) : (const uint32_t *)l.poses.ptr;
        l.pose_stream = (hipStream_t)src_stream;
        l.pose_check = device;
        l.paint_src = !paints ? nullptr : paints_device ? reinterpret_cast<const uint32_t *>(paints) : (const uint32_t *)l.paints.ptr;
        l.paint_check = paints_device;
        // (prepare_frame picks the lane's copy of the draw-data words for a painted frame, the retained stream otherwise)
        l.painted_generation = paints ? c->retained.generation : 0u;
        return 0;
    };
    bool entered = false;
    const auto enqueue = [&](Lane &l) -> int {
        entered = true;
        c->cfg_unsent = true;  // (as an instance frame: VELLO_HIP_BUF_CONFIG gets the Config when it is next read or written)
        if (st) {
            if (host_pose_bytes) {
                std::memcpy(st->host, transforms, host_pose_bytes);
                HIP_TRY(c, hipMemcpyAsync(l.poses.ptr, st->host, host_pose_bytes, hipMemcpyHostToDevice, l.stream));
            }
            if (host_paint_bytes) {
                std::memcpy((char *)st->host + host_pose_bytes, paints, host_paint_bytes);
                HIP_TRY(c, hipMemcpyAsync(l.paints.ptr, (char *)st->host + host_pose_bytes, host_paint_bytes, hipMemcpyHostToDevice, l.stream));
            }
            HIP_TRY(c, hipEventRecord(st->done, l.stream));
            st->busy = true;
        }
        if (src_stream) {  // behind what the caller's stream has been given so far
            HIP_TRY(c, hipEventRecord(c->pose_mark, (hipStream_t)src_stream));
            HIP_TRY(c, hipStreamWaitEvent(l.stream, c->pose_mark, 0));
        }
        return 0;
    };
    r = enter_frame(c, params, out_device, out_stride, false, VELLO_HIP_STAGE_FINE, set_up, staged, enqueue);
    // poses and paints belonged to this frame, enqueued or refused: the lane keeps neither the caller's memory nor the caller's stream
    lane.pose_src = nullptr;
    lane.pose_stream = nullptr;
    lane.pose_check = false;
    lane.paint_src = nullptr;
    lane.paint_check = false;
    if (!entered) lane.painted_generation = painted_was;  // (refused: the lane's latest frame is still the one before)
    return r;
}

int vello_hip_render_retained(vello_hip_ctx *c, const float *transforms, int transforms_is_device, void *src_stream,
                              const vello_hip_render_params *params, void *out_device, size_t out_stride) {
    return vello_hip_render_retained_painted(c, transforms, transforms_is_device, nullptr, 0, src_stream, params, out_device, out_stride);
}

int vello_hip_run_stages(vello_hip_ctx *c, const vello_hip_render_params *params, int first, int last) {
    if (!c || first < 0 || last >= VELLO_HIP_STAGE_COUNT || first > last) return VELLO_HIP_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    Lane &l = c->lanes[c->last_lane];
    Frame f;
    int r;
    if (last >= VELLO_HIP_STAGE_FINE && (r = check_base_image(c, params, nullptr, 0))) return r;
    r = prepare_frame(c, l, params, nullptr, 0, f, true);
    if (r) return r;
    if (f.retained) {
        // after a retained frame: the lane's copy holds that frame's composed words and the stages go on from them -- its poses may
        // have been the caller's device memory, which is not read again; a lane that holds none of this list (a list retained
        // since) gets the rest poses
        f.pose_stream = nullptr;
        f.pose_check = false;
        f.pose_words = l.posed_generation == c->retained.generation ? nullptr : (const uint32_t *)c->retained_rest.ptr;
    }
    // (after a morphed frame: prepare_frame has picked the lane's copy of the path-data words, which holds that frame's words -- no
    // source is set on the lane outside vello_hip_render_resident_morphed, so nothing is blended again)
    if ((r = run_stage_range(c, l, f, first, last))) return r;
    HIP_TRY(c, hipStreamSynchronize(l.stream));
    return VELLO_HIP_OK;
}

int vello_hip_get_bump(vello_hip_ctx *c, vello_hip_bump *out) {
    if (!c || !out || !c->lanes[c->last_lane].zero_region.ptr) return VELLO_HIP_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    Lane &l = c->lanes[c->last_lane];
    HIP_TRY(c, hipStreamSynchronize(l.stream));
    HIP_TRY(c, hipMemcpy(out, l.zero_region.ptr, sizeof(vello_hip_bump), hipMemcpyDeviceToHost));
    return VELLO_HIP_OK;
}

int vello_hip_sync_frame(vello_hip_ctx *c, uint32_t age) {
    if (!c || age >= c->n_active) return VELLO_HIP_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    uint32_t n = c->n_active;
    Lane &l = c->lanes[(c->last_lane + n - age) % n];
    HIP_TRY(c, hipStreamSynchronize(l.stream));
    // (once per scene: what flatten counted, so that later frames can leave out a launch that would exit at once)
    SceneSlot &sc = slot_of(c, l);
    if (l.used && l.flatten_ran && l.zero_region.ptr && l.frame_generation == sc.generation && (sc.stroke_lines < 0 || (l.slices_on && !l.frame_damaged && sc.slice_demand < 0))) {
        Control ctl;
        HIP_TRY(c, hipMemcpy(&ctl, l.zero_region.ptr, sizeof ctl, hipMemcpyDeviceToHost));
        if (ctl.bump.failed == 0u) learn_from_frame(sc, ctl, l);
    }
    return VELLO_HIP_OK;
}

int vello_hip_sync(vello_hip_ctx *c) {
    if (!c) return VELLO_HIP_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    int r = sync_all(c);
    if (r) return r;
    if (!c->have_cfg) return VELLO_HIP_OK;
    // only the lanes of the current rotation: a lane dropped by set_frames_in_flight keeps its old control block
    int first = VELLO_HIP_OK;
    for (uint32_t i = 0; i < c->n_active && i < c->lanes.size(); i++) {
        r = check_lane(c, c->lanes[i]);
        if (r == VELLO_HIP_E_HIP) return r;
        if (r && !first) first = r;
    }
    return first;
}

uint32_t vello_hip_last_render_attempts(vello_hip_ctx *c) { return c ? c->last_render_attempts : 0u; }
uint64_t vello_hip_fused_launches(vello_hip_ctx *c) { return c ? c->fused_launches : 0u; }

void *vello_hip_get_stream(vello_hip_ctx *c) { return c ? (void *)c->lanes[c->last_lane].stream : nullptr; }

int vello_hip_set_auto_grow(vello_hip_ctx *c, int enabled) {
    if (!c) return VELLO_HIP_E_INVALID;
    c->auto_grow = enabled != 0;
    return VELLO_HIP_OK;
}

// A frame takes the setting when it is prepared (Frame::viewport_cull travels to flatten's kernels by value), so frames already
// enqueued keep theirs.  The scene's remembered soup size (SceneSlot::soup_lines) only picks path_count's chunk size -- its grid
// strides over the pool -- so a frame after a toggle is at worst cut into the other chunk size once.
int vello_hip_set_viewport_cull(vello_hip_ctx *c, int enabled) {
    if (!c) return VELLO_HIP_E_INVALID;
    c->viewport_cull = enabled != 0;
    return VELLO_HIP_OK;
}

// As the culling switch: a frame takes the view when it is prepared (Frame::view travels to k_view_transforms by value, and the
// frame's composed transform words are its lane's own), so frames already enqueued keep theirs.  What the engine remembers of a
// scene's earlier frames (SceneSlot) only picks among kernels and launch shapes that are all correct for any view: DESIGN.md 13.
int vello_hip_set_view_transform(vello_hip_ctx *c, const float view[6]) {
    if (!c) return VELLO_HIP_E_INVALID;
    if (!view) {
        c->has_view = false;
        return VELLO_HIP_OK;
    }
    for (int k = 0; k < 6; k++)
        if (!(view[k] - view[k] == 0.0f)) {  // NaN or infinity
            c->last_error = "set_view_transform: the view has an entry that is not finite";
            return VELLO_HIP_E_INVALID;
        }
    c->has_view = true;
    c->view = Xform{view[0], view[1], view[2], view[3], view[4], view[5]};
    return VELLO_HIP_OK;
}

// As the view: a frame takes the setting when it is prepared (Frame::stroke_scale / stroke_min travel to k_style_widths by value, and
// the frame's style words are its lane's own copy), so frames already enqueued keep theirs.  Nothing the engine remembers of a
// scene depends on a width: the scene index holds tags and flags, and what a finished frame teaches (SceneSlot) only picks among
// kernels and launch shapes that are all correct for any width.  The refusals are made here, where no frame is at stake.
int vello_hip_set_stroke_scale(vello_hip_ctx *c, const float stroke[2]) {
    if (!c) return VELLO_HIP_E_INVALID;
    if (!stroke) {
        c->has_stroke = false;
        return VELLO_HIP_OK;
    }
    const float s = stroke[0], m = stroke[1];
    if (!(s - s == 0.0f) || !(s > 0.0f)) {
        c->last_error = "set_stroke_scale: the scale must be finite and > 0";
        return VELLO_HIP_E_INVALID;
    }
    if (!(m - m == 0.0f) || !(m >= 0.0f)) {
        c->last_error = "set_stroke_scale: the minimum width must be finite and >= 0";
        return VELLO_HIP_E_INVALID;
    }
    c->has_stroke = true;
    c->stroke_scale = s;
    c->stroke_min = m;
    return VELLO_HIP_OK;
}

// As the two switches above: a frame takes the rectangle when it is prepared (Frame::damage, cut to that frame's target, travels to
// k_coarse and k_fine by value), so frames already enqueued keep theirs.  The only refusal is made here, where no frame is at stake:
// the rotation stays where it was.  What the engine remembers of a scene's earlier frames is not taught by a damaged frame where it
// would differ from a whole frame's (learn_from_frame).
int vello_hip_set_damage_rect(vello_hip_ctx *c, const uint32_t rect[4]) {
    if (!c) return VELLO_HIP_E_INVALID;
    if (!rect) {
        c->has_damage = false;
        return VELLO_HIP_OK;
    }
    if (rect[0] > rect[2] || rect[1] > rect[3]) {
        c->last_error = "set_damage_rect: the rectangle is x0 y0 x1 y1 with x0 <= x1 and y0 <= y1 (half open; an empty one is legal)";
        return VELLO_HIP_E_INVALID;
    }
    c->has_damage = true;
    for (int k = 0; k < 4; k++) c->damage[k] = rect[k];
    return VELLO_HIP_OK;
}

// As the switches above: a frame takes image, stride, stream and event when it is prepared (Frame::base_image ... travel to k_fine_base
// and to the two stream waits by value), so frames already enqueued keep theirs.  What can be refused without a frame is refused
// here; what depends on the frame's size and target when it is enqueued (check_base_image).  Nothing the engine remembers of a
// scene depends on the base: no stage ahead of fine reads it.
int vello_hip_set_base_image(vello_hip_ctx *c, const void *image_device, size_t stride, void *src_stream) {
    if (!c) return VELLO_HIP_E_INVALID;
    const auto refuse = [&](const char *why) {
        c->last_error = std::string("set_base_image: ") + why;
        return VELLO_HIP_E_INVALID;
    };
    if (!image_device && src_stream) return refuse("src_stream goes with an image");
    if ((reinterpret_cast<uintptr_t>(image_device) & 3u) != 0u) return refuse("the address of the image is not a multiple of 4");
    if ((stride & 3u) != 0u) return refuse("the stride is not a multiple of 4");
    if ((uint64_t)stride > 0xffffffffull) return refuse("the stride must be below 2^32");
    if (image_device && src_stream) {
        // the stream as it stands now: what the frames that follow wait for (a failure here leaves the setting as it was)
        HIP_TRY(c, hipSetDevice(c->device));
        if (!c->base_ready) HIP_TRY(c, hipEventCreateWithFlags(&c->base_ready, hipEventDisableTiming));
        if (!c->base_mark) HIP_TRY(c, hipEventCreateWithFlags(&c->base_mark, hipEventDisableTiming));
        HIP_TRY(c, hipEventRecord(c->base_ready, (hipStream_t)src_stream));
    }
    c->base_image = (const uint8_t *)image_device;
    c->base_stride = image_device ? stride : 0u;
    c->base_stream = image_device ? (hipStream_t)src_stream : nullptr;
    c->base_checked = 0u;
    return VELLO_HIP_OK;
}

int vello_hip_render(vello_hip_ctx *c, const uint8_t *scene, size_t scene_len, const vello_hip_layout *layout,
                     const vello_hip_render_params *params, const uint32_t *ramps, uint32_t n_ramps, void *out_rgba8, size_t out_stride,
                     int out_is_device, vello_hip_bump *bump_out) {
    if (!c || !params) return VELLO_HIP_E_INVALID;
    int r = check_target(c, params, out_rgba8, out_stride, out_is_device != 0);
    if (r) return r;
    if ((r = check_base_image(c, params, out_is_device ? out_rgba8 : nullptr, out_stride))) return r;
    if (c->auto_grow && (r = presize_pools(c, scene, scene_len, layout, params))) return r;
    r = vello_hip_upload_scene(c, scene, scene_len, layout, ramps, n_ramps);
    if (r) return r;
    int sync_r = VELLO_HIP_OK;
    // robust mode: re-run with grown pools until the frame fits (each overflowing stage hides the demand of
    // the stages behind it, so a handful of rounds at most)
    for (int attempt = 0; attempt < 8; attempt++) {
        c->last_render_attempts = (uint32_t)attempt + 1u;
        r = vello_hip_render_resident(c, params, out_is_device ? out_rgba8 : nullptr, out_stride);
        if (r) return r;
        Lane &l = c->lanes[c->last_lane];
        HIP_TRY(c, hipStreamSynchronize(l.stream));
        vello_hip_bump b;
        HIP_TRY(c, hipMemcpy(&b, l.zero_region.ptr, sizeof b, hipMemcpyDeviceToHost));
        sync_r = check_lane(c, l);  // this frame's lane only: another lane's older failure is not this frame's
        if (bump_out) *bump_out = b;
        if (sync_r != VELLO_HIP_E_CAPACITY || !c->auto_grow) break;
        if (vello_hip_grow_pools(c, &b, nullptr) != VELLO_HIP_OK) break;
    }
    if (sync_r) return sync_r;
    if (out_rgba8 && !out_is_device) {
        // R's rows and columns only (the whole target when no damage rectangle is set): the rest of the caller's memory stays as it is
        const PixelRect d = damage_of(c, params);
        const size_t row = (size_t)params->width * 4u, at = (size_t)d.x0 * 4u;
        if (!empty(d))
            HIP_TRY(c, hipMemcpy2D((uint8_t *)out_rgba8 + (size_t)d.y0 * row_stride(params, out_stride) + at, row_stride(params, out_stride),
                                   (const uint8_t *)c->lanes[c->last_lane].buf[VELLO_HIP_BUF_OUTPUT].ptr + (size_t)d.y0 * row + at, row,
                                   (size_t)(d.x1 - d.x0) * 4u, d.y1 - d.y0, hipMemcpyDeviceToHost));
    }
    return VELLO_HIP_OK;
}

}  // extern "C"
