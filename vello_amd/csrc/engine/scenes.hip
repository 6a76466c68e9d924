// Scenes: making a packed scene resident in a slot, the shared scene as a library of fragments, frames composed from instances,
// an instance list retained across frames.
#include <cstring>

#include "ctx.h"

using namespace vk;

namespace {

// ensure() for a slot's scene buffer: `bytes` of scene (what VELLO_HIP_BUF_SCENE shows) and, from the next 16-byte boundary on, a
// tail of `tail` bytes for the composed transform words.  Like ensure() it never shrinks -- neither part: the tail's capacity is
// kept in a field of its own, written only where the allocation happens, so that scenes whose transform counts go up and down
// (a lane's vello_hip_render_frame scenes) settle on the largest and allocate nothing from then on.
int ensure_scene(vello_hip_ctx *c, SceneSlot &sc, size_t bytes, size_t tail) {
    if (sc.scene.ptr && sc.scene.size >= bytes && sc.view_cap_bytes >= tail) return 0;
    const size_t visible = sc.scene.size > bytes ? sc.scene.size : bytes;
    const size_t cap = sc.view_cap_bytes > tail ? sc.view_cap_bytes : tail;
    if (sc.scene.ptr) HIP_TRY(c, hipFree(sc.scene.ptr));
    sc.scene.ptr = nullptr;
    sc.scene.size = 0;
    sc.view_cap_bytes = 0;
    const size_t at = (visible + 15u) & ~(size_t)15u;
    HIP_TRY(c, hipMalloc(&sc.scene.ptr, at + cap + 256));
    sc.scene.size = visible;
    sc.view_at = at / 4u;
    sc.view_cap_bytes = cap;
    c->scene_allocations++;
    return 0;
}

// Whether `layout` describes a buffer of scene_len bytes (the streams' contents are judged by load_slot and the pathtag scan)
int check_layout(vello_hip_ctx *c, const uint8_t *scene, size_t scene_len, const vello_hip_layout *layout) {
    if ((!scene && scene_len) || !layout || (scene_len & 3u)) return VELLO_HIP_E_INVALID;
    const vello_hip_layout &L = *layout;
    size_t words = scene_len / 4u;
    if (L.path_tag_base > L.path_data_base || L.path_data_base > L.draw_tag_base || L.draw_tag_base > L.draw_data_base ||
        L.draw_data_base > L.transform_base || L.transform_base > L.style_base || L.style_base > words ||
        (size_t)L.draw_tag_base + L.n_draw_objects > words) {
        c->last_error = "layout does not describe the scene buffer";
        return VELLO_HIP_E_INVALID;
    }
    if ((((size_t)L.path_data_base - L.path_tag_base) * 4u) % 1024u != 0u) {
        c->last_error = "path tag stream is not padded to 4*256 tags (resolve.rs:622-639)";
        return VELLO_HIP_E_INVALID;
    }
    return VELLO_HIP_OK;
}

// Sizes the slot for a scene of this (checked) layout and length and forgets what earlier frames told of the scene it held: what
// load_slot does before it copies the bytes, and vello_hip_render_instances before k_compose_scene writes them.
int size_slot(vello_hip_ctx *c, SceneSlot &sc, const vello_hip_layout &L, size_t scene_len) {
    int r;
    // 64 B of slack: flatten reads tag ix+1 and the (wrapped) style word of pre-style tags speculatively
    // ... and, behind them, room for the composed transform words of frames with a view (SceneSlot::view_at)
    const uint32_t set_words = ((L.style_base - L.transform_base) / 6u + 1u) * 6u;
    const uint32_t sets = &sc == &c->shared || &sc == &c->retained ? MAX_LANES : 1u;
    // ... and, the retained slot only, behind those a copy per lane of the draw-data stream for painted frames (SceneSlot::dd_at) --
    // unless the copies would lie beyond a u32 word offset from the scene's start: such a list takes no paints and gets no room
    // ... and, behind those, the style words of frames with a stroke scale (SceneSlot::st_at): as many copies, each the stream's
    // entries and slot -1 in front; from an even word (the transform copies are whole entries of six words from a 16-byte boundary)
    const size_t st_set_words = ((scene_len / 4u - L.style_base) / STYLE_SIZE_IN_WORDS + 1u) * STYLE_SIZE_IN_WORDS;
    const size_t xf_tail_words = ((size_t)set_words * sets + 1u) & ~(size_t)1u;
    const size_t st_tail_words = st_set_words * sets;
    const uint32_t dd_words = L.transform_base - L.draw_data_base;
    uint32_t dd_sets = 0u;
    if (&sc == &c->retained) {
        const size_t visible = sc.scene.size > scene_len + 64 ? sc.scene.size : scene_len + 64;  // (what ensure_scene settles on)
        const uint64_t reach = (uint64_t)((visible + 15u) / 4u) + xf_tail_words + st_tail_words + (uint64_t)dd_words * MAX_LANES;
        if (reach <= 0xffffffffull) dd_sets = MAX_LANES;
    }
    if ((r = ensure_scene(c, sc, scene_len + 64, (xf_tail_words + st_tail_words + (size_t)dd_words * dd_sets) * 4u))) return r;
    sc.view_sets = sets;
    sc.view_set_words = set_words;
    sc.st_at = sc.view_at + xf_tail_words;
    sc.st_sets = sets;
    sc.st_set_words = st_set_words > 0xffffffffull ? 0xffffffffu : (uint32_t)st_set_words;  // (out of reach either way: style_base refuses)
    sc.dd_at = sc.st_at + st_tail_words;
    sc.dd_sets = dd_sets;
    sc.dd_set_words = dd_words;
    sc.pd_sets = 0u;  // (room for morphed frames' path data is made when the scene is first morphed: ensure_morph_room)
    sc.i16_segments = false;
    sc.layout = L;
    sc.scene_len = scene_len;
    uint32_t n_path_tags = (L.path_data_base - L.path_tag_base) * 4u;
    sc.n_tag_words = align_up(n_path_tags, 1024u) / 4u;
    sc.n_pathtag_parts = (sc.n_tag_words + PATHTAG_PART_WORDS - 1u) / PATHTAG_PART_WORDS;
    if (sc.n_pathtag_parts == 0) sc.n_pathtag_parts = 1;
    sc.n_draw_parts = (L.n_draw_objects + DRAW_PART - 1u) / DRAW_PART;
    sc.zero_bytes = sizeof(Control) + ((size_t)sc.n_pathtag_parts * 10u + (size_t)sc.n_draw_parts * 8u) * 8u;
    // Which fine specialisation the scene needs: any draw tag other than COLOR / BEGIN_CLIP / END_CLIP / NOP
    // (draw.rs:15-51) makes coarse emit a gradient, image or blur command.
    sc.brushes = false;
    sc.composed = false;
    sc.stroke_lines = -1;
    sc.heavy_curves = sc.heavy_strokes = -1;
    sc.soup_lines = -1;
    sc.slice_demand = -1;
    sc.generation += 1u;
    sc.index.valid = false;  // (it spoke for the bytes the slot held)
    return VELLO_HIP_OK;
}

// One fragment against the host bytes of its (checked) library: the rules of vello_hip_upload_fragments in include/vello_hip.h.
// `mask` (nullable: no masks are kept) is the bit array of the fragments' colour words so far, `mask_bits` bits long: the fragment's bits
// are appended, one per word of its draw_data range (vello_hip_render_instances_painted has the rule).
int check_fragment(vello_hip_ctx *c, const uint8_t *scene, size_t scene_len, const vello_hip_layout &L, const vello_hip_fragment &fr,
                          uint32_t index, FragmentInfo &out, std::vector<uint32_t> *mask, uint64_t mask_bits) {
    auto refuse = [&](const char *why) {
        c->last_error = "upload_fragments: fragment " + std::to_string(index) + ": " + why;
        return VELLO_HIP_E_INVALID;
    };
    const uint32_t *words = reinterpret_cast<const uint32_t *>(scene);
    const uint64_t n_words = scene_len / 4u;
    const uint32_t draws_room = L.draw_data_base - L.draw_tag_base;
    // the streams' lengths and what one entry is in the units of ComposeArgs
    const uint64_t stream_len[6] = {((uint64_t)L.path_data_base - L.path_tag_base) * 4u, (uint64_t)L.draw_tag_base - L.path_data_base,
                                    L.n_draw_objects < draws_room ? L.n_draw_objects : draws_room, (uint64_t)L.transform_base - L.draw_data_base,
                                    ((uint64_t)L.style_base - L.transform_base) / 6u, (n_words - L.style_base) / STYLE_SIZE_IN_WORDS};
    const uint32_t unit[6] = {1u, 1u, 1u, 1u, 6u, STYLE_SIZE_IN_WORDS};
    const uint32_t *range[6] = {fr.path_tags, fr.path_data, fr.draws, fr.draw_data, fr.transforms, fr.styles};
    uint32_t n_entries[6];
    for (int s = 0; s < 6; s++) {
        if (range[s][0] > range[s][1] || range[s][1] > stream_len[s]) return refuse("a range is not ordered or leaves its stream");
        n_entries[s] = range[s][1] - range[s][0];
        out.begin[s] = range[s][0] * unit[s];  // (<= the stream's words: no overflow)
        out.len[s] = n_entries[s] * unit[s];
    }
    const uint8_t *tags = scene + (size_t)L.path_tag_base * 4u;
    uint32_t n_path = 0, n_xf = 0, n_style = 0;
    bool has_xf = false, has_style = false;
    for (uint32_t i = fr.path_tags[0]; i < fr.path_tags[1]; i++) {
        const uint32_t t = tags[i];
        if (((t & PATH_TAG_SEG_TYPE) != 0u || (t & PATH_TAG_PATH) != 0u) && !(has_xf && has_style))
            return refuse("a segment or PATH tag comes before the fragment's first TRANSFORM and STYLE markers");
        if (t & PATH_TAG_PATH) n_path++;
        if (t & PATH_TAG_TRANSFORM) n_xf++, has_xf = true;
        if (t & PATH_TAG_STYLE) n_style++, has_style = true;
    }
    if (n_path != n_entries[2]) return refuse("`draws` is not as long as the tag range has PATH markers");
    if (n_xf != n_entries[4] || n_style != n_entries[5]) return refuse("`transforms` / `styles` are not as long as the tag range has TRANSFORM / STYLE markers");
    uint64_t draw_data_words = 0, info_words = 0;
    uint32_t clip_tags = 0, depth = 0;
    out.brushes = false;
    out.mask_bit = (uint32_t)mask_bits;
    if (mask) mask->resize((size_t)((mask_bits + n_entries[3] + 31u) / 32u), 0u);
    for (uint32_t i = fr.draws[0]; i < fr.draws[1]; i++) {
        const uint32_t t = words[L.draw_tag_base + i];
        if (t != DRAWTAG_FILL_COLOR && t != DRAWTAG_BEGIN_CLIP && t != DRAWTAG_END_CLIP && t != DRAWTAG_NOP) out.brushes = true;
        // both draw objects hold a DrawColor first (draw.rs:70-74, :175-186); a word past the range belongs to a fragment refused below
        if (mask && (t == DRAWTAG_FILL_COLOR || t == DRAWTAG_BLURRED_ROUNDED_RECT) && draw_data_words < n_entries[3]) {
            const uint64_t bit = mask_bits + draw_data_words;
            (*mask)[(size_t)(bit >> 5)] |= 1u << (bit & 31u);
        }
        clip_tags += t & 1u;
        draw_data_words += (t >> 2) & 0x7u;
        info_words += (t >> 6) & 0xfu;
        if (t == DRAWTAG_BEGIN_CLIP) depth++;
        if (t == DRAWTAG_END_CLIP) {
            if (depth == 0u) return refuse("an END_CLIP without a BEGIN_CLIP before it in the fragment");
            depth--;
        }
    }
    if (depth != 0u) return refuse("a BEGIN_CLIP is left open");
    if (draw_data_words != n_entries[3]) return refuse("`draw_data` is not as long as the fragment's draw tags ask for");
    if (info_words > 0xffffffffull) return refuse("more than 2^32 info words");  // (up to 15 per draw tag)
    out.n_clips = clip_tags;
    out.info_words = (uint32_t)info_words;
    return VELLO_HIP_OK;
}

// The composed scene of an instance list: its layout, its length, what fine needs to know of it, and the sums the table is built from.
struct ComposePlan {
    vello_hip_layout layout;
    size_t scene_len;
    uint32_t len[6];      // per stream, in the units of ComposeArgs (tags: bytes, without the padding)
    uint32_t tag_words;   // the tag stream with its padding
    bool brushes;
};

static_assert(PAINT_SOLID == VELLO_HIP_PAINT_SOLID && sizeof(vello_hip_paint) == 8, "ComposePaintArgs::paints is the paint list verbatim");

int plan_instances(vello_hip_ctx *c, const vello_hip_instance *inst, const vello_hip_paint *paints, uint32_t n, ComposePlan &p) {
    if (!c->have_fragments || !c->shared.resident) {
        c->last_error = "no fragment table (vello_hip_upload_fragments)";
        return VELLO_HIP_E_INVALID;
    }
    if (n > 0u && !inst) {
        c->last_error = "instances: inst is NULL";
        return VELLO_HIP_E_INVALID;
    }
    if (paints && !c->have_masks) {
        c->last_error = "instances: the fragments' draw_data ranges add up to 2^32 words or more: the library takes no paints";
        return VELLO_HIP_E_INVALID;
    }
    uint64_t len[6] = {}, n_clips = 0, info = 0;
    p.brushes = false;
    const size_t n_frags = c->fragments.size();
    for (uint32_t i = 0; i < n; i++) {
        if (inst[i].fragment >= n_frags) {
            c->last_error = "instance " + std::to_string(i) + ": fragment " + std::to_string(inst[i].fragment) + " of " + std::to_string(n_frags);
            return VELLO_HIP_E_INVALID;
        }
        for (int k = 0; k < 6; k++)
            if (!(inst[i].transform[k] - inst[i].transform[k] == 0.0f)) {  // NaN or infinity
                c->last_error = "instance " + std::to_string(i) + ": the transform has an entry that is not finite";
                return VELLO_HIP_E_INVALID;
            }
        if (paints && paints[i].flags != VELLO_HIP_PAINT_KEEP && paints[i].flags != VELLO_HIP_PAINT_SOLID) {
            c->last_error = "instance " + std::to_string(i) + ": paint flags " + std::to_string(paints[i].flags) + " (VELLO_HIP_PAINT_KEEP or _SOLID)";
            return VELLO_HIP_E_INVALID;
        }
        const FragmentInfo &fi = c->fragments[inst[i].fragment];
        for (int s = 0; s < 6; s++) len[s] += fi.len[s];
        n_clips += fi.n_clips;
        info += fi.info_words;
        p.brushes = p.brushes || fi.brushes;
    }
    // (sums of at most 2^32 terms below 2^32: no u64 overflow)
    const uint64_t tag_bytes_padded = (len[0] + 1023u) & ~(uint64_t)1023u;
    const uint64_t total = tag_bytes_padded / 4u + len[1] + len[2] + len[3] + len[4] + len[5];
    if (total >= ((uint64_t)1 << 32) || tag_bytes_padded >= ((uint64_t)1 << 32) || n_clips > 0xffffffffull || info > 0xffffffffull) {
        c->last_error = "instances: the composed scene has 2^32 words or more, or a count that leaves u32";
        return VELLO_HIP_E_INVALID;
    }
    for (int s = 0; s < 6; s++) p.len[s] = (uint32_t)len[s];
    p.tag_words = (uint32_t)(tag_bytes_padded / 4u);
    vello_hip_layout &L = p.layout;
    L.n_draw_objects = L.n_paths = p.len[2];
    L.n_clips = (uint32_t)n_clips;
    L.bin_data_start = (uint32_t)info;
    L.path_tag_base = 0u;
    L.path_data_base = p.tag_words;
    L.draw_tag_base = L.path_data_base + p.len[1];
    L.draw_data_base = L.draw_tag_base + p.len[2];
    L.transform_base = L.draw_data_base + p.len[3];
    L.style_base = L.transform_base + p.len[4];
    p.scene_len = (size_t)total * 4u;
    return VELLO_HIP_OK;
}

// The table of an instance list as k_compose_scene reads it (engine.h ComposeArgs): six exclusive prefixes, the fragment indices, the
// transforms and -- with a paint list -- the paints, written to `table` (compose_table_words(n, paints) words).
void fill_compose_table(vello_hip_ctx *c, const vello_hip_instance *inst, const vello_hip_paint *paints, uint32_t n, uint32_t *table) {
    uint32_t *off[6], run[6] = {};
    for (int s = 0; s < 6; s++) off[s] = table + (size_t)s * (n + 1u);
    uint32_t *frag_of = table + 6u * ((size_t)n + 1u);
    for (uint32_t i = 0; i < n; i++) {
        const FragmentInfo &fi = c->fragments[inst[i].fragment];
        for (int s = 0; s < 6; s++) {
            off[s][i] = run[s];
            run[s] += fi.len[s];
        }
        frag_of[i] = inst[i].fragment;
        std::memcpy(frag_of + n + (size_t)i * 6u, inst[i].transform, 24);
    }
    for (int s = 0; s < 6; s++) off[s][n] = run[s];
    if (paints && n) std::memcpy(frag_of + 7u * (size_t)n, paints, (size_t)n * sizeof *paints);
}

// k_compose_scene (its painted form with a paint list) of the planned list from the device copy of its table into `dst`, on `st`
int launch_compose(vello_hip_ctx *c, const ComposePlan &p, uint32_t n, bool painted, const uint32_t *table_dev, uint32_t *dst, hipStream_t st) {
    ComposeArgs a{};
    a.lib = (const uint32_t *)c->shared.scene.ptr;
    a.dst = dst;
    a.table = table_dev;
    a.frags = (const uint32_t *)c->frag_table.ptr;
    a.n = n;
    const vello_hip_layout &S = c->shared.layout, &D = p.layout;
    const uint32_t src_base[6] = {S.path_tag_base, S.path_data_base, S.draw_tag_base, S.draw_data_base, S.transform_base, S.style_base};
    const uint32_t dst_base[6] = {D.path_tag_base, D.path_data_base, D.draw_tag_base, D.draw_data_base, D.transform_base, D.style_base};
    const uint64_t total = p.scene_len / 4u;
    uint64_t steps = (total + 256u * COMPOSE_TARGET_WGS - 1u) / (256u * COMPOSE_TARGET_WGS);
    steps = steps < 1u ? 1u : steps > COMPOSE_MAX_STEPS ? COMPOSE_MAX_STEPS : steps;
    a.steps = (uint32_t)steps;
    uint32_t wg = 0u;
    for (int s = 0; s < 6; s++) {
        a.src_base[s] = src_base[s];
        a.dst_base[s] = dst_base[s];
        a.len[s] = s == 0 ? p.tag_words : p.len[s];
        a.wg_first[s] = wg;
        wg += (uint32_t)(((uint64_t)a.len[s] + steps * 256u - 1u) / (steps * 256u));  // (< 2^32 words / 256 in all)
    }
    a.wg_first[6] = wg;
    a.tag_bytes = p.len[0];
    ComposePaintArgs pa{};
    if (painted) {
        pa.paints = a.table + 6u * ((size_t)n + 1u) + 7u * (size_t)n;
        pa.frag_bits = (const uint32_t *)c->frag_masks.ptr;
        pa.masks = pa.frag_bits + c->fragments.size();
    }
    launch_compose_scene(a, painted ? &pa : nullptr, st);
    HIP_TRY(c, hipGetLastError());
    return 0;
}

// The index of the shared scene (SceneIndex, ctx.h), built where the upload already blocks: the pathtag scan into the index's
// arrays -- with lane 0's zero region, which is idle and sized for the scene, as its control block and look-back state -- then
// k_scene_index_lists, and the lengths and the verdict read back.  Scenes small enough for k_front are not indexed: their stages
// share launches, and launches are what they cost.  A scan whose look-back gave up leaves the scene without an index.
int build_scene_index(vello_hip_ctx *c) {
    SceneSlot &sc = c->shared;
    const vello_hip_layout &L = sc.layout;
    SceneIndex &ix = sc.index;
    ix.valid = false;
    if ((sc.n_tag_words * 4u <= FRONT_MAX_TAGS && L.n_draw_objects <= FRONT_MAX_DRAW_OBJECTS && L.n_paths <= FRONT_MAX_DRAW_OBJECTS) ||
        L.n_paths > 0x40000000u)  // (k_frame_begin counts the boxes in 8-byte words)
        return 0;
    Lane &l = c->lanes[0];
    hipStream_t st = l.stream;
    const size_t n_tags = (size_t)sc.n_tag_words * 4u;
    int r;
    if ((r = ensure(c, ix.monoids, (size_t)(sc.n_tag_words + 4u) * sizeof(TagMonoid)))) return r;
    if ((r = ensure(c, ix.bboxes, (size_t)(L.n_paths + 1u) * sizeof(PathBbox)))) return r;
    if ((r = ensure(c, ix.lists, 3u * n_tags * 4u))) return r;
    if ((r = ensure(c, ix.counts, 16))) return r;
    Frame f{};
    std::memcpy(&f.cfg.layout, &L, sizeof(Layout));
    f.n_tag_words = sc.n_tag_words;
    f.n_scene_words = (uint32_t)(sc.scene_len / 4u);
    f.scene = (const uint32_t *)sc.scene.ptr;
    f.control = (Control *)l.zero_region.ptr;
    f.pathtag_state = (unsigned long long *)((char *)l.zero_region.ptr + sizeof(Control));
    f.tag_monoids = (TagMonoid *)ix.monoids.ptr;
    f.path_bboxes = (PathBbox *)ix.bboxes.ptr;
    HIP_TRY(c, hipMemsetAsync(l.zero_region.ptr, 0, sc.zero_bytes, st));
    HIP_TRY(c, hipMemsetAsync(ix.counts.ptr, 0, 16, st));
    launch_pathtag_scan(f, st);
    launch_scene_index_lists(f, (uint32_t *)ix.lists.ptr, (uint32_t *)ix.counts.ptr, st);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(st));
    uint32_t counts[4], failed = 0u;
    HIP_TRY(c, hipMemcpy(counts, ix.counts.ptr, sizeof counts, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(&failed, l.zero_region.ptr, 4, hipMemcpyDeviceToHost));  // (bump.failed: the control block's first word)
    if ((failed & ~FAILED_SCENE) != 0u) return 0;
    ix.failed = failed;
    ix.n_fill = counts[0], ix.n_strokes = counts[1], ix.n_lines = counts[2];
    ix.valid = true;
    c->scene_index_builds++;
    return 0;
}

}  // namespace

namespace vk {

// The retained instance list goes with the fragment table it was composed from (the callers have waited for the frames in flight).
// Its buffers stay for the next list; vello_hip_release_retained frees them.
void drop_retained(vello_hip_ctx *c) {
    c->have_retained = false;
    c->retained.resident = false;
    c->retained_n = 0;
}

// Validates the layout, sizes the slot and copies scene + ramps on `st`; returns once the source buffers may be
// reused (they are caller-owned only for the duration of the call, recording.rs:124-129).
int load_slot(vello_hip_ctx *c, SceneSlot &sc, hipStream_t st, const uint8_t *scene, size_t scene_len,
                     const vello_hip_layout *layout, const uint32_t *ramps, uint32_t n_ramps) {
    int r;
    if ((r = check_layout(c, scene, scene_len, layout))) return r;
    const vello_hip_layout &L = *layout;
    if ((r = size_slot(c, sc, L, scene_len))) return r;
    {
        // The same pass checks what draw_leaf / clip_leaf will index with (shared/drawtag.wgsl:47-54: bit 0 = clip,
        // bits 2-4 = draw data words, bits 6-9 = info words).  WebGPU's robust buffer access absorbs an inconsistent
        // stream upstream; here it must be refused.  (The path tag stream is checked by the pathtag scan, on the GPU.)
        const uint32_t *words_p = reinterpret_cast<const uint32_t *>(scene);
        uint64_t draw_data_words = 0, info_words = 0, clip_tags = 0;
        for (uint32_t i = 0; i < L.n_draw_objects; i++) {
            uint32_t t = words_p[L.draw_tag_base + i];
            if (t != DRAWTAG_FILL_COLOR && t != DRAWTAG_BEGIN_CLIP && t != DRAWTAG_END_CLIP && t != DRAWTAG_NOP) sc.brushes = true;
            clip_tags += t & 1u;
            draw_data_words += (t >> 2) & 0x7u;
            info_words += (t >> 6) & 0xfu;
        }
        // clip_tags == n_clips, not <=: k_clip walks n_clips entries of clip_inp and draw_leaf writes one per clip tag
        // (resolve counts exactly the BEGIN/END_CLIP tags below n_draw_objects: the END_CLIPs it appends for unclosed
        // layers lie behind them, resolve.rs:139-141); fewer tags would leave entries uninitialised
        if (draw_data_words > (uint64_t)(L.transform_base - L.draw_data_base) || info_words > L.bin_data_start || clip_tags != L.n_clips ||
            L.n_draw_objects > L.n_paths) {
            c->last_error = "draw tags need more draw data / info words / paths than the layout provides, or their clip count differs from n_clips";
            return VELLO_HIP_E_INVALID;
        }
    }
    if (&sc == &c->shared) {
        // a segment tag whose points are pairs of i16 (path_tag.rs: PATH_TAG_F32 clear): such a scene's path-data words cannot be
        // blended as floats (vello_hip_render_resident_morphed, rule 4).  Only the shared slot's frames can be morphed, so only its
        // uploads look.  Four tags a word, no branch and no early exit -- an OR over the stream that the compiler vectorises: bit 0 of
        // every byte of `seg` is "a segment" (either bit of the type field), of `f32` PATH_TAG_F32.
        static_assert(PATH_TAG_SEG_TYPE == 3u && PATH_TAG_F32 == 8u, "the bit tricks below");
        const uint8_t *tags = scene + (size_t)L.path_tag_base * 4u;
        const size_t n_words = (size_t)L.path_data_base - L.path_tag_base;
        uint32_t any = 0u;
        for (size_t i = 0; i < n_words; i++) {
            uint32_t w;
            std::memcpy(&w, tags + i * 4u, 4);
            const uint32_t seg = (w | (w >> 1)) & 0x01010101u, f32 = (w >> 3) & 0x01010101u;
            any |= seg & ~f32;
        }
        sc.i16_segments = any != 0u;
    }
    if (scene_len) HIP_TRY(c, hipMemcpyAsync(sc.scene.ptr, scene, scene_len, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemsetAsync((char *)sc.scene.ptr + scene_len, 0, 64, st));
    sc.n_ramps = 0;
    if (ramps && n_ramps) {
        if ((r = ensure(c, sc.ramps, (size_t)n_ramps * 512u * 4u))) return r;
        HIP_TRY(c, hipMemcpyAsync(sc.ramps.ptr, ramps, (size_t)n_ramps * 512u * 4u, hipMemcpyHostToDevice, st));
        sc.n_ramps = n_ramps;
    }
    HIP_TRY(c, hipStreamSynchronize(st));
    sc.resident = true;
    return VELLO_HIP_OK;
}

// Room for the per-lane copies of the shared scene's path-data stream (SceneSlot::pd_at), made at most once per resident scene: by
// vello_hip_upload_path_keyframes or by the first morphed frame.  The copies go behind the transform copies in the tail of the
// scene's allocation; where the tail is too short the scene moves into a larger allocation -- bytes, slack and transform copies as
// they are -- which waits for the frames in flight and counts as a scene allocation.  A buffer that has held a morphed scene of
// this size keeps its tail (ensure_scene never shrinks it): the next such scene allocates nothing.  VELLO_HIP_E_INVALID, nothing
// changed, for a scene whose copies would lie beyond a u32 word offset from its start.
int ensure_morph_room(vello_hip_ctx *c) {
    SceneSlot &sc = c->shared;
    if (sc.pd_sets != 0u) return 0;
    const uint32_t n = sc.layout.draw_tag_base - sc.layout.path_data_base;
    const uint64_t set_words = ((uint64_t)n + PD_SLACK_WORDS + 3u) & ~(uint64_t)3u;
    // (behind the transform copies and the style copies)
    const uint64_t pd_at = ((uint64_t)sc.st_at + (uint64_t)sc.st_set_words * sc.st_sets + 3u) & ~(uint64_t)3u;
    if (pd_at + set_words * MAX_LANES > 0xffffffffull) {
        c->last_error = "the scene is too large for per-frame path data (its bytes and copies together must lie within 2^32 words)";
        return VELLO_HIP_E_INVALID;
    }
    const size_t tail = (size_t)(pd_at - sc.view_at + set_words * MAX_LANES) * 4u;
    int r;
    if ((r = sync_all(c))) return r;
    if (sc.view_cap_bytes < tail) {
        const size_t at = sc.view_at * 4u;
        void *grown = nullptr;
        HIP_TRY(c, hipMalloc(&grown, at + tail + 256));
        const hipError_t e = hipMemcpy(grown, sc.scene.ptr, at + sc.view_cap_bytes, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) {
            (void)hipFree(grown);
            c->last_error = std::string("path-data copies: ") + hipGetErrorString(e);
            return VELLO_HIP_E_HIP;
        }
        HIP_TRY(c, hipFree(sc.scene.ptr));
        sc.scene.ptr = grown;
        sc.view_cap_bytes = tail;
        c->scene_allocations++;
    }
    // every copy's slack: the words that follow the stream in the scene (the scene's own slack makes them PD_SLACK_WORDS)
    uint32_t *words = (uint32_t *)sc.scene.ptr;
    for (uint32_t k = 0; k < MAX_LANES; k++)
        HIP_TRY(c, hipMemcpy(words + pd_at + k * set_words + n, words + sc.layout.draw_tag_base, PD_SLACK_WORDS * 4u, hipMemcpyDeviceToDevice));
    sc.pd_at = (size_t)pd_at;
    sc.pd_set_words = (uint32_t)set_words;
    sc.pd_sets = MAX_LANES;
    return 0;
}

}  // namespace vk

extern "C" {

uint32_t vello_hip_path_data_words(vello_hip_ctx *c) {
    return c && c->shared.resident ? c->shared.layout.draw_tag_base - c->shared.layout.path_data_base : 0u;
}

// Keyframes for vello_hip_render_resident_morphed: copied once into a buffer of the context's; the frames that may still read the
// set this one replaces are waited for, as an upload waits.  Everything that can refuse the call is asked before anything changes.
int vello_hip_upload_path_keyframes(vello_hip_ctx *c, const uint32_t *words, uint32_t n_keys, uint32_t n_words) {
    if (!c) return VELLO_HIP_E_INVALID;
    auto refuse = [&](const char *why) {
        c->last_error = std::string("upload_path_keyframes: ") + why;
        return VELLO_HIP_E_INVALID;
    };
    if (!c->shared.resident) return refuse("no scene uploaded");
    if (n_words != vello_hip_path_data_words(c)) return refuse("n_words is not vello_hip_path_data_words of the resident scene");
    if (n_keys > 0u && !words) return refuse("words is NULL");
    HIP_TRY(c, hipSetDevice(c->device));
    int r;
    if ((r = sync_all(c))) return r;
    if (n_keys == 0u) {
        c->n_keys = 0u;
        return VELLO_HIP_OK;
    }
    if ((r = ensure_morph_room(c))) return r;
    // on the device a keyframe begins on a 16-byte boundary whatever its length, so that k_path_blend reads every one of them with
    // 16-byte accesses: rows of key_stride words
    const uint32_t stride = (uint32_t)(((uint64_t)n_words + 3u) & ~(uint64_t)3u);
    const size_t bytes = (size_t)n_keys * stride * 4u;
    // from here on a failure leaves no keyframes
    c->n_keys = 0u;
    if ((r = ensure(c, c->keyframes, bytes ? bytes : 16u))) return r;
    if (n_words)
        HIP_TRY(c, hipMemcpy2D(c->keyframes.ptr, (size_t)stride * 4u, words, (size_t)n_words * 4u, (size_t)n_words * 4u, n_keys, hipMemcpyHostToDevice));
    c->key_stride = stride;
    c->n_keys = n_keys;
    return VELLO_HIP_OK;
}

int vello_hip_upload_scene(vello_hip_ctx *c, const uint8_t *scene, size_t scene_len, const vello_hip_layout *layout,
                           const uint32_t *ramps, uint32_t n_ramps) {
    if (!c) return VELLO_HIP_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    int r;
    // frames still in flight read the old scene
    if ((r = sync_all(c))) return r;
    c->have_fragments = false;  // (vello_hip_upload_fragments sets its table once the scene is resident)
    c->n_keys = 0u;             // (path keyframes speak for the scene they were uploaded for)
    c->have_masks = false;
    c->frag_masks_host.clear();
    c->fragments.clear();
    drop_retained(c);
    if ((r = load_slot(c, c->shared, c->lanes[0].stream, scene, scene_len, layout, ramps, n_ramps))) return r;
    for (auto &l : c->lanes) {
        l.which = LaneScene::Shared;
        if ((r = alloc_lane_scene(c, l, c->shared))) return r;
    }
    // (the lanes are idle and sized for the scene: the index's scan borrows lane 0's zero region)
    if ((r = build_scene_index(c))) {
        c->shared.resident = false;
        return r;
    }
    return VELLO_HIP_OK;
}

uint64_t vello_hip_scene_allocations(vello_hip_ctx *c) { return c ? c->scene_allocations : 0u; }
uint64_t vello_hip_scene_index_builds(vello_hip_ctx *c) { return c ? c->scene_index_builds : 0u; }

int vello_hip_upload_fragments(vello_hip_ctx *c, const uint8_t *scene, size_t scene_len, const vello_hip_layout *layout, const uint32_t *ramps,
                               uint32_t n_ramps, const vello_hip_fragment *frags, uint32_t n_frags) {
    if (!c) return VELLO_HIP_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    // whatever goes wrong from here on, nothing stays resident (frames in flight keep what they were enqueued with)
    c->shared.resident = false;
    c->have_fragments = false;
    c->n_keys = 0u;
    c->have_masks = false;
    c->frag_masks_host.clear();
    c->fragments.clear();
    drop_retained(c);
    if (n_frags > 0u && !frags) {
        c->last_error = "upload_fragments: frags is NULL";
        return VELLO_HIP_E_INVALID;
    }
    int r;
    if ((r = check_layout(c, scene, scene_len, layout))) return r;
    std::vector<FragmentInfo> infos(n_frags);
    // [n_frags] bit offsets, then the colour-word masks (ctx::frag_masks); bit offsets stay within u32 or no masks are kept
    std::vector<uint32_t> masks;
    uint64_t mask_bits = 0;
    // (known before the walk: a library that takes no paints never has its bit array built)
    uint64_t total_bits = 0;
    for (uint32_t i = 0; i < n_frags; i++)
        if (frags[i].draw_data[0] <= frags[i].draw_data[1]) total_bits += frags[i].draw_data[1] - frags[i].draw_data[0];
    bool keep_masks = total_bits <= 0xffffffffull;
    for (uint32_t i = 0; i < n_frags; i++) {
        if ((r = check_fragment(c, scene, scene_len, *layout, frags[i], i, infos[i], keep_masks ? &masks : nullptr, mask_bits))) return r;
        mask_bits += infos[i].len[3];
        if (mask_bits > 0xffffffffull) keep_masks = false, masks = {};
    }
    if ((r = vello_hip_upload_scene(c, scene, scene_len, layout, ramps, n_ramps))) return r;
    // (the lanes are idle: upload_scene waited for them, so no frame reads the table that ensure() may free)
    std::vector<uint32_t> begins((size_t)n_frags * 6u);
    for (uint32_t i = 0; i < n_frags; i++) std::memcpy(&begins[(size_t)i * 6u], infos[i].begin, sizeof infos[i].begin);
    if ((r = ensure(c, c->frag_table, begins.size() * 4u))) {
        c->shared.resident = false;
        return r;
    }
    if (n_frags) {
        const hipError_t e = hipMemcpy(c->frag_table.ptr, begins.data(), begins.size() * 4u, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            c->shared.resident = false;
            c->last_error = std::string("upload_fragments: ") + hipGetErrorString(e);
            return VELLO_HIP_E_HIP;
        }
    }
    if (keep_masks) {
        std::vector<uint32_t> block((size_t)n_frags + masks.size());
        for (uint32_t i = 0; i < n_frags; i++) block[i] = infos[i].mask_bit;
        if (!masks.empty()) std::memcpy(&block[n_frags], masks.data(), masks.size() * 4u);
        if ((r = ensure(c, c->frag_masks, block.size() * 4u))) {
            c->shared.resident = false;
            return r;
        }
        if (!block.empty()) {
            const hipError_t e = hipMemcpy(c->frag_masks.ptr, block.data(), block.size() * 4u, hipMemcpyHostToDevice);
            if (e != hipSuccess) {
                c->shared.resident = false;
                c->last_error = std::string("upload_fragments: ") + hipGetErrorString(e);
                return VELLO_HIP_E_HIP;
            }
        }
    }
    c->fragments = std::move(infos);
    c->have_fragments = true;
    c->have_masks = keep_masks;
    if (keep_masks) c->frag_masks_host = std::move(masks);  // (vello_hip_upload_scene above cleared it)
    return VELLO_HIP_OK;
}

int vello_hip_instances_layout(vello_hip_ctx *c, const vello_hip_instance *inst, uint32_t n, vello_hip_layout *layout_out, size_t *scene_len_out) {
    if (!c) return VELLO_HIP_E_INVALID;
    ComposePlan p;
    if (int r = plan_instances(c, inst, nullptr, n, p)) return r;
    if (layout_out) *layout_out = p.layout;
    if (scene_len_out) *scene_len_out = p.scene_len;
    return VELLO_HIP_OK;
}

// vello_hip_render_frame with k_compose_scene in the host copy's place.  Everything that can refuse the frame is asked before the
// lane is taken; the instance table goes through a pinned block to the lane's own table, on the lane's stream, ahead of the kernel.
// With a paint list the table carries it behind the transforms and the kernel's painted form runs; without one, the table, the
// arguments and the kernel are the unpainted frame's.
int vello_hip_render_instances_painted(vello_hip_ctx *c, const vello_hip_instance *inst, const vello_hip_paint *paints, uint32_t n,
                                       const vello_hip_render_params *params, void *out_device, size_t out_stride) {
    if (!c || !params) return VELLO_HIP_E_INVALID;
    ComposePlan p;
    int r = plan_instances(c, inst, paints, n, p);
    if (r) return r;
    if ((r = check_target(c, params, out_device, out_stride, true))) return r;
    const size_t table_bytes = compose_table_words(n, paints != nullptr) * 4u;
    Staging *st = nullptr;
    const auto set_up = [&](Lane &l, bool &) -> int {
        HIP_TRY(c, hipStreamSynchronize(l.stream));
        // The slot holds no scene until the frame is enqueued: a failure on the way leaves the lane without one, not with a
        // composed scene whose bytes were never written.
        l.own.resident = false;
        if (int sr = size_slot(c, l.own, p.layout, p.scene_len)) return sr;
        l.own.brushes = p.brushes;
        l.own.composed = true;
        l.own.n_ramps = 0;
        l.which = LaneScene::Own;
        return 0;
    };
    const auto staged = [&](Lane &l) -> int {
        if (int sr = acquire_staging(c, table_bytes, st)) return sr;
        if (int sr = ensure(c, l.compose_table, table_bytes)) return sr;
        l.own.resident = true;  // (prepare_frame asks for it)
        return 0;
    };
    // the instance table and k_compose_scene, ahead of the stages
    const auto enqueue = [&](Lane &l) -> int {
        // the Config was not sent (a blocking copy): VELLO_HIP_BUF_CONFIG gets it when it is next read or written
        c->cfg_unsent = true;
        fill_compose_table(c, inst, paints, n, (uint32_t *)st->host);
        l.own.resident = false;
        HIP_TRY(c, hipMemcpyAsync(l.compose_table.ptr, st->host, table_bytes, hipMemcpyHostToDevice, l.stream));
        HIP_TRY(c, hipEventRecord(st->done, l.stream));
        st->busy = true;
        if (int lr = launch_compose(c, p, n, paints != nullptr, (const uint32_t *)l.compose_table.ptr, (uint32_t *)l.own.scene.ptr, l.stream)) return lr;
        l.own.resident = true;
        l.compose_n = n;
        return 0;
    };
    // (the rotation moves only once nothing can refuse the frame)
    return enter_frame(c, params, out_device, out_stride, false, VELLO_HIP_STAGE_FINE, set_up, staged, enqueue);
}

int vello_hip_render_instances(vello_hip_ctx *c, const vello_hip_instance *inst, uint32_t n, const vello_hip_render_params *params, void *out_device,
                               size_t out_stride) {
    return vello_hip_render_instances_painted(c, inst, nullptr, n, params, out_device, out_stride);
}

// The instance list composed ONCE into the context's retained slot.  Five streams are k_compose_scene's (its painted form with a
// paint list), as an instance frame's; the transform stream is then written over from the host with the library's entries
// verbatim -- copied, not multiplied by an identity, which would turn a -0 into +0 -- and, in the same pass over the list, the host
// builds the table that names each entry's instance and collects the rest poses.  Runs once per list: blocking copies, and it waits
// for the frames in flight, which may be reading the list it replaces.
int vello_hip_retain_instances(vello_hip_ctx *c, const vello_hip_instance *inst, const vello_hip_paint *paints, uint32_t n) {
    if (!c) return VELLO_HIP_E_INVALID;
    ComposePlan p;
    int r = plan_instances(c, inst, paints, n, p);
    if (r) return r;
    if ((uint64_t)n * 6u > 0xffffffffull) {  // (k_instance_transforms indexes the poses in u32 words)
        c->last_error = "retain_instances: more than 2^32 / 6 instances";
        return VELLO_HIP_E_INVALID;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    if ((r = sync_all(c))) return r;
    // from here on a failure leaves no list retained
    drop_retained(c);
    SceneSlot &sc = c->retained;
    if ((r = size_slot(c, sc, p.layout, p.scene_len))) return r;
    sc.brushes = p.brushes;
    sc.composed = true;
    sc.n_ramps = 0;
    const uint32_t n_xf = p.len[4] / 6u;
    // the table, the transform stream as the library holds it, the owners, the rest poses
    std::vector<uint32_t> table(compose_table_words(n, paints != nullptr));
    fill_compose_table(c, inst, paints, n, table.data());
    std::vector<uint32_t> lib_xf(c->shared.layout.style_base - c->shared.layout.transform_base), xf(p.len[4]), owner(n_xf), rest((size_t)n * 6u);
    if (!lib_xf.empty())
        HIP_TRY(c, hipMemcpy(lib_xf.data(), (const uint32_t *)c->shared.scene.ptr + c->shared.layout.transform_base, lib_xf.size() * 4u, hipMemcpyDeviceToHost));
    size_t at = 0;
    for (uint32_t i = 0; i < n; i++) {
        const FragmentInfo &fi = c->fragments[inst[i].fragment];
        if (fi.len[4]) std::memcpy(&xf[at], &lib_xf[fi.begin[4]], (size_t)fi.len[4] * 4u);
        for (uint32_t e = 0; e < fi.len[4] / 6u; e++) owner[at / 6u + e] = i;
        at += fi.len[4];
        std::memcpy(&rest[(size_t)i * 6u], inst[i].transform, 24);
    }
    // the per-word table of k_instance_paints: for every draw-data word its instance, and bit 31 where the fragment's mask has the
    // word as a colour word (n <= 2^32 / 6 leaves the bit free).  A library without masks takes no paints: no table.
    std::vector<uint32_t> ddmap(c->have_masks ? p.len[3] : 0u);
    if (c->have_masks) {
        size_t w = 0;
        for (uint32_t i = 0; i < n; i++) {
            const FragmentInfo &fi = c->fragments[inst[i].fragment];
            for (uint32_t k = 0; k < fi.len[3]; k++) {
                const uint32_t bit = fi.mask_bit + k;
                ddmap[w++] = i | (((c->frag_masks_host[bit >> 5] >> (bit & 31u)) & 1u) != 0u ? DD_MAP_COLOUR : 0u);
            }
        }
    }
    DevBuf table_dev;  // (freed on the way out: the list is composed once)
    if ((r = ensure(c, table_dev, table.size() * 4u))) return r;
    if ((r = ensure(c, c->retained_owner, owner.size() * 4u))) return r;
    if ((r = ensure(c, c->retained_rest, rest.size() * 4u))) return r;
    if ((r = ensure(c, c->retained_prefix, ((size_t)n + 1u) * 4u))) return r;
    if ((r = ensure(c, c->retained_ddmap, ddmap.size() * 4u))) return r;
    hipStream_t st = c->lanes[0].stream;
    HIP_TRY(c, hipMemcpy(table_dev.ptr, table.data(), table.size() * 4u, hipMemcpyHostToDevice));
    if ((r = launch_compose(c, p, n, paints != nullptr, (const uint32_t *)table_dev.ptr, (uint32_t *)sc.scene.ptr, st))) return r;
    HIP_TRY(c, hipStreamSynchronize(st));
    if (!xf.empty()) HIP_TRY(c, hipMemcpy((uint32_t *)sc.scene.ptr + p.layout.transform_base, xf.data(), xf.size() * 4u, hipMemcpyHostToDevice));
    if (!owner.empty()) HIP_TRY(c, hipMemcpy(c->retained_owner.ptr, owner.data(), owner.size() * 4u, hipMemcpyHostToDevice));
    if (!rest.empty()) HIP_TRY(c, hipMemcpy(c->retained_rest.ptr, rest.data(), rest.size() * 4u, hipMemcpyHostToDevice));
    if (!ddmap.empty()) HIP_TRY(c, hipMemcpy(c->retained_ddmap.ptr, ddmap.data(), ddmap.size() * 4u, hipMemcpyHostToDevice));
    // (the table's third row: the exclusive prefix of the instances' draw-tag counts, n + 1 entries)
    HIP_TRY(c, hipMemcpy(c->retained_prefix.ptr, table.data() + 2u * ((size_t)n + 1u), ((size_t)n + 1u) * 4u, hipMemcpyHostToDevice));
    // the lanes that showed the list this one replaces: their scene-dependent buffers must fit the new one
    for (auto &l : c->lanes)
        if (l.which == LaneScene::Retained && (r = alloc_lane_scene(c, l, sc))) return r;
    c->retained_n = n;
    sc.resident = true;
    c->have_retained = true;
    return VELLO_HIP_OK;
}

int vello_hip_release_retained(vello_hip_ctx *c) {
    if (!c) return VELLO_HIP_E_INVALID;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int r = sync_all(c)) return r;
    drop_retained(c);
    for (DevBuf *b : {&c->retained.scene, &c->retained_owner, &c->retained_rest, &c->retained_prefix, &c->retained_ddmap}) {
        if (b->ptr) HIP_TRY(c, hipFree(b->ptr));
        b->ptr = nullptr;
        b->size = 0;
    }
    c->retained.view_cap_bytes = 0;
    c->retained.view_sets = 0;
    c->retained.st_sets = 0;
    c->retained.dd_sets = 0;
    return VELLO_HIP_OK;
}

}  // extern "C"
