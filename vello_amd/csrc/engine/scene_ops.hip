// Device-side operations on scene data outside the pipeline's stages: atlas copies, the view's transform words, a retained list's
// per-frame transform and draw-data words, a morphed frame's path-data words, a stroke scale's style words, scene composition.
#include "engine.h"

namespace vk {

// k_atlas_copy: the rectangles of one vello_hip_copy_images_device call as ONE concatenated texel space, cut into chunks of
// `steps` x 256 texels, a chunk per workgroup.  Lane i of a wave takes texel base + i, so a wave reads and writes 64
// consecutive dwords of a row (or the tail of one row and the head of the next); a thousand 16x16 sprites are 1 000
// workgroups of full waves, not 16 000 rows of quarter waves, and a 4K frame is 2 000 workgroups.  A thread finds its
// first texel's rectangle by binary search over the host's prefix and walks on from there by the 256-texel step.
// Plain dword accesses: the atlas x is arbitrary, so a destination row is only 4-byte aligned.
constexpr uint32_t ATLAS_COPY_MAX_STEPS = 16u, ATLAS_COPY_TARGET_WGS = 2048u;

__global__ void __launch_bounds__(256) k_atlas_copy(const AtlasCopyDesc *__restrict__ descs, uint32_t n, uint64_t total, uint32_t steps,
                                                    uint32_t *__restrict__ atlas, uint32_t atlas_w) {
    uint64_t t = (uint64_t)blockIdx.x * steps * 256u + threadIdx.x;
    if (t >= total) return;
    uint32_t lo = 0u, hi = n - 1u;  // the last entry whose first <= t
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1u) >> 1;
        if (descs[mid].first <= t) lo = mid;
        else hi = mid - 1u;
    }
    uint32_t r = lo;
    AtlasCopyDesc d = descs[r];
    uint64_t local = t - d.first;
    for (uint32_t k = 0; k < steps && t < total; k++, t += 256u, local += 256u) {
        uint64_t size = (uint64_t)d.width * d.height;
        while (local >= size) {  // (t < total: a later entry holds it; every entry of the table holds texels)
            local -= size;
            d = descs[++r];
            size = (uint64_t)d.width * d.height;
        }
        const uint32_t li = (uint32_t)local;  // < width * height <= 65535^2
        const uint32_t row = li / d.width, col = li - row * d.width;
        const uint32_t v = *(const uint32_t *)(uintptr_t)(d.src + (uint64_t)row * d.src_stride + (uint64_t)col * 4u);
        atlas[d.dst + (uint64_t)row * atlas_w + col] = v;
    }
}

void launch_atlas_copy(const AtlasCopyDesc *descs, uint32_t n, uint64_t total, uint32_t *atlas, uint32_t atlas_w, hipStream_t s) {
    // enough steps per workgroup that the grid stays near ATLAS_COPY_TARGET_WGS (8 per CU), at most ATLAS_COPY_MAX_STEPS
    uint64_t steps = (total + 256u * ATLAS_COPY_TARGET_WGS - 1u) / (256u * ATLAS_COPY_TARGET_WGS);
    steps = steps < 1u ? 1u : steps > ATLAS_COPY_MAX_STEPS ? ATLAS_COPY_MAX_STEPS : steps;
    const uint64_t wgs = (total + steps * 256u - 1u) / (steps * 256u);
    hipLaunchKernelGGL(k_atlas_copy, dim3((uint32_t)wgs), dim3(256), 0, s, descs, n, total, (uint32_t)steps, atlas, atlas_w);
}

// k_view_transforms: the view transform of vello_hip_set_view_transform composed into a frame's own copy of the transform stream, a
// lane per entry.  Slot i of `out` is entry i - 1: slot 0 is the six words BELOW the stream, copied verbatim (a path encoded before any
// transform reads them, read_transform in common.h; zeros when the scene has no six words there -- the pathtag scan then hands out no
// index -1), slots 1 .. n_xf are V.T as vello_encoding's Transform::mul computes it (math.rs:51-73): f32, every product and every sum
// rounded on its own (the tree is built without fp contraction), in this operand order and association.  Six dword loads and six
// dword stores per lane at a stride of 24 bytes: the stream is 4-byte aligned only, and a wave's 64 entries are 1.5 KB of
// consecutive memory either way.  The kernel reads the scene and writes the copy; nothing else of the frame runs beside it on
// the lane's stream.
__global__ void __launch_bounds__(256) k_view_transforms(const uint32_t *__restrict__ scene, uint32_t transform_base, uint32_t n_xf, Xform v,
                                                         uint32_t *__restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i > n_xf) return;
    uint32_t *o = out + (size_t)i * 6u;
    if (i == 0u) {
        const bool below = transform_base >= 6u;
#pragma unroll
        for (uint32_t k = 0; k < 6u; k++) o[k] = below ? scene[transform_base - 6u + k] : 0u;
        return;
    }
    const Xform t = read_transform(scene, transform_base, i - 1u);
    const float m0 = v.m0 * t.m0 + v.m2 * t.m1, m1 = v.m1 * t.m0 + v.m3 * t.m1;
    const float m2 = v.m0 * t.m2 + v.m2 * t.m3, m3 = v.m1 * t.m2 + v.m3 * t.m3;
    const float t0 = (v.m0 * t.t0 + v.m2 * t.t1) + v.t0, t1 = (v.m1 * t.t0 + v.m3 * t.t1) + v.t1;
    o[0] = __float_as_uint(m0);
    o[1] = __float_as_uint(m1);
    o[2] = __float_as_uint(m2);
    o[3] = __float_as_uint(m3);
    o[4] = __float_as_uint(t0);
    o[5] = __float_as_uint(t1);
}

void launch_view_transforms(const Frame &f, hipStream_t s) {
    const uint32_t n_xf = (f.cfg.layout.style_base - f.cfg.layout.transform_base) / 6u;
    // (slot 0 of the copy is entry -1: six words in front of xf_base)
    hipLaunchKernelGGL(k_view_transforms, dim3((n_xf + 1u + 255u) / 256u), dim3(256), 0, s, f.scene, f.cfg.layout.transform_base, n_xf, f.view,
                       const_cast<uint32_t *>(f.scene) + (f.xf_base - 6u));
}

// a . b as vello_encoding's Transform::mul computes it (math.rs:51-73) -- k_view_transforms' arithmetic: f32, every product and every
// sum rounded on its own, in this operand order and association
__device__ __forceinline__ Xform xform_mul(const Xform &a, const Xform &b) {
    Xform r;
    r.m0 = a.m0 * b.m0 + a.m2 * b.m1;
    r.m1 = a.m1 * b.m0 + a.m3 * b.m1;
    r.m2 = a.m0 * b.m2 + a.m2 * b.m3;
    r.m3 = a.m1 * b.m2 + a.m3 * b.m3;
    r.t0 = (a.m0 * b.t0 + a.m2 * b.t1) + a.t0;
    r.t1 = (a.m1 * b.t0 + a.m3 * b.t1) + a.t1;
    return r;
}

// k_instance_transforms: the composed transform words of a frame of the retained instance list (vello_hip_render_retained; the
// arguments are in engine.h), a lane per transform entry as k_view_transforms -- which it replaces for such a frame.  Slot 0 of `out`
// is the six words below the retained scene's transform stream, verbatim; slot e + 1 is X.T_e with X the pose of the instance that
// owns entry e, rounded to six f32 words, and with a view View.(X.T_e): both products in this one kernel, each by xform_mul.
// A lane reads its owner with its neighbours' (one coalesced dword load a wave), the six words of T at the 24-byte stride
// k_view_transforms reads them at (a wave's entries are 1.5 KB of consecutive memory) and the six words of its owner's pose: owners do
// not decrease along the stream, so a wave's poses are the poses of a run of instances -- one or two cache lines where an instance
// holds several entries, 1.5 KB read like T where every instance holds one.  Dword accesses throughout: stream, poses and copy
// are 4-byte aligned only.  No LDS: nothing is shared beyond what the cache holds.
// Where the poses are the caller's device memory (Frame::pose_check) the same grid tests them: lane i < n tests pose i, whether or
// not instance i owns an entry, and a NaN or an infinity ORs FAILED_SCENE into the frame's bump.failed -- that launch sits behind
// the frame's zero fill and ahead of its pathtag scan, so the frame is discarded as one whose tag stream contradicts its scene.
// `failed` is null for host poses and the rest poses, which the host has tested: no test, and the grid covers the entries only.
__global__ void __launch_bounds__(256) k_instance_transforms(InstanceXfArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (a.failed != nullptr && i < a.n) {
        const uint32_t *p = a.poses + (size_t)i * 6u;
        bool finite = true;
#pragma unroll
        for (uint32_t k = 0; k < 6u; k++) finite = finite && (p[k] & 0x7f800000u) != 0x7f800000u;
        if (!finite) atomicOr(a.failed, FAILED_SCENE);
    }
    if (i > a.n_xf) return;
    uint32_t *o = a.out + (size_t)i * 6u;
    if (i == 0u) {
        const bool below = a.transform_base >= 6u;
#pragma unroll
        for (uint32_t k = 0; k < 6u; k++) o[k] = below ? a.scene[a.transform_base - 6u + k] : 0u;
        return;
    }
    const uint32_t owner = a.owner[i - 1u];  // < n: the host built the table from the list it retained
    const Xform t = read_transform(a.scene, a.transform_base, i - 1u);
    const Xform x = read_transform(a.poses, 0u, owner);
    Xform r = xform_mul(x, t);
    if (a.has_view) r = xform_mul(a.view, r);
    o[0] = __float_as_uint(r.m0);
    o[1] = __float_as_uint(r.m1);
    o[2] = __float_as_uint(r.m2);
    o[3] = __float_as_uint(r.m3);
    o[4] = __float_as_uint(r.t0);
    o[5] = __float_as_uint(r.t1);
}

void launch_instance_transforms(const Frame &f, bool check_poses, hipStream_t s) {  // check_poses: Frame::pose_check, behind the zero fill
    InstanceXfArgs a{};
    a.scene = f.scene;
    a.owner = f.xf_owner;
    a.poses = f.pose_words;
    a.out = const_cast<uint32_t *>(f.scene) + (f.xf_base - 6u);  // (slot 0 of the copy is entry -1: six words in front of xf_base)
    a.failed = check_poses ? &f.control->bump.failed : nullptr;
    a.transform_base = f.cfg.layout.transform_base;
    a.n_xf = (f.cfg.layout.style_base - f.cfg.layout.transform_base) / 6u;
    a.n = f.n_instances;
    a.has_view = f.has_view ? 1u : 0u;
    a.view = f.view;
    // (n * 6 and n_xf * 6 are below 2^32: vello_hip_retain_instances)
    const uint32_t lanes = a.n_xf + 1u > (check_poses ? a.n : 0u) ? a.n_xf + 1u : a.n;
    hipLaunchKernelGGL(k_instance_transforms, dim3((lanes + 255u) / 256u), dim3(256), 0, s, a);
}

// k_instance_paints: the draw-data words of a PAINTED frame of the retained instance list (vello_hip_render_retained_painted; the
// arguments are in engine.h), a lane per draw-data word of the retained scene, beside k_instance_transforms at the head of the frame.
// Word w of `out` -- the lane's copy of the stream, which the draw stage and k_coarse_prep then read in the stream's place -- is the
// retained word, or paints[owner].rgba where the word is a colour word and its owner's paint is SOLID.  Which instance owns a word,
// and whether it is a colour word, is one entry of a table the host built when the list was retained (owner | colour << 31): a lane
// reads it with its neighbours' (one coalesced dword load a wave), as it reads the retained word and writes the copy.  Owners do not
// decrease along the stream, so the paints a wave reads are those of a run of instances: lanes of one instance read the same two
// words, and a wave of one-word fragments reads 512 consecutive bytes.  Only colour words read a paint at all.  Dword accesses
// throughout: paints and streams are 4-byte aligned only.  No LDS: nothing is shared beyond what the cache holds.  A wholesale
// copy rather than a list of the colour words alone: the readers take ONE base for the whole stream, and the non-colour words of a
// symbol map are a few words an instance.
// Where the paints are the caller's device memory (Frame::paint_check) the same grid tests them: lane i < n tests paint i, whether
// or not instance i owns a word, and a flags value other than KEEP or SOLID ORs FAILED_SCENE into the frame's bump.failed -- that
// launch sits behind the frame's zero fill and ahead of its pathtag scan, as k_instance_transforms' test of device poses does.
// `failed` is null for host paints, which the host has tested: no test, and the grid covers the words only.
__global__ void __launch_bounds__(256) k_instance_paints(InstancePaintArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (a.failed != nullptr && i < a.n) {
        if (a.paints[(size_t)i * 2u] > PAINT_SOLID) atomicOr(a.failed, FAILED_SCENE);
    }
    if (i >= a.n_words) return;
    const uint32_t m = a.map[i];
    uint32_t v = a.scene[(size_t)a.draw_data_base + i];
    if ((m & DD_MAP_COLOUR) != 0u) {
        const uint32_t *paint = a.paints + (size_t)(m & ~DD_MAP_COLOUR) * 2u;  // owner < n: the host built the table from the list it retained
        if (paint[0] == PAINT_SOLID) v = paint[1];
    }
    a.out[i] = v;
}

void launch_instance_paints(const Frame &f, bool check_paints, hipStream_t s) {
    InstancePaintArgs a{};
    a.scene = f.scene;
    a.map = f.dd_map;
    a.paints = f.paint_words;
    a.out = const_cast<uint32_t *>(f.scene) + f.dd_base;
    a.failed = check_paints ? &f.control->bump.failed : nullptr;
    a.draw_data_base = f.cfg.layout.draw_data_base;
    a.n_words = f.cfg.layout.transform_base - f.cfg.layout.draw_data_base;
    a.n = f.n_instances;
    const uint32_t lanes = a.n_words > (check_paints ? a.n : 0u) ? a.n_words : (check_paints ? a.n : 0u);
    if (lanes == 0u) return;  // (no draw data and nothing to test)
    hipLaunchKernelGGL(k_instance_paints, dim3((lanes + 255u) / 256u), dim3(256), 0, s, a);
}

// k_path_blend: the path-data words of a MORPHED frame of the resident scene (vello_hip_render_resident_morphed; the arguments are in
// engine.h), beside k_view_transforms at the head of the frame.  Word i of `out` -- the lane's copy of the stream, which flatten then
// reads in the stream's place -- is a[i], b[i] or a[i] + t * (b[i] - a[i]): f32, the difference, the product and the sum each rounded
// on its own (the tree is built without fp contraction, as k_view_transforms' arithmetic is), in this operand order.  The copy modes
// move bits: a NaN's payload and a zero's sign arrive as they were.  A plain streaming pass -- two reads and a write per word, one read
// in the copy modes; no LDS, nothing is shared -- over a grid capped at PATH_BLEND_MAX_WGS workgroups (eight per CU) that strides
// over the rest.  VEC: every address the mode touches is 16-byte aligned (the host has looked): lane l of a step takes the four words
// of one dwordx4 access, a wave 1 KB of consecutive memory per stream, and the up to three words behind the last whole quad are
// lanes 0 .. 2 of workgroup 0 with dword accesses.  !VEC (a keyframe whose length is no multiple of four, a tensor slice that starts
// one float in): a word a lane, 256 B a wave.  The mode is wave-uniform: a kernel argument.
__device__ __forceinline__ uint32_t path_blend_word(uint32_t a, uint32_t b, float t) {
    // __fsub_rn / __fmul_rn / __fadd_rn of the contract: in this toolchain they ARE the plain operators, in inline functions of a
    // header -- outside the reach of a pragma here, so without the Makefile's -ffp-contract=off they fuse.  The operators under the
    // pragma do not: built with no contraction flag at all (hipcc's default honours pragmas) this function has no fma where
    // k_view_transforms has four.  (An explicit -ffp-contract=fast overrides pragmas by definition.)
#pragma clang fp contract(off)
    const float fa = __uint_as_float(a), fb = __uint_as_float(b);
    const float d = fb - fa;
    const float p = t * d;
    return __float_as_uint(fa + p);
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_path_blend(PathBlendArgs g) {
    const uint32_t *__restrict__ const a = g.mode == PATH_BLEND_COPY_B ? g.b : g.a;  // (the ONE stream of a copy mode)
    const uint32_t *__restrict__ const b = g.b;
    uint32_t *__restrict__ const out = g.out;
    const bool mix = g.mode == PATH_BLEND_MIX;
    const uint32_t first = blockIdx.x * 256u + threadIdx.x, stride = gridDim.x * 256u;
    if (VEC) {
        const uint32_t n4 = g.n >> 2;
        const uint4 *a4 = reinterpret_cast<const uint4 *>(a), *b4 = reinterpret_cast<const uint4 *>(b);
        uint4 *o4 = reinterpret_cast<uint4 *>(out);
        for (uint32_t i = first; i < n4; i += stride) {
            uint4 v = a4[i];
            if (mix) {
                const uint4 w = b4[i];
                v = make_uint4(path_blend_word(v.x, w.x, g.t), path_blend_word(v.y, w.y, g.t), path_blend_word(v.z, w.z, g.t),
                               path_blend_word(v.w, w.w, g.t));
            }
            o4[i] = v;
        }
        const uint32_t i = (n4 << 2) + first;  // the words behind the last whole quad
        if (first < 3u && i < g.n) out[i] = mix ? path_blend_word(a[i], b[i], g.t) : a[i];
    } else {
        for (uint32_t i = first; i < g.n; i += stride) out[i] = mix ? path_blend_word(a[i], b[i], g.t) : a[i];
    }
}

void launch_path_blend(const Frame &f, hipStream_t s) {
    PathBlendArgs g{};
    g.a = f.pd_a;
    g.b = f.pd_b;
    g.out = const_cast<uint32_t *>(f.scene) + f.pd_base;
    g.n = f.cfg.layout.draw_tag_base - f.cfg.layout.path_data_base;
    g.mode = f.pd_mode;
    g.t = f.pd_t;
    if (g.n == 0u) return;  // (a scene without path data)
    // the scalar / vector split, decided here: the addresses of the streams the mode reads and of the copy
    uintptr_t bits = reinterpret_cast<uintptr_t>(g.out);
    if (g.mode != PATH_BLEND_COPY_B) bits |= reinterpret_cast<uintptr_t>(g.a);
    if (g.mode != PATH_BLEND_COPY_A) bits |= reinterpret_cast<uintptr_t>(g.b);
    const bool vec = (bits & 15u) == 0u;
    const uint32_t per_wg = vec ? PATH_BLEND_VEC_WORDS : 256u;
    uint32_t wgs = (uint32_t)(((uint64_t)g.n + per_wg - 1u) / per_wg);
    if (wgs > PATH_BLEND_MAX_WGS) wgs = PATH_BLEND_MAX_WGS;
    if (vec) hipLaunchKernelGGL(k_path_blend<true>, dim3(wgs), dim3(256), 0, s, g);
    else hipLaunchKernelGGL(k_path_blend<false>, dim3(wgs), dim3(256), 0, s, g);
}

// k_style_widths: the style words of a frame with a stroke scale (vello_hip_set_stroke_scale; the arguments are in engine.h), beside
// k_view_transforms at the head of the frame, a lane per style entry as that kernel takes a transform entry.  Entry e of `out` -- the
// lane's copy of the stream, which flatten then reads in the stream's place -- is (flags, w'): the flags verbatim, and
// w' = max(fl(w * scale), min_width) where the entry is a stroke of positive width, the bits of w everywhere else (a fill, a width
// of 0, a negative one, a NaN: the comparison w > 0 fails for all of them).  One f32 multiply and one compare; scale and min_width
// are kernel arguments, so wave-uniform.  VEC: stream and copy are both 8-byte aligned (the host has looked): one dwordx2 load and
// one dwordx2 store a lane, 512 B of consecutive memory a wave.  !VEC (a style stream that begins on an odd word): two dword loads
// and two dword stores at a stride of 8 bytes -- the same 512 B a wave.  Workgroup 0's first lane also writes slot -1, the two words
// in front of `out`: the two words below the scene's stream verbatim, which a segment met before any STYLE marker reads (zeros when
// the scene has no two words there -- a scene that short has no tags).  No LDS, nothing is shared.
__device__ __forceinline__ uint32_t style_width_word(uint32_t flags, uint32_t w_bits, float scale, float min_width) {
    // (a single operation -- nothing to contract -- under the file's discipline all the same: path_blend_word has the reasons)
#pragma clang fp contract(off)
    const float w = __uint_as_float(w_bits);
    if ((flags & STYLE_FLAGS_STYLE) == 0u || !(w > 0.0f)) return w_bits;
    const float x = w * scale;
    return __float_as_uint(x < min_width ? min_width : x);
}

template <bool VEC>
__global__ void __launch_bounds__(256) k_style_widths(StyleWidthArgs a) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e == 0u) {
        const bool below = a.style_base >= 2u;
        a.out[-2] = below ? a.scene[a.style_base - 2u] : 0u;
        a.out[-1] = below ? a.scene[a.style_base - 1u] : 0u;
    }
    if (e >= a.n_styles) return;
    const uint32_t *src = a.scene + (size_t)a.style_base + (size_t)e * 2u;
    uint32_t *dst = a.out + (size_t)e * 2u;
    if (VEC) {
        const uint64_t v = *reinterpret_cast<const uint64_t *>(src);  // (little endian: the flags are the low word)
        const uint32_t flags = (uint32_t)v;
        *reinterpret_cast<uint64_t *>(dst) = (uint64_t)style_width_word(flags, (uint32_t)(v >> 32), a.scale, a.min_width) << 32 | flags;
    } else {
        const uint32_t flags = src[0], w = src[1];
        dst[0] = flags;
        dst[1] = style_width_word(flags, w, a.scale, a.min_width);
    }
}

void launch_style_widths(const Frame &f, hipStream_t s) {
    StyleWidthArgs a{};
    a.scene = f.scene;
    a.out = const_cast<uint32_t *>(f.scene) + f.st_base;  // (slot -1 of the copy: two words in front of st_base)
    a.style_base = f.cfg.layout.style_base;
    a.n_styles = (f.n_scene_words - f.cfg.layout.style_base) / STYLE_SIZE_IN_WORDS;
    a.scale = f.stroke_scale;
    a.min_width = f.stroke_min;
    if (a.n_styles == 0u) return;  // (no style entry: no tag reads a style word, slot -1 included)
    // the access width, decided here: the scene's allocation is 256-byte aligned, so word parities are address parities -- the copy
    // begins on an even word (size_slot), the stream where the scene's layout puts it
    const bool vec = ((reinterpret_cast<uintptr_t>(a.scene + a.style_base) | reinterpret_cast<uintptr_t>(a.out)) & 7u) == 0u;
    const uint32_t wgs = (a.n_styles + 255u) / 256u;
    if (vec) hipLaunchKernelGGL(k_style_widths<true>, dim3(wgs), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_style_widths<false>, dim3(wgs), dim3(256), 0, s, a);
}

// k_compose_scene: a frame's packed scene written from instances of the library's fragments (vello_hip_render_instances; the contract is
// in include/vello_hip.h, the arguments in engine.h).  A thread per destination word, a workgroup per chunk of steps x 256 consecutive
// words of ONE stream, lane i of a wave on word base + i as in k_atlas_copy.  Which instance a word belongs to is a search for the last
// entry of the stream's prefix that is <= the word's offset (empty instances repeat an offset; the last one of a run is the one that
// holds words).  Fragments may be a dozen words long, so the search is the cost: threads 0 and 64 find the chunk's first and last
// instance in the table, the workgroup copies that slice of the prefix into LDS, and every thread searches the slice, from the
// instance of its previous word on.  The staging area holds an entry per word of the largest chunk plus two, which is every slice of
// a word stream without empty instances (an instance that holds words holds at least one).  A slice can be longer where empty
// instances lie in between and, in the tag stream, where fragments are shorter than four tags (a word holds up to four one-tag
// instances): such a chunk is not staged and its threads search the table itself.
//   word streams   a dword copy from the library;
//   transforms     word k of an entry needs two words of T and two or three of V: V.T as k_view_transforms computes it;
//   tags           byte-granular: where the four tags of a word come from one instance, two dword loads and a funnel shift; a word
//                  that straddles instances (or the stream's end) is put together from byte loads.  Words of the padding are zero.
// The body is shared by two kernels.  k_compose_scene is the unpainted frame's and takes ComposeArgs alone.  k_compose_scene_painted
// (vello_hip_render_instances_painted with a paint list) differs on the draw-data stream only: a lane whose instance is painted SOLID
// tests the colour-word mask bit of the library word it has just loaded -- the fragment's bit offset plus the word's offset in the
// fragment -- and writes the instance's rgba in the word's place where the bit is set.  The paint's two words and the mask word are
// loads at the instance's granularity: lanes of one instance read the same addresses.
constexpr uint32_t COMPOSE_LDS_OFFSETS = COMPOSE_MAX_STEPS * 256u + 2u;

template <bool PAINTED>
__device__ __forceinline__ void compose_scene(const ComposeArgs &a, const ComposePaintArgs &pa) {
    __shared__ uint32_t s_off[COMPOSE_LDS_OFFSETS];
    __shared__ uint32_t s_ends[2];
    const uint32_t bid = blockIdx.x, tid = threadIdx.x;
    uint32_t s = 0u;
#pragma unroll
    for (uint32_t k = 1u; k < 7u; k++) s += a.wg_first[k] <= bid ? 1u : 0u;  // (non-decreasing: the last stream that starts at or before bid)
    if (s == 6u) {
        if (tid < 16u) a.dst[(size_t)a.dst_base[5] + a.len[5] + tid] = 0u;
        return;
    }
    const uint32_t chunk = a.steps * 256u;
    const uint32_t lo = (bid - a.wg_first[s]) * chunk;                         // < len[s]: the host launches ceil(len / chunk) workgroups
    const uint32_t rem = a.len[s] - lo < chunk ? a.len[s] - lo : chunk;        // words of this chunk
    // the chunk in the units of the stream's prefix (bytes for tags: the host keeps the padded tag bytes within u32)
    const uint32_t ulo = s == 0u ? lo * 4u : lo;
    uint32_t uend = s == 0u ? (lo + rem) * 4u : lo + rem;
    if (s == 0u && uend > a.tag_bytes) uend = a.tag_bytes;
    const bool any = ulo < uend;  // (else: a chunk of the tags' padding)
    const uint32_t *off = a.table + (size_t)s * (a.n + 1u);
    const uint32_t *frag_of = a.table + 6u * ((size_t)a.n + 1u);
    if (any && (tid == 0u || tid == 64u)) {
        const uint32_t x = tid == 0u ? ulo : uend - 1u;
        uint32_t i = 0u, h = a.n - 1u;  // (any: some instance holds x, so n > 0)
        while (i < h) {
            const uint32_t mid = (i + h + 1u) >> 1;
            if (off[mid] <= x) i = mid;
            else h = mid - 1u;
        }
        s_ends[tid >> 6] = i;
    }
    __syncthreads();
    const uint32_t first = any ? s_ends[0] : 0u, last = any ? s_ends[1] : 0u;
    const uint32_t m = last - first + 2u;  // off[first .. last + 1]
    const bool staged = any && m <= COMPOSE_LDS_OFFSETS;
    if (staged)
        for (uint32_t k = tid; k < m; k += 256u) s_off[k] = off[first + k];
    __syncthreads();
    auto at = [&](uint32_t i) -> uint32_t { return staged ? s_off[i - first] : off[i]; };  // first <= i <= last + 1
    uint32_t cur = first;
    for (uint32_t k = 0u; k < a.steps; k++) {
        const uint32_t idx = k * 256u + tid;
        if (idx >= rem) break;
        const uint32_t l = lo + idx;
        uint32_t *d = a.dst + (size_t)a.dst_base[s] + l;
        const uint32_t x = s == 0u ? l * 4u : l;
        if (x >= uend) {  // the tags' padding
            *d = 0u;
            continue;
        }
        uint32_t i = cur, h = last;
        while (i < h) {
            const uint32_t mid = (i + h + 1u) >> 1;
            if (at(mid) <= x) i = mid;
            else h = mid - 1u;
        }
        cur = i;
        const uint32_t o = at(i);
        const uint32_t begin = a.frags[(size_t)frag_of[i] * 6u + s];
        if (s == 0u) {
            if (x + 4u <= at(i + 1u)) {
                const uint32_t sb = begin + (x - o);  // byte of the library's tag stream
                const uint32_t *p = a.lib + (size_t)a.src_base[0] + (sb >> 2);
                const uint32_t sh = (sb & 3u) * 8u;
                const uint32_t w0 = p[0], w1 = sh ? p[1] : 0u;
                *d = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);
            } else {
                const uint8_t *tags = reinterpret_cast<const uint8_t *>(a.lib + (size_t)a.src_base[0]);
                uint32_t v = 0u, j = i;
                for (uint32_t b = 0u; b < 4u; b++) {
                    const uint32_t pos = x + b;
                    if (pos >= uend) break;  // (the stream's end: uend == tag_bytes here)
                    while (pos >= at(j + 1u)) j++;  // (pos < uend: an instance <= last holds it)
                    v |= (uint32_t)tags[(size_t)a.frags[(size_t)frag_of[j] * 6u] + (pos - at(j))] << (8u * b);
                }
                *d = v;
            }
        } else if (s == 4u) {
            const uint32_t r = x - o, comp = r % 6u, pair = comp >> 1, odd = comp & 1u;
            const uint32_t *t = a.lib + (size_t)a.src_base[4] + begin + (r - comp) + 2u * pair;
            const uint32_t *v = frag_of + a.n + (size_t)i * 6u;
            float c = __uint_as_float(v[odd]) * __uint_as_float(t[0]) + __uint_as_float(v[2u + odd]) * __uint_as_float(t[1]);
            if (pair == 2u) c = c + __uint_as_float(v[4u + odd]);
            *d = __float_as_uint(c);
        } else if (PAINTED && s == 3u) {
            uint32_t v = a.lib[(size_t)a.src_base[3] + begin + (x - o)];
            const uint32_t *paint = pa.paints + (size_t)i * 2u;  // (i holds a word: i < n)
            if (paint[0] == PAINT_SOLID) {
                const uint32_t bit = pa.frag_bits[frag_of[i]] + (x - o);  // < the masks' bits: the host keeps their sum within u32
                if ((pa.masks[bit >> 5] >> (bit & 31u)) & 1u) v = paint[1];
            }
            *d = v;
        } else {
            *d = a.lib[(size_t)a.src_base[s] + begin + (x - o)];
        }
    }
}

__global__ void __launch_bounds__(256) k_compose_scene(ComposeArgs a) { compose_scene<false>(a, ComposePaintArgs{}); }

__global__ void __launch_bounds__(256) k_compose_scene_painted(ComposeArgs a, ComposePaintArgs pa) { compose_scene<true>(a, pa); }

void launch_compose_scene(const ComposeArgs &a, const ComposePaintArgs *pa, hipStream_t s) {
    if (pa) hipLaunchKernelGGL(k_compose_scene_painted, dim3(a.wg_first[6] + 1u), dim3(256), 0, s, a, *pa);
    else hipLaunchKernelGGL(k_compose_scene, dim3(a.wg_first[6] + 1u), dim3(256), 0, s, a);
}

}  // namespace vk
