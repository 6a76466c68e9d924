"""Per-frame path data (vello_hip_render_resident_morphed) against the CPU oracle.  The oracle has no such input: it is handed the
SUBSTITUTED scene -- the packed bytes with the path-data words [path_data_base, draw_tag_base) replaced by W = blend(A, B, t), computed
here in numpy f32 by the formula of include/vello_hip.h (numpy rounds every f32 operation on its own), not by the library under test --
while the engine is handed the raw scene and the morph.  tests.parity.compare_frame and tests.cull_parity.compare_culled_frame do the
comparing through MorphEngine, an adapter that swaps the scene on the engine's side only: every intermediate is held to the tolerances
the suite already uses.  Keyframes are synthesised from the scene's own words (a smooth function of position: equal points stay
equal, closed subpaths stay closed), so no second encode is needed."""
import ctypes

import numpy as np

from oracle.oracle import Oracle
from tests import cull_parity, parity
from tests import view_parity as vp
from tests.parity import canonical_nan_lines, sorted_rows

BLACK, WHITE = 0xFF000000, 0xFFFFFFFF
SCENE, DEVICE = 0xFFFFFFFF, 0xFFFFFFFE  # VELLO_HIP_PATH_DATA_SCENE / _DEVICE
E_INVALID = -1
f32 = np.float32


# ---------------------------------------------------------------------------------------------------------------
# The expectation
# ---------------------------------------------------------------------------------------------------------------
def path_words(packed, layout):
    """The scene's path-data words (a uint32 copy)."""
    return np.ascontiguousarray(packed, dtype=np.uint8).view(np.uint32)[layout.path_data_base: layout.draw_tag_base].copy()


def blend(a, b, t):
    """Rule 2 of the contract on uint32 words: A verbatim, B verbatim, or fl(A + fl(t * fl(B - A))) in f32."""
    a, b = np.ascontiguousarray(a, dtype=np.uint32), np.ascontiguousarray(b, dtype=np.uint32)
    t = f32(t)
    if t == f32(0.0):
        return a.copy()
    if t == f32(1.0):
        return b.copy()
    fa, fb = a.view(np.float32), b.view(np.float32)
    with np.errstate(all="ignore"):
        d = fb - fa
        p = t * d
        w = fa + p
    assert d.dtype == p.dtype == w.dtype == np.float32
    return w.view(np.uint32).copy()


def blend_fused(a, b, t):
    """What a contraction of the product and the sum into an FMA would give: t * d + A with ONE rounding (the product of two f32
    is exact in f64; the f64 sum's own rounding is far below an f32 ulp)."""
    fa, fb = np.asarray(a).view(np.float32), np.asarray(b).view(np.float32)
    d = fb - fa
    return (np.float64(f32(t)) * d.astype(np.float64) + fa.astype(np.float64)).astype(np.float32).view(np.uint32)


def substitute(packed, layout, words):
    """The packed scene with `words` in the place of its path-data stream; no other word changes."""
    out = np.ascontiguousarray(packed, dtype=np.uint8).copy()
    w = out.view(np.uint32)
    assert len(words) == layout.draw_tag_base - layout.path_data_base
    w[layout.path_data_base: layout.draw_tag_base] = np.asarray(words).view(np.uint32)
    return out


def keyframe(words, amp, freq, phase=0.0):
    """q = p + amp * sin(freq * p.yx + phase) on the (x, y) pairs of an f32 scene's path data: a smooth function of position."""
    p = np.asarray(words).view(np.float32).reshape(-1, 2).astype(np.float64)
    q = p + amp * np.sin(freq * p[:, ::-1] + phase)
    return q.astype(np.float32).reshape(-1).view(np.uint32).copy()


def expected_words(own, keys, device, src_a, src_b, t):
    def src(s):
        return own if s == SCENE else device if s == DEVICE else keys[s]

    return src(src_a).copy() if src_a == src_b else blend(src(src_a), src(src_b), t)


# ---------------------------------------------------------------------------------------------------------------
# Device memory for the two builds
# ---------------------------------------------------------------------------------------------------------------
class EmuMemory:
    """Device memory of the SIMT-emulated build: host memory.  `words(w, aligned)`: a float32 array holding `w` at an address that
    is a multiple of 16, or one that is a multiple of 4 only."""
    points_is_device = True

    def words(self, w, aligned=True):
        w = np.asarray(w).view(np.float32)
        buf = np.zeros(len(w) + 8, dtype=np.float32)
        off = (-(buf.ctypes.data // 4)) % 4 + (0 if aligned else 1)
        out = buf[off: off + len(w)]
        out[:] = w
        assert len(w) == 0 or out.ctypes.data % 16 == (0 if aligned else 4)
        return out

    def target(self, w, h):
        return np.zeros((h, w, 4), dtype=np.uint8)

    def numpy(self, t):
        return t


class GpuMemory:
    points_is_device = False

    def words(self, w, aligned=True):
        import torch

        w = np.ascontiguousarray(np.asarray(w).view(np.float32))
        buf = torch.zeros(len(w) + 8, dtype=torch.float32, device="cuda")
        off = (-(buf.data_ptr() // 4)) % 4 + (0 if aligned else 1)
        if len(w) == 0:  # (an empty slice has no address: the buffer's own, as an int)
            self._keep = buf
            return buf.data_ptr() + 4 * off
        out = buf[off: off + len(w)]
        out.copy_(torch.from_numpy(w))
        torch.cuda.synchronize()
        assert len(w) == 0 or out.data_ptr() % 16 == (0 if aligned else 4)
        return out

    def target(self, w, h):
        import torch

        return torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")

    def numpy(self, t):
        return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------
# The adapter
# ---------------------------------------------------------------------------------------------------------------
class MorphEngine:
    """What compare_frame / compare_culled_frame see as the engine: every blocking render they ask for -- with the SUBSTITUTED bytes,
    which go to the oracle -- is an upload of the RAW scene (and the keyframes) and one morphed resident frame into the engine's own
    target; everything else is the engine's own."""

    def __init__(self, engine, raw_packed, morph, keys=None, points=None, mem=None):
        self._engine, self._raw, self._morph, self._keys, self._points, self._mem = engine, raw_packed, morph, keys, points, mem
        self.frames = 0

    def __getattr__(self, name):
        return getattr(self._engine, name)

    def render(self, packed, layout, width, height, base_color, aa, ramps=None):
        e = self._engine
        e.upload_scene(self._raw, layout, ramps)
        if self._keys is not None:
            e.upload_path_keyframes(np.stack(self._keys))
        self.frames += 1
        e.render_resident(width, height, base_color, aa, morph=self._morph, points=self._points,
                          points_is_device=self._mem.points_is_device if self._mem is not None else False)
        r = e.sync()
        assert r in (0, -4), f"sync: {r}: {e._lib.vello_hip_last_error(e._h).decode()}"
        bump = e.bump()
        img = e.read_buffer("output", np.uint8, width * height * 4).reshape(height, width, 4).copy()
        return img, bump


def compare_morph_frame(engine, packed, layout, morph, width, height, base_color, aa, name, keys=None, device=None, mem=None, aligned=True,
                        culled=False, differs=True, view=None, raw_ref=None, **kw):
    """compare_frame (or compare_culled_frame) of the raw scene under `morph` = (src_a, src_b, t) against the oracle on the substituted
    scene; asserts first that the substituted scene's image is not the raw scene's, so that an engine that ignores the morph fails.
    `keys`: the keyframes (uint32 word arrays); `device`: the words of the device source, placed by `mem` at an aligned or a
    misaligned address; `view`: a view transform set on the engine, composed into the oracle's scene."""
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    own = path_words(packed, layout)
    want = expected_words(own, keys, device, *morph)
    sub = substitute(packed, layout, want)
    points = mem.words(device, aligned) if (device is not None and DEVICE in morph[:2]) else None
    me = MorphEngine(engine, packed, morph, keys, points, mem)
    eng, scene = me, sub
    if view is not None:
        eng, scene = vp.ViewEngine(me, packed, view), vp.compose(sub, layout, view)
    if differs:
        raw = raw_ref if raw_ref is not None else vp.raw_image(packed if view is None else vp.compose(packed, layout, view), layout, width, height, base_color, aa, kw.get("resolved"))
        ref = vp.raw_image(scene, layout, width, height, base_color, aa, kw.get("resolved"))
        assert not np.array_equal(raw, ref), f"{name}: the morph changes nothing in this scene: the case proves nothing"
    elif differs is None:  # (a scene without area: its soup tells)
        assert not np.array_equal(_oracle_soup(packed, layout, width, height, base_color, aa), _oracle_soup(scene, layout, width, height, base_color, aa)), name
    if culled:
        out = cull_parity.compare_culled_frame(eng, scene, layout, width, height, base_color, aa, name, **kw)
    else:
        out = parity.compare_frame(eng, scene, layout, width, height, base_color, aa, name, **kw)
    assert me.frames > 0
    return out[0], out[1], out[2]


def _oracle_soup(packed, layout, w, h, base, aa):
    o = Oracle()
    o.set_scene(packed, layout, w, h, base, int(aa))
    o.render()
    return sorted_rows(canonical_nan_lines(o.buffer("lines", np.uint32)[: o.bump()["lines"] * 6]), 6)


# ---------------------------------------------------------------------------------------------------------------
# Scenes
# ---------------------------------------------------------------------------------------------------------------
def polygon_words_scene(n_words, size=64.0, seed=5):
    """Closed straight polygons under the identity transform whose path data is exactly n_words words (a polygon of m vertices is
    m + 1 points: the closing line's end is encoded): every path-data word is a coordinate of the line soup."""
    from vello_amd import Affine, BezPath, Color, Fill, Scene

    assert n_words % 2 == 0 and n_words >= 6
    units = n_words // 2  # points: triangles (4) and quadrilaterals (5), and where those cannot add up two-vertex polygons (3)
    c, b = next((c, b) for c in range(0, 3) for b in range(0, 5) if (units - 3 * c - 5 * b) >= 0 and (units - 3 * c - 5 * b) % 4 == 0)
    ms = [2] * c + [4] * b + [3] * ((units - 3 * c - 5 * b) // 4)
    rng = np.random.default_rng(seed)
    s = Scene()
    for k, m in enumerate(ms):
        cx, cy = rng.uniform(4.0, size - 4.0, 2)
        r = rng.uniform(3.0, size / 5)
        a = np.sort(rng.uniform(0, 2 * np.pi, m)) if m > 2 else np.array([0.3, 2.9])
        p = BezPath()
        p.move_to((float(cx + r * np.cos(a[0])), float(cy + r * np.sin(a[0]))))
        for t in a[1:]:
            p.line_to((float(cx + r * np.cos(t)), float(cy + r * np.sin(t))))
        p.close_path()
        s.fill(Fill.NonZero, Affine.IDENTITY, Color((k % 5) / 4.0, (k % 3) / 2.0, (k % 7) / 6.0, 1.0), None, p)
    packed, layout = s.resolve()
    assert layout.draw_tag_base - layout.path_data_base == n_words, (n_words, layout)
    return np.ascontiguousarray(packed, dtype=np.uint8), layout


def hand_scene(n_words):
    """A scene without paths (n_words == 0), or one whose path-data stream holds n_words words that no segment reads: an empty tag
    stream of one padded block, then the words.  Nothing of such a morph is visible; the frame must still be the empty scene's."""
    from vello_amd import Layout

    packed = np.zeros((1024 + n_words) * 4, dtype=np.uint8)
    packed.view(np.uint32)[1024:] = np.arange(n_words, dtype=np.uint32) + 0x3F800000
    b = 1024 + n_words
    return packed, Layout(0, 0, 0, 0, 0, 1024, b, b, b, b)


def small_triangles_scene(n, size=256.0, seed=9):
    """n small filled triangles: a tag stream above the small-scene launches' limit, a soup of 3 n lines."""
    from vello_amd import Affine, BezPath, Color, Fill, Scene

    rng = np.random.default_rng(seed)
    s = Scene()
    for k in range(n):
        cx, cy = rng.uniform(0.0, size, 2)
        r = rng.uniform(1.5, 5.0)
        a = np.sort(rng.uniform(0, 2 * np.pi, 3))
        p = BezPath()
        p.move_to((float(cx + r * np.cos(a[0])), float(cy + r * np.sin(a[0]))))
        p.line_to((float(cx + r * np.cos(a[1])), float(cy + r * np.sin(a[1]))))
        p.line_to((float(cx + r * np.cos(a[2])), float(cy + r * np.sin(a[2]))))
        p.close_path()
        s.fill(Fill.NonZero, Affine.IDENTITY, Color((k % 5) / 4.0, (k % 3) / 2.0, (k % 7) / 6.0, 0.8), None, p)
    packed, layout = s.resolve()
    return np.ascontiguousarray(packed, dtype=np.uint8), layout


def two_keys(packed, layout, amp=5.0):
    own = path_words(packed, layout)
    return [keyframe(own, amp, 0.11, 0.4), keyframe(own, -0.8 * amp, 0.07, 1.3)]


def _tol(aa):
    return 1 if int(aa) == 0 else 0


# ---------------------------------------------------------------------------------------------------------------
# 1. Sizes and alignment of the kernel
# ---------------------------------------------------------------------------------------------------------------
def vec_words(engine):
    """PATH_BLEND_VEC_WORDS (engine.h): words a workgroup of k_path_blend takes per grid step in its 16-byte form."""
    return engine.stage_constants()["path_blend_vec_words"]


SIZES = (0, 2, 6, 254, 256, 258, 1022, 1026, 2 * 1024 + 6)


def check_size(engine, mem, name, n_words):
    """The three modes at one stream length, from keyframes, the scene's own stream and a device source at a 16-byte-aligned address
    and at one that is only 4-byte aligned: the soup as a multiset and the image equal the oracle's on the substituted scene.  Every
    case first asserts that the oracle tells the substituted scene from the raw one -- by the image; by the soup at 6 words, which are
    one polygon of two vertices (no area); not at 0 and 2 words, where no segment reads the stream: there the frame must simply be the
    empty scene's, whatever the launch does."""
    from vello_amd import AaConfig

    assert SIZES[-1] > 2 * vec_words(engine)
    visible = n_words >= 6
    packed, layout = polygon_words_scene(n_words) if visible else hand_scene(n_words)
    own = path_words(packed, layout)
    if visible:
        keys = two_keys(packed, layout, 4.0)
        device = keyframe(own, 6.0, 0.05, 2.0)
    else:
        keys = [own + np.uint32(1), own + np.uint32(2)]
        device = own + np.uint32(3)
    w = h = 64
    raw = vp.raw_image(packed, layout, w, h, BLACK, AaConfig.Msaa16)
    cases = [("copy_a_dev16", (DEVICE, 1, 0.0), True), ("copy_b_dev4", (0, DEVICE, 1.0), False), ("mix_dev16_key0", (DEVICE, 0, 0.5), True),
             ("mix_key0_dev4", (0, DEVICE, 0.3), False), ("mix_scene_key1", (SCENE, 1, 0.5), True), ("copy_same_key1", (1, 1, 0.3), True),
             ("points_dev4", (DEVICE, DEVICE, 0.7), False)]
    for cname, morph, aligned in cases:
        compare_morph_frame(engine, packed, layout, morph, w, h, BLACK, AaConfig.Msaa16, f"{name}_{n_words}_{cname}", keys=keys, device=device, mem=mem,
                            aligned=aligned, differs=(True if n_words > 6 else None) if visible else False, raw_ref=raw, back_half=False)


def check_odd_sizes(engine, mem, name):
    """Stream lengths the f32 polygon scenes cannot have -- 2 words that ONE segment reads, and 3, 5, 7: one and three words behind the
    last whole quad of the 16-byte form, and no whole quad at all -- from scenes of i16 segments, whose frames are verbatim copies
    (a blend of such a scene is refused: check_refusals).  Every word is a point of the soup; the oracle tells the substituted scene
    from the raw one by its soup (a two-vertex polygon has no area)."""
    from vello_amd import AaConfig

    w = h = 64
    for n_words in (2, 3, 5, 7):
        packed, layout = i16_scene(6, single=True) if n_words == 2 else i16_scene(2 * n_words)
        own = path_words(packed, layout)
        assert len(own) == n_words
        keys = [own + np.uint32(3), own + np.uint32(5 << 16)]  # (x + 3; y + 5)
        device = own + np.uint32((2 << 16) + 4)
        for cname, morph, aligned in (("copy_a_dev16", (DEVICE, 1, 0.0), True), ("copy_b_dev4", (0, DEVICE, 1.0), False), ("copy_b_key1", (SCENE, 1, 1.0), True),
                                      ("same_key0", (0, 0, 0.5), True), ("points_dev16", (DEVICE, DEVICE, 0.25), True)):
            compare_morph_frame(engine, packed, layout, morph, w, h, BLACK, AaConfig.Msaa16, f"{name}_{n_words}_{cname}", keys=keys, device=device, mem=mem,
                                aligned=aligned, differs=None, back_half=False)


def check_unaligned_scene_stream(engine, mem, name):
    """The scene's own stream as a source when it does NOT begin on a 16-byte boundary (path_data_base % 4 == 1): the dword form;
    the packed scenes of the encoder always begin on one, which is what every other case has."""
    from vello_amd import AaConfig

    packed, layout = shifted_scene(*polygon_words_scene(258, seed=6))
    keys = two_keys(packed, layout, 4.0)
    w = h = 64
    for cname, morph in (("mix", (SCENE, 1, 0.5)), ("copy", (SCENE, SCENE, 0.5)), ("mix_b", (0, SCENE, 0.3))):
        compare_morph_frame(engine, packed, layout, morph, w, h, BLACK, AaConfig.Msaa16, f"{name}_{cname}", keys=keys, differs=cname != "copy", back_half=False)


# ---------------------------------------------------------------------------------------------------------------
# 2. Blend arithmetic
# ---------------------------------------------------------------------------------------------------------------
def check_arithmetic(engine, mem, name):
    from vello_amd import AaConfig

    packed, layout = polygon_words_scene(258, seed=6)
    keys = two_keys(packed, layout, 4.0)
    w = h = 64
    raw = vp.raw_image(packed, layout, w, h, BLACK, AaConfig.Msaa16)
    for t in (0.0, -0.0, 1.0, 0.5, 0.3, 1.5, -0.25):
        compare_morph_frame(engine, packed, layout, (0, 1, t), w, h, BLACK, AaConfig.Msaa16, f"{name}_t{t}", keys=keys, raw_ref=raw, back_half=False)
    compare_morph_frame(engine, packed, layout, (1, 1, 0.3), w, h, BLACK, AaConfig.Msaa16, f"{name}_same", keys=keys, raw_ref=raw, back_half=False)
    # words for which a fused t * d + A differs from the three roundings: the soup's coordinates ARE the words (identity transform)
    unfused, fused = blend(keys[0], keys[1], 0.3), blend_fused(keys[0], keys[1], 0.3)
    assert (unfused != fused).sum() >= 4, f"{name}: these words cannot tell an FMA from the contract's formula"
    compare_morph_frame(engine, packed, layout, (0, 1, 0.3), w, h, BLACK, AaConfig.Msaa16, f"{name}_unfused", keys=keys, raw_ref=raw, back_half=False)


def check_verbatim_bits(engine, mem, name):
    """A verbatim frame whose source holds a NaN point (with a payload) and a -0.0: the frame of the scene uploaded with those bytes."""
    from vello_amd import AaConfig

    packed, layout = polygon_words_scene(258, seed=7)
    src = keyframe(path_words(packed, layout), 3.0, 0.09)
    src[10] = 0x7FC12345
    src[11] = 0xFFC00001
    src[40] = 0x80000000
    w = h = 64
    sub = substitute(packed, layout, src)
    assert not np.array_equal(_oracle_soup(packed, layout, w, h, BLACK, AaConfig.Msaa16), _oracle_soup(sub, layout, w, h, BLACK, AaConfig.Msaa16)), \
        f"{name}: the source changes nothing in this scene: the case proves nothing"
    img0, b0 = engine.render(sub, layout, w, h, BLACK, AaConfig.Msaa16)
    raw_img, _ = engine.render(packed, layout, w, h, BLACK, AaConfig.Msaa16)
    assert not np.array_equal(img0, raw_img), f"{name}: the source's image is the raw scene's"
    img0, b0 = engine.render(sub, layout, w, h, BLACK, AaConfig.Msaa16)
    soup0 = sorted_rows(engine.read_buffer("lines", np.uint32, b0["lines"] * 24), 6)
    boxes0 = engine.read_buffer("path_bboxes", np.int32, layout.n_paths * 24)
    for cname, morph, keys, device in (("device", (DEVICE, DEVICE, 0.0), None, src), ("key_t1", (SCENE, 0, 1.0), [src], None)):
        me = MorphEngine(engine, packed, morph, keys, mem.words(device, False) if device is not None else None, mem)
        img1, b1 = me.render(None, layout, w, h, BLACK, AaConfig.Msaa16)
        assert b0 == b1, f"{name}_{cname}: {b0} {b1}"
        soup1 = sorted_rows(engine.read_buffer("lines", np.uint32, b1["lines"] * 24), 6)
        assert np.array_equal(soup0, soup1), f"{name}_{cname}: the soup is not the soup of the scene uploaded with these bytes"
        assert np.array_equal(boxes0, engine.read_buffer("path_bboxes", np.int32, layout.n_paths * 24)), f"{name}_{cname}: path boxes"
        assert np.array_equal(img0, img1), f"{name}_{cname}: image"


# ---------------------------------------------------------------------------------------------------------------
# 3. Every path a frame can take
# ---------------------------------------------------------------------------------------------------------------
def check_front_fusion(engine, mem, name):
    import workloads
    from vello_amd import AaConfig

    for cname, scene, w, h in (("circle", workloads.circle_scene(), 256, 256), ("stroke_styles", workloads.stroke_styles_scene(), 256, 256)):
        packed, layout = scene.resolve()
        keys = two_keys(packed, layout, 9.0)
        try:
            engine.set_debug_flags(flatten_coop=True)
            before = engine.fused_launches()
            compare_morph_frame(engine, packed, layout, (0, 1, 0.4), w, h, WHITE, AaConfig.Msaa16, f"{name}_{cname}_fused", keys=keys)
            assert engine.fused_launches() > before, f"{name}_{cname}: the fused path was not taken"
            compare_morph_frame(engine, packed, layout, (SCENE, 1, 0.6), w, h, WHITE, AaConfig.Area, f"{name}_{cname}_fused_area", keys=keys, tol=1)
            engine.set_debug_flags(flatten_coop=True, no_fusion=True)
            before = engine.fused_launches()
            compare_morph_frame(engine, packed, layout, (0, 1, 0.4), w, h, WHITE, AaConfig.Msaa16, f"{name}_{cname}_nofusion", keys=keys)
            assert engine.fused_launches() == before
        finally:
            engine.set_debug_flags()


def check_indexed(engine, mem, name):
    """A scene above front_max_tags: with the index its upload builds and with no_scene_index; morphed frames build no index."""
    from vello_amd import AaConfig

    packed, layout = small_triangles_scene(4400)
    assert (layout.path_data_base - layout.path_tag_base) * 4 > engine.stage_constants()["front_max_tags"]
    keys = two_keys(packed, layout, 3.0)
    device = keyframe(path_words(packed, layout), 4.0, 0.05, 2.0)
    w = h = 256
    for in_flight in (1, 2):  # (with frames in flight an indexed frame's flatten is the merged front, k_flatten_front)
        try:
            engine.set_frames_in_flight(in_flight)
            for flag in ((False, True) if in_flight == 1 else (False,)):
                engine.set_debug_flags(no_scene_index=flag)
                builds = engine.scene_index_builds()
                compare_morph_frame(engine, packed, layout, (0, DEVICE, 0.35), w, h, BLACK, AaConfig.Msaa16, f"{name}_index_{int(not flag)}_{in_flight}", keys=keys,
                                    device=device, mem=mem, back_half=in_flight == 1)
                # (compare_frame renders once, its back half once more: an upload each, a morphed frame each)
                uploads = 2 if in_flight == 1 else 1
                assert engine.scene_index_builds() == builds + uploads, f"{name}: morphed frames built {engine.scene_index_builds() - builds - uploads} scene indexes"
                for t in (0.1, 0.9):
                    engine.render_resident(w, h, BLACK, AaConfig.Msaa16, morph=(0, 1, t))
                assert engine.sync() == 0 and engine.scene_index_builds() == builds + uploads
        finally:
            engine.set_debug_flags()
            engine.set_frames_in_flight(1)


def check_strokes(engine, mem, name, stroke_kernel):
    from vello_amd import AaConfig

    packed, layout = cull_parity.polyline_scene(n=120, size=256.0).resolve()
    keys = two_keys(packed, layout, 7.0)
    try:
        engine.set_debug_flags(stroke_kernel=stroke_kernel)
        compare_morph_frame(engine, packed, layout, (0, 1, 0.45), 200, 152, WHITE, AaConfig.Msaa16, f"{name}_polylines_{int(stroke_kernel)}", keys=keys)
    finally:
        engine.set_debug_flags()


def check_curves(engine, mem, name, which_kernels, case):
    import workloads
    from vello_amd import AaConfig

    mk = [workloads.cardioid_scene, workloads.funky_paths_scene, workloads.tricky_strokes_scene][case]
    r = mk()
    s, w, h = r if isinstance(r, tuple) else (r, 512, 512)
    w, h = min(w, 320), min(h, 320)
    packed, layout = s.resolve()
    # (the cardioid is 2048 x 1536: seen whole through a view that scales it down)
    view, amp = ((0.15, 0.0, 0.0, 0.15, 0.0, 0.0), 60.0) if case == 0 else (None, 11.0)
    keys = two_keys(packed, layout, amp)
    try:
        engine.set_debug_flags(**{which_kernels: True})
        if case == 1:
            engine.set_frames_in_flight(2)
        aa = AaConfig.Area if case == 2 else AaConfig.Msaa16
        compare_morph_frame(engine, packed, layout, (0, 1, 0.55), w, h, BLACK, aa, f"{name}_{mk.__name__}_{which_kernels}", keys=keys, tol=_tol(aa), view=view)
    finally:
        engine.set_frames_in_flight(1)
        engine.set_debug_flags()


def check_tiger(engine, mem, name, size=512):
    from vello_amd import AaConfig

    packed, layout = cull_parity.tiger()
    keys = two_keys(packed, layout, 14.0)
    compare_morph_frame(engine, packed, layout, (SCENE, 1, 0.5), size, size, WHITE, AaConfig.Msaa8, name, keys=keys)


# ---------------------------------------------------------------------------------------------------------------
# 4. Composition with the other per-frame options
# ---------------------------------------------------------------------------------------------------------------
def check_view(engine, mem, name):
    import workloads
    from vello_amd import AaConfig

    packed, layout = workloads.random_test_scene(3, n_paths=150, size=256.0, strokes=True, clips=True).resolve()
    keys = two_keys(packed, layout, 8.0)
    for vname in ("rot_shear", "zoom_in"):
        compare_morph_frame(engine, packed, layout, (0, 1, 0.5), 200, 160, BLACK, AaConfig.Msaa16, f"{name}_{vname}", keys=keys, view=dict(vp.views(200, 160))[vname])


def check_culled(engine, mem, name):
    """With vello_hip_set_viewport_cull: the rule is applied to the lines of the MORPHED scene, and lines are really dropped."""
    from vello_amd import AaConfig

    packed, layout = cull_parity.polyline_scene().resolve()
    keys = two_keys(packed, layout, 25.0)
    compare_morph_frame(engine, packed, layout, (0, 1, 0.5), 175, 131, WHITE, AaConfig.Msaa16, f"{name}_polylines", keys=keys, culled=True, require_culling=True)


# ---------------------------------------------------------------------------------------------------------------
# 5. Frames in flight, 8. run_stages, 7. queries
# ---------------------------------------------------------------------------------------------------------------
def _oracle_image(packed, layout, w, h, base, aa):
    o = Oracle()
    o.set_scene(packed, layout, w, h, base, int(aa))
    return o.render().copy()


def check_in_flight(engine, mem, name):
    """Four frames in flight on ONE resident scene, four values of t (and a device source) in four targets, then a plain resident
    frame on a lane that just ran a morphed one; no scene buffer is allocated after the first morphed frame."""
    import workloads
    from vello_amd import AaConfig

    w, h = 128, 96
    packed, layout = workloads.random_test_scene(5, n_paths=80, size=128.0, strokes=True, clips=True).resolve()
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    own = path_words(packed, layout)
    keys = two_keys(packed, layout, 8.0)
    device = keyframe(own, 10.0, 0.04, 0.7)
    points = mem.words(device, False)
    morphs = [(0, 1, 0.25), (SCENE, 0, 0.75), (DEVICE, 1, 0.5), (DEVICE, DEVICE, 0.0)]
    want = [_oracle_image(substitute(packed, layout, expected_words(own, keys, device, *m)), layout, w, h, BLACK, AaConfig.Msaa16) for m in morphs]
    plain = _oracle_image(packed, layout, w, h, BLACK, AaConfig.Msaa16)
    assert all(not np.array_equal(x, plain) for x in want) and not np.array_equal(want[0], want[1])
    kw = {"points_is_device": mem.points_is_device}
    try:
        engine.set_frames_in_flight(4)
        engine.upload_scene(packed, layout)
        t0 = mem.target(w, h)
        engine.render_resident(w, h, BLACK, AaConfig.Msaa16, out=t0)
        assert engine.sync() == 0
        plain_before = mem.numpy(t0).copy()
        assert np.array_equal(plain_before, plain)
        engine.upload_path_keyframes(np.stack(keys))
        allocations = None
        for rnd in range(5):
            targets = [mem.target(w, h) for _ in range(4)]
            for k in range(4):
                m = morphs[(k + rnd) % 4]
                engine.render_resident(w, h, BLACK, AaConfig.Msaa16, out=targets[k], morph=m, points=points if DEVICE in m[:2] else None, **kw)
                if allocations is None:
                    allocations = engine.scene_allocations()  # (after the first morphed frame)
            assert engine.sync() == 0
            for k in range(4):
                assert np.array_equal(mem.numpy(targets[k]), want[(k + rnd) % 4]), f"{name}: round {rnd}, frame {k} does not show its own morph"
        assert engine.scene_allocations() == allocations, f"{name}: {engine.scene_allocations() - allocations} scene buffers allocated in the steady state"
        # every lane has just run a morphed frame: a plain frame on each shows the scene's own points, byte for byte
        targets = [mem.target(w, h) for _ in range(4)]
        for k in range(4):
            engine.render_resident(w, h, BLACK, AaConfig.Msaa16, out=targets[k])
        assert engine.sync() == 0
        for k in range(4):
            assert np.array_equal(mem.numpy(targets[k]), plain_before), f"{name}: the plain frame on lane {k} after a morphed one"
        assert np.array_equal(engine.read_buffer("scene", np.uint8, packed.nbytes), packed), f"{name}: the resident scene was modified"
        cfg = engine.read_buffer("config", np.uint32, 88)
        assert int(cfg[5 + 5]) == layout.path_data_base, f"{name}: VELLO_HIP_BUF_CONFIG does not hold the scene's own layout"
    finally:
        engine.set_frames_in_flight(1)


def check_run_stages_and_queries(engine, mem, name):
    """run_stages(FLATTEN .. FINE) after a morphed frame reproduces the morphed image from the lane's words; pick answers against the
    morphed geometry; read_buffer("scene") returns the uploaded bytes."""
    from vello_amd import AaConfig, Affine, Color, Fill, Rect, Scene

    s = Scene()
    s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(255, 0, 0), None, Rect(10.0, 10.0, 40.0, 40.0))
    s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(0, 255, 0), None, Rect(60.0, 60.0, 90.0, 90.0))
    packed, layout = s.resolve()
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    own = path_words(packed, layout)
    moved = (own.view(np.float32) + f32(100.0)).view(np.uint32)  # both squares 100 px down and right
    w = h = 200
    aa = AaConfig.Msaa16
    want = _oracle_image(substitute(packed, layout, blend(own, moved, 0.5)), layout, w, h, BLACK, aa)
    engine.upload_scene(packed, layout)
    engine.upload_path_keyframes(moved.reshape(1, -1))
    pts = np.array([[75.0, 75.0], [25.0, 25.0], [125.0, 125.0]], dtype=np.float32)
    engine.render_resident(w, h, BLACK, aa)
    assert engine.sync() == 0
    assert [int(v) for v in engine.pick(pts)[:, 0]] == [1, 0, 0xFFFFFFFF]
    engine.render_resident(w, h, BLACK, aa, morph=(SCENE, 0, 0.5))  # squares at 60..90 and 110..140
    assert engine.sync() == 0
    img = engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4).copy()
    assert np.array_equal(img, want), f"{name}: morphed image"
    assert [int(v) for v in engine.pick(pts)[:, 0]] == [0, 0xFFFFFFFF, 1], f"{name}: pick does not answer against the morphed geometry"
    engine.write_buffer("output", np.zeros(w * h * 4, dtype=np.uint8))
    engine.run_stages(w, h, BLACK, aa, "flatten", "fine")
    assert np.array_equal(engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4), want), f"{name}: run_stages after a morphed frame"
    assert np.array_equal(engine.read_buffer("scene", np.uint8, packed.nbytes), packed), f"{name}: the resident scene was modified"
    engine.render_resident(w, h, BLACK, aa)
    assert engine.sync() == 0
    assert np.array_equal(engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4), _oracle_image(packed, layout, w, h, BLACK, aa))


# ---------------------------------------------------------------------------------------------------------------
# 6. Device source ordering (GPU only)
# ---------------------------------------------------------------------------------------------------------------
def check_ordering(engine, name):
    """A torch op writes the points on a side stream behind work that keeps that stream busy; the frame is enqueued with that stream
    as src_stream; the same stream then overwrites the tensor.  The frame shows the first contents: it ran behind the write, and the
    overwrite ran behind the kernel that read the points.  Nothing waits on the host in between."""
    import torch
    from vello_amd import AaConfig

    packed, layout = small_triangles_scene(600, size=128.0)
    own = path_words(packed, layout)
    first, second = keyframe(own, 5.0, 0.11, 0.4), keyframe(own, -6.0, 0.07, 1.3)
    w = h = 128
    want = _oracle_image(substitute(packed, layout, first), layout, w, h, BLACK, AaConfig.Msaa16)
    assert not np.array_equal(want, _oracle_image(substitute(packed, layout, second), layout, w, h, BLACK, AaConfig.Msaa16))
    a = torch.from_numpy(first.view(np.float32)).cuda()
    b = torch.from_numpy(second.view(np.float32)).cuda()
    points = torch.zeros(len(own), dtype=torch.float32, device="cuda")
    busy = torch.ones(1 << 24, dtype=torch.float32, device="cuda")
    target = torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    engine.upload_scene(packed, layout)
    side = torch.cuda.Stream()
    for rnd in range(3):
        with torch.cuda.stream(side):
            for _ in range(8):
                busy.mul_(1.0000001)
            points.copy_(a)
        engine.render_resident(w, h, BLACK, AaConfig.Msaa16, out=target, points=points, src_stream=side)
        with torch.cuda.stream(side):
            points.copy_(b)
        assert engine.sync() == 0
        side.synchronize()
        assert np.array_equal(target.cpu().numpy(), want), f"{name}: round {rnd}: the frame does not show the first contents of the tensor"
        assert np.array_equal(points.cpu().numpy().view(np.uint32), second)
        points.zero_()
        torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# 9. Refusals
# ---------------------------------------------------------------------------------------------------------------
def shifted_scene(packed, layout):
    """The same scene one word further into its buffer (a zero word in front, every base one higher): its path-data stream no longer
    begins on a 16-byte boundary of the device buffer."""
    from vello_amd import Layout

    out = np.concatenate([np.zeros(1, dtype=np.uint32), np.ascontiguousarray(packed, dtype=np.uint8).view(np.uint32)])
    lay = Layout(*layout[:4], *[v + 1 for v in layout[4:]])
    assert lay.path_data_base % 4 == 1
    return np.ascontiguousarray(out).view(np.uint8), lay


def i16_scene(n_f32_words=40, single=False):
    """A polygon scene whose tag stream is rewritten by hand to i16 segment tags: its path data is re-packed as pairs of i16 (the
    layout's streams move up accordingly), n_f32_words / 2 words -- any length, odd ones included.  `single` (of the 6-word scene:
    one polygon of two vertices): the first of its two segment tags becomes a no-op and the stream its first two words -- ONE line,
    whose two words are all the path data there is.  Returns (packed, layout)."""
    from vello_amd import Layout

    packed, layout = polygon_words_scene(n_f32_words, seed=3)
    w = packed.view(np.uint32)
    tags = packed[layout.path_tag_base * 4: layout.path_data_base * 4].copy()
    seg = (tags & 3) != 0
    assert seg.any() and ((tags[seg] & 8) != 0).all()
    tags[seg] &= np.uint8(0xFF ^ 8)
    pts = np.rint(path_words(packed, layout).view(np.float32).reshape(-1, 2)).astype(np.int64)
    data = ((pts[:, 0] & 0xFFFF) | ((pts[:, 1] & 0xFFFF) << 16)).astype(np.uint32)
    if single:
        ix = np.flatnonzero(seg)
        assert n_f32_words == 6 and len(ix) == 2 and (tags[ix[1]] & 4) != 0
        tags[ix[0]] = 0
        data = data[:2]
    rest = w[layout.draw_tag_base:]
    out = np.concatenate([tags.view(np.uint32), data, rest])
    shift = len(data) - (layout.draw_tag_base - layout.path_data_base)
    lay = Layout(layout.n_draw_objects, layout.n_paths, layout.n_clips, layout.bin_data_start, layout.path_tag_base, layout.path_data_base,
                 layout.draw_tag_base + shift, layout.draw_data_base + shift, layout.transform_base + shift, layout.style_base + shift)
    return np.ascontiguousarray(out).view(np.uint8), lay


def check_refusals(engine, mem, name):
    """Every refusal of rule 7: VELLO_HIP_E_INVALID, nothing enqueued, the rotation where it was -- the next frame lands on the lane it
    would have."""
    from vello_amd import AaConfig
    from vello_amd._lib import RenderParamsStruct

    lib, h = engine._lib, engine._h
    aa = AaConfig.Msaa16
    W = H = 64
    packed, layout = polygon_words_scene(258, seed=8)
    own = path_words(packed, layout)
    keys = two_keys(packed, layout, 4.0)
    n = len(own)
    p = RenderParamsStruct(W, H, BLACK, int(aa))
    fl = ctypes.c_float

    def call(a, b, t, dev=None, stream=None, params=p, out=None, stride=0, ctx=h):
        return lib.vello_hip_render_resident_morphed(ctx, a, b, fl(t), dev, stream, ctypes.byref(params) if params is not None else None, out, stride)

    def err():
        return lib.vello_hip_last_error(h).decode()

    # no resident scene (a fresh engine has none); a null context
    assert call(SCENE, SCENE, 0.0) == E_INVALID and "no scene" in err()
    assert lib.vello_hip_upload_path_keyframes(h, keys[0].ctypes.data, 1, n) == E_INVALID
    assert engine.path_data_words() == 0
    assert call(SCENE, SCENE, 0.0, ctx=None) == E_INVALID
    assert lib.vello_hip_upload_path_keyframes(None, None, 0, 0) == E_INVALID and lib.vello_hip_path_data_words(None) == 0

    points = mem.words(keys[1], True)
    addr = points.ctypes.data if isinstance(points, np.ndarray) else points.data_ptr()
    targets = [mem.target(W, H) for _ in range(3)]
    tptr = [vp._target_ptr(t) for t in targets]
    engine.set_frames_in_flight(2)
    try:
        engine.upload_scene(packed, layout)
        assert engine.path_data_words() == n
        # keyframes: a wrong length, a null pointer: nothing changes (still no keyframes: index 0 is refused)
        assert lib.vello_hip_upload_path_keyframes(h, keys[0].ctypes.data, 1, n + 1) == E_INVALID
        assert lib.vello_hip_upload_path_keyframes(h, None, 1, n) == E_INVALID
        assert call(0, SCENE, 0.0) == E_INVALID and "keyframes" in err()
        engine.upload_path_keyframes(np.stack(keys))
        want_a = _oracle_image(substitute(packed, layout, keys[0]), layout, W, H, BLACK, aa)
        want_b = _oracle_image(substitute(packed, layout, keys[1]), layout, W, H, BLACK, aa)
        # The two lanes' internal targets get an image each: lane 0 key 0's, lane 1 key 1's.  A frame into an external target leaves
        # its lane's internal one alone, and read_buffer("output") shows the newest frame's lane's: it tells which lane a frame took.
        engine.render_resident(W, H, BLACK, aa, morph=(0, 0, 0.0))
        engine.render_resident(W, H, BLACK, aa, morph=(1, 1, 0.0))
        assert engine.sync() == 0

        def lane_image():
            return engine.read_buffer("output", np.uint8, W * H * 4).reshape(H, W, 4)

        assert np.array_equal(lane_image(), want_b) and not np.array_equal(want_a, want_b)
        before = mem.numpy(targets[1]).copy()
        nan, inf = float("nan"), float("inf")
        bad_aa = RenderParamsStruct(W, H, BLACK, 7)
        zero_w = RenderParamsStruct(0, H, BLACK, int(aa))
        refusals = [
            ("a source index >= n_keys", lambda: call(2, 0, 0.5, out=tptr[1])),
            ("a source index >= n_keys (b)", lambda: call(0, 0xFFFFFFFD, 0.5, out=tptr[1])),
            ("DEVICE with null device_words", lambda: call(DEVICE, 0, 0.5, out=tptr[1])),
            ("DEVICE with misaligned device_words", lambda: call(DEVICE, 0, 0.5, dev=addr + 2, out=tptr[1])),
            ("device_words without a DEVICE source", lambda: call(0, 1, 0.5, dev=addr, out=tptr[1])),
            ("src_stream without a DEVICE source", lambda: call(0, 1, 0.5, stream=ctypes.c_void_p(engine.stream() or 1), out=tptr[1])),
            ("t NaN", lambda: call(0, 1, nan, out=tptr[1])),
            ("t +inf", lambda: call(0, 1, inf, out=tptr[1])),
            ("t -inf", lambda: call(0, 0, -inf, out=tptr[1])),
            ("AA mode", lambda: call(0, 1, 0.5, params=bad_aa, out=tptr[1])),
            ("zero width", lambda: call(0, 1, 0.5, params=zero_w, out=tptr[1])),
            ("null params", lambda: call(0, 1, 0.5, params=None, out=tptr[1])),
            ("misaligned target", lambda: call(0, 1, 0.5, out=tptr[1] + 2)),
            ("stride below a row", lambda: call(0, 1, 0.5, out=tptr[1], stride=W * 4 - 4)),
            ("stride no multiple of 4", lambda: call(0, 1, 0.5, out=tptr[1], stride=W * 4 + 2)),
        ]
        if not mem.points_is_device:  # (GPU builds: host memory is not device memory)
            host = np.zeros(n + 4, dtype=np.float32)
            refusals.append(("non-device device_words", lambda: call(DEVICE, DEVICE, 0.0, dev=host.ctypes.data, out=tptr[1])))
        allocs = engine.scene_allocations()
        for what, f in refusals:
            assert f() == E_INVALID, f"{name}: {what} was not refused"
            assert err(), what
            assert engine.sync() == 0
            assert np.array_equal(mem.numpy(targets[1]), before), f"{name}: {what}: a refused frame wrote its target"
            # the rotation is where it was: the next frame takes lane 0, the one after it lane 1
            engine.render_resident(W, H, BLACK, aa, out=targets[0], morph=(1, 1, 0.0))
            assert engine.sync() == 0 and np.array_equal(lane_image(), want_a), f"{name}: {what}: a refused frame moved the rotation"
            engine.render_resident(W, H, BLACK, aa, out=targets[2], morph=(0, 1, 0.0))
            assert engine.sync() == 0 and np.array_equal(lane_image(), want_b), f"{name}: {what}: a refused frame moved the rotation"
            assert np.array_equal(mem.numpy(targets[0]), want_b) and np.array_equal(mem.numpy(targets[2]), want_a), f"{name}: frames around the refusals"
        assert engine.scene_allocations() == allocs
        # an upload of a scene drops the keyframes
        engine.upload_scene(packed, layout)
        assert call(0, 0, 0.0) == E_INVALID and "keyframes" in err()
        engine.render_resident(W, H, BLACK, aa, morph=(SCENE, SCENE, 0.3))
        assert engine.sync() == 0
        engine.upload_path_keyframes(np.stack(keys))
        engine.upload_path_keyframes(None)
        assert call(0, 0, 0.0) == E_INVALID
        engine.upload_path_keyframes(keys[0])
        engine.render(packed, layout, W, H, BLACK, aa)  # (vello_hip_render's own upload)
        assert call(0, 0, 0.0) == E_INVALID
    finally:
        engine.set_frames_in_flight(1)
    # blends need floats: a scene with i16 segment tags refuses a blend and renders verbatim frames
    ipacked, ilayout = i16_scene()
    iown = path_words(ipacked, ilayout)
    ikey = iown.copy()
    ikey[: len(ikey) // 2] += np.uint32(3)  # x + 3 in the low half-word of some points
    ref_own = _oracle_image(ipacked, ilayout, W, H, BLACK, aa)
    ref_key = _oracle_image(substitute(ipacked, ilayout, ikey), ilayout, W, H, BLACK, aa)
    assert not np.array_equal(ref_own, ref_key) and ref_own.any()
    engine.upload_scene(ipacked, ilayout)
    engine.upload_path_keyframes(ikey.reshape(1, -1))
    assert call(SCENE, 0, 0.5) == E_INVALID and "i16" in err()
    for morph, ref in (((SCENE, 0, 0.0), ref_own), ((SCENE, 0, 1.0), ref_key), ((0, 0, 0.5), ref_key)):
        engine.render_resident(W, H, BLACK, aa, morph=morph)
        assert engine.sync() == 0
        assert np.array_equal(engine.read_buffer("output", np.uint8, W * H * 4).reshape(H, W, 4), ref), f"{name}: verbatim frame {morph} of an i16 scene"


# ---------------------------------------------------------------------------------------------------------------
# Public layer
# ---------------------------------------------------------------------------------------------------------------
def check_bindings(engine, mem, name):
    """path_data_view, upload_path_keyframes with float32 and uint32 arrays, render_resident(points=...) alone."""
    import vello_amd
    from vello_amd import AaConfig

    packed, layout = polygon_words_scene(258, seed=4)
    view = vello_amd.path_data_view(packed, layout)
    assert view.dtype == np.float32 and len(view) == 258 and np.array_equal(view.view(np.uint32), path_words(packed, layout))
    keys = two_keys(packed, layout, 4.0)
    W = H = 64
    want = _oracle_image(substitute(packed, layout, keys[1]), layout, W, H, BLACK, AaConfig.Msaa16)
    engine.upload_scene(packed, layout)
    assert engine.path_data_words() == 258
    for arr in (np.stack(keys), np.stack(keys).view(np.float32)):
        engine.upload_path_keyframes(arr)
        engine.render_resident(W, H, BLACK, AaConfig.Msaa16, morph=(vello_amd.PATH_DATA_SCENE, 1, 1.0))
        assert engine.sync() == 0
        assert np.array_equal(engine.read_buffer("output", np.uint8, W * H * 4).reshape(H, W, 4), want), name
    engine.upload_path_keyframes(None)
    engine.render_resident(W, H, BLACK, AaConfig.Msaa16, points=mem.words(keys[1], True), points_is_device=mem.points_is_device)
    assert engine.sync() == 0
    assert np.array_equal(engine.read_buffer("output", np.uint8, W * H * 4).reshape(H, W, 4), want), name
    if mem.points_is_device is False:
        with np.testing.assert_raises(ValueError):
            engine.render_resident(W, H, BLACK, AaConfig.Msaa16, points=keys[1].view(np.float32))
