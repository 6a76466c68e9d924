"""The view transform (vello_hip_set_view_transform) against the CPU oracle.  The oracle has no such option: it is handed the
COMPOSED scene -- the packed bytes with the transform stream [transform_base, style_base) replaced by V.T, computed here in numpy f32
by the formula of include/vello_hip.h (not through Scene.append, so that the expectation does not depend on the library under test) --
while the engine is handed the raw scene with the view set.  tests.parity.compare_frame and tests.cull_parity.compare_culled_frame
do the comparing through ViewEngine, an adapter that swaps the scene on the engine's side only: every intermediate is held to the
tolerances the suite already uses."""
import os

import numpy as np

from oracle.oracle import Oracle
from tests import cull_parity, parity
from tests.parity import canonical_nan_lines, sorted_rows

BLACK, WHITE = 0xFF000000, 0xFFFFFFFF
f32 = np.float32


def view_floats(view):
    """Six f32 [m0 m1 m2 m3 t0 t1] of an Affine or a sequence (Transform::from_kurbo)."""
    c = view.c if hasattr(view, "c") else tuple(view)
    return np.array([float(v) for v in c], dtype=np.float32)


def compose(packed, layout, view):
    """The packed scene with every entry T of its transform stream replaced by V.T (vello_encoding/src/math.rs:51-73): f32, every
    product and every sum rounded on its own.  No other word changes -- the six words below the stream included."""
    v = view_floats(view)
    out = np.ascontiguousarray(packed, dtype=np.uint8).copy()
    words = out.view(np.uint32)
    n_xf = (layout.style_base - layout.transform_base) // 6
    if n_xf == 0:
        return out
    t = words[layout.transform_base: layout.transform_base + n_xf * 6].view(np.float32).reshape(-1, 6).copy()
    with np.errstate(all="ignore"):
        c = np.empty_like(t)
        c[:, 0] = f32(v[0] * t[:, 0]) + f32(v[2] * t[:, 1])
        c[:, 1] = f32(v[1] * t[:, 0]) + f32(v[3] * t[:, 1])
        c[:, 2] = f32(v[0] * t[:, 2]) + f32(v[2] * t[:, 3])
        c[:, 3] = f32(v[1] * t[:, 2]) + f32(v[3] * t[:, 3])
        c[:, 4] = (f32(v[0] * t[:, 4]) + f32(v[2] * t[:, 5])) + v[4]
        c[:, 5] = (f32(v[1] * t[:, 4]) + f32(v[3] * t[:, 5])) + v[5]
    assert c.dtype == np.float32
    words[layout.transform_base: layout.transform_base + n_xf * 6] = c.reshape(-1).view(np.uint32)
    return out


class ViewEngine:
    """What compare_frame / compare_culled_frame see as the engine: every blocking render they ask for -- with the COMPOSED bytes,
    which go to the oracle -- is a render of the RAW scene with the view set; everything else is the engine's own.  The view is
    taken off again after every frame, so that a forgotten view cannot leak into the next case."""

    def __init__(self, engine, raw_packed, view):
        self._engine, self._raw, self._view = engine, raw_packed, view
        self.frames = 0

    def __getattr__(self, name):
        return getattr(self._engine, name)

    def render(self, packed, layout, width, height, base_color, aa, ramps=None):
        self._engine.set_view_transform(self._view)
        try:
            self.frames += 1
            return self._engine.render(self._raw, layout, width, height, base_color, aa, ramps=ramps)
        finally:
            self._engine.set_view_transform(None)


def raw_image(packed, layout, width, height, base_color, aa, resolved=None):
    o = Oracle(capacity_scale=4, auto_grow=True)
    o.set_scene(packed, layout, width, height, base_color, int(aa))
    if resolved is not None:
        o.set_ramps(resolved.ramps)
        o.set_image_atlas(resolved.atlas_image())
    return o.render()


def compare_view_frame(engine, packed, layout, view, width, height, base_color, aa, name, culled=False, differs=True, **kw):
    """compare_frame (or compare_culled_frame) of the raw scene under `view` against the oracle on the composed scene; asserts first
    that the composed scene's image is not the raw scene's, so that an engine that ignores the view fails."""
    composed = compose(packed, layout, view)
    ve = ViewEngine(engine, np.ascontiguousarray(packed, dtype=np.uint8), view)
    if culled:
        out = cull_parity.compare_culled_frame(ve, composed, layout, width, height, base_color, aa, name, **kw)
    else:
        out = parity.compare_frame(ve, composed, layout, width, height, base_color, aa, name, **kw)
    assert ve.frames > 0
    img, ref, bump = out[0], out[1], out[2]
    if differs:
        raw = raw_image(packed, layout, width, height, base_color, aa, kw.get("resolved"))
        assert not np.array_equal(raw, ref), f"{name}: the view changes nothing in this scene: the case proves nothing"
    print(f"{name}: bump.lines {bump['lines']}")
    try:
        os.makedirs(parity.DUMP_DIR, exist_ok=True)
        with open(os.path.join(parity.DUMP_DIR, "view_transform_lines.txt"), "a") as fh:
            fh.write(f"{name} bump.lines {bump['lines']}\n")
    except OSError:
        pass
    return img, ref, bump


# ---------------------------------------------------------------------------------------------------------------
# Views (about a target of w x h)
# ---------------------------------------------------------------------------------------------------------------
def views(w, h):
    """(name, Affine): a pan, a zoom in about the middle, a zoom out to a fraction of the target, rotation x non-uniform scale x shear,
    a mirror (negative determinant: joins and caps change their orientation)."""
    from vello_amd import Affine

    cx, cy = w / 2.0, h / 2.0
    about = lambda a: Affine.translate(cx, cy) * a * Affine.translate(-cx, -cy)  # noqa: E731
    return [("pan", Affine.translate(-0.31 * w, 0.17 * h)),
            ("zoom_in", about(Affine.scale(2.75))),
            ("zoom_out", Affine.translate(0.1 * w, 0.2 * h) * Affine.scale(0.3)),
            ("rot_shear", about(Affine.rotate(0.6) * Affine.scale_non_uniform(1.4, 0.7) * Affine.skew(0.3, -0.15))),
            ("mirror", Affine.translate(w, 0.0) * Affine.scale_non_uniform(-1.0, 1.0) * about(Affine.rotate(-0.2)))]


IDENTITY = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def _aa_tol(aa):
    return 1 if int(aa) == 0 else 0


def _resolve(scene):
    import vello_amd

    return vello_amd.Resolver().resolve(scene)


def check_scene_views(engine, name, scene, w, h, base_color=BLACK, which=None, aas=None, flags=None, in_flight=1, back_half=True):
    """`scene` under each of views(w, h) (or those named in `which`), every intermediate and the image against the oracle."""
    from vello_amd import AaConfig

    r = _resolve(scene)
    aas = aas or (AaConfig.Msaa16, AaConfig.Area)
    try:
        if flags:
            engine.set_debug_flags(**flags)
        if in_flight != 1:
            engine.set_frames_in_flight(in_flight)
        for k, (vname, v) in enumerate(views(w, h)):
            if which is not None and vname not in which:
                continue
            aa = aas[k % len(aas)]
            compare_view_frame(engine, r.packed, r.layout, v, w, h, base_color, aa, f"{name}_{vname}_{int(aa)}", tol=_aa_tol(aa), resolved=r,
                               back_half=back_half)
    finally:
        if in_flight != 1:
            engine.set_frames_in_flight(1)
        if flags:
            engine.set_debug_flags()


def check_identity(engine, name):
    """The explicit identity composes (it is not a shortcut) and equals the off state on a finite scene: image, soup, counters."""
    import workloads
    from vello_amd import AaConfig

    packed, layout = workloads.random_test_scene(3, n_paths=200, size=256.0, strokes=True, clips=True).resolve()
    img0, b0 = engine.render(packed, layout, 256, 256, BLACK, AaConfig.Msaa16)
    soup0 = sorted_rows(canonical_nan_lines(engine.read_buffer("lines", np.uint32, b0["lines"] * 24)), 6)
    engine.set_view_transform(IDENTITY)
    try:
        img1, b1 = engine.render(packed, layout, 256, 256, BLACK, AaConfig.Msaa16)
        soup1 = sorted_rows(canonical_nan_lines(engine.read_buffer("lines", np.uint32, b1["lines"] * 24)), 6)
    finally:
        engine.set_view_transform(None)
    assert b0 == b1, f"{name}: {b0} {b1}"
    assert np.array_equal(soup0, soup1) and np.array_equal(img0, img1), name
    compare_view_frame(engine, packed, layout, IDENTITY, 256, 256, BLACK, AaConfig.Msaa16, name + "_oracle", differs=False)


def check_polygons_polylines(engine, name, stroke_kernel):
    check_scene_views(engine, f"{name}_polygons", cull_parity.polygon_scene(n=150, size=256.0), 200, 152, flags={"stroke_kernel": stroke_kernel},
                      which=("pan", "rot_shear"))
    check_scene_views(engine, f"{name}_polylines", cull_parity.polyline_scene(n=120, size=256.0), 200, 152, WHITE, flags={"stroke_kernel": stroke_kernel})


def check_curves(engine, name, which_kernels, case):
    """Curves and stroked curves by both kernel sets of flatten's heavy list."""
    import workloads

    mk = [workloads.cardioid_scene, workloads.funky_paths_scene, workloads.tricky_strokes_scene][case]
    r = mk()
    s, w, h = r if isinstance(r, tuple) else (r, 512, 512)
    w, h = min(w, 512), min(h, 512)
    check_scene_views(engine, f"{name}_{mk.__name__}_{which_kernels}", s, w, h, flags={which_kernels: True},
                      which=("zoom_in", "mirror") if case else ("pan", "rot_shear", "mirror"), in_flight=2 if case == 1 else 1)


def _sized(r, w=256, h=256):
    return r if isinstance(r, tuple) else (r, w, h)


def check_stroke_styles(engine, name, ref):
    import workloads

    if ref:
        s, w, h = _sized(workloads.ref_stroke_styles_scene(), 512, 512)
        check_scene_views(engine, name, s, min(w, 320), min(h, 300), WHITE, which=("zoom_out", "mirror", "rot_shear"))
    else:
        check_scene_views(engine, name, workloads.stroke_styles_scene(), 256, 256, WHITE)


BRUSH_SCENES = ("brushes_scene", "gradient_extend_scene", "two_point_radial_scene", "image_sampling_scene", "blurred_rounded_rect_scene")


def check_brushes(engine, name, which_scene):
    """Every transform-consuming branch of draw_leaf: gradient, image and blur inverses."""
    import workloads

    s, w, h = _sized(getattr(workloads, which_scene)())
    check_scene_views(engine, f"{name}_{which_scene}", s, min(w, 256), min(h, 256), which=("pan", "zoom_in", "rot_shear", "mirror"))


def check_clips(engine, name, which_scene):
    import workloads

    s, w, h = _sized(getattr(workloads, which_scene)())
    check_scene_views(engine, f"{name}_{which_scene}", s, min(w, 256), min(h, 256), which=("pan", "zoom_out", "rot_shear"))


def check_tiger(engine, name):
    from vello_amd import AaConfig

    packed, layout = cull_parity.tiger()
    for vname, v in views(320, 320):
        if vname in ("zoom_in", "rot_shear"):
            compare_view_frame(engine, packed, layout, v, 320, 320, WHITE, AaConfig.Msaa8, f"{name}_{vname}")


def check_front_fusion(engine, name):
    """A small scene whose stages share launches (k_front): the launches are taken under a view too (the scan and the stages that read
    transforms as two launches of the kernel), and NO_FUSION gives the same buffers."""
    import workloads
    from vello_amd import AaConfig

    for cname, scene, w, h in (("circle", workloads.circle_scene(), 256, 256), ("stroke_styles", workloads.stroke_styles_scene(), 256, 256)):
        packed, layout = scene.resolve()
        v = dict(views(w, h))["rot_shear"]
        try:
            engine.set_debug_flags(flatten_coop=True)
            before = engine.fused_launches()
            compare_view_frame(engine, packed, layout, v, w, h, WHITE, AaConfig.Msaa16, f"{name}_{cname}_fused")
            assert engine.fused_launches() > before, f"{name}_{cname}: the fused path was not taken"
            compare_view_frame(engine, packed, layout, v, w, h, WHITE, AaConfig.Area, f"{name}_{cname}_fused_area", tol=1)
            engine.set_debug_flags(flatten_coop=True, no_fusion=True)
            before = engine.fused_launches()
            compare_view_frame(engine, packed, layout, v, w, h, WHITE, AaConfig.Msaa16, f"{name}_{cname}_nofusion")
            assert engine.fused_launches() == before
        finally:
            engine.set_debug_flags()


# Non-extreme fuzz seeds below 40 whose image under their view (views(128, 128)[seed % 5]) IS the raw scene's, by the oracle on both
# (content that covers the target either way, or lies off it either way): they still hold the engine to the oracle, but cannot tell
# an engine that ignores the view.  Every other non-extreme seed asserts that the view changes the image.
FUZZ_VIEW_INVARIANT = frozenset((6, 20, 28, 30, 35, 37))


def check_fuzz(engine, name, seeds, extreme):
    """workloads.fuzz under a view, as the cull suite picks its seeds.  The non-extreme seeds assert that the view changes the image,
    but for those the oracle finds invariant (FUZZ_VIEW_INVARIANT; seeds of 40 and more are not classified and do not assert it); the
    extreme seeds have non-finite geometry: whether the view
    changes the image is not asserted for them."""
    import vello_amd
    from vello_amd import AaConfig
    from workloads.fuzz import fuzz_scene

    engine.set_auto_grow(True)
    try:
        for seed in seeds:
            r = vello_amd.Resolver().resolve(fuzz_scene(seed, n_ops=14, extreme=True) if extreme else fuzz_scene(seed))
            aa = [AaConfig.Area, AaConfig.Msaa8, AaConfig.Msaa16][seed % 3]
            vname, v = views(128, 128)[seed % 5]
            compare_view_frame(engine, r.packed, r.layout, v, 128, 128, [BLACK, WHITE, 0x00000000, 0x80FF8040][seed % 4], aa, f"{name}_{seed}_{vname}",
                               tol=_aa_tol(aa), resolved=r, order_sensitive=True, back_half=not extreme, min_agree=None if extreme else 0.99,
                               differs=not extreme and seed < 40 and seed not in FUZZ_VIEW_INVARIANT, oracle=Oracle(capacity_scale=4, auto_grow=True))
    finally:
        engine.set_auto_grow(False)


# ---------------------------------------------------------------------------------------------------------------
# Stream shapes
# ---------------------------------------------------------------------------------------------------------------
def check_stream_shapes(engine, name):
    from vello_amd import AaConfig, Affine, Color, Fill, Rect, Scene

    # n_xf = 1
    s = Scene()
    for k in range(5):
        s.fill(Fill.NonZero, Affine.IDENTITY, Color(0.2 * k, 1.0 - 0.2 * k, 0.5, 1.0), None, Rect(10.0 + 20 * k, 10.0, 25.0 + 20 * k, 90.0))
    packed, layout = s.resolve()
    assert (layout.style_base - layout.transform_base) // 6 == 1
    compare_view_frame(engine, packed, layout, views(128, 100)[3][1], 128, 100, BLACK, AaConfig.Msaa8, f"{name}_one_transform")
    # one transform per path, a count that is no multiple of 64 or 256
    s = Scene()
    n = 331
    for k in range(n):
        a = Affine.translate(6.0 + 11.0 * (k % 23), 5.0 + 13.0 * (k // 23)) * Affine.rotate(0.07 * k) * Affine.scale(0.5 + (k % 7) * 0.2)
        s.fill(Fill.NonZero, a, Color((k % 5) / 4.0, (k % 3) / 2.0, (k % 7) / 6.0, 1.0), None, Rect(-4.0, -3.0, 4.0, 3.0))
    packed, layout = s.resolve()
    n_xf = (layout.style_base - layout.transform_base) // 6
    assert n_xf == n and n_xf % 64 != 0, n_xf
    for vname in ("zoom_in", "mirror"):
        compare_view_frame(engine, packed, layout, dict(views(260, 200))[vname], 260, 200, BLACK, AaConfig.Msaa16, f"{name}_{n}_transforms_{vname}")
    # an empty scene
    packed, layout = Scene().resolve()
    compare_view_frame(engine, packed, layout, views(64, 64)[1][1], 64, 64, 0xFF102030, AaConfig.Msaa8, f"{name}_empty", differs=False)


def check_trans_ix_minus_one(engine, name):
    """scene.rs:179-183 as a scene's first operation: tags with trans_ix = 0 - 1 read the six words below the stream, uncomposed; the
    layer's content stays suppressed and the later fill moves with the view."""
    from vello_amd import AaConfig, Affine, Circle, Color, Fill, Rect, Scene, Stroke

    s = Scene()
    s.push_clip_layer(Stroke(0.0), Affine.IDENTITY, Circle((40.0, 40.0), 20.0))
    s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(0, 255, 0), None, Rect(0.0, 0.0, 80.0, 80.0))
    s.pop_layer()
    s.fill(Fill.NonZero, Affine.translate(3.0, 4.0), Color.from_rgb8(255, 0, 0), None, Rect(10.0, 10.0, 30.0, 30.0))
    r = _resolve(s)
    img, _, _ = compare_view_frame(engine, r.packed, r.layout, Affine.translate(30.0, 25.0), 80, 80, BLACK, AaConfig.Msaa8, name, resolved=r)
    assert (img[:, :, 1] == 0).all(), "the zero-width stroke clip suppresses everything inside the layer"
    assert tuple(img[50, 50]) == (255, 0, 0, 255) and tuple(img[20, 20]) == (0, 0, 0, 255), "the later fill moved with the view"


# ---------------------------------------------------------------------------------------------------------------
# Life cycle
# ---------------------------------------------------------------------------------------------------------------
def _target_ptr(t):
    return t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr()


def render_resident_into(engine, w, h, base_color, aa, target):
    """vello_hip_render_resident into `target`: a torch tensor on the GPU, or -- the emulated build only, where device memory is host
    memory -- a numpy array (Engine.render_resident refuses those for the real library's sake)."""
    import ctypes

    p = engine._params(w, h, base_color, aa)
    engine._check(engine._lib.vello_hip_render_resident(engine._h, ctypes.byref(p), _target_ptr(target), w * 4), "render_resident")


def render_frame_into(engine, packed, layout, w, h, base_color, aa, target, ramps=None):
    import ctypes

    from vello_amd._lib import LayoutStruct

    p = engine._params(w, h, base_color, aa)
    lay = LayoutStruct(*layout)
    rp, nr = None, 0
    if ramps is not None and len(ramps):
        ramps = np.ascontiguousarray(ramps, dtype=np.uint32)
        rp, nr = ramps.ctypes.data, ramps.size // 512
    engine._check(engine._lib.vello_hip_render_frame(engine._h, packed.ctypes.data, packed.nbytes, ctypes.byref(lay), ctypes.byref(p), rp, nr,
                                                     _target_ptr(target), w * 4), "render_frame")


def check_in_flight(engine, name, make_target, to_numpy):
    """Four frames in flight on ONE resident scene, four views, four targets, then NULL: every target is its own view's oracle image, the
    last the raw scene's; the resident scene's bytes are the upload afterwards."""
    import workloads
    from vello_amd import AaConfig

    w, h = 200, 160
    packed, layout = workloads.random_test_scene(5, n_paths=200, size=256.0, strokes=True, clips=True).resolve()
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    vs = [v for _, v in views(w, h)[:4]]
    want = []
    for v in vs + [None]:
        o = Oracle()
        o.set_scene(packed if v is None else compose(packed, layout, v), layout, w, h, BLACK, int(AaConfig.Msaa16))
        want.append(o.render().copy())
    assert all(not np.array_equal(want[i], want[4]) for i in range(4))
    try:
        engine.set_frames_in_flight(4)
        engine.upload_scene(packed, layout)
        for rnd in range(2):
            targets = [make_target(w, h) for _ in range(5)]
            for k in range(4):
                engine.set_view_transform(vs[(k + rnd) % 4])
                render_resident_into(engine, w, h, BLACK, AaConfig.Msaa16, targets[k])
            engine.set_view_transform(None)
            render_resident_into(engine, w, h, BLACK, AaConfig.Msaa16, targets[4])
            assert engine.sync() == 0
            for k in range(4):
                assert np.array_equal(to_numpy(targets[k]), want[(k + rnd) % 4]), f"{name}: round {rnd}, frame {k} does not show its own view"
            assert np.array_equal(to_numpy(targets[4]), want[4]), f"{name}: round {rnd}: the frame after NULL is not the raw scene"
        assert np.array_equal(engine.read_buffer("scene", np.uint8, packed.nbytes), packed), f"{name}: the resident scene was modified"
    finally:
        engine.set_view_transform(None)
        engine.set_frames_in_flight(1)


def check_render_frame_and_stages(engine, name, make_target, to_numpy):
    """A view set between vello_hip_render_frame calls (each frame's private scene under the view of its call), and vello_hip_run_stages
    ranges that start at FLATTEN and at DRAW_SCAN."""
    import workloads
    from vello_amd import AaConfig

    w, h = 200, 160
    r = _resolve(workloads.brushes_scene())
    packed = np.ascontiguousarray(r.packed, dtype=np.uint8)
    layout = r.layout
    if r.atlas_size:
        engine.resize_image_atlas(r.atlas_size, r.atlas_size)
        for x, y, px in r.uploads:
            engine.write_image(x, y, px)
    va, vb = views(w, h)[0][1], views(w, h)[3][1]

    def want(v):
        o = Oracle()
        o.set_scene(packed if v is None else compose(packed, layout, v), layout, w, h, BLACK, int(AaConfig.Msaa8))
        o.set_ramps(r.ramps)
        o.set_image_atlas(r.atlas_image())
        return o.render().copy(), o

    try:
        engine.set_frames_in_flight(2)
        t = [make_target(w, h) for _ in range(3)]
        for k, v in enumerate((va, vb, None)):
            engine.set_view_transform(v)
            render_frame_into(engine, packed, layout, w, h, BLACK, AaConfig.Msaa8, t[k], ramps=r.ramps)
        assert engine.sync() == 0
        for k, v in enumerate((va, vb, None)):
            assert np.array_equal(to_numpy(t[k]), want(v)[0]), f"{name}: render_frame {k}"
    finally:
        engine.set_view_transform(None)
        engine.set_frames_in_flight(1)
    # run_stages: the front of the frame without a view, then the range from FLATTEN (and from DRAW_SCAN) under one
    ref, o = want(vb)
    n_lines = o.bump()["lines"]
    soup_o = sorted_rows(canonical_nan_lines(o.buffer("lines", np.uint32)[: n_lines * 6]), 6)
    info_o = parity.canonical_nan_words(o.buffer("info_bin_data", np.uint32)[: layout.bin_data_start])
    engine.upload_scene(packed, layout, r.ramps)
    try:
        engine.run_stages(w, h, BLACK, AaConfig.Msaa8, "pathtag_scan", "pathtag_scan")
        engine.set_view_transform(vb)
        engine.run_stages(w, h, BLACK, AaConfig.Msaa8, "flatten", "fine")
        b = engine.bump()
        assert b["failed"] == 0 and b["lines"] == n_lines, f"{name}: {b}"
        assert np.array_equal(sorted_rows(canonical_nan_lines(engine.read_buffer("lines", np.uint32, n_lines * 24)), 6), soup_o), f"{name}: soup from FLATTEN"
        assert np.array_equal(engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4), ref), f"{name}: image of the range from FLATTEN"
        # from DRAW_SCAN: the front of the frame under another view, the draw stage under this one -- its info words are this view's
        engine.set_view_transform(va)
        engine.run_stages(w, h, BLACK, AaConfig.Msaa8, "pathtag_scan", "flatten")
        engine.set_view_transform(vb)
        engine.run_stages(w, h, BLACK, AaConfig.Msaa8, "draw_scan", "draw_scan")
        assert np.array_equal(parity.canonical_nan_words(engine.read_buffer("info_bin_data", np.uint32, layout.bin_data_start * 4)), info_o), f"{name}: draw info from DRAW_SCAN"
        info_a = parity.canonical_nan_words(want(va)[1].buffer("info_bin_data", np.uint32)[: layout.bin_data_start])
        assert not np.array_equal(info_a, info_o)
        assert np.array_equal(engine.read_buffer("scene", np.uint8, packed.nbytes), packed), f"{name}: the resident scene was modified"
        cfg = engine.read_buffer("config", np.uint32, 88)
        assert int(cfg[5 + 8]) == layout.transform_base, f"{name}: VELLO_HIP_BUF_CONFIG does not hold the scene's own layout"
    finally:
        engine.set_view_transform(None)


def check_no_reallocation(engine, name, make_target, to_numpy):
    """vello_hip_render_frame scenes whose transform counts alternate between k and k + 1 on one lane: once the lane's scene buffer
    holds the larger one, no frame allocates again (a re-allocation frees device memory, which waits for every frame in flight) --
    with a view and without."""
    from vello_amd import AaConfig, Affine, Color, Fill, Rect, Scene

    def scene(n):
        s = Scene()
        for k in range(n):
            s.fill(Fill.NonZero, Affine.translate(5.0 + 9.0 * k, 7.0 + 3.0 * k), Color(0.1 * (k % 10), 0.5, 1.0 - 0.1 * (k % 10), 1.0), None, Rect(0.0, 0.0, 8.0, 8.0))
        packed, layout = s.resolve()
        assert (layout.style_base - layout.transform_base) // 6 == n
        return np.ascontiguousarray(packed, dtype=np.uint8), layout

    w, h = 128, 64
    small, large = scene(10), scene(11)
    assert small[0].nbytes < large[0].nbytes
    v = Affine.translate(3.0, 2.0)
    want = {}
    for key, (packed, layout) in (("small", small), ("large", large)):
        for vk, view in (("view", v), ("raw", None)):
            o = Oracle()
            o.set_scene(packed if view is None else compose(packed, layout, view), layout, w, h, BLACK, int(AaConfig.Msaa8))
            want[key, vk] = o.render().copy()
    for n_lanes in (1, 2):
        try:
            engine.set_frames_in_flight(n_lanes)
            t = make_target(w, h)
            # (both scenes once on every lane: the buffers reach their high-water mark)
            for key in ("small", "large") * n_lanes + ("large", "small") * n_lanes:
                render_frame_into(engine, *(small if key == "small" else large), w, h, BLACK, AaConfig.Msaa8, t)
            assert engine.sync() == 0
            before = engine.scene_allocations()
            for k in range(12):
                key = ("small", "large", "large", "small", "large", "small")[k % 6]
                vk = "view" if k % 4 < 2 else "raw"
                engine.set_view_transform(v if vk == "view" else None)
                render_frame_into(engine, *(small if key == "small" else large), w, h, BLACK, AaConfig.Msaa8, t)
                assert engine.sync() == 0
                assert np.array_equal(to_numpy(t), want[key, vk]), f"{name}: frame {k} ({key}, {vk}), {n_lanes} in flight"
            assert engine.scene_allocations() == before, f"{name}: {engine.scene_allocations() - before} scene buffers re-allocated in the steady state"
        finally:
            engine.set_view_transform(None)
            engine.set_frames_in_flight(1)


def check_errors(engine, name):
    """NaN or infinity in the view: E_INVALID, nothing changes (neither the off state nor a view set before)."""
    import ctypes

    import workloads
    from vello_amd import AaConfig

    packed, layout = workloads.stroke_styles_scene().resolve()
    lib = engine._lib
    assert lib.vello_hip_set_view_transform(None, (ctypes.c_float * 6)(*IDENTITY)) == -1
    img0, b0 = engine.render(packed, layout, 256, 256, WHITE, AaConfig.Msaa16)
    for bad in (float("nan"), float("inf"), float("-inf")):
        for k in range(6):
            v = list(IDENTITY)
            v[k] = bad
            assert lib.vello_hip_set_view_transform(engine._h, (ctypes.c_float * 6)(*v)) == -1, (bad, k)
    img1, b1 = engine.render(packed, layout, 256, 256, WHITE, AaConfig.Msaa16)
    assert b0 == b1 and np.array_equal(img0, img1), f"{name}: a refused view changed the next frame"
    v = views(256, 256)[3][1]
    engine.set_view_transform(v)
    try:
        bad = list(IDENTITY)
        bad[4] = float("nan")
        assert lib.vello_hip_set_view_transform(engine._h, (ctypes.c_float * 6)(*bad)) == -1
        img2, _ = engine.render(packed, layout, 256, 256, WHITE, AaConfig.Msaa16)
    finally:
        engine.set_view_transform(None)
    o = Oracle()
    o.set_scene(compose(packed, layout, v), layout, 256, 256, WHITE, int(AaConfig.Msaa16))
    assert np.array_equal(img2, o.render()), f"{name}: a refused view replaced the one set before"
    # a singular view is legal: everything collapses onto a line, as the composed scene does
    compare_view_frame(engine, packed, layout, (1.0, 0.5, 2.0, 1.0, 10.0, 20.0), 256, 256, WHITE, AaConfig.Msaa16, f"{name}_singular")


def check_culled(engine, name):
    """With vello_hip_set_viewport_cull: the rule is applied to the lines of the VIEWED scene, and lines are really dropped."""
    from vello_amd import AaConfig, Affine

    r = _resolve(cull_parity.polyline_scene())
    v = Affine.translate(-205.0, -154.0)
    compare_view_frame(engine, r.packed, r.layout, v, 175, 131, WHITE, AaConfig.Msaa16, f"{name}_polylines_pan", culled=True, require_culling=True)
    v = Affine.translate(-614.0, -461.0) * Affine.scale(3.0)
    compare_view_frame(engine, r.packed, r.layout, v, 256, 249, WHITE, AaConfig.Area, f"{name}_polylines_zoom", culled=True, require_culling=True, tol=1)
    packed, layout = cull_parity.tiger()
    v = Affine.translate(-300.0, -260.0) * Affine.scale(2.5)
    compare_view_frame(engine, packed, layout, v, 320, 320, WHITE, AaConfig.Msaa8, f"{name}_tiger_zoom", culled=True, require_culling=True)


def check_estimator(make_engine, name):
    """estimate_capacities(view=V) is estimate_capacities of the composed scene: the estimator composes in f32 by the same formula where
    it reads a transform, and the rest is the same f64 walk over the same words, so equality is exact.  Auto-grow from tiny pools under a
    zoom-in view: the pre-sizing asks the estimator with the context's view, so the first attempt fits."""
    import vello_amd
    import vello_amd.renderer
    import workloads
    from vello_amd import AaConfig

    packed, layout = workloads.random_test_scene(3, n_paths=300, size=512.0, strokes=True, clips=True).resolve()
    w, h = 400, 300
    for vname, v in views(w, h):
        a = vello_amd.renderer.estimate_capacities(packed, layout, w, h, view=v)
        b = vello_amd.renderer.estimate_capacities(compose(packed, layout, v), layout, w, h)
        assert a == b, f"{name} {vname}: {a} != {b}"
    assert vello_amd.renderer.estimate_capacities(packed, layout, w, h, view=None) == vello_amd.renderer.estimate_capacities(packed, layout, w, h)
    plain = vello_amd.renderer.estimate_capacities(packed, layout, w, h)
    zoom = dict(views(w, h))["zoom_in"]
    zoomed = vello_amd.renderer.estimate_capacities(packed, layout, w, h, view=zoom)
    assert zoomed["seg_counts"] > plain["seg_counts"], (plain, zoomed)
    with np.testing.assert_raises(vello_amd.VelloHipError):
        vello_amd.renderer.estimate_capacities(packed, layout, w, h, view=(1, 0, 0, float("nan"), 0, 0))
    # auto-grow: tiny pools, the zoom-in view
    o = Oracle(capacity_scale=4, auto_grow=True)
    o.set_scene(compose(packed, layout, zoom), layout, w, h, BLACK, int(AaConfig.Msaa16))
    ref = o.render()
    tiny = {"lines": 1024, "seg_counts": 1024, "segments": 1024, "tiles": 1024, "ptcl": 64 * 19 * 25 + 1024, "bin_data": layout.bin_data_start + 256}
    eng = make_engine(tiny)
    eng.set_auto_grow(True)
    eng.set_view_transform(zoom)
    img, bump = eng.render(packed, layout, w, h, BLACK, AaConfig.Msaa16)
    assert bump["failed"] == 0 and np.array_equal(img, ref), f"{name}: {bump}"
    assert eng.last_render_attempts() == 1, f"{name}: {eng.last_render_attempts()} attempts: the pre-sizing did not use the view"
    caps = eng.capacities()
    assert caps["lines"] >= zoomed["lines"] and caps["seg_counts"] >= zoomed["seg_counts"], (caps, zoomed)
    # (the pools the pre-sizing grows are set to the estimate itself: sized without the view, seg_counts would be plain["seg_counts"],
    # which is below zoomed["seg_counts"] (asserted above) -- and a single attempt means the grow loop never ran to raise it)
    assert caps["seg_counts"] > plain["seg_counts"]


def check_renderer(name):
    """Public layer: Renderer.render_to_texture with RenderParams(view=...) equals the Engine path (the oracle on the composed scene);
    a later frame without view is the raw scene."""
    import vello_amd
    import workloads
    from vello_amd import AaConfig, Color, RenderParams

    scene = workloads.random_test_scene(3, n_paths=200, size=256.0, strokes=True, clips=True)
    packed, layout = scene.resolve()
    w, h = 200, 160
    v = views(w, h)[3][1]
    r = vello_amd.Renderer()
    imgs = []
    for view in (v, None, view_floats(v)):
        out = np.zeros((h, w, 4), dtype=np.uint8)
        r.render_to_texture(scene, out, RenderParams(Color.from_rgb8(0, 0, 0), w, h, AaConfig.Msaa16, view=view))
        imgs.append(out)
    o = Oracle()
    o.set_scene(compose(packed, layout, v), layout, w, h, BLACK, int(AaConfig.Msaa16))
    assert np.array_equal(imgs[0], o.render()), f"{name}: RenderParams(view=...)"
    assert np.array_equal(imgs[2], imgs[0])
    o.set_scene(packed, layout, w, h, BLACK, int(AaConfig.Msaa16))
    assert np.array_equal(imgs[1], o.render()), f"{name}: the frame after a view frame is not the raw scene"
    with np.testing.assert_raises(vello_amd.VelloHipError):
        r.render_to_texture(scene, np.zeros((h, w, 4), dtype=np.uint8), RenderParams(Color.from_rgb8(0, 0, 0), w, h, AaConfig.Msaa16, view=(1, 0, 0, 1, float("inf"), 0)))
