"""The per-frame stroke scale (vello_hip_set_stroke_scale) against the CPU oracle.  The oracle has no such input: it is handed the
SUBSTITUTED scene -- the packed bytes with the width word of every style entry replaced by rule 1 of the contract, computed here in
numpy f32 (numpy rounds the one f32 product on its own), not by the library under test -- while the engine is handed the raw scene and
the setting.  tests.parity.compare_frame and tests.cull_parity.compare_culled_frame do the comparing through StrokeEngine, an adapter
that sets the setting around every blocking render on the engine's side only: every intermediate buffer and counter is held to the
tolerances the suite already uses.  Every case first asserts that the oracle tells the substituted scene from the raw one, so that an
engine that ignores the setting cannot pass."""
import ctypes

import numpy as np

from oracle.oracle import Oracle
from tests import cull_parity, parity
from tests import morph_parity as mp
from tests import view_parity as vp
from tests.parity import canonical_nan_lines, sorted_rows

BLACK, WHITE = 0xFF000000, 0xFFFFFFFF
E_INVALID = -1
STYLE_FLAGS_STYLE = 0x80000000
f32 = np.float32
THIRD = float(f32(1.0) / f32(3.0))  # 1/3f: products with full-mantissa widths round


# ---------------------------------------------------------------------------------------------------------------
# The expectation
# ---------------------------------------------------------------------------------------------------------------
def style_words(packed, layout):
    """(flags, width bits) of the scene's style entries: two uint32 views into `packed` (a C-contiguous uint8 array)."""
    w = packed.reshape(-1).view(np.uint32)
    n = (len(w) - layout.style_base) // 2
    st = w[layout.style_base: layout.style_base + 2 * n].reshape(-1, 2)
    return st[:, 0], st[:, 1]


def scaled(packed, layout, setting):
    """Rule 1: the packed scene with w' = (x < m ? m : x), x = fl(w * s), in the place of the width of every entry that is a stroke
    (flags & STYLE_FLAGS_STYLE) of width w > 0; every other word, every other width included, bit for bit."""
    s, m = f32(setting[0]), f32(setting[1])
    out = np.ascontiguousarray(packed, dtype=np.uint8).copy()
    flags, bits = style_words(out, layout)
    w = bits.view(np.float32)
    with np.errstate(all="ignore"):
        hit = ((flags & np.uint32(STYLE_FLAGS_STYLE)) != 0) & (w > f32(0.0))
        x = w * s
        assert x.dtype == np.float32
        x = np.where(x < m, m, x).astype(np.float32)
    bits[hit] = x.view(np.uint32)[hit]
    return out


def oracle_frame(packed, layout, w, h, base, aa, resolved=None):
    """(sorted soup, image) of the oracle on these bytes."""
    o = Oracle(capacity_scale=4, auto_grow=True)
    o.set_scene(packed, layout, w, h, base, int(aa))
    if resolved is not None:
        o.set_ramps(resolved.ramps)
        o.set_image_atlas(resolved.atlas_image())
    img = o.render().copy()
    return sorted_rows(canonical_nan_lines(o.buffer("lines", np.uint32)[: o.bump()["lines"] * 6]), 6), img


def assert_told_apart(name, raw, sub, layout, w, h, base, aa, resolved=None):
    a, b = oracle_frame(raw, layout, w, h, base, aa, resolved), oracle_frame(sub, layout, w, h, base, aa, resolved)
    assert a[0].shape != b[0].shape or not np.array_equal(a[0], b[0]) or not np.array_equal(a[1], b[1]), \
        f"{name}: the oracle cannot tell the scaled scene from the raw one: the case proves nothing"
    return b[1]


# ---------------------------------------------------------------------------------------------------------------
# The adapter
# ---------------------------------------------------------------------------------------------------------------
class StrokeEngine:
    """What compare_frame / compare_culled_frame see as the engine: every blocking render they ask for -- with the SUBSTITUTED bytes,
    which go to the oracle -- is the same render of the RAW bytes (`raw`; None: the bytes as handed in, for the adapters below it that
    bring their own) with the setting set on the engine; it is taken off again after every frame, so that a forgotten setting cannot
    leak into the next case.  `inner` may be another adapter (ViewEngine, MorphEngine, InstanceEngine ...)."""

    def __init__(self, inner, raw, setting):
        self._inner, self._raw, self._setting = inner, raw, setting
        self.frames = 0

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def render(self, packed, layout, width, height, base_color, aa, ramps=None):
        self._inner.set_stroke_scale(*self._setting)
        try:
            self.frames += 1
            return self._inner.render(packed if self._raw is None else self._raw, layout, width, height, base_color, aa, ramps=ramps)
        finally:
            self._inner.set_stroke_scale(None)


class FrameEngine:
    """Every blocking render is a vello_hip_render_frame of the same bytes (a private scene)."""

    def __init__(self, engine):
        self._engine = engine

    def __getattr__(self, k):
        return getattr(self._engine, k)

    def render(self, packed, layout, w, h, base, aa, ramps=None):
        e = self._engine
        e.render_frame(packed, layout, w, h, base, aa, ramps=ramps)
        assert e.sync() == 0
        return e.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4).copy(), e.bump()


class ResidentEngine:
    """Every blocking render is an upload of the bytes and a render_resident (the upload builds the scene index of a large scene)."""

    def __init__(self, engine):
        self._engine = engine

    def __getattr__(self, k):
        return getattr(self._engine, k)

    def render(self, packed, layout, w, h, base, aa, ramps=None):
        e = self._engine
        e.upload_scene(packed, layout, ramps)
        e.render_resident(w, h, base, aa)
        r = e.sync()
        assert r in (0, -4), r
        return e.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4).copy(), e.bump()


def compare_scaled_frame(engine, packed, layout, setting, w, h, base, aa, name, view=None, culled=False, wrap=None, **kw):
    """compare_frame (or compare_culled_frame) of the raw scene under `setting` = (s, m) against the oracle on the substituted scene.
    `view`: a view transform set on the engine, composed into the oracle's scene; `wrap`: an adapter put around the engine, below
    the setting (FrameEngine, ResidentEngine)."""
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    sub = scaled(packed, layout, setting)
    inner = wrap(engine) if wrap is not None else engine
    raw_scene, scene = packed, sub
    if view is not None:
        inner = vp.ViewEngine(inner, packed, view)
        raw_scene, scene = vp.compose(packed, layout, view), vp.compose(sub, layout, view)
    assert_told_apart(name, raw_scene, scene, layout, w, h, base, aa, kw.get("resolved"))
    se = StrokeEngine(inner, packed, setting)
    if culled:
        out = cull_parity.compare_culled_frame(se, scene, layout, w, h, base, aa, name, **kw)
    else:
        out = parity.compare_frame(se, scene, layout, w, h, base, aa, name, **kw)
    assert se.frames > 0
    return out[0], out[1], out[2]


def _tol(aa):
    return 1 if int(aa) == 0 else 0


# ---------------------------------------------------------------------------------------------------------------
# Scenes
# ---------------------------------------------------------------------------------------------------------------
def widths(n, seed=1):
    """n stroke widths with full mantissas: 1.1f, 2.7f, 0.3f first, then random ones of 0.3 .. 3.9."""
    rng = np.random.default_rng(seed)
    w = np.concatenate([np.array([1.1, 2.7, 0.3], dtype=np.float32), rng.uniform(0.3, 3.9, n).astype(np.float32)])[:n]
    return w


def lines_scene(n, odd, size=128.0):
    """n short stroked lines, a style entry each (the widths differ from stroke to stroke), on a grid over a size x size target.
    `odd`: the same scene one word further into its buffer, so that its style stream begins on an odd word.  (A draw object more does
    not shift the parity: a solid fill adds one draw tag and one draw-data word, its points and its transform even counts of words,
    and so does every stroke here -- the encoder's style stream always begins on an even word; the scene is moved by hand instead.)"""
    from vello_amd import Affine, BezPath, Cap, Color, Join, Scene, Stroke

    wd = widths(n)
    cols = int(np.ceil(np.sqrt(n)))
    step = (size - 8.0) / cols
    s = Scene()
    for k in range(n):
        x, y = 4.0 + step * (k % cols), 4.0 + step * (k // cols)
        p = BezPath()
        p.move_to((float(x), float(y)))
        p.line_to((float(x + 0.7 * step), float(y + 0.4 * step)))
        st = Stroke(float(wd[k]), join=Join(k % 3), start_cap=Cap(k % 3), end_cap=Cap((k // 3) % 3))
        s.stroke(st, Affine.IDENTITY, Color((k % 5) / 4.0, (k % 3) / 2.0, (k % 7) / 6.0, 1.0), None, p)
    packed, layout = s.resolve()
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    if odd:
        packed, layout = mp.shifted_scene(packed, layout)
        packed = np.ascontiguousarray(packed)
    flags, bits = style_words(packed, layout)
    assert len(flags) == n and ((flags & np.uint32(STYLE_FLAGS_STYLE)) != 0).all(), (n, len(flags))
    assert np.array_equal(bits.view(np.float32), wd), "a style entry per stroke, in order"
    assert layout.style_base % 2 == (1 if odd else 0), layout
    return packed, layout


PARTITIONS = (1, 2, 255, 256, 257, 513)


def branches_scene():
    """Rule 1's branches in one scene: a fill; a stroke with x > m; a stroke with x < m; a layer whose clip is a zero-width stroke (it
    stays empty under m > 0) around a fill; and three strokes whose width words are patched by hand to -1, a NaN with a payload and
    -0.  Returns (packed, layout, the indices of the patched style entries)."""
    from vello_amd import Affine, BezPath, Color, Fill, Rect, Scene, Stroke

    def seg(x0, y0, x1, y1):
        p = BezPath()
        p.move_to((x0, y0))
        p.line_to((x1, y1))
        p.line_to((x1 + 6.0, y0 + 3.0))
        return p

    s = Scene()
    s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(40, 90, 220), None, Rect(6.0, 6.0, 50.0, 30.0))
    s.stroke(Stroke(9.3), Affine.IDENTITY, Color.from_rgb8(250, 60, 40), None, seg(10.0, 50.0, 70.0, 60.0))      # x = 3.1 > m
    s.stroke(Stroke(1.7), Affine.IDENTITY, Color.from_rgb8(60, 250, 40), None, seg(10.0, 80.0, 70.0, 90.0))      # x = 0.57 < m
    s.push_clip_layer(Stroke(0.0), Affine.IDENTITY, seg(60.0, 10.0, 110.0, 40.0))
    s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(250, 250, 90), None, Rect(55.0, 5.0, 120.0, 45.0))
    s.pop_layer()
    first = None
    for k in range(3):
        s.stroke(Stroke(4.1 + k), Affine.IDENTITY, Color.from_rgb8(200, 40 + 60 * k, 250), None, seg(80.0, 60.0 + 18.0 * k, 118.0, 66.0 + 18.0 * k))
    packed, layout = s.resolve()
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    flags, bits = style_words(packed, layout)
    wf = bits.view(np.float32)
    first = int(np.flatnonzero(wf == f32(4.1))[0])
    patched = [first, first + 1, first + 2]
    assert [float(v) for v in wf[patched]] == [float(f32(4.1)), float(f32(5.1)), float(f32(6.1))]
    assert ((flags[patched] & np.uint32(STYLE_FLAGS_STYLE)) != 0).all()
    bits[patched[0]] = f32(-1.0).view(np.uint32)
    bits[patched[1]] = 0x7FC12345
    bits[patched[2]] = 0x80000000
    return packed, layout, patched


# ---------------------------------------------------------------------------------------------------------------
# 1. Kernel partitions, 2. rule 1's branches
# ---------------------------------------------------------------------------------------------------------------
def check_partition(engine, name, n, odd):
    from vello_amd import AaConfig

    packed, layout = lines_scene(n, odd)
    setting = (THIRD, 0.45)
    flags, bits = style_words(packed, layout)
    x = bits.view(np.float32) * f32(THIRD)
    if n >= 255:
        assert (x < f32(0.45)).any() and (x > f32(0.45)).any(), "both sides of the minimum"
        exact = (bits.view(np.float32).astype(np.float64) * np.float64(f32(THIRD)))
        assert (exact != x.astype(np.float64)).any(), "no product rounds: the case cannot tell a wider multiply"
    compare_scaled_frame(engine, packed, layout, setting, 128, 128, BLACK, AaConfig.Msaa16, f"{name}_{n}_{int(odd)}")


def check_branches(engine, name):
    from vello_amd import AaConfig

    packed, layout, patched = branches_scene()
    setting = (THIRD, 0.75)
    sub = scaled(packed, layout, setting)
    (f0, b0), (f1, b1) = style_words(packed, layout), style_words(sub, layout)
    assert np.array_equal(f0, f1)
    assert np.array_equal(b0[patched], b1[patched]) and [int(v) for v in b1[patched]] == [0xBF800000, 0x7FC12345, 0x80000000]
    fills = (f0 & np.uint32(STYLE_FLAGS_STYLE)) == 0
    assert fills.any() and np.array_equal(b0[fills], b1[fills])
    w1 = b1.view(np.float32)
    assert (w1 == f32(0.75)).sum() == 1 and (w1 == f32(9.3) * f32(THIRD)).sum() == 1
    for aa in (AaConfig.Msaa16, AaConfig.Area):
        # (a NaN-wide stroke: a NaN wins or loses a min / max depending on the order -- compare_frame's own rule for such scenes)
        compare_scaled_frame(engine, packed, layout, setting, 128, 128, BLACK, aa, f"{name}_{int(aa)}", tol=_tol(aa), order_sensitive=int(aa) == 0,
                             min_agree=None, back_half=False)


# ---------------------------------------------------------------------------------------------------------------
# 3. Off-state identity
# ---------------------------------------------------------------------------------------------------------------
def _hold_same(name, refs, got, layout, w, h):
    """`got` = (buffers, bump) of a frame against two frames of the reference route: word for word in every buffer whose layout the
    frame alone decides (the reference route's own two frames must agree there too), in compare_frame's canonical forms in the buffers
    of tests.retained_parity._ROWS, where the order of atomics decides."""
    from tests import retained_parity as rp

    (ref, ref_bump), (ref2, ref2_bump) = refs
    buf, bump = got
    for k, v in ref_bump.items():
        if k == "ptcl" and ref2_bump[k] != v:
            continue
        assert ref2_bump[k] == v, f"{name}: two frames of the reference route differ in bump.{k}"
        assert bump[k] == v, f"{name}: bump.{k} {bump[k]} != {v}"
    for k, v in ref.items():
        if k == "ptcl":
            continue  # (the words behind a tile's CMD_END are an earlier frame's -- here a frame of other widths: the lists are walked below)
        if k == "config":
            # (a resident frame does not send its Config to the device copy, a frame with the setting marks it for sending: what the
            # buffer must show is the scene's own layout -- never the style copy's base)
            assert [int(x) for x in buf[k][5:15]] == list(layout), f"{name}: VELLO_HIP_BUF_CONFIG does not hold the scene's own layout"
            continue
        if k in rp._ROWS:
            # (what the order of atomics lays out -- tile and segment offsets follow the order in which workgroups bump their pools, and two
            # frames that happen to agree say nothing about a third: these buffers are held in their canonical forms below)
            continue
        assert np.array_equal(v, ref2[k]), f"{name}: two frames of the reference route differ in {k}"
        assert np.array_equal(buf[k], v), f"{name}: VELLO_HIP_BUF_{k.upper()} differs"
    rp._compare_canonical(name, buf, ref, bump, ref_bump, layout, w, h)


def check_off_state(engine, name):
    """(1, 0) equals the off state in every buffer; NULL after a scaled frame restores it; a plain frame after a scaled one on the same
    buffer set shows the scene's widths."""
    import workloads
    from tests import retained_parity as rp
    from vello_amd import AaConfig

    w, h, aa = 160, 128, AaConfig.Msaa16
    packed, layout = workloads.random_test_scene(5, n_paths=80, size=128.0, strokes=True, clips=True).resolve()
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    sub = scaled(packed, layout, (2.5, 0.0))
    plain_img = oracle_frame(packed, layout, w, h, BLACK, aa)[1]
    wide_img = assert_told_apart(name, packed, sub, layout, w, h, BLACK, aa)
    engine.upload_scene(packed, layout)

    def frame(setting):
        engine.set_stroke_scale(*setting) if setting else engine.set_stroke_scale(None)
        engine.render_resident(w, h, BLACK, aa)
        assert engine.sync() == 0
        return rp._snapshot(engine, layout, w, h)

    try:
        refs = [frame(None), frame(None)]
        assert np.array_equal(refs[0][0]["output"].view(np.uint8).reshape(h, w, 4), plain_img)
        _hold_same(f"{name}_one_zero", refs, frame((1.0, 0.0)), layout, w, h)
        wide = frame((2.5, 0.0))
        assert np.array_equal(wide[0]["output"].view(np.uint8).reshape(h, w, 4), wide_img), f"{name}: the scaled frame"
        _hold_same(f"{name}_null_after_scaled", refs, frame(None), layout, w, h)
        assert np.array_equal(engine.read_buffer("scene", np.uint8, packed.nbytes), packed), f"{name}: the resident scene was modified"
    finally:
        engine.set_stroke_scale(None)


# ---------------------------------------------------------------------------------------------------------------
# 4. Every path a frame can take
# ---------------------------------------------------------------------------------------------------------------
def check_front_fusion(engine, name):
    import workloads
    from vello_amd import AaConfig

    packed, layout = workloads.stroke_styles_scene().resolve()
    try:
        engine.set_debug_flags(flatten_coop=True)
        before = engine.fused_launches()
        compare_scaled_frame(engine, packed, layout, (0.5, 2.0), 256, 256, WHITE, AaConfig.Msaa16, f"{name}_fused")
        assert engine.fused_launches() > before, f"{name}: the fused path was not taken"
        engine.set_debug_flags(flatten_coop=True, no_fusion=True)
        before = engine.fused_launches()
        compare_scaled_frame(engine, packed, layout, (0.5, 2.0), 256, 256, WHITE, AaConfig.Msaa16, f"{name}_nofusion")
        assert engine.fused_launches() == before
    finally:
        engine.set_debug_flags()


def check_tiny_fused(engine, name):
    """A scene of a few dozen segments: everything up to tile_alloc is ONE launch, cut behind the scan for a frame with the setting."""
    from vello_amd import AaConfig

    packed, layout = lines_scene(5, False, size=64.0)
    before = engine.fused_launches()
    compare_scaled_frame(engine, packed, layout, (3.0, 0.0), 64, 64, BLACK, AaConfig.Msaa16, name)
    assert engine.fused_launches() > before


def check_indexed(engine, name, back_half=True):
    """A scene above front_max_tags: with the index its upload builds and with no_scene_index; scaled frames build no index."""
    from tests import scene_index_parity as sip
    from vello_amd import AaConfig

    packed, layout = sip.case_scene("mixed")
    w, h, aa = sip.W, sip.H, AaConfig.Msaa16
    engine.set_auto_grow(True)
    try:
        for in_flight, flags in ((1, False), (1, True), (2, False)):  # (with frames in flight an indexed frame's flatten is k_flatten_front)
            engine.set_frames_in_flight(in_flight)
            engine.set_debug_flags(no_scene_index=flags)
            builds = engine.scene_index_builds()
            compare_scaled_frame(engine, packed, layout, (1.75, 1.0), w, h, BLACK, aa, f"{name}_{in_flight}_{int(not flags)}", wrap=ResidentEngine,
                                 oracle=sip.make_oracle(), back_half=back_half and in_flight == 1)
            uploads = 2 if back_half and in_flight == 1 else 1
            assert engine.scene_index_builds() == builds + uploads, f"{name}: scaled frames built {engine.scene_index_builds() - builds - uploads} scene indexes"
            for s in (0.5, 3.0):
                engine.set_stroke_scale(s, 0.25)
                engine.render_resident(w, h, BLACK, aa)
            engine.set_stroke_scale(None)
            assert engine.sync() == 0 and engine.scene_index_builds() == builds + uploads
    finally:
        engine.set_stroke_scale(None)
        engine.set_debug_flags()
        engine.set_frames_in_flight(1)
        engine.set_auto_grow(False)


def check_stroked_lines(engine, name, stroke_kernel):
    from vello_amd import AaConfig

    packed, layout = cull_parity.polyline_scene(n=120, size=256.0).resolve()
    try:
        engine.set_debug_flags(stroke_kernel=stroke_kernel)
        compare_scaled_frame(engine, packed, layout, (2.25, 0.0), 200, 152, WHITE, AaConfig.Msaa16, f"{name}_{int(stroke_kernel)}")
    finally:
        engine.set_debug_flags()


def check_curves(engine, name, which_kernels):
    """Stroked curves with round, bevel and miter joins and the three caps through a heavy walk."""
    import workloads
    from vello_amd import AaConfig

    packed, layout = workloads.stroke_styles_scene().resolve()
    try:
        engine.set_debug_flags(**{which_kernels: True})
        compare_scaled_frame(engine, packed, layout, (1.6, 0.0), 256, 256, BLACK, AaConfig.Msaa16, f"{name}_{which_kernels}")
    finally:
        engine.set_debug_flags()


def check_area(engine, name):
    import workloads
    from vello_amd import AaConfig

    packed, layout = workloads.random_test_scene(3, n_paths=120, size=200.0, strokes=True, clips=False).resolve()
    compare_scaled_frame(engine, packed, layout, (0.4, 1.25), 200, 160, BLACK, AaConfig.Area, name, tol=1)


def check_tiger(engine, name, size=512):
    from vello_amd import AaConfig

    packed, layout = cull_parity.tiger()
    compare_scaled_frame(engine, packed, layout, (0.5, 0.75), size, size, WHITE, AaConfig.Msaa8, name)


# ---------------------------------------------------------------------------------------------------------------
# 5. Composition with the other per-frame inputs
# ---------------------------------------------------------------------------------------------------------------
def _mixed(seed=3):
    import workloads

    packed, layout = workloads.random_test_scene(seed, n_paths=150, size=256.0, strokes=True, clips=True).resolve()
    return np.ascontiguousarray(packed, dtype=np.uint8), layout


def check_view(engine, name):
    """A view of zoom 2 with s = 0.5: strokes keep their width on screen."""
    from vello_amd import AaConfig, Affine

    packed, layout = _mixed()
    view = Affine.translate(-60.0, -40.0) * Affine.scale(2.0)
    compare_scaled_frame(engine, packed, layout, (0.5, 0.0), 200, 160, BLACK, AaConfig.Msaa16, name, view=view)


def check_culled(engine, name):
    """With vello_hip_set_viewport_cull: the rule is applied to the lines of the SCALED strokes, and lines are really dropped."""
    from vello_amd import AaConfig

    packed, layout = cull_parity.polyline_scene().resolve()
    compare_scaled_frame(engine, packed, layout, (2.5, 0.0), 175, 131, WHITE, AaConfig.Msaa16, name, culled=True, require_culling=True)


def check_damage(engine, name):
    from tests import damage_parity as dp
    from vello_amd import AaConfig

    packed, layout = _mixed(4)
    setting = (2.0, 1.5)
    sub = scaled(packed, layout, setting)
    assert_told_apart(name, packed, sub, layout, 200, 150, BLACK, AaConfig.Msaa16)
    ref = dp.Reference(sub, layout, 200, 150, BLACK, AaConfig.Msaa16)
    se = StrokeEngine(engine, packed, setting)
    dp.compare_damaged_frame(se, ref, dp.COMPOSE_RECT, name, no_cull=True)
    assert se.frames >= 4


def check_morph(engine, name):
    from vello_amd import AaConfig

    packed, layout = cull_parity.polyline_scene(n=60, size=200.0).resolve()
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    keys = mp.two_keys(packed, layout, 7.0)
    morph = (0, 1, 0.375)
    setting = (1.8, 0.0)
    want = mp.expected_words(mp.path_words(packed, layout), keys, None, *morph)
    morphed = mp.substitute(packed, layout, want)
    sub = scaled(morphed, layout, setting)
    assert_told_apart(name, morphed, sub, layout, 200, 150, BLACK, AaConfig.Msaa16)
    me = mp.MorphEngine(engine, packed, morph, keys)
    se = StrokeEngine(me, None, setting)
    parity.compare_frame(se, sub, layout, 200, 150, BLACK, AaConfig.Msaa16, name)
    assert me.frames > 0 and se.frames > 0


def check_render_frame(engine, name):
    from vello_amd import AaConfig

    packed, layout = _mixed(6)
    compare_scaled_frame(engine, packed, layout, (0.6, 1.0), 200, 160, BLACK, AaConfig.Msaa16, name, wrap=FrameEngine)


def _stroked_library(w, h, seed=31):
    from tests import retained_parity as rp

    return rp.scene_list(["solid", "polylines", "linear", "stroke_styles", "clip"], 9, w, h, seed)


def check_instances_painted(engine, name):
    """render_instances_painted: the kernel reads the COMPOSED style stream on the device."""
    from tests import instance_parity as ip
    from tests import paint_parity as pp
    from tests import retained_parity as rp
    from vello_amd import AaConfig

    w, h, aa = 200, 160, AaConfig.Msaa16
    lib, inst = _stroked_library(w, h)
    paints = rp.some_paints(len(inst))
    lib.upload(engine)
    packed, layout = rp.compose(lib, inst, paints)
    setting = (2.5, 0.0)
    sub = scaled(packed, layout, setting)
    late = ip._Late(lib)
    assert_told_apart(name, packed, sub, layout, w, h, BLACK, aa, late)
    pe = pp.PaintedEngine(engine, inst, paints)
    se = StrokeEngine(pe, None, setting)
    parity.compare_frame(se, sub, layout, w, h, BLACK, aa, name, resolved=late)
    assert pe.frames > 0
    assert np.array_equal(engine.read_buffer("scene", np.uint8, packed.nbytes), packed), f"{name}: VELLO_HIP_BUF_SCENE is not the composed scene"


def check_retained_painted(engine, name, device_poses=None):
    """render_retained_painted with device poses: the kernel reads the RETAINED style stream on the device."""
    from tests import instance_parity as ip
    from tests import repaint_parity as rpp
    from tests import retained_parity as rp
    from vello_amd import AaConfig

    w, h, aa = 200, 160, AaConfig.Msaa16
    lib, inst = _stroked_library(w, h, 33)
    n = len(inst)
    poses = rp.turned(inst, w, h, 2)
    p = rpp.frame_paints(n)
    q = rpp.effective(None, p, n)
    lib.upload(engine)
    packed, layout = rp.compose(lib, rp.posed(inst, poses), q)
    setting = (0.5, 1.0)
    sub = scaled(packed, layout, setting)
    late = ip._Late(lib)
    assert_told_apart(name, packed, sub, layout, w, h, BLACK, aa, late)
    kw = dict(poses=poses, pose_source="device", paints=p)
    if device_poses is not None:
        kw["device_poses"] = device_poses
    re = rpp.RepaintEngine(engine, inst, None, kw)
    se = StrokeEngine(re, None, setting)
    parity.compare_frame(se, sub, layout, w, h, BLACK, aa, name, resolved=late)
    assert re.frames > 0 and re.retains == 1
    rpp.assert_retained_bytes(engine, lib, inst, None, name)


# ---------------------------------------------------------------------------------------------------------------
# 6. Frames in flight
# ---------------------------------------------------------------------------------------------------------------
def check_in_flight(engine, mem, name):
    """Four frames in flight on ONE resident scene carry four settings into four targets, a plain frame after each; no scene buffer is
    allocated in the steady state."""
    from vello_amd import AaConfig

    w, h, aa = 128, 96, AaConfig.Msaa16
    packed, layout = _mixed(5)
    settings = [(0.5, 0.0), (2.0, 0.0), (THIRD, 1.5), (1.0, 12.0)]
    want = [oracle_frame(scaled(packed, layout, s), layout, w, h, BLACK, aa)[1] for s in settings]
    plain = oracle_frame(packed, layout, w, h, BLACK, aa)[1]
    assert all(not np.array_equal(x, plain) for x in want) and len({x.tobytes() for x in want}) == 4
    try:
        engine.set_frames_in_flight(4)
        engine.upload_scene(packed, layout)
        allocations = engine.scene_allocations()
        for rnd in range(3):
            scaled_t = [mem.target(w, h) for _ in range(4)]
            plain_t = [mem.target(w, h) for _ in range(4)]
            for k in range(4):  # (every lane: a scaled frame; then, on the same lanes, a plain one each)
                engine.set_stroke_scale(*settings[(k + rnd) % 4])
                engine.render_resident(w, h, BLACK, aa, out=scaled_t[k])
            engine.set_stroke_scale(None)
            for k in range(4):
                engine.render_resident(w, h, BLACK, aa, out=plain_t[k])
            assert engine.sync() == 0
            for k in range(4):
                assert np.array_equal(mem.numpy(scaled_t[k]), want[(k + rnd) % 4]), f"{name}: round {rnd}, frame {k} does not show its own setting"
                assert np.array_equal(mem.numpy(plain_t[k]), plain), f"{name}: round {rnd}: the plain frame on lane {k} after a scaled one"
            # ... and interleaved: scaled, plain, scaled, plain
            ts = [mem.target(w, h) for _ in range(4)]
            for k in range(4):
                engine.set_stroke_scale(*settings[k]) if k % 2 == 0 else engine.set_stroke_scale(None)
                engine.render_resident(w, h, BLACK, aa, out=ts[k])
            engine.set_stroke_scale(None)
            assert engine.sync() == 0
            for k in range(4):
                assert np.array_equal(mem.numpy(ts[k]), want[k] if k % 2 == 0 else plain), f"{name}: round {rnd}: interleaved frame {k}"
        assert engine.scene_allocations() == allocations, f"{name}: {engine.scene_allocations() - allocations} scene buffers allocated in the steady state"
        assert np.array_equal(engine.read_buffer("scene", np.uint8, packed.nbytes), packed), f"{name}: the resident scene was modified"
        cfg = engine.read_buffer("config", np.uint32, 88)
        assert int(cfg[5 + 9]) == layout.style_base, f"{name}: VELLO_HIP_BUF_CONFIG does not hold the scene's own layout"
    finally:
        engine.set_stroke_scale(None)
        engine.set_frames_in_flight(1)


# ---------------------------------------------------------------------------------------------------------------
# 7. Queries and stage runs
# ---------------------------------------------------------------------------------------------------------------
def check_queries_and_stages(engine, name):
    """pick on a point that only the widened stroke covers; pick_rect on its box; run_stages with and without FLATTEN in the range;
    read_buffer("scene") unchanged."""
    from vello_amd import AaConfig, Affine, BezPath, Cap, Color, Fill, Rect, Scene, Stroke

    s = Scene()
    s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(255, 0, 0), None, Rect(10.0, 10.0, 40.0, 40.0))
    p = BezPath()
    p.move_to((60.0, 100.0))
    p.line_to((140.0, 100.0))
    s.stroke(Stroke(2.0).with_caps(Cap.Butt), Affine.IDENTITY, Color.from_rgb8(0, 255, 0), None, p)  # y in 99 .. 101
    packed, layout = s.resolve()
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    w = h = 200
    aa = AaConfig.Msaa16
    setting = (8.0, 0.0)  # y in 92 .. 108
    plain = oracle_frame(packed, layout, w, h, BLACK, aa)[1]
    wide = oracle_frame(scaled(packed, layout, setting), layout, w, h, BLACK, aa)[1]
    assert not np.array_equal(plain, wide)
    pts = np.array([[100.0, 105.5], [100.0, 100.5], [25.0, 25.0], [100.0, 120.0]], dtype=np.float32)
    box = (59.0, 91.0, 141.0, 109.0)    # encloses the widened stroke
    above = (59.0, 91.0, 141.0, 96.0)   # touches the widened stroke only

    def image():
        return engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4)

    try:
        engine.upload_scene(packed, layout)
        engine.render_resident(w, h, BLACK, aa)
        assert engine.sync() == 0 and np.array_equal(image(), plain)
        assert [int(v) for v in engine.pick(pts)[:, 0]] == [0xFFFFFFFF, 1, 0, 0xFFFFFFFF]
        assert int(engine.pick_rect(above)[0][1]) == 0
        engine.set_stroke_scale(*setting)
        engine.render_resident(w, h, BLACK, aa)
        assert engine.sync() == 0 and np.array_equal(image(), wide), f"{name}: scaled image"
        assert [int(v) for v in engine.pick(pts)[:, 0]] == [1, 1, 0, 0xFFFFFFFF], f"{name}: pick does not answer against the scaled strokes"
        draws = engine.pick_rect(above)[0]
        assert int(draws[1]) & 1 and int(draws[0]) == 0, f"{name}: pick_rect does not answer against the scaled strokes ({draws})"
        assert int(engine.pick_rect(box)[0][1]) == 3, f"{name}: pick_rect on the widened stroke's box"
        # run_stages without FLATTEN in the range goes on from the lane's buffers as they are: the soup of the scaled frame
        engine.write_buffer("output", np.zeros(w * h * 4, dtype=np.uint8))
        engine.set_stroke_scale(None)
        engine.run_stages(w, h, BLACK, aa, "draw_scan", "fine")
        assert np.array_equal(image(), wide), f"{name}: run_stages behind flatten after a scaled frame"
        # with FLATTEN in the range the setting in force applies: off, then on
        engine.run_stages(w, h, BLACK, aa, "pathtag_scan", "fine")
        assert np.array_equal(image(), plain), f"{name}: run_stages with FLATTEN, setting off"
        engine.set_stroke_scale(*setting)
        engine.run_stages(w, h, BLACK, aa, "flatten", "fine")
        assert np.array_equal(image(), wide), f"{name}: run_stages with FLATTEN, setting on"
        assert np.array_equal(engine.read_buffer("scene", np.uint8, packed.nbytes), packed), f"{name}: the resident scene was modified"
        engine.set_stroke_scale(None)
        engine.render_resident(w, h, BLACK, aa)
        assert engine.sync() == 0 and np.array_equal(image(), plain)
    finally:
        engine.set_stroke_scale(None)


# ---------------------------------------------------------------------------------------------------------------
# 8. Refusals
# ---------------------------------------------------------------------------------------------------------------
def check_refusals(engine, mem, name):
    """Every refusal of rule 7: VELLO_HIP_E_INVALID, the setting and the rotation where they were -- checked after each by rendering."""
    from vello_amd import AaConfig

    lib, h = engine._lib, engine._h
    aa = AaConfig.Msaa16
    W = H = 64
    packed, layout = lines_scene(40, False, size=64.0)
    held = (2.5, 0.5)
    want_held = oracle_frame(scaled(packed, layout, held), layout, W, H, BLACK, aa)[1]
    plain = oracle_frame(packed, layout, W, H, BLACK, aa)[1]
    assert not np.array_equal(want_held, plain)
    nan, inf = float("nan"), float("inf")

    def call(s, m, ctx=h):
        return lib.vello_hip_set_stroke_scale(ctx, (ctypes.c_float * 2)(s, m))

    def err():
        return lib.vello_hip_last_error(h).decode()

    assert lib.vello_hip_set_stroke_scale(None, None) == E_INVALID and call(1.0, 0.0, ctx=None) == E_INVALID
    bad = [("s NaN", nan, 0.0, "scale"), ("s +inf", inf, 0.0, "scale"), ("s -inf", -inf, 0.0, "scale"), ("s 0", 0.0, 0.0, "scale"), ("s -0", -0.0, 0.0, "scale"),
           ("s < 0", -1.0, 0.0, "scale"), ("m NaN", 1.0, nan, "minimum"), ("m +inf", 1.0, inf, "minimum"), ("m -inf", 1.0, -inf, "minimum"),
           ("m < 0", 1.0, -0.5, "minimum")]
    engine.set_frames_in_flight(2)
    try:
        engine.upload_scene(packed, layout)
        # lane 0's internal target gets the plain image, lane 1's the held setting's: read_buffer("output") tells which lane a frame took
        engine.render_resident(W, H, BLACK, aa)
        engine.set_stroke_scale(*held)
        engine.render_resident(W, H, BLACK, aa)
        assert engine.sync() == 0

        def lane_image():
            return engine.read_buffer("output", np.uint8, W * H * 4).reshape(H, W, 4)

        assert np.array_equal(lane_image(), want_held)
        targets = [mem.target(W, H) for _ in range(2)]
        for state in ("on", "off"):
            if state == "off":
                engine.set_stroke_scale(None)
            want = want_held if state == "on" else plain
            for what, s, m, word in bad:
                assert call(s, m) == E_INVALID, f"{name}: {what} was not refused"
                assert word in err(), f"{name}: {what}: the message does not name the rule: {err()!r}"
                # the setting is what it was, and so is the rotation: the next frame takes lane 0, the one after it lane 1
                engine.render_resident(W, H, BLACK, aa, out=targets[0])
                assert engine.sync() == 0 and np.array_equal(lane_image(), plain), f"{name}: {what} ({state}): a refusal moved the rotation"
                engine.render_resident(W, H, BLACK, aa, out=targets[1])
                assert engine.sync() == 0 and np.array_equal(lane_image(), want_held), f"{name}: {what} ({state}): a refusal moved the rotation"
                for t in targets:
                    assert np.array_equal(mem.numpy(t), want), f"{name}: {what} ({state}): a refusal changed the setting"
    finally:
        engine.set_stroke_scale(None)
        engine.set_frames_in_flight(1)


# ---------------------------------------------------------------------------------------------------------------
# 9. Estimation
# ---------------------------------------------------------------------------------------------------------------
def check_estimator(make_engine, name):
    """estimate_capacities(stroke=...) is estimate_capacities of the substituted scene; NULL equals _view; monotone in s for lines and
    segments on a stroked scene; the same refusals; auto-grow renders a frame that overflows only under a large s."""
    import vello_amd
    from vello_amd import AaConfig, Affine
    from vello_amd._lib import Capacities, LayoutStruct, RenderParamsStruct
    from vello_amd.renderer import estimate_capacities as est

    import workloads

    packed, layout = workloads.stroke_styles_scene().resolve()
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    w = h = 256
    view = Affine.translate(-30.0, -20.0) * Affine.scale(1.7)
    for v in (None, view):
        assert est(packed, layout, w, h, view=v, stroke=None) == est(packed, layout, w, h, view=v)
        for setting in ((THIRD, 0.45), (4.0, 0.0), (1.0, 0.0), (0.01, 25.0)):
            assert est(packed, layout, w, h, view=v, stroke=setting) == est(scaled(packed, layout, setting), layout, w, h, view=v), (name, setting)
    lib = vello_amd.load_library()
    lay, p, c = LayoutStruct(*layout), RenderParamsStruct(w, h, 0, 0), Capacities()

    def raw(stroke, v=None):
        return lib.vello_hip_estimate_capacities_styled(packed.ctypes.data, packed.nbytes, ctypes.byref(lay), ctypes.byref(p), v, stroke, ctypes.byref(c))

    assert raw(None) == 0
    nan, inf = float("nan"), float("inf")
    for s, m in ((nan, 0.0), (inf, 0.0), (0.0, 0.0), (-1.0, 0.0), (1.0, nan), (1.0, inf), (1.0, -0.5)):
        assert raw((ctypes.c_float * 2)(s, m)) == E_INVALID, (name, s, m)
    last = None
    for s in (0.25, 1.0, 4.0, 16.0, 64.0):
        e = est(packed, layout, w, h, stroke=(s, 0.0))
        if last is not None:
            assert e["lines"] >= last["lines"] and e["seg_counts"] >= last["seg_counts"] and e["segments"] >= last["segments"], (name, s, e, last)
        last = e
    assert last["seg_counts"] > est(packed, layout, w, h)["seg_counts"] and last["lines"] > est(packed, layout, w, h)["lines"]
    # auto-grow: pools that hold the plain frame and overflow under a large s
    big = (24.0, 0.0)
    plain_need, big_need = est(packed, layout, w, h), est(packed, layout, w, h, stroke=big)
    caps = dict(plain_need)
    caps["blend_spill"] = 4096
    engine = make_engine(caps)
    img, bump = engine.render(packed, layout, w, h, WHITE, AaConfig.Msaa16)
    assert bump["failed"] == 0, f"{name}: the plain frame does not fit its own estimate: {bump}"
    engine.set_stroke_scale(*big)
    img, bump = engine.render(packed, layout, w, h, WHITE, AaConfig.Msaa16)
    assert bump["failed"] != 0, f"{name}: the scaled frame fits the plain frame's pools: the case proves nothing ({bump})"
    engine.set_auto_grow(True)
    img, bump = engine.render(packed, layout, w, h, WHITE, AaConfig.Msaa16)
    assert bump["failed"] == 0, f"{name}: auto-grow did not fit the scaled frame: {bump}"
    assert engine.last_render_attempts() == 1, f"{name}: {engine.last_render_attempts()} attempts: the pools were not sized from the styled estimate"
    grown = engine.capacities()
    assert grown["seg_counts"] >= big_need["seg_counts"] and grown["lines"] >= big_need["lines"]
    assert np.array_equal(img, oracle_frame(scaled(packed, layout, big), layout, w, h, WHITE, AaConfig.Msaa16)[1]), f"{name}: the grown frame's image"
    engine.set_stroke_scale(None)


# ---------------------------------------------------------------------------------------------------------------
# 10. Bindings
# ---------------------------------------------------------------------------------------------------------------
def check_engine_binding(engine, name):
    """Engine.set_stroke_scale(scale, min_width), its defaults and its off switch."""
    from vello_amd import AaConfig

    W = H = 64
    aa = AaConfig.Msaa16
    packed, layout = lines_scene(40, False, size=64.0)
    engine.upload_scene(packed, layout)

    def image(*setting):
        engine.set_stroke_scale(*setting)
        engine.render_resident(W, H, BLACK, aa)
        assert engine.sync() == 0
        return engine.read_buffer("output", np.uint8, W * H * 4).reshape(H, W, 4).copy()

    try:
        assert np.array_equal(image(2.5), oracle_frame(scaled(packed, layout, (2.5, 0.0)), layout, W, H, BLACK, aa)[1]), f"{name}: min_width defaults to 0"
        assert np.array_equal(image(0.5, 2.0), oracle_frame(scaled(packed, layout, (0.5, 2.0)), layout, W, H, BLACK, aa)[1])
        assert np.array_equal(image(), oracle_frame(packed, layout, W, H, BLACK, aa)[1]), f"{name}: set_stroke_scale() switches it off"
        with np.testing.assert_raises(RuntimeError):
            engine.set_stroke_scale(-1.0)
    finally:
        engine.set_stroke_scale(None)


def check_renderer(name):
    """RenderParams(stroke_scale=(s, m)) holds for that frame only."""
    import vello_amd
    from vello_amd import AaConfig, Affine, BezPath, Color, RenderParams, Renderer, Scene, Stroke

    s = Scene()
    for k in range(6):
        p = BezPath()
        p.move_to((8.0, 10.0 + 16.0 * k))
        p.line_to((110.0, 18.0 + 16.0 * k))
        s.stroke(Stroke(1.1 + 0.8 * k), Affine.IDENTITY, Color((k % 5) / 4.0, 1.0, (k % 3) / 2.0, 1.0), None, p)
    W, H = 128, 112
    packed, layout = s.resolve()
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    setting = (THIRD, 1.25)
    base = Color.from_rgb8(0, 0, 0)
    plain = oracle_frame(packed, layout, W, H, BLACK, AaConfig.Msaa16)[1]
    want = oracle_frame(scaled(packed, layout, setting), layout, W, H, BLACK, AaConfig.Msaa16)[1]
    assert not np.array_equal(plain, want)
    r = Renderer()
    t = np.zeros((H, W, 4), dtype=np.uint8)
    r.render_to_texture(s, t, RenderParams(base, W, H, AaConfig.Msaa16, stroke_scale=setting))
    assert np.array_equal(t, want), f"{name}: RenderParams(stroke_scale=...)"
    r.render_to_texture(s, t, RenderParams(base, W, H, AaConfig.Msaa16))
    assert np.array_equal(t, plain), f"{name}: the setting outlived its frame"
    with np.testing.assert_raises(vello_amd.VelloHipError):
        r.render_to_texture(s, t, RenderParams(base, W, H, AaConfig.Msaa16, stroke_scale=(0.0, 0.0)))
    r.render_to_texture(s, t, RenderParams(base, W, H, AaConfig.Msaa16))
    assert np.array_equal(t, plain), f"{name}: a refused setting changed the next frame"
