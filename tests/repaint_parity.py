"""Per-frame paints of retained instance lists (vello_hip_render_retained_painted) against the CPU oracle and against
vello_hip_render_instances_painted.  A list is retained with paints R and rendered under poses X and frame paints P; the frame must be
the one of (fragment_i, X_i) under Q, Q_i = P_i where P_i is SOLID, else R_i.  The oracle is handed paint_parity.compose(lib,
posed(inst, X), Q) -- numpy, not the library under test.  Every intermediate is held at the tolerances the suite already uses; nothing
here has a tolerance of its own.

`device_paints(array)` / `device_poses(array)` turn a PAINT_DTYPE / (n, 6) float32 array into what stands for device memory: a torch
tensor on the GPU, or -- the emulated build, where the two are one address space -- the numpy array itself."""
import ctypes

import numpy as np

from tests import instance_parity as ip
from tests import paint_parity as pp
from tests import parity
from tests import retained_parity as rp
from tests import view_parity

BLACK, WHITE = ip.BLACK, ip.WHITE
KEEP, SOLID = pp.KEEP, pp.SOLID


def _same(x):
    return x


def paint_list(paints, n):
    """A PAINT_DTYPE array of what Engine.render_instances takes as `paints` (None: KEEP everywhere)."""
    from vello_amd import PAINT_DTYPE

    out = np.zeros(n, dtype=PAINT_DTYPE)
    if paints is not None:
        for i, (f, c) in enumerate(pp._pairs(paints, n)):
            out[i] = (f, c)
    return out


def effective(retained, frame, n):
    """Q: the frame's paint where it is SOLID, else what the list was retained with."""
    r, p = paint_list(retained, n), paint_list(frame, n)
    q = r.copy()
    solid = p["flags"] == SOLID
    q[solid] = p[solid]
    return q


def frame_paints(n, seed=0):
    """KEEP and SOLID interleaved, colours no retained paint (pp.word) and no library colour has: translucent and opaque ones."""
    return [None if (k + seed) % 2 == 0 else ((0xFF, 0xC0)[k % 4 == 1] << 24) | (0x203000 + 0x050309 * k + seed) & 0xFFFFFF for k in range(n)]


def render(engine, w, h, base, aa, poses=None, pose_source="host", paints=None, paint_source="host", device_poses=_same, device_paints=_same,
           out=None, src_stream=None, keep=None):
    """One render_retained call with frame paints.  Sources: "rest" / "none" (NULL), "host", or "device" (through device_*; what they
    return is appended to `keep`, which the caller holds until the frame has finished)."""
    kw = {}
    if poses is not None and pose_source != "rest":
        if pose_source == "host":
            kw["transforms"] = np.ascontiguousarray(poses, dtype=np.float32)
        else:
            d = device_poses(np.ascontiguousarray(poses, dtype=np.float32))
            kw.update(transforms=d, transforms_is_device=isinstance(d, np.ndarray))
            if keep is not None:
                keep.append(d)
    if paints is not None and paint_source != "none":
        pt = paint_list(paints, len(paints))
        if paint_source == "host":
            kw["paints"] = pt
        else:
            d = device_paints(pt)
            kw.update(paints=d, paints_is_device=isinstance(d, np.ndarray))
            if keep is not None:
                keep.append(d)
    return engine.render_retained(w, h, base, aa, out=out, src_stream=src_stream, **kw)


def frame(engine, w, h, base, aa, **kw):
    """A blocking frame: (image, bump); pools that overflow are grown and the frame is rendered again."""
    keep = []
    for _ in range(12):
        render(engine, w, h, base, aa, keep=keep, **kw)
        r = engine.sync()
        if r != -4:
            break
        assert engine.grow_pools(engine.bump()), "E_CAPACITY, but no pool had to grow"
    assert r == 0, f"sync: {r}"
    return engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4).copy(), engine.bump()


def want(lib, inst, poses, q, w, h, base, aa, view=None):
    """The oracle's image of (fragment_i, X_i) under the paints q."""
    shown = rp.posed(inst, poses) if poses is not None else inst
    return rp.want(lib, shown, w, h, base, aa, q, view)


def assert_retained_bytes(engine, lib, inst, retained, name):
    kept, lay = rp.retained_bytes(lib, inst, retained)
    assert np.array_equal(engine.read_buffer("scene", np.uint8, kept.nbytes), kept), f"{name}: VELLO_HIP_BUF_SCENE is not the retained scene"
    cfg = engine.read_buffer("config", np.uint32, 88)
    assert [int(v) for v in cfg[5:15]] == list(lay), f"{name}: VELLO_HIP_BUF_CONFIG does not hold the composed layout"


class RepaintEngine(ip.InstanceEngine):
    """What compare_frame sees as the engine: the list is retained once (with R), every blocking render it asks for -- with the
    COMPOSED bytes, which go to the oracle -- is a retained frame under poses X and frame paints P."""

    def __init__(self, engine, instances, retained, kw):
        super().__init__(engine, instances)
        self._rest, self._retained, self._kw = instances, retained, kw
        self.retains = 0

    def render(self, packed, layout, width, height, base_color, aa, ramps=None):
        e = self._engine
        lay, nbytes = e.instances_layout(self._instances)
        assert lay == layout and nbytes == len(packed), (lay, layout, nbytes, len(packed))
        if not self.retains:
            e.retain_instances(self._rest, paints=self._retained)
            self.retains += 1
        self.frames += 1
        return frame(e, width, height, base_color, aa, **self._kw)


# ---------------------------------------------------------------------------------------------------------------
# 1. Against the oracle
# ---------------------------------------------------------------------------------------------------------------
def check_oracle(engine, name, pose_source, paint_source, device_poses=_same, device_paints=_same):
    """compare_frame, every intermediate, of a list of solid, gradient, image, blur, clip and blend fragments retained with R and
    rendered under turned poses and frame paints P, KEEP and SOLID interleaved; MSAA16 and area AA."""
    from vello_amd import AaConfig

    w, h = 160, 120
    which = ["solid", "linear", "image", "blur", "clip", "blend"]
    lib, inst = rp.scene_list(which, 13, w, h, 31)
    n = len(inst)
    poses = rp.turned(inst, w, h, 31)
    retained = rp.some_paints(n)
    p = frame_paints(n)
    q = effective(retained, p, n)
    assert (q["flags"] == SOLID).sum() > (paint_list(p, n)["flags"] == SOLID).sum() > 0  # (some instances keep their retained paint)
    lib.upload(engine)
    shown = rp.posed(inst, poses)
    packed, _, layout = pp.compose(lib.packed, lib.layout, lib.fragments, shown, q)
    for aa in (AaConfig.Msaa16, AaConfig.Area):
        kw = dict(poses=poses, pose_source=pose_source, paints=p, paint_source=paint_source, device_poses=device_poses, device_paints=device_paints)
        re = RepaintEngine(engine, inst, retained, kw)
        img, ref, _ = parity.compare_frame(re, packed, layout, w, h, BLACK, aa, f"{name}_{int(aa)}", resolved=ip._Late(lib), tol=1 if int(aa) == 0 else 0)
        assert re.frames > 0 and re.retains == 1
        assert_retained_bytes(engine, lib, inst, retained, name)
        assert not np.array_equal(ref, want(lib, inst, poses, retained, w, h, BLACK, aa)), f"{name}: the frame's paints change nothing: the case proves nothing"


# ---------------------------------------------------------------------------------------------------------------
# 2. Against render_instances_painted, bit for bit
# ---------------------------------------------------------------------------------------------------------------
def _hold_bitwise(engine, name, layout, w, h, reference, candidates):
    """`reference()` renders a blocking frame of the reference route (called twice), every `candidates[label]()` one of the route
    under test.  The buffers whose slots atomics hand out (rp._ROWS: waves race for the bump allocators, so their ORDER is not the
    frame's -- two reference frames that happen to agree in one do not make it so) are held to the reference frame in
    parity.compare_frame's canonical forms; the two reference frames may differ in those buffers only.  Every other buffer is equal
    word for word, and every bump counter is the reference's (bump.ptcl where the reference's own two agree: the chunks of a
    restarted command list are not the frame's).  Returns the reference's buffers and bump."""
    refs = []
    for _ in range(2):
        reference()
        refs.append(rp._snapshot(engine, layout, w, h))
    (ref, ref_bump), (ref2, ref2_bump) = refs
    for k, v in ref.items():
        assert k in rp._ROWS or np.array_equal(v, ref2[k]), f"{name}: two frames of the reference route differ in {k}"
    for label, run in candidates.items():
        run()
        got, bump = rp._snapshot(engine, layout, w, h)
        assert set(bump) == set(ref_bump) == set(ref2_bump)
        for k, v in ref_bump.items():
            if k == "ptcl" and ref2_bump[k] != v:
                continue  # (the command words are walked below)
            assert ref2_bump[k] == v, f"{name}: two frames of the reference route differ in bump.{k}: {ref_bump} {ref2_bump}"
            assert bump[k] == v, f"{name}_{label}: bump.{k} {bump[k]} != {v}"
        for k, v in ref.items():
            if k not in rp._ROWS:
                assert np.array_equal(got[k], v), f"{name}_{label}: VELLO_HIP_BUF_{k.upper()} differs from the reference route's frame"
        rp._compare_canonical(f"{name}_{label}", got, ref, bump, ref_bump, layout, w, h)
    return ref, ref_bump


def check_bitwise(engine, name, view=None, cull=False, pose_source="host", paint_source="host", device_poses=_same, device_paints=_same):
    """The frame of (fragment_i, X_i) under Q through render_instances_painted and through retain(R) + render_retained(X, P)."""
    import vello_amd
    from vello_amd import AaConfig

    w, h, aa = 160, 120, AaConfig.Msaa16
    frs = ip.brush_fragments()
    lib = vello_amd.FragmentLibrary([frs["solid"], frs["blur"], frs["clip"], ip.polygon(6), frs["linear"], frs["blend"]])
    lib.upload(engine)
    inst = ip.scatter(np.random.default_rng(23), 23, 6, w, h, scale=(0.8, 2.2))
    n = len(inst)
    poses = rp.turned(inst, w, h, 6)
    retained, p = rp.some_paints(n), frame_paints(n, 1)
    q = effective(retained, p, n)
    shown = rp.posed(inst, poses)
    packed, _, layout = pp.compose(lib.packed, lib.layout, lib.fragments, shown, q)
    keep = []

    def reference():
        engine.render_instances(shown, w, h, BLACK, aa, paints=q)
        assert engine.sync() == 0
        assert np.array_equal(engine.read_buffer("scene", np.uint8, packed.nbytes), packed)

    def candidate():
        engine.retain_instances(inst, paints=retained)
        render(engine, w, h, BLACK, aa, poses, pose_source, p, paint_source, device_poses, device_paints, keep=keep)
        assert engine.sync() == 0

    try:
        if view is not None:
            engine.set_view_transform(view)
        engine.set_viewport_cull(cull)
        ref, _ = _hold_bitwise(engine, name, layout, w, h, reference, {"repaint": candidate})
    finally:
        engine.set_view_transform(None)
        engine.set_viewport_cull(False)
    assert_retained_bytes(engine, lib, inst, retained, name)
    img = ref["output"].view(np.uint8).reshape(h, w, 4)
    assert np.array_equal(img, want(lib, inst, poses, q, w, h, BLACK, aa, view)), f"{name}: image"
    assert not np.array_equal(img, want(lib, inst, poses, retained, w, h, BLACK, aa, view)), f"{name}: the frame's paints changed nothing"


def check_occlusion(engine, name, device_paints=_same):
    """A cover over a dozen polygons: retained translucent and painted opaque this frame, then retained opaque and painted translucent.
    Coarse reads the frame's colours: bump.segments and bump.ptcl -- every buffer -- follow the render_instances_painted frame of the
    frame's colours, and the opaque frame needs fewer segments than the translucent one."""
    import vello_amd
    from vello_amd import AaConfig, Affine, Color, Fill, Rect, Scene

    cover = Scene()
    cover.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(200, 200, 60), None, Rect(-50.0, -40.0, 50.0, 40.0))
    lib = vello_amd.FragmentLibrary([ip.polygon(k, seed=k, r=10.0) for k in (3, 5, 6, 8)] + [cover])
    lib.upload(engine)
    w, h, aa = 160, 128, AaConfig.Msaa16
    rng = np.random.default_rng(17)
    inst = [(i % 4, (1.5, 0.0, 0.0, 1.5, float(rng.uniform(40, 120)), float(rng.uniform(34, 94)))) for i in range(12)]
    inst.append((4, (1.0, 0.0, 0.0, 1.0, 80.0, 64.0)))  # x 30 .. 130, y 24 .. 104: the tiles 2 .. 7 x 2 .. 5 whole
    n = len(inst)
    opaque, translucent = 0xFF203040, 0x80102030
    segments = {}
    keep = []
    for label, r_cover, p_cover, source in (("to_opaque", translucent, opaque, "device"), ("to_translucent", opaque, translucent, "host")):
        retained = [pp.word(i) for i in range(12)] + [r_cover]
        p = [None] * 12 + [p_cover]
        q = effective(retained, p, n)
        _, _, layout = pp.compose(lib.packed, lib.layout, lib.fragments, inst, q)

        def reference():
            engine.render_instances(inst, w, h, WHITE, aa, paints=q)
            assert engine.sync() == 0

        def candidate():
            engine.retain_instances(inst, paints=retained)
            render(engine, w, h, WHITE, aa, None, "rest", p, source, device_paints=device_paints, keep=keep)
            assert engine.sync() == 0

        ref, ref_bump = _hold_bitwise(engine, f"{name}_{label}", layout, w, h, reference, {"repaint": candidate})
        segments[label] = ref_bump["segments"]
        assert np.array_equal(ref["output"].view(np.uint8).reshape(h, w, 4), want(lib, inst, None, q, w, h, WHITE, aa)), f"{name}_{label}: image"
    assert segments["to_opaque"] < segments["to_translucent"], f"{name}: the opaque cover occluded nothing ({segments})"


def check_all_keep(engine, name, device_paints=_same):
    """All-KEEP paints, from host and from device, are the unpainted render_retained frame in every buffer and counter."""
    import vello_amd
    from vello_amd import AaConfig

    w, h, aa = 128, 96, AaConfig.Msaa16
    frs = ip.brush_fragments()
    lib = vello_amd.FragmentLibrary([frs["solid"], frs["blur"], ip.polygon(5), frs["blend"]])
    lib.upload(engine)
    inst = ip.scatter(np.random.default_rng(5), 14, 4, w, h, scale=(0.8, 2.0))
    n = len(inst)
    poses = rp.turned(inst, w, h, 3)
    retained = rp.some_paints(n)
    engine.retain_instances(inst, paints=retained)
    _, _, layout = pp.compose(lib.packed, lib.layout, lib.fragments, rp.posed(inst, poses), paint_list(retained, n))
    from vello_amd import PAINT_DTYPE

    keep_all = np.zeros(n, dtype=PAINT_DTYPE)
    keep_all["rgba"] = 0xFF00FF00  # (KEEP with any rgba changes nothing)
    keep = []

    def run(paints, source):
        def go():
            render(engine, w, h, BLACK, aa, poses, "host", paints, source, device_paints=device_paints, keep=keep)
            assert engine.sync() == 0
        return go

    ref, _ = _hold_bitwise(engine, name, layout, w, h, run(None, "none"), {"keep_host": run(keep_all, "host"), "keep_device": run(keep_all, "device")})
    assert np.array_equal(ref["output"].view(np.uint8).reshape(h, w, 4), want(lib, inst, poses, retained, w, h, BLACK, aa))
    assert_retained_bytes(engine, lib, inst, retained, name)


# ---------------------------------------------------------------------------------------------------------------
# 3. Kernel shapes
# ---------------------------------------------------------------------------------------------------------------
def shape_library():
    """One-word polygons; `multi`: fill colour + linear gradient + blurred rect (11 words: colour words at 0 and 6, none between or
    behind); `blend`: fill, BEGIN_CLIP (blend and alpha words), fill; a gradient-only fragment; an empty fragment."""
    import vello_amd
    from vello_amd import Affine, Color, Fill, Gradient, Rect, Scene

    stops = [(0.0, Color.from_rgb8(255, 40, 40)), (1.0, Color.from_rgb8(40, 40, 255))]
    multi = Scene()
    multi.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(60, 200, 90), None, Rect(-6.0, -5.0, 0.0, 0.0))
    multi.fill(Fill.NonZero, Affine.IDENTITY, Gradient.new_linear((-6.0, 0.0), (6.0, 0.0)).with_stops(stops), None, Rect(0.0, -5.0, 6.0, 0.0))
    multi.draw_blurred_rounded_rect(Affine.IDENTITY, (-5.0, 1.0, 5.0, 6.0), Color.from_rgb8(250, 180, 60), 1.5, 1.0)
    frs = ip.brush_fragments()
    lib = vello_amd.FragmentLibrary([ip.polygon(3, r=4.0), ip.polygon(5, r=4.0), multi, frs["blend"], frs["linear"]])
    lib.multi, lib.blend, lib.gradient = 2, 3, 4
    lib.empty = len(lib.fragments)
    lib.fragments.append(dict(ip.EMPTY))
    assert [f["draw_data"][1] - f["draw_data"][0] for f in lib.fragments] == [1, 1, 11, 4, 5, 0]
    mask = pp.colour_mask(lib.packed, lib.layout, lib.fragments[lib.multi])
    assert [int(i) for i in np.nonzero(mask)[0]] == [0, 6]
    tags = [int(t) for t in lib.packed.view(np.uint32)[lib.layout.draw_tag_base + lib.fragments[lib.blend]["draws"][0]:][:3]]
    assert tags == [pp.FILL_COLOR, pp.BEGIN_CLIP, pp.FILL_COLOR]
    return lib


def _dd_words(lib, inst):
    return sum(lib.fragments[f]["draw_data"][1] - lib.fragments[f]["draw_data"][0] for f, _ in inst)


def shape_cases(lib):
    """name -> instances: the smallest lists at which a lane per draw-data word, 256 to a workgroup, can go wrong."""
    rng = np.random.default_rng(3)

    def place(frags):
        return [(f, t) for f, (_, t) in zip(frags, ip.scatter(rng, len(frags), 1, 128, 96, scale=(0.6, 1.6)))]

    cases = {"dd0": place([lib.empty] * 5), "dd1": place([0])}
    for n in (255, 256, 257):
        cases[f"dd{n}"] = place([k % 2 for k in range(n)])
    # several colour words an instance with other words between them, layers, and empty fragments in between (owners skip instances)
    cases["multi_and_empties"] = place([lib.multi, lib.empty, lib.empty, 0, lib.empty, lib.blend, lib.multi, lib.empty, lib.gradient, 1] * 6 + [lib.empty])
    # 23 x 11 + 3 = 256 words: the next instance's first word is lane 0 of the second workgroup
    cases["owner_on_boundary"] = place([lib.multi] * 23 + [0, lib.empty, 1, 0, lib.multi, lib.blend, 1])
    assert _dd_words(lib, cases["owner_on_boundary"][:27]) == 256 and cases["owner_on_boundary"][27][0] == lib.multi
    # more instances than draw-data words: with device paints the lanes that test the paints run beyond the words
    cases["more_instances_than_words"] = place([lib.empty] * 150 + [0] + [lib.empty] * 149 + [lib.multi] + [lib.empty] * 99)
    assert _dd_words(lib, cases["more_instances_than_words"]) == 12 < len(cases["more_instances_than_words"]) == 400
    # SOLID paints on empty and gradient-only instances alone
    cases["nothing_to_paint"] = place([lib.empty, lib.gradient, lib.empty, lib.gradient])
    return cases


def check_shapes(engine, name, device_poses=_same, device_paints=_same):
    """Every shape under host paints, device paints and NULL: the image is the oracle's, exactly (MSAA8), and VELLO_HIP_BUF_SCENE
    shows the retained bytes each time.  Every instance is painted SOLID but every fifth."""
    from vello_amd import AaConfig

    lib = shape_library()
    lib.upload(engine)
    w, h, aa = 128, 96, AaConfig.Msaa8
    for label, inst in shape_cases(lib).items():
        n = len(inst)
        retained = [None if k % 3 else 0xFF000000 | (0x40 + k % 150) << 8 for k in range(n)]
        p = [None if k % 5 == 4 else 0xFF000000 | (0x30 + (7 * k) % 200) << 16 | 0x55 for k in range(n)]
        if label == "nothing_to_paint":
            p = [0xFF112233] * n
        q = effective(retained, p, n)
        engine.retain_instances(inst, paints=retained)
        kept, _ = rp.retained_bytes(lib, inst, retained)
        w_q, w_r = want(lib, inst, None, q, w, h, WHITE, aa), want(lib, inst, None, retained, w, h, WHITE, aa)
        if _dd_words(lib, inst) and label != "nothing_to_paint":
            assert not np.array_equal(w_q, w_r), f"{name}_{label}: the paints change nothing: the case proves nothing"
        else:
            assert np.array_equal(w_q, w_r)
        for source in ("host", "device", "none", "device"):
            img, _ = frame(engine, w, h, WHITE, aa, paints=p, paint_source=source, device_paints=device_paints)
            assert np.array_equal(img, w_r if source == "none" else w_q), f"{name}_{label}: image under {source} paints"
            assert np.array_equal(engine.read_buffer("scene", np.uint8, kept.nbytes), kept), f"{name}_{label}: retained bytes under {source} paints"
    # the words themselves, of the case that has every kind: a painted frame's stages run again from its colour words
    inst = shape_cases(lib)["multi_and_empties"]
    poses = rp.turned(inst, w, h, 2)
    n = len(inst)
    p = [0xFF000000 | (k + 1) for k in range(n)]
    engine.retain_instances(inst)
    q = effective(None, p, n)
    shown = rp.posed(inst, poses)
    packed, plain, layout = pp.compose(lib.packed, lib.layout, lib.fragments, shown, q)
    dd, dd0 = (x.view(np.uint32)[layout.draw_data_base: layout.transform_base] for x in (packed, plain))
    changed = np.nonzero(dd != dd0)[0]
    assert len(changed) == sum({lib.multi: 2, lib.blend: 2, 0: 1, 1: 1}.get(f, 0) for f, _ in inst)  # (no float, no blend / alpha word)
    kw = dict(poses=poses, pose_source="device", paints=p, paint_source="device", device_poses=device_poses, device_paints=device_paints)
    re = RepaintEngine(engine, inst, None, kw)
    parity.compare_frame(re, packed, layout, w, h, WHITE, aa, f"{name}_words", resolved=ip._Late(lib))


# ---------------------------------------------------------------------------------------------------------------
# 4. Life cycle
# ---------------------------------------------------------------------------------------------------------------
def _raw(engine, transforms, t_dev, paints, p_dev, src_stream, w, h, base, aa, target=None, stride=None):
    p = engine._params(w, h, base, aa)
    return engine._lib.vello_hip_render_retained_painted(engine._h, rp._ptr(transforms), int(t_dev), rp._ptr(paints), int(p_dev),
                                                         ctypes.c_void_p(src_stream) if src_stream else None, ctypes.byref(p), rp._ptr(target),
                                                         w * 4 if stride is None else stride)


def check_life_cycle(engine, name, make_target, to_numpy, device_poses=_same, device_paints=_same):
    import vello_amd
    import workloads
    from oracle.oracle import Oracle
    from vello_amd import AaConfig

    w, h, aa = 160, 120, AaConfig.Msaa16
    frs = ip.brush_fragments()
    lib = vello_amd.FragmentLibrary([frs["solid"], frs["linear"], frs["blur"], ip.polygon(6), frs["blend"]])
    lib.upload(engine)
    rng = np.random.default_rng(21)
    inst = ip.scatter(rng, 19, 5, w, h, scale=(0.8, 2.5))
    n = len(inst)
    retained = rp.some_paints(n)
    poses = [rp.turned(inst, w, h, k) for k in range(4)]
    sets = [frame_paints(n, k) for k in range(4)]
    qs = [effective(retained, p, n) for p in sets]
    wants = [want(lib, inst, poses[k], qs[k], w, h, BLACK, aa) for k in range(4)]
    want_unpainted = want(lib, inst, poses[1], retained, w, h, BLACK, aa)
    other_list = ip.scatter(rng, 7, 5, w, h, scale=(0.8, 2.5))
    want_other_list = rp.want(lib, other_list, w, h, BLACK, aa)
    want_lib = rp.want(lib, [(k, rp.IDENT) for k in range(5)], w, h, BLACK, aa)
    other, other_layout = workloads.random_test_scene(5, n_paths=60, size=128.0, strokes=True, clips=True).resolve()
    other = np.ascontiguousarray(other, dtype=np.uint8)
    o = Oracle()
    o.set_scene(other, other_layout, w, h, BLACK, int(aa))
    want_scene = o.render().copy()
    assert len({x.tobytes() for x in wants + [want_unpainted, want_other_list, want_lib, want_scene]}) == 8
    engine.retain_instances(inst, paints=retained)
    kept, _ = rp.retained_bytes(lib, inst, retained)
    keep = []
    src = ("host", "device")
    dev = dict(device_poses=device_poses, device_paints=device_paints, keep=keep)
    try:
        engine.set_frames_in_flight(4)
        # four frames in flight: four paint sets and four pose sets into four targets, sources alternating
        for rnd in range(2):
            t = [make_target(w, h) for _ in range(4)]
            for k in range(4):
                j = (k + rnd) % 4
                render(engine, w, h, BLACK, aa, poses[j], src[k % 2], sets[j], src[(k + rnd + 1) % 2], out=t[k], **dev)
            assert engine.sync() == 0
            for k in range(4):
                assert np.array_equal(to_numpy(t[k]), wants[(k + rnd) % 4]), f"{name}: round {rnd}, frame {k} does not show its own paints and poses"
        # a painted, an unpainted and a painted frame on the same lane (four lanes: every fourth frame)
        t = [make_target(w, h) for _ in range(9)]
        for k in range(9):
            if k == 4:
                rp.render_retained(engine, w, h, BLACK, aa, poses[1], "host", out=t[k])
            else:
                render(engine, w, h, BLACK, aa, poses[k % 4], "host", sets[k % 4], src[k % 2], out=t[k], **dev)
        assert engine.sync() == 0
        for k in range(9):
            assert np.array_equal(to_numpy(t[k]), want_unpainted if k == 4 else wants[k % 4]), f"{name}: painted / unpainted / painted, frame {k}"
        # between render_resident, render_frame and render_instances frames on the rotating lanes
        t = [make_target(w, h) for _ in range(8)]
        render(engine, w, h, BLACK, aa, poses[0], "device", sets[0], "device", out=t[0], **dev)
        view_parity.render_resident_into(engine, w, h, BLACK, aa, t[1])
        render(engine, w, h, BLACK, aa, poses[1], "host", sets[1], "host", out=t[2], **dev)
        view_parity.render_frame_into(engine, other, other_layout, w, h, BLACK, aa, t[3])
        render(engine, w, h, BLACK, aa, poses[2], "host", sets[2], "device", out=t[4], **dev)
        ip.render_instances_into(engine, other_list, w, h, BLACK, aa, t[5])
        render(engine, w, h, BLACK, aa, poses[3], "device", sets[3], "host", out=t[6], **dev)
        rp.render_retained(engine, w, h, BLACK, aa, poses[1], "host", out=t[7])
        assert engine.sync() == 0
        for k, wnt in enumerate((wants[0], want_lib, wants[1], want_scene, wants[2], want_other_list, wants[3], want_unpainted)):
            assert np.array_equal(to_numpy(t[k]), wnt), f"{name}: interleaved frame {k}"
        # no scene allocation across 20 painted frames, whatever the lanes held before
        for k in range(4):
            render(engine, w, h, BLACK, aa, poses[k], "host", sets[k], "host", out=t[k], **dev)
        assert engine.sync() == 0
        before = engine.scene_allocations()
        for k in range(20):
            render(engine, w, h, BLACK, aa, poses[k % 4], src[k % 2], sets[k % 4], src[(k // 2) % 2], out=t[k % 4], **dev)
        assert engine.sync() == 0
        assert engine.scene_allocations() == before, f"{name}: {engine.scene_allocations() - before} scene buffers allocated by painted retained frames"
        for k in range(4):
            assert np.array_equal(to_numpy(t[k]), wants[k]), f"{name}: steady-state frame {k}"
    finally:
        engine.set_frames_in_flight(1)
    # run_stages after a painted frame: on the frame's colour words and transform words, neither source read again
    img, _ = frame(engine, w, h, BLACK, aa, poses=poses[2], pose_source="device", paints=sets[2], paint_source="device", device_poses=device_poses,
                   device_paints=device_paints)
    assert np.array_equal(img, wants[2])
    for front_last, first in (("pathtag_scan", "flatten"), ("flatten", "draw_scan"), (None, "pathtag_scan")):
        engine.write_buffer("output", np.zeros(w * h * 4, dtype=np.uint8))
        if front_last:
            engine.run_stages(w, h, BLACK, aa, "pathtag_scan", front_last)
        engine.run_stages(w, h, BLACK, aa, first, "fine")
        assert engine.bump()["failed"] == 0
        assert np.array_equal(engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4), wants[2]), f"{name}: run_stages from {first} after a painted frame"
    # ... and after an unpainted frame on the same lane: the retained colours
    img, _ = rp.frame(engine, w, h, BLACK, aa, poses[1], "host")
    assert np.array_equal(img, want_unpainted)
    engine.write_buffer("output", np.zeros(w * h * 4, dtype=np.uint8))
    engine.run_stages(w, h, BLACK, aa, "pathtag_scan", "flatten")
    engine.run_stages(w, h, BLACK, aa, "draw_scan", "fine")
    assert np.array_equal(engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4), want_unpainted), f"{name}: run_stages after an unpainted frame"
    # retained bytes and library bytes unchanged
    assert np.array_equal(engine.read_buffer("scene", np.uint8, kept.nbytes), kept), f"{name}: the retained bytes changed"
    engine.render_resident(w, h, BLACK, aa)
    assert engine.sync() == 0
    assert np.array_equal(engine.read_buffer("scene", np.uint8, lib.packed.nbytes), lib.packed), f"{name}: the library's bytes changed"
    # retain again: the list and its table are replaced, paints apply to the new list
    engine.retain_instances(other_list)
    p2 = frame_paints(len(other_list), 2)
    x2 = rp.turned(other_list, w, h, 9)
    for source in ("host", "device"):
        img, _ = frame(engine, w, h, BLACK, aa, poses=x2, paints=p2, paint_source=source, device_paints=device_paints)
        assert np.array_equal(img, want(lib, other_list, x2, effective(None, p2, len(other_list)), w, h, BLACK, aa)), f"{name}: paints on the second list ({source})"
    # a paint list of the wrong length
    try:
        engine.render_retained(w, h, BLACK, aa, paints=[None] * (len(other_list) + 1))
        raise AssertionError(f"{name}: a paint list of the wrong length was accepted")
    except ValueError:
        pass
    # uploads drop the list; release, then a painted frame, is VELLO_HIP_E_INVALID
    pt = paint_list(sets[0], n)
    for drop in (lambda: engine.upload_scene(lib.packed, lib.layout, lib.ramps), lambda: lib.upload(engine), engine.release_retained):
        lib.upload(engine)
        engine.retain_instances(inst)
        frame(engine, w, h, BLACK, aa, poses=poses[0], paints=sets[0])
        drop()
        assert _raw(engine, None, 0, pt, 0, None, w, h, BLACK, aa) == -1, f"{name}: a painted frame of a dropped list was accepted"
    engine.release_retained()
    lib.upload(engine)
    engine.render_resident(w, h, BLACK, aa)
    assert engine.sync() == 0


def check_source_stream_emu(engine, name):
    """Device paints and poses with a src_stream, overwritten right after the call: the frame shows the first contents (the emulator
    runs a launch when it is enqueued; the GPU twin has a torch op on another stream write them)."""
    import vello_amd
    from vello_amd import AaConfig

    w, h, aa = 96, 64, AaConfig.Msaa8
    lib = vello_amd.FragmentLibrary([ip.polygon(5), ip.polygon(8)])
    lib.upload(engine)
    inst = ip.scatter(np.random.default_rng(2), 6, 2, w, h, scale=(0.8, 2.0))
    n = len(inst)
    x1, x2 = rp.turned(inst, w, h, 1), rp.turned(inst, w, h, 2)
    p1, p2 = paint_list(frame_paints(n, 0), n), paint_list(frame_paints(n, 1), n)
    engine.retain_instances(inst)
    dx, dp = x1.copy(), p1.copy()
    engine.render_retained(w, h, BLACK, aa, transforms=dx, transforms_is_device=True, paints=dp, paints_is_device=True, src_stream=engine.stream() or 1)
    dx[...] = x2
    dp[...] = p2
    assert engine.sync() == 0
    got = engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4)
    assert np.array_equal(got, want(lib, inst, x1, p1, w, h, BLACK, aa)), name
    # src_stream with device paints alone (host poses)
    engine.render_retained(w, h, BLACK, aa, transforms=x2, paints=p2.copy(), paints_is_device=True, src_stream=engine.stream() or 1)
    assert engine.sync() == 0
    got = engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4)
    assert np.array_equal(got, want(lib, inst, x2, p2, w, h, BLACK, aa)), name


# ---------------------------------------------------------------------------------------------------------------
# 6. Refusals and the rotation
# ---------------------------------------------------------------------------------------------------------------
def check_errors(engine, name, make_target, to_numpy, device_poses=_same, device_paints=_same, host_memory=None):
    """Every VELLO_HIP_E_INVALID of the painted entry point.  Four lanes and rp.check_errors' scheme: accepted frame k must take lane k
    -- VELLO_HIP_BUF_OUTPUT, the internal target of the lane that rendered last, then shows what a first round left in lane k's -- so
    a refusal that moved the rotation shows; every target holds its own frame, a refused frame has written none."""
    import vello_amd
    from vello_amd import AaConfig, PAINT_DTYPE

    w, h, aa = 96, 64, AaConfig.Msaa8
    frs = ip.brush_fragments()
    lib = vello_amd.FragmentLibrary([frs["solid"], frs["blur"], ip.polygon(4)])
    lib.upload(engine)
    good = [(0, (1.0, 0.0, 0.0, 1.0, 30.0, 30.0)), (1, (1.5, 0.0, 0.0, 1.5, 60.0, 30.0)), (2, (1.0, 0.0, 0.0, 1.0, 20.0, 44.0))]
    n = len(good)
    poses = rp.turned(good, w, h, 2)
    ok = paint_list([0xFF102030, None, 0xFF405060], n)
    engine.retain_instances(good)
    xs = [rp.turned(good, w, h, 10 + k) for k in range(4)]
    ps = [[0xFF000000 | (0x101010 * (k + 2)), None if k % 2 else 0xC0102030, 0xFF00FF00 >> k | 0xFF000000] for k in range(4)]
    wants = [want(lib, good, xs[k], effective(None, ps[k], n), w, h, BLACK, aa) for k in range(4)]
    assert len({x.tobytes() for x in wants}) == 4
    t0 = make_target(w, h)
    assert engine._lib.vello_hip_render_retained_painted(None, None, 0, None, 0, None, None, None, 0) == -1
    keep = []
    try:
        engine.set_frames_in_flight(4)
        # round A leaves lane i's INTERNAL target holding image 3 - i; the frames of round B have targets of their own and leave it alone
        for k in range(4):
            render(engine, w, h, BLACK, aa, xs[3 - k], "host", ps[3 - k], "host")
        assert engine.sync() == 0

        def lane_shown():
            return engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4)

        def last_error():
            return engine._lib.vello_hip_last_error(engine._h)

        t = [make_target(w, h) for _ in range(5)]
        for k in range(4):
            render(engine, w, h, BLACK, aa, xs[k], ("host", "device")[k % 2], ps[k], ("device", "host")[k % 2], device_poses, device_paints, out=t[k], keep=keep)
            assert np.array_equal(lane_shown(), wants[3 - k]), f"{name}: frame {k} did not take lane {k}: the lane rotation moved on a refused frame"
            shown = engine.read_buffer("scene", np.uint8, 64)
            # host flags other than 0 or 1, naming the instance
            for j, flags in enumerate((2, 7, 0xFFFFFFFF)):
                bad = ok.copy()
                bad["flags"][(k + j) % 3] = flags
                assert _raw(engine, poses, 0, bad, 0, None, w, h, BLACK, aa, t[k]) == -1
                assert f"instance {(k + j) % 3}".encode() in last_error(), last_error()
            # src_stream with only host or NULL sources
            s = engine.stream() or 1
            assert _raw(engine, poses, 0, ok, 0, s, w, h, BLACK, aa, t[k]) == -1
            assert _raw(engine, None, 0, ok, 0, s, w, h, BLACK, aa, t[k]) == -1
            assert _raw(engine, poses, 0, None, 0, s, w, h, BLACK, aa, t[k]) == -1
            assert _raw(engine, None, 0, None, 0, s, w, h, BLACK, aa, t[k]) == -1
            # a misaligned device pointer; host memory handed in as device memory (GPU builds)
            d = device_paints(ok)
            keep.append(d)
            assert _raw(engine, poses, 0, rp._ptr(d) + 2, 1, None, w, h, BLACK, aa, t[k]) == -1
            assert b"multiple of 4" in last_error(), last_error()
            if host_memory is not None:
                for kind, mem in host_memory(ok).items():
                    assert _raw(engine, poses, 0, mem, 1, None, w, h, BLACK, aa, t[k]) == -1, f"{name}: {kind} host memory accepted as device paints"
                    assert b"not device memory" in last_error(), f"{name}: {kind}"
            # a refusal of vello_hip_render_retained, with good paints: a NaN pose, a bad target, bad parameters
            v = poses.copy()
            v[k % 3, k] = float("nan")
            assert _raw(engine, v, 0, ok, 0, None, w, h, BLACK, aa, t[k]) == -1
            assert _raw(engine, poses, 0, ok, 0, None, w, h, BLACK, aa, t[k], stride=w * 4 - 4) == -1
            assert _raw(engine, poses, 0, ok, 0, None, 0, h, BLACK, aa, t[k]) == -1
            assert _raw(engine, poses, 0, ok, 0, None, w, h, BLACK, 5, t[k]) == -1
            assert engine._lib.vello_hip_render_retained_painted(None, None, 0, None, 0, None, None, None, 0) == -1
            assert np.array_equal(engine.read_buffer("scene", np.uint8, 64), shown), f"{name}: a refused call changed what VELLO_HIP_BUF_SCENE shows"
            assert np.array_equal(lane_shown(), wants[3 - k]), f"{name}: a refused call moved the rotation's last lane"
        render(engine, w, h, BLACK, aa, xs[0], "host", ps[0], "host", out=t[4])
        assert np.array_equal(lane_shown(), wants[3]), f"{name}: the last refusals moved the rotation"
        assert engine.sync() == 0
        for k in range(4):
            assert np.array_equal(to_numpy(t[k]), wants[k]), f"{name}: frame {k} (a refused frame wrote its target?)"
        assert np.array_equal(to_numpy(t[4]), wants[0])
    finally:
        engine.set_frames_in_flight(1)
    # no list at all (paints on a library without masks: check_no_masks)
    engine.release_retained()
    assert _raw(engine, None, 0, ok, 0, None, w, h, BLACK, aa, t0) == -1
    assert b"retain" in engine._lib.vello_hip_last_error(engine._h)
    lib.upload(engine)


def no_mask_library(k=65536):
    """A hand-packed library whose fragment table's draw-data ranges add up to 2^32 words, so that the engine keeps no colour masks for
    it: k radial-gradient draw objects (seven draw-data words each, the most a draw tag has) on empty paths -- tags TRANSFORM,
    STYLE, PATH x k -- taken whole by as many overlapping fragments as it takes, and one last fragment of its first draw object alone.
    Returns (bytes, Layout, fragments, index of the small fragment)."""
    from vello_amd import Layout

    radial = 0x29C  # DRAWTAG_FILL_RAD_GRADIENT: 7 draw-data words, 10 info words
    assert (radial >> 2) & 7 == 7 and (radial >> 6) & 0xF == 10
    n_tags = k + 2
    tag_bytes = (n_tags + 1023) // 1024 * 1024
    tags = np.zeros(tag_bytes, dtype=np.uint8)
    tags[0], tags[1], tags[2:n_tags] = 0x20, 0x40, 0x10
    dd = np.zeros((k, 7), dtype=np.float32)
    dd[:, 6] = 10.0  # (index 0, p0 = p1 = (0, 0), r0 = 0, r1 = 10)
    xf = np.array([1.0, 0.0, 0.0, 1.0, 0.0, 0.0], dtype=np.float32)
    style = np.zeros(2, dtype=np.uint32)  # a non-zero fill
    words = np.concatenate([tags.view(np.uint32), np.full(k, radial, dtype=np.uint32), dd.reshape(-1).view(np.uint32), xf.view(np.uint32), style])
    t = tag_bytes // 4
    layout = Layout(k, k, 0, 10 * k, 0, t, t, t + k, t + 8 * k, t + 8 * k + 6)
    whole = dict(path_tags=(0, n_tags), path_data=(0, 0), draws=(0, k), draw_data=(0, 7 * k), transforms=(0, 1), styles=(0, 1))
    small = dict(path_tags=(0, 3), path_data=(0, 0), draws=(0, 1), draw_data=(0, 7), transforms=(0, 1), styles=(0, 1))
    n_whole = (2 ** 32 + 7 * k - 1) // (7 * k)
    return np.ascontiguousarray(words).view(np.uint8), layout, [whole] * n_whole + [small], n_whole


def check_no_masks(engine, name, make_target, to_numpy):
    """Paints on a library that keeps no masks: the list is retained and its unpainted frames are served; a paint list -- host, or
    handed in as device memory -- is VELLO_HIP_E_INVALID, with nothing enqueued and the rotation where it was."""
    from vello_amd import AaConfig

    w, h, aa = 64, 48, AaConfig.Msaa8
    packed, layout, frags, small = no_mask_library()
    assert sum(f["draw_data"][1] - f["draw_data"][0] for f in frags) >= 2 ** 32
    engine.upload_fragments(packed, layout, frags)
    inst = [(small, (1.0, 0.0, 0.0, 1.0, 20.0 + 9.0 * i, 20.0)) for i in range(3)]
    engine.retain_instances(inst)
    bases = [0xFF000000 | (0x40 * (k + 1)) for k in range(4)]
    ok = paint_list([0xFF102030, None, 0xFF405060], 3)
    try:
        engine.set_frames_in_flight(4)
        for k in range(4):  # lane k's internal target: the base colour of frame 3 - k (the gradients' paths are empty)
            engine.render_retained(w, h, bases[3 - k], aa)
        assert engine.sync() == 0
        t = [make_target(w, h) for _ in range(4)]
        for k in range(4):
            engine.render_retained(w, h, bases[k], aa, out=t[k])
            shown = engine.read_buffer("output", np.uint32, w * h)
            assert (shown == bases[3 - k]).all(), f"{name}: frame {k} did not take lane {k}"
            for is_device in (0, 1):
                assert _raw(engine, None, 0, ok, is_device, None, w, h, BLACK, aa, t[k]) == -1, f"{name}: a paint list was accepted"
                assert b"takes no paints" in engine._lib.vello_hip_last_error(engine._h), engine._lib.vello_hip_last_error(engine._h)
            assert (engine.read_buffer("output", np.uint32, w * h) == bases[3 - k]).all(), f"{name}: a refused call moved the rotation"
        assert engine.sync() == 0
        for k in range(4):
            assert (to_numpy(t[k]).reshape(-1, 4).view(np.uint32) == bases[k]).all(), f"{name}: frame {k} (a refused frame wrote its target?)"
    finally:
        engine.set_frames_in_flight(1)
    # the retained form refuses paints as well, as before
    assert rp._raw_retain(engine, inst, ok) == -1
    engine.release_retained()


def check_device_flags(engine, name, make_target, to_numpy, device_paints=_same):
    """A device paint with flags 7 on a 64x48 target with a 3-instance list: VELLO_HIP_E_INVALID at sync, the target's bytes unchanged,
    the next frame with good paints correct -- an ordinary discarded frame."""
    import vello_amd
    from vello_amd import AaConfig

    w, h, aa = 64, 48, AaConfig.Msaa8
    lib = vello_amd.FragmentLibrary([ip.polygon(5), ip.polygon(7), ip.brush_fragments()["solid"]])
    lib.upload(engine)
    inst = [(0, (1.0, 0.0, 0.0, 1.0, 16.0, 16.0)), (1, (1.2, 0.0, 0.0, 1.2, 40.0, 20.0)), (2, (1.0, 0.0, 0.0, 1.0, 30.0, 34.0))]
    n = len(inst)
    poses = rp.turned(inst, w, h, 4)
    good = paint_list([0xFF102030, 0xFF908070, None], n)
    engine.retain_instances(inst)
    for which in range(n):
        t = make_target(w, h)
        if isinstance(t, np.ndarray):
            t[...] = 0x5A
        else:
            t.fill_(0x5A)
        before = to_numpy(t).copy()  # (a copy to the host: the fill has finished)
        assert (before == 0x5A).all()
        bad = good.copy()
        bad["flags"][which] = 7
        keep = []
        render(engine, w, h, BLACK, aa, poses, "host", bad, "device", device_paints=device_paints, out=t, keep=keep)
        assert engine.sync() == -1, f"{name}: device paint flags of 7 on instance {which} were not found"
        assert np.array_equal(to_numpy(t), before), f"{name}: the discarded frame wrote its target"
        render(engine, w, h, BLACK, aa, poses, "host", good, "device", device_paints=device_paints, out=t, keep=keep)
        assert engine.sync() == 0
        assert np.array_equal(to_numpy(t), want(lib, inst, poses, good, w, h, BLACK, aa)), f"{name}: the frame after a discarded one"


# ---------------------------------------------------------------------------------------------------------------
# 7. Pool overflow
# ---------------------------------------------------------------------------------------------------------------
def check_overflow(make_engine, name, device_poses=_same, device_paints=_same):
    """Pool overflow from tiny pools under a painted device frame: E_CAPACITY at sync, grow_pools, then the frame."""
    import vello_amd
    from vello_amd import AaConfig

    w, h, aa = 128, 96, AaConfig.Msaa8
    engine = make_engine(dict(lines=64, seg_counts=64, segments=64, tiles=256))
    lib = vello_amd.FragmentLibrary([ip.polygon(9), ip.polygon(14)])
    lib.upload(engine)
    inst = ip.scatter(np.random.default_rng(4), 30, 2, w, h, scale=(1.0, 2.5))
    n = len(inst)
    poses = rp.turned(inst, w, h, 3)
    p = frame_paints(n, 3)
    engine.retain_instances(inst)
    keep = []
    kw = dict(poses=poses, pose_source="device", paints=p, paint_source="device", device_poses=device_poses, device_paints=device_paints, keep=keep)
    render(engine, w, h, BLACK, aa, **kw)
    assert engine.sync() == -4, f"{name}: the tiny pools did not overflow"
    rounds = 0
    while True:
        assert engine.grow_pools(engine.bump()), f"{name}: E_CAPACITY, but no pool had to grow"
        rounds += 1
        render(engine, w, h, BLACK, aa, **kw)
        r = engine.sync()
        if r != -4:
            break
        assert rounds < 12
    assert r == 0
    img = engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4)
    assert np.array_equal(img, want(lib, inst, poses, effective(None, p, n), w, h, BLACK, aa)), f"{name}: the frame after grow_pools"
