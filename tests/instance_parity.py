"""Scene instances (vello_hip_upload_fragments / vello_hip_render_instances) against the CPU oracle.  The oracle knows nothing of
fragments: it is handed the COMPOSED scene, put together here in numpy from the library's packed bytes, the fragments' ranges and the
rules of include/vello_hip.h (not through Scene.append, so that the expectation does not depend on the library under test), while the
engine is handed the library and the instance list.  tests.parity.compare_frame does the comparing through InstanceEngine, an adapter
that swaps the scene on the engine's side only: every intermediate is held to the tolerances the suite already uses."""
import math

import numpy as np

from oracle.oracle import Oracle
from tests import parity

BLACK, WHITE = 0xFF000000, 0xFFFFFFFF
f32 = np.float32
STREAMS = ("path_tags", "path_data", "draws", "draw_data", "transforms", "styles")
EMPTY = {k: (0, 0) for k in STREAMS}


def _floats(t):
    return np.array([float(v) for v in (t.c if hasattr(t, "c") else t)], dtype=np.float32)


def compose(packed, layout, fragments, instances):
    """(bytes, Layout) of the scene that `instances` -- (fragment index, transform) pairs -- compose from the library: per stream the
    concatenation of the fragments' ranges, the tags zero-padded to a multiple of 1024, every transform entry T of instance i
    replaced by V_i.T (f32, every product and every sum rounded on its own), the layout from the running sums and the draw tags."""
    from vello_amd import Layout

    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    words = packed.view(np.uint32)
    L = layout
    src = {"path_tags": packed[L.path_tag_base * 4: L.path_data_base * 4], "path_data": words[L.path_data_base: L.draw_tag_base],
           "draws": words[L.draw_tag_base: L.draw_data_base], "draw_data": words[L.draw_data_base: L.transform_base],
           "transforms": words[L.transform_base: L.style_base].view(np.float32).reshape(-1, 6), "styles": words[L.style_base:].reshape(-1, 2)}
    parts = {k: [] for k in STREAMS}
    for fi, t in instances:
        fr = fragments[int(fi)]
        for k in STREAMS:
            b, e = fr[k]
            piece = src[k][b:e]
            if k == "transforms" and e > b:
                v = _floats(t)
                tt = piece
                with np.errstate(all="ignore"):
                    c = np.empty_like(tt)
                    c[:, 0] = f32(v[0] * tt[:, 0]) + f32(v[2] * tt[:, 1])
                    c[:, 1] = f32(v[1] * tt[:, 0]) + f32(v[3] * tt[:, 1])
                    c[:, 2] = f32(v[0] * tt[:, 2]) + f32(v[2] * tt[:, 3])
                    c[:, 3] = f32(v[1] * tt[:, 2]) + f32(v[3] * tt[:, 3])
                    c[:, 4] = (f32(v[0] * tt[:, 4]) + f32(v[2] * tt[:, 5])) + v[4]
                    c[:, 5] = (f32(v[1] * tt[:, 4]) + f32(v[3] * tt[:, 5])) + v[5]
                assert c.dtype == np.float32
                piece = c
            parts[k].append(piece)

    def cat(k, dtype):
        return np.concatenate([np.ascontiguousarray(p).reshape(-1).view(dtype) for p in parts[k]]) if parts[k] else np.zeros(0, dtype=dtype)

    tags = cat("path_tags", np.uint8)
    tags = np.concatenate([tags, np.zeros(-len(tags) % 1024, dtype=np.uint8)])
    pd, dt, dd = cat("path_data", np.uint32), cat("draws", np.uint32), cat("draw_data", np.uint32)
    xf, st = cat("transforms", np.uint32), cat("styles", np.uint32)
    out = np.concatenate([tags.view(np.uint32), pd, dt, dd, xf, st]).view(np.uint8)
    b1 = len(tags) // 4
    b2, b3 = b1 + len(pd), b1 + len(pd) + len(dt)
    b4 = b3 + len(dd)
    lay = Layout(n_draw_objects=len(dt), n_paths=len(dt), n_clips=int((dt & 1).sum()), bin_data_start=int(((dt >> 6) & 0xF).sum()),
                 path_tag_base=0, path_data_base=b1, draw_tag_base=b2, draw_data_base=b3, transform_base=b4, style_base=b4 + len(xf))
    assert out.nbytes == 4 * (lay.style_base + len(st))
    return out, lay


class InstanceEngine:
    """What compare_frame sees as the engine: every blocking render it asks for -- with the COMPOSED bytes, which go to the oracle --
    is a frame of the instance list on the resident library; pools that overflow are grown and the frame is rendered again, as
    Engine.render's callers do with auto-grow.  Everything else is the engine's own."""

    def __init__(self, engine, instances):
        from vello_amd.renderer import instance_array

        self._engine, self._instances = engine, instance_array(instances)
        self.frames = 0

    def __getattr__(self, name):
        return getattr(self._engine, name)

    def render(self, packed, layout, width, height, base_color, aa, ramps=None):
        e = self._engine
        lay, nbytes = e.instances_layout(self._instances)
        assert lay == layout and nbytes == len(packed), (lay, layout, nbytes, len(packed))
        for _ in range(12):
            self.frames += 1
            e.render_instances(self._instances, width, height, base_color, aa)
            r = e.sync()
            if r != -4:
                break
            assert e.grow_pools(e.bump()), "E_CAPACITY, but no pool had to grow"
        assert r == 0, f"sync: {r}"
        return e.read_buffer("output", np.uint8, width * height * 4).reshape(height, width, 4).copy(), e.bump()


def library_image(lib, width, height, base_color, aa):
    o = Oracle(capacity_scale=4, auto_grow=True)
    o.set_scene(lib.packed, lib.layout, width, height, base_color, int(aa))
    o.set_ramps(lib.ramps)
    o.set_image_atlas(lib.resolved.atlas_image())
    return o.render()


def compare_instance_frame(engine, lib, instances, width, height, base_color, aa, name, differs=True, upload=True, **kw):
    """compare_frame of `instances` of the library `lib` (a FragmentLibrary) against the oracle on the numpy-composed scene; asserts
    that the composed image is not the library's own, so that an engine that ignores the instances fails."""
    if upload:
        lib.upload(engine)
    packed, layout = compose(lib.packed, lib.layout, lib.fragments, instances)
    ie = InstanceEngine(engine, instances)
    img, ref, bump = parity.compare_frame(ie, packed, layout, width, height, base_color, aa, name, resolved=_Late(lib), **kw)
    assert ie.frames > 0
    got = engine.read_buffer("scene", np.uint8, packed.nbytes)
    assert np.array_equal(got, packed), f"{name}: VELLO_HIP_BUF_SCENE is not the composed scene"
    if differs:
        assert not np.array_equal(library_image(lib, width, height, base_color, aa), ref), f"{name}: the instances show what the library shows: the case proves nothing"
    return img, ref, bump


class _Late:
    """The late-bound resources compare_frame hands the oracle: the library's.  The atlas is already in the engine (FragmentLibrary.upload);
    atlas_size 0 keeps compare_frame from resizing -- and so clearing -- it."""

    def __init__(self, lib):
        self.ramps, self.atlas_size, self.uploads = lib.ramps, 0, []
        self._image = lib.resolved.atlas_image()

    def atlas_image(self):
        return self._image


# ---------------------------------------------------------------------------------------------------------------
# Fragments
# ---------------------------------------------------------------------------------------------------------------
def polygon(k, seed=0, r=10.0):
    """A Scene of one filled polygon of k vertices about the origin: TRANSFORM, STYLE, k LINETO tags (the closing one included), PATH."""
    from vello_amd import Affine, BezPath, Color, Fill, Scene

    rng = np.random.default_rng(1000 + 31 * k + seed)
    s = Scene()
    p = BezPath()
    a = np.sort(rng.uniform(0, 2 * np.pi, k)) if k > 2 else np.array([0.0, 2.0, 4.0])[:max(k, 2)]
    rr = r * rng.uniform(0.6, 1.0, len(a))
    p.move_to((float(rr[0] * np.cos(a[0])), float(rr[0] * np.sin(a[0]))))
    for t, q in zip(a[1:], rr[1:]):
        p.line_to((float(q * np.cos(t)), float(q * np.sin(t))))
    p.close_path()
    s.fill(Fill.NonZero, Affine.IDENTITY, Color(float(rng.uniform(0.2, 1)), float(rng.uniform(0.2, 1)), float(rng.uniform(0.2, 1)), 1.0), None, p)
    return s


def tag_shape_library():
    """Polygons of 3 .. 18 vertices -- tag ranges of every length mod 4 at every source offset mod 4 (asserted) -- plus, as sub-ranges
    of the first polygon, two one-tag fragments (its TRANSFORM marker with its transform entry, its STYLE marker with its style) and
    an empty fragment."""
    import vello_amd

    # a polygon of k vertices is k + 3 tags: vertex counts picked so that the running offset meets every residue with every length
    ks, off, need = [], 0, {(r, o) for r in range(4) for o in range(4)}
    while need:
        r = next((r for r in range(4) if (r, off % 4) in need), 1)
        k = 3 + (r - 6) % 4 + 4 * (len(ks) % 3)
        ks.append(k)
        need.discard(((k + 3) % 4, off % 4))
        off += k + 3
    lib = vello_amd.FragmentLibrary([polygon(k, seed=i) for i, k in enumerate(ks)])
    seen = {((f["path_tags"][1] - f["path_tags"][0]) % 4, f["path_tags"][0] % 4) for f in lib.fragments}
    assert len(seen) == 16, sorted(seen)
    f0 = lib.fragments[0]
    t0, x0, s0 = f0["path_tags"][0], f0["transforms"][0], f0["styles"][0]
    assert lib.packed[lib.layout.path_tag_base * 4 + t0] == 0x20 and lib.packed[lib.layout.path_tag_base * 4 + t0 + 1] == 0x40
    lib.one_transform = len(lib.fragments)
    lib.fragments.append(dict(EMPTY, path_tags=(t0, t0 + 1), transforms=(x0, x0 + 1)))
    lib.one_style = len(lib.fragments)
    lib.fragments.append(dict(EMPTY, path_tags=(t0 + 1, t0 + 2), styles=(s0, s0 + 1)))
    lib.empty = len(lib.fragments)
    lib.fragments.append(dict(EMPTY))
    lib.n_polygons = len(ks)
    return lib


def scatter(rng, n, n_frags, w, h, scale=(0.5, 2.0)):
    """n instances of fragments drawn about the origin, placed over a w x h target under rotation and uniform scale."""
    out = []
    for _ in range(n):
        a, s = rng.uniform(0, 2 * math.pi), rng.uniform(*scale)
        out.append((int(rng.integers(0, n_frags)), (s * math.cos(a), s * math.sin(a), -s * math.sin(a), s * math.cos(a), rng.uniform(0, w), rng.uniform(0, h))))
    return out


def check_bytes(engine, name, lib, instances, w=64, h=48, upload=True):
    """VELLO_HIP_BUF_SCENE equals the numpy bytes exactly and instances_layout the numpy layout; the frame itself is the oracle's."""
    from vello_amd import AaConfig

    if upload:
        lib.upload(engine)
    packed, layout = compose(lib.packed, lib.layout, lib.fragments, instances)
    lay, nbytes = engine.instances_layout(instances)
    assert lay == layout and nbytes == packed.nbytes, f"{name}: {lay} {nbytes} != {layout} {packed.nbytes}"
    engine.render_instances(instances, w, h, BLACK, AaConfig.Msaa8)
    assert engine.sync() == 0, name
    got = engine.read_buffer("scene", np.uint8, packed.nbytes + 64)
    assert np.array_equal(got[:packed.nbytes], packed), f"{name}: composed bytes differ first at byte {np.nonzero(got[:packed.nbytes] != packed)[0][:1]}"
    assert not got[packed.nbytes:].any(), f"{name}: the 64 bytes of slack are not zero"
    cfg = engine.read_buffer("config", np.uint32, 88)
    assert [int(v) for v in cfg[5:15]] == list(layout), f"{name}: VELLO_HIP_BUF_CONFIG does not hold the composed layout"
    o = Oracle(capacity_scale=4, auto_grow=True)
    o.set_scene(packed, layout, w, h, BLACK, int(AaConfig.Msaa8))
    assert np.array_equal(engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4), o.render()), f"{name}: image"
    return packed, layout


def check_tag_shapes(engine, name):
    """Every tag length mod 4 at every source AND destination offset mod 4, one-tag fragments, an empty fragment, n = 0, one instance,
    totals on and one past a multiple of 1024."""
    lib = tag_shape_library()
    lib.upload(engine)
    rng = np.random.default_rng(7)
    P = lib.n_polygons
    tags_of = [f["path_tags"][1] - f["path_tags"][0] for f in lib.fragments]
    ident = (1.0, 0.0, 0.0, 1.0, 20.0, 20.0)
    check_bytes(engine, name + "_n0", lib, [], upload=False)
    check_bytes(engine, name + "_one", lib, [(5, ident)], upload=False)
    assert P > 5
    check_bytes(engine, name + "_only_empty", lib, [(lib.empty, ident)] * 3, upload=False)
    # every polygon after 0 .. 3 one-tag fragments: every destination offset mod 4 for every (length, source offset)
    inst = []
    for shift in range(4):
        for k in range(P):
            inst += [(lib.one_transform if (j + k) % 2 else lib.one_style, ident) for j in range(shift)]
            inst += [(lib.empty, ident), (k, scatter(rng, 1, 1, 64, 48)[0][1])]
    check_bytes(engine, name + "_all_offsets", lib, inst, upload=False)
    # straddling words made of one-tag fragments only, between two polygons
    check_bytes(engine, name + "_one_tag_runs", lib, [(0, ident)] + [(lib.one_transform, ident), (lib.one_style, ident)] * 9 + [(lib.empty, ident), (3, ident)], upload=False)
    # more instances in one chunk than the kernel stages offsets for: 3 000 empty ones between two polygons
    check_bytes(engine, name + "_empties", lib, [(0, ident)] + [(lib.empty, ident)] * 3000 + [(3, ident), (lib.one_style, ident)], upload=False)
    # a tag total of exactly 1024 and of 1025
    base = [(int(rng.integers(0, P)), scatter(rng, 1, 1, 64, 48)[0][1]) for _ in range(60)]
    while sum(tags_of[f] for f, _ in base) > 1024:
        base.pop()
    pad = 1024 - sum(tags_of[f] for f, _ in base)
    for extra, label in ((0, "1024"), (1, "1025")):
        inst = base + [(lib.one_style, ident)] * (pad + extra)
        packed, layout = check_bytes(engine, f"{name}_tags_{label}", lib, inst, upload=False)
        assert layout.path_data_base * 4 == (1024 if extra == 0 else 2048)
    # the library itself is untouched, and render_resident still shows it whole
    engine.render_resident(64, 48, BLACK, 1)
    assert engine.sync() == 0
    assert np.array_equal(engine.read_buffer("scene", np.uint8, lib.packed.nbytes), lib.packed), f"{name}: the library's bytes changed"


def check_many(engine, name, n_same=1000, n_tiny=20000):
    """A fragment used 1 000 times; 20 000 tiny instances (triangles and quads)."""
    import vello_amd

    lib = vello_amd.FragmentLibrary([polygon(k, r=4.0) for k in (3, 4, 5, 7)])
    lib.upload(engine)
    rng = np.random.default_rng(11)
    check_bytes(engine, f"{name}_same_{n_same}", lib, [(2, t) for _, t in scatter(rng, n_same, 1, 128, 96)], 128, 96, upload=False)
    check_bytes(engine, f"{name}_tiny_{n_tiny}", lib, scatter(rng, n_tiny, 2, 128, 96, scale=(0.3, 1.0)), 128, 96, upload=False)


def check_one_tag_chunks(engine, name, n=12000):
    """Whole chunks of the tag stream made of one-tag fragments: four instances per destination word, so the chunk's slice of the
    prefix is four times what the kernel stages and its threads search the table itself, with no empty instance involved."""
    lib = tag_shape_library()
    ident = (1.0, 0.0, 0.0, 1.0, 20.0, 20.0)
    inst = [(0, ident)] + [(lib.one_transform if j % 3 else lib.one_style, ident) for j in range(n)] + [(3, ident)]
    check_bytes(engine, f"{name}_{n}", lib, inst)


def check_long_chunks(engine, name, steps):
    """Composed scenes long enough that a workgroup's chunk is `steps` x 256 words (the kernel walks on from its previous word's
    instance): polygons of 4 000 and 20 003 vertices, shrunk so that the frame costs little, until the scene passes
    (steps - 1) x 2 048 x 256 words; the instances are spread so that chunks of every stream hold several."""
    import vello_amd

    lib = vello_amd.FragmentLibrary([polygon(4000), polygon(20003), polygon(5)])
    rng = np.random.default_rng(steps)
    inst, tags, rest = [], 0, 0
    while (tags + 1023) // 1024 * 256 + rest <= (steps - 1) * 2048 * 256:
        f = int(rng.integers(0, 3)) if len(inst) % 8 else 1
        inst.append((f, (0.05, 0.0, 0.0, 0.05, float(rng.uniform(4, 60)), float(rng.uniform(4, 44)))))
        fr = lib.fragments[f]
        tags += fr["path_tags"][1] - fr["path_tags"][0]
        rest += _composed_words(fr, 1) - (fr["path_tags"][1] - fr["path_tags"][0] + 1023) // 1024 * 256
    packed, layout = check_bytes(engine, f"{name}_{steps}", lib, inst)
    assert (steps - 1) * 2048 * 256 < packed.nbytes // 4 <= steps * 2048 * 256, packed.nbytes


def brush_fragments():
    """Fragments about the origin, one per brush kind and layer kind: solid, linear / radial / sweep gradient, image, blurred rounded
    rect, a clip layer around a gradient fill, a blend layer."""
    from vello_amd import (Affine, BlendMode, Circle, Color, Compose, Fill, Gradient, ImageData, Mix, Rect, RoundedRect, Scene, Stroke)

    out = {}
    s = Scene()
    s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(220, 40, 40), None, Rect(-12.0, -8.0, 12.0, 8.0))
    s.stroke(Stroke(2.5), Affine.IDENTITY, Color.from_rgb8(250, 250, 90), None, Circle((0.0, 0.0), 11.0))
    out["solid"] = s
    stops = [(0.0, Color.from_rgb8(255, 0, 0)), (0.5, Color.from_rgb8(0, 255, 0)), (1.0, Color.from_rgb8(0, 0, 255))]
    for kind, g in (("linear", Gradient.new_linear((-14.0, 0.0), (14.0, 0.0))), ("radial", Gradient.new_radial((0.0, 0.0), 14.0)),
                    ("sweep", Gradient.new_sweep((0.0, 0.0), 0.0, 2.0 * math.pi))):
        s = Scene()
        s.fill(Fill.NonZero, Affine.IDENTITY, g.with_stops(stops), None, RoundedRect(-14.0, -10.0, 14.0, 10.0, 4.0))
        out[kind] = s
    rng = np.random.default_rng(3)
    px = rng.integers(0, 256, (12, 16, 4), dtype=np.uint8)
    px[..., 3] = 255
    s = Scene()
    s.draw_image(ImageData(px), Affine.translate(-8.0, -6.0))
    out["image"] = s
    s = Scene()
    s.draw_blurred_rounded_rect(Affine.IDENTITY, (-12.0, -9.0, 12.0, 9.0), Color.from_rgb8(90, 200, 250), 3.0, 2.0)
    out["blur"] = s
    s = Scene()
    s.push_clip_layer(Fill.NonZero, Affine.IDENTITY, Circle((0.0, 0.0), 10.0))
    s.fill(Fill.NonZero, Affine.IDENTITY, Gradient.new_linear((0.0, -12.0), (0.0, 12.0)).with_stops(stops[::-1]), None, Rect(-14.0, -14.0, 14.0, 14.0))
    s.pop_layer()
    out["clip"] = s
    s = Scene()
    s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(40, 90, 220), None, Rect(-12.0, -12.0, 6.0, 6.0))
    s.push_layer(Fill.NonZero, BlendMode(Mix.Multiply, Compose.SrcOver), 0.8, Affine.IDENTITY, Rect(-8.0, -8.0, 12.0, 12.0))
    s.fill(Fill.EvenOdd, Affine.IDENTITY, Color.from_rgb8(250, 160, 40), None, Circle((2.0, 2.0), 9.0))
    s.pop_layer()
    out["blend"] = s
    return out


def check_host_agreement(engine, name):
    """With the same Resolver, the composed bytes are what Scene.append(fragment, transform) per instance + resolve give."""
    import vello_amd
    from vello_amd import Affine, Scene

    frs = brush_fragments()
    keys = ["solid", "linear", "image", "clip", "radial", "blend"]
    resolver = vello_amd.Resolver()
    lib = vello_amd.FragmentLibrary([frs[k] for k in keys], resolver=resolver)
    lib.upload(engine)
    rng = np.random.default_rng(5)
    affs = [Affine.translate(float(rng.uniform(20, 140)), float(rng.uniform(20, 100))) * Affine.rotate(float(rng.uniform(0, 6.0))) * Affine.scale(float(rng.uniform(0.6, 2.0)))
            for _ in range(11)]
    picks = [int(rng.integers(0, len(keys))) for _ in affs]
    host = Scene()
    for k, a in zip(picks, affs):
        host.append(frs[keys[k]], a)
    hr = resolver.resolve(host)
    instances = list(zip(picks, affs))
    packed, layout = compose(lib.packed, lib.layout, lib.fragments, instances)
    assert layout == hr.layout, f"{name}: {layout} != {hr.layout}"
    assert np.array_equal(packed, hr.packed), f"{name}: the numpy composition is not Scene.append + resolve"
    from vello_amd import AaConfig

    engine.render_instances(instances, 160, 120, BLACK, AaConfig.Msaa16)
    assert engine.sync() == 0
    assert np.array_equal(engine.read_buffer("scene", np.uint8, packed.nbytes), hr.packed), f"{name}: the engine's composition is not Scene.append + resolve"


def _scene_fragments(which):
    """Whole test scenes as fragments (drawn for a 256-ish canvas)."""
    import workloads
    from tests import cull_parity

    mk = {"polygons": lambda: cull_parity.polygon_scene(n=60, size=128.0), "polylines": lambda: cull_parity.polyline_scene(n=50, size=128.0),
          "cardioid": workloads.cardioid_scene, "funky": workloads.funky_paths_scene, "stroke_styles": workloads.stroke_styles_scene,
          "clip_blend": lambda: workloads.clip_blend_scene(size=128.0), "circle": workloads.circle_scene}
    r = mk[which]()
    return r[0] if isinstance(r, tuple) else r


def check_frame(engine, name, which, flags=None, aas=None, w=256, h=200, base=BLACK, n=7, in_flight=1, back_half=True):
    """Full compare_frame of instances of `which` fragments (names of _scene_fragments / brush_fragments) under affines."""
    import vello_amd
    from vello_amd import AaConfig, Affine

    brushes = brush_fragments()
    lib = vello_amd.FragmentLibrary([brushes[k] if k in brushes else _scene_fragments(k) for k in which])
    rng = np.random.default_rng(len(name))
    inst = []
    for k in range(n):
        f = k % len(which)
        small = which[f] in brushes
        sc = rng.uniform(1.0, 3.0) if small else rng.uniform(0.25, 0.7)
        a = Affine.translate(float(rng.uniform(0.1, 0.7) * w), float(rng.uniform(0.1, 0.7) * h)) * Affine.rotate(float(rng.uniform(-0.6, 0.6))) * Affine.scale(float(sc))
        inst.append((f, a))
    try:
        if flags:
            engine.set_debug_flags(**flags)
        if in_flight != 1:
            engine.set_frames_in_flight(in_flight)
        for aa in aas or (AaConfig.Msaa16, AaConfig.Area):
            compare_instance_frame(engine, lib, inst, w, h, base, aa, f"{name}_{int(aa)}", tol=1 if int(aa) == 0 else 0, back_half=back_half)
    finally:
        if in_flight != 1:
            engine.set_frames_in_flight(1)
        if flags:
            engine.set_debug_flags()


def check_front_fusion(engine, name):
    """A composed scene small enough for the fused front: the launches are taken, and NO_FUSION gives the same buffers."""
    import vello_amd
    from vello_amd import AaConfig, Affine

    lib = vello_amd.FragmentLibrary([polygon(5), polygon(8), brush_fragments()["solid"]])
    inst = [(k % 3, Affine.translate(30.0 + 25.0 * k, 30.0 + 11.0 * k) * Affine.rotate(0.4 * k) * Affine.scale(1.0 + 0.3 * k)) for k in range(6)]
    try:
        engine.set_debug_flags(flatten_coop=True)
        before = engine.fused_launches()
        compare_instance_frame(engine, lib, inst, 200, 150, WHITE, AaConfig.Msaa16, name + "_fused")
        assert engine.fused_launches() > before, f"{name}: the fused path was not taken"
        engine.set_debug_flags(flatten_coop=True, no_fusion=True)
        before = engine.fused_launches()
        compare_instance_frame(engine, lib, inst, 200, 150, WHITE, AaConfig.Area, name + "_nofusion", tol=1)
        assert engine.fused_launches() == before
    finally:
        engine.set_debug_flags()


# ---------------------------------------------------------------------------------------------------------------
# Life cycle
# ---------------------------------------------------------------------------------------------------------------
def _target_ptr(t):
    return t.ctypes.data if isinstance(t, np.ndarray) else t.data_ptr()


def render_instances_into(engine, instances, w, h, base_color, aa, target):
    """vello_hip_render_instances into `target`: a torch tensor on the GPU, or -- the emulated build only, where device memory is host
    memory -- a numpy array (Engine.render_instances refuses those for the real library's sake)."""
    import ctypes

    from vello_amd.renderer import instance_array

    inst = instance_array(instances)
    p = engine._params(w, h, base_color, aa)
    engine._check(engine._lib.vello_hip_render_instances(engine._h, inst.ctypes.data, len(inst), ctypes.byref(p), _target_ptr(target), w * 4), "render_instances")


def _want(lib, instances, w, h, base, aa, view=None):
    from tests import view_parity

    packed, layout = compose(lib.packed, lib.layout, lib.fragments, instances)
    if view is not None:
        packed = view_parity.compose(packed, layout, view)
    o = Oracle(capacity_scale=4, auto_grow=True)
    o.set_scene(packed, layout, w, h, base, int(aa))
    o.set_ramps(lib.ramps)
    o.set_image_atlas(lib.resolved.atlas_image())
    return o.render().copy()


def check_life_cycle(engine, name, make_target, to_numpy):
    """Four frames in flight with four instance lists into four targets; instance frames interleaved with render_resident and
    render_frame; lists that grow and shrink without re-allocation after the largest; a view on top; culling on; the library's
    bytes unchanged afterwards."""
    import workloads
    import vello_amd
    from tests import view_parity
    from vello_amd import AaConfig, Affine

    w, h, aa = 160, 120, AaConfig.Msaa16
    frs = brush_fragments()
    lib = vello_amd.FragmentLibrary([frs["solid"], frs["linear"], frs["clip"], polygon(6), frs["blend"]])
    lib.upload(engine)
    rng = np.random.default_rng(21)
    lists = [scatter(rng, n, 5, w, h, scale=(0.8, 2.5)) for n in (9, 40, 3, 17)]
    want = [_want(lib, li, w, h, BLACK, aa) for li in lists]
    want_lib = _want(lib, [(k, (1, 0, 0, 1, 0, 0)) for k in range(5)], w, h, BLACK, aa)
    other, other_layout = workloads.random_test_scene(5, n_paths=60, size=128.0, strokes=True, clips=True).resolve()
    other = np.ascontiguousarray(other, dtype=np.uint8)
    o = Oracle()
    o.set_scene(other, other_layout, w, h, BLACK, int(aa))
    want_other = o.render().copy()
    assert len({x.tobytes() for x in want + [want_lib, want_other]}) == 6
    try:
        engine.set_frames_in_flight(4)
        for rnd in range(2):
            t = [make_target(w, h) for _ in range(4)]
            for k in range(4):
                render_instances_into(engine, lists[(k + rnd) % 4], w, h, BLACK, aa, t[k])
            assert engine.sync() == 0
            for k in range(4):
                assert np.array_equal(to_numpy(t[k]), want[(k + rnd) % 4]), f"{name}: round {rnd}, frame {k} does not show its own instances"
        # interleaved with render_resident (the library whole) and render_frame (a scene of its own) on the rotating lanes
        t = [make_target(w, h) for _ in range(7)]
        render_instances_into(engine, lists[0], w, h, BLACK, aa, t[0])
        view_parity.render_resident_into(engine, w, h, BLACK, aa, t[1])
        render_instances_into(engine, lists[1], w, h, BLACK, aa, t[2])
        view_parity.render_frame_into(engine, other, other_layout, w, h, BLACK, aa, t[3])
        render_instances_into(engine, lists[2], w, h, BLACK, aa, t[4])
        view_parity.render_resident_into(engine, w, h, BLACK, aa, t[5])
        render_instances_into(engine, lists[3], w, h, BLACK, aa, t[6])
        assert engine.sync() == 0
        for k, wnt in enumerate((want[0], want_lib, want[1], want_other, want[2], want_lib, want[3])):
            assert np.array_equal(to_numpy(t[k]), wnt), f"{name}: interleaved frame {k}"
        # every lane has held the largest list: growing and shrinking lists allocate nothing
        for _ in range(4):
            render_instances_into(engine, lists[1], w, h, BLACK, aa, t[0])
        assert engine.sync() == 0
        before = engine.scene_allocations()
        for k in range(12):
            render_instances_into(engine, lists[k % 4], w, h, BLACK, aa, t[k % 4])
        assert engine.sync() == 0
        assert engine.scene_allocations() == before, f"{name}: {engine.scene_allocations() - before} scene buffers re-allocated in the steady state"
        for k in range(4):
            assert np.array_equal(to_numpy(t[k]), want[k]), f"{name}: steady-state frame {k}"
    finally:
        engine.set_frames_in_flight(1)
    # a view on top, culling on
    view = Affine.translate(0.3 * w, -0.1 * h) * Affine.rotate(0.3) * Affine.scale(1.4)
    tv = make_target(w, h)
    try:
        engine.set_view_transform(view)
        engine.set_viewport_cull(True)
        render_instances_into(engine, lists[1], w, h, BLACK, aa, tv)
        assert engine.sync() == 0
        b_cull = engine.bump()
    finally:
        engine.set_view_transform(None)
        engine.set_viewport_cull(False)
    wv = _want(lib, lists[1], w, h, BLACK, aa, view=view)
    assert not np.array_equal(wv, want[1])
    assert np.array_equal(to_numpy(tv), wv), f"{name}: instances under a view with culling"
    try:
        engine.set_view_transform(view)
        render_instances_into(engine, lists[1], w, h, BLACK, aa, tv)
        assert engine.sync() == 0
        b_all = engine.bump()
    finally:
        engine.set_view_transform(None)
    assert np.array_equal(to_numpy(tv), wv), f"{name}: instances under a view"
    assert b_cull["lines"] < b_all["lines"], f"{name}: culling dropped no line ({b_cull['lines']} / {b_all['lines']})"
    # run_stages acts on the composed scene of the last frame
    engine.run_stages(w, h, BLACK, aa, "pathtag_scan", "fine")
    assert np.array_equal(engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4), want[1]), f"{name}: run_stages after an instance frame"
    view_parity.render_resident_into(engine, w, h, BLACK, aa, tv)
    assert engine.sync() == 0
    assert np.array_equal(to_numpy(tv), want_lib)
    assert np.array_equal(engine.read_buffer("scene", np.uint8, lib.packed.nbytes), lib.packed), f"{name}: the library's bytes changed"


def check_errors(engine, name, make_target, to_numpy):
    """Every VELLO_HIP_E_INVALID of the three entry points, with nothing enqueued and the lane rotation unmoved; upload_scene drops the
    table."""
    import ctypes

    import vello_amd
    from vello_amd import AaConfig
    from vello_amd._lib import FragmentStruct, LayoutStruct
    from vello_amd.renderer import INSTANCE_DTYPE, instance_array

    w, h, aa = 96, 64, AaConfig.Msaa8
    frs = brush_fragments()
    from vello_amd import Affine, Circle, Color, Fill, Rect, Scene

    two_fills = Scene()  # BEGIN_CLIP, a fill, a fill with its own TRANSFORM and STYLE markers, END_CLIP
    two_fills.push_clip_layer(Fill.NonZero, Affine.IDENTITY, Circle((0.0, 0.0), 10.0))
    two_fills.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(255, 0, 0), None, Rect(-8.0, -8.0, 2.0, 2.0))
    two_fills.fill(Fill.EvenOdd, Affine.translate(1.0, 1.0), Color.from_rgb8(0, 255, 0), None, Rect(-2.0, -2.0, 8.0, 8.0))
    two_fills.pop_layer()
    lib = vello_amd.FragmentLibrary([frs["solid"], frs["clip"], polygon(4), two_fills, polygon(20000)])
    # ... and the whole library as one fragment of some 45 000 words: 2^32 words are some 95 000 instances of it (a 2.7 MB list)
    whole = len(lib.fragments)
    lib.fragments.append({k: (0, lib.fragments[-1][k][1]) for k in STREAMS})
    ident = (1.0, 0.0, 0.0, 1.0, 30.0, 30.0)
    good = [(0, ident), (1, (1.5, 0.0, 0.0, 1.5, 60.0, 30.0)), (2, ident)]
    # no table yet
    engine.upload_scene(lib.packed, lib.layout, lib.ramps)
    with np.testing.assert_raises(vello_amd.VelloHipError):
        engine.render_instances(good, w, h, BLACK, aa)
    with np.testing.assert_raises(vello_amd.VelloHipError):
        engine.instances_layout(good)
    lib.upload(engine)
    # Four lanes whose private scene slots have never been used, four lists of falling size: every accepted frame must take the next
    # lane and so allocate its slot; a refusal that moved the rotation would send a later frame to a lane whose slot already fits
    refusals = [[[(len(lib.fragments), ident)], [(0, ident), (0xFFFFFFFF, ident)]], [], []]
    for k in range(6):
        for j, bad in enumerate((float("nan"), float("inf"), float("-inf"))):
            v = list(ident)
            v[k] = bad
            refusals[1 + (k + j) % 2].append(good + [(1, tuple(v))])
    lists = [good * 4, good * 3, good * 2, good]
    # a composed scene of 2^32 words: the shortest list of `whole` that reaches them is refused by both entry points; one instance
    # fewer is a scene instances_layout still describes (host only: nothing is allocated for it)
    n_over = _first_n(lambda n: _composed_words(lib.fragments[whole], n) >= 1 << 32)
    too_long = np.zeros(n_over, dtype=INSTANCE_DTYPE)
    too_long["fragment"], too_long["transform"] = whole, ident
    assert n_over * 28 < 8 << 20
    lay, nbytes = engine.instances_layout(too_long[:-1])
    assert nbytes == 4 * _composed_words(lib.fragments[whole], n_over - 1) and nbytes > (1 << 34) - (1 << 19), nbytes
    assert lay.n_draw_objects == (n_over - 1) * lib.layout.n_draw_objects and lay.n_clips == (n_over - 1) * lib.layout.n_clips
    refusals[0].append(too_long)
    refusals[2].append(too_long)
    try:
        engine.set_frames_in_flight(4)
        t = [make_target(w, h) for _ in range(4)]
        p = engine._params(w, h, BLACK, aa)
        for k in range(4):
            before = engine.scene_allocations()
            render_instances_into(engine, lists[k], w, h, BLACK, aa, t[k])
            assert engine.scene_allocations() == before + 1, f"{name}: frame {k} did not take lane {k}: the lane rotation moved on a refused frame"
            shown = engine.read_buffer("scene", np.uint8, 64)
            for bl in refusals[k] if k < 3 else []:
                inst = instance_array(bl)
                r = engine._lib.vello_hip_render_instances(engine._h, inst.ctypes.data, len(inst), ctypes.byref(p), _target_ptr(t[k]), w * 4)
                assert r == -1, (bl[-1], r)
                assert engine._lib.vello_hip_instances_layout(engine._h, inst.ctypes.data, len(inst), None, None) == -1
                assert engine.scene_allocations() == before + 1, f"{name}: a refused frame allocated a scene buffer"
            if k == 2:
                assert engine._lib.vello_hip_render_instances(engine._h, None, 2, ctypes.byref(p), _target_ptr(t[k]), w * 4) == -1
                assert engine._lib.vello_hip_render_instances(None, None, 0, ctypes.byref(p), None, 0) == -1
            assert np.array_equal(engine.read_buffer("scene", np.uint8, 64), shown), f"{name}: a refused frame changed what VELLO_HIP_BUF_SCENE shows"
        assert engine.sync() == 0
        for k in range(4):
            assert np.array_equal(to_numpy(t[k]), _want(lib, lists[k], w, h, BLACK, aa)), f"{name}: frame {k} (a refused frame wrote its target?)"
    finally:
        engine.set_frames_in_flight(1)
    _check_count_overflow(engine, name, make_target(w, h), p, w)
    # fragments that upload_fragments refuses: nothing stays resident
    L = lib.layout
    f0, f1 = lib.fragments[0], lib.fragments[3]
    assert f1["draws"][1] - f1["draws"][0] == 4

    def upload(frags):
        arr = (FragmentStruct * len(frags))()
        for i, f in enumerate(frags):
            for k in STREAMS:
                getattr(arr[i], k)[:] = f[k]
        lay = LayoutStruct(*L)
        rp = lib.ramps.ctypes.data if lib.ramps is not None else None
        nr = lib.ramps.size // 512 if lib.ramps is not None else 0
        return engine._lib.vello_hip_upload_fragments(engine._h, lib.packed.ctypes.data, lib.packed.nbytes, ctypes.byref(lay), rp, nr, arr, len(frags))

    n_tags = (L.path_data_base - L.path_tag_base) * 4
    b, e = f1["draws"]
    bad_frags = {
        "range not ordered": dict(f0, path_data=(f0["path_data"][1], f0["path_data"][0])) if f0["path_data"][1] else None,
        "tags past the stream": dict(f0, path_tags=(f0["path_tags"][0], n_tags + 1)),
        "styles past the stream": dict(f0, styles=(f0["styles"][0], (len(lib.packed) // 4 - L.style_base) // 2 + 1)),
        "draws shorter than PATH markers": dict(f0, draws=(f0["draws"][0], f0["draws"][1] - 1)),
        "transforms longer than TRANSFORM markers": dict(f0, transforms=(f0["transforms"][0], f0["transforms"][1] + 1)),
        "styles shorter than STYLE markers": dict(f0, styles=(f0["styles"][0], f0["styles"][1] - 1)),
        "draw data shorter than the draw tags ask for": dict(f0, draw_data=(f0["draw_data"][0], f0["draw_data"][1] - 1)),
        "a clip left open": _cut_at_path(lib, f1, b, b + 2),
        "an END_CLIP without its BEGIN_CLIP": _cut_at_path(lib, f1, b + 2, e),
        "no TRANSFORM / STYLE first": dict(f0, path_tags=(f0["path_tags"][0] + 2, f0["path_tags"][1]), transforms=(f0["transforms"][0] + 1, f0["transforms"][1]),
                                            styles=(f0["styles"][0] + 1, f0["styles"][1])),
    }
    for why, fr in bad_frags.items():
        if fr is None:
            continue
        lib.upload(engine)
        assert upload([f0, fr]) == -1, f"{name}: accepted a fragment with {why}"
        assert engine._lib.vello_hip_last_error(engine._h), why
        with np.testing.assert_raises(vello_amd.VelloHipError):
            engine.render_instances(good[:1], w, h, BLACK, aa)
        with np.testing.assert_raises(vello_amd.VelloHipError):
            engine.render_resident(w, h, BLACK, aa)
    # upload_scene drops the table; the scene stays
    lib.upload(engine)
    engine.render_instances(good, w, h, BLACK, aa)
    assert engine.sync() == 0
    engine.upload_scene(lib.packed, lib.layout, lib.ramps)
    with np.testing.assert_raises(vello_amd.VelloHipError):
        engine.render_instances(good, w, h, BLACK, aa)
    engine.render_resident(w, h, BLACK, aa)
    assert engine.sync() == 0


def _composed_words(fr, n):
    """Words of the scene that n instances of the fragment `fr` compose."""
    per = {k: fr[k][1] - fr[k][0] for k in STREAMS}
    return (n * per["path_tags"] + 1023) // 1024 * 256 + n * (per["path_data"] + per["draws"] + per["draw_data"] + 6 * per["transforms"] + 2 * per["styles"])


def _first_n(pred):
    """The smallest n >= 1 for which the monotonic `pred` holds."""
    lo, hi = 0, 1
    while not pred(hi):
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if pred(mid) else (mid, hi)
    return hi


def _check_count_overflow(engine, name, target, p, w):
    """A count that leaves u32 in a composed scene of fewer than 2^32 words.  Only the info-word sum can: a draw tag asks for up to 15
    info words, while a clip tag or a draw object is at least a word of the scene itself.  No Scene gets there (a drawn image brings
    more path data than info words), so the library is written out by hand: one fragment of a TRANSFORM marker, a STYLE marker and
    1 000 PATH markers -- 1 000 empty paths -- each drawn as an image (draw tag 0x28c: 3 words of draw data, 10 info words).  It passes
    every check of upload_fragments and is never rendered: both lists that reach 2^32 info words are refused."""
    import ctypes

    from vello_amd import Layout
    from vello_amd.renderer import INSTANCE_DTYPE

    k = 1000
    tags = np.zeros(1024, dtype=np.uint8)
    tags[0], tags[1], tags[2:2 + k] = 0x20, 0x40, 0x10
    draw_tags = np.full(k, 0x28C, dtype=np.uint32)
    xf = np.array([1, 0, 0, 1, 0, 0], dtype=np.float32).view(np.uint32)
    packed = np.concatenate([tags.view(np.uint32), draw_tags, np.zeros(3 * k, dtype=np.uint32), xf, np.zeros(2, dtype=np.uint32)]).view(np.uint8)
    layout = Layout(n_draw_objects=k, n_paths=k, n_clips=0, bin_data_start=10 * k, path_tag_base=0, path_data_base=256, draw_tag_base=256,
                    draw_data_base=256 + k, transform_base=256 + 4 * k, style_base=256 + 4 * k + 6)
    fr = {"path_tags": (0, 2 + k), "path_data": (0, 0), "draws": (0, k), "draw_data": (0, 3 * k), "transforms": (0, 1), "styles": (0, 1)}
    engine.upload_fragments(packed, layout, [fr])
    shown = engine.read_buffer("scene", np.uint8, 64)
    n_over = _first_n(lambda n: n * 10 * k >= 1 << 32)
    assert _composed_words(fr, n_over) < 1 << 31
    inst = np.zeros(n_over, dtype=INSTANCE_DTYPE)
    inst["transform"] = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)
    lay, nbytes = engine.instances_layout(inst[:-1])
    assert lay.bin_data_start == (n_over - 1) * 10 * k and nbytes == 4 * _composed_words(fr, n_over - 1)
    before = engine.scene_allocations()
    assert engine._lib.vello_hip_instances_layout(engine._h, inst.ctypes.data, len(inst), None, None) == -1, f"{name}: 2^32 info words"
    assert engine._lib.vello_hip_render_instances(engine._h, inst.ctypes.data, len(inst), ctypes.byref(p), _target_ptr(target), w * 4) == -1
    assert engine.scene_allocations() == before, f"{name}: a refused frame allocated a scene buffer"
    assert np.array_equal(engine.read_buffer("scene", np.uint8, 64), shown), f"{name}: a refused frame changed what VELLO_HIP_BUF_SCENE shows"


def _cut_at_path(lib, fr, d0, d1):
    """The sub-fragment of `fr` that holds its draw objects [d0, d1) -- tags cut behind PATH markers, transforms / styles / draw data
    counted from the tags and draw tags in between -- with the fragment's first TRANSFORM and STYLE markers kept in front when d0 is
    the first: used to make fragments whose clips do not balance."""
    L = lib.layout
    words = lib.packed.view(np.uint32)
    tags = lib.packed[L.path_tag_base * 4: L.path_data_base * 4]
    t0, t1 = fr["path_tags"]
    ends = [t0 + i + 1 for i, t in enumerate(tags[t0:t1]) if t & 0x10]  # the tag behind each PATH marker
    cuts = [t0] + ends
    a, b = cuts[d0 - fr["draws"][0]], cuts[d1 - fr["draws"][0]]
    pre = tags[t0:a]
    inside = tags[a:b]
    dt = words[L.draw_tag_base + fr["draws"][0]: L.draw_tag_base + d1]
    dd_before = int(((dt[: d0 - fr["draws"][0]] >> 2) & 7).sum())
    dd_in = int(((dt[d0 - fr["draws"][0]:] >> 2) & 7).sum())

    def n(seg, bit):
        return int(((seg & bit) != 0).sum())

    # path data words per tag: LINETO 2, QUADTO 4, CUBICTO 6 (f32 coordinates), + 2 for the point a subpath starts with -- not needed:
    # the refusal comes from the draw tags before anything reads path data, so its range is left empty
    return {"path_tags": (a, b), "path_data": (0, 0), "draws": (d0, d1), "draw_data": (fr["draw_data"][0] + dd_before, fr["draw_data"][0] + dd_before + dd_in),
            "transforms": (fr["transforms"][0] + n(pre, 0x20), fr["transforms"][0] + n(pre, 0x20) + n(inside, 0x20)),
            "styles": (fr["styles"][0] + n(pre, 0x40), fr["styles"][0] + n(pre, 0x40) + n(inside, 0x40))}


# ---------------------------------------------------------------------------------------------------------------
# The symbol map (GPU suite, scripts/scene_instances_bench.py)
# ---------------------------------------------------------------------------------------------------------------
def symbol_fragments(seed=0x5EED0001, n_frags=64):
    """One path per fragment, about the origin, drawn from the distributions of workloads.paris_like_scene_d2: 70 % stroked open
    polylines, 25 % filled polygons, 5 % filled cubic blobs, its palette."""
    from vello_amd import Affine, BezPath, Fill, Scene, Stroke
    from workloads.scenes import CLOSE_PATH, CURVE_TO, MOVE_TO, PALETTE, _polyline

    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    kinds = rng.random(n_frags)
    for i in range(n_frags):
        s = Scene()
        col = PALETTE[int(rng.integers(0, len(PALETTE)))]
        k = kinds[i]
        if k < 0.70:
            n = int(rng.integers(8, 61))
            step = rng.uniform(4.0, 40.0)
            heading = rng.uniform(0, 2 * math.pi) + np.cumsum(rng.normal(0.0, 0.4, n))
            pts = np.stack([np.cumsum(np.cos(heading) * step), np.cumsum(np.sin(heading) * step)], axis=1)
            pts -= pts.mean(axis=0)
            s.stroke(Stroke(math.exp(rng.uniform(math.log(0.5), math.log(4.0)))), Affine.IDENTITY, col, None, _polyline(pts, False))
        elif k < 0.95:
            n = int(rng.integers(6, 41))
            r = rng.uniform(5.0, 60.0)
            ang = np.sort(rng.uniform(0, 2 * math.pi, n))
            rr = r * rng.uniform(0.7, 1.0, n)
            s.fill(Fill.NonZero, Affine.IDENTITY, col, None, _polyline(np.stack([rr * np.cos(ang), rr * np.sin(ang)], axis=1), True))
        else:
            n = int(rng.integers(4, 13))
            r = rng.uniform(10.0, 60.0)
            ang = np.linspace(0, 2 * math.pi, n, endpoint=False) + rng.uniform(0, 1)
            rr = r * rng.uniform(0.7, 1.0, n)
            px, py = rr * np.cos(ang), rr * np.sin(ang)
            verbs, coords = [MOVE_TO], [px[0], py[0]]
            for j in range(n):
                a, b = j, (j + 1) % n
                t = 0.55 * r * (2 * math.pi / n) / 1.5
                verbs.append(CURVE_TO)
                coords.extend([px[a] - t * math.sin(ang[a]), py[a] + t * math.cos(ang[a]), px[b] + t * math.sin(ang[b]), py[b] - t * math.cos(ang[b]), px[b], py[b]])
            verbs.append(CLOSE_PATH)
            s.fill(Fill.NonZero, Affine.IDENTITY, col, None, BezPath.from_arrays(verbs, coords))
        out.append(s)
    return out


def symbol_instances(seed, n_frags=64, n=30000, size=1600.0, phase=0.0):
    """n placements over a size x size canvas as an INSTANCE_DTYPE array: a fragment, a position, a rotation (+ phase: an animation
    turns every symbol) and no scale, so that the geometry weighs what the d2 scene's does."""
    from vello_amd import INSTANCE_DTYPE

    rng = np.random.Generator(np.random.PCG64(seed))
    inst = np.zeros(n, dtype=INSTANCE_DTYPE)
    inst["fragment"] = rng.integers(0, n_frags, n)
    a = rng.uniform(0, 2 * math.pi, n) + phase
    t = inst["transform"]
    t[:, 0], t[:, 1], t[:, 2], t[:, 3] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)
    t[:, 4], t[:, 5] = rng.uniform(0, size, n), rng.uniform(0, size, n)
    return inst


def instance_list(inst):
    """An INSTANCE_DTYPE array as the (fragment, transform) pairs compose() takes."""
    return [(int(f), t) for f, t in zip(inst["fragment"], inst["transform"])]
