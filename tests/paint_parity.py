"""Per-instance paints (vello_hip_render_instances_painted) against the CPU oracle.  As in tests/instance_parity.py the oracle knows
nothing of instances, and nothing of paints: it is handed the composed scene -- instance_parity.compose's, with the colour words of the
painted instances replaced here in numpy by the rule of include/vello_hip.h, applied to the library's draw tags.  Every comparison is
exact: VELLO_HIP_BUF_SCENE against the numpy bytes, the 64 bytes of slack zero, VELLO_HIP_BUF_CONFIG against the unpainted layout, the
image against the oracle's on the painted bytes.  Every painted case asserts that its expected bytes differ from the unpainted
composition, so that a build that ignores paints fails, and paints are distinct per instance (0xFF000000 | i-style words), so that a
word taken from the wrong instance shows."""
import ctypes

import numpy as np

from oracle.oracle import Oracle
from tests import instance_parity as ip
from tests import parity

BLACK, WHITE = ip.BLACK, ip.WHITE
KEEP, SOLID = 0, 1
FILL_COLOR, BLURRED_ROUNDED_RECT, BEGIN_CLIP = 0x44, 0x2D4, 0x49
IDENT = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def word(i):
    """A paint no other instance has and no library colour equals (the makers' colours are opaque with channels of at least 40)."""
    return 0xFF000000 | (int(i) + 1)


# ---------------------------------------------------------------------------------------------------------------
# The numpy reference
# ---------------------------------------------------------------------------------------------------------------
def colour_mask(packed, layout, fr):
    """One bool per word of the fragment's draw_data range: walk its draw tags in order, a running offset d = 0, a tag t advancing d
    by (t >> 2) & 7; word d of a FILL_COLOR or BLURRED_ROUNDED_RECT tag is a colour word, nothing else is."""
    words = np.ascontiguousarray(packed, dtype=np.uint8).view(np.uint32)
    b, e = fr["draws"]
    tags = words[layout.draw_tag_base + b: layout.draw_tag_base + e]
    mask = np.zeros(fr["draw_data"][1] - fr["draw_data"][0], dtype=bool)
    d = 0
    for t in tags:
        t = int(t)
        if t in (FILL_COLOR, BLURRED_ROUNDED_RECT):
            mask[d] = True
        d += (t >> 2) & 7
    assert d == len(mask)
    return mask


def _pairs(paints, n):
    """(flags, rgba) per instance of what Engine.render_instances takes as `paints`: None, an int word, a Color, or a PAINT_DTYPE array."""
    from vello_amd import PAINT_DTYPE, Color

    if isinstance(paints, np.ndarray) and paints.dtype == PAINT_DTYPE:
        out = [(int(f), int(c)) for f, c in zip(paints["flags"], paints["rgba"])]
    else:
        out = [(KEEP, 0) if p is None else (SOLID, p.premul_rgba8() if isinstance(p, Color) else int(p)) for p in paints]
    assert len(out) == n
    return out


def compose(packed, layout, fragments, instances, paints):
    """(painted bytes, unpainted bytes, Layout): instance_parity.compose, patched.  Per instance the draw-data offset is the running sum
    of the fragments' draw-data lengths; the colour words of an instance whose paint is SOLID become its rgba."""
    plain, lay = ip.compose(packed, layout, fragments, instances)
    out = plain.copy()
    dd = out.view(np.uint32)[lay.draw_data_base: lay.transform_base]
    masks = {}
    off = 0
    for (fi, _), (flags, rgba) in zip(instances, _pairs(paints, len(instances))):
        fi = int(fi)
        fr = fragments[fi]
        n = fr["draw_data"][1] - fr["draw_data"][0]
        if flags == SOLID and n:
            if fi not in masks:
                masks[fi] = colour_mask(packed, layout, fr)
            dd[off: off + n][masks[fi]] = rgba
        off += n
    assert off == len(dd)
    return out, plain, lay


def oracle_image(lib, packed, layout, w, h, base, aa):
    o = Oracle(capacity_scale=4, auto_grow=True)
    o.set_scene(packed, layout, w, h, base, int(aa))
    o.set_ramps(lib.ramps)
    o.set_image_atlas(lib.resolved.atlas_image())
    return o.render().copy()


def check_bytes(engine, name, lib, instances, paints, w=64, h=48, upload=True, differs=True, aa=None):
    """One painted frame: scene bytes, slack, config and image, all exact.  Returns (painted, unpainted, layout)."""
    from vello_amd import AaConfig

    aa = AaConfig.Msaa8 if aa is None else aa
    if upload:
        lib.upload(engine)
    packed, plain, layout = compose(lib.packed, lib.layout, lib.fragments, instances, paints)
    if differs:
        assert not np.array_equal(packed, plain), f"{name}: the paints change no byte: the case proves nothing"
    else:
        assert np.array_equal(packed, plain), f"{name}: the paints were to change nothing"
    lay, nbytes = engine.instances_layout(instances)
    assert lay == layout and nbytes == packed.nbytes, f"{name}: {lay} {nbytes} != {layout} {packed.nbytes}"
    engine.render_instances(instances, w, h, BLACK, aa, paints=paints)
    assert engine.sync() == 0, name
    got = engine.read_buffer("scene", np.uint8, packed.nbytes + 64)
    bad = np.nonzero(got[:packed.nbytes] != packed)[0]
    assert bad.size == 0, f"{name}: painted bytes differ first at word {bad[0] // 4} (draw data begins at word {layout.draw_data_base})"
    assert not got[packed.nbytes:].any(), f"{name}: the 64 bytes of slack are not zero"
    cfg = engine.read_buffer("config", np.uint32, 88)
    assert [int(v) for v in cfg[5:15]] == list(layout), f"{name}: VELLO_HIP_BUF_CONFIG does not hold the composed layout"
    img = engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4)
    assert np.array_equal(img, oracle_image(lib, packed, layout, w, h, BLACK, aa)), f"{name}: image"
    return packed, plain, layout


class PaintedEngine(ip.InstanceEngine):
    """InstanceEngine through the painted entry point: what compare_frame sees as the engine."""

    def __init__(self, engine, instances, paints):
        super().__init__(engine, instances)
        self._paints = paints

    def render(self, packed, layout, width, height, base_color, aa, ramps=None):
        e = self._engine
        lay, nbytes = e.instances_layout(self._instances)
        assert lay == layout and nbytes == len(packed), (lay, layout, nbytes, len(packed))
        for _ in range(12):
            self.frames += 1
            e.render_instances(self._instances, width, height, base_color, aa, paints=self._paints)
            r = e.sync()
            if r != -4:
                break
            assert e.grow_pools(e.bump()), "E_CAPACITY, but no pool had to grow"
        assert r == 0, f"sync: {r}"
        return e.read_buffer("output", np.uint8, width * height * 4).reshape(height, width, 4).copy(), e.bump()


def compare_painted_frame(engine, lib, instances, paints, w, h, base, aa, name, upload=True, **kw):
    """The full compare_frame -- every intermediate, with culling and, in its back half, without -- of a painted frame."""
    if upload:
        lib.upload(engine)
    packed, plain, layout = compose(lib.packed, lib.layout, lib.fragments, instances, paints)
    assert not np.array_equal(packed, plain), f"{name}: the paints change no byte"
    pe = PaintedEngine(engine, instances, paints)
    img, ref, bump = parity.compare_frame(pe, packed, layout, w, h, base, aa, name, resolved=ip._Late(lib), **kw)
    assert pe.frames > 0
    assert np.array_equal(engine.read_buffer("scene", np.uint8, packed.nbytes), packed), f"{name}: VELLO_HIP_BUF_SCENE is not the painted scene"
    return img, ref, bump


def grid(n, w, h, scale=1.0):
    """n placements on a grid over w x h."""
    cols = max(1, int(np.ceil(np.sqrt(n * w / h))))
    rows = (n + cols - 1) // cols
    return [(scale, 0.0, 0.0, scale, (i % cols + 0.5) * w / cols, (i // cols + 0.5) * h / rows) for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------
# 1. Mask bit positions
# ---------------------------------------------------------------------------------------------------------------
def mask_library():
    """Some 70 one-colour polygons with solid (two colour words), linear (five words, none a colour), blur (a colour word and four
    floats), clip and blend interleaved, so that the library's draw-data stream crosses 32-word boundaries with a colour word on bit 31
    and on bit 0 of a mask word, each beside a word that is none; and, last, the whole library once more as ONE fragment: its mask
    does not begin where its draw data begins; and one whose draw tags and draw data are not aligned as the library's are."""
    import vello_amd

    br = ip.brush_fragments()
    plan = ["p"] * 32 + ["linear", "blur", "solid", "clip", "blend"] + ["p"] * 4 + ["linear"] + ["p"] * 30 + ["blur", "p", "p", "p", "p"]
    scenes, k = [], 0
    for what in plan:
        if what == "p":
            scenes.append(ip.polygon(3 + k % 5, seed=k, r=6.0))
            k += 1
        else:
            scenes.append(br[what])
    lib = vello_amd.FragmentLibrary(scenes)
    lib.kinds = plan
    assert k == 70
    lib.whole = len(lib.fragments)
    lib.fragments.append({s: (0, lib.fragments[-1][s][1]) for s in ip.STREAMS})
    # ... and a hand-written fragment that overlaps others at another alignment: polygon 0 with, as its one draw-data word, the first
    # word of the linear gradient's five.  To that fragment the word is a colour; to the gradient's own fragment it is none.
    d = lib.fragments[plan.index("linear")]["draw_data"][0]
    lib.misaligned = len(lib.fragments)
    lib.fragments.append(dict(lib.fragments[0], draw_data=(d, d + 1)))
    return lib


def check_mask_bits(engine, name):
    lib = mask_library()
    n = lib.whole
    mask = np.concatenate([colour_mask(lib.packed, lib.layout, f) for f in lib.fragments[:n]])
    assert len(mask) == lib.layout.transform_base - lib.layout.draw_data_base and len(mask) > 96, len(mask)  # crosses words 32, 64 and 96
    assert np.array_equal(mask, colour_mask(lib.packed, lib.layout, lib.fragments[lib.whole]))
    assert any(mask[p] and not mask[p + 1] for p in range(31, len(mask) - 1, 32)), "no colour word on bit 31 beside a word that is none"
    assert any(mask[p] and not mask[p - 1] for p in range(32, len(mask), 32)), "no colour word on bit 0 beside a word that is none"
    assert 0 < mask.sum() < len(mask)
    w, h = 256, 200
    # every fragment once painted and once kept; the fragment that is the whole library painted, over everything
    places = grid(2 * n, w, h, 0.7)
    inst = [(i % n, places[i]) for i in range(2 * n)] + [(lib.whole, (0.5, 0.0, 0.0, 0.5, 128.0, 100.0))]
    inst += [(lib.misaligned, (2.0, 0.0, 0.0, 2.0, 40.0, 40.0)), (lib.misaligned, (2.0, 0.0, 0.0, 2.0, 200.0, 150.0))]
    paints = [word(i) if i < n else None for i in range(2 * n)] + [word(2 * n), word(2 * n + 1), None]
    assert colour_mask(lib.packed, lib.layout, lib.fragments[lib.misaligned]).tolist() == [True]
    assert not mask[lib.fragments[lib.misaligned]["draw_data"][0]]
    packed, plain, layout = check_bytes(engine, name, lib, inst, paints, w, h)
    changed = np.nonzero(packed.view(np.uint32) != plain.view(np.uint32))[0]
    assert changed.size == 2 * int(mask.sum()) + 1, f"{name}: {changed.size} words changed, the painted fragments hold {2 * int(mask.sum()) + 1} colour words"
    assert packed.view(np.uint32)[layout.transform_base - 2] == word(2 * n + 1)
    # ... and the other way round
    check_bytes(engine, name + "_swapped", lib, inst, [None if p is not None else word(i) for i, p in enumerate(paints)], w, h, upload=False)


# ---------------------------------------------------------------------------------------------------------------
# 2 - 4. Chunks of the draw-data stream
# ---------------------------------------------------------------------------------------------------------------
def check_chunk_boundaries(engine, name):
    """700 instances of one-word polygons: the draw-data stream is 700 words, three chunks of 256 at steps == 1, and word i is instance
    i's colour.  Painted iff i % 3 != 0 paints the words 256, 511 and 512 and keeps word 255 (255 is a multiple of 3: no rule of period
    3 paints all four boundary words); a second frame paints 255 as well."""
    import vello_amd

    lib = vello_amd.FragmentLibrary([ip.polygon(k, seed=k, r=5.0) for k in (3, 4, 5, 6)])
    lib.upload(engine)
    places = grid(700, 128, 96, 0.5)
    inst = [(i % 4, places[i]) for i in range(700)]
    for label, painted in (("mod3", lambda i: i % 3 != 0), ("edges", lambda i: i % 3 != 0 or i in (255, 256, 511, 512))):
        paints = [word(i) if painted(i) else None for i in range(700)]
        packed, plain, layout = check_bytes(engine, f"{name}_{label}", lib, inst, paints, 128, 96, upload=False)
        assert layout.transform_base - layout.draw_data_base == 700 and packed.nbytes // 4 <= 2048 * 256  # steps == 1
        dd = packed.view(np.uint32)[layout.draw_data_base: layout.transform_base]
        for i in (256, 511, 512) + ((255,) if label == "edges" else ()):
            assert dd[i] == word(i), (label, i)
        if label == "mod3":
            assert dd[255] == plain.view(np.uint32)[layout.draw_data_base + 255] != word(255)


def check_long_chunks(engine, name, steps):
    """The library and the shrink of instance_parity.check_long_chunks, with 1 100 instances of its 5-gon per step in front: the
    draw-data stream alone spans more than two chunks of steps x 256 words.  Every third instance is painted."""
    import vello_amd

    lib = vello_amd.FragmentLibrary([ip.polygon(4000), ip.polygon(20003), ip.polygon(5)])
    rng = np.random.default_rng(steps)

    def place():
        return (0.05, 0.0, 0.0, 0.05, float(rng.uniform(4, 60)), float(rng.uniform(4, 44)))

    inst = [(2, place()) for _ in range(550 * steps + 40)]
    tags = sum(lib.fragments[f]["path_tags"][1] - lib.fragments[f]["path_tags"][0] for f, _ in inst)
    rest = sum(ip._composed_words(lib.fragments[f], 1) - (lib.fragments[f]["path_tags"][1] - lib.fragments[f]["path_tags"][0] + 1023) // 1024 * 256 for f, _ in inst)
    while (tags + 1023) // 1024 * 256 + rest <= (steps - 1) * 2048 * 256:
        f = int(rng.integers(0, 3)) if len(inst) % 8 else 1
        inst.append((f, place()))
        fr = lib.fragments[f]
        tags += fr["path_tags"][1] - fr["path_tags"][0]
        rest += ip._composed_words(fr, 1) - (fr["path_tags"][1] - fr["path_tags"][0] + 1023) // 1024 * 256
    paints = [word(i) if i % 3 == 0 else None for i in range(len(inst))]
    packed, plain, layout = check_bytes(engine, f"{name}_{steps}", lib, inst, paints)
    assert (steps - 1) * 2048 * 256 < packed.nbytes // 4 <= steps * 2048 * 256, packed.nbytes
    assert sum(1 for f, _ in inst if f == 2) >= 550 * steps and layout.transform_base - layout.draw_data_base > 2 * steps * 256


def check_unstaged(engine, name):
    """More instances in one chunk than the kernel stages offsets for: 3 000 empty instances, every one painted, between painted
    neighbours.  The empty instances' paints are ignored; the neighbours get their own."""
    import vello_amd

    lib = vello_amd.FragmentLibrary([ip.polygon(5, r=8.0), ip.polygon(7, r=8.0), ip.brush_fragments()["blur"]])
    empty = len(lib.fragments)
    lib.fragments.append(dict(ip.EMPTY))
    inst = [(0, (1, 0, 0, 1, 14.0, 14.0))] + [(empty, IDENT)] * 3000 + [(1, (1, 0, 0, 1, 40.0, 30.0)), (2, (1, 0, 0, 1, 30.0, 16.0))]
    paints = [word(i) for i in range(len(inst))]
    packed, plain, layout = check_bytes(engine, name, lib, inst, paints)
    dd = packed.view(np.uint32)[layout.draw_data_base: layout.transform_base]
    assert [int(v) for v in dd[:3]] == [word(0), word(3001), word(3002)] and len(dd) == 7


# ---------------------------------------------------------------------------------------------------------------
# 5, 6. What is a colour word, and what a colour is
# ---------------------------------------------------------------------------------------------------------------
def check_no_colour_words(engine, name):
    """Gradient, image and clip-around-gradient fragments, all painted: the bytes of the unpainted composition.  In `blend` both fill
    colours change and the layer's blend and alpha words do not; in `blur` word 0 changes and the four floats keep their bits."""
    import vello_amd

    br = ip.brush_fragments()
    keys = ["linear", "radial", "sweep", "image", "clip"]
    lib = vello_amd.FragmentLibrary([br[k] for k in keys + ["blend", "blur"]])
    lib.upload(engine)
    w, h = 160, 120
    places = grid(7, w, h, 1.5)
    inst = [(i, places[i]) for i in range(5)]
    check_bytes(engine, name + "_none", lib, inst, [word(i) for i in range(5)], w, h, upload=False, differs=False)
    for fi, label in ((5, "blend"), (6, "blur")):
        one = [(fi, places[fi])]
        packed, plain, layout = check_bytes(engine, f"{name}_{label}", lib, one, [0xFF123456], w, h, upload=False)
        dd, dd0 = (x.view(np.uint32)[layout.draw_data_base: layout.transform_base] for x in (packed, plain))
        tags = [int(t) for t in packed.view(np.uint32)[layout.draw_tag_base: layout.draw_data_base]]
        if label == "blend":
            assert tags[:3] == [FILL_COLOR, BEGIN_CLIP, FILL_COLOR] and len(dd) == 4
            assert [int(v) for v in dd] == [0xFF123456, int(dd0[1]), int(dd0[2]), 0xFF123456] and dd0[0] != dd0[3]
        else:
            assert tags == [BLURRED_ROUNDED_RECT] and len(dd) == 5
            assert dd[0] == 0xFF123456 != dd0[0] and np.array_equal(dd[1:], dd0[1:])


def check_colour_values(engine, name):
    """Any rgba is a colour: transparent black, white, and the two draw tags whose first word is a colour."""
    import vello_amd

    lib = vello_amd.FragmentLibrary([ip.polygon(5, r=9.0), ip.polygon(6, seed=1, r=9.0), ip.brush_fragments()["blur"]])
    lib.upload(engine)
    values = [0x00000000, 0xFFFFFFFF, 0x00000044, 0x000002D4]
    places = grid(8, 96, 64)
    inst = [(i % 3, places[i]) for i in range(8)]
    paints = [values[i % 4] for i in range(8)]
    packed, plain, layout = check_bytes(engine, name, lib, inst, paints, 96, 64, upload=False)
    dd = packed.view(np.uint32)[layout.draw_data_base: layout.transform_base]
    assert {int(v) for v in dd} >= set(values)
    # KEEP with any rgba changes nothing
    from vello_amd import PAINT_DTYPE

    keep = np.zeros(8, dtype=PAINT_DTYPE)
    keep["rgba"] = values * 2
    check_bytes(engine, name + "_keep", lib, inst, keep, 96, 64, upload=False, differs=False)


# ---------------------------------------------------------------------------------------------------------------
# 7. Occlusion
# ---------------------------------------------------------------------------------------------------------------
def check_occlusion(engine, name):
    """A rectangle that covers whole tiles over a dozen polygons, painted opaque in one frame and with alpha 0x80 in another: coarse
    reads the composed colour, so the first may occlude the polygons and the second may not."""
    import vello_amd
    from vello_amd import AaConfig, Affine, Color, Fill, Rect, Scene

    cover = Scene()
    cover.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(200, 200, 60), None, Rect(-50.0, -40.0, 50.0, 40.0))
    lib = vello_amd.FragmentLibrary([ip.polygon(k, seed=k, r=10.0) for k in (3, 5, 6, 8)] + [cover])
    lib.upload(engine)
    w, h = 160, 128
    rng = np.random.default_rng(17)
    inst = [(i % 4, (1.5, 0.0, 0.0, 1.5, float(rng.uniform(40, 120)), float(rng.uniform(34, 94)))) for i in range(12)]
    inst.append((4, (1.0, 0.0, 0.0, 1.0, 80.0, 64.0)))  # x 30 .. 130, y 24 .. 104: the tiles 2 .. 7 x 2 .. 5 whole
    images, segments = {}, {}
    for label, rgba in (("opaque", 0xFF203040), ("translucent", 0x80102030)):
        paints = [word(i) for i in range(12)] + [rgba]
        for aa in (AaConfig.Msaa16, AaConfig.Area):
            img, ref, bump = compare_painted_frame(engine, lib, inst, paints, w, h, WHITE, aa, f"{name}_{label}_{int(aa)}", upload=False,
                                                   tol=1 if int(aa) == 0 else 0)
            images[label, int(aa)] = ref
            segments[label, int(aa)] = bump["segments"]
    for aa in (0, 2):  # (bump.segments of the frame with culling on: coarse drops what an opaque full-tile cover hides)
        assert segments["opaque", aa] < segments["translucent", aa], f"{name}: the opaque cover occluded nothing ({segments})"
    inner = (slice(48, 80), slice(48, 112))
    assert (images["opaque", 2][inner] == np.array([0x40, 0x30, 0x20, 0xFF], dtype=np.uint8)).all(), "the opaque cover does not hide the polygons"
    assert len(np.unique(images["translucent", 2][inner].reshape(-1, 4), axis=0)) > 1, "nothing shows through the translucent cover"


# ---------------------------------------------------------------------------------------------------------------
# 8. Host agreement
# ---------------------------------------------------------------------------------------------------------------
def fill_fragment(k, color, seed=0, r=10.0):
    """A one-fill fragment whose geometry depends on (k, seed) alone and whose colour is the caller's."""
    from vello_amd import Affine, BezPath, Fill, Scene

    rng = np.random.default_rng(500 + 17 * k + seed)
    a = np.sort(rng.uniform(0, 2 * np.pi, k))
    rr = r * rng.uniform(0.6, 1.0, k)
    p = BezPath()
    p.move_to((float(rr[0] * np.cos(a[0])), float(rr[0] * np.sin(a[0]))))
    for t, q in zip(a[1:], rr[1:]):
        p.line_to((float(q * np.cos(t)), float(q * np.sin(t))))
    p.close_path()
    s = Scene()
    s.fill(Fill.NonZero, Affine.IDENTITY, color, None, p)
    return s


def check_host_agreement(engine, name):
    """What rgba means to the host encoder: the painted composition of one-fill fragments equals Resolver.resolve of a Scene that appends
    the same geometry ENCODED with that colour under the same transforms -- bytes and layout -- the paint word being
    Color.premul_rgba8(), for opaque colours and for translucent ones."""
    import vello_amd
    from vello_amd import AaConfig, Affine, Color, Scene

    shapes = [(3, 0), (5, 1), (8, 2), (4, 3)]
    grey = Color.from_rgb8(128, 128, 128)
    resolver = vello_amd.Resolver()
    lib = vello_amd.FragmentLibrary([fill_fragment(k, grey, seed) for k, seed in shapes], resolver=resolver)
    lib.upload(engine)
    rng = np.random.default_rng(9)
    colours = [Color.from_rgb8(250, 20, 30), Color(0.2, 0.9, 0.4, 0.5), Color.from_rgb8(10, 200, 240), Color(1.0, 0.5, 0.25, 0.5),
               Color(0.3, 0.3, 1.0, 0.5), Color.from_rgb8(255, 255, 255), Color(0.0, 0.0, 0.0, 0.5)]
    affs = [Affine.translate(float(rng.uniform(20, 140)), float(rng.uniform(20, 100))) * Affine.rotate(float(rng.uniform(0, 6.0))) * Affine.scale(float(rng.uniform(0.8, 2.5)))
            for _ in colours]
    picks = [int(rng.integers(0, len(shapes))) for _ in colours]
    host = Scene()
    for f, a, col in zip(picks, affs, colours):
        host.append(fill_fragment(*shapes[f][:1], col, shapes[f][1]), a)
    hr = resolver.resolve(host)
    instances = list(zip(picks, affs))
    packed, plain, layout = compose(lib.packed, lib.layout, lib.fragments, instances, colours)
    alphas = {c.premul_rgba8() >> 24 for c in colours}
    assert 0xFF in alphas and any(0x7F <= a <= 0x80 for a in alphas), alphas
    assert not np.array_equal(packed, plain)
    assert layout == hr.layout, f"{name}: {layout} != {hr.layout}"
    assert np.array_equal(packed, hr.packed), f"{name}: the numpy composition is not what the host encodes with these colours"
    engine.render_instances(instances, 160, 120, BLACK, AaConfig.Msaa16, paints=colours)
    assert engine.sync() == 0
    assert np.array_equal(engine.read_buffer("scene", np.uint8, packed.nbytes), hr.packed), f"{name}: the engine's painted composition is not the host's encoding"
    assert np.array_equal(engine.read_buffer("output", np.uint8, 160 * 120 * 4).reshape(120, 160, 4), oracle_image(lib, hr.packed, hr.layout, 160, 120, BLACK, AaConfig.Msaa16))


# ---------------------------------------------------------------------------------------------------------------
# 9. paints == NULL, n == 0
# ---------------------------------------------------------------------------------------------------------------
def _params_ptr(engine, w, h, base, aa):
    return engine._params(w, h, base, aa)


def _painted_raw(engine, inst, paints_ptr, n, p, target_ptr, stride):
    return engine._lib.vello_hip_render_instances_painted(engine._h, inst.ctypes.data if inst is not None else None, paints_ptr, n, ctypes.byref(p), target_ptr, stride)


def check_null_and_empty(engine, name):
    """paints == NULL is vello_hip_render_instances: bytes, image and bump counters; n == 0 with and without a paints pointer is the
    base colour."""
    import vello_amd
    from vello_amd import AaConfig
    from vello_amd.renderer import instance_array

    br = ip.brush_fragments()
    lib = vello_amd.FragmentLibrary([ip.polygon(5), br["solid"], br["blend"], br["linear"]])
    lib.upload(engine)
    w, h, aa = 96, 64, AaConfig.Msaa16
    places = grid(9, w, h, 1.2)
    inst = instance_array([(i % 4, places[i]) for i in range(9)])
    plain, layout = ip.compose(lib.packed, lib.layout, lib.fragments, ip.instance_list(inst))
    engine.render_instances(inst, w, h, BLACK, aa)
    assert engine.sync() == 0
    want = [engine.read_buffer("scene", np.uint8, plain.nbytes + 64).copy(), engine.read_buffer("output", np.uint8, w * h * 4).copy(), engine.bump()]
    assert np.array_equal(want[0][:plain.nbytes], plain)
    # a painted frame in between, so that the NULL frame is not simply what the buffers still hold
    engine.render_instances(inst, w, h, BLACK, aa, paints=[word(i) for i in range(9)])
    assert engine.sync() == 0
    assert not np.array_equal(engine.read_buffer("scene", np.uint8, plain.nbytes), plain)
    p = _params_ptr(engine, w, h, BLACK, aa)
    assert _painted_raw(engine, inst, None, len(inst), p, None, 0) == 0
    assert engine.sync() == 0
    got = [engine.read_buffer("scene", np.uint8, plain.nbytes + 64), engine.read_buffer("output", np.uint8, w * h * 4), engine.bump()]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], f"{name}: paints == NULL is not render_instances"
    # n == 0
    base = 0xFF336699
    p = _params_ptr(engine, w, h, base, aa)
    dummy = np.zeros(1, dtype=vello_amd.PAINT_DTYPE)
    for label, ptr in (("null", None), ("pointer", dummy.ctypes.data)):
        engine.render_instances(inst, w, h, BLACK, aa)  # something else first
        assert _painted_raw(engine, None, ptr, 0, p, None, 0) == 0, label
        assert engine.sync() == 0
        img = engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4)
        assert (img == np.array([0x99, 0x66, 0x33, 0xFF], dtype=np.uint8)).all(), f"{name}: n == 0 ({label}) is not the base colour"
    engine.render_instances([], w, h, base, aa, paints=[])
    assert engine.sync() == 0
    assert (engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4) == np.array([0x99, 0x66, 0x33, 0xFF], dtype=np.uint8)).all()


# ---------------------------------------------------------------------------------------------------------------
# 10. Life cycle
# ---------------------------------------------------------------------------------------------------------------
def render_painted_into(engine, instances, paints, w, h, base, aa, target):
    """vello_hip_render_instances_painted into `target` (a torch tensor on the GPU; the emulated build: a numpy array)."""
    from vello_amd import paint_array
    from vello_amd.renderer import instance_array

    inst = instance_array(instances)
    pt = paint_array(paints) if paints is not None else None
    p = engine._params(w, h, base, aa)
    engine._check(_painted_raw(engine, inst, pt.ctypes.data if pt is not None else None, len(inst), p, ip._target_ptr(target), w * 4), "render_instances_painted")


def check_life_cycle(engine, name, make_target, to_numpy):
    """Four frames in flight: one list, four paint arrays, four targets, each the oracle's for its own paints; then an unpainted frame on
    each lane shows the library's colours; no scene re-allocation in the steady state; a view and culling on top; run_stages after a
    painted frame; the library's bytes unchanged; render_resident still shows the library whole."""
    import vello_amd
    from tests import view_parity
    from vello_amd import AaConfig, Affine

    w, h, aa = 160, 120, AaConfig.Msaa16
    frs = ip.brush_fragments()
    lib = vello_amd.FragmentLibrary([frs["solid"], frs["linear"], frs["clip"], ip.polygon(6), frs["blend"], frs["blur"]])
    lib.upload(engine)
    rng = np.random.default_rng(23)
    inst = ip.scatter(rng, 24, 6, w, h, scale=(0.8, 2.5))
    n = len(inst)
    paint_sets = [[word(100 * k + i) if (i + k) % 2 else None for i in range(n)] for k in range(3)] + [[0x80402010 + i for i in range(n)]]

    def want_for(paints, view=None):
        packed, plain, layout = compose(lib.packed, lib.layout, lib.fragments, inst, paints)
        if view is not None:
            packed = view_parity.compose(packed, layout, view)
        return oracle_image(lib, packed, layout, w, h, BLACK, aa)

    want = [want_for(ps) for ps in paint_sets]
    want_plain = ip._want(lib, inst, w, h, BLACK, aa)
    want_lib = ip._want(lib, [(k, IDENT) for k in range(6)], w, h, BLACK, aa)
    assert len({x.tobytes() for x in want + [want_plain, want_lib]}) == 6
    try:
        engine.set_frames_in_flight(4)
        for rnd in range(2):
            t = [make_target(w, h) for _ in range(4)]
            for k in range(4):
                render_painted_into(engine, inst, paint_sets[(k + rnd) % 4], w, h, BLACK, aa, t[k])
            assert engine.sync() == 0
            for k in range(4):
                assert np.array_equal(to_numpy(t[k]), want[(k + rnd) % 4]), f"{name}: round {rnd}, frame {k} does not show its own paints"
        # an unpainted frame on each lane: the library's colours (through both entry points)
        t = [make_target(w, h) for _ in range(4)]
        for k in range(4):
            if k % 2:
                ip.render_instances_into(engine, inst, w, h, BLACK, aa, t[k])
            else:
                render_painted_into(engine, inst, None, w, h, BLACK, aa, t[k])
        assert engine.sync() == 0
        for k in range(4):
            assert np.array_equal(to_numpy(t[k]), want_plain), f"{name}: the unpainted frame on lane {k} does not show the library's colours"
        # steady state: painted and unpainted frames of one list allocate nothing
        before = engine.scene_allocations()
        for k in range(12):
            render_painted_into(engine, inst, paint_sets[k % 4] if k % 3 else None, w, h, BLACK, aa, t[k % 4])
        assert engine.sync() == 0
        assert engine.scene_allocations() == before, f"{name}: {engine.scene_allocations() - before} scene buffers re-allocated in the steady state"
        for k in range(8, 12):
            assert np.array_equal(to_numpy(t[k % 4]), want[k % 4] if k % 3 else want_plain), f"{name}: steady-state frame {k}"
    finally:
        engine.set_frames_in_flight(1)
    # a view on top, culling on
    view = Affine.translate(0.3 * w, -0.1 * h) * Affine.rotate(0.3) * Affine.scale(1.4)
    tv = make_target(w, h)
    wv = want_for(paint_sets[1], view=view)
    assert not np.array_equal(wv, want[1])
    for cull in (True, False):
        try:
            engine.set_view_transform(view)
            engine.set_viewport_cull(cull)
            render_painted_into(engine, inst, paint_sets[1], w, h, BLACK, aa, tv)
            assert engine.sync() == 0
        finally:
            engine.set_view_transform(None)
            engine.set_viewport_cull(False)
        assert np.array_equal(to_numpy(tv), wv), f"{name}: painted instances under a view, culling {cull}"
    # run_stages acts on the painted scene of the last frame
    engine.run_stages(w, h, BLACK, aa, "pathtag_scan", "fine")
    assert np.array_equal(engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4), want[1]), f"{name}: run_stages after a painted frame"
    view_parity.render_resident_into(engine, w, h, BLACK, aa, tv)
    assert engine.sync() == 0
    assert np.array_equal(to_numpy(tv), want_lib), f"{name}: render_resident does not show the library whole"
    assert np.array_equal(engine.read_buffer("scene", np.uint8, lib.packed.nbytes), lib.packed), f"{name}: the library's bytes changed"


# ---------------------------------------------------------------------------------------------------------------
# 11. Errors
# ---------------------------------------------------------------------------------------------------------------
def check_errors(engine, name, make_target, to_numpy):
    """flags 2, 3 and 0x80000001 on the first, a middle and the last instance, a null context, no fragment table: -1, nothing
    allocated, VELLO_HIP_BUF_SCENE unchanged, the rotation unmoved (the first-allocation trick of instance_parity.check_errors: four
    lanes whose private slots have never been used, so every accepted frame must take the next lane and allocate its slot)."""
    import vello_amd
    from vello_amd import AaConfig, PAINT_DTYPE
    from vello_amd.renderer import instance_array

    w, h, aa = 96, 64, AaConfig.Msaa8
    lib = vello_amd.FragmentLibrary([ip.brush_fragments()["solid"], ip.polygon(4), ip.polygon(7)])
    places = grid(12, w, h)
    good = [(i % 3, places[i]) for i in range(3)]
    lists = [good * 4, good * 3, good * 2, good]
    p = engine._params(w, h, BLACK, aa)
    t = [make_target(w, h) for _ in range(4)]
    # no table yet
    engine.upload_scene(lib.packed, lib.layout, lib.ramps)
    before = engine.scene_allocations()
    inst = instance_array(good)
    pt = np.zeros(3, dtype=PAINT_DTYPE)
    assert _painted_raw(engine, inst, pt.ctypes.data, 3, p, ip._target_ptr(t[0]), w * 4) == -1, "no fragment table"
    assert _painted_raw(engine, inst, None, 3, p, ip._target_ptr(t[0]), w * 4) == -1
    assert engine.scene_allocations() == before
    assert engine._lib.vello_hip_render_instances_painted(None, inst.ctypes.data, pt.ctypes.data, 3, ctypes.byref(p), ip._target_ptr(t[0]), w * 4) == -1, "null context"
    lib.upload(engine)
    try:
        engine.set_frames_in_flight(4)
        for k in range(4):
            n = len(lists[k])
            paints = [word(10 * k + i) if i % 2 == 0 else None for i in range(n)]
            before = engine.scene_allocations()
            render_painted_into(engine, lists[k], paints, w, h, BLACK, aa, t[k])
            assert engine.scene_allocations() == before + 1, f"{name}: frame {k} did not take lane {k}: the lane rotation moved on a refused frame"
            shown = engine.read_buffer("scene", np.uint8, 64)
            inst = instance_array(lists[k])
            for flags in (2, 3, 0x80000001):
                for at in (0, n // 2, n - 1):
                    bad = vello_amd.paint_array(paints)
                    bad[at]["flags"] = flags
                    r = _painted_raw(engine, inst, bad.ctypes.data, n, p, ip._target_ptr(t[k]), w * 4)
                    assert r == -1, (flags, at, r)
                    assert f"instance {at}:".encode() in engine._lib.vello_hip_last_error(engine._h), engine._lib.vello_hip_last_error(engine._h)
                    assert engine.scene_allocations() == before + 1, f"{name}: a refused frame allocated a scene buffer"
            # the refusals of vello_hip_render_instances apply: a fragment out of range, a transform that is not finite, inst == NULL
            ok = vello_amd.paint_array(paints)
            for bad_inst in ([(3, places[0])] + lists[k][1:], lists[k][:-1] + [(0, (float("nan"), 0, 0, 1, 0, 0))]):
                assert _painted_raw(engine, instance_array(bad_inst), ok.ctypes.data, n, p, ip._target_ptr(t[k]), w * 4) == -1
            assert _painted_raw(engine, None, ok.ctypes.data, n, p, ip._target_ptr(t[k]), w * 4) == -1
            assert engine._lib.vello_hip_render_instances_painted(None, None, None, 0, ctypes.byref(p), None, 0) == -1
            assert engine.scene_allocations() == before + 1
            assert np.array_equal(engine.read_buffer("scene", np.uint8, 64), shown), f"{name}: a refused frame changed what VELLO_HIP_BUF_SCENE shows"
        assert engine.sync() == 0
        for k in range(4):
            n = len(lists[k])
            paints = [word(10 * k + i) if i % 2 == 0 else None for i in range(n)]
            packed, plain, layout = compose(lib.packed, lib.layout, lib.fragments, lists[k], paints)
            assert np.array_equal(to_numpy(t[k]), oracle_image(lib, packed, layout, w, h, BLACK, aa)), f"{name}: frame {k} (a refused frame wrote its target?)"
    finally:
        engine.set_frames_in_flight(1)
    # the Python binding: a paint list of another length, a refused flags value
    with np.testing.assert_raises(ValueError):
        engine.render_instances(good, w, h, BLACK, aa, paints=[None])
    bad = np.zeros(3, dtype=PAINT_DTYPE)
    bad["flags"] = (0, 1, 7)
    with np.testing.assert_raises(vello_amd.VelloHipError):
        engine.render_instances(good, w, h, BLACK, aa, paints=bad)
    # upload_scene drops the table and the masks
    engine.upload_scene(lib.packed, lib.layout, lib.ramps)
    with np.testing.assert_raises(vello_amd.VelloHipError):
        engine.render_instances(good, w, h, BLACK, aa, paints=[word(0)] * 3)


# ---------------------------------------------------------------------------------------------------------------
# 13. The struct's mirrors
# ---------------------------------------------------------------------------------------------------------------
def check_struct_mirrors():
    """vello_hip_paint in the header, PaintStruct / PAINT_DTYPE and the Rust struct: names, order, types, 8 bytes, both constants."""
    import os
    import re

    from vello_amd._lib import PaintStruct
    from vello_amd.renderer import PAINT_DTYPE, PAINT_KEEP, PAINT_SOLID

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(root, "include", "vello_hip.h")).read(), flags=re.S)
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(root, "shim", "vello_hip", "src", "ffi.rs")).read())
    body = re.search(r"typedef struct vello_hip_paint \{(.*?)\} vello_hip_paint;", header, flags=re.S).group(1)
    want = []
    for decl in body.split(";"):
        if decl.strip():
            ty, names = decl.split(None, 1)
            assert ty == "uint32_t", ty
            want += [n.strip() for n in names.split(",")]
    assert want == ["flags", "rgba"]
    rbody = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive[^\]]*\]\s*)?pub struct vello_hip_paint \{(.*?)\}", rust, flags=re.S).group(1)
    assert [(f.split(":")[0].replace("pub", "").strip(), f.split(":")[1].strip()) for f in rbody.split(",") if ":" in f] == [(n, "u32") for n in want]
    assert [(n, t) for n, t in PaintStruct._fields_] == [(n, ctypes.c_uint32) for n in want] and ctypes.sizeof(PaintStruct) == 8
    assert PAINT_DTYPE.names == tuple(want) and PAINT_DTYPE.itemsize == 8 and all(PAINT_DTYPE[n] == np.dtype("<u4") for n in want)
    assert [PAINT_DTYPE.fields[n][1] for n in want] == [0, 4]
    enum = re.search(r"enum\s*\{\s*VELLO_HIP_PAINT_KEEP\s*=\s*(\d+)\s*,\s*VELLO_HIP_PAINT_SOLID\s*=\s*(\d+)\s*\}", header)
    assert enum and (int(enum.group(1)), int(enum.group(2))) == (0, 1) == (PAINT_KEEP, PAINT_SOLID)
    for k, v in (("VELLO_HIP_PAINT_KEEP", 0), ("VELLO_HIP_PAINT_SOLID", 1)):
        assert re.search(r"pub const %s: u32 = %d;" % (k, v), rust), k
    assert re.search(r"pub fn vello_hip_render_instances_painted\(", rust)
