"""Hit testing (vello_hip_pick) against a numpy reference and against the oracle's image.  `reference` implements rules 1-4 of the
contract in include/vello_hip.h literally, in float64 and with the sequential clip-stack walk, on the ORACLE's buffers after it ran
the same scene bytes: lines, draw_monoids, path_bboxes and the scene's draw tags.  It never reads the engine's buffers.  The engine's
answers must equal it exactly on every point: the f64 arithmetic is correctly rounded on both sides and the engine's line soup is the
oracle's as a multiset, which the suite already holds.

The checks are shared by tests/test_pick_emu.py (the SIMT-emulated build, where a numpy array stands for device memory) and
tests/test_pick_gpu.py (torch tensors on the MI355X): `dev` is what turns an array into "device memory" and back."""
import ctypes

import numpy as np

from oracle.oracle import Oracle
from tests import instance_parity as ip
from tests import retained_parity as rp
from tests import view_parity

BLACK, WHITE = ip.BLACK, ip.WHITE
NONE = 0xFFFFFFFF
f32, f64 = np.float32, np.float64
FILL_COLOR, BEGIN_CLIP, END_CLIP = 0x44, 0x49, 0x21
PAINT_TAGS = (0x44, 0x114, 0x29C, 0x254, 0x28C, 0x2D4)  # fill colour, linear / radial / sweep gradient, image, blurred rounded rect
E_INVALID, E_CAPACITY = -1, -4


# ---------------------------------------------------------------------------------------------------------------
# The reference
# ---------------------------------------------------------------------------------------------------------------
def run_oracle(packed, layout, w, h, base, aa, lib=None):
    """An Oracle that has rendered the scene bytes: its buffers are what `reference` reads."""
    o = Oracle(capacity_scale=4, auto_grow=True)
    o.set_scene(np.ascontiguousarray(packed, dtype=np.uint8), layout, w, h, base, int(aa))
    if lib is not None:
        o.set_ramps(lib.ramps)
        o.set_image_atlas(lib.resolved.atlas_image())
    o.image = o.render().copy()
    assert o.bump()["failed"] == 0
    return o


def reference(oracle, points, offsets=None):
    """(n, 2) uint32 of (draw_ix, instance_ix).  `offsets`: the numpy-side exclusive prefix of the instances' draw counts ([n + 1]) of a
    frame composed from instances, None for any other frame."""
    cfg = oracle.config()
    width, height = int(cfg[2]), int(cfg[3])
    n_draw, n_paths, draw_tag_base = int(cfg[5]), int(cfg[6]), int(cfg[11])
    packed = oracle._scene_args[0]
    tags = [int(t) for t in packed.view(np.uint32)[draw_tag_base: draw_tag_base + n_draw]]
    n_lines = oracle.bump()["lines"]
    rows = oracle.buffer("lines", np.uint32)[: n_lines * 6].reshape(-1, 6)
    rows = rows[rows[:, 0] < n_paths]
    line_path = rows[:, 0].astype(np.int64)
    xy = np.ascontiguousarray(rows[:, 2:6]).view(f32).astype(f64)
    p0x, p0y, p1x, p1y = xy[:, 0], xy[:, 1], xy[:, 2], xy[:, 3]
    draw_path = [int(v) for v in oracle.buffer("draw_monoids", np.uint32)[: n_draw * 4].reshape(-1, 4)[:, 0]]
    even_odd = (oracle.buffer("path_bboxes", np.uint32)[: n_paths * 6].reshape(-1, 6)[:, 4] & 1) != 0
    pts = np.ascontiguousarray(points, dtype=f32).reshape(-1, 2)
    out = np.full((len(pts), 2), NONE, dtype=np.uint32)
    for k, (x, y) in enumerate(pts):
        qx, qy = f64(x), f64(y)
        if not (np.isfinite(qx) and np.isfinite(qy) and 0.0 <= qx < width and 0.0 <= qy < height):
            continue
        with np.errstate(all="ignore"):
            d = (p1x - p0x) * (qy - p0y) - (qx - p0x) * (p1y - p0y)
            up = (p0y <= qy) & (qy < p1y) & (d < 0.0)
            down = (p1y <= qy) & (qy < p0y) & (d > 0.0)
        winding = np.zeros(n_paths, dtype=np.int64)
        np.add.at(winding, line_path[up], 1)
        np.add.at(winding, line_path[down], -1)
        hit = np.where(even_odd, (winding & 1) != 0, winding != 0)

        def is_hit(i):
            return draw_path[i] < n_paths and bool(hit[draw_path[i]])

        stack, best = [], None
        for i, t in enumerate(tags):
            if t == BEGIN_CLIP:
                stack.append(is_hit(i))
            elif t == END_CLIP:
                if stack:
                    stack.pop()
            elif t in PAINT_TAGS and is_hit(i) and all(stack):
                best = i
        if best is not None:
            out[k, 0] = best
            if offsets is not None and len(offsets) > 1:
                out[k, 1] = int(np.searchsorted(np.asarray(offsets[:-1], dtype=np.int64), best, side="right")) - 1
    return out


def draw_offsets(lib, instances):
    """The exclusive prefix of the instances' draw-object counts: [n + 1], from the fragments' ranges alone."""
    counts = [lib.fragments[int(f)]["draws"][1] - lib.fragments[int(f)]["draws"][0] for f, _ in instances]
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def probe_points(w, h, seed=0, n_random=150, step=4):
    """Pixel centres on a grid, lattice points (integer coordinates: vertex rows and edges of integer geometry) and random points."""
    rng = np.random.default_rng(4000 + seed)
    ys, xs = np.mgrid[0:h:step, 0:w:step]
    centres = np.stack([xs.ravel() + 0.5, ys.ravel() + 0.5], axis=1)
    lattice = np.stack([xs.ravel()[::3], ys.ravel()[::3]], axis=1).astype(f64)
    rnd = np.stack([rng.uniform(-2, w + 2, n_random), rng.uniform(-2, h + 2, n_random)], axis=1)
    return np.concatenate([centres, lattice, rnd]).astype(f32)


def check(engine, oracle, points, name, offsets=None, hand=None, **kw):
    """The engine's answers equal the reference's on every point; `hand`: the draw index known by hand per point (None: not known)."""
    points = np.ascontiguousarray(points, dtype=f32).reshape(-1, 2)
    got = engine.pick(points, **kw)
    want = reference(oracle, points, offsets)
    assert got.shape == want.shape and got.dtype == np.uint32
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, f"{name}: {len(bad)} of {len(points)} points differ, first {points[bad[0]]}: engine {got[bad[0]]}, reference {want[bad[0]]}"
    if hand is not None:
        for k, hk in enumerate(hand):
            if hk is not None:
                assert int(want[k, 0]) == (NONE if hk == "none" else hk), f"{name}: point {points[k]}: reference {want[k]}, known by hand {hk}"
    return got


def resolve(scene):
    packed, layout = scene.resolve()[:2]
    return np.ascontiguousarray(packed, dtype=np.uint8), layout


def scene_frame(engine, scene, w, h, aa=None, base=BLACK):
    """A blocking vello_hip_render frame of a Scene (or of (bytes, layout)) and the oracle of the same bytes."""
    from vello_amd import AaConfig

    aa = AaConfig.Area if aa is None else aa
    packed, layout = scene if isinstance(scene, tuple) else resolve(scene)
    _, bump = engine.render(packed, layout, w, h, base, aa)
    assert bump["failed"] == 0, bump
    return run_oracle(packed, layout, w, h, base, aa), bump


def instance_frame(engine, lib, inst, w, h, aa, paints=None, base=BLACK, upload=True):
    """A blocking instance frame and (oracle of the numpy-composed bytes, numpy offsets)."""
    if upload:
        lib.upload(engine)
    for _ in range(12):
        engine.render_instances(inst, w, h, base, aa, paints=paints)
        r = engine.sync()
        if r != E_CAPACITY:
            break
        assert engine.grow_pools(engine.bump())
    assert r == 0
    packed, layout = rp.compose(lib, inst, paints)
    return run_oracle(packed, layout, w, h, base, aa, lib), draw_offsets(lib, inst)


# ---------------------------------------------------------------------------------------------------------------
# 1. Geometry known by hand
# ---------------------------------------------------------------------------------------------------------------
def _ulp(v, up):
    return float(np.nextafter(f32(v), f32(np.inf if up else -np.inf)))


def check_hand_square(engine, name):
    """Rect(10, 10, 30, 30): the half-open rule on vertex rows, points on edges and vertices, one ulp to either side.  The ray goes
    left: the left edge is outside (the only line it could count is the one it lies on), the right edge inside; the top row is
    inside (p0y <= qy), the bottom row outside (qy < p1y)."""
    from vello_amd import Affine, Color, Fill, Rect, Scene

    s = Scene()
    s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(200, 60, 60), None, Rect(10.0, 10.0, 30.0, 30.0))
    o, bump = scene_frame(engine, s, 64, 48)
    assert bump["lines"] == 4
    cases = [((20.0, 20.0), 0), ((20.0, 10.0), 0), ((20.0, 30.0), "none"), ((20.0, _ulp(10, False)), "none"), ((20.0, _ulp(30, False)), 0),
             ((10.0, 20.0), "none"), ((_ulp(10, True), 20.0), 0), ((_ulp(10, False), 20.0), "none"),
             ((30.0, 20.0), 0), ((_ulp(30, True), 20.0), "none"), ((_ulp(30, False), 20.0), 0),
             ((10.0, 10.0), "none"), ((30.0, 10.0), 0), ((30.0, 30.0), "none"), ((10.0, 30.0), "none"),
             ((_ulp(10, True), 10.0), 0), ((_ulp(30, True), 10.0), "none"), ((30.0, _ulp(30, False)), 0), ((5.5, 20.5), "none"), ((40.5, 20.5), "none")]
    check(engine, o, [p for p, _ in cases], name, hand=[hk for _, hk in cases])
    check(engine, o, probe_points(64, 48, 1), name + "_probe")


def _pentagram(cx, cy, r=14.0):
    from vello_amd import BezPath

    v = [(round(cx + r * np.sin(2 * np.pi * k / 5)), round(cy - r * np.cos(2 * np.pi * k / 5))) for k in range(5)]
    p = BezPath()
    p.move_to((float(v[0][0]), float(v[0][1])))
    for k in (2, 4, 1, 3):
        p.line_to((float(v[k][0]), float(v[k][1])))
    p.close_path()
    return p


def check_hand_shapes(engine, name):
    """A pentagram's centre under both fill rules; strokes (inside the width, in the hole of a closed one); overlapping fills; a
    transparent fill on top."""
    from vello_amd import Affine, BezPath, Color, Fill, Rect, Scene, Stroke

    s = Scene()
    s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(250, 200, 40), None, _pentagram(20, 24))   # 0
    s.fill(Fill.EvenOdd, Affine.IDENTITY, Color.from_rgb8(40, 200, 250), None, _pentagram(52, 24))   # 1
    line = BezPath()
    line.move_to((70.0, 10.0))
    line.line_to((110.0, 10.0))
    s.stroke(Stroke(6.0), Affine.IDENTITY, Color.from_rgb8(90, 250, 90), None, line)                # 2
    s.stroke(Stroke(4.0), Affine.IDENTITY, Color.from_rgb8(250, 90, 250), None, Rect(72.0, 24.0, 112.0, 44.0))  # 3
    s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(200, 60, 60), None, Rect(10.0, 50.0, 40.0, 70.0))     # 4
    s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(60, 60, 200), None, Rect(30.0, 56.0, 60.0, 76.0))     # 5
    s.fill(Fill.NonZero, Affine.IDENTITY, Color(1.0, 1.0, 1.0, 0.0), None, Rect(50.0, 60.0, 80.0, 78.0))        # 6: transparent
    packed, layout = resolve(s)
    assert layout.n_draw_objects == 7
    o, _ = scene_frame(engine, (packed, layout), 128, 80)
    cases = [((20.5, 24.5), 0), ((52.5, 24.5), "none"), ((52.5, 14.5), 1), ((20.5, 14.5), 0),
             ((90.5, 10.5), 2), ((90.5, 12.5), 2), ((90.5, 14.5), "none"), ((90.5, 6.5), "none"),
             ((72.5, 34.5), 3), ((92.5, 34.5), "none"), ((92.5, 24.5), 3), ((112.5, 43.5), 3),
             ((20.5, 60.5), 4), ((35.5, 60.5), 5), ((45.5, 72.5), 5), ((55.5, 65.5), 6), ((70.5, 70.5), 6), ((5.5, 5.5), "none")]
    check(engine, o, [p for p, _ in cases], name, hand=[hk for _, hk in cases])
    check(engine, o, probe_points(128, 80, 2), name + "_probe")


def check_brush_fragments(engine, name, which=("blur", "solid", "linear", "image")):
    """The brush fragments (the blurred rect among them) as an instance frame: paint draws of every kind are candidates."""
    import vello_amd
    from vello_amd import AaConfig

    frs = ip.brush_fragments()
    lib = vello_amd.FragmentLibrary([frs[k] for k in which])
    w, h = 128, 96
    inst = [(k, (2.0, 0.0, 0.0, 2.0, 30.0 + 22.0 * k, 28.0 + 14.0 * k)) for k in range(len(which))]
    o, off = instance_frame(engine, lib, inst, w, h, AaConfig.Area)
    pts = np.concatenate([probe_points(w, h, 3), np.array([[10.5, 14.5]], dtype=f32)])
    got = check(engine, o, pts, name, offsets=off)
    assert got[-1, 0] != NONE and got[-1, 1] == 0, f"{name}: a corner of the blurred rect is {got[-1]}"
    tags = {int(lib.packed.view(np.uint32)[lib.layout.draw_tag_base + d]) for d in range(lib.layout.n_draw_objects)}
    assert 0x2D4 in tags
    assert len(set(got[:, 1].tolist()) - {NONE}) == len(which), f"{name}: not every fragment was hit"


# ---------------------------------------------------------------------------------------------------------------
# 2. Clips
# ---------------------------------------------------------------------------------------------------------------
def check_clip_fragments(engine, name):
    import vello_amd
    from vello_amd import AaConfig

    frs = ip.brush_fragments()
    which = ["clip", "blend", ip._scene_fragments("clip_blend")]
    lib = vello_amd.FragmentLibrary([frs[k] if isinstance(k, str) else k for k in which])
    w, h = 200, 160
    inst = [(0, (2.0, 0.0, 0.0, 2.0, 40.0, 40.0)), (1, (2.0, 0.0, 0.0, 2.0, 100.0, 50.0)), (2, (0.6, 0.0, 0.0, 0.6, 60.0, 70.0)), (0, (1.5, 0.5, -0.5, 1.5, 150.0, 120.0))]
    o, off = instance_frame(engine, lib, inst, w, h, AaConfig.Area)
    got = check(engine, o, probe_points(w, h, 4, step=5), name, offsets=off)
    assert (got[:, 0] != NONE).sum() > 50


def clip_scene():
    """Nested clips -- outer missed / inner hit and the other way round --, a draw after the EndClip of a missed clip, an even-odd clip."""
    from vello_amd import Affine, BezPath, Color, Fill, Rect, Scene

    s = Scene()
    full = Rect(0.0, 0.0, 120.0, 90.0)

    def fill(r, k):
        s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(40 + 20 * k, 250 - 20 * k, 90), None, r)

    s.push_clip_layer(Fill.NonZero, Affine.IDENTITY, Rect(10.0, 10.0, 40.0, 40.0))    # 0 outer
    s.push_clip_layer(Fill.NonZero, Affine.IDENTITY, Rect(30.0, 30.0, 60.0, 60.0))    # 1 inner
    fill(full, 0)                                                                      # 2: visible in [30, 40)^2 only
    s.pop_layer()                                                                      # 3
    fill(Rect(0.0, 0.0, 20.0, 90.0), 1)                                                # 4: under the outer clip only
    s.pop_layer()                                                                      # 5
    fill(Rect(50.0, 50.0, 70.0, 70.0), 2)                                              # 6: after the EndClips
    two = BezPath()                                                                    # an even-odd clip: two nested squares
    for a, b in ((70.0, 10.0), (80.0, 20.0)):
        c = 180.0 - a
        two.move_to((a, b))
        two.line_to((c, b))
        two.line_to((c, 60.0 - b))
        two.line_to((a, 60.0 - b))
        two.close_path()
    s.push_clip_layer(Fill.EvenOdd, Affine.IDENTITY, two)                              # 7
    fill(full, 3)                                                                      # 8: the ring between the squares
    s.pop_layer()                                                                      # 9
    return s


def check_clip_scene(engine, name):
    packed, layout = resolve(clip_scene())
    assert layout.n_draw_objects == 10 and layout.n_clips == 6
    o, _ = scene_frame(engine, (packed, layout), 120, 90)
    cases = [((35.5, 35.5), 2), ((15.5, 15.5), 4), ((25.5, 25.5), "none"), ((45.5, 45.5), "none"), ((55.5, 55.5), 6), ((5.5, 80.5), "none"),
             ((75.5, 15.5), 8), ((90.5, 30.5), "none"), ((105.5, 45.5), 8), ((65.5, 5.5), "none")]
    check(engine, o, [p for p, _ in cases], name, hand=[hk for _, hk in cases])
    check(engine, o, probe_points(120, 90, 5), name + "_probe")


# ---------------------------------------------------------------------------------------------------------------
# 3. Against the oracle's image
# ---------------------------------------------------------------------------------------------------------------
def image_scene():
    """Opaque, uniquely coloured fills and strokes, every feature at least 2 px thick, overlapping; 128 x 96."""
    from vello_amd import Affine, Circle, Color, Fill, Rect, Scene, Stroke

    s = Scene()
    cols = []

    def col():
        k = len(cols)
        c = (40 + 50 * (k % 4), 60 + 40 * ((k // 2) % 4), 250 - 45 * (k % 5))
        cols.append(c)
        return Color.from_rgb8(*c)

    s.fill(Fill.NonZero, Affine.IDENTITY, col(), None, Rect(6.0, 6.0, 70.0, 50.0))
    s.fill(Fill.NonZero, Affine.IDENTITY, col(), None, Circle((80.0, 40.0), 26.0))
    s.fill(Fill.NonZero, Affine.rotate(0.3), col(), None, Rect(40.0, 30.0, 90.0, 60.0))
    s.stroke(Stroke(5.0), Affine.IDENTITY, col(), None, Rect(14.0, 20.0, 110.0, 84.0))
    s.stroke(Stroke(4.0), Affine.IDENTITY, col(), None, Circle((40.0, 60.0), 18.0))
    s.fill(Fill.EvenOdd, Affine.IDENTITY, col(), None, _pentagram(96, 70, 20.0))
    assert len(set(cols)) == len(cols)
    return s, cols


def settled_pixels(img, colour):
    """Pixels that show `colour` (r, g, b) together with their eight neighbours."""
    m = (img[..., 0] == colour[0]) & (img[..., 1] == colour[1]) & (img[..., 2] == colour[2])
    out = np.zeros_like(m)
    out[1:-1, 1:-1] = m[1:-1, 1:-1]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out[1:-1, 1:-1] &= m[1 + dy: m.shape[0] - 1 + dy, 1 + dx: m.shape[1] - 1 + dx]
    return out


def image_expectation(img, cols, base=(0, 0, 0)):
    """(points, expected draw index or NONE) for every settled pixel and every pixel settled on the base colour."""
    pts, want = [], []
    for k, c in list(enumerate(cols)) + [(NONE, base)]:
        ys, xs = np.nonzero(settled_pixels(img, c))
        pts.append(np.stack([xs + 0.5, ys + 0.5], axis=1))
        want.append(np.full(len(xs), k, dtype=np.uint32))
    return np.concatenate(pts).astype(f32), np.concatenate(want)


def check_image(engine, name, pick=None):
    """Independent of `reference`: where the oracle's image is settled on draw k's colour the pick is k, where it is settled on the
    base colour the pick is NONE.  `pick`: what answers in the engine's place (the reference itself, to hold it to the same check)."""
    from vello_amd import AaConfig

    scene, cols = image_scene()
    w, h = 128, 96
    packed, layout = resolve(scene)
    if engine is not None:
        o, _ = scene_frame(engine, (packed, layout), w, h, AaConfig.Area)
    else:
        o = run_oracle(packed, layout, w, h, BLACK, AaConfig.Area)
    pts, want = image_expectation(o.image, cols)
    assert len(pts) * 2 >= w * h, f"{name}: only {len(pts)} of {w * h} pixels are settled"
    assert all((want == k).any() for k in range(len(cols))), f"{name}: a draw has no settled pixel"
    if pick is not None:
        got = pick(o, pts)
    else:  # (VELLO_HIP_PICK_MAX_POINTS to a call)
        got = np.concatenate([engine.pick(pts[k: k + 4096]) for k in range(0, len(pts), 4096)])
    bad = np.nonzero(got[:, 0] != want)[0]
    assert len(bad) == 0, f"{name}: {len(bad)} settled pixels differ, first {pts[bad[0]]}: pick {got[bad[0]]}, image says {want[bad[0]]}"
    assert (got[:, 1] == NONE).all()


# ---------------------------------------------------------------------------------------------------------------
# 4. Kernel shapes
# ---------------------------------------------------------------------------------------------------------------
def raw_scene(tags, path_data, n_draws):
    """A packed scene written out by hand: one TRANSFORM (identity), one non-zero fill STYLE, the given path tags, n_draws FILL_COLOR
    draws."""
    from vello_amd import Layout

    t = np.zeros(1024, dtype=np.uint8)
    t[: 2 + len(tags)] = [0x20, 0x40] + list(tags)
    pd = np.asarray(path_data, dtype=f32).view(np.uint32)
    dt = np.full(n_draws, FILL_COLOR, dtype=np.uint32)
    dd = np.full(n_draws, 0xFF2060F0, dtype=np.uint32)
    xf = np.array([1, 0, 0, 1, 0, 0], dtype=f32).view(np.uint32)
    st = np.array([0x40000000, 0], dtype=np.uint32)
    packed = np.concatenate([t.view(np.uint32), pd, dt, dd, xf, st]).view(np.uint8)
    b = 256 + len(pd)
    layout = Layout(n_draw_objects=n_draws, n_paths=n_draws, n_clips=0, bin_data_start=n_draws, path_tag_base=0, path_data_base=256, draw_tag_base=b,
                    draw_data_base=b + n_draws, transform_base=b + 2 * n_draws, style_base=b + 2 * n_draws + 6)
    return packed, layout


def check_soup_shapes(engine, name):
    """0 lines (empty paths), 1 line, and one below / at / one above the line pass's lines per workgroup."""
    import vello_amd
    from vello_amd import AaConfig

    chunk = engine.pick_constants()["lines_per_workgroup"]
    w, h = 64, 48
    pts = probe_points(w, h, 6, n_random=40, step=6)
    o, bump = scene_frame(engine, raw_scene([0x10, 0x10], [], 2), w, h)
    assert bump["lines"] == 0
    assert (check(engine, o, pts, name + "_0")[:, 0] == NONE).all()
    # one upward line from (10, 10) to (10, 30): LINETO | F32 | SUBPATH_END with its two points, then the PATH marker
    o, bump = scene_frame(engine, raw_scene([0x0D, 0x10], [10.0, 10.0, 10.0, 30.0], 1), w, h)
    assert bump["lines"] == 1
    got = check(engine, o, np.concatenate([pts, np.array([[20.5, 20.5], [5.5, 20.5], [20.5, 30.0], [20.5, 10.0]], dtype=f32)]), name + "_1")
    assert got[-4:, 0].tolist() == [0, NONE, NONE, 0], got[-4:]
    for k in (chunk - 1, chunk, chunk + 1):
        lib = vello_amd.FragmentLibrary([ip.polygon(k, r=20.0)])
        o, off = instance_frame(engine, lib, [(0, (1.0, 0.0, 0.0, 1.0, 32.0, 24.0))], w, h, AaConfig.Area)
        assert o.bump()["lines"] == k and engine.bump()["lines"] == k
        got = check(engine, o, pts, f"{name}_{k}", offsets=off)
        assert (got[:, 0] == 0).any() and (got[:, 0] == NONE).any()


def many_draws(n, clip_at=None, pop_at=None):
    """n draw objects: small squares on a 16 x 12 grid of a 128 x 96 target (3 px apart, 5 px wide: neighbours overlap); with
    clip_at / pop_at a clip layer that the grid misses -- Rect(120, 88, 127, 95) holds no square's centre -- opens and closes there."""
    from vello_amd import Affine, Color, Fill, Rect, Scene

    s = Scene()
    k = 0
    for i in range(n):
        if i == clip_at:
            s.push_clip_layer(Fill.NonZero, Affine.IDENTITY, Rect(120.0, 88.0, 127.0, 95.0))
        elif i == pop_at:
            s.pop_layer()
        else:
            x, y = 2.0 + 7.0 * (k % 16), 2.0 + 7.0 * ((k // 16) % 12)
            s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(40 + k % 200, 250 - k % 200, 90), None, Rect(x, y, x + 9.0, y + 9.0))
            k += 1
    return s


def check_draw_shapes(engine, name):
    """D = 0, 1, one below / at / one above the resolve pass's step; three steps with a missed BeginClip in the first whose EndClip
    lies in the third: the carry across steps and a candidate in the last step."""
    step = engine.pick_constants()["draws_per_step"]
    w, h = 128, 96
    pts = probe_points(w, h, 7, n_random=30, step=7)
    for d in (0, 1, step - 1, step, step + 1):
        packed, layout = resolve(many_draws(d))
        assert layout.n_draw_objects == d
        o, _ = scene_frame(engine, (packed, layout), w, h)
        got = check(engine, o, pts, f"{name}_{d}")
        assert (got[:, 0] != NONE).any() == (d > 0)
    d = 2 * step + 40
    clip_at, pop_at = 5, 2 * step + 6
    packed, layout = resolve(many_draws(d, clip_at, pop_at))
    assert layout.n_draw_objects == d and layout.n_clips == 2 and pop_at // step == 2 and clip_at // step == 0
    o, _ = scene_frame(engine, (packed, layout), w, h)
    got = check(engine, o, pts, f"{name}_carry")
    seen = got[:, 0][got[:, 0] != NONE]
    assert len(seen) and ((seen < clip_at) | (seen > pop_at)).all(), f"{name}: a draw under the missed clip was picked"
    assert (seen > pop_at).any(), f"{name}: no candidate in the last step"
    # the same point with and without the clip: under it the squares of the first two steps are gone
    o2, _ = scene_frame(engine, resolve(many_draws(d)), w, h)
    both = check(engine, o2, pts, f"{name}_no_clip")
    assert (both[:, 0] != got[:, 0]).any()


def check_query_counts(engine, name):
    """n = 0, 1, 63, 64, 65; a count that spans batches (the small-batch debug flag); VELLO_HIP_PICK_MAX_POINTS and one more."""
    import vello_amd
    from vello_amd.renderer import PICK_MAX_POINTS

    w, h = 128, 96
    o, _ = scene_frame(engine, many_draws(40), w, h)
    rng = np.random.default_rng(12)
    pts = np.stack([rng.uniform(0, w, PICK_MAX_POINTS + 1), rng.uniform(0, h, PICK_MAX_POINTS + 1)], axis=1).astype(f32)
    for n in (0, 1, 63, 64, 65):
        got = check(engine, o, pts[:n], f"{name}_n{n}")
        assert got.shape == (n, 2)
    small = engine.pick_constants()["small_batch"]
    n = 2 * small + 1
    whole = check(engine, o, pts[:n], f"{name}_one_batch")
    try:
        engine.set_debug_flags(pick_small_batches=True)
        cut = check(engine, o, pts[:n], f"{name}_three_batches")
    finally:
        engine.set_debug_flags()
    assert np.array_equal(whole, cut) and (whole[:, 0] != NONE).any()
    check(engine, o, pts[:PICK_MAX_POINTS], f"{name}_max")
    out = np.full((PICK_MAX_POINTS + 1, 2), 0xA5A5A5A5, dtype=np.uint32)
    with np.testing.assert_raises(vello_amd.VelloHipError) as e:
        engine.pick(pts, out=out)
    assert e.exception.code == E_INVALID and (out == 0xA5A5A5A5).all()


# ---------------------------------------------------------------------------------------------------------------
# 5. Instances
# ---------------------------------------------------------------------------------------------------------------
def instance_library():
    """Polygons, a fragment of three draws, and an EMPTY fragment."""
    import vello_amd
    from vello_amd import Affine, Color, Fill, Rect, Scene

    three = Scene()
    for k in range(3):
        three.fill(Fill.NonZero, Affine.translate(5.0 * k, 3.0 * k), Color.from_rgb8(250 - 70 * k, 80 + 60 * k, 60), None, Rect(-6.0, -4.0, 6.0, 4.0))
    lib = vello_amd.FragmentLibrary([ip.polygon(5), ip.polygon(7), three])
    lib.three = 2
    lib.empty = len(lib.fragments)
    lib.fragments.append(dict(ip.EMPTY))
    return lib


def instance_list(lib, w, h, seed=0):
    rng = np.random.default_rng(70 + seed)
    frags = [0, lib.empty, lib.empty, lib.three, lib.empty, 1, lib.three, 0, lib.empty, 1, 0, lib.three, lib.empty]
    return [(f, t) for f, (_, t) in zip(frags, ip.scatter(rng, len(frags), 1, w, h, scale=(0.8, 1.6)))]


def check_instances(engine, name, dev):
    """render_instances and _painted frames over a library with EMPTY fragments between drawn ones and a fragment of three draws; a
    retained list under turned poses from host and device memory, and under a view; render_frame / render_resident frames."""
    from vello_amd import AaConfig, Affine

    lib = instance_library()
    w, h, aa = 128, 96, AaConfig.Msaa8
    inst = instance_list(lib, w, h)
    off = draw_offsets(lib, inst)
    assert len(set(off.tolist())) < len(off), "no repeated offset"
    pts = probe_points(w, h, 8, step=3)
    o, off = instance_frame(engine, lib, inst, w, h, aa)
    got = check(engine, o, pts, name + "_instances", offsets=off)
    owners = set(got[:, 1].tolist()) - {NONE}
    assert owners and all(lib.fragments[inst[i][0]] != ip.EMPTY for i in owners), f"{name}: an empty instance owns a draw"
    three = [i for i, (f, _) in enumerate(inst) if f == lib.three]
    assert any(len(set(got[got[:, 1] == i, 0].tolist())) > 1 for i in three), f"{name}: no instance of three draws was hit on two of them"
    paints = rp.some_paints(len(inst))
    o, off = instance_frame(engine, lib, inst, w, h, aa, paints=paints, upload=False)
    assert np.array_equal(check(engine, o, pts, name + "_painted", offsets=off), got), f"{name}: paints changed the pick"
    # retained, rest poses and turned poses from host and device memory
    engine.retain_instances(inst)
    poses = rp.turned(inst, w, h, 3)
    rp.frame(engine, w, h, BLACK, aa, None, "rest")
    rest = check(engine, o, pts, name + "_retained_rest", offsets=off)
    assert np.array_equal(rest, got)
    shown = rp.posed(inst, poses)
    o_t = run_oracle(*rp.compose(lib, shown), w, h, BLACK, aa, lib)
    for source in ("host", "device"):
        rp.frame(engine, w, h, BLACK, aa, poses, source, dev.to_device)
        moved = check(engine, o_t, pts, f"{name}_retained_{source}", offsets=off)
        assert (moved != rest).any(), f"{name}: the pick ignored the {source} poses"
    view = Affine.translate(9.0, -6.0) * Affine.rotate(0.2) * Affine.scale(1.2)
    try:
        engine.set_view_transform(view)
        rp.frame(engine, w, h, BLACK, aa, poses, "device", dev.to_device)
    finally:
        engine.set_view_transform(None)
    packed, layout = rp.compose(lib, shown)
    o_v = run_oracle(view_parity.compose(packed, layout, view), layout, w, h, BLACK, aa, lib)
    viewed = check(engine, o_v, pts, name + "_retained_view", offsets=off)
    assert (viewed != moved).any()
    # frames that were not composed from instances name no instance
    engine.render_resident(w, h, BLACK, aa)
    assert engine.sync() == 0
    o_lib = run_oracle(lib.packed, lib.layout, w, h, BLACK, aa, lib)
    res = check(engine, o_lib, probe_points(w, h, 9, step=2)[:600], name + "_resident")
    assert (res[:, 1] == NONE).all() and (res[:, 0] != NONE).any()
    view_parity.render_frame_into(engine, packed, layout, w, h, BLACK, aa, dev.target(w, h))
    fr = check(engine, o_t, pts, name + "_render_frame")
    assert (fr[:, 1] == NONE).all() and np.array_equal(fr[:, 0], moved[:, 0])
    assert engine.sync() == 0


# ---------------------------------------------------------------------------------------------------------------
# 6. Which frame
# ---------------------------------------------------------------------------------------------------------------
def check_which_frame(engine, name, dev):
    """Four frames in flight under four pose sets: the pick answers for the fourth; afterwards sync is 0, every target holds its own
    image, a following frame is right and no scene buffer was allocated."""
    from vello_amd import AaConfig

    lib = instance_library()
    lib.upload(engine)
    w, h, aa = 128, 96, AaConfig.Msaa8
    inst = instance_list(lib, w, h, 1)
    off = draw_offsets(lib, inst)
    engine.retain_instances(inst)
    sets = [rp.turned(inst, w, h, 20 + k) for k in range(4)]
    oracles = [run_oracle(*rp.compose(lib, rp.posed(inst, p)), w, h, BLACK, aa, lib) for p in sets]
    pts = probe_points(w, h, 10, step=3)
    refs = [reference(o, pts, off) for o in oracles]
    assert all((refs[3] != r).any() for r in refs[:3])
    keep = []
    try:
        engine.set_frames_in_flight(4)
        for k in range(4):  # (every lane has held the list: nothing is allocated from here on)
            rp.render_retained(engine, w, h, BLACK, aa, sets[k], "host")
        assert engine.sync() == 0
        before = engine.scene_allocations()
        t = [dev.target(w, h) for _ in range(5)]
        for k in range(4):
            rp.render_retained(engine, w, h, BLACK, aa, sets[k], ("host", "device")[k % 2], dev.to_device, out=t[k], keep=keep)
        got = engine.pick(pts)
        assert np.array_equal(got, refs[3]), f"{name}: the pick does not answer for the frame submitted last"
        assert engine.sync() == 0
        for k in range(4):
            assert np.array_equal(dev.to_numpy(t[k]), oracles[k].image), f"{name}: target {k} after the pick"
        rp.render_retained(engine, w, h, BLACK, aa, sets[1], "device", dev.to_device, out=t[4], keep=keep)
        assert np.array_equal(engine.pick(pts), refs[1]), f"{name}: the pick after the following frame"
        assert engine.sync() == 0
        assert np.array_equal(dev.to_numpy(t[4]), oracles[1].image), f"{name}: the frame after a pick"
        assert engine.scene_allocations() == before, f"{name}: a pick allocated a scene buffer"
    finally:
        engine.set_frames_in_flight(1)


# ---------------------------------------------------------------------------------------------------------------
# 7. Sources and sinks
# ---------------------------------------------------------------------------------------------------------------
def check_sources(engine, name, dev):
    """Host points to a host result and to a caller's array; device points to a device result; bad points among good ones; viewport
    culling on and off."""
    from vello_amd import AaConfig

    w, h = 120, 90
    packed, layout = resolve(clip_scene())
    o, _ = scene_frame(engine, (packed, layout), w, h, AaConfig.Msaa8)
    pts = probe_points(w, h, 11, step=5)
    want = reference(o, pts)
    assert np.array_equal(engine.pick(pts), want)
    out = np.zeros((len(pts), 2), dtype=np.uint32)
    assert engine.pick(pts, out=out) is out and np.array_equal(out, want)
    d_pts, d_out = dev.to_device(pts), dev.result(len(pts))
    kw = {"points_is_device": True} if isinstance(d_pts, np.ndarray) else {}
    r = engine.pick(d_pts, out=d_out, **kw)
    assert r is d_out and np.array_equal(dev.result_numpy(d_out), want), f"{name}: device points to a device result"
    assert np.array_equal(engine.pick(d_pts, **kw), want), f"{name}: device points to a host result"
    assert np.array_equal(dev.result_numpy(engine.pick(pts, out=dev.result(len(pts)))), want), f"{name}: host points to a device result"
    # points that always miss, mixed among good ones
    mixed = pts.copy()
    bad = [(-0.5, 10.0), (10.0, -0.5), (float(w), 10.0), (10.0, float(h)), (float("nan"), 10.0), (10.0, float("nan")), (float("inf"), 10.0),
           (10.0, float("-inf")), (float("-inf"), float("inf")), (1e30, 1e30)]
    where = np.arange(len(bad)) * 7 + 3
    mixed[where] = bad
    for p, k2 in ((mixed, {}), (dev.to_device(mixed), kw)):
        got = engine.pick(p, **k2)
        assert (got[where] == NONE).all(), f"{name}: a point that always misses was hit"
        keep = np.ones(len(pts), dtype=bool)
        keep[where] = False
        assert np.array_equal(got[keep], want[keep]), f"{name}: a bad point changed its neighbours' answers"
        assert np.array_equal(got, reference(o, mixed))
    # viewport culling: identical answers (a scene that reaches past every side of the target)
    from vello_amd import Affine

    view = Affine.translate(-30.0, -25.0) * Affine.scale(2.2)
    moved = view_parity.compose(packed, layout, view)
    o_v = run_oracle(moved, layout, w, h, BLACK, AaConfig.Msaa8)
    engine.upload_scene(packed, layout)
    answers, lines = [], []
    try:
        engine.set_view_transform(view)
        for cull in (False, True):
            engine.set_viewport_cull(cull)
            engine.render_resident(w, h, BLACK, AaConfig.Msaa8)
            assert engine.sync() == 0
            lines.append(engine.bump()["lines"])
            answers.append(check(engine, o_v, pts, f"{name}_cull{int(cull)}"))
    finally:
        engine.set_view_transform(None)
        engine.set_viewport_cull(False)
    assert lines[1] < lines[0], f"{name}: culling dropped no line"
    assert np.array_equal(answers[0], answers[1])


# ---------------------------------------------------------------------------------------------------------------
# 8. Refusals and failed frames
# ---------------------------------------------------------------------------------------------------------------
def _ptr(x):
    if x is None:
        return None
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr() if hasattr(x, "data_ptr") else int(x)


def raw_pick(engine, points, n, points_is_device, src_stream, out, out_is_device):
    return engine._lib.vello_hip_pick(engine._h, _ptr(points), n, int(points_is_device), ctypes.c_void_p(src_stream) if src_stream else None, _ptr(out),
                                      int(out_is_device))


def check_refusals(make_engine, name, dev, host_memory=None):
    """Every VELLO_HIP_E_INVALID of the entry point, each leaving `out` untouched and naming its rule."""
    from vello_amd import AaConfig
    from vello_amd.renderer import PICK_MAX_POINTS

    engine = make_engine(None)
    w, h = 64, 48
    pts = probe_points(w, h, 13, n_random=5, step=16)
    n = len(pts)
    PAT = 0x5A5A5A5A
    out = np.full((PICK_MAX_POINTS + 1, 2), PAT, dtype=np.uint32)
    d_pts, d_out = dev.to_device(pts), dev.result(n, PAT)

    def last():
        return engine._lib.vello_hip_last_error(engine._h)

    def untouched():
        return (out == PAT).all() and (dev.result_numpy(d_out) == PAT).all()

    # no frame was ever rendered
    assert raw_pick(engine, pts, n, 0, None, out, 0) == E_INVALID and b"no frame" in last() and untouched()
    assert raw_pick(engine, pts, 0, 0, None, out, 0) == 0 and untouched(), f"{name}: n == 0"
    o, _ = scene_frame(engine, many_draws(12), w, h, AaConfig.Msaa8)
    assert raw_pick(engine, pts, 0, 0, None, out, 0) == 0 and raw_pick(engine, None, 0, 0, None, None, 0) == 0 and untouched(), f"{name}: n == 0"
    assert raw_pick(engine, None, n, 0, None, out, 0) == E_INVALID and b"points" in last()
    assert raw_pick(engine, pts, n, 0, None, None, 0) == E_INVALID and b"out" in last()
    assert engine._lib.vello_hip_pick(None, _ptr(pts), n, 0, None, _ptr(out), 0) == E_INVALID
    big = np.zeros((PICK_MAX_POINTS + 1, 2), dtype=f32)
    assert raw_pick(engine, big, PICK_MAX_POINTS + 1, 0, None, out, 0) == E_INVALID and b"MAX_POINTS" in last()
    assert raw_pick(engine, pts, n, 0, engine.stream() or 1, out, 0) == E_INVALID and b"src_stream" in last()
    assert raw_pick(engine, _ptr(d_pts) + 2, n - 1, 1, None, out, 0) == E_INVALID and b"multiple of 4" in last()
    assert raw_pick(engine, pts, n - 1, 0, None, _ptr(d_out) + 2, 1) == E_INVALID and b"multiple of 4" in last()
    if host_memory is not None:  # (GPU build: host memory handed in as device memory, pageable and pinned)
        for kind, mem in host_memory(pts).items():
            assert raw_pick(engine, mem, n, 1, None, out, 0) == E_INVALID and b"not device memory" in last(), f"{name}: {kind} points"
            assert raw_pick(engine, pts, n, 0, None, mem, 1) == E_INVALID and b"not device memory" in last(), f"{name}: {kind} result"
    assert untouched(), f"{name}: a refused call wrote its result"
    # ... and the accepted call still answers
    assert raw_pick(engine, d_pts, n, 1, None, d_out, 1) == 0
    assert np.array_equal(dev.result_numpy(d_out), reference(o, pts))
    assert engine.sync() == 0


def check_failed_frame(make_engine, name, dev):
    """From tiny pools, a frame that ends in E_CAPACITY: the pick returns E_CAPACITY and writes nothing; after grow_pools and a good
    frame it answers."""
    import vello_amd
    from vello_amd import AaConfig

    w, h, aa = 128, 96, AaConfig.Msaa8
    engine = make_engine(dict(lines=64, seg_counts=64, segments=64, tiles=256))
    lib = vello_amd.FragmentLibrary([ip.polygon(9), ip.polygon(14)])
    lib.upload(engine)
    inst = ip.scatter(np.random.default_rng(4), 30, 2, w, h, scale=(1.0, 2.5))
    pts = probe_points(w, h, 14, step=6)
    out = np.full((len(pts), 2), 0x5A5A5A5A, dtype=np.uint32)
    engine.render_instances(inst, w, h, BLACK, aa)
    with np.testing.assert_raises(vello_amd.VelloHipError) as e:
        engine.pick(pts, out=out)
    assert e.exception.code == E_CAPACITY, f"{name}: {e.exception}"
    assert (out == 0x5A5A5A5A).all(), f"{name}: the pick of a failed frame wrote its result"
    assert engine.sync() == E_CAPACITY, f"{name}: the pick hid the frame's failure from sync"
    rounds = 0
    while True:
        assert engine.grow_pools(engine.bump())
        rounds += 1
        engine.render_instances(inst, w, h, BLACK, aa)
        r = engine.sync()
        if r != E_CAPACITY:
            break
        assert rounds < 12
    assert r == 0
    o = run_oracle(*rp.compose(lib, inst), w, h, BLACK, aa, lib)
    got = check(engine, o, pts, name, offsets=draw_offsets(lib, inst), out=out)
    assert got is out and (got[:, 0] != NONE).any()
