"""Marquee selection (vello_hip_pick_rect) against a numpy reference and against the oracle's image.  `reference` implements rules
0-3 of the contract in include/vello_hip.h literally -- rule 0 in float32, the line tests in float64, the sequential clip-stack walk --
on the ORACLE's buffers after it ran the same scene bytes: lines, draw_monoids, path_bboxes and the scene's draw tags, and the
numpy-side draw offsets of an instance frame.  It never reads the engine's buffers.  The engine must equal it exactly: every draw
word, every instance word, all four counts.  There is no tolerance: the f64 arithmetic is correctly rounded on both sides and the
engine's line soup is the oracle's as a multiset, which the suite already holds.

The checks are shared by tests/test_pick_rect_emu.py (the SIMT-emulated build, where a numpy array stands for device memory) and
tests/test_pick_rect_gpu.py (torch tensors on the MI355X): `dev` is what turns an array into "device memory" and back."""
import ctypes

import numpy as np

from tests import instance_parity as ip
from tests import pick_parity as pk
from tests import retained_parity as rp
from tests import view_parity

BLACK = pk.BLACK
f32, f64 = np.float32, np.float64
TOUCHED, ENCLOSED = 1, 2
E_INVALID, E_CAPACITY = pk.E_INVALID, pk.E_CAPACITY
INF, NAN = float("inf"), float("nan")


# ---------------------------------------------------------------------------------------------------------------
# The reference
# ---------------------------------------------------------------------------------------------------------------
def region(rect, w, h):
    """Rule 0, every step in float32: (x0', y0', x1', y1', cx, cy), or None for an empty R'."""
    r = [f32(v) for v in rect]
    if any(np.isnan(v) for v in r):
        return None
    out = []
    for a, b, size in ((r[0], r[2], f32(w)), (r[1], r[3], f32(h))):
        lo, hi = (a, b) if a < b else (b, a)
        out.append((lo if lo > f32(0) else f32(0), hi if hi < size else size))
    (x0, x1), (y0, y1) = out
    if not (x0 < x1 and y0 < y1):
        return None
    c = []
    for lo, hi in ((x0, x1), (y0, y1)):
        m = f32(lo + f32(f32(hi - lo) * f32(0.5)))
        c.append(m if m < hi else lo)
    return x0, y0, x1, y1, c[0], c[1]


def _parsed(oracle):
    """What the reference reads of an oracle, parsed once."""
    if getattr(oracle, "_region_parsed", None) is None:
        cfg = oracle.config()
        n_draw, n_paths, draw_tag_base = int(cfg[5]), int(cfg[6]), int(cfg[11])
        packed = oracle._scene_args[0]
        tags = [int(t) for t in packed.view(np.uint32)[draw_tag_base: draw_tag_base + n_draw]]
        n_lines = oracle.bump()["lines"]
        rows = oracle.buffer("lines", np.uint32)[: n_lines * 6].reshape(-1, 6)
        rows = rows[rows[:, 0] < n_paths]
        xy32 = np.ascontiguousarray(rows[:, 2:6]).view(f32)
        draw_path = [int(v) for v in oracle.buffer("draw_monoids", np.uint32)[: n_draw * 4].reshape(-1, 4)[:, 0]]
        boxes = oracle.buffer("path_bboxes", np.uint32)[: n_paths * 6].reshape(-1, 6).copy()
        oracle._region_parsed = dict(width=int(cfg[2]), height=int(cfg[3]), n_draw=n_draw, n_paths=n_paths, tags=tags, line_path=rows[:, 0].astype(np.int64),
                                     xy32=xy32.copy(), xy=xy32.astype(f64), draw_path=draw_path, even_odd=(boxes[:, 4] & 1) != 0,
                                     box=np.ascontiguousarray(boxes[:, 0:4]).view(np.int32).astype(np.int64))
    return oracle._region_parsed


def line_meets(oracle, rect):
    """Rule 1's MEETS per counted line of the oracle's soup (a bool per line), and the lines' paths."""
    p = _parsed(oracle)
    reg = region(rect, p["width"], p["height"])
    if reg is None:
        return np.zeros(len(p["line_path"]), dtype=bool), p["line_path"]
    x0, y0, x1, y1 = reg[:4]
    a = p["xy32"]
    with np.errstate(all="ignore"):  # (np.minimum / np.maximum hand a NaN on: such a line fails the box test)
        box = ((np.minimum(a[:, 0], a[:, 2]) < x1) & (np.maximum(a[:, 0], a[:, 2]) > x0) & (np.minimum(a[:, 1], a[:, 3]) < y1) &
               (np.maximum(a[:, 1], a[:, 3]) > y0))
        p0x, p0y, p1x, p1y = (p["xy"][:, k] for k in range(4))
        ds = [(p1x - p0x) * (f64(qy) - p0y) - (f64(qx) - p0x) * (p1y - p0y) for qx in (x0, x1) for qy in (y0, y1)]
        all_pos = (ds[0] > 0.0) & (ds[1] > 0.0) & (ds[2] > 0.0) & (ds[3] > 0.0)
        all_neg = (ds[0] < 0.0) & (ds[1] < 0.0) & (ds[2] < 0.0) & (ds[3] < 0.0)
    return box & ~all_pos & ~all_neg, p["line_path"]


def reference(oracle, rect, offsets=None):
    """(draw words [n_draw] uint32, instance words [n] uint32 or None, the four counts).  `offsets`: the numpy-side exclusive prefix of
    the instances' draw counts ([n + 1]) of a frame composed from instances, None for any other frame."""
    p = _parsed(oracle)
    n_draw, n_paths, tags, draw_path = p["n_draw"], p["n_paths"], p["tags"], p["draw_path"]
    draws = np.zeros(n_draw, dtype=np.uint32)
    n_inst = 0 if offsets is None else len(offsets) - 1
    insts = np.zeros(n_inst, dtype=np.uint32) if n_inst else None
    reg = region(rect, p["width"], p["height"])
    if reg is not None:
        x0, y0, x1, y1, cx, cy = (f64(v) for v in reg)
        m, line_path = line_meets(oracle, rect)
        meets = np.zeros(n_paths, dtype=bool)
        meets[line_path[m]] = True
        p0x, p0y, p1x, p1y = (p["xy"][:, k] for k in range(4))
        with np.errstate(all="ignore"):
            d = (p1x - p0x) * (cy - p0y) - (cx - p0x) * (p1y - p0y)
            up = (p0y <= cy) & (cy < p1y) & (d < 0.0)
            down = (p1y <= cy) & (cy < p0y) & (d > 0.0)
        winding = np.zeros(n_paths, dtype=np.int64)
        np.add.at(winding, line_path[up], 1)
        np.add.at(winding, line_path[down], -1)
        touch = meets | np.where(p["even_odd"], (winding & 1) != 0, winding != 0)
        b = p["box"]
        boxed = (x0 <= b[:, 0]) & (b[:, 2] <= x1) & (y0 <= b[:, 1]) & (b[:, 3] <= y1)
        nonempty = (b[:, 0] < b[:, 2]) & (b[:, 1] < b[:, 3])

        def of(table, i):
            return draw_path[i] < n_paths and bool(table[draw_path[i]])

        stack = []
        for i, t in enumerate(tags):
            if t == pk.BEGIN_CLIP:
                stack.append(of(touch, i))
            elif t == pk.END_CLIP:
                if stack:
                    stack.pop()
            elif t in pk.PAINT_TAGS and of(touch, i) and all(stack):
                draws[i] = TOUCHED | (ENCLOSED if of(boxed, i) else 0)
        for k in range(n_inst):
            own = range(int(offsets[k]), int(offsets[k + 1]))
            if any(draws[i] & TOUCHED for i in own):
                insts[k] |= TOUCHED
            if any(draws[i] & ENCLOSED for i in own) and all(draws[i] & ENCLOSED for i in own if tags[i] in pk.PAINT_TAGS and of(nonempty, i)):
                insts[k] |= ENCLOSED
    counts = {"draws_touched": int((draws & TOUCHED != 0).sum()), "draws_enclosed": int((draws & ENCLOSED != 0).sum()),
              "instances_touched": 0 if insts is None else int((insts & TOUCHED != 0).sum()),
              "instances_enclosed": 0 if insts is None else int((insts & ENCLOSED != 0).sum())}
    return draws, insts, counts


def check(engine, oracle, rect, name, offsets=None, hand=None):
    """The engine's words and counts equal the reference's; `hand`: the draw words known by hand (a list, None where not known)."""
    want = reference(oracle, rect, offsets)
    got = engine.pick_rect(rect)
    assert engine.pick_rect_sizes() == (len(want[0]), 0 if want[1] is None else len(want[1])), f"{name}: sizes"
    assert got[0].dtype == np.uint32 and np.array_equal(got[0], want[0]), f"{name} {rect}: draws: engine {got[0].tolist()}, reference {want[0].tolist()}"
    if want[1] is None:
        assert got[1] is None
    else:
        assert np.array_equal(got[1], want[1]), f"{name} {rect}: instances: engine {got[1].tolist()}, reference {want[1].tolist()}"
    assert got[2] == want[2], f"{name} {rect}: counts: engine {got[2]}, reference {want[2]}"
    if hand is not None:
        for i, hk in enumerate(hand):
            if hk is not None:
                assert int(want[0][i]) == hk, f"{name} {rect}: draw {i}: reference {int(want[0][i])}, known by hand {hk}"
    return want


def some_rects(w, h, seed=0, n=12):
    """Marquees of every kind: integer-aligned, a few pixels wide, reaching the target's edges, partly and wholly off it, reversed,
    empty, the whole target."""
    rng = np.random.default_rng(8100 + seed)
    out = [(0.0, 0.0, float(w), float(h)), (-INF, -INF, INF, INF), (w * 0.25, h * 0.25, w * 0.75, h * 0.75), (w * 0.75, h * 0.75, w * 0.25, h * 0.25),
           (0.0, 0.0, w * 0.5, float(h)), (w * 0.5, 0.0, float(w), float(h)), (-20.0, -20.0, 8.0, 8.0), (w - 6.0, h - 6.0, w + 30.0, h + 30.0),
           (-30.0, -30.0, -5.0, -5.0), (10.0, 10.0, 10.0, 30.0), (NAN, 0.0, 10.0, 10.0)]
    for k in range(n):
        cx, cy = rng.uniform(0, w), rng.uniform(0, h)
        hw, hh = (rng.uniform(0.5, 4.0), rng.uniform(0.5, 4.0)) if k % 3 == 0 else (rng.uniform(4, w * 0.6), rng.uniform(4, h * 0.6))
        r = (cx - hw, cy - hh, cx + hw, cy + hh)
        out.append(tuple(float(np.rint(v)) for v in r) if k % 3 == 1 else r)
    return out


def check_rects(engine, oracle, rects, name, offsets=None):
    """`check` over a list of marquees; returns the reference's answers."""
    return [check(engine, oracle, r, f"{name}[{k}]", offsets) for k, r in enumerate(rects)]


# ---------------------------------------------------------------------------------------------------------------
# 1. Geometry known by hand
# ---------------------------------------------------------------------------------------------------------------
def _up(v):
    return float(np.nextafter(f32(v), f32(np.inf)))


def _down(v):
    return float(np.nextafter(f32(v), f32(-np.inf)))


SQUARE_CASES = [((12, 12, 20, 20), 1), ((5, 5, 35, 35), 3), ((10, 10, 30, 30), 3), ((_up(10), 10, 30, 30), 1), ((5, 5, 15, 15), 1), ((10, 10, 20, 20), 1),
                ((0, 10, 10, 30), 0), ((0, 10, _up(10), 30), 1), ((30, 10, 40, 30), 0), ((_down(30), 10, 40, 30), 1), ((0, 0, 10, 10), 0),
                ((0, 0, _up(10), _up(10)), 1), ((-50, -50, 500, 500), 3), ((35, 35, 5, 5), 3), ((-INF, -INF, INF, INF), 3), ((40, 5, 60, 40), 0),
                ((20, 20, 20, 30), 0), ((NAN, 5, 35, 35), 0), ((5, 5, 35, NAN), 0), ((-20, -20, -5, -5), 0), ((100, 100, 200, 200), 0)]


def check_hand_square(engine, name):
    """Rect(10, 10, 30, 30) on a 64 x 48 target (4 lines): the issue's table of marquees, word by word."""
    from vello_amd import Affine, Color, Fill, Rect, Scene

    s = Scene()
    s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(200, 60, 60), None, Rect(10.0, 10.0, 30.0, 30.0))
    o, bump = pk.scene_frame(engine, s, 64, 48)
    assert bump["lines"] == 4
    for rect, word in SQUARE_CASES:
        want = check(engine, o, [float(v) for v in rect], name, hand=[word])
        assert want[2]["draws_touched"] == (word & 1) and want[2]["draws_enclosed"] == (word >> 1)


def check_hand_shapes(engine, name):
    """The pentagram under both fill rules with a marquee in its centre; a stroke met across its width and the hole of a closed one."""
    packed, layout = _hand_shapes()
    o, _ = pk.scene_frame(engine, (packed, layout), 128, 80)
    # the centre of the pentagrams: inside the non-zero fill (HIT, no line met), in the even-odd one's hole
    check(engine, o, (18.0, 22.0, 22.0, 26.0), name + "_centre_nz", hand=[1, 0, 0, 0, 0, 0, 0])
    check(engine, o, (50.0, 22.0, 54.0, 26.0), name + "_centre_eo", hand=[0, 0, 0, 0, 0, 0, 0])
    check(engine, o, (50.0, 12.0, 54.0, 16.0), name + "_point_eo", hand=[0, 1, None, 0, 0, 0, 0])
    # across the open stroke's width (its outline is met), beside it; the hole of the closed stroke, and across its band
    check(engine, o, (88.0, 2.0, 92.0, 20.0), name + "_across", hand=[0, 0, 1, 0, 0, 0, 0])
    check(engine, o, (88.0, 14.0, 92.0, 20.0), name + "_beside", hand=[0, 0, 0, 0, 0, 0, 0])
    check(engine, o, (85.0, 30.0, 99.0, 38.0), name + "_hole", hand=[0, 0, 0, 0, 0, 0, 0])
    check(engine, o, (68.0, 30.0, 80.0, 38.0), name + "_band", hand=[0, 0, 0, 1, 0, 0, 0])
    check(engine, o, (60.0, 0.0, 128.0, 50.0), name + "_both", hand=[0, None, 3, 3, 0, 0, 0])
    check_rects(engine, o, some_rects(128, 80, 1), name + "_rects")


def _hand_shapes():
    from vello_amd import Affine, BezPath, Color, Fill, Rect, Scene, Stroke

    s = Scene()
    s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(250, 200, 40), None, pk._pentagram(20, 24))   # 0
    s.fill(Fill.EvenOdd, Affine.IDENTITY, Color.from_rgb8(40, 200, 250), None, pk._pentagram(52, 24))   # 1
    line = BezPath()
    line.move_to((70.0, 10.0))
    line.line_to((110.0, 10.0))
    s.stroke(Stroke(6.0), Affine.IDENTITY, Color.from_rgb8(90, 250, 90), None, line)                    # 2
    s.stroke(Stroke(4.0), Affine.IDENTITY, Color.from_rgb8(250, 90, 250), None, Rect(72.0, 24.0, 112.0, 44.0))  # 3
    s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(200, 60, 60), None, Rect(10.0, 50.0, 40.0, 70.0))     # 4
    s.fill(Fill.NonZero, Affine.IDENTITY, Color.from_rgb8(60, 60, 200), None, Rect(30.0, 56.0, 60.0, 76.0))     # 5
    s.fill(Fill.NonZero, Affine.IDENTITY, Color(1.0, 1.0, 1.0, 0.0), None, Rect(50.0, 60.0, 80.0, 78.0))        # 6: transparent
    packed, layout = pk.resolve(s)
    assert layout.n_draw_objects == 7
    return packed, layout


def check_brush_fragments(engine, name, which=("blur", "solid", "linear", "image")):
    """The brush fragments (the blurred rect among them) as an instance frame: paint draws of every kind are selected."""
    import vello_amd
    from vello_amd import AaConfig

    frs = ip.brush_fragments()
    lib = vello_amd.FragmentLibrary([frs[k] for k in which])
    w, h = 128, 96
    inst = [(k, (2.0, 0.0, 0.0, 2.0, 30.0 + 22.0 * k, 28.0 + 14.0 * k)) for k in range(len(which))]
    o, off = pk.instance_frame(engine, lib, inst, w, h, AaConfig.Area)
    tags = {int(lib.packed.view(np.uint32)[lib.layout.draw_tag_base + d]) for d in range(lib.layout.n_draw_objects)}
    assert 0x2D4 in tags
    got = check_rects(engine, o, some_rects(w, h, 2) + [(8.0, 12.0, 13.0, 17.0)], name, offsets=off)
    assert got[-1][1][0] & TOUCHED, f"{name}: a corner of the blurred rect is {got[-1][1]}"
    assert (got[0][1] & TOUCHED).all(), f"{name}: the whole target does not touch every fragment"


# ---------------------------------------------------------------------------------------------------------------
# 2. Clips
# ---------------------------------------------------------------------------------------------------------------
CLIP_CASES = [((32, 32, 38, 38), {2}), ((12, 12, 18, 18), {4}), ((22, 22, 28, 28), set()), ((45, 45, 49, 49), set()), ((52, 52, 58, 58), {6}),
              ((85, 25, 95, 35), set()), ((72, 12, 78, 18), {8}), ((0, 70, 8, 88), set())]


def check_clip_scene(engine, name):
    packed, layout = pk.resolve(pk.clip_scene())
    assert layout.n_draw_objects == 10 and layout.n_clips == 6
    o, _ = pk.scene_frame(engine, (packed, layout), 120, 90)
    for rect, touched in CLIP_CASES:
        check(engine, o, [float(v) for v in rect], name, hand=[1 if i in touched else 0 for i in range(10)])
    # the whole target: the four paint draws, all ENCLOSED under the box rule
    check(engine, o, (0.0, 0.0, 120.0, 90.0), name + "_whole", hand=[3 if i in (2, 4, 6, 8) else 0 for i in range(10)])
    check_rects(engine, o, some_rects(120, 90, 3), name + "_rects")


def check_clip_fragments(engine, name):
    import vello_amd
    from vello_amd import AaConfig

    frs = ip.brush_fragments()
    which = ["clip", "blend", ip._scene_fragments("clip_blend")]
    lib = vello_amd.FragmentLibrary([frs[k] if isinstance(k, str) else k for k in which])
    w, h = 200, 160
    inst = [(0, (2.0, 0.0, 0.0, 2.0, 40.0, 40.0)), (1, (2.0, 0.0, 0.0, 2.0, 100.0, 50.0)), (2, (0.6, 0.0, 0.0, 0.6, 60.0, 70.0)), (0, (1.5, 0.5, -0.5, 1.5, 150.0, 120.0))]
    o, off = pk.instance_frame(engine, lib, inst, w, h, AaConfig.Area)
    got = check_rects(engine, o, some_rects(w, h, 4), name, offsets=off)
    assert got[0][2]["draws_touched"] > 10 and got[0][2]["instances_touched"] == 4


# ---------------------------------------------------------------------------------------------------------------
# 3. Against the oracle's image
# ---------------------------------------------------------------------------------------------------------------
def image_rects(w, h, n=300):
    """Seeded marquees: a third integer-aligned, a third a few pixels wide, a third partly or wholly off the target."""
    rng = np.random.default_rng(8300)
    out = []
    for k in range(n):
        if k % 3 == 0:
            x0, y0 = int(rng.integers(0, w - 4)), int(rng.integers(0, h - 4))
            out.append((float(x0), float(y0), float(rng.integers(x0 + 2, w + 1)), float(rng.integers(y0 + 2, h + 1))))
        elif k % 3 == 1:
            x0, y0 = rng.uniform(0, w - 6), rng.uniform(0, h - 6)
            out.append((x0, y0, x0 + rng.uniform(1.5, 6.0), y0 + rng.uniform(1.5, 6.0)))
        else:
            x0, y0 = rng.uniform(-60, w + 20), rng.uniform(-60, h + 20)
            out.append((x0, y0, x0 + rng.uniform(10, 200), y0 + rng.uniform(10, 200)))
    return out


def check_image(engine, name, answer=None):
    """Independent of `reference`: every draw whose colour is settled on a pixel whose unit square lies in R' is TOUCHED; for random
    points strictly inside R' the draw that pick_parity.reference names there is TOUCHED; ENCLOSED implies TOUCHED.  `answer`: what
    gives the draw words in the engine's place (the reference itself, to hold it to the same check)."""
    from vello_amd import AaConfig

    scene, cols = pk.image_scene()
    w, h = 128, 96
    packed, layout = pk.resolve(scene)
    if engine is not None:
        o, _ = pk.scene_frame(engine, (packed, layout), w, h, AaConfig.Area)
    else:
        o = pk.run_oracle(packed, layout, w, h, BLACK, AaConfig.Area)
    settled = [pk.settled_pixels(o.image, c) for c in cols]
    rng = np.random.default_rng(8301)
    pairs, words = 0, set()
    for k, rect in enumerate(image_rects(w, h)):
        draws = answer(o, rect) if answer is not None else engine.pick_rect(rect)[0]
        words |= set(int(v) for v in draws)
        assert all(int(v) in (0, 1, 3) for v in draws), f"{name} {rect}: words {draws.tolist()}: ENCLOSED without TOUCHED, or another bit"
        reg = region(rect, w, h)
        if reg is None:
            assert not draws.any(), f"{name} {rect}: an empty R' selected {draws.tolist()}"
            continue
        x0, y0, x1, y1 = (float(v) for v in reg[:4])
        px0, py0, px1, py1 = int(np.ceil(x0)), int(np.ceil(y0)), int(np.floor(x1)), int(np.floor(y1))  # pixels [px0, px1) x [py0, py1) lie in R'
        for d, m in enumerate(settled):
            if px0 < px1 and py0 < py1 and m[py0:py1, px0:px1].any():
                pairs += 1
                assert draws[d] & TOUCHED, f"{name} {rect}: draw {d} shows inside the marquee and is not TOUCHED ({draws.tolist()})"
        pts = np.stack([rng.uniform(x0, x1, 4), rng.uniform(y0, y1, 4)], axis=1).astype(f32)
        pts = pts[(pts[:, 0] > x0) & (pts[:, 0] < x1) & (pts[:, 1] > y0) & (pts[:, 1] < y1)]
        for pt, (d, _) in zip(pts, pk.reference(o, pts)):
            if d != pk.NONE:
                pairs += 1
                assert draws[d] & TOUCHED, f"{name} {rect}: draw {d} is picked at {pt} inside the marquee and is not TOUCHED ({draws.tolist()})"
    assert pairs >= 500, f"{name}: only {pairs} (rectangle, draw) pairs were checked"
    assert {0, 1, 3} <= words, f"{name}: words seen {words}"


# ---------------------------------------------------------------------------------------------------------------
# 4. Kernel shapes
# ---------------------------------------------------------------------------------------------------------------
def _edge_marquees(o, w, h):
    """Per line of the oracle's soup a small marquee just outside the polygon about the origin-centred instance at (32, 24) that meets
    this line and no other: whichever slot of the soup the line lands in, it alone decides the answer."""
    p = _parsed(o)
    out = []
    for x0, y0, x1, y1 in p["xy32"].astype(f64):
        mx, my = (x0 + x1) / 2, (y0 + y1) / 2
        nx, ny = mx - 32.0, my - 24.0
        s = 0.03 / np.hypot(nx, ny)
        out.append((mx + nx * s - 0.06, my + ny * s - 0.06, mx + nx * s + 0.06, my + ny * s + 0.06))
    return out


def check_soup_shapes(engine, name):
    """Soups of 0, 1, L - 1, L and L + 1 lines (L: lines per workgroup of the line pass).  For the polygons every line in turn is the
    only one a marquee meets, so the deciding line is in the last slot of a workgroup, and in the first of the next, whatever the
    order of the soup; then a path whose lines straddle two workgroups."""
    import vello_amd
    from vello_amd import AaConfig

    chunk = engine.pick_constants()["rect_lines_per_workgroup"]
    assert chunk > 0
    w, h = 64, 48
    rects = some_rects(w, h, 5, n=6)
    o, bump = pk.scene_frame(engine, pk.raw_scene([0x10, 0x10], [], 2), w, h)
    assert bump["lines"] == 0
    assert all(not r[0].any() for r in check_rects(engine, o, rects, name + "_0"))
    # one upward line from (10, 10) to (10, 30): an open path, a leftward ray from x > 10 crosses it
    o, bump = pk.scene_frame(engine, pk.raw_scene([0x0D, 0x10], [10.0, 10.0, 10.0, 30.0], 1), w, h)
    assert bump["lines"] == 1
    for rect, word in (((5.0, 15.0, 15.0, 25.0), 1), ((12.0, 12.0, 20.0, 20.0), 1), ((2.0, 12.0, 8.0, 20.0), 0), ((10.0, 12.0, 20.0, 40.0), 1),
                       ((0.0, 0.0, 10.0, 48.0), 0), ((0.0, 0.0, 64.0, 48.0), 3)):
        check(engine, o, rect, name + "_1", hand=[word])
    for k in (chunk - 1, chunk, chunk + 1):
        lib = vello_amd.FragmentLibrary([ip.polygon(k, r=20.0)])
        o, off = pk.instance_frame(engine, lib, [(0, (1.0, 0.0, 0.0, 1.0, 32.0, 24.0))], w, h, AaConfig.Area)
        assert o.bump()["lines"] == k and engine.bump()["lines"] == k
        check_rects(engine, o, rects, f"{name}_{k}", offsets=off)
        edges = _edge_marquees(o, w, h)
        alone = 0
        for j, rect in enumerate(edges if k != chunk - 1 else edges[::8]):
            m, _ = line_meets(o, rect)
            want = check(engine, o, rect, f"{name}_{k}_edge{j}", offsets=off)
            if m.sum() == 1:
                alone += 1
                assert want[0][0] == TOUCHED
        assert alone * 2 > len(edges if k != chunk - 1 else edges[::8]), f"{name}: too few marquees meet one line only"
    # two paths, the second one's lines on both sides of the first workgroup's end (in the order of the scene)
    lib = vello_amd.FragmentLibrary([ip.polygon(chunk - 9, r=12.0), ip.polygon(23, r=9.0)])
    inst = [(0, (1.0, 0.0, 0.0, 1.0, 18.0, 24.0)), (1, (1.0, 0.0, 0.0, 1.0, 46.0, 24.0))]
    o, off = pk.instance_frame(engine, lib, inst, w, h, AaConfig.Area)
    assert engine.bump()["lines"] == chunk + 14
    got = check_rects(engine, o, rects + [(34.0, 12.0, 64.0, 40.0), (36.0, 14.0, 56.0, 34.0), (44.0, 22.0, 48.0, 26.0), (0.0, 0.0, 31.0, 48.0)], name + "_straddle",
                      offsets=off)
    assert got[-4][1].tolist() == [0, 3] and got[-3][1].tolist() == [0, 3] and got[-2][1].tolist() == [0, 1] and got[-1][1].tolist() == [3, 0]


def check_draw_shapes(engine, name):
    """D = 0, 1, one below / at / one above the draw pass's draws per workgroup and 3 D + 1; a missed clip whose BeginClip lies in the
    first workgroup and whose EndClip in the third, so that the draws it hides lie one and two workgroups later: the carry over more
    than one chunk."""
    step = engine.pick_constants()["rect_draws_per_workgroup"]
    assert step > 0
    w, h = 128, 96
    rects = [(0.0, 0.0, 128.0, 96.0), (0.0, 0.0, 60.0, 40.0), (30.5, 20.5, 33.0, 23.0), (100.0, 70.0, 128.0, 96.0), (-5.0, -5.0, 1.0, 1.0)]
    for d in (0, 1, step - 1, step, step + 1, 3 * step + 1):
        packed, layout = pk.resolve(pk.many_draws(d))
        assert layout.n_draw_objects == d
        o, _ = pk.scene_frame(engine, (packed, layout), w, h)
        got = check_rects(engine, o, rects, f"{name}_{d}")
        assert got[0][2]["draws_touched"] == d and got[0][2]["draws_enclosed"] == d
        assert d < 200 or 0 < got[1][2]["draws_touched"] < d
    d = 3 * step + 1
    clip_at, pop_at = 5, 2 * step + 6
    packed, layout = pk.resolve(pk.many_draws(d, clip_at, pop_at))
    assert layout.n_draw_objects == d and layout.n_clips == 2 and pop_at // step == 2 and clip_at // step == 0
    o, _ = pk.scene_frame(engine, (packed, layout), w, h)
    got = check_rects(engine, o, rects, f"{name}_carry")
    for (draws, _, _), rect in zip(got[1:2], rects[1:2]):  # (the marquee does not meet the clip's path at (120, 88) .. (127, 95))
        seen = np.nonzero(draws)[0]
        assert len(seen) and ((seen < clip_at) | (seen > pop_at)).all(), f"{name} {rect}: a draw under the missed clip is selected"
        assert (seen > pop_at).any() and (seen < clip_at).any(), f"{name} {rect}: nothing before or after the missed clip"
    # a marquee that touches the clip's path: the draws under it count again
    got = check(engine, o, (90.0, 60.0, 128.0, 96.0), f"{name}_clip_met")
    seen = np.nonzero(got[0])[0]
    assert ((seen > clip_at) & (seen < pop_at)).any()
    # a missed clip left open up to the last draw, across two workgroup boundaries
    packed, layout = pk.resolve(pk.many_draws(2 * step + 9, clip_at=step - 1, pop_at=2 * step + 8))
    o, _ = pk.scene_frame(engine, (packed, layout), w, h)
    got = check_rects(engine, o, rects[1:3], f"{name}_open")
    assert all(np.nonzero(g[0])[0].max() < step - 1 for g in got)


# ---------------------------------------------------------------------------------------------------------------
# 5. Instances
# ---------------------------------------------------------------------------------------------------------------
def check_three_draws(engine, name):
    """Empty fragments between drawn ones, and a fragment of three draws of which the marquee encloses two: TOUCHED, not ENCLOSED.
    Lists of one instance and of none."""
    import vello_amd
    from vello_amd import AaConfig

    lib = pk.instance_library()
    w, h, aa = 128, 96, AaConfig.Area
    # the three rects of the fragment under scale 2 at (40, 40): [28, 52] x [32, 48], [38, 62] x [38, 54], [48, 72] x [44, 60]
    inst = [(lib.empty, (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)), (lib.three, (2.0, 0.0, 0.0, 2.0, 40.0, 40.0)), (lib.empty, (1.0, 0.0, 0.0, 1.0, 5.0, 5.0)),
            (0, (1.0, 0.0, 0.0, 1.0, 100.0, 70.0)), (lib.empty, (1.0, 0.0, 0.0, 1.0, 9.0, 9.0))]
    o, off = pk.instance_frame(engine, lib, inst, w, h, aa)
    assert off.tolist() == [0, 0, 3, 3, 4, 4]
    want = check(engine, o, (20.0, 20.0, 65.0, 56.0), name + "_two_of_three", offsets=off, hand=[3, 3, 1, 0])
    assert want[1].tolist() == [0, 1, 0, 0, 0], want[1]
    want = check(engine, o, (20.0, 20.0, 75.0, 62.0), name + "_three_of_three", offsets=off, hand=[3, 3, 3, 0])
    assert want[1].tolist() == [0, 3, 0, 0, 0], want[1]
    want = check(engine, o, (0.0, 0.0, 128.0, 96.0), name + "_whole", offsets=off, hand=[3, 3, 3, 3])
    assert want[1].tolist() == [0, 3, 0, 3, 0] and want[2]["instances_enclosed"] == 2
    check_rects(engine, o, some_rects(w, h, 6), name + "_rects", offsets=off)
    # one instance; an empty one alone; no instance at all
    o, off = pk.instance_frame(engine, lib, inst[1:2], w, h, aa, upload=False)
    assert check(engine, o, (20.0, 20.0, 65.0, 56.0), name + "_one", offsets=off)[1].tolist() == [1]
    for few in (inst[:1], []):
        o, off = pk.instance_frame(engine, lib, few, w, h, aa, upload=False)
        assert engine.pick_rect_sizes() == (0, len(few))
        draws, insts, counts = engine.pick_rect((0.0, 0.0, 128.0, 96.0))
        assert len(draws) == 0 and (insts is None if not few else insts.tolist() == [0]) and not any(counts.values())
        check(engine, o, (0.0, 0.0, 128.0, 96.0), name + f"_{len(few)}", offsets=off if few else None)


def check_instances(engine, name, dev):
    """render_instances and _painted frames over a library with EMPTY fragments between drawn ones; a retained list under turned poses
    from host and device memory, and under a view; frames that were not composed from instances take no instances_out."""
    import vello_amd
    from vello_amd import AaConfig, Affine

    lib = pk.instance_library()
    w, h, aa = 128, 96, AaConfig.Msaa8
    inst = pk.instance_list(lib, w, h)
    rects = some_rects(w, h, 7)
    o, off = pk.instance_frame(engine, lib, inst, w, h, aa)
    got = check_rects(engine, o, rects, name + "_instances", offsets=off)
    assert any(1 in g[1].tolist() for g in got) and any(3 in g[1].tolist() for g in got) and any(0 in g[1].tolist() for g in got)
    assert all(g[1][i] == 0 for g in got for i, (f, _) in enumerate(inst) if f == lib.empty), f"{name}: an empty instance is selected"
    paints = rp.some_paints(len(inst))
    o, off = pk.instance_frame(engine, lib, inst, w, h, aa, paints=paints, upload=False)
    painted = check_rects(engine, o, rects, name + "_painted", offsets=off)
    assert all(np.array_equal(a[1], b[1]) for a, b in zip(got, painted)), f"{name}: paints changed the selection"
    # retained: rest poses, turned poses from host and device memory, painted, under a view
    engine.retain_instances(inst)
    rp.frame(engine, w, h, BLACK, aa, None, "rest")
    check_rects(engine, o, rects, name + "_retained_rest", offsets=off)
    poses = rp.turned(inst, w, h, 3)
    shown = rp.posed(inst, poses)
    o_t = pk.run_oracle(*rp.compose(lib, shown), w, h, BLACK, aa, lib)
    for source in ("host", "device"):
        rp.frame(engine, w, h, BLACK, aa, poses, source, dev.to_device)
        moved = check_rects(engine, o_t, rects, f"{name}_retained_{source}", offsets=off)
        assert any(not np.array_equal(a[1], b[1]) for a, b in zip(got, moved)), f"{name}: the selection ignored the {source} poses"
    view = Affine.translate(9.0, -6.0) * Affine.rotate(0.2) * Affine.scale(1.2)
    try:
        engine.set_view_transform(view)
        rp.frame(engine, w, h, BLACK, aa, poses, "device", dev.to_device)
    finally:
        engine.set_view_transform(None)
    packed, layout = rp.compose(lib, shown)
    o_v = pk.run_oracle(view_parity.compose(packed, layout, view), layout, w, h, BLACK, aa, lib)
    viewed = check_rects(engine, o_v, rects, name + "_retained_view", offsets=off)
    assert any(not np.array_equal(a[1], b[1]) for a, b in zip(viewed, moved))
    # frames that were not composed from instances: no instance words, and instances_out is refused
    engine.render_resident(w, h, BLACK, aa)
    assert engine.sync() == 0
    o_lib = pk.run_oracle(lib.packed, lib.layout, w, h, BLACK, aa, lib)
    check_rects(engine, o_lib, rects[:4], name + "_resident")
    out = np.full(4, 0x5A5A5A5A, dtype=np.uint32)
    with np.testing.assert_raises(vello_amd.VelloHipError) as e:
        engine.pick_rect(rects[0], instances_out=out)
    assert e.exception.code == E_INVALID and b"no instances" in engine._lib.vello_hip_last_error(engine._h) and (out == 0x5A5A5A5A).all()
    view_parity.render_frame_into(engine, packed, layout, w, h, BLACK, aa, dev.target(w, h))
    fr = check_rects(engine, o_t, rects, name + "_render_frame")
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(fr, moved))
    assert engine.sync() == 0


def check_retained_painted(engine, name, dev):
    """The words of a selection, in device memory, become the next retained frame's paints: the round trip the entry point exists for."""
    import vello_amd
    from vello_amd import AaConfig

    lib = pk.instance_library()
    lib.upload(engine)
    w, h, aa = 128, 96, AaConfig.Area
    inst = pk.instance_list(lib, w, h, 2)
    off = pk.draw_offsets(lib, inst)
    engine.retain_instances(inst)
    paints = rp.some_paints(len(inst))
    engine.render_retained(w, h, BLACK, aa, paints=paints)
    assert engine.sync() == 0
    o = pk.run_oracle(*rp.compose(lib, inst, paints), w, h, BLACK, aa, lib)
    check_rects(engine, o, some_rects(w, h, 8), name, offsets=off)


# ---------------------------------------------------------------------------------------------------------------
# 6. Culling
# ---------------------------------------------------------------------------------------------------------------
def check_culling(engine, name):
    """Identical outputs with viewport culling on and off: a scene with lines off all four sides of the target, marquees that reach
    its edges."""
    from vello_amd import AaConfig, Affine

    w, h = 120, 90
    packed, layout = pk.resolve(pk.clip_scene())
    view = Affine.translate(-30.0, -25.0) * Affine.scale(2.2)
    o_v = pk.run_oracle(view_parity.compose(packed, layout, view), layout, w, h, BLACK, AaConfig.Msaa8)
    xy = _parsed(o_v)["xy"]
    assert (xy[:, [0, 2]].max(axis=1) < 0).any() and (xy[:, [0, 2]].min(axis=1) > w).any() and (xy[:, [1, 3]].max(axis=1) < 0).any() and \
        (xy[:, [1, 3]].min(axis=1) > h).any(), f"{name}: the scene does not reach past every side"
    rects = some_rects(w, h, 9) + [(0.0, 0.0, 120.0, 1.0), (0.0, 89.0, 120.0, 90.0), (119.0, 0.0, 120.0, 90.0), (0.0, 0.0, 1.0, 90.0), (0.0, 80.0, 120.0, 200.0),
                                   (100.0, -50.0, 300.0, 300.0)]
    engine.upload_scene(packed, layout)
    answers, lines = [], []
    try:
        engine.set_view_transform(view)
        for cull in (False, True):
            engine.set_viewport_cull(cull)
            engine.render_resident(w, h, BLACK, AaConfig.Msaa8)
            assert engine.sync() == 0
            lines.append(engine.bump()["lines"])
            answers.append(check_rects(engine, o_v, rects, f"{name}_cull{int(cull)}"))
    finally:
        engine.set_view_transform(None)
        engine.set_viewport_cull(False)
    assert lines[1] < lines[0], f"{name}: culling dropped no line"
    assert any(a[0].any() for a in answers[0])


# ---------------------------------------------------------------------------------------------------------------
# 7. Which frame, and 9. nothing else moves
# ---------------------------------------------------------------------------------------------------------------
def check_which_frame(engine, name, dev):
    """Four frames in flight under four pose sets: the fourth answers; afterwards sync is 0, every target holds its own image, the bump
    counters are the same, a following frame is right and no scene buffer was allocated.  After grow_pools or an upload the call is
    refused."""
    import vello_amd
    from vello_amd import AaConfig

    lib = pk.instance_library()
    lib.upload(engine)
    w, h, aa = 128, 96, AaConfig.Msaa8
    inst = pk.instance_list(lib, w, h, 1)
    off = pk.draw_offsets(lib, inst)
    engine.retain_instances(inst)
    sets = [rp.turned(inst, w, h, 20 + k) for k in range(4)]
    oracles = [pk.run_oracle(*rp.compose(lib, rp.posed(inst, p)), w, h, BLACK, aa, lib) for p in sets]
    rects = some_rects(w, h, 10, n=6)
    refs = [[reference(o, r, off) for r in rects] for o in oracles]
    assert all(any(not np.array_equal(a[1], b[1]) for a, b in zip(refs[3], r)) for r in refs[:3])

    def answers():
        return [engine.pick_rect(r) for r in rects]

    def same(got, want):
        return all(np.array_equal(g[0], x[0]) and np.array_equal(g[1], x[1]) and g[2] == x[2] for g, x in zip(got, want))

    keep = []
    try:
        engine.set_frames_in_flight(4)
        for k in range(4):  # (every lane has held the list: nothing is allocated from here on)
            rp.render_retained(engine, w, h, BLACK, aa, sets[k], "host")
        assert engine.sync() == 0
        engine.pick_rect(rects[0])  # (the query's own scratch is the context's, made by the first call)
        before = engine.scene_allocations()
        t = [dev.target(w, h) for _ in range(5)]
        for k in range(4):
            rp.render_retained(engine, w, h, BLACK, aa, sets[k], ("host", "device")[k % 2], dev.to_device, out=t[k], keep=keep)
        assert same(answers(), refs[3]), f"{name}: the frame submitted last does not answer"
        assert engine.sync() == 0
        bump = engine.bump()
        assert same(answers(), refs[3]) and engine.bump() == bump and engine.sync() == 0, f"{name}: a call moved the bump counters or sync"
        for k in range(4):
            assert np.array_equal(dev.to_numpy(t[k]), oracles[k].image), f"{name}: target {k} after the calls"
        rp.render_retained(engine, w, h, BLACK, aa, sets[1], "device", dev.to_device, out=t[4], keep=keep)
        assert same(answers(), refs[1]), f"{name}: the call after the following frame"
        assert engine.sync() == 0
        assert np.array_equal(dev.to_numpy(t[4]), oracles[1].image), f"{name}: the frame after a call"
        assert engine.scene_allocations() == before, f"{name}: a call allocated a scene buffer"
    finally:
        engine.set_frames_in_flight(1)
    # pools grown since, scene replaced since
    out = np.full(len(refs[0][0][0]), 0x5A5A5A5A, dtype=np.uint32)
    grown = dict(engine.bump(), lines=engine.bump()["lines"] + (1 << 22))
    assert engine.grow_pools(grown)
    for what in ("grow_pools", "upload"):
        with np.testing.assert_raises(vello_amd.VelloHipError) as e:
            engine.pick_rect(rects[0], draws_out=out, instances=False)
        assert e.exception.code == E_INVALID and (out == 0x5A5A5A5A).all(), f"{name}: after {what}"
        with np.testing.assert_raises(vello_amd.VelloHipError):
            engine.pick_rect_sizes()
        if what == "grow_pools":
            rp.frame(engine, w, h, BLACK, aa, sets[0], "host")
            assert same(answers(), refs[0])
            lib.upload(engine)


# ---------------------------------------------------------------------------------------------------------------
# 8. Sources and sinks, refusals, failed frames
# ---------------------------------------------------------------------------------------------------------------
def _ptr(x):
    if x is None:
        return None
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr() if hasattr(x, "data_ptr") else int(x)


def raw(engine, rect, draws, n_draws, insts, n_insts, is_device, counts):
    r4 = None if rect is None else np.ascontiguousarray(rect, dtype=f32)
    return engine._lib.vello_hip_pick_rect(engine._h, _ptr(r4), _ptr(draws), n_draws, _ptr(insts), n_insts, int(is_device),
                                           ctypes.byref(counts) if counts is not None else None)


def check_sinks(engine, name, dev):
    """Host and device outputs; draws only, instances only, counts only; outputs pre-filled with a pattern are fully overwritten on
    success, the empty R' included."""
    from vello_amd import AaConfig
    from vello_amd._lib import RegionCounts

    lib = pk.instance_library()
    w, h, aa = 128, 96, AaConfig.Area
    inst = pk.instance_list(lib, w, h)
    o, off = pk.instance_frame(engine, lib, inst, w, h, aa)
    nd, ni = engine.pick_rect_sizes()
    assert (nd, ni) == (int(off[-1]), len(inst))
    PAT = 0xA5A5A5A5
    numpy_dev = isinstance(dev.words(1), np.ndarray)
    for rect in [(20.0, 10.0, 90.0, 70.0), (0.0, 0.0, 128.0, 96.0), (30.0, 30.0, 30.0, 60.0), (NAN, 0.0, 5.0, 5.0), (300.0, 300.0, 400.0, 400.0)]:
        want = reference(o, rect, off)
        empty = region(rect, w, h) is None
        assert empty or want[0].any() or rect[0] == 300.0
        for device in (False, True):
            kw = {"out_is_device": True} if device and numpy_dev else {}
            mk = (lambda n: dev.words(n, PAT)) if device else (lambda n: np.full(n, PAT, dtype=np.uint32))
            back = dev.words_numpy if device else (lambda a: a)
            d, i = mk(nd), mk(ni)
            rd, ri, c = engine.pick_rect(rect, draws_out=d, instances_out=i, **kw)
            assert rd is d and ri is i and np.array_equal(back(d), want[0]) and np.array_equal(back(i), want[1]) and c == want[2], f"{name} {rect}: both, device {device}"
            d = mk(nd)
            rd, ri, c = engine.pick_rect(rect, draws_out=d, instances=False, **kw)
            assert ri is None and np.array_equal(back(d), want[0]) and c == want[2], f"{name} {rect}: draws only, device {device}"
            i = mk(ni)
            rd, ri, c = engine.pick_rect(rect, instances_out=i, draws=False, **kw)
            assert rd is None and np.array_equal(back(i), want[1]) and c == want[2], f"{name} {rect}: instances only, device {device}"
        assert engine.pick_rect(rect, draws=False, instances=False) == (None, None, want[2]), f"{name} {rect}: counts only"
        counts = RegionCounts(7, 7, 7, 7)
        d = np.full(nd, PAT, dtype=np.uint32)
        assert raw(engine, rect, d, nd, None, 0, 0, None) == 0 and np.array_equal(d, want[0]), f"{name} {rect}: no counts"
        assert raw(engine, rect, None, 0, None, 0, 0, counts) == 0 and counts.as_dict() == want[2]
    assert engine.sync() == 0


def check_refusals(make_engine, name, dev, host_memory=None):
    """Every VELLO_HIP_E_INVALID of the entry point, each leaving the outputs untouched and naming its rule."""
    from vello_amd import AaConfig
    from vello_amd._lib import RegionCounts

    engine = make_engine(None)
    w, h = 64, 48
    rect = (5.0, 5.0, 40.0, 40.0)
    PAT = 0x5A5A5A5A
    n = 12
    out, out_i = np.full(n + 4, PAT, dtype=np.uint32), np.full(n + 4, PAT, dtype=np.uint32)
    d_out = dev.words(n + 4, PAT)
    counts = RegionCounts(PAT, PAT, PAT, PAT)
    sizes = (ctypes.c_uint32(PAT), ctypes.c_uint32(PAT))

    def last():
        return engine._lib.vello_hip_last_error(engine._h)

    def untouched():
        return (out == PAT).all() and (out_i == PAT).all() and (dev.words_numpy(d_out) == PAT).all() and all(v == PAT for v in counts.as_dict().values())

    # no frame was ever rendered
    assert raw(engine, rect, out, n, None, 0, 0, counts) == E_INVALID and b"no frame" in last() and untouched()
    assert engine._lib.vello_hip_pick_rect_sizes(engine._h, ctypes.byref(sizes[0]), ctypes.byref(sizes[1])) == E_INVALID and b"no frame" in last()
    assert sizes[0].value == PAT and sizes[1].value == PAT
    assert engine._lib.vello_hip_pick_rect_sizes(None, ctypes.byref(sizes[0]), ctypes.byref(sizes[1])) == E_INVALID
    o, _ = pk.scene_frame(engine, pk.many_draws(n), w, h, AaConfig.Msaa8)
    assert engine.pick_rect_sizes() == (n, 0)
    assert engine._lib.vello_hip_pick_rect(None, _ptr(np.zeros(4, dtype=f32)), _ptr(out), n, None, 0, 0, None) == E_INVALID
    assert raw(engine, None, out, n, None, 0, 0, counts) == E_INVALID and b"rect" in last()
    assert raw(engine, rect, None, 0, None, 0, 0, None) == E_INVALID and b"all NULL" in last()
    assert raw(engine, rect, out, n - 1, None, 0, 0, counts) == E_INVALID and b"n_draws" in last()
    assert raw(engine, rect, out, n + 1, None, 0, 0, counts) == E_INVALID and b"n_draws" in last()
    assert raw(engine, rect, out, n, out_i, 0, 0, counts) == E_INVALID and b"no instances" in last()
    assert raw(engine, rect, None, 0, out_i, 3, 0, counts) == E_INVALID and b"no instances" in last()
    assert raw(engine, rect, _ptr(d_out) + 2, n, None, 0, 1, counts) == E_INVALID and b"multiple of 4" in last()
    if host_memory is not None:  # (GPU build: host memory handed in as device memory, pageable and pinned)
        for kind, mem in host_memory(n).items():
            assert raw(engine, rect, mem, n, None, 0, 1, counts) == E_INVALID and b"not device memory" in last(), f"{name}: {kind} draws_out"
    assert untouched(), f"{name}: a refused call wrote an output"
    # an instance frame: the instance count is held too
    lib = pk.instance_library()
    inst = pk.instance_list(lib, w, h)
    o_i, off = pk.instance_frame(engine, lib, inst, w, h, AaConfig.Area)
    ni = len(inst)
    assert ni <= n + 4
    assert raw(engine, rect, None, 0, out_i, ni - 1, 0, counts) == E_INVALID and b"n_instances" in last()
    assert raw(engine, rect, None, 0, _ptr(d_out) + 2, ni, 1, counts) == E_INVALID and b"multiple of 4" in last()
    if host_memory is not None:
        for kind, mem in host_memory(ni).items():
            assert raw(engine, rect, None, 0, mem, ni, 1, counts) == E_INVALID and b"not device memory" in last(), f"{name}: {kind} instances_out"
    assert untouched(), f"{name}: a refused call wrote an output"
    # ... and the accepted call still answers
    want = reference(o_i, rect, off)
    assert raw(engine, rect, None, 0, d_out, ni, 1, counts) == 0
    assert np.array_equal(dev.words_numpy(d_out)[:ni], want[1]) and (dev.words_numpy(d_out)[ni:] == PAT).all() and counts.as_dict() == want[2]
    assert engine.sync() == 0


def check_failed_frame(make_engine, name, dev):
    """From tiny pools, a frame that ends in E_CAPACITY: the call returns E_CAPACITY and writes nothing; after grow_pools and a good
    frame it answers."""
    import vello_amd
    from vello_amd import AaConfig

    w, h, aa = 128, 96, AaConfig.Msaa8
    engine = make_engine(dict(lines=64, seg_counts=64, segments=64, tiles=256))
    lib = vello_amd.FragmentLibrary([ip.polygon(9), ip.polygon(14)])
    lib.upload(engine)
    inst = ip.scatter(np.random.default_rng(4), 30, 2, w, h, scale=(1.0, 2.5))
    PAT = 0x5A5A5A5A
    rect = (10.0, 10.0, 100.0, 80.0)
    engine.render_instances(inst, w, h, BLACK, aa)
    nd, ni = engine.pick_rect_sizes()
    assert (nd, ni) == (30, 30)
    for device in (False, True):
        d = dev.words(nd, PAT) if device else np.full(nd, PAT, dtype=np.uint32)
        i = dev.words(ni, PAT) if device else np.full(ni, PAT, dtype=np.uint32)
        kw = {"out_is_device": True} if device and isinstance(d, np.ndarray) else {}
        with np.testing.assert_raises(vello_amd.VelloHipError) as e:
            engine.pick_rect(rect, draws_out=d, instances_out=i, **kw)
        assert e.exception.code == E_CAPACITY, f"{name}: {e.exception}"
        back = dev.words_numpy if device else (lambda a: a)
        assert (back(d) == PAT).all() and (back(i) == PAT).all(), f"{name}: the call on a failed frame wrote an output"
    assert engine.sync() == E_CAPACITY, f"{name}: the call hid the frame's failure from sync"
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
    o = pk.run_oracle(*rp.compose(lib, inst), w, h, BLACK, aa, lib)
    want = check(engine, o, rect, name, offsets=pk.draw_offsets(lib, inst))
    assert want[0].any()
