"""The core pipeline's kernels at their partition boundaries.  Every size comes from Engine.stage_constants() (vello_hip_stage_constant):
the generators below place a given tag, draw object, clip, line or tile row at a given offset from a boundary, the checks assert -- from
the resolved scene bytes, the engine's buffers or its bump counters -- that the boundary was hit, and every frame ends in
parity.compare_frame (all stages, the back half, MSAA bit-exact, area AA within 1 plus the exact same-order check) or, for clips,
in parity.compare_clip_stage.  Colours are distinct and translucent, so that a swapped or dropped draw changes pixels.

The checks are shared by tests/test_stage_shapes_emu.py (the SIMT-emulated build: workgroups one after another, the portable twins of the
wave primitives) and tests/test_stage_shapes_gpu.py (the MI355X, where the cross-wave and cross-workgroup parts really run)."""
import numpy as np

from oracle.oracle import Oracle
from tests.parity import compare_clip_stage, compare_frame

BLACK = 0xFF000000
TRANSFORM, STYLE, PATH = 0x20, 0x40, 0x10  # path tag bytes of the markers
W, H = 128, 96


def make_oracle():
    return Oracle(capacity_scale=4, auto_grow=True)


def colour(k, alpha=150):
    from vello_amd import Color

    return Color.from_rgba8(30 + (k * 37) % 220, 250 - (k * 53) % 220, 40 + (k * 91) % 200, alpha)


def tag_bytes(packed, layout):
    """(the resolved tag stream with its padding, the number of live tags): tag bytes are non-zero, the padding is zero."""
    t = np.ascontiguousarray(packed, dtype=np.uint8)[layout.path_tag_base * 4: layout.path_data_base * 4]
    nz = np.nonzero(t)[0]
    return t, (int(nz[-1]) + 1 if len(nz) else 0)


def frames(engine, packed, layout, w, h, name, aas, oracle, in_flight=1, stroke_kernel=False):
    """compare_frame under every AA mode of `aas`, with `in_flight` frames in flight; stroke_kernel: flatten's stroked-line kernel
    takes the stroked lines however few they are (with frames in flight it is a launch of its own)."""
    from vello_amd import AaConfig

    engine.set_auto_grow(True)
    engine.set_frames_in_flight(in_flight)
    try:
        if stroke_kernel:
            engine.set_debug_flags(stroke_kernel=True)
        for aa in aas:
            compare_frame(engine, packed, layout, w, h, BLACK, aa, f"{name}_{int(aa)}_f{in_flight}", tol=1 if aa == AaConfig.Area else 0, oracle=oracle)
    finally:
        engine.set_frames_in_flight(1)
        if stroke_kernel:
            engine.set_debug_flags()


# ---------------------------------------------------------------------------------------------------------------
# (a) Tags at a boundary
# ---------------------------------------------------------------------------------------------------------------
def _filler(s, k, quad):
    """A closed 3-point (4 tags) or 4-point (5 tags) fill under the identity and the non-zero rule, 9 px wide on a 7 px grid."""
    from vello_amd import Affine, BezPath, Fill

    x, y = 2.0 + 7.0 * (k % 17), 2.0 + 7.0 * ((k // 17) % 12)
    p = BezPath()
    p.move_to((x, y))
    p.line_to((x + 9.0, y))
    if quad:
        p.line_to((x + 9.0, y + 9.0))
    p.line_to((x, y + 9.0))
    p.close_path()
    s.fill(Fill.NonZero, Affine.IDENTITY, colour(k), None, p)


def _n_tags(s):
    return len(s.stream("path_tags"))


def filler_prefix(s, n_tags):
    """Fillers whose tags number exactly n_tags (the scene must be empty): returns the number of fillers."""
    assert _n_tags(s) == 0
    _filler(s, 0, False)
    first = _n_tags(s)  # (TRANSFORM and STYLE ahead of the first path's tags)
    rest = n_tags - first
    assert rest >= 12, "a prefix holds at least a few fillers"
    n_quad = rest % 4
    n_tri = (rest - 5 * n_quad) // 4
    k = 1
    for _ in range(n_tri):
        _filler(s, k, False)
        k += 1
    for _ in range(n_quad):
        _filler(s, k, True)
        k += 1
    assert _n_tags(s) == n_tags, (_n_tags(s), n_tags)
    return k


def probe_stroked_polyline(s, k):
    """A stroked open polyline with round joins and caps that ends in a cubic."""
    from vello_amd import Affine, BezPath, Stroke

    p = BezPath()
    p.move_to((12.0, 80.0))
    p.line_to((30.0, 20.0))
    p.line_to((48.0, 70.0))
    p.line_to((66.0, 14.0))
    p.curve_to((90.0, 10.0), (118.0, 40.0), (96.0, 84.0))
    s.stroke(Stroke(6.0), Affine.IDENTITY, colour(k), None, p)


def probe_closed_stroke(s, k):
    """A closed stroke under a rotation."""
    from vello_amd import Affine, BezPath, Join, Stroke

    p = BezPath()
    p.move_to((40.0, 4.0))
    p.line_to((100.0, 10.0))
    p.line_to((90.0, 50.0))
    p.line_to((50.0, 44.0))
    p.close_path()
    s.stroke(Stroke(5.0, join=Join.Miter), Affine.rotate(0.3), colour(k), None, p)


def probe_cubics(s, k):
    """A filled even-odd path of four cubics that crosses itself."""
    from vello_amd import Affine, BezPath, Fill

    p = BezPath()
    p.move_to((20.0, 48.0))
    p.curve_to((20.0, -10.0), (110.0, 100.0), (110.0, 48.0))
    p.curve_to((110.0, 10.0), (70.0, 10.0), (64.0, 48.0))
    p.curve_to((58.0, 90.0), (20.0, 90.0), (30.0, 30.0))
    p.curve_to((40.0, 0.0), (10.0, 70.0), (20.0, 48.0))
    p.close_path()
    s.fill(Fill.EvenOdd, Affine.IDENTITY, colour(k), None, p)


def probe_alternating(s, k):
    """Six paths that alternate stroke and fill, each with a new transform and a new style."""
    from vello_amd import Affine, BezPath, Fill, Stroke

    for i in range(6):
        p = BezPath()
        p.move_to((10.0 + 16.0 * i, 10.0))
        p.line_to((30.0 + 16.0 * i, 60.0))
        p.line_to((4.0 + 16.0 * i, 70.0))
        xf = Affine.translate(2.0 * i + 1.0, 1.5 * i + 0.5) * Affine.rotate(0.02 * (i + 1))
        if i % 2 == 0:
            s.stroke(Stroke(2.0 + i), xf, colour(k + i), None, p)
        else:
            p.close_path()
            s.fill(Fill.EvenOdd if i % 4 == 1 else Fill.NonZero, xf, colour(k + i), None, p)


def probe_one_line(s, k):
    """A one-line path."""
    from vello_amd import Affine, BezPath, Stroke

    p = BezPath()
    p.move_to((8.0, 90.0))
    p.line_to((120.0, 6.0))
    s.stroke(Stroke(4.0), Affine.IDENTITY, colour(k), None, p)


PROBES = {"polyline": probe_stroked_polyline, "closed_stroke": probe_closed_stroke, "cubics": probe_cubics, "alternating": probe_alternating,
          "one_line": probe_one_line}
TAG_BOUNDARIES = {"flatten_block": ("flatten_block_tags", 1), "pathtag_part": ("pathtag_part_tags", 1), "pathtag_part_2": ("pathtag_part_tags", 2)}


def probe_length(probe):
    """The probe's tags behind a filler (its TRANSFORM and STYLE markers included where it has them)."""
    from vello_amd import Scene

    s = Scene()
    _filler(s, 0, False)
    before = _n_tags(s)
    PROBES[probe](s, 1)
    return _n_tags(s) - before


def tag_offsets(probe, thinned):
    """How many of the probe's tags lie below the boundary: 0 .. its length -- every tag in turn is the last one below the boundary and
    the first one above it; thinned: its first, a middle and its last tag on the edge."""
    n = probe_length(probe)
    return sorted({0, 1, n // 2, n - 1, n}) if thinned else list(range(n + 1))


def tag_scene(probe, boundary, below):
    """Fillers, the probe with `below` of its tags under tag index `boundary`, three more fillers.  Returns (packed, layout, the
    probe's first tag, its length), the position read from the resolved tag stream."""
    from vello_amd import Scene

    s = Scene()
    k = filler_prefix(s, boundary - below)
    PROBES[probe](s, k)
    end = _n_tags(s)
    for i in range(3):
        _filler(s, k + 7 + i, i == 1)
    enc = s.stream("path_tags").copy()
    packed, layout = s.resolve()
    t, live = tag_bytes(packed, layout)
    assert live == len(enc) and np.array_equal(t[:live], enc), "the resolved tag stream is not the encoding's"
    start = boundary - below
    # the fillers before the probe end in a PATH marker and hold neither a TRANSFORM nor a STYLE marker but the scene's first two
    assert t[start - 1] == PATH and not np.isin(t[2:start], (TRANSFORM, STYLE)).any(), "the probe does not begin where it should"
    assert start <= boundary <= end and end - start == probe_length(probe), (start, boundary, end)
    return packed, layout, start, end - start, t


def check_tags_at_boundary(engine, probe, boundary, below, name, in_flight=1, oracle=None, stroke_kernel=False):
    """The probe's tag `below - 1` is the last tag under the boundary and its tag `below` the first above it."""
    from vello_amd import AaConfig

    key, mult = TAG_BOUNDARIES[boundary]
    edge = engine.stage_constants()[key] * mult
    packed, layout, start, n, t = tag_scene(probe, edge, below)
    assert start + below == edge and 0 <= below <= n, f"{name}: the probe misses tag {edge}"
    assert len(t) > edge, f"{name}: the stream ends at the boundary"
    frames(engine, packed, layout, W, H, name, (AaConfig.Msaa16, AaConfig.Area), oracle or make_oracle(), in_flight, stroke_kernel)
    return int(t[edge - 1]), int(t[edge])


def check_probe_slide(engine, probe, boundary, name, thinned=False, in_flight=1, stroke_kernel=False):
    """The probe slid tag by tag across the boundary; the alternating probe must put each kind of marker on either side of the edge."""
    oracle = make_oracle()
    last, first = set(), set()
    for below in tag_offsets(probe, thinned):
        a, b = check_tags_at_boundary(engine, probe, boundary, below, f"{name}_{below}", in_flight, oracle, stroke_kernel)
        last.add(a)
        first.add(b)
    if probe == "alternating" and not thinned:
        for marker in (TRANSFORM, STYLE, PATH):
            assert marker in last and marker in first, f"{name}: marker {marker:#x} never lay on the edge (last {last}, first {first})"


def check_unpadded_stream(engine, blocks, extra, name, in_flight=1):
    """A tag stream of exactly blocks x the flatten block (+ extra) live tags whose last path is a stroke with round joins: with extra
    == 0 nothing pads the stream, and what follows the last tag is path data."""
    from vello_amd import AaConfig, Affine, BezPath, Scene, Stroke

    block = engine.stage_constants()["flatten_block_tags"]
    want = blocks * block + extra
    s = Scene()
    stroke_tags = 5  # STYLE, two lines, the cap marker, PATH
    k = filler_prefix(s, want - stroke_tags)
    p = BezPath()
    p.move_to((10.0, 10.0))
    p.line_to((100.0, 30.0))
    p.line_to((40.0, 85.0))
    s.stroke(Stroke(7.0), Affine.IDENTITY, colour(k), None, p)
    assert _n_tags(s) == want, (_n_tags(s), want)
    packed, layout = s.resolve()
    t, live = tag_bytes(packed, layout)
    assert live == want, f"{name}: {live} live tags, not {want}"
    if extra == 0:
        assert len(t) == live, f"{name}: the stream is padded ({len(t)} bytes for {live} tags)"
    else:
        assert len(t) == (blocks + 1) * block, f"{name}: {len(t)} bytes for {live} tags"
    frames(engine, packed, layout, W, H, name, (AaConfig.Msaa16, AaConfig.Area), make_oracle(), in_flight)


# ---------------------------------------------------------------------------------------------------------------
# (b) Draw objects at a boundary
# ---------------------------------------------------------------------------------------------------------------
def draw_scene(n, stacked, clip_at=None, pop_at=None):
    """n draw objects built with the Scene API (so the bytes are Scene.resolve()'s own): one-segment paths -- stroked lines with butt
    caps, three tags each -- spread on a grid of the 128 x 96 target or stacked in one tile; with clip_at / pop_at a clip layer that
    cuts through the draws opens and closes at those draw-object indices."""
    from vello_amd import Affine, BezPath, Cap, Fill, Rect, Scene, Stroke

    s = Scene()
    style = Stroke(3.0, start_cap=Cap.Butt, end_cap=Cap.Butt)
    k = 0
    for i in range(n):
        if i == clip_at:
            s.push_clip_layer(Fill.NonZero, Affine.IDENTITY, Rect(20.0, 18.0, 70.0, 60.0) if not stacked else Rect(19.0, 18.0, 25.0, 30.0))
        elif i == pop_at:
            s.pop_layer()
        else:
            if stacked:  # all inside tile (1, 1)
                x, y, dx, dy = 18.0 + (k % 5), 19.0 + (k // 5) % 7, 8.0, 4.0 - (k % 3)
            else:
                x, y, dx, dy = 2.0 + 7.0 * (k % 17), 3.0 + 7.0 * ((k // 17) % 13), 8.0, 3.0 - (k % 4)
            p = BezPath()
            p.move_to((x, y))
            p.line_to((x + dx, y + dy))
            s.stroke(style, Affine.IDENTITY, colour(k, 60 if stacked else 150), None, p)
            k += 1
    return s


# 0, 1, and one below / at / one above every size at which a stage cuts the draw objects: (constant, multiple, offset)
DRAW_COUNT_CASES = [(None, 0, 0), (None, 0, 1)] + [(key, m, d) for key, m in (("draw_part", 1), ("draw_part", 2), ("draw_workgroup", 1), ("coarse_batch", 1),
                                                                              ("coarse_batch", 2)) for d in (-1, 0, 1)]


def case_id(case):
    return "-".join(str(v) for v in case if v is not None)


def check_draw_count(engine, case, stacked, name, in_flight=1):
    from vello_amd import AaConfig

    key, mult, delta = case
    n = (engine.stage_constants()[key] * mult if key else 0) + delta
    packed, layout = draw_scene(n, stacked).resolve()
    assert layout.n_draw_objects == n and layout.n_paths == n and layout.n_clips == 0
    img, ref, bump = None, None, None
    oracle = make_oracle()
    frames(engine, packed, layout, W, H, name, (AaConfig.Msaa16, AaConfig.Area), oracle, in_flight)
    if stacked and n:  # one bin, and tile (1, 1) holds every draw: the path records' tile boxes, as the engine wrote them
        p = engine.read_buffer("paths", np.uint32, n * 32).reshape(-1, 8)
        assert (p[:, 0] == 1).all() and (p[:, 1] == 1).all() and (p[:, 2] == 2).all() and (p[:, 3] == 2).all(), f"{name}: a draw left tile (1, 1)"


def check_clip_across_draw_partition(engine, straddle, stacked, name):
    """A clip layer whose BeginClip is the last draw object of a partition and whose EndClip is the first of the next; straddle: the
    pair encloses a whole partition."""
    from vello_amd import AaConfig

    part = engine.stage_constants()["draw_part"]
    clip_at, pop_at = (part - 1, part) if not straddle else (part - 3, 2 * part + 2)
    n = 2 * part + 40
    packed, layout = draw_scene(n, stacked, clip_at, pop_at).resolve()
    tags = np.ascontiguousarray(packed).view(np.uint32)[layout.draw_tag_base: layout.draw_tag_base + n]
    assert layout.n_draw_objects == n and layout.n_clips == 2
    assert tags[clip_at] == 0x49 and tags[pop_at] == 0x21, f"{name}: the clip's draw tags are not where they should be"
    assert clip_at // part + (2 if straddle else 1) == pop_at // part
    frames(engine, packed, layout, W, H, name, (AaConfig.Msaa16, AaConfig.Area), make_oracle())


def _fused_per_frame(engine, packed, layout):
    from vello_amd import AaConfig

    before = engine.fused_launches()
    _, bump = engine.render(packed, layout, W, H, BLACK, AaConfig.Msaa16)
    assert bump["failed"] == 0, bump
    return engine.fused_launches() - before


def _front_switch(engine, name, scenes):
    """scenes: (label, packed, layout, fused launches per frame) on either side of a switch of run_stage_range; flatten's kernel set
    is pinned as parity.check_front_fusion pins it."""
    from vello_amd import AaConfig

    engine.set_auto_grow(True)
    oracle = make_oracle()
    try:
        engine.set_debug_flags(flatten_coop=True)
        for label, packed, layout, per_frame in scenes:
            got = _fused_per_frame(engine, packed, layout)
            assert got == per_frame, f"{name}_{label}: {got} fused launches a frame, not {per_frame}"
            for aa in (AaConfig.Msaa16, AaConfig.Area):
                compare_frame(engine, packed, layout, W, H, BLACK, aa, f"{name}_{label}_{int(aa)}", tol=1 if aa == AaConfig.Area else 0, oracle=oracle)
    finally:
        engine.set_debug_flags()


def check_front_max_draw_objects(engine, stacked, name):
    """FRONT_MAX_DRAW_OBJECTS - 1 / at / + 1 draw objects of three tags each (well under FRONT_MAX_TAGS): the front stages share two
    launches up to the limit and none beyond it."""
    c = engine.stage_constants()
    scenes = []
    for n in (c["front_max_draw_objects"] - 1, c["front_max_draw_objects"], c["front_max_draw_objects"] + 1):
        packed, layout = draw_scene(n, stacked).resolve()
        assert layout.n_draw_objects == n and layout.n_paths == n
        assert len(tag_bytes(packed, layout)[0]) <= c["front_max_tags"], "the tag limit would decide, not the draw-object limit"
        scenes.append((str(n), packed, layout, 2 if n <= c["front_max_draw_objects"] else 0))
    _front_switch(engine, name, scenes)


def check_front_max_tags(engine, name):
    """A padded tag stream of exactly FRONT_MAX_TAGS tags against one flatten block more, both under FRONT_MAX_DRAW_OBJECTS."""
    from vello_amd import Scene

    c = engine.stage_constants()
    scenes = []
    for n_tags, per_frame in ((c["front_max_tags"], 2), (c["front_max_tags"] + 1, 0)):
        s = Scene()
        k = filler_prefix(s, n_tags - 15)
        for i in range(3):
            _filler(s, k + i, True)
        assert _n_tags(s) == n_tags
        packed, layout = s.resolve()
        t, live = tag_bytes(packed, layout)
        assert live == n_tags and layout.n_draw_objects <= c["front_max_draw_objects"]
        assert len(t) == (c["front_max_tags"] if per_frame else c["front_max_tags"] + c["flatten_block_tags"]), len(t)
        scenes.append((str(len(t)), packed, layout, per_frame))
    _front_switch(engine, name, scenes)


def spare_path_data(packed, layout, n):
    """Scene.resolve()'s bytes with n unused words behind the path data (n == 0: the bytes and the layout as they are)."""
    w = np.ascontiguousarray(packed, dtype=np.uint8).view(np.uint32)
    out = np.concatenate([w[: layout.draw_tag_base], np.zeros(n, dtype=np.uint32), w[layout.draw_tag_base:]]).view(np.uint8)
    return out, layout._replace(draw_tag_base=layout.draw_tag_base + n, draw_data_base=layout.draw_data_base + n, transform_base=layout.transform_base + n,
                                style_base=layout.style_base + n)


def check_front_tiny_segments(engine, name):
    """One closed polygon whose path data bounds its segments by exactly FRONT_TINY_SEGMENTS (everything up to tile_alloc is one
    launch), by one more and by two more (two launches).  The bound is the words of path data (engine.h flatten_n_seg_max): two a
    point, so the odd one is the polygon of the first case with one unused word behind its path data."""
    from vello_amd import Affine, BezPath, Fill, Scene

    c = engine.stage_constants()
    tiny = c["front_tiny_segments"]

    def polygon(points):
        p = BezPath()
        for i in range(points):
            a = 2.0 * np.pi * i / points
            r = 40.0 if i % 2 else 25.0
            xy = (64.0 + r * np.cos(a), 48.0 + r * np.sin(a))
            p.line_to(xy) if i else p.move_to(xy)
        p.close_path()
        s = Scene()
        s.fill(Fill.EvenOdd, Affine.IDENTITY, colour(3), None, p)
        return s.resolve()

    def seg_max(packed, layout):
        return min(len(tag_bytes(packed, layout)[0]), layout.draw_tag_base - layout.path_data_base)

    at = polygon(tiny // 2 - 1)  # (the closing line repeats the first point)
    same, same_layout = spare_path_data(*at, 0)
    assert np.array_equal(same, at[0]) and same_layout == at[1]
    scenes = []
    for packed, layout in (at, spare_path_data(*at, 1), polygon(tiny // 2)):
        n = seg_max(packed, layout)
        assert layout.n_clips == 0
        scenes.append((str(n), packed, layout, 1 if n <= tiny else 2))
    assert [int(sc[0]) for sc in scenes] == [tiny, tiny + 1, tiny + 2], [sc[0] for sc in scenes]
    _front_switch(engine, name, scenes)


# ---------------------------------------------------------------------------------------------------------------
# (c) Clips: parity.clip_partition_structures through compare_clip_stage
# ---------------------------------------------------------------------------------------------------------------
def check_clip_partition(engine, case, name):
    from tests.parity import clip_partition_structures

    part = engine.stage_constants()["clip_part"]
    label, ops, edge = list(clip_partition_structures(part))[case]
    layout = compare_clip_stage(engine, ops, np.random.default_rng(900 + case), f"{name}_{label}", oracle=make_oracle())
    assert layout.n_clips == len(ops), f"{name}_{label}: {layout.n_clips} clips for {len(ops)} operations"
    if edge is not None:  # the push at the last index of a partition, its pop at the first index of the next
        assert (edge + 1) % part == 0 and ops[edge] == 1 and ops[edge + 1] == -1


# ---------------------------------------------------------------------------------------------------------------
# (d) Lines and crossings
# ---------------------------------------------------------------------------------------------------------------
def line_scene(k):
    """k lines, each inside one tile of the 128 x 96 target: triangles and quadrilaterals stacked on the 48 tiles.  (k == 1, 2 and 5
    are no sum of threes and fours: k == 1 is a single line written out by hand, as pick_parity.check_soup_shapes has it.)"""
    from vello_amd import Affine, BezPath, Fill, Scene

    if k == 1:
        from tests.pick_parity import raw_scene

        return raw_scene([0x0D, 0x10], [20.0, 18.0, 26.0, 30.0], 1)
    assert k >= 3 and k not in (5,)
    n_quad = k % 3  # 4 q + 3 t == k
    n_tri = (k - 4 * n_quad) // 3
    s = Scene()
    for i in range(n_tri + n_quad):
        tile = i % 48
        x, y = 16.0 * (tile % 8) + 1.0 + (i // 48) % 4, 16.0 * (tile // 8) + 1.0 + (i // 192) % 4
        p = BezPath()
        p.move_to((x, y))
        p.line_to((x + 10.0, y + 2.0))
        if i >= n_tri:
            p.line_to((x + 9.0, y + 10.0))
        p.line_to((x + 2.0, y + 9.0))
        p.close_path()
        s.fill(Fill.EvenOdd if i % 2 else Fill.NonZero, Affine.IDENTITY, colour(i, 90), None, p)
    return s.resolve()


# 1, and C - 1 / C / C + 1 / 2 C + 1 for every chunk size of path_count and path_tiling's workgroup: (constant, multiple, offset)
LINE_COUNT_CASES = [(None, 0, 1)] + [(key, m, d) for key in ("path_count_chunk", "path_count_chunk_small", "path_count_chunk_in_flight", "path_tiling_workgroup")
                                     for m, d in ((1, -1), (1, 0), (1, 1), (2, 1))]


def check_lines(engine, case, name):
    """k lines and k crossings.  path_count's three forms by frame order, as test_emu_parity.path_count_both_forms selects them: the
    first frame after an upload (the soup's size unknown: the large chunks), the third (known to be small: the small chunks), the
    first frame after an upload with two frames in flight (the in-flight form) -- each frame's image and counters against the oracle;
    then every stage through compare_frame."""
    from vello_amd import AaConfig

    key, mult, delta = case
    k = (engine.stage_constants()[key] * mult if key else 0) + delta
    packed, layout = line_scene(k)
    engine.set_auto_grow(True)
    o = make_oracle()
    o.set_scene(packed, layout, W, H, BLACK, int(AaConfig.Msaa16))
    ref = o.render()
    ob = o.bump()
    assert ob["failed"] == 0 and ob["lines"] == k and ob["seg_counts"] == k, f"{name}: the oracle counts {ob}, not {k} lines and crossings"

    def frame(label):
        engine.render_resident(W, H, BLACK, AaConfig.Msaa16)
        engine.sync_frame(0)
        img = engine.read_buffer("output", np.uint8, W * H * 4).reshape(H, W, 4)
        bump = engine.bump()
        assert bump["failed"] == 0 and bump["lines"] == k and bump["seg_counts"] == k, f"{name}_{label}: {bump}"
        assert all(bump[key] == ob[key] for key in ("tile", "binning")), f"{name}_{label}: {bump} against {ob}"
        assert np.array_equal(img, ref), f"{name}_{label}: the image differs"

    engine.set_frames_in_flight(1)
    engine.upload_scene(packed, layout)
    for label in ("first", "second", "third"):
        frame(label)
    engine.set_frames_in_flight(2)
    try:
        engine.upload_scene(packed, layout)
        frame("in_flight")
    finally:
        engine.set_frames_in_flight(1)
    frames(engine, packed, layout, W, H, name, (AaConfig.Msaa16, AaConfig.Area), o)


# ---------------------------------------------------------------------------------------------------------------
# (e) Backdrop rectangles
# ---------------------------------------------------------------------------------------------------------------
BACKDROP_WIDTHS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513)


def backdrop_block_rows(c, width):
    """Rows per block of k_backdrop's scan: the largest power of two with block_rows * width <= backdrop_block_tiles, 1 from there on."""
    b = c["backdrop_block_tiles"]
    return 1 if width >= b else b >> (width - 1).bit_length()


# (width in tiles, height relative to four blocks of rows, small paths before the rectangle)
BACKDROP_CASES = [(w, rel, (i + rel + 1) % 4) for i, w in enumerate(BACKDROP_WIDTHS) for rel in (-1, 0, 1)]


def backdrop_height(c, width, rel):
    """Just below, at and above four blocks of rows -- the rows a workgroup's four waves take in one turn -- where that is at most 32
    rows; 1, 2 and 3 rows otherwise (a path one tile wide is skipped by the kernel: it has no blocks)."""
    rows = 4 * backdrop_block_rows(c, width) if width > 1 else 1 << 30
    return rows + rel if rows <= 32 else 2 + rel


def backdrop_scene(wt, ht, before):
    """`before` small fills, then ONE path spanning wt x ht tiles -- an outer contour, an inner contour of the same direction and a
    slanted contour of the opposite direction, so that backdrops of 2, 1 and -1 run along the rows and differ row by row -- filled
    once non-zero and once even-odd under a sub-pixel translation."""
    from vello_amd import Affine, BezPath, Fill, Rect, Scene

    s = Scene()
    for i in range(before):
        s.fill(Fill.NonZero, Affine.IDENTITY, colour(i, 120), None, Rect(3.0 + 5.0 * i, 2.0, 9.0 + 5.0 * i, 11.0))
    x1, y1 = 16.0 * wt - 1.5, 16.0 * ht - 1.5
    p = BezPath()
    for inset in (1.0, 4.5):
        p.move_to((inset, inset))
        p.line_to((x1 - inset, inset))
        p.line_to((x1 - inset, y1 - inset))
        p.line_to((inset, y1 - inset))
        p.close_path()
    # the other way round, from the top right to the bottom left: its left edge crosses every row at another tile
    p.move_to((0.75 * x1, 2.0))
    p.line_to((0.25 * x1 - 6.0, y1 - 2.0))
    p.line_to((0.5 * x1, y1 - 2.0))
    p.line_to((x1 - 3.0, 2.0))
    p.close_path()
    s.fill(Fill.NonZero, Affine.IDENTITY, colour(7, 140), None, p)
    s.fill(Fill.EvenOdd, Affine.translate(0.3, 0.4), colour(8, 140), None, p)
    return s.resolve()


def check_backdrop(engine, case, name, in_flight=1):
    from vello_amd import AaConfig

    c = engine.stage_constants()
    wt, rel, before = case
    ht = backdrop_height(c, wt, rel)
    packed, layout = backdrop_scene(wt, ht, before)
    n = before + 2
    assert layout.n_draw_objects == n
    w, h = wt * 16 + (5 if (wt + rel) % 2 else 0), ht * 16
    frames(engine, packed, layout, w, h, f"{name}_{wt}x{ht}", (AaConfig.Msaa8,), make_oracle(), in_flight)
    p = engine.read_buffer("paths", np.uint32, n * 32).reshape(-1, 8)
    for i in (before, before + 1):
        assert (int(p[i, 2] - p[i, 0]), int(p[i, 3] - p[i, 1])) == (wt, ht), f"{name}: path {i} spans {p[i, :4]}, not {wt} x {ht} tiles"
    t = engine.read_buffer("tiles", np.int32, int(p[before, 4] + wt * ht) * 8).reshape(-1, 2)[int(p[before, 4]):, 0]
    if wt >= 8:
        assert len(set(t.tolist())) >= 3, f"{name}: the rows hold backdrops {sorted(set(t.tolist()))} only"
    return n % 4


# ---------------------------------------------------------------------------------------------------------------
# (f) Bins
# ---------------------------------------------------------------------------------------------------------------
# one below / at / one above the bins k_coarse's grid is rounded to, and the bins a binning workgroup takes a thread each (more: it loops)
BIN_COUNT_CASES = [(key, 1, d) for key in ("coarse_grid_bins", "draw_workgroup") for d in (-1, 0, 1)]


def check_bins(engine, case, name):
    """A target one bin high and n_bins wide (the cheapest factorisation), crossed by one long translucent rectangle, with a few small
    fills in the last bin."""
    from vello_amd import AaConfig, Affine, Fill, Rect, Scene

    n_bins = engine.stage_constants()[case[0]] * case[1] + case[2]
    w, h = n_bins * 256, 16
    s = Scene()
    s.fill(Fill.NonZero, Affine.IDENTITY, colour(1, 120), None, Rect(3.0, 2.0, w - 5.0, 13.0))
    for i in range(4):
        x = w - 250.0 + 60.0 * i
        s.fill(Fill.EvenOdd if i % 2 else Fill.NonZero, Affine.IDENTITY, colour(2 + i, 150), None, Rect(x, 1.0 + i, x + 40.0, 9.0 + i))
    packed, layout = s.resolve()
    o = make_oracle()
    frames(engine, packed, layout, w, h, name, (AaConfig.Msaa8,), o)
    cfg = o.config()  # (width_in_tiles, height_in_tiles first; the engine's Path boxes and bin lists were held to this oracle's)
    wb, hb = (int(cfg[0]) + 15) // 16, (int(cfg[1]) + 15) // 16
    assert wb * hb == n_bins, f"{name}: {wb} x {hb} bins, not {n_bins}"
    aligned = (n_bins + 255) // 256 * 256
    counts = engine.read_buffer("bin_headers", np.uint32, aligned * 8).reshape(-1, 2)[:n_bins, 0]
    assert (counts >= 1).all() and counts[-1] == 5, f"{name}: bin element counts {counts[:3]} .. {counts[-3:]}"
