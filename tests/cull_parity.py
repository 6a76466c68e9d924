"""Viewport culling (vello_hip_set_viewport_cull) against the CPU oracle.  The oracle has no such option: the expected soup S is
the oracle's soup R filtered by the rule in numpy; everything else -- path boxes in front of the soup, backdrops, counts, PTCL,
segments and the image behind it -- must be what the oracle computes from the WHOLE soup."""
import collections
import os

import numpy as np

from oracle.oracle import Oracle
from tests import parity
from tests.parity import BUMP_KEYS, canonical_nan_lines, canonical_nan_words, sorted_rows

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


STAGING_LINES = 1536  # flatten.hip: the smallest staging area that can run over (FLATTEN_STROKE_ROUND_LINES; a heavy workgroup stages 2 816)


def cullable(rows, width, height):
    """The rule of include/vello_hip.h, in f32 with exactly its comparisons: rows are LineSoup records (u32 x 6)."""
    f = np.ascontiguousarray(rows).reshape(-1, 6)[:, 2:].view(np.float32)
    S = np.float32(0.0625)
    wt, ht = np.float32((width + 15) // 16), np.float32((height + 15) // 16)
    zero = np.float32(0.0)
    with np.errstate(all="ignore"):
        x0, y0, x1, y1 = f[:, 0] * S, f[:, 1] * S, f[:, 2] * S, f[:, 3] * S
        return ((y0 >= ht) & (y1 >= ht)) | ((y0 <= zero) & (y1 <= zero)) | ((x0 >= wt) & (x1 >= wt))


def view_of(scene, dx, dy, zoom=1.0):
    """`scene` panned by (dx, dy) and scaled: what a window at (dx, dy) of the zoomed content shows."""
    from vello_amd import Affine, Scene

    s = Scene()
    s.append(scene, Affine.translate(-dx, -dy) * Affine.scale(zoom))
    return s


def tiger():
    from vello_amd import Layout

    d = np.load(os.path.join(GOLD, "tiger_scene.npz"))
    return d["packed"], Layout(*[int(v) for v in d["layout"]])


def _counter(rows):
    return collections.Counter(r.tobytes() for r in np.ascontiguousarray(rows).reshape(-1, 6))


def soup_between(name, soup, S, R):
    """S <= soup <= R as multisets of (NaN-canonical) rows."""
    cs, csoup, cr = _counter(S), _counter(soup), _counter(R)
    assert not (cs - csoup), f"{name}: {sum((cs - csoup).values())} lines the rule keeps are missing from the soup"
    assert not (csoup - cr), f"{name}: {sum((csoup - cr).values())} lines of the soup are not the reference's"


def oracle_soup(oracle, width, height):
    """(R, S) of the oracle's last frame, NaN-canonical rows."""
    n = oracle.bump()["lines"]
    R = canonical_nan_lines(oracle.buffer("lines", np.uint32)[: n * 6])
    return R, R[~cullable(R, width, height)]


def engine_soup(engine, n):
    return canonical_nan_lines(engine.read_buffer("lines", np.uint32, n * 24))


def compare_culled_frame(engine, packed, layout, width, height, base_color, aa, name, tol=0, oracle=None, resolved=None,
                         exact_soup=True, require_culling=True, order_sensitive=False, back_half=True, stats=None):
    """Points 1-4 of the option's contract (include/vello_hip.h).  exact_soup=False is for the case in which a piece bypasses
    flatten's staging area: S <= soup <= R.  exact_soup=None (the extreme fuzzer, whose curves between points at 1e4 ... 3e38 are single
    pieces of tens of thousands of lines): exact unless the frame has more lines than a heavy workgroup's staging area holds
    (STAGING_LINES) -- with fewer, no piece can have bypassed it.  Leaves the option off.  Returns (img, ref, bump, |R|, |S|)."""
    oracle = oracle or Oracle()
    oracle.set_scene(packed, layout, width, height, base_color, int(aa))
    ramps = None
    if resolved is not None:
        ramps = resolved.ramps
        oracle.set_ramps(ramps)
        oracle.set_image_atlas(resolved.atlas_image())
        if resolved.atlas_size:
            engine.resize_image_atlas(resolved.atlas_size, resolved.atlas_size)
            for x, y, px in resolved.uploads:
                engine.write_image(x, y, px)
    ref = oracle.render()
    ob = oracle.bump()
    assert ob["failed"] == 0, f"{name}: the oracle's pools overflow: {ob}"
    R, S = oracle_soup(oracle, width, height)
    if require_culling:
        assert len(S) < len(R), f"{name}: nothing to cull ({len(R)} lines)"
    if exact_soup is None:
        exact_soup = len(R) <= STAGING_LINES
    L = layout
    engine.set_viewport_cull(True)
    try:
        img, bump = engine.render(packed, layout, width, height, base_color, aa, ramps=ramps)
        print(f"{name}: lines {len(R)} -> rule keeps {len(S)}, engine {bump['lines']}")
        if stats is not None:
            stats.update(R=len(R), S=len(S), soup=bump["lines"])
        # point 2 and 4: the count
        if exact_soup:
            assert bump["lines"] == len(S), f"{name}: bump.lines {bump['lines']}, the rule keeps {len(S)} of {len(R)}"
        else:
            assert len(S) <= bump["lines"] <= len(R), f"{name}: bump.lines {bump['lines']} outside [{len(S)}, {len(R)}]"
        assert bump["failed"] == 0, f"{name}: {bump}"
        # point 3 (counters): as compare_frame -- coarse's occlusion culling may only shrink segments / ptcl without clips
        exact = [k for k in BUMP_KEYS if k not in ("segments", "ptcl", "lines")]
        ok = all(bump[k] == ob[k] for k in exact) and bump["segments"] <= ob["segments"]
        if L.n_clips != 0:
            ok = ok and bump["segments"] == ob["segments"]
        assert ok, f"{name}: bump counters differ: hip {bump} oracle {ob}"
        # point 1: everything in front of the soup
        n_tw = L.path_data_base - L.path_tag_base
        assert np.array_equal(engine.read_buffer("tag_monoids", np.uint32, n_tw * 20), oracle.buffer("tag_monoids", np.uint32)[: n_tw * 5]), f"{name}: tag_monoids differ"
        assert np.array_equal(engine.read_buffer("path_bboxes", np.int32, L.n_paths * 24), oracle.buffer("path_bboxes", np.int32)[: L.n_paths * 6]), \
            f"{name}: path_bboxes differ (they are the union of ALL lines, culled or not)"
        assert np.array_equal(engine.read_buffer("draw_monoids", np.uint32, L.n_draw_objects * 16), oracle.buffer("draw_monoids", np.uint32)[: L.n_draw_objects * 4]), \
            f"{name}: draw_monoids differ"
        assert np.array_equal(canonical_nan_words(engine.read_buffer("info_bin_data", np.uint32, L.bin_data_start * 4)),
                              canonical_nan_words(oracle.buffer("info_bin_data", np.uint32)[: L.bin_data_start])), f"{name}: draw info differs"
        if L.n_clips:
            assert np.array_equal(engine.read_buffer("clip_bboxes", np.uint32, L.n_clips * 16), oracle.buffer("clip_bboxes", np.uint32)[: L.n_clips * 4]), \
                f"{name}: clip_bboxes differ"
        assert np.array_equal(engine.read_buffer("draw_bboxes", np.uint32, L.n_draw_objects * 16), oracle.buffer("draw_bboxes", np.uint32)[: L.n_draw_objects * 4]), \
            f"{name}: draw_bboxes differ"
        p_h = engine.read_buffer("paths", np.uint32, L.n_draw_objects * 32).reshape(-1, 8)
        p_o = oracle.buffer("paths", np.uint32)[: L.n_draw_objects * 8].reshape(-1, 8)
        assert np.array_equal(p_h[:, :4], p_o[:, :4]), f"{name}: path tile bboxes differ"
        # point 2: the soup
        soup = engine_soup(engine, bump["lines"])
        if exact_soup:
            a, b = sorted_rows(soup, 6), sorted_rows(S, 6)
            assert np.array_equal(a, b), f"{name}: the soup is not the reference's filtered by the rule ({(a != b).any(axis=1).sum()} rows)"
        else:
            soup_between(name, soup, S, R)
        # point 3: backdrops per path
        t_h = engine.read_buffer("tiles", np.int32, ob["tile"] * 8).reshape(-1, 2)
        t_o = oracle.buffer("tiles", np.int32)[: ob["tile"] * 2].reshape(-1, 2)
        for i in range(L.n_draw_objects):
            n = int((p_o[i, 2] - p_o[i, 0]) * (p_o[i, 3] - p_o[i, 1]))
            assert not n or np.array_equal(t_h[p_h[i, 4]: p_h[i, 4] + n, 0], t_o[p_o[i, 4]: p_o[i, 4] + n, 0]), f"{name}: tile backdrops differ (path {i})"
        # point 3: the image, by compare_frame's rules
        diff = np.abs(img.astype(np.int32) - ref.astype(np.int32))
        if not order_sensitive:
            assert diff.max() <= tol, f"{name}: image differs from oracle: max {diff.max()}, {(diff > tol).sum()} values over tol {tol}"
        if tol > 0:
            n_tiles = ((width + 15) // 16) * ((height + 15) // 16)
            used = {"segments": bump["segments"] * 6, "ptcl": 64 * n_tiles + bump["ptcl"], "tiles": ob["tile"] * 2, "info_bin_data": L.bin_data_start + ob["binning"]}
            same_order = parity.fine_on_engine_inputs(engine, oracle, width, height, used)
            assert np.array_equal(img, same_order), f"{name}: fine differs from the oracle's fine on the same segment order"
            oracle.render()  # (the same-order check overwrote the oracle's tiles / PTCL / segments with the engine's)
        # point 3, the back half: coarse's occlusion culling off, so that every counter and record is the reference's
        if back_half:
            engine.update_debug_flags(no_cull=True)
            try:
                img2, b2 = engine.render(packed, layout, width, height, base_color, aa, ramps=ramps)
            finally:
                engine.update_debug_flags(no_cull=False)
            assert b2["lines"] == bump["lines"], f"{name}: bump.lines {b2['lines']} in the second frame, {bump['lines']} in the first"
            assert all(b2[k] == ob[k] for k in BUMP_KEYS if k not in ("ptcl", "lines")), f"{name}: bump counters differ with NO_CULL: hip {b2} oracle {ob}"
            n_tiles = ((width + 15) // 16) * ((height + 15) // 16)
            n_bin = parity.compare_bins(name, engine.read_buffer("bin_headers", np.uint32), engine.read_buffer("info_bin_data", np.uint32, (L.bin_data_start + ob["binning"]) * 4),
                                        oracle.buffer("bin_headers", np.uint32), oracle.buffer("info_bin_data", np.uint32), L.n_draw_objects, width, height, L.bin_data_start)
            assert n_bin == ob["binning"], f"{name}: bin lists hold {n_bin} entries, bump.binning {ob['binning']}"
            # (the ENGINE's soup for the engine's records: line_ix indexes the smaller soup)
            parity.compare_seg_counts(name, engine.read_buffer("seg_counts", np.uint32, ob["seg_counts"] * 8), engine.read_buffer("lines", np.uint32, b2["lines"] * 24),
                                      oracle.buffer("seg_counts", np.uint32), oracle.buffer("lines", np.uint32)[: ob["lines"] * 6], ob["seg_counts"])
            ptcl_h = engine.read_buffer("ptcl", np.uint32, (64 * n_tiles + b2["ptcl"]) * 4)
            fh, fo, fn, _ = parity.walk_ptcl_pair(name, ptcl_h, oracle.buffer("ptcl", np.uint32)[: 64 * n_tiles + ob["ptcl"]], n_tiles)
            assert int(fn.sum()) == ob["segments"], f"{name}: CMD_FILLs cover {int(fn.sum())} segments, bump.segments {ob['segments']}"
            parity.compare_segment_slices(name, engine.read_buffer("segments", np.uint32, ob["segments"] * 24), oracle.buffer("segments", np.uint32)[: ob["segments"] * 6], fh, fo, fn)
            if aa != 0:
                assert np.array_equal(img2, ref), f"{name}: image differs with NO_CULL"
    finally:
        engine.set_viewport_cull(False)
    return img, ref, bump, len(R), len(S)


def polygon_scene(seed=11, n=400, size=512.0):
    """Filled polygons and nothing else: every line leaves through flatten's light pass."""
    from vello_amd import Affine, BezPath, Color, Fill, Scene

    rng = np.random.default_rng(seed)
    s = Scene()
    for k in range(n):
        cx, cy = rng.uniform(-30, size + 30, 2)
        r = rng.uniform(3.0, size / 6)
        p = BezPath()
        m = int(rng.integers(3, 9))
        a = np.sort(rng.uniform(0, 2 * np.pi, m))
        p.move_to((float(cx + r * np.cos(a[0])), float(cy + r * np.sin(a[0]))))
        for t in a[1:]:
            p.line_to((float(cx + r * np.cos(t)), float(cy + r * np.sin(t))))
        p.close_path()
        s.fill(Fill.EvenOdd if k % 2 else Fill.NonZero, Affine.IDENTITY, Color(float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), float(rng.uniform(0.4, 1))), None, p)
    return s


def polyline_scene(seed=12, n=300, size=512.0):
    """Stroked open polylines (all joins and caps) and nothing else: the stroke workgroups' lines, or the heavy list's."""
    from vello_amd import Affine, BezPath, Cap, Color, Join, Scene, Stroke

    rng = np.random.default_rng(seed)
    s = Scene()
    for k in range(n):
        p = BezPath()
        x, y = rng.uniform(-30, size + 30, 2)
        p.move_to((float(x), float(y)))
        for _ in range(int(rng.integers(2, 12))):
            x, y = x + rng.uniform(-40, 40), y + rng.uniform(-40, 40)
            p.line_to((float(x), float(y)))
        st = Stroke(float(rng.uniform(0.5, 6.0)), join=Join(k % 3), start_cap=Cap((k // 3) % 3), end_cap=Cap((k // 9) % 3))
        s.stroke(st, Affine.IDENTITY, Color(float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), 1.0), None, p)
    return s


def boundary_scene(width, height):
    """Hand-made lines around the three culling edges of a width x height target: ends exactly on y == 16 ht, y == 0, x == 16 wt and
    one ulp inside each, horizontal lines lying on the top and bottom edges, lines wholly left of the target (they stay)."""
    from vello_amd import Affine, BezPath, Color, Fill, Scene, Stroke

    f32 = np.float32
    W, H = f32(16 * ((width + 15) // 16)), f32(16 * ((height + 15) // 16))
    below = lambda v: float(np.nextafter(f32(v), f32(-np.inf)))  # noqa: E731
    above = lambda v: float(np.nextafter(f32(v), f32(np.inf)))  # noqa: E731
    W, H = float(W), float(H)
    s = Scene()
    k = [0]

    def tri(a, b, c):
        p = BezPath()
        p.move_to(a)
        p.line_to(b)
        p.line_to(c)
        p.close_path()
        k[0] += 1
        s.fill(Fill.NonZero if k[0] % 2 else Fill.EvenOdd, Affine.IDENTITY, Color(0.2 + 0.1 * (k[0] % 7), 0.9 - 0.1 * (k[0] % 5), 0.5, 0.8), None, p)

    mx, my = W / 2, H / 2
    # bottom edge: on it, one ulp inside, one ulp outside; a horizontal line ON the edge
    tri((mx - 3, H), (mx + 3, H), (mx, H + 9))
    tri((mx - 3, below(H)), (mx + 3, H), (mx, H + 9))
    tri((mx - 3, above(H)), (mx + 3, above(H)), (mx, H + 9))
    tri((1.0, H), (W - 1, H), (mx, my))
    # top edge
    tri((mx - 3, 0.0), (mx + 3, 0.0), (mx, -9.0))
    tri((mx - 3, above(0.0)), (mx + 3, 0.0), (mx, -9.0))
    tri((mx - 3, 1e-41), (mx + 3, 0.0), (mx, -9.0))  # (a subnormal: times 0.0625 still positive or zero as f32 has it)
    tri((mx - 3, -0.0), (mx + 3, -0.0), (mx, -9.0))
    tri((1.0, 0.0), (W - 1, 0.0), (mx, my))
    # right edge
    tri((W, my - 3), (W, my + 3), (W + 9, my))
    tri((below(W), my - 3), (W, my + 3), (W + 9, my))
    tri((above(W), my - 3), (above(W), my + 3), (W + 9, my))
    tri((W, 1.0), (W, H - 1), (mx, my))
    # left of the target: kept, and its backdrops fill the rows
    tri((-20.0, 1.0), (-5.0, my), (-30.0, H - 1))
    tri((0.0, 1.0), (0.0, H - 1), (-9.0, my))
    # corners and far away
    tri((W, H), (W + 5, H + 5), (W, H + 9))
    tri((-5.0, -5.0), (W + 5, -5.0), (W + 5, H + 5))
    tri((-1e4, -1e4), (1e4, -1e4), (0.0, 1e4))
    p = BezPath()
    p.move_to((-8.0, my))
    p.line_to((W + 8, my))
    p.line_to((W + 8, H + 8))
    p.line_to((mx, -8.0))
    s.stroke(Stroke(3.0), Affine.IDENTITY, Color(1.0, 1.0, 1.0, 1.0), None, p)
    return s


# ---------------------------------------------------------------------------------------------------------------
# The cases, shared by the emulated suite (test_viewport_cull_emu.py) and the GPU's (test_viewport_cull_gpu.py)
# ---------------------------------------------------------------------------------------------------------------
BLACK, WHITE = 0xFF000000, 0xFFFFFFFF


def _aa_tol(aa):
    return 1 if int(aa) == 0 else 0


def check_light_pass(engine, name):
    """Line-only fills: every line is staged and flushed by flatten_light_workgroup (k_flatten_light)."""
    import workloads
    from vello_amd import AaConfig

    packed, layout = view_of(polygon_scene(), 205, 154).resolve()
    for aa in (AaConfig.Area, AaConfig.Msaa16):
        compare_culled_frame(engine, packed, layout, 175, 131, BLACK, aa, f"{name}_polygons_{int(aa)}", tol=_aa_tol(aa))
    packed, layout = view_of(workloads.random_test_scene(3, n_paths=300, size=512.0, strokes=False), 205, 154).resolve()
    compare_culled_frame(engine, packed, layout, 175, 131, BLACK, AaConfig.Msaa8, f"{name}_fills")


def check_stroked_polylines(engine, name, stroke_kernel):
    """Stroked polylines through the stroke workgroups (stroke_kernel=True: k_flatten_main's with one frame in flight,
    k_flatten_strokes with two) or as entries of the heavy list (flush_staged_lines in k_flatten_main / k_flatten_heavy)."""
    from vello_amd import AaConfig

    packed, layout = view_of(polyline_scene(), 205, 154).resolve()
    try:
        engine.set_debug_flags(stroke_kernel=stroke_kernel)
        compare_culled_frame(engine, packed, layout, 175, 131, WHITE, AaConfig.Area, f"{name}_1", tol=1)
        engine.set_frames_in_flight(2)
        compare_culled_frame(engine, packed, layout, 175, 131, WHITE, AaConfig.Msaa16, f"{name}_2inflight")
    finally:
        engine.set_frames_in_flight(1)
        engine.set_debug_flags()


def curve_views():
    """(name, scene, w, h): views into the middle of scenes of curves and stroked curves, targets that are not multiples of 16."""
    import workloads

    out = []
    for which in ("cardioid", "funky_paths", "tricky_strokes"):
        r = getattr(workloads, which + "_scene")()
        s, w, h = r if isinstance(r, tuple) else (r, 512, 512)
        # (pan to the centre at twice the size, half the target: lines above, below, right of and left of the window)
        out.append((which, view_of(s, w * 0.75, h * 0.75, 2.0), w // 2 - 3, h // 2 - 5))
    out.append(("stroke_styles", view_of(workloads.stroke_styles_scene(), 102, 77), 90, 67))
    return out


def check_curves(engine, name, case, which, in_flight=True):
    """Curves and stroked curves by both kernel sets of the heavy list (flatten_coop / flatten_alone), one and two frames in flight."""
    from vello_amd import AaConfig

    cname, scene, w, h = curve_views()[case]
    packed, layout = scene.resolve()
    try:
        engine.set_debug_flags(**{which: True})
        compare_culled_frame(engine, packed, layout, w, h, BLACK, AaConfig.Area, f"{name}_{cname}_{which}", tol=1)
        if in_flight:
            engine.set_frames_in_flight(2)
            compare_culled_frame(engine, packed, layout, w, h, BLACK, AaConfig.Msaa16, f"{name}_{cname}_{which}_2inflight")
    finally:
        engine.set_frames_in_flight(1)
        engine.set_debug_flags()


def random_views():
    import workloads

    s = workloads.random_test_scene(3, n_paths=300, size=512.0, strokes=True, clips=True)
    return [("pan", view_of(s, 205, 154), 175, 131), ("zoom", view_of(s, 614, 461, 3.0), 256, 249)]


def check_random_view(engine, name, case):
    """Fills, strokes (every style), curves and clip layers, a view into the middle of the content; with the stroke kernel forced as well,
    so that all three flush sites run in one frame."""
    from vello_amd import AaConfig

    cname, scene, w, h = random_views()[case]
    packed, layout = scene.resolve()
    try:
        compare_culled_frame(engine, packed, layout, w, h, BLACK, AaConfig.Msaa16, f"{name}_{cname}")
        engine.set_debug_flags(stroke_kernel=True)
        compare_culled_frame(engine, packed, layout, w, h, BLACK, AaConfig.Area, f"{name}_{cname}_strokekernel", tol=1)
        engine.set_frames_in_flight(2)
        compare_culled_frame(engine, packed, layout, w, h, BLACK, AaConfig.Msaa8, f"{name}_{cname}_strokekernel_2inflight")
    finally:
        engine.set_frames_in_flight(1)
        engine.set_debug_flags()


def check_small_scene_fusion(engine, name):
    """Small scenes: the light pass (and, below a few dozen segments, the heavy list) as turns of k_front; the same with every stage a
    kernel of its own."""
    import workloads
    from vello_amd import AaConfig

    cases = [("stroke_styles", view_of(workloads.stroke_styles_scene(), 102, 77), 90, 67, 2),
             ("clip_blend", view_of(workloads.clip_blend_scene(), 102, 77), 90, 67, 2),
             ("circle", view_of(workloads.circle_scene(), 128, 100), 120, 100, 1)]
    try:
        for cname, scene, w, h, per_frame in cases:
            packed, layout = scene.resolve()
            engine.set_debug_flags(flatten_coop=True)  # (pinned: the one-launch front needs the cooperative set, see parity.check_front_fusion)
            engine.set_viewport_cull(True)
            before = engine.fused_launches()
            engine.render(packed, layout, w, h, WHITE, AaConfig.Msaa16)
            assert engine.fused_launches() - before == per_frame, (cname, engine.fused_launches() - before, per_frame)
            compare_culled_frame(engine, packed, layout, w, h, WHITE, AaConfig.Msaa16, f"{name}_{cname}_fused")
            compare_culled_frame(engine, packed, layout, w, h, WHITE, AaConfig.Area, f"{name}_{cname}_fused_area", tol=1)
            engine.set_debug_flags(flatten_coop=True, no_fusion=True)
            before = engine.fused_launches()
            compare_culled_frame(engine, packed, layout, w, h, WHITE, AaConfig.Msaa16, f"{name}_{cname}_nofusion")
            assert engine.fused_launches() == before
    finally:
        engine.set_viewport_cull(False)
        engine.set_debug_flags()


def check_tiger(engine, name):
    from vello_amd import AaConfig

    packed, layout = tiger()
    compare_culled_frame(engine, packed, layout, 320, 320, WHITE, AaConfig.Msaa8, name)


def check_staging_bypass(engine, name):
    """The one case allowed the weaker soup assertion: a workgroup that emits more lines than its staging area holds writes the
    pieces beyond it straight to the soup, culled or not."""
    import workloads
    from vello_amd import AaConfig

    packed, layout = view_of(workloads.heavy_strokes_scene(), 410, 307).resolve()
    stats = {}
    compare_culled_frame(engine, packed, layout, 346, 259, BLACK, AaConfig.Msaa8, name, exact_soup=False, stats=stats)
    return stats


BOUNDARY_TARGETS = [(1, 1), (17, 33), (64, 64), (100, 52), (16, 16)]


def check_boundaries(engine, name):
    from vello_amd import AaConfig

    for w, h in BOUNDARY_TARGETS:
        packed, layout = boundary_scene(w, h).resolve()
        for aa in (AaConfig.Area, AaConfig.Msaa16):
            compare_culled_frame(engine, packed, layout, w, h, BLACK, aa, f"{name}_{w}x{h}_{int(aa)}", tol=_aa_tol(aa))


def check_fuzz(engine, name, seeds, extreme):
    """workloads.fuzz at 128 x 128 and 100 x 52; `extreme` has points at +-1e4 ... 3e38, on tile corners, NaN and inf."""
    import vello_amd
    from vello_amd import AaConfig
    from workloads.fuzz import fuzz_scene

    engine.set_auto_grow(True)
    n_culled = 0
    try:
        for seed in seeds:
            r = vello_amd.Resolver().resolve(fuzz_scene(seed, n_ops=14, extreme=True) if extreme else fuzz_scene(seed))
            aa = [AaConfig.Area, AaConfig.Msaa8, AaConfig.Msaa16][seed % 3]
            for w, h in ((128, 128), (100, 52)):
                _, _, _, nr, ns = compare_culled_frame(engine, r.packed, r.layout, w, h, [BLACK, WHITE, 0x00000000, 0x80FF8040][seed % 4], aa,
                                                       f"{name}_{seed}_{w}x{h}", tol=_aa_tol(aa), resolved=r, order_sensitive=True, require_culling=False,
                                                       back_half=not extreme, exact_soup=None if extreme else True, oracle=Oracle(capacity_scale=4, auto_grow=True))
                n_culled += nr - ns
    finally:
        engine.set_auto_grow(False)
    assert n_culled > 0, f"{name}: no seed had anything to cull"


def check_toggle_resident(engine, name):
    """off -> on -> off on one engine with one resident scene gives R, S, R; then, with two frames in flight and the option changed
    between two render_resident calls, each frame has the soup of its own setting."""
    import workloads
    from vello_amd import AaConfig

    w, h = 175, 131
    packed, layout = view_of(workloads.random_test_scene(3, n_paths=300, size=512.0, strokes=True, clips=True), 205, 154).resolve()
    o = Oracle()
    o.set_scene(packed, layout, w, h, BLACK, int(AaConfig.Msaa16))
    ref = o.render()
    R, S = oracle_soup(o, w, h)
    assert len(S) < len(R)
    want = {False: sorted_rows(R, 6), True: sorted_rows(S, 6)}

    def frame(on, what):
        engine.sync_frame(0)
        b = engine.bump()
        assert b["failed"] == 0 and b["lines"] == len(want[on]), f"{name} {what}: bump.lines {b['lines']}, expected {len(want[on])}"
        assert np.array_equal(sorted_rows(engine_soup(engine, b["lines"]), 6), want[on]), f"{name} {what}: soup"
        assert np.array_equal(engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4), ref), f"{name} {what}: image"

    try:
        engine.upload_scene(packed, layout)
        for k, on in enumerate((False, True, False, True, True, False)):
            engine.set_viewport_cull(on)
            engine.render_resident(w, h, BLACK, AaConfig.Msaa16)
            frame(on, f"frame {k} ({'on' if on else 'off'})")
        engine.set_frames_in_flight(2)
        for k in range(3):
            # two frames enqueued back to back, the setting changed in between: each keeps the one it was enqueued with
            first_on = k % 2 == 0
            engine.set_viewport_cull(first_on)
            engine.render_resident(w, h, BLACK, AaConfig.Msaa16)
            engine.set_viewport_cull(not first_on)
            engine.render_resident(w, h, BLACK, AaConfig.Msaa16)
            engine.sync_frame(1)
            frame(not first_on, f"in flight {k}, newest")
            # (read_buffer follows the newest lane: the older frame's lane becomes the newest again two frames on)
        assert engine.sync() == 0
    finally:
        engine.set_viewport_cull(False)
        engine.set_frames_in_flight(1)


def check_line_pool(make_engine, name):
    """A line pool of |S| + 64 elements and a line-only view (nothing bypasses staging): without the option the frame reports
    VELLO_HIP_E_CAPACITY with bump.lines == |R|, with it the frame is correct with bump.lines == |S|; with auto-grow both are correct."""
    from vello_amd import AaConfig

    w, h = 175, 131
    packed, layout = view_of(polygon_scene(), 205, 154).resolve()
    o = Oracle()
    o.set_scene(packed, layout, w, h, BLACK, int(AaConfig.Msaa16))
    ref = o.render()
    R, S = oracle_soup(o, w, h)
    assert len(S) + 64 < len(R)
    eng = make_engine({"lines": len(S) + 64})
    assert eng.capacities()["lines"] == len(S) + 64
    img, bump = eng.render(packed, layout, w, h, BLACK, AaConfig.Msaa16)
    assert bump["failed"] != 0 and bump["lines"] == len(R), f"{name}: option off: {bump}"
    assert eng.sync() == -4
    eng.set_viewport_cull(True)
    img, bump = eng.render(packed, layout, w, h, BLACK, AaConfig.Msaa16)
    assert bump["failed"] == 0 and bump["lines"] == len(S), f"{name}: option on: {bump}"
    assert np.array_equal(img, ref), f"{name}: image with the option on"
    assert eng.sync() == 0
    assert eng.capacities()["lines"] == len(S) + 64
    for on in (True, False):
        eng2 = make_engine({"lines": len(S) + 64})
        eng2.set_auto_grow(True)
        eng2.set_viewport_cull(on)
        img, bump = eng2.render(packed, layout, w, h, BLACK, AaConfig.Msaa16)
        assert bump["failed"] == 0 and bump["lines"] == (len(S) if on else len(R)), f"{name}: auto-grow, option {on}: {bump}"
        assert np.array_equal(img, ref), f"{name}: image with auto-grow, option {on}"


def check_renderer_option(name):
    """Through the public layer: Renderer(RendererOptions(viewport_cull=True)).render_to_texture gives the image it gives without
    the option, from fewer lines."""
    import vello_amd
    import workloads
    from vello_amd import AaConfig, Color, RendererOptions, RenderParams

    scene = view_of(workloads.random_test_scene(3, n_paths=300, size=512.0, strokes=True, clips=True), 205, 154)
    imgs, lines = [], []
    for on in (False, True):
        r = vello_amd.Renderer(RendererOptions(viewport_cull=on))
        for aa in (AaConfig.Msaa16, AaConfig.Area):
            out = np.zeros((131, 175, 4), dtype=np.uint8)
            r.render_to_texture(scene, out, RenderParams(Color.from_rgb8(0, 0, 0), 175, 131, aa))
            imgs.append(out)
            lines.append(r.last_bump()["lines"])
    assert np.array_equal(imgs[0], imgs[2]), f"{name}: MSAA16 image differs with the option"
    assert np.abs(imgs[1].astype(int) - imgs[3].astype(int)).max() <= 1, f"{name}: area-AA image differs with the option"
    assert lines[2] < lines[0] and lines[3] < lines[1], f"{name}: bump.lines {lines}"
