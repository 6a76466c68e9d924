"""The scene index (vello_hip_scene_index_builds): frames of a resident scene that read the index its upload built against
the same frames with VELLO_HIP_DEBUG_NO_SCENE_INDEX -- the per-frame zero fill, pathtag scan and whole-stream light pass -- and against
the CPU oracle.  The scenes are the smallest that are indexed at all: just past VELLO_HIP_SHAPE_FRONT_MAX_TAGS, five scan partitions.
Shared by the emulated suite (test_scene_index_emu.py) and the GPU's (test_scene_index_gpu.py)."""
import functools

import numpy as np

from oracle.oracle import Oracle
from tests import parity
from tests.parity import BUMP_KEYS, canonical_nan_lines, sorted_rows
from tests.view_parity import render_frame_into, render_resident_into

W = H = 256
BLACK, WHITE = 0xFF000000, 0xFFFFFFFF
MIN_TAGS = 17500  # past FRONT_MAX_TAGS (16 384): 5 partitions of 4 096 tags, 18 light-pass blocks of 1 024


def make_oracle():
    return Oracle(capacity_scale=4, auto_grow=True)


def _n_tags(s):
    return s._lib.vh_scene_stream_bytes(s._h, 0)


def mixed_scene(seed, fills=True, strokes=True, unclosed=False, swap=False):
    """Filled polygons, filled cubics, stroked polylines and stroked curves of random lengths (so paths straddle the 4 096-tag
    partitions and the 1 024-tag flatten blocks wherever they fall), small shapes on a 256 x 256 target.  Paths come in pairs of one
    verb sequence: the first is filled and the second stroked -- swap: the other way round, so the scene has the same layout numbers
    and every list of the index is another; fills / strokes leave a kind out (both paths of a pair are then of the one that is left).
    unclosed: the scene lies inside a layer that is never popped (resolve appends a PATH marker beyond n_paths for it)."""
    from vello_amd import Affine, BezPath, Cap, Color, Fill, Join, Mix, Rect, Scene, Stroke

    rng = np.random.default_rng(seed)
    s = Scene()
    k = 0
    if unclosed:
        s.push_layer(Fill.NonZero, Mix.Normal, 0.8, Affine.IDENTITY, Rect(10.0, 10.0, 240.0, 230.0))
    while _n_tags(s) < MIN_TAGS:
        curves = rng.uniform() < 0.4
        verbs = [int(rng.integers(0, 2)) if curves else -1 for _ in range(int(rng.integers(2, 19)))]
        closed = rng.uniform() < 0.5
        for half in range(2):
            cx, cy = rng.uniform(-6.0, W + 6.0, 2)
            r = float(rng.uniform(1.5, 9.0))
            p = BezPath()
            p.move_to((float(cx), float(cy)))
            x, y = cx, cy
            for v in verbs:
                d = rng.uniform(-r, r, 6)
                if v < 0:
                    x, y = x + d[0], y + d[1]
                    p.line_to((float(x), float(y)))
                elif v == 0:
                    p.quad_to((float(x + d[0]), float(y + d[1])), (float(x + d[2]), float(y + d[3])))
                    x, y = x + d[2], y + d[3]
                else:
                    p.curve_to((float(x + d[0]), float(y + d[1])), (float(x + d[2]), float(y + d[3])), (float(x + d[4]), float(y + d[5])))
                    x, y = x + d[4], y + d[5]
            if closed:
                p.close_path()
            col = Color(float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), float(rng.uniform(0.3, 1)))
            xf = Affine.IDENTITY if k % 5 else Affine.translate(float(rng.uniform(-2, 2)), float(rng.uniform(-2, 2)))
            st = Stroke(float(rng.uniform(0.4, 2.5)), join=Join(k % 3), start_cap=Cap((k // 3) % 3), end_cap=Cap((k // 9) % 3))
            fill = fills and (not strokes or (half == 0) != swap)
            if fill:
                s.fill(Fill.EvenOdd if (k // 2) % 2 else Fill.NonZero, xf, col, None, p)
            else:
                s.stroke(st, xf, col, None, p)
            k += 1
    return s


def list_lengths(packed, layout):
    """(fill segment tags, stroked tags that are not lines, stroked lines) of a packed scene, by the rule of flatten's light pass: a
    segment tag is stroked when the style in force at it has STYLE_FLAGS_STYLE set."""
    b = np.ascontiguousarray(packed, dtype=np.uint8)
    w = b.view(np.uint32)
    tags = b[layout.path_tag_base * 4: layout.path_data_base * 4]
    seg = tags & 3
    style_ix = np.cumsum((tags & 0x40) != 0) - 1  # (inclusive: a marker's own style; segment tags carry no marker)
    flags = w[layout.style_base + np.maximum(style_ix, 0) * 2]
    stroked = (flags & np.uint32(0x80000000)) != 0
    is_seg = seg != 0
    return int((is_seg & ~stroked).sum()), int((is_seg & stroked & (seg != 1)).sum()), int((is_seg & stroked & (seg == 1)).sum())


@functools.lru_cache(maxsize=None)
def case_scene(which):
    """(packed, layout) of a named case, resolved once per process."""
    if which == "mixed":
        packed, layout = mixed_scene(1).resolve()
    elif which == "mixed_swapped":
        packed, layout = mixed_scene(1, swap=True).resolve()
    elif which == "fills_only":
        packed, layout = mixed_scene(2, strokes=False).resolve()
    elif which == "strokes_only":
        packed, layout = mixed_scene(3, fills=False).resolve()
    elif which == "unclosed_layer":
        packed, layout = mixed_scene(4, unclosed=True).resolve()
    elif which == "spare_paths":  # the layout counts paths beyond the stream's last PATH marker
        packed, layout = mixed_scene(5).resolve()
        layout = layout._replace(n_paths=layout.n_paths + 37)
    else:
        raise KeyError(which)
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    n_tags = (layout.path_data_base - layout.path_tag_base) * 4
    assert n_tags > 16384 and -(-n_tags // 4096) == 5, (which, n_tags)
    nf, ns, nl = list_lengths(packed, layout)
    for n in (nf, ns, nl):
        assert n == 0 or (n % 64 != 0 and n % 256 != 0), (which, nf, ns, nl)
    if which == "fills_only":
        assert ns == 0 and nl == 0 and nf > 0
    elif which == "strokes_only":
        assert nf == 0 and ns > 0 and nl > 0
    else:
        assert nf > 0 and ns > 0 and nl > 0
    return packed, layout


CASES = ("mixed", "fills_only", "strokes_only", "unclosed_layer", "spare_paths")


def snapshot(engine, layout, w=W, h=H, image=None):
    """What a finished frame left in the newest lane: bump counters, flatten's list lengths, tag monoids, path boxes, the soup."""
    b = engine.bump()
    n_tw = layout.path_data_base - layout.path_tag_base
    ctl = engine.control_words()
    return {
        "bump": b,
        "heavy_count": [int(v) for v in ctl[10:13]],
        "tag_monoids": engine.read_buffer("tag_monoids", np.uint32, n_tw * 20).copy(),
        "path_bboxes": engine.read_buffer("path_bboxes", np.int32, layout.n_paths * 24).copy(),
        "lines": sorted_rows(canonical_nan_lines(engine.read_buffer("lines", np.uint32, min(b["lines"], engine.capacities()["lines"]) * 24)), 6),
        "image": engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4).copy() if image is None else image,
    }


def assert_same(name, a, b, segments_exact=True):
    keys = [k for k in BUMP_KEYS if segments_exact or k not in ("segments", "ptcl")]
    assert all(a["bump"][k] == b["bump"][k] for k in keys), f"{name}: bump counters {a['bump']} vs {b['bump']}"
    assert a["heavy_count"] == b["heavy_count"], f"{name}: flatten's list lengths {a['heavy_count']} vs {b['heavy_count']}"
    assert np.array_equal(a["tag_monoids"], b["tag_monoids"]), f"{name}: tag monoids differ"
    assert np.array_equal(a["path_bboxes"], b["path_bboxes"]), f"{name}: path boxes differ"
    assert np.array_equal(a["lines"], b["lines"]), f"{name}: the soups differ as multisets"
    assert np.array_equal(a["image"], b["image"]), f"{name}: images differ"


def resident_frame(engine, layout, aa, indexed, n_frames=1, make_target=None, to_numpy=None):
    """n_frames frames of the resident scene enqueued back to back (into targets of their own when there are several), waited for;
    returns the newest frame's snapshot and every frame's image."""
    engine.update_debug_flags(no_scene_index=not indexed)
    targets = [make_target(W, H) for _ in range(n_frames)] if make_target else []
    for k in range(n_frames):
        if targets:
            render_resident_into(engine, W, H, BLACK, aa, targets[k])
        else:
            engine.render_resident(W, H, BLACK, aa)
    assert engine.sync() == 0, engine.bump()
    images = [to_numpy(t).copy() for t in targets]
    return snapshot(engine, layout, image=images[-1] if images else None), images


# ---------------------------------------------------------------------------------------------------------------
# 1. Indexed against NO_SCENE_INDEX on the same scene, and against the oracle
# ---------------------------------------------------------------------------------------------------------------
def check_twin(engine, which, kernels, in_flight, name, make_target, to_numpy, back_half=True):
    """back_half=False (the emulated suite, where a frame takes seconds): the oracle comparison stops at the image -- nothing behind
    the soup reads the index -- and only the MSAA twins are enqueued in_flight at a time."""
    from vello_amd import AaConfig

    packed, layout = case_scene(which)
    engine.set_auto_grow(True)
    try:
        engine.set_debug_flags(stroke_kernel=True, **{kernels: True})
        engine.set_frames_in_flight(in_flight)
        # against the oracle, through the blocking entry point (its upload builds the index)
        before = engine.scene_index_builds()
        for aa in (AaConfig.Msaa16, AaConfig.Area):
            # (inside a layer a last-ulp difference of an area is amplified by the un-premultiplication at its end: the area-AA
            # image is then held to the oracle's fine on the engine's own segment order, as compare_frame documents)
            parity.compare_frame(engine, packed, layout, W, H, BLACK, aa, f"{name}_{int(aa)}", tol=1 if aa == AaConfig.Area else 0, oracle=make_oracle(),
                                 order_sensitive=aa == AaConfig.Area and layout.n_clips != 0, back_half=back_half)
        assert engine.scene_index_builds() > before, f"{name}: the scene was not indexed"
        # against its twin, as resident frames: in_flight frames back to back, the newest one's buffers
        engine.upload_scene(packed, layout)
        for aa in (AaConfig.Msaa16, AaConfig.Area):
            n_frames = in_flight if back_half or aa != AaConfig.Area else 1
            a, ia = resident_frame(engine, layout, aa, True, n_frames, make_target, to_numpy)
            b, ib = resident_frame(engine, layout, aa, False, n_frames, make_target, to_numpy)
            # (area AA sums a tile's segments in soup order, which no two frames share: MSAA images are the exact ones)
            # (and inside a layer that difference is amplified without bound: there the oracle's fine on the frame's own order, above,
            # is the check of the area-AA image)
            if aa == AaConfig.Area:
                if layout.n_clips == 0:
                    assert np.abs(a["image"].astype(int) - b["image"].astype(int)).max() <= 1, f"{name}: area-AA images"
                b["image"] = a["image"]
            assert_same(f"{name}_{int(aa)}", a, b)
            if aa != AaConfig.Area:
                for k in range(len(ia)):
                    assert np.array_equal(ia[k], ib[k]) and np.array_equal(ia[k], ia[0]), f"{name}: frame {k} of {in_flight} in flight"
    finally:
        engine.set_frames_in_flight(1)
        engine.set_debug_flags()
        engine.set_auto_grow(False)


# ---------------------------------------------------------------------------------------------------------------
# 2. One index, many frames: views, culling
# ---------------------------------------------------------------------------------------------------------------
def check_many_frames(engine, name):
    from vello_amd import AaConfig, Affine

    packed, layout = case_scene("mixed")
    views = [None, Affine.translate(-60.0, -45.0) * Affine.scale(1.5), Affine.rotate(0.3) * Affine.translate(20.0, -30.0)]
    engine.set_auto_grow(True)
    try:
        engine.set_debug_flags(stroke_kernel=True)
        before = engine.scene_index_builds()
        engine.upload_scene(packed, layout)
        for cull in (False, True):
            engine.set_viewport_cull(cull)
            for k, v in enumerate(views):
                engine.set_view_transform(v)
                a, _ = resident_frame(engine, layout, AaConfig.Msaa16, True)
                b, _ = resident_frame(engine, layout, AaConfig.Msaa16, False)
                assert a["bump"]["failed"] == 0 and a["bump"]["lines"] > 0
                assert_same(f"{name}_view{k}_cull{int(cull)}", a, b)
        assert engine.scene_index_builds() == before + 1, f"{name}: {engine.scene_index_builds() - before} index builds for one upload"
    finally:
        engine.set_view_transform(None)
        engine.set_viewport_cull(False)
        engine.set_debug_flags()
        engine.set_auto_grow(False)


# ---------------------------------------------------------------------------------------------------------------
# 3. Invalidation
# ---------------------------------------------------------------------------------------------------------------
def check_invalidation(engine, fresh_engine, name, make_target, to_numpy):
    import workloads
    from vello_amd import AaConfig, FragmentLibrary

    pa, la = case_scene("mixed")
    pb, lb = case_scene("mixed_swapped")
    assert tuple(la) == tuple(lb) and not np.array_equal(pa, pb), "B must have A's layout numbers"
    aa = AaConfig.Msaa16
    small, small_layout = workloads.random_test_scene(5, n_paths=60, size=float(W), strokes=True, clips=True).resolve()
    small = np.ascontiguousarray(small, dtype=np.uint8)
    o = Oracle()
    o.set_scene(small, small_layout, W, H, BLACK, int(aa))
    small_ref = o.render().copy()
    for e in (engine, fresh_engine):
        e.set_auto_grow(True)
        e.set_debug_flags(stroke_kernel=True)
    try:
        fresh_engine.upload_scene(pb, lb)
        want, _ = resident_frame(fresh_engine, lb, aa, True)
        before = engine.scene_index_builds()
        engine.upload_scene(pa, la)
        a, _ = resident_frame(engine, la, aa, True)
        engine.upload_scene(pb, lb)
        b, _ = resident_frame(engine, lb, aa, True)
        assert engine.scene_index_builds() == before + 2, f"{name}: {engine.scene_index_builds() - before} builds for two uploads"
        assert_same(f"{name}_B", b, want)
        assert not np.array_equal(a["image"], b["image"])
        # a write into the resident scene's bytes drops the index: the frames behind it are the per-frame path's, and still right
        engine.write_buffer("scene", pb[:64].copy())
        c, _ = resident_frame(engine, lb, aa, True)
        assert_same(f"{name}_after_write", c, want)
        assert engine.scene_index_builds() == before + 2
        # frames of private scenes and of instances between resident ones: each is what it is without them
        lib = FragmentLibrary([mixed_scene(1)])
        assert np.array_equal(lib.packed, pa)
        engine.set_frames_in_flight(3)
        lib.upload(engine)
        assert engine.scene_index_builds() == before + 3
        t = [make_target(W, H) for _ in range(6)]
        ident = [(0, (1.0, 0.0, 0.0, 1.0, 0.0, 0.0))]
        render_resident_into(engine, W, H, BLACK, aa, t[0])
        render_frame_into(engine, small, small_layout, W, H, BLACK, aa, t[1])
        render_resident_into(engine, W, H, BLACK, aa, t[2])
        engine.render_instances(ident, W, H, BLACK, aa, out=t[3])
        render_resident_into(engine, W, H, BLACK, aa, t[4])
        render_frame_into(engine, small, small_layout, W, H, BLACK, aa, t[5])
        assert engine.sync() == 0
        for k in (0, 2, 3, 4):
            assert np.array_equal(to_numpy(t[k]), a["image"]), f"{name}: frame {k} of the interleaved run is not scene A"
        for k in (1, 5):
            assert np.array_equal(to_numpy(t[k]), small_ref), f"{name}: private frame {k} of the interleaved run"
        assert engine.scene_index_builds() == before + 3
    finally:
        for e in (engine, fresh_engine):
            e.set_frames_in_flight(1)
            e.set_debug_flags()
            e.set_auto_grow(False)


# ---------------------------------------------------------------------------------------------------------------
# 4. First frames after an upload, back to back on three lanes
# ---------------------------------------------------------------------------------------------------------------
def check_first_frames(engine, name, make_target, to_numpy):
    from vello_amd import AaConfig

    packed, layout = case_scene("mixed")
    engine.set_auto_grow(True)
    try:
        engine.set_debug_flags(stroke_kernel=True)
        engine.set_frames_in_flight(3)
        ref = None
        for rnd in range(2):
            engine.upload_scene(packed, layout)  # (what earlier frames told of the scene is forgotten: these are first frames)
            _, images = resident_frame(engine, layout, AaConfig.Msaa16, True, 3, make_target, to_numpy)
            ref = images[0] if ref is None else ref
            for k, img in enumerate(images):
                assert np.array_equal(img, ref), f"{name}: round {rnd}, frame {k}"
        b, _ = resident_frame(engine, layout, AaConfig.Msaa16, False, 1, make_target, to_numpy)
        assert np.array_equal(b["image"], ref), f"{name}: the unindexed frame"
    finally:
        engine.set_frames_in_flight(1)
        engine.set_debug_flags()
        engine.set_auto_grow(False)


# ---------------------------------------------------------------------------------------------------------------
# 5. An overrunning tag stream
# ---------------------------------------------------------------------------------------------------------------
def check_overrun(engine, name):
    import vello_amd
    from vello_amd import AaConfig

    packed, layout = case_scene("mixed")
    bad = packed.copy()
    bad[layout.path_tag_base * 4: layout.path_data_base * 4] = 0x0B  # every tag a f32 cubic: more path data than the stream holds
    try:
        engine.upload_scene(bad, layout)  # (the verdict is the scan's: the upload itself succeeds, as it does without an index)
        got = {}
        for indexed in (True, False):
            engine.update_debug_flags(no_scene_index=not indexed)
            frames = []
            for k in range(2):
                engine.render_resident(W, H, BLACK, AaConfig.Msaa16)
                r = engine.sync()
                err = engine._lib.vello_hip_last_error(engine._h)
                frames.append((r, err, engine.bump(), [int(v) for v in engine.control_words()[10:14]]))
            got[indexed] = frames
        for k in range(2):
            assert got[True][k][0] == got[False][k][0] == -1, f"{name}: frame {k}: {got[True][k][0]}, {got[False][k][0]}"
            assert got[True][k][1] == got[False][k][1], f"{name}: frame {k}: the messages differ"
            assert got[True][k][2] == got[False][k][2], f"{name}: frame {k}: bump {got[True][k][2]} vs {got[False][k][2]}"
            assert got[True][k][3] == got[False][k][3] == [0, 0, 0, 0], f"{name}: frame {k}: flatten's lists {got[True][k][3]} vs {got[False][k][3]}"
        with __import__("pytest").raises(vello_amd.VelloHipError):
            engine.render(bad, layout, W, H, BLACK, AaConfig.Msaa16)
    finally:
        engine.set_debug_flags()
    # the context is not poisoned
    parity.compare_frame(engine, packed, layout, W, H, BLACK, AaConfig.Msaa16, f"{name}_after", oracle=make_oracle(), back_half=False)
