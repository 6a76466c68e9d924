"""Damage rectangles (vello_hip_set_damage_rect) against the CPU oracle.  The oracle has no such option and none is added: the
expectation is the oracle's WHOLE frame.  A frame with a rectangle R (W = the tiles that meet it) must put the whole frame's pixels
into R and leave every other byte of the target alone; everything ahead of coarse must be the whole frame's; behind it, the
command lists and segments of W's tiles must be the whole frame's and no tile outside W may get anything.

`mem` is where "device memory" lives (tests/placement_parity.py): HostMemory for the SIMT-emulated build, TorchMemory for the MI355X."""
import ctypes
import functools

import numpy as np
import pytest

from oracle.oracle import Oracle
from tests import cull_parity as cp
from tests import parity
from tests import placement_parity as plp
from tests.parity import BUMP_KEYS, CMD_BEGIN_CLIP, CMD_END, CMD_END_CLIP, CMD_JUMP, _CMD_SIZE, canonical_nan_lines, canonical_nan_words, sorted_rows

BLACK, WHITE = 0xFF000000, 0xFFFFFFFF
E_INVALID = -1
LEAD = plp.LEAD
BLEND_STACK_SPLIT = 4  # common.h / fine.wgsl: blend-stack entries a thread keeps in registers; deeper ones spill, 256 words a tile and level


# ---------------------------------------------------------------------------------------------------------------
# Geometry of the contract
# ---------------------------------------------------------------------------------------------------------------
def cut(rect, w, h):
    """R: the rectangle cut to the target (contract point 1)."""
    x0, y0, x1, y1 = (int(v) for v in rect)
    return min(x0, w), min(y0, h), min(x1, w), min(y1, h)


def window(rect, w, h):
    """W as (tx0, ty0, tx1, ty1); all zero for an empty R."""
    x0, y0, x1, y1 = cut(rect, w, h)
    if x0 >= x1 or y0 >= y1:
        return 0, 0, 0, 0
    return x0 // 16, y0 // 16, (x1 + 15) // 16, (y1 + 15) // 16


def tiles_outside(rect, w, h):
    """Boolean per tile of the target (row-major): not in W."""
    wt, ht = (w + 15) // 16, (h + 15) // 16
    tx0, ty0, tx1, ty1 = window(rect, w, h)
    ty, tx = np.divmod(np.arange(wt * ht), wt)
    return ~((tx >= tx0) & (tx < tx1) & (ty >= ty0) & (ty < ty1))


def end_outside(ptcl, rect, w, h):
    """A copy of a PTCL buffer with CMD_END as the first command of every tile outside W: parity.walk_ptcl_pair can then walk all tiles
    of a buffer whose blocks outside W hold stale words."""
    p = np.array(ptcl, copy=True)
    p[np.nonzero(tiles_outside(rect, w, h))[0] * 64 + 1] = CMD_END
    return p


def tile_blend_depth(ptcl, tile):
    """The deepest nesting of BEGIN_CLIP in a tile's command list (coarse.wgsl's max_blend_depth)."""
    ix, d, m = tile * 64 + 1, 0, 0
    for _ in range(1 << 20):
        t = int(ptcl[ix])
        if t == CMD_JUMP:
            ix = int(ptcl[ix + 1])
            continue
        if t == CMD_END:
            return m
        if t == CMD_BEGIN_CLIP:
            d += 1
            m = max(m, d)
        elif t == CMD_END_CLIP:
            d -= 1
        ix += int(_CMD_SIZE[t])
    raise AssertionError("PTCL walk did not terminate")


def blend_spill(ptcl, tiles):
    return sum(max(0, tile_blend_depth(ptcl, int(t)) - BLEND_STACK_SPLIT) * 256 for t in tiles)


# ---------------------------------------------------------------------------------------------------------------
# The oracle's whole frame, computed once per scene and shared
# ---------------------------------------------------------------------------------------------------------------
class Reference:
    def __init__(self, packed, layout, w, h, base, aa, resolved=None, oracle=None):
        self.packed, self.layout, self.w, self.h, self.base, self.aa, self.resolved = packed, layout, w, h, base, aa, resolved
        self.o = oracle or Oracle()
        self.o.set_scene(packed, layout, w, h, base, int(aa))
        if resolved is not None:
            self.o.set_ramps(resolved.ramps)
            self.o.set_image_atlas(resolved.atlas_image())
        self.img = self.o.render().copy()
        self.bump = dict(self.o.bump())
        assert self.bump["failed"] == 0, self.bump
        self.n_tiles = ((w + 15) // 16) * ((h + 15) // 16)
        self.ptcl = self.o.buffer("ptcl", np.uint32)[: 64 * self.n_tiles + self.bump["ptcl"]].copy()

    def restore(self):
        """(after the same-order check overwrote the oracle's tiles / PTCL / segments with the engine's)"""
        self.o.render()

    def segments_of(self, rect):
        """Segments of W's tiles, by the oracle's command lists."""
        p = end_outside(self.ptcl, rect, self.w, self.h)
        _, _, fn, _ = parity.walk_ptcl_pair("oracle", p, p, self.n_tiles)
        return int(fn.sum())

    def base_pixel(self):
        assert self.base >> 24 == 0xFF, "an opaque base colour: its pixel is its bytes"
        return np.array([self.base & 255, (self.base >> 8) & 255, (self.base >> 16) & 255, 255], dtype=np.uint8)

    def assert_window_sees_something(self, rect, name):
        """A case whose window sees nothing proves nothing: R holds pixels that are not the base colour, and so does a tile outside W."""
        x0, y0, x1, y1 = cut(rect, self.w, self.h)
        drawn = (self.img != self.base_pixel()).any(axis=2)
        assert drawn[y0:y1, x0:x1].any(), f"{name}: R holds the base colour only"
        tx0, ty0, tx1, ty1 = window(rect, self.w, self.h)
        if (tx0, ty0, tx1, ty1) != (0, 0, (self.w + 15) // 16, (self.h + 15) // 16):
            out = drawn.copy()
            out[ty0 * 16: ty1 * 16, tx0 * 16: tx1 * 16] = False
            assert out.any(), f"{name}: nothing is drawn outside W"


@functools.lru_cache(maxsize=None)
def main_reference(which, aa):
    """The scenes of the matrix at 300 x 280 (19 x 18 tiles, 2 x 2 bins, the right and bottom bins and tiles partial): `clipped` takes
    coarse's front-to-back form; `polygons` (cull_parity.polygon_scene: no clips) and `opaque_polygons` (the same with every third
    polygon opaque, so that whatever alpha the first one's random colours round to, covers exist) the back-to-front one."""
    import workloads

    if which == "clipped":
        scene = cp.view_of(workloads.random_test_scene(3, n_paths=300, size=512.0, strokes=True, clips=True), 205, 154)
    elif which == "polygons":
        scene = cp.view_of(cp.polygon_scene(), 205, 154)
    else:
        scene = cp.view_of(opaque_polygon_scene(), 205, 154)
    packed, layout = scene.resolve()
    assert (layout.n_clips != 0) == (which == "clipped")
    return Reference(packed, layout, MAIN_W, MAIN_H, BLACK, aa)


def opaque_polygon_scene():
    """cull_parity.polygon_scene()'s polygons; every third is opaque, so that the scene takes coarse's back-to-front walk."""
    from vello_amd import Affine, BezPath, Color, Fill, Scene

    rng = np.random.default_rng(11)
    s = Scene()
    for k in range(400):
        cx, cy = rng.uniform(-30, 542, 2)
        r = rng.uniform(3.0, 512.0 / 6)
        p = BezPath()
        a = np.sort(rng.uniform(0, 2 * np.pi, int(rng.integers(3, 9))))
        p.move_to((float(cx + r * np.cos(a[0])), float(cy + r * np.sin(a[0]))))
        for t in a[1:]:
            p.line_to((float(cx + r * np.cos(t)), float(cy + r * np.sin(t))))
        p.close_path()
        alpha = 1.0 if k % 3 == 0 else float(rng.uniform(0.4, 0.9))
        s.fill(Fill.EvenOdd if k % 2 else Fill.NonZero, Affine.IDENTITY, Color(float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), float(rng.uniform(0, 1)), alpha), None, p)
    return s


# ---------------------------------------------------------------------------------------------------------------
# The comparison, once
# ---------------------------------------------------------------------------------------------------------------
def _tol(aa):
    return 1 if int(aa) == 0 else 0


def check_front_half(name, engine, ref, bump, soup=None):
    """Contract point 3: every buffer ahead of coarse is the whole frame's (as cull_parity.compare_culled_frame holds them).  `soup`:
    the expected soup when it is not the oracle's whole one (viewport culling)."""
    o, ob, L, w, h = ref.o, ref.bump, ref.layout, ref.w, ref.h
    want_lines = ob["lines"] if soup is None else len(soup)
    assert bump["failed"] == 0, f"{name}: {bump}"
    assert bump["lines"] == want_lines, f"{name}: bump.lines {bump['lines']}, expected {want_lines}"
    for k in ("binning", "tile", "seg_counts"):
        assert bump[k] == ob[k], f"{name}: bump.{k} {bump[k]}, the whole frame's is {ob[k]}"
    n_tw = L.path_data_base - L.path_tag_base
    assert np.array_equal(engine.read_buffer("tag_monoids", np.uint32, n_tw * 20), o.buffer("tag_monoids", np.uint32)[: n_tw * 5]), f"{name}: tag_monoids differ"
    assert np.array_equal(engine.read_buffer("path_bboxes", np.int32, L.n_paths * 24), o.buffer("path_bboxes", np.int32)[: L.n_paths * 6]), f"{name}: path_bboxes differ"
    assert np.array_equal(engine.read_buffer("draw_monoids", np.uint32, L.n_draw_objects * 16), o.buffer("draw_monoids", np.uint32)[: L.n_draw_objects * 4]), \
        f"{name}: draw_monoids differ"
    assert np.array_equal(canonical_nan_words(engine.read_buffer("info_bin_data", np.uint32, L.bin_data_start * 4)),
                          canonical_nan_words(o.buffer("info_bin_data", np.uint32)[: L.bin_data_start])), f"{name}: draw info differs"
    if L.n_clips:
        assert np.array_equal(engine.read_buffer("clip_bboxes", np.uint32, L.n_clips * 16), o.buffer("clip_bboxes", np.uint32)[: L.n_clips * 4]), f"{name}: clip_bboxes differ"
    assert np.array_equal(engine.read_buffer("draw_bboxes", np.uint32, L.n_draw_objects * 16), o.buffer("draw_bboxes", np.uint32)[: L.n_draw_objects * 4]), \
        f"{name}: draw_bboxes differ"
    p_h = engine.read_buffer("paths", np.uint32, L.n_draw_objects * 32).reshape(-1, 8)
    p_o = o.buffer("paths", np.uint32)[: L.n_draw_objects * 8].reshape(-1, 8)
    assert np.array_equal(p_h[:, :4], p_o[:, :4]), f"{name}: path tile bboxes differ"
    lines_h = engine.read_buffer("lines", np.uint32, bump["lines"] * 24)
    a = sorted_rows(canonical_nan_lines(lines_h), 6)
    b = sorted_rows(canonical_nan_lines(o.buffer("lines", np.uint32)[: ob["lines"] * 6]) if soup is None else soup, 6)
    assert np.array_equal(a, b), f"{name}: the line soup differs as a multiset"
    t_h = engine.read_buffer("tiles", np.int32, ob["tile"] * 8).reshape(-1, 2)
    t_o = o.buffer("tiles", np.int32)[: ob["tile"] * 2].reshape(-1, 2)
    for i in range(L.n_draw_objects):
        n = int((p_o[i, 2] - p_o[i, 0]) * (p_o[i, 3] - p_o[i, 1]))
        assert not n or np.array_equal(t_h[p_h[i, 4]: p_h[i, 4] + n, 0], t_o[p_o[i, 4]: p_o[i, 4] + n, 0]), f"{name}: tile backdrops differ (path {i})"
    n_bin = parity.compare_bins(name, engine.read_buffer("bin_headers", np.uint32), engine.read_buffer("info_bin_data", np.uint32, (L.bin_data_start + ob["binning"]) * 4),
                                o.buffer("bin_headers", np.uint32), o.buffer("info_bin_data", np.uint32), L.n_draw_objects, w, h, L.bin_data_start)
    assert n_bin == ob["binning"], f"{name}: bin lists hold {n_bin} entries, bump.binning {ob['binning']}"
    parity.compare_seg_counts(name, engine.read_buffer("seg_counts", np.uint32, ob["seg_counts"] * 8), lines_h, o.buffer("seg_counts", np.uint32),
                              o.buffer("lines", np.uint32)[: ob["lines"] * 6], ob["seg_counts"])


def check_pixels(name, got, before, ref_img, rect, tol):
    """`got`, `before`: [h][stride] bytes of the target's rows after and before the frame.  Inside R the oracle's pixels within `tol`,
    everywhere else -- the rest of R's rows, the other rows, the row padding -- the bytes that were there."""
    h, w = ref_img.shape[:2]
    x0, y0, x1, y1 = cut(rect, w, h)
    inside = np.zeros(got.shape, dtype=bool)
    if x0 < x1 and y0 < y1:
        inside[y0:y1, x0 * 4: x1 * 4] = True
    changed = np.argwhere(~inside & (got != before))
    assert changed.size == 0, f"{name}: {len(changed)} bytes outside R were written, first at row {changed[0][0]}, byte {changed[0][1]}"
    if inside.any():
        a = got[y0:y1, x0 * 4: x1 * 4].astype(np.int32)
        b = ref_img[y0:y1, x0:x1].reshape(y1 - y0, -1).astype(np.int32)
        diff = np.abs(a - b)
        print(f"{name}: R {x0, y0, x1, y1}: max difference {diff.max()} (tolerance {tol})")
        assert diff.max() <= tol, f"{name}: R differs from the whole frame: max {diff.max()}, {(diff > tol).sum()} values over {tol}"


def fine_on_engine_window(engine, ref, bump, rect):
    """parity.fine_on_engine_inputs over W: the oracle's fine on the ENGINE's segments, tiles, info and command lists, the lists of
    tiles outside W (stale words) ended at once.  Returns the oracle's image; the caller looks at R only."""
    o, ob, L = ref.o, ref.bump, ref.layout
    used = {"segments": bump["segments"] * 6, "tiles": ob["tile"] * 2, "info_bin_data": L.bin_data_start + ob["binning"]}
    for name in used:
        dst = o.buffer(name, np.uint8)
        src = engine.read_buffer(name, np.uint8, min(dst.size, used[name] * 4))
        dst[: src.size] = src
    ptcl = end_outside(engine.read_buffer("ptcl", np.uint32, (64 * ref.n_tiles + bump["ptcl"]) * 4), rect, ref.w, ref.h)
    dst = o.buffer("ptcl", np.uint32)
    n = min(dst.size, ptcl.size)
    dst[:n] = ptcl[:n]
    o.run("fine", "fine")
    img = o.buffer("output", np.uint8)[: ref.w * ref.h * 4].reshape(ref.h, ref.w, 4).copy()
    ref.restore()
    return img


def check_back_half(name, engine, ref, bump, rect, no_cull):
    """Contract point 4 on the frame the engine holds.  no_cull: W's lists word for word (parity.walk_ptcl_pair's rules), bump.segments
    the sum of their fills, the segment slices of those fills.  Otherwise coarse's occlusion culling may only shrink the count."""
    want_segs = ref.segments_of(rect)
    smaller = tiles_outside(rect, ref.w, ref.h).any()
    if not no_cull:
        assert bump["segments"] <= want_segs, f"{name}: bump.segments {bump['segments']}, W's tiles hold {want_segs}"
        if ref.layout.n_clips != 0:  # (no occlusion culling in a scene with clips: exact)
            assert bump["segments"] == want_segs, f"{name}: bump.segments {bump['segments']}, W's tiles hold {want_segs}"
        return
    ptcl_h = end_outside(engine.read_buffer("ptcl", np.uint32, (64 * ref.n_tiles + bump["ptcl"]) * 4), rect, ref.w, ref.h)
    fh, fo, fn, _ = parity.walk_ptcl_pair(name, ptcl_h, end_outside(ref.ptcl, rect, ref.w, ref.h), ref.n_tiles)
    assert int(fn.sum()) == want_segs
    assert bump["segments"] == int(fn.sum()), f"{name}: bump.segments {bump['segments']}, the fills of W's lists cover {int(fn.sum())}"
    parity.compare_segment_slices(name, engine.read_buffer("segments", np.uint32, bump["segments"] * 24), ref.o.buffer("segments", np.uint32)[: ref.bump["segments"] * 6],
                                  fh, fo, fn)
    if smaller:
        assert bump["segments"] < ref.bump["segments"], f"{name}: bump.segments {bump['segments']} is not below the whole frame's {ref.bump['segments']}"
    else:
        assert bump["segments"] == ref.bump["segments"]
    # bump.blend: the spill of W's tiles alone
    inside = np.nonzero(~tiles_outside(rect, ref.w, ref.h))[0]
    if ref.layout.n_clips != 0 and len(inside) <= 64:
        assert bump["blend"] == blend_spill(ref.ptcl, inside), f"{name}: bump.blend {bump['blend']}"


def _frame(engine, ref, rect, mem, pad, lead_extra, seed):
    """One blocking frame with `rect` set.  With `mem` (a plain Engine): into a caller's device surface of seeded random bytes, rows
    `pad` bytes apart beyond width * 4, first row `lead_extra` bytes past a 16-byte boundary.  Without (an adapter of another parity
    module, whose render goes to the lane's internal target): into that target, filled with random bytes behind a whole frame.
    Returns (rows after, rows before, bump)."""
    w, h = ref.w, ref.h
    ramps = ref.resolved.ramps if ref.resolved is not None else None
    if mem is not None:
        stride, lead = w * 4 + pad, LEAD + lead_extra
        buf = mem.surface(lead + h * stride + LEAD, seed)
        before = mem.numpy(buf)
        engine.set_damage_rect(rect)
        try:
            _, bump = engine.render(ref.packed, ref.layout, w, h, ref.base, ref.aa, ramps=ramps, out=mem.view(buf, lead, h, w, stride), out_is_device=True)
        finally:
            engine.set_damage_rect(None)
        got = mem.numpy(buf)
        outside = np.ones(got.size, dtype=bool)
        outside[lead: lead + h * stride] = False
        assert np.array_equal(got[outside], before[outside]), "bytes in front of or behind the target's rows were written"
        return got[lead: lead + h * stride].reshape(h, stride), before[lead: lead + h * stride].reshape(h, stride), bump
    engine.set_damage_rect(None)
    engine.render(ref.packed, ref.layout, w, h, ref.base, ref.aa, ramps=ramps)  # (sizes the internal target)
    before = np.random.default_rng(0xDA3A6E00 + seed).integers(0, 256, w * h * 4, dtype=np.uint8)
    engine.write_buffer("output", before)
    engine.set_damage_rect(rect)
    try:
        _, bump = engine.render(ref.packed, ref.layout, w, h, ref.base, ref.aa, ramps=ramps)
    finally:
        engine.set_damage_rect(None)
    got = engine.read_buffer("output", np.uint8, w * h * 4)
    return got.reshape(h, w * 4), before.reshape(h, w * 4), bump


def compare_damaged_frame(engine, ref, rect, name, mem=None, no_cull=True, pad=8, lead_extra=0, seed=0, soup=None, front=True, require_content=True):
    """A frame of ref's scene with `rect` set, against ref (the oracle's whole frame).  `engine`: an Engine, or an adapter of another
    parity module that renders ref.packed's equivalent its own way.  no_cull: a second frame with VELLO_HIP_DEBUG_NO_CULL for the
    word-for-word checks.  Leaves the option off.  Returns the first frame's bump."""
    if require_content:
        ref.assert_window_sees_something(rect, name)
    tol = _tol(ref.aa)
    got, before, bump = _frame(engine, ref, rect, mem, pad, lead_extra, seed)
    check_pixels(name, got, before, ref.img, rect, tol)
    assert bump["failed"] == 0, f"{name}: {bump}"
    x0, y0, x1, y1 = cut(rect, ref.w, ref.h)
    if tol > 0 and x0 < x1 and y0 < y1:
        same_order = fine_on_engine_window(engine, ref, bump, rect)
        a = got[y0:y1, x0 * 4: x1 * 4]
        assert np.array_equal(a, same_order[y0:y1, x0:x1].reshape(y1 - y0, -1)), f"{name}: R differs from the oracle's fine on the engine's segment order"
    if front:
        check_front_half(name, engine, ref, bump, soup)
    check_back_half(name, engine, ref, bump, rect, no_cull=False)
    if no_cull:
        engine.update_debug_flags(no_cull=True)
        try:
            got2, before2, b2 = _frame(engine, ref, rect, mem, pad, lead_extra, seed + 1)
        finally:
            engine.update_debug_flags(no_cull=False)
        check_pixels(name + "_nocull", got2, before2, ref.img, rect, tol)
        check_back_half(name + "_nocull", engine, ref, b2, rect, no_cull=True)
    return bump


# ---------------------------------------------------------------------------------------------------------------
# The matrix: tile, quadrant and bin edges
# ---------------------------------------------------------------------------------------------------------------
MAIN_W, MAIN_H = 300, 280
RECTS = {
    "in_one_tile": (129, 129, 143, 143),       # inside tile (8, 8)
    "one_tile": (16, 16, 32, 32),
    "first_tile_short": (0, 0, 15, 15),
    "quadrant_corner": (127, 127, 129, 129),   # four quadrants of bin (0, 0), one pixel each way
    "bin_corner": (255, 255, 257, 257),        # four bins, one pixel each way
    "inside_bin_1_1": (257, 257, 299, 279),    # the grid's bin origin is not 0
    "last_pixel": (299, 279, 300, 280),
    "left_bins": (15, 17, 255, 279),           # tile edges one pixel off; bins (0, 0) and (0, 1), not their right neighbours
    "top_strip": (0, 16, 300, 128),            # every column, tile-aligned rows; one quadrant row
    "across": (17, 127, 257, 256),             # into all four bins' columns, stops on the lower bins' first row
    "whole": (0, 0, 300, 280),
}
CONFIGS = {"clipped_area": ("clipped", 0), "clipped_msaa16": ("clipped", 2), "polygons_area": ("polygons", 0), "polygons_msaa16": ("polygons", 2),
           "opaque_polygons_msaa16": ("opaque_polygons", 2)}


def check_matrix(engine, mem, name, config, rect_name):
    from vello_amd import AaConfig

    which, aa = CONFIGS[config]
    ref = main_reference(which, AaConfig(aa))
    compare_damaged_frame(engine, ref, RECTS[rect_name], f"{name}_{config}_{rect_name}", mem=mem, no_cull=True,
                          lead_extra=(0, 4, 12)[sorted(RECTS).index(rect_name) % 3], seed=sorted(RECTS).index(rect_name))


def snapshot(engine, ref, bump):
    """Every buffer and counter a frame leaves, as far as the frame used it."""
    L, ob = ref.layout, ref.bump
    sizes = {"tag_monoids": (L.path_data_base - L.path_tag_base) * 20, "path_bboxes": L.n_paths * 24, "lines": bump["lines"] * 24,
             "draw_monoids": L.n_draw_objects * 16, "info_bin_data": (L.bin_data_start + bump["binning"]) * 4, "clip_bboxes": L.n_clips * 16,
             "draw_bboxes": L.n_draw_objects * 16, "paths": L.n_draw_objects * 32, "tiles": bump["tile"] * 8, "seg_counts": bump["seg_counts"] * 8,
             "segments": bump["segments"] * 24, "ptcl": (64 * ref.n_tiles + bump["ptcl"]) * 4, "blend_spill": bump["blend"] * 4}
    out = {k: engine.read_buffer(k, np.uint8, n).copy() for k, n in sizes.items() if n}
    out["bin_headers"] = engine.read_buffer("bin_headers", np.uint8).copy()
    out["control"] = engine.control_words().copy()
    return out


def check_larger_than_target(engine, mem, name):
    """A rectangle larger than the target, and one that is exactly the target: the off state's buffers and counters, every one equal.
    (One engine, one resident scene, area AA left out: what the order of atomics decides differs between any two frames.)"""
    from vello_amd import AaConfig

    ref = main_reference("opaque_polygons", AaConfig.Msaa16)
    w, h = ref.w, ref.h

    def frame(rect):
        engine.set_damage_rect(rect)
        try:
            img, bump = engine.render(ref.packed, ref.layout, w, h, ref.base, ref.aa)
        finally:
            engine.set_damage_rect(None)
        return img, bump, snapshot(engine, ref, bump)

    img0, b0, s0 = frame(None)
    assert np.array_equal(img0, ref.img)
    for rect in ((0, 0, 1000, 1000), (0, 0, w, h), (0, 0, 0xFFFFFFFF, 0xFFFFFFFF)):
        img, b, s = frame(rect)
        assert np.array_equal(img, img0), f"{name} {rect}: image"
        assert b == b0, f"{name} {rect}: bump {b}, off state {b0}"
        # (line soup, tile and segment placement follow the order of atomics between any two frames: compared as multisets of rows)
        for k in s0:
            if k in ("lines", "segments"):  # (which slot a row gets is the order of atomics, between any two frames)
                assert np.array_equal(sorted_rows(s[k].view(np.uint32), 6), sorted_rows(s0[k].view(np.uint32), 6)), f"{name} {rect}: {k} differ from the off state's"
            elif k in ("tag_monoids", "path_bboxes", "draw_monoids", "clip_bboxes", "draw_bboxes"):
                assert np.array_equal(s[k], s0[k]), f"{name} {rect}: {k} differs from the off state's"
            elif k == "control":  # bump allocators, flatten's list lengths, fine's buckets, slice items, coverage words
                assert np.array_equal(s[k][:16], s0[k][:16]) and np.array_equal(s[k][16:50], s0[k][16:50]), f"{name} {rect}: control block"
            else:  # (records whose indices follow the order of atomics: held to the oracle below)
                assert s[k].shape == s0[k].shape, f"{name} {rect}: {k}"
        # ... and the frame as a whole by the oracle, as any whole frame is held
        check_front_half(f"{name} {rect}", engine, ref, b)
    compare_damaged_frame(engine, ref, (0, 0, 1000, 1000), f"{name}_oracle", mem=mem, no_cull=True)


# ---------------------------------------------------------------------------------------------------------------
# k_fine's store
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def store_reference(w):
    import workloads
    from vello_amd import AaConfig

    packed, layout = workloads.random_test_scene(2, n_paths=60, size=48.0, strokes=True, clips=True).resolve()
    return Reference(packed, layout, w, 20, BLACK, AaConfig.Msaa8)


# x0 mod 4 and x1 mod 4 each take 0 .. 3; (5, 7) lies inside one lane's four pixels; widths of 1; x1 = 37 on the 37-wide target
STORE_SPANS = ((0, 40), (4, 8), (5, 7), (1, 2), (2, 3), (3, 4), (6, 13), (7, 38), (8, 9), (11, 12), (0, 1), (39, 40), (1, 39), (2, 40))
STORE_SPANS_37 = ((0, 37), (36, 37), (33, 37), (5, 37))
STORE_PLACEMENTS = ((0, 8), (4, 8), (12, 8))  # (bytes the first row sits past a 16-byte boundary, row padding)


STORE_PARTS = 3


def check_store(engine, mem, name, part):
    """Every alignment of R's two vertical edges against a lane's four pixels, rows [3, 18) of a 40 x 20 target (two tile rows); the
    spans are dealt to STORE_PARTS test cases."""
    n = 0
    for w, spans in ((40, STORE_SPANS), (37, STORE_SPANS_37)):
        ref = store_reference(w)
        assert {a % 4 for a, _ in STORE_SPANS} == {b % 4 for _, b in STORE_SPANS} == {0, 1, 2, 3}
        for k, (x0, x1) in enumerate(spans):
            if k % STORE_PARTS != part:
                continue
            for lead_extra, pad in (STORE_PLACEMENTS if k % 5 == 2 or (x0, x1) in ((5, 7), (7, 38), (0, 40)) else STORE_PLACEMENTS[:1]):
                compare_damaged_frame(engine, ref, (x0, 3, x1, 18), f"{name}_{w}_{x0}_{x1}_lead{lead_extra}", mem=mem, no_cull=False, pad=pad, lead_extra=lead_extra,
                                      seed=n, front=False, require_content=False)
                n += 1
    ref = store_reference(40)
    drawn = (ref.img != ref.base_pixel()).any(axis=2)
    assert drawn[3:18].any() and drawn[:3].any()


# ---------------------------------------------------------------------------------------------------------------
# Empty and refused
# ---------------------------------------------------------------------------------------------------------------
EMPTY_RECTS = ((100, 50, 100, 200), (20, 90, 250, 90), (300, 0, 400, 280), (0, 280, 300, 500), (0, 0, 0, 0), (5000, 5000, 6000, 6000))


def check_empty(engine, mem, name, rects):
    from vello_amd import AaConfig

    ref = main_reference("clipped", AaConfig.Msaa16)
    # a covered point: pick answers as after the whole frame
    drawn = np.argwhere((ref.img != ref.base_pixel()).any(axis=2))
    pts = np.array([[x + 0.5, y + 0.5] for y, x in drawn[:: max(1, len(drawn) // 40)]], dtype=np.float32)
    engine.render(ref.packed, ref.layout, ref.w, ref.h, ref.base, ref.aa)
    want_pick = engine.pick(pts).copy()
    assert (want_pick[:, 0] != 0xFFFFFFFF).any()
    for k, rect in enumerate(rects):
        bump = compare_damaged_frame(engine, ref, rect, f"{name}_{rect}", mem=mem, no_cull=False, seed=k, require_content=False)
        assert bump["segments"] == 0 and bump["ptcl"] == 0 and bump["blend"] == 0, f"{name} {rect}: {bump}"
        assert engine.sync() == 0
        assert np.array_equal(engine.pick(pts), want_pick), f"{name} {rect}: pick after an empty frame"


def check_pick_after_damage(engine, mem, name):
    """vello_hip_pick and vello_hip_pick_rect after a damaged frame answer as after the whole frame: they read what lies ahead of coarse."""
    from vello_amd import AaConfig

    ref = main_reference("clipped", AaConfig.Msaa16)
    drawn = np.argwhere((ref.img != ref.base_pixel()).any(axis=2))
    pts = np.array([[x + 0.5, y + 0.5] for y, x in drawn[:: max(1, len(drawn) // 60)]], dtype=np.float32)
    engine.render(ref.packed, ref.layout, ref.w, ref.h, ref.base, ref.aa)
    want_pick = engine.pick(pts).copy()
    want_rect = engine.pick_rect((40.0, 30.0, 200.0, 150.0))
    compare_damaged_frame(engine, ref, RECTS["one_tile"], f"{name}_one_tile", mem=mem, no_cull=False, front=False)
    assert np.array_equal(engine.pick(pts), want_pick), f"{name}: pick after a damaged frame"
    got_rect = engine.pick_rect((40.0, 30.0, 200.0, 150.0))
    assert np.array_equal(got_rect[0], want_rect[0]) and got_rect[2] == want_rect[2], f"{name}: pick_rect after a damaged frame"


def check_refused(engine, fresh_engine, name):
    from vello_amd import AaConfig

    ref = main_reference("polygons", AaConfig.Msaa16)
    lib, h = engine._lib, engine._h
    engine.upload_scene(ref.packed, ref.layout)
    engine.render_resident(ref.w, ref.h, ref.base, ref.aa)
    assert engine.sync() == 0
    for rect in ((10, 0, 9, 20), (0, 21, 30, 20), (0xFFFFFFFF, 0, 0, 0)):
        r = lib.vello_hip_set_damage_rect(h, (ctypes.c_uint32 * 4)(*rect))
        assert r == E_INVALID, f"{name} {rect}: {r}"
        err = lib.vello_hip_last_error(h).decode()
        assert "x0 <= x1" in err and "y0 <= y1" in err, f"{name}: the error does not name the rule: {err!r}"
    assert lib.vello_hip_set_damage_rect(None, None) == E_INVALID
    # nothing changed: the next plain frame is a fresh engine's, bit for bit
    img, bump = engine.render(ref.packed, ref.layout, ref.w, ref.h, ref.base, ref.aa)
    img2, bump2 = fresh_engine.render(ref.packed, ref.layout, ref.w, ref.h, ref.base, ref.aa)
    assert np.array_equal(img, img2) and np.array_equal(img, ref.img) and bump == bump2, f"{name}: {bump} {bump2}"
    # a refusal while a rectangle is set keeps that rectangle
    engine.set_damage_rect((16, 16, 32, 32))
    assert lib.vello_hip_set_damage_rect(h, (ctypes.c_uint32 * 4)(10, 0, 9, 20)) == E_INVALID
    try:
        _, b = engine.render(ref.packed, ref.layout, ref.w, ref.h, ref.base, ref.aa)
    finally:
        engine.set_damage_rect(None)
    assert 0 < b["segments"] < bump["segments"]


# ---------------------------------------------------------------------------------------------------------------
# Slices
# ---------------------------------------------------------------------------------------------------------------
def check_slices(engine, mem, name):
    """Forced slices, MSAA16: a long tile (13 FILLs: four slices) inside W, a second one outside.  The damaged frame cuts only W's tile
    into slices; the whole frame rendered next is exact and its counters are the oracle's."""
    from tests import fine_parity as fp
    from vello_amd import AaConfig, Affine, Scene

    tl = fp.TileList(48, 48).pairs(13)
    s = Scene()
    s.append(tl.s)
    s.append(tl.s, Affine.translate(32.0, 0.0))
    packed, layout = s.resolve()
    ref = Reference(packed, layout, 48, 48, BLACK, AaConfig.Msaa16)
    c = engine.stage_constants()
    per_tile = fp.slice_items(13, c["fine_slice_fills_forced"], c["fine_slice_min_fills_forced"])
    assert per_tile >= 2
    engine.set_debug_flags(fine_slices=True)
    try:
        img, bump = engine.render(packed, layout, 48, 48, BLACK, AaConfig.Msaa16)
        assert np.array_equal(img, ref.img) and engine.fine_slice_stats()[0] == 2 * per_tile, (engine.fine_slice_stats(), per_tile)
        for rect in ((0, 0, 16, 16), (33, 2, 47, 9)):
            compare_damaged_frame(engine, ref, rect, f"{name}_{rect}", mem=mem, no_cull=False)
            assert engine.fine_slice_stats()[0] == per_tile, f"{name} {rect}: {engine.fine_slice_stats()[0]} slice items, W's tile has {per_tile}"
            img, bump = engine.render(packed, layout, 48, 48, BLACK, AaConfig.Msaa16)
            assert np.array_equal(img, ref.img), f"{name} {rect}: the whole frame after the damaged one"
            assert all(bump[k] == ref.bump[k] for k in BUMP_KEYS if k != "ptcl"), f"{name} {rect}: {bump} oracle {ref.bump}"
            assert engine.fine_slice_stats()[0] == 2 * per_tile
    finally:
        engine.set_debug_flags()


def check_slice_demand(engine, name):
    """Resident MSAA frames of a scene the engine has not seen whole: the first ones damaged (they must not teach it the scene's slice
    demand), then a whole one, which asks for the slices of both long tiles and is exact.  (What a wrongly learnt demand costs is
    slice blocks, not pixels: this holds what a test can see of it.)"""
    from tests import fine_parity as fp
    from vello_amd import AaConfig, Affine, Scene

    tl = fp.TileList(48, 16).pairs(13)
    s = Scene()
    s.append(tl.s)
    s.append(tl.s, Affine.translate(32.0, 0.0))
    packed, layout = s.resolve()
    ref = Reference(packed, layout, 48, 16, BLACK, AaConfig.Msaa16)
    engine.set_debug_flags(fine_slices=True)
    try:
        engine.upload_scene(packed, layout)
        engine.set_damage_rect((0, 0, 16, 16))
        for _ in range(2):
            engine.render_resident(48, 16, BLACK, AaConfig.Msaa16)
            engine.sync_frame(0)
            assert engine.sync() == 0
        engine.set_damage_rect(None)
        engine.render_resident(48, 16, BLACK, AaConfig.Msaa16)
        assert engine.sync() == 0
        whole_items = engine.fine_slice_stats()[0]
        assert np.array_equal(engine.read_buffer("output", np.uint8, 48 * 16 * 4).reshape(16, 48, 4), ref.img), name
        assert whole_items > 0 and whole_items % 2 == 0
    finally:
        engine.set_damage_rect(None)
        engine.set_debug_flags()


# ---------------------------------------------------------------------------------------------------------------
# Blend spill
# ---------------------------------------------------------------------------------------------------------------
def check_blend_spill(engine, mem, name):
    """workloads.clip_blend_scene nested deeper than the blend stack's registers in a tile inside W and in tiles outside: bump.blend is
    the spill of W's tiles alone, by the oracle's per-tile depth."""
    import workloads
    from vello_amd import AaConfig

    from vello_amd import Affine, BlendMode, Compose, Fill, Mix, Rect, Scene

    # clip_blend_scene inside four blend layers that cover the target: every tile's nesting is four deeper than the scene's own
    s = Scene()
    for d in range(4):
        s.push_layer(Fill.NonZero, BlendMode((Mix.Screen, Mix.Normal)[d % 2], Compose.SrcOver), 0.9, Affine.IDENTITY, Rect(-8.0, -8.0, 136.0, 136.0))
    s.append(workloads.clip_blend_scene(size=128.0, depth=6))
    for d in range(4):
        s.pop_layer()
    packed, layout = s.resolve()
    w = h = 128
    ref = Reference(packed, layout, w, h, BLACK, AaConfig.Msaa16)
    depth = np.array([tile_blend_depth(ref.ptcl, t) for t in range(ref.n_tiles)])
    assert blend_spill(ref.ptcl, range(ref.n_tiles)) == ref.bump["blend"], "the per-tile depths do not add up to the oracle's bump.blend"
    deep = np.nonzero(depth > BLEND_STACK_SPLIT)[0]
    assert len(deep) >= 2, depth
    wt = (w + 15) // 16
    drawn = (ref.img != ref.base_pixel()).any(axis=2)
    shown = [int(t) for t in deep if drawn[t // wt * 16 + 5: t // wt * 16 + 9, t % wt * 16 + 3: t % wt * 16 + 16].any()]
    assert shown, "no deeply nested tile shows anything"
    t = max(shown, key=lambda t: (depth[t], t))
    tx, ty = t % wt, t // wt
    for rect in ((tx * 16, ty * 16, tx * 16 + 16, ty * 16 + 16), (tx * 16 + 3, ty * 16 + 5, tx * 16 + 18, ty * 16 + 9)):
        inside = np.nonzero(~tiles_outside(rect, w, h))[0]
        assert (depth[inside] > BLEND_STACK_SPLIT).any() and (depth[np.nonzero(tiles_outside(rect, w, h))[0]] > BLEND_STACK_SPLIT).any()
        bump = compare_damaged_frame(engine, ref, rect, f"{name}_{rect}", mem=mem, no_cull=True)
        want = blend_spill(ref.ptcl, inside)
        assert 0 < want < ref.bump["blend"]
        assert bump["blend"] == want, f"{name} {rect}: bump.blend {bump['blend']}, W's tiles spill {want} (the whole frame {ref.bump['blend']})"


# ---------------------------------------------------------------------------------------------------------------
# Frames in flight
# ---------------------------------------------------------------------------------------------------------------
IN_FLIGHT_W, IN_FLIGHT_H = 140, 120
IN_FLIGHT_RECTS = ((0, 0, 60, 50), (70, 3, 140, 59), (17, 62, 80, 120), (81, 60, 139, 119))
IN_FLIGHT_BASES = (0xFF203040, 0xFF00A0FF, 0xFFFFFFFF, 0xFF60FF60)


@functools.lru_cache(maxsize=None)
def base_reference(base):
    from vello_amd import AaConfig

    r = main_reference("clipped", AaConfig.Msaa16)
    return Reference(r.packed, r.layout, IN_FLIGHT_W, IN_FLIGHT_H, base, r.aa)


def in_flight_engine(make_engine):
    """An engine whose pools fit the in-flight scene twice over (four lanes of the default pools take the emulator seconds to allocate)."""
    ref = base_reference(BLACK)
    ob = ref.bump
    return make_engine({"lines": 2 * ob["lines"] + 1024, "tiles": 2 * ob["tile"] + 1024, "seg_counts": 2 * ob["seg_counts"] + 1024,
                        "segments": 2 * ob["seg_counts"] + 1024, "ptcl": 64 * ref.n_tiles + 4 * ob["ptcl"] + 4096,
                        "bin_data": ref.layout.bin_data_start + 2 * ob["binning"] + 1024, "blend_spill": 2 * ob["blend"] + 1024})


def check_in_flight(engine, mem, name, toggle):
    """Four frames in flight, one device target that holds the whole frame: four damaged frames enqueued back to back, four disjoint
    rectangles, a base colour each.  Each rectangle holds its own frame's pixels, the rest the first whole frame's.  toggle: the option
    changed between two render_resident calls instead: one damaged and one whole frame, in that order and in the other."""
    from vello_amd import AaConfig

    ref = base_reference(BLACK)
    w, h, aa = ref.w, ref.h, AaConfig.Msaa16
    refs = [base_reference(b) for b in IN_FLIGHT_BASES]
    for r, rect in zip(refs, IN_FLIGHT_RECTS):
        x0, y0, x1, y1 = rect
        assert not np.array_equal(r.img[y0:y1, x0:x1], ref.img[y0:y1, x0:x1]), "the base colour does not show in this rectangle"
    stride = w * 4 + 8
    engine.upload_scene(ref.packed, ref.layout)
    engine.set_frames_in_flight(4)
    try:
        if toggle:
            return _check_toggle(engine, mem, name, ref, stride)
        buf = mem.surface(LEAD + h * stride + LEAD, 77)
        view = mem.view(buf, LEAD, h, w, stride)
        engine.render_resident(w, h, BLACK, aa, out=view)
        assert engine.sync() == 0
        before = mem.numpy(buf)
        plp.check_surface(f"{name}_whole", before, plp._canary(before.size, 77), [(LEAD, stride, ref.img, 0)])
        for base, rect in zip(IN_FLIGHT_BASES, IN_FLIGHT_RECTS):
            engine.set_damage_rect(rect)
            engine.render_resident(w, h, base, aa, out=view)
        engine.set_damage_rect(None)
        assert engine.sync() == 0
        got = mem.numpy(buf)
        want = before.copy()
        rows = want[LEAD: LEAD + h * stride].reshape(h, stride)
        for r, (x0, y0, x1, y1) in zip(refs, IN_FLIGHT_RECTS):
            rows[y0:y1, x0 * 4: x1 * 4] = r.img[y0:y1, x0:x1].reshape(y1 - y0, -1)
        assert np.array_equal(got, want), f"{name}: {(got != want).sum()} bytes differ"
    finally:
        engine.set_damage_rect(None)
        engine.set_frames_in_flight(1)


def _check_toggle(engine, mem, name, ref, stride):
    """(frames already enqueued keep the rectangle they were enqueued with)"""
    from vello_amd import AaConfig

    w, h, aa = ref.w, ref.h, AaConfig.Msaa16
    try:
        for first_damaged in (True, False):
            a, b = mem.surface(LEAD + h * stride + LEAD, 78), mem.surface(LEAD + h * stride + LEAD, 79)
            ca, cb = mem.numpy(a), mem.numpy(b)
            rect = IN_FLIGHT_RECTS[1]
            engine.set_damage_rect(rect if first_damaged else None)
            engine.render_resident(w, h, BLACK, aa, out=mem.view(a, LEAD, h, w, stride))
            engine.set_damage_rect(None if first_damaged else rect)
            engine.render_resident(w, h, BLACK, aa, out=mem.view(b, LEAD, h, w, stride))
            engine.set_damage_rect(None)
            assert engine.sync() == 0
            for buf2, canary, damaged in ((a, ca, first_damaged), (b, cb, not first_damaged)):
                g = mem.numpy(buf2)
                check_pixels(f"{name}_toggle_{first_damaged}_{damaged}", g[LEAD: LEAD + h * stride].reshape(h, stride), canary[LEAD: LEAD + h * stride].reshape(h, stride),
                             ref.img, rect if damaged else (0, 0, w, h), 0)
    finally:
        engine.set_damage_rect(None)
        engine.set_frames_in_flight(1)


# ---------------------------------------------------------------------------------------------------------------
# Composition: none of the other per-frame options learns about the rectangle
# ---------------------------------------------------------------------------------------------------------------
COMPOSE_RECT = (37, 21, 150, 99)


def check_with_viewport_cull(engine, mem, name):
    from vello_amd import AaConfig

    ref = main_reference("polygons", AaConfig.Msaa16)
    R, S = cp.oracle_soup(ref.o, ref.w, ref.h)
    assert len(S) < len(R)
    engine.set_viewport_cull(True)
    try:
        compare_damaged_frame(engine, ref, COMPOSE_RECT, name, mem=mem, no_cull=True, soup=S)
    finally:
        engine.set_viewport_cull(False)


def check_with_view(engine, name):
    from tests import view_parity as vp
    from vello_amd import AaConfig, Affine

    raw = main_reference("clipped", AaConfig.Msaa16)
    packed, layout = np.ascontiguousarray(raw.packed, dtype=np.uint8), raw.layout
    view = Affine.translate(-40.0, -25.0) * Affine.scale(1.3)
    ref = Reference(vp.compose(packed, layout, view), layout, 200, 150, BLACK, AaConfig.Msaa16)
    assert not np.array_equal(ref.img, raw.img[:150, :200])
    ve = vp.ViewEngine(engine, packed, view)
    compare_damaged_frame(ve, ref, COMPOSE_RECT, name, no_cull=True)
    assert ve.frames >= 4


class _FrameEngine:
    """An adapter as the other parity modules': every blocking render is a vello_hip_render_frame of the same bytes (a private scene)."""

    def __init__(self, engine):
        self._engine = engine

    def __getattr__(self, k):
        return getattr(self._engine, k)

    def render(self, packed, layout, w, h, base, aa, ramps=None):
        e = self._engine
        e.render_frame(packed, layout, w, h, base, aa, ramps=ramps)
        assert e.sync() == 0
        return e.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4).copy(), e.bump()


def check_render_frame(engine, name):
    from vello_amd import AaConfig

    compare_damaged_frame(_FrameEngine(engine), main_reference("clipped", AaConfig.Area), COMPOSE_RECT, name, no_cull=True)


def check_instances(engine, name):
    from tests import instance_parity as ip
    from tests import retained_parity as rp
    from vello_amd import AaConfig

    w, h = 160, 120
    lib, inst = rp.scene_list(["solid", "linear", "clip", "blend"], 9, w, h, 31)
    lib.upload(engine)
    packed, layout = ip.compose(lib.packed, lib.layout, lib.fragments, inst)
    ref = Reference(packed, layout, w, h, BLACK, AaConfig.Msaa16, resolved=ip._Late(lib))
    ie = ip.InstanceEngine(engine, inst)
    compare_damaged_frame(ie, ref, (21, 17, 120, 90), name, no_cull=True)
    assert ie.frames >= 4


def check_retained_painted(engine, name):
    """render_retained_painted with ONE solid paint and R = the box of what that paint changes: behind a whole frame of the retained
    colours, the damaged frame makes the target the whole painted frame."""
    from tests import instance_parity as ip
    from tests import repaint_parity as rpp
    from tests import retained_parity as rp
    from vello_amd import AaConfig

    w, h = 160, 120
    lib, inst = rp.scene_list(["solid", "linear", "clip", "blend"], 9, w, h, 31)
    n = len(inst)
    lib.upload(engine)
    plain = rp.want(lib, inst, w, h, BLACK, AaConfig.Msaa16)
    for j in range(n):
        p = [None] * n
        p[j] = 0xFF10E0F0
        q = rpp.effective(None, p, n)
        packed, layout = rp.compose(lib, inst, q)
        ref = Reference(packed, layout, w, h, BLACK, AaConfig.Msaa16, resolved=ip._Late(lib))
        ys, xs = np.nonzero((ref.img != plain).any(axis=2))
        if len(ys) and (xs.max() + 1 - xs.min()) * (ys.max() + 1 - ys.min()) * 4 < w * h:
            break
    else:
        raise AssertionError("no instance whose paint changes a small part of the frame")
    rect = (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1)
    re = rpp.RepaintEngine(engine, inst, None, dict(paints=p))
    compare_damaged_frame(re, ref, rect, name, no_cull=True, require_content=False)
    # the use itself: the retained colours whole, then the painted frame's damage alone
    engine.set_damage_rect(None)
    img, _ = rpp.frame(engine, w, h, BLACK, AaConfig.Msaa16)
    assert np.array_equal(img, plain)
    engine.set_damage_rect(rect)
    try:
        img, _ = rpp.frame(engine, w, h, BLACK, AaConfig.Msaa16, paints=p)
    finally:
        engine.set_damage_rect(None)
    assert np.array_equal(img, ref.img), f"{name}: whole frame + the paint's damage is not the painted frame"


def check_morphed(engine, name):
    from tests import morph_parity as mp
    from vello_amd import AaConfig

    packed, layout = mp.small_triangles_scene(300, size=200.0)
    keys = mp.two_keys(packed, layout)
    morph = (0, 1, 0.375)
    want = mp.expected_words(mp.path_words(packed, layout), keys, None, *morph)
    ref = Reference(mp.substitute(packed, layout, want), layout, 200, 150, BLACK, AaConfig.Msaa16)
    assert not np.array_equal(ref.img, mp._oracle_image(packed, layout, 200, 150, BLACK, AaConfig.Msaa16))
    me = mp.MorphEngine(engine, packed, morph, keys)
    compare_damaged_frame(me, ref, COMPOSE_RECT, name, no_cull=True)
    assert me.frames >= 4


class _ResidentEngine:
    """Every blocking render is a render_resident of the scene uploaded once."""

    def __init__(self, engine, packed, layout):
        self._engine = engine
        engine.upload_scene(packed, layout)
        self.frames = 0

    def __getattr__(self, k):
        return getattr(self._engine, k)

    def render(self, packed, layout, w, h, base, aa, ramps=None):
        e = self._engine
        self.frames += 1
        e.render_resident(w, h, base, aa)
        assert e.sync() == 0
        return e.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4).copy(), e.bump()


def check_indexed(engine, name):
    from tests import scene_index_parity as sip
    from vello_amd import AaConfig

    packed, layout = sip.case_scene("fills_only")
    ref = Reference(packed, layout, sip.W, sip.H, BLACK, AaConfig.Msaa16, oracle=sip.make_oracle())
    before = engine.scene_index_builds()
    re = _ResidentEngine(engine, packed, layout)
    assert engine.scene_index_builds() == before + 1, "the scene is not indexed: the case proves nothing"
    compare_damaged_frame(re, ref, COMPOSE_RECT, name, no_cull=True)
    assert re.frames >= 4 and engine.scene_index_builds() == before + 1, f"{name}: frames built an index"


def check_fused_front(engine, mem, name):
    """The small-scene fused front: vello_hip_fused_launches advances as it does without the option."""
    import workloads
    from vello_amd import AaConfig

    packed, layout = workloads.stroke_styles_scene().resolve()
    ref = Reference(packed, layout, 256, 256, WHITE, AaConfig.Msaa16)
    engine.set_debug_flags(flatten_coop=True)
    try:
        before = engine.fused_launches()
        engine.render(packed, layout, 256, 256, WHITE, AaConfig.Msaa16)
        per_frame = engine.fused_launches() - before
        assert per_frame > 0, "the scene's front is not fused: the case proves nothing"
        engine.set_damage_rect((40, 40, 100, 90))
        before = engine.fused_launches()
        engine.render(packed, layout, 256, 256, WHITE, AaConfig.Msaa16)
        engine.set_damage_rect(None)
        assert engine.fused_launches() - before == per_frame, f"{name}: {engine.fused_launches() - before} fused launches, {per_frame} without the option"
        compare_damaged_frame(engine, ref, (40, 40, 100, 90), name, mem=mem, no_cull=True)
    finally:
        engine.set_damage_rect(None)
        engine.set_debug_flags()


def check_run_stages(engine, name):
    """vello_hip_run_stages(COARSE .. FINE) with a rectangle, behind a whole frame's front half run without one."""
    from vello_amd import AaConfig

    ref = main_reference("clipped", AaConfig.Msaa16)
    w, h = ref.w, ref.h
    engine.render(ref.packed, ref.layout, w, h, ref.base, ref.aa)
    before = np.random.default_rng(5).integers(0, 256, w * h * 4, dtype=np.uint8)
    engine.write_buffer("output", before)
    engine.upload_scene(ref.packed, ref.layout)
    engine.run_stages(w, h, ref.base, ref.aa, "pathtag_scan", "backdrop")
    engine.set_damage_rect(COMPOSE_RECT)
    try:
        engine.run_stages(w, h, ref.base, ref.aa, "coarse", "fine")
    finally:
        engine.set_damage_rect(None)
    bump = engine.bump()
    got = engine.read_buffer("output", np.uint8, w * h * 4)
    check_pixels(name, got.reshape(h, w * 4), before.reshape(h, w * 4), ref.img, COMPOSE_RECT, 0)
    check_front_half(name, engine, ref, bump)
    check_back_half(name, engine, ref, bump, COMPOSE_RECT, no_cull=False)


# ---------------------------------------------------------------------------------------------------------------
# Pools
# ---------------------------------------------------------------------------------------------------------------
def check_segment_pool(make_engine, mem, name):
    """A segment pool of (the segments of W's tiles) + 64: the whole frame reports VELLO_HIP_E_CAPACITY, the damaged frame is correct
    (cull_parity.check_line_pool's pattern)."""
    from vello_amd import AaConfig

    ref = main_reference("clipped", AaConfig.Msaa16)
    rect = RECTS["left_bins"]
    n = ref.segments_of(rect)
    assert n + 64 < ref.bump["segments"]
    eng = make_engine({"segments": n + 64})
    assert eng.capacities()["segments"] == n + 64
    img, bump = eng.render(ref.packed, ref.layout, ref.w, ref.h, ref.base, ref.aa)
    assert bump["failed"] != 0 and bump["segments"] == ref.bump["segments"], f"{name}: option off: {bump}"
    assert eng.sync() == -4
    bump = compare_damaged_frame(eng, ref, rect, name, mem=mem, no_cull=False)
    assert bump["failed"] == 0 and bump["segments"] == n
    assert eng.sync() == 0
    assert eng.capacities()["segments"] == n + 64


# ---------------------------------------------------------------------------------------------------------------
# Public layer
# ---------------------------------------------------------------------------------------------------------------
def check_renderer(name):
    """Renderer.render_to_texture with RenderParams(damage=...) into a pre-filled array: inside the plain call's image, outside
    untouched; the next call without `damage` is whole."""
    import vello_amd
    import workloads
    from vello_amd import AaConfig, Color, RenderParams

    scene = cp.view_of(workloads.random_test_scene(3, n_paths=300, size=512.0, strokes=True, clips=True), 205, 154)
    w, h = 175, 131
    r = vello_amd.Renderer()
    plain = np.zeros((h, w, 4), dtype=np.uint8)
    r.render_to_texture(scene, plain, RenderParams(Color.from_rgb8(0, 0, 0), w, h, AaConfig.Msaa16))
    whole_segments = r.last_bump()["segments"]
    rect = (33, 18, 150, 97)
    before = np.random.default_rng(3).integers(0, 256, (h, w, 4), dtype=np.uint8)
    out = before.copy()
    r.render_to_texture(scene, out, RenderParams(Color.from_rgb8(0, 0, 0), w, h, AaConfig.Msaa16, damage=rect))
    check_pixels(name, out.reshape(h, w * 4), before.reshape(h, w * 4), plain, rect, 0)
    assert not np.array_equal(out[18:97, 33:150], before[18:97, 33:150])
    assert 0 < r.last_bump()["segments"] < whole_segments
    out = before.copy()
    r.render_to_texture(scene, out, RenderParams(Color.from_rgb8(0, 0, 0), w, h, AaConfig.Msaa16))
    assert np.array_equal(out, plain), f"{name}: the call after a damaged one is not whole"
    with pytest.raises(vello_amd.VelloHipError):
        r.render_to_texture(scene, out, RenderParams(Color.from_rgb8(0, 0, 0), w, h, AaConfig.Msaa16, damage=(9, 0, 8, 5)))
    out = before.copy()
    r.render_to_texture(scene, out, RenderParams(Color.from_rgb8(0, 0, 0), w, h, AaConfig.Msaa16))
    assert np.array_equal(out, plain), f"{name}: the call after a refused one is not whole"
