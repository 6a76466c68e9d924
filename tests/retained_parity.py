"""Retained instance lists (vello_hip_retain_instances / vello_hip_render_retained / vello_hip_release_retained) against the CPU oracle
and against vello_hip_render_instances_painted.  The oracle is handed instance_parity.compose(lib, (fragment_i, X_i)) -- numpy, not the
library under test -- through parity.compare_frame, whose engine is RetainedEngine: it retains the list once and then renders every
frame compare_frame asks for with render_retained under the poses X.  Every intermediate is held at the tolerances the suite already
uses; nothing here has a tolerance of its own.

`device(poses)` turns an (n, 6) float32 array into what stands for device memory: a torch tensor on the GPU, or -- the emulated build,
where the two are one address space -- the numpy array itself, passed with transforms_is_device."""
import ctypes
import math

import numpy as np

from tests import instance_parity as ip
from tests import paint_parity as pp
from tests import parity
from tests import view_parity

BLACK, WHITE = ip.BLACK, ip.WHITE
IDENT = (1.0, 0.0, 0.0, 1.0, 0.0, 0.0)


def posed(instances, poses):
    """The list with pose i in instance i's transform's place: what render_instances would be handed for the same frame."""
    assert len(instances) == len(poses)
    return [(int(f), tuple(float(v) for v in p)) for (f, _), p in zip(instances, poses)]


def rest_poses(instances):
    from vello_amd.renderer import instance_array

    return np.ascontiguousarray(instance_array(instances)["transform"], dtype=np.float32).reshape(-1, 6)


def turned(instances, w, h, seed=0):
    """A pose per instance that is not its rest pose: another rotation and scale about another place on the w x h target."""
    rng = np.random.default_rng(900 + seed)
    rest = rest_poses(instances)
    out = np.zeros_like(rest)
    for i, t in enumerate(rest):
        s = math.hypot(t[0], t[1]) * rng.uniform(0.8, 1.25)
        a = math.atan2(t[1], t[0]) + rng.uniform(0.3, 1.2)
        out[i] = (s * math.cos(a), s * math.sin(a), -s * math.sin(a), s * math.cos(a), rng.uniform(0.15, 0.85) * w, rng.uniform(0.15, 0.85) * h)
    return out


def compose(lib, instances, paints=None):
    """(bytes, Layout) of the composed scene, painted when `paints` is given."""
    if paints is None:
        return ip.compose(lib.packed, lib.layout, lib.fragments, instances)
    packed, _, lay = pp.compose(lib.packed, lib.layout, lib.fragments, instances, paints)
    return packed, lay


def retained_bytes(lib, instances, paints=None):
    """What VELLO_HIP_BUF_SCENE shows of a retained list: the composed (painted) scene with every transform entry the library's,
    verbatim -- the fragments' transform ranges concatenated, not multiplied by anything."""
    packed, lay = compose(lib, instances, paints)
    out = packed.copy()
    L = lib.layout
    src = lib.packed.view(np.uint32)[L.transform_base: L.style_base]
    parts = [src[6 * lib.fragments[int(f)]["transforms"][0]: 6 * lib.fragments[int(f)]["transforms"][1]] for f, _ in instances]
    xf = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)
    assert len(xf) == lay.style_base - lay.transform_base
    out.view(np.uint32)[lay.transform_base: lay.style_base] = xf
    return out, lay


def want(lib, instances, w, h, base, aa, paints=None, view=None):
    """The oracle's image of the composed (painted, viewed) scene."""
    packed, layout = compose(lib, instances, paints)
    if view is not None:
        packed = view_parity.compose(packed, layout, view)
    return pp.oracle_image(lib, packed, layout, w, h, base, aa)


def _numpy_device(poses):
    return np.ascontiguousarray(poses, dtype=np.float32)


def render_retained(engine, w, h, base, aa, poses=None, source="host", device=_numpy_device, out=None, src_stream=None, keep=None):
    """One render_retained call.  source: "rest" (NULL), "host", or "device" (through `device`; the array is appended to `keep`, which
    the caller holds until the frame has finished)."""
    if source == "rest" or poses is None:
        return engine.render_retained(w, h, base, aa, out=out)
    if source == "host":
        return engine.render_retained(w, h, base, aa, transforms=np.ascontiguousarray(poses, dtype=np.float32), out=out)
    d = device(poses)
    if keep is not None:
        keep.append(d)
    return engine.render_retained(w, h, base, aa, transforms=d, out=out, src_stream=src_stream, transforms_is_device=isinstance(d, np.ndarray))


def frame(engine, w, h, base, aa, poses=None, source="host", device=_numpy_device):
    """A blocking retained frame: (image, bump); pools that overflow are grown and the frame is rendered again."""
    keep = []
    for _ in range(12):
        render_retained(engine, w, h, base, aa, poses, source, device, keep=keep)
        r = engine.sync()
        if r != -4:
            break
        assert engine.grow_pools(engine.bump()), "E_CAPACITY, but no pool had to grow"
    assert r == 0, f"sync: {r}"
    return engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4).copy(), engine.bump()


class RetainedEngine(ip.InstanceEngine):
    """What compare_frame sees as the engine: the list is retained once, every blocking render it asks for -- with the COMPOSED bytes,
    which go to the oracle -- is a retained frame under `poses`."""

    def __init__(self, engine, instances, poses, paints=None, source="host", device=_numpy_device):
        super().__init__(engine, instances)
        self._rest, self._poses, self._paints, self._source, self._device = instances, poses, paints, source, device
        self.retains = 0

    def render(self, packed, layout, width, height, base_color, aa, ramps=None):
        e = self._engine
        lay, nbytes = e.instances_layout(self._instances)
        assert lay == layout and nbytes == len(packed), (lay, layout, nbytes, len(packed))
        if not self.retains:
            e.retain_instances(self._rest, paints=self._paints)
            self.retains += 1
        self.frames += 1
        return frame(e, width, height, base_color, aa, self._poses, self._source, self._device)


def compare_retained_frame(engine, lib, instances, poses, w, h, base, aa, name, paints=None, source="host", device=_numpy_device, upload=True,
                           differs=True, **kw):
    """compare_frame of the retained list under `poses` against the oracle on the numpy-composed scene of (fragment_i, X_i); asserts
    that the posed image is not the rest-pose image, so that an engine that ignores `transforms` fails, and that VELLO_HIP_BUF_SCENE
    shows the retained bytes."""
    if upload:
        lib.upload(engine)
    shown = posed(instances, poses) if source != "rest" else instances
    packed, layout = compose(lib, shown, paints)
    re = RetainedEngine(engine, instances, poses, paints, source, device)
    img, ref, bump = parity.compare_frame(re, packed, layout, w, h, base, aa, name, resolved=ip._Late(lib), **kw)
    assert re.frames > 0 and re.retains == 1
    kept, lay = retained_bytes(lib, instances, paints)
    assert lay == layout
    assert np.array_equal(engine.read_buffer("scene", np.uint8, kept.nbytes), kept), f"{name}: VELLO_HIP_BUF_SCENE is not the retained scene"
    cfg = engine.read_buffer("config", np.uint32, 88)
    assert [int(v) for v in cfg[5:15]] == list(layout), f"{name}: VELLO_HIP_BUF_CONFIG does not hold the composed layout"
    if differs:
        assert not np.array_equal(want(lib, instances, w, h, base, aa, paints), ref), f"{name}: the posed image is the rest-pose image: the case proves nothing"
    return img, ref, bump


def scene_list(which, n, w, h, seed):
    """(FragmentLibrary, instances) of `which` fragments (names of instance_parity._scene_fragments / brush_fragments) under affines,
    as instance_parity.check_frame places them."""
    import vello_amd
    from vello_amd import Affine

    brushes = ip.brush_fragments()
    lib = vello_amd.FragmentLibrary([brushes[k] if k in brushes else ip._scene_fragments(k) for k in which])
    rng = np.random.default_rng(seed)
    inst = []
    for k in range(n):
        f = k % len(which)
        sc = rng.uniform(1.0, 3.0) if which[f] in brushes else rng.uniform(0.25, 0.7)
        a = Affine.translate(float(rng.uniform(0.1, 0.7) * w), float(rng.uniform(0.1, 0.7) * h)) * Affine.rotate(float(rng.uniform(-0.6, 0.6))) * Affine.scale(float(sc))
        inst.append((f, tuple(float(v) for v in a.c)))
    return lib, inst


def check_frame(engine, name, which, flags=None, aas=None, w=256, h=200, base=BLACK, n=7, paints=None, source="host", device=_numpy_device):
    """1. Against the oracle: the full compare_frame of a retained list of `which` fragments under turned poses."""
    from vello_amd import AaConfig

    lib, inst = scene_list(which, n, w, h, len(name))
    poses = turned(inst, w, h, len(name))
    try:
        if flags:
            engine.set_debug_flags(**flags)
        for aa in aas or (AaConfig.Msaa16, AaConfig.Area):
            compare_retained_frame(engine, lib, inst, poses, w, h, base, aa, f"{name}_{int(aa)}", paints=paints(len(inst)) if paints else None,
                                   source=source, device=device, tol=1 if int(aa) == 0 else 0)
    finally:
        if flags:
            engine.set_debug_flags()


def some_paints(n):
    return [None if k % 3 == 0 else pp.word(k) for k in range(n)]


# ---------------------------------------------------------------------------------------------------------------
# 2. Against render_instances_painted, bit for bit
# ---------------------------------------------------------------------------------------------------------------
# rows (in words) of the buffers whose slots atomics hand out: two runs of ONE route may differ in their order
_ROWS = {"lines": 6, "tiles": 2, "seg_counts": 2, "segments": 6, "ptcl": 1, "info_bin_data": 1, "bin_headers": 2, "paths": 8, "blend_spill": 1}


def _snapshot(engine, layout, w, h):
    """Every VELLO_HIP_BUF_* but the scene, as far as the frame wrote it, and the whole control block behind the bump counters."""
    b = engine.bump()
    assert b["failed"] == 0, b
    L = layout
    n_tiles = ((w + 15) // 16) * ((h + 15) // 16)
    used = {"config": 88, "tag_monoids": (L.path_data_base - L.path_tag_base) * 20, "path_bboxes": L.n_paths * 24, "bump": 32, "lines": b["lines"] * 24,
            "draw_monoids": L.n_draw_objects * 16, "info_bin_data": (L.bin_data_start + b["binning"]) * 4, "clip_inp": L.n_clips * 8,
            "clip_bboxes": L.n_clips * 16, "draw_bboxes": L.n_draw_objects * 16, "bin_headers": None, "paths": L.n_draw_objects * 32,
            "tiles": b["tile"] * 8, "seg_counts": b["seg_counts"] * 8, "segments": b["segments"] * 24, "ptcl": (64 * n_tiles + b["ptcl"]) * 4,
            "blend_spill": b["blend"] * 4, "output": w * h * 4}
    return {k: engine.read_buffer(k, np.uint32, v).copy() for k, v in used.items()}, b


def _compare_canonical(name, got, ref, bump, ref_bump, layout, w, h):
    """The buffers of _ROWS of a retained frame against the reference route's frame in parity.compare_frame's canonical forms: what
    the order of atomics decides is normalised away, everything else is equal word for word.  (Both are the engine's frames with
    the same culling, so -- unlike compare_back_half -- no second frame is needed: the counters but bump.ptcl are equal.)"""
    L = layout
    n_tiles = ((w + 15) // 16) * ((h + 15) // 16)
    lines_g, lines_r = got["lines"], ref["lines"]
    assert np.array_equal(parity.sorted_rows(parity.canonical_nan_lines(lines_g), 6), parity.sorted_rows(parity.canonical_nan_lines(lines_r), 6)), \
        f"{name}: line soup differs as a multiset"
    assert np.array_equal(got["info_bin_data"][: L.bin_data_start], ref["info_bin_data"][: L.bin_data_start]), f"{name}: draw info differs"
    n_bin = parity.compare_bins(name, got["bin_headers"], got["info_bin_data"], ref["bin_headers"], ref["info_bin_data"], L.n_draw_objects, w, h,
                                L.bin_data_start)
    assert n_bin == ref_bump["binning"], f"{name}: bin lists hold {n_bin} entries, bump.binning {ref_bump['binning']}"
    p_g, p_r = got["paths"].reshape(-1, 8), ref["paths"].reshape(-1, 8)
    assert np.array_equal(p_g[:, :4], p_r[:, :4]), f"{name}: path tile bboxes differ"
    t_g, t_r = got["tiles"].view(np.int32).reshape(-1, 2), ref["tiles"].view(np.int32).reshape(-1, 2)
    for i in range(L.n_draw_objects):  # (tile offsets follow bump order: per path, the backdrops)
        n = int((p_r[i, 2] - p_r[i, 0]) * (p_r[i, 3] - p_r[i, 1]))
        assert not n or np.array_equal(t_g[p_g[i, 4]: p_g[i, 4] + n, 0], t_r[p_r[i, 4]: p_r[i, 4] + n, 0]), f"{name}: tile backdrops differ (path {i})"
    parity.compare_seg_counts(name, got["seg_counts"], lines_g, ref["seg_counts"], lines_r, ref_bump["seg_counts"])
    fg, fr, fn, _ = parity.walk_ptcl_pair(name, got["ptcl"][: 64 * n_tiles + bump["ptcl"]], ref["ptcl"][: 64 * n_tiles + ref_bump["ptcl"]], n_tiles)
    assert int(fn.sum()) <= ref_bump["segments"], f"{name}: CMD_FILLs cover {int(fn.sum())} segments, bump.segments {ref_bump['segments']}"
    parity.compare_segment_slices(name, got["segments"], ref["segments"], fg, fr, fn)
    assert np.array_equal(np.sort(got["blend_spill"]), np.sort(ref["blend_spill"])), f"{name}: blend spill differs as a multiset"


def check_bitwise(engine, name, view=None, cull=False, source="host", device=_numpy_device, painted=True):
    """The same list and poses through render_instances_painted (twice) and through retain + render_retained: every buffer and the bump
    counters equal bit for bit.  Where the reference route's own two frames differ in a buffer -- only the buffers of _ROWS can: the
    order in which atomics hand out their slots is not the frame's -- that buffer is held to the reference frame in
    parity.compare_frame's canonical forms (_compare_canonical: bin lists, tile backdrops, SegmentCounts, PTCL words, per-fill segment
    slices, the line soup as a multiset); everywhere else, and on every buffer when the two reference frames agree, the comparison
    is exact.  Every counter is the reference frame's; bump.ptcl alone may differ, and only where the reference route's two frames
    differ in it (the chunks of a restarted command list).  VELLO_HIP_BUF_SCENE is the one exception: the library's T's verbatim, a
    -0.0 among them."""
    import vello_amd
    from vello_amd import AaConfig, Affine, Color, Fill, Rect, Scene

    w, h, aa = 160, 120, AaConfig.Msaa16
    frs = ip.brush_fragments()
    neg = Scene()  # a transform entry with a -0.0 in it
    neg.fill(Fill.NonZero, Affine((1.0, -0.0, -0.0, 1.0, 3.0, -2.0)), Color.from_rgb8(40, 200, 90), None, Rect(-9.0, -6.0, 9.0, 6.0))
    three = Scene()  # three transform entries in one fragment
    for k in range(3):
        three.fill(Fill.NonZero, Affine.translate(4.0 * k, 3.0 * k) * Affine.rotate(0.3 * k), Color.from_rgb8(60 + 60 * k, 90, 250 - 60 * k), None, Rect(-7.0, -5.0, 7.0, 5.0))
    lib = vello_amd.FragmentLibrary([frs["solid"], neg, frs["clip"], three, frs["linear"], frs["blend"]])
    L = lib.layout
    assert (lib.packed.view(np.uint32)[L.transform_base: L.style_base] == 0x80000000).any(), "no -0.0 in the library's transforms"
    lib.upload(engine)
    rng = np.random.default_rng(17)
    inst = ip.scatter(rng, 23, 6, w, h, scale=(0.8, 2.2))
    poses = turned(inst, w, h, 5)
    paints = some_paints(len(inst)) if painted else None
    shown = posed(inst, poses) if source != "rest" else inst
    packed, layout = compose(lib, shown, paints)
    try:
        if view is not None:
            engine.set_view_transform(view)
        engine.set_viewport_cull(cull)
        refs = []
        for _ in range(2):
            engine.render_instances(shown, w, h, BLACK, aa, paints=paints)
            assert engine.sync() == 0
            assert np.array_equal(engine.read_buffer("scene", np.uint8, packed.nbytes), packed)
            refs.append(_snapshot(engine, layout, w, h))
        engine.retain_instances(inst, paints=paints)
        keep = []
        render_retained(engine, w, h, BLACK, aa, poses, source, device, keep=keep)
        assert engine.sync() == 0
        got, bump = _snapshot(engine, layout, w, h)
    finally:
        engine.set_view_transform(None)
        engine.set_viewport_cull(False)
    (ref, ref_bump), (ref2, ref2_bump) = refs
    assert set(bump) == set(ref_bump) == set(ref2_bump)
    for k, v in ref_bump.items():
        if k == "ptcl" and ref2_bump[k] != v:
            continue  # (chunks of a restarted command list: not the frame's; the command words are walked below)
        assert ref2_bump[k] == v, f"{name}: two frames of the reference route differ in bump.{k}: {ref_bump} {ref2_bump}"
        assert bump[k] == v, f"{name}: bump.{k} {bump[k]} != {v}"
    for k, v in ref.items():
        if np.array_equal(v, ref2[k]):
            assert np.array_equal(got[k], v), f"{name}: VELLO_HIP_BUF_{k.upper()} differs from the render_instances_painted frame"
        else:
            assert k in _ROWS, f"{name}: two frames of the reference route differ in {k}"
    # (always: where nothing is unordered -- the emulator -- the canonical forms hold a fortiori, and the comparison itself is exercised)
    _compare_canonical(name, got, ref, bump, ref_bump, layout, w, h)
    kept, _ = retained_bytes(lib, inst, paints)
    scene = engine.read_buffer("scene", np.uint8, kept.nbytes + 64)
    assert np.array_equal(scene[:kept.nbytes], kept), f"{name}: VELLO_HIP_BUF_SCENE is not the retained scene (the library's T's verbatim)"
    assert not scene[kept.nbytes:].any(), f"{name}: the 64 bytes of slack are not zero"
    assert (kept.view(np.uint32)[layout.transform_base: layout.style_base] == 0x80000000).any()
    img = got["output"].view(np.uint8).reshape(h, w, 4)
    assert np.array_equal(img, want(lib, shown, w, h, BLACK, aa, paints, view)), f"{name}: image"
    if source != "rest":
        assert not np.array_equal(img, want(lib, inst, w, h, BLACK, aa, paints, view)), f"{name}: the poses changed nothing"


# ---------------------------------------------------------------------------------------------------------------
# 3. Kernel shapes
# ---------------------------------------------------------------------------------------------------------------
def shape_library():
    """Polygons (one transform entry each), a fragment of three transform entries, an empty fragment."""
    import vello_amd
    from vello_amd import Affine, Color, Fill, Rect, Scene

    three = Scene()
    for k in range(3):
        three.fill(Fill.NonZero, Affine.translate(3.0 * k, 2.0 * k), Color.from_rgb8(250 - 70 * k, 80 + 60 * k, 60), None, Rect(-4.0, -3.0, 4.0, 3.0))
    lib = vello_amd.FragmentLibrary([ip.polygon(3, r=4.0), ip.polygon(5, r=4.0), three])
    assert [f["transforms"][1] - f["transforms"][0] for f in lib.fragments] == [1, 1, 3]
    lib.three = 2
    lib.empty = len(lib.fragments)
    lib.fragments.append(dict(ip.EMPTY))
    return lib


def _n_xf(lib, inst):
    return sum(lib.fragments[f]["transforms"][1] - lib.fragments[f]["transforms"][0] for f, _ in inst)


def shape_cases(lib):
    """name -> (instances, n_xf): the smallest lists at which a lane per entry, 256 to a workgroup, can go wrong."""
    rng = np.random.default_rng(3)

    def place(frags):
        return [(f, t) for f, (_, t) in zip(frags, ip.scatter(rng, len(frags), 1, 128, 96, scale=(0.6, 1.6)))]

    cases = {"n0": place([]), "xf1": place([0])}
    for n in (255, 256, 257):
        cases[f"xf{n}"] = place([k % 2 for k in range(n)])
    # owners that span lanes, and empty fragments in between, so that owners skip instances
    cases["three_and_empties"] = place([lib.three, lib.empty, lib.empty, 0, lib.empty, lib.three, lib.three, lib.empty, 1] * 7 + [lib.empty])
    cases["only_empty"] = place([lib.empty] * 5)
    cases["same_1000"] = place([1] * 1000)
    # 85 instances of three entries are entries 0 .. 254: the next instance's first entry is slot 256, lane 0 of the second workgroup
    cases["owner_on_boundary"] = place([lib.three] * 85 + [0, lib.three, 1])
    assert _n_xf(lib, cases["owner_on_boundary"][:85]) == 255
    return cases


def check_shapes(engine, name, device=_numpy_device):
    """Every shape under host and device poses: the image is the oracle's, exactly (MSAA8)."""
    from vello_amd import AaConfig

    lib = shape_library()
    lib.upload(engine)
    w, h, aa = 128, 96, AaConfig.Msaa8
    for label, inst in shape_cases(lib).items():
        poses = turned(inst, w, h, len(label))
        engine.retain_instances(inst)
        kept, lay = retained_bytes(lib, inst)
        for source in ("host", "device", "rest"):
            img, bump = frame(engine, w, h, WHITE, aa, poses, source, device)
            shown = inst if source == "rest" else posed(inst, poses)
            assert np.array_equal(img, want(lib, shown, w, h, WHITE, aa)), f"{name}_{label}: image under {source} poses"
            assert np.array_equal(engine.read_buffer("scene", np.uint8, kept.nbytes), kept), f"{name}_{label}: retained bytes"
        if _n_xf(lib, inst) == 0:
            assert (img.reshape(-1, 4) == (255, 255, 255, 255)).all(), f"{name}_{label}: not the base colour"
    # every intermediate of one of them, on a scene with draw data ahead of the transform stream: slot 0 of the frame's copy holds
    # those words verbatim, as the stream's own neighbourhood does in the oracle's scene
    inst = shape_cases(lib)["owner_on_boundary"]
    assert compose(lib, inst)[1].transform_base - compose(lib, inst)[1].draw_data_base >= 6
    compare_retained_frame(engine, lib, inst, turned(inst, w, h, 1), w, h, WHITE, aa, f"{name}_boundary", source="device", device=device, upload=False)


# ---------------------------------------------------------------------------------------------------------------
# 4. Pose sources
# ---------------------------------------------------------------------------------------------------------------
def check_sources(engine, name, device=_numpy_device):
    """NULL is the rest poses; a host array; a device array: three images of one list, each the oracle's; a static list under a
    moving view with no poses at all."""
    import vello_amd
    from vello_amd import AaConfig, Affine

    frs = ip.brush_fragments()
    lib = vello_amd.FragmentLibrary([frs["solid"], frs["linear"], ip.polygon(6), frs["clip"]])
    lib.upload(engine)
    w, h, aa = 128, 96, AaConfig.Msaa16
    rng = np.random.default_rng(8)
    inst = ip.scatter(rng, 11, 4, w, h, scale=(0.8, 2.0))
    engine.retain_instances(inst)
    pa, pb = turned(inst, w, h, 1), turned(inst, w, h, 2)
    w_rest, w_a, w_b = want(lib, inst, w, h, BLACK, aa), want(lib, posed(inst, pa), w, h, BLACK, aa), want(lib, posed(inst, pb), w, h, BLACK, aa)
    assert len({x.tobytes() for x in (w_rest, w_a, w_b)}) == 3
    for source, poses, wnt in (("rest", None, w_rest), ("host", pa, w_a), ("device", pb, w_b), ("rest", None, w_rest), ("device", pa, w_a), ("host", pb, w_b)):
        img, _ = frame(engine, w, h, BLACK, aa, poses, source, device)
        assert np.array_equal(img, wnt), f"{name}: {source} poses"
    try:
        for k in range(3):
            view = Affine.translate(6.0 * k, -4.0 * k) * Affine.rotate(0.1 * (k + 1))
            engine.set_view_transform(view)
            img, _ = frame(engine, w, h, BLACK, aa, None, "rest")
            assert np.array_equal(img, want(lib, inst, w, h, BLACK, aa, view=view)), f"{name}: rest poses under view {k}"
    finally:
        engine.set_view_transform(None)


# ---------------------------------------------------------------------------------------------------------------
# 5. Life cycle
# ---------------------------------------------------------------------------------------------------------------
def check_life_cycle(engine, name, make_target, to_numpy, device=_numpy_device):
    import vello_amd
    import workloads
    from oracle.oracle import Oracle
    from vello_amd import AaConfig

    w, h, aa = 160, 120, AaConfig.Msaa16
    frs = ip.brush_fragments()
    lib = vello_amd.FragmentLibrary([frs["solid"], frs["linear"], frs["clip"], ip.polygon(6), frs["blend"]])
    lib.upload(engine)
    rng = np.random.default_rng(21)
    inst = ip.scatter(rng, 19, 5, w, h, scale=(0.8, 2.5))
    sets = [turned(inst, w, h, k) for k in range(4)]
    wants = [want(lib, posed(inst, p), w, h, BLACK, aa) for p in sets]
    other_list = ip.scatter(rng, 7, 5, w, h, scale=(0.8, 2.5))
    want_other_list = want(lib, other_list, w, h, BLACK, aa)
    want_lib = want(lib, [(k, IDENT) for k in range(5)], w, h, BLACK, aa)
    other, other_layout = workloads.random_test_scene(5, n_paths=60, size=128.0, strokes=True, clips=True).resolve()
    other = np.ascontiguousarray(other, dtype=np.uint8)
    o = Oracle()
    o.set_scene(other, other_layout, w, h, BLACK, int(aa))
    want_scene = o.render().copy()
    assert len({x.tobytes() for x in wants + [want_other_list, want_lib, want_scene]}) == 7
    engine.retain_instances(inst)
    kept, lay = retained_bytes(lib, inst)
    keep = []
    try:
        engine.set_frames_in_flight(4)
        # four frames in flight: four pose sets into four targets, from alternating sources
        for rnd in range(2):
            t = [make_target(w, h) for _ in range(4)]
            for k in range(4):
                render_retained(engine, w, h, BLACK, aa, sets[(k + rnd) % 4], ("host", "device")[k % 2], device, out=t[k], keep=keep)
            assert engine.sync() == 0
            for k in range(4):
                assert np.array_equal(to_numpy(t[k]), wants[(k + rnd) % 4]), f"{name}: round {rnd}, frame {k} does not show its own poses"
        # between render_resident, render_frame and render_instances frames on the rotating lanes
        t = [make_target(w, h) for _ in range(8)]
        render_retained(engine, w, h, BLACK, aa, sets[0], "device", device, out=t[0], keep=keep)
        view_parity.render_resident_into(engine, w, h, BLACK, aa, t[1])
        render_retained(engine, w, h, BLACK, aa, sets[1], "host", out=t[2])
        view_parity.render_frame_into(engine, other, other_layout, w, h, BLACK, aa, t[3])
        render_retained(engine, w, h, BLACK, aa, sets[2], "device", device, out=t[4], keep=keep)
        ip.render_instances_into(engine, other_list, w, h, BLACK, aa, t[5])
        render_retained(engine, w, h, BLACK, aa, sets[3], "host", out=t[6])
        render_retained(engine, w, h, BLACK, aa, None, "rest", out=t[7])
        assert engine.sync() == 0
        for k, wnt in enumerate((wants[0], want_lib, wants[1], want_scene, wants[2], want_other_list, wants[3], want(lib, inst, w, h, BLACK, aa))):
            assert np.array_equal(to_numpy(t[k]), wnt), f"{name}: interleaved frame {k}"
        # no scene allocation across 20 retained frames, whatever the lanes held before
        for k in range(4):
            render_retained(engine, w, h, BLACK, aa, sets[k], "host", out=t[k])
        assert engine.sync() == 0
        before = engine.scene_allocations()
        for k in range(20):
            render_retained(engine, w, h, BLACK, aa, sets[k % 4], ("host", "device")[k % 2], device, out=t[k % 4], keep=keep)
        assert engine.sync() == 0
        assert engine.scene_allocations() == before, f"{name}: {engine.scene_allocations() - before} scene buffers allocated by retained frames"
        for k in range(4):
            assert np.array_equal(to_numpy(t[k]), wants[k]), f"{name}: steady-state frame {k}"
    finally:
        engine.set_frames_in_flight(1)
    # run_stages after a retained frame: from FLATTEN and from DRAW_SCAN, on the frame's composed words
    img, _ = frame(engine, w, h, BLACK, aa, sets[2], "device", device)
    assert np.array_equal(img, wants[2])
    for front_last, first in (("pathtag_scan", "flatten"), ("flatten", "draw_scan"), (None, "pathtag_scan")):
        engine.write_buffer("output", np.zeros(w * h * 4, dtype=np.uint8))
        if front_last:
            engine.run_stages(w, h, BLACK, aa, "pathtag_scan", front_last)
        engine.run_stages(w, h, BLACK, aa, first, "fine")
        assert engine.bump()["failed"] == 0
        assert np.array_equal(engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4), wants[2]), f"{name}: run_stages from {first} after a retained frame"
    # library bytes and retained bytes unchanged
    assert np.array_equal(engine.read_buffer("scene", np.uint8, kept.nbytes), kept), f"{name}: the retained bytes changed"
    engine.render_resident(w, h, BLACK, aa)
    assert engine.sync() == 0
    assert np.array_equal(engine.read_buffer("scene", np.uint8, lib.packed.nbytes), lib.packed), f"{name}: the library's bytes changed"
    # retain twice: the second list replaces the first
    engine.retain_instances(other_list)
    img, _ = frame(engine, w, h, BLACK, aa, None, "rest")
    assert np.array_equal(img, want_other_list), f"{name}: the second retained list did not replace the first"
    p2 = turned(other_list, w, h, 9)
    img, _ = frame(engine, w, h, BLACK, aa, p2, "device", device)
    assert np.array_equal(img, want(lib, posed(other_list, p2), w, h, BLACK, aa))
    # a painted list
    paints = some_paints(len(other_list))
    engine.retain_instances(other_list, paints=paints)
    img, _ = frame(engine, w, h, BLACK, aa, p2, "host")
    assert np.array_equal(img, want(lib, posed(other_list, p2), w, h, BLACK, aa, paints)), f"{name}: painted retained list"
    # uploads drop the list; release, then a frame, is VELLO_HIP_E_INVALID
    for drop in (lambda: engine.upload_scene(lib.packed, lib.layout, lib.ramps), lambda: lib.upload(engine), engine.release_retained):
        lib.upload(engine)
        engine.retain_instances(inst)
        frame(engine, w, h, BLACK, aa, sets[0], "host")
        drop()
        assert _raw(engine, None, 0, None, w, h, BLACK, aa) == -1, f"{name}: a frame of a dropped list was accepted"
    engine.release_retained()  # (none left: still fine)
    lib.upload(engine)
    engine.render_resident(w, h, BLACK, aa)
    assert engine.sync() == 0


def check_overflow(make_engine, name, device=_numpy_device):
    """Pool overflow from tiny pools: E_CAPACITY at sync, grow_pools, then the frame."""
    import vello_amd
    from vello_amd import AaConfig

    w, h, aa = 128, 96, AaConfig.Msaa8
    engine = make_engine(dict(lines=64, seg_counts=64, segments=64, tiles=256))
    lib = vello_amd.FragmentLibrary([ip.polygon(9), ip.polygon(14)])
    lib.upload(engine)
    inst = ip.scatter(np.random.default_rng(4), 30, 2, w, h, scale=(1.0, 2.5))
    poses = turned(inst, w, h, 3)
    engine.retain_instances(inst)
    keep = []
    render_retained(engine, w, h, BLACK, aa, poses, "device", device, keep=keep)
    assert engine.sync() == -4, f"{name}: the tiny pools did not overflow"
    rounds = 0
    while True:
        assert engine.grow_pools(engine.bump()), f"{name}: E_CAPACITY, but no pool had to grow"
        rounds += 1
        render_retained(engine, w, h, BLACK, aa, poses, "device", device, keep=keep)
        r = engine.sync()
        if r != -4:
            break
        assert rounds < 12
    assert r == 0
    img = engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4)
    assert np.array_equal(img, want(lib, posed(inst, poses), w, h, BLACK, aa)), f"{name}: the frame after grow_pools"


# ---------------------------------------------------------------------------------------------------------------
# 6. Refusals
# ---------------------------------------------------------------------------------------------------------------
def _ptr(x):
    if x is None:
        return None
    return x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr() if hasattr(x, "data_ptr") else int(x)


def _raw(engine, transforms, is_device, src_stream, w, h, base, aa, target=None, stride=None):
    p = engine._params(w, h, base, aa)
    return engine._lib.vello_hip_render_retained(engine._h, _ptr(transforms), int(is_device), ctypes.c_void_p(src_stream) if src_stream else None,
                                                 ctypes.byref(p), _ptr(target), w * 4 if stride is None else stride)


def _raw_retain(engine, instances, paints=None, n=None):
    from vello_amd.renderer import instance_array, paint_array

    inst = instance_array(instances) if instances is not None else None
    pt = paint_array(paints) if paints is not None and not isinstance(paints, np.ndarray) else paints
    count = len(inst) if n is None else n
    return engine._lib.vello_hip_retain_instances(engine._h, _ptr(inst), _ptr(pt), count)


def check_errors(engine, name, make_target, to_numpy, device=_numpy_device, host_memory=None):
    """Every VELLO_HIP_E_INVALID of the three entry points.  Four lanes: accepted frame k must take lane k -- VELLO_HIP_BUF_OUTPUT,
    the internal target of the lane that rendered last, then shows what a first round left in lane k's -- so a refusal that moved
    the rotation shows; every target holds its own frame, a refused frame has written none."""
    import vello_amd
    from vello_amd import AaConfig, PAINT_DTYPE

    w, h, aa = 96, 64, AaConfig.Msaa8
    frs = ip.brush_fragments()
    lib = vello_amd.FragmentLibrary([frs["solid"], frs["clip"], ip.polygon(4)])
    lib.upload(engine)
    good = [(0, (1.0, 0.0, 0.0, 1.0, 30.0, 30.0)), (1, (1.5, 0.0, 0.0, 1.5, 60.0, 30.0)), (2, (1.0, 0.0, 0.0, 1.0, 20.0, 44.0))]
    poses = turned(good, w, h, 2)
    t0 = make_target(w, h)
    # no retained list
    assert _raw(engine, None, 0, None, w, h, BLACK, aa, t0) == -1
    assert b"retain" in engine._lib.vello_hip_last_error(engine._h)
    engine.retain_instances(good)
    sets = [turned(good, w, h, 10 + k) for k in range(4)]
    wants = [want(lib, posed(good, p), w, h, BLACK, aa) for p in sets]
    odd = np.zeros(poses.nbytes + 8, dtype=np.uint8)
    bad_paint = np.zeros(len(good), dtype=PAINT_DTYPE)
    bad_paint["flags"][1] = 7
    try:
        engine.set_frames_in_flight(4)
        # round A leaves lane i's INTERNAL target holding image i; the frames of round B have targets of their own and leave it alone
        for k in range(4):
            render_retained(engine, w, h, BLACK, aa, sets[3 - k], "host")
        assert engine.sync() == 0

        def lane_shown():
            return engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4)

        t = [make_target(w, h) for _ in range(5)]
        keep = []
        for k in range(4):
            render_retained(engine, w, h, BLACK, aa, sets[k], ("host", "device")[k % 2], device, out=t[k], keep=keep)
            assert np.array_equal(lane_shown(), wants[3 - k]), f"{name}: frame {k} did not take lane {k}: the lane rotation moved on a refused frame"
            shown = engine.read_buffer("scene", np.uint8, 64)
            # host poses with a NaN or an infinity, naming the instance
            for j, bad in enumerate((float("nan"), float("inf"), float("-inf"))):
                v = poses.copy()
                v[(k + j) % 3, (2 * k + j) % 6] = bad
                assert _raw(engine, v, 0, None, w, h, BLACK, aa, t[k]) == -1
                assert f"instance {(k + j) % 3}".encode() in engine._lib.vello_hip_last_error(engine._h), engine._lib.vello_hip_last_error(engine._h)
            # src_stream with a host pointer, and with no poses
            assert _raw(engine, poses, 0, engine.stream() or 1, w, h, BLACK, aa, t[k]) == -1
            assert _raw(engine, None, 0, engine.stream() or 1, w, h, BLACK, aa, t[k]) == -1
            # a misaligned device pointer; host memory handed in as device memory (GPU builds)
            d = device(poses)
            assert _raw(engine, _ptr(d) + 2, 1, None, w, h, BLACK, aa, t[k]) == -1
            if host_memory is not None:  # (GPU build: host memory handed in as device memory, pageable and pinned)
                for kind, mem in host_memory(poses).items():
                    assert _raw(engine, mem, 1, None, w, h, BLACK, aa, t[k]) == -1, f"{name}: {kind} host memory accepted as device poses"
                    assert b"not device memory" in engine._lib.vello_hip_last_error(engine._h), f"{name}: {kind}"
            # the target contract and the render parameters
            assert _raw(engine, poses, 0, None, w, h, BLACK, aa, t[k], stride=w * 4 - 4) == -1
            assert _raw(engine, poses, 0, None, 0, h, BLACK, aa, t[k]) == -1
            assert _raw(engine, poses, 0, None, w, h, BLACK, 5, t[k]) == -1
            assert engine._lib.vello_hip_render_retained(None, None, 0, None, None, None, 0) == -1
            # every refusal of retain: the earlier list stays
            for bl, pt, n in (([(len(lib.fragments), IDENT)], None, None), (good + [(1, (1.0, 0.0, float("nan"), 1.0, 0.0, 0.0))], None, None),
                              (good, bad_paint, None), (None, None, 2)):
                assert _raw_retain(engine, bl, pt, n) == -1
            assert np.array_equal(engine.read_buffer("scene", np.uint8, 64), shown), f"{name}: a refused call changed what VELLO_HIP_BUF_SCENE shows"
            assert np.array_equal(lane_shown(), wants[3 - k]), f"{name}: a refused call moved the rotation's last lane"
        render_retained(engine, w, h, BLACK, aa, sets[0], "host", out=t[4])
        assert np.array_equal(lane_shown(), wants[3]), f"{name}: the last refusals moved the rotation"
        assert engine.sync() == 0
        for k in range(4):
            assert np.array_equal(to_numpy(t[k]), wants[k]), f"{name}: frame {k} (a refused frame wrote its target, or a refused retain dropped the list?)"
    finally:
        engine.set_frames_in_flight(1)
    # no fragment table: nothing to retain, and the list that was is gone
    engine.upload_scene(lib.packed, lib.layout, lib.ramps)
    assert _raw_retain(engine, good) == -1
    assert _raw(engine, None, 0, None, w, h, BLACK, aa, t0) == -1
    lib.upload(engine)


def check_device_nan(engine, name, make_target, to_numpy, device=_numpy_device):
    """A device pose with a NaN entry on a 64x48 target with a 3-instance list: VELLO_HIP_E_INVALID at sync, the target's bytes
    unchanged, the next frame with finite poses correct."""
    import vello_amd
    from vello_amd import AaConfig

    w, h, aa = 64, 48, AaConfig.Msaa8
    lib = vello_amd.FragmentLibrary([ip.polygon(5), ip.polygon(7), ip.brush_fragments()["solid"]])
    lib.upload(engine)
    inst = [(0, (1.0, 0.0, 0.0, 1.0, 16.0, 16.0)), (1, (1.2, 0.0, 0.0, 1.2, 40.0, 20.0)), (2, (1.0, 0.0, 0.0, 1.0, 30.0, 34.0))]
    poses = turned(inst, w, h, 4)
    engine.retain_instances(inst)
    for bad in (float("nan"), float("inf")):
        t = make_target(w, h)
        if isinstance(t, np.ndarray):
            t[...] = 0x5A
        else:
            t.fill_(0x5A)
        before = to_numpy(t).copy()  # (a copy to the host: the fill has finished)
        assert (before == 0x5A).all()
        v = poses.copy()
        v[1, 4] = bad
        keep = []
        render_retained(engine, w, h, BLACK, aa, v, "device", device, out=t, keep=keep)
        assert engine.sync() == -1, f"{name}: a device pose of {bad} was not found"
        assert np.array_equal(to_numpy(t), before), f"{name}: the discarded frame wrote its target"
        render_retained(engine, w, h, BLACK, aa, poses, "device", device, out=t, keep=keep)
        assert engine.sync() == 0
        assert np.array_equal(to_numpy(t), want(lib, posed(inst, poses), w, h, BLACK, aa)), f"{name}: the frame after a discarded one"
