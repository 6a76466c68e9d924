"""Base images (vello_hip_set_base_image) against the CPU oracle.  The oracle has no such option and none is added: a pixel's result
depends on the base only through its own initial rgba (oracle/vo_fine.c), so for an image built from a palette of K words the
expected pixel (x, y) is pixel (x, y) of the oracle's whole frame rendered with base_color = PALETTE[k(x, y)] -- K oracle renders per
(scene, AA), cached.  k(x, y) = (x // 3 + y // 5) % K: the colour changes inside a lane's four pixels and across tile edges.
Tolerances are tests/damage_parity.py's own: 0 for MSAA8 and MSAA16, 1 for area AA.

`mem` is where "device memory" lives (tests/placement_parity.py): HostMemory for the SIMT-emulated build, TorchMemory for the MI355X."""
import ctypes
import functools

import numpy as np
import pytest

from tests import cull_parity as cp
from tests import damage_parity as dp
from tests import placement_parity as plp

E_INVALID, E_CAPACITY = -1, -4
LEAD = plp.LEAD
# two opaque words, a translucent premultiplied one, transparent black, and one with a channel above its alpha (legal, as for base_color)
PALETTE = (0xFF203040, 0xFFE0C010, 0x80402010, 0x00000000, 0x40FF2010)
K = len(PALETTE)
IGNORED_BASE = 0xFF112233  # params.base_color of frames over an image: no palette word, and never seen
DRAW_TAGS_BRUSH = (0x114, 0x29C, 0x254, 0x28C)  # linear, radial, sweep gradient; image
DRAW_TAG_IMAGE = 0x28C


def palette_index(w, h, shift=0):
    y, x = np.mgrid[0:h, 0:w]
    return (x // 3 + y // 5 + shift) % K


def palette_bytes(w, h, shift=0):
    """The palette image as [h, w, 4] bytes (R in the low byte of a word)."""
    words = np.array(PALETTE, dtype="<u4")[palette_index(w, h, shift)]
    return np.ascontiguousarray(words).view(np.uint8).reshape(h, w, 4)


class Expect:
    """The K oracle frames of one scene, target size and AA mode; `ref` is the first one's Reference (its buffers and counters are
    every frame's: nothing ahead of fine reads the base)."""

    def __init__(self, packed, layout, w, h, aa, resolved=None, oracle=None):
        self.packed, self.layout, self.w, self.h, self.aa, self.resolved = packed, layout, w, h, aa, resolved
        self.ref = dp.Reference(packed, layout, w, h, PALETTE[0], aa, resolved=resolved, oracle=oracle() if oracle else None)
        imgs = [self.ref.img]
        for word in PALETTE[1:]:
            imgs.append(plp.oracle_image(packed, layout, w, h, word, aa, resolved) if oracle is None
                        else dp.Reference(packed, layout, w, h, word, aa, resolved=resolved, oracle=oracle()).img)
        self.imgs = np.stack(imgs)
        assert len({im.tobytes() for im in imgs}) == K, "two palette words give one frame: the scene hides its base"
        self.tol = 1 if int(aa) == 0 else 0

    def image(self, shift=0):
        yy, xx = np.mgrid[0:self.h, 0:self.w]
        return self.imgs[palette_index(self.w, self.h, shift), yy, xx]

    def uniform(self, k):
        return self.imgs[k]

    @property
    def ramps(self):
        return self.resolved.ramps if self.resolved is not None else None


@functools.lru_cache(maxsize=None)
def main_expect(which, aa):
    """damage_parity's three scenes at 300 x 280."""
    from vello_amd import AaConfig

    r = dp.main_reference(which, AaConfig(aa))
    return Expect(r.packed, r.layout, r.w, r.h, AaConfig(aa))


@functools.lru_cache(maxsize=None)
def small_expect(aa, w=37, h=19):
    """A 37 x 19 target: a partial tile both ways and a partial lane group."""
    import workloads
    from vello_amd import AaConfig

    packed, layout = workloads.random_test_scene(2, n_paths=60, size=48.0, strokes=True, clips=True).resolve()
    return Expect(packed, layout, w, h, AaConfig(aa))


# ---------------------------------------------------------------------------------------------------------------
# Memory
# ---------------------------------------------------------------------------------------------------------------
def put(view, rows):
    """[h, w, 4] bytes into a view of a surface (numpy: the emulated build's device memory; a torch tensor on the GPU)."""
    if isinstance(view, np.ndarray):
        view[...] = rows
    else:
        import torch

        view.copy_(torch.from_numpy(np.ascontiguousarray(rows)).to(view.device))
        torch.cuda.synchronize()


class Placed:
    """A surface of seeded random bytes with a [h, w, 4] view `lead` bytes in, rows `stride` bytes apart."""

    def __init__(self, mem, w, h, stride, lead, seed, rows=None):
        self.mem, self.w, self.h, self.stride, self.lead = mem, w, h, stride, lead
        self.buf = mem.surface(lead + h * stride + LEAD, seed)
        self.view = mem.view(self.buf, lead, h, w, stride)
        if rows is not None:
            put(self.view, rows)
        self.before = mem.numpy(self.buf)

    def address(self):
        return self.mem.address(self.buf) + self.lead

    def after(self):
        return self.mem.numpy(self.buf)

    def rows(self, flat):
        return flat[self.lead: self.lead + self.h * self.stride].reshape(self.h, self.stride)

    def assert_unchanged(self, name):
        assert np.array_equal(self.after(), self.before), f"{name}: the surface was written"

    def check(self, name, img, rect, tol):
        """Inside `rect` (None: the whole target) `img` within tol; every other byte of the surface as it was."""
        got = self.after()
        outside = np.ones(got.size, dtype=bool)
        outside[self.lead: self.lead + self.h * self.stride] = False
        assert np.array_equal(got[outside], self.before[outside]), f"{name}: bytes in front of or behind the target's rows were written"
        dp.check_pixels(name, self.rows(got), self.rows(self.before), img, rect if rect is not None else (0, 0, self.w, self.h), tol)


def image_surface(mem, ex, seed, img_lead=0, img_pad=12, shift=0):
    """The palette image somewhere in device memory: rows img_pad bytes apart beyond width * 4, the first one img_lead bytes past a
    16-byte boundary (0: the 16-byte loads; 4: word by word)."""
    return Placed(mem, ex.w, ex.h, ex.w * 4 + img_pad, LEAD + img_lead, 0x1A6E00 + seed, palette_bytes(ex.w, ex.h, shift))


class over:
    """with over(engine, image view[, rect]): the settings for the frames inside, taken off again whatever happens."""

    def __init__(self, engine, image, rect=None, **kw):
        self.engine, self.image, self.rect, self.kw = engine, image, rect, kw

    def __enter__(self):
        self.engine.set_base_image(self.image, **self.kw)
        if self.rect is not None:
            self.engine.set_damage_rect(self.rect)

    def __exit__(self, *exc):
        self.engine.set_base_image(None)
        self.engine.set_damage_rect(None)


def frame_over(engine, mem, ex, name, pad=8, lead_extra=0, img_lead=0, img_pad=12, rect=None, in_place=False, seed=0, shift=0):
    """One blocking vello_hip_render of ex's scene over the palette image into a caller's device target.  in_place: the target is
    pre-filled with the image and the image IS the target.  Returns the bump."""
    w, h = ex.w, ex.h
    pal = palette_bytes(w, h, shift)
    target = Placed(mem, w, h, w * 4 + pad, LEAD + lead_extra, seed, pal if in_place else None)
    image = target if in_place else image_surface(mem, ex, seed, img_lead, img_pad, shift)
    with over(engine, image.view, rect):
        _, bump = engine.render(ex.packed, ex.layout, w, h, IGNORED_BASE, ex.aa, ramps=ex.ramps, out=target.view, out_is_device=True)
    assert bump["failed"] == 0, f"{name}: {bump}"
    target.check(name, ex.image(shift), rect, ex.tol)
    if not in_place:
        image.assert_unchanged(name + ": the image")
    return bump


# ---------------------------------------------------------------------------------------------------------------
# 1. The matrix
# ---------------------------------------------------------------------------------------------------------------
CONFIGS = {f"{which}_aa{aa}": (which, aa) for which in ("clipped", "polygons", "opaque_polygons", "small") for aa in (0, 1, 2)}


def check_matrix(engine, mem, name, config):
    """Both load forms (an image address that is 16-byte aligned, one that is 4-byte aligned only), image stride > width * 4; the
    target equals the palette expectation, its padding and the bytes around it are untouched; the buffers ahead of fine are the
    oracle's."""
    which, aa = CONFIGS[config]
    ex = small_expect(aa) if which == "small" else main_expect(which, aa)
    k = sorted(CONFIGS).index(config)
    for j, (img_lead, lead_extra) in enumerate(((0, 0), (4, (4, 8, 12)[k % 3]))):
        bump = frame_over(engine, mem, ex, f"{name}_{config}_img{img_lead}", lead_extra=lead_extra, img_lead=img_lead, seed=2 * k + j)
    dp.check_front_half(f"{name}_{config}", engine, ex.ref, bump)
    dp.check_back_half(f"{name}_{config}", engine, ex.ref, bump, (0, 0, ex.w, ex.h), no_cull=False)


# ---------------------------------------------------------------------------------------------------------------
# 2. The BRUSHES form
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def brushes_expect(aa):
    import vello_amd
    import workloads
    from vello_amd import AaConfig

    r = vello_amd.Resolver().resolve(workloads.brushes_scene())
    tags = np.ascontiguousarray(r.packed, dtype=np.uint8).view(np.uint32)[r.layout.draw_tag_base: r.layout.draw_tag_base + r.layout.n_draw_objects]
    # (what Frame::brushes is worked out from: the scene's draw tags)
    assert any(int(t) in DRAW_TAGS_BRUSH[:3] for t in tags) and DRAW_TAG_IMAGE in [int(t) for t in tags], "no gradient and image draw: fine's plain form would run"
    return Expect(r.packed, r.layout, 256, 256, AaConfig(aa), resolved=r), r


def check_brushes(engine, mem, name, aa):
    ex, r = brushes_expect(aa)
    engine.upload_resolved(r)
    for img_lead in (0, 4):
        target = Placed(mem, ex.w, ex.h, ex.w * 4 + 4, LEAD, 40 + img_lead)
        image = image_surface(mem, ex, 41 + img_lead, img_lead)
        with over(engine, image.view):
            engine.render_resident(ex.w, ex.h, IGNORED_BASE, ex.aa, out=target.view)
            assert engine.sync() == 0
        target.check(f"{name}_aa{aa}_img{img_lead}", ex.image(), None, ex.tol)


# ---------------------------------------------------------------------------------------------------------------
# 3. Slices and the blend spill
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sliced_expect(aa):
    import workloads
    from vello_amd import AaConfig

    packed, layout = workloads.random_test_scene(2, n_paths=300, size=128.0, strokes=True, clips=True).resolve()
    return Expect(packed, layout, 128, 128, AaConfig(aa))


def check_slices(engine, mem, name, aa):
    """Every tile's list cut into slices (VELLO_HIP_DEBUG_FINE_SLICES): blend_pass reads the base, the slices' waves read none."""
    ex = sliced_expect(aa)
    engine.set_debug_flags(fine_slices=True)
    try:
        for img_lead, rect in ((0, None), (4, (5, 3, 101, 97))):
            frame_over(engine, mem, ex, f"{name}_aa{aa}_img{img_lead}", img_lead=img_lead, rect=rect, seed=50 + img_lead)
            assert engine.fine_slice_stats()[0] > 0, f"{name}: no tile was sliced: the case proves nothing"
        frame_over(engine, mem, ex, f"{name}_aa{aa}_in_place", in_place=True, seed=55)
    finally:
        engine.set_debug_flags()


@functools.lru_cache(maxsize=None)
def deep_expect():
    """damage_parity.check_blend_spill's scene: nested deeper than BLEND_STACK_SPLIT clips in every tile."""
    import workloads
    from vello_amd import AaConfig, Affine, BlendMode, Compose, Fill, Mix, Rect, Scene

    s = Scene()
    for d in range(4):
        s.push_layer(Fill.NonZero, BlendMode((Mix.Screen, Mix.Normal)[d % 2], Compose.SrcOver), 0.9, Affine.IDENTITY, Rect(-8.0, -8.0, 136.0, 136.0))
    s.append(workloads.clip_blend_scene(size=128.0, depth=6))
    for d in range(4):
        s.pop_layer()
    packed, layout = s.resolve()
    ex = Expect(packed, layout, 128, 128, AaConfig.Msaa16)
    depth = max(dp.tile_blend_depth(ex.ref.ptcl, t) for t in range(ex.ref.n_tiles))
    assert depth > dp.BLEND_STACK_SPLIT and ex.ref.bump["blend"] > 0, depth
    return ex


def check_blend_spill(engine, mem, name):
    ex = deep_expect()
    bump = frame_over(engine, mem, ex, name, img_lead=4, seed=60)
    assert bump["blend"] == ex.ref.bump["blend"], f"{name}: {bump}"
    engine.set_debug_flags(fine_slices=True)
    try:
        frame_over(engine, mem, ex, name + "_sliced", seed=61)
    finally:
        engine.set_debug_flags()


# ---------------------------------------------------------------------------------------------------------------
# 4. In place, 5. damage + a separate image
# ---------------------------------------------------------------------------------------------------------------
IN_PLACE_RECTS = (None, (5, 3, 30, 17), (16, 16, 32, 32))


def check_in_place(engine, mem, name, aa):
    """The target holds the palette image and image == out: inside R the expectation, every other byte as before the frame."""
    for ex, tag in ((small_expect(aa), "small"), (main_expect("clipped", aa), "main")):
        for k, rect in enumerate(IN_PLACE_RECTS):
            frame_over(engine, mem, ex, f"{name}_{tag}_aa{aa}_{rect}", rect=rect, in_place=True, lead_extra=(0, 4, 8)[k], seed=70 + k)


def check_damage_separate(engine, mem, name, aa):
    ex = main_expect("clipped", aa)
    for k, rect in enumerate(((5, 3, 30, 17), (16, 16, 32, 32), (37, 21, 150, 99), (297, 277, 300, 280))):
        frame_over(engine, mem, ex, f"{name}_aa{aa}_{rect}", rect=rect, img_lead=(0, 4)[k % 2], lead_extra=(0, 12)[k // 2], seed=80 + k)
    # an empty R: nothing is written
    target = Placed(mem, ex.w, ex.h, ex.w * 4, LEAD, 85)
    image = image_surface(mem, ex, 86)
    with over(engine, image.view, (100, 50, 100, 200)):
        engine.render(ex.packed, ex.layout, ex.w, ex.h, IGNORED_BASE, ex.aa, out=target.view, out_is_device=True)
    target.assert_unchanged(name + "_empty")


# ---------------------------------------------------------------------------------------------------------------
# 6. Equivalences
# ---------------------------------------------------------------------------------------------------------------
def check_uniform(engine, mem, name):
    """A uniform image gives the base_color frame: target, every buffer check_front_half / check_back_half read, every bump counter;
    set then NULL gives the off state."""
    from vello_amd import AaConfig
    from tests.parity import sorted_rows

    ex = main_expect("opaque_polygons", int(AaConfig.Msaa16))
    w, h, ref = ex.w, ex.h, ex.ref

    def frame(image, base):
        target = Placed(mem, w, h, w * 4 + 8, LEAD, 90)
        engine.set_base_image(image)
        try:
            _, bump = engine.render(ex.packed, ex.layout, w, h, base, ex.aa, out=target.view, out_is_device=True)
        finally:
            engine.set_base_image(None)
        return target, bump, dp.snapshot(engine, ref, bump)

    for k in (0, 2):
        word = PALETTE[k]
        t0, b0, s0 = frame(None, word)
        t0.check(f"{name}_off_{k}", ex.uniform(k), None, 0)
        rows = np.broadcast_to(np.array([word], dtype="<u4").view(np.uint8), (h, w, 4))
        image = Placed(mem, w, h, w * 4 + 16, LEAD, 91, rows)
        t1, b1, s1 = frame(image.view, IGNORED_BASE)
        t1.check(f"{name}_uniform_{k}", ex.uniform(k), None, 0)
        assert np.array_equal(t1.after(), t0.after()), f"{name}: the uniform image's target is not the base colour's"
        assert b1 == b0, f"{name}: bump {b1}, off state {b0}"
        for key in s0:
            if key in ("lines", "segments"):  # (which slot a row gets is the order of atomics, between any two frames)
                assert np.array_equal(sorted_rows(s1[key].view(np.uint32), 6), sorted_rows(s0[key].view(np.uint32), 6)), f"{name}: {key}"
            elif key in ("tag_monoids", "path_bboxes", "draw_monoids", "clip_bboxes", "draw_bboxes"):
                assert np.array_equal(s1[key], s0[key]), f"{name}: {key} differs from the off state's"
            elif key == "control":
                assert np.array_equal(s1[key][:16], s0[key][:16]) and np.array_equal(s1[key][16:50], s0[key][16:50]), f"{name}: control block"
            else:
                assert s1[key].shape == s0[key].shape, f"{name}: {key}"
        dp.check_front_half(f"{name}_uniform_{k}", engine, ref, b1)
        dp.check_back_half(f"{name}_uniform_{k}", engine, ref, b1, (0, 0, w, h), no_cull=False)
        # set, then NULL: the off state
        t2, b2, _ = frame(None, word)
        assert np.array_equal(t2.after(), t0.after()) and b2 == b0, f"{name}: set then NULL is not the off state"


def check_no_instances(engine, mem, name):
    """An instance frame with n == 0 shows the image's own words, un-premultiplied (the oracle's frame of the empty composed scene)."""
    from tests import instance_parity as ip
    from tests import retained_parity as rp
    from vello_amd import AaConfig

    w, h = 40, 24
    lib, _ = rp.scene_list(["solid", "clip"], 3, w, h, 31)
    lib.upload(engine)
    packed, layout = ip.compose(lib.packed, lib.layout, lib.fragments, [])
    imgs = np.stack([plp.oracle_image(packed, layout, w, h, word, AaConfig.Msaa8, ip._Late(lib)) for word in PALETTE])
    assert all((imgs[k] == imgs[k][0, 0]).all() for k in range(K))
    yy, xx = np.mgrid[0:h, 0:w]
    want = imgs[palette_index(w, h), yy, xx]
    for img_lead in (0, 4):
        target = Placed(mem, w, h, w * 4 + 8, LEAD, 95)
        image = Placed(mem, w, h, w * 4 + 12, LEAD + img_lead, 96, palette_bytes(w, h))
        with over(engine, image.view):
            engine.render_instances([], w, h, IGNORED_BASE, AaConfig.Msaa8, out=target.view)
            assert engine.sync() == 0
        target.check(f"{name}_img{img_lead}", want, None, 0)


# ---------------------------------------------------------------------------------------------------------------
# 7. Frames in flight
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def in_flight_expect(aa):
    from vello_amd import AaConfig

    r = dp.main_reference("clipped", AaConfig.Msaa16)
    return Expect(r.packed, r.layout, dp.IN_FLIGHT_W, dp.IN_FLIGHT_H, AaConfig(aa))


def check_in_flight(engine, mem, name, aa):
    """Four frames enqueued back to back into four targets: three over different images, one over none.  Each target shows its own
    image (MSAA: a non-brush scene with frames in flight takes fine's WAVES = 5 instantiation)."""
    ex = in_flight_expect(aa)
    w, h = ex.w, ex.h
    engine.upload_scene(ex.packed, ex.layout)
    engine.set_frames_in_flight(4)
    try:
        shifts = (0, 1, None, 3)
        targets = [Placed(mem, w, h, w * 4 + 8, LEAD + (0, 4, 0, 12)[j], 100 + j) for j in range(4)]
        images = [None if s is None else image_surface(mem, ex, 110 + j, (0, 4, 0, 0)[j], shift=s) for j, s in enumerate(shifts)]
        for round_ in range(2):  # (the second round's frames follow frames with other settings on the same lanes)
            for j in range(4):
                engine.set_base_image(None if images[j] is None else images[j].view)
                engine.render_resident(w, h, PALETTE[1] if images[j] is None else IGNORED_BASE, ex.aa, out=targets[j].view)
            engine.set_base_image(None)
            assert engine.sync() == 0
            for j, s in enumerate(shifts):
                targets[j].check(f"{name}_aa{aa}_round{round_}_frame{j}", ex.uniform(1) if s is None else ex.image(s), None, ex.tol)
    finally:
        engine.set_base_image(None)
        engine.set_frames_in_flight(1)


# ---------------------------------------------------------------------------------------------------------------
# 8. The other entry points: frames into the lane's internal target through the other parity modules' adapters
# ---------------------------------------------------------------------------------------------------------------
def internal_frame(adapter, engine, mem, ex, name, img_lead=0, seed=0):
    """adapter.render(...) -- a blocking frame of ex's scene its own way, read back from VELLO_HIP_BUF_OUTPUT -- over the palette image."""
    image = image_surface(mem, ex, 120 + seed, img_lead)
    with over(engine, image.view):
        img, bump = adapter.render(ex.packed, ex.layout, ex.w, ex.h, IGNORED_BASE, ex.aa, ramps=ex.ramps)
    assert bump["failed"] == 0, f"{name}: {bump}"
    diff = np.abs(np.asarray(img).astype(np.int32) - ex.image().astype(np.int32))
    print(f"{name}: max difference {diff.max()} (tolerance {ex.tol})")
    assert diff.max() <= ex.tol, f"{name}: differs from the palette expectation: max {diff.max()}, {(diff > ex.tol).sum()} values"
    image.assert_unchanged(name + ": the image")


def check_render_frame(engine, mem, name):
    internal_frame(dp._FrameEngine(engine), engine, mem, small_expect(0), name + "_area", img_lead=4)
    internal_frame(dp._FrameEngine(engine), engine, mem, small_expect(2), name + "_msaa16")


def check_out_none(engine, mem, name):
    ex = small_expect(1)
    internal_frame(dp._ResidentEngine(engine, ex.packed, ex.layout), engine, mem, ex, name)


def check_host_target(engine, mem, name):
    """The blocking vello_hip_render with a host target: the image lies under the lane's internal target, the copy-out is unchanged."""
    ex = small_expect(2)
    image = image_surface(mem, ex, 130, 4)
    out = np.zeros((ex.h, ex.w, 4), dtype=np.uint8)
    with over(engine, image.view):
        _, bump = engine.render(ex.packed, ex.layout, ex.w, ex.h, IGNORED_BASE, ex.aa, out=out)
    assert bump["failed"] == 0 and np.array_equal(out, ex.image()), name


def check_morphed(engine, mem, name):
    from tests import morph_parity as mp
    from vello_amd import AaConfig

    packed, layout = mp.small_triangles_scene(120, size=96.0)
    keys = mp.two_keys(packed, layout)
    morph = (0, 1, 0.375)
    want = mp.expected_words(mp.path_words(packed, layout), keys, None, *morph)
    ex = Expect(mp.substitute(packed, layout, want), layout, 100, 70, AaConfig.Msaa16)
    internal_frame(mp.MorphEngine(engine, packed, morph, keys), engine, mem, ex, name)


def check_retained_painted(engine, mem, name):
    from tests import instance_parity as ip
    from tests import repaint_parity as rpp
    from tests import retained_parity as rp
    from vello_amd import AaConfig

    w, h = 96, 72
    lib, inst = rp.scene_list(["solid", "linear", "clip", "blend"], 6, w, h, 31)
    lib.upload(engine)
    p = [None] * len(inst)
    p[1] = 0xFF10E0F0
    packed, layout = rp.compose(lib, inst, rpp.effective(None, p, len(inst)))
    ex = Expect(packed, layout, w, h, AaConfig.Msaa8, resolved=ip._Late(lib))
    internal_frame(rpp.RepaintEngine(engine, inst, None, dict(paints=p)), engine, mem, ex, name, img_lead=4)


def check_with_view(engine, mem, name):
    from tests import view_parity as vp
    from vello_amd import AaConfig, Affine

    raw = small_expect(2)
    packed = np.ascontiguousarray(raw.packed, dtype=np.uint8)
    view = Affine.translate(-4.0, -2.5) * Affine.scale(1.3)
    ex = Expect(vp.compose(packed, raw.layout, view), raw.layout, raw.w, raw.h, AaConfig.Msaa16)
    assert not np.array_equal(ex.imgs[0], raw.imgs[0])
    internal_frame(vp.ViewEngine(engine, packed, view), engine, mem, ex, name)


def check_with_stroke_scale(engine, mem, name):
    from tests import stroke_scale_parity as ssp
    from vello_amd import AaConfig

    raw = small_expect(2)
    packed = np.ascontiguousarray(raw.packed, dtype=np.uint8)
    setting = (2.5, 1.0)
    ex = Expect(ssp.scaled(packed, raw.layout, setting), raw.layout, raw.w, raw.h, AaConfig.Msaa16)
    assert not np.array_equal(ex.imgs[0], raw.imgs[0]), "the stroke scale does not show"
    internal_frame(ssp.StrokeEngine(engine, packed, setting), engine, mem, ex, name, img_lead=4)


def check_run_stages(engine, mem, name):
    """vello_hip_run_stages(COARSE .. FINE) over an image, behind a front half run without one; a range without FINE asks nothing."""
    ex = small_expect(2)
    w, h = ex.w, ex.h
    engine.render(ex.packed, ex.layout, w, h, PALETTE[0], ex.aa)  # (sizes the internal target)
    engine.write_buffer("output", np.random.default_rng(5).integers(0, 256, w * h * 4, dtype=np.uint8))
    engine.upload_scene(ex.packed, ex.layout)
    image = image_surface(mem, ex, 140, 4)
    engine.run_stages(w, h, IGNORED_BASE, ex.aa, "pathtag_scan", "backdrop")
    with over(engine, image.view):
        engine.run_stages(w, h, IGNORED_BASE, ex.aa, "coarse", "fine")
    bump = engine.bump()
    got = engine.read_buffer("output", np.uint8, w * h * 4).reshape(h, w, 4)
    assert bump["failed"] == 0 and np.array_equal(got, ex.image()), name
    dp.check_front_half(name, engine, ex.ref, bump)


# ---------------------------------------------------------------------------------------------------------------
# 9. A failed frame
# ---------------------------------------------------------------------------------------------------------------
def check_failed_frame(make_engine, mem, name):
    """A segment pool too small: VELLO_HIP_E_CAPACITY, the target untouched -- in place too -- and the image unchanged."""
    from vello_amd import AaConfig

    ex = main_expect("clipped", int(AaConfig.Msaa16))
    eng = make_engine({"segments": ex.ref.bump["segments"] // 2})
    for in_place in (False, True):
        target = Placed(mem, ex.w, ex.h, ex.w * 4 + 8, LEAD, 150, palette_bytes(ex.w, ex.h) if in_place else None)
        image = target if in_place else image_surface(mem, ex, 151)
        with over(eng, image.view):
            _, bump = eng.render(ex.packed, ex.layout, ex.w, ex.h, IGNORED_BASE, ex.aa, out=target.view, out_is_device=True)
        assert bump["failed"] != 0 and eng.sync() == E_CAPACITY, f"{name}: {bump}"
        target.assert_unchanged(f"{name}_in_place{in_place}: the target")
        image.assert_unchanged(f"{name}_in_place{in_place}: the image")


# ---------------------------------------------------------------------------------------------------------------
# 10. Refusals
# ---------------------------------------------------------------------------------------------------------------
def check_refusals(engine, mem, name, host_address=None):
    """Every rule of contract point 5; after each, a good frame over the image that was set before it is correct."""
    ex = small_expect(2)
    w, h = ex.w, ex.h
    lib, eh = engine._lib, engine._h
    image = image_surface(mem, ex, 160)
    addr, stride = image.address(), image.stride

    def good(tag):
        # the setting stands as it was before the refusal: the image set below
        target = Placed(mem, w, h, w * 4 + 8, LEAD, 161)
        _, bump = engine.render(ex.packed, ex.layout, w, h, IGNORED_BASE, ex.aa, out=target.view, out_is_device=True)
        assert bump["failed"] == 0
        target.check(f"{name}: the frame after {tag}", ex.image(), None, 0)

    def refused(r, tag, *words):
        assert r == E_INVALID, f"{name} {tag}: {r}"
        err = lib.vello_hip_last_error(eh).decode()
        assert all(wd in err for wd in words), f"{name} {tag}: the error does not name the rule: {err!r}"

    engine.upload_scene(ex.packed, ex.layout)
    engine.set_frames_in_flight(2)
    try:
        engine.set_base_image(addr, stride)
        good("the set")
        # at the call
        assert lib.vello_hip_set_base_image(None, addr, stride, None) == E_INVALID
        refused(lib.vello_hip_set_base_image(eh, addr + 2, stride, None), "address + 2", "address", "multiple of 4")
        refused(lib.vello_hip_set_base_image(eh, addr, stride + 2, None), "stride + 2", "stride", "multiple of 4")
        refused(lib.vello_hip_set_base_image(eh, addr, 1 << 32, None), "stride 2^32", "stride", "2^32")
        refused(lib.vello_hip_set_base_image(eh, None, 0, ctypes.c_void_p(8)), "a stream without an image", "src_stream")
        good("the refusals at the call")
        # when a frame is enqueued: nothing is enqueued, the rotation stays -- the two lanes go on alternating, which the frames
        # in flight below show by landing in their own targets
        p = engine._params(w, h, IGNORED_BASE, ex.aa)
        target = Placed(mem, w, h, w * 4 + 8, LEAD, 162)
        tptr, tstride = target.address(), target.stride

        def enqueue():
            return lib.vello_hip_render_resident(eh, ctypes.byref(p), ctypes.c_void_p(tptr), tstride)

        engine.set_base_image(addr, w * 4 - 4)
        refused(enqueue(), "a stride below width * 4", "stride", "width * 4")
        # the image shifted one row against the target
        engine.set_base_image(tptr + tstride, tstride)
        refused(enqueue(), "a partial overlap", "overlap")
        engine.set_base_image(tptr + 4, tstride)
        refused(enqueue(), "a partial overlap by a pixel", "overlap")
        engine.set_base_image(tptr, tstride + 4)
        refused(enqueue(), "the target's address under another stride", "overlap")
        if host_address is not None:  # (GPU builds)
            engine.set_base_image(host_address, w * 4)
            refused(enqueue(), "host memory", "device memory")
        assert engine.sync() == 0
        target.assert_unchanged(name + ": the refused frames' target")
        engine.set_base_image(addr, stride)
        good("the refusals at the enqueue")
        # two frames in flight after the refusals: each lands in its own target
        ta, tb = Placed(mem, w, h, w * 4, LEAD, 163), Placed(mem, w, h, w * 4, LEAD, 164)
        engine.render_resident(w, h, IGNORED_BASE, ex.aa, out=ta.view)
        engine.set_base_image(None)
        engine.render_resident(w, h, PALETTE[1], ex.aa, out=tb.view)
        assert engine.sync() == 0
        ta.check(name + ": in flight, over the image", ex.image(), None, 0)
        tb.check(name + ": in flight, over none", ex.uniform(1), None, 0)
    finally:
        engine.set_base_image(None)
        engine.set_frames_in_flight(1)


# ---------------------------------------------------------------------------------------------------------------
# 12. The public layers
# ---------------------------------------------------------------------------------------------------------------
def check_engine_binding(engine, mem, name):
    """Engine.set_base_image with a [h, w, 4] uint8 view, a [h, w] int32 one and a raw address."""
    ex = small_expect(1)
    w, h = ex.w, ex.h
    image = Placed(mem, w, h, w * 4, LEAD, 170, palette_bytes(w, h))
    if isinstance(image.view, np.ndarray):
        as_words = image.view.view(np.int32).reshape(h, w)
    else:
        import torch

        as_words = image.view.view(torch.int32).reshape(h, w)
    assert (as_words.ctypes.data if isinstance(as_words, np.ndarray) else as_words.data_ptr()) == image.address()
    for tag, args in (("bytes", (image.view,)), ("words", (as_words,)), ("address", (image.address(), w * 4)), ("address_stride0", (image.address(),))):
        target = Placed(mem, w, h, w * 4 + 8, LEAD, 171)
        engine.set_base_image(*args)
        try:
            engine.render(ex.packed, ex.layout, w, h, IGNORED_BASE, ex.aa, out=target.view, out_is_device=True)
        finally:
            engine.set_base_image()
        target.check(f"{name}_{tag}", ex.image(), None, 0)
    with pytest.raises(ValueError):
        engine.set_base_image(np.zeros((h, w, 3), dtype=np.uint8))
    with pytest.raises(ValueError):
        engine.set_base_image(np.zeros((h, w), dtype=np.float32))
    with pytest.raises(ValueError):
        engine.set_base_image(image.view, stride=w * 4 + 4)


def check_renderer(mem, name):
    """Renderer.render_to_texture with RenderParams(base_image=...): that frame only; the next one is the off state."""
    import vello_amd
    import workloads
    from vello_amd import AaConfig, Color, RenderParams

    scene = cp.view_of(workloads.random_test_scene(3, n_paths=300, size=512.0, strokes=True, clips=True), 205, 154)
    w, h = 75, 51
    r = vello_amd.Renderer()
    black = Color.from_rgb8(0, 0, 0)
    packed, layout = scene.resolve()
    ex = Expect(packed, layout, w, h, AaConfig.Msaa16)
    plain = np.zeros((h, w, 4), dtype=np.uint8)
    r.render_to_texture(scene, plain, RenderParams(black, w, h, AaConfig.Msaa16))
    image = image_surface(mem, ex, 180, 4)
    out = np.zeros((h, w, 4), dtype=np.uint8)
    r.render_to_texture(scene, out, RenderParams(black, w, h, AaConfig.Msaa16, base_image=image.view))
    assert np.array_equal(out, ex.image()), f"{name}: the frame over the image"
    out = np.zeros((h, w, 4), dtype=np.uint8)
    r.render_to_texture(scene, out, RenderParams(black, w, h, AaConfig.Msaa16))
    assert np.array_equal(out, plain), f"{name}: the call after one over an image is not the off state"
    with pytest.raises(vello_amd.VelloHipError):
        r.render_to_texture(scene, out, RenderParams(black, w, h, AaConfig.Msaa16, base_image=(image.address(), w * 4 - 4)))
    out = np.zeros((h, w, 4), dtype=np.uint8)
    r.render_to_texture(scene, out, RenderParams(black, w, h, AaConfig.Msaa16))
    assert np.array_equal(out, plain), f"{name}: the call after a refused one is not the off state"
