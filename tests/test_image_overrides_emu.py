"""Image overrides without a GPU: vello_hip_copy_images_device (k_atlas_copy) and the Renderer's override_image /
mark_override_image_dirty / register_texture bookkeeping, run on the SIMT-emulated build of the kernel sources.  There the
"device" sources are numpy arrays: the emulated runtime's device memory is host memory."""
import numpy as np
import pytest

import vello_amd
from oracle.oracle import Oracle
from vello_amd import AaConfig, Affine, Color, ImageBrush, ImageData, ImageQuality, RenderParams, Scene, VelloHipError

WHITE = 0xFFFFFFFF
E_INVALID = -1


def _pixels(rng, h, w, opaque=True):
    px = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    if opaque:
        px[:, :, 3] = 255
    return px


def _oracle_frame(r, atlas, width, height, aa, base=WHITE):
    o = Oracle()
    o.set_scene(r.packed, r.layout, width, height, base, int(aa))
    o.set_ramps(r.ramps)
    o.set_image_atlas(atlas)
    return o.render()


def _assert_same(img, ref, tol, what):
    d = np.abs(img.astype(np.int32) - ref.astype(np.int32))
    assert d.max() <= tol, f"{what}: max diff {d.max()} at {np.argwhere(d > tol)[:4].tolist()}"


def _sprite_scene(images, cols, cell, scale=1.0):
    s = Scene()
    for k, im in enumerate(images):
        x, y = (k % cols) * cell, (k // cols) * cell
        s.draw_image(ImageBrush(im, quality=ImageQuality.Low), Affine.translate(float(x), float(y)) * Affine.scale(scale))
    return s


def test_emu_copy_images_device_batches_match_oracle(emu_engine):
    # strided views, a full-width source and 300 tiny rectangles in ONE batch; the frame that samples them equals the oracle
    # rendered with the atlas put together from host copies at the resolver's placements
    rng = np.random.default_rng(5)
    big = _pixels(rng, 40, 70, opaque=False)
    sources = {}
    images = []
    strided = ImageData.empty(24, 18)
    sources[strided.id] = big[5:23, 11:35]  # a slice: row stride 280 bytes, origin inside the parent
    images.append(strided)
    whole = ImageData.empty(33, 7)
    sources[whole.id] = _pixels(rng, 7, 33)
    images.append(whole)
    tiny_parent = _pixels(rng, 302, 12)
    for k in range(300):
        im = ImageData.empty(3, 1 + k % 3)
        sources[im.id] = tiny_parent[k:k + im.height, 4 * (k % 3):4 * (k % 3) + 3]
        images.append(im)
    scene = _sprite_scene(images, 20, 6, scale=1.0)
    r = vello_amd.Resolver(atlas_sizes=(128, 256)).resolve(scene)
    assert not r.uploads and len(r.device_uploads) == len(images)
    emu_engine.resize_image_atlas(r.atlas_size, r.atlas_size)
    emu_engine.copy_images_device([(x, y, w, h, sources[i], sources[i].strides[0]) for x, y, w, h, i in r.device_uploads])
    for aa, tol in ((AaConfig.Msaa16, 0), (AaConfig.Area, 1)):
        img, bump = emu_engine.render(r.packed, r.layout, 128, 100, WHITE, aa, ramps=r.ramps)
        assert bump["failed"] == 0
        _assert_same(img, _oracle_frame(r, r.atlas_image(sources), 128, 100, aa), tol, f"batch aa={int(aa)}")


def test_emu_copy_images_device_refuses_bad_batches_and_leaves_the_atlas(emu_engine):
    rng = np.random.default_rng(9)
    a, b = ImageData.empty(16, 16), ImageData.empty(8, 12)
    src_a, src_b = _pixels(rng, 16, 16), _pixels(rng, 12, 8)
    scene = _sprite_scene([a, b], 2, 20, scale=2.0)
    r = vello_amd.Resolver(atlas_sizes=(64, 64)).resolve(scene)
    emu_engine.resize_image_atlas(r.atlas_size, r.atlas_size)
    (xa, ya, _, _, _), (xb, yb, _, _, _) = r.device_uploads
    emu_engine.copy_images_device([(xa, ya, 16, 16, src_a, 64), (xb, yb, 8, 12, src_b, 32)])
    ref = _oracle_frame(r, r.atlas_image({a.id: src_a, b.id: src_b}), 80, 48, AaConfig.Msaa8)
    img, _ = emu_engine.render(r.packed, r.layout, 80, 48, WHITE, AaConfig.Msaa8, ramps=r.ramps)
    _assert_same(img, ref, 0, "before")
    junk = np.full((64, 64, 4), 7, dtype=np.uint8)
    bad_batches = [
        [(xa, ya, 16, 16, junk, 256), (60, 0, 8, 8, junk, 256)],   # a valid rectangle, then one past the right edge
        [(0, 57, 4, 8, junk, 256)],                                # past the bottom edge
        [(xa, ya, 16, 16, junk, 256), (0, 0, 4, 4, 0, 16)],        # a null source
        [(0, 0, 4, 4, junk[:, 1:], 255)],                          # a stride that is not a multiple of 4
    ]
    for batch in bad_batches:
        with pytest.raises(VelloHipError, match=r"\(-1\)"):
            emu_engine.copy_images_device(batch)
    lib = emu_engine._lib
    assert lib.vello_hip_copy_images_device(emu_engine._h, None, 2, None) == E_INVALID
    assert b"copies" in lib.vello_hip_last_error(emu_engine._h)
    # empty batches and empty rectangles (null sources allowed there) do nothing
    assert lib.vello_hip_copy_images_device(emu_engine._h, None, 0, None) == 0
    emu_engine.copy_images_device([(0, 0, 0, 5, 0, 0), (3, 3, 5, 0, None, 0)])
    img, _ = emu_engine.render(r.packed, r.layout, 80, 48, WHITE, AaConfig.Msaa8, ramps=r.ramps)
    _assert_same(img, ref, 0, "after the refused batches")


class _Mirror:
    """The renderer's resolver is private: a second Resolver fed the same scenes places the images in the same spots (the
    placement depends on the scene sequence only).  `resident` is what the test expects in the atlas for each override."""

    def __init__(self):
        self.resolver = vello_amd.Resolver()
        self.resident = {}

    def frame(self, scene, width, height, aa):
        r = self.resolver.resolve(scene)
        return _oracle_frame(r, r.atlas_image(self.resident), width, height, aa), r


def test_emu_renderer_override_copies_exactly_when_upstream_would(emu_engine):
    # An override source is copied into the atlas on first use, after mark_override_image_dirty, after override_image replaces
    # it and after the atlas grows -- and at no other time: rewriting the source between renders shows only after those events.
    rng = np.random.default_rng(21)
    renderer = vello_amd.Renderer()
    mirror = _Mirror()
    W = H = 64
    params = RenderParams(Color.from_rgb8(255, 255, 255), W, H, AaConfig.Msaa16)
    src = _pixels(rng, 16, 16)
    im = renderer.register_texture(src)
    assert im.pixels is None and (im.width, im.height) == (16, 16)
    host_im = ImageData(_pixels(rng, 8, 8))
    scene = _sprite_scene([im, host_im], 2, 24, scale=1.5)

    def check(expected, what, s=scene):
        mirror.resident[im.id] = expected.copy()
        ref, r = mirror.frame(s, W, H, AaConfig.Msaa16)
        out = np.zeros((H, W, 4), dtype=np.uint8)
        renderer.render_to_texture(s, out, params)
        _assert_same(out, ref, 0, what)
        return r

    first = src.copy()
    check(first, "first use")
    src[:] = _pixels(rng, 16, 16)  # rewritten in place, not marked: the resident copy stays
    check(first, "unmarked rewrite")
    renderer.mark_override_image_dirty(im)
    second = src.copy()
    check(second, "after mark_override_image_dirty")
    check(second, "clean again")
    other = _pixels(rng, 16, 16)
    assert renderer.override_image(im, other) is src
    check(other, "after override_image replaced the source")
    other[:] = _pixels(rng, 16, 16)
    check(mirror.resident[im.id], "unmarked rewrite of the new source")
    # the atlas grows (a 1016x1016 image does not fit beside it in 1024x1024): every resident is copied again
    huge = ImageData(np.full((1016, 1016, 4), 90, dtype=np.uint8))
    grown = Scene()
    grown.append(scene)
    grown.draw_image(ImageBrush(huge, quality=ImageQuality.Low), Affine.translate(40.0, 40.0) * Affine.scale(0.01))
    r = check(other, "after the atlas grew", grown)
    assert r.atlas_resized and r.atlas_size > 1024


def test_emu_renderer_refuses_a_pixel_less_image_without_override(emu_engine):
    rng = np.random.default_rng(3)
    renderer = vello_amd.Renderer()
    params = RenderParams(Color.from_rgb8(255, 255, 255), 32, 32, AaConfig.Area)
    lonely = ImageData.empty(8, 8)
    scene = _sprite_scene([lonely], 1, 8, scale=2.0)
    out = np.full((32, 32, 4), 0x5A, dtype=np.uint8)
    with pytest.raises(VelloHipError, match=rf"\(-1\).*invalid empty image \(id {lonely.id}\)"):
        renderer.render_to_texture(scene, out, params)
    assert (out == 0x5A).all()
    # bound later, the same image renders (the failed frame left it to be uploaded again)
    src = _pixels(rng, 8, 8)
    assert renderer.override_image(lonely, src) is None
    renderer.render_to_texture(scene, out, params)
    r = vello_amd.Resolver().resolve(scene)
    _assert_same(out, _oracle_frame(r, r.atlas_image({lonely.id: src}), 32, 32, AaConfig.Area), 1, "bound later")
    # and unregistered, it is refused again once it has to be uploaded
    renderer.unregister_texture(lonely)
    out[:] = 0x5A
    with pytest.raises(VelloHipError, match="invalid empty image"):
        renderer.render_to_texture(scene, out, params)
    assert (out == 0x5A).all()
    with pytest.raises(ValueError):
        renderer.override_image(lonely, _pixels(rng, 8, 9))


def test_emu_copy_images_device_several_steps_per_thread(emu_engine):
    # past 2048 x 256 texels a workgroup takes several 256-texel steps (and walks from one rectangle into the next): a
    # 700x790 source at an odd atlas x beside small ones, checked through a frame that samples every part of it
    rng = np.random.default_rng(77)
    big = ImageData.empty(700, 790)
    smalls = [ImageData.empty(5 + k % 4, 3 + k % 5) for k in range(40)]
    sources = {big.id: _pixels(rng, 790, 704)[:, 3:703]}
    for im in smalls:
        sources[im.id] = _pixels(rng, im.height, im.width)
    s = Scene()
    for k, im in enumerate(smalls):
        s.draw_image(ImageBrush(im, quality=ImageQuality.Low), Affine.translate(float(8 * (k % 10)), float(8 * (k // 10))))
    s.draw_image(ImageBrush(big, quality=ImageQuality.Low), Affine.translate(0.0, 40.0) * Affine.scale(0.1))
    r = vello_amd.Resolver().resolve(s)
    emu_engine.resize_image_atlas(r.atlas_size, r.atlas_size)
    emu_engine.copy_images_device([(x, y, w, h, sources[i], sources[i].strides[0]) for x, y, w, h, i in r.device_uploads])
    img, _ = emu_engine.render(r.packed, r.layout, 80, 120, WHITE, AaConfig.Msaa16, ramps=r.ramps)
    _assert_same(img, _oracle_frame(r, r.atlas_image(sources), 80, 120, AaConfig.Msaa16), 0, "several steps")


def test_emu_renderer_override_is_copied_again_after_an_eviction_repack(emu_engine):
    # An eviction repacks the atlas (image_cache.rs:167-182): every survivor moves and is uploaded again -- an override too,
    # so a source rewritten without mark_override_image_dirty shows after the repack (and not before it)
    rng = np.random.default_rng(31)
    renderer = vello_amd.Renderer()
    mirror = _Mirror()
    W = H = 64
    params = RenderParams(Color.from_rgb8(255, 255, 255), W, H, AaConfig.Msaa16)
    src = _pixels(rng, 16, 16)
    im = renderer.register_texture(src)
    wide_a = ImageData(np.full((500, 1000, 4), 60, dtype=np.uint8))
    wide_b = ImageData(np.full((600, 1000, 4), 200, dtype=np.uint8))

    def scene_with(*extra):
        s = _sprite_scene([im], 1, 0, scale=2.0)
        for k, e in enumerate(extra):
            s.draw_image(ImageBrush(e, quality=ImageQuality.Low), Affine.translate(40.0, 10.0 + 20.0 * k) * Affine.scale(0.02))
        return s

    def check(expected, what, s):
        mirror.resident[im.id] = expected.copy()
        ref, r = mirror.frame(s, W, H, AaConfig.Msaa16)
        out = np.zeros((H, W, 4), dtype=np.uint8)
        renderer.render_to_texture(s, out, params)
        _assert_same(out, ref, 0, what)
        return r

    first = src.copy()
    check(first, "with A", scene_with(wide_a))
    src[:] = _pixels(rng, 16, 16)  # rewritten, not marked
    for k in range(2):  # A goes unused for two generations: stale
        r = check(first, f"alone {k}", scene_with())
        assert not r.atlas_resized
    # B does not fit beside A in 1024x1024: A is evicted and the survivors are repacked at the same size
    r = check(src, "after the eviction repack", scene_with(wide_b))
    assert r.evicted == 1 and r.atlas_resized and r.atlas_size == 1024


def test_emu_upload_resolved_copies_pixel_less_images_from_sources(emu_engine):
    rng = np.random.default_rng(12)
    im = ImageData.empty(12, 10)
    src = _pixels(rng, 10, 12)
    scene = _sprite_scene([im, ImageData(_pixels(rng, 6, 6))], 2, 20, scale=1.5)
    r = vello_amd.Resolver().resolve(scene)
    with pytest.raises(VelloHipError, match=f"invalid empty image \\(id {im.id}\\)"):
        emu_engine.upload_resolved(r)
    emu_engine.upload_resolved(r, sources={im.id: src})
    out, _ = emu_engine.render(r.packed, r.layout, 48, 32, WHITE, AaConfig.Msaa8, ramps=r.ramps)
    _assert_same(out, _oracle_frame(r, r.atlas_image({im.id: src}), 48, 32, AaConfig.Msaa8), 0, "upload_resolved")
