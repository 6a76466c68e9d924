"""Image overrides on the MI355X: register_texture / override_image sources copied into the atlas by k_atlas_copy, held to the
CPU oracle rendered with an atlas built from host copies at the resolver's placements."""
import numpy as np
import pytest

import vello_amd
import workloads
from oracle.oracle import Oracle
from vello_amd import (AaConfig, Affine, Color, Extend, ImageAlphaType, ImageBrush, ImageData, ImageFormat, ImageQuality, Rect,
                       RenderParams, Scene, VelloHipError)
from vello_amd.scene import Fill

WHITE = 0xFFFFFFFF


def _oracle_frame(r, atlas, width, height, aa, base=WHITE):
    o = Oracle()
    o.set_scene(r.packed, r.layout, width, height, base, int(aa))
    o.set_ramps(r.ramps)
    o.set_image_atlas(atlas)
    return o.render()


def _assert_same(img, ref, tol, what):
    d = np.abs(img.astype(np.int32) - ref.astype(np.int32))
    assert d.max() <= tol, f"{what}: max diff {d.max()} at {np.argwhere(d > tol)[:4].tolist()}"


def _tensor(rng, h, w, opaque=False, premultiplied=False):
    import torch

    px = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    if opaque:
        px[:, :, 3] = 255
    if premultiplied:
        px[:, :, :3] = (px[:, :, :3].astype(np.uint32) * px[:, :, 3:4] // 255).astype(np.uint8)
    return torch.from_numpy(px).to("cuda:0")


@pytest.fixture()
def torch_gpu(gpu_engine):
    import torch

    return torch


@pytest.mark.gpu
def test_gpu_registered_textures_match_oracle(torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(11)
    renderer = vello_amd.Renderer()
    parent = _tensor(rng, 90, 120)
    strided = parent[7:67, 13:93]  # a slice of a larger tensor: row stride 480 bytes, origin inside it
    plain = renderer.register_texture(_tensor(rng, 48, 40, opaque=True))
    sliced = renderer.register_texture(strided)
    bgra = ImageData.empty(33, 21, ImageFormat.Bgra8, ImageAlphaType.Alpha)
    premul = ImageData.empty(50, 30, ImageFormat.Rgba8, ImageAlphaType.AlphaPremultiplied)
    bgra_src, premul_src = _tensor(rng, 21, 33), _tensor(rng, 30, 50, premultiplied=True)
    renderer.override_image(bgra, bgra_src)
    renderer.override_image(premul, premul_src)
    sources = {plain.id: renderer._overrides[plain.id], sliced.id: strided, bgra.id: bgra_src, premul.id: premul_src}
    torch.cuda.synchronize()
    s = Scene()
    extends = [Extend.Pad, Extend.Repeat, Extend.Reflect]
    xforms = [Affine.translate(20.0, 30.0) * Affine.rotate(0.4) * Affine.scale(1.7),
              Affine.translate(150.0, 20.0) * Affine.skew(0.3, -0.2) * Affine.scale(1.3),
              Affine.translate(40.0, 150.0) * Affine.scale_non_uniform(2.2, 0.8),
              Affine.translate(170.0, 170.0) * Affine.rotate(-0.9) * Affine.scale(0.7)]
    for k, im in enumerate((plain, sliced, bgra, premul)):
        for q, quality in enumerate((ImageQuality.Low, ImageQuality.Medium, ImageQuality.High)):
            brush = ImageBrush(im, x_extend=extends[(k + q) % 3], y_extend=extends[(k + 2 * q + 1) % 3], quality=quality)
            xf = Affine.translate(0.0, 80.0 * q) * xforms[k]
            s.fill(Fill.NonZero, xf, brush, Affine.translate(-5.0, -4.0), Rect(0.0, 0.0, 60.0, 45.0))
    r = vello_amd.Resolver().resolve(s)
    atlas = r.atlas_image({i: t.cpu().numpy() for i, t in sources.items()})
    for aa, tol in ((AaConfig.Msaa8, 0), (AaConfig.Msaa16, 0), (AaConfig.Area, 1)):
        out = torch.zeros((256, 256, 4), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        renderer.render_to_texture(s, out, RenderParams(Color.from_rgb8(255, 255, 255), 256, 256, aa))
        torch.cuda.synchronize()
        _assert_same(out.cpu().numpy(), _oracle_frame(r, atlas, 256, 256, aa), tol, f"aa={int(aa)}")


@pytest.mark.gpu
def test_gpu_render_to_texture_with_frames_in_flight(torch_gpu):
    # Frame A renders into a device buffer; that buffer is copied into the atlas at once and frame B, which samples it, is
    # enqueued right behind -- no host sync between steps, four frames in flight, every lane producer and consumer.
    torch = torch_gpu
    eng = vello_amd.Engine(device=0)
    eng.set_frames_in_flight(4)
    A = 64
    target = ImageData.empty(A, A)
    sb = Scene()
    sb.fill(Fill.NonZero, Affine.translate(8.0, 8.0) * Affine.rotate(0.3) * Affine.scale(1.6), ImageBrush(target, quality=ImageQuality.Medium),
            None, Rect(0.0, 0.0, float(A), float(A)))
    rb = vello_amd.Resolver().resolve(sb)
    (x, y, _, _, _), = rb.device_uploads
    eng.resize_image_atlas(rb.atlas_size, rb.atlas_size)
    steps = 10
    scenes_a = [workloads.random_test_scene(100 + i, n_paths=60, size=float(A), strokes=True).resolve() for i in range(steps)]
    bufs_a = [torch.zeros((A, A, 4), dtype=torch.uint8, device="cuda:0") for _ in range(steps)]
    bufs_b = [torch.zeros((160, 160, 4), dtype=torch.uint8, device="cuda:0") for _ in range(steps)]
    torch.cuda.synchronize()
    spare = torch.zeros((A, A, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for i in range(steps):
        pa, la = scenes_a[i]
        if i == steps // 2:  # one frame more shifts the lanes: those that produced so far consume from here on, and back
            eng.render_frame(pa, la, A, A, 0xFF102030, AaConfig.Msaa16, out=spare)
        eng.render_frame(pa, la, A, A, 0xFF102030, AaConfig.Msaa16, out=bufs_a[i])
        eng.copy_images_device([(x, y, A, A, bufs_a[i], A * 4)])
        eng.render_frame(rb.packed, rb.layout, 160, 160, WHITE, AaConfig.Msaa16, out=bufs_b[i], ramps=rb.ramps)
    assert eng.sync() == 0
    for i in range(steps):
        pa, la = scenes_a[i]
        o = Oracle()
        o.set_scene(pa, la, A, A, 0xFF102030, int(AaConfig.Msaa16))
        ref_a = o.render()
        _assert_same(bufs_a[i].cpu().numpy(), ref_a, 0, f"A{i}")
        _assert_same(bufs_b[i].cpu().numpy(), _oracle_frame(rb, rb.atlas_image({target.id: ref_a}), 160, 160, AaConfig.Msaa16), 0, f"B{i}")


@pytest.mark.gpu
def test_gpu_override_waits_for_the_source_stream(torch_gpu):
    # a torch kernel on a side stream rewrites the texture; mark dirty and render with that stream current, no synchronize
    torch = torch_gpu
    rng = np.random.default_rng(4)
    renderer = vello_amd.Renderer()
    tex = _tensor(rng, 64, 64, opaque=True)
    im = renderer.register_texture(tex)
    s = Scene()
    s.draw_image(ImageBrush(im, quality=ImageQuality.Low), Affine.translate(16.0, 16.0) * Affine.scale(1.5))
    params = RenderParams(Color.from_rgb8(255, 255, 255), 128, 128, AaConfig.Msaa16)
    torch.cuda.synchronize()
    out = np.zeros((128, 128, 4), dtype=np.uint8)
    renderer.render_to_texture(s, out, params)
    side = torch.cuda.Stream()
    big = torch.randn((2048, 2048), device="cuda:0")
    new = torch.from_numpy(rng.integers(0, 256, size=(64, 64, 4), dtype=np.uint8)).to("cuda:0")
    new[:, :, 3] = 255
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):  # keep the side stream busy, so a copy that did not wait would read the old texels
            big = big @ big * 1e-3
        tex.copy_(new)
        renderer.mark_override_image_dirty(im)
        renderer.render_to_texture(s, out, params)
    r = vello_amd.Resolver().resolve(s)
    _assert_same(out, _oracle_frame(r, r.atlas_image({im.id: new.cpu().numpy()}), 128, 128, AaConfig.Msaa16), 0, "after the rewrite")
    # the same on torch's default stream (the C ABI cannot name it: the binding relays it through a pool stream)
    torch.cuda.synchronize()
    newer = torch.from_numpy(rng.integers(0, 256, size=(64, 64, 4), dtype=np.uint8)).to("cuda:0")
    newer[:, :, 3] = 255
    torch.cuda.synchronize()
    assert torch.cuda.current_stream().cuda_stream == 0
    for _ in range(8):
        big = big @ big * 1e-3
    tex.copy_(newer)
    renderer.mark_override_image_dirty(im)
    renderer.render_to_texture(s, out, params)
    r = vello_amd.Resolver().resolve(s)
    _assert_same(out, _oracle_frame(r, r.atlas_image({im.id: newer.cpu().numpy()}), 128, 128, AaConfig.Msaa16), 0, "default stream")
    # and the source may be overwritten on the default stream right after the copy was enqueued: the copy read it first
    eng = vello_amd.Engine(device=0)
    eng.resize_image_atlas(64, 64)
    eng.copy_images_device([(0, 0, 64, 64, tex, 256)], stream=torch.cuda.current_stream())
    tex.zero_()
    ri = vello_amd.Resolver(atlas_sizes=(64, 64)).resolve(s)
    img, _ = eng.render(ri.packed, ri.layout, 128, 128, WHITE, AaConfig.Msaa16, ramps=ri.ramps)
    _assert_same(img, _oracle_frame(ri, ri.atlas_image({im.id: newer.cpu().numpy()}), 128, 128, AaConfig.Msaa16), 0, "read before overwritten")


@pytest.mark.gpu
def test_gpu_removed_override_is_refused_and_target_untouched(torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(8)
    renderer = vello_amd.Renderer()
    im = renderer.register_texture(_tensor(rng, 16, 16, opaque=True))
    s = Scene()
    s.draw_image(ImageBrush(im), Affine.translate(4.0, 4.0))
    params = RenderParams(Color.from_rgb8(255, 255, 255), 32, 32, AaConfig.Area)
    out = torch.zeros((32, 32, 4), dtype=torch.uint8, device="cuda:0")
    renderer.render_to_texture(s, out, params)
    renderer.override_image(im, None)
    renderer.mark_override_image_dirty(im)
    out.fill_(0x5A)
    torch.cuda.synchronize()
    with pytest.raises(VelloHipError, match=r"\(-1\).*invalid empty image"):
        renderer.render_to_texture(s, out, params)
    torch.cuda.synchronize()
    assert bool((out == 0x5A).all())
    # a host source is not device memory: refused by the engine, nothing enqueued
    with pytest.raises(VelloHipError, match="not device memory"):
        eng = vello_amd.Engine(device=0)
        eng.resize_image_atlas(64, 64)
        eng.copy_images_device([(0, 0, 4, 4, np.zeros((4, 4, 4), dtype=np.uint8), 16)])


@pytest.mark.gpu
def test_gpu_thousand_registered_images_and_atlas_growth(torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(1000)
    renderer = vello_amd.Renderer()
    pool = torch.from_numpy(rng.integers(0, 256, size=(1000, 16, 16, 4), dtype=np.uint8)).to("cuda:0")
    images = [renderer.register_texture(pool[k]) for k in range(1000)]
    wide = renderer.register_texture(_tensor(rng, 1000, 1016, opaque=True))  # does not fit beside them: the atlas grows
    torch.cuda.synchronize()
    s = Scene()
    for k, im in enumerate(images):
        s.draw_image(ImageBrush(im, quality=ImageQuality.Low), Affine.translate(float(16 * (k % 32)), float(16 * (k // 32))))
    s.draw_image(ImageBrush(wide, quality=ImageQuality.Medium), Affine.translate(300.0, 500.0) * Affine.scale(0.2))
    mirror = vello_amd.Resolver()
    r = mirror.resolve(s)
    assert r.atlas_size > 1024 and len(r.device_uploads) == 1001
    sources = {im.id: pool[k].cpu().numpy() for k, im in enumerate(images)}
    sources[wide.id] = renderer._overrides[wide.id].cpu().numpy()
    out = torch.zeros((720, 512, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    renderer.render_to_texture(s, out, RenderParams(Color.from_rgb8(255, 255, 255), 512, 720, AaConfig.Msaa16))
    torch.cuda.synchronize()
    _assert_same(out.cpu().numpy(), _oracle_frame(r, r.atlas_image(sources), 512, 720, AaConfig.Msaa16), 0, "1000 images")


@pytest.mark.gpu
def test_gpu_large_and_small_sources_in_one_batch(torch_gpu):
    # 6 M texels (a workgroup takes 12 steps: two groups of loads, the second partial) beside 60 small rectangles, all in ONE
    # k_atlas_copy launch, sampled through a frame that reads every part of the large one
    torch = torch_gpu
    rng = np.random.default_rng(6)
    big = ImageData.empty(3001, 2003)
    smalls = [ImageData.empty(5 + k % 4, 3 + k % 5) for k in range(60)]
    parent = _tensor(rng, 2003, 3010)
    sources = {big.id: parent[:, 7:3008]}
    for im in smalls:
        sources[im.id] = _tensor(rng, im.height, im.width)
    s = Scene()
    for k, im in enumerate(smalls):
        s.draw_image(ImageBrush(im, quality=ImageQuality.Low), Affine.translate(float(10 * (k % 20)), float(10 * (k // 20))))
    s.draw_image(ImageBrush(big, quality=ImageQuality.Low), Affine.translate(0.0, 40.0) * Affine.scale(0.13))
    r = vello_amd.Resolver().resolve(s)
    eng = vello_amd.Engine(device=0)
    eng.resize_image_atlas(r.atlas_size, r.atlas_size)
    torch.cuda.synchronize()
    eng.copy_images_device([(x, y, w, h, sources[i], sources[i].stride(0)) for x, y, w, h, i in r.device_uploads],
                           stream=torch.cuda.current_stream())
    img, bump = eng.render(r.packed, r.layout, 400, 310, WHITE, AaConfig.Msaa16, ramps=r.ramps)
    assert bump["failed"] == 0
    atlas = r.atlas_image({i: t.cpu().numpy() for i, t in sources.items()})
    _assert_same(img, _oracle_frame(r, atlas, 400, 310, AaConfig.Msaa16), 0, "large + small")
