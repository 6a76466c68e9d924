"""Where a frame lands: the target's address, its row stride, and the atlas's shape, against the CPU oracle.  Every other suite
renders into a packed target at an allocation's start and samples a square atlas; here a frame goes into a VIEW of a surface of
seeded random bytes, and the expectation is built from the oracle alone: a copy of the untouched surface with oracle.render()
pasted into the first width * 4 bytes of each of the view's rows.  In the MSAA modes the whole surface must equal it byte for
byte; with area AA the frame's own bytes within 1 LSB (segment order changes f32 summation: the suite's bar) and every other byte
exactly.  So a store past `width`, a row computed from the wrong stride, or a 16-byte store at an address that only looked aligned
shows as a canary byte that changed.

`mem` is where "device memory" lives: HostMemory for the SIMT-emulated build (numpy arrays stand for device memory there),
TorchMemory for the MI355X."""
import numpy as np

from oracle.oracle import Oracle
from tests import instance_parity as ip
from tests import parity
from tests import view_parity as vp

BLACK = 0xFF000000
BASE_COLORS = (0xFF000000, 0x80FF8040, 0x00000000)
LEAD = 64  # canary bytes in front of a target (a multiple of 16: the target's own offset decides its alignment)


# ---------------------------------------------------------------------------------------------------------------
# Memory
# ---------------------------------------------------------------------------------------------------------------
def _canary(nbytes, seed):
    return np.random.default_rng(0xCA7A0000 + seed).integers(0, 256, nbytes, dtype=np.uint8)


class HostMemory:
    """Flat uint8 numpy buffers whose first byte is 64-byte aligned (numpy itself promises less than the 16 the store paths of
    k_fine tell apart)."""

    def surface(self, nbytes, seed):
        raw = np.empty(nbytes + 64, dtype=np.uint8)
        buf = raw[(-raw.ctypes.data) % 64:][:nbytes]
        assert buf.ctypes.data % 64 == 0
        buf[:] = _canary(nbytes, seed)
        return buf

    def address(self, buf):
        return buf.ctypes.data

    def view(self, buf, offset, h, w, stride):
        assert offset + (h - 1) * stride + w * 4 <= buf.size
        return np.lib.stride_tricks.as_strided(buf[offset:], shape=(h, w, 4), strides=(stride, 4, 1))

    def flat(self, buf, offset):
        return buf[offset:]

    def numpy(self, buf):
        return np.array(buf, copy=True)


class TorchMemory:
    """Flat torch.uint8 tensors on the GPU.  The canary is written on torch's stream and torch.cuda.synchronize() runs before the
    engine is asked to render (the engine's stream is its own)."""

    def surface(self, nbytes, seed):
        import torch

        buf = torch.from_numpy(_canary(nbytes, seed)).to("cuda")
        torch.cuda.synchronize()
        assert buf.data_ptr() % 64 == 0
        return buf

    def address(self, buf):
        return buf.data_ptr()

    def view(self, buf, offset, h, w, stride):
        assert offset + (h - 1) * stride + w * 4 <= buf.numel()
        return buf.as_strided((h, w, 4), (stride, 4, 1), offset)

    def flat(self, buf, offset):
        return buf[offset:]

    def numpy(self, buf):
        return buf.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------
# Expectation and comparison
# ---------------------------------------------------------------------------------------------------------------
def check_surface(name, got, canary, frames):
    """`got` (the surface after the frames) against `canary` (before) with `frames` = [(offset, stride, oracle image, tol)] pasted."""
    assert got.shape == canary.shape
    want = canary.copy()
    inside = np.zeros(canary.size, dtype=bool)
    for offset, stride, img, _ in frames:
        h, w = img.shape[:2]
        for y in range(h):
            a = offset + y * stride
            assert not inside[a: a + w * 4].any(), f"{name}: the case's own frames overlap"
            want[a: a + w * 4] = img[y].reshape(-1)
            inside[a: a + w * 4] = True
    changed = np.nonzero(~inside & (got != canary))[0]
    assert changed.size == 0, f"{name}: {changed.size} bytes outside the frame were written, first at surface offset {changed[0]}"
    for k, (offset, stride, img, tol) in enumerate(frames):
        h, w = img.shape[:2]
        rows = np.stack([got[offset + y * stride: offset + y * stride + w * 4] for y in range(h)]).reshape(h, w, 4)
        diff = np.abs(rows.astype(np.int32) - img.astype(np.int32))
        print(f"{name}: frame {k}: max difference {diff.max()} (tolerance {tol})")
        assert diff.max() <= tol, f"{name}: frame {k} differs from the oracle: max {diff.max()}, {(diff > tol).sum()} values over {tol}"
    if all(f[3] == 0 for f in frames):
        assert np.array_equal(got, want), name


def _tol(aa):
    return 1 if int(aa) == 0 else 0


def oracle_image(packed, layout, w, h, base, aa, resolved=None):
    o = Oracle(capacity_scale=4, auto_grow=True)
    o.set_scene(packed, layout, w, h, base, int(aa))
    if resolved is not None:
        o.set_ramps(resolved.ramps)
        o.set_image_atlas(resolved.atlas_image())
    return o.render().copy()


# ---------------------------------------------------------------------------------------------------------------
# a. The placement matrix on render_resident
# ---------------------------------------------------------------------------------------------------------------
TARGETS = ((1, 1), (3, 5), (4, 4), (5, 17), (16, 16), (17, 33), (20, 20), (97, 53), (128, 128))
SUB_ORIGINS = ((0, 1), (2, 3), (1, 2))  # (y0, x0) in a surface w + 7 pixels wide


def placements(w, h):
    """[(name, surface bytes, offset of the target's first byte, stride of the rows, stride handed to the engine or None: taken
    from the view)].  Stride 0 is the header's shorthand for width * 4."""
    row = w * 4
    out = []
    for name, stride, arg in (("stride0", row, 0), ("packed", row, None), ("plus4", row + 4, None), ("plus12", row + 12, None),
                              ("pad256", (row + 255) // 256 * 256, None)):
        out.append((name, LEAD + (h - 1) * stride + row + LEAD, LEAD, stride, arg))
    for y0, x0 in SUB_ORIGINS:
        stride = (w + 7) * 4
        out.append((f"sub_{y0}_{x0}", LEAD + (h + y0 + 1) * stride + LEAD, LEAD + y0 * stride + x0 * 4, stride, None))
    return out


def matrix_cases():
    """[(target index, w, h, placement index, placement, aa, base colour)]: the AA mode and the base colour cycle over the cases, out
    of step with each other, so that every target meets every mode and every colour."""
    from vello_amd import AaConfig

    out = []
    for ti, (w, h) in enumerate(TARGETS):
        for pi, p in enumerate(placements(w, h)):
            aa = (AaConfig.Area, AaConfig.Msaa8, AaConfig.Msaa16)[(ti + pi) % 3]
            out.append((ti, w, h, pi, p, aa, BASE_COLORS[(ti + pi // 3) % 3]))
    return out


def store_paths_reached():
    """{(row address % 16, whether the row's last thread holds four whole pixels)} over every row of every case of the matrix, for a
    surface whose first byte is 16-aligned (both memories assert 64).  k_fine's thread (row y, pixels px0 .. px0 + 3) stores at
    base + y * stride + px0 * 16: the same residue as its row, and it takes the 16-byte store iff that is 0 and px0 + 4 <= width."""
    reached = set()
    for _, w, h, _, (_, _, offset, stride, _), _, _ in matrix_cases():
        px0 = (w - 1) // 4 * 4
        for y in range(h):
            reached.add(((offset + y * stride) % 16, px0 + 4 <= w))
    return reached


def check_matrix_inputs():
    """A condition on the cases, not on the engine: a later edit of the matrix cannot quietly drop a store path."""
    cases = matrix_cases()
    assert len(cases) == len(TARGETS) * 8 and {(c[1], c[2]) for c in cases} == set(TARGETS)
    want = {(r, full) for r in (0, 4, 8, 12) for full in (True, False)}
    assert store_paths_reached() == want, sorted(want - store_paths_reached())
    assert {int(c[5]) for c in cases} == {0, 1, 2} and {c[6] for c in cases} == set(BASE_COLORS)


def check_matrix_target(engine, mem, name, ti):
    """Every placement of target `ti`: workloads.fuzz.fuzz_scene(ti) resident once, the oracle asked once per (aa, base colour)."""
    import vello_amd
    from workloads.fuzz import fuzz_scene

    w, h = TARGETS[ti]
    r = vello_amd.Resolver().resolve(fuzz_scene(ti, size=max(w, h, 8)))
    engine.upload_resolved(r)
    refs = {}
    n = 0
    for cti, _, _, pi, (pname, nbytes, offset, stride, arg), aa, base in matrix_cases():
        if cti != ti:
            continue
        if (int(aa), base) not in refs:
            refs[int(aa), base] = oracle_image(r.packed, r.layout, w, h, base, aa, r)
        buf = mem.surface(nbytes, 1000 * ti + pi)
        canary = mem.numpy(buf)
        assert mem.address(buf) % 16 == 0
        if arg is not None:
            engine.render_resident(w, h, base, aa, out=mem.flat(buf, offset), out_stride=arg)
        else:
            engine.render_resident(w, h, base, aa, out=mem.view(buf, offset, h, w, stride))
        assert engine.sync() == 0
        check_surface(f"{name}_{w}x{h}_{pname}_aa{int(aa)}", mem.numpy(buf), canary, [(offset, stride, refs[int(aa), base], _tol(aa))])
        n += 1
    assert n == 8


# ---------------------------------------------------------------------------------------------------------------
# b. Every entry point and every k_fine instantiation, strided
# ---------------------------------------------------------------------------------------------------------------
def _plain_scene(seed=2, n_paths=60, size=64.0):
    import workloads

    return workloads.random_test_scene(seed, n_paths=n_paths, size=size, strokes=True, clips=True)


def _strided(mem, w, h, stride, seed, lead=LEAD):
    buf = mem.surface(lead + (h - 1) * stride + w * 4 + LEAD, seed)
    return buf, mem.numpy(buf)


def check_render_host(engine, name):
    """vello_hip_render to a HOST target at an odd stride (hipMemcpy2D with the caller's pitch) and an odd address."""
    from vello_amd import AaConfig

    w, h, aa = 37, 29, AaConfig.Msaa16
    packed, layout = _plain_scene().resolve()
    host = HostMemory()
    stride, lead = w * 4 + 3, LEAD + 1
    buf, canary = _strided(host, w, h, stride, 11, lead)
    out, bump = engine.render(packed, layout, w, h, BLACK, aa, out=host.flat(buf, lead), out_stride=stride)
    assert bump["failed"] == 0
    check_surface(name, host.numpy(buf), canary, [(lead, stride, oracle_image(packed, layout, w, h, BLACK, aa), 0)])


def check_render_device(engine, mem, name):
    """vello_hip_render with out_is_device: fine writes the caller's memory directly."""
    from vello_amd import AaConfig

    w, h, aa = 37, 29, AaConfig.Area
    packed, layout = _plain_scene().resolve()
    stride = w * 4 + 4
    buf, canary = _strided(mem, w, h, stride, 12)
    _, bump = engine.render(packed, layout, w, h, BASE_COLORS[1], aa, out=mem.view(buf, LEAD, h, w, stride), out_is_device=True)
    assert bump["failed"] == 0
    check_surface(name, mem.numpy(buf), canary, [(LEAD, stride, oracle_image(packed, layout, w, h, BASE_COLORS[1], aa), _tol(aa))])


def check_render_frame(engine, mem, name):
    from vello_amd import AaConfig

    w, h, aa = 37, 29, AaConfig.Msaa8
    packed, layout = _plain_scene(seed=3).resolve()
    stride = w * 4 + 12
    buf, canary = _strided(mem, w, h, stride, 13, LEAD + 8)
    engine.render_frame(packed, layout, w, h, BLACK, aa, out=mem.view(buf, LEAD + 8, h, w, stride))
    assert engine.sync() == 0
    check_surface(name, mem.numpy(buf), canary, [(LEAD + 8, stride, oracle_image(packed, layout, w, h, BLACK, aa), 0)])


def instance_library():
    import vello_amd

    frs = ip.brush_fragments()
    return vello_amd.FragmentLibrary([frs["solid"], frs["linear"], frs["clip"], ip.polygon(6), frs["blend"]])


def check_render_instances(engine, mem, name):
    from vello_amd import AaConfig

    w, h, aa = 61, 45, AaConfig.Msaa16
    lib = instance_library()
    lib.upload(engine)
    instances = ip.scatter(np.random.default_rng(21), 9, 5, w, h, scale=(0.8, 2.5))
    stride = (w + 7) * 4
    buf, canary = _strided(mem, w, h, stride, 14, LEAD + 12)
    engine.render_instances(instances, w, h, BLACK, aa, out=mem.view(buf, LEAD + 12, h, w, stride))
    assert engine.sync() == 0
    check_surface(name, mem.numpy(buf), canary, [(LEAD + 12, stride, ip._want(lib, instances, w, h, BLACK, aa), 0)])


def check_renderer(mem, name, device):
    """Renderer.render_to_texture into a strided view: a host array (hipMemcpy2D), or device memory (`device`: the GPU build only --
    the public layer takes a numpy array for host memory)."""
    import vello_amd
    from vello_amd import AaConfig, Color, RenderParams

    w, h, aa = 37, 29, AaConfig.Msaa16
    scene = _plain_scene(seed=4)
    packed, layout = scene.resolve()
    m = mem if device else HostMemory()
    stride = w * 4 + 20
    buf, canary = _strided(m, w, h, stride, 15, LEAD + 4)
    vello_amd.Renderer().render_to_texture(scene, m.view(buf, LEAD + 4, h, w, stride), RenderParams(Color.from_rgb8(0, 0, 0), w, h, aa))
    check_surface(name, m.numpy(buf), canary, [(LEAD + 4, stride, oracle_image(packed, layout, w, h, BLACK, aa), 0)])


def check_brushes(engine, mem, name, aa):
    """workloads.brushes_scene() at 256 x 256: k_fine's BRUSHES instantiation of this AA mode does the stores."""
    import vello_amd
    import workloads

    w = h = 256
    r = vello_amd.Resolver().resolve(workloads.brushes_scene())
    engine.upload_resolved(r)
    stride = w * 4 + 4
    buf, canary = _strided(mem, w, h, stride, 16 + int(aa))
    engine.render_resident(w, h, BLACK, aa, out=mem.view(buf, LEAD, h, w, stride))
    assert engine.sync() == 0
    check_surface(name, mem.numpy(buf), canary, [(LEAD, stride, oracle_image(r.packed, r.layout, w, h, BLACK, aa, r), _tol(aa))])


def check_fine_slices(engine, mem, name):
    """Every tile's list cut into slices (VELLO_HIP_DEBUG_FINE_SLICES): the wave that composites a sliced tile does the stores."""
    import workloads
    from vello_amd import AaConfig

    w = h = 128
    aa = AaConfig.Msaa16
    packed, layout = workloads.random_test_scene(2, n_paths=300, size=128.0, strokes=True, clips=True).resolve()
    stride = w * 4 + 12
    buf, canary = _strided(mem, w, h, stride, 20, LEAD + 4)
    try:
        engine.set_debug_flags(fine_slices=True)
        engine.upload_scene(packed, layout)
        engine.render_resident(w, h, BLACK, aa, out=mem.view(buf, LEAD + 4, h, w, stride))
        assert engine.sync() == 0
        assert engine.fine_slice_stats()[0] > 0, f"{name}: no tile was sliced: the case proves nothing"
    finally:
        engine.set_debug_flags()
    check_surface(name, mem.numpy(buf), canary, [(LEAD + 4, stride, oracle_image(packed, layout, w, h, BLACK, aa), 0)])


# ---------------------------------------------------------------------------------------------------------------
# c. Contact sheet with frames in flight
# ---------------------------------------------------------------------------------------------------------------
def check_contact_sheet(engine, mem, name):
    """Four 96 x 80 frames of ONE resident non-brush scene -- four views, four base colours, MSAA8 and MSAA16 -- into the quadrants
    of one (2 * 96 + 5) x (2 * 80 + 3) surface, four frames in flight, three rounds without a wait: with several frames in flight
    non-brush scenes take k_fine's frames-in-flight instantiation.  Quadrant k is written by the k-th frame of each round, i.e. by
    the same lane of the rotation every time, so its last writer is round 2's."""
    import workloads
    from vello_amd import AaConfig

    w, h = 96, 80
    sw, sh = 2 * w + 5, 2 * h + 3
    stride = sw * 4
    packed, layout = workloads.random_test_scene(5, n_paths=50, size=128.0, strokes=True, clips=True).resolve()
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    named = dict(vp.views(w, h))
    views = [vp.IDENTITY, named["zoom_in"], named["rot_shear"], named["mirror"]]
    bases = [0xFF000000, 0x80FF8040, 0x00000000, 0xFF203040]
    aas = [AaConfig.Msaa16, AaConfig.Msaa8, AaConfig.Msaa8, AaConfig.Msaa16]
    origins = [(0, 0), (0, w + 5), (h + 3, 0), (h + 3, w + 5)]
    offsets = [LEAD + y0 * stride + x0 * 4 for y0, x0 in origins]
    want = {}
    for k in range(4):
        v = views[(k + 2) % 4]  # (round 2)
        want[k] = oracle_image(vp.compose(packed, layout, v), layout, w, h, bases[k], aas[k])
    assert len({x.tobytes() for x in want.values()}) == 4
    buf = mem.surface(LEAD + sh * stride + LEAD, 30)
    canary = mem.numpy(buf)
    try:
        engine.set_frames_in_flight(4)
        engine.upload_scene(packed, layout)
        for rnd in range(3):
            for k in range(4):
                engine.set_view_transform(views[(k + rnd) % 4])
                engine.render_resident(w, h, bases[k], aas[k], out=mem.view(buf, offsets[k], h, w, stride))
        assert engine.sync() == 0
        assert np.array_equal(engine.read_buffer("scene", np.uint8, packed.nbytes), packed), f"{name}: the resident scene was modified"
    finally:
        engine.set_view_transform(None)
        engine.set_frames_in_flight(1)
    check_surface(name, mem.numpy(buf), canary, [(offsets[k], stride, want[k], 0) for k in range(4)])


# ---------------------------------------------------------------------------------------------------------------
# d. Refusals
# ---------------------------------------------------------------------------------------------------------------
def check_refusals(engine, mem, name):
    """Targets that break the contract of include/vello_hip.h are refused with VELLO_HIP_E_INVALID before anything is uploaded or
    enqueued.  None of these inputs reaches a kernel: that is the point of the check."""
    import vello_amd
    from vello_amd import AaConfig

    w, h, aa = 40, 24, AaConfig.Msaa16
    row = w * 4
    lib = instance_library()
    lib.upload(engine)
    resident = np.ascontiguousarray(lib.packed, dtype=np.uint8)
    instances = ip.scatter(np.random.default_rng(5), 6, 5, w, h, scale=(0.8, 2.0))
    other, other_layout = _plain_scene(seed=6).resolve()  # (what render / render_frame would upload: not the resident scene)
    other = np.ascontiguousarray(other, dtype=np.uint8)
    assert other.nbytes != resident.nbytes or not np.array_equal(other, resident)
    want = oracle_image(lib.packed, lib.layout, w, h, BLACK, aa, lib.resolved)

    # a good frame first: the lanes have rendered, the buffers exist
    stride = row + 4
    buf, canary = _strided(mem, w, h, stride, 40)
    engine.render_resident(w, h, BLACK, aa, out=mem.view(buf, LEAD, h, w, stride))
    assert engine.sync() == 0
    check_surface(f"{name}_before", mem.numpy(buf), canary, [(LEAD, stride, want, 0)])
    allocations = engine.scene_allocations()

    buf = mem.surface(LEAD + h * (row + 16) + LEAD, 41)
    canary = mem.numpy(buf)
    entry_points = {
        "render_resident": lambda out, s: engine.render_resident(w, h, BLACK, aa, out=out, out_stride=s),
        "render_frame": lambda out, s: engine.render_frame(other, other_layout, w, h, BLACK, aa, out=out, out_stride=s),
        "render_instances": lambda out, s: engine.render_instances(instances, w, h, BLACK, aa, out=out, out_stride=s),
        "render": lambda out, s: engine.render(other, other_layout, w, h, BLACK, aa, out=out, out_stride=s, out_is_device=True),
    }
    bad = (("stride_below_row", LEAD, row - 4), ("stride_not_multiple_of_4", LEAD, row + 2), ("address_plus_2", LEAD + 2, row + 4),
           ("stride_2_to_32", LEAD, 1 << 32))

    def after(what):
        assert np.array_equal(mem.numpy(buf), canary), f"{what}: the refused target was written"
        assert engine.sync() == 0, what
        assert np.array_equal(engine.read_buffer("scene", np.uint8, resident.nbytes), resident), f"{what}: the resident scene changed"
        assert engine.scene_allocations() == allocations, f"{what}: a refused frame allocated a scene buffer"

    for ename, call in entry_points.items():
        for bname, offset, s in bad:
            what = f"{name}_{ename}_{bname}"
            with np.testing.assert_raises(vello_amd.VelloHipError):
                call(mem.flat(buf, offset), s)
            after(what)
    # the host target of the blocking entry point: any address, but rows may not overlap
    host = HostMemory()
    hbuf = host.surface(LEAD + h * row + LEAD, 42)
    hcanary = host.numpy(hbuf)
    with np.testing.assert_raises(vello_amd.VelloHipError):
        engine.render(other, other_layout, w, h, BLACK, aa, out=host.flat(hbuf, LEAD), out_stride=row - 1)
    assert np.array_equal(hbuf, hcanary), f"{name}: the refused host target was written"
    after(f"{name}_render_host_stride_below_row")
    # the next valid strided frame is the oracle's, into the surface the refusals left alone
    stride = row + 12
    engine.render_resident(w, h, BLACK, aa, out=mem.view(buf, LEAD + 4, h, w, stride))
    assert engine.sync() == 0
    check_surface(f"{name}_after", mem.numpy(buf), canary, [(LEAD + 4, stride, want, 0)])
    engine.render_instances(instances, w, h, BLACK, aa, out=mem.view(buf, LEAD + 4, h, w, stride))
    assert engine.sync() == 0
    check_surface(f"{name}_after_instances", mem.numpy(buf), canary, [(LEAD + 4, stride, ip._want(lib, instances, w, h, BLACK, aa), 0)])


# ---------------------------------------------------------------------------------------------------------------
# e. Non-square atlas
# ---------------------------------------------------------------------------------------------------------------
# (atlas width, atlas height, [(image width, image height, x, y)]): per atlas one image flush with the right edge, one flush with
# the bottom edge, and one at x >= H (the wide atlases), respectively y >= W (the tall one) -- where exchanged extents would call
# a texel out of range, or address it with the wrong pitch
ATLASES = ((200, 24, ((24, 16, 176, 0), (13, 9, 3, 15), (32, 20, 60, 2))),
           (24, 200, ((24, 16, 0, 5), (13, 9, 4, 191), (20, 32, 2, 100))),
           (72, 40, ((24, 16, 48, 0), (13, 9, 2, 31), (20, 20, 44, 18))))


class _Atlas:
    """The late-bound resources parity.compare_frame hands the oracle.  atlas_size 0: the engine's atlas is already filled, and
    compare_frame must not resize -- and so clear -- it."""

    def __init__(self, image):
        self.ramps, self.atlas_size, self.uploads, self._image = None, 0, [], image

    def atlas_image(self):
        return self._image


def atlas_scene(which):
    """Three image fills over a 160 x 120 frame, each under a rotated brush transform (bilinear and bicubic taps reach the image's
    edge texels, and the extend modes wrap across them).  Returns (patched packed bytes, layout, atlas as the oracle takes it,
    [(x, y, texels)])."""
    import vello_amd
    from vello_amd import Affine, Extend, Fill, ImageAlphaType, ImageBrush, ImageData, ImageFormat, ImageQuality, Rect, Scene
    from workloads.scenes import _test_image

    aw, ah, places = ATLASES[which]
    q = [ImageQuality((which + k) % 3) for k in range(3)]
    texels = [_test_image(places[0][0], places[0][1], 10 + which), _test_image(places[1][0], places[1][1], 20 + which),
              _test_image(places[2][0], places[2][1], 30 + which, premultiplied=True)]
    images = [ImageData(texels[0]), ImageData(texels[1], ImageFormat.Bgra8),
              ImageData(texels[2], ImageFormat.Rgba8, ImageAlphaType.AlphaPremultiplied)]
    s = Scene()
    s.fill(Fill.NonZero, Affine.IDENTITY, ImageBrush(images[0], Extend.Pad, Extend.Pad, q[0]),
           Affine.translate(20, 30) * Affine.rotate(0.4) * Affine.scale(1.3), Rect(2, 2, 78, 118))
    s.fill(Fill.NonZero, Affine.IDENTITY, ImageBrush(images[1], Extend.Repeat, Extend.Reflect, q[1], 0.8),
           Affine.translate(90, 5) * Affine.rotate(0.3) * Affine.scale(1.7), Rect(82, 2, 158, 58))
    s.fill(Fill.NonZero, Affine.IDENTITY, ImageBrush(images[2], Extend.Reflect, Extend.Repeat, q[2]),
           Affine.translate(100, 70) * Affine.rotate(-0.5) * Affine.scale_non_uniform(0.9, 1.4), Rect(82, 62, 158, 118))
    r = vello_amd.Resolver().resolve(s)
    assert len(r.uploads) == 3
    packed = np.ascontiguousarray(r.packed, dtype=np.uint8).copy()
    words = packed.view(np.uint32)
    lo, hi = r.layout.draw_data_base, r.layout.transform_base
    atlas = np.zeros((ah, aw, 4), dtype=np.uint8)
    writes = []
    # DrawImage = [xy, width_height, sample_alpha] (resolver.cpp / resolve.rs:300-316 patch xy = (x << 16) | y): the resolver's
    # place of each image is replaced by this test's
    found = {}
    for x0, y0, px in r.uploads:
        ih, iw = px.shape[:2]
        k = [i for i in range(3) if texels[i].shape == px.shape and np.array_equal(texels[i], px)]
        assert len(k) == 1
        at = [i for i in range(lo, hi - 1) if words[i] == ((x0 << 16) | y0) and words[i + 1] == ((iw << 16) | ih)]
        assert len(at) == 1, (at, x0, y0)
        found[k[0]] = at[0]
    for k in range(3):
        iw, ih, x, y = places[k]
        assert x + iw <= aw and y + ih <= ah
        words[found[k]] = (x << 16) | y
        assert not atlas[y:y + ih, x:x + iw].any(), "the case's own images overlap"
        atlas[y:y + ih, x:x + iw] = texels[k]
        writes.append((x, y, texels[k]))
    assert places[0][2] + places[0][0] == aw and places[1][3] + places[1][1] == ah
    assert places[2][2] >= ah if aw > ah else places[2][3] >= aw
    return packed, r.layout, atlas, writes


def _framed(texels, seed):
    """`texels` as a slice of a larger array of other bytes: (the larger array, the slice)."""
    h, w = texels.shape[:2]
    big = np.random.default_rng(seed).integers(0, 256, (h + 3, w + 5, 4), dtype=np.uint8)
    big[1:1 + h, 2:2 + w] = texels
    return big, big[1:1 + h, 2:2 + w]


def check_atlas(engine, name, which, device_source=None):
    """Atlas ATLASES[which], filled through write_image from slices of larger host arrays (device_source None), or through one
    copy_images_device batch from strided sources (`device_source`: host array -> the same array in device memory)."""
    from vello_amd import AaConfig

    packed, layout, atlas, writes = atlas_scene(which)
    aw, ah = ATLASES[which][0], ATLASES[which][1]
    engine.resize_image_atlas(aw, ah)
    keep = []
    if device_source is None:
        for k, (x, y, px) in enumerate(writes):
            big, view = _framed(px, 50 + k)
            assert not view.flags["C_CONTIGUOUS"]
            engine.write_image(x, y, view)
    else:
        copies = []
        for k, (x, y, px) in enumerate(writes):
            big = device_source(_framed(px, 60 + k)[0])
            keep.append(big)
            view = big[1:1 + px.shape[0], 2:2 + px.shape[1]]
            stride = view.strides[0] if isinstance(view, np.ndarray) else view.stride(0)
            assert stride == (px.shape[1] + 5) * 4
            copies.append((x, y, px.shape[1], px.shape[0], view, stride))
        engine.copy_images_device(copies)
    for aa in (AaConfig.Area, AaConfig.Msaa16):
        parity.compare_frame(engine, packed, layout, 160, 120, BLACK, aa, f"{name}_{aw}x{ah}_aa{int(aa)}", tol=_tol(aa), resolved=_Atlas(atlas))
    del keep
