"""vello::Renderer / RenderParams / AaConfig (vello/src/lib.rs:175-193, :357-369, :432-515) and a
direct binding of the engine C ABI (include/vello_hip.h) for measurement and differential tests."""
import collections
import ctypes
import enum

import numpy as np

from ._lib import (load_library, is_emulated, VelloHipError, Capacities, Bump, LayoutStruct, RenderParamsStruct, ImageCopyStruct, FragmentStruct,
                   InstanceStruct, PaintStruct, RegionCounts)
from .scene import Color, ImageAlphaType, ImageData, ImageFormat


class AaConfig(enum.IntEnum):
    Area = 0
    Msaa8 = 1
    Msaa16 = 2


Layout = collections.namedtuple("Layout", [
    "n_draw_objects", "n_paths", "n_clips", "bin_data_start", "path_tag_base", "path_data_base", "draw_tag_base",
    "draw_data_base", "transform_base", "style_base"])

STAGES = ["pathtag_scan", "flatten", "draw_scan", "clip", "binning", "tile_alloc", "path_count", "backdrop", "coarse",
          "path_tiling", "fine"]
BUFFERS = ["scene", "config", "tag_monoids", "path_bboxes", "bump", "lines", "draw_monoids", "info_bin_data", "clip_inp",
           "clip_bboxes", "draw_bboxes", "bin_headers", "paths", "tiles", "seg_counts", "segments", "ptcl", "blend_spill",
           "output"]

E_CAPACITY = -4
PICK_NONE = 0xFFFFFFFF  # VELLO_HIP_PICK_NONE: no draw object under the point / the frame was not composed from instances
PICK_MAX_POINTS = 4096  # VELLO_HIP_PICK_MAX_POINTS
REGION_TOUCHED, REGION_ENCLOSED = 1, 2  # VELLO_HIP_REGION_*: the two bits of a word of Engine.pick_rect
PATH_DATA_SCENE, PATH_DATA_DEVICE = 0xFFFFFFFF, 0xFFFFFFFE  # VELLO_HIP_PATH_DATA_*: the sources of a morphed frame that are not keyframes


class RenderParams:
    """`view` (an Affine, or six floats [m0 m1 m2 m3 t0 t1]; default None) is a view transform for this frame only: the engine
    composes it in front of every transform of the scene (vello_hip_set_view_transform).  `damage` ((x0, y0, x1, y1) in pixels,
    half open; default None) is a damage rectangle for this frame only: the frame writes only those pixels of the target
    (vello_hip_set_damage_rect).  `stroke_scale` ((scale, min_width); default None) is a stroke scale for this frame only: every
    stroke width w > 0 is rendered as max(w * scale, min_width) (vello_hip_set_stroke_scale).  `base_image` (what
    Engine.set_base_image takes as `image`, or an (image, stride) pair; default None) is a base image for this frame only: the frame
    is drawn over its premultiplied RGBA8 words instead of `base_color` (vello_hip_set_base_image); a tensor is ordered behind
    torch's current stream."""

    def __init__(self, base_color, width, height, antialiasing_method=AaConfig.Area, view=None, damage=None, stroke_scale=None,
                 base_image=None):
        self.base_color, self.width, self.height, self.antialiasing_method = base_color, width, height, antialiasing_method
        self.view = view
        self.damage = damage
        self.stroke_scale = stroke_scale
        self.base_image = base_image


def _base_image_source(image, stride=None):
    """(address, row stride in bytes) of a base image: an [H, W, 4] uint8 or [H, W] int32 / uint32 tensor on the GPU whose texels
    are premultiplied RGBA8 words (any row stride that is a multiple of 4, so a slice of a larger tensor works), or a raw device
    address with `stride` (None / 0: width * 4 of the frame).  A numpy array of the same shape stands for device memory only in the
    SIMT-emulated build that the CPU tests load; the GPU build refuses its address when the frame is enqueued."""
    if image is None:
        return None, 0
    if isinstance(image, (int, np.integer)):
        return int(image), int(stride or 0)
    is_np = isinstance(image, np.ndarray)
    if not is_np and not hasattr(image, "data_ptr"):
        raise ValueError("a base image is a tensor on the GPU or a device address")
    strides = image.strides if is_np else tuple(st * image.element_size() for st in image.stride())
    shape, item = tuple(image.shape), (image.itemsize if is_np else image.element_size())
    words = len(shape) == 2 and item == 4 and strides[1] == 4
    bytes4 = len(shape) == 3 and shape[2] == 4 and item == 1 and strides[2] == 1 and strides[1] == 4
    if not (words or bytes4) or "float" in str(image.dtype):
        raise ValueError("a base image is an [H, W, 4] uint8 or [H, W] int32 tensor of premultiplied RGBA8 words")
    if not is_np and not image.is_cuda:
        raise ValueError("a base image lives on the GPU")
    if stride not in (None, 0) and int(stride) != strides[0]:
        raise ValueError(f"stride {stride} given for a tensor whose rows are {strides[0]} bytes apart")
    return (image.ctypes.data if is_np else image.data_ptr()), int(strides[0])


def _damage_words(rect):
    """x0 y0 x1 y1 as the four u32 of vello_hip_set_damage_rect (None: the option off)."""
    if rect is None:
        return None
    rect = tuple(rect)
    if len(rect) != 4 or any(int(v) < 0 or int(v) > 0xFFFFFFFF for v in rect):
        raise ValueError("a damage rectangle is (x0, y0, x1, y1) in pixels, half open")
    return (ctypes.c_uint32 * 4)(*[int(v) for v in rect])


def _view_floats(view):
    """Transform::from_kurbo (vello_encoding/src/math.rs): the six coefficients of an Affine (or six numbers) as f32."""
    if view is None:
        return None
    coeffs = view.c if hasattr(view, "c") else tuple(view)
    if len(coeffs) != 6:
        raise ValueError("a view transform has six coefficients [m0 m1 m2 m3 t0 t1]")
    return (ctypes.c_float * 6)(*[float(v) for v in coeffs])


def _stroke_floats(scale, min_width=0.0):
    """(scale, min_width) as the two f32 of vello_hip_set_stroke_scale (scale None: the option off)."""
    if scale is None:
        return None
    return (ctypes.c_float * 2)(float(scale), float(min_width))


def path_data_view(packed, layout):
    """The path-data words of a packed scene -- [path_data_base, draw_tag_base) of `layout` -- as a float32 view of `packed` (a
    C-contiguous uint8 array: writing through the view edits the scene).  (x, y) pairs in a scene whose segment tags are all f32;
    what Engine.upload_path_keyframes and Engine.render_resident(points=...) take has this length and this meaning."""
    if not isinstance(packed, np.ndarray) or packed.dtype != np.uint8 or not packed.flags["C_CONTIGUOUS"]:
        raise ValueError("packed is a C-contiguous uint8 array")
    return packed.reshape(-1).view(np.float32)[layout.path_data_base: layout.draw_tag_base]


INSTANCE_DTYPE = np.dtype([("fragment", "<u4"), ("transform", "<f4", (6,))])  # vello_hip_instance, 28 bytes
assert INSTANCE_DTYPE.itemsize == ctypes.sizeof(InstanceStruct)
PAINT_DTYPE = np.dtype([("flags", "<u4"), ("rgba", "<u4")])  # vello_hip_paint, 8 bytes
assert PAINT_DTYPE.itemsize == ctypes.sizeof(PaintStruct)
PAINT_KEEP, PAINT_SOLID = 0, 1  # VELLO_HIP_PAINT_KEEP / _SOLID
FRAGMENT_STREAMS = ("path_tags", "path_data", "draws", "draw_data", "transforms", "styles")


def instance_array(instances):
    """An INSTANCE_DTYPE array of (fragment index, transform) pairs; a transform is an Affine or six floats [m0 m1 m2 m3 t0 t1]."""
    if isinstance(instances, np.ndarray) and instances.dtype == INSTANCE_DTYPE:
        return np.ascontiguousarray(instances)
    out = np.zeros(len(instances), dtype=INSTANCE_DTYPE)
    for i, (fragment, transform) in enumerate(instances):
        out[i]["fragment"] = int(fragment)
        out[i]["transform"] = [float(v) for v in (transform.c if hasattr(transform, "c") else transform)]
    return out


def paint_array(paints):
    """A PAINT_DTYPE array of per-instance paints: None keeps the library's colours, an int is a premultiplied RGBA8 word (R in the
    low byte, as base_color), a Color is quantised as the encoder quantises a solid brush (Color.premul_rgba8)."""
    if isinstance(paints, np.ndarray) and paints.dtype == PAINT_DTYPE:
        return np.ascontiguousarray(paints)
    out = np.zeros(len(paints), dtype=PAINT_DTYPE)
    for i, paint in enumerate(paints):
        if paint is not None:
            out[i] = (PAINT_SOLID, paint.premul_rgba8() if isinstance(paint, Color) else int(paint))
    return out


class FragmentLibrary:
    """A list of Scenes appended into ONE Scene (Scene.append without a transform), resolved once: what Engine.upload_fragments
    makes resident.  `fragments[i]` holds scene i's half-open range in each of the six streams, taken from the stream sizes before
    and after its append; `resolved` is the Resolver's result for the whole (its ramps and atlas serve every instance frame)."""

    def __init__(self, scenes, resolver=None):
        from .scene import Resolver, Scene

        self.scene = Scene()
        self.fragments = []
        before = self._sizes()
        for s in scenes:
            self.scene.append(s)
            after = self._sizes()
            self.fragments.append({k: (before[k], after[k]) for k in FRAGMENT_STREAMS})
            before = after
        self.resolved = (resolver or Resolver()).resolve(self.scene)
        self.packed, self.layout, self.ramps = self.resolved.packed, self.resolved.layout, self.resolved.ramps

    def _sizes(self):
        lib, h = self.scene._lib, self.scene._h
        unit = {"path_tags": 1, "path_data": 4, "draws": 4, "draw_data": 4, "transforms": 24, "styles": 8}
        return {k: lib.vh_scene_stream_bytes(h, i) // unit[k] for i, k in enumerate(FRAGMENT_STREAMS)}

    def upload(self, engine):
        """Atlas, ramps, packed scene and the fragment table (Engine.upload_resolved with upload_fragments in upload_scene's place)."""
        r = self.resolved
        if r.atlas_size:
            engine.resize_image_atlas(r.atlas_size, r.atlas_size)
            for x, y, px in r.uploads:
                engine.write_image(x, y, px)
        engine.upload_fragments(r.packed, r.layout, self.fragments, r.ramps)


class RendererOptions:
    def __init__(self, device=0, antialiasing_support=7, capacities=None, viewport_cull=False):
        self.device, self.antialiasing_support, self.capacities = device, antialiasing_support, capacities
        self.viewport_cull = viewport_cull  # Engine.set_viewport_cull


def _caps(capacities):
    if capacities is None:
        return None
    c = Capacities()
    for k, v in capacities.items():
        setattr(c, k, v)
    return ctypes.byref(c)


def _data_ptr(texture, width=None, height=None):
    """Accepts a numpy array (host) or a torch tensor (host or device): dense uint8 rows of `width` RGBA8 pixels.
    With width / height given, the buffer must hold the whole target (the engine writes height * width * 4 bytes)."""
    if isinstance(texture, np.ndarray):
        if texture.dtype != np.uint8 or not texture.flags["C_CONTIGUOUS"]:
            raise ValueError("target must be a C-contiguous uint8 array")
        nbytes, ptr, is_dev = texture.nbytes, texture.ctypes.data, False
    else:
        import torch

        if texture.dtype != torch.uint8 or not texture.is_contiguous():
            raise ValueError("target must be a contiguous torch.uint8 tensor")
        nbytes, ptr, is_dev = texture.numel(), texture.data_ptr(), bool(texture.is_cuda)
    if width is not None and nbytes < int(width) * int(height) * 4:
        raise ValueError(f"target holds {nbytes} bytes, a {width}x{height} RGBA8 frame needs {int(width) * int(height) * 4}")
    return ptr, is_dev


def _target(lib, texture, width, height, device_only=False, stride=None):
    """(address, row stride in bytes, is_device) of a render target: the first height x width x 4 bytes of a dense uint8 buffer (as
    _data_ptr takes it), or an [H, W, 4] uint8 array / tensor of at least that size whose texels are RGBA8 words (stride(2) == 1,
    stride(1) == 4) and whose rows lie stride(0) bytes apart -- a slice of a larger surface works, as for _texture_source.  The
    engine writes the first width * 4 bytes of the first `height` rows and nothing else (include/vello_hip.h).  A numpy array is a
    host target; it stands for device memory only in the SIMT-emulated build, so with `device_only` the GPU build refuses it.
    `stride` (bytes) replaces the geometry read from `texture`, which then only supplies the address: the engine judges it."""
    width, height = int(width), int(height)
    is_np = isinstance(texture, np.ndarray)
    if not is_np:
        import torch

        if not isinstance(texture, torch.Tensor):
            raise ValueError("target must be a numpy array or a torch tensor")
    dtype_ok = texture.dtype == np.uint8 if is_np else str(texture.dtype) == "torch.uint8"
    if not dtype_ok:
        raise ValueError("target must hold uint8")
    ndim = texture.ndim if is_np else texture.dim()
    strides = tuple(texture.strides) if is_np else tuple(texture.stride())
    dense = texture.flags["C_CONTIGUOUS"] if is_np else texture.is_contiguous()
    if stride is not None:
        ptr, stride = (texture.ctypes.data if is_np else texture.data_ptr()), int(stride)
        is_dev = False if is_np else bool(texture.is_cuda)
    elif dense:
        ptr, is_dev = _data_ptr(texture, width, height)
        stride = width * 4
    elif ndim == 3 and texture.shape[2] == 4 and strides[2] == 1 and strides[1] == 4 and (strides[0] >= 0):
        if texture.shape[0] < height or texture.shape[1] < width:
            raise ValueError(f"target is {texture.shape[1]}x{texture.shape[0]}, the frame {width}x{height}")
        ptr = texture.ctypes.data if is_np else texture.data_ptr()
        stride = int(strides[0])
        is_dev = False if is_np else bool(texture.is_cuda)
    else:
        raise ValueError("target must be dense, or an [H, W, 4] uint8 view with stride(2) == 1 and stride(1) == 4")
    if device_only and not is_dev:
        if not (is_np and is_emulated(lib)):
            raise ValueError("this entry point writes to device memory: the target must be a tensor on the GPU")
        is_dev = True
    return ptr, stride, is_dev


def _texture_source(source):
    """(address, row stride in bytes, height, width) of an override source: an [H, W, 4] uint8 tensor on the GPU whose texels
    are RGBA8 words (stride(2) == 1, stride(1) == 4; any row stride, so a slice of a larger tensor works).  A numpy array of
    the same shape stands for device memory only in the SIMT-emulated build that the CPU tests load; the GPU build refuses it."""
    if isinstance(source, np.ndarray):
        if source.dtype != np.uint8 or source.ndim != 3 or source.shape[2] != 4 or source.strides[2] != 1 or source.strides[1] != 4:
            raise ValueError("an override source is an [H, W, 4] uint8 array of RGBA8 words")
        return source.ctypes.data, source.strides[0], source.shape[0], source.shape[1]
    import torch

    if (not isinstance(source, torch.Tensor) or source.dtype != torch.uint8 or source.dim() != 3 or source.shape[2] != 4
            or source.stride(2) != 1 or source.stride(1) != 4):
        raise ValueError("an override source is a torch.uint8 tensor of shape [H, W, 4] with stride(2) == 1 and stride(1) == 4")
    if not source.is_cuda:
        raise ValueError("an override source lives on the GPU")
    return source.data_ptr(), source.stride(0), source.shape[0], source.shape[1]


def _source_stream(stream):
    """(hipStream_t for src_stream, relay) for a torch stream.  The null stream cannot be named through the C ABI (NULL there
    means "no source stream"), so its work is relayed through a pool stream ordered behind it; the caller then makes the null
    stream wait for the relay (relay = (null stream, pool stream)).  Device-side ordering only, no host wait."""
    import torch

    if stream.cuda_stream:
        return stream.cuda_stream, None
    pool = torch.cuda.Stream(device=stream.device)
    pool.wait_stream(stream)
    return pool.cuda_stream, (stream, pool)


class Renderer:
    """Renderer::new + Renderer::render_to_texture.  Raises VelloHipError when no GPU is usable."""

    def __init__(self, options=None):
        options = options or RendererOptions()
        self._lib = load_library()
        err = ctypes.create_string_buffer(512)
        self._h = self._lib.vh_renderer_new(options.device, options.antialiasing_support, _caps(options.capacities), err, 512)
        if not self._h:
            raise VelloHipError(err.value.decode() or "vello_hip_create failed")
        self._overrides = {}  # image id -> source (the renderer keeps it alive, as upstream holds the wgpu::Texture)
        if getattr(options, "viewport_cull", False):
            r = self._lib.vello_hip_set_viewport_cull(self._lib.vh_renderer_engine(self._h), 1)
            if r != 0:
                raise VelloHipError(f"vello_hip_set_viewport_cull failed ({r})")

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.vh_renderer_free(self._h)
        except Exception:
            pass
        self._h = None

    def render_to_texture(self, scene, texture, params):
        """Override sources are copied into the atlas in one batch behind the work already enqueued on torch's current stream,
        which then waits for the copy (vello_hip_copy_images_device)."""
        ptr, stride, is_dev = _target(self._lib, texture, params.width, params.height)
        src_stream = relay = None
        if any(not isinstance(t, np.ndarray) for t in self._overrides.values()):
            import torch

            src_stream, relay = _source_stream(torch.cuda.current_stream())
        # a damage rectangle holds for this frame only: set on the engine before the call, cleared after it (as the view is)
        damage = _damage_words(getattr(params, "damage", None))
        engine = self._lib.vh_renderer_engine(self._h)
        if damage is not None and self._lib.vello_hip_set_damage_rect(engine, damage) != 0:
            raise VelloHipError(f"render_to_texture: {self._lib.vello_hip_last_error(engine).decode()}")
        # ... and so does a stroke scale
        stroke = getattr(params, "stroke_scale", None)
        stroke = None if stroke is None else _stroke_floats(*stroke)
        if stroke is not None and self._lib.vello_hip_set_stroke_scale(engine, stroke) != 0:
            if damage is not None:
                self._lib.vello_hip_set_damage_rect(engine, None)
            raise VelloHipError(f"render_to_texture: {self._lib.vello_hip_last_error(engine).decode()}")
        # ... and so does a base image (a tensor: ordered behind torch's current stream, which then waits for the frame's fine)
        base = getattr(params, "base_image", None)
        base_relay = None
        if base is not None:
            try:
                b_addr, b_stride = _base_image_source(*base) if isinstance(base, tuple) else _base_image_source(base)
                b_stream = None
                if hasattr(base[0] if isinstance(base, tuple) else base, "is_cuda"):
                    import torch

                    b_stream, base_relay = _source_stream(torch.cuda.current_stream())
                if self._lib.vello_hip_set_base_image(engine, b_addr, b_stride, b_stream) != 0:
                    raise VelloHipError(f"render_to_texture: {self._lib.vello_hip_last_error(engine).decode()}")
            except Exception:
                if damage is not None:
                    self._lib.vello_hip_set_damage_rect(engine, None)
                if stroke is not None:
                    self._lib.vello_hip_set_stroke_scale(engine, None)
                raise
        try:
            r = self._lib.vh_renderer_render_to_texture_view(self._h, scene._h, ptr, stride, 1 if is_dev else 0, params.width, params.height,
                                                             params.base_color._ptr(), int(params.antialiasing_method), src_stream,
                                                             _view_floats(getattr(params, "view", None)))
        finally:
            if damage is not None:
                self._lib.vello_hip_set_damage_rect(engine, None)
            if stroke is not None:
                self._lib.vello_hip_set_stroke_scale(engine, None)
            if base is not None:
                self._lib.vello_hip_set_base_image(engine, None, 0, None)
        if base_relay is not None:
            base_relay[0].wait_stream(base_relay[1])
        if relay is not None:
            relay[0].wait_stream(relay[1])
        if r != 0:
            raise VelloHipError(f"render_to_texture failed ({r}): {self._lib.vh_renderer_error(self._h).decode()}")

    def override_image(self, image, source):
        """Renderer::override_image (lib.rs:536-545): whenever `image` is scheduled for upload into the atlas, its texels are
        copied from `source` (an [H, W, 4] RGBA8 tensor on the GPU of the image's size; see _texture_source) instead of its
        pixels; None removes the override.  Marks the image dirty.  Returns the previous source or None."""
        if source is not None:
            addr, row_stride, h, w = _texture_source(source)
            if (h, w) != (image.height, image.width):
                raise ValueError(f"override source is {w}x{h}, the image {image.width}x{image.height}")
            self._lib.vh_renderer_override_image(self._h, ctypes.c_uint64(image.id), 1, addr, row_stride, None)
        else:
            self._lib.vh_renderer_override_image(self._h, ctypes.c_uint64(image.id), 0, 0, 0, None)
        previous = self._overrides.pop(image.id, None)
        if source is not None:
            self._overrides[image.id] = source
        return previous

    def mark_override_image_dirty(self, image):
        """Renderer::mark_override_image_dirty (lib.rs:547-555): the source's contents changed; the next render that uses the
        image copies it again (otherwise the atlas keeps the texels of the last copy)."""
        self._lib.vh_renderer_mark_override_image_dirty(self._h, ctypes.c_uint64(image.id))

    def register_texture(self, texture):
        """Renderer::register_texture (lib.rs:557-604): a pixel-less Rgba8 / straight-alpha ImageData of the texture's size with
        the texture as its override."""
        _, _, h, w = _texture_source(texture)
        image = ImageData.empty(w, h, ImageFormat.Rgba8, ImageAlphaType.Alpha)
        self.override_image(image, texture)
        return image

    def unregister_texture(self, image):
        """Renderer::unregister_texture (lib.rs:606-609)."""
        self.override_image(image, None)

    def last_bump(self):
        b = Bump()
        self._lib.vh_renderer_last_bump(self._h, ctypes.byref(b))
        return b.as_dict()


class Engine:
    """Direct binding of include/vello_hip.h (one context = one GPU, one stream)."""

    def __init__(self, device=0, aa_mask=7, capacities=None):
        self._lib = load_library()
        h = ctypes.c_void_p()
        r = self._lib.vello_hip_create(device, aa_mask, _caps(capacities), ctypes.byref(h))
        if r != 0:
            raise VelloHipError(f"vello_hip_create failed ({r}): {self._lib.vello_hip_last_error(None).decode()}")
        self._h = h

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._lib.vello_hip_destroy(self._h)
        except Exception:
            pass
        self._h = None

    def _check(self, r, what):
        if r != 0:
            err = VelloHipError(f"{what} failed ({r}): {self._lib.vello_hip_last_error(self._h).decode()}")
            err.code = r  # the VELLO_HIP_E_* code
            raise err

    @staticmethod
    def _params(width, height, base_color, aa):
        bc = base_color.premul_rgba8() if isinstance(base_color, Color) else int(base_color)
        return RenderParamsStruct(width, height, bc, int(aa))

    def upload_scene(self, packed, layout, ramps=None):
        """Command::Upload of the packed scene (+ the gradient ramp texture: n_ramps x 512 RGBA8 texels as uint32)."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        lay = LayoutStruct(*layout)
        rp, nr = None, 0
        if ramps is not None and len(ramps):
            ramps = np.ascontiguousarray(ramps, dtype=np.uint32)
            rp, nr = ramps.ctypes.data, ramps.size // 512
        self._retained_n = None  # (an upload drops the retained list)
        self._check(self._lib.vello_hip_upload_scene(self._h, packed.ctypes.data, packed.nbytes, ctypes.byref(lay), rp, nr), "upload_scene")

    def resize_image_atlas(self, width, height):
        self._check(self._lib.vello_hip_resize_image_atlas(self._h, width, height), "resize_image_atlas")

    def write_image(self, x, y, pixels):
        """vello_hip_write_image of an [H, W, 4] uint8 host array; its row stride is the array's own, so a slice of a larger array
        is uploaded without a copy (anything else is made dense first)."""
        pixels = np.asarray(pixels, dtype=np.uint8)
        if pixels.ndim != 3 or pixels.shape[2] != 4 or pixels.strides[2] != 1 or pixels.strides[1] != 4 or pixels.strides[0] < pixels.shape[1] * 4:
            pixels = np.ascontiguousarray(pixels)
        h, w = pixels.shape[:2]
        self._check(self._lib.vello_hip_write_image(self._h, x, y, w, h, pixels.ctypes.data, pixels.strides[0] if pixels.ndim == 3 else w * 4),
                    "write_image")

    def copy_images_device(self, copies, stream=None):
        """vello_hip_copy_images_device: `copies` are (x, y, width, height, address, row stride in bytes) entries, copied into the
        atlas by one kernel launch.  The entries of a call are copied concurrently: their destinations must not overlap, and no
        source may lie in the atlas.  Calls are ordered among themselves and against frames (behind the frames enqueued before,
        in front of those enqueued after).  An address is an int or an array / tensor (its first texel).  `stream`
        (a hipStream_t as an int, or a torch stream -- torch's default stream included) is the stream that writes the sources: the
        copy runs behind it, and it waits for the copy.  Returns without waiting."""
        arr = (ImageCopyStruct * max(len(copies), 1))()
        for i, (x, y, w, h, addr, row_stride) in enumerate(copies):
            if hasattr(addr, "data_ptr"):
                addr = addr.data_ptr()
            elif isinstance(addr, np.ndarray):
                addr = addr.ctypes.data
            arr[i] = ImageCopyStruct(int(addr or 0), int(row_stride), int(x), int(y), int(w), int(h))
        relay = None
        if hasattr(stream, "cuda_stream"):
            s, relay = _source_stream(stream)
        else:
            s = stream
        r = self._lib.vello_hip_copy_images_device(self._h, arr, len(copies), ctypes.c_void_p(int(s)) if s else None)
        if relay is not None:
            relay[0].wait_stream(relay[1])
        self._check(r, "copy_images_device")

    def upload_resolved(self, resolved, sources=None):
        """Everything a Resolver result carries: atlas (re)creation + image writes, ramps, packed scene.  Pixel-less images
        (resolved.device_uploads) are copied from `sources` ({image id: device source, as override_image takes}) in one
        copy_images_device batch; one without a source is refused, as Renderer refuses it, before anything is uploaded."""
        missing = [i for _, _, _, _, i in resolved.device_uploads if sources is None or i not in sources]
        if missing:
            raise VelloHipError(f"Tried to draw an invalid empty image (id {missing[0]}): no source for a pixel-less image")
        if resolved.atlas_size:
            self.resize_image_atlas(resolved.atlas_size, resolved.atlas_size)
            for x, y, px in resolved.uploads:
                self.write_image(x, y, px)
            if resolved.device_uploads:
                copies = []
                for x, y, w, h, i in resolved.device_uploads:
                    addr, row_stride, sh, sw = _texture_source(sources[i])
                    if (sh, sw) != (h, w):
                        raise ValueError(f"source of image {i} is {sw}x{sh}, the image {w}x{h}")
                    copies.append((x, y, w, h, addr, row_stride))
                self.copy_images_device(copies)
        self.upload_scene(resolved.packed, resolved.layout, resolved.ramps)

    def render_frame(self, packed, layout, width, height, base_color, aa, out=None, ramps=None, out_stride=None):
        """vello_hip_render_frame: upload this frame's scene into the next in-flight slot and enqueue the frame."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        lay = LayoutStruct(*layout)
        p = self._params(width, height, base_color, aa)
        ptr, stride = None, 0
        if out is not None:
            ptr, stride, _ = _target(self._lib, out, width, height, device_only=True, stride=out_stride)
        rp, nr = None, 0
        if ramps is not None and len(ramps):
            ramps = np.ascontiguousarray(ramps, dtype=np.uint32)
            rp, nr = ramps.ctypes.data, ramps.size // 512
        self._check(self._lib.vello_hip_render_frame(self._h, packed.ctypes.data, packed.nbytes, ctypes.byref(lay), ctypes.byref(p),
                                                     rp, nr, ptr, stride), "render_frame")

    def upload_fragments(self, packed, layout, fragments, ramps=None):
        """vello_hip_upload_fragments: upload_scene plus a fragment table.  `fragments` is a sequence of dicts (or objects with
        these attributes) holding a half-open (begin, end) range per stream: path_tags, path_data, draws, draw_data, transforms,
        styles -- what FragmentLibrary.fragments holds."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        lay = LayoutStruct(*layout)
        rp, nr = None, 0
        if ramps is not None and len(ramps):
            ramps = np.ascontiguousarray(ramps, dtype=np.uint32)
            rp, nr = ramps.ctypes.data, ramps.size // 512
        arr = (FragmentStruct * max(len(fragments), 1))()
        for i, f in enumerate(fragments):
            for name, _ in FragmentStruct._fields_:
                b, e = f[name] if isinstance(f, dict) else getattr(f, name)
                getattr(arr[i], name)[:] = (int(b), int(e))
        self._retained_n = None  # (an upload drops the retained list)
        self._check(self._lib.vello_hip_upload_fragments(self._h, packed.ctypes.data, packed.nbytes, ctypes.byref(lay), rp, nr, arr,
                                                         len(fragments)), "upload_fragments")

    def instances_layout(self, instances):
        """vello_hip_instances_layout: (Layout, scene length in bytes) of the scene that `instances` compose from the resident
        fragments; host only."""
        inst = instance_array(instances)
        lay, n = LayoutStruct(), ctypes.c_size_t()
        self._check(self._lib.vello_hip_instances_layout(self._h, inst.ctypes.data, len(inst), ctypes.byref(lay), ctypes.byref(n)),
                    "instances_layout")
        return Layout(*[getattr(lay, k) for k, _ in LayoutStruct._fields_]), int(n.value)

    def render_instances(self, instances, width, height, base_color, aa, out=None, out_stride=None, paints=None):
        """vello_hip_render_instances: composes this frame's scene on the GPU from `instances` -- (fragment index, transform) pairs
        or an INSTANCE_DTYPE array -- of the fragments of upload_fragments, and enqueues the frame like render_frame.  With `paints`
        (what paint_array takes, one entry per instance) it is vello_hip_render_instances_painted: the colour words of every instance
        with a paint become that paint."""
        inst = instance_array(instances)
        p = self._params(width, height, base_color, aa)
        ptr, stride = None, 0
        if out is not None:
            ptr, stride, _ = _target(self._lib, out, width, height, device_only=True, stride=out_stride)
        if paints is None:
            self._check(self._lib.vello_hip_render_instances(self._h, inst.ctypes.data, len(inst), ctypes.byref(p), ptr, stride), "render_instances")
            return
        pt = paint_array(paints)
        if len(pt) != len(inst):
            raise ValueError(f"{len(pt)} paints for {len(inst)} instances")
        # (an empty numpy array still has an address: n == 0 with a paint list is a call with a non-null pointer)
        self._check(self._lib.vello_hip_render_instances_painted(self._h, inst.ctypes.data, pt.ctypes.data, len(inst), ctypes.byref(p), ptr, stride),
                    "render_instances_painted")

    def retain_instances(self, instances, paints=None):
        """vello_hip_retain_instances: composes `instances` (and `paints`, as render_instances takes them) ONCE into the context's
        retained scene; render_retained then draws the list under per-frame poses.  Waits for the frames in flight; a second call
        replaces the list, an upload drops it."""
        inst = instance_array(instances)
        pt = None
        if paints is not None:
            pt = paint_array(paints)
            if len(pt) != len(inst):
                raise ValueError(f"{len(pt)} paints for {len(inst)} instances")
        self._retained_n = None
        self._check(self._lib.vello_hip_retain_instances(self._h, inst.ctypes.data, pt.ctypes.data if pt is not None else None, len(inst)),
                    "retain_instances")
        self._retained_n = len(inst)

    def render_retained(self, width, height, base_color, aa, transforms=None, out=None, out_stride=None, src_stream=None,
                        transforms_is_device=False, paints=None, paints_is_device=False):
        """vello_hip_render_retained: one frame of the retained list under this frame's poses, enqueued like render_instances.
        `transforms`: None (the rest poses), an (n, 6) float32 numpy array (host memory: copied during the call), or poses in device
        memory -- a float32 tensor of n * 6 elements on the engine's GPU, or its address as an int -- which the host never reads.
        `transforms_is_device` says that a numpy array stands for device memory (the emulated build only).  `src_stream` (a
        hipStream_t as an int, or a torch stream) is the stream that writes device poses: the frame runs behind it, and it waits for
        the kernel that reads them.
        `paints` makes it vello_hip_render_retained_painted, this frame's colours: what paint_array takes or a PAINT_DTYPE array (host
        memory: copied during the call; None entries and PAINT_KEEP keep what the list was retained with), or paints in device
        memory -- an int32 / uint32 tensor of n * 2 elements (flags, rgba) on the engine's GPU, or its address as an int -- which the
        host never reads.  `paints_is_device` says that a numpy array stands for device memory (the emulated build only).
        `src_stream` then orders device paints as it orders device poses."""
        numpy_is_device = bool(transforms_is_device)
        p = self._params(width, height, base_color, aa)
        ptr, stride = None, 0
        if out is not None:
            ptr, stride, _ = _target(self._lib, out, width, height, device_only=True, stride=out_stride)
        n = getattr(self, "_retained_n", None)
        keep, tp, is_dev = None, None, 0
        if transforms is None:
            pass
        elif isinstance(transforms, np.ndarray):
            if numpy_is_device and not is_emulated(self._lib):
                raise ValueError("a numpy array is host memory: device poses are a tensor on the GPU")
            keep = np.ascontiguousarray(transforms, dtype=np.float32)
            if n is not None and keep.size != n * 6:
                raise ValueError(f"{keep.size} floats for {n} retained instances (6 each)")
            tp, is_dev = keep.ctypes.data, int(numpy_is_device)
        elif hasattr(transforms, "data_ptr"):
            import torch

            if transforms.dtype != torch.float32 or not transforms.is_contiguous():
                raise ValueError("poses are a contiguous float32 tensor of n * 6 elements")
            if n is not None and transforms.numel() != n * 6:
                raise ValueError(f"{transforms.numel()} floats for {n} retained instances (6 each)")
            if transforms.is_cuda:
                tp, is_dev = transforms.data_ptr(), 1
            else:
                keep = transforms.numpy()
                tp = keep.ctypes.data
        else:
            tp, is_dev = int(transforms), 1
        relay = None
        if hasattr(src_stream, "cuda_stream"):
            s, relay = _source_stream(src_stream)
        else:
            s = src_stream
        keep_p, pp, p_dev = None, None, 0
        if paints is None:
            pass
        elif hasattr(paints, "data_ptr"):
            import torch

            if paints.dtype not in (torch.int32, torch.uint32) or not paints.is_contiguous():
                raise ValueError("paints are a contiguous int32 / uint32 tensor of n * 2 elements (flags, rgba)")
            if n is not None and paints.numel() != n * 2:
                raise ValueError(f"{paints.numel()} words for {n} retained instances (2 each)")
            if paints.is_cuda:
                pp, p_dev = paints.data_ptr(), 1
            else:
                keep_p = paints.numpy()
                pp = keep_p.ctypes.data
        elif isinstance(paints, (int, np.integer)):
            pp, p_dev = int(paints), 1
        else:
            if paints_is_device and not is_emulated(self._lib):
                raise ValueError("a numpy array is host memory: device paints are a tensor on the GPU")
            keep_p = paint_array(paints)
            if n is not None and len(keep_p) != n:
                raise ValueError(f"{len(keep_p)} paints for {n} retained instances")
            # (an empty numpy array still has an address: n == 0 with a paint list is a call with a non-null pointer)
            pp, p_dev = keep_p.ctypes.data, int(bool(paints_is_device))
        stream_arg = ctypes.c_void_p(int(s)) if s else None
        if paints is None:
            r = self._lib.vello_hip_render_retained(self._h, tp, is_dev, stream_arg, ctypes.byref(p), ptr, stride)
        else:
            r = self._lib.vello_hip_render_retained_painted(self._h, tp, is_dev, pp, p_dev, stream_arg, ctypes.byref(p), ptr, stride)
        if relay is not None:
            relay[0].wait_stream(relay[1])
        self._check(r, "render_retained" if paints is None else "render_retained_painted")

    def release_retained(self):
        """vello_hip_release_retained: frees the retained list (fine when there is none)."""
        self._retained_n = None
        self._check(self._lib.vello_hip_release_retained(self._h), "release_retained")

    def pick(self, points, out=None, src_stream=None, points_is_device=None):
        """vello_hip_pick: the topmost draw object and its instance under each point of the frame submitted last (the contract is in
        include/vello_hip.h).  `points`: an (n, 2) float32 numpy array (host memory), or a float32 tensor of n * 2 elements -- on the
        GPU it is read in place, behind `src_stream` (a hipStream_t as an int, or a torch stream) when one is given.
        `points_is_device` says that a numpy array stands for device memory (the emulated build only).  Returns an (n, 2) uint32 numpy
        array of (draw_ix, instance_ix), PICK_NONE where there is none; with `out` -- an (n, 2) uint32 numpy array, or an int32 /
        uint32 tensor of n * 2 elements on the GPU -- the answers are written there and `out` is returned.  Blocks until they are.
        A frame that failed raises VelloHipError with the code vello_hip_sync reports for it in `.code`."""
        numpy_is_device = bool(points_is_device)
        keep, is_dev = None, 0
        if isinstance(points, np.ndarray):
            if numpy_is_device and not is_emulated(self._lib):
                raise ValueError("a numpy array is host memory: device points are a tensor on the GPU")
            keep = np.ascontiguousarray(points, dtype=np.float32)
            pp, n2, is_dev = keep.ctypes.data, keep.size, int(numpy_is_device)
        elif hasattr(points, "data_ptr"):
            import torch

            if points.dtype != torch.float32 or not points.is_contiguous():
                raise ValueError("points are a contiguous float32 tensor of n * 2 elements")
            n2 = points.numel()
            if points.is_cuda:
                pp, is_dev = points.data_ptr(), 1
            else:
                keep = points.numpy()
                pp = keep.ctypes.data
        else:
            raise ValueError("points are an (n, 2) float32 numpy array or a float32 tensor")
        if n2 % 2:
            raise ValueError(f"{n2} floats: points are (x, y) pairs")
        n = n2 // 2
        out_dev = 0
        if out is None:
            out = np.zeros((n, 2), dtype=np.uint32)
        if isinstance(out, np.ndarray):
            if out.dtype != np.uint32 or not out.flags["C_CONTIGUOUS"] or out.size != n2:
                raise ValueError(f"out must be a C-contiguous uint32 array of {n} x 2 entries")
            op = out.ctypes.data
        else:
            if str(out.dtype) not in ("torch.int32", "torch.uint32") or not out.is_contiguous() or out.numel() != n2 or not out.is_cuda:
                raise ValueError(f"out must be a contiguous int32 / uint32 tensor of {n} x 2 entries on the GPU (or a numpy array)")
            op, out_dev = out.data_ptr(), 1
        relay = None
        if hasattr(src_stream, "cuda_stream"):
            s, relay = _source_stream(src_stream)
        else:
            s = src_stream
        r = self._lib.vello_hip_pick(self._h, pp, n, is_dev, ctypes.c_void_p(int(s)) if s else None, op, out_dev)
        if relay is not None:
            relay[0].wait_stream(relay[1])
        self._check(r, "pick")
        return out

    def pick_ms(self):
        """vello_hip_pick_ms: device milliseconds of the last pick's (or pick_rect's) launches, taken while set_profiling has any stage enabled."""
        ms = ctypes.c_float()
        self._check(self._lib.vello_hip_pick_ms(self._h, ctypes.byref(ms)), "pick_ms")
        return float(ms.value)

    def pick_rect_sizes(self):
        """vello_hip_pick_rect_sizes: (draw objects, instances) of the frame submitted last -- the sizes of pick_rect's two outputs;
        0 instances when the frame was not composed from instances."""
        nd, ni = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._lib.vello_hip_pick_rect_sizes(self._h, ctypes.byref(nd), ctypes.byref(ni)), "pick_rect_sizes")
        return int(nd.value), int(ni.value)

    def pick_rect(self, rect, draws_out=None, instances_out=None, draws=True, instances=True, out_is_device=None):
        """vello_hip_pick_rect: marquee selection on the frame submitted last (the contract is in include/vello_hip.h).  `rect` is
        (x0, y0, x1, y1) in target pixels.  Returns (draws, instances, counts): a uint32 word per draw object and per instance --
        REGION_TOUCHED, REGION_ENCLOSED, both or 0 -- and the four totals as a dict.  Without `draws_out` / `instances_out` the words
        come back in new numpy arrays; `draws=False` / `instances=False` leave an output out (None is returned for it), and
        `instances` is None as well for a frame that was not composed from instances.  `draws_out` / `instances_out`: C-contiguous
        uint32 numpy arrays of pick_rect_sizes() entries (host memory), or int32 / uint32 tensors on the GPU, which the kernels write
        in place -- both of one kind; they are returned.  `out_is_device` says that numpy arrays stand for device memory (the emulated
        build only).  Blocks.  A frame that failed raises VelloHipError with the code vello_hip_sync reports for it in `.code`."""
        r4 = np.ascontiguousarray(rect, dtype=np.float32).reshape(-1)
        if r4.size != 4:
            raise ValueError("rect is (x0, y0, x1, y1)")
        n_draw, n_inst = self.pick_rect_sizes()
        if draws_out is None and draws:
            if out_is_device:
                raise ValueError("out_is_device goes with draws_out / instances_out")
            draws_out = np.zeros(n_draw, dtype=np.uint32)
        if instances_out is None and instances and n_inst:
            if out_is_device:
                raise ValueError("out_is_device goes with draws_out / instances_out")
            instances_out = np.zeros(n_inst, dtype=np.uint32)
        kinds, ptrs = set(), []
        for name, o in (("draws_out", draws_out), ("instances_out", instances_out)):
            if o is None:
                ptrs.append((None, 0))
            elif isinstance(o, np.ndarray):
                if o.dtype != np.uint32 or not o.flags["C_CONTIGUOUS"]:
                    raise ValueError(f"{name} must be a C-contiguous uint32 array")
                if out_is_device and not is_emulated(self._lib):
                    raise ValueError("a numpy array is host memory: a device output is a tensor on the GPU")
                kinds.add(bool(out_is_device))
                ptrs.append((o.ctypes.data, o.size))
            else:
                if str(o.dtype) not in ("torch.int32", "torch.uint32") or not o.is_contiguous() or not o.is_cuda:
                    raise ValueError(f"{name} must be a contiguous int32 / uint32 tensor on the GPU (or a numpy array)")
                kinds.add(True)
                ptrs.append((o.data_ptr(), o.numel()))
        if len(kinds) > 1:
            raise ValueError("draws_out and instances_out are both host memory or both device memory")
        counts = RegionCounts()
        r = self._lib.vello_hip_pick_rect(self._h, r4.ctypes.data, ptrs[0][0], ptrs[0][1], ptrs[1][0], ptrs[1][1], int(bool(kinds and kinds.pop())),
                                          ctypes.byref(counts))
        self._check(r, "pick_rect")
        return draws_out, instances_out, counts.as_dict()

    def pick_constants(self):
        """vello_hip_pick_constant: the shapes of the pick's kernels (a test seam) -- lines per workgroup of the line pass, draw objects
        per step of the resolve pass, queries per batch under the pick_small_batches debug flag, bytes of the winding-table budget;
        lines per workgroup of pick_rect's line pass and draw objects per workgroup of its draw pass."""
        names = ("lines_per_workgroup", "draws_per_step", "small_batch", "scratch_bytes", "rect_lines_per_workgroup", "rect_draws_per_workgroup")
        return {k: int(self._lib.vello_hip_pick_constant(i)) for i, k in enumerate(names)}

    STAGE_CONSTANTS = ("pathtag_part_tags", "flatten_block_tags", "draw_part", "clip_part", "draw_workgroup", "coarse_batch", "coarse_grid_bins",
                       "path_count_chunk", "path_count_chunk_small", "path_count_chunk_in_flight", "path_tiling_workgroup", "backdrop_block_tiles",
                       "front_max_tags", "front_max_draw_objects", "front_tiny_segments",
                       "fine_window_words", "fine_batch_fills", "fine_batch_segments", "fine_item_cap", "fine_simple_records", "fine_prefetch_reach",
                       "fine_slice_fills", "fine_slice_min_fills", "fine_slice_min_fills_in_flight", "fine_slice_fills_forced",
                       "fine_slice_min_fills_forced", "fine_heavy_words", "fine_bucket_words", "fine_buckets", "ptcl_initial_alloc",
                       "path_blend_vec_words")

    def stage_constants(self):
        """vello_hip_stage_constant: the sizes at which the pipeline's kernels and the host's launch switches cut their work (a test
        seam; include/vello_hip.h lists them), by name."""
        return {k: int(self._lib.vello_hip_stage_constant(i)) for i, k in enumerate(self.STAGE_CONSTANTS)}

    def path_data_words(self):
        """vello_hip_path_data_words: words of the resident scene's path-data stream (0 when no scene is resident)."""
        return int(self._lib.vello_hip_path_data_words(self._h))

    def upload_path_keyframes(self, keyframes):
        """vello_hip_upload_path_keyframes: K alternative path-data streams of the resident scene -- a [K, N] float32 or uint32 array
        (N = path_data_words(); the words go in bit for bit), or None / an empty list to drop the set.  Waits for the frames in
        flight; a second call replaces the set, an upload of a scene drops it."""
        if keyframes is None or len(keyframes) == 0:
            self._check(self._lib.vello_hip_upload_path_keyframes(self._h, None, 0, self.path_data_words()), "upload_path_keyframes")
            return
        k = np.asarray(keyframes)
        if k.dtype not in (np.dtype(np.float32), np.dtype(np.uint32)):
            raise ValueError("keyframes are float32 or uint32 words")
        if k.ndim == 1:
            k = k.reshape(1, -1)
        if k.ndim != 2:
            raise ValueError("keyframes are a [K, N] array")
        k = np.ascontiguousarray(k)
        self._check(self._lib.vello_hip_upload_path_keyframes(self._h, k.ctypes.data, k.shape[0], k.shape[1]), "upload_path_keyframes")

    def render_resident(self, width, height, base_color, aa, out=None, out_stride=None, morph=None, points=None, src_stream=None,
                        points_is_device=False):
        """vello_hip_render_resident.  `out`: a dense uint8 target of height * width * 4 bytes, or an [H, W, 4] view whose rows lie
        stride(0) bytes apart (_target); `out_stride` (bytes) overrides the stride taken from it.
        `morph` = (src_a, src_b, t) makes it vello_hip_render_resident_morphed: this frame's path-data words are
        A + t * (B - A) in f32 (A verbatim at t == 0 or src_a == src_b, B verbatim at t == 1).  A source is a keyframe index of
        upload_path_keyframes, PATH_DATA_SCENE (the resident scene's own points) or PATH_DATA_DEVICE, which names `points`: a
        float32 tensor of path_data_words() elements on the engine's GPU, or its address as an int -- the host never reads it.
        `points` alone is morph=(PATH_DATA_DEVICE, PATH_DATA_DEVICE, 0).  `points_is_device` says that a numpy array stands for
        device memory (the emulated build only).  `src_stream` (a hipStream_t as an int, or a torch stream) is the stream that
        writes `points`: the frame runs behind it, and it waits for the kernel that reads them."""
        p = self._params(width, height, base_color, aa)
        ptr, stride = None, 0
        if out is not None:
            ptr, stride, _ = _target(self._lib, out, width, height, device_only=True, stride=out_stride)
        if morph is None and points is None and src_stream is None:
            self._check(self._lib.vello_hip_render_resident(self._h, ctypes.byref(p), ptr, stride), "render_resident")
            return
        if morph is None:
            morph = (PATH_DATA_DEVICE, PATH_DATA_DEVICE, 0.0)
        src_a, src_b, t = morph
        keep, pp = None, None
        if points is None:
            pass
        elif isinstance(points, np.ndarray):
            if not (points_is_device and is_emulated(self._lib)):
                raise ValueError("a numpy array is host memory: per-frame points are a tensor on the GPU (a host uploads keyframes)")
            if points.dtype not in (np.dtype(np.float32), np.dtype(np.uint32)):
                raise ValueError("points are float32 words")
            if not points.flags["C_CONTIGUOUS"]:
                raise ValueError("points are contiguous")
            if points.size != self.path_data_words():
                raise ValueError(f"{points.size} floats for a scene of {self.path_data_words()} path-data words")
            keep = points  # (its own address: a slice that starts one float in stays one)
            pp = keep.ctypes.data
        elif hasattr(points, "data_ptr"):
            import torch

            if points.dtype != torch.float32 or not points.is_contiguous() or not points.is_cuda:
                raise ValueError("points are a contiguous float32 tensor on the GPU")
            if points.numel() != self.path_data_words():
                raise ValueError(f"{points.numel()} floats for a scene of {self.path_data_words()} path-data words")
            pp = points.data_ptr()
        else:
            pp = int(points)
        relay = None
        if hasattr(src_stream, "cuda_stream"):
            s, relay = _source_stream(src_stream)
        else:
            s = src_stream
        r = self._lib.vello_hip_render_resident_morphed(self._h, int(src_a) & 0xFFFFFFFF, int(src_b) & 0xFFFFFFFF, ctypes.c_float(float(t)), pp,
                                                        ctypes.c_void_p(int(s)) if s else None, ctypes.byref(p), ptr, stride)
        if relay is not None:
            relay[0].wait_stream(relay[1])
        self._check(r, "render_resident_morphed")

    def render(self, packed, layout, width, height, base_color, aa, ramps=None, out=None, out_stride=None, out_is_device=None):
        """One blocking frame; returns (HxWx4 uint8 image, bump dict).  With `out` (a target as render_resident takes it; a host
        array too) the frame is written there and `out` is returned in the image's place.  `out_stride` overrides the row stride
        taken from `out` (bytes; a host target may have any stride of at least width * 4, an odd one included: pass a flat uint8
        buffer); `out_is_device` says that a numpy array stands for device memory (the emulated build only)."""
        packed = np.ascontiguousarray(packed, dtype=np.uint8)
        lay = LayoutStruct(*layout)
        p = self._params(width, height, base_color, aa)
        if out is None:
            out = np.zeros((height, width, 4), dtype=np.uint8)
        out_ptr, stride, is_dev = _target(self._lib, out, width, height, stride=out_stride)
        if out_is_device:
            if not is_dev and not (isinstance(out, np.ndarray) and is_emulated(self._lib)):
                raise ValueError("out_is_device: the target is not device memory")
            is_dev = True
        b = Bump()
        rp, nr = None, 0
        if ramps is not None and len(ramps):
            ramps = np.ascontiguousarray(ramps, dtype=np.uint32)
            rp, nr = ramps.ctypes.data, ramps.size // 512
        self._retained_n = None  # (its upload drops the retained list)
        r = self._lib.vello_hip_render(self._h, packed.ctypes.data, packed.nbytes, ctypes.byref(lay), ctypes.byref(p), rp, nr,
                                       out_ptr, stride, 1 if is_dev else 0, ctypes.byref(b))
        if r != 0 and r != E_CAPACITY:
            self._check(r, "render")
        return out, b.as_dict()

    def capacities(self):
        c = Capacities()
        self._check(self._lib.vello_hip_get_capacities(self._h, ctypes.byref(c)), "get_capacities")
        return {k: getattr(c, k) for k, _ in Capacities._fields_}

    def grow_pools(self, bump):
        """vello_hip_grow_pools with a bump dict; returns True if any pool grew."""
        b = Bump(*[bump[k] for k, _ in Bump._fields_])
        return self._lib.vello_hip_grow_pools(self._h, ctypes.byref(b), None) == 0

    def set_auto_grow(self, enabled=True):
        self._check(self._lib.vello_hip_set_auto_grow(self._h, 1 if enabled else 0), "set_auto_grow")

    def set_viewport_cull(self, enabled=True):
        """vello_hip_set_viewport_cull: flatten leaves the lines that lie wholly off the target's top, bottom or right side out
        of the soup (bump["lines"] counts the rest); path boxes and everything behind the soup, the image included, are unchanged.
        Applies to frames enqueued after the call."""
        self._check(self._lib.vello_hip_set_viewport_cull(self._h, 1 if enabled else 0), "set_viewport_cull")

    def set_damage_rect(self, rect=None):
        """vello_hip_set_damage_rect: frames enqueued from here on render only the tiles that `rect` ((x0, y0, x1, y1) in pixels,
        half open) touches and write only its pixels; everything ahead of coarse is the whole frame's.  None: whole frames."""
        self._check(self._lib.vello_hip_set_damage_rect(self._h, _damage_words(rect)), "set_damage_rect")

    def set_view_transform(self, view=None):
        """vello_hip_set_view_transform: frames enqueued from here on are rendered as if every transform T of the scene were
        view . T (an Affine, or six floats [m0 m1 m2 m3 t0 t1]); None switches it off.  The resident scene is not modified, and
        frames already enqueued keep the view they were enqueued with."""
        self._check(self._lib.vello_hip_set_view_transform(self._h, _view_floats(view)), "set_view_transform")

    def set_base_image(self, image=None, stride=None, src_stream=None):
        """vello_hip_set_base_image: frames enqueued from here on are drawn over `image` -- one premultiplied RGBA8 word per pixel --
        instead of their base colour; nothing ahead of fine learns about it.  `image`: a torch uint8 [h, w, 4] or int32 [h, w] tensor
        on the engine's GPU (its row stride is taken from the tensor; it may be a slice of a larger one, and it may be the frame's
        target: the frame then draws over what the target holds), or a raw device address with `stride` in bytes (None: width * 4 of
        the frame).  `src_stream` (a hipStream_t as an int, or a torch stream) is the stream that writes the image: the frames' fine
        runs behind the work enqueued on it so far, and it waits for each such frame's fine.  (torch's default stream cannot be
        named through the C ABI: its work so far is relayed through a pool stream, and it is that stream, not the default one, which
        waits for the frames -- pass a side stream where the image is overwritten afterwards.)  None switches it off.  The engine
        keeps no reference to the tensor: the caller keeps it, and a torch stream, alive while the setting stands and until the
        frames have finished."""
        addr, row = _base_image_source(image, stride)
        if hasattr(src_stream, "cuda_stream"):
            s, relay = _source_stream(src_stream)
            self._base_streams = (src_stream, relay)  # (kept alive while the setting stands)
        else:
            s, self._base_streams = src_stream, None
        self._check(self._lib.vello_hip_set_base_image(self._h, addr, row, ctypes.c_void_p(int(s)) if s else None), "set_base_image")

    def set_stroke_scale(self, scale=None, min_width=0.0):
        """vello_hip_set_stroke_scale: frames enqueued from here on are rendered as if every stroke width w > 0 of the scene were
        max(w * scale, min_width), in f32 (a view that zooms by z wants scale = 1 / z for strokes that keep their width on screen);
        scale=None switches it off.  The resident scene is not modified, and frames already enqueued keep their setting."""
        self._check(self._lib.vello_hip_set_stroke_scale(self._h, _stroke_floats(scale, min_width)), "set_stroke_scale")

    def set_debug_flags(self, no_cull=False, stroke_kernel=False, seq_clip=False, fine_slices=False, flatten_coop=False, flatten_alone=False, no_fusion=False,
                        pick_small_batches=False, no_scene_index=False):
        """vello_hip_set_debug_flags: no_cull makes coarse emit every draw (reference-exact PTCL / segments); stroke_kernel
        runs flatten's stroked-line kernel whatever the number of stroked lines; seq_clip matches clips with the one-wave
        stack machine instead of the partitioned kernels; fine_slices cuts every tile's command list into slices of
        4 fills for fine's MSAA modes (normally only lists of >= 96 fills are cut, engine.h FINE_SLICE_MIN_FILLS); flatten_coop /
        flatten_alone pick the kernels of flatten's heavy list (the wave-cooperative walk / every lane on its own) instead of leaving
        the choice to the engine; no_fusion launches every stage of a small scene as a kernel of its own (normally consecutive stages
        up to tile_alloc share launches there); pick_small_batches answers a pick's queries three at a time; no_scene_index renders a resident scene
        without the index its upload built (scene_index_builds): the per-frame scan and whole-stream light pass.  Flags not named are cleared (update_debug_flags keeps them)."""
        self._debug = {"no_cull": bool(no_cull), "stroke_kernel": bool(stroke_kernel), "seq_clip": bool(seq_clip),
                       "fine_slices": bool(fine_slices), "flatten_coop": bool(flatten_coop), "flatten_alone": bool(flatten_alone),
                       "no_fusion": bool(no_fusion), "pick_small_batches": bool(pick_small_batches), "no_scene_index": bool(no_scene_index)}
        d = self._debug
        flags = ((1 if d["no_cull"] else 0) | (2 if d["stroke_kernel"] else 0) | (4 if d["seq_clip"] else 0) | (8 if d["fine_slices"] else 0) |
                 (16 if d["flatten_coop"] else 0) | (32 if d["flatten_alone"] else 0) | (64 if d["no_fusion"] else 0) | (128 if d["pick_small_batches"] else 0) |
                 (256 if d["no_scene_index"] else 0))
        self._check(self._lib.vello_hip_set_debug_flags(self._h, flags), "set_debug_flags")

    def update_debug_flags(self, **changes):
        """set_debug_flags with the flags not named left as they are."""
        d = dict(getattr(self, "_debug", {}))
        d.update(changes)
        self.set_debug_flags(**d)

    def last_render_attempts(self):
        return int(self._lib.vello_hip_last_render_attempts(self._h))

    def fused_launches(self):
        """vello_hip_fused_launches: launches in which stages of a small scene shared a kernel, since the engine was created."""
        return int(self._lib.vello_hip_fused_launches(self._h))

    def scene_allocations(self):
        """vello_hip_scene_allocations: scene buffers allocated since the engine was created."""
        return int(self._lib.vello_hip_scene_allocations(self._h))

    def scene_index_builds(self):
        """vello_hip_scene_index_builds: scene indexes built since the engine was created (one per upload of a scene too large for the
        small-scene launches; frames build none)."""
        return int(self._lib.vello_hip_scene_index_builds(self._h))

    def set_frames_in_flight(self, n):
        self._check(self._lib.vello_hip_set_frames_in_flight(self._h, n), "set_frames_in_flight")
        self.KERNELS = dict(self.KERNELS, flatten=self.FLATTEN_KERNELS[0 if n == 1 else 1])

    def lane_stream_priority(self, lane):
        """vello_hip_lane_stream_priority: (priority of frame lane `lane`'s stream, the device's least priority, its greatest); a
        numerically lower value is a greater priority.  The lanes of a context share one priority, not the default's when the device
        has a range: a pool of hardware queues of their own (VELLO_HIP_DEBUG_LANE_QUEUES=default in the environment: the default's)."""
        p, least, greatest = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        self._check(self._lib.vello_hip_lane_stream_priority(self._h, lane, ctypes.byref(p), ctypes.byref(least), ctypes.byref(greatest)),
                    "lane_stream_priority")
        return p.value, least.value, greatest.value

    def stream(self):
        """vello_hip_get_stream: the hipStream_t (as an int) of the lane that rendered the newest frame."""
        return int(self._lib.vello_hip_get_stream(self._h) or 0)

    def sync_frame(self, age=0):
        self._check(self._lib.vello_hip_sync_frame(self._h, age), "sync_frame")

    def sync(self):
        return self._lib.vello_hip_sync(self._h)

    def bump(self):
        b = Bump()
        self._check(self._lib.vello_hip_get_bump(self._h, ctypes.byref(b)), "get_bump")
        return b.as_dict()

    def run_stages(self, width, height, base_color, aa, first, last):
        p = self._params(width, height, base_color, aa)
        first = STAGES.index(first) if isinstance(first, str) else first
        last = STAGES.index(last) if isinstance(last, str) else last
        self._check(self._lib.vello_hip_run_stages(self._h, ctypes.byref(p), first, last), "run_stages")

    def read_buffer(self, name, dtype=np.uint8, count_bytes=None, offset=0):
        bid = BUFFERS.index(name)
        size = self._lib.vello_hip_buffer_size(self._h, bid)
        n = size - offset if count_bytes is None else min(count_bytes, size - offset)
        out = np.zeros(n, dtype=np.uint8)
        self._check(self._lib.vello_hip_read_buffer(self._h, bid, out.ctypes.data, offset, n), f"read_buffer({name})")
        return out.view(dtype) if n % np.dtype(dtype).itemsize == 0 else out

    def control_words(self):
        """The first 64 words of the last frame's 128-word control block (engine.h Control; the rest are flatten's arc
        sub-list counters): bump allocators, tickets, flatten's list lengths, fine's bucket counters [16:48], slice items [48]
        and coverage-scratch words [49] handed out by coarse."""
        return self.read_buffer("bump", np.uint32, 256)

    def fine_slice_stats(self):
        """(slice items, coverage-scratch words) coarse handed out for the last frame."""
        w = self.control_words()
        return int(w[48]), int(w[49])

    def write_buffer(self, name, data, offset=0):
        bid = BUFFERS.index(name)
        data = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        self._check(self._lib.vello_hip_write_buffer(self._h, bid, data.ctypes.data, offset, data.nbytes), f"write_buffer({name})")

    def set_profiling(self, stages):
        mask = 0
        for s in stages:
            mask |= 1 << (STAGES.index(s) if isinstance(s, str) else s)
        self._lib.vello_hip_set_profiling(self._h, mask)

    def stage_ms(self):
        ms = (ctypes.c_float * len(STAGES))()
        cnt = (ctypes.c_uint32 * len(STAGES))()
        self._check(self._lib.vello_hip_get_stage_ms(self._h, ms, cnt), "get_stage_ms")
        return {STAGES[i]: (ms[i], cnt[i]) for i in range(len(STAGES))}

    # flatten: with one frame in flight the stroked lines' workgroups ride in the heavy list's launch (k_flatten_main) and what
    # they set aside follows (k_flatten_tail); with several, the stroked lines' kernel runs first and the heavy one takes it all
    FLATTEN_KERNELS = (("k_flatten_light", "k_flatten_main", "k_flatten_tail"), ("k_flatten_light", "k_flatten_strokes", "k_flatten_heavy"))
    KERNELS = {"flatten": FLATTEN_KERNELS[0], "coarse": ("k_coarse_prep", "k_coarse")}

    def kernel_ms(self):
        """vello_hip_get_kernel_ms for the stages that are several kernels: {kernel: (summed ms, profiled launches)}."""
        out = {}
        for stage, names in self.KERNELS.items():
            ms = (ctypes.c_float * 3)()
            cnt = ctypes.c_uint32()
            self._check(self._lib.vello_hip_get_kernel_ms(self._h, STAGES.index(stage), ms, ctypes.byref(cnt)), "get_kernel_ms")
            for k, n in enumerate(names):
                out[n] = (ms[k], cnt.value)
        return out


def estimate_capacities(packed, layout, width, height, view=None, stroke=None):
    """vello_hip_estimate_capacities: conservative pool sizes (dict) for a packed scene at a target size (host only); with
    `view` (as Engine.set_view_transform takes it), vello_hip_estimate_capacities_view: for the scene under that view; with
    `stroke` ((scale, min_width), as Engine.set_stroke_scale takes them), vello_hip_estimate_capacities_styled: for the scene
    with its stroke widths under that setting."""
    lib = load_library()
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    lay = LayoutStruct(*layout)
    p = RenderParamsStruct(width, height, 0, 0)
    c = Capacities()
    if stroke is not None:
        r = lib.vello_hip_estimate_capacities_styled(packed.ctypes.data, packed.nbytes, ctypes.byref(lay), ctypes.byref(p), _view_floats(view),
                                                     _stroke_floats(*stroke), ctypes.byref(c))
    elif view is None:
        r = lib.vello_hip_estimate_capacities(packed.ctypes.data, packed.nbytes, ctypes.byref(lay), ctypes.byref(p), ctypes.byref(c))
    else:
        r = lib.vello_hip_estimate_capacities_view(packed.ctypes.data, packed.nbytes, ctypes.byref(lay), ctypes.byref(p), _view_floats(view),
                                                   ctypes.byref(c))
    if r != 0:
        raise VelloHipError(f"vello_hip_estimate_capacities failed ({r})")
    return {k: getattr(c, k) for k, _ in Capacities._fields_}


def gather_frames(engines, src_frames, dst_frames, frame_bytes, dst_device=0, wait=True):
    """vello_hip_gather_frames / vello_hip_gather_wait: the frame each engine (one per GPU, one process) enqueued last is
    copied to dst_frames[i] on dst_device by SDMA peer copies (no CUs).  src / dst: torch tensors or device pointers."""
    lib = load_library()
    n = len(engines)

    def ptr(x):
        return ctypes.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))

    ctxs = (ctypes.c_void_p * n)(*[e._h for e in engines])
    srcs = (ctypes.c_void_p * n)(*[ptr(x) for x in src_frames])
    dsts = (ctypes.c_void_p * n)(*[ptr(x) for x in dst_frames])
    r = lib.vello_hip_gather_frames(ctxs, n, dst_device, srcs, dsts, frame_bytes)
    if r != 0:
        raise VelloHipError(f"vello_hip_gather_frames failed ({r})")
    if wait:
        r = lib.vello_hip_gather_wait(ctxs, n)
        if r != 0:
            raise VelloHipError(f"vello_hip_gather_wait failed ({r})")
