"""ctypes loader for libvello_hip.so (built in-tree by __graft_entry__.build / csrc/Makefile)."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_LIB_PATH_OVERRIDE = None


class VelloHipError(RuntimeError):
    pass


def library_path():
    return _LIB_PATH_OVERRIDE or os.path.join(_HERE, "lib", "libvello_hip.so")


def _use_library(path):
    """Test hook: point the bindings at another build of the same sources (tests/simt_emu)."""
    global _LIB, _LIB_PATH_OVERRIDE
    _LIB = None
    _LIB_PATH_OVERRIDE = path


def is_emulated(lib):
    """True for the SIMT-emulated build of the kernel sources that the CPU tests load through _use_library (tests/simt_emu): device
    memory is host memory there, so a numpy array may stand for a device target.  Told by an entry point only that build has."""
    return hasattr(lib, "simt_emu_switch")


class Capacities(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("lines", "bin_data", "tiles", "seg_counts", "segments", "blend_spill", "ptcl")]


class Bump(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("failed", "binning", "ptcl", "tile", "seg_counts", "segments", "blend", "lines")]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class LayoutStruct(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in (
        "n_draw_objects", "n_paths", "n_clips", "bin_data_start", "path_tag_base", "path_data_base",
        "draw_tag_base", "draw_data_base", "transform_base", "style_base")]


class RenderParamsStruct(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in ("width", "height", "base_color", "aa")]


class ImageCopyStruct(ctypes.Structure):  # vello_hip_image_copy
    _fields_ = [("src", ctypes.c_uint64), ("src_stride", ctypes.c_uint64)] + [(n, ctypes.c_uint32) for n in ("x", "y", "width", "height")]


class FragmentStruct(ctypes.Structure):  # vello_hip_fragment: half-open [begin, end) ranges into the six streams
    _fields_ = [(n, ctypes.c_uint32 * 2) for n in ("path_tags", "path_data", "draws", "draw_data", "transforms", "styles")]


class InstanceStruct(ctypes.Structure):  # vello_hip_instance
    _fields_ = [("fragment", ctypes.c_uint32), ("transform", ctypes.c_float * 6)]


class PaintStruct(ctypes.Structure):  # vello_hip_paint
    _fields_ = [("flags", ctypes.c_uint32), ("rgba", ctypes.c_uint32)]


class RegionCounts(ctypes.Structure):  # vello_hip_region_counts
    _fields_ = [(n, ctypes.c_uint32) for n in ("draws_touched", "draws_enclosed", "instances_touched", "instances_enclosed")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


def load_library():
    """Loads the product library; raises (never falls back) when it is missing."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise VelloHipError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). vello_amd has no CPU fallback.")
    # PyTorch-ROCm bundles its own libamdhip64 (same SONAME as /opt/rocm's).  Whichever copy is mapped first
    # serves the whole process, and torch cannot initialise on a foreign copy -> let torch map its runtime first.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    c = ctypes
    vp, u32, sz, i32 = c.c_void_p, c.c_uint32, c.c_size_t, c.c_int

    def sig(name, res, args):
        try:
            f = getattr(lib, name)
        except AttributeError:
            # an OLDER build of the library under the _use_library hook (same-box A/B against an earlier commit, scripts/ab_*.py)
            # may lack a later entry point; the product library must have them all
            if _LIB_PATH_OVERRIDE is not None and os.sep + "ab_tmp" + os.sep in _LIB_PATH_OVERRIDE:
                return
            raise
        f.restype = res
        f.argtypes = args

    # include/vello_hip.h
    sig("vello_hip_create", i32, [i32, u32, c.POINTER(Capacities), c.POINTER(vp)])
    sig("vello_hip_destroy", None, [vp])
    sig("vello_hip_render", i32, [vp, vp, sz, c.POINTER(LayoutStruct), c.POINTER(RenderParamsStruct), vp, u32, vp, sz, i32, c.POINTER(Bump)])
    sig("vello_hip_upload_scene", i32, [vp, vp, sz, c.POINTER(LayoutStruct), vp, u32])
    sig("vello_hip_render_frame", i32, [vp, vp, sz, c.POINTER(LayoutStruct), c.POINTER(RenderParamsStruct), vp, u32, vp, sz])
    sig("vello_hip_render_resident", i32, [vp, c.POINTER(RenderParamsStruct), vp, sz])
    sig("vello_hip_upload_fragments", i32, [vp, vp, sz, c.POINTER(LayoutStruct), vp, u32, c.POINTER(FragmentStruct), u32])
    sig("vello_hip_instances_layout", i32, [vp, vp, u32, c.POINTER(LayoutStruct), c.POINTER(sz)])
    sig("vello_hip_render_instances", i32, [vp, vp, u32, c.POINTER(RenderParamsStruct), vp, sz])
    sig("vello_hip_render_instances_painted", i32, [vp, vp, vp, u32, c.POINTER(RenderParamsStruct), vp, sz])
    sig("vello_hip_retain_instances", i32, [vp, vp, vp, u32])
    sig("vello_hip_render_retained", i32, [vp, vp, i32, vp, c.POINTER(RenderParamsStruct), vp, sz])
    sig("vello_hip_render_retained_painted", i32, [vp, vp, i32, vp, i32, vp, c.POINTER(RenderParamsStruct), vp, sz])
    sig("vello_hip_release_retained", i32, [vp])
    sig("vello_hip_path_data_words", u32, [vp])
    sig("vello_hip_upload_path_keyframes", i32, [vp, vp, u32, u32])
    sig("vello_hip_render_resident_morphed", i32, [vp, u32, u32, c.c_float, vp, vp, c.POINTER(RenderParamsStruct), vp, sz])
    sig("vello_hip_pick", i32, [vp, vp, u32, i32, vp, vp, i32])
    sig("vello_hip_pick_constant", u32, [i32])
    sig("vello_hip_pick_rect_sizes", i32, [vp, c.POINTER(u32), c.POINTER(u32)])
    sig("vello_hip_pick_rect", i32, [vp, vp, vp, u32, vp, u32, i32, c.POINTER(RegionCounts)])
    sig("vello_hip_stage_constant", u32, [i32])
    sig("vello_hip_pick_ms", i32, [vp, c.POINTER(c.c_float)])
    sig("vello_hip_set_frames_in_flight", i32, [vp, u32])
    sig("vello_hip_lane_stream_priority", i32, [vp, u32, c.POINTER(i32), c.POINTER(i32), c.POINTER(i32)])
    sig("vello_hip_resize_image_atlas", i32, [vp, u32, u32])
    sig("vello_hip_write_image", i32, [vp, u32, u32, u32, u32, vp, sz])
    sig("vello_hip_copy_images_device", i32, [vp, c.POINTER(ImageCopyStruct), u32, vp])
    sig("vello_hip_get_capacities", i32, [vp, c.POINTER(Capacities)])
    sig("vello_hip_grow_pools", i32, [vp, c.POINTER(Bump), c.POINTER(Capacities)])
    sig("vello_hip_set_auto_grow", i32, [vp, i32])
    sig("vello_hip_set_viewport_cull", i32, [vp, i32])
    sig("vello_hip_set_view_transform", i32, [vp, c.POINTER(c.c_float)])
    sig("vello_hip_set_damage_rect", i32, [vp, c.POINTER(u32)])
    sig("vello_hip_set_debug_flags", i32, [vp, u32])
    sig("vello_hip_last_render_attempts", u32, [vp])
    sig("vello_hip_fused_launches", ctypes.c_uint64, [vp])
    sig("vello_hip_scene_allocations", ctypes.c_uint64, [vp])
    sig("vello_hip_scene_index_builds", ctypes.c_uint64, [vp])
    sig("vello_hip_estimate_capacities", i32, [vp, sz, c.POINTER(LayoutStruct), c.POINTER(RenderParamsStruct), c.POINTER(Capacities)])
    sig("vello_hip_estimate_capacities_view", i32, [vp, sz, c.POINTER(LayoutStruct), c.POINTER(RenderParamsStruct), c.POINTER(c.c_float),
                                               c.POINTER(Capacities)])
    sig("vello_hip_set_stroke_scale", i32, [vp, c.POINTER(c.c_float)])
    sig("vello_hip_set_base_image", i32, [vp, vp, sz, vp])
    sig("vello_hip_estimate_capacities_styled", i32, [vp, sz, c.POINTER(LayoutStruct), c.POINTER(RenderParamsStruct), c.POINTER(c.c_float),
                                                 c.POINTER(c.c_float), c.POINTER(Capacities)])
    sig("vello_hip_gather_frames", i32, [c.POINTER(vp), u32, i32, c.POINTER(vp), c.POINTER(vp), sz])
    sig("vello_hip_gather_wait", i32, [c.POINTER(vp), u32])
    sig("vello_hip_sync_frame", i32, [vp, u32])
    sig("vello_hip_sync", i32, [vp])
    sig("vello_hip_get_bump", i32, [vp, c.POINTER(Bump)])
    sig("vello_hip_get_stream", vp, [vp])
    sig("vello_hip_run_stages", i32, [vp, c.POINTER(RenderParamsStruct), i32, i32])
    sig("vello_hip_read_buffer", i32, [vp, i32, vp, sz, sz])
    sig("vello_hip_write_buffer", i32, [vp, i32, vp, sz, sz])
    sig("vello_hip_buffer_size", sz, [vp, i32])
    sig("vello_hip_set_profiling", i32, [vp, u32])
    sig("vello_hip_get_stage_ms", i32, [vp, c.POINTER(c.c_float), c.POINTER(u32)])
    sig("vello_hip_get_kernel_ms", i32, [vp, i32, c.POINTER(c.c_float), c.POINTER(u32)])
    sig("vello_hip_stage_name", c.c_char_p, [i32])
    sig("vello_hip_last_error", c.c_char_p, [vp])
    sig("vello_hip_make_mask_lut", None, [vp])
    sig("vello_hip_make_mask_lut_16", None, [vp])
    # host mirror (harness glue)
    dp = c.POINTER(c.c_double)
    fp = c.POINTER(c.c_float)
    sig("vh_bezpath_free", None, [vp])
    sig("vh_bezpath_from_svg", vp, [c.c_char_p])
    sig("vh_bezpath_circle", vp, [c.c_double] * 4)
    sig("vh_bezpath_rect", vp, [c.c_double] * 4)
    sig("vh_bezpath_rounded_rect", vp, [c.c_double] * 6)
    sig("vh_bezpath_line", vp, [c.c_double] * 4)
    sig("vh_bezpath_n_verbs", sz, [vp])
    sig("vh_bezpath_n_coords", sz, [vp])
    sig("vh_bezpath_copy", None, [vp, vp, vp])
    sig("vh_scene_new", vp, [])
    sig("vh_scene_free", None, [vp])
    sig("vh_scene_reset", None, [vp])
    sig("vh_scene_fill", None, [vp, i32, dp, fp, vp, vp, sz])
    sig("vh_scene_stroke", i32, [vp, c.c_double, i32, c.c_double, i32, i32, dp, fp, vp, vp, sz])
    sig("vh_scene_push_layer", None, [vp, i32, u32, u32, c.c_float, dp, vp, vp, sz])
    sig("vh_scene_push_luminance_mask_layer", None, [vp, i32, c.c_float, dp, vp, vp, sz])
    sig("vh_scene_push_clip_layer", None, [vp, i32, dp, vp, vp, sz])
    sig("vh_scene_push_layer_stroked", i32, [vp, i32, c.c_double, i32, c.c_double, i32, i32, u32, u32, c.c_float, dp, vp, vp, sz])
    sig("vh_scene_pop_layer", None, [vp])
    sig("vh_scene_append", None, [vp, vp, dp])
    sig("vh_brush_solid", vp, [fp])
    sig("vh_brush_gradient", vp, [i32, dp, u32, u32, fp, sz])
    sig("vh_brush_image", vp, [c.c_uint64, u32, u32, u32, u32, vp, u32, u32, u32, c.c_float])
    sig("vh_brush_free", None, [vp])
    sig("vh_scene_fill_brush", None, [vp, i32, dp, vp, dp, vp, vp, sz])
    sig("vh_scene_stroke_brush", i32, [vp, c.c_double, i32, c.c_double, i32, i32, dp, vp, dp, vp, vp, sz])
    sig("vh_scene_draw_blurred_rounded_rect", None, [vp, dp, dp, fp, c.c_double, c.c_double])
    sig("vh_scene_draw_blurred_rounded_rect_in", None, [vp, vp, vp, sz, dp, dp, fp, c.c_double, c.c_double])
    sig("vh_scene_draw_image", None, [vp, vp, dp])
    sig("vh_scene_n_patches", sz, [vp])
    sig("vh_resolver_new", vp, [])
    sig("vh_resolver_new_with_atlas_sizes", vp, [u32, u32])
    sig("vh_resolver_free", None, [vp])
    sig("vh_resolver_resolve", sz, [vp, vp, c.POINTER(vp), c.POINTER(u32), c.POINTER(vp), c.POINTER(u32)])
    sig("vh_resolver_upload", vp, [vp, u32, c.POINTER(u32)])
    sig("vh_resolver_upload_id", c.c_uint64, [vp, u32])
    sig("vh_resolver_mark_image_dirty", None, [vp, c.c_uint64])
    sig("vh_resolver_image_cache_info", None, [vp, c.POINTER(u32)])
    sig("vh_scene_stream_bytes", sz, [vp, i32])
    sig("vh_scene_stream_copy", None, [vp, i32, vp])
    sig("vh_scene_counts", None, [vp, c.POINTER(u32)])
    sig("vh_scene_resolve", sz, [vp, c.POINTER(vp), c.POINTER(u32)])
    sig("vh_f32_to_f16", c.c_uint16, [c.c_float])
    sig("vh_f16_to_f32", c.c_float, [c.c_uint16])
    sig("vh_color_premul_rgba8", u32, [fp])
    sig("vh_style_from_stroke", None, [c.c_double, i32, c.c_double, i32, i32, c.POINTER(u32)])
    sig("vh_renderer_new", vp, [i32, u32, c.POINTER(Capacities), c.c_char_p, sz])
    sig("vh_renderer_free", None, [vp])
    sig("vh_renderer_render_to_texture", i32, [vp, vp, vp, sz, i32, u32, u32, fp, u32])
    sig("vh_renderer_render_to_texture_on", i32, [vp, vp, vp, sz, i32, u32, u32, fp, u32, vp])
    sig("vh_renderer_render_to_texture_view", i32, [vp, vp, vp, sz, i32, u32, u32, fp, u32, vp, fp])
    sig("vh_renderer_override_image", i32, [vp, c.c_uint64, i32, c.c_uint64, c.c_uint64, c.POINTER(c.c_uint64)])
    sig("vh_renderer_mark_override_image_dirty", None, [vp, c.c_uint64])
    sig("vh_renderer_error", c.c_char_p, [vp])
    sig("vh_renderer_engine", vp, [vp])
    sig("vh_renderer_last_bump", None, [vp, c.POINTER(Bump)])
    _LIB = lib
    return lib


def kernel_sources_hash():
    """sha1 over what the kernel objects are built from: what a profile or a PMC pass says it measured.  A commit hash moves with
    every documentation commit and does not exist on the GPU box; this says whether the KERNELS are the ones the numbers came
    from (bench.py: roofline.traffic_stale)."""
    import hashlib
    import os

    here = os.path.dirname(os.path.abspath(__file__))
    root = os.path.join(here, "csrc")
    engine = os.path.join(root, "engine")
    # the Makefile and sources.mk, the KERNELS sources sources.mk names, every header they may include (engine/*.h, *.inc) and the
    # public header with the layout / config / flag types the kernels use -- nothing that is not built (no stray files, no backups)
    with open(os.path.join(root, "sources.mk")) as fh:
        kernels = next(line.split("=", 1)[1].split() for line in fh if line.split("=", 1)[0].strip() == "KERNELS")
    files = [os.path.join(root, "Makefile"), os.path.join(root, "sources.mk")]
    files += [os.path.join(engine, k + ".hip") for k in kernels]
    files += sorted(os.path.join(engine, f) for f in os.listdir(engine) if f.endswith((".h", ".inc")))
    h = hashlib.sha1()
    for f in files:
        with open(f, "rb") as fh:
            h.update(os.path.basename(f).encode())
            h.update(fh.read())
    header = os.path.join(os.path.dirname(here), "include", "vello_hip.h")
    if os.path.isfile(header):
        with open(header, "rb") as fh:
            h.update(b"vello_hip.h")
            h.update(fh.read())
    else:  # (a layout without the repository's include/: still a hash, and not one of a tree that has the header)
        h.update(b"vello_hip.h: absent")
    return h.hexdigest()[:12]
