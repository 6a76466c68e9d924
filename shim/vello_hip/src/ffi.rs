//! `extern "C"` mirror of include/vello_hip.h.  Kept in step with the header by tests/test_shim.py (it parses both
//! files and compares every function's name, arity and argument / return types, every struct's fields and every
//! constant).  Pointers to vello_encoding's `Layout` / `BumpAllocators` are passed as the header's own structs: both
//! are `#[repr(C)]` Pod with the same fields (vello_encoding/src/resolve.rs:18-39, config.rs:24-37).
#![allow(non_camel_case_types)]
use core::ffi::{c_char, c_int, c_void};

#[repr(C)]
pub struct vello_hip_ctx {
    _private: [u8; 0],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vello_hip_layout {
    pub n_draw_objects: u32,
    pub n_paths: u32,
    pub n_clips: u32,
    pub bin_data_start: u32,
    pub path_tag_base: u32,
    pub path_data_base: u32,
    pub draw_tag_base: u32,
    pub draw_data_base: u32,
    pub transform_base: u32,
    pub style_base: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vello_hip_render_params {
    pub width: u32,
    pub height: u32,
    pub base_color: u32,
    pub aa: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vello_hip_bump {
    pub failed: u32,
    pub binning: u32,
    pub ptcl: u32,
    pub tile: u32,
    pub seg_counts: u32,
    pub segments: u32,
    pub blend: u32,
    pub lines: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vello_hip_capacities {
    pub lines: u32,
    pub bin_data: u32,
    pub tiles: u32,
    pub seg_counts: u32,
    pub segments: u32,
    pub blend_spill: u32,
    pub ptcl: u32,
}

/// One rectangle of `vello_hip_copy_images_device`: `src` is a device address on the context's GPU.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vello_hip_image_copy {
    pub src: u64,
    pub src_stride: u64,
    pub x: u32,
    pub y: u32,
    pub width: u32,
    pub height: u32,
}

/// Half-open `[begin, end)` ranges of one fragment in the six streams of the resident scene (`vello_hip_upload_fragments`).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vello_hip_fragment {
    pub path_tags: [u32; 2],
    pub path_data: [u32; 2],
    pub draws: [u32; 2],
    pub draw_data: [u32; 2],
    pub transforms: [u32; 2],
    pub styles: [u32; 2],
}

/// One instance of `vello_hip_render_instances`: a fragment index and its transform `[m0 m1 m2 m3 t0 t1]`.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct vello_hip_instance {
    pub fragment: u32,
    pub transform: [f32; 6],
}

/// Per-instance paint of `vello_hip_render_instances_painted`: `rgba` is a premultiplied RGBA8 `DrawColor` word, R in the low byte.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vello_hip_paint {
    pub flags: u32,
    pub rgba: u32,
}

/// One answer of `vello_hip_pick`: the topmost draw object under the point and the instance that owns it, `VELLO_HIP_PICK_NONE`
/// where there is none.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vello_hip_pick_hit {
    pub draw_ix: u32,
    pub instance_ix: u32,
}

/// The four totals of one `vello_hip_pick_rect` call.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct vello_hip_region_counts {
    pub draws_touched: u32,
    pub draws_enclosed: u32,
    pub instances_touched: u32,
    pub instances_enclosed: u32,
}

/// The two bits of a word of `vello_hip_pick_rect`.
pub const VELLO_HIP_REGION_TOUCHED: u32 = 1;
pub const VELLO_HIP_REGION_ENCLOSED: u32 = 2;
/// The header's `#define`s of the same names: no draw object / no instance, and the most points of one `vello_hip_pick` call (4096).
pub const VELLO_HIP_PICK_NONE: u32 = 0xFFFF_FFFF;
pub const VELLO_HIP_PICK_MAX_POINTS: u32 = 0x1000;
pub const VELLO_HIP_PICK_LINES_PER_WORKGROUP: c_int = 0;
pub const VELLO_HIP_PICK_DRAWS_PER_STEP: c_int = 1;
pub const VELLO_HIP_PICK_SMALL_BATCH: c_int = 2;
pub const VELLO_HIP_PICK_SCRATCH_BYTES: c_int = 3;
pub const VELLO_HIP_PICK_RECT_LINES_PER_WORKGROUP: c_int = 4;
pub const VELLO_HIP_PICK_RECT_DRAWS_PER_WORKGROUP: c_int = 5;
/// The header's `#define`s of the same names: the two sources of `vello_hip_render_resident_morphed` that are not keyframe indices.
pub const VELLO_HIP_PATH_DATA_SCENE: u32 = 0xFFFF_FFFF;
pub const VELLO_HIP_PATH_DATA_DEVICE: u32 = 0xFFFF_FFFE;
pub const VELLO_HIP_PAINT_KEEP: u32 = 0;
pub const VELLO_HIP_PAINT_SOLID: u32 = 1;
pub const VELLO_HIP_AA_AREA: u32 = 0;
pub const VELLO_HIP_AA_MSAA8: u32 = 1;
pub const VELLO_HIP_AA_MSAA16: u32 = 2;
pub const VELLO_HIP_AA_MASK_AREA: u32 = 1;
pub const VELLO_HIP_AA_MASK_MSAA8: u32 = 2;
pub const VELLO_HIP_AA_MASK_MSAA16: u32 = 4;
pub const VELLO_HIP_AA_MASK_ALL: u32 = 7;
pub const VELLO_HIP_OK: c_int = 0;
pub const VELLO_HIP_E_INVALID: c_int = -1;
pub const VELLO_HIP_E_HIP: c_int = -2;
pub const VELLO_HIP_E_NO_DEVICE: c_int = -3;
pub const VELLO_HIP_E_CAPACITY: c_int = -4;
pub const VELLO_HIP_E_INTERNAL: c_int = -5;
pub const VELLO_HIP_DEBUG_NO_CULL: u32 = 1;
pub const VELLO_HIP_DEBUG_STROKE_KERNEL: u32 = 2;
pub const VELLO_HIP_DEBUG_SEQ_CLIP: u32 = 4;
pub const VELLO_HIP_DEBUG_FINE_SLICES: u32 = 8;
pub const VELLO_HIP_DEBUG_FLATTEN_COOP: u32 = 16;
pub const VELLO_HIP_DEBUG_FLATTEN_ALONE: u32 = 32;
pub const VELLO_HIP_DEBUG_NO_FUSION: u32 = 64;
pub const VELLO_HIP_DEBUG_PICK_SMALL_BATCHES: u32 = 128;
pub const VELLO_HIP_DEBUG_NO_SCENE_INDEX: u32 = 256;
pub const VELLO_HIP_STAGE_COUNT: usize = 11;

unsafe extern "C" {
    pub fn vello_hip_create(device: c_int, aa_mask: u32, caps: *const vello_hip_capacities, out: *mut *mut vello_hip_ctx) -> c_int;
    pub fn vello_hip_destroy(ctx: *mut vello_hip_ctx);
    pub fn vello_hip_render(ctx: *mut vello_hip_ctx, scene: *const u8, scene_len: usize, layout: *const vello_hip_layout, params: *const vello_hip_render_params, ramps: *const u32, n_ramps: u32, out_rgba8: *mut c_void, out_stride: usize, out_is_device: c_int, bump_out: *mut vello_hip_bump) -> c_int;
    pub fn vello_hip_upload_scene(ctx: *mut vello_hip_ctx, scene: *const u8, scene_len: usize, layout: *const vello_hip_layout, ramps: *const u32, n_ramps: u32) -> c_int;
    pub fn vello_hip_render_resident(ctx: *mut vello_hip_ctx, params: *const vello_hip_render_params, out_device: *mut c_void, out_stride: usize) -> c_int;
    pub fn vello_hip_render_frame(ctx: *mut vello_hip_ctx, scene: *const u8, scene_len: usize, layout: *const vello_hip_layout, params: *const vello_hip_render_params, ramps: *const u32, n_ramps: u32, out_device: *mut c_void, out_stride: usize) -> c_int;
    pub fn vello_hip_upload_fragments(ctx: *mut vello_hip_ctx, scene: *const u8, scene_len: usize, layout: *const vello_hip_layout, ramps: *const u32, n_ramps: u32, frags: *const vello_hip_fragment, n_frags: u32) -> c_int;
    pub fn vello_hip_instances_layout(ctx: *mut vello_hip_ctx, inst: *const vello_hip_instance, n: u32, layout_out: *mut vello_hip_layout, scene_len_out: *mut usize) -> c_int;
    pub fn vello_hip_render_instances(ctx: *mut vello_hip_ctx, inst: *const vello_hip_instance, n: u32, params: *const vello_hip_render_params, out_device: *mut c_void, out_stride: usize) -> c_int;
    pub fn vello_hip_render_instances_painted(ctx: *mut vello_hip_ctx, inst: *const vello_hip_instance, paints: *const vello_hip_paint, n: u32, params: *const vello_hip_render_params, out_device: *mut c_void, out_stride: usize) -> c_int;
    pub fn vello_hip_retain_instances(ctx: *mut vello_hip_ctx, inst: *const vello_hip_instance, paints: *const vello_hip_paint, n: u32) -> c_int;
    pub fn vello_hip_render_retained(ctx: *mut vello_hip_ctx, transforms: *const f32, transforms_is_device: c_int, src_stream: *mut c_void, params: *const vello_hip_render_params, out_device: *mut c_void, out_stride: usize) -> c_int;
    pub fn vello_hip_render_retained_painted(ctx: *mut vello_hip_ctx, transforms: *const f32, transforms_is_device: c_int, paints: *const vello_hip_paint, paints_is_device: c_int, src_stream: *mut c_void, params: *const vello_hip_render_params, out_device: *mut c_void, out_stride: usize) -> c_int;
    pub fn vello_hip_release_retained(ctx: *mut vello_hip_ctx) -> c_int;
    pub fn vello_hip_path_data_words(ctx: *mut vello_hip_ctx) -> u32;
    pub fn vello_hip_upload_path_keyframes(ctx: *mut vello_hip_ctx, words: *const u32, n_keys: u32, n_words: u32) -> c_int;
    pub fn vello_hip_render_resident_morphed(ctx: *mut vello_hip_ctx, src_a: u32, src_b: u32, t: f32, device_words: *const u32, src_stream: *mut c_void, params: *const vello_hip_render_params, out_device: *mut c_void, out_stride: usize) -> c_int;
    pub fn vello_hip_pick(ctx: *mut vello_hip_ctx, points: *const f32, n: u32, points_is_device: c_int, src_stream: *mut c_void, out: *mut vello_hip_pick_hit, out_is_device: c_int) -> c_int;
    pub fn vello_hip_pick_ms(ctx: *mut vello_hip_ctx, ms_out: *mut f32) -> c_int;
    pub fn vello_hip_pick_constant(which: c_int) -> u32;
    pub fn vello_hip_pick_rect_sizes(ctx: *mut vello_hip_ctx, n_draws_out: *mut u32, n_instances_out: *mut u32) -> c_int;
    pub fn vello_hip_pick_rect(ctx: *mut vello_hip_ctx, rect: *const f32, draws_out: *mut u32, n_draws: u32, instances_out: *mut u32, n_instances: u32, out_is_device: c_int, counts_out: *mut vello_hip_region_counts) -> c_int;
    pub fn vello_hip_stage_constant(which: c_int) -> u32;
    pub fn vello_hip_resize_image_atlas(ctx: *mut vello_hip_ctx, width: u32, height: u32) -> c_int;
    pub fn vello_hip_write_image(ctx: *mut vello_hip_ctx, x: u32, y: u32, width: u32, height: u32, rgba8: *const u8, stride: usize) -> c_int;
    pub fn vello_hip_copy_images_device(ctx: *mut vello_hip_ctx, copies: *const vello_hip_image_copy, n: u32, src_stream: *mut c_void) -> c_int;
    pub fn vello_hip_get_capacities(ctx: *mut vello_hip_ctx, out: *mut vello_hip_capacities) -> c_int;
    pub fn vello_hip_grow_pools(ctx: *mut vello_hip_ctx, demand: *const vello_hip_bump, new_caps: *mut vello_hip_capacities) -> c_int;
    pub fn vello_hip_last_render_attempts(ctx: *mut vello_hip_ctx) -> u32;
    pub fn vello_hip_fused_launches(ctx: *mut vello_hip_ctx) -> u64;
    pub fn vello_hip_estimate_capacities(scene: *const u8, scene_len: usize, layout: *const vello_hip_layout, params: *const vello_hip_render_params, out: *mut vello_hip_capacities) -> c_int;
    pub fn vello_hip_set_auto_grow(ctx: *mut vello_hip_ctx, enabled: c_int) -> c_int;
    pub fn vello_hip_set_viewport_cull(ctx: *mut vello_hip_ctx, enabled: c_int) -> c_int;
    pub fn vello_hip_scene_allocations(ctx: *mut vello_hip_ctx) -> u64;
    pub fn vello_hip_scene_index_builds(ctx: *mut vello_hip_ctx) -> u64;
    pub fn vello_hip_set_view_transform(ctx: *mut vello_hip_ctx, view: *const f32) -> c_int;
    pub fn vello_hip_set_damage_rect(ctx: *mut vello_hip_ctx, rect: *const u32) -> c_int;
    pub fn vello_hip_estimate_capacities_view(scene: *const u8, scene_len: usize, layout: *const vello_hip_layout, params: *const vello_hip_render_params, view: *const f32, out: *mut vello_hip_capacities) -> c_int;
    pub fn vello_hip_set_stroke_scale(ctx: *mut vello_hip_ctx, stroke: *const f32) -> c_int;
    pub fn vello_hip_set_base_image(ctx: *mut vello_hip_ctx, image_device: *const c_void, stride: usize, src_stream: *mut c_void) -> c_int;
    pub fn vello_hip_estimate_capacities_styled(scene: *const u8, scene_len: usize, layout: *const vello_hip_layout, params: *const vello_hip_render_params, view: *const f32, stroke: *const f32, out: *mut vello_hip_capacities) -> c_int;
    pub fn vello_hip_set_debug_flags(ctx: *mut vello_hip_ctx, flags: u32) -> c_int;
    pub fn vello_hip_set_frames_in_flight(ctx: *mut vello_hip_ctx, n: u32) -> c_int;
    pub fn vello_hip_lane_stream_priority(ctx: *mut vello_hip_ctx, lane: u32, priority: *mut c_int, device_least: *mut c_int, device_greatest: *mut c_int) -> c_int;
    pub fn vello_hip_sync_frame(ctx: *mut vello_hip_ctx, age: u32) -> c_int;
    pub fn vello_hip_sync(ctx: *mut vello_hip_ctx) -> c_int;
    pub fn vello_hip_get_bump(ctx: *mut vello_hip_ctx, out: *mut vello_hip_bump) -> c_int;
    pub fn vello_hip_get_stream(ctx: *mut vello_hip_ctx) -> *mut c_void;
    pub fn vello_hip_gather_frames(ctxs: *const *mut vello_hip_ctx, n: u32, dst_device: c_int, src_frames: *const *const c_void, dst_frames: *const *mut c_void, frame_bytes: usize) -> c_int;
    pub fn vello_hip_gather_wait(ctxs: *const *mut vello_hip_ctx, n: u32) -> c_int;
    pub fn vello_hip_run_stages(ctx: *mut vello_hip_ctx, params: *const vello_hip_render_params, first_stage: c_int, last_stage: c_int) -> c_int;
    pub fn vello_hip_read_buffer(ctx: *mut vello_hip_ctx, buf_id: c_int, dst: *mut c_void, offset: usize, size: usize) -> c_int;
    pub fn vello_hip_write_buffer(ctx: *mut vello_hip_ctx, buf_id: c_int, src: *const c_void, offset: usize, size: usize) -> c_int;
    pub fn vello_hip_buffer_size(ctx: *mut vello_hip_ctx, buf_id: c_int) -> usize;
    pub fn vello_hip_set_profiling(ctx: *mut vello_hip_ctx, stage_mask: u32) -> c_int;
    pub fn vello_hip_get_stage_ms(ctx: *mut vello_hip_ctx, ms_out: *mut f32, count_out: *mut u32) -> c_int;
    pub fn vello_hip_get_kernel_ms(ctx: *mut vello_hip_ctx, stage: c_int, ms_out: *mut f32, count_out: *mut u32) -> c_int;
    pub fn vello_hip_stage_name(stage: c_int) -> *const c_char;
    pub fn vello_hip_last_error(ctx: *mut vello_hip_ctx) -> *const c_char;
    pub fn vello_hip_make_mask_lut(out: *mut u8);
    pub fn vello_hip_make_mask_lut_16(out: *mut u8);
}
