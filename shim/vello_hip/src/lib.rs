//! `HipRenderer`: the `vello::Renderer` surface (vello/src/lib.rs:432-515) over libvello_hip.so.
//!
//! Everything above the seam is vello's own host code and runs unchanged: `Scene` -> `Encoding` ->
//! `Resolver::resolve` (packed scene bytes, `Layout`, gradient `Ramps`, `Images`).  Where `Renderer::render_to_texture`
//! turns those into a `Recording` for `WgpuEngine::run_recording` (vello/src/render.rs:84-112,
//! vello/src/wgpu_engine.rs:380-777), `HipRenderer::render_to_buffer` hands them to the C ABI.
//!
//! SOURCE ONLY: no Rust toolchain exists in the build image; see Cargo.toml.
pub mod ffi;

use core::ffi::{c_int, c_void, CStr};
use ffi::*;
use std::collections::HashMap;
use vello::{AaConfig, AaSupport, RenderParams, Scene};
use vello::peniko::ImageData;
use vello::kurbo::Affine;
use vello_encoding::{Layout, Resolver, Transform};

#[derive(Debug)]
pub enum Error {
    /// vello::Error::NoCompatibleDevice (vello/src/lib.rs:262): no gfx950 device; there is no CPU fallback.
    NoCompatibleDevice,
    /// An AA mode that was not enabled in the `AaSupport` given to `new` (render.rs:566-598 panics upstream),
    /// or a packed scene whose streams contradict each other.
    Invalid(String),
    /// A HIP runtime error.
    Hip(String),
    /// A bump-allocated pool overflowed and auto-grow is off: the target is untouched (fine.wgsl:1070-1074); the
    /// counters say what the frame needs (`HipRenderer::grow_pools`).
    Capacity(vello_hip_bump),
    /// An engine-internal wait gave up (a look-back or grid barrier whose partner never arrived): the frame is discarded.
    Internal(String),
}

/// What `override_image` binds to an image in place of its pixels -- upstream a `wgpu::TexelCopyTextureInfoBase<Texture>`
/// (vello/src/lib.rs:536-545), here a device address on the renderer's GPU: `src` points at the texel of the image's
/// origin, rows of RGBA8 words `stride` bytes apart (0 = width * 4).  The caller keeps the memory alive while it is bound.
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub struct DeviceTexture {
    pub src: u64,
    pub stride: u64,
}

pub struct HipRenderer {
    ctx: *mut vello_hip_ctx,
    resolver: Resolver,
    packed: Vec<u8>,
    atlas_size: (u32, u32),
    /// `WgpuEngine::image_overrides` (vello/src/wgpu_engine.rs:486-504): blob id -> device source
    overrides: HashMap<u64, DeviceTexture>,
}
// Renderer: Send, !Sync (vello/src/lib.rs:351-352): a context is single-threaded, different contexts are independent
unsafe impl Send for HipRenderer {}

fn to_hip_layout(l: &Layout) -> vello_hip_layout {
    vello_hip_layout {
        n_draw_objects: l.n_draw_objects,
        n_paths: l.n_paths,
        n_clips: l.n_clips,
        bin_data_start: l.bin_data_start,
        path_tag_base: l.path_tag_base,
        path_data_base: l.path_data_base,
        draw_tag_base: l.draw_tag_base,
        draw_data_base: l.draw_data_base,
        transform_base: l.transform_base,
        style_base: l.style_base,
    }
}

impl HipRenderer {
    /// `Renderer::new` (vello/src/lib.rs:432-459).  Takes the one field of `RendererOptions` that means something here --
    /// `antialiasing_support` -- as an `AaSupport`: `RendererOptions` itself is `#[cfg(feature = "wgpu")]`
    /// (vello/src/lib.rs:371-373) and this crate depends on vello WITHOUT that feature (no wgpu in the build at all);
    /// `use_cpu`, `num_init_threads` and `pipeline_cache` configure wgpu's shader compilation.
    pub fn new(device: i32, aa: AaSupport) -> Result<Self, Error> {
        let mask = (aa.area as u32) * VELLO_HIP_AA_MASK_AREA
            | (aa.msaa8 as u32) * VELLO_HIP_AA_MASK_MSAA8
            | (aa.msaa16 as u32) * VELLO_HIP_AA_MASK_MSAA16;
        let mut ctx = core::ptr::null_mut();
        let rc = unsafe { vello_hip_create(device as c_int, mask, core::ptr::null(), &mut ctx) };
        if rc != VELLO_HIP_OK {
            return Err(Error::NoCompatibleDevice);
        }
        // the robust path upstream is a TODO (lib.rs:753-764); here a frame that overflows grows the pools and re-runs
        unsafe { vello_hip_set_auto_grow(ctx, 1) };
        Ok(Self { ctx, resolver: Resolver::new(), packed: Vec::new(), atlas_size: (0, 0), overrides: HashMap::new() })
    }

    /// `vello_hip_set_viewport_cull`: flatten leaves the lines that lie wholly off the target's top, bottom or right side out
    /// of the line soup (the image does not change; `include/vello_hip.h` has the rule).  Off by default; applies to the
    /// frames rendered after the call.
    pub fn set_viewport_cull(&mut self, enabled: bool) {
        unsafe { vello_hip_set_viewport_cull(self.ctx, enabled as c_int) };
    }

    /// `vello_hip_set_view_transform`: the frames rendered after the call show the scene as `Scene::append(scene, Some(view))`
    /// would have encoded it -- the engine composes `view` in front of every transform of the packed scene on the GPU, in f32 as
    /// `Transform::mul` does (`include/vello_hip.h` has the contract).  `None` switches it off.  A view with a NaN or infinite
    /// coefficient is refused and changes nothing.
    pub fn set_view_transform(&mut self, view: Option<Affine>) -> Result<(), Error> {
        let rc = match view {
            Some(affine) => {
                let t = Transform::from_kurbo(&affine);
                let v: [f32; 6] = [t.matrix[0], t.matrix[1], t.matrix[2], t.matrix[3], t.translation[0], t.translation[1]];
                unsafe { vello_hip_set_view_transform(self.ctx, v.as_ptr()) }
            }
            None => unsafe { vello_hip_set_view_transform(self.ctx, core::ptr::null()) },
        };
        if rc == VELLO_HIP_OK { Ok(()) } else { Err(Self::error(self.ctx, rc, vello_hip_bump::default())) }
    }

    /// `Renderer::override_image` (vello/src/lib.rs:536-545): whenever the resolver schedules `image` for upload, its texels
    /// are copied from `texture` (device to atlas, batched with the frame's other overrides) instead of its blob; `None`
    /// removes the override.  Marks the image dirty; returns the previous source.
    pub fn override_image(&mut self, image: &ImageData, texture: Option<DeviceTexture>) -> Option<DeviceTexture> {
        self.resolver.mark_image_dirty(image);
        match texture {
            Some(texture) => self.overrides.insert(image.data.id(), texture),
            None => self.overrides.remove(&image.data.id()),
        }
    }

    /// `Renderer::mark_override_image_dirty` (vello/src/lib.rs:547-555): the source's contents changed.
    pub fn mark_override_image_dirty(&mut self, image: &ImageData) {
        self.resolver.mark_image_dirty(image);
    }

    /// What a failed call left in the context.  A free function over the raw context pointer (not `&self`): it is called
    /// while `render_to_buffer` still holds the `Ramps` / `Images` that `Resolver::resolve` lends out of `self.resolver`
    /// (`resolve<'a>(&'a mut self, ..) -> (Layout, Ramps<'a>, Images<'a>)`, vello_encoding/src/resolve.rs:183-187).
    fn error(ctx: *mut vello_hip_ctx, rc: c_int, bump: vello_hip_bump) -> Error {
        let msg = unsafe { CStr::from_ptr(vello_hip_last_error(ctx)) }.to_string_lossy().into_owned();
        match rc {
            VELLO_HIP_E_NO_DEVICE => Error::NoCompatibleDevice,
            VELLO_HIP_E_INVALID => Error::Invalid(msg),
            VELLO_HIP_E_CAPACITY => Error::Capacity(bump),
            VELLO_HIP_E_INTERNAL => Error::Internal(msg),
            _ => Error::Hip(msg),
        }
    }

    /// `Renderer::render_to_texture` (vello/src/lib.rs:474-515) into a caller-owned linear RGBA8 buffer (host memory, or
    /// device memory of the context's GPU): un-premultiplied, rows of `stride` bytes, origin top-left.
    /// The target (include/vello_hip.h, at `vello_hip_render_resident`): on the device, `target` and `stride` are multiples of 4
    /// and `stride` is 0 (= width * 4) or width * 4 <= stride < 2^32; on the host any alignment, `stride` 0 or >= width * 4.
    /// Exactly the bytes [y * stride, y * stride + width * 4) of each row y < height are written and no other byte; a target
    /// that breaks this is `Error::Invalid` before anything is uploaded or enqueued.
    pub fn render_to_buffer(&mut self, scene: &Scene, target: *mut c_void, stride: usize, on_device: bool,
                            params: &RenderParams) -> Result<(), Error> {
        // identical to Render::render_encoding_coarse up to the uploads (vello/src/render.rs:135-232).
        // Borrows: `resolve` borrows `self.resolver` mutably for as long as `ramps` / `images` live, and `self.packed`
        // for the call only.  Everything below therefore touches `self` through DISJOINT fields (`self.ctx`, a `Copy`
        // raw pointer read once up front; `self.atlas_size`; `self.packed`; `self.overrides`, lent out before the resolve) and
        // never through a `&self` / `&mut self` method, which would borrow all of `self` while the resolver is lent out (E0502).
        let ctx = self.ctx;
        // (a shared loan of the `overrides` field, disjoint from the resolver's)
        let overrides = &self.overrides;
        let (layout, ramps, images) = self.resolver.resolve(scene.encoding(), &mut self.packed);
        // `images.images: &[(ImageData, u32, u32)]` (vello_encoding/src/image_cache.rs:24): iterate by reference.  An image
        // with neither an override nor pixels is refused before anything is enqueued (wgpu_engine.rs:505-514 panics); the
        // frame's images are kept (cheap clones: a blob is an Arc) to be marked dirty again once the resolver's loans end.
        let refused: Option<(u64, Vec<ImageData>)> = images
            .images
            .iter()
            .find(|(image, _, _)| {
                overrides.get(&image.data.id()).is_none() && image.data.data().is_empty() && image.width != 0 && image.height != 0
            })
            .map(|(image, _, _)| (image.data.id(), images.images.iter().map(|(im, _, _)| im.clone()).collect()));
        let rc;
        let mut bump = vello_hip_bump::default();
        if refused.is_some() {
            rc = VELLO_HIP_E_INVALID;
        } else {
            // vello/src/render.rs:160-203: the persistent image atlas follows the Resolver's image cache
            if (images.width, images.height) != self.atlas_size {
                let rc = unsafe { vello_hip_resize_image_atlas(ctx, images.width, images.height) };
                if rc != VELLO_HIP_OK {
                    return Err(Self::error(ctx, rc, vello_hip_bump::default()));
                }
                self.atlas_size = (images.width, images.height);
            }
            // overrides: ONE device-to-atlas batch (wgpu_engine.rs:486-504 copies texture to texture per image); blobs: host writes
            let mut copies: Vec<vello_hip_image_copy> = Vec::new();
            for (image, x, y) in images.images.iter() {
                if let Some(t) = overrides.get(&image.data.id()) {
                    copies.push(vello_hip_image_copy { src: t.src, src_stride: t.stride, x: *x, y: *y, width: image.width, height: image.height });
                    continue;
                }
                let bytes: &[u8] = image.data.data();
                let rc = unsafe { vello_hip_write_image(ctx, *x, *y, image.width, image.height, bytes.as_ptr(), 0) };
                if rc != VELLO_HIP_OK {
                    return Err(Self::error(ctx, rc, vello_hip_bump::default()));
                }
            }
            if !copies.is_empty() {
                let rc = unsafe { vello_hip_copy_images_device(ctx, copies.as_ptr(), copies.len() as u32, core::ptr::null_mut()) };
                if rc != VELLO_HIP_OK {
                    return Err(Self::error(ctx, rc, vello_hip_bump::default()));
                }
            }
            let p = vello_hip_render_params {
                width: params.width,
                height: params.height,
                base_color: params.base_color.premultiply().to_rgba8().to_u32(), // vello_encoding/src/config.rs:183
                aa: match params.antialiasing_method {
                    AaConfig::Area => VELLO_HIP_AA_AREA,
                    AaConfig::Msaa8 => VELLO_HIP_AA_MSAA8,
                    AaConfig::Msaa16 => VELLO_HIP_AA_MSAA16,
                },
            };
            let hl = to_hip_layout(&layout);
            // `Ramps { data: &[u32], width, height }` is `Copy` (ramp_cache.rs:16-21); an empty slice's pointer is dangling but
            // non-null and is never read (n_ramps = 0)
            rc = unsafe {
                vello_hip_render(ctx, self.packed.as_ptr(), self.packed.len(), &hl, &p, ramps.data.as_ptr(), ramps.height,
                                 target, stride, on_device as c_int, &mut bump)
            };
        }
        if let Some((id, again)) = refused {
            // resolve() marked these images resident and clean: ask for them again, so that a source bound after this failure is
            // copied by the next render (vello_amd/csrc/host/renderer.cpp does the same)
            for image in &again {
                self.resolver.mark_image_dirty(image);
            }
            return Err(Error::Invalid(format!(
                "Tried to draw an invalid empty image (id {}). Maybe it was registered to a different renderer, or \
                 unregistered before this render was submitted.",
                id
            )));
        }
        if rc == VELLO_HIP_OK { Ok(()) } else { Err(Self::error(ctx, rc, bump)) }
    }

    /// The vello_tests entry point (`render_then_debug_sync`, vello_tests/src/lib.rs:76): a frame into a fresh Vec.
    pub fn render_to_vec(&mut self, scene: &Scene, params: &RenderParams) -> Result<Vec<u8>, Error> {
        let mut out = vec![0u8; params.width as usize * params.height as usize * 4];
        self.render_to_buffer(scene, out.as_mut_ptr().cast(), params.width as usize * 4, false, params)?;
        Ok(out)
    }

    /// vello_hip_grow_pools after `Error::Capacity` when auto-grow was switched off.
    pub fn grow_pools(&mut self, demand: &vello_hip_bump) -> bool {
        unsafe { vello_hip_grow_pools(self.ctx, demand, core::ptr::null_mut()) == VELLO_HIP_OK }
    }

    /// `vello_hip_render_instances_painted`: a frame composed on the GPU from `(fragment, transform)` pairs of the fragment table
    /// made resident through `raw()` and `vello_hip_upload_fragments`, instance `i` drawn with `paints[i]` when a paint list is
    /// given, one per instance (`None`: `vello_hip_render_instances`).  A paint's `rgba` is the premultiplied RGBA8 word a solid brush encodes to
    /// (`DrawColor`, vello_encoding/src/draw.rs:70-74).  Enqueues the frame into device memory and returns without waiting.
    pub fn render_instances_painted(&mut self, instances: &[vello_hip_instance], paints: Option<&[vello_hip_paint]>, target: *mut c_void,
                                    stride: usize, params: &vello_hip_render_params) -> Result<(), Error> {
        if let Some(p) = paints {
            assert_eq!(p.len(), instances.len());
        }
        let paints_ptr = paints.map_or(core::ptr::null(), |p| p.as_ptr());
        let rc = unsafe { vello_hip_render_instances_painted(self.ctx, instances.as_ptr(), paints_ptr, instances.len() as u32, params, target, stride) };
        if rc == VELLO_HIP_OK { Ok(()) } else { Err(Self::error(self.ctx, rc, vello_hip_bump::default())) }
    }

    /// `vello_hip_retain_instances`: composes the list once into the context's retained scene; `render_retained` then re-poses it per
    /// frame.  Waits for the frames in flight.
    pub fn retain_instances(&mut self, instances: &[vello_hip_instance], paints: Option<&[vello_hip_paint]>) -> Result<(), Error> {
        if let Some(p) = paints {
            assert_eq!(p.len(), instances.len());
        }
        let paints_ptr = paints.map_or(core::ptr::null(), |p| p.as_ptr());
        let rc = unsafe { vello_hip_retain_instances(self.ctx, instances.as_ptr(), paints_ptr, instances.len() as u32) };
        if rc == VELLO_HIP_OK { Ok(()) } else { Err(Self::error(self.ctx, rc, vello_hip_bump::default())) }
    }

    /// `vello_hip_render_retained` with poses in host memory, one `[m0 m1 m2 m3 t0 t1]` per retained instance (`None`: the rest
    /// poses).  Enqueues the frame into device memory and returns without waiting.
    pub fn render_retained(&mut self, poses: Option<&[[f32; 6]]>, target: *mut c_void, stride: usize, params: &vello_hip_render_params) -> Result<(), Error> {
        let poses_ptr = poses.map_or(core::ptr::null(), |p| p.as_ptr().cast::<f32>());
        let rc = unsafe { vello_hip_render_retained(self.ctx, poses_ptr, 0, core::ptr::null_mut(), params, target, stride) };
        if rc == VELLO_HIP_OK { Ok(()) } else { Err(Self::error(self.ctx, rc, vello_hip_bump::default())) }
    }

    /// `vello_hip_render_retained` with poses in device memory (`6 * n` floats on the context's device, 4-byte aligned), written by
    /// work on `src_stream` (a `hipStream_t`, nullable): the frame waits for that work, the stream for the kernel that reads them.
    ///
    /// # Safety
    /// `poses` must stay valid, and unchanged by anything but `src_stream`, until the frame has read it.
    pub unsafe fn render_retained_device(&mut self, poses: *const f32, src_stream: *mut c_void, target: *mut c_void, stride: usize,
                                         params: &vello_hip_render_params) -> Result<(), Error> {
        let rc = vello_hip_render_retained(self.ctx, poses, 1, src_stream, params, target, stride);
        if rc == VELLO_HIP_OK { Ok(()) } else { Err(Self::error(self.ctx, rc, vello_hip_bump::default())) }
    }

    /// `vello_hip_render_retained_painted` with poses and this frame's paints in host memory, one of each per retained instance
    /// (`None`: the rest poses / an unpainted frame).  A paint with `VELLO_HIP_PAINT_KEEP` keeps what the list was retained with.
    pub fn render_retained_painted(&mut self, poses: Option<&[[f32; 6]]>, paints: Option<&[vello_hip_paint]>, target: *mut c_void, stride: usize,
                                   params: &vello_hip_render_params) -> Result<(), Error> {
        let poses_ptr = poses.map_or(core::ptr::null(), |p| p.as_ptr().cast::<f32>());
        let paints_ptr = paints.map_or(core::ptr::null(), |p| p.as_ptr());
        let rc = unsafe { vello_hip_render_retained_painted(self.ctx, poses_ptr, 0, paints_ptr, 0, core::ptr::null_mut(), params, target, stride) };
        if rc == VELLO_HIP_OK { Ok(()) } else { Err(Self::error(self.ctx, rc, vello_hip_bump::default())) }
    }

    /// `vello_hip_render_retained_painted` with poses and paints in device memory (`6 * n` floats and `2 * n` words on the context's
    /// device, 4-byte aligned, either nullable), written by work on `src_stream` (a `hipStream_t`, nullable): the frame waits for
    /// that work, the stream for the last kernel that reads them.
    ///
    /// # Safety
    /// `poses` and `paints` must stay valid, and unchanged by anything but `src_stream`, until the frame has read them.
    pub unsafe fn render_retained_painted_device(&mut self, poses: *const f32, paints: *const vello_hip_paint, src_stream: *mut c_void,
                                                 target: *mut c_void, stride: usize, params: &vello_hip_render_params) -> Result<(), Error> {
        let rc = vello_hip_render_retained_painted(self.ctx, poses, 1, paints, 1, src_stream, params, target, stride);
        if rc == VELLO_HIP_OK { Ok(()) } else { Err(Self::error(self.ctx, rc, vello_hip_bump::default())) }
    }

    /// `vello_hip_release_retained`.
    pub fn release_retained(&mut self) -> bool {
        unsafe { vello_hip_release_retained(self.ctx) == VELLO_HIP_OK }
    }

    pub fn raw(&self) -> *mut vello_hip_ctx {
        self.ctx
    }
}

impl Drop for HipRenderer {
    fn drop(&mut self) {
        unsafe { vello_hip_destroy(self.ctx) }
    }
}
