#!/usr/bin/env python3
"""The view transform (vello_hip_set_view_transform): (a) view on against off, same build, alternating -- frames/s one frame at a time
and four in flight on the d2 scene at 1600 x 1600 and 800 x 800 and on the 1024 x 576 mmark window (the view that is "on" is a pan of
a few pixels for d2 and the window's own view for mmark, whose "off" is the window re-encoded on the host: the same picture either
way); (b) the case the feature exists for: a pan sequence over the resident d2 scene at 800 x 800 with viewport culling on, a new view
every frame, by set_view_transform + render_resident against the only route there was before -- the same views composed and packed on
the host ahead of time and cycled through vello_hip_render_frame, so that only the upload is charged to it, not the encoding.
profiles/view_transform.txt quotes its output.

    python scripts/view_transform_bench.py [--steps 200] [--warmup 20] [--rounds 3] [--only d2_800] [--view 0|1] [--skip-pan]

--only / --view pin one case and one setting for a profiler run (rocprofv3 --kernel-trace --stats -- python scripts/...)."""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import vello_amd  # noqa: E402
import workloads  # noqa: E402
from vello_amd import AaConfig, Affine, Scene  # noqa: E402

WHITE = 0xFFFFFFFF


def cases():
    """(name, scene for 'off', scene for 'on', view for 'on', w, h)"""
    d2 = workloads.paris_like_scene_d2().resolve()
    mm = workloads.mmark_scene()
    window = Affine.translate(-600, -500) * Affine.scale(1.5)
    encoded = Scene()
    encoded.append(mm, window)
    pan = Affine.translate(-3.25, -1.5)
    return [("d2_1600", d2, d2, pan, 1600, 1600), ("d2_800", d2, d2, pan, 800, 800), ("mmark_window", encoded.resolve(), mm.resolve(), window, 1024, 576)]


def frames_per_s(eng, w, h, nif, steps, warmup, targets, view_of_frame=None):
    def frame(i):
        if view_of_frame is not None:
            eng.set_view_transform(view_of_frame(i))
        eng.render_resident(w, h, WHITE, AaConfig.Msaa16, out=targets[i % nif])

    for i in range(warmup):
        frame(i)
    assert eng.sync() == 0
    t0 = time.perf_counter()
    for i in range(steps):
        frame(i)
    assert eng.sync() == 0
    return steps / (time.perf_counter() - t0)


def pan_views(n):
    """n views of a pan over the top-left quarter of d2: a different one every frame."""
    return [Affine.translate(-400.0 * (0.5 - 0.5 * np.cos(2 * np.pi * k / n)), -300.0 * (0.5 - 0.5 * np.cos(4 * np.pi * k / n))) for k in range(n)]


def composed_scenes(packed, layout, views):
    """What a host-side Scene.append(scene, view) + resolve leaves in the transform stream, without the encoding: the packed bytes with
    the stream replaced (the formula of include/vello_hip.h, numpy f32)."""
    out = []
    base, n_xf = layout.transform_base, (layout.style_base - layout.transform_base) // 6
    for a in views:
        v = np.array(a.c, dtype=np.float32)
        p = np.ascontiguousarray(packed, dtype=np.uint8).copy()
        t = p.view(np.uint32)[base: base + n_xf * 6].view(np.float32).reshape(-1, 6)
        c = np.stack([v[0] * t[:, 0] + v[2] * t[:, 1], v[1] * t[:, 0] + v[3] * t[:, 1], v[0] * t[:, 2] + v[2] * t[:, 3], v[1] * t[:, 2] + v[3] * t[:, 3],
                      (v[0] * t[:, 4] + v[2] * t[:, 5]) + v[4], (v[1] * t[:, 4] + v[3] * t[:, 5]) + v[5]], axis=1).astype(np.float32)
        t[:] = c
        out.append(p)
    return out


def pan_sequence(steps, warmup, rounds):
    packed, layout = workloads.paris_like_scene_d2().resolve()
    w = h = 800
    n_views = 40
    views = pan_views(n_views)
    scenes = composed_scenes(packed, layout, views)
    print(f"pan sequence: d2 at {w}x{h}, culling on, {n_views} views cycled, scene {scenes[0].nbytes / 1e6:.1f} MB, "
          f"{(layout.style_base - layout.transform_base) // 6} transforms", flush=True)
    eng = vello_amd.Engine(device=0, capacities=bench.D2_CAPS)
    eng.set_viewport_cull(True)
    targets = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0") for _ in range(4)]
    torch.cuda.synchronize()
    lay = vello_amd._lib.LayoutStruct(*layout)
    p = eng._params(w, h, WHITE, AaConfig.Msaa16)

    def upload_route(nif, n):
        for i in range(n):
            s = scenes[i % n_views]
            eng._check(eng._lib.vello_hip_render_frame(eng._h, s.ctypes.data, s.nbytes, ctypes.byref(lay), ctypes.byref(p), None, 0,
                                                       targets[i % nif].data_ptr(), w * 4), "render_frame")
        assert eng.sync() == 0

    for nif in (1, 4):
        eng.set_frames_in_flight(nif)
        for r in range(rounds):
            eng.upload_scene(packed, layout)
            f = frames_per_s(eng, w, h, nif, steps, warmup, targets, view_of_frame=lambda i: views[i % n_views])
            eng.set_view_transform(None)
            print(f"  in flight {nif} round {r} set_view_transform + render_resident: {f:9.1f} frames/s", flush=True)
            upload_route(nif, warmup)
            t0 = time.perf_counter()
            upload_route(nif, steps)
            f = steps / (time.perf_counter() - t0)
            print(f"  in flight {nif} round {r} pre-composed scenes + render_frame  : {f:9.1f} frames/s", flush=True)
    # the two routes show the same frames
    eng.set_frames_in_flight(1)
    eng.upload_scene(packed, layout)
    eng.set_view_transform(views[7])
    eng.render_resident(w, h, WHITE, AaConfig.Msaa16, out=targets[0])
    eng.set_view_transform(None)
    assert eng.sync() == 0
    a = targets[0].cpu().numpy().copy()
    eng._check(eng._lib.vello_hip_render_frame(eng._h, scenes[7].ctypes.data, scenes[7].nbytes, ctypes.byref(lay), ctypes.byref(p), None, 0,
                                               targets[1].data_ptr(), w * 4), "render_frame")
    assert eng.sync() == 0
    print(f"  same frame by both routes: {np.array_equal(a, targets[1].cpu().numpy())}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--view", type=int, default=None)
    ap.add_argument("--skip-pan", action="store_true")
    a = ap.parse_args()
    for name, off_scene, on_scene, view, w, h in cases():
        if a.only and name != a.only:
            continue
        eng = vello_amd.Engine(device=0, capacities=bench.D2_CAPS)
        targets = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0") for _ in range(4)]
        torch.cuda.synchronize()
        settings = (0, 1) if a.view is None else (a.view,)
        n_xf = (on_scene[1].style_base - on_scene[1].transform_base) // 6
        print(f"{name} {w}x{h}: {n_xf} transforms", flush=True)
        for nif in (1, 4):
            eng.set_frames_in_flight(nif)
            for r in range(a.rounds):
                for on in settings:
                    eng.upload_scene(*(on_scene if on else off_scene))
                    eng.set_view_transform(view if on else None)
                    f = frames_per_s(eng, w, h, nif, a.steps, a.warmup, targets)
                    eng.set_view_transform(None)
                    print(f"  in flight {nif} round {r} view {'on ' if on else 'off'}: {f:9.1f} frames/s", flush=True)
        del eng
    if not a.only and not a.skip_pan:
        pan_sequence(a.steps, a.warmup, a.rounds)


if __name__ == "__main__":
    main()
