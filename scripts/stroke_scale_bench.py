#!/usr/bin/env python3
"""The per-frame stroke scale (vello_hip_set_stroke_scale) on d2, bench.py's headline scene, 1600 x 1600, MSAA16.
  (a) frames per second, one frame at a time (submit, wait) and with four frames in flight (submit --frames, wait once), of resident
      frames
        off        no setting: the launches a frame ran before the feature
        (1, 0)     the same image: the off state's frame plus k_style_widths
        (0.5, 0)   thinner strokes
        (2, 0)     wider strokes
      and of the host alternative for the last two -- widths patched on the host plus vello_hip_render_frame.  The patched scenes are
      made before the clock starts, so the host's own patching is NOT in the number: what is timed is the upload of the packed scene and
      a frame without the scene index.  The kinds alternate within a repetition, --reps repetitions, medians and the spread.  With
      --lib PATH (another build of the library, e.g. the parent commit's as ab_tmp/libvello_hip_B.so: it has no such setting) only `off`
      is timed, on that build.
      The setting is set once per timed window, outside the clock: a frame under it pays no call the host alternative does not.
  (b) with --trace: nothing is timed; --frames frames under (0.5, 0), a line, for a profiler run that shows k_style_widths alone (no
      entry point launches the kernel outside a frame, so HIP events around it cannot be had from here: the kernel's time is the
      profiler's, and (1, 0) against off above is what it costs a frame):
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ks -- python scripts/stroke_scale_bench.py --trace --frames 50
profiles/stroke_scale.txt quotes its output.

    python scripts/stroke_scale_bench.py [--frames 200] [--reps 5] [--warmup 20] [--lib PATH]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import vello_amd  # noqa: E402
from tests import stroke_scale_parity as sp  # noqa: E402
from vello_amd import AaConfig  # noqa: E402

WHITE = 0xFFFFFFFF
W = H = 1600
AA = AaConfig.Msaa16


def timed(eng, submit, n, in_flight):
    """Frames per second of n frames: one at a time (a wait after each) or all submitted, one wait at the end."""
    t0 = time.perf_counter()
    for k in range(n):
        submit(k)
        if in_flight == 1:
            assert eng.sync() == 0
    assert eng.sync() == 0, eng.bump()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of libvello_hip.so (under ab_tmp/): the off state only")
    args = ap.parse_args()
    if args.lib:
        import vello_amd._lib as L

        L._use_library(os.path.abspath(args.lib))
        print(f"library: {args.lib}", flush=True)

    wl = bench.Workload("d2", 0)
    packed = np.ascontiguousarray(wl.packed, dtype=np.uint8)
    flags, bits = sp.style_words(packed, wl.layout)
    n_strokes = int(((flags & np.uint32(sp.STYLE_FLAGS_STYLE)) != 0).sum())
    print(f"d2: {packed.nbytes / 1e6:.2f} MB packed, {len(flags)} style entries ({8 * len(flags) / 1e3:.1f} KB; {n_strokes} strokes): k_style_widths reads and "
          f"writes that much, {(len(flags) + 255) // 256} workgroups; style_base is {'even' if wl.layout.style_base % 2 == 0 else 'odd'}", flush=True)
    target = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng = vello_amd.Engine(device=0, capacities=wl.caps)
    eng.set_auto_grow(True)
    eng.upload_scene(packed, wl.layout)
    allocations, builds = eng.scene_allocations(), eng.scene_index_builds()

    def resident(k):
        eng.render_resident(W, H, WHITE, AA, out=target)

    if args.trace:
        eng.set_stroke_scale(0.5, 0.0)
        for k in range(args.frames):
            eng.render_resident(W, H, WHITE, AA, out=target)
            assert eng.sync() == 0
        print(f"{args.frames} frames under (0.5, 0)", flush=True)
        return

    def reupload(setting):
        patched = sp.scaled(packed, wl.layout, setting)

        def f(k):
            eng.render_frame(patched, wl.layout, W, H, WHITE, AA, out=target)

        return f

    # (name, the setting in force for the whole timed window -- set once, outside the clock -- and the frame)
    kinds = [("off", None, resident)]
    if not args.lib:
        # (the pools hold the widest frame before the clock starts: a frame under (2, 0) asks for more segments than the plain one)
        for setting in ((2.0, 0.0),):
            eng.set_stroke_scale(*setting)
            for _ in range(4):
                eng.render_resident(W, H, WHITE, AA, out=target)
                r = eng.sync()
                if r == 0:
                    break
                assert r == -4 and eng.grow_pools(eng.bump()), r
            eng.set_stroke_scale(None)
        kinds += [("(1, 0)", (1.0, 0.0), resident), ("(0.5, 0)", (0.5, 0.0), resident), ("(2, 0)", (2.0, 0.0), resident),
                  ("host (0.5, 0)", None, reupload((0.5, 0.0))), ("host (2, 0)", None, reupload((2.0, 0.0)))]
        # the same image under (1, 0)
        resident(0)
        assert eng.sync() == 0
        off = target.cpu().numpy().copy()
        eng.set_stroke_scale(1.0, 0.0)
        resident(0)
        eng.set_stroke_scale(None)
        assert eng.sync() == 0
        print(f"(1, 0) gives the off state's image: {np.array_equal(off, target.cpu().numpy())}", flush=True)
    for in_flight in (1, 4):
        eng.set_frames_in_flight(in_flight)
        fps = {name: [] for name, _, _ in kinds}

        def window(setting, f, n):
            if setting is not None:
                eng.set_stroke_scale(*setting)
            try:
                return timed(eng, f, n, in_flight)
            finally:
                if setting is not None:
                    eng.set_stroke_scale(None)

        for name, setting, f in kinds:
            window(setting, f, args.warmup)
        for _ in range(args.reps):
            for name, setting, f in kinds:  # (alternating: what else runs on the box moves all of them alike)
                fps[name].append(window(setting, f, args.frames))
        med = {name: float(np.median(v)) for name, v in fps.items()}
        for name, _, _ in kinds:
            v = np.array(fps[name])
            print(f"  {in_flight} in flight, {name:13s}: {med[name]:8.1f} frames/s median of {args.reps} x {args.frames} frames (min {v.min():.1f}, max {v.max():.1f}) "
                  f"= {1e3 / med[name]:.3f} ms a frame", flush=True)
        if not args.lib:
            print(f"  {in_flight} in flight: the setting costs {1e6 / med['(1, 0)'] - 1e6 / med['off']:+.1f} us a frame against the off state "
                  f"({100 * (med['(1, 0)'] / med['off'] - 1):+.2f} % frames/s); resident frames are {med['(0.5, 0)'] / med['host (0.5, 0)']:.2f} x (0.5) and "
                  f"{med['(2, 0)'] / med['host (2, 0)']:.2f} x (2) the host alternative's", flush=True)
    print(f"scene allocations since the upload: {eng.scene_allocations() - allocations} (the re-uploaded frames' private slots); "
          f"scene indexes built: {eng.scene_index_builds() - builds}", flush=True)


if __name__ == "__main__":
    main()
