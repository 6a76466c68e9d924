#!/usr/bin/env python3
"""Base images (vello_hip_set_base_image) on d2, bench.py's headline scene, 1600 x 1600, MSAA16, resident frames into one device
target.
  (a) frames per second, one frame at a time (submit, wait) and with four frames in flight (submit --frames, wait once), of frames
      without the setting (`off`), over a separate base image (`separate`: a second 1600 x 1600 surface), and in place (`in place`:
      the image is the target).  The kinds alternate within a repetition, --reps repetitions, medians and the spread.
      Device-synchronised host clock.
  (b) k_fine_base against k_fine by HIP events: vello_hip_get_stage_ms of FINE per kind, in a pass of its own behind the timed ones
      (profiling launches the stages one by one: it is not on while frames/s are taken), a wait after every frame, with one frame
      in flight configured (fine's WAVES = 4 instantiation) and with four (the WAVES = 5 one).
  (c) that a uniform image gives the off state's target, and that a frame in place over an opaque earlier frame is that frame again.
  With --lib PATH (another build of the library, e.g. the parent commit's as ab_tmp/libvello_hip_B.so: it has no such setting) only
  `off` is timed, on that build: what the setting costs the frames that do not use it.
profiles/base_image.txt quotes its output.

    python scripts/base_image_bench.py [--frames 200] [--reps 5] [--warmup 20] [--lib PATH]"""
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
from vello_amd import AaConfig  # noqa: E402

WHITE = 0xFFFFFFFF
W = H = 1600
AA = AaConfig.Msaa16


def timed(eng, submit, n, in_flight):
    """Frames per second of n frames: one at a time (a wait after each) or all submitted, one wait at the end."""
    t0 = time.perf_counter()
    for _ in range(n):
        submit()
        if in_flight == 1:
            assert eng.sync() == 0
    assert eng.sync() == 0, eng.bump()
    return n / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--lib", default=None, help="another build of libvello_hip.so (under ab_tmp/): the off state only")
    args = ap.parse_args()
    if args.lib:
        import vello_amd._lib as L

        L._use_library(os.path.abspath(args.lib))
        print(f"library: {args.lib}", flush=True)

    wl = bench.Workload("d2", 0)
    target = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    # a base that is not uniform: a gradient of opaque words (premultiplied = straight), so that in-place frames stay well defined
    yy, xx = np.mgrid[0:H, 0:W]
    rows = np.stack([(xx * 255 // (W - 1)), (yy * 255 // (H - 1)), ((xx + yy) // 7 % 256), np.full((H, W), 255)], axis=2).astype(np.uint8)
    image = torch.from_numpy(rows).to("cuda:0")
    torch.cuda.synchronize()
    eng = vello_amd.Engine(device=0, capacities=wl.caps)
    eng.upload_scene(np.ascontiguousarray(wl.packed, dtype=np.uint8), wl.layout)
    kinds = (("off", None),) if args.lib else (("off", None), ("separate", image), ("in place", target))

    def frame(img):
        def submit():
            if not args.lib:
                eng.set_base_image(img)
            eng.render_resident(W, H, WHITE, AA, out=target)
        return submit

    if not args.lib:
        # (c) what the frames/s below are frames of
        frame(None)()
        assert eng.sync() == 0
        off = target.cpu().numpy().copy()
        white = torch.full((H, W, 4), 255, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        frame(white)()
        assert eng.sync() == 0
        print(f"  a uniform image of the base colour gives the off state's target: {np.array_equal(target.cpu().numpy(), off)}", flush=True)
        frame(image)()
        assert eng.sync() == 0
        over = target.cpu().numpy().copy()
        print(f"  the frame over the gradient differs from the off state's in {(over != off).any(axis=2).mean() * 100:.1f} % of the pixels; "
              f"opaque everywhere: {bool((over[:, :, 3] == 255).all())}", flush=True)

    med = {}
    for in_flight in (1, 4):
        eng.set_frames_in_flight(in_flight)
        fps = {name: [] for name, _ in kinds}
        for name, img in kinds:
            timed(eng, frame(img), args.warmup, in_flight)
        for _ in range(args.reps):
            for name, img in kinds:  # (alternating: what else runs on the box moves all kinds alike)
                fps[name].append(timed(eng, frame(img), args.frames, in_flight))
        for name, _ in kinds:
            v = np.array(fps[name])
            med[in_flight, name] = float(np.median(v))
            print(f"  {in_flight} in flight, {name:9s}: {med[in_flight, name]:8.1f} frames/s median of {args.reps} x {args.frames} frames "
                  f"(min {v.min():.1f}, max {v.max():.1f}) = {1e3 / med[in_flight, name]:.4f} ms a frame, "
                  f"{(1e3 / med[in_flight, name] - 1e3 / med[in_flight, 'off']) * 1e3:+.1f} us against off", flush=True)
    if args.lib:
        return
    # (b) fine by HIP events, one frame at a time, profiled in a pass of its own
    print("  fine by HIP events (us a frame, vello_hip_get_stage_ms over --frames frames, a wait after every frame): with one frame in", flush=True)
    print("  flight configured (the WAVES = 4 instantiation) and with four (the WAVES = 5 one, alone on the chip)", flush=True)
    for lanes in (1, 4):
        eng.set_frames_in_flight(lanes)
        for rep in range(2):
            for name, img in kinds:
                eng.set_base_image(img)
                eng.set_profiling(("fine",))
                eng.stage_ms()  # (drains what earlier frames left)
                for _ in range(args.frames):
                    eng.render_resident(W, H, WHITE, AA, out=target)
                    assert eng.sync() == 0
                ms = eng.stage_ms()
                eng.set_profiling(())
                print(f"    {lanes} configured, pass {rep}, {name:9s}: fine {1e3 * ms['fine'][0] / max(ms['fine'][1], 1):7.1f}", flush=True)
    eng.set_base_image(None)
    eng.set_frames_in_flight(1)


if __name__ == "__main__":
    main()
