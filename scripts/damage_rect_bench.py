#!/usr/bin/env python3
"""Damage rectangles (vello_hip_set_damage_rect) on d2, bench.py's headline scene, 1600 x 1600, MSAA16, resident frames into one
device target.
  (a) frames per second, one frame at a time (submit, wait) and with four frames in flight (submit --frames, wait once), of whole
      frames and of frames with a rectangle R centred on the target: 1600^2 (the whole target through the option), 800^2, 256^2,
      64^2, 16^2, and a full-width strip 1600 x 64.  The kinds alternate within a repetition, --reps repetitions, medians and the
      spread.  Device-synchronised host clock.
  (b) vello_hip_get_stage_ms of COARSE, PATH_TILING and FINE per kind, in a pass of its own behind the timed ones (profiling launches
      the stages one by one: it is not on while frames/s are taken), with bump.segments and |W|.
  With --lib PATH (another build of the library, e.g. the parent commit's as ab_tmp/libvello_hip_B.so: it has no such option) only
  whole frames are timed, on that build: what the option costs the frames that do not use it.
profiles/damage_rect.txt quotes its output.

    python scripts/damage_rect_bench.py [--frames 200] [--reps 5] [--warmup 20] [--lib PATH]"""
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


def centred(w, h):
    return ((W - w) // 2, (H - h) // 2, (W - w) // 2 + w, (H - h) // 2 + h)


KINDS = (("whole (off)", None), ("1600 x 1600", centred(1600, 1600)), ("800 x 800", centred(800, 800)), ("256 x 256", centred(256, 256)),
         ("64 x 64", centred(64, 64)), ("16 x 16", centred(16, 16)), ("1600 x 64 strip", centred(1600, 64)))


def n_window_tiles(rect):
    if rect is None:
        return (W // 16) * (H // 16)
    x0, y0, x1, y1 = rect
    return ((x1 + 15) // 16 - x0 // 16) * ((y1 + 15) // 16 - y0 // 16)


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
    ap.add_argument("--lib", default=None, help="another build of libvello_hip.so (under ab_tmp/): whole frames only")
    args = ap.parse_args()
    if args.lib:
        import vello_amd._lib as L

        L._use_library(os.path.abspath(args.lib))
        print(f"library: {args.lib}", flush=True)

    wl = bench.Workload("d2", 0)
    target = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng = vello_amd.Engine(device=0, capacities=wl.caps)
    eng.upload_scene(np.ascontiguousarray(wl.packed, dtype=np.uint8), wl.layout)
    kinds = KINDS[:1] if args.lib else KINDS

    def frame(rect):
        def submit():
            if not args.lib:
                eng.set_damage_rect(rect)
            eng.render_resident(W, H, WHITE, AA, out=target)
        return submit

    med = {}
    for in_flight in (1, 4):
        eng.set_frames_in_flight(in_flight)
        fps = {name: [] for name, _ in kinds}
        for name, rect in kinds:
            timed(eng, frame(rect), args.warmup, in_flight)
        for _ in range(args.reps):
            for name, rect in kinds:  # (alternating: what else runs on the box moves all kinds alike)
                fps[name].append(timed(eng, frame(rect), args.frames, in_flight))
        for name, _ in kinds:
            v = np.array(fps[name])
            med[in_flight, name] = float(np.median(v))
            print(f"  {in_flight} in flight, {name:16s}: {med[in_flight, name]:8.1f} frames/s median of {args.reps} x {args.frames} frames "
                  f"(min {v.min():.1f}, max {v.max():.1f}) = {1e3 / med[in_flight, name]:.3f} ms a frame, "
                  f"{med[in_flight, name] / med[in_flight, kinds[0][0]]:.2f} x whole", flush=True)
    if args.lib:
        return
    # the three stages behind the window, one frame at a time, profiled in a pass of their own
    eng.set_frames_in_flight(1)
    stages = ("coarse", "path_tiling", "fine")
    print("  stage times (us a frame, vello_hip_get_stage_ms over --frames frames, one frame at a time), bump.segments, |W|", flush=True)
    for name, rect in kinds:
        eng.set_damage_rect(rect)
        eng.set_profiling(stages)
        eng.stage_ms()  # (drains what earlier frames left)
        for _ in range(args.frames):
            eng.render_resident(W, H, WHITE, AA, out=target)
            assert eng.sync() == 0
        ms = eng.stage_ms()
        eng.set_profiling(())
        bump = eng.bump()
        us = {s: 1e3 * ms[s][0] / max(ms[s][1], 1) for s in stages}
        print(f"    {name:16s}: coarse {us['coarse']:7.1f}  path_tiling {us['path_tiling']:7.1f}  fine {us['fine']:7.1f}   segments {bump['segments']:8d}  "
              f"|W| {n_window_tiles(rect):6d}", flush=True)
    eng.set_damage_rect(None)


if __name__ == "__main__":
    main()
