#!/usr/bin/env python3
"""Marquee selection (vello_hip_pick_rect) on the two large frames of the suite: d2 (bench.py's headline scene, rendered resident) and
the symbol map (64 fragments, 30 000 instances, composed on the GPU), both 1600 x 1600, MSAA16.  Each frame is rendered once; then
vello_hip_pick_rect is timed into device outputs for three marquees -- about 1 % of the target, a quarter of it, all of it:
  (a) device time of the call's launches -- the zero fill, k_region_lines, the two kernels of the draw pass, k_region_instances -- by
      the two events of vello_hip_pick_ms, median of --reps calls after --warmup;
  (b) the whole blocking call on the host clock, the lane idle: what a caller pays;
beside them the counts, 24 B x lines / the launches' time against the copy bandwidth of this GPU in this run
(bench.measure_copy_peak) -- a lower bound of the line pass's rate: the kernels one by one come from a kernel-trace run -- and, on the
same frames in the same session, vello_hip_pick with one point, the yardstick a one-rectangle query is compared with.
profiles/pick_rect.txt quotes its output.

    python scripts/pick_rect_bench.py [--reps 30] [--warmup 5] [--scenes d2,symbols] [--marquees small,quarter,all] [--lib PATH]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ks -- python scripts/pick_rect_bench.py --scenes d2 --marquees all
    --lib: another build of the same sources (the A/B of the line pass's atomics: scripts/experiments/region_plain_or.patch)"""
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
import vello_amd._lib as L  # noqa: E402
from tests import instance_parity as ip  # noqa: E402
from vello_amd import AaConfig  # noqa: E402

WHITE = 0xFFFFFFFF
W = H = 1600
AA = AaConfig.Msaa16
MARQUEES = {"small": (700.0, 700.0, 860.0, 860.0), "quarter": (400.0, 400.0, 1200.0, 1200.0), "all": (0.0, 0.0, float(W), float(H))}


def measure(label, eng, render, args, copy_gbps):
    render()
    assert eng.sync() == 0, eng.bump()
    lines = eng.bump()["lines"]
    soup = 24 * lines
    n_draw, n_inst = eng.pick_rect_sizes()
    print(f"{label}: {lines} lines ({soup / 1e6:.2f} MB of soup), {n_draw} draw objects, {n_inst} instances", flush=True)
    draws = torch.zeros(max(n_draw, 1), dtype=torch.int32, device="cuda:0")[:n_draw]
    insts = torch.zeros(n_inst, dtype=torch.int32, device="cuda:0") if n_inst else None
    pt = torch.tensor([[800.5, 800.5]], dtype=torch.float32, device="cuda:0")
    hit = torch.zeros((1, 2), dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    eng.set_profiling(["fine"])
    try:
        for name in args.marquees:
            rect = MARQUEES[name]
            dev, host = [], []
            for k in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                _, _, counts = eng.pick_rect(rect, draws_out=draws, instances_out=insts, instances=insts is not None)
                host.append((time.perf_counter() - t0) * 1e3)
                dev.append(eng.pick_ms())
            dev, host = np.array(dev[args.warmup:]), np.array(host[args.warmup:])
            med = float(np.median(dev))
            rate = soup / (med * 1e-3) / 1e9 if med > 0 else float("nan")
            share = 100.0 * (rect[2] - rect[0]) * (rect[3] - rect[1]) / (W * H)
            print(f"  {name:8s} ({share:5.1f} % of the target): launches median {med * 1e3:8.1f} us (min {dev.min() * 1e3:.1f}, max {dev.max() * 1e3:.1f}), "
                  f"call on the host clock median {np.median(host) * 1e3:8.1f} us; soup / launches {rate:7.1f} GB/s"
                  + (f" ({100 * rate / copy_gbps:.1f} % of the {copy_gbps:.0f} GB/s copy)" if copy_gbps else "") + f"; {counts}", flush=True)
        dev, host = [], []
        for k in range(args.warmup + args.reps):
            t0 = time.perf_counter()
            eng.pick(pt, out=hit)
            host.append((time.perf_counter() - t0) * 1e3)
            dev.append(eng.pick_ms())
        dev, host = np.array(dev[args.warmup:]), np.array(host[args.warmup:])
        print(f"  vello_hip_pick, one point: launches median {np.median(dev) * 1e3:8.1f} us (min {dev.min() * 1e3:.1f}, max {dev.max() * 1e3:.1f}), "
              f"call on the host clock median {np.median(host) * 1e3:8.1f} us", flush=True)
    finally:
        eng.set_profiling([])
        eng.stage_ms()  # (returns the frames' events to the pool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--marquees", type=lambda v: v.split(","), default=list(MARQUEES), help="small, quarter, all; comma separated")
    ap.add_argument("--scenes", default="d2,symbols", help="d2, symbols or both (for a profiler run of one)")
    ap.add_argument("--lib", default=None, help="another build of libvello_hip.so to measure in the tree's place")
    args = ap.parse_args()
    if args.lib:
        L._use_library(os.path.abspath(args.lib))
        print(f"library: {args.lib}", flush=True)
    copy_gbps = bench.measure_copy_peak(0)
    print(f"copy bandwidth of this GPU in this run (float4 copy of 1 GiB, read + written): {copy_gbps and round(copy_gbps, 1)} GB/s", flush=True)
    target = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    if "d2" in args.scenes:
        wl = bench.Workload("d2", 0)
        eng = vello_amd.Engine(device=0, capacities=wl.caps)
        eng.upload_scene(wl.packed, wl.layout)
        measure("d2 (render_resident)", eng, lambda: eng.render_resident(W, H, WHITE, AA, out=target), args, copy_gbps)
        del eng
    if "symbols" not in args.scenes:
        return

    lib = vello_amd.FragmentLibrary(ip.symbol_fragments())
    inst = ip.symbol_instances(0x5EED0003)
    eng = vello_amd.Engine(device=0, capacities=bench.D2_CAPS)
    lib.upload(eng)
    measure("symbol map (render_instances, 30 000 instances)", eng, lambda: eng.render_instances(inst, W, H, WHITE, AA, out=target), args, copy_gbps)
    # the instance words are the OR of their draws' TOUCHED bits
    draws, insts, counts = eng.pick_rect(MARQUEES["quarter"])
    off = np.concatenate([[0], np.cumsum([lib.fragments[int(f)]["draws"][1] - lib.fragments[int(f)]["draws"][0] for f in inst["fragment"]])])
    own = np.searchsorted(off[:-1], np.nonzero(draws & 1)[0], side="right") - 1
    assert set(own.tolist()) == set(np.nonzero(insts & 1)[0].tolist()) and counts["instances_touched"] == len(set(own.tolist()))
    print(f"symbol map: quarter marquee: {counts}, every touched instance owns a touched draw", flush=True)


if __name__ == "__main__":
    main()
