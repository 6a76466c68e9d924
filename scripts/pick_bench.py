#!/usr/bin/env python3
"""Hit testing (vello_hip_pick) on the two large frames of the suite: d2 (bench.py's headline scene, rendered resident) and the symbol
map (64 fragments, 30 000 instances, composed on the GPU), both 1600 x 1600, MSAA16.  Each frame is rendered once; then
vello_hip_pick is timed for n = 1, 64 and 4096 device points into a device result:
  (a) device time of the pick's launches -- every batch's zero fill, k_pick_lines and k_pick_resolve -- by the two events of
      vello_hip_pick_ms, median of --reps calls after --warmup;
  (b) the whole blocking call on the host clock, the lane idle (the wait for the frame, the read of its bump counters, the launches,
      the final wait): what a caller pays;
beside them the soup's size, the batches the call was cut into (engine.h pick_batch), 24 B x lines / time per batch against the copy
bandwidth of this GPU in this run (bench.measure_copy_peak: scripts/calib/copy_bw.hip), and the frame's own one-at-a-time time.
profiles/pick.txt quotes its output.

    python scripts/pick_bench.py [--reps 30] [--warmup 5] [--frames 30] [--points 1,64,4096] [--scenes d2,symbols]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ks -- python scripts/pick_bench.py --scenes d2 --points 1   (the kernels one by one)"""
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
from tests import instance_parity as ip  # noqa: E402
from vello_amd import AaConfig  # noqa: E402

WHITE = 0xFFFFFFFF
W = H = 1600
AA = AaConfig.Msaa16


def frame_ms(render, eng, n):
    """One frame at a time: submit, wait; median milliseconds of n."""
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        render()
        assert eng.sync() == 0
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts[n // 4:]))


def measure(label, eng, render, n_paths, args, copy_gbps):
    render()
    assert eng.sync() == 0, eng.bump()
    lines = eng.bump()["lines"]
    soup = 24 * lines
    consts = eng.pick_constants()
    fit = consts["scratch_bytes"] // (4 * n_paths) if n_paths else 4096
    batch = max(1, min(4096, fit))
    print(f"{label}: {lines} lines ({soup / 1e6:.2f} MB of soup), {n_paths} paths, winding row {4 * n_paths} B: {batch} queries per batch", flush=True)
    f_ms = frame_ms(render, eng, args.frames)
    print(f"  the frame itself, one at a time: {f_ms:.3f} ms", flush=True)
    rng = np.random.default_rng(5)
    eng.set_profiling(["fine"])
    try:
        for n in args.points:
            pts = torch.from_numpy(np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], axis=1).astype(np.float32)).to("cuda:0")
            out = torch.zeros((n, 2), dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            dev, host = [], []
            for k in range(args.warmup + args.reps):
                t0 = time.perf_counter()
                eng.pick(pts, out=out)
                host.append((time.perf_counter() - t0) * 1e3)
                dev.append(eng.pick_ms())
            dev, host = np.array(dev[args.warmup:]), np.array(host[args.warmup:])
            batches = -(-n // batch)
            per_batch = float(np.median(dev)) / batches
            hits = int((out.cpu().numpy().view(np.uint32)[:, 0] != vello_amd.PICK_NONE).sum())
            rate = soup / (per_batch * 1e-3) / 1e9 if per_batch > 0 else float("nan")
            print(f"  n = {n:4d}: launches median {np.median(dev):8.3f} ms (min {dev.min():.3f}, max {dev.max():.3f}), call on the host clock median {np.median(host):8.3f} ms; "
                  f"{batches} batch(es), {per_batch * 1e3:8.1f} us per batch = soup at {rate:7.1f} GB/s"
                  + (f" ({100 * rate / copy_gbps:.1f} % of the {copy_gbps:.0f} GB/s copy)" if copy_gbps else "") + f"; {hits} of {n} points hit", flush=True)
    finally:
        eng.set_profiling([])
        eng.stage_ms()  # (returns the frames' events to the pool)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--points", type=lambda v: [int(x) for x in v.split(",")], default=[1, 64, 4096], help="query counts, comma separated")
    ap.add_argument("--scenes", default="d2,symbols", help="d2, symbols or both (for a profiler run of one)")
    args = ap.parse_args()
    copy_gbps = bench.measure_copy_peak(0)
    print(f"copy bandwidth of this GPU in this run (float4 copy of 1 GiB, read + written): {copy_gbps and round(copy_gbps, 1)} GB/s", flush=True)
    target = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()

    if "d2" in args.scenes:
        wl = bench.Workload("d2", 0)
        eng = vello_amd.Engine(device=0, capacities=wl.caps)
        eng.upload_scene(wl.packed, wl.layout)
        measure("d2 (render_resident)", eng, lambda: eng.render_resident(W, H, WHITE, AA, out=target), wl.layout.n_paths, args, copy_gbps)
        del eng
    if "symbols" not in args.scenes:
        return

    lib = vello_amd.FragmentLibrary(ip.symbol_fragments())
    inst = ip.symbol_instances(0x5EED0003)
    eng = vello_amd.Engine(device=0, capacities=bench.D2_CAPS)
    lib.upload(eng)
    lay, _ = eng.instances_layout(inst)
    measure("symbol map (render_instances, 30 000 instances)", eng, lambda: eng.render_instances(inst, W, H, WHITE, AA, out=target), lay.n_paths, args, copy_gbps)
    # the owner of every hit is an instance of the list
    pts = torch.from_numpy(np.random.default_rng(6).uniform(0, W, (4096, 2)).astype(np.float32)).to("cuda:0")
    torch.cuda.synchronize()
    got = eng.pick(pts)
    hit = got[:, 0] != vello_amd.PICK_NONE
    assert (got[hit, 1] < len(inst)).all() and (got[~hit, 1] == vello_amd.PICK_NONE).all()
    print(f"symbol map: {int(hit.sum())} of 4096 points hit, owners within the list", flush=True)


if __name__ == "__main__":
    main()
