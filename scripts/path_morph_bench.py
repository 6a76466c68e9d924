#!/usr/bin/env python3
"""Per-frame path data (vello_hip_render_resident_morphed) on d2, bench.py's headline scene, 1600 x 1600, MSAA16.  Keyframe 0 is
the scene's own path data, keyframe 1 a smooth displacement of it (tests/morph_parity.keyframe); every frame's t is its own.
  (a) frames per second, one frame at a time (submit, wait) and with four frames in flight (submit --frames, wait once), of
        morphed    vello_hip_render_resident_morphed(key 0, key 1, t_k)
        resident   vello_hip_render_resident: the same pipeline without the blend -- the difference is the cost of the feature
        re-upload  vello_hip_render_frame fed the same frames' host-blended bytes: the only way to show such frames without it.  The
                   blended scenes are made before the clock starts (a ring of --ring), so the host's own blend is NOT in the number:
                   what is timed is the upload of the packed scene and a frame without the scene index;
      the three alternate within a repetition, --reps repetitions, medians and the spread.  With --lib PATH (another build of the
      library, e.g. the parent commit's as ab_tmp/libvello_hip_B.so: it has no morphed frames) only `resident` and `re-upload` are
      timed, on that build: what the feature's upload-time work costs the entry points that existed before it;
  (b) with --trace-modes: nothing is timed; --frames frames of each of the kernel's three modes in turn (copy A, copy B, mix) from the
      keyframes, then the mix once more from a device tensor that is only 4-byte aligned, a line per block, for a profiler run that
      shows k_path_blend alone:
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o ks -- python scripts/path_morph_bench.py --trace-modes --frames 20
      (the dispatches of k_path_blend in the trace are then 20 of each block, in that order).
profiles/path_morph.txt quotes its output.

    python scripts/path_morph_bench.py [--frames 200] [--reps 5] [--warmup 20] [--ring 8] [--lib PATH]"""
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
from tests import morph_parity as mp  # noqa: E402
from vello_amd import AaConfig  # noqa: E402

WHITE = 0xFFFFFFFF
W = H = 1600
AA = AaConfig.Msaa16


def t_of(k):
    return 0.05 + 0.9 * ((k * 37) % 101) / 100.0  # (never 0 or 1: every frame is a real blend)


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
    ap.add_argument("--ring", type=int, default=8)
    ap.add_argument("--trace-modes", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of libvello_hip.so (under ab_tmp/): resident and re-uploaded frames only")
    args = ap.parse_args()
    if args.lib:
        import vello_amd._lib as L

        L._use_library(os.path.abspath(args.lib))
        print(f"library: {args.lib}", flush=True)

    wl = bench.Workload("d2", 0)
    packed = np.ascontiguousarray(wl.packed, dtype=np.uint8)
    own = mp.path_words(packed, wl.layout)
    keys = np.stack([own, mp.keyframe(own, 3.0, 0.02, 0.4)])
    n = len(own)
    print(f"d2: {packed.nbytes / 1e6:.2f} MB packed, {n} path-data words ({4 * n / 1e6:.2f} MB): a blend reads {8 * n / 1e6:.2f} MB and writes "
          f"{4 * n / 1e6:.2f} MB, a copy reads and writes {4 * n / 1e6:.2f} MB each", flush=True)
    target = torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    eng = vello_amd.Engine(device=0, capacities=wl.caps)
    eng.upload_scene(packed, wl.layout)
    if not args.lib:
        eng.upload_path_keyframes(keys)
    allocations, builds = eng.scene_allocations(), eng.scene_index_builds()

    def morphed(k, morph=None):
        eng.render_resident(W, H, WHITE, AA, out=target, morph=morph or (0, 1, t_of(k)))

    def resident(k):
        eng.render_resident(W, H, WHITE, AA, out=target)

    if args.trace_modes:
        # (the fourth block: keyframe 1 again, as a tensor slice that starts one float in -- the kernel's dword form)
        buf = torch.zeros(n + 1, dtype=torch.float32, device="cuda:0")
        buf[1:].copy_(torch.from_numpy(keys[1].view(np.float32)))
        torch.cuda.synchronize()
        dev = vello_amd.PATH_DATA_DEVICE
        for name, morph, points in (("copy A", (0, 1, 0.0), None), ("copy B", (0, 1, 1.0), None), ("mix", (0, 1, 0.37), None),
                                    ("mix, dword accesses", (0, dev, 0.37), buf[1:])):
            for k in range(args.frames):
                eng.render_resident(W, H, WHITE, AA, out=target, morph=morph, points=points)
                assert eng.sync() == 0
            print(f"{args.frames} frames, k_path_blend in mode {name}", flush=True)
        return

    ring = [mp.substitute(packed, wl.layout, mp.blend(keys[0], keys[1], t_of(k))) for k in range(args.ring)]

    def reupload(k):
        eng.render_frame(ring[k % args.ring], wl.layout, W, H, WHITE, AA, out=target)

    copy_gbps = bench.measure_copy_peak(0)
    print(f"copy bandwidth of this GPU in this run (float4 copy of 1 GiB, read + written): {copy_gbps and round(copy_gbps, 1)} GB/s", flush=True)
    kinds = (("morphed", morphed), ("resident", resident), ("re-upload", reupload))[1 if args.lib else 0:]
    for in_flight in (1, 4):
        eng.set_frames_in_flight(in_flight)
        fps = {name: [] for name, _ in kinds}
        for name, f in kinds:
            timed(eng, f, args.warmup, in_flight)
        for _ in range(args.reps):
            for name, f in kinds:  # (alternating: what else runs on the box moves all three alike)
                fps[name].append(timed(eng, f, args.frames, in_flight))
        med = {name: float(np.median(v)) for name, v in fps.items()}
        for name, _ in kinds:
            v = np.array(fps[name])
            print(f"  {in_flight} in flight, {name:9s}: {med[name]:8.1f} frames/s median of {args.reps} x {args.frames} frames (min {v.min():.1f}, max {v.max():.1f}) "
                  f"= {1e3 / med[name]:.3f} ms a frame", flush=True)
        if not args.lib:
            print(f"  {in_flight} in flight: the morph costs {1e6 / med['morphed'] - 1e6 / med['resident']:+.1f} us a frame against resident frames "
                  f"({100 * (med['morphed'] / med['resident'] - 1):+.2f} % frames/s); morphed frames are {med['morphed'] / med['re-upload']:.2f} x the re-uploaded ones", flush=True)
    print(f"scene allocations since the keyframes' upload: {eng.scene_allocations() - allocations} (the re-uploaded frames' private slots); "
          f"scene indexes built: {eng.scene_index_builds() - builds}", flush=True)


if __name__ == "__main__":
    main()
