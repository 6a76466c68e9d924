#!/usr/bin/env python3
"""Viewport culling (vello_hip_set_viewport_cull) on against off, same build, alternating: frames/s one frame at a time and four
in flight, the stages the option touches (vello_hip_get_stage_ms / get_kernel_ms) and bump.lines, on the d2 scene at 1600 x 1600
and its top-left 800 x 800 and on a 1024 x 576 window into the mmark scene.  profiles/viewport_cull.txt quotes its output.

    python scripts/viewport_cull_bench.py [--steps 200] [--warmup 20] [--rounds 3] [--only d2_800] [--cull 0|1]

--only / --cull pin one case and one setting for a profiler run (rocprofv3 --kernel-trace --stats -- python scripts/...)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bench  # noqa: E402
import vello_amd  # noqa: E402
import workloads  # noqa: E402
from vello_amd import AaConfig, Affine, Scene  # noqa: E402

WHITE = 0xFFFFFFFF
STAGES = ("flatten", "path_count", "path_tiling")


def cases():
    d2 = workloads.paris_like_scene_d2().resolve()
    view = Scene()
    view.append(workloads.mmark_scene(), Affine.translate(-600, -500) * Affine.scale(1.5))
    return [("d2_1600", d2, 1600, 1600, bench.D2_CAPS), ("d2_800", d2, 800, 800, bench.D2_CAPS), ("mmark_view", view.resolve(), 1024, 576, bench.D2_CAPS)]


def frames_per_s(eng, w, h, nif, steps, warmup, targets):
    for i in range(warmup):
        eng.render_resident(w, h, WHITE, AaConfig.Msaa16, out=targets[i % nif])
    assert eng.sync() == 0
    t0 = time.perf_counter()
    for i in range(steps):
        eng.render_resident(w, h, WHITE, AaConfig.Msaa16, out=targets[i % nif])
    assert eng.sync() == 0
    return steps / (time.perf_counter() - t0)


def stage_times(eng, w, h, frames, target):
    eng.set_profiling(STAGES)
    eng.stage_ms(), eng.kernel_ms()  # (reading clears the sums)
    for _ in range(frames):
        eng.render_resident(w, h, WHITE, AaConfig.Msaa16, out=target)
    assert eng.sync() == 0
    st, km = eng.stage_ms(), eng.kernel_ms()
    eng.set_profiling(())
    out = {s: 1e3 * st[s][0] / max(st[s][1], 1) for s in STAGES}
    out.update({k: 1e3 * v[0] / max(v[1], 1) for k, v in km.items() if k.startswith("k_flatten")})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--cull", type=int, default=None)
    a = ap.parse_args()
    for name, (packed, layout), w, h, caps in cases():
        if a.only and name != a.only:
            continue
        eng = vello_amd.Engine(device=0, capacities=caps)
        eng.upload_scene(packed, layout)
        targets = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0") for _ in range(4)]
        torch.cuda.synchronize()
        settings = (0, 1) if a.cull is None else (a.cull,)
        lines = {}
        for on in settings:
            eng.set_viewport_cull(bool(on))
            eng.render_resident(w, h, WHITE, AaConfig.Msaa16, out=targets[0])
            assert eng.sync() == 0
            b = eng.bump()
            assert b["failed"] == 0, b
            lines[on] = b["lines"]
        print(f"{name} {w}x{h}: bump.lines " + ", ".join(f"{'on' if on else 'off'} {n}" for on, n in lines.items()), flush=True)
        for nif in (1, 4):
            eng.set_frames_in_flight(nif)
            eng.upload_scene(packed, layout)
            for r in range(a.rounds):
                for on in settings:
                    eng.set_viewport_cull(bool(on))
                    f = frames_per_s(eng, w, h, nif, a.steps, a.warmup, targets)
                    print(f"  in flight {nif} round {r} cull {'on ' if on else 'off'}: {f:9.1f} frames/s", flush=True)
        eng.set_frames_in_flight(1)
        eng.upload_scene(packed, layout)
        for r in range(2):
            for on in settings:
                eng.set_viewport_cull(bool(on))
                t = stage_times(eng, w, h, 30, targets[0])
                print(f"  stage us/frame round {r} cull {'on ' if on else 'off'}: " + "  ".join(f"{k} {v:7.1f}" for k, v in t.items()), flush=True)
        del eng


if __name__ == "__main__":
    main()
