#!/usr/bin/env python3
"""Scene instances (vello_hip_render_instances) on the symbol map of the GPU suite -- 64 fragments drawn from the road map's
distributions, 30 000 instances, 1600 x 1600, MSAA16 -- with every symbol turning a little further each frame:
(a) frames/s by render_instances against the route there was before on the same build: the same frames' composed bytes, made ahead of
    time, through vello_hip_render_frame (host composition is not charged to it), alternating, one frame at a time and four in flight;
(b) the time of the render_instances call itself, the lanes idle;
(c) with --mode, one route alone for a profiler run (rocprofv3 --kernel-trace --stats -- python scripts/scene_instances_bench.py
    --mode instances --rounds 1): k_compose_scene's own time against the bound 2 x scene bytes / 8 TB/s.
(d) with --paints, every instance painted (vello_hip_render_instances_painted), the colours changing with the phase: the old route is
    given the PAINTED bytes, the call is timed painted and not, and a profiler run shows k_compose_scene_painted beside k_compose_scene;
(e) with --library, another build of libvello_hip.so (an earlier commit's, under ab_tmp/) for a same-session A/B of the unpainted path.
profiles/scene_instances.txt and profiles/instance_paints.txt quote its output.

    python scripts/scene_instances_bench.py [--steps 200] [--warmup 20] [--rounds 3] [--phases 8] [--mode both|instances|frames]
                                            [--paints] [--library ab_tmp/libvello_hip_B.so]"""
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
from tests import instance_parity as ip  # noqa: E402
from vello_amd import AaConfig  # noqa: E402

WHITE = 0xFFFFFFFF
W = H = 1600


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--phases", type=int, default=8)
    ap.add_argument("--instances", type=int, default=30000)
    ap.add_argument("--mode", choices=["both", "instances", "frames"], default="both")
    ap.add_argument("--paints", action="store_true", help="paint every instance, the colours changing with the phase")
    ap.add_argument("--library", help="another build of libvello_hip.so (under ab_tmp/)")
    a = ap.parse_args()
    if a.library:
        vello_amd._lib._use_library(os.path.abspath(a.library))
    lib = vello_amd.FragmentLibrary(ip.symbol_fragments())
    lists = [ip.symbol_instances(0x5EED0003, n=a.instances, phase=0.05 * k) for k in range(a.phases)]
    paints = [None] * a.phases
    if a.paints:
        for k in range(a.phases):
            paints[k] = np.zeros(a.instances, dtype=vello_amd.PAINT_DTYPE)
            paints[k]["flags"] = 1
            paints[k]["rgba"] = 0xFF000000 | ((np.arange(a.instances, dtype=np.uint32) * 2654435761 + k * 0x010305) & 0xFFFFFF)
    eng = vello_amd.Engine(device=0, capacities=bench.D2_CAPS)
    lib.upload(eng)
    targets = [torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0") for _ in range(4)]
    torch.cuda.synchronize()
    p = eng._params(W, H, WHITE, AaConfig.Msaa16)
    # the frames' composed bytes, as the engine composes them (tests/instance_parity.py holds them to a numpy composition)
    scenes, layouts = [], []
    for li, pt in zip(lists, paints):
        lay, nbytes = eng.instances_layout(li)
        eng.render_instances(li, W, H, WHITE, AaConfig.Msaa16, out=targets[0], **({"paints": pt} if a.paints else {}))
        r = eng.sync()
        assert r == 0, f"sync {r}: {eng.bump()}"
        scenes.append(eng.read_buffer("scene", np.uint8, nbytes).copy())
        layouts.append(vello_amd._lib.LayoutStruct(*lay))
    want = targets[0].cpu().numpy().copy()
    b = eng.bump()
    print(f"symbol map: {len(lib.fragments)} fragments (library {lib.packed.nbytes} B), {a.instances} instances, composed scene {scenes[0].nbytes} B "
          f"({scenes[0].nbytes / 1e6:.2f} MB), instance list {lists[0].nbytes} B, table {(60 if a.paints else 52) * a.instances + 24} B{', every instance painted' if a.paints else ''}, lines {b['lines']}, segments {b['segments']}", flush=True)
    print(f"bound for k_compose_scene: 2 x {scenes[0].nbytes} B / 8 TB/s = {2 * scenes[0].nbytes / 8e12 * 1e6:.2f} us", flush=True)

    def call(li, pt, target):
        if pt is None:
            return eng._lib.vello_hip_render_instances(eng._h, li.ctypes.data, len(li), ctypes.byref(p), target.data_ptr(), W * 4)
        return eng._lib.vello_hip_render_instances_painted(eng._h, li.ctypes.data, pt.ctypes.data, len(li), ctypes.byref(p), target.data_ptr(), W * 4)

    def by_instances(nif, n):
        for i in range(n):
            eng._check(call(lists[i % a.phases], paints[i % a.phases], targets[i % nif]), "render_instances")
        assert eng.sync() == 0

    def by_frames(nif, n):
        for i in range(n):
            s = scenes[i % a.phases]
            eng._check(eng._lib.vello_hip_render_frame(eng._h, s.ctypes.data, s.nbytes, ctypes.byref(layouts[i % a.phases]), ctypes.byref(p), None, 0,
                                                       targets[i % nif].data_ptr(), W * 4), "render_frame")
        assert eng.sync() == 0

    routes = [("render_instances              ", by_instances), ("pre-composed bytes + render_frame", by_frames)]
    if a.mode != "both":
        routes = [r for r in routes if (r[1] is by_instances) == (a.mode == "instances")]
    for nif in (1, 4):
        eng.set_frames_in_flight(nif)
        for rnd in range(a.rounds):
            for label, route in routes:
                route(nif, a.warmup)
                t0 = time.perf_counter()
                route(nif, a.steps)
                print(f"  in flight {nif} round {rnd} {label}: {a.steps / (time.perf_counter() - t0):9.1f} frames/s", flush=True)
    eng.set_frames_in_flight(1)
    if a.mode != "frames":
        # the call itself, the lane idle
        for label, pts in (("render_instances", [None] * a.phases),) + ((("render_instances_painted", paints),) if a.paints else ()):
            ts = []
            for i in range(60):
                assert eng.sync() == 0
                t0 = time.perf_counter()
                r = call(lists[i % a.phases], pts[i % a.phases], targets[0])
                ts.append(time.perf_counter() - t0)
                assert r == 0
            assert eng.sync() == 0
            ts = np.array(ts[10:]) * 1e6
            print(f"{label} call at {a.instances} instances (lane idle, 50 calls): median {np.median(ts):.0f} us, min {ts.min():.0f} us, max {ts.max():.0f} us", flush=True)
    # both routes show the same frame
    eng._check(eng._lib.vello_hip_render_frame(eng._h, scenes[-1].ctypes.data, scenes[-1].nbytes, ctypes.byref(layouts[-1]), ctypes.byref(p), None, 0,
                                               targets[1].data_ptr(), W * 4), "render_frame")
    assert eng.sync() == 0
    print(f"same frame by both routes: {np.array_equal(want, targets[1].cpu().numpy())}", flush=True)


if __name__ == "__main__":
    main()
