#!/usr/bin/env python3
"""Per-frame paints of retained instance lists (vello_hip_render_retained_painted, k_instance_paints) on the symbol map of the GPU
suite -- 64 fragments, 30 000 instances, 1600 x 1600, MSAA16 -- with every symbol turning a little further AND taking a fresh colour
each frame (8 pose sets, 8 paint sets), against the only routes ANOTHER build of the library (the parent commit's, under ab_tmp/)
offers for the same frames, both builds loaded into this process:
(a) frames/s one frame at a time and four in flight, in alternating rounds:
      this build    render_retained_painted, device paints + device poses (tensors the host never reads); host paints + host poses
      the other     (a) render_instances_painted per frame; (b) retain_instances + render_retained per frame
    and, the feature unused, unpainted render_retained frames on both builds (beside each other here; with --mode unpainted [--lib
    PATH] one build alone in the process, to be run once per build, alternating);
(b) the time of the call itself, the lane idle, with device and with host paints, at 300 and at 30 000 instances;
(c) the last frame by every route, byte for byte;
(d) with --mode, one route alone for a profiler run
        rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/retained_paints_bench.py --mode painted --rounds 1
    and with --summarise DIR the kernels' own times from that run's trace: k_instance_paints against its traffic bound
    (table + retained words + paints read, words stored) / 8 TB/s.
bench.py's d2 with the feature unused against the other build is not this script's: scripts/ab_bench.py A / B, alternating.
profiles/retained_paints.txt quotes its output and gives the command behind every figure.

    python scripts/retained_paints_bench.py --parent ab_tmp/libvello_hip_B.so [--steps 200] [--warmup 20] [--rounds 3] [--phases 8]
                                            [--mode all|painted|parent|unpainted] [--lib PATH]"""
import argparse
import csv
import ctypes
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

WHITE = 0xFFFFFFFF
W = H = 1600
KERNELS = ("k_instance_paints", "k_instance_transforms", "k_compose_scene_painted", "k_compose_scene")


def summarise(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {trace_dir}"
    times = {}
    for path in files:
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name", "")
                k = next((k for k in KERNELS if k in name), None)  # (the longer name of the two compose kernels comes first)
                if k:
                    times.setdefault(k, []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for k, v in sorted(times.items()):
        v = np.array(v)
        print(f"{k}: {len(v)} dispatches, median {np.median(v):.2f} us, min {v.min():.2f} us, max {v.max():.2f} us (rocprofv3 kernel trace)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--phases", type=int, default=8)
    ap.add_argument("--instances", type=int, default=30000)
    ap.add_argument("--mode", choices=["all", "painted", "parent", "unpainted"], default="all")
    ap.add_argument("--lib", help="--mode unpainted: the build to load (default: the in-tree library)")
    ap.add_argument("--parent", default=os.path.join("ab_tmp", "libvello_hip_B.so"), help="the other build of libvello_hip.so (under ab_tmp/)")
    ap.add_argument("--summarise", help="a rocprofv3 output directory: print the kernels' times from its kernel trace and leave")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)

    import torch

    import bench
    import vello_amd
    from tests import instance_parity as ip
    from vello_amd import PAINT_DTYPE, AaConfig

    L = vello_amd._lib
    lib = vello_amd.FragmentLibrary(ip.symbol_fragments())
    lists = [ip.symbol_instances(0x5EED0003, n=a.instances, phase=0.05 * k) for k in range(a.phases)]
    host_poses = [np.ascontiguousarray(li["transform"], dtype=np.float32) for li in lists]
    rng = np.random.default_rng(0x5EED0007)
    host_paints = []
    for k in range(a.phases):  # every instance a fresh opaque colour each frame
        pt = np.zeros(a.instances, dtype=PAINT_DTYPE)
        pt["flags"] = 1
        pt["rgba"] = rng.integers(0, 1 << 24, a.instances, dtype=np.uint32) | np.uint32(0xFF000000)
        host_paints.append(pt)
    if a.mode == "unpainted":
        # the feature unused, ONE build alone in the process (two engines in one process share the hardware queues, and which was
        # created first shows in the frames/s with frames in flight): unpainted retained frames, device poses; run once per build, alternating
        if a.lib:
            L._use_library(os.path.abspath(a.lib))
        e = vello_amd.Engine(device=0, capacities=bench.D2_CAPS)
        lib.upload(e)
        e.retain_instances(lists[0])
        targets = [torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0") for _ in range(4)]
        dev_poses = [torch.from_numpy(p).to("cuda:0") for p in host_poses]
        torch.cuda.synchronize()
        p = e._params(W, H, WHITE, AaConfig.Msaa16)
        for nif in (1, 4):
            e.set_frames_in_flight(nif)
            for rnd in range(a.rounds):
                for n in (a.warmup, a.steps):
                    t0 = time.perf_counter()
                    for i in range(n):
                        e._check(e._lib.vello_hip_render_retained(e._h, dev_poses[i % a.phases].data_ptr(), 1, None, ctypes.byref(p), targets[i % nif].data_ptr(), W * 4), "render_retained")
                    assert e.sync() == 0
                print(f"  {a.lib or 'in-tree'}: in flight {nif} round {rnd} unpainted render_retained, device poses: {a.steps / (time.perf_counter() - t0):9.1f} frames/s", flush=True)
        return
    engines = {}
    if a.mode != "painted":
        L._use_library(os.path.abspath(a.parent))
        engines["parent"] = vello_amd.Engine(device=0, capacities=bench.D2_CAPS)
        L._use_library(None)
    if a.mode != "parent":
        engines["this"] = vello_amd.Engine(device=0, capacities=bench.D2_CAPS)
    for e in engines.values():
        lib.upload(e)
    targets = [torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0") for _ in range(4)]
    dev_poses = [torch.from_numpy(p).to("cuda:0") for p in host_poses]
    dev_paints = [torch.from_numpy(p.view(np.int32).reshape(-1, 2).copy()).to("cuda:0") for p in host_paints]
    torch.cuda.synchronize()
    any_engine = next(iter(engines.values()))
    p = any_engine._params(W, H, WHITE, AaConfig.Msaa16)
    this, parent = engines.get("this"), engines.get("parent")
    lay, nbytes = any_engine.instances_layout(lists[0])
    n_dd = lay.transform_base - lay.draw_data_base
    traffic = 4 * n_dd + 4 * n_dd + 8 * a.instances + 4 * n_dd
    print(f"symbol map: {len(lib.fragments)} fragments, {a.instances} instances, composed scene {nbytes} B ({nbytes / 1e6:.2f} MB), {n_dd} draw-data words", flush=True)
    print(f"k_instance_paints traffic: table {4 * n_dd} + retained words {4 * n_dd} + paints {8 * a.instances} + stores {4 * n_dd} = {traffic} B; "
          f"bound at 8 TB/s: {traffic / 8e12 * 1e6:.2f} us", flush=True)
    last = a.phases - 1
    images = {}

    def shot(label, engine, target):
        assert engine.sync() == 0, engine.bump()
        images[label] = target.cpu().numpy().copy()

    def painted_call(i, t, device=True):
        k = i % a.phases
        if device:
            return this._lib.vello_hip_render_retained_painted(this._h, dev_poses[k].data_ptr(), 1, dev_paints[k].data_ptr(), 1, None, ctypes.byref(p), t.data_ptr(), W * 4)
        return this._lib.vello_hip_render_retained_painted(this._h, host_poses[k].ctypes.data, 0, host_paints[k].ctypes.data, 0, None, ctypes.byref(p), t.data_ptr(), W * 4)

    def painted_device(nif, n):
        for i in range(n):
            this._check(painted_call(i, targets[i % nif]), "render_retained_painted")
        assert this.sync() == 0

    def painted_host(nif, n):
        for i in range(n):
            this._check(painted_call(i, targets[i % nif], device=False), "render_retained_painted")
        assert this.sync() == 0

    def parent_instances_painted(nif, n):
        for i in range(n):
            k = i % a.phases
            parent._check(parent._lib.vello_hip_render_instances_painted(parent._h, lists[k].ctypes.data, host_paints[k].ctypes.data, len(lists[k]), ctypes.byref(p),
                                                                         targets[i % nif].data_ptr(), W * 4), "render_instances_painted")
        assert parent.sync() == 0

    def parent_retain_each(nif, n):
        for i in range(n):
            k = i % a.phases
            parent._check(parent._lib.vello_hip_retain_instances(parent._h, lists[k].ctypes.data, host_paints[k].ctypes.data, len(lists[k])), "retain_instances")
            parent._check(parent._lib.vello_hip_render_retained(parent._h, None, 0, None, ctypes.byref(p), targets[i % nif].data_ptr(), W * 4), "render_retained")
        assert parent.sync() == 0

    def unpainted(engine):
        def run(nif, n):
            for i in range(n):
                engine._check(engine._lib.vello_hip_render_retained(engine._h, dev_poses[i % a.phases].data_ptr(), 1, None, ctypes.byref(p), targets[i % nif].data_ptr(), W * 4),
                              "render_retained")
            assert engine.sync() == 0
        return run

    routes = []
    if this:
        this.retain_instances(lists[0])
        routes += [("this: render_retained_painted, device paints + poses ", painted_device), ("this: render_retained_painted, host paints + poses   ", painted_host)]
    if parent:
        routes += [("parent (a): render_instances_painted per frame       ", parent_instances_painted),
                   ("parent (b): retain_instances + render_retained       ", parent_retain_each)]
    for nif in (1, 4):
        for e in engines.values():
            e.set_frames_in_flight(nif)
        for rnd in range(a.rounds):
            for label, route in routes:
                route(nif, a.warmup)
                t0 = time.perf_counter()
                route(nif, a.steps)
                print(f"  in flight {nif} round {rnd} {label}: {a.steps / (time.perf_counter() - t0):9.1f} frames/s", flush=True)
    # the feature unused: unpainted retained frames of one list on both builds, alternating
    if this and parent:
        parent.retain_instances(lists[0])
        this.retain_instances(lists[0])
        for nif in (1, 4):
            for e in engines.values():
                e.set_frames_in_flight(nif)
            for rnd in range(a.rounds):
                for label, e in (("this:   unpainted render_retained, device poses", this), ("parent: unpainted render_retained, device poses", parent)):
                    route = unpainted(e)
                    route(nif, a.warmup)
                    t0 = time.perf_counter()
                    route(nif, a.steps)
                    print(f"  in flight {nif} round {rnd} {label}: {a.steps / (time.perf_counter() - t0):9.1f} frames/s", flush=True)
    for e in engines.values():
        e.set_frames_in_flight(1)

    def call_times(label, sync, call):
        ts = []
        for i in range(60):
            assert sync() == 0
            t0 = time.perf_counter()
            r = call(i)
            ts.append(time.perf_counter() - t0)
            assert r == 0
        assert sync() == 0
        ts = np.array(ts[10:]) * 1e6
        print(f"{label} (lane idle, 50 calls): median {np.median(ts):.1f} us, min {ts.min():.1f} us, max {ts.max():.1f} us", flush=True)

    if this:
        for n in (300, a.instances):
            this.retain_instances(lists[0][:n])
            for rep in range(2):  # (twice: the spread between two runs of the same thing)
                call_times(f"render_retained_painted call, device paints + poses, {n} instances, run {rep}", this.sync, lambda i: painted_call(i, targets[0]))
            call_times(f"render_retained_painted call, host paints + poses, {n} instances", this.sync, lambda i: painted_call(i, targets[0], device=False))
        call_times(f"render_retained call, device poses, no paints, {a.instances} instances", this.sync,
                   lambda i: this._lib.vello_hip_render_retained(this._h, dev_poses[i % a.phases].data_ptr(), 1, None, ctypes.byref(p), targets[0].data_ptr(), W * 4))
        # the last frame by every route
        this._check(painted_call(last, targets[0]), "render_retained_painted")
        shot("this, device", this, targets[0])
        this._check(painted_call(last, targets[0], device=False), "render_retained_painted")
        shot("this, host", this, targets[0])
    if parent:
        call_times(f"render_instances_painted call, the other build, {a.instances} instances", parent.sync,
                   lambda i: parent._lib.vello_hip_render_instances_painted(parent._h, lists[i % a.phases].ctypes.data, host_paints[i % a.phases].ctypes.data, a.instances,
                                                                            ctypes.byref(p), targets[0].data_ptr(), W * 4))
        parent._check(parent._lib.vello_hip_render_instances_painted(parent._h, lists[last].ctypes.data, host_paints[last].ctypes.data, a.instances, ctypes.byref(p),
                                                                     targets[1].data_ptr(), W * 4), "render_instances_painted")
        shot("parent (a)", parent, targets[1])
        parent.retain_instances(lists[last], paints=host_paints[last])
        parent.render_retained(W, H, WHITE, AaConfig.Msaa16, out=targets[1])
        shot("parent (b)", parent, targets[1])
    if len(images) > 1:
        first = next(iter(images.values()))
        print("the last frame by every route (" + ", ".join(images) + f"): byte for byte equal: {all(np.array_equal(first, v) for v in images.values())}", flush=True)


if __name__ == "__main__":
    main()
