#!/usr/bin/env python3
"""Retained instance lists (vello_hip_retain_instances / vello_hip_render_retained) on the symbol map of the GPU suite -- 64 fragments
drawn from the road map's distributions, 30 000 instances, 1600 x 1600, MSAA16 -- with every symbol turning a little further each
frame, against vello_hip_render_instances frames of the same list and poses on ANOTHER build of the library (the parent commit's,
under ab_tmp/), both loaded into this process:
(a) frames/s one frame at a time and four in flight, in alternating rounds: retained frames with device poses (a tensor per phase, never
    read by the host), retained frames with host poses, and the other build's render_instances;
(b) the time of the render_retained call itself with device poses, the lanes idle, at 300 and at 30 000 instances -- the host does
    no per-instance work, so the two agree within the spread -- beside the other build's render_instances call at 30 000;
(c) with --mode, one route alone for a profiler run
        rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/retained_instances_bench.py --mode retained --rounds 1
    and with --summarise DIR the kernels' own times from that run's trace: k_instance_transforms against its traffic bound
    (owner + T + pose reads + stores) / 8 TB/s, k_compose_scene in the other build's frames.
    The kernel's time is taken from the profiler's kernel trace, not from HIP events of this script: the kernel is launched inside
    the frame, ahead of every stage's events, and no seam launches it alone.
(d) bench.py's d2 with the feature unused against the other build is not this script's: scripts/ab_bench.py A / B, alternating.
profiles/retained_instances.txt quotes its output and gives the command behind every figure.

    python scripts/retained_instances_bench.py --parent ab_tmp/libvello_hip_B.so [--steps 200] [--warmup 20] [--rounds 3] [--phases 8]
                                               [--mode all|retained|parent]"""
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
KERNELS = ("k_instance_transforms", "k_compose_scene", "k_view_transforms")


def summarise(trace_dir):
    files = glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)
    assert files, f"no kernel trace under {trace_dir}"
    times = {}
    for path in files:
        with open(path, newline="") as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name", "")
                for k in KERNELS:
                    if k in name and "painted" not in name:
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
    ap.add_argument("--mode", choices=["all", "retained", "parent"], default="all")
    ap.add_argument("--parent", default=os.path.join("ab_tmp", "libvello_hip_B.so"), help="the other build of libvello_hip.so (under ab_tmp/)")
    ap.add_argument("--summarise", help="a rocprofv3 output directory: print the kernels' times from its kernel trace and leave")
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)

    import torch

    import bench
    import vello_amd
    from tests import instance_parity as ip
    from vello_amd import AaConfig

    L = vello_amd._lib
    lib = vello_amd.FragmentLibrary(ip.symbol_fragments())
    lists = [ip.symbol_instances(0x5EED0003, n=a.instances, phase=0.05 * k) for k in range(a.phases)]
    host_poses = [np.ascontiguousarray(li["transform"], dtype=np.float32) for li in lists]
    engines = {}
    if a.mode != "retained":
        L._use_library(os.path.abspath(a.parent))
        engines["parent"] = vello_amd.Engine(device=0, capacities=bench.D2_CAPS)
        L._use_library(None)
    if a.mode != "parent":
        engines["this"] = vello_amd.Engine(device=0, capacities=bench.D2_CAPS)
    for e in engines.values():
        lib.upload(e)
    targets = [torch.zeros((H, W, 4), dtype=torch.uint8, device="cuda:0") for _ in range(4)]
    dev_poses = [torch.from_numpy(p).to("cuda:0") for p in host_poses]
    torch.cuda.synchronize()
    any_engine = next(iter(engines.values()))
    p = any_engine._params(W, H, WHITE, AaConfig.Msaa16)
    this, parent = engines.get("this"), engines.get("parent")
    lay, nbytes = any_engine.instances_layout(lists[0])
    n_xf = (lay.style_base - lay.transform_base) // 6
    traffic = 4 * n_xf + 24 * n_xf + 24 * a.instances + 24 * (n_xf + 1)
    print(f"symbol map: {len(lib.fragments)} fragments, {a.instances} instances, composed scene {nbytes} B ({nbytes / 1e6:.2f} MB), {n_xf} transform entries", flush=True)
    print(f"k_instance_transforms traffic: owner {4 * n_xf} + T {24 * n_xf} + poses {24 * a.instances} + stores {24 * (n_xf + 1)} = {traffic} B; "
          f"bound at 8 TB/s: {traffic / 8e12 * 1e6:.2f} us", flush=True)
    want = None
    if this:
        this.retain_instances(lists[0])
        this.render_retained(W, H, WHITE, AaConfig.Msaa16, transforms=dev_poses[-1], out=targets[0])
        assert this.sync() == 0, this.bump()
        want = targets[0].cpu().numpy().copy()

    def retained_device(nif, n):
        for i in range(n):
            this._check(this._lib.vello_hip_render_retained(this._h, dev_poses[i % a.phases].data_ptr(), 1, None, ctypes.byref(p), targets[i % nif].data_ptr(), W * 4), "render_retained")
        assert this.sync() == 0

    def retained_host(nif, n):
        for i in range(n):
            this._check(this._lib.vello_hip_render_retained(this._h, host_poses[i % a.phases].ctypes.data, 0, None, ctypes.byref(p), targets[i % nif].data_ptr(), W * 4), "render_retained")
        assert this.sync() == 0

    def parent_instances(nif, n):
        for i in range(n):
            li = lists[i % a.phases]
            parent._check(parent._lib.vello_hip_render_instances(parent._h, li.ctypes.data, len(li), ctypes.byref(p), targets[i % nif].data_ptr(), W * 4), "render_instances")
        assert parent.sync() == 0

    routes = []
    if this:
        routes += [("render_retained, device poses        ", retained_device), ("render_retained, host poses          ", retained_host)]
    if parent:
        routes += [("render_instances, the other build    ", parent_instances)]
    for nif in (1, 4):
        for e in engines.values():
            e.set_frames_in_flight(nif)
        for rnd in range(a.rounds):
            for label, route in routes:
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
                call_times(f"render_retained call, device poses, {n} instances, run {rep}", this.sync,
                           lambda i: this._lib.vello_hip_render_retained(this._h, dev_poses[i % a.phases].data_ptr(), 1, None, ctypes.byref(p), targets[0].data_ptr(), W * 4))
        call_times(f"render_retained call, host poses, {a.instances} instances", this.sync,
                   lambda i: this._lib.vello_hip_render_retained(this._h, host_poses[i % a.phases].ctypes.data, 0, None, ctypes.byref(p), targets[0].data_ptr(), W * 4))
        call_times(f"render_retained call, rest poses, {a.instances} instances", this.sync,
                   lambda i: this._lib.vello_hip_render_retained(this._h, None, 0, None, ctypes.byref(p), targets[0].data_ptr(), W * 4))
    if parent:
        call_times(f"render_instances call, the other build, {a.instances} instances", parent.sync,
                   lambda i: parent._lib.vello_hip_render_instances(parent._h, lists[i % a.phases].ctypes.data, a.instances, ctypes.byref(p), targets[0].data_ptr(), W * 4))
    if this and parent:
        parent._check(parent._lib.vello_hip_render_instances(parent._h, lists[-1].ctypes.data, a.instances, ctypes.byref(p), targets[1].data_ptr(), W * 4), "render_instances")
        assert parent.sync() == 0
        print(f"same frame by both routes: {np.array_equal(want, targets[1].cpu().numpy())}", flush=True)


if __name__ == "__main__":
    main()
