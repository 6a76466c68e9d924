"""N > 1 path on CPU: gloo ranks (2 and 4, uneven scene counts) shard scenes round-robin, render (SIMT-emulated kernels stand in for
the GPU here: test infrastructure) and gather frames to rank 0, which checks every frame against the oracle."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZE = 160
SEED0 = 0x5EED0001


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, n_scenes, result_path):
    import sys

    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import vello_amd._lib as L

    from tests.emu_lib import emu_library_path

    L._use_library(emu_library_path())
    import vello_amd
    import workloads
    from vello_amd.distributed import gather_frames, shard_scenes

    engine = vello_amd.Engine()
    mine = shard_scenes(n_scenes, rank, world)
    frames_at_root = {}
    for step in range((n_scenes + world - 1) // world):
        if step < len(mine):
            scene = workloads.paris_like_scene(SEED0 + mine[step], n_paths=120, size=float(SIZE))
            packed, layout = scene.resolve()
            img, bump = engine.render(packed, layout, SIZE, SIZE, 0xFFFFFFFF, vello_amd.AaConfig.Msaa16)
            assert bump["failed"] == 0
        else:
            img = np.zeros((SIZE, SIZE, 4), dtype=np.uint8)
        got = gather_frames(torch.from_numpy(img), rank, world)
        if rank == 0:
            for r, f in enumerate(got):
                ix = step * world + r
                if ix < n_scenes:
                    frames_at_root[ix] = f.numpy().copy()
    dist.barrier()
    if rank == 0:
        np.savez(result_path, **{f"f{k}": v for k, v in frames_at_root.items()})
    dist.destroy_process_group()


def test_two_rank_scene_sharding_and_gather(built, tmp_path):
    import workloads
    from oracle.oracle import Oracle
    from vello_amd.distributed import shard_scenes

    assert shard_scenes(5, 0, 2) == [0, 2, 4] and shard_scenes(5, 1, 2) == [1, 3]
    n_scenes, world = 3, 2
    result = str(tmp_path / "frames.npz")
    mp.spawn(_worker, args=(world, _free_port(), n_scenes, result), nprocs=world, join=True)
    frames = np.load(result)
    assert len(frames.files) == n_scenes
    o = Oracle()
    for i in range(n_scenes):
        packed, layout = workloads.paris_like_scene(SEED0 + i, n_paths=120, size=float(SIZE)).resolve()
        o.set_scene(packed, layout, SIZE, SIZE, 0xFFFFFFFF, 2)
        assert np.array_equal(frames[f"f{i}"], o.render()), f"scene {i} gathered at rank 0 differs from the oracle"


def test_four_rank_uneven_scene_counts(built, tmp_path):
    # 6 scenes on 4 ranks: ranks 0 and 1 render two scenes, ranks 2 and 3 one and then take part in the second gather
    # with an empty frame (the collective needs every rank); every scene still arrives at rank 0 exactly once
    import workloads
    from oracle.oracle import Oracle
    from vello_amd.distributed import shard_scenes

    assert [shard_scenes(6, r, 4) for r in range(4)] == [[0, 4], [1, 5], [2], [3]]
    n_scenes, world = 6, 4
    result = str(tmp_path / "frames4.npz")
    mp.spawn(_worker, args=(world, _free_port(), n_scenes, result), nprocs=world, join=True)
    frames = np.load(result)
    assert sorted(frames.files) == [f"f{i}" for i in range(n_scenes)]
    o = Oracle()
    for i in range(n_scenes):
        packed, layout = workloads.paris_like_scene(SEED0 + i, n_paths=120, size=float(SIZE)).resolve()
        o.set_scene(packed, layout, SIZE, SIZE, 0xFFFFFFFF, 2)
        assert np.array_equal(frames[f"f{i}"], o.render()), f"scene {i} gathered at rank 0 differs from the oracle"


def test_frame_pipeline_exchanges_every_frame_once_in_order():
    # bench.py --gpus N keeps n frames in flight and gathers the oldest one while the younger ones render; the
    # bookkeeping is checked here with recording fakes (no GPU): order, wait ages, slot reuse only after the exchange
    from vello_amd.distributed import FramePipeline

    for n in (1, 2, 3, 6):
        for k in (1, 2, 5, 6, 7, 20):
            log, rendered, exchanged, handles = [], [], [], {}
            frame_of_slot = {}

            def render(slot):
                assert handles.get(slot) is None, "slot re-rendered before its exchange was waited for"
                frame_of_slot[slot] = len(rendered)
                rendered.append(slot)
                log.append(("render", slot))

            def wait_frame(age):
                assert 0 <= age < n and age < len(rendered)
                log.append(("wait", len(rendered) - 1 - age))

            def exchange(slot):
                f = frame_of_slot[slot]
                assert ("wait", f) in log, "exchange before the frame was waited for"
                exchanged.append(f)
                handles[slot] = f
                return slot

            def wait_exchange(slot):
                handles[slot] = None

            p = FramePipeline(n, render, wait_frame, exchange, wait_exchange)
            for _ in range(k):
                p.step()
            p.flush()
            assert exchanged == list(range(k)), (n, k, exchanged)
            assert p.issued == 0
    # single-GPU form: no exchange, nothing but renders into rotating slots
    calls = []
    p = FramePipeline(3, calls.append, lambda age: calls.append(("wait", age)))
    for _ in range(7):
        p.step()
    p.flush()
    assert calls == [0, 1, 2, 0, 1, 2, 0]


# ---- bench.py's N > 1 control flow (launch contract, barriers, MAX over ranks, pipelined gather, one JSON line) ----
# A multi-GPU box is never available to the tests, so the distributed branch of bench.py is exercised here with the
# GPU-facing pieces replaced by recording fakes: torch.cuda.* no-ops, "nccl" -> gloo, an Engine that paints its rank
# into the target.  What runs for real: argument/env handling, FramePipeline, gather_frames over gloo, the barrier /
# all_reduce(MAX) timing protocol, the exchange-alone measurement and the JSON contract.
def _bench_worker(rank, world, port, out_path, extra_args=()):
    import io
    import json
    import runpy
    import sys
    import types

    sys.path.insert(0, ROOT)
    os.environ.update({"MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "RANK": str(rank), "LOCAL_RANK": str(rank),
                       "WORLD_SIZE": str(world)})
    torch.cuda.is_available = lambda: True
    torch.cuda.set_device = lambda d: None
    torch.cuda.synchronize = lambda *a, **k: None

    class _Event:
        def __init__(self, *a, **k):
            pass

        def record(self, *a):
            pass

        def synchronize(self):
            pass

        def elapsed_time(self, other):
            return 1.0

    torch.cuda.Event = _Event
    real_init = dist.init_process_group
    dist.init_process_group = lambda backend=None, **kw: real_init("gloo", **kw)
    for name in ("zeros", "tensor", "empty"):
        real = getattr(torch, name)

        def on_cpu(*a, _real=real, **kw):
            kw.pop("device", None)
            return _real(*a, **kw)

        setattr(torch, name, on_cpu)

    import vello_amd
    import vello_amd.renderer
    import workloads

    calls = {"render": 0, "sync_frame": 0}

    class FakeEngine:
        def __init__(self, device=0, capacities=None):
            self.prof = []

        def capacities(self):
            return {"lines": 1, "tiles": 1}

        def upload_scene(self, packed, layout, ramps=None):
            pass

        def set_frames_in_flight(self, n):
            pass

        def render_resident(self, w, h, base, aa, out=None):
            calls["render"] += 1
            out.fill_(rank + 1 + 10 * (calls["render"] % 20))  # (rank and frame number: the dumped frame is the last step's)

        def render_frame(self, packed, layout, w, h, base, aa, out=None):
            out.fill_(rank + 1)

        def sync_frame(self, age):
            calls["sync_frame"] += 1
            return 0

        def sync(self):
            return 0

        def set_profiling(self, stages):
            self.prof = list(stages)

        def stage_ms(self):
            return {k: ((2.0 if k == "fine" else 0.5), 10) for k in vello_amd.renderer.STAGES}

        def bump(self):
            return {"failed": 0, "binning": 10, "ptcl": 1000, "tile": 100, "seg_counts": 50, "segments": 50, "blend": 0, "lines": 60}

        def fine_slice_stats(self):
            return 0, 0

        KERNELS = vello_amd.renderer.Engine.KERNELS

        def kernel_ms(self):
            return {k: (0.3, 10) for names in self.KERNELS.values() for k in names}

    vello_amd.Engine = FakeEngine
    real_scene = workloads.paris_like_scene
    workloads.paris_like_scene = lambda seed: real_scene(seed, n_paths=60, size=1600.0)
    real_d2 = workloads.paris_like_scene_d2
    workloads.paris_like_scene_d2 = lambda seed: real_d2(seed, n_paths=60, size=1600.0)

    sys.argv = ["bench.py", "--gpus", str(world), "--steps", "7", "--warmup", "2", *extra_args]
    buf = io.StringIO()
    real_stdout = sys.stdout
    sys.stdout = buf
    try:
        runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
    finally:
        sys.stdout = real_stdout
    lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("{")]
    with open(f"{out_path}.{rank}", "w") as fh:
        json.dump({"lines": lines, "calls": calls}, fh)


def test_bench_two_rank_control_flow(built, tmp_path):
    import json

    world = 2
    out = str(tmp_path / "bench")
    mp.spawn(_bench_worker, args=(world, _free_port(), out, ("--full",)), nprocs=world, join=True)
    r0 = json.load(open(out + ".0"))
    r1 = json.load(open(out + ".1"))
    assert len(r0["lines"]) == 1 and r1["lines"] == [], "rank 0 prints exactly ONE JSON line, other ranks none"
    line = json.loads(r0["lines"][0])
    assert line["n_gpus"] == 2 and line["steps"] == 7 and line["warmup"] == 2 and line["scaling"] == "weak"
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["vs_baseline"] is None
    # whole-job value: both ranks' frames over the max-over-ranks time
    assert abs(line["value"] - 2 * 7 / (line["ms_per_step"] * 7e-3)) / line["value"] < 1e-2
    assert line["config"]["parallelism"] == "scenes2" and line["config"]["exchange_alone_ms"] is not None
    assert len(line["config"]["per_rank_frames_per_s"]) == 2 and all(v > 0 for v in line["config"]["per_rank_frames_per_s"])
    assert "SURVEY 8d d2" in line["config"]["workload"] and "70 %" in line["config"]["workload"]
    assert "cpu_baseline" not in line or line["cpu_baseline"] is None or line["n_gpus"] == 1
    assert line["roofline"]["kernel"] == "k_fine"
    assert r0["calls"]["render"] >= 9 and r1["calls"]["render"] >= 9


@pytest.mark.parametrize("world", [1, 2])
def test_bench_plain_run_times_steps_and_dumps_outputs(built, tmp_path, world):
    """Without --full: warm-up + exactly --steps renders per rank, nothing beside them, the lean line, and --dump-outputs
    writes the last timed step's frame(s) (rank 0's gather at N > 1) as float32."""
    import json

    out = str(tmp_path / "bench")
    dump = str(tmp_path / "outputs")
    mp.spawn(_bench_worker, args=(world, _free_port(), out, ("--dump-outputs", dump)), nprocs=world, join=True)
    ranks = [json.load(open(f"{out}.{r}")) for r in range(world)]
    assert len(ranks[0]["lines"]) == 1 and all(r["lines"] == [] for r in ranks[1:])
    line = json.loads(ranks[0]["lines"][0])
    assert line["n_gpus"] == world and line["steps"] == 7 and line["warmup"] == 2
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f32+u32"
    assert abs(line["value"] - world * 7 / (line["ms_per_step"] * 7e-3)) / line["value"] < 1e-2
    assert "roofline" not in line and "cpu_baseline" not in line and "value_200_steps" not in line["config"]
    assert all(r["calls"]["render"] == 2 + 7 for r in ranks)  # (warm-up + timed steps, no other frame)
    last = 1 + 10 * (9 % 20)  # the fake engine's fill of its 9th render, plus the rank
    if world == 1:
        assert os.listdir(dump) == ["frame.npy"]
        frame = np.load(os.path.join(dump, "frame.npy"))
        assert frame.dtype == np.float32 and frame.shape == (1600, 1600, 4)
        assert (frame == last).all()
    else:
        assert os.listdir(dump) == ["frames.npy"]
        frames = np.load(os.path.join(dump, "frames.npy"))
        assert frames.dtype == np.float32 and frames.shape == (world, 1 << 20)  # (bench.DUMP_SAMPLE)
        for r in range(world):
            assert (frames[r] == last + r).all()
