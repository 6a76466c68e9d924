"""The frame lanes' streams on the MI355X: the lanes of a context are created with one stream priority that is not the
default's, so that they sit in a pool of hardware queues of their own.  Nothing a frame computes may depend on that: frames in flight
at every depth, after changes of depth, on two contexts, behind image uploads and behind a caller's pose stream are held bit for bit
to the same frames rendered one at a time -- which the existing suite holds to the oracle -- and the placement rule itself is read
through vello_hip_lane_stream_priority, in this process and in a child with VELLO_HIP_DEBUG_LANE_QUEUES=default."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import vello_amd
import workloads
from vello_amd import AaConfig, Affine, ImageBrush, ImageData, ImageQuality, Rect, Scene
from vello_amd.scene import Fill

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHITE = 0xFFFFFFFF
W = H = 128
AA = AaConfig.Msaa16
MAX_LANES = 8


def _targets(n, w=W, h=H):
    import torch

    t = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0") for _ in range(n)]
    torch.cuda.synchronize()  # (the engine's streams do not wait for torch's)
    return t


def _numpy(t):
    return t.cpu().numpy()


_SMALL = []


@pytest.fixture()
def small_scene(gpu_engine):
    """A few dozen paths, fills and strokes, and the image one frame at a time draws of it (computed once -- behind gpu_engine, which
    skips without a device -- and never written to)."""
    if not _SMALL:
        _SMALL.append(_small_scene())
    return _SMALL[0]


def _small_scene():
    packed, layout = workloads.random_test_scene(41, n_paths=48, size=float(W), strokes=True).resolve()
    eng = vello_amd.Engine(device=0)
    eng.upload_scene(packed, layout)
    out, = _targets(1)
    eng.render_resident(W, H, WHITE, AA, out=out)
    assert eng.sync() == 0
    ref = _numpy(out)
    ref.setflags(write=False)
    assert len(np.unique(ref.reshape(-1, 4), axis=0)) > 8, "the scene draws next to nothing"
    return packed, layout, ref


def _round_robin(eng, n, ref, what):
    """2n frames of the resident scene round-robin into n targets with n frames in flight; every one is `ref`."""
    eng.set_frames_in_flight(n)
    outs = _targets(n)
    for i in range(2 * n):
        eng.render_resident(W, H, WHITE, AA, out=outs[i % n])
    assert eng.sync() == 0, f"{what}: {eng.bump()}"
    for k, o in enumerate(outs):
        assert np.array_equal(_numpy(o), ref), f"{what}: target {k} of {n} differs from the one-at-a-time image"


@pytest.mark.parametrize("n", range(1, MAX_LANES + 1))
def test_gpu_every_depth(gpu_engine, small_scene, n):
    packed, layout, ref = small_scene
    gpu_engine.upload_scene(packed, layout)
    _round_robin(gpu_engine, n, ref, f"depth {n}")


def test_gpu_changing_depth(gpu_engine, small_scene):
    packed, layout, ref = small_scene
    gpu_engine.upload_scene(packed, layout)
    for n in (1, 4, 1, 8):
        _round_robin(gpu_engine, n, ref, f"depth 1 -> 4 -> 1 -> 8, at {n}")


def test_gpu_two_contexts(gpu_engine, small_scene):
    packed, layout, ref = small_scene
    other_packed, other_layout = workloads.random_test_scene(42, n_paths=40, size=float(W), strokes=True).resolve()
    solo = vello_amd.Engine(device=0)
    solo.upload_scene(other_packed, other_layout)
    o, = _targets(1)
    solo.render_resident(W, H, WHITE, AA, out=o)
    assert solo.sync() == 0
    other_ref = _numpy(o)
    del solo
    a, b = gpu_engine, vello_amd.Engine(device=0)
    a.upload_scene(packed, layout)
    b.upload_scene(other_packed, other_layout)
    a.set_frames_in_flight(3)
    b.set_frames_in_flight(3)
    outs_a, outs_b = _targets(3), _targets(3)
    for i in range(6):
        a.render_resident(W, H, WHITE, AA, out=outs_a[i % 3])
        b.render_resident(W, H, WHITE, AA, out=outs_b[i % 3])
    assert a.sync() == 0 and b.sync() == 0
    for k in range(3):
        assert np.array_equal(_numpy(outs_a[k]), ref), f"first context, target {k}"
        assert np.array_equal(_numpy(outs_b[k]), other_ref), f"second context, target {k}"


def test_gpu_image_upload_and_override(gpu_engine):
    """Every frame is preceded by a host upload of one image and a device copy into the other's place (the upload stream, lane_mark and
    atlas_ready): frame i shows texel set i, with four frames in flight as one at a time."""
    import torch

    rng = np.random.default_rng(17)
    steps = 8
    host_px = rng.integers(0, 256, size=(steps, 24, 32, 4), dtype=np.uint8)
    dev_px = torch.from_numpy(rng.integers(0, 256, size=(steps, 20, 28, 4), dtype=np.uint8)).to("cuda:0")
    uploaded, overridden = ImageData(host_px[0]), ImageData.empty(28, 20)
    s = Scene()
    s.fill(Fill.NonZero, Affine.translate(6.0, 8.0) * Affine.rotate(0.2) * Affine.scale(1.5), ImageBrush(uploaded, quality=ImageQuality.Medium), None,
           Rect(0.0, 0.0, 32.0, 24.0))
    s.fill(Fill.NonZero, Affine.translate(60.0, 50.0) * Affine.scale(2.0), ImageBrush(overridden, quality=ImageQuality.Low), None, Rect(0.0, 0.0, 28.0, 20.0))
    s.append(workloads.random_test_scene(43, n_paths=24, size=float(W), strokes=True))
    r = vello_amd.Resolver().resolve(s)
    (hx, hy, _), = r.uploads
    (dx, dy, dw, dh, _), = r.device_uploads
    eng = gpu_engine
    eng.resize_image_atlas(r.atlas_size, r.atlas_size)
    eng.upload_scene(r.packed, r.layout, ramps=r.ramps)
    torch.cuda.synchronize()

    def frames(n):
        eng.set_frames_in_flight(n)
        outs = _targets(steps)
        for i in range(steps):
            eng.write_image(hx, hy, host_px[i])
            eng.copy_images_device([(dx, dy, dw, dh, dev_px[i], dw * 4)])
            eng.render_resident(W, H, WHITE, AA, out=outs[i])
            if n == 1:
                assert eng.sync() == 0
        assert eng.sync() == 0
        return [_numpy(o) for o in outs]

    alone = frames(1)
    assert not np.array_equal(alone[0], alone[1]), "the texel sets do not show"
    for i, (got, ref) in enumerate(zip(frames(4), alone)):
        assert np.array_equal(got, ref), f"frame {i} with four in flight differs from the one-at-a-time frame"


def test_gpu_retained_list_behind_a_pose_stream(gpu_engine):
    """A retained list whose poses a torch op writes on another stream (pose_stream, pose_mark), four frames in flight."""
    import torch

    from tests import instance_parity as ip
    from tests import retained_parity as rp

    eng = gpu_engine
    lib = vello_amd.FragmentLibrary([ip.polygon(5), ip.polygon(8)])
    lib.upload(eng)
    inst = ip.scatter(np.random.default_rng(3), 12, 2, W, H, scale=(0.8, 2.0))
    eng.retain_instances(inst)
    steps = 8
    poses = [torch.from_numpy(np.ascontiguousarray(rp.turned(inst, W, H, k), dtype=np.float32)).to("cuda:0") for k in range(steps)]
    torch.cuda.synchronize()
    alone = []
    out, = _targets(1)
    for k in range(steps):
        eng.render_retained(W, H, WHITE, AA, transforms=poses[k], out=out)
        assert eng.sync() == 0
        alone.append(_numpy(out))
    assert not np.array_equal(alone[0], alone[1]), "the poses do not show"
    eng.set_frames_in_flight(4)
    outs = _targets(steps)
    written = [torch.zeros_like(p) for p in poses]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for k in range(steps):
            written[k].copy_(poses[k] * 1.0)  # (a kernel on the side stream writes the poses)
            eng.render_retained(W, H, WHITE, AA, transforms=written[k], out=outs[k], src_stream=side)
    assert eng.sync() == 0
    side.synchronize()
    for k in range(steps):
        assert np.array_equal(_numpy(outs[k]), alone[k]), f"frame {k} with four in flight differs from the one-at-a-time frame"


def _null_stream_priority():
    import ctypes

    import torch

    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    p = ctypes.c_int(12345)
    assert hip.hipStreamGetPriority(None, ctypes.byref(p)) == 0
    return p.value


def test_gpu_placement_rule(gpu_engine):
    eng = gpu_engine
    eng.set_frames_in_flight(MAX_LANES)
    seen = [eng.lane_stream_priority(lane) for lane in range(MAX_LANES)]
    priorities = {p for p, _, _ in seen}
    (least, greatest), = {(lo, hi) for _, lo, hi in seen}
    assert len(priorities) == 1, f"the lanes' priorities differ: {seen}"
    chosen, = priorities
    assert min(least, greatest) <= chosen <= max(least, greatest)
    null = _null_stream_priority()
    if least != greatest:
        assert chosen != null, f"the lanes share the null stream's priority {null} (range {least} .. {greatest})"
    else:
        assert chosen == null
    with pytest.raises(vello_amd.VelloHipError):
        eng.lane_stream_priority(MAX_LANES)
    # a lane out of the rotation keeps its stream
    eng.set_frames_in_flight(2)
    assert eng.lane_stream_priority(MAX_LANES - 1)[0] == chosen


_CHILD = """
import ctypes, json, os, sys
sys.path.insert(0, sys.argv[1])
import torch
import vello_amd
eng = vello_amd.Engine(device=0)
eng.set_frames_in_flight(8)
hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
p = ctypes.c_int(12345)
assert hip.hipStreamGetPriority(None, ctypes.byref(p)) == 0
print(json.dumps({"lanes": [eng.lane_stream_priority(k)[0] for k in range(8)], "null": p.value}))
"""


def test_gpu_placement_rule_default_seam(gpu_engine):
    env = dict(os.environ, VELLO_HIP_DEBUG_LANE_QUEUES="default")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["lanes"] == [got["null"]] * MAX_LANES, got


def test_gpu_unknown_seam_value_is_refused(gpu_engine, monkeypatch):
    monkeypatch.setenv("VELLO_HIP_DEBUG_LANE_QUEUES", "fastest")
    with pytest.raises(vello_amd.VelloHipError, match=r"\(-1\).*VELLO_HIP_DEBUG_LANE_QUEUES"):
        vello_amd.Engine(device=0)
