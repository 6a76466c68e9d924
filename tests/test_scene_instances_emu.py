"""Scene instances (vello_hip_upload_fragments / vello_hip_instances_layout / vello_hip_render_instances) on the SIMT-emulated build of
the kernel sources: k_compose_scene's bytes against a numpy composition, the composed frame against the CPU oracle through
compare_frame, life cycle and errors (tests/instance_parity.py).  The symbol map is the GPU suite's."""
import numpy as np
import pytest

from tests import instance_parity as ip


def _target(w, h):
    return np.zeros((h, w, 4), dtype=np.uint8)  # (stands for device memory in the emulated build)


def test_emu_instances_tag_shapes(emu_engine):
    ip.check_tag_shapes(emu_engine, "emu_inst_tags")


def test_emu_instances_many(emu_engine):
    ip.check_many(emu_engine, "emu_inst_many")


def test_emu_instances_one_tag_chunks(emu_engine):
    ip.check_one_tag_chunks(emu_engine, "emu_inst_one_tag")


@pytest.mark.parametrize("steps", [2, pytest.param(8, marks=pytest.mark.slow)])
def test_emu_instances_long_chunks(emu_engine, steps):
    ip.check_long_chunks(emu_engine, "emu_inst_long", steps)


def test_emu_instances_host_agreement(emu_engine):
    ip.check_host_agreement(emu_engine, "emu_inst_host")


@pytest.mark.parametrize("stroke_kernel", [True, False])
def test_emu_instances_polygons_polylines(emu_engine, stroke_kernel):
    ip.check_frame(emu_engine, f"emu_inst_lines_{int(stroke_kernel)}", ["polygons", "polylines"], flags={"stroke_kernel": stroke_kernel}, n=5, base=ip.WHITE)


@pytest.mark.parametrize("which", ["flatten_coop", "flatten_alone"])
def test_emu_instances_curves(emu_engine, which):
    ip.check_frame(emu_engine, f"emu_inst_curves_{which}", ["cardioid", "stroke_styles", "funky"], flags={which: True}, n=5, base=ip.WHITE,
                   in_flight=2 if which == "flatten_alone" else 1)


def test_emu_instances_brushes(emu_engine):
    ip.check_frame(emu_engine, "emu_inst_brushes", ["solid", "linear", "radial", "sweep", "image", "blur"], n=13)


def test_emu_instances_layers(emu_engine):
    ip.check_frame(emu_engine, "emu_inst_layers", ["clip", "blend", "clip_blend", "solid"], n=9)


def test_emu_instances_front_fusion(emu_engine):
    ip.check_front_fusion(emu_engine, "emu_inst_front")


def test_emu_instances_life_cycle(emu_engine):
    ip.check_life_cycle(emu_engine, "emu_inst_life", _target, lambda t: t)


def test_emu_instances_errors(emu_engine):
    ip.check_errors(emu_engine, "emu_inst_errors", _target, lambda t: t)


def test_instance_structs_match_header_and_shim():
    """vello_hip_fragment / vello_hip_instance have array fields: the header, the ctypes mirrors and the Rust shim agree on names, order,
    element types and lengths (and so on sizes: 48 and 28 bytes)."""
    import ctypes
    import os
    import re

    from vello_amd._lib import FragmentStruct, InstanceStruct

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(root, "include", "vello_hip.h")).read(), flags=re.S)
    rust = re.sub(r"//[^\n]*", "", open(os.path.join(root, "shim", "vello_hip", "src", "ffi.rs")).read())
    c_types = {"uint32_t": ("u32", ctypes.c_uint32), "float": ("f32", ctypes.c_float)}
    for name, mirror in (("vello_hip_fragment", FragmentStruct), ("vello_hip_instance", InstanceStruct)):
        body = re.search(r"struct %s \{(.*?)\};" % name, header, flags=re.S).group(1)
        want = []
        for decl in body.split(";"):
            m = re.match(r"\s*(\w+)\s+(\w+)(?:\[(\d+)\])?\s*$", decl)
            if m:
                want.append((m.group(2), m.group(1), int(m.group(3) or 1)))
        assert len(want) == (6 if name == "vello_hip_fragment" else 2)
        assert re.search(r"typedef struct %s %s;" % (name, name), header)
        rbody = re.search(r"pub struct %s \{(.*?)\}" % name, rust, flags=re.S).group(1)
        got_rust = [(f.split(":")[0].replace("pub", "").strip(), f.split(":")[1].strip()) for f in rbody.split(",") if ":" in f]
        assert got_rust == [(n, c_types[t][0] if k == 1 else f"[{c_types[t][0]}; {k}]") for n, t, k in want], (name, got_rust)
        got_py = [(n, t._type_, t._length_) if hasattr(t, "_length_") else (n, t, 1) for n, t in mirror._fields_]
        assert got_py == [(n, c_types[t][1], k) for n, t, k in want], (name, got_py)
        assert ctypes.sizeof(mirror) == sum(4 * k for _, _, k in want)
