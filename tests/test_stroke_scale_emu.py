"""The per-frame stroke scale (vello_hip_set_stroke_scale) on the SIMT-emulated build of the kernel sources: k_style_widths' partitions
and alignments, rule 1's branches, the off state, every path a frame can take, the other per-frame inputs, frames in flight, queries,
run_stages, the refusals, the estimator and the bindings, against the CPU oracle on the substituted scene
(tests/stroke_scale_parity.py)."""
import pytest

from tests import morph_parity as mp
from tests import stroke_scale_parity as sp

MEM = mp.EmuMemory()


def _engine_factory():
    import vello_amd

    return lambda caps: vello_amd.Engine(capacities=caps)


@pytest.mark.parametrize("odd", [False, True])
@pytest.mark.parametrize("n", sp.PARTITIONS)
def test_emu_stroke_scale_partitions(emu_engine, n, odd):
    sp.check_partition(emu_engine, "emu_stroke_scale_part", n, odd)


def test_emu_stroke_scale_branches(emu_engine):
    sp.check_branches(emu_engine, "emu_stroke_scale_branches")


def test_emu_stroke_scale_off_state(emu_engine):
    sp.check_off_state(emu_engine, "emu_stroke_scale_off")


def test_emu_stroke_scale_front_fusion(emu_engine):
    sp.check_front_fusion(emu_engine, "emu_stroke_scale_front")


def test_emu_stroke_scale_tiny_fused(emu_engine):
    sp.check_tiny_fused(emu_engine, "emu_stroke_scale_tiny")


def test_emu_stroke_scale_indexed(emu_engine):
    sp.check_indexed(emu_engine, "emu_stroke_scale_indexed", back_half=False)


@pytest.mark.parametrize("stroke_kernel", [True, False])
def test_emu_stroke_scale_stroked_lines(emu_engine, stroke_kernel):
    sp.check_stroked_lines(emu_engine, "emu_stroke_scale_lines", stroke_kernel)


@pytest.mark.parametrize("which", ["flatten_coop", "flatten_alone"])
def test_emu_stroke_scale_curves(emu_engine, which):
    sp.check_curves(emu_engine, "emu_stroke_scale_curves", which)


def test_emu_stroke_scale_area(emu_engine):
    sp.check_area(emu_engine, "emu_stroke_scale_area")


@pytest.mark.slow
def test_emu_stroke_scale_tiger(emu_engine):
    sp.check_tiger(emu_engine, "emu_stroke_scale_tiger")


def test_emu_stroke_scale_view(emu_engine):
    sp.check_view(emu_engine, "emu_stroke_scale_view")


def test_emu_stroke_scale_culled(emu_engine):
    sp.check_culled(emu_engine, "emu_stroke_scale_culled")


def test_emu_stroke_scale_damage(emu_engine):
    sp.check_damage(emu_engine, "emu_stroke_scale_damage")


def test_emu_stroke_scale_morph(emu_engine):
    sp.check_morph(emu_engine, "emu_stroke_scale_morph")


def test_emu_stroke_scale_render_frame(emu_engine):
    sp.check_render_frame(emu_engine, "emu_stroke_scale_render_frame")


def test_emu_stroke_scale_instances_painted(emu_engine):
    sp.check_instances_painted(emu_engine, "emu_stroke_scale_instances")


def test_emu_stroke_scale_retained_painted(emu_engine):
    sp.check_retained_painted(emu_engine, "emu_stroke_scale_retained")


def test_emu_stroke_scale_in_flight(emu_engine):
    sp.check_in_flight(emu_engine, MEM, "emu_stroke_scale_in_flight")


def test_emu_stroke_scale_queries_and_stages(emu_engine):
    sp.check_queries_and_stages(emu_engine, "emu_stroke_scale_queries")


def test_emu_stroke_scale_refusals(emu_engine):
    sp.check_refusals(emu_engine, MEM, "emu_stroke_scale_refusals")


def test_emu_stroke_scale_estimator_and_auto_grow(emu_engine):
    sp.check_estimator(_engine_factory(), "emu_stroke_scale_estimate")


def test_emu_stroke_scale_engine_binding(emu_engine):
    sp.check_engine_binding(emu_engine, "emu_stroke_scale_binding")


def test_emu_stroke_scale_renderer_params(emu_engine):
    sp.check_renderer("emu_stroke_scale_renderer")


@pytest.mark.slow
def test_stroke_scale_host_paths_under_sanitizers(tmp_path):
    # tests/c_abi/stroke_scale_host.cpp drives the setting, its refusals, frames of every entry point under it and the styled estimate.
    # The program AND the engine's sources (their SIMT-emulated build, from a scratch copy of the tree: the in-tree build stays as it
    # is) are compiled with -fsanitize=address,undefined into ONE executable, so the sanitizers' runtime is the program's own: device
    # buffers are heap blocks there, and a style copy laid out or indexed one word wrong is a reported overflow.  A child process.
    import os
    import shutil
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    san = "-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer"
    (tmp_path / "tests").mkdir()
    shutil.copytree(os.path.join(root, "tests", "simt_emu"), tmp_path / "tests" / "simt_emu", ignore=shutil.ignore_patterns("build", "*.so"))
    shutil.copytree(os.path.join(root, "vello_amd", "csrc"), tmp_path / "vello_amd" / "csrc", ignore=shutil.ignore_patterns("build", "*.o"))
    shutil.copytree(os.path.join(root, "include"), tmp_path / "include")
    emu = str(tmp_path / "tests" / "simt_emu")
    flags = f"-O1 -g -std=c++17 -fPIC -ffp-contract=off -fno-fast-math -mfma -I . -x c++ {san} -Wno-unknown-pragmas"
    # (the objects only: the Makefile's own link step knows nothing of the sanitizers)
    objs = subprocess.run(["make", "-s", "-C", emu, "--eval", "print-obj: ; @echo $(OBJ)", "print-obj"], check=True, capture_output=True, text=True).stdout.split()
    assert any(o.endswith("frames.o") for o in objs) and any(o.endswith("scene_ops.o") for o in objs), objs
    r = subprocess.run(["make", "-s", "-j8", "-C", emu, f"CXXFLAGS={flags}", *objs], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    exe = str(tmp_path / "stroke_scale_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", *san.split(), os.path.join(root, "tests", "c_abi", "stroke_scale_host.cpp"),
                    *[os.path.join(emu, o) for o in objs], "-I", root, "-lpthread", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
