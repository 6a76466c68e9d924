"""The C-ABI library loads without a GPU and exports every symbol include/vello_hip.h declares;
create() fails loudly (no CPU fallback).  CPU only."""
import ctypes
import os
import re

import pytest

import vello_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "vello_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(vello_hip_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported(built):
    lib = ctypes.CDLL(vello_amd.library_path())
    syms = declared_symbols()
    assert len(syms) >= 18
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/vello_hip.h but not exported"


def test_struct_sizes_match_reference_layouts(built):
    from vello_amd._lib import Bump, Capacities, LayoutStruct, RenderParamsStruct

    assert ctypes.sizeof(LayoutStruct) == 40 and ctypes.sizeof(Bump) == 32
    assert ctypes.sizeof(RenderParamsStruct) == 16 and ctypes.sizeof(Capacities) == 28


def test_no_cpu_fallback_without_gpu(built):
    import torch

    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(vello_amd.VelloHipError, match="no CPU fallback"):
        vello_amd.Renderer()
    with pytest.raises(vello_amd.VelloHipError):
        vello_amd.Engine()


def test_product_never_imports_oracle():
    for dirpath, _, files in os.walk(os.path.join(ROOT, "vello_amd")):
        for f in files:
            if f.endswith((".py", ".cpp", ".hpp", ".h", ".hip")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "libvello_oracle" not in text and "import oracle" not in text and "from oracle" not in text, f
                assert "simt_emu" not in text or f == "_lib.py", f


def listed_kernels():
    """KERNELS of vello_amd/csrc/sources.mk: the engine/<name>.hip sources the library is built from."""
    text = open(os.path.join(ROOT, "vello_amd", "csrc", "sources.mk")).read()
    return re.search(r"^KERNELS\s*=(.*)$", text, flags=re.M).group(1).split()


def test_engine_tree_holds_only_built_sources():
    # every file under csrc/engine/ is a KERNELS source or reached by #include "..." from one: a copy of a kernel that the build
    # never compiles cannot sit beside the built ones (nor feed kernel_sources_hash()'s headers)
    engine = os.path.join(ROOT, "vello_amd", "csrc", "engine")
    todo, reached = [os.path.join(engine, k + ".hip") for k in listed_kernels()], set()
    while todo:
        f = os.path.normpath(todo.pop())
        if f not in reached:
            reached.add(f)
            text = open(f).read()
            todo += [os.path.join(os.path.dirname(f), inc) for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, flags=re.M)]
    present = {os.path.normpath(os.path.join(d, f)) for d, _, files in os.walk(engine) for f in files}
    assert sorted(present - reached) == []


def test_kernel_sources_hash_covers_what_is_built(tmp_path):
    # bench.py's roofline.traffic_stale: on a copy of the tree, a stray engine/*.hip leaves the hash as it is, an edit to a listed
    # source or a missing public header moves it
    import importlib.util
    import shutil

    from vello_amd._lib import kernel_sources_hash

    shutil.copytree(os.path.join(ROOT, "vello_amd", "csrc"), tmp_path / "vello_amd" / "csrc", ignore=shutil.ignore_patterns("build"))
    shutil.copy(os.path.join(ROOT, "vello_amd", "_lib.py"), tmp_path / "vello_amd")
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    spec = importlib.util.spec_from_file_location("lib_copy", tmp_path / "vello_amd" / "_lib.py")
    copy = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(copy)
    engine = tmp_path / "vello_amd" / "csrc" / "engine"
    h0 = copy.kernel_sources_hash()
    assert h0 == kernel_sources_hash()
    (engine / "x.hip").write_text((engine / "fine.hip").read_text() + "// a stray copy\n")
    assert copy.kernel_sources_hash() == h0
    listed = engine / (listed_kernels()[-1] + ".hip")
    listed.write_text(listed.read_text() + "// edited\n")
    h1 = copy.kernel_sources_hash()
    assert h1 != h0
    os.remove(tmp_path / "include" / "vello_hip.h")
    assert copy.kernel_sources_hash() not in (h0, h1)


def test_mask_luts_match_oracle(built):
    import numpy as np

    from oracle import oracle as O

    lib = vello_amd.load_library()
    l8 = np.zeros(1024, np.uint8)
    l16 = np.zeros(8192, np.uint8)
    lib.vello_hip_make_mask_lut(l8.ctypes.data)
    lib.vello_hip_make_mask_lut_16(l16.ctypes.data)
    assert np.array_equal(l8, O.make_mask_lut()) and np.array_equal(l16, O.make_mask_lut_16())


def test_cpp_example_builds_and_fails_loudly_without_a_gpu(built, tmp_path):
    # examples/hello_gradient.cpp: the host C++ mirror end to end (Scene -> Renderer::render_to_texture).  Here (no GPU)
    # it must build, link against the product library and refuse to run; linked against the emulated kernels (test
    # infrastructure) it must draw the scene.
    import subprocess

    import numpy as np
    import torch

    exe = str(tmp_path / "hello")
    src = os.path.join(ROOT, "examples", "hello_gradient.cpp")
    lib = os.path.join(ROOT, "vello_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", src, "-I", ROOT, "-L", lib, "-lvello_hip", f"-Wl,-rpath,{lib}", "-o", exe], check=True)
    if not torch.cuda.is_available():
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode == 2 and "no CPU fallback" in r.stderr
    emu = os.path.join(ROOT, "tests", "simt_emu")
    subprocess.run(["g++", "-std=c++17", "-O1", src, "-I", ROOT, "-L", emu, "-lvello_emu", f"-Wl,-rpath,{emu}", "-o", exe + "_emu"], check=True)
    out = str(tmp_path / "out.ppm")
    r = subprocess.run([exe + "_emu", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    data = open(out, "rb").read()
    header = b"P6\n512 512\n255\n"
    img = np.frombuffer(data[len(header):], dtype=np.uint8).reshape(512, 512, 3)
    assert tuple(img[10, 10]) == (26, 26, 31)            # base colour
    assert tuple(img[256, 300]) != tuple(img[256, 200])  # the sweep gradient varies around the centre
    assert tuple(img[256, 66]) == tuple(img[256, 446])   # the stroke-clipped ring, symmetric


def test_destroy_frees_every_device_buffer(built, tmp_path):
    # tests/c_abi/engine_lifecycle.cpp drives every allocator of the host driver once and destroys the context.  Only the program
    # is built with -fsanitize=address; linked against the emulated kernels, whose hipMalloc is calloc, LeakSanitizer sees any
    # device buffer or staging block that vello_hip_destroy forgets.  A child process of its own.
    import subprocess

    exe = str(tmp_path / "engine_lifecycle")
    src = os.path.join(ROOT, "tests", "c_abi", "engine_lifecycle.cpp")
    emu = os.path.join(ROOT, "tests", "simt_emu")
    # (the sanitizer's runtime is linked into the program itself: it is there first whatever else the process loads)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address", "-static-libasan", src, "-I", ROOT, "-L", emu, "-lvello_emu",
                    f"-Wl,-rpath,{emu}", "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "Sanitizer" not in r.stderr, r.stderr
