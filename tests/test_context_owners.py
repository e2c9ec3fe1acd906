"""The context's memory behind its owner types (csrc/fx_owner.h) without a GPU: a stand-alone program (tests/context_owners.cpp)
links the library's host sources -- those of the Makefile's `asan` target -- against its launcher stubs (csrc/fx_host_stubs.cpp,
here with stubs that succeed; a program overrides a launcher by defining it) and malloc-backed fakes of the HIP runtime calls that
create, upload and destroy make, and checks on the fakes' own table of blocks that create / destroy frees
everything exactly once, that a create with any one of its runtime calls failing returns an error, stores NULL and leaves nothing
behind, and that fx_device_bytes is the sum of the live device blocks across every grow site of an upload.  Built without
sanitizers here, the way tests/test_launch_policy.py builds its program."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frenetix-motion-planner_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
HOST_SOURCES = ("fx_api.hip", "fx_api_step.hip", "fx_api_exchange.hip", "fx_api_host.hip", "fx_api_risk.hip", "fx_api_materialise.hip",
                "fx_api_sort.hip", "fx_api_rescore.hip", "fx_api_hypotheses.hip")


def build_host_program(name, tmp_path):
    """tests/<name>.cpp with the host sources and the stubs, by the compiler's host pass; returns the executable"""
    exe = str(tmp_path / name)
    subprocess.run([HIPCC, "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Wno-unused-command-line-argument",
                    "-DFX_STUB_RESULT=hipSuccess", "-I", CSRC, "-I", os.path.join(ROOT, "include")] +
                   [os.path.join(CSRC, s) for s in HOST_SOURCES + ("fx_host_stubs.cpp",)] +
                   [os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe], check=True)
    return exe


def test_host_sources_are_the_asan_targets():
    with open(os.path.join(CSRC, "Makefile")) as f:
        line = next(l for l in f if "libfxplan_host_asan.so" in l)
    assert [w for w in line.split() if w.endswith(".hip")] == list(HOST_SOURCES)


def test_context_owners(tmp_path):
    run = subprocess.run([build_host_program("context_owners", tmp_path)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.startswith("ok"), run.stdout[-2000:] + run.stderr[-2000:]
