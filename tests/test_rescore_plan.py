"""The launch rule of the re-score pass (csrc/fx_rescore_plan.h, fx_rescore_plan) without a GPU: a stand-alone
program (tests/rescore_plan.cpp, built as test_item_rounds.py builds its program) answers a table of (candidates, vectors, forced
regime), and every answer is held to the rule's statement:

  * the regime follows the number of vectors alone: candidate per lane below FX_RESCORE_VECTOR_MIN vectors, vector per lane from
    there on, whatever the candidate count; a forced regime is taken as it is;
  * no launch dimension is zero, grid.x stays within 2^31 - 1 and grid.y within 65 535;
  * the chunks (groups) cover every vector and none is empty; the tiles (slices) cover every candidate and none is empty;
  * a lane-regime workgroup takes at most FX_RESCORE_CHUNK_MAX vectors -- what its LDS is declared for;
  * the partials are vectors x partials per vector.

The sizes the GPU tests are parametrised on (tests/rescore_planes.py) are derived from the header's constants here, so a change there
fails here instead of leaving the GPU tests beside the switch."""
import os
import subprocess

import pytest

from frenetix_motion_planner_amd import _abi
from tests import rescore_planes as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

CANDIDATES = (0, 1, 63, 64, 65, 255, 256, 257, 630, 4_097, 50_388, 1_000_000, (1 << 31) - 1, 1 << 31, 1 << 33)
VECTORS = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 256, 1_000, 32_767, 32_768)
CASES = [(n, w, f) for n in CANDIDATES for w in VECTORS for f in (0, 1, 2)]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rescore") / "rescore_plan")
    subprocess.run([HIPCC, "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Wno-unused-command-line-argument",
                    "-I", rp.CSRC, os.path.join(ROOT, "tests", "rescore_plan.cpp"), "-o", exe], check=True)
    text = "\n".join(f"{n} {w} {f}" for n, w, f in CASES) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0].startswith("constants ") and len(out) == 1 + len(CASES) and all(l.startswith("plan ") for l in out[1:])
    keys = ("lane", "vector", "tile", "chunk_max", "vector_min", "workgroups", "waves", "slice_min", "max_vectors")
    consts = dict(zip(keys, (int(x) for x in out[0].split()[1:])))
    plans = {c: dict(zip(("regime", "n_part", "per", "vec_chunk", "grid_y", "finish_blocks", "partials"), (int(x) for x in l.split()[1:])))
             for c, l in zip(CASES, out[1:])}
    return consts, plans


def test_sizes_follow_the_source(answers):
    consts, _ = answers
    k = rp.source_constants()
    assert consts == k                                                   # what the compiler sees is what the header's text says
    assert (k["lane"], k["vector"]) == (rp.LANE, rp.VECTOR) == (1, 2)
    assert k["vector_min"] == rp.VECTOR_MIN == 64 and k["tile"] == rp.TILE == 256
    assert {k["vector_min"] - 1, k["vector_min"], k["vector_min"] + 1, 1, 63, 64, 65} == set(rp.N_VECS)
    assert {1, 63, 64, 65, k["tile"] + 1} <= set(rp.SIZES) and max(rp.SIZES) > 16 * k["tile"] and max(rp.SIZES) % k["tile"] == 1
    assert k["max_vectors"] == _abi.FX_RESCORE_MAX_VECTORS and k["max_vectors"] <= 65_535 and max(VECTORS) == k["max_vectors"]
    assert k["chunk_max"] <= k["tile"]                                   # thread v of a workgroup combines the waves of its vector v


def test_the_regime_follows_the_vectors_alone(answers):
    consts, plans = answers
    for (n, w, f), p in plans.items():
        want = f if f else (rp.VECTOR if w >= consts["vector_min"] else rp.LANE)
        assert p["regime"] == want, (n, w, f, p)
    # both sides of the switch at every candidate count, and the switch is where the header says
    assert all(plans[(n, 63, 0)]["regime"] == rp.LANE and plans[(n, 64, 0)]["regime"] == rp.VECTOR for n in CANDIDATES)


def test_launch_dimensions(answers):
    consts, plans = answers
    for (n, w, f), p in plans.items():
        what = (n, w, f, p)
        assert 1 <= p["n_part"] and 1 <= p["grid_y"] <= 65_535 and 1 <= p["finish_blocks"] and 1 <= p["vec_chunk"] and 1 <= p["per"], what
        if n <= (1 << 31) - 1:
            assert p["n_part"] <= (1 << 31) - 1, what                    # (beyond: the entry point refuses, FX_ERR_CAPACITY)
        assert 4 * p["finish_blocks"] >= w > 4 * (p["finish_blocks"] - 1), what
        # every vector in a chunk, no chunk empty; every candidate in a tile or slice, none empty
        assert p["vec_chunk"] * p["grid_y"] >= w > p["vec_chunk"] * (p["grid_y"] - 1), what
        assert p["per"] * p["n_part"] >= n and (n == 0 or n > p["per"] * (p["n_part"] - 1)), what
        assert p["partials"] == w * p["n_part"], what
        if p["regime"] == rp.LANE:
            assert p["per"] == consts["tile"] and p["vec_chunk"] <= consts["chunk_max"], what
            assert p["n_part"] == max(1, -(-n // consts["tile"])), what
            # chunked finer only while the call is short of workgroups
            if p["vec_chunk"] < min(w, consts["chunk_max"]):
                coarser = min(2 * p["vec_chunk"], min(w, consts["chunk_max"]))
                assert p["n_part"] * -(-w // coarser) < consts["workgroups"], what
        else:
            assert p["vec_chunk"] == 64 and p["grid_y"] == -(-w // 64), what
            assert p["n_part"] * p["grid_y"] <= consts["waves"] + p["grid_y"], what
            assert n < consts["slice_min"] or 2 * p["per"] >= consts["slice_min"], what   # (slices of about slice_min at the least)


def test_shapes_of_the_measured_sizes(answers):
    """config 3 and the planner size at the vector counts tools/bench_rescore.py measures"""
    _, plans = answers
    p = plans[(50_388, 16, 0)]
    assert (p["regime"], p["n_part"], p["vec_chunk"], p["grid_y"]) == (rp.LANE, 197, 4, 4)
    p = plans[(50_388, 256, 0)]
    assert (p["regime"], p["grid_y"], p["n_part"], p["per"]) == (rp.VECTOR, 4, 509, 99)
    p = plans[(630, 1, 0)]
    assert (p["regime"], p["n_part"], p["vec_chunk"], p["grid_y"]) == (rp.LANE, 3, 1, 1)
    p = plans[(630, 256, 0)]
    assert (p["regime"], p["n_part"], p["per"]) == (rp.VECTOR, 20, 32)
