"""The launch table of the batched re-score (csrc/fx_rescore_batch_plan.h) without a GPU: a stand-alone program
(tests/rescore_batch_plan.cpp, built as test_rescore_plan.py builds its program) answers tables of entries, and every answer is held
to the table's statement:

  * every entry has the plan fx_rescore_plan gives it alone (the program of test_rescore_plan.py answers that), and its partial range
    is fx_rescore_partials of that plan; the ranges of a call do not overlap and fill the call's partial buffers;
  * the device table holds the lane-regime entries first, each regime in call order; the first workgroups ascend with the slot, from
    0 in each regime; the finish waves follow the slots, the outputs the call order;
  * every workgroup of a regime's launch maps back to exactly one (entry, tile or slice, chunk or group), and every such triple of
    an entry is hit exactly once;
  * no launch dimension of a launch that runs is zero;
  * n_vec < 1, more than FX_RESCORE_MAX_VECTORS vectors and a flat grid above 2^31 - 1 are refused, naming the entry."""
import os
import subprocess

import pytest

from frenetix_motion_planner_amd import _abi
from tests import rescore_planes as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GRID_MAX = (1 << 31) - 1

MANY = [(63 + (a * 7) % 68, (1, 2, 5, 63, 64, 65, 3, 70)[a % 8]) for a in range(129)]
CALLS = [
    (0, [(1, 65), (63, 1), (64, 64), (65, 63), (257, 2)]),          # the GPU test's shapes: both regimes
    (1, [(1, 65), (63, 1), (64, 64), (65, 63), (257, 2)]),          # ... every entry forced into the lane regime
    (2, [(1, 65), (63, 1), (64, 64), (65, 63), (257, 2)]),          # ... and into the vector regime
    (0, [(630, 16)] * 32), (0, [(630, 1)] * 32), (0, [(630, 256)] * 32), (0, [(10_488, 16)] * 5), (0, [(50_388, 16)]),   # the measured shapes
    (0, MANY[:65]), (0, MANY), (2, MANY), (1, MANY),
    (0, [(0, 1), (0, 64), (5, 3)]),                                  # agents without candidates: one empty partial per vector
    (0, [(630, 32_768), (630, 1)]),                                  # the most vectors an agent may have
    (0, []),
]
REFUSED = [
    ((0, [(630, 4), (630, 0)]), 1, 1), ((0, [(630, -3)]), 1, 0),
    ((0, [(630, 4), (63, 32_769), (1, 1)]), 2, 1),
    ((0, [(1 << 40, 1)]), 3, 0),                                     # tiles of one entry beyond a launch
    ((0, [((1 << 31) * 128, 2), ((1 << 31) * 128, 2), (64, 1)]), 3, 1),    # each entry fits, their sum does not
    ((1, [(1 << 37, 32_768)]), 3, 0),
]


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    d = tmp_path_factory.mktemp("rescore_batch")
    flags = [HIPCC, "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Wno-unused-command-line-argument", "-I", rp.CSRC]
    exe, one = str(d / "rescore_batch_plan"), str(d / "rescore_plan")
    subprocess.run(flags + [os.path.join(ROOT, "tests", "rescore_batch_plan.cpp"), "-o", exe], check=True)
    subprocess.run(flags + [os.path.join(ROOT, "tests", "rescore_plan.cpp"), "-o", one], check=True)
    calls = CALLS + [c for c, _, _ in REFUSED]
    text = "".join(f"{f} {len(es)} " + " ".join(f"{n} {w}" for n, w in es) + "\n" for f, es in calls)
    lines = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert lines[0].startswith("constants ")
    consts = [int(x) for x in lines[0].split()[1:]]
    out, cur = [], None
    for l in lines[1:]:
        kind, *v = l.split()
        v = [int(x) for x in v]
        if kind == "batch":
            cur = dict(zip(("rc", "bad", "n_lane", "n_vector", "lane_wgs", "vector_wgs", "partials", "vectors", "finish_blocks"), v), rows=[], wgs=[])
            out.append(cur)
        elif kind == "row":
            cur["rows"].append(dict(zip(("regime", "n_part", "per", "vec_chunk", "grid_y", "slot", "wg0", "part0", "fin0", "out0", "own_partials"), v)))
        else:
            assert kind == "wg"
            cur["wgs"].append(tuple(v))
    assert len(out) == len(calls)
    # the plan of every entry alone, from the per-agent rule's own program
    alone = sorted({(n, w, f) for f, es in CALLS for n, w in es})
    text = "".join(f"{n} {w} {f}\n" for n, w, f in alone)
    single = subprocess.run([one], input=text, capture_output=True, text=True, check=True).stdout.splitlines()[1:]
    plans = {k: [int(x) for x in l.split()[1:]] for k, l in zip(alone, single)}
    return consts, dict(zip(range(len(calls)), out)), plans


def test_constants(answers):
    consts, _, _ = answers
    assert consts == [_abi.FX_NUM_COSTS + 1, GRID_MAX, _abi.FX_RESCORE_MAX_VECTORS]


def test_every_entry_has_the_plan_it_has_alone(answers):
    _, out, plans = answers
    for k, (forced, entries) in enumerate(CALLS):
        t = out[k]
        assert t["rc"] == 0 and len(t["rows"]) == len(entries), (k, t["rc"])
        for (n, w), r in zip(entries, t["rows"]):
            regime, n_part, per, vec_chunk, grid_y, _, partials = plans[(n, w, forced)]
            assert (r["regime"], r["n_part"], r["per"], r["vec_chunk"], r["grid_y"], r["own_partials"]) == (regime, n_part, per, vec_chunk, grid_y, partials), (k, n, w)
            assert r["own_partials"] == w * r["n_part"]


def test_offsets_and_ranges(answers):
    _, out, _ = answers
    for k, (forced, entries) in enumerate(CALLS):
        t, rows = out[k], out[k]["rows"]
        E = len(entries)
        lane = [i for i, r in enumerate(rows) if r["regime"] == rp.LANE]
        vec = [i for i, r in enumerate(rows) if r["regime"] == rp.VECTOR]
        assert (t["n_lane"], t["n_vector"]) == (len(lane), len(vec)) and (forced == 0 or not (vec if forced == rp.LANE else lane))
        # the device table: lane entries first, each regime in call order
        assert [rows[i]["slot"] for i in lane + vec] == list(range(E))
        by_slot = lane + vec
        for group, total in ((lane, t["lane_wgs"]), (vec, t["vector_wgs"])):
            at = 0
            for i in group:
                assert rows[i]["wg0"] == at, (k, i)
                assert rows[i]["n_part"] >= 1 and rows[i]["grid_y"] >= 1            # no entry without a workgroup
                at += rows[i]["n_part"] * rows[i]["grid_y"]
            assert at == total <= GRID_MAX and (total > 0) == bool(group)           # no launch of zero workgroups runs
        # partial ranges: consecutive in slot order, disjoint, each the entry's own; finish waves follow the slots
        at = fin = 0
        for i in by_slot:
            assert rows[i]["part0"] == at and rows[i]["fin0"] == fin, (k, i)
            at += rows[i]["own_partials"]
            fin += entries[i][1]
        assert at == t["partials"] and fin == t["vectors"] == sum(w for _, w in entries)
        assert t["finish_blocks"] == -(-t["vectors"] // 4) and (E == 0 or t["finish_blocks"] >= 1)
        # outputs in call order
        at = 0
        for (n, w), r in zip(entries, rows):
            assert r["out0"] == at
            at += w


def test_every_workgroup_maps_back_to_one_place(answers):
    _, out, _ = answers
    checked = 0
    for k, (forced, entries) in enumerate(CALLS):
        t, rows = out[k], out[k]["rows"]
        for regime, total in ((rp.LANE, t["lane_wgs"]), (rp.VECTOR, t["vector_wgs"])):
            wgs = [w for w in t["wgs"] if w[0] == regime]
            if total > 100_000:      # (the program then answers the first and the last workgroup of every entry)
                for i, r in enumerate(rows):
                    if r["regime"] == regime:
                        last = r["wg0"] + r["n_part"] * r["grid_y"] - 1
                        assert (regime, r["wg0"], i, 0, 0) in wgs and (regime, last, i, r["n_part"] - 1, r["grid_y"] - 1) in wgs
                continue
            assert [w[1] for w in wgs] == list(range(total))
            seen = set()
            for _, wg, entry, part, chunk in wgs:
                r = rows[entry]
                assert r["regime"] == regime and 0 <= part < r["n_part"] and 0 <= chunk < r["grid_y"], (k, wg)
                assert wg == r["wg0"] + chunk * r["n_part"] + part
                seen.add((entry, part, chunk))
                # the workgroup has work: a vector in its chunk, and (but for an agent without candidates) a candidate in its part
                assert chunk * r["vec_chunk"] < entries[entry][1] and (entries[entry][0] == 0 or part * r["per"] < entries[entry][0])
            assert len(seen) == total == sum(r["n_part"] * r["grid_y"] for r in rows if r["regime"] == regime)
            checked += total
    assert checked > 10_000


def test_capacity_limits_are_refused(answers):
    _, out, _ = answers
    for j, (_, rc, bad) in enumerate(REFUSED):
        t = out[len(CALLS) + j]
        assert (t["rc"], t["bad"]) == (rc, bad) and not t["rows"], (j, t["rc"], t["bad"])


def test_the_rule_of_one_agent_is_not_repeated():
    """fx_rescore_plan.h states its constants and its condition once (tests/rescore_planes.py, source_constants); the batch header
    adds none of them"""
    rp.source_constants()
    hdr = open(os.path.join(rp.CSRC, "fx_rescore_batch_plan.h")).read()
    assert "FX_RESCORE_VECTOR_MIN" not in hdr and "#define FX_RESCORE_TILE" not in hdr and "fx_rescore_plan(" in hdr
