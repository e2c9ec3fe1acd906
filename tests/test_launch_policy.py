"""The launch policy of the plan step (csrc/fx_policy.h) without a GPU: a stand-alone program (tests/policy_table.cpp) runs the pure
functions on every row of the recorded table -- profiles/policy/step_info_parent.json, written by tools/dump_step_info.py on an
MI355X at the commit named inside: sizes either side of every threshold, every force, batches, every refusal -- and must answer
what real contexts answered: the 16 numbers of fx_step_info_ex, or the refusal's error code and message.

The rows of the one-launch step depend on the device's occupancy answer in [11] - [13] and bit 16 of [15]; the recording keeps the
three answers next to the row, and the second test holds the pure sizing function to the recorded (steps per item, workgroups, LDS)."""
import importlib.util
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDING = os.path.join(ROOT, "profiles", "policy", "step_info_parent.json")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FORCE_ORDER = ("G", "wpe", "variant", "block", "mapping", "obst_stage", "obst_CH", "fused", "store", "step_kernel", "step_kernel_CH")
CAPS_ORDER = ("max_agents", "max_candidates", "max_steps", "max_ref_knots", "max_obstacles", "max_pred_steps")
AGENT_ORDER = ("N", "M", "K", "P", "mode", "nT", "nV", "nD", "n_rows", "matrix", "shard_begin", "shard_count", "n_bound", "have_hull")


_spec = importlib.util.spec_from_file_location("dump_step_info", os.path.join(ROOT, "tools", "dump_step_info.py"))
dump_step_info = importlib.util.module_from_spec(_spec)   # (the table, the recording's format and the runner of its rows)
_spec.loader.exec_module(dump_step_info)


def recorded_rows():
    with open(RECORDING) as f:
        return dump_step_info.unpack(json.load(f))


def row_text(r, second=False):
    """a row as tests/policy_table.cpp reads it; second: the step behind the recorded first one (it knows that one's costed candidates)"""
    occ, wg = r.get("occupancy", {}), r["env"]["FX_OBST_WG"]
    w = [r["name"] + ("#second" if second else "")] + [r["caps"][k] for k in CAPS_ORDER] + [r["force"][k] for k in FORCE_ORDER]
    w += [r["package"], r["last_live"] if second else -1, occ.get("3", 0), occ.get("5", 0), occ.get("8", 0), r["env"]["FX_LDS_PAD"],
          0 if wg < 0 else (2 if wg else 1), len(r["agents"])]
    for a in r["agents"]:
        w += [a[k] for k in AGENT_ORDER] + [len(a["cost_id"])] + a["cost_id"]
    return " ".join(str(x) for x in w)


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    """what the pure functions answer to every recorded row: name -> ("ok", 16 numbers, (CH, blocks, lds)) or ("err", code, message)"""
    exe = str(tmp_path_factory.mktemp("policy") / "policy_table")
    subprocess.run([HIPCC, "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Wno-unused-command-line-argument",
                    "-I", os.path.join(ROOT, "frenetix-motion-planner_amd", "csrc"), os.path.join(ROOT, "tests", "policy_table.cpp"), "-o", exe],
                   check=True)
    rows = recorded_rows()
    text = [row_text(r) for r in rows] + [row_text(r, second=True) for r in rows if "info_second" in r]
    out = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout
    got = {}
    for line in out.splitlines():
        name, kind, rest = line.split(" ", 2)
        if kind == "ok":
            v = [int(x) for x in rest.split()]
            got[name] = ("ok", v[:16], tuple(v[16:]))
        else:
            code, msg = rest.split(" ", 1)
            got[name] = ("err", int(code), msg)
    assert len(got) == len(text)
    return got


def test_table_covers_what_it_must():
    rows = recorded_rows()
    assert len(rows) >= 150
    assert len({r["name"] for r in rows}) == len(rows)
    assert sum("error" in r for r in rows) >= 10


def test_every_row_as_recorded(answers):
    wrong = []
    for r in recorded_rows():
        got = answers[r["name"]]
        if "error" in r:
            want = ("err", r["error"]["code"], r["error"]["message"])
            if got != want:
                wrong.append((r["name"], want, got))
            continue
        want, have = list(r["info"]), list(got[1]) if got[0] == "ok" else got
        if got[0] == "ok" and r["force"]["step_kernel"] == 2:   # what the device's occupancy answer decides: the second test
            for v in (want, have):
                v[11:14] = [0, 0, 0]
                v[15] &= ~(1 << 16)
        if have != want:
            wrong.append((r["name"], want, have))
    assert not wrong, f"{len(wrong)} rows differ from the recording (name, recorded, answered): {wrong[:12]}"


def test_one_launch_step_sizing_as_recorded(answers):
    rows = [r for r in recorded_rows() if "info" in r and r["force"]["step_kernel"] == 2]
    assert sum((r["info"][15] >> 16) & 1 for r in rows) >= 6 and any(not (r["info"][15] >> 16) & 1 for r in rows)
    wrong = []
    for r in rows:
        for name, info in ((r["name"], r["info"]), (r["name"] + "#second", r["info_second"])):
            ran = (info[15] >> 16) & 1
            want = (info[11], info[12] // 4, info[13]) if ran else (0, 0, 0)   # [12]: waves of 256-lane workgroups
            if answers[name][2] != want:
                wrong.append((name, want, answers[name][2]))
            if name.endswith("#second") and (answers[name][0] != "ok" or answers[name][1] != info):   # (with the occupancy: all 16)
                wrong.append((name, info, answers[name][1]))
    assert not wrong, wrong
