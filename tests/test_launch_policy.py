"""The launch policy of the plan step (csrc/fx_policy.h) without a GPU: a stand-alone program (tests/policy_table.cpp) runs the pure
functions on every row of the recorded table -- profiles/policy/step_info_parent.json, written by tools/dump_step_info.py on an
MI355X at the commit named inside: sizes either side of every threshold, every force, batches, every refusal -- and must answer
what real contexts answered: the 16 numbers of fx_step_info_ex, or the refusal's error code and message.

The rows of the one-launch step depend on the device's occupancy answer in [11] - [13] and bit 16 of [15]; the recording keeps the
three answers next to the row, and the second test holds the pure sizing function to the recorded (steps per item, workgroups, LDS).

The same program prints, for the rows' agents, the generic kernel's LDS sizes (fx_generic_base_lds, fx_generic_lds) -- held here to the
closed forms the launch sites spelled out before the rules were written once -- and walks of the passes' block layout (csrc/fx_pass.h,
FxBlockLayout), held to its rule: every part at a multiple of 256 bytes, at least 8 bytes long, none overlapping -- and the two
rules of the passes that work in items (fx_item_chunk_steps, fx_item_batch), held to closed forms derived from their statements."""
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
    got, lds, launch, layouts, items = {}, {}, {}, [], {}
    for line in out.splitlines():
        name, kind, rest = (line.split(" ", 2) + [""])[:3]
        if name == "#layout":
            v = [int(x) for x in line.split()[1:]]
            assert len(v) == 2 * v[0] + 2
            layouts.append((v[1:1 + v[0]], v[1 + v[0]:1 + 2 * v[0]], v[-1]))
        elif name == "#items":
            v = [int(x) for x in rest.split()]
            items[(kind,) + tuple(v[:-1])] = v[-1]
        elif kind == "lds":
            v = [int(x) for x in rest.split()]
            lds[name] = [tuple(v[i:i + 6]) for i in range(0, len(v), 6)]
        elif kind == "launch":
            launch[name] = tuple(int(x) for x in rest.split())
        elif kind == "ok":
            v = [int(x) for x in rest.split()]
            got[name] = ("ok", v[:16], tuple(v[16:]))
        else:
            code, msg = rest.split(" ", 1)
            got[name] = ("err", int(code), msg)
    assert len(got) == len(text) and len(lds) == len(text)
    got["#lds"], got["#launch"], got["#layouts"], got["#items"] = lds, launch, layouts, items
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


FX_REF_FIELDS, FX_TP = 8, 14   # csrc/fx_device.h: doubles per reference knot / per step of the time table in LDS


def generic_launch_lds(M, S, rec):
    """what fx_evaluate and fx_materialise_candidates_agent asked of the generic kernel's launch before fx_generic_lds"""
    return 8 * (M * FX_REF_FIELDS + FX_TP * S + ((M + 1) & ~1)) + rec


def generic_base_lds(M, S):
    """what the upload and the list pass held against the 160 KiB of a CU (minus 1 KiB) before they shared fx_generic_base_lds"""
    return (M * (FX_REF_FIELDS + 1) + 2 + FX_TP * S) * 8


def test_generic_lds_closed_forms(answers):
    rows = recorded_rows()
    agents = 0
    for r in rows:
        per_agent = answers["#lds"][r["name"]]
        assert len(per_agent) == len(r["agents"])
        for a, (M, S, rec, base, generic, generic_rec) in zip(r["agents"], per_agent):
            assert (M, S) == (a["M"], a["N"] + 1)
            assert base == generic_base_lds(M, S), (r["name"], M, S)
            assert generic == generic_launch_lds(M, S, 0) and generic_rec == generic_launch_lds(M, S, rec), (r["name"], M, S, rec)
            agents += 1
    launches = answers["#launch"]
    for name, (M, S, rec, lds) in launches.items():
        assert lds == generic_launch_lds(M, S, rec), name
    # the table reaches what the forms depend on: odd and even knot counts, several horizons, launches with staged records
    assert agents >= 150 and len(launches) >= 10 and any(v[2] > 0 for v in launches.values())
    assert {M & 1 for per in answers["#lds"].values() for (M, *_r) in per} == {0, 1}
    assert len({S for per in answers["#lds"].values() for (_m, S, *_r) in per}) >= 2
    assert any(rec > 0 for per in answers["#lds"].values() for (_m, _s, rec, *_r) in per)


def test_block_layout_rule(answers):
    layouts = answers["#layouts"]
    assert any(sorted(parts) == [0, 1, 255, 256, 257] for parts, _o, _t in layouts) and any(not parts for parts, _o, _t in layouts)
    for parts, offs, total in layouts:
        at = 0
        for b, o in zip(parts, offs):
            assert o % 256 == 0 and o == at, (parts, offs)      # aligned, and the first free byte: no overlap, no hole beyond the padding
            room = -(-max(b, 8) // 256) * 256                    # at least 8 bytes, whole 256-byte units
            assert room >= max(b, 8) and room - max(b, 8) < 256
            at = o + room
        assert total == at and total % 256 == 0, (parts, offs, total)
        spans = sorted((o, o + max(b, 8)) for b, o in zip(parts, offs))
        assert all(e0 <= s1 for (_s0, e0), (s1, _e1) in zip(spans, spans[1:])), (parts, offs)


def test_item_rules_closed_forms(answers):
    """Steps per chunk: as many as keep a call at 4096 items or more -- one at the planner's grid (34 tiles x 8 obstacles x 15 pairs
    of steps = 4080 items, too few to double), the whole horizon at config 3 -- a forced size capped at the horizon, one step where
    there is none.  Candidates per batch: whole tiles of 64 within 64 MiB of scratch -- 64 MiB // 33600 B // 64 = 31 tiles -- never
    fewer than one tile, never more tiles than the call has."""
    items = answers["#items"]
    want = {("chunk", 2176, 31, 8, 0): 1, ("chunk", 50388, 31, 20, 0): 30,
            ("batch", 7 * 20 * 30 * 8, 2176): 1984, ("batch", 100, 1): 64, ("batch", 100, 0): 64, ("batch", 100, 65): 128,
            ("batch", 2 * (64 << 20), 1000): 64}
    for n, K in ((1, 1), (2176, 8), (50388, 20)):
        want["chunk", n, 31, K, 99] = 30
    for n, K in ((1, 0), (2176, 8), (50388, 20)):
        want["chunk", n, 1, K, 0] = 1
    assert items == want
