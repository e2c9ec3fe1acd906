"""The launch rule of the hypotheses pass (csrc/fx_hypotheses_plan.h, fx_hypotheses_plan) without a GPU: a
stand-alone program (tests/hypotheses_plan.cpp, built as test_rescore_plan.py builds its program) answers a table of (candidates,
samples, obstacles, steps per item, hypotheses, scratch limit), and every answer is held to the rule's statement:

  * an item is one (tile of 64 candidates, chunk of CH steps): tiles cover every candidate, chunks every step 1 .. S - 1, the last
    chunk may be short; the finish launch has one workgroup per 256 candidates;
  * a round holds as many hypotheses as keep its tables plus its scratch within the limit, at least one, and never more than the
    call has or a launch's grid.y holds; the rounds cover every hypothesis and none is empty;
  * three launches per round;
  * the parts of a hypothesis' table do not overlap, hold what pack_obstacle_tables writes, and the table is whole 256-byte lines."""
import os
import re
import subprocess

import pytest

from frenetix_motion_planner_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frenetix-motion-planner_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

CANDIDATES = (0, 1, 63, 64, 65, 630, 50_388)
HYPS = (1, 2, 13, 64, 1_024, 4_096)
SHAPES = ((31, 20, 3), (31, 5, 3), (31, 64, 5), (32, 7, 2), (2, 1, 3), (128, 64, 2))      # (S, K, CH)
LIMITS = (64 << 20, 1 << 20, 1)
CASES = [(c, s, k, ch, h, lim) for c in CANDIDATES for (s, k, ch) in SHAPES for h in HYPS for lim in LIMITS]
CASES += [((1 << 31) * 64, 31, 5, 3, 1, 64 << 20)]         # one hypothesis' items do not fit a launch


def pad(b):
    return (max(b, 8) + 255) // 256 * 256


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hypotheses") / "hypotheses_plan")
    subprocess.run([HIPCC, "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Wno-unused-command-line-argument",
                    "-I", CSRC, os.path.join(ROOT, "tests", "hypotheses_plan.cpp"), "-o", exe], check=True)
    text = "\n".join(" ".join(str(x) for x in c) for c in CASES) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0].startswith("constants ") and len(out) == 1 + 2 * len(CASES)
    consts = dict(zip(("max", "grid_y", "finish_tile", "hot_stride", "launches_per_round"), (int(x) for x in out[0].split()[1:])))
    pk = ("ok", "CH", "NC", "n_tiles", "items", "n_part", "table_words", "scratch_bytes", "per_round", "rounds", "launches")
    tk = ("hot", "rec", "pm", "hm", "margin", "words")
    plans = {}
    for c, lp, lt in zip(CASES, out[1::2], out[2::2]):
        assert lp.startswith("plan ") and lt.startswith("table ")
        plans[c] = (dict(zip(pk, (int(x) for x in lp.split()[1:]))), dict(zip(tk, (int(x) for x in lt.split()[1:]))))
    return consts, plans


def test_constants_follow_the_sources(answers):
    consts, _ = answers
    dev = open(os.path.join(CSRC, "fx_device.h")).read()
    assert consts["hot_stride"] == int(re.search(r"#define FX_HOT_STRIDE (\d+)", dev).group(1))
    assert consts["max"] == _abi.FX_HYPOTHESES_MAX >= 1024
    hdr = open(os.path.join(ROOT, "include", "fxplan.h")).read()
    assert int(re.search(r"#define FX_HYPOTHESES_MAX (\d+)", hdr).group(1)) == consts["max"]
    assert consts["grid_y"] == 65_535 and consts["finish_tile"] == 256 and consts["launches_per_round"] == 3
    # the default limit of a round is the passes' FX_ITEM_SCRATCH_BYTES
    api = open(os.path.join(CSRC, "fx_api_hypotheses.hip")).read()
    assert "limit_forced ? limit_forced : FX_ITEM_SCRATCH_BYTES" in api
    assert re.search(r"#define FX_ITEM_SCRATCH_BYTES \(\(size_t\)64 << 20\)", open(os.path.join(CSRC, "fx_pass.h")).read())


def test_every_case_follows_the_rule(answers):
    consts, plans = answers
    for (C, S, K, CH, H, limit), (p, t) in plans.items():
        if C >= (1 << 31) * 64:
            assert p["ok"] == 0 and p["items"] > (1 << 31) - 1
            continue
        ld = (max(C, 1) + 63) // 64 * 64
        steps = S - 1
        assert p["ok"] == 1 and p["CH"] == CH
        assert p["NC"] == max(-(-steps // CH), 1) and p["NC"] * CH >= steps and (p["NC"] - 1) * CH < max(steps, 1)
        assert p["n_tiles"] == max(-(-C // 64), 1) and p["n_tiles"] * 64 <= ld
        assert p["items"] == p["n_tiles"] * p["NC"] and 0 < p["items"] <= (1 << 31) - 1
        assert p["n_part"] == max(-(-C // 256), 1)
        # the table: hot | rec | pmask | hmask | margin, consecutive, whole 256-byte lines
        assert (t["hot"], t["rec"], t["pm"], t["hm"], t["margin"]) == (0, S * K * 10, S * K * 22, S * K * 22 + S, S * K * 22 + 2 * S)
        assert t["words"] * 8 == pad((t["margin"] + 1) * 8) and p["table_words"] == t["words"]
        scratch = pad(8 * p["NC"] * ld) + pad(8 * p["NC"] * p["n_tiles"]) + pad(8 * ld) + pad(ld) + 2 * pad(8 * p["n_part"])
        assert p["scratch_bytes"] == scratch
        each = 8 * p["table_words"] + scratch
        # the scratch bound: a round stays within the limit, or holds one hypothesis; one more would not have fitted
        assert 1 <= p["per_round"] <= min(H, consts["grid_y"])
        assert p["per_round"] * each <= limit or p["per_round"] == 1
        assert p["per_round"] == H or (p["per_round"] + 1) * each > limit
        assert p["rounds"] == -(-H // p["per_round"]) and (p["rounds"] - 1) * p["per_round"] < H
        assert p["launches"] == 3 * p["rounds"]


def test_the_sizes_of_the_issue(answers):
    """config 3 (50 388 candidates, 20 obstacles, 31 samples) and the planner's 630 x 5 at three steps per item"""
    _, plans = answers
    p, _ = plans[(50_388, 31, 20, 3, 1, 64 << 20)]
    assert (p["NC"], p["n_tiles"], p["items"], p["n_part"], p["rounds"], p["launches"]) == (10, 788, 7_880, 197, 1, 3)
    p, _ = plans[(50_388, 31, 20, 3, 1_024, 64 << 20)]
    assert p["per_round"] == (64 << 20) // (8 * p["table_words"] + p["scratch_bytes"]) == 14 and p["rounds"] == 74 and p["launches"] == 222
    p, _ = plans[(630, 31, 5, 3, 1_024, 64 << 20)]
    assert p["per_round"] == 775 and p["rounds"] == 2
    p, _ = plans[(630, 31, 5, 3, 2, 64 << 20)]
    assert (p["per_round"], p["rounds"], p["launches"]) == (2, 1, 3)
    for C in (1, 63, 64, 65):
        p, _ = plans[(C, 31, 5, 3, 2, 64 << 20)]
        assert p["n_tiles"] == (2 if C == 65 else 1) and p["items"] == 10 * p["n_tiles"] and p["n_part"] == 1
