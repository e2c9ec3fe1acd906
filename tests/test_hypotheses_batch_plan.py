"""The rows and rounds of the hypotheses pass over several agents (csrc/fx_hypotheses_batch_plan.h, fx_hypotheses_batch_plan;
DESIGN.md section 27) without a GPU: a stand-alone program (tests/hypotheses_batch_plan.cpp, built with the host compiler) answers a
list of calls, and every answer is held to the rule's statement:

  * a row's numbers are fx_hypotheses_plan's for its agent alone;
  * a round's tables plus scratch stay within the limit and none of its three flat grids exceeds 2^31 - 1 workgroups -- or it holds
    one pair; a round is closed only where the next pair would break one of the two;
  * the rounds cover every (agent, hypothesis) pair exactly once, in call order, a row being one agent's contiguous range;
  * the first-index arrays ascend from 0 and sum to the grids; the rows' scratch segments and tables do not overlap;
  * three launches per round; a forced tiny limit gives one pair per round."""
import os
import shutil
import subprocess

import pytest

from frenetix_motion_planner_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "frenetix-motion-planner_amd", "csrc")
CXX = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++") or "/opt/rocm/lib/llvm/bin/clang++"
GRID_MAX = (1 << 31) - 1
DEFAULT = 64 << 20

# the GPU test's context: (C, S, K, H) per agent
MIXED = [(1, 32, 1, 1), (63, 32, 4, 3), (64, 32, 7, 7), (65, 32, 20, 2), (257, 32, 2, 5), (65, 32, 64, 1)]
MANY = [(63 + (7 * i) % 68, 32, 1 + i % 5, 1 + i % 2) for i in range(129)]
HUGE = [(64 << 26, 33, 1, 2), (64 << 26, 33, 1, 2)]            # 2^30 items per hypothesis at two steps per item
CALLS = [(lim, ch, MIXED) for ch in (2, 3, 5) for lim in (DEFAULT, 1, 40_000, 100_000, 400_000)]
CALLS += [(DEFAULT, 3, MIXED[::-1]), (DEFAULT, 3, [MIXED[4], MIXED[0], MIXED[2]]), (DEFAULT, 3, MIXED[:1]), (DEFAULT, 3, [])]
CALLS += [(lim, 3, MANY) for lim in (DEFAULT, 1, 200_000)]
CALLS += [(DEFAULT, 3, [(630, 31, 5, h)] * 32) for h in (1, 4, 16, 4096)]
CALLS += [(1 << 62, 2, HUGE)]
REFUSED = [((DEFAULT, 3, [MIXED[0], (63, 32, 4, 0)]), 1, 1), ((DEFAULT, 3, [(63, 32, 4, -2), MIXED[0]]), 1, 0),
           ((DEFAULT, 3, [MIXED[0], MIXED[1], (64, 32, 7, 4097)]), 2, 2), ((DEFAULT, 3, [MIXED[0], ((1 << 31) * 64, 31, 5, 1)]), 3, 1)]
CALLS += [c for c, _, _ in REFUSED]


def pad(b):
    return (max(b, 8) + 255) // 256 * 256


@pytest.fixture(scope="module")
def answers(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hypotheses_batch") / "hypotheses_batch_plan")
    subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-I", CSRC,
                    os.path.join(ROOT, "tests", "hypotheses_batch_plan.cpp"), "-o", exe], check=True)
    text = "\n".join(f"{lim} {ch} {len(es)} " + " ".join(" ".join(str(x) for x in e) for e in es) for lim, ch, es in CALLS) + "\n"
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
    assert out[0].split() == ["constants", str(_abi.FX_HYPOTHESES_MAX), str(GRID_MAX), "3"]
    got, cur = [], None
    for l in out[1:]:
        w = l.split()
        if w[0] == "call":
            cur = dict(call=[int(x) for x in w[1:]], entry=[], row=[], round=[], locate=[])
            got.append(cur)
        else:
            cur[w[0]].append([int(x) for x in w[1:] if x != "|"])
    assert len(got) == len(CALLS)
    return got


def test_refusals_name_the_entry(answers):
    for (call, rc, bad) in REFUSED:
        a = answers[CALLS.index(call)]
        assert a["call"][:2] == [rc, bad] and not a["row"] and not a["round"]


def test_every_call_follows_the_rule(answers):
    n_checked = 0
    for (limit, CH, entries), a in zip(CALLS, answers):
        rc, _, ch, n, n_rows, n_rounds, pairs, table_bytes, scratch, launches = a["call"]
        if rc:
            continue
        n_checked += 1
        assert n == len(entries) == len(a["entry"]) and n_rows == len(a["row"]) and n_rounds == len(a["round"])
        assert pairs == sum(e[3] for e in entries) and launches == 3 * n_rounds
        if not entries:
            assert n_rows == n_rounds == pairs == 0
            continue
        assert ch == CH
        # a row's numbers are fx_hypotheses_plan's, and those are the rule's of section 25
        each, plan = [], []
        out0 = tab0 = 0
        for (C, S, K, H), e in zip(entries, a["entry"]):
            assert e[1:7] == e[9:15]
            ld = (max(C, 1) + 63) // 64 * 64
            NC, n_tiles, items, n_part, words, sb = e[1:7]
            assert NC == max(-(-(S - 1) // CH), 1) and n_tiles == max(-(-C // 64), 1) and items == NC * n_tiles <= GRID_MAX
            assert n_part == max(-(-C // 256), 1) and words * 8 == pad((S * K * 22 + 2 * S + 1) * 8)
            assert sb == pad(8 * NC * ld) + pad(8 * NC * n_tiles) + pad(8 * ld) + pad(ld) + 2 * pad(8 * n_part)
            assert e[7] == out0 and e[8] == tab0
            out0, tab0 = out0 + H, tab0 + H * words * 8
            each.append(words * 8 + sb)
            plan.append(dict(items=items, n_part=n_part, words=words, sb=sb, NC=NC, K=K))
        assert tab0 == table_bytes
        # the rows cover every pair exactly once, in call order
        seen = []
        for r in a["row"]:
            seen += [(r[0], h) for h in range(r[2], r[2] + r[3])]
            assert r[3] >= 1
        assert seen == [(i, h) for i, e in enumerate(entries) for h in range(e[3])]
        # the rounds: consecutive rows, ascending first indices from 0 that sum to the grids, the limits
        row_at = 0
        for k, (row0, nr, K_max, items, fins, prs, nbytes, scr) in enumerate(a["round"]):
            assert row0 == row_at and nr >= 1
            rows = a["row"][row0:row0 + nr]
            row_at += nr
            assert all(r[1] == k for r in rows) and K_max == max(plan[r[0]]["K"] for r in rows)
            assert len({r[0] for r in rows}) == nr                                 # an agent has at most one row per round
            i0 = f0 = s0 = sc0 = 0
            for r in rows:
                p = plan[r[0]]
                assert (r[4], r[5], r[6], r[8]) == (i0, f0, s0, sc0)
                i0, f0, s0, sc0 = i0 + r[3] * p["items"], f0 + r[3] * p["n_part"], s0 + r[3], sc0 + r[3] * p["sb"]
                assert r[10] <= r[3] * p["sb"]                                     # the row's arrays fit its segment
                assert r[7] == a["entry"][r[0]][8] + r[2] * p["words"] * 8 and r[9] == a["entry"][r[0]][7] + r[2]
            assert (items, fins, prs, scr) == (i0, f0, s0, sc0) and scr <= scratch
            assert nbytes == sum(r[3] * each[r[0]] for r in rows)
            assert prs >= 1 and (prs == 1 or (nbytes <= limit and max(items, fins, prs) <= GRID_MAX))
            if k + 1 < n_rounds:                                                   # closed only where the next pair would not fit
                nxt = a["row"][row_at][0]
                p = plan[nxt]
                assert nbytes + each[nxt] > limit or items + p["items"] > GRID_MAX or fins + p["n_part"] > GRID_MAX or prs + 1 > GRID_MAX
        assert row_at == n_rows and scratch == max(r[7] for r in a["round"])
        # the kernel's search and divisions find (row, hypothesis, tile, chunk) of a row's first and last item
        for (rnd, at, row, h, tile, chunk), want in zip(a["locate"], [(k, e) for k in range(n_rows if n_rows <= 64 else 0) for e in (0, 1)]):
            r = a["row"][want[0]]
            p = plan[r[0]]
            assert rnd == r[1] and row == want[0]
            assert (h, tile, chunk) == ((0, 0, 0) if want[1] == 0 else (r[3] - 1, p["items"] // p["NC"] - 1, p["NC"] - 1))
    assert n_checked == len(CALLS) - len(REFUSED)


def test_a_forced_tiny_limit_gives_one_pair_per_round(answers):
    for (limit, CH, entries), a in zip(CALLS, answers):
        if limit == 1:
            pairs = sum(e[3] for e in entries)
            assert len(a["round"]) == pairs == len(a["row"]) and a["call"][9] == 3 * pairs
            assert all(r[5] == 1 and r[1] == 1 for r in a["round"])


def test_the_shapes_the_cases_are_there_for(answers):
    by = {(lim, ch, tuple(es)): a for (lim, ch, es), a in zip(CALLS, answers)}
    # the mixed context under the default limit: one round, one row per agent, three launches
    a = by[(DEFAULT, 3, tuple(MIXED))]
    assert len(a["round"]) == 1 and len(a["row"]) == len(MIXED) and a["call"][9] == 3 and a["round"][0][2] == 64
    # middle limits: an agent's hypotheses cut across rounds, and several agents in one round
    a = by[(100_000, 3, tuple(MIXED))]
    cut = {r[0] for r in a["row"] if r[3] < MIXED[r[0]][3]}
    assert cut == {1, 2, 3, 4} and [rd[1] for rd in a["round"]][:2] == [2, 2] and len(a["round"]) == 11
    a = by[(400_000, 3, tuple(MIXED))]
    assert [rd[1] for rd in a["round"]] == [3, 3, 1, 1] and a["round"][3][2] == 64          # (what tests/test_hypotheses_batch_gpu.py forces)
    # more rows than a wave has lanes
    a = by[(DEFAULT, 3, tuple(MANY))]
    assert len(a["round"]) == 1 and a["round"][0][1] == 129
    # the grid limit alone closes rounds: 2^30 items per pair, two pairs do not share a launch
    a = by[(1 << 62, 2, tuple(HUGE))]
    assert [rd[3] for rd in a["round"]] == [1 << 30] * 4 and len(a["row"]) == 4 and [r[3] for r in a["row"]] == [1] * 4
    # the planner's batch: 32 agents x 630 candidates, one round up to 16 hypotheses each
    for h, rounds in ((1, 1), (4, 1), (16, 1)):
        a = by[(DEFAULT, 3, tuple([(630, 31, 5, h)] * 32))]
        assert len(a["round"]) == rounds and a["round"][0][3] == 32 * h * 100 and a["round"][0][5] == 32 * h
    a = by[(DEFAULT, 3, tuple([(630, 31, 5, 4096)] * 32))]
    assert len(a["round"]) > 32 and a["call"][6] == 32 * 4096


def test_the_sources_say_so():
    """three launches per round in the launcher, the default limit and the hook in the host entry, and no new host file"""
    api = open(os.path.join(CSRC, "fx_api_hypotheses.hip")).read()
    assert api.count("limit_forced ? limit_forced : FX_ITEM_SCRATCH_BYTES") == 2 and "fx_hypotheses_batch_plan(" in api
    k = open(os.path.join(CSRC, "fx_kernels.hip")).read()
    body = k[k.index('extern "C" hipError_t fx_launch_hypotheses_batch('):]
    body = body[:body.index("\n}\n") + 3]                                  # (the launcher's own text)
    assert body.count("hipLaunchKernelGGL(") == 3 and "return hipGetLastError();" in body
    hdr = open(os.path.join(CSRC, "fx_hypotheses_batch_plan.h")).read()
    assert '#include "fx_hypotheses_plan.h"' in hdr and "fx_hypotheses_plan(it.C" in hdr
