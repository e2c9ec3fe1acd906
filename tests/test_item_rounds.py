"""The round rule of a pass that works in items over several agents (csrc/fx_pass.h, fx_item_rounds) without a
GPU: a stand-alone program (tests/item_rounds.cpp, built as test_launch_policy.py builds policy_table.cpp) answers a table of
cases, and every answer is held to the rule's statement -- not to a second implementation of it:

  * every candidate of every agent lies in exactly one segment, the segments of an agent ascend and agents come in call order;
  * every segment but an agent's last is whole tiles of 64;
  * a round's scratch (whole tiles per segment, laid out without gaps or overlap) fits the limit unless the round is one
    oversized tile;
  * no round is closed while the next tile still fits.

The table of such a call (fx_item_table: what each row and each round of its launches covers) is answered by the same program on
the same cases and held to its statement in the same way; two more cases stand at the capacity of a launch.

The kernels find the row of an item or of a finish workgroup by "one load per 64 rows and a ballot" (row_of, batch_row_of): the
last row whose first index lies at or before it.  The program applies that rule, as a plain loop, to EVERY flat index of every
round's two launches and reports how many land outside the row whose extent holds them; tables of 64, 65, 129 and 130 agents --
with agents without candidates, or rows without items, at the positions 0, 63, 64 and last -- carry it past the 64-row boundary,
in one round and at a limit that puts more than 64 rows into one round: the host half of what the row search relies on."""
import os
import subprocess

import pytest

from frenetix_motion_planner_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
LIB_LIMIT = 64 << 20   # FX_ITEM_SCRATCH_BYTES: what fx_item_batch works on

PLANNER = 8 * 5 * 30          # bytes of scratch per candidate: 5 obstacles, 30 steps
CONFIG5 = 8 * 20 * 50
CASES = {
    # name: (limit, [(n, per_candidate_bytes), ...])
    "one planner-sized agent": (LIB_LIMIT, [(630, PLANNER)]),
    "one large agent, as fx_item_batch": (LIB_LIMIT, [(103_428, CONFIG5)]),
    "one agent of exact tiles": (LIB_LIMIT, [(64 * 1048, 8 * 1024)]),
    "many small agents in one round": (LIB_LIMIT, [(60, PLANNER), (256, 8), (315, 8 * 8 * 30), (2048, 8 * 20 * 30), (30, PLANNER)] * 2),
    "an agent spanning three rounds": (4 * 64 * PLANNER, [(100, PLANNER), (64 * 9 + 5, PLANNER), (60, PLANNER)]),
    "rounds closed inside and between agents": (5 * 64 * 100, [(64 * 3, 100), (64 * 3, 100), (65, 300), (1, 100)]),
    "a tile larger than the limit": (1000, [(130, 100), (10, 100)]),
    "an oversized tile behind small ones": (64 * 100 * 3, [(64, 100), (70, 1000), (64, 100)]),
    "no agents": (LIB_LIMIT, []),
    "agents without candidates": (LIB_LIMIT, [(0, PLANNER), (70, PLANNER), (0, PLANNER)]),
    "33 agents": (LIB_LIMIT, [(60, PLANNER)] * 32 + [(2048, 8 * 20 * 30)]),
    "33 agents, small rounds": (10 * 64 * PLANNER, [(60 + 7 * i, PLANNER) for i in range(33)]),
    "agents that need no scratch": (2 * 64 * PLANNER, [(630, 0), (130, PLANNER), (200, 0), (130, PLANNER)]),
}


# ---- beyond one wave of agents: (limit, agents) of 64, 65, 129 and 130 agents of one or two tiles each ----
WAVE_COUNTS = (64, 65, 129, 130)


def _many(A, holes, per_zero, rounds):
    """A agents of 30 ... 129 candidates; `holes`: the agents at the positions 0, 63, 64 and last have no candidate; per_zero: they
    need no scratch (their rows run no item); rounds "one": the library's limit; "several": what the tiles of the first 70 agents
    take (of the first 25 below 129 agents, where 65 rows in one round leave nothing for another)"""
    special = {0, 63, 64, A - 1}
    agents = [(0 if holes and i in special else 30 + 11 * (i % 10), 0 if per_zero and i in special else 8 * (1 + i % 4) * 30) for i in range(A)]
    if rounds == "one":
        return LIB_LIMIT, agents
    return sum(tiles(n) * 64 * per for n, per in agents[:70 if A >= 129 else 25]), agents


def tiles(count):
    return -(-count // 64)


WAVE_CASES = {f"{A} agents, {what}, {rounds}": _many(A, what == "agents without candidates", what == "rows without items", rounds)
              for A in WAVE_COUNTS for what in ("agents without candidates", "rows without items") for rounds in ("one", "several")}
CASES.update(WAVE_CASES)


def items_per_tile(a, per):
    """what the table function is told of every row of agent a (chunks x obstacles in the library): 0 exactly where the agent takes
    no scratch, otherwise a small count that differs from agent to agent"""
    return 0 if per == 0 else 5 * (1 + a % 3) + a % 2


# the launches' capacity: one agent of 4 096 tiles in one round, at 2^31 items and at the most a launch takes
CAPACITY = {
    "2^31 items": (LIB_LIMIT, [(4096 * 64, 8)], 1 << 19),
    "2^31 - 4096 items": (LIB_LIMIT, [(4096 * 64, 8)], (1 << 19) - 1),
}


@pytest.fixture(scope="module")
def program_output(tmp_path_factory):
    """per case the program's two lines as integers: (segments' line, table's line)"""
    exe = str(tmp_path_factory.mktemp("rounds") / "item_rounds")
    subprocess.run([HIPCC, "--cuda-host-only", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-Wno-unused-command-line-argument",
                    "-I", os.path.join(ROOT, "frenetix-motion-planner_amd", "csrc"), os.path.join(ROOT, "tests", "item_rounds.cpp"), "-o", exe],
                   check=True)
    cases = {name: (limit, [(n, per, items_per_tile(a, per)) for a, (n, per) in enumerate(agents)]) for name, (limit, agents) in CASES.items()}
    cases.update({name: (limit, [(n, per, ipt) for n, per in agents]) for name, (limit, agents, ipt) in CAPACITY.items()})
    text = "\n".join(" ".join(str(x) for x in [limit, len(agents)] + [v for a in agents for v in a]) for limit, agents in cases.values())
    out = subprocess.run([exe], input=text + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == 3 * len(cases)
    lines = [[int(x) for x in line.split()[1:]] for line in out]
    assert all(line.startswith("case ") for line in out[0::3]) and all(line.startswith("table ") for line in out[1::3])
    assert all(line.startswith("lookup ") for line in out[2::3])
    return dict(zip(cases, zip(lines[0::3], lines[1::3], lines[2::3])))


@pytest.fixture(scope="module")
def answers(program_output):
    got = {}
    for name in CASES:
        v = program_output[name][0]
        assert len(v) == 2 + 5 * v[0]
        got[name] = (v[1], [tuple(v[2 + 5 * k:7 + 5 * k]) for k in range(v[0])])   # (agent, round, first, count, scratch_off)
    return got


def parse_table(v):
    """the table's line: None where fx_item_table refused, else (scratch, rounds, rows, agent_row) with
    rounds (row0, n_rows, items, fin_blocks) and rows (nb, item0, fin0)"""
    if v[0] != 0:
        assert len(v) == 1
        return None
    scratch, n_rounds = v[1], v[2]
    at = 3
    rounds = [tuple(v[at + 4 * k:at + 4 * k + 4]) for k in range(n_rounds)]
    at += 4 * n_rounds
    n_rows = v[at]
    rows = [tuple(v[at + 1 + 3 * k:at + 4 + 3 * k]) for k in range(n_rows)]
    at += 1 + 3 * n_rows
    agent_row = v[at + 1:]
    assert len(agent_row) == v[at]
    return scratch, rounds, rows, agent_row


@pytest.mark.parametrize("name", list(CASES))
def test_rounds_follow_the_rule(answers, name):
    limit, agents = CASES[name]
    _, segs = answers[name]
    # call order, ascending, contiguous, complete; one segment per (agent, round); all but an agent's last are whole tiles
    assert segs == sorted(segs, key=lambda s: (s[0], s[2]))
    assert [s[1] for s in segs] == sorted(s[1] for s in segs) and len({(s[0], s[1]) for s in segs}) == len(segs)
    for a, (n, per) in enumerate(agents):
        mine = [s for s in segs if s[0] == a]
        at = 0
        for k, (_, _, first, count, _) in enumerate(mine):
            assert first == at and count > 0
            assert first % 64 == 0 and (count % 64 == 0 or k == len(mine) - 1)
            at += count
        assert at == n
    assert {s[0] for s in segs} <= set(range(len(agents)))
    # rounds count from 0 without a gap; the scratch of a round is laid out in segment order without gaps
    rounds = sorted({s[1] for s in segs})
    assert rounds == list(range(len(rounds)))
    used = {}
    for r in rounds:
        at = 0
        for a, _, first, count, off in [s for s in segs if s[1] == r]:
            assert off == at
            at += tiles(count) * 64 * agents[a][1]
        used[r] = at
        members = [s for s in segs if s[1] == r]
        scratch_tiles = sum(tiles(s[3]) for s in members if agents[s[0]][1] > 0)
        assert at <= limit or scratch_tiles == 1, (r, at)      # (fits, or is the one oversized tile -- beside tiles that need no scratch)
    # no round was closed while the next tile -- the first of the next round -- still fitted
    for r in rounds[1:]:
        a = [s for s in segs if s[1] == r][0][0]
        assert used[r - 1] + 64 * agents[a][1] > limit, r


def test_one_agent_is_fx_item_batch(answers):
    """a call of one agent at the library's limit: the batches of the per-agent pass"""
    for name in ("one planner-sized agent", "one large agent, as fx_item_batch", "one agent of exact tiles"):
        (limit, [(n, per)]), (batch, segs) = CASES[name], answers[name]
        assert limit == LIB_LIMIT and batch % 64 == 0 and batch > 0
        want = [(0, k, first, min(batch, n - first), 0) for k, first in enumerate(range(0, n, batch))]
        assert segs == want, name
    assert len(answers["one large agent, as fx_item_batch"][1]) == 13 and len(answers["one planner-sized agent"][1]) == 1


def test_the_cases_are_what_their_names_say(answers):
    assert {s[1] for s in answers["many small agents in one round"][1]} == {0} and len(answers["many small agents in one round"][1]) == 10
    spans = answers["an agent spanning three rounds"][1]
    assert [s[1] for s in spans if s[0] == 1] == [0, 1, 2] and spans[0][:2] == (0, 0) and spans[-1][:2] == (2, 3)
    big = answers["a tile larger than the limit"][1]
    assert [s[1:4] for s in big] == [(0, 0, 64), (1, 64, 64), (2, 128, 2), (3, 0, 10)]
    assert answers["no agents"][1] == [] and [s[0] for s in answers["agents without candidates"][1]] == [1]
    assert len(answers["33 agents"][1]) == 33 and {s[1] for s in answers["33 agents"][1]} == {0}
    assert len({s[1] for s in answers["33 agents, small rounds"][1]}) > 3
    # a tile of two agents shares a round: agent 0's two rounds end inside agent 1
    closed = answers["rounds closed inside and between agents"][1]
    assert [s[:2] for s in closed] == [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (3, 2)]


@pytest.mark.parametrize("name", list(CASES))
def test_table_follows_its_statement(program_output, answers, name):
    """fx_item_table on the segments of every case, every row of agent a with items_per_tile(a): held to the statement in fx_pass.h"""
    _, agents = CASES[name]
    _, segs = answers[name]
    scratch, rounds, rows, agent_row = parse_table(program_output[name][1])
    assert len(rows) == len(segs) and len(agent_row) == len(agents)
    # the rows of a round are consecutive, in call order, and exactly [row0, row0 + n_rows)
    assert len(rounds) == len({s[1] for s in segs})
    for r, (row0, n_rows, items, fin_blocks) in enumerate(rounds):
        mine = [k for k, s in enumerate(segs) if s[1] == r]
        assert mine == list(range(row0, row0 + n_rows)) and n_rows > 0
        item_at = fin_at = 0
        for k in mine:
            a, _, _, count, off = segs[k]
            nb, item0, fin0 = rows[k]
            assert nb == tiles(count) * 64                       # the count rounded up to whole tiles
            assert (item0, fin0) == (item_at, fin_at)            # from 0 at the round's first row; fin0 strictly ascends
            item_at += nb // 64 * items_per_tile(a, agents[a][1])   # (a row without items shares item0 with the row behind it)
            fin_at += -(-count // 256)
            assert fin_at > fin0
        assert (items, fin_blocks) == (item_at, fin_at)          # a round's items and finish workgroups are the sums
    # the scratch of the largest round, every row's segment whole tiles
    assert scratch == max([s[4] + rows[k][0] * agents[s[0]][1] for k, s in enumerate(segs)], default=0)
    # agent_row names a row of the agent, or is -1 exactly when the agent has no candidate
    for a, (n, _) in enumerate(agents):
        assert (agent_row[a] == -1) == (n == 0)
        assert agent_row[a] == -1 or segs[agent_row[a]][0] == a


def test_table_cases_cover_rows_without_items(program_output, answers):
    """the cases do hold rows without items in front of rows with some, and rounds of several rows: what the kernels' row search meets"""
    rows = parse_table(program_output["agents that need no scratch"][1])[2]
    segs = answers["agents that need no scratch"][1]
    shared = [k for k in range(len(rows) - 1) if segs[k][1] == segs[k + 1][1] and rows[k][1] == rows[k + 1][1]]
    assert shared and all(CASES["agents that need no scratch"][1][segs[k][0]][1] == 0 for k in shared)
    assert max(r[1] for r in parse_table(program_output["33 agents"][1])[1]) == 33


def test_a_round_beyond_a_launch_is_refused(program_output):
    """one agent of 4 096 tiles: 2^19 items per tile are 2^31 items, one more than a launch's grid takes; 2^19 - 1 are accepted"""
    assert program_output["2^31 items"][1] == [_abi.FX_ERR_CAPACITY]
    scratch, rounds, rows, agent_row = parse_table(program_output["2^31 - 4096 items"][1])
    assert rounds == [(0, 1, (1 << 31) - 4096, 1024)] and rows == [(4096 * 64, 0, 0)] and agent_row == [0]
    assert scratch == 4096 * 64 * 8


@pytest.mark.parametrize("name", list(CASES))
def test_row_search_finds_the_row_of_every_index(program_output, answers, name):
    """the kernels' rule -- the last row that starts at or before the index -- on every item and every finish workgroup of every
    round: the row whose [item0, item0 + items) / [fin0, fin0 + fin_blocks) holds the index; item0 and fin0 ascend within a round"""
    _, agents = CASES[name]
    scratch, rounds, rows, agent_row = parse_table(program_output[name][1])
    items, items_wrong, fins, fins_wrong, unsorted = program_output[name][2]
    assert (items, fins) == (sum(r[2] for r in rounds), sum(r[3] for r in rounds))       # every index of every launch was looked up
    assert (items_wrong, fins_wrong, unsorted) == (0, 0, 0)
    assert fins == sum(-(-s[3] // 256) for s in answers[name][1])


def test_wave_cases_are_what_their_names_say(program_output, answers):
    """the tables of 64 ... 130 agents do cross the 64-row boundary: a round of more than 64 rows wherever there are that many
    agents with candidates, further rounds of fewer behind it at the small limit, rows without items that share item0 with the row
    behind them at the positions 63 and 64, and items on both sides of the boundary"""
    for name, (limit, agents) in WAVE_CASES.items():
        A = len(agents)
        scratch, rounds, rows, agent_row = parse_table(program_output[name][1])
        segs = answers[name][1]
        with_rows = sum(n > 0 for n, _ in agents)
        assert len(agent_row) == A and [r >= 0 for r in agent_row] == [n > 0 for n, _ in agents]
        # agent_row names the agent's (last) row: rows are in call order, so the rows of the agents in front lie before it
        assert [segs[r][0] for r in agent_row if r >= 0] == [a for a, (n, _) in enumerate(agents) if n > 0]
        widest = max(r[1] for r in rounds)
        if name.endswith("one"):
            assert len(rounds) == 1 and widest == with_rows
        else:
            assert len(rounds) >= 2 and min(r[1] for r in rounds) < 64
        assert (widest > 64) == (with_rows > 64 and (name.endswith("one") or A >= 129)), (name, widest)
        if "rows without items" in name:
            r0 = rounds[0]
            special = [a for a in (0, 63, 64, A - 1) if a < r0[1]]      # (rows of round 0: one per agent, in call order)
            for a in special:
                assert agents[a][1] == 0 and segs[a][0] == a
                nxt = rows[a + 1][1] if a + 1 < r0[1] else r0[2]
                assert rows[a][1] == nxt, (name, a)                   # shares item0 with the row behind it (or ends the launch)
            if widest > 64:
                assert 0 < rows[63][1] and (r0[1] <= 66 or any(rows[k][1] > rows[65][1] for k in range(66, r0[1])))
        items = program_output[name][2][0]
        assert items == sum(tiles(s[3]) * items_per_tile(s[0], agents[s[0]][1]) for s in segs) > 0
