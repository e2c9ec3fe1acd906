"""The obstacle kernel's wave -> chunk map (csrc/fx_obstacle_kernel.h, FX_OBST_CHUNK_MAP): in a ten-wave workgroup of a ten-chunk
horizon the waves take their chunks through a fixed permutation instead of by index.  The split decomposition of the 50 388-candidate
step is forced on 135 candidates (tests/test_split_step_heads.py): every step is held to the CPU oracle, and its costs, flag words
and result to the same step with the map switched off (FX_OBST_CHUNK_INDEX=1, read with the upload) bit for bit -- the partials
meet in LDS by chunk and are added in chunk order, so the map may not show in any result.

Horizons: 31 samples (ten chunks: the map applies), 8 samples (three chunks, fewer waves than the map's span), 32 samples (eleven
chunks, the last one a single step), and batches of two agents whose horizons differ -- ten waves per workgroup with a three-chunk
agent beside the ten-chunk one, eleven waves with the eleven-chunk agent beside it (the map is off for the whole launch)."""
import numpy as np
import pytest

from frenetix_motion_planner_amd import synthetic
from tests.test_hip_parity import RESULT_KEYS, compare, hip_hulls

pytestmark = pytest.mark.gpu

GRID = (3, 5, 8)   # 3 x 5 x 9 = 135 candidates (the current lateral offset joins the eight sampled ones)
MAIN = dict(ref_kind="arc", v0=10.0, grid=GRID, n_obstacles=5, lead_gap=20.0)
SCENES = {
    "main": MAIN,                                                          # 29 costed candidates: half a tile
    "debug": dict(MAIN, draw_traj_set=True, kinematic_debug=True),         # all 135 costed: tiles of 64 + 64 + 7
    "s8": dict(MAIN, lead_gap=12.0, horizon=3.85, dt=0.55, n_pred=7),      # 8 samples: chunks of 3 + 3 + 1 steps
    "s32": dict(MAIN, horizon=3.1, n_pred=31),                             # 32 samples: eleven chunks, the last one step
    "second": dict(MAIN, seed=11, v0=8.0, lead_gap=15.0),
    "infeasible": dict(ref_kind="arc", kappa=0.05, v0=40.0, v_des=40.0, grid=GRID, n_obstacles=5),   # nothing costed: an empty list
}
CHUNKS = {"main": 10, "debug": 10, "s8": 3, "s32": 11, "second": 10, "infeasible": 10}


@pytest.fixture(scope="module")
def eng():
    from frenetix_motion_planner_amd.engine import FrenetEngine
    e = FrenetEngine(max_candidates=4096, max_steps=32, max_ref_knots=1024, max_obstacles=64, max_pred_steps=64, max_agents=4)
    e.set_tuning(2, 2, 2, 0, 2)   # two lanes per candidate, two waves per SIMD, grid kernel, wave split
    e.set_obstacle_stage(2, 3)
    yield e
    e.close()


@pytest.fixture(scope="module")
def scenes():
    """name -> (inputs, the oracle's inputs, the oracle's answer), computed once"""
    from oracle import oracle
    out = {}
    for name, kw in SCENES.items():
        inp = synthetic.make_inputs(hull_builder=hip_hulls(), **kw)
        ref_inp = synthetic.make_inputs(hull_builder=oracle.build_obstacle_hulls, **kw)
        assert inp.n_candidates == 135 and -(-inp.N // 3) == CHUNKS[name], (name, inp.n_candidates, inp.N)
        out[name] = (inp, ref_inp, oracle.plan_step(ref_inp))
    return out


def is_split(eng, waves, agents=1):
    info = eng.step_info()
    assert info["grid_kernel"] == 1 and info["lanes_per_candidate"] == 2 and info["wave_split"] == 1, info
    assert info["obstacle_kernel"] == 1 and info["obstacle_steps_per_item"] == 3 and info["obstacle_workgroup_waves"] == waves, info
    assert not info["fused_selection"] and not info["step_kernel"] and info["agents"] == agents, info


def bits(eng, n_agents=1):
    """every agent's costs (as bit patterns) and flag words"""
    out = []
    for a in range(n_agents):
        cost, flags = eng.costs(a)
        out.append((np.array(cost, dtype=np.float64).view(np.uint64).copy(), np.array(flags).copy()))
    return out


def run(eng, scenes, names, monkeypatch, by_index):
    """one step of the named scenes (a batch where there are several), held to the oracle; -> (results, bits)"""
    if by_index:
        monkeypatch.setenv("FX_OBST_CHUNK_INDEX", "1")
    else:
        monkeypatch.delenv("FX_OBST_CHUNK_INDEX", raising=False)
    eng.upload([scenes[n][0] for n in names] if len(names) > 1 else scenes[names[0]][0])
    eng.evaluate()
    res = eng.finish()
    is_split(eng, max(CHUNKS[n] for n in names), agents=len(names))
    for a, n in enumerate(names):
        inp, ref_inp, want = scenes[n]
        compare(eng, inp, want, res[a], ref_inp=ref_inp, agent=a)
    return [{k: r[k] for k in RESULT_KEYS} for r in res], bits(eng, len(names))


def mapped_equals_indexed(eng, scenes, names, monkeypatch):
    res_m, bits_m = run(eng, scenes, names, monkeypatch, by_index=False)
    res_i, bits_i = run(eng, scenes, names, monkeypatch, by_index=True)
    res_m2, bits_m2 = run(eng, scenes, names, monkeypatch, by_index=False)   # and back: the hook leaves nothing behind
    for a in range(len(names)):
        assert res_m[a] == res_i[a] == res_m2[a], (names[a], res_m[a], res_i[a])
        for got in (bits_i[a], bits_m2[a]):
            assert np.array_equal(bits_m[a][0], got[0]), f"{names[a]}: costs differ in their bits"
            assert np.array_equal(bits_m[a][1], got[1]), f"{names[a]}: flag words differ"
    return res_m


@pytest.mark.parametrize("name", ["main", "debug", "s8", "s32", "infeasible"])
def test_step_against_oracle_and_against_chunks_by_index(eng, scenes, monkeypatch, name):
    want = scenes[name][2]
    if name == "infeasible":
        assert int(want["costed"].sum()) == 0
    elif name == "debug":
        assert int(want["costed"].sum()) == 135 and want["result"]["n_collisions"] > 0
    else:
        assert int(want["costed"].sum()) > 0 and want["result"]["n_collisions"] > 0 and want["result"]["best_index"] >= 0
    res = mapped_equals_indexed(eng, scenes, [name], monkeypatch)[0]
    assert res["best_index"] == want["result"]["best_index"] and res["n_collisions"] == want["result"]["n_collisions"]


@pytest.mark.parametrize("pair", [("debug", "s8"), ("main", "s32"), ("s8", "second")])
def test_batch_of_two_agents_with_different_horizons(eng, scenes, monkeypatch, pair):
    """ten waves per workgroup with a three-chunk agent beside the ten-chunk one (the map applies to the ten-chunk agent only), eleven
    waves where an eleven-chunk agent rides along (no map for either)"""
    res = mapped_equals_indexed(eng, scenes, list(pair), monkeypatch)
    for a, n in enumerate(pair):
        want = scenes[n][2]["result"]
        assert res[a]["best_index"] == want["best_index"] and res[a]["n_collisions"] == want["n_collisions"], n
