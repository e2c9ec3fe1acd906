"""The context's own buffers sit behind owner types (csrc/fx_owner.h): device arrays that keep fx_device_bytes themselves, pinned
blocks, events, the stream.  This file holds the grow sites of an upload -- the planes, the road-boundary pair, the obstacle
kernel's scratch -- to what their hand-written versions did: one engine runs a small step, a large one and the small one again, and
owns afterwards exactly what a fresh engine of the same capacities owns after the large step alone; the third step changes nothing;
cost, flags and winner of every step equal, bit for bit, those of a fresh engine that ran only that step; an engine opened after
close() reports the same device_bytes at the same points.

Shapes: 3 x 3 x 5 = 45 candidates (below one tile of 64: ld = 64) and 5 x 5 x 5 = 125 (one full tile and a ragged one: ld = 128),
N = 10 steps (S = 11 samples), two obstacles, the bundle stored.  Three kinds: plain; with a road boundary (road_half_width = 2.6);
with the obstacle stage forced into its own kernel (set_obstacle_stage(2)).  In the plain kind only the planes grow between the
two steps, by 8 * FX_NUM_PLANES * S * (128 - 64) bytes (fx_policy.h: sizeof(double) * FX_NUM_PLANES * S * ld).

Nothing here creates a communicator, so the gather block of the survivor exchange is not observed."""
import dataclasses

import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi

pytestmark = pytest.mark.gpu

GRIDS = {"small": (3, 3, 5), "large": (5, 5, 5)}
LD = {"small": 64, "large": 128}
KINDS = ("plain", "road", "obstacle_stage")
S = 11
CAPACITY = 125


def _inputs(size, kind):
    from frenetix_motion_planner_amd import synthetic
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    grid = GRIDS[size]
    n_t = grid[0]
    inp = synthetic.make_inputs(hull_builder=build_obstacle_hulls, ref_kind="arc", v0=10.0, grid=(n_t, grid[1], grid[2] - 1), n_obstacles=2,
                                horizon=1.0, n_pred=10, write_bundle=True, write_costmap=True,
                                road_half_width=2.6 if kind == "road" else None,
                                cost_weights=dict(synthetic.DEFAULT_COST_WEIGHTS, prediction=0.2))
    # N = 10: end times on the last n_t steps of the horizon, lateral offsets a vehicle reaches within a second (d0 = 0.2 last)
    inp = dataclasses.replace(inp, t_samp=np.arange(10 - n_t + 1, 11) * inp.dt, d_samp=np.append(np.linspace(-0.3, 0.3, grid[2] - 1), 0.2))
    assert inp.N == S - 1 and inp.n_candidates == grid[0] * grid[1] * grid[2]
    return inp


def _engine(kind):
    from frenetix_motion_planner_amd.engine import FrenetEngine
    e = FrenetEngine(max_candidates=CAPACITY, device=0)
    if kind == "obstacle_stage":
        e.set_obstacle_stage(2)
    return e


def _step(e, inp):
    res = e.plan_step(inp)
    cost, flags = e.costs()
    return res["best_index"], res["best_cost"], res["n_feasible"], res["n_collisions"], cost.view(np.uint64).copy(), flags.copy()


def _same(got, want):
    return all(np.array_equal(a, b) if isinstance(b, np.ndarray) else a == b for a, b in zip(got, want)) and len(got) == len(want)


@pytest.mark.parametrize("kind", KINDS)
def test_small_large_small_equals_fresh_engines(kind):
    inputs = {size: _inputs(size, kind) for size in GRIDS}
    alone = {}   # size -> (results, device_bytes) of a fresh engine that ran only that step; computed once, left unchanged
    for size in GRIDS:
        with _engine(kind) as e:
            bytes0 = e.device_bytes
            alone[size] = (_step(e, inputs[size]), e.device_bytes)
            assert e.step_info()["obstacle_kernel"] == (kind == "obstacle_stage")
    planes = {size: 8 * _abi.FX_NUM_PLANES * S * LD[size] for size in GRIDS}
    print(kind, "device_bytes: created", bytes0, {size: alone[size][1] for size in GRIDS}, "planes", planes)
    assert alone["large"][1] > alone["small"][1] > bytes0
    assert np.isfinite(alone["large"][0][1]) and alone["large"][0][2] > 0   # (not a comparison of refusals)

    eng = _engine(kind)
    try:
        assert eng.device_bytes == bytes0
        seen = []
        for size in ("small", "large", "small"):
            assert _same(_step(eng, inputs[size]), alone[size][0]), size
            seen.append(eng.device_bytes)
        print(kind, "device_bytes after small, large, small:", seen)
        assert seen[0] == alone["small"][1]
        assert seen[1] == alone["large"][1]   # a block that grows gives back what it held
        assert seen[2] == seen[1]             # grow-only
        if kind == "plain":
            assert seen[0] - bytes0 == planes["small"]
            assert seen[1] - seen[0] == planes["large"] - planes["small"] == 8 * _abi.FX_NUM_PLANES * S * (128 - 64)
        else:   # the boundary pair / the obstacle scratch came on top of the planes
            assert seen[0] - bytes0 > planes["small"] and seen[1] - bytes0 > planes["large"]
    finally:
        eng.close()
    eng.close()   # (a closed engine closes again without a call into the library)

    with _engine(kind) as again:   # close and reopen: the same account at the same points
        assert again.device_bytes == bytes0
        assert _same(_step(again, inputs["small"]), alone["small"][0])
        assert again.device_bytes == seen[0]


def test_failed_create_leaves_no_context():
    """a create that fails stores NULL: the engine has no context, and closing it is a no-op"""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    e = FrenetEngine.__new__(FrenetEngine)
    with pytest.raises(ValueError, match="bad capacity arguments"):
        e.__init__(max_candidates=0)
    assert not e._ctx.value
    e.close()
    e.close()
