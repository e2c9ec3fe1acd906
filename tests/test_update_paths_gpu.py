"""The in-place step update (fx_update_state, and fx_update_step / fx_plan_and_package / fx_plan_batch_begin, which call it) held
to a fresh upload on every kernel path.

Two contexts throughout: `eng` uploads the base inputs once, evaluates, then applies updates; `eng2` does a fresh plan_step of the
inputs the update is meant to produce (the "twin").  Every comparison has two legs:

  a. bit equality with the fresh upload: flag words, costs, raw cost terms, the bundle where one is written, boundary steps where a
     boundary exists, every key of the result;
  b. the fresh upload against oracle.plan_step of the same inputs through tests.test_hip_parity.compare (its doors, no new
     tolerance) -- once per distinct input, not per decomposition.

Fields are changed ONE AT A TIME on a running state (the twin of a partial update is the previous twin with that one array
replaced: new positions travel with the old hulls), then everything at once through FrenetEngine._state_update_of.  The field list
runs under the automatic decomposition, every forced decomposition of tests/test_hip_reference_vectors.VARIANTS, 16 and 32 lanes
per candidate, select-only mode, the generic kernel with windowed costs, 65 obstacles (multi-word masks) and a road boundary.  A
variant the library declines, or that falls back, is checked as it ran and then SKIPPED with the reason; the last test asserts that
every variant ran as asked for at least one case, that every field changed the oracle's answer somewhere, and prints the tally.

Leaving the projection domain: with more than one lane per candidate and the obstacle stage inside the walk, a lane part that
starts behind the step at which the candidate left the reference path re-sums its prediction cost from the device's RAW
predictions (fx_eval_kernel.h, finish_candidate) -- the only device reader of those arrays.  A short reference, debug flags so that
such candidates are costed, predictions moved by metres through an update: the preconditions are asserted on the oracle's output
before anything runs on the GPU.  (fx_update_state used to stage those arrays for a generic-kernel plan only: the six grid-kernel
cases failed, 728 - 1 036 of the 1 274 costs differing in their last digits, until it staged them for every plan with that reader.)

Tried on deliberately broken builds of the library, one at a time: the staged range cut back to the packed tables fails the eight
leaving-domain cases; the re-pack skipped when only the origin moved fails the x0_lon case under 17 (base, variant) pairs (one to
four lanes per candidate, the obstacle kernel, the one-launch step); the obs_cov_inv copy dropped fails 52 of the 71 tests.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from frenetix_motion_planner_amd import _abi, synthetic
from tests.test_hip_parity import CASES as PARITY_CASES
from tests.test_hip_parity import compare
from tests.test_hip_reference_vectors import VARIANTS, _automatic, _tuning

pytestmark = pytest.mark.gpu

# ---- shapes: the smallest that still reach each path (grids (3, 5, 7) and (7, 13, 13), 31 and 21 samples, K = 0, 1, 6, 65) ----
BASES = {
    "k6_s31": dict(ref_kind="arc", v0=10.0, grid=(7, 13, 13), n_obstacles=6, lead_gap=20.0),
    # standstill at speed mode: step 0 does not move, so its heading is x0_orientation (reactive_planner.py:525)
    "k1_s21_standstill": dict(ref_kind="arc", v0=0.0, low_vel_threshold=-1.0, v_des=4.0, grid=(3, 5, 7), horizon=2.0, n_pred=20,
                              n_obstacles=1, draw_traj_set=True, kinematic_debug=True),
    "k0_s31": dict(ref_kind="scurve", v0=8.0, grid=(3, 5, 7)),
    "select_only": dict(ref_kind="arc", v0=10.0, grid=(7, 13, 13), n_obstacles=6, lead_gap=20.0, write_bundle=False, write_costmap=False),
    "allcosts": PARITY_CASES["allcosts"],                       # windowed costs: generic kernel, one lane per candidate
    "k65": dict(ref_kind="arc", kappa=0.008, v0=9.0, grid=(3, 5, 7), n_obstacles=65, obstacle_min_gap=14.0, seed=11),
    "boundary": dict(ref_kind="arc", v0=10.0, grid=(3, 5, 7), n_obstacles=1, road_half_width=3.0),
}
LANES = {"lanes_16": (_tuning(16, 0, 0), lambda i: i["lanes_per_candidate"] == 16, False),
         "lanes_32": (_tuning(32, 0, 0), lambda i: i["lanes_per_candidate"] == 32, False)}
ALL_VARIANTS = {"automatic": (lambda e: None, lambda i: True, False), **VARIANTS, **LANES}
PATHS = [(b, v) for b in ("k6_s31", "k1_s21_standstill") for v in ALL_VARIANTS] + \
        [("k0_s31", v) for v in ("automatic", "lanes_32", "generic_kernel", "wave_split_4")] + \
        [("select_only", "automatic"), ("select_only", "lanes_16"), ("allcosts", "automatic"), ("k65", "automatic"),
         ("boundary", "automatic"), ("boundary", "lanes_4")]
SPECIAL_INFO = {"allcosts": lambda i: i["grid_kernel"] == 0 and i["lanes_per_candidate"] == 1,
                "k65": lambda i: i["grid_kernel"] == 0 and i["lanes_per_candidate"] > 1}

RAN = {}         # variant -> field cases that ran as asked
SKIPPED = {}     # variant -> {reason}
CHANGED = {}     # field -> bases on which the oracle's answer moved with it
LEAVING = {}     # the leaving-domain preconditions, for the tally
EXECUTED = [0]   # path tests that ran in this process (the tally judges whole runs only)
ORACLE_DONE = set()
STATE_FIELDS = ("x0_lon", "x0_lat", "x0_orientation", "v_des", "low_vel_mode", "t_samp", "v_samp", "d_samp")
OBS_FIELDS = ("pos", "cov_inv", "npred", "hull", "nhull")


def _hip_hulls():
    from frenetix_motion_planner_amd.engine import build_obstacle_hulls
    return build_obstacle_hulls


def _ora_hulls():
    from oracle import oracle
    return oracle.build_obstacle_hulls


def _engine(**kw):
    from frenetix_motion_planner_amd.engine import FrenetEngine
    return FrenetEngine(**dict(dict(max_candidates=8192, max_steps=30, max_ref_knots=512, max_obstacles=72, max_pred_steps=32,
                                    max_agents=4), **kw))


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng2():
    e = _engine()
    yield e
    e.close()


# ---------------------------------------------------------------------------------------------- inputs, twins, updates
def _with(o, **kw):
    """the packed predictions `o` with some arrays replaced (a new dict: the cached pointers of the old one must not travel)"""
    d = {k: v for k, v in o.items() if k != "_ptrs"}
    for k, v in kw.items():
        d[k] = np.ascontiguousarray(v, dtype=o[k].dtype)
    return d


def _alt(inp, builder, dx=0.0, dy=0.0, cov_scale=1.0, cov_off=0.0, cut=None):
    """the base predictions moved by (dx, dy), covariances scaled and skewed, obstacle cut[0] shortened to cut[1] predictions -- packed
    with the (K, P) of the base"""
    from frenetix_motion_planner_amd.problem import pack_predictions
    preds = {}
    for n, (key, p) in enumerate(inp.predictions.items()):
        q = dict(p, pos_list=np.ascontiguousarray(np.asarray(p["pos_list"]) + np.array([dx, dy])),
                 cov_list=np.ascontiguousarray(np.asarray(p["cov_list"]) * cov_scale + cov_off * np.array([[0.0, 1.0], [1.0, 0.0]])))
        if cut is not None and n == cut[0]:
            q = {k: (np.ascontiguousarray(np.asarray(v)[:cut[1]]) if k.endswith("_list") else v) for k, v in q.items()}
        preds[key] = q
    o = pack_predictions(preds, inp.n_samples, builder)
    assert (o["K"], o["P"]) == (inp.obstacles["K"], inp.obstacles["P"])
    return o


def _set_npred(value):
    def mod(inp, builder):
        npred = inp.obstacles["npred"].copy()
        npred[-1] = value(inp.obstacles)
        inp.obstacles = _with(inp.obstacles, npred=npred)
    return mod


def _mod(**kw):
    def mod(inp, builder):
        for k, f in kw.items():
            setattr(inp, k, f(inp))
    return mod


def _obs(fields, **alt_kw):
    def mod(inp, builder):
        kw = dict(alt_kw)
        if "cut" in kw and inp.obstacles["K"] < 2:
            kw.pop("cut")   # (one obstacle: cutting it would change P)
        alt = _alt(inp, builder, **kw)
        inp.obstacles = _with(inp.obstacles, **{f: alt[f] for f in fields})
    return mod


def _everything(inp, builder):
    inp.x0_lon = inp.x0_lon + np.array([1.7, -0.4, 0.2])
    inp.x0_lat = inp.x0_lat + np.array([-0.11, 0.03, 0.02])
    inp.x0_orientation = float(inp.x0_orientation) - 0.03
    inp.v_des = float(inp.v_des) - 2.25
    inp.low_vel_mode = False
    inp.t_samp, inp.v_samp, inp.d_samp = inp.t_samp + inp.dt, inp.v_samp - 0.2, inp.d_samp * 1.05 - 0.02
    if inp.obstacles["K"]:
        inp.obstacles = _with(_alt(inp, builder, dx=-2.0, dy=1.1, cov_scale=0.8, cov_off=-0.01))


# (name, what the update carries, how the running state changes); obstacle fields are skipped on a base without obstacles
FIELD_CASES = [
    ("x0_lon", ("x0_lon",), _mod(x0_lon=lambda i: i.x0_lon + np.array([0.8, 0.0, 0.05]))),   # obstacles kept: re-pack from the kept raw arrays
    ("x0_lat", ("x0_lat",), _mod(x0_lat=lambda i: i.x0_lat + np.array([0.07, 0.02, -0.01]))),
    ("x0_orientation", ("x0_orientation",), _mod(x0_orientation=lambda i: float(i.x0_orientation) + 0.05)),
    ("v_des", ("v_des",), _mod(v_des=lambda i: float(i.v_des) + 1.5)),
    ("low_vel_mode_on", ("low_vel_mode",), _mod(low_vel_mode=lambda i: True)),
    ("low_vel_mode_off", ("low_vel_mode",), _mod(low_vel_mode=lambda i: False)),
    ("t_samp", ("t_samp",), _mod(t_samp=lambda i: i.t_samp - i.dt)),
    ("v_samp", ("v_samp",), _mod(v_samp=lambda i: i.v_samp + 0.35)),
    ("d_samp", ("d_samp",), _mod(d_samp=lambda i: i.d_samp * 0.9 + 0.05)),
    ("obs_pos", ("pos",), _obs(("pos",), dx=1.5, dy=0.4)),
    ("obs_cov_inv", ("cov_inv",), _obs(("cov_inv",), cov_scale=1.7, cov_off=0.02)),
    ("obs_hull", ("hull", "nhull"), _obs(("hull", "nhull"), dx=-2.5, dy=0.6, cut=(1, 1))),   # (obstacle 1: no hull left)
    ("obs_npred_2", ("npred",), _set_npred(lambda o: 2)),
    ("obs_npred_1", ("npred",), _set_npred(lambda o: 1)),
    ("obs_npred_long", ("npred",), _set_npred(lambda o: o["P"] + 1)),
    ("everything", None, _everything),
]


def _build(base, builder):
    return synthetic.make_inputs(hull_builder=builder, **BASES[base])


def _snapshot(inp):
    s = copy.copy(inp)          # (the mods replace arrays, they never write into one)
    s.__dict__.pop("_skey", None)
    return s


@functools.lru_cache(maxsize=None)
def field_twins(base):
    """[(field case, what the update carries, twin for the device, twin for the oracle)] of a base, the state running on"""
    hip, ora = _build(base, _hip_hulls()), _build(base, _ora_hulls())
    out = [("base", (), _snapshot(hip), _snapshot(ora))]
    for name, fields, mod in FIELD_CASES:
        if name.startswith("obs_") and not hip.obstacles["K"]:
            continue
        mod(hip, _hip_hulls())
        mod(ora, _ora_hulls())
        out.append((name, fields, _snapshot(hip), _snapshot(ora)))
    return out


@functools.lru_cache(maxsize=None)
def oracle_of(base, n):
    from oracle import oracle
    return oracle.plan_step(field_twins(base)[n][3])


def make_update(twin, fields):
    """FxStateUpdate carrying exactly `fields` of `twin` (None: everything, the way the engine itself builds it)"""
    from frenetix_motion_planner_amd.engine import FrenetEngine
    if fields is None:
        return FrenetEngine._state_update_of(twin)
    u = FrenetEngine.make_state_update(**{f: getattr(twin, f) for f in fields if f in STATE_FIELDS})
    o = twin.obstacles
    for f in fields:
        if f in OBS_FIELDS:
            setattr(u, "obs_" + f, o[f].ctypes.data)
            u.K, u.P = int(o["K"]), int(o["P"])
    u._twin = twin   # (the arrays live as long as the update does)
    return u


def read_all(e, inp, agent=0):
    """everything a step leaves on the device for one agent"""
    cost, flags = e.costs(agent)
    d = dict(cost=cost, flags=flags)
    if inp.write_costmap and len(inp.cost_names):
        d["costmap"] = e.costmap(agent)
    if inp.write_bundle:
        d["bundle"] = e.bundle(agent)
    if inp.mode & _abi.FX_MODE_ROAD_BOUNDARY:
        d["boundary_steps"] = e.boundary_steps(agent)
    return d


def assert_same(got, want, res_got, res_want, what):
    assert set(got) == set(want), what
    for k in want:
        assert np.array_equal(got[k], want[k]), f"{what}: {k} differs from the fresh upload ({int((got[k] != want[k]).sum())} entries)"
    assert set(res_got) == set(res_want)
    for k in res_want:
        assert res_got[k] == res_want[k], f"{what}: result['{k}'] {res_got[k]} != {res_want[k]} of the fresh upload"


def _force(variant, *engines):
    """the variant's forced decomposition on every engine (it takes effect at the next upload)"""
    for e in engines:
        ALL_VARIANTS[variant][0](e)


def _note_skip(variant, reason):
    SKIPPED.setdefault(variant, set()).add(reason)


def _fallback_reason(info):
    return (f"the library fell back: lanes {info['lanes_per_candidate']}, grid kernel {info['grid_kernel']}, wave split {info['wave_split']}, "
            f"obstacle kernel {info['obstacle_kernel']}, fused selection {info['fused_selection']}, one launch {info['step_kernel']}")


# ---------------------------------------------------------------------------------------------- the fields, leg b
@pytest.mark.parametrize("base", sorted(BASES))
def test_fresh_uploads_of_the_twins_vs_oracle(eng2, base):
    """leg b: the fresh upload of every twin against the oracle (automatic decomposition), and the precondition that the field
    moved the oracle's answer at all"""
    twins = field_twins(base)
    for n, (name, fields, hip, ora) in enumerate(twins):
        out = oracle_of(base, n)
        res = eng2.plan_step(hip)
        compare(eng2, hip, out, res, ref_inp=ora)
        if n:
            prev = oracle_of(base, n - 1)
            moved = not (np.array_equal(prev["flags"], out["flags"]) and np.array_equal(prev["cost"], out["cost"])
                         and np.array_equal(prev["planes"], out["planes"]))
            if moved:
                CHANGED.setdefault(name, set()).add(base)
    ORACLE_DONE.add(base)


# ---------------------------------------------------------------------------------------------- the fields, leg a
@pytest.mark.parametrize("base,variant", PATHS)
def test_update_of_each_field_equals_fresh_upload(eng, eng2, base, variant):
    _, ran_as_asked, needs_predictions = ALL_VARIANTS[variant]
    EXECUTED[0] += 1
    twins = field_twins(base)
    assert twins[0][2].obstacles["K"] or not needs_predictions
    try:
        _force(variant, eng, eng2)
        try:
            eng.upload(twins[0][2])        # ONE upload; everything behind it is an update
            eng.evaluate()
            r0 = eng.finish()[0]
        except ValueError as e:
            if "not applicable" in str(e):
                _note_skip(variant, f"declined on {base}: {e}")
                pytest.skip(f"declined by the library: {e}")
            raise
        info0 = eng.step_info()
        rb = eng2.plan_step(twins[0][2])
        assert_same(read_all(eng, twins[0][2]), read_all(eng2, twins[0][2]), r0, rb, f"{base}/{variant}/base")
        for name, fields, hip, _ in twins[1:]:
            eng.update_state(make_update(hip, fields))
            eng.evaluate()
            ra = eng.finish()[0]
            info = eng.step_info()
            rb = eng2.plan_step(hip)
            info2 = eng2.step_info()
            keys = ("grid_kernel", "lanes_per_candidate", "wave_split", "obstacle_kernel", "fused_selection", "step_kernel", "block")
            assert all(info[k] == info2[k] == info0[k] for k in keys), (name, info, info2)
            assert_same(read_all(eng, hip), read_all(eng2, hip), ra, rb, f"{base}/{variant}/{name}")
        if base in SPECIAL_INFO:
            assert SPECIAL_INFO[base](info0), info0
        if not ran_as_asked(info0):
            _note_skip(variant, f"{base}: {_fallback_reason(info0)}")
            pytest.skip(_fallback_reason(info0) + " (the step as it ran passes)")
        RAN[variant] = RAN.get(variant, 0) + len(twins) - 1
    finally:
        _automatic(eng)
        _automatic(eng2)


# ---------------------------------------------------------------------------------------------- leaving the projection domain
LEAVE_KW = dict(ref_kind="arc", n_knots=70, s_knot=40, v0=12.0, grid=(7, 13, 13), n_obstacles=6, draw_traj_set=True, kinematic_debug=True)
# (kernel variant, lanes per candidate, part mapping: 1 lane split, 2 wave split)
LEAVE_PATHS = [(2, 2, 1), (2, 4, 1), (2, 16, 1), (2, 32, 1), (2, 2, 2), (2, 4, 2), (1, 4, 1), (1, 32, 1)]


def _moved_predictions(inp):
    """every prediction moved by metres, another cov_inv, one prediction shortened: the old hulls stay"""
    o = inp.obstacles
    npred = o["npred"].copy()
    npred[2] = 12
    return _with(o, pos=o["pos"] + np.array([3.0, -2.0]), cov_inv=o["cov_inv"] * 0.6, npred=npred)


def _tail_prediction_cost(o, S):
    """[S] the prediction cost of steps i .. S - 1 at (x, y) = (0, 0), what a candidate that left the domain before step i
    is charged for them (collision_probability.py:279-297 behind the reference's break, :547)"""
    term = np.zeros(S + 1)
    for i in range(1, S):
        for k in range(o["K"]):
            if i < o["npred"][k] and i - 1 < o["P"]:
                mu, iv = -o["pos"][k, i - 1], o["cov_inv"].reshape(o["K"], o["P"], 2, 2)[k, i - 1]
                m = float(mu @ iv @ mu)
                term[i] += 1.0 / (m * m)
    return np.cumsum(term[::-1])[::-1][:S]


@functools.lru_cache(maxsize=None)
def leaving_case():
    from oracle import oracle
    base = {b: synthetic.make_inputs(hull_builder=h, **LEAVE_KW) for b, h in (("hip", _hip_hulls()), ("ora", _ora_hulls()))}
    twin = {}
    for b, inp in base.items():
        twin[b] = _snapshot(inp)
        twin[b].obstacles = _moved_predictions(inp)
    out_old, out = oracle.plan_step(base["ora"]), oracle.plan_step(twin["ora"])
    return base, twin, out_old, out


def test_leaving_the_domain_preconditions_hold_on_the_oracle():
    _assert_leaving_preconditions()


def _assert_leaving_preconditions():
    """Computed on the CPU before anything of this case runs on the GPU: more than 20 costed candidates leave the projection domain
    at a step in [2, S - 2], and what they are charged for the steps behind it differs between the old and the new predictions"""
    base, twin, out_old, out = leaving_case()
    inp = twin["ora"]
    S = inp.n_samples
    left = out["costed"] & (((out["reasons"] >> 9) & 1) != 0)
    s = out["planes"][:, _abi.PLANE_INDEX["s"], :]
    outside = (s > inp.coordinate_system.ref_pos[-1]) | (s < inp.coordinate_system.ref_pos[0])
    fail = np.where(outside.any(axis=1), outside.argmax(axis=1), S)
    mid = left & (fail >= 2) & (fail <= S - 2)
    assert mid.sum() > 20, int(mid.sum())
    xy = out["planes"][mid][:, :2, :]
    assert all((xy[n, :, f:] == 0.0).all() and (xy[n, :, :f] != 0.0).any() for n, f in enumerate(fail[mid]))   # the reference's loop broke there
    # a part of G lanes starts behind the fail step for these: G = 2 splits the 31 samples at 16
    early = mid & (fail < S // 2)
    assert early.sum() > 20, int(early.sum())
    tail_old, tail_new = _tail_prediction_cost(base["ora"].obstacles, S), _tail_prediction_cost(inp.obstacles, S)
    f1 = fail[mid & (fail <= S - 3)] + 1    # (step S - 1 pairs with prediction S - 2 = P: nothing is charged for it)
    rel = np.abs(tail_new[f1] - tail_old[f1]) / np.maximum(tail_old[f1], tail_new[f1])
    assert len(f1) > 20 and (rel > 1e-3).all()
    j = inp.cost_names.index("prediction")
    assert (out["costmap"][mid, j] != out_old["costmap"][mid, j]).all()
    LEAVING.update(costed=int(out["costed"].sum()), leave_mid_horizon=int(mid.sum()), leave_before_half=int(early.sum()),
                   collisions=int(out["collision"].sum()),
                   min_tail_change=float(rel.min()))


def test_leaving_the_domain_fresh_upload_vs_oracle(eng2):
    base, twin, out_old, out = leaving_case()
    res = eng2.plan_step(twin["hip"])
    compare(eng2, twin["hip"], out, res, ref_inp=twin["ora"])


@pytest.mark.parametrize("variant,lanes,mapping", LEAVE_PATHS)
def test_leaving_the_domain_after_an_update_equals_fresh_upload(eng, eng2, variant, lanes, mapping):
    """obstacle stage fused, more than one lane per candidate, predictions changed by an update: the parts behind the fail step
    must be charged with the NEW predictions"""
    EXECUTED[0] += 1
    _assert_leaving_preconditions()
    base, twin, _, _ = leaving_case()
    name = f"leaving:{'grid' if variant == 2 else 'generic'}_lanes_{lanes}_{'wave' if mapping == 2 else 'lane'}_split"
    try:
        for e in (eng, eng2):
            e.set_tuning(lanes, 0, variant, 0, mapping)
            e.set_obstacle_stage(1)
        try:
            eng.upload(base["hip"])
            eng.evaluate()
            eng.finish()
        except ValueError as e:
            if "not applicable" in str(e):
                _note_skip(name, f"declined: {e}")
                pytest.skip(f"declined by the library: {e}")
            raise
        eng.update_state(make_update(twin["hip"], ("pos", "cov_inv", "npred")))
        eng.evaluate()
        ra = eng.finish()[0]
        info = eng.step_info()
        rb = eng2.plan_step(twin["hip"])
        assert_same(read_all(eng, twin["hip"]), read_all(eng2, twin["hip"]), ra, rb, name)
        asked = (info["grid_kernel"] == (variant == 2) and info["lanes_per_candidate"] == lanes and info["obstacle_kernel"] == 0
                 and info["wave_split"] == (mapping == 2))
        if not asked:
            _note_skip(name, _fallback_reason(info))
            pytest.skip(_fallback_reason(info) + " (the step as it ran passes)")
        RAN[name] = RAN.get(name, 0) + 1
    finally:
        _automatic(eng)
        _automatic(eng2)


# ---------------------------------------------------------------------------------------------- batches
BATCH_KW = [dict(ref_kind="arc", v0=9.0, grid=(3, 5, 7), seed=1),                                        # K = 0, 31 samples
            dict(ref_kind="arc", v0=7.0, grid=(3, 5, 7), n_obstacles=1, horizon=2.0, n_pred=20, seed=2),   # K = 1, 21 samples
            dict(ref_kind="scurve", v0=11.0, grid=(3, 7, 13), n_obstacles=6, lead_gap=18.0, seed=3),      # K = 6, 31 samples
            dict(ref_kind="arc", v0=8.0, grid=(3, 5, 7), n_obstacles=6, horizon=2.0, n_pred=20, as_matrix=True, seed=4)]   # K = 6, 21 samples, sampling matrix


def _batch():
    return [synthetic.make_inputs(hull_builder=_hip_hulls(), **kw) for kw in BATCH_KW]


def _agent_update(inp, step, sampling=True):
    """the twin of agent `inp` after update number `step`, and what the update carries"""
    t = _snapshot(inp)
    t.x0_lon = inp.x0_lon + np.array([0.6 * step, 0.1, 0.0])
    t.x0_lat = inp.x0_lat + np.array([0.02 * step, 0.0, 0.01])
    t.v_des = float(inp.v_des) + 0.75 * step
    fields = ["x0_lon", "x0_lat", "v_des"]
    if sampling and inp.sampling_matrix is None:
        t.v_samp, t.d_samp = inp.v_samp + 0.1 * step, inp.d_samp * (1.0 - 0.02 * step)
        fields += ["v_samp", "d_samp"]
    if inp.obstacles["K"]:
        t.obstacles = _with(_alt(inp, _hip_hulls(), dx=0.9 * step, dy=-0.3 * step, cov_scale=1.0 + 0.1 * step))
        fields += list(OBS_FIELDS)
    return t, tuple(fields)


def _compare_batch(eng, eng2, twins, ra, what, packages=False):
    eng2.upload(twins)
    eng2.evaluate()
    rb = eng2.finish()
    for a, t in enumerate(twins):
        assert_same(read_all(eng, t, a), read_all(eng2, t, a), ra[a], rb[a], f"{what}, agent {a}")
        if packages:
            pa, pb = eng.package(a, 0.01 * a), eng2.package(a, 0.01 * a)
            assert (pa is None) == (pb is None)
            if pa is not None:
                assert pa.index == pb.index and pa.cost == pb.cost and pa.flags == pb.flags and pa.traj_len == pb.traj_len
                assert np.array_equal(pa.block, pb.block) and np.array_equal(pa.raw_costs, pb.raw_costs)
                assert np.array_equal(pa.lon, pb.lon) and np.array_equal(pa.lat, pb.lat) and pa.tau_lat == pb.tau_lat


def _start_batch(eng, agents):
    eng.upload(agents)
    eng.evaluate()
    eng.finish()


def test_batch_update_of_a_subset_of_the_agents(eng, eng2):
    """agents {1, 3} through update_state(agent=); the agent with a sampling matrix takes a state-and-predictions update and refuses
    a sampling update, which leaves it as it was"""
    from frenetix_motion_planner_amd._lib import FxError
    agents = _batch()
    assert [a.obstacles["K"] for a in agents] == [0, 1, 6, 6] and [a.n_samples for a in agents] == [31, 21, 31, 21]
    _start_batch(eng, agents)
    twins = list(agents)
    for a in (1, 3):
        twins[a], fields = _agent_update(agents[a], 1)
        eng.update_state(make_update(twins[a], fields), agent=a)
    with pytest.raises((ValueError, FxError)):
        eng.update_state(eng.make_state_update(v_des=99.0, v_samp=agents[1].v_samp), agent=3)   # refused as a whole: v_des stays
    eng.evaluate()
    _compare_batch(eng, eng2, twins, eng.finish(), "subset {1, 3}")


def test_batch_begin_with_null_entries(eng, eng2):
    """the same subset through fx_plan_batch_begin, NULL for the agents that keep their state; the packages compared as well"""
    from frenetix_motion_planner_amd._lib import check, lib
    agents = _batch()
    _start_batch(eng, agents)
    twins, ups = list(agents), [None] * 4
    for a in (1, 3):
        twins[a], fields = _agent_update(agents[a], 2)
        ups[a] = make_update(twins[a], fields)
    ptrs = (C.c_void_p * 4)(*[C.addressof(u) if u is not None else None for u in ups])
    check(lib().fx_plan_batch_begin(eng._ctx, 4, C.addressof(ptrs)))
    ra = eng.finish()
    eng2.set_package(True)
    try:
        _compare_batch(eng, eng2, twins, ra, "fx_plan_batch_begin with NULL entries", packages=True)
    finally:
        eng2.set_package(False)


def test_two_updates_of_one_agent_before_one_evaluation(eng, eng2):
    """the later values win, the fields only the earlier update carried stay"""
    agents = _batch()
    _start_batch(eng, agents)
    first, _ = _agent_update(agents[2], 1)
    second, _ = _agent_update(agents[2], 3)
    eng.update_state(make_update(first, ("x0_lon", "v_des", "v_samp", "pos", "hull", "nhull")), agent=2)
    eng.update_state(make_update(second, ("v_des", "d_samp", "cov_inv")), agent=2)
    twin = _snapshot(agents[2])
    twin.x0_lon, twin.v_samp, twin.v_des, twin.d_samp = first.x0_lon, first.v_samp, second.v_des, second.d_samp
    twin.obstacles = _with(agents[2].obstacles, pos=first.obstacles["pos"], hull=first.obstacles["hull"], nhull=first.obstacles["nhull"],
                           cov_inv=second.obstacles["cov_inv"])
    eng.evaluate()
    twins = list(agents)
    twins[2] = twin
    _compare_batch(eng, eng2, twins, eng.finish(), "two updates of agent 2")


def test_update_evaluate_update_evaluate_without_a_finish_between(eng, eng2):
    """the second update finds the first evaluation in flight and drains it before the staging block is rewritten"""
    agents = _batch()
    _start_batch(eng, agents)
    twins = list(agents)
    for step in (1, 2):
        for a in range(4):
            twins[a], fields = _agent_update(agents[a], step)
            eng.update_state(make_update(twins[a], fields), agent=a)
        eng.evaluate()
    _compare_batch(eng, eng2, twins, eng.finish(), "update, evaluate, update, evaluate, finish")


# ---------------------------------------------------------------------------------------------- closed-loop sequences
SEQ_KW = dict(ref_kind="arc", v0=10.0, grid=(7, 13, 13), n_obstacles=6, lead_gap=20.0)
SEQ_STEPS = 20


def _one_launch(e):
    VARIANTS["one_launch"][0](e)


SEQ_MODES = {   # how the decomposition is forced, how the updated step is taken
    "automatic": (lambda e: None, "update_state"),
    "obstacle_kernel": (lambda e: e.set_obstacle_stage(2), "update_state"),
    "one_launch": (_one_launch, "update_state"),
    "fx_update_step": (lambda e: None, "update_step"),
    "fx_plan_and_package": (lambda e: None, "plan_and_package"),
}


@functools.lru_cache(maxsize=None)
def sequence(builder_name):
    """the inputs of 20 closed-loop steps: the ego advances along the reference (1 m per step, two knots), the predictions move with
    it, the sampled velocities follow the ego's, LOW_VEL_MODE is switched on from step 8 on"""
    from frenetix_motion_planner_amd.problem import pack_predictions
    builder = _hip_hulls() if builder_name == "hip" else _ora_hulls()
    base = synthetic.make_inputs(hull_builder=builder, **SEQ_KW)
    cs, s0 = base.coordinate_system, float(base.x0_lon[0])
    steps = [base]
    for j in range(1, SEQ_STEPS + 1):
        t = _snapshot(base)
        t.x0_lon = base.x0_lon + np.array([1.0 * j, -0.05 * j, 0.02 * (j % 3)])
        t.x0_lat = base.x0_lat + np.array([0.01 * j, 0.002 * (j % 5), 0.0])
        t.x0_orientation = float(cs.ref_theta[cs.segment_of(float(t.x0_lon[0]))])
        t.v_des = float(base.v_des) - 0.1 * j
        t.v_samp = base.v_samp - 0.05 * j
        t.low_vel_mode = j >= 8
        shift = cs.convert_to_cartesian_coords(s0 + 1.0 * j, 0.0) - cs.convert_to_cartesian_coords(s0, 0.0)
        preds = {k: dict(p, pos_list=np.asarray(p["pos_list"]) + shift[None, :]) for k, p in base.predictions.items()}
        t.obstacles = pack_predictions(preds, base.n_samples, builder)
        steps.append(t)
    return steps


def _plan_and_package(e, update, yaw_rate0, inp):
    """fx_plan_and_package itself: (result dict, FxPackage, block)"""
    from frenetix_motion_planner_amd._lib import check, lib
    res, pkg = (_abi.FxResult * 1)(), _abi.FxPackage()
    block = np.empty((_abi.FX_PKG_ROWS, inp.n_samples))
    check(lib().fx_plan_and_package(e._ctx, C.byref(update) if update is not None else None, float(yaw_rate0), res, C.byref(pkg), block.ctypes.data))
    return res[0].as_dict(), pkg, block


@pytest.mark.parametrize("mode", sorted(SEQ_MODES))
def test_closed_loop_sequence_equals_fresh_uploads(eng, eng2, mode):
    from oracle import oracle
    force, how = SEQ_MODES[mode]
    EXECUTED[0] += 1
    steps = sequence("hip")
    lives = set()
    try:
        for e in (eng, eng2):
            force(e)
        eng.upload(steps[0])
        eng.evaluate()
        eng.finish()
        info0 = eng.step_info()
        for j in range(1, SEQ_STEPS + 1):
            t = steps[j]
            up = eng._state_update_of(t)
            if how == "update_state":
                eng.update_state(up)
                eng.evaluate()
                ra = eng.finish()[0]
            elif how == "update_step":
                ra = eng.update_step_raw(up)[0].as_dict()
            else:
                ra, pkg_a, block_a = _plan_and_package(eng, up, 0.02 * j, t)
            info = eng.step_info()
            assert all(info[k] == info0[k] for k in ("grid_kernel", "lanes_per_candidate", "obstacle_kernel", "step_kernel")), (j, info)
            if how == "plan_and_package":
                eng2.upload(t)
                rb, pkg_b, block_b = _plan_and_package(eng2, None, 0.02 * j, t)
                assert pkg_a.found == pkg_b.found == 1, j
                for name, _ in _abi.FxPackage._fields_:
                    va, vb = getattr(pkg_a, name), getattr(pkg_b, name)
                    assert (list(va) == list(vb)) if hasattr(va, "__len__") else (va == vb), (j, name)
                assert np.array_equal(block_a, block_b), j
            else:
                rb = eng2.plan_step(t)
            assert_same(read_all(eng, t), read_all(eng2, t), ra, rb, f"sequence {mode}, step {j}")
            lives.add(ra["n_feasible"])
            if mode == "automatic" and j in (1, 10, 20):
                ref_inp = sequence("ora")[j]
                compare(eng2, t, oracle.plan_step(ref_inp), rb, ref_inp=ref_inp)
        assert len(lives) > 3     # the live count the one-launch step is sized by moves along the sequence
        asked = {"obstacle_kernel": info0["obstacle_kernel"] == 1, "one_launch": info0["step_kernel"] == 1}.get(mode, True)
        if not asked:
            _note_skip("sequence:" + mode, _fallback_reason(info0))
            pytest.skip(_fallback_reason(info0) + " (the sequence as it ran passes)")
        RAN["sequence:" + mode] = SEQ_STEPS
    finally:
        _automatic(eng)
        _automatic(eng2)


# ---------------------------------------------------------------------------------------------- z. the tally (keep this test last)
def test_zz_every_variant_ran_as_asked_somewhere():
    wanted = list(ALL_VARIANTS) + ["sequence:" + m for m in SEQ_MODES] + \
        [f"leaving:{'grid' if v == 2 else 'generic'}_lanes_{g}_{'wave' if m == 2 else 'lane'}_split" for v, g, m in LEAVE_PATHS]
    total = len(PATHS) + len(LEAVE_PATHS) + len(SEQ_MODES)
    if EXECUTED[0] < total or len(ORACLE_DONE) < len(BASES):
        pytest.skip(f"only {EXECUTED[0]} of the {total} path tests and {len(ORACLE_DONE)} of the {len(BASES)} oracle legs ran in this "
                    "process: nothing to sum")
    print("\nupdate paths: variants run as asked (field cases): " + ", ".join(f"{v} {RAN[v]}" for v in wanted if v in RAN))
    print("skipped: " + ("; ".join(f"{v}: {sorted(r)}" for v, r in sorted(SKIPPED.items())) if SKIPPED else "none"))
    print(f"leaving-domain preconditions: {LEAVING}")
    print("fields that moved the oracle's answer: " + ", ".join(f"{f} ({len(b)} bases)" for f, b in sorted(CHANGED.items())))
    missing = [v for v in wanted if v not in RAN]
    assert not missing, f"never ran as asked: {missing} (skipped: {SKIPPED})"
    fields = [name for name, _, _ in FIELD_CASES]
    assert not [f for f in fields if f not in CHANGED], f"fields that changed nothing anywhere: {[f for f in fields if f not in CHANGED]}"
    assert LEAVING.get("leave_mid_horizon", 0) > 20
