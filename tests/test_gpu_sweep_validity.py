"""k_score_sweep decides VALIDITY, not failure codes, unless the codes are kept (navgpu_fleet_desc::keep_sample_costs).

A fleet without keep_sample_costs runs the sweep's KEEP = false form: a robot whose path / goal critic fails at its own cell leaves
by the robot-level exit (no image, no rollout), a lane stops at its first failure of any critic, no code is worked out.  Its
contract is the same navgpu_plan_result as the KEEP = true form, bit for bit.  Every scenario here is therefore built in TWO fleets
with identical inputs, one with and one without keep_sample_costs; the results are compared field by field (all but `reserved`)
between the two and against the oracle's findBestPath (DwaPlanner.cycle), and the winning trajectory where there is one.  The keep
fleet's per-sample costs, codes and statuses are compared with the oracle's as well: they only exist through the sweep's table path
(use_dwa, discretize_by_time), so the scenario is known to take the kernel under test.  Every scenario asserts through the oracle
that it is what it claims (which grid fails at the robot's own cell, which codes occur), so that no case can pass vacuously.

128 x 128 maps, four robots per fleet, 6 x 5 x 5 samples, 1 - 20 steps."""
import numpy as np
import pytest

from test_gpu_parity import INSCRIBED, LETHAL, NOINFO, L, nav  # noqa: F401

pytestmark = pytest.mark.gpu

N_CELLS = 128
C0 = N_CELLS // 2          # the robots' cell (64, 64): pose (3.225, 3.225)
GOAL = (C0 + 34, C0 + 10)  # the local goal's cell (x, y): 35 cells away, beyond every sample's reach
FIELDS = ("best_index", "n_samples", "n_scored", "n_valid", "n_points", "oscillation_flags", "xv", "yv", "thetav", "cost")
BASE = dict(vx_samples=6, vy_samples=5, vth_samples=5, sim_time=2.0, sim_granularity=0.1, discretize_by_time=1, use_dwa=1, allow_unknown=0)


def _bits(r):
    """Every field of a navgpu_plan_result but `reserved`, as exact bit patterns."""
    out = [np.asarray(getattr(r, f)).tobytes() for f in FIELDS]
    return out + [np.asarray(list(r.drive), np.float64).tobytes()]


def _same_result(a, b, what):
    for f, x, y in zip(FIELDS + ("drive",), _bits(a), _bits(b)):
        assert x == y, (what, f, getattr(a, f, None), getattr(b, f, None))


def _scene(orc, synth, kind, seed, unknown=False, goal=GOAL):
    """One robot's costmap (inflated), pose, velocity and plan.  kind: 'ordinary', 'sealed' (the local goal in a 9 x 9 lethal block),
    'blocked' (a lethal cell two cells from the robot's own cell: the robot stands in its inscribed zone, which the path grid's
    wavefront does not enter - the plan begins outside it, or its first cell would be a seed whatever it costs), 'both'."""
    rs = np.random.RandomState(seed)
    cells = np.zeros((N_CELLS, N_CELLS), np.uint8)
    yy, xx = np.mgrid[0:N_CELLS, 0:N_CELLS]
    d = np.hypot(xx - C0, yy - C0)
    cells[(rs.rand(N_CELLS, N_CELLS) < 0.006) & (d > 11) & (np.hypot(xx - goal[0], yy - goal[1]) > 14)] = LETHAL  # posts: the samples graze some
    if kind in ("sealed", "both"):
        cells[goal[1] - 4:goal[1] + 5, goal[0] - 4:goal[0] + 5] = LETHAL
    if kind in ("blocked", "both"):
        cells[C0 + 2, C0] = LETHAL
    master = orc.inflate(cells, synth.RES, synth.INFLATION_RADIUS, synth.COST_SCALING, synth.inscribed_radius(synth.FOOTPRINT), exact=True)
    if unknown:  # NO_INFORMATION cells in reach: legal (cost 255) with allow_unknown, obstacles in the MapGrids either way
        master[(rs.rand(N_CELLS, N_CELLS) < 0.004) & (master == 0) & (d > 6) & (d < 30)] = NOINFO
    c = (C0 + 0.5) * synth.RES
    pos = np.array([c, c, rs.uniform(-0.4, 0.7)], np.float32)
    vel = np.array([rs.uniform(0.2, 0.4), 0.0, rs.uniform(-0.3, 0.3)], np.float32)
    t = np.linspace(0.25 if kind in ("blocked", "both") else 0.0, 1.0, 80)
    plan = np.stack([c + t * (goal[0] - C0) * synth.RES, c + t * (goal[1] - C0) * synth.RES], 1)
    return dict(master=master, pos=pos, vel=vel, plan=plan)


def _pocket_scene(orc, synth, seed):
    """A closed ring of INSCRIBED cells with no lethal cell behind them, across the faster samples' reach: legal for the footprint's
    outline (pointCost fails LETHAL and NO_INFORMATION only, costmap_model.cpp), an obstacle in the path / goal grids (-3), its
    inside unreachable (-2) - the lanes that get there fail a MapGrid critic in mid-trajectory and no critic before it."""
    s = _scene(orc, synth, "ordinary", seed, goal=(C0, C0 + 35))  # straight up: the pocket is off the plan
    m = s["master"]
    m[C0 - 12:C0 + 13, C0 + 14:C0 + 29] = 0
    m[C0 - 12:C0 + 13, [C0 + 14, C0 + 28]] = INSCRIBED
    m[[C0 - 12, C0 + 12], C0 + 14:C0 + 29] = INSCRIBED
    s["pos"][2] = 0.05
    s["vel"][:] = (0.4, 0.0, 0.0)
    return s


class _Pair:
    """The same scenario in two fleets (with and without keep_sample_costs) and one oracle planner per robot."""

    def __init__(self, nav, orc, scenes, cfg_kw, fp):
        from navigation_amd import synth
        N = L(nav)
        self.fp, self.scenes, self.n = fp, scenes, len(scenes)
        self.cfg = nav.DwaConfig(**cfg_kw)
        ocfg = orc.DwaConfig(**self.cfg.as_dict())
        self.fleets = []
        for keep in (True, False):
            fl = nav.Fleet(self.n, N_CELLS, N_CELLS, synth.RES, layers=N.LAYER_OBSTACLE, max_sim_steps=32, max_plan=128, keep_sample_costs=keep)
            fl.configure_planner(self.cfg)
            fl.set_footprint(fp)
            fl.upload(N.GRID_MASTER, np.stack([s["master"] for s in scenes]))
            fl.set_plan()
            self.fleets.append(fl)
        self.keep, self.lean = self.fleets
        self.planners = [orc.DwaPlanner(s["master"], synth.RES, 0.0, 0.0, ocfg) for s in scenes]
        for p in self.planners:
            p.set_plan()

    def inputs(self, dyaw=0.0):
        pos = np.stack([s["pos"] for s in self.scenes]).astype(np.float32)
        pos[:, 2] += np.float32(dyaw)
        return pos, np.stack([s["vel"] for s in self.scenes]).astype(np.float32), np.stack([s["plan"] for s in self.scenes])

    def oracle(self, pos, vel, plans):
        """findBestPath per robot; with the path and goal grids' value at the robot's own cell."""
        out = []
        for k, p in enumerate(self.planners):
            o, traj, _, cfull, ost = p.cycle(pos[k], vel[k], plans[k], self.fp)
            out.append(dict(res=o, traj=traj, cost=cfull, status=ost, path0=p.grid(0)[C0, C0], goal0=p.grid(1)[C0, C0]))
        return out

    def check_results(self, rk, rl, orc_out, what):
        for k in range(self.n):
            _same_result(rk[k], rl[k], (what, "keep / lean", k))
            _same_result(rl[k], orc_out[k]["res"], (what, "lean / oracle", k))

    def check_samples_and_trajectories(self, orc_out, what):
        for k in range(self.n):
            o = orc_out[k]
            cost, status, _ = self.keep.samples(k)  # the table path's per-sample record: the sweep ran
            assert np.array_equal(status, o["status"]), (what, k)
            sc = status == 1
            neg = sc & (o["cost"] < 0)
            assert np.array_equal(cost[sc] < 0, o["cost"][sc] < 0) and np.array_equal(cost[neg], o["cost"][neg]), (what, k)
            assert np.array_equal(cost[sc & ~neg], o["cost"][sc & ~neg]), (what, k)
            assert self.keep.results(k, 1)[0].n_scored == int(sc.sum())
            if o["res"].best_index >= 0:
                tk, tl = self.keep.trajectory(k), self.lean.trajectory(k)
                assert tk.shape == tl.shape == o["traj"].shape and np.array_equal(tk, tl), (what, k)
                assert np.allclose(tl, o["traj"], rtol=0, atol=1e-6), (what, k)

    def cycle(self, what, dyaw=0.0):
        pos, vel, plans = self.inputs(dyaw)
        rk = self.keep.find_best_path(pos, vel, plans)
        rl = self.lean.find_best_path(pos, vel, plans)
        orc_out = self.oracle(pos, vel, plans)
        self.check_results(rk, rl, orc_out, what)
        self.check_samples_and_trajectories(orc_out, what)
        return rl, orc_out

    def close(self):
        for fl in self.fleets:
            fl.close()


def _failing(v):  # a MapGrid value that fails its critic: obstacleCosts() = cells, unreachableCellCosts() = cells + 1
    return v >= N_CELLS * N_CELLS


KINDS = ("sealed", "blocked", "both", "ordinary")
VARIANTS = {
    "base": dict(),
    "sum_scores": dict(sum_scores=1, occdist_scale=0.02),
    "two_point_footprint": dict(),
    "one_step": dict(sim_time=0.1),                  # K = 1: point 0 is also the last
    "eight_steps": dict(sim_time=0.8),
    "allow_unknown": dict(allow_unknown=1),
    "rollout_trig": dict(rollout_trig=1),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_sealed_blocked_both_and_ordinary_in_one_launch(nav, orc, variant):
    """start_fail = 5 (goal sealed), 4 (own cell blocked in the path grid), both, and an ordinary robot: one fleet, one launch."""
    from navigation_amd import synth
    fp = np.array([[0.15, 0.0], [-0.15, 0.0]]) if variant == "two_point_footprint" else synth.FOOTPRINT
    scenes = [_scene(orc, synth, kind, 10 + i, unknown=variant == "allow_unknown") for i, kind in enumerate(KINDS)]
    pair = _Pair(nav, orc, scenes, dict(BASE, **VARIANTS[variant]), fp)
    try:
        res, o = pair.cycle(variant)
        sealed, blocked, both, ordinary = range(4)
        # the scenarios are what they claim: which critic fails at the robot's own cell, by the oracle's grids
        assert _failing(o[sealed]["goal0"]) and not _failing(o[sealed]["path0"])
        assert _failing(o[blocked]["path0"]) and scenes[blocked]["master"][C0, C0] == INSCRIBED  # (no wavefront enters the inscribed zone)
        assert _failing(o[both]["path0"]) and _failing(o[both]["goal0"])
        assert not _failing(o[ordinary]["path0"]) and not _failing(o[ordinary]["goal0"])
        for k in (sealed, blocked, both):
            r = res[k]
            assert r.n_valid == 0 and r.best_index == -1 and r.cost == -7.0 and list(r.drive) == [0.0, 0.0, 0.0], (variant, k)
            assert r.n_scored == int((o[k]["status"] == 1).sum()) > 20, (variant, k)
            assert (o[k]["cost"][o[k]["status"] == 1] < 0).all()
        assert res[ordinary].n_valid > 0 and res[ordinary].best_index >= 0
        if variant not in ("one_step", "eight_steps", "two_point_footprint"):  # (given the reach) the ordinary robot's samples meet obstacles as well
            oc = o[ordinary]["cost"][o[ordinary]["status"] == 1]
            assert (oc == -6.0).any() and (oc >= 0).any()
    finally:
        pair.close()


def test_sealed_goal_with_goal_critics_off_does_not_take_the_exit(nav, orc):
    """goal_distance_bias = 0: the goal and goal_front critics are never evaluated, a sealed goal fails nothing."""
    from navigation_amd import synth
    scenes = [_scene(orc, synth, "sealed", 30), _scene(orc, synth, "ordinary", 31)]
    pair = _Pair(nav, orc, scenes, dict(BASE, goal_distance_bias=0.0), synth.FOOTPRINT)
    try:
        res, o = pair.cycle("goal bias 0")
        assert _failing(o[0]["goal0"]) and not _failing(o[0]["path0"])  # sealed all the same
        assert res[0].n_valid > 0 and res[0].best_index >= 0 and res[1].n_valid > 0
    finally:
        pair.close()


def test_pocket_fails_map_grid_critics_in_mid_trajectory(nav, orc):
    """Some lanes fail the path / goal critic on the way (-3 on the ring, -2 inside it) and stop there; others stay valid."""
    from navigation_amd import synth
    scenes = [_pocket_scene(orc, synth, 40), _pocket_scene(orc, synth, 41), _scene(orc, synth, "sealed", 42)]
    scenes[1]["vel"][:] = (0.3, 0.0, 0.2)
    pair = _Pair(nav, orc, scenes, dict(BASE), synth.FOOTPRINT)
    try:
        res, o = pair.cycle("pocket")
        for k in (0, 1):
            oc = o[k]["cost"][o[k]["status"] == 1]
            assert not _failing(o[k]["path0"]) and not _failing(o[k]["goal0"])
            assert ((oc == -3.0) | (oc == -2.0)).sum() >= 5 and (oc >= 0).sum() >= 5, (k, np.unique(oc[oc < 0], return_counts=True))
            assert res[k].n_valid == int((oc >= 0).sum()) > 0
        assert res[2].n_valid == 0
    finally:
        pair.close()


def test_two_cycles_in_flight_count_from_zero(nav, orc):
    """The sealed-goal fleet, two cycles queued back to back: every cycle's counters start from zero."""
    from navigation_amd import synth
    from navigation_amd._lib import PlanResult
    scenes = [_scene(orc, synth, kind, 50 + i) for i, kind in enumerate(("sealed", "sealed", "ordinary", "both"))]
    pair = _Pair(nav, orc, scenes, dict(BASE), synth.FOOTPRINT)
    try:
        ins = [pair.inputs(0.0), pair.inputs(0.15)]
        got = []
        for fl in pair.fleets:
            fl.set_cycles_in_flight(2)
            for pos, vel, plans in ins:
                fl.stage_planner(pos, vel, plans)
                fl.planner_cycle()
            first = list(fl.results_previous_into((PlanResult * pair.n)()))
            got.append((first, fl.results()))
        for c, (pos, vel, plans) in enumerate(ins):
            o = pair.oracle(pos, vel, plans)
            pair.check_results(got[0][c], got[1][c], o, ("in flight", c))
            for k in (0, 1, 3):
                r = got[1][c][k]
                assert _failing(o[k]["goal0"]) and r.n_valid == 0 and r.cost == -7.0
                assert r.n_scored == int((o[k]["status"] == 1).sum()) > 20
            assert got[1][c][2].n_valid > 0
    finally:
        pair.close()
