"""k_bfs_rows and k_bfs_rows2 at the edges of their work units: a wave skips the groups of four bitmap words (128 columns) that
no frontier cell can reach before the waves next exchange rows, D levels later (kRowsHalo = 7, kRows2Levels = 8).  The scenes
put the front on those edges: the group boundaries (columns 128 k), the wave boundaries (rows 50 k, rows2: 112 k), and the
cells that cross one at every phase of a block of levels.  All three MapGrids are compared bit for bit with the oracle, one
map size per kernel:

    W = 7    160 x 64    2 groups, 2 waves
    W = 13   400 x 110   4 groups, 3 waves
    W = 20   640 x 60    5 groups, 2 waves
    rows2    700 x 130   6 groups, 2 waves

The scenes of a size and family are the robots of one fleet.  Each fleet runs one cycle in the default bounded mode, the
robot's region straddling a group boundary (what that search left is read by the scoring: every sample's status and cost is
compared), and one with whole grids, which are downloaded and compared.

Level counts (empty and wall scenes, whole grids): a search runs blocks of D levels and stops at the first exchange that
finds nothing new in the block or nothing open in the region.  With M the largest finite distance, the cells at distance M
are found in block ceil(M / D).  If M is a multiple of D they are that block's last frontier, still open, and one more block
finds nothing: D (M / D + 1) levels.  Otherwise the frontier is empty when the block ends, and in these scenes every free
cell has been reached, so nothing is open: D ceil(M / D) levels.  Both are D (floor(M / D) + 1), and so is a search without
a seed on the map (one block that finds nothing).  D (ceil(M / D) + 1) is not what the kernel did before it skipped groups by
the block, e.g. M = 160 took 161 levels, so that is not asserted.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LETHAL, NOINFO = 254, 255
GROUP = 128    # columns of a group of four words
# kernel: map size, D = levels between two exchanges (kRowsHalo, kRows2Levels), rows a wave owns (kRowsPerWave, kRows2PerWave)
KERNELS = {"7": (160, 64, 7, 50), "13": (400, 110, 7, 50), "20": (640, 60, 7, 50), "rows2": (700, 130, 8, 112)}


@pytest.fixture(scope="module")
def nav():
    import navigation_amd as nav
    nav.lib()  # raises if libnavgpu.so is missing: no fallback
    assert nav.lib().navgpu_device_count() > 0, "no HIP device visible"
    return nav


def _boundaries(nx, ny):
    wave = next(w for kx, ky, _, w in KERNELS.values() if (kx, ky) == (nx, ny))
    return [c for c in range(GROUP, nx, GROUP)], [r for r in range(wave, ny, wave)]


def _point_plan(x, y, res):
    return np.array([[(x + 0.5) * res, (y + 0.5) * res]])


def _robot_for(goal_xy, nx, ny, res):
    """A pose 30 cells above or below the goal (a bounded search needs the goal further than twice the reach, 24.2 cells here)
    and 8 columns left of the group boundary nearest to it, so that the robot's box (+- 17 cells) straddles the boundary."""
    gx, gy = goal_xy
    cols, _ = _boundaries(nx, ny)
    c = min(cols, key=lambda b: abs(b - gx))
    y = gy - 30 if gy - 30 >= 3 else gy + 30
    assert 3 <= y < ny - 3
    return [(c - 8 + 0.5) * res, (y + 0.5) * res, 0.3]


def _scenes_empty(nx, ny, res):
    cols, rows = _boundaries(nx, ny)
    out = []
    for i, (dx, dy) in enumerate((dx, dy) for dx in range(-9, 10) for dy in range(-9, 10)):
        c, r = cols[i % len(cols)], rows[(i // len(cols)) % len(rows)]
        out.append((np.zeros((ny, nx), np.uint8), _point_plan(c + dx, r + dy, res), (c + dx, r + dy)))
    return out


def _scenes_gap_wall(nx, ny, res):
    """A wall along column 128 k - 1 / 128 k with one gap; the seed 1 .. 16 cells from the gap on either side: the only cell that
    crosses does so at every phase of a block."""
    cols, rows = _boundaries(nx, ny)
    out = []
    i = 0
    for off in (-1, 0):
        for s in range(1, 17):
            for side in (-1, 1):
                c, r = cols[i % len(cols)], rows[(i // len(cols)) % len(rows)]
                gap = r + (i % 5) - 2
                m = np.zeros((ny, nx), np.uint8)
                m[:, c + off] = LETHAL
                m[gap, c + off] = 0
                out.append((m, _point_plan(c + off + side * s, gap, res), (c + off + side * s, gap)))
                i += 1
    return out


def _scenes_wave_wall(nx, ny, res):
    """A wall along a wave's last row / the next one's first with one gap within 8 columns of a group boundary; the seed above or below the gap."""
    cols, rows = _boundaries(nx, ny)
    out = []
    i = 0
    for off in (-1, 0):
        for dc in range(-8, 9):
            for s in (1, 4, 7, 10):
                for side in (-1, 1):
                    c, r = cols[i % len(cols)], rows[(i // len(cols)) % len(rows)]
                    y = r + off + side * s
                    if not 0 <= y < ny:
                        y = r + off - side * s
                    m = np.zeros((ny, nx), np.uint8)
                    m[r + off, :] = LETHAL
                    m[r + off, c + dc] = 0
                    out.append((m, _point_plan(c + dc, y, res), (c + dc, y)))
                    i += 1
    return out


def _scenes_corridor(nx, ny, res):
    """A one-cell corridor along column 128 k; its left wall (column 128 k - 1) has a gap every 9 rows, so the front keeps
    poking into the neighbouring group from its edge bits."""
    cols, _ = _boundaries(nx, ny)
    out = []
    for c in cols:
        for phase in range(9):
            m = np.zeros((ny, nx), np.uint8)
            m[:, c - 1] = LETHAL
            m[:, c + 1] = LETHAL
            m[phase::9, c - 1] = 0
            m[ny - 1, c + 1] = 0  # the right-hand side is reached round the far end
            out.append((m, _point_plan(c, 0, res), (c, 0)))
    return out


def _scenes_clutter(nx, ny, res):
    rs = np.random.RandomState(1234 + nx)
    cols, _ = _boundaries(nx, ny)
    sx, sy = nx * res, ny * res
    out = []
    for i in range(20):
        m = np.zeros((ny, nx), np.uint8)
        for _ in range(max(3, nx * ny // 900)):
            cx, cy, r = rs.randint(0, nx), rs.randint(0, ny), rs.randint(1, 4)
            m[max(0, cy - r):cy + r + 1, max(0, cx - r):cx + r + 1] = LETHAL
        m[rs.random_sample(m.shape) < 0.01] = NOINFO
        plan = np.stack([np.linspace(0.1 * sx, 0.9 * sx, 40), np.linspace(0.2 * sy, 0.8 * sy, 40)], 1)
        if i % 2:
            plan = plan[::-1].copy()
        for px, py in plan:  # keep the plan itself traversable
            m[int(py / res), int(px / res)] = 0
        out.append((m, plan, (int(plan[-1, 0] / res), int(plan[-1, 1] / res))))
    return out


def _run(nav, orc, W, scenes, check_levels):
    from navigation_amd import _lib as N, synth
    nx, ny, D, _ = KERNELS[W]
    res = synth.RES
    n = len(scenes)
    cfg = nav.DwaConfig(vx_samples=3, vy_samples=1, vth_samples=3, sim_time=0.5, sim_granularity=0.1, discretize_by_time=1)
    masters = np.stack([s[0] for s in scenes])
    plans = [s[1] for s in scenes]
    pos = np.array([_robot_for(s[2], nx, ny, res) for s in scenes])
    vel = np.zeros((n, 3))
    # the reference, once
    ocfg = orc.DwaConfig(**cfg.as_dict())
    ref = []
    for k in range(n):
        p = orc.DwaPlanner(masters[k], res, 0.0, 0.0, ocfg)
        p.set_plan()
        o, _, _, cfull, st = p.cycle(pos[k].astype(np.float32), np.zeros(3, np.float32), plans[k], synth.FOOTPRINT)
        ref.append((o.best_index, o.n_valid, cfull, st, [p.grid(w).reshape(ny, nx) for w in range(3)]))

    fl = nav.Fleet(n, nx, ny, res, layers=N.LAYER_OBSTACLE, keep_sample_costs=True, max_sim_steps=16, max_plan=max(16, max(len(p) for p in plans)))
    try:
        fl.configure_planner(cfg)
        fl.set_footprint(synth.FOOTPRINT)
        fl.upload(N.GRID_MASTER, masters)
        fl.set_plan()
        lv = {}
        for bounded in (True, False):
            fl.set_bounded_map_grids(bounded)
            r = fl.find_best_path(pos, vel, plans)
            lv[bounded] = fl.wavefront_levels().astype(np.int64)
            if bounded:
                boxes = fl.wavefront_boxes()
                cols, _ = _boundaries(nx, ny)
                straddles = [any(b[0] < c <= b[1] for c in cols) for b in boxes]
                assert all(straddles), ("a robot's region does not straddle a group boundary", W, boxes[straddles.index(False)])
            for k in range(n):
                best, n_valid, cfull, st, _ = ref[k]
                cost, status, _ = fl.samples(k)
                assert (r[k].best_index, r[k].n_valid) == (best, n_valid), (W, k, bounded)
                assert np.array_equal(status, st), (W, k, bounded)
                scored = st == 1
                assert np.allclose(cost[scored], cfull[scored], rtol=0, atol=1e-5), (W, k, bounded)
        assert (lv[True] <= lv[False]).all()
        for gid, which in ((N.GRID_PATH, 0), (N.GRID_GOAL, 1), (N.GRID_GOAL_FRONT, 2)):
            g = fl.download(gid).astype(np.float64)
            og = np.stack([ref[k][4][which] for k in range(n)])
            bad = np.nonzero((g != og).reshape(n, -1).any(1))[0]
            assert bad.size == 0, f"MapGrid {which} differs ({nx}x{ny}) in scenes {bad[:8].tolist()}"
            if check_levels:
                far = np.where(og < nx * ny, og, -1.0).reshape(n, -1).max(1).astype(np.int64)
                want = D * (np.maximum(far, 0) // D + 1)  # (no seed on the map, far = -1: one block that finds nothing)
                got = lv[False][:, which]
                print(f"W={W} grid {which}: levels {got[:6].tolist()} want {want[:6].tolist()} M {far[:6].tolist()}")
                off = np.nonzero(got != want)[0]
                assert off.size == 0, (W, which, off[:8].tolist(), got[off[:8]].tolist(), want[off[:8]].tolist(), far[off[:8]].tolist())
    finally:
        fl.close()


FAMILIES = {"empty": (_scenes_empty, True), "gap_wall": (_scenes_gap_wall, True), "wave_wall": (_scenes_wave_wall, True),
            "corridor": (_scenes_corridor, False), "clutter": (_scenes_clutter, False)}


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("W", list(KERNELS))
def test_mapgrids_at_group_and_wave_boundaries(nav, orc, W, family):
    from navigation_amd import synth
    make, check_levels = FAMILIES[family]
    nx, ny = KERNELS[W][:2]
    _run(nav, orc, W, make(nx, ny, synth.RES), check_levels)
