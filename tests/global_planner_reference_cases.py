"""The cases of tests/golden/g18_global_planner_reference.npz, shared by tools/make_global_planner_goldens.py (which runs the reference's
own global_planner classes on them), tests/test_global_planner_reference.py (which holds oracle/global_planner_oracle.hpp to what they
gave and checks that the cases reach what they are there for) and tests/test_gpu_global_planner_reference.py (which holds k_gp_plan to
the same file).  A case is one plan at the level of navgpu_global_planner_plan: a costmap as the caller hands it over (outlineMap not
yet applied), start and goal in map coordinates as GlobalPlanner::makePlan computes them, and the planner's parameters.

Maps are 24 to 64 cells a side; starts and goals keep three cells from every edge (nearer ones are rejected by the library, and the
reference reads outside its arrays there).  What each map is for is said where it is built; test_cases_reach_what_they_are_for asserts
it from the inputs and the recorded results, so an edit here cannot silently drop a condition."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_global_planner_reference.npz")
PARAM_KEYS = ("use_dijkstra", "use_quadratic", "use_grid_path", "old_navfn_behavior", "allow_unknown", "lethal_cost", "neutral_cost", "outline_map")
DEFAULTS = dict(use_dijkstra=1, use_quadratic=1, use_grid_path=0, old_navfn_behavior=0, allow_unknown=1, lethal_cost=253, neutral_cost=50,
                outline_map=1, cost_factor=3.0)
POT_HIGH = np.float32(1.0e10)
MAX_SIDE = 64


def full_params(kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def goal_cell(c):
    return int(c["goal"][0]), int(c["goal"][1])


def outlined(c):
    """the costmap as calculatePotentials sees it: GlobalPlanner::outlineMap's 254 border unless the case turns it off"""
    cm = np.array(c["cmap"], np.uint8)
    if full_params(c["params"])["outline_map"]:
        cm[0, :] = cm[-1, :] = 254
        cm[:, 0] = cm[:, -1] = 254
    return cm


def pad(a, fill):
    out = np.full((MAX_SIDE, MAX_SIDE), fill, a.dtype)
    out[:a.shape[0], :a.shape[1]] = a
    return out


# ------------------------------------------------------------------------------------------------ the maps
def _rings(cm, values=(230, 140, 60)):
    """an inflation layer's look: rings of falling cost round every 254 cell"""
    solid = cm == 254
    reach = solid.copy()
    for v in values:
        grown = reach.copy()
        grown[1:, :] |= reach[:-1, :]
        grown[:-1, :] |= reach[1:, :]
        grown[:, 1:] |= reach[:, :-1]
        grown[:, :-1] |= reach[:, 1:]
        cm[grown & ~reach & (cm == 0)] = v
        reach = grown
    return cm


def _specials(cm, x, y, lethal):
    """five lone cells on row y from column x, two apart, on cleared ground: lethal - 2 (the last cost Dijkstra enters), lethal - 1 (A*
    enters it, Dijkstra does not), lethal, 254 and 255 (entered only when unknown cells are allowed)"""
    cm[y - 1:y + 2, x - 1:x + 10] = 0
    for i, v in enumerate((lethal - 2, lethal - 1, lethal, 254, 255)):
        cm[y, x + 2 * i] = min(v, 255)
    return cm


def field_map(lethal=253):
    """48 x 40: blocks with cost rings, speckled costs of every size (cost * factor + neutral reaches the clamp) and the special cells
    in the start's corner"""
    rs = np.random.RandomState(1801)
    cm = np.zeros((40, 48), np.uint8)
    for x0, y0, w, h in ((14, 6, 5, 9), (26, 20, 4, 12), (8, 26, 9, 3), (34, 8, 6, 4)):
        cm[y0:y0 + h, x0:x0 + w] = 254
    _rings(cm)
    sp = (rs.random_sample(cm.shape) < 0.12) & (cm == 0)
    cm[sp] = rs.randint(1, 200, sp.sum())
    cm[3:9, 3:9] = 0            # round the start
    _specials(cm, 3, 11, lethal)
    cm[30:36, 39:45] = 0        # round the goal
    return cm


FIELD_START, FIELD_GOAL = (5.37, 5.62), (41.4, 32.7)


def endpoint_map():
    """31 x 24 (odd nx): open ground, and on the far side of the goal's 5 x 5 block (columns 20 - 24, rows 10 - 14) cells the expansion
    stops short of: free ones, a 206, a 230, a 254 and a 255.  Expander::clearEndpoint gives each a potential from costs + neutral_cost
    handed over as an unsigned char: 256 and more wrap round"""
    cm = np.zeros((24, 31), np.uint8)
    cm[14, 24], cm[13, 24], cm[14, 23], cm[12, 24] = 206, 230, 254, 255
    return cm


ENDPOINT_START, ENDPOINT_GOAL = (5.4, 6.3), (22.6, 12.3)


def speckle_case(seed, n=40, **params):
    """a start and a goal drawn on speckle_map(seed, n), the ground round both cleared"""
    rs = np.random.RandomState(seed)
    cm = speckle_map(seed, n)
    s, g = rs.uniform(5, n - 7, 2), rs.uniform(5, n - 7, 2)
    for x, y in (s, g):
        cm[int(y) - 1:int(y) + 3, int(x) - 1:int(x) + 3] = 0
    return _case(f"speckle{seed}", cm, s, g, **params)


def wall_map():
    """37 x 29 (odd nx): a wall from the left edge whose end the path rounds - grid steps beside its POT_HIGH cells - with gradient steps
    on the open ground either side"""
    cm = np.zeros((29, 37), np.uint8)
    cm[14, 0:27] = 254
    cm[13, 20:27] = 254
    return cm


def serpentine_map():
    """64 x 64: a wall every 6 rows with an 8-cell gap on alternating sides (tests/global_plan_ref.py's): a path of several hundred
    points, a goal potential many priority steps above lethal_cost"""
    n = 64
    cm = np.zeros((n, n), np.uint8)
    for j, row in enumerate(range(9, n - 6, 6)):
        cm[row, :] = 254
        if j % 2 == 0:
            cm[row, n - 10:n - 2] = 0
        else:
            cm[row, 2:10] = 0
    return cm


def open_map():
    """33 x 24, nothing on it: A*'s keys tie all over the heap"""
    return np.zeros((24, 33), np.uint8)


def astar_map():
    """40 x 28 for A* with neutral_cost 50 and lethal_cost 253: in front of a doorway a column of costs 206 ... 252 (costs + neutral_cost is
    narrowed to unsigned char there: a 230 costs 24), with a 252 - the last cost A* enters -, a 253 and a 254 beside the door; further on a
    column of 255 with a gap"""
    cm = np.zeros((28, 40), np.uint8)
    cm[4:24, 14] = 206 + 2 * np.arange(20)
    cm[12:16, 14] = 252, 230, 253, 254
    cm[4:24, 15] = 254
    cm[12:16, 15] = 0
    cm[4:24, 24] = 255
    cm[18:20, 24] = 0
    cm[0:4, 10:30] = 254
    cm[24:28, 10:30] = 254
    return cm


def sealed_map():
    """30 x 26: the goal inside a closed box"""
    cm = np.zeros((26, 30), np.uint8)
    cm[8:18, 16] = cm[8:18, 26] = 254
    cm[8, 16:27] = cm[17, 16:27] = 254
    return cm


def walled_border_map():
    """36 x 24 whose border is lethal already, for outline_map = 0"""
    cm = np.zeros((24, 36), np.uint8)
    cm[0, :] = cm[-1, :] = 254
    cm[:, 0] = cm[:, -1] = 254
    cm[6:24, 17] = 254
    _rings(cm, (200, 90))
    return cm


def speckle_map(seed, n=48, density=0.03):
    """tests/test_navfn.py's random costmaps (3 % lethal cells, 15 % single-cell costs, 1 % unknown): GradientPath zig-zags beside the
    single-cell spikes until its oscillation test fires"""
    rs = np.random.RandomState(seed)
    cm = np.zeros((n, n), np.uint8)
    cm[rs.random_sample((n, n)) < density] = 254
    blur = (rs.random_sample((n, n)) < 0.15) & (cm == 0)
    cm[blur] = rs.randint(1, 253, blur.sum())
    cm[(rs.random_sample((n, n)) < 0.01) & (cm == 0)] = 255
    return cm


def _case(name, cmap, start, goal, **params):
    if params.get("old_navfn_behavior"):  # makePlan plans from the cells themselves then (planner_core.cpp:261-263, :276-278)
        start, goal = (float(int(start[0])), float(int(start[1]))), (float(int(goal[0])), float(int(goal[1])))
    return dict(name=name, cmap=cmap, start=(float(start[0]), float(start[1])), goal=(float(goal[0]), float(goal[1])), params=params)


# the parameter sets of tests/test_goldens.py's G8_VARIANTS and tests/test_navfn.py's GP_WF_VARIANTS, once each
VARIANT_SETS = [dict(), dict(use_quadratic=0, use_grid_path=1), dict(use_dijkstra=0, use_grid_path=1), dict(old_navfn_behavior=1),
                dict(use_dijkstra=0), dict(allow_unknown=0, cost_factor=0.55, neutral_cost=66), dict(use_quadratic=0), dict(use_grid_path=1)]


def cases():
    out = []
    field = field_map()
    for k, kw in enumerate(VARIANT_SETS):
        out.append(_case(f"field_v{k}", field, FIELD_START, FIELD_GOAL, **kw))
    # neutral_cost either side of the constructor's 50, both calculators; the first set is VARIANT_SETS[5]
    out.append(_case("field_n66_linear", field, FIELD_START, FIELD_GOAL, neutral_cost=66, cost_factor=0.55, use_quadratic=0))
    out.append(_case("field_n30", field, FIELD_START, FIELD_GOAL, neutral_cost=30, use_grid_path=1))
    out.append(_case("field_n30_linear", field, FIELD_START, FIELD_GOAL, neutral_cost=30, use_quadratic=0, cost_factor=2.0, use_grid_path=1))
    # lethal_cost 255 and 200
    out.append(_case("field_l255", field_map(255), FIELD_START, FIELD_GOAL, lethal_cost=255))
    out.append(_case("field_l255_known", field_map(255), FIELD_START, FIELD_GOAL, lethal_cost=255, allow_unknown=0))
    out.append(_case("field_l200", field_map(200), FIELD_START, FIELD_GOAL, lethal_cost=200, cost_factor=1.5))
    out.append(_case("field_l200_astar", field_map(200), FIELD_START, FIELD_GOAL, lethal_cost=200, use_dijkstra=0, use_grid_path=1))
    out.append(_case("field_known_astar", field, FIELD_START, FIELD_GOAL, use_dijkstra=0, use_grid_path=1, allow_unknown=0))
    # precise start: an offset that rounds to 1, an integral start
    out.append(_case("field_start_rounds_up", field, (5.996, 5.31), FIELD_GOAL))
    out.append(_case("field_start_integral", field, (6.0, 5.0), FIELD_GOAL))
    wall = wall_map()
    out.append(_case("wall", wall, (5.3, 5.6), (6.4, 22.7)))
    out.append(_case("wall_linear", wall, (5.3, 5.6), (6.4, 22.7), use_quadratic=0))
    out.append(_case("wall_n30", wall, (5.3, 5.6), (6.4, 22.7), neutral_cost=30))
    out.append(_case("wall_astar_grid", wall, (5.3, 5.6), (6.4, 22.7), use_dijkstra=0, use_grid_path=1))
    serp = serpentine_map()
    out.append(_case("serpentine", serp, (4.3, 4.6), (58.2, 59.4)))
    out.append(_case("serpentine_astar", serp, (4.3, 4.6), (58.2, 59.4), use_dijkstra=0, use_grid_path=1))
    out.append(_case("open_astar_grid", open_map(), (4.5, 4.5), (27.5, 18.5), use_dijkstra=0, use_grid_path=1))
    out.append(_case("open_astar_gradient_fails", open_map(), (17.2, 5.51), (15.22, 4.53), use_dijkstra=0))
    out.append(_case("open_astar_gradient_circles", open_map(), (12.3, 19.7), (27.6, 5.2), use_dijkstra=0))
    out.append(_case("open_astar_gradient_arrives", open_map(), (6.5, 12.5), (27.5, 12.5), use_dijkstra=0))
    am = astar_map()
    out.append(_case("astar_bands", am, (5.5, 13.5), (33.5, 14.5), use_dijkstra=0, use_grid_path=1))
    out.append(_case("astar_bands_linear", am, (5.5, 13.5), (33.5, 14.5), use_dijkstra=0, use_grid_path=1, use_quadratic=0))
    out.append(_case("astar_bands_known", am, (5.5, 13.5), (33.5, 14.5), use_dijkstra=0, use_grid_path=1, allow_unknown=0))
    ep = endpoint_map()
    out.append(_case("endpoint", ep, ENDPOINT_START, ENDPOINT_GOAL))
    out.append(_case("endpoint_grid", ep, ENDPOINT_START, ENDPOINT_GOAL, use_grid_path=1))
    out.append(_case("endpoint_linear_known", ep, ENDPOINT_START, ENDPOINT_GOAL, use_quadratic=0, allow_unknown=0, use_grid_path=1))
    out.append(_case("endpoint_n66", ep, ENDPOINT_START, ENDPOINT_GOAL, neutral_cost=66, use_grid_path=1))
    out.append(_case("endpoint_astar", ep, ENDPOINT_START, ENDPOINT_GOAL, use_dijkstra=0, use_grid_path=1))
    out.append(speckle_case(38))
    out.append(speckle_case(29))
    sealed = sealed_map()
    out.append(_case("sealed", sealed, (5.4, 12.6), (21.5, 12.5)))
    out.append(_case("sealed_astar", sealed, (5.4, 12.6), (21.5, 12.5), use_dijkstra=0))
    wb = walled_border_map()
    out.append(_case("walled_border_no_outline", wb, (6.4, 12.3), (29.6, 15.2), outline_map=0))
    return out


# ------------------------------------------------------------------------------------------------ the fixture
class Plan:
    """one recorded plan: inputs cropped to the map's shape, and the reference's results"""

    def __init__(self, g, k):
        ny, nx = (int(v) for v in g["map_shapes"][g["map_index"][k]])
        self.name = str(g["names"][k])
        self.cmap = g["maps"][g["map_index"][k]][:ny, :nx]
        self.params = {key: int(v) for key, v in zip(PARAM_KEYS, g["params"][k])}
        self.params["cost_factor"] = float(g["cost_factors"][k])
        self.start, self.goal = g["starts"][k], g["goals"][k]
        self.goal_cell = g["goal_cells"][k]
        self.found_legal = int(g["found_legal"][k])
        self.potential_before = g["potential_before"][k][:ny, :nx]
        self.potential = g["potential"][k][:ny, :nx]
        self.path_ret, self.path_len = int(g["path_ret"][k]), int(g["path_len"][k])
        at = int(g["path_len"][:k].sum())
        self.path = g["path"][at:at + self.path_len]

    @property
    def seen(self):
        """the costmap as the expansion saw it"""
        return outlined(dict(cmap=self.cmap, params=self.params))

    @property
    def goal_block(self):
        m = np.zeros(self.cmap.shape, bool)
        m[self.goal_cell[1] - 2:self.goal_cell[1] + 3, self.goal_cell[0] - 2:self.goal_cell[0] + 3] = True
        return m


def load(path=GOLDEN):
    """-> (list of Plan, meta dict)"""
    g = np.load(path)
    return [Plan(g, k) for k in range(len(g["names"]))], json.loads(str(g["meta"]))
