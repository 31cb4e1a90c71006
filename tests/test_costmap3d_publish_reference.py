"""The publishing yardstick (tests/costmap3d_publish_ref.py) held to closed forms, on the CPU: the canonical prune against the
reference's own octree file and against cubes whose leaves can be counted by hand, the window-edge rule, negative keys, the diff
bounds, the forgotten boxes for every sign of a roll, updateCells and the subscription state machine."""
import itertools
import os

import numpy as np
import pytest

import costmap3d_publish_ref as pub
from costmap3d_layers_ref import ABSENT, FREE, LETHAL, NONLETHAL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "costmap3d")


def file_leaves():
    from navigation_amd.costmap3d import read_octomap_bt
    t = read_octomap_bt(os.path.join(GOLDEN, "aisles.bt"))
    level = np.rint(np.log2(t["sizes"] / t["res"])).astype(int)
    key = np.rint((t["centres"] - 0.5 * t["sizes"][:, None]) / t["res"]).astype(int)
    return {(int(k[0]), int(k[1]), int(k[2]), int(l), pub.CLS_LETHAL) for k, l in zip(key, level)}


def cells_of(leaves):
    out = []
    for kx, ky, kz, level, _ in leaves:
        r = range(1 << level)
        out += [(kx + i, ky + j, kz + k) for i in r for j in r for k in r]
    return out


def by_level(leaves):
    n = {}
    for l in leaves:
        n[l[3]] = n.get(l[3], 0) + 1
    return n


def test_the_prune_of_the_aisles_cells_is_the_files_leaf_set():
    leaves = file_leaves()
    assert by_level(leaves) == {0: 10421, 1: 33}
    cells = cells_of(leaves)
    assert len(cells) == len(set(cells)) == 10685
    assert pub.prune_cells(cells) == leaves


@pytest.mark.parametrize("corner", [(0, 0, 0), (-64, 64, -128)])
def test_a_full_aligned_cube_is_one_leaf_and_less_a_cell_it_is_42(corner):
    vol = np.full((64, 64, 64), LETHAL, np.uint8)
    assert pub.prune(vol, corner) == {corner + (6, pub.CLS_LETHAL)}
    for hole in ((0, 0, 0), (63, 63, 63), (21, 40, 7)):
        less = vol.copy()
        less[hole] = ABSENT
        leaves = pub.prune(less, corner)
        assert by_level(leaves) == {l: 7 for l in range(6)} and len(leaves) == 42
        assert sorted(cells_of(leaves)) == sorted((corner[0] + i, corner[1] + j, corner[2] + k) for i, j, k in zip(*np.nonzero(less)))


def test_a_cube_that_is_not_aligned_breaks_up():
    vol = np.full((64, 64, 64), LETHAL, np.uint8)
    assert by_level(pub.prune(vol, (32, 0, 0))) == {5: 8}
    block = np.full((2, 2, 2), NONLETHAL, np.uint8)
    assert pub.prune(block, (4, -6, 10)) == {(4, -6, 10, 1, pub.CLS_NONLETHAL)}
    for axis in range(3):
        ok = [4, -6, 10]
        ok[axis] += 1
        leaves = pub.prune(block, ok)
        assert by_level(leaves) == {0: 8} and {l[4] for l in leaves} == {pub.CLS_NONLETHAL}


def test_negative_keys_floor():
    block = np.full((4, 4, 4), FREE, np.uint8)
    assert pub.prune(block, (-4, -8, -12)) == {(-4, -8, -12, 2, pub.CLS_FREE)}
    assert by_level(pub.prune(block, (-3, -8, -12))) == {1: 4, 0: 32}  # x keys -3..0: the pair (-2, -1) merges, -3 and 0 stay cells
    assert pub.prune_cells([(-1, -1, -1)]) == {(-1, -1, -1, 0, pub.CLS_LETHAL)}


def test_classes_do_not_merge_and_window_edges_need_no_rule():
    block = np.full((2, 2, 2), LETHAL, np.uint8)
    block[1, 0, 1] = NONLETHAL
    leaves = pub.prune(block, (0, 0, 0))
    assert len(leaves) == 8 and sum(l[4] == pub.CLS_NONLETHAL for l in leaves) == 1
    # a window that starts at the odd key -13: the cell's sibling at -14 does not exist, so the parent cannot be full
    vol = np.zeros((8, 4, 4), np.uint8)
    vol[0, 0:2, 0:2] = LETHAL
    vol[1:3, 0:2, 0:2] = LETHAL
    assert by_level(pub.prune(vol, (-13, 4, 0))) == {0: 4, 1: 1}
    top = np.zeros((4, 4, 3), np.uint8)  # and at the upper z edge: levels 2 and 3 do not exist
    top[0:2, 0:2, 2] = LETHAL
    assert by_level(pub.prune(top, (0, 0, 0))) == {0: 4}


def test_the_delta_is_the_cells_that_differ_read_at_their_lattice_position():
    p = pub.Publisher()
    master = np.zeros((8, 8, 4), np.uint8)
    master[2, 3, 1] = LETHAL
    master[4:6, 4:6, 0:2] = NONLETHAL
    first = p.delta(master, (10, 20, 0))
    assert first["values"] == pub.prune(master, (10, 20, 0)) == {(12, 23, 1, 0, 0), (14, 24, 0, 1, 1)}
    assert first["bounds"] == {(12, 23, 1, 0, 0), (14, 24, 0, 1, 0)} and first["forgotten"] == [] and (first["update_seq"], first["bounds_seq"]) == (0, 0)
    again = p.delta(master, (10, 20, 0))
    assert again["values"] == set() and again["bounds"] == set() and again["update_seq"] == 1
    master[2, 3, 1] = FREE
    master[4:6, 4:6, 0:2] = ABSENT
    third = p.delta(master, (10, 20, 0))
    assert third["values"] == {(12, 23, 1, 0, pub.CLS_FREE)} and third["bounds"] == {(12, 23, 1, 0, 0), (14, 24, 0, 1, 0)}
    # the window moves by (+1, 0): the same world cells at other indices are no change
    moved = np.zeros_like(master)
    moved[1, 3, 1] = FREE
    fourth = p.delta(moved, (11, 20, 0))
    assert fourth["values"] == set() and fourth["bounds"] == set() and fourth["forgotten"] == [(10, 20, 0, 10, 27, 3)]
    full = p.full(moved, (11, 20, 0))
    assert (full["update_seq"], full["bounds_seq"], full["universe"]) == (4, 3, 1) and full["values"] == {(12, 23, 1, 0, pub.CLS_FREE)}
    assert pub.Publisher().full(moved, (11, 20, 0))["bounds_seq"] == 0xFFFFFFFF


@pytest.mark.parametrize("dx,dy", list(itertools.product((-3, 0, 2), (-2, 0, 5))) + [(-70, 0), (0, 9), (8, 8)])
def test_the_forgotten_boxes_cover_what_left_the_window(dx, dy):
    size, was = (8, 6, 4), (-5, 7, -2)
    now = (was[0] + dx, was[1] + dy, was[2])
    boxes = pub.forgotten_boxes(was, now, size)
    covered = np.zeros(size, int)
    for b in boxes:
        assert all(b[a] <= b[3 + a] for a in range(3)) and (b[2], b[5]) == (-2, 1)
        covered += pub.leaves_volume_box(b, was, size)
    want = np.ones(size, bool)
    want &= ~pub.leaves_volume_box((now[0], now[1], now[2], now[0] + size[0] - 1, now[1] + size[1] - 1, now[2] + size[2] - 1), was, size)
    assert np.array_equal(covered, want.astype(int))  # every cell that left exactly once
    assert len(boxes) == (0 if not want.any() else 1 if (dx == 0 or dy == 0 or want.all()) else 2)
    if dx and dy and len(boxes) == 2:  # the x strip over the old y range first, then the y strip over the remaining x range
        assert (boxes[0][1], boxes[0][4]) == (was[1], was[1] + size[1] - 1) and boxes[1][3] - boxes[1][0] + 1 == size[0] - abs(dx)


def test_update_cells_erases_inside_the_bounds_then_sets():
    ok, size = (-4, 0, 0), (8, 8, 8)
    vol = np.zeros(size, np.uint8)
    vol[0:4, 0:4, 0:4] = LETHAL
    vol[6, 6, 6] = FREE
    changed = np.zeros(size, bool)
    msg = dict(bounds={(-4, 0, 0, 1, 0), (2, 6, 6, 0, 0), (-8, 0, 0, 2, 0)},                      # the last one lies off the window
               values={(-4, 0, 0, 0, pub.CLS_NONLETHAL), (-4, 0, 0, 0, pub.CLS_FREE), (0, 4, 4, 1, pub.CLS_LETHAL)}, forgotten=[(-1, 3, 3, 5, 3, 3)])
    E = pub.update_cells(vol, changed, ok, msg, pub.AS_GIVEN)
    assert E.sum() == 8 + 1 + 5 and np.array_equal(changed, E)                                     # the forgotten box is clipped to x <= 3
    assert vol[0, 0, 0] == NONLETHAL and (vol[0:2, 0:2, 0:2] != ABSENT).sum() == 1                # erased, then the higher class of the two
    assert vol[6, 6, 6] == ABSENT and (vol[4:6, 4:6, 4:6] == ABSENT).all()                        # a value outside the bounds is ignored
    assert vol[3, 3, 3] == ABSENT and vol[2, 3, 3] == LETHAL and vol[3, 2, 3] == LETHAL
    binary = np.zeros(size, np.uint8)
    pub.update_cells(binary, np.zeros(size, bool), ok, dict(universe=1, values=msg["values"]), pub.BINARY)
    assert binary[0, 0, 0] == LETHAL and (binary[4:6, 4:6, 4:6] == LETHAL).all() and (binary != ABSENT).sum() == 9


def test_the_subscription_state_machine():
    s = pub.Subscription()
    assert s.verdict(5, 5) == pub.IGNORED                    # the first message is a normal update
    assert s.verdict(5, 4) == pub.RESYNC                     # the reference's quirk: whatever comes next resubscribes
    assert s.verdict(5, 4) == pub.APPLIED                    # the full map (sentinel), then updates in sequence
    assert s.verdict(5, 5) == pub.APPLIED and s.verdict(6, 6) == pub.APPLIED
    assert s.verdict(plain_map=True) == pub.IGNORED          # updates are in use
    assert s.verdict(3, 3) == pub.APPLIED                    # backwards is applied
    assert s.verdict(5, 5) == pub.RESYNC                     # a gap: 3 + 1 < 5
    assert s.verdict(7, 7) == pub.IGNORED and s.verdict(7, 6) == pub.RESYNC and s.verdict(7, 6) == pub.APPLIED
    w = pub.Subscription()
    assert w.verdict(plain_map=True) == pub.APPLIED          # before any update a plain map is taken
    assert w.verdict(0, 0xFFFFFFFF) == pub.APPLIED           # a first full map of a fresh publisher
    assert w.verdict(0, 0) == pub.APPLIED                    # 0xFFFFFFFF + 1 wraps to 0
    assert w.verdict(1, 1) == pub.APPLIED and w.verdict(3, 3) == pub.RESYNC
    lost = pub.Subscription()
    assert lost.verdict(9, 8) == pub.APPLIED and lost.verdict(10, 10) == pub.RESYNC and lost.verdict(10, 9) == pub.APPLIED
