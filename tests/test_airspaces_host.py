"""Independent airspaces, on the host: the three scoring rules -- `envelope_from_rows`, `airspaces_from_envelopes`, `airspace_order`, the
specifications of `uavac_minsnap_envelope_dev`, `uavac_fleet_airspaces_dev` and of what `Engine.airspaces` chains behind them -- on
hand-made boxes, the prototypes, and THE THEOREM on the CPU: the prioritised searches run per airspace, on the missions in their
original relative order, give every mission the answer of the search over the whole group.  Nothing here needs a GPU."""
import os
import re

import numpy as np
import pytest

from conftest import REPO

RADIUS, VEL, DT = 0.5, 3.0, 0.02
DELTA, MAX_LAYERS = np.array([0.0, 0.0, -0.25]), 15
# the cuboids of tests/test_gpu_wide.py with x and y scaled by 3, for the missions spread by 3
CUBOIDS_3 = np.array([[33.39, 37.11, 18.63, 22.29, -20, 20], [9.51, 63.87, 4.83, 47.49, -4.613, -4.087]])


def spread_missions(B, spread, m=3):
    """`synthetic_missions(B, m)` with every mission moved away from the origin in x and y: its first waypoint times `spread`."""
    from oracle import minsnap_oracle as mo
    wps = mo.synthetic_missions(B, m)
    wps[:, :, :2] += (spread - 1) * wps[:, :1, :2]
    return wps


def base_starts(B):
    return (np.arange(B) % 5) * 7


def boxes(*lo_hi):
    a = np.array(lo_hi, dtype=np.float64)
    return a[:, :3].copy(), a[:, 3:].copy()


def unit(x, y=0.0, z=0.0):
    return [x, y, z, x + 1.0, y + 1.0, z + 1.0]


def components(lo, hi, radius, go=None):
    """The components by a plain search over the link matrix: what the labels must say at the fixed point."""
    B = len(lo)
    go = [0, B] if go is None else go
    with np.errstate(invalid="ignore"):
        link = ((lo[:, None, :] - hi[None, :, :] < radius).all(axis=2))
    link = link & link.T
    for g0, g1 in zip(go[:-1], go[1:]):
        link[g0:g1, :g0] = link[g0:g1, g1:] = False
    lab = np.arange(B)
    for b in range(B):
        if lab[b] != b:
            continue
        todo = [b]
        while todo:
            i = todo.pop()
            for j in np.flatnonzero(link[i]):
                if j != i and lab[j] > b:
                    lab[j] = b
                    todo.append(j)
    return lab, link


# ------------------------------------------------------------------------------------------------ 1: the rules on hand-made boxes
def test_envelope_from_rows_is_min_and_max_and_nan_for_what_has_no_box():
    from uav_ac.scoring import envelope_from_rows
    rows = np.array([[0, 0, 0], [2, -1, 5], [1, 3, -2], [7, 7, 7], [np.nan, 0, 0], [1, 1, 1]], dtype=np.float64)
    ro = np.array([0, 3, 3, 4, 5, 6])                       # mission 1 has no rows, mission 3 a NaN
    lo, hi = envelope_from_rows(rows, ro)
    assert lo[0].tolist() == [0, -1, -2] and hi[0].tolist() == [2, 3, 5] and lo[2].tolist() == hi[2].tolist() == [7, 7, 7]
    assert np.isnan(lo[[1, 3]]).all() and np.isnan(hi[[1, 3]]).all() and lo[4].tolist() == [1, 1, 1]
    reach = rows + np.array([0.0, 0.0, -4.0])
    reach[5, 1] = np.inf                                    # not finite on the other side only
    lo2, hi2 = envelope_from_rows(rows, ro, reach)
    assert lo2[0].tolist() == [0, -1, -6] and hi2[0].tolist() == [2, 3, 5] and lo2[2].tolist() == [7, 7, 3] and hi2[2].tolist() == [7, 7, 7]
    assert np.isnan(lo2[[1, 3, 4]]).all() and np.isnan(hi2[[1, 3, 4]]).all()
    with pytest.raises(ValueError, match="one row per row"):
        envelope_from_rows(rows, ro, reach[:-1])


def test_a_chain_links_its_ends_through_the_middle_and_the_gap_is_strict():
    from uav_ac.scoring import airspace_order, airspaces_from_envelopes
    # A - B - C along x: gaps of 0.25 between neighbours, 1.5 between A and C; D exactly 0.5 from C; E holds a NaN; F is far away
    lo, hi = boxes(unit(0.0), unit(1.25), unit(2.5), unit(4.0), [0, 0, 0, 1, np.nan, 1], unit(50.0))
    lab, link = components(lo, hi, 0.5)
    assert link[0, 1] and link[1, 2] and not link[0, 2] and not link[2, 3] and not link[4].any() and not link[:, 4].any()
    labels, changed, converged = airspaces_from_envelopes(lo, hi, 0.5)
    assert labels.dtype == np.int32 and labels.tolist() == lab.tolist() == [0, 0, 0, 3, 4, 5] and converged and changed >= 1
    assert airspaces_from_envelopes(lo, hi, np.nextafter(0.5, 1.0))[0].tolist() == [0, 0, 0, 0, 4, 5]      # just above the gap: D joins
    # radius 0: only boxes that overlap by more than a face; touching faces are a gap of exactly 0
    lo0, hi0 = boxes(unit(0.0), unit(1.0), unit(1.5), unit(10.0))
    assert airspaces_from_envelopes(lo0, hi0, 0.0)[0].tolist() == [0, 1, 1, 3]
    order, rank, offs = airspace_order(labels)
    assert order.tolist() == [0, 1, 2, 3, 4, 5] and offs.tolist() == [0, 3, 4, 5, 6]
    for bad in (-1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="radius"):
            airspaces_from_envelopes(lo, hi, bad)
    with pytest.raises(ValueError, match="rounds"):
        airspaces_from_envelopes(lo, hi, 0.5, rounds=0)


def test_groups_cut_the_links_and_the_order_keeps_an_airspace_in_its_order():
    from uav_ac.scoring import airspace_order, airspaces_from_envelopes
    # eight boxes on two spots, alternating: one group -> two airspaces that interleave; cut into groups of 0, 1, 3 and 4 missions
    lo, hi = boxes(*[unit(20.0 * (b % 2)) for b in range(8)])
    labels, _, converged = airspaces_from_envelopes(lo, hi, 0.5)
    assert converged and labels.tolist() == [0, 1, 0, 1, 0, 1, 0, 1]
    order, rank, offs = airspace_order(labels)
    assert order.tolist() == [0, 2, 4, 6, 1, 3, 5, 7] and offs.tolist() == [0, 4, 8] and rank[order].tolist() == list(range(8))
    go = np.array([0, 0, 1, 4, 8])
    labels, _, converged = airspaces_from_envelopes(lo, hi, 0.5, go)
    assert converged and labels.tolist() == components(lo, hi, 0.5, go)[0].tolist() == [0, 1, 2, 1, 4, 5, 4, 5]
    order, rank, offs = airspace_order(labels, go)
    assert order.tolist() == [0, 1, 3, 2, 4, 6, 5, 7] and offs.tolist() == [0, 1, 3, 4, 6, 8]
    # offsets that do not reach the end leave a tail that no group holds: linked to nobody
    assert airspaces_from_envelopes(lo, hi, 0.5, np.array([0, 4]))[0].tolist() == [0, 1, 0, 1, 4, 5, 6, 7]


def test_one_round_at_a_time_resumed_is_one_long_call_and_the_jump_saves_rounds():
    from uav_ac.scoring import airspaces_from_envelopes
    # a chain of 40 boxes laid out so that the batch index DESCENDS along it: box b stands at position 39 - b, and the lowest index sits
    # at the far end -- plain min-label propagation moves it one hop per round
    n = 40
    lo, hi = boxes(*[unit(1.25 * (n - 1 - b)) for b in range(n)])
    labels, changed, converged = airspaces_from_envelopes(lo, hi, 0.5)
    assert converged and (labels == 0).all()
    lab, plain = np.arange(n), 0                            # the same rule without the jump
    _, link = components(lo, hi, 0.5)
    while True:
        new = np.minimum(lab, np.where(link, lab[None, :], n).min(axis=1))
        if np.array_equal(new, lab):
            break
        lab, plain = new, plain + 1
    assert plain == n - 1 and changed < plain // 2, (changed, plain)
    # the same labels and the same count from calls of one round each, resumed
    lab1, total, calls = None, 0, 0
    while True:
        lab1, c, done = airspaces_from_envelopes(lo, hi, 0.5, rounds=1, labels=lab1)
        total, calls = total + c, calls + 1
        assert c == (0 if done else 1)
        if done:
            break
    assert np.array_equal(lab1, labels) and total == changed and calls == changed + 1
    short = airspaces_from_envelopes(lo, hi, 0.5, rounds=2)
    assert short[1:] == (2, False) and len(set(short[0].tolist())) > 1                  # not converged: a finer partition
    assert all(labels[b] == 0 for b in range(n)) and (short[0] <= np.arange(n)).all()


def test_prototypes_match_the_header_and_the_library_exports_them():
    import ctypes as C
    from uav_ac import _native as nat
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "uavac.h")).read(), flags=re.S)
    ctype = {"uavac_ctx *": C.c_void_p, "int": C.c_int, "double": C.c_double, "int64_t": C.c_int64}
    for name in ("uavac_minsnap_envelope_dev", "uavac_fleet_airspaces_dev"):
        proto = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert proto, name
        want = []
        for arg in proto.group(1).split(","):
            arg = " ".join(arg.split())
            want.append(C.c_void_p if "*" in arg else ctype[arg.rsplit(" ", 1)[0]])
        assert name in nat.exported_symbols()
        restype, argtypes = nat._SIGNATURES[name]
        assert restype is C.c_int and argtypes == want, (name, argtypes, want)
        assert hasattr(nat.lib(), name)
    lib = nat.lib()
    assert lib.uavac_version() == nat.VERSION == 310
    assert lib.uavac_minsnap_envelope_dev(None, None, None, None, 1, 1, 0.01, None, None) == nat.EINVAL           # no context
    assert lib.uavac_fleet_airspaces_dev(None, None, None, 0, 1, 0.5, 1, 0, None, None) == nat.EINVAL


def test_the_two_object_files_are_budgeted():
    from uav_ac import _buildcheck as bc
    rows = {r.obj: r for r in bc.BUDGETS}
    env, air = rows["minsnap_envelope.o"], rows["fleet_airspaces.o"]
    assert env.key == "planning_registers" and env.limit == 168 and env.at_least == 4 and env.scratch_free
    assert air.kernels == ("airspace_begin_kernel", "airspace_link_kernel", "airspace_jump_kernel", "airspace_info_kernel") and air.scratch_free
    built = bc.check_airspace_kernels()
    if built is None:
        pytest.skip("no object files / LLVM tools here (library built elsewhere)")
    assert len(built) == 4 and max(built.values()) <= 64
    assert sum("minsnap_envelope_kernel" in n for n, _, _ in bc.check_planning_registers()) == 4


# ------------------------------------------------------------------------------------------------ 2: the theorem, on the CPU
_CASE = {}


def oracle_case(B=150, spread=3):
    """Rows of the oracle's own solve and sampler for the spread missions, computed once and left unchanged."""
    if (B, spread) not in _CASE:
        from oracle import minsnap_oracle as mo
        parts = [mo.plan(w, VEL, DT, "solve") for w in spread_missions(B, spread)]
        ro = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
        _CASE[(B, spread)] = (np.concatenate(parts), ro)
    return _CASE[(B, spread)]


def nontrivial(labels, link, stag=None):
    """What a case must show for the comparison to mean anything, asserted on the rule's own answer."""
    sizes = np.bincount(labels, minlength=len(labels))
    assert (sizes >= 2).sum() >= 3 and (sizes == 1).any(), sizes[sizes > 0]
    no_clique = [c for c in np.flatnonzero(sizes >= 3) if not (link[np.ix_(labels == c, labels == c)] | np.eye(sizes[c], dtype=bool)).all()]
    assert no_clique, "every airspace is a clique"
    if stag is not None:
        assert (stag[1] > 0).any() and (stag[1] == -1).any(), np.unique(stag[1], return_counts=True)


def per_airspace_earlier(labels, examined):
    """How many examined missions of its airspace come before each examined mission, in batch order."""
    want = np.zeros(len(labels), dtype=np.int32)
    seen = {}
    for b in range(len(labels)):
        if examined[b]:
            want[b] = seen.get(labels[b], 0)
            seen[labels[b]] = want[b] + 1
    return want


def test_the_searches_per_airspace_give_the_answers_of_the_whole_group():
    from uav_ac.scoring import (airspace_order, airspaces_from_envelopes, envelope_from_rows, layer_obstacles_from_rows, stagger_from_rows,
                                take_rows)
    B = 150
    rows, ro = oracle_case(B, 3)
    start = base_starts(B)

    # start delays: the boxes of the rows as they are
    lo, hi = envelope_from_rows(rows, ro)
    labels, _, converged = airspaces_from_envelopes(lo, hi, RADIUS)
    truth, link = components(lo, hi, RADIUS)
    assert converged and np.array_equal(labels, truth)
    whole = stagger_from_rows(rows, ro, RADIUS, None, start, max_group=B)
    nontrivial(labels, link, whole)
    order, rank, offs = airspace_order(labels)
    rows_t, ro_t = take_rows(rows, ro, order)
    split = stagger_from_rows(rows_t, ro_t, RADIUS, offs, start[order], max_group=B)[:, rank]
    assert np.array_equal(split[:2], whole[:2])                                       # start rows and steps, all 150
    assert np.array_equal(split[2], per_airspace_earlier(labels, whole[1] != -2)) and (split[2] != whole[2]).sum() > B // 2

    # layers at the granted starts: the boxes must cover every layer 0 .. MAX_LAYERS
    granted = whole[0]

    def layered(r):
        memo = {}

        def rows_at(q):
            if q not in memo:
                memo[q] = r[:, 0:3] + q * DELTA
            return memo[q]
        return rows_at
    lo, hi = envelope_from_rows(rows, ro, layered(rows)(MAX_LAYERS))
    for q in range(MAX_LAYERS + 1):                                                   # (the monotonicity the box argument rests on)
        lq, hq = envelope_from_rows(layered(rows)(q), ro)
        assert (lq >= lo).all() and (hq <= hi).all()
    labels, _, converged = airspaces_from_envelopes(lo, hi, RADIUS)
    truth, link = components(lo, hi, RADIUS)
    assert converged and np.array_equal(labels, truth)
    nontrivial(labels, link)
    whole = layer_obstacles_from_rows(layered(rows), ro, RADIUS, CUBOIDS_3, None, granted, MAX_LAYERS, max_group=B)
    assert (whole[0] > 0).any() and (whole[1] == -1).any() and (whole[3] > 0).any(), "nobody moved, unresolved or blocked"
    order, rank, offs = airspace_order(labels)
    rows_t, ro_t = take_rows(rows, ro, order)
    split = layer_obstacles_from_rows(layered(rows_t), ro_t, RADIUS, CUBOIDS_3, offs, granted[order], MAX_LAYERS, max_group=B)[:, rank]
    assert np.array_equal(split[[0, 1, 3]], whole[[0, 1, 3]])                           # layer, steps, blocked
    assert np.array_equal(split[2], per_airspace_earlier(labels, whole[1] != -2))
