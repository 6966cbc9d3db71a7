"""The four fleet specifications of `uav_ac.scoring` -- `separation_from_rows`, `stagger_from_rows`, `layer_from_rows` and
`layer_obstacles_from_rows`, the NumPy rules the fleet kernels are tested against bit for bit -- against a deliberately naive
restatement: scalar Python `float` arithmetic, triple loops over missions, clock rows and partners, written from the docstrings alone
and sharing nothing with `scoring` but its public names.  Equality is exact, array for array.

Small seeded fleets: 16 missions in the groups [0, 4, 4, 9, 10, 16] (an empty group and a group of one), 3 .. 12 rows each, straight
lines between points on a 0.25 grid in the unit cube, one mission without rows, one with a NaN coordinate, start rows -2 .. 5."""
import math

import numpy as np
import pytest

SEEDS = range(6)
B, GROUPS, RADIUS = 16, [0, 4, 4, 9, 10, 16], 0.3
STEP, STAGGER_STEPS = 2, 6
DELTA, LAYER_STEPS, CUBOID = (0.0, 0.0, -0.25), 3, [0.2, 0.8, 0.2, 0.8, -0.3, 0.6]
MAX_CLOCK = 1 << 29


def fleet(seed):
    """-> rows (N, 11), row_offsets (B + 1,), start_rows (B,)"""
    rng = np.random.default_rng(seed)
    n = rng.integers(3, 13, B)
    n[6] = 0
    ends = rng.integers(0, 5, (B, 2, 3)) * 0.25
    starts = rng.integers(-2, 6, B)
    ro = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    rows = np.zeros((int(ro[-1]), 11))
    for b in range(B):
        if n[b]:
            rows[ro[b]:ro[b + 1], 0:3] = np.linspace(ends[b, 0], ends[b, 1], n[b])
    rows[ro[12] + 1, int(rng.integers(0, 3))] = np.nan
    return rows, ro, starts


class Layers:
    """rows_at for given rows: layer q is the positions with q * DELTA added; memoised, and it records which layers were asked for."""

    def __init__(self, rows):
        self.rows, self.memo, self.asked = rows, {}, []

    def __call__(self, q):
        self.asked.append(q)
        if q not in self.memo:
            self.memo[q] = self.rows[:, 0:3] + q * np.asarray(DELTA) if q else self.rows[:, 0:3]
        return self.memo[q]


# ------------------------------------------------------------------------------------------------ the naive restatements
def inside(p, q, r2):
    dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
    return (dx * dx + dy * dy) + dz * dz < r2


def at(pos, ro, b, k, s):
    """where mission b with start s stands at clock row k: its own row clamp(k - s, 0, N_b - 1), as three floats"""
    n = int(ro[b + 1] - ro[b])
    r = int(ro[b]) + min(max(k - s, 0), n - 1)
    return float(pos[r][0]), float(pos[r][1]), float(pos[r][2])


def finite_rows(pos, ro, b):
    return all(math.isfinite(float(pos[r][c])) for r in range(int(ro[b]), int(ro[b + 1])) for c in range(3))


def naive_separation(rows, ro, radius, go, starts):
    N = [int(ro[b + 1] - ro[b]) for b in range(B)]
    S = [max(0, int(s)) for s in starts]
    inc = [N[b] > 0 and finite_rows(rows, ro, b) for b in range(B)]
    r2 = radius * radius
    sep, isep = [math.nan] * B, [[-1] * B, [-1] * B, [0] * B, [-1] * B, [0] * B]
    for g in range(len(go) - 1):
        members = [b for b in range(go[g], go[g + 1]) if inc[b]]
        H = max([S[b] + N[b] for b in members], default=0)
        for b in members:
            best, partners, first = (math.inf, -1, -1), set(), -1
            for k in range(H):
                p = at(rows, ro, b, k, S[b])
                for j in members:
                    if j == b:
                        continue
                    q = at(rows, ro, j, k, S[j])
                    dx, dy, dz = p[0] - q[0], p[1] - q[1], p[2] - q[2]
                    d2 = (dx * dx + dy * dy) + dz * dz
                    if (d2, k, j) < best:
                        best = (d2, k, j)
                    if d2 < r2:
                        partners.add(j)
                        first = k if first < 0 else first
            sep[b] = math.sqrt(best[0])
            isep[0][b], isep[1][b], isep[2][b], isep[3][b], isep[4][b] = best[2], best[1], len(partners), first, len(members) - 1
    return np.array(sep), np.array(isep, dtype=np.int32)


def naive_search(ro, radius, go, max_steps, included_on, candidate, blocked=None):
    """The prioritised search as the three docstrings state it.  candidate(i, q) -> (positions, start) of mission i's candidate q;
    a granted candidate is what a later mission is checked against.  blocked(i, q): a cuboid refuses the candidate (then every
    included mission is examined, the first of its group too)."""
    N = [int(ro[b + 1] - ro[b]) for b in range(B)]
    inc = [0 < N[b] <= MAX_CLOCK and finite_rows(included_on, ro, b) for b in range(B)]
    r2 = radius * radius
    out = [[0] * B, [-2] * B, [0] * B, [0] * B]              # granted candidate, steps, earlier, blocked
    for g in range(len(go) - 1):
        done = []                                            # (mission, positions, start) of the decided ones
        for i in range(go[g], go[g + 1]):
            if not inc[i]:
                continue
            out[2][i], steps, refused = len(done), -1, 0
            for q in range(max_steps + 1):
                if blocked is not None and blocked(i, q):
                    refused += 1
                    continue
                clear = True
                if done:
                    pos_i, s = candidate(i, q)
                    for j, pos_j, t in done:
                        for k in range(max(s + N[i], t + N[j])):
                            if inside(at(pos_i, ro, i, k, s), at(pos_j, ro, j, k, t), r2):
                                clear = False
                if clear:
                    steps = q
                    break
            out[0][i], out[1][i], out[3][i] = max(steps, 0), steps, refused
            done.append((i,) + candidate(i, max(steps, 0)))
    return np.array(out, dtype=np.int32)


def naive_stagger(rows, ro, radius, go, starts, step, max_steps):
    S = [min(max(int(s), 0), MAX_CLOCK) for s in starts]
    out = naive_search(ro, radius, go, max_steps, rows, lambda i, q: (rows, S[i] + q * step))
    granted = [S[b] + max(int(out[1][b]), 0) * step for b in range(B)]
    return np.array([granted, out[1], out[2]], dtype=np.int32)


def naive_layers(rows_at, ro, radius, go, starts, max_steps, cuboids=None):
    S = [min(max(int(s), 0), MAX_CLOCK) for s in starts]

    def blocked(i, q):
        p = rows_at(q)
        for r in range(int(ro[i]), int(ro[i + 1])):
            x, y, z = float(p[r][0]), float(p[r][1]), float(p[r][2])
            for c in cuboids:
                if x >= c[0] and x <= c[1] and y >= c[2] and y <= c[3] and z >= c[4] and z <= c[5]:
                    return True
        return False

    out = naive_search(ro, radius, go, max_steps, rows_at(0), lambda i, q: (rows_at(q), S[i]),
                       blocked if cuboids is not None else None)
    return out[:3] if cuboids is None else out


# ------------------------------------------------------------------------------------------------ the tests
_CACHE = {}


def results(seed):
    if seed not in _CACHE:
        from uav_ac import scoring
        rows, ro, starts = fleet(seed)
        plain, obs = Layers(rows), Layers(rows)
        _CACHE[seed] = dict(
            rows=rows, ro=ro, starts=starts, plain=plain, obs=obs,
            separation=scoring.separation_from_rows(rows, ro, RADIUS, GROUPS, starts),
            stagger=scoring.stagger_from_rows(rows, ro, RADIUS, GROUPS, starts, step=STEP, max_steps=STAGGER_STEPS),
            layer=scoring.layer_from_rows(plain, ro, RADIUS, GROUPS, starts, max_steps=LAYER_STEPS),
            layer_obs=scoring.layer_obstacles_from_rows(obs, ro, RADIUS, [CUBOID], GROUPS, starts, max_steps=LAYER_STEPS))
    return _CACHE[seed]


def same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want, equal_nan=got.dtype.kind == "f")


@pytest.mark.parametrize("seed", SEEDS)
def test_every_specification_equals_its_naive_restatement(seed):
    k = results(seed)
    rows, ro, starts = k["rows"], k["ro"], k["starts"]
    sep, isep = naive_separation(rows, ro, RADIUS, GROUPS, starts)
    assert same(k["separation"][0], sep) and same(k["separation"][1], isep)
    assert same(k["stagger"], naive_stagger(rows, ro, RADIUS, GROUPS, starts, STEP, STAGGER_STEPS))
    assert same(k["layer"], naive_layers(Layers(rows), ro, RADIUS, GROUPS, starts, LAYER_STEPS))
    assert same(k["layer_obs"], naive_layers(Layers(rows), ro, RADIUS, GROUPS, starts, LAYER_STEPS, [CUBOID]))
    # the excluded missions: no rows, a NaN coordinate
    for b in (6, 12):
        assert np.isnan(k["separation"][0][b]) and k["stagger"][1, b] == k["layer"][1, b] == k["layer_obs"][1, b] == -2


@pytest.mark.parametrize("seed", SEEDS)
def test_rows_at_is_asked_lazily(seed):
    """layer 0 first, and never a layer above the highest one a mission examined"""
    k = results(seed)
    for asked, block in ((k["plain"].asked, k["layer"]), (k["obs"].asked, k["layer_obs"])):
        steps = block[1]
        highest = max([0] + [int(s) if s >= 0 else LAYER_STEPS for s in steps if s != -2])
        assert asked[0] == 0 and max(asked) <= highest, (asked[:4], max(asked), highest)


def test_the_fleets_exercise_every_outcome():
    """not vacuous: over the seeds every search leaves somebody unexamined, unresolved, where they were and moved, and a cuboid blocks"""
    for name in ("stagger", "layer", "layer_obs"):
        steps = np.concatenate([results(seed)[name][1] for seed in SEEDS])
        print(name, {c: int((steps == c).sum()) for c in (-2, -1, 0)}, "above 0:", int((steps > 0).sum()))
        assert (steps == -2).any() and (steps == -1).any() and (steps == 0).any() and (steps > 0).any(), name
    blocked = [int((results(seed)["layer_obs"][3] > 0).sum()) for seed in SEEDS]
    print("missions with blocked > 0 per seed:", blocked)
    assert max(blocked) > 0
