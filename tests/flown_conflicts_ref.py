"""What the two test files of the flown conflict list share (no test in here): the seeded synthetic logs of
tests/test_gpu_flown_separation.py -- the same recipe, the same seeds, hence the same logs --, what the rule gives on them, computed once
per K and left unchanged, and the figures that say the sets are not trivial."""
import numpy as np

B, SIZES = 193, (63, 64, 65, 1)
GO = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
RADIUS = 0.5
NAN_SOMETIMES, NAN_ALWAYS = 70, 130
TILE = 64
PARTNER, FIRST, LAST, INSIDE, MIN_TICK = range(5)

_LOGS = {}


def synthetic(K):
    """(the log (K, 13, B) on the host, `conflicts_from_log` on it in the groups GO, `separation_from_log` on it): positions on the
    0.125 grid inside a 3 m box, vehicle 70 NaN in x every third tick, vehicle 130 NaN throughout; the other ten rows hold junk that
    must never be read."""
    if K not in _LOGS:
        from uav_ac.scoring import conflicts_from_log, separation_from_log
        rng = np.random.default_rng(100 + K)
        log = rng.uniform(-1e3, 1e3, (K, 13, B))
        log[:, 0:3, :] = rng.integers(0, 25, (K, 3, B)) * 0.125
        log[::3, 0, NAN_SOMETIMES] = np.nan                  # (with K = 1 that is its only tick)
        log[:, 0:3, NAN_ALWAYS] = np.nan
        _LOGS[K] = (log, conflicts_from_log(log, RADIUS, GO), separation_from_log(log, RADIUS, GO))
    return _LOGS[K]


def figures(log, want, group=2):
    """(entries, most per vehicle, entries with a gap, entries whose minimum is tied between ticks, vehicles of group `group` -- the one
    of 65 -- with partners in both of its j-tiles) of a list on its log"""
    off, d, i = want
    owner = np.repeat(np.arange(len(off) - 1), np.diff(off))
    tied = 0
    for e in range(len(owner)):
        diff = log[:, 0:3, owner[e]] - log[:, 0:3, i[PARTNER, e]]
        d2 = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
        tied += int((d2 == np.nanmin(d2)).sum() > 1)
    g0, g1 = int(GO[group]), int(GO[group + 1])
    both = sum(bool((i[PARTNER, off[b]:off[b + 1]] < g0 + TILE).any() and (i[PARTNER, off[b]:off[b + 1]] >= g0 + TILE).any())
               for b in range(g0, g1))
    return int(off[-1]), int(np.diff(off).max()), int((i[INSIDE] < i[LAST] - i[FIRST] + 1).sum()), tied, both


# what the rule gives with these seeds: the sets cannot silently go trivial
FIGURES = {1: (156,), 33: (4282, 32, 738, 70, 29), 100: (8874, 57, 4514, 534, 49)}
