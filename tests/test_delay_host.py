"""Start delays as a plan transform, the part that needs no GPU: the two entry points are exported and declared as the header declares
them, a NULL context is refused, the build keeps the kernels inside their budgets, and the rule itself -- `uav_ac.scoring.delay_rows`,
the NumPy statement on sampled rows that `Engine.delay` is tested against bit for bit (tests/test_gpu_delay.py) -- gives the rows that
hand-made input has by inspection.  The backbone of the GPU tests is checked here on the oracle's own rows:
`separation_from_rows(delay_rows(rows, S))` equals `separation_from_rows(rows, start_rows=S)` bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO

KINDS = {"int": C.c_int, "double": C.c_double, "int64_t": C.c_int64}


def declared(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "uavac.h")).read(), flags=re.S)
    args = re.search(rf"int\s+{name}\s*\(([^)]*)\)\s*;", text).group(1)
    params = [" ".join(a.split()) for a in args.split(",")]
    return [C.c_void_p if "*" in a else KINDS[a.split()[0]] for a in params], params


def test_entry_points_are_exported_and_declared_like_the_header():
    from uav_ac import _native as nat
    for name, n_args in (("uavac_minsnap_delay_offsets_dev", 6), ("uavac_minsnap_delay_dev", 13)):
        assert name in nat.exported_symbols()
        getattr(nat.lib(), name)
        restype, argtypes = nat._SIGNATURES[name]
        kinds, params = declared(name)
        assert restype is C.c_int and len(argtypes) == n_args and kinds == list(argtypes), params
    # a NULL context is refused before anything else is looked at (pure host code: no GPU needed)
    assert nat.lib().uavac_minsnap_delay_offsets_dev(None, None, 1, 1, None, None) == nat.EINVAL
    assert nat.lib().uavac_minsnap_delay_dev(None, None, None, None, None, 1, 1, 0.01, None, None, None, None, None) == nat.EINVAL


def test_the_build_keeps_the_delay_kernels_in_registers():
    from uav_ac import _buildcheck
    counts = _buildcheck.check_delay_kernels()
    if counts is None:
        pytest.skip("no object files here (a library that was built elsewhere)")
    assert len(counts) == 2 and max(counts.values()) <= 64
    assert any("minsnap_delay_kernel" in k for k in counts) and any("delay_counts_kernel" in k for k in counts)


def hand_made():
    """Two missions of 3 and 2 rows whose row 0 carries a velocity and an acceleration of rounding size, as a solved mission's does."""
    rows = np.zeros((5, 11))
    rows[:, 0:3] = [[1, 2, -3], [1.5, 2, -3], [2, 2, -3], [7, 8, -9], [7, 8.5, -9]]
    rows[:, 3:6] = [[1e-11, -2e-11, 0], [3, 0, 0], [3, 0, 0], [0, 4e-12, 0], [0, 3, 0]]
    rows[:, 6:9] = [[5e-12, 0, 0], [0.5, 0, 0], [0, 0, 0], [0, 1e-12, 0], [0, 0.25, 0]]
    rows[:, 9] = [0.0, 0.0, 0.0, np.pi / 2, np.pi / 2]
    rows[:, 10] = [0, 0, 1, 0, 0]
    return rows, np.array([0, 3, 5]), np.array([0.0, np.pi / 2])


def test_delay_rows_on_hand_made_rows():
    from uav_ac.scoring import delay_rows
    rows, ro, fy = hand_made()
    out, oro = delay_rows(rows, ro, [2, 0], fy)
    assert oro.tolist() == [0, 5, 7] and oro.dtype == np.int64 and out.shape == (7, 11)
    hold = np.array([1, 2, -3, 0, 0, 0, 0, 0, 0, 0.0, 0])
    assert np.array_equal(out[0], hold) and np.array_equal(out[1], hold)
    assert not np.array_equal(out[0], rows[0])               # a hold row is not row 0 repeated: only the position is
    shifted = rows[0:3].copy()
    shifted[:, 10] += 1
    assert np.array_equal(out[2:5], shifted)
    assert np.array_equal(out[5:7], rows[3:5])               # S = 0: copied as it is, spline ids included
    out, oro = delay_rows(rows, ro, [0, 3], fy)
    assert oro.tolist() == [0, 3, 8] and np.array_equal(out[0:3], rows[0:3])
    assert np.array_equal(out[3:6], np.tile([7, 8, -9, 0, 0, 0, 0, 0, 0, np.pi / 2, 0], (3, 1)))
    assert np.array_equal(out[6:8, :10], rows[3:5, :10]) and out[6:8, 10].tolist() == [1, 1]
    assert not np.signbit(out[3:6, 3:9]).any()               # the zeros of a hold row are +0: what 0 * t + 0 gives
    # no delay at all is the identity; a negative start counts as 0
    for S in ([0, 0], [-4, -1]):
        out, oro = delay_rows(rows, ro, S, fy)
        assert np.array_equal(out, rows) and oro.tolist() == ro.tolist()
    with pytest.raises(ValueError):
        delay_rows(rows, ro, [1], fy)
    with pytest.raises(ValueError):                          # a mission without rows has no hold position among the rows
        delay_rows(rows[:3], [0, 3, 3], [0, 1], fy)
    out, oro = delay_rows(rows[:3], [0, 3, 3], [1, 0], fy)   # ... but it may stay as it is
    assert oro.tolist() == [0, 4, 4]


def test_the_audit_of_delayed_rows_equals_the_audit_with_start_rows_on_oracle_missions():
    """The identity the GPU tests rest on, on 24 missions planned and sampled by the oracle: every output, bit for bit."""
    from oracle import c_oracle
    from oracle import minsnap_oracle as mo
    from uav_ac.scoring import delay_rows, separation_from_rows
    ref = c_oracle.plan_threads(mo.synthetic_missions(24, 8), 3.0, 0.01)
    rows, ro = ref["rows"], ref["row_offsets"]
    S = np.random.default_rng(7).choice([0, 1, 63, 64, 65, 300], size=24)
    assert len(set(S.tolist())) == 6
    go = [0, 12, 24]
    drows, dro = delay_rows(rows, ro, S, ref["first_yaw"])
    assert np.array_equal(np.diff(dro), np.diff(ro) + S)
    sep_d, isep_d = separation_from_rows(drows, dro, 0.5, go)
    sep_s, isep_s = separation_from_rows(rows, ro, 0.5, go, start_rows=S)
    assert np.array_equal(sep_d.view(np.int64), sep_s.view(np.int64)) and np.array_equal(isep_d, isep_s)
    _, isep_0 = separation_from_rows(rows, ro, 0.5, go)
    assert not np.array_equal(isep_0, isep_s)                # (the delays matter on this set)
    for b in (0, 11, 23):                                    # the hold rows: position of row 0, at rest, first heading, spline 0
        h = drows[dro[b]:dro[b] + S[b]]
        first = rows[ro[b]]
        assert (h[:, 0:3] == first[0:3]).all() and (h[:, 3:9] == 0).all() and (h[:, 9] == ref["first_yaw"][b]).all() and (h[:, 10] == 0).all()
        own = drows[dro[b] + S[b]:dro[b + 1]]
        assert np.array_equal(own[:, :10], rows[ro[b]:ro[b + 1], :10])
        assert np.array_equal(own[:, 10], rows[ro[b]:ro[b + 1], 10] + (S[b] > 0))
