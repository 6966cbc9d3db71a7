"""Optimised segment durations, host side: the NumPy reference of the loop (tests/timeopt_ref.py) is pinned -- monotone cost, kept
total, the floor, m = 1 untouched, and the cost ratios it reaches on the three mission sets the feature was motivated with -- the
Gauss-Legendre form of the cost agrees with upstream's c^T H c, and the library exports the four entry points include/uavac.h declares."""
import os
import re

import numpy as np
import pytest

from conftest import REPO

import timeopt_ref as tr
from boundary_ref import dense_coeffs
from oracle import minsnap_oracle as mo

NEW_ENTRY_POINTS = ("uavac_minsnap_row_counts_t_dev", "uavac_minsnap_plan_t_dev", "uavac_minsnap_cost_dev",
                    "uavac_minsnap_optimize_times_dev")

# synthetic_missions arguments -> cost_after / cost_before (min, median, max) of the reference after 6 iterations at 3 m/s, as this
# reference gave them when it was written (NumPy 'solve' on the dense KKT system); asserted to 1e-6 relative: LAPACK builds differ in
# the last bits of a solve, the perturbation study behind the GPU test's bars (lstsq for solve) moved final costs by <= 2.9e-7
PINNED = {
    (12, 3): (0.551092222760449, 0.9263802313493423, 0.96695277275651),
    (12, 8): (0.3159616214228854, 0.8164830535908334, 0.9194152443062145),
    (12, 8, 1.0, 6.0): (0.01881489128592128, 0.46967781759969773, 0.7717137048321322),
}


@pytest.fixture(scope="module", params=list(PINNED), ids=lambda a: "x".join(str(v) for v in a))
def optimised(request):
    wps = mo.synthetic_missions(*request.param)
    runs = []
    for wp in wps:
        T0 = mo.segment_times(wp, 3.0)
        runs.append((T0,) + tr.optimize_times(wp, T0, 6))
    return request.param, runs


def test_reference_descends_and_keeps_its_invariants(optimised):
    _, runs = optimised
    for T0, T, history, accepted in runs:
        assert len(history) == 7
        assert all(b <= a for a, b in zip(history, history[1:])), history
        assert abs(T.sum() - T0.sum()) <= 1e-12 * T0.sum()
        assert T.min() >= tr.FLOOR * T0.min()
        assert 0 <= accepted <= 6
        assert (accepted == 0) == bool(np.array_equal(T, T0))


def test_reference_reaches_the_pinned_cost_ratios(optimised):
    args, runs = optimised
    r = np.array([history[-1] / history[0] for _, _, history, _ in runs])
    got = (r.min(), np.median(r), r.max())
    print(args, got)
    for g, want in zip(got, PINNED[args]):
        assert abs(g - want) <= 1e-6 * want, (args, got, PINNED[args])


def test_reference_leaves_a_single_segment_alone():
    wp = mo.synthetic_missions(3, 1)[1]
    T0 = mo.segment_times(wp, 3.0)
    T, history, accepted = tr.optimize_times(wp, T0, 4)
    assert np.array_equal(T, T0) and accepted == 0 and history == [history[0]] * 5


@pytest.mark.parametrize("m", [1, 2, 8, 12, 20])
def test_gauss_legendre_cost_is_the_snap_cost(m):
    """Four nodes integrate the degree-6 integrand exactly: the two formulas differ by rounding alone.  Measured: <= 4.7e-13 at m = 1,
    <= 5.5e-14 from m = 2 on -- all of it c^T H c's own cancellation (against exact rational arithmetic the quadrature is within 3e-15)."""
    worst = 0.0
    for wp in mo.synthetic_missions(12, m):
        T = mo.segment_times(wp, 3.0)
        c = dense_coeffs(wp, T)
        a, b = tr.gl_cost(c, T), tr.chc_cost(c, T)
        worst = max(worst, abs(a - b) / b)
    print(m, worst)
    assert worst <= 1e-12


def test_header_declares_and_library_exports_the_entry_points():
    from uav_ac import _native as nat
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "uavac.h")).read(), flags=re.S)
    lib = nat.lib()
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in nat.exported_symbols()
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == text.split(name + "(")[1].split(")")[0].count(",") + 1, name
    # nothing runs without a context: the entry points refuse a NULL one before they look at anything else
    assert lib.uavac_minsnap_row_counts_t_dev(None, None, None, 1, 1, 0.01, None, None) == nat.EINVAL
    assert lib.uavac_minsnap_plan_t_dev(None, None, None, 1, 1, None, 0.01, None, None, None, None, None, 0, None, None) == nat.EINVAL
    assert lib.uavac_minsnap_cost_dev(None, None, None, None, 1, 1, None) == nat.EINVAL
    assert lib.uavac_minsnap_optimize_times_dev(None, None, None, 1, 1, None, 1, None, None, None) == nat.EINVAL
    # the loop's constants are part of the contract: the header names them, the reference uses the same values
    full = open(os.path.join(REPO, "include", "uavac.h")).read()
    for macro, value in (("UAVAC_TIMEOPT_PROBE_STEP", tr.PROBE_STEP), ("UAVAC_TIMEOPT_CANDIDATES", tr.CANDIDATES),
                         ("UAVAC_TIMEOPT_ALPHA0", tr.ALPHA0), ("UAVAC_TIMEOPT_ALPHA_MAX", tr.ALPHA_MAX), ("UAVAC_TIMEOPT_FLOOR", tr.FLOOR)):
        found = re.search(r"#define\s+" + macro + r"\s+(\S+)", full)
        assert found and float(found.group(1)) == value, macro


def test_build_checks_cover_the_new_kernels():
    from uav_ac import _buildcheck
    from uav_ac import _native as nat
    nat.lib()
    counts = _buildcheck.check_timeopt_kernels()
    if counts is None:
        pytest.skip("no object files here (a library that was built elsewhere)")
    assert len(counts) == len(_buildcheck.TIMEOPT_KERNELS) + 1 and max(counts.values()) <= 128
