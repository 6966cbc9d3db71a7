"""Minimum-snap plans with boundary derivatives, on the CPU: the reference the GPU tests compare with (tests/boundary_ref.py) is
checked against itself -- `np.linalg.solve` against `lstsq`, and the property that makes a handover possible at all: re-solving the
tail of a rest-to-rest mission from an interior knot's own (v, a, j) gives that tail back -- and the two new entry points are
declared, exported and bound."""
import os
import re

import numpy as np
import pytest

import boundary_ref as br
from conftest import REPO, col_err
from oracle import minsnap_oracle as mo

VELOCITY = 3.0


@pytest.mark.parametrize("m", [1, 2, 3, 8, 20])
def test_dense_reference_with_boundary_values_agrees_with_itself(m):
    wps = mo.synthetic_missions(4, m)
    bcs = br.draw_boundaries(4, 7 + m)
    for wp, bc in zip(wps, bcs):
        times = mo.segment_times(wp, VELOCITY)
        solve, lstsq = br.dense_coeffs(wp, times, bc, "solve"), br.dense_coeffs(wp, times, bc, "lstsq")
        assert col_err(lstsq, solve) < 1e-5
        # ... and it is the system that was meant: the curve has the boundary values, and zero of them is the oracle's own solve
        assert np.abs(br.derivatives(solve, 0, 0.0) - bc[:3]).max() < 1e-9
        assert np.abs(br.derivatives(solve, m - 1, times[-1]) - bc[3:]).max() < 1e-9
        rest = mo.solve_coefficients(wp, VELOCITY, "solve")[0]
        assert np.array_equal(br.dense_coeffs(wp, times, np.zeros((6, 3))), rest) and np.array_equal(br.dense_coeffs(wp, times), rest)


@pytest.mark.parametrize("k", [1, 4, 7])
def test_tail_resolved_from_an_interior_knot_is_the_tail(k):
    m = 8
    for wp in mo.synthetic_missions(4, m):
        times = mo.segment_times(wp, VELOCITY)
        full = br.dense_coeffs(wp, times)
        bc = np.concatenate([br.derivatives(full, k, 0.0), np.zeros((3, 3))])
        tail = br.dense_coeffs(wp[k:], times[k:], bc)
        assert col_err(tail, full[8 * k:]) < 1e-9


NEW_SYMBOLS = ("uavac_minsnap_solve_bc_dev", "uavac_minsnap_plan_bc_dev")


def test_the_boundary_entry_points_are_declared_exported_and_prototyped():
    from uav_ac import _native as nat
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "uavac.h")).read(), flags=re.S)
    lib = nat.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in nat.exported_symbols()
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == text.split(name + "(")[1].split(")")[0].count(",") + 1, name
    # nothing runs without a context: the entry points refuse a NULL one before they look at anything else
    assert lib.uavac_minsnap_solve_bc_dev(None, None, None, None, 1, 1, None, None, None) == nat.EINVAL
    assert lib.uavac_minsnap_plan_bc_dev(None, None, 1, 1, None, 0.01, None, None, None, None, None, None, None, 0, None, None) == nat.EINVAL


def test_the_boundary_kernel_is_in_the_register_budget_check_and_free_of_scratch():
    from uav_ac import _buildcheck
    from uav_ac import _native as nat
    nat.lib()
    counts = _buildcheck.check_planning_registers()
    if counts is None:
        pytest.skip("no build directory / LLVM tools: library was built elsewhere")
    private = [(k.name, k.private_segment_fixed_size) for k in _buildcheck.check_budgets("planning_registers") if "minsnap_solve_bc_kernel" in k.name]
    mine = [(n, v, s) for n, v, s in counts if "minsnap_solve_bc_kernel" in n]
    assert len(mine) == 2 and all(v <= 256 and s == 0 for _, v, s in mine), mine          # uniform and ragged
    assert len(private) == 2 and all(p == 0 for _, p in private), private
