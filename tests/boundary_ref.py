"""Reference for minimum-snap plans with boundary derivatives  --  TEST INFRASTRUCTURE, a helper module (no fixtures, no tests).

The reference-form dense solve: the (14m+2)^2 KKT system of `oracle.minsnap_oracle` (`constraint_system`, `snap_cost_matrix`; monomial
basis, ascending powers) with the six rows that pin velocity, acceleration and jerk at the first and last waypoint given VALUES
instead of zeros: b[2m : 2m+3] = (v, a, j) at the start, b[2m+3 : 2m+6] = (v, a, j) at the goal.  Shares nothing with the reduced
knot-derivative form of csrc/minsnap_kkt.h."""
import numpy as np

from oracle import minsnap_oracle as mo

# the ranges the boundary values of the tests are drawn from: velocity [m/s], acceleration [m/s^2], jerk [m/s^3]
BC_RANGES = (3.0, 4.0, 8.0)


def draw_boundaries(B: int, seed: int) -> np.ndarray:
    """(B, 6, 3): rows 0-2 = (v, a, j) at the first waypoint, rows 3-5 at the last one, U(-3, 3), U(-4, 4), U(-8, 8)."""
    rng = np.random.default_rng(seed)
    r = np.array(BC_RANGES + BC_RANGES)[None, :, None]
    return rng.uniform(-1.0, 1.0, (B, 6, 3)) * r


def dense_coeffs(waypoints: np.ndarray, times: np.ndarray, bc: np.ndarray = None, method: str = "solve") -> np.ndarray:
    """Coefficients (8m, 3) of one mission from the dense KKT system; bc (6, 3) or None (rest to rest); method "solve" | "lstsq"."""
    wp = np.asarray(waypoints, dtype=float)
    times = np.asarray(times, dtype=float)
    m = wp.shape[0] - 1
    A, b = mo.constraint_system(wp, times)
    if bc is not None:
        b[2 * m:2 * m + 6] = np.asarray(bc, dtype=float).reshape(6, 3)
    H = mo.snap_cost_matrix(times)
    nc = A.shape[0]
    kkt = np.block([[H, A.T], [A, np.zeros((nc, nc))]])
    rhs = np.vstack((np.zeros((H.shape[0], b.shape[1])), b))
    sol = np.linalg.lstsq(kkt, rhs, rcond=None)[0] if method == "lstsq" else np.linalg.solve(kkt, rhs)
    return sol[:H.shape[0]]


def derivatives(coeffs: np.ndarray, segment: int, t: float) -> np.ndarray:
    """(3, 3): velocity, acceleration, jerk of segment `segment` of coeffs (8m, 3) at local time t."""
    c = np.asarray(coeffs, dtype=float).reshape(-1, 8, 3)[segment]
    return np.stack([mo.basis_row(k, t) @ c for k in (1, 2, 3)])
