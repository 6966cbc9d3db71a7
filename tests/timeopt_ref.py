"""Reference for the optimisation of segment durations  --  TEST INFRASTRUCTURE, a helper module (no fixtures, no tests).

The loop of include/uavac.h (uavac_minsnap_optimize_times_dev) restated in NumPy, one mission at a time, on the reference-form dense
KKT solve (`boundary_ref.dense_coeffs(..., method="solve")`) with the cost as upstream writes it, c^T H c with
`oracle.minsnap_oracle.snap_cost_matrix`.  Shares nothing with csrc/minsnap_timeopt.hip but the constants below, which are part of the
contract.  `gl_cost` restates the device's cost formula (four-point Gauss-Legendre) for the host-side comparison of the two."""
import numpy as np

from boundary_ref import dense_coeffs
from oracle import minsnap_oracle as mo

PROBE_STEP = 1.0e-6
CANDIDATES = 6
ALPHA0 = 0.25
ALPHA_MAX = 0.5
FLOOR = 0.2

GL_X = (-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526)
GL_W = (0.3478548451374538, 0.6521451548625461, 0.6521451548625461, 0.3478548451374538)


def chc_cost(coeffs: np.ndarray, times: np.ndarray) -> float:
    """c^T H c summed over the axes: coeffs (8m, 3), times (m,)."""
    return float(np.einsum("ia,ij,ja->", coeffs, mo.snap_cost_matrix(np.asarray(times, dtype=float)), coeffs))


def gl_cost(coeffs: np.ndarray, times: np.ndarray) -> float:
    """The same integral by the four-point Gauss-Legendre rule on Horner-evaluated snap, in the device's order of operations."""
    c = np.asarray(coeffs, dtype=float).reshape(-1, 8, 3)
    total = 0.0
    for s, T in enumerate(np.asarray(times, dtype=float)):
        half = 0.5 * T
        seg = 0.0
        for x, w in zip(GL_X, GL_W):
            t = half + half * x
            sn = ((840.0 * c[s, 7] * t + 360.0 * c[s, 6]) * t + 120.0 * c[s, 5]) * t + 24.0 * c[s, 4]
            q = sn * sn
            seg = seg + (half * w) * ((q[0] + q[1]) + q[2])
        total = total + seg
    return float(total)


def cost_of(waypoints: np.ndarray, times: np.ndarray, method: str = "solve") -> float:
    return chc_cost(dense_coeffs(waypoints, times, method=method), times)


def optimize_times(waypoints: np.ndarray, times0: np.ndarray, iterations: int, method: str = "solve"):
    """-> (times, history, accepted): the durations after `iterations` iterations, the cost before the first and after every iteration
    (iterations + 1 values), and the number of steps taken."""
    wp = np.asarray(waypoints, dtype=float)
    T0 = np.asarray(times0, dtype=float).copy()
    m = len(T0)
    T = T0.copy()
    J = cost_of(wp, T, method)
    history, accepted, alpha = [J], 0, ALPHA0
    if m < 2 or not np.isfinite(J):
        return T, history + [J] * iterations, 0
    total = 0.0
    for t in T0:
        total = total + t
    floor = FLOOR * T0.min()
    for _ in range(iterations):
        h = PROBE_STEP * total / m
        d = np.empty(m)
        for i in range(m):
            g = np.full(m, -1.0 / (m - 1))
            g[i] = 1.0
            d[i] = (cost_of(wp, T + h * g, method) - J) / h
        G = np.array([d[k] - sum(d[i] for i in range(m) if i != k) / (m - 1) for k in range(m)])
        D = -G
        if not np.all(np.isfinite(d)) or np.max(np.abs(D)) == 0.0:
            history.append(J)
            continue
        D = D * (T.min() / np.max(np.abs(D)))
        best, best_j, best_T = J, -1, None
        for j in range(CANDIDATES):
            a = alpha * 2.0 ** -j
            Tc = T + a * D
            if Tc.min() < floor:
                continue
            s = 0.0
            for t in Tc:
                s = s + t
            Tc = Tc * (total / s)
            Jc = cost_of(wp, Tc, method)
            if Jc < best:
                best, best_j, best_T = Jc, j, Tc
        if best_j >= 0:
            T, J, accepted = best_T, best, accepted + 1
            alpha = min(ALPHA_MAX, 2.0 * alpha * 2.0 ** -best_j)
        else:
            alpha = alpha * 2.0 ** -CANDIDATES
        history.append(J)
    return T, history, accepted
