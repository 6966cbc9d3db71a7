/*
 * uavac_oracle.c -- scalar C restatement of the reference hot path.
 * TEST INFRASTRUCTURE, NOT PRODUCT: only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg may load it (through oracle/c_oracle.py).  libuavac.so never links it.
 *
 * One UAV / one mission at a time, in the reference's own formulation (upstream paths):
 *   planner   uav_ac/planning/minimum_snap.py: times :311-321, A/b :171-255 + :293-309,
 *             H :155-169, KKT solve with method="solve" (np.linalg.solve = LU with partial
 *             pivoting) :138-153, sampler :100-119, polynom :257-286, yaw scan :126-136
 *   control   uav_ac/control/controller.py:26-191, uav_ac/quadrotor/quad.py:88-155,189-213,
 *             uav_ac/main.py:37-61
 *   dynamics  rotor wrench uav_ac/simulation/mujoco_sim.py:232-251 + MuJoCo Euler free-joint step
 *             (parity vs MuJoCo itself is UNPINNED, see control_oracle.py)
 *
 * Pinned by tests/test_oracle_c.py against the golden vectors produced by importing the
 * reference (tests/golden/make_golden.py).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define NC 8
#define PI 3.14159265358979323846

/* ------------------------------------------------------------------------------- planner */
static void polynom(int order, double t, double *row) { /* minimum_snap.py:257-286 */
    for (int i = 0; i < NC; ++i) {
        double poly = 1.0, der = (double)i;
        for (int k = 0; k < order; ++k) {
            poly *= der;
            if (der > 0) der -= 1.0;
        }
        row[i] = poly * pow(t, der);
    }
}

void oracle_times(const double *wp, int m, double velocity, double *times) { /* :311-321 */
    for (int i = 0; i < m; ++i) {
        double dx = wp[3 * (i + 1)] - wp[3 * i], dy = wp[3 * (i + 1) + 1] - wp[3 * i + 1],
               dz = wp[3 * (i + 1) + 2] - wp[3 * i + 2];
        /* np.linalg.norm of a 3-vector = sqrt(x.dot(x)); BLAS ddot accumulates with fused multiply-adds (see
         * rrt_oracle.c).  Only this form reproduces the committed reference times bit for bit. */
        double t = sqrt(fma(dz, dz, fma(dy, dy, dx * dx))) / velocity;
        if (i == 0 || i == m - 1) t *= 1.5;
        times[i] = t;
    }
}

/* dense LU with partial pivoting, nrhs right-hand sides, in place; returns 0 or -1 if singular */
static int lu_solve(double *A, double *b, int n, int nrhs) {
    for (int k = 0; k < n; ++k) {
        int p = k;
        double best = fabs(A[k * n + k]);
        for (int i = k + 1; i < n; ++i)
            if (fabs(A[i * n + k]) > best) { best = fabs(A[i * n + k]); p = i; }
        if (!(best > 0.0)) return -1;
        if (p != k) {
            for (int j = 0; j < n; ++j) { double t = A[k * n + j]; A[k * n + j] = A[p * n + j]; A[p * n + j] = t; }
            for (int j = 0; j < nrhs; ++j) { double t = b[k * nrhs + j]; b[k * nrhs + j] = b[p * nrhs + j]; b[p * nrhs + j] = t; }
        }
        for (int i = k + 1; i < n; ++i) {
            double l = A[i * n + k] / A[k * n + k];
            if (l == 0.0) continue;
            for (int j = k + 1; j < n; ++j) A[i * n + j] -= l * A[k * n + j];
            for (int j = 0; j < nrhs; ++j) b[i * nrhs + j] -= l * b[k * nrhs + j];
        }
    }
    for (int i = n - 1; i >= 0; --i)
        for (int j = 0; j < nrhs; ++j) {
            double s = b[i * nrhs + j];
            for (int c = i + 1; c < n; ++c) s -= A[i * n + c] * b[c * nrhs + j];
            b[i * nrhs + j] = s / A[i * n + i];
        }
    return 0;
}

/* coeffs [8m][3]; returns 0 ok, -1 singular, -2 out of memory */
int oracle_solve(const double *wp, int m, double velocity, double *coeffs, double *times) {
    oracle_times(wp, m, velocity, times);
    int nu = NC * m, ncon = 6 * m + 2, n = nu + ncon;
    double *K = (double *)calloc((size_t)n * n, sizeof(double));
    double *rhs = (double *)calloc((size_t)n * 3, sizeof(double));
    if (!K || !rhs) { free(K); free(rhs); return -2; }
    double row[NC], row0[NC];
    int r = 0;
    /* A occupies K[nu + r][c] and its transpose K[c][nu + r] */
#define SETA(rr, cc, v) do { K[(size_t)(nu + (rr)) * n + (cc)] = (v); K[(size_t)(cc) * n + nu + (rr)] = (v); } while (0)
    polynom(0, 0.0, row0);                                      /* positions at t = 0  (:240-245) */
    for (int s = 0; s < m; ++s, ++r) {
        for (int i = 0; i < NC; ++i) SETA(r, s * NC + i, row0[i]);
        for (int j = 0; j < 3; ++j) rhs[(size_t)(nu + r) * 3 + j] = wp[3 * s + j];
    }
    for (int s = 0; s < m; ++s, ++r) {                          /* positions at t = T  (:248-255) */
        polynom(0, times[s], row);
        for (int i = 0; i < NC; ++i) SETA(r, s * NC + i, row[i]);
        for (int j = 0; j < 3; ++j) rhs[(size_t)(nu + r) * 3 + j] = wp[3 * (s + 1) + j];
    }
    for (int k = 1; k <= 3; ++k, ++r) {                         /* start at rest (:214-217) */
        polynom(k, 0.0, row);
        for (int i = 0; i < NC; ++i) SETA(r, i, row[i]);
    }
    for (int k = 1; k <= 3; ++k, ++r) {                         /* goal at rest (:220-223) */
        polynom(k, times[m - 1], row);
        for (int i = 0; i < NC; ++i) SETA(r, (m - 1) * NC + i, row[i]);
    }
    for (int s = 1; s < m; ++s)                                 /* continuity k = 1..4 (:191-198) */
        for (int k = 1; k <= 4; ++k, ++r) {
            polynom(k, times[s - 1], row);
            polynom(k, 0.0, row0);
            for (int i = 0; i < NC; ++i) { SETA(r, (s - 1) * NC + i, row[i]); SETA(r, s * NC + i, -row0[i]); }
        }
    for (int s = 0; s < m; ++s)                                 /* snap cost (:155-169) */
        for (int a = 4; a < NC; ++a)
            for (int c = 4; c < NC; ++c) {
                double fa = a * (a - 1) * (a - 2) * (a - 3), fc = c * (c - 1) * (c - 2) * (c - 3);
                int e = a + c - 7;
                K[(size_t)(s * NC + a) * n + s * NC + c] = fa * fc * pow(times[s], e) / e;
            }
    int rc = lu_solve(K, rhs, n, 3);
    if (rc == 0) memcpy(coeffs, rhs, sizeof(double) * nu * 3);
    free(K); free(rhs);
    return rc;
}

int64_t oracle_row_count(const double *times, int m, double dt) { /* len(np.arange(0, T, dt)) */
    int64_t n = 0;
    for (int s = 0; s < m; ++s) { double q = ceil(times[s] / dt); if (q > 0) n += (int64_t)q; }
    return n;
}

static double floored_mod(double a, double b) { /* Python / NumPy float % for b > 0 */
    double r = fmod(a, b);
    if (r != 0.0 && r < 0.0) r += b;
    return r;
}

/* traj [nrows][11]; returns rows written */
int64_t oracle_sample(const double *coeffs, const double *times, int m, double dt, double *traj) {
    int64_t n = 0;
    double row[NC];
    for (int s = 0; s < m; ++s) {                               /* :100-119 */
        int64_t cnt = (int64_t)ceil(times[s] / dt);
        for (int64_t k = 0; k < cnt; ++k, ++n) {
            double t = (double)k * dt;
            double *o = traj + n * 11;
            for (int ord = 0; ord < 3; ++ord) {
                polynom(ord, t, row);
                for (int j = 0; j < 3; ++j) {
                    double acc = 0.0;
                    for (int i = 0; i < NC; ++i) acc += row[i] * coeffs[(size_t)(s * NC + i) * 3 + j];
                    o[3 * ord + j] = acc;
                }
            }
            o[10] = (double)s;
        }
    }
    /* yaw scan (:126-136): unwrap over the valid subset, hold, back-fill */
    int have = 0;
    double prev_raw = 0.0, cum = 0.0, last = 0.0;
    int64_t first = -1;
    for (int64_t i = 0; i < n; ++i) {
        double vx = traj[i * 11 + 3], vy = traj[i * 11 + 4];
        if (sqrt(vx * vx + vy * vy) >= 1e-3) {
            double a = atan2(vy, vx);
            if (have) {
                double dd = a - prev_raw;
                double ddmod = floored_mod(dd + PI, 2 * PI) - PI;
                if (ddmod == -PI && dd > 0) ddmod = PI;
                double corr = ddmod - dd;
                if (fabs(dd) < PI) corr = 0.0;
                cum += corr;
            } else { first = i; }
            have = 1;
            prev_raw = a;
            last = a + cum;
        }
        traj[i * 11 + 9] = have ? last : 0.0;
    }
    if (first > 0) for (int64_t i = 0; i < first; ++i) traj[i * 11 + 9] = traj[first * 11 + 9];
    return n;
}

/* ------------------------------------------------------------------------------- control */
typedef struct {
    double g, dt, dt_outer, mass, I[3], arm, kf, kappa, min_thrust, max_thrust, tau_rise, tau_fall;
    double max_ascent, max_descent, max_speed_xy, max_horiz_accel, max_tilt;
    double kp_xy, kd_xy, kp_z, kd_z, ki_z, kp_roll, kp_pitch, kp_yaw, kp_p, kp_q, kp_r;
    int32_t F, ground;
    double ground_z, ground_clearance, ground_timeconst;
} oracle_vehicle;   /* same field order as uavac_vehicle so tests can share one ctypes struct */

static double clipd(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

static void quat_to_rot(const double *q, double R[3][3]) { /* quad.py:133-155 */
    double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    double a = q[0] / n, b = q[1] / n, c = q[2] / n, d = q[3] / n;
    double S[3][3] = {{0, -d, c}, {d, 0, -b}, {-c, b, 0}};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double ss = 0.0;
            for (int k = 0; k < 3; ++k) ss += S[i][k] * S[k][j];
            R[i][j] = (i == j ? 1.0 : 0.0) + 2.0 * ss + 2.0 * a * S[i][j];
        }
}

typedef struct {
    double X[13], omega[4], omega_cmd[4], integ, thrust, pqr[3];
    int32_t idx, inner, collided, gbits;
} uav_t;

static void controller_tick(const oracle_vehicle *V, uav_t *u, const double *traj, int64_t nrows) {
    if (u->inner % V->F == 0 && nrows > 0) {                    /* main.py:47-61 */
        const double *tg = traj + (int64_t)u->idx * 11;
        double R[3][3];
        quat_to_rot(u->X + 3, R);
        /* altitude, controller.py:26-56 */
        double zd = clipd(tg[5], -V->max_ascent, V->max_descent);
        double e = tg[2] - u->X[2], ed = zd - u->X[9];
        u->integ = clipd(u->integ + e * V->dt_outer, -10.0, 10.0);
        double acc = V->kp_z * e + V->ki_z * u->integ + V->kd_z * ed + tg[8] - V->g;
        acc = acc / R[2][2];
        double c = clipd(-V->mass * acc, 4 * V->min_thrust, 4 * V->max_thrust);
        u->thrust = c;
        /* lateral, controller.py:58-97 */
        double vdx = tg[3], vdy = tg[4];
        double vm = sqrt(vdx * vdx + vdy * vdy);
        if (vm > V->max_speed_xy) { vdx = vdx / vm * V->max_speed_xy; vdy = vdy / vm * V->max_speed_xy; }
        double ax = V->kp_xy * (tg[0] - u->X[0]) + V->kd_xy * (vdx - u->X[7]) + tg[6];
        double ay = V->kp_xy * (tg[1] - u->X[1]) + V->kd_xy * (vdy - u->X[8]) + tg[7];
        double am = sqrt(ax * ax + ay * ay);
        if (am > V->max_horiz_accel) { ax = ax / am * V->max_horiz_accel; ay = ay / am * V->max_horiz_accel; }
        double az = -c / V->mass;
        double bx = clipd(ax / az, -V->max_tilt, V->max_tilt), by = clipd(ay / az, -V->max_tilt, V->max_tilt);
        /* roll / pitch, controller.py:132-154 */
        double bdx = V->kp_roll * (bx - R[0][2]), bdy = V->kp_pitch * (by - R[1][2]);
        double pc = (R[1][0] / R[2][2]) * bdx + (-R[0][0] / R[2][2]) * bdy;
        double qc = (R[1][1] / R[2][2]) * bdx + (-R[0][1] / R[2][2]) * bdy;
        /* yaw, controller.py:156-168 with quad.py:189-213 on the stored quaternion */
        const double *q = u->X + 3;
        double phi = atan2(2 * (q[0] * q[1] + q[2] * q[3]), 1 - 2 * (q[1] * q[1] + q[2] * q[2]));
        double theta = asin(clipd(2 * (q[0] * q[2] - q[3] * q[1]), -1.0, 1.0));
        double psi = atan2(2 * (q[0] * q[3] + q[1] * q[2]), 1 - 2 * (q[2] * q[2] + q[3] * q[3]));
        double pd = floored_mod(tg[9], 2 * PI);
        double ye = floored_mod(pd - psi + PI, 2 * PI) - PI;
        double rc = (V->kp_yaw * ye * cos(theta) - qc * sin(phi)) / cos(phi);
        u->pqr[0] = pc; u->pqr[1] = qc; u->pqr[2] = rc;
        u->idx = (u->idx + 1 < nrows - 1) ? u->idx + 1 : (int32_t)(nrows - 1);
    }
    /* body rates, controller.py:115-130 */
    const double *w = u->X + 10;
    double kp[3] = {V->kp_p, V->kp_q, V->kp_r}, Iw[3], M[3];
    for (int i = 0; i < 3; ++i) Iw[i] = V->I[i] * w[i];
    M[0] = V->I[0] * kp[0] * (u->pqr[0] - w[0]) + (w[1] * Iw[2] - w[2] * Iw[1]);
    M[1] = V->I[1] * kp[1] * (u->pqr[1] - w[1]) + (w[2] * Iw[0] - w[0] * Iw[2]);
    M[2] = V->I[2] * kp[2] * (u->pqr[2] - w[2]) + (w[0] * Iw[1] - w[1] * Iw[0]);
    /* allocation, quad.py:105-122 */
    double cbar = clipd(u->thrust, 4 * V->min_thrust, 4 * V->max_thrust);
    double pb = M[0] / V->arm, qb = M[1] / V->arm, rb = -M[2] / V->kappa;
    double mf[4] = {(pb + qb + rb) / 4, (-pb + qb - rb) / 4, (-pb - qb + rb) / 4, (pb - qb - rb) / 4};
    double col = cbar / 4, lim = 1e300;
    for (int i = 0; i < 4; ++i) {
        double l = 1.0;
        if (mf[i] > 0) l = (V->max_thrust - col) / mf[i];
        else if (mf[i] < 0) l = (V->min_thrust - col) / mf[i];
        if (l < lim) lim = l;
    }
    double sc = clipd(lim, 0.0, 1.0);
    for (int i = 0; i < 4; ++i) {                               /* quad.py:88-103 */
        double f = clipd(col + sc * mf[i], V->min_thrust, V->max_thrust);
        u->omega_cmd[i] = sqrt(f / V->kf);
        double tau = u->omega_cmd[i] > u->omega[i] ? V->tau_rise : V->tau_fall;
        u->omega[i] += (1 - exp(-V->dt / tau)) * (u->omega_cmd[i] - u->omega[i]);
    }
    u->inner += 1;
}

static void dynamics_step(const oracle_vehicle *V, uav_t *u) {
    double f[4], dt = V->dt;
    for (int i = 0; i < 4; ++i) f[i] = V->kf * u->omega[i] * u->omega[i];
    double T = f[0] + f[1] + f[2] + f[3];
    double tau[3] = {V->arm * (f[0] + f[3] - f[1] - f[2]), V->arm * (f[0] + f[1] - f[2] - f[3]),
                     V->kappa * (-f[0] + f[1] - f[2] + f[3])};
    double R[3][3];
    quat_to_rot(u->X + 3, R);
    double *w = u->X + 10, Iw[3];
    for (int i = 0; i < 3; ++i) Iw[i] = V->I[i] * w[i];
    double cr[3] = {w[1] * Iw[2] - w[2] * Iw[1], w[2] * Iw[0] - w[0] * Iw[2], w[0] * Iw[1] - w[1] * Iw[0]};
    double acc[3] = {-(T / V->mass) * R[0][2], -(T / V->mass) * R[1][2], V->g - (T / V->mass) * R[2][2]};
    double wn2 = 0.0;
    /* BUILD-DEFINED ground contact (MuJoCo's soft-constraint solver cannot run here): while the body's
     * lowest point is below the plane, the vertical velocity update may not exceed the critically damped reference
     * vz + dt (-b vz - k r), b = 2/tc, k = 1/tc^2; the plane only pushes; no friction, no contact torque. */
    double vz_ref = 0.0;
    int touching = 0;
    if (V->ground) {
        double r = u->X[2] - (V->ground_z - V->ground_clearance), tc = V->ground_timeconst;
        if (r > 0.0) { touching = 1; vz_ref = u->X[9] + dt * -(2.0 / tc * u->X[9] + r / (tc * tc)); }
    }
    for (int i = 0; i < 3; ++i) {
        u->X[7 + i] += dt * acc[i];
        if (i == 2 && touching && vz_ref < u->X[9]) u->X[9] = vz_ref;
        w[i] += dt * ((tau[i] - cr[i]) / V->I[i]);
        u->X[i] += dt * u->X[7 + i];
        wn2 += w[i] * w[i];
    }
    double *q = u->X + 3, nq[4] = {q[0], q[1], q[2], q[3]};
    double wn = sqrt(wn2);
    if (wn > 0.0) {
        double h = 0.5 * wn * dt, s = sin(h) / wn, d0 = cos(h), d1 = s * w[0], d2 = s * w[1], d3 = s * w[2];
        nq[0] = q[0] * d0 - q[1] * d1 - q[2] * d2 - q[3] * d3;
        nq[1] = q[0] * d1 + q[1] * d0 + q[2] * d3 - q[3] * d2;
        nq[2] = q[0] * d2 - q[1] * d3 + q[2] * d0 + q[3] * d1;
        nq[3] = q[0] * d3 + q[1] * d2 - q[2] * d1 + q[3] * d0;
    }
    double nn = sqrt(nq[0] * nq[0] + nq[1] * nq[1] + nq[2] * nq[2] + nq[3] * nq[3]);
    for (int i = 0; i < 4; ++i) q[i] = nq[i] / nn;
    if (V->ground) {                                  /* MujocoSimulation._record_collisions, mujoco_sim.py:220-230 */
        if (V->ground_z - u->X[2] >= 0.1) u->gbits |= 2;                           /* TAKEOFF_HEIGHT reached (sticky) */
        int now = u->X[2] - (V->ground_z - V->ground_clearance) > 0.0;
        u->gbits = now ? (u->gbits | 1) : (u->gbits & ~1);
        if (now && (u->gbits & 2)) u->gbits |= 4;                                  /* contact after take-off (sticky) */
    }
}

/* state [26] / istate [4] in the row order of include/uavac.h; logs [K][13] and [K][12] (or NULL) */
void oracle_rollout(const oracle_vehicle *V, const double *traj, int64_t nrows, double *state, int32_t *istate,
                    int K, double *state_log, double *cmd_log, const double *aabbs, int n_obs) {
    uav_t u;
    memcpy(u.X, state, 13 * sizeof(double));
    memcpy(u.omega, state + 13, 4 * sizeof(double));
    memcpy(u.omega_cmd, state + 17, 4 * sizeof(double));
    u.integ = state[21]; u.thrust = state[22];
    memcpy(u.pqr, state + 23, 3 * sizeof(double));
    u.idx = istate[0]; u.inner = istate[1]; u.collided = istate[2]; u.gbits = istate[3];
    for (int k = 0; k < K; ++k) {
        controller_tick(V, &u, traj, nrows);
        if (cmd_log) {
            double *c = cmd_log + (size_t)k * 12;
            c[0] = u.thrust; memcpy(c + 1, u.pqr, 24); memcpy(c + 4, u.omega_cmd, 32); memcpy(c + 8, u.omega, 32);
        }
        dynamics_step(V, &u);
        for (int o = 0; o < n_obs; ++o) {
            const double *c = aabbs + 6 * o;
            if (u.X[0] >= c[0] && u.X[0] <= c[1] && u.X[1] >= c[2] && u.X[1] <= c[3] && u.X[2] >= c[4] && u.X[2] <= c[5])
                u.collided = 1;
        }
        if (state_log) memcpy(state_log + (size_t)k * 13, u.X, 13 * sizeof(double));
    }
    memcpy(state, u.X, 13 * sizeof(double));
    memcpy(state + 13, u.omega, 4 * sizeof(double));
    memcpy(state + 17, u.omega_cmd, 4 * sizeof(double));
    state[21] = u.integ; state[22] = u.thrust;
    memcpy(state + 23, u.pqr, 3 * sizeof(double));
    istate[0] = u.idx; istate[1] = u.inner; istate[2] = u.collided; istate[3] = u.gbits;
}

/* ------------------------------------------------------------------ all-core timing leg (bench.py cpu_baseline)
 * n_threads POSIX threads, each planning and flying whole missions (mission i of wps[n][m+1][3], i = tid,
 * tid + n_threads, ... recycled) with its own buffers until budget_s of wall time has passed.  Returns the
 * missions completed by all threads; *elapsed_s = wall time from start to the last thread's end. */
#include <pthread.h>
#include <time.h>

typedef struct {
    const oracle_vehicle *V;
    const double *wps;
    int n, m, ticks, tid, n_threads;
    double velocity, dt, t_end;
    int64_t done;
} bench_arg;

static double now_s(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static void *bench_worker(void *p) {
    bench_arg *a = (bench_arg *)p;
    const int m = a->m;
    double *coeffs = (double *)malloc(sizeof(double) * 24 * (size_t)m);
    double *times = (double *)malloc(sizeof(double) * (size_t)m);
    double *slog = (double *)malloc(sizeof(double) * 13 * (size_t)a->ticks);
    double *traj = NULL;
    int64_t cap = 0;
    for (int64_t i = a->tid; now_s() < a->t_end; i += a->n_threads) {
        const double *wp = a->wps + (size_t)(i % a->n) * (size_t)(m + 1) * 3;
        if (oracle_solve(wp, m, a->velocity, coeffs, times) != 0) break;
        const int64_t rows = oracle_row_count(times, m, a->dt);
        if (rows > cap) { free(traj); cap = rows + rows / 4; traj = (double *)malloc(sizeof(double) * 11 * (size_t)cap); }
        oracle_sample(coeffs, times, m, a->dt, traj);
        double state[26] = {0};
        int32_t istate[4] = {0, 0, 0, 0};
        state[0] = traj[0]; state[1] = traj[1]; state[2] = traj[2]; state[3] = 1.0;
        const double hover = sqrt(a->V->mass * a->V->g / (4.0 * a->V->kf));
        for (int r = 13; r < 21; ++r) state[r] = hover;
        oracle_rollout(a->V, traj, rows, state, istate, a->ticks, slog, NULL, NULL, 0);
        ++a->done;
    }
    free(coeffs); free(times); free(slog); free(traj);
    return NULL;
}

int64_t oracle_bench_threads(const oracle_vehicle *V, const double *wps, int n, int m, double velocity, double dt,
                             int ticks, int n_threads, double budget_s, double *elapsed_s) {
    pthread_t *th = (pthread_t *)malloc(sizeof(pthread_t) * (size_t)n_threads);
    bench_arg *args = (bench_arg *)malloc(sizeof(bench_arg) * (size_t)n_threads);
    const double t0 = now_s();
    for (int t = 0; t < n_threads; ++t) {
        bench_arg a = {V, wps, n, m, ticks, t, n_threads, velocity, dt, t0 + budget_s, 0};
        args[t] = a;
        pthread_create(&th[t], NULL, bench_worker, &args[t]);
    }
    int64_t done = 0;
    for (int t = 0; t < n_threads; ++t) { pthread_join(th[t], NULL); done += args[t].done; }
    *elapsed_s = now_s() - t0;
    free(th); free(args);
    return done;
}

/* ------------------------------------------------------------------ whole-batch reference (tests only)
 * B missions wps[B][m+1][3], each planned by oracle_solve / oracle_sample (never from a GPU plan) and flown K ticks by
 * oracle_rollout from hover at its first waypoint, on n_threads POSIX threads (lanes handed out 64 at a time).  Outputs
 * (every one may be NULL): out_state [B][26], out_istate [B][4], out_seg_rows [B][m], out_coeffs [B][8m][3], out_first_yaw [B]
 * (the yaw of the mission's first row), out_sel_log [n_sel][13][B] = the state after tick sel_ticks[i] in the GPU's log layout,
 * out_sel_cmd [n_sel][12][B] the same for the command log, out_lane_log [n_ll][K][13] = every tick of lane log_lanes[j].
 * Per-thread buffers only, freed on return.  Returns 0, -1 when a mission's system is singular, -2 when out of memory, -3 on
 * bad arguments. */
typedef struct {
    const oracle_vehicle *V;
    const double *wps, *aabbs;
    int B, m, K, n_obs, n_sel;
    double velocity, dt;
    const int *tick_sel;           /* [K]: index into sel_ticks or -1 */
    const int *lane_sel;           /* [B]: index into log_lanes or -1 */
    int *next;                     /* shared lane counter */
    double *out_state, *out_coeffs, *out_first_yaw, *out_sel_log, *out_sel_cmd, *out_lane_log;
    int32_t *out_istate, *out_seg_rows;
    int rc;
} fleet_arg;

static void *fleet_worker(void *p) {
    fleet_arg *a = (fleet_arg *)p;
    const int m = a->m, K = a->K, B = a->B;
    double *coeffs = (double *)malloc(sizeof(double) * 24 * (size_t)m);
    double *times = (double *)malloc(sizeof(double) * (size_t)m);
    double *slog = (double *)malloc(sizeof(double) * 13 * (size_t)(K > 0 ? K : 1));
    double *clog = a->out_sel_cmd ? (double *)malloc(sizeof(double) * 12 * (size_t)(K > 0 ? K : 1)) : NULL;
    double *traj = NULL;
    int64_t cap = 0;
    if (!coeffs || !times || !slog || (a->out_sel_cmd && !clog)) { a->rc = -2; goto done; }
    for (;;) {
        const int b0 = __atomic_fetch_add(a->next, 64, __ATOMIC_RELAXED);
        if (b0 >= B) break;
        const int b1 = b0 + 64 < B ? b0 + 64 : B;
        for (int b = b0; b < b1; ++b) {
            const double *wp = a->wps + (size_t)b * (size_t)(m + 1) * 3;
            if (oracle_solve(wp, m, a->velocity, coeffs, times) != 0) { a->rc = -1; goto done; }
            int64_t rows = 0;
            for (int s = 0; s < m; ++s) {
                const int64_t cnt = (int64_t)ceil(times[s] / a->dt);
                if (a->out_seg_rows) a->out_seg_rows[(size_t)b * m + s] = (int32_t)cnt;
                rows += cnt;
            }
            if (rows > cap) {
                free(traj);
                cap = rows + rows / 4;
                traj = (double *)malloc(sizeof(double) * 11 * (size_t)cap);
                if (!traj) { a->rc = -2; goto done; }
            }
            oracle_sample(coeffs, times, m, a->dt, traj);
            if (a->out_coeffs) memcpy(a->out_coeffs + (size_t)b * 24 * m, coeffs, sizeof(double) * 24 * (size_t)m);
            if (a->out_first_yaw) a->out_first_yaw[b] = rows > 0 ? traj[9] : 0.0;
            double state[26] = {0};
            int32_t istate[4] = {0, 0, 0, 0};
            state[0] = wp[0]; state[1] = wp[1]; state[2] = wp[2]; state[3] = 1.0;
            const double hover = sqrt(a->V->mass * a->V->g / (4.0 * a->V->kf));
            for (int r = 13; r < 21; ++r) state[r] = hover;
            oracle_rollout(a->V, traj, rows, state, istate, K, slog, clog, a->aabbs, a->n_obs);
            if (a->out_state) memcpy(a->out_state + (size_t)b * 26, state, sizeof state);
            if (a->out_istate) memcpy(a->out_istate + (size_t)b * 4, istate, sizeof istate);
            for (int k = 0; k < K; ++k) {
                const int i = a->tick_sel[k];
                if (i < 0) continue;
                if (a->out_sel_log)
                    for (int c = 0; c < 13; ++c) a->out_sel_log[((size_t)i * 13 + c) * B + b] = slog[(size_t)k * 13 + c];
                if (a->out_sel_cmd)
                    for (int c = 0; c < 12; ++c) a->out_sel_cmd[((size_t)i * 12 + c) * B + b] = clog[(size_t)k * 12 + c];
            }
            const int j = a->lane_sel[b];
            if (j >= 0 && a->out_lane_log) memcpy(a->out_lane_log + (size_t)j * K * 13, slog, sizeof(double) * 13 * (size_t)K);
        }
    }
done:
    free(coeffs); free(times); free(slog); free(clog); free(traj);
    return NULL;
}

int oracle_fleet_threads(const oracle_vehicle *V, const double *wps, int B, int m, double velocity, double dt, int K,
                         const double *aabbs, int n_obs, const int32_t *sel_ticks, int n_sel, const int64_t *log_lanes, int n_ll,
                         int n_threads, double *out_state, int32_t *out_istate, int32_t *out_seg_rows, double *out_coeffs,
                         double *out_first_yaw, double *out_sel_log, double *out_sel_cmd, double *out_lane_log) {
    if (!V || !wps || B < 0 || m < 1 || K < 0 || n_sel < 0 || n_ll < 0 || n_obs < 0 || (n_obs > 0 && !aabbs) ||
        (n_sel > 0 && !sel_ticks) || (n_ll > 0 && !log_lanes))
        return -3;
    if (n_threads < 1) n_threads = 1;
    int *tick_sel = (int *)malloc(sizeof(int) * (size_t)(K > 0 ? K : 1));
    int *lane_sel = (int *)malloc(sizeof(int) * (size_t)(B > 0 ? B : 1));
    pthread_t *th = (pthread_t *)malloc(sizeof(pthread_t) * (size_t)n_threads);
    fleet_arg *args = (fleet_arg *)malloc(sizeof(fleet_arg) * (size_t)n_threads);
    int rc = 0, next = 0;
    if (!tick_sel || !lane_sel || !th || !args) { rc = -2; goto out; }
    for (int k = 0; k < K; ++k) tick_sel[k] = -1;
    for (int i = 0; i < n_sel; ++i) {
        if (sel_ticks[i] < 0 || sel_ticks[i] >= K) { rc = -3; goto out; }
        tick_sel[sel_ticks[i]] = i;
    }
    for (int b = 0; b < B; ++b) lane_sel[b] = -1;
    for (int j = 0; j < n_ll; ++j) {
        if (log_lanes[j] < 0 || log_lanes[j] >= B) { rc = -3; goto out; }
        lane_sel[log_lanes[j]] = j;
    }
    int started = 0;
    for (int t = 0; t < n_threads; ++t) {
        fleet_arg a = {V, wps, aabbs, B, m, K, n_obs, n_sel, velocity, dt, tick_sel, lane_sel, &next, out_state, out_coeffs,
                       out_first_yaw, out_sel_log, out_sel_cmd, out_lane_log, out_istate, out_seg_rows, 0};
        args[t] = a;
        if (pthread_create(&th[t], NULL, fleet_worker, &args[t]) != 0) { rc = -2; break; }
        ++started;
    }
    for (int t = 0; t < started; ++t) {
        pthread_join(th[t], NULL);
        if (args[t].rc != 0 && (rc == 0 || args[t].rc == -1)) rc = args[t].rc;
    }
out:
    free(tick_sel); free(lane_sel); free(th); free(args);
    return rc;
}

/* ------------------------------------------------------------------ whole-batch plan reference (tests only)
 * Missions [b0, b1) of a batch, each planned by oracle_solve and sampled by oracle_sample (bit for bit those two, mission by
 * mission), on n_threads POSIX threads (missions handed out 16 at a time).  Uniform batch: seg_offsets == NULL, wps [B][m+1][3].
 * Ragged batch: seg_offsets [B+1], mission b has seg_offsets[b+1] - seg_offsets[b] segments (1 .. m) and its waypoints are rows
 * seg_offsets[b] + b .. seg_offsets[b+1] + b of wps (S + B, 3) -- the layout of include/uavac.h.  Every output is relative to the
 * range (segment 0 = the first segment of mission b0, row 0 = its first row) and may be NULL:
 *   out_times / out_seg_rows   per segment, back to back;           out_row_offsets [n+1] (n = b1 - b0), out_row_offsets[0] = 0
 *   out_coeffs [segments][8][3];                                    out_first_yaw [n] (yaw of each mission's first row, 0 if none)
 *   out_rows [rows][11] (rows_capacity rows);                       out_jerk / out_snap [rows][3] (polynom orders 3 and 4)
 *   out_hit [segments] = 1 where a row of the spline lies in `cuboid` (inclusive bounds, minimum_snap.py:81-87 + :327-357)
 * With none of coeffs / rows / first_yaw / jerk / snap / hit asked for, only durations and row counts are computed (no solve):
 * what a caller needs to size the row buffer.  Returns 0, -1 when a system is singular, -2 out of memory, -3 bad arguments,
 * -4 when the rows do not fit rows_capacity (nothing solved then). */
typedef struct {
    const double *wps, *cuboid;
    const int64_t *seg_offsets;
    int m;
    int64_t b0, b1;
    double velocity, dt;
    const int64_t *seg0, *row0;                /* [n+1]: range-relative first segment and first row of every mission */
    int64_t *next;
    double *out_coeffs, *out_first_yaw, *out_rows, *out_jerk, *out_snap;
    int32_t *out_hit;
    int rc;
} plan_arg;

static int mission_segments(const int64_t *seg_offsets, int m, int64_t b) {
    return seg_offsets ? (int)(seg_offsets[b + 1] - seg_offsets[b]) : m;
}

static const double *mission_wps(const double *wps, const int64_t *seg_offsets, int m, int64_t b) {
    return wps + (size_t)3 * (seg_offsets ? (size_t)(seg_offsets[b] + b) : (size_t)b * (size_t)(m + 1));
}

/* jerk / snap of one mission's rows: polynom(3 | 4, t) . coeffs, in oracle_sample's dot-product order */
static void sample_derivs(const double *coeffs, const double *times, int m, double dt, double *jerk, double *snap) {
    int64_t n = 0;
    double row[NC];
    for (int s = 0; s < m; ++s) {
        const int64_t cnt = (int64_t)ceil(times[s] / dt);
        for (int64_t k = 0; k < cnt; ++k, ++n) {
            const double t = (double)k * dt;
            for (int ord = 3; ord <= 4; ++ord) {
                double *o = ord == 3 ? jerk : snap;
                if (!o) continue;
                polynom(ord, t, row);
                for (int j = 0; j < 3; ++j) {
                    double acc = 0.0;
                    for (int i = 0; i < NC; ++i) acc += row[i] * coeffs[(size_t)(s * NC + i) * 3 + j];
                    o[n * 3 + j] = acc;
                }
            }
        }
    }
}

static void *plan_worker(void *p) {
    plan_arg *a = (plan_arg *)p;
    const int m = a->m;
    const int64_t n = a->b1 - a->b0;
    double *coeffs = (double *)malloc(sizeof(double) * 24 * (size_t)m);
    double *times = (double *)malloc(sizeof(double) * (size_t)m);
    double *traj = NULL;
    int64_t cap = 0;
    if (!coeffs || !times) { a->rc = -2; goto done; }
    for (;;) {
        const int64_t i0 = __atomic_fetch_add(a->next, 16, __ATOMIC_RELAXED);
        if (i0 >= n) break;
        const int64_t i1 = i0 + 16 < n ? i0 + 16 : n;
        for (int64_t i = i0; i < i1; ++i) {
            const int64_t b = a->b0 + i;
            const int mb = mission_segments(a->seg_offsets, m, b);
            if (oracle_solve(mission_wps(a->wps, a->seg_offsets, m, b), mb, a->velocity, coeffs, times) != 0) { a->rc = -1; goto done; }
            const int64_t rows = a->row0[i + 1] - a->row0[i];
            if (rows > cap) {
                free(traj);
                cap = rows + rows / 4;
                traj = (double *)malloc(sizeof(double) * 11 * (size_t)cap);
                if (!traj) { a->rc = -2; goto done; }
            }
            if (oracle_sample(coeffs, times, mb, a->dt, traj) != rows) { a->rc = -3; goto done; }
            const int64_t s0 = a->seg0[i], r0 = a->row0[i];
            if (a->out_coeffs) memcpy(a->out_coeffs + (size_t)s0 * 24, coeffs, sizeof(double) * 24 * (size_t)mb);
            if (a->out_first_yaw) a->out_first_yaw[i] = rows > 0 ? traj[9] : 0.0;
            if (a->out_rows) memcpy(a->out_rows + (size_t)r0 * 11, traj, sizeof(double) * 11 * (size_t)rows);
            if (a->out_jerk || a->out_snap)
                sample_derivs(coeffs, times, mb, a->dt, a->out_jerk ? a->out_jerk + (size_t)r0 * 3 : NULL,
                              a->out_snap ? a->out_snap + (size_t)r0 * 3 : NULL);
            if (a->out_hit) {
                const double *c = a->cuboid;
                for (int s = 0; s < mb; ++s) a->out_hit[s0 + s] = 0;
                for (int64_t r = 0; r < rows; ++r) {
                    const double *o = traj + r * 11;
                    if (o[0] >= c[0] && o[0] <= c[1] && o[1] >= c[2] && o[1] <= c[3] && o[2] >= c[4] && o[2] <= c[5])
                        a->out_hit[s0 + (int)o[10]] = 1;
                }
            }
        }
    }
done:
    free(coeffs); free(times); free(traj);
    return NULL;
}

int oracle_plan_threads(const double *wps, const int64_t *seg_offsets, int B, int m, int64_t b0, int64_t b1, double velocity,
                        double dt, const double *cuboid, int n_threads, double *out_times, int32_t *out_seg_rows,
                        int64_t *out_row_offsets, double *out_coeffs, double *out_rows, int64_t rows_capacity,
                        double *out_first_yaw, double *out_jerk, double *out_snap, int32_t *out_hit) {
    if (!wps || B < 0 || m < 1 || b0 < 0 || b1 < b0 || b1 > B || !(dt > 0.0) || !(velocity > 0.0) || (out_hit && !cuboid))
        return -3;
    if (seg_offsets)
        for (int64_t b = b0; b < b1; ++b) {
            const int64_t mb = seg_offsets[b + 1] - seg_offsets[b];
            if (mb < 1 || mb > m) return -3;
        }
    if (n_threads < 1) n_threads = 1;
    if (n_threads > 16) n_threads = 16;
    const int64_t n = b1 - b0;
    int64_t *seg0 = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n + 1));
    int64_t *row0 = (int64_t *)malloc(sizeof(int64_t) * (size_t)(n + 1));
    double *times = (double *)malloc(sizeof(double) * (size_t)m);
    pthread_t *th = (pthread_t *)malloc(sizeof(pthread_t) * (size_t)n_threads);
    plan_arg *args = (plan_arg *)malloc(sizeof(plan_arg) * (size_t)n_threads);
    int rc = 0;
    int64_t next = 0;
    if (!seg0 || !row0 || !times || !th || !args) { rc = -2; goto out; }
    seg0[0] = row0[0] = 0;
    for (int64_t i = 0; i < n; ++i) {                            /* durations and row counts: oracle_solve's own times */
        const int64_t b = b0 + i;
        const int mb = mission_segments(seg_offsets, m, b);
        oracle_times(mission_wps(wps, seg_offsets, m, b), mb, velocity, times);
        int64_t rows = 0;
        for (int s = 0; s < mb; ++s) {
            const int64_t cnt = (int64_t)ceil(times[s] / dt);
            if (out_times) out_times[seg0[i] + s] = times[s];
            if (out_seg_rows) out_seg_rows[seg0[i] + s] = (int32_t)cnt;
            rows += cnt;
        }
        seg0[i + 1] = seg0[i] + mb;
        row0[i + 1] = row0[i] + rows;
    }
    if (out_row_offsets) memcpy(out_row_offsets, row0, sizeof(int64_t) * (size_t)(n + 1));
    if (!(out_coeffs || out_rows || out_first_yaw || out_jerk || out_snap || out_hit)) goto out;
    if ((out_rows || out_jerk || out_snap) && row0[n] > rows_capacity) { rc = -4; goto out; }
    int started = 0;
    for (int t = 0; t < n_threads; ++t) {
        plan_arg a = {wps, cuboid, seg_offsets, m, b0, b1, velocity, dt, seg0, row0, &next, out_coeffs, out_first_yaw, out_rows,
                      out_jerk, out_snap, out_hit, 0};
        args[t] = a;
        if (pthread_create(&th[t], NULL, plan_worker, &args[t]) != 0) { rc = -2; break; }
        ++started;
    }
    for (int t = 0; t < started; ++t) {
        pthread_join(th[t], NULL);
        if (args[t].rc != 0 && (rc == 0 || args[t].rc == -1)) rc = args[t].rc;
    }
out:
    free(seg0); free(row0); free(times); free(th); free(args);
    return rc;
}

/* ------------------------------------------------------------------ high-precision solve (tests only)
 * oracle_solve's dense KKT assembly and pivoted LU carried out in long double (x87 extended on x86-64: 64-bit mantissa), from
 * the same fp64 durations: a reference for the TRUE error of the kernels' solves and of the fp64 oracle.  Returns 0, -1 singular,
 * -2 out of memory, -5 when this platform's long double is not wider than double (no silent fall-back to fp64). */
#include <float.h>

int oracle_ldbl_mant_dig(void) { return LDBL_MANT_DIG; }

static void polynom_ld(int order, long double t, long double *row) {
    for (int i = 0; i < NC; ++i) {
        long double poly = 1.0L, der = (long double)i;
        for (int k = 0; k < order; ++k) {
            poly *= der;
            if (der > 0) der -= 1.0L;
        }
        row[i] = poly * powl(t, der);
    }
}

static int lu_solve_ld(long double *A, long double *b, int n, int nrhs) {
    for (int k = 0; k < n; ++k) {
        int p = k;
        long double best = fabsl(A[k * n + k]);
        for (int i = k + 1; i < n; ++i)
            if (fabsl(A[i * n + k]) > best) { best = fabsl(A[i * n + k]); p = i; }
        if (!(best > 0.0L)) return -1;
        if (p != k) {
            for (int j = 0; j < n; ++j) { long double t = A[k * n + j]; A[k * n + j] = A[p * n + j]; A[p * n + j] = t; }
            for (int j = 0; j < nrhs; ++j) { long double t = b[k * nrhs + j]; b[k * nrhs + j] = b[p * nrhs + j]; b[p * nrhs + j] = t; }
        }
        for (int i = k + 1; i < n; ++i) {
            long double l = A[i * n + k] / A[k * n + k];
            if (l == 0.0L) continue;
            for (int j = k + 1; j < n; ++j) A[i * n + j] -= l * A[k * n + j];
            for (int j = 0; j < nrhs; ++j) b[i * nrhs + j] -= l * b[k * nrhs + j];
        }
    }
    for (int i = n - 1; i >= 0; --i)
        for (int j = 0; j < nrhs; ++j) {
            long double s = b[i * nrhs + j];
            for (int c = i + 1; c < n; ++c) s -= A[i * n + c] * b[c * nrhs + j];
            b[i * nrhs + j] = s / A[i * n + i];
        }
    return 0;
}

int oracle_solve_ld(const double *wp, int m, double velocity, double *coeffs, double *times) {
    if (LDBL_MANT_DIG < 64) return -5;
    oracle_times(wp, m, velocity, times);
    int nu = NC * m, ncon = 6 * m + 2, n = nu + ncon;
    long double *K = (long double *)calloc((size_t)n * n, sizeof(long double));
    long double *rhs = (long double *)calloc((size_t)n * 3, sizeof(long double));
    if (!K || !rhs) { free(K); free(rhs); return -2; }
    long double row[NC], row0[NC];
    int r = 0;
#define SETA_LD(rr, cc, v) do { K[(size_t)(nu + (rr)) * n + (cc)] = (v); K[(size_t)(cc) * n + nu + (rr)] = (v); } while (0)
    polynom_ld(0, 0.0L, row0);
    for (int s = 0; s < m; ++s, ++r) {
        for (int i = 0; i < NC; ++i) SETA_LD(r, s * NC + i, row0[i]);
        for (int j = 0; j < 3; ++j) rhs[(size_t)(nu + r) * 3 + j] = wp[3 * s + j];
    }
    for (int s = 0; s < m; ++s, ++r) {
        polynom_ld(0, times[s], row);
        for (int i = 0; i < NC; ++i) SETA_LD(r, s * NC + i, row[i]);
        for (int j = 0; j < 3; ++j) rhs[(size_t)(nu + r) * 3 + j] = wp[3 * (s + 1) + j];
    }
    for (int k = 1; k <= 3; ++k, ++r) {
        polynom_ld(k, 0.0L, row);
        for (int i = 0; i < NC; ++i) SETA_LD(r, i, row[i]);
    }
    for (int k = 1; k <= 3; ++k, ++r) {
        polynom_ld(k, times[m - 1], row);
        for (int i = 0; i < NC; ++i) SETA_LD(r, (m - 1) * NC + i, row[i]);
    }
    for (int s = 1; s < m; ++s)
        for (int k = 1; k <= 4; ++k, ++r) {
            polynom_ld(k, times[s - 1], row);
            polynom_ld(k, 0.0L, row0);
            for (int i = 0; i < NC; ++i) { SETA_LD(r, (s - 1) * NC + i, row[i]); SETA_LD(r, s * NC + i, -row0[i]); }
        }
#undef SETA_LD
    for (int s = 0; s < m; ++s)
        for (int a = 4; a < NC; ++a)
            for (int c = 4; c < NC; ++c) {
                long double fa = a * (a - 1) * (a - 2) * (a - 3), fc = c * (c - 1) * (c - 2) * (c - 3);
                int e = a + c - 7;
                K[(size_t)(s * NC + a) * n + s * NC + c] = fa * fc * powl((long double)times[s], e) / e;
            }
    int rc = lu_solve_ld(K, rhs, n, 3);
    if (rc == 0)
        for (int i = 0; i < nu * 3; ++i) coeffs[i] = (double)rhs[i];
    free(K); free(rhs);
    return rc;
}

/* ------------------------------------------------------------------ high-precision tick (tests only)
 * oracle_rollout's tick -- controller (main.py:37-61, controller.py:26-168, quad.py:88-122) then vehicle (mujoco_sim.py:232-251 +
 * the Euler free-joint step and the build-defined ground contact) -- with every operation in long double, from the same fp64
 * state, rows and vehicle, rounded to fp64 where a value leaves: the end state and the two logs.  Between ticks of one call the
 * state stays in long double.  Written from the upstream formulas, not from the fp64 functions above: the rotation matrix in
 * closed form, the quaternion product as the Hamilton product.  Integer outputs follow oracle_rollout's rules.  Does nothing
 * where long double is no wider than double (callers ask oracle_ldbl_mant_dig first). */
typedef long double ld;
#define PI_LD 3.141592653589793238462643383279502884L

static ld clip_ld(ld x, ld lo, ld hi) { return x < lo ? lo : (x > hi ? hi : x); }

static ld pymod_ld(ld a, ld b) { /* Python's float % for b > 0 */
    ld r = fmodl(a, b);
    if (r < 0.0L) r += b;
    return r;
}

typedef struct {
    ld p[3], q[4], v[3], w[3], om[4], omc[4], integ, thrust, pqr[3];
    int32_t idx, inner, collided, gbits;
} uav_ld;

/* body -> world rotation of the normalised quaternion (quad.py:133-155, written out) */
static void rot_ld(const ld *q, ld R[3][3]) {
    const ld n = sqrtl(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const ld a = q[0] / n, b = q[1] / n, c = q[2] / n, d = q[3] / n;
    R[0][0] = 1.0L - 2.0L * (c * c + d * d); R[0][1] = 2.0L * (b * c - a * d);        R[0][2] = 2.0L * (b * d + a * c);
    R[1][0] = 2.0L * (b * c + a * d);        R[1][1] = 1.0L - 2.0L * (b * b + d * d); R[1][2] = 2.0L * (c * d - a * b);
    R[2][0] = 2.0L * (b * d - a * c);        R[2][1] = 2.0L * (c * d + a * b);        R[2][2] = 1.0L - 2.0L * (b * b + c * c);
}

static void controller_tick_ld(const oracle_vehicle *V, uav_ld *u, const double *traj, int64_t nrows) {
    const ld mass = V->mass, fmin_ = V->min_thrust, fmax_ = V->max_thrust;
    if (u->inner % V->F == 0 && nrows > 0) {
        const double *tg = traj + (int64_t)u->idx * 11;
        ld R[3][3];
        rot_ld(u->q, R);
        /* altitude */
        const ld zd = clip_ld((ld)tg[5], -(ld)V->max_ascent, (ld)V->max_descent);
        const ld ez = (ld)tg[2] - u->p[2], ezd = zd - u->v[2];
        u->integ = clip_ld(u->integ + ez * (ld)V->dt_outer, -10.0L, 10.0L);
        const ld acc = ((ld)V->kp_z * ez + (ld)V->ki_z * u->integ + (ld)V->kd_z * ezd + (ld)tg[8] - (ld)V->g) / R[2][2];
        const ld c = clip_ld(-mass * acc, 4.0L * fmin_, 4.0L * fmax_);
        u->thrust = c;
        /* lateral */
        ld vdx = tg[3], vdy = tg[4];
        const ld vm = sqrtl(vdx * vdx + vdy * vdy);
        if (vm > (ld)V->max_speed_xy) { vdx = vdx / vm * (ld)V->max_speed_xy; vdy = vdy / vm * (ld)V->max_speed_xy; }
        ld ax = (ld)V->kp_xy * ((ld)tg[0] - u->p[0]) + (ld)V->kd_xy * (vdx - u->v[0]) + (ld)tg[6];
        ld ay = (ld)V->kp_xy * ((ld)tg[1] - u->p[1]) + (ld)V->kd_xy * (vdy - u->v[1]) + (ld)tg[7];
        const ld am = sqrtl(ax * ax + ay * ay);
        if (am > (ld)V->max_horiz_accel) { ax = ax / am * (ld)V->max_horiz_accel; ay = ay / am * (ld)V->max_horiz_accel; }
        const ld az = -c / mass;
        const ld bx = clip_ld(ax / az, -(ld)V->max_tilt, (ld)V->max_tilt), by = clip_ld(ay / az, -(ld)V->max_tilt, (ld)V->max_tilt);
        /* roll / pitch */
        const ld bdx = (ld)V->kp_roll * (bx - R[0][2]), bdy = (ld)V->kp_pitch * (by - R[1][2]);
        const ld pc = (R[1][0] * bdx - R[0][0] * bdy) / R[2][2];
        const ld qc = (R[1][1] * bdx - R[0][1] * bdy) / R[2][2];
        /* yaw, on the Euler angles of the stored quaternion (quad.py:189-213) */
        const ld *q = u->q;
        const ld phi = atan2l(2.0L * (q[0] * q[1] + q[2] * q[3]), 1.0L - 2.0L * (q[1] * q[1] + q[2] * q[2]));
        const ld theta = asinl(clip_ld(2.0L * (q[0] * q[2] - q[3] * q[1]), -1.0L, 1.0L));
        const ld psi = atan2l(2.0L * (q[0] * q[3] + q[1] * q[2]), 1.0L - 2.0L * (q[2] * q[2] + q[3] * q[3]));
        const ld pd = pymod_ld((ld)tg[9], 2.0L * PI_LD);
        const ld ye = pymod_ld(pd - psi + PI_LD, 2.0L * PI_LD) - PI_LD;
        u->pqr[0] = pc; u->pqr[1] = qc;
        u->pqr[2] = ((ld)V->kp_yaw * ye * cosl(theta) - qc * sinl(phi)) / cosl(phi);
        u->idx = (u->idx + 1 < nrows - 1) ? u->idx + 1 : (int32_t)(nrows - 1);
    }
    /* body rates: I kp (cmd - w) + w x (I w) */
    const ld *w = u->w;
    const ld I0 = V->I[0], I1 = V->I[1], I2 = V->I[2];
    const ld Mx = I0 * (ld)V->kp_p * (u->pqr[0] - w[0]) + (w[1] * (I2 * w[2]) - w[2] * (I1 * w[1]));
    const ld My = I1 * (ld)V->kp_q * (u->pqr[1] - w[1]) + (w[2] * (I0 * w[0]) - w[0] * (I2 * w[2]));
    const ld Mz = I2 * (ld)V->kp_r * (u->pqr[2] - w[2]) + (w[0] * (I1 * w[1]) - w[1] * (I0 * w[0]));
    /* allocation */
    const ld col = clip_ld(u->thrust, 4.0L * fmin_, 4.0L * fmax_) / 4.0L;
    const ld pb = Mx / (ld)V->arm, qb = My / (ld)V->arm, rb = -Mz / (ld)V->kappa;
    const ld mf[4] = {(pb + qb + rb) / 4.0L, (-pb + qb - rb) / 4.0L, (-pb - qb + rb) / 4.0L, (pb - qb - rb) / 4.0L};
    ld lim = 1.0L;                                                  /* min over rotors of the limit, clipped to [0, 1] below */
    int any = 0;
    for (int i = 0; i < 4; ++i) {
        ld l = 1.0L;
        if (mf[i] > 0.0L) l = (fmax_ - col) / mf[i];
        else if (mf[i] < 0.0L) l = (fmin_ - col) / mf[i];
        if (!any || l < lim) lim = l;
        any = 1;
    }
    const ld sc = clip_ld(lim, 0.0L, 1.0L);
    for (int i = 0; i < 4; ++i) {
        const ld f = clip_ld(col + sc * mf[i], fmin_, fmax_);
        u->omc[i] = sqrtl(f / (ld)V->kf);
        const ld tau = u->omc[i] > u->om[i] ? (ld)V->tau_rise : (ld)V->tau_fall;
        u->om[i] += (1.0L - expl(-(ld)V->dt / tau)) * (u->omc[i] - u->om[i]);
    }
    u->inner += 1;
}

static void dynamics_step_ld(const oracle_vehicle *V, uav_ld *u) {
    const ld dt = V->dt, kf = V->kf, arm = V->arm, mass = V->mass;
    ld f[4];
    for (int i = 0; i < 4; ++i) f[i] = kf * u->om[i] * u->om[i];
    const ld T = f[0] + f[1] + f[2] + f[3];
    const ld tau[3] = {arm * (f[0] + f[3] - f[1] - f[2]), arm * (f[0] + f[1] - f[2] - f[3]), (ld)V->kappa * (-f[0] + f[1] - f[2] + f[3])};
    ld R[3][3];
    rot_ld(u->q, R);
    ld *w = u->w;
    const ld I[3] = {V->I[0], V->I[1], V->I[2]};
    const ld gyro[3] = {w[1] * (I[2] * w[2]) - w[2] * (I[1] * w[1]), w[2] * (I[0] * w[0]) - w[0] * (I[2] * w[2]),
                        w[0] * (I[1] * w[1]) - w[1] * (I[0] * w[0])};
    const ld acc[3] = {-(T / mass) * R[0][2], -(T / mass) * R[1][2], (ld)V->g - (T / mass) * R[2][2]};
    ld vz_ref = 0.0L;
    int touching = 0;
    if (V->ground) {
        const ld r = u->p[2] - ((ld)V->ground_z - (ld)V->ground_clearance), tc = V->ground_timeconst;
        if (r > 0.0L) { touching = 1; vz_ref = u->v[2] + dt * -(2.0L / tc * u->v[2] + r / (tc * tc)); }
    }
    for (int i = 0; i < 3; ++i) u->v[i] += dt * acc[i];
    if (touching && vz_ref < u->v[2]) u->v[2] = vz_ref;
    ld wn2 = 0.0L;
    for (int i = 0; i < 3; ++i) {
        w[i] += dt * ((tau[i] - gyro[i]) / I[i]);
        u->p[i] += dt * u->v[i];
        wn2 += w[i] * w[i];
    }
    /* q <- normalise(q (x) [cos h, sin(h) w / |w|]), h = |w| dt / 2 */
    const ld *q = u->q;
    ld nq[4] = {q[0], q[1], q[2], q[3]};
    const ld wn = sqrtl(wn2);
    if (wn > 0.0L) {
        const ld h = 0.5L * wn * dt, s = sinl(h) / wn, d0 = cosl(h), d1 = s * w[0], d2 = s * w[1], d3 = s * w[2];
        nq[0] = q[0] * d0 - q[1] * d1 - q[2] * d2 - q[3] * d3;
        nq[1] = q[0] * d1 + q[1] * d0 + q[2] * d3 - q[3] * d2;
        nq[2] = q[0] * d2 - q[1] * d3 + q[2] * d0 + q[3] * d1;
        nq[3] = q[0] * d3 + q[1] * d2 - q[2] * d1 + q[3] * d0;
    }
    const ld nn = sqrtl(nq[0] * nq[0] + nq[1] * nq[1] + nq[2] * nq[2] + nq[3] * nq[3]);
    for (int i = 0; i < 4; ++i) u->q[i] = nq[i] / nn;
    if (V->ground) {
        const ld zc = (ld)V->ground_z - (ld)V->ground_clearance;
        if ((ld)V->ground_z - u->p[2] >= 0.1L) u->gbits |= 2;
        const int now = u->p[2] - zc > 0.0L;
        u->gbits = now ? (u->gbits | 1) : (u->gbits & ~1);
        if (now && (u->gbits & 2)) u->gbits |= 4;
    }
}

static void x_of_ld(const uav_ld *u, double *X) {
    for (int i = 0; i < 3; ++i) { X[i] = (double)u->p[i]; X[7 + i] = (double)u->v[i]; X[10 + i] = (double)u->w[i]; }
    for (int i = 0; i < 4; ++i) X[3 + i] = (double)u->q[i];
}

void oracle_rollout_ld(const oracle_vehicle *V, const double *traj, int64_t nrows, double *state, int32_t *istate,
                       int K, double *state_log, double *cmd_log, const double *aabbs, int n_obs) {
    if (LDBL_MANT_DIG < 64) return;
    uav_ld u;
    for (int i = 0; i < 3; ++i) { u.p[i] = state[i]; u.v[i] = state[7 + i]; u.w[i] = state[10 + i]; u.pqr[i] = state[23 + i]; }
    for (int i = 0; i < 4; ++i) { u.q[i] = state[3 + i]; u.om[i] = state[13 + i]; u.omc[i] = state[17 + i]; }
    u.integ = state[21]; u.thrust = state[22];
    u.idx = istate[0]; u.inner = istate[1]; u.collided = istate[2]; u.gbits = istate[3];
    for (int k = 0; k < K; ++k) {
        controller_tick_ld(V, &u, traj, nrows);
        if (cmd_log) {
            double *c = cmd_log + (size_t)k * 12;
            c[0] = (double)u.thrust;
            for (int i = 0; i < 3; ++i) c[1 + i] = (double)u.pqr[i];
            for (int i = 0; i < 4; ++i) { c[4 + i] = (double)u.omc[i]; c[8 + i] = (double)u.om[i]; }
        }
        dynamics_step_ld(V, &u);
        for (int o = 0; o < n_obs; ++o) {
            const double *c = aabbs + 6 * o;
            if (u.p[0] >= c[0] && u.p[0] <= c[1] && u.p[1] >= c[2] && u.p[1] <= c[3] && u.p[2] >= c[4] && u.p[2] <= c[5])
                u.collided = 1;
        }
        if (state_log) x_of_ld(&u, state_log + (size_t)k * 13);
    }
    x_of_ld(&u, state);
    for (int i = 0; i < 4; ++i) { state[13 + i] = (double)u.om[i]; state[17 + i] = (double)u.omc[i]; }
    state[21] = (double)u.integ; state[22] = (double)u.thrust;
    for (int i = 0; i < 3; ++i) state[23 + i] = (double)u.pqr[i];
    istate[0] = u.idx; istate[1] = u.inner; istate[2] = u.collided; istate[3] = u.gbits;
}

/* Margins of the discontinuous decisions one OUTER + vehicle tick takes from (state, istate), in long double, for tests that must
 * not compare values across a decision the reference itself takes by a hair: out[0] = distance of the yaw error's argument
 * (pd - psi + pi) mod 2 pi from the wrap (0 or 2 pi), out[1] = |R22|, out[2] = |r| of the ground test before the step,
 * out[3] = |r| after it, out[4] = |ground_z - z - take-off height| after it.  Entries that do not apply (no outer tick, no
 * ground) are 1. */
void oracle_tick_margins_ld(const oracle_vehicle *V, const double *traj, int64_t nrows, const double *state, const int32_t *istate,
                            double *out) {
    for (int i = 0; i < 5; ++i) out[i] = 1.0;
    if (LDBL_MANT_DIG < 64) return;
    ld q[4] = {state[3], state[4], state[5], state[6]};
    if (istate[1] % V->F == 0 && nrows > 0) {
        ld R[3][3];
        rot_ld(q, R);
        out[1] = (double)fabsl(R[2][2]);
        const double *tg = traj + (int64_t)istate[0] * 11;
        const ld psi = atan2l(2.0L * (q[0] * q[3] + q[1] * q[2]), 1.0L - 2.0L * (q[2] * q[2] + q[3] * q[3]));
        const ld a = pymod_ld(pymod_ld((ld)tg[9], 2.0L * PI_LD) - psi + PI_LD, 2.0L * PI_LD);
        out[0] = (double)(a < 2.0L * PI_LD - a ? a : 2.0L * PI_LD - a);
    }
    if (V->ground) {
        double s[26];
        int32_t is[4];
        memcpy(s, state, sizeof s); memcpy(is, istate, sizeof is);
        const ld zc = (ld)V->ground_z - (ld)V->ground_clearance;
        out[2] = (double)fabsl((ld)state[2] - zc);
        oracle_rollout_ld(V, traj, nrows, s, is, 1, NULL, NULL, NULL, 0);
        out[3] = (double)fabsl((ld)s[2] - zc);
        out[4] = (double)fabsl((ld)V->ground_z - (ld)s[2] - 0.1L);
    }
}
