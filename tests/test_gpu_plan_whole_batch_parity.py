"""Every mission of the planning chain, in the solve and sample forms the batch and the options select, against an independent
reference: the C oracle plans every mission itself (`c_oracle.plan_threads`: oracle_solve + oracle_sample on POSIX threads),
slice by slice while the GPU works, and each slice is compared on the device.  Before this file the oracle saw the headline plan
(config 3: 65 536 missions, m = 12, the keep form of the two-ended solve) in no mission at all, most solve and sampler forms only
HIP against HIP, and the dense-yaw-column sampler forms with 1, 4 and 16 chunks per store never ran.  Every case asserts the
kernel it reached (`Context.last_solve_kernel` / `last_sample_kernel`).

Bars, the same for every mission: durations, row counts and row offsets exactly equal; coefficients within 1e-9 (SURVEY 8(c)
column metric, per mission); positions, velocities, accelerations within 1e-5 (column metric); spline ids exact; first headings
within 1e-9.  The yaw column is compared RAW: a difference of k 2 pi is accepted only from a row where the oracle's heading steps
by pi to within 1e-9 (a genuine np.unwrap tie, decided by the last bit of two atan2 results) and must then stay to the end of
the mission; such forks are counted and printed (`-s`), as are the largest errors seen."""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL, COEFF_TOL, YAW0_TOL, TIE_TOL = 1e-5, 1e-9, 1e-9, 1e-9
VEL, DT = 3.0, 0.01
SLICE = 4096
SENTINEL = -1.2345e300
TWO_PI = 2 * math.pi
WORST = {}                                    # case -> {metric: largest error seen}; printed at the end of the module
FORKS = {}                                    # case -> missions whose yaw forks by 2 pi at an unwrap tie
FACE_TIES = {}                                # case -> splines whose hit flag differs where a sample lies on a face
DEFAULTS = dict(solve_order=1, solve_park=-1, solve_lanes=-1, solve_keep=-1, sampler_waves=4, sampler_group=1, yaw_group=8)


@pytest.fixture(scope="module")
def eng():
    from uav_ac.fleet import Engine
    e = Engine("cuda:0")
    yield e
    for k, v in DEFAULTS.items():
        e.ctx.set_option(k, v)


@pytest.fixture(scope="module")
def pool():
    ex = ThreadPoolExecutor(max_workers=2)    # the oracle runs (on its own threads) while the GPU plans and compares
    yield ex
    ex.shutdown(wait=True)
    for case in sorted(WORST):
        w = ", ".join(f"{k} {v:.3e}" for k, v in sorted(WORST[case].items()))
        print(f"plan parity {case}: {w}; yaw forks at unwrap ties {FORKS.get(case, 0)}; hit flags at face ties {FACE_TIES.get(case, 0)}")


class _opts:
    """ctx options for the duration of a with-block; the defaults afterwards."""

    def __init__(self, eng, **kw):
        self.eng, self.kw = eng, kw

    def __enter__(self):
        for k, v in self.kw.items():
            self.eng.ctx.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.eng.ctx.set_option(k, DEFAULTS[k])


def _simds():
    import torch
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count


def _note(case, **errs):
    w = WORST.setdefault(case, {})
    for k, v in errs.items():
        w[k] = max(w.get(k, 0.0), float(v))


def _tf(v):
    return "true" if v else "false"


def _expect_solve(B, m, order=1, lanes=-1, park=-1, keep=-1, ragged=False):
    """The kernel uavac_launch_coeff_solve and the two launchers behind it pick for these options (their dispatch, restated)."""
    S = _simds()
    cus = S // 4
    if order == 1 or (order < 0 and not (m <= 8 and not ragged and B >= 48 * S)):
        waves32 = (B + 31) // 32
        nm = {64: 32, 32: 16, 16: 8}.get(lanes, 16 if waves32 <= S // 2 else 32)
        waves = (B + nm - 1) // nm
        lk = (m - 1) // 2 if m > 1 else 0
        pk = lk * 28 * 2 * nm * 8
        static = 8 * 64 * 28 + (32 * 12 if ragged else 12)
        fits = lk > 0 and pk + static <= 150 * 1024
        per_cu = (156 * 1024) // (pk + static) if fits else 0
        lds = fits and (park != 0 if park >= 0 else waves <= cus * min(per_cu, 8))
        kp = not ragged and not lds and (keep != 0 if keep >= 0 else (lanes < 0 and waves32 >= S and lk >= 4))
        if kp:
            return "minsnap_solve_tw_kernel<false, false, 32, 5>"
        return f"minsnap_solve_tw_kernel<{_tf(ragged)}, {_tf(lds)}, {nm}, 0>"
    waves64 = (B + 63) // 64
    ln = lanes if lanes in (64, 32, 16) else (32 if waves64 <= S else 64)
    waves = (B + ln - 1) // ln
    pk = (m - 1 if m > 1 else 0) * 28 * ln * 8
    static = 8 * 64 * 25 + (64 * 12 if ragged else 12)
    fits = m > 1 and pk + static <= 150 * 1024
    per_cu = (156 * 1024) // (pk + static) if fits else 0
    lds = fits and (park != 0 if park >= 0 else waves <= cus * min(per_cu, 8))
    kp = not ragged and not lds and (keep != 0 if keep >= 0 else (lanes < 0 and waves64 >= S))
    if kp:
        return "minsnap_solve_bt_kernel<false, false, 64, 5>"
    return f"minsnap_solve_bt_kernel<{_tf(ragged)}, {_tf(lds)}, {ln}, 0>"


# ------------------------------------------------------------------------------------------------------------ comparisons
def _check_solve(case, eng, got, ref, ragged=False):
    """Durations and row counts equal, coefficients within 1e-9 per mission, first headings within 1e-9 (raw) -- every mission.
    got: a Plan / RaggedBatch or a dict of device tensors (times, seg_rows, coeffs[, first_yaw]) for the range of ref."""
    import torch
    dev = eng.device
    g = got if isinstance(got, dict) else {k: getattr(got, k) for k in ("times", "seg_rows", "coeffs", "first_yaw")}
    t = g["times"].reshape(-1).cpu().numpy()
    assert np.array_equal(t, ref["times"].reshape(-1)), f"{case}: durations differ at {np.flatnonzero(t != ref['times'].reshape(-1))[:8]}"
    sr = g["seg_rows"].reshape(-1).cpu().numpy()
    bad = np.flatnonzero(sr != ref["seg_rows"].reshape(-1))
    assert len(bad) == 0, f"{case}: row counts differ at segments {bad[:8].tolist()}"
    co = g["coeffs"].reshape(-1, 8, 3)
    rc = torch.from_numpy(np.ascontiguousarray(ref["coeffs"]).reshape(-1, 8, 3)).to(dev)
    if ragged:                                                   # per mission: segments seg_offsets[b] .. seg_offsets[b + 1]
        so = torch.from_numpy(ref["seg_offsets"]).to(dev)
        mid = torch.searchsorted(so, torch.arange(rc.shape[0], device=dev), right=True) - 1
        B = len(ref["seg_offsets"]) - 1
        scale = torch.zeros((B, 3), dtype=torch.float64, device=dev).scatter_reduce(
            0, mid[:, None].expand(-1, 3), rc.abs().amax(1), reduce="amax").clamp_min(1.0)
        e = float(((co - rc).abs().amax(1) / scale[mid]).max()) if rc.shape[0] else 0.0
    else:
        n, m = ref["seg_rows"].shape
        co, rc = co.reshape(n, 8 * m, 3), rc.reshape(n, 8 * m, 3)
        e = float(((co - rc).abs().amax(1) / rc.abs().amax(1).clamp_min(1.0)).max()) if n else 0.0
    _note(case, coeffs=e)
    assert e <= COEFF_TOL, f"{case}: coefficients off by {e:.3e}"
    if g.get("first_yaw") is not None and "first_yaw" in ref:
        fy = float(np.abs(g["first_yaw"].cpu().numpy() - ref["first_yaw"]).max()) if len(ref["first_yaw"]) else 0.0
        _note(case, first_yaw=fy)
        assert fy <= YAW0_TOL, f"{case}: first headings off by {fy:.3e}"


def _check_rows(case, eng, got, ref_rows, ref_ro):
    """got (N, 11) device rows of the missions whose oracle rows are ref_rows (N, 11) host, range-relative offsets ref_ro."""
    import torch
    dev = eng.device
    assert got.shape[0] == ref_rows.shape[0], (case, got.shape, ref_rows.shape)
    if got.shape[0] == 0:
        return
    r = torch.from_numpy(np.ascontiguousarray(ref_rows)).to(dev)
    bad = (got[:, 10] != r[:, 10]).nonzero()
    assert len(bad) == 0, f"{case}: spline ids differ from row {int(bad[0])}"
    e = float(((got[:, :9] - r[:, :9]).abs().amax(0) / r[:, :9].abs().amax(0).clamp_min(1.0)).max())
    _note(case, rows=e)
    assert e <= TOL, f"{case}: positions / velocities / accelerations off by {e:.3e}"
    forks = _check_yaw(case, got[:, 9], r[:, 9], torch.from_numpy(np.ascontiguousarray(ref_ro)).to(dev))
    FORKS[case] = FORKS.get(case, 0) + forks
    del r


def _check_yaw(case, got, ref, ro):
    """Raw yaw: within TOL beyond whole turns; a whole-turn difference k 2 pi is 0 on a mission's first row and changes only inside
    a mission, at a row where the oracle's heading steps by pi to within 1e-9 (an np.unwrap tie), at most once per mission.
    -> the number of such forks."""
    import torch
    N = ref.shape[0]
    d = got - ref
    k = torch.round(d / TWO_PI)
    resid = float((d - k * TWO_PI).abs().max()) / max(1.0, float(ref.abs().max()))
    _note(case, yaw=resid)
    assert resid <= TOL, f"{case}: yaw off by {resid:.3e} (beyond whole turns)"
    mid = torch.searchsorted(ro, torch.arange(N, device=ref.device), right=True) - 1
    first = torch.zeros(N, dtype=torch.bool, device=ref.device)
    first[ro[:-1]] = True
    bad0 = (first & (k != 0)).nonzero()[:, 0]
    assert len(bad0) == 0, f"{case}: yaw off by whole turns from the first row of mission {int(mid[bad0[0]])}"
    change = ((k[1:] != k[:-1]) & ~first[1:]).nonzero()[:, 0] + 1
    if len(change) == 0:
        return 0
    step = (ref[change] - ref[change - 1]).abs()
    tie = (step - math.pi).abs() <= TIE_TOL
    assert bool(tie.all()), (f"{case}: yaw jumps by 2 pi at row {int(change[~tie][0])} (mission {int(mid[change[~tie][0]])}) where the "
                             f"oracle's heading steps by {float(step[~tie][0]):.17g}: no unwrap tie")
    fm = mid[change]
    assert len(torch.unique(fm)) == len(fm), f"{case}: a mission's yaw forks twice"
    return int(len(fm))


def _sliced(case, eng, pool, wps, plan, slice_=SLICE):
    """Every mission of a plan with rows against the oracle, slice by slice: the oracle of the next slice runs while this one is
    compared (at most two slices' rows on the host)."""
    from oracle import c_oracle as cc
    B = plan.B
    ro_all = plan.row_offsets.cpu().numpy()
    bounds = list(range(0, B, slice_)) + [B]
    nxt = pool.submit(cc.plan_threads, wps, plan.velocity, plan.dt, bounds[0], bounds[1])
    for i in range(len(bounds) - 1):
        b0, b1 = bounds[i], bounds[i + 1]
        ref = nxt.result()
        if i + 2 < len(bounds):
            nxt = pool.submit(cc.plan_threads, wps, plan.velocity, plan.dt, b1, bounds[i + 2])
        assert np.array_equal(ro_all[b0:b1 + 1] - ro_all[b0], ref["row_offsets"]), f"{case}: row offsets differ in [{b0}, {b1})"
        sl = {"times": plan.times[b0:b1], "seg_rows": plan.seg_rows[b0:b1], "coeffs": plan.coeffs[b0:b1], "first_yaw": plan.first_yaw[b0:b1]}
        _check_solve(case, eng, sl, ref)
        if plan.traj is not None:
            _check_rows(case, eng, plan.traj[int(ro_all[b0]):int(ro_all[b1])], ref["rows"], ref["row_offsets"])
        del ref


def _ld_errors(case, plan, wps, picks):
    """True error (against the long double solve) of the kernel's coefficients and of the fp64 oracle's, on picked missions."""
    from oracle import c_oracle as cc
    co = plan.coeffs[list(picks)].cpu().numpy()
    e_k = e_o = 0.0
    for i, b in enumerate(picks):
        ld, _ = cc.solve_ld(wps[b], plan.velocity)
        _, c64, _ = cc.plan(wps[b], plan.velocity, plan.dt)
        sc = np.maximum(1.0, np.abs(ld).max(0))
        e_k = max(e_k, float((np.abs(co[i] - ld).max(0) / sc).max()))
        e_o = max(e_o, float((np.abs(c64 - ld).max(0) / sc).max()))
    _note(case, kernel_vs_ld=e_k, oracle_vs_ld=e_o)
    assert e_k <= COEFF_TOL and e_o <= COEFF_TOL, (case, e_k, e_o)


# ------------------------------------------------------------------------------------------------------- A, B: bench shapes
@pytest.mark.parametrize("case,m", [("A config3 m=12", 12), ("B config5-shape m=20", 20)])
def test_bench_plan_every_mission(eng, pool, case, m):
    """A: config 3, the headline plan -- bench.missions(65 536, 12), default options: the keep form of the two-ended solve (five
    blocks per lane in registers, the sixth in LDS) and the default streaming sampler; ~85 M rows.  B: the same generator at
    m = 20, where a lane's blocks past the sixth go to the HBM workspace."""
    import bench
    B = 65536
    wps = bench.missions(B, m, 0, B)
    plan = eng.plan(wps, VEL, DT)
    assert eng.ctx.last_solve_kernel() == "minsnap_solve_tw_kernel<false, false, 32, 5>" == _expect_solve(B, m)
    assert eng.ctx.last_sample_kernel() == "minsnap_sample_stream_kernel<4, false, false, false>"
    assert eng.take_flags() == [0, 0, 0, 0]
    _sliced(case, eng, pool, wps, plan)
    _ld_errors(case, plan, wps, [0, 1, 4095, 4096, 32767, B - 2, B - 1])


# ------------------------------------------------------------------------------------------------------- C: solve forms x m
C_MS = [1, 2, 3, 4, 5, 6, 7, 11, 12, 13, 15, 20, 33, 63, 64]


def _ragged_of(wps, seed):
    """Ragged batch of the same missions cut to lengths 1 .. m (every length present)."""
    rng = np.random.default_rng(seed)
    m = wps.shape[1] - 1
    lens = rng.integers(1, m + 1, len(wps))
    lens[:m] = np.arange(1, m + 1)
    missions = [w[:n + 1] for w, n in zip(wps, lens)]
    so = np.zeros(len(wps) + 1, np.int64)
    np.cumsum(lens, out=so[1:])
    return missions, so, np.concatenate(missions)


@pytest.mark.parametrize("m", C_MS)
def test_solve_forms_every_mission(eng, pool, m):
    """Every solve form at this m against the oracle, every mission: two-ended x lanes {64, 32, 16} x park {0, 1} x keep {0, 1},
    one-ended x lanes x keep, ragged batches of lengths 1 .. m through both orders.  Where parking in LDS does not fit, the
    name shows the launch stayed in HBM.  Rows of the default sampler once per m."""
    from oracle import c_oracle as cc
    from oracle import minsnap_oracle as mo
    B = 1001 if m <= 20 else 203
    wps = mo.synthetic_missions(B, m)
    missions, so, flat = _ragged_of(wps, 100 + m)
    fut = pool.submit(cc.plan_threads, wps, VEL, DT)
    fut_r = pool.submit(cc.plan_threads, flat, VEL, DT, 0, B, so, False)
    case = f"C m={m}"
    ref = fut.result()
    names, unfit = set(), set()
    for order, lanes, park, keep in ([(1, ln, pk, kp) for ln in (64, 32, 16) for pk in (0, 1) for kp in (0, 1)] +
                                     [(0, ln, -1, kp) for ln in (64, 32, 16) for kp in (0, 1)]):
        with _opts(eng, solve_order=order, solve_lanes=lanes, solve_park=park, solve_keep=keep):
            plan = eng.plan(wps, VEL, DT, rows=False)
            name = eng.ctx.last_solve_kernel()
        want = _expect_solve(B, m, order, lanes, park, keep)
        assert name == want, (case, order, lanes, park, keep, name, want)
        args = name[name.index("<") + 1:-1].split(", ")
        if park == 1 and order == 1 and m > 2:
            nm = {64: 32, 32: 16, 16: 8}[lanes]
            fits = (m - 1) // 2 * 28 * 2 * nm * 8 + 8 * 64 * 28 + 12 <= 150 * 1024
            assert args[1] == _tf(fits), name                      # where the parked blocks do not fit LDS the launch stays in HBM
            if not fits:
                assert args[3] == ("5" if keep == 1 else "0"), name
                unfit.add(name)
        names.add(name)
        _check_solve(case, eng, plan, ref)
    plan = eng.plan(wps, VEL, DT)
    assert eng.ctx.last_solve_kernel() == _expect_solve(B, m)
    _check_rows(case, eng, plan.traj, ref["rows"], ref["row_offsets"])
    ref_r = fut_r.result()
    ref_r["seg_offsets"] = so
    for order in (1, 0):
        with _opts(eng, solve_order=order):
            rb = eng.plan_ragged(missions, VEL, DT, rows=False)
            name = eng.ctx.last_solve_kernel()
        assert name == _expect_solve(B, m, order, ragged=True), (case, order, name)
        names.add(name)
        _check_solve(case + " ragged", eng, rb, ref_r, ragged=True)
    assert len(names) >= 3
    assert bool(unfit) == (m >= 33), unfit                         # (64 lanes of a wave cannot park from m = 33 on)


def test_solve_default_dispatch_at_the_chip_thresholds(eng, pool):
    """The default dispatch where its choices flip, every mission against the oracle: B = 32 S - 1 / 32 S (S = SIMDs of the chip:
    keep off / on at m = 12), B = 16 S / 16 S + 1 (16 -> 32 missions per wave), and solve_order = -1 at B = 48 S -+ 1, m = 8
    (two-ended below, one-ended from there on)."""
    from oracle import c_oracle as cc
    from oracle import minsnap_oracle as mo
    S = _simds()
    sets = {12: mo.synthetic_missions(32 * S, 12), 8: mo.synthetic_missions(48 * S + 1, 8)}
    futs = {m: pool.submit(cc.plan_threads, w, VEL, DT, 0, len(w), None, False) for m, w in sets.items()}
    seen = set()
    for m, B, order in ((12, 32 * S - 1, 1), (12, 32 * S, 1), (12, 16 * S, 1), (12, 16 * S + 1, 1), (8, 48 * S - 1, -1), (8, 48 * S + 1, -1)):
        with _opts(eng, solve_order=order):
            plan = eng.plan(sets[m][:B], VEL, DT, rows=False)
            name = eng.ctx.last_solve_kernel()
        assert name == _expect_solve(B, m, order), (B, m, order, name)
        seen.add(name)
        ref = futs[m].result()
        sub = {k: ref[k][:B] for k in ("times", "seg_rows", "coeffs", "first_yaw")}
        _check_solve(f"C dispatch m={m}", eng, plan, sub)
    assert "minsnap_solve_tw_kernel<false, false, 32, 5>" in seen and any(n.startswith("minsnap_solve_bt_kernel") for n in seen)
    assert any(", 16, 0>" in n for n in seen) and any("<false, false, 32, 0>" in n for n in seen)


# ------------------------------------------------------------------------------------------------------- D: sampler forms
def _stress_missions(seed):
    """Vertical first legs and vertical legs mid-mission (no heading for several 64-row chunks), circles whose heading winds many
    times, one- and two-row missions: (name, wps, velocity)."""
    from oracle import minsnap_oracle as mo
    rng = np.random.default_rng(seed)
    climb = []
    for i in range(48):
        h = rng.uniform(4.0, 10.0)
        p0 = np.array([rng.uniform(0, 5), rng.uniform(0, 5), -1.0])
        legs = np.cumsum(rng.uniform(-3, 3, (5, 3)) * np.array([1, 1, 0.1]), axis=0)
        w = np.vstack([p0, p0 + [0, 0, -h], p0 + [0, 0, -h] + legs])
        if i % 2:                                                # the vertical leg in mid-mission instead
            w = np.vstack([w[0], w[0] + legs[0], w[0] + legs[0] + [0, 0, -h], w[0] + legs[0] + [0, 0, -h] + legs[1:5] - legs[0]])
        climb.append(w)
    circ = []
    for i in range(48):
        th = (1 if i % 2 else -1) * np.linspace(0, 9 * np.pi, 25) + rng.uniform(0, TWO_PI)
        rad = rng.uniform(1.5, 4.0)
        circ.append(np.stack([10 + rad * np.cos(th), 10 + rad * np.sin(th), -3 + 0.1 * np.sin(3 * th)], axis=1))
    tiny = mo.synthetic_missions(160, 2) * 0.004                 # legs of ~1 cm: one or two rows per spline
    return [("8d", mo.synthetic_missions(256, 12), VEL), ("climb", np.stack(climb), 1.0), ("circle", np.stack(circ), 2.0),
            ("tiny", tiny, VEL)]


D_DTS = (0.005, 0.01, 0.02)


@pytest.fixture(scope="module")
def stress(pool):
    from oracle import c_oracle as cc
    out = []
    for name, wps, v in _stress_missions(31):
        for dt in D_DTS:
            out.append((f"{name} dt={dt}", wps, v, dt, pool.submit(cc.plan_threads, wps, v, dt, 0, len(wps), None, True, True)))
    return out


def test_sampler_waves_and_groups_every_row(eng, stress):
    """sampler_waves {1, 2, 4, 8, 16} x sampler_group {1, 3, 64} on the 8(d) draw and the stress mix at dt 0.005 / 0.01 / 0.02:
    every row against the oracle.  At m = 12, W = 16 a group of 64 does not fit LDS: the launch shows the group it shrank to."""
    for label, wps, v, dt, fut in stress:
        ref = fut.result()
        for W in (1, 2, 4, 8, 16):
            for G in ((1,) if W == 1 else (1, 3, 64)):
                with _opts(eng, sampler_waves=W, sampler_group=G):
                    plan = eng.plan(wps, v, dt)
                    name, shape = eng.ctx.last_sample_kernel(), eng.ctx.last_sample_launch()
                if W == 1:
                    assert name == "minsnap_sample_kernel<false, false, 8>", name
                else:
                    assert name == f"minsnap_sample_stream_kernel<{W}, false, false, false>", name
                    assert shape["threads"] == 64 * W and 1 <= shape["group"] <= G and shape["lds"] <= 150 * 1024
                    assert shape["group"] == _stream_group(W, G, wps.shape[1] - 1), shape
                    assert shape["grid"] == -(-len(wps) // shape["group"])
                assert eng.take_flags() == [0, 0, 0, 0]
                case = f"D sampler {label}"
                assert np.array_equal(plan.row_offsets.cpu().numpy(), ref["row_offsets"])
                _check_solve(case, eng, plan, ref)
                _check_rows(case, eng, plan.traj, ref["rows"], ref["row_offsets"])


def _stream_group(W, G, m):
    """Missions per workgroup of the streaming sampler: the group asked for, shrunk until its LDS fits 150 KB (launch_stream)."""
    def lds(g):
        return 8 * (W * 704 + g * 24 * m) + 4 * g * ((m + 3) & ~1) + 8 * (2 * g + 1) + 8 * g + 4 * 2 * g
    while G > 1 and lds(G) > 150 * 1024:
        G -= 1
    return G


def test_sampler_group_shrinks_to_fit_lds_at_m64(eng, pool):
    """m = 64, 16 waves, a group of 64 missions asked for: the group shrinks until the workgroup's LDS fits, every row against
    the oracle."""
    from oracle import c_oracle as cc
    from oracle import minsnap_oracle as mo
    wps = mo.synthetic_missions(150, 64)
    fut = pool.submit(cc.plan_threads, wps, VEL, DT)
    for W, G in ((16, 64), (8, 64), (2, 3)):
        with _opts(eng, sampler_waves=W, sampler_group=G):
            plan = eng.plan(wps, VEL, DT)
            name, shape = eng.ctx.last_sample_kernel(), eng.ctx.last_sample_launch()
        assert name == f"minsnap_sample_stream_kernel<{W}, false, false, false>", name
        want = _stream_group(W, G, 64)
        assert shape["group"] == want and shape["grid"] == -(-150 // want) and shape["lds"] <= 150 * 1024, (W, G, shape)
        if G == 64:
            assert want < G, want
        ref = fut.result()
        _check_solve(f"D group m=64 W={W}", eng, plan, ref)
        _check_rows(f"D group m=64 W={W}", eng, plan.traj, ref["rows"], ref["row_offsets"])


def test_sampler_all_sixteen_address_phases(eng, stress):
    """The chunk grid follows the row buffer's address (16 phases of a 128-byte line): the rows written at offsets 0 .. 15
    doubles into a sentinel-filled buffer, every phase reached, every row against the oracle, nothing outside the rows touched."""
    import torch
    label, wps, v, dt, fut = stress[1]                             # the 8(d) draw at dt = 0.01
    ref = fut.result()
    plan = eng.plan(wps, v, dt)
    N = plan.total_rows
    big = torch.full((N * 11 + 64,), SENTINEL, dtype=torch.float64, device=eng.device)
    base = (16 - (big.data_ptr() >> 3) % 16) % 16                  # first element on a 128-byte line
    phases = set()
    for off in range(16):
        big.fill_(SENTINEL)
        s = base + off
        plan.traj = big[s:s + N * 11].view(N, 11)
        eng.sample(plan)
        assert eng.ctx.last_sample_kernel() == "minsnap_sample_stream_kernel<4, false, false, false>"
        phases.add(eng.ctx.last_sample_launch()["phase"])
        assert bool((big[:s] == SENTINEL).all()) and bool((big[s + N * 11:] == SENTINEL).all()), off
        _check_rows(f"D phases {label}", eng, plan.traj, ref["rows"], ref["row_offsets"])
    assert len(phases) == 16, sorted(phases)


def test_sampler_dense_yaw_column_forms(eng, stress):
    """The one-wave sampler with the dense yaw column: 1, 4, 8 and 16 chunks per store (minsnap_sample_kernel<false, false, 1 | 4 |
    8 | 16> -- three of them ran in no test before), rows and column against the oracle; the column equals the rows' yaw."""
    import torch
    seen = set()
    for label, wps, v, dt, fut in stress:
        ref = fut.result()
        for yg in (1, 4, 8, 16):
            with _opts(eng, sampler_waves=1, yaw_group=yg):
                plan = eng.plan(wps, v, dt, dense_yaw=True)
                name = eng.ctx.last_sample_kernel()
            assert name == f"minsnap_sample_kernel<false, false, {yg}>", name
            seen.add(name)
            assert torch.equal(plan.yaw, plan.traj[:, 9])
            _check_rows(f"D yaw column {label}", eng, plan.traj, ref["rows"], ref["row_offsets"])
    assert len(seen) == 4


def test_sampler_jerk_and_snap(eng, stress):
    """uavac_minsnap_sample_derivs_dev on both sampler forms: jerk and snap of every row against the oracle's (polynom orders 3
    and 4), and the rows it rewrites."""
    import torch
    for label, wps, v, dt, fut in stress:
        ref = fut.result()
        for W in (1, 4):
            with _opts(eng, sampler_waves=W):
                plan = eng.plan(wps, v, dt, dense_yaw=True)
                jerk, snap = eng.sample_derivatives(plan)
                name = eng.ctx.last_sample_kernel()
            assert name == ("minsnap_sample_kernel<false, true, 8>" if W == 1 else "minsnap_sample_stream_kernel<4, false, true, false>"), name
            case = f"D derivs {label}"
            for key, got in (("jerk", jerk), ("snap", snap)):
                r = torch.from_numpy(ref[key]).to(eng.device)
                e = float(((got - r).abs().amax(0) / r.abs().amax(0).clamp_min(1.0)).max())
                _note(case, **{key: e})
                assert e <= TOL, (case, key, e)
            _check_rows(case, eng, plan.traj, ref["rows"], ref["row_offsets"])


def _face_margin(rows, cub):
    """Per row: how far inside (> 0) or outside (< 0) the cuboid, in the face coordinate that decides it."""
    lo = np.stack([rows[:, 0] - cub[0], cub[1] - rows[:, 0], rows[:, 1] - cub[2], cub[3] - rows[:, 1], rows[:, 2] - cub[4], cub[5] - rows[:, 2]], axis=1)
    return lo.min(axis=1)


def test_ragged_hit_flags_against_oracle_rows(eng, pool):
    """Per-spline hit flags of ragged batches (one-wave and streaming samplers) for a few cuboids, against flags recomputed from
    the oracle's rows.  A flag may differ only where the oracle's sample nearest a face lies within 1e-9 of it (counted)."""
    from oracle import c_oracle as cc
    from oracle import minsnap_oracle as mo
    missions, so, flat = _ragged_of(mo.synthetic_missions(700, 9), 7)
    cubs = [np.array([6.0, 14.0, 2.0, 9.0, -4.0, -2.8]), np.array([0.0, 24.0, 0.0, 14.0, -3.0, -3.0 + 1e-12]),
            np.array([10.0, 12.0, 5.0, 7.0, -10.0, 0.0])]
    futs = [pool.submit(cc.plan_threads, flat, VEL, DT, 0, len(missions), so, True, False, c) for c in cubs]
    for c, fut in zip(cubs, futs):
        ref = fut.result()
        assert 0 < ref["hit"].sum() < len(ref["hit"])
        for W in (1, 4):
            with _opts(eng, sampler_waves=W):
                rb = eng.plan_ragged(missions, VEL, DT, cuboid=c)
                name = eng.ctx.last_sample_kernel()
            assert name == ("minsnap_sample_kernel<true, false, 8, true>" if W == 1 else "minsnap_sample_stream_kernel<4, true, false, true>"), name
            case = f"D hits W={W}"
            _check_rows(case, eng, rb.traj, ref["rows"], ref["row_offsets"])
            hit = rb.hit.cpu().numpy()
            bad = np.flatnonzero(hit != ref["hit"])
            rows = ref["rows"]
            seg_ro = np.concatenate([[0], np.cumsum(ref["seg_rows"])])
            for s in bad:
                r = rows[seg_ro[s]:seg_ro[s + 1]]
                near = float(np.abs(_face_margin(r, c)).min())
                assert near <= 1e-9, (case, int(s), int(hit[s]), int(ref["hit"][s]), near)
            FACE_TIES[case] = FACE_TIES.get(case, 0) + len(bad)


# ------------------------------------------------------------------------------------------------------- E: row-count edges
def _edge_missions(dt, n=96):
    """Missions of three legs along x whose durations lie within a few ulps of a whole number of dt -- in the first, the middle
    and the last leg (the first and last take the 1.5 time factor) -- on both sides of it."""
    rng = np.random.default_rng(int(dt * 1e4))
    out = []
    for i in range(n):
        k = rng.integers(100, 200, 3)
        lens = k * dt / np.array([1.5, 1.0, 1.5])                # T = 1.5 L, L, 1.5 L at v = 1
        x = np.concatenate([[rng.uniform(0, 5)], np.zeros(3)])
        for j in range(3):
            x[j + 1] = x[j] + lens[j]
            for _ in range(int(rng.integers(-4, 5))):           # a few ulps either way
                x[j + 1] = np.nextafter(x[j + 1], np.inf if i % 2 else -np.inf)
        w = np.zeros((4, 3))
        w[:, 0], w[:, 1], w[:, 2] = x, 2.0, -3.0
        out.append(w)
    return np.stack(out)


def test_row_counts_at_whole_multiples_of_dt(eng, pool):
    """Row counts of legs whose T / dt lies within a few ulps of an integer equal len(np.arange(0, T, dt)) (oracle_row_count)
    exactly, and the rows agree with the oracle's."""
    from oracle import c_oracle as cc
    near = 0
    for dt in D_DTS:
        wps = _edge_missions(dt)
        ref = cc.plan_threads(wps, 1.0, dt)
        q = ref["times"] / dt
        near += int((np.abs(q - np.round(q)) <= 8 * np.spacing(np.round(q))).sum())
        for t, n in zip(ref["times"].reshape(-1), ref["seg_rows"].reshape(-1)):
            assert n == len(np.arange(0.0, t, dt))
        plan = eng.plan(wps, 1.0, dt)
        _check_solve(f"E dt={dt}", eng, plan, ref)
        assert np.array_equal(plan.row_offsets.cpu().numpy(), ref["row_offsets"])
        _check_rows(f"E dt={dt}", eng, plan.traj, ref["rows"], ref["row_offsets"])
        free = eng.plan(wps, 1.0, dt, rows=False)
        _check_solve(f"E rows-free dt={dt}", eng, free, ref)
    assert near >= 100, near                                      # the cases do sit at the edge


# ------------------------------------------------------------------------------------------------------- F: rows-free, capped
def test_rows_free_first_headings_and_the_row_capacity(eng, pool):
    """plan(rows=False): durations, row counts, coefficients and the first heading of every mission against the oracle.  The
    sampler with a capacity of exactly total_rows accepts; with total_rows - 1 it refuses (flag 2) and the sentinel past the
    buffer is untouched."""
    import torch
    from oracle import c_oracle as cc
    from oracle import minsnap_oracle as mo
    wps = mo.synthetic_missions(4096, 8)
    wps[::16, 1] = wps[::16, 0] + [0.0, 0.0, -5.0]               # every 16th mission climbs first: its first heading comes late
    fut = pool.submit(cc.plan_threads, wps, VEL, DT)
    plan = eng.plan(wps, VEL, DT, rows=False)
    assert plan.traj is None
    ref = fut.result()
    _check_solve("F rows-free", eng, plan, ref)
    N = plan.total_rows
    assert N == ref["row_offsets"][-1]
    big = torch.full((N + 64, 11), SENTINEL, dtype=torch.float64, device=eng.device)
    eng.take_flags()
    full = eng.plan_from_parts(plan.coeffs, plan.times, plan.seg_rows, plan.m, VEL, DT, total_rows=N, traj=big[:N])
    assert eng.take_flags() == [0, 0, 0, 0]
    assert eng.ctx.last_sample_kernel() == "minsnap_sample_stream_kernel<4, false, false, false>"
    _check_rows("F capped", eng, full.traj, ref["rows"], ref["row_offsets"])
    assert bool((big[N:] == SENTINEL).all())
    big.fill_(SENTINEL)
    eng.plan_from_parts(plan.coeffs, plan.times, plan.seg_rows, plan.m, VEL, DT, total_rows=N - 1, traj=big[:N - 1])
    assert eng.take_flags()[2] == 1
    assert bool((big[N - 1:] == SENTINEL).all()), "rows were written past the capacity"
