"""The retiming loop (`Engine.retime`, `uavac_minsnap_retime_dev`) on the bench distribution: B = 65 536 missions of 12 segments
(the bench's generator), velocity 3, dt 0.01, the default vehicle's flight limits, margin 1e-3.  What it costs -- missions/s, passes,
and how much of a pass is the rows-free chain and how much the audit -- and what it buys: the retimed and the un-retimed plan are
both flown to the end with score=True and their tracking scores reported side by side.

    retime_rate.py [OUT.jsonl] [rounds] [B] [m]

Timing: the loop synchronises once per pass, so it is timed with the host clock around calls that end in a device synchronise;
its parts (the rows-free chain at per-mission speeds, the audit, the factors kernel) with hipEvents around batches of launches.
Warm-up first, the arms interleaved over rounds in one process; median and minimum per arm, one JSON line per arm.
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uav-autonomous-control_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bench import missions  # noqa: E402
from uav_ac import _native as nat  # noqa: E402
from uav_ac.engine import _ptr  # noqa: E402
from uav_ac.fleet import Engine  # noqa: E402
from uav_ac.scoring import acceptance, plan_feasibility  # noqa: E402

VEL, DT, MARGIN, MAX_PASSES = 3.0, 0.01, 1e-3, 4


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fly(eng, plan, chunk=4000):
    """The whole plan flown plan-fed with score=True -> the tracking summary (host floats)."""
    fleet = eng.fleet(plan, from_plan=True)
    rows = int((plan.row_offsets[1:] - plan.row_offsets[:-1]).max().item())
    ticks = (rows + 2) * int(fleet.vehicle.inner_per_outer)
    for _ in range((ticks + chunk - 1) // chunk):
        fleet.rollout(chunk, score=True)
    s = fleet.tracking()
    acc = acceptance(s)
    f = lambda t: float(t[~torch.isnan(t)].mean().item())          # noqa: E731
    return {"ticks": ((ticks + chunk - 1) // chunk) * chunk, "complete": int(s["complete"].sum().item()),
            "mean_error_mean": f(s["mean_error"]), "mean_error_worst": float(s["mean_error"].nan_to_num(0).max().item()),
            "max_error_mean": f(s["max_error"]), "max_error_worst": float(s["max_error"].nan_to_num(0).max().item()),
            "final_error_mean": f(s["final_error"]), "passed": int(acc["passed"].sum().item())}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 65536
    M = int(sys.argv[4]) if len(sys.argv) > 4 else 12
    eng = Engine("cuda:0")
    wps = missions(B, M, 0, B)
    free = eng.plan(wps, VEL, DT, rows=False)
    res = eng.retime(free, margin=MARGIN, max_passes=MAX_PASSES)
    torch.cuda.synchronize()
    before, after = plan_feasibility(eng.audit(free)), plan_feasibility(res.audit)
    lim = torch.tensor([3.0, 3.0, 2.0, 12.0], device=eng.device)[:, None]
    ratio = (res.audit.block[1:5] / lim).amax(dim=0)
    outcome = {"B": B, "m": M, "passes": res.passes, "converged": int(res.converged.sum().item()),
               "feasible_before": int(before["feasible"].sum().item()), "feasible_after": int(after["feasible"].sum().item()),
               "factor_min": float(res.factors.min().item()), "factor_median": float(res.factors.median().item()),
               "factor_max": float(res.factors.max().item()), "worst_peak_over_limit_after": float(ratio.max().item()),
               "rows_before": int(free.total_rows), "rows_after": int(res.plan.total_rows), "flags": eng.take_flags()}
    print(json.dumps({"outcome": outcome}), flush=True)

    # the parts of a pass, on buffers of their own
    mixed = eng.plan(wps, res.velocities, DT, rows=False)
    block = torch.empty((nat.AUDIT_ROWS, B), dtype=torch.float64, device=eng.device)
    vel, fac = res.velocities.clone(), torch.empty((B,), dtype=torch.float64, device=eng.device)
    cnt = torch.zeros((2,), dtype=torch.int32, device=eng.device)
    limits = (C.c_double * 4)(3.0, 3.0, 2.0, 12.0)

    def audit():
        eng.ctx.call("uavac_minsnap_audit_dev", _ptr(mixed.coeffs), _ptr(mixed.seg_rows), None, B, M, DT, None, 0, _ptr(block), None, None)

    def factors():
        eng.ctx.call("uavac_minsnap_retime_factors_dev", _ptr(block), B, limits, MARGIN, _ptr(vel), _ptr(fac), _ptr(cnt))

    arms = {"rows-free chain at per-mission speeds": (lambda: eng.replan(mixed), 20),
            "rows-free chain at one speed": (lambda: eng.replan(free), 20),
            "audit, no cuboids": (audit, 20),
            "factors kernel": (factors, 50)}
    eng._bind_stream()
    for fn, _ in arms.values():
        fn()
    for _ in range(2):
        eng.retime(free, margin=MARGIN, max_passes=MAX_PASSES)
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    loop, audit_only = [], []
    for _ in range(rounds):
        for k, (fn, reps) in arms.items():
            times[k].append(timed(fn, reps))
        loop.append(wall(lambda: eng.retime(free, margin=MARGIN, max_passes=MAX_PASSES))[0])
        audit_only.append(wall(lambda: eng.retime(free, margin=MARGIN, max_passes=0))[0])
    times["Engine.retime, max_passes=4 (host clock, allocations and syncs included)"] = loop
    times["Engine.retime, max_passes=0 (one pass: audit only)"] = audit_only
    box = eng.ctx.device_identity()
    lines = [json.dumps({"outcome": outcome})]
    med = {k: float(np.median(ts)) for k, ts in times.items()}
    for k, ts in times.items():
        lines.append(json.dumps({"arm": k, "B": B, "m": M, "median_ms": round(med[k], 4), "min_ms": round(min(ts), 4),
                                 "max_ms": round(max(ts), 4), "rounds": rounds, "box": box}))
        print(lines[-1], flush=True)
    n_pass = res.passes + 1                                           # the pass after the last retiming judges only
    loop_ms = med["Engine.retime, max_passes=4 (host clock, allocations and syncs included)"]
    shares = {"missions_per_s": round(B / (loop_ms * 1e-3)), "passes_run": n_pass,
              "chain_share": round(n_pass * med["rows-free chain at per-mission speeds"] / loop_ms, 3),
              "audit_share": round(n_pass * med["audit, no cuboids"] / loop_ms, 3),
              "factors_share": round(n_pass * med["factors kernel"] / loop_ms, 4)}
    lines.append(json.dumps({"loop": shares}))
    print(lines[-1], flush=True)

    # what it buys: both plans flown to the end, scored
    flights = {"un-retimed (3 m/s)": fly(eng, free), "retimed": fly(eng, res.plan)}
    lines.append(json.dumps({"tracking": flights}))
    print(lines[-1], flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
