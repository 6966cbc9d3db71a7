"""The plan audit (`uavac_minsnap_audit_dev`) against what it took before it existed to learn the same things about a rows-free plan:
sample its rows, run one hit-sampler pass per cuboid, reduce.  B = 65 536 missions of 8 segments (the bench's generator),
velocity 3, dt 0.01, the four cuboids of the laboratory course.  hipEvents around batches of launches, warm-up first, the arms
interleaved over rounds in one process; median and minimum per arm, one JSON line per arm.

    plan_audit_rate.py [OUT.jsonl] [rounds]

The row path is the one a caller of the previous release had: `uavac_minsnap_sample_capped_dev` into a row buffer (allocated once,
outside the timing), `uavac_minsnap_sample_hits_dev` once per cuboid (each writes all rows again and a flag per spline), then torch
reductions over the rows: the seven peaks per mission (scatter-max over a row -> mission index that is built once, outside the timing)
and the hit flags per mission.  It yields flags, not counts or first indices: the audit's answers are a superset.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uav-autonomous-control_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bench import missions  # noqa: E402
from uav_ac.engine import _ptr  # noqa: E402
from uav_ac.fleet import Engine  # noqa: E402

LAB_AABBS = np.array([[3.7, 4.3, 4.0, 10.0, -3.4, -2.8], [10.7, 11.3, 4.0, 10.0, -2.2, 0.0], [13.3, 14.7, 6.3, 7.7, -6.0, 0.0],
                      [20.2, 20.8, 4.0, 10.0, -3.3, -2.7]])
B, M, VEL, DT = 65536, 8, 3.0, 0.01


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    eng = Engine("cuda:0")
    dev = eng.device
    wps = missions(B, M, 0, B)
    plan = eng.plan(wps, VEL, DT)                     # with a row buffer: the row path samples into it
    free = eng.plan(wps, VEL, DT, rows=False)
    cubs = torch.as_tensor(LAB_AABBS).to(dev)
    N = plan.total_rows
    lengths = plan.row_offsets[1:] - plan.row_offsets[:-1]
    mission_of_row = torch.repeat_interleave(torch.arange(B, device=dev), lengths)[:, None].expand(N, 7).contiguous()
    hit = torch.empty((LAB_AABBS.shape[0], B, M), dtype=torch.int32, device=dev)
    peaks = torch.empty((B, 7), dtype=torch.float64, device=dev)

    def rows_path():
        eng.sample(plan)
        for c in range(cubs.shape[0]):
            eng.ctx.call("uavac_minsnap_sample_hits_dev", _ptr(plan.coeffs), None, _ptr(plan.seg_rows), _ptr(plan.row_offsets), B, M, DT,
                         _ptr(plan.traj), _ptr(cubs[c]), _ptr(hit[c]))
        t = plan.traj
        v2 = t[:, 3] * t[:, 3] + t[:, 4] * t[:, 4]
        src = torch.stack([v2, -t[:, 5], t[:, 5], t[:, 6] * t[:, 6] + t[:, 7] * t[:, 7], -t[:, 8], t[:, 8], v2 + t[:, 5] * t[:, 5]], dim=1)
        peaks.fill_(float("-inf"))
        peaks.scatter_reduce_(0, mission_of_row, src, "amax", include_self=True)
        peaks[:, [0, 3, 6]] = torch.sqrt(peaks[:, [0, 3, 6]])
        return peaks, hit.amax(dim=2)

    arms = {}
    for lanes in (16, 64):
        for n in (4, 0):
            def audit(lanes=lanes, n=n):
                eng.ctx.set_option("audit_lanes", lanes)
                return eng.audit(free, cubs if n else None)
            arms[f"audit lanes={lanes} cuboids={n}"] = (audit, 20)
    arms["rows path: sample + 4 hit passes + reductions"] = (rows_path, 3)
    arms["rows path, sampler only"] = (lambda: eng.sample(plan), 10)

    # the two paths agree before anything is timed (peaks exactly, hit flags as "any sample inside")
    eng.ctx.set_option("audit_lanes", 16)
    a = eng.audit(free, cubs)
    p, h = rows_path()
    torch.cuda.synchronize()
    got = torch.stack([a.speed_xy, a.ascent, a.descent, a.accel_xy, a.accel_up, a.accel_down, a.speed], dim=1)
    agree = {"peaks_differ": int((got != p).sum()), "hit_flags_differ": int(((a.hit_rows > 0) != (h > 0)).sum()),
             "row_totals_differ": int((a.rows.to(torch.int64) != lengths).sum())}
    print(json.dumps({"agreement of the two paths (elements that differ)": agree}), flush=True)
    for fn, _ in arms.values():                       # warm-up of every arm
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, (fn, reps) in arms.items():
            times[k].append(timed(fn, reps))
    eng.ctx.set_option("audit_lanes", 16)
    box = eng.ctx.device_identity()
    lines = []
    for k, ts in times.items():
        lines.append(json.dumps({"arm": k, "B": B, "m": M, "rows": int(N), "median_ms": round(float(np.median(ts)), 4),
                                 "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "rounds": rounds, "box": box}))
        print(lines[-1], flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
