"""What selecting, reordering and prioritising missions costs (`uavac_minsnap_take_dev`, `uavac_fleet_order_dev`; `Engine.take`, and
`priority=` on `Engine.stagger` / `Engine.layer`), beside the calls that set the scale.  Eight segments (the bench's generator), velocity
3, dt 0.01, radius 0.5, the two shapes the README quotes for the fleet calls:

    65 536 missions in groups of 64        4 096 missions in groups of 256

    take_rate.py [OUT.jsonl] [rounds]            records are APPENDED to OUT.jsonl

Per shape, in one process, warm-up first, the arms interleaved over the rounds, hipEvents around each arm; median, minimum, maximum and
spread per arm, one JSON line per arm with the device's identity:
  * `Engine.take` with a within-group permutation (every group reversed) beside `Engine.shift` on the same plan.  Both read and write
    every coefficient once, so the shift is the yardstick; the take also copies durations, row counts and first headings, scans the
    segment counts and the row counts, and reads the (B + 1,) offsets back -- its one host sync, which the shift does not have.  The
    three launches of the take alone, into buffers allocated outside the timing and without the read, are an arm of their own;
  * `uavac_fleet_order_dev` alone, in the shape's groups and (65 536 only) for ONE group of all missions -- the sum of g^2 at its worst;
  * `Engine.stagger` and `Engine.layer` (delta (0, 0, -0.25), max_steps 63) without a priority and with a random permutation as priority
    on the same plan.  The two searches do different work -- another order is another problem --, so the pair says what the
    composition costs next to a search, not what the order and the take cost exactly: that is the first two items.
Before anything is timed: the taken batch is the plan's missions in the order asked for, bit for bit; the order is the permutation
NumPy gives; priority = arange(B) gives the searches' answers without a priority."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uav-autonomous-control_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bench import missions  # noqa: E402

M, VEL, DT, RADIUS, DELTA, MAX_STEPS = 8, 3.0, 0.01, 0.5, (0.0, 0.0, -0.25), 63
SHAPES = ((65536, 64), (4096, 256))                      # (missions, group size)


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def _p(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def main(out_path, rounds):
    from uav_ac.fleet import Engine
    from uav_ac.scoring import priority_order
    eng = Engine("cuda:0")
    box = eng.ctx.device_identity()
    kw = dict(device=eng.device)
    lines = []
    for B, n in SHAPES:
        plan = eng.plan(missions(B, M, 0, B), VEL, DT, rows=False)
        rng = np.random.default_rng(20261019)
        reverse = np.concatenate([np.arange(g0, min(g0 + n, B))[::-1] for g0 in range(0, B, n)])
        index = torch.as_tensor(reverse.astype(np.int32)).to(eng.device)
        offsets = torch.as_tensor(np.tile(DELTA, (B, 1))).to(eng.device)
        priority_host = rng.permutation(B).astype(np.float64)
        priority = torch.as_tensor(priority_host).to(eng.device)
        go = torch.arange(0, B + 1, n, dtype=torch.int64, **kw)
        one = torch.tensor([0, B], dtype=torch.int64, **kw)
        order, rank = torch.empty((B,), dtype=torch.int32, **kw), torch.empty((B,), dtype=torch.int32, **kw)
        # the buffers of the take's three launches, allocated once
        tail = torch.empty((B + 1,), dtype=torch.int64, **kw)
        co, tm = torch.empty((B * M, 8, 3), dtype=torch.float64, **kw), torch.empty((B * M,), dtype=torch.float64, **kw)
        sr, ro = torch.empty((B * M,), dtype=torch.int32, **kw), torch.empty((B + 1,), dtype=torch.int64, **kw)
        fy = torch.empty((B,), dtype=torch.float64, **kw)

        def take():
            return eng.take(plan, index)

        def take_launches():
            eng._bind_stream()
            eng.ctx.call("uavac_minsnap_take_offsets_dev", None, B, M, _p(index), B, _p(tail))
            eng.ctx.call("uavac_minsnap_take_dev", _p(plan.coeffs), _p(plan.times), _p(plan.seg_rows), None, B, M, _p(plan.first_yaw), _p(index),
                         B, _p(tail), _p(co), _p(tm), _p(sr), _p(fy))
            eng.ctx.call("uavac_minsnap_row_offsets_ragged_dev", _p(sr), _p(tail), B, M, _p(ro))

        def shift():
            return eng.shift(plan, offsets)

        def order_in(groups, G):
            eng._bind_stream()
            eng.ctx.call("uavac_fleet_order_dev", _p(priority), _p(groups), G, B, _p(order), _p(rank))

        # before anything is timed: the take, the order and the identity are right
        at = index.long()
        t = take()
        take_launches()
        torch.cuda.synchronize()
        assert torch.equal(t.coeffs.reshape(B, -1), plan.coeffs.reshape(B, -1)[at]) and torch.equal(t.times.reshape(B, M), plan.times[at])
        assert torch.equal(t.seg_rows.reshape(B, M), plan.seg_rows[at]) and torch.equal(t.first_yaw, plan.first_yaw[at])
        assert torch.equal(co, t.coeffs) and torch.equal(tm, t.times) and torch.equal(sr, t.seg_rows) and torch.equal(ro, t.row_offsets)
        for groups, G in ((go, B // n), (one, 1)):
            order_in(groups, G)
            want = priority_order(priority_host, groups.cpu().numpy())
            assert np.array_equal(order.cpu().numpy(), want[0]) and np.array_equal(rank.cpu().numpy(), want[1])
        ident = torch.arange(B, dtype=torch.float64, **kw)
        stag = eng.stagger(plan, RADIUS, groups=n)
        assert torch.equal(eng.stagger(plan, RADIUS, groups=n, priority=ident).block, stag.block)
        lay = eng.layer(plan, RADIUS, groups=n, delta=DELTA, max_steps=MAX_STEPS)
        assert torch.equal(eng.layer(plan, RADIUS, groups=n, delta=DELTA, max_steps=MAX_STEPS, priority=ident).block, lay.block)
        stag_p = eng.stagger(plan, RADIUS, groups=n, priority=priority)
        lay_p = eng.layer(plan, RADIUS, groups=n, delta=DELTA, max_steps=MAX_STEPS, priority=priority)
        shares = {"stagger": {"unresolved": float((stag.steps == -1).double().mean()), "delayed": float((stag.steps > 0).double().mean())},
                  "stagger, priority": {"unresolved": float((stag_p.steps == -1).double().mean()),
                                        "delayed": float((stag_p.steps > 0).double().mean())},
                  "layer": {"unresolved": float((lay.steps == -1).double().mean()), "layered": float((lay.layers > 0).double().mean())},
                  "layer, priority": {"unresolved": float((lay_p.steps == -1).double().mean()),
                                      "layered": float((lay_p.layers > 0).double().mean())}}
        del t, stag, lay, stag_p, lay_p

        arms = {"Engine.take, every group reversed (three launches, gathers, one host read)": (take, 20, {}),
                "the take's three launches alone, preallocated, no read": (take_launches, 50, {}),
                "Engine.shift on the same plan (the yardstick: every coefficient read and written once)": (shift, 50, {}),
                f"uavac_fleet_order_dev alone, groups of {n}": (lambda: order_in(go, B // n), 50, {"sum of g^2": (B // n) * n * n}),
                "Engine.stagger": (lambda: eng.stagger(plan, RADIUS, groups=n), 1, shares["stagger"]),
                "Engine.stagger, priority = a random permutation": (lambda: eng.stagger(plan, RADIUS, groups=n, priority=priority), 1,
                                                                    shares["stagger, priority"]),
                "Engine.layer": (lambda: eng.layer(plan, RADIUS, groups=n, delta=DELTA, max_steps=MAX_STEPS), 1, shares["layer"]),
                "Engine.layer, priority = a random permutation": (lambda: eng.layer(plan, RADIUS, groups=n, delta=DELTA, max_steps=MAX_STEPS,
                                                                                    priority=priority), 1, shares["layer, priority"])}
        if B == 65536:
            arms[f"uavac_fleet_order_dev alone, ONE group of {B}"] = (lambda: order_in(one, 1), 3, {"sum of g^2": B * B})
        for fn, _, _ in arms.values():                   # warm-up of every arm
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in arms}
        for _ in range(rounds):
            for name, (fn, reps, _) in arms.items():
                times[name].append(timed(fn, reps))
        for name, ts in times.items():
            med = float(np.median(ts))
            line = {"arm": name, "B": B, "group": n, "m": M, "median_ms": round(med, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
                    "spread (max - min) / median": round((max(ts) - min(ts)) / med, 4), "rounds": rounds, "reps_per_round": arms[name][1],
                    "missions_per_s": B / (med * 1e-3), **arms[name][2], "box": box}
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
        del plan, arms, co, tm, sr, ro, fy, tail
        torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None, help="the jsonl file the records are appended to")
    ap.add_argument("rounds", nargs="?", type=int, default=5)
    ap.add_argument("--shapes", default=None, help="B:group[,B:group...] instead of the two shapes above (a rehearsal at a small size)")
    args = ap.parse_args()
    if args.shapes:
        SHAPES = tuple(tuple(int(v) for v in pair.split(":")) for pair in args.shapes.split(","))
    main(args.out, args.rounds)
