"""The prioritised searches per independent airspace (`Engine.stagger / layer(..., airspaces=True)`: `uavac_minsnap_envelope_dev`,
`uavac_fleet_airspaces_dev`, order, take, the unchanged search on the airspace offsets) against the only route to the same answers that
existed before: ONE group of all missions with `wide=True`.  Eight segments (the bench's generator), velocity 3, dt 0.01, radius 0.5,
starts 0; stagger with step 1 and max_steps 255, layer with delta (0, 0, -0.25) and max_steps 63 -- the settings of tools/wide_rate.py.
The missions are spread by `wps[:, :, :2] += (spread - 1) * wps[:, :1, :2]`: every mission moved away from the origin in x and y,
its first waypoint times `spread`.  Shapes (missions : spread):

    4 096 : 1     one airspace: the feature cannot help, its cost is pure overhead
    4 096 : 30    the largest airspace above 256 (the block-wise search with group_cap = that size)        65 536 : 128   likewise
    4 096 : 40    the largest airspace below 256 (the narrow search)                                       65 536 : 160   likewise

    airspaces_rate.py [OUT.jsonl] [rounds] [--shapes B:spread,...] [--searches stagger,layer] [--reference-rounds N] [--no-reference]

Both routes must give the SAME start rows and steps (stagger), layers, steps and blocked counts (layer) for every mission before
anything is timed.  hipEvents around each arm, warm-up first, the arms interleaved over rounds in one process; median, minimum and
maximum per arm, one JSON line per arm with the device's identity, the number of airspaces, the largest one and the labelling rounds.
The reference point is the one-group wide call, never the new code itself; no ratio is fixed anywhere.  The parts of the new route
are reported separately: the boxes, the labelling, order plus take (with its host read), and the search on the taken plan; and the
whole call, which also pays the labelling's host read and the gathers back.  `--reference-rounds`: fewer rounds for the one-group
call, which at 65 536 missions takes minutes (0: assert against it once and time it in that one run, without a warm-up);
`--no-reference`: the new route alone, where the one-group call does not fit the time at hand -- nothing is compared then, and every
record of such a run says so."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uav-autonomous-control_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bench import missions  # noqa: E402

M, VEL, DT, RADIUS = 8, 3.0, 0.01, 0.5
STAGGER = dict(step=1, max_steps=255)
LAYER = dict(delta=(0.0, 0.0, -0.25), max_steps=63)
SHAPES = ((4096, 1.0), (4096, 30.0), (4096, 40.0), (65536, 128.0), (65536, 160.0))      # (missions, spread)
ROUNDS_PER_CALL = 32


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def spread_missions(B, spread):
    wps = missions(B, M, 0, B)
    wps[:, :, :2] += (spread - 1.0) * wps[:, :1, :2]
    return wps


def main(out_path, rounds, searches, reference_rounds, with_reference=True):
    from uav_ac.engine import _ptr
    from uav_ac.fleet import Engine
    eng = Engine("cuda:0")
    box = eng.ctx.device_identity()
    lines = []
    for B, spread in SHAPES:
        plan = eng.plan(spread_missions(B, spread), VEL, DT, rows=False)
        for kind in searches:
            reach = None if kind == "stagger" else eng._layer_reach(LAYER["delta"], LAYER["max_steps"])
            rows = [0, 1] if kind == "stagger" else [0, 1, 3]            # start rows and steps; layers, steps and blocked

            def search(p=plan, **kw):
                return eng.stagger(p, RADIUS, **STAGGER, **kw) if kind == "stagger" else eng.layer(p, RADIUS, **LAYER, **kw)

            def answers(res):
                block = res.block
                if block.shape[0] == 3 and kind == "layer":                 # (the narrow search without obstacles: nothing is blocked)
                    block = torch.cat([block, torch.zeros_like(block[:1])])
                return block[rows]

            # the same answers from both routes before anything is timed (at --reference-rounds 0 this run is the reference's time)
            split = answers(search(airspaces=True))
            if with_reference:
                got = {}
                first_reference = timed(lambda: got.update(whole=search(wide=True)))
                whole = answers(got.pop("whole"))
            else:                                            # (--no-reference: nothing to compare with, and the records say so)
                whole, reference_rounds = split, -1
            torch.cuda.synchronize()
            differ = int((whole != split).any(dim=0).sum())
            asp = eng.airspaces(plan, RADIUS, reach=reach, rounds=ROUNDS_PER_CALL)
            taken = eng.take(plan, asp.order)
            wide_route = asp.largest > eng.NARROW_SEARCH
            route = dict(groups=asp.offsets, wide=wide_route, group_cap=asp.largest if wide_route else None)
            share = {"airspaces": int(len(asp.sizes_host)), "largest airspace": int(asp.largest), "singletons": int((asp.sizes_host == 1).sum()),
                     "labelling rounds that changed a label": int(asp.rounds), "search per airspace": "block-wise" if wide_route else "narrow",
                     "moved": float((whole[1] > 0).double().mean()), "unresolved": float((whole[1] == -1).double().mean()),
                     "missions that differ between the two routes": differ if with_reference else "not compared: no reference run"}
            print(json.dumps({"B": B, "spread": spread, "search": kind, **share}), flush=True)
            assert differ == 0, differ

            env = eng.envelope(plan, reach)
            labels = torch.empty((B,), dtype=torch.int32, device=eng.device)
            info = torch.empty((2,), dtype=torch.int32, device=eng.device)

            def labelling():
                eng._bind_stream()
                eng.ctx.call("uavac_fleet_airspaces_dev", _ptr(env.block), None, 0, B, RADIUS, ROUNDS_PER_CALL, 0, _ptr(labels), _ptr(info))

            def order_take():
                keys = asp.labels.to(torch.float64)
                order, rank = torch.empty_like(asp.order), torch.empty_like(asp.rank)
                eng._bind_stream()
                eng.ctx.call("uavac_fleet_order_dev", _ptr(keys), None, 0, B, _ptr(order), _ptr(rank))
                return eng.take(plan, order)

            arms = {"the boxes (uavac_minsnap_envelope_dev)": lambda: eng.envelope(plan, reach),
                    f"the labelling ({ROUNDS_PER_CALL} rounds enqueued, uavac_fleet_airspaces_dev)": labelling,
                    "order + take (uavac_fleet_order_dev, Engine.take with its host read)": order_take,
                    "the search on the taken plan, per airspace": lambda: search(taken, **route),
                    f"Engine.{kind}(airspaces=True), the whole call": lambda: search(airspaces=True)}
            reference = f"REFERENCE: Engine.{kind}(wide=True), one group of all missions"
            if reference_rounds > 0:
                arms[reference] = lambda: search(wide=True)
            for fn in arms.values():                         # warm-up of every arm
                fn()
            torch.cuda.synchronize()
            times = {name: [] for name in arms}
            for rnd in range(rounds):
                for name in (list(arms) if rnd % 2 == 0 else list(arms)[::-1]):
                    if name != reference or rnd < reference_rounds:
                        times[name].append(timed(arms[name]))
            if reference_rounds == 0:
                times[reference] = [first_reference]
            for name, ts in times.items():
                med = float(np.median(ts))
                line = {"arm": name, "search": kind, "B": B, "spread": spread, "m": M, "radius": RADIUS,
                        **(STAGGER if kind == "stagger" else {"delta": list(LAYER["delta"]), "max_steps": LAYER["max_steps"]}),
                        "ms_per_round": [round(t, 3) for t in ts], "median_ms": round(med, 3), "min_ms": round(min(ts), 3),
                        "max_ms": round(max(ts), 3), "rounds": len(ts), "warmed up": reference_rounds != 0 or name != reference, **share,
                        "box": box}
                lines.append(json.dumps(line))
                print(lines[-1], flush=True)
            del asp, taken, env, arms
        del plan
        torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None, help="the jsonl file (appended to: the shapes are measured in several runs)")
    ap.add_argument("rounds", nargs="?", type=int, default=5)
    ap.add_argument("--shapes", default=None, help="B:spread[,B:spread...] instead of the five shapes above")
    ap.add_argument("--searches", default="stagger,layer")
    ap.add_argument("--reference-rounds", type=int, default=None, help="rounds of the one-group call (default: as many as the others)")
    ap.add_argument("--no-reference", action="store_true", help="the new route alone: nothing is compared, and the records say so")
    args = ap.parse_args()
    if args.shapes:
        SHAPES = tuple((int(b), float(s)) for b, s in (pair.split(":") for pair in args.shapes.split(",")))
    main(args.out, args.rounds, args.searches.split(","), args.rounds if args.reference_rounds is None else args.reference_rounds,
         with_reference=not args.no_reference)
