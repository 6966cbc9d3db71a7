"""Deconfliction against committed traffic that never moves (`uavac_minsnap_stagger_against_dev`, `uavac_minsnap_layer_against_dev`,
`uavac_minsnap_separation_against_dev`; `Engine.stagger / layer(..., traffic=)`, `Engine.separation_against`) beside the only route there
was before: `wide=True` on `Engine.concat([committed, arrivals])`, interleaved per group, with the same groups -- which re-decides
everybody.  The bench's missions, 8 segments, velocity 3, dt 0.01, radius 0.5, starts 0; stagger with step 1 and max_steps 255, layers
of 0.25 m with max_steps 63.  Two shapes, 64 groups each:

    61 440 committed in groups of 960, 4 096 arrivals, 64 per group          the shape the feature is for
    4 096 committed, 64 per group, 61 440 arrivals in groups of 960          the other way round: where it should not pay

    against_rate.py [OUT.jsonl] [rounds] [--shapes committed:per_group:arrivals:per_group,...]

The two routes answer DIFFERENT questions -- the re-run may delay or move committed missions --, so only times are compared, and the
record says how many committed missions the re-run moved.  What is asserted before anything is timed: the cross audit at the granted
starts finds no traffic mission inside the radius of a resolved arrival.  hipEvents around each arm, warm-up first, the arms interleaved
over rounds in one process; median, minimum and maximum per arm, one JSON line per arm with the device's identity."""
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
SHAPES = ((61440, 960, 4096, 64), (4096, 64, 61440, 960))      # (committed, per group, arrivals, per group)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def main(out_path, rounds):
    from uav_ac.fleet import Engine
    eng = Engine("cuda:0")
    box = eng.ctx.device_identity()
    lines = []
    for Bt, nt, B, n in SHAPES:
        G = Bt // nt
        assert G * nt == Bt and G * n == B, "whole groups on both sides, as many on each"
        everybody = eng.plan(missions(Bt + B, M, 0, Bt + B), VEL, DT, rows=False)
        # group g of the fleet: nt committed missions, then n arrivals
        at = np.arange(Bt + B).reshape(G, nt + n)
        committed, arrivals = eng.take(everybody, at[:, :nt].reshape(-1)), eng.take(everybody, at[:, nt:].reshape(-1))
        whole = eng.concat([committed, arrivals])
        index = np.concatenate([np.concatenate([np.arange(g * nt, (g + 1) * nt), Bt + np.arange(g * n, (g + 1) * n)]) for g in range(G)])
        whole = eng.take(whole, index)
        is_arrival = torch.as_tensor(index >= Bt).to(eng.device)
        del everybody
        traffic = dict(traffic=committed, traffic_groups=nt)
        arms = {
            "stagger, traffic=": lambda: eng.stagger(arrivals, RADIUS, groups=n, **STAGGER, **traffic),
            "stagger, wide=True on the concatenation": lambda: eng.stagger(whole, RADIUS, groups=nt + n, wide=True, **STAGGER),
            "layer, traffic=": lambda: eng.layer(arrivals, RADIUS, groups=n, **LAYER, **traffic),
            "layer, wide=True on the concatenation": lambda: eng.layer(whole, RADIUS, groups=nt + n, wide=True, **LAYER),
            "separation_against": lambda: eng.separation_against(arrivals, committed, RADIUS, n, nt),
            "separation of the concatenation": lambda: eng.separation(whole, RADIUS, groups=nt + n),
        }
        said = {}
        for kind in ("stagger", "layer"):
            new, old = arms[f"{kind}, traffic="](), arms[f"{kind}, wide=True on the concatenation"]()
            ok = new.steps >= 0
            cross = eng.separation_against(eng.shift(arrivals, new.offsets) if kind == "layer" else arrivals, committed, RADIUS, n, nt,
                                           start_rows=new.start_rows if kind == "stagger" else None)
            torch.cuda.synchronize()
            assert int(cross.conflicts[ok].sum()) == 0, (kind, "a resolved arrival is inside the radius of a committed mission")
            said[kind] = {"arrivals resolved": float(ok.double().mean()), "arrivals moved": float((new.steps > 0).double().mean()),
                          "committed missions the re-run moved": int((old.steps[~is_arrival] > 0).sum()),
                          "committed missions the re-run left unresolved": int((old.steps[~is_arrival] == -1).sum()),
                          "arrivals the re-run resolved": float((old.steps[is_arrival] >= 0).double().mean())}
            print(json.dumps({"committed": Bt, "arrivals": B, "groups": G, "search": kind, **said[kind]}), flush=True)
        for fn in arms.values():                             # warm-up of every arm
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in arms}
        for rnd in range(rounds):
            for name in (list(arms) if rnd % 2 == 0 else list(arms)[::-1]):
                times[name].append(timed(arms[name]))
        for name, ts in times.items():
            med = float(np.median(ts))
            line = {"arm": name, "committed": Bt, "committed_per_group": nt, "arrivals": B, "arrivals_per_group": n, "groups": G, "m": M,
                    "radius": RADIUS, **(STAGGER if name.startswith("stagger") else {"delta": list(LAYER["delta"]), "max_steps": LAYER["max_steps"]}
                                         if name.startswith("layer") else {}),
                    "ms_per_round": [round(t, 3) for t in ts], "median_ms": round(med, 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
                    "rounds": rounds, **said.get(name.split(",")[0], {}), "box": box}
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
        del committed, arrivals, whole, arms
        torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None, help="the jsonl file")
    ap.add_argument("rounds", nargs="?", type=int, default=5)
    ap.add_argument("--shapes", default=None, help="committed:per_group:arrivals:per_group[,...] instead of the two shapes above (a rehearsal at a small size)")
    args = ap.parse_args()
    if args.shapes:
        SHAPES = tuple(tuple(int(v) for v in s.split(":")) for s in args.shapes.split(","))
    main(args.out, args.rounds)
