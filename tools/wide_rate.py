"""The prioritised searches for groups of any size (`uavac_minsnap_stagger_wide_dev`, `uavac_minsnap_layer_wide_dev`; `Engine.stagger` and
`Engine.layer` with `wide=True`) at every block size (ctx option "search_block": 64, 128, 256), and beside the narrow calls where both
exist.  Eight segments (the bench's generator), velocity 3, dt 0.01, radius 0.5, starts 0; stagger with step 1 and max_steps 255, layer
with delta (0, 0, -0.25) and max_steps 63.  Three shapes:

    one group of 4 096 missions        65 536 missions in groups of 1 024        4 096 missions in groups of 256 (wide beside narrow)

    wide_rate.py [OUT.jsonl] [rounds] [--shapes B:group[:narrow],...]
    wide_rate.py [OUT.jsonl] [rounds] --against OTHER.so     the NARROW calls of this build against another build, records appended

Every route to an answer must give the SAME block (every row, every mission) before anything is timed: the three block sizes among
each other, and the wide call against the narrow one at the third shape.  hipEvents around each arm, warm-up first, the arms
interleaved over rounds in one process; median, minimum and maximum per arm, one JSON line per arm with the device's identity and the
shares of moved and unresolved missions.  The third shape is the price of the seed machinery where it is not needed: reported, not
bounded.
`--against OTHER.so` (tools/against.py): the gate of the change that gave the search its block-wise form -- `uavac_minsnap_stagger_dev`,
`uavac_minsnap_layer_dev` and `uavac_minsnap_layer_obs_dev` (four cuboids) through this build and through another build of the same ABI
(the parent commit's), both loaded privately into one process, on the same plan, alternating which goes first, at 65 536 missions in
groups of 64 and 4 096 in groups of 256; the outputs are compared byte for byte first."""
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
SHAPES = ((4096, 4096, False), (65536, 1024, False), (4096, 256, True))      # (missions, group size, beside the narrow call)
BLOCKS = (64, 128, 256)


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
    for B, n, narrow in SHAPES:
        plan = eng.plan(missions(B, M, 0, B), VEL, DT, rows=False)
        groups = None if n >= B else n

        def search(kind, blk):
            """blk: a block size of the wide call, or None for the narrow call"""
            if blk is not None:
                eng.ctx.set_option("search_block", blk)
            kw = dict(groups=groups, wide=blk is not None)
            return eng.stagger(plan, RADIUS, **STAGGER, **kw) if kind == "stagger" else eng.layer(plan, RADIUS, **LAYER, **kw)

        arms = {}
        for kind in ("stagger", "layer"):
            answers = {blk: search(kind, blk).block[:3].clone() for blk in BLOCKS + ((None,) if narrow else ())}
            torch.cuda.synchronize()
            first = answers[BLOCKS[0]]
            for blk, block in answers.items():           # every route gives the same block before anything is timed
                assert torch.equal(block, first), (kind, B, n, blk, int((block != first).any(dim=0).sum()))
            share = {"moved": float((first[1] > 0).double().mean()), "unresolved": float((first[1] == -1).double().mean()),
                     "examined": float((first[1] != -2).double().mean()), "highest candidate": int(first[1].max())}
            print(json.dumps({"B": B, "group": n, "search": kind, "routes that agree": len(answers), **share}), flush=True)
            for blk in answers:
                name = f"{kind}, narrow call" if blk is None else f"{kind}, wide, search_block {blk}"
                arms[name] = (lambda kind=kind, blk=blk: search(kind, blk), share)
        for fn, _ in arms.values():                      # warm-up of every arm
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in arms}
        for rnd in range(rounds):
            for name in (list(arms) if rnd % 2 == 0 else list(arms)[::-1]):
                times[name].append(timed(arms[name][0]))
        for name, ts in times.items():
            med = float(np.median(ts))
            line = {"arm": name, "B": B, "group": n, "m": M, "radius": RADIUS, **(STAGGER if name.startswith("stagger") else
                                                                                   {"delta": list(LAYER["delta"]), "max_steps": LAYER["max_steps"]}),
                    "ms_per_round": [round(t, 3) for t in ts], "median_ms": round(med, 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
                    "rounds": rounds, "missions_per_s": B / (med * 1e-3), **arms[name][1], "box": box}
            lines.append(json.dumps(line))
            print(lines[-1], flush=True)
        eng.ctx.set_option("search_block", 0)
        del plan, arms
        torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def main_against(out_path, rounds, other):
    import ctypes as C
    from against import Builds, P, ptr
    from layer_rate import cuboids
    from uav_ac.fleet import Engine
    head = [P, P, P, P, C.c_int, C.c_int, C.c_double, P, C.c_int, P, C.c_double]
    builds = Builds(other, {"uavac_minsnap_stagger_dev": head + [C.c_int, C.c_int, P],
                            "uavac_minsnap_layer_dev": head + [C.c_double] * 3 + [C.c_int, P, P],
                            "uavac_minsnap_layer_obs_dev": head + [C.c_double] * 3 + [C.c_int, P, C.c_int, P, P]})
    eng = Engine("cuda:0")
    kw = dict(device=eng.device)
    cub = torch.as_tensor(cuboids(4)).to(eng.device)
    for B, n in ((65536, 64), (4096, 256)):
        plan = eng.plan(missions(B, M, 0, B), VEL, DT, rows=False)
        torch.cuda.synchronize()
        go = torch.arange(0, B + 1, n, dtype=torch.int64, **kw)
        out = {name: (torch.empty((4, B), dtype=torch.int32, **kw), torch.empty((B, 3), dtype=torch.float64, **kw)) for name in builds.lib}
        names = {id(lib): name for name, lib in builds.lib.items()}
        args = (ptr(plan.coeffs), ptr(plan.seg_rows), None, B, M, DT, ptr(go), B // n, None, RADIUS)

        def stagger(lib, ctx):
            il, _ = out[names[id(lib)]]
            assert lib.uavac_minsnap_stagger_dev(ctx, *args, STAGGER["step"], STAGGER["max_steps"], ptr(il)) == 0
            return (il[:3],)

        def layer(lib, ctx):
            il, off = out[names[id(lib)]]
            assert lib.uavac_minsnap_layer_dev(ctx, *args, *LAYER["delta"], LAYER["max_steps"], ptr(il), ptr(off)) == 0
            return il[:3], off

        def layer_obs(lib, ctx):
            il, off = out[names[id(lib)]]
            assert lib.uavac_minsnap_layer_obs_dev(ctx, *args, *LAYER["delta"], LAYER["max_steps"], ptr(cub), 4, ptr(il), ptr(off)) == 0
            return il, off
        for arm, call in (("uavac_minsnap_stagger_dev", stagger), ("uavac_minsnap_layer_dev", layer), ("uavac_minsnap_layer_obs_dev", layer_obs)):
            builds.alternate(arm, call, rounds, reps=2, B=B, group=n, m=M, radius=RADIUS)
        del plan, go, out
        torch.cuda.empty_cache()
    builds.write(out_path)


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=None, help="the jsonl file")
    ap.add_argument("rounds", nargs="?", type=int, default=3)
    ap.add_argument("--shapes", default=None, help="B:group[:narrow][,...] instead of the three shapes above (a rehearsal at a small size)")
    ap.add_argument("--against", default=None, help="another libuavac.so: the three narrow calls of both builds, alternating")
    args = ap.parse_args()
    if args.shapes:
        SHAPES = tuple((int(v[0]), int(v[1]), len(v) > 2) for v in (s.split(":") for s in args.shapes.split(",")))
    if args.against:
        main_against(args.out, args.rounds, args.against)
    else:
        main(args.out, args.rounds)
