"""The flown conflict list (`uavac_flown_conflict_offsets_dev` + `uavac_flown_conflicts_dev`, `Engine.flown_conflicts`) against its
yardstick, the flown separation audit on the same log (`Engine.flown_separation`), and against the only other route to the same answers
that keeps the log on the device: chunked pairwise distances from the same state log in torch, and the pairs listed from them.  The
logs are real ones: eight segments (the bench's generator), velocity 3, dt 0.01, flown plan-fed for 1 000 ticks with a state log;
radius 0.5; the flown audit's two shapes:

    65 536 vehicles in groups of 64        4 096 vehicles in one group

    flown_conflicts_rate.py [OUT.jsonl] [rounds]
    flown_conflicts_rate.py [OUT.jsonl] [rounds] --against OTHER.so    both calls of this build against another build's (tools/against.py), appended

The two routes must give the SAME answers (offsets and every record, bit for bit) before anything is timed.  hipEvents around each arm,
warm-up first, the arms interleaved over rounds in one process; median, minimum and maximum per arm, one JSON line per arm with the
device's identity and the entry count, and one line per shape with the RATIOS this tool is for -- both calls over the flown audit, the
torch route over both calls -- each formed per round from that round's times, with the median and the spread over the rounds.
`Engine.flown_conflicts` includes its one host read (the number of entries) between the two calls; the arm "offsets call only" shows the
first call alone, so the fill (the second discovery, the list and the measure over the log) is the difference.

The torch route, per call: the positions (K, 3, B) of the log as (G, n, K) per axis; then, in chunks that keep a temporary under 1 GiB,
d^2 = (dx dx + dy dy) + dz dz for all pairs of a group as (chunk, i, j, k), the diagonal set to NaN, per pair `any` of d^2 < r^2, the
first and the last tick inside, their number, and the first minimum over the ticks whose d^2 is a number; the listed pairs in (vehicle,
partner) order.  Eager torch rounds every product and sum on its own, so the bits are the kernel's."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uav-autonomous-control_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from bench import missions  # noqa: E402
from uav_ac.fleet import Engine  # noqa: E402

M, VEL, DT, RADIUS, K = 8, 3.0, 0.01, 0.5, 1000
SHAPES = ((65536, 64), (4096, 4096))                     # (vehicles, group size)
TEMP_BYTES = 1 << 30


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def torch_route(log, n, radius):
    """-> (offsets (B + 1,), pair_d (E,), pair_i (5, E)) from the log (K, 13, B), groups of n consecutive vehicles."""
    dev = log.device
    ticks, _, B = log.shape
    G = B // n
    P = [log[:, c, :].t().reshape(G, n, ticks) for c in range(3)]                             # per axis (G, n, K)
    r2 = radius * radius
    per_i = n * ticks * 8
    ci = max(1, min(n, TEMP_BYTES // per_i))
    cg = max(1, min(G, TEMP_BYTES // (per_i * ci))) if ci == n else 1
    eye = torch.eye(n, dtype=torch.bool, device=dev)
    counts = torch.zeros((B,), dtype=torch.int64, device=dev)
    found = []
    for g0 in range(0, G, cg):
        for i0 in range(0, n, ci):
            d2 = None
            for c in range(3):
                Pg = P[c][g0:g0 + cg]
                d = Pg[:, i0:i0 + ci, None, :] - Pg[:, None, :, :]                            # (cg, ci, n, K): own minus partner
                d = d * d
                d2 = d if d2 is None else d2 + d          # (dx dx + dy dy) + dz dz, left to right
            d2.masked_fill_(eye[i0:i0 + ci][None, :, :, None], float("nan"))                  # a vehicle is nobody's partner
            inside = d2 < r2                                                                  # (a NaN is never below anything)
            g, i, j = inside.any(dim=3).nonzero(as_tuple=True)                                # ascending vehicle, then ascending partner
            hit, dd = inside[g, i, j], d2[g, i, j]                                            # (e, K)
            dd = torch.where(dd.isnan(), torch.full_like(dd, float("inf")), dd)
            low = dd.argmin(dim=1)                                                            # the first minimum: the lowest tick
            own = (g0 + g) * n + i0 + i
            counts += torch.bincount(own, minlength=B)
            found.append((torch.sqrt(dd.gather(1, low[:, None])[:, 0]),
                          torch.stack([(g0 + g) * n + j, hit.to(torch.int8).argmax(dim=1),
                                       ticks - 1 - hit.flip(1).to(torch.int8).argmax(dim=1), hit.sum(dim=1), low]).to(torch.int32)))
    offsets = torch.zeros((B + 1,), dtype=torch.int64, device=dev)
    offsets[1:] = counts.cumsum(0)
    return offsets, torch.cat([f[0] for f in found]), torch.cat([f[1] for f in found], dim=1)


def spread(values):
    return {"median": round(float(np.median(values)), 3), "min": round(float(min(values)), 3), "max": round(float(max(values)), 3)}


def main_against(out_path, rounds, other):
    """Both calls through this build and through another one (tools/against.py), on the same log (flown once, through the Engine)."""
    import ctypes as C
    import against
    from against import P, ptr as p
    log_args = [P, P, C.c_int, C.c_int, C.c_int64, P, C.c_int, C.c_double]
    builds = against.Builds(other, {"uavac_flown_conflict_offsets_dev": log_args + [P],
                                    "uavac_flown_conflicts_dev": log_args + [P, C.c_int64, P, P]})
    eng = Engine("cuda:0")
    kw = dict(device="cuda:0")
    for B, n in SHAPES:
        plan = eng.plan(missions(B, M, 0, B), VEL, DT, rows=False)
        log, _ = eng.fleet(plan).rollout(K, state_log=True)
        ticks, _, pitch = eng._log_view(log)
        go = torch.arange(0, B + 1, n, dtype=torch.int64, **kw)
        torch.cuda.synchronize()

        def both_calls(lib, ctx):
            """what `Engine.flown_conflicts` does: the offsets, the host read of the entry count, the buffers, the fill"""
            off = torch.empty((B + 1,), dtype=torch.int64, **kw)
            args = (ctx, p(log), ticks, B, pitch, p(go), B // n, RADIUS)
            assert lib.uavac_flown_conflict_offsets_dev(*args, p(off)) == 0
            E = int(off[B].item())
            d, i = torch.empty((E,), dtype=torch.float64, **kw), torch.empty((5, E), dtype=torch.int32, **kw)
            if E:
                assert lib.uavac_flown_conflicts_dev(*args, p(off), E, p(d), p(i)) == 0
            return off, d, i
        builds.alternate("flown conflict list, both calls", both_calls, rounds, B=B, group=n, ticks=ticks)
        del plan, log, go
        torch.cuda.empty_cache()
    builds.write(out_path)


def main():
    from against import split_argv
    argv, other = split_argv(sys.argv[1:])
    out_path = argv[0] if len(argv) > 0 else None
    rounds = int(argv[1]) if len(argv) > 1 else 5
    if other:
        return main_against(out_path, rounds, other)
    eng = Engine("cuda:0")
    box = eng.ctx.device_identity()
    lines = []
    for B, n in SHAPES:
        plan = eng.plan(missions(B, M, 0, B), VEL, DT, rows=False)
        fleet = eng.fleet(plan)
        log, _ = fleet.rollout(K, state_log=True)
        groups = None if n == B else n
        pair_ticks = (B // n) * n * (n - 1) * K
        ticks, _, pitch = eng._log_view(log)
        offsets_only = torch.empty((B + 1,), dtype=torch.int64, device=eng.device)
        go, G = eng._groups(groups, B)

        def offsets_call():
            eng._bind_stream()
            eng.ctx.call("uavac_flown_conflict_offsets_dev", log.data_ptr(), ticks, B, pitch, go.data_ptr() if go is not None else None, G,
                         RADIUS, offsets_only.data_ptr())

        # the two routes agree before anything is timed: offsets and every record, bit for bit; and the list agrees with the flown audit
        cl = eng.flown_conflicts(log, RADIUS, groups=groups)
        a = eng.flown_separation(log, RADIUS, groups=groups)
        want_off, want_d, want_i = torch_route(log, n, RADIUS)
        offsets_call()
        torch.cuda.synchronize()
        differ = {"offsets": int((cl.offsets != want_off).sum()), "offsets call": int((offsets_only != want_off).sum()),
                  "entries": abs(cl.total - int(want_off[-1]))}
        if not differ["entries"]:
            differ.update({"pair_d": int((cl.min_distance != want_d).sum()), "pair_i": int((cl.block != want_i).sum())})
        differ["counts against the flown audit"] = int((cl.offsets[1:] - cl.offsets[:-1] != a.conflicts).sum())
        print(json.dumps({"B": B, "group": n, "ticks": K, "entries": cl.total, "most partners of one vehicle": int(a.conflicts.max()),
                          "outputs that differ between the two routes": differ}), flush=True)
        assert not any(differ.values()), differ

        arms = {"flown conflict list, both calls": (lambda: eng.flown_conflicts(log, RADIUS, groups=groups), 5),
                "flown conflict list, offsets call only": (offsets_call, 5),
                "flown separation audit": (lambda: eng.flown_separation(log, RADIUS, groups=groups), 5),
                "torch route: chunked pairwise distances from the same log + list": (lambda: torch_route(log, n, RADIUS), 1)}
        for fn, _ in arms.values():                      # warm-up of every arm
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name in arms}
        for _ in range(rounds):
            for name, (fn, reps) in arms.items():
                times[name].append(timed(fn, reps))
        for name, ts in times.items():
            med = float(np.median(ts))
            lines.append(json.dumps({"arm": name, "B": B, "group": n, "ticks": K, "pair_ticks": pair_ticks, "entries": cl.total,
                                     "median_ms": round(med, 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "rounds": rounds,
                                     "box": box}))
            print(lines[-1], flush=True)
        both, first, audit, other = (np.array(times[name]) for name in arms)
        lines.append(json.dumps({"ratios": True, "B": B, "group": n, "ticks": K, "rounds": rounds, "entries": cl.total,
                                 "both calls / flown separation audit": spread(both / audit),
                                 "offsets call / flown separation audit": spread(first / audit),
                                 "fill (both calls - offsets call) ms": spread(both - first),
                                 "torch route / both calls": spread(other / both), "box": box}))
        print(lines[-1], flush=True)
        del plan, fleet, log, cl, a, want_off, want_d, want_i
        torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
