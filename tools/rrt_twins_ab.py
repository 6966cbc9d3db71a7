"""What the host layer of the RRT* twins (csrc/rrt_star.hip: argument checks, device scratch, staging) costs per call, this build against
another build of the same ABI -- `--against OTHER.so`, as in tools/against.py: both loaded privately into one process, outputs compared
byte for byte before anything is timed, the build that goes first alternating.  Wall-clock times, the device drained at the end of each:
  steer x N           N = 2 000 back-to-back `uavac_rrt_steer` at E = 1, as RRTStar._adapt_random_node_position calls it
  edge_lengths x N    N back-to-back `uavac_rrt_edge_lengths` at E = 200 against one point, as RRTStar._find_nearest_node calls it
  rrt_star            one `uavac_rrt_star` at B = 64, 1 000 iterations, on the lab cuboids and inputs of tools/rrt_rate.py
  rrt_star_dev        `uavac_rrt_star_dev` at the same shape: no host layer, the control
Run it with a byte-identical copy of one library as OTHER.so: the spread of that ratio is the margin of the method.
    python tools/rrt_twins_ab.py --against OTHER.so [--rounds 9] [--out profiles/rrt_twins_ab.jsonl]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uav-autonomous-control_amd"), os.path.join(ROOT, "tools")]
from against import Builds, ptr, split_argv                      # noqa: E402
from uav_ac import _native as nat                                # noqa: E402
from uav_ac.planning.rrt import draw_random_nodes_batch          # noqa: E402

argv, other = split_argv(sys.argv[1:])
assert other, __doc__
rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 9
out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
N = 2_000
NAMES = ("uavac_rrt_steer", "uavac_rrt_edge_lengths", "uavac_rrt_star", "uavac_rrt_star_dev")
builds = Builds(other, {name: nat._SIGNATURES[name][1] for name in NAMES})
np_ptr = nat.np_ptr
rng = np.random.default_rng(5)

# ---- the per-call primitives of the facade
sample, nearest, steered = rng.uniform(0.0, 10.0, (1, 3)), rng.uniform(0.0, 10.0, (1, 3)), np.empty((1, 3))
E = 200
tree, query, lengths = rng.uniform(0.0, 10.0, (E, 3)), rng.uniform(0.0, 10.0, 3), np.empty(E)


def steer(lib, ctx):
    for _ in range(N):
        rc = lib.uavac_rrt_steer(ctx, np_ptr(sample), np_ptr(nearest), 1, 1.5, np_ptr(steered))
    assert rc == 0
    return (steered,)


def edge_lengths(lib, ctx):
    for _ in range(N):
        rc = lib.uavac_rrt_edge_lengths(ctx, np_ptr(tree), np_ptr(query), 1, E, np_ptr(lengths))
    assert rc == 0
    return (lengths,)


builds.wall(f"uavac_rrt_steer x {N}", steer, rounds, E=1, calls=N)
builds.wall(f"uavac_rrt_edge_lengths x {N}", edge_lengths, rounds, E=E, calls=N)

# ---- one batch, through the twin and through the device entry point (tools/rrt_rate.py's problems)
LAB = np.array([[3.7, 4.3, 4.0, 10.0, -3.4, -2.8], [10.7, 11.3, 4.0, 10.0, -2.2, 0.0],
                [13.3, 14.7, 6.3, 7.7, -6.0, 0.0], [20.2, 20.8, 4.0, 10.0, -3.3, -2.7]])
lw, up = np.array([0.0, 0.0, -6.0]), np.array([24.0, 14.0, 0.0])
B, max_iter, step = 64, 1000, 1.5
cap = max_iter + 1
rng = np.random.default_rng(5)
starts = np.round(rng.uniform([0.5, 1, -3], [2, 13, -1], (B, 3)), 2)
goals = np.round(rng.uniform([22, 1, -3], [23.5, 13, -1], (B, 3)), 2)
samples = draw_random_nodes_batch(np.arange(B), lw, up, goals, max_iter)
outs = [np.empty((B, cap, 3)), np.empty((B, cap), np.int32), np.empty((B, cap), np.int32), np.empty((B, cap), np.int32),
        np.empty((B, cap, 3)), np.empty((B, 6), np.int32), np.empty(B)]
ins_d = [torch.as_tensor(a).cuda() for a in (starts, goals, samples, LAB)]
outs_d = [torch.as_tensor(a).cuda() for a in outs]


def rrt_star(lib, ctx):
    assert lib.uavac_rrt_star(ctx, np_ptr(starts), np_ptr(goals), B, step, max_iter, np_ptr(samples), np_ptr(LAB), len(LAB),
                              *[np_ptr(a) for a in outs]) == 0
    return outs


def rrt_star_dev(lib, ctx):
    s_d, g_d, smp_d, lab_d = ins_d
    assert lib.uavac_rrt_star_dev(ctx, ptr(s_d), ptr(g_d), B, step, max_iter, ptr(smp_d), ptr(lab_d), len(LAB), *[ptr(t) for t in outs_d]) == 0
    return outs_d


builds.wall("uavac_rrt_star", rrt_star, rounds, B=B, max_iter=max_iter)
builds.wall("uavac_rrt_star_dev", rrt_star_dev, rounds, B=B, max_iter=max_iter)
builds.write(out_path)
