"""What the host layer of the C ABI (csrc/uavac_api.hip: argument checks, device scratch, staging) costs per call, this build against
another build of the same ABI -- `--against OTHER.so`, as in tools/against.py: both loaded privately into one process, outputs compared
byte for byte before anything is timed, the build that goes first alternating.  Wall-clock times, the stream drained at the end of each:
  plan, rollout       the host-pointer twins of tools/host_path_rate.py at its shape (B = 4 096, m = 8, K = 1 000)
  separation_dev x N  N = 10 000 back-to-back calls of a device entry point that takes scratch (B = 64, m = 4)
  cost_dev x N        ... and of one that does not
Run it with a byte-identical copy of one library as OTHER.so: the spread of that ratio is the margin of the method.
    python tools/host_layer_ab.py --against OTHER.so [--rounds 7] [--call-rounds 7] [--out profiles/host_layer_ab.jsonl]
(--rounds: of the twins, milliseconds each; --call-rounds: of the back-to-back arms, N calls each)"""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "uav-autonomous-control_amd"), os.path.join(ROOT, "tools")]
from against import THIS, Builds, ptr, split_argv                # noqa: E402
from bench import missions                                       # noqa: E402
from uav_ac import _native as nat                                # noqa: E402

argv, other = split_argv(sys.argv[1:])
assert other, __doc__
twin_rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 7
call_rounds = int(argv[argv.index("--call-rounds") + 1]) if "--call-rounds" in argv else 7
out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
N = 10_000
NAMES = ("uavac_minsnap_row_counts", "uavac_minsnap_solve", "uavac_minsnap_sample", "uavac_state_init", "uavac_control_rollout",
         "uavac_minsnap_plan_dev", "uavac_minsnap_separation_dev", "uavac_minsnap_cost_dev")
builds = Builds(other, {name: nat._SIGNATURES[name][1] for name in NAMES})
dev = torch.device("cuda:0")
np_ptr = nat.np_ptr


# ---- the host-pointer twins at tools/host_path_rate.py's shape
B, m, K = 4096, 8, 1000
wps = nat.as_f64(missions(B, m, 0, B))
times, seg, offs, coeffs = np.empty((B, m)), np.empty((B, m), np.int32), np.empty(B + 1, np.int64), np.empty((B, 8 * m, 3))
traj = [None]


def plan(lib, ctx):
    assert lib.uavac_minsnap_row_counts(ctx, np_ptr(wps), B, m, 3.0, 0.01, np_ptr(times), np_ptr(seg), np_ptr(offs)) == 0
    assert lib.uavac_minsnap_solve(ctx, np_ptr(wps), B, m, 3.0, np_ptr(coeffs), None) == 0
    if traj[0] is None:
        traj[0] = np.empty((int(offs[-1]), 11))
    assert lib.uavac_minsnap_sample(ctx, np_ptr(coeffs), np_ptr(times), B, m, 0.01, np_ptr(offs), np_ptr(traj[0])) == 0
    return times, seg, offs, coeffs, traj[0]


builds.wall("host-pointer plan", plan, twin_rounds, B=B, m=m)
V = nat.Vehicle.default()
state0, istate0 = np.zeros((nat.STATE_ROWS, B)), np.zeros((nat.ISTATE_ROWS, B), np.int32)
assert builds.lib[THIS].uavac_state_init(builds.ctx[THIS], C.byref(V), np_ptr(np.ascontiguousarray(wps[:, 0, :])), B, 1, np_ptr(state0),
                                         np_ptr(istate0)) == 0
log = np.empty((K, 13, B))


def roll(lib, ctx):
    state, istate = state0.copy(), istate0.copy()
    assert lib.uavac_control_rollout(ctx, C.byref(V), np_ptr(traj[0]), np_ptr(offs), np_ptr(state), np_ptr(istate), B, K, np_ptr(log), None,
                                     None, 0) == 0
    return state, istate, log


builds.wall("host-pointer rollout", roll, twin_rounds, B=B, K=K)

# ---- back-to-back calls of two device entry points
B, m = 64, 4
wp_d = torch.as_tensor(nat.as_f64(missions(B, m, 0, B))).to(dev)
times_d, seg_d = torch.zeros(B, m, dtype=torch.float64, device=dev), torch.zeros(B, m, dtype=torch.int32, device=dev)
offs_d, coeffs_d = torch.zeros(B + 1, dtype=torch.int64, device=dev), torch.zeros(B, 8 * m, 3, dtype=torch.float64, device=dev)
assert builds.lib[THIS].uavac_minsnap_plan_dev(builds.ctx[THIS], ptr(wp_d), B, m, 3.0, 0.01, ptr(times_d), ptr(seg_d), ptr(offs_d), ptr(coeffs_d),
                                               None, None, 0, None, None) == 0
sep_d, isep_d = torch.zeros(B, dtype=torch.float64, device=dev), torch.zeros(5, B, dtype=torch.int32, device=dev)
cost_d = torch.zeros(B, dtype=torch.float64, device=dev)


def separation(lib, ctx):
    for _ in range(N):
        rc = lib.uavac_minsnap_separation_dev(ctx, ptr(coeffs_d), ptr(seg_d), None, B, m, 0.01, None, 1, None, 1.0, ptr(sep_d), ptr(isep_d))
    assert rc == 0
    return sep_d, isep_d


def cost(lib, ctx):
    for _ in range(N):
        rc = lib.uavac_minsnap_cost_dev(ctx, ptr(coeffs_d), ptr(times_d), None, B, m, ptr(cost_d))
    assert rc == 0
    return (cost_d,)


builds.wall(f"uavac_minsnap_separation_dev x {N}", separation, call_rounds, B=B, m=m, calls=N)
builds.wall(f"uavac_minsnap_cost_dev x {N}", cost, call_rounds, B=B, m=m, calls=N)
builds.write(out_path)
