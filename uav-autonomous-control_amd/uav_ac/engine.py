"""Batched planning over libuavac.so: `Engine` (one GPU, one `uavac_ctx`) and the device-resident plans it returns.

The batched form of `MinimumSnap(...).get_trajectory()` (uav_ac/planning/minimum_snap.py:59-124, upstream path) and of
`RRTStar.run()` (planning/rrt.py).  PyTorch is plumbing only: it owns device memory and the HIP stream; all arithmetic
happens in the hand-written HIP kernels behind the C ABI (include/uavac.h).  No CPU fallback exists.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _native as nat
from .plans import (Airspaces, ConflictList, DeconflictResult, FlightAudit, LayerResult, Plan, PlanAudit, PlanDemand, PlanEnvelope,  # noqa: F401
                    PlanNeed, RaggedBatch, RaggedPlan, RetimeResult, RRTDeviceBatch, Segments, SeparationAudit, StaggerResult, TimeOptResult, _ptr, segments,
                    uniform_offsets)  # (the plans and result records live in uav_ac/plans.py; every name is re-exported here)


def _torch():
    import torch
    return torch


class Engine:
    """One GPU, one `uavac_ctx`.  Kernels are enqueued on torch's current stream for that device."""
    FAST_ROW_BUFFER_FRACTION_OF_PEAK = 0.70    # `place_rows`: a row buffer the sampler fills at this share of the device's HBM peak is of the fast kind

    def __init__(self, device=None):
        torch = _torch()
        if not torch.cuda.is_available():
            raise nat.UavacError(nat.EHIP, "no GPU visible: the uavac engine has no CPU fallback")
        dev = torch.device("cuda") if device is None else torch.device(device)
        if dev.type != "cuda":
            raise nat.UavacError(nat.EHIP, f"device {dev} is not a GPU: the uavac engine has no CPU fallback")
        if dev.index is None:                                   # "cuda": the thread's current device
            dev = torch.device("cuda", torch.cuda.current_device())
        self.device = dev
        # the ctx remembers its device; every C entry point makes it current for its own duration (and restores the
        # caller's), so an Engine for cuda:1 works while cuda:0 is torch's current device
        self.ctx = nat.Context(self.device.index)
        self._torch = torch
        self._comm = None
        self._row_pool = None            # plan(..., pool=True): the one pooled row buffer (rows x 11, float64)

    # -- plumbing ---------------------------------------------------------------
    def _bind_stream(self):
        self.ctx.set_stream(self._torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, a, dtype):
        torch = self._torch
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(self.device)

    def clock_probe_begin(self, window_us: int, stream=None):
        """Start ONE wavefront on `stream` (a side stream: it then runs BESIDE whatever the current stream executes) that stamps
        shader cycles and real time `window_us` apart (`uavac_clock_probe_dev`).  Returns the ticket for `clock_probe_ghz`."""
        torch = self._torch
        with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream(self.device)):
            stamps = torch.empty((4,), dtype=torch.int64, device=self.device)      # (the kernel writes all four; no fill on another stream)
            self._bind_stream()
            self.ctx.call("uavac_clock_probe_dev", int(window_us), _ptr(stamps))
        self._bind_stream()                                   # back on the caller's stream
        return stamps

    @staticmethod
    def clock_probe_ghz(stamps) -> float:
        """Shader clock over a finished probe's window: (cycles1 - cycles0) / (real1 - real0) x 100 MHz.  (Synchronises.)"""
        c0, r0, c1, r1 = (int(v) for v in stamps.cpu().tolist())
        return (c1 - c0) / max(1, r1 - r0) * 0.1

    def _speeds(self, velocity, B: int):
        """`velocity` as the planning entry points take it -> (scalar, None) for one cruise speed, (NaN, (B,) f64 device tensor) for
        one per mission (anything that is not a number: a tensor, an array, a sequence)."""
        torch = self._torch
        if isinstance(velocity, (int, float, np.floating, np.integer)) or (getattr(velocity, "ndim", 1) == 0):
            return float(velocity), None
        v = self._dev(velocity, torch.float64).reshape(-1)
        if v.numel() != B:
            raise ValueError(f"one cruise speed per mission: expected {B} velocities, got {v.numel()}")
        return float("nan"), v

    # -- planning ---------------------------------------------------------------
    def plan(self, waypoints, velocity=1.0, dt: float = 0.01, strict: bool = True, dense_yaw: bool = False,
             placement_trials: int = 1, pool: bool = False, rows: bool = True, boundary=None, times=None) -> Plan:
        """Batched `MinimumSnap(path, None, velocity, dt).get_trajectory()` (minimum_snap.py:59-61,97-124).
        `strict`: raise UavacError(ESINGULAR) when a mission's knot system is singular (a repeated waypoint) instead of
        returning NaN coefficients for it; with strict=False inspect `plan.status`.
        `dense_yaw`: also keep the yaw column on its own (`plan.yaw`, 8 B per row).  Not needed to fly the plan: the
        plan-fed rollout scans the yaw itself from `plan.first_yaw` (8 B per mission).
        `placement_trials` > 1 (opt-in; default 1 = take the first allocation): draw up to that many row buffers one after the
        other and keep the first of the fast kind, else the fastest seen (`place_rows`: at most TWO alive at any time).  Row
        buffers come in three kinds (DESIGN K2, NOTES R4-6): the bench's 7.5 GB of rows take the default chunk-streaming sampler
        1.24-1.26 ms into a fast one, 1.38-1.43 into a slow one, and a process's first large allocation is usually a slow one.
        `pool=True`: the row buffer comes from / goes to the Engine's pool -- ONE buffer, found once (with `placement_trials`), handed
        to every later pooled plan of at most that many rows, so that the search is paid once per process.  Pooled plans share
        their rows' storage: one of them is current at a time (the use it is meant for: the same fleet planned again and again).
        `rows=False`: the ROWS-FREE chain (`uavac_minsnap_plan_dev` with traj = NULL): durations, row counts, offsets, coefficients
        and the missions' first headings (`uavac_minsnap_first_yaw_dev`), not one sampled row -- `plan.traj` is None.  Everything a
        plan-fed `Fleet` and `RcclComm.gather_plan` need; for the ranks of a multi-GPU job whose trajectories are sampled where they
        are wanted (the gather's root re-samples them from the gathered plan, bit-identical).  `Engine.sample_rows(plan)` adds the
        rows later.
        `velocity`: a number -- one cruise speed for the batch, the scalar entry points exactly as ever -- or a (B,) tensor / array:
        one per mission (`uavac_minsnap_*_v_dev`; `plan.velocities`, and `plan.velocity` is NaN).  Mission b is then bit for bit what
        a scalar call at velocity[b] gives it.  A speed that is not positive and finite cannot be refused without a sync: it raises
        device flag 0 (`take_flags`) and leaves its mission without rows.
        `boundary`: a (B, 6, 3) array or tensor -- velocity, acceleration, jerk at every mission's FIRST waypoint (rows 0-2) and at its
        LAST one (rows 3-5), columns x y z -- for missions that start and / or end in motion (`uavac_minsnap_plan_bc_dev`, with rows
        or rows-free; `Fleet.boundary()` gives the live velocities of a flying fleet).  None: rest to rest, the reference's
        constraints.  Durations, row counts and offsets do not depend on it; row 0 of a mission then carries velocity v0.  The plan
        keeps the tensor (`plan.boundary`, read again at every `replan` / `solve`: change it in place to replan from another state)
        and cannot be retimed (`retime` raises).
        `times`: a (B, m) array or tensor of segment durations to plan from AS GIVEN (`uavac_minsnap_plan_t_dev`) instead of
        upstream's |leg| / velocity rule -- rest to rest only: not with `boundary`, nor with a `velocity` other than the default.
        The plan is `free_times`: `velocity` is NaN, `replan` / `solve` re-run the chain from `plan.times` as they stand (change them
        in place and replan), `retime` raises.  Given the durations of a velocity plan it reproduces that plan bit for bit.  A
        duration that is not positive and finite is a ValueError under `strict`; without it the duration raises device flag 0
        (`take_flags`) and leaves its mission without rows.
        """
        torch = self._torch
        wp = self._dev(waypoints, torch.float64)
        if wp.dim() != 3 or wp.shape[2] != 3 or wp.shape[1] < 2:
            raise ValueError(f"waypoints must have shape (B, m+1, 3), got {tuple(wp.shape)}")
        if not bool(torch.isfinite(wp).all()):
            raise ValueError("waypoints must be finite")
        B, m = int(wp.shape[0]), int(wp.shape[1]) - 1
        if times is not None:
            self._refuse_with_times(velocity, boundary)
            if pool or int(placement_trials) > 1:
                raise ValueError("pool and placement_trials are not offered with times=")
            tm = self._dev(times, torch.float64)
            if tuple(tm.shape) != (B, m):
                raise ValueError(f"times must have shape (B, m) = ({B}, {m}), got {tuple(tm.shape)}")
            return self._plan_from_times(wp, tm.clone(), dt, rows, strict, dense_yaw=dense_yaw)
        velocity, speeds = self._speeds(velocity, B)
        kw = dict(device=self.device)
        if boundary is not None:
            boundary = self._dev(boundary, torch.float64)
            if tuple(boundary.shape) != (B, 6, 3):
                raise ValueError(f"boundary must have shape (B, 6, 3) = ({B}, 6, 3), got {tuple(boundary.shape)}")
            if not bool(torch.isfinite(boundary).all()):
                raise ValueError("boundary must be finite")
            if speeds is None:                                   # the chain with boundaries takes its speeds from the device
                speeds = torch.full((B,), float(velocity), dtype=torch.float64, **kw)
        times = torch.empty((B, m), dtype=torch.float64, **kw)
        seg_rows = torch.empty((B, m), dtype=torch.int32, **kw)
        row_offsets = torch.empty((B + 1,), dtype=torch.int64, **kw)
        coeffs = torch.empty((B, 8 * m, 3), dtype=torch.float64, **kw)
        status = torch.zeros((B,), dtype=torch.int32, **kw)
        self._bind_stream()
        if not rows:
            if dense_yaw or pool or int(placement_trials) > 1:
                raise ValueError("dense_yaw, pool and placement_trials are about the rows: not with rows=False")
            plan = Plan(B, m, float(velocity), float(dt), waypoints=wp, times=times, seg_rows=seg_rows, row_offsets=row_offsets, coeffs=coeffs,
                        status=status, traj=None, total_rows=0, first_yaw=torch.empty((B,), dtype=torch.float64, **kw), velocities=speeds,
                        boundary=boundary)
            self.replan(plan)
            plan.epoch = 0
            plan.total_rows = int(row_offsets[-1].item())       # (the one host sync; the rows would have needed it to be allocated)
            if strict:
                self.check(plan)
            return plan
        self._row_counts(wp, None, B, m, velocity, speeds, dt, times, seg_rows, row_offsets)
        if boundary is None:
            self.ctx.call("uavac_minsnap_solve_dev", _ptr(wp), _ptr(times), B, m, _ptr(coeffs), _ptr(status))
        total = int(row_offsets[-1].item())                 # the one host sync: sizes the trajectory buffer
        pooled = pool and self._row_pool is not None and self._row_pool.shape[0] >= total
        traj = self._row_pool[:total] if pooled else torch.empty((total, nat.TRAJ_COLS), dtype=torch.float64, **kw)
        yaw = torch.empty((total,), dtype=torch.float64, **kw) if dense_yaw else None
        plan = Plan(B, m, float(velocity), float(dt), waypoints=wp, times=times, seg_rows=seg_rows, row_offsets=row_offsets, coeffs=coeffs,
                    status=status, traj=traj, total_rows=total, yaw=yaw, first_yaw=torch.empty((B,), dtype=torch.float64, **kw),
                    velocities=speeds, boundary=boundary)
        del traj                                                 # (place_rows may release the first draw: no second reference to it)
        if boundary is None:
            self.sample(plan)
        else:                                                    # the whole chain into the buffer just sized (uavac_minsnap_plan_bc_dev)
            self.replan(plan)
            plan.epoch = 0
            plan.total_rows = total
        if int(placement_trials) > 1 and total > 0 and not pooled:
            self.place_rows(plan, int(placement_trials))
        if pool and not pooled:
            self._row_pool = plan.traj                           # (a larger pooled plan later replaces it)
        plan.pooled = bool(pool)
        if strict:
            self.check(plan)
        return plan

    @staticmethod
    def _refuse_with_times(velocity, boundary):
        if boundary is not None:
            raise ValueError("times= plans rest to rest: not with boundary=")
        if not (isinstance(velocity, (int, float, np.floating, np.integer)) and float(velocity) == 1.0):
            raise ValueError("times= gives the durations themselves: not with a velocity")

    def _plan_from_times(self, wp, times, dt: float, rows: bool, strict: bool, dense_yaw: bool = False, so=None, so_host=None,
                         max_m: int = 0):
        """The free_times plan of waypoints `wp` at durations `times` (device tensors; `times` becomes the plan's own): a Plan, or with
        seg_offsets `so` / `so_host` a RaggedBatch of at most `max_m` segments per mission.  Rows-free: one call of
        `uavac_minsnap_plan_t_dev`; with rows: the row counts first, to size the row buffer (the one host sync), then the chain."""
        torch = self._torch
        kw = dict(device=self.device)
        ragged = so is not None
        B = int(len(so_host) - 1 if ragged else wp.shape[0])
        m = int(max_m if ragged else wp.shape[1] - 1)
        seg_rows = torch.empty(times.shape, dtype=torch.int32, **kw)
        row_offsets = torch.empty((B + 1,), dtype=torch.int64, **kw)
        coeffs = torch.empty((times.numel(), 8, 3) if ragged else (B, 8 * m, 3), dtype=torch.float64, **kw)
        status = torch.zeros((B,), dtype=torch.int32, **kw)
        first_yaw = torch.empty((B,), dtype=torch.float64, **kw)
        traj = yaw = None
        self._bind_stream()
        if strict and not bool(((times > 0) & torch.isfinite(times)).all()):      # (without strict: device flag 0, no rows)
            raise ValueError("times must be positive and finite")
        if rows:
            self._row_counts(wp, so, B, m, None, None, dt, times, seg_rows, row_offsets, free_times=True)
            total = int(row_offsets[-1].item())
            traj = torch.empty((total, nat.TRAJ_COLS), dtype=torch.float64, **kw)
            yaw = torch.empty((total,), dtype=torch.float64, **kw) if dense_yaw else None
        elif dense_yaw:
            raise ValueError("dense_yaw is about the rows: not with rows=False")
        self.ctx.call("uavac_minsnap_plan_t_dev", _ptr(wp), _ptr(so), B, m, _ptr(times), float(dt), _ptr(seg_rows), _ptr(row_offsets),
                      _ptr(coeffs), _ptr(status), _ptr(traj), 0 if traj is None else int(traj.shape[0]), _ptr(yaw), _ptr(first_yaw))
        parts = dict(waypoints=wp, times=times, seg_rows=seg_rows, row_offsets=row_offsets, coeffs=coeffs, status=status, traj=traj,
                     total_rows=int(row_offsets[-1].item()), first_yaw=first_yaw, free_times=True)
        if ragged:
            plan = RaggedBatch(B, m, float("nan"), float(dt), seg_offsets=so, seg_offsets_host=so_host, **parts)
        else:
            plan = Plan(B, m, float("nan"), float(dt), yaw=yaw, **parts)
        if strict:
            self.check(plan)
        return plan

    def empty_plan(self, m: int, velocity: float = 1.0, dt: float = 0.01, rows: bool = True) -> Plan:
        """A Plan of NO missions: what a rank holds that plans and flies nothing -- the root of a final gather that only assembles
        the trajectories -- so that it takes part in the gathers (`RcclComm.gather_rows` / `gather_plan`) with empty blocks."""
        torch = self._torch
        kw = dict(device=self.device)
        m = int(m)
        z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, **kw)      # noqa: E731
        return Plan(0, m, float(velocity), float(dt), waypoints=z((0, m + 1, 3), torch.float64), times=z((0, m), torch.float64),
                    seg_rows=z((0, m), torch.int32), row_offsets=z((1,), torch.int64), coeffs=z((0, 8 * m, 3), torch.float64),
                    status=z((0,), torch.int32), traj=z((0, nat.TRAJ_COLS), torch.float64) if rows else None, total_rows=0,
                    first_yaw=z((0,), torch.float64))

    def hbm_peak_bytes_per_s(self) -> float:
        """The device's HBM peak from its own properties (memory clock x bus width x 2, DDR): 8.0e12 on MI355X."""
        p = self._torch.cuda.get_device_properties(self.device)
        clock_khz = getattr(p, "memory_clock_rate", 0) or 0
        width_bits = getattr(p, "memory_bus_width", 0) or 0
        peak = 2.0 * clock_khz * 1e3 * width_bits / 8.0
        return peak if peak > 1e11 else 8.0e12

    def place_rows(self, plan: Plan, trials: int):
        """Optional: choose `plan.traj` among up to `trials` candidate allocations by timing the sampler on each (see `plan`)."""
        torch = self._torch

        def timed(buf):
            # The chip's clock sags within milliseconds of idling (an allocation, a device query) and takes ~30 ms of work to come
            # back: blocks of three sampler runs are timed until two blocks in a row agree to 2 % (ten at most), the last one counts.
            plan.traj = buf
            self.sample(plan)                                    # first touch of fresh pages is not what is compared
            prev = None
            for _ in range(10):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(3):
                    self.sample(plan)
                b.record()
                b.synchronize()
                t = a.elapsed_time(b) / 3
                if prev is not None and abs(t - prev) <= 0.02 * prev:
                    break
                prev = t
            return t

        # Draws come one after the other and at most two buffers are alive: the best so far and the candidate.  A released
        # buffer goes back to the DRIVER (torch.cuda.empty_cache(): torch's cache would hand the very same block to the next
        # request) and the next allocation is other physical memory -- consecutive draws walk through the device's memory, of
        # which stretches are fast and stretches are slow (twelve draws on one box: 4 slow, 5 fast, 3 slow; NOTES R4-6).
        # Stop at the first buffer the rows stream into at >= 0.70 of the HBM peak -- the fast kind -- else keep the fastest.
        # (Round 3 kept every candidate alive side by side: 4x the row memory; round 2 stopped at "7 % below the slowest
        # seen", which a still slower outlier satisfied for a slow buffer.)
        row_bytes = float(plan.total_rows) * nat.TRAJ_COLS * 8.0
        fast_ms = row_bytes / (self.FAST_ROW_BUFFER_FRACTION_OF_PEAK * self.hbm_peak_bytes_per_s()) * 1e3
        best, times = plan.traj, [timed(plan.traj)]
        best_t = times[0]
        while len(times) < trials and best_t > fast_ms:
            try:
                cand = torch.empty_like(best)
            except RuntimeError:                                 # out of memory: keep what there is
                break
            times.append(timed(cand))                            # (every candidate holds the same rows afterwards)
            if times[-1] < best_t:
                best, best_t = cand, times[-1]
            del cand
            plan.traj = best
            torch.cuda.empty_cache()
        plan.traj = best
        plan.placement_ms = times

    def replan(self, plan: Plan):
        """The whole chain again into plan's buffers -- times + row counts, offsets, solve, sampler (+ yaw column) --
        enqueued by ONE call into the C ABI (`uavac_minsnap_plan_dev`): no allocation, no sync, no Python between
        the four launches.  The buffers keep their size: a plan that would need more rows than `plan.traj` holds is
        refused on the device AS A WHOLE (flag 2, see `take_flags`): every array of the plan keeps what it held, so the
        previous plan stays consistent and flyable.  A rows-free plan (`plan.traj` is None) runs the rows-free chain: times + row
        counts, offsets, solve, first headings -- nothing to refuse.  A `free_times` plan runs the chain from `plan.times` as they
        stand (`uavac_minsnap_plan_t_dev`): change the durations in place, then replan.  Either way `plan.total_rows` is re-read from the device by
        whoever reads it next: the new waypoints may need more rows (rows-free) or fewer (rows that fit) than the old ones."""
        if plan.B == 0:
            return                                               # (`empty_plan`: nothing to plan)
        self._bind_stream()
        # the chain's entry point from (free_times, boundary, velocities): the four take the same buffers behind what they plan from
        head = (_ptr(plan.waypoints), plan.B, plan.m)
        out = (_ptr(plan.seg_rows), _ptr(plan.row_offsets), _ptr(plan.coeffs), _ptr(plan.status), _ptr(plan.traj),
               0 if plan.traj is None else int(plan.traj.shape[0]), _ptr(plan.yaw), _ptr(plan.first_yaw))
        if getattr(plan, "free_times", False):                   # given durations: the chain from plan.times as they stand, never from a speed
            self.ctx.call("uavac_minsnap_plan_t_dev", _ptr(plan.waypoints), None, plan.B, plan.m, _ptr(plan.times), plan.dt, *out)
        elif getattr(plan, "boundary", None) is not None:        # start / end in motion (read from the device at every replan, like the speeds)
            self.ctx.call("uavac_minsnap_plan_bc_dev", *head, _ptr(plan.velocities), plan.dt, _ptr(plan.boundary), _ptr(plan.times), *out)
        elif getattr(plan, "velocities", None) is None:
            self.ctx.call("uavac_minsnap_plan_dev", *head, plan.velocity, plan.dt, _ptr(plan.times), *out)
        else:                                                    # one cruise speed per mission (read from the device at every replan)
            self.ctx.call("uavac_minsnap_plan_v_dev", *head, _ptr(plan.velocities), plan.dt, _ptr(plan.times), *out)
        plan.__dict__["_rows_stale"] = True                      # (no sync here: Plan.total_rows reads it when asked)
        plan.epoch += 1

    def sample_rows(self, plan: Plan, traj=None):
        """Give a rows-free plan (or a rows-free RaggedBatch, `plan_ragged(..., rows=False)`) its rows: allocate (or take `traj`,
        >= plan.total_rows rows) and sample -- the same rows, bit for bit, as `plan(..., rows=True)` would have written."""
        torch = self._torch
        total = int(plan.row_offsets[-1].item())
        if traj is None:
            traj = torch.empty((total, nat.TRAJ_COLS), dtype=torch.float64, device=self.device)
        elif traj.shape[0] < total or traj.dtype != torch.float64 or not traj.is_contiguous():
            raise ValueError("traj must be a contiguous float64 tensor with at least total_rows rows")
        plan.traj, plan.total_rows = traj[:total], total
        s = segments(plan)
        if s.ragged:                                             # a ragged batch: its own sampler entry, segments back to back
            self._bind_stream()
            self.ctx.call("uavac_minsnap_sample_ragged_dev", _ptr(plan.coeffs), _ptr(plan.seg_rows), _ptr(s.so), _ptr(plan.row_offsets),
                          s.B, s.m, s.S, float(plan.dt), _ptr(plan.traj), total, None, None, _ptr(plan.first_yaw))
        else:
            self.sample(plan)
        return plan

    def _coeff_plan(self, plan, refuse: str = None):
        """What the calls that read coefficients and row counts take, as the Plan or RaggedBatch that holds them: a RaggedPlan goes
        through the batch it was sampled from; one without a batch -- `plan_collision_free(device_loop=False)` -- is re-planned
        rows-free from its final waypoints, which gives the same coefficients bit for bit, or, for the calls that cannot work on a
        re-planned copy, refused with a ValueError of the caller's words `refuse`."""
        if not isinstance(plan, RaggedPlan):
            return plan
        if plan.batch is None and refuse is not None:
            raise ValueError(refuse)
        return plan.batch if plan.batch is not None else self.plan_ragged(plan.final_waypoints, plan.velocity, plan.dt, strict=False,
                                                                          rows=False)

    def _first_yaw_of(self, plan, clone: bool = False):
        """The first headings a derived batch carries over: the plan's own (`clone`: a copy of them), or computed when it has none."""
        fy = getattr(plan, "first_yaw", None)
        if fy is None:
            return self.first_yaw(plan)
        return fy.clone() if clone else fy

    def _derived(self, src, *, B, max_m, seg_offsets, seg_offsets_host, seg_rows, row_offsets, coeffs, times, total_rows, first_yaw,
                 status=None, velocities=None):
        """The rows-free RaggedBatch every plan transform returns, assembled like `ragged_from_parts`: no waypoints (it cannot be planned
        again from waypoints; `start_positions` falls back to c0), no rows, `free_times`; velocity and dt are `src`'s; `status` None = ok."""
        if status is None:
            status = self._torch.zeros((B,), dtype=self._torch.int32, device=self.device)
        return RaggedBatch(B, max_m, float(src.velocity), float(src.dt), seg_offsets=seg_offsets, seg_offsets_host=seg_offsets_host,
                           waypoints=None, times=times, seg_rows=seg_rows, row_offsets=row_offsets, coeffs=coeffs, status=status,
                           traj=None, total_rows=total_rows, first_yaw=first_yaw, hit=None, velocities=velocities, free_times=True)

    @staticmethod
    def _plan_args(plan):
        """The leading arguments of those calls: coeffs, seg_rows, seg_offsets (NULL for a uniform Plan), B, m (the largest), dt."""
        s = segments(plan)
        return (_ptr(plan.coeffs), _ptr(plan.seg_rows), _ptr(s.so), s.B, s.m, float(plan.dt))

    def _groups(self, groups, B: int, max_group: int = None):
        """`groups` as the fleet calls take it (None, a group size, or the offsets as array or tensor) -> (the offsets (G + 1,) i64 on the
        device or None, G).  `max_group`: a larger group is refused where its size is known without a sync -- offsets that are a device
        tensor go through."""
        torch = self._torch
        if groups is None:
            if max_group is not None and B > max_group:
                raise ValueError(f"one group of {B} missions; at most {max_group} per group")
            return None, 0
        if isinstance(groups, (int, np.integer)):
            if groups < 1:
                raise ValueError("a group size must be >= 1")
            groups = list(range(0, B, int(groups))) + [B]
        if max_group is not None and not (hasattr(groups, "is_cuda") and groups.is_cuda):
            sizes = np.diff(np.asarray(groups.numpy() if hasattr(groups, "numpy") else groups, dtype=np.int64).reshape(-1))
            if sizes.size and sizes.max() > max_group:
                raise ValueError(f"a group of {int(sizes.max())} missions; at most {max_group} per group")
        go = self._dev(groups, torch.int64).reshape(-1)
        G = int(go.numel()) - 1
        if G < 1:
            raise ValueError("group offsets hold at least two entries")
        return go, G

    def _group_cap(self, groups, B: int, group_cap=None) -> int:
        """The `group_cap` of the searches for groups of any size (`wide=True`): the largest group where the sizes are known without a
        sync -- `groups` None, a group size, or offsets on the host; a `group_cap` below it is a ValueError --, for offsets that are a
        device tensor the caller's `group_cap`, else B."""
        if group_cap is not None and int(group_cap) < 1:
            raise ValueError("group_cap must be >= 1")
        if hasattr(groups, "is_cuda") and groups.is_cuda:
            return B if group_cap is None else int(group_cap)
        if groups is None:
            largest = B
        elif isinstance(groups, (int, np.integer)):
            largest = min(int(groups), B)
        else:
            sizes = np.diff(np.asarray(groups.numpy() if hasattr(groups, "numpy") else groups, dtype=np.int64).reshape(-1))
            largest = max(int(sizes.max()) if sizes.size else 1, 1)
        if group_cap is not None and int(group_cap) < largest:
            raise ValueError(f"a group of {largest} missions; group_cap is {int(group_cap)}")
        return largest

    def _start_rows(self, start_rows, B: int):
        """One start row per mission -> (B,) i32 on the device."""
        start = self._dev(start_rows, self._torch.int32).reshape(-1)
        if start.numel() != B:
            raise ValueError(f"one start row per mission: expected {B}, got {start.numel()}")
        return start

    def first_yaw(self, plan):
        """The missions' first headings from coefficients and row counts alone (`uavac_minsnap_first_yaw_dev`; a Plan or a
        RaggedBatch) -> (B,) f64: bit for bit what the sampler writes into `plan.first_yaw`."""
        torch = self._torch
        out = torch.empty((plan.B,), dtype=torch.float64, device=self.device)
        self._bind_stream()
        self.ctx.call("uavac_minsnap_first_yaw_dev", *self._plan_args(plan), _ptr(out))
        return out

    def audit(self, plan, obstacles=None) -> PlanAudit:
        """What the plan's sampled rows would show, per mission, without sampling them (`uavac_minsnap_audit_dev`): the row total,
        the peaks of horizontal speed, climb and descent rate, horizontal / upward / downward acceleration and speed, and for each
        cuboid of `obstacles` ((n, 6) array or tensor, xmin xmax ymin ymax zmin zmax; n <= 16) how many samples lie inside it and
        which does first.  `plan`: a Plan (with rows or rows-free), a RaggedBatch, or a RaggedPlan (audited from the batch it was
        sampled from; one without a batch -- `plan_collision_free(device_loop=False)` -- is re-planned rows-free from its final
        waypoints, which gives the same coefficients bit for bit).  Reads coefficients and row counts only, never `plan.traj`;
        stream-ordered like the other _dev calls, no sync.  `uav_ac.scoring.plan_feasibility` turns the result into verdicts."""
        torch = self._torch
        plan = self._coeff_plan(plan)
        B = int(plan.B)
        kw = dict(device=self.device)
        cub, n = (None, 0) if obstacles is None else self._cuboids(obstacles, "audit")
        block = torch.empty((nat.AUDIT_ROWS, B), dtype=torch.float64, **kw)
        hit_rows = torch.empty((n, B), dtype=torch.int32, **kw)
        first_hit = torch.empty((n, B), dtype=torch.int32, **kw)
        self._bind_stream()
        self.ctx.call("uavac_minsnap_audit_dev", *self._plan_args(plan), _ptr(cub) if n else None, n, _ptr(block),
                      _ptr(hit_rows) if n else None, _ptr(first_hit) if n else None)
        return PlanAudit(*block.unbind(0), hit_rows, first_hit, block)

    def demand(self, plan, obstacles=None, vehicle: Optional[nat.Vehicle] = None) -> PlanDemand:
        """What the plan asks of the vehicle, per mission, without sampling its rows (`uavac_minsnap_demand_dev`): the largest and the
        least specific thrust a perfectly tracked plan needs, the bank it needs about each axis -- the bank command the control law
        clips to `max_tilt`, which `Engine.audit` does not report and `Engine.retime` bounds only with `demand=True` --, the roll / pitch rate the curve
        demands, the rows that ask for thrust downward, and for each cuboid of `obstacles` (as `Engine.audit` takes them, n <= 16) how
        near the samples pass it and at which row first: the plan-side counterpart of `Engine.flown_audit`'s bank_x, bank_y, body_rate
        and clearance.  `plan`: what `Engine.audit` takes.  `vehicle`: its `g` is used; None = `uavac_vehicle_default`.
        -> PlanDemand, bit for bit what NumPy gives on the sampled rows and jerk (`uav_ac.scoring.demand_from_rows`).  Reads
        coefficients and row counts only, never `plan.traj`; stream-ordered like the other _dev calls, no sync.
        `uav_ac.scoring.demand_feasibility` turns the result into verdicts, `uav_ac.scoring.audit_gap` sets it beside a flight audit."""
        torch = self._torch
        plan = self._coeff_plan(plan)
        B = int(plan.B)
        kw = dict(device=self.device)
        cub, n = (None, 0) if obstacles is None else self._cuboids(obstacles, "demand")
        g = float((nat.Vehicle.default() if vehicle is None else vehicle).g)
        block = torch.empty((nat.DEMAND_ROWS, B), dtype=torch.float64, **kw)
        iblock = torch.empty((nat.IDEMAND_ROWS, B), dtype=torch.int32, **kw)
        clearance = torch.empty((n, B), dtype=torch.float64, **kw)
        clearance_row = torch.empty((n, B), dtype=torch.int32, **kw)
        self._bind_stream()
        self.ctx.call("uavac_minsnap_demand_dev", *self._plan_args(plan), g, _ptr(cub) if n else None, n, _ptr(block), _ptr(iblock),
                      _ptr(clearance) if n else None, _ptr(clearance_row) if n else None)
        return PlanDemand(*block.unbind(0), *iblock.unbind(0), clearance, clearance_row, block)

    @staticmethod
    def _demand_limits(vehicle):
        """The HOST array `demand_limits` of the need calls: g, max_tilt and the specific thrust of four rotors at max_thrust / min_thrust."""
        from .scoring import demand_limits
        return (C.c_double * 4)(*demand_limits(vehicle))

    def need(self, plan, vehicle: Optional[nat.Vehicle] = None) -> PlanNeed:
        """By how much each mission of `plan` must be slowed down for `vehicle` (None = `uavac_vehicle_default`) to be able to give what
        it asks, per limit, without sampling its rows (`uavac_minsnap_need_dev`): the slowdown factor that the tilt bound, the upright
        condition, the largest and the least rotor thrust each ask for on their own -- above 1 where `scoring.demand_feasibility` fails
        the plan on tilt_ok, upright or thrust_ok.  `plan`: what `Engine.audit` takes.  -> PlanNeed, bit for bit what NumPy gives on the
        sampled rows (`uav_ac.scoring.need_from_rows`).  Reads coefficients and row counts only, never `plan.traj`; stream-ordered like
        the other _dev calls, no sync.  `Engine.retime(..., demand=True)` acts on it."""
        torch = self._torch
        plan = self._coeff_plan(plan)
        limits = self._demand_limits(vehicle)
        block = torch.empty((nat.NEED_ROWS, int(plan.B)), dtype=torch.float64, device=self.device)
        self._bind_stream()
        self.ctx.call("uavac_minsnap_need_dev", *self._plan_args(plan), limits, _ptr(block))
        return PlanNeed(*block.unbind(0), block)

    def separation(self, plan, radius: float, groups=None, start_rows=None) -> SeparationAudit:
        """The plan's missions audited against each other (`uavac_minsnap_separation_dev`): per mission the closest approach to any
        other mission of its group, to which one and at which row of the group's shared clock, how many others come inside `radius`
        (metres) and when the first one does -- computed from coefficients and row counts, bit for bit what NumPy gives on the sampled
        rows (`uav_ac.scoring.separation_from_rows`).  `plan`: what `Engine.audit` takes (a Plan with rows or rows-free, a RaggedBatch,
        a RaggedPlan through its batch).  `groups`: None = all missions share one airspace; an int = consecutive groups of that many
        missions (the last one shorter); or the offsets (G + 1,) themselves, ascending from 0 to B (array or tensor).  `start_rows`
        (B,) i32: the clock row at which each mission starts (None: all 0); before it a mission waits on its first row, after its end
        it holds its last.  Never reads `plan.traj`; stream-ordered like the other _dev calls, no sync."""
        B, held, pair_args = self._pair_args(plan, radius, groups, start_rows)      # (`held` keeps the pointers' tensors alive)
        return self._separation_audit("uavac_minsnap_separation_dev", pair_args, B)

    def _traffic_args(self, plan, traffic, traffic_groups, traffic_start_rows, go, G: int):
        """The TRAFFIC of the calls against committed traffic -> (the tensors behind the pointers, the seven arguments of the C calls:
        t_coeffs, t_seg_rows, t_seg_offsets, Bt, mt, t_group_offsets, t_start_rows).  `traffic`: what `Engine.audit` takes, on the
        plan's dt; `traffic_groups` like `groups`, with as many groups as the plan has (`go`, `G`: the plan's, from `_groups`) -- both
        None, or both given; `traffic_start_rows` (Bt,) or None.  Anything else is a ValueError."""
        traffic = self._coeff_plan(traffic)
        if float(traffic.dt) != float(plan.dt):
            raise ValueError(f"the traffic's dt ({float(traffic.dt)}) is not the plan's ({float(plan.dt)}): their rows would not share a clock")
        Bt = int(traffic.B)
        tgo, Gt = self._groups(traffic_groups, Bt)
        if (go is None) != (tgo is None) or G != Gt:
            raise ValueError(f"the plan has {G if go is not None else 1} group(s), the traffic {Gt if tgo is not None else 1}: `groups` and "
                             "`traffic_groups` are both None or hold the same number of groups")
        tstart = None if traffic_start_rows is None else self._start_rows(traffic_start_rows, Bt)
        t = segments(traffic)
        return (traffic, tgo, tstart), (_ptr(traffic.coeffs), _ptr(traffic.seg_rows), _ptr(t.so), t.B, t.m, _ptr(tgo), _ptr(tstart))

    def separation_against(self, plan, traffic, radius: float, groups=None, traffic_groups=None, start_rows=None,
                           traffic_start_rows=None) -> SeparationAudit:
        """The plan's missions audited against ANOTHER plan, committed `traffic` (`uavac_minsnap_separation_against_dev`): per mission
        of `plan` the closest approach to any traffic mission of its group, to which one (`partner` is the TRAFFIC batch index) and at
        which row of the shared clock, how many traffic missions come inside `radius` and when the first one does; `compared` is the
        included traffic of its group.  Missions of `plan` are never compared with each other (`Engine.separation` does that).  Bit
        for bit what NumPy gives on the sampled rows (`uav_ac.scoring.separation_against_rows`).  `plan`, `groups`, `start_rows` as
        `Engine.separation` takes them; `traffic` likewise, with the same `dt` (otherwise ValueError), `traffic_start_rows` (Bt,) or
        None; `traffic_groups` like `groups`: group g of the plan meets group g of the traffic, so both are None (all against all) or
        both hold the same number of groups, otherwise ValueError.  The horizon covers both sides.  A mission whose group has no
        traffic reports +inf / -1 / -1 / 0 / -1 / 0.  Never reads `traj`; stream-ordered, no sync.  This is the audit that confirms
        `Engine.stagger / layer / deconflict(..., traffic=)`."""
        plan = self._coeff_plan(plan)
        B = int(plan.B)
        go, G = self._groups(groups, B)
        start = None if start_rows is None else self._start_rows(start_rows, B)
        held, targs = self._traffic_args(plan, traffic, traffic_groups, traffic_start_rows, go, G)      # (`held` keeps the pointers' tensors alive)
        return self._separation_audit("uavac_minsnap_separation_against_dev",
                                      (*self._plan_args(plan), _ptr(go), G, *targs, _ptr(start), float(radius)), B)

    def _separation_audit(self, call: str, args, B: int) -> SeparationAudit:
        """The planned or the flown separation audit: `call` on its leading arguments `args`, into a fresh result."""
        torch = self._torch
        sep = torch.empty((B,), dtype=torch.float64, device=self.device)
        block = torch.empty((nat.SEP_ROWS, B), dtype=torch.int32, device=self.device)
        self._bind_stream()
        self.ctx.call(call, *args, _ptr(sep), _ptr(block))
        return SeparationAudit(sep, *block.unbind(0), block)

    def _conflict_list(self, offsets_call: str, fill_call: str, args, B: int) -> ConflictList:
        """The planned or the flown conflict list, both calls on their leading arguments `args`: the offsets, ONE small host read (the
        number of entries, to size the result), and the fill, which is skipped without entries."""
        torch = self._torch
        offsets = torch.empty((B + 1,), dtype=torch.int64, device=self.device)
        self._bind_stream()
        self.ctx.call(offsets_call, *args, _ptr(offsets))
        E = int(offsets[B].item())                                       # the one sync
        dist = torch.empty((E,), dtype=torch.float64, device=self.device)
        block = torch.empty((nat.CONF_ROWS, E), dtype=torch.int32, device=self.device)
        if E:
            self.ctx.call(fill_call, *args, _ptr(offsets), E, _ptr(dist), _ptr(block))
        return ConflictList(offsets, *block.unbind(0), dist, E, block)

    def _pair_args(self, plan, radius, groups, start_rows):
        """What `separation` and `conflicts` take, checked once -> (B, the tensors behind the pointers, the arguments of the C call up
        to and with the radius)."""
        plan = self._coeff_plan(plan)
        B = int(plan.B)
        go, G = self._groups(groups, B)
        start = None if start_rows is None else self._start_rows(start_rows, B)
        return B, (plan, go, start), (*self._plan_args(plan), _ptr(go), G, _ptr(start), float(radius))

    def conflicts(self, plan, radius: float, groups=None, start_rows=None) -> ConflictList:
        """Every pair of the plan's missions that `Engine.separation` counts as a conflict, with when and how near
        (`uavac_minsnap_conflict_offsets_dev`, `uavac_minsnap_conflicts_dev`): mission i lists each mission of its group that comes
        inside `radius` at some row of the shared clock, in ascending batch index, with the first and the last row inside, the number
        of rows inside, and the pair's closest approach and its row -- computed from coefficients and row counts, bit for bit what
        NumPy gives on the sampled rows (`uav_ac.scoring.conflicts_from_rows`).  `plan`, `groups` and `start_rows` as
        `Engine.separation` takes them, and on the same inputs diff(offsets) is its `conflicts`, the least `first_row` of a mission
        its `first_conflict`, and its (min_distance, row, partner) the least (min_distance, min_row, partner) of the mission's
        entries.  The two directions of a pair carry the same record (`uav_ac.scoring.conflict_pairs`).  Never reads `plan.traj`.
        ONE small host read: the number of entries, to size the result; without entries the second launch is skipped."""
        B, held, pair_args = self._pair_args(plan, radius, groups, start_rows)      # (`held` keeps the pointers' tensors alive)
        return self._conflict_list("uavac_minsnap_conflict_offsets_dev", "uavac_minsnap_conflicts_dev", pair_args, B)

    def conflicts_against(self, plan, traffic, radius: float, groups=None, traffic_groups=None, start_rows=None,
                          traffic_start_rows=None) -> ConflictList:
        """Every traffic mission that `Engine.separation_against` counts as a conflict of a plan mission, with when and how near
        (`uavac_minsnap_conflict_against_offsets_dev`, `uavac_minsnap_conflicts_against_dev`): mission i of `plan` lists each mission
        of its group's committed `traffic` that comes inside `radius` at some row of the shared clock, in ascending TRAFFIC batch
        index (`partner`), with the first and the last row inside, the number of rows inside, and the pair's closest approach and its
        row -- bit for bit what NumPy gives on the sampled rows (`uav_ac.scoring.conflicts_against_rows`).  Every argument as
        `Engine.separation_against` takes it, with its ValueErrors (another `dt`, unmatched groups), and on the same inputs
        diff(offsets) is its `conflicts`, the least `first_row` of a mission its `first_conflict`, and its (min_distance, row,
        partner) the least (min_distance, min_row, partner) of the mission's entries.  Missions of `plan` are never compared with
        each other (`Engine.conflicts` does that).  `uav_ac.scoring.conflicts_transposed(cl, traffic.B)` is the same list seen from
        the traffic's side.  Never reads `traj`, writes to neither plan.  ONE small host read: the number of entries, to size the
        result; without entries the second launch is skipped.  After `Engine.deconflict(..., traffic=)` this names the committed
        missions that stand in the way of each unresolved arrival."""
        plan = self._coeff_plan(plan)
        B = int(plan.B)
        go, G = self._groups(groups, B)
        start = None if start_rows is None else self._start_rows(start_rows, B)
        held, targs = self._traffic_args(plan, traffic, traffic_groups, traffic_start_rows, go, G)      # (`held` keeps the pointers' tensors alive)
        return self._conflict_list("uavac_minsnap_conflict_against_offsets_dev", "uavac_minsnap_conflicts_against_dev",
                                   (*self._plan_args(plan), _ptr(go), G, *targs, _ptr(start), float(radius)), B)

    def stagger(self, plan, radius: float, groups=None, start_rows=None, step: int = 1, max_steps: int = 255,
                priority=None, wide: bool = False, group_cap=None, airspaces: bool = False, traffic=None, traffic_groups=None,
                traffic_start_rows=None) -> StaggerResult:
        """Prioritised deconfliction by start delay (`uavac_minsnap_stagger_dev`): the call that acts on `Engine.separation`'s
        verdict.  Within a group the missions are taken in ascending batch index -- the lowest index is never delayed --, and each
        gets the smallest start `start_rows[b] + q * step`, q = 0 .. `max_steps`, that keeps it outside `radius` of every mission
        decided before it over the whole shared clock; a mission for which no candidate is clear stays at its base start with
        steps = -1 (two missions that share a first or last waypoint can never be resolved by waiting).  A greedy answer in priority
        order, not a minimum of the total delay.  Exactly what NumPy gives on the sampled rows (`uav_ac.scoring.stagger_from_rows`).
        `plan`, `groups` and `start_rows` (the BASE starts) as `Engine.separation` takes them; a group of more than
        `STAGGER_MAX_GROUP` missions is a ValueError when the groups are given as an int or on the host -- offsets that are a device
        tensor go through, the missions of such a group report steps = -2 and sticky flag 0 is raised (`take_flags`).  Never reads
        `plan.traj`; stream-ordered, no sync.  Confirm with `Engine.separation(plan, radius, groups, start_rows=result.start_rows)`:
        no pair of resolved missions is inside the radius.  To fly the granted starts make them part of the plan:
        `Engine.delay(plan, result.start_rows)` (the rollout's cursor has no start row and needs none).
        `priority` (B,) array or tensor, or None: an order other than the batch index.  Within a group the missions are then taken in
        ascending priority -- a LOWER number goes first, -0.0 ties with +0.0, NaN comes after +inf, ties go to the lower batch index
        (`uavac_fleet_order_dev`, `uav_ac.scoring.priority_order`) --, and "the lowest index is never delayed" becomes "the first of its
        group's order".  A composition: the search runs unchanged on `Engine.take(plan, order)` with `start_rows[order]`, and its answers
        are gathered back, so the result is in the caller's batch order and is exactly `stagger_from_rows` on `take_rows(rows,
        row_offsets, order)` mapped back with `rank`; the one host read is `Engine.take`'s.  None: the call as it always was.
        `wide=True`: groups of ANY size (`uavac_minsnap_stagger_wide_dev`): the same rule and the same integers -- exactly
        `stagger_from_rows(..., max_group=group_cap)` --, decided block by block: per block of 64 missions (ctx option "search_block": 64, 128, 256; same results)
        a chip-wide kernel marks the candidates that meet a mission of an earlier block, then the search above decides the block.
        `group_cap` bounds the largest group: it is taken from `groups` when they are None, an int or on the host; for offsets that are
        a device tensor it is the caller's value, else B -- which costs ceil(B / block) pairs of mostly empty launches, so give it --,
        and a group above it reports steps = -2 and raises sticky flag 0.  `priority` composes unchanged.  `wide=False`: the call as it
        always was, `group_cap` is not looked at.
        `airspaces=True`: the same answers for groups of any size at the cost of the airspaces' sizes, not the groups'.  The groups are
        split into the airspaces of `Engine.airspaces(plan, radius, groups)` -- missions in different ones can never meet, whatever
        their starts --, and a composition like `priority=`'s runs the unchanged search per airspace: `Engine.take(plan, order)`, the
        search on the airspace offsets, the answers gathered back with `rank`.  `start_rows` and `steps` are exactly those of
        `wide=True` on the caller's groups (`stagger_from_rows(..., max_group=B)`); `earlier` counts WITHIN THE AIRSPACE.  The size
        limits now apply to airspaces, not groups: the narrow call when the largest airspace holds at most `STAGGER_MAX_GROUP`
        missions, else the block-wise one with `group_cap` = that size; `wide` and `group_cap` are not looked at.  With `priority` the
        order within an airspace is the priority's.  Host reads: `Engine.airspaces`' and `Engine.take`'s.  False: exactly the native
        calls made without the keyword.
        `traffic`: committed missions that NEVER MOVE (`uavac_minsnap_stagger_against_dev`) -- a second plan (what `Engine.audit`
        takes, on the same `dt`) whose missions have been granted their starts and layers, or are in the air, and around which the
        missions of `plan` are fitted.  A traffic mission stands as planned at `traffic_start_rows[j]` (None: all 0); `traffic_groups`
        like `groups`: group g of the plan meets group g of the traffic, so both are None or hold the same number of groups.  One
        more clause in "clear": the candidate is also outside `radius` of every traffic mission of its group over the whole shared
        clock; `earlier` counts the group's traffic plus the plan's missions before it, and the first mission of a group is examined
        whenever its group has traffic.  Exactly `uav_ac.scoring.stagger_against_rows(..., max_group=group_cap)`; a group without
        traffic answers as `wide=True` does.  Always the block-wise form: `wide` is not looked at, `group_cap` works as for
        `wide=True`, and the cost is arrivals x (traffic + earlier arrivals), not all x all.  Nothing of the traffic is decided or
        written: two traffic missions that conflict with each other stay as they are.  `priority` composes as before -- the plan is
        taken in order, the traffic is untouched.  Confirm with `Engine.separation_against(plan, traffic, radius, ...,
        start_rows=result.start_rows)`.  `airspaces=True` together with `traffic` is a ValueError (airspaces are not labelled across
        two plans), and so are a different `dt` and group counts that do not match.  None: exactly the native calls made without
        the keyword."""
        against = dict(traffic=traffic, traffic_groups=traffic_groups, traffic_start_rows=traffic_start_rows)
        if airspaces:
            if traffic is not None:
                raise ValueError("airspaces=True does not take traffic: airspaces are not labelled across two plans")
            taken, rank, start, route = self._airspace_front(plan, radius, groups, None, priority, start_rows)
            return self._stagger_back(self.stagger(taken, radius, start_rows=start, step=step, max_steps=max_steps, **route), rank)
        wide = wide or traffic is not None
        if priority is not None:
            B = int(self._coeff_plan(plan).B)
            order, rank, start = self._priority_order(priority, groups, B, None if wide else nat.STAGGER_MAX_GROUP, start_rows)
            return self._stagger_back(self.stagger(self.take(plan, order), radius, groups, start, step, max_steps, wide=wide,
                                                   group_cap=group_cap, **against), rank)
        torch = self._torch
        plan = self._coeff_plan(plan)
        B = int(plan.B)
        step, max_steps = int(step), int(max_steps)
        if step < 1:
            raise ValueError("step must be >= 1")
        if not (0 <= max_steps <= nat.STAGGER_MAX_STEPS):
            raise ValueError(f"max_steps must be in 0 .. {nat.STAGGER_MAX_STEPS}")
        if step * max_steps > 2 ** 29:
            raise ValueError("step * max_steps must not exceed 2^29 rows")
        cap = self._group_cap(groups, B, group_cap) if wide else None
        go, G = self._groups(groups, B, None if wide else nat.STAGGER_MAX_GROUP)
        start = None if start_rows is None else self._start_rows(start_rows, B)
        block = torch.empty((nat.STAGGER_ROWS, B), dtype=torch.int32, device=self.device)
        if traffic is not None:
            held, targs = self._traffic_args(plan, traffic, traffic_groups, traffic_start_rows, go, G)      # (`held` keeps the tensors alive)
            self._bind_stream()
            self.ctx.call("uavac_minsnap_stagger_against_dev", *self._plan_args(plan), _ptr(go), G, *targs, cap, _ptr(start), float(radius),
                          step, max_steps, _ptr(block))
            return StaggerResult(*block.unbind(0), block)
        self._bind_stream()
        if wide:
            self.ctx.call("uavac_minsnap_stagger_wide_dev", *self._plan_args(plan), _ptr(go), G, cap, _ptr(start), float(radius), step,
                          max_steps, _ptr(block))
            return StaggerResult(*block.unbind(0), block)
        self.ctx.call("uavac_minsnap_stagger_dev", *self._plan_args(plan), _ptr(go), G, _ptr(start), float(radius), step, max_steps,
                      _ptr(block))
        return StaggerResult(*block.unbind(0), block)

    def delay(self, plan, start_rows, rows: bool = False) -> RaggedBatch:
        """Start delays as part of the plan (`uavac_minsnap_delay_dev`): every mission with start row S > 0 gets a leading HOLD segment
        -- c0 of its first segment, c1 .. c7 = 0, S rows, duration S * dt -- and keeps its own segments unchanged; a mission with S = 0
        is copied as it is.  The sampler then writes S hold rows (the first position, zero velocity and acceleration, the mission's
        first heading, spline id 0) followed by the original rows bit for bit (`uav_ac.scoring.delay_rows`), and
        `Engine.separation(delayed, radius, groups)` equals `Engine.separation(plan, radius, groups, start_rows=start_rows)` bit for
        bit.  `plan`: what `Engine.separation` takes (a Plan with rows or rows-free, a RaggedBatch, a RaggedPlan through its batch);
        it is left as it is.  `start_rows` (B,) array or tensor, e.g. `StaggerResult.start_rows`; one outside 0 .. 2^29 is clamped and
        raises sticky flag 0 (`take_flags`).  A plan that starts in motion (`boundary=`) is accepted: its hold stands still and its
        first own row moves, which is what the audit's clock means by "waits on its first row" too.
        -> a rows-free RaggedBatch (`rows=True`: with rows, through `sample_rows`) of at most m + 1 segments per mission, assembled like
        `ragged_from_parts`: `waypoints` None (it cannot be re-planned from waypoints; `start_positions` falls back to c0),
        `free_times` True, `first_yaw` the input's (`Engine.first_yaw(plan)` if it carries none), velocity and dt carried over.
        `eng.fleet(delayed)` and `fleet.follow(delayed)` fly it plan-fed like any rows-free ragged batch; `fleet.tracking()` scores the
        hold rows like any others.  ONE host sync: the read of the (B + 1,) segment offsets (with the row total), which a RaggedBatch
        carries on the host.  A plan whose missions already have UAVAC_MAX_SEGMENTS segments is a ValueError."""
        torch = self._torch
        plan = self._coeff_plan(plan)
        s = segments(plan)
        B, m, S_in, so_in = s.B, s.m, s.S, _ptr(s.so)
        if m >= nat.MAX_SEGMENTS:
            raise ValueError(f"a mission of {m} segments cannot take a hold segment: at most {nat.MAX_SEGMENTS} per mission")
        start = self._start_rows(start_rows, B)
        kw = dict(device=self.device)
        # (buffers for the largest result, S_in + B segments, narrowed once the offsets are known: the one read comes last)
        tail = torch.empty((B + 2,), dtype=torch.int64, **kw)            # the segment offsets (B + 1,) and, behind them, the row total
        co = torch.empty((S_in + B, 8, 3), dtype=torch.float64, **kw)
        sr = torch.empty((S_in + B,), dtype=torch.int32, **kw)
        tm = None if plan.times is None else torch.empty((S_in + B,), dtype=torch.float64, **kw)
        row_offsets = torch.empty((B + 1,), dtype=torch.int64, **kw)
        first_yaw = self._first_yaw_of(plan, clone=True)
        self._bind_stream()
        self.ctx.call("uavac_minsnap_delay_offsets_dev", so_in, B, m, _ptr(start), _ptr(tail))
        self.ctx.call("uavac_minsnap_delay_dev", _ptr(plan.coeffs), _ptr(plan.times), _ptr(plan.seg_rows), so_in, B, m, float(plan.dt),
                      _ptr(start), _ptr(tail), _ptr(co), _ptr(tm), _ptr(sr))
        self.ctx.call("uavac_minsnap_row_offsets_ragged_dev", _ptr(sr), _ptr(tail), B, m + 1, _ptr(row_offsets))
        tail[B + 1:].copy_(row_offsets[B:])
        host = tail.cpu().numpy()                                        # the one sync
        S = int(host[B])
        out = self._derived(plan, B=B, max_m=m + 1, seg_offsets=tail[:B + 1], seg_offsets_host=host[:B + 1].copy(), seg_rows=sr[:S],
                            row_offsets=row_offsets, coeffs=co[:S], times=None if tm is None else tm[:S], total_rows=int(host[B + 1]),
                            first_yaw=first_yaw)
        return self.sample_rows(out) if rows else out

    def layer(self, plan, radius: float, groups=None, start_rows=None, delta=(0.0, 0.0, -0.5), max_steps: int = 63,
              obstacles=None, priority=None, wide: bool = False, group_cap=None, airspaces: bool = False, traffic=None,
              traffic_groups=None, traffic_start_rows=None) -> LayerResult:
        """Prioritised deconfliction by offset (`uavac_minsnap_layer_dev`): the second lever on `Engine.separation`'s verdict, for the
        conflicts that waiting cannot resolve (a shared first or last waypoint, a crossing of a busy region).  `start_rows` are FIXED
        starts -- `StaggerResult.start_rows`, for instance; nobody is delayed by this call.  Within a group the missions are taken in
        ascending batch index -- the lowest index is never moved --, and each gets the lowest layer q = 0 .. `max_steps` -- the mission
        with q * `delta` (three finite metres, NED: a negative z is UP; any direction is allowed) added to c0 of every segment -- that
        keeps it outside `radius` of every mission decided before it, on its granted layer, over the whole shared clock; a mission for
        which no layer is clear stays on layer 0 with steps = -1.  A greedy answer in priority order, not a minimum of the total
        displacement.  Exactly what NumPy gives on the sampled rows of the shifted plans (`uav_ac.scoring.layer_from_rows`).
        `plan` and `groups` as `Engine.stagger` takes them, with the same limit of `LAYER_MAX_GROUP` missions per group.  Never reads
        `plan.traj`; stream-ordered, no sync.  Make the result part of the plan with `Engine.shift(plan, result.offsets)`;
        `Engine.separation(shifted, radius, groups, start_rows)` then finds no pair of resolved missions inside the radius.  The search
        knows nothing about obstacles unless obstacles are given: run `Engine.audit(shifted, obstacles)` again, a layer can move a
        mission into a cuboid.
        `obstacles` ((n, 6) array or tensor as `Engine.audit` takes it, n <= 16; zero rows are allowed): the search with obstacles
        (`uavac_minsnap_layer_obs_dev`, `uav_ac.scoring.layer_obstacles_from_rows`).  A layer on which any sampled row of the mission's
        own lies inside a cuboid is refused before it is compared with anybody; every included mission is examined, the first of its
        group too, which is then moved only by a cuboid; `result.block` is (4, B) and `result.blocked` counts the refused layers below
        the granted one (all of them for an unresolved mission).  `Engine.audit(shifted, obstacles).hit_rows` is then 0 for every
        resolved mission.  steps = -1 with blocked = max_steps + 1 (`uav_ac.scoring.blocked_out`): every layer hits a cuboid, the
        mission needs a new plan around the obstacle (`plan_collision_free`), not an offset.
        `priority` (B,) array or tensor, or None: an order other than the batch index, by the rule and the composition of
        `Engine.stagger` -- a lower number goes first, ties to the lower batch index; "the lowest index is never moved" becomes "the
        first of its group's order"; the search runs unchanged on `Engine.take(plan, order)` with `start_rows[order]`, and `block`
        (column-wise) and `offsets` (row-wise) are gathered back into the caller's batch order.  Exactly `layer_from_rows` /
        `layer_obstacles_from_rows` on `take_rows(...)` of the shifted plans' rows, mapped back with `rank`.  The one host read is
        `Engine.take`'s.  None: the call as it always was.
        `wide=True`, `group_cap`: groups of any size (`uavac_minsnap_layer_wide_dev`), as in `Engine.stagger`: the same rule, exactly
        `layer_obstacles_from_rows(..., max_group=group_cap)`.  The one kernel is the search with obstacles: `result.block` is (4, B)
        whether `obstacles` are given or not, and without them `blocked` is all 0 and rows 0-2 are `layer_from_rows`'.
        `airspaces=True`: as in `Engine.stagger`, with the airspaces of `Engine.airspaces(plan, radius, groups, reach=max_steps * delta)`:
        the boxes cover every layer 0 .. `max_steps`, so missions in different airspaces can never meet whatever layers they are
        granted.  `layers`, `steps`, `blocked` and `offsets` are exactly those of `wide=True` on the caller's groups; `earlier` counts
        within the airspace; the limit `LAYER_MAX_GROUP` applies to airspaces (above it the block-wise search with `group_cap` = the
        largest airspace, whose block is (4, B); below it the narrow calls, (3, B) without `obstacles`).
        `traffic`, `traffic_groups`, `traffic_start_rows`: committed missions that never move (`uavac_minsnap_layer_against_dev`), as
        in `Engine.stagger`: a candidate layer must also be outside `radius` of every traffic mission of its group, which is compared
        AS IT IS, on no layer, at its own start row -- pass the plan the traffic flies, shifted and delayed if it was.  Exactly
        `uav_ac.scoring.layer_against_rows(..., max_group=group_cap)`; always the block-wise form with the cuboid policy (`block` is
        (4, B), `wide` is not looked at); `earlier` counts the group's traffic too; `priority` composes unchanged; `airspaces=True`
        with `traffic`, another `dt` and group counts that do not match are ValueErrors."""
        against = dict(traffic=traffic, traffic_groups=traffic_groups, traffic_start_rows=traffic_start_rows)
        if airspaces:
            if traffic is not None:
                raise ValueError("airspaces=True does not take traffic: airspaces are not labelled across two plans")
            taken, rank, start, route = self._airspace_front(plan, radius, groups, self._layer_reach(delta, max_steps), priority, start_rows)
            return self._layer_back(self.layer(taken, radius, start_rows=start, delta=delta, max_steps=max_steps, obstacles=obstacles, **route),
                                    rank)
        wide = wide or traffic is not None
        if priority is not None:
            B = int(self._coeff_plan(plan).B)
            order, rank, start = self._priority_order(priority, groups, B, None if wide else nat.LAYER_MAX_GROUP, start_rows)
            return self._layer_back(self.layer(self.take(plan, order), radius, groups, start, delta, max_steps, obstacles, wide=wide,
                                               group_cap=group_cap, **against), rank)
        torch = self._torch
        plan = self._coeff_plan(plan)
        B = int(plan.B)
        max_steps = int(max_steps)
        if not (0 <= max_steps <= nat.LAYER_MAX_STEPS):
            raise ValueError(f"max_steps must be in 0 .. {nat.LAYER_MAX_STEPS}")
        d = np.asarray(delta.detach().cpu().numpy() if hasattr(delta, "detach") else delta, dtype=np.float64).reshape(-1)
        if d.size != 3 or not np.isfinite(d).all():
            raise ValueError("delta must be three finite numbers")
        cap = self._group_cap(groups, B, group_cap) if wide else None
        go, G = self._groups(groups, B, None if wide else nat.LAYER_MAX_GROUP)
        start = None if start_rows is None else self._start_rows(start_rows, B)
        offsets = torch.empty((B, 3), dtype=torch.float64, device=self.device)
        if wide:
            cub, n = (None, 0) if obstacles is None else self._cuboids(obstacles, "search")
            block = torch.empty((nat.LAYER_OBS_ROWS, B), dtype=torch.int32, device=self.device)
            if traffic is not None:
                held, targs = self._traffic_args(plan, traffic, traffic_groups, traffic_start_rows, go, G)      # (`held` keeps the tensors alive)
                self._bind_stream()
                self.ctx.call("uavac_minsnap_layer_against_dev", *self._plan_args(plan), _ptr(go), G, *targs, cap, _ptr(start), float(radius),
                              float(d[0]), float(d[1]), float(d[2]), max_steps, _ptr(cub) if n else None, n, _ptr(block), _ptr(offsets))
                return LayerResult(*block[:nat.LAYER_ROWS].unbind(0), block, offsets)
            self._bind_stream()
            self.ctx.call("uavac_minsnap_layer_wide_dev", *self._plan_args(plan), _ptr(go), G, cap, _ptr(start), float(radius), float(d[0]),
                          float(d[1]), float(d[2]), max_steps, _ptr(cub) if n else None, n, _ptr(block), _ptr(offsets))
            return LayerResult(*block[:nat.LAYER_ROWS].unbind(0), block, offsets)
        if obstacles is not None:
            cub, n = self._cuboids(obstacles, "search")
            block = torch.empty((nat.LAYER_OBS_ROWS, B), dtype=torch.int32, device=self.device)
            self._bind_stream()
            self.ctx.call("uavac_minsnap_layer_obs_dev", *self._plan_args(plan), _ptr(go), G, _ptr(start), float(radius), float(d[0]),
                          float(d[1]), float(d[2]), max_steps, _ptr(cub) if n else None, n, _ptr(block), _ptr(offsets))
            return LayerResult(*block[:nat.LAYER_ROWS].unbind(0), block, offsets)
        block = torch.empty((nat.LAYER_ROWS, B), dtype=torch.int32, device=self.device)
        self._bind_stream()
        self.ctx.call("uavac_minsnap_layer_dev", *self._plan_args(plan), _ptr(go), G, _ptr(start), float(radius), float(d[0]), float(d[1]),
                      float(d[2]), max_steps, _ptr(block), _ptr(offsets))
        return LayerResult(*block.unbind(0), block, offsets)

    def shift(self, plan, offsets, rows: bool = False) -> RaggedBatch:
        """Offsets as part of the plan (`uavac_minsnap_shift_dev`): every segment of mission b gets c0' = c0 + offsets[b] (one rounded
        sum per axis); c1 .. c7, the durations, the row counts and the first headings keep every bit, and so does a mission whose three
        offsets are all zero (`uav_ac.scoring.shift_coeffs`).  The sampled rows of the result differ from the input's in columns 0:3
        only.  `offsets` (B, 3) array or tensor, e.g. `LayerResult.offsets`; non-finite ones pass through, and the mission then counts as
        excluded downstream like any non-finite plan.  `plan`: what `Engine.delay` takes (a Plan with rows or rows-free, a RaggedBatch,
        a RaggedPlan through its batch); it is left as it is.
        -> a rows-free RaggedBatch (`rows=True`: with rows, through `sample_rows`) with the input's segment counts, assembled like
        `ragged_from_parts`: `waypoints` None (`start_positions` falls back to c0, the SHIFTED first waypoint), `free_times` True,
        `first_yaw` the input's (`Engine.first_yaw(plan)` if it carries none), velocity and dt carried over.  `eng.fleet(shifted)`,
        `fleet.follow(shifted)` and `Engine.delay(shifted, starts)` work unchanged.  No host sync: the segment counts and the row total
        are on the host already.  The OBSTACLE AUDIT has to be re-run on the result (`Engine.audit(shifted, obstacles)`): an offset
        can move a mission into a cuboid that the original plan avoided."""
        torch = self._torch
        plan = self._coeff_plan(plan)
        s = segments(plan)
        B, m, S = s.B, s.m, s.S
        off = self._dev(offsets, torch.float64).reshape(-1)
        if off.numel() != 3 * B:
            raise ValueError(f"one offset (x, y, z) per mission: expected ({B}, 3), got {off.numel()} numbers")
        off = off.contiguous()
        so = s.so.clone() if s.ragged else uniform_offsets(B, m, self.device)
        src = plan.coeffs.reshape(S, 8, 3)
        co = torch.empty((S, 8, 3), dtype=torch.float64, device=self.device)
        first_yaw = self._first_yaw_of(plan, clone=True)
        self._bind_stream()
        self.ctx.call("uavac_minsnap_shift_dev", _ptr(src), _ptr(s.so), B, m, S, _ptr(off), _ptr(co))
        out = self._derived(plan, B=B, max_m=m, seg_offsets=so, seg_offsets_host=np.array(s.so_host, dtype=np.int64),
                            seg_rows=plan.seg_rows.reshape(-1).clone(), row_offsets=plan.row_offsets.clone(), coeffs=co,
                            times=None if plan.times is None else plan.times.reshape(-1).clone(), total_rows=int(plan.total_rows),
                            first_yaw=first_yaw)
        return self.sample_rows(out) if rows else out

    def _take_index(self, index, B: int):
        """What `Engine.take` selects -> (n,) i32 on the device.  `index`: integers (array, list or tensor), or a boolean mask of one
        entry per mission, which is turned into the indices of its True entries (a mask on the device costs one small read: their
        number).  Checked where it is on the host: an empty selection, a mask of another length, numbers that are not integers and an
        index outside 0 .. B - 1 are ValueErrors; the indices of a device tensor go through unread."""
        torch = self._torch
        t = index if isinstance(index, torch.Tensor) else torch.as_tensor(np.asarray(index))
        t = t.reshape(-1)
        if t.numel() < 1:
            raise ValueError("an empty selection: take needs at least one mission")
        if t.dtype == torch.bool:
            if t.numel() != B:
                raise ValueError(f"a mask holds one entry per mission: expected {B}, got {t.numel()}")
            t = torch.nonzero(t).reshape(-1)
        elif t.is_floating_point() or t.is_complex():
            raise ValueError("index must hold integers or be a boolean mask")
        if t.numel() < 1:
            raise ValueError("an empty selection: take needs at least one mission")
        if not t.is_cuda and (int(t.min()) < 0 or int(t.max()) >= B):
            raise ValueError(f"index must be in 0 .. {B - 1}")
        return t.to(device=self.device, dtype=torch.int32).contiguous()

    def take(self, plan, index, rows: bool = False) -> RaggedBatch:
        """Missions of a plan selected on the device (`uavac_minsnap_take_dev`): mission i of the result is mission `index[i]` of `plan`,
        every bit of it -- coefficients, durations, row counts, first heading (`uav_ac.scoring.take_parts`), so its sampled rows are
        that mission's rows bit for bit (`uav_ac.scoring.take_rows`), `Engine.audit` of the result is the audit's columns `index`,
        and a group taken whole is audited, staggered and layered as it was inside its batch.  `index` (n,) integers, array or tensor:
        any order, duplicates allowed, n may exceed B; or a boolean (B,) mask, e.g. `~result.resolved`, which selects its True entries
        in ascending order.  An index outside 0 .. B - 1 is a ValueError where the index is on the host; in a device tensor it is
        clamped into range and raises sticky flag 0 (`take_flags`).  An empty selection is a ValueError.  `plan`: what `Engine.delay`
        takes (a Plan with rows or rows-free, a RaggedBatch, a RaggedPlan through its batch); it is left as it is.
        -> a rows-free RaggedBatch (`rows=True`: with rows, through `sample_rows`) of n missions, assembled like `Engine.delay`'s:
        `waypoints` None (`start_positions` falls back to c0), `free_times` True, `max_m` the input's, velocity and dt carried over,
        `first_yaw` gathered (from `Engine.first_yaw(plan)` if the input carries none), `status` and `velocities` gathered when
        present.  ONE host sync: the read of the (n + 1,) segment offsets with the row total, as in `Engine.delay` (a mask on the
        device adds the read of its count)."""
        torch = self._torch
        plan = self._coeff_plan(plan)
        s = segments(plan)
        B, m, so_in = s.B, s.m, _ptr(s.so)
        idx = self._take_index(index, B)
        n = int(idx.numel())
        kw = dict(device=self.device)
        cap = n * m                                                      # (buffers for the largest result, narrowed once the offsets are known)
        tail = torch.empty((n + 2,), dtype=torch.int64, **kw)            # the segment offsets (n + 1,) and, behind them, the row total
        co = torch.empty((cap, 8, 3), dtype=torch.float64, **kw)
        sr = torch.empty((cap,), dtype=torch.int32, **kw)
        tm = None if plan.times is None else torch.empty((cap,), dtype=torch.float64, **kw)
        row_offsets = torch.empty((n + 1,), dtype=torch.int64, **kw)
        fy_in = self._first_yaw_of(plan)
        first_yaw = torch.empty((n,), dtype=torch.float64, **kw)
        self._bind_stream()
        self.ctx.call("uavac_minsnap_take_offsets_dev", so_in, B, m, _ptr(idx), n, _ptr(tail))
        self.ctx.call("uavac_minsnap_take_dev", _ptr(plan.coeffs), _ptr(plan.times), _ptr(plan.seg_rows), so_in, B, m, _ptr(fy_in),
                      _ptr(idx), n, _ptr(tail), _ptr(co), _ptr(tm), _ptr(sr), _ptr(first_yaw))
        self.ctx.call("uavac_minsnap_row_offsets_ragged_dev", _ptr(sr), _ptr(tail), n, m, _ptr(row_offsets))
        tail[n + 1:].copy_(row_offsets[n:])
        at = idx.clamp(0, B - 1).long()                                  # (as the kernel clamps it)
        status = plan.status[at] if getattr(plan, "status", None) is not None else None
        velocities = plan.velocities[at] if getattr(plan, "velocities", None) is not None else None
        host = tail.cpu().numpy()                                        # the one sync
        S = int(host[n])
        out = self._derived(plan, B=n, max_m=m, seg_offsets=tail[:n + 1], seg_offsets_host=host[:n + 1].copy(), seg_rows=sr[:S],
                            row_offsets=row_offsets, coeffs=co[:S], times=None if tm is None else tm[:S], total_rows=int(host[n + 1]),
                            first_yaw=first_yaw, status=status, velocities=velocities)
        return self.sample_rows(out) if rows else out

    def concat(self, plans) -> RaggedBatch:
        """The missions of several plans back to back in one batch -- plumbing (`torch.cat` of the per-segment arrays with the offsets
        moved up; a uniform Plan contributes offsets of arange * m), no kernel, no host sync.  `plans`: a sequence of what
        `Engine.delay` takes; every part is left as it is.  All parts must have the same `dt`, otherwise ValueError.
        -> a rows-free RaggedBatch assembled like `Engine.delay`'s (`waypoints` None, `free_times` True): `max_m` the largest of the
        parts', `times` kept iff every part has them, `first_yaw` and `status` joined (`Engine.first_yaw(part)` / zeros for a part
        that carries none), `velocity` the common value -- or NaN with `velocities` filled in, when the parts differ or one of them
        has a speed per mission."""
        torch = self._torch
        parts = [self._coeff_plan(p) for p in plans]
        if not parts:
            raise ValueError("concat needs at least one plan")
        dts = {float(p.dt) for p in parts}
        if len(dts) != 1:
            raise ValueError(f"the plans differ in dt ({sorted(dts)}): their rows would not share a clock")
        kw = dict(device=self.device)
        views = [segments(p) for p in parts]
        so, so_host, counts, base = [], [], [], 0
        for p, s in zip(parts, views):
            part = s.so.to(dtype=torch.int64, **kw) if s.ragged else uniform_offsets(s.B, s.m, self.device)
            so.append(part[:-1] + base), so_host.append(np.asarray(s.so_host[:-1], dtype=np.int64) + base)
            base += s.S
            counts.append(p.row_offsets[1:] - p.row_offsets[:-1])
        so = torch.cat(so + [torch.full((1,), base, dtype=torch.int64, **kw)])
        so_host = np.concatenate(so_host + [np.array([base], dtype=np.int64)])
        row_offsets = torch.cat([torch.zeros((1,), dtype=torch.int64, **kw), torch.cumsum(torch.cat(counts), 0)])
        times = torch.cat([p.times.reshape(-1) for p in parts]) if all(p.times is not None for p in parts) else None
        first_yaw = torch.cat([self._first_yaw_of(p) for p in parts])
        status = torch.cat([p.status.to(torch.int32) if getattr(p, "status", None) is not None else torch.zeros((p.B,), dtype=torch.int32, **kw)
                            for p in parts])
        out = self._derived(parts[0], B=sum(s.B for s in views), max_m=max(s.m for s in views), seg_offsets=so, seg_offsets_host=so_host,
                            seg_rows=torch.cat([p.seg_rows.reshape(-1) for p in parts]), row_offsets=row_offsets,
                            coeffs=torch.cat([p.coeffs.reshape(-1, 8, 3) for p in parts]), times=times,
                            total_rows=sum(int(p.total_rows) for p in parts), first_yaw=first_yaw, status=status)
        speeds = {float(p.velocity) for p in parts}
        per_mission = any(getattr(p, "velocities", None) is not None for p in parts)
        if per_mission or (len(speeds) != 1 and not all(np.isnan(v) for v in speeds)):      # no common speed: one per mission
            out.velocity = float("nan")
            out.velocities = torch.cat([p.velocities if getattr(p, "velocities", None) is not None
                                        else torch.full((p.B,), float(p.velocity), dtype=torch.float64, **kw) for p in parts])
        return out

    def _put_index(self, index, B: int, n: int) -> np.ndarray:
        """Where `Engine.put` puts the n missions of `other` -> (n,) i64 on the host, checked: integers (or a boolean (B,) mask with n
        True entries), one per mission of `other`, in 0 .. B - 1, no index twice.  A device tensor costs one small read."""
        a = np.asarray(index.detach().cpu().numpy() if hasattr(index, "detach") else index).reshape(-1)
        if a.dtype == np.bool_:
            if a.size != B:
                raise ValueError(f"a mask holds one entry per mission: expected {B}, got {a.size}")
            a = np.flatnonzero(a)
        elif not np.issubdtype(a.dtype, np.integer):
            raise ValueError("index must hold integers or be a boolean mask")
        a = a.astype(np.int64)
        if a.size != n:
            raise ValueError(f"one index per mission of `other`: expected {n}, got {a.size}")
        if a.size and (a.min() < 0 or a.max() >= B):
            raise ValueError(f"index must be in 0 .. {B - 1}")
        if np.unique(a).size != a.size:
            raise ValueError("index must not name a mission twice")
        return a

    def put(self, plan, index, other, rows: bool = False) -> RaggedBatch:
        """`plan` with mission `index[i]` replaced by mission i of `other` -- how re-planned missions go back into a fleet's plan:
        `take(concat([plan, other]), sel)` with sel = arange(B), sel[index] = B + arange(n).  Every mission of the result is, bit for
        bit, `other`'s at `index` and `plan`'s elsewhere.  `index` (n,) unique integers in 0 .. B - 1, n = other.B, array or tensor
        (or a boolean (B,) mask with n True entries, e.g. `~result.resolved`): checked on the host, with one small read when it is a
        device tensor; anything else is a ValueError.  `plan` and `other`: what `Engine.delay` takes, with the same `dt`; both are
        left as they are.  -> a rows-free RaggedBatch as `Engine.take` returns it (`rows=True`: with rows); the host sync is `take`'s."""
        plan, other = self._coeff_plan(plan), self._coeff_plan(other)
        B, n = int(plan.B), int(other.B)
        at = self._put_index(index, B, n)
        sel = np.arange(B, dtype=np.int64)
        sel[at] = B + np.arange(n, dtype=np.int64)
        return self.take(self.concat([plan, other]), sel, rows=rows)

    def envelope(self, plan, reach=None) -> PlanEnvelope:
        """Every mission's swept box without sampling its rows (`uavac_minsnap_envelope_dev`): the minimum and the maximum per axis of
        the positions the sampler writes -- as numbers exactly `uav_ac.scoring.envelope_from_rows` on the sampled rows.  `reach`: None, a
        (3,) vector for every mission or a (B, 3) array or tensor: the box is then the hull of the plan's rows and of the rows of
        `Engine.shift(plan, reach)`, and holds every layer in between (`reach = max_steps * delta` of a layer search).  `plan`: what
        `Engine.audit` takes.  A mission without rows or with a position that is not finite reports NaN in all six.  Never reads
        `plan.traj`; stream-ordered, no sync."""
        torch = self._torch
        plan = self._coeff_plan(plan)
        B = int(plan.B)
        r = None
        if reach is not None:
            r = self._dev(reach, torch.float64)
            if r.numel() == 3:
                r = r.reshape(1, 3).expand(B, 3)
            elif r.numel() != 3 * B or (r.dim() == 2 and tuple(r.shape) != (B, 3)):
                raise ValueError(f"reach is (3,) or ({B}, 3), got {tuple(r.shape)}")
            r = r.reshape(B, 3).contiguous()
        block = torch.empty((B, 6), dtype=torch.float64, device=self.device)
        self._bind_stream()
        self.ctx.call("uavac_minsnap_envelope_dev", *self._plan_args(plan), _ptr(r), _ptr(block))
        return PlanEnvelope(block[:, :3], block[:, 3:], block)

    def airspaces(self, plan, radius: float, groups=None, reach=None, rounds: int = 32) -> Airspaces:
        """The fleet split into groups of missions that can never come inside `radius` of each other, whatever their starts -- and,
        with `reach` = max_steps * delta, whatever layers 0 .. max_steps they are granted: the connected components, within each of
        the caller's `groups`, of "the swept boxes are nearer than `radius` on every axis" (`uavac_fleet_airspaces_dev` on
        `Engine.envelope(plan, reach)`; `uav_ac.scoring.airspaces_from_envelopes`).  The prioritised searches run per airspace, on
        the missions in their original relative order, give every mission the answer of the search over its whole group:
        `Engine.stagger / layer / deconflict(..., airspaces=True)` do that.
        A chain on the device: the boxes, the labels (`rounds` rounds per call), `uavac_fleet_order_dev` with the labels as
        priorities (exact in float64; stable, so an airspace keeps its order), the boundaries where the label changes.  ONE small
        host read covers the labelling's verdict and the boundaries, on the footing of `Engine.take`'s; while the labels are not final
        the labelling is called again where it stopped and the read repeated -- labels that are not final never leave this call.
        `plan` and `groups` as `Engine.stagger` takes them (any group size).  -> Airspaces."""
        torch = self._torch
        plan = self._coeff_plan(plan)
        B = int(plan.B)
        radius, rounds = float(radius), int(rounds)
        if not (np.isfinite(radius) and radius >= 0.0):
            raise ValueError("radius must be finite and >= 0")
        if rounds < 1:
            raise ValueError("rounds must be >= 1")
        go, G = self._groups(groups, B)
        env = self.envelope(plan, reach)
        kw = dict(dtype=torch.int32, device=self.device)
        labels, order, rank = (torch.empty((B,), **kw) for _ in range(3))
        tail = torch.empty((2 + B,), **kw)                               # info, and behind it: does an airspace begin in this slot?
        self._bind_stream()
        changed, resume = 0, 0
        while True:
            self.ctx.call("uavac_fleet_airspaces_dev", _ptr(env.block), _ptr(go), G, B, radius, rounds, resume, _ptr(labels), _ptr(tail))
            keys = labels.to(torch.float64)
            self.ctx.call("uavac_fleet_order_dev", _ptr(keys), _ptr(go), G, B, _ptr(order), _ptr(rank))
            sorted_labels = labels[order.long()]
            tail[2] = 1
            tail[3:] = (sorted_labels[1:] != sorted_labels[:-1]).to(torch.int32)
            host = tail.cpu().numpy()                                    # the one read (per labelling call)
            changed += int(host[0])
            if host[1]:
                break
            resume = 1
        offsets_host = np.concatenate([np.flatnonzero(host[2:]), [B]]).astype(np.int64)
        sizes = np.diff(offsets_host)
        return Airspaces(labels, order, rank, torch.as_tensor(offsets_host).to(self.device), offsets_host, sizes, int(sizes.max()), changed)

    NARROW_SEARCH = min(nat.STAGGER_MAX_GROUP, nat.LAYER_MAX_GROUP)     # the largest airspace the narrow searches take

    @staticmethod
    def _layer_reach(delta, max_steps) -> np.ndarray:
        """The reach of a layer search, fl(max_steps * delta) per axis: what `airspaces` needs to cover every layer 0 .. max_steps."""
        max_steps = int(max_steps)
        if not (0 <= max_steps <= nat.LAYER_MAX_STEPS):
            raise ValueError(f"max_steps must be in 0 .. {nat.LAYER_MAX_STEPS}")
        d = np.asarray(delta.detach().cpu().numpy() if hasattr(delta, "detach") else delta, dtype=np.float64).reshape(-1)
        if d.size != 3 or not np.isfinite(d).all():
            raise ValueError("delta must be three finite numbers")
        return np.float64(max_steps) * d

    def _airspace_front(self, plan, radius, groups, reach, priority, start_rows):
        """The front of the `airspaces=True` forms -> (the plan taken in airspace order, rank, the start rows in slot order or None, the
        searches' `groups` / `wide` / `group_cap`).  With a `priority` two stable passes: the order by priority within the caller's
        groups, then that order by label -- within an airspace the order is the priority's, ties to the earlier slot."""
        torch = self._torch
        plan = self._coeff_plan(plan)
        B = int(plan.B)
        asp = self.airspaces(plan, radius, groups, reach)
        order, rank = asp.order, asp.rank
        if priority is not None:
            by_priority, slot_of, _ = self._priority_order(priority, groups, B, None, None)
            go, G = self._groups(groups, B)
            keys = asp.labels[by_priority.long()].to(torch.float64)
            by_label, slot_then = (torch.empty((B,), dtype=torch.int32, device=self.device) for _ in range(2))
            self._bind_stream()
            self.ctx.call("uavac_fleet_order_dev", _ptr(keys), _ptr(go), G, B, _ptr(by_label), _ptr(slot_then))
            order, rank = by_priority[by_label.long()].contiguous(), slot_then[slot_of.long()].contiguous()
        start = None if start_rows is None else self._start_rows(start_rows, B)[order.long()]
        wide = asp.largest > self.NARROW_SEARCH
        return self.take(plan, order), rank, start, dict(groups=asp.offsets, wide=wide, group_cap=asp.largest if wide else None)

    def _priority_order(self, priority, groups, B: int, max_group: int, start_rows):
        """The front of the `priority=` forms: the within-group order of `priority` (`uavac_fleet_order_dev`) -> (order, rank, the start
        rows in slot order or None), device tensors.  The groups are checked against `max_group` (None: no limit, the `wide` forms) here,
        before anything is copied."""
        torch = self._torch
        pr = self._dev(priority, torch.float64).reshape(-1)
        if pr.numel() != B:
            raise ValueError(f"one priority per mission: expected {B}, got {pr.numel()}")
        go, G = self._groups(groups, B, max_group)
        order = torch.empty((B,), dtype=torch.int32, device=self.device)
        rank = torch.empty((B,), dtype=torch.int32, device=self.device)
        self._bind_stream()
        self.ctx.call("uavac_fleet_order_dev", _ptr(pr), _ptr(go), G, B, _ptr(order), _ptr(rank))
        start = None if start_rows is None else self._start_rows(start_rows, B)[order.long()]
        return order, rank, start

    @staticmethod
    def _stagger_back(res: StaggerResult, rank) -> StaggerResult:
        """A stagger result in slot order -> the caller's batch order (no row of it holds a batch index)."""
        block = res.block[:, rank.long()].contiguous()
        return StaggerResult(*block.unbind(0), block)

    @staticmethod
    def _layer_back(res: LayerResult, rank) -> LayerResult:
        """A layer result in slot order -> the caller's batch order: the block column-wise, the offsets row-wise."""
        at = rank.long()
        block = res.block[:, at].contiguous()
        return LayerResult(*block[:nat.LAYER_ROWS].unbind(0), block, res.offsets[at].contiguous())

    def deconflict(self, plan, radius: float, groups=None, obstacles=None, start_rows=None, step: int = 1, max_delay_steps: int = 255,
                   delta=(0.0, 0.0, -0.5), max_layers: int = 63, priority=None, wide: bool = False, group_cap=None,
                   airspaces: bool = False, traffic=None, traffic_groups=None, traffic_start_rows=None) -> DeconflictResult:
        """The fleet chain as one call: stagger -> layer -> shift -> delay.  `Engine.stagger(plan, radius, groups, start_rows, step,
        max_delay_steps)` makes missions wait; `Engine.layer(plan, radius, groups, start_rows=stagger.start_rows, delta=delta,
        max_steps=max_layers, obstacles=obstacles)` moves, at the granted starts, the ones that waiting cannot clear -- and, with
        `obstacles`, every mission that a cuboid is in the way of; the plan to fly is `Engine.delay(Engine.shift(plan, layer.offsets),
        stagger.start_rows)`.  A pure composition of those calls: every argument means what it means there, and the one host read is
        `Engine.delay`'s.  `plan` is left as it is.
        -> DeconflictResult: `plan` (a rows-free RaggedBatch; `eng.fleet(result.plan)` flies it), `stagger`, `layer`, and `resolved`
        (B,) bool on the device = layer.steps >= 0.
        GUARANTEES, among the RESOLVED missions of `result.plan`: `Engine.separation(result.plan, radius, groups)` finds no pair of them
        inside the radius, and with `obstacles` `Engine.audit(result.plan, obstacles).hit_rows` is 0 for each of them (a hold row is the
        mission's first row, which the search tested).  WHAT IT DOES NOT: it is greedy in priority order (ascending batch index), not a
        minimum of the total delay or displacement; a mission that is not resolved keeps layer 0 and its granted start, wherever that
        leaves it, and may be inside the radius of others or inside a cuboid -- look at `resolved`.  A mission whose every layer is
        blocked (`uav_ac.scoring.blocked_out(result.layer, max_layers)`) needs a re-plan around the obstacle (`plan_collision_free`),
        not an offset.  The start delays know nothing about obstacles: a delay does not move a path.  Without `obstacles` nothing is
        known about cuboids at all.
        `priority` (B,) array or tensor, or None: the order of both searches, by the rule of `Engine.stagger` (a lower number goes
        first, ties to the lower batch index; "ascending batch index" above becomes "ascending priority": the first of its group's
        order is never delayed, and is moved only by a cuboid).  Both searches run on ONE `Engine.take(plan, order)` -- the layer search
        takes the stagger's granted starts as they come, in slot order -- and their answers are gathered back: `stagger`, `layer`,
        `resolved` and `plan`, which is built from the original `plan`, are all in the caller's batch order.  One host read more,
        `Engine.take`'s.  None: the calls as they always were.
        WHAT STAYS UNRESOLVED: `eng.take(plan, ~result.resolved)` takes those missions out to look at them; re-plan them from your own
        waypoints (`plan_ragged` / `plan_collision_free`: `waypoints` is None after a transform, so the caller keeps them),
        `eng.put(plan, ~result.resolved, replanned)` puts them back, and `deconflict` runs again -- with a priority that takes them
        first if they are to win this time.
        `wide=True`, `group_cap`: groups of any size; both searches run as `Engine.stagger(..., wide=True, group_cap=group_cap)` and
        `Engine.layer(..., wide=True, group_cap=group_cap)`, and the guarantees above hold unchanged.
        `airspaces=True`: both searches per airspace, as `Engine.stagger` and `Engine.layer` describe it.  The airspaces are computed
        ONCE, with `reach` = `max_layers` * `delta` -- boxes that cover the layers cover the starts too --, both searches run on one
        `Engine.take(plan, order)`, and `plan` is built from the caller's plan as in the `priority=` form: the same `stagger.start_rows`
        / `steps`, `layer.layers` / `steps` / `blocked` / `offsets`, `resolved` and `plan`, bit for bit, as `wide=True` gives;
        `earlier` counts within the airspace, and the size limits apply to airspaces.
        `traffic`, `traffic_groups`, `traffic_start_rows`: NEWCOMERS AROUND COMMITTED TRAFFIC THAT NEVER MOVES -- the missions of an
        earlier `deconflict` that have been granted their starts and layers, or are in the air.  The chain is the same: stagger
        against the traffic, layer against the traffic at the granted starts, shift, delay -- `Engine.stagger(..., traffic=)` and
        `Engine.layer(..., traffic=)`, always block-wise (`wide` is not looked at, `group_cap` as for `wide=True`).  `traffic` is the
        plan the committed missions FLY (an earlier `result.plan`: shifted and delayed), with `traffic_start_rows` None, or any plan
        with its start rows.  `result.plan` holds the NEWCOMERS ONLY, and nothing of the traffic is decided, moved or written -- two
        committed missions that conflict with each other stay as they are, which a `priority=` on a re-run of everybody could not
        promise.  `Engine.concat([traffic, result.plan])` is the new committed fleet.  GUARANTEES, in addition to those above:
        `Engine.separation_against(result.plan, traffic, radius, groups, traffic_groups, traffic_start_rows=traffic_start_rows)`
        reports `conflicts == 0` for every resolved mission.  `airspaces=True` with `traffic` is a ValueError (airspaces are not
        labelled across two plans); so are a different `dt` and group counts that do not match."""
        against = dict(traffic=traffic, traffic_groups=traffic_groups, traffic_start_rows=traffic_start_rows)
        if airspaces:
            if traffic is not None:
                raise ValueError("airspaces=True does not take traffic: airspaces are not labelled across two plans")
            taken, rank, start, route = self._airspace_front(plan, radius, groups, self._layer_reach(delta, max_layers), priority, start_rows)
            stag = self.stagger(taken, radius, start_rows=start, step=step, max_steps=max_delay_steps, **route)
            lay = self.layer(taken, radius, start_rows=stag.start_rows, delta=delta, max_steps=max_layers, obstacles=obstacles, **route)
            stag, lay = self._stagger_back(stag, rank), self._layer_back(lay, rank)
            flown = self.delay(self.shift(plan, lay.offsets), stag.start_rows)
            return DeconflictResult(flown, stag, lay, lay.steps >= 0)
        w = dict(wide=wide or traffic is not None, group_cap=group_cap, **against)
        if priority is not None:
            B = int(self._coeff_plan(plan).B)
            order, rank, start = self._priority_order(priority, groups, B, None if w["wide"] else min(nat.STAGGER_MAX_GROUP, nat.LAYER_MAX_GROUP),
                                                      start_rows)
            taken = self.take(plan, order)
            stag = self.stagger(taken, radius, groups=groups, start_rows=start, step=step, max_steps=max_delay_steps, **w)
            lay = self.layer(taken, radius, groups=groups, start_rows=stag.start_rows, delta=delta, max_steps=max_layers, obstacles=obstacles,
                             **w)
            stag, lay = self._stagger_back(stag, rank), self._layer_back(lay, rank)
            flown = self.delay(self.shift(plan, lay.offsets), stag.start_rows)
            return DeconflictResult(flown, stag, lay, lay.steps >= 0)
        stag = self.stagger(plan, radius, groups=groups, start_rows=start_rows, step=step, max_steps=max_delay_steps, **w)
        lay = self.layer(plan, radius, groups=groups, start_rows=stag.start_rows, delta=delta, max_steps=max_layers, obstacles=obstacles, **w)
        flown = self.delay(self.shift(plan, lay.offsets), stag.start_rows)
        return DeconflictResult(flown, stag, lay, lay.steps >= 0)

    def _cuboids(self, obstacles, per: str):
        """(the cuboids as a contiguous (n, 6) float64 device tensor, n) of `obstacles` ((n, 6) array or tensor: xmin xmax ymin ymax zmin
        zmax); another shape, or more than `AUDIT_MAX_CUBOIDS` of them, is a ValueError."""
        cub = self._dev(obstacles, self._torch.float64)
        if cub.numel() % 6 or (cub.dim() == 2 and cub.shape[1] != 6):
            raise ValueError(f"obstacles must be (n, 6): xmin xmax ymin ymax zmin zmax, got {tuple(cub.shape)}")
        cub = cub.reshape(-1, 6).contiguous()
        n = int(cub.shape[0])
        if n > nat.AUDIT_MAX_CUBOIDS:
            raise ValueError(f"{n} cuboids; at most {nat.AUDIT_MAX_CUBOIDS} per {per}")
        return cub, n

    def _log_view(self, state_log):
        """(K, B, pitch) of a state log the flown audits can read in place -- the (K, 13, B) view a logged rollout returns (at whatever
        log pitch) or a dense caller tensor: float64 on the engine's device with stride(2) == 1 and stride(0) == 13 * stride(1) (the
        pitch is stride(1)); anything else is a ValueError."""
        torch = self._torch
        if not isinstance(state_log, torch.Tensor) or state_log.dim() != 3 or state_log.dtype != torch.float64 \
                or state_log.device != self.device:
            raise ValueError("state_log must be a float64 tensor (K, 13, B) on the engine's device")
        K, R, B = (int(v) for v in state_log.shape)
        if R != nat.STATE_LOG_ROWS or K < 1 or B < 1:
            raise ValueError(f"state_log must have shape (K >= 1, {nat.STATE_LOG_ROWS}, B >= 1), got {tuple(state_log.shape)}")
        pitch = int(state_log.stride(1))
        if state_log.stride(2) != 1 or pitch < B or (K > 1 and state_log.stride(0) != nat.STATE_LOG_ROWS * pitch):
            raise ValueError("state_log must be laid out [K][13][pitch]: stride(2) == 1, stride(1) = pitch >= B, stride(0) == 13 * pitch")
        return K, B, pitch

    def flown_separation(self, state_log, radius: float, groups=None) -> SeparationAudit:
        """The separation the fleet FLEW (`uavac_flown_separation_dev`): `Engine.separation` speaks about plans, this about the
        vehicles, which track them with an error -- from the positions in a rollout's state log, on the device, without pulling the
        log to the host.  `state_log`: the (K, 13, B) view that `fleet.rollout(K, state_log=True)` returns (at whatever log pitch), or
        a dense caller tensor: float64 with stride(2) == 1 and stride(0) == 13 * stride(1) (the pitch is stride(1)); anything else is a
        ValueError.  `radius` and `groups` as in `Engine.separation`.
        -> SeparationAudit in the same terms, bit for bit what NumPy gives on the log (`uav_ac.scoring.separation_from_log`): the
        closest approach to any other vehicle of the group, that partner, and in `row` the TICK of the closest approach (clock row of
        the plan = tick // F, with F the vehicle's inner ticks per outer tick, `inner_per_outer`); `conflicts` and `first_conflict`
        (a tick too) against `radius`; `compared` = the partners with at least one pair-tick whose distance is a number, so a vehicle
        whose log holds NaN is visible.  A vehicle with nobody to compare with reports +inf / -1 / -1 / 0 / -1 / 0.
        `uav_ac.scoring.separation_ok` applies unchanged.  Stream-ordered like the other _dev calls, no sync."""
        K, B, pitch = self._log_view(state_log)
        go, G = self._groups(groups, B)
        return self._separation_audit("uavac_flown_separation_dev", (_ptr(state_log), K, B, pitch, _ptr(go), G, float(radius)), B)

    def flown_conflicts(self, state_log, radius: float, groups=None) -> ConflictList:
        """Every pair of vehicles that `Engine.flown_separation` counts as a conflict, with when and how near
        (`uavac_flown_conflict_offsets_dev`, `uavac_flown_conflicts_dev`): vehicle i lists each vehicle of its group that the flight
        brought inside `radius` at some tick, in ascending batch index -- from the positions in a rollout's state log, on the device,
        bit for bit what NumPy gives on the log (`uav_ac.scoring.conflicts_from_log`).  `state_log`, `radius` and `groups` as
        `Engine.flown_separation` takes them (a log in another layout is a ValueError).
        -> ConflictList whose `*_row` fields hold TICKS here: `first_row` and `last_row` the first and the last tick inside,
        `rows_inside` the number of ticks inside (a tick at which either position is NaN is not inside), `min_row` the tick of the pair's
        closest approach (clock row of the plan = tick // F, with F the vehicle's `inner_per_outer`).  On the same log diff(offsets)
        is the flown audit's `conflicts`, the least `first_row` of a vehicle its `first_conflict`, and its (min_distance, row, partner)
        the least (min_distance, min_row, partner) of the vehicle's entries; the two directions of a pair carry the same record
        (`uav_ac.scoring.conflict_pairs`; `scoring.conflict_diff` compares the list with `Engine.conflicts` of the plan).
        ONE small host read: the number of entries, to size the result; without entries the second launch is skipped."""
        K, B, pitch = self._log_view(state_log)
        go, G = self._groups(groups, B)
        return self._conflict_list("uavac_flown_conflict_offsets_dev", "uavac_flown_conflicts_dev",
                                   (_ptr(state_log), K, B, pitch, _ptr(go), G, float(radius)), B)

    def flown_audit(self, state_log, obstacles=None) -> FlightAudit:
        """The plan audit of a FLIGHT (`uavac_flown_audit_dev`): `Engine.audit` says what a plan's rows would show, this what the
        vehicles DID, which track the plan with an error -- one pass over a rollout's state log on the device, without pulling the log
        to the host.  `state_log` as `Engine.flown_separation` takes it (the view a logged rollout returns, at whatever pitch, or a
        dense tensor; anything else is a ValueError); `obstacles` as `Engine.audit` takes them ((n, 6), n <= 16).
        -> FlightAudit, bit for bit what NumPy gives on the log (`uav_ac.scoring.audit_from_log`).  A tick counts iff its 13 logged
        values are finite: `ticks` says how many did and `first_bad` which was the first that did not (-1: none); the peaks of
        horizontal speed, climb, descent and speed, of the two rotation-matrix elements the control law clips its attitude command to
        with max_tilt (`bank_x`, `bank_y`) and of the body rate are over those ticks, NaN when there is none.  Per cuboid:
        `hit_ticks` -- how many valid ticks the vehicle spent inside it (the inclusive test of the rollout's `collided` bit) --,
        `first_hit` (a tick, -1: none), and `clearance` with `clearance_tick`: the closest approach to the cuboid and when (0 exactly
        where there are hits).  `uav_ac.scoring.flight_feasibility` turns it into verdicts.  Stream-ordered like the other _dev calls,
        no sync."""
        torch = self._torch
        K, B, pitch = self._log_view(state_log)
        kw = dict(device=self.device)
        cub, n = (None, 0) if obstacles is None else self._cuboids(obstacles, "audit")
        block = torch.empty((nat.FLOWN_AUDIT_ROWS, B), dtype=torch.float64, **kw)
        first_bad = torch.empty((B,), dtype=torch.int32, **kw)
        hit_ticks, first_hit, clearance_tick = (torch.empty((n, B), dtype=torch.int32, **kw) for _ in range(3))
        clearance = torch.empty((n, B), dtype=torch.float64, **kw)
        self._bind_stream()
        per_cuboid = [_ptr(t) if n else None for t in (hit_ticks, first_hit, clearance, clearance_tick)]
        self.ctx.call("uavac_flown_audit_dev", _ptr(state_log), K, B, pitch, _ptr(cub) if n else None, n, _ptr(block), _ptr(first_bad),
                      *per_cuboid)
        return FlightAudit(*block.unbind(0), first_bad, hit_ticks, first_hit, clearance, clearance_tick, block)

    DEFAULT_RETIME_MARGIN = 1e-3

    def retime(self, plan, vehicle: Optional[nat.Vehicle] = None, margin: float = DEFAULT_RETIME_MARGIN, max_passes: int = 4,
               demand: bool = False) -> RetimeResult:
        """Slow down exactly the missions of `plan` that ask for more than the control law gives (`vehicle`'s max_speed_xy,
        max_ascent, max_descent, max_horiz_accel; None = `uavac_vehicle_default`), by exactly the factor they need
        (`uavac_minsnap_retime_dev`): per pass the rows-free chain at the current per-mission speeds, the audit, and per mission
        r = max(speed_xy / L0, ascent / L1, descent / L2, sqrt(accel_xy / L3)); a mission with r > 1 is planned again at
        velocity / (r / (1 - margin)), which leaves its curve where it is and scales its velocity peaks by 1 / k, its acceleration
        peaks by 1 / k^2.  Stops when no mission was slowed down or after `max_passes` retimings (0: audit only, no speed changes);
        one host sync per pass, no row sampled inside the loop.
        `margin`: the audit's peaks are maxima over SAMPLES, and the slower plan is sampled elsewhere on the curve, so its peaks may
        lie above peak / k by the gap between sampled and continuous maxima -- about 1e-4 relative on the bench distribution (3 m
        legs at 3 m/s) at dt = 0.01, and larger for a coarser dt.  The default of 1e-3 clears that with room and costs 0.1 % of
        speed; a margin below the gap costs further passes, not correctness (`converged` tells).
        `plan`: a Plan, a RaggedBatch, or a RaggedPlan that has its batch; it is left as it is.  -> RetimeResult whose `.plan` is of
        the same kind, with fresh buffers: rows-free if the input was, else with rows sampled ONCE at the end.  A plan with boundary
        derivatives (`plan(..., boundary=...)`) is refused (ValueError): its curve moves when its durations change; so is a `free_times`
        plan, whose durations did not come from a speed.  Missions whose plan
        is singular (or has no rows) keep their speed, report a NaN factor and converged = False; the device flags are left to the
        caller (`take_flags`).
        `demand`: False = the four limits above and nothing else.  True = also the limits `Engine.demand` reports on and
        `scoring.demand_feasibility` judges -- the bank command within max_tilt, no thrust downward, the rotor thrust between
        min_thrust and max_thrust (`uavac_minsnap_retime_demand_dev`: per pass one more kernel, `Engine.need`'s, and r is the larger of
        the maximum above and the four slowdown factors of the PlanNeed).  The result then carries `need`, the PlanNeed of the returned
        plan, and `binding`, per mission the index into `scoring.BINDING_NAMES` of the limit that is nearest in the last audit.  The
        body rate and the cuboid clearance are not retimed to: the one has no closed form, the other does not move with the timing."""
        torch = self._torch
        wrapper = plan if isinstance(plan, RaggedPlan) else None
        plan = self._coeff_plan(plan, refuse="this RaggedPlan has no batch (plan_collision_free(device_loop=False)): retime "
                                             "eng.plan_ragged(plan.final_waypoints, ...)")
        if plan.waypoints is None:
            raise ValueError("retiming plans again from the waypoints: a plan assembled from gathered parts has none")
        if getattr(plan, "boundary", None) is not None:
            raise ValueError("a plan with boundary derivatives cannot be retimed: retiming rests on the curve staying where it is under a "
                             "change of durations, and a curve with fixed physical end derivatives does not")
        if getattr(plan, "free_times", False):
            raise ValueError("a plan from given durations cannot be retimed: retiming recomputes the durations from cruise speeds, "
                             "which would discard the given ones")
        s = segments(plan)
        B, m = s.B, s.m
        V = nat.Vehicle.default() if vehicle is None else vehicle
        limits = (C.c_double * 4)(float(V.max_speed_xy), float(V.max_ascent), float(V.max_descent), float(V.max_horiz_accel))
        kw = dict(device=self.device)
        old = getattr(plan, "velocities", None)
        speeds = old.clone() if old is not None else torch.full((B,), float(plan.velocity), dtype=torch.float64, **kw)
        times, seg_rows, coeffs = torch.empty_like(plan.times), torch.empty_like(plan.seg_rows), torch.empty_like(plan.coeffs)
        row_offsets = torch.empty((B + 1,), dtype=torch.int64, **kw)
        status = torch.zeros((B,), dtype=torch.int32, **kw)
        first_yaw = torch.empty((B,), dtype=torch.float64, **kw)
        block = torch.empty((nat.AUDIT_ROWS, B), dtype=torch.float64, **kw)
        factors = torch.empty((B,), dtype=torch.float64, **kw)
        converged = torch.empty((B,), dtype=torch.int32, **kw)
        passes = C.c_int(0)
        need = binding = None
        if demand:
            dlimits = self._demand_limits(V)
            nblock = torch.empty((nat.NEED_ROWS, B), dtype=torch.float64, **kw)
            binding = torch.empty((B,), dtype=torch.int32, **kw)
            need = PlanNeed(*nblock.unbind(0), nblock)
        self._bind_stream()
        if demand:
            self.ctx.call("uavac_minsnap_retime_demand_dev", _ptr(plan.waypoints), _ptr(s.so), B, m, _ptr(speeds),
                          float(plan.dt), limits, dlimits, float(margin), int(max_passes), _ptr(times), _ptr(seg_rows), _ptr(row_offsets),
                          _ptr(coeffs), _ptr(status), _ptr(first_yaw), _ptr(block), _ptr(nblock), _ptr(factors), _ptr(binding),
                          _ptr(converged), C.byref(passes))
        else:
            self.ctx.call("uavac_minsnap_retime_dev", _ptr(plan.waypoints), _ptr(s.so), B, m, _ptr(speeds),
                          float(plan.dt), limits, float(margin), int(max_passes), _ptr(times), _ptr(seg_rows), _ptr(row_offsets),
                          _ptr(coeffs), _ptr(status), _ptr(first_yaw), _ptr(block), _ptr(factors), _ptr(converged), C.byref(passes))
        parts = dict(waypoints=plan.waypoints, times=times, seg_rows=seg_rows, row_offsets=row_offsets, coeffs=coeffs, status=status,
                     traj=None, total_rows=int(row_offsets[-1].item()), first_yaw=first_yaw, velocities=speeds)
        if s.ragged:
            out = RaggedBatch(B, m, float("nan"), float(plan.dt), seg_offsets=s.so, seg_offsets_host=s.so_host, **parts)
        else:
            out = Plan(B, m, float("nan"), float(plan.dt), **parts)
        if plan.traj is not None:
            self.sample_rows(out)                                # the rows, once
        if wrapper is not None:
            out = RaggedPlan(B, float("nan"), float(plan.dt), wrapper.final_waypoints, row_offsets=out.row_offsets, traj=out.traj,
                             total_rows=out.total_rows, start_positions=wrapper.start_positions, converged=wrapper.converged, batch=out)
        empty = torch.empty((0, B), dtype=torch.int32, **kw)
        return RetimeResult(out, speeds, factors, int(passes.value), converged != 0, PlanAudit(*block.unbind(0), empty, empty, block),
                            need, binding)

    def cost(self, plan):
        """The snap cost of every mission of a Plan / RaggedBatch (or a RaggedPlan that has its batch) -> (B,) f64 on the device: the
        sum over segments and axes of the integral of snap^2 over the segment, upstream's c^T H c (`uavac_minsnap_cost_dev`: by
        four-point Gauss-Legendre quadrature, exact for the integrand and free of c^T H c's cancellation).  NaN for a mission with a
        non-finite coefficient.  Stream-ordered, no sync."""
        torch = self._torch
        plan = self._coeff_plan(plan, refuse="this RaggedPlan has no batch, hence no coefficients")
        if plan.coeffs is None or plan.times is None:
            raise ValueError("the cost needs the plan's coefficients and durations")
        s = segments(plan)
        out = torch.empty((s.B,), dtype=torch.float64, device=self.device)
        if s.B == 0:
            return out
        self._bind_stream()
        self.ctx.call("uavac_minsnap_cost_dev", _ptr(plan.coeffs), _ptr(plan.times), _ptr(s.so), s.B, s.m, _ptr(out))
        return out

    def optimize_times(self, plan, iterations: int = 8, rows: Optional[bool] = None) -> TimeOptResult:
        """Divide every mission's total time between its legs so that the snap cost falls (`uavac_minsnap_optimize_times_dev`): the
        second half of the minimum-snap method.  Per iteration m probe solves per mission give the gradient of the cost along
        total-preserving directions, six step sizes along the projected descent direction are solved and costed, and the best one that
        is strictly better is taken; all missions at once, no host sync inside the loop.  The total time of a mission is kept, no
        duration falls below 0.2 of the mission's shortest, and the cost never rises.
        `plan`: a rest-to-rest Plan or RaggedBatch (durations from a speed or given); it is left untouched.  One with `boundary` is
        refused (ValueError).  -> TimeOptResult whose `.plan` is a NEW `free_times` plan on the same waypoints, planned by
        `uavac_minsnap_plan_t_dev` from the optimised durations; `rows`: with or without rows (None: as the input has them).
        `cost_after` is the cost of exactly that plan.
        The promise is a lower snap cost, NOT feasibility: single missions can come out with a higher peak speed, so `audit` stays the
        judge.  And the new curve passes the same waypoints but not the same points in between: a plan that came out of the obstacle
        loop must be audited against its cuboids again -- `Engine.audit(result.plan, obstacles)`."""
        torch = self._torch
        plan = self._coeff_plan(plan, refuse="this RaggedPlan has no batch: optimise eng.plan_ragged(plan.final_waypoints, ...)")
        if getattr(plan, "boundary", None) is not None:
            raise ValueError("the duration optimisation is rest to rest: not for a plan with boundary derivatives")
        if plan.waypoints is None:
            raise ValueError("the optimisation solves again from the waypoints: a plan assembled from gathered parts has none")
        if int(iterations) < 0:
            raise ValueError("iterations must be >= 0")
        s = segments(plan)
        B, m = s.B, s.m
        kw = dict(device=self.device)
        times = plan.times.clone()
        before = torch.empty((B,), dtype=torch.float64, **kw)
        after = torch.empty((B,), dtype=torch.float64, **kw)
        accepted = torch.empty((B,), dtype=torch.int32, **kw)
        self._bind_stream()
        self.ctx.call("uavac_minsnap_optimize_times_dev", _ptr(plan.waypoints), _ptr(s.so), B, m, _ptr(times), int(iterations),
                      _ptr(before), _ptr(after), _ptr(accepted))
        with_rows = (plan.traj is not None) if rows is None else bool(rows)
        out = self._plan_from_times(plan.waypoints, times, plan.dt, with_rows, False, so=s.so, so_host=s.so_host, max_m=m)
        return TimeOptResult(out, before, after, accepted)

    def sample_range(self, plan: Plan, b0: int, b1: int):
        """The rows (and first headings) of missions [b0, b1) of a uniform plan, written where `sample(plan)` writes them: the
        row offsets are absolute, so a sub-range is the same kernel on offset pointers.  Any cover of [0, B) by ranges, in any
        order, leaves the rows of one `sample(plan)` bit for bit -- what lets the root of a pipelined plan gather sample a part
        of every peer's block while the next part arrives.  No allocation, no sync."""
        b0, b1 = int(b0), int(b1)
        if not (0 <= b0 <= b1 <= plan.B):
            raise ValueError("need 0 <= b0 <= b1 <= plan.B")
        if plan.traj is None:
            raise ValueError("a rows-free plan has no row buffer: Engine.sample_rows(plan) allocates one and samples")
        if b1 == b0:
            return
        self._bind_stream()
        fy = getattr(plan, "first_yaw", None)
        # (the offsets are absolute: the capacity is the whole buffer's; a range that would end past it writes nothing, flag 2)
        self.ctx.call("uavac_minsnap_sample_capped_dev", _ptr(plan.coeffs[b0:b1]), _ptr(plan.seg_rows[b0:b1]), _ptr(plan.row_offsets[b0:]),
                      b1 - b0, plan.m, plan.dt, _ptr(plan.traj), int(plan.traj.shape[0]), _ptr(plan.yaw),
                      _ptr(None if fy is None else fy[b0:b1]))

    def plan_from_parts(self, coeffs, times, seg_rows, m: int, velocity: float, dt: float, total_rows: int = None,
                        traj=None, sample: bool = True) -> Plan:
        """A Plan from its solved parts -- coefficients (B, 8m, 3), durations (B, m) or None, rows per spline (B, m) -- e.g.
        the peers' plans after `RcclComm.gather_plan`: row offsets from the row counts (`uavac_minsnap_row_offsets_dev`),
        then the sampler writes the rows (and the first headings).  The rows are a deterministic function of coefficients,
        row counts and dt: bit-identical to the rows of the plan the parts came from.  `total_rows` (when the caller knows
        it) avoids the one host synchronisation that sizes the row buffer; `traj`: a preallocated (>= total, 11) buffer.
        `sample=False`: lay the rows out (offsets, buffers) but leave the sampling to the caller's `sample_range` calls."""
        torch = self._torch
        co = self._dev(coeffs, torch.float64).reshape(-1, 8 * int(m), 3)
        sr = self._dev(seg_rows, torch.int32).reshape(-1, int(m))
        B = int(co.shape[0])
        if sr.shape[0] != B or B < 1:
            raise ValueError("coeffs and seg_rows disagree on the number of missions")
        tm = None if times is None else self._dev(times, torch.float64).reshape(B, int(m))
        kw = dict(device=self.device)
        row_offsets = torch.empty((B + 1,), dtype=torch.int64, **kw)
        self._bind_stream()
        self.ctx.call("uavac_minsnap_row_offsets_dev", _ptr(sr), B, int(m), _ptr(row_offsets))
        total = int(row_offsets[-1].item()) if total_rows is None else int(total_rows)
        if traj is None:
            traj = torch.empty((total, nat.TRAJ_COLS), dtype=torch.float64, **kw)
        elif traj.shape[0] < total or traj.dtype != torch.float64 or not traj.is_contiguous():
            raise ValueError("traj must be a contiguous float64 tensor with at least total_rows rows")
        plan = Plan(B, int(m), float(velocity), float(dt), waypoints=None, times=tm, seg_rows=sr, row_offsets=row_offsets, coeffs=co,
                    status=torch.zeros((B,), dtype=torch.int32, **kw), traj=traj[:total], total_rows=total,
                    first_yaw=torch.empty((B,), dtype=torch.float64, **kw))
        if sample:
            self.sample(plan)
        return plan

    def ragged_from_parts(self, coeffs, times, seg_rows, seg_counts, velocity: float, dt: float, total_rows: int = None,
                          traj=None) -> RaggedBatch:
        """`plan_from_parts` for a ragged batch: coefficients (S, 8, 3), durations (S,) or None, rows per spline (S,) back to back
        and the number of splines of every mission (B,) -> RaggedBatch with the rows re-sampled (bit-identical)."""
        torch = self._torch
        co = self._dev(coeffs, torch.float64).reshape(-1, 8, 3)
        sr = self._dev(seg_rows, torch.int32).reshape(-1)
        cnt = np.asarray(seg_counts.cpu() if hasattr(seg_counts, "cpu") else seg_counts, dtype=np.int64).reshape(-1)
        B, S = len(cnt), int(cnt.sum())
        if S != co.shape[0] or S != sr.shape[0] or B < 1 or cnt.min() < 1 or cnt.max() > nat.MAX_SEGMENTS:
            raise ValueError("segment counts, coefficients and row counts disagree")
        so_host = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(cnt, out=so_host[1:])
        so = self._dev(so_host, torch.int64)
        max_m = int(cnt.max())
        kw = dict(device=self.device)
        row_offsets = torch.empty((B + 1,), dtype=torch.int64, **kw)
        self._bind_stream()
        self.ctx.call("uavac_minsnap_row_offsets_ragged_dev", _ptr(sr), _ptr(so), B, max_m, _ptr(row_offsets))
        total = int(row_offsets[-1].item()) if total_rows is None else int(total_rows)
        if traj is None:
            traj = torch.empty((total, nat.TRAJ_COLS), dtype=torch.float64, **kw)
        first_yaw = torch.empty((B,), dtype=torch.float64, **kw)
        self.ctx.call("uavac_minsnap_sample_ragged_dev", _ptr(co), _ptr(sr), _ptr(so), _ptr(row_offsets), B, max_m, S, float(dt),
                      _ptr(traj), int(traj.shape[0]), None, None, _ptr(first_yaw))
        tm = None if times is None else self._dev(times, torch.float64).reshape(-1)
        # the first waypoint of every mission is c0 of its first spline; the others are not needed to fly or to ship the plan
        return RaggedBatch(B, max_m, float(velocity), float(dt), seg_offsets=so, seg_offsets_host=so_host, waypoints=None, times=tm,
                           seg_rows=sr, row_offsets=row_offsets, coeffs=co, status=torch.zeros((B,), dtype=torch.int32, **kw),
                           traj=traj[:total], total_rows=total, first_yaw=first_yaw)

    def take_flags(self):
        """Synchronise and return-and-clear the sticky device-side flags of the `_dev` planning entry points:
        [non-finite duration, singular system, trajectory buffer too small, mission longer than 2^31-1 rows]."""
        fl = (C.c_int32 * 4)()
        self._bind_stream()
        self.ctx.call("uavac_take_flags", fl)
        return [int(v) for v in fl]

    def sample_derivatives(self, plan: Plan):
        """Jerk and snap along the plan's rows: (N, 3) each -- `polynom(8, 3, t) @ coeffs` and `polynom(8, 4, t) @
        coeffs`, the samples minimum_snap.py:111-112 holds in comments.  Separate arrays; plan.traj keeps its 11
        columns (and is rewritten with the same values)."""
        torch = self._torch
        jerk = torch.empty((plan.total_rows, 3), dtype=torch.float64, device=self.device)
        snap = torch.empty((plan.total_rows, 3), dtype=torch.float64, device=self.device)
        self._bind_stream()
        self.ctx.call("uavac_minsnap_sample_derivs_dev", _ptr(plan.coeffs), _ptr(plan.seg_rows), _ptr(plan.row_offsets),
                      plan.B, plan.m, plan.dt, _ptr(plan.traj), _ptr(plan.yaw), _ptr(plan.first_yaw), _ptr(jerk), _ptr(snap))
        return jerk, snap

    def yaw_scan(self, velocities, offsets=None):
        """Batched `MinimumSnap._calculate_yaws` (minimum_snap.py:126-136): velocities (N, 3) rows of B sequences back
        to back, sequence b = rows offsets[b]:offsets[b+1] (default: one sequence).  -> yaws (N,) on the GPU."""
        torch = self._torch
        v = self._dev(velocities, torch.float64)
        if v.dim() != 2 or v.shape[1] != 3:
            raise ValueError(f"velocities must have shape (N, 3), got {tuple(v.shape)}")
        n = int(v.shape[0])
        off = self._dev([0, n] if offsets is None else offsets, torch.int64)
        if off.dim() != 1 or off.numel() < 2:
            raise ValueError("offsets must be a 1-D array of B+1 row indices")
        yaws = torch.empty((n,), dtype=torch.float64, device=self.device)
        if n:
            self._bind_stream()
            self.ctx.call("uavac_yaw_scan_dev", _ptr(v), _ptr(off), int(off.numel()) - 1, _ptr(yaws))
        return yaws

    def plan_collision_free(self, waypoints, obstacles, velocity: float = 1.0, dt: float = 0.01,
                            max_iterations: int = 64, strict: bool = True, recheck_passes: int = 0,
                            device_loop: bool = True) -> RaggedPlan:
        """Batched `MinimumSnap(path, obstacles, velocity, dt).get_trajectory()` with obstacles
        (minimum_snap.py:63-95) for B missions at once.

        Per mission the reference's semantics are kept: obstacles are visited in order; for each one the mission is
        planned, every spline with a sample inside the cuboid gets a midpoint inserted before its end waypoint,
        and it is re-planned until clean; earlier obstacles are not re-checked.  Here all missions advance
        together, and a round is ONE call into the C ABI (`uavac_minsnap_obstacle_round_dev`): the still-active missions
        are planned as a ragged batch, their splines scanned for samples inside the cuboid (no rows are stored inside the
        loop), and the midpoints inserted into the next round's waypoint arrays by a kernel; the host reads back four
        counters per round.  The trajectories are sampled once, from the final waypoints.  `device_loop=False` runs round
        2's loop instead (rows sampled in every round, hit flags to the host, midpoints inserted with NumPy): same
        waypoints, kept for comparison.
        `waypoints`: (B, m+1, 3) array or a list of (m_b+1, 3) arrays.  The loop is bounded (the reference's is
        not: it cannot end when a waypoint lies inside a cuboid, or when a leg crosses one squarely).  A mission
        that exhausts `max_iterations` or UAVAC_MAX_SEGMENTS raises RuntimeError when `strict`; otherwise it is
        reported in `RaggedPlan.converged` (False) with its last (still colliding) trajectory and the batch goes on.
        `recheck_passes` > 0 goes beyond the reference: missions that received midpoints are swept over the whole
        obstacle list again (up to that many extra passes, until a pass inserts nothing), which removes the
        conflicts a late midpoint can create with an earlier obstacle.
        """
        if device_loop:
            return self._plan_collision_free_device(waypoints, obstacles, velocity, dt, max_iterations, strict, recheck_passes)
        return self._plan_collision_free_host(waypoints, obstacles, velocity, dt, max_iterations, strict, recheck_passes)

    def _plan_collision_free_device(self, waypoints, obstacles, velocity, dt, max_iterations, strict, recheck_passes) -> RaggedPlan:
        torch = self._torch
        wps = [np.ascontiguousarray(w, dtype=np.float64) for w in waypoints]
        B = len(wps)
        if B == 0 or any(w.ndim != 2 or w.shape[1] != 3 or w.shape[0] < 2 for w in wps):
            raise ValueError("waypoints must be B arrays of shape (m+1, 3)")
        M = nat.MAX_SEGMENTS
        counts = np.array([w.shape[0] - 1 for w in wps], dtype=np.int64)
        if counts.max() > M:
            raise ValueError(f"a mission has {int(counts.max())} segments; at most {M}")
        cuboids = np.zeros((0, 6)) if obstacles is None else np.asarray(obstacles, dtype=np.float64).reshape(-1, 6)
        so_host = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(counts, out=so_host[1:])
        kw = dict(device=self.device)
        S_cap = B * M                                           # no mission ever has more than M segments
        wp_a = torch.empty((S_cap + B, 3), dtype=torch.float64, **kw)
        wp_b = torch.empty_like(wp_a)
        wp_a[:int(so_host[-1]) + B] = self._dev(np.concatenate(wps, axis=0), torch.float64)
        so_a, so_b = self._dev(so_host, torch.int64), torch.empty((B + 1,), dtype=torch.int64, **kw)
        failed = torch.zeros((B,), dtype=torch.int32, **kw)
        max_m = int(counts.max())
        if len(cuboids):
            times = torch.empty((S_cap,), dtype=torch.float64, **kw)
            seg_rows = torch.empty((S_cap,), dtype=torch.int32, **kw)
            row_offsets = torch.empty((B + 1,), dtype=torch.int64, **kw)
            coeffs = torch.empty((S_cap, 8, 3), dtype=torch.float64, **kw)
            hit = torch.empty((S_cap,), dtype=torch.int32, **kw)
            active = torch.empty((B,), dtype=torch.int32, **kw)
            overflow = torch.zeros((B,), dtype=torch.int32, **kw)
            touched = torch.zeros((B,), dtype=torch.int32, **kw)
            counters = torch.zeros((4,), dtype=torch.int32, **kw)
            cub_dev = self._dev(cuboids, torch.float64)
            todo = torch.ones((B,), dtype=torch.int32, **kw)
            self._bind_stream()
            for sweep in range(1 + max(0, int(recheck_passes))):
                touched.zero_()
                for ci in range(len(cuboids)):
                    torch.mul(todo, 1 - failed, out=active)
                    n_active = int(active.sum().item())
                    for it in range(max_iterations + 1):
                        if n_active == 0:
                            break
                        self.ctx.call("uavac_minsnap_obstacle_round_dev", _ptr(wp_a), _ptr(so_a), B, max_m, float(velocity), float(dt),
                                      _ptr(cub_dev[ci]), _ptr(active), _ptr(overflow), _ptr(touched), _ptr(wp_b), _ptr(so_b),
                                      _ptr(counters), _ptr(times), _ptr(seg_rows), _ptr(row_offsets), _ptr(coeffs), _ptr(hit))
                        wp_a, wp_b, so_a, so_b = wp_b, wp_a, so_b, so_a
                        n_active, n_over, max_m, _total = (int(v) for v in counters.tolist())      # the round's one read-back
                        if n_over:
                            if strict:
                                raise RuntimeError(f"obstacle correction needs more than {M} splines")
                            failed.logical_or_(overflow)                 # stays as it is, reported in `converged`
                    else:
                        if n_active:
                            if strict:
                                raise RuntimeError("obstacle correction did not converge (a waypoint inside an obstacle?)")
                            failed.logical_or_(active)
                todo = touched * (1 - failed)                          # only missions that changed can have new conflicts
                if int(todo.sum().item()) == 0:
                    break
            flags = self.take_flags()
            if flags[0]:
                raise ValueError("non-finite waypoint or segment duration")
        # the trajectories, once, from the final waypoints
        so_final = so_a.cpu().numpy()
        S = int(so_final[-1])
        wp_final = wp_a[:S + B]
        batch = self._plan_ragged_tensors(wp_final, so_a, so_final, int((so_final[1:] - so_final[:-1]).max()), velocity, dt, None)
        if strict:
            self.check(batch)
        wp_host = wp_final.cpu().numpy()
        final_wps = [wp_host[so_final[b] + b:so_final[b + 1] + b + 1].copy() for b in range(B)]
        converged = ~failed.cpu().numpy().astype(bool)
        return RaggedPlan(B, float(velocity), float(dt), final_wps, row_offsets=batch.row_offsets, traj=batch.traj,
                          total_rows=batch.total_rows, start_positions=batch.start_positions.contiguous(), converged=converged, batch=batch)

    def _plan_collision_free_host(self, waypoints, obstacles, velocity, dt, max_iterations, strict, recheck_passes) -> RaggedPlan:
        """Round 2's loop: every round a ragged planning batch with rows, hit flags to the host, NumPy midpoint insertion."""
        torch = self._torch
        wps = [np.ascontiguousarray(w, dtype=np.float64) for w in waypoints]
        B = len(wps)
        if B == 0 or any(w.ndim != 2 or w.shape[1] != 3 or w.shape[0] < 2 for w in wps):
            raise ValueError("waypoints must be B arrays of shape (m+1, 3)")
        cuboids = np.zeros((0, 6)) if obstacles is None else np.asarray(obstacles, dtype=np.float64).reshape(-1, 6)
        source = [None] * B                                    # mission -> (group Plan, index inside it)
        failed = set()

        def run_round(ids, cub):
            """One planning call for every mission of `ids` (their segment counts differ: a ragged batch)."""
            members = []
            for b in ids:
                if wps[b].shape[0] - 1 > nat.MAX_SEGMENTS:
                    if strict:
                        raise RuntimeError(f"obstacle correction needs more than {nat.MAX_SEGMENTS} splines")
                    failed.add(b)                                     # keeps the plan of the previous round
                else:
                    members.append(b)
            if not members:
                return []
            batch = self.plan_ragged([wps[b] for b in members], velocity, dt, cuboid=cub)
            for j, b in enumerate(members):
                source[b] = (batch, j)
            again = []
            if batch.hit is not None:
                hit = batch.hit.cpu().numpy().astype(bool)
                so = batch.seg_offsets_host
                hit_missions = np.flatnonzero(np.add.reduceat(hit, so[:-1]) > 0) if len(hit) else []
                for j in hit_missions:
                    b = members[j]
                    idx = np.flatnonzero(hit[so[j]:so[j + 1]]) + 1    # spline s -> insert before waypoint s+1
                    if wps[b].shape[0] - 1 + len(idx) > nat.MAX_SEGMENTS and not strict:
                        failed.add(b)                                 # would outgrow the kernels: stop here
                        continue
                    mids = (wps[b][idx - 1] + wps[b][idx]) / 2
                    wps[b] = np.insert(wps[b], idx, mids, axis=0)
                    again.append(b)
            return again

        if len(cuboids) == 0:
            run_round(list(range(B)), None)
        todo = list(range(B))                                  # missions the next pass over the obstacles looks at
        for sweep in range(1 + max(0, int(recheck_passes))):
            touched = set()
            for cub in cuboids:
                active = [b for b in todo if b not in failed]
                for it in range(max_iterations + 1):
                    if not active:
                        break
                    active = run_round(active, cub)
                    touched.update(active)
                else:
                    if strict:
                        raise RuntimeError("obstacle correction did not converge (a waypoint inside an obstacle?)")
                    failed.update(active)
            todo = sorted(touched - failed)                     # only missions that changed can have new conflicts
            if not todo:
                break

        # stitch the final trajectories together in mission order
        nrows = torch.zeros((B,), dtype=torch.int64, device=self.device)
        by_plan = {}
        for b, (plan, j) in enumerate(source):
            by_plan.setdefault(id(plan), (plan, [], []))
            by_plan[id(plan)][1].append(b)
            by_plan[id(plan)][2].append(j)
        parts = []
        for plan, ids, js in by_plan.values():
            ids_t = torch.as_tensor(ids, device=self.device)
            js_t = torch.as_tensor(js, device=self.device)
            length = (plan.row_offsets[1:] - plan.row_offsets[:-1])[js_t]
            nrows[ids_t] = length
            parts.append((plan, ids_t, js_t, length))
        offsets = torch.zeros((B + 1,), dtype=torch.int64, device=self.device)
        offsets[1:] = torch.cumsum(nrows, 0)
        total = int(offsets[-1].item())
        traj = torch.empty((total, nat.TRAJ_COLS), dtype=torch.float64, device=self.device)
        for plan, ids_t, js_t, length in parts:
            rep = torch.repeat_interleave(torch.arange(len(js_t), device=self.device), length)
            within = torch.arange(int(length.sum().item()), device=self.device) - (torch.cumsum(length, 0) - length)[rep]
            traj[offsets[ids_t][rep] + within] = plan.traj[plan.row_offsets[js_t][rep] + within]
        starts = torch.as_tensor(np.stack([w[0] for w in wps]), dtype=torch.float64, device=self.device)
        converged = np.ones(B, dtype=bool)
        converged[sorted(failed)] = False
        return RaggedPlan(B, float(velocity), float(dt), wps, row_offsets=offsets, traj=traj, total_rows=total, start_positions=starts,
                          converged=converged)

    def plan_ragged(self, waypoints, velocity=1.0, dt: float = 0.01, cuboid=None, strict: bool = True,
                    rows: bool = True, times=None) -> RaggedBatch:
        """`MinimumSnap(path_b, None, velocity, dt).get_trajectory()` for B paths of DIFFERENT lengths in one batch
        (minimum_snap.py:13-57 takes any path; `Engine.plan` wants equal lengths).  `waypoints`: B arrays (m_b + 1, 3),
        1 <= m_b <= UAVAC_MAX_SEGMENTS.  Mission b's rows and coefficients equal those of `plan` on it alone, bit for
        bit.  `cuboid` (6,): also return per-spline hit flags (the collision scan of minimum_snap.py:81-87).
        `rows=False`: no rows (`batch.traj` is None), the first headings from `uavac_minsnap_first_yaw_dev`; not with `cuboid`.
        `velocity`: a number, or a (B,) tensor / array of one cruise speed per mission (see `plan`).
        `times`: B arrays (m_b,) of segment durations to plan from as given (see `plan`; `batch.free_times`); not with `cuboid`."""
        torch = self._torch
        wps = [np.ascontiguousarray(w, dtype=np.float64) for w in waypoints]
        B = len(wps)
        if B == 0 or any(w.ndim != 2 or w.shape[1] != 3 or w.shape[0] < 2 for w in wps):
            raise ValueError("waypoints must be B arrays of shape (m_b + 1, 3)")
        counts = np.array([w.shape[0] - 1 for w in wps], dtype=np.int64)
        max_m = int(counts.max())
        if max_m > nat.MAX_SEGMENTS:
            raise ValueError(f"a mission has {max_m} segments; at most {nat.MAX_SEGMENTS}")
        so_host = np.zeros(B + 1, dtype=np.int64)
        np.cumsum(counts, out=so_host[1:])
        S = int(so_host[-1])
        wp = self._dev(np.concatenate(wps, axis=0), torch.float64)
        so = self._dev(so_host, torch.int64)
        if times is not None:
            self._refuse_with_times(velocity, None)
            if cuboid is not None:
                raise ValueError("times= with a cuboid is not offered: Engine.audit(batch, obstacles) reports the hits")
            tms = [np.ascontiguousarray(t, dtype=np.float64).reshape(-1) for t in times]
            if len(tms) != B or any(t.shape[0] != c for t, c in zip(tms, counts)):
                raise ValueError("times must be B arrays of shape (m_b,)")
            return self._plan_from_times(wp, self._dev(np.concatenate(tms), torch.float64), dt, rows, strict, so=so, so_host=so_host,
                                         max_m=max_m)
        batch = self._plan_ragged_tensors(wp, so, so_host, max_m, velocity, dt, cuboid, rows)
        if strict:
            self.check(batch)
        return batch

    def _plan_ragged_tensors(self, wp, so, so_host, max_m: int, velocity, dt: float, cuboid, rows: bool = True) -> RaggedBatch:
        """`plan_ragged` on device-resident waypoints wp (S + B, 3) / seg_offsets so (B + 1,) (so_host: the same on the host)."""
        torch = self._torch
        B, S = len(so_host) - 1, int(so_host[-1])
        velocity, speeds = self._speeds(velocity, B)
        kw = dict(device=self.device)
        times = torch.empty((S,), dtype=torch.float64, **kw)
        seg_rows = torch.empty((S,), dtype=torch.int32, **kw)
        row_offsets = torch.empty((B + 1,), dtype=torch.int64, **kw)
        coeffs = torch.empty((S, 8, 3), dtype=torch.float64, **kw)
        status = torch.zeros((B,), dtype=torch.int32, **kw)
        first_yaw = torch.empty((B,), dtype=torch.float64, **kw)
        hit = aabb = None
        if cuboid is not None:
            hit = torch.empty((S,), dtype=torch.int32, **kw)
            aabb = self._dev(np.asarray(cuboid, dtype=np.float64).reshape(6), torch.float64)
        self._bind_stream()
        self._row_counts(wp, so, B, max_m, velocity, speeds, dt, times, seg_rows, row_offsets)
        self.ctx.call("uavac_minsnap_solve_ragged_dev", _ptr(wp), _ptr(times), _ptr(so), B, max_m, _ptr(coeffs), _ptr(status))
        batch = RaggedBatch(B, max_m, float(velocity), float(dt), seg_offsets=so, seg_offsets_host=so_host, waypoints=wp, times=times,
                            seg_rows=seg_rows, row_offsets=row_offsets, coeffs=coeffs, status=status, traj=None, total_rows=0,
                            first_yaw=first_yaw, hit=hit, velocities=speeds)
        if not rows:
            if cuboid is not None:
                raise ValueError("the collision scan walks the rows' positions: not with rows=False")
            self.ctx.call("uavac_minsnap_first_yaw_dev", _ptr(coeffs), _ptr(seg_rows), _ptr(so), B, max_m, float(dt), _ptr(first_yaw))
            batch.total_rows = int(row_offsets[-1].item())
            return batch
        batch.total_rows = total = int(row_offsets[-1].item())
        batch.traj = torch.empty((total, nat.TRAJ_COLS), dtype=torch.float64, **kw)
        self.ctx.call("uavac_minsnap_sample_ragged_dev", _ptr(coeffs), _ptr(seg_rows), _ptr(so), _ptr(row_offsets), B, max_m,
                      S, float(dt), _ptr(batch.traj), total, _ptr(aabb), _ptr(hit), _ptr(first_yaw))
        return batch

    def _row_counts(self, wp, so, B: int, m: int, velocity, velocities, dt: float, times, seg_rows, row_offsets, free_times: bool = False):
        """Durations, row counts and row offsets by the entry point that (`free_times`, `velocities`, ragged: `so` is not None) pick:
        from the durations as given, or from |leg| / speed at one cruise speed or at one per mission.  (The caller binds the stream.)"""
        out = (_ptr(seg_rows), _ptr(row_offsets))
        if free_times:
            self.ctx.call("uavac_minsnap_row_counts_t_dev", _ptr(times), _ptr(so), B, m, float(dt), *out)
            return
        name = {(False, False): "uavac_minsnap_row_counts_dev", (False, True): "uavac_minsnap_row_counts_v_dev",
                (True, False): "uavac_minsnap_row_counts_ragged_dev", (True, True): "uavac_minsnap_row_counts_ragged_v_dev"}
        head = (_ptr(wp),) if so is None else (_ptr(wp), _ptr(so))
        self.ctx.call(name[so is not None, velocities is not None], *head, B, m, float(velocity) if velocities is None else _ptr(velocities),
                      float(dt), _ptr(times), *out)

    def solve(self, plan: Plan):
        """Re-run times/row counts + coefficient solve into plan's buffers (no allocation, no sync); a `free_times` plan keeps its
        durations and re-runs the row counts and the solve from them."""
        self._bind_stream()
        self._row_counts(plan.waypoints, None, plan.B, plan.m, plan.velocity, getattr(plan, "velocities", None), plan.dt, plan.times,
                         plan.seg_rows, plan.row_offsets, free_times=getattr(plan, "free_times", False))
        if getattr(plan, "boundary", None) is not None:
            self.ctx.call("uavac_minsnap_solve_bc_dev", _ptr(plan.waypoints), _ptr(plan.times), None, plan.B, plan.m,
                          _ptr(plan.boundary), _ptr(plan.coeffs), _ptr(plan.status))
        else:
            self.ctx.call("uavac_minsnap_solve_dev", _ptr(plan.waypoints), _ptr(plan.times), plan.B, plan.m,
                          _ptr(plan.coeffs), _ptr(plan.status))
        plan.epoch += 1

    def sample(self, plan: Plan):
        """Re-run the sampler + yaw scan into plan.traj (and plan.yaw / plan.first_yaw when the plan has them); no
        allocation, no sync."""
        if plan.traj is None:
            raise ValueError("a rows-free plan has no row buffer: Engine.sample_rows(plan) allocates one and samples")
        self._bind_stream()
        # with the capacity of plan.traj: rows that would not fit are refused as a whole on the device (flag 2, `take_flags`)
        self.ctx.call("uavac_minsnap_sample_capped_dev", _ptr(plan.coeffs), _ptr(plan.seg_rows), _ptr(plan.row_offsets),
                      plan.B, plan.m, plan.dt, _ptr(plan.traj), int(plan.traj.shape[0]), _ptr(plan.yaw),
                      _ptr(getattr(plan, "first_yaw", None)))

    def check(self, plan: Plan):
        """Raise like the C ABI's host twins would: singular knot systems (repeated waypoints)."""
        if bool((plan.status != 0).any()):
            bad = int((plan.status != 0).nonzero()[0])
            raise nat.UavacError(nat.ESINGULAR, f"mission {bad}: singular knot system (repeated waypoint?)")

    # -- RRT* ---------------------------------------------------------------------
    def rrt_star(self, starts, goals, max_distance: float, samples, obstacles=None) -> "RRTDeviceBatch":
        """B independent RRT* runs (uav_ac/planning/rrt.py `RRTStar.run`), one wavefront each, inputs and results
        resident on the GPU.  `samples` (B, max_iterations, 3): the nodes `_generate_random_node` returns, e.g. from
        `uav_ac.planning.rrt.draw_random_nodes_batch`.  Layouts as documented in include/uavac.h."""
        torch = self._torch
        s = self._dev(starts, torch.float64)
        g = self._dev(goals, torch.float64)
        smp = self._dev(samples, torch.float64)
        if s.dim() != 2 or s.shape[1] != 3 or g.shape != s.shape:
            raise ValueError("starts and goals must both have shape (B, 3)")
        B = int(s.shape[0])
        if smp.dim() != 3 or smp.shape[0] != B or smp.shape[2] != 3 or smp.shape[1] < 1:
            raise ValueError("samples must have shape (B, max_iterations, 3)")
        if not bool(torch.isfinite(s).all() and torch.isfinite(g).all() and torch.isfinite(smp).all()):
            raise ValueError("starts, goals and samples must be finite")
        cub = None if obstacles is None else self._dev(np.asarray(obstacles, dtype=np.float64).reshape(-1, 6), torch.float64)
        n_obs = 0 if cub is None else int(cub.shape[0])
        max_iter = int(smp.shape[1])
        cap = max_iter + 1
        kw = dict(device=self.device)
        nodes = torch.empty((B, cap, 3), dtype=torch.float64, **kw)
        path = torch.empty((B, cap, 3), dtype=torch.float64, **kw)
        canon = torch.empty((B, cap), dtype=torch.int32, **kw)
        parent = torch.empty((B, cap), dtype=torch.int32, **kw)
        best_parent = torch.empty((B, cap), dtype=torch.int32, **kw)
        counts = torch.empty((B, 6), dtype=torch.int32, **kw)
        cost = torch.empty((B,), dtype=torch.float64, **kw)
        self._bind_stream()
        self.ctx.call("uavac_rrt_star_dev", _ptr(s), _ptr(g), B, float(max_distance), max_iter, _ptr(smp),
                      _ptr(cub) if n_obs else None, n_obs, _ptr(nodes), _ptr(canon), _ptr(parent), _ptr(best_parent),
                      _ptr(path), _ptr(counts), _ptr(cost))
        return RRTDeviceBatch(nodes, canon, parent, best_parent, path, counts, cost)

    def rrt_draw_nodes(self, seeds, goals, limits_lw, limits_up, n: int, epsilon: float = 0.15, with_consumed: bool = False):
        """What `RRTStar._generate_random_node` returns in `n` calls after `np.random.seed(seeds[b])`, for B problems,
        generated on the GPU (NumPy's legacy MT19937 stream, bit for bit) -> samples (B, n, 3) [, consumed (B, n)]."""
        torch = self._torch
        g = self._dev(np.round(np.asarray(goals.cpu() if isinstance(goals, torch.Tensor) else goals, dtype=np.float64), 2),
                      torch.float64)
        B = int(g.shape[0])
        sd = np.asarray(seeds, dtype=np.int64).reshape(-1)
        if len(sd) != B or sd.min() < 0 or sd.max() > 0xffffffff:
            raise ValueError("one seed in [0, 2**32) per problem")
        sd_t = torch.as_tensor(sd.astype(np.uint32).view(np.int32), device=self.device)
        lw = np.ascontiguousarray(limits_lw, dtype=np.float64)[:3].copy()
        up = np.ascontiguousarray(limits_up, dtype=np.float64)[:3].copy()
        samples = torch.empty((B, int(n), 3), dtype=torch.float64, device=self.device)
        consumed = torch.empty((B, int(n)), dtype=torch.int64, device=self.device) if with_consumed else None
        self._bind_stream()
        self.ctx.call("uavac_rrt_draw_nodes_dev", _ptr(sd_t), _ptr(g), B, int(n), nat.np_ptr(lw), nat.np_ptr(up), float(epsilon),
                      _ptr(samples), _ptr(consumed))
        return (samples, consumed) if with_consumed else samples

    def rrt_star_seeded(self, starts, goals, space_limits, seeds, max_distance: float, max_iterations: int, obstacles=None,
                        epsilon: float = 0.15) -> "RRTDeviceBatch":
        """B runs of `np.random.seed(seeds[b]); RRTStar(space_limits, starts[b], goals[b], max_distance, max_iterations,
        obstacles).run()` entirely on the GPU: the node draws (`rrt_draw_nodes`) and the planner (`rrt_star`)."""
        goals = np.round(np.asarray(goals, dtype=np.float64), 2)
        samples = self.rrt_draw_nodes(seeds, goals, space_limits[0], space_limits[1], max_iterations, epsilon)
        return self.rrt_star(starts, goals, max_distance, samples, obstacles)

    def rrt_simplify(self, batch: "RRTDeviceBatch", obstacles=None):
        """`RRTStar.simplify_path` (rrt.py:93-116) of every best path of `batch` in one launch.
        -> (paths (B, cap, 3), lengths (B,)) on the GPU; rows past a path's length are zero."""
        torch = self._torch
        B, cap = int(batch.best_path.shape[0]), int(batch.best_path.shape[1])
        cub = None if obstacles is None else self._dev(np.asarray(obstacles, dtype=np.float64).reshape(-1, 6), torch.float64)
        n_obs = 0 if cub is None else int(cub.shape[0])
        lens = batch.counts[:, 4].contiguous()
        out = torch.empty_like(batch.best_path)
        out_lens = torch.empty((B,), dtype=torch.int32, device=self.device)
        self._bind_stream()
        self.ctx.call("uavac_rrt_simplify_dev", _ptr(batch.best_path), _ptr(lens), B, cap, _ptr(cub) if n_obs else None, n_obs,
                      _ptr(out), _ptr(out_lens))
        return out, out_lens

    # -- control ----------------------------------------------------------------
    def fleet(self, plan: Plan, vehicle: Optional[nat.Vehicle] = None, hover: bool = True,
              positions=None, from_plan=None, yaw_from: str = "scan") -> "Fleet":
        from .fleet import Fleet
        return Fleet(self, plan, vehicle, hover, positions, from_plan, yaw_from)
