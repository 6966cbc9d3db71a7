"""What `Engine` hands out: the device-resident plans (`Plan`, `RaggedBatch`, `RaggedPlan`), the one view of a plan's segments that
the calls behind them share (`segments`), and the result records of the audits, searches and transforms.  No arithmetic here and no
call into the C ABI: `uav_ac.engine` does that and re-exports every name of this module."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from functools import lru_cache
from typing import NamedTuple

import numpy as np

from . import _native as nat

_P = C.c_void_p


def _ptr(t) -> _P:
    return _P(0 if t is None else t.data_ptr())


@dataclass
class Plan:
    """Device-resident result of planning B missions of m segments."""
    B: int
    m: int
    velocity: float
    dt: float
    waypoints: "object"      # (B, m+1, 3) f64
    times: "object"          # (B, m) f64
    seg_rows: "object"       # (B, m) i32
    row_offsets: "object"    # (B+1,) i64
    coeffs: "object"         # (B, 8m, 3) f64
    status: "object"         # (B,) i32: 0 ok, 1 singular
    traj: "object"           # (N, 11) f64, missions back to back; None for a rows-free plan (Engine.plan(..., rows=False))
    total_rows: int          # N (known for a rows-free plan too: what the root of a plan gather will sample; after
                             # `Engine.replan` it is re-read from the device on first use, see _plan_total_rows)
    yaw: "object" = None     # (N,) f64 or None: the yaw column on its own (== traj[:, 9]); one way to feed the plan-fed rollout
    first_yaw: "object" = None   # (B,) f64: heading of each mission's first row that has one; lets the rollout scan the yaw itself
    placement_ms: "object" = None    # sampler times of the candidate row buffers when plan(..., placement_trials > 1) chose one
    pooled: bool = False             # the rows live in the Engine's pooled buffer (shared with every other pooled plan of that Engine)
    epoch: int = 0                   # bumped whenever the plan is re-solved / re-sampled in place (Engine.replan / solve / sample):
                                     # an attached Fleet then rebuilds the yaw scan it carries instead of trusting a stale one
    velocities: "object" = None      # (B,) f64, device: one cruise speed per mission (`velocity` is then NaN); None = the one `velocity`
    boundary: "object" = None        # (B, 6, 3) f64, device: (v, a, j) at the first waypoint (rows 0-2) and at the last (rows 3-5); None =
                                     # rest to rest.  Read again at every replan / solve.  Such a plan always has `velocities` (a scalar
                                     # `velocity` is kept and broadcast)
    free_times: bool = False         # the durations were GIVEN (`Engine.plan(..., times=...)`, `Engine.optimize_times`), not derived from a
                                     # speed: `velocity` is NaN, `velocities` None; replan / solve re-run the chain from `times` as they stand

    def mission(self, b: int) -> np.ndarray:
        """Rows of mission b as a fresh host array (N_b, 11) -- the reference's `full_trajectory`."""
        if self.traj is None:
            raise ValueError("a rows-free plan holds no rows: Engine.sample_rows(plan) samples them")
        ro = self.row_offsets[b:b + 2].cpu().numpy()
        return self.traj[int(ro[0]):int(ro[1])].cpu().numpy().copy()

    @property
    def algorithmic_bytes(self) -> int:
        """24(m+1) in + 192 m coefficients out + 88 N rows out, per mission, summed (a rows-free plan: the
        first heading, 8 B per mission, instead of the rows)."""
        rows = 88 * self.total_rows if self.traj is not None else 8 * self.B
        return self.B * (24 * (self.m + 1) + 192 * self.m) + rows


def _plan_total_rows(self) -> int:
    # `Engine.replan` leaves the new row count on the device only (replan does not synchronise): the first reader after it --
    # `RcclComm.plan_counts`, whose all-gather sizes the root's row buffer, among them -- takes it from there.
    if self.__dict__.get("_rows_stale"):
        self.__dict__["_total_rows"] = int(self.row_offsets[-1].item())
        self.__dict__["_rows_stale"] = False
    return self.__dict__["_total_rows"]


def _set_plan_total_rows(self, value):
    self.__dict__["_total_rows"] = int(value)
    self.__dict__["_rows_stale"] = False


Plan.total_rows = property(_plan_total_rows, _set_plan_total_rows)


@dataclass
class RaggedPlan:
    """Trajectories of B missions whose segment counts differ (after obstacle-driven midpoint insertion).
    Has what `Fleet` needs from a Plan: traj, row_offsets, start positions."""
    B: int
    velocity: float
    dt: float
    final_waypoints: list            # B host arrays (m_b + 1, 3): the waypoint lists after insertion
    row_offsets: "object"            # (B+1,) i64
    traj: "object"                   # (N, 11) f64
    total_rows: int
    start_positions: "object"        # (B, 3) f64
    converged: "object" = None       # (B,) bool, host: False where the bounded obstacle loop gave up
    batch: "object" = None           # the RaggedBatch the rows were sampled from (coefficients, rows per spline, first headings):
                                     # lets a Fleet fly the plan from its coefficients and RcclComm.gather_plan ship it

    def mission(self, b: int) -> np.ndarray:
        ro = self.row_offsets[b:b + 2].cpu().numpy()
        return self.traj[int(ro[0]):int(ro[1])].cpu().numpy().copy()

    def __getattr__(self, name):     # coeffs, seg_rows, seg_offsets, first_yaw, max_m, times ...: the batch's, when there is one
        batch = self.__dict__.get("batch")
        if batch is not None and name in ("coeffs", "seg_rows", "seg_offsets", "seg_offsets_host", "first_yaw", "max_m", "times",
                                          "waypoints", "status"):
            return getattr(batch, name)
        raise AttributeError(name)


@dataclass
class RaggedBatch:
    """One ragged planning call (`Engine.plan_ragged`): B missions with m_b segments each, everything per-segment back to
    back in mission order (include/uavac.h, "Ragged batches")."""
    B: int
    max_m: int
    velocity: float
    dt: float
    seg_offsets: "object"            # (B+1,) i64, device
    seg_offsets_host: np.ndarray     # the same on the host
    waypoints: "object"              # (S + B, 3) f64
    times: "object"                  # (S,) f64
    seg_rows: "object"               # (S,) i32
    row_offsets: "object"            # (B+1,) i64
    coeffs: "object"                 # (S, 8, 3) f64
    status: "object"                 # (B,) i32, 0 = ok
    traj: "object"                   # (N, 11) f64; None for a rows-free batch
    total_rows: int
    first_yaw: "object"              # (B,) f64
    hit: "object" = None             # (S,) i32 when a cuboid was given
    velocities: "object" = None      # (B,) f64, device: one cruise speed per mission (`velocity` is then NaN); None = the one `velocity`
    free_times: bool = False         # the durations were given (`Engine.plan_ragged(..., times=...)`, `Engine.optimize_times`): see Plan

    def mission(self, b: int) -> np.ndarray:
        if self.traj is None:
            raise ValueError("a rows-free batch (plan_ragged(..., rows=False)) holds no rows")
        ro = self.row_offsets[b:b + 2].cpu().numpy()
        return self.traj[int(ro[0]):int(ro[1])].cpu().numpy().copy()

    @property
    def start_positions(self):
        """(B, 3): first waypoint of every mission (what `Fleet` starts its vehicles from)."""
        import torch
        if self.waypoints is None:                  # assembled from gathered parts: c0 of a mission's first spline IS its first waypoint
            return self.coeffs[self.seg_offsets[:-1], 0, :]
        first = self.seg_offsets[:-1] + torch.arange(self.B, dtype=self.seg_offsets.dtype, device=self.seg_offsets.device)
        return self.waypoints[first]

    def mission_coeffs(self, b: int) -> np.ndarray:
        s0, s1 = int(self.seg_offsets_host[b]), int(self.seg_offsets_host[b + 1])
        return self.coeffs[s0:s1].reshape(-1, 3).cpu().numpy().copy()


class Segments(NamedTuple):
    """How a plan's segments are laid out, whichever kind it is (`segments`)."""
    ragged: bool             # a RaggedBatch (or a RaggedPlan that has one): segments back to back, m_b per mission
    B: int
    m: int                   # the largest segment count per mission (a uniform Plan: its m)
    S: int                   # the segment total
    so: "object"             # (B+1,) i64, device: the segment offsets; None for a uniform Plan (NULL in the C ABI)
    so_host: np.ndarray      # the same on the host; arange(B + 1) * m for a uniform Plan -- shared and read-only: copy it to keep it


@lru_cache(maxsize=16)
def _uniform_offsets_host(B: int, m: int) -> np.ndarray:
    so = np.arange(B + 1, dtype=np.int64) * m
    so.flags.writeable = False
    return so


def uniform_offsets(B: int, m: int, device):
    """The segment offsets of a uniform plan as a fresh (B+1,) i64 device tensor: what a RaggedBatch made from one carries."""
    import torch
    return torch.arange(B + 1, dtype=torch.int64, device=device) * m


def segments(plan) -> Segments:
    """The one place that asks whether a plan is uniform or ragged.  (`hasattr(plan, "seg_offsets")` stays the way to tell them
    apart, so `Plan` gets no such attribute.)"""
    B = int(plan.B)
    if hasattr(plan, "seg_offsets"):
        return Segments(True, B, int(plan.max_m), int(plan.seg_offsets_host[-1]), plan.seg_offsets, plan.seg_offsets_host)
    m = int(plan.m)
    return Segments(False, B, m, B * m, None, _uniform_offsets_host(B, m))


@dataclass
class PlanAudit:
    """What the sampled rows of a plan would show, per mission (`Engine.audit`, include/uavac.h uavac_minsnap_audit_dev): device
    tensors, the peaks (B,) f64 -- maxima over exactly the rows the sampler writes, NaN for a mission with a non-finite sample --
    and per cuboid (n, B) i32 how many samples lie inside it and the mission-local index of the first one (-1: none).
    `uav_ac.scoring.plan_feasibility` judges it against a vehicle's flight limits."""
    rows: "object"           # (B,) f64: the mission's row total
    speed_xy: "object"       # peak sqrt(vx^2 + vy^2)
    ascent: "object"         # peak climb rate max(-vz) (NED)
    descent: "object"        # peak descent rate max(vz)
    accel_xy: "object"       # peak sqrt(ax^2 + ay^2)
    accel_up: "object"       # peak max(-az)
    accel_down: "object"     # peak max(az)
    speed: "object"          # peak sqrt(vx^2 + vy^2 + vz^2)
    hit_rows: "object"       # (n, B) i32
    first_hit: "object"      # (n, B) i32
    block: "object" = None   # the [AUDIT_ROWS][B] block the eight rows above are views of


@dataclass
class PlanDemand:
    """What a plan asks of the vehicle, per mission (`Engine.demand`, include/uavac.h uavac_minsnap_demand_dev): device tensors, maxima
    and minima over exactly the rows the sampler writes -- NaN, and -1 in every index, for a mission with a non-finite sample or
    without rows.  The thrust columns are SPECIFIC thrust in m/s^2; newtons are `vehicle.mass` times that.
    `uav_ac.scoring.demand_feasibility` judges it against the vehicle, `uav_ac.scoring.audit_gap` sets it beside a FlightAudit."""
    rows: "object"           # (B,) f64: the mission's row total
    thrust_max: "object"     # peak |a - g e3|: the specific thrust a perfectly tracked plan needs
    thrust_min: "object"     # ... and the least of it (0: a row in free fall)
    bank_x: "object"         # peak |ax| / |a - g e3|: the bank command that max_tilt clips (control_law.h), as the plan demands it
    bank_y: "object"         # peak |ay| / |a - g e3|
    body_rate: "object"      # peak roll / pitch rate the curve demands, rad/s (no yaw rate)
    inverted_rows: "object"  # (B,) i32: rows that ask for thrust downward (g - az <= 0)
    first_inverted: "object"  # (B,) i32: the mission-local index of the first of them (-1: none)
    clearance: "object"      # (n, B) f64: closest approach of a sample to cuboid c (0 inside or on a face)
    clearance_row: "object"  # (n, B) i32: the mission-local index of the first row that attains it
    block: "object" = None   # the [DEMAND_ROWS][B] block the six f64 rows above are views of


@dataclass
class PlanNeed:
    """By how much each mission must be slowed down for the vehicle to be able to give what the plan asks (`Engine.need`, include/uavac.h
    uavac_minsnap_need_dev): device tensors (B,) f64, per limit the slowdown FACTOR it asks for on its own -- above 1: the plan breaks
    that limit; 0: no row comes near it -- from maxima over exactly the rows the sampler writes; NaN for a mission with a non-finite
    sample or without rows.  `uav_ac.scoring.retime_factors(..., need=...)` and `Engine.retime(..., demand=True)` act on it."""
    tilt: "object"           # the bank command within max_tilt about both axes
    upright: "object"        # no row asks for thrust downward
    thrust_max: "object"     # four rotors at max_thrust suffice
    thrust_min: "object"     # four rotors at min_thrust do not push too hard
    block: "object" = None   # the [NEED_ROWS][B] block the four rows above are views of


@dataclass
class SeparationAudit:
    """The fleet's audit against itself (`Engine.separation`, include/uavac.h uavac_minsnap_separation_dev): device tensors, per
    mission over the shared row clock of its group.  An excluded mission (no rows, or a coefficient that is not finite) reports NaN /
    -1 / -1 / 0 / -1 / 0.  `uav_ac.scoring.separation_ok` turns it into verdicts."""
    min_distance: "object"   # (B,) f64: closest approach to any other mission of the group; +inf when there was nobody to compare with
    partner: "object"        # (B,) i32: batch index of that mission (-1 with +inf / NaN)
    row: "object"            # (B,) i32: clock row of the closest approach (-1 with +inf / NaN); from `Engine.flown_separation`: the tick
    conflicts: "object"      # (B,) i32: how many other missions come inside the radius
    first_conflict: "object"  # (B,) i32: first clock row with anybody inside the radius (-1: none)
    compared: "object"       # (B,) i32: how many partners the mission was compared with (group size - 1 unless some are excluded)
    block: "object" = None   # the [SEP_ROWS][B] i32 block the five rows above are views of


@dataclass
class ConflictList:
    """The separation audit's conflict graph in CSR form (`Engine.conflicts`, include/uavac.h uavac_minsnap_conflicts_dev): device
    tensors.  Mission i lists its partners -- every mission of its group that comes inside the radius at some row of the shared clock
    -- in the entries [offsets[i], offsets[i + 1]), in ascending batch index; a pair shows in both directions, with the same record.
    `uav_ac.scoring.conflict_pairs` gives the unique pairs on the host.  From `Engine.flown_conflicts` (uavac_flown_conflicts_dev) the
    same record of a FLIGHT: vehicles for missions, and TICKS of the state log in the `*_row` fields."""
    offsets: "object"        # (B + 1,) i64: exclusive prefix sum of the audit's `conflicts`
    partner: "object"        # (E,) i32: batch index of the partner
    first_row: "object"      # (E,) i32: first clock row at which the pair is inside the radius
    last_row: "object"       # (E,) i32: last such row
    rows_inside: "object"    # (E,) i32: how many rows (less than last - first + 1 when the pair parts and meets again)
    min_row: "object"        # (E,) i32: clock row of the pair's closest approach, the lowest one on a tie
    min_distance: "object"   # (E,) f64: the pair's closest approach over the group's clock
    total: int = 0           # E, the number of entries (twice the number of pairs)
    block: "object" = None   # the [CONF_ROWS][E] i32 block the five rows above are views of


@dataclass
class FlightAudit:
    """What the vehicles DID, per vehicle, from a rollout's state log (`Engine.flown_audit`, include/uavac.h uavac_flown_audit_dev):
    device tensors.  A tick counts iff all 13 logged values are finite; the peaks (B,) f64 are maxima over those ticks (NaN when there
    is none), and per cuboid (n, B) the ticks spent inside it, the first of them, and the closest approach with its tick.
    `uav_ac.scoring.flight_feasibility` judges it against a vehicle's flight limits."""
    ticks: "object"          # (B,) f64: the number of valid ticks
    speed_xy: "object"       # peak sqrt(vx^2 + vy^2)
    ascent: "object"         # peak climb rate max(-vz) (NED)
    descent: "object"        # peak descent rate max(vz)
    speed: "object"          # peak sqrt(vx^2 + vy^2 + vz^2)
    bank_x: "object"         # peak |2 (q1 q3 + q0 q2)|: the rotation-matrix element R13 that max_tilt clips in the command
    bank_y: "object"         # peak |2 (q2 q3 - q0 q1)|: R23
    body_rate: "object"      # peak sqrt(p^2 + q^2 + r^2)
    first_bad: "object"      # (B,) i32: the first tick with a value that is not finite (-1: none)
    hit_ticks: "object"      # (n, B) i32: valid ticks inside cuboid c
    first_hit: "object"      # (n, B) i32: the first of them (-1: none)
    clearance: "object"      # (n, B) f64: closest approach to cuboid c (0 inside or on a face; NaN without a valid tick)
    clearance_tick: "object"  # (n, B) i32: its tick (the first such tick; -1 without a valid tick)
    block: "object" = None   # the [FLOWN_AUDIT_ROWS][B] block the eight rows above are views of


@dataclass
class StaggerResult:
    """Start delays that clear the separation audit (`Engine.stagger`, include/uavac.h uavac_minsnap_stagger_dev): device tensors, per
    mission.  `Engine.separation(plan, radius, groups, start_rows=result.start_rows)` confirms it; `uav_ac.scoring.stagger_ok` turns
    it into verdicts."""
    start_rows: "object"     # (B,) i32: the granted start row (the base start for an unresolved or unexamined mission)
    steps: "object"          # (B,) i32: the candidate index granted (delay = steps * step rows); -1 unresolved; -2 not examined
    earlier: "object"        # (B,) i32: how many missions it was checked against (the included missions before it in its group)
    block: "object" = None   # the [STAGGER_ROWS][B] i32 block the three rows above are views of


@dataclass
class LayerResult:
    """Offset layers that clear the separation audit at fixed starts (`Engine.layer`, include/uavac.h uavac_minsnap_layer_dev): device
    tensors, per mission.  `Engine.separation(Engine.shift(plan, result.offsets), radius, groups, start_rows)` confirms it;
    `uav_ac.scoring.layer_ok` turns it into verdicts."""
    layers: "object"         # (B,) i32: the granted layer (0 for an unresolved or unexamined mission)
    steps: "object"          # (B,) i32: the candidate index granted (== layers); -1 unresolved; -2 not examined
    earlier: "object"        # (B,) i32: how many missions it was checked against (the included missions before it in its group)
    block: "object" = None   # the [LAYER_ROWS][B] i32 block the three rows above are views of; [LAYER_OBS_ROWS][B] from a search with obstacles
    offsets: "object" = None  # (B, 3) f64: the granted layer * delta, what `Engine.shift` takes

    @property
    def blocked(self):
        """(B,) i32 from a search with obstacles (`Engine.layer(..., obstacles=)`): how many of the candidates below the granted layer
        (all of them for an unresolved mission) a cuboid refused -- row 3 of `block`; None from a search without obstacles."""
        if self.block is None or self.block.shape[0] != nat.LAYER_OBS_ROWS:
            return None
        return self.block[nat.LAYER_OBS_ROWS - 1]


@dataclass
class PlanEnvelope:
    """Every mission's swept box (`Engine.envelope`, include/uavac.h uavac_minsnap_envelope_dev): device tensors, the minimum and the
    maximum per axis of the positions the sampler writes -- with a reach, of the shifted plan's as well.  NaN in all six for a mission
    without rows or with a position that is not finite."""
    lo: "object"             # (B, 3) f64
    hi: "object"             # (B, 3) f64
    block: "object" = None   # the [B][6] block the two above are views of


@dataclass
class Airspaces:
    """A fleet split into groups that can never meet (`Engine.airspaces`, include/uavac.h uavac_fleet_airspaces_dev): the connected
    components of "swept boxes nearer than the radius", per caller group, and the order that puts each of them side by side."""
    labels: "object"         # (B,) i32, device: the lowest batch index of the mission's airspace (final: the engine resumes until they are)
    order: "object"          # (B,) i32, device: the mission in every slot -- sorted by label within each caller group, stably
    rank: "object"           # (B,) i32, device: its inverse, rank[order[s]] = s
    offsets: "object"        # (A + 1,) i64, device: airspace a holds the slots [offsets[a], offsets[a + 1]) -- what the searches take as groups
    offsets_host: np.ndarray  # the same on the host
    sizes_host: np.ndarray   # (A,) i64, host: diff(offsets_host)
    largest: int             # the largest airspace: at most 256 takes the narrow searches, more the wide ones with group_cap = largest
    rounds: int              # labelling rounds that changed a label


@dataclass
class DeconflictResult:
    """What `Engine.deconflict` returns: the plan to fly and the two searches it was made from."""
    plan: "object"           # rows-free RaggedBatch: delay(shift(plan, layer.offsets), stagger.start_rows)
    stagger: StaggerResult   # the start delays (`Engine.stagger`)
    layer: LayerResult       # the offset layers at those starts (`Engine.layer`, with the obstacles if any were given)
    resolved: "object"       # (B,) bool, device: layer.steps >= 0


@dataclass
class RetimeResult:
    """What `Engine.retime` returns: the plan at speeds that keep every converged mission inside the flight limits."""
    plan: "object"           # of the kind that was given (Plan / RaggedBatch / RaggedPlan), planned at `velocities`; with rows if it had rows
    velocities: "object"     # (B,) f64, device: the cruise speed of every mission after retiming (== plan.velocities)
    factors: "object"        # (B,) f64: product of the mission's slow-down factors (1.0: never touched; NaN: a NaN peak, e.g. singular)
    passes: int              # retimings done (0: every mission was inside the limits, or max_passes = 0)
    converged: "object"      # (B,) bool: the mission's last audit asked for no retiming
    audit: PlanAudit         # the audit of `plan` (no cuboids)
    need: "object" = None    # `retime(demand=True)`: the PlanNeed of `plan`; None otherwise
    binding: "object" = None  # `retime(demand=True)`: (B,) i32, the index into scoring.BINDING_NAMES of the limit nearest to each mission in
                              # its last audit (the first of equals; -1: a NaN mission); None otherwise


@dataclass
class TimeOptResult:
    """What `Engine.optimize_times` returns."""
    plan: "object"           # a NEW free_times plan of the kind that was given (Plan / RaggedBatch) on the same waypoints, planned from the
                             # optimised durations
    cost_before: "object"    # (B,) f64, device: snap cost of the input's durations
    cost_after: "object"     # (B,) f64: snap cost of `plan` (== Engine.cost(plan), bit for bit); <= cost_before
    accepted: "object"       # (B,) i32: steps the mission took (0: its durations are the input's, bit for bit)


@dataclass
class RRTDeviceBatch:
    """Device-resident results of `Engine.rrt_star` (torch tensors; layouts of include/uavac.h).
    counts[:, k]: 0 n_nodes, 1 iterations begun, 2 status, 3 entries when best_tree was stored, 4 best_path rows,
    5 dynamic_it_counter."""
    nodes: "object"
    canon: "object"
    parent: "object"
    best_parent: "object"
    best_path: "object"
    counts: "object"
    best_cost: "object"

    def to_host(self):
        """-> uav_ac.planning.rrt.RRTBatch (NumPy)."""
        from .planning.rrt import RRTBatch
        c = self.counts.cpu().numpy()
        return RRTBatch(self.nodes.cpu().numpy(), self.canon.cpu().numpy(), self.parent.cpu().numpy(),
                        self.best_parent.cpu().numpy(), self.best_path.cpu().numpy(), c[:, 0].copy(), c[:, 1].copy(),
                        c[:, 2].copy(), c[:, 3].copy(), c[:, 4].copy(), c[:, 5].copy(), self.best_cost.cpu().numpy())
