"""The build checks: what `make`, `__graft_entry__.build()` and the autobuild of `uav_ac._native.lib()` run on the object files
under build/ before a library counts as built (`run_all`), and what the CPU tests call piece by piece.

* One reader (`read_object`) takes an object file's gfx950 code object apart once per process: a record per kernel from the
  metadata notes (`parse_kernels`), the disassembly on demand (`_disassemble_cfg`).
* One table (`BUDGETS`) says per object file which kernels must be there, how many, and how many vector registers each may
  take; one function (`check_budget`) applies a row.  A kernel past its budget still computes the right thing, only slower -- a
  logged rollout launch at 258 vector registers (a 6-register 'optimisation' tried in round 3) took 1.96 ms instead of 1.27 ms:
  one wave per SIMD instead of two -- so no functional test sees it and a toolchain bump can cross it silently.
* `UNBUDGETED` lists the object files that have no budget; an object file in neither list fails the build (`check_inventory`).
* The two hand-placed prefetches are followed in the disassembly (`check_row_prefetch`, `check_heading_prefetch`); the shipped
  library exports no diagnostic symbol (`check_no_diagnostics`).

A check that cannot run (no object files, no LLVM tools: a library that was built elsewhere) answers None; `run_all` treats
that as a failure."""
import collections
import os
import re
import shutil
import subprocess
import tempfile

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM_BIN = "/opt/rocm/lib/llvm/bin"

Kernel = collections.namedtuple("Kernel", "name vgpr_count vgpr_spill_count sgpr_count sgpr_spill_count agpr_count "
                                          "private_segment_fixed_size group_segment_fixed_size")


def parse_kernels(notes: str):
    """[Kernel] from the text of a code object's metadata notes (`llvm-readelf --notes`): the items of the `amdhsa.kernels:` list,
    each read from the keys that stand at the item's own indentation -- by name, in whatever order; the `.name` of a kernel
    argument stands deeper and is not one of them.  Notes without that list (no device code): no kernels."""
    body = re.search(r"^amdhsa\.kernels:[^\n]*\n((?:[ \t]+[^\n]*\n?)*)", notes, flags=re.M)
    dash = re.match(r"( *)- ", body.group(1)) if body else None
    if not dash:
        return []
    indent, kernels = dash.group(1), []
    for item in re.split(rf"^{indent}- ", body.group(1), flags=re.M)[1:]:
        keys = dict(re.findall(rf"^(?:{indent}  )?\.(\w+):[ \t]*(\S*)", item, flags=re.M))     # (the item's first line lost its indentation to the split)
        try:
            kernels.append(Kernel(keys["name"], *(int(keys[f]) for f in Kernel._fields[1:])))
        except KeyError as exc:
            raise RuntimeError(f"kernel {keys.get('name')}: no {exc} in the code object's metadata")
    return kernels


def template_args(name: str):
    """The literal template arguments at the head of a mangled kernel name's argument list, ints and bools in order:
    `..control_rollout_kernelILi4ELi2ELb0E..EEv..` -> (4, 2, False, ..); () for a kernel that is no template."""
    head = re.search(r"I((?:L[a-z]n?\d+E)+)", name)
    return tuple(v == "1" if t == "b" else int(v.replace("n", "-")) for t, v in re.findall(r"L([a-z])(n?\d+)E", head.group(1))) if head else ()


class Ins(str):
    """One instruction of a disassembled kernel: its text (the str itself), its address and, for a branch, the address it may go to."""
    addr = None
    target = None

    def __new__(cls, text, addr=None, target=None):
        self = super().__new__(cls, text)
        self.addr, self.target = addr, target
        return self


_BRANCH = ("s_cbranch", "s_branch")
_INDIRECT = ("s_setpc", "s_swappc", "s_call", "s_rfe", "s_cbranch_g_fork", "s_cbranch_i_fork", "s_cbranch_join")


def parse_listing(text: str):
    """{kernel name: [Ins]} from the text of `llvm-objdump -d --no-show-raw-insn`: instruction text with its address and branch
    target, which is what a check needs to follow the control flow."""
    kernels, cur, base = {}, None, 0
    for line in text.splitlines():
        head = re.match(r"([0-9a-f]+) <([^>]+)>:", line)
        if head:
            base = int(head.group(1), 16)
            cur = kernels.setdefault(head.group(2), [])
        elif cur is not None:
            code, _, note = line.partition("//")
            ins = code.strip()
            if not ins or ins.endswith(":"):
                continue
            at = re.match(r"\s*([0-9A-Fa-f]+):", note)
            to = re.search(r"<[^>]*\+0x([0-9a-fA-F]+)>\s*$", note) if ins.startswith(_BRANCH) else None
            if ins.startswith(_BRANCH) and to is None and re.search(r"<[^>+]+>\s*$", note):
                to_addr = base                                            # a branch to the kernel's first instruction
            else:
                to_addr = base + int(to.group(1), 16) if to else None
            cur.append(Ins(ins, int(at.group(1), 16) if at else None, to_addr))
    return kernels


_objects = {}            # what `read_object` has read in this process, by path


def read_object(obj: str):
    """The gfx950 code object inside an object file, taken out once: {"kernels": [Kernel], "image": the code object's bytes,
    "listing": None until `_disassemble_cfg` fills it}.  An object file without device code reads as no kernels; None when the
    object file or the LLVM tools are not there.  Kept per process and read again when the file's size or modification time, or
    LLVM_BIN, is no longer what it was."""
    objdump, readelf = os.path.join(LLVM_BIN, "llvm-objdump"), os.path.join(LLVM_BIN, "llvm-readelf")
    if not (os.path.exists(obj) and os.path.exists(objdump) and os.path.exists(readelf)):
        return None
    stat = os.stat(obj)
    seen = (stat.st_size, stat.st_mtime_ns, LLVM_BIN)
    if obj not in _objects or _objects[obj]["seen"] != seen:
        notes, image = "", b""
        with tempfile.TemporaryDirectory() as tmp:
            shutil.copy(obj, os.path.join(tmp, "o.o"))
            subprocess.run([objdump, "--offloading", "o.o"], cwd=tmp, check=True, capture_output=True)
            for co in (f for f in os.listdir(tmp) if "gfx950" in f):
                notes = subprocess.run([readelf, "--notes", os.path.join(tmp, co)], check=True, capture_output=True, text=True).stdout
                with open(os.path.join(tmp, co), "rb") as fh:
                    image = fh.read()
        _objects[obj] = {"seen": seen, "kernels": parse_kernels(notes), "image": image, "listing": None}
    return _objects[obj]


def _disassemble_cfg(obj: str):
    """{kernel name: [Ins]} of the code object inside `obj` (`parse_listing`), disassembled once; None like `read_object`."""
    co = read_object(obj)
    if co is None:
        return None
    if co["listing"] is None:
        with tempfile.NamedTemporaryFile(suffix=".co") as fh:
            fh.write(co["image"])
            fh.flush()
            co["listing"] = parse_listing(subprocess.run([os.path.join(LLVM_BIN, "llvm-objdump"), "-d", "--no-show-raw-insn", fh.name],
                                                         check=True, capture_output=True, text=True).stdout if co["image"] else "")
    return co["listing"]


# ------------------------------------------------------------------------------------------------ the budgets
LDS_BYTES_PER_CU = 160 * 1024
VGPRS_AT_WAVES_PER_SIMD = {8: 64, 7: 72, 6: 80, 5: 96, 4: 128, 3: 168, 2: 256, 1: 512}     # the largest allocation that still runs that many
FROM_LDS = "from the LDS the kernel ends up with"

# One row per budget.  `key`: where `run_all` reports the row (rows may share one); `obj`: the object file(s) under build/;
# `noun`: what messages call the kernels; `kernels`: names that must be there.  The object holds exactly len(kernels) + `extra`
# kernels (further instantiations of a listed one) -- or, with `at_least`, at least that many kernels of the listed names, and
# the row speaks of those alone.  `limit`, the most vector registers a kernel may take: a number; {kernel: number}; a function
# of the kernel's template arguments; or FROM_LDS -- workgroups of four waves, so min(8, 160 KiB // LDS) workgroups per CU are
# as many waves per SIMD, and the kernel must fit the allocation that still runs that many; a decision kernel of the layer
# search, and of the block-wise searches, must keep three workgroups per CU.  No kernel may spill a vector register; with `scratch_free` none may use scratch
# memory at all (zero private-segment bytes).
Budget = collections.namedtuple("Budget", "key obj noun kernels limit extra at_least scratch_free", defaults=(0, None, True))
BUDGETS = (
    # every rollout variant fits TWO waves on a SIMD: a logged launch puts a compute and a store wave of one kernel on each
    Budget("rollout_registers", "control_rollout.o", "rollout", ("control_rollout_kernel",), 256, at_least=40, scratch_free=False),
    # the chunk-streaming sampler: six waves per SIMD, four with jerk / snap or sixteen waves (a spill here showed as 3 % more HBM
    # writes and no other symptom, NOTES R4-2)
    Budget("planning_registers", "minsnap_sample_stream.o", "streaming-sampler", ("minsnap_sample_stream_kernel",),
           lambda w, hits, derivs, ragged: 128 if derivs or w == 16 else 80, at_least=20, scratch_free=False),
    # the one-ended and the two-ended solve: two waves per SIMD, one for the variant that keeps five knots in registers
    Budget("planning_registers", "minsnap_solve_bt.o minsnap_solve_tw.o", "solve", ("minsnap_solve_bt_kernel", "minsnap_solve_tw_kernel"),
           lambda ragged, park_lds, n, nreg: 512 if nreg == 5 else 256, at_least=20, scratch_free=False),
    # the plan audit: three waves per SIMD (built: 100 .. 146)
    Budget("planning_registers", "minsnap_audit.o", "plan-audit", ("minsnap_audit_kernel",), 168, at_least=4, scratch_free=False),
    # the plan demand: the audit's budget -- with sixteen cuboids 49 920 B of LDS, three workgroups per CU, hence three waves
    # per SIMD (built: 122 .. 136, no scratch memory)
    Budget("planning_registers", "minsnap_demand.o", "plan-demand", ("minsnap_demand_kernel",), 168, at_least=4),
    # the slowdown factors of the tilt and thrust limits: the audit's shape and budget, no LDS (built: 112 and 120 at 64 and 16 lanes
    # per mission, no scratch memory)
    Budget("planning_registers", "minsnap_need.o", "plan-need", ("minsnap_need_kernel",), 168, at_least=2),
    # the swept boxes: the audit's shape and budget, no LDS (built: 82 and 90 at 64 and 16 lanes per mission, 88 and 102
    # with a reach, no scratch memory)
    Budget("planning_registers", "minsnap_envelope.o", "plan-envelope", ("minsnap_envelope_kernel",), 168, at_least=4),
    # the solve with boundary derivatives, uniform and ragged: two waves per SIMD (built: 211 / 217)
    Budget("planning_registers", "minsnap_solve_bc.o", "boundary-solve", ("minsnap_solve_bc_kernel",), 256, extra=1),
    # plans from given durations, the snap cost, the duration optimisation's bookkeeping: loops over a mission's segments that keep
    # no per-segment arrays; at least four waves per SIMD (built: the cost kernel 64, the others 10 .. 40; two row-count variants)
    Budget("timeopt_kernels", "minsnap_timeopt.o", "time-optimisation",
           ("row_counts_t_kernel", "plan_t_commit_kernel", "minsnap_cost_kernel", "timeopt_expand_kernel", "timeopt_init_kernel",
            "timeopt_probe_kernel", "timeopt_direction_kernel", "timeopt_candidate_kernel", "timeopt_select_kernel"), 128, extra=1),
    # the fleet's separation audit: the pair kernel's 48 KB LDS tile admits three workgroups per CU, so three waves per SIMD; its
    # two coefficient sets are indexed by constants only (built: 164, the pre-pass 14, the merge 20)
    Budget("separation_kernels", "minsnap_separation.o", "separation",
           ("separation_prepass_kernel", "minsnap_separation_kernel", "separation_merge_kernel"), 168),
    # the audit's conflict list: the discovery and the measure keep the 48 KB tile (three workgroups per CU, <= 168); the
    # pre-pass, the counts (32 B for their scan) and the list run eight waves per SIMD (<= 64)
    Budget("conflict_kernels", "minsnap_conflicts.o", "conflict-list",
           ("conflict_prepass_kernel", "conflict_discover_kernel", "conflict_count_kernel", "conflict_list_kernel", "conflict_measure_kernel"),
           FROM_LDS),
    # start delays that clear the audit: the decision kernel's 48 KB tile plus 1 KB of granted starts, three workgroups per CU
    # (built: 145, the pre-pass 14)
    Budget("stagger_kernels", "minsnap_stagger.o", "stagger", ("stagger_prepass_kernel", "minsnap_stagger_kernel"), 168),
    # start delays as a leading hold segment: plain copies, eight waves per SIMD (built: 24 each)
    Budget("delay_kernels", "minsnap_delay.o", "delay", ("delay_counts_kernel", "minsnap_delay_kernel"), 64),
    # missions selected and reordered, priorities into a within-group order: two plain copies and a count over 2 KB LDS tiles
    # of keys, eight waves per SIMD (built: 24, 28 and 18)
    Budget("take_kernels", "minsnap_take.o", "take", ("take_counts_kernel", "minsnap_take_kernel", "fleet_order_kernel"), 64),
    # independent airspaces from the boxes: the link kernel's 13 KB tile of boxes and labels, eight waves per SIMD like the order
    # kernel it is shaped after (built: 40, the others 3 .. 6)
    Budget("airspace_kernels", "fleet_airspaces.o", "airspace",
           ("airspace_begin_kernel", "airspace_link_kernel", "airspace_jump_kernel", "airspace_info_kernel"), 64),
    # the separation the fleet flew, from a state log: the 48 KB tile like the plan audit's (built: 143, the merge 18)
    Budget("flown_separation_kernels", "flown_separation.o", "flown-separation", ("flown_separation_kernel", "flown_merge_kernel"), 168),
    # the conflict list of a flight: the discovery keeps the 48 KB tile (built: 114); the measure keeps 48 log values per lane
    # in flight and is launched for four waves per SIMD (`__launch_bounds__(256, 4)`; built: 112); the counts and the list of
    # conflict_csr.h run eight (built: 24 each, as in minsnap_conflicts.o)
    Budget("flown_conflict_kernels", "flown_conflicts.o", "flown-conflict-list",
           ("flown_discover_kernel", "conflict_count_kernel", "conflict_list_kernel", "flown_measure_kernel"),
           {"flown_discover_kernel": 168, "conflict_count_kernel": 64, "conflict_list_kernel": 64, "flown_measure_kernel": 128}),
    # the plan audit of a flight: the streaming kernel is launched for four waves per SIMD (`__launch_bounds__(256, 4)`: one
    # workgroup per SIMD keeps 26 row loads per wavefront in flight; built: 82, the merge 44)
    Budget("flown_audit_kernels", "flown_audit.o", "flown-audit", ("flown_audit_kernel", "flown_audit_merge_kernel"), 128),
    # offset layers that clear the audit, and the offset transform (built: the decision kernel 50192 B of LDS -- the 48 KB tile,
    # 1 KB of granted layers, two words -- hence three workgroups per CU and <= 168, at 137; the pre-pass and the transform no
    # LDS, hence eight and <= 64, at 14 and 21)
    Budget("layer_kernels", "minsnap_layer.o", "layer", ("layer_prepass_kernel", "minsnap_layer_kernel", "minsnap_shift_kernel"), FROM_LDS),
    # the same search refusing layers that put a mission into a cuboid, the two instantiations with cuboids (built: 50976 B of
    # LDS -- 768 B of cuboids, two more words -- hence still three workgroups per CU, at 142; the pre-pass 14)
    Budget("layer_obs_kernels", "minsnap_layer_obs.o", "obstacle-aware layer", ("layer_prepass_kernel", "minsnap_layer_kernel"), FROM_LDS),
    # the two searches for groups of any size (csrc/fleet_wide.h): the block search is the decision kernel above and keeps its three
    # workgroups per CU; the seed kernel holds the 48 KB tile and two words, hence three as well and <= 168 (built: stagger 142
    # and 127, layer 151 and 144 -- the seed first; the pre-passes 14)
    Budget("stagger_wide_kernels", "minsnap_stagger_wide.o", "wide stagger",
           ("stagger_prepass_kernel", "wide_stagger_seed_kernel", "wide_stagger_kernel"), FROM_LDS),
    Budget("layer_wide_kernels", "minsnap_layer_wide.o", "wide layer", ("layer_prepass_kernel", "wide_layer_seed_kernel", "wide_layer_kernel"),
           FROM_LDS),
    # the same searches against traffic that never moves (csrc/fleet_against.h): the two kernels above, and the traffic's seed
    # kernel, which holds the 48 KB tile and two words like the block seed, hence three workgroups per CU and <= 168; the two
    # pre-passes and the carry (32 B) run eight waves per SIMD
    Budget("stagger_against_kernels", "minsnap_stagger_against.o", "stagger against traffic",
           ("stagger_prepass_kernel", "traffic_prepass_kernel", "traffic_carry_kernel", "against_stagger_seed_kernel", "wide_stagger_seed_kernel",
            "wide_stagger_kernel"), FROM_LDS),
    Budget("layer_against_kernels", "minsnap_layer_against.o", "layer against traffic",
           ("layer_prepass_kernel", "traffic_prepass_kernel", "traffic_carry_kernel", "against_layer_seed_kernel", "wide_layer_seed_kernel",
            "wide_layer_kernel"), FROM_LDS),
    # the cross audit: the plan audit's pair kernel with its partners taken from the traffic, the 48 KB tile, three workgroups per CU
    Budget("separation_against_kernels", "minsnap_separation_against.o", "cross-audit",
           ("against_prepass_kernel", "separation_against_kernel", "against_merge_kernel"), FROM_LDS),
    # the cross audit's conflict list: the discovery is the cross audit's loop nest keeping bits only, the measure walks one mission of
    # either plan; both keep the 48 KB tile (three workgroups per CU, <= 168); the pre-pass, the counts and the list of conflict_csr.h
    # run eight waves per SIMD (<= 64)
    Budget("cross_conflict_kernels", "minsnap_conflicts_against.o", "cross-conflict-list",
           ("conflict_against_prepass_kernel", "conflict_against_discover_kernel", "conflict_count_kernel", "conflict_list_kernel",
            "conflict_against_measure_kernel"), FROM_LDS),
)
DECISION_KERNELS =("minsnap_layer_kernel", "wide_layer_kernel", "wide_stagger_kernel")      # FROM_LDS: these keep three workgroups per CU
COUNTED = ("rollout_registers", "planning_registers")      # `run_all` reports these as a number of kernels, the others as {kernel: VGPRs}

# The object files that have no budget, and why not.
UNBUDGETED = {
    "control_probe.o": "the single-tick kernels of the host-owned loops, the heading self-check and measurement probes: off the flagship path, never given a limit",
    "minsnap_first_yaw.o": "one kernel, a mission's first heading without rows: one short pass per plan, never given a limit",
    "minsnap_obstacles.o": "the obstacle loop's scan, count and scatter: never given a limit",
    "minsnap_retime.o": "the retiming factors and a fill: never given a limit",
    "minsnap_sample.o": "the sampler before the streaming one and the yaw scan: kept for small batches, never given a limit",
    "minsnap_solve.o": "row offsets, row counts, the plan commit and the first solve kernel: bookkeeping, never given a limit",
    "rrt_star.o": "one wavefront per problem with the tree in LDS: its occupancy is set by LDS, never given a register limit",
    "uavac_api.o": "host code only: the context and the C ABI's entry points",
    "uavac_comm.o": "host code only: the multi-GPU gather over RCCL",
}


def vgpr_limit(rule, k: Kernel):
    """The most vector registers the kernel `k` may take under the limit rule of a BUDGETS row, or a str that says why it has none."""
    if callable(rule):
        return rule(*template_args(k.name))
    if isinstance(rule, dict):
        mine = [limit for name, limit in rule.items() if name in k.name]
        return min(mine) if mine else "no limit listed for it"
    if rule is FROM_LDS:
        lds = k.group_segment_fixed_size
        waves = min(8, LDS_BYTES_PER_CU // lds) if lds else 8
        if any(name in k.name for name in DECISION_KERNELS) and waves < 3:
            return f"{lds} bytes of LDS: fewer than three workgroups per CU"
        return VGPRS_AT_WAVES_PER_SIMD.get(waves, 0)           # (a workgroup that does not fit a CU at all: limit 0)
    return rule


def check_budget(row: Budget, kernels):
    """Apply one row of BUDGETS to the kernel records of its object file(s).  Raises RuntimeError naming every kernel outside
    the row; returns the records the row speaks of."""
    mine = [k for k in kernels if any(name in k.name for name in row.kernels)] if row.at_least else list(kernels)
    bad = []
    for k in mine:
        limit = vgpr_limit(row.limit, k)
        if isinstance(limit, str):
            bad.append((k.name[:90], limit))
        elif k.vgpr_count > limit or k.vgpr_spill_count:
            bad.append((k.name[:90], k.vgpr_count, k.vgpr_spill_count, limit))
        if row.scratch_free and k.private_segment_fixed_size:
            bad.append((k.name[:90], f"{k.private_segment_fixed_size} private-segment bytes"))
    missing = [] if row.at_least else [name for name in row.kernels if not any(name in k.name for k in mine)]
    short = len(mine) < row.at_least if row.at_least else len(mine) != len(row.kernels) + row.extra
    if bad or missing or short:
        raise RuntimeError(f"{row.noun} kernels outside their budgets (name, VGPRs, spills, limit): {bad}; missing: {missing}; {len(mine)} kernels "
                           f"found in {row.obj} where {'at least ' + str(row.at_least) if row.at_least else len(row.kernels) + row.extra} of "
                           f"{', '.join(row.kernels)} belong (compiler: {compiler_version()})")
    return mine


def check_budgets(key: str):
    """Every row of BUDGETS that reports under `key`, on the object files under build/.  Raises RuntimeError like `check_budget`;
    returns the [Kernel] the rows speak of, None when an object file cannot be read."""
    found = []
    for row in (r for r in BUDGETS if r.key == key):
        read = [read_object(os.path.join(PKG, "build", o)) for o in row.obj.split()]
        if None in read:
            return None
        found += check_budget(row, [k for co in read for k in co["kernels"]])
    return found


def vgprs(kernels):
    """{kernel name: vector registers} of [Kernel], the form in which `run_all` reports a budget; None stays None."""
    return None if kernels is None else {k.name: k.vgpr_count for k in kernels}


def _triples(kernels):
    """[(kernel name, vector registers, spills)] of [Kernel]; None stays None."""
    return None if kernels is None else [k[:3] for k in kernels]


# The names by which the host tests (tests/test_*_host.py) and DESIGN.md section 3 know the rows: one-line lookups, nothing else.
def check_rollout_registers(): return _triples(check_budgets("rollout_registers"))                      # noqa: E704
def check_planning_registers(): return _triples(check_budgets("planning_registers"))                    # noqa: E704
def check_timeopt_kernels(): return vgprs(check_budgets("timeopt_kernels"))                             # noqa: E704
def check_separation_kernels(): return vgprs(check_budgets("separation_kernels"))                       # noqa: E704
def check_conflict_kernels(): return vgprs(check_budgets("conflict_kernels"))                           # noqa: E704
def check_stagger_kernels(): return vgprs(check_budgets("stagger_kernels"))                             # noqa: E704
def check_delay_kernels(): return vgprs(check_budgets("delay_kernels"))                                 # noqa: E704
def check_take_kernels(): return vgprs(check_budgets("take_kernels"))                                   # noqa: E704
def check_airspace_kernels(): return vgprs(check_budgets("airspace_kernels"))                           # noqa: E704
def check_flown_separation_kernels(): return vgprs(check_budgets("flown_separation_kernels"))           # noqa: E704
def check_flown_conflict_kernels(): return vgprs(check_budgets("flown_conflict_kernels"))               # noqa: E704
def check_flown_audit_kernels(): return vgprs(check_budgets("flown_audit_kernels"))                     # noqa: E704
def check_layer_kernels(): return vgprs(check_budgets("layer_kernels"))                                 # noqa: E704
def check_layer_obs_kernels(): return vgprs(check_budgets("layer_obs_kernels"))                         # noqa: E704
def check_stagger_wide_kernels(): return vgprs(check_budgets("stagger_wide_kernels"))                   # noqa: E704
def check_layer_wide_kernels(): return vgprs(check_budgets("layer_wide_kernels"))                       # noqa: E704
def check_stagger_against_kernels(): return vgprs(check_budgets("stagger_against_kernels"))             # noqa: E704
def check_layer_against_kernels(): return vgprs(check_budgets("layer_against_kernels"))                 # noqa: E704
def check_separation_against_kernels(): return vgprs(check_budgets("separation_against_kernels"))       # noqa: E704
def check_cross_conflict_kernels(): return vgprs(check_budgets("cross_conflict_kernels"))               # noqa: E704
TIMEOPT_KERNELS = next(row.kernels for row in BUDGETS if row.key == "timeopt_kernels")
FLOWN_CONFLICT_KERNELS = next(row.kernels for row in BUDGETS if row.key == "flown_conflict_kernels")


def check_inventory():
    """Every object file under build/ stands in BUDGETS or in UNBUDGETED, and every one listed there was built.  Raises
    RuntimeError otherwise; returns their number, None without a build directory."""
    build = os.path.join(PKG, "build")
    if not os.path.isdir(build):
        return None
    have = {f for f in os.listdir(build) if f.endswith(".o")}
    listed = {o for row in BUDGETS for o in row.obj.split()} | set(UNBUDGETED)
    if have != listed:
        raise RuntimeError(f"object files under build/ that neither BUDGETS nor UNBUDGETED of uav_ac/_buildcheck.py lists: {sorted(have - listed)}; "
                           f"listed there but not built: {sorted(listed - have)}")
    return len(have)


# ------------------------------------------------------------------------------------------------ the prefetches
def _successors(ins):
    """Successor indices of every instruction of a kernel (fall-through and branch targets); raises on a branch the disassembly
    gives no target for."""
    index = {x.addr: i for i, x in enumerate(ins) if getattr(x, "addr", None) is not None}
    succ = []
    for i, x in enumerate(ins):
        if x.startswith("s_endpgm"):
            succ.append(())
        elif x.startswith(_INDIRECT):
            raise RuntimeError(f"indirect control flow ('{x}'): the check cannot follow it")
        elif x.startswith(_BRANCH):
            t = index.get(getattr(x, "target", None))
            if t is None:
                raise RuntimeError(f"branch '{x}' without a known target")
            succ.append((t,) if x.startswith("s_branch") else (i + 1, t))
        else:
            succ.append((i + 1,))
    return [tuple(j for j in s if j < len(ins)) for s in succ]


def _vregs(text: str):
    regs = set()
    for lo, hi, one in re.findall(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", text):
        regs.update(range(int(lo), int(hi) + 1) if lo else (int(one),))
    return regs


_ROW_LOAD = re.compile(r"global_load_dwordx4 v\[(\d+):(\d+)\], (v\[\d+:\d+\]), off(?: offset:(\d+))?$")


def check_row_prefetch(obj: str = None, scored: bool = False):
    """The row-fed rollout kernels prefetch a trajectory row with loads the compiler does not know to be in flight (inline asm,
    control_rollout.hip row_issue / row_wait).  That is only right while the loads land in the very registers row_wait() hands
    on: for every row-fed variant, (1) every group of five row loads writes the same twenty registers, (2) no other instruction
    reads or writes one of them at a point that a row load can reach without passing an `s_waitcnt vmcnt(0)` -- decided on the
    kernel's CONTROL-FLOW GRAPH (branch targets from the disassembly; a forward may-analysis "row loads possibly in flight"), not
    on the linear layout: a wait that sits in a block the executed path branches over proves nothing (round-5 advice).  Code
    that no row load reaches (ahead of the first one) is free to use the registers.  Raises RuntimeError otherwise; returns the
    number of variants checked, None when the object file cannot be read.  `scored`: the same check on the scored twins
    (scored_control_rollout_kernel, 8 row-fed variants) instead of the unscored kernels (16)."""
    kernels = _disassemble_cfg(obj or os.path.join(PKG, "build", "control_rollout.o"))
    if kernels is None:
        return None
    checked, bad = 0, []
    for name, ins in kernels.items():
        if "control_rollout_kernel" not in name or ("scored_control_rollout_kernel" in name) != scored:
            continue
        groups, i = [], 0
        while i + 4 < len(ins):
            ms = [_ROW_LOAD.match(x) for x in ins[i:i + 5]]
            if all(ms) and [int(m.group(4) or 0) for m in ms] == [0, 16, 32, 48, 64] and len({m.group(3) for m in ms}) == 1:
                groups.append((i, frozenset(r for m in ms for r in range(int(m.group(1)), int(m.group(2)) + 1))))
                i += 5
            else:
                i += 1
        if template_args(name)[5]:                 # POLY (its coefficient loads look alike; the compiler issues and waits for those itself)
            continue
        checked += 1
        if len(groups) != 2 or len({g for _, g in groups}) != 1 or len(groups[0][1]) != 20:
            bad.append((name[:90], f"row-load groups: {[(i, sorted(g)[:1], len(g)) for i, g in groups]}"))
            continue
        dest, inside = groups[0][1], {j for i, _ in groups for j in range(i, i + 5)}
        try:
            succ = _successors(ins)
        except RuntimeError as exc:
            bad.append((name[:90], str(exc)))
            continue
        # in_flight[j]: some path reaches instruction j with a row load issued and no vmcnt(0) wait since
        in_flight = [False] * (len(ins) + 1)
        work = []
        for j in inside:
            for k in succ[j]:
                if not in_flight[k]:
                    in_flight[k] = True
                    work.append(k)
        while work:
            j = work.pop()
            if j >= len(ins) or j in inside or re.match(r"s_waitcnt vmcnt\(0\)", ins[j]):
                continue                            # (a row load's own successors are seeded above; a wait ends the flight)
            for k in succ[j]:
                if not in_flight[k]:
                    in_flight[k] = True
                    work.append(k)
        for j, x in enumerate(ins):
            if j not in inside and in_flight[j] and (_vregs(x) & dest):
                bad.append((name[:90], f"'{x}' touches a row register while the row loads may be in flight"))
                break
    if bad or checked < (8 if scored else 16):
        raise RuntimeError(f"row prefetch of the row-fed {'scored ' if scored else ''}rollout kernels: {checked} variants checked; {bad} (compiler: {compiler_version()})")
    return checked


_LDS_LOAD = re.compile(r"ds_read_b128 v\[(\d+):(\d+)\], (v\d+)(?: offset:(\d+))?$")


def check_heading_prefetch(obj: str = None):
    """The streaming sampler fetches the heading polynomial's twenty coefficients from LDS with ten `ds_read_b128` the compiler does not
    know to be in flight (minsnap_yaw.h, HeadingFromLds::begin / ready) while the division runs.  Same question as for the rollout's row
    prefetch, same answer: in every sampler variant, between each group of ten such loads and the next `s_waitcnt ... lgkmcnt(0)` no
    instruction touches a destination register and no branch intervenes.  Raises RuntimeError otherwise; returns the number of groups
    checked, None when the object file cannot be read."""
    kernels = _disassemble_cfg(obj or os.path.join(PKG, "build", "minsnap_sample_stream.o"))
    if kernels is None:
        return None
    groups, bad = 0, []
    for name, ins in kernels.items():
        if "minsnap_sample_stream_kernel" not in name:
            continue
        i = 0
        while i + 9 < len(ins):
            ms = [_LDS_LOAD.match(x) for x in ins[i:i + 10]]
            if not (all(ms) and [int(m.group(4) or 0) for m in ms] == list(range(0, 160, 16)) and len({m.group(3) for m in ms}) == 1):
                i += 1
                continue
            dest = {r for m in ms for r in range(int(m.group(1)), int(m.group(2)) + 1)}
            groups += 1
            j = i + 10
            while j < len(ins) and not re.match(r"s_waitcnt .*lgkmcnt\(0\)", ins[j]):
                if _vregs(ins[j]) & dest or ins[j].startswith(("s_cbranch", "s_branch", "s_endpgm")):
                    bad.append((name[:80], f"'{ins[j]}' between the coefficient loads and their wait"))
                    break
                j += 1
            i += 10
    if bad or groups < 20:
        raise RuntimeError(f"heading prefetch of the streaming sampler: {groups} load groups checked; {bad} (compiler: {compiler_version()})")
    return groups


def check_no_diagnostics(lib_path: str = None):
    """The shipped library exports no diagnostic entry point (`uavac_diag_*`): those exist only in tools/diag builds."""
    lib_path = lib_path or os.path.join(PKG, "lib", "libuavac.so")
    readelf = os.path.join(LLVM_BIN, "llvm-readelf")
    if not (os.path.exists(lib_path) and os.path.exists(readelf)):
        return None
    syms = subprocess.run([readelf, "--dyn-syms", "-W", lib_path], check=True, capture_output=True, text=True).stdout
    diag = [line.split()[-1] for line in syms.splitlines() if "diag" in line.lower() and " UND " not in line]
    if diag:
        raise RuntimeError(f"{lib_path} exports diagnostic symbols {diag}: it was built with a UAVAC_DIAG_* define")
    return True


def library_sha256(lib_path: str = None) -> str:
    import hashlib
    with open(lib_path or os.path.join(PKG, "lib", "libuavac.so"), "rb") as fh:
        return hashlib.sha256(fh.read()).hexdigest()


STAMP = os.path.join(PKG, "lib", "libuavac.buildcheck.json")


def run_all(verbose: bool = False, write_stamp: bool = True) -> dict:
    """EVERY build check, for every place that builds the library (`__graft_entry__.build()`, the autobuild of
    `uav_ac._native.lib()`, `make`): every object file under build/ listed, every row of BUDGETS, then the row prefetch and the
    sampler's heading prefetch in the disassembly and no diagnostic symbol.  A check that cannot run (no object files, no LLVM
    tools) is a FAILURE here: the output-only asm operands of row_issue / HeadingFromLds are only as safe as these checks, so a
    build they did not see must not pass for one they did.  Raises RuntimeError; on success writes
    lib/libuavac.buildcheck.json -- the library's sha256, its uavac_build_info() and the compiler the checks saw -- which
    travels with the library (tests/test_gpu_round6.py compares it with the library the GPU process loaded)."""
    import ctypes
    import json

    def ran(key, r, said):
        if r is None:
            raise RuntimeError(f"build check '{key}' could not run (object files under {PKG}/build or the LLVM tools under {LLVM_BIN} are "
                               "missing): the library would ship unchecked")
        if verbose:
            print(f"build: {said(r)}")
        return r

    ran("inventory", check_inventory(), lambda r: f"{r} object files, each with a budget or a reason to have none")
    budgets = {}
    for key in dict.fromkeys(row.key for row in BUDGETS):
        rows = [row for row in BUDGETS if row.key == key]
        found = ran(key, check_budgets(key), lambda r: f"{len(r)} {' / '.join(row.noun for row in rows)} kernels, at most {max(k.vgpr_count for k in r)} "
                    f"VGPRs, no spills{', no scratch memory' if all(row.scratch_free for row in rows) else ''}")
        budgets[key] = len(found) if key in COUNTED else vgprs(found)
    result = {"rollout_registers": budgets.pop("rollout_registers"),
              "row_prefetch": ran("row_prefetch", check_row_prefetch(),
                                  lambda r: f"row prefetch of {r} row-fed rollout kernels verified on the control-flow graph of the disassembly"),
              "scored_row_prefetch": ran("scored_row_prefetch", check_row_prefetch(scored=True),
                                         lambda r: f"row prefetch of {r} row-fed scored rollout kernels verified the same way"),
              "heading_prefetch": ran("heading_prefetch", check_heading_prefetch(),
                                      lambda r: f"{r} coefficient prefetches of the streaming sampler verified in the disassembly"),
              "no_diagnostics": ran("no_diagnostics", check_no_diagnostics(), lambda r: "no diagnostic symbol exported"),
              **budgets}
    lib_path = os.path.join(PKG, "lib", "libuavac.so")
    fn = ctypes.CDLL(lib_path).uavac_build_info
    fn.restype = ctypes.c_char_p
    stamp = {"library_sha256": library_sha256(lib_path), "build_info": fn().decode(), "checked_with": compiler_version(), "checks": result}
    if write_stamp:
        tmp = STAMP + f".tmp.{os.getpid()}"
        with open(tmp, "w") as fh:
            json.dump(stamp, fh, indent=1)
        os.replace(tmp, STAMP)
    return stamp


def read_stamp():
    """The record `run_all` left beside the library, or None."""
    import json
    if not os.path.exists(STAMP):
        return None
    with open(STAMP) as fh:
        return json.load(fh)


def compiler_version() -> str:
    try:
        out = subprocess.run(["/opt/rocm/bin/hipcc", "--version"], capture_output=True, text=True, timeout=60).stdout
        return " / ".join(line.strip() for line in out.splitlines()[:2])
    except Exception:                                        # pragma: no cover
        return "unknown"


if __name__ == "__main__":                                   # `make` (the Makefile's default target) runs this after linking
    import sys
    try:
        _s = run_all(verbose=True)
    except Exception as exc:
        print(f"build checks FAILED: {exc}", file=sys.stderr)
        sys.exit(1)
    print(f"build: checks passed for library {_s['library_sha256'][:16]}")
