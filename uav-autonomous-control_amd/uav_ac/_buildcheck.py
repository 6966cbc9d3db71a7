"""Build-time check of the rollout kernels' register budget (used by __graft_entry__.build() and by the CPU tests).

Every variant of `control_rollout_kernel` must fit TWO wavefronts on a SIMD: at most 256 of its 512 vector registers, no
vector-register spills.  A logged launch puts a compute and a store wave of the same kernel on every SIMD; at 258 registers
(a 6-register 'optimisation' tried in round 3) the bench launch took 1.96 ms instead of 1.27 ms -- a cliff that no functional
test sees and that a toolchain bump can cross silently.  Read from the code object inside build/control_rollout.o."""
import os
import re
import shutil
import subprocess
import tempfile

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM_BIN = "/opt/rocm/lib/llvm/bin"
VGPR_LIMIT = 256


def _kernel_notes(obj: str):
    """The metadata notes of the gfx950 code object inside an object file, or None when the object file or the LLVM tools are not
    there (a library that was built elsewhere)."""
    objdump, readelf = os.path.join(LLVM_BIN, "llvm-objdump"), os.path.join(LLVM_BIN, "llvm-readelf")
    if not (os.path.exists(obj) and os.path.exists(objdump) and os.path.exists(readelf)):
        return None
    tmp = tempfile.mkdtemp()
    try:
        shutil.copy(obj, os.path.join(tmp, "o.o"))
        subprocess.run([objdump, "--offloading", "o.o"], cwd=tmp, check=True, capture_output=True)
        co = [f for f in os.listdir(tmp) if "gfx950" in f][0]
        notes = subprocess.run([readelf, "--notes", os.path.join(tmp, co)], check=True, capture_output=True, text=True).stdout
    finally:
        shutil.rmtree(tmp)
    return notes


def kernel_register_counts(obj: str, kernel: str):
    """[(kernel name, vgpr_count, vgpr_spill_count)] of every kernel of the object file whose name contains `kernel`, or None
    when the object file or the LLVM tools are not there (a library that was built elsewhere)."""
    notes = _kernel_notes(obj)
    if notes is None:
        return None
    found = re.findall(r"\.name:\s+(\S*" + re.escape(kernel) + r"\S*).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", notes, flags=re.S)
    return [(n, int(v), int(s)) for n, v, s in found]


def kernel_private_bytes(obj: str, kernel: str):
    """[(kernel name, private_segment_fixed_size)] -- the scratch memory per lane, which is 0 for a kernel that lives in registers --
    of every kernel of the object file whose name contains `kernel`; None like `kernel_register_counts`."""
    notes = _kernel_notes(obj)
    if notes is None:
        return None
    # (the metadata lists a kernel's keys in alphabetical order: .name comes before .private_segment_fixed_size)
    found = re.findall(r"\.name:\s+(\S*" + re.escape(kernel) + r"\S*)\s.*?\.private_segment_fixed_size:\s+(\d+)", notes, flags=re.S)
    return [(n, int(v)) for n, v in found]


def rollout_register_counts(obj: str = None):
    """The same for every control_rollout_kernel variant."""
    return kernel_register_counts(obj or os.path.join(PKG, "build", "control_rollout.o"), "control_rollout_kernel")


def check_planning_registers():
    """The planning kernels' budgets: the chunk-streaming sampler without jerk / snap runs six waves per SIMD (<= 80 vector
    registers; with jerk / snap four: <= 128), the solve one or two (the variant that keeps five knots in registers: <= 512, the
    others <= 256), the solve with boundary derivatives two (<= 256, and no scratch memory at all: zero private-segment bytes), the
    plan audit three (<= 168); none may spill (a spill in the sampler showed as 3 % more HBM writes and no other symptom, NOTES R4-2).
    Returns the counts, None when they cannot be read."""
    s = kernel_register_counts(os.path.join(PKG, "build", "minsnap_sample_stream.o"), "minsnap_sample_stream_kernel")
    k = kernel_register_counts(os.path.join(PKG, "build", "minsnap_solve_bt.o"), "minsnap_solve_bt_kernel")
    k2 = kernel_register_counts(os.path.join(PKG, "build", "minsnap_solve_tw.o"), "minsnap_solve_tw_kernel")
    a = kernel_register_counts(os.path.join(PKG, "build", "minsnap_audit.o"), "minsnap_audit_kernel")
    bc_obj = os.path.join(PKG, "build", "minsnap_solve_bc.o")
    kb, pb = kernel_register_counts(bc_obj, "minsnap_solve_bc_kernel"), kernel_private_bytes(bc_obj, "minsnap_solve_bc_kernel")
    if s is None or k is None or k2 is None or a is None or kb is None or pb is None:
        return None
    k = k + k2                                        # (the two-ended solve: same budgets, same naming of the last template argument)
    bad = []
    for n, v, sp in s:
        args = re.search(r"minsnap_sample_stream_kernelILi(\d+)ELb([01])ELb([01])ELb([01])E", n)
        waves, derivs = int(args.group(1)), args.group(3) == "1"
        limit = 128 if (derivs or waves == 16) else 80
        if v > limit or sp:
            bad.append((n[:70], v, sp, limit))
    for n, v, sp in k:
        limit = 512 if n.rstrip("E").endswith("Li5") or "Li5EE" in n else 256
        if v > limit or sp:
            bad.append((n[:70], v, sp, limit))
    for n, v, sp in a:                                # the plan audit: three waves per SIMD (built: 100 .. 146 registers)
        if v > 168 or sp:
            bad.append((n[:70], v, sp, 168))
    for n, v, sp in kb:                               # the solve with boundary derivatives: two waves per SIMD (built: 211 / 217 registers)
        if v > 256 or sp:
            bad.append((n[:70], v, sp, 256))
    for n, priv in pb:
        if priv:
            bad.append((n[:70], f"{priv} private-segment bytes", 0, 0))
    if len(s) < 20 or len(k) < 20 or len(a) < 4 or len(kb) != 2 or len(pb) != 2 or bad:
        raise RuntimeError(f"planning kernels outside their register budgets (name, VGPRs, spills, limit): {bad}; {len(s)} sampler, "
                           f"{len(k)} solve, {len(kb)} boundary-solve and {len(a)} audit variants found (compiler: {compiler_version()})")
    return s + k + a + kb


LDS_BYTES_PER_CU = 160 * 1024
VGPRS_AT_WAVES_PER_SIMD = {8: 64, 7: 72, 6: 80, 5: 96, 4: 128, 3: 168, 2: 256, 1: 512}     # the largest allocation that still runs that many


def kernel_lds_bytes(obj: str, kernel: str):
    """[(kernel name, group_segment_fixed_size)] -- the static LDS of a workgroup -- of every kernel of the object file whose name
    contains `kernel`; None like `kernel_register_counts`."""
    notes = _kernel_notes(obj)
    if notes is None:
        return None
    # (the metadata lists a kernel's keys in alphabetical order: .group_segment_fixed_size comes before .name)
    found = re.findall(r"\.group_segment_fixed_size:\s+(\d+)(?:(?!\.group_segment_fixed_size:).)*?\.name:\s+(\S*" + re.escape(kernel) + r"\S*)",
                       notes, flags=re.S)
    return [(n, int(v)) for v, n in found]


def _check_object(obj_name: str, kernels, what: str, vgpr_limit=None, extra_kernels: int = 0):
    """The budget of the kernels of one object file under build/: every kernel of `kernels` must be there and the object must hold
    exactly len(kernels) + `extra_kernels` of them (further instantiations of a listed kernel), none may spill or use scratch memory at
    all (zero private-segment bytes), and none may need more than `vgpr_limit` vector registers.  `vgpr_limit` None: the limit of each
    kernel follows from the LDS it ends up with -- workgroups of four waves, so min(8, 160 KiB // LDS) workgroups per CU are as many
    waves per SIMD, and the kernel must fit the allocation that still runs that many --, and a decision kernel of the layer search must
    keep three workgroups per CU.  Returns {kernel: VGPRs}, None when the counts cannot be read."""
    obj = os.path.join(PKG, "build", obj_name)
    regs, priv = kernel_register_counts(obj, "_kernel"), kernel_private_bytes(obj, "_kernel")
    lds = kernel_lds_bytes(obj, "_kernel") if vgpr_limit is None else []
    if regs is None or priv is None or lds is None:
        return None
    lds = dict(lds)
    bad = [(n[:70], f"{p} private-segment bytes", 0, 0) for n, p in priv if p]
    for n, v, sp in regs:
        limit = vgpr_limit
        if limit is None:
            if n not in lds:
                bad.append((n[:70], "no LDS size found", 0, 0))
                continue
            waves = min(8, LDS_BYTES_PER_CU // lds[n]) if lds[n] else 8
            limit = VGPRS_AT_WAVES_PER_SIMD.get(waves, 0)      # (a workgroup that does not fit a CU at all: limit 0)
            if "minsnap_layer_kernel" in n and waves < 3:
                bad.append((n[:70], f"{lds[n]} bytes of LDS: fewer than three workgroups per CU", 0, 0))
        if v > limit or sp:
            bad.append((n[:70], v, sp, limit))
    missing = [k for k in kernels if not any(k in n for n, _, _ in regs)]
    if bad or missing or len(regs) != len(kernels) + extra_kernels or len(priv) != len(regs):
        raise RuntimeError(f"{what} kernels outside their budgets (name, VGPRs, spills, limit): {bad}; missing: {missing}; "
                           f"{len(regs)} kernels found (compiler: {compiler_version()})")
    return {n: v for n, v, _ in regs}


TIMEOPT_KERNELS = ("row_counts_t_kernel", "plan_t_commit_kernel", "minsnap_cost_kernel", "timeopt_expand_kernel", "timeopt_init_kernel",
                   "timeopt_probe_kernel", "timeopt_direction_kernel", "timeopt_candidate_kernel", "timeopt_select_kernel")


def check_timeopt_kernels():
    """The kernels of csrc/minsnap_timeopt.hip (plans from given durations, the snap cost, the bookkeeping of the duration
    optimisation): `_check_object` -- their loops over a mission's segments keep no per-segment arrays -- with all of them at least
    four waves per SIMD (<= 128 vector registers; built: the cost kernel 64, the others 10 .. 40).  Returns {kernel: VGPRs} (the two
    row-count variants under their mangled names), None when the counts cannot be read."""
    return _check_object("minsnap_timeopt.o", TIMEOPT_KERNELS, "time-optimisation", vgpr_limit=128, extra_kernels=1)


SEPARATION_KERNELS = ("separation_prepass_kernel", "minsnap_separation_kernel", "separation_merge_kernel")


def check_separation_kernels():
    """The kernels of csrc/minsnap_separation.hip (the fleet's separation audit): `_check_object` -- the two coefficient sets of the pair
    kernel are indexed by constants only --, and the pair kernel, whose 48 KB LDS tile admits three workgroups per CU, must run three
    waves per SIMD (<= 168 vector registers; built: 164, the pre-pass 14, the merge 20).  Returns {kernel: VGPRs}, None when the
    counts cannot be read."""
    return _check_object("minsnap_separation.o", SEPARATION_KERNELS, "separation", vgpr_limit=168)


CONFLICT_KERNELS = ("conflict_prepass_kernel", "conflict_discover_kernel", "conflict_count_kernel", "conflict_list_kernel",
                    "conflict_measure_kernel")


def check_conflict_kernels():
    """The kernels of csrc/minsnap_conflicts.hip (the separation audit's conflict list): `_check_object` -- the coefficient sets of the
    discovery and of the measure are indexed by constants only -- with the register limit of each from the LDS it ends up with: the
    discovery and the measure keep the audit's 48 KB tile, hence three workgroups per CU and <= 168; the pre-pass, the counts (32 B for
    its scan) and the list run eight waves per SIMD and <= 64.  Returns {kernel: VGPRs}, None when the counts cannot be read."""
    return _check_object("minsnap_conflicts.o", CONFLICT_KERNELS, "conflict-list")


STAGGER_KERNELS = ("stagger_prepass_kernel", "minsnap_stagger_kernel")


def check_stagger_kernels():
    """The kernels of csrc/minsnap_stagger.hip (start delays that clear the separation audit): `_check_object` -- the two coefficient
    sets of the decision kernel are indexed by constants only --, and the decision kernel, whose 48 KB LDS tile plus 1 KB of granted
    starts admits three workgroups per CU, must run three waves per SIMD (<= 168 vector registers; built: 145, the pre-pass 14).
    Returns {kernel: VGPRs}, None when the counts cannot be read."""
    return _check_object("minsnap_stagger.o", STAGGER_KERNELS, "stagger", vgpr_limit=168)


FLOWN_SEPARATION_KERNELS = ("flown_separation_kernel", "flown_merge_kernel")


def check_flown_separation_kernels():
    """The kernels of csrc/flown_separation.hip (the separation the fleet flew, from a state log): `_check_object`, and the pair kernel,
    whose 48 KB LDS tile admits three workgroups per CU like the plan audit's, must run three waves per SIMD (<= 168 vector registers;
    built: 143, the merge 18).  Returns {kernel: VGPRs}, None when the counts cannot be read."""
    return _check_object("flown_separation.o", FLOWN_SEPARATION_KERNELS, "flown-separation", vgpr_limit=168)


FLOWN_CONFLICT_KERNELS = ("flown_discover_kernel", "conflict_count_kernel", "conflict_list_kernel", "flown_measure_kernel")
FLOWN_CONFLICT_LIMITS = {"flown_discover_kernel": 168, "conflict_count_kernel": 64, "conflict_list_kernel": 64, "flown_measure_kernel": 128}


def check_flown_conflict_kernels():
    """The kernels of csrc/flown_conflicts.hip (the conflict list of a flight, from a state log): `_check_object`, and each kernel
    inside its own limit: the discovery, whose 48 KB LDS tile admits three workgroups per CU like `flown_separation_kernel`'s, must
    run three waves per SIMD (<= 168 vector registers; built: 114); the measure keeps 48 log values per lane in flight and is
    launched for four waves per SIMD (`__launch_bounds__(256, 4)`: <= 128; built: 112); the counts and the list of conflict_csr.h run
    eight (<= 64; built: 24 each, as in minsnap_conflicts.o).  Returns {kernel: VGPRs}, None when the counts cannot be read."""
    regs = _check_object("flown_conflicts.o", FLOWN_CONFLICT_KERNELS, "flown-conflict-list", vgpr_limit=168)
    if regs is None:
        return None
    over = [(n[:70], v, limit) for k, limit in FLOWN_CONFLICT_LIMITS.items() for n, v in regs.items() if k in n and v > limit]
    if over:
        raise RuntimeError(f"flown-conflict-list kernels outside their budgets (name, VGPRs, limit): {over} (compiler: {compiler_version()})")
    return regs


FLOWN_AUDIT_KERNELS = ("flown_audit_kernel", "flown_audit_merge_kernel")


def check_flown_audit_kernels():
    """The kernels of csrc/flown_audit.hip (the plan audit of a flight, from a state log): `_check_object`, and the streaming kernel,
    which is launched for four waves per SIMD (`__launch_bounds__(256, 4)`: one workgroup per SIMD keeps 26 row loads per wavefront
    in flight), must fit that (<= 128 vector registers; built: 82, the merge 44).  Returns {kernel: VGPRs}, None when the counts
    cannot be read."""
    return _check_object("flown_audit.o", FLOWN_AUDIT_KERNELS, "flown-audit", vgpr_limit=128)


DELAY_KERNELS = ("delay_counts_kernel", "minsnap_delay_kernel")


def check_delay_kernels():
    """The kernels of csrc/minsnap_delay.hip (start delays as a leading hold segment of the plan): `_check_object`; both are plain
    copies that run at least eight waves per SIMD (<= 64 vector registers; built: 24 each).  Returns {kernel: VGPRs}, None when the
    counts cannot be read."""
    return _check_object("minsnap_delay.o", DELAY_KERNELS, "delay", vgpr_limit=64)


TAKE_KERNELS = ("take_counts_kernel", "minsnap_take_kernel", "fleet_order_kernel")


def check_take_kernels():
    """The kernels of csrc/minsnap_take.hip (missions of a plan selected and reordered, priorities into a within-group order):
    `_check_object`; the first two are plain copies like the delay kernels, the third counts over 2 KB LDS tiles of keys, and all run at
    least eight waves per SIMD (<= 64 vector registers; built: 24, 28 and 18).  Returns {kernel: VGPRs}, None when the counts cannot
    be read."""
    return _check_object("minsnap_take.o", TAKE_KERNELS, "take", vgpr_limit=64)


LAYER_KERNELS = ("layer_prepass_kernel", "minsnap_layer_kernel", "minsnap_shift_kernel")


def check_layer_kernels():
    """The kernels of csrc/minsnap_layer.hip (offset layers that clear the separation audit, and the offset transform): `_check_object`
    -- the coefficient sets of the decision kernel are indexed by constants only -- with the register limit of each from the LDS it
    ends up with (built: the decision kernel 50192 B of LDS -- the 48 KB tile, 1 KB of granted layers, two words -- hence three
    workgroups per CU and <= 168, at 137; the pre-pass and the transform no LDS, hence eight and <= 64, at 14 and 21).  Returns
    {kernel: VGPRs}, None when the counts cannot be read."""
    return _check_object("minsnap_layer.o", LAYER_KERNELS, "layer")


LAYER_OBS_KERNELS = ("layer_prepass_kernel", "minsnap_layer_kernel")


def check_layer_obs_kernels():
    """The kernels of csrc/minsnap_layer_obs.hip (the same search, refusing layers that put a mission into a cuboid): the same check as
    `check_layer_kernels` on the two instantiations with cuboids (built: the decision kernel 50976 B of LDS -- the search's 50192 B,
    768 B of cuboids, two more words -- hence still three workgroups per CU and <= 168, at 142; the pre-pass no LDS, <= 64, at 14).
    Returns {kernel: VGPRs}, None when the counts cannot be read."""
    return _check_object("minsnap_layer_obs.o", LAYER_OBS_KERNELS, "obstacle-aware layer")


def check_rollout_registers(obj: str = None):
    """Raise RuntimeError when a rollout variant needs more than 256 vector registers or spills any; returns the counts."""
    counts = rollout_register_counts(obj)
    if counts is None:
        return None
    if len(counts) < 40:
        raise RuntimeError(f"only {len(counts)} control_rollout_kernel variants found in the code object")
    over = [(n[:80], v) for n, v, _ in counts if v > VGPR_LIMIT]
    spills = [(n[:80], s) for n, _, s in counts if s > 0]
    if over or spills:
        raise RuntimeError(f"rollout kernels outside the two-waves-per-SIMD budget: > {VGPR_LIMIT} VGPRs {over}; spills {spills} "
                           f"(compiler: {compiler_version()})")
    return counts


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


def _disassemble_cfg(obj: str):
    """{kernel name: [Ins]} of the gfx950 code object inside `obj` -- instruction text with its address and branch target, which is
    what a check needs to follow the control flow -- or None when the object file or the LLVM tools are missing."""
    objdump = os.path.join(LLVM_BIN, "llvm-objdump")
    if not (os.path.exists(obj) and os.path.exists(objdump)):
        return None
    tmp = tempfile.mkdtemp()
    try:
        shutil.copy(obj, os.path.join(tmp, "o.o"))
        subprocess.run([objdump, "--offloading", "o.o"], cwd=tmp, check=True, capture_output=True)
        co = [f for f in os.listdir(tmp) if "gfx950" in f][0]
        text = subprocess.run([objdump, "-d", "--no-show-raw-insn", os.path.join(tmp, co)], check=True, capture_output=True,
                              text=True).stdout
    finally:
        shutil.rmtree(tmp)
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


def _disassemble(obj: str):
    """{kernel name: [instruction text]}: `_disassemble_cfg` for the checks that read straight-line code."""
    return _disassemble_cfg(obj)


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
        poly = re.search(r"control_rollout_kernelILi\d+ELi\d+ELb[01]ELb[01]ELb[01]ELb([01])E", name).group(1) == "1"
        if poly:                                   # (its coefficient loads look alike; the compiler issues and waits for those itself)
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
    kernels = _disassemble(obj or os.path.join(PKG, "build", "minsnap_sample_stream.o"))
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
    `uav_ac._native.lib()`, `make check`): the rollout kernels' register budget, the row prefetch and the sampler's heading
    prefetch in the disassembly, no diagnostic symbol, the planning kernels' budgets.  A check that cannot run (no object files,
    no LLVM tools) is a FAILURE here: the output-only asm operands of row_issue / HeadingFromLds are only as safe as these
    checks, so a build they did not see must not pass for one they did.  Raises RuntimeError; on success writes
    lib/libuavac.buildcheck.json -- the library's sha256, its uavac_build_info() and the compiler the checks saw -- which
    travels with the library (tests/test_gpu_round6.py compares it with the library the GPU process loaded)."""
    import ctypes
    import json
    result = {}
    steps = (("rollout_registers", check_rollout_registers, lambda r: f"{len(r)} rollout kernels, at most {max(v for _, v, _ in r)} VGPRs, no spills"),
             ("row_prefetch", check_row_prefetch, lambda r: f"row prefetch of {r} row-fed rollout kernels verified on the control-flow graph of the disassembly"),
             ("scored_row_prefetch", lambda: check_row_prefetch(scored=True),
              lambda r: f"row prefetch of {r} row-fed scored rollout kernels verified the same way"),
             ("heading_prefetch", check_heading_prefetch, lambda r: f"{r} coefficient prefetches of the streaming sampler verified in the disassembly"),
             ("no_diagnostics", check_no_diagnostics, lambda r: "no diagnostic symbol exported"),
             ("planning_registers", check_planning_registers, lambda r: f"{len(r)} sampler / solve kernels inside their register budgets, no spills"),
             ("timeopt_kernels", check_timeopt_kernels,
              lambda r: f"{len(r)} time-optimisation kernels, at most {max(r.values())} VGPRs, no spills, no scratch memory"),
             ("separation_kernels", check_separation_kernels,
              lambda r: f"{len(r)} separation kernels, at most {max(r.values())} VGPRs, no spills, no scratch memory"),
             ("conflict_kernels", check_conflict_kernels,
              lambda r: f"{len(r)} conflict-list kernels, at most {max(r.values())} VGPRs, no spills, no scratch memory"),
             ("stagger_kernels", check_stagger_kernels,
              lambda r: f"{len(r)} stagger kernels, at most {max(r.values())} VGPRs, no spills, no scratch memory"),
             ("delay_kernels", check_delay_kernels,
              lambda r: f"{len(r)} delay kernels, at most {max(r.values())} VGPRs, no spills, no scratch memory"),
             ("take_kernels", check_take_kernels,
              lambda r: f"{len(r)} take kernels, at most {max(r.values())} VGPRs, no spills, no scratch memory"),
             ("flown_separation_kernels", check_flown_separation_kernels,
              lambda r: f"{len(r)} flown-separation kernels, at most {max(r.values())} VGPRs, no spills, no scratch memory"),
             ("flown_conflict_kernels", check_flown_conflict_kernels,
              lambda r: f"{len(r)} flown-conflict-list kernels, at most {max(r.values())} VGPRs, no spills, no scratch memory"),
             ("flown_audit_kernels", check_flown_audit_kernels,
              lambda r: f"{len(r)} flown-audit kernels, at most {max(r.values())} VGPRs, no spills, no scratch memory"),
             ("layer_kernels", check_layer_kernels,
              lambda r: f"{len(r)} layer kernels, at most {max(r.values())} VGPRs, no spills, no scratch memory"),
             ("layer_obs_kernels", check_layer_obs_kernels,
              lambda r: f"{len(r)} obstacle-aware layer kernels, at most {max(r.values())} VGPRs, no spills, no scratch memory"))
    for key, fn, say in steps:
        r = fn()
        if r is None:
            raise RuntimeError(f"build check '{key}' could not run (object files under {PKG}/build or the LLVM tools under {LLVM_BIN} are "
                               "missing): the library would ship unchecked")
        result[key] = len(r) if isinstance(r, list) else r      # (the time-optimisation, separation, stagger, delay and flown-separation checks: their {kernel: VGPRs} records)
        if verbose:
            print(f"build: {say(r)}")
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
