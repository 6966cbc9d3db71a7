"""The build checks' reader and budget table (uav_ac/_buildcheck.py) on doctored metadata text and doctored kernel records: what
they must read the same and what they must refuse, each refusal with the kernel's name in the message.  CPU only; no object
file is read except by the two inventory tests at the end."""
import os
import shutil

import pytest

from conftest import PKG
from uav_ac import _buildcheck as bc

NS = "_ZN12_GLOBAL__N_1"
KEYS = {"agpr_count": 0, "group_segment_fixed_size": 0, "kernarg_segment_size": 48, "max_flat_workgroup_size": 256,
        "private_segment_fixed_size": 0, "sgpr_count": 22, "sgpr_spill_count": 0, "uniform_work_group_size": 1, "vgpr_count": 24,
        "vgpr_spill_count": 0, "wavefront_size": 64}


@pytest.fixture(autouse=True)
def _no_compiler_call(monkeypatch):
    monkeypatch.setattr(bc, "compiler_version", lambda: "a compiler")


def notes_text(kernels, backwards=False, arg_name=None):
    """Metadata notes as `llvm-readelf --notes` prints them, for [(name, {key: value})]; `backwards`: a kernel's keys in reversed
    order; `arg_name`: the first kernel argument carries that `.name`."""
    out = ["Displaying notes found in: .note", "  Owner                Data size \tDescription",
           "  AMDGPU               0x00000c55\tNT_AMDGPU_METADATA (AMDGPU Metadata)", "    AMDGPU Metadata:", "        ---", "amdhsa.kernels:"]
    for name, over in kernels:
        args = ["    .args:", "      - .address_space:  global"] + ([f"        .name:           {arg_name}"] if arg_name else []) + \
               ["        .offset:         0", "        .size:           8", "        .value_kind:     global_buffer",
                "      - .offset:         8", "        .size:           4", "        .value_kind:     by_value"]
        keys = {**KEYS, **over, "name": name, "symbol": name + ".kd"}
        blocks = [args if k == "args" else [f"    {'.' + k + ':':<16} {keys[k]}"] for k in sorted(list(keys) + ["args"], reverse=backwards)]
        lines = [line for block in blocks for line in block]
        out += ["  - " + lines[0][4:]] + lines[1:]
    return "\n".join(out + ["amdhsa.target:   amdgcn-amd-amdhsa--gfx950", "amdhsa.version:", "  - 1", "  - 2", "...", ""])


def K(name, vgpr=24, spill=0, private=0, lds=0):
    return bc.Kernel(NS + name, vgpr, spill, 22, 0, 0, private, lds)


def row(key, obj=None):
    return next(r for r in bc.BUDGETS if r.key == key and (obj is None or obj in r.obj))


def refused(r, kernels, *words):
    with pytest.raises(RuntimeError) as exc:
        bc.check_budget(r, kernels)
    for word in words:
        assert word in str(exc.value), (word, str(exc.value))


# ------------------------------------------------------------------------------------------------ the reader
TWO = [(NS + "19delay_counts_kernelEPKliiPKiPiPlS4_", {"group_segment_fixed_size": 32, "vgpr_count": 25}),
       (NS + "20minsnap_delay_kernelEPKdS1_PKiPKliidS3_S5_PdS6_PiS7_", {"sgpr_count": 63, "private_segment_fixed_size": 16, "vgpr_spill_count": 3,
                                                                         "agpr_count": 4, "sgpr_spill_count": 5})]


def test_records_are_read_by_key_name_whatever_the_order():
    want = [bc.Kernel(TWO[0][0], 25, 0, 22, 0, 0, 0, 32), bc.Kernel(TWO[1][0], 24, 3, 63, 5, 4, 16, 0)]
    assert bc.parse_kernels(notes_text(TWO)) == want
    assert notes_text(TWO, backwards=True) != notes_text(TWO) and ".wavefront_size" in notes_text(TWO, backwards=True).split("  - ")[1].splitlines()[0]
    assert bc.parse_kernels(notes_text(TWO, backwards=True)) == want


def test_an_argument_called_kernel_is_no_kernel():
    for backwards in (False, True):
        got = bc.parse_kernels(notes_text(TWO, backwards=backwards, arg_name="scratch_of_the_kernel"))
        assert [k.name for k in got] == [name for name, _ in TWO]


def test_text_without_device_code_holds_no_kernels():
    assert bc.parse_kernels("") == []
    assert bc.parse_kernels("There are no notes in this file.\n") == []
    assert bc.parse_kernels(notes_text([])) == []
    assert bc.parse_kernels(notes_text([]).replace("amdhsa.kernels:", "amdhsa.kernels: []")) == []


def test_a_kernel_block_without_a_register_count_is_refused_by_name():
    text = "\n".join(line for line in notes_text(TWO).splitlines() if ".vgpr_count" not in line)
    with pytest.raises(RuntimeError, match="delay_counts_kernel.*vgpr_count"):
        bc.parse_kernels(text)


def test_template_arguments_of_a_mangled_name():
    rollout = NS + "22control_rollout_kernelILi4ELi2ELb1ELb0ELb0ELb0ELb0ELb1ELi2EEEv4VehKPKdPKlPdPiiiS6_S6_S3_iim"
    assert bc.template_args(rollout) == (4, 2, True, False, False, False, False, True, 2)
    assert bc.template_args(NS + "20layer_prepass_kernelILb0EEEvPKdPKiPKliiS4_NS_5DeltaEPiS8_S8_PdS8_") == (False,)
    assert bc.template_args(NS + "17row_counts_kernelILb1EdEEvPKdiiT0_dPdPiS5_PlS5_PKl") == (True,)          # (a type follows the literal)
    assert bc.template_args(NS + "9an_offsetILin3ELj7EEEvPd") == (-3, 7)
    assert bc.template_args(NS + "20minsnap_delay_kernelEPKdS1_PKiPKliidS3_S5_PdS6_PiS7_") == ()


# ------------------------------------------------------------------------------------------------ the table
DELAY = [K("19delay_counts_kernelEPKl"), K("20minsnap_delay_kernelEPKd")]
FLOWN = [K("21flown_discover_kernelEPKd", 168, lds=49152), K("3csr21conflict_count_kernelEPKi", 64), K("3csr20conflict_list_kernelEPKi", 64),
         K("20flown_measure_kernelEPKd", 128)]
LAYER = [K("20minsnap_shift_kernelEPKd", 64), K("20layer_prepass_kernelILb0EEEvPKd", 64), K("20minsnap_layer_kernelILb0EEEvPKd", 168, lds=50192)]


def sampler(w, derivs, vgpr):
    return K(f"28minsnap_sample_stream_kernelILi{w}ELb1ELb{int(derivs)}ELb0EEEvPKd", vgpr)


def solve(kind, nreg, vgpr, n=0):
    return K(f"23minsnap_solve_{kind}_kernelILb0ELb0ELi{32 + n}ELi{nreg}EEEvPKd", vgpr)


SAMPLERS = [sampler(w, d, 128 if d or w == 16 else 80) for w in (2, 4, 8, 16) for d in (False, True)] * 3
SOLVES = [solve(kind, 5 if n == 0 else 0, 512 if n == 0 else 256, n) for kind in ("bt", "tw") for n in range(10)]


def swap(kernels, fragment, **change):
    """`kernels` with the record whose name contains `fragment` changed."""
    hit = [k for k in kernels if fragment in k.name]
    assert len(hit) >= 1
    return [k._replace(**change) if k is hit[0] else k for k in kernels]


def test_records_at_their_limits_pass():
    assert bc.check_budget(row("delay_kernels"), swap(DELAY, "delay_counts", vgpr_count=64)) is not None
    assert len(bc.check_budget(row("flown_conflict_kernels"), FLOWN)) == 4
    assert len(bc.check_budget(row("layer_kernels"), LAYER)) == 3
    assert len(bc.check_budget(row("planning_registers", "sample_stream"), SAMPLERS)) == 24
    assert len(bc.check_budget(row("planning_registers", "solve_bt"), SOLVES)) == 20
    # an "at least" row speaks of its own kernels alone: the rollout's object holds two helpers beside the variants
    rollout = [K(f"22control_rollout_kernelILi1ELi{i}ELb1EEEv4VehK", 256) for i in range(40)]
    assert len(bc.check_budget(row("rollout_registers"), rollout + [K("17state_init_kernelE4VehK", 300)])) == 40


def test_a_spill_and_scratch_memory_are_refused():
    refused(row("delay_kernels"), swap(DELAY, "delay_counts", vgpr_spill_count=1), "delay_counts_kernel")
    refused(row("delay_kernels"), swap(DELAY, "minsnap_delay", private_segment_fixed_size=8), "minsnap_delay_kernel", "8 private-segment bytes")
    refused(row("planning_registers", "sample_stream"), swap(SAMPLERS, "ILi4ELb1ELb0E", vgpr_spill_count=2), "minsnap_sample_stream_kernelILi4ELb1ELb0E")
    bc_solve = [K("23minsnap_solve_bc_kernelILb1EEEvPKd", 211), K("23minsnap_solve_bc_kernelILb0EEEvPKd", 217)]
    assert len(bc.check_budget(row("planning_registers", "solve_bc"), bc_solve)) == 2
    refused(row("planning_registers", "solve_bc"), swap(bc_solve, "ILb0E", private_segment_fixed_size=4), "minsnap_solve_bc_kernelILb0E")


def test_one_register_over_each_kind_of_limit_is_refused():
    refused(row("delay_kernels"), swap(DELAY, "delay_counts", vgpr_count=65), "delay_counts_kernel", "65")                  # one number
    for name, limit in row("flown_conflict_kernels").limit.items():                                                         # a number per kernel
        refused(row("flown_conflict_kernels"), swap(FLOWN, name, vgpr_count=limit + 1), name, str(limit + 1))
    refused(row("planning_registers", "sample_stream"), swap(SAMPLERS, "ILi2ELb1ELb0E", vgpr_count=81), "ILi2ELb1ELb0E")   # by template argument
    refused(row("planning_registers", "sample_stream"), swap(SAMPLERS, "ILi2ELb1ELb1E", vgpr_count=129), "ILi2ELb1ELb1E")
    refused(row("planning_registers", "sample_stream"), swap(SAMPLERS, "ILi16ELb1ELb0E", vgpr_count=129), "ILi16ELb1ELb0E")
    refused(row("planning_registers", "solve_bt"), swap(SOLVES, "tw_kernelILb0ELb0ELi33ELi0E", vgpr_count=257), "tw_kernelILb0ELb0ELi33ELi0E")
    refused(row("planning_registers", "solve_bt"), swap(SOLVES, "bt_kernelILb0ELb0ELi32ELi5E", vgpr_count=513), "bt_kernelILb0ELb0ELi32ELi5E")
    refused(row("layer_kernels"), swap(LAYER, "minsnap_layer_kernel", vgpr_count=169), "minsnap_layer_kernel", "169")       # from LDS
    refused(row("layer_kernels"), swap(LAYER, "layer_prepass", vgpr_count=65), "layer_prepass_kernel", "65")
    refused(row("layer_kernels"), swap(LAYER, "minsnap_shift", vgpr_count=129, group_segment_fixed_size=40 * 1024), "minsnap_shift_kernel", "129")


def test_a_layer_decision_kernel_with_two_workgroups_per_cu_is_refused():
    lds = bc.LDS_BYTES_PER_CU // 3 + 1
    assert len(bc.check_budget(row("layer_kernels"), swap(LAYER, "minsnap_layer_kernel", group_segment_fixed_size=lds - 1))) == 3
    refused(row("layer_kernels"), swap(LAYER, "minsnap_layer_kernel", group_segment_fixed_size=lds), "minsnap_layer_kernel", "fewer than three workgroups")
    refused(row("layer_obs_kernels"), swap(LAYER[1:], "minsnap_layer_kernel", group_segment_fixed_size=lds, vgpr_count=24), "minsnap_layer_kernel",
            "fewer than three workgroups")


def test_a_missing_kernel_an_extra_instantiation_and_too_few_variants_are_refused():
    refused(row("delay_kernels"), DELAY[1:], "missing: ['delay_counts_kernel']")
    refused(row("layer_kernels"), LAYER + [K("20layer_prepass_kernelILb1EEEvPKd", 14)], "4 kernels found", "layer_prepass_kernel")
    refused(row("delay_kernels"), DELAY + [K("17fill_f64_kernelEPdmd")], "3 kernels found", "minsnap_delay_kernel")
    assert len(bc.check_budget(row("timeopt_kernels"), [K(f"19{name}E", 10) for name in row("timeopt_kernels").kernels] +
                               [K("19row_counts_t_kernelILb0EEEvPKd", 10)])) == 10        # (the one further instantiation the row allows)
    rollout = [K(f"22control_rollout_kernelILi1ELi{i}ELb1EEEv4VehK", 256) for i in range(39)]
    refused(row("rollout_registers"), rollout, "39 kernels found", "at least 40 of control_rollout_kernel")
    refused(row("planning_registers", "sample_stream"), SAMPLERS[:19], "at least 20 of minsnap_sample_stream_kernel")
    refused(row("planning_registers", "solve_bt"), SOLVES[:19], "at least 20 of minsnap_solve_bt_kernel, minsnap_solve_tw_kernel")
    refused(row("planning_registers", "audit"), [K(f"20minsnap_audit_kernelILi64ELb{i}EEEvPKd", 100) for i in range(3)], "at least 4 of minsnap_audit_kernel")
    refused(row("planning_registers", "solve_bc"), [K("23minsnap_solve_bc_kernelILb1EEEvPKd", 211)], "1 kernels found", "minsnap_solve_bc_kernel")


# ------------------------------------------------------------------------------------------------ the inventory
def test_every_object_file_is_budgeted_or_listed_as_unbudgeted():
    listed = {o for r in bc.BUDGETS for o in r.obj.split()}
    assert not listed & set(bc.UNBUDGETED) and all(len(why) > 10 for why in bc.UNBUDGETED.values())
    if not os.path.isdir(os.path.join(PKG, "build")):
        pytest.skip("no build directory here (a library that was built elsewhere)")
    assert {f for f in os.listdir(os.path.join(PKG, "build")) if f.endswith(".o")} == listed | set(bc.UNBUDGETED)
    assert bc.check_inventory() == len(listed) + len(bc.UNBUDGETED)


def test_a_stray_object_file_fails_the_build():
    small = os.path.join(PKG, "build", "minsnap_first_yaw.o")
    if not os.path.exists(small):
        pytest.skip("no object files here (a library that was built elsewhere)")
    stray = os.path.join(PKG, "build", "extra.o")
    shutil.copy(small, stray)
    try:
        with pytest.raises(RuntimeError, match=r"neither BUDGETS nor UNBUDGETED.*extra\.o"):
            bc.run_all(write_stamp=False)
    finally:
        os.remove(stray)
