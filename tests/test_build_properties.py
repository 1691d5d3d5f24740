"""Code-generation properties the measured performance depends on (no GPU needed: hipcc cross-compiles).

The sweep kernels are bound by vector-ALU cycles and need all 8 wave slots of a SIMD: 64 VGPRs is the limit.
A behaviour-neutral source change once compiled the looping kernel to 66 VGPRs and cost 3 % (DESIGN.md
section 4); this test makes such a drift visible on the CPU box."""
import os
import re
import shutil
import subprocess

import pytest

import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
sys.path.insert(0, ROOT)
from pyisingmontecarlo_amd.build import HIP_CODEGEN_FLAGS, HIP_SOURCES  # noqa: E402  (the flags the shipped library is built with)
ASM_FLAGS = HIP_CODEGEN_FLAGS + ["-S", "--cuda-device-only"]


@pytest.fixture(scope="module")
def unit_asm(tmp_path_factory):
    """the device assembly of every translation unit of the library that may hold device code, compiled with the library's own flags"""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc not available")
    tmp = tmp_path_factory.mktemp("asm")
    procs = []
    for name in HIP_SOURCES:
        if not name.endswith(".hip"):
            continue
        out = tmp / (name + ".s")
        procs.append((name, out, subprocess.Popen([HIPCC] + ASM_FLAGS + ["-o", str(out), os.path.join(ROOT, "pyisingmontecarlo_amd", "csrc", name)],
                                                  stderr=subprocess.DEVNULL)))
    texts = {}
    for name, out, proc in procs:
        assert proc.wait() == 0, name
        texts[name] = out.read_text()
    return texts


def _kernel_meta(asm, mangled_prefix):
    metas = []
    for m in re.finditer(r"\.name:\s+(" + re.escape(mangled_prefix) + r"\w*)", asm):
        after = asm[m.start():m.start() + 900]
        before = asm[max(0, m.start() - 700):m.start() + 900]
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", after).group(1))
        spill = int(re.search(r"\.vgpr_spill_count:\s+(\d+)", after).group(1))
        scratch = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", before).group(1))
        metas.append((m.group(1), vgpr, spill, scratch))
    return metas


@pytest.mark.parametrize("prefix", ["_ZN7isingmc21lat_sweep_loop_kernel", "_ZN7isingmc16lat_sweep_kernel"])
def test_sweep_kernels_keep_eight_waves_per_simd(unit_asm, prefix):
    metas = _kernel_meta(unit_asm["lattice_kernels.hip"], prefix)
    assert metas, "kernel not found in the device assembly"
    for name, vgpr, spill, scratch in metas:
        if prefix.endswith("loop_kernel") and "ILb1E" in name:
            continue  # the +-J looping instantiation needs 66-68 registers (7 waves); measured faster than the alternatives
        assert vgpr <= 64, f"{name}: {vgpr} VGPRs (> 64: fewer than 8 waves per SIMD)"
        assert spill == 0 and scratch == 0, f"{name}: spills to scratch"


def test_packed_sweep_kernel_keeps_eight_waves(unit_asm):
    """Capped at 64 VGPRs with __launch_bounds__(256, 8): three spilled registers cost less than the eighth wave
    gains (the kernel is bound by the latency of its dependent memory phases): +2 % on 256^3 x 64."""
    metas = _kernel_meta(unit_asm["packed_kernels.hip"], "_ZN7isingmc15pk_sweep_kernel")
    assert metas, "kernel not found in the device assembly"
    for name, vgpr, spill, scratch in metas:
        assert vgpr <= 64 and spill <= 4 and scratch <= 32, f"{name}: {vgpr} VGPRs, {spill} spills, {scratch} B scratch"


def test_packed_uniform_degree_kernels_keep_eight_waves(unit_asm):
    """pk_sweep_uni_kernel<D, UB, PMJ, TABLE>: at most a few spilled registers at __launch_bounds__(256, 8)."""
    metas = _kernel_meta(unit_asm["packed_uni_kernels.hip"], "_ZN7isingmc19pk_sweep_uni_kernel")
    assert len(metas) == 32
    for name, vgpr, spill, scratch in metas:
        assert vgpr <= 64 and spill <= 4 and scratch <= 32, f"{name}: {vgpr} VGPRs, {spill} spills, {scratch} B scratch"
        if "ELb0ELb" in name:  # one coupling sign: the c5 kernels
            assert spill == 0 and scratch == 0, f"{name}: spills"


def test_multi_class_kernels_keep_their_occupancy(unit_asm):
    """lat_mc_sweep_kernel: the uniform-field instantiation the field benchmark runs (<FIELD, uniform sign, 2^k mapping, no
    sign planes>) stays at 7 waves per SIMD (<= 72 VGPRs; a runtime branch on the sign-plane pointer once made it 97), the
    open-boundary ones at 8 (<= 64), and nothing spills."""
    metas = _kernel_meta(unit_asm["mc_kernels.hip"], "_ZN7isingmc19lat_mc_sweep_kernel")
    assert len(metas) == 24
    for name, vgpr, spill, scratch in metas:
        assert spill == 0 and scratch == 0, f"{name}: spills"
        if "ILi1ELb0ELb1ELb0E" in name:
            assert vgpr <= 72, f"{name}: {vgpr} VGPRs"
        if "ILi2E" in name:
            assert vgpr <= 65, f"{name}: {vgpr} VGPRs"


def test_no_vector_store_data_is_overwritten_right_behind_the_store(unit_asm):
    """A buffer_store_dwordx3/x4 reads its data registers some cycles after it issues.  The compiler's hazard model
    (GCNHazardRecognizer::createsVALUHazard) inserts wait states only when the store's soffset is an immediate; with a REGISTER
    soffset it inserts none -- and on a loaded MI355X the fused sweep+measure kernel, whose bit counts overwrote the data
    registers in the very next instruction, stored bit counts instead of spins (round 3; wrong configurations from ~1500
    workgroups per launch on; isolated in profiles/r03_store_hazard.txt: the window is the one instruction slot behind the store).
    No kernel of ANY translation unit of the library (compiled with the library's own flags) may write such a store's data
    registers within 8 instructions of it: ANY instruction whose destination overlaps them counts (vector ALU, LDS reads, memory
    loads, accumulator moves), and a branch inside the window is followed on BOTH paths (fall-through: one slot; taken: four slots,
    the instruction fetch is redirected); a branch to a label the scan cannot find fails the test."""
    texts = unit_asm
    store = re.compile(r"\s(buffer_store_dwordx[34])\s+v\[(\d+):(\d+)\],\s*\S+,\s*s\[\d+:\d+\],\s*(\S+)")
    dest = re.compile(r"^(\w+)\s+(?:v(\d+)\b|v\[(\d+):(\d+)\]|a(\d+)\b|a\[(\d+):(\d+)\])")   # first operand = destination
    no_dest = ("buffer_store", "global_store", "flat_store", "ds_write", "ds_add", "ds_sub", "ds_max", "ds_min", "ds_and", "ds_or", "ds_xor",
               "v_cmp", "v_cmpx", "buffer_atomic", "global_atomic", "s_", "exp")
    stores = 0
    for name, text in texts.items():
        lines = text.split("\n")
        labels = {m.group(1): i for i, l in enumerate(lines) for m in [re.match(r"^(\.LBB\w+):", l)] if m}
        kernel = "?"
        for i, line in enumerate(lines):
            m0 = re.match(r"^(_Z\w+):", line)
            if m0:
                kernel = m0.group(1)
            m = store.search(line)
            if not m or not re.match(r"s\d+$", m.group(4)):
                continue  # immediate soffset: the compiler inserts the wait states itself
            stores += 1
            lo, hi = int(m.group(2)), int(m.group(3))

            def scan(j, budget, seen_at):
                """walk the instruction stream from line j with `budget` instruction slots left; follow branch targets too"""
                while j < len(lines) and budget > 0:
                    t = lines[j].strip()
                    j += 1
                    if not t or t.startswith((";", ".p2align", ".loc", ".cfi")) or re.match(r"^\.LBB\w+:", t):
                        continue  # (a label: other paths may enter here -- they are scanned from their own stores)
                    if t.startswith("s_endpgm"):
                        return
                    budget -= 1
                    br = re.match(r"^s_c?branch\w*\s+(\.LBB\w+)", t)
                    if br:
                        key = (br.group(1), budget)
                        assert br.group(1) in labels, f"{name}: {kernel[:70]}: branch to an unknown label behind `{line.strip()}`"
                        if key not in seen_at:  # a TAKEN branch redirects the instruction fetch: counted as four slots of the window
                            seen_at.add(key)
                            scan(labels[br.group(1)] + 1, budget - 3, seen_at)
                        if t.startswith("s_branch"):
                            return  # unconditional: no fall-through
                        continue
                    d = dest.match(t)
                    if d and not t.startswith(no_dest):
                        a = int(d.group(2) or d.group(3) or d.group(5) or d.group(6))
                        b = int(d.group(2) or d.group(4) or d.group(5) or d.group(7))
                        is_acc = d.group(5) is not None or d.group(6) is not None
                        assert is_acc or b < lo or a > hi, f"{name}: {kernel[:70]}: `{t}` {8 - budget} instruction(s) behind `{line.strip()}`"

            scan(i + 1, 8, set())
    assert stores >= 4, "no register-offset vector stores found: has the pattern of this test gone stale?"


# kernels per name in the units whose launchers turn runtime values into template arguments (csrc/kernel_pick.hpp)
KERNEL_CENSUS = {
    "lattice_kernels.hip": {"lat_init": 1, "lat_measure": 4, "lat_resident": 8, "lat_sweep": 12, "lat_sweep_loop": 4, "lat_sweep_measure": 12},
    "spread_kernels.hip": {"lat_resident_spread": 24},
    "strip_kernels.hip": {"lat_strip": 16},
    "mc_kernels.hip": {"lat_mc_sweep": 24, "lat_mc_resident": 24, "lat_mc_measure_aniso": 2, "lat_mc_measure_open": 2},
    "packed_uni_kernels.hip": {"pk_sweep_uni": 32, "pk_philox_table": 1},
    "real_kernels.hip": {"rj_sweep": 48, "rj_measure": 24, "rj_energy_from_counts": 1},
    "general_kernels.hip": {"gen_init": 1, "gen_sweep": 8, "gen_measure": 2, "gen_reduce": 1, "gen_resident": 6},
    "best_kernels.hip": {"best_decide": 2, "best_keep_rows": 1, "best_keep_bits": 1},
    "overlap_class_kernels.hip": {"ovl_lat_class": 1, "ovl_lat_class_between": 1, "ovl_pk_class": 2},
}


def test_the_launcher_units_hold_exactly_their_instantiations(unit_asm):
    """The launchers select an instantiation per choice, and a choice that depends on another one is decided inside the selection
    (UNI only together with VEC, sign planes only for the modes with a field, ...): a Cartesian selection would compile kernels nothing
    launches, a dropped branch would leave a launch without its kernel.  Neither shows in any result; the count per kernel name does."""
    for unit, expected in KERNEL_CENSUS.items():
        census = {}
        for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", unit_asm[unit], re.M):
            m = re.match(r"_ZN7isingmc(?:12_GLOBAL__N_1|L)?(\d+)", sym)  # (in an unnamed namespace, or static)
            assert m, f"{unit}: {sym}"
            name = sym[m.end():m.end() + int(m.group(1))]
            assert name.endswith("_kernel"), f"{unit}: {sym}"
            census[name[:-len("_kernel")]] = census.get(name[:-len("_kernel")], 0) + 1
        assert census == expected, unit


# every unit that is neither a kernel unit nor the probe's: none of them may compile device code
HOST_UNITS = [name for name in HIP_SOURCES if name.endswith(".hip") and not name.endswith("_kernels.hip") and name != "debug.hip"]


def test_every_kernel_is_compiled_in_exactly_one_unit(unit_asm):
    """Kernels live in *_kernels.hip units behind plain launchers.  A header that defines a kernel and reaches a second unit (through
    internal.hpp, say) compiles a copy of that kernel into the unit's code object: dead device code, and one more place where the
    register allocation of a tuned kernel could drift unseen.  Across the library every kernel symbol occurs in exactly one unit, the
    host units hold none, and debug.hip holds its clock probe alone."""
    where = {}
    for name, text in unit_asm.items():
        for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
            where.setdefault(sym, []).append(name)
    for kernel, unit in (("lat_sweep_loop_kernel", "lattice_kernels.hip"), ("gen_sweep_kernel", "general_kernels.hip"),
                         ("pk_sweep_kernel", "packed_kernels.hip"), ("pt_swap_kernel", "tempering_kernels.hip")):
        assert any(kernel in sym and units == [unit] for sym, units in where.items()), f"{kernel} not found in {unit}: has the pattern of this test gone stale?"
    twice = {sym: units for sym, units in where.items() if len(units) != 1}
    assert not twice, twice
    for name in HOST_UNITS:
        assert name in unit_asm, name
        held = [sym for sym, units in where.items() if name in units]
        assert not held, f"{name} compiles device code: {held}"
    probe = [sym for sym, units in where.items() if "debug.hip" in units]
    assert len(probe) == 1 and "clock_probe_kernel" in probe[0], probe
