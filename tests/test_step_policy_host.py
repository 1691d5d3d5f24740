"""The launch policy behind the step loop (csrc/step_policy.hpp), without a device: `tests/step_policy_host.cpp` is built with
AddressSanitizer + UndefinedBehaviorSanitizer as an executable of its own.  It first runs its literal cases -- the kernel family,
the quads per thread of the looping sweep, the lanes and the chunk of a run call, the staging of the resident CSR kernel, the two
packed measurement grids: one case on each side of every threshold -- and then answers the queries below, which hold the rules
restated in tests/lat_variants_reference.py, tests/mc_variants_reference.py, tests/strip_ladder_reference.py and
tests/test_csr_reference_host.py against the header.  The restatements stay the independent statement; here they are checked
against the code that launches.

The kernel paths are bit-identical by design, so no GPU test can see any of these rules: a threshold that drifts costs speed and
fails nothing there.  This test is the guard."""
import os
import shutil
import subprocess

import pytest

import lat_variants_reference as LV
import mc_variants_reference as MV
import strip_ladder_reference as SL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pyisingmontecarlo_amd", "csrc")


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    """ask(queries) -> one answer (a list of ints) per query line; every run also repeats the program's literal cases"""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = str(tmp_path_factory.mktemp("step_policy") / "step_policy_host")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-I" + CSRC,
                            "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            os.path.join(ROOT, "tests", "step_policy_host.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and ("cannot find -lasan" in build.stderr or "cannot find -lubsan" in build.stderr or "libasan" in build.stderr):
        pytest.skip("sanitizer runtimes are not installed with this g++")
    assert build.returncode == 0, build.stderr[-3000:]
    assert "warning" not in build.stderr, build.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")

    def run(queries):
        out = subprocess.run([exe], input="".join(q + "\n" for q in queries), env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
        assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr[-3000:]
        lines = out.stdout.splitlines()
        assert lines[-1] == "step_policy_host: ok" and len(lines) == len(queries) + 1, out.stdout[-3000:]
        assert not any(line.startswith("error") for line in lines), out.stdout[-3000:]
        return [[int(x) for x in line.split()] for line in lines[:-1]]
    return run


def _opts(options):
    return "".join(f" opt.{k}={v}" for k, v in options.items())


def test_literal_cases_and_plain_compile(ask):
    assert ask([]) == []
    src = open(os.path.join(CSRC, "step_policy.hpp")).read()
    includes = [line for line in src.splitlines() if line.startswith("#include")]
    assert not any("hip" in line or "internal.hpp" in line for line in includes), includes
    assert "isingmc_states" not in src and "isingmc_graph" not in src
    plain = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", "-include", os.path.join(CSRC, "step_policy.hpp"),
                            "-x", "c++", os.devnull], capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0 and "warning" not in plain.stderr, plain.stderr[-3000:]


def test_lat_variants_reference_agrees(ask):
    cases = [(s, LV.variant_options(s, spread, lpq)) for s in LV.RESIDENT for spread, lpq in LV.resident_variants(s)]
    got = ask([f"lat_resident W={s.W} H={s.H}" + _opts(o) for s, o in cases])
    for (s, o), answer in zip(cases, got):
        spread, lpq, threads, lds = LV.resident_launch(s.W, s.H, o)
        assert answer == [int(spread), lpq, threads, lds], (s.name, o)
    fits = LV.RESIDENT + [LV.HOST_ONLY]
    assert [a[0] for a in ask([f"lat_fits W={s.W} H={s.H}" + _opts(s.options) for s in fits])] == [1] * len(LV.RESIDENT) + [0]
    assert all(LV.resident_fits(s.W, s.H, s.options) for s in LV.RESIDENT) and not LV.resident_fits(LV.HOST_ONLY.W, LV.HOST_ONLY.H, {})
    shapes = LV.RESIDENT + LV.FUSED + LV.MEASURE + [LV.HOST_ONLY]
    for s, (vec, cols_log2, uni, wpr, wpp, nquads) in zip(shapes, ask([f"shape W={s.W} H={s.H}" for s in shapes])):
        assert (bool(vec), bool(uni)) == (LV.vec(s.W, s.H), LV.uni(s.W, s.H)), s.name
        assert (wpr, wpp, nquads) == LV.geometry(s.W, s.H) and (not vec or cols_log2 == LV.cols_log2(s.W, s.H)), s.name


def test_mc_variants_reference_agrees(ask):
    cases = [(s.W, s.H, R, dict(s.options, **extra)) for s in MV.SHAPES for R in (3, 257)
             for extra in ({}, {"resident_spread": 2}, {"resident_spread": 0})]
    # ... and the shapes tests/test_mc_variants_host.py asks the restatement about beside its table
    cases += [args for args, _ in MV.LAUNCH_CASES] + [(256, 1028, 3, {})]
    fits = ask([f"lat_fits W={W} H={H} mc_mode={MV.MC_FIELD}" + _opts(o) for W, H, _, o in cases])
    launch = ask([f"mc_resident W={W} H={H} R={R} mc_mode={MV.MC_FIELD} n_cu={MV.N_CU}" + _opts(o) for W, H, R, o in cases])
    for (W, H, R, o), f, (spread, threads, lds) in zip(cases, fits, launch):
        assert bool(f[0]) == MV.resident_fits(W, H, o), (W, H, o)
        assert (bool(spread), threads) == MV.resident_launch(W, H, R, o), (W, H, R, o)
        nquads = MV.geometry(W, H)[2]
        assert lds == 2 * MV.geometry(W, H)[1] * 4 + (nquads * 8 * 16 if spread else 0)   # the planes, and a uint4 per lane in the spread form


def test_strip_ladder_reference_agrees(ask):
    shapes = []
    for nw, table in SL.SHAPES.items():
        for (W, H), _, S, _ in table:
            shapes += [(W, H, nw), (W, S, nw), (W, H + 1, nw)]
    # the refusals of test_strip_plan_restated (tests/test_strip_ladder_host.py)
    shapes += [args for args, _ in SL.STRIP_PLAN_CASES]
    got = ask([f"strip_plan W={W} H={H} R=1 timesteps=2 occ=8 n_cu=256 opt.strip_nw={nw}" for W, H, nw in shapes])
    served = 0
    for (W, H, nw), (use, nw_out, S, n_strips, qpr_log2, per_pass) in zip(shapes, got):
        want = SL.strip_plan(W, H, nw)
        assert bool(use) == (want is not None), (W, H, nw)
        if want:
            assert (1 << qpr_log2, S, n_strips) == want and nw_out == nw and per_pass == 1, (W, H, nw)
            served += 1
    assert served == 7   # the six shapes of the table and 256 x 128 cut by one wave
    rounds = [args for args, _ in SL.IN_KERNEL_CASES]
    queries = []
    for n_slots, n_rungs, timesteps, swap_every, *rest in rounds:
        passes, tracking = (rest[0] if rest else 1), (rest[1] if len(rest) > 1 else False)
        per_pass = n_slots if passes == 1 else (n_slots + passes - 1) // passes
        queries.append(f"pt_rounds strips=1 rpp={per_pass} R={n_slots} rungs={n_rungs} rounds={timesteps // swap_every} swap_every={swap_every} recorder={int(tracking)}")
    assert [a[0] for a in ask(queries)] == [SL.rounds_inside_the_launch(*r) for r in rounds]
    # what the restatement leaves to its caller: no strips for this ladder, the switch
    assert ask(["pt_rounds strips=0 rpp=8 R=8 rungs=8 rounds=6 swap_every=4", "pt_rounds strips=1 rpp=8 R=8 rungs=8 rounds=6 swap_every=4 opt.pt_in_kernel=0"]) == [[0], [0]]


def test_rb_rule_agrees(ask):
    import csr_reference as CR
    from test_csr_reference_host import rb_rule
    cases = [(1, 16387)] + [((c + 255) // 256, R) for c in CR.MULTI_CLASS_SIZES for R in (8003, 13)]
    assert [a[0] for a in ask([f"gen_rb blocks={b} R={R}" for b, R in cases])] == [rb_rule(b, R) for b, R in cases]
    forced = [(b, R, f) for b, R in cases for f in (1, 2, 4, 8)]
    assert [a[0] for a in ask([f"gen_rb blocks={b} R={R} opt.gen_rb={f}" for b, R, f in forced])] == [f for _, _, f in forced]
    assert ask(["gen_rb blocks=1 R=16387 opt.gen_rb=3", "gen_rb blocks=1 R=16387 opt.gen_rb=8 rb_max=4"]) == [[8], [4]]   # no width; the compiled bound
