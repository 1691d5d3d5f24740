// Stand-alone driver of csrc/step_policy.hpp (built with ASan + UBSan by tests/test_step_policy_host.py), no device.
//  1. The rules that have no restatement in tests/*_reference.py are pinned here with literal cases, one on each side of every
//     threshold: the expected values were derived by hand from the text of the rules as they stood in isingmc.hip.
//  2. Then it answers queries from stdin, one per line -- `rule key=value ...` -- with one line each, so that the pytest can hold
//     the Python restatements against the header.  Keys: W H (a lattice), or nvars state_words largest_class n_pos packed_ok rj_ok
//     stable_path stage1 stage2 (a general graph); mc_mode n_cu; opt.<name> (Options::set); the rule's own arguments.
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "step_policy.hpp"

using namespace isingmc::step_policy;

static int g_failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::printf("step_policy_host: line %d: %s\n", __LINE__, #cond);         \
            g_failures++;                                                            \
        }                                                                            \
    } while (0)

static GraphFacts lattice(uint32_t W, uint32_t H, int mc_mode = 0)
{
    const LatticeShape s = lattice_shape(W, H);
    GraphFacts g;
    g.kind = GraphKind::Lattice2D;
    g.mc_mode = mc_mode;
    g.nvars = uint64_t(W) * H;
    g.wpr = s.wpr; g.wpp = s.wpp; g.H = H; g.nquads = s.nquads; g.cols_log2 = s.cols_log2; g.vec = s.vec;
    g.state_words = 2 * uint64_t(s.wpp);
    return g;
}

static GraphFacts general(uint64_t nvars, uint64_t state_words, bool packed_ok, bool rj_ok)
{
    GraphFacts g;
    g.nvars = nvars;
    g.state_words = state_words;
    g.packed_ok = packed_ok;
    g.rj_ok = rj_ok;
    g.n_pos = uint32_t(nvars);
    return g;
}

static Options opt(const char *name = nullptr, long value = 0)
{
    Options o;
    if (name && !o.set(name, value)) g_failures++;
    return o;
}

static const auto occ8 = [](auto...) { return 8; };

static void family_cases()
{
    const Options o;
    const auto fam = [](const GraphFacts &g, const Options &op, size_t n) { return int(choose_family(g, op, n)); };
    CHECK(fam(lattice(64, 4), opt("force_packed", 1), 100) == 0);
    // bit-sliced: work = nvars * n against 2^19 off-resident (more than 12 000 sites), 2^22 on a graph the resident CSR kernel takes
    CHECK(fam(general(524287, 64, true, false), o, 1) == 1 && fam(general(524288, 64, true, false), o, 1) == 2);
    CHECK(fam(general(2047, 64, true, false), o, 2049) == 1 && fam(general(4096, 128, true, false), o, 1024) == 2);
    CHECK(fam(general(4096, 128, true, false), o, 128) == 1);   // 2^19 is not enough on a resident-size graph
    CHECK(fam(general(4096, 8193, true, false), o, 128) == 2);  // ... whose state is one word too long for the resident kernel
    CHECK(fam(general(4096, 8192, true, false), o, 128) == 1);
    CHECK(fam(general(12001, 64, true, false), o, 44) == 2 && fam(general(12000, 64, true, false), o, 44) == 1); // 528 044 >= 2^19; resident below
    CHECK(fam(general(8001, 64, true, false), o, 15) == 1 && fam(general(8001, 64, true, false), o, 66) == 1);   // 66: resident (<= 12 000 from 16 on)
    CHECK(fam(general(40000, 64, true, true), o, 14) == 2); // both layouts: the bit-sliced rule (560 000 >= 2^19)
    // real couplings
    const auto real = [](uint64_t nvars, uint64_t words = 64) { return general(nvars, words, false, true); };
    CHECK(fam(real(7999), o, 16) == 1 && fam(real(8000), o, 16) == 3);
    CHECK(fam(real(8000), o, 15) == 1 && fam(real(8001), o, 15) == 3); // 15 replicas: resident up to 8 000 sites; beyond, from one replica on
    CHECK(fam(real(1536), o, 1023) == 1 && fam(real(1536), o, 1024) == 3); // work = 3 * 2^19 exactly
    CHECK(fam(real(1500), o, 1048) == 1 && fam(real(1500), o, 1049) == 3);
    CHECK(fam(real(1499), o, 2000) == 1);
    CHECK(fam(real(20000), o, 1) == 3 && fam(real(20000), o, 0) == 1);
    CHECK(fam(real(1000, 8192), o, 1) == 1 && fam(real(1000, 8193), o, 1) == 3);
    CHECK(fam(real(12000), o, 16) == 3 && fam(real(12001), o, 16) == 3);
    // force_*, disable_*, stable_path: with no replica the per-replica family
    CHECK(fam(real(100), opt("force_real", 1), 1) == 3 && fam(real(100), opt("force_real", 1), 0) == 1);
    CHECK(fam(general(100, 4, true, true), opt("force_real", 1), 1) == 3 && fam(general(100, 4, true, true), o, 1) == 1);
    CHECK(fam(real(20000), opt("disable_real", 1), 64) == 1);
    CHECK(fam(general(100, 4, true, false), opt("force_packed", 1), 1) == 2 && fam(general(100, 4, true, false), opt("force_packed", 1), 0) == 1);
    CHECK(fam(general(524288, 64, true, false), opt("disable_packed", 1), 1000) == 1);
    GraphFacts st = real(100);
    st.stable_path = true;
    CHECK(fam(st, o, 1) == 3 && fam(st, o, 0) == 1);
    st = general(100, 4, true, false);
    st.stable_path = true;
    CHECK(fam(st, o, 1) == 2 && fam(st, o, 0) == 1);
    // the ELL table behind one buffer descriptor: n_pos * 6 * 4 bytes below 2^31
    GraphFacts big = general(100, 4, true, false);
    big.n_pos = 89478485;
    CHECK(fam(big, opt("force_packed", 1), 1) == 2);
    big.n_pos = 89478486;
    CHECK(fam(big, opt("force_packed", 1), 1) == 1);
}

static void sweep_iters_cases()
{
    const Options o;
    const GraphFacts big = lattice(4096, 4096), mid = lattice(1024, 1024), odd = lattice(256, 1028);
    CHECK(big.nquads == 65536 && mid.nquads == 4096 && odd.nquads == 1028);
    CHECK(sweep_iters(big, o, 256, 256, 2048) == 16);  // 4096 workgroups of 16 quads per thread: two whole rounds
    CHECK(sweep_iters(big, o, 128, 128, 2048) == 8);   // 16: 2048 < 2 * 2048
    CHECK(sweep_iters(big, o, 255, 255, 2048) == 2);   // no k with wgs % 2048 == 0: two quads per thread
    CHECK(sweep_iters(mid, o, 256, 256, 0) == 2 && sweep_iters(mid, o, 256, 255, 0) == 1); // 8 * 256 workgroups of two quads
    CHECK(sweep_iters(odd, o, 4096, 4096, 0) == 1);    // 1028 quads: no whole workgroups of two
    CHECK(sweep_iters(big, opt("sweep_iters", 32), 1, 1, 2048) == 32 && sweep_iters(big, opt("sweep_iters", 4), 256, 256, 2048) == 4);
    CHECK(sweep_iters(big, opt("sweep_iters", 3), 256, 256, 2048) == 1 && sweep_iters(big, opt("sweep_iters", 64), 256, 256, 2048) == 1);
    CHECK(sweep_iters(big, opt("sweep_iters", 1), 256, 256, 2048) == 1 && sweep_iters(odd, opt("sweep_iters", 2), 256, 256, 2048) == 1);
    // the occupancy figure is asked only where the rule reads it: the looping kernel's mapping, nothing forced
    CHECK(sweep_iters_reads_residency(big, o) && !sweep_iters_reads_residency(big, opt("sweep_iters", 2)) && !sweep_iters_reads_residency(lattice(768, 12), o));
}

static void plan_cases()
{
    const Options o, nostrip = opt("strip", 0);
    const auto plan = [](const GraphFacts &g, const Options &op, ContainerFacts c, size_t timesteps, bool eps) {
        return plan_steps(g, op, c, timesteps, eps, occ8);
    };
    // ---- packed: lanes by waves per launch = groups * largest class / 256 (bit-sliced) or / 64 (real), chunk 2048
    GraphFacts pk = general(1 << 20, 1 << 15, true, false);
    const auto packed = [](size_t groups, bool rj = false) { return ContainerFacts{32 * groups, groups, true, rj, false}; };
    pk.largest_class = 262144;
    CHECK(plan(pk, o, packed(2), 64, false).lanes == 2 && plan(pk, o, packed(2), 63, false).lanes == 1);   // 2048 waves
    CHECK(plan(pk, o, packed(16), 4, false).lanes == 2 && plan(pk, o, packed(16), 3, false).lanes == 1);   // 16384 waves
    CHECK(plan(pk, o, packed(15), 63, false).lanes == 1);
    pk.largest_class = 262143;
    CHECK(plan(pk, o, packed(2), 64, false).lanes == 1 && plan(pk, o, packed(16), 4, false).lanes == 1);   // 2047, 16383 waves
    pk.largest_class = 65536;
    CHECK(plan(pk, o, packed(2, true), 64, false).lanes == 2 && plan(pk, o, packed(2), 64, false).lanes == 1);
    CHECK(plan(pk, opt("pk_streams", 4), packed(2), 1, false).lanes == 2 && plan(pk, opt("pk_streams", 4), packed(8), 1, false).lanes == 4);
    CHECK(plan(pk, opt("pk_streams", 4), packed(1), 1, false).lanes == 1);
    pk.largest_class = 262144;
    CHECK(plan(pk, o, packed(16), 64, true).lanes == 1); // per-step energies: one lane
    const StepPlan pp = plan(pk, o, packed(2), 5000, false);
    CHECK(pp.path == StepPath::Packed && pp.chunk == 2048 && pp.step_slots == 1 && plan(pk, o, packed(2), 100, true).chunk == 100);
    // ---- lattice streams: waves per launch = R * ceil(nquads / 256) * 4 against 64 * 1024
    const GraphFacts mid = lattice(1024, 1024), field = lattice(1024, 1024, 1);
    const auto reps = [](size_t R) { return ContainerFacts{R, 0, false, false, false}; };
    for (const GraphFacts &g : {mid, field}) {
        CHECK(plan(g, nostrip, reps(1023), 63, false).lanes == 1 && plan(g, nostrip, reps(1023), 64, false).lanes == 2); // 65472 waves
        CHECK(plan(g, nostrip, reps(1024), 7, false).lanes == 1 && plan(g, nostrip, reps(1024), 8, false).lanes == 2);   // 65536 waves
        CHECK(plan(g, nostrip, reps(1024), 63, false).lanes == 2 && plan(g, nostrip, reps(1023), 8, false).lanes == 1);
        CHECK(plan(g, nostrip, reps(1), 64, false).lanes == 1 && plan(g, opt("streams", 4), reps(2), 1, false).lanes == 2);
        CHECK(plan(g, nostrip, reps(1024), 64, true).lanes == 1);
    }
    CHECK(plan(mid, nostrip, reps(8), 10, false).path == StepPath::LatStream && plan(field, o, reps(8), 10, false).path == StepPath::McStream);
    // ---- chunk: 32 MiB of 16-byte counters per (step, replica, slot); 65536 timesteps at most on the four resident paths
    const StepPlan eps = plan(mid, nostrip, reps(1024), 1000, true);
    CHECK(eps.step_slots == 16 && eps.chunk == 128 && plan(mid, nostrip, reps(1024), 100, true).chunk == 100);
    CHECK(plan(field, o, reps(1024), 10000, true).step_slots == 1 && plan(field, o, reps(1024), 10000, true).chunk == 2048);
    CHECK(plan(mid, nostrip, reps(size_t(1) << 22), 1000, true).chunk == 1);
    CHECK(plan(mid, nostrip, reps(8), 100000, false).chunk == 100000 && plan(field, o, reps(8), 100000, false).chunk == 100000);
    const GraphFacts tiny = lattice(64, 4), tiny_field = lattice(256, 8, 2), strips = lattice(1024, 1024);
    CHECK(plan(tiny, o, reps(8), 100000, false).path == StepPath::LatResident && plan(tiny, o, reps(8), 100000, false).chunk == 65536);
    CHECK(plan(tiny, o, reps(8), 100000, true).chunk == 65536 && plan(tiny, o, reps(8), 65535, false).chunk == 65535);
    CHECK(plan(tiny_field, o, reps(8), 100000, false).path == StepPath::McResident && plan(tiny_field, o, reps(8), 100000, false).chunk == 65536);
    CHECK(plan(lattice(1024, 192), o, reps(8), 100000, false).path == StepPath::LatResident); // 768 quads: resident before the strips are asked
    const StepPlan sp = plan(strips, o, reps(8), 100000, false);
    CHECK(sp.path == StepPath::LatStrip && sp.chunk == 65536 && sp.strip.use && sp.strip.nw == 4 && sp.strip.S == 64 && sp.strip.n_strips == 16 &&
          sp.strip.qpr_log2 == 2 && sp.strip.replicas_per_pass == 8 && sp.lanes == 1);
    CHECK(plan(strips, o, ContainerFacts{8, 0, false, false, true}, 100000, false).path == StepPath::LatStream); // a strip launch timed out once
    CHECK(plan(strips, o, reps(8), 1, false).path == StepPath::LatStream);
    CHECK(plan(tiny, opt("disable_resident", 1), reps(8), 100000, false).path == StepPath::LatStream);
    CHECK(plan(lattice(512, 512), o, reps(8), 10, false).path == StepPath::LatResident);   // 1024 quads
    CHECK(plan(lattice(256, 1028), nostrip, reps(8), 10, false).path == StepPath::LatStream); // 1028 quads
    const GraphFacts small = general(8000, 250, false, false), large = general(8001, 251, false, false);
    CHECK(plan(small, o, reps(15), 100000, false).path == StepPath::GenResident && plan(small, o, reps(15), 100000, false).chunk == 65536);
    CHECK(plan(large, o, reps(15), 100000, false).path == StepPath::GenCsr && plan(large, o, reps(15), 100000, false).chunk == 100000);
    CHECK(plan(large, o, reps(16), 10, false).path == StepPath::GenResident && plan(general(12001, 376, false, false), o, reps(16), 10, false).path == StepPath::GenCsr);
    CHECK(plan(small, opt("disable_resident", 1), reps(15), 10, false).path == StepPath::GenCsr && plan(small, o, reps(15), 10, false).lanes == 1);
    CHECK(strip_lds_bytes(64, 16) == 8512);
}

static void gen_resident_cases()
{
    // resident[m] = min(2048 / threads, 160 KB / (bytes[m] + 1 KB)) workgroups per compute unit, 0 beyond 150 KB; 256 compute units
    const auto launch = [](uint32_t words1, uint32_t words2, uint64_t largest, size_t R, int gen_stage = -1) {
        GraphFacts g = general(1000, 100, false, false);
        g.largest_class = largest;
        g.gen_stage_words[1] = words1;
        g.gen_stage_words[2] = words2;
        return gen_resident_launch(g, opt("gen_stage", gen_stage), R);
    };
    const auto is = [](const GenResidentLaunch &L, int stage, unsigned threads, size_t lds) { return L.stage == stage && L.threads == threads && L.lds_bytes == lds; };
    CHECK(is(launch(4096, 2048, 256, 2048), 1, 256, 16384));  // every replica resident with the whole graph staged (8 per CU)
    CHECK(is(launch(4096, 2048, 256, 2049), 1, 256, 16384));  // ... not all, but the topology alone fits no more workgroups: 8 against 8
    CHECK(is(launch(16384, 2048, 256, 512), 1, 256, 65536));  // 2 per CU
    CHECK(is(launch(16384, 2048, 256, 513), 2, 256, 8192));   // ... one replica more: the topology alone, 8 per CU
    CHECK(is(launch(32768, 2048, 1024, 10000), 1, 1024, 131072)); // workgroups of more than 512 threads keep the full copy
    CHECK(is(launch(32768, 2048, 513, 10000), 1, 513, 131072) && is(launch(32768, 2048, 512, 10000), 2, 512, 8192));
    CHECK(is(launch(38400, 2048, 64, 256), 1, 64, 153600) && is(launch(38401, 2048, 64, 256), 2, 64, 8192)); // 150 KB
    CHECK(is(launch(40000, 39000, 30, 1), 0, 64, 400));       // neither fits: the state alone
    CHECK(is(launch(4096, 2048, 256, 1, 0), 0, 256, 400) && is(launch(16384, 2048, 256, 100000, 1), 1, 256, 65536));
    CHECK(is(launch(4096, 2048, 256, 1, 2), 2, 256, 8192) && is(launch(40000, 2048, 256, 1, 1), 0, 256, 400));
    CHECK(is(launch(40000, 39000, 256, 1, 2), 0, 256, 400));
}

static void measure_grid_cases()
{
    const auto grid = [](uint32_t n_pos, size_t groups) {
        const PkMeasureGrid m = pk_measure_grid(n_pos, groups);
        return std::make_pair(m.pos_per_thread, m.blocks);
    };
    CHECK(grid(8388608, 1) == std::make_pair(32u, 1024u) && grid(8380416, 1) == std::make_pair(16u, 2046u)); // 1024 / 1023 workgroups at 32
    CHECK(grid(512, 1) == std::make_pair(8u, 1u) && grid(33554432, 1) == std::make_pair(32u, 2048u));
    CHECK(grid(8192, 1024) == std::make_pair(32u, 1u) && grid(8192, 1023) == std::make_pair(16u, 2u));
    const Options o;
    const int g = 256; // compute units
    CHECK(rj_measure_grid_x(g, o, 8, 5000, 1) == 2048 && rj_measure_grid_x(g, o, 8, 100, 1) == 100 && rj_measure_grid_x(g, o, 8, 5000, 4) == 512);
    CHECK(rj_measure_grid_x(g, o, 8, 5000, 4096) == 1 && rj_measure_grid_x(g, o, 8, 0, 1) == 1);
    CHECK(rj_measure_grid_x(g, opt("real_measure_wgs", 300), 8, 5000, 2) == 150);
    CHECK(rj_measure_grid_x(0, o, 8, 5000, 1) == 8);
}

// ---- queries ------------------------------------------------------------------------------------------------------------------------
using Query = std::map<std::string, long long>;
static long long get(const Query &q, const char *key, long long dflt = 0)
{
    const auto it = q.find(key);
    return it == q.end() ? dflt : it->second;
}

static std::string answer(const std::string &rule, const Query &q)
{
    GraphFacts g;
    if (q.count("W")) g = lattice(uint32_t(get(q, "W")), uint32_t(get(q, "H")), int(get(q, "mc_mode")));
    else {
        g = general(uint64_t(get(q, "nvars")), uint64_t(get(q, "state_words")), get(q, "packed_ok") != 0, get(q, "rj_ok") != 0);
        g.largest_class = uint64_t(get(q, "largest_class"));
        g.n_pos = uint32_t(get(q, "n_pos", get(q, "nvars")));
        g.stable_path = get(q, "stable_path") != 0;
        g.gen_stage_words[1] = uint32_t(get(q, "stage1"));
        g.gen_stage_words[2] = uint32_t(get(q, "stage2"));
    }
    g.n_cu = int(get(q, "n_cu", 256));
    Options o;
    for (const auto &kv : q)
        if (kv.first.rfind("opt.", 0) == 0 && !o.set(kv.first.substr(4), long(kv.second))) return "error: unknown option " + kv.first;
    const size_t R = size_t(get(q, "R", 1));
    const int occ = int(get(q, "occ", 8));
    std::ostringstream out;
    if (rule == "shape") out << g.vec << ' ' << g.cols_log2 << ' ' << uniform_mapping(g) << ' ' << g.wpr << ' ' << g.wpp << ' ' << g.nquads;
    else if (rule == "lat_fits") out << lat_resident_fits(g, o);
    else if (rule == "lat_resident") {
        const LatResidentLaunch L = lat_resident_launch(g, o, R, [occ](int, unsigned, size_t) { return occ; });
        out << L.spread << ' ' << (L.spread ? L.lpq : 0) << ' ' << L.threads << ' ' << L.lds_bytes;
    } else if (rule == "mc_resident") {
        const LatResidentLaunch L = mc_resident_launch(g, o, R);
        out << L.spread << ' ' << L.threads << ' ' << L.lds_bytes;
    } else if (rule == "strip_plan") {
        const StripChoice P = strip_plan(g, o, R, get(q, "strip_disabled") != 0, size_t(get(q, "timesteps", 2)), [occ](int, size_t) { return occ; });
        out << P.use << ' ' << P.nw << ' ' << P.S << ' ' << P.n_strips << ' ' << P.qpr_log2 << ' ' << P.replicas_per_pass;
    } else if (rule == "pt_rounds")
        out << pt_rounds_in_kernel(get(q, "strips", 1) != 0, size_t(get(q, "rpp")), o, R, size_t(get(q, "rungs")), size_t(get(q, "rounds")),
                                   size_t(get(q, "swap_every")), get(q, "recorder") != 0);
    else if (rule == "gen_rb") out << gen_replicas_per_thread(size_t(get(q, "blocks")), R, o, size_t(get(q, "rb_max", 8)));
    else if (rule == "family") out << int(choose_family(g, o, size_t(get(q, "n"))));
    else return "error: unknown rule " + rule;
    return out.str();
}

int main()
{
    family_cases();
    sweep_iters_cases();
    plan_cases();
    gen_resident_cases();
    measure_grid_cases();
    for (std::string line; std::getline(std::cin, line);) {
        std::istringstream in(line);
        std::string rule, word;
        Query q;
        in >> rule;
        while (in >> word) {
            const size_t eq = word.find('=');
            q[word.substr(0, eq)] = eq == std::string::npos ? 1 : std::stoll(word.substr(eq + 1));
        }
        if (!rule.empty()) std::cout << answer(rule, q) << '\n';
    }
    if (g_failures) return 1;
    std::printf("step_policy_host: ok\n");
    return 0;
}
