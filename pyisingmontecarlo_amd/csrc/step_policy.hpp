// The launch policy behind the step loop: which kernel family a container takes, which path a run call takes, and the shape of
// every launch whose shape is a choice -- as pure functions of values.  Almost every rule here is a measured threshold; its
// evidence (ratios, profile files, the ISINGMC_* switch that forces the choice) stands beside it.
// Plain C++17 (no HIP include, no runtime call): isingmc.hip and tempering.hip read a plan and launch; an occupancy figure of
// the runtime enters as a value, or as a callable where the query depends on what the rule computes on the way.
// tests/step_policy_host.cpp drives the header as an executable of its own (tests/test_step_policy_host.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "options.hpp"

namespace isingmc {
namespace step_policy {

// The bounds of the kernel headers that the rules compare against, restated on purpose: the headers that define them declare
// launchers over HIP types, and this file must compile without HIP.  isingmc.hip asserts that the values are the headers'.
constexpr uint32_t GEN_RESIDENT_BYTES = 32 * 1024; // general_types.hpp GEN_RESIDENT_MAX_BYTES
constexpr uint32_t LAT_RESIDENT_BYTES = 64 * 1024; // lattice_types.hpp LDS_RESIDENT_MAX_BYTES
constexpr uint32_t LAT_MEASURE_SLOTS = 16;         // lattice_types.hpp MEASURE_SLOTS
constexpr int PACKED_MAX_DEG = 6;                  // packed_types.hpp PK_MAX_DEG
constexpr uint32_t PACKED_MEASURE_POS = 32;        // packed_types.hpp PK_MEASURE_POS_PER_THREAD
constexpr uint32_t STRIP_WAVES_PER_CU = 16;        // strip_types.hpp STRIP_MAX_WAVES_PER_CU
constexpr int MC_MODE_NONE = 0;                    // mc_types.hpp MC_NONE

enum class GraphKind { Lattice2D, General };

// What the rules read of a graph (graph_facts of isingmc.hip fills it from the library's graph object)
struct GraphFacts {
    GraphKind kind = GraphKind::General;
    int mc_mode = MC_MODE_NONE; // lattices: the multi-class kernels' mode (a field, open boundaries, two |J|)
    uint64_t nvars = 0, state_words = 0;
    // lattices (LatGeom)
    uint32_t wpr = 0, wpp = 0, H = 0, nquads = 0;
    int cols_log2 = -1;
    bool vec = false, uniform_sign = true;
    // general graphs
    uint32_t n_colours = 2;
    uint64_t largest_class = 0;          // positions of the largest colour class, padding included
    uint32_t n_pos = 0;                  // positions of the replica-packed layout
    bool packed_ok = false, rj_ok = false;
    uint32_t rj_slots = 0;
    int pk_uni_deg = 0;
    bool stable_path = false;
    int n_cu = 256;
    uint32_t gen_stage_words[3] = {0, 0, 0}; // [mode] = gen_stage_words(..., mode) for modes 1 and 2 of gen_resident_kernel STAGE
};

// What the rules read of a container
struct ContainerFacts {
    size_t R = 0, groups = 0;
    bool packed = false, rj = false;
    bool strip_disabled = false; // a strip launch of the container timed out once
};

// The shape of a recognised W x H lattice in its checkerboard layout (graph.hip builds the graph from it)
struct LatticeShape {
    uint32_t wpr, wpp, nquads; // words per colour-row = W / 64, per plane = H * wpr, quads = wpp / 4
    bool vec;
    int cols_log2; // log2(quads per row) when the division-free, parity-uniform thread mapping applies (thread_to_quad), else -1
};
inline LatticeShape lattice_shape(uint32_t W, uint32_t H)
{
    LatticeShape G{};
    G.wpr = W / 64;
    G.wpp = H * G.wpr;
    G.nquads = G.wpp / 4;
    G.vec = G.wpr % 4 == 0;
    G.cols_log2 = -1;
    if (G.vec) {
        const uint32_t cols = G.wpr / 4;
        if ((cols & (cols - 1)) == 0) {
            int cl = 0;
            while ((1u << cl) < cols) cl++;
            const uint32_t rows_per_pair = cl >= 6 ? 1 : 2 * (64u >> cl);
            if (H % rows_per_pair == 0 && G.nquads % 64 == 0) G.cols_log2 = cl;
        }
    }
    return G;
}

// the division-free mapping: what the looping sweep kernel and the UNI instantiations need
inline bool uniform_mapping(const GraphFacts &g) { return g.vec && g.cols_log2 >= 0; }

// ------------------------------------------------------------------------------------------------
// kernel family
// ------------------------------------------------------------------------------------------------
// 0 checkerboard lattice kernels, 1 f64 CSR (one replica per word set), 2 replica-packed bit-sliced (S6), 3 replica-packed real-coupling (S7)
enum class Family { Checkerboard = 0, Csr = 1, PackedBits = 2, PackedReal = 3 };

// worth it from 16 replicas on and when the graph is too big for the LDS-resident per-replica kernel
// LDS-resident kernel for small graphs only: one workgroup walks a whole replica, ~13 us + 2.8..5 ns per site
// and timestep whatever the replica count, against ~5 us per colour class for the per-colour launches --
// measured crossover ~8 000 sites at 4 replicas, ~14 000 at 64 (profiles/r01_resident_threshold.txt); a
// 200 000-site graph ran 13x slower resident than streamed.
inline bool gen_resident_fits(const GraphFacts &g, size_t n_replicas)
{
    return g.state_words * sizeof(uint32_t) <= GEN_RESIDENT_BYTES && g.nvars <= (n_replicas < 16 ? 8000u : 12000u);
}

// Packed or per-replica?  The packed kernels launch once per colour class and timestep; the LDS-resident CSR kernel runs a whole
// call in one launch with one workgroup per replica, which wins on small graphs (they are bound by parallelism, and a word of 32
// replicas concentrates them on few compute units).  Measured (profiles/r03_real_small.txt, r03_few_replicas.txt,
// r03_packed_resident_experiment.txt; attempts/s of the packed path over the per-replica one):
//  * real-coupling path, graphs the resident CSR kernel takes: 8 000 sites 1.7x at 16 replicas, 4 096 sites 1.0x at 64 and 1.5x at
//    256, 1 728 sites 0.7x at 256 and 2.6x at 1 024, never at 1 024 sites; big graphs: 0.9x at 4 replicas, 1.5x at 8, 2.7x at 15;
//  * bit-sliced path (a thread decides FOUR positions: a quarter of the threads): resident-size graphs 0.8x at 4 096 sites x 256,
//    3.0x x 1 024; 0.67x at 8 000 x 256, 2.6x x 1 024; 13 824 sites 0.7x at 16 replicas, 1.2x at 64; 128^3: 1.4x at ONE replica.
inline bool packed_worth_it(const GraphFacts &g, size_t n_replicas, bool real_path)
{
    const uint64_t work = uint64_t(g.nvars) * n_replicas; // attempts per timestep
    const bool csr_resident = gen_resident_fits(g, n_replicas); // (the A/B switch ISINGMC_DISABLE_RESIDENT changes kernels, never the family)
    if (real_path) {
        // partial groups draw only their own replicas' Philox calls: 1.09x the CSR launches at ONE experiment (2048^2 Gaussian glass,
        // profiles/r03_few_replicas.txt; re-measured in profiles/r04_real_eligibility.txt), 1.4x at 2, 2.0x at 4, 2.9x at 8
        if (!csr_resident) return n_replicas >= 1;
        return n_replicas >= 16 && (g.nvars >= 8000 || (g.nvars >= 1500 && work >= (uint64_t(3) << 19))); // 1.5 x 2^20: re-measured with the graph staged in LDS
    }
    return work >= (uint64_t(1) << (csr_resident ? 22 : 19));
}

// The family a container of n_replicas experiments takes on this graph (ISINGMC_FORCE_REAL / _DISABLE_REAL / _FORCE_PACKED /
// _DISABLE_PACKED in the environment at creation); also what the C ABI's family-for-a-graph query answers.  A recognised lattice never runs packed.
inline Family choose_family(const GraphFacts &g, const Options &o, size_t n_replicas)
{
    if (g.kind == GraphKind::Lattice2D) return Family::Checkerboard;
    if (g.rj_ok && !o.disable_real && (!g.packed_ok || o.force_real)) {
        // (stable_path: the family follows from the graph alone -- experiment k must not change when the call asks for more of them)
        if (o.force_real || g.stable_path) return n_replicas > 0 ? Family::PackedReal : Family::Csr;
        return packed_worth_it(g, n_replicas, true) ? Family::PackedReal : Family::Csr;
    }
    if (!g.packed_ok || o.disable_packed) return Family::Csr;
    // pk_sweep_kernel addresses the ELL table through one buffer descriptor with 32-bit byte offsets
    if (uint64_t(g.n_pos) * PACKED_MAX_DEG * sizeof(uint32_t) >= (uint64_t(1) << 31)) return Family::Csr;
    if (o.force_packed || g.stable_path) return n_replicas > 0 ? Family::PackedBits : Family::Csr;
    return packed_worth_it(g, n_replicas, false) ? Family::PackedBits : Family::Csr;
}

// ------------------------------------------------------------------------------------------------
// persistent strip kernel (strip_kernels.hpp): when and how
// ------------------------------------------------------------------------------------------------
struct StripChoice {
    bool use = false;
    int nw = 1; // waves per strip (workgroup)
    uint32_t S = 0, n_strips = 0, qpr_log2 = 0; // rows per strip, strips per replica, log2(quads per row)
    size_t replicas_per_pass = 0; // a pass = one launch over a block of replicas for all timesteps of the chunk
};

// dynamic LDS of one strip workgroup: two planes of S rows and their two halo rows, and the poll words
inline size_t strip_lds_bytes(uint32_t S, uint32_t wpr) { return (size_t(2) * (S + 2) * wpr + 16) * sizeof(uint32_t); }

// Mid-size lattices only: a per-colour launch of the streaming kernel must be short enough for the ~5 us it loses
// between dependent launches to matter (<= ISINGMC_STRIP_MAX_WG workgroups in all, default the resident limit), the geometry must cut into strips of 256 quads with at least two strips per replica, and the poll of a
// half-sweep must fit one workgroup (2 rows of <= 128 words).  ISINGMC_STRIP=0 disables, =1 forces (tests, A/B runs).
// blocks_per_cu(nw, lds bytes): the runtime's occupancy figure of the instantiation the launch would run
template <typename Occupancy>
StripChoice strip_plan(const GraphFacts &g, const Options &o, size_t R, bool strip_disabled, size_t timesteps, Occupancy &&blocks_per_cu)
{
    StripChoice P;
    const int mode = o.strip;
    if (mode == 0 || strip_disabled || g.kind != GraphKind::Lattice2D || !g.vec || timesteps < 2) return P;
    const uint32_t qpr = g.wpr / 4;
    if ((qpr & (qpr - 1)) != 0 || qpr > 32) return P; // power of two, at least two rows per wave
    P.nw = o.strip_nw == 1 ? 1 : 4; // measured on 1024^2 x 64 (round 4, with wave priorities): 8.4 (4) / 8.6 (1) us per timestep; with exchange rounds 10.4 (4) / 12.0 (1)
    const uint32_t S = 64 * uint32_t(P.nw) / qpr;
    if (g.H % S != 0 || g.H / S < 2) return P;
    // Every workgroup of a launch must be resident at once.  Per CU: what the runtime's occupancy calculation grants this
    // instantiation with its dynamic LDS (registers, LDS, wave slots), and never more than the policy bound of
    // STRIP_WAVES_PER_CU waves (beyond it the per-colour launches are faster anyway).
    const int by_occupancy = blocks_per_cu(P.nw, strip_lds_bytes(S, g.wpr));
    const size_t per_cu = std::min<size_t>(size_t(STRIP_WAVES_PER_CU) / size_t(P.nw), size_t(std::max(by_occupancy, 0)));
    const size_t limit = per_cu * size_t(std::max(g.n_cu, 1)); // workgroups resident at once
    const size_t n_strips = g.H / S, total = R * n_strips;
    if (limit == 0 || n_strips > limit) return P;
    // one pass only by default: with twice the replicas (1024^2 x 128) the per-colour launches are long enough to win (16.7 vs 18.6 us)
    if (mode != 1 && total > size_t(o.strip_max_wg >= 0 ? o.strip_max_wg : int(limit))) return P;
    const size_t passes = (total + limit - 1) / limit;
    P.replicas_per_pass = (R + passes - 1) / passes;
    while (P.replicas_per_pass * n_strips > limit) P.replicas_per_pass--;
    if (P.replicas_per_pass == 0) return P;
    P.S = S;
    P.n_strips = uint32_t(n_strips);
    uint32_t ql = 0;
    while ((1u << ql) < qpr) ql++;
    P.qpr_log2 = ql;
    P.use = true;
    return P;
}

// Exchange rounds of isingmc_pt_run(rounds * swap_every + tail, swap_every) that the strips of ONE persistent launch decide
// among themselves (the last round of the block is always decided at the kernel boundary); 0: one launch per round.
// strips, replicas_per_pass: the ladder's strip_plan.
// recorder_on: minimum tracking reads every round's energies, sums per rung (S19) and the periodic series
// (S21, S22) the configurations and the permutation between the rounds: one launch per round.  ISINGMC_PT_IN_KERNEL=0: never
inline size_t pt_rounds_in_kernel(bool strips, size_t replicas_per_pass, const Options &o, size_t R, size_t n_rungs, size_t rounds, size_t swap_every,
                                  bool recorder_on)
{
    const bool in_kernel = strips && replicas_per_pass >= R && rounds >= 2 && rounds * swap_every <= 65536 && R == n_rungs &&
                           o.pt_in_kernel != 0 && !recorder_on;
    return in_kernel ? rounds - 1 : 0;
}

// ------------------------------------------------------------------------------------------------
// run_steps: one plan per call (kernel path, chunk of timesteps, replica lanes)
// ------------------------------------------------------------------------------------------------
enum class StepPath { Packed, LatResident, LatStrip, LatStream, McResident, McStream, GenResident, GenCsr };

struct StepPlan {
    StepPath path = StepPath::GenCsr;
    size_t chunk = 0;      // timesteps per runner call (per-step energies are read back chunk by chunk)
    size_t step_slots = 1; // per-step counter slots per replica: the streaming kernels measure into LAT_MEASURE_SLOTS partial counters
    size_t lanes = 1;      // replica lanes (streams)
    StripChoice strip;
};

// small lattices: one LDS-resident launch per chunk of timesteps instead of two launches per timestep (up to 1024 quads per
// colour: beyond that one workgroup per replica is slower than the launches it saves); the multi-class kernels' bound too.
// ISINGMC_DISABLE_RESIDENT=1 (at creation): always use the per-colour launches (A/B runs, parity tests of both paths)
inline bool lat_resident_fits(const GraphFacts &g, const Options &o)
{
    return g.state_words * sizeof(uint32_t) <= LAT_RESIDENT_BYTES && g.nquads <= 1024 && o.disable_resident == 0;
}

// strip_blocks_per_cu(nw, lds bytes): as strip_plan's, asked only where the strip kernel is a candidate
template <typename Occupancy>
StepPlan plan_steps(const GraphFacts &g, const Options &o, const ContainerFacts &c, size_t timesteps, bool energies_per_step,
                    Occupancy &&strip_blocks_per_cu)
{
    const size_t R = c.R;
    StepPlan P;
    if (c.packed) {
        P.path = StepPath::Packed;
        P.chunk = std::min<size_t>(timesteps, 2048);
        // The replica groups are independent: mid-size launches (a few waves per SIMD: the 64^3 glass x 64 replicas puts ONE wave on a
        // SIMD per colour-class launch) leave the chip idle around every kernel boundary, so the groups go to several streams and one
        // lane's launch gap / ramp / tail overlaps the other lanes' work (as the lattice path's replica lanes).  ISINGMC_PK_STREAMS=<n> forces.
        if (!energies_per_step && c.groups >= 2) {
            const uint64_t waves_per_launch = c.groups * g.largest_class / (c.rj ? 64 : 256); // a thread decides 1 (real) / 4 (bit-sliced) positions
            const int forced = o.pk_streams;
            if (forced > 0) P.lanes = size_t(forced);
            // measured (tools/pk_lanes_ab.py, profiles/r03_pk_lanes_ab.txt): two lanes +7 % (2048^2 x 256) to +43 % (512^2 x 64) from ~2 000 waves per
            // launch on, -3..-13 % below (32^3 x 64: the launches are too short for the fork / join); four lanes: worse than two almost everywhere
            // Short calls (the 10-timestep blocks between tempering rounds) double their launch count with lanes and run into the host's
            // launch rate sooner: 64^3 x 64 rungs went from 24.5 to 31 us per timestep; they take lanes only for long launches
            else if (timesteps >= 64 ? waves_per_launch >= 2048 : timesteps >= 4 && waves_per_launch >= 16384) P.lanes = 2;
            P.lanes = std::min(P.lanes, c.groups);
        }
        return P;
    }
    if (g.kind != GraphKind::Lattice2D) P.path = gen_resident_fits(g, R) && o.disable_resident == 0 ? StepPath::GenResident : StepPath::GenCsr;
    // lattices with a field or open boundaries: the multi-class kernels
    else if (g.mc_mode != MC_MODE_NONE) P.path = lat_resident_fits(g, o) ? StepPath::McResident : StepPath::McStream;
    else if (lat_resident_fits(g, o)) P.path = StepPath::LatResident;
    else {
        P.strip = strip_plan(g, o, R, c.strip_disabled, timesteps, strip_blocks_per_cu);
        P.path = P.strip.use ? StepPath::LatStrip : StepPath::LatStream;
    }
    if (energies_per_step && P.path == StepPath::LatStream) P.step_slots = LAT_MEASURE_SLOTS;
    // per-step counters: 16 B per (step, replica) and counter slot, at most 32 MiB per chunk on each side of the bus
    P.chunk = energies_per_step ? std::max<size_t>(1, std::min<size_t>(timesteps, (size_t(32) << 20) / (16 * R * P.step_slots))) : timesteps;
    if (P.path == StepPath::LatResident || P.path == StepPath::LatStrip || P.path == StepPath::McResident || P.path == StepPath::GenResident)
        P.chunk = std::min<size_t>(P.chunk, 65536);
    // mid-size launches (a few waves per SIMD) leave the GPU idle around every kernel boundary: run the
    // replica blocks on several streams.  Large launches (c2) keep the chip full on one stream.
    if ((P.path == StepPath::LatStream || P.path == StepPath::McStream) && !energies_per_step) {
        const size_t waves_per_launch = R * ((g.nquads + 255) / 256) * 4;
        if (o.streams > 0) P.lanes = size_t(o.streams);
        // < 64 waves per SIMD per launch: +17..33 % with 2 lanes (4 go host-bound); short calls lose it to fork/join.
        // Large launches: +2.8 % (one block's drain overlaps the other's ramp); the fork/join is ~45 us per call
        else if (waves_per_launch < 64 * 1024 ? timesteps >= 64 : timesteps >= 8) P.lanes = 2;
        P.lanes = std::min(P.lanes, R);
    }
    return P;
}

// ------------------------------------------------------------------------------------------------
// launch shapes
// ------------------------------------------------------------------------------------------------
// Quads per thread of a streaming half-sweep (1 = the one-quad kernel, else lat_sweep_loop_kernel), for a dispatch of `n`
// replicas of the container's R.  A looping thread walks `iters` quads nquads / iters apart: that distance must be a whole,
// even number of rows (the kernel carries the row parity and the column across its iterations), i.e. 2 * iters divides H.
//  - resident-sized launch: the largest power of two <= 16 at which the workgroups of ALL lanes of the half-sweep together
//    are a whole multiple, and at least twice, of the workgroups the device holds at once (resident_wgs: occupancy query x CUs):
//    every wave slot is refilled by the wave's own next quad, all workgroups are equally long and the rounds are whole, so there
//    is no tail to quantise; the second round lets the CUs that ran ahead take more than their share.  4096^2 x 256 on 256
//    CUs: 65536 one-quad workgroups, 2048 resident => 16 quads per thread, two rounds.  Measured there, same box, against
//    two quads per thread: 16 quads +3.0 %, 8 quads +2.7 %, 32 quads (ONE round) +1.3 %; one lane instead of two: -7 % at
//    16, -11 % at 32 (profiles/2026-10-17_resident_sweep_ab.txt);
//  - else two quads per thread while that leaves >= 8 workgroups per CU (measured before the rule above existed: 2 quads +4 %,
//    4 +2.7 %, 8 +1.3 % on uniform J; +-J: 2 quads +2.6 %).  Workgroups of 128 or 64 threads: no gain.
// ISINGMC_SWEEP_ITERS=1|2|4|8|16|32 forces the choice (measurement and tests).
// does sweep_iters read resident_wgs for this lattice?  (a forced choice, or a lattice without the looping kernel's mapping: no query)
inline bool sweep_iters_reads_residency(const GraphFacts &g, const Options &o) { return uniform_mapping(g) && o.sweep_iters == 0; }

inline uint32_t sweep_iters(const GraphFacts &g, const Options &o, size_t R, size_t n, int resident_wgs)
{
    const auto fits = [&](uint32_t k) { return g.nquads % (256 * k) == 0 && g.H % (2 * k) == 0; };
    const int forced = o.sweep_iters;
    if (forced) return forced > 1 && forced <= 32 && (forced & (forced - 1)) == 0 && fits(uint32_t(forced)) ? uint32_t(forced) : 1u;
    const size_t resident = size_t(resident_wgs);
    for (uint32_t k = 16; resident > 0 && k > 1; k >>= 1) {
        if (!fits(k)) continue;
        const size_t wgs = size_t(g.nquads / (256 * k)) * R;
        if (wgs >= 2 * resident && wgs % resident == 0) return k;
    }
    return fits(2) && size_t(g.nquads / 512) * n >= size_t(8) * 256 ? 2u : 1u;
}

// one LDS-resident launch of a small lattice: its form, its workgroup and its dynamic LDS
struct LatResidentLaunch {
    bool spread;      // lat_resident_spread_kernel / the SPREAD form of lat_mc_resident_kernel instead of one lane per quad
    int lpq;          // lanes per quad of the spread form
    unsigned threads;
    size_t lds_bytes;
};

// small lattices: eight (four, two) lanes per quad, one (two, four) Philox calls each (lat_resident_spread_kernel)
// ... while every replica of the call is resident at once: beyond that the one-lane-per-quad kernel's small workgroups fill
// the chip better (measured, tools/small_lattice_spread_ab.py: 64^2 x 2048 4.1 against 5.9 us, x 4096 10.5 against 9.1;
// 128^2 x 512 4.4 against 5.4, x 1024 8.7 against 5.3).  ISINGMC_RESIDENT_SPREAD=0 / 2: never / whenever the lattice allows
// blocks_per_cu(lpq, threads, lds bytes): the runtime's occupancy figure of the spread instantiation, asked only in mode 1
template <typename Occupancy>
LatResidentLaunch lat_resident_launch(const GraphFacts &g, const Options &o, size_t R, Occupancy &&blocks_per_cu)
{
    const int spread_mode = o.resident_spread;
    // eight lanes per quad only: with four or two (256 / 512 quads per colour, 1024 threads) the barriers of a 16-wave workgroup
    // cost more than the shorter chain saves (256^2 x 64: 5.7 against 5.1 us; ISINGMC_RESIDENT_LPQ=4 / 2 for A/B runs)
    const int lpq_forced = o.resident_lpq;
    const int lpq = lpq_forced == 4 || lpq_forced == 2 ? lpq_forced : 8;
    bool spread = spread_mode != 0 && size_t(g.nquads) * size_t(lpq) <= 1024;
    const unsigned spread_threads = unsigned((size_t(g.nquads) * size_t(lpq) + 63) / 64 * 64);
    const size_t spread_lds = g.state_words * sizeof(uint32_t) + size_t(g.nquads) * 8 * 16; // (16: a uint4 of random words per lane)
    if (spread && spread_mode != 2) {
        const int per_cu = blocks_per_cu(lpq, spread_threads, spread_lds);
        spread = per_cu > 0 && R <= size_t(g.n_cu) * size_t(per_cu);
    }
    const unsigned threads = spread ? spread_threads : unsigned(std::min<size_t>(1024, (g.nquads + 63) / 64 * 64));
    const size_t lds = spread ? spread_lds : g.state_words * sizeof(uint32_t);
    return {spread, lpq, threads, lds};
}

// small lattices, few enough replicas to be resident at once: eight lanes per quad (lat_mc_resident_kernel SPREAD; the
// kernel takes the spread form when the launch's LDS holds the random words too).  ISINGMC_RESIDENT_SPREAD=0: off
inline LatResidentLaunch mc_resident_launch(const GraphFacts &g, const Options &o, size_t R)
{
    const int mc_spread_mode = o.resident_spread;
    const size_t spread_threads = (size_t(g.nquads) * 8 + 63) / 64 * 64;
    const bool mc_spread = mc_spread_mode != 0 && spread_threads <= 1024 &&
                           (mc_spread_mode == 2 || R <= size_t(g.n_cu) * std::max<size_t>(1, 1024 / spread_threads));
    const unsigned threads = mc_spread ? unsigned(spread_threads) : unsigned(std::min<size_t>(1024, (g.nquads + 63) / 64 * 64));
    const size_t mc_lds = g.state_words * sizeof(uint32_t) + (mc_spread ? size_t(g.nquads) * 8 * 16 : 0);
    return {mc_spread, 8, threads, mc_lds};
}

struct GenResidentLaunch {
    int stage; // gen_resident_kernel STAGE: 0 the state alone in LDS, 1 the graph too, 2 its topology too
    unsigned threads;
    size_t lds_bytes;
};

// the graph in LDS too (gen_resident_kernel STAGE) while every replica of the call can still be resident at once (160 KB
// of LDS per compute unit): small graphs, where a timestep is a chain of dependent loads.  Everything when that fits,
// else the topology alone (the links of the chain); ISINGMC_GEN_STAGE=0 / 1 / 2 forces none / all / topology (A/B runs)
inline GenResidentLaunch gen_resident_launch(const GraphFacts &g, const Options &o, size_t R)
{
    const unsigned threads = std::max<unsigned>(64, unsigned(std::min<uint64_t>(1024, g.largest_class)));
    const int stage_mode = o.gen_stage;
    const size_t lds_cu = 160 * 1024, lds_max = 150 * 1024; // (a few KB stay free for the kernel's static LDS)
    int stage = 0;
    size_t bytes[3] = {0, 0, 0}, resident[3] = {0, 0, 0};
    for (int mode = 1; mode <= 2; mode++) {
        bytes[mode] = size_t(g.gen_stage_words[mode]) * 4;
        if (bytes[mode] <= lds_max) resident[mode] = std::min<size_t>(2048 / threads, lds_cu / (bytes[mode] + 1024)); // workgroups per compute unit
    }
    if (stage_mode == 0) stage = 0;
    else if (stage_mode == 1 || stage_mode == 2) stage = resident[stage_mode] ? stage_mode : 0;
    else if (resident[1] && (R <= size_t(g.n_cu) * resident[1] || threads > 512 || resident[2] <= resident[1])) stage = 1;
    // (measured, tools/small_graph_stage_ab.py: workgroups of <= 512 threads gain from running side by side, so when
    //  the full copy would keep some of the call's replicas waiting the smaller one wins: 32^2 x 1024 5.7 against
    //  6.2 us, 8^3 x 1024 3.5 against 4.4; 1024-thread workgroups do not: 12^3 x 512 6.6 against 9.4)
    else if (resident[2]) stage = 2;
    return {stage, threads, stage ? bytes[stage] : size_t(g.state_words * sizeof(uint32_t))};
}

// replicas per thread of gen_sweep_kernel for a class of `blocks` 256-position blocks: rb_max (the compiled GEN_RB) amortises the
// CSR stream of a big class; a class that would leave the chip short of workgroups (< 8 per CU) halves it until the grid is
// large enough (200 000 sites x 64 replicas: 56 us per launch at 8 replicas per thread)
// ISINGMC_GEN_RB_FORCE=1 / 2 / 4 / 8 (option gen_rb) forces, up to the compiled GEN_RB (tests, A/B runs): same results
inline size_t gen_replicas_per_thread(size_t blocks, size_t R, const Options &o, size_t rb_max)
{
    size_t rb = rb_max;
    while (rb > 1 && (R < rb || blocks * ((R + rb - 1) / rb) < 2048)) rb /= 2;
    if (const int f = o.gen_rb; f == 1 || f == 2 || f == 4 || f == 8) rb = std::min<size_t>(size_t(f), rb_max);
    return rb;
}

// bit-sliced packed measurement: positions per thread, halved until the launch has >= 1024 workgroups (not below 8: the
// transpose at the end of a chunk costs as much as ~16 positions), and the workgroups per group
struct PkMeasureGrid {
    uint32_t pos_per_thread;
    unsigned blocks;
};
inline PkMeasureGrid pk_measure_grid(uint32_t n_pos, size_t groups)
{
    uint32_t ppt = PACKED_MEASURE_POS;
    while (ppt > 8 && size_t((n_pos + 256 * ppt - 1) / (256 * ppt)) * groups < 1024) ppt /= 2;
    return {ppt, unsigned(std::max<uint32_t>(1, std::min<uint32_t>(2048, (n_pos + 256 * ppt - 1) / (256 * ppt))))};
}

// real-coupling measurement, workgroups per group of a launch over `ng` groups: all workgroups resident at once (blocks_per_cu:
// the runtime's occupancy figure for the instantiation, at least 1), every one walks its share of the scan_blocks blocks; a grid
// one round and a bit long would run its tail at a fraction of the chip
// ISINGMC_REAL_MEASURE_WGS=<n> (option real_measure_wgs) replaces the figure (tests, A/B runs): exact integer sums, same results
inline size_t rj_measure_grid_x(int n_cu, const Options &o, int blocks_per_cu, size_t scan_blocks, size_t ng)
{
    const size_t resident = o.real_measure_wgs > 0 ? size_t(o.real_measure_wgs) : size_t(blocks_per_cu) * size_t(std::max(n_cu, 1));
    return std::max<size_t>(std::min(scan_blocks, std::max<size_t>(1, resident / ng)), 1);
}

} // namespace step_policy
} // namespace isingmc
