// Host-side logic of libisingmc.so that needs no device: seeds, schedules, lattice recogniser,
// adjacency + greedy colouring.  See include/isingmc.h for the reference lines each part replaces.
#pragma once
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "autocorr_ring.hpp"
#include "general_types.hpp"

namespace isingmc {

// xoshiro256++ seeded by SplitMix64: rand 0.8 SmallRng::seed_from_u64 on 64-bit targets
// (published algorithm; what lattice.rs:85-90 instantiates).
struct SmallRng {
    uint64_t s[4];
    explicit SmallRng(uint64_t seed);
    uint64_t next_u64();
};

std::vector<uint64_t> make_seeds(bool has_seed, uint64_t seed_gen, size_t n);

// lattice.rs:320-334 + 358-365; returns "" or an error message
std::string expand_schedule(const uint64_t *stop_t, const double *stop_beta, size_t n_stops,
                            size_t timesteps, bool compat_constant_beta, double *betas_out);

struct Lattice2D {
    bool ok = false;
    int W = 0, H = 0;
    double jabs = 0.0;                  // |J| of the horizontal bonds (of every bond when isotropic)
    double jabs_y = 0.0;                // |J| of the vertical bonds
    bool uniform_sign = true;
    bool jpos_uniform = false;          // sign when uniform: true = J > 0 (antiferromagnetic)
    bool open_x = false, open_y = false; // no bonds between columns W-1 and 0 / rows H-1 and 0 (all of them absent)
    std::vector<uint8_t> jright, jdown; // per site: 1 if that bond has J > 0 (empty when uniform)
};

Lattice2D recognise_lattice2d(const uint64_t *ea, const uint64_t *eb, const double *ej,
                              size_t n_edges, size_t nvars);

// adjacency in edge-list order (self-loops dropped, their J summed into self_energy)
struct Adjacency {
    std::vector<uint64_t> ptr; // nvars + 1
    std::vector<uint32_t> nbr;
    std::vector<double> w;
    double self_energy = 0.0;
};

Adjacency build_adjacency(const uint64_t *ea, const uint64_t *eb, const double *ej, size_t n_edges,
                          size_t nvars);

struct Colouring {
    std::vector<uint32_t> colour;     // per site
    uint32_t n_colours = 0;
    std::vector<uint64_t> class_base; // n_colours + 1, packed positions, classes padded to 256
    std::vector<uint64_t> pos;        // site -> packed position
    uint64_t n_pos = 0;
};

Colouring greedy_colouring(const Adjacency &A, size_t nvars);

// One parallel-tempering exchange round on the beta ladder.  Rung i (beta_i) holds
// replica slot perm[i]; round parity picks the pairs (i, i+1); swap iff
// u < exp((beta_i - beta_j)(E_i - E_j)), u from Philox keyed by (seed, round, i).  Swaps exchange the
// perm entries (temperatures move, configurations stay).  Returns the number of accepted swaps.
uint64_t pt_swap_round(uint64_t seed, uint64_t round, size_t n_rungs, const double *betas,
                       const double *slot_energy, uint32_t *perm);

// The ladder statistics of one exchange round (device twins: pt_swap_kernel and the exchange rounds of the strip
// kernel), called after pt_swap_round with the permutation before and after it and the energies it decided from.  Per rung:
// sum_e += E, sum_e2 += E * E of the slot that held it before the round (product and additions rounded separately); per pair of
// the round's parity: attempts, and accepts where the entries changed; n_rungs >= 2: the slot now at rung 0 completes a round trip
// if it was labelled DOWN (2) and becomes UP (1), the slot now at the last rung becomes DOWN, then every rung counts the label
// of the slot it now holds; *rounds += 1.  round_trips and labels are indexed by slot, the other arrays by rung (pairs: lower rung).
void pt_statistics_round(uint64_t round, size_t n_rungs, const uint32_t *perm_before, const uint32_t *perm_after, const double *slot_energy,
                         uint64_t *attempts, uint64_t *accepts, uint64_t *n_up, uint64_t *n_down, double *sum_e, double *sum_e2,
                         uint64_t *round_trips, uint8_t *labels, uint64_t *rounds);

// The source table of one population-annealing resampling (device twin: pa_kernels.hip).  Weights
// W[r] = floor(det_exp(-(dbeta (E[r] - E_ref))) 2^32) with E_ref = min E (dbeta >= 0) or max E, S = sum W, inclusive prefix sums C;
// offset u = mulhi64(U, S) with U the low 64 bits of Philox4x32-10({step lo, step hi, 0, "PARS"}, seed); new slot j copies the
// replica src[j] = the r with n C[r - 1] <= j S + u < n C[r] (systematic resampling; src is non-decreasing).  Returns S; n >= 1.
uint64_t pa_sources(uint64_t seed, uint64_t step, size_t n, const double *energies, double dbeta, uint32_t *src_out, double *eref_out);

// The step chooser of population annealing (device twin: the pa_choose_* kernels of pa_kernels.hip): the largest
// step k / 65536 of dbeta_max, k = 1 .. 65536, that a fixed 16-ary search finds with N(k) 2^32 >= t32 n S(k), where the weights are
// those of pa_sources for dbeta_k = double(k) * (dbeta_max 2^-16), E_ref = min E, S = sum W and N = sum min(S, n W) in 128 bits.
// Four rounds: the candidates lo + j width / 16, j = 1 .. 16 (15 after the first round), the leading ones that hold move lo; all 16
// of the first round: k = 65536.  k = max(lo, 1).  n in 1 .. 2^31, dbeta_max > 0, t32 in 1 .. 2^32, everything finite.
struct PaChoice {
    uint32_t k;
    double dbeta;
    uint64_t sum, num_lo, num_hi;
};
uint64_t pa_target32(double target); // ceil(target 2^32): the smallest 2^-32 fixed-point number that is not below target
PaChoice pa_choose_step(size_t n, const double *energies, double dbeta_max, uint64_t t32);
const char *pa_choose_refusal(double dbeta_max, double target); // why these arguments are refused, or nullptr

// ---- replica-packed real-coupling path: host halves of the spec ---------------------------
// Scales: F_i = |h_i| + sum_e |J_e|, Fmax = max F_i, med = the lower median nonzero |coupling or bias|;
// k = ilogb(min(Fmax, 64 med)) + 1 - 30 is the graph's quantum; site i quantises what it sees at k_i = max(k, ilogb(F_i) + 1 - 30)
// (dshift[i] = min(k_i - k, 31); > 0: a HEAVY site -- one pinning bias, one enormous bond): jq in ADJACENCY order (A.w's, each
// entry as seen from its row's site), hq per site.  eligible: degree <= 31, Fmax > 0, and every heavy site dominated by one
// term (4 max term >= 3 F_i: no cancellation among its large terms can make the coarser quantum matter).
// Energy levels (the ORIGINAL couplings, not the dynamics' rounded ones): k_energy = ilogb(Fmax) + 2 - 30,
// x ~ hi 2^k_energy + lo 2^(k_energy - 24); jhi / jlo in adjacency order (one value per bond), hhi / hlo per site.
constexpr int RJ_ENERGY_LO_BITS = 24;
struct RjQuant {
    bool eligible = false, heavy = false;
    int k = 0, k_energy = 0;
    uint32_t max_degree = 0;
    std::vector<int32_t> jq, hq, jhi, jlo, hhi, hlo;
    std::vector<uint8_t> dshift;
};
RjQuant rj_quantise(const Adjacency &A, size_t nvars, const double *biases);
// acceptance scale of beta: accept iff max(X >> shift, 0) <= (Lambda_q(u) * mant) >> 32
void rj_beta(double beta, int k, uint32_t *shift_out, uint32_t *mant_out);
// LT[i], i = 0 .. 2048: log2(1 + i/2048) in Q24, centred for linear interpolation (see oracle/ising_oracle.c engine E)
void rj_log_table(uint32_t *out);

// Items (replicas, pairs, replica groups, pair blocks) per batch of a non-local move whose labelling workspace takes
// words_per_item 32-bit words per item: as many as workspace_bytes hold, at least one, at most `items` and at most 32768 (a batch
// is the y dimension of one grid).  Internal to the library: not among its dynamic symbols.
__attribute__((visibility("hidden"))) size_t nonlocal_batch(size_t items, size_t words_per_item, size_t workspace_bytes);

// Non-local steps of a run call: the timesteps t in [t0, t0 + timesteps) with t % k == k - 1; none when k == 0.
// What a cluster series (S24) needs room for before the call enqueues anything.
uint64_t nonlocal_steps_in(uint64_t t0, uint64_t timesteps, uint64_t k);

// Site classes of the replica-packed families (device reader: overlap_class_kernels.hip).  site[n_pos]: the site of
// every position, PAD_SITE on padding; cls[n_tables][nvars]: a class below n_classes or CLASS_NONE per site.  Per table the
// classed positions are sorted by class (ascending position inside a class) into `order`, and the sorted list is cut into
// segments {table, class, first, count} -- `first` indexes `order`, count <= CLASS_SEGMENT_MAX, a segment never mixes classes or
// tables; an empty class has no segment.  sizes[n_tables][n_classes]: sites per class.  The caller has checked the class values.
constexpr uint32_t CLASS_NONE = 0xFFFFFFFFu;
constexpr uint32_t CLASS_SEGMENT_MAX = 1024; // positions one workgroup of ovl_pk_class_kernel counts
struct ClassSegments {
    std::vector<uint32_t> order;
    std::vector<uint32_t> seg; // four words per segment
    std::vector<uint64_t> sizes;
};
ClassSegments class_segments(const uint32_t *site, size_t n_pos, const uint32_t *cls, size_t nvars, size_t n_tables, size_t n_classes);

// The sample points of a measurement the step loop takes on a period (the recorder table of recorders.hip).
// A sample follows every timestep t > t0 with (t - t0) % every == 0.  A call repeated after a strip launch gave up
// (with_strip_retry) takes no sample twice: the samples up to replay_to were taken by the attempt that is repeated (last_t: the
// timestep of the last sample the step loop took).
struct Periodic {
    size_t every = 0; // 0 = off
    uint64_t t0 = 0, last_t = 0, replay_to = 0;
    uint64_t phase(uint64_t t) const { return (t - t0) % every; }
    // timesteps from t up to and including the next sample point (no bound while off)
    size_t stretch(uint64_t t) const { return every ? size_t(every - phase(t)) : std::numeric_limits<size_t>::max(); }
    bool due(uint64_t t) const { return every && phase(t) == 0 && t > replay_to; }
    uint64_t points(uint64_t t, uint64_t n) const { return (t - t0 + n) / every - (t - t0) / every; } // sample points in (t, t + n]
    void restart(uint64_t t) { t0 = t; last_t = 0; } // the sample points are counted from t
    // around the repeat of a call that started at timestep t: it skips the samples already taken
    void replay_since(uint64_t t) { replay_to = every && last_t > t ? last_t : 0; }
};

// The bookkeeping of the lag ring when samples_taken samples are in it, 1 <= n_lags: what the launch of sample number
// samples_taken is given, and what a read-out divides by.  live = min(samples_taken, n_lags) lags have a snapshot; the sample goes
// into write_slot = samples_taken mod n_lags.  slot_of_lag(0) = write_slot (where lag 0, the current configuration, goes),
// slot_of_lag(l) = the slot of the snapshot l samples back (autocorr_ring.hpp) for 1 <= l <= live, AUTOCORR_NO_SLOT beyond.
// count(l): the terms summed into lag l by the samples so far, max(0, samples_taken - l).  Nothing is allocated.
constexpr uint32_t AUTOCORR_NO_SLOT = 0xFFFFFFFFu;
struct AutocorrPlan {
    uint64_t samples_taken = 0;
    uint32_t n_lags = 1, live = 0, write_slot = 0;
    uint32_t slot_of_lag(uint32_t l) const { return l == 0 ? write_slot : l <= live ? acr_slot_of_lag(write_slot, l, n_lags) : AUTOCORR_NO_SLOT; }
    uint64_t count(uint32_t l) const { return samples_taken > l ? samples_taken - l : 0; }
};
AutocorrPlan autocorr_plan(uint64_t samples_taken, uint32_t n_lags);

// packed checkerboard planes of one replica -> W*H bytes in site order (16 bytes per SSE2 store)
void unpack_lattice(uint32_t W, uint32_t H, const uint32_t *words, uint8_t *spins);

} // namespace isingmc
