/*
 * isingmc.h -- C ABI of libisingmc.so, the MI355X (gfx950) classical Ising Metropolis engine.
 *
 * This is the drop-in boundary for the hot path of Renmusxd/PyIsingMonteCarlo: the reference's
 * pyo3 shell (src/lattice.rs, src/classicising.rs) drives one `qmc::classical::graph::GraphState`
 * per experiment from a rayon loop; a maintainer replaces that loop with the calls below
 * (INTEGRATION.md shows the `extern "C"` block).  Each entry point names the reference
 * interface it replaces.  Plain pointers and sizes only; the caller owns every host buffer; the
 * handles own all device memory.  Every function returns ISINGMC_OK or an error code and never
 * aborts the process (the reference aborts on engine errors: lattice.rs:206 + Cargo.toml:14);
 * isingmc_last_error() returns the message of the calling thread's last failure.
 *
 * There is NO CPU fallback: without a usable HIP device every device entry point fails with
 * ISINGMC_ERR_NO_DEVICE.  The isingmc_host_* helpers are pure host code and need no device.
 *
 * Hamiltonian: E = sum_edges J_ab s_a s_b - sum_i h_i s_i, s = +1 for True (README.md:45-46;
 * bias sign [UNVERIFIED]).
 */
#ifndef ISINGMC_H
#define ISINGMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISINGMC_ABI_VERSION 4

enum {
    ISINGMC_OK = 0,
    ISINGMC_ERR_INVALID = 1,   /* bad argument: maps to Python ValueError */
    ISINGMC_ERR_NO_DEVICE = 2, /* no HIP device / bad ordinal: RuntimeError */
    ISINGMC_ERR_HIP = 3,       /* a HIP runtime call failed: RuntimeError */
    ISINGMC_ERR_ALLOC = 4      /* host or device allocation failed: MemoryError */
};

/* graph kinds reported by isingmc_graph_info */
enum {
    ISINGMC_KIND_GENERAL = 0,  /* greedy-coloured CSR path, any edge list */
    ISINGMC_KIND_LATTICE2D = 1 /* W x H square lattice, uniform |J|, periodic or open, optional uniform field: checkerboard path */
};

/* isingmc_graph_create flags */
#define ISINGMC_FLAG_FORCE_GENERAL 1u /* skip the lattice recogniser (BASELINE config c5) */
/* Fix the kernel family from the GRAPH alone, never from the number of experiments: experiment k of a call then depends on
 * seed k only (lattice.rs:83-91, 198), i.e. run_monte_carlo(beta, T, R)[k] is the same for every R > k.  Without the flag the
 * faster family for the given R is chosen (small R on the f64 CSR kernels, large R replica-packed), and the two families are
 * different Markov chains for the same Hamiltonian. */
#define ISINGMC_FLAG_STABLE_PATH 2u

typedef struct isingmc_graph isingmc_graph;   /* edges + biases: the per-experiment adjacency that
                                                 GraphState::new builds (lattice.rs:199), built once */
typedef struct isingmc_states isingmc_states; /* R replicas = R x GraphState<SmallRng> on one device */

typedef struct {
    int32_t kind;        /* ISINGMC_KIND_* */
    int32_t device;      /* HIP device ordinal */
    uint64_t nvars;      /* max index + 1 (lattice.rs:51-55) */
    uint64_t n_edges;
    int32_t width;       /* LATTICE2D: W (columns), else 0 */
    int32_t height;      /* LATTICE2D: H (rows), else 0 */
    double jabs;         /* LATTICE2D: the common |J| */
    int32_t uniform_sign;/* LATTICE2D: 1 if every bond has the same sign */
    uint32_t n_colours;  /* independent sets per timestep (2 on the lattice path) */
    uint64_t state_words;/* 32-bit words of packed spin state per replica */
    int32_t fast_path;   /* LATTICE2D: 0 = periodic, no field; 1 = uniform field (set_global_bias, lattice.rs:129-131;
                            ClassicIsing longitudinal, classicising.rs:69); 2 = open boundaries;
                            3 = anisotropic (|J| of the horizontal bonds != |J| of the vertical ones);
                            4 = open boundaries and a field */
    int32_t open_x, open_y; /* LATTICE2D: no bonds between columns W-1 and 0 / rows H-1 and 0 */
    double field;        /* LATTICE2D: the uniform bias h of E = sum J s s - h sum s (0 without) */
    double jabs_y;       /* LATTICE2D: |J| of the vertical bonds (jabs is then the horizontal bonds'; equal unless fast_path == 3) */
    int32_t field_signs; /* LATTICE2D: 1 when the biases are +-field from site to site (sign planes), field = |h| then */
    int32_t packed_degree; /* GENERAL: d in 3..6 when the replica-packed path may use its one-degree kernel
                              (every site has d neighbours, every coupling the same size), else 0 */
    int32_t real_slots;    /* GENERAL: 4, 7, 11, 15, 23 or 31 when the replica-packed REAL-COUPLING path applies (any f64 couplings,
                              lattice.rs:46-50, and any site biases, lattice.rs:104-131; degree <= real_slots), else 0 */
    int32_t real_quantum_log2; /* that path's DYNAMICS compute with couplings rounded to multiples of 2^real_quantum_log2
                              (2^-30 of the largest |h_i| + sum_e |J_e|, never more than 2^-24 of the median term; heavy sites:
                              2^-30 of their own |h_i| + sum_e |J_e|) */
    int32_t real_energy_log2;  /* ... and its ENERGIES are those of the original couplings to within 2^(real_energy_log2 - 25)
                              per term (two exact integer levels; = Fmax 2^-54) */
    int32_t real_heavy_sites;  /* sites that quantise at a coarser scale of their own (pinned by a large bias, ...) */
    int32_t stable_path;       /* 1 when created with ISINGMC_FLAG_STABLE_PATH */
    int32_t packed_but_one_headers; /* one-degree packed kernel: (64-position block, slot) pairs that are one translation for every
                              lane but one (a lattice row wrapping around inside the block) -- served without a table read */
} isingmc_graph_info_t;

const char *isingmc_last_error(void);
int isingmc_abi_version(void);
/* The library recycles freed device blocks, pinned host blocks, streams and events between calls (a call of the reference's
 * API creates and drops its replicas; for small lattices hipMalloc / hipFree cost more than the timesteps).  This hands everything
 * that is idle back to the runtime; returns the number of bytes released.  (ISINGMC_NO_ALLOC_CACHE=1 disables the recycling.) */
size_t isingmc_release_cached_resources(void);
int isingmc_device_count(int *count);

/* ---- host-only helpers (no device) ------------------------------------------------------ */

/* lattice.rs:83-91 make_seeds: master SmallRng (seed_from_u64(seed_gen), or OS entropy when
 * has_seed == 0) -> one u64 per experiment. */
int isingmc_host_make_seeds(int has_seed, uint64_t seed_gen, size_t n, uint64_t *seeds_out);

/* lattice.rs:320-334 + 358-365 (and 406-420 + 445-451): sort the (t, beta) stops, default
 * [(0,1),(T,1)], pad to [0,T], and expand to one beta per timestep by linear interpolation.
 * compat_constant_beta != 0 reproduces the reference's behaviour (the interpolation index is a
 * captured constant, so beta is the last stop's beta for the whole run). */
int isingmc_host_expand_schedule(const uint64_t *stop_t, const double *stop_beta, size_t n_stops,
                                 size_t timesteps, int compat_constant_beta, double *betas_out);

/* Recogniser: is this edge list a W x H square lattice with ids y*W+x, every bond present once,
 * one |J| per direction, periodic or open (ALL wrap-around bonds of a direction absent) in each direction?
 * *is_lattice = 0 when not (then the general path is used), else 1 + 2 (open in x) + 4 (open in y)
 * + 8 (|J| of the horizontal bonds, returned in *jabs, differs from the vertical bonds'). */
int isingmc_host_recognise_lattice2d(const uint64_t *edge_a, const uint64_t *edge_b,
                                     const double *edge_j, size_t n_edges, size_t nvars,
                                     int *is_lattice, int *width, int *height, double *jabs,
                                     int *uniform_sign);

/* Greedy colouring used by the general path (sites in index order, smallest free colour). */
int isingmc_host_colour_graph(const uint64_t *edge_a, const uint64_t *edge_b, size_t n_edges,
                              size_t nvars, uint32_t *colours_out, uint32_t *n_colours_out);

/* One exchange round of the classical parallel-tempering ladder -- the classical counterpart of
 * TemperingContainer::parallel_tempering_step driven from tempering.rs:191-194 (quantum in the
 * reference).  Rung i has inverse temperature betas[i] and currently holds replica slot perm[i];
 * slot_energy[s] is that slot's energy (all-gathered across ranks by the caller).  Pairs (i, i+1)
 * with i of the round's parity are swapped with probability min(1, exp((b_i-b_j)(E_i-E_j))) using
 * a Philox stream keyed by (seed, round, i): every rank computes the same decisions from the same
 * inputs.  perm is updated in place; *swaps_out receives the number of accepted swaps. */
int isingmc_host_pt_swap_round(uint64_t seed, uint64_t round, size_t n_rungs, const double *betas,
                               const double *slot_energy, uint32_t *perm, uint64_t *swaps_out);

/* The ladder statistics of one exchange round (the rule is stated at isingmc_pt_set_statistics), the host twin of
 * what the exchange kernels keep on the device: called after isingmc_host_pt_swap_round with the round's number, the permutation
 * before and after it and the energies it decided from, on caller-held arrays: attempts / accepts uint64[n_rungs - 1] (may be
 * NULL for n_rungs < 2), n_up / n_down uint64[n_rungs], sum_e / sum_e2 double[n_rungs], round_trips uint64[n_rungs] and labels
 * uint8[n_rungs] by slot, *rounds. */
int isingmc_host_pt_statistics_round(uint64_t round, size_t n_rungs, const uint32_t *perm_before, const uint32_t *perm_after,
                                     const double *slot_energy, uint64_t *attempts, uint64_t *accepts, uint64_t *n_up,
                                     uint64_t *n_down, double *sum_e, double *sum_e2, uint64_t *round_trips, uint8_t *labels,
                                     uint64_t *rounds);

/* The source table of one population-annealing resampling, the host twin of what isingmc_pa_resample computes
 * on the device.  energies[n] are the replicas' energies (the f64 values of isingmc_get_energies), dbeta = beta_to - beta_from of
 * either sign.  E_ref = min E for dbeta >= 0, else max E; x[r] = -(dbeta * (E[r] - E_ref)), three separately rounded f64
 * operations; W[r] = floor(det_exp(x[r]) 2^32) as a 64-bit integer (the replica at E_ref has exactly 2^32); S = sum W and the
 * inclusive prefix sums C are exact integer sums.  One Philox4x32-10 call with counter {step lo, step hi, 0, "PARS"} and the key
 * (seed lo, seed hi) gives the 64-bit word U = (r[1] << 32) | r[0] and the offset u = the high 64 bits of U S.  New slot j takes
 * the configuration of old replica src_out[j] = the r with n C[r-1] <= j S + u < n C[r] (128-bit compare): systematic resampling,
 * src non-decreasing, replica r copied n_r times with |n_r - n W[r] / S| < 1.  *sum_out = S, *eref_out = E_ref (either may be
 * NULL).  ln(S / (n 2^32)) - dbeta E_ref estimates ln Z(beta_to) - ln Z(beta_from).  n in 1 .. 2^31, everything finite. */
int isingmc_host_pa_sources(uint64_t seed, uint64_t step, size_t n, const double *energies, double dbeta, uint32_t *src_out,
                            uint64_t *sum_out, double *eref_out);

/* The temperature step of a population-annealing schedule, chosen from the population itself, the host twin of
 * what isingmc_pa_choose_step computes on the device.  energies[n] as for isingmc_host_pa_sources; dbeta_max > 0 and finite; target
 * in (0, 1], taken as t32 = ceil(target 2^32).  Candidates k = 1 .. 65536 with dbeta_k = double(k) * (dbeta_max 2^-16), one rounded
 * multiplication.  Per candidate: W[r](k) = the weights of isingmc_host_pa_sources for dbeta_k (E_ref = min E), S(k) = sum W,
 * N(k) = sum_r min(S, n W[r]) as a 128-bit integer; the candidate HOLDS when N(k) 2^32 >= t32 n S(k) (128-bit compare), that is
 * when the overlap (1/n) sum_r min(1, tau_r) of the energy histograms at the two temperatures -- tau_r = n W[r] / S, the expected
 * number of copies of replica r -- is at least the target.  The search is fixed (the result is defined even where rounding makes
 * the predicate non-monotone): lo = 0, width = 65536; four rounds with step = width / 16 evaluate lo + j step for j = 1 .. 16
 * (first round) or 1 .. 15, j* = the number of leading candidates that hold, lo += j* step, width = step; j* = 16 in the first round
 * ends the search with k = 65536.  Result: k = max(lo, 1), dbeta_k, S(k) and N(k) = *num_hi_out 2^64 + *num_lo_out (any output may
 * be NULL).  A population of equal energies takes the whole dbeta_max; k >= 1 guarantees progress. */
int isingmc_host_pa_choose_step(size_t n, const double *energies, double dbeta_max, double target, uint32_t *k_out, double *dbeta_out,
                                uint64_t *sum_out, uint64_t *num_lo_out, uint64_t *num_hi_out);

/* The position lists of a class set on the replica-packed families, as isingmc_site_classes_create builds them
 * for the device.  site[n_pos]: the site at every position of the packed layout, 0xFFFFFFFF on padding; cls[n_tables][nvars]: a
 * class below n_classes or 0xFFFFFFFF (no class) per site.  Per table the classed, non-padding positions are sorted by class,
 * ascending inside a class, into order_out; the sorted list is cut into segments of at most 1024 positions, four words
 * {table, class, first, count} each in seg_out (`first` indexes order_out; a segment never mixes classes; an empty class has
 * none); tables after one another.  Capacities the caller provides: order_out n_tables * n_pos words, seg_out
 * 4 * n_tables * (n_classes + n_pos / 1024) words; *n_order_out / *n_seg_out: positions / segments written.
 * sizes_out[n_tables][n_classes]: sites per class (may be NULL).  Refuses what isingmc_site_classes_create refuses. */
int isingmc_host_class_segments(const uint32_t *site, size_t n_pos, const uint32_t *cls, size_t nvars, size_t n_tables, size_t n_classes,
                                uint32_t *order_out, size_t *n_order_out, uint32_t *seg_out, size_t *n_seg_out, uint64_t *sizes_out);

/* Host halves of the replica-packed REAL-COUPLING path -- what the device kernels are fed with, exposed
 * so that they can be checked without a GPU.  That path serves edge lists with couplings of several sizes
 * (lattice.rs:46-50 takes any f64) and arbitrary site biases (set_individual_bias / set_global_bias, lattice.rs:104-131)
 * on graphs of degree <= 31.  Scales: F_i = |h_i| + sum_e |J_e|, Fmax = max_i F_i, med = the lower median nonzero
 * |coupling or bias|; the graph's quantum is 2^k, k = ilogb(min(Fmax, 64 med)) + 1 - 30; site i quantises what it sees in units
 * of 2^(k + d_i), d_i = max(0, ilogb(F_i) + 1 - 30 - k) capped at 31 (d_i > 0: a heavy site, e.g. one pinned by a large bias).
 * jq_out: TWO values per input edge -- the bond as seen from edge_a[e] and from edge_b[e] (0, 0 for self-loops); hq_out and
 * dshift_out: one per site; *eligible_out: degree <= 31, Fmax > 0 and every heavy site dominated by one term
 * (4 max(|h_i|, max_e |J_e|) >= 3 F_i) -- else the f64 CSR path is used. */
int isingmc_host_rj_quantise(const uint64_t *edge_a, const uint64_t *edge_b, const double *edge_j, size_t n_edges,
                             size_t nvars, const double *biases, int32_t *jq_out, int32_t *hq_out, uint8_t *dshift_out,
                             int *k_out, int *eligible_out);
/* the energy of that path is the energy of the ORIGINAL couplings in two exact integer levels:
 * x ~ hi 2^kE + lo 2^(kE - 24), kE = ilogb(Fmax) + 2 - 30, |x - (hi 2^kE + lo 2^(kE-24))| <= Fmax 2^-54;
 * jhi_out / jlo_out per input edge (0 for self-loops), hhi_out / hlo_out per site */
int isingmc_host_rj_energy_levels(const uint64_t *edge_a, const uint64_t *edge_b, const double *edge_j, size_t n_edges,
                                  size_t nvars, const double *biases, int32_t *jhi_out, int32_t *jlo_out, int32_t *hhi_out,
                                  int32_t *hlo_out, int *k_energy_out);
/* acceptance scale of one inverse temperature: a flip of site i with half energy change X (units of 2^(k + d_i)) is accepted iff
 * max(X >> (*shift_out - m), 0) <= ((Lambda_q(u) * *mant_out) >> 32) >> (d_i - m), m = min(*shift_out, d_i), Lambda_q(u) = 32 - log2(u) in Q24 for the 32-bit uniform u */
int isingmc_host_rj_beta(double beta, int k, uint32_t *shift_out, uint32_t *mant_out);
/* the 2049 entries of the log2(1 + i/2048) table behind Lambda_q (Q24, centred for linear interpolation) */
int isingmc_host_rj_log_table(uint32_t *table_out);

/* ---- graph: replaces the adjacency half of GraphState::new (lattice.rs:199, classicising.rs:73)
 * edges as three parallel arrays (the Vec<((usize,usize),f64)> of lattice.rs:47); biases NULL
 * (all zero) or nvars doubles (lattice.rs:186-189).  device = HIP ordinal. */
int isingmc_graph_create(const uint64_t *edge_a, const uint64_t *edge_b, const double *edge_j,
                         size_t n_edges, size_t nvars, const double *biases, int device,
                         unsigned flags, isingmc_graph **graph_out);
int isingmc_graph_info(const isingmc_graph *graph, isingmc_graph_info_t *info_out);
void isingmc_graph_destroy(isingmc_graph *graph);
/* The kernel FAMILY a container of n_experiments created now would run on: 0 checkerboard lattice kernels, 1 f64 CSR kernels
 * (one replica per word set), 2 replica-packed bit-sliced, 3 replica-packed real-coupling.  Families 1-3 are different Markov
 * chains for the same Hamiltonian: on a general graph the results of experiment k depend on the number of experiments of the call
 * wherever this answer does (unless the graph was created with ISINGMC_FLAG_STABLE_PATH); isingmc_states_family: of a container. */
int isingmc_graph_family_for(const isingmc_graph *graph, size_t n_experiments, int *family_out);
int isingmc_states_family(const isingmc_states *states, int *family_out);

/* ---- states: replaces R x { SmallRng::seed_from_u64(seed); GraphState::new(..., rng);
 * set_state(initial) } (lattice.rs:198-203) and GraphState::new_with_state_and_rng
 * (classicising.rs:71).  seeds[r] keys replica r's Philox stream (results do not depend on which
 * device or in which batch a replica runs).  initial_state: NULL (random start) or nvars bytes
 * (nonzero = True) copied into every replica.  The graph must outlive the states. */
int isingmc_states_create(isingmc_graph *graph, size_t n_replicas, const uint64_t *seeds,
                          const uint8_t *initial_state, isingmc_states **states_out);
/* One shard of the same fan-out: experiments [first, first + count) of the n_total whose seeds are
 * all_seeds[n_total] (the zip of lattice.rs:192-197 cut into contiguous blocks, one per GPU).  Every
 * choice that shapes a trajectory is made from the GLOBAL experiment index and count, so the union of
 * the shards' results equals one unsharded call whatever the cut.  isingmc_states_create(g, n, seeds)
 * is the shard [0, n) of n. */
int isingmc_states_create_range(isingmc_graph *graph, size_t n_total, const uint64_t *all_seeds,
                                size_t first, size_t count, const uint8_t *initial_state,
                                isingmc_states **states_out);
/* ClassicIsing.add_graph (classicising.rs:62-79): append one replica. */
int isingmc_states_append(isingmc_states *states, uint64_t seed, const uint8_t *initial_state);
/* GraphState::set_state (lattice.rs:202) on one replica. */
int isingmc_states_set_state(isingmc_states *states, size_t replica, const uint8_t *state);
size_t isingmc_states_count(const isingmc_states *states);
void isingmc_states_destroy(isingmc_states *states);
/* One of the path / tuning switches of THIS container: `name` is the environment variable's name without the ISINGMC_ prefix
 * (e.g. "strip", "disable_resident", "pk_streams", "sample_slab_bytes"; case-insensitive).  Every switch is read from the
 * environment once, when a graph / a container is created -- never at call time -- so two containers of one process can differ.
 * The kernel FAMILY (force_real, disable_real, force_packed, disable_packed) is fixed at creation and cannot be changed here. */
int isingmc_states_set_option(isingmc_states *states, const char *name, long value);
/* The option "philox_rounds" (ISINGMC_PHILOX_ROUNDS, default 10) is the one switch that selects another trajectory: the rounds of
 * Philox4x32 in the draws of the Metropolis sweeps, 10 or 7.  It serves the periodic, field-free, one-|J| checkerboard lattices
 * (family 0 without a field, open boundaries or a second |J|) and there only the sweeps' plane and tie calls: initial
 * configurations, exchange decisions, Swendsen-Wang bonds, isoenergetic cluster moves and population-annealing offsets draw with
 * ten rounds whatever it says, so a container starts from the same configurations and a ladder decides its exchanges from the
 * same words at either value.  ISINGMC_ERR_INVALID, the value left as it was, for any value but 7 and 10 and for 7 on a container
 * of another family.  The generator keeps no state: the option may change between calls and holds for the calls planned after it.
 * From the environment, 7 is the default of the containers it serves and the others keep 10; a value that is no round count fails
 * the creation.  Philox4x32-7 is the fewest rounds with no reported BigCrush failure (Salmon et al., SC'11); 10 stays the default. */
int isingmc_states_philox_rounds(const isingmc_states *states, int *rounds_out); /* the rounds the container's sweeps draw with */
/* ... and the rounds a container created NOW on this graph would start with (the environment as it is; 10 where 7 is not served) */
int isingmc_graph_philox_rounds(const isingmc_graph *graph, int *rounds_out);

/* Per-replica inverse temperatures (parallel-tempering ladder; shaped after
 * LatticeTempering.add_graph(beta), tempering.rs:70-113).  NULL clears them.  While set, the
 * betas argument of isingmc_do_time_steps is ignored. */
int isingmc_states_set_betas(isingmc_states *states, const double *beta_per_replica);

/* replaces `for _ in 0..timesteps { gs.do_time_step(beta, None, None, None, only_basic) }`
 * (lattice.rs:204-207, 271-280, 358-368, 445-455; classicising.rs:97-109) for all replicas.
 * One timestep = one full sweep = nvars single-spin Metropolis attempts per replica.
 * Timestep k uses beta = betas[k * beta_stride] (stride 0: constant beta).
 * energies_per_step: NULL, or double[R][timesteps] receiving get_energy() after every timestep
 * (lattice.rs:454).  Blocking: returns after the device has finished. */
int isingmc_do_time_steps(isingmc_states *states, size_t timesteps, const double *betas,
                          size_t beta_stride, double *energies_per_step);
/* Same work, additionally reporting the device time of the sweep kernels (HIP events recorded on
 * the engine's stream around the launches) -- the measurement hook of bench.py. */
int isingmc_do_time_steps_timed(isingmc_states *states, size_t timesteps, const double *betas,
                                size_t beta_stride, float *device_ms_out);

/* GraphState::get_energy (lattice.rs:208, 284, 370; classicising.rs:171): double[R]. */
int isingmc_get_energies(isingmc_states *states, double *energies_out);
/* sum_i s_i per replica: int64[R] (the build's own observable for <|M|> parity). */
int isingmc_get_magnetisations(isingmc_states *states, int64_t *mags_out);
/* GraphState::get_state / state_ref (lattice.rs:209-211, 281-283): replica r's nvars spins as
 * bytes (1 = True) at states_out + r * replica_stride_bytes (stride >= nvars; lets the caller
 * write straight into a bool[R,S,N] array). */
int isingmc_get_states(isingmc_states *states, uint8_t *states_out, size_t replica_stride_bytes);
/* Raw packed device words of every replica (layout: DESIGN.md S2), uint32[R][state_words]. */
int isingmc_get_packed_states(isingmc_states *states, uint32_t *words_out);
/* The device words exactly as they lie in memory (synchronises): checkerboard containers uint32[count][state_words], the same
 * as isingmc_get_packed_states; replica-packed containers uint32[groups][positions] with replica s in bit s % 32 of group s / 32 --
 * padding positions and the bits of a last group that no replica owns included.  *n_words_out (may be NULL) receives the number
 * of words; words_out == NULL asks for that number alone. */
int isingmc_get_raw_state(isingmc_states *states, uint32_t *words_out, size_t *n_words_out);
/* Absolute timestep counter of the replicas (Philox counter word; persists across calls). */
uint64_t isingmc_states_timestep(const isingmc_states *states);
/* Sets that counter (t < 2^48): with the seeds, isingmc_states_set_state and this, a run that was stopped after t timesteps
 * resumes on exactly the trajectory it would have followed (the reference has no equivalent: its rng state is not exposed). */
int isingmc_states_set_timestep(isingmc_states *states, uint64_t t);

/* ---- Swendsen-Wang cluster updates (this build's own non-local move, no reference counterpart) ----
 * With k > 0 every timestep t with t % k == k - 1 (t = isingmc_states_timestep) is a cluster step instead of a Metropolis sweep:
 * bonds between satisfied neighbours are activated with probability 1 - exp(-2 beta |J|), every connected cluster is flipped with
 * probability 1/2.  It counts as one timestep in every call (per-step energies, sampling, schedules, isingmc_states_set_timestep).
 * Served: checkerboard lattice containers with fast_path == 0 (periodic, no field, one |J|) and one coupling sign, W H < 2^32 - 1,
 * no ladder attached; and replica-packed bit-sliced containers of any general graph (one |J|, no biases, degree <= 6,
 * any sign pattern: cubic, triangular, honeycomb, diluted lattices, random regular graphs), no ladder attached.  Everything else --
 * a general graph on the f64 CSR family (the packed family is chosen by size, by ISINGMC_FORCE_PACKED=1 or by
 * ISINGMC_FLAG_STABLE_PATH at creation), the real-coupling path -- returns ISINGMC_ERR_INVALID and leaves k as it was.  k = 0 (the
 * default) switches it off.
 * The workspace of a cluster step (8.4 bytes per site and replica; packed containers: 284 bytes per position and group of 32
 * replicas) is limited by the option "cluster_workspace_bytes" (isingmc_states_set_option; replicas -- whole groups of a packed
 * container -- are processed in batches that fit, at least one at a time; results do not depend on it). */
int isingmc_states_set_cluster_every(isingmc_states *states, size_t k);
int isingmc_states_cluster_every(const isingmc_states *states, size_t *k_out);
/* the last cluster step of every replica: number of clusters and size of the largest one, uint64[R] each (synchronises);
 * ISINGMC_ERR_INVALID before the first cluster step */
int isingmc_cluster_stats(isingmc_states *states, uint64_t *n_clusters_out, uint64_t *largest_out);

/* ---- Isoenergetic cluster moves between replica pairs (Houdayer 2001; no reference counterpart) ----
 * With k > 0 every timestep t with t % k == k - 1 is an isoenergetic cluster move instead of a Metropolis sweep: the replicas with
 * GLOBAL experiment indices (2 p, 2 p + 1) form pair p; the connected clusters of the sites where the two configurations differ
 * (overlap q = -1) are each flipped, in both replicas, with probability 1/2.  The move is rejection-free, conserves the sum of the
 * two energies exactly for any couplings and does not read beta: it is valid between replicas at the same temperature only, so
 * per-replica betas must be equal inside every pair.  A last replica without a partner is left unchanged (its timestep counts).
 * Served: checkerboard lattice containers with fast_path == 0 (periodic, no field, one |J|) of ANY sign pattern (ferromagnet,
 * antiferromagnet, +-J glass), W H < 2^32 - 1, and (S12) replica-packed containers of both families -- bit-sliced and
 * real-coupling: any graph, couplings and biases those paths run; the two replicas swap their spins on a cluster, which
 * conserves the sum of the two energies with fields too -- no ladder attached, Swendsen-Wang steps off, a shard that starts on an
 * even experiment index and does not end inside a pair; everything else (containers on the f64 CSR general-graph family among
 * it) returns ISINGMC_ERR_INVALID and leaves k as it was.  While it is on, isingmc_states_set_cluster_every(k > 0),
 * isingmc_pt_attach and unequal pair betas are refused.  k = 0 (the default) switches it off.  Workspace: that of a
 * Swendsen-Wang step per PAIR (packed containers: about 130 bytes per position and replica GROUP, batched by whole groups), under
 * the same option "cluster_workspace_bytes". */
int isingmc_states_set_icm_every(isingmc_states *states, size_t k);
int isingmc_states_icm_every(const isingmc_states *states, size_t *k_out);
/* the last isoenergetic cluster move of every pair: number of q = -1 clusters, size of the largest one and number of q = -1 sites n
 * (overlap of the pair: 1 - 2 n / N), uint64[count / 2] each (synchronises); ISINGMC_ERR_INVALID before the first such move */
int isingmc_icm_stats(isingmc_states *states, uint64_t *n_clusters_out, uint64_t *largest_out, uint64_t *minus_sites_out);

/* The isoenergetic cluster move of S9 between TWO containers of one graph handle: pair p = replica slots_a[p] of
 * `a` and replica slots_b[p] of `b`; the key of a's replica draws the flip bits, t = the containers' common timestep.  Both
 * timestep counters advance by one (the move is a timestep in place of a sweep) and energies a tempering measurement had cached
 * are dropped in both.  Enqueue only: a's stream waits for what b's stream holds so far, runs the move, and b's stream waits
 * for it; nothing waits on the host (except when the workspace, which stays with `a` under its option
 * "cluster_workspace_bytes", has to grow).
 *   slots_a / slots_b: uint32[n_pairs] in host memory, every slot at most once per table; per-replica betas set with
 *     isingmc_states_set_betas must be bitwise equal inside every pair (containers without per-replica betas: no requirement;
 *     with a ladder attached the caller pairs equal rungs: the betas live on the device).
 *   both NULL: both containers carry a tempering ladder of their own (isingmc_pt_attach with world size 1, slot offset 0, one
 *     slot per rung) over bitwise equal betas, n_pairs = the number of rungs, and pair r = (a's slot at rung r, b's slot at rung
 *     r): the kernels read the two permutations on the device.
 * Served: two checkerboard containers (S10), or two replica-packed containers of ONE family, bit-sliced or real-coupling
 * (DESIGN.md S13): there slot s is bit (first + s) % 32 of its replica group, the key of a's GLOBAL group and the global bit of
 * a's slot draw the flip bits, and slots in no pair -- the bits a container does not own included -- stay as they were.
 * Refused with ISINGMC_ERR_INVALID and a message (both containers stay as they were): a == b, two graph handles, a container
 * on the f64 CSR general-graph family, two containers on different replica-packed families, a checkerboard lattice
 * isingmc_states_set_icm_every does not accept (fields, open boundaries, anisotropic couplings, W H >= 2^32 - 1), unequal
 * timesteps, Swendsen-Wang steps or isoenergetic cluster moves switched on inside either container, unequal
 * pair betas, slots out of range or used twice, the NULL form without two matching ladders. */
int isingmc_icm_between(isingmc_states *a, isingmc_states *b, const uint32_t *slots_a, const uint32_t *slots_b, size_t n_pairs);
/* the last isingmc_icm_between call with `a` as its first container, per pair in the order of the call: as isingmc_icm_stats,
 * uint64[n_pairs] each with n_pairs that of the call (synchronises) */
int isingmc_icm_between_stats(isingmc_states *a, uint64_t *n_clusters_out, uint64_t *largest_out, uint64_t *minus_sites_out, size_t n_pairs);

/* ---- Spin and link overlaps between replica pairs (no reference counterpart) ----
 * Exact integers of the configurations as they are, counted on the device; for pair p of configurations (x, y) of one graph
 *   spin_out[p] = sum_i s_i^x s_i^y                          over the nvars sites (sites in no edge count like any other)
 *   link_out[p] = sum_e s_{a_e}^x s_{b_e}^x s_{a_e}^y s_{b_e}^y   one term per entry e of the edge list given at graph creation:
 *     entries with zero coupling are included, duplicated entries are separate terms, and an entry with a_e == b_e (graph
 *     creation accepts it and folds its J into a constant of the energy) is the constant term +1.
 * The overlaps are q = spin / nvars and q_l = link / n_edges; no coupling and no bias is read.  int64[n_pairs] each;
 * link_out == NULL skips all bond work, spin_out may not be NULL.
 *   b == NULL or b == a: pairs inside one container.  Both tables NULL: the pairing of the isoenergetic moves -- the replicas with
 *     GLOBAL experiment indices (2 p, 2 p + 1) form pair p, n_pairs must be count / 2, a last replica without a partner is left
 *     out; a shard that starts at an odd experiment index is refused.
 *   two containers, both tables NULL: pair p = (slot p of a, slot p of b), n_pairs <= the smaller count.
 *   slots_a / slots_b: uint32[n_pairs] in host memory, pair p = (slot slots_a[p] of a, slot slots_b[p] of b); any slot below its
 *     container's count, any number of times; a pair (r, r) is legal (spin = nvars, link = n_edges).
 * The call synchronises.  It writes no configuration, consumes no random number and leaves the timestep counters alone; it asks
 * for neither equal betas nor equal timesteps nor a cluster period, and works with a tempering ladder attached.  Workspace: 16
 * bytes per pair; the tabled form on replica-packed containers also gathers 4 bytes per position and block of 32 pairs, batched
 * under a's option "cluster_workspace_bytes".
 * Served: checkerboard lattice containers with fast_path == 0 (periodic, no field, one |J|) of any sign pattern, and
 * replica-packed containers of both families.  Refused with ISINGMC_ERR_INVALID and a message: the f64 CSR general-graph family;
 * lattices with a field, open boundaries or anisotropic couplings; two containers of different graph handles or kernel families;
 * a slot at or beyond its container's count; n_pairs == 0; one table without the other. */
int isingmc_overlaps(isingmc_states *a, isingmc_states *b, const uint32_t *slots_a, const uint32_t *slots_b, size_t n_pairs,
                     int64_t *spin_out, int64_t *link_out);

/* ---- Spin overlaps resolved by a class label per site (no reference counterpart) ----
 * A class table gives every site i < nvars a class cls[i] in 0 .. n_classes - 1, or ISINGMC_NO_CLASS ("counted nowhere"); a class
 * set is n_tables such tables over one graph.  For pair p of configurations (x, y)
 *   out[p][t][c] = sum over the sites i with cls[t][i] == c of s_i^x s_i^y          int64[n_pairs][n_tables][n_classes]
 * exact integers, counted on the device.  Sites in no edge count like any other, an empty class gives 0, and for a table without
 * ISINGMC_NO_CLASS the sum over c is spin_out[p] of isingmc_overlaps.  With the plane at coordinate x of a lattice as class x the
 * result is the overlap profile Q_x whose Fourier transform gives the wave-vector-dependent spin-glass susceptibility along
 * that axis (pyisingmontecarlo_amd/correlation.py); sublattices give staggered overlaps, a marked region a window overlap.
 * isingmc_site_classes_create rearranges the tables into the layouts the kernels read and keeps them on the graph's device: a
 * measurement is repeated thousands of times during a run.  cls: uint32[n_tables][nvars] in host memory, in the site numbering
 * of the edge list.  Limits, each refused with ISINGMC_ERR_INVALID and a message: 1 <= n_tables <= 8; 1 <= n_classes <= 4096;
 * n_tables * n_classes <= 8192 (the checkerboard kernel's histogram: 32 KiB of LDS); a class value >= n_classes that is not
 * ISINGMC_NO_CLASS.  A handle serves the graph it was made for and is destroyed before it; destroy accepts NULL.
 * isingmc_site_classes_sizes: the number of sites of every class, uint64[n_tables][n_classes] (the result of a pair (r, r)).
 * isingmc_overlaps_by_class: a, b, slots_a, slots_b and n_pairs choose the pairs exactly as in isingmc_overlaps, with the same
 * validation and messages, and the same containers are served and refused.  It also refuses a handle made for another graph and
 * NULL classes or out.  The call synchronises.  It writes no configuration, consumes no random number and leaves the timestep
 * counters alone.  Workspace: 8 bytes per (pair, table, class), and on replica-packed containers with slot tables the gather of
 * isingmc_overlaps; the pairs are batched under a's option "cluster_workspace_bytes".  On replica-packed containers a class costs
 * at least one workgroup per 32 replicas, however few sites it has. */
#define ISINGMC_NO_CLASS 0xFFFFFFFFu
typedef struct isingmc_site_classes isingmc_site_classes;
int isingmc_site_classes_create(isingmc_graph *graph, const uint32_t *cls, size_t n_tables, size_t n_classes, isingmc_site_classes **out);
int isingmc_site_classes_destroy(isingmc_site_classes *classes);
int isingmc_site_classes_sizes(const isingmc_site_classes *classes, uint64_t *sizes_out);
int isingmc_overlaps_by_class(isingmc_states *a, isingmc_states *b, const uint32_t *slots_a, const uint32_t *slots_b, size_t n_pairs,
                              const isingmc_site_classes *classes, int64_t *out);

/* ---- The overlap series: overlaps per sample, logged on the device (no reference counterpart) ----
 * A device-resident log with one row per sample.  A record appends a row without the host waiting for anything; the log is read
 * once, afterwards.  A row is int64[n_pairs][1 + link + n_tables * n_classes]: for pair p the spin overlap, with
 * ISINGMC_SERIES_LINK the link overlap, and with a class set out[p][t][c] -- the exact integers spin_out, link_out and out of
 * isingmc_overlaps and isingmc_overlaps_by_class, by their conventions (zero couplings, duplicated entries and entries a_e == b_e
 * included).  The log holds `capacity` rows in one device block of the series, at most the option "overlap_series_bytes" of `a`
 * (isingmc_states_set_option; ISINGMC_OVERLAP_SERIES_BYTES, default 1 GiB); the host keeps the timestep of every row (a's counter
 * when the record was enqueued) and the row count.
 * isingmc_overlap_series_create: the containers served and refused are those of isingmc_overlaps, with its messages; b == NULL:
 *   pairs inside `a`.  classes may be NULL.  With ISINGMC_SERIES_BY_RUNG both containers carry a whole tempering ladder over
 *   bitwise equal betas (the condition of the table-free form of isingmc_icm_between), n_pairs is the number of rungs and pair r =
 *   (a's slot at rung r, b's slot at rung r), the permutations read on the device when the record runs.
 * isingmc_overlap_series_record: one row for the configurations as they are, enqueue only.  slots_a / slots_b choose the pairs as
 *   in isingmc_overlaps (both NULL: the pairs (2 p, 2 p + 1) of one container, (slot p, slot p) of two; n_pairs as given at
 *   creation); a BY_RUNG series takes no tables.  The tables are copied before the call returns.  a's stream waits for what b's
 *   stream holds, and b's stream for the record.  A full log refuses with ISINGMC_ERR_INVALID: nothing is enqueued, the rows stay.
 * isingmc_overlap_series_set_every: every > 0: from now on (t0 = a's timestep) a record without tables follows every timestep t
 *   with (t - t0) % every == 0, whatever kind of timestep it is, inside isingmc_do_time_steps*, isingmc_run_sampling and
 *   isingmc_run_sampling_moments; 0 switches it off and keeps the rows.  Only for a series inside one container (b == NULL,
 *   n_pairs = count / 2, no ISINGMC_SERIES_BY_RUNG), one such series per container.  isingmc_states_set_timestep re-bases t0;
 *   a run call whose rows would not fit fails before it enqueues anything; isingmc_states_append, isingmc_pa_run and
 *   isingmc_pa_resample are refused while it is on.
 * isingmc_overlap_series_count: rows held and the capacity (either pointer may be NULL).
 * isingmc_overlap_series_get: waits for a's stream, then copies the rows [first, first + n): timesteps_out[n],
 *   spin_out[n][n_pairs], link_out[n][n_pairs], class_out[n][n_pairs][n_tables][n_classes]; any pointer may be NULL.  Changes nothing.
 * isingmc_overlap_series_reset: the row count back to 0 (enqueue only); the period stays.
 * A series is destroyed before its containers and its class set; isingmc_pt_detach is refused on a container with a live BY_RUNG
 * series. */
typedef struct isingmc_overlap_series isingmc_overlap_series;
#define ISINGMC_SERIES_LINK 1u    /* also the link overlap */
#define ISINGMC_SERIES_BY_RUNG 2u /* pair r = (a's slot at rung r, b's slot at rung r), permutations read on the device */
int isingmc_overlap_series_create(isingmc_states *a, isingmc_states *b, size_t n_pairs, const isingmc_site_classes *classes,
                                  unsigned flags, size_t capacity, isingmc_overlap_series **out);
int isingmc_overlap_series_record(isingmc_overlap_series *s, const uint32_t *slots_a, const uint32_t *slots_b);
int isingmc_overlap_series_set_every(isingmc_overlap_series *s, size_t every);
int isingmc_overlap_series_count(const isingmc_overlap_series *s, size_t *n_out, size_t *capacity_out);
int isingmc_overlap_series_get(isingmc_overlap_series *s, size_t first, size_t n, uint64_t *timesteps_out,
                               int64_t *spin_out, int64_t *link_out, int64_t *class_out);
int isingmc_overlap_series_reset(isingmc_overlap_series *s);
int isingmc_overlap_series_destroy(isingmc_overlap_series *s);

/* ---- The observable series: energy and magnetisation per sample, logged on the device (no reference counterpart) ----
 * The sibling of the overlap series for the observables of ONE container `a`: a device-resident log with one row per sample.  A
 * record appends a row without the host waiting for anything; the log is read once, afterwards.  A series has n_columns = count
 * columns: the replicas in slot order, or with ISINGMC_OBS_BY_RUNG the rungs in ladder order -- column i is then the slot that holds
 * rung i when the record runs; the permutation is read on the device, behind the timestep and before any exchange round that follows.
 * A row holds, per column,
 *   energy         f64, bit for bit the value isingmc_get_energies would return for that configuration at that moment
 *   magnetisation  int64, sum_i s_i, as isingmc_get_magnetisations
 *   by_class[t][c] with a class set: int64, the sum of s_i over the sites of class c of table t.  ISINGMC_NO_CLASS sites count
 *                  nowhere, an empty class gives 0, a table without ISINGMC_NO_CLASS adds up to the magnetisation; padding positions,
 *                  bits a packed group does not own and replicas beyond count never count.
 * A record consumes no random number and writes no configuration; it counts into a block the series owns and leaves the timestep
 * counters, the container's measurement scratch and whatever the ladder's next exchange round decides from exactly as they were: an
 * exchange round that follows a record takes the same decisions as without it.  The log holds `capacity` rows in one device block of
 * the series, at most the option "observable_series_bytes" of `a` (isingmc_states_set_option; ISINGMC_OBSERVABLE_SERIES_BYTES,
 * default 1 GiB); the host keeps the timestep of every row (a's counter when the record was enqueued) and the row count.
 * isingmc_observable_series_create: served are exactly the containers with a device-side energy array -- periodic, field-free,
 *   isotropic checkerboard lattices (fast_path == 0) and both replica-packed families, shards of a larger set of experiments
 *   included.  ISINGMC_ERR_INVALID, the container unchanged: the f64 CSR family; lattices with field, open boundary or anisotropy;
 *   unknown flags; neither ISINGMC_OBS_ENERGY nor ISINGMC_OBS_MAGNETISATION nor a class set; capacity == 0; a class set of another
 *   graph; a log beyond the byte budget.  ISINGMC_OBS_BY_RUNG needs the whole ladder on the container (world size 1, count ==
 *   n_rungs, slot offset 0); without it an attached ladder is allowed and the columns are slots.
 * isingmc_observable_series_record: one row for the configurations as they are, enqueue only.  A full log refuses with
 *   ISINGMC_ERR_INVALID: nothing is enqueued, the rows stay.
 * isingmc_observable_series_set_every: every > 0: from now on (t0 = a's timestep) a record follows every timestep t with
 *   (t - t0) % every == 0, whatever kind of timestep it is, inside isingmc_do_time_steps*, isingmc_run_sampling,
 *   isingmc_run_sampling_moments and therefore isingmc_pt_time_steps; isingmc_pt_run takes one launch per round while the period is
 *   on (same decisions, same results), and a series by rung takes its row behind an isingmc_icm_between move whose timestep is a
 *   sample point.  0 switches it off and keeps the rows.  One such series per container.  isingmc_states_set_timestep re-bases t0; a
 *   run call whose rows would not fit fails before it enqueues anything -- isingmc_pt_run counts the rows of its whole call before
 *   its first round, and isingmc_icm_between the row behind the move before its launches; isingmc_states_append, isingmc_pa_run
 *   and isingmc_pa_resample are refused while it is on.
 * isingmc_observable_series_count: rows held and the capacity (either pointer may be NULL).
 * isingmc_observable_series_get: waits once for a's stream, then copies the rows [first, first + n): timesteps_out[n],
 *   energy_out[n][n_columns], magnetisation_out[n][n_columns], class_out[n][n_columns][n_tables][n_classes]; any pointer may be NULL;
 *   asking for a part the series does not hold is refused.  Changes nothing.
 * isingmc_observable_series_reset: the row count back to 0 (enqueue only); the period stays.
 * A series is destroyed before its container and its class set; isingmc_pt_detach is refused on a container with a live BY_RUNG
 * series. */
typedef struct isingmc_observable_series isingmc_observable_series;
#define ISINGMC_OBS_ENERGY 1u        /* the energy of every column */
#define ISINGMC_OBS_MAGNETISATION 2u /* the magnetisation of every column */
#define ISINGMC_OBS_BY_RUNG 4u       /* column i = the slot at rung i, the permutation read on the device */
int isingmc_observable_series_create(isingmc_states *a, const isingmc_site_classes *classes, unsigned flags, size_t capacity,
                                     isingmc_observable_series **out);
int isingmc_observable_series_record(isingmc_observable_series *s);
int isingmc_observable_series_set_every(isingmc_observable_series *s, size_t every);
int isingmc_observable_series_count(const isingmc_observable_series *s, size_t *n_out, size_t *capacity_out);
int isingmc_observable_series_get(isingmc_observable_series *s, size_t first, size_t n, uint64_t *timesteps_out, double *energy_out,
                                  int64_t *magnetisation_out, int64_t *class_out);
int isingmc_observable_series_reset(isingmc_observable_series *s);
int isingmc_observable_series_destroy(isingmc_observable_series *s);

/* ---- The cluster series: declared in isingmc_cluster_series.h, which the end of this header includes ---- */
/* The counting rule of the room check, without a device: *steps_out = the timesteps t in [t0, t0 + timesteps) with t % k == k - 1
 * (0 when k == 0). */
int isingmc_host_nonlocal_steps(uint64_t t0, size_t timesteps, size_t k, uint64_t *steps_out);

/* ---- each replica's lowest-energy configuration, kept on the device (no reference counterpart) ----
 * A container may keep, per replica, the lowest energy its configuration has had at an UPDATE, the timestep of that update and
 * the configuration itself.  An update measures the f64 energies of isingmc_get_energies on the device and, for every replica
 * with e < record (strictly: ties keep the earliest update; records start at +inf), sets record = e, timestep = t and copies
 * the replica's configuration into a second state buffer.  Nothing crosses the bus until isingmc_best_get.
 * isingmc_states_set_track_best(states, every): every = 0 (the default) is off; every = k > 0: inside isingmc_do_time_steps*,
 * the calls built on it (isingmc_pt_time_steps, isingmc_pa_run) and isingmc_run_sampling an update follows every timestep after
 * which t % k == 0.  The calls are cut into stretches at those timesteps; no configuration, energy or timestep they produce
 * changes.  While tracking is on, isingmc_pt_measure also serves the records from the energies it has just written (rounds
 * that would run inside one persistent launch take one launch per round, as with the option pt_in_kernel = 0),
 * isingmc_pa_resample does so before its gather, and isingmc_pa_run adds one update after its last sweeps.  Records belong to
 * the SLOT: neither a ladder's permutation nor a resampling moves them.  isingmc_states_set_state leaves them alone.
 * Memory: a second state buffer as large as the state plus 28 bytes per replica, allocated when tracking is first switched on
 * (or by the first isingmc_best_update) and freed with the container.
 * Served: checkerboard lattice containers with fast_path == 0 and both replica-packed families (the containers with a device-side
 * energy array).  Refused with ISINGMC_ERR_INVALID and a message, the container unchanged: the f64 CSR general-graph family;
 * lattices with a field, open boundaries or anisotropic couplings; isingmc_states_append while tracking is on. */
int isingmc_states_set_track_best(isingmc_states *states, size_t every);
int isingmc_states_track_best(const isingmc_states *states, size_t *every_out);
/* enqueue only: one update at the container's current timestep, whatever the period */
int isingmc_best_update(isingmc_states *states);
/* synchronises.  energies_out: double[count] (+inf where no update has happened); states_out: one byte per spin as
 * isingmc_get_states, taken from the second buffer (all zero where no update has happened); timesteps_out: uint64[count];
 * *improvements_out: how often any record has been set since the last reset.  Any pointer may be NULL. */
int isingmc_best_get(isingmc_states *states, double *energies_out, uint8_t *states_out, size_t replica_stride_bytes,
                     uint64_t *timesteps_out, uint64_t *improvements_out);
/* the second buffer's words as they lie in memory, as isingmc_get_raw_state (padding positions and the bits of a packed group
 * this container does not own hold no defined value) */
int isingmc_best_raw_state(isingmc_states *states, uint32_t *words_out, size_t *n_words_out);
/* records back to +inf, timesteps and the improvement count to 0; the second buffer keeps its words */
int isingmc_best_reset(isingmc_states *states);

/* ---- per-site spin sums and per-bond sums over the samples of a run (the classical counterpart of
 * run_quantum_monte_carlo_and_measure_spins) ----
 * Thermal averages resolved per site without a configuration leaving the device: the local magnetisations <s_i> and the bond
 * correlations <s_a s_b> as exact integer sums, True = +1 as in isingmc_get_states.  n = the samples taken so far.
 *   summed mode (flags 0):         site[i] = sum over samples and over the container's replicas of s_i, int64[nvars]; with
 *                                  ISINGMC_MOMENTS_BONDS also bond[e] = that sum of s_a s_b for entry e of the edge list given at
 *                                  graph creation, int64[n_edges], by the conventions of link_out of isingmc_overlaps: zero
 *                                  couplings count, duplicated entries are separate, an entry a_e == b_e adds +1 per sample and replica
 *   ISINGMC_MOMENTS_PER_REPLICA:   site[r][i] = sum over the samples of replica r of s_i, int64[count][nvars]; no bond sums
 *   ISINGMC_MOMENTS_PER_RUNG:       a container with a tempering ladder attached: site[i][v] = sum over the samples of
 *                                  s_v of the configuration that held rung i when the sample was taken, int64[n_rungs][nvars], i in
 *                                  ladder order; no bond sums.  A sample uses the permutation as it stands on the stream behind its
 *                                  timestep, before any exchange round that follows: a configuration counts at the beta it was just
 *                                  swept at.  The kernel reads the permutation on the device; nothing waits on the host.  Samples are
 *                                  taken inside isingmc_pt_time_steps, isingmc_pt_run (one launch per round while it is on, with the
 *                                  same decisions and results), isingmc_do_time_steps* and isingmc_icm_between (the move is timestep
 *                                  t of both containers; each one with this mode on takes its sample behind it).  Memory and limits
 *                                  are those of the per-replica mode.  Accepted only with the whole ladder on the container (world
 *                                  size 1, count == n_rungs, slot_offset 0); the order is isingmc_pt_attach, then this.
 * Sites in no edge count like any other; padding positions of a packed container, the bits of a packed group the container does
 * not own and replicas beyond count never count.
 * every > 0 records t0 = the current timestep; from then on, inside isingmc_do_time_steps* and isingmc_run_sampling, a sample of
 * all replicas follows every timestep t > t0 with (t - t0) % every == 0, whatever kind of timestep it is (sweep, Swendsen-Wang
 * step, isoenergetic move): the stretch of Metropolis sweeps is cut there and the sample is enqueued behind it.  No
 * configuration, energy, random number or timestep of the run changes.  every == 0 (the default) switches accumulation off and
 * keeps the sums; switching it on again with the same flags goes on counting, with other flags (or another replica count, or
 * another value of the option moments_planes) the sums start from zero.  isingmc_states_set_timestep while it is on re-bases t0.
 * Memory: summed mode 256 bytes per state word (768 with bonds) on a lattice, 8 bytes per position and 16 per edge entry on a packed
 * container.  Per-replica mode keeps K time planes of the state's own size (the option moments_planes, 1 .. 16, default 8; one
 * sample adds the state into them, and every 2^K - 1 samples they are flushed) plus 32-bit totals of 32 times the state's size, so a
 * replica holds at most 2^32 - 1 samples.  The option moments_bytes (default 4 GiB) bounds all of it.
 * Served: exactly the containers isingmc_overlaps serves -- periodic field-free checkerboard lattices of any sign pattern and
 * both replica-packed families.  Refused with ISINGMC_ERR_INVALID and a message, the container unchanged: the f64 CSR family;
 * a tempering ladder attached unless the sums are per rung (and isingmc_pt_attach while accumulation is on: a slot changes its
 * temperature); isingmc_pa_run, isingmc_pa_resample and isingmc_states_append while it is on; ISINGMC_MOMENTS_BONDS together with
 * ISINGMC_MOMENTS_PER_REPLICA; sums larger than moments_bytes; ISINGMC_MOMENTS_PER_RUNG without a ladder attached, on a shard of a
 * larger ladder, together with either other flag, or in isingmc_run_sampling_moments (it runs no exchange rounds); isingmc_pt_detach
 * while sums per rung are switched on. */
#define ISINGMC_MOMENTS_PER_REPLICA 1u
#define ISINGMC_MOMENTS_BONDS 2u
#define ISINGMC_MOMENTS_PER_RUNG 4u
int isingmc_states_set_moments_every(isingmc_states *states, size_t every, unsigned flags);
int isingmc_states_moments_every(const isingmc_states *states, size_t *every_out, unsigned *flags_out);
/* enqueue only: one sample at the container's current timestep, whatever the period (never switched on: summed mode, sites alone) */
int isingmc_moments_accumulate(isingmc_states *states);
/* synchronises and flushes the time planes.  *n_samples_out = n; site_out / bond_out as above, in the site numbering and edge
 * order of graph creation.  Any pointer may be NULL; bond_out needs ISINGMC_MOMENTS_BONDS. */
int isingmc_moments_get(isingmc_states *states, uint64_t *n_samples_out, int64_t *site_out, int64_t *bond_out);
/* sums and n back to zero; the setting stays */
int isingmc_moments_reset(isingmc_states *states);
/* The loop of isingmc_run_sampling with the samples summed instead of copied out: the sums are zeroed, then
 *   thermalization x do_time_step(beta);  n_samples x { sampling_freq x do_time_step(beta);  one sample }
 * is enqueued back to back and the host waits once, for energies_out: double[count], the energies of the final configurations
 * (NULL allowed).  Accumulation is off on entry and off again on return; isingmc_moments_get reads the sums.  beta is ignored
 * while per-replica betas are set.  Same trajectory and same samples as isingmc_run_sampling with these arguments. */
int isingmc_run_sampling_moments(isingmc_states *states, double beta, size_t thermalization, size_t sampling_freq,
                                 size_t n_samples, unsigned flags, double *energies_out);

/* ---- spin autocorrelation over time lags, measured on the device ("the lag ring"; the classical counterpart of
 * lattice.rs:628 run_quantum_monte_carlo_and_measure_variable_autocorrelation) ----
 * A lag ring of a container holds L = n_lags snapshots of its configurations in the state buffer's own layout and R x (L + 1) 64-bit
 * sums.  Samples are numbered j = 0, 1, ... since creation or the last reset.  Sample j adds, for every replica r and every lag
 * l = 1 .. min(j, L), D_r(l) = #{sites i : s_i(now) != s_i(at sample j - l)} to diff[r][l], and then stores the current
 * configuration as snapshot j mod L (the slot that held lag L, the oldest).  diff[r][0] stays 0; lag l has
 * counts[l] = max(0, samples - l) terms, and C_r(l) = 1 - 2 diff[r][l] / (nvars counts[l]).  Exact integers, independent of the
 * order of execution; only real sites of owned replicas count.  A sample is ONE launch on the container's stream: nothing is waited
 * for, no random number is consumed, no configuration, energy or timestep changes.
 * isingmc_autocorr_create: served are the containers isingmc_overlaps serves -- periodic, field-free checkerboard lattices (any sign
 *   pattern) and both replica-packed families, shards included.  Refused with ISINGMC_ERR_INVALID before anything is allocated: the
 *   f64 CSR family; fields, open boundaries, anisotropy; a tempering ladder attached (and isingmc_pt_attach while a ring lives: a slot
 *   changes its temperature); n_lags outside 1 .. 256; flags != 0; a second ring on one container; a ring (snapshots + sums) larger
 *   than the option "autocorr_bytes" (isingmc_states_set_option; ISINGMC_AUTOCORR_BYTES, default 4 GiB).  While a ring lives,
 *   isingmc_states_append, isingmc_pa_run and isingmc_pa_resample are refused.
 * isingmc_autocorr_set_every: every > 0: from now on (t0 = the container's timestep) a sample follows every timestep t with
 *   (t - t0) % every == 0, whatever kind of timestep it is (Metropolis sweep, Swendsen-Wang step, isoenergetic move), inside
 *   isingmc_do_time_steps*, isingmc_run_sampling and isingmc_run_sampling_moments; 0 switches the period off, ring and sums stay.
 *   isingmc_states_set_timestep re-bases t0; the sample number goes on.
 * isingmc_autocorr_sample: one sample now, enqueue only.
 * isingmc_autocorr_count: samples taken since creation or the last reset, and L (either pointer may be NULL); no device access.
 * isingmc_autocorr_get: waits once for the container's stream; counts_out: uint64[L + 1], diff_out: uint64[R][L + 1] (either may
 *   be NULL).  Changes nothing.
 * isingmc_autocorr_reset: sums and sample number to 0 (enqueue only); the period stays.
 * isingmc_autocorr_destroy: waits for the container's stream and frees the ring; the container takes a new one afterwards.  The
 *   ring must be destroyed before its container.
 * isingmc_run_sampling_autocorr: the loop of isingmc_run_sampling with the samples taken by the ring instead of copied out: the ring
 *   is reset, then  thermalization x do_time_step(beta);  n_samples x { sampling_freq x do_time_step(beta);  one sample }  is enqueued
 *   back to back and the host waits once, for energies_out: double[count] (NULL allowed).  site_sums != 0: the per-replica site sums
 *   (ISINGMC_MOMENTS_PER_REPLICA, zeroed first) take the same samples; isingmc_moments_get reads them, and sums beyond the option
 *   moments_bytes refuse the call.  The ring's period (and with site_sums the sums') must be off on entry and is off on return.
 * isingmc_host_autocorr_plan: the ring's bookkeeping without a device, as the launch of sample number samples_taken uses it:
 *   slot_of_lag_out: uint32[L + 1] -- [0] = the slot the sample is stored in, [l] = the slot of the snapshot l samples back for
 *   l = 1 .. *live_lags_out = min(samples_taken, L), 0xFFFFFFFF beyond; *write_slot_out = samples_taken mod L; counts_out:
 *   uint64[L + 1] = max(0, samples_taken - l), the terms in lag l after samples_taken samples.  Any pointer may be NULL. */
typedef struct isingmc_autocorr isingmc_autocorr;
int isingmc_autocorr_create(isingmc_states *states, size_t n_lags, unsigned flags, isingmc_autocorr **out);
int isingmc_autocorr_set_every(isingmc_autocorr *ac, size_t every);
int isingmc_autocorr_sample(isingmc_autocorr *ac);
int isingmc_autocorr_count(const isingmc_autocorr *ac, uint64_t *samples_out, size_t *n_lags_out);
int isingmc_autocorr_get(isingmc_autocorr *ac, uint64_t *counts_out, uint64_t *diff_out);
int isingmc_autocorr_reset(isingmc_autocorr *ac);
int isingmc_autocorr_destroy(isingmc_autocorr *ac);
int isingmc_run_sampling_autocorr(isingmc_autocorr *ac, double beta, size_t thermalization, size_t sampling_freq, size_t n_samples,
                                  int site_sums, double *energies_out);
int isingmc_host_autocorr_plan(uint64_t samples_taken, size_t n_lags, uint32_t *slot_of_lag_out, uint32_t *live_lags_out,
                               uint32_t *write_slot_out, uint64_t *counts_out);

/* replaces the whole sampling loop of lattice.rs:271-287 / classicising.rs:144-173:
 *   thermalization x do_time_step(beta);  n_samples x { sampling_freq x do_time_step(beta);
 *   states[r][k][:] = state_ref();  energies[r][k] = get_energy() }
 * energies_out: double[R][n_samples]; states_out: bytes [R][n_samples][nvars] (the bool[R,S,N] array).
 * beta is ignored while per-replica betas are set.  Sweeps, sample copies and measurements are
 * enqueued back to back; the host waits once per chunk of samples. */
int isingmc_run_sampling(isingmc_states *states, double beta, size_t thermalization, size_t sampling_freq,
                         size_t n_samples, double *energies_out, uint8_t *states_out);

/* ---- on-stream parallel tempering (periodic field-free lattices; replica-packed real-coupling containers) ----
 * The classical counterpart of the loop in tempering.rs:177-194 { timesteps; parallel_tempering_step }
 * with NO host synchronisation inside it: sweeps, the energy measurement, the exchange decisions
 * (same arithmetic as isingmc_host_pt_swap_round) and the relabelling of the slots' betas are all
 * enqueued on the engine's HIP stream.  Between isingmc_pt_measure and isingmc_pt_swap a multi-GPU
 * caller all-gathers the `local` buffer of every rank into the `all` buffer ON THAT STREAM (RCCL:
 * ncclAllGather / torch.distributed.all_gather_into_tensor under torch.cuda.ExternalStream); with a
 * single rank isingmc_pt_measure fills `all` itself.
 *
 * attach: ladder_betas[n_rungs] in ladder order; this shard owns slots
 * [slot_offset, slot_offset + n_replicas) of n_rungs, every rank owning slots_per_rank slots (the last
 * ranks fewer); rung i starts on slot i; `seed` keys the exchange decisions. */
int isingmc_pt_attach(isingmc_states *states, const double *ladder_betas, size_t n_rungs, size_t slot_offset,
                      size_t slots_per_rank, size_t world_size, uint64_t seed);
/* would isingmc_pt_attach accept this container and geometry?  *ok_out = 1 / 0, no side effects (when 0,
 * isingmc_last_error() says why): the ranks of a sharded ladder agree on the answer BEFORE any of them attaches */
int isingmc_pt_can_attach(const isingmc_states *states, size_t n_rungs, size_t slot_offset, size_t slots_per_rank,
                          size_t world_size, int *ok_out);
/* release the ladder (synchronises); configurations and timestep stay, the per-replica betas are cleared; the ladder's
 * statistics (below) are discarded with it: the next ladder starts without any, switched off */
int isingmc_pt_detach(isingmc_states *states);
/* device pointers: local = double[slots_per_rank] (send buffer), all = double[world_size*slots_per_rank] */
int isingmc_pt_buffers(isingmc_states *states, void **d_local_out, void **d_all_out, size_t *per_rank_out);
int isingmc_pt_time_steps(isingmc_states *states, size_t timesteps); /* enqueue only */
int isingmc_pt_measure(isingmc_states *states);                      /* enqueue only */
/* single rank: `timesteps` sweeps with an exchange round after every swap_every-th one, enqueued in one call (on
 * mid-size lattices one persistent launch whose strips exchange temperatures themselves; same decisions) */
int isingmc_pt_run(isingmc_states *states, size_t timesteps, size_t swap_every);
int isingmc_pt_swap(isingmc_states *states);                         /* enqueue only */
/* synchronises; perm_out = uint32[n_rungs] (rung -> slot), exchange rounds done, accepted swaps */
int isingmc_pt_state(isingmc_states *states, uint32_t *perm_out, uint64_t *round_out, uint64_t *swaps_out);

/* ---- ladder statistics (no reference counterpart): what choosing the betas needs, kept on the device ----
 * While they are on, every exchange round -- isingmc_pt_swap, and the rounds that the strips of isingmc_pt_run's persistent
 * launch decide among themselves: statistics do NOT put that call on one launch per round -- updates, with `round` the
 * round's number, p / p' the permutation rung -> slot before / after it and E[slot] the energies it decides from:
 *   1. every rung i: sum_e[i] += E[p[i]], sum_e2[i] += E[p[i]] * E[p[i]] (f64; the product and both additions rounded
 *      separately, one addition per rung and round in round order: numpy reproduces the sums bit for bit).  A configuration
 *      counts at the beta it was just swept at.
 *   2. every pair (i, i + 1) with i = round (mod 2), i + 1 < n_rungs: attempts[i] += 1, accepts[i] += 1 if it was exchanged.
 *   3. n_rungs >= 2, with one label per slot (0 = none, the start; 1 = up; 2 = down): the slot s = p'[0] gains a round trip if
 *      its label is down, and becomes up; the slot p'[n_rungs - 1] becomes down; then every rung i adds (label[p'[i]] == up)
 *      to n_up[i] and (label[p'[i]] == down) to n_down[i].  n_up / (n_up + n_down) is the flow fraction of feedback-optimised
 *      ladders (Katzgraber, Trebst, Huse and Troyer 2006).
 *   4. rounds += 1.
 * The relabelling launch of isingmc_pt_attach updates nothing.  Decisions, configurations, energies and random numbers do not
 * change.  A shard of a larger ladder is accepted: every rank's exchange kernel sees the whole permutation and all gathered
 * energies, so every rank holds the statistics of the whole ladder, identical, without communication.
 *
 * set_statistics: the first switch-on allocates one device block (2 (n - 1) + 2 n uint64 counters, 2 n f64 sums, n uint64 round
 * trips, n label bytes, the round count) and zeroes it on the stream; on = 0 stops counting and keeps the values.
 * statistics_get (synchronises): attempts / accepts uint64[n_rungs - 1]; n_up / n_down uint64[n_rungs] and sum_e / sum_e2
 * double[n_rungs] by rung; round_trips uint64[n_rungs] and labels uint8[n_rungs] by GLOBAL slot; *in_kernel_rounds_out = how many
 * of the counted rounds were decided inside persistent launches (a host count).  Any pointer may be NULL.
 * statistics_reset (enqueue only): everything back to zero, the labels to none; the setting stays.
 * Refused with ISINGMC_ERR_INVALID, container unchanged: no ladder attached; get or reset before the first switch-on. */
int isingmc_pt_set_statistics(isingmc_states *states, int on);
int isingmc_pt_statistics_get(isingmc_states *states, uint64_t *rounds_out, uint64_t *in_kernel_rounds_out, uint64_t *attempts_out,
                              uint64_t *accepts_out, uint64_t *n_up_out, uint64_t *n_down_out, double *sum_e_out, double *sum_e2_out,
                              uint64_t *round_trips_out, uint8_t *labels_out);
int isingmc_pt_statistics_reset(isingmc_states *states);

/* the engine's hipStream_t (for enqueuing the collective) and a host-side wait for it */
int isingmc_states_stream(isingmc_states *states, void **stream_out);
int isingmc_synchronize(isingmc_states *states);

/* ---- in-process ladder across several devices --------------------------------------------------------------
 * One host thread, one isingmc_states per device, each with the SAME ladder attached (isingmc_pt_attach with world_size =
 * n_shards, slot_offset = k * slots_per_rank): the group runs the exchange step of tempering.rs:191-194 between them without any
 * binding of the caller's to a collective library.  backend 0: RCCL (ncclCommInitAll + ncclAllGather on the engines' streams;
 * librccl.so is loaded with dlopen when the group is created, so single-GPU users need nothing) when every shard has a device of
 * its own and the library resolves, else event-ordered device copies (hipMemcpyPeerAsync); 1: RCCL or an error; 2: copies.
 * isingmc_pt_group_run enqueues { timesteps; measure; all-gather; swap } for the whole ladder; nothing waits on the host until
 * isingmc_pt_group_synchronize.  The shards stay the caller's (destroy the group first). */
typedef struct isingmc_pt_group isingmc_pt_group;
int isingmc_pt_group_create(isingmc_states **shards, size_t n_shards, int backend, isingmc_pt_group **group_out);
int isingmc_pt_group_backend(const isingmc_pt_group *group); /* 1 = RCCL, 2 = device copies */
int isingmc_pt_group_allgather(isingmc_pt_group *group);     /* enqueue only: local buffers -> every shard's all buffer */
int isingmc_pt_group_run(isingmc_pt_group *group, size_t timesteps, size_t swap_every); /* enqueue only */
int isingmc_pt_group_synchronize(isingmc_pt_group *group);
void isingmc_pt_group_destroy(isingmc_pt_group *group);

/* ---- population annealing: resampling on the device (Hukushima and Iba 2003, Machta 2010; no reference
 * counterpart) ----
 * A population is one container whose replicas share one beta.  Between two temperatures the caller resamples it: new slot j
 * takes the configuration of old replica src[j], with src from the rule of isingmc_host_pa_sources applied to the energies of
 * the current configurations.  Resampling moves CONFIGURATIONS only: the Philox keys stay with the slots and the timestep
 * counter does not advance, so the copies of one configuration diverge from the next sweep on.  Cluster periods
 * (isingmc_states_set_cluster_every / _set_icm_every) may be on: all replicas share one beta, so the pairs stay valid.
 * Memory: from the first resampling on the container keeps a second state buffer exactly as large as its state (the gathers
 * write into it and the two are swapped), plus 28 bytes per replica of tables; both are freed with the container.
 * Served: checkerboard containers with fast_path == 0 and both replica-packed families.  Refused with ISINGMC_ERR_INVALID and a
 * message by every entry point of this block, the container untouched: the f64 CSR family; lattices with fields, open boundaries or anisotropic couplings (they
 * have no device-side energy array); a tempering ladder attached; per-replica betas set; a shard of a larger set of experiments;
 * an empty container; more than 2^31 replicas; a non-finite dbeta.  The steps may be given (isingmc_pa_run) or chosen from the
 * population as the schedule runs (isingmc_pa_choose_step, isingmc_pa_run_adaptive). */
/* enqueue only: measure, weights, prefix sum, source table, gather.  dbeta = beta_to - beta_from; (seed, step) key the offset. */
int isingmc_pa_resample(isingmc_states *states, double dbeta, uint64_t seed, uint64_t step);
/* the gather alone with the caller's table src[count] in host memory: new slot j <- old replica src[j]; any table with entries
 * below the replica count is valid (custom resampling schemes).  The families follow.  Synchronises. */
int isingmc_pa_apply_sources(isingmc_states *states, const uint32_t *src);
/* A whole schedule in one call: for k = 0 .. n_betas - 1 { k > 0: the resampling for betas[k] - betas[k-1] keyed by (seed, k);
 * sweeps_per_beta timesteps at betas[k] }.  Everything is enqueued -- the acceptance tables of all betas are uploaded before the
 * first launch, every resampling leaves its record in a device log -- and the host waits ONCE, at the end, then fills
 * sum_out / eref_out / distinct_out / mean_energy_out[n_betas - 1] (any may be NULL) with the step records in order.  (While a
 * cluster period is on, the cluster steps' workspace makes the host wait once per beta.)  Same results as the loop of
 * isingmc_pa_resample and isingmc_do_time_steps. */
int isingmc_pa_run(isingmc_states *states, const double *betas, size_t n_betas, size_t sweeps_per_beta, uint64_t seed,
                   uint64_t *sum_out, double *eref_out, uint64_t *distinct_out, double *mean_energy_out);
/* The step chooser: measures the energies as isingmc_pa_resample would, runs the rule of
 * isingmc_host_pa_choose_step on the device (grid-wide integer reductions, stream-ordered launches) and synchronises to return
 * the decision.  It READS only: configurations, random numbers, the timestep, the families and the record of isingmc_pa_last stay
 * as they are.  An isingmc_pa_resample(*dbeta_out) that follows forms exactly the weights the choice was made with: its record's sum
 * equals *sum_out.  Refused like the other entry points of this block (and like isingmc_pa_resample while a recorder objects), and for
 * a dbeta_max that is not finite and positive or a target outside (0, 1]; the container untouched. */
int isingmc_pa_choose_step(isingmc_states *states, double dbeta_max, double target, uint32_t *k_out, double *dbeta_out, uint64_t *sum_out,
                           uint64_t *num_lo_out, uint64_t *num_hi_out);
/* A schedule from beta_start up to beta_end whose steps are chosen as it runs: sweeps_per_beta timesteps at beta_start, then
 * { isingmc_pa_choose_step with dbeta_max = min(dbeta_cap, beta_end - beta); beta += dbeta -- or, when k = 65536 and that
 * dbeta_max reaches beta_end, beta = beta_end exactly; the resampling for dbeta keyed by (seed, step index 1, 2, ..);
 * sweeps_per_beta timesteps } until beta = beta_end.  dbeta_cap > 0 (infinity: no cap).  Same results as that loop of
 * isingmc_pa_choose_step, isingmc_pa_resample and isingmc_do_time_steps.  The host waits once per temperature, for the decision
 * (it builds the acceptance tables from the beta); the search is enqueued behind the sweeps.  betas_out[max_steps + 1] receives the
 * schedule, *n_betas_out its length; sum_out / eref_out / distinct_out / mean_energy_out[max_steps] (any may be NULL) the step
 * records as isingmc_pa_run reports them.  If max_steps steps do not reach beta_end: ISINGMC_ERR_INVALID, the container at the last
 * completed temperature betas_out[*n_betas_out - 1], the outputs filled that far.  isingmc_pa_run on betas_out repeats the run
 * wherever betas[k] - betas[k-1] gives back every chosen dbeta exactly (always for the last step; for all steps when beta_start,
 * beta_end and dbeta_cap are dyadic, as multiples of 2^-20 below 1 are); elsewhere the two differ by the rounding of that difference. */
int isingmc_pa_run_adaptive(isingmc_states *states, double beta_start, double beta_end, size_t sweeps_per_beta, uint64_t seed,
                            double target, double dbeta_cap, size_t max_steps, double *betas_out, size_t *n_betas_out,
                            uint64_t *sum_out, double *eref_out, uint64_t *distinct_out, double *mean_energy_out);
/* synchronises; the record of the last resampling (isingmc_pa_resample, or the last step of isingmc_pa_run): src_out[count]
 * (NULL allowed; that resampling's own table -- a later isingmc_pa_apply_sources does not touch it), S, E_ref, the number of distinct sources and the population's mean energy before the resampling.
 * ISINGMC_ERR_INVALID before the first resampling. */
int isingmc_pa_last(isingmc_states *states, uint32_t *src_out, uint64_t *sum_out, double *eref_out, uint64_t *distinct_out,
                    double *mean_energy_out);
/* family_out[count]: the slot whose configuration at the last reset (or at creation) each slot's configuration descends from;
 * synchronises.  The reset makes every slot its own family again. */
int isingmc_pa_families(isingmc_states *states, uint32_t *family_out);
int isingmc_pa_reset_families(isingmc_states *states);

/* ---- measurement hook (bench.py; no reference counterpart) ------------------------------------------
 * Runs `timesteps` sweeps at `beta` like isingmc_do_time_steps and, beside them on a side stream, one
 * wave that stamps the shader-cycle counter against the 100 MHz constant counter for `probe_ms`
 * milliseconds: *ghz_out = the shader clock the chip holds under this kernel. */
int isingmc_debug_shader_clock(isingmc_states *states, size_t timesteps, double beta, double probe_ms,
                               double *ghz_out);

/* ---- test hook (no reference counterpart) -------------------------------------------------------------
 * The device blocks and pinned host blocks that graphs, containers and running calls of this process hold
 * at the moment, taken from the library's block caches (idle blocks do not count; with
 * ISINGMC_NO_ALLOC_CACHE=1 nothing is tracked and both are 0).  Equal counts before an object is created
 * and after it is destroyed: every block it took has come back. */
int isingmc_debug_live_blocks(size_t *device_blocks_out, size_t *pinned_blocks_out);

#ifdef __cplusplus
}
#endif
#include "isingmc_cluster_series.h"
#endif /* ISINGMC_H */
