// Internal declarations shared by the host translation units of libisingmc.so (not installed, not part of the C ABI):
//   core.hip       error state, device-block / pinned-block / stream / event caches, environment helpers
//   graph.hip      edge-list checks, host-only C ABI helpers, lattice / general / packed / real-coupling graph construction
//   isingmc.hip    replica containers, every sweep / measurement launch (their policy: step_policy.hpp), the persistent strip kernel's host side
//   nonlocal.hip   host side of the non-local moves: Swendsen-Wang steps, isoenergetic cluster moves inside and between containers
//   overlaps.hip   spin and link overlaps between replica pairs (isingmc_overlaps), and the spin overlap by site class
//                  (isingmc_site_classes_*, isingmc_overlaps_by_class); the overlap core they share with the series
//   overlap_series.hip  the device-resident log of overlap measurements, one row per sample (isingmc_overlap_series_*)
//   observable_series.hip  the device-resident log of energy and magnetisation per sample (isingmc_observable_series_*)
//   cluster_series.hip  the device-resident log of cluster-size moments, one row per non-local step (isingmc_cluster_series_*)
//   recorders.hip  the table of the measurements the step loop takes on a period, and the log core of the series
//   best.hip       each replica's lowest-energy configuration, kept on the device (isingmc_best_*)
//   moments.hip    per-site spin sums and per-bond sums over the samples of a run (isingmc_moments_*)
//   autocorr.hip   the lag ring: spin autocorrelation over time lags against stored snapshots (isingmc_autocorr_*)
//   sampling.hip   get_states and the double-buffered sampling pipeline
//   tempering.hip  on-stream parallel tempering, the in-process ladder group (RCCL through dlopen)
//   population.hip population annealing: the on-stream resampling step (isingmc_pa_*)
//   debug.hip      shader-clock probe
// Device and pinned blocks, pooled streams and events are held in the handles of owned_block.hpp, which hand them back: no unit
// frees one by hand.  The path / tuning switches of a graph or a container are options.hpp.
// Every kernel but the probe's is defined in a *_kernels.hip unit of its own and launched through the plain C++ launchers that the
// headers below declare; none of them defines a kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/isingmc.h"
#include "autocorr_kernels.hpp"
#include "best_kernels.hpp"
#include "cluster_kernels.hpp"
#include "general_launch.hpp"
#include "host_logic.hpp"
#include "lattice_types.hpp"
#include "packed_between_kernels.hpp"
#include "packed_cluster_kernels.hpp"
#include "packed_icm_kernels.hpp"
#include "packed_types.hpp"
#include "pa_kernels.hpp"
#include "mc_types.hpp"
#include "moments_kernels.hpp"
#include "observable_series_kernels.hpp"
#include "overlap_class_kernels.hpp"
#include "overlap_kernels.hpp"
#include "overlap_series_kernels.hpp"
#include "options.hpp"
#include "owned_block.hpp"
#include "real_types.hpp"
#include "spread_types.hpp"
#include "step_policy.hpp"
#include "strip_types.hpp"
#include "tempering_types.hpp"

using namespace isingmc;


#define IM_INTERNAL __attribute__((visibility("hidden")))

// ---- errors (core.hip) ----------------------------------------------------------------------------------------------------
IM_INTERNAL int fail(int code, const std::string &msg); // sets the calling thread's isingmc_last_error() and returns `code`
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t err__ = (expr);                                                                 \
        if (err__ != hipSuccess)                                                                   \
            return fail(err__ == hipErrorOutOfMemory ? ISINGMC_ERR_ALLOC : ISINGMC_ERR_HIP,        \
                        std::string(#expr) + ": " + hipGetErrorString(err__));                     \
    } while (0)

#define TRY(expr)                                                                                  \
    do {                                                                                           \
        int rc__ = (expr);                                                                         \
        if (rc__ != ISINGMC_OK) return rc__;                                                       \
    } while (0)


// ---- caches (core.hip): device blocks, pinned host blocks, streams, events are recycled; every owner drains its streams before
// it hands a block back (hipFree used to synchronise the device).  Blocks are held in the handles of owned_block.hpp, which free them.
IM_INTERNAL hipError_t cached_malloc(void **out, size_t bytes);
IM_INTERNAL hipError_t cached_host_malloc(void **out, size_t bytes);
IM_INTERNAL hipError_t stream_quiesce(hipStream_t st); // a query when everything has completed, else a synchronisation
// Pooled streams and events are held in the handles of owned_block.hpp, which hand them back; these fill one (as dev_alloc a block)
IM_INTERNAL int stream_create(PooledStream &out);
IM_INTERNAL int event_create(PooledEvent &out); // no timing: ordering between streams
IM_INTERNAL int event_create(TimedEvent &out);  // with timing: the *_timed entry point
IM_INTERNAL int use_device(int device);
// the runtime's occupancy answers (workgroups per compute unit) behind one cache: each query is asked once per process
IM_INTERNAL int cached_lat_sweep_loop_blocks_per_cu(bool pmj, unsigned lds_bytes, int rounds);
IM_INTERNAL int cached_rj_measure_blocks_per_cu(uint32_t slots, bool bipartite, bool count_up);
IM_INTERNAL int cached_strip_blocks_per_cu(bool pmj, int nw, bool ladder, size_t lds_bytes, int rounds);
IM_INTERNAL int cached_spread_blocks_per_cu(bool vec, bool pmj, int lanes_per_quad, unsigned threads, size_t lds_bytes, int rounds);

// ---- options.hpp: struct Options, the path / tuning switches of a graph or a container, and the environment helpers ----------

struct isingmc_graph {
    int device = 0;
    int kind = ISINGMC_KIND_GENERAL;
    uint64_t nvars = 0, n_edges = 0;
    uint64_t state_words = 0;
    bool has_bias = false;
    // lattice path
    LatGeom geom{};
    bool vec = false;
    double jabs = 0.0;
    bool uniform_sign = true;
    uint32_t jneg_uniform = 0;
    uint32_t *d_jneg = nullptr; // [2 colours][4 directions][wpp]
    // multi-class checkerboard kernels (mc_types.hpp): uniform field or open boundaries on a recognised lattice
    int mc_mode = MC_NONE;
    double jabs_y = 0.0;  // MC_ANISO: |J| of the vertical bonds (jabs = the horizontal ones')
    double field = 0.0;   // MC_FIELD: h of E = sum J s s - h sum s
    McOpen open{0, 0, 0}; // MC_OPEN, MC_FIELD_OPEN
    uint32_t *d_fneg = nullptr; // fields of one size and both signs: sign planes [2][wpp] (bit set where h_i < 0); field = |h| then
    // general path
    GenGraphDev gdev{};
    uint32_t gen_edges2 = 0; // directed edges of the CSR (rowptr[n_pos])
    bool w_is_float = false;
    std::vector<uint64_t> class_base;
    std::vector<uint64_t> pos; // site -> packed position
    double self_energy = 0.0;
    uint32_t n_colours = 2;
    // replica-packed variant of the general path (uniform |J|, no fields, degree <= PK_MAX_DEG)
    bool packed_ok = false;
    PkGraphDev pk{};
    // every real site has this degree (3..6): packed_uni_kernels.hpp; 0 otherwise
    int pk_uni_deg = 0;
    bool pk_uni_pmj = false;             // couplings of both signs
    PkUniHeaders pk_uni{};
    uint32_t pk_uni_but_one = 0;         // (block, slot) headers that are a translation for every lane but one
    std::vector<uint32_t> pk_class_full; // per colour class: end of its last 256-block without padding
    std::vector<uint8_t> pk_class_table; // per colour class: some block header of its full blocks is PK_HDR_MIXED (needs table entries)
    uint64_t n_directed = 0;
    // replica-packed real-coupling path (real_kernels.hpp): any couplings and biases, degree <= 15
    bool rj_ok = false;
    RjGraphDev rj{};                      // the dynamics' view
    RjGraphDev rj_hi{}, rj_lo{};          // the same topology with the two integer levels of the ORIGINAL couplings (energies)
    int rj_k = 0;                         // the dynamics' couplings are integers in units of 2^rj_k (heavy sites: 2^(rj_k + dshift))
    int rj_k_energy = 0;                  // energy = 2^rj_k_energy S(hi) + 2^(rj_k_energy - 24) S(lo)
    uint32_t rj_heavy_sites = 0;
    bool stable_path = false;             // ISINGMC_FLAG_STABLE_PATH: the kernel family never depends on the number of experiments
    Options opt;                          // the environment's switches when the graph was created
    std::vector<uint32_t> class_real_end; // per colour class: end of its real sites (the padding follows)
    int n_cu = 256;                       // compute units of the device (queried once, at creation)
    // The order of the edge list, for results per entry.  General graphs: the two sites of every entry.  Recognised
    // lattices: the bond slot 2 site + direction (0 right, 1 down) of every entry -- empty when entry e is slot e, the order the
    // usual generators emit.  edge_order_kept = false: a lattice too large for 32-bit slots in another order (bond sums refused).
    std::vector<uint32_t> edge_ends, edge_slots;
    bool edge_order_kept = true;
    std::vector<DevBlock<unsigned char>> dev_allocs;

    ~isingmc_graph()
    {
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize(); // the blocks are recycled when dev_allocs goes: no kernel may still be reading the graph
    }
};

// device tables of ONE beta for a run_steps call that must not upload any (step_presets_build)
struct StepPreset {
    const LatThr *thr = nullptr;       // checkerboard paths
    const uint32_t *pk_tabs = nullptr; // bit-sliced packed path: PK_TAB_WORDS words
    const RjBeta *rj = nullptr;        // real-coupling packed path
};

// The measurements the step loop takes on a period (recorders.hip holds their table), in the order it samples them.  REC_CLUSTERS
// has no period of its own (its `every` stays 0): the non-local steps themselves append its rows
enum Recorder { REC_BEST, REC_MOMENTS, REC_OVERLAPS, REC_OBSERVABLES, REC_AUTOCORR, REC_CLUSTERS, REC_COUNT };
struct SeriesLog;

// The state of a container that ONE unit owns, a struct per unit; isingmc_states holds one of each.  Other units read them (a
// refusal, a join before a launch); the owner alone allocates, grows and resets.

// ---- isingmc.hip (the persistent strip kernel's host side, strip_kernels.hpp) -------------------------------------------------
struct StripState {
    DevBlock<unsigned long long> d_halo; // halo granules
    size_t halo_cap = 0;                 // granules allocated
    DevBlock<uint32_t> d_err;            // error word
    uint32_t epoch = 0;                  // tag epoch
    DevBlock<unsigned long long> d_pt_mail, d_pt_round_counts; // in-kernel exchange rounds (StripLadder)
    DevBlock<uint32_t> d_pt_perm2;
    DevBlock<unsigned long long> d_fin; // [cap] final-measurement counters of the strip kernel (zero between launches)
    bool test_failed = false; // ISINGMC_STRIP_TEST_FAIL_ONCE has fired for this object
    bool disabled = false;    // a strip launch of this object timed out once: the per-colour launches serve it from then on
    DevBlock<uint32_t> d_snapshot; // the planes a synchronous call started from (restored when a strip launch gives up)
    size_t snapshot_cap = 0;
    bool guard = false; // inside with_strip_retry: a strip launch is checked before an update may keep what it left
};

// ---- sampling.hip (isingmc_run_sampling: two slabs of samples in flight) ------------------------------------------------------
struct SamplingState {
    PooledStream copy_stream;
    PooledEvent ready[2], copied[2];
    DevBlock<uint32_t> d_samples[2];
    PinnedBlock<uint32_t> h_samples[2];
    DevBlock<unsigned long long> d_counts[2];
    PinnedBlock<unsigned long long> h_counts[2];
    DevBlock<double> d_e[2];
    PinnedBlock<double> h_e[2];
    DevBlock<long long> d_m;
    size_t cap_words = 0, cap_counts = 0, cap_e = 0;
};

// ---- tempering.hip (on-stream parallel tempering, isingmc_pt_*): the host side of the ladder; PtDev is what the kernels read ----
struct TemperingState {
    bool attached = false;
    DevBlock<double> d_ladder, d_local, d_all;
    DevBlock<uint64_t> d_ladder_thr;
    DevBlock<uint32_t> d_perm;
    DevBlock<unsigned long long> d_counters;
    size_t per = 0, world = 1;
    std::vector<double> ladder_betas; // host copy of d_ladder (two ladders are compared without a device read)
    DevBlock<unsigned long long> d_stats; // ladder statistics: the block of PtStats, from the first switch-on to the detach
    bool stats_on = false;                // the container's pt.stats == d_stats while on, nullptr while off
    uint64_t in_kernel_rounds = 0;        // rounds counted inside persistent strip launches (host count: which path a run took)
};

// ---- nonlocal.hip -------------------------------------------------------------------------------------------------------------
// Swendsen-Wang cluster steps (cluster_kernels.hpp): timestep t is one when every > 0 and t % every == every - 1
struct ClusterState {
    size_t every = 0;
    DevBlock<uint32_t> d_stats; // [stats_cap][2]: clusters, largest cluster of the last cluster step (packed: per counter slot)
    size_t stats_cap = 0;
    bool have_stats = false;
};
// isoenergetic cluster moves between the replicas (2 p, 2 p + 1): timestep t is one when every > 0 and
// t % every == every - 1; never on together with the cluster steps
struct IcmState {
    size_t every = 0;
    DevBlock<uint32_t> d_stats; // [stats_cap][2] clusters, largest cluster, then [stats_cap] q = -1 sites: the last ICM step of every pair
    size_t stats_cap = 0;
    bool have_stats = false;
};
// isoenergetic cluster moves between this container and another one (isingmc_icm_between): everything here
// belongs to the FIRST container of the call and stays with it, so that a call only enqueues
struct IcmBetweenState {
    DevBlock<uint32_t> d_work; // labelling workspace of `batch` pairs (cluster_words_per_replica each); packed containers
    size_t batch = 0;          // (DESIGN.md S13): of `batch` pair BLOCKS (pk_between_words_per_block each)
    DevBlock<uint32_t> d_inv;  // packed containers: (local group, bit) -> pair of the call, this container's groups first,
    size_t inv_cap = 0;        // then the other one's (words)
    DevBlock<uint32_t> d_slots; // [2][cap] slot tables of the host-table form
    DevBlock<uint32_t> d_stats; // [cap][2] clusters, largest cluster, then [cap] q = -1 sites: the last call
    size_t cap = 0, pairs = 0;
    bool have_stats = false;
    PooledEvent ev[2]; // the other container's stream has arrived / this container's launches are enqueued
};

// ---- population.hip -----------------------------------------------------------------------------------------------------------
// population annealing (isingmc_pa_*): everything here is allocated by the first resampling and stays
struct PaState {
    DevBlock<uint32_t> d_state; // the second state buffer the gathers write into: as large as the container's d_state (state_words words)
    size_t state_words = 0;
    size_t cap = 0;              // replicas the tables below hold
    DevBlock<double> d_energy;          // [cap]
    DevBlock<unsigned long long> d_cum; // [cap] weights, then their inclusive prefix sums; pa_scan_blocks(cap) block sums follow
    DevBlock<uint32_t> d_src;           // [cap] source table of the last isingmc_pa_resample
    DevBlock<uint32_t> d_user_src;      // [cap] the caller's table of the last isingmc_pa_apply_sources
    DevBlock<uint32_t> d_family, d_family2; // [cap] family of every slot, and the buffer its gather writes into
    DevBlock<PaRecord> d_record;
    bool have_record = false;    // an isingmc_pa_resample has been enqueued
    bool families_set = false;   // d_family holds the table (else: the identity)
};
// the step chooser (isingmc_pa_choose_step): blocks of its own, so that a choice touches nothing a resampling keeps
struct PaChooseState {
    DevBlock<double> d_energy;  // [cap]
    size_t cap = 0;
    DevBlock<PaChoose> d_choose;
};

// ---- best.hip -----------------------------------------------------------------------------------------------------------------
// each replica's lowest-energy configuration (isingmc_best_*): allocated when tracking is switched on (or by the
// first isingmc_best_update) for the replicas the container holds then, and kept
struct BestState {
    DevBlock<uint32_t> d_state; // as large as the container's d_state, same layout; padding positions and unowned bits of a packed
    size_t state_words = 0;      // container hold no defined value (cleared once, so that the raw read-out is deterministic)
    size_t cap = 0;              // replicas the records below hold
    DevBlock<double> d_e;                // [cap] records, +inf before the first update
    DevBlock<unsigned long long> d_t;    // [cap] the timestep each record was set at
    DevBlock<double> d_energy;           // [cap] the energies an update measures
    DevBlock<uint32_t> d_flags;          // a flag per replica (checkerboard) / an improvement mask per group (packed)
    DevBlock<unsigned long long> d_count; // improvements so far
};

// ---- moments.hip --------------------------------------------------------------------------------------------------------------
// per-site and per-bond sums over the samples of a run (isingmc_moments_*): allocated when accumulation is
// switched on (or by the first isingmc_moments_accumulate) for the replicas the container holds then, and kept
struct MomentsState {
    unsigned flags = 0;      // ISINGMC_MOMENTS_* of the sums held
    uint64_t n = 0;          // samples in the sums
    bool have = false;       // the blocks below are allocated, for R replicas
    size_t R = 0;
    DevBlock<unsigned long long> d_site, d_bond; // summed mode: set-bit counts in the layouts of moments_kernels.hpp
    DevBlock<uint2> d_edges;                      // packed containers with bond sums: the two positions of every edge entry
    DevBlock<uint32_t> d_planes, d_totals;        // per-replica mode: k time planes of the state's shape, 32-bit totals
    int k = 0;
    uint32_t pending = 0;    // samples in the time planes since the last flush (< 2^k)
};

// ---- autocorr.hip -------------------------------------------------------------------------------------------------------------
// the lag ring (isingmc_autocorr_*): allocated by isingmc_autocorr_create for the replicas the container holds
// then, gone with isingmc_autocorr_destroy; one ring per container
struct AutocorrState {
    bool live = false;   // a ring exists (its handle is out)
    uint32_t n_lags = 0; // L
    uint64_t samples = 0; // samples enqueued since creation or the last reset: the next one is sample number `samples`
    size_t R = 0;         // replicas the sums hold
    size_t slot_words = 0; // words of one snapshot: the state buffer's
    DevBlock<uint32_t> d_ring;           // [L][slot_words]
    DevBlock<unsigned long long> d_sums; // [counter slots][L + 1]
};

struct isingmc_states {
    isingmc_graph *g = nullptr;
    Options opt; // the environment's switches when the container was created (isingmc_states_set_option changes one)
    size_t R = 0, cap = 0;
    DevBlock<uint32_t> d_state;
    DevBlock<uint2> d_keys;
    uint64_t t = 0; // absolute timestep = Philox counter
    PooledStream stream;
    std::vector<PooledStream> lanes; // sweep launches of disjoint replica blocks alternate over these (see run_steps)
    std::vector<PooledEvent> lane_events;
    PooledEvent fork_event;
    size_t n_lanes = 1; // lanes in use by the current run_steps call
    TimedEvent ev0, ev1;
    bool has_betas = false;
    std::vector<double> betas;
    DevBlock<LatThr> d_thr;
    DevBlock<LatThrMC> d_thr_mc; // per-replica thresholds of the multi-class kernels (has_betas on a field / open lattice)
    DevBlock<double> d_beta;
    const StepPreset *step_preset = nullptr; // set around a run_steps call by isingmc_pa_run: the tables of its beta are on the device
    // measurement scratch
    DevBlock<unsigned long long> d_meas; // lattice: [R][2]
    bool meas_zero = false;               // d_meas is known to be all zero (left so by the tempering measurement)
    bool meas_fresh = false; // the tempering send buffer holds the energies of the CURRENT configurations (written by the last strip launch)
    DevBlock<double> d_pe, d_oe;
    DevBlock<long long> d_pm, d_om;
    uint32_t n_partials = 0;
    // replica-packed general path: one word per position = 32 replicas of a group
    bool packed = false;
    size_t groups = 0;
    size_t pk_bit0 = 0; // replica r of this shard is bit (r + pk_bit0) % 32 of group (r + pk_bit0) / 32 (shards cut GLOBAL groups)
    size_t pk_slots() const { return 32 * groups; } // counter slots: one per (group, bit), owned or not
    DevBlock<uint32_t> d_tab; // threshold tables [groups or steps][PK_TAB_WORDS]
    // one-degree packed kernels: the wave-uniform halves of the Philox calls of timesteps [pk_philox_t0, + pk_philox_steps) for
    // pk_philox_groups groups (packed_types.hpp); kept across calls -- a tempering round of ten timesteps does not pay a table launch
    DevBlock<uint32_t> d_pk_philox;
    uint64_t pk_philox_t0 = 0;
    size_t pk_philox_steps = 0, pk_philox_groups = 0;
    bool rj = false;           // packed container on the real-coupling path (real_kernels.hpp) instead of the bit-sliced one
    DevBlock<RjBeta> d_rj_betas; // per-replica acceptance scales [32 groups] (has_betas)
    DevBlock<unsigned long long> d_pk_slot_thr; // on-stream tempering on the bit-sliced packed path: T_m per slot [32 groups][PK_MAX_DEG]
    size_t n_total = 0, first = 0; // this container is the shard [first, first + R) of n_total experiments
    // the sample points of the periodic recorders.  REC_BEST: an update follows every timestep after which t % every == 0 (t0 stays
    // 0).  REC_OVERLAPS / REC_OBSERVABLES: a row of series[...], the one series of its kind that records on a period.
    // REC_AUTOCORR: the lag ring's samples (S26; its state is acr below, not a series).  REC_CLUSTERS: series[...] is the container's
    // one live cluster series (S24)
    Periodic rec[REC_COUNT];
    SeriesLog *series[REC_COUNT] = {};
    size_t osr_by_rung_live = 0; // live overlap series that read this container's ladder permutation on the device: no isingmc_pt_detach
    size_t obs_by_rung_live = 0; // ... and live observable series that do
    // what one unit owns (the structs above)
    StripState strip;
    SamplingState sampling;
    PtDev pt{};
    TemperingState tempering;
    ClusterState cl;
    IcmState icm;
    IcmBetweenState icmb;
    PaState pa;
    PaChooseState pac;
    BestState best;
    MomentsState mom;
    AutocorrState acr;

    // The body runs before any member goes: with the device current, nothing of this object may still be running when the
    // members' blocks, streams and events go back to their caches, where the next request may pick them up at once (hipFree used
    // to wait for the whole device).  The handles release; nothing is released by hand.
    ~isingmc_states()
    {
        if (!g) return;
        (void)hipSetDevice(g->device);
        if (stream) (void)stream_quiesce(stream);
        for (hipStream_t st : lanes) (void)stream_quiesce(st);
        if (sampling.copy_stream) (void)stream_quiesce(sampling.copy_stream);
    }
};

// `count` elements into `out`; whatever `out` held is freed, but only once the new block is there.  The caller has made sure that
// nothing enqueued reads the old block.
template <typename T>
static int dev_alloc(DevBlock<T> &out, size_t count)
{
    void *p = nullptr;
    HIP_TRY(cached_malloc(&p, std::max<size_t>(count, 1) * sizeof(T)));
    out = DevBlock<T>(static_cast<T *>(p));
    return ISINGMC_OK;
}

// ... `count` elements of any type that `owner` keeps until it goes (a graph's tables, the scratch of one call)
using DevBlocks = std::vector<DevBlock<unsigned char>>;
template <typename T>
static int dev_alloc(DevBlocks &owner, T **out, size_t count)
{
    *out = nullptr;
    DevBlock<unsigned char> b;
    TRY(dev_alloc(b, std::max<size_t>(count, 1) * sizeof(T)));
    *out = reinterpret_cast<T *>(b.get());
    owner.push_back(std::move(b));
    return ISINGMC_OK;
}

// A device block that a container owns takes another size: nothing enqueued on `stream` may still use the old block, which goes
// back to the cache.  `count` elements, recorded as *cap = new_cap (the owner's unit); a failed allocation leaves {nullptr, 0}.
template <typename T>
static int dev_regrow(hipStream_t stream, DevBlock<T> &block, size_t *cap, size_t count, size_t new_cap)
{
    HIP_TRY(stream_quiesce(stream));
    block.reset();
    *cap = 0;
    TRY(dev_alloc(block, count));
    *cap = new_cap;
    return ISINGMC_OK;
}

// device -> host on the container's stream, waited for
template <typename T>
static int read_back(isingmc_states *s, std::vector<T> &h, const T *d, size_t n)
{
    h.resize(n);
    HIP_TRY(hipMemcpyAsync(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return ISINGMC_OK;
}

// `waiter` goes on behind what `ahead` holds so far.  ev: an event of the caller's -- which one it owns is part of its lifetime
// rules (a container's icmb.ev for the between move and the synchronising overlap calls, a series' own for its records)
static inline int stream_wait_for(hipStream_t waiter, hipStream_t ahead, hipEvent_t ev)
{
    HIP_TRY(hipEventRecord(ev, ahead));
    HIP_TRY(hipStreamWaitEvent(waiter, ev, 0));
    return ISINGMC_OK;
}

// device scratch of one API call: freed on every exit path, after the stream has drained
struct DeviceScratch {
    hipStream_t stream;
    DevBlocks blocks;
    explicit DeviceScratch(hipStream_t st) : stream(st) {}
    DeviceScratch(const DeviceScratch &) = delete;
    ~DeviceScratch() { if (!blocks.empty()) (void)hipStreamSynchronize(stream); }
    template <typename T>
    int alloc(T **out, size_t count) { return dev_alloc(blocks, out, count); }
};

template <typename T>
static int graph_upload(isingmc_graph *g, const T **dst, const std::vector<T> &src)
{
    T *d = nullptr;
    TRY(dev_alloc(g->dev_allocs, &d, src.size()));
    if (!src.empty()) HIP_TRY(hipMemcpy(d, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    *dst = d;
    return ISINGMC_OK;
}

template <typename F>
static void parallel_for(size_t n, F &&body, size_t bytes_per_item = size_t(1) << 20)
{
    // small jobs run on the calling thread: starting and joining threads costs ~100 us, more than expanding a few KB
    const size_t nthreads = n * bytes_per_item < (size_t(1) << 18)
                                ? 1 : std::min<size_t>(n, std::max(1u, std::min(32u, std::thread::hardware_concurrency())));
    if (nthreads <= 1) {
        for (size_t i = 0; i < n; i++) body(i);
        return;
    }
    std::vector<std::thread> pool;
    for (size_t tid = 0; tid < nthreads; tid++)
        pool.emplace_back([&, tid] {
            for (size_t i = tid; i < n; i += nthreads) body(i);
        });
    for (auto &th : pool) th.join();
}

// ---- graph.hip ---------------------------------------------------------------------------------------------------------------
IM_INTERNAL uint64_t threshold_fixed(double beta, double dE);
IM_INTERNAL LatThr lattice_thresholds(double beta, double jabs);
IM_INTERNAL LatThrMC lattice_thresholds_mc(const isingmc_graph *g, double beta);
IM_INTERNAL double lattice_energy(const isingmc_graph *g, unsigned long long sat, unsigned long long up);
IM_INTERNAL void pack_state(const isingmc_graph *g, const uint8_t *spins, uint32_t *words);
IM_INTERNAL void unpack_state(const isingmc_graph *g, const uint32_t *words, uint8_t *spins);

// ---- tempering.hip -----------------------------------------------------------------------------------------------------------
IM_INTERNAL int energies_enqueue(isingmc_states *s, double *d_out); // checkerboard (periodic, no field) and both packed families

// ---- isingmc.hip (replica containers and launches) ---------------------------------------------------------------------------
constexpr size_t MAX_GRID_Y = 32768;
constexpr int STRIP_TIMED_OUT = 1000; // internal status, never returned through the C ABI
struct StripPlan {
    bool use = false;
    int nw = 1; // waves per strip (workgroup)
    StripArgs a{};
    size_t replicas_per_pass = 0; // a pass = one launch over a block of replicas for all timesteps of the chunk
};
IM_INTERNAL int run_steps(isingmc_states *s, size_t timesteps, const double *betas, size_t beta_stride, double *energies_per_step,
                          float *device_ms, bool sync = true, double *final_energies = nullptr);
IM_INTERNAL int step_presets_build(isingmc_states *s, const double *betas, size_t n, DeviceScratch &scratch, std::vector<StepPreset> &out);
IM_INTERNAL int set_betas(isingmc_states *s, const double *beta_per_replica, bool all_equal);
IM_INTERNAL int lanes_join(isingmc_states *s); // the main stream waits for the replica lanes of the current run_steps call
IM_INTERNAL int measure_enqueue(isingmc_states *s, unsigned long long *counts_slot, double *e_slot, long long *m_slot, bool want_up = true);
IM_INTERNAL void lat_measure_enqueue(isingmc_states *s, unsigned long long *out, size_t out_stride); // lattice containers: the counting launches alone
IM_INTERNAL double pk_energy(const isingmc_graph *g, bool rj, unsigned long long c0, unsigned long long c1);
IM_INTERNAL int pk_get_states(isingmc_states *s, uint8_t *states_out, size_t replica_stride_bytes, uint32_t *packed_out,
                              const uint32_t *d_words = nullptr); // d_words: a buffer laid out as d_state (nullptr: d_state itself)
IM_INTERNAL step_policy::GraphFacts graph_facts(const isingmc_graph *g); // what step_policy.hpp reads of a graph
IM_INTERNAL StripPlan strip_plan(const isingmc_states *s, size_t timesteps, bool ladder = false); // step_policy::strip_plan for this container
IM_INTERNAL int launch_strip(isingmc_states *s, const StripPlan &P, size_t r0, size_t n, size_t nk, const LatThr *d_thr_steps, uint32_t thr_stride,
                             unsigned long long *steps_out, double *final_energies, const StripLadder *ladder = nullptr);
IM_INTERNAL int strip_check(isingmc_states *s);
IM_INTERNAL int strip_error(int rc);
IM_INTERNAL bool may_use_strips(const isingmc_states *s);
// Philox4x32-7 for the sweeps: the periodic, field-free, one-|J| checkerboard lattices alone
IM_INTERNAL bool philox_rounds_served_by(const isingmc_states *s);
IM_INTERNAL int snapshot_take(isingmc_states *s);
IM_INTERNAL int snapshot_restore(isingmc_states *s);

// ---- sampling.hip ------------------------------------------------------------------------------------------------------------
// one byte per spin of every replica out of `d_words`, a buffer laid out as d_state (isingmc_get_states passes d_state)
IM_INTERNAL int expand_states(isingmc_states *s, const uint32_t *d_words, uint8_t *states_out, size_t replica_stride_bytes);

// ---- best.hip (each replica's lowest-energy configuration) -------------------------------------------------------------------
// enqueue: decide + keep from d_energy[R], the energies of the CURRENT configurations, on the container's stream (lanes joined)
IM_INTERNAL int best_from_energies(isingmc_states *s, const double *d_energy);
IM_INTERNAL int best_update_enqueue(isingmc_states *s); // energies_enqueue into the container's own array, then the above

// ---- moments.hip (per-site and per-bond sums over the samples of a run) -------------------------------------------------------
IM_INTERNAL int moments_sample_enqueue(isingmc_states *s); // enqueue: one sample of all replicas into the sums (joins the lanes)

// ---- autocorr.hip (the lag ring) ----------------------------------------------------------------------------------------------
IM_INTERNAL int autocorr_sample_enqueue(isingmc_states *s); // enqueue: one sample of all replicas against the ring (joins the lanes)

// ---- overlaps.hip (which containers and pairings an overlap measurement serves) --------------------------------------------------
// A class set as the kernels of overlap_class_kernels.hip read it: on a recognised lattice the tables in plane order with one
// shared-class entry per word, on a graph with a replica-packed layout the positions sorted by class and cut into segments.  A
// graph that only the f64 CSR family serves gets the sizes alone: the measurement refuses its containers.
struct isingmc_site_classes {
    const isingmc_graph *g = nullptr;
    int device = 0;
    size_t n_tables = 0, n_classes = 0;
    std::vector<uint64_t> sizes; // [n_tables][n_classes]
    bool has_lat = false, has_pk = false;
    LatClassDev lat{};
    PkClassDev pk{};
    DevBlocks dev_allocs;
};

// The pairs of one call, validated: what isingmc_overlaps, isingmc_overlaps_by_class and the overlap series share.  On success b is
// never NULL and either default_pairs holds (the pairing (2 p, 2 p + 1) inside one container, no tables) or slots_a / slots_b are
// host tables of n_pairs entries below their containers' counts (`identity` backs them for two containers without tables).
struct OverlapPairing {
    isingmc_states *b = nullptr;
    const uint32_t *slots_a = nullptr, *slots_b = nullptr;
    bool default_pairs = false;
    std::vector<uint32_t> identity;
};
// why these containers cannot be measured against each other ("" when they can; a == b: pairs inside one container)
IM_INTERNAL std::string overlaps_obstacle(const isingmc_states *a, const isingmc_states *b);
IM_INTERNAL int overlap_pairing(isingmc_states *a, isingmc_states *b, const uint32_t *slots_a, const uint32_t *slots_b, size_t n_pairs, OverlapPairing &P);
// why this class set cannot resolve the overlaps of a's replicas ("" when it can)
IM_INTERNAL std::string classes_obstacle(const isingmc_site_classes *classes, const isingmc_states *a);

// The overlap core: isingmc_overlaps, isingmc_overlaps_by_class and the records of the overlap series are one measurement, cut
// into the same batches and enqueued by the same two functions; they differ in where the workspace lives and in what becomes of
// the accumulators.
// One measurement: device slot tables, or nullptr for the pairs (2 p, 2 p + 1) of one container
struct OverlapJob {
    isingmc_states *a, *b; // b == a: pairs inside one container
    const uint32_t *d_sa, *d_sb;
    size_t n_pairs;
    bool link;                           // (the spin / link pass)
    const isingmc_site_classes *classes; // (the class pass; nullptr when there is none)
    bool default_pairs() const { return d_sa == nullptr; }
    size_t bins() const { return classes ? classes->n_tables * classes->n_classes : 0; }
};
// Its batches under a's cluster_workspace_bytes
struct OverlapPlan {
    size_t acc_pairs = 0, acc0 = 0; // accumulator columns of the spin / link launches and the column of pair 0
    size_t blocks = 0, batch = 0;   // packed containers with tables: pair blocks of 32 pairs and those of one batch (else batch = 0)
    size_t cols = 1, items = 0, col0 = 0, cbatch = 0; // by class: pair columns per item, items, the column of pair 0, items per batch
};
IM_INTERNAL OverlapPlan overlap_plan(const isingmc_states *a, size_t n_pairs, bool default_pairs, size_t bins);
// Its workspace: acc[2 acc_pairs] for the spin / link pass, cacc[cbatch cols bins] for the class pass, and where batch != 0 the
// gathered overlap words of one batch of either pass, words[batch n_pos] / words[cbatch n_pos]
struct OverlapWork {
    unsigned long long *acc, *cacc;
    uint32_t *words;
};
// What becomes of a finished batch of accumulators -- (accumulators, first column of the batch, columns in the batch) -- by
// reference to the caller's callable, which outlives the call it is passed to.  (No std::function: a record of the series
// must not allocate per batch.)
class OverlapSink {
    void *f;
    int (*call)(void *, const unsigned long long *, size_t, size_t);

public:
    template <typename F>
    OverlapSink(F &fn) : f(&fn), call([](void *p, const unsigned long long *acc, size_t c0, size_t n) { return (*static_cast<F *>(p))(acc, c0, n); }) {}
    int operator()(const unsigned long long *acc, size_t c0, size_t n) const { return call(f, acc, c0, n); }
};
// Enqueue on a's stream; the caller has joined the lanes and put a's stream behind b's.  The spin / link pass clears acc, counts
// into it and hands all acc_pairs columns to the sink once; the class pass does so batch by batch with cacc.
IM_INTERNAL int overlap_enqueue(const OverlapJob &J, const OverlapPlan &P, const OverlapWork &W, OverlapSink sink);
IM_INTERNAL int overlap_class_enqueue(const OverlapJob &J, const OverlapPlan &P, const OverlapWork &W, OverlapSink sink);
IM_INTERNAL int overlap_lanes_join(isingmc_states *a, isingmc_states *b); // both containers' sweeps so far on their main streams

// ---- recorders.hip (the periodic recorders as one table; the log core of the two series) -----------------------------------------
// Every recorder due at timestep s->t takes its sample, unless the attempt this call repeats took it already (with_strip_retry).
// after_strip: a call that may be repeated first waits for the strip launch before and checks it.  The status returned is that wait's
// alone; everything else goes into rc, and an error in rc ends the sampling.
IM_INTERNAL int recorders_sample(isingmc_states *s, bool after_strip, int &rc);
IM_INTERNAL int recorder_sample_now(isingmc_states *s, Recorder which); // that one recorder, if timestep s->t is its sample point
IM_INTERNAL int recorders_room_or_fail(const isingmc_states *s, size_t timesteps); // before a run enqueues anything: would a series run full in it?
IM_INTERNAL void recorders_restart(isingmc_states *s, uint64_t t);       // isingmc_states_set_timestep: the sample points are counted from t
IM_INTERNAL void recorders_replay_since(isingmc_states *s, uint64_t t0); // around the repeat of a call that started at t0
enum class RecorderRefusal { Append, Resample };
IM_INTERNAL const char *recorders_refusal(const isingmc_states *s, RecorderRefusal what); // the sentence of the first recorder that is on and objects, or nullptr
static inline size_t recorders_stretch(const isingmc_states *s) // timesteps from s->t up to and including the next sample point
{
    size_t n = std::numeric_limits<size_t>::max();
    for (const Periodic &p : s->rec) n = std::min(n, p.stretch(s->t));
    return n;
}
static inline bool recorders_any_on(const isingmc_states *s) { return recorders_stretch(s) != std::numeric_limits<size_t>::max(); } // (a sample point is ahead)

// The log of a series: `capacity` rows of `row` 8-byte entries on the device and the timestep of every row held.  Both series derive
// from it; `noun` ("overlap" / "observable") names them in the sentences, a->series[which] is the one that records on a period.
struct SeriesLog {
    isingmc_states *const a;
    const Recorder which;
    const char *const noun;
    size_t capacity = 0, row = 0;
    DevBlock<unsigned long long> d_log; // [capacity][row]
    std::vector<uint64_t> timesteps;    // of the rows: its size is the row count
    SeriesLog(isingmc_states *a_, Recorder which_, const char *noun_) : a(a_), which(which_), noun(noun_) {}
    unsigned long long *next_row() const { return d_log.get() + timesteps.size() * row; }
    bool periodic() const { return a->series[which] == this; }
    int period_off() { if (periodic()) { a->series[which] = nullptr; a->rec[which].every = 0; } return ISINGMC_OK; } // the rows stay
    int period_on(size_t every) { a->series[which] = this; a->rec[which].every = every; a->rec[which].restart(a->t); return ISINGMC_OK; }
};
IM_INTERNAL int series_budget_or_fail(const char *noun, long long budget_option, size_t capacity, unsigned long long row_bytes);
IM_INTERNAL int series_full_or_ok(const SeriesLog *L);          // fails when the log holds `capacity` rows
IM_INTERNAL int series_room_or_fail(const isingmc_states *s, Recorder which, size_t timesteps);
IM_INTERNAL int series_period_free_or_fail(const SeriesLog *L); // fails when another series of the kind holds the container's period
IM_INTERNAL int series_count(const SeriesLog *L, size_t *n_out, size_t *capacity_out);
IM_INTERNAL int series_reset(SeriesLog *L);
// get: rows in range, `refusal` (the caller's own, or nullptr), the wait for a's stream, the strip check; then the timesteps and rows
IM_INTERNAL int series_read(SeriesLog *L, size_t first, size_t n, const char *refusal, uint64_t *timesteps_out, bool want_rows, std::vector<unsigned long long> &rows);
IM_INTERNAL void series_unregister(SeriesLog *L); // destroy: drains a's stream and gives the period up

// ---- overlap_series.hip / observable_series.hip (the device-resident logs, one row per sample) ----------------------------------
IM_INTERNAL int osr_sample_enqueue(isingmc_states *s); // enqueue: one row of the container's periodic series at timestep s->t
IM_INTERNAL int obs_sample_enqueue(isingmc_states *s);
IM_INTERNAL bool obs_sample_by_rung(const isingmc_states *s); // the container's periodic observable series is one by rung

// ---- cluster_series.hip (the device-resident log of cluster-size moments, one row per non-local step) -----------------------------
// Around the batches of the non-local step at timestep s->t, of kind ISINGMC_CLUSTER_SERIES_SW / _ICM.  begin: with a live series
// of that kind, the next row cleared and *out pointing at it (first_slot, n_cols; the step sets slot0 per batch); else out->row
// stays nullptr and the step runs as without a series.  end (only behind a begin that gave a row): n_clusters, largest and sites
// out of the step's statistics -- stats[slot][2], minus[slot] or nullptr -- and the row counts.  Enqueue only.
IM_INTERNAL int cluster_series_begin(isingmc_states *s, int kind, ClusterMomentsOut *out);
IM_INTERNAL int cluster_series_end(isingmc_states *s, const ClusterMomentsOut &out, const uint32_t *stats, const uint32_t *minus);
IM_INTERNAL int cluster_series_room_or_fail(const isingmc_states *s, size_t timesteps); // before a run enqueues anything
IM_INTERNAL void cluster_series_replay_since(isingmc_states *s, uint64_t t0); // the repeat of a call that started at t0 writes its rows again
// why this container cannot take Swendsen-Wang steps / isoenergetic cluster moves ("" when it can) (nonlocal.hip)
IM_INTERNAL std::string cluster_obstacle(const isingmc_states *s);
IM_INTERNAL std::string icm_obstacle(const isingmc_states *s);

// ---- nonlocal.hip (Swendsen-Wang steps and isoenergetic cluster moves) -------------------------------------------------------
// What the non-local steps of ONE run_steps call keep between them: filled by the call's first such step, the device blocks in the
// call's DeviceScratch.  The host copies live as long as the call: they feed asynchronous copies.
struct NonlocalRun {
    ClusterWork cl{nullptr, nullptr, nullptr, nullptr};      // workspace of one batch: of replicas (cluster steps) or pairs (S9) of a lattice,
    PkClusterWork pk_cl{nullptr, nullptr, nullptr, nullptr}; // of replica groups of a packed container (S11),
    PkIcmWork pk_icm{nullptr, nullptr, nullptr};             // of replica groups for the isoenergetic move (S12)
    size_t batch = 0;                                        // items of that batch (0: no workspace yet)
    uint64_t *d_cl_thr = nullptr;                            // bond thresholds per counter slot (per-replica betas)
    std::vector<uint64_t> h_cl_thr{};
    uint32_t *d_icm_mask = nullptr;                          // packed containers: the moving pairs of every group
    std::vector<uint32_t> h_icm_mask{};
};
IM_INTERNAL bool is_cluster_step(const isingmc_states *s); // is timestep s->t a Swendsen-Wang step / an isoenergetic cluster move?
IM_INTERNAL bool is_icm_step(const isingmc_states *s);
// timestep s->t as that move and s->t++, nothing else.  beta: the call's beta of this step (not read with per-replica betas)
IM_INTERNAL int run_cluster_step(isingmc_states *s, NonlocalRun &n, DeviceScratch &scratch, double beta);
IM_INTERNAL int run_icm_step(isingmc_states *s, NonlocalRun &n, DeviceScratch &scratch);
IM_INTERNAL bool icm_unequal_pair_betas(const isingmc_states *s, const double *betas);
// the clauses every non-local move and measurement of a checkerboard lattice shares ("" when none applies)
IM_INTERNAL std::string lattice_obstacle(const isingmc_graph *g, const std::string &what, bool any_sign, bool labels = true);

// counter pairs of a measurement (measure_enqueue): one per (group, bit) slot of a packed container, one per replica otherwise
static inline size_t counter_slots(const isingmc_states *s) { return s->packed ? s->pk_slots() : s->R; }
static inline size_t counter_slot(const isingmc_states *s, size_t r) { return s->packed ? r + s->pk_bit0 : r; }
static inline double counters_energy(const isingmc_states *s, unsigned long long c0, unsigned long long c1)
{
    return s->packed ? pk_energy(s->g, s->rj, c0, c1) : lattice_energy(s->g, c0, c1);
}

// A synchronous call that may launch the strip kernel keeps the planes it started from: if a launch gives up (its workgroups
// were not all resident: a co-tenant, a CU mask), the planes and the clock are put back and the call is repeated, on the
// per-colour launches by then (strip_check has disabled the strip kernel of the object).
template <typename F>
static int with_strip_retry(isingmc_states *s, bool may_strip, F &&call)
{
    if (!may_strip) return strip_error(call());
    TRY(use_device(s->g->device));
    const uint64_t t0 = s->t;
    TRY(snapshot_take(s));
    s->strip.guard = true;
    const int rc = call();
    s->strip.guard = false;
    if (rc != STRIP_TIMED_OUT) return rc;
    TRY(snapshot_restore(s));
    recorders_replay_since(s, t0); // (the repeat skips the samples already in the sums and the rows already in the two series,
                                   //  and writes the rows of the cluster series again)
    s->t = t0;
    const int rc2 = strip_error(call());
    for (Periodic &p : s->rec) p.replay_to = 0;
    return rc2;
}
