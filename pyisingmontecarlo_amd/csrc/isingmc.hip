// libisingmc.so: replica containers and every Monte-Carlo launch of the C ABI of include/isingmc.h (gfx950 only).
// Host orchestration only -- every Monte-Carlo operation runs in the kernels of the lattice, general, packed, strip, spread,
// multi-class, one-degree and real-coupling translation units, behind their launchers.  There is no CPU fallback.
// (internal.hpp: how the host side is cut into translation units.)
#include "internal.hpp"

// ------------------------------------------------------------------------------------------------
// states
// ------------------------------------------------------------------------------------------------

static int lanes_reserve(isingmc_states *s, size_t n);
static int lanes_fork(isingmc_states *s, size_t n);

using step_policy::Family;
using step_policy::StepPath;
using step_policy::StepPlan;

// the kernel headers' bounds as the policy header states them
static_assert(step_policy::GEN_RESIDENT_BYTES == GEN_RESIDENT_MAX_BYTES && step_policy::LAT_RESIDENT_BYTES == LDS_RESIDENT_MAX_BYTES &&
              step_policy::LAT_MEASURE_SLOTS == MEASURE_SLOTS && step_policy::PACKED_MAX_DEG == PK_MAX_DEG &&
              step_policy::PACKED_MEASURE_POS == PK_MEASURE_POS_PER_THREAD && step_policy::STRIP_WAVES_PER_CU == STRIP_MAX_WAVES_PER_CU &&
              step_policy::MC_MODE_NONE == MC_NONE, "step_policy.hpp restates a bound of a kernel header with another value");

step_policy::GraphFacts graph_facts(const isingmc_graph *g)
{
    step_policy::GraphFacts f;
    const bool lattice = g->kind == ISINGMC_KIND_LATTICE2D;
    f.kind = lattice ? step_policy::GraphKind::Lattice2D : step_policy::GraphKind::General;
    f.mc_mode = g->mc_mode;
    f.nvars = g->nvars;
    f.state_words = g->state_words;
    f.wpr = g->geom.wpr; f.wpp = g->geom.wpp; f.H = g->geom.H; f.nquads = g->geom.nquads; f.cols_log2 = g->geom.cols_log2;
    f.vec = g->vec;
    f.uniform_sign = g->uniform_sign;
    f.n_colours = g->n_colours;
    for (size_t c = 0; c + 1 < g->class_base.size(); c++) f.largest_class = std::max<uint64_t>(f.largest_class, g->class_base[c + 1] - g->class_base[c]);
    f.n_pos = g->pk.n_pos;
    f.packed_ok = g->packed_ok;
    f.rj_ok = g->rj_ok;
    f.rj_slots = g->rj.slots;
    f.pk_uni_deg = g->pk_uni_deg;
    f.stable_path = g->stable_path;
    f.n_cu = g->n_cu;
    if (!lattice)
        for (int mode = 1; mode <= 2; mode++)
            f.gen_stage_words[mode] = gen_stage_words(g->gdev.n_pos, g->gen_edges2, g->gdev.bias != nullptr, g->w_is_float ? 4 : 8, mode);
    return f;
}

static step_policy::ContainerFacts container_facts(const isingmc_states *s) { return {s->R, s->groups, s->packed, s->rj, s->strip.disabled}; }

// replica-packed general path (defined further down)
static int pk_create(isingmc_states *s, const uint64_t *all_seeds, size_t first, size_t n, const uint8_t *initial_state);
static int pk_set_state(isingmc_states *s, size_t replica, const uint8_t *spins);
static int pk_set_betas(isingmc_states *s);
static int pk_append(isingmc_states *s, uint64_t seed, const uint8_t *initial_state);

// random start for replicas [first, first+count)
static int init_random(isingmc_states *s, size_t first, size_t count)
{
    const isingmc_graph *g = s->g;
    for (size_t r0 = first; r0 < first + count; r0 += MAX_GRID_Y) {
        const size_t n = std::min(MAX_GRID_Y, first + count - r0);
        if (g->kind == ISINGMC_KIND_LATTICE2D) HIP_TRY(lat_launch_init(s->stream, s->d_state, g->geom, s->d_keys, uint32_t(r0), uint32_t(n)));
        else HIP_TRY(gen_launch_init(s->stream, s->d_state, g->gdev, s->d_keys, uint32_t(r0), uint32_t(n)));
    }
    return ISINGMC_OK;
}

static int upload_state(isingmc_states *s, size_t first, size_t count, const uint8_t *spins)
{
    s->meas_fresh = false;
    const size_t sw = s->g->state_words;
    std::vector<uint32_t> words(sw);
    pack_state(s->g, spins, words.data());
    // the same row for every replica: one copy per batch of rows (a population of 2^20 small lattices took one copy per ROW)
    const size_t batch = std::min(count, std::max<size_t>(1, (size_t(1) << 22) / sw)); // at most 16 MiB of host rows
    std::vector<uint32_t> rows(batch * sw);
    for (size_t k = 0; k < batch; k++) std::copy(words.begin(), words.end(), rows.begin() + k * sw);
    for (size_t r = first; r < first + count; r += batch)
        HIP_TRY(hipMemcpyAsync(s->d_state + r * sw, rows.data(), std::min(batch, first + count - r) * sw * sizeof(uint32_t),
                               hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return ISINGMC_OK;
}

static int reserve(isingmc_states *s, size_t cap)
{
    if (cap <= s->cap) return ISINGMC_OK;
    const isingmc_graph *g = s->g;
    DevBlock<uint32_t> d_state; // a failure below frees the new buffers
    DevBlock<uint2> d_keys;
    TRY(dev_alloc(d_state, cap * g->state_words));
    TRY(dev_alloc(d_keys, cap));
    // enqueue-only calls (isingmc_pt_*, the sampling loop) may still be running on the engine's non-blocking stream, which the
    // null-stream copies below are NOT ordered against; and the old blocks go back to the cache at the end
    HIP_TRY(stream_quiesce(s->stream));
    for (hipStream_t st : s->lanes) HIP_TRY(stream_quiesce(st));
    if (s->sampling.copy_stream) HIP_TRY(stream_quiesce(s->sampling.copy_stream));
    if (s->R) {
        HIP_TRY(hipMemcpy(d_state, s->d_state, s->R * g->state_words * sizeof(uint32_t), hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(d_keys, s->d_keys, s->R * sizeof(uint2), hipMemcpyDeviceToDevice));
        HIP_TRY(hipDeviceSynchronize()); // device-to-device copies may still run when hipMemcpy returns; the old blocks are recycled below
    }
    s->d_state = std::move(d_state);
    s->d_keys = std::move(d_keys);
    s->d_thr.reset(); s->d_beta.reset(); s->d_meas.reset(); // the old sizes go before the new ones come
    s->d_pe.reset(); s->d_oe.reset(); s->d_pm.reset(); s->d_om.reset();
    s->strip.d_fin.reset(); // [cap] too: launch_strip allocates it again
    TRY(dev_alloc(s->d_thr, cap));
    TRY(dev_alloc(s->d_beta, cap));
    if (g->kind == ISINGMC_KIND_LATTICE2D) {
        TRY(dev_alloc(s->d_meas, 2 * cap));
        s->meas_zero = false;
    } else {
        s->n_partials = (g->gdev.n_pos + 255) / 256;
        TRY(dev_alloc(s->d_pe, cap * s->n_partials));
        TRY(dev_alloc(s->d_pm, cap * s->n_partials));
        TRY(dev_alloc(s->d_oe, cap));
        TRY(dev_alloc(s->d_om, cap));
    }
    s->cap = cap;
    return ISINGMC_OK;
}

static int add_replicas(isingmc_states *s, size_t count, const uint64_t *seeds, const uint8_t *initial_state)
{
    const size_t first = s->R;
    if (first + count > s->cap) TRY(reserve(s, std::max(first + count, s->cap + s->cap / 2)));
    std::vector<uint2> keys(count);
    for (size_t i = 0; i < count; i++) keys[i] = make_uint2(uint32_t(seeds[i]), uint32_t(seeds[i] >> 32));
    if (count) HIP_TRY(hipMemcpy(s->d_keys + first, keys.data(), count * sizeof(uint2), hipMemcpyHostToDevice));
    s->R = first + count;
    if (initial_state) TRY(upload_state(s, first, count, initial_state));
    else {
        TRY(init_random(s, first, count));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    return ISINGMC_OK;
}

// Experiments [first, first + count) of n_total (one shard of the rayon fan-out of lattice.rs:192-197).  Everything that
// shapes a trajectory is decided from the GLOBAL experiment index and count -- the packed / per-replica choice, the
// 32-replica group a replica belongs to, the group's key and the replica's bit -- so that the results do not depend on
// how the experiments are cut into shards.  A shard that starts or ends inside a group simulates the whole group
// (the replicas of a group share Philox words and number their ties together).
extern "C" int isingmc_states_create_range(isingmc_graph *g, size_t n_total, const uint64_t *all_seeds, size_t first,
                                           size_t count, const uint8_t *initial_state, isingmc_states **states_out)
{
    if (!g || !states_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    *states_out = nullptr;
    if (n_total && !all_seeds) return fail(ISINGMC_ERR_INVALID, "seeds is NULL");
    if (first > n_total || count > n_total - first) return fail(ISINGMC_ERR_INVALID, "replica range out of bounds");
    TRY(use_device(g->device));
    auto s = std::make_unique<isingmc_states>();
    s->g = g;
    TRY(stream_create(s->stream));
    TRY(event_create(s->ev0));
    TRY(event_create(s->ev1));
    TRY(lanes_reserve(s.get(), 2)); // created up front: the first multi-lane run must not pay for stream creation
    s->n_total = n_total;
    s->first = first;
    s->opt = Options::from_env();
    const Family family = step_policy::choose_family(graph_facts(g), s->opt, count ? n_total : 0); // (an empty shard: one replica per word set)
    if (family == Family::PackedBits || family == Family::PackedReal) {
        s->rj = family == Family::PackedReal;
        TRY(pk_create(s.get(), all_seeds, first, count, initial_state));
    } else {
        TRY(reserve(s.get(), std::max<size_t>(count, 1)));
        TRY(add_replicas(s.get(), count, all_seeds + first, initial_state));
    }
    // ISINGMC_PHILOX_ROUNDS is the process's default for the containers the option serves; the others draw with ten rounds
    // whatever it says (isingmc_states_philox_rounds tells).  A value that is no round count fails the creation.
    if (s->opt.philox_rounds != 7 && s->opt.philox_rounds != 10)
        return fail(ISINGMC_ERR_INVALID, "ISINGMC_PHILOX_ROUNDS=" + std::to_string(s->opt.philox_rounds) + ": the sweeps draw with 7 or 10 Philox rounds");
    if (!philox_rounds_served_by(s.get())) s->opt.philox_rounds = 10;
    *states_out = s.release();
    return ISINGMC_OK;
}

extern "C" int isingmc_states_create(isingmc_graph *g, size_t n_replicas, const uint64_t *seeds,
                                     const uint8_t *initial_state, isingmc_states **states_out)
{
    return isingmc_states_create_range(g, n_replicas, seeds, 0, n_replicas, initial_state, states_out);
}

extern "C" int isingmc_states_append(isingmc_states *s, uint64_t seed, const uint8_t *initial_state)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (s->has_betas) return fail(ISINGMC_ERR_INVALID, "clear the per-replica betas before appending replicas");
    if (const char *why = recorders_refusal(s, RecorderRefusal::Append)) return fail(ISINGMC_ERR_INVALID, why);
    TRY(use_device(s->g->device));
    if (s->packed) return pk_append(s, seed, initial_state);
    return add_replicas(s, 1, &seed, initial_state);
}

extern "C" int isingmc_states_set_state(isingmc_states *s, size_t replica, const uint8_t *state)
{
    if (!s || !state) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    if (replica >= s->R) return fail(ISINGMC_ERR_INVALID, "replica index out of range");
    TRY(use_device(s->g->device));
    if (s->packed) return pk_set_state(s, replica, state);
    return upload_state(s, replica, 1, state);
}

// kernel family: 0 checkerboard lattice kernels, 1 f64 CSR (one replica per word set), 2 replica-packed bit-sliced, 3 replica-packed real-coupling
extern "C" int isingmc_states_family(const isingmc_states *s, int *family_out)
{
    if (!s || !family_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    *family_out = s->g->kind == ISINGMC_KIND_LATTICE2D ? 0 : !s->packed ? 1 : s->rj ? 3 : 2;
    return ISINGMC_OK;
}

// ... and the family a container of n_experiments created NOW on this graph would take (the environment's switches as they are)
extern "C" int isingmc_graph_family_for(const isingmc_graph *g, size_t n_experiments, int *family_out)
{
    if (!g || !family_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    *family_out = int(step_policy::choose_family(graph_facts(g), Options::from_env(), n_experiments));
    return ISINGMC_OK;
}

extern "C" size_t isingmc_states_count(const isingmc_states *s) { return s ? s->R : 0; }

extern "C" uint64_t isingmc_states_timestep(const isingmc_states *s) { return s ? s->t : 0; }

extern "C" int isingmc_states_set_timestep(isingmc_states *s, uint64_t t)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    // the counter words hold 48 bits of t (philox.hpp ctr2: t_lo in word 0, bits 32..47 beside the colour / call index)
    if (t >> 48) return fail(ISINGMC_ERR_INVALID, "timestep counter must be below 2^48");
    TRY(use_device(s->g->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->t = t;
    recorders_restart(s, t); // the sample points of the moment sums and of the periodic series (S21, S22) are counted from here
    return ISINGMC_OK;
}

extern "C" void isingmc_states_destroy(isingmc_states *s) { delete s; }

bool philox_rounds_served_by(const isingmc_states *s)
{
    return !s->packed && s->g->kind == ISINGMC_KIND_LATTICE2D && s->g->mc_mode == MC_NONE;
}

// the option "philox_rounds": a refusal leaves the value as it was
static int philox_rounds_set(isingmc_states *s, long value)
{
    if (value != 7 && value != 10)
        return fail(ISINGMC_ERR_INVALID, "philox_rounds = " + std::to_string(value) + ": the sweeps draw with 7 or 10 Philox rounds");
    if (value == 7 && !philox_rounds_served_by(s)) {
        const isingmc_graph *g = s->g;
        const std::string family = s->packed ? (s->rj ? "the replica-packed real-coupling family" : "the replica-packed bit-sliced family")
                                   : g->kind != ISINGMC_KIND_LATTICE2D ? "the f64 CSR family"
                                   : "the multi-class checkerboard kernels (a field, open boundaries or two |J|)";
        return fail(ISINGMC_ERR_INVALID, "philox_rounds = 7 serves the periodic, field-free, one-|J| checkerboard lattices alone; this container runs on " +
                                             family + ", which draws with ten rounds");
    }
    s->opt.philox_rounds = int(value);
    return ISINGMC_OK;
}

extern "C" int isingmc_states_set_option(isingmc_states *s, const char *name, long value)
{
    if (!s || !name) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    const std::string n(name);
    const std::string bare = option_bare_name(n); // as Options::set reads it
    for (const char *family : {"force_real", "disable_real", "force_packed", "disable_packed"})
        if (bare == family) // (the whole name: "disable_packed_uniform" is a switch of its own, eight characters longer)
            return fail(ISINGMC_ERR_INVALID, "the kernel family of a container is fixed when it is created (set ISINGMC_" + std::string(family) +
                                                 " in the environment before isingmc_states_create)");
    if (bare == "philox_rounds") return philox_rounds_set(s, value);
    if (bare == "autocorr_bytes") { s->opt.autocorr_bytes = value; return ISINGMC_OK; } // (outside Options::table(), as options.hpp says)
    if (!s->opt.set(n, value)) return fail(ISINGMC_ERR_INVALID, "unknown option '" + n + "'");
    return ISINGMC_OK;
}

extern "C" int isingmc_graph_philox_rounds(const isingmc_graph *g, int *rounds_out)
{
    if (!g || !rounds_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    const int env = Options::from_env().philox_rounds; // (a value that is no round count fails the creation itself)
    *rounds_out = env == 7 && g->kind == ISINGMC_KIND_LATTICE2D && g->mc_mode == MC_NONE ? 7 : 10; // a recognised lattice never runs packed
    return ISINGMC_OK;
}

extern "C" int isingmc_states_philox_rounds(const isingmc_states *s, int *rounds_out)
{
    if (!s || !rounds_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    *rounds_out = s->opt.philox_rounds;
    return ISINGMC_OK;
}

extern "C" int isingmc_states_set_betas(isingmc_states *s, const double *beta_per_replica)
{
    return set_betas(s, beta_per_replica, false);
}

// all_equal: the caller passes one beta R times (run_sampling) -- then a shard that cuts a replica group is fine
int set_betas(isingmc_states *s, const double *beta_per_replica, bool all_equal)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (!beta_per_replica) {
        s->has_betas = false;
        s->betas.clear();
        return ISINGMC_OK;
    }
    for (size_t r = 0; r < s->R; r++)
        if (!std::isfinite(beta_per_replica[r])) return fail(ISINGMC_ERR_INVALID, "beta must be finite");
    if (s->icm.every && icm_unequal_pair_betas(s, beta_per_replica))
        return fail(ISINGMC_ERR_INVALID, "isoenergetic cluster moves are switched on: the two replicas of every pair (2 p, 2 p + 1) need equal betas");
    TRY(use_device(s->g->device));
    if (!all_equal) { // one beta R times is as good as a uniform beta: any cut of a group is fine then
        all_equal = true;
        for (size_t r = 1; r < s->R; r++) all_equal &= beta_per_replica[r] == beta_per_replica[0];
    }
    if (s->packed && !s->rj && !all_equal && (s->pk_bit0 != 0 || ((s->first + s->R) % 32 != 0 && s->first + s->R != s->n_total)))
        // the replicas of a group number their ties together: a group's trajectory depends on all 32 betas, and this
        // shard only knows its own (the real-coupling path decides every replica on its own: any cut is fine there)
        return fail(ISINGMC_ERR_INVALID, "per-replica betas on a replica-packed shard: the shard must start and end on multiples of 32 experiments (or at the last experiment)");
    s->betas.assign(beta_per_replica, beta_per_replica + s->R);
    if (s->packed) {
        if (s->R) TRY(pk_set_betas(s));
        s->has_betas = true;
        return ISINGMC_OK;
    }
    if (s->g->kind == ISINGMC_KIND_LATTICE2D && s->g->mc_mode != MC_NONE) {
        std::vector<LatThrMC> thr(s->R);
        for (size_t r = 0; r < s->R; r++) thr[r] = lattice_thresholds_mc(s->g, s->betas[r]);
        HIP_TRY(stream_quiesce(s->stream)); // the old table may still be read by enqueued timesteps; its block is recycled
        s->d_thr_mc.reset();
        TRY(dev_alloc(s->d_thr_mc, s->cap));
        if (s->R) HIP_TRY(hipMemcpyAsync(s->d_thr_mc, thr.data(), s->R * sizeof(LatThrMC), hipMemcpyHostToDevice, s->stream));
    } else if (s->g->kind == ISINGMC_KIND_LATTICE2D) {
        std::vector<LatThr> thr(s->R);
        for (size_t r = 0; r < s->R; r++) thr[r] = lattice_thresholds(s->betas[r], s->g->jabs);
        if (s->R) HIP_TRY(hipMemcpyAsync(s->d_thr, thr.data(), s->R * sizeof(LatThr), hipMemcpyHostToDevice, s->stream));
    } else if (s->R) {
        HIP_TRY(hipMemcpyAsync(s->d_beta, s->betas.data(), s->R * sizeof(double), hipMemcpyHostToDevice, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->has_betas = true;
    return ISINGMC_OK;
}

// ------------------------------------------------------------------------------------------------
// replica-packed general path (packed_kernels.hpp): state = uint32[groups][n_pos], group g = replicas
// 32g .. 32g+31, keyed by the seed of its first replica
// ------------------------------------------------------------------------------------------------

// threshold table of one group for per-replica betas (beta_of(r) for r = 0..31)
template <typename F>
static void pk_fill_table(uint32_t *tab, double jabs, F &&beta_of)
{
    std::fill(tab, tab + PK_TAB_WORDS, 0u);
    for (uint32_t m = 1; m <= uint32_t(PK_MAX_DEG); m++)
        for (uint32_t r = 0; r < 32; r++) {
            const uint64_t T = threshold_fixed(beta_of(r), 2.0 * jabs * double(m));
            if (T >> THR_BITS) tab[PK_TAB_ALL + m - 1] |= 1u << r;
            const uint32_t hi = uint32_t(T >> 32) & ((1u << N_PLANES) - 1);
            for (int p = 0; p < N_PLANES; p++)
                if ((hi >> (N_PLANES - 1 - p)) & 1u) tab[PK_TAB_TBW + (m - 1) * N_PLANES + p] |= 1u << r;
            tab[PK_TAB_LO + (m - 1) * 32 + r] = uint32_t(T);
        }
    // (meaningful when every replica has the same beta: the one-degree kernel's uniform-beta instantiation reads them)
    for (uint32_t idx = 0; idx < uint32_t(PK_MAX_DEG) * N_PLANES; idx++)
        if (tab[PK_TAB_TBW + idx] & 1u) tab[PK_TAB_SEL + (idx >> 5)] |= 1u << (idx & 31);
}

static int pk_create(isingmc_states *s, const uint64_t *all_seeds, size_t first, size_t n, const uint8_t *initial_state)
{
    const isingmc_graph *g = s->g;
    s->packed = true;
    const size_t group0 = first / 32; // global groups [group0, group0 + groups) intersect this shard
    s->pk_bit0 = first % 32;
    s->groups = (s->pk_bit0 + n + 31) / 32;
    s->R = s->cap = n;
    TRY(dev_alloc(s->d_state, s->groups * g->pk.n_pos));
    TRY(dev_alloc(s->d_keys, s->groups));
    TRY(dev_alloc(s->d_meas, 2 * s->pk_slots()));
    s->meas_zero = false;
    std::vector<uint2> keys(s->groups);
    for (size_t k = 0; k < s->groups; k++) { // a group is keyed by the seed of its first GLOBAL replica
        const uint64_t seed = all_seeds[32 * (group0 + k)];
        keys[k] = make_uint2(uint32_t(seed), uint32_t(seed >> 32));
    }
    HIP_TRY(hipMemcpy(s->d_keys, keys.data(), keys.size() * sizeof(uint2), hipMemcpyHostToDevice));
    if (initial_state) { // every replica starts from the same configuration: a word is all ones or all zeros
        std::vector<uint32_t> words(g->pk.n_pos, 0u);
        for (uint64_t i = 0; i < g->nvars; i++) words[g->pos[i]] = initial_state[i] ? 0xFFFFFFFFu : 0u;
        for (size_t k = 0; k < s->groups; k++)
            HIP_TRY(hipMemcpy(s->d_state + k * g->pk.n_pos, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    } else {
        for (size_t g0 = 0; g0 < s->groups; g0 += MAX_GRID_Y) {
            const size_t ng = std::min(MAX_GRID_Y, s->groups - g0);
            HIP_TRY(pk_launch_init(s->stream, s->d_state, g->pk, s->d_keys, uint32_t(g0), uint32_t(ng)));
        }
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    return ISINGMC_OK;
}

// ClassicIsing.add_graph (classicising.rs:62-79) on a replica-packed container.  A replica appended into a partly filled
// group starts from the random start of its bit position (the "PKIN" words of the group's key) NOW, at the current timestep --
// a fresh experiment, as GraphState::new gives the reference (classicising.rs:73) and as every other path here does; with an
// initial_state it is set explicitly.  (Bit-sliced path: a group simulates all of its 32 bit positions from the moment it is
// created -- the spec numbers ties over whole groups -- so until round 3 the new replica took over the chain its bit had been
// running: a thermalised start where the caller asked for a random one.)  Replica 32 g opens a new group keyed by its seed,
// randomly started now.  Only whole containers grow (not shards of a larger set of experiments).
static int pk_append(isingmc_states *s, uint64_t seed, const uint8_t *initial_state)
{
    const isingmc_graph *g = s->g;
    if (s->first != 0 || s->n_total != s->R) return fail(ISINGMC_ERR_INVALID, "a shard of a larger set of experiments cannot grow");
    const size_t slot = s->R;
    if (slot % 32 == 0) { // a new group
        const size_t groups = s->groups + 1;
        DevBlock<uint32_t> d_state; // a failure below frees the new buffers
        DevBlock<uint2> d_keys;
        DevBlock<unsigned long long> d_meas;
        TRY(dev_alloc(d_state, groups * g->pk.n_pos));
        TRY(dev_alloc(d_keys, groups));
        TRY(dev_alloc(d_meas, 2 * 32 * groups));
        HIP_TRY(hipStreamSynchronize(s->stream));
        HIP_TRY(hipMemcpy(d_state, s->d_state, s->groups * g->pk.n_pos * sizeof(uint32_t), hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(d_keys, s->d_keys, s->groups * sizeof(uint2), hipMemcpyDeviceToDevice));
        HIP_TRY(hipDeviceSynchronize()); // as in reserve(): the old blocks go back to the cache below
        const uint2 key = make_uint2(uint32_t(seed), uint32_t(seed >> 32));
        HIP_TRY(hipMemcpy(d_keys + s->groups, &key, sizeof key, hipMemcpyHostToDevice));
        s->d_state = std::move(d_state);
        s->d_keys = std::move(d_keys);
        s->d_meas = std::move(d_meas);
        s->meas_zero = false;
        s->d_tab.reset(); // per-group tables: rebuilt by the next set_betas
        s->d_pk_philox.reset(); // rows per group count
        s->pk_philox_steps = 0;
        s->d_rj_betas.reset();
        HIP_TRY(pk_launch_init(s->stream, s->d_state, g->pk, s->d_keys, uint32_t(s->groups), 1));
        HIP_TRY(hipStreamSynchronize(s->stream));
        s->groups = groups;
    }
    s->R = s->cap = s->n_total = slot + 1;
    if (initial_state) TRY(pk_set_state(s, slot, initial_state));
    else if (slot % 32 != 0) {
        // (real-coupling path: the bits of a group this container does not own are not simulated at all, rj_sweep_kernel PARTIAL,
        //  so the column holds whatever it held)
        HIP_TRY(pk_launch_init_replica(s->stream, s->d_state, g->pk, s->d_keys, uint32_t(slot / 32), uint32_t(slot % 32)));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    return ISINGMC_OK;
}

static int pk_set_state(isingmc_states *s, size_t replica, const uint8_t *spins)
{
    const isingmc_graph *g = s->g;
    std::vector<uint32_t> bits(g->state_words, 0u);
    for (uint64_t i = 0; i < g->nvars; i++)
        if (spins[i]) bits[g->pos[i] >> 5] |= 1u << (g->pos[i] & 31);
    DeviceScratch scratch(s->stream);
    uint32_t *d_bits = nullptr;
    TRY(scratch.alloc(&d_bits, bits.size()));
    HIP_TRY(hipMemcpy(d_bits, bits.data(), bits.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(pk_launch_set_replica(s->stream, s->d_state, g->pk.n_pos, d_bits, uint32_t((replica + s->pk_bit0) / 32),
                                  uint32_t((replica + s->pk_bit0) % 32)));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return ISINGMC_OK;
}

static int pk_set_betas(isingmc_states *s)
{
    if (s->rj) { // one acceptance scale per (group, bit); bits this shard does not own take the nearest owned replica's
        std::vector<RjBeta> tab(32 * s->groups);
        for (size_t sl = 0; sl < tab.size(); sl++) {
            const size_t r = sl < s->pk_bit0 ? 0 : std::min(s->R - 1, sl - s->pk_bit0);
            rj_beta(s->betas[r], s->g->rj_k, &tab[sl].shift, &tab[sl].mant);
        }
        if (!s->d_rj_betas) TRY(dev_alloc(s->d_rj_betas, tab.size()));
        HIP_TRY(hipStreamSynchronize(s->stream)); // no launch may still be reading the old scales
        HIP_TRY(hipMemcpy(s->d_rj_betas, tab.data(), tab.size() * sizeof(RjBeta), hipMemcpyHostToDevice));
        return ISINGMC_OK;
    }
    std::vector<uint32_t> tabs(s->groups * PK_TAB_WORDS);
    for (size_t k = 0; k < s->groups; k++)
        pk_fill_table(tabs.data() + k * PK_TAB_WORDS, s->g->jabs,
                      [&](uint32_t r) { return s->betas[std::min(s->R - 1, 32 * k + r)]; }); // pk_bit0 == 0 (checked by the caller)
    if (!s->d_tab) TRY(dev_alloc(s->d_tab, tabs.size())); // groups is fixed for the life of a packed container (no append): allocated once
    HIP_TRY(hipStreamSynchronize(s->stream)); // no launch may still be reading the old tables
    HIP_TRY(hipMemcpy(s->d_tab, tabs.data(), tabs.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return ISINGMC_OK;
}

// The acceptance tables of n betas on the device, for calls that run a schedule without waiting on the host between its
// temperatures (isingmc_pa_run): entry k serves run_steps through isingmc_states::step_preset.  Blocking uploads, before the
// schedule is enqueued; the blocks belong to `scratch`.
int step_presets_build(isingmc_states *s, const double *betas, size_t n, DeviceScratch &scratch, std::vector<StepPreset> &out)
{
    const isingmc_graph *g = s->g;
    out.assign(n, StepPreset{});
    if (s->packed && s->rj) {
        std::vector<RjBeta> h(n);
        for (size_t k = 0; k < n; k++) rj_beta(betas[k], g->rj_k, &h[k].shift, &h[k].mant);
        RjBeta *d = nullptr;
        TRY(scratch.alloc(&d, n));
        HIP_TRY(hipMemcpy(d, h.data(), n * sizeof(RjBeta), hipMemcpyHostToDevice));
        for (size_t k = 0; k < n; k++) out[k].rj = d + k;
    } else if (s->packed) {
        std::vector<uint32_t> h(n * PK_TAB_WORDS);
        for (size_t k = 0; k < n; k++) pk_fill_table(h.data() + k * PK_TAB_WORDS, g->jabs, [&](uint32_t) { return betas[k]; });
        uint32_t *d = nullptr;
        TRY(scratch.alloc(&d, h.size()));
        HIP_TRY(hipMemcpy(d, h.data(), h.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        for (size_t k = 0; k < n; k++) out[k].pk_tabs = d + k * PK_TAB_WORDS;
    } else {
        std::vector<LatThr> h(n);
        for (size_t k = 0; k < n; k++) h[k] = lattice_thresholds(betas[k], g->jabs);
        LatThr *d = nullptr;
        TRY(scratch.alloc(&d, n));
        HIP_TRY(hipMemcpy(d, h.data(), n * sizeof(LatThr), hipMemcpyHostToDevice));
        for (size_t k = 0; k < n; k++) out[k].thr = d + k;
    }
    return ISINGMC_OK;
}

// real-coupling path: one launch per colour class; a workgroup walks several 256-position blocks (it loads the log table once)
static void rj_launch_timestep(isingmc_states *s, const RjBeta *betas, uint32_t beta_stride, size_t gb, size_t ge, hipStream_t stream)
{
    const isingmc_graph *g = s->g;
    const int target_wgs = s->opt.real_target_wgs;
    for (uint32_t c = 0; c < g->n_colours; c++) {
        const uint32_t b = uint32_t(g->class_base[c]), e = g->class_real_end[c];
        if (e == b) continue;
        const size_t threads = rj_threads(g->rj.slots);
        const size_t nblocks = (size_t(e - b) + threads - 1) / threads;
        // The first and the last group of the container may own only part of their 32 replica bits (few experiments, a shard
        // cut inside a group): those groups get launches of their own that draw only the Philox calls of the owned bits.
        const auto quads_of = [&](size_t grp, uint32_t *lo, uint32_t *hi) {
            const size_t lo_bit = grp == 0 ? s->pk_bit0 : 0;
            const size_t hi_bit = grp + 1 == s->groups ? (s->pk_bit0 + s->R - 1) % 32 + 1 : 32;
            *lo = uint32_t(lo_bit / 4);
            *hi = uint32_t((hi_bit + 3) / 4);
        };
        for (size_t g0 = gb; g0 < ge;) {
            uint32_t q_lo, q_hi;
            quads_of(g0, &q_lo, &q_hi);
            size_t ng = 1; // extend over the following groups with the same quads (all the whole groups in the middle)
            for (uint32_t l2, h2; g0 + ng < ge && ng < MAX_GRID_Y; ng++) {
                quads_of(g0 + ng, &l2, &h2);
                if (l2 != q_lo || h2 != q_hi) break;
            }
            const size_t gx0 = std::min(nblocks, std::max<size_t>(1, (size_t(target_wgs) + ng - 1) / ng));
            const size_t per = (nblocks + gx0 - 1) / gx0, gx = (nblocks + per - 1) / per; // equal shares, no short last round
            (void)rj_launch_sweep(dim3(unsigned(gx), unsigned(ng)), stream, s->d_state + g0 * g->pk.n_pos, g->rj, b, e, s->t,
                                  s->d_keys + g0, betas + (beta_stride ? g0 * beta_stride : 0), beta_stride, q_lo, q_hi);
            g0 += ng;
        }
    }
}

static int pk_launch_timestep(isingmc_states *s, const uint32_t *tabs, uint32_t tab_stride, const uint32_t *philox_tab, size_t gb, size_t ge,
                               hipStream_t stream)
{
    const isingmc_graph *g = s->g;
    const bool no_uni = s->opt.disable_packed_uniform != 0; // A/B switch: results are the same either way
    for (uint32_t c = 0; c < g->n_colours; c++) {
        const uint32_t b = uint32_t(g->class_base[c]), e = uint32_t(g->class_base[c + 1]);
        if (e == b) continue;
        // blocks of real sites of a one-degree graph: the specialised kernel; the class's padded tail (and
        // every other graph): the general one.  tab_stride == 0 <=> one table, one beta for every replica.
        const uint32_t mid = g->pk_uni_deg && !no_uni ? g->pk_class_full[c] : b;
        for (size_t g0 = gb; g0 < ge; g0 += MAX_GRID_Y) {
            const size_t ng = std::min(MAX_GRID_Y, ge - g0);
            if (mid > b)
                (void)pk_uni_launch_sweep(g->pk_uni_deg, tab_stride == 0, g->pk_uni_pmj, uint32_t(ng), stream,
                                          s->d_state + g0 * g->pk.n_pos, g->pk, g->pk_uni, b, mid, s->t, s->d_keys + g0,
                                          tabs + (tab_stride ? g0 * tab_stride : 0), tab_stride,
                                          philox_tab + g0 * pk_uni_philox_table_words(), g->pk_class_table[c] != 0);
            if (e > mid)
                HIP_TRY(pk_launch_sweep(uint32_t(ng), stream, s->d_state + g0 * g->pk.n_pos, g->pk, mid, e, s->t, s->d_keys + g0,
                                        tabs + (tab_stride ? g0 * tab_stride : 0), tab_stride));
        }
    }
    return ISINGMC_OK;
}


// energy of one replica of a packed container from the counters of its slot
double pk_energy(const isingmc_graph *g, bool rj, unsigned long long c0, unsigned long long c1)
{
    // real-coupling path: c0, c1 = -2 x the hi / lo level sums of the energy (exact, even integers; rj_measure_kernel, run once
    // per level): E = (2^kE hi + 2^(kE - 24) lo) + self loops -- the energy of the ORIGINAL couplings to Fmax 2^-54 per term
    if (rj) return (std::ldexp(double(-(int64_t(c0) / 2)), g->rj_k_energy) + std::ldexp(double(-(int64_t(c1) / 2)), g->rj_k_energy - RJ_ENERGY_LO_BITS)) + g->self_energy;
    (void)c1;
    // bit-sliced path: E = |J| (undirected bonds - 2 satisfied) + self loops; c0 = directed satisfied count (doubled)
    return g->jabs * (double(int64_t(g->n_directed / 2)) - double(int64_t(c0))) + g->self_energy;
}

// packed words -> one byte per spin, replica by replica
int pk_get_states(isingmc_states *s, uint8_t *states_out, size_t replica_stride_bytes, uint32_t *packed_out, const uint32_t *d_words)
{
    const isingmc_graph *g = s->g;
    std::vector<uint32_t> words(s->groups * g->pk.n_pos);
    HIP_TRY(hipMemcpyAsync(words.data(), d_words ? d_words : s->d_state, words.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    parallel_for(s->R, [&](size_t r) {
        const uint32_t *w = words.data() + ((r + s->pk_bit0) / 32) * g->pk.n_pos;
        const uint32_t bit = uint32_t((r + s->pk_bit0) % 32);
        if (states_out) {
            uint8_t *out = states_out + r * replica_stride_bytes;
            for (uint64_t i = 0; i < g->nvars; i++) out[i] = (w[g->pos[i]] >> bit) & 1u;
        }
        if (packed_out) { // the per-replica layout of the thread-per-site path (bit-packed by position)
            uint32_t *out = packed_out + r * g->state_words;
            std::fill(out, out + g->state_words, 0u);
            for (uint64_t i = 0; i < g->nvars; i++)
                out[g->pos[i] >> 5] |= ((w[g->pos[i]] >> bit) & 1u) << (g->pos[i] & 31);
        }
    });
    return ISINGMC_OK;
}

// ------------------------------------------------------------------------------------------------
// sweeps
// ------------------------------------------------------------------------------------------------
// resident_wgs: workgroups of the looping kernel the device holds at once (sweep_resident_wgs, once per run call)
static int launch_lat_sweep(isingmc_states *s, const step_policy::GraphFacts &G, int resident_wgs, uint32_t colour, const LatThr &thr, uint64_t t_arg)
{
    const isingmc_graph *g = s->g;
    // diagnostic: ISINGMC_DEBUG_SWEEP_LDS=<bytes> of unused LDS per workgroup lowers the occupancy
    const unsigned dbg_lds = unsigned(std::max(0, s->opt.debug_sweep_lds));
    const bool uni = step_policy::uniform_mapping(G); // what the looping kernel needs
    // replicas are independent: with n_lanes > 1 the replica blocks go to different streams, so that the
    // launch gap / ramp / tail of one block's half-sweep overlaps the other blocks' work
    const size_t per_lane = (s->R + s->n_lanes - 1) / s->n_lanes;
    for (size_t lane = 0; lane < s->n_lanes; lane++) {
        const size_t lo = lane * per_lane, hi = std::min(s->R, lo + per_lane);
        hipStream_t stream = s->n_lanes > 1 ? s->lanes[lane] : s->stream;
        for (size_t r0 = lo; r0 < hi; r0 += MAX_GRID_Y) {
            const size_t n = std::min(MAX_GRID_Y, hi - r0);
            const uint32_t iters = uni ? step_policy::sweep_iters(G, s->opt, s->R, n, resident_wgs) : 1;
            HIP_TRY(lat_launch_sweep(g->vec, !g->uniform_sign, iters, uint32_t(n), dbg_lds, stream, s->d_state + r0 * g->state_words, g->geom,
                                     colour, t_arg, s->d_keys + r0, thr, s->has_betas ? s->d_thr + r0 : nullptr, g->d_jneg, g->jneg_uniform,
                                     s->opt.philox_rounds));
        }
    }
    return ISINGMC_OK;
}

// fork: the lanes wait for everything queued on the main stream; join: the main stream waits for the lanes
static int lanes_reserve(isingmc_states *s, size_t n)
{
    while (s->lanes.size() < n) {
        PooledStream st;
        PooledEvent ev;
        TRY(stream_create(st));
        TRY(event_create(ev));
        s->lanes.push_back(std::move(st));
        s->lane_events.push_back(std::move(ev));
    }
    if (!s->fork_event) TRY(event_create(s->fork_event));
    return ISINGMC_OK;
}

static int lanes_fork(isingmc_states *s, size_t n)
{
    TRY(lanes_reserve(s, n));
    HIP_TRY(hipEventRecord(s->fork_event, s->stream));
    for (size_t i = 0; i < n; i++) HIP_TRY(hipStreamWaitEvent(s->lanes[i], s->fork_event, 0));
    s->n_lanes = n;
    return ISINGMC_OK;
}

int lanes_join(isingmc_states *s)
{
    for (size_t i = 0; i < s->n_lanes && s->n_lanes > 1; i++) {
        HIP_TRY(hipEventRecord(s->lane_events[i], s->lanes[i]));
        HIP_TRY(hipStreamWaitEvent(s->stream, s->lane_events[i], 0));
    }
    s->n_lanes = 1;
    return ISINGMC_OK;
}

void lat_measure_enqueue(isingmc_states *s, unsigned long long *out, size_t out_stride)
{
    const isingmc_graph *g = s->g;
    const bool pmj = !g->uniform_sign;
    for (size_t r0 = 0; r0 < s->R; r0 += MAX_GRID_Y) {
        const size_t n = std::min(MAX_GRID_Y, s->R - r0);
        const uint32_t blocks = (g->geom.nquads + 256 * MEASURE_QUADS_PER_THREAD - 1) / (256 * MEASURE_QUADS_PER_THREAD);
        if (g->mc_mode == MC_ANISO) { // the two directions' bonds carry different |J|: counted apart
            (void)mc_launch_measure_aniso(pmj, dim3(blocks, unsigned(n)), s->stream, s->d_state + r0 * g->state_words, g->geom, g->d_jneg,
                                          g->jneg_uniform, out + r0 * out_stride, out_stride);
            continue;
        }
        if (g->mc_mode == MC_OPEN || g->mc_mode == MC_FIELD_OPEN || g->d_fneg) {
            // the bonds across an open boundary do not exist: they must not count as satisfied; with field-sign planes the
            // spins along their site's field are counted too
            (void)mc_launch_measure_open(pmj, dim3(blocks, unsigned(n)), s->stream, s->d_state + r0 * g->state_words, g->geom, g->d_jneg,
                                         g->jneg_uniform, g->open, g->d_fneg, out + r0 * out_stride, out_stride);
            continue;
        }
        (void)lat_launch_measure(g->vec, pmj, uint32_t(n), s->stream, s->d_state + r0 * g->state_words, g->geom, g->d_jneg, g->jneg_uniform,
                                 out + r0 * out_stride, out_stride);
    }
}

// colour-1 half-sweep fused with the measurement of the finished timestep (single stream: the per-step energy
// mode does not use replica lanes)
static int launch_lat_sweep_measure(isingmc_states *s, const LatThr &thr, uint64_t t_arg, unsigned long long *out, size_t out_stride)
{
    const isingmc_graph *g = s->g;
    for (size_t r0 = 0; r0 < s->R; r0 += MAX_GRID_Y) {
        const size_t n = std::min(MAX_GRID_Y, s->R - r0);
        HIP_TRY(lat_launch_sweep_measure(g->vec, !g->uniform_sign, uint32_t(n), s->stream, s->d_state + r0 * g->state_words, g->geom, t_arg,
                                         s->d_keys + r0, thr, s->has_betas ? s->d_thr + r0 : nullptr, g->d_jneg, g->jneg_uniform,
                                         out + r0 * out_stride, out_stride, s->opt.philox_rounds));
    }
    return ISINGMC_OK;
}

// one launch per colour class, step_policy::gen_replicas_per_thread replicas per thread
static int launch_gen_timestep(isingmc_states *s, double beta)
{
    const isingmc_graph *g = s->g;
    for (uint32_t c = 0; c < g->n_colours; c++) {
        const uint32_t b = uint32_t(g->class_base[c]), e = uint32_t(g->class_base[c + 1]);
        if (e == b) continue;
        const size_t rb = step_policy::gen_replicas_per_thread((e - b + 255) / 256, s->R, s->opt, GEN_RB);
        const size_t chunk = MAX_GRID_Y * rb;
        for (size_t r0 = 0; r0 < s->R; r0 += chunk) {
            const size_t n = std::min(chunk, s->R - r0);
            HIP_TRY(gen_launch_sweep(g->w_is_float, int(rb), uint32_t(n), s->stream, s->d_state + r0 * g->state_words, g->gdev, b, e, s->t,
                                     s->d_keys + r0, beta, s->has_betas ? s->d_beta + r0 : nullptr));
        }
    }
    return ISINGMC_OK;
}

// ------------------------------------------------------------------------------------------------
// measurements enqueued behind the sweeps (per-step energies, sampling, tempering rounds)
// ------------------------------------------------------------------------------------------------
int measure_enqueue(isingmc_states *s, unsigned long long *counts_slot, double *e_slot, long long *m_slot, bool want_up)
{
    const isingmc_graph *g = s->g;
    const size_t R = s->R;
    if (s->packed) { // counts_slot: [pk_slots()][2], one pair per (group, bit) -- a shard may own only some bits of a group
        HIP_TRY(hipMemsetAsync(counts_slot, 0, 2 * s->pk_slots() * sizeof(unsigned long long), s->stream));
        if (s->rj) {
            const bool bip = g->n_colours == 2;
            const int per_cu = std::max(1, cached_rj_measure_blocks_per_cu(g->rj.slots, bip, want_up));
            // two colour classes: the bonds from class 0 alone; class 1 is visited only for its bias terms or the up spins
            const uint32_t class0_end = bip ? uint32_t(g->class_base[1]) : 0u;
            const uint32_t scan_end = bip && !g->has_bias && !want_up ? class0_end : g->pk.n_pos;
            const size_t scan_blocks = scan_end / rj_threads(g->rj.slots);
            for (size_t g0 = 0; g0 < s->groups; g0 += MAX_GRID_Y) {
                const size_t ng = std::min(MAX_GRID_Y, s->groups - g0);
                const size_t gx = step_policy::rj_measure_grid_x(g->n_cu, s->opt, per_cu, scan_blocks, ng);
                // hi level (+ the up spins when wanted) into the first counter of a slot, lo level into the second
                HIP_TRY(rj_launch_measure(dim3(unsigned(gx), unsigned(ng)), s->stream, s->d_state + g0 * g->pk.n_pos, g->rj_hi,
                                          g->pk.site, class0_end, scan_end, want_up, counts_slot + 2 * 32 * g0));
                if (!want_up)
                    HIP_TRY(rj_launch_measure(dim3(unsigned(gx), unsigned(ng)), s->stream, s->d_state + g0 * g->pk.n_pos, g->rj_lo,
                                              g->pk.site, class0_end, scan_end, false, counts_slot + 2 * 32 * g0 + 1));
            }
            return ISINGMC_OK;
        }
        const step_policy::PkMeasureGrid grid = step_policy::pk_measure_grid(g->pk.n_pos, s->groups);
        for (size_t g0 = 0; g0 < s->groups; g0 += MAX_GRID_Y) {
            const size_t ng = std::min(MAX_GRID_Y, s->groups - g0);
            HIP_TRY(pk_launch_measure(grid.blocks, uint32_t(ng), s->stream, s->d_state + g0 * g->pk.n_pos, g->pk, counts_slot + 2 * 32 * g0, grid.pos_per_thread,
                                      g->n_colours == 2 ? uint32_t(g->class_base[1]) : g->pk.n_pos, g->n_colours == 2 ? 2u : 1u));
        }
    } else if (g->kind == ISINGMC_KIND_LATTICE2D) {
        HIP_TRY(hipMemsetAsync(counts_slot, 0, 2 * R * sizeof(unsigned long long), s->stream));
        lat_measure_enqueue(s, counts_slot, 2);
    } else {
        for (size_t r0 = 0; r0 < R; r0 += MAX_GRID_Y) {
            const size_t n = std::min(MAX_GRID_Y, R - r0);
            HIP_TRY(gen_launch_measure(g->w_is_float, uint32_t(n), s->n_partials, s->stream, s->d_state + r0 * g->state_words, g->gdev,
                                       s->d_pe + r0 * s->n_partials, s->d_pm + r0 * s->n_partials));
        }
        HIP_TRY(gen_launch_reduce(s->stream, s->d_pe, s->d_pm, s->n_partials, uint32_t(R), e_slot, m_slot));
    }
    HIP_TRY(hipGetLastError());
    return ISINGMC_OK;
}

// energies / magnetisations of the current configurations into host arrays (either may be NULL)
static int measure(isingmc_states *s, double *energies, int64_t *mags)
{
    const isingmc_graph *g = s->g;
    const size_t R = s->R;
    if (R == 0) return ISINGMC_OK;
    if (s->rj && energies && mags) { // the second counter of a slot holds the lo level of the energy OR the up spins
        TRY(measure(s, energies, nullptr));
        return measure(s, nullptr, mags);
    }
    if (s->packed || g->kind == ISINGMC_KIND_LATTICE2D) {
        TRY(measure_enqueue(s, s->d_meas, nullptr, nullptr, /*want_up=*/mags != nullptr));
        s->meas_zero = false;
        std::vector<unsigned long long> h;
        TRY(read_back(s, h, s->d_meas.get(), 2 * counter_slots(s)));
        for (size_t r = 0; r < R; r++) {
            const size_t sl = counter_slot(s, r);
            if (energies) energies[r] = counters_energy(s, h[2 * sl], h[2 * sl + 1]);
            if (mags) mags[r] = 2 * int64_t(h[2 * sl + 1]) - int64_t(g->nvars);
        }
        return ISINGMC_OK;
    }
    TRY(measure_enqueue(s, nullptr, s->d_oe, s->d_om));
    std::vector<double> he(R);
    std::vector<long long> hm(R);
    HIP_TRY(hipMemcpyAsync(he.data(), s->d_oe, R * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(hm.data(), s->d_om, R * sizeof(long long), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (size_t r = 0; r < R; r++) {
        if (energies) energies[r] = he[r] + g->self_energy;
        if (mags) mags[r] = hm[r];
    }
    return ISINGMC_OK;
}

// ------------------------------------------------------------------------------------------------
// persistent strip kernel (strip_kernels.hpp): when and how is step_policy::strip_plan; here its host side
// ------------------------------------------------------------------------------------------------
static StripPlan to_strip_plan(const step_policy::StripChoice &c)
{
    StripPlan P;
    P.use = c.use;
    P.nw = c.nw;
    P.a.S = c.S;
    P.a.n_strips = c.n_strips;
    P.a.qpr_log2 = c.qpr_log2;
    P.replicas_per_pass = c.replicas_per_pass;
    return P;
}

// the occupancy figure of the strip instantiation this container would launch
static auto strip_occupancy(const isingmc_states *s, bool ladder)
{
    return [s, ladder](int nw, size_t lds) { return cached_strip_blocks_per_cu(!s->g->uniform_sign, nw, ladder, lds, s->opt.philox_rounds); };
}

StripPlan strip_plan(const isingmc_states *s, size_t timesteps, bool ladder)
{
    return to_strip_plan(step_policy::strip_plan(graph_facts(s->g), s->opt, s->R, s->strip.disabled, timesteps, strip_occupancy(s, ladder)));
}

// strip launches of one process on one device never overlap: each needs all its workgroups resident at once
static std::mutex g_strip_mutex;
static hipEvent_t g_strip_done[64] = {};

// one pass: replicas [r0, r0 + n) for timesteps [s->t, s->t + nk).  steps_out / final_out: see lat_strip_kernel
int launch_strip(isingmc_states *s, const StripPlan &P, size_t r0, size_t n, size_t nk, const LatThr *d_thr_steps,
                 uint32_t thr_stride, unsigned long long *steps_out, double *final_energies, const StripLadder *ladder)
{
    const isingmc_graph *g = s->g;
    const size_t granules = s->cap * size_t(P.a.n_strips) * 4 * g->geom.wpr;
    if (s->strip.halo_cap < granules) {
        TRY(dev_regrow(s->stream, s->strip.d_halo, &s->strip.halo_cap, granules, granules));
        HIP_TRY(hipMemsetAsync(s->strip.d_halo, 0, granules * sizeof(unsigned long long), s->stream));
        s->strip.epoch = 0;
    }
    if (!s->strip.d_err) {
        TRY(dev_alloc(s->strip.d_err, 4));
        HIP_TRY(hipMemsetAsync(s->strip.d_err, 0, 4 * sizeof(uint32_t), s->stream));
    }
    StripFinal fin{nullptr, nullptr, 0.0, 0};
    if (final_energies) {
        if (!s->strip.d_fin) {
            TRY(dev_alloc(s->strip.d_fin, s->cap));
            HIP_TRY(hipMemsetAsync(s->strip.d_fin, 0, s->cap * sizeof(unsigned long long), s->stream));
        }
        fin = StripFinal{s->strip.d_fin + r0, final_energies + r0, g->jabs, 2ll * (long long)g->nvars};
    }
    if (uint64_t(s->strip.epoch) + 2 * nk + 2 >= 0xFFFFFFF0ull) { // tags are unique per states object: restart them
        HIP_TRY(hipMemsetAsync(s->strip.d_halo, 0, s->strip.halo_cap * sizeof(unsigned long long), s->stream));
        s->strip.epoch = 0;
    }
    // test hook (tests/test_gpu_strip.py): the first strip launch of this object runs with the error word already raised,
    // as if a workgroup had timed out -- in-order dispatch makes a real timeout need a co-tenant or a replica of more strips
    // than the chip holds -- so that the host's recovery (restore the planes, repeat on the per-colour launches) is exercised
    if (!s->strip.test_failed && s->opt.strip_test_fail_once) {
        const uint32_t one = STRIP_ERR_TIMEOUT;
        HIP_TRY(hipMemcpyAsync(s->strip.d_err, &one, sizeof one, hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        s->strip.test_failed = true;
    }
    StripArgs a = P.a;
    a.epoch = s->strip.epoch;
    a.xcd_remap = n % 8 == 0;
    const size_t lds = step_policy::strip_lds_bytes(a.S, g->geom.wpr);
    {
        std::lock_guard<std::mutex> lock(g_strip_mutex);
        hipEvent_t &ev = g_strip_done[g->device & 63];
        if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        else HIP_TRY(hipStreamWaitEvent(s->stream, ev, 0));
        HIP_TRY(strip_launch(!g->uniform_sign, P.nw, unsigned(n * a.n_strips), lds, s->stream, s->d_state + r0 * g->state_words, g->geom, a, s->t,
                             uint32_t(nk), s->d_keys + r0, d_thr_steps, thr_stride, s->has_betas ? s->d_thr + r0 : nullptr, g->d_jneg,
                             g->jneg_uniform, s->strip.d_halo + r0 * size_t(a.n_strips) * 4 * g->geom.wpr, steps_out, fin,
                             ladder ? *ladder : StripLadder{}, uint32_t(s->R), s->strip.d_err, s->opt.philox_rounds));
        HIP_TRY(hipEventRecord(ev, s->stream));
    }
    return ISINGMC_OK;
}

// after a synchronisation: did a strip launch give up (its workgroups were not all resident)?  Then everything the strip
// kernels share between launches is reset and the object takes the per-colour launches from now on.  Callers that kept
// the planes they started from (run_steps, isingmc_run_sampling) repeat their work; the others report the error.
int strip_check(isingmc_states *s)
{
    if (!s->strip.d_err) return ISINGMC_OK;
    uint32_t h = 0;
    HIP_TRY(hipMemcpy(&h, s->strip.d_err, sizeof h, hipMemcpyDeviceToHost));
    if (h == 0) return ISINGMC_OK;
    (void)hipMemset(s->strip.d_err, 0, sizeof h);
    if (s->strip.d_fin) (void)hipMemset(s->strip.d_fin, 0, s->cap * sizeof(unsigned long long));
    if (s->strip.d_pt_round_counts) (void)hipMemset(s->strip.d_pt_round_counts, 0, 2 * s->R * sizeof(unsigned long long));
    if (s->strip.d_pt_mail) (void)hipMemset(s->strip.d_pt_mail, 0, 4 * s->R * sizeof(unsigned long long));
    if (s->strip.d_halo) (void)hipMemset(s->strip.d_halo, 0, s->strip.halo_cap * sizeof(unsigned long long));
    s->strip.epoch = 0;
    s->meas_fresh = false;
    s->strip.disabled = true;
    return STRIP_TIMED_OUT;
}

int strip_error(int rc)
{
    if (rc != STRIP_TIMED_OUT) return rc;
    return fail(ISINGMC_ERR_HIP, "the persistent strip kernel timed out waiting for a neighbour strip (its workgroups were not all "
                                 "resident: is another process using this GPU?) inside a sequence of enqueue-only calls; the "
                                 "configurations of this object are invalid.  The object uses the per-colour launches from now on "
                                 "(ISINGMC_STRIP=0 selects them from the start)");
}

static int run_steps_impl(isingmc_states *s, size_t timesteps, const double *betas, size_t beta_stride, double *energies_per_step,
                          float *device_ms, bool sync, double *final_energies);

// planes of a states object before a call that may launch the strip kernel (D2D copy on the engine's stream: ~3 us for
// 1024^2 x 64), so that a timeout costs a repeat of the call instead of the configurations
int snapshot_take(isingmc_states *s)
{
    const size_t words = s->R * s->g->state_words;
    if (s->strip.snapshot_cap < words) TRY(dev_regrow(s->stream, s->strip.d_snapshot, &s->strip.snapshot_cap, words, words));
    HIP_TRY(hipMemcpyAsync(s->strip.d_snapshot, s->d_state, words * sizeof(uint32_t), hipMemcpyDeviceToDevice, s->stream));
    return ISINGMC_OK;
}

int snapshot_restore(isingmc_states *s)
{
    HIP_TRY(hipMemcpyAsync(s->d_state, s->strip.d_snapshot, s->R * s->g->state_words * sizeof(uint32_t), hipMemcpyDeviceToDevice, s->stream));
    return ISINGMC_OK;
}

bool may_use_strips(const isingmc_states *s)
{
    return s && s->R && !s->packed && !s->strip.disabled && s->g->kind == ISINGMC_KIND_LATTICE2D && s->g->mc_mode == MC_NONE &&
           s->opt.strip != 0;
}

int run_steps(isingmc_states *s, size_t timesteps, const double *betas, size_t beta_stride,
              double *energies_per_step, float *device_ms, bool sync, double *final_energies)
{
    if (s) TRY(recorders_room_or_fail(s, timesteps));
    const bool may_strip = sync && timesteps >= 2 && may_use_strips(s) && strip_plan(s, timesteps).use;
    return with_strip_retry(s, may_strip, [&] {
        return run_steps_impl(s, timesteps, betas, beta_stride, energies_per_step, device_ms, sync, final_energies);
    });
}

// ------------------------------------------------------------------------------------------------
// run_steps: one plan per call (step_policy::plan_steps: kernel path, chunk of timesteps, replica lanes), one runner per path for each chunk
// ------------------------------------------------------------------------------------------------
// one run_steps call: its arguments, its plan and its scratch (freed on every exit path, after the stream has drained)
struct StepRun {
    isingmc_states *s;
    step_policy::GraphFacts G; // what the plan and the runners' launch shapes are decided from
    StepPlan P;
    const double *betas;
    size_t beta_stride, timesteps;
    double *energies_per_step, *final_energies;
    StripPlan strip = to_strip_plan(P.strip);
    int sweep_resident_wgs = 0; // streaming sweeps: workgroups of lat_sweep_loop_kernel the device holds at once (occupancy x CUs)
    DeviceScratch scratch{s->stream};
    unsigned long long *d_counts = nullptr; // per-step counters [chunk][counter slots][step_slots][2] (lattice and packed paths)
    double *d_energies = nullptr;           // per-step energies [chunk x R] (general paths)
    long long *d_mags = nullptr;
    // per-step tables: one per timestep of a chunk, or one for the call (beta_stride == 0)
    LatThr *d_thr = nullptr;
    double *d_betas = nullptr;
    uint32_t *d_pk_tabs = nullptr;
    RjBeta *d_rj = nullptr;
    std::vector<unsigned long long> h_counts{};
    std::vector<LatThr> h_thr{};
    std::vector<std::array<uint32_t, PK_TAB_WORDS>> h_pk_tabs{};
    std::vector<RjBeta> h_rj{};
    bool pk_tabs_written = false; // run_packed has written the call's acceptance table (a call may begin with a cluster step)
    NonlocalRun nonlocal{};       // cluster steps and isoenergetic moves of the call (nonlocal.hip)
};

// the host's tables of the chunk [k0, k0 + nk)
template <typename T, typename F>
static void fill_step_tables(const StepRun &c, size_t k0, size_t nk, std::vector<T> &h, F &&table_of)
{
    h.resize(c.beta_stride ? nk : 1);
    for (size_t k = 0; k < h.size(); k++) h[k] = table_of(c.betas[(k0 + k) * c.beta_stride]);
}

static double step_beta(const StepRun &c, size_t k) { return c.s->has_betas ? 0.0 : c.betas[k * c.beta_stride]; }

static int upload_lat_thresholds(StepRun &c, size_t k0, size_t nk)
{
    if (c.s->has_betas || c.s->step_preset) return ISINGMC_OK;
    fill_step_tables(c, k0, nk, c.h_thr, [&](double beta) { return lattice_thresholds(beta, c.s->g->jabs); });
    HIP_TRY(hipMemcpyAsync(c.d_thr, c.h_thr.data(), c.h_thr.size() * sizeof(LatThr), hipMemcpyHostToDevice, c.s->stream));
    return ISINGMC_OK;
}

static int run_packed(StepRun &c, size_t k0, size_t nk)
{
    isingmc_states *s = c.s;
    const isingmc_graph *g = s->g;
    // one-degree kernels: the wave-uniform halves of every timestep's Philox calls, PK_PHILOX_STEPS timesteps ahead, written by one
    // small launch when the rows run out (s->d_pk_philox: kept across calls)
    constexpr size_t PK_PHILOX_STEPS = 2048; // (>= chunk)
    const size_t philox_words = !s->rj && g->pk_uni_deg && !s->opt.disable_packed_uniform ? s->groups * pk_uni_philox_table_words() : 0;
    // one table per timestep of the chunk, or one for the call: written by the call's first Metropolis chunk, which is not
    // chunk 0 when the call begins with a cluster step
    const bool new_step_tabs = !s->has_betas && !s->step_preset && (c.beta_stride || !c.pk_tabs_written);
    const bool new_philox_rows = philox_words && !(s->pk_philox_steps && s->pk_philox_groups == s->groups && s->t >= s->pk_philox_t0 &&
                                                   s->t + nk <= s->pk_philox_t0 + s->pk_philox_steps);
    if (k0 > 0 && (new_step_tabs || new_philox_rows)) { // the chunk's tables are overwritten: every lane must have finished reading them
        if (s->n_lanes > 1) TRY(lanes_join(s));
        if (new_step_tabs) HIP_TRY(hipStreamSynchronize(s->stream)); // (written from the host)
    }
    if (new_step_tabs && s->rj) { // real-coupling path: one acceptance scale per timestep
        fill_step_tables(c, k0, nk, c.h_rj, [&](double beta) {
            RjBeta b{};
            rj_beta(beta, g->rj_k, &b.shift, &b.mant);
            return b;
        });
        HIP_TRY(hipMemcpy(c.d_rj, c.h_rj.data(), c.h_rj.size() * sizeof(RjBeta), hipMemcpyHostToDevice));
    } else if (new_step_tabs) {
        fill_step_tables(c, k0, nk, c.h_pk_tabs, [&](double beta) {
            std::array<uint32_t, PK_TAB_WORDS> tab;
            pk_fill_table(tab.data(), g->jabs, [&](uint32_t) { return beta; });
            return tab;
        });
        HIP_TRY(hipMemcpy(c.d_pk_tabs, c.h_pk_tabs.data(), c.h_pk_tabs.size() * sizeof(c.h_pk_tabs[0]), hipMemcpyHostToDevice));
    }
    if (new_step_tabs) c.pk_tabs_written = true;
    if (new_philox_rows) { // (on the main stream, the lanes joined: in order with every sweep that read the old rows)
        if (!s->d_pk_philox) TRY(dev_alloc(s->d_pk_philox, PK_PHILOX_STEPS * philox_words));
        HIP_TRY(pk_uni_launch_philox_table(s->stream, s->d_pk_philox, s->d_keys, uint32_t(s->groups), s->t, uint32_t(PK_PHILOX_STEPS)));
        s->pk_philox_t0 = s->t;
        s->pk_philox_steps = PK_PHILOX_STEPS;
        s->pk_philox_groups = s->groups;
    }
    const size_t n_lanes = c.P.lanes, per_lane = (s->groups + n_lanes - 1) / n_lanes, CS = s->pk_slots();
    if (n_lanes > 1 && s->n_lanes <= 1) TRY(lanes_fork(s, n_lanes)); // (behind the table launch: the lanes wait for it)
    for (size_t k = 0; k < nk; k++) {
        for (size_t lane = 0; lane < n_lanes; lane++) {
            const size_t gb = lane * per_lane, ge = std::min(s->groups, gb + per_lane);
            if (gb >= ge) continue;
            hipStream_t st = n_lanes > 1 ? s->lanes[lane] : s->stream;
            if (s->rj) {
                if (s->has_betas) rj_launch_timestep(s, s->d_rj_betas, 32, gb, ge, st);
                else rj_launch_timestep(s, c.d_rj + (c.beta_stride ? k : 0), 0, gb, ge, st);
            } else {
                const uint32_t *rows = philox_words ? s->d_pk_philox + size_t(s->t - s->pk_philox_t0) * philox_words : nullptr; // timestep s->t's
                if (s->has_betas) TRY(pk_launch_timestep(s, s->d_tab, PK_TAB_WORDS, rows, gb, ge, st));
                else TRY(pk_launch_timestep(s, c.d_pk_tabs + (c.beta_stride ? k * PK_TAB_WORDS : 0), 0, rows, gb, ge, st));
            }
        }
        s->t++;
        // energies after every timestep: the measurements are enqueued behind their sweeps into one counter slot per step
        if (c.d_counts) TRY(measure_enqueue(s, c.d_counts + k * CS * 2, nullptr, nullptr, /*want_up=*/false));
    }
    return ISINGMC_OK;
}

static int run_lat_resident(StepRun &c, size_t k0, size_t nk)
{
    isingmc_states *s = c.s;
    const isingmc_graph *g = s->g;
    const size_t R = s->R;
    TRY(upload_lat_thresholds(c, k0, nk));
    const step_policy::LatResidentLaunch L = step_policy::lat_resident_launch(c.G, s->opt, R, [&](int lpq, unsigned threads, size_t lds) {
        return cached_spread_blocks_per_cu(g->vec, !g->uniform_sign, lpq, threads, lds, s->opt.philox_rounds);
    });
    if (L.spread) {
        HIP_TRY(spread_launch(g->vec, !g->uniform_sign, L.lpq, unsigned(R), L.threads, L.lds_bytes, s->stream, s->d_state, g->geom, s->t, uint32_t(nk), s->d_keys,
                              c.d_thr, uint32_t(c.beta_stride ? 1 : 0), s->has_betas ? s->d_thr : nullptr, g->d_jneg, g->jneg_uniform,
                              c.d_counts, uint32_t(R), s->opt.philox_rounds));
    } else {
        HIP_TRY(lat_launch_resident(g->vec, !g->uniform_sign, unsigned(R), L.threads, L.lds_bytes, s->stream, s->d_state, g->geom, s->t, uint32_t(nk),
                                    s->d_keys, c.d_thr, uint32_t(c.beta_stride ? 1 : 0), s->has_betas ? s->d_thr : nullptr, g->d_jneg,
                                    g->jneg_uniform, c.d_counts, s->opt.philox_rounds));
    }
    s->t += nk;
    if (k0 + nk < c.timesteps && !c.d_counts) HIP_TRY(hipStreamSynchronize(s->stream)); // h_thr is reused by the next chunk
    return ISINGMC_OK;
}

// mid-size lattices: the whole chunk of timesteps in one persistent launch per block of replicas
static int run_lat_strip(StepRun &c, size_t k0, size_t nk)
{
    isingmc_states *s = c.s;
    const size_t R = s->R;
    TRY(upload_lat_thresholds(c, k0, nk));
    // final_energies (device, [R]): the energies of the final configurations come with the last launch (tempering rounds)
    const bool last = k0 + nk == c.timesteps;
    for (size_t r0 = 0; r0 < R; r0 += c.strip.replicas_per_pass)
        TRY(launch_strip(s, c.strip, r0, std::min(c.strip.replicas_per_pass, R - r0), nk, c.d_thr, uint32_t(c.beta_stride ? 1 : 0),
                         c.d_counts ? c.d_counts + 2 * r0 : nullptr, last ? c.final_energies : nullptr));
    s->strip.epoch += uint32_t(2 * nk);
    s->t += nk;
    if (c.final_energies && last) s->meas_fresh = true;
    if (k0 + nk < c.timesteps && !c.d_counts) HIP_TRY(hipStreamSynchronize(s->stream)); // h_thr is reused by the next chunk
    return ISINGMC_OK;
}

static int run_mc_resident(StepRun &c, size_t k0, size_t nk)
{
    isingmc_states *s = c.s;
    const isingmc_graph *g = s->g;
    const size_t R = s->R;
    DeviceScratch thr_scratch(s->stream); // freed (after a stream sync) at the end of this chunk
    LatThrMC *d_thr_mc_steps = nullptr;
    if (!s->has_betas) {
        std::vector<LatThrMC> h;
        fill_step_tables(c, k0, nk, h, [&](double beta) { return lattice_thresholds_mc(g, beta); });
        TRY(thr_scratch.alloc(&d_thr_mc_steps, h.size()));
        HIP_TRY(hipMemcpy(d_thr_mc_steps, h.data(), h.size() * sizeof(LatThrMC), hipMemcpyHostToDevice));
    }
    const step_policy::LatResidentLaunch L = step_policy::mc_resident_launch(c.G, s->opt, R);
    for (size_t r0 = 0; r0 < R; r0 += 65535) {
        const size_t n = std::min<size_t>(65535, R - r0);
        HIP_TRY(mc_launch_resident(g->mc_mode, !g->uniform_sign, unsigned(n), L.threads, L.lds_bytes,
                                   s->stream, s->d_state + r0 * g->state_words, g->geom, s->t, uint32_t(nk), s->d_keys + r0,
                                   d_thr_mc_steps, uint32_t(c.beta_stride ? 1 : 0),
                                   s->has_betas ? s->d_thr_mc + r0 : nullptr, g->d_jneg, g->jneg_uniform, g->open, g->d_fneg,
                                   c.d_counts ? c.d_counts + 2 * r0 : nullptr, uint32_t(R)));
    }
    s->t += nk;
    return ISINGMC_OK;
}

static int run_gen_resident(StepRun &c, size_t k0, size_t nk)
{
    isingmc_states *s = c.s;
    const isingmc_graph *g = s->g;
    const size_t R = s->R;
    const size_t nb = c.beta_stride ? nk : 1;
    if (!s->has_betas) HIP_TRY(hipMemcpyAsync(c.d_betas, c.betas + k0 * c.beta_stride, nb * sizeof(double), hipMemcpyHostToDevice, s->stream));
    const step_policy::GenResidentLaunch L = step_policy::gen_resident_launch(c.G, s->opt, R);
    HIP_TRY(gen_launch_resident(g->w_is_float, L.stage, unsigned(R), L.threads, L.lds_bytes, s->stream,
                                s->d_state, g->gdev, s->t, uint32_t(nk), s->d_keys, c.d_betas, uint32_t(c.beta_stride ? 1 : 0),
                                s->has_betas ? s->d_beta : nullptr, c.d_energies, g->self_energy, g->gen_edges2));
    s->t += nk;
    if (!c.d_energies && k0 + nk < c.timesteps) HIP_TRY(hipStreamSynchronize(s->stream));
    return ISINGMC_OK;
}

// lattices: two launches per timestep (the second fused with the measurement when the energies of every step are wanted)
static int run_lat_stream(StepRun &c, size_t k0, size_t nk)
{
    isingmc_states *s = c.s;
    const size_t R = s->R, SS = c.P.step_slots;
    for (size_t k = k0; k < k0 + nk; k++) {
        const LatThr thr = lattice_thresholds(step_beta(c, k), s->g->jabs);
        TRY(launch_lat_sweep(s, c.G, c.sweep_resident_wgs, 0u, thr, s->t));
        if (c.d_counts) TRY(launch_lat_sweep_measure(s, thr, s->t, c.d_counts + (k - k0) * R * 2 * SS, 2 * SS));
        else TRY(launch_lat_sweep(s, c.G, c.sweep_resident_wgs, 1u, thr, s->t));
        s->t++;
    }
    return ISINGMC_OK;
}

// lattices with a field or open boundaries: one launch per colour (+ one measurement per step)
static int run_mc_stream(StepRun &c, size_t k0, size_t nk)
{
    isingmc_states *s = c.s;
    const isingmc_graph *g = s->g;
    const size_t R = s->R;
    for (size_t k = k0; k < k0 + nk; k++) {
        const LatThrMC thr = lattice_thresholds_mc(g, step_beta(c, k));
        const size_t per_lane = (R + s->n_lanes - 1) / s->n_lanes; // replica blocks on the lanes' streams, as launch_lat_sweep
        for (uint32_t colour = 0; colour < 2; colour++)
            for (size_t lane = 0; lane < s->n_lanes; lane++) {
                const size_t lo = lane * per_lane, hi = std::min(R, lo + per_lane);
                hipStream_t stream = s->n_lanes > 1 ? s->lanes[lane] : s->stream;
                for (size_t r0 = lo; r0 < hi; r0 += MAX_GRID_Y) {
                    const size_t n = std::min(MAX_GRID_Y, hi - r0);
                    HIP_TRY(mc_launch_sweep(g->mc_mode, !g->uniform_sign, dim3((g->geom.nquads + 255) / 256, unsigned(n)), stream,
                                            s->d_state + r0 * g->state_words, g->geom, colour, s->t, s->d_keys + r0, thr,
                                            s->has_betas ? s->d_thr_mc + r0 : nullptr, g->d_jneg, g->jneg_uniform, g->open, g->d_fneg));
                }
            }
        s->t++;
        // get_energy after this timestep: a measurement pass behind the sweep (as on the general path)
        if (c.d_counts) TRY(measure_enqueue(s, c.d_counts + (k - k0) * R * 2, nullptr, nullptr));
    }
    return ISINGMC_OK;
}

// general graphs: one launch per colour class (+ one measurement per step)
static int run_gen_csr(StepRun &c, size_t k0, size_t nk)
{
    isingmc_states *s = c.s;
    for (size_t k = k0; k < k0 + nk; k++) {
        TRY(launch_gen_timestep(s, step_beta(c, k)));
        s->t++;
        if (c.d_energies) TRY(measure_enqueue(s, nullptr, c.d_energies + (k - k0) * s->R, c.d_mags));
    }
    return ISINGMC_OK;
}

// the energy after a non-local timestep (a chunk of its own): into counter slot 0 of step 0 of the chunk
static int measure_nonlocal_step(StepRun &c)
{
    if (!c.d_counts) return ISINGMC_OK;
    if (c.s->packed) return measure_enqueue(c.s, c.d_counts, nullptr, nullptr, /*want_up=*/false);
    lat_measure_enqueue(c.s, c.d_counts, 2 * c.P.step_slots);
    return ISINGMC_OK;
}

// the per-step energies of the chunk [k0, k0 + nk) into energies_per_step[r * timesteps + k0 + k]
static int read_step_energies(StepRun &c, size_t k0, size_t nk)
{
    isingmc_states *s = c.s;
    const size_t R = s->R, T = c.timesteps;
    double *out = c.energies_per_step + k0;
    if (c.d_energies) { // general paths: [replica][step] from the resident kernel, [step][replica] from the reductions
        std::vector<double> he;
        TRY(read_back(s, he, c.d_energies, nk * R));
        const bool resident = c.P.path == StepPath::GenResident;
        for (size_t k = 0; k < nk; k++)
            for (size_t r = 0; r < R; r++) out[r * T + k] = resident ? he[r * nk + k] : he[k * R + r] + s->g->self_energy;
        return ISINGMC_OK;
    }
    const size_t CS = counter_slots(s), SS = c.P.step_slots;
    TRY(read_back(s, c.h_counts, c.d_counts, nk * CS * SS * 2));
    for (size_t k = 0; k < nk; k++)
        for (size_t r = 0; r < R; r++) {
            const unsigned long long *p = c.h_counts.data() + (k * CS + counter_slot(s, r)) * SS * 2;
            unsigned long long c0 = 0, c1 = 0;
            for (size_t sl = 0; sl < SS; sl++) {
                c0 += p[2 * sl];
                c1 += p[2 * sl + 1];
            }
            out[r * T + k] = counters_energy(s, c0, c1);
        }
    return ISINGMC_OK;
}

static int run_steps_impl(isingmc_states *s, size_t timesteps, const double *betas, size_t beta_stride, double *energies_per_step,
                          float *device_ms, bool sync, double *final_energies)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (timesteps && !betas && !s->has_betas) return fail(ISINGMC_ERR_INVALID, "betas is NULL");
    if (!s->has_betas)
        for (size_t k = 0; k < timesteps; k++)
            if (!std::isfinite(betas[k * beta_stride])) return fail(ISINGMC_ERR_INVALID, "beta must be finite");
    if (device_ms) *device_ms = 0.f;
    TRY(use_device(s->g->device));
    const size_t R = s->R;
    if (R == 0) s->t += timesteps; // time passes for an empty container too (replicas appended later start here)
    if (R == 0 || timesteps == 0) return ISINGMC_OK;
    s->meas_fresh = false;
    const step_policy::GraphFacts G = graph_facts(s->g);
    StepRun c{s, G, step_policy::plan_steps(G, s->opt, container_facts(s), timesteps, energies_per_step != nullptr, strip_occupancy(s, false)),
              betas, beta_stride, timesteps, energies_per_step, final_energies};
    const StepPlan &P = c.P;
    if (P.path == StepPath::LatStream && step_policy::sweep_iters_reads_residency(G, s->opt))
        c.sweep_resident_wgs = cached_lat_sweep_loop_blocks_per_cu(!s->g->uniform_sign, unsigned(std::max(0, s->opt.debug_sweep_lds)), s->opt.philox_rounds) * s->g->n_cu;
    const size_t n_tabs = s->has_betas ? 0 : beta_stride ? P.chunk : 1;
    if (s->step_preset) { // the caller's device tables of this call's ONE beta (a population-annealing schedule): nothing to upload
        if (beta_stride || s->has_betas) return fail(ISINGMC_ERR_INVALID, "preset step tables serve one beta per call");
        c.d_thr = const_cast<LatThr *>(s->step_preset->thr);
        c.d_rj = const_cast<RjBeta *>(s->step_preset->rj);
        c.d_pk_tabs = const_cast<uint32_t *>(s->step_preset->pk_tabs);
    } else {
        if (n_tabs && (P.path == StepPath::LatResident || P.path == StepPath::LatStrip)) TRY(c.scratch.alloc(&c.d_thr, n_tabs));
        if (n_tabs && P.path == StepPath::Packed && s->rj) TRY(c.scratch.alloc(&c.d_rj, n_tabs));
        if (n_tabs && P.path == StepPath::Packed && !s->rj) TRY(c.scratch.alloc(&c.d_pk_tabs, n_tabs * PK_TAB_WORDS));
    }
    if (n_tabs && P.path == StepPath::GenResident) TRY(c.scratch.alloc(&c.d_betas, n_tabs));
    const bool general = P.path == StepPath::GenResident || P.path == StepPath::GenCsr;
    if (energies_per_step && general) TRY(c.scratch.alloc(&c.d_energies, P.chunk * R));
    if (energies_per_step && P.path == StepPath::GenCsr) TRY(c.scratch.alloc(&c.d_mags, R));
    if (energies_per_step && !general) TRY(c.scratch.alloc(&c.d_counts, P.chunk * counter_slots(s) * P.step_slots * 2));
    if (device_ms) HIP_TRY(hipEventRecord(s->ev0, s->stream));
    // every exit path below joins the lanes again: later calls (measure, get_states) use s->stream alone
    struct LaneJoin {
        isingmc_states *s;
        ~LaneJoin() { if (s->n_lanes > 1) (void)lanes_join(s); }
    } lane_join{s};
    if (P.lanes > 1 && P.path != StepPath::Packed) TRY(lanes_fork(s, P.lanes)); // (the packed runner forks behind its table launches)
    int rc = ISINGMC_OK;
    for (size_t k0 = 0, nk = 0; k0 < timesteps && rc == ISINGMC_OK; k0 += nk) {
        nk = std::min(P.chunk, timesteps - k0);
        // cluster steps cut the call: a chunk is one cluster step, or a Metropolis stretch that ends before the next one
        // (Swendsen-Wang steps and isoenergetic cluster moves exclude each other: at most one period applies)
        const bool cluster = is_cluster_step(s), icm = is_icm_step(s);
        if (cluster || icm) nk = 1;
        else {
            if (const size_t every = s->cl.every ? s->cl.every : s->icm.every) nk = std::min<size_t>(nk, every - 1 - s->t % every);
            // the periodic recorders cut the call too: a stretch ends with their next sample point
            nk = std::min(nk, recorders_stretch(s));
            // (joined by the cluster step or the update before this stretch; the packed runner forks behind its table launches)
            if (P.lanes > 1 && s->n_lanes <= 1 && P.path != StepPath::Packed) TRY(lanes_fork(s, P.lanes));
        }
        if (c.d_counts && P.path != StepPath::Packed) // (measure_enqueue clears the packed counters itself)
            HIP_TRY(hipMemsetAsync(c.d_counts, 0, nk * R * P.step_slots * 2 * sizeof(unsigned long long), s->stream));
        if (cluster) rc = run_cluster_step(s, c.nonlocal, c.scratch, step_beta(c, k0));
        else if (icm) rc = run_icm_step(s, c.nonlocal, c.scratch);
        else switch (P.path) {
        case StepPath::Packed: rc = run_packed(c, k0, nk); break;
        case StepPath::LatResident: rc = run_lat_resident(c, k0, nk); break;
        case StepPath::LatStrip: rc = run_lat_strip(c, k0, nk); break;
        case StepPath::LatStream: rc = run_lat_stream(c, k0, nk); break;
        case StepPath::McResident: rc = run_mc_resident(c, k0, nk); break;
        case StepPath::McStream: rc = run_mc_stream(c, k0, nk); break;
        case StepPath::GenResident: rc = run_gen_resident(c, k0, nk); break;
        case StepPath::GenCsr: rc = run_gen_csr(c, k0, nk); break;
        }
        if (rc == ISINGMC_OK && (cluster || icm)) rc = measure_nonlocal_step(c);
        if (rc == ISINGMC_OK && energies_per_step) rc = read_step_energies(c, k0, nk);
        TRY(recorders_sample(s, P.path == StepPath::LatStrip, rc)); // (the status is the strip wait's alone; the samples' goes into rc)
    }
    if (s->n_lanes > 1) { const int jrc = lanes_join(s); if (rc == ISINGMC_OK) rc = jrc; }
    if (device_ms && rc == ISINGMC_OK) {
        hipError_t err = hipEventRecord(s->ev1, s->stream);
        if (err == hipSuccess) err = hipEventSynchronize(s->ev1);
        if (err == hipSuccess) err = hipEventElapsedTime(device_ms, s->ev0, s->ev1);
        if (err != hipSuccess) rc = fail(ISINGMC_ERR_HIP, hipGetErrorString(err));
    }
    if (rc != ISINGMC_OK) return rc;
    HIP_TRY(hipGetLastError());
    if (sync) {
        HIP_TRY(hipStreamSynchronize(s->stream));
        if (P.path == StepPath::LatStrip) TRY(strip_check(s));
    }
    return ISINGMC_OK;
}

extern "C" int isingmc_do_time_steps(isingmc_states *s, size_t timesteps, const double *betas, size_t beta_stride,
                                     double *energies_per_step)
{
    return run_steps(s, timesteps, betas, beta_stride, energies_per_step, nullptr);
}

extern "C" int isingmc_do_time_steps_timed(isingmc_states *s, size_t timesteps, const double *betas,
                                           size_t beta_stride, float *device_ms_out)
{
    if (!device_ms_out) return fail(ISINGMC_ERR_INVALID, "device_ms_out is NULL");
    return run_steps(s, timesteps, betas, beta_stride, nullptr, device_ms_out);
}

extern "C" int isingmc_get_energies(isingmc_states *s, double *energies_out)
{
    if (!s || !energies_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    TRY(use_device(s->g->device));
    return measure(s, energies_out, nullptr);
}

extern "C" int isingmc_get_magnetisations(isingmc_states *s, int64_t *mags_out)
{
    if (!s || !mags_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    TRY(use_device(s->g->device));
    return measure(s, nullptr, mags_out);
}

extern "C" int isingmc_get_packed_states(isingmc_states *s, uint32_t *words_out)
{
    if (!s || !words_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    TRY(use_device(s->g->device));
    if (s->R == 0) return ISINGMC_OK;
    if (s->packed) return pk_get_states(s, nullptr, 0, words_out);
    HIP_TRY(hipMemcpyAsync(words_out, s->d_state, s->R * s->g->state_words * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return ISINGMC_OK;
}

extern "C" int isingmc_get_raw_state(isingmc_states *s, uint32_t *words_out, size_t *n_words_out)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    const size_t n = s->packed ? s->groups * size_t(s->g->pk.n_pos) : s->R * s->g->state_words;
    if (n_words_out) *n_words_out = n;
    if (!words_out || n == 0) return ISINGMC_OK;
    TRY(use_device(s->g->device));
    HIP_TRY(hipMemcpyAsync(words_out, s->d_state, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return strip_error(strip_check(s));
}
