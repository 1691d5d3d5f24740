// libisingmc.so: each replica's lowest-energy configuration, kept on the device (isingmc_best_* and
// isingmc_states_set_track_best) -- which containers are served, the records and the second state buffer, the update enqueued
// behind a measurement, the read-outs.  Nothing here is a kernel: they are in best_kernels.hip, whose header states the rule.
#include "internal.hpp"

// why this container cannot keep records ("" when it can): exactly the containers energies_enqueue serves; no side effects
static std::string best_obstacle(const isingmc_states *s)
{
    const isingmc_graph *g = s->g;
    if (s->packed) return "";
    if (g->kind != ISINGMC_KIND_LATTICE2D)
        return "minimum tracking needs the device-side energy array of the checkerboard lattice path or of a replica-packed family; this graph "
               "runs on the f64 CSR general-graph kernel family (the replica-packed family is chosen by size, or by ISINGMC_FORCE_PACKED=1 / "
               "the stable-path flag at creation)";
    if (g->mc_mode != MC_NONE)
        return "minimum tracking needs the device-side energy array, which lattices with fields, open boundaries or anisotropic couplings do "
               "not have";
    if (g->state_words % 4 != 0) return "minimum tracking copies a replica in 16-byte pieces: W H / 32 must be a multiple of 4";
    return "";
}

static size_t best_state_size(const isingmc_states *s) { return s->packed ? s->groups * size_t(s->g->pk.n_pos) : s->cap * s->g->state_words; }

static int best_reset_enqueue(isingmc_states *s)
{
    const std::vector<double> inf(s->best.cap, std::numeric_limits<double>::infinity());
    HIP_TRY(hipMemcpyAsync(s->best.d_e, inf.data(), inf.size() * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemsetAsync(s->best.d_t, 0, s->best.cap * sizeof(unsigned long long), s->stream));
    HIP_TRY(hipMemsetAsync(s->best.d_count, 0, sizeof(unsigned long long), s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream)); // (the host vector above)
    return ISINGMC_OK;
}

// the records and the second state buffer, sized for the container as it is now; a container that has grown since (tracking was
// off meanwhile: isingmc_states_append is refused while it is on) starts its records again
static int best_reserve(isingmc_states *s)
{
    const size_t words = best_state_size(s);
    if (s->best.d_state && s->best.state_words == words && s->best.cap == s->R) return ISINGMC_OK;
    HIP_TRY(stream_quiesce(s->stream)); // recycled blocks: nothing enqueued may still use the old ones
    s->best = BestState{}; // (every member: the blocks go back, the sizes are 0)
    // Padding positions and the bits of a packed group this container does not own take whatever the copies bring along: they
    // have no defined value.  The buffer is cleared once, so that isingmc_best_raw_state is deterministic.
    TRY(dev_alloc(s->best.d_state, words));
    TRY(dev_alloc(s->best.d_e, s->R));
    TRY(dev_alloc(s->best.d_t, s->R));
    TRY(dev_alloc(s->best.d_energy, s->R));
    TRY(dev_alloc(s->best.d_flags, s->packed ? s->groups : s->R));
    TRY(dev_alloc(s->best.d_count, 1));
    HIP_TRY(hipMemsetAsync(s->best.d_state, 0, words * sizeof(uint32_t), s->stream));
    s->best.state_words = words;
    s->best.cap = s->R;
    return best_reset_enqueue(s);
}

extern "C" int isingmc_states_set_track_best(isingmc_states *s, size_t every)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (every) {
        const std::string why = best_obstacle(s);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
        TRY(use_device(s->g->device));
        TRY(best_reserve(s));
    }
    s->rec[REC_BEST].every = every;
    return ISINGMC_OK;
}

extern "C" int isingmc_states_track_best(const isingmc_states *s, size_t *every_out)
{
    if (!s || !every_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    *every_out = s->rec[REC_BEST].every;
    return ISINGMC_OK;
}

int best_from_energies(isingmc_states *s, const double *d_energy)
{
    if (s->R == 0) return ISINGMC_OK;
    if (s->n_lanes > 1) TRY(lanes_join(s)); // the sweeps before this update may have run on replica lanes
    const isingmc_graph *g = s->g;
    HIP_TRY(best_launch_decide(s->stream, s->packed, d_energy, uint32_t(s->R), uint32_t(s->pk_bit0), uint32_t(s->groups), s->t, s->best.d_e, s->best.d_t,
                               s->best.d_flags, s->best.d_count));
    if (s->packed)
        HIP_TRY(best_launch_keep_bits(s->stream, s->d_state, s->best.d_state, s->best.d_flags, uint32_t(s->R), uint32_t(s->pk_bit0), s->groups, g->pk.n_pos));
    else
        HIP_TRY(best_launch_keep_rows(s->stream, s->d_state, s->best.d_state, s->best.d_flags, s->R, g->state_words));
    return ISINGMC_OK;
}

int best_update_enqueue(isingmc_states *s)
{
    if (s->R == 0) return ISINGMC_OK;
    if (s->n_lanes > 1) TRY(lanes_join(s));
    TRY(energies_enqueue(s, s->best.d_energy));
    return best_from_energies(s, s->best.d_energy);
}

extern "C" int isingmc_best_update(isingmc_states *s)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    {
        const std::string why = best_obstacle(s);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    TRY(use_device(s->g->device));
    TRY(best_reserve(s));
    return best_update_enqueue(s);
}

static int best_ready(isingmc_states *s)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (!s->best.d_state || s->best.cap != s->R)
        return fail(ISINGMC_ERR_INVALID, "this container keeps no records: switch tracking on (isingmc_states_set_track_best) or call isingmc_best_update first");
    TRY(use_device(s->g->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return strip_error(strip_check(s));
}

extern "C" int isingmc_best_get(isingmc_states *s, double *energies_out, uint8_t *states_out, size_t replica_stride_bytes, uint64_t *timesteps_out,
                                uint64_t *improvements_out)
{
    TRY(best_ready(s));
    if (states_out && replica_stride_bytes < s->g->nvars) return fail(ISINGMC_ERR_INVALID, "replica stride smaller than nvars");
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the timestep records are read out as they lie");
    if (energies_out && s->R) HIP_TRY(hipMemcpy(energies_out, s->best.d_e, s->R * sizeof(double), hipMemcpyDeviceToHost));
    if (timesteps_out && s->R) HIP_TRY(hipMemcpy(timesteps_out, s->best.d_t, s->R * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (improvements_out) HIP_TRY(hipMemcpy(improvements_out, s->best.d_count, sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (states_out) TRY(expand_states(s, s->best.d_state, states_out, replica_stride_bytes));
    return ISINGMC_OK;
}

extern "C" int isingmc_best_raw_state(isingmc_states *s, uint32_t *words_out, size_t *n_words_out)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    const size_t n = s->packed ? s->groups * size_t(s->g->pk.n_pos) : s->R * s->g->state_words; // as isingmc_get_raw_state
    if (n_words_out) *n_words_out = n;
    if (!words_out || n == 0) return ISINGMC_OK;
    TRY(best_ready(s));
    HIP_TRY(hipMemcpy(words_out, s->best.d_state, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return ISINGMC_OK;
}

extern "C" int isingmc_best_reset(isingmc_states *s)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (!s->best.d_state) return ISINGMC_OK; // nothing recorded yet: the records start at +inf anyway
    TRY(use_device(s->g->device));
    return best_reset_enqueue(s);
}
