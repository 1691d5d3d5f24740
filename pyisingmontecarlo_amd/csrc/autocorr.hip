// libisingmc.so: host side of the lag ring (isingmc_autocorr_*) -- spin autocorrelation over time lags, measured on
// the device against snapshots the ring keeps in the state buffer's own layout: which containers are served, the byte budget, the
// sample enqueued behind a timestep (one launch: count against the live snapshots, replace the oldest), the read-out per replica.
// Nothing here is a kernel: they are in autocorr_kernels.hip, whose header states the rule and why one launch is enough.
#include "internal.hpp"

// the handle: the ring's state is the container's (AutocorrState, one ring per container)
struct isingmc_autocorr {
    isingmc_states *a;
};

static size_t acr_state_words(const isingmc_states *s) { return s->packed ? s->groups * size_t(s->g->pk.n_pos) : s->R * size_t(s->g->state_words); }

// why this container cannot have a lag ring ("" when it can): exactly the containers isingmc_overlaps serves; no side effects
static std::string acr_obstacle(const isingmc_states *s)
{
    const isingmc_graph *g = s->g;
    if (!s->packed) {
        if (g->kind != ISINGMC_KIND_LATTICE2D)
            return "a lag ring needs a container on the checkerboard lattice path or on a replica-packed family; this graph runs on the f64 CSR "
                   "general-graph kernel family (the replica-packed family is chosen by size, or by ISINGMC_FORCE_PACKED=1 / the stable-path flag "
                   "at creation)";
        const std::string why = lattice_obstacle(g, "lag rings", true, false);
        if (!why.empty()) return why;
    }
    if (s->tempering.attached)
        return "a tempering ladder is attached: a slot changes its temperature at every exchange, so its lags would mix the temperatures "
               "(isingmc_pt_detach first)";
    return "";
}

extern "C" int isingmc_autocorr_create(isingmc_states *s, size_t n_lags, unsigned flags, isingmc_autocorr **out)
{
    if (!s || !out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (flags) return fail(ISINGMC_ERR_INVALID, "unknown flag: a lag ring takes no flags (0)");
    if (n_lags < 1 || n_lags > ACR_MAX_LAGS)
        return fail(ISINGMC_ERR_INVALID, "n_lags = " + std::to_string(n_lags) + ": a lag ring holds 1 .. " + std::to_string(ACR_MAX_LAGS) + " lags");
    {
        const std::string why = acr_obstacle(s);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    if (s->acr.live) return fail(ISINGMC_ERR_INVALID, "a lag ring is live on this container already: one ring per container (isingmc_autocorr_destroy first)");
    if (s->R == 0) return fail(ISINGMC_ERR_INVALID, "the container holds no replica: nothing to measure");
    const size_t words = acr_state_words(s), rows = counter_slots(s);
    if (!s->packed && (rows * ((size_t(s->g->state_words) + 1023) / 1024) > 0x7FFFFFFFull))
        return fail(ISINGMC_ERR_INVALID, "a lag ring serves at most 2^31 - 1 workgroups of 1024 state words per sample");
    const unsigned long long ring_bytes = (unsigned long long)words * sizeof(uint32_t), sums_bytes = (unsigned long long)rows * (n_lags + 1) * 8;
    const unsigned long long budget = (unsigned long long)std::max(0ll, s->opt.autocorr_bytes);
    if (ring_bytes > budget / n_lags || ring_bytes * n_lags + sums_bytes > budget)
        return fail(ISINGMC_ERR_INVALID, "a ring of " + std::to_string(n_lags) + " snapshots of " + std::to_string(ring_bytes) + " bytes and " +
                                             std::to_string(sums_bytes) + " bytes of sums is larger than the option autocorr_bytes = " +
                                             std::to_string(budget) + " allows (isingmc_states_set_option raises the budget)");
    TRY(use_device(s->g->device));
    AutocorrState A;
    TRY(dev_alloc(A.d_ring, words * n_lags));
    TRY(dev_alloc(A.d_sums, rows * (n_lags + 1)));
    // recycled blocks hold whatever they held: the sums start at zero; a snapshot is never read before a sample has written it
    HIP_TRY(hipMemsetAsync(A.d_sums, 0, rows * (n_lags + 1) * sizeof(unsigned long long), s->stream));
    A.live = true;
    A.n_lags = uint32_t(n_lags);
    A.R = s->R;
    A.slot_words = words;
    s->acr = std::move(A);
    s->rec[REC_AUTOCORR] = Periodic{};
    *out = new isingmc_autocorr{s};
    return ISINGMC_OK;
}

extern "C" int isingmc_autocorr_destroy(isingmc_autocorr *ac)
{
    if (!ac) return ISINGMC_OK;
    isingmc_states *s = ac->a;
    (void)hipSetDevice(s->g->device);
    (void)stream_quiesce(s->stream); // the blocks go back to the cache: no sample may still be running
    s->rec[REC_AUTOCORR] = Periodic{};
    s->acr = AutocorrState{};
    delete ac;
    return ISINGMC_OK;
}

int autocorr_sample_enqueue(isingmc_states *s)
{
    AutocorrState &A = s->acr;
    if (!A.live) return fail(ISINGMC_ERR_INVALID, "this container holds no lag ring");
    if (A.R != s->R) return fail(ISINGMC_ERR_INVALID, "the container holds another number of replicas than when the ring was made: its snapshots are those replicas'");
    if (s->n_lanes > 1) TRY(lanes_join(s)); // the sweeps before this sample may have run on replica lanes
    const AutocorrPlan P = autocorr_plan(A.samples, A.n_lags);
    const isingmc_graph *g = s->g;
    if (!s->packed)
        HIP_TRY(autocorr_launch_lattice(s->stream, s->d_state, A.d_ring, s->R, g->state_words, A.n_lags, P.live, P.write_slot, A.d_sums));
    else
        HIP_TRY(autocorr_launch_packed(s->stream, s->d_state, A.d_ring, g->pk.site, g->pk.n_pos, s->groups, uint32_t(s->pk_bit0), uint32_t(s->R), A.n_lags,
                                       P.live, P.write_slot, A.d_sums));
    A.samples++;
    return ISINGMC_OK;
}

extern "C" int isingmc_autocorr_sample(isingmc_autocorr *ac)
{
    if (!ac) return fail(ISINGMC_ERR_INVALID, "NULL ring");
    TRY(use_device(ac->a->g->device));
    return autocorr_sample_enqueue(ac->a);
}

extern "C" int isingmc_autocorr_set_every(isingmc_autocorr *ac, size_t every)
{
    if (!ac) return fail(ISINGMC_ERR_INVALID, "NULL ring");
    isingmc_states *s = ac->a;
    if (every) s->rec[REC_AUTOCORR].restart(s->t);
    s->rec[REC_AUTOCORR].every = every;
    return ISINGMC_OK;
}

extern "C" int isingmc_autocorr_count(const isingmc_autocorr *ac, uint64_t *samples_out, size_t *n_lags_out)
{
    if (!ac) return fail(ISINGMC_ERR_INVALID, "NULL ring");
    if (samples_out) *samples_out = ac->a->acr.samples;
    if (n_lags_out) *n_lags_out = ac->a->acr.n_lags;
    return ISINGMC_OK;
}

extern "C" int isingmc_autocorr_reset(isingmc_autocorr *ac)
{
    if (!ac) return fail(ISINGMC_ERR_INVALID, "NULL ring");
    isingmc_states *s = ac->a;
    TRY(use_device(s->g->device));
    // samples enqueued so far still count into the sums ahead of this on the stream; the snapshots need no clearing: live starts at 0
    HIP_TRY(hipMemsetAsync(s->acr.d_sums, 0, counter_slots(s) * (size_t(s->acr.n_lags) + 1) * sizeof(unsigned long long), s->stream));
    s->acr.samples = 0;
    s->rec[REC_AUTOCORR].last_t = 0;
    return ISINGMC_OK;
}

extern "C" int isingmc_autocorr_get(isingmc_autocorr *ac, uint64_t *counts_out, uint64_t *diff_out)
{
    if (!ac) return fail(ISINGMC_ERR_INVALID, "NULL ring");
    isingmc_states *s = ac->a;
    const AutocorrState &A = s->acr;
    if (A.R != s->R) return fail(ISINGMC_ERR_INVALID, "the container holds another number of replicas than when the ring was made: its sums are those replicas'");
    TRY(use_device(s->g->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    TRY(strip_error(strip_check(s)));
    const size_t row = size_t(A.n_lags) + 1;
    if (counts_out) {
        const AutocorrPlan P = autocorr_plan(A.samples, A.n_lags);
        for (uint32_t l = 0; l <= A.n_lags; l++) counts_out[l] = P.count(l);
    }
    if (!diff_out) return ISINGMC_OK;
    std::vector<unsigned long long> h;
    TRY(read_back(s, h, A.d_sums.get(), counter_slots(s) * row));
    for (size_t r = 0; r < s->R; r++) std::copy(h.begin() + counter_slot(s, r) * row, h.begin() + (counter_slot(s, r) + 1) * row, diff_out + r * row);
    return ISINGMC_OK;
}

// The ring (and with site_sums the sums) zeroed, thermalisation with the periods off, then n_samples x { sampling_freq timesteps; one
// sample }, everything enqueued back to back.  The zeroing belongs to the attempt: the periods are off again when an attempt returns,
// so with_strip_retry's replay guard (which reads them) skips nothing in a repeat -- the repeat takes every sample again, into sums
// and a sample number that start from zero again.
static int run_sampling_autocorr_impl(isingmc_autocorr *ac, double beta, size_t thermalization, size_t sampling_freq, size_t n_samples, bool site_sums)
{
    isingmc_states *s = ac->a;
    TRY(isingmc_autocorr_reset(ac));
    if (site_sums) {
        TRY(isingmc_moments_reset(s));
        s->rec[REC_MOMENTS].last_t = 0;
    }
    struct BetaGuard { // a uniform beta as per-replica thresholds for the call: the step launches need no host tables
        isingmc_states *s;
        bool active;
        ~BetaGuard() { if (active) (void)isingmc_states_set_betas(s, nullptr); }
    } guard{s, false};
    if (!s->has_betas && s->R) {
        const std::vector<double> b(s->R, beta);
        TRY(set_betas(s, b.data(), /*all_equal=*/true));
        guard.active = true;
    }
    struct Off {
        isingmc_states *s;
        bool site_sums;
        ~Off() { s->rec[REC_AUTOCORR].every = 0; if (site_sums) s->rec[REC_MOMENTS].every = 0; }
    } off{s, site_sums};
    s->rec[REC_AUTOCORR].every = 0;
    if (site_sums) s->rec[REC_MOMENTS].every = 0;
    TRY(run_steps(s, thermalization, nullptr, 0, nullptr, nullptr, /*sync=*/false));
    for (Recorder which : {REC_AUTOCORR, REC_MOMENTS}) {
        if (which == REC_MOMENTS && !site_sums) continue;
        s->rec[which].every = sampling_freq;
        s->rec[which].t0 = s->t;
    }
    TRY(run_steps(s, n_samples * sampling_freq, nullptr, 0, nullptr, nullptr, /*sync=*/false));
    if (!s->strip.guard) return ISINGMC_OK;
    HIP_TRY(hipStreamSynchronize(s->stream)); // (a call that may be repeated: what the last strip launch left is checked here)
    return strip_check(s);
}

extern "C" int isingmc_run_sampling_autocorr(isingmc_autocorr *ac, double beta, size_t thermalization, size_t sampling_freq, size_t n_samples,
                                             int site_sums, double *energies_out)
{
    if (!ac) return fail(ISINGMC_ERR_INVALID, "NULL ring");
    isingmc_states *s = ac->a;
    if (sampling_freq == 0) return fail(ISINGMC_ERR_INVALID, "sampling_freq must be positive");
    if (!s->has_betas && !std::isfinite(beta)) return fail(ISINGMC_ERR_INVALID, "beta must be finite");
    if (s->rec[REC_AUTOCORR].every) return fail(ISINGMC_ERR_INVALID, "the lag ring of this container samples on a period already: the sampling run sets its own (isingmc_autocorr_set_every(ring, 0) first)");
    if (site_sums && s->rec[REC_MOMENTS].every) return fail(ISINGMC_ERR_INVALID, "moment sums are switched on for this container already: the sampling run sets its own period (switch accumulation off first)");
    TRY(recorders_room_or_fail(s, thermalization + sampling_freq * n_samples));
    if (site_sums) { // the per-replica site sums of S18 for the same samples: reserved (or refused: moments_bytes), their period left to the run
        TRY(isingmc_states_set_moments_every(s, sampling_freq, ISINGMC_MOMENTS_PER_REPLICA));
        s->rec[REC_MOMENTS].every = 0;
    }
    const bool may_strip = may_use_strips(s) && (strip_plan(s, thermalization).use || strip_plan(s, n_samples * sampling_freq).use);
    TRY(with_strip_retry(s, may_strip, [&] { return run_sampling_autocorr_impl(ac, beta, thermalization, sampling_freq, n_samples, site_sums != 0); }));
    if (energies_out) return isingmc_get_energies(s, energies_out); // waits
    HIP_TRY(hipStreamSynchronize(s->stream));
    return strip_error(strip_check(s));
}

extern "C" int isingmc_host_autocorr_plan(uint64_t samples_taken, size_t n_lags, uint32_t *slot_of_lag_out, uint32_t *live_lags_out,
                                          uint32_t *write_slot_out, uint64_t *counts_out)
{
    if (n_lags < 1 || n_lags > ACR_MAX_LAGS)
        return fail(ISINGMC_ERR_INVALID, "n_lags = " + std::to_string(n_lags) + ": a lag ring holds 1 .. " + std::to_string(ACR_MAX_LAGS) + " lags");
    const AutocorrPlan P = autocorr_plan(samples_taken, uint32_t(n_lags));
    for (uint32_t l = 0; l <= n_lags; l++) {
        if (slot_of_lag_out) slot_of_lag_out[l] = P.slot_of_lag(l);
        if (counts_out) counts_out[l] = P.count(l);
    }
    if (live_lags_out) *live_lags_out = P.live;
    if (write_slot_out) *write_slot_out = P.write_slot;
    return ISINGMC_OK;
}
