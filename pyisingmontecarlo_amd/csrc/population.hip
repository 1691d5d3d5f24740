// libisingmc.so: population annealing -- the resampling step on the container's stream (isingmc_pa_*).
// The kernels live in pa_kernels.hip; the energies come from the measurement the tempering rounds use (energies_enqueue).
#include "internal.hpp"

// why this container cannot be resampled ("" when it can): no side effects
static std::string pa_obstacle(const isingmc_states *s)
{
    const isingmc_graph *g = s->g;
    if (!s->packed && g->kind != ISINGMC_KIND_LATTICE2D)
        return "population annealing is not implemented for containers on the f64 CSR general-graph family (the replica-packed families "
               "are chosen by size, by ISINGMC_FORCE_PACKED=1 or by ISINGMC_FLAG_STABLE_PATH at creation)";
    if (!s->packed && g->mc_mode != MC_NONE)
        return "population annealing needs the device-side energy array, which lattices with fields, open boundaries or anisotropic "
               "couplings do not have";
    if (s->tempering.attached) return "a tempering ladder is attached to this container: a population shares one beta";
    if (s->has_betas) return "per-replica betas are set for this container: a population shares one beta";
    if (s->first != 0 || s->first + s->R < s->n_total) return "this container is a shard of a larger set of experiments: one population lives in one container";
    if (s->R == 0) return "the container holds no replica";
    if (s->R > PA_MAX_REPLICAS) return "populations above 2^31 replicas are not supported";
    return "";
}

static size_t pa_state_size(const isingmc_states *s) { return s->packed ? s->groups * size_t(s->g->pk.n_pos) : s->cap * s->g->state_words; }

// the second state buffer and the tables, sized for the container as it is now (it may have grown since the last call)
static int pa_reserve(isingmc_states *s)
{
    const size_t words = pa_state_size(s);
    if (s->pa.d_state && s->pa.state_words == words && s->pa.cap >= s->R) return ISINGMC_OK;
    HIP_TRY(stream_quiesce(s->stream)); // recycled blocks: nothing enqueued may still use the old ones
    std::vector<uint32_t> family(s->R);
    for (size_t r = 0; r < s->R; r++) family[r] = uint32_t(r);
    if (s->pa.families_set && s->pa.cap) // a container that grew keeps its families; the new slots found their own
        HIP_TRY(hipMemcpy(family.data(), s->pa.d_family, std::min(s->pa.cap, s->R) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    s->pa.d_state.reset(); s->pa.d_energy.reset(); s->pa.d_cum.reset(); s->pa.d_src.reset();
    s->pa.d_user_src.reset(); s->pa.d_family.reset(); s->pa.d_family2.reset();
    s->pa.cap = s->pa.state_words = 0;
    s->pa.families_set = false;
    TRY(dev_alloc(s->pa.d_state, words));
    TRY(dev_alloc(s->pa.d_energy, s->R));
    TRY(dev_alloc(s->pa.d_cum, s->R + pa_scan_blocks(s->R)));
    TRY(dev_alloc(s->pa.d_src, s->R));
    TRY(dev_alloc(s->pa.d_user_src, s->R));
    TRY(dev_alloc(s->pa.d_family, s->R));
    TRY(dev_alloc(s->pa.d_family2, s->R));
    if (!s->pa.d_record) TRY(dev_alloc(s->pa.d_record, 1));
    HIP_TRY(hipMemcpy(s->pa.d_family, family.data(), s->R * sizeof(uint32_t), hipMemcpyHostToDevice));
    s->pa.state_words = words;
    s->pa.cap = s->R;
    s->pa.families_set = true;
    return ISINGMC_OK;
}

// enqueue: new slot j <- old slot d_src[j], configurations and families; then nothing the container had cached about its
// configurations holds any longer
static int pa_gather(isingmc_states *s, const uint32_t *d_src)
{
    const isingmc_graph *g = s->g;
    if (s->packed) // pk_bit0 == 0: a shard is refused
        HIP_TRY(pa_launch_bit_gather(s->stream, s->d_state, s->pa.d_state, d_src, uint32_t(s->R), s->groups, g->pk.n_pos, g->pk.site));
    else
        HIP_TRY(pa_launch_row_gather(s->stream, s->d_state, s->pa.d_state, d_src, s->R, g->state_words));
    HIP_TRY(pa_launch_gather_u32(s->stream, s->pa.d_family, d_src, uint32_t(s->R), s->pa.d_family2));
    std::swap(s->d_state, s->pa.d_state); // every launch reads the pointer when it is enqueued: the stream orders the rest
    std::swap(s->pa.d_family, s->pa.d_family2);
    s->meas_fresh = false; // energies a strip launch left for the next tempering measurement
    // (the strip path's snapshot is taken anew by every synchronous call: nothing to drop)
    if (s->strip.d_halo) { // halo rows the strips exchanged: the state a fresh allocation starts from
        HIP_TRY(hipMemsetAsync(s->strip.d_halo, 0, s->strip.halo_cap * sizeof(unsigned long long), s->stream));
        s->strip.epoch = 0;
    }
    return ISINGMC_OK;
}

// enqueue one resampling; its record goes to *d_rec (device)
static int pa_resample_enqueue(isingmc_states *s, double dbeta, uint64_t seed, uint64_t step, PaRecord *d_rec)
{
    const uint32_t R = uint32_t(s->R);
    TRY(energies_enqueue(s, s->pa.d_energy));
    // minimum tracking: the records see the population before the gather; they stay with the slots
    if (s->rec[REC_BEST].every) TRY(best_from_energies(s, s->pa.d_energy));
    HIP_TRY(pa_launch_weights(s->stream, s->pa.d_energy, R, dbeta, seed, step, s->pa.d_cum, d_rec));
    HIP_TRY(pa_launch_scan(s->stream, s->pa.d_cum, R, s->pa.d_cum + R));
    HIP_TRY(pa_launch_sources(s->stream, s->pa.d_cum, R, d_rec, s->pa.d_src));
    return pa_gather(s, s->pa.d_src);
}

extern "C" int isingmc_pa_resample(isingmc_states *s, double dbeta, uint64_t seed, uint64_t step)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (!std::isfinite(dbeta)) return fail(ISINGMC_ERR_INVALID, "dbeta must be finite");
    {
        const std::string why = pa_obstacle(s);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    if (const char *why = recorders_refusal(s, RecorderRefusal::Resample)) return fail(ISINGMC_ERR_INVALID, why);
    TRY(use_device(s->g->device));
    TRY(pa_reserve(s));
    TRY(pa_resample_enqueue(s, dbeta, seed, step, s->pa.d_record));
    s->pa.have_record = true;
    return ISINGMC_OK;
}

// The whole schedule in one call: for k = 0 .. n - 1 { k > 0: resample for betas[k] - betas[k - 1] with step counter k;
// sweeps_per_beta timesteps at betas[k] }, everything enqueued, ONE wait at the end.  The acceptance tables of every beta go to
// the device before the first launch and every resampling writes its record into its own slot of a device log.  (With a
// cluster period on, the cluster steps' workspace is per run of timesteps and the host waits once per beta to hand it back.)
extern "C" int isingmc_pa_run(isingmc_states *s, const double *betas, size_t n_betas, size_t sweeps_per_beta, uint64_t seed, uint64_t *sum_out,
                              double *eref_out, uint64_t *distinct_out, double *mean_energy_out)
{
    if (!s || !betas || n_betas == 0) return fail(ISINGMC_ERR_INVALID, "NULL argument / no betas");
    for (size_t k = 0; k < n_betas; k++)
        if (!std::isfinite(betas[k])) return fail(ISINGMC_ERR_INVALID, "beta must be finite");
    {
        const std::string why = pa_obstacle(s);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    if (const char *why = recorders_refusal(s, RecorderRefusal::Resample)) return fail(ISINGMC_ERR_INVALID, why);
    TRY(use_device(s->g->device));
    TRY(pa_reserve(s));
    const size_t n_steps = n_betas - 1;
    DeviceScratch scratch(s->stream); // the tables and the log: handed back after the final wait
    std::vector<StepPreset> presets;
    TRY(step_presets_build(s, betas, n_betas, scratch, presets));
    PaRecord *d_log = nullptr;
    TRY(scratch.alloc(&d_log, n_steps));
    int rc = ISINGMC_OK;
    for (size_t k = 0; k < n_betas && rc == ISINGMC_OK; k++) {
        if (k > 0) rc = pa_resample_enqueue(s, betas[k] - betas[k - 1], seed, k, d_log + (k - 1));
        if (rc != ISINGMC_OK) break;
        s->step_preset = &presets[k];
        rc = run_steps(s, sweeps_per_beta, &betas[k], 0, nullptr, nullptr, /*sync=*/false);
        s->step_preset = nullptr;
    }
    if (rc == ISINGMC_OK && s->rec[REC_BEST].every) rc = best_update_enqueue(s); // the final population
    if (rc == ISINGMC_OK && n_steps) {
        HIP_TRY(hipMemcpyAsync(s->pa.d_record, d_log + (n_steps - 1), sizeof(PaRecord), hipMemcpyDeviceToDevice, s->stream));
        s->pa.have_record = true;
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    TRY(strip_error(strip_check(s)));
    if (rc != ISINGMC_OK) return strip_error(rc);
    std::vector<PaRecord> log(n_steps);
    if (n_steps) HIP_TRY(hipMemcpy(log.data(), d_log, n_steps * sizeof(PaRecord), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < n_steps; k++) {
        if (sum_out) sum_out[k] = log[k].sum;
        if (eref_out) eref_out[k] = log[k].eref;
        if (distinct_out) distinct_out[k] = log[k].distinct;
        if (mean_energy_out) mean_energy_out[k] = log[k].mean;
    }
    return ISINGMC_OK;
}

// ---- the step chooser ----------------------------------------------------------------------------------------
// measure into the chooser's own array, search, wait for the decision: nothing a resampling or a sweep keeps is written
static int pa_choose(isingmc_states *s, double dbeta_max, double target, PaChoose *out)
{
    if (!s->pac.d_choose) TRY(dev_alloc(s->pac.d_choose, 1));
    if (s->pac.cap < s->R) TRY(dev_regrow(s->stream, s->pac.d_energy, &s->pac.cap, s->R, s->R));
    TRY(energies_enqueue(s, s->pac.d_energy));
    HIP_TRY(pa_launch_choose(s->stream, s->pac.d_energy, uint32_t(s->R), std::ldexp(dbeta_max, -16), pa_target32(target), s->pac.d_choose));
    HIP_TRY(hipMemcpyAsync(out, s->pac.d_choose, sizeof(PaChoose), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return strip_error(strip_check(s));
}

// what every entry point of the chooser refuses before it touches the container
static int pa_choose_admit(const isingmc_states *s, double dbeta_max, double target)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (const char *why = pa_choose_refusal(dbeta_max, target)) return fail(ISINGMC_ERR_INVALID, why);
    const std::string why = pa_obstacle(s);
    if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    if (const char *rec = recorders_refusal(s, RecorderRefusal::Resample)) return fail(ISINGMC_ERR_INVALID, rec);
    return ISINGMC_OK;
}

extern "C" int isingmc_pa_choose_step(isingmc_states *s, double dbeta_max, double target, uint32_t *k_out, double *dbeta_out, uint64_t *sum_out,
                                      uint64_t *num_lo_out, uint64_t *num_hi_out)
{
    TRY(pa_choose_admit(s, dbeta_max, target));
    TRY(use_device(s->g->device));
    PaChoose c;
    TRY(pa_choose(s, dbeta_max, target, &c));
    if (k_out) *k_out = c.k;
    if (dbeta_out) *dbeta_out = c.dbeta_k;
    if (sum_out) *sum_out = c.sum_k;
    if (num_lo_out) *num_lo_out = c.num_lo_k;
    if (num_hi_out) *num_hi_out = c.num_hi_k;
    return ISINGMC_OK;
}

// The schedule is made as it runs: sweeps at beta_start, then { choose; resample with the chosen step, keyed by (seed, step index);
// sweeps } until beta_end.  The host waits once per temperature, for the decision: it needs the beta to build the acceptance tables,
// which go to the device while the resampling runs.  The sweeps of a temperature are in flight while the next search is enqueued.
extern "C" int isingmc_pa_run_adaptive(isingmc_states *s, double beta_start, double beta_end, size_t sweeps_per_beta, uint64_t seed, double target,
                                       double dbeta_cap, size_t max_steps, double *betas_out, size_t *n_betas_out, uint64_t *sum_out,
                                       double *eref_out, uint64_t *distinct_out, double *mean_energy_out)
{
    if (n_betas_out) *n_betas_out = 0;
    if (!betas_out || !n_betas_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    if (!std::isfinite(beta_start) || !std::isfinite(beta_end) || beta_end < beta_start)
        return fail(ISINGMC_ERR_INVALID, "beta_start and beta_end must be finite with beta_start <= beta_end (heating schedules are not chosen)");
    if (!(dbeta_cap > 0.0)) return fail(ISINGMC_ERR_INVALID, "dbeta_cap must be positive (infinity: no cap)");
    TRY(pa_choose_admit(s, 1.0, target));
    TRY(use_device(s->g->device));
    TRY(pa_reserve(s));
    std::unique_ptr<DeviceScratch> tables; // the acceptance tables of the temperature whose sweeps are in flight
    const auto sweep = [&](double beta) {
        tables = std::make_unique<DeviceScratch>(s->stream);
        std::vector<StepPreset> preset;
        TRY(step_presets_build(s, &beta, 1, *tables, preset));
        s->step_preset = &preset[0];
        const int rc = run_steps(s, sweeps_per_beta, &beta, 0, nullptr, nullptr, /*sync=*/false);
        s->step_preset = nullptr;
        return rc;
    };
    // the record of the resampling before the sweeps in flight: read when the stream has drained
    const auto read_record = [&](size_t step) {
        PaRecord rec;
        HIP_TRY(hipMemcpy(&rec, s->pa.d_record, sizeof rec, hipMemcpyDeviceToHost));
        if (sum_out) sum_out[step] = rec.sum;
        if (eref_out) eref_out[step] = rec.eref;
        if (distinct_out) distinct_out[step] = rec.distinct;
        if (mean_energy_out) mean_energy_out[step] = rec.mean;
        return int(ISINGMC_OK);
    };
    double beta = beta_start;
    size_t steps = 0;
    betas_out[0] = beta;
    int rc = sweep(beta);
    while (rc == ISINGMC_OK && beta < beta_end && steps < max_steps) {
        const double dbeta_max = std::min(dbeta_cap, beta_end - beta);
        PaChoose c;
        rc = pa_choose(s, dbeta_max, target, &c); // (waits: the sweeps before are done)
        if (rc != ISINGMC_OK) break;
        tables.reset();
        if (steps) rc = read_record(steps - 1);
        if (rc != ISINGMC_OK) break;
        *n_betas_out = steps + 1; // the temperatures completed
        const double dbeta = c.dbeta_k;
        // the whole of a dbeta_max that reaches beta_end -- the rest of the way (whatever its rounding), or a cap beyond it -- ends the schedule
        const bool reaches = !(dbeta_cap < beta_end - beta) || beta + dbeta_max >= beta_end;
        beta = c.k == PA_CHOOSE_GRID && reaches ? beta_end : beta + dbeta;
        steps++;
        rc = pa_resample_enqueue(s, dbeta, seed, steps, s->pa.d_record);
        if (rc != ISINGMC_OK) break;
        s->pa.have_record = true;
        betas_out[steps] = beta;
        rc = sweep(beta);
    }
    if (rc == ISINGMC_OK && s->rec[REC_BEST].every) rc = best_update_enqueue(s); // the final population
    HIP_TRY(hipStreamSynchronize(s->stream));
    tables.reset();
    TRY(strip_error(strip_check(s)));
    if (rc != ISINGMC_OK) return strip_error(rc);
    if (steps) TRY(read_record(steps - 1));
    *n_betas_out = steps + 1;
    if (beta < beta_end)
        return fail(ISINGMC_ERR_INVALID, "max_steps = " + std::to_string(max_steps) + " temperature steps did not reach beta_end: the population stands at beta " +
                                             std::to_string(beta) + " (n_betas_out temperatures completed)");
    return ISINGMC_OK;
}

extern "C" int isingmc_pa_apply_sources(isingmc_states *s, const uint32_t *src)
{
    if (!s || !src) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    {
        const std::string why = pa_obstacle(s);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    for (size_t j = 0; j < s->R; j++)
        if (src[j] >= s->R) return fail(ISINGMC_ERR_INVALID, "source table entry " + std::to_string(j) + " is not a replica of this container");
    TRY(use_device(s->g->device));
    TRY(pa_reserve(s));
    HIP_TRY(hipMemcpyAsync(s->pa.d_user_src, src, s->R * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    TRY(pa_gather(s, s->pa.d_user_src));
    HIP_TRY(hipStreamSynchronize(s->stream)); // the caller's table is free again
    return strip_error(strip_check(s));
}

extern "C" int isingmc_pa_last(isingmc_states *s, uint32_t *src_out, uint64_t *sum_out, double *eref_out, uint64_t *distinct_out,
                               double *mean_energy_out)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (!s->pa.have_record) return fail(ISINGMC_ERR_INVALID, "no resampling has been run on this container (isingmc_pa_resample)");
    TRY(use_device(s->g->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    TRY(strip_error(strip_check(s)));
    PaRecord rec;
    HIP_TRY(hipMemcpy(&rec, s->pa.d_record, sizeof rec, hipMemcpyDeviceToHost));
    if (src_out) HIP_TRY(hipMemcpy(src_out, s->pa.d_src, std::min(s->R, s->pa.cap) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (sum_out) *sum_out = rec.sum;
    if (eref_out) *eref_out = rec.eref;
    if (distinct_out) *distinct_out = rec.distinct;
    if (mean_energy_out) *mean_energy_out = rec.mean;
    return ISINGMC_OK;
}

extern "C" int isingmc_pa_families(isingmc_states *s, uint32_t *family_out)
{
    if (!s || !family_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    TRY(use_device(s->g->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    TRY(strip_error(strip_check(s)));
    for (size_t r = 0; r < s->R; r++) family_out[r] = uint32_t(r); // slots no resampling has touched found their own family
    if (s->pa.families_set) HIP_TRY(hipMemcpy(family_out, s->pa.d_family, std::min(s->R, s->pa.cap) * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return ISINGMC_OK;
}

extern "C" int isingmc_pa_reset_families(isingmc_states *s)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    {
        const std::string why = pa_obstacle(s);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    if (!s->pa.families_set) return ISINGMC_OK;
    TRY(use_device(s->g->device));
    HIP_TRY(hipStreamSynchronize(s->stream));
    std::vector<uint32_t> family(s->pa.cap);
    for (size_t r = 0; r < family.size(); r++) family[r] = uint32_t(r);
    HIP_TRY(hipMemcpy(s->pa.d_family, family.data(), family.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return ISINGMC_OK;
}
