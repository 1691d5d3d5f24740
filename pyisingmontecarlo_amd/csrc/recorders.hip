// libisingmc.so: the measurements the step loop takes on a period -- minimum tracking, the moment sums (S18), the
// overlap series (S21), the observable series (S22), the lag ring (S26) -- as one table with the functions over it that serve every place which has to
// know all recorders (a new recorder is a row), and the log core the series share.  The cluster series (S24) is a row too: it has
// no period, the non-local steps append its rows, but it can run full and it objects to what the others object to.  Nothing here is
// a kernel.
#include "internal.hpp"

// Plain function pointers in a constant table (as OverlapSink argues in internal.hpp: nothing on the sampling path allocates).
struct RecorderRow {
    int (*enqueue)(isingmc_states *);                    // one sample at timestep s->t
    int (*room_or_fail)(const isingmc_states *, size_t); // before a run enqueues anything; nullptr: the recorder cannot run full
    bool replay_guard; // the repeat of a call skips the samples its first attempt took (minimum tracking: it finds the same records again)
    bool restarts;     // isingmc_states_set_timestep counts the sample points from the new timestep (minimum tracking: t0 stays 0)
    const char *refuse_append, *refuse_resample; // why replicas cannot be added / resampled while it is on (nullptr: they can)
    bool (*live)(const isingmc_states *) = nullptr; // on without a period or a series in the container's slot (nullptr: never)
};

static const RecorderRow RECORDERS[REC_COUNT] = {
    {best_update_enqueue, nullptr, false, false,
     "minimum tracking is switched on for this container (isingmc_states_set_track_best): its records are sized for the replicas it holds; switch tracking on after the graphs are added", nullptr},
    {moments_sample_enqueue, nullptr, true, true,
     "moment sums are switched on for this container (isingmc_states_set_moments_every): they are sized for the replicas it holds; switch accumulation on after the graphs are added",
     "moment sums are switched on for this container (isingmc_states_set_moments_every): a resampling replaces the replicas whose samples they hold; switch accumulation off first"},
    {osr_sample_enqueue, [](const isingmc_states *s, size_t n) { return series_room_or_fail(s, REC_OVERLAPS, n); }, true, true,
     "an overlap series records on a period for this container (isingmc_overlap_series_set_every): its pairs are those of the replicas it holds; switch the period on after the graphs are added",
     "an overlap series records on a period for this container (isingmc_overlap_series_set_every): a resampling replaces the replicas whose pairs it follows; switch the period off first"},
    {obs_sample_enqueue, [](const isingmc_states *s, size_t n) { return series_room_or_fail(s, REC_OBSERVABLES, n); }, true, true,
     "an observable series records on a period for this container (isingmc_observable_series_set_every): its columns are the replicas it holds; switch the period on after the graphs are added",
     "an observable series records on a period for this container (isingmc_observable_series_set_every): a resampling replaces the replicas whose columns it follows; switch the period off first"},
    {autocorr_sample_enqueue, nullptr, true, true,
     "a lag ring is live on this container (isingmc_autocorr_create): its snapshots and sums are sized for the replicas it holds; make the ring after the graphs are added",
     "a lag ring is live on this container (isingmc_autocorr_create): a resampling replaces the replicas whose snapshots it holds; destroy the ring first",
     [](const isingmc_states *s) { return s->acr.live; }},
    {nullptr, cluster_series_room_or_fail, false, false, // (never due: the rows are the non-local steps'; a repeat writes them again, below)
     "a cluster series is live on this container (isingmc_cluster_series_create): its columns are the replicas it holds; make the series after the graphs are added",
     "a cluster series is live on this container (isingmc_cluster_series_create): a resampling replaces the replicas whose columns it follows; destroy the series first"},
};

int recorders_sample(isingmc_states *s, bool after_strip, int &rc)
{
    for (int i = 0; i < REC_COUNT; i++) {
        Periodic &p = s->rec[i];
        if (rc != ISINGMC_OK || !p.due(s->t)) continue;
        if (s->strip.guard && after_strip) {
            HIP_TRY(hipStreamSynchronize(s->stream));
            rc = strip_check(s);
        }
        if (rc == ISINGMC_OK) rc = recorder_sample_now(s, Recorder(i));
    }
    return ISINGMC_OK;
}

int recorder_sample_now(isingmc_states *s, Recorder which)
{
    Periodic &p = s->rec[which];
    if (!p.due(s->t)) return ISINGMC_OK;
    TRY(RECORDERS[which].enqueue(s));
    p.last_t = s->t;
    return ISINGMC_OK;
}

int recorders_room_or_fail(const isingmc_states *s, size_t timesteps)
{
    for (const RecorderRow &r : RECORDERS)
        if (r.room_or_fail) TRY(r.room_or_fail(s, timesteps));
    return ISINGMC_OK;
}

void recorders_restart(isingmc_states *s, uint64_t t)
{
    for (int i = 0; i < REC_COUNT; i++)
        if (RECORDERS[i].restarts) s->rec[i].restart(t);
}

void recorders_replay_since(isingmc_states *s, uint64_t t0)
{
    for (int i = 0; i < REC_COUNT; i++)
        if (RECORDERS[i].replay_guard) s->rec[i].replay_since(t0);
    cluster_series_replay_since(s, t0);
}

const char *recorders_refusal(const isingmc_states *s, RecorderRefusal what)
{
    for (int i = 0; i < REC_COUNT; i++) {
        const char *why = what == RecorderRefusal::Append ? RECORDERS[i].refuse_append : RECORDERS[i].refuse_resample;
        const bool on = s->rec[i].every || s->series[i] || (RECORDERS[i].live && RECORDERS[i].live(s)); // a period, the series in the container's slot, a row's own state
        if (on && why) return why;
    }
    return nullptr;
}

// ---- the log core of the two series ------------------------------------------------------------------------------------------
int series_budget_or_fail(const char *noun, long long budget_option, size_t capacity, unsigned long long row_bytes)
{
    const unsigned long long budget = (unsigned long long)std::max(0ll, budget_option); // (row_bytes < 2^32 x 8194 x 8: no overflow)
    if (row_bytes <= budget && capacity <= budget / row_bytes) return ISINGMC_OK;
    return fail(ISINGMC_ERR_INVALID, "a log of " + std::to_string(capacity) + " rows of " + std::to_string(row_bytes) +
                                         " bytes is larger than the option " + noun + "_series_bytes = " + std::to_string(budget) +
                                         " allows (isingmc_states_set_option raises the budget)");
}

int series_full_or_ok(const SeriesLog *L)
{
    if (L->timesteps.size() < L->capacity) return ISINGMC_OK;
    const std::string noun = L->noun;
    return fail(ISINGMC_ERR_INVALID, "the " + noun + " series is full: it holds " + std::to_string(L->capacity) + " rows, its capacity (isingmc_" +
                                         noun + "_series_get, then isingmc_" + noun + "_series_reset)");
}

int series_room_or_fail(const isingmc_states *s, Recorder which, size_t timesteps)
{
    const SeriesLog *L = s->series[which];
    if (!s->rec[which].every || !L) return ISINGMC_OK;
    const uint64_t samples = s->rec[which].points(s->t, timesteps); // sample points: t0 + every, t0 + 2 every, ...
    const size_t have = L->timesteps.size();
    if (samples <= L->capacity - have) return ISINGMC_OK;
    const std::string noun = L->noun;
    return fail(ISINGMC_ERR_INVALID, "the " + noun + " series of this container would run full: the call takes " + std::to_string(samples) +
                                         " samples and the log has room for " + std::to_string(L->capacity - have) + " of its " +
                                         std::to_string(L->capacity) + " rows (isingmc_" + noun + "_series_get, then isingmc_" + noun +
                                         "_series_reset; or switch the period off)");
}

int series_period_free_or_fail(const SeriesLog *L)
{
    const SeriesLog *other = L->a->series[L->which];
    if (!other || other == L) return ISINGMC_OK;
    return fail(ISINGMC_ERR_INVALID, std::string("another ") + L->noun + " series of this container records on a period already: one periodic series per container");
}

int series_count(const SeriesLog *L, size_t *n_out, size_t *capacity_out)
{
    if (!L) return fail(ISINGMC_ERR_INVALID, "NULL series");
    if (n_out) *n_out = L->timesteps.size();
    if (capacity_out) *capacity_out = L->capacity;
    return ISINGMC_OK;
}

int series_reset(SeriesLog *L)
{
    if (!L) return fail(ISINGMC_ERR_INVALID, "NULL series");
    // rows enqueued so far still land in the log, ahead on a's stream of whatever overwrites them: nothing to wait for
    L->timesteps.clear();
    if (L->periodic()) L->a->rec[L->which].last_t = 0;
    return ISINGMC_OK;
}

int series_read(SeriesLog *L, size_t first, size_t n, const char *refusal, uint64_t *timesteps_out, bool want_rows, std::vector<unsigned long long> &rows)
{
    const size_t have = L->timesteps.size();
    if (first > have || n > have - first) return fail(ISINGMC_ERR_INVALID, "rows out of range: the series holds " + std::to_string(have) + " rows");
    if (refusal) return fail(ISINGMC_ERR_INVALID, refusal);
    isingmc_states *a = L->a;
    TRY(use_device(a->g->device));
    HIP_TRY(hipStreamSynchronize(a->stream));
    TRY(strip_error(strip_check(a)));
    if (timesteps_out) std::copy(L->timesteps.begin() + first, L->timesteps.begin() + first + n, timesteps_out);
    if (n == 0 || !want_rows) return ISINGMC_OK;
    return read_back(a, rows, L->d_log.get() + first * L->row, n * L->row);
}

void series_unregister(SeriesLog *L)
{
    isingmc_states *a = L->a;
    (void)hipSetDevice(a->g->device);
    (void)stream_quiesce(a->stream); // the blocks go back to the cache: no record may still be running
    L->period_off();
}
