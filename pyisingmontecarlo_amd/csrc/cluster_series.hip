// libisingmc.so: host side of the cluster series (isingmc_cluster_series_*) -- a device-resident log with one row per
// non-local step of its container: per column (replica of a Swendsen-Wang step, pair of an isoenergetic move) the number of
// clusters, the largest, and the sums of s, s^2 and s^4 over the cluster sizes.  The step itself forms the sums, in the launch
// that finds its largest cluster (cluster_moments.hpp); run_cluster_step / run_icm_step of nonlocal.hip bracket their batches with
// cluster_series_begin / _end below.  Nothing comes back to the host before isingmc_cluster_series_get.  Nothing here is a kernel.
#include "internal.hpp"

// rows of uint64[n_columns][CLS_ROW]; the container's slot s->series[REC_CLUSTERS] holds the one live series
struct isingmc_cluster_series : SeriesLog {
    explicit isingmc_cluster_series(isingmc_states *a_) : SeriesLog(a_, REC_CLUSTERS, "cluster") {}
    int kind = ISINGMC_CLUSTER_SERIES_SW;
    size_t n_columns = 0;
};

static isingmc_cluster_series *live_series(const isingmc_states *s) { return static_cast<isingmc_cluster_series *>(s->series[REC_CLUSTERS]); }

extern "C" int isingmc_cluster_series_create(isingmc_states *a, int kind, size_t capacity, isingmc_cluster_series **out)
{
    if (!a || !out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (kind != ISINGMC_CLUSTER_SERIES_SW && kind != ISINGMC_CLUSTER_SERIES_ICM)
        return fail(ISINGMC_ERR_INVALID, "unknown kind: ISINGMC_CLUSTER_SERIES_SW and ISINGMC_CLUSTER_SERIES_ICM are the kinds of a cluster series");
    if (live_series(a)) return fail(ISINGMC_ERR_INVALID, "this container has a live cluster series already: one cluster series per container (isingmc_cluster_series_destroy first)");
    if (kind == ISINGMC_CLUSTER_SERIES_SW) {
        const std::string why = cluster_obstacle(a);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
        if (a->icm.every) return fail(ISINGMC_ERR_INVALID, "isoenergetic cluster moves are switched on for this container (isingmc_states_set_icm_every): one non-local move at a time");
    } else {
        const std::string why = icm_obstacle(a);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    if (capacity == 0) return fail(ISINGMC_ERR_INVALID, "capacity is 0: the log holds no row");
    const size_t columns = kind == ISINGMC_CLUSTER_SERIES_SW ? a->R : a->R / 2;
    if (columns == 0)
        return fail(ISINGMC_ERR_INVALID, kind == ISINGMC_CLUSTER_SERIES_SW ? "the container holds no replica: no cluster step to log"
                                                                           : "the container holds no pair of replicas: no isoenergetic cluster move to log");
    TRY(series_budget_or_fail("cluster", a->opt.cluster_series_bytes, capacity, (unsigned long long)columns * CLS_ROW * 8));
    TRY(use_device(a->g->device));
    std::unique_ptr<isingmc_cluster_series> S(new isingmc_cluster_series(a));
    S->kind = kind;
    S->n_columns = columns;
    S->capacity = capacity;
    S->row = columns * CLS_ROW;
    TRY(dev_alloc(S->d_log, capacity * S->row));
    a->series[REC_CLUSTERS] = S.get();
    *out = S.release();
    return ISINGMC_OK;
}

extern "C" int isingmc_cluster_series_destroy(isingmc_cluster_series *S)
{
    if (!S) return ISINGMC_OK;
    series_unregister(S); // (drains a's stream; the container's slot is free again)
    delete S;
    return ISINGMC_OK;
}

extern "C" int isingmc_cluster_series_count(const isingmc_cluster_series *S, size_t *n, size_t *capacity) { return series_count(S, n, capacity); }

extern "C" int isingmc_cluster_series_get(isingmc_cluster_series *S, size_t first, size_t n, uint64_t *timesteps_out, uint64_t *rows_out)
{
    if (!S) return fail(ISINGMC_ERR_INVALID, "NULL series");
    std::vector<unsigned long long> h;
    TRY(series_read(S, first, n, nullptr, timesteps_out, rows_out != nullptr, h));
    if (rows_out && !h.empty()) std::memcpy(rows_out, h.data(), h.size() * sizeof(unsigned long long));
    return ISINGMC_OK;
}

extern "C" int isingmc_cluster_series_reset(isingmc_cluster_series *S) { return series_reset(S); }

extern "C" int isingmc_host_nonlocal_steps(uint64_t t0, size_t timesteps, size_t k, uint64_t *steps_out)
{
    if (!steps_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    if (t0 + timesteps < t0) return fail(ISINGMC_ERR_INVALID, "t0 + timesteps is beyond 2^64");
    *steps_out = nonlocal_steps_in(t0, timesteps, k);
    return ISINGMC_OK;
}

// the period whose steps append rows to S
static size_t series_every(const isingmc_states *s, const isingmc_cluster_series *S)
{
    return S->kind == ISINGMC_CLUSTER_SERIES_SW ? s->cl.every : s->icm.every;
}

int cluster_series_room_or_fail(const isingmc_states *s, size_t timesteps)
{
    const isingmc_cluster_series *S = live_series(s);
    if (!S || s->R == 0) return ISINGMC_OK; // (an empty container takes no step)
    const uint64_t steps = nonlocal_steps_in(s->t, timesteps, series_every(s, S));
    const size_t have = S->timesteps.size();
    if (steps <= S->capacity - have) return ISINGMC_OK;
    return fail(ISINGMC_ERR_INVALID, "the cluster series of this container would run full: the call takes " + std::to_string(steps) +
                                         " non-local steps and the log has room for " + std::to_string(S->capacity - have) + " of its " +
                                         std::to_string(S->capacity) + " rows (isingmc_cluster_series_get, then isingmc_cluster_series_reset)");
}

void cluster_series_replay_since(isingmc_states *s, uint64_t t0)
{
    isingmc_cluster_series *S = live_series(s);
    if (!S) return;
    // the rows of the attempt that is repeated: its steps are taken again from the restored configurations and land in the same rows
    while (!S->timesteps.empty() && S->timesteps.back() >= t0) S->timesteps.pop_back();
}

int cluster_series_begin(isingmc_states *s, int kind, ClusterMomentsOut *out)
{
    isingmc_cluster_series *S = live_series(s);
    *out = ClusterMomentsOut{};
    if (!S || S->kind != kind) return ISINGMC_OK;
    TRY(series_full_or_ok(S)); // (run_steps has counted the call's steps before: a backstop)
    const size_t columns = kind == ISINGMC_CLUSTER_SERIES_SW ? s->R : s->R / 2;
    if (columns != S->n_columns) return fail(ISINGMC_ERR_INVALID, "the container holds another number of replicas than when the cluster series was made: its columns are those replicas");
    out->row = S->next_row();
    out->first_slot = uint32_t(!s->packed ? 0 : kind == ISINGMC_CLUSTER_SERIES_SW ? s->pk_bit0 : s->pk_bit0 / 2); // (pk_bit0 is even with pairs)
    out->n_cols = uint32_t(columns);
    HIP_TRY(hipMemsetAsync(out->row, 0, S->row * sizeof(unsigned long long), s->stream));
    return ISINGMC_OK;
}

int cluster_series_end(isingmc_states *s, const ClusterMomentsOut &out, const uint32_t *stats, const uint32_t *minus)
{
    isingmc_cluster_series *S = live_series(s);
    HIP_TRY(cluster_series_launch_store(s->stream, stats, minus, s->g->nvars, out.first_slot, out.n_cols, out.row));
    S->timesteps.push_back(s->t);
    return ISINGMC_OK;
}
