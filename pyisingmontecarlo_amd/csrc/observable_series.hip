// libisingmc.so: host side of the observable series (isingmc_observable_series_*) -- a device-resident log with one
// row per sample: per column (replica slot, or rung of the ladder) the energy, the magnetisation and the magnetisation by site class.
// A record runs the container's measuring launches (measure_enqueue, as isingmc_get_energies / isingmc_get_magnetisations and the
// tempering rounds do) into counters the series owns, the class counting launches, and behind them the store kernels of
// observable_series_kernels.hip, which write the row entries; nothing comes back to the host before isingmc_observable_series_get.
// Nothing here is a kernel.
#include "internal.hpp"

// rows of {energy f64[n_columns]} {magnetisation i64[n_columns]} {by class i64[n_columns][bins]}, the parts held
struct isingmc_observable_series : SeriesLog {
    explicit isingmc_observable_series(isingmc_states *a_) : SeriesLog(a_, REC_OBSERVABLES, "observable") {}
    const isingmc_site_classes *classes = nullptr;
    unsigned flags = 0;
    size_t n_columns = 0;
    size_t bins = 0, entries = 0; // n_tables * n_classes; 8-byte entries of one column: energy + magnetisation + bins
    DevBlock<unsigned long long> d_sizes; // sizes[n_tables][n_classes]: what the class store subtracts
    DevBlock<unsigned long long> d_cnt;   // [2][counter slots][2]: the counters of one record (the second block: the real-coupling
                                          // family's up spins, whose launch shares its counter with the lo level of the energy)
    DevBlock<unsigned long long> d_cacc;  // the class counters of one batch; grows only behind stream_quiesce of a's stream
    size_t cacc_cap = 0;
};

static bool obs_energy(const isingmc_observable_series *S) { return (S->flags & ISINGMC_OBS_ENERGY) != 0; }
static bool obs_mag(const isingmc_observable_series *S) { return (S->flags & ISINGMC_OBS_MAGNETISATION) != 0; }
static bool obs_by_rung(const isingmc_observable_series *S) { return (S->flags & ISINGMC_OBS_BY_RUNG) != 0; }

// why this container has no observable series ("" when it has): exactly the containers energies_enqueue serves
static std::string obs_obstacle(const isingmc_states *a)
{
    if (a->packed) return "";
    const isingmc_graph *g = a->g;
    if (g->kind != ISINGMC_KIND_LATTICE2D)
        return "an observable series needs a container on the checkerboard lattice path or on a replica-packed family; this graph runs on the f64 CSR "
               "general-graph kernel family (the replica-packed family is chosen by size, or by ISINGMC_FORCE_PACKED=1 / the stable-path flag "
               "at creation)";
    return lattice_obstacle(g, "observable series", true, false);
}

// what ISINGMC_OBS_BY_RUNG asks of the container's ladder ("" when it serves), in the words of ISINGMC_MOMENTS_PER_RUNG
static std::string obs_ladder_obstacle(const isingmc_states *a)
{
    if (!a->tempering.attached)
        return "a series by rung needs a tempering ladder: none is attached to this container (isingmc_pt_attach first, then make the series)";
    if (a->tempering.world != 1 || a->pt.slot_offset != 0 || a->pt.n_rungs != a->R)
        return "a series by rung needs the whole ladder on this container (world size 1, one slot per rung): a shard of a larger ladder is not served";
    return "";
}

extern "C" int isingmc_observable_series_create(isingmc_states *a, const isingmc_site_classes *classes, unsigned flags, size_t capacity,
                                                isingmc_observable_series **out)
{
    if (!a || !out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (flags & ~unsigned(ISINGMC_OBS_ENERGY | ISINGMC_OBS_MAGNETISATION | ISINGMC_OBS_BY_RUNG))
        return fail(ISINGMC_ERR_INVALID, "unknown flag: ISINGMC_OBS_ENERGY, ISINGMC_OBS_MAGNETISATION and ISINGMC_OBS_BY_RUNG are the flags of an observable series");
    {
        const std::string why = obs_obstacle(a);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    if (!(flags & (ISINGMC_OBS_ENERGY | ISINGMC_OBS_MAGNETISATION)) && !classes)
        return fail(ISINGMC_ERR_INVALID, "nothing to log: give ISINGMC_OBS_ENERGY, ISINGMC_OBS_MAGNETISATION or a class set");
    if (capacity == 0) return fail(ISINGMC_ERR_INVALID, "capacity is 0: the log holds no row");
    if (a->R == 0) return fail(ISINGMC_ERR_INVALID, "the container holds no replica: nothing to measure");
    if (flags & ISINGMC_OBS_BY_RUNG) {
        const std::string why = obs_ladder_obstacle(a);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    if (classes) {
        const std::string why = classes_obstacle(classes, a);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    const isingmc_graph *g = a->g;
    const size_t bins = classes ? classes->n_tables * classes->n_classes : 0;
    const size_t entries = ((flags & ISINGMC_OBS_ENERGY) ? 1 : 0) + ((flags & ISINGMC_OBS_MAGNETISATION) ? 1 : 0) + bins;
    TRY(series_budget_or_fail("observable", a->opt.observable_series_bytes, capacity, (unsigned long long)a->R * entries * 8));
    TRY(use_device(g->device));
    std::unique_ptr<isingmc_observable_series> S(new isingmc_observable_series(a));
    S->classes = classes;
    S->flags = flags;
    S->n_columns = a->R;
    S->capacity = capacity;
    S->row = a->R * entries;
    S->bins = bins;
    S->entries = entries;
    TRY(dev_alloc(S->d_log, capacity * S->row));
    TRY(dev_alloc(S->d_cnt, 2 * 2 * counter_slots(a)));
    if (bins) {
        std::vector<unsigned long long> sizes(classes->sizes.begin(), classes->sizes.end());
        TRY(dev_alloc(S->d_sizes, sizes.size()));
        HIP_TRY(hipMemcpy(S->d_sizes, sizes.data(), sizes.size() * sizeof(unsigned long long), hipMemcpyHostToDevice)); // once: waited for here
    }
    if (obs_by_rung(S.get())) a->obs_by_rung_live++;
    *out = S.release();
    return ISINGMC_OK;
}

extern "C" int isingmc_observable_series_destroy(isingmc_observable_series *S)
{
    if (!S) return ISINGMC_OK;
    series_unregister(S);
    if (obs_by_rung(S)) S->a->obs_by_rung_live--;
    delete S;
    return ISINGMC_OK;
}

// The class counters of every slot, batch by batch under a's cluster_workspace_bytes, each batch followed by its store launch.
static int obs_classes_enqueue(isingmc_observable_series *S, const uint32_t *d_perm, long long *row)
{
    isingmc_states *a = S->a;
    const isingmc_graph *g = a->g;
    const size_t bins = S->bins, workspace = size_t(std::max(1, a->opt.cluster_workspace_bytes));
    // an item: a replica of a lattice container, a replica group (32 counter slots) of a packed one
    const size_t items = a->packed ? a->groups : a->R, slots_per_item = a->packed ? 32 : 1;
    const size_t item_bytes = slots_per_item * bins * sizeof(unsigned long long);
    const size_t batch = std::min({items, std::max<size_t>(1, workspace / item_bytes), MAX_GRID_Y});
    if (batch * slots_per_item * bins > S->cacc_cap) TRY(dev_regrow(a->stream, S->d_cacc, &S->cacc_cap, batch * slots_per_item * bins, batch * slots_per_item * bins));
    for (size_t i0 = 0; i0 < items; i0 += batch) {
        const size_t n = std::min(batch, items - i0);
        HIP_TRY(hipMemsetAsync(S->d_cacc, 0, n * item_bytes, a->stream));
        if (a->packed) // the state words themselves as "overlap words": column j of a group = bit j, its set bits = the up spins
            HIP_TRY(overlap_class_launch_packed(a->stream, a->d_state + i0 * g->pk.n_pos, g->pk.n_pos, /*paired=*/false, S->classes->pk, uint32_t(n), S->d_cacc));
        else
            HIP_TRY(obs_launch_lat_class(a->stream, a->d_state + i0 * g->state_words, g->geom, S->classes->lat, uint32_t(n), S->d_cacc));
        // by rung any column may read the batch's slots; else the batch's columns are a range of the row, and the launch covers them alone
        const uint32_t first_slot = uint32_t(counter_slot(a, 0));
        uint32_t column0 = 0, n_columns = uint32_t(S->n_columns);
        if (!d_perm) obs_batch_columns(i0 * slots_per_item, n * slots_per_item, first_slot, uint32_t(S->n_columns), &column0, &n_columns);
        HIP_TRY(obs_launch_class_store(a->stream, ObsClassStore{S->d_cacc, S->d_sizes, d_perm, row, i0 * slots_per_item, n * slots_per_item,
                                                                first_slot, column0, n_columns, uint32_t(bins)}));
    }
    return ISINGMC_OK;
}

// One row for the configurations as they are.  Enqueue only, unless the class workspace has to grow.  Nothing of the container is
// written: the counters are the series' own, so d_meas / meas_zero, meas_fresh and the ladder's energy buffers stay as they are.
static int obs_enqueue(isingmc_observable_series *S)
{
    isingmc_states *a = S->a;
    const isingmc_graph *g = a->g;
    if (a->R != S->n_columns) return fail(ISINGMC_ERR_INVALID, "the container holds another number of replicas than when the series was made: its columns are those replicas");
    const uint32_t *d_perm = nullptr;
    if (obs_by_rung(S)) {
        const std::string why = obs_ladder_obstacle(a); // (the ladder may have been detached and attached again since)
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
        d_perm = a->tempering.d_perm;
    }
    if (a->n_lanes > 1) TRY(lanes_join(a)); // the sweeps before this record may have run on replica lanes
    const size_t C = S->n_columns, slots = counter_slots(a);
    unsigned long long *const row = S->next_row();
    double *row_e = obs_energy(S) ? reinterpret_cast<double *>(row) : nullptr;
    long long *row_m = obs_mag(S) ? reinterpret_cast<long long *>(row) + (obs_energy(S) ? C : 0) : nullptr;
    long long *row_c = reinterpret_cast<long long *>(row) + ((obs_energy(S) ? C : 0) + (obs_mag(S) ? C : 0));
    if (row_e || row_m) {
        unsigned long long *cnt_e = S->d_cnt, *cnt_u = S->d_cnt;
        if (a->packed && a->rj) {
            // the two energy levels in one measurement, the up spins in one more: the second counter of a slot holds either
            if (row_e) TRY(measure_enqueue(a, cnt_e, nullptr, nullptr, /*want_up=*/false));
            if (row_m) {
                if (row_e) cnt_u = S->d_cnt + 2 * slots;
                TRY(measure_enqueue(a, cnt_u, nullptr, nullptr, /*want_up=*/true));
            }
        } else {
            TRY(measure_enqueue(a, cnt_e, nullptr, nullptr, /*want_up=*/true)); // bond and up-spin counters in one pass over the state
        }
        ObsStore st{};
        st.cnt_e = cnt_e;
        st.cnt_u = cnt_u;
        st.perm = d_perm;
        st.row_e = row_e;
        st.row_m = row_m;
        st.family = !a->packed ? OBS_LATTICE : a->rj ? OBS_REAL : OBS_PACKED;
        st.first_slot = uint32_t(counter_slot(a, 0));
        st.n_columns = uint32_t(C);
        st.k_energy = g->rj_k_energy;
        st.jabs = g->jabs;
        st.half_directed = double(int64_t(g->n_directed / 2));
        st.self_energy = g->self_energy;
        st.n_bonds = 2ll * (long long)g->nvars;
        st.nvars = (long long)g->nvars;
        HIP_TRY(obs_launch_store(a->stream, st));
    }
    if (S->bins) TRY(obs_classes_enqueue(S, d_perm, row_c));
    S->timesteps.push_back(a->t);
    return ISINGMC_OK;
}

extern "C" int isingmc_observable_series_record(isingmc_observable_series *S)
{
    if (!S) return fail(ISINGMC_ERR_INVALID, "NULL series");
    TRY(series_full_or_ok(S));
    TRY(use_device(S->a->g->device));
    return obs_enqueue(S);
}

extern "C" int isingmc_observable_series_set_every(isingmc_observable_series *S, size_t every)
{
    if (!S) return fail(ISINGMC_ERR_INVALID, "NULL series");
    if (every == 0) return S->period_off(); // off: the rows stay
    TRY(series_period_free_or_fail(S));
    return S->period_on(every);
}

int obs_sample_enqueue(isingmc_states *s)
{
    isingmc_observable_series *S = static_cast<isingmc_observable_series *>(s->series[REC_OBSERVABLES]);
    TRY(series_full_or_ok(S));
    return obs_enqueue(S);
}

bool obs_sample_by_rung(const isingmc_states *s)
{
    const auto *S = static_cast<const isingmc_observable_series *>(s->series[REC_OBSERVABLES]);
    return S && obs_by_rung(S);
}

extern "C" int isingmc_observable_series_count(const isingmc_observable_series *S, size_t *n, size_t *capacity) { return series_count(S, n, capacity); }

extern "C" int isingmc_observable_series_get(isingmc_observable_series *S, size_t first, size_t n, uint64_t *timesteps_out, double *energy_out,
                                             int64_t *magnetisation_out, int64_t *class_out)
{
    if (!S) return fail(ISINGMC_ERR_INVALID, "NULL series");
    const char *why = energy_out && !obs_energy(S) ? "no energies are held: make the series with ISINGMC_OBS_ENERGY (energy_out may be NULL)"
                      : magnetisation_out && !obs_mag(S) ? "no magnetisations are held: make the series with ISINGMC_OBS_MAGNETISATION (magnetisation_out may be NULL)"
                      : class_out && !S->bins ? "no magnetisations by class are held: make the series with a class set (class_out may be NULL)" : nullptr;
    std::vector<unsigned long long> h;
    TRY(series_read(S, first, n, why, timesteps_out, energy_out || magnetisation_out || class_out, h));
    const size_t C = S->n_columns, row = S->row;
    const size_t off_m = obs_energy(S) ? C : 0, off_c = off_m + (obs_mag(S) ? C : 0);
    for (size_t i = 0; i < h.size() / row; i++) {
        const unsigned long long *r = h.data() + i * row;
        if (energy_out) std::memcpy(energy_out + i * C, r, C * sizeof(double));
        if (magnetisation_out) std::memcpy(magnetisation_out + i * C, r + off_m, C * sizeof(int64_t));
        if (class_out) std::memcpy(class_out + i * C * S->bins, r + off_c, C * S->bins * sizeof(int64_t));
    }
    return ISINGMC_OK;
}

extern "C" int isingmc_observable_series_reset(isingmc_observable_series *S) { return series_reset(S); }
