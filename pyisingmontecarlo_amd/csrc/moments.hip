// libisingmc.so: per-site spin sums and per-bond sums over the samples of a run, kept on the device (by rung of a tempering ladder S19;
// isingmc_moments_* and isingmc_states_set_moments_every) -- which containers are served, the totals and their byte budget, the
// sample enqueued behind a timestep, the read-out in the site numbering and edge order of graph creation.  Nothing here is a
// kernel: they are in moments_kernels.hip, whose header states what is counted and where.
#include "internal.hpp"

static bool mom_per_replica(unsigned flags) { return (flags & ISINGMC_MOMENTS_PER_REPLICA) != 0; }
static bool mom_bonds(unsigned flags) { return (flags & ISINGMC_MOMENTS_BONDS) != 0; }
static bool mom_per_rung(unsigned flags) { return (flags & ISINGMC_MOMENTS_PER_RUNG) != 0; }
// the per-replica and the per-rung sums share time planes and 32-bit totals of the state's shape: their rows are slots or rungs
static bool mom_rows(unsigned flags) { return mom_per_replica(flags) || mom_per_rung(flags); }
static size_t mom_state_words(const isingmc_states *s) { return s->packed ? s->groups * size_t(s->g->pk.n_pos) : s->R * s->g->state_words; }

// device bytes of the sums of this container as it is now
static unsigned long long mom_bytes(const isingmc_states *s, unsigned flags, int k)
{
    const isingmc_graph *g = s->g;
    if (mom_rows(flags)) return (unsigned long long)(k + 32) * mom_state_words(s) * sizeof(uint32_t);
    if (!s->packed) return (mom_bonds(flags) ? 3ull : 1ull) * 32 * g->state_words * sizeof(unsigned long long);
    return g->pk.n_pos * sizeof(unsigned long long) + (mom_bonds(flags) ? g->n_edges * (sizeof(unsigned long long) + sizeof(uint2)) : 0ull);
}

// why this container cannot accumulate these sums ("" when it can): exactly the containers isingmc_overlaps serves; no side effects
static std::string mom_obstacle(const isingmc_states *s, unsigned flags)
{
    const isingmc_graph *g = s->g;
    if (flags & ~unsigned(ISINGMC_MOMENTS_PER_REPLICA | ISINGMC_MOMENTS_BONDS | ISINGMC_MOMENTS_PER_RUNG))
        return "unknown flag: ISINGMC_MOMENTS_PER_REPLICA, ISINGMC_MOMENTS_BONDS and ISINGMC_MOMENTS_PER_RUNG are the flags of the moment sums";
    if (mom_per_rung(flags) && (mom_per_replica(flags) || mom_bonds(flags)))
        return "sums per rung go alone: ISINGMC_MOMENTS_PER_RUNG takes neither ISINGMC_MOMENTS_PER_REPLICA (a rung is held by one slot at a time) "
               "nor ISINGMC_MOMENTS_BONDS (bond sums per rung are not offered)";
    if (mom_per_replica(flags) && mom_bonds(flags))
        return "bond sums per replica are not offered: ISINGMC_MOMENTS_BONDS goes with the sums over all replicas only";
    if (!s->packed) {
        if (g->kind != ISINGMC_KIND_LATTICE2D)
            return "moment sums need containers on the checkerboard lattice path or on a replica-packed family; this graph runs on the f64 CSR "
                   "general-graph kernel family (the replica-packed family is chosen by size, or by ISINGMC_FORCE_PACKED=1 / the stable-path flag "
                   "at creation)";
        const std::string why = lattice_obstacle(g, "moment sums", true, false);
        if (!why.empty()) return why;
    }
    if (s->tempering.attached && !mom_per_rung(flags))
        return "a tempering ladder is attached: a slot changes its temperature at every exchange, so sums per slot or over all slots mix the "
               "temperatures (ISINGMC_MOMENTS_PER_RUNG sums by rung; or isingmc_pt_detach first)";
    if (mom_per_rung(flags) && !s->tempering.attached)
        return "sums per rung need a tempering ladder: none is attached to this container (isingmc_pt_attach first, then switch the sums on)";
    if (mom_per_rung(flags) && (s->tempering.world != 1 || s->pt.slot_offset != 0 || s->pt.n_rungs != s->R))
        return "sums per rung need the whole ladder on this container (world size 1, one slot per rung): a shard of a larger ladder is not served";
    if (mom_bonds(flags) && !g->edge_order_kept)
        return "this lattice is too large for bond sums in the order of its edge list (2 W H must stay below 2^32 unless entry e is bond e)";
    if (mom_bonds(flags) && s->packed && (g->n_edges >> 32)) return "bond sums serve at most 2^32 - 1 edge-list entries";
    if (s->R >> 31) return "moment sums serve at most 2^31 - 1 replicas";
    const int k = s->opt.moments_planes;
    if (mom_rows(flags) && (k < 1 || k > MOM_MAX_TIME_PLANES)) return "the option moments_planes must be 1 .. 16";
    const unsigned long long need = mom_bytes(s, flags, k), budget = (unsigned long long)std::max(0ll, s->opt.moments_bytes);
    if (need > budget)
        return "the moment sums of this container take " + std::to_string(need) + " bytes of device memory, more than the option moments_bytes = " +
               std::to_string(budget) + " allows (per-replica and per-rung totals are 32 times the state; isingmc_states_set_option raises the budget)";
    return "";
}

static int mom_zero_enqueue(isingmc_states *s)
{
    const unsigned flags = s->mom.flags;
    if (mom_rows(flags)) {
        const size_t words = mom_state_words(s);
        HIP_TRY(hipMemsetAsync(s->mom.d_planes, 0, size_t(s->mom.k) * words * sizeof(uint32_t), s->stream));
        HIP_TRY(hipMemsetAsync(s->mom.d_totals, 0, 32 * words * sizeof(uint32_t), s->stream));
    } else if (!s->packed) {
        HIP_TRY(hipMemsetAsync(s->mom.d_site, 0, (mom_bonds(flags) ? 3 : 1) * 32 * s->g->state_words * sizeof(unsigned long long), s->stream));
    } else {
        HIP_TRY(hipMemsetAsync(s->mom.d_site, 0, s->g->pk.n_pos * sizeof(unsigned long long), s->stream));
        if (mom_bonds(flags)) HIP_TRY(hipMemsetAsync(s->mom.d_bond, 0, std::max<size_t>(s->g->n_edges, 1) * sizeof(unsigned long long), s->stream));
    }
    s->mom.n = 0;
    s->mom.pending = 0;
    return ISINGMC_OK;
}

// The sums for `flags`, sized for the container as it is now.  Sums of the same mode, planes and replica count are kept as they
// are (accumulation switched off and on again goes on counting); anything else starts from zero.
static int mom_reserve(isingmc_states *s, unsigned flags)
{
    const isingmc_graph *g = s->g;
    const int k = mom_rows(flags) ? s->opt.moments_planes : 0;
    if (s->mom.have && s->mom.flags == flags && s->mom.R == s->R && s->mom.k == k) return ISINGMC_OK;
    HIP_TRY(stream_quiesce(s->stream)); // recycled blocks: nothing enqueued may still use the old ones
    s->mom.d_site.reset(); s->mom.d_bond.reset(); s->mom.d_edges.reset(); s->mom.d_planes.reset(); s->mom.d_totals.reset();
    s->mom.have = false;
    if (mom_rows(flags)) {
        const size_t words = mom_state_words(s);
        TRY(dev_alloc(s->mom.d_planes, size_t(k) * words));
        TRY(dev_alloc(s->mom.d_totals, 32 * words));
    } else if (!s->packed) {
        TRY(dev_alloc(s->mom.d_site, (mom_bonds(flags) ? 3 : 1) * 32 * g->state_words));
    } else {
        TRY(dev_alloc(s->mom.d_site, g->pk.n_pos));
        if (mom_bonds(flags)) {
            std::vector<uint2> ends(g->n_edges);
            for (size_t e = 0; e < g->n_edges; e++) ends[e] = make_uint2(uint32_t(g->pos[g->edge_ends[2 * e]]), uint32_t(g->pos[g->edge_ends[2 * e + 1]]));
            TRY(dev_alloc(s->mom.d_bond, g->n_edges));
            TRY(dev_alloc(s->mom.d_edges, g->n_edges));
            if (g->n_edges) HIP_TRY(hipMemcpy(s->mom.d_edges, ends.data(), ends.size() * sizeof(uint2), hipMemcpyHostToDevice));
        }
    }
    s->mom.flags = flags;
    s->mom.R = s->R;
    s->mom.k = k;
    s->mom.have = true;
    return mom_zero_enqueue(s);
}

extern "C" int isingmc_states_set_moments_every(isingmc_states *s, size_t every, unsigned flags)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (every) {
        const std::string why = mom_obstacle(s, flags);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
        TRY(use_device(s->g->device));
        TRY(mom_reserve(s, flags));
        s->rec[REC_MOMENTS].restart(s->t);
    }
    s->rec[REC_MOMENTS].every = every;
    return ISINGMC_OK;
}

extern "C" int isingmc_states_moments_every(const isingmc_states *s, size_t *every_out, unsigned *flags_out)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (every_out) *every_out = s->rec[REC_MOMENTS].every;
    if (flags_out) *flags_out = s->mom.flags;
    return ISINGMC_OK;
}

static int mom_flush_enqueue(isingmc_states *s)
{
    if (!s->mom.pending) return ISINGMC_OK;
    const size_t rows = s->packed ? s->groups : s->R, row_words = s->packed ? size_t(s->g->pk.n_pos) : size_t(s->g->state_words);
    HIP_TRY(moments_launch_flush(s->stream, s->mom.d_planes, rows, row_words, s->mom.k, s->mom.d_totals));
    s->mom.pending = 0;
    return ISINGMC_OK;
}

int moments_sample_enqueue(isingmc_states *s)
{
    if (s->R == 0) return ISINGMC_OK;
    if (s->n_lanes > 1) TRY(lanes_join(s)); // the sweeps before this sample may have run on replica lanes
    const isingmc_graph *g = s->g;
    const unsigned flags = s->mom.flags;
    if (mom_rows(flags)) {
        if (s->mom.n >= 0xFFFFFFFFull) return fail(ISINGMC_ERR_INVALID, "the per-replica and per-rung totals are 32-bit counts: 2^32 - 1 samples are in them (isingmc_moments_reset)");
        if (!mom_per_rung(flags))
            HIP_TRY(moments_launch_add(s->stream, s->d_state, mom_state_words(s), s->mom.k, s->mom.d_planes));
        // per rung: the permutation is read by the kernel, as the exchange rounds enqueued so far leave it
        else if (!s->packed)
            HIP_TRY(moments_launch_add_by_rung(s->stream, s->d_state, s->tempering.d_perm, s->R, g->state_words, s->mom.k, s->mom.d_planes));
        else
            HIP_TRY(moments_launch_packed_add_by_rung(s->stream, s->d_state, s->tempering.d_perm, s->R, g->pk.n_pos, uint32_t(s->pk_bit0), mom_state_words(s),
                                                      s->mom.k, s->mom.d_planes));
        if (++s->mom.pending == (1u << s->mom.k) - 1) TRY(mom_flush_enqueue(s));
    } else if (!s->packed) {
        HIP_TRY(moments_launch_lattice_sum(s->stream, s->d_state, g->geom, s->R, mom_bonds(flags), s->mom.d_site));
    } else {
        HIP_TRY(moments_launch_packed_sum(s->stream, s->d_state, g->pk.n_pos, s->groups, uint32_t(s->pk_bit0), uint32_t(s->R), s->mom.d_site,
                                          s->mom.d_edges, mom_bonds(flags) ? size_t(g->n_edges) : 0, s->mom.d_bond));
    }
    s->mom.n++;
    return ISINGMC_OK;
}

extern "C" int isingmc_moments_accumulate(isingmc_states *s)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    const unsigned flags = s->mom.have ? s->mom.flags : 0u; // never switched on: the sums over all replicas, sites alone
    {
        const std::string why = mom_obstacle(s, flags);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    TRY(use_device(s->g->device));
    TRY(mom_reserve(s, flags));
    return moments_sample_enqueue(s);
}

extern "C" int isingmc_moments_reset(isingmc_states *s)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (!s->mom.have) return ISINGMC_OK; // nothing counted yet
    TRY(use_device(s->g->device));
    return mom_zero_enqueue(s);
}

// The sampling run of isingmc_run_sampling with the samples summed on the device instead of copied out: thermalise, then
// n_samples x { sampling_freq timesteps; one sample }, everything enqueued back to back; the one wait is the final energies'.
static int run_sampling_moments_impl(isingmc_states *s, double beta, size_t thermalization, size_t sampling_freq, size_t n_samples)
{
    struct BetaGuard { // a uniform beta as per-replica thresholds for the call: the step launches need no host tables (run_sampling_impl)
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
        ~Off() { s->rec[REC_MOMENTS].every = 0; }
    } off{s};
    s->rec[REC_MOMENTS].every = 0;
    TRY(run_steps(s, thermalization, nullptr, 0, nullptr, nullptr, /*sync=*/false));
    s->rec[REC_MOMENTS].every = sampling_freq;
    s->rec[REC_MOMENTS].t0 = s->t;
    TRY(run_steps(s, n_samples * sampling_freq, nullptr, 0, nullptr, nullptr, /*sync=*/false));
    if (!s->strip.guard) return ISINGMC_OK;
    HIP_TRY(hipStreamSynchronize(s->stream)); // (a call that may be repeated: what the last strip launch left is checked here)
    return strip_check(s);
}

extern "C" int isingmc_run_sampling_moments(isingmc_states *s, double beta, size_t thermalization, size_t sampling_freq, size_t n_samples,
                                            unsigned flags, double *energies_out)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (sampling_freq == 0) return fail(ISINGMC_ERR_INVALID, "sampling_freq must be positive");
    if (!s->has_betas && !std::isfinite(beta)) return fail(ISINGMC_ERR_INVALID, "beta must be finite");
    if (mom_per_rung(flags))
        return fail(ISINGMC_ERR_INVALID, "the sampling run takes no ISINGMC_MOMENTS_PER_RUNG: it runs no exchange rounds; a ladder runs through isingmc_pt_run / "
                                         "isingmc_pt_time_steps with the sums switched on (isingmc_states_set_moments_every)");
    if (s->rec[REC_MOMENTS].every) return fail(ISINGMC_ERR_INVALID, "moment sums are switched on for this container already: the sampling run sets its own period (switch accumulation off first)");
    {
        const std::string why = mom_obstacle(s, flags);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    TRY(recorders_room_or_fail(s, thermalization + sampling_freq * n_samples));
    TRY(use_device(s->g->device));
    TRY(mom_reserve(s, flags));
    TRY(mom_zero_enqueue(s));
    s->rec[REC_MOMENTS].last_t = 0;
    const bool may_strip = may_use_strips(s) && (strip_plan(s, thermalization).use || strip_plan(s, n_samples * sampling_freq).use);
    TRY(with_strip_retry(s, may_strip, [&] { return run_sampling_moments_impl(s, beta, thermalization, sampling_freq, n_samples); }));
    if (mom_rows(s->mom.flags)) TRY(mom_flush_enqueue(s));
    if (energies_out) return isingmc_get_energies(s, energies_out); // waits
    HIP_TRY(hipStreamSynchronize(s->stream));
    return strip_error(strip_check(s));
}

extern "C" int isingmc_moments_get(isingmc_states *s, uint64_t *n_samples_out, int64_t *site_out, int64_t *bond_out)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (!s->mom.have || s->mom.R != s->R)
        return fail(ISINGMC_ERR_INVALID, "this container holds no moment sums: switch accumulation on (isingmc_states_set_moments_every) or call isingmc_moments_accumulate first");
    const unsigned flags = s->mom.flags;
    if (bond_out && !mom_bonds(flags)) return fail(ISINGMC_ERR_INVALID, "no bond sums are held: switch accumulation on with ISINGMC_MOMENTS_BONDS (bond_out may be NULL)");
    TRY(use_device(s->g->device));
    const isingmc_graph *g = s->g;
    if (mom_rows(flags)) TRY(mom_flush_enqueue(s));
    HIP_TRY(hipStreamSynchronize(s->stream));
    TRY(strip_error(strip_check(s)));
    if (n_samples_out) *n_samples_out = s->mom.n;
    const int64_t n = int64_t(s->mom.n), nR = n * int64_t(s->R);
    const size_t N = g->nvars;
    if (mom_rows(flags)) { // row r: replica r's slot, or rung r itself
        const bool by_rung = mom_per_rung(flags);
        if (!site_out || s->R == 0) return ISINGMC_OK;
        std::vector<uint32_t> h;
        TRY(read_back(s, h, s->mom.d_totals.get(), 32 * mom_state_words(s)));
        if (s->packed) { // totals[slot or rung][n_pos]
            const size_t n_pos = g->pk.n_pos;
            parallel_for(s->R, [&](size_t r) {
                const uint32_t *row = h.data() + (by_rung ? r : counter_slot(s, r)) * n_pos;
                for (size_t i = 0; i < N; i++) site_out[r * N + i] = 2 * int64_t(row[g->pos[i]]) - n;
            }, N * 8);
        } else { // totals[replica or rung][32][state words]
            const LatGeom &L = g->geom;
            const size_t sw = g->state_words;
            parallel_for(s->R, [&](size_t r) {
                const uint32_t *rep = h.data() + r * 32 * sw;
                for (uint32_t y = 0; y < L.H; y++)
                    for (uint32_t x = 0; x < L.W; x++) {
                        const uint32_t i = x >> 1;
                        const size_t w = size_t((x + y) & 1) * L.wpp + size_t(y) * L.wpr + (i >> 5);
                        site_out[r * N + size_t(y) * L.W + x] = 2 * int64_t(rep[size_t(i & 31) * sw + w]) - n;
                    }
            }, N * 8);
        }
        return ISINGMC_OK;
    }
    std::vector<unsigned long long> h;
    if (!s->packed) { // totals[kind][32][state words]; plane order as pack_state
        const LatGeom &L = g->geom;
        const size_t sw = g->state_words;
        const bool bonds = bond_out && mom_bonds(flags);
        if (!site_out && !bonds) return ISINGMC_OK;
        TRY(read_back(s, h, s->mom.d_site.get(), (mom_bonds(flags) ? 3 : 1) * 32 * sw));
        const auto total = [&](uint32_t kind, size_t site) {
            const uint32_t y = uint32_t(site / L.W), x = uint32_t(site - size_t(y) * L.W), i = x >> 1;
            const size_t w = size_t((x + y) & 1) * L.wpp + size_t(y) * L.wpr + (i >> 5);
            return int64_t(h[(size_t(kind) * 32 + (i & 31)) * sw + w]);
        };
        if (site_out)
            for (size_t i = 0; i < N; i++) site_out[i] = 2 * total(0, i) - nR;
        if (bonds) // entry e is the bond slot 2 site + direction: the right (kind 1) or the down (kind 2) bond of that site
            for (size_t e = 0; e < g->n_edges; e++) {
                const size_t slot = g->edge_slots.empty() ? e : g->edge_slots[e];
                bond_out[e] = 2 * total(1 + uint32_t(slot & 1), slot >> 1) - nR;
            }
        return ISINGMC_OK;
    }
    if (site_out) {
        TRY(read_back(s, h, s->mom.d_site.get(), size_t(g->pk.n_pos)));
        for (size_t i = 0; i < N; i++) site_out[i] = 2 * int64_t(h[g->pos[i]]) - nR;
    }
    if (bond_out && g->n_edges) {
        TRY(read_back(s, h, s->mom.d_bond.get(), size_t(g->n_edges)));
        for (size_t e = 0; e < g->n_edges; e++) bond_out[e] = 2 * int64_t(h[e]) - nR;
    }
    return ISINGMC_OK;
}
