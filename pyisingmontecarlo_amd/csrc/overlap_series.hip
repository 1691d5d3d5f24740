// libisingmc.so: host side of the overlap series (isingmc_overlap_series_*) -- a device-resident log with one row of
// overlaps per sample.  A record runs the two passes of the overlap core (overlaps.hip), as isingmc_overlaps and
// isingmc_overlaps_by_class do, in a workspace the series owns, and behind each batch the store kernel of
// overlap_series_kernels.hip, which writes the row entries; nothing comes back to the host before isingmc_overlap_series_get.
// Nothing here is a kernel.
#include "internal.hpp"

struct isingmc_overlap_series : SeriesLog { // rows of [n_pairs][entries], read as long long
    isingmc_states *b = nullptr; // b == a: pairs inside one container
    explicit isingmc_overlap_series(isingmc_states *a_) : SeriesLog(a_, REC_OVERLAPS, "overlap") {}
    const isingmc_site_classes *classes = nullptr;
    unsigned flags = 0;
    size_t n_pairs = 0;
    size_t bins = 0, entries = 0; // n_tables * n_classes; entries of one pair: 1 + link + bins
    DevBlock<unsigned long long> d_sizes;  // {nvars, n_edges, sizes[n_tables][n_classes]}: what the store kernel subtracts from
    DevBlock<uint32_t> d_slots;            // [2][n_pairs] the slot tables of the record being enqueued
    // workspace of one record; it grows only behind stream_quiesce of a's stream
    DevBlock<unsigned long long> d_acc, d_cacc; // {D, B} per pair column; the class bins of one batch
    DevBlock<uint32_t> d_words;                 // packed containers with tables: the gathered overlap words of one batch
    size_t acc_cap = 0, cacc_cap = 0, words_cap = 0;
    std::vector<std::vector<uint32_t>> uploads; // host tables that an enqueued copy may still read
    PooledEvent ev[2];                          // b's stream has arrived / the record is enqueued
};

static bool osr_link(const isingmc_overlap_series *S) { return (S->flags & ISINGMC_SERIES_LINK) != 0; }
static bool osr_by_rung(const isingmc_overlap_series *S) { return (S->flags & ISINGMC_SERIES_BY_RUNG) != 0; }

// what the table-free form of isingmc_icm_between asks of two ladders ("" when they serve), in its words
static std::string osr_ladders_obstacle(const isingmc_states *a, const isingmc_states *b, size_t n_pairs)
{
    if (!b || a == b) return "ISINGMC_SERIES_BY_RUNG pairs the rungs of two ladders: it needs two different containers";
    if (!a->tempering.attached || !b->tempering.attached) return "without slot tables both containers need an attached tempering ladder (isingmc_pt_attach)";
    for (const isingmc_states *s : {a, b})
        if (s->tempering.world != 1 || s->pt.slot_offset != 0 || s->pt.n_rungs != s->R)
            return "without slot tables each ladder must live on its container alone (world size 1, one slot per rung): sharded ladders are not served";
    if (a->pt.n_rungs != b->pt.n_rungs) return "the two ladders differ in their number of rungs";
    if (a->tempering.ladder_betas.size() != b->tempering.ladder_betas.size() ||
        std::memcmp(a->tempering.ladder_betas.data(), b->tempering.ladder_betas.data(), a->tempering.ladder_betas.size() * sizeof(double)) != 0)
        return "the two ladders differ in their betas: the replicas of a pair need equal betas";
    if (n_pairs != a->R) return "without slot tables n_pairs must be the number of rungs";
    return "";
}

extern "C" int isingmc_overlap_series_create(isingmc_states *a, isingmc_states *b, size_t n_pairs, const isingmc_site_classes *classes,
                                             unsigned flags, size_t capacity, isingmc_overlap_series **out)
{
    if (!a || !out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    *out = nullptr;
    if (flags & ~unsigned(ISINGMC_SERIES_LINK | ISINGMC_SERIES_BY_RUNG))
        return fail(ISINGMC_ERR_INVALID, "unknown flag: ISINGMC_SERIES_LINK and ISINGMC_SERIES_BY_RUNG are the flags of an overlap series");
    {
        const std::string why = overlaps_obstacle(a, b ? b : a);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    const isingmc_graph *g = a->g;
    if (n_pairs == 0) return fail(ISINGMC_ERR_INVALID, "n_pairs is 0: nothing to measure");
    if (n_pairs > 0xFFFFFFFFull - 32) return fail(ISINGMC_ERR_INVALID, "more than 2^32 - 33 pairs in one call");
    if (capacity == 0) return fail(ISINGMC_ERR_INVALID, "capacity is 0: the log holds no row");
    if (flags & ISINGMC_SERIES_BY_RUNG) {
        const std::string why = osr_ladders_obstacle(a, b, n_pairs);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    if (classes) {
        const std::string why = classes_obstacle(classes, a);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    const size_t bins = classes ? classes->n_tables * classes->n_classes : 0;
    const size_t entries = 1 + ((flags & ISINGMC_SERIES_LINK) ? 1 : 0) + bins;
    TRY(series_budget_or_fail("overlap", a->opt.overlap_series_bytes, capacity, (unsigned long long)n_pairs * entries * sizeof(long long)));
    TRY(use_device(g->device));
    std::unique_ptr<isingmc_overlap_series> S(new isingmc_overlap_series(a));
    S->b = b ? b : a;
    S->classes = classes;
    S->flags = flags;
    S->n_pairs = n_pairs;
    S->capacity = capacity;
    S->row = n_pairs * entries;
    S->bins = bins;
    S->entries = entries;
    TRY(dev_alloc(S->d_log, capacity * S->row));
    TRY(dev_alloc(S->d_slots, 2 * n_pairs));
    std::vector<unsigned long long> sizes{(unsigned long long)g->nvars, (unsigned long long)g->n_edges};
    if (classes) sizes.insert(sizes.end(), classes->sizes.begin(), classes->sizes.end());
    TRY(dev_alloc(S->d_sizes, sizes.size()));
    HIP_TRY(hipMemcpy(S->d_sizes, sizes.data(), sizes.size() * sizeof(unsigned long long), hipMemcpyHostToDevice)); // once: waited for here
    for (PooledEvent &ev : S->ev) TRY(event_create(ev));
    if (osr_by_rung(S.get()))
        for (isingmc_states *s : {S->a, S->b}) s->osr_by_rung_live++;
    *out = S.release();
    return ISINGMC_OK;
}

extern "C" int isingmc_overlap_series_destroy(isingmc_overlap_series *S)
{
    if (!S) return ISINGMC_OK;
    series_unregister(S);
    if (osr_by_rung(S))
        for (isingmc_states *s : {S->a, S->b}) s->osr_by_rung_live--;
    delete S;
    return ISINGMC_OK;
}

template <typename T>
static int osr_ensure(isingmc_overlap_series *S, DevBlock<T> &block, size_t *cap, size_t need)
{
    if (need <= *cap) return ISINGMC_OK;
    return dev_regrow(S->a->stream, block, cap, need, need);
}

// One row for the configurations as they are: the measurement of the overlap core (overlaps.hip) in the workspace of the series,
// with the store kernel behind every batch of accumulators.  d_sa / d_sb: device slot tables, nullptr for the pairs (2 p, 2 p + 1)
// of one container.  Enqueue only, unless the workspace has to grow.
static int osr_enqueue(isingmc_overlap_series *S, const uint32_t *d_sa, const uint32_t *d_sb)
{
    isingmc_states *a = S->a, *b = S->b;
    const OverlapJob J{a, b, d_sa, d_sb, S->n_pairs, osr_link(S), S->classes};
    const OverlapPlan P = overlap_plan(a, S->n_pairs, J.default_pairs(), S->bins);
    TRY(osr_ensure(S, S->d_acc, &S->acc_cap, 2 * P.acc_pairs));
    TRY(osr_ensure(S, S->d_cacc, &S->cacc_cap, P.cbatch * P.cols * S->bins));
    TRY(osr_ensure(S, S->d_words, &S->words_cap, (P.batch ? std::max(P.batch, P.cbatch) : 0) * a->g->pk.n_pos));
    const OverlapWork W{S->d_acc, S->d_cacc, S->d_words};
    TRY(overlap_lanes_join(a, b));
    // b's sweeps and exchange rounds so far, before a's stream reads b's configurations and permutation
    if (a != b) TRY(stream_wait_for(a->stream, b->stream, S->ev[0]));
    long long *const row = reinterpret_cast<long long *>(S->next_row());
    const uint32_t entries = uint32_t(S->entries), n_spin = J.link ? 2 : 1, bins = uint32_t(S->bins);
    // spin and link overlap: entries 0 and 1 of every pair
    auto store = [&](const unsigned long long *acc, size_t c0, size_t n) -> int {
        HIP_TRY(osr_launch_store(a->stream, OsrStore{acc, S->d_sizes, row, c0, P.acc0, n, S->n_pairs, 2, n_spin, entries, 0}));
        return ISINGMC_OK;
    };
    TRY(overlap_enqueue(J, P, W, store));
    // by class: the entries behind them, batch by batch
    auto store_classes = [&](const unsigned long long *acc, size_t c0, size_t n) -> int {
        HIP_TRY(osr_launch_store(a->stream, OsrStore{acc, S->d_sizes + 2, row, c0, P.col0, n, S->n_pairs, bins, bins, entries, n_spin}));
        return ISINGMC_OK;
    };
    if (bins) TRY(overlap_class_enqueue(J, P, W, store_classes));
    if (a != b) TRY(stream_wait_for(b->stream, a->stream, S->ev[1])); // b's next sweeps must not run under a's reads
    S->timesteps.push_back(a->t);
    return ISINGMC_OK;
}

extern "C" int isingmc_overlap_series_record(isingmc_overlap_series *S, const uint32_t *slots_a, const uint32_t *slots_b)
{
    if (!S) return fail(ISINGMC_ERR_INVALID, "NULL series");
    isingmc_states *a = S->a, *b = S->b;
    const size_t n_pairs = S->n_pairs;
    const uint32_t *d_sa = nullptr, *d_sb = nullptr;
    OverlapPairing P;
    if (osr_by_rung(S)) {
        if (slots_a || slots_b) return fail(ISINGMC_ERR_INVALID, "a series made with ISINGMC_SERIES_BY_RUNG takes no slot tables: its pairs are the rungs of the two ladders");
        const std::string why = osr_ladders_obstacle(a, b, n_pairs); // (a ladder may have been detached and attached again since)
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
        d_sa = a->tempering.d_perm;
        d_sb = b->tempering.d_perm;
    } else {
        TRY(overlap_pairing(a, b, slots_a, slots_b, n_pairs, P));
    }
    TRY(series_full_or_ok(S));
    TRY(use_device(a->g->device));
    if (!osr_by_rung(S) && !P.default_pairs) {
        // the tables go into a block of the series; the host copy lives until a's stream has passed the upload
        if (!S->uploads.empty() && hipStreamQuery(a->stream) == hipSuccess) S->uploads.clear();
        S->uploads.emplace_back(2 * n_pairs);
        uint32_t *h = S->uploads.back().data();
        std::copy(P.slots_a, P.slots_a + n_pairs, h);
        std::copy(P.slots_b, P.slots_b + n_pairs, h + n_pairs);
        HIP_TRY(hipMemcpyAsync(S->d_slots, h, 2 * n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, a->stream));
        d_sa = S->d_slots;
        d_sb = S->d_slots + n_pairs;
    }
    return osr_enqueue(S, d_sa, d_sb);
}

extern "C" int isingmc_overlap_series_set_every(isingmc_overlap_series *S, size_t every)
{
    if (!S) return fail(ISINGMC_ERR_INVALID, "NULL series");
    isingmc_states *a = S->a;
    if (every == 0) return S->period_off(); // off: the rows stay
    if (S->b != a || osr_by_rung(S))
        return fail(ISINGMC_ERR_INVALID, "a period is for a series inside one container (b == NULL, no ISINGMC_SERIES_BY_RUNG): between two containers "
                                         "there is no common step loop; record explicitly, as with isingmc_icm_between");
    TRY(series_period_free_or_fail(S));
    OverlapPairing P;
    TRY(overlap_pairing(a, a, nullptr, nullptr, S->n_pairs, P)); // a periodic record takes no tables: the pairs (2 p, 2 p + 1)
    return S->period_on(every);
}

int osr_sample_enqueue(isingmc_states *s)
{
    isingmc_overlap_series *S = static_cast<isingmc_overlap_series *>(s->series[REC_OVERLAPS]);
    TRY(series_full_or_ok(S));
    return osr_enqueue(S, nullptr, nullptr);
}

extern "C" int isingmc_overlap_series_count(const isingmc_overlap_series *S, size_t *n, size_t *capacity) { return series_count(S, n, capacity); }

extern "C" int isingmc_overlap_series_get(isingmc_overlap_series *S, size_t first, size_t n, uint64_t *timesteps_out, int64_t *spin_out,
                                          int64_t *link_out, int64_t *class_out)
{
    if (!S) return fail(ISINGMC_ERR_INVALID, "NULL series");
    const char *why = link_out && !osr_link(S) ? "no link overlaps are held: make the series with ISINGMC_SERIES_LINK (link_out may be NULL)"
                      : class_out && !S->bins ? "no overlaps by class are held: make the series with a class set (class_out may be NULL)" : nullptr;
    std::vector<unsigned long long> h;
    TRY(series_read(S, first, n, why, timesteps_out, spin_out || link_out || class_out, h));
    S->uploads.clear(); // (a's stream has drained)
    const size_t E = S->entries, bins = S->bins, off = osr_link(S) ? 2 : 1;
    for (size_t i = 0; i < h.size() / E; i++) { // (row, pair)
        const long long *e = reinterpret_cast<const long long *>(h.data()) + i * E;
        if (spin_out) spin_out[i] = e[0];
        if (link_out) link_out[i] = e[1];
        if (class_out) std::copy(e + off, e + off + bins, class_out + i * bins);
    }
    return ISINGMC_OK;
}

extern "C" int isingmc_overlap_series_reset(isingmc_overlap_series *S) { return series_reset(S); }
