// libisingmc.so: host side of the non-local moves -- when a container may take them, their workspaces and statistics, and the
// batches in which their launches go out.  Nothing here is a kernel: every move runs in cluster_kernels.hip,
// packed_cluster_kernels.hip, packed_icm_kernels.hip or packed_between_kernels.hip, whose headers also state the layout of the
// workspace blocks handed to them.  (internal.hpp: how the host side is cut into translation units.)
#include "internal.hpp"

// items per batch of a labelling workspace of words_per_item words each, under the container's cluster_workspace_bytes
static size_t workspace_batch(const isingmc_states *s, size_t items, size_t words_per_item)
{
    return nonlocal_batch(items, words_per_item, size_t(std::max(1, s->opt.cluster_workspace_bytes)));
}

// The clauses every non-local move of a checkerboard lattice shares ("" when none applies); `what` begins the message.
// any_sign: the move reads no coupling (the isoenergetic moves), so +-J sign patterns are fine.  labels: it labels sites (the
// overlap measurement of overlaps.hip does not).
std::string lattice_obstacle(const isingmc_graph *g, const std::string &what, bool any_sign, bool labels)
{
    if (g->mc_mode == MC_FIELD || g->mc_mode == MC_FIELD_OPEN) return what + " are not implemented for lattices with a field";
    if (g->mc_mode == MC_OPEN) return what + " are not implemented for open boundaries (periodic lattices only)";
    if (g->mc_mode != MC_NONE) return what + " are not implemented for anisotropic couplings (|Jx| != |Jy|)";
    if (!any_sign && !g->uniform_sign) return what + " are not implemented for +-J sign patterns (one coupling sign only)";
    if (labels && g->nvars >= 0xFFFFFFFFull) return what + " label sites with 32 bits: W H must be below 2^32 - 1";
    return "";
}

// statistics of the isoenergetic moves on the device: [cap][2] clusters, largest cluster, then [cap] q = -1 sites.  Entries
// [slot0, slot0 + n) into the caller's arrays, waited for
static int read_pair_stats(isingmc_states *s, const uint32_t *d_stats, size_t cap, size_t slot0, size_t n, uint64_t *n_clusters_out,
                           uint64_t *largest_out, uint64_t *minus_sites_out)
{
    std::vector<uint32_t> h;
    TRY(read_back(s, h, d_stats, 3 * cap));
    for (size_t p = 0; p < n; p++) {
        n_clusters_out[p] = h[2 * (slot0 + p)];
        largest_out[p] = h[2 * (slot0 + p) + 1];
        minus_sites_out[p] = h[2 * cap + slot0 + p];
    }
    return ISINGMC_OK;
}

// ------------------------------------------------------------------------------------------------
// Swendsen-Wang cluster steps (cluster_kernels.hip; S11 on replica-packed containers, packed_cluster_kernels.hip)
// ------------------------------------------------------------------------------------------------

// why this container cannot take cluster steps ("" when it can)
std::string cluster_obstacle(const isingmc_states *s)
{
    const isingmc_graph *g = s->g;
    if (s->packed) { // S11: any graph of the bit-sliced packed path, any sign pattern
        if (s->rj) return "cluster updates are not implemented for the replica-packed real-coupling path (couplings of one size and no biases only)";
    } else {
        if (g->kind != ISINGMC_KIND_LATTICE2D)
            return "cluster updates need a container on the checkerboard lattice path or on the replica-packed bit-sliced path; this graph runs on "
                   "the f64 CSR general-graph kernel family (cluster updates on general graphs need the replica-packed family: chosen by size, "
                   "or by ISINGMC_FORCE_PACKED=1 / the stable-path flag at creation)";
        const std::string why = lattice_obstacle(g, "cluster updates", false);
        if (!why.empty()) return why;
    }
    if (s->tempering.attached) return "a tempering ladder is attached to this container (isingmc_pt_detach first)";
    return "";
}

extern "C" int isingmc_states_set_cluster_every(isingmc_states *s, size_t k)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (k) {
        const std::string why = cluster_obstacle(s);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
        if (s->icm.every) return fail(ISINGMC_ERR_INVALID, "isoenergetic cluster moves are switched on for this container (isingmc_states_set_icm_every): one non-local move at a time");
    }
    s->cl.every = k;
    return ISINGMC_OK;
}

extern "C" int isingmc_states_cluster_every(const isingmc_states *s, size_t *k_out)
{
    if (!s || !k_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    *k_out = s->cl.every;
    return ISINGMC_OK;
}

extern "C" int isingmc_cluster_stats(isingmc_states *s, uint64_t *n_clusters_out, uint64_t *largest_out)
{
    if (!s || !n_clusters_out || !largest_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    if (!s->cl.have_stats || s->cl.stats_cap < counter_slots(s)) return fail(ISINGMC_ERR_INVALID, "no cluster step has run on these replicas yet");
    TRY(use_device(s->g->device));
    std::vector<uint32_t> h;
    TRY(read_back(s, h, s->cl.d_stats.get(), 2 * counter_slots(s)));
    for (size_t r = 0; r < s->R; r++) { // (packed: one pair per (group, bit) slot)
        n_clusters_out[r] = h[2 * counter_slot(s, r)];
        largest_out[r] = h[2 * counter_slot(s, r) + 1];
    }
    return ISINGMC_OK;
}

// T = floor((1 - exp(-2 beta |J|)) 2^32) in f64 (expm1 of glibc, as the tests' restatement); 2^32 = always, 0 = never
static uint64_t cluster_threshold(double beta, double jabs)
{
    if (!(beta > 0.0)) return 0;
    return uint64_t(std::floor(std::ldexp(-std::expm1(-2.0 * beta * jabs), 32)));
}

bool is_cluster_step(const isingmc_states *s) { return s->cl.every && s->t % s->cl.every == s->cl.every - 1; }

// Timestep s->t as a cluster step of every replica, batch by batch on the main stream.  A lattice container works in batches of
// replicas; a replica-packed bit-sliced one in batches of whole replica groups, every bit of a group simulated,
// owned or not, as by the sweeps.  Statistics and thresholds go by counter slot: the replica, or the (group, bit).
int run_cluster_step(isingmc_states *s, NonlocalRun &n, DeviceScratch &scratch, double beta)
{
    const isingmc_graph *g = s->g;
    const size_t items = s->packed ? s->groups : s->R, slots = counter_slots(s), n_pos = g->pk.n_pos;
    if (s->n_lanes > 1) TRY(lanes_join(s)); // the Metropolis stretch before this step may have run on replica lanes
    if (!n.batch) {
        const size_t words = s->packed ? pk_cluster_words_per_group(n_pos) : cluster_words_per_replica(g->nvars);
        const size_t batch = workspace_batch(s, items, words);
        uint32_t *block = nullptr;
        TRY(scratch.alloc(&block, batch * words));
        if (s->packed) n.pk_cl = pk_cluster_carve(block, batch, n_pos);
        else n.cl = cluster_carve(block, batch, g->nvars);
        n.batch = batch;
    }
    if (s->cl.stats_cap < slots) { // a lattice container may grow; the groups of a packed one are fixed for its life: allocated once
        const size_t cap = s->packed ? slots : s->cap;
        TRY(dev_regrow(s->stream, s->cl.d_stats, &s->cl.stats_cap, 2 * cap, cap));
    }
    uint64_t thr = 0;
    if (!s->has_betas) thr = cluster_threshold(beta, g->jabs);
    else if (!n.d_cl_thr) { // per-replica betas do not change inside a call; bits a packed shard does not own take the nearest owned replica's
        n.h_cl_thr.resize(slots);
        for (size_t sl = 0; sl < slots; sl++)
            n.h_cl_thr[sl] = cluster_threshold(s->betas[sl < s->pk_bit0 ? 0 : std::min(s->R - 1, sl - s->pk_bit0)], g->jabs);
        TRY(scratch.alloc(&n.d_cl_thr, slots));
        HIP_TRY(hipMemcpyAsync(n.d_cl_thr, n.h_cl_thr.data(), slots * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream));
    }
    HIP_TRY(hipMemsetAsync(s->cl.d_stats, 0, 2 * slots * sizeof(uint32_t), s->stream));
    ClusterMomentsOut row; // a live cluster series: every batch adds its columns' moments into the same row
    TRY(cluster_series_begin(s, ISINGMC_CLUSTER_SERIES_SW, &row));
    for (size_t i0 = 0; i0 < items; i0 += n.batch) {
        const uint32_t ni = uint32_t(std::min(n.batch, items - i0));
        row.slot0 = uint32_t(s->packed ? 32 * i0 : i0);
        if (s->packed)
            HIP_TRY(pk_cluster_launch_step(s->stream, s->d_state + i0 * n_pos, g->pk, s->t, s->d_keys + i0, thr, n.d_cl_thr ? n.d_cl_thr + 32 * i0 : nullptr,
                                           n.pk_cl, ni, s->cl.d_stats + 2 * 32 * i0, row));
        else
            HIP_TRY(cluster_launch_step(s->stream, s->d_state + i0 * g->state_words, g->geom, s->t, s->d_keys + i0, g->jneg_uniform, thr,
                                        n.d_cl_thr ? n.d_cl_thr + i0 : nullptr, n.cl, ni, s->cl.d_stats + 2 * i0, row));
    }
    if (row.row) TRY(cluster_series_end(s, row, s->cl.d_stats, nullptr));
    s->cl.have_stats = true;
    s->t++;
    return ISINGMC_OK;
}

// ------------------------------------------------------------------------------------------------
// Isoenergetic cluster moves between replica pairs (cluster_kernels.hip; S12 on replica-packed containers of both
// families, packed_icm_kernels.hip)
// ------------------------------------------------------------------------------------------------

// the isoenergetic cluster move is valid between replicas at one temperature only
bool icm_unequal_pair_betas(const isingmc_states *s, const double *betas)
{
    for (size_t r = 0; r + 1 < s->R; r += 2)
        if (betas[r] != betas[r + 1]) return true;
    return false;
}

// why this container cannot take isoenergetic cluster moves ("" when it can)
std::string icm_obstacle(const isingmc_states *s)
{
    const isingmc_graph *g = s->g;
    if (s->packed) { // S12: any graph of either packed family (the move reads no coupling and no bias)
        if (s->cl.every)
            return "Swendsen-Wang cluster updates are switched on for this replica-packed general-graph container (isingmc_states_set_cluster_every): "
                   "one non-local move at a time";
    } else {
        if (g->kind != ISINGMC_KIND_LATTICE2D)
            return "isoenergetic cluster moves need a container on the checkerboard lattice path; this graph runs on a general-graph kernel family";
        const std::string why = lattice_obstacle(g, "isoenergetic cluster moves", true);
        if (!why.empty()) return why;
    }
    if (s->tempering.attached) return "a tempering ladder is attached to this container (isingmc_pt_detach first)";
    if (s->cl.every) return "Swendsen-Wang cluster updates are switched on for this container (isingmc_states_set_cluster_every): one non-local move at a time";
    // pairs are (2 p, 2 p + 1) of the GLOBAL experiment index: a shard must hold both replicas of every pair it touches
    // (packed: the pair is then bits (2 j, 2 j + 1) of one state word, pk_bit0 = first % 32 being even)
    if (s->first % 2) return "this shard starts at an odd experiment index: its first replica's partner lives on another shard";
    if ((s->first + s->R) % 2 && s->first + s->R < s->n_total) return "this shard ends inside a pair: its last replica's partner lives on another shard";
    if (s->has_betas && icm_unequal_pair_betas(s, s->betas.data()))
        return "per-replica betas differ inside a pair: the two replicas of every pair (2 p, 2 p + 1) need equal betas";
    return "";
}

extern "C" int isingmc_states_set_icm_every(isingmc_states *s, size_t k)
{
    if (!s) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (k) {
        const std::string why = icm_obstacle(s);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    s->icm.every = k;
    return ISINGMC_OK;
}

extern "C" int isingmc_states_icm_every(const isingmc_states *s, size_t *k_out)
{
    if (!s || !k_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    *k_out = s->icm.every;
    return ISINGMC_OK;
}

extern "C" int isingmc_icm_stats(isingmc_states *s, uint64_t *n_clusters_out, uint64_t *largest_out, uint64_t *minus_sites_out)
{
    if (!s || !n_clusters_out || !largest_out || !minus_sites_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    const size_t pairs = s->R / 2, slot0 = s->packed ? s->pk_bit0 / 2 : 0; // (packed: device slot 16 group + pair; pk_bit0 is even)
    if (!s->icm.have_stats || s->icm.stats_cap < slot0 + pairs) return fail(ISINGMC_ERR_INVALID, "no isoenergetic cluster move has run on these replicas yet");
    TRY(use_device(s->g->device));
    return read_pair_stats(s, s->icm.d_stats, s->icm.stats_cap, slot0, pairs, n_clusters_out, largest_out, minus_sites_out);
}

bool is_icm_step(const isingmc_states *s) { return s->icm.every && s->t % s->icm.every == s->icm.every - 1; }

// Timestep s->t as an isoenergetic cluster move of every pair, batch by batch on the main stream.  A lattice container works in
// batches of pairs (one labelling problem per PAIR; a last replica without a partner stays as it is).  A replica-packed one of
// either family works in batches of whole replica groups, 16 pairs each: pair j of GLOBAL group G moves when both
// its experiments exist (32 G + 2 j + 1 < n_total), owned by this shard or not.
int run_icm_step(isingmc_states *s, NonlocalRun &n, DeviceScratch &scratch)
{
    const isingmc_graph *g = s->g;
    const size_t groups = s->groups, pairs = s->R / 2, n_pos = g->pk.n_pos;
    const size_t items = s->packed ? groups : pairs, pair_slots = s->packed ? 16 * groups : pairs;
    if (s->n_lanes > 1) TRY(lanes_join(s)); // the Metropolis stretch before this step may have run on replica lanes
    if (items && !n.batch) {
        const size_t words = s->packed ? pk_icm_words_per_group(n_pos) : cluster_words_per_replica(g->nvars);
        const size_t batch = workspace_batch(s, items, words);
        uint32_t *block = nullptr;
        TRY(scratch.alloc(&block, batch * words));
        if (s->packed) n.pk_icm = pk_icm_carve(block, batch, n_pos);
        else n.cl = cluster_carve(block, batch, g->nvars);
        n.batch = batch;
    }
    if (s->packed && !n.d_icm_mask) {
        n.h_icm_mask.resize(groups);
        const size_t G0 = s->first / 32;
        for (size_t gi = 0; gi < groups; gi++) {
            uint32_t m = 0;
            for (size_t j = 0; j < 16; j++)
                if (32 * (G0 + gi) + 2 * j + 1 < s->n_total) m |= 1u << (2 * j);
            n.h_icm_mask[gi] = m;
        }
        TRY(scratch.alloc(&n.d_icm_mask, groups));
        HIP_TRY(hipMemcpyAsync(n.d_icm_mask, n.h_icm_mask.data(), groups * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream)); // (h_icm_mask lives as long as the call)
    }
    // (a lattice container of one replica has no pair and still gets its block; a packed one has 16 slots per group from the start,
    //  and its groups are fixed for its life: allocated once)
    if (!s->icm.d_stats || s->icm.stats_cap < pair_slots) {
        const size_t cap = s->packed ? pair_slots : std::max<size_t>(1, s->cap / 2);
        TRY(dev_regrow(s->stream, s->icm.d_stats, &s->icm.stats_cap, 3 * cap, cap));
    }
    uint32_t *const minus = s->icm.d_stats + 2 * s->icm.stats_cap;
    HIP_TRY(hipMemsetAsync(s->icm.d_stats, 0, 3 * s->icm.stats_cap * sizeof(uint32_t), s->stream));
    ClusterMomentsOut row; // a live cluster series: every batch adds its pairs' moments into the same row
    TRY(cluster_series_begin(s, ISINGMC_CLUSTER_SERIES_ICM, &row));
    for (size_t i0 = 0; i0 < items; i0 += n.batch) {
        const uint32_t ni = uint32_t(std::min(n.batch, items - i0));
        row.slot0 = uint32_t(s->packed ? 16 * i0 : i0);
        if (s->packed)
            HIP_TRY(pk_icm_launch_step(s->stream, s->d_state + i0 * n_pos, g->pk, s->rj ? g->rj.nbr : nullptr, s->rj ? g->rj.slots : 0, s->t, s->d_keys + i0,
                                       n.d_icm_mask + i0, n.pk_icm, ni, s->icm.d_stats + 2 * 16 * i0, minus + 16 * i0, row));
        else
            HIP_TRY(icm_launch_step(s->stream, s->d_state + 2 * i0 * g->state_words, g->geom, s->t, s->d_keys + 2 * i0, n.cl, ni, s->icm.d_stats + 2 * i0,
                                    minus + i0, row));
    }
    if (row.row) TRY(cluster_series_end(s, row, s->icm.d_stats, minus));
    s->icm.have_stats = true;
    s->t++;
    return ISINGMC_OK;
}

// ------------------------------------------------------------------------------------------------
// Isoenergetic cluster moves between two containers (cluster_kernels.hip): the move of S9 with pair p =
// (slot slots_a[p] of a, slot slots_b[p] of b) -- what two tempering ladders over the same betas need, whose rung permutations
// live on the device.  Two replica-packed containers of one family take the same call in the form of DESIGN.md S13
// (packed_between_kernels.hip)
// ------------------------------------------------------------------------------------------------

// why these two containers cannot take a move between them ("" when they can): icm_obstacle without its ladder and shard clauses
static std::string icm_between_obstacle(const isingmc_states *a, const isingmc_states *b)
{
    if (a == b) return "an isoenergetic cluster move between two containers needs two different containers";
    if (a->g != b->g) return "the two containers belong to different graph handles: both must be replicas of one isingmc_graph";
    const isingmc_graph *g = a->g; // (one graph handle: one device)
    if (a->packed && b->packed) { // S13: any graph of either packed family, both containers on the same one
        if (a->rj != b->rj)
            return "the two containers run on different kernel families (one on the replica-packed bit-sliced family, the other on the "
                   "replica-packed real-coupling family): a move between containers needs both on the same family";
    } else {
        if (g->kind != ISINGMC_KIND_LATTICE2D || a->packed || b->packed)
            return "isoenergetic cluster moves need containers on the checkerboard lattice path; this graph runs on a general-graph kernel family";
        const std::string why = lattice_obstacle(g, "isoenergetic cluster moves", true);
        if (!why.empty()) return why;
    }
    for (const isingmc_states *s : {a, b}) {
        if (s->cl.every) return "Swendsen-Wang cluster updates are switched on for one of the containers (isingmc_states_set_cluster_every): one non-local move at a time";
        if (s->icm.every) return "isoenergetic cluster moves inside one of the containers are switched on (isingmc_states_set_icm_every): one non-local move at a time";
    }
    if (a->t != b->t) return "the two containers stand at unequal timesteps: the move is timestep t of both";
    return "";
}

// Before the launches of a move of n_pairs pairs: slot tables, statistics and events of `a` (they stay with it: nothing here waits
// for the device unless a table grows), the caller's slot tables on the device, a's stream behind b's, the statistics cleared.
// *d_sa, *d_sb: the device tables of the move -- the upload, or the two ladders' permutations when slots_a == nullptr.
static int between_prepare(isingmc_states *a, isingmc_states *b, const uint32_t *slots_a, const uint32_t *slots_b, size_t n_pairs,
                           const uint32_t **d_sa, const uint32_t **d_sb)
{
    if (a->icmb.cap < n_pairs) {
        HIP_TRY(stream_quiesce(a->stream));
        a->icmb.d_slots.reset();
        a->icmb.d_stats.reset();
        a->icmb.cap = 0;
        a->icmb.have_stats = false;
        const size_t cap = std::max(n_pairs, a->cap);
        TRY(dev_alloc(a->icmb.d_slots, 2 * cap));
        TRY(dev_alloc(a->icmb.d_stats, 3 * cap));
        a->icmb.cap = cap;
    }
    for (PooledEvent &ev : a->icmb.ev)
        if (!ev) TRY(event_create(ev));
    *d_sa = a->tempering.d_perm;
    *d_sb = b->tempering.d_perm;
    if (slots_a) {
        HIP_TRY(hipMemcpyAsync(a->icmb.d_slots, slots_a, n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, a->stream));
        HIP_TRY(hipMemcpyAsync(a->icmb.d_slots + a->icmb.cap, slots_b, n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, a->stream));
        *d_sa = a->icmb.d_slots;
        *d_sb = a->icmb.d_slots + a->icmb.cap;
    }
    TRY(stream_wait_for(a->stream, b->stream, a->icmb.ev[0])); // b's sweeps and exchange rounds so far, before a's stream touches b's configurations and permutation
    HIP_TRY(hipMemsetAsync(a->icmb.d_stats, 0, 3 * a->icmb.cap * sizeof(uint32_t), a->stream));
    return ISINGMC_OK;
}

// Sums per rung: the move has been a timestep of both containers, and whichever of them has its period fall on it
// takes its sample, each on its own stream (b's waits for the move).  The other modes of S18 take no sample here, as before.
static int between_sample(isingmc_states *a, isingmc_states *b)
{
    for (isingmc_states *s : {a, b})
        if (s->mom.flags & ISINGMC_MOMENTS_PER_RUNG) TRY(recorder_sample_now(s, REC_MOMENTS)); // (no repeat is under way here: replay_to is 0)
    // ... and a periodic observable series by rung (S22) takes its row, by the same rule
    for (isingmc_states *s : {a, b})
        if (obs_sample_by_rung(s)) TRY(recorder_sample_now(s, REC_OBSERVABLES));
    return ISINGMC_OK;
}

// behind the launches: b goes on with the new configurations, and the move has been timestep t of both containers
static int between_finish(isingmc_states *a, isingmc_states *b, size_t n_pairs)
{
    TRY(stream_wait_for(b->stream, a->stream, a->icmb.ev[1]));
    a->icmb.pairs = n_pairs;
    a->icmb.have_stats = true;
    for (isingmc_states *s : {a, b}) {
        s->t++;
        s->meas_fresh = false; // cached ladder energies (and those a strip launch left behind) belong to the configurations before the move
    }
    return between_sample(a, b);
}

extern "C" int isingmc_icm_between(isingmc_states *a, isingmc_states *b, const uint32_t *slots_a, const uint32_t *slots_b, size_t n_pairs)
{
    if (!a || !b) return fail(ISINGMC_ERR_INVALID, "NULL states");
    {
        const std::string why = icm_between_obstacle(a, b);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    if ((slots_a == nullptr) != (slots_b == nullptr)) return fail(ISINGMC_ERR_INVALID, "give both slot tables or neither");
    const isingmc_graph *g = a->g;
    if (!slots_a) { // pair r = (a's rung r, b's rung r): the permutations are read on the device
        if (!a->tempering.attached || !b->tempering.attached) return fail(ISINGMC_ERR_INVALID, "without slot tables both containers need an attached tempering ladder (isingmc_pt_attach)");
        for (const isingmc_states *s : {a, b})
            if (s->tempering.world != 1 || s->pt.slot_offset != 0 || s->pt.n_rungs != s->R)
                return fail(ISINGMC_ERR_INVALID, "without slot tables each ladder must live on its container alone (world size 1, one slot per rung): sharded ladders are not served");
        if (a->pt.n_rungs != b->pt.n_rungs) return fail(ISINGMC_ERR_INVALID, "the two ladders differ in their number of rungs");
        if (a->tempering.ladder_betas.size() != b->tempering.ladder_betas.size() ||
            std::memcmp(a->tempering.ladder_betas.data(), b->tempering.ladder_betas.data(), a->tempering.ladder_betas.size() * sizeof(double)) != 0)
            return fail(ISINGMC_ERR_INVALID, "the two ladders differ in their betas: the replicas of a pair need equal betas");
        if (n_pairs != a->R) return fail(ISINGMC_ERR_INVALID, "without slot tables n_pairs must be the number of rungs");
    } else {
        if (n_pairs > a->R || n_pairs > b->R) return fail(ISINGMC_ERR_INVALID, "more pairs than replicas");
        std::vector<uint8_t> seen_a(a->R, 0), seen_b(b->R, 0);
        for (size_t p = 0; p < n_pairs; p++) {
            if (slots_a[p] >= a->R || slots_b[p] >= b->R) return fail(ISINGMC_ERR_INVALID, "slot out of range");
            if (seen_a[slots_a[p]]++ || seen_b[slots_b[p]]++) return fail(ISINGMC_ERR_INVALID, "a duplicate slot: every replica belongs to at most one pair");
        }
        // per-replica betas set by the host are known here; a ladder relabels them on the device (the caller pairs equal rungs)
        if (a->has_betas != b->has_betas && !a->tempering.attached && !b->tempering.attached)
            return fail(ISINGMC_ERR_INVALID, "per-replica betas are set on one container only: the replicas of a pair need equal betas");
        if (a->has_betas && b->has_betas && !a->tempering.attached && !b->tempering.attached)
            for (size_t p = 0; p < n_pairs; p++)
                if (std::memcmp(&a->betas[slots_a[p]], &b->betas[slots_b[p]], sizeof(double)) != 0)
                    return fail(ISINGMC_ERR_INVALID, "per-replica betas differ inside a pair: the two replicas of every pair need equal betas");
    }
    // a periodic observable series by rung whose log has no room for the row behind this move: nothing is enqueued
    for (const isingmc_states *s : {a, b})
        if (obs_sample_by_rung(s)) TRY(series_room_or_fail(s, REC_OBSERVABLES, 1));
    TRY(use_device(g->device));
    if (n_pairs == 0) { // time passes all the same
        a->t++;
        b->t++;
        return between_sample(a, b);
    }
    for (isingmc_states *s : {a, b})
        if (s->n_lanes > 1) TRY(lanes_join(s));
    // The labelling workspace stays with `a` too, under a's cluster_workspace_bytes: of a batch of pairs on lattices, of whole pair
    // blocks (32 pairs each) on packed containers.  It follows the batch: another block whenever the batch DIFFERS.
    const size_t n_pos = g->pk.n_pos, items = a->packed ? (n_pairs + 31) / 32 : n_pairs;
    const size_t words = a->packed ? pk_between_words_per_block(n_pos) : cluster_words_per_replica(g->nvars);
    const size_t batch = workspace_batch(a, items, words);
    if (!a->icmb.d_work || a->icmb.batch != batch) TRY(dev_regrow(a->stream, a->icmb.d_work, &a->icmb.batch, batch * words, batch));
    const size_t inv_words = 32 * (a->groups + b->groups); // packed: (local group, bit) -> pair, a's groups first
    if (a->packed && a->icmb.inv_cap < inv_words) TRY(dev_regrow(a->stream, a->icmb.d_inv, &a->icmb.inv_cap, inv_words, inv_words));
    const uint32_t *d_sa = nullptr, *d_sb = nullptr;
    TRY(between_prepare(a, b, slots_a, slots_b, n_pairs, &d_sa, &d_sb));
    uint32_t *const stats = a->icmb.d_stats, *const minus = a->icmb.d_stats + 2 * a->icmb.cap;
    if (a->packed) {
        const PkBetweenWork work = pk_between_carve(a->icmb.d_work, batch, n_pos);
        const PkBetweenSide A{{a->d_state, d_sa, uint32_t(a->pk_bit0), uint32_t(a->R)}, a->icmb.d_inv, uint32_t(a->groups)};
        const PkBetweenSide B{{b->d_state, d_sb, uint32_t(b->pk_bit0), uint32_t(b->R)}, a->icmb.d_inv + 32 * a->groups, uint32_t(b->groups)};
        HIP_TRY(pk_between_launch_tables(a->stream, A, B, uint32_t(n_pairs)));
        for (size_t b0 = 0; b0 < items; b0 += batch)
            HIP_TRY(pk_between_launch_batch(a->stream, A, B, g->pk, a->rj ? g->rj.nbr : nullptr, a->rj ? g->rj.slots : 0, a->t, a->d_keys, work, uint32_t(b0),
                                            uint32_t(std::min(batch, items - b0)), uint32_t(n_pairs), stats, minus));
    } else {
        const ClusterWork cl = cluster_carve(a->icmb.d_work, batch, g->nvars);
        for (size_t p0 = 0; p0 < items; p0 += batch)
            HIP_TRY(icm_between_launch_step(a->stream, a->d_state, b->d_state, d_sa + p0, d_sb + p0, g->geom, a->t, a->d_keys, cl,
                                            uint32_t(std::min(batch, items - p0)), stats + 2 * p0, minus + p0));
    }
    return between_finish(a, b, n_pairs);
}

extern "C" int isingmc_icm_between_stats(isingmc_states *a, uint64_t *n_clusters_out, uint64_t *largest_out, uint64_t *minus_sites_out, size_t n_pairs)
{
    if (!a || !n_clusters_out || !largest_out || !minus_sites_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    if (!a->icmb.have_stats) return fail(ISINGMC_ERR_INVALID, "no isoenergetic cluster move between containers has been called on this container yet");
    if (n_pairs != a->icmb.pairs) return fail(ISINGMC_ERR_INVALID, "n_pairs differs from the number of pairs of the last move");
    TRY(use_device(a->g->device));
    return read_pair_stats(a, a->icmb.d_stats, a->icmb.cap, 0, n_pairs, n_clusters_out, largest_out, minus_sites_out);
}
