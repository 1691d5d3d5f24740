// libisingmc.so: host side of the overlap measurement (isingmc_overlaps) -- which containers and pairings it
// serves, the accumulators and slot tables of one call, the batches of the arbitrary-pair form on replica-packed containers.
// Nothing here is a kernel: they are in overlap_kernels.hip, whose header states what is counted.
#include "internal.hpp"

// why these containers cannot be measured against each other ("" when they can; a == b: pairs inside one container)
static std::string overlaps_obstacle(const isingmc_states *a, const isingmc_states *b)
{
    if (a->g != b->g) return "the two containers belong to different graph handles: both must be replicas of one isingmc_graph";
    const isingmc_graph *g = a->g; // (one graph handle: one device)
    if (a->packed != b->packed || (a->packed && a->rj != b->rj))
        return "the two containers run on different kernel families: overlaps between containers need both on the same family";
    if (a->packed) return ""; // any graph of either packed family: no coupling and no bias is read
    if (g->kind != ISINGMC_KIND_LATTICE2D)
        return "overlaps need containers on the checkerboard lattice path or on a replica-packed family; this graph runs on the f64 CSR "
               "general-graph kernel family (the replica-packed family is chosen by size, or by ISINGMC_FORCE_PACKED=1 / the stable-path flag "
               "at creation)";
    return lattice_obstacle(g, "overlaps", true, false);
}

extern "C" int isingmc_overlaps(isingmc_states *a, isingmc_states *b, const uint32_t *slots_a, const uint32_t *slots_b, size_t n_pairs,
                                int64_t *spin_out, int64_t *link_out)
{
    if (!a) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (!spin_out) return fail(ISINGMC_ERR_INVALID, "NULL argument: spin_out (link_out alone may be NULL)");
    if (!b) b = a;
    {
        const std::string why = overlaps_obstacle(a, b);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    if ((slots_a == nullptr) != (slots_b == nullptr)) return fail(ISINGMC_ERR_INVALID, "give both slot tables or neither");
    if (n_pairs == 0) return fail(ISINGMC_ERR_INVALID, "n_pairs is 0: nothing to measure");
    const bool default_pairs = !slots_a && a == b; // (2 p, 2 p + 1) of the GLOBAL experiment index, as the isoenergetic moves pair them
    std::vector<uint32_t> identity;
    if (default_pairs) {
        if (a->first % 2) return fail(ISINGMC_ERR_INVALID, "this shard starts at an odd experiment index: its first replica's partner lives on another shard");
        if (n_pairs != a->R / 2) return fail(ISINGMC_ERR_INVALID, "without slot tables n_pairs must be count / 2 (pair p = replicas (2 p, 2 p + 1))");
    } else if (!slots_a) { // two containers: pair p = (slot p of a, slot p of b)
        if (n_pairs > a->R || n_pairs > b->R) return fail(ISINGMC_ERR_INVALID, "without slot tables n_pairs must not exceed the smaller of the two counts");
        identity.resize(n_pairs);
        for (size_t p = 0; p < n_pairs; p++) identity[p] = uint32_t(p);
        slots_a = slots_b = identity.data();
    } else {
        if (n_pairs > 0xFFFFFFFFull - 32) return fail(ISINGMC_ERR_INVALID, "more than 2^32 - 33 pairs in one call");
        for (size_t p = 0; p < n_pairs; p++)
            if (slots_a[p] >= a->R || slots_b[p] >= b->R) return fail(ISINGMC_ERR_INVALID, "slot out of range: every table entry must be below its container's count");
    }
    const isingmc_graph *g = a->g;
    const bool link = link_out != nullptr;
    TRY(use_device(g->device));
    for (isingmc_states *s : {a, b})
        if (s->n_lanes > 1) TRY(lanes_join(s));
    // accumulators {D, B} per pair; the packed kernels write whole groups (16 pairs) or pair blocks (32 pairs)
    const size_t n_pos = g->pk.n_pos, blocks = (n_pairs + 31) / 32;
    const size_t acc_pairs = !a->packed ? n_pairs : default_pairs ? 16 * a->groups : 32 * blocks;
    const size_t acc0 = a->packed && default_pairs ? a->pk_bit0 / 2 : 0; // (device slot 16 group + pair; pk_bit0 is even)
    DeviceScratch scratch(a->stream);
    unsigned long long *d_acc = nullptr;
    TRY(scratch.alloc(&d_acc, 2 * acc_pairs));
    HIP_TRY(hipMemsetAsync(d_acc, 0, 2 * acc_pairs * sizeof(unsigned long long), a->stream));
    uint32_t *d_sa = nullptr, *d_sb = nullptr;
    if (!default_pairs) { // (the host tables live as long as the call, which waits for the device before it returns)
        TRY(scratch.alloc(&d_sa, 2 * n_pairs));
        d_sb = d_sa + n_pairs;
        HIP_TRY(hipMemcpyAsync(d_sa, slots_a, n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, a->stream));
        HIP_TRY(hipMemcpyAsync(d_sb, slots_b, n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, a->stream));
    }
    if (a != b) { // b's sweeps and exchange rounds so far, before a's stream reads b's configurations
        if (!a->icmb_ev[0]) HIP_TRY(pooled_event_create(&a->icmb_ev[0], true));
        HIP_TRY(hipEventRecord(a->icmb_ev[0], b->stream));
        HIP_TRY(hipStreamWaitEvent(a->stream, a->icmb_ev[0], 0));
    }
    const uint32_t *nbr_rj = a->rj ? g->rj.nbr : nullptr;
    const uint32_t rj_slots = a->rj ? g->rj.slots : 0;
    if (!a->packed) {
        HIP_TRY(overlap_launch_lattice(a->stream, a->d_state, b->d_state, d_sa, d_sb, g->geom, link, n_pairs, d_acc));
    } else if (default_pairs) {
        HIP_TRY(overlap_launch_packed_pairs(a->stream, a->d_state, g->pk, nbr_rj, rj_slots, link, a->groups, d_acc));
    } else { // pair blocks of 32 pairs, their overlap words batched under a's cluster_workspace_bytes
        const size_t batch = nonlocal_batch(blocks, n_pos, size_t(std::max(1, a->opt.cluster_workspace_bytes)));
        uint32_t *d_words = nullptr;
        TRY(scratch.alloc(&d_words, batch * n_pos));
        const OverlapSide A{a->d_state, d_sa, uint32_t(a->pk_bit0), uint32_t(a->R)}, B{b->d_state, d_sb, uint32_t(b->pk_bit0), uint32_t(b->R)};
        for (size_t b0 = 0; b0 < blocks; b0 += batch)
            HIP_TRY(overlap_launch_packed_tables(a->stream, A, B, g->pk, nbr_rj, rj_slots, link, uint32_t(b0), uint32_t(std::min(batch, blocks - b0)),
                                                 uint32_t(n_pairs), d_words, d_acc));
    }
    std::vector<unsigned long long> h;
    TRY(read_back(a, h, d_acc, 2 * acc_pairs)); // waits: b may go on as soon as the call returns
    for (size_t p = 0; p < n_pairs; p++) {
        spin_out[p] = int64_t(g->nvars) - 2 * int64_t(h[2 * (acc0 + p)]);
        if (link) link_out[p] = int64_t(g->n_edges) - 2 * int64_t(h[2 * (acc0 + p) + 1]);
    }
    return ISINGMC_OK;
}
