// libisingmc.so: host side of the overlap measurement (isingmc_overlaps) -- which containers and pairings it
// serves, and the overlap core: the one plan of a measurement's batches and the two launch sequences that the synchronising
// calls here and the records of overlap_series.hip share.
// Nothing here is a kernel: they are in overlap_kernels.hip, whose header states what is counted.
#include "internal.hpp"

// why these containers cannot be measured against each other ("" when they can; a == b: pairs inside one container)
std::string overlaps_obstacle(const isingmc_states *a, const isingmc_states *b)
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

// the pairs of one call, validated (OverlapPairing, internal.hpp)
int overlap_pairing(isingmc_states *a, isingmc_states *b, const uint32_t *slots_a, const uint32_t *slots_b, size_t n_pairs, OverlapPairing &P)
{
    if (!b) b = a;
    {
        const std::string why = overlaps_obstacle(a, b);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    if ((slots_a == nullptr) != (slots_b == nullptr)) return fail(ISINGMC_ERR_INVALID, "give both slot tables or neither");
    if (n_pairs == 0) return fail(ISINGMC_ERR_INVALID, "n_pairs is 0: nothing to measure");
    P.default_pairs = !slots_a && a == b; // (2 p, 2 p + 1) of the GLOBAL experiment index, as the isoenergetic moves pair them
    if (P.default_pairs) {
        if (a->first % 2) return fail(ISINGMC_ERR_INVALID, "this shard starts at an odd experiment index: its first replica's partner lives on another shard");
        if (n_pairs != a->R / 2) return fail(ISINGMC_ERR_INVALID, "without slot tables n_pairs must be count / 2 (pair p = replicas (2 p, 2 p + 1))");
    } else if (!slots_a) { // two containers: pair p = (slot p of a, slot p of b)
        if (n_pairs > a->R || n_pairs > b->R) return fail(ISINGMC_ERR_INVALID, "without slot tables n_pairs must not exceed the smaller of the two counts");
        P.identity.resize(n_pairs);
        for (size_t p = 0; p < n_pairs; p++) P.identity[p] = uint32_t(p);
        slots_a = slots_b = P.identity.data();
    } else {
        if (n_pairs > 0xFFFFFFFFull - 32) return fail(ISINGMC_ERR_INVALID, "more than 2^32 - 33 pairs in one call");
        for (size_t p = 0; p < n_pairs; p++)
            if (slots_a[p] >= a->R || slots_b[p] >= b->R) return fail(ISINGMC_ERR_INVALID, "slot out of range: every table entry must be below its container's count");
    }
    P.b = b;
    P.slots_a = slots_a;
    P.slots_b = slots_b;
    return ISINGMC_OK;
}

int overlap_lanes_join(isingmc_states *a, isingmc_states *b)
{
    for (isingmc_states *s : {a, b})
        if (s->n_lanes > 1) TRY(lanes_join(s));
    return ISINGMC_OK;
}

std::string classes_obstacle(const isingmc_site_classes *classes, const isingmc_states *a)
{
    if (classes->g != a->g) return "the class set was made for another graph handle: its tables follow that graph's layout";
    if (a->packed ? !classes->has_pk : !classes->has_lat) return "the class set holds no layout for this container's kernel family";
    return "";
}

// ---- the overlap core (internal.hpp): one plan and one launch sequence per pass -------------------------------------------------

OverlapPlan overlap_plan(const isingmc_states *a, size_t n_pairs, bool default_pairs, size_t bins)
{
    const size_t n_pos = a->g->pk.n_pos, workspace = size_t(std::max(1, a->opt.cluster_workspace_bytes));
    OverlapPlan P;
    // accumulators {D, B} per pair; the packed kernels write whole groups (16 pairs) or pair blocks (32 pairs)
    P.blocks = (n_pairs + 31) / 32;
    P.acc_pairs = !a->packed ? n_pairs : default_pairs ? 16 * a->groups : 32 * P.blocks;
    P.acc0 = a->packed && default_pairs ? a->pk_bit0 / 2 : 0; // (device slot 16 group + pair; pk_bit0 is even)
    if (a->packed && !default_pairs) P.batch = nonlocal_batch(P.blocks, n_pos, workspace);
    if (!bins) return P;
    if (!a->packed) { // batches of pairs, two words per accumulator
        P.items = n_pairs;
        P.cbatch = nonlocal_batch(n_pairs, 2 * bins, workspace);
    } else { // replica groups (16 pair columns, no workspace) or pair blocks of 32 pairs with their gathered overlap words
        P.cols = default_pairs ? 16 : 32;
        P.items = default_pairs ? a->groups : P.blocks;
        P.col0 = P.acc0;
        P.cbatch = nonlocal_batch(P.items, 2 * P.cols * bins + (default_pairs ? 0 : n_pos), workspace);
    }
    return P;
}

// what the packed kernels read of a job: its two containers as PkSide, and the neighbour table of the real-coupling family
struct OverlapSides {
    PkSide A, B;
    const uint32_t *nbr_rj;
    uint32_t rj_slots;
};
static OverlapSides overlap_sides(const OverlapJob &J)
{
    const isingmc_states *a = J.a, *b = J.b;
    return {{a->d_state, J.d_sa, uint32_t(a->pk_bit0), uint32_t(a->R)},
            {b->d_state, J.d_sb, uint32_t(b->pk_bit0), uint32_t(b->R)},
            a->rj ? a->g->rj.nbr : nullptr,
            a->rj ? a->g->rj.slots : 0};
}

int overlap_enqueue(const OverlapJob &J, const OverlapPlan &P, const OverlapWork &W, OverlapSink sink)
{
    const isingmc_states *a = J.a, *b = J.b;
    const isingmc_graph *g = a->g;
    const OverlapSides S = overlap_sides(J);
    HIP_TRY(hipMemsetAsync(W.acc, 0, 2 * P.acc_pairs * sizeof(unsigned long long), a->stream));
    if (!a->packed) {
        HIP_TRY(overlap_launch_lattice(a->stream, a->d_state, b->d_state, J.d_sa, J.d_sb, g->geom, J.link, J.n_pairs, W.acc));
    } else if (J.default_pairs()) {
        HIP_TRY(overlap_launch_packed_pairs(a->stream, a->d_state, g->pk, S.nbr_rj, S.rj_slots, J.link, a->groups, W.acc));
    } else { // pair blocks of 32 pairs, their overlap words batched under a's cluster_workspace_bytes
        for (size_t b0 = 0; b0 < P.blocks; b0 += P.batch)
            HIP_TRY(overlap_launch_packed_tables(a->stream, S.A, S.B, g->pk, S.nbr_rj, S.rj_slots, J.link, uint32_t(b0),
                                                 uint32_t(std::min(P.batch, P.blocks - b0)), uint32_t(J.n_pairs), W.words, W.acc));
    }
    return sink(W.acc, 0, P.acc_pairs);
}

int overlap_class_enqueue(const OverlapJob &J, const OverlapPlan &P, const OverlapWork &W, OverlapSink sink)
{
    const isingmc_states *a = J.a, *b = J.b;
    const isingmc_graph *g = a->g;
    const isingmc_site_classes *C = J.classes;
    const bool default_pairs = J.default_pairs();
    const size_t bins = J.bins(), n_pos = g->pk.n_pos, rw = 2 * size_t(g->geom.wpp);
    const OverlapSides S = overlap_sides(J);
    for (size_t i0 = 0; i0 < P.items; i0 += P.cbatch) {
        const size_t n = std::min(P.cbatch, P.items - i0);
        HIP_TRY(hipMemsetAsync(W.cacc, 0, n * P.cols * bins * sizeof(unsigned long long), a->stream));
        if (!a->packed) {
            HIP_TRY(overlap_class_launch_lattice(a->stream, default_pairs ? a->d_state + 2 * i0 * rw : a->d_state.get(), b->d_state,
                                                 J.d_sa ? J.d_sa + i0 : nullptr, J.d_sb ? J.d_sb + i0 : nullptr, g->geom, C->lat, uint32_t(n), W.cacc));
        } else {
            if (!default_pairs) HIP_TRY(overlap_launch_packed_gather(a->stream, S.A, S.B, g->pk, uint32_t(i0), uint32_t(n), uint32_t(J.n_pairs), W.words));
            HIP_TRY(overlap_class_launch_packed(a->stream, default_pairs ? a->d_state + i0 * n_pos : W.words, uint32_t(n_pos), default_pairs, C->pk,
                                                uint32_t(n), W.cacc));
        }
        TRY(sink(W.cacc, i0 * P.cols, n * P.cols));
    }
    return ISINGMC_OK;
}

// ---- the synchronising calls: workspace from the call's DeviceScratch, accumulators read back ------------------------------------

// a's stream after b's sweeps and exchange rounds so far, before it reads b's configurations (the event is the between move's)
static int overlap_order_after(isingmc_states *a, isingmc_states *b)
{
    if (a == b) return ISINGMC_OK;
    if (!a->icmb.ev[0]) TRY(event_create(a->icmb.ev[0]));
    return stream_wait_for(a->stream, b->stream, a->icmb.ev[0]);
}

// the host tables of the pairing as the job's device tables (they live as long as the call, which waits for the device before it returns)
static int overlap_upload(DeviceScratch &scratch, const OverlapPairing &P, OverlapJob &J)
{
    if (P.default_pairs) return ISINGMC_OK;
    uint32_t *d = nullptr;
    TRY(scratch.alloc(&d, 2 * J.n_pairs));
    HIP_TRY(hipMemcpyAsync(d, P.slots_a, J.n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, J.a->stream));
    HIP_TRY(hipMemcpyAsync(d + J.n_pairs, P.slots_b, J.n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice, J.a->stream));
    J.d_sa = d;
    J.d_sb = d + J.n_pairs;
    return ISINGMC_OK;
}

extern "C" int isingmc_overlaps(isingmc_states *a, isingmc_states *b, const uint32_t *slots_a, const uint32_t *slots_b, size_t n_pairs,
                                int64_t *spin_out, int64_t *link_out)
{
    if (!a) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (!spin_out) return fail(ISINGMC_ERR_INVALID, "NULL argument: spin_out (link_out alone may be NULL)");
    OverlapPairing P;
    TRY(overlap_pairing(a, b, slots_a, slots_b, n_pairs, P));
    b = P.b;
    const isingmc_graph *g = a->g;
    TRY(use_device(g->device));
    TRY(overlap_lanes_join(a, b));
    const OverlapPlan L = overlap_plan(a, n_pairs, P.default_pairs, 0);
    OverlapJob J{a, b, nullptr, nullptr, n_pairs, link_out != nullptr, nullptr};
    OverlapWork W{nullptr, nullptr, nullptr};
    DeviceScratch scratch(a->stream);
    TRY(scratch.alloc(&W.acc, 2 * L.acc_pairs));
    TRY(overlap_upload(scratch, P, J));
    if (L.batch) TRY(scratch.alloc(&W.words, L.batch * g->pk.n_pos));
    TRY(overlap_order_after(a, b));
    std::vector<unsigned long long> h;
    auto sink = [&](const unsigned long long *acc, size_t, size_t n) { return read_back(a, h, acc, 2 * n); }; // waits: b may go on as soon as the call returns
    TRY(overlap_enqueue(J, L, W, sink));
    for (size_t p = 0; p < n_pairs; p++) {
        spin_out[p] = int64_t(g->nvars) - 2 * int64_t(h[2 * (L.acc0 + p)]);
        if (J.link) link_out[p] = int64_t(g->n_edges) - 2 * int64_t(h[2 * (L.acc0 + p) + 1]);
    }
    return ISINGMC_OK;
}

// ---- overlaps resolved by a class label per site ----------------------------------------------------------------
// (the class set itself, isingmc_site_classes, is in internal.hpp: the overlap series reads it too)

// the limits of a class set and the values of its tables ("" when they hold)
static std::string class_set_obstacle(const uint32_t *cls, size_t nvars, size_t n_tables, size_t n_classes)
{
    if (n_tables < 1 || n_tables > 8) return "n_tables must be 1 .. 8";
    if (n_classes < 1 || n_classes > 4096) return "n_classes must be 1 .. 4096";
    if (n_tables * n_classes > OVC_MAX_BINS) return "n_tables * n_classes must not exceed 8192 (the histogram of the checkerboard kernel: 32 KiB of LDS)";
    if (n_tables * nvars > 0xFFFFFFFFull) return "n_tables * nvars must stay below 2^32";
    for (size_t i = 0; i < n_tables * nvars; i++)
        if (cls[i] >= n_classes && cls[i] != ISINGMC_NO_CLASS)
            return "class value out of range: table " + std::to_string(i / nvars) + " gives site " + std::to_string(i % nvars) + " the class " +
                   std::to_string(cls[i]) + ", which is neither below n_classes = " + std::to_string(n_classes) + " nor ISINGMC_NO_CLASS";
    return "";
}

extern "C" int isingmc_host_class_segments(const uint32_t *site, size_t n_pos, const uint32_t *cls, size_t nvars, size_t n_tables, size_t n_classes,
                                           uint32_t *order_out, size_t *n_order_out, uint32_t *seg_out, size_t *n_seg_out, uint64_t *sizes_out)
{
    if (!site || !cls || !order_out || !n_order_out || !seg_out || !n_seg_out) return fail(ISINGMC_ERR_INVALID, "NULL argument (sizes_out alone may be NULL)");
    {
        const std::string why = class_set_obstacle(cls, nvars, n_tables, n_classes);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    for (size_t p = 0; p < n_pos; p++)
        if (site[p] != PAD_SITE && site[p] >= nvars) return fail(ISINGMC_ERR_INVALID, "site table entry out of range: a position holds a site below nvars or the padding mark");
    const ClassSegments S = class_segments(site, n_pos, cls, nvars, n_tables, n_classes);
    std::copy(S.order.begin(), S.order.end(), order_out);
    std::copy(S.seg.begin(), S.seg.end(), seg_out);
    if (sizes_out) std::copy(S.sizes.begin(), S.sizes.end(), sizes_out);
    *n_order_out = S.order.size();
    *n_seg_out = S.seg.size() / 4;
    return ISINGMC_OK;
}

template <typename T>
static int classes_upload(isingmc_site_classes *c, const T **dst, const T *src, size_t count)
{
    T *d = nullptr;
    TRY(dev_alloc(c->dev_allocs, &d, count));
    if (count) HIP_TRY(hipMemcpy(d, src, count * sizeof(T), hipMemcpyHostToDevice));
    *dst = d;
    return ISINGMC_OK;
}

static int site_classes_fill(isingmc_site_classes *c, const uint32_t *cls)
{
    const isingmc_graph *g = c->g;
    const size_t nvars = g->nvars, T = c->n_tables;
    c->sizes.assign(T * c->n_classes, 0);
    for (size_t t = 0; t < T; t++)
        for (size_t i = 0; i < nvars; i++)
            if (cls[t * nvars + i] != ISINGMC_NO_CLASS) c->sizes[t * c->n_classes + cls[t * nvars + i]]++;
    if (g->kind == ISINGMC_KIND_LATTICE2D) { // plane order: site (x, y) is bit (x / 2) % 32 of word y wpr + x / 64 of plane (x + y) & 1
        const LatGeom &L = g->geom;
        const size_t words = 2 * size_t(L.wpp);
        std::vector<uint32_t> perm(T * nvars), word_cls(T * words);
        for (size_t t = 0; t < T; t++) {
            for (uint32_t y = 0; y < L.H; y++)
                for (uint32_t x = 0; x < L.W; x++) {
                    const uint32_t plane = (x + y) & 1, i = x >> 1;
                    perm[(t * words + size_t(plane) * L.wpp + size_t(y) * L.wpr + (i >> 5)) * 32 + (i & 31)] = cls[t * nvars + size_t(y) * L.W + x];
                }
            for (size_t w = 0; w < words; w++) {
                const uint32_t *line = perm.data() + (t * words + w) * 32;
                word_cls[t * words + w] = std::all_of(line, line + 32, [&](uint32_t v) { return v == line[0]; }) ? line[0] : OVC_MIXED;
            }
        }
        TRY(classes_upload(c, &c->lat.cls, perm.data(), perm.size()));
        TRY(classes_upload(c, &c->lat.word_cls, word_cls.data(), word_cls.size()));
        c->lat.n_tables = uint32_t(T);
        c->lat.n_classes = uint32_t(c->n_classes);
        c->has_lat = true;
    } else if (g->packed_ok || g->rj_ok) { // the content of PkGraphDev::site, from the host's site -> position table
        const size_t n_pos = g->pk.n_pos;
        std::vector<uint32_t> site(n_pos, PAD_SITE), order(T * n_pos), seg(4 * T * (c->n_classes + n_pos / CLASS_SEGMENT_MAX));
        for (size_t i = 0; i < nvars; i++) site[g->pos[i]] = uint32_t(i);
        size_t n_order = 0, n_seg = 0;
        TRY(isingmc_host_class_segments(site.data(), n_pos, cls, nvars, T, c->n_classes, order.data(), &n_order, seg.data(), &n_seg, nullptr));
        const uint32_t *d_seg = nullptr;
        TRY(classes_upload(c, &c->pk.order, order.data(), n_order));
        TRY(classes_upload(c, &d_seg, seg.data(), 4 * n_seg));
        c->pk.seg = reinterpret_cast<const uint4 *>(d_seg);
        c->pk.n_seg = uint32_t(n_seg);
        c->pk.n_tables = uint32_t(T);
        c->pk.n_classes = uint32_t(c->n_classes);
        c->has_pk = true;
    }
    return ISINGMC_OK;
}

extern "C" int isingmc_site_classes_create(isingmc_graph *graph, const uint32_t *cls, size_t n_tables, size_t n_classes, isingmc_site_classes **out)
{
    if (!graph || !cls || !out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    *out = nullptr;
    {
        const std::string why = class_set_obstacle(cls, graph->nvars, n_tables, n_classes);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    TRY(use_device(graph->device));
    std::unique_ptr<isingmc_site_classes, int (*)(isingmc_site_classes *)> c(new isingmc_site_classes, isingmc_site_classes_destroy);
    c->g = graph;
    c->device = graph->device;
    c->n_tables = n_tables;
    c->n_classes = n_classes;
    TRY(site_classes_fill(c.get(), cls));
    *out = c.release();
    return ISINGMC_OK;
}

extern "C" int isingmc_site_classes_destroy(isingmc_site_classes *classes)
{
    if (!classes) return ISINGMC_OK;
    (void)hipSetDevice(classes->device); // (every measurement has waited for its kernels: nothing reads the blocks any more)
    delete classes;
    return ISINGMC_OK;
}

extern "C" int isingmc_site_classes_sizes(const isingmc_site_classes *classes, uint64_t *sizes_out)
{
    if (!classes || !sizes_out) return fail(ISINGMC_ERR_INVALID, "NULL argument");
    std::copy(classes->sizes.begin(), classes->sizes.end(), sizes_out);
    return ISINGMC_OK;
}

extern "C" int isingmc_overlaps_by_class(isingmc_states *a, isingmc_states *b, const uint32_t *slots_a, const uint32_t *slots_b, size_t n_pairs,
                                         const isingmc_site_classes *classes, int64_t *out)
{
    if (!a) return fail(ISINGMC_ERR_INVALID, "NULL states");
    if (!classes || !out) return fail(ISINGMC_ERR_INVALID, "NULL argument: classes and out are both needed");
    OverlapPairing P;
    TRY(overlap_pairing(a, b, slots_a, slots_b, n_pairs, P));
    b = P.b;
    {
        const std::string why = classes_obstacle(classes, a);
        if (!why.empty()) return fail(ISINGMC_ERR_INVALID, why);
    }
    TRY(use_device(a->g->device));
    TRY(overlap_lanes_join(a, b));
    const size_t bins = classes->n_tables * classes->n_classes;
    const OverlapPlan L = overlap_plan(a, n_pairs, P.default_pairs, bins);
    OverlapJob J{a, b, nullptr, nullptr, n_pairs, false, classes};
    OverlapWork W{nullptr, nullptr, nullptr};
    DeviceScratch scratch(a->stream);
    TRY(overlap_upload(scratch, P, J));
    TRY(overlap_order_after(a, b));
    TRY(scratch.alloc(&W.cacc, L.cbatch * L.cols * bins));
    if (L.batch) TRY(scratch.alloc(&W.words, L.cbatch * a->g->pk.n_pos));
    std::vector<unsigned long long> h;
    // the accumulators of pair p as the p-th [n_tables][n_classes] block of the result; columns that hold no pair of the call are passed over
    auto sink = [&](const unsigned long long *acc, size_t c0, size_t n) -> int {
        TRY(read_back(a, h, acc, n * bins));
        // (locals: through the captures every term of the inner loop would be loaded again behind each store)
        const size_t nb = bins, col0 = L.col0;
        const uint64_t *const sizes = classes->sizes.data();
        for (size_t c = 0; c < n; c++) {
            const size_t column = c0 + c, p = column - col0;
            if (column < col0 || p >= n_pairs) continue;
            const unsigned long long *const D = h.data() + c * nb;
            int64_t *const o = out + p * nb;
            for (size_t i = 0; i < nb; i++) o[i] = int64_t(sizes[i]) - 2 * int64_t(D[i]);
        }
        return ISINGMC_OK;
    };
    return overlap_class_enqueue(J, L, W, sink);
}
