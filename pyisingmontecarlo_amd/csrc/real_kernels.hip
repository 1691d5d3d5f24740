// Translation unit of the replica-packed real-coupling kernels (see real_types.hpp for why it is apart from isingmc.hip).
#include "real_kernels.hpp"

#include "kernel_pick.hpp"

namespace isingmc {

static or_last<4, 7, 11, 15, 23, 31> rj_slots(uint32_t slots) { return {int(slots)}; } // the slot counts with an RjShape

uint32_t rj_threads(uint32_t slots)
{
    uint32_t n = 256;
    pick(rj_slots(slots), [&](auto S) { n = uint32_t(RjShape<S.value>::THREADS); });
    return n;
}

hipError_t rj_launch_sweep(dim3 grid, hipStream_t stream, uint32_t *state, const RjGraphDev &G, uint32_t class_begin, uint32_t real_end,
                           uint64_t t, const uint2 *group_keys, const RjBeta *betas, uint32_t beta_stride, uint32_t q_lo, uint32_t q_hi)
{
    const bool whole = q_lo == 0 && q_hi >= 8; // every replica bit of the groups of this launch is decided
    const bool heavy = G.dshift != nullptr;
    // (partly owned groups of graphs WITHOUT heavy sites have their own instantiations: carrying the heavy-site shift cost the
    //  few-replica runs 9 % -- 2048^2 Gaussian x 8: 4.98 -> 4.54e11 -- when round 4 first folded them into the heavy ones)
    pick(rj_slots(G.slots), beta_stride == 0, !whole, heavy, [&](auto S, auto UB, auto PARTIAL, auto HEAVY) {
        hipLaunchKernelGGL((rj_sweep_kernel<S.value, UB.value, PARTIAL.value, HEAVY.value>), grid, dim3(RjShape<S.value>::THREADS), 0, stream, state, G,
                           class_begin, real_end, t, group_keys, betas, q_lo, q_hi);
    });
    return hipGetLastError();
}

// f(kernel, threads): the instantiation for (slots, bipartite, count_up) and its workgroup size, for its launch and its occupancy query alike
template <typename F>
static void rj_pick_measure(uint32_t slots, bool bip, bool up, F &&f)
{
    pick(rj_slots(slots), bip, up, [&](auto S, auto BIP, auto UP) { f(rj_measure_kernel<S.value, BIP.value, UP.value>, RjShape<S.value>::THREADS); });
}

hipError_t rj_launch_measure(dim3 grid, hipStream_t stream, const uint32_t *state, const RjGraphDev &G, const uint32_t *site,
                             uint32_t class0_end, uint32_t scan_end, bool count_up, unsigned long long *out)
{
    rj_pick_measure(G.slots, class0_end != 0, count_up, [&](auto kernel, int threads) {
        hipLaunchKernelGGL(kernel, grid, dim3(threads), 0, stream, state, G, site, class0_end, scan_end, out);
    });
    return hipGetLastError();
}

hipError_t rj_launch_energy_from_counts(hipStream_t stream, unsigned long long *meas, uint32_t first_slot, uint32_t n, int k_energy,
                                        double self_energy, double *out)
{
    hipLaunchKernelGGL(rj_energy_from_counts_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, meas, first_slot, n, k_energy, self_energy, out);
    return hipGetLastError();
}

int rj_measure_blocks_per_cu(uint32_t slots, bool bipartite, bool count_up)
{
    int n = 0;
    rj_pick_measure(slots, bipartite, count_up, [&](auto kernel, int threads) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, threads, 0) != hipSuccess) n = 0;
    });
    (void)hipGetLastError();
    return n;
}

} // namespace isingmc
