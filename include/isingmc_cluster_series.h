/* libisingmc.so: the cluster series.  A part of the C ABI of isingmc.h, which includes this header at its end: include
 * isingmc.h.  The entry points stand in a header of their own beside the two periodic series of isingmc.h because the cluster series
 * has no period and no record call: its rows are appended by the container's non-local steps. */
#ifndef ISINGMC_CLUSTER_SERIES_H
#define ISINGMC_CLUSTER_SERIES_H
#include "isingmc.h"
#ifdef __cplusplus
extern "C" {
#endif

/* ---- The cluster series: cluster-size moments of every non-local step, logged on the device (no reference counterpart) ----
 * The third device-resident log of ONE container `a`.  Its sample points are the container's non-local steps themselves: every
 * Swendsen-Wang step (kind ISINGMC_CLUSTER_SERIES_SW) or every isoenergetic cluster move inside the container (kind
 * ISINGMC_CLUSTER_SERIES_ICM) of isingmc_do_time_steps*, isingmc_run_sampling and isingmc_run_sampling_moments appends one row behind
 * itself on a's stream, without the host waiting for anything; no other step is touched.  Columns: the replicas in slot order
 * (SW; n_columns = count), or the pairs (2 p, 2 p + 1) (ICM; n_columns = count / 2).  A row holds six uint64 per column, over the
 * sizes s of the clusters the step built for that column:
 *   n_clusters, largest   what isingmc_cluster_stats / isingmc_icm_stats return after that step (they return the same with a series)
 *   sites                 sum s: nvars for a Swendsen-Wang step, the q = -1 sites of the pair for an isoenergetic move
 *   S2                    sum s^2, exact
 *   S4_lo, S4_hi          sum s^4 = S4_hi 2^64 + S4_lo, exact
 * Given the bonds of a Swendsen-Wang step, E[M^2 | bonds] = S2 and E[M^4 | bonds] = 3 S2^2 - 2 S4 (M: the magnetisation, of the
 * sublattice-signed spins on an antiferromagnet): chi = <S2> / N and <M^4> with far less variance than from the configurations.  The
 * sums are integer additions, independent of execution order and of how cluster_workspace_bytes cuts the step into batches.  While a
 * series is live the step's largest-cluster kernel is replaced by one that also forms the sums: the configurations, the random
 * numbers and the statistics are those of a container without a series.  The log holds `capacity` rows in one device block of the
 * series, at most the option "cluster_series_bytes" of `a` (isingmc_states_set_option; ISINGMC_CLUSTER_SERIES_BYTES, default 1 GiB).
 * isingmc_cluster_series_create: ISINGMC_ERR_INVALID, the container unchanged: an unknown kind; a container that could not take that
 *   kind of step, in the words isingmc_states_set_cluster_every / isingmc_states_set_icm_every refuse it with; a container that has
 *   a live cluster series already (one per container); capacity == 0; no column; a log beyond the byte budget.  The period itself may
 *   be switched on before or after.
 * A run call whose non-local steps (t % k == k - 1 inside the call, isingmc_host_nonlocal_steps) would overfill the log fails before
 *   it enqueues anything.  While a series is live isingmc_states_append, isingmc_pa_resample, isingmc_pa_run and isingmc_pt_attach
 *   are refused.  isingmc_icm_between appends nothing: its pairs live in two containers.
 * isingmc_cluster_series_count: rows held and the capacity (either pointer may be NULL).
 * isingmc_cluster_series_get: waits once for a's stream, then copies the rows [first, first + n): timesteps_out[n] (the timestep
 *   each step was), rows_out[n][n_columns][6]; either pointer may be NULL.  Changes nothing.
 * isingmc_cluster_series_reset: the row count back to 0 (enqueue only).
 * A series is destroyed before its container. */
typedef struct isingmc_cluster_series isingmc_cluster_series;
#define ISINGMC_CLUSTER_SERIES_SW 0  /* a row per Swendsen-Wang step, a column per replica */
#define ISINGMC_CLUSTER_SERIES_ICM 1 /* a row per isoenergetic cluster move inside the container, a column per pair */
int isingmc_cluster_series_create(isingmc_states *a, int kind, size_t capacity, isingmc_cluster_series **out);
int isingmc_cluster_series_count(const isingmc_cluster_series *s, size_t *n_out, size_t *capacity_out);
int isingmc_cluster_series_get(isingmc_cluster_series *s, size_t first, size_t n, uint64_t *timesteps_out, uint64_t *rows_out);
int isingmc_cluster_series_reset(isingmc_cluster_series *s);
int isingmc_cluster_series_destroy(isingmc_cluster_series *s);

#ifdef __cplusplus
}
#endif
#endif /* ISINGMC_CLUSTER_SERIES_H */
