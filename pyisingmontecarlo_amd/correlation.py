"""From overlaps resolved by plane to the wave-vector-dependent spin-glass susceptibility and the second-moment
correlation length -- numpy only, no device.

For a wave vector k along a lattice axis,  sum_i q_i e^{i k x_i} = sum_x e^{i k x} Q_x  with Q_x the overlap q_i = s_i^a s_i^b summed
over the plane at coordinate x: the device returns the L integers Q_x per pair and axis (States.overlaps_by_class with the tables
of plane_classes), and the rest is a Fourier transform of L numbers.

The rows of an overlap series (OverlapSeries.get, ClassicalTempering.get_measured_overlaps) feed both directly:
overlap_moments takes `spin` [n, P], and chi_sg / correlation_length take by_class[..., t, :] -- [n, P, L] for axis t -- as they
come, the sample and pair axes being leading axes like any other.

The rows of an observable series (ObservableSeries.get) do the same for the magnetisation of a ferromagnet:
magnetisation_moments takes `magnetisation` [n, C], and structure_factor takes by_class[..., t, :] -- the plane magnetisations M_x of
axis t -- as they come; its rows, averaged over samples, feed correlation_length unchanged.
"""
import numpy as np


def plane_classes(shape):
    """uint32[ndim, prod(shape)]: table a gives site i the class coords[a], its coordinate along axis a, where
    i = np.ravel_multi_index(coords, shape) (C order: the LAST axis runs fastest).  The caller's site numbering must be this one:
    a 2-d lattice with site y * W + x is shape (H, W) -- table 0 the rows y, table 1 the columns x -- and a cubic lattice with
    site (z * L + y) * L + x is shape (L, L, L) with the tables z, y, x."""
    shape = tuple(int(n) for n in shape)
    return np.indices(shape, dtype=np.uint32).reshape(len(shape), -1)


def chi_sg(planes, nvars):
    """|fft(planes, axis=-1)|^2 / nvars: entry n is chi_SG at k_n = 2 pi n / L for ONE pair, planes[..., x] = Q_x the L plane
    overlaps of one axis (leading axes, such as pairs, are kept).  Average it over pairs and samples before anything else."""
    f = np.fft.fft(np.asarray(planes, dtype=np.float64), axis=-1)
    return (f.real ** 2 + f.imag ** 2) / float(nvars)


def overlap_moments(spin, nvars):
    """(<q>, <q^2>, <q^4>, binder) per column of spin[n, ...]: q = spin / nvars averaged over the n samples of axis 0 (the rows of
    an overlap series), and the Binder ratio (3 - <q^4> / <q^2>^2) / 2 -- 1 when every sample has |q| = 1, 0 for a Gaussian q.  A
    column whose <q^2> is 0 has no ratio: NaN.  Average over disorder realisations BEFORE the ratio, as with correlation_length."""
    q = np.asarray(spin, dtype=np.float64) / float(nvars)
    q1, q2, q4 = q.mean(axis=0), (q ** 2).mean(axis=0), (q ** 4).mean(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        binder = np.where(q2 > 0, (3.0 - q4 / q2 ** 2) / 2.0, np.nan)
    return q1, q2, q4, binder


def magnetisation_moments(mag, nvars):
    """(<m>, <|m|>, <m^2>, <m^4>, U4) per column of mag[n, ...]: m = mag / nvars averaged over the n samples of axis 0 (the rows of
    an observable series), and the Binder cumulant U4 = 1 - <m^4> / (3 <m^2>^2) -- 2/3 when every sample has |m| = 1, 0 for a
    Gaussian m.  A column whose <m^2> is 0 has no cumulant: NaN.  The susceptibility is beta N (<m^2> - <|m|>^2)."""
    m = np.asarray(mag, dtype=np.float64) / float(nvars)
    m1, ma, m2, m4 = m.mean(axis=0), np.abs(m).mean(axis=0), (m ** 2).mean(axis=0), (m ** 4).mean(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        u4 = np.where(m2 > 0, (3.0 * m2 ** 2 - m4) / (3.0 * m2 ** 2), np.nan)  # (one rounding: exactly 2/3 for |m| = 1)
    return m1, ma, m2, m4, u4


def cluster_estimators(s2, s4_lo, s4_hi, nvars):
    """(chi, <m^2>, <m^4>, U4) per column from the rows of a cluster series of Swendsen-Wang steps (DESIGN.md S24:
    ClusterSeries.get), s2[n, ...] = sum s^2 and s4 = s4_hi 2^64 + s4_lo = sum s^4 over the cluster sizes of each step.  Given the
    bonds of a step the clusters take their signs independently, so E[M^2 | bonds] = S2 and E[M^4 | bonds] = 3 S2^2 - 2 S4:
    chi = <S2> / N, <m^2> = <S2> / N^2, <m^4> = <3 S2^2 - 2 S4> / N^4 and U4 = 1 - <m^4> / (3 <m^2>^2), averaged over the n rows of
    axis 0 in float64.  S4 <= S2^2, so 3 S2^2 - 2 S4 >= S2^2: the difference loses no digits.  On an antiferromagnet m is the
    staggered magnetisation."""
    n = float(nvars)
    S2 = np.asarray(s2, dtype=np.uint64).astype(np.float64)
    S4 = np.asarray(s4_hi, dtype=np.uint64).astype(np.float64) * 2.0 ** 64 + np.asarray(s4_lo, dtype=np.uint64).astype(np.float64)
    m2 = S2.mean(axis=0) / n ** 2
    m4 = (3.0 * S2 ** 2 - 2.0 * S4).mean(axis=0) / n ** 4
    with np.errstate(divide="ignore", invalid="ignore"):
        u4 = np.where(m2 > 0, (3.0 * m2 ** 2 - m4) / (3.0 * m2 ** 2), np.nan)
    return m2 * n, m2, m4, u4


def structure_factor(planes, nvars):
    """|sum_x e^{i k x} M_x|^2 / nvars per row and wave number: entry n is S(k_n) at k_n = 2 pi n / L for ONE configuration,
    planes[..., x] = M_x the L plane magnetisations of one axis (the by_class rows of plane_classes; leading axes, such as samples
    and replicas, are kept).  Average it over samples before correlation_length takes the ratio."""
    f = np.fft.fft(np.asarray(planes, dtype=np.float64), axis=-1)
    return (f.real ** 2 + f.imag ** 2) / float(nvars)


def correlation_length(chi0, chik, L, n=1):
    """xi_L = sqrt(chi0 / chik - 1) / (2 sin(pi n / L)) from chi0 = chi_SG(0) and chik = chi_SG(k_n), k_n = 2 pi n / L.

    Both arguments are AVERAGED susceptibilities: the average of chi_sg over the pairs of a sample (the thermal average) and over
    the samples (the disorder average) comes BEFORE the ratio.  The ratio of one pair's values is not an estimate of anything: a
    single |q_hat(k)|^2 is exponentially distributed and the mean of the ratios diverges."""
    chi0, chik = np.asarray(chi0, dtype=np.float64), np.asarray(chik, dtype=np.float64)
    return np.sqrt(chi0 / chik - 1.0) / (2.0 * np.sin(np.pi * n / L))


def autocorrelation(diff, counts, nvars):
    """C[..., l] = 1 - 2 diff[..., l] / (nvars counts[l]) from the sums of a lag ring (Autocorrelation.get): diff[R, L + 1]
    the differing sites summed over the counts[l] terms of lag l.  A lag without a term (counts[l] == 0) has no value: NaN.  Units
    of the lag axis: samples."""
    d = np.asarray(diff, dtype=np.uint64).astype(np.float64)
    n = np.asarray(counts, dtype=np.uint64).astype(np.float64) * float(nvars)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n > 0, 1.0 - 2.0 * d / n, np.nan)


def integrated_time(corr, c=6.0):
    """(tau_int float64[...], window int64[...]) per row of corr[..., l], l = 0 .. L, with Sokal's automatic window:
    tau(W) = 1/2 + sum_{l=1..W} C(l), summed in the order of l, and the smallest W >= 1 with W >= c tau(W).  A row without such a W
    within the measured lags returns tau(L) and window = -1: the run or the ring is too short for that row.  Units: samples."""
    corr = np.asarray(corr, dtype=np.float64)
    L = corr.shape[-1] - 1
    if L < 1:  # lag 0 alone: tau(0) = 1/2, no window
        return np.full(corr.shape[:-1], 0.5), np.full(corr.shape[:-1], -1, dtype=np.int64)
    tau = 0.5 + np.cumsum(corr[..., 1:], axis=-1)              # tau[..., W - 1] = tau(W)
    ok = np.arange(1, L + 1, dtype=np.float64) >= c * tau       # (a NaN compares false)
    found = ok.any(axis=-1)
    first = np.where(found, ok.argmax(axis=-1), L - 1)
    tau_int = np.take_along_axis(tau, np.asarray(first)[..., None], axis=-1)[..., 0]
    return tau_int, np.where(found, first + 1, -1).astype(np.int64)
