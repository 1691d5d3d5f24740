// Host shim with the Python surface of the reference's pyo3 module `py_monte_carlo`
// (src/lib.rs:14-22) for the classical hot path: classes Lattice (src/lattice.rs:27-470) and
// ClassicIsing (src/classicising.rs:11-180).  Same method names, positional order, keyword names,
// None-defaults, return tuple order, dtypes (float64 / bool) and ValueError messages.  The reference
// host is Rust/pyo3; no Rust toolchain exists in this image, so the shim is C++/pybind11 over the C
// ABI of include/isingmc.h -- exactly the calls a pyo3 maintainer would bind.
// All Monte-Carlo work happens in libisingmc.so's HIP kernels; nothing here computes a spin flip.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <memory>
#include <limits>
#include <optional>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "isingmc.h"

namespace py = pybind11;

using Edge = std::pair<std::pair<size_t, size_t>, double>;

namespace {

void check(int rc)
{
    if (rc == ISINGMC_OK) return;
    const std::string msg = isingmc_last_error();
    if (rc == ISINGMC_ERR_INVALID) throw py::value_error(msg);
    if (rc == ISINGMC_ERR_ALLOC) throw std::bad_alloc();
    throw std::runtime_error(msg);
}

int default_device()
{
    if (const char *d = std::getenv("ISINGMC_DEVICE")) return std::atoi(d);
    if (const char *lr = std::getenv("LOCAL_RANK")) { // one process per GPU under torchrun
        int count = 0;
        if (isingmc_device_count(&count) == ISINGMC_OK && std::atoi(lr) < count) return std::atoi(lr);
    }
    return 0;
}

// ISINGMC_DEVICES=0,1,...: the devices Lattice.run_monte_carlo* fans its experiments out over (one host thread and
// one isingmc_states per entry; an ordinal may repeat).  Unset: the one device of default_device().
std::vector<int> default_devices()
{
    std::vector<int> out;
    if (const char *e = std::getenv("ISINGMC_DEVICES")) {
        const std::string str(e);
        size_t pos = 0;
        while (pos <= str.size()) {
            const size_t comma = std::min(str.find(',', pos), str.size());
            const std::string tok = str.substr(pos, comma - pos);
            if (!tok.empty()) {
                if (tok == "all") {
                    int count = 0;
                    if (isingmc_device_count(&count) == ISINGMC_OK)
                        for (int d = 0; d < count; d++) out.push_back(d);
                } else {
                    out.push_back(std::atoi(tok.c_str()));
                }
            }
            pos = comma + 1;
        }
    }
    if (out.empty()) out.push_back(default_device());
    return out;
}

bool compat_anneal_bug()
{
    const char *e = std::getenv("ISINGMC_COMPAT_ANNEAL_BUG");
    return e && e[0] && e[0] != '0';
}

struct GraphHandle {
    isingmc_graph *g = nullptr;
    ~GraphHandle() { isingmc_graph_destroy(g); }
};

struct StatesHandle {
    isingmc_states *s = nullptr;
    std::shared_ptr<GraphHandle> graph; // the graph must outlive the states
    ~StatesHandle() { isingmc_states_destroy(s); }
};

// class tables as Python gives them: one integer array of nvars classes or a stack [n_tables, nvars]; n_classes
// None = the largest class + 1, ISINGMC_NO_CLASS entries left aside
struct ClassTables {
    std::vector<uint32_t> cls;
    size_t n_tables = 0, n_classes = 0;
};

ClassTables class_tables(const py::object &tables, const py::object &n_classes, size_t nvars)
{
    const auto arr = py::array_t<int64_t, py::array::c_style | py::array::forcecast>::ensure(tables);
    if (!arr || arr.ndim() < 1 || arr.ndim() > 2 || size_t(arr.shape(arr.ndim() - 1)) != nvars)
        throw py::value_error("class tables must be one integer array of nvars entries, or a stack [n_tables, nvars] of them");
    ClassTables T;
    T.n_tables = arr.ndim() == 2 ? size_t(arr.shape(0)) : 1;
    T.cls.resize(size_t(arr.size()));
    const int64_t *v = arr.data();
    int64_t largest = -1;
    for (size_t i = 0; i < T.cls.size(); i++) {
        if (v[i] < 0 || v[i] > int64_t(ISINGMC_NO_CLASS)) throw py::value_error("class value out of range: a class is a non-negative integer or NO_CLASS (0xFFFFFFFF)");
        T.cls[i] = uint32_t(v[i]);
        if (T.cls[i] != ISINGMC_NO_CLASS) largest = std::max(largest, v[i]);
    }
    T.n_classes = n_classes.is_none() ? size_t(largest + 1 > 0 ? largest + 1 : 1) : n_classes.cast<size_t>();
    return T;
}

struct ClassesHandle {
    isingmc_site_classes *c = nullptr;
    ~ClassesHandle() { isingmc_site_classes_destroy(c); }
};

// a device series with the class set it reads: the series goes first, and both before their container.
// columns: the pairs of an overlap series, the replicas of an observable series
template <typename Series, int (*Destroy)(Series *)>
struct SeriesHandleOf {
    Series *s = nullptr;
    ClassesHandle classes;
    bool link = false;
    size_t columns = 0, n_tables = 0, n_classes = 0;
    ~SeriesHandleOf() { Destroy(s); }
};
using SeriesHandle = SeriesHandleOf<isingmc_overlap_series, isingmc_overlap_series_destroy>;
using ObsSeriesHandle = SeriesHandleOf<isingmc_observable_series, isingmc_observable_series_destroy>;
using ClusterSeriesHandle = SeriesHandleOf<isingmc_cluster_series, isingmc_cluster_series_destroy>; // (no class set; columns: replicas or pairs)

// the lag ring of a container: it goes before the container
struct AutocorrHandle {
    isingmc_autocorr *ac = nullptr;
    size_t every = 0, n_lags = 0;
    ~AutocorrHandle() { isingmc_autocorr_destroy(ac); }
};

// C[r][l] = 1 - 2 diff[r][l] / (N counts[l]) as float64[R, cols] for the lags 0 .. cols - 1 of sums laid out [R][row]; NaN where a lag has no term
py::array_t<double> autocorr_array(const std::vector<uint64_t> &counts, const std::vector<uint64_t> &diff, size_t R, size_t row, size_t cols, size_t nvars)
{
    py::array_t<double> corr(std::vector<ssize_t>{ssize_t(R), ssize_t(cols)});
    double *c = corr.mutable_data();
    for (size_t r = 0; r < R; r++)
        for (size_t l = 0; l < cols; l++)
            c[r * cols + l] = counts[l] ? 1.0 - 2.0 * double(diff[r * row + l]) / (double(nvars) * double(counts[l])) : std::numeric_limits<double>::quiet_NaN();
    return corr;
}

// the rows of a cluster series, t[n] and rows[n][columns][6] as isingmc_cluster_series_get hands them out, as (timesteps uint64[m],
// n_clusters, largest, sites, s2, s4_lo, s4_hi: uint64[m, C] each): the m rows of timesteps >= from_t
py::tuple cluster_series_rows(const std::vector<uint64_t> &t, const std::vector<uint64_t> &rows, size_t columns, uint64_t from_t)
{
    const size_t n = t.size();
    size_t skip = 0;
    while (skip < n && t[skip] < from_t) skip++;
    const ssize_t N = ssize_t(n - skip), C = ssize_t(columns);
    py::array_t<uint64_t> ts(std::vector<ssize_t>{N});
    std::copy(t.begin() + skip, t.end(), ts.mutable_data());
    py::tuple out(7);
    out[0] = ts;
    for (size_t e = 0; e < 6; e++) {
        py::array_t<uint64_t> a(std::vector<ssize_t>{N, C});
        uint64_t *d = a.mutable_data();
        for (size_t k = skip; k < n; k++)
            for (size_t c = 0; c < columns; c++) d[(k - skip) * columns + c] = rows[(k * columns + c) * 6 + e];
        out[e + 1] = a;
    }
    return out;
}

struct EdgeArrays {
    std::vector<uint64_t> a, b;
    std::vector<double> j;
    size_t nvars = 0;
};

// [((a, b), j), ...] -> three arrays, straight off the CPython objects: the generic pybind11 caster
// takes tens of seconds on the 3.4e7 edges of a 4096^2 lattice, this loop about one.
EdgeArrays split_edges(const py::object &edges)
{
    PyObject *seq = PySequence_Fast(edges.ptr(), "edges must be a sequence of ((a, b), j) entries");
    if (!seq) throw py::error_already_set();
    const py::object guard = py::reinterpret_steal<py::object>(seq);
    const Py_ssize_t n = PySequence_Fast_GET_SIZE(seq);
    PyObject **items = PySequence_Fast_ITEMS(seq);
    EdgeArrays E;
    E.a.resize(n);
    E.b.resize(n);
    E.j.resize(n);
    auto pair_of = [](PyObject *o, PyObject *&x, PyObject *&y) {
        if (PyTuple_Check(o) && PyTuple_GET_SIZE(o) == 2) { x = PyTuple_GET_ITEM(o, 0); y = PyTuple_GET_ITEM(o, 1); return true; }
        if (PyList_Check(o) && PyList_GET_SIZE(o) == 2) { x = PyList_GET_ITEM(o, 0); y = PyList_GET_ITEM(o, 1); return true; }
        return false;
    };
    for (Py_ssize_t k = 0; k < n; k++) {
        PyObject *ab = nullptr, *j = nullptr, *a = nullptr, *b = nullptr;
        if (!pair_of(items[k], ab, j) || !pair_of(ab, a, b))
            throw py::type_error("edges must be ((a, b), j) entries: bad entry " + std::to_string(k));
        const unsigned long long ua = PyLong_AsUnsignedLongLong(a), ub = PyLong_AsUnsignedLongLong(b);
        const double dj = PyFloat_AsDouble(j);
        if (PyErr_Occurred()) throw py::error_already_set();
        E.a[k] = ua;
        E.b[k] = ub;
        E.j[k] = dj;
        E.nvars = std::max<size_t>(E.nvars, std::max(ua, ub) + 1); // lattice.rs:51-55
    }
    return E;
}

std::shared_ptr<GraphHandle> make_graph(const EdgeArrays &E, const std::vector<double> *biases, int device,
                                        bool force_general, bool stable_path = false)
{
    auto h = std::make_shared<GraphHandle>();
    py::gil_scoped_release nogil;
    // The sign of the bias term lives in the un-vendored crate (unverified convention).  The library's
    // Hamiltonian is E = sum J s s - sum h s (a positive bias favours True); ISINGMC_COMPAT_BIAS_SIGN=-1 hands it -h, i.e.
    // E = sum J s s + sum h s, should the crate turn out to use that sign.
    std::vector<double> flipped;
    const char *sign = std::getenv("ISINGMC_COMPAT_BIAS_SIGN");
    if (biases && sign && std::atoi(sign) < 0) {
        flipped.resize(biases->size());
        for (size_t i = 0; i < flipped.size(); i++) flipped[i] = -(*biases)[i];
        biases = &flipped;
    }
    check(isingmc_graph_create(E.a.data(), E.b.data(), E.j.data(), E.a.size(), E.nvars,
                               biases ? biases->data() : nullptr, device,
                               (force_general ? ISINGMC_FLAG_FORCE_GENERAL : 0u) | (stable_path ? ISINGMC_FLAG_STABLE_PATH : 0u), &h->g));
    return h;
}

std::vector<uint8_t> to_bytes(const std::vector<bool> &v)
{
    return std::vector<uint8_t>(v.begin(), v.end());
}

using Range = std::optional<std::pair<size_t, size_t>>;

// ------------------------------------------------------------------------------------------------
// Lattice (src/lattice.rs:27-470, classical methods)
// ------------------------------------------------------------------------------------------------
class Lattice {
public:
    Lattice(const py::object &edges, std::optional<uint64_t> seed_gen, std::optional<bool> use_allocator)
        : E_(std::make_shared<EdgeArrays>(split_edges(edges))), seed_gen_(seed_gen),
          use_allocator_(use_allocator.value_or(true)), devices_(default_devices())
    {
        if (E_->a.empty()) throw py::value_error("Must supply some edges for graph"); // lattice.rs:70-72
    }

    // extension: numpy ingest without building 10^7 Python tuples
    static Lattice from_arrays(py::array_t<uint64_t, py::array::c_style | py::array::forcecast> a,
                               py::array_t<uint64_t, py::array::c_style | py::array::forcecast> b,
                               py::array_t<double, py::array::c_style | py::array::forcecast> j,
                               std::optional<uint64_t> seed_gen)
    {
        if (a.ndim() != 1 || a.size() != b.size() || a.size() != j.size())
            throw py::value_error("edge arrays must be 1-d and of equal length");
        if (a.size() == 0) throw py::value_error("Must supply some edges for graph");
        Lattice L;
        auto E = std::make_shared<EdgeArrays>();
        E->a.assign(a.data(), a.data() + a.size());
        E->b.assign(b.data(), b.data() + b.size());
        E->j.assign(j.data(), j.data() + j.size());
        for (ssize_t k = 0; k < a.size(); k++) E->nvars = std::max<size_t>(E->nvars, std::max(E->a[k], E->b[k]) + 1);
        L.E_ = E;
        L.seed_gen_ = seed_gen;
        L.devices_ = default_devices();
        return L;
    }

    void set_seed_gen(std::optional<uint64_t> seed_gen) { seed_gen_ = seed_gen; } // lattice.rs:78-80

    std::vector<uint64_t> make_seeds(size_t num_experiments) const // lattice.rs:83-91
    {
        std::vector<uint64_t> seeds(num_experiments);
        check(isingmc_host_make_seeds(seed_gen_.has_value(), seed_gen_.value_or(0), num_experiments, seeds.data()));
        return seeds;
    }

    void set_enable_rvb_update(bool v) { enable_rvb_ = v; }      // lattice.rs:94-96 (QMC only; stored)
    void set_enable_heatbath_update(bool v) { enable_heatbath_ = v; } // lattice.rs:99-101

    void set_individual_bias(size_t var, double bias) // lattice.rs:104-126
    {
        if (var >= E_->nvars)
            throw py::value_error("Index out of bounds: variable " + std::to_string(var) + " out of " +
                                  std::to_string(E_->nvars));
        if (biases_.empty()) biases_.assign(E_->nvars, global_bias_);
        biases_[var] = bias;
        graphs_.clear();
    }

    void set_global_bias(double bias) // lattice.rs:129-131
    {
        biases_.clear();
        global_bias_ = bias;
        graphs_.clear();
    }

    void set_transverse_field(double transverse) // lattice.rs:134-146
    {
        if (transverse > 0.0) transverse_ = transverse;
        else if (transverse == 0.0) transverse_.reset();
        else throw py::value_error("Transverse field must be positive");
    }

    void set_initial_state(const std::vector<bool> &initial_state) // lattice.rs:149-161
    {
        if (initial_state.size() == E_->nvars) initial_state_ = to_bytes(initial_state);
        else if (initial_state.empty()) initial_state_.clear();
        else throw py::value_error("Initial state must be of the same size as biases, or 0.");
    }

    // extensions: device ordinal, and forcing the general edge-list path (BASELINE config c5)
    void set_device(int device) { devices_ = {device}; graphs_.clear(); }
    void set_devices(const std::vector<int> &devices) // extension: the device list of the in-process fan-out
    {
        if (devices.empty()) throw py::value_error("the device list must not be empty");
        devices_ = devices;
        graphs_.clear();
    }
    std::vector<int> get_devices() const { return devices_; }
    void set_force_general_path(bool v) { force_general_ = v; graphs_.clear(); }
    // Experiment k of a call depends on seed k alone in the reference (lattice.rs:83-91, 198).  Here the kernel FAMILY -- and with
    // it the Markov chain -- of a general graph normally follows the number of experiments of the call;
    // set_stable_path(True) fixes it from the graph alone: row k of run_monte_carlo(beta, T, R) is then the same for every R > k.
    void set_stable_path(bool v) { stable_path_ = v; graphs_.clear(); }
    // extension: every k-th timestep of the run_* methods is a Swendsen-Wang cluster step (isingmc_states_set_cluster_every;
    // 0 = off, the default).  Applied to every container the run_* methods create; a graph the cluster step does not serve raises
    // ValueError there.  (Not wired to only_basic_moves: its default None would switch it on.)
    void set_cluster_update_every(size_t k) { cluster_every_ = k; }
    // extension: every k-th timestep of the run_* methods is an isoenergetic cluster move between the experiments (2 p, 2 p + 1)
    // (isingmc_states_set_icm_every; 0 = off, the default): the non-local move for +-J glasses.  Applied to every container the
    // run_* methods create; the device blocks then hold whole pairs.
    void set_replica_cluster_update_every(size_t k) { icm_every_ = k; }
    // extension: the rounds of Philox4x32 in the draws of the Metropolis sweeps, 10 or 7 (option "philox_rounds").
    // Applied to every container the run_* methods create; a graph whose containers run on a family that 7 does not serve raises
    // ValueError there -- never a run with ten rounds instead.
    void set_rng_rounds(int rounds)
    {
        if (rounds != 7 && rounds != 10) throw py::value_error("rng_rounds must be 7 or 10 (rounds of Philox4x32 in the sweeps' draws)");
        rng_rounds_ = rounds;
    }
    // the option on a container just created (nothing when set_rng_rounds was never called: the environment's default stays)
    int apply_rng_rounds(isingmc_states *s) const { return rng_rounds_ ? isingmc_states_set_option(s, "philox_rounds", *rng_rounds_) : ISINGMC_OK; }
    py::dict engine_info(std::optional<size_t> num_experiments)
    {
        isingmc_graph_info_t info;
        check(isingmc_graph_info(graph()->g, &info));
        py::dict d;
        d["stable_path"] = bool(info.stable_path);
        d["cluster_update_every"] = cluster_every_;
        d["replica_cluster_update_every"] = icm_every_;
        int rounds = 10; // what set_rng_rounds asked for, else what a container created now would start with
        check(isingmc_graph_philox_rounds(graph()->g, &rounds));
        d["rng_rounds"] = rng_rounds_.value_or(rounds);
        if (num_experiments) { // the kernel family a call with that many experiments runs on
            int family = 0;
            check(isingmc_graph_family_for(graph()->g, *num_experiments, &family));
            static const char *names[] = {"checkerboard", "csr_f64", "packed_bitsliced", "packed_real"};
            d["family"] = names[family & 3];
        }
        d["kind"] = info.kind == ISINGMC_KIND_LATTICE2D ? "lattice2d" : "general";
        d["device"] = info.device;
        d["nvars"] = info.nvars;
        d["width"] = info.width;
        d["height"] = info.height;
        d["n_colours"] = info.n_colours;
        d["uniform_sign"] = bool(info.uniform_sign);
        d["field"] = info.field;
        d["open_x"] = bool(info.open_x);
        d["open_y"] = bool(info.open_y);
        d["packed_degree"] = info.packed_degree;
        d["real_slots"] = info.real_slots; // 4 .. 31: the real-coupling packed path applies (graphs beyond the LDS-resident CSR kernel: from ONE experiment on)
        d["real_quantum_log2"] = info.real_quantum_log2;
        d["real_energy_log2"] = info.real_energy_log2;
        d["real_heavy_sites"] = info.real_heavy_sites;
        return d;
    }

    // lattice.rs:171-221
    py::tuple run_monte_carlo(double beta, size_t timesteps, size_t num_experiments, std::optional<bool>,
                              std::optional<bool>, Range replica_range)
    {
        require_classical();
        const auto [lo, hi] = bounds(num_experiments, replica_range);
        const size_t R = hi - lo, N = E_->nvars;
        py::array_t<double> energies(std::vector<ssize_t>{ssize_t(R)});
        py::array_t<bool> states(std::vector<ssize_t>{ssize_t(R), ssize_t(N)});
        double *e = energies.mutable_data();
        uint8_t *st = reinterpret_cast<uint8_t *>(states.mutable_data());
        fan_out(num_experiments, lo, hi, [&](isingmc_states *s, size_t off) {
            int rc = isingmc_do_time_steps(s, timesteps, &beta, 0, nullptr);
            if (rc == ISINGMC_OK) rc = isingmc_get_energies(s, e + off);
            if (rc == ISINGMC_OK) rc = isingmc_get_states(s, st + off * N, N);
            return rc;
        });
        return py::make_tuple(energies, states);
    }

    // lattice.rs:231-299
    py::tuple run_monte_carlo_sampling(double beta, size_t timesteps, size_t num_experiments, std::optional<bool>,
                                       std::optional<size_t> thermalization_time, std::optional<size_t> sampling_freq,
                                       std::optional<bool>, Range replica_range)
    {
        require_classical();
        const size_t therm = thermalization_time.value_or(0), freq = sampling_freq.value_or(1);
        if (freq == 0) throw py::value_error("sampling_freq must be positive");
        const size_t S = timesteps / freq; // lattice.rs:247
        const auto [lo, hi] = bounds(num_experiments, replica_range);
        const size_t R = hi - lo, N = E_->nvars;
        py::array_t<double> energies(std::vector<ssize_t>{ssize_t(R), ssize_t(S)});
        py::array_t<bool> states(std::vector<ssize_t>{ssize_t(R), ssize_t(S), ssize_t(N)});
        double *e = energies.mutable_data();
        uint8_t *st = reinterpret_cast<uint8_t *>(states.mutable_data());
        // lattice.rs:271-287: thermalise, then S x { freq steps; record state + energy } -- one library call per shard
        fan_out(num_experiments, lo, hi, [&](isingmc_states *s, size_t off) {
            return isingmc_run_sampling(s, beta, therm, freq, S, e + off * S, st + off * S * N);
        });
        return py::make_tuple(energies, states);
    }

    // extension: the classical counterpart of run_quantum_monte_carlo_and_measure_spins.  The bookkeeping of
    // run_monte_carlo_sampling -- thermalise, then timesteps sweeps with a sample every sampling_freq -- with the samples summed on
    // the device: no configuration crosses the bus.  Returns (energies f64[R] of the final configurations, mean_spins f64[R, N], or
    // f64[N] when per_experiment is false), plus mean_bonds f64[n_edges] (the average of s_a s_b per edge-list entry) when bonds is
    // set, which needs per_experiment=False.  Means are the exact integer sums over their counts, True = +1; NaN without a sample.
    // One device: the sums live in one container.  Cluster periods set on this object apply.
    py::tuple run_monte_carlo_and_measure_spins(double beta, size_t timesteps, size_t num_experiments, std::optional<size_t> thermalization_time,
                                                std::optional<size_t> sampling_freq, bool per_experiment, bool bonds)
    {
        require_classical();
        const size_t therm = thermalization_time.value_or(0), freq = sampling_freq.value_or(1);
        if (freq == 0) throw py::value_error("sampling_freq must be positive");
        if (bonds && per_experiment) throw py::value_error("bond sums per experiment are not offered: bonds=True needs per_experiment=False");
        if (devices_.size() != 1) throw py::value_error("spin measurement runs on one device: the sums live in one container (set_device)");
        const size_t S = timesteps / freq, R = num_experiments, N = E_->nvars, NE = E_->a.size();
        const unsigned flags = (per_experiment ? ISINGMC_MOMENTS_PER_REPLICA : 0u) | (bonds ? ISINGMC_MOMENTS_BONDS : 0u);
        py::array_t<double> energies(std::vector<ssize_t>{ssize_t(R)});
        py::array_t<double> spins(per_experiment ? std::vector<ssize_t>{ssize_t(R), ssize_t(N)} : std::vector<ssize_t>{ssize_t(N)});
        py::array_t<double> bond_means(std::vector<ssize_t>{ssize_t(bonds ? NE : 0)});
        double *e = energies.mutable_data(), *sp = spins.mutable_data(), *bm = bond_means.mutable_data();
        std::vector<int64_t> site(per_experiment ? R * N : N), bond(bonds ? NE : 0);
        uint64_t n = 0;
        fan_out(num_experiments, 0, R, [&](isingmc_states *s, size_t) {
            int rc = isingmc_run_sampling_moments(s, beta, therm, freq, S, flags, e);
            if (rc == ISINGMC_OK) rc = isingmc_moments_get(s, &n, site.data(), bonds ? bond.data() : nullptr);
            return rc;
        });
        const double per_site = double(n) * (per_experiment ? 1.0 : double(R));
        for (size_t i = 0; i < site.size(); i++) sp[i] = double(site[i]) / per_site;
        for (size_t k = 0; k < bond.size(); k++) bm[k] = double(bond[k]) / (double(n) * double(R));
        if (bonds) return py::make_tuple(energies, spins, bond_means);
        return py::make_tuple(energies, spins);
    }

    // extension: the classical counterpart of run_quantum_monte_carlo_and_measure_variable_autocorrelation
    // (lattice.rs:628), the variable being the spin.  The trajectory and the bookkeeping of run_monte_carlo_sampling with the same
    // seeds -- sampling_wait_buffer timesteps of thermalisation, then timesteps sweeps with a sample every sampling_freq, S =
    // timesteps / sampling_freq samples -- with every sample compared on the device against the max_lag samples before it: one
    // enqueue-only run and one wait for it (the reads of the sums that follow find the stream idle), no configuration crosses the bus.  Returns C float64[R, L + 1], L = min(max_lag, S - 1),
    // C[r, l] = 1 - 2 diff[r, l] / (N (S - l)) = the average over the S - l sample pairs l samples apart of (1/N) sum_i s_i s_i';
    // lag axis in samples.  connected=True: the per-replica site sums of S18 take the same samples and (1/N) sum_i <s_i>_r^2 is
    // subtracted from every lag but not renormalised, <s_i>_r the mean over the S samples.  That estimate of the squared mean is
    // biased upwards by about tau_int / S per site (the variance of a mean of S correlated samples), so at runs of a few tau the
    // connected function comes out too low by that much at every lag; C(0) is then 1 - (1/N) sum <s_i>^2, not 1.  Sums beyond the
    // option moments_bytes raise that option's error.  One device: the ring lives in one container.  Cluster periods set on this
    // object apply.
    py::array_t<double> run_monte_carlo_and_measure_variable_autocorrelation(double beta, size_t timesteps, size_t num_experiments,
                                                                             std::optional<size_t> sampling_wait_buffer, std::optional<size_t> sampling_freq,
                                                                             size_t max_lag, bool connected)
    {
        require_classical();
        const size_t therm = sampling_wait_buffer.value_or(0), freq = sampling_freq.value_or(1);
        if (freq == 0) throw py::value_error("sampling_freq must be positive");
        if (max_lag < 1 || max_lag > 256) throw py::value_error("max_lag must be 1 .. 256 (the lags a ring holds)");
        if (devices_.size() != 1) throw py::value_error("autocorrelation measurement runs on one device: the ring lives in one container (set_device)");
        const size_t S = timesteps / freq, R = num_experiments, N = E_->nvars;
        if (S < 2) throw py::value_error("an autocorrelation needs at least two samples: timesteps / sampling_freq is below 2");
        const size_t L = std::min(max_lag, S - 1), row = L + 1;
        std::vector<uint64_t> counts(row), diff(R * row);
        std::vector<int64_t> site(connected ? R * N : 0);
        uint64_t n = 0;
        fan_out(num_experiments, 0, R, [&](isingmc_states *s, size_t) {
            AutocorrHandle h; // (the ring goes before the container fan_out destroys)
            int rc = isingmc_autocorr_create(s, L, 0, &h.ac);
            if (rc == ISINGMC_OK) rc = isingmc_run_sampling_autocorr(h.ac, beta, therm, freq, S, connected ? 1 : 0, nullptr);
            if (rc == ISINGMC_OK) rc = isingmc_autocorr_get(h.ac, counts.data(), diff.data());
            if (rc == ISINGMC_OK && connected) rc = isingmc_moments_get(s, &n, site.data(), nullptr);
            return rc;
        });
        py::array_t<double> corr = autocorr_array(counts, diff, R, row, row, N);
        if (connected) {
            double *c = corr.mutable_data();
            for (size_t r = 0; r < R; r++) {
                double m2 = 0.0; // (1/N) sum_i <s_i>_r^2, summed in site order
                for (size_t i = 0; i < N; i++) {
                    const double m = double(site[r * N + i]) / double(n);
                    m2 += m * m;
                }
                m2 /= double(N);
                for (size_t l = 0; l < row; l++) c[r * row + l] -= m2;
            }
        }
        return corr;
    }

    // extension: the sibling of run_monte_carlo_and_measure_spins for the two observables every study starts from.
    // The trajectory and the bookkeeping of run_monte_carlo_sampling with these arguments -- thermalise, then timesteps sweeps with a
    // sample every sampling_freq -- with the energy and the magnetisation of every sample logged on the device: nothing waits per
    // sample and no configuration crosses the bus.  The host waits where the two isingmc_do_time_steps calls end (the thermalisation,
    // then the run: the C ABI has no enqueue-only plain run to put the period's origin behind the thermalisation) and reads the log
    // once.  Returns (energies f64[R, S], magnetisations
    // int64[R, S]), plus by_class int64[R, S, T, K] with class tables as get_overlaps_by_class takes them.  One device: the log
    // lives in one container.  Cluster periods set on this object apply.
    py::tuple run_monte_carlo_and_measure_observables(double beta, size_t timesteps, size_t num_experiments, std::optional<size_t> thermalization_time,
                                                      std::optional<size_t> sampling_freq, const py::object &classes)
    {
        require_classical();
        const size_t therm = thermalization_time.value_or(0), freq = sampling_freq.value_or(1);
        if (freq == 0) throw py::value_error("sampling_freq must be positive");
        if (devices_.size() != 1) throw py::value_error("observable measurement runs on one device: the log lives in one container (set_device)");
        const size_t S = timesteps / freq, R = num_experiments;
        const ClassTables T = classes.is_none() ? ClassTables{} : class_tables(classes, py::none(), E_->nvars);
        const size_t bins = T.n_tables * T.n_classes;
        const std::shared_ptr<GraphHandle> gh = graph(0);
        py::array_t<double> energies(std::vector<ssize_t>{ssize_t(R), ssize_t(S)});
        py::array_t<int64_t> mags(std::vector<ssize_t>{ssize_t(R), ssize_t(S)});
        py::array_t<int64_t> by_class(std::vector<ssize_t>{ssize_t(bins ? R : 0), ssize_t(S), ssize_t(T.n_tables), ssize_t(T.n_classes)});
        double *e = energies.mutable_data();
        int64_t *m = mags.mutable_data(), *c = by_class.mutable_data();
        fan_out(num_experiments, 0, R, [&](isingmc_states *s, size_t) {
            if (S == 0 || R == 0) return isingmc_do_time_steps(s, therm, &beta, 0, nullptr);
            ObsSeriesHandle h; // (the series goes before the class set, and both before the container fan_out destroys)
            int rc = ISINGMC_OK;
            if (bins) rc = isingmc_site_classes_create(gh->g, T.cls.data(), T.n_tables, T.n_classes, &h.classes.c);
            if (rc == ISINGMC_OK) rc = isingmc_observable_series_create(s, h.classes.c, ISINGMC_OBS_ENERGY | ISINGMC_OBS_MAGNETISATION, S, &h.s);
            if (rc == ISINGMC_OK && therm) rc = isingmc_do_time_steps(s, therm, &beta, 0, nullptr);
            if (rc == ISINGMC_OK) rc = isingmc_observable_series_set_every(h.s, freq); // the sample points are counted from here
            if (rc == ISINGMC_OK) rc = isingmc_do_time_steps(s, S * freq, &beta, 0, nullptr);
            std::vector<double> he(S * R);
            std::vector<int64_t> hm(S * R), hc(S * R * bins);
            if (rc == ISINGMC_OK) rc = isingmc_observable_series_get(h.s, 0, S, nullptr, he.data(), hm.data(), bins ? hc.data() : nullptr);
            if (rc != ISINGMC_OK) return rc;
            for (size_t k = 0; k < S; k++) // rows [S][R] -> [R][S]
                for (size_t r = 0; r < R; r++) {
                    e[r * S + k] = he[k * R + r];
                    m[r * S + k] = hm[k * R + r];
                    if (bins) std::copy(hc.begin() + (k * R + r) * bins, hc.begin() + (k * R + r + 1) * bins, c + (r * S + k) * bins);
                }
            return int(ISINGMC_OK);
        });
        if (bins) return py::make_tuple(energies, mags, by_class);
        return py::make_tuple(energies, mags);
    }

    // extension: the improved estimators' raw material.  thermalization_time + timesteps timesteps at beta with the
    // cluster period set on this object (set_cluster_update_every: a column per experiment; set_replica_cluster_update_every: a
    // column per pair), the cluster-size moments of every non-local step logged on the device: one run, one read.  Returns
    // (timesteps uint64[n], n_clusters, largest, sites, s2, s4_lo, s4_hi: uint64[n, C] each) for the steps at timesteps >=
    // thermalization_time.  One device: the log lives in one container.  ValueError with neither period on.
    py::tuple run_monte_carlo_and_measure_clusters(double beta, size_t timesteps, size_t num_experiments, std::optional<size_t> thermalization_time)
    {
        require_classical();
        if (!cluster_every_ && !icm_every_)
            throw py::value_error("no cluster period is on: set_cluster_update_every(k) or set_replica_cluster_update_every(k) first (neither is set)");
        if (devices_.size() != 1) throw py::value_error("cluster measurement runs on one device: the log lives in one container (set_device)");
        const size_t therm = thermalization_time.value_or(0), total = therm + timesteps, k = cluster_every_ ? cluster_every_ : icm_every_;
        const int kind = cluster_every_ ? ISINGMC_CLUSTER_SERIES_SW : ISINGMC_CLUSTER_SERIES_ICM;
        const size_t columns = cluster_every_ ? num_experiments : num_experiments / 2;
        uint64_t steps = 0;
        check(isingmc_host_nonlocal_steps(0, total, k, &steps));
        std::vector<uint64_t> t(steps), rows(size_t(steps) * columns * 6);
        fan_out(num_experiments, 0, num_experiments, [&](isingmc_states *s, size_t) {
            ClusterSeriesHandle h; // (the series goes before the container fan_out destroys)
            int rc = isingmc_cluster_series_create(s, kind, std::max<size_t>(1, size_t(steps)), &h.s);
            if (rc == ISINGMC_OK) rc = isingmc_do_time_steps(s, total, &beta, 0, nullptr);
            if (rc == ISINGMC_OK) rc = isingmc_cluster_series_get(h.s, 0, size_t(steps), t.data(), rows.data());
            return rc;
        });
        return cluster_series_rows(t, rows, columns, therm);
    }

    // lattice.rs:309-385
    py::tuple run_monte_carlo_annealing(const std::vector<std::pair<size_t, double>> &betas, size_t timesteps,
                                        size_t num_experiments, std::optional<bool>, std::optional<bool>,
                                        Range replica_range)
    {
        require_classical();
        const std::vector<double> schedule = expand(betas, timesteps);
        const auto [lo, hi] = bounds(num_experiments, replica_range);
        const size_t R = hi - lo, N = E_->nvars;
        py::array_t<double> energies(std::vector<ssize_t>{ssize_t(R)});
        py::array_t<bool> states(std::vector<ssize_t>{ssize_t(R), ssize_t(N)});
        double *e = energies.mutable_data();
        uint8_t *st = reinterpret_cast<uint8_t *>(states.mutable_data());
        fan_out(num_experiments, lo, hi, [&](isingmc_states *s, size_t off) {
            int rc = isingmc_do_time_steps(s, timesteps, schedule.data(), 1, nullptr);
            if (rc == ISINGMC_OK) rc = isingmc_get_energies(s, e + off);
            if (rc == ISINGMC_OK) rc = isingmc_get_states(s, st + off * N, N);
            return rc;
        });
        return py::make_tuple(energies, states);
    }

    // lattice.rs:395-470
    py::tuple run_monte_carlo_annealing_and_get_energies(const std::vector<std::pair<size_t, double>> &betas,
                                                         size_t timesteps, size_t num_experiments,
                                                         std::optional<bool>, std::optional<bool>, Range replica_range)
    {
        require_classical();
        const std::vector<double> schedule = expand(betas, timesteps);
        const auto [lo, hi] = bounds(num_experiments, replica_range);
        const size_t R = hi - lo, N = E_->nvars;
        py::array_t<double> energies(std::vector<ssize_t>{ssize_t(R), ssize_t(timesteps)});
        py::array_t<bool> states(std::vector<ssize_t>{ssize_t(R), ssize_t(N)});
        double *e = energies.mutable_data();
        uint8_t *st = reinterpret_cast<uint8_t *>(states.mutable_data());
        fan_out(num_experiments, lo, hi, [&](isingmc_states *s, size_t off) {
            int rc = isingmc_do_time_steps(s, timesteps, schedule.data(), 1, e + off * timesteps);
            if (rc == ISINGMC_OK) rc = isingmc_get_states(s, st + off * N, N);
            return rc;
        });
        return py::make_tuple(energies, states);
    }

    // extension: the annealing run of run_monte_carlo_annealing with every experiment's lowest-energy configuration
    // kept on the device: an update of the records follows every timestep after which t % every == 0 (isingmc_states_set_track_best).
    // Returns (min_energies f64[R], min_states bool[R, N], min_timesteps uint64[R]); cluster periods set on this object apply.
    // One device: the records live in one container.
    py::tuple run_monte_carlo_annealing_and_get_minimum(const std::vector<std::pair<size_t, double>> &betas, size_t timesteps,
                                                        size_t num_experiments, size_t every, std::optional<bool>)
    {
        require_classical();
        if (every == 0) throw py::value_error("every must be positive: an update of the records follows every timestep after which t % every == 0");
        if (devices_.size() != 1) throw py::value_error("minimum tracking runs on one device: the records live in one container (set_device)");
        const std::vector<double> schedule = expand(betas, timesteps);
        const size_t R = num_experiments, N = E_->nvars;
        py::array_t<double> energies(std::vector<ssize_t>{ssize_t(R)});
        py::array_t<bool> states(std::vector<ssize_t>{ssize_t(R), ssize_t(N)});
        py::array_t<uint64_t> steps(std::vector<ssize_t>{ssize_t(R)});
        double *e = energies.mutable_data();
        uint8_t *st = reinterpret_cast<uint8_t *>(states.mutable_data());
        uint64_t *ts = steps.mutable_data();
        fan_out(num_experiments, 0, R, [&](isingmc_states *s, size_t) {
            int rc = isingmc_states_set_track_best(s, every);
            if (rc == ISINGMC_OK) rc = isingmc_do_time_steps(s, timesteps, schedule.data(), 1, nullptr);
            if (rc == ISINGMC_OK) rc = isingmc_best_get(s, e, st, N, ts, nullptr);
            return rc;
        });
        return py::make_tuple(energies, states, steps);
    }

    // the schedule of a population-annealing run as it was taken, with the record of every resampling (one fewer than betas)
    struct PaLog {
        std::vector<double> betas, erefs, mean;
        std::vector<uint64_t> sums, distinct;
    };

    // What the two population-annealing entry points share: the refusals (check_schedule: those of the caller's own arguments, in
    // their place among them), the container, the schedule `run` drives on it (keyed by the last of make_seeds(population + 1))
    // and the read-out of the final population.
    template <typename Check, typename Run>
    py::object population_annealing(const Check &check_schedule, const Run &run, size_t sweeps_per_beta, size_t population, bool return_states, bool measure_overlaps,
                                    bool track_minimum, const py::object &overlap_classes)
    {
        require_classical();
        if (!overlap_classes.is_none() && !measure_overlaps)
            throw py::value_error("overlap_classes resolves the overlaps of measure_overlaps=True by site class: it needs measure_overlaps");
        const ClassTables classes = overlap_classes.is_none() ? ClassTables{} : class_tables(overlap_classes, py::none(), E_->nvars);
        check_schedule();
        if (population == 0) throw py::value_error("population must be positive");
        if (sweeps_per_beta == 0) throw py::value_error("sweeps_per_beta must be positive");
        if (devices_.size() != 1) throw py::value_error("population annealing runs on one device: one population lives in one container (set_device)");
        const size_t R = population, N = E_->nvars;
        const std::vector<uint64_t> seeds = make_seeds(R + 1);
        const std::shared_ptr<GraphHandle> gh = graph(0);
        py::array_t<double> energies(std::vector<ssize_t>{ssize_t(R)});
        py::array_t<bool> states(std::vector<ssize_t>{ssize_t(return_states ? R : 0), ssize_t(N)});
        PaLog log;
        py::array_t<uint32_t> families(std::vector<ssize_t>{ssize_t(R)});
        double *e = energies.mutable_data();
        uint32_t *fam = families.mutable_data();
        uint8_t *st = reinterpret_cast<uint8_t *>(states.mutable_data());
        const size_t n_ovl = measure_overlaps ? R / 2 : 0;
        py::array_t<int64_t> ovl_pairs(std::vector<ssize_t>{ssize_t(n_ovl), 2}), ovl_spin(std::vector<ssize_t>{ssize_t(n_ovl)}),
            ovl_link(std::vector<ssize_t>{ssize_t(n_ovl)});
        int64_t *op = ovl_pairs.mutable_data(), *os = ovl_spin.mutable_data(), *ol = ovl_link.mutable_data();
        py::array_t<int64_t> ovl_class(std::vector<ssize_t>{ssize_t(classes.n_tables ? n_ovl : 0), ssize_t(classes.n_tables), ssize_t(classes.n_classes)});
        int64_t *oc = ovl_class.mutable_data();
        py::array_t<bool> min_state(std::vector<ssize_t>{ssize_t(track_minimum ? N : 0)});
        uint8_t *mst = reinterpret_cast<uint8_t *>(min_state.mutable_data());
        double min_energy = std::numeric_limits<double>::infinity();
        uint64_t min_t = 0;
        int rc = ISINGMC_OK;
        std::string msg;
        {
            py::gil_scoped_release nogil;
            StatesHandle h;
            h.graph = gh;
            const uint8_t *ini = initial_state_.empty() ? nullptr : initial_state_.data();
            rc = isingmc_states_create(gh->g, R, seeds.data(), ini, &h.s);
            if (rc == ISINGMC_OK) rc = apply_rng_rounds(h.s);
            if (rc == ISINGMC_OK && cluster_every_) rc = isingmc_states_set_cluster_every(h.s, cluster_every_);
            if (rc == ISINGMC_OK && icm_every_) rc = isingmc_states_set_icm_every(h.s, icm_every_);
            // the update points are the resamplings and the end of the run: a period no timestep reaches leaves the sweeps uncut
            if (rc == ISINGMC_OK && track_minimum) rc = isingmc_states_set_track_best(h.s, size_t(1) << 62);
            if (rc == ISINGMC_OK) rc = run(h.s, seeds[R], log);
            if (rc == ISINGMC_OK) rc = isingmc_get_energies(h.s, e);
            if (rc == ISINGMC_OK && return_states) rc = isingmc_get_states(h.s, st, N);
            if (rc == ISINGMC_OK) rc = isingmc_pa_families(h.s, fam);
            if (rc == ISINGMC_OK && n_ovl) {
                std::vector<uint32_t> sa(n_ovl), sb(n_ovl);
                for (size_t p = 0; p < n_ovl; p++) {
                    op[2 * p] = int64_t(sa[p] = uint32_t(p));
                    op[2 * p + 1] = int64_t(sb[p] = uint32_t(p + n_ovl));
                }
                rc = isingmc_overlaps(h.s, nullptr, sa.data(), sb.data(), n_ovl, os, ol);
                if (rc == ISINGMC_OK && classes.n_tables) {
                    ClassesHandle ch;
                    rc = isingmc_site_classes_create(gh->g, classes.cls.data(), classes.n_tables, classes.n_classes, &ch.c);
                    if (rc == ISINGMC_OK) rc = isingmc_overlaps_by_class(h.s, nullptr, sa.data(), sb.data(), n_ovl, ch.c, oc);
                    if (rc != ISINGMC_OK) msg = isingmc_last_error(); // (before the handle's destructor calls into the library again)
                }
            }
            if (rc == ISINGMC_OK && track_minimum) { // the population's minimum: the first slot with the lowest record
                std::vector<double> be(R);
                std::vector<uint64_t> bt(R);
                std::vector<uint8_t> bs(R * N);
                rc = isingmc_best_get(h.s, be.data(), bs.data(), N, bt.data(), nullptr);
                size_t arg = 0;
                for (size_t r = 1; r < R && rc == ISINGMC_OK; r++)
                    if (be[r] < be[arg]) arg = r;
                if (rc == ISINGMC_OK) {
                    min_energy = be[arg];
                    min_t = bt[arg];
                    std::copy(bs.begin() + arg * N, bs.begin() + (arg + 1) * N, mst);
                }
            }
            if (rc != ISINGMC_OK && msg.empty()) msg = isingmc_last_error();
        }
        if (rc == ISINGMC_ERR_INVALID) throw py::value_error(msg);
        if (rc == ISINGMC_ERR_ALLOC) throw std::bad_alloc();
        if (rc != ISINGMC_OK) throw std::runtime_error(msg);
        const std::vector<double> &betas = log.betas;
        const size_t n = betas.size();
        py::array_t<double> log_z(std::vector<ssize_t>{ssize_t(n)}), mean_e(std::vector<ssize_t>{ssize_t(n)});
        py::array_t<int64_t> distinct(std::vector<ssize_t>{ssize_t(n - 1)});
        double *lz = log_z.mutable_data(), *me = mean_e.mutable_data();
        int64_t *ds = distinct.mutable_data();
        lz[0] = 0.0;
        for (size_t k = 1; k < n; k++) {
            // ln Q = ln(S / (R 2^32)) - dbeta E_ref estimates ln Z(betas[k]) - ln Z(betas[k - 1])
            const double dbeta = betas[k] - betas[k - 1];
            lz[k] = lz[k - 1] + (std::log(std::ldexp(double(log.sums[k - 1]), -32) / double(R)) - dbeta * log.erefs[k - 1]);
            ds[k - 1] = int64_t(log.distinct[k - 1]);
            me[k - 1] = log.mean[k - 1];
        }
        double sum_e = 0.0, rho = 0.0;
        for (size_t r = 0; r < R; r++) sum_e += e[r];
        me[n - 1] = sum_e / double(R); // the final measurement
        std::vector<uint32_t> count(R, 0u);
        for (size_t r = 0; r < R; r++) count[fam[r]]++;
        for (size_t f = 0; f < R; f++) rho += double(count[f]) * double(count[f]);
        rho /= double(R); // rho_t = R sum_f (n_f / R)^2
        py::dict d;
        d["energies"] = energies;
        d["states"] = return_states ? py::object(states) : py::object(py::none());
        d["log_z_ratio"] = log_z;
        d["mean_energy"] = mean_e;
        d["distinct_sources"] = distinct;
        d["families"] = families;
        d["rho_t"] = rho;
        d["betas"] = py::array_t<double>(ssize_t(n), betas.data());
        if (measure_overlaps) {
            d["overlap_pairs"] = ovl_pairs;
            d["spin_overlaps"] = ovl_spin;
            d["link_overlaps"] = ovl_link;
            if (classes.n_tables) d["overlaps_by_class"] = ovl_class;
        }
        if (track_minimum) {
            d["min_energy"] = min_energy;
            d["min_state"] = min_state;
            // a record set at timestep t (t = k sweeps_per_beta at the resampling before beta k, n sweeps_per_beta at the end) was
            // produced by the sweeps at beta ceil(t / sweeps_per_beta) - 1
            d["min_beta_index"] = min_t ? (min_t + sweeps_per_beta - 1) / sweeps_per_beta - 1 : size_t(0);
        }
        return py::module_::import("types").attr("SimpleNamespace")(**d);
    }

    // extension: population annealing.  `population` replicas are cooled through the non-decreasing `betas`:
    // before the sweeps at betas[k], k > 0, the population is resampled on the device for the step betas[k] - betas[k - 1]
    // (isingmc_pa_resample, step counter k, keyed by the LAST of make_seeds(population + 1); the first `population` seeds key the
    // replicas); then sweeps_per_beta timesteps at betas[k] (cluster periods set on this object apply).  One library call
    // (isingmc_pa_run) enqueues it all; nothing waits on the host until the end.
    // measure_overlaps: the result also carries the spin and link overlaps of the final population between the
    // replicas (p, p + R / 2) (isingmc_overlaps); pairs of one family are the caller's to drop.
    // overlap_classes (needs measure_overlaps): class tables, one array of nvars classes or a stack of them; the
    // result also carries overlaps_by_class, int64[R / 2, n_tables, n_classes] for the same pairs (isingmc_overlaps_by_class).
    // track_minimum: every SLOT keeps the lowest-energy configuration that ever sat in it, seen before every
    // resampling and after the last sweeps; the result carries the population's minimum over the slots as min_energy, min_state
    // and min_beta_index (the index of the beta whose sweeps produced it).
    py::object run_population_annealing(const std::vector<double> &betas, size_t sweeps_per_beta, size_t population, bool return_states,
                                        bool measure_overlaps, bool track_minimum, const py::object &overlap_classes)
    {
        const auto check = [&] {
            if (betas.empty()) throw py::value_error("betas must hold at least one inverse temperature");
            for (size_t k = 0; k < betas.size(); k++)
                if (!std::isfinite(betas[k]) || (k && betas[k] < betas[k - 1])) throw py::value_error("betas must be finite and non-decreasing");
        };
        // the whole schedule is enqueued; the host waits once, at its end, and reads the step records
        const auto run = [&](isingmc_states *s, uint64_t seed, PaLog &log) {
            const size_t n = betas.size();
            log.betas = betas;
            log.sums.resize(n - 1); log.erefs.resize(n - 1); log.distinct.resize(n - 1); log.mean.resize(n - 1);
            return isingmc_pa_run(s, betas.data(), n, sweeps_per_beta, seed, log.sums.data(), log.erefs.data(), log.distinct.data(), log.mean.data());
        };
        return population_annealing(check, run, sweeps_per_beta, population, return_states, measure_overlaps, track_minimum, overlap_classes);
    }

    // extension: population annealing from beta_start up to beta_end with the temperature steps chosen on the device
    // from the population itself (isingmc_pa_run_adaptive): the largest step, of at most max_dbeta (None: no cap), at which the
    // energy histograms of the two temperatures still overlap by target_overlap.  0.85 is the value customary in the literature, a
    // default and not a measured optimum.  The result is that of run_population_annealing; its `betas` is the schedule that was
    // taken, which log_z_ratio, mean_energy and distinct_sources are indexed by.  The host waits once per temperature.  ValueError
    // if max_steps steps do not reach beta_end.
    py::object run_population_annealing_adaptive(double beta_start, double beta_end, size_t sweeps_per_beta, size_t population, double target_overlap,
                                                 std::optional<double> max_dbeta, size_t max_steps, bool return_states, bool measure_overlaps,
                                                 bool track_minimum, const py::object &overlap_classes)
    {
        const auto check = [&] {
            if (!std::isfinite(beta_start) || !std::isfinite(beta_end) || beta_end < beta_start)
                throw py::value_error("beta_start and beta_end must be finite with beta_start <= beta_end");
            if (max_steps >= (size_t(1) << 32)) throw py::value_error("max_steps must be below 2^32");
        };
        const auto run = [&](isingmc_states *s, uint64_t seed, PaLog &log) {
            log.betas.resize(max_steps + 1);
            log.sums.resize(max_steps); log.erefs.resize(max_steps); log.distinct.resize(max_steps); log.mean.resize(max_steps);
            size_t n = 0;
            const int rc = isingmc_pa_run_adaptive(s, beta_start, beta_end, sweeps_per_beta, seed, target_overlap,
                                                   max_dbeta ? *max_dbeta : std::numeric_limits<double>::infinity(), max_steps, log.betas.data(), &n,
                                                   log.sums.data(), log.erefs.data(), log.distinct.data(), log.mean.data());
            n = std::max<size_t>(n, 1);
            log.betas.resize(n);
            log.sums.resize(n - 1); log.erefs.resize(n - 1); log.distinct.resize(n - 1); log.mean.resize(n - 1);
            return rc;
        };
        return population_annealing(check, run, sweeps_per_beta, population, return_states, measure_overlaps, track_minimum, overlap_classes);
    }

    Lattice clone() const { return *this; } // lattice.rs:1038-1040 (the immutable device graph is shared)

    static void sample_into(isingmc_states *s, double beta, size_t therm, size_t freq, size_t S, size_t, size_t,
                            double *energies, uint8_t *states)
    {
        // lattice.rs:271-287: thermalise, then S x { freq steps; record state + energy } -- one library call,
        // enqueued end to end on the device stream
        check(isingmc_run_sampling(s, beta, therm, freq, S, energies, states));
    }

private:
    Lattice() = default;

    void require_classical() const
    {
        if (transverse_) // lattice.rs:217-219
            throw py::value_error("Cannot run classic monte carlo with transverse field");
    }

    // one graph per entry of the device list, built on first use (the first one serves engine_info)
    std::shared_ptr<GraphHandle> graph(size_t slot = 0)
    {
        if (graphs_.size() != devices_.size()) graphs_.assign(devices_.size(), nullptr);
        if (!graphs_[slot]) {
            std::vector<double> b;
            const std::vector<double> *bp = nullptr;
            if (!biases_.empty()) bp = &biases_;
            else if (global_bias_ != 0.0) { b.assign(E_->nvars, global_bias_); bp = &b; } // lattice.rs:186-189
            graphs_[slot] = make_graph(*E_, bp, devices_[slot], force_general_, stable_path_);
        }
        return graphs_[slot];
    }

    static std::pair<size_t, size_t> bounds(size_t num_experiments, const Range &range)
    {
        if (!range) return {0, num_experiments};
        if (range->first > range->second || range->second > num_experiments) throw py::value_error("replica_range out of bounds");
        return {range->first, range->second};
    }

    // The rayon fan-out of lattice.rs:192-197, over devices: experiments [lo, hi) are cut into contiguous blocks,
    // one per entry of the device list (ISINGMC_DEVICES / set_devices; aligned to 32 experiments once a block
    // holds that many), and every block runs on its device from a host thread of its own:
    //   seed -> rng; GraphState::new; set_state(initial)  (lattice.rs:198-203) = isingmc_states_create_range,
    // then body(states, offset of the block in the output arrays).  Philox keys, replica groups and the path
    // choice follow the GLOBAL experiment index, so the arrays do not depend on the device list.
    template <typename Body>
    void fan_out(size_t num_experiments, size_t lo, size_t hi, Body &&body)
    {
        const std::vector<uint64_t> seeds = make_seeds(num_experiments);
        const size_t n = hi - lo, D = devices_.size();
        size_t per = (n + D - 1) / std::max<size_t>(D, 1);
        if (per >= 32) per = (per + 31) / 32 * 32;
        if (icm_every_) { // pairs are (2 p, 2 p + 1) of the global experiment index: no device cut may split one
            if (lo % 2) throw py::value_error("replica_range must start at an even experiment with replica cluster updates on: experiments (2p, 2p + 1) form a pair");
            per += per % 2;
        }
        struct Block { size_t slot, lo, hi; int rc = ISINGMC_OK; std::string msg; };
        std::vector<Block> blocks;
        for (size_t d = 0; d < D; d++) {
            const size_t b = std::min(hi, lo + d * per), e = std::min(hi, b + per);
            if (e > b || (d == 0 && n == 0)) blocks.push_back({d, b, e});
        }
        for (const Block &blk : blocks) (void)graph(blk.slot); // may raise: with the GIL, before any thread starts
        const uint8_t *ini = initial_state_.empty() ? nullptr : initial_state_.data();
        const auto run_block = [&](Block &blk) {
            isingmc_states *st = nullptr;
            blk.rc = isingmc_states_create_range(graphs_[blk.slot]->g, num_experiments, seeds.data(), blk.lo, blk.hi - blk.lo, ini, &st);
            if (blk.rc == ISINGMC_OK) blk.rc = apply_rng_rounds(st);
            if (blk.rc == ISINGMC_OK && cluster_every_) blk.rc = isingmc_states_set_cluster_every(st, cluster_every_);
            if (blk.rc == ISINGMC_OK && icm_every_) blk.rc = isingmc_states_set_icm_every(st, icm_every_);
            if (blk.rc == ISINGMC_OK) blk.rc = body(st, blk.lo - lo);
            if (blk.rc != ISINGMC_OK) blk.msg = isingmc_last_error(); // per thread: read it where it was set
            isingmc_states_destroy(st);
        };
        {
            py::gil_scoped_release nogil;
            if (blocks.size() == 1) run_block(blocks[0]);
            else {
                std::vector<std::thread> pool;
                for (Block &blk : blocks) pool.emplace_back([&run_block, &blk] { run_block(blk); });
                for (auto &th : pool) th.join();
            }
        }
        for (const Block &blk : blocks) {
            if (blk.rc == ISINGMC_OK) continue;
            if (blk.rc == ISINGMC_ERR_INVALID) throw py::value_error(blk.msg);
            if (blk.rc == ISINGMC_ERR_ALLOC) throw std::bad_alloc();
            throw std::runtime_error(blk.msg);
        }
    }

    static std::vector<double> expand(const std::vector<std::pair<size_t, double>> &betas, size_t timesteps)
    {
        std::vector<uint64_t> t;
        std::vector<double> b;
        for (const auto &s : betas) { t.push_back(s.first); b.push_back(s.second); }
        std::vector<double> out(timesteps);
        check(isingmc_host_expand_schedule(t.data(), b.data(), t.size(), timesteps, compat_anneal_bug(), out.data()));
        return out;
    }

    std::shared_ptr<EdgeArrays> E_;
    std::vector<double> biases_; // empty = BiasType::Global(global_bias_)
    double global_bias_ = 0.0;
    std::optional<double> transverse_;
    std::vector<uint8_t> initial_state_;
    bool enable_rvb_ = false, enable_heatbath_ = false;
    std::optional<uint64_t> seed_gen_;
    bool use_allocator_ = true;
    std::vector<int> devices_;  // one block of experiments per entry (ISINGMC_DEVICES; an ordinal may repeat)
    bool force_general_ = false, stable_path_ = false;
    size_t cluster_every_ = 0, icm_every_ = 0;
    std::optional<int> rng_rounds_; // set_rng_rounds
    std::vector<std::shared_ptr<GraphHandle>> graphs_;
};

// ------------------------------------------------------------------------------------------------
// ClassicIsing (src/classicising.rs:11-180): replicas persist on the device between calls
// ------------------------------------------------------------------------------------------------
class ClassicIsing {
public:
    ClassicIsing(const py::object &edges, std::optional<double> longitudinal,
                 std::optional<size_t> num_experiments, std::optional<uint64_t> seed, std::optional<bool> use_basic_moves)
        : E_(split_edges(edges)), longitudinal_(longitudinal.value_or(0.0)),
          use_basic_moves_(use_basic_moves.value_or(false))
    {
        // the reference unwraps None here and aborts the process (classicising.rs:34-39)
        if (E_.a.empty()) throw py::value_error("Must supply some edges for graph");
        if (seed) master_seed_ = *seed;
        else check(isingmc_host_make_seeds(0, 0, 1, &master_seed_)); // SmallRng::from_entropy()
        std::vector<double> bias;
        if (longitudinal_ != 0.0) bias.assign(E_.nvars, longitudinal_); // classicising.rs:69
        graph_ = make_graph(E_, bias.empty() ? nullptr : &bias, default_device(), false);
        st_ = std::make_shared<StatesHandle>();
        st_->graph = graph_;
        // all experiments of the constructor at once (seed i = the i-th draw of the container's rng, as add_graph would
        // draw them one by one): the library picks its path from the count and the graph size -- a graph that is not a
        // recognised lattice usually runs on the replica-packed kernels (isingmc.hip packed_worth_it) -- and later add_graph calls grow that container
        const size_t n = num_experiments.value_or(1);
        drawn_.resize(n);
        check(isingmc_host_make_seeds(1, master_seed_, n, drawn_.data()));
        check(isingmc_states_create(graph_->g, n, drawn_.data(), nullptr, &st_->s));
    }

    // classicising.rs:62-79: seed = self.rng.gen(); GraphState::new / new_with_state_and_rng
    void add_graph(std::optional<std::vector<bool>> initial_state, std::optional<bool>)
    {
        std::vector<uint8_t> ini;
        if (initial_state) {
            if (initial_state->size() != E_.nvars)
                throw py::value_error("Initial state must be of the same size as biases, or 0.");
            ini = to_bytes(*initial_state);
        }
        drawn_.resize(drawn_.size() + 1);
        check(isingmc_host_make_seeds(1, master_seed_, drawn_.size(), drawn_.data())); // n-th draw of the master rng
        py::gil_scoped_release nogil;
        check(isingmc_states_append(st_->s, drawn_.back(), initial_state ? ini.data() : nullptr));
    }

    // classicising.rs:88-110
    void run_monte_carlo(double beta, size_t timesteps, std::optional<size_t> nspinupdates, std::optional<size_t>,
                         std::optional<size_t>, std::optional<bool>)
    {
        const size_t sweeps = sweeps_for(timesteps, nspinupdates);
        py::gil_scoped_release nogil;
        check(isingmc_do_time_steps(st_->s, sweeps, &beta, 0, nullptr));
    }

    // classicising.rs:119-179
    py::tuple run_monte_carlo_sampling(double beta, size_t timesteps, std::optional<size_t> nspinupdates,
                                       std::optional<size_t>, std::optional<size_t>, std::optional<bool>,
                                       std::optional<size_t> thermalization_time, std::optional<size_t> sampling_freq)
    {
        const size_t therm = thermalization_time.value_or(0), freq = sampling_freq.value_or(1);
        if (freq == 0) throw py::value_error("sampling_freq must be positive");
        const size_t S = timesteps / freq, R = isingmc_states_count(st_->s), N = E_.nvars;
        py::array_t<double> energies(std::vector<ssize_t>{ssize_t(R), ssize_t(S)});
        py::array_t<bool> states(std::vector<ssize_t>{ssize_t(R), ssize_t(S), ssize_t(N)});
        if (whole_sweeps(nspinupdates)) { // every timestep is made of whole sweeps: one pipelined library call
            const size_t mult = nspinupdates ? *nspinupdates / N : 1;
            double *e_out = energies.mutable_data();
            uint8_t *s_out = reinterpret_cast<uint8_t *>(states.mutable_data());
            {
                py::gil_scoped_release nogil;
                Lattice::sample_into(st_->s, beta, therm * mult, freq * mult, S, R, N, e_out, s_out);
            }
            return py::make_tuple(energies, states);
        }
        // attempts per timestep that are not whole sweeps: the blocks between samples hold varying numbers of sweeps
        std::vector<size_t> block(S + 1);
        block[0] = sweeps_for(therm, nspinupdates);
        for (size_t k = 0; k < S; k++) block[k + 1] = sweeps_for(freq, nspinupdates);
        double *e = energies.mutable_data();
        uint8_t *st = reinterpret_cast<uint8_t *>(states.mutable_data());
        {
            py::gil_scoped_release nogil;
            std::vector<double> e_k(R);
            check(isingmc_do_time_steps(st_->s, block[0], &beta, 0, nullptr));
            for (size_t k = 0; k < S; k++) {
                check(isingmc_do_time_steps(st_->s, block[k + 1], &beta, 0, nullptr));
                check(isingmc_get_energies(st_->s, e_k.data()));
                for (size_t r = 0; r < R; r++) e[r * S + k] = e_k[r];
                if (R) check(isingmc_get_states(st_->s, st + k * N, S * N)); // replica r's sample k sits at (r S + k) N
            }
        }
        return py::make_tuple(energies, states);
    }

    // extensions: read the persistent replicas without advancing them
    py::array_t<double> get_energies()
    {
        py::array_t<double> e(std::vector<ssize_t>{ssize_t(isingmc_states_count(st_->s))});
        check(isingmc_get_energies(st_->s, e.mutable_data()));
        return e;
    }
    py::array_t<bool> get_states()
    {
        py::array_t<bool> s(std::vector<ssize_t>{ssize_t(isingmc_states_count(st_->s)), ssize_t(E_.nvars)});
        check(isingmc_get_states(st_->s, reinterpret_cast<uint8_t *>(s.mutable_data()), E_.nvars));
        return s;
    }
    size_t get_num_graphs() const { return isingmc_states_count(st_->s); }
    // extension: the rounds of Philox4x32 in the sweeps' draws of the persistent replicas, 10 or 7, from the next call
    // on; ValueError where the option "philox_rounds" refuses (another value, or 7 on a family it does not serve)
    void set_rng_rounds(int rounds) { check(isingmc_states_set_option(st_->s, "philox_rounds", rounds)); }
    int get_rng_rounds() const
    {
        int rounds = 10;
        check(isingmc_states_philox_rounds(st_->s, &rounds));
        return rounds;
    }
    // extension: spin and link overlaps between the persistent replicas, exact integers counted on the device.
    // pairs: None = the replicas (2 p, 2 p + 1), or an integer [n, 2] array of graph indices.  Returns (spin, link) as int64[n]
    // (link = None when not asked for); ValueError where isingmc_overlaps refuses.
    py::tuple get_overlaps(const py::object &pairs, bool link)
    {
        std::vector<uint32_t> sa, sb;
        const size_t n = overlap_pairs(pairs, sa, sb);
        py::array_t<int64_t> spin(std::vector<ssize_t>{ssize_t(n)}), lnk(std::vector<ssize_t>{ssize_t(link ? n : 0)});
        int64_t *s_out = spin.mutable_data(), *l_out = link ? lnk.mutable_data() : nullptr;
        {
            py::gil_scoped_release nogil;
            check(isingmc_overlaps(st_->s, nullptr, pairs_ptr(sa), pairs_ptr(sb), n, s_out, l_out));
        }
        return py::make_tuple(spin, link ? py::object(lnk) : py::object(py::none()));
    }
    // extension: the spin overlap between the persistent replicas resolved by site class.  classes: one integer
    // array of nvars classes or a stack [n_tables, nvars] (NO_CLASS = 0xFFFFFFFF: counted nowhere); n_classes: None = the largest
    // class + 1; pairs as get_overlaps takes them.  Returns int64[n, n_tables, n_classes]; ValueError where the library refuses.
    py::array_t<int64_t> get_overlaps_by_class(const py::object &classes, const py::object &n_classes, const py::object &pairs)
    {
        const ClassTables T = class_tables(classes, n_classes, E_.nvars);
        std::vector<uint32_t> sa, sb;
        const size_t n = overlap_pairs(pairs, sa, sb);
        py::array_t<int64_t> out(std::vector<ssize_t>{ssize_t(n), ssize_t(T.n_tables), ssize_t(T.n_classes)});
        int64_t *o = out.mutable_data();
        {
            py::gil_scoped_release nogil;
            ClassesHandle ch;
            check(isingmc_site_classes_create(st_->graph->g, T.cls.data(), T.n_tables, T.n_classes, &ch.c));
            check(isingmc_overlaps_by_class(st_->s, nullptr, pairs_ptr(sa), pairs_ptr(sb), n, ch.c, o));
        }
        return out;
    }
    // extension: every persistent replica's lowest-energy configuration, kept on the device.
    // set_track_minimum(every): an update of the records follows every timestep after which t % every == 0 (0: off); add_graph is
    // refused while it is on.  get_minimum() -> (energies f64[R], states bool[R, N], timesteps uint64[R], improvements);
    // reset_minimum() sets the records back to +inf.  ValueError where isingmc_states_set_track_best refuses.
    void set_track_minimum(size_t every) { check(isingmc_states_set_track_best(st_->s, every)); }
    py::tuple get_minimum()
    {
        const size_t R = isingmc_states_count(st_->s), N = E_.nvars;
        py::array_t<double> e(std::vector<ssize_t>{ssize_t(R)});
        py::array_t<bool> s(std::vector<ssize_t>{ssize_t(R), ssize_t(N)});
        py::array_t<uint64_t> t(std::vector<ssize_t>{ssize_t(R)});
        uint64_t improvements = 0;
        double *e_out = e.mutable_data();
        uint8_t *s_out = reinterpret_cast<uint8_t *>(s.mutable_data());
        uint64_t *t_out = t.mutable_data();
        {
            py::gil_scoped_release nogil;
            check(isingmc_best_get(st_->s, e_out, s_out, N, t_out, &improvements));
        }
        return py::make_tuple(e, s, t, improvements);
    }
    void reset_minimum() { check(isingmc_best_reset(st_->s)); }
    // extension: per-site spin sums (and per-bond sums) over the samples of the persistent replicas' runs.
    // set_measure_spins_every(k): a sample of all replicas follows every k-th timestep from now on (0: off, the sums stay); add_graph
    // is refused while it is on.  get_measured_spins() -> (n, spins int64[N] or int64[R, N], bonds int64[n_edges] or None): the raw
    // integer sums, True = +1, and the number of samples in them.  ValueError where isingmc_states_set_moments_every refuses.
    void set_measure_spins_every(size_t k, bool per_experiment, bool bonds)
    {
        check(isingmc_states_set_moments_every(st_->s, k, (per_experiment ? ISINGMC_MOMENTS_PER_REPLICA : 0u) | (bonds ? ISINGMC_MOMENTS_BONDS : 0u)));
    }
    py::tuple get_measured_spins()
    {
        size_t every = 0;
        unsigned flags = 0;
        check(isingmc_states_moments_every(st_->s, &every, &flags));
        const bool per = flags & ISINGMC_MOMENTS_PER_REPLICA, bonds = flags & ISINGMC_MOMENTS_BONDS;
        const size_t R = isingmc_states_count(st_->s), N = E_.nvars;
        py::array_t<int64_t> site(per ? std::vector<ssize_t>{ssize_t(R), ssize_t(N)} : std::vector<ssize_t>{ssize_t(N)});
        py::array_t<int64_t> bond(std::vector<ssize_t>{ssize_t(bonds ? E_.a.size() : 0)});
        int64_t *s_out = site.mutable_data(), *b_out = bonds ? bond.mutable_data() : nullptr;
        uint64_t n = 0;
        {
            py::gil_scoped_release nogil;
            check(isingmc_moments_get(st_->s, &n, s_out, b_out));
        }
        return py::make_tuple(n, site, bonds ? py::object(bond) : py::object(py::none()));
    }
    void reset_measured_spins() { check(isingmc_moments_reset(st_->s)); }
    // the handle of a new series over `columns` columns, with the class set made from the caller's tables (None: no class set)
    template <typename H>
    std::unique_ptr<H> series_handle(const py::object &classes, size_t columns)
    {
        auto h = std::make_unique<H>();
        h->columns = columns;
        if (classes.is_none()) return h;
        const ClassTables T = class_tables(classes, py::none(), E_.nvars);
        check(isingmc_site_classes_create(st_->graph->g, T.cls.data(), T.n_tables, T.n_classes, &h->classes.c));
        h->n_tables = T.n_tables;
        h->n_classes = T.n_classes;
        return h;
    }
    // extension: the overlaps between the persistent replicas (2 p, 2 p + 1), logged on the device once per sample.
    // set_measure_overlaps_every(k, link, classes, capacity): a row follows every k-th timestep from now on, without the host
    // waiting (0: off, the rows stay); a call with k > 0 starts a new log of `capacity` rows.  classes: class tables as
    // get_overlaps_by_class takes them, or None.  get_measured_overlaps() -> (timesteps uint64[n], spin int64[n, P], link int64[n, P]
    // or None, by_class int64[n, P, T, C] or None); reset_measured_overlaps() empties the log and keeps the period.  add_graph is
    // refused while it is on.  ValueError where isingmc_overlap_series_create / _set_every refuse.
    void set_measure_overlaps_every(size_t k, bool link, const py::object &classes, size_t capacity)
    {
        if (k == 0) {
            if (series_) check(isingmc_overlap_series_set_every(series_->s, 0));
            return;
        }
        auto h = series_handle<SeriesHandle>(classes, isingmc_states_count(st_->s) / 2);
        h->link = link;
        check(isingmc_overlap_series_create(st_->s, nullptr, h->columns, h->classes.c, link ? ISINGMC_SERIES_LINK : 0u, capacity, &h->s));
        series_.reset(); // (the old log goes, and its period with it, before the new one takes the container's one period)
        check(isingmc_overlap_series_set_every(h->s, k));
        series_ = std::move(h);
    }
    py::tuple get_measured_overlaps()
    {
        if (!series_) throw py::value_error("no overlaps are logged: call set_measure_overlaps_every(k) first");
        const SeriesHandle &h = *series_;
        size_t n = 0;
        check(isingmc_overlap_series_count(h.s, &n, nullptr));
        const ssize_t N = ssize_t(n), P = ssize_t(h.columns);
        py::array_t<uint64_t> t(std::vector<ssize_t>{N});
        py::array_t<int64_t> spin(std::vector<ssize_t>{N, P}), lnk(std::vector<ssize_t>{h.link ? N : 0, P});
        py::array_t<int64_t> cls(std::vector<ssize_t>{h.n_tables ? N : 0, P, ssize_t(h.n_tables), ssize_t(h.n_classes)});
        uint64_t *t_out = t.mutable_data();
        int64_t *s_out = spin.mutable_data(), *l_out = h.link ? lnk.mutable_data() : nullptr, *c_out = h.n_tables ? cls.mutable_data() : nullptr;
        {
            py::gil_scoped_release nogil;
            check(isingmc_overlap_series_get(h.s, 0, n, t_out, s_out, l_out, c_out));
        }
        return py::make_tuple(t, spin, h.link ? py::object(lnk) : py::object(py::none()), h.n_tables ? py::object(cls) : py::object(py::none()));
    }
    void reset_measured_overlaps() { if (series_) check(isingmc_overlap_series_reset(series_->s)); }
    // extension: energy, magnetisation and magnetisation by class of every persistent replica, logged on the device
    // once per sample.  set_measure_observables_every(k, classes, capacity): a row follows every k-th timestep from now on, without
    // the host waiting (0: off, the rows stay); a call with k > 0 starts a new log of `capacity` rows.  classes: class tables as
    // get_overlaps_by_class takes them, or None.  get_measured_observables() -> (timesteps uint64[n], energies f64[n, R],
    // magnetisations int64[n, R], by_class int64[n, R, T, K] or None); reset_measured_observables() empties the log and keeps the
    // period.  add_graph is refused while it is on.  ValueError where isingmc_observable_series_create / _set_every refuse.
    void set_measure_observables_every(size_t k, const py::object &classes, size_t capacity)
    {
        if (k == 0) {
            if (obs_series_) check(isingmc_observable_series_set_every(obs_series_->s, 0));
            return;
        }
        auto h = series_handle<ObsSeriesHandle>(classes, isingmc_states_count(st_->s));
        check(isingmc_observable_series_create(st_->s, h->classes.c, ISINGMC_OBS_ENERGY | ISINGMC_OBS_MAGNETISATION, capacity, &h->s));
        obs_series_.reset(); // (the old log goes, and its period with it, before the new one takes the container's one period)
        check(isingmc_observable_series_set_every(h->s, k));
        obs_series_ = std::move(h);
    }
    py::tuple get_measured_observables()
    {
        if (!obs_series_) throw py::value_error("no observables are logged: call set_measure_observables_every(k) first");
        const ObsSeriesHandle &h = *obs_series_;
        size_t n = 0;
        check(isingmc_observable_series_count(h.s, &n, nullptr));
        const ssize_t N = ssize_t(n), R = ssize_t(h.columns);
        py::array_t<uint64_t> t(std::vector<ssize_t>{N});
        py::array_t<double> e(std::vector<ssize_t>{N, R});
        py::array_t<int64_t> m(std::vector<ssize_t>{N, R});
        py::array_t<int64_t> cls(std::vector<ssize_t>{h.n_tables ? N : 0, R, ssize_t(h.n_tables), ssize_t(h.n_classes)});
        uint64_t *t_out = t.mutable_data();
        double *e_out = e.mutable_data();
        int64_t *m_out = m.mutable_data(), *c_out = h.n_tables ? cls.mutable_data() : nullptr;
        {
            py::gil_scoped_release nogil;
            check(isingmc_observable_series_get(h.s, 0, n, t_out, e_out, m_out, c_out));
        }
        return py::make_tuple(t, e, m, h.n_tables ? py::object(cls) : py::object(py::none()));
    }
    void reset_measured_observables() { if (obs_series_) check(isingmc_observable_series_reset(obs_series_->s)); }
    // extension: the cluster-size moments of every non-local step of the persistent replicas, logged on the device.
    // set_measure_clusters(capacity): a new log of `capacity` rows; its kind follows whichever period is on -- Swendsen-Wang steps
    // (set_cluster_update_every: a column per replica) or isoenergetic moves (set_replica_cluster_update_every: a column per pair);
    // ValueError if neither is.  get_measured_clusters() -> (timesteps uint64[n], n_clusters, largest, sites, s2, s4_lo, s4_hi:
    // uint64[n, C] each); reset_measured_clusters() empties the log.  add_graph is refused while the log lives.
    void set_measure_clusters(size_t capacity)
    {
        size_t sw = 0, icm = 0;
        check(isingmc_states_cluster_every(st_->s, &sw));
        check(isingmc_states_icm_every(st_->s, &icm));
        if (!sw && !icm) throw py::value_error("neither cluster period is on: set_cluster_update_every(k) or set_replica_cluster_update_every(k) first");
        cluster_series_.reset(); // (the old log goes before the new one takes the container's one slot)
        auto h = std::make_unique<ClusterSeriesHandle>();
        h->columns = sw ? isingmc_states_count(st_->s) : isingmc_states_count(st_->s) / 2;
        check(isingmc_cluster_series_create(st_->s, sw ? ISINGMC_CLUSTER_SERIES_SW : ISINGMC_CLUSTER_SERIES_ICM, capacity, &h->s));
        cluster_series_ = std::move(h);
    }
    py::tuple get_measured_clusters()
    {
        if (!cluster_series_) throw py::value_error("no clusters are logged: call set_measure_clusters() first");
        size_t n = 0;
        check(isingmc_cluster_series_count(cluster_series_->s, &n, nullptr));
        std::vector<uint64_t> t(n), rows(n * cluster_series_->columns * 6);
        {
            py::gil_scoped_release nogil;
            check(isingmc_cluster_series_get(cluster_series_->s, 0, n, t.data(), rows.data()));
        }
        return cluster_series_rows(t, rows, cluster_series_->columns, 0);
    }
    void reset_measured_clusters() { if (cluster_series_) check(isingmc_cluster_series_reset(cluster_series_->s)); }
    // extension: the spin autocorrelation of every persistent replica over time lags, measured on the device.
    // set_measure_autocorrelation_every(k, max_lag): a sample follows every k-th timestep from now on, whatever kind of timestep it
    // is, without the host waiting (0: off, ring and sums stay); a call with k > 0 starts a new ring of max_lag = 1 .. 256 snapshots.
    // get_measured_autocorrelation() -> (lags_in_timesteps int64[L + 1] = l k, counts uint64[L + 1], corr float64[R, L + 1]):
    // corr[:, 0] is 1 once a sample is in, a lag without a term is NaN.  reset_measured_autocorrelation() zeroes sums and sample
    // number and keeps the period.  add_graph is refused while the ring lives.  ValueError where isingmc_autocorr_create refuses.
    void set_measure_autocorrelation_every(size_t k, size_t max_lag)
    {
        if (k == 0) {
            if (autocorr_) check(isingmc_autocorr_set_every(autocorr_->ac, 0));
            return;
        }
        // The old ring has to go before the new one takes the container's one slot.  A lag count out of range is refused before that;
        // what only the library can refuse -- a ring beyond autocorr_bytes -- comes after, and its ValueError says that the old ring
        // has gone (the container's family, the other reason, cannot have changed since the old ring was made)
        if (max_lag < 1 || max_lag > 256) throw py::value_error("max_lag must be 1 .. 256 (the lags a ring holds)");
        const bool had_ring = bool(autocorr_);
        autocorr_.reset();
        auto h = std::make_unique<AutocorrHandle>();
        if (isingmc_autocorr_create(st_->s, max_lag, 0, &h->ac) != ISINGMC_OK)
            throw py::value_error(std::string(isingmc_last_error()) + (had_ring ? " (the ring measured so far has been destroyed)" : ""));
        check(isingmc_autocorr_set_every(h->ac, k));
        h->every = k;
        h->n_lags = max_lag;
        autocorr_ = std::move(h);
    }
    py::tuple get_measured_autocorrelation()
    {
        if (!autocorr_) throw py::value_error("no autocorrelation is measured: call set_measure_autocorrelation_every(k) first");
        const size_t R = isingmc_states_count(st_->s), row = autocorr_->n_lags + 1;
        std::vector<uint64_t> counts(row), diff(R * row);
        {
            py::gil_scoped_release nogil;
            check(isingmc_autocorr_get(autocorr_->ac, counts.data(), diff.data()));
        }
        py::array_t<int64_t> lags(std::vector<ssize_t>{ssize_t(row)});
        py::array_t<uint64_t> cnt(std::vector<ssize_t>{ssize_t(row)});
        for (size_t l = 0; l < row; l++) {
            lags.mutable_data()[l] = int64_t(l * autocorr_->every);
            cnt.mutable_data()[l] = counts[l];
        }
        return py::make_tuple(lags, cnt, autocorr_array(counts, diff, R, row, row, E_.nvars));
    }
    void reset_measured_autocorrelation() { if (autocorr_) check(isingmc_autocorr_reset(autocorr_->ac)); }
    // extension: Swendsen-Wang cluster steps on the persistent replicas (see Lattice.set_cluster_update_every); the graph is known
    // here, so one the cluster step does not serve raises ValueError at once
    void set_cluster_update_every(size_t k) { check(isingmc_states_set_cluster_every(st_->s, k)); }
    // extension: isoenergetic cluster moves between the persistent replicas (2 p, 2 p + 1) (see Lattice.set_replica_cluster_update_every)
    void set_replica_cluster_update_every(size_t k) { check(isingmc_states_set_icm_every(st_->s, k)); }

private:
    static const uint32_t *pairs_ptr(const std::vector<uint32_t> &v) { return v.empty() ? nullptr : v.data(); }
    // `pairs` of get_overlaps / get_overlaps_by_class as two slot tables (left empty for None); returns the number of pairs
    size_t overlap_pairs(const py::object &pairs, std::vector<uint32_t> &sa, std::vector<uint32_t> &sb) const
    {
        const size_t R = isingmc_states_count(st_->s);
        if (pairs.is_none()) return R / 2;
        const auto arr = py::array_t<int64_t, py::array::c_style | py::array::forcecast>::ensure(pairs);
        if (!arr || arr.ndim() != 2 || arr.shape(1) != 2) throw py::value_error("pairs must be an integer array of shape [n, 2]");
        const size_t n = size_t(arr.shape(0));
        const int64_t *v = arr.data();
        sa.resize(n);
        sb.resize(n);
        for (size_t p = 0; p < n; p++) {
            if (v[2 * p] < 0 || v[2 * p + 1] < 0 || size_t(v[2 * p]) >= R || size_t(v[2 * p + 1]) >= R)
                throw py::value_error("slot out of range: every graph index of `pairs` must be below get_num_graphs()");
            sa[p] = uint32_t(v[2 * p]);
            sb[p] = uint32_t(v[2 * p + 1]);
        }
        return n;
    }
    // nspinupdates = single-spin attempts per timestep (classicising.rs:88-110 hands it to do_time_step; crate default:
    // nvars).  The engine attempts every site once per sweep, in the colour order, so attempts are executed sweep by
    // sweep: `timesteps` timesteps of n attempts add timesteps x n attempts to a cursor that persists across calls,
    // every nvars accumulated attempts run as one sweep, and the remainder (< nvars attempts) stays pending for the next
    // call.  Whole multiples of nvars are exactly that many sweeps per timestep; any other positive count is honoured on
    // average (the total number of attempts is exact up to the pending remainder), with a one-off warning.
    bool whole_sweeps(const std::optional<size_t> &nspinupdates) const
    {
        return !nspinupdates || (*nspinupdates > 0 && *nspinupdates % E_.nvars == 0 && pending_attempts_ == 0);
    }
    size_t sweeps_for(size_t timesteps, const std::optional<size_t> &nspinupdates)
    {
        if (!nspinupdates) return timesteps;
        if (*nspinupdates == 0) throw py::value_error("nspinupdates must be positive");
        if (*nspinupdates % E_.nvars != 0 && !warned_partial_) {
            warned_partial_ = true;
            if (PyErr_WarnEx(PyExc_UserWarning,
                             "nspinupdates is not a multiple of the number of variables: attempts are executed sweep by sweep "
                             "(every site once, in the colour order); the attempts that do not complete a sweep stay pending "
                             "and count towards the next timesteps", 1) < 0)
                throw py::error_already_set();
        }
        const unsigned __int128 total = (unsigned __int128)timesteps * *nspinupdates + pending_attempts_;
        const unsigned __int128 sweeps = total / E_.nvars;
        if (sweeps > (unsigned __int128)std::numeric_limits<size_t>::max() / 4) throw py::value_error("too many spin updates");
        pending_attempts_ = size_t(total % E_.nvars);
        return size_t(sweeps);
    }

    size_t pending_attempts_ = 0;
    bool warned_partial_ = false;
    EdgeArrays E_;
    double longitudinal_;
    bool use_basic_moves_; // stored, never read -- as in the reference (classicising.rs:45,54)
    uint64_t master_seed_ = 0;
    std::vector<uint64_t> drawn_;
    std::shared_ptr<GraphHandle> graph_;
    std::shared_ptr<StatesHandle> st_;
    std::unique_ptr<SeriesHandle> series_; // (declared last: destroyed before the container it reads)
    std::unique_ptr<ObsSeriesHandle> obs_series_; // (the same)
    std::unique_ptr<ClusterSeriesHandle> cluster_series_; // (the same)
    std::unique_ptr<AutocorrHandle> autocorr_; // (the same)
};

} // namespace

PYBIND11_MODULE(_py_monte_carlo, m)
{
    m.doc() = "MI355X-native classical Ising Metropolis engine behind the py_monte_carlo API";
    using namespace py::literals;

    py::class_<Lattice>(m, "Lattice")
        .def(py::init<const py::object &, std::optional<uint64_t>, std::optional<bool>>(), "edges"_a,
             "seed_gen"_a = py::none(), "use_allocator"_a = py::none())
        .def_static("from_arrays", &Lattice::from_arrays, "edge_a"_a, "edge_b"_a, "edge_j"_a, "seed_gen"_a = py::none())
        .def("set_seed_gen", &Lattice::set_seed_gen, "seed_gen"_a = py::none())
        .def("make_seeds", &Lattice::make_seeds, "num_experiments"_a)
        .def("set_enable_rvb_update", &Lattice::set_enable_rvb_update, "enable_updates"_a)
        .def("set_enable_heatbath_update", &Lattice::set_enable_heatbath_update, "enable_heatbath"_a)
        .def("set_individual_bias", &Lattice::set_individual_bias, "var"_a, "bias"_a)
        .def("set_global_bias", &Lattice::set_global_bias, "bias"_a)
        .def("set_transverse_field", &Lattice::set_transverse_field, "transverse"_a)
        .def("set_initial_state", &Lattice::set_initial_state, "initial_state"_a)
        .def("set_device", &Lattice::set_device, "device"_a)
        .def("set_devices", &Lattice::set_devices, "devices"_a)
        .def("get_devices", &Lattice::get_devices)
        .def("set_force_general_path", &Lattice::set_force_general_path, "force"_a)
        .def("set_stable_path", &Lattice::set_stable_path, "stable"_a)
        .def("set_cluster_update_every", &Lattice::set_cluster_update_every, "k"_a)
        .def("set_replica_cluster_update_every", &Lattice::set_replica_cluster_update_every, "k"_a)
        .def("set_rng_rounds", [](py::object self, int rounds) { self.cast<Lattice &>().set_rng_rounds(rounds); return self; }, "rounds"_a)
        .def("engine_info", &Lattice::engine_info, "num_experiments"_a = py::none())
        .def("run_monte_carlo", &Lattice::run_monte_carlo, "beta"_a, "timesteps"_a, "num_experiments"_a,
             "only_basic_moves"_a = py::none(), "edge_move_importance_sampling"_a = py::none(),
             "replica_range"_a = py::none())
        .def("run_monte_carlo_sampling", &Lattice::run_monte_carlo_sampling, "beta"_a, "timesteps"_a,
             "num_experiments"_a, "only_basic_moves"_a = py::none(), "thermalization_time"_a = py::none(),
             "sampling_freq"_a = py::none(), "edge_move_importance_sampling"_a = py::none(),
             "replica_range"_a = py::none())
        .def("run_monte_carlo_and_measure_spins", &Lattice::run_monte_carlo_and_measure_spins, "beta"_a, "timesteps"_a,
             "num_experiments"_a, "thermalization_time"_a = py::none(), "sampling_freq"_a = py::none(),
             "per_experiment"_a = true, "bonds"_a = false)
        .def("run_monte_carlo_and_measure_observables", &Lattice::run_monte_carlo_and_measure_observables, "beta"_a, "timesteps"_a,
             "num_experiments"_a, "thermalization_time"_a = py::none(), "sampling_freq"_a = py::none(), "classes"_a = py::none())
        .def("run_monte_carlo_and_measure_variable_autocorrelation", &Lattice::run_monte_carlo_and_measure_variable_autocorrelation, "beta"_a,
             "timesteps"_a, "num_experiments"_a, "sampling_wait_buffer"_a = py::none(), "sampling_freq"_a = py::none(), "max_lag"_a = 32,
             "connected"_a = false)
        .def("run_monte_carlo_and_measure_clusters", &Lattice::run_monte_carlo_and_measure_clusters, "beta"_a, "timesteps"_a,
             "num_experiments"_a, "thermalization_time"_a = py::none())
        .def("run_monte_carlo_annealing", &Lattice::run_monte_carlo_annealing, "betas"_a, "timesteps"_a,
             "num_experiments"_a, "only_basic_moves"_a = py::none(), "edge_move_importance_sampling"_a = py::none(),
             "replica_range"_a = py::none())
        .def("run_monte_carlo_annealing_and_get_energies", &Lattice::run_monte_carlo_annealing_and_get_energies,
             "betas"_a, "timesteps"_a, "num_experiments"_a, "only_basic_moves"_a = py::none(),
             "edge_move_importance_sampling"_a = py::none(), "replica_range"_a = py::none())
        .def("run_population_annealing", &Lattice::run_population_annealing, "betas"_a, "sweeps_per_beta"_a, "population"_a,
             py::kw_only(), "return_states"_a = true, "measure_overlaps"_a = false, "track_minimum"_a = false,
             "overlap_classes"_a = py::none())
        .def("run_population_annealing_adaptive", &Lattice::run_population_annealing_adaptive, "beta_start"_a, "beta_end"_a,
             "sweeps_per_beta"_a, "population"_a, py::kw_only(), "target_overlap"_a = 0.85, "max_dbeta"_a = py::none(),
             "max_steps"_a = 10000, "return_states"_a = true, "measure_overlaps"_a = false, "track_minimum"_a = false,
             "overlap_classes"_a = py::none())
        .def("run_monte_carlo_annealing_and_get_minimum", &Lattice::run_monte_carlo_annealing_and_get_minimum, "betas"_a, "timesteps"_a,
             "num_experiments"_a, "every"_a = 1, "only_basic_moves"_a = py::none())
        .def("clone", &Lattice::clone);
    // the reference's quantum (SSE) entry points (lattice.rs:478-1036) live in the un-vendored qmc crate and are out of
    // scope: present by name, so a script written for the reference fails with a reason instead of an AttributeError
    for (const char *name : {"run_quantum_monte_carlo", "run_quantum_monte_carlo_sampling",
                             "run_quantum_monte_carlo_and_measure_variable_autocorrelation",
                             "run_quantum_monte_carlo_and_measure_spin_product_autocorrelation",
                             "run_quantum_monte_carlo_and_measure_bond_autocorrelation",
                             "run_quantum_monte_carlo_and_measure_spins", "get_offset", "average_on_and_off_diagonal_and_consts"}) {
        const std::string what = std::string("Lattice.") + name + ": quantum (SSE) Monte Carlo is not part of this build (classical Metropolis only)";
        py::setattr(m.attr("Lattice"), name, py::cpp_function([what](const py::args &, const py::kwargs &) -> py::object {
                        PyErr_SetString(PyExc_NotImplementedError, what.c_str());
                        throw py::error_already_set();
                    }, py::is_method(m.attr("Lattice"))));
    }

    py::class_<ClassicIsing>(m, "ClassicIsing")
        .def(py::init<const py::object &, std::optional<double>, std::optional<size_t>, std::optional<uint64_t>,
                      std::optional<bool>>(),
             "edges"_a, "longitudinal"_a = py::none(), "num_experiments"_a = py::none(), "seed"_a = py::none(),
             "use_basic_moves"_a = py::none())
        .def("add_graph", &ClassicIsing::add_graph, "initial_state"_a = py::none(),
             "edge_move_importance_sampling"_a = py::none())
        .def("run_monte_carlo", &ClassicIsing::run_monte_carlo, "beta"_a, "timesteps"_a, "nspinupdates"_a = py::none(),
             "nedgeupdates"_a = py::none(), "nwormupdates"_a = py::none(), "only_basic_moves"_a = py::none())
        .def("run_monte_carlo_sampling", &ClassicIsing::run_monte_carlo_sampling, "beta"_a, "timesteps"_a,
             "nspinupdates"_a = py::none(), "nedgeupdates"_a = py::none(), "nwormupdates"_a = py::none(),
             "only_basic_moves"_a = py::none(), "thermalization_time"_a = py::none(), "sampling_freq"_a = py::none())
        .def("get_energies", &ClassicIsing::get_energies)
        .def("get_states", &ClassicIsing::get_states)
        .def("get_num_graphs", &ClassicIsing::get_num_graphs)
        .def("set_rng_rounds", [](py::object self, int rounds) { self.cast<ClassicIsing &>().set_rng_rounds(rounds); return self; }, "rounds"_a)
        .def("get_rng_rounds", &ClassicIsing::get_rng_rounds)
        .def("get_overlaps", &ClassicIsing::get_overlaps, "pairs"_a = py::none(), "link"_a = true)
        .def("get_overlaps_by_class", &ClassicIsing::get_overlaps_by_class, "classes"_a, "n_classes"_a = py::none(), "pairs"_a = py::none())
        .def("set_measure_overlaps_every", &ClassicIsing::set_measure_overlaps_every, "k"_a, "link"_a = true, "classes"_a = py::none(),
             "capacity"_a = 4096)
        .def("get_measured_overlaps", &ClassicIsing::get_measured_overlaps)
        .def("reset_measured_overlaps", &ClassicIsing::reset_measured_overlaps)
        .def("set_measure_observables_every", &ClassicIsing::set_measure_observables_every, "k"_a, "classes"_a = py::none(), "capacity"_a = 4096)
        .def("get_measured_observables", &ClassicIsing::get_measured_observables)
        .def("reset_measured_observables", &ClassicIsing::reset_measured_observables)
        .def("set_measure_clusters", &ClassicIsing::set_measure_clusters, "capacity"_a = 4096)
        .def("get_measured_clusters", &ClassicIsing::get_measured_clusters)
        .def("reset_measured_clusters", &ClassicIsing::reset_measured_clusters)
        .def("set_measure_autocorrelation_every", &ClassicIsing::set_measure_autocorrelation_every, "k"_a, "max_lag"_a = 32)
        .def("get_measured_autocorrelation", &ClassicIsing::get_measured_autocorrelation)
        .def("reset_measured_autocorrelation", &ClassicIsing::reset_measured_autocorrelation)
        .def("set_track_minimum", &ClassicIsing::set_track_minimum, "every"_a)
        .def("get_minimum", &ClassicIsing::get_minimum)
        .def("reset_minimum", &ClassicIsing::reset_minimum)
        .def("set_measure_spins_every", &ClassicIsing::set_measure_spins_every, "k"_a, "per_experiment"_a = false, "bonds"_a = false)
        .def("get_measured_spins", &ClassicIsing::get_measured_spins)
        .def("reset_measured_spins", &ClassicIsing::reset_measured_spins)
        .def("set_cluster_update_every", &ClassicIsing::set_cluster_update_every, "k"_a)
        .def("set_replica_cluster_update_every", &ClassicIsing::set_replica_cluster_update_every, "k"_a);
}
