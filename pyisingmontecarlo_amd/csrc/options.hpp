// Path / tuning switches.  They are read from the environment ONCE, when a graph or a replica container is created, into an
// options block of that handle; isingmc_states_set_option changes one of them on one container.  Nothing below *_create calls
// getenv: two containers of one process can run different paths, and a test that sets a variable must do so before it creates
// the object it wants to steer.  (Measurement / A-B switches and test hooks; none of them changes a result, only which kernel
// produces it -- except FORCE / DISABLE of a kernel FAMILY, which select another spec: DESIGN.md section 2.)
// Plain C++ (no HIP include): tests/options_host.cpp drives the block as an executable of its own.
#pragma once
#include <algorithm>
#include <cctype>
#include <cstdlib>
#include <string>
#include <vector>

inline bool env_flag(const char *name)
{
    const char *e = std::getenv(name);
    return e && e[0] && e[0] != '0';
}

inline int env_int(const char *name, int dflt)
{
    const char *e = std::getenv(name);
    return e && e[0] ? std::atoi(e) : dflt;
}

// an option's name as the table below holds it: lower case, without the ISINGMC_ prefix
inline std::string option_bare_name(const std::string &name)
{
    std::string n;
    for (char c : name) n += char(std::tolower(static_cast<unsigned char>(c)));
    return n.rfind("isingmc_", 0) == 0 ? n.substr(8) : n;
}

struct Options {
    // the members carry the defaults; table() below names each switch once, for from_env() and set() alike
    int force_real = 0, disable_real = 0, force_packed = 0, disable_packed = 0; // kernel family (decided at creation)
    int disable_packed_uniform = 0, disable_resident = 0;
    int strip = -1, strip_nw = 4, strip_max_wg = -1, strip_test_fail_once = 0; // persistent strip kernel: -1 auto / 0 off / 1 force
    int streams = 0, pk_streams = 0;                                            // replica lanes: 0 = the measured rule
    int sweep_iters = 0, debug_sweep_lds = 0;
    int resident_spread = 1, resident_lpq = 0, gen_stage = -1;
    int gen_rb = 0; // replicas per thread of the streaming CSR kernel: 0 = the rule of launch_gen_timestep, 1 / 2 / 4 / 8 forces
    int sample_slab_bytes = 64 << 20, pt_in_kernel = 1, real_target_wgs = 3072;
    int real_measure_wgs = 0; // workgroups the real-coupling measurement shares among its groups: 0 = the occupancy figure (measure_enqueue)
    int cluster_workspace_bytes = 1 << 30; // labels, cluster sizes and bond planes of one batch of replicas
    int moments_planes = 8;               // time planes of the per-replica moment sums: a flush every 2^K - 1 samples
    long long moments_bytes = 4ll << 30;   // the most device memory the moment sums of one container may take (64 bits: beyond an int)
    long long overlap_series_bytes = 1ll << 30; // the most device memory the log of one overlap series may take
    long long observable_series_bytes = 1ll << 30; // ... and the log of one observable series
    long long cluster_series_bytes = 1ll << 30;    // ... and the log of one cluster series
    // Rounds of the sweeps' Philox calls, 10 or 7: the one switch here that selects another trajectory.  Written
    // only through philox_rounds_set (isingmc.hip), which checks the value and the container; read wherever a call is planned.
    // Not in the table: set() does not reach it
    int philox_rounds = 10;
    // The most device memory the snapshots and sums of a container's lag ring may take (next to moments_bytes in
    // meaning, 64 bits).  Not in the table either -- tests/options_host.cpp pins the table's names and count: the environment is read
    // below, and isingmc_states_set_option assigns it by name (isingmc.hip)
    long long autocorr_bytes = 4ll << 30;

    // FLAG: set or not in the environment (anything but "" and "0..." is on; every flag is off by default).  INT: atoi, the
    // default when unset or empty.  INT64: atoll when set.  set() assigns the value as it comes, whatever the kind.
    enum Kind { FLAG, INT, INT64 };
    struct Entry {
        std::string name, env; // what set() accepts; the environment variable
        Kind kind;
        int Options::*i;
        long long Options::*w;
    };
    static const std::vector<Entry> &table()
    {
        // env: the variable's name where it is not ISINGMC_ + the upper-case name
        auto entry = [](const char *name, Kind kind, int Options::*i, long long Options::*w, const char *env) {
            std::string e = env ? env : "ISINGMC_";
            if (!env) for (const char *c = name; *c; c++) e += char(std::toupper(static_cast<unsigned char>(*c)));
            return Entry{name, e, kind, i, w};
        };
        auto flag = [&](const char *name, int Options::*m) { return entry(name, FLAG, m, nullptr, nullptr); };
        auto num = [&](const char *name, int Options::*m, const char *env = nullptr) { return entry(name, INT, m, nullptr, env); };
        auto wide = [&](const char *name, long long Options::*m) { return entry(name, INT64, nullptr, m, nullptr); };
        static const std::vector<Entry> t = {
            flag("force_real", &Options::force_real), flag("disable_real", &Options::disable_real),
            flag("force_packed", &Options::force_packed), flag("disable_packed", &Options::disable_packed),
            flag("disable_packed_uniform", &Options::disable_packed_uniform), flag("disable_resident", &Options::disable_resident),
            num("strip", &Options::strip), num("strip_nw", &Options::strip_nw), num("strip_max_wg", &Options::strip_max_wg),
            flag("strip_test_fail_once", &Options::strip_test_fail_once),
            num("streams", &Options::streams), num("pk_streams", &Options::pk_streams),
            num("sweep_iters", &Options::sweep_iters), num("debug_sweep_lds", &Options::debug_sweep_lds),
            num("resident_spread", &Options::resident_spread), num("resident_lpq", &Options::resident_lpq),
            num("gen_stage", &Options::gen_stage), num("gen_rb", &Options::gen_rb, "ISINGMC_GEN_RB_FORCE"),
            num("sample_slab_bytes", &Options::sample_slab_bytes), num("pt_in_kernel", &Options::pt_in_kernel),
            num("real_target_wgs", &Options::real_target_wgs), num("real_measure_wgs", &Options::real_measure_wgs),
            num("cluster_workspace_bytes", &Options::cluster_workspace_bytes), num("moments_planes", &Options::moments_planes),
            wide("moments_bytes", &Options::moments_bytes), wide("overlap_series_bytes", &Options::overlap_series_bytes),
            wide("observable_series_bytes", &Options::observable_series_bytes), wide("cluster_series_bytes", &Options::cluster_series_bytes)};
        return t;
    }

    static Options from_env()
    {
        Options o;
        for (const Entry &e : table()) {
            if (e.kind == FLAG) o.*e.i = env_flag(e.env.c_str());
            else if (e.kind == INT) o.*e.i = env_int(e.env.c_str(), o.*e.i);
            else if (const char *v = std::getenv(e.env.c_str())) o.*e.w = std::atoll(v);
        }
        // the environment's values alone are clamped: set() takes what it is given
        o.sample_slab_bytes = std::max(1, o.sample_slab_bytes);
        o.real_target_wgs = std::max(256, o.real_target_wgs);
        o.cluster_workspace_bytes = std::max(1, o.cluster_workspace_bytes);
        o.philox_rounds = env_int("ISINGMC_PHILOX_ROUNDS", o.philox_rounds);
        if (const char *v = std::getenv("ISINGMC_AUTOCORR_BYTES")) o.autocorr_bytes = std::atoll(v);
        return o;
    }

    // name: the environment variable's name without the ISINGMC_ prefix, lower or upper case
    bool set(const std::string &name_in, long value)
    {
        const std::string n = option_bare_name(name_in);
        for (const Entry &e : table())
            if (n == e.name) {
                if (e.kind == INT64) this->*e.w = value;
                else this->*e.i = int(value);
                return true;
            }
        return false;
    }
};
