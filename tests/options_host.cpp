// Stand-alone check of csrc/options.hpp (built with ASan + UBSan by tests/test_options_host.py): the names isingmc_states_set_option
// has always taken, in every spelling; the environment read against the members' defaults; the clamps of the environment's values.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "options.hpp"

static int g_failures = 0;
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::printf("options_host: line %d: %s\n", __LINE__, #cond);             \
            g_failures++;                                                            \
        }                                                                            \
    } while (0)

// every member, by name: what the table is checked against is written out here, not read from the table
#define INT_MEMBERS(X)                                                                                                              \
    X(force_real) X(disable_real) X(force_packed) X(disable_packed) X(disable_packed_uniform) X(disable_resident) X(strip)        \
    X(strip_nw) X(strip_max_wg) X(strip_test_fail_once) X(streams) X(pk_streams) X(sweep_iters) X(debug_sweep_lds)                \
    X(resident_spread) X(resident_lpq) X(gen_stage) X(gen_rb) X(sample_slab_bytes) X(pt_in_kernel) X(real_target_wgs)             \
    X(real_measure_wgs) X(cluster_workspace_bytes) X(moments_planes)
#define WIDE_MEMBERS(X) X(moments_bytes) X(overlap_series_bytes) X(observable_series_bytes) X(cluster_series_bytes)

static bool same(const Options &a, const Options &b)
{
    bool eq = a.philox_rounds == b.philox_rounds;
#define X(m) eq = eq && a.m == b.m;
    INT_MEMBERS(X) WIDE_MEMBERS(X)
#undef X
    return eq;
}

static std::string upper(std::string s)
{
    for (char &c : s) c = char(std::toupper(static_cast<unsigned char>(c)));
    return s;
}

static void clear_env()
{
#define X(m) unsetenv(("ISINGMC_" + upper(#m)).c_str());
    INT_MEMBERS(X) WIDE_MEMBERS(X)
#undef X
    unsetenv("ISINGMC_GEN_RB_FORCE");
    unsetenv("ISINGMC_PHILOX_ROUNDS");
}

int main()
{
    clear_env();
    const Options dflt;
    // the defaults the library has shipped with
    CHECK(dflt.strip == -1 && dflt.strip_nw == 4 && dflt.strip_max_wg == -1 && dflt.resident_spread == 1 && dflt.gen_stage == -1);
    CHECK(dflt.sample_slab_bytes == (64 << 20) && dflt.pt_in_kernel == 1 && dflt.real_target_wgs == 3072 && dflt.cluster_workspace_bytes == (1 << 30));
    CHECK(dflt.moments_planes == 8 && dflt.moments_bytes == (4ll << 30) && dflt.overlap_series_bytes == (1ll << 30));
    CHECK(dflt.observable_series_bytes == (1ll << 30) && dflt.cluster_series_bytes == (1ll << 30) && dflt.philox_rounds == 10);
    CHECK(dflt.force_real == 0 && dflt.streams == 0 && dflt.gen_rb == 0 && dflt.real_measure_wgs == 0);

    // an empty environment gives the defaults, member by member (no clamp applies to a default)
    CHECK(same(Options::from_env(), dflt));

    // set(): every name in lower case, upper case and with the prefix, each reaching its own member
    int value = 100;
#define X(m)                                                                                        \
    for (const std::string &name : {std::string(#m), upper(#m), "ISINGMC_" + upper(#m), "isingmc_" + std::string(#m)}) { \
        Options o, expect;                                                                          \
        value++;                                                                                    \
        CHECK(o.set(name, value));                                                                  \
        expect.m = value;                                                                           \
        CHECK(same(o, expect));                                                                     \
    }
    INT_MEMBERS(X) WIDE_MEMBERS(X)
#undef X
    { // a value beyond an int reaches the 64-bit members whole
        Options o;
        CHECK(o.set("moments_bytes", 5l << 32) && o.moments_bytes == (5ll << 32));
    }
    { // unknown names are refused and change nothing; philox_rounds is out of set()'s reach; gen_rb is not set under its variable's name
        Options o;
        for (const char *name : {"", "isingmc_", "no_such_option", "strip_", "force", "philox_rounds", "ISINGMC_PHILOX_ROUNDS", "gen_rb_force", "ISINGMC_GEN_RB_FORCE"})
            CHECK(!o.set(name, 7));
        CHECK(same(o, dflt));
    }

    // the environment: every variable reaches its own member
    value = 1000;
#define X(m)                                                                                        \
    {                                                                                               \
        const std::string var = std::string(#m) == "gen_rb" ? "ISINGMC_GEN_RB_FORCE" : "ISINGMC_" + upper(#m); \
        Options expect;                                                                             \
        value++;                                                                                    \
        setenv(var.c_str(), std::to_string(value).c_str(), 1);                                      \
        expect.m = is_flag(#m) ? 1 : value;                                                         \
        CHECK(same(Options::from_env(), expect));                                                   \
        unsetenv(var.c_str());                                                                      \
    }
    auto is_flag = [](const std::string &m) {
        for (const char *f : {"force_real", "disable_real", "force_packed", "disable_packed", "disable_packed_uniform", "disable_resident", "strip_test_fail_once"})
            if (m == f) return true;
        return false;
    };
    INT_MEMBERS(X) WIDE_MEMBERS(X)
#undef X
    { // flags: "0" and "" are off; integers: "" is the default; the variable of gen_rb is not ISINGMC_GEN_RB
        setenv("ISINGMC_FORCE_PACKED", "0", 1);
        setenv("ISINGMC_DISABLE_RESIDENT", "", 1);
        setenv("ISINGMC_STRIP_NW", "", 1);
        setenv("ISINGMC_GEN_RB", "4", 1);
        CHECK(same(Options::from_env(), dflt));
        clear_env();
        unsetenv("ISINGMC_GEN_RB");
        setenv("ISINGMC_PHILOX_ROUNDS", "7", 1);
        Options expect;
        expect.philox_rounds = 7;
        CHECK(same(Options::from_env(), expect));
        clear_env();
    }

    // the clamps hold for the environment's values, and for those alone
    for (const char *low : {"0", "-5"}) {
        setenv("ISINGMC_SAMPLE_SLAB_BYTES", low, 1);
        setenv("ISINGMC_CLUSTER_WORKSPACE_BYTES", low, 1);
        setenv("ISINGMC_REAL_TARGET_WGS", low, 1);
        Options expect;
        expect.sample_slab_bytes = 1;
        expect.cluster_workspace_bytes = 1;
        expect.real_target_wgs = 256;
        CHECK(same(Options::from_env(), expect));
    }
    setenv("ISINGMC_REAL_TARGET_WGS", "255", 1);
    CHECK(Options::from_env().real_target_wgs == 256);
    setenv("ISINGMC_REAL_TARGET_WGS", "257", 1);
    CHECK(Options::from_env().real_target_wgs == 257);
    clear_env();
    {
        Options o;
        CHECK(o.set("sample_slab_bytes", 0) && o.set("cluster_workspace_bytes", -5) && o.set("real_target_wgs", 8));
        CHECK(o.sample_slab_bytes == 0 && o.cluster_workspace_bytes == -5 && o.real_target_wgs == 8);
    }

    CHECK(option_bare_name("ISINGMC_Strip_NW") == "strip_nw" && option_bare_name("isingmc_") == "" && option_bare_name("STRIP") == "strip");
    CHECK(Options::table().size() == 28);

    if (g_failures) return 1;
    std::printf("options_host: ok\n");
    return 0;
}
