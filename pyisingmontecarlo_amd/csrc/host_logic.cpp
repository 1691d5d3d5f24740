// Host-side logic (no device code).  Reference lines per function: see host_logic.hpp / isingmc.h.
#include "host_logic.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>
#include <random>
#include <unordered_map>

namespace isingmc {

static inline uint64_t rotl(uint64_t x, int k) { return (x << k) | (x >> (64 - k)); }

SmallRng::SmallRng(uint64_t state)
{
    for (auto &word : s) { // SplitMix64 fills the 256-bit state
        state += 0x9e3779b97f4a7c15ull;
        uint64_t z = state;
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        word = z ^ (z >> 31);
    }
}

uint64_t SmallRng::next_u64()
{
    const uint64_t result = rotl(s[0] + s[3], 23) + s[0];
    const uint64_t t = s[1] << 17;
    s[2] ^= s[0];
    s[3] ^= s[1];
    s[1] ^= s[2];
    s[0] ^= s[3];
    s[2] ^= t;
    s[3] = rotl(s[3], 45);
    return result;
}

std::vector<uint64_t> make_seeds(bool has_seed, uint64_t seed_gen, size_t n)
{
    if (!has_seed) { // SmallRng::from_entropy()
        std::random_device rd;
        seed_gen = (uint64_t(rd()) << 32) ^ uint64_t(rd());
    }
    SmallRng rng(seed_gen);
    std::vector<uint64_t> out(n);
    for (auto &v : out) v = rng.next_u64();
    return out;
}

std::string expand_schedule(const uint64_t *stop_t, const double *stop_beta, size_t n_stops,
                            size_t timesteps, bool compat_constant_beta, double *betas_out)
{
    std::vector<std::pair<uint64_t, double>> betas(n_stops);
    for (size_t k = 0; k < n_stops; k++) {
        if (!std::isfinite(stop_beta[k])) return "beta schedule values must be finite";
        betas[k] = {stop_t[k], stop_beta[k]};
    }
    std::stable_sort(betas.begin(), betas.end(),
                     [](const auto &a, const auto &b) { return a.first < b.first; });
    if (betas.empty()) {
        betas.push_back({0, 1.0});
        betas.push_back({timesteps, 1.0});
    }
    if (betas.front().first > 0) betas.insert(betas.begin(), {0, betas.front().second});
    const uint64_t last_user_t = betas.back().first;
    if (betas.back().first < timesteps) betas.push_back({timesteps, betas.back().second});

    size_t idx = 0;
    for (size_t step = 0; step < timesteps; step++) {
        // the reference evaluates the interpolation at a captured constant (the last stop's time)
        const uint64_t i = compat_constant_beta ? last_user_t : step;
        while (idx + 2 < betas.size() && i > betas[idx + 1].first) idx++;
        const auto [ia, va] = betas[idx];
        const auto [ib, vb] = betas[idx + 1];
        const double frac = (ib == ia) ? 0.0 : double(int64_t(i) - int64_t(ia)) / double(ib - ia);
        betas_out[step] = (vb - va) * frac + va;
    }
    return "";
}

Lattice2D recognise_lattice2d(const uint64_t *ea, const uint64_t *eb, const double *ej,
                              size_t n_edges, size_t nvars)
{
    Lattice2D out;
    const uint64_t N = nvars;
    if (N < 16 || n_edges > 2 * N || n_edges < N || N > (uint64_t(1) << 40)) return out;
    // |a-b| is 1 or W-1 for horizontal bonds, W or N-W for vertical ones; N-W of the bonds
    // have |a-b| == W, which makes W the most frequent difference other than 1.
    std::unordered_map<uint64_t, uint64_t> hist;
    for (size_t k = 0; k < n_edges; k++) {
        const uint64_t d = ea[k] > eb[k] ? ea[k] - eb[k] : eb[k] - ea[k];
        if (d != 1 && ++hist[d] && hist.size() > 64) return out; // a lattice has <= 3 such values
    }
    uint64_t W = 0, best = 0;
    for (const auto &[d, cnt] : hist)
        if (cnt > best || (cnt == best && d < W)) { best = cnt; W = d; }
    if (W < 4 || N % W != 0) return out;
    const uint64_t H = N / W;
    if (H < 4 || (H & 1) || (W & 1) || W > (1u << 30) || H > (1u << 30)) return out;

    std::vector<uint8_t> seen(2 * N, 0), jpos(2 * N, 0);
    double jabs_dir[2] = {-1.0, -1.0}; // |J| of the horizontal / vertical bonds: one value per direction
    bool any_pos = false, any_neg = false;
    for (size_t k = 0; k < n_edges; k++) {
        const uint64_t lo = std::min(ea[k], eb[k]), hi = std::max(ea[k], eb[k]);
        if (hi >= N) return out;
        const uint64_t d = hi - lo;
        uint64_t slot;
        if (d == 1 && lo % W != W - 1) slot = 2 * lo;               // right bond of lo
        else if (d == W - 1 && lo % W == 0) slot = 2 * hi;          // right bond of hi wraps to lo
        else if (d == W) slot = 2 * lo + 1;                         // down bond of lo
        else if (d == N - W && lo < W) slot = 2 * hi + 1;           // down bond of hi wraps to lo
        else return out;
        if (seen[slot]) return out;
        seen[slot] = 1;
        double &jd = jabs_dir[slot & 1];
        if (jd < 0.0) jd = std::fabs(ej[k]);
        if (!(std::fabs(ej[k]) == jd)) return out; // one |J| per direction only (NaN fails too)
        const bool pos = ej[k] > 0.0;
        jpos[slot] = pos;
        (pos ? any_pos : any_neg) = true;
    }
    // every interior bond once; the bonds that wrap around in x (right bonds of column W-1) and in y (down bonds of row
    // H-1) either all present (periodic) or all absent (open boundary) in each direction
    uint64_t wrap_x = 0, wrap_y = 0;
    for (uint64_t i = 0; i < N; i++) {
        const bool last_col = i % W == W - 1, last_row = i >= N - W;
        if (last_col) wrap_x += seen[2 * i];
        else if (!seen[2 * i]) return out;
        if (last_row) wrap_y += seen[2 * i + 1];
        else if (!seen[2 * i + 1]) return out;
    }
    if ((wrap_x != 0 && wrap_x != H) || (wrap_y != 0 && wrap_y != W)) return out;
    out.ok = true;
    out.W = int(W);
    out.H = int(H);
    out.jabs = jabs_dir[0];
    out.jabs_y = jabs_dir[1];
    out.open_x = wrap_x == 0;
    out.open_y = wrap_y == 0;
    out.uniform_sign = !(any_pos && any_neg);
    out.jpos_uniform = any_pos && !any_neg;
    if (!out.uniform_sign) {
        out.jright.resize(N);
        out.jdown.resize(N);
        for (uint64_t i = 0; i < N; i++) {
            out.jright[i] = jpos[2 * i];
            out.jdown[i] = jpos[2 * i + 1];
        }
    }
    return out;
}

Adjacency build_adjacency(const uint64_t *ea, const uint64_t *eb, const double *ej, size_t n_edges,
                          size_t nvars)
{
    Adjacency A;
    A.ptr.assign(nvars + 1, 0);
    for (size_t k = 0; k < n_edges; k++) {
        if (ea[k] == eb[k]) { A.self_energy += ej[k]; continue; }
        A.ptr[ea[k] + 1]++;
        A.ptr[eb[k] + 1]++;
    }
    for (size_t i = 0; i < nvars; i++) A.ptr[i + 1] += A.ptr[i];
    A.nbr.resize(A.ptr[nvars]);
    A.w.resize(A.ptr[nvars]);
    std::vector<uint64_t> fill(A.ptr.begin(), A.ptr.end() - 1);
    for (size_t k = 0; k < n_edges; k++) { // neighbours of a site stay in edge-list order
        if (ea[k] == eb[k]) continue;
        A.nbr[fill[ea[k]]] = uint32_t(eb[k]);
        A.w[fill[ea[k]]++] = ej[k];
        A.nbr[fill[eb[k]]] = uint32_t(ea[k]);
        A.w[fill[eb[k]]++] = ej[k];
    }
    return A;
}

Colouring greedy_colouring(const Adjacency &A, size_t nvars)
{
    Colouring C;
    C.colour.resize(nvars);
    uint64_t maxdeg = 0;
    for (size_t i = 0; i < nvars; i++) maxdeg = std::max(maxdeg, A.ptr[i + 1] - A.ptr[i]);
    std::vector<uint8_t> used(maxdeg + 2);
    uint32_t nc = 1;
    for (size_t i = 0; i < nvars; i++) {
        const uint64_t deg = A.ptr[i + 1] - A.ptr[i];
        std::fill(used.begin(), used.begin() + deg + 2, 0);
        for (uint64_t e = A.ptr[i]; e < A.ptr[i + 1]; e++) {
            const uint32_t j = A.nbr[e];
            if (j < i && C.colour[j] <= deg) used[C.colour[j]] = 1;
        }
        uint32_t c = 0;
        while (used[c]) c++;
        C.colour[i] = c;
        nc = std::max(nc, c + 1);
    }
    C.n_colours = nc;
    std::vector<uint64_t> count(nc, 0);
    for (size_t i = 0; i < nvars; i++) count[C.colour[i]]++;
    C.class_base.assign(nc + 1, 0);
    for (uint32_t c = 0; c < nc; c++) C.class_base[c + 1] = C.class_base[c] + (count[c] + 255) / 256 * 256; // whole waves (64) and wave-strided position-quads (4 x 64)
    C.n_pos = C.class_base[nc];
    C.pos.resize(nvars);
    std::fill(count.begin(), count.end(), 0);
    for (size_t i = 0; i < nvars; i++) C.pos[i] = C.class_base[C.colour[i]] + count[C.colour[i]]++;
    return C;
}

} // namespace isingmc

// ---- parallel-tempering swap step (classical ladder; scheduling shaped after tempering.rs:172-212)
namespace isingmc {

static void philox4x32_10_host(const uint32_t ctr[4], uint32_t k0, uint32_t k1, uint32_t out[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = uint64_t(0xD2511F53u) * c0, p1 = uint64_t(0xCD9E8D57u) * c2;
        const uint32_t n0 = uint32_t(p1 >> 32) ^ c1 ^ k0, n2 = uint32_t(p0 >> 32) ^ c3 ^ k1;
        c1 = uint32_t(p1);
        c3 = uint32_t(p0);
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// same arithmetic as the device det_exp (general_kernels.hpp): f64 + fma only
static double det_exp_host(double x)
{
    if (x >= 0.0) return 1.0;
    if (x < -40.0) return 0.0;
    const double LOG2E = 1.4426950408889634074;
    const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    const double kf = std::floor(std::fma(x, LOG2E, 0.5));
    double r = std::fma(-kf, LN2_HI, x);
    r = std::fma(-kf, LN2_LO, r);
    const double coef[13] = {1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0,
                             1.0 / 40320.0, 1.0 / 5040.0, 1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0,
                             1.0 / 6.0, 0.5, 1.0, 1.0};
    double p = 1.0 / 6227020800.0;
    for (double c : coef) p = std::fma(p, r, c);
    return std::ldexp(p, int(kf));
}

uint64_t pt_swap_round(uint64_t seed, uint64_t round, size_t n_rungs, const double *betas,
                       const double *slot_energy, uint32_t *perm)
{
    uint64_t swaps = 0;
    for (size_t i = round & 1; i + 1 < n_rungs; i += 2) { // even rounds pair (0,1),(2,3).., odd (1,2),..
        const double d = (betas[i] - betas[i + 1]) * (slot_energy[perm[i]] - slot_energy[perm[i + 1]]);
        bool accept = d >= 0.0;
        if (!accept) {
            const uint32_t ctr[4] = {uint32_t(i), uint32_t(round), uint32_t(round >> 32), 0x50545357u /* "PTSW" */};
            uint32_t r[4];
            philox4x32_10_host(ctr, uint32_t(seed), uint32_t(seed >> 32), r);
            const uint64_t x = (uint64_t(r[1]) << 32) | r[0];
            const double u = double(x >> 11) * (1.0 / 9007199254740992.0);
            accept = u < det_exp_host(d);
        }
        if (accept) {
            std::swap(perm[i], perm[i + 1]);
            swaps++;
        }
    }
    return swaps;
}

void pt_statistics_round(uint64_t round, size_t n_rungs, const uint32_t *perm_before, const uint32_t *perm_after, const double *slot_energy,
                         uint64_t *attempts, uint64_t *accepts, uint64_t *n_up, uint64_t *n_down, double *sum_e, double *sum_e2,
                         uint64_t *round_trips, uint8_t *labels, uint64_t *rounds)
{
    for (size_t i = 0; i < n_rungs; i++) {
        // (the volatile temporaries keep a compiler that contracts by default from fusing the product into the second sum)
        const double e = slot_energy[perm_before[i]];
        volatile double sq = e * e;
        volatile double s = sum_e[i] + e;
        volatile double s2 = sum_e2[i] + sq;
        sum_e[i] = s;
        sum_e2[i] = s2;
    }
    for (size_t i = round & 1; i + 1 < n_rungs; i += 2) {
        attempts[i] += 1;
        if (perm_after[i] != perm_before[i]) accepts[i] += 1;
    }
    if (n_rungs >= 2) {
        const uint32_t cold = perm_after[0], hot = perm_after[n_rungs - 1];
        if (labels[cold] == 2) round_trips[cold] += 1;
        labels[cold] = 1;
        labels[hot] = 2;
        for (size_t i = 0; i < n_rungs; i++) {
            n_up[i] += labels[perm_after[i]] == 1;
            n_down[i] += labels[perm_after[i]] == 2;
        }
    }
    *rounds += 1;
}

// ---- population annealing: the resampling rule ----------------------------------------------
uint64_t pa_sources(uint64_t seed, uint64_t step, size_t n, const double *energies, double dbeta, uint32_t *src_out, double *eref_out)
{
    double eref = energies[0];
    for (size_t r = 1; r < n; r++) eref = dbeta >= 0.0 ? std::min(eref, energies[r]) : std::max(eref, energies[r]);
    std::vector<uint64_t> C(n);
    uint64_t S = 0;
    for (size_t r = 0; r < n; r++) {
        // one subtraction, one multiplication, one negation, each rounded on its own (the volatile temporaries keep a
        // compiler that contracts by default from fusing them: the device computes exactly these three operations)
        volatile double d = energies[r] - eref;
        volatile double m = dbeta * d;
        const double x = -m;
        S += uint64_t(std::ldexp(det_exp_host(x), 32)); // in [0, 2^32]
        C[r] = S;
    }
    const uint32_t ctr[4] = {uint32_t(step), uint32_t(step >> 32), 0u, 0x50415253u /* "PARS" */};
    uint32_t rnd[4];
    philox4x32_10_host(ctr, uint32_t(seed), uint32_t(seed >> 32), rnd);
    const uint64_t U = (uint64_t(rnd[1]) << 32) | rnd[0];
    using u128 = unsigned __int128;
    const uint64_t u = uint64_t((u128(U) * S) >> 64);
    size_t r = 0;
    for (size_t j = 0; j < n; j++) { // j S + u < n S = n C[n - 1]: r never runs past the end
        const u128 t = u128(j) * S + u;
        while (t >= u128(n) * C[r]) r++;
        src_out[j] = uint32_t(r);
    }
    if (eref_out) *eref_out = eref;
    return S;
}

// ---- population annealing: the step chooser ---------------------------------------------------
uint64_t pa_target32(double target) { return uint64_t(std::ceil(std::ldexp(target, 32))); }

const char *pa_choose_refusal(double dbeta_max, double target)
{
    if (!std::isfinite(dbeta_max) || !(dbeta_max > 0.0)) return "dbeta_max must be finite and positive (heating steps are not chosen)";
    if (!(target > 0.0) || !(target <= 1.0)) return "the target overlap must lie in (0, 1]";
    return nullptr;
}

PaChoice pa_choose_step(size_t n, const double *energies, double dbeta_max, uint64_t t32)
{
    using u128 = unsigned __int128;
    const double eref = *std::min_element(energies, energies + n);
    const double unit = std::ldexp(dbeta_max, -16);
    std::vector<double> d(n);
    for (size_t r = 0; r < n; r++) d[r] = energies[r] - eref;
    std::vector<uint64_t> W(n);
    PaChoice kept{};
    // candidate k: (holds, S, N)
    const auto evaluate = [&](uint32_t k, PaChoice *out) {
        volatile double dbeta = double(k) * unit; // (rounded on their own, like the exponent below: see pa_sources)
        uint64_t S = 0;
        for (size_t r = 0; r < n; r++) {
            volatile double m = dbeta * d[r];
            const double x = -m;
            S += W[r] = uint64_t(std::ldexp(det_exp_host(x), 32));
        }
        u128 N = 0;
        for (size_t r = 0; r < n; r++) N += std::min<uint64_t>(S, uint64_t(n) * W[r]);
        *out = PaChoice{k, dbeta, S, uint64_t(N), uint64_t(N >> 64)};
        return (N << 32) >= u128(t32 * uint64_t(n)) * S;
    };
    uint32_t lo = 0, width = 65536;
    for (int round = 1; round <= 4; round++) {
        const uint32_t step = width / 16, nc = round == 1 ? 16 : 15;
        uint32_t jstar = 0;
        PaChoice c{};
        while (jstar < nc && evaluate(lo + (jstar + 1) * step, &c)) {
            kept = c;
            jstar++;
        }
        if (round == 4 && lo == 0 && jstar == 0) kept = c; // k = 1: the candidate that has just failed
        lo += jstar * step;
        width = step;
        if (round == 1 && jstar == 16) break;
    }
    return kept; // k = max(lo, 1)
}

// ---- replica-packed real-coupling path --------------------------------------------------------
RjQuant rj_quantise(const Adjacency &A, size_t nvars, const double *biases)
{
    RjQuant Q;
    double fmax = 0.0;
    std::vector<double> mags, F(nvars, 0.0); // mags: nonzero |coupling| (every bond once) and |bias|
    for (size_t i = 0; i < nvars; i++) {
        double f = biases ? std::fabs(biases[i]) : 0.0;
        if (f != 0.0) mags.push_back(f);
        for (uint64_t e = A.ptr[i]; e < A.ptr[i + 1]; e++) {
            f += std::fabs(A.w[e]);
            // every bond sits in the adjacency twice: taken from its lower-numbered end (duplicated bonds are separate terms)
            if (A.nbr[e] > i && A.w[e] != 0.0) mags.push_back(std::fabs(A.w[e]));
        }
        F[i] = f;
        fmax = std::max(fmax, f);
        Q.max_degree = std::max<uint32_t>(Q.max_degree, uint32_t(A.ptr[i + 1] - A.ptr[i]));
    }
    double median = 0.0; // the lower median
    if (!mags.empty()) {
        std::nth_element(mags.begin(), mags.begin() + (mags.size() - 1) / 2, mags.end());
        median = mags[(mags.size() - 1) / 2];
    }
    // the graph's quantum: from the largest local field, but never coarser than 2^-24 of the typical (median) term; sites whose
    // local field is beyond that range (one pinning bias, one enormous bond) are HEAVY: they quantise at their own scale k_i
    const double fbase = std::min(fmax, 64.0 * median);
    Q.k = fbase > 0.0 ? std::ilogb(fbase) + 1 - 30 : 0;
    Q.k_energy = fmax > 0.0 ? std::ilogb(fmax) + 2 - 30 : 0;
    Q.jq.resize(A.w.size());
    Q.hq.assign(nvars, 0);
    Q.dshift.assign(nvars, 0);
    bool dominated = true;
    for (size_t i = 0; i < nvars; i++) {
        const int ki = std::max(Q.k, F[i] > 0.0 ? std::ilogb(F[i]) + 1 - 30 : Q.k);
        if (ki > Q.k) {
            Q.heavy = true;
            Q.dshift[i] = uint8_t(std::min(ki - Q.k, 31));
            double m = biases ? std::fabs(biases[i]) : 0.0;
            for (uint64_t e = A.ptr[i]; e < A.ptr[i + 1]; e++) m = std::max(m, std::fabs(A.w[e]));
            dominated &= 4.0 * m >= 3.0 * F[i]; // then |X_i| >= F_i / 2 whatever the spins
        }
        for (uint64_t e = A.ptr[i]; e < A.ptr[i + 1]; e++) Q.jq[e] = int32_t(std::nearbyint(std::ldexp(A.w[e], -ki)));
        if (biases) Q.hq[i] = int32_t(std::nearbyint(std::ldexp(biases[i], -ki)));
    }
    // the energy of the ORIGINAL couplings in two integer levels: x ~ hi 2^kE + lo 2^(kE - 24)
    const auto levels = [&](double x, int32_t *hi, int32_t *lo) {
        const double h = std::nearbyint(std::ldexp(x, -Q.k_energy));
        *hi = int32_t(h);
        *lo = int32_t(std::nearbyint(std::ldexp(x - std::ldexp(h, Q.k_energy), RJ_ENERGY_LO_BITS - Q.k_energy)));
    };
    Q.jhi.resize(A.w.size());
    Q.jlo.resize(A.w.size());
    for (size_t e = 0; e < A.w.size(); e++) levels(A.w[e], &Q.jhi[e], &Q.jlo[e]);
    Q.hhi.assign(nvars, 0);
    Q.hlo.assign(nvars, 0);
    if (biases)
        for (size_t i = 0; i < nvars; i++) levels(biases[i], &Q.hhi[i], &Q.hlo[i]);
    Q.eligible = Q.max_degree <= 31 && fmax > 0.0 && dominated;
    return Q;
}

void rj_beta(double beta, int k, uint32_t *shift_out, uint32_t *mant_out)
{
    uint32_t shift = 31, mant = 0xFFFFFFFFu; // beta <= 0: every attempt is accepted
    if (beta > 0.0) {
        const double kappa = std::ldexp(0.69314718055994530942 / (2.0 * beta), -k);
        const int e = kappa > 0.0 && std::isfinite(kappa) ? std::ilogb(kappa) : (kappa > 0.0 ? 2000 : -2000);
        const int r = std::max(e - 23, 0);
        if (r <= 31) {
            shift = uint32_t(r);
            mant = uint32_t(std::floor(std::ldexp(kappa, 8 - r))); // kappa 2^-r < 2^24
        }
    }
    *shift_out = shift;
    *mant_out = mant;
}

void rj_log_table(uint32_t *out)
{
    const double h = 1.0 / 2048.0, LOG2E = 1.4426950408889634074;
    out[0] = 0;
    for (int i = 1; i <= 2048; i++) {
        const double x = double(i) * h;
        out[i] = uint32_t(std::nearbyint(std::ldexp(std::log2(1.0 + x) + h * h * LOG2E / (16.0 * (1.0 + x) * (1.0 + x)), 24) + 0.5));
    }
}

} // namespace isingmc

// ---- packed checkerboard planes -> one byte per spin (get_state copy-out, lattice.rs:209-211) ------------
#include <emmintrin.h>
#include <immintrin.h>
namespace isingmc {

// bit k of the index -> byte k of the entry
static const uint64_t *spread_lut()
{
    static uint64_t lut[256];
    static bool ready = [] {
        for (int b = 0; b < 256; b++) {
            uint64_t v = 0;
            for (int k = 0; k < 8; k++) v |= uint64_t((b >> k) & 1) << (8 * k);
            lut[b] = v;
        }
        return true;
    }();
    (void)ready;
    return lut;
}

// STREAM: non-temporal 16-byte stores (the bool arrays are written once and read by the caller much later: without
// the read-for-ownership of ordinary stores the expansion runs 2-2.7x faster, 5.5 -> 11-14 GB/s on 8 threads)
template <bool STREAM>
static void unpack_lattice_impl(uint32_t W, uint32_t H, const uint32_t *words, uint8_t *spins)
{
    const uint64_t *lut = spread_lut();
    const uint32_t wpr = W / 64;
    const size_t wpp = size_t(H) * wpr;
    for (uint32_t y = 0; y < H; y++) {
        // colour c of row y sits at x = 2i + ((y+c)&1): even x is colour (y&1), odd x the other one
        const uint32_t *even = words + (y & 1 ? wpp : 0) + size_t(y) * wpr;
        const uint32_t *odd = words + (y & 1 ? 0 : wpp) + size_t(y) * wpr;
        uint8_t *out = spins + size_t(y) * W;
        for (uint32_t xw = 0; xw < wpr; xw++) {
            const uint32_t we = even[xw], wo = odd[xw];
            for (int k = 0; k < 4; k++) { // 8 + 8 bits -> 16 interleaved bytes
                const __m128i a = _mm_cvtsi64_si128((long long)lut[(we >> (8 * k)) & 0xFF]);
                const __m128i b = _mm_cvtsi64_si128((long long)lut[(wo >> (8 * k)) & 0xFF]);
                if (STREAM) _mm_stream_si128(reinterpret_cast<__m128i *>(out + 64 * xw + 16 * k), _mm_unpacklo_epi8(a, b));
                else _mm_storeu_si128(reinterpret_cast<__m128i *>(out + 64 * xw + 16 * k), _mm_unpacklo_epi8(a, b));
            }
        }
    }
    if (STREAM) _mm_sfence();
}

// AVX-512BW + BMI2 hosts: the two colour words of 64 sites are interleaved into one 64-bit mask by two pdep, and
// vpmovm2b-style (maskz_mov) turns the mask into 64 bytes -- 8 instructions per 64 sites where the table version takes ~32
__attribute__((target("avx512f,avx512bw,bmi2"))) static void unpack_lattice_avx512(uint32_t W, uint32_t H, const uint32_t *words,
                                                                                   uint8_t *spins, bool aligned64)
{
    const uint32_t wpr = W / 64;
    const size_t wpp = size_t(H) * wpr;
    const __m512i ones = _mm512_set1_epi8(1);
    for (uint32_t y = 0; y < H; y++) {
        const uint32_t *even = words + (y & 1 ? wpp : 0) + size_t(y) * wpr; // as unpack_lattice_impl
        const uint32_t *odd = words + (y & 1 ? 0 : wpp) + size_t(y) * wpr;
        uint8_t *out = spins + size_t(y) * W;
        for (uint32_t xw = 0; xw < wpr; xw++) {
            const __mmask64 m = _pdep_u64(even[xw], 0x5555555555555555ull) | _pdep_u64(odd[xw], 0xAAAAAAAAAAAAAAAAull);
            const __m512i v = _mm512_maskz_mov_epi8(m, ones);
            if (aligned64) _mm512_stream_si512(reinterpret_cast<__m512i *>(out + 64 * size_t(xw)), v);
            else _mm512_storeu_si512(out + 64 * size_t(xw), v);
        }
    }
    if (aligned64) _mm_sfence();
}

void unpack_lattice(uint32_t W, uint32_t H, const uint32_t *words, uint8_t *spins)
{
    static const bool avx512 = __builtin_cpu_supports("avx512bw") && __builtin_cpu_supports("bmi2") && !std::getenv("ISINGMC_NO_AVX512");
    if (avx512) {
        unpack_lattice_avx512(W, H, words, spins, (reinterpret_cast<uintptr_t>(spins) & 63u) == 0);
        return;
    }
    if ((reinterpret_cast<uintptr_t>(spins) & 15u) == 0) unpack_lattice_impl<true>(W, H, words, spins); // rows are multiples of 64 bytes
    else unpack_lattice_impl<false>(W, H, words, spins);
}

size_t nonlocal_batch(size_t items, size_t words_per_item, size_t workspace_bytes)
{
    const size_t fit = std::max<size_t>(1, workspace_bytes) / (words_per_item * sizeof(uint32_t));
    return std::min({items, size_t(32768), std::max<size_t>(1, fit)});
}

uint64_t nonlocal_steps_in(uint64_t t0, uint64_t timesteps, uint64_t k)
{
    return k ? (t0 + timesteps) / k - t0 / k : 0; // multiples of k among t + 1 for t in [t0, t0 + timesteps)
}

AutocorrPlan autocorr_plan(uint64_t samples_taken, uint32_t n_lags)
{
    AutocorrPlan P;
    P.samples_taken = samples_taken;
    P.n_lags = n_lags;
    P.live = uint32_t(std::min<uint64_t>(samples_taken, n_lags));
    P.write_slot = uint32_t(samples_taken % n_lags);
    return P;
}

ClassSegments class_segments(const uint32_t *site, size_t n_pos, const uint32_t *cls, size_t nvars, size_t n_tables, size_t n_classes)
{
    ClassSegments S;
    S.sizes.assign(n_tables * n_classes, 0);
    std::vector<uint32_t> start(n_classes + 1);
    for (size_t t = 0; t < n_tables; t++) {
        const uint32_t *c = cls + t * nvars;
        uint64_t *size = S.sizes.data() + t * n_classes;
        for (size_t p = 0; p < n_pos; p++)
            if (site[p] != PAD_SITE && c[site[p]] != CLASS_NONE) size[c[site[p]]]++;
        // counting sort of the positions by class: ascending position inside a class
        const size_t base = S.order.size();
        start[0] = uint32_t(base);
        for (size_t k = 0; k < n_classes; k++) start[k + 1] = start[k] + uint32_t(size[k]);
        S.order.resize(start[n_classes]);
        for (size_t k = 0; k < n_classes; k++)
            for (uint32_t first = start[k]; first < start[k + 1]; first += CLASS_SEGMENT_MAX)
                S.seg.insert(S.seg.end(), {uint32_t(t), uint32_t(k), first, std::min(CLASS_SEGMENT_MAX, start[k + 1] - first)});
        for (size_t p = 0; p < n_pos; p++)
            if (site[p] != PAD_SITE && c[site[p]] != CLASS_NONE) S.order[start[c[site[p]]]++] = uint32_t(p);
    }
    return S;
}

} // namespace isingmc
