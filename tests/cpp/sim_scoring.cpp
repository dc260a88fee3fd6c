// CPU pin of l3d_dev.h: the scoring similarity of phase B (k_lists.hip, k_views.hip) at its thresholds.
// Line3D::similarityForScoring (line3D.cc:1417-1446, with angleBetweenSeg3D :1571-1583) takes three expf and one acos and
// compares the minimum with 0.5; the kernels compare the ARGUMENTS with thresholds that sim_thresholds finds by bisection,
// look for candidates inside padded depth windows only, and decide the angle in fp32 away from the thresholds.
//   1. thresholds  every float within 2^16 ulp of y_thr, x_hi, x_lo, 0 and +-1 and a stride over the rest: the comparison
//                  equals the reference's expression and never flips back (the monotonicity the bisection assumes)
//   2. sim_decide  against the reference on tuples forced to within +-3 ulp of a threshold in any component, with NaN,
//                  -inf, denormal, infinite and overflowing terms, zero lengths, dot products above 1 and exactly 0
//   3. sim_far     the division-free early-out never drops a tuple the reference accepts, over the float range of reg
//   4. windows     window_sq and support_radius hold every depth difference the reference accepts
//   5. fp32 angle  dir_decide32: certain => the fp64 decision, for directions unprojected next to a threshold
//   6. sim_value   equal or adjacent to the reference's fmin of three expf
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../line3dpp_amd/csrc/l3d_dev.h"

using namespace l3d;

// ---- the reference, literally ------------------------------------------------------------------------------------------
static float ref_angle(float dot_p) {   // angleBetweenSeg3D(s1, s2, undirected = true)
    float angle = (float)(std::acos((double)std::fmax(std::fmin(dot_p, 1.0f), -1.0f)) / M_PI * 180.0f);
    if (angle > 90.0f) angle = 180.0f - angle;
    return angle;
}
static float ref_similarity(const d3& dir1, float len1, const d3& dir2, float len2, float a1, float a2, float b1, float b2,
                            float reg1, float reg2, float two_sigA_sqr) {
    if (len1 < kEps || len2 < kEps) return 0.0f;
    const float dot_p = (float)dot(dir1, dir2);
    const float angle = ref_angle(dot_p);
    const float sim_a = expf(-angle * angle / two_sigA_sqr);
    const float d1 = a1 - b1;
    const float d2 = a2 - b2;
    const float sim_p = std::fmin(expf(-d1 * d1 / reg1), expf(-d2 * d2 / reg2));
    const float sim = std::fmin(sim_a, sim_p);
    return sim > 0.5f ? sim : 0.0f;
}

// ---- floats as a line of integers (-0 and +0 share 0) ---------------------------------------------------------------------
static int64_t ord(float f) { int32_t i; std::memcpy(&i, &f, 4); return i < 0 ? -(int64_t)(i & 0x7FFFFFFF) : (int64_t)i; }
static float unord(int64_t o) {
    const uint32_t u = o < 0 ? (0x80000000u | (uint32_t)(-o)) : (uint32_t)o;
    float f; std::memcpy(&f, &u, 4); return f;
}
static float step(float f, int64_t n) { return unord(ord(f) + n); }

static unsigned long g_bad = 0;
static bool g_reached = true;
static void bad(const char* what, double a = 0, double b = 0, double c = 0) {
    if (++g_bad < 20) std::printf("MISMATCH %s: %a %a %a\n", what, a, b, c);
}
static void need(bool cond, const char* what) { if (!cond) { g_reached = false; std::printf("not reached: %s\n", what); } }

static const d3 kAxis[3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
// two directions whose double dot product is exactly x: an axis, and x along it plus the rest along another axis
static void dirs_with_dot(float x, int a, d3& da, d3& db) {
    da = kAxis[a];
    const double s = std::sqrt(std::fmax(0.0, 1.0 - (double)x * x));
    db = kAxis[a] * (double)x + kAxis[(a + 1) % 3] * s;
}
static bool decide_angle(float x, const SimConst sc) {   // sim_decide with both position terms at -0
    d3 da, db; dirs_with_dot(x, 0, da, db);
    return sim_decide(da, false, 1.0f, 1.0f, 1.0f, 1.0f, db, false, 1.0f, 1.0f, sc);
}

// ---- 1. thresholds -------------------------------------------------------------------------------------------------------
static void add_window(std::vector<int64_t>& v, float centre, int64_t lo, int64_t hi) {
    const int64_t c = ord(centre);
    for (int64_t o = std::max(c - 65536, lo); o <= std::min(c + 65536, hi); ++o) v.push_back(o);
}
static void thresholds() {
    const float sigmas[9] = {0.3f, 1.0f, 5.0f, 10.0f, 45.0f, 76.4f, 76.45f, 80.0f, 90.0f};
    unsigned long n_y = 0, n_x = 0, two_form = 0, zero_form = 0;
    for (float sigma : sigmas) {
        const float tsq = 2.0f * sigma * sigma;
        const SimConst sc = sim_thresholds(tsq);
        // the exponent: [-2, 0] and a little beyond 0
        std::vector<int64_t> ys;
        const int64_t ylo = ord(-2.0f), yhi = ord(1e-30f);
        add_window(ys, sc.y_thr, ylo, yhi); add_window(ys, 0.0f, ylo, yhi); add_window(ys, -2.0f, ylo, yhi);
        for (int64_t o = ylo; o <= 0; o += 2039) ys.push_back(o);
        std::sort(ys.begin(), ys.end()); ys.erase(std::unique(ys.begin(), ys.end()), ys.end());
        bool seen = false;
        for (int64_t o : ys) {
            const float y = unord(o);
            const bool want = expf(y) > 0.5f, got = y > sc.y_thr;
            if (want != got) bad("y > y_thr", y, sc.y_thr);
            if (want) seen = true; else if (seen) bad("expf(y) > 0.5 flips back", y);
            ++n_y;
        }
        // the dot product: [-1, 1] and 2^16 ulp beyond either end (the clamp)
        std::vector<int64_t> xs;
        const int64_t xlo = ord(-1.0f) - 65536, xhi = ord(1.0f) + 65536;
        add_window(xs, sc.x_hi, xlo, xhi); add_window(xs, sc.x_lo, xlo, xhi); add_window(xs, 0.0f, xlo, xhi);
        add_window(xs, 1.0f, xlo, xhi); add_window(xs, -1.0f, xlo, xhi);
        for (int64_t o = xlo; o <= xhi; o += 4093) xs.push_back(o);
        std::sort(xs.begin(), xs.end()); xs.erase(std::unique(xs.begin(), xs.end()), xs.end());
        auto check = [&](float x, bool& seen_true) {
            const float angle = ref_angle(x);
            const bool want = expf(-angle * angle / tsq) > 0.5f, got = decide_angle(x, sc);
            if (want != got) bad("x >= x_hi || x <= x_lo", x, sc.x_hi, sc.x_lo);
            if (want) seen_true = true; else if (seen_true) bad("the angular term flips back", x, sigma);
            ++n_x;
        };
        bool up = false, down = false;
        for (size_t i = 0; i < xs.size(); ++i) if (xs[i] >= 0) check(unord(xs[i]), up);        // 0 ... 1 and beyond
        for (size_t i = xs.size(); i-- > 0;) if (xs[i] <= 0) check(unord(xs[i]), down);        // 0 ... -1 and beyond
        const bool zero = sc.x_hi == 0.0f && sc.x_lo == 0.0f;
        if (zero) ++zero_form; else ++two_form;
        // (x_lo need not be -x_hi: 180 - angle rounds once more)
        if (!zero && !(sc.x_hi > 0.0f && sc.x_hi <= 1.0f && sc.x_lo < 0.0f && sc.x_lo >= -1.0f)) bad("x_hi, x_lo", sc.x_hi, sc.x_lo);
        std::printf("sigma_a %-6g two_sigA_sqr %-9g y_thr %a x_hi %a x_lo %a%s\n", sigma, tsq, sc.y_thr, sc.x_hi, sc.x_lo,
                    zero ? "  (every direction passes)" : "");
    }
    std::printf("thresholds: %lu exponents, %lu dot products; %lu two-threshold forms, %lu x_hi == 0 forms\n", n_y, n_x, two_form, zero_form);
    need(two_form >= 6 && zero_form >= 3, "both forms of the angular thresholds");
}

// ---- tuples --------------------------------------------------------------------------------------------------------------
struct Rng {
    std::mt19937_64 g{2024};
    std::uniform_real_distribution<double> u{0.0, 1.0};
    double U() { return u(g); }
    double S() { return 2.0 * u(g) - 1.0; }
    double logu(double lo10, double hi10) { return std::pow(10.0, lo10 + (hi10 - lo10) * u(g)); }
    uint64_t operator()() { return g(); }
    d3 unit() { for (;;) { d3 v{S(), S(), S()}; const double n = norm(v); if (n > 0.1 && n <= 1.0) return v * (1.0 / n); } }
};

// (d, reg) with -d * d / reg == y_thr + n ulp in float arithmetic, reg near `reg`; false if the neighbourhood has none
static bool force_y(float y_thr, int n, float reg, float& d_out, float& reg_out) {
    const float yt = step(y_thr, n);
    const float d0 = (float)std::sqrt(-(double)yt * (double)reg);
    for (int dd = 0; dd <= 8; ++dd)
        for (int rr = 0; rr <= 16; ++rr) {
            const float d = step(d0, (dd & 1) ? -(dd + 1) / 2 : dd / 2), r = step(reg, (rr & 1) ? -(rr + 1) / 2 : rr / 2);
            if (-d * d / r == yt) { d_out = d; reg_out = r; return true; }
        }
    return false;
}

static void forced_tuples() {
    Rng rng;
    const float sigmas[4] = {1.0f, 10.0f, 45.0f, 80.0f};
    SimConst scs[4];
    for (int i = 0; i < 4; ++i) scs[i] = sim_thresholds(2.0f * sigmas[i] * sigmas[i]);
    unsigned long n = 0, accepted = 0, arm_y[2][7] = {}, arm_x[2][7] = {}, nan_terms = 0, all_nan = 0, minus_inf = 0, zero_len[2] = {},
                  denorm = 0, inf_reg = 0, overflow = 0, clamp = 0, dot_zero = 0, far_form = 0;
    const float eps_f = (float)kEps;
    for (int it = 0; it < 6000000; ++it) {
        const float sigma = sigmas[it & 3];
        const float tsq = 2.0f * sigma * sigma;
        const SimConst sc = scs[it & 3];
        float a[2], b[2], reg[2];
        int near_n[2] = {99, 99};
        for (int c = 0; c < 2; ++c) {
            const unsigned mode = rng() % 10;
            float d = 0.0f;
            reg[c] = (float)rng.logu(-30, 30);
            if (mode <= 1) d = (float)(std::sqrt((double)reg[c]) * 0.3 * rng.U());                   // far inside
            else if (mode <= 4) {                                                                      // at the threshold
                const int nn = (int)(rng() % 7) - 3;
                if (force_y(sc.y_thr, nn, reg[c], d, reg[c])) near_n[c] = nn;
            }
            else if (mode == 5) { reg[c] = 0.0f; d = 0.0f; }                                           // NaN
            else if (mode == 6) { reg[c] = 0.0f; d = (float)rng.logu(-20, 10); }                       // -inf
            else if (mode == 7) {                                                                      // denormal / infinite reg
                if (rng() & 1) { reg[c] = unord(1 + (int64_t)(rng() % 8388607)); d = (rng() & 1) ? 0.0f : std::sqrt(reg[c]) * (float)rng.U(); ++denorm; }
                else { reg[c] = INFINITY; d = (rng() & 1) ? (float)rng.logu(-20, 30) : INFINITY; ++inf_reg; }
            }
            else if (mode == 8) { d = (float)rng.logu(19.3, 38); if (rng() & 1) reg[c] = (float)rng.logu(30, 38.5); ++overflow; }   // d * d = inf
            else d = (float)(std::sqrt((double)reg[c]) * 1.2 * rng.U());                               // anywhere around
            // d is the difference itself: one side is 0
            if (rng() & 1) { a[c] = d; b[c] = 0.0f; } else { a[c] = 0.0f; b[c] = d; }
        }
        d3 da, db;
        const unsigned am = rng() % 10;
        int near_x = 99, which = 0;
        if (am <= 1) { da = rng.unit(); db = da; }
        else if (am <= 5) {
            const int nn = (int)(rng() % 7) - 3;
            which = (int)(rng() & 1);
            dirs_with_dot(step(which ? sc.x_lo : sc.x_hi, nn), (int)(rng() % 3), da, db);
            near_x = nn;
        }
        else if (am == 6) { da = rng.unit(); db = da * ((rng() & 1 ? 1.0 : -1.0) * (1.0 + (1 + rng() % 4) * 1.2e-7)); }   // |dot| > 1
        else if (am == 7) { const int ax = (int)(rng() % 3); da = kAxis[ax]; db = kAxis[(ax + 1 + rng() % 2) % 3]; }      // dot == 0
        else { da = rng.unit(); db = rng.unit(); }
        float len[2] = {1.0f, 1.0f};
        if (rng() % 16 == 0) { const float tiny[4] = {0.0f, 1e-13f, eps_f, std::nextafterf(eps_f, 1.0f)}; const int s = (int)(rng() & 1); len[s] = tiny[rng() % 4]; ++zero_len[s]; }

        const float want = ref_similarity(da, len[0], db, len[1], a[0], a[1], b[0], b[1], reg[0], reg[1], tsq);
        const bool got = sim_decide(da, len[0] < kEps, a[0], a[1], reg[0], reg[1], db, len[1] < kEps, b[0], b[1], sc);
        if (got != (want > 0.0f)) bad("sim_decide", want, sigma, it);
        // the form of k_views.hip: the early-out in front
        const float d1 = a[0] - b[0], d2 = a[1] - b[1];
        const bool far = sim_far(d1, d2, reg[0], reg[1]);
        if ((!far && got) != (want > 0.0f)) bad("!sim_far && sim_decide", want, sigma, it);
        if (got) {
            const float v = sim_value(da, a[0], a[1], reg[0], reg[1], db, b[0], b[1], sc);
            if (std::llabs(ord(v) - ord(want)) > 1) bad("sim_value", v, want, it);
        }
        ++n; accepted += got; far_form += far;
        const float y1 = -d1 * d1 / reg[0], y2 = -d2 * d2 / reg[1];
        nan_terms += (y1 != y1) + (y2 != y2); all_nan += (y1 != y1) && (y2 != y2);
        minus_inf += (y1 == -INFINITY) + (y2 == -INFINITY);
        if (near_n[0] != 99 && ord(y1) - ord(sc.y_thr) == near_n[0]) ++arm_y[0][near_n[0] + 3];
        if (near_n[1] != 99 && ord(y2) - ord(sc.y_thr) == near_n[1]) ++arm_y[1][near_n[1] + 3];
        const float dp = (float)dot(da, db);
        if (near_x != 99 && dp == step(which ? sc.x_lo : sc.x_hi, near_x)) ++arm_x[which][near_x + 3];
        clamp += std::fabs(dp) > 1.0f; dot_zero += dp == 0.0f;
    }
    std::printf("forced tuples: %lu cases, %lu accepted, %lu past the early-out; NaN terms %lu (both: %lu), -inf terms %lu, zero length %lu + %lu, "
                "denormal reg %lu, infinite reg %lu, d*d overflow %lu, |dot| > 1 %lu, dot == 0 %lu\n",
                n, accepted, far_form, nan_terms, all_nan, minus_inf, zero_len[0], zero_len[1], denorm, inf_reg, overflow, clamp, dot_zero);
    for (int c = 0; c < 2; ++c) {
        std::printf("  y%d at y_thr-3 ... +3 ulp:", c + 1);
        for (int k = 0; k < 7; ++k) { std::printf(" %lu", arm_y[c][k]); need(arm_y[c][k] > 10000, "a step of y around y_thr"); }
        std::printf("\n");
    }
    for (int c = 0; c < 2; ++c) {
        std::printf("  x at %s-3 ... +3 ulp:", c ? "x_lo" : "x_hi");
        for (int k = 0; k < 7; ++k) { std::printf(" %lu", arm_x[c][k]); need(arm_x[c][k] > 10000, "a step of x around a threshold"); }
        std::printf("\n");
    }
    need(accepted > 100000 && all_nan > 10000 && minus_inf > 100000 && zero_len[0] > 10000 && zero_len[1] > 10000 && denorm > 100000 &&
         inf_reg > 100000 && overflow > 100000 && clamp > 100000 && dot_zero > 100000 && far_form > 100000, "an arm of the forced tuples");
}

// ---- 3. the early-out over the float range of reg ------------------------------------------------------------------------
static void early_out() {
    Rng rng;
    unsigned long n = 0, n_far = 0, lost = 0;
    float y_max = -INFINITY;
    const SimConst sc = sim_thresholds(200.0f);
    const d3 dir = kAxis[0];
    auto one = [&](float d, float reg) {
        ++n;
        if (!sim_far(d, 0.0f, reg, 1.0f)) return;
        ++n_far;
        const float y = -d * d / reg;
        if (!(y <= sc.y_thr)) { ++lost; bad("early-out: the term is NaN or passes", d, reg, y); }
        if (y > y_max) y_max = y;
        // as the first and as the second term, against identical directions and a passing other term
        if (ref_similarity(dir, 1.0f, dir, 1.0f, d, 0.0f, 0.0f, 0.0f, reg, 1.0f, 200.0f) > 0.0f ||
            ref_similarity(dir, 1.0f, dir, 1.0f, 0.0f, 0.0f, 0.0f, d, 1.0f, reg, 200.0f) > 0.0f) { ++lost; bad("early-out drops an accepted tuple", d, reg); }
        if (!sim_far(0.0f, d, 1.0f, reg)) bad("early-out: second term", d, reg);
    };
    for (int64_t e = 0; e < 255; ++e)                    // every exponent, denormals included
        for (int m = 0; m < 12000; ++m) {
            uint32_t u = ((uint32_t)e << 23) | (m < 4 ? (m == 0 ? 0u : m == 1 ? 1u : m == 2 ? 0x7FFFFFu : 0x400000u) : (uint32_t)(rng() & 0x7FFFFF));
            float reg; std::memcpy(&reg, &u, 4);
            // the smallest d with d * d > 0.72f * reg, found float by float from the root
            float d = (float)std::sqrt(0.72 * (double)reg);
            for (int s = 0; s < 64 && d * d > 0.72f * reg && d > 0.0f; ++s) d = step(d, -1);
            for (int s = 0; s < 64 && !(d * d > 0.72f * reg); ++s) d = step(d, 1);
            one(d, reg); one(step(d, 1), reg); one(step(d, 2), reg); one(-d, reg); one(step(d, -1), reg);
            one(d * 1.0001f, reg); one(d * (float)(1.0 + rng.U()), reg); one((float)rng.logu(-45, 38), reg); one(INFINITY, reg);
        }
    // (a regulariser is a sum of squares: never negative)
    const float special[3] = {0.0f, INFINITY, NAN};
    for (float reg : special)
        for (int m = 0; m < 1000; ++m) { one((float)rng.logu(-45, 38), reg); one(0.0f, reg); one(INFINITY, reg); one(NAN, reg); }
    std::printf("early-out: %lu cases, %lu past it, the largest exponent among those %.9g (y_thr %.9g); %lu accepted by the reference\n",
                n, n_far, y_max, sc.y_thr, lost);
    need(n_far > 1000000, "the early-out");
}

// ---- 4. + 5. geometry ------------------------------------------------------------------------------------------------------
struct Geo {
    double C[3], Ct[3], r1[3], r2[3];
    float k, kt, cc_dist;
};
static void put(double* o, const d3& v) { o[0] = v.x; o[1] = v.y; o[2] = v.z; }
static Geo random_geo(Rng& rng, bool aligned) {
    Geo g;
    const d3 c = rng.unit() * rng.logu(-2, 4);
    const d3 r1 = rng.unit();
    d3 p = cross(r1, rng.unit()); p = normalized(p);
    const d3 r2 = normalized(r1 + p * rng.logu(-3.5, -0.3));       // the segment subtends 3e-4 ... 0.5 rad
    const double cc = rng.logu(-3, 3);
    const d3 t = aligned ? r1 * ((rng() & 1) ? -1.0 : 1.0) : rng.unit();
    put(g.C, c); put(g.Ct, c + t * cc); put(g.r1, r1); put(g.r2, r2);
    g.k = (float)rng.logu(-5, -1); g.kt = (float)rng.logu(-5, -1);
    // l3d_api.hip: |C_src - C_tgt|, rounded up
    g.cc_dist = std::nextafterf((float)(norm(c - d3{g.Ct[0], g.Ct[1], g.Ct[2]}) * (1.0 + 1e-6)), INFINITY);
    return g;
}
// the two regularisers of hypothesis (a1, a2), as exact_support (k_lists.hip) and make_dentry (k_views.hip) compute them
static void regs_of(const Geo& g, float a1, float a2, float& reg1, float& reg2) {
    const Seg3 si = unproject(g.C, g.r1, g.r2, a1, a2);
    const float sig1 = a1 * g.k, sig2 = a2 * g.k;
    reg1 = 2.0f * sig1 * sig1; reg2 = 2.0f * sig2 * sig2;
    const d3 ct{g.Ct[0], g.Ct[1], g.Ct[2]};
    const float sig1_t = (float)(norm(si.P1 - ct) * (double)g.kt);
    const float sig2_t = (float)(norm(si.P2 - ct) * (double)g.kt);
    reg1 = 0.5f * (reg1 + 2.0f * sig1_t * sig1_t);
    reg2 = 0.5f * (reg2 + 2.0f * sig2_t * sig2_t);
}

static void windows() {
    Rng rng;
    const SimConst sc = sim_thresholds(200.0f);
    unsigned long n = 0, outside = 0;
    double min_w = INFINITY, min_r = INFINITY;
    for (int it = 0; it < 1500000; ++it) {
        const Geo g = random_geo(rng, (it & 3) == 0);
        const float a1 = (float)rng.logu(-2, 4), a2 = (float)(a1 * (1.0 + 0.3 * rng.S()));
        float reg[2];
        regs_of(g, a1, a2, reg[0], reg[1]);
        const float a[2] = {a1, a2};
        for (int c = 0; c < 2; ++c) {
            if (!(reg[c] > 0.0f) || !std::isfinite(reg[c])) continue;
            const double lim = std::sqrt(-(double)sc.y_thr * (double)reg[c]);
            for (int sgn = -1; sgn <= 1; sgn += 2) {
                // the farthest supporter depth the reference's term still accepts: from just outside, float by float inwards
                float b = (float)((double)a[c] + sgn * lim * (1.0 + 1e-6));
                for (int s = 0; s < 8; ++s) b = std::nextafterf(b, sgn * INFINITY);
                bool ok = false;
                for (int s = 0; s < 200 && b != a[c]; ++s, b = std::nextafterf(b, a[c])) {
                    const float d = a[c] - b;
                    if (expf(-d * d / reg[c]) > 0.5f) { ok = true; break; }
                }
                if (!ok) continue;     // the depth's own ulp is wider than the window: only d == 0 is accepted
                const float d = a[c] - b;
                const float W = window_sq(a[c], g.k, g.kt, g.cc_dist);
                ++n;
                if (!(d * d <= W)) { ++outside; bad("window_sq", d, W, reg[c]); }
                min_w = std::fmin(min_w, (double)W / ((double)d * (double)d));
                if (c == 0) {          // k_support's window is on the first depth
                    float r = support_radius(reg[0]);
                    if (!(r < 1e30f)) r = INFINITY;
                    const float kl = a1 - r, kh = a1 + r;
                    if (!(std::fabs(d) <= r) || !(b >= kl) || !(b <= kh)) { ++outside; bad("support_radius", d, r, reg[0]); }
                    min_r = std::fmin(min_r, (double)r / std::fabs((double)d));
                }
            }
        }
    }
    std::printf("windows: %lu accepted extremes, %lu outside; smallest window_sq / d^2 = %.6f, smallest radius / |d| = %.6f\n", n, outside, min_w, min_r);
    need(n > 2000000, "the windows");
}

static void angular_fp32() {
    Rng rng;
    const float sigmas[4] = {1.0f, 5.0f, 10.0f, 45.0f};
    SimConst scs[4];
    for (int i = 0; i < 4; ++i) scs[i] = sim_thresholds(2.0f * sigmas[i] * sigmas[i]);
    unsigned long n = 0, near = 0, certain_n = 0, wrong = 0, near_hi = 0, near_lo = 0;
    double max_diff = 0.0;
    for (int it = 0; it < 400000; ++it) {
        const float sigma = sigmas[it & 3];
        const SimConst sc = scs[it & 3];
        const Geo g = random_geo(rng, false);
        const float a1 = (float)rng.logu(-2, 4), a2 = (float)(a1 * (1.0 + 0.3 * rng.S()));
        const Seg3 sa = unproject(g.C, g.r1, g.r2, a1, a2);
        if (!(sa.length > 0.0f)) continue;
        const float b1 = (float)(a1 * (1.0 + 0.1 * rng.S()));
        const bool lo_side = (it >> 2) & 1;
        const double target = lo_side ? (double)sc.x_lo : (double)sc.x_hi;
        auto f = [&](double b2) { const Seg3 sb = unproject(g.C, g.r1, g.r2, b1, (float)b2); return dot(sa.dir, sb.dir) - target; };
        double lo = b1 * 1e-4, hi = b1 * 1e4;
        // the direction of b turns from -r1 (b2 -> 0) to r2 (b2 -> inf): a sign change between two of these points brackets a root
        const double pts[5] = {lo, b1 * 0.5, (double)b1 * (1.0 + 1e-3 * rng.S()), b1 * 2.0, hi};
        int seg = -1;
        double fp[5];
        for (int i = 0; i < 5; ++i) fp[i] = f(pts[i]);
        const int first = (int)(rng() % 4);
        for (int i = 0; i < 4; ++i) { const int j = (first + i) % 4; if ((fp[j] < 0) != (fp[j + 1] < 0)) { seg = j; break; } }
        if (seg < 0) continue;
        lo = pts[seg]; hi = pts[seg + 1];
        const bool lo_neg = fp[seg] < 0;
        for (int s = 0; s < 60; ++s) { const double m = 0.5 * (lo + hi); if ((f(m) < 0) == lo_neg) lo = m; else hi = m; }
        const int64_t stride = 1 + (int64_t)(rng() % 48);
        for (int s = -12; s <= 12; ++s) {
            const float b2 = step((float)lo, s * stride);
            const Seg3 sb = unproject(g.C, g.r1, g.r2, b1, b2);
            if (!(sb.length > 0.0f)) continue;
            const double xd = dot(sa.dir, sb.dir);
            const float x = fmaxf(fminf((float)xd, 1.0f), -1.0f);
            // k_support: directions staged as floats, the dot product summed left to right
            const float ax = (float)sa.dir.x, ay = (float)sa.dir.y, az = (float)sa.dir.z, bx = (float)sb.dir.x, by = (float)sb.dir.y, bz = (float)sb.dir.z;
            const float xf = fmaxf(fminf(ax * bx + ay * by + az * bz, 1.0f), -1.0f);
            ++n;
            max_diff = std::fmax(max_diff, std::fabs((double)xf - (double)x));
            if (!(std::fabs(xd - sc.x_hi) < 1e-5 || std::fabs(xd - sc.x_lo) < 1e-5)) continue;
            ++near; if (lo_side) ++near_lo; else ++near_hi;
            const int d32 = dir_decide32(xf, sc);
            const bool exact = x >= sc.x_hi || x <= sc.x_lo;
            if (d32 >= 0) { ++certain_n; if ((d32 != 0) != exact) { ++wrong; bad("dir_decide32 certain but different", xf, x, sigma); } }
        }
    }
    std::printf("fp32 angle: %lu direction pairs, %lu within 1e-5 of a threshold (x_hi %lu, x_lo %lu), %lu of them certain, %lu of those wrong; "
                "largest |xf - x| = %.4g (kDirSlack %.4g)\n", n, near, near_hi, near_lo, certain_n, wrong, max_diff, (double)kDirSlack);
    if (!(max_diff < (double)kDirSlack)) bad("|xf - x| reaches kDirSlack", max_diff);
    need(near_hi > 1000000 && near_lo > 1000000 && certain_n > 500000 && near - certain_n > 500000, "the fp32 angular path");
}

// ---- 6. the value ------------------------------------------------------------------------------------------------------------
static void values() {
    Rng rng;
    const float sigmas[3] = {1.0f, 10.0f, 80.0f};
    SimConst scs[3];
    for (int i = 0; i < 3; ++i) scs[i] = sim_thresholds(2.0f * sigmas[i] * sigmas[i]);
    unsigned long n = 0, accepted = 0, differ = 0, at_most_half = 0, far_off = 0;
    for (int it = 0; it < 6000000; ++it) {
        const float sigma = sigmas[it % 3];
        const float tsq = 2.0f * sigma * sigma;
        const SimConst sc = scs[it % 3];
        float a[2], b[2], reg[2];
        for (int c = 0; c < 2; ++c) {
            reg[c] = (float)rng.logu(-8, 8);
            a[c] = (float)rng.logu(-2, 4);
            const unsigned mode = rng() % 8;
            const double w = mode == 0 ? 0.0 : mode <= 2 ? 0.8326 * (1.0 - 1e-6 * rng.U()) : 0.9 * rng.U();   // 0.8326 = sqrt(ln 2)
            b[c] = (float)(a[c] + ((rng() & 1) ? 1.0 : -1.0) * w * std::sqrt((double)reg[c]));
            if (mode == 7) { reg[c] = 0.0f; b[c] = a[c]; }        // NaN: drops out
        }
        const d3 da = rng.unit();
        d3 p = normalized(cross(da, rng.unit()));
        const double amax = std::fmin(sigma * 0.8326 * std::sqrt(2.0), 90.0) / 180.0 * M_PI;      // where the angular term is 0.5
        const unsigned am = rng() % 4;
        const double ang = am == 0 ? 0.0 : am == 1 ? amax * (1.0 - 1e-6 * rng.U()) : 1.1 * amax * rng.U();
        d3 db = da * std::cos(ang) + p * std::sin(ang);
        if (rng() & 1) db = db * -1.0;
        ++n;
        if (!sim_decide(da, false, a[0], a[1], reg[0], reg[1], db, false, b[0], b[1], sc)) continue;
        ++accepted;
        const float v = sim_value(da, a[0], a[1], reg[0], reg[1], db, b[0], b[1], sc);
        const float want = ref_similarity(da, 1.0f, db, 1.0f, a[0], a[1], b[0], b[1], reg[0], reg[1], tsq);
        const int64_t du = std::llabs(ord(v) - ord(want));
        if (du > 1) { ++far_off; bad("sim_value more than 1 ulp from the reference", v, want, sigma); }
        differ += du == 1;
        at_most_half += v <= 0.5f;
    }
    std::printf("sim_value: %lu cases, %lu accepted; %lu differ from the reference by one ulp, %lu by more; %lu accepted with a value <= 0.5\n",
                n, accepted, differ, far_off, at_most_half);
    need(accepted > 1000000, "sim_value");
}

int main() {
    thresholds();
    forced_tuples();
    early_out();
    windows();
    angular_fp32();
    values();
    std::printf("decision and value forms vs similarityForScoring: %s, %lu mismatches\n", g_bad ? "DIFFERENT" : "identical", g_bad);
    if (!g_reached) std::printf("an arm was not reached\n");
    return (g_bad || !g_reached) ? 1 : 0;
}
