// CPU pin of l3d_dev.h: sim_affinity (the similarity of the affinity fill, k_affinity.hip) in the arms no scene reaches.
//   1. The kernel takes ONE exponential, of the minimum of the five arguments.  Line3D::similarity (line3D.cc:1467-1553)
//      takes five exponentials and the minimum of those.  With expf_ref = (float)exp((double)y) for every one of them the two
//      forms must be bit-equal (exp is monotone, fmin skips NaN alike): sim_literal below is that second form.
//   2. sim(h1, h2) == sim(h2, h1) bit for bit: the two position terms trade places, the dot product commutes.  The arm
//      "the reverse candidate exists but fails while I pass" of k_aff_flag is unreachable from the library's own
//      similarities because of this.
// Inputs: random hypotheses, and forced ones -- a length below L3D_EPS on either side; identical, opposite and slightly
// over-long directions (the float dot product exceeds 1: the clamp runs); an angle of exactly 90 degrees; a depth equal to
// the cutoff; med_scene_depth_lines at 0 and around L3D_EPS; k = 0 (a regulariser of 0: NaN at distance 0, -inf beyond);
// all four position terms NaN.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>

#include "../../line3dpp_amd/csrc/l3d_dev.h"

using namespace l3d;

// the five-exponential form: one regulariser, one argument and one exponential per term (the angle, then the four end-point
// distances in the kernel's order), and only then the minimum
static float sim_literal(const HypRec& h1, const HypRec& h2, float k1, float md1, float k2, float md2, float msdl, float two_sigA_sqr) {
    if (h1.length < kEps || h2.length < kEps) return 0.0f;
    const float dot_p = (float)dot(d3{h1.dir[0], h1.dir[1], h1.dir[2]}, d3{h2.dir[0], h2.dir[1], h2.dir[2]});
    float angle = (float)(std::acos((double)std::fmax(std::fmin(dot_p, 1.0f), -1.0f)) / M_PI * 180.0f);
    if (angle > 90.0f) angle = 180.0f - angle;
    const bool cap = msdl > kEps;
    const float cutoff[2] = {cap ? std::fmin(md1, msdl) : md1, cap ? std::fmin(md2, msdl) : md2};
    const float kk[2] = {k1, k2};
    // term t = 2 * side + end: the point `end` of hypothesis `side`, its distance to the OTHER hypothesis's line
    const float dist[4] = {dist_p2l(h2, h1.P1), dist_p2l(h2, h1.P2), dist_p2l(h1, h2.P1), dist_p2l(h1, h2.P2)};
    const float depth[4] = {h1.m.dp1, h1.m.dp2, h2.m.dp1, h2.m.dp2};
    float e[5];
    e[0] = expf_ref(-angle * angle / two_sigA_sqr);
    for (int t = 0; t < 4; ++t) {
        const int side = t / 2;
        const float sigma = (depth[t] > cutoff[side] ? cutoff[side] : depth[t]) * kk[side];
        e[1 + t] = expf_ref(-dist[t] * dist[t] / (2.0f * sigma * sigma));
    }
    return std::fmin(e[0], std::fmin(std::fmin(e[1], e[2]), std::fmin(e[3], e[4])));
}

// bit equality; two NaNs count as equal whatever their payload
static bool same(float a, float b) {
    if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && std::isnan(b);
    return std::memcmp(&a, &b, 4) == 0;
}

int main() {
    std::mt19937_64 rng(20);
    std::uniform_real_distribution<double> U(-1.0, 1.0);
    auto unit = [&](double* v) { double a = U(rng), b = U(rng), c = U(rng), l = std::sqrt(a * a + b * b + c * c) + 1e-30; v[0] = a / l; v[1] = b / l; v[2] = c / l; };
    auto finish = [](HypRec& h, double len) { for (int k = 0; k < 3; ++k) h.P2[k] = h.P1[k] + len * h.dir[k]; h.length = (float)len; h.valid = 1; };
    auto random_hyp = [&](HypRec& h) {
        std::memset(&h, 0, sizeof h);
        for (int k = 0; k < 3; ++k) h.P1[k] = 10 * U(rng);
        unit(h.dir);
        finish(h, 0.1 + 2.5 * (U(rng) + 1));
        h.m.dp1 = (float)(0.5 + 15 * (U(rng) + 1)); h.m.dp2 = (float)(0.5 + 15 * (U(rng) + 1));
    };
    unsigned long n = 0, bad_form = 0, bad_sym = 0, clamp = 0, right_angle = 0, at_cutoff = 0, zero_reg = 0, all_nan = 0, nan_out = 0,
                  short_len = 0, minus_inf = 0, passes = 0;
    const float eps_f = (float)kEps;
    const float msdls[6] = {0.0f, eps_f, std::nextafterf(eps_f, 1.0f), std::nextafterf(eps_f, 0.0f), 4.0f, 12.0f};
    for (int mode = 0; mode < 9; ++mode) {
        const int iters = mode == 0 ? 2000000 : 150000;
        for (int it = 0; it < iters; ++it) {
            HypRec h1, h2;
            random_hyp(h1); random_hyp(h2);
            float k1 = (float)(0.001 + 0.05 * (U(rng) + 1)), k2 = (float)(0.001 + 0.05 * (U(rng) + 1));
            float md1 = (float)(1 + 15 * (U(rng) + 1)), md2 = (float)(1 + 15 * (U(rng) + 1));
            float msdl = msdls[rng() % 6];
            const float two_sig = (rng() & 1) ? 200.0f : 8.0f;
            if (mode == 0 && (it & 1)) {      // nearby lines, so that the position terms are not all far below the threshold
                for (int k = 0; k < 3; ++k) { h2.P1[k] = h1.P1[k] + 0.05 * U(rng); h2.dir[k] = h1.dir[k] + 0.05 * U(rng); }
                const double l = norm(d3{h2.dir[0], h2.dir[1], h2.dir[2]});
                for (int k = 0; k < 3; ++k) h2.dir[k] /= l;
                finish(h2, h2.length);
            }
            if (mode == 1) {                  // a length below L3D_EPS on either side (and exactly L3D_EPS as a float)
                const float tiny[3] = {0.0f, 1e-13f, eps_f};
                if (it & 1) h1.length = tiny[it % 3]; else h2.length = tiny[it % 3];
                if (h1.length < kEps || h2.length < kEps) ++short_len;
            }
            if (mode == 2) {                  // identical, opposite and over-long directions: |float dot| exceeds 1
                const double sgn = (it & 1) ? 1.0 : -1.0, scale = 1.0 + ((it >> 1) % 4) * 1.2e-7;
                for (int k = 0; k < 3; ++k) h2.dir[k] = sgn * h1.dir[k] * scale;
                if ((it >> 3) & 1) for (int k = 0; k < 3; ++k) h1.dir[k] *= scale;
                if ((it >> 4) & 1) h2.dir[it % 3] = std::nextafter(h2.dir[it % 3], 2.0);
            }
            if (mode == 3) {                  // an angle of exactly 90 degrees (not folded), and one ulp to either side
                const int a = it % 3, b = (a + 1) % 3;
                for (int k = 0; k < 3; ++k) { h1.dir[k] = k == a; h2.dir[k] = k == b; }
                if ((it >> 2) % 3 == 1) h2.dir[a] = 1e-17; else if ((it >> 2) % 3 == 2) h2.dir[a] = -1e-17;
                k1 = k2 = 1e3f; msdl = 0.0f;  // wide regularisers: the angle term decides
            }
            if (mode == 4) {                  // a depth equal to the cutoff (the view's median, or the scene's)
                msdl = (it & 1) ? msdl : 0.0f;
                const float c1 = msdl > kEps ? std::fmin(md1, msdl) : md1, c2 = msdl > kEps ? std::fmin(md2, msdl) : md2;
                h1.m.dp1 = c1; h2.m.dp2 = c2;
                if (it & 2) { h1.m.dp2 = std::nextafterf(c1, 100.0f); h2.m.dp1 = std::nextafterf(c2, 0.0f); }
                ++at_cutoff;
            }
            if (mode == 5) msdl = msdls[it % 4];   // med_scene_depth_lines at 0 and around L3D_EPS
            if (mode == 6 || mode == 7) {     // k = 0: a regulariser of 0
                if (it & 1) k1 = 0.0f;
                if (it & 2) k2 = 0.0f;
                if (!(it & 3)) k1 = k2 = 0.0f;
                ++zero_reg;
            }
            if (mode == 7 || mode == 8) {     // the same line, end points on it: every distance is 0
                for (int k = 0; k < 3; ++k) { h1.P1[k] = 0; h1.dir[k] = k == it % 3; h2.P1[k] = (k == it % 3) ? 0.5 : 0.0; h2.dir[k] = h1.dir[k]; }
                finish(h1, 1.0); finish(h2, 2.0);
                if (mode == 7 && !(it & 3)) ++all_nan;
            }
            const float dp = (float)dot(d3{h1.dir[0], h1.dir[1], h1.dir[2]}, d3{h2.dir[0], h2.dir[1], h2.dir[2]});
            if (std::fabs(dp) > 1.0f) ++clamp;
            if (mode == 3 && dp == 0.0f) ++right_angle;
            const float a = sim_affinity(h1, h2, k1, md1, k2, md2, msdl, two_sig);
            const float b = sim_affinity(h2, h1, k2, md2, k1, md1, msdl, two_sig);
            const float c = sim_literal(h1, h2, k1, md1, k2, md2, msdl, two_sig);
            ++n;
            if (!same(a, c)) { if (++bad_form < 10) std::printf("form: mode %d it %d: %a vs %a\n", mode, it, a, c); }
            if (!same(a, b)) { if (++bad_sym < 10) std::printf("symmetry: mode %d it %d: %a vs %a\n", mode, it, a, b); }
            if (std::isnan(a)) ++nan_out;
            if (a == 0.0f && mode == 6) ++minus_inf;
            if (a > kMinAffinity) ++passes;
            if (mode == 7 && !(it & 3) && a != 1.0f) { if (++bad_form < 10) std::printf("all four position terms NaN: %a, not 1\n", a); }
            if (mode == 8 && a != 1.0f) { if (++bad_form < 10) std::printf("the same line: %a, not 1\n", a); }
            if (mode == 3 && dp == 0.0f && a != expf_ref(-90.0f * 90.0f / two_sig)) { if (++bad_form < 10) std::printf("90 degrees: %a\n", a); }
        }
    }
    std::printf("%lu cases (%lu above 0.5): clamp ran %lu times, exact right angles %lu, depth at the cutoff %lu, zero regulariser %lu "
                "(similarity 0: %lu), all position terms NaN %lu, short hypotheses %lu, NaN results %lu\n",
                n, passes, clamp, right_angle, at_cutoff, zero_reg, minus_inf, all_nan, short_len, nan_out);
    const bool reached = clamp > 1000 && right_angle > 1000 && all_nan > 1000 && short_len > 1000 && minus_inf > 1000 && passes > 100000;
    std::printf("one exponential of the minimum vs five exponentials: %s, %lu mismatches\n", bad_form ? "DIFFERENT" : "identical", bad_form);
    std::printf("sim(h1, h2) vs sim(h2, h1): %s, %lu asymmetric\n", bad_sym ? "DIFFERENT" : "symmetric", bad_sym);
    if (!reached) std::printf("an arm was not reached\n");
    return (bad_form || bad_sym || !reached) ? 1 : 0;
}
