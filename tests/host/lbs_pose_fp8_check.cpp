// Host check of the e4m3 pose-correction operands (csrc/k2b_lbs_fp8.h, pose_fp8_strips of k2b_model_tables.h) and of the route
// rule that selects them (lbs_route of k2b_lbs_plan.h), against definitions written out a second time: 17-24 joints x 1-24 shape
// coefficients, the mesh and a 21-vertex subset of it.  No HIP; built with the address and undefined-behaviour sanitizers.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "k2b_lbs_plan.h"
#include "k2b_model_tables.h"

using namespace k2b;

static int failures = 0;
#define CHECK(cond, ...)                                                           \
    do {                                                                           \
        if (!(cond)) {                                                             \
            if (++failures <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                          \
    } while (0)

// the value of a code, from the format's definition (bias 7, subnormals at exponent field 0, 0x7f / 0xff NaN)
static double value_of(int c) {
    const int e = (c >> 3) & 15, m = c & 7;
    if (e == 15 && m == 7) return NAN;
    const double mag = e == 0 ? m * std::ldexp(1.0, -9) : (1.0 + m / 8.0) * std::ldexp(1.0, e - 7);
    return (c & 0x80) ? -mag : mag;
}
// nearest finite value, ties to the even code, saturating
static uint8_t encode_by_search(double x) {
    if (std::isnan(x)) return (uint8_t)(0x7f | (std::signbit(x) ? 0x80 : 0));
    const double a = std::fabs(x);
    int best = 0;
    for (int c = 1; c <= 0x7e; ++c) {
        const double d = std::fabs(value_of(c) - a), db = std::fabs(value_of(best) - a);
        if (d < db || (d == db && (c & 1) == 0)) best = c;
    }
    return (uint8_t)(best | (std::signbit(x) ? 0x80 : 0));
}

static void check_encoder() {
    for (int c = 0; c < 256; ++c) {
        const double v = value_of(c);
        if (std::isnan(v)) { CHECK(std::isnan(e4m3_decode((uint8_t)c)), "decode of NaN code %d", c); continue; }
        CHECK((double)e4m3_decode((uint8_t)c) == v, "decode(%d) = %g, want %g", c, (double)e4m3_decode((uint8_t)c), v);
        CHECK(e4m3_encode((float)v) == c, "encode(decode(%d)) = %d", c, (int)e4m3_encode((float)v));
    }
    std::mt19937 rng(5);
    std::uniform_real_distribution<double> ex(-12.0, 10.0);
    for (int i = 0; i < 20000; ++i) {
        const float x = (float)(std::exp2(ex(rng)) * ((rng() & 1) ? -1.0 : 1.0));
        CHECK(e4m3_encode(x) == encode_by_search(x), "encode(%a) = %d, want %d", (double)x, (int)e4m3_encode(x), (int)encode_by_search(x));
    }
    for (int c = 0; c < 0x7e; ++c) {                       // midpoints of neighbours and their fp32 neighbours
        const float mid = (float)((value_of(c) + value_of(c + 1)) / 2);
        for (const float x : {mid, std::nextafterf(mid, 0.f), std::nextafterf(mid, 1e9f), -mid})
            CHECK(e4m3_encode(x) == encode_by_search(x), "tie %a: %d, want %d", (double)x, (int)e4m3_encode(x), (int)encode_by_search(x));
    }
    CHECK(e4m3_encode(1e30f) == 0x7e && e4m3_encode(-INFINITY) == 0xfe && e4m3_encode(464.f) == 0x7e, "saturation");
    CHECK(e4m3_encode(0.f) == 0 && e4m3_encode(-0.f) == 0x80 && e4m3_encode(NAN) == 0x7f, "zeros and NaN");
    for (int e = -60; e <= 60; ++e) {
        CHECK(f8_pow2(e) == std::ldexp(1.f, e), "pow2(%d)", e);
        if (e > -60 && e < 60) CHECK(e4m3_scale_exp(448.f * std::ldexp(1.f, e)) == e && e4m3_scale_exp(449.f * std::ldexp(1.f, e)) == e + 1, "scale_exp at 2^%d", e);
    }
    CHECK(e4m3_scale_exp(0.f) == 0 && e8m0(0) == 127 && e8m0(kF8XLoExp) == 112, "scale bytes");
    printf("encoder: %s\n", failures ? "FAILED" : "ok");
}

static void check_route() {
    const int before = failures;
    for (int J = 2; J <= 64; ++J)
        for (int NB = 1; NB <= 32; ++NB)
            for (int mode = 0; mode < 8; ++mode) {
                const bool streams = mode & 1, tile = mode & 2, f16 = mode & 4;
                const LbsRouteRecord r = lbs_route(J, NB, streams, tile, f16), r4 = lbs_route(J, NB, streams, tile);
                const bool want = r.route == LbsRoute::stream && !f16 && 9 * (J - 1) >= 192;
                CHECK(r.pose_fp8 == want, "J %d NB %d mode %d: pose_fp8 %d", J, NB, mode, (int)r.pose_fp8);
                CHECK(r.route == r4.route && r.k_steps_x == r4.k_steps_x && r.w_frags == r4.w_frags && r.pose_capacity == r4.pose_capacity && r.groups_a == r4.groups_a,
                      "J %d NB %d mode %d: the switch moves more than pose_fp8", J, NB, mode);
                if (r.pose_fp8) CHECK(r.k_steps_x == 14 && (J == 23 || J == 24) && 9 * (J - 1) + NB + 2 <= 224, "J %d NB %d: e4m3 form outside 7 k-steps", J, NB);
            }
    CHECK(lbs_route(24, 10, true, false).pose_fp8 && !lbs_route(24, 10, true, false, true).pose_fp8 && !lbs_route(22, 10, true, false).pose_fp8, "the headline model");
    printf("route: %s\n", failures == before ? "ok" : "FAILED");
}

// The strips of one image against the f16 image of the same constants, the layout written out again:
//   spd [k-step][16-vertex tile][coordinate][hi | lo][1 KiB]; f16 piece: lane = row + 16 (k >> 3), 8 halfs k & 7;
//   e4m3 piece: lane group g = 16 bytes per lane: Pd_lo8[0..15], Pd_lo8[16..31], Pd_hi8[0..15], Pd_hi8[16..31]
static void check_image(int J, int NB, int V, const std::vector<int>& ids, bool given, int glo, int ghi, std::mt19937& rng, int* lo_exp, int* hi_exp) {
    const int P = 9 * (J - 1);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    std::vector<float> vt((size_t)V * 3), sd((size_t)V * 3 * NB), pd((size_t)P * 3 * V), w((size_t)V * J);
    std::mt19937 data(1000 * J + NB);                      // the same constants for the mesh and its subset
    for (float& x : vt) x = u(data);
    for (float& x : sd) x = 0.05f * u(data);
    for (float& x : pd) x = 0.02f * u(data) * u(data);
    for (float& x : w) x = 0.5f + 0.5f * u(data);
    (void)rng;
    const LbsRouteRecord r = lbs_route(J, NB, true, false), rt = lbs_route(J, NB, true, false, true);
    tables::VertexSetShape s8{J, NB, P, r.k_steps_x, r.w_frags, r.pose_fp8, given, glo, ghi}, s16{J, NB, P, rt.k_steps_x, rt.w_frags, rt.pose_fp8};
    const tables::VertexSetImages a = tables::vertex_set_images(s8, ids, {}, vt.data(), sd.data(), pd.data(), w.data(), V);
    const tables::VertexSetImages b = tables::vertex_set_images(s16, ids, {}, vt.data(), sd.data(), pd.data(), w.data(), V);
    const int n = (int)ids.size(), nv16 = a.nv16;
    CHECK(a.spd.size() == b.spd.size() && a.nv16 == b.nv16 && a.nv16 == (n + 127) / 128 * 8 && a.sw == b.sw, "J %d NB %d: sizes / W image", J, NB);
    CHECK(b.pd8_lo_exp == 0 && b.pd8_hi_exp == 0, "the f16 image has no scales");
    if (a.spd.size() != b.spd.size()) return;
    float max_lo = 0.f, max_hi = 0.f;
    for (int ks = 0; ks < 7; ++ks)
        for (int t = 0; t < nv16; ++t)
            for (int c = 0; c < 3; ++c) {
                const size_t base = (((size_t)ks * nv16 + t) * 3 + c) * 1024;
                CHECK(!memcmp(&a.spd[base], &b.spd[base], 1024), "hi piece (%d, %d, %d)", ks, t, c);
                if (ks >= kF8PoseSteps) { CHECK(!memcmp(&a.spd[base + 512], &b.spd[base + 512], 1024), "lo piece of k-step %d", ks); continue; }
                for (int e = 0; e < 512; ++e) {
                    max_hi = std::fmax(max_hi, std::fabs((float)b.spd[base + e]));
                    max_lo = std::fmax(max_lo, std::fabs((float)b.spd[base + 512 + e]));
                }
            }
    if (!given) {
        CHECK(max_lo <= 448.f * std::ldexp(1.f, a.pd8_lo_exp) && max_lo > 448.f * std::ldexp(1.f, a.pd8_lo_exp - 1), "lo scale 2^%d for %g", a.pd8_lo_exp, (double)max_lo);
        CHECK(max_hi <= 448.f * std::ldexp(1.f, a.pd8_hi_exp) && max_hi > 448.f * std::ldexp(1.f, a.pd8_hi_exp - 1), "hi scale 2^%d for %g", a.pd8_hi_exp, (double)max_hi);
    } else {
        CHECK(a.pd8_lo_exp == glo && a.pd8_hi_exp == ghi, "given scales");
    }
    *lo_exp = a.pd8_lo_exp; *hi_exp = a.pd8_hi_exp;
    for (int ks = 0; ks < kF8PoseSteps; ++ks)
        for (int t = 0; t < nv16; ++t)
            for (int c = 0; c < 3; ++c) {
                const size_t base = (((size_t)ks * nv16 + t) * 3 + c) * 1024;
                const uint8_t* strip = reinterpret_cast<const uint8_t*>(&a.spd[base + 512]);
                for (int row = 0; row < 16; ++row)
                    for (int k = 0; k < 32; ++k) {
                        const int at16 = ((k >> 3) * 16 + row) * 8 + (k & 7);
                        const double hi = (double)(float)b.spd[base + at16], lo = (double)(float)b.spd[base + 512 + at16];
                        const uint8_t lo8 = strip[((k >> 4) * 16 + row) * 16 + (k & 15)], hi8 = strip[((2 + (k >> 4)) * 16 + row) * 16 + (k & 15)];
                        CHECK(lo8 == encode_by_search(std::ldexp(lo, -a.pd8_lo_exp)) && hi8 == encode_by_search(std::ldexp(hi, -a.pd8_hi_exp)),
                              "J %d NB %d (%d, %d, %d) row %d k %d: codes %d %d", J, NB, ks, t, c, row, k, (int)lo8, (int)hi8);
                        if (t * 16 + row >= n) CHECK(lo8 == 0 && hi8 == 0, "padding row holds codes");
                    }
            }
}

int main() {
    check_encoder();
    check_route();
    const int before = failures;
    std::mt19937 rng(9);
    int images = 0;
    for (int J = 17; J <= 24; ++J)
        for (int NB = 1; NB <= 24; ++NB) {                // (the route allows 1-24 coefficients with 23 joints, 1-15 with 24)
            const LbsRouteRecord r = lbs_route(J, NB, true, false);
            if (!r.pose_fp8) continue;
            const int V = 150 + 7 * NB;                    // two 128-vertex groups, the second partial
            std::vector<int> all(V), sub;
            for (int i = 0; i < V; ++i) all[i] = i;
            for (int i = 0; i < 21; ++i) sub.push_back((i * 37 + NB) % V);
            int lo = 0, hi = 0, lo2 = 0, hi2 = 0;
            check_image(J, NB, V, all, false, 0, 0, rng, &lo, &hi);
            check_image(J, NB, V, sub, true, lo, hi, rng, &lo2, &hi2);      // the 21-vertex operand set of the joints-only call
            ++images;
        }
    CHECK(images == 24 + 15, "%d models with the e4m3 form", images);
    printf("images: %s\n", failures == before ? "ok" : "FAILED");
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
