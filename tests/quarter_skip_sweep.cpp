// Stand-alone host program of tests/test_quarter_skip_host.py: sweeps quarter_may_contribute (cull.hip.h, as host code)
// over (splat, box) cases and holds every `false` against a float64 evaluation at every pixel centre of the box.
// Prints one line of counts; exit status 1 if a skip was wrong.  Built with -fsanitize=address,undefined by the test.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "cull.hip.h"

namespace {

struct Splat { float mx, my, A, B, C, op; };
struct Box { float x0, y0, x1, y1; };

// the binning predicate (rect_may_contribute of cull.hip.h is device code), transliterated for the comparison that is
// only printed: same operations in the same order
float old_edge_min_q(float A, float B, float C, float r, float d, float lo, float hi) {
    float t = -(d * r);
    t = fminf(hi, fmaxf(lo, t));
    return A * d * d + 2.0f * B * d * t + C * t * t;
}
bool old_rect_may_contribute(const Splat& s, const Box& b) {
    if (s.op < 1.0f / 255.0f) return false;
    if (!(s.A > 0.0f) || !(s.C > 0.0f)) return true;
    if (s.mx >= b.x0 && s.mx <= b.x1 && s.my >= b.y0 && s.my <= b.y1) return true;
    const float dx0 = b.x0 - s.mx, dx1 = b.x1 - s.mx, dy0 = b.y0 - s.my, dy1 = b.y1 - s.my;
    const float dxn = s.mx < b.x0 ? dx0 : dx1, dyn = s.my < b.y0 ? dy0 : dy1;
    const float q = fminf(old_edge_min_q(s.A, s.B, s.C, s.B / s.C, dxn, dy0, dy1), old_edge_min_q(s.C, s.B, s.A, s.B / s.A, dyn, dx0, dx1));
    const float DX = fmaxf(fabsf(dx0), fabsf(dx1)), DY = fmaxf(fabsf(dy0), fabsf(dy1));
    const float M = s.A * DX * DX + 2.0f * fabsf(s.B) * DX * DY + s.C * DY * DY;
    const float t = 255.0f * s.op;
    uint32_t bits;
    __builtin_memcpy(&bits, &t, 4);
    const float e = (float)((int)((bits >> 23) & 0xffu) - 127);
    const uint32_t mb = (bits & 0x007fffffu) | 0x3f800000u;
    float m;
    __builtin_memcpy(&m, &mb, 4);
    const float tau = 1.3862944f * (e + (m - 1.0f) + 0.0861f);
    return !(q > tau + 0.00001f * M + 0.01f);
}

// can ANY pixel centre of the box count?  float64; a NaN counts (the pair loop keeps such an entry valid)
// 1e-5: covers the pair loop's fp32 power, its exp2 argument and v_exp_f32 (cull.hip.h, steps 4-6: below 1e-6 M + 1e-6 in
// units of q, i.e. below the margins the function itself adds)
bool reaches(const Splat& s, const Box& b) {
    const double lim = (1.0 / 255.0) * (1.0 - 1e-5);
    for (double py = b.y0; py <= b.y1; py += 1.0)
        for (double px = b.x0; px <= b.x1; px += 1.0) {
            const double dx = px - (double)s.mx, dy = py - (double)s.my;
            const double q = (double)s.A * dx * dx + 2.0 * (double)s.B * dx * dy + (double)s.C * dy * dy;
            const double power = -0.5 * q;
            const bool out = power > 0.0 || (double)s.op * std::exp(power) < lim;
            if (!out) return true;
        }
    return false;
}

struct Tally {
    long long cases = 0, skipped = 0, wrong = 0, new_keeps_old_rejects = 0, old_keeps_new_rejects = 0;
    void one(const Splat& s, const Box& b) {
        const bool keep = pgr::quarter_may_contribute(s.mx, s.my, s.A, s.B, s.C, s.op, s.B / s.C, s.B / s.A, b.x0, b.y0, b.x1, b.y1);
        const bool old_keep = old_rect_may_contribute(s, b);
        ++cases;
        new_keeps_old_rejects += keep && !old_keep;
        old_keeps_new_rejects += !keep && old_keep;
        if (keep) return;
        ++skipped;
        if (reaches(s, b)) {
            if (wrong++ < 10)
                std::printf("WRONG SKIP: centre (%.9g, %.9g) conic (%.9g, %.9g, %.9g) op %.9g box [%g,%g]x[%g,%g]\n", s.mx, s.my, s.A,
                            s.B, s.C, s.op, b.x0, b.x1, b.y0, b.y1);
        }
    }
};

struct Conic { float A, B, C; };

Conic rotated(double s_major, double s_minor, double deg) {
    const double th = deg * 3.14159265358979323846 / 180.0, c = std::cos(th), s = std::sin(th);
    const double ia = 1.0 / (s_major * s_major), ib = 1.0 / (s_minor * s_minor);
    return {(float)(c * c * ia + s * s * ib), (float)(c * s * (ia - ib)), (float)(s * s * ia + c * c * ib)};
}

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
double uniform() {      // xorshift64*, [0, 1)
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (double)((rng_state * 0x2545F4914F6CDD1Dull) >> 11) / 9007199254740992.0;
}

}  // namespace

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const int W = 61, H = 45;       // the last column and row clip the boxes at (56, 40)
    const float ops[] = {0.0f, 1e-42f, (1.0f / 255.0f) * (1.0f - 1e-3f), (1.0f / 255.0f) * (1.0f + 1e-3f), 0.5f, 0.99f, 1.0f, 1e30f};

    std::vector<Conic> conics;
    for (double sigma : {0.55, 1.0, 3.0, 10.0, 50.0}) conics.push_back(rotated(sigma, sigma, 0.0));
    for (double minor : {0.55, 2.0})
        for (double deg : {0.0, 45.0, 135.0}) conics.push_back(rotated(1000.0 * minor, minor, deg));
    conics.push_back({0.0f, 0.0f, 1.0f});      // A <= 0
    conics.push_back({-1.0f, 0.3f, 1.0f});
    conics.push_back({1.0f, 0.0f, 0.0f});      // C <= 0
    conics.push_back({1.0f, 0.3f, -1.0f});
    conics.push_back({1.0f, 2.0f, 1.0f});      // A C < B^2
    conics.push_back({1.0f, -2.0f, 1.0f});
    conics.push_back({0.01f, 0.5f, 4.0f});

    std::vector<Box> boxes;
    const int origins[][2] = {{0, 0}, {16, 24}, {56, 40}};
    for (const auto& o : origins)
        for (int w : {1, 2, 3, 5, 8})
            for (int h : {1, 2, 3, 5, 8})
                boxes.push_back({(float)o[0], (float)o[1], (float)std::min(o[0] + w - 1, W - 1), (float)std::min(o[1] + h - 1, H - 1)});

    // a centre along one axis of a box [lo, hi]: inside, on either edge, and 1, 8 and 1e6 pixels outside on either side
    auto centres = [](float lo, float hi) {
        return std::vector<float>{0.5f * (lo + hi) + 0.3f * (hi > lo ? 1.0f : 0.0f), lo, hi, lo - 1.0f, hi + 1.0f, lo - 8.0f, hi + 8.0f,
                                  lo - 1e6f, hi + 1e6f};
    };

    Tally t;
    for (const Box& b : boxes)
        for (float mx : centres(b.x0, b.x1))
            for (float my : centres(b.y0, b.y1)) {
                for (const Conic& c : conics)
                    for (float op : ops) t.one({mx, my, c.A, c.B, c.C, op}, b);
                // NaN or Inf in each field of an ordinary splat
                for (float bad : {nan, inf, -inf})
                    for (int field = 0; field < 6; ++field)
                        for (float op : ops) {
                            float f[6] = {mx, my, 0.25f, 0.05f, 0.11f, op};
                            f[field] = bad;
                            t.one({f[0], f[1], f[2], f[3], f[4], f[5]}, b);
                        }
            }
    // near the threshold: random splats placed so that the box minimum of q is around 2 ln(255 op)
    for (int i = 0; i < 400000; ++i) {
        const Box& b = boxes[(size_t)(uniform() * boxes.size())];
        const double minor = 0.55 + 6.0 * uniform(), ratio = std::pow(1000.0, uniform());
        const Conic c = rotated(minor * ratio, minor, 180.0 * uniform());
        const float op = (float)std::pow(10.0, -2.6 + 2.6 * uniform());
        const double tau = std::fmax(2.0 * std::log(255.0 * op), 0.0) * (0.8 + 0.8 * uniform());
        const double ang = 6.283185307179586 * uniform(), ux = std::cos(ang), uy = std::sin(ang);
        const double qu = c.A * ux * ux + 2.0 * c.B * ux * uy + c.C * uy * uy;
        const double len = std::sqrt(tau / qu);       // q(len u) = tau
        // a point of the box (a corner half of the time: the nearest point of a box is a corner or lies on an edge)
        const double bx = uniform() < 0.5 ? (uniform() < 0.5 ? b.x0 : b.x1) : b.x0 + (b.x1 - b.x0) * uniform();
        const double by = uniform() < 0.5 ? (uniform() < 0.5 ? b.y0 : b.y1) : b.y0 + (b.y1 - b.y0) * uniform();
        t.one({(float)(bx - len * ux), (float)(by - len * uy), c.A, c.B, c.C, op}, b);
    }
    std::printf("cases %lld skipped %lld wrong %lld new_keeps_old_rejects %lld old_keeps_new_rejects %lld\n", t.cases, t.skipped,
                t.wrong, t.new_keeps_old_rejects, t.old_keeps_new_rejects);
    return t.wrong ? 1 : 0;
}
