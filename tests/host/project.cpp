// filter_project alone (instant-distance_amd/csrc/idist_device.hpp), on the CPU lockstep emulator: y_lane and |x - mu|^2 must equal,
// bit for bit, the sequential loop written out below — pos ascending, y then d2, one f64 accumulator each — whatever the order in
// which the routine requests its operands.  Compiled twice by tests/test_filter_project.py: with -DIDIST_PROJECT_BLOCKED (the blocks
// of the device build) and without (the emulator's own plain loop).  Strides: multiples of 16 with remainders 0 and 16 modulo the
// block of 32, among them one block and a half and the longest row a thin walk takes.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../instant-distance_amd/csrc/idist_device.hpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static double uniform() {                      // xorshift64*, in (0, 1)
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return ((rng_state * 0x2545F4914F6CDD1Dull) >> 11) * (1.0 / 9007199254740992.0) + 1e-17;
}
static double normal() { return std::sqrt(-2.0 * std::log(uniform())) * std::cos(6.283185307179586 * uniform()); }

static int check(const char* name, uint32_t stride, const std::vector<float>& B, const std::vector<float>& x, const std::vector<float>& mu) {
    idist::IndexView ix{};
    ix.stride = stride;
    ix.f.basis = B.data();
    ix.f.mu = mu.data();
    std::vector<double> y(64), d2(64);
    emu::launch(1, 64, 0, [&] {
        double dd;
        const double yy = idist::filter_project(ix, x.data(), dd);
        y[idist::lane_id()] = yy;
        d2[idist::lane_id()] = dd;
    });
    int bad = 0;
    for (int lane = 0; lane < 64; lane++) {
        double wy = 0.0, wd2 = 0.0;
        for (uint32_t pos = 0; pos < stride; pos++) {
            const double d = (double)x[pos] - (double)mu[pos];
            wy = __builtin_fma((double)B[(size_t)pos * 64 + lane], d, wy);
            wd2 = __builtin_fma(d, d, wd2);
        }
        if (lane >= idist::kFiltPrincipalM) wy = 0.0;
        if (memcmp(&wy, &y[lane], 8) || memcmp(&wd2, &d2[lane], 8)) {
            if (!bad) printf("%s, stride %u, lane %d: y %a (want %a), d2 %a (want %a)\n", name, stride, lane, y[lane], wy, d2[lane], wd2);
            bad++;
        }
    }
    return bad ? 1 : 0;
}

int main() {
    int bad = 0, cases = 0;
    for (uint32_t stride : {16u, 32u, 48u, 128u, 144u, 208u, 304u, 512u, 624u}) {
        std::vector<float> B((size_t)stride * 64), x(stride), mu(stride);
        for (float& v : B) v = (float)normal();
        for (uint32_t pos = 0; pos < stride; pos++)
            for (int c = idist::kFiltPrincipalM; c < 64; c++) B[(size_t)pos * 64 + c] = 0.0f;       // (as the table is made)
        for (float& v : x) v = (float)(normal() * 3.0);
        for (float& v : mu) v = (float)normal();
        bad += check("random", stride, B, x, mu);
        // every position matters, once each: a row that differs from mu in ONE coordinate (the last granule's and a block's first too)
        for (uint32_t pos : {0u, 15u, 16u, 31u, 32u, stride + stride - 17u, stride - 16u, stride - 1u}) {
            std::vector<float> x1(mu);
            x1[pos % stride] += 1.5f;
            bad += check("one coordinate", stride, B, x1, mu);
            cases++;
        }
        // extreme scales: products that round differently under any reassociation
        std::vector<float> xs(x);
        for (uint32_t pos = 0; pos < stride; pos++) xs[pos] *= (pos % 3 == 0 ? 1e18f : (pos % 3 == 1 ? 1e-18f : 1.0f));
        bad += check("mixed scales", stride, B, xs, mu);
        // a non-finite coordinate in the row, in the centre, and in both
        for (float val : {std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()}) {
            std::vector<float> xn(x), mn(mu);
            xn[stride - 3u] = val;
            bad += check("non-finite x", stride, B, xn, mu);
            mn[stride / 2u] = val;
            bad += check("non-finite mu", stride, B, x, mn);
            xn[stride / 2u] = val;
            bad += check("non-finite x and mu", stride, B, xn, mn);
            cases += 3;
        }
        cases += 2;
    }
    if (bad) { printf("%d of %d cases differ\n", bad, cases); return 1; }
    printf("project ok: %d cases\n", cases);
    return 0;
}
