// Hnsw::search_allowed / HnswMap::search_allowed of the C++ host mirror (instant-distance_amd/host/instant_distance.hpp) against a
// scan of its own: whatever rung answers, a query gets min(k, allowed points) allowed items, nearest first; with max_rungs = 0
// they are the exact k nearest allowed points.  Exit code 0 = all assertions hold.  Built and run by tests/test_allowed.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>

#include "../../instant-distance_amd/host/instant_distance.hpp"

using namespace instant_distance;

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } \
    } while (0)

struct Point {
    float x, y, z;
    static constexpr int METRIC = IDIST_METRIC_L2SQ;
    size_t dim() const { return 3; }
    void write_f32(float* o) const { o[0] = x; o[1] = y; o[2] = z; }
};

int main() {
    const int n = 3000, k = 7;
    std::mt19937_64 rng(5);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    std::vector<Point> points;
    std::vector<int> values;
    for (int i = 0; i < n; i++) { points.push_back(Point{u(rng), u(rng), u(rng)}); values.push_back(i); }
    auto m = Builder::default_().seed(3).ef_search(20).build(points, values);
    auto [hnsw, pids] = Builder::default_().seed(3).ef_search(20).build_hnsw(points);
    Search search;
    // shares: every point, a third, one in fifty, three points (< k), none
    const double shares[] = {1.0, 0.33, 0.02, -3.0, 0.0};
    for (double share : shares) {
        std::vector<bool> allowed(n, false);          // by PointId
        size_t n_allowed = 0;
        for (int i = 0; i < n; i++) {
            const bool on = share < 0 ? i < (int)-share : u(rng) < share;
            allowed[i] = on;
            n_allowed += on;
        }
        for (int t = 0; t < 5; t++) {
            const Point q{u(rng), u(rng), u(rng)};
            uint32_t rung = 0;
            auto items = hnsw.search_allowed(q, allowed, k, search, -1, &rung);
            REQUIRE(items.size() == std::min<size_t>(k, n_allowed));
            REQUIRE(n_allowed ? rung != IDIST_RUNG_NONE : rung == IDIST_RUNG_NONE);
            if (n_allowed && n_allowed <= (size_t)k) REQUIRE(rung == IDIST_RUNG_EXACT);
            for (size_t i = 0; i < items.size(); i++) {
                REQUIRE(allowed[items[i].pid.v]);
                REQUIRE(items[i].point == &hnsw[items[i].pid]);
                if (i) REQUIRE(items[i - 1].distance <= items[i].distance);
            }
            // the exact scan alone: the k nearest allowed points of a scan of our own (distances within rounding)
            auto exact = hnsw.search_allowed(q, allowed, k, search, 0, &rung);
            REQUIRE(exact.size() == items.size());
            REQUIRE(exact.empty() || rung == IDIST_RUNG_EXACT);
            std::vector<std::pair<float, uint32_t>> all;
            for (int i = 0; i < n; i++) {
                if (!allowed[i]) continue;
                const Point& p = hnsw[PointId{(uint32_t)i}];
                all.push_back({(p.x - q.x) * (p.x - q.x) + (p.y - q.y) * (p.y - q.y) + (p.z - q.z) * (p.z - q.z), (uint32_t)i});
            }
            std::sort(all.begin(), all.end());
            for (size_t i = 0; i < exact.size(); i++) {
                REQUIRE(std::fabs(exact[i].distance - all[i].first) <= 1e-6f);
                if (exact[i].pid.v != all[i].second) REQUIRE(std::fabs(all[i].first - exact[i].distance) <= 1e-6f);
                REQUIRE(items[i].distance >= exact[i].distance - 1e-6f);     // a rung's answer is never better than the exact one
            }
        }
    }
    // the map returns the values of the same ids (same seed: the same PointIds)
    std::vector<bool> allowed(n, false);
    for (int i = 0; i < n; i += 3) allowed[i] = true;
    const Point q{0.5f, 0.5f, 0.5f};
    Search s2;
    auto a = hnsw.search_allowed(q, allowed, k, search);
    auto b = m.search_allowed(q, allowed, k, s2);
    REQUIRE(a.size() == (size_t)k && b.size() == a.size());
    for (size_t i = 0; i < a.size(); i++) {
        REQUIRE(a[i].pid == b[i].pid && a[i].distance == b[i].distance);
        REQUIRE(pids[*b[i].value].v == b[i].pid.v);
    }
    // arguments
    for (size_t bad_k : {(size_t)0, (size_t)21}) {
        bool threw = false;
        try { hnsw.search_allowed(q, allowed, bad_k, search); } catch (const Error& e) { threw = e.status == IDIST_ERR_INVALID_ARG; }
        REQUIRE(threw);
    }
    printf("allowed ok\n");
    return 0;
}
