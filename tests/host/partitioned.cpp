// The life cycle of one idist_partitioned against the C ABI (include/idist.h): ownership and reuse of its staging memory, not parity
// (tests/test_partitioned*.py hold that).  Three parts of 0, 200 and 333 rows, dim 20 (half a block at the end, no multiple of 8),
// L2SQ, ef_search 16.  Every search call runs with 5 queries, with 300 whose first five are the same (every staging buffer grows;
// 300 crosses the 256-thread block of the counts kernel and the 64-query chunk of the prefix sum), and with 5 again: the third
// call's outputs equal the first's byte for byte, and so do rows 0..4 of the second.  A refused range call leaves nothing behind;
// the object, and a plain search context, are freed AFTER the indexes they borrowed.
// Exit code 0 = all assertions hold.  Built and run by tests/test_host_cpp.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/idist.h"

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, idist_last_error()); exit(1); } \
    } while (0)
#define OK(call) REQUIRE((call) == IDIST_OK)

namespace {

constexpr uint32_t kDim = 20, kEf = 16, kK = 10, kParts = 3, kSmall = 5, kLarge = 300;
constexpr uint32_t kRows[kParts] = {0, 200, 333};
constexpr uint32_t kN = 533, kWords = (kN + 31) / 32;
constexpr float kRadius = 2.0f;                          // squared distances of uniform rows in 20-d: 3.3 +- 0.9

// everything one call writes, in one byte string per array; `width` bounds the counts
struct Out {
    std::vector<uint32_t> pid, count, rung, counters;
    std::vector<float> dist;
    std::vector<uint64_t> lims;
};

template <typename T> bool same(const std::vector<T>& a, const std::vector<T>& b, size_t n) {
    return a.size() >= n && b.size() >= n && memcmp(a.data(), b.data(), n * sizeof(T)) == 0;
}
// rows [0, nq) of `b` equal `a`'s (row-major arrays of `w` items per query)
bool same_rows(const Out& a, const Out& b, uint32_t nq, uint32_t w, bool rungs) {
    return same(a.pid, b.pid, (size_t)nq * w) && same(a.dist, b.dist, (size_t)nq * w) && same(a.count, b.count, nq) &&
           same(a.counters, b.counters, (size_t)nq * 3) && (!rungs || same(a.rung, b.rung, (size_t)nq * kParts));
}
void check_lists(const Out& o, uint32_t nq, uint32_t w) {
    for (uint32_t q = 0; q < nq; q++) {
        REQUIRE(o.count[q] <= w);
        for (uint32_t j = 0; j < o.count[q]; j++) REQUIRE(o.pid[(size_t)q * w + j] < kN);
    }
}
Out lists(uint32_t nq, uint32_t w) {
    Out o;
    o.pid.assign((size_t)nq * w, 0xA5A5A5A5u);
    o.dist.assign((size_t)nq * w, -1.0f);
    o.count.assign(nq, 0xA5A5A5A5u);
    o.rung.assign((size_t)nq * kParts, 0xA5A5A5A5u);
    o.counters.assign((size_t)nq * 3, 0xA5A5A5A5u);
    return o;
}

struct Case {
    idist_partitioned* p;
    const float* queries;
    const uint32_t* sets;                                // [kLarge][kWords]: sets 0 and 1 serve the alternating call, set q query q
    const uint32_t* set_of;                              // [kLarge], alternating

    Out search(uint32_t nq) const {
        Out o = lists(nq, kEf);
        OK(idist_partitioned_search_batch(p, queries, nq, o.pid.data(), o.dist.data(), o.count.data(), o.counters.data()));
        check_lists(o, nq, kEf);
        return o;
    }
    Out bruteforce(uint32_t nq) const {
        Out o = lists(nq, kK);
        OK(idist_partitioned_bruteforce(p, queries, nq, kK, o.pid.data(), o.dist.data()));
        o.count.assign(nq, kK);                          // (533 points: every row is full)
        check_lists(o, nq, kK);
        return o;
    }
    Out allowed(uint32_t nq, bool own_sets) const {
        Out o = lists(nq, kK);
        OK(idist_partitioned_search_batch_allowed_sets(p, queries, nq, sets, own_sets ? nq : 2u, own_sets ? nullptr : set_of, kK, -1,
                                                       o.pid.data(), o.dist.data(), o.count.data(), o.rung.data(), o.counters.data()));
        check_lists(o, nq, kK);
        return o;
    }
    // the range call and its fetch: pid / dist are the flat arrays, count[q] = lims[q + 1] - lims[q]
    Out range(uint32_t nq) const {
        Out o = lists(nq, 0);
        o.lims.assign((size_t)nq + 1, ~0ull);
        OK(idist_partitioned_search_batch_range(p, queries, nq, &kRadius, 1, -1, 1ull << 40, o.lims.data(), o.rung.data(), o.counters.data()));
        REQUIRE(o.lims[0] == 0);
        for (uint32_t q = 0; q < nq; q++) {
            REQUIRE(o.lims[q] <= o.lims[q + 1] && o.lims[q + 1] - o.lims[q] <= kN);
            o.count[q] = (uint32_t)(o.lims[q + 1] - o.lims[q]);
        }
        const uint64_t total = o.lims[nq];
        REQUIRE(total > 0);                              // the radius was chosen so that results exist
        o.pid.assign(total, 0xA5A5A5A5u);
        o.dist.assign(total, -1.0f);
        OK(idist_partitioned_range_fetch(p, o.pid.data(), o.dist.data()));
        for (uint64_t j = 0; j < total; j++) REQUIRE(o.pid[j] < kN && o.dist[j] <= kRadius);
        return o;
    }
};

bool same_range(const Out& a, const Out& b, uint32_t nq) {
    const size_t total = (size_t)a.lims[nq];
    return same(a.lims, b.lims, (size_t)nq + 1) && same(a.pid, b.pid, total) && same(a.dist, b.dist, total) &&
           same(a.rung, b.rung, (size_t)nq * kParts) && same(a.counters, b.counters, (size_t)nq * 3);
}

}  // namespace

int main() {
    std::mt19937_64 rng(20);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    idist_config cfg;
    OK(idist_default_config(&cfg));
    cfg.ef_search = kEf;
    cfg.metric = IDIST_METRIC_L2SQ;
    idist_index* parts[kParts] = {nullptr, nullptr, nullptr};
    for (uint32_t i = 0; i < kParts; i++) {
        std::vector<float> rows((size_t)kRows[i] * kDim + 1);     // (+ 1: a valid pointer for the empty part)
        for (float& x : rows) x = u(rng);
        OK(idist_index_build(rows.data(), kRows[i], kDim, &cfg, 0, &parts[i]));
    }
    std::vector<float> queries((size_t)kLarge * kDim);
    for (float& x : queries) x = u(rng);
    // set s: every second one dense (half the points), the others sparse (a twentieth); the last point, in the partial word, is in all
    std::vector<uint32_t> sets((size_t)kLarge * kWords, 0u), set_of(kLarge);
    for (uint32_t s = 0; s < kLarge; s++) {
        set_of[s] = s % 2u;
        for (uint32_t g = 0; g < kN; g++)
            if (u(rng) < (s % 2u ? 0.05f : 0.5f) || g == kN - 1) sets[(size_t)s * kWords + g / 32u] |= 1u << (g % 32u);
    }

    idist_partitioned* p = nullptr;
    OK(idist_partitioned_new(parts, kParts, &p));
    const Case c{p, queries.data(), sets.data(), set_of.data()};
    {
        const Out a = c.search(kSmall), b = c.search(kLarge), a2 = c.search(kSmall);
        REQUIRE(same_rows(a, a2, kSmall, kEf, false) && same_rows(a, b, kSmall, kEf, false));
    }
    {
        const Out a = c.bruteforce(kSmall), b = c.bruteforce(kLarge), a2 = c.bruteforce(kSmall);
        REQUIRE(same_rows(a, a2, kSmall, kK, false) && same_rows(a, b, kSmall, kK, false));
    }
    for (bool own_sets : {false, true}) {
        const Out a = c.allowed(kSmall, own_sets), b = c.allowed(kLarge, own_sets), a2 = c.allowed(kSmall, own_sets);
        REQUIRE(same_rows(a, a2, kSmall, kK, true) && same_rows(a, b, kSmall, kK, true));
        for (uint32_t q = 0; q < kSmall; q++) REQUIRE(a.rung[(size_t)q * kParts] == IDIST_RUNG_NONE);   // part 0 is empty
    }
    {
        const Out a = c.range(kSmall), b = c.range(kLarge), a2 = c.range(kSmall);
        REQUIRE(same_range(a, a2, kSmall) && same_range(a, b, kSmall));
        // a refused call (results exist, none may be returned) holds nothing; the next ordinary call is what it was before
        Out r = lists(kSmall, 0);
        r.lims.assign(kSmall + 1, ~0ull);
        REQUIRE(idist_partitioned_search_batch_range(p, c.queries, kSmall, &kRadius, 1, -1, 0, r.lims.data(), r.rung.data(), r.counters.data()) != IDIST_OK);
        std::vector<uint32_t> pid(a.lims[kSmall]);
        std::vector<float> dist(a.lims[kSmall]);
        REQUIRE(idist_partitioned_range_fetch(p, pid.data(), dist.data()) != IDIST_OK);
        const Out a3 = c.range(kSmall);
        REQUIRE(same_range(a, a3, kSmall));
    }

    // a second object over the same parts: made, used once, freed
    {
        idist_partitioned* p2 = nullptr;
        OK(idist_partitioned_new(parts, kParts, &p2));
        const Case c2{p2, queries.data(), sets.data(), set_of.data()};
        const Out a = c.search(kSmall), a2 = c2.search(kSmall);
        REQUIRE(same_rows(a, a2, kSmall, kEf, false));
        idist_partitioned_free(p2);
    }
    // the parts are borrowed: the object, and a plain context on part 1, outlive them
    idist_search_ctx* ctx = nullptr;
    OK(idist_search_ctx_new(parts[1], 0, &ctx));
    {
        Out o = lists(kSmall, kEf);
        OK(idist_search_batch(parts[1], ctx, queries.data(), kSmall, o.pid.data(), o.dist.data(), o.count.data(), o.counters.data()));
        for (uint32_t q = 0; q < kSmall; q++) REQUIRE(o.count[q] <= kEf);
    }
    for (idist_index* ix : parts) idist_index_free(ix);
    idist_partitioned_free(p);
    idist_search_ctx_free(ctx);
    printf("partitioned ok\n");
    return 0;
}
