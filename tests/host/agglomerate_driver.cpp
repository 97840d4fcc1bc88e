// Stand-alone run of exaspim_agglomerate (csrc/agglomerate.cpp, host code only) for a build with
// -fsanitize=address,undefined: tests/test_agglomerate_scale_cpu.py compiles the two files into one
// program and runs it as a child process. No device, no input files: three graphs from a fixed LCG
// (a band graph, a hub, a wide near-tie graph), each at two thresholds. Prints the segment counts;
// exit status 1 on any refusal, 0 otherwise. What the sanitizers find goes to stderr.
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../include/exaspim_affinity.h"

namespace exaspim {
static char g_message[512];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_message, sizeof g_message, fmt, ap);
    va_end(ap);
}
}  // namespace exaspim

namespace {

const uint64_t kOne = 1ull << 24;

struct Lcg {
    uint64_t state;
    uint64_t next() {   // Knuth's MMIX constants; the high bits are the good ones
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return state >> 24;
    }
    uint64_t below(uint64_t n) { return next() % n; }
};

struct Row {
    int32_t lo, hi;
    int64_t count;
    uint64_t sum;
};

struct Graph {
    const char* name;
    int32_t k;
    std::vector<Row> rows;
    std::vector<int64_t> sizes;
};

void add(Graph& g, int32_t a, int32_t b, int64_t count, uint64_t sum) {
    if (a != b) g.rows.push_back(Row{std::min(a, b), std::max(a, b), count, sum});
}

// sorted by (lo, hi), of repeated pairs the first stays
void finish(Graph& g, Lcg& rng) {
    std::stable_sort(g.rows.begin(), g.rows.end(),
                     [](const Row& x, const Row& y) { return x.lo != y.lo ? x.lo < y.lo : x.hi < y.hi; });
    g.rows.erase(std::unique(g.rows.begin(), g.rows.end(),
                             [](const Row& x, const Row& y) { return x.lo == y.lo && x.hi == y.hi; }),
                 g.rows.end());
    g.sizes.resize((size_t)g.k + 1);
    for (int64_t& s : g.sizes) s = 1 + (int64_t)rng.below(40);
}

// every fragment next to its three successors, eight affinity levels: ties everywhere
Graph band_graph(Lcg& rng) {
    Graph g{"band", 4000, {}, {}};
    for (int32_t f = 1; f <= g.k; ++f)
        for (int32_t d = 1; d <= 3 && f + d <= g.k; ++d) {
            const int64_t count = 1 + (int64_t)rng.below(6);
            add(g, f, f + d, count, (uint64_t)count * (rng.below(8) * (kOne / 7)));
        }
    finish(g, rng);
    return g;
}

// one fragment in the middle of the ids with 3000 neighbours, which also touch one another
Graph hub_graph(Lcg& rng) {
    Graph g{"hub", 3001, {}, {}};
    const int32_t hub = 1500;
    for (int32_t f = 1; f <= g.k; ++f) {
        const int64_t count = 1 + (int64_t)rng.below(49);
        add(g, hub, f, count, rng.below((uint64_t)count * kOne + 1));
    }
    for (int i = 0; i < 6000; ++i) {
        const int64_t count = 1 + (int64_t)rng.below(49);
        add(g, 1 + (int32_t)rng.below(g.k), 1 + (int32_t)rng.below(g.k), count,
            rng.below((uint64_t)count * kOne + 1));
    }
    finish(g, rng);
    return g;
}

// counts up to 2^26 (9000 of them stay within a total of 2^39), sum = count * level + {-1, 0, 1}
Graph wide_graph(Lcg& rng) {
    Graph g{"wide", 3000, {}, {}};
    for (int i = 0; i < 9000; ++i) {
        const int64_t count = 1 + (int64_t)rng.below(1ull << 26);
        const uint64_t level = rng.below(5) * (kOne / 4);
        const int64_t delta = (int64_t)rng.below(3) - 1;
        int64_t sum = count * (int64_t)level + delta;
        sum = std::max<int64_t>(0, std::min<int64_t>(sum, count * (int64_t)kOne));
        add(g, 1 + (int32_t)rng.below(g.k), 1 + (int32_t)rng.below(g.k), count, (uint64_t)sum);
    }
    finish(g, rng);
    return g;
}

int run(const Graph& g, float threshold) {
    std::vector<int32_t> edges;
    std::vector<int64_t> counts;
    std::vector<uint64_t> sums;
    for (const Row& r : g.rows) {
        edges.push_back(r.lo);
        edges.push_back(r.hi);
        counts.push_back(r.count);
        sums.push_back(r.sum);
    }
    std::vector<int32_t> table((size_t)g.k + 1, -1);
    int32_t n_segments = -1;
    const int rc = exaspim_agglomerate(edges.data(), counts.data(), sums.data(), (int64_t)counts.size(),
                                       g.sizes.data(), g.k, threshold, 20, table.data(), &n_segments);
    if (rc != EXASPIM_OK) {
        printf("%s at %.2f: refused with %d: %s\n", g.name, threshold, rc, exaspim::g_message);
        return 1;
    }
    int32_t largest = 0;
    for (int32_t v : table) largest = std::max(largest, v);
    printf("%s at %.2f: %d fragments, %zu edges, %d segments\n", g.name, threshold, g.k, counts.size(),
           n_segments);
    if (largest != n_segments || table[0] != 0) {
        printf("%s at %.2f: the table's largest label is %d\n", g.name, threshold, largest);
        return 1;
    }
    return 0;
}

}  // namespace

int main() {
    Lcg rng{20240521};
    const Graph graphs[] = {band_graph(rng), hub_graph(rng), wide_graph(rng)};
    int failed = 0;
    for (const Graph& g : graphs)
        for (const float threshold : {0.5f, 0.9f}) failed |= run(g, threshold);
    return failed;
}
