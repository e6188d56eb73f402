// unionfind_host.cpp -- the union-find of iscc_search_amd/csrc/unionfind.hip.h run by host threads (tests/test_unionfind_host.py
// compiles this file with -fsanitize=thread and runs it).  The header's functions are the ones the join kernels call: here they
// compile through the host side of its atomic shim, and 16 threads unite the edges of graphs whose components a sequential DFS
// knows -- where a wrong loop costs nothing.
//
// Per graph: every thread unites its share of the edges (every edge is taken by EDGE_SHARE threads, each in an order of its own),
// checks parent[x] <= x on both ends after every union, and after a barrier the threads flatten the array.  Then every
// parent[i] must be the smallest vertex of i's component.
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <random>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "unionfind.hip.h"

namespace {

constexpr int THREADS = 16;
constexpr int EDGE_SHARE = 8;      // threads that unite each edge

using Edge = std::pair<uint32_t, uint32_t>;

std::vector<uint32_t> component_minimum(uint32_t n, const std::vector<Edge>& edges) {
    std::vector<uint32_t> deg(n + 1, 0), adj(2 * edges.size());
    for (const Edge& e : edges) { deg[e.first + 1]++; deg[e.second + 1]++; }
    for (uint32_t i = 0; i < n; ++i) deg[i + 1] += deg[i];
    std::vector<uint32_t> fill(deg.begin(), deg.end() - 1);
    for (const Edge& e : edges) { adj[fill[e.first]++] = e.second; adj[fill[e.second]++] = e.first; }
    std::vector<uint32_t> comp(n, isk::UF_NONE), stack;
    for (uint32_t s = 0; s < n; ++s) {           // ascending: the first vertex that reaches a component is its minimum
        if (comp[s] != isk::UF_NONE) continue;
        comp[s] = s;
        stack.push_back(s);
        while (!stack.empty()) {
            const uint32_t v = stack.back();
            stack.pop_back();
            for (uint32_t k = deg[v]; k < deg[v + 1]; ++k)
                if (comp[adj[k]] == isk::UF_NONE) { comp[adj[k]] = s; stack.push_back(adj[k]); }
        }
    }
    return comp;
}

bool run(const std::string& name, uint32_t n, const std::vector<Edge>& edges) {
    std::vector<uint32_t> parent(n);
    std::iota(parent.begin(), parent.end(), 0u);
    std::atomic<uint64_t> above{0};               // entries seen above their index
    std::atomic<int> arrived{0};
    auto work = [&](int t) {
        // the edges e with e % (THREADS / EDGE_SHARE) == t % (THREADS / EDGE_SHARE), in this thread's own order
        std::vector<uint32_t> mine;
        constexpr int classes = THREADS / EDGE_SHARE;
        for (size_t e = (size_t)(t % classes); e < edges.size(); e += classes) mine.push_back((uint32_t)e);
        std::mt19937_64 rng(1000 + t);
        if (t % 3 == 1) std::reverse(mine.begin(), mine.end());
        if (t % 3 == 2) std::shuffle(mine.begin(), mine.end(), rng);
        uint64_t bad = 0;
        for (uint32_t e : mine) {
            const uint32_t a = edges[e].first, b = edges[e].second;
            isk::uf_union(parent.data(), a, b);
            bad += isk::uf_load(&parent[a]) > a;
            bad += isk::uf_load(&parent[b]) > b;
        }
        // no union is in flight once every thread is here (the one place a thread waits: the flatten step's precondition, the
        // kernel boundary on the device)
        arrived.fetch_add(1, std::memory_order_acq_rel);
        while (arrived.load(std::memory_order_acquire) < THREADS) std::this_thread::yield();
        for (uint32_t i = (uint32_t)t; i < n; i += THREADS) {
            isk::uf_flatten(parent.data(), i);
            bad += isk::uf_load(&parent[i]) > i;
        }
        above.fetch_add(bad, std::memory_order_relaxed);
    };
    std::vector<std::thread> threads;
    for (int t = 0; t < THREADS; ++t) threads.emplace_back(work, t);
    for (std::thread& th : threads) th.join();
    const std::vector<uint32_t> want = component_minimum(n, edges);
    uint64_t wrong = 0;
    for (uint32_t i = 0; i < n; ++i) wrong += parent[i] != want[i];
    uint32_t components = 0;
    for (uint32_t i = 0; i < n; ++i) components += want[i] == i;
    std::printf("%-28s %8u vertices %9zu edges %7u components: %llu entries above their index, %llu not the component minimum\n", name.c_str(), n,
                edges.size(), components, (unsigned long long)above.load(), (unsigned long long)wrong);
    return above.load() == 0 && wrong == 0;
}

std::vector<Edge> path_over(const std::vector<uint32_t>& labels) {
    std::vector<Edge> edges;
    for (size_t k = 0; k + 1 < labels.size(); ++k) edges.emplace_back(labels[k], labels[k + 1]);
    return edges;
}

}  // namespace

int main() {
    bool ok = true;
    std::mt19937_64 rng(42);
    {   // a clique: every union lands on the same few roots
        const uint32_t n = 2000;
        std::vector<Edge> edges;
        for (uint32_t a = 0; a < n; ++a)
            for (uint32_t b = a + 1; b < n; ++b) edges.emplace_back(b, a);
        ok &= run("clique", n, edges);
    }
    {   // paths of 10^5 vertices: without compression a chain that every find walks
        const uint32_t n = 100000;
        std::vector<uint32_t> labels(n);
        std::iota(labels.begin(), labels.end(), 0u);
        ok &= run("path, ascending labels", n, path_over(labels));
        std::reverse(labels.begin(), labels.end());
        ok &= run("path, descending labels", n, path_over(labels));
        std::shuffle(labels.begin(), labels.end(), rng);
        ok &= run("path, permuted labels", n, path_over(labels));
    }
    {   // a random sparse graph: many components of every small size
        const uint32_t n = 100000;
        std::vector<Edge> edges;
        for (uint32_t e = 0; e < 70000; ++e) edges.emplace_back((uint32_t)(rng() % n), (uint32_t)(rng() % n));
        ok &= run("random sparse", n, edges);
    }
    std::printf(ok ? "ok\n" : "FAILED\n");
    return ok ? 0 : 1;
}
