// csrc/lnb_sample.h on the host: the counts a verify column sees (lnb_sample_delta_count) against "bump the table, call the plain walk" -- the rules loop's own way
// of holding the counted text -- on small rows.  Stand-alone, g++ -std=c++17 under the address and undefined-behaviour sanitizers (tests/test_spec_rules_cpu.py).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../llama-nuts-and-bolts_amd/csrc/lnb_sample.h"

int main() {
    std::vector<double> etab(65536);
    for (uint32_t i = 0; i < 65536; i++) { const uint32_t b = i << 16; float x; memcpy(&x, &b, 4); etab[i] = std::exp((double)x); }
    const LnbSampler samplers[] = {{0.0f, 1.0f, 0, 0, 1}, {0.7f, 0.9f, 40, 0, 786}};
    uint64_t seed = 20261126;
    auto rnd = [&]() { return seed = lnb_sample_splitmix64(seed); };
    int cases = 0, moved = 0;
    for (int V : {9, 67, 200}) for (int round = 0; round < 40; round++) {
        std::vector<uint16_t> row(V), adj(V);
        std::vector<uint32_t> base(V), bumped, delta_table(V);
        for (int j = 0; j < V; j++) {                        // bf16 values in about [-4, 4); a quarter of the entries counted already
            row[j] = (uint16_t)(((rnd() & 1) << 15) | ((126 + (rnd() & 3)) << 7) | (rnd() & 127));
            base[j] = rnd() % 4 == 0 ? (uint32_t)(rnd() % 5) : 0u;
        }
        int delta[15];
        const int nd = (int)(rnd() % 16);
        for (int t = 0; t < nd; t++) delta[t] = t > 0 && rnd() % 3 == 0 ? delta[t - 1] : (int)(rnd() % V);      // (repeats: multiplicity counts)
        bumped = base;
        for (int t = 0; t < nd; t++) bumped[delta[t]] += 1u;
        for (int j = 0; j < V; j++) delta_table[j] = lnb_sample_delta_count(base[j], j, delta, nd);
        if (delta_table != bumped) { printf("FAILED: counts (V %d, round %d)\n", V, round); return 1; }
        for (const LnbSampler& s : samplers) {
            int tok[3]; const uint32_t* tabs[3] = {delta_table.data(), bumped.data(), base.data()};
            for (int k = 0; k < 3; k++) {
                const LnbRulesDev ru = {1.3f, 0.5f, 1.0f, 0.05f, (lnbs_u32*)tabs[k], nullptr};
                tok[k] = lnb_sample_row_serial(row.data(), V, etab.data(), &s, 0, (lnbs_u64)(8 + round), nullptr, &ru, adj.data());
            }
            if (tok[0] != tok[1]) { printf("FAILED: token %d, the bumped table gives %d (V %d, round %d)\n", tok[0], tok[1], V, round); return 1; }
            moved += tok[0] != tok[2]; cases++;
        }
    }
    if (moved * 10 < cases) { printf("FAILED: the deltas moved %d of %d tokens: the comparison is empty\n", moved, cases); return 1; }
    printf("spec_rules_test: ok (%d cases, %d moved by their deltas)\n", cases, moved);
    return 0;
}
