// TEST INFRASTRUCTURE ONLY.  A stand-alone program around plan_sub_batches / round_weights (csrc/nd_subplan.h), the arithmetic that
// cuts a batch call's length-sorted piles into sub-batches: built with -fsanitize=address,undefined by tests/test_sub_plan.py and run
// directly.  2,000 seeded draws are checked for the properties below, three fixed cases for their cuts; the first failure is printed
// and the exit status is 1.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <vector>

#include "nd_subplan.h"

namespace {

constexpr size_t kMaxPiles = 384;
constexpr uint64_t kColumnCap = 900000000ull;

uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {  // splitmix64: the draws are the same on every machine
    uint64_t x = (g_state += 0x9e3779b97f4a7c15ull);
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
    return x ^ (x >> 31);
}
uint64_t between(uint64_t lo, uint64_t hi) { return lo + rnd() % (hi - lo + 1); }

int fail(int draw, const char *what) {
    printf("draw %d: %s\n", draw, what);
    return 1;
}

int check_draw(int draw) {
    const size_t n = (size_t)between(1, 3000);
    const int drivers = (int)between(1, 8), rounds = (int)between(1, 2);
    std::vector<uint64_t> est(n);
    for (uint64_t &e : est) e = between(1000, 3000000);
    std::sort(est.begin(), est.end(), std::greater<uint64_t>());
    const std::vector<size_t> cuts = ndgpu::plan_sub_batches(est, drivers, ndgpu::round_weights(rounds, nullptr), kMaxPiles, kColumnCap);
    if (cuts.size() < 2 || cuts.front() != 0 || cuts.back() != n) return fail(draw, "the cuts do not start at 0 and end at n");
    uint64_t total = 0;
    bool full_piece = false;
    for (size_t j = 0; j + 1 < cuts.size(); j++) {
        if (cuts[j + 1] <= cuts[j]) return fail(draw, "the cuts do not rise strictly");
        const size_t piles = cuts[j + 1] - cuts[j];
        if (piles > kMaxPiles) return fail(draw, "a piece has more than 384 piles");
        full_piece = full_piece || piles == kMaxPiles;
        uint64_t cost = 0;
        for (size_t k = cuts[j]; k < cuts[j + 1]; k++) cost += est[k];
        if (piles > 1 && cost > kColumnCap) return fail(draw, "a piece of more than one pile costs more than the column cap");
        total += cost;
    }
    const uint64_t pieces = (uint64_t)drivers * (uint64_t)rounds, share = total / pieces + 1;
    if (share >= 2000000ull && share <= kColumnCap && !full_piece && n >= 4 * pieces && cuts.size() - 1 != pieces)
        return fail(draw, "not exactly drivers x rounds pieces where neither cap nor floor bites");
    return 0;
}

int check_fixed(const char *name, const std::vector<uint64_t> &est, int drivers, int rounds, size_t max_piles, const std::vector<size_t> &want) {
    const std::vector<size_t> cuts = ndgpu::plan_sub_batches(est, drivers, ndgpu::round_weights(rounds, nullptr), max_piles, kColumnCap);
    if (cuts == want) return 0;
    printf("%s: cuts", name);
    for (size_t c : cuts) printf(" %zu", c);
    printf("\n");
    return 1;
}

}  // namespace

int main() {
    for (int draw = 0; draw < 2000; draw++)
        if (check_draw(draw)) return 1;
    // uniform cost, the 1,666 piles of a config-2 step on 8 contexts x 2 rounds: 16 pieces of 104 or 105 piles
    if (check_fixed("uniform", std::vector<uint64_t>(1666, 100000), 8, 2, kMaxPiles,
                    {0, 104, 208, 312, 416, 521, 625, 729, 833, 937, 1041, 1145, 1249, 1354, 1458, 1562, 1666}))
        return 1;
    if (check_fixed("one pile", std::vector<uint64_t>(1, 50000), 8, 1, kMaxPiles, {0, 1})) return 1;
    // 1,000 piles of 5,000 columns on 2 contexts: either half holds 500 piles, the pile cap cuts it after 384
    if (check_fixed("pile cap", std::vector<uint64_t>(1000, 5000), 2, 1, kMaxPiles, {0, 384, 500, 884, 1000})) return 1;
    // NDGPU_TAPER's parse: positive numbers, normalised; nothing usable leaves the equal rounds
    const std::vector<double> w = ndgpu::round_weights(2, "3,1"), d = ndgpu::round_weights(2, "x"), z = ndgpu::round_weights(1, "0,-1");
    if (w.size() != 2 || w[0] != 0.75 || w[1] != 0.25 || d != std::vector<double>{0.5, 0.5} || z != std::vector<double>{1.0}) {
        printf("round_weights\n");
        return 1;
    }
    printf("ok\n");
    return 0;
}
