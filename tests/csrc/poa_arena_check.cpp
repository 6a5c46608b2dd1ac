// The arena arithmetic of a resident POA graph (csrc/nd_lqplan.h: poa_arena_layout, poa_arena_offsets) on its own: a plain program,
// built by tests/test_poa_arena.py with -fsanitize=address,undefined.  Prints "ok" or what is wrong.
#include <cstdio>
#include <vector>

#include "nd_lqplan.h"

using namespace ndgpu;

static int fail(const char *what, uint64_t a, uint64_t b) {
    printf("%s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
    return 1;
}

// element bytes and element count of every part, written out beside the header's rule
static void part_shape(int p, uint64_t bound, uint64_t &elem, uint64_t &count) {
    switch (p) {
        case kPaLabels: case kPaScore: case kPaRows: elem = 8, count = bound; break;
        case kPaRoute: elem = 4, count = bound; break;
        case kPaPreds: elem = 2, count = 2 * bound; break;
        case kPaStack: elem = 2, count = 2 * bound + 2; break;
        case kPaBase: case kPaDone: case kPaStarted: elem = 1, count = bound; break;
        default: elem = 2, count = bound; break;
    }
}

static int check_layout(uint64_t bound) {
    PoaArena A;
    if (!poa_arena_layout(bound, A)) return fail("a bound within the limit has no layout", bound, 0);
    if (A.bound != bound) return fail("bound not recorded", bound, A.bound);
    uint64_t end = 0, sum = 0;
    for (int p = 0; p < (int)kPaCount; p++) {
        uint64_t elem, count;
        part_shape(p, bound, elem, count);
        if (A.len[p] != elem * count) return fail("size of a part", (uint64_t)p, A.len[p]);
        if (A.off[p] % 8) return fail("a part is not 8-byte aligned", (uint64_t)p, A.off[p]);
        if (A.off[p] < end) return fail("parts overlap or run backwards", (uint64_t)p, A.off[p]);   // monotone, disjoint
        end = A.off[p] + A.len[p];
        sum += (A.len[p] + 7) / 8 * 8;
    }
    if (A.bytes < end || A.bytes % 8 || A.bytes != sum) return fail("total", A.bytes, sum);
    // what the kernels rely on: the route holds X + Y <= bound words, the predecessor rows nodes + edges entries, the stack a root, a
    // group per started group and a group per out-edge
    if (A.len[kPaRoute] / 4 < bound || A.len[kPaPreds] / 2 < 2 * bound || A.len[kPaStack] / 2 < 2 * bound + 1) return fail("capacity", bound, 0);
    return 0;
}

int main() {
    PoaArena A;
    for (uint64_t b : {(uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)7, (uint64_t)64, (uint64_t)1801, (uint64_t)60000, (uint64_t)65534, (uint64_t)65535})
        if (check_layout(b)) return 1;
    for (uint64_t b = 1; b < 300; b++)
        if (check_layout(b)) return 1;
    A.bytes = 12345, A.bound = 777;
    for (uint64_t b : {(uint64_t)0, (uint64_t)65536, (uint64_t)70000, ~(uint64_t)0})
        if (poa_arena_layout(b, A) || A.bytes != 12345 || A.bound != 777) return fail("a bound outside the limit was laid out", b, A.bytes);
    // sizes written out: bound 1 -- three 8-byte parts, the route (4 -> 8), 17 two-byte parts (2 -> 8), predecessor rows (4 -> 8), the
    // stack (8), three bytes (1 -> 8 each)
    (void)poa_arena_layout(1, A);
    if (A.bytes != 3 * 8 + 8 + 17 * 8 + 8 + 8 + 3 * 8) return fail("bytes of bound 1", A.bytes, 0);
    (void)poa_arena_layout(2, A);
    if (A.bytes != 3 * 16 + 8 + 17 * 8 + 8 + 16 + 3 * 8) return fail("bytes of bound 2", A.bytes, 0);
    (void)poa_arena_layout(65535, A);
    const uint64_t big = 3 * 524280ull + 262144 + 17 * 131072ull + 262144 + 262144 + 3 * 65536ull;
    if (A.bytes != big) return fail("bytes of bound 65535", A.bytes, big);
    // a batch: running offsets, a refused bound takes no room, 64-bit totals for 10^6 problems of the largest arena
    {
        const uint64_t bounds[5] = {1, 65536, 2, 0, 65535};
        uint64_t off[5];
        const uint64_t total = poa_arena_offsets(bounds, 5, off);
        if (off[0] != 0 || off[1] != 208 || off[2] != 208 || off[3] != 208 + 240 || off[4] != off[3] || total != off[4] + big)
            return fail("offsets of a batch", total, off[4]);
    }
    {
        const size_t n = 1000000;
        std::vector<uint64_t> bounds(n, 65535), off(n);
        const uint64_t total = poa_arena_offsets(bounds.data(), n, off.data());
        if (total != big * n || total <= (1ull << 32) || off[n - 1] != big * (n - 1)) return fail("total of 10^6 problems", total, big * n);
        for (size_t i = 1; i < n; i++)
            if (off[i] - off[i - 1] != big || off[i] % 8) return fail("offsets of 10^6 problems", (uint64_t)i, off[i]);
    }
    printf("ok\n");
    return 0;
}
