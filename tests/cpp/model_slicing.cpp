// model_slicing.cpp -- slice_plan of line3dpp_amd/csrc/l3d_model.h, the one slicing rule of the comparison (DESIGN §18,
// 32 bytes per (query, slice) cell) and of the merge (§19, 4 bytes), both under 256 MiB: its invariants over a grid of
// sizes, and pins of the rule as it stands, worked out by hand.  Prints "identical" and returns 0 when all hold.
#include <cstdint>
#include <cstdio>

#include "../../line3dpp_amd/csrc/l3d_model.h"

using l3d::SlicePlan;
using l3d::slice_plan;

static int failures = 0;
static void expect(bool ok, const char* what, uint32_t n_q, uint32_t n_r, uint32_t asked, size_t bytes, const SlicePlan& p) {
    if (ok) return;
    ++failures;
    std::printf("FAILED %s: n_q %u n_r %u asked %u bytes %zu -> (%u, %u)\n", what, n_q, n_r, asked, bytes, p.n_slices, p.slice_chunks);
}

int main() {
    const size_t budget = (size_t)256 << 20;
    const uint32_t sizes[] = {1u, 255u, 256u, 257u, 65536u, (1u << 30) - 1};
    const uint32_t asks[] = {0u, 1u, 2u, 7u, 0xFFFFFFFFu};
    const size_t cells[] = {4, 32};
    int n_cases = 0;
    for (uint32_t n_q : sizes)
        for (uint32_t n_r : sizes)
            for (uint32_t asked : asks)
                for (size_t bytes : cells) {
                    const SlicePlan p = slice_plan(n_q, n_r, asked, bytes, budget);
                    const uint64_t n_chunks = ((uint64_t)n_r + 255) / 256, ns = p.n_slices, sc = p.slice_chunks;
                    ++n_cases;
                    expect(ns >= 1 && sc >= 1, "at least one slice of one chunk", n_q, n_r, asked, bytes, p);
                    expect((ns - 1) * sc < n_chunks && n_chunks <= ns * sc, "no slice empty, every chunk covered", n_q, n_r, asked, bytes, p);
                    expect(ns == 1 || (uint64_t)bytes * n_q * ns <= budget, "the cells stay within the budget", n_q, n_r, asked, bytes, p);
                    // the slicing asked for, and whether the cap lets it stand
                    const uint64_t want = asked ? (asked < n_chunks ? asked : n_chunks) : 1;
                    const uint64_t want_slices = (n_chunks + want - 1) / want;
                    if (want_slices == 1 || (uint64_t)bytes * n_q * want_slices <= budget)
                        expect(sc == want && ns == want_slices, "the cap does not bind: the slicing asked for", n_q, n_r, asked, bytes, p);
                }
    struct Pin { const char* stage; uint32_t n_q, n_r; size_t bytes; uint32_t n_slices, slice_chunks; };
    const Pin pins[] = {
        {"compare", 16640u, 16640u, 32, 65u, 1u},            // 65 chunks, the cap (504) does not bind
        {"compare", 1u << 20, 1u << 20, 32, 8u, 512u},       // 4096 chunks, cap 8
        {"compare", 1u << 21, 2304u, 32, 3u, 3u},            // 9 chunks, cap 4: three slices of three
        {"compare", 1u << 21, 2560u, 32, 4u, 3u},            // 10 chunks, cap 4
        {"merge", 1u << 20, 1u << 20, 4, 64u, 64u},          // 4096 chunks, cap 64
    };
    for (const Pin& x : pins) {
        const SlicePlan p = slice_plan(x.n_q, x.n_r, 0, x.bytes, budget);
        expect(p.n_slices == x.n_slices && p.slice_chunks == x.slice_chunks, x.stage, x.n_q, x.n_r, 0, x.bytes, p);
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("identical: %d cases of the grid, %d pins\n", n_cases, (int)(sizeof(pins) / sizeof(pins[0])));
    return 0;
}
