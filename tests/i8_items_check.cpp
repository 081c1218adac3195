// Stand-alone check of csrc/flow_i8_items.h, the int8 flow sweep's split of a step's rows into wave items (tests/test_flow_i8_items_cpu.py
// builds it with the sanitizers and runs it).  For every (Ho, nstrips, slots) below: the items, decoded as the kernel decodes them,
// write every (strip, row) exactly once; the final round holds the number of items the plan states, and that is at least as many as the
// final round of two-row items alone, unless the plan is a single round; the plan's modelled time is never above that of two-row items
// alone; shapes whose two-row items fill whole rounds keep them.
#include "flow_i8_items.h"

#include <cstdio>
#include <vector>

static int fails = 0;
#define CHECK(c, ...)                                                          \
    do {                                                                       \
        if (!(c)) {                                                            \
            if (++fails < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                      \
    } while (0)

static void one(int Ho, int nstrips, long long slots) {
    const I8ItemPlan p = flow_i8_item_plan(Ho, nstrips, slots);
    const long long rows = (long long)nstrips * Ho, total2 = (long long)nstrips * ((Ho + 1) / 2);
    std::vector<unsigned char> writers((size_t)rows, 0);
    CHECK(p.nrp == (Ho + 1) / 2 && p.n2 >= 0 && p.n1 >= 0 && p.n2 + p.n1 > 0, "Ho %d nstrips %d slots %lld", Ho, nstrips, slots);
    CHECK(Ho >= 2 || p.n2 == 0, "two-row items of a one-row frame: Ho %d", Ho);
    for (long long i = 0; i < p.n2 + p.n1; ++i) {   // as ssd_flow_i8_kernel decodes an item
        if (i < p.n2) {
            const long long strip = i / p.nrp, rp = i - strip * p.nrp;
            const long long y0 = 2 * rp < Ho - 2 ? 2 * rp : Ho - 2, ylo = 2 * rp;
            CHECK(strip < nstrips && y0 >= 0 && y0 + 1 < Ho, "two-row item %lld: strip %lld rows %lld..", i, strip, y0);
            if (strip >= nstrips || y0 < 0 || y0 + 1 >= Ho) continue;
            for (long long y = y0; y < y0 + 2; ++y)
                if (y >= ylo) ++writers[(size_t)(strip * Ho + y)];
        } else {
            const long long row = p.row0 + (i - p.n2);
            CHECK(row >= 0 && row < rows, "one-row item %lld: row %lld of %lld", i, row, rows);
            if (row < 0 || row >= rows) continue;
            ++writers[(size_t)row];   // (strip row / Ho, row row % Ho)
        }
    }
    long long bad = 0;
    for (long long r = 0; r < rows; ++r) bad += writers[(size_t)r] != 1;
    CHECK(bad == 0, "Ho %d nstrips %d slots %lld: %lld cells without exactly one writer", Ho, nstrips, slots, bad);

    // rounds: whole rounds of two-row items, then rounds of one-row items
    const long long s = slots < 1 ? 1 : slots;
    CHECK(p.n1 == 0 || p.n2 % s == 0, "Ho %d nstrips %d slots %lld: one-row items behind a broken round (%lld two-row items)", Ho, nstrips, slots, p.n2);
    const long long tail = p.n1 ? p.n1 : p.n2, rounds = (p.n1 ? p.n2 / s : 0) + (tail + s - 1) / s, last = tail - (tail - 1) / s * s;
    CHECK(rounds == p.rounds && last == p.last, "Ho %d nstrips %d slots %lld: rounds %lld (%lld stated), last %lld (%lld stated)", Ho, nstrips, slots, rounds, p.rounds, last, p.last);
    const long long rounds_u = (total2 + s - 1) / s, last_u = total2 - (total2 - 1) / s * s;
    if (Ho >= 2) {
        CHECK(p.rounds == 1 || p.last >= last_u, "Ho %d nstrips %d slots %lld: final round %lld items, two-row items alone %lld", Ho, nstrips, slots, p.last, last_u);
        const double t = p.n1 ? (double)(p.n2 / s) + kI8OneRowCost * (double)((p.n1 + s - 1) / s) : (double)rounds;
        CHECK(t <= (double)rounds_u, "Ho %d nstrips %d slots %lld: modelled time %.2f, two-row items alone %lld", Ho, nstrips, slots, t, rounds_u);
        if (total2 % s == 0) CHECK(p.n1 == 0 && p.n2 == total2, "Ho %d nstrips %d slots %lld: whole rounds of two-row items not kept", Ho, nstrips, slots);
    }
}

int main() {
    const int Hos[] = {1, 2, 3, 7, 442, 682, 1042}, strips[] = {1, 2, 38, 118};
    const long long slots[] = {4, 12, 2048, 3072};
    for (int Ho : Hos)
        for (int ns : strips)
            for (long long s : slots) one(Ho, ns, s);
    // the slot counts of the GPU test's small shapes, and around them
    for (int Ho = 1; Ho <= 12; ++Ho)
        for (int ns = 1; ns <= 4; ++ns)
            for (long long s = 1; s <= 30; ++s) one(Ho, ns, s);
    one(3, 2, 0);
    // the frames of the benchmark at three waves per SIMD: VGA and 720p keep their two-row items, 1080p's 0.01 of a round goes to one-row items
    {
        const I8ItemPlan v = flow_i8_item_plan(442, 38, 3072), h = flow_i8_item_plan(682, 78, 3072), f = flow_i8_item_plan(1042, 118, 3072);
        CHECK(v.n1 == 0 && v.rounds == 3, "vga: n1 %lld rounds %lld", v.n1, v.rounds);
        CHECK(h.n1 == 0 && h.rounds == 9, "720p: n1 %lld rounds %lld", h.n1, h.rounds);
        CHECK(f.n2 == 20 * 3072 && f.n1 == 76 && f.rounds == 21, "1080p: n2 %lld n1 %lld rounds %lld", f.n2, f.n1, f.rounds);
    }
    if (fails) { printf("%d failures\n", fails); return 1; }
    printf("ok\n");
    return 0;
}
