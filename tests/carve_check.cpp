// carve_check.cpp -- a host program over csrc/dfe_carve.h, built and run by tests/test_carve_cpu.py under ASan / UBSan.
// Exit status 0 and "ok" on stdout when every check holds; the first failed check prints its line and exits 1.
#include "dfe_carve.h"
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(c) do { if (!(c)) { printf("carve_check.cpp:%d: %s\n", __LINE__, #c); exit(1); } } while (0)

struct F2 { float x, y; };   // float2-sized elements
struct Bufs { float *a; double *b; F2 *c; int64_t *d; float *none; unsigned char *e; };

// one layout, as a launcher writes it: n elements of every type, a take of nothing in the middle
static Bufs lay(DfeCarve &c, size_t n) {
    Bufs r;
    r.a = c.take<float>(n);
    r.b = c.take<double>(n);
    r.none = c.take<float>(0);
    r.c = c.take<F2>(n);
    r.d = c.take<int64_t>(n);
    r.e = c.take<unsigned char>(n);
    return r;
}

int main() {
    for (size_t n : {(size_t)1, (size_t)63, (size_t)64, (size_t)65}) {
        DfeCarve plan;
        const Bufs p = lay(plan, n);
        CHECK(!p.a && !p.b && !p.c && !p.d && !p.e && !p.none);   // sizes only: no pointer is formed
        CHECK(plan.off % 256 == 0 && plan.off >= n * (4 + 8 + 8 + 8 + 1));
        // a block of exactly plan.off bytes on a 256-byte boundary: ASan sees a write one byte past any buffer that ends the block
        void *mem = aligned_alloc(256, plan.off);
        CHECK(mem);
        DfeCarve c(mem);
        const Bufs r = lay(c, n);
        CHECK(c.off == plan.off);                                  // both passes agree
        CHECK(r.none == nullptr);                                  // a zero take: no pointer ...
        {
            DfeCarve with(mem), without(mem);
            with.take<float>(n); with.take<double>(0); with.take<float>(n);
            without.take<float>(n); without.take<float>(n);
            CHECK(with.off == without.off);                        // ... and no space
        }
        struct Span { char *p; size_t bytes; } s[5] = {{(char *)r.a, n * sizeof(float)}, {(char *)r.b, n * sizeof(double)}, {(char *)r.c, n * sizeof(F2)},
                                                       {(char *)r.d, n * sizeof(int64_t)}, {(char *)r.e, n}};
        for (int i = 0; i < 5; ++i) {
            CHECK(s[i].p && (size_t)(s[i].p - (char *)mem) % 256 == 0);            // 256-byte aligned relative to the base
            CHECK(s[i].p + s[i].bytes <= (char *)mem + plan.off);                  // inside the block
            if (i) CHECK(s[i - 1].p + s[i - 1].bytes <= s[i].p);                   // in order, no overlap
        }
        // fill every buffer through its typed pointer with its own pattern, then read all of them back
        for (size_t i = 0; i < n; ++i) { r.a[i] = 1.f + i; r.b[i] = 2.0 + i; r.c[i] = F2{3.f + i, -3.f - i}; r.d[i] = 4 + (int64_t)i; r.e[i] = (unsigned char)(5 + i); }
        for (size_t i = 0; i < n; ++i)
            CHECK(r.a[i] == 1.f + i && r.b[i] == 2.0 + i && r.c[i].x == 3.f + i && r.c[i].y == -3.f - i && r.d[i] == 4 + (int64_t)i && r.e[i] == (unsigned char)(5 + i));
        free(mem);
    }
    CHECK(DfeCarve::up(0) == 0 && DfeCarve::up(1) == 256 && DfeCarve::up(256) == 256 && DfeCarve::up(257) == 512);
    puts("ok");
    return 0;
}
