// contig_pool_check.cpp -- csrc/dfe_contig_pool.h as a host program (tests/test_contig_pool_cpu.py builds and runs it under the
// sanitizers): reuse, a larger block than asked, the smallest block that fits, per-device keying, a second release, trim.
#include "dfe_contig_pool.h"
#include <cstdio>
#include <cstdlib>

#define REQUIRE(x) do { if (!(x)) { printf("line %d: %s\n", __LINE__, #x); return 1; } } while (0)

int main() {
    static char mem[6][16];   // six addresses that stand for blocks
    void *a = mem[0], *b = mem[1], *c = mem[2], *d = mem[3], *e = mem[4];
    DfeContigPool pool;
    size_t got = 0;
    // nothing idle: nothing to take; a pointer the pool does not know is the caller's to free
    REQUIRE(pool.take(0, 1, &got) == nullptr);
    REQUIRE(pool.release(mem[5]) == DfeContigPool::NotPooled);
    // a block in use is not handed out; released, it is reused for the same size
    pool.add(0, a, 3000);
    REQUIRE(pool.take(0, 3000, &got) == nullptr && pool.idle_bytes(0) == 0);
    REQUIRE(pool.release(a) == DfeContigPool::Idle && pool.idle_bytes(0) == 3000);
    REQUIRE(pool.take(0, 3000, &got) == a && got == 3000 && pool.idle_bytes(0) == 0);
    // a second release is refused and leaves the block idle, not doubly so: it is handed out once
    REQUIRE(pool.release(a) == DfeContigPool::Idle);
    REQUIRE(pool.release(a) == DfeContigPool::NotInUse && pool.idle_bytes(0) == 3000);
    REQUIRE(pool.take(0, 10, &got) == a && got == 3000);          // larger than asked: the size says so
    REQUIRE(pool.take(0, 10, &got) == nullptr);
    REQUIRE(pool.release(a) == DfeContigPool::Idle);
    // a request that no idle block holds gets none; of several that do, the smallest
    pool.add(0, b, 26000);
    pool.add(0, c, 9000);
    REQUIRE(pool.release(b) == DfeContigPool::Idle && pool.release(c) == DfeContigPool::Idle);
    REQUIRE(pool.take(0, 26001, &got) == nullptr);
    REQUIRE(pool.take(0, 3001, &got) == c && got == 9000);
    REQUIRE(pool.take(0, 3001, &got) == b && got == 26000);
    REQUIRE(pool.take(0, 3001, &got) == nullptr);
    REQUIRE(pool.release(b) == DfeContigPool::Idle && pool.release(c) == DfeContigPool::Idle);
    // a device sees its own blocks only
    pool.add(1, d, 5000);
    pool.add(1, e, 100);
    REQUIRE(pool.release(d) == DfeContigPool::Idle && pool.release(e) == DfeContigPool::Idle);
    REQUIRE(pool.idle_bytes(0) == 38000 && pool.idle_bytes(1) == 5100 && pool.idle_bytes(2) == 0);
    REQUIRE(pool.take(1, 6000, &got) == nullptr);                  // (device 0 has two that would do)
    REQUIRE(pool.take(1, 200, &got) == d && got == 5000);
    REQUIRE(pool.take(0, 4000, &got) == c);                        // (device 1's idle block of 100 bytes is not in the way)
    REQUIRE(pool.release(c) == DfeContigPool::Idle);
    // trim: idle blocks of one device, largest first, down to the bound; blocks in use and other devices stay
    std::vector<void *> out;
    REQUIRE(pool.trim(0, (size_t)-1, &out) == 38000 && out.empty());
    REQUIRE(pool.trim(0, 12000, &out) == 12000 && out.size() == 1 && out[0] == b);
    out.clear();
    REQUIRE(pool.trim(0, 11999, &out) == 3000 && out.size() == 1 && out[0] == c);
    out.clear();
    REQUIRE(pool.trim(1, 0, &out) == 0 && out.size() == 1 && out[0] == e);     // (d is in use)
    REQUIRE(pool.release(b) == DfeContigPool::NotPooled);          // off the books: the caller's to free
    REQUIRE(pool.release(d) == DfeContigPool::Idle && pool.idle_bytes(1) == 5000 && pool.idle_bytes(0) == 3000);
    out.clear();
    REQUIRE(pool.trim(0, 0, &out) == 0 && out.size() == 1 && out[0] == a && pool.take(0, 1, &got) == nullptr);
    printf("ok\n");
    return 0;
}
