// dfe_carve.h -- how every launcher lays its buffers out in a block of device memory.  No HIP header: a plain host program can include it.
#pragma once
#include <cstddef>
// A launcher writes its layout ONCE, as a function over a DfeCarve that takes the buffers in order and returns their pointers.  Run with
// no base, the pass gives the block's size in `off` (every pointer nullptr); run again on the block, it gives the addresses.  Every
// buffer starts on a 256-byte boundary of the block; a take of no elements returns nullptr and uses no space.
struct DfeCarve {
    char *base;
    size_t off = 0;
    explicit DfeCarve(void *b = nullptr) : base((char *)b) {}
    static size_t up(size_t bytes) { return (bytes + 255) / 256 * 256; }
    template <class T> T *take(size_t n) {
        T *p = (base && n) ? (T *)(base + off) : nullptr;
        off += up(n * sizeof(T));
        return p;
    }
};
