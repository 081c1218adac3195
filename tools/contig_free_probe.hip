// contig_free_probe.hip -- stand-alone: does freeing physically contiguous device memory (hipExtMallocWithFlags, hipDeviceMallocContiguous)
// leave later allocations of the process reading or writing other memory?  No library code: allocate, fill with one kernel, count the wrong
// words with a second kernel and again on the host, free; a few dozen cycles of the sizes libdfe's arenas take.
//   hipcc --offload-arch=gfx950 -O2 tools/contig_free_probe.hip -o contig_free_probe && ./contig_free_probe [cycles] [contig 0/1]
// Prints one line per block with wrong words and a total; exit status 1 if any word was wrong.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(2); } } while (0)

__global__ void fill_kernel(unsigned *p, size_t n, unsigned salt) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = (unsigned)i * 2654435761u + salt;
}
__global__ void count_kernel(const unsigned *p, size_t n, unsigned salt, unsigned long long *wrong) {
    unsigned long long w = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) w += p[i] != (unsigned)i * 2654435761u + salt;
    if (w) atomicAdd(wrong, w);
}

static unsigned long long *g_wrong;
static unsigned g_salt = 1;
static long long g_total = 0;

static void *alloc(size_t bytes, bool contig) {
    void *p = nullptr;
    if (contig && hipExtMallocWithFlags(&p, bytes, hipDeviceMallocContiguous) == hipSuccess) return p;
    (void)hipGetLastError();
    CHECK(hipMalloc(&p, bytes));
    return p;
}

// fill the block from the device, count wrong words from the device (another launch) and on the host, by 4-KiB page
static void use(void *p, size_t bytes, const char *what, int cycle) {
    const size_t n = bytes / 4;
    const unsigned salt = g_salt++;
    CHECK(hipMemset(g_wrong, 0, 8));
    hipLaunchKernelGGL(fill_kernel, dim3(1024), dim3(256), 0, 0, (unsigned *)p, n, salt);
    hipLaunchKernelGGL(count_kernel, dim3(777), dim3(256), 0, 0, (const unsigned *)p, n, salt, g_wrong);
    unsigned long long dev = 0;
    CHECK(hipMemcpy(&dev, g_wrong, 8, hipMemcpyDeviceToHost));
    std::vector<unsigned> h(n);
    CHECK(hipMemcpy(h.data(), p, n * 4, hipMemcpyDeviceToHost));
    size_t host = 0, pages = 0;
    for (size_t i = 0; i < n; i += 1024) {
        size_t w = 0;
        for (size_t j = i; j < n && j < i + 1024; ++j) w += h[j] != (unsigned)j * 2654435761u + salt;
        host += w;
        pages += w != 0;
    }
    if (dev || host) {
        printf("cycle %d %s %p %zu bytes: %llu words wrong as the device reads them, %zu as the host does, in %zu of %zu 4-KiB pages\n", cycle, what, p, bytes, dev,
               host, pages, (n + 1023) / 1024);
        g_total += (long long)(dev + host);
    }
}

int main(int argc, char **argv) {
    const int cycles = argc > 1 ? atoi(argv[1]) : 40;
    const bool contig = argc > 2 ? atoi(argv[2]) != 0 : true;
    CHECK(hipMalloc((void **)&g_wrong, 8));
    // a context's life as the arena tests make it: a small flag, a contiguous arena that grows once or twice (freed, allocated larger), a
    // plain arena, a side buffer; everything freed at the end
    const size_t sizes[] = {2830464, 3184128, 716800, 26214400, 12441600, 1064960, 5505024, 9437184};
    for (int c = 0; c < cycles; ++c) {
        void *flag = alloc(4, false);
        void *a = alloc(sizes[c % 8], contig);
        use(a, sizes[c % 8], "arena", c);
        void *plain = alloc(sizes[(c + 1) % 8], false);
        use(plain, sizes[(c + 1) % 8], "plain", c);
        CHECK(hipDeviceSynchronize());
        CHECK(hipFree(a));
        a = alloc(sizes[(c + 3) % 8] + 4096 * (size_t)(c % 5), contig);
        use(a, sizes[(c + 3) % 8], "arena, grown", c);
        void *aux = alloc(sizes[(c + 5) % 8] / 4, false);
        use(aux, sizes[(c + 5) % 8] / 4, "side", c);
        use(plain, sizes[(c + 1) % 8], "plain, again", c);
        CHECK(hipDeviceSynchronize());
        CHECK(hipFree(a)); CHECK(hipFree(plain)); CHECK(hipFree(aux)); CHECK(hipFree(flag));
    }
    printf("%d cycles, contiguous %d: %lld wrong words in all\n", cycles, (int)contig, g_total);
    return g_total ? 1 : 0;
}
