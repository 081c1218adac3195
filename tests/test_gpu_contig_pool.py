"""The pool of physically contiguous blocks through the C ABI (include/dfe.h at dfe_device_alloc; csrc/dfe_contig_pool.h has the books,
tests/test_contig_pool_cpu.py tests them on the host): a freed block is reused, a smaller request gets the same, larger block, a second
dfe_device_free is refused and the block is handed out once, and dfe_contig_pool_trim reports what lies idle.  The sizes are chosen above
everything that lies idle in the process, so that no block of another test can serve them; nothing is given back to the driver here
(keep_bytes = SIZE_MAX): that is the operation the pool exists to avoid."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu
MiB = 1 << 20
SIZE_MAX = C.c_size_t(-1).value


def test_device_alloc_reuses_contiguous_blocks(dfe, cuda):
    from depth_estimation_amd.context import Context

    lib, ctx = dfe.lib(), Context(0)

    def idle():
        n = C.c_size_t(0)
        ctx.check(lib.dfe_contig_pool_trim(ctx.handle, SIZE_MAX, C.byref(n)))
        return n.value

    def alloc(nbytes):
        p, contig = C.c_void_p(), C.c_int(-1)
        ctx.check(lib.dfe_device_alloc(ctx.handle, nbytes, C.byref(p), C.byref(contig)))
        assert contig.value == 1, "the driver granted no contiguous block: the pool is not involved"
        return p.value

    try:
        idle0 = idle()
        n = idle0 + 3 * MiB                                  # more than all idle blocks together: a new block
        p1 = alloc(n)
        assert idle() == idle0
        ctx.check(lib.dfe_device_free(ctx.handle, p1))
        assert idle() == idle0 + n                           # idle, not freed
        assert alloc(n) == p1 and idle() == idle0            # reused
        ctx.check(lib.dfe_device_free(ctx.handle, p1))
        assert alloc(n - MiB) == p1                          # a smaller request that only this block holds: the larger block
        ctx.check(lib.dfe_device_free(ctx.handle, p1))
        rc = lib.dfe_device_free(ctx.handle, p1)             # a second free: refused, nothing changes
        assert rc != 0 and idle() == idle0 + n, (rc, ctx.last_error())
        p2 = alloc(n - MiB)
        p3 = alloc(n - MiB)
        assert p2 == p1 and p3 != p1                         # handed out once
        ctx.check(lib.dfe_device_free(ctx.handle, p2))
        ctx.check(lib.dfe_device_free(ctx.handle, p3))
        assert idle() == idle0 + n + (n - MiB)
        assert lib.dfe_device_free(ctx.handle, None) == 0
    finally:
        ctx.close()
