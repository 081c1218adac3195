// dfe_contig_pool.h -- the books of the process's physically contiguous device blocks.  No HIP header: a plain host program can include it
// (tests/contig_pool_check.cpp).
#pragma once
#include <cstddef>
#include <map>
#include <mutex>
#include <vector>
// Why there is a pool.  Freeing hipDeviceMallocContiguous memory is not safe on the driver this library was developed on: behind a few
// dozen allocate / free cycles of contiguous blocks, LATER allocations of the process (contiguous or not) read and write other memory in
// 4-KiB pieces (tools/contig_free_probe.hip shows it without any library code).  So a contiguous block that its
// owner lets go of is not freed: it waits here, idle, for the next contiguous request of its device that it can hold.
// The contract:
//   add(device, p, bytes)      a block the driver just granted; it is in use
//   take(device, bytes, &got)  the smallest idle block of `device` with at least `bytes` bytes, now in use, its size in got; else nullptr.
//                              The block may be larger than asked: its user owns all of it
//   release(p)                 NotPooled: p is not a contiguous block (the caller frees it); Idle: p went idle; NotInUse: p is idle already
//                              (a second free: refused, the block stays where it is)
//   trim(device, keep, out)    takes idle blocks of `device` off the books, largest first, until at most `keep` idle bytes stay; the caller
//                              frees what it gets in `out`.  Returns the idle bytes that stay
//   idle_bytes(device)         what a trim to 0 would take
// One mutex; nothing here touches the device.
class DfeContigPool {
public:
    enum Released { NotPooled, Idle, NotInUse };
    void add(int device, void *p, size_t bytes) {
        std::lock_guard<std::mutex> lock(mu_);
        blocks_[p] = Block{device, bytes, false};
    }
    void *take(int device, size_t bytes, size_t *got) {
        std::lock_guard<std::mutex> lock(mu_);
        auto best = blocks_.end();
        for (auto it = blocks_.begin(); it != blocks_.end(); ++it)
            if (it->second.idle && it->second.device == device && it->second.bytes >= bytes && (best == blocks_.end() || it->second.bytes < best->second.bytes)) best = it;
        if (best == blocks_.end()) return nullptr;
        best->second.idle = false;
        *got = best->second.bytes;
        return best->first;
    }
    Released release(void *p) {
        std::lock_guard<std::mutex> lock(mu_);
        auto it = blocks_.find(p);
        if (it == blocks_.end()) return NotPooled;
        if (it->second.idle) return NotInUse;
        it->second.idle = true;
        return Idle;
    }
    size_t idle_bytes(int device) {
        std::lock_guard<std::mutex> lock(mu_);
        return idle_locked(device);
    }
    size_t trim(int device, size_t keep, std::vector<void *> *out) {
        std::lock_guard<std::mutex> lock(mu_);
        size_t idle = idle_locked(device);
        while (idle > keep) {
            auto big = blocks_.end();
            for (auto it = blocks_.begin(); it != blocks_.end(); ++it)
                if (it->second.idle && it->second.device == device && (big == blocks_.end() || it->second.bytes > big->second.bytes)) big = it;
            idle -= big->second.bytes;
            out->push_back(big->first);
            blocks_.erase(big);
        }
        return idle;
    }

private:
    struct Block { int device; size_t bytes; bool idle; };
    size_t idle_locked(int device) const {
        size_t n = 0;
        for (const auto &kv : blocks_)
            if (kv.second.idle && kv.second.device == device) n += kv.second.bytes;
        return n;
    }
    std::mutex mu_;
    std::map<void *, Block> blocks_;
};
