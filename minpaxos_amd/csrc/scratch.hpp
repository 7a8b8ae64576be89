// scratch.hpp — a family's scratch described once (host only): its struct of typed pointers is
// built from a Carver and the call's sizes, by x_work_bytes on no base (it returns bytes()) and by
// launch_x on the engine's buffer (it refuses the call when bytes() exceeds what it was given).
// The _dev entry points never allocate, so a size that drifted from its carve-up would be a write
// past engine-owned memory: here there is nothing to drift.
#pragma once
#include <stdint.h>

#include <vector>

namespace mpx {

struct Region {
    void* p;
    uint64_t bytes;
};

struct Carver {
    char* base;                 // nullptr: sizes only
    std::vector<Region>* seen;  // (optional) every region handed out (work_bytes_check.cpp)
    uint64_t end = 0;
    explicit Carver(void* b = nullptr, std::vector<Region>* s = nullptr) : base((char*)b), seen(s) {}
    // the next 256-byte aligned region of count T (nullptr when there is no base)
    template <typename T>
    T* take(uint64_t count) {
        char* const p = base ? base + end : nullptr;
        const uint64_t n = (count * sizeof(T) + 255) & ~255ull;
        end += n;
        if (seen) seen->push_back(Region{p, n});
        return reinterpret_cast<T*>(p);
    }
    uint64_t bytes() const { return end; }
};

}  // namespace mpx
