// tests/san/san_check.hpp — TEST INFRASTRUCTURE ONLY: what the sanitizer drivers beside it
// (abi_driver.cpp, proposer_driver.cpp, unmarshal_driver.cpp, commit_driver.cpp) share: the check
// macros and the guarded buffers of the staging checks.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mpx.h"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                                    \
        }                                                                  \
    } while (0)
// a failure on a live handle names its reason
#define FAILS(e, call, code)                                   \
    do {                                                       \
        const int _rc = (call);                                \
        if (_rc != (code)) fprintf(stderr, "  got %d: %s\n", _rc, mpx_last_error(e)); \
        CHECK(_rc == (code));                                  \
        CHECK(strlen(mpx_last_error(e)) > 0);                  \
    } while (0)

// ---- staging checks -----------------------------------------------------------------------------
// The stub's launchers (hip_stub.cpp, "kernel launchers") read every input byte, fill their k-th
// pure output with the byte 0xA0 + k over exactly the extent the kernel may write, copy state
// across and invert every byte of the other in/out arrays. So through a host form: an output holds
// its pattern over its extent, the guard bytes behind it are untouched, state comes back as it
// went in and the other in/out arrays come back inverted over their extent. A staging slot that
// is too small, misplaced or overlapping breaks one of these (or faults under ASan).
constexpr size_t kGuard = 64;
constexpr uint8_t kGuardByte = 0x5C;

// an output array of `bytes` bytes, guard bytes behind it
struct Out {
    std::vector<uint8_t> v;
    size_t bytes;
    explicit Out(size_t b) : v(b + kGuard, kGuardByte), bytes(b) {}
    template <typename T>
    T* as() { return reinterpret_cast<T*>(v.data()); }
    size_t cap() const { return v.size(); }
    // the pattern of output k over the first n bytes (default: the whole extent), guards intact
    bool is(int k, size_t n) const {
        for (size_t i = 0; i < v.size(); ++i)
            if (v[i] != (i < n ? (uint8_t)(0xA0 + k) : kGuardByte)) return false;
        return true;
    }
    bool is(int k) const { return is(k, bytes); }
    bool untouched() const { return is(0, 0); }
};

// an input or in/out array of `bytes` distinctive bytes (and as distinctive guard bytes)
struct In {
    std::vector<uint8_t> v, orig;
    size_t bytes;
    In(size_t b, unsigned seed) : v(b + kGuard), bytes(b) {
        for (size_t i = 0; i < v.size(); ++i) v[i] = (uint8_t)(seed * 29 + i * 13 + (i >> 8));
        orig = v;
    }
    template <typename T>
    T* as() { return reinterpret_cast<T*>(v.data()); }
    bool intact() const { return v == orig; }
    // an in/out array that is not state: every byte of the extent inverted, guards intact
    bool flipped() const {
        for (size_t i = 0; i < v.size(); ++i)
            if (v[i] != (uint8_t)(i < bytes ? ~orig[i] : orig[i])) return false;
        return true;
    }
};
// ... holding n elements the entry point validates, instead of the distinctive bytes
template <typename T>
In holding(const T* p, size_t n, unsigned seed) {
    In x(n * sizeof(T), seed);
    if (n) memcpy(x.v.data(), p, n * sizeof(T));
    x.orig = x.v;
    return x;
}
// out holds in's bytes over its extent (state copied across), guards intact
inline bool carries(const Out& out, const In& in) {
    for (size_t i = 0; i < out.v.size(); ++i)
        if (out.v[i] != (i < out.bytes ? in.orig[i] : kGuardByte)) return false;
    return true;
}
