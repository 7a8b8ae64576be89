// work_bytes_check.cpp — host-only check of the families' scratch sizes
// (tests/test_work_bytes.py).
// Links libmpx.so, calls no HIP function, needs no GPU.
//
// A _dev entry point never allocates: it runs in whatever mpx_*_reserve(max) put aside, so
//   1. every x_work_bytes must not decrease in its size arguments (a reservation for a maximum
//      covers every smaller call);
//   2. apply_reserve_bytes(t, o, m) must cover apply_work_bytes(t, o, m') for every m' <= m, on
//      every pipeline the handle's settings can pick;
//   3. the regions a family carves from a base must lie inside [base, base + work_bytes), each
//      256-byte aligned and starting at or after the end of the one before (scratch.hpp's Carver
//      reports them; the fan-out has two alternative carve-ups, each starting at the base).
// Sizes: every value 0..70000, a geometric ladder with its +-1 neighbours up to 2^31 - 2, and
// 2^k +- 2 for k = 10..30.
// It also prints a hash of all totals per family, to compare two builds of the library.
// Built against the csrc/ of a commit from before scratch.hpp (and run on its library) it
// skips 3, which needs the Carver argument of the size functions.
//   work_bytes_check [--write-decode FILE | --compare-decode FILE]
// writes the decode totals, or prints their largest difference from a written file.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kernels.hpp"
using namespace mpx;
// SIZE_OF(fn, args in x): the family's size function of x, carved on the Probe it is handed
#if __has_include("scratch.hpp")
using Probe = Carver;
constexpr bool kHaveCarver = true;
#define SIZE_OF(fn, ...) [=](uint64_t x, Probe&& c) { return fn(__VA_ARGS__, std::move(c)); }
#else
struct Probe {};
constexpr bool kHaveCarver = false;
#define SIZE_OF(fn, ...) [=](uint64_t x, Probe&&) { return fn(__VA_ARGS__); }
#endif

namespace {
int g_fail = 0;
void fail(const char* what, const char* fam, uint64_t a, uint64_t b) {
    if (++g_fail <= 20)
        std::printf("FAIL %s: %s at %llu (%llu)\n", what, fam, (unsigned long long)a,
                    (unsigned long long)b);
}

std::vector<uint64_t> sizes() {
    const uint64_t top = (1ull << 31) - 2;
    std::vector<uint64_t> v;
    for (uint64_t i = 0; i <= 70000; ++i) v.push_back(i);
    for (double x = 70001; x < (double)top; x *= 1.19) {
        const uint64_t u = (uint64_t)x;
        v.insert(v.end(), {u - 1, u, u + 1});
    }
    for (int k = 10; k <= 30; ++k) v.insert(v.end(), {(1ull << k) - 2, (1ull << k) + 2});
    v.insert(v.end(), {top - 1, top});
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}

struct Hash {  // FNV-1a over the totals
    uint64_t h = 1469598103934665603ull;
    void add(uint64_t x) {
        for (int i = 0; i < 8; ++i, x >>= 8) h = (h ^ (x & 255)) * 1099511628211ull;
    }
};

// 3: the regions of one carve-up
template <typename F>
void regions_ok(const char* fam, uint64_t at, uint64_t total, F size_of) {
#if __has_include("scratch.hpp")
    char* const base = (char*)(1ull << 40);  // never dereferenced
    std::vector<Region> seen;
    const uint64_t got = size_of(at, Carver(base, &seen));
    if (got != total) fail("carved total differs from work_bytes", fam, at, got);
    const char* end = base;  // of the region before
    for (const Region& r : seen) {
        const char* p = (const char*)r.p;
        if (p == base) end = base;  // an alternative carve-up of the same bytes
        if (((uintptr_t)p & 255) || p < end || p + r.bytes > base + total)
            fail("region outside, out of order or misaligned", fam, at, (uint64_t)(p - base));
        end = p + r.bytes;
    }
#endif
}

// 1 (where the family's size must not decrease) and 3 over the ascending sizes; returns the totals
template <typename F>
std::vector<uint64_t> family(const char* name, const std::vector<uint64_t>& S, bool monotone,
                             F size_of) {
    std::vector<uint64_t> tot;
    uint64_t prev = 0, top = 0;
    Hash h;
    for (const uint64_t s : S) {
        const uint64_t b = size_of(s, Probe());
        if (monotone && b < prev) fail("work_bytes decreases", name, s, b);
        regions_ok(name, s, b, size_of);
        prev = b;
        top = std::max(top, b);
        tot.push_back(b);
        h.add(b);
    }
    std::printf("%-28s max %14llu  hash %016llx\n", name, (unsigned long long)top,
                (unsigned long long)h.h);
    return tot;
}
}  // namespace

int main(int argc, char** argv) {
    const std::vector<uint64_t> S = sizes();
    std::printf("%zu sizes, region check %s\n", S.size(),
                kHaveCarver ? "on" : "skipped (no scratch.hpp)");

    const std::vector<uint64_t> dec = family("decode", S, true, SIZE_OF(decode_work_bytes, x));
    family("stream", S, true, SIZE_OF(stream_work_bytes, x));
    family("fanout", S, true, SIZE_OF(fanout_work_bytes, x));
    family("accept_replies", S, true, SIZE_OF(accept_replies_work_bytes, x));
    family("unmarshal (n, n_log = n)", S, true, SIZE_OF(unmarshal_work_bytes, x, x));
    family("unmarshal (n = 1000, n_log)", S, true, SIZE_OF(unmarshal_work_bytes, 1000, x));
    family("commits (N = 5, sends, other = 0)", S, true, SIZE_OF(commits_work_bytes, 5, x, 0));
    family("commits (N = 16, sends = other)", S, true, SIZE_OF(commits_work_bytes, 16, x, x));
    family("commits (sends = 0, other)", S, true, SIZE_OF(commits_work_bytes, 1, 0, x));
    family("logenc (n, m = 4n)", S, true, SIZE_OF(logenc_work_bytes, x, 4 * x));
    family("logenc (n = 1000, m)", S, true, SIZE_OF(logenc_work_bytes, 1000, x));
    family("client (len, 1000 conns, 16 groups)", S, true, SIZE_OF(client_work_bytes, x, 1000, 16));
    family("client (len = 2^20, conns)", S, true, SIZE_OF(client_work_bytes, 1 << 20, x, 16));
    family("client (len = 2^20, groups)", S, true, SIZE_OF(client_work_bytes, 1 << 20, 1000, x));
    family("replies (sends)", S, true, SIZE_OF(reply_work_bytes, x));
    family("execute (slots, 1000 groups)", S, true, SIZE_OF(execute_work_bytes, x, 1000));
    family("execute (2^20 slots, groups)", S, true, SIZE_OF(execute_work_bytes, 1 << 20, x));
    family("record (items)", S, true, SIZE_OF(record_work_bytes, x));
    family("accepts stored (N = 5, sends, 2^16 slots)", S, true,
           SIZE_OF(accepts_stored_work_bytes, 5, x, 1 << 16));
    family("accepts stored (N = 16, 1000 sends, slots)", S, true,
           SIZE_OF(accepts_stored_work_bytes, 16, 1000, x));
    family("prepare replies (N = 5, replies, 2^16 slots)", S, true,
           SIZE_OF(prepare_replies_work_bytes, 5, x, 1 << 16));
    family("prepare replies (N = 16, 1000 replies, slots)", S, true,
           SIZE_OF(prepare_replies_work_bytes, 16, 1000, x));
    family("prepare replies (gather: 1, frames, 0)", S, true,
           SIZE_OF(prepare_replies_work_bytes, 1, x, 0));
    for (const int32_t cap : {1, 8192, 1 << 20, 1 << 24, 1 << 25}) {
        char name[64];
        std::snprintf(name, sizeof(name), "replay (inst_cap %d)", cap);
        family(name, S, true, SIZE_OF(replay_work_bytes, x, cap));
    }

    // 2: the reservation covers every smaller call (the running maximum of work_bytes, which
    // falls where the call changes pipeline)
    for (const int lg : {10, 21, 24})
        for (const uint32_t path :
             {MPX_APPLY_AUTO, MPX_APPLY_SORTED, MPX_APPLY_PARTITIONED, MPX_APPLY_SMALL})
            for (const uint32_t fast_min : {0u, 100000u}) {
                KvTable t{};
                t.cap = 1ull << lg;
                t.lgnb = (uint32_t)lg - 8;
                const ApplyOpts o{0, path, fast_min, 0};
                char name[64];
                std::snprintf(name, sizeof(name), "apply 2^%d path %u min %u", lg, path, fast_min);
                const std::vector<uint64_t> tot =
                    family(name, S, false, SIZE_OF(apply_work_bytes, t, o, x));
                uint64_t need = 0;
                for (size_t i = 0; i < S.size(); ++i) {
                    need = std::max(need, tot[i]);
                    if (apply_reserve_bytes(t, o, S[i]) < need)
                        fail("reserve below a smaller call", name, S[i], need);
                }
            }

    if (argc == 3 && !std::strcmp(argv[1], "--write-decode")) {
        FILE* f = std::fopen(argv[2], "wb");
        if (!f || std::fwrite(dec.data(), 8, dec.size(), f) != dec.size()) return 2;
        std::fclose(f);
    } else if (argc == 3 && !std::strcmp(argv[1], "--compare-decode")) {
        std::vector<uint64_t> old(dec.size());
        FILE* f = std::fopen(argv[2], "rb");
        if (!f || std::fread(old.data(), 8, old.size(), f) != old.size()) return 2;
        std::fclose(f);
        int64_t lo = 0, hi = 0;
        for (size_t i = 0; i < dec.size(); ++i) {
            lo = std::min(lo, (int64_t)(dec[i] - old[i]));
            hi = std::max(hi, (int64_t)(dec[i] - old[i]));
        }
        std::printf("decode totals against %s: from %lld to %+lld bytes\n", argv[2], (long long)lo,
                    (long long)hi);
        if (lo <= -5 * 256 || hi >= 5 * 256)
            fail("decode total moved by 5 x 256 bytes or more", "decode", 0, 0);
    }
    if (g_fail) {
        std::printf("%d failures\n", g_fail);
        return 1;
    }
    std::printf("work_bytes ok\n");
    return 0;
}
