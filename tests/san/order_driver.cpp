// tests/san/order_driver.cpp — TEST INFRASTRUCTURE ONLY: drives mpx_order_records and its
// _reserve / _dev forms of the CPU build of engine.cpp + order.cpp over the stub runtime
// (hip_stub.cpp) and the sorting stand-in of order_stub.cpp under ASan + UBSan. Every
// argument-validation path of the host form must answer its code before anything is staged; valid
// calls on guarded buffers must bring back exactly the expected records, permutation and result
// through the staging arena, leave the inputs and the guard bytes alone and write nothing for an
// absent perm. Exit status 0 = all checks passed.
#include <algorithm>

#include "san_check.hpp"

static mpx_engine* open_engine() {
    mpx_engine* e = nullptr;
    mpx_config cfg{5, MPX_MODE_MIN, 1 << 10, 0, 0, 0};
    CHECK(mpx_open(0, &cfg, &e) == MPX_OK && e);
    return e;
}

static bool guards_intact(const Out& o) {
    for (size_t i = o.bytes; i < o.v.size(); ++i)
        if (o.v[i] != kGuardByte) return false;
    return true;
}

// sizes[k] records per source on instances base + (a hash of the position) % n_inst; the call on
// guarded buffers, compared with a stable sort done here
static void valid_case(mpx_engine* e, std::vector<size_t> sizes, size_t n_inst, int32_t base,
                       uint32_t bits, bool with_perm, bool dev) {
    const size_t S = sizes.size();
    size_t n = 0;
    for (size_t k : sizes) n += k;
    std::vector<In> recs, arrs;
    std::vector<mpx_order_src> src(S ? S : 1);
    std::vector<mpx_accept_reply> cat;
    std::vector<uint64_t> key;
    for (size_t s = 0; s < S; ++s) {
        recs.emplace_back(sizes[s] * 16, (unsigned)(3 + 2 * s));
        arrs.emplace_back(sizes[s] * 4, (unsigned)(4 + 2 * s));
    }
    for (size_t s = 0; s < S; ++s) {  // (the vectors no longer move)
        mpx_accept_reply* r = recs[s].as<mpx_accept_reply>();
        uint32_t* a = arrs[s].as<uint32_t>();
        for (size_t i = 0; i < sizes[s]; ++i) {
            r[i].instance = base + (int32_t)((cat.size() * 2654435761u >> 7) % n_inst);
            a[i] = bits ? a[i] & ((bits >= 32 ? 0u : 1u << bits) - 1u) : a[i];
            cat.push_back(r[i]);
            key.push_back(((uint64_t)(r[i].instance - base) << bits) | (bits ? a[i] : 0));
        }
        recs[s].orig = recs[s].v;
        arrs[s].orig = arrs[s].v;
        src[s] = mpx_order_src{sizes[s] ? r : nullptr, bits && sizes[s] ? a : nullptr, sizes[s]};
    }
    std::vector<uint32_t> p(n);
    for (size_t i = 0; i < n; ++i) p[i] = (uint32_t)i;
    std::stable_sort(p.begin(), p.end(), [&](uint32_t x, uint32_t y) { return key[x] < key[y]; });
    Out out(n * 16), perm(n * 4);
    mpx_order_result res[2];
    memset(res, 0x5C, sizeof(res));
    uint32_t* pp = with_perm ? perm.as<uint32_t>() : nullptr;
    if (dev) {
        CHECK(mpx_order_records_reserve(e, n, n_inst) == MPX_OK);
        CHECK(mpx_order_records_dev(e, src.data(), S, n_inst, base, bits, 0, out.as<void>(), pp, res,
                                    nullptr) == MPX_OK);
    } else {
        CHECK(mpx_order_records(e, src.data(), S, n_inst, base, bits, 0, n ? out.as<void>() : nullptr,
                                pp, res) == MPX_OK);
    }
    bool same = true, same_perm = true;
    for (size_t i = 0; i < n; ++i) {
        same &= !memcmp(out.v.data() + 16 * i, &cat[p[i]], 16);
        if (with_perm) same_perm &= perm.as<uint32_t>()[i] == p[i];
    }
    CHECK(same && same_perm && guards_intact(out));
    CHECK(with_perm ? guards_intact(perm) : perm.untouched());
    CHECK(res[0].n == n && res[0].pad == 0 && (n ? res[0].lo <= res[0].hi : res[0].hi == -1));
    const uint8_t* after = (const uint8_t*)&res[1];
    for (size_t i = 0; i < sizeof(res[1]); ++i) CHECK(after[i] == 0x5C);
    for (size_t s = 0; s < S; ++s) CHECK(recs[s].intact() && arrs[s].intact());
}

static void validation(mpx_engine* e) {
    mpx_accept_reply r[4] = {{104, 1, 1, 1, {0, 0, 0}}, {100, 1, 1, 1, {0, 0, 0}},
                             {107, 1, 1, 1, {0, 0, 0}}, {100, 2, 2, 0, {0, 0, 0}}};
    uint32_t a[4] = {3, 1, 2, 0};
    Out out(64), perm(16);
    mpx_order_result res;
    memset(&res, 0x5C, sizeof(res));
    mpx_order_src one[1] = {{r, nullptr, 4}};
    mpx_order_src keyed[2] = {{r, a, 2}, {r + 2, a + 2, 2}};
    auto call = [&](const mpx_order_src* s, size_t ns, size_t n_inst, int32_t base, uint32_t bits,
                    uint32_t flags) {
        return mpx_order_records(e, s, ns, n_inst, base, bits, flags, out.as<void>(),
                                 perm.as<uint32_t>(), &res);
    };
    // null arguments
    FAILS(e, mpx_order_records(e, nullptr, 1, 8, 100, 0, 0, out.as<void>(), nullptr, &res), MPX_E_INVAL);
    FAILS(e, mpx_order_records(e, one, 1, 8, 100, 0, 0, nullptr, nullptr, &res), MPX_E_INVAL);
    FAILS(e, mpx_order_records(e, one, 1, 8, 100, 0, 0, out.as<void>(), nullptr, nullptr), MPX_E_INVAL);
    mpx_order_src norecs[1] = {{nullptr, nullptr, 4}};
    FAILS(e, call(norecs, 1, 8, 100, 0, 0), MPX_E_INVAL);
    // more than MPX_ORDER_MAX_SRC sources, unknown flags, the window, arrival_bits
    std::vector<mpx_order_src> many(MPX_ORDER_MAX_SRC + 1, one[0]);
    FAILS(e, call(many.data(), many.size(), 8, 100, 0, 0), MPX_E_INVAL);
    FAILS(e, call(one, 1, 8, 100, 0, 2), MPX_E_INVAL);
    FAILS(e, call(one, 1, 0, 100, 0, 0), MPX_E_INVAL);
    FAILS(e, call(one, 1, ((size_t)1 << 32) + 1, -2147483647 - 1, 0, 0), MPX_E_INVAL);
    FAILS(e, call(one, 1, 8, 2147483647 - 6, 0, 0), MPX_E_INVAL);
    FAILS(e, call(keyed, 2, 8, 100, 33, 0), MPX_E_INVAL);
    // arrival keys for some sources only, bits without keys, keys without bits, a key too wide
    mpx_order_src mixed[2] = {{r, a, 2}, {r + 2, nullptr, 2}};
    FAILS(e, call(mixed, 2, 8, 100, 2, 0), MPX_E_INVAL);
    FAILS(e, call(one, 1, 8, 100, 2, 0), MPX_E_INVAL);
    FAILS(e, call(keyed, 2, 8, 100, 0, 0), MPX_E_INVAL);
    FAILS(e, call(keyed, 2, 8, 100, 1, 0), MPX_E_INVAL);
    // a record just below and just above the window
    FAILS(e, call(one, 1, 7, 101, 0, 0), MPX_E_NIL_INSTANCE);
    FAILS(e, call(one, 1, 7, 100, 0, 0), MPX_E_NIL_INSTANCE);
    // the size limit
    mpx_order_src huge[2] = {{r, nullptr, 0x80000000ull}, {r, nullptr, 0x7FFFFFFFull}};
    FAILS(e, call(huge, 2, 8, 100, 0, 0), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_order_records_reserve(e, 0xFFFFFFFFull, 8), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_order_records_reserve(e, 8, ((size_t)1 << 32) + 1), MPX_E_INVAL);
    // the device form: the same arguments, and its alignment rules
    FAILS(e, mpx_order_records_dev(e, many.data(), many.size(), 8, 100, 0, 0, out.as<void>(), nullptr, &res, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_order_records_dev(e, mixed, 2, 8, 100, 2, 0, out.as<void>(), nullptr, &res, nullptr), MPX_E_INVAL);
    CHECK(out.untouched() && perm.untouched());  // nothing was touched
    const uint8_t* rb = (const uint8_t*)&res;
    for (size_t i = 0; i < sizeof(res); ++i) CHECK(rb[i] == 0x5C);
    // ... and the smallest window that holds the records is legal: {100, 100, 104, 107}
    CHECK(call(one, 1, 8, 100, 0, 0) == MPX_OK);
    CHECK(res.n == 4 && res.n_runs == 3 && res.lo == 100 && res.hi == 107 && res.flags == 0);
    CHECK(perm.as<uint32_t>()[0] == 1 && perm.as<uint32_t>()[1] == 3 && perm.as<uint32_t>()[2] == 0 &&
          perm.as<uint32_t>()[3] == 2);
    // keys (100,1) (100,0) (104,3) (107,2)
    CHECK(call(keyed, 2, 8, 100, 2, MPX_ORDER_GENERAL) == MPX_OK);
    CHECK(perm.as<uint32_t>()[0] == 3 && perm.as<uint32_t>()[1] == 1 && perm.as<uint32_t>()[2] == 0 &&
          perm.as<uint32_t>()[3] == 2);
    // a source without records may come with null pointers, among keyed ones too
    mpx_order_src holes[3] = {{nullptr, nullptr, 0}, {r, a, 4}, {nullptr, nullptr, 0}};
    CHECK(call(holes, 3, 8, 100, 2, 0) == MPX_OK && res.n == 4);
    CHECK(mpx_order_records(e, nullptr, 0, 8, 100, 0, 0, nullptr, nullptr, &res) == MPX_OK);
    CHECK(res.n == 0 && res.n_runs == 0 && res.lo == 0 && res.hi == -1 &&
          res.flags == MPX_ORD_WAS_ORDERED);
}

int main() {
    mpx_engine* e = open_engine();
    if (!e) return 1;
    validation(e);
    for (const bool with_perm : {true, false}) {
        valid_case(e, {5}, 8, 100, 0, with_perm, false);
        valid_case(e, {0, 7, 0, 9}, 5, -3, 0, with_perm, false);
        valid_case(e, {40, 0, 33}, 16, 0, 6, with_perm, false);
        // ... of a size at which the arrays have slots of more than one 256-byte unit
        valid_case(e, {300, 17, 0, 211}, 97, -40, 0, with_perm, false);
        valid_case(e, {300, 17, 0, 211}, 97, -40, 9, with_perm, false);
        valid_case(e, std::vector<size_t>(MPX_ORDER_MAX_SRC, 21), 1000, 2147483647 - 999, 32, with_perm,
                   false);
        valid_case(e, {}, 8, 0, 0, with_perm, false);
        valid_case(e, {0, 0}, 8, 0, 0, with_perm, false);
    }
    // the device form never allocates: on a fresh handle it needs its reserve call first (a call
    // of no record does not)
    mpx_engine* f = open_engine();
    if (!f) return 1;
    {
        mpx_accept_reply r[2] = {{1, 0, 0, 0, {0, 0, 0}}, {0, 0, 0, 0, {0, 0, 0}}};
        mpx_order_src s[1] = {{r, nullptr, 2}};
        alignas(16) uint8_t out[32];
        mpx_order_result res;
        FAILS(f, mpx_order_records_dev(f, s, 1, 2, 0, 0, 0, out, nullptr, &res, nullptr), MPX_E_INVAL);
        CHECK(strstr(mpx_last_error(f), "mpx_order_records_dev") &&
              strstr(mpx_last_error(f), "mpx_order_records_reserve"));
        CHECK(mpx_order_records_dev(f, s, 0, 2, 0, 0, 0, nullptr, nullptr, &res, nullptr) == MPX_OK);
        CHECK(mpx_order_records_reserve(f, 2, 2) == MPX_OK);
        FAILS(f, mpx_order_records_dev(f, s, 1, 2, 0, 0, 0, out + 4, nullptr, &res, nullptr), MPX_E_INVAL);
        CHECK(mpx_order_records_dev(f, s, 1, 2, 0, 0, 0, out, nullptr, &res, nullptr) == MPX_OK);
        CHECK(res.n == 2 && res.lo == 0 && res.hi == 1);
    }
    valid_case(f, {300, 17, 0, 211}, 97, -40, 9, true, true);
    valid_case(f, {300, 17, 0, 211}, 97, -40, 0, false, true);
    CHECK(mpx_close(f) == MPX_OK);
    CHECK(mpx_close(e) == MPX_OK);
    mpx_order_result res;
    CHECK(mpx_order_records(nullptr, nullptr, 0, 1, 0, 0, 0, nullptr, nullptr, &res) == MPX_E_INVAL);
    CHECK(mpx_order_records_reserve(nullptr, 1, 1) == MPX_E_INVAL);
    CHECK(mpx_order_records_dev(nullptr, nullptr, 0, 1, 0, 0, 0, nullptr, nullptr, &res, nullptr) == MPX_E_INVAL);
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("order_driver: all checks passed\n");
    return failures ? 1 : 0;
}
