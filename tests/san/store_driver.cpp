// tests/san/store_driver.cpp — TEST INFRASTRUCTURE ONLY: drives mpx_store_commands, mpx_store_compact
// and their _reserve / _dev forms of the CPU build of engine.cpp + store.cpp over the stub runtime
// (hip_stub.cpp) and the storing, compacting stand-ins of store_stub.cpp under ASan + UBSan. Every
// argument-validation path of both forms of both calls must answer its code before anything is
// staged or launched; valid calls on guarded buffers must bring back exactly the appended commands,
// the winners' slots, the cursor and the counts through the staging arena, leave the inputs, the
// rest of the arena and of the window and the guard bytes alone. Exit status 0 = all checks passed.
#include <algorithm>

#include "san_check.hpp"

static mpx_engine* open_engine() {
    mpx_engine* e = nullptr;
    mpx_config cfg{5, MPX_MODE_MIN, 1 << 10, 0, 0, 0};
    CHECK(mpx_open(0, &cfg, &e) == MPX_OK && e);
    return e;
}

static bool all_guard(const Out& o, size_t from, size_t to) {
    for (size_t i = from; i < to; ++i)
        if (o.v[i] != kGuardByte) return false;
    return true;
}

// n_src sources of frames with sizes[(s + v) % sizes.size()] commands each; runs of run[r % run.size()]
// messages per instance from instance 100 + 3 r, alternating sources, every third message not
// storing, every fifth a CommitShort; the window is 3 * runs + 2 slots; the arena holds `used`
// commands already and cap_extra more than the call needs (or one less: cap_extra == -1)
static void valid_store(mpx_engine* e, size_t n_src, size_t runs, std::vector<uint32_t> sizes,
                        std::vector<int> run, uint64_t used, long cap_extra, bool sends, bool dev,
                        uint32_t call_flags) {
    const int32_t base = 100;
    const size_t n_inst = 3 * runs + 2;
    struct Src {
        std::vector<uint64_t> off{0};
        std::vector<uint8_t> op;
        std::vector<int64_t> key, val;
        size_t recs = 0;
    };
    std::vector<Src> S(sends ? 1 : n_src);
    std::vector<mpx_accept_msg> msgs;
    std::vector<mpx_accept_send> snd;
    std::vector<uint8_t> eff;
    std::vector<std::pair<size_t, size_t>> rec_of;  // (source, record in it) per item
    struct Want {
        int64_t rel;
        size_t src;
        uint64_t lo, len;
    };
    std::vector<Want> want;  // winners
    uint64_t storing = 0;
    size_t m = 0;
    for (size_t r = 0; r < runs; ++r) {
        const int32_t instance = base + (int32_t)(3 * r);
        bool first = true;
        for (int k = 0; k < run[r % run.size()]; ++k, ++m) {
            const size_t s = sends ? 0 : m % n_src;
            Src& x = S[s];
            const bool keep = !sends && m % 5 == 4, stores = !keep && m % 3 != 2;
            const uint32_t len = keep ? 0 : sizes[(s + m) % sizes.size()];  // a CommitShort carries none
            const uint64_t lo = x.op.size();
            for (uint32_t j = 0; j < len; ++j) {
                x.op.push_back((uint8_t)((lo + j) % 7));
                x.key.push_back((int64_t)(1000 * (s + 1) + lo + j));
                x.val.push_back(-(int64_t)(lo + j) - 1);
            }
            if (sends) {
                snd.push_back(mpx_accept_send{stores ? instance : (m % 2 ? -1 : instance), 3, -1,
                                              stores ? (m % 2 ? MPX_PH_ACCEPT : MPX_PH_PREPARE)
                                                     : (m % 2 ? MPX_PH_NOT_LEADER : MPX_PH_REFUSED),
                                              lo, len, 0});
            } else {
                if (!keep) x.off.push_back(x.op.size());
                msgs.push_back(mpx_accept_msg{instance, 3, 1, keep ? MPX_VALUE_KEEP : (uint32_t)(x.off.size() - 2)});
                eff.push_back(stores ? 3 : (keep && m % 2 ? 2 : 1));
                rec_of.push_back({s, x.recs});
            }
            ++x.recs;
            if (stores) {
                ++storing;
                if (!first) want.pop_back();
                want.push_back(Want{instance - base, s, lo, len});
                first = false;
            }
        }
    }
    const size_t n = m;
    std::vector<uint32_t> perm(n ? n : 1);
    std::vector<size_t> rec_base(S.size() + 1, 0);
    for (size_t s = 0; s < S.size(); ++s) rec_base[s + 1] = rec_base[s] + S[s].recs;
    for (size_t i = 0; i < n && !sends; ++i) perm[i] = (uint32_t)(rec_base[rec_of[i].first] + rec_of[i].second);
    uint64_t total = 0;
    for (const Want& w : want) total += w.len;
    const bool fits = cap_extra >= 0;
    const uint64_t cap = used + total + (fits ? (uint64_t)cap_extra : 0) - (fits ? 0 : 1);
    if (!fits && !total) return;
    // the arena and the window before the call
    Out op(cap), key(cap * 8), val(cap * 8), winst(n_inst * sizeof(mpx_inst_cmds));
    for (size_t i = 0; i < n_inst; ++i) winst.as<mpx_inst_cmds>()[i] = mpx_inst_cmds{i, 1, i % 2 ? 1u : 0u};
    const std::vector<uint8_t> inst0 = winst.v;
    alignas(16) uint64_t cur[2] = {used, 0x5C5C5C5C5C5C5C5Cull};
    alignas(16) mpx_store_result res[2];
    memset(res, 0x5C, sizeof(res));
    std::vector<In> held;
    held.reserve(4 * S.size() + 3);
    std::vector<mpx_store_src> src(S.size());
    for (size_t s = 0; s < S.size(); ++s) {
        Src& x = S[s];
        const size_t k = x.op.size();
        held.push_back(holding(x.off.data(), x.off.size(), 11 + s));
        src[s].cmd_off = sends ? nullptr : held.back().as<uint64_t>();
        src[s].n_frames = sends ? 0 : x.off.size() - 1;
        held.push_back(holding(x.op.data(), k, 12 + s));
        src[s].op = k ? held.back().as<uint8_t>() : nullptr;
        held.push_back(holding(x.key.data(), k, 13 + s));
        src[s].key = k ? held.back().as<int64_t>() : nullptr;
        held.push_back(holding(x.val.data(), k, 14 + s));
        src[s].val = k ? held.back().as<int64_t>() : nullptr;
        src[s].n_cmds = k, src[s].n_recs = x.recs;
    }
    In d_items = sends ? holding(snd.data(), n, 3) : holding(msgs.data(), n, 3);
    In d_eff = holding(eff.data(), sends ? 0 : n, 4), d_perm = holding(perm.data(), sends ? 0 : n, 5);
    mpx_store_batch b{};
    b.kind = sends ? MPX_SC_SENDS : MPX_SC_MSGS, b.flags = call_flags;
    b.items = n ? d_items.as<void>() : nullptr, b.effect = sends || !n ? nullptr : d_eff.as<uint8_t>();
    b.n = n, b.perm = sends || !n ? nullptr : d_perm.as<uint32_t>();
    b.src = src.data(), b.n_src = src.size(), b.n_inst = n_inst, b.inst_base = base, b.store_mask = 2;
    if (!sends && !n && src.size() > 1) b.perm = d_perm.as<uint32_t>();
    mpx_store_arena a{cap ? op.as<uint8_t>() : nullptr, cap ? key.as<int64_t>() : nullptr,
                      cap ? val.as<int64_t>() : nullptr, (size_t)cap, cur};
    if (dev) {
        CHECK(mpx_store_commands_reserve(e, n) == MPX_OK);
        CHECK(mpx_store_commands_dev(e, &b, &a, winst.as<mpx_inst_cmds>(), res, nullptr) == MPX_OK);
        CHECK(mpx_synchronize(e) == MPX_OK);
    } else {
        CHECK(mpx_store_commands(e, &b, &a, winst.as<mpx_inst_cmds>(), res) == MPX_OK);
    }
    CHECK(d_items.intact() && d_eff.intact() && d_perm.intact());
    for (const In& x : held) CHECK(x.intact());
    CHECK(res[0].n_stored == want.size() && res[0].n_cmds == total && res[0].n_superseded == storing - want.size());
    CHECK(res[0].flags == (fits ? 0u : MPX_SC_FULL));
    const uint8_t* after = (const uint8_t*)&res[1];
    for (size_t i = 0; i < sizeof(res[1]); ++i) CHECK(after[i] == 0x5C);
    CHECK(cur[1] == 0x5C5C5C5C5C5C5C5Cull);
    if (!fits) {
        CHECK(cur[0] == used && op.untouched() && key.untouched() && val.untouched() && winst.v == inst0);
        return;
    }
    CHECK(cur[0] == used + total);
    std::vector<uint8_t> inst1 = inst0;
    uint64_t at = used;
    for (const Want& w : want) {
        for (uint64_t j = 0; j < w.len; ++j) {
            CHECK(op.as<uint8_t>()[at + j] == S[w.src].op[w.lo + j]);
            CHECK(key.as<int64_t>()[at + j] == S[w.src].key[w.lo + j]);
            CHECK(val.as<int64_t>()[at + j] == S[w.src].val[w.lo + j]);
        }
        const mpx_inst_cmds x{at, (uint32_t)w.len, MPX_IC_HAS_CMDS};
        memcpy(inst1.data() + w.rel * sizeof(x), &x, sizeof(x));
        at += w.len;
    }
    CHECK(winst.v == inst1);
    CHECK(all_guard(op, 0, used) && all_guard(op, at, op.v.size()));
    CHECK(all_guard(key, 0, used * 8) && all_guard(key, at * 8, key.v.size()));
    CHECK(all_guard(val, 0, used * 8) && all_guard(val, at * 8, val.v.size()));
}

// a window of n_inst slots: slot i has lens[i % lens.size()] commands somewhere in the source
// arena, retired (flag clear) where i % retire == 1
static void valid_compact(mpx_engine* e, size_t n_inst, std::vector<uint32_t> lens, size_t retire,
                          long cap_extra, bool dev) {
    std::vector<mpx_inst_cmds> inst(n_inst ? n_inst : 1);
    uint64_t f_used = 2, total = 0, flagged = 0;
    for (size_t i = 0; i < n_inst; ++i) {
        const uint32_t k = lens[i % lens.size()];
        const bool has = i % retire != 1;
        inst[i] = mpx_inst_cmds{f_used, k, has ? MPX_IC_HAS_CMDS : 0u};
        f_used += k + (i % 4 == 0);
        if (has) total += k, ++flagged;
    }
    const size_t f_cap = f_used + 3;
    std::vector<uint8_t> fop(f_cap);
    std::vector<int64_t> fkey(f_cap), fval(f_cap);
    for (size_t j = 0; j < f_cap; ++j) fop[j] = j % 7, fkey[j] = 5000 + (int64_t)j, fval[j] = -(int64_t)j - 1;
    const bool fits = cap_extra >= 0;
    if (!fits && !total) return;
    const uint64_t cap = fits ? total + cap_extra : total - 1;
    In d_fop = holding(fop.data(), f_cap, 3), d_fkey = holding(fkey.data(), f_cap, 4), d_fval = holding(fval.data(), f_cap, 5);
    Out op(cap), key(cap * 8), val(cap * 8), winst(n_inst * sizeof(mpx_inst_cmds));
    if (n_inst) memcpy(winst.v.data(), inst.data(), n_inst * sizeof(mpx_inst_cmds));
    const std::vector<uint8_t> inst0 = winst.v;
    alignas(16) uint64_t fcur[2] = {f_used, 7}, tcur[2] = {0x1234, 0x5C5C5C5C5C5C5C5Cull};
    alignas(16) mpx_store_result res[2];
    memset(res, 0x5C, sizeof(res));
    const mpx_store_arena from{d_fop.as<uint8_t>(), d_fkey.as<int64_t>(), d_fval.as<int64_t>(), f_cap, fcur};
    const mpx_store_arena to{cap ? op.as<uint8_t>() : nullptr, cap ? key.as<int64_t>() : nullptr,
                             cap ? val.as<int64_t>() : nullptr, (size_t)cap, tcur};
    mpx_inst_cmds* w = n_inst ? winst.as<mpx_inst_cmds>() : nullptr;
    if (dev) {
        CHECK(mpx_store_compact_reserve(e, n_inst) == MPX_OK);
        CHECK(mpx_store_compact_dev(e, w, n_inst, &from, &to, res, nullptr) == MPX_OK);
        CHECK(mpx_synchronize(e) == MPX_OK);
    } else {
        CHECK(mpx_store_compact(e, w, n_inst, &from, &to, res) == MPX_OK);
    }
    CHECK(d_fop.intact() && d_fkey.intact() && d_fval.intact() && fcur[0] == f_used && fcur[1] == 7);
    CHECK(res[0].n_stored == flagged && res[0].n_cmds == total && res[0].n_superseded == 0);
    CHECK(res[0].flags == (fits ? 0u : MPX_SC_FULL) && tcur[1] == 0x5C5C5C5C5C5C5C5Cull);
    const uint8_t* after = (const uint8_t*)&res[1];
    for (size_t i = 0; i < sizeof(res[1]); ++i) CHECK(after[i] == 0x5C);
    if (!fits) {
        CHECK(tcur[0] == 0x1234 && op.untouched() && key.untouched() && val.untouched() && winst.v == inst0);
        return;
    }
    CHECK(tcur[0] == total);
    uint64_t at = 0;
    for (size_t i = 0; i < n_inst; ++i) {
        const mpx_inst_cmds got = winst.as<mpx_inst_cmds>()[i];
        if (!(inst[i].flags & MPX_IC_HAS_CMDS)) {
            CHECK(memcmp(&got, &inst[i], sizeof(got)) == 0);
            continue;
        }
        CHECK(got.first_cmd == at && got.n_cmds == inst[i].n_cmds && got.flags == MPX_IC_HAS_CMDS);
        for (uint32_t j = 0; j < inst[i].n_cmds; ++j) {
            CHECK(op.as<uint8_t>()[at + j] == fop[inst[i].first_cmd + j]);
            CHECK(key.as<int64_t>()[at + j] == fkey[inst[i].first_cmd + j]);
            CHECK(val.as<int64_t>()[at + j] == fval[inst[i].first_cmd + j]);
        }
        at += inst[i].n_cmds;
    }
    CHECK(all_guard(op, at, op.v.size()) && all_guard(key, at * 8, key.v.size()) && all_guard(val, at * 8, val.v.size()));
    CHECK(all_guard(winst, n_inst * sizeof(mpx_inst_cmds), winst.v.size()));
}

#define SHIFTED(T, p, by) ((T*)((char*)(p) + (by)))

static void validation_store(mpx_engine* e) {
    // a window of 4 slots from instance 10; two sources of two frames
    alignas(16) mpx_accept_msg msgs[3] = {{10, 1, 0, 0}, {11, 1, 0, 0}, {12, 1, 0, 1}};
    alignas(16) mpx_accept_send sends[2] = {{10, 1, -1, MPX_PH_ACCEPT, 0, 2, 0}, {11, 1, -1, MPX_PH_PREPARE, 2, 1, 0}};
    alignas(16) uint8_t eff[3] = {2, 2, 2};
    alignas(16) uint32_t perm[3] = {2, 0, 3};
    alignas(16) uint64_t off0[3] = {0, 1, 3}, off1[3] = {0, 3, 4};
    alignas(16) uint8_t op0[3] = {1, 2, 1}, op1[4] = {2, 1, 2, 1};
    alignas(16) int64_t key0[3] = {1, 2, 3}, val0[3] = {4, 5, 6}, key1[4] = {7, 8, 9, 10}, val1[4] = {1, 1, 1, 1};
    mpx_store_src src[2] = {{off0, 2, op0, key0, val0, 3, 2}, {off1, 2, op1, key1, val1, 4, 2}};
    Out op(8), key(64), val(64), winst(64);
    memset(winst.v.data(), 0, 64);
    alignas(16) uint64_t cur[2] = {0, 0};
    alignas(16) mpx_store_result res;
    memset(&res, 0x5C, sizeof(res));
    CHECK(mpx_store_commands_reserve(e, 8) == MPX_OK);
    mpx_store_batch ok{};
    ok.kind = MPX_SC_MSGS, ok.items = msgs, ok.effect = eff, ok.n = 3, ok.perm = perm, ok.src = src, ok.n_src = 2;
    ok.n_inst = 4, ok.inst_base = 10, ok.store_mask = 2;
    mpx_store_arena oa{op.as<uint8_t>(), key.as<int64_t>(), val.as<int64_t>(), 8, cur};
    mpx_inst_cmds* inst = winst.as<mpx_inst_cmds>();
    auto both = [&](const mpx_store_batch* b, const mpx_store_arena* a, mpx_inst_cmds* w, mpx_store_result* rs, int code) {
        FAILS(e, mpx_store_commands(e, b, a, w, rs), code);
        FAILS(e, mpx_store_commands_dev(e, b, a, w, rs, nullptr), code);
    };
    // null arguments
    both(nullptr, &oa, inst, &res, MPX_E_INVAL);
    both(&ok, nullptr, inst, &res, MPX_E_INVAL);
    both(&ok, &oa, nullptr, &res, MPX_E_INVAL);
    both(&ok, &oa, inst, nullptr, MPX_E_INVAL);
    mpx_store_batch x = ok;
    mpx_store_arena y = oa;
    x.items = nullptr;
    both(&x, &oa, inst, &res, MPX_E_INVAL);
    x = ok, x.effect = nullptr;
    both(&x, &oa, inst, &res, MPX_E_INVAL);
    x = ok, x.src = nullptr;
    both(&x, &oa, inst, &res, MPX_E_INVAL);
    y = oa, y.op = nullptr;
    both(&ok, &y, inst, &res, MPX_E_INVAL);
    y = oa, y.key = nullptr;
    both(&ok, &y, inst, &res, MPX_E_INVAL);
    y = oa, y.val = nullptr;
    both(&ok, &y, inst, &res, MPX_E_INVAL);
    y = oa, y.used = nullptr;
    both(&ok, &y, inst, &res, MPX_E_INVAL);
    for (int f = 0; f < 4; ++f) {
        mpx_store_src s2[2] = {src[0], src[1]};
        if (f == 0) s2[1].cmd_off = nullptr;
        if (f == 1) s2[1].op = nullptr;
        if (f == 2) s2[0].key = nullptr;
        if (f == 3) s2[0].val = nullptr;
        x = ok, x.src = s2;
        both(&x, &oa, inst, &res, MPX_E_INVAL);
    }
    // kind, flags, reserved, the sources' count, perm, the records' count
    x = ok, x.kind = 2;
    both(&x, &oa, inst, &res, MPX_E_INVAL);
    x = ok, x.flags = 2;
    both(&x, &oa, inst, &res, MPX_E_INVAL);
    x = ok, x.reserved = 1;
    both(&x, &oa, inst, &res, MPX_E_INVAL);
    x = ok, x.n_src = 0;
    both(&x, &oa, inst, &res, MPX_E_INVAL);
    x = ok, x.n_src = 17;
    both(&x, &oa, inst, &res, MPX_E_INVAL);
    x = ok, x.perm = nullptr;
    both(&x, &oa, inst, &res, MPX_E_INVAL);
    x = ok, x.n = 5;
    both(&x, &oa, inst, &res, MPX_E_INVAL);
    x = ok, x.kind = MPX_SC_SENDS, x.items = sends, x.n = 2;  // sends take one source
    both(&x, &oa, inst, &res, MPX_E_INVAL);
    x = ok, x.n = (size_t)0xFFFFFFFFull;
    both(&x, &oa, inst, &res, MPX_E_UNSUPPORTED);
    FAILS(e, mpx_store_commands_reserve(e, (size_t)0xFFFFFFFFull), MPX_E_UNSUPPORTED);
    // the host form: d_n, the cursor, the items
    x = ok, x.d_n = cur;
    FAILS(e, mpx_store_commands(e, &x, &oa, inst, &res), MPX_E_INVAL);
    cur[0] = 9;
    FAILS(e, mpx_store_commands(e, &ok, &oa, inst, &res), MPX_E_INVAL);
    cur[0] = 0;
    perm[1] = 4;
    FAILS(e, mpx_store_commands(e, &ok, &oa, inst, &res), MPX_E_INVAL);
    perm[1] = 0;
    msgs[1].value_id = 2;
    FAILS(e, mpx_store_commands(e, &ok, &oa, inst, &res), MPX_E_INVAL);
    msgs[1].value_id = 0;
    off0[1] = 4;  // [0, 4) leaves the 3 commands; and [4, 3) decreases
    FAILS(e, mpx_store_commands(e, &ok, &oa, inst, &res), MPX_E_INVAL);
    msgs[1].value_id = 1;
    FAILS(e, mpx_store_commands(e, &ok, &oa, inst, &res), MPX_E_INVAL);
    msgs[1].value_id = 0, off0[1] = 1;
    for (const int32_t bad : {9, 14}) {
        msgs[2].instance = bad;
        FAILS(e, mpx_store_commands(e, &ok, &oa, inst, &res), MPX_E_NIL_INSTANCE);
    }
    eff[2] = 1;  // ... not judged when it does not store
    CHECK(mpx_store_commands(e, &ok, &oa, inst, &res) == MPX_OK && res.n_stored == 2 && res.n_cmds == 4 && cur[0] == 4);
    CHECK(inst[0].first_cmd == 0 && inst[0].n_cmds == 3 && inst[1].first_cmd == 3 && inst[1].n_cmds == 1);
    CHECK(key.as<int64_t>()[0] == 7 && key.as<int64_t>()[3] == 1 && all_guard(key, 32, key.v.size()));
    eff[2] = 2, msgs[2].instance = 12, cur[0] = 0;
    src[0].n_cmds = (size_t)1 << 40, src[1].n_cmds = (size_t)1 << 40;  // 2^32 commands in all
    off0[1] = 0x80000000ull, off0[2] = off0[1], off1[1] = 0x80000000ull, off1[2] = 0x100000000ull;
    msgs[2].value_id = 0;
    FAILS(e, mpx_store_commands(e, &ok, &oa, inst, &res), MPX_E_UNSUPPORTED);
    src[0].n_cmds = 3, src[1].n_cmds = 4, off0[1] = 1, off0[2] = 3, off1[1] = 3, off1[2] = 4, msgs[2].value_id = 1;
    x = ok, x.kind = MPX_SC_SENDS, x.items = sends, x.n = 2, x.n_src = 1, x.effect = nullptr, x.perm = nullptr;
    sends[1].n_cmds = 2;
    FAILS(e, mpx_store_commands(e, &x, &oa, inst, &res), MPX_E_INVAL);
    sends[1].n_cmds = 1, sends[0].instance = 9;
    FAILS(e, mpx_store_commands(e, &x, &oa, inst, &res), MPX_E_NIL_INSTANCE);
    sends[0].instance = 10;
    for (Out* z : {&op, &key, &val}) memset(z->v.data(), kGuardByte, z->v.size());
    memset(winst.v.data(), kGuardByte, winst.v.size());
    memset(&res, 0x5C, sizeof(res));
    // the device form's alignment rules
    auto dev = [&](const mpx_store_batch& b, const mpx_store_arena& a, mpx_inst_cmds* w, mpx_store_result* rs) {
        return mpx_store_commands_dev(e, &b, &a, w, rs, nullptr);
    };
    x = ok, x.items = SHIFTED(const void, msgs, 8);
    FAILS(e, dev(x, oa, inst, &res), MPX_E_INVAL);
    x = ok, x.perm = SHIFTED(const uint32_t, perm, 2);
    FAILS(e, dev(x, oa, inst, &res), MPX_E_INVAL);
    x = ok, x.d_n = SHIFTED(const uint64_t, cur, 4);
    FAILS(e, dev(x, oa, inst, &res), MPX_E_INVAL);
    for (int f = 0; f < 3; ++f) {
        mpx_store_src s2[2] = {src[0], src[1]};
        if (f == 0) s2[1].cmd_off = SHIFTED(const uint64_t, off1, 4);
        if (f == 1) s2[0].key = SHIFTED(const int64_t, key0, 4);
        if (f == 2) s2[1].val = SHIFTED(const int64_t, val1, 4);
        x = ok, x.src = s2;
        FAILS(e, dev(x, oa, inst, &res), MPX_E_INVAL);
    }
    y = oa, y.key = SHIFTED(int64_t, oa.key, 4);
    FAILS(e, dev(ok, y, inst, &res), MPX_E_INVAL);
    y = oa, y.val = SHIFTED(int64_t, oa.val, 4);
    FAILS(e, dev(ok, y, inst, &res), MPX_E_INVAL);
    y = oa, y.used = SHIFTED(uint64_t, cur, 4);
    FAILS(e, dev(ok, y, inst, &res), MPX_E_INVAL);
    FAILS(e, dev(ok, oa, SHIFTED(mpx_inst_cmds, inst, 8), &res), MPX_E_INVAL);
    FAILS(e, dev(ok, oa, inst, SHIFTED(mpx_store_result, &res, 4)), MPX_E_INVAL);
    // nothing was touched
    CHECK(op.untouched() && key.untouched() && val.untouched() && winst.untouched() && cur[0] == 0);
    const uint8_t* rb = (const uint8_t*)&res;
    for (size_t i = 0; i < sizeof(res); ++i) CHECK(rb[i] == 0x5C);
    // the device form reports a faulty item through the error word: it neither stores nor supersedes
    msgs[1].value_id = 2;
    CHECK(dev(ok, oa, inst, &res) == MPX_OK);
    FAILS(e, mpx_synchronize(e), MPX_E_INVAL);
    CHECK(res.n_stored == 2 && res.n_cmds == 4 && cur[0] == 4 && inst[0].n_cmds == 3 && inst[2].first_cmd == 3);
    CHECK(all_guard(winst, 16, 32));
    msgs[1].value_id = 0, msgs[2].instance = 14, cur[0] = 1;
    CHECK(dev(ok, oa, inst, &res) == MPX_OK);
    FAILS(e, mpx_synchronize(e), MPX_E_NIL_INSTANCE);
    CHECK(res.n_stored == 2 && res.n_cmds == 4 && cur[0] == 5 && inst[1].first_cmd == 4 && inst[1].n_cmds == 1);
    msgs[2].instance = 12, cur[0] = 9;  // a cursor past the capacity: nothing is written
    CHECK(dev(ok, oa, inst, &res) == MPX_OK);
    FAILS(e, mpx_synchronize(e), MPX_E_INVAL);
    CHECK(res.flags == MPX_SC_FULL && cur[0] == 9);
    cur[0] = 0;
    // d_n cuts the batch; op bytes and effect may sit at any address
    alignas(16) uint64_t dn[2] = {1, 0};
    alignas(16) uint8_t eff2[4] = {0, 2, 2, 2};
    x = ok, x.d_n = dn, x.effect = eff2 + 1;
    y = oa, y.op = oa.op + 1, y.cap = 7;
    CHECK(dev(x, y, inst, &res) == MPX_OK && mpx_synchronize(e) == MPX_OK && res.n_stored == 1 && res.n_cmds == 3 && cur[0] == 3);
    cur[0] = 0;
    // no item: legal with null arrays, the result is written
    mpx_store_batch none{};
    none.src = src, none.n_src = 1;
    mpx_store_arena na{nullptr, nullptr, nullptr, 0, cur};
    CHECK(mpx_store_commands(e, &none, &na, nullptr, &res) == MPX_OK && res.n_stored == 0 && res.n_cmds == 0 && res.flags == 0);
    none.flags = MPX_SC_GENERAL;
    CHECK(mpx_store_commands(e, &none, &na, nullptr, &res) == MPX_OK && res.n_cmds == 0 && cur[0] == 0);
}

static void validation_compact(mpx_engine* e) {
    alignas(16) mpx_inst_cmds inst[3] = {{1, 2, 1}, {0, 1, 0}, {3, 1, 1}};
    alignas(16) uint8_t fop[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    alignas(16) int64_t fkey[8] = {1, 2, 3, 4, 5, 6, 7, 8}, fval[8] = {8, 7, 6, 5, 4, 3, 2, 1};
    alignas(16) uint64_t fcur[2] = {4, 0}, tcur[2] = {77, 0};
    Out op(4), key(32), val(32);
    alignas(16) mpx_store_result res;
    memset(&res, 0x5C, sizeof(res));
    CHECK(mpx_store_compact_reserve(e, 8) == MPX_OK);
    const mpx_store_arena from{fop, fkey, fval, 8, fcur};
    const mpx_store_arena to{op.as<uint8_t>(), key.as<int64_t>(), val.as<int64_t>(), 4, tcur};
    auto both = [&](mpx_inst_cmds* w, size_t n, const mpx_store_arena* f, const mpx_store_arena* t,
                    mpx_store_result* rs, int code) {
        FAILS(e, mpx_store_compact(e, w, n, f, t, rs), code);
        FAILS(e, mpx_store_compact_dev(e, w, n, f, t, rs, nullptr), code);
    };
    both(nullptr, 3, &from, &to, &res, MPX_E_INVAL);
    both(inst, 3, nullptr, &to, &res, MPX_E_INVAL);
    both(inst, 3, &from, nullptr, &res, MPX_E_INVAL);
    both(inst, 3, &from, &to, nullptr, MPX_E_INVAL);
    mpx_store_arena y = from;
    y.op = nullptr;
    both(inst, 3, &y, &to, &res, MPX_E_INVAL);
    y = from, y.used = nullptr;
    both(inst, 3, &y, &to, &res, MPX_E_INVAL);
    y = to, y.key = nullptr;
    both(inst, 3, &from, &y, &res, MPX_E_INVAL);
    y = to, y.val = nullptr;
    both(inst, 3, &from, &y, &res, MPX_E_INVAL);
    y = to, y.used = nullptr;
    both(inst, 3, &from, &y, &res, MPX_E_INVAL);
    both(inst, (size_t)0xFFFFFFFFull, &from, &to, &res, MPX_E_UNSUPPORTED);
    FAILS(e, mpx_store_compact_reserve(e, (size_t)0xFFFFFFFFull), MPX_E_UNSUPPORTED);
    // from and to overlap: one array inside the other's range, or one cursor for both
    y = to, y.op = fop + 7;
    both(inst, 3, &from, &y, &res, MPX_E_INVAL);
    y = to, y.key = fkey + 2;
    both(inst, 3, &from, &y, &res, MPX_E_INVAL);
    y = to, y.val = fval;
    both(inst, 3, &from, &y, &res, MPX_E_INVAL);
    y = to, y.used = fcur;
    both(inst, 3, &from, &y, &res, MPX_E_INVAL);
    both(inst, 3, &from, &from, &res, MPX_E_INVAL);
    // the host form: the source's cursor, a flagged slot's range
    fcur[0] = 9;
    FAILS(e, mpx_store_compact(e, inst, 3, &from, &to, &res), MPX_E_INVAL);
    fcur[0] = 4, inst[2].n_cmds = 2;  // [3, 5) leaves [0, 4)
    FAILS(e, mpx_store_compact(e, inst, 3, &from, &to, &res), MPX_E_INVAL);
    inst[2] = mpx_inst_cmds{5, 0, 1};
    FAILS(e, mpx_store_compact(e, inst, 3, &from, &to, &res), MPX_E_INVAL);
    inst[2] = mpx_inst_cmds{3, 1, 1};
    inst[1] = mpx_inst_cmds{900, 900, 0};  // ... not judged without the flag
    // the device form's alignment rules
    FAILS(e, mpx_store_compact_dev(e, SHIFTED(mpx_inst_cmds, inst, 8), 2, &from, &to, &res, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_store_compact_dev(e, inst, 3, &from, &to, SHIFTED(mpx_store_result, &res, 4), nullptr), MPX_E_INVAL);
    y = from, y.key = SHIFTED(int64_t, fkey, 4);
    FAILS(e, mpx_store_compact_dev(e, inst, 3, &y, &to, &res, nullptr), MPX_E_INVAL);
    y = to, y.val = SHIFTED(int64_t, to.val, 4);
    FAILS(e, mpx_store_compact_dev(e, inst, 3, &from, &y, &res, nullptr), MPX_E_INVAL);
    y = to, y.used = SHIFTED(uint64_t, tcur, 4);
    FAILS(e, mpx_store_compact_dev(e, inst, 3, &from, &y, &res, nullptr), MPX_E_INVAL);
    CHECK(op.untouched() && key.untouched() && val.untouched() && tcur[0] == 77);
    const uint8_t* rb = (const uint8_t*)&res;
    for (size_t i = 0; i < sizeof(res); ++i) CHECK(rb[i] == 0x5C);
    // the device form reports a faulty slot through the error word: it contributes no commands
    inst[0].n_cmds = 4;
    CHECK(mpx_store_compact_dev(e, inst, 3, &from, &to, &res, nullptr) == MPX_OK);
    FAILS(e, mpx_synchronize(e), MPX_E_INVAL);
    CHECK(res.n_stored == 2 && res.n_cmds == 1 && tcur[0] == 1 && inst[0].n_cmds == 0 && inst[2].first_cmd == 0);
    CHECK(inst[1].first_cmd == 900 && key.as<int64_t>()[0] == 4 && all_guard(key, 8, key.v.size()));
    // op bytes may sit at any address; an empty window writes the result and the cursor
    inst[0] = mpx_inst_cmds{1, 2, 1}, inst[2] = mpx_inst_cmds{3, 1, 1};
    y = to, y.op = to.op + 1, y.cap = 3;
    CHECK(mpx_store_compact_dev(e, inst, 3, &from, &y, &res, nullptr) == MPX_OK && mpx_synchronize(e) == MPX_OK);
    CHECK(res.n_cmds == 3 && tcur[0] == 3 && op.as<uint8_t>()[1] == 2 && op.as<uint8_t>()[3] == 4);
    CHECK(mpx_store_compact(e, nullptr, 0, &from, &to, &res) == MPX_OK && res.n_stored == 0 && tcur[0] == 0);
}

int main() {
    mpx_engine* e = open_engine();
    if (!e) return 1;
    validation_store(e);
    validation_compact(e);
    for (const bool dev : {false, true})
        for (const uint32_t call_flags : {0u, MPX_SC_GENERAL})
            for (const long cap_extra : {0L, 5L, -1L}) {
                valid_store(e, 1, 1, {2}, {1}, 0, cap_extra, false, dev, call_flags);
                valid_store(e, 3, 9, {2, 0, 1, 5, 3}, {1, 3, 2, 4}, 3, cap_extra, false, dev, call_flags);
                // ... of a size at which the arrays have slots of more than one 256-byte unit
                valid_store(e, 4, 150, {300, 17, 0, 2, 1}, {1, 2, 5}, 7, cap_extra, false, dev, call_flags);
                valid_store(e, 1, 40, {3, 0, 40, 1}, {1, 3, 2}, 2, cap_extra, true, dev, call_flags);
                valid_store(e, 2, 0, {1}, {1}, 4, cap_extra, false, dev, call_flags);
            }
    for (const bool dev : {false, true})
        for (const long cap_extra : {0L, 9L, -1L}) {
            valid_compact(e, 1, {3}, 5, cap_extra, dev);
            valid_compact(e, 9, {2, 0, 5, 1}, 3, cap_extra, dev);
            valid_compact(e, 700, {1, 17, 0, 2}, 4, cap_extra, dev);
            valid_compact(e, 0, {1}, 2, cap_extra, dev);
        }
    // the device forms never allocate: on a fresh handle they need their reserve call first
    mpx_engine* f = open_engine();
    if (!f) return 1;
    {
        alignas(16) mpx_accept_msg msgs[1] = {{0, 1, 0, 0}};
        alignas(16) uint8_t eff[1] = {2}, sop[2] = {1, 2}, op[4];
        alignas(16) uint64_t off[2] = {0, 2}, cur[2] = {1, 0}, tcur[2] = {0, 0};
        alignas(16) int64_t skey[2] = {5, 6}, sval[2] = {7, 8}, key[4], val[4], tkey[4], tval[4];
        alignas(16) uint8_t top[4];
        alignas(16) mpx_inst_cmds inst[1] = {{0, 0, 0}};
        alignas(16) mpx_store_result res;
        const mpx_store_src src{off, 1, sop, skey, sval, 2, 1};
        mpx_store_batch b{};
        b.items = msgs, b.effect = eff, b.n = 1, b.src = &src, b.n_src = 1, b.n_inst = 1, b.store_mask = 2;
        const mpx_store_arena a{op, key, val, 4, cur}, t{top, tkey, tval, 4, tcur};
        FAILS(f, mpx_store_commands_dev(f, &b, &a, inst, &res, nullptr), MPX_E_INVAL);
        CHECK(strstr(mpx_last_error(f), "mpx_store_commands_dev") && strstr(mpx_last_error(f), "mpx_store_commands_reserve"));
        FAILS(f, mpx_store_compact_dev(f, inst, 1, &a, &t, &res, nullptr), MPX_E_INVAL);
        CHECK(strstr(mpx_last_error(f), "mpx_store_compact_dev") && strstr(mpx_last_error(f), "mpx_store_compact_reserve"));
        CHECK(mpx_store_commands_reserve(f, 1) == MPX_OK);
        CHECK(mpx_store_commands_dev(f, &b, &a, inst, &res, nullptr) == MPX_OK && mpx_synchronize(f) == MPX_OK);
        CHECK(res.n_cmds == 2 && cur[0] == 3 && inst[0].first_cmd == 1 && key[2] == 6);
        CHECK(mpx_store_compact_dev(f, inst, 1, &a, &t, &res, nullptr) == MPX_OK && mpx_synchronize(f) == MPX_OK);
        CHECK(res.n_cmds == 2 && tcur[0] == 2 && inst[0].first_cmd == 0 && tkey[1] == 6);
        // more items than were reserved for: refused before the items are looked at
        mpx_store_src many = src;
        many.n_recs = 5000;
        b.n = 5000, b.src = &many;
        FAILS(f, mpx_store_commands_dev(f, &b, &a, inst, &res, nullptr), MPX_E_INVAL);
        FAILS(f, mpx_store_compact_dev(f, inst, 5000, &a, &t, &res, nullptr), MPX_E_INVAL);
        CHECK(mpx_store_compact_reserve(f, 5000) == MPX_OK);  // (one scratch for both calls)
        b.n = 1, b.src = &src, b.flags = MPX_SC_GENERAL, cur[0] = 0;
        CHECK(mpx_store_commands_dev(f, &b, &a, inst, &res, nullptr) == MPX_OK && mpx_synchronize(f) == MPX_OK);
        CHECK(res.n_cmds == 2 && cur[0] == 2 && inst[0].first_cmd == 0 && key[1] == 6);
    }
    CHECK(mpx_close(f) == MPX_OK);
    CHECK(mpx_close(e) == MPX_OK);
    mpx_store_result res;
    mpx_store_batch none{};
    mpx_store_arena na{};
    CHECK(mpx_store_commands(nullptr, &none, &na, nullptr, &res) == MPX_E_INVAL);
    CHECK(mpx_store_commands_reserve(nullptr, 1) == MPX_E_INVAL);
    CHECK(mpx_store_commands_dev(nullptr, &none, &na, nullptr, &res, nullptr) == MPX_E_INVAL);
    CHECK(mpx_store_compact(nullptr, nullptr, 0, &na, &na, &res) == MPX_E_INVAL);
    CHECK(mpx_store_compact_reserve(nullptr, 1) == MPX_E_INVAL);
    CHECK(mpx_store_compact_dev(nullptr, nullptr, 0, &na, &na, &res, nullptr) == MPX_E_INVAL);
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("store_driver: all checks passed\n");
    return failures ? 1 : 0;
}
