// tests/san/record_driver.cpp — TEST INFRASTRUCTURE ONLY: drives mpx_record_log and its _reserve /
// _dev forms of the CPU build of engine.cpp + record.cpp over the stub runtime (hip_stub.cpp) and the
// encoding stand-in of record_stub.cpp under ASan + UBSan. Every argument-validation path of both
// forms must answer its code before anything is staged or launched; valid calls on guarded buffers
// must bring back exactly the run's bytes, item_off and res through the staging arena and leave the
// inputs and the guard bytes alone. Exit status 0 = all checks passed.
#include <algorithm>

#include "san_check.hpp"

static mpx_engine* open_engine() {
    mpx_engine* e = nullptr;
    mpx_config cfg{5, MPX_MODE_MIN, 1 << 10, 0, 0, 0};
    CHECK(mpx_open(0, &cfg, &e) == MPX_OK && e);
    return e;
}

static void put(std::vector<uint8_t>& w, uint64_t x, int bytes) {
    for (int k = 0; k < bytes; ++k) w.push_back((uint8_t)(x >> (8 * k)));
}

// n items over n_src sources: item m has sizes[m % sizes.size()] commands; every third does not
// record (COMMITS: is a CommitShort); DECIDED: every fifth accepted slot is masked out, in a window
// of 3 n + 2 slots. cap_extra: what out holds beyond the run (-1: one byte less)
static void valid(mpx_engine* e, uint32_t kind, uint32_t format, size_t n_src, size_t n,
                  std::vector<uint32_t> sizes, long cap_extra, bool dev, uint32_t call_flags, bool want_off) {
    const bool msgs = kind <= MPX_LR_COMMITS;
    const int32_t base = 100;
    const size_t n_inst = 3 * n + 2;
    struct Src {
        std::vector<uint64_t> off{0};
        std::vector<uint8_t> op;
        std::vector<int64_t> key, val;
        size_t recs = 0;
    };
    std::vector<Src> S(msgs ? n_src : 1);
    std::vector<mpx_accept_msg> m16;
    std::vector<mpx_accept_send> m32;
    std::vector<uint8_t> eff, mask(n_inst, 0), want;
    std::vector<uint64_t> want_item(n + 1, 0);
    std::vector<std::pair<size_t, size_t>> rec_of;
    const uint32_t status = kind == MPX_LR_ACCEPTS ? 2 : kind == MPX_LR_SENDS ? 1 : 3;
    uint64_t n_recs = 0, n_cmds = 0;
    for (size_t m = 0; m < n; ++m) {
        want_item[m] = want.size();
        const size_t s = msgs ? m % n_src : 0;
        Src& x = S[s];
        const bool third = m % 3 == 2;
        const int32_t instance = base + (int32_t)(3 * m / 2), ballot = (int32_t)(m * 7 - 3);
        const bool with = kind == MPX_LR_DECIDED ? false : !third;
        const uint32_t len = with ? sizes[m % sizes.size()] : 0;
        const uint64_t lo = x.op.size();
        for (uint32_t j = 0; j < len; ++j) {
            x.op.push_back((uint8_t)((lo + j) % 7));
            x.key.push_back((int64_t)(1000 * (s + 1) + lo + j));
            x.val.push_back(-(int64_t)(lo + j) - 1);
        }
        bool records;
        if (msgs) {
            const bool shortc = kind == MPX_LR_COMMITS && third;
            if (!shortc) x.off.push_back(x.op.size());
            m16.push_back(mpx_accept_msg{instance, ballot, 1, shortc ? MPX_VALUE_KEEP : (uint32_t)(x.off.size() - 2)});
            eff.push_back(kind == MPX_LR_ACCEPTS ? (third ? 1 : 3) : (third ? 1 : 2));
            rec_of.push_back({s, x.recs});
            records = kind == MPX_LR_COMMITS || !third;
        } else {
            const uint32_t fl = !third ? MPX_PH_ACCEPT : m % 2 ? MPX_PH_PREPARE : MPX_PH_REFUSED;
            m32.push_back(mpx_accept_send{instance, ballot, -1, fl, lo, len, 0});
            records = !third;
            if (kind == MPX_LR_DECIDED && records) {
                mask[instance - base] = m % 5 != 0;
                records = m % 5 != 0;
            }
        }
        ++x.recs;
        if (!records) continue;
        put(want, (uint32_t)ballot, 4);
        if (format == MPX_LOG_DURABLE) put(want, status, 4), put(want, (uint32_t)instance, 4);
        else put(want, status, 1);
        for (uint32_t j = 0; j < len; ++j)
            put(want, x.op[lo + j], 1), put(want, (uint64_t)x.key[lo + j], 8), put(want, (uint64_t)x.val[lo + j], 8);
        ++n_recs, n_cmds += len;
    }
    want_item[n] = want.size();
    const bool fits = cap_extra >= 0;
    if (!fits && want.empty()) return;
    const size_t cap = fits ? want.size() + cap_extra : want.size() - 1;
    std::vector<uint32_t> perm(n ? n : 1);
    std::vector<size_t> rec_base(S.size() + 1, 0);
    for (size_t s = 0; s < S.size(); ++s) rec_base[s + 1] = rec_base[s] + S[s].recs;
    for (size_t i = 0; i < n && msgs; ++i) perm[i] = (uint32_t)(rec_base[rec_of[i].first] + rec_of[i].second);
    std::vector<In> held;
    held.reserve(4 * S.size());
    std::vector<mpx_store_src> src(S.size());
    for (size_t s = 0; s < S.size(); ++s) {
        Src& x = S[s];
        const size_t k = x.op.size();
        held.push_back(holding(x.off.data(), x.off.size(), 11 + s));
        src[s].cmd_off = msgs ? held.back().as<uint64_t>() : nullptr;
        src[s].n_frames = msgs ? x.off.size() - 1 : 0;
        held.push_back(holding(x.op.data(), k, 12 + s));
        src[s].op = k ? held.back().as<uint8_t>() : nullptr;
        held.push_back(holding(x.key.data(), k, 13 + s));
        src[s].key = k ? held.back().as<int64_t>() : nullptr;
        held.push_back(holding(x.val.data(), k, 14 + s));
        src[s].val = k ? held.back().as<int64_t>() : nullptr;
        src[s].n_cmds = k, src[s].n_recs = x.recs;
    }
    In d_items = msgs ? holding(m16.data(), n, 3) : holding(m32.data(), n, 3);
    In d_eff = holding(eff.data(), msgs ? n : 0, 4), d_perm = holding(perm.data(), msgs ? n : 0, 5);
    In d_mask = holding(mask.data(), n_inst, 6);
    Out out(cap), ioff((n + 1) * 8);
    alignas(16) mpx_record_result res[2];
    memset(res, 0x5C, sizeof(res));
    mpx_record_batch b{};
    b.kind = kind, b.flags = call_flags, b.format = format;
    b.items = n ? d_items.as<void>() : nullptr, b.effect = msgs && n ? d_eff.as<uint8_t>() : nullptr;
    b.n = n, b.perm = msgs && (n || n_src > 1) ? d_perm.as<uint32_t>() : nullptr;
    if (kind == MPX_LR_DECIDED) b.mask = d_mask.as<uint8_t>(), b.n_inst = n_inst, b.inst_base = base;
    else b.src = src.data(), b.n_src = src.size();
    uint8_t* const o = cap ? out.as<uint8_t>() : nullptr;
    uint64_t* const io = want_off ? ioff.as<uint64_t>() : nullptr;
    if (dev) {
        CHECK(mpx_record_log_reserve(e, n) == MPX_OK);
        CHECK(mpx_record_log_dev(e, &b, o, cap, io, res, nullptr) == MPX_OK);
        CHECK(mpx_synchronize(e) == MPX_OK);
    } else {
        CHECK(mpx_record_log(e, &b, o, cap, io, res) == MPX_OK);
    }
    CHECK(d_items.intact() && d_eff.intact() && d_perm.intact() && d_mask.intact());
    for (const In& x : held) CHECK(x.intact());
    CHECK(res[0].n_recs == n_recs && res[0].n_cmds == n_cmds && res[0].n_bytes == want.size());
    CHECK(res[0].flags == (fits ? 0u : MPX_LR_FULL));
    const uint8_t* after = (const uint8_t*)&res[1];
    for (size_t i = 0; i < sizeof(res[1]); ++i) CHECK(after[i] == 0x5C);
    if (want_off) {
        CHECK(memcmp(ioff.v.data(), want_item.data(), (n + 1) * 8) == 0);
        for (size_t i = (n + 1) * 8; i < ioff.v.size(); ++i) CHECK(ioff.v[i] == kGuardByte);
    } else {
        CHECK(ioff.untouched());
    }
    if (!fits) {
        CHECK(out.untouched());
        return;
    }
    CHECK(std::equal(want.begin(), want.end(), out.v.begin()));
    for (size_t i = want.size(); i < out.v.size(); ++i) CHECK(out.v[i] == kGuardByte);
}

#define SHIFTED(T, p, by) ((T*)((char*)(p) + (by)))

static void validation(mpx_engine* e) {
    alignas(16) mpx_accept_msg msgs[3] = {{10, 1, 0, 0}, {11, 1, 0, 0}, {12, 1, 0, 1}};
    alignas(16) mpx_accept_send sends[2] = {{10, 1, -1, MPX_PH_ACCEPT, 0, 2, 0}, {11, 1, -1, MPX_PH_ACCEPT, 2, 1, 0}};
    alignas(16) uint8_t eff[3] = {2, 2, 2}, mask[4] = {1, 1, 1, 1};
    alignas(16) uint32_t perm[3] = {2, 0, 3};
    alignas(16) uint64_t off0[3] = {0, 1, 3}, off1[3] = {0, 3, 4}, dn[2] = {1, 0};
    alignas(16) uint8_t op0[3] = {1, 2, 1}, op1[4] = {2, 1, 2, 1};
    alignas(16) int64_t key0[3] = {1, 2, 3}, val0[3] = {4, 5, 6}, key1[4] = {7, 8, 9, 10}, val1[4] = {1, 1, 1, 1};
    mpx_store_src src[2] = {{off0, 2, op0, key0, val0, 3, 2}, {off1, 2, op1, key1, val1, 4, 2}};
    Out out(200), ioff(32);
    alignas(16) mpx_record_result res;
    memset(&res, 0x5C, sizeof(res));
    CHECK(mpx_record_log_reserve(e, 8) == MPX_OK);
    mpx_record_batch ok{};
    ok.kind = MPX_LR_ACCEPTS, ok.format = MPX_LOG_DURABLE, ok.items = msgs, ok.effect = eff, ok.n = 3;
    ok.perm = perm, ok.src = src, ok.n_src = 2;
    uint8_t* const o = out.as<uint8_t>();
    uint64_t* const io = ioff.as<uint64_t>();
    auto both = [&](const mpx_record_batch* b, uint8_t* w, size_t cap, mpx_record_result* rs, int code) {
        FAILS(e, mpx_record_log(e, b, w, cap, io, rs), code);
        FAILS(e, mpx_record_log_dev(e, b, w, cap, io, rs, nullptr), code);
    };
    // null arguments
    both(nullptr, o, 200, &res, MPX_E_INVAL);
    both(&ok, nullptr, 200, &res, MPX_E_INVAL);
    both(&ok, o, 200, nullptr, MPX_E_INVAL);
    mpx_record_batch x = ok;
    x.items = nullptr;
    both(&x, o, 200, &res, MPX_E_INVAL);
    x = ok, x.effect = nullptr;
    both(&x, o, 200, &res, MPX_E_INVAL);
    x = ok, x.kind = MPX_LR_COMMITS, x.effect = nullptr;
    both(&x, o, 200, &res, MPX_E_INVAL);
    x = ok, x.src = nullptr;
    both(&x, o, 200, &res, MPX_E_INVAL);
    x = ok, x.kind = MPX_LR_DECIDED, x.items = sends, x.n = 2, x.n_inst = 4, x.inst_base = 10, x.mask = nullptr;
    both(&x, o, 200, &res, MPX_E_INVAL);
    for (int f = 0; f < 4; ++f) {
        mpx_store_src s2[2] = {src[0], src[1]};
        if (f == 0) s2[1].cmd_off = nullptr;
        if (f == 1) s2[1].op = nullptr;
        if (f == 2) s2[0].key = nullptr;
        if (f == 3) s2[0].val = nullptr;
        x = ok, x.src = s2;
        both(&x, o, 200, &res, MPX_E_INVAL);
    }
    // kind, format, flags, reserved, the sources' count, perm, the records' count
    x = ok, x.kind = 4;
    both(&x, o, 200, &res, MPX_E_INVAL);
    x = ok, x.format = MPX_LOG_CATCHUP;
    both(&x, o, 200, &res, MPX_E_INVAL);
    x = ok, x.format = 3;
    both(&x, o, 200, &res, MPX_E_INVAL);
    x = ok, x.flags = 2;
    both(&x, o, 200, &res, MPX_E_INVAL);
    x = ok, x.reserved = 1;
    both(&x, o, 200, &res, MPX_E_INVAL);
    x = ok, x.n_src = 0;
    both(&x, o, 200, &res, MPX_E_INVAL);
    x = ok, x.n_src = 17;
    both(&x, o, 200, &res, MPX_E_INVAL);
    x = ok, x.kind = MPX_LR_DECIDED, x.items = sends, x.n = 2, x.n_inst = 4, x.inst_base = 10, x.mask = mask, x.n_src = 17;
    both(&x, o, 200, &res, MPX_E_INVAL);
    x = ok, x.perm = nullptr;
    both(&x, o, 200, &res, MPX_E_INVAL);
    x = ok, x.n = 5;
    both(&x, o, 200, &res, MPX_E_INVAL);
    x = ok, x.kind = MPX_LR_SENDS, x.items = sends, x.n = 2;  // sends take one source
    both(&x, o, 200, &res, MPX_E_INVAL);
    x = ok, x.n = (size_t)0xFFFFFFFFull;
    both(&x, o, 200, &res, MPX_E_UNSUPPORTED);
    x = ok, x.format = MPX_LOG_DURABLE_CLASSIC;  // CLASSIC's handleAccept record is not covered
    both(&x, o, 200, &res, MPX_E_UNSUPPORTED);
    FAILS(e, mpx_record_log_reserve(e, (size_t)0xFFFFFFFFull), MPX_E_UNSUPPORTED);
    // the host form: d_n, the items
    x = ok, x.d_n = dn;
    FAILS(e, mpx_record_log(e, &x, o, 200, io, &res), MPX_E_INVAL);
    perm[1] = 4;
    FAILS(e, mpx_record_log(e, &ok, o, 200, io, &res), MPX_E_INVAL);
    perm[1] = 0;
    msgs[1].value_id = 2;
    FAILS(e, mpx_record_log(e, &ok, o, 200, io, &res), MPX_E_INVAL);
    x = ok, x.kind = MPX_LR_COMMITS;
    FAILS(e, mpx_record_log(e, &x, o, 200, io, &res), MPX_E_INVAL);
    msgs[1].value_id = 0;
    off0[1] = 4;  // [0, 4) leaves the 3 commands; and [4, 3) decreases
    FAILS(e, mpx_record_log(e, &ok, o, 200, io, &res), MPX_E_INVAL);
    msgs[1].value_id = 1;
    FAILS(e, mpx_record_log(e, &ok, o, 200, io, &res), MPX_E_INVAL);
    msgs[1].value_id = 2, off0[1] = 1, eff[1] = 1;  // ... not judged when it does not record
    CHECK(mpx_record_log(e, &ok, o, 200, io, &res) == MPX_OK && res.n_recs == 2 && res.n_cmds == 4 && res.n_bytes == 92);
    CHECK(io[0] == 0 && io[1] == 63 && io[2] == 63 && io[3] == 92 && o[0] == 1 && o[4] == 2 && o[8] == 10 && o[12] == 2);
    x = ok, x.kind = MPX_LR_COMMITS;  // a Commit without MPX_CH_CMDS writes metadata only, unjudged
    CHECK(mpx_record_log(e, &x, o, 200, io, &res) == MPX_OK && res.n_recs == 3 && res.n_bytes == 104 && io[2] == 75);
    msgs[1].value_id = 0, eff[1] = 2;
    src[0].n_cmds = (size_t)1 << 40, src[1].n_cmds = (size_t)1 << 40;  // 2^32 bytes and more in all
    off1[1] = 0x10000000ull, off1[2] = 0x10000000ull, msgs[0].value_id = 0, msgs[2].value_id = 0;
    FAILS(e, mpx_record_log(e, &ok, o, 200, io, &res), MPX_E_UNSUPPORTED);
    src[0].n_cmds = 3, src[1].n_cmds = 4, off1[1] = 3, off1[2] = 4, msgs[2].value_id = 1;
    x = ok, x.kind = MPX_LR_SENDS, x.items = sends, x.n = 2, x.n_src = 1, x.effect = nullptr, x.perm = nullptr;
    sends[1].n_cmds = 2;
    FAILS(e, mpx_record_log(e, &x, o, 200, io, &res), MPX_E_INVAL);
    sends[1].n_cmds = 1;
    x.kind = MPX_LR_DECIDED, x.n_inst = 4, x.inst_base = 10, x.mask = mask, x.src = nullptr, x.n_src = 0;
    for (const int32_t bad : {9, 14}) {
        sends[0].instance = bad;
        FAILS(e, mpx_record_log(e, &x, o, 200, io, &res), MPX_E_NIL_INSTANCE);
    }
    sends[0].flags = MPX_PH_PREPARE;  // ... not judged when it was not accepted
    CHECK(mpx_record_log(e, &x, o, 200, io, &res) == MPX_OK && res.n_recs == 1 && res.n_bytes == 12 && o[8] == 11 && o[4] == 3);
    x.format = MPX_LOG_DURABLE_CLASSIC;
    CHECK(mpx_record_log(e, &x, o, 200, io, &res) == MPX_OK && res.n_recs == 1 && res.n_bytes == 5 && o[4] == 3);
    sends[0].flags = MPX_PH_ACCEPT, sends[0].instance = 10;
    memset(out.v.data(), kGuardByte, out.v.size());
    memset(ioff.v.data(), kGuardByte, ioff.v.size());
    memset(&res, 0x5C, sizeof(res));
    // the device form's alignment rules
    auto dev = [&](const mpx_record_batch& b, uint8_t* w, uint64_t* i8, mpx_record_result* rs) {
        return mpx_record_log_dev(e, &b, w, 200, i8, rs, nullptr);
    };
    x = ok, x.items = SHIFTED(const void, msgs, 8);
    FAILS(e, dev(x, o, io, &res), MPX_E_INVAL);
    x = ok, x.perm = SHIFTED(const uint32_t, perm, 2);
    FAILS(e, dev(x, o, io, &res), MPX_E_INVAL);
    x = ok, x.d_n = SHIFTED(const uint64_t, dn, 4);
    FAILS(e, dev(x, o, io, &res), MPX_E_INVAL);
    for (int f = 0; f < 3; ++f) {
        mpx_store_src s2[2] = {src[0], src[1]};
        if (f == 0) s2[1].cmd_off = SHIFTED(const uint64_t, off1, 4);
        if (f == 1) s2[0].key = SHIFTED(const int64_t, key0, 4);
        if (f == 2) s2[1].val = SHIFTED(const int64_t, val1, 4);
        x = ok, x.src = s2;
        FAILS(e, dev(x, o, io, &res), MPX_E_INVAL);
    }
    FAILS(e, dev(ok, o, SHIFTED(uint64_t, io, 4), &res), MPX_E_INVAL);
    FAILS(e, dev(ok, o, io, SHIFTED(mpx_record_result, &res, 4)), MPX_E_INVAL);
    // nothing was touched
    CHECK(out.untouched() && ioff.untouched());
    const uint8_t* rb = (const uint8_t*)&res;
    for (size_t i = 0; i < sizeof(res); ++i) CHECK(rb[i] == 0x5C);
    // the device form reports a faulty item through the error word: it records nothing
    msgs[1].value_id = 2;
    CHECK(dev(ok, o, io, &res) == MPX_OK);
    FAILS(e, mpx_synchronize(e), MPX_E_INVAL);
    CHECK(res.n_recs == 2 && res.n_cmds == 4 && res.n_bytes == 92 && io[1] == 63 && io[2] == 63);
    msgs[1].value_id = 0;
    x = ok, x.kind = MPX_LR_DECIDED, x.items = sends, x.n = 2, x.n_inst = 4, x.inst_base = 10, x.mask = mask;
    x.src = nullptr, x.n_src = 0, x.effect = nullptr, x.perm = nullptr;
    sends[1].instance = 14;
    CHECK(dev(x, o, io, &res) == MPX_OK);
    FAILS(e, mpx_synchronize(e), MPX_E_NIL_INSTANCE);
    CHECK(res.n_recs == 1 && res.n_bytes == 12 && io[1] == 12 && io[2] == 12);
    sends[1].instance = 11;
    // d_n cuts the batch; out, op, effect and mask may sit at any address; item_off is optional
    alignas(16) uint8_t eff2[4] = {0, 2, 2, 2};
    memset(out.v.data(), kGuardByte, out.v.size());
    x = ok, x.d_n = dn, x.effect = eff2 + 1;
    CHECK(mpx_record_log_dev(e, &x, o + 3, 63, nullptr, &res, nullptr) == MPX_OK && mpx_synchronize(e) == MPX_OK);
    CHECK(res.n_recs == 1 && res.n_cmds == 3 && res.n_bytes == 63 && o[2] == kGuardByte && o[3] == 1 && o[66] == kGuardByte);
    // no item: legal with null arrays, the result is written
    mpx_record_batch none{};
    none.format = MPX_LOG_DURABLE, none.src = src, none.n_src = 1;
    for (const uint32_t f : {0u, MPX_LR_GENERAL}) {
        none.flags = f;
        memset(&res, 0x5C, sizeof(res));
        CHECK(mpx_record_log(e, &none, nullptr, 0, io, &res) == MPX_OK);
        CHECK(res.n_recs == 0 && res.n_cmds == 0 && res.n_bytes == 0 && res.flags == 0 && io[0] == 0);
    }
}

int main() {
    mpx_engine* e = open_engine();
    if (!e) return 1;
    validation(e);
    for (const bool dev : {false, true})
        for (const uint32_t call_flags : {0u, MPX_LR_GENERAL})
            for (const long cap_extra : {0L, 5L, -1L})
                for (const uint32_t kind : {MPX_LR_ACCEPTS, MPX_LR_COMMITS, MPX_LR_SENDS, MPX_LR_DECIDED})
                    for (const uint32_t format : {MPX_LOG_DURABLE, MPX_LOG_DURABLE_CLASSIC}) {
                        if (kind == MPX_LR_ACCEPTS && format == MPX_LOG_DURABLE_CLASSIC) continue;
                        valid(e, kind, format, 1, 1, {2}, cap_extra, dev, call_flags, true);
                        valid(e, kind, format, 3, 29, {2, 0, 1, 5, 3}, cap_extra, dev, call_flags, cap_extra != 5);
                        // ... of a size at which the arrays have slots of more than one 256-byte unit
                        valid(e, kind, format, 4, 700, {300, 17, 0, 2, 1}, cap_extra, dev, call_flags, true);
                        valid(e, kind, format, 2, 0, {1}, cap_extra, dev, call_flags, true);
                    }
    // the device form never allocates: on a fresh handle it needs its reserve call first
    mpx_engine* f = open_engine();
    if (!f) return 1;
    {
        alignas(16) mpx_accept_msg msgs[1] = {{0, 1, 0, 0}};
        alignas(16) uint8_t eff[1] = {2}, sop[2] = {1, 2}, out[64];
        alignas(16) uint64_t off[2] = {0, 2};
        alignas(16) int64_t skey[2] = {5, 6}, sval[2] = {7, 8};
        alignas(16) mpx_record_result res;
        const mpx_store_src src{off, 1, sop, skey, sval, 2, 1};
        mpx_record_batch b{};
        b.kind = MPX_LR_ACCEPTS, b.format = MPX_LOG_DURABLE, b.items = msgs, b.effect = eff, b.n = 1, b.src = &src, b.n_src = 1;
        FAILS(f, mpx_record_log_dev(f, &b, out, 64, nullptr, &res, nullptr), MPX_E_INVAL);
        CHECK(strstr(mpx_last_error(f), "mpx_record_log_dev") && strstr(mpx_last_error(f), "mpx_record_log_reserve"));
        CHECK(mpx_record_log_reserve(f, 1) == MPX_OK);
        CHECK(mpx_record_log_dev(f, &b, out, 64, nullptr, &res, nullptr) == MPX_OK && mpx_synchronize(f) == MPX_OK);
        CHECK(res.n_cmds == 2 && res.n_bytes == 46 && out[12] == 1 && out[13] == 5);
        // more items than were reserved for: refused before the items are looked at
        mpx_store_src many = src;
        many.n_recs = 5000;
        b.n = 5000, b.src = &many;
        FAILS(f, mpx_record_log_dev(f, &b, out, 64, nullptr, &res, nullptr), MPX_E_INVAL);
        CHECK(mpx_record_log_reserve(f, 5000) == MPX_OK);
        b.n = 1, b.src = &src, b.flags = MPX_LR_GENERAL;
        CHECK(mpx_record_log_dev(f, &b, out, 64, nullptr, &res, nullptr) == MPX_OK && mpx_synchronize(f) == MPX_OK);
        CHECK(res.n_cmds == 2 && res.n_bytes == 46);
    }
    CHECK(mpx_close(f) == MPX_OK);
    CHECK(mpx_close(e) == MPX_OK);
    mpx_record_result res;
    mpx_record_batch none{};
    CHECK(mpx_record_log(nullptr, &none, nullptr, 0, nullptr, &res) == MPX_E_INVAL);
    CHECK(mpx_record_log_reserve(nullptr, 1) == MPX_E_INVAL);
    CHECK(mpx_record_log_dev(nullptr, &none, nullptr, 0, nullptr, &res, nullptr) == MPX_E_INVAL);
    CHECK(mpx_record_bound(3, 7) == 12 * 3 + 17 * 7);
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("record_driver: all checks passed\n");
    return failures ? 1 : 0;
}
