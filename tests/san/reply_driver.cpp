// tests/san/reply_driver.cpp — TEST INFRASTRUCTURE ONLY: drives mpx_build_replies and its
// _reserve / _dev forms of the CPU build of engine.cpp + replies.cpp over the stub runtime
// (hip_stub.cpp) and the expanding stand-in of reply_stub.cpp under ASan + UBSan. Every
// argument-validation path of both forms must answer its code before anything is staged or
// launched; valid calls on guarded buffers must bring back exactly the expected records,
// mpx_commit_sends and counts through the staging arena, leave the inputs and the guard bytes
// alone and write nothing past the records the call produced. Exit status 0 = all checks passed.
#include <algorithm>

#include "san_check.hpp"

static mpx_engine* open_engine() {
    mpx_engine* e = nullptr;
    mpx_config cfg{5, MPX_MODE_MIN, 1 << 10, 0, 0, 0};
    CHECK(mpx_open(0, &cfg, &e) == MPX_OK && e);
    return e;
}

static bool tail_untouched(const Out& o, size_t from) {
    for (size_t i = from; i < o.v.size(); ++i)
        if (o.v[i] != kGuardByte) return false;
    return true;
}

static mpx_accept_send send(int32_t inst, uint32_t flags, uint64_t first, uint32_t n) {
    return mpx_accept_send{inst, 7, -1, flags, first, n, 0};
}
static mpx_reply_batch batch(uint32_t kind, const mpx_accept_send* s, size_t n, const mpx_proposal* m,
                             size_t n_props) {
    mpx_reply_batch b{};
    b.sends = s, b.n_sends = n, b.meta = m, b.n_props = n_props, b.kind = kind;
    b.pad_client = MPX_RB_NO_PAD;
    return b;
}

// slots of n_cmds[s] proposals each, flags[s]; instance 100 + s, selected by sel[s]; proposal j is
// {timestamp 1000 + j, id -j, client j % 5}; EXECUTED: the results of slot s start at ret_first[s]
// = 3 * s + the commands before it (so never at first_cmd), ret[i] = 7 * i - 3
static void valid_case(mpx_engine* e, uint32_t kind, std::vector<uint32_t> n_cmds,
                       std::vector<uint32_t> flags, std::vector<uint8_t> sel, size_t cap_short,
                       size_t pad_extra, bool with_cs, bool dev, uint32_t call_flags) {
    const size_t S = n_cmds.size();
    const bool refusals = kind == MPX_RB_FALSE;
    std::vector<mpx_accept_send> sends(S ? S : 1);
    std::vector<uint64_t> rf(S ? S : 1);
    size_t n_props = 0;
    for (size_t s = 0; s < S; ++s) {
        sends[s] = send(100 + (int32_t)s, flags[s], n_props, n_cmds[s]);
        rf[s] = 3 * s + n_props;
        n_props += n_cmds[s];
    }
    const size_t n_ret = n_props + 3 * S;
    std::vector<mpx_proposal> meta(n_props ? n_props : 1);
    std::vector<int64_t> ret(n_ret ? n_ret : 1);
    for (size_t j = 0; j < n_props; ++j) meta[j] = mpx_proposal{1000 + (int64_t)j, -(int32_t)j, (uint32_t)(j % 5)};
    for (size_t i = 0; i < n_ret; ++i) ret[i] = 7 * (int64_t)i - 3;
    // what the call must produce
    std::vector<mpx_reply_rec> want;
    std::vector<uint32_t> want_cs(S);
    uint64_t slots = 0;
    for (size_t s = 0; s < S; ++s) {
        const bool eligible = flags[s] & (refusals ? MPX_PH_NOT_LEADER | MPX_PH_REFUSED
                                                   : MPX_PH_ACCEPT | MPX_PH_PREPARE);
        const bool on = eligible && (refusals || sel[s]);
        want_cs[s] = on ? MPX_CS_SEND : 0;
        slots += on;
        if (!on) continue;
        const uint32_t cnt = refusals && !(flags[s] & MPX_PH_NOT_LEADER) ? std::min(n_cmds[s], 1u) : n_cmds[s];
        for (uint32_t k = 0; k < cnt; ++k) {
            const mpx_proposal m = meta[sends[s].first_cmd + k];
            if (refusals) want.push_back(mpx_reply_rec{0, 0, -1, m.client});
            else want.push_back(mpx_reply_rec{kind == MPX_RB_EXECUTED ? ret[rf[s] + k] : 0,
                                              m.timestamp, m.command_id, m.client});
        }
    }
    const size_t total = want.size();
    const bool pad = pad_extra != (size_t)-1;
    const size_t cap = pad ? total + pad_extra : total - std::min(total, cap_short);
    In d_sends = holding(sends.data(), S, 3), d_meta = holding(meta.data(), n_props, 4),
       d_ret = holding(ret.data(), n_ret, 5), d_rf = holding(rf.data(), S, 6);
    In d_mask(S, 7);
    for (size_t s = 0; s < S; ++s) d_mask.v[s] = sel[s] ? (uint8_t)(1 + s) : 0;
    d_mask.orig = d_mask.v;
    Out recs(cap * sizeof(mpx_reply_rec)), cs(S * sizeof(mpx_commit_send));
    mpx_reply_result res[2];
    memset(res, 0x5C, sizeof(res));
    mpx_reply_batch b = batch(kind, S ? d_sends.as<mpx_accept_send>() : nullptr, S,
                              n_props ? d_meta.as<mpx_proposal>() : nullptr, n_props);
    b.inst_base = 100, b.n_inst = S, b.flags = call_flags;
    if (!refusals) b.mask = d_mask.as<uint8_t>();
    if (kind == MPX_RB_EXECUTED) b.ret = d_ret.as<int64_t>(), b.n_ret = n_ret, b.ret_first = d_rf.as<uint64_t>();
    if (pad) b.pad_client = 99;
    mpx_reply_rec* r = cap ? recs.as<mpx_reply_rec>() : nullptr;
    mpx_commit_send* c = with_cs && !refusals ? cs.as<mpx_commit_send>() : nullptr;
    if (dev) {
        CHECK(mpx_build_replies_reserve(e, S) == MPX_OK);
        CHECK(mpx_build_replies_dev(e, &b, r, cap, c, res, nullptr) == MPX_OK);
        CHECK(mpx_synchronize(e) == MPX_OK);
    } else {
        CHECK(mpx_build_replies(e, &b, r, cap, c, res) == MPX_OK);
    }
    CHECK(d_sends.intact() && d_meta.intact() && d_ret.intact() && d_rf.intact() && d_mask.intact());
    CHECK(res[0].n_replies == total && res[0].n_slots == slots);
    const size_t real = std::min(total, cap), wrote = pad ? cap : real;
    for (size_t i = 0; i < wrote; ++i) {
        const mpx_reply_rec g = recs.as<mpx_reply_rec>()[i];
        const mpx_reply_rec w = i < real ? want[i] : mpx_reply_rec{0, 0, 0, 99};
        CHECK(g.value == w.value && g.timestamp == w.timestamp && g.command_id == w.command_id &&
              g.client == w.client);
    }
    CHECK(tail_untouched(recs, wrote * sizeof(mpx_reply_rec)));
    if (c) {
        for (size_t s = 0; s < S; ++s) {
            const mpx_commit_send g = cs.as<mpx_commit_send>()[s];
            CHECK(g.instance == 100 + (int32_t)s && g.ballot == 7 && g.first_cmd == sends[s].first_cmd &&
                  g.n_cmds == n_cmds[s] && g.flags == want_cs[s] && g.pad[0] == 0 && g.pad[1] == 0);
        }
        CHECK(tail_untouched(cs, S * sizeof(mpx_commit_send)));
    } else {
        CHECK(cs.untouched());
    }
    const uint8_t* after = (const uint8_t*)&res[1];
    for (size_t i = 0; i < sizeof(res[1]); ++i) CHECK(after[i] == 0x5C);
}

static void validation(mpx_engine* e) {
    alignas(16) mpx_accept_send s[3] = {send(10, MPX_PH_ACCEPT, 0, 2), send(11, MPX_PH_ACCEPT, 2, 1),
                                        send(-1, MPX_PH_NOT_LEADER, 3, 1)};
    alignas(16) mpx_proposal m[4] = {{1, 1, 0}, {2, 2, 1}, {3, 3, 2}, {4, 4, 3}};
    alignas(16) int64_t ret[4] = {5, 6, 7, 8};
    alignas(16) uint64_t rf[3] = {0, 2, 3};
    uint8_t mask[2] = {1, 1};
    Out recs(4 * sizeof(mpx_reply_rec)), cs(3 * sizeof(mpx_commit_send));
    mpx_reply_result res;
    memset(&res, 0x5C, sizeof(res));
    mpx_reply_rec* r = recs.as<mpx_reply_rec>();
    mpx_commit_send* c = cs.as<mpx_commit_send>();
    CHECK(mpx_build_replies_reserve(e, 3) == MPX_OK);
    auto both = [&](const mpx_reply_batch* b, mpx_reply_rec* rr, size_t cap, mpx_commit_send* cc,
                    mpx_reply_result* rs, int code) {
        FAILS(e, mpx_build_replies(e, b, rr, cap, cc, rs), code);
        FAILS(e, mpx_build_replies_dev(e, b, rr, cap, cc, rs, nullptr), code);
    };
    const mpx_reply_batch ok = batch(MPX_RB_DECIDED, s, 3, m, 4);
    // null arguments
    both(nullptr, r, 4, c, &res, MPX_E_INVAL);
    both(&ok, r, 4, c, nullptr, MPX_E_INVAL);
    both(&ok, nullptr, 4, c, &res, MPX_E_INVAL);
    mpx_reply_batch x = ok;
    x.sends = nullptr;
    both(&x, r, 4, c, &res, MPX_E_INVAL);
    x = ok, x.meta = nullptr;
    both(&x, r, 4, c, &res, MPX_E_INVAL);
    // unknown kind or flags, reserved
    x = ok, x.kind = 0;
    both(&x, r, 4, c, &res, MPX_E_INVAL);
    x = ok, x.kind = 4;
    both(&x, r, 4, c, &res, MPX_E_INVAL);
    x = ok, x.flags = 2;
    both(&x, r, 4, c, &res, MPX_E_INVAL);
    x = ok, x.reserved = 1;
    both(&x, r, 4, c, &res, MPX_E_INVAL);
    // the kind's forbidden or missing arrays
    x = ok, x.kind = MPX_RB_FALSE;
    both(&x, r, 4, c, &res, MPX_E_INVAL);  // commit_sends
    x.mask = mask, x.n_inst = 2, x.inst_base = 10;
    both(&x, r, 4, nullptr, &res, MPX_E_INVAL);
    x = ok, x.kind = MPX_RB_FALSE, x.ret = ret, x.n_ret = 4;
    both(&x, r, 4, nullptr, &res, MPX_E_INVAL);
    x = ok, x.kind = MPX_RB_FALSE, x.ret_first = rf;
    both(&x, r, 4, nullptr, &res, MPX_E_INVAL);
    x = ok, x.ret = ret, x.n_ret = 4;
    both(&x, r, 4, c, &res, MPX_E_INVAL);  // DECIDED with ret
    x = ok, x.ret_first = rf;
    both(&x, r, 4, c, &res, MPX_E_INVAL);
    x = ok, x.kind = MPX_RB_EXECUTED;
    both(&x, r, 4, c, &res, MPX_E_INVAL);  // EXECUTED without ret
    // the limits
    x = ok, x.n_sends = (size_t)0xFFFFFFFFull;
    both(&x, r, 4, c, &res, MPX_E_UNSUPPORTED);
    FAILS(e, mpx_build_replies_reserve(e, (size_t)0xFFFFFFFFull), MPX_E_UNSUPPORTED);
    // the slots, host form: a command range, a result range, the window
    alignas(16) mpx_accept_send bad[3] = {s[0], send(11, MPX_PH_ACCEPT, 2, 3), s[2]};
    x = ok, x.sends = bad;
    FAILS(e, mpx_build_replies(e, &x, r, 4, c, &res), MPX_E_INVAL);
    bad[1] = send(11, MPX_PH_ACCEPT, 5, 0);
    FAILS(e, mpx_build_replies(e, &x, r, 4, c, &res), MPX_E_INVAL);
    bad[1] = send(11, MPX_PH_NOT_LEADER, 2, 3);  // not eligible under DECIDED: not looked at
    CHECK(mpx_build_replies(e, &x, r, 4, nullptr, &res) == MPX_OK && res.n_replies == 2 && res.n_slots == 1);
    CHECK(tail_untouched(recs, 2 * sizeof(mpx_reply_rec)));
    memset(recs.v.data(), kGuardByte, recs.v.size());
    memset(&res, 0x5C, sizeof(res));
    x = ok, x.kind = MPX_RB_EXECUTED, x.ret = ret, x.n_ret = 2;
    FAILS(e, mpx_build_replies(e, &x, r, 4, c, &res), MPX_E_INVAL);
    x.n_ret = 4, x.ret_first = rf, rf[1] = 4;
    FAILS(e, mpx_build_replies(e, &x, r, 4, c, &res), MPX_E_INVAL);
    rf[1] = 2;
    x = ok, x.mask = mask, x.n_inst = 1, x.inst_base = 10;
    FAILS(e, mpx_build_replies(e, &x, r, 4, c, &res), MPX_E_NIL_INSTANCE);
    x.n_inst = 2, x.inst_base = 11;
    FAILS(e, mpx_build_replies(e, &x, r, 4, c, &res), MPX_E_NIL_INSTANCE);
    // the device form's alignment rules
    auto dev = [&](const mpx_reply_batch& b, mpx_reply_rec* rr, mpx_commit_send* cc, mpx_reply_result* rs) {
        return mpx_build_replies_dev(e, &b, rr, 4, cc, rs, nullptr);
    };
    x = ok, x.sends = (const mpx_accept_send*)((const char*)s + 8);
    FAILS(e, dev(x, r, c, &res), MPX_E_INVAL);
    x = ok, x.meta = (const mpx_proposal*)((const char*)m + 8);
    FAILS(e, dev(x, r, c, &res), MPX_E_INVAL);
    FAILS(e, dev(ok, r, (mpx_commit_send*)((char*)c + 8), &res), MPX_E_INVAL);
    FAILS(e, dev(ok, (mpx_reply_rec*)((char*)r + 4), c, &res), MPX_E_INVAL);
    FAILS(e, dev(ok, r, c, (mpx_reply_result*)((char*)&res + 4)), MPX_E_INVAL);
    x = ok, x.kind = MPX_RB_EXECUTED, x.n_ret = 4, x.ret = (const int64_t*)((const char*)ret + 4);
    FAILS(e, dev(x, r, c, &res), MPX_E_INVAL);
    x.ret = ret, x.ret_first = (const uint64_t*)((const char*)rf + 4);
    FAILS(e, dev(x, r, c, &res), MPX_E_INVAL);
    // nothing was touched
    CHECK(recs.untouched() && cs.untouched());
    const uint8_t* rb = (const uint8_t*)&res;
    for (size_t i = 0; i < sizeof(res); ++i) CHECK(rb[i] == 0x5C);
    // the device form reports a faulty slot through the error word: its code at the next
    // synchronising call, the slot emits nothing, its neighbours do
    bad[1] = send(11, MPX_PH_ACCEPT, 2, 3);
    x = ok, x.sends = bad;
    CHECK(dev(x, r, c, &res) == MPX_OK);
    FAILS(e, mpx_synchronize(e), MPX_E_INVAL);
    CHECK(res.n_replies == 2 && res.n_slots == 1 && c[0].flags == MPX_CS_SEND && c[1].flags == 0 &&
          c[1].n_cmds == 3 && c[2].flags == 0 && r[1].command_id == 2);
    x = ok, x.mask = mask, x.n_inst = 1, x.inst_base = 10;
    CHECK(dev(x, r, c, &res) == MPX_OK);
    FAILS(e, mpx_synchronize(e), MPX_E_NIL_INSTANCE);
    CHECK(res.n_replies == 2 && res.n_slots == 1 && c[1].flags == 0);
    // ... and the same call is legal once repaired; recs may sit at an odd multiple of 8, the
    // mask at any address
    x.n_inst = 2;
    x.mask = mask + 0;
    CHECK(mpx_build_replies_dev(e, &x, (mpx_reply_rec*)((char*)r + 8), 3, c, &res, nullptr) == MPX_OK &&
          mpx_synchronize(e) == MPX_OK && res.n_replies == 3 && res.n_slots == 2);
    // no slot, no capacity: legal, with null arrays
    const mpx_reply_batch none = batch(MPX_RB_DECIDED, nullptr, 0, nullptr, 0);
    CHECK(mpx_build_replies(e, &none, nullptr, 0, nullptr, &res) == MPX_OK);
    CHECK(res.n_replies == 0 && res.n_slots == 0);
    // a capacity of 0 with a null recs still counts, and still fills the commit sends
    CHECK(mpx_build_replies(e, &ok, nullptr, 0, c, &res) == MPX_OK && res.n_replies == 3 &&
          res.n_slots == 2 && c[1].flags == MPX_CS_SEND && c[2].flags == 0);
}

int main() {
    mpx_engine* e = open_engine();
    if (!e) return 1;
    validation(e);
    const uint32_t A = MPX_PH_ACCEPT, P = MPX_PH_PREPARE, NL = MPX_PH_NOT_LEADER, RF = MPX_PH_REFUSED;
    const size_t no_pad = (size_t)-1;
    for (const uint32_t kind : {MPX_RB_FALSE, MPX_RB_DECIDED, MPX_RB_EXECUTED})
        for (const uint32_t call_flags : {0u, MPX_RB_GENERAL})
            for (const size_t cap_short : {(size_t)0, (size_t)1, (size_t)1000000}) {
                valid_case(e, kind, {2}, {kind == MPX_RB_FALSE ? NL : A}, {1}, cap_short, no_pad, true, false, call_flags);
                valid_case(e, kind, {3, 0, 5, 1, 4, 2}, {A, A, NL, RF, P, A}, {1, 1, 1, 1, 0, 1}, cap_short, no_pad,
                           true, false, call_flags);
                // ... of a size at which the arrays have slots of more than one 256-byte unit
                valid_case(e, kind, {300, 17, 0, 211, 40}, {A, RF, A, NL, P}, {1, 0, 1, 1, 1}, cap_short, no_pad,
                           cap_short != 1, false, call_flags);
                valid_case(e, kind, {}, {}, {}, cap_short, no_pad, true, false, call_flags);
                valid_case(e, kind, {4, 4}, {A, NL}, {0, 0}, cap_short, no_pad, true, false, call_flags);
            }
    for (const uint32_t kind : {MPX_RB_FALSE, MPX_RB_DECIDED, MPX_RB_EXECUTED})
        for (const size_t pad_extra : {(size_t)0, (size_t)1, (size_t)40}) {
            valid_case(e, kind, {300, 17, 0, 211, 40}, {A, RF, A, NL, P}, {1, 0, 1, 1, 1}, 0, pad_extra, true, false, 0);
            valid_case(e, kind, {}, {}, {}, 0, pad_extra, false, false, MPX_RB_GENERAL);
        }
    // the device form never allocates: on a fresh handle it needs its reserve call first (a call
    // of no slot does not), and a reserve that is too small is refused as well
    mpx_engine* f = open_engine();
    if (!f) return 1;
    {
        alignas(16) mpx_accept_send s[2] = {send(1, A, 0, 1), send(2, A, 1, 1)};
        alignas(16) mpx_proposal m[2] = {{1, 1, 0}, {2, 2, 1}};
        alignas(16) mpx_reply_rec r[2];
        alignas(16) mpx_reply_result res;
        mpx_reply_batch b = batch(MPX_RB_DECIDED, s, 2, m, 2);
        FAILS(f, mpx_build_replies_dev(f, &b, r, 2, nullptr, &res, nullptr), MPX_E_INVAL);
        CHECK(strstr(mpx_last_error(f), "mpx_build_replies_dev") &&
              strstr(mpx_last_error(f), "mpx_build_replies_reserve"));
        b.n_sends = 0;
        b.pad_client = 5;
        CHECK(mpx_build_replies_dev(f, &b, r, 2, nullptr, &res, nullptr) == MPX_OK);
        CHECK(mpx_synchronize(f) == MPX_OK && res.n_replies == 0 && r[1].client == 5 && r[0].value == 0);
        b.n_sends = 2;
        b.pad_client = MPX_RB_NO_PAD;
        CHECK(mpx_build_replies_reserve(f, 2) == MPX_OK);
        b.n_sends = 100000;  // (refused before the sends are looked at)
        FAILS(f, mpx_build_replies_dev(f, &b, r, 2, nullptr, &res, nullptr), MPX_E_INVAL);
        b.n_sends = 2;
        CHECK(mpx_build_replies_dev(f, &b, r, 2, nullptr, &res, nullptr) == MPX_OK);
        CHECK(mpx_synchronize(f) == MPX_OK && res.n_replies == 2 && r[1].command_id == 2);
    }
    for (const uint32_t call_flags : {0u, MPX_RB_GENERAL}) {
        valid_case(f, MPX_RB_EXECUTED, {300, 17, 0, 211, 40}, {A, RF, A, NL, P}, {1, 0, 1, 1, 1}, 0, no_pad, true, true, call_flags);
        valid_case(f, MPX_RB_DECIDED, {300, 17, 0, 211, 40}, {A, RF, A, NL, P}, {1, 0, 1, 1, 1}, 100, no_pad, true, true, call_flags);
        valid_case(f, MPX_RB_FALSE, {300, 17, 0, 211, 40}, {A, RF, A, NL, P}, {1, 0, 1, 1, 1}, 0, 33, false, true, call_flags);
    }
    CHECK(mpx_close(f) == MPX_OK);
    CHECK(mpx_close(e) == MPX_OK);
    mpx_reply_result res;
    const mpx_reply_batch none = batch(MPX_RB_DECIDED, nullptr, 0, nullptr, 0);
    CHECK(mpx_build_replies(nullptr, &none, nullptr, 0, nullptr, &res) == MPX_E_INVAL);
    CHECK(mpx_build_replies_reserve(nullptr, 1) == MPX_E_INVAL);
    CHECK(mpx_build_replies_dev(nullptr, &none, nullptr, 0, nullptr, &res, nullptr) == MPX_E_INVAL);
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("reply_driver: all checks passed\n");
    return failures ? 1 : 0;
}
