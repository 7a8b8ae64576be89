// tests/san/prepare_handle_driver.cpp — TEST INFRASTRUCTURE ONLY: drives mpx_gather_prepares,
// mpx_prepare_handle and mpx_encode_prepare_replies and their _reserve / _dev forms of the CPU
// build of engine.cpp + prepare_handle.cpp over the stub runtime (hip_stub.cpp) and stand-ins for
// the launchers that really do the work (prepare_handle_stub.cpp), under ASan + UBSan. Every
// argument-validation path of the three calls must answer its code before anything is staged;
// valid MIN and CLASSIC calls bring the hand-worked bytes of tests/prepare_handle_kat.py back
// through the staging on guarded buffers, and a 2^20-entry arena is staged as the referenced
// commands alone. Exit status 0 = all checks passed.
#include <string>

#include "san_check.hpp"

struct PhStubSeen {
    uint64_t calls, n_src, n_inst, non_nil, flagged, n_groups;
};
extern PhStubSeen ph_stub_seen;

constexpr uint64_t kOffGuard = 0x5C5C5C5C5C5C5C5Cull;
constexpr int32_t N = 3;

static mpx_engine* open_engine(int mode) {
    mpx_engine* e = nullptr;
    mpx_config cfg{N, mode, 1 << 10, 0, 0, 0};
    CHECK(mpx_open(0, &cfg, &e) == MPX_OK && e);
    return e;
}

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> v;
    int hi = -1;
    for (char c : s) {
        const int d = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
        if (d < 0) continue;
        if (hi < 0) hi = d;
        else v.push_back((uint8_t)(hi * 16 + d)), hi = -1;
    }
    return v;
}

// The known answers of tests/prepare_handle_kat.py, two groups side by side in one window of
// 2 x 8 slots at base 10 so that the second group's span is staged alone:
//   MIN      group 0 is "min_no_log" moved to [10, 18): follower 1, slots 10..14 full, crt 15,
//            committedUpTo 14, Prepare {leader 2, 0x21, LastCommitted 14};
//            group 1 is "min_command_and_log" moved to [18, 26): follower 2, 18 {COMMITTED, 0x11,
//            [(1 5 6)]}, 19 {COMMITTED, 0x12, nil Cmds}, 20 {ACCEPTED, 0x13, [(1 7 8), (2 9 0)]},
//            crt 20, committedUpTo 19, Prepare {leader 0, 0x20, LastCommitted 17}
//   CLASSIC  "classic_nil" on instance 17 of group 0 (defaultBallot 5) and "classic_inst" on
//            instance 20 of group 1 {ACCEPTED, 9, [(1 2 3)]}, defaultBallot 3
static const char* kC78 = "01 0700000000000000 0800000000000000 02 0900000000000000 0000000000000000";
static const char* kC56 = "01 0500000000000000 0600000000000000";
static const char* kC23 = "01 0200000000000000 0300000000000000";
static std::vector<uint8_t> min_f0() {  // to leader 2
    return unhex("0c 01000000 0e000000 01 21000000 0e000000 00 00");
}
static std::vector<uint8_t> min_f1() {  // to leader 0
    return unhex(std::string("0c 02000000 14000000 01 20000000 13000000 04") + kC78 + "04" +
                 "11000000 03000000 02" + kC56 + "12000000 03000000 00");
}
static std::vector<uint8_t> cl_f0() { return unhex("0c 11000000 01 05000000 00"); }  // to leader 1
static std::vector<uint8_t> cl_f1() {  // to leader 2
    return unhex(std::string("0c 14000000 00 09000000 02") + kC23);
}

struct Kat {
    bool min;
    alignas(16) mpx_prepare_msg msgs[2];
    alignas(16) mpx_acceptor_state st[16];
    alignas(16) mpx_inst_cmds inst[16];
    alignas(16) mpx_proposer_group groups[2];
    alignas(16) mpx_group_prep_state gps[2];
    alignas(16) int32_t pc[6];
    std::vector<uint8_t> sop;
    std::vector<int64_t> skey, sval;
    explicit Kat(int mode, size_t arena_size = 8) : min(mode == MPX_MODE_MIN) {
        for (int i = 0; i < 16; ++i) {
            st[i] = mpx_acceptor_state{MPX_STATUS_NIL, -1, MPX_VALUE_KEEP, 0};
            inst[i] = mpx_inst_cmds{0, 0, 0};
        }
        sop.assign(arena_size, 0xEE), skey.assign(arena_size, -1), sval.assign(arena_size, -1);
        for (int g = 0; g < 2; ++g) {
            gps[g] = mpx_group_prep_state{1, 2, 3, 4, 5, 6, 7, 8};
            for (int q = 0; q < N; ++q) pc[g * N + q] = 100 + g;
        }
        const size_t a = arena_size - 3, m = arena_size / 2;  // a range at the arena's very end
        if (min) {
            for (int i = 0; i < 5; ++i) st[i] = {MPX_COMMITTED, 0x10, 0, 0};
            st[8] = {MPX_COMMITTED, 0x11, 0, 0}, st[9] = {MPX_COMMITTED, 0x12, MPX_VALUE_KEEP, 0};
            st[10] = {MPX_ACCEPTED, 0x13, 0, 0};
            inst[8] = {m, 1, MPX_IC_HAS_CMDS}, inst[10] = {a, 2, MPX_IC_HAS_CMDS};
            inst[9] = {77, 5, 0};  // unflagged: Cmds == nil, first_cmd / n_cmds are not read
            inst[2] = {0, 1, MPX_IC_HAS_CMDS};  // in no frame
            sop[m] = 1, skey[m] = 5, sval[m] = 6;
            sop[a] = 1, skey[a] = 7, sval[a] = 8, sop[a + 1] = 2, skey[a + 1] = 9, sval[a + 1] = 0;
            groups[0] = {0x10, 1, 0, 2, 15, 14, {0, 0}}, groups[1] = {0x13, 2, 1, 2, 20, 19, {0, 0}};
            msgs[0] = {0, 0x21, 2, 14}, msgs[1] = {1, 0x20, 0, 17};
        } else {
            st[10] = {MPX_ACCEPTED, 9, 0, 0};
            inst[10] = {a, 1, MPX_IC_HAS_CMDS};
            sop[a] = 1, skey[a] = 2, sval[a] = 3;
            groups[0] = {5, 0, 0, 0, 10, 9, {0, 0}}, groups[1] = {3, 0, 0, 0, 18, 17, {0, 0}};
            msgs[0] = {17, 5, 1, 1}, msgs[1] = {20, 8, 2, 1};
        }
    }
};

static bool holds(const Out& out, const std::vector<uint8_t>& want, size_t n) {
    for (size_t i = 0; i < out.v.size(); ++i)
        if (out.v[i] != (i < n ? want[i] : kGuardByte)) return false;
    return true;
}

// Prepare frames between a Beacon and a CommitShort, the `other` list as mpx_decode_stream leaves it
static void gather_case(mpx_engine* e, int mode, bool dev) {
    const bool min = mode == MPX_MODE_MIN;
    std::vector<uint8_t> buf = unhex("06 1111111111111111");
    std::vector<mpx_peer_frame> oth = {{0, MPX_PEER_BEACON, {0, 0, 0}}};
    oth.push_back({(uint32_t)buf.size(), MPX_PEER_PREPARE, {0, 0, 0}});
    const std::vector<uint8_t> p0 = min ? unhex("08 02000000 21000000 0e000000")
                                        : unhex("08 01000000 11000000 05000000 01");
    buf.insert(buf.end(), p0.begin(), p0.end());
    oth.push_back({(uint32_t)buf.size(), MPX_PEER_COMMIT_SHORT, {0, 0, 0}});
    const std::vector<uint8_t> cs = unhex("0b 01000000 02000000 03000000 04000000");
    buf.insert(buf.end(), cs.begin(), cs.end());
    oth.push_back({(uint32_t)buf.size(), MPX_PEER_PREPARE, {0, 0, 0}});
    const std::vector<uint8_t> p1 = min ? unhex("08 00000000 20000000 11000000")
                                        : unhex("08 02000000 14000000 08000000 ff");
    buf.insert(buf.end(), p1.begin(), p1.end());
    const size_t len = buf.size();
    buf.resize((len + 15) & ~(size_t)15);  // (the device form may read up to len rounded up to 16)
    In b = holding(buf.data(), buf.size(), 1), o = holding(oth.data(), oth.size(), 2);
    for (const size_t cap : {(size_t)2, (size_t)1, (size_t)0}) {
        Out msgs(cap * sizeof(mpx_prepare_msg)), idx(cap * 4);
        uint64_t cnt[2] = {kOffGuard, kOffGuard};
        if (dev) CHECK(mpx_encode_prepare_replies_reserve(e, oth.size(), 0, 1) == MPX_OK);
        const int rc =
            dev ? mpx_gather_prepares_dev(e, b.as<uint8_t>(), len, o.as<mpx_peer_frame>(), oth.size(),
                                          nullptr, 7, msgs.as<mpx_prepare_msg>(), idx.as<uint32_t>(),
                                          cap, cnt, nullptr)
                : mpx_gather_prepares(e, b.as<uint8_t>(), len, o.as<mpx_peer_frame>(), oth.size(), 7,
                                      msgs.as<mpx_prepare_msg>(), idx.as<uint32_t>(), cap, cnt);
        if (rc != MPX_OK) fprintf(stderr, "  got %d: %s\n", rc, mpx_last_error(e));
        CHECK(rc == MPX_OK && cnt[0] == 2 && cnt[1] == kOffGuard);
        const mpx_prepare_msg want[2] = {min ? mpx_prepare_msg{7, 0x21, 2, 14} : mpx_prepare_msg{17, 5, 1, 1},
                                         min ? mpx_prepare_msg{7, 0x20, 0, 17} : mpx_prepare_msg{20, 8, 2, 255}};
        const uint32_t widx[2] = {1, 3};
        CHECK(memcmp(msgs.v.data(), want, cap * sizeof(mpx_prepare_msg)) == 0);
        CHECK(memcmp(idx.v.data(), widx, cap * 4) == 0);
        for (size_t i = cap * sizeof(mpx_prepare_msg); i < msgs.v.size(); ++i) CHECK(msgs.v[i] == kGuardByte);
        for (size_t i = cap * 4; i < idx.v.size(); ++i) CHECK(idx.v[i] == kGuardByte);
        CHECK(b.intact() && o.intact());
    }
}

// handle -> encode on guarded copies; only: -1 both messages, else that message alone (its
// group's span is then staged alone). spare < 0: out_cap is short.
static void valid_case(mpx_engine* e, int mode, const Kat& k, int only, int spare, bool dev) {
    const bool min = mode == MPX_MODE_MIN;
    const size_t n = only < 0 ? 2 : 1, rb = min ? sizeof(mpx_prepare_reply_min) : sizeof(mpx_prepare_reply);
    In msgs = holding(k.msgs + (only < 0 ? 0 : only), n, 1), st = holding(k.st, 16, 2),
       inst = holding(k.inst, 16, 3), sop = holding(k.sop.data(), k.sop.size(), 4),
       skey = holding(k.skey.data(), k.skey.size(), 5), sval = holding(k.sval.data(), k.sval.size(), 6);
    alignas(16) mpx_proposer_group groups[2] = {k.groups[0], k.groups[1]};
    alignas(16) mpx_group_prep_state gps[2] = {k.gps[0], k.gps[1]};
    alignas(16) int32_t pc[8] = {k.pc[0], k.pc[1], k.pc[2], k.pc[3], k.pc[4], k.pc[5], 0, 0};
    Out rep(n * rb), to(n * 4), eff(n), lf(min ? n * 4 : 0);
    const int rc = dev ? mpx_prepare_handle_dev(e, msgs.as<mpx_prepare_msg>(), n, st.as<mpx_acceptor_state>(),
                                                16, 10, groups, 2, 8, min ? gps : nullptr,
                                                min ? pc : nullptr, rep.as<void>(), to.as<int32_t>(),
                                                eff.as<uint8_t>(), min ? lf.as<int32_t>() : nullptr, nullptr)
                       : mpx_prepare_handle(e, msgs.as<mpx_prepare_msg>(), n, st.as<mpx_acceptor_state>(), 16,
                                            10, groups, 2, 8, min ? gps : nullptr, min ? pc : nullptr,
                                            rep.as<void>(), to.as<int32_t>(), eff.as<uint8_t>(),
                                            min ? lf.as<int32_t>() : nullptr);
    if (rc != MPX_OK) fprintf(stderr, "  got %d: %s\n", rc, mpx_last_error(e));
    CHECK(rc == MPX_OK);
    if (!dev) CHECK(ph_stub_seen.n_groups == n && ph_stub_seen.n_inst == 8 * n);  // the span alone
    CHECK(msgs.intact() && st.intact());
    for (size_t i = n * rb; i < rep.v.size(); ++i) CHECK(rep.v[i] == kGuardByte);
    for (size_t i = n * 4; i < to.v.size(); ++i) CHECK(to.v[i] == kGuardByte);
    for (size_t i = n; i < eff.v.size(); ++i) CHECK(eff.v[i] == kGuardByte);
    for (size_t i = min ? n * 4 : 0; i < lf.v.size(); ++i) CHECK(lf.v[i] == kGuardByte);
    // records, effects and the groups after
    for (size_t j = 0; j < n; ++j) {
        const int m = only < 0 ? (int)j : only;
        if (min) {
            const mpx_prepare_reply_min want[2] = {{1, 14, 0x21, 14, 1, MPX_VALUE_KEEP}, {2, 20, 0x20, 19, 1, 10}};
            CHECK(memcmp(rep.v.data() + j * rb, &want[m], rb) == 0);
            CHECK(lf.as<int32_t>()[j] == (m ? 18 : 15));
            CHECK(eff.v[j] == (m ? (MPX_PRH_OK | MPX_PRH_RAISED | MPX_PRH_LOG) : (MPX_PRH_OK | MPX_PRH_RAISED)));
            CHECK(to.as<int32_t>()[j] == (m ? 0 : 2));
            const mpx_proposer_group wg[2] = {{0x21, 1, 2, 0, 15, 14, {0, 0}}, {0x20, 2, 0, 0, 21, 19, {0, 0}}};
            CHECK(memcmp(&groups[m], &wg[m], sizeof(wg[0])) == 0);
            const int32_t first = 10 + 8 * m, bal = m ? 0x20 : 0x21;
            const mpx_group_prep_state wp{bal, 0, 0, bal, first, MPX_VALUE_KEEP, 7, 8};
            CHECK(memcmp(&gps[m], &wp, sizeof(wp)) == 0);
            for (int q = 0; q < N; ++q) CHECK(pc[m * N + q] == first);
        } else {
            const mpx_prepare_reply want[2] = {{17, 5, 1, MPX_VALUE_KEEP}, {20, 9, 0, 10}};
            CHECK(memcmp(rep.v.data() + j * rb, &want[m], rb) == 0);
            CHECK(eff.v[j] == (m ? MPX_PRH_RAISED : MPX_PRH_OK));
            CHECK(to.as<int32_t>()[j] == (m ? 2 : 1));
            CHECK(groups[m].default_ballot == (m ? 8 : 5));
        }
    }
    if (only >= 0) {  // the other group was not touched
        CHECK(memcmp(&groups[1 - only], &k.groups[1 - only], sizeof(groups[0])) == 0);
        CHECK(memcmp(&gps[1 - only], &k.gps[1 - only], sizeof(gps[0])) == 0);
        CHECK(pc[(1 - only) * N] == k.pc[(1 - only) * N]);
    }
    // the frames: destination by destination
    const std::vector<uint8_t> f0 = min ? min_f0() : cl_f0(), f1 = min ? min_f1() : cl_f1();
    std::vector<uint8_t> want;
    uint64_t woff[4] = {0, 0, 0, 0};
    for (int q = 0; q < N; ++q) {
        for (size_t j = 0; j < n; ++j) {
            const int m = only < 0 ? (int)j : only;
            if (to.as<int32_t>()[j] != q) continue;
            const std::vector<uint8_t>& f = m ? f1 : f0;
            want.insert(want.end(), f.begin(), f.end());
        }
        woff[q + 1] = want.size();
    }
    In reps = holding(rep.v.data(), n * rb, 7), tos = holding(to.v.data(), n * 4, 8),
       lfs = holding(lf.v.data(), min ? n * 4 : 0, 9);
    mpx_prepare_reply_batch b{};
    b.replies = reps.as<void>(), b.reply_to = tos.as<int32_t>();
    b.log_from = min ? lfs.as<int32_t>() : nullptr;
    b.n = n, b.n_dest = N, b.inst_base = 10, b.n_inst = 16;
    b.st = min ? st.as<mpx_acceptor_state>() : nullptr, b.inst = inst.as<mpx_inst_cmds>();
    b.src_op = sop.as<uint8_t>(), b.src_key = skey.as<int64_t>(), b.src_val = sval.as<int64_t>();
    b.n_src = k.sop.size();
    const size_t total = want.size(), out_cap = total + spare;
    Out out(spare < 0 ? total : out_cap);
    std::vector<uint64_t> off((size_t)N + 2, kOffGuard);
    if (dev) CHECK(mpx_encode_prepare_replies_reserve(e, n, 16, N) == MPX_OK);
    const int rc2 = dev ? mpx_encode_prepare_replies_dev(e, &b, out.as<uint8_t>(), out_cap, off.data(), nullptr)
                        : mpx_encode_prepare_replies(e, &b, out.as<uint8_t>(), out_cap, off.data());
    if (spare < 0 && !dev) {
        CHECK(rc2 == MPX_E_INVAL && strstr(mpx_last_error(e), "out_cap"));
        CHECK(out.untouched());
    } else {
        if (rc2 != MPX_OK) fprintf(stderr, "  got %d: %s\n", rc2, mpx_last_error(e));
        CHECK(rc2 == MPX_OK);
        CHECK(holds(out, want, total < out_cap ? total : out_cap));
    }
    for (int q = 0; q <= N; ++q) CHECK(off[q] == woff[q]);
    CHECK(off[(size_t)N + 1] == kOffGuard);
    CHECK(reps.intact() && tos.intact() && lfs.intact() && st.intact() && inst.intact());
    CHECK(sop.intact() && skey.intact() && sval.intact());
}

static void validation(mpx_engine* e, int mode) {
    const bool min = mode == MPX_MODE_MIN;
    Kat k(mode);
    const uint64_t calls = ph_stub_seen.calls;
    // ---- the gather
    {
        alignas(16) uint8_t buf[32] = {8};
        mpx_peer_frame oth[1] = {{0, MPX_PEER_PREPARE, {0, 0, 0}}};
        alignas(16) mpx_prepare_msg m[1];
        uint32_t idx[1];
        uint64_t cnt = kOffGuard;
        FAILS(e, mpx_gather_prepares(e, buf, 32, oth, 1, 0, m, idx, 1, nullptr), MPX_E_INVAL);
        FAILS(e, mpx_gather_prepares(e, nullptr, 32, oth, 1, 0, m, idx, 1, &cnt), MPX_E_INVAL);
        FAILS(e, mpx_gather_prepares(e, buf, 32, nullptr, 1, 0, m, idx, 1, &cnt), MPX_E_INVAL);
        FAILS(e, mpx_gather_prepares(e, buf, 32, oth, 1, 0, nullptr, idx, 1, &cnt), MPX_E_INVAL);
        FAILS(e, mpx_gather_prepares(e, buf, 32, oth, 1, 0, m, nullptr, 1, &cnt), MPX_E_INVAL);
        FAILS(e, mpx_gather_prepares(e, buf, (size_t)1 << 31, oth, 1, 0, m, idx, 1, &cnt), MPX_E_UNSUPPORTED);
        FAILS(e, mpx_gather_prepares(e, buf, 32, oth, (size_t)1 << 32, 0, m, idx, 1, &cnt), MPX_E_UNSUPPORTED);
        // a frame that ends one byte past the buffer (13 bytes in MIN, 14 in CLASSIC)
        FAILS(e, mpx_gather_prepares(e, buf, min ? 12 : 13, oth, 1, 0, m, idx, 1, &cnt), MPX_E_INVAL);
        CHECK(cnt == kOffGuard);
        FAILS(e, mpx_gather_prepares_dev(e, buf + 4, 28, oth, 1, nullptr, 0, m, idx, 1, &cnt, nullptr), MPX_E_INVAL);
        CHECK(strstr(mpx_last_error(e), "aligned"));
    }
    // ---- the handler
    {
        alignas(16) uint8_t rep[64];
        int32_t to[2], lf[2];
        uint8_t eff[2];
        auto call = [&](const mpx_prepare_msg* m, size_t n, size_t n_inst, size_t n_groups, uint32_t ipg) {
            return mpx_prepare_handle(e, m, n, k.st, n_inst, 10, k.groups, n_groups, ipg, nullptr, nullptr,
                                      rep, to, eff, min ? lf : nullptr);
        };
        FAILS(e, call(nullptr, 2, 16, 2, 8), MPX_E_INVAL);
        FAILS(e, call(k.msgs, 2, 16, 2, 0), MPX_E_INVAL);
        FAILS(e, call(k.msgs, 2, 15, 2, 8), MPX_E_INVAL);
        FAILS(e, call(k.msgs, 2, 0, 0, 8), MPX_E_INVAL);
        FAILS(e, call(k.msgs, (size_t)1 << 32, 16, 2, 8), MPX_E_UNSUPPORTED);
        FAILS(e, mpx_prepare_handle(e, k.msgs, 2, nullptr, 16, 10, k.groups, 2, 8, nullptr, nullptr, rep,
                                    to, eff, lf), MPX_E_INVAL);
        FAILS(e, mpx_prepare_handle(e, k.msgs, 2, k.st, 16, 10, nullptr, 2, 8, nullptr, nullptr, rep, to,
                                    eff, lf), MPX_E_INVAL);
        FAILS(e, mpx_prepare_handle(e, k.msgs, 2, k.st, 16, 10, k.groups, 2, 8, nullptr, nullptr, nullptr,
                                    to, eff, lf), MPX_E_INVAL);
        FAILS(e, mpx_prepare_handle(e, k.msgs, 2, k.st, 16, 10, k.groups, 2, 8, nullptr, nullptr, rep,
                                    nullptr, eff, lf), MPX_E_INVAL);
        FAILS(e, mpx_prepare_handle(e, k.msgs, 2, k.st, 16, 10, k.groups, 2, 8, nullptr, nullptr, rep, to,
                                    nullptr, lf), MPX_E_INVAL);
        if (min)
            FAILS(e, mpx_prepare_handle(e, k.msgs, 2, k.st, 16, 10, k.groups, 2, 8, nullptr, nullptr, rep,
                                        to, eff, nullptr), MPX_E_INVAL);
        alignas(16) mpx_prepare_msg m[2] = {k.msgs[1], k.msgs[0]};  // out of order
        FAILS(e, call(m, 2, 16, 2, 8), MPX_E_INVAL);
        m[0] = k.msgs[0], m[1] = k.msgs[1];
        m[1].leader_id = N;
        FAILS(e, call(m, 2, 16, 2, 8), MPX_E_BAD_ID);
        m[1].leader_id = -1;
        FAILS(e, call(m, 2, 16, 2, 8), MPX_E_BAD_ID);
        m[1] = k.msgs[1];
        m[1].key = min ? 2 : 26;  // no such group / past the window
        FAILS(e, call(m, 2, 16, 2, 8), min ? MPX_E_INVAL : MPX_E_NIL_INSTANCE);
        m[1] = k.msgs[1];
        m[0].key = min ? -1 : 9;
        FAILS(e, call(m, 2, 16, 2, 8), min ? MPX_E_INVAL : MPX_E_NIL_INSTANCE);
        CHECK(call(m, 0, 16, 2, 8) == MPX_OK);  // an empty batch
        FAILS(e, mpx_prepare_handle_dev(e, (const mpx_prepare_msg*)((const char*)k.msgs + 8), 1, k.st, 16,
                                        10, k.groups, 2, 8, nullptr, nullptr, rep, to, eff, lf, nullptr),
              MPX_E_INVAL);
        FAILS(e, mpx_prepare_handle_dev(e, k.msgs, 1, k.st, 16, 10, k.groups, 2, 8, nullptr, nullptr,
                                        rep + 4, to, eff, lf, nullptr), MPX_E_INVAL);
        CHECK(strstr(mpx_last_error(e), "aligned"));
    }
    // ---- the encoder
    {
        Out guarded(4096);
        uint8_t* const out = guarded.as<uint8_t>();
        std::vector<uint64_t> off((size_t)N + 1, kOffGuard);
        alignas(16) mpx_prepare_reply_min rm[1] = {{2, 20, 0x20, 19, 1, 10}};
        alignas(16) mpx_prepare_reply rc[1] = {{20, 9, 0, 10}};
        int32_t to[1] = {0}, lf[1] = {18};
        mpx_prepare_reply_batch b{};
        b.replies = min ? (const void*)rm : (const void*)rc, b.reply_to = to, b.log_from = min ? lf : nullptr;
        b.n = 1, b.n_dest = N, b.inst_base = 10, b.n_inst = 16, b.st = k.st, b.inst = k.inst;
        b.src_op = k.sop.data(), b.src_key = k.skey.data(), b.src_val = k.sval.data(), b.n_src = 8;
        auto call = [&](const mpx_prepare_reply_batch& x) {
            return mpx_encode_prepare_replies(e, &x, out, 4096, off.data());
        };
        CHECK(call(b) == MPX_OK);
        off.assign((size_t)N + 1, kOffGuard);
        guarded = Out(4096);
        uint8_t* const o2 = guarded.as<uint8_t>();
        auto call2 = [&](const mpx_prepare_reply_batch& x) {
            return mpx_encode_prepare_replies(e, &x, o2, 4096, off.data());
        };
        FAILS(e, mpx_encode_prepare_replies(e, nullptr, o2, 4096, off.data()), MPX_E_INVAL);
        FAILS(e, mpx_encode_prepare_replies(e, &b, nullptr, 4096, off.data()), MPX_E_INVAL);
        FAILS(e, mpx_encode_prepare_replies(e, &b, o2, 4096, nullptr), MPX_E_INVAL);
        mpx_prepare_reply_batch x = b;
        x.reserved = 1;
        FAILS(e, call2(x), MPX_E_INVAL);
        x = b, x.n_dest = 0;
        FAILS(e, call2(x), MPX_E_INVAL);
        x = b, x.n_dest = MPX_MAX_REPLICAS + 1;
        FAILS(e, call2(x), MPX_E_INVAL);
        x = b, x.n = (size_t)1 << 32;
        FAILS(e, call2(x), MPX_E_UNSUPPORTED);
        x = b, x.replies = nullptr;
        FAILS(e, call2(x), MPX_E_INVAL);
        x = b, x.reply_to = nullptr;
        FAILS(e, call2(x), MPX_E_INVAL);
        to[0] = N;  // reply_to >= n_dest
        FAILS(e, call2(b), MPX_E_INVAL);
        to[0] = 0;
        rm[0].value_id = rc[0].value_id = 16;  // value_id outside the window
        FAILS(e, call2(b), MPX_E_INVAL);
        rm[0].value_id = rc[0].value_id = 10;
        k.inst[10].first_cmd = 8;  // the Command's range leaves the arena
        FAILS(e, call2(b), MPX_E_INVAL);
        k.inst[10].first_cmd = ~0ull;
        FAILS(e, call2(b), MPX_E_INVAL);
        k.inst[10].first_cmd = 5;
        x = b, x.src_val = nullptr;
        FAILS(e, call2(x), MPX_E_INVAL);
        if (min) {
            x = b, x.log_from = nullptr;
            FAILS(e, call2(x), MPX_E_INVAL);
            x = b, x.st = nullptr;
            FAILS(e, call2(x), MPX_E_INVAL);
            x = b, x.inst = nullptr;
            FAILS(e, call2(x), MPX_E_INVAL);
            lf[0] = 9;  // the log range leaves the window at either end
            FAILS(e, call2(b), MPX_E_INVAL);
            lf[0] = 18, rm[0].last_committed = 26;
            FAILS(e, call2(b), MPX_E_INVAL);
            rm[0].last_committed = 19;
            k.st[9].status = MPX_STATUS_NIL;  // a nil instance inside the log range
            FAILS(e, call2(b), MPX_E_NIL_INSTANCE);
            k.st[9].status = MPX_COMMITTED;
            k.inst[8].n_cmds = 9;  // a log instance's range leaves the arena
            FAILS(e, call2(b), MPX_E_INVAL);
            k.inst[8].n_cmds = 1;
        }
        CHECK(guarded.untouched() && off[0] == kOffGuard && off[(size_t)N] == kOffGuard);
        // slots no frame reads are not judged; a skipped reply is not judged either
        k.st[3].status = MPX_STATUS_NIL;
        k.inst[2] = {~0ull, 5, MPX_IC_HAS_CMDS};
        CHECK(call2(b) == MPX_OK && off[(size_t)N] == (min ? min_f1().size() : cl_f1().size()));
        to[0] = -1;
        rm[0].value_id = rc[0].value_id = 99, lf[0] = -100;
        CHECK(call2(b) == MPX_OK && off[(size_t)N] == 0);
        to[0] = 0, rm[0].value_id = rc[0].value_id = 10, lf[0] = 18;
        FAILS(e, mpx_encode_prepare_replies_reserve(e, (size_t)1 << 32, 8, N), MPX_E_UNSUPPORTED);
        FAILS(e, mpx_encode_prepare_replies_reserve(e, 8, ((size_t)1 << 32) + 1, N), MPX_E_UNSUPPORTED);
        FAILS(e, mpx_encode_prepare_replies_reserve(e, 8, 8, 0), MPX_E_INVAL);
        FAILS(e, mpx_encode_prepare_replies_reserve(e, 8, 8, MPX_MAX_REPLICAS + 1), MPX_E_INVAL);
        // the device form: the same shape checks, and the alignments
        CHECK(mpx_encode_prepare_replies_reserve(e, 4, 16, N) == MPX_OK);
        auto dev = [&](const mpx_prepare_reply_batch& y) {
            return mpx_encode_prepare_replies_dev(e, &y, o2, 4096, off.data(), nullptr);
        };
        FAILS(e, mpx_encode_prepare_replies_dev(e, nullptr, o2, 4096, off.data(), nullptr), MPX_E_INVAL);
        FAILS(e, mpx_encode_prepare_replies_dev(e, &b, o2, 4096, nullptr, nullptr), MPX_E_INVAL);
        x = b, x.reserved = 7;
        FAILS(e, dev(x), MPX_E_INVAL);
        x = b, x.st = (const mpx_acceptor_state*)((const char*)k.st + 8);
        FAILS(e, dev(x), MPX_E_INVAL);
        x = b, x.inst = (const mpx_inst_cmds*)((const char*)k.inst + 8);
        FAILS(e, dev(x), MPX_E_INVAL);
        x = b, x.replies = (const char*)b.replies + 4;
        FAILS(e, dev(x), MPX_E_INVAL);
        x = b, x.src_key = (const int64_t*)((const char*)b.src_key + 4);
        FAILS(e, dev(x), MPX_E_INVAL);
        x = b, x.reply_to = (const int32_t*)((const char*)to + 2);
        FAILS(e, dev(x), MPX_E_INVAL);
        FAILS(e, mpx_encode_prepare_replies_dev(e, &b, o2, 4096, (uint64_t*)((char*)off.data() + 4), nullptr),
              MPX_E_INVAL);
        CHECK(strstr(mpx_last_error(e), "aligned"));
    }
    (void)calls;
}

int main() {
    for (int mode : {MPX_MODE_MIN, MPX_MODE_CLASSIC}) {
        const bool min = mode == MPX_MODE_MIN;
        mpx_engine* e = open_engine(mode);
        if (!e) return 1;
        validation(e, mode);
        gather_case(e, mode, false);
        Kat k(mode);
        for (const int spare : {40, 0, -1}) valid_case(e, mode, k, -1, spare, false);
        valid_case(e, mode, k, 0, 40, false);
        valid_case(e, mode, k, 1, 40, false);
        // what the encoder's host form staged for message 1 alone: MIN the span 18 .. 20 and its
        // three referenced commands, CLASSIC the one slot and its one command
        CHECK(ph_stub_seen.n_src == (min ? 3u : 1u) && ph_stub_seen.n_inst == (min ? 3u : 1u));
        CHECK(ph_stub_seen.flagged == (min ? 2u : 1u));
        // a 2^20-entry arena: a referenced range ends exactly at its end
        Kat big(mode, (size_t)1 << 20);
        valid_case(e, mode, big, -1, 40, false);
        CHECK(ph_stub_seen.n_src == (min ? 3u : 1u));  // 51 bytes of commands, not 17 MiB
        CHECK(mpx_close(e) == MPX_OK);
        // the device forms never allocate: on a fresh handle the encoder and the gather need the
        // reserve call first (an empty call does not)
        mpx_engine* f = open_engine(mode);
        if (!f) return 1;
        Out out(4096);
        std::vector<uint64_t> off((size_t)N + 1, kOffGuard);
        alignas(16) mpx_prepare_reply_min rm[1] = {{2, 20, 0x20, 19, 1, MPX_VALUE_KEEP}};
        int32_t to[1] = {0}, lf[1] = {20};
        mpx_prepare_reply_batch b{};
        b.replies = rm, b.reply_to = to, b.log_from = lf, b.n = 1, b.n_dest = N, b.inst_base = 10;
        b.n_inst = 16, b.st = k.st, b.inst = k.inst;
        FAILS(f, mpx_encode_prepare_replies_dev(f, &b, out.as<uint8_t>(), 4096, off.data(), nullptr), MPX_E_INVAL);
        CHECK(strstr(mpx_last_error(f), "mpx_encode_prepare_replies_dev") &&
              strstr(mpx_last_error(f), "mpx_encode_prepare_replies_reserve"));
        CHECK(out.untouched());
        alignas(16) uint8_t buf[16] = {8};
        mpx_peer_frame oth[1] = {{0, MPX_PEER_PREPARE, {0, 0, 0}}};
        alignas(16) mpx_prepare_msg m[1];
        uint32_t idx[1];
        uint64_t cnt = 0;
        FAILS(f, mpx_gather_prepares_dev(f, buf, 16, oth, 1, nullptr, 0, m, idx, 1, &cnt, nullptr), MPX_E_INVAL);
        CHECK(strstr(mpx_last_error(f), "mpx_encode_prepare_replies_reserve"));
        b.n = 0;
        CHECK(mpx_encode_prepare_replies_dev(f, &b, out.as<uint8_t>(), 4096, off.data(), nullptr) == MPX_OK);
        gather_case(f, mode, true);
        valid_case(f, mode, k, -1, 40, true);
        valid_case(f, mode, k, -1, -1, true);  // (never writes at or past out_cap)
        CHECK(ph_stub_seen.n_src == 8 && ph_stub_seen.n_inst == 16);  // nothing is staged
        CHECK(mpx_close(f) == MPX_OK);
    }
    CHECK(mpx_gather_prepares(nullptr, nullptr, 0, nullptr, 0, 0, nullptr, nullptr, 0, nullptr) == MPX_E_INVAL);
    CHECK(mpx_prepare_handle(nullptr, nullptr, 0, nullptr, 0, 0, nullptr, 0, 0, nullptr, nullptr, nullptr,
                             nullptr, nullptr, nullptr) == MPX_E_INVAL);
    CHECK(mpx_encode_prepare_replies(nullptr, nullptr, nullptr, 0, nullptr) == MPX_E_INVAL);
    CHECK(mpx_encode_prepare_replies_reserve(nullptr, 1, 1, 1) == MPX_E_INVAL);
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("prepare_handle_driver: all checks passed\n");
    return failures ? 1 : 0;
}
