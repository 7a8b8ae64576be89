// tests/san/proposer_driver.cpp — TEST INFRASTRUCTURE ONLY: drives the proposer entry points
// (mpx_propose_handle, mpx_encode_accepts and their _reserve / _dev forms) of the CPU build of
// engine.cpp over the stub runtime (hip_stub.cpp) under ASan + UBSan. Every argument-validation
// path must answer its code (MPX_E_INVAL, MPX_E_NIL_INSTANCE, MPX_E_UNSUPPORTED for a size limit)
// before anything is staged; a valid call answers MPX_OK and, over the stub's stand-ins for the
// proposer launchers, stages its arrays whole and apart (the staging checks of san_check.hpp).
// Exit status 0 = all checks passed.
#include "san_check.hpp"

constexpr uint64_t kOffGuard = 0x5C5C5C5C5C5C5C5Cull;
constexpr size_t kStubAcceptFrame = 24;  // the stub's Accept frame (hip_stub.cpp, stub_frames)

static mpx_engine* open_engine(int32_t N, int mode) {
    mpx_engine* e = nullptr;
    mpx_config cfg{N, mode, 1 << 10, 0, 0, 0};
    CHECK(mpx_open(0, &cfg, &e) == MPX_OK && e);
    return e;
}

// a valid mpx_propose_handle call of G groups of ipg on guarded buffers; every group brings 3
// proposals and the last 5003, so send_off[g] = g and send_off[G] = G + 1. groups, st and lb (when
// given) are updated in place, sends is the output (one slot per send_off[G] of its sends_cap) and
// send_off is the host's
static void propose_case(mpx_engine* e, const mpx_proposer_group* g, size_t G, uint32_t ipg,
                         bool with_lb, size_t sends_cap, bool dev) {
    std::vector<uint64_t> off(G + 1), soff_dev(G + 1), soff(G + 2, kOffGuard);
    for (size_t i = 0; i <= G; ++i) off[i] = 3 * i + (i == G ? 5000 : 0), soff_dev[i] = i + (i == G);
    const size_t n_inst = G * ipg;
    In grp = holding(g, G, 1), poff = holding(off.data(), G + 1, 2),
       st(n_inst * sizeof(mpx_acceptor_state), 3), lb(n_inst * sizeof(mpx_inst_state), 4);
    Out snd(sends_cap * sizeof(mpx_accept_send));
    mpx_inst_state* plb = with_lb ? lb.as<mpx_inst_state>() : nullptr;
    if (dev) {
        CHECK(mpx_propose_handle_dev(e, grp.as<mpx_proposer_group>(), G, poff.as<uint64_t>(),
                                     soff_dev.data(), st.as<mpx_acceptor_state>(), plb, n_inst, 100,
                                     ipg, snd.as<mpx_accept_send>(), nullptr) == MPX_OK);
    } else {
        CHECK(mpx_propose_handle(e, grp.as<mpx_proposer_group>(), G, poff.as<uint64_t>(),
                                 st.as<mpx_acceptor_state>(), plb, n_inst, 100, ipg, soff.data(),
                                 snd.as<mpx_accept_send>(), sends_cap) == MPX_OK);
        for (size_t i = 0; i <= G; ++i) CHECK(soff[i] == soff_dev[i]);
        CHECK(soff[G + 1] == kOffGuard);
    }
    CHECK(grp.flipped() && poff.intact() && st.flipped() && (with_lb ? lb.flipped() : lb.intact()));
    CHECK(snd.is(0, (G + 1) * sizeof(mpx_accept_send)));
}

static void propose(mpx_engine* e) {
    const int32_t base = 100;
    const uint32_t ipg = 4;
    // (default_ballot, self_id, leader, prepare_oks, crt_instance, committed_upto)
    mpx_proposer_group g[2] = {{17, 1, 1, 3, 100, 99, {0, 0}}, {17, 1, 1, 3, 104, 103, {0, 0}}};
    uint64_t poff[3] = {0, 2, 5003};
    std::vector<mpx_acceptor_state> st(8, mpx_acceptor_state{MPX_STATUS_NIL, 0, 0, 0});
    std::vector<mpx_inst_state> lb(8);
    uint64_t soff[3] = {9, 9, 9};
    mpx_accept_send sends[3];
    memset(sends, 0x5C, sizeof(sends));
    // null arguments
    FAILS(e, mpx_propose_handle(e, nullptr, 2, poff, st.data(), lb.data(), 8, base, ipg, soff, sends, 3), MPX_E_INVAL);
    FAILS(e, mpx_propose_handle(e, g, 2, nullptr, st.data(), lb.data(), 8, base, ipg, soff, sends, 3), MPX_E_INVAL);
    FAILS(e, mpx_propose_handle(e, g, 2, poff, nullptr, lb.data(), 8, base, ipg, soff, sends, 3), MPX_E_INVAL);
    FAILS(e, mpx_propose_handle(e, g, 2, poff, st.data(), lb.data(), 8, base, ipg, nullptr, sends, 3), MPX_E_INVAL);
    FAILS(e, mpx_propose_handle(e, g, 2, poff, st.data(), lb.data(), 8, base, ipg, soff, nullptr, 3), MPX_E_INVAL);
    // the window's shape
    FAILS(e, mpx_propose_handle(e, g, 2, poff, st.data(), lb.data(), 7, base, ipg, soff, sends, 3), MPX_E_INVAL);
    FAILS(e, mpx_propose_handle(e, g, 2, poff, st.data(), lb.data(), 8, base, 0, soff, sends, 3), MPX_E_INVAL);
    FAILS(e, mpx_propose_handle(e, g, 0, poff, st.data(), lb.data(), 8, base, ipg, soff, sends, 3), MPX_E_INVAL);
    // the offsets: decreasing, and more slots than sends_cap (send_off is complete by then)
    uint64_t bad_off[3] = {0, 5, 4};
    FAILS(e, mpx_propose_handle(e, g, 2, bad_off, st.data(), lb.data(), 8, base, ipg, soff, sends, 3), MPX_E_INVAL);
    FAILS(e, mpx_propose_handle(e, g, 2, poff, st.data(), lb.data(), 8, base, ipg, soff, sends, 2), MPX_E_INVAL);
    CHECK(soff[0] == 0 && soff[1] == 1 && soff[2] == 3);
    // a leader with proposals whose crtInstance is outside its window: the index panic
    g[1].crt_instance = 108;
    FAILS(e, mpx_propose_handle(e, g, 2, poff, st.data(), lb.data(), 8, base, ipg, soff, sends, 3), MPX_E_NIL_INSTANCE);
    g[1].crt_instance = 103;
    FAILS(e, mpx_propose_handle(e, g, 2, poff, st.data(), lb.data(), 8, base, ipg, soff, sends, 3), MPX_E_NIL_INSTANCE);
    g[1].crt_instance = 104;
    // the device form validates the same shape
    FAILS(e, mpx_propose_handle_dev(e, nullptr, 2, poff, soff, st.data(), nullptr, 8, base, ipg, sends, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_propose_handle_dev(e, g, 2, poff, soff, st.data(), nullptr, 9, base, ipg, sends, nullptr), MPX_E_INVAL);
    // nothing was touched
    CHECK(g[0].crt_instance == 100 && st[0].status == MPX_STATUS_NIL && lb[0].status == 0);
    CHECK(sends[0].instance == 0x5C5C5C5C && sends[2].pad == 0x5C5C5C5Cu);
    // valid calls: with and without lb, a sends array larger than the slots, the device form
    propose_case(e, g, 2, ipg, true, 3, false);
    propose_case(e, g, 2, ipg, false, 3, false);
    propose_case(e, g, 2, ipg, true, 5, false);
    propose_case(e, g, 2, ipg, false, 3, true);
    propose_case(e, g, 2, ipg, true, 3, true);
    // ... and of a size at which every array has a slot of more than one 256-byte unit
    std::vector<mpx_proposer_group> big(40);
    for (int32_t i = 0; i < 40; ++i) big[i] = {17, 1, 1, 3, base + 16 * i, base + 16 * i - 1, {0, 0}};
    propose_case(e, big.data(), 40, 16, true, 41, false);
    propose_case(e, big.data(), 40, 16, false, 64, false);
    propose_case(e, big.data(), 40, 16, true, 41, true);
    // a crtInstance outside the window is never indexed by a follower
    g[1].crt_instance = 103;
    g[1].leader = 0;
    propose_case(e, g, 2, ipg, true, 3, false);
    // no group at all: send_off[0] is still written
    uint64_t none[2] = {7, kOffGuard};
    CHECK(mpx_propose_handle(e, nullptr, 0, nullptr, nullptr, nullptr, 0, base, ipg, none, nullptr, 0) == MPX_OK);
    CHECK(none[0] == 0 && none[1] == kOffGuard);
    CHECK(mpx_propose_handle_dev(e, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, base, ipg, nullptr, nullptr) == MPX_OK);
}

// The valid batch of encode() on guarded buffers, its two sends repeated up to n_sends (every
// other one carries MPX_PH_ACCEPT and puts one stub frame in every destination's run): the inputs
// come back intact, dest_off holds the stub's offsets and out its pattern over dest_off[N] bytes.
// spare: out_cap - dest_off[N]; below 0 the call answers MPX_E_INVAL with dest_off written and
// out untouched. cmds: with the command arrays, else the sends carry none and they are absent (in
// CLASSIC the log is absent too).
static void encode_case(mpx_engine* e, int mode, int32_t N, const mpx_accept_batch& b0, bool cmds,
                        size_t n_sends, int spare, bool dev) {
    const bool min = mode == MPX_MODE_MIN;
    const size_t n_inst = b0.n_groups * b0.ipg, flagged = (n_sends + 1) / 2;
    const size_t total = (size_t)N * flagged * kStubAcceptFrame, out_cap = total + spare;
    std::vector<mpx_accept_send> sv(n_sends);
    for (size_t i = 0; i < n_sends; ++i) {
        sv[i] = b0.sends[i & 1];
        if (!cmds) sv[i].n_cmds = 0;
    }
    const size_t m = cmds ? 100 : 0;  // (the sends name the first two; the values are not looked at)
    In snd = holding(sv.data(), n_sends, 1), grp = holding(b0.groups, b0.n_groups, 2),
       pc = holding(b0.peer_commits, b0.n_groups * N, 3), op(m, 4), key(m * 8, 5), val(m * 8, 6),
       lrec = holding(b0.log_recs, n_inst, 7), lcoff = holding(b0.log_cmd_off, n_inst + 1, 8),
       lop = holding(b0.log_op, b0.n_log_cmds, 9), lkey = holding(b0.log_key, b0.n_log_cmds, 10),
       lval = holding(b0.log_val, b0.n_log_cmds, 11);
    mpx_accept_batch b = b0;
    b.sends = snd.as<mpx_accept_send>();
    b.n_sends = n_sends;
    b.groups = grp.as<mpx_proposer_group>();
    b.peer_commits = pc.as<int32_t>();
    b.cmd_op = cmds ? op.as<uint8_t>() : nullptr;
    b.cmd_key = cmds ? key.as<int64_t>() : nullptr;
    b.cmd_val = cmds ? val.as<int64_t>() : nullptr;
    b.n_cmds = m;
    const bool log = min || cmds;
    b.log_recs = log ? lrec.as<mpx_log_rec>() : nullptr;
    b.log_cmd_off = log ? lcoff.as<uint64_t>() : nullptr;
    b.log_op = log ? lop.as<uint8_t>() : nullptr;
    b.log_key = log ? lkey.as<int64_t>() : nullptr;
    b.log_val = log ? lval.as<int64_t>() : nullptr;
    if (!log) b.peer_commits = nullptr, b.n_log_cmds = 0;
    Out out(spare < 0 ? total : out_cap);
    std::vector<uint64_t> off((size_t)N + 2, kOffGuard);
    const int rc = dev ? mpx_encode_accepts_dev(e, &b, out.as<uint8_t>(), out_cap, off.data(), nullptr)
                       : mpx_encode_accepts(e, &b, out.as<uint8_t>(), out_cap, off.data());
    if (spare < 0 && !dev) {  // (the device form leaves the comparison to its caller)
        CHECK(rc == MPX_E_INVAL && strstr(mpx_last_error(e), "out_cap"));
        CHECK(out.untouched());
    } else {
        CHECK(rc == MPX_OK);
        CHECK(out.is(0, total < out_cap ? total : out_cap));
    }
    for (int32_t q = 0; q <= N; ++q) CHECK(off[q] == (uint64_t)q * flagged * kStubAcceptFrame);
    CHECK(off[(size_t)N + 1] == kOffGuard);
    CHECK(snd.intact() && grp.intact() && pc.intact() && op.intact() && key.intact() && val.intact());
    CHECK(lrec.intact() && lcoff.intact() && lop.intact() && lkey.intact() && lval.intact());
}

static void encode(mpx_engine* e, int mode, int32_t N) {
    const bool min = mode == MPX_MODE_MIN;
    mpx_proposer_group g[2] = {{32, 0, 0, 3, 103, 101, {0, 0}}, {32, 1, 1, 3, 105, 103, {0, 0}}};
    // window: base 100, two groups of 4; group 0's log holds 100, 101; 102.. are nil
    std::vector<mpx_log_rec> lrec(8, mpx_log_rec{0, MPX_STATUS_NIL, 0, 0});
    lrec[0] = mpx_log_rec{5, MPX_COMMITTED, 0, 0};
    lrec[1] = mpx_log_rec{6, MPX_COMMITTED, 0, 0};
    uint64_t lcoff[9] = {0, 1, 1, 1, 1, 1, 1, 1, 1};
    uint8_t lop[1] = {1}, op[2] = {1, 2};
    int64_t lkey[1] = {2}, lval[1] = {3}, key[2] = {10, 11}, val[2] = {20, 21};
    std::vector<int32_t> pc(2 * (size_t)N, 99);
    mpx_accept_send sends[2] = {{102, 32, 101, MPX_PH_ACCEPT, 0, 2, 0},
                                {-1, 0, 0, MPX_PH_NOT_LEADER, 0, 2, 0}};
    mpx_accept_batch b{};
    b.sends = sends;
    b.n_sends = 2;
    b.inst_base = 100;
    b.ipg = 4;
    b.n_groups = 2;
    b.groups = g;
    b.peer_commits = pc.data();
    b.cmd_op = op;
    b.cmd_key = key;
    b.cmd_val = val;
    b.n_cmds = 2;
    b.log_recs = lrec.data();
    b.log_cmd_off = lcoff;
    b.log_op = lop;
    b.log_key = lkey;
    b.log_val = lval;
    b.n_log_cmds = 1;
    b.alive_mask = 0xFFFF;
    Out guarded(4096);
    uint8_t* const out = guarded.as<uint8_t>();
    const size_t out_size = 4096;
    std::vector<uint64_t> off((size_t)N + 1, kOffGuard);
    auto call = [&](const mpx_accept_batch& x) {
        return mpx_encode_accepts(e, &x, out, out_size, off.data());
    };
    FAILS(e, mpx_encode_accepts(e, nullptr, out, out_size, off.data()), MPX_E_INVAL);
    FAILS(e, mpx_encode_accepts(e, &b, nullptr, out_size, off.data()), MPX_E_INVAL);
    FAILS(e, mpx_encode_accepts(e, &b, out, out_size, nullptr), MPX_E_INVAL);
    mpx_accept_batch x = b;
    x.sends = nullptr;
    FAILS(e, call(x), MPX_E_INVAL);
    x = b;
    x.groups = nullptr;
    FAILS(e, call(x), MPX_E_INVAL);
    x = b;
    x.ipg = 0;
    FAILS(e, call(x), MPX_E_INVAL);
    x = b;
    x.n_groups = 0;
    FAILS(e, call(x), MPX_E_INVAL);
    x = b;
    x.cmd_key = nullptr;
    FAILS(e, call(x), MPX_E_INVAL);
    // a send outside the window, commands outside the arrays, self_id outside [0, N)
    sends[0].instance = 108;
    FAILS(e, call(b), MPX_E_INVAL);
    sends[0].instance = 99;
    FAILS(e, call(b), MPX_E_INVAL);
    sends[0].instance = 102;
    sends[0].first_cmd = 1;
    FAILS(e, call(b), MPX_E_INVAL);
    sends[0].first_cmd = ~0ull;
    FAILS(e, call(b), MPX_E_INVAL);
    sends[0].first_cmd = 0;
    g[0].self_id = N;
    FAILS(e, call(b), MPX_E_INVAL);
    g[0].self_id = -1;
    FAILS(e, call(b), MPX_E_INVAL);
    g[0].self_id = 0;
    if (min) {
        x = b;
        x.peer_commits = nullptr;
        FAILS(e, call(x), MPX_E_INVAL);
        x = b;
        x.log_recs = nullptr;
        FAILS(e, call(x), MPX_E_INVAL);
        x = b;
        x.log_cmd_off = nullptr;
        FAILS(e, call(x), MPX_E_INVAL);
        x = b;
        x.log_op = nullptr;
        FAILS(e, call(x), MPX_E_INVAL);
        // last_committed >= instance, and below first_g - 1
        sends[0].last_committed = 102;
        FAILS(e, call(b), MPX_E_INVAL);
        sends[0].last_committed = 98;
        FAILS(e, call(b), MPX_E_INVAL);
        sends[0].last_committed = 101;
        // the log's offsets
        lcoff[3] = 0;
        FAILS(e, call(b), MPX_E_INVAL);
        lcoff[3] = 1;
        lcoff[8] = 2;
        FAILS(e, call(b), MPX_E_INVAL);
        lcoff[8] = 1;
        // a nil instance inside a catch-up range: 101 is nil, peers are at 99 / 100
        lrec[1].status = MPX_STATUS_NIL;
        FAILS(e, call(b), MPX_E_NIL_INSTANCE);
    }
    FAILS(e, mpx_encode_accepts_reserve(e, (size_t)1 << 32, 8, 1), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_encode_accepts_dev(e, nullptr, out, out_size, off.data(), nullptr), MPX_E_INVAL);
    FAILS(e, mpx_encode_accepts_dev(e, &b, out, out_size, nullptr, nullptr), MPX_E_INVAL);
    x = b;
    x.ipg = 0;
    FAILS(e, mpx_encode_accepts_dev(e, &x, out, out_size, off.data(), nullptr), MPX_E_INVAL);
    // nothing was touched
    CHECK(guarded.untouched() && off[0] == kOffGuard && off[(size_t)N] == kOffGuard);
    if (min) {
        for (auto& v : pc) v = 101;  // a nil instance in the log, but no peer needs it
        CHECK(call(b) == MPX_OK);
        for (auto& v : pc) v = 99;
        sends[0].flags = MPX_PH_REFUSED;  // ... or the slot is skipped
        CHECK(call(b) == MPX_OK && off[(size_t)N] == 0);
        sends[0].flags = MPX_PH_ACCEPT;
        lrec[1].status = MPX_COMMITTED;
    }
    // valid calls
    CHECK(call(b) == MPX_OK && off[(size_t)N] == (size_t)N * kStubAcceptFrame);
    x = b;
    x.flags = MPX_AB_THRIFTY;
    x.alive_mask = 0;
    CHECK(call(x) == MPX_OK);
    x = b;
    x.n_sends = 0;
    CHECK(call(x) == MPX_OK && off[(size_t)N] == 0);
    // ... on guarded buffers: with and without commands, an out_cap with room to spare, one that
    // just fits, one that is a byte short, and the empty batch
    for (const bool cmds : {true, false}) {
        encode_case(e, mode, N, b, cmds, 2, 40, false);
        encode_case(e, mode, N, b, cmds, 75, 40, false);
        encode_case(e, mode, N, b, cmds, 75, 0, false);
        encode_case(e, mode, N, b, cmds, 75, -1, false);
        encode_case(e, mode, N, b, cmds, 2, -1, false);
        encode_case(e, mode, N, b, cmds, 0, 40, false);
        encode_case(e, mode, N, b, cmds, 0, 0, false);
    }
    // the device form never allocates: on a fresh handle it needs its reserve call first (an empty
    // call does not)
    mpx_engine* f = open_engine(N, mode);
    if (!f) return;
    FAILS(f, mpx_encode_accepts_dev(f, &b, out, out_size, off.data(), nullptr), MPX_E_INVAL);
    CHECK(strstr(mpx_last_error(f), "mpx_encode_accepts_dev") && strstr(mpx_last_error(f), "mpx_encode_accepts_reserve"));
    encode_case(f, mode, N, b, true, 0, 40, true);
    CHECK(mpx_encode_accepts_reserve(f, 16, 8, 1) == MPX_OK);
    encode_case(f, mode, N, b, true, 16, 40, true);
    encode_case(f, mode, N, b, false, 16, -1, true);  // (never writes at or past out_cap)
    CHECK(mpx_close(f) == MPX_OK);
}

int main() {
    for (int mode : {MPX_MODE_MIN, MPX_MODE_CLASSIC}) {
        for (int32_t N : {1, 3, 5}) {
            mpx_engine* e = open_engine(N, mode);
            if (!e) return 1;
            propose(e);
            if (N > 1) encode(e, mode, N);
            CHECK(mpx_close(e) == MPX_OK);
        }
    }
    CHECK(mpx_propose_handle(nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 0, 0, nullptr, nullptr, 0) == MPX_E_INVAL);
    CHECK(mpx_encode_accepts(nullptr, nullptr, nullptr, 0, nullptr) == MPX_E_INVAL);
    CHECK(mpx_encode_accepts_reserve(nullptr, 1, 1, 1) == MPX_E_INVAL);
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("proposer_driver: all checks passed\n");
    return failures ? 1 : 0;
}
