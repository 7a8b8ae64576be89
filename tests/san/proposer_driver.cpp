// tests/san/proposer_driver.cpp — TEST INFRASTRUCTURE ONLY: drives the proposer entry points
// (mpx_propose_handle, mpx_encode_accepts and their _reserve / _dev forms) of the CPU build of
// engine.cpp over the stub runtime (hip_stub.cpp) under ASan + UBSan. The stub has no stand-ins
// for the proposer launchers, so the weak symbols stay null: every argument-validation path must
// answer before that is looked at (MPX_E_INVAL, MPX_E_NIL_INSTANCE), and a valid call answers
// MPX_E_UNSUPPORTED. Exit status 0 = all checks passed.
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

static void propose(mpx_engine* e, int mode) {
    const int32_t base = 100;
    const uint32_t ipg = 4;
    // (default_ballot, self_id, leader, prepare_oks, crt_instance, committed_upto)
    mpx_proposer_group g[2] = {{17, 1, 1, 3, 100, 99, {0, 0}}, {17, 1, 1, 3, 104, 103, {0, 0}}};
    uint64_t poff[3] = {0, 2, 5003};
    std::vector<mpx_acceptor_state> st(8, mpx_acceptor_state{MPX_STATUS_NIL, 0, 0, 0});
    std::vector<mpx_inst_state> lb(8);
    uint64_t soff[3] = {9, 9, 9};
    mpx_accept_send sends[3];
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
    // ... which a follower, or a leader without proposals, never indexes
    g[1].leader = 0;
    FAILS(e, mpx_propose_handle(e, g, 2, poff, st.data(), lb.data(), 8, base, ipg, soff, sends, 3), MPX_E_UNSUPPORTED);
    g[1].leader = 1;
    g[1].crt_instance = 104;
    // valid calls: the kernels are not in this build
    FAILS(e, mpx_propose_handle(e, g, 2, poff, st.data(), lb.data(), 8, base, ipg, soff, sends, 3), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_propose_handle(e, g, 2, poff, st.data(), nullptr, 8, base, ipg, soff, sends, 3), MPX_E_UNSUPPORTED);
    uint64_t none[1] = {7};
    FAILS(e, mpx_propose_handle(e, nullptr, 0, nullptr, nullptr, nullptr, 0, base, ipg, none, nullptr, 0), MPX_E_UNSUPPORTED);
    CHECK(none[0] == 0);
    CHECK(g[0].crt_instance == 100 && st[0].status == MPX_STATUS_NIL);  // nothing was touched
    // the device form validates the same shape
    FAILS(e, mpx_propose_handle_dev(e, nullptr, 2, poff, soff, st.data(), nullptr, 8, base, ipg, sends, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_propose_handle_dev(e, g, 2, poff, soff, st.data(), nullptr, 9, base, ipg, sends, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_propose_handle_dev(e, g, 2, poff, soff, st.data(), nullptr, 8, base, ipg, sends, nullptr), MPX_E_UNSUPPORTED);
    (void)mode;
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
    std::vector<uint8_t> out(4096);
    std::vector<uint64_t> off((size_t)N + 1);
    auto call = [&](const mpx_accept_batch& x) {
        return mpx_encode_accepts(e, &x, out.data(), out.size(), off.data());
    };
    FAILS(e, mpx_encode_accepts(e, nullptr, out.data(), out.size(), off.data()), MPX_E_INVAL);
    FAILS(e, mpx_encode_accepts(e, &b, nullptr, out.size(), off.data()), MPX_E_INVAL);
    FAILS(e, mpx_encode_accepts(e, &b, out.data(), out.size(), nullptr), MPX_E_INVAL);
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
        for (auto& v : pc) v = 101;  // ... but not when no peer needs it
        FAILS(e, call(b), MPX_E_UNSUPPORTED);
        for (auto& v : pc) v = 99;
        sends[0].flags = MPX_PH_REFUSED;  // ... or when the slot is skipped
        FAILS(e, call(b), MPX_E_UNSUPPORTED);
        sends[0].flags = MPX_PH_ACCEPT;
        lrec[1].status = MPX_COMMITTED;
    }
    // valid calls
    FAILS(e, call(b), MPX_E_UNSUPPORTED);
    x = b;
    x.flags = MPX_AB_THRIFTY;
    x.alive_mask = 0;
    FAILS(e, call(x), MPX_E_UNSUPPORTED);
    x = b;
    x.n_sends = 0;
    FAILS(e, call(x), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_encode_accepts_reserve(e, 16, 8, 1), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_encode_accepts_dev(e, nullptr, out.data(), out.size(), off.data(), nullptr), MPX_E_INVAL);
    FAILS(e, mpx_encode_accepts_dev(e, &b, out.data(), out.size(), nullptr, nullptr), MPX_E_INVAL);
    x = b;
    x.ipg = 0;
    FAILS(e, mpx_encode_accepts_dev(e, &x, out.data(), out.size(), off.data(), nullptr), MPX_E_INVAL);
    FAILS(e, mpx_encode_accepts_dev(e, &b, out.data(), out.size(), off.data(), nullptr), MPX_E_UNSUPPORTED);
}

int main() {
    for (int mode : {MPX_MODE_MIN, MPX_MODE_CLASSIC}) {
        for (int32_t N : {1, 3, 5}) {
            mpx_engine* e = nullptr;
            mpx_config cfg{N, mode, 1 << 10, 0, 0, 0};
            CHECK(mpx_open(0, &cfg, &e) == MPX_OK && e);
            if (!e) return 1;
            propose(e, mode);
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
