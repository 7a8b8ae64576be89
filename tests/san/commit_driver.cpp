// tests/san/commit_driver.cpp — TEST INFRASTRUCTURE ONLY: drives the commit entry points
// (mpx_commit_handle, mpx_encode_commits, mpx_gather_commit_shorts and their _reserve / _dev
// forms) of the CPU build of engine.cpp over the stub runtime (hip_stub.cpp) under ASan + UBSan.
// The stub has no stand-ins for the commit launchers, so the weak symbols stay null: every
// argument-validation path must answer before that is looked at (MPX_E_INVAL), and a valid call
// answers MPX_E_UNSUPPORTED. Exit status 0 = all checks passed.
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

static void handle(mpx_engine* e) {
    const int32_t base = 100;
    const uint32_t ipg = 4;
    mpx_accept_msg msgs[3] = {{100, 17, 1, 5}, {101, 17, 1, MPX_VALUE_KEEP}, {105, 18, 1, 6}};
    std::vector<mpx_acceptor_state> st(8, mpx_acceptor_state{MPX_STATUS_NIL, 0, 0, 0});
    int32_t cu[2] = {99, 103};
    uint8_t eff[3] = {9, 9, 9};
    mpx_log_rec log[3];
    // null arguments
    FAILS(e, mpx_commit_handle(e, nullptr, 3, st.data(), 8, base, cu, 2, ipg, eff, log), MPX_E_INVAL);
    FAILS(e, mpx_commit_handle(e, msgs, 3, nullptr, 8, base, cu, 2, ipg, eff, log), MPX_E_INVAL);
    FAILS(e, mpx_commit_handle(e, msgs, 3, st.data(), 8, base, nullptr, 2, ipg, eff, log), MPX_E_INVAL);
    FAILS(e, mpx_commit_handle(e, msgs, 3, st.data(), 8, base, cu, 2, ipg, nullptr, log), MPX_E_INVAL);
    // the window's shape
    FAILS(e, mpx_commit_handle(e, msgs, 3, st.data(), 7, base, cu, 2, ipg, eff, log), MPX_E_INVAL);
    FAILS(e, mpx_commit_handle(e, msgs, 3, st.data(), 8, base, cu, 2, 0, eff, log), MPX_E_INVAL);
    FAILS(e, mpx_commit_handle(e, msgs, 3, st.data(), 8, base, cu, 0, ipg, eff, log), MPX_E_INVAL);
    // committed_upto outside [first_g - 1, first_g + ipg - 1], below and above, in either group
    for (int g = 0; g < 2; ++g)
        for (const int32_t bad : {base + 4 * g - 2, base + 4 * g + 4}) {
            const int32_t keep = cu[g];
            cu[g] = bad;
            FAILS(e, mpx_commit_handle(e, msgs, 3, st.data(), 8, base, cu, 2, ipg, eff, log), MPX_E_INVAL);
            cu[g] = keep;
        }
    // ... and its two ends are legal
    cu[0] = base + 3;
    FAILS(e, mpx_commit_handle(e, msgs, 3, st.data(), 8, base, cu, 2, ipg, eff, log), MPX_E_UNSUPPORTED);
    cu[0] = 99;
    // valid calls: the kernels are not in this build
    FAILS(e, mpx_commit_handle(e, msgs, 3, st.data(), 8, base, cu, 2, ipg, eff, log), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_commit_handle(e, msgs, 3, st.data(), 8, base, cu, 2, ipg, eff, nullptr), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_commit_handle(e, nullptr, 0, st.data(), 8, base, cu, 2, ipg, nullptr, nullptr), MPX_E_UNSUPPORTED);
    CHECK(st[0].status == MPX_STATUS_NIL && cu[0] == 99 && eff[0] == 9);  // nothing was touched
    // the device form validates the same shape
    FAILS(e, mpx_commit_handle_dev(e, nullptr, 3, st.data(), 8, base, cu, 2, ipg, eff, log, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_commit_handle_dev(e, msgs, 3, nullptr, 8, base, cu, 2, ipg, eff, log, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_commit_handle_dev(e, msgs, 3, st.data(), 9, base, cu, 2, ipg, eff, log, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_commit_handle_dev(e, msgs, 3, st.data(), 8, base, cu, 2, ipg, eff, nullptr, nullptr), MPX_E_UNSUPPORTED);
}

static void encode(mpx_engine* e, int32_t N) {
    mpx_proposer_group g[2] = {{32, 0, 0, 3, 103, 101, {0, 0}}, {32, N - 1, N - 1, 3, 105, 103, {0, 0}}};
    uint8_t op[3] = {1, 2, 3};
    int64_t key[3] = {10, 11, 12}, val[3] = {20, 21, 22};
    mpx_commit_send sends[3] = {{101, 32, 0, 2, MPX_CS_SEND, {0, 0}},
                                {102, 32, 2, 0, 0, {0, 0}},
                                {105, 33, 2, 1, MPX_CS_SEND, {0, 0}}};
    mpx_commit_batch b{};
    b.sends = sends;
    b.n_sends = 3;
    b.inst_base = 100;
    b.ipg = 4;
    b.n_groups = 2;
    b.groups = g;
    b.cmd_op = op;
    b.cmd_key = key;
    b.cmd_val = val;
    b.n_cmds = 3;
    b.alive_mask = 0xFFFF;
    std::vector<uint8_t> out(4096);
    std::vector<uint64_t> off((size_t)N + 1);
    auto call = [&](const mpx_commit_batch& x) {
        return mpx_encode_commits(e, &x, out.data(), out.size(), off.data());
    };
    FAILS(e, mpx_encode_commits(e, nullptr, out.data(), out.size(), off.data()), MPX_E_INVAL);
    FAILS(e, mpx_encode_commits(e, &b, nullptr, out.size(), off.data()), MPX_E_INVAL);
    FAILS(e, mpx_encode_commits(e, &b, out.data(), out.size(), nullptr), MPX_E_INVAL);
    mpx_commit_batch x = b;
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
    sends[0].instance = 101;
    sends[0].first_cmd = 2;
    FAILS(e, call(b), MPX_E_INVAL);
    sends[0].first_cmd = ~0ull;
    FAILS(e, call(b), MPX_E_INVAL);
    sends[0].first_cmd = 0;
    sends[2].n_cmds = 2;
    FAILS(e, call(b), MPX_E_INVAL);
    sends[2].n_cmds = 1;
    g[0].self_id = N;
    FAILS(e, call(b), MPX_E_INVAL);
    g[0].self_id = -1;
    FAILS(e, call(b), MPX_E_INVAL);
    g[0].self_id = 0;
    // ... none of which counts on a skipped slot
    sends[1].instance = 7;
    sends[1].first_cmd = 99;
    FAILS(e, call(b), MPX_E_UNSUPPORTED);
    // valid calls
    x = b;
    x.flags = MPX_AB_THRIFTY;
    x.alive_mask = 0;
    FAILS(e, call(x), MPX_E_UNSUPPORTED);
    x = b;
    x.n_sends = 0;
    FAILS(e, call(x), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_encode_commits_reserve(e, 16, 8), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_encode_commits_dev(e, nullptr, out.data(), out.size(), off.data(), nullptr), MPX_E_INVAL);
    FAILS(e, mpx_encode_commits_dev(e, &b, out.data(), out.size(), nullptr, nullptr), MPX_E_INVAL);
    x = b;
    x.ipg = 0;
    FAILS(e, mpx_encode_commits_dev(e, &x, out.data(), out.size(), off.data(), nullptr), MPX_E_INVAL);
    FAILS(e, mpx_encode_commits_dev(e, &b, out.data(), out.size(), off.data(), nullptr), MPX_E_UNSUPPORTED);
}

static void gather(mpx_engine* e) {
    alignas(16) uint8_t buf[64] = {0};
    buf[0] = MPX_PEER_BEACON;
    buf[9] = MPX_PEER_COMMIT_SHORT;
    buf[26] = MPX_PEER_COMMIT_SHORT;
    mpx_peer_frame oth[3] = {{0, MPX_PEER_BEACON, {0, 0, 0}},
                             {9, MPX_PEER_COMMIT_SHORT, {0, 0, 0}},
                             {26, MPX_PEER_COMMIT_SHORT, {0, 0, 0}}};
    mpx_accept_msg msgs[2];
    int32_t cnt[2];
    uint32_t idx[2];
    uint64_t ns = 77;
    FAILS(e, mpx_gather_commit_shorts(e, nullptr, 43, oth, 3, msgs, cnt, idx, 2, &ns), MPX_E_INVAL);
    FAILS(e, mpx_gather_commit_shorts(e, buf, 43, nullptr, 3, msgs, cnt, idx, 2, &ns), MPX_E_INVAL);
    FAILS(e, mpx_gather_commit_shorts(e, buf, 43, oth, 3, nullptr, cnt, idx, 2, &ns), MPX_E_INVAL);
    FAILS(e, mpx_gather_commit_shorts(e, buf, 43, oth, 3, msgs, nullptr, idx, 2, &ns), MPX_E_INVAL);
    FAILS(e, mpx_gather_commit_shorts(e, buf, 43, oth, 3, msgs, cnt, nullptr, 2, &ns), MPX_E_INVAL);
    FAILS(e, mpx_gather_commit_shorts(e, buf, 43, oth, 3, msgs, cnt, idx, 2, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_gather_commit_shorts(e, buf, 0, oth, 3, msgs, cnt, idx, 2, &ns), MPX_E_INVAL);
    // a CommitShort that runs past the buffer, by one byte and by its whole body
    FAILS(e, mpx_gather_commit_shorts(e, buf, 42, oth, 3, msgs, cnt, idx, 2, &ns), MPX_E_INVAL);
    oth[2].offset = 4000;
    FAILS(e, mpx_gather_commit_shorts(e, buf, 43, oth, 3, msgs, cnt, idx, 2, &ns), MPX_E_INVAL);
    // ... which a frame of another code may (it is skipped)
    oth[2].code = MPX_PEER_PREPARE;
    FAILS(e, mpx_gather_commit_shorts(e, buf, 43, oth, 3, msgs, cnt, idx, 2, &ns), MPX_E_UNSUPPORTED);
    oth[2] = mpx_peer_frame{26, MPX_PEER_COMMIT_SHORT, {0, 0, 0}};
    // valid calls
    FAILS(e, mpx_gather_commit_shorts(e, buf, 43, oth, 3, msgs, cnt, idx, 2, &ns), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_gather_commit_shorts(e, buf, 43, oth, 3, nullptr, nullptr, nullptr, 0, &ns), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_gather_commit_shorts(e, nullptr, 0, nullptr, 0, msgs, cnt, idx, 2, &ns), MPX_E_UNSUPPORTED);
    CHECK(ns == 77);
    // the device form: the same arguments, and the stream's alignment
    FAILS(e, mpx_gather_commit_shorts_dev(e, buf, 43, oth, 3, nullptr, msgs, cnt, idx, 2, nullptr, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_gather_commit_shorts_dev(e, buf + 1, 42, oth, 3, nullptr, msgs, cnt, idx, 2, &ns, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_gather_commit_shorts_dev(e, buf, 43, oth, 3, nullptr, msgs, cnt, idx, 2, &ns, nullptr), MPX_E_UNSUPPORTED);
}

int main() {
    for (int mode : {MPX_MODE_MIN, MPX_MODE_CLASSIC}) {
        for (int32_t N : {1, 3, 5}) {
            mpx_engine* e = nullptr;
            mpx_config cfg{N, mode, 1 << 10, 0, 0, 0};
            CHECK(mpx_open(0, &cfg, &e) == MPX_OK && e);
            if (!e) return 1;
            handle(e);
            encode(e, N);
            gather(e);
            CHECK(mpx_close(e) == MPX_OK);
        }
    }
    CHECK(mpx_commit_handle(nullptr, nullptr, 0, nullptr, 0, 0, nullptr, 0, 0, nullptr, nullptr) == MPX_E_INVAL);
    CHECK(mpx_encode_commits(nullptr, nullptr, nullptr, 0, nullptr) == MPX_E_INVAL);
    CHECK(mpx_encode_commits_reserve(nullptr, 1, 1) == MPX_E_INVAL);
    CHECK(mpx_gather_commit_shorts(nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr) == MPX_E_INVAL);
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("commit_driver: all checks passed\n");
    return failures ? 1 : 0;
}
