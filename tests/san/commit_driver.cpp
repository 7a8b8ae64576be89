// tests/san/commit_driver.cpp — TEST INFRASTRUCTURE ONLY: drives the commit entry points
// (mpx_commit_handle, mpx_encode_commits, mpx_gather_commit_shorts and their _reserve / _dev
// forms) of the CPU build of engine.cpp over the stub runtime (hip_stub.cpp) under ASan + UBSan.
// Every argument-validation path must answer its code (MPX_E_INVAL, MPX_E_UNSUPPORTED for a size
// limit) before anything is staged; a valid call answers MPX_OK and, over the stub's stand-ins
// for the commit launchers, stages its arrays whole and apart (the staging checks of
// san_check.hpp). Exit status 0 = all checks passed.
#include "san_check.hpp"

constexpr uint64_t kOffGuard = 0x5C5C5C5C5C5C5C5Cull;
constexpr size_t kStubCommitFrame = MPX_COMMIT_SHORT_FRAME;  // (hip_stub.cpp, stub_frames)

static mpx_engine* open_engine(int32_t N, int mode) {
    mpx_engine* e = nullptr;
    mpx_config cfg{N, mode, 1 << 10, 0, 0, 0};
    CHECK(mpx_open(0, &cfg, &e) == MPX_OK && e);
    return e;
}

// a valid mpx_commit_handle call of n messages over G groups of 4 on guarded buffers: st and
// committed_upto are updated in place, effect and log_recs (when given) are the outputs
static void handle_case(mpx_engine* e, const mpx_accept_msg* msgs, size_t n, const int32_t* cu0,
                        size_t G, bool with_log, bool dev) {
    In msg = holding(msgs, n, 1), st(4 * G * sizeof(mpx_acceptor_state), 2), cu = holding(cu0, G, 3);
    Out eff(n), log(n * sizeof(mpx_log_rec));
    mpx_log_rec* plog = with_log ? log.as<mpx_log_rec>() : nullptr;
    if (dev)
        CHECK(mpx_commit_handle_dev(e, msg.as<mpx_accept_msg>(), n, st.as<mpx_acceptor_state>(),
                                    4 * G, 100, cu.as<int32_t>(), G, 4, eff.as<uint8_t>(), plog,
                                    nullptr) == MPX_OK);
    else
        CHECK(mpx_commit_handle(e, n ? msg.as<mpx_accept_msg>() : nullptr, n,
                                st.as<mpx_acceptor_state>(), 4 * G, 100, cu.as<int32_t>(), G, 4,
                                n ? eff.as<uint8_t>() : nullptr, plog) == MPX_OK);
    CHECK(msg.intact() && st.flipped() && cu.flipped() && eff.is(0));
    CHECK(with_log ? log.is(1) : log.untouched());
}

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
    // the device form validates the same shape
    FAILS(e, mpx_commit_handle_dev(e, nullptr, 3, st.data(), 8, base, cu, 2, ipg, eff, log, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_commit_handle_dev(e, msgs, 3, nullptr, 8, base, cu, 2, ipg, eff, log, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_commit_handle_dev(e, msgs, 3, st.data(), 9, base, cu, 2, ipg, eff, log, nullptr), MPX_E_INVAL);
    CHECK(st[0].status == MPX_STATUS_NIL && cu[0] == 99 && eff[0] == 9);  // nothing was touched
    // valid calls: with and without log_recs, no message, the device form
    handle_case(e, msgs, 3, cu, 2, true, false);
    handle_case(e, msgs, 3, cu, 2, false, false);
    handle_case(e, msgs, 0, cu, 2, false, false);
    handle_case(e, msgs, 0, cu, 2, true, false);
    handle_case(e, msgs, 3, cu, 2, false, true);
    handle_case(e, msgs, 3, cu, 2, true, true);
    // ... and the two ends of committed_upto's range are legal
    const int32_t ends[2] = {base + 3, base + 3};
    handle_case(e, msgs, 3, ends, 2, true, false);
    // ... and of a size at which the arrays have slots of more than one 256-byte unit
    std::vector<mpx_accept_msg> many(300, msgs[0]);
    std::vector<int32_t> cus(100);
    for (int32_t g = 0; g < 100; ++g) cus[g] = base + 4 * g - 1;
    handle_case(e, many.data(), 300, cus.data(), 100, true, false);
    handle_case(e, many.data(), 300, cus.data(), 100, false, false);
    handle_case(e, many.data(), 300, cus.data(), 100, true, true);
}

// The valid batch of encode() on guarded buffers, its three sends repeated up to n_sends (two of
// three carry MPX_CS_SEND and put one stub frame in every destination's run): the inputs come back
// intact, dest_off holds the stub's offsets and out its pattern over dest_off[N] bytes. spare:
// out_cap - dest_off[N]; below 0 the call answers MPX_E_INVAL with dest_off written and out
// untouched. cmds: with the command arrays, else the sends carry none and they are absent.
static void encode_case(mpx_engine* e, int32_t N, const mpx_commit_batch& b0, bool cmds,
                        size_t n_sends, int spare, bool dev) {
    const size_t flagged = n_sends - (n_sends + 1) / 3;
    const size_t total = (size_t)N * flagged * kStubCommitFrame, out_cap = total + spare;
    std::vector<mpx_commit_send> sv(n_sends);
    for (size_t i = 0; i < n_sends; ++i) {
        sv[i] = b0.sends[i % 3];
        if (!cmds) sv[i].first_cmd = sv[i].n_cmds = 0;
    }
    const size_t m = cmds ? 100 : 0;  // (the sends name the first three; the values are not looked at)
    In snd = holding(sv.data(), n_sends, 1), grp = holding(b0.groups, b0.n_groups, 2), op(m, 3),
       key(m * 8, 4), val(m * 8, 5);
    mpx_commit_batch b = b0;
    b.sends = snd.as<mpx_commit_send>();
    b.n_sends = n_sends;
    b.groups = grp.as<mpx_proposer_group>();
    b.cmd_op = cmds ? op.as<uint8_t>() : nullptr;
    b.cmd_key = cmds ? key.as<int64_t>() : nullptr;
    b.cmd_val = cmds ? val.as<int64_t>() : nullptr;
    b.n_cmds = m;
    Out out(spare < 0 ? total : out_cap);
    std::vector<uint64_t> off((size_t)N + 2, kOffGuard);
    const int rc = dev ? mpx_encode_commits_dev(e, &b, out.as<uint8_t>(), out_cap, off.data(), nullptr)
                       : mpx_encode_commits(e, &b, out.as<uint8_t>(), out_cap, off.data());
    if (spare < 0 && !dev) {  // (the device form leaves the comparison to its caller)
        CHECK(rc == MPX_E_INVAL && strstr(mpx_last_error(e), "out_cap"));
        CHECK(out.untouched());
    } else {
        CHECK(rc == MPX_OK);
        CHECK(out.is(0, total < out_cap ? total : out_cap));
    }
    for (int32_t q = 0; q <= N; ++q) CHECK(off[q] == (uint64_t)q * flagged * kStubCommitFrame);
    CHECK(off[(size_t)N + 1] == kOffGuard);
    CHECK(snd.intact() && grp.intact() && op.intact() && key.intact() && val.intact());
}

static void encode(mpx_engine* e, int mode, int32_t N) {
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
    Out guarded(4096);
    uint8_t* const out = guarded.as<uint8_t>();
    const size_t out_size = 4096;
    std::vector<uint64_t> off((size_t)N + 1, kOffGuard);
    auto call = [&](const mpx_commit_batch& x) {
        return mpx_encode_commits(e, &x, out, out_size, off.data());
    };
    FAILS(e, mpx_encode_commits(e, nullptr, out, out_size, off.data()), MPX_E_INVAL);
    FAILS(e, mpx_encode_commits(e, &b, nullptr, out_size, off.data()), MPX_E_INVAL);
    FAILS(e, mpx_encode_commits(e, &b, out, out_size, nullptr), MPX_E_INVAL);
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
    FAILS(e, mpx_encode_commits_reserve(e, (size_t)1 << 33, 8), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_encode_commits_dev(e, nullptr, out, out_size, off.data(), nullptr), MPX_E_INVAL);
    FAILS(e, mpx_encode_commits_dev(e, &b, out, out_size, nullptr, nullptr), MPX_E_INVAL);
    x = b;
    x.ipg = 0;
    FAILS(e, mpx_encode_commits_dev(e, &x, out, out_size, off.data(), nullptr), MPX_E_INVAL);
    // nothing was touched
    CHECK(guarded.untouched() && off[0] == kOffGuard && off[(size_t)N] == kOffGuard);
    // ... none of which counts on a skipped slot
    sends[1].instance = 7;
    sends[1].first_cmd = 99;
    CHECK(call(b) == MPX_OK && off[(size_t)N] == (size_t)N * 2 * kStubCommitFrame);
    // valid calls
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
        encode_case(e, N, b, cmds, 3, 40, false);
        encode_case(e, N, b, cmds, 77, 40, false);
        encode_case(e, N, b, cmds, 77, 0, false);
        encode_case(e, N, b, cmds, 77, -1, false);
        encode_case(e, N, b, cmds, 3, -1, false);
        encode_case(e, N, b, cmds, 0, 40, false);
        encode_case(e, N, b, cmds, 0, 0, false);
    }
    // the device form never allocates: on a fresh handle it needs its reserve call first (an empty
    // call does not)
    mpx_engine* f = open_engine(N, mode);
    if (!f) return;
    FAILS(f, mpx_encode_commits_dev(f, &b, out, out_size, off.data(), nullptr), MPX_E_INVAL);
    CHECK(strstr(mpx_last_error(f), "mpx_encode_commits_dev") && strstr(mpx_last_error(f), "mpx_encode_commits_reserve"));
    encode_case(f, N, b, true, 0, 40, true);
    CHECK(mpx_encode_commits_reserve(f, 16, 8) == MPX_OK);
    encode_case(f, N, b, true, 16, 40, true);
    encode_case(f, N, b, false, 16, -1, true);  // (never writes at or past out_cap)
    CHECK(mpx_close(f) == MPX_OK);
}

// a valid mpx_gather_commit_shorts call over n_other frames, gather()'s three repeated (the
// repeats name the same bytes), on guarded buffers: buf and other come back intact, *n_shorts is the CommitShort count and msgs, count and
// frame_index hold their patterns over min(cap, count) elements
static void gather_case(mpx_engine* e, const uint8_t* buf0, const mpx_peer_frame* oth0,
                        size_t n_other, size_t cap, bool arrays, bool dev) {
    uint64_t want = 0;
    std::vector<mpx_peer_frame> ov(n_other);
    for (size_t i = 0; i < n_other; ++i) ov[i] = oth0[i % 3];
    for (size_t i = 0; i < n_other; ++i) want += ov[i].code == MPX_PEER_COMMIT_SHORT;
    const size_t k = want < cap ? want : cap, len = n_other ? 43 : 0;
    // (the device form wants a 16-byte-aligned buffer: a vector's storage is)
    In buf = holding(buf0, 43, 1), oth = holding(ov.data(), n_other, 2);
    Out msgs(cap * sizeof(mpx_accept_msg)), cnt(cap * 4), idx(cap * 4);
    uint64_t ns[2] = {kOffGuard, kOffGuard};
    mpx_accept_msg* pm = arrays ? msgs.as<mpx_accept_msg>() : nullptr;
    int32_t* pc = arrays ? cnt.as<int32_t>() : nullptr;
    uint32_t* pi = arrays ? idx.as<uint32_t>() : nullptr;
    if (dev)
        CHECK(mpx_gather_commit_shorts_dev(e, buf.as<uint8_t>(), len, oth.as<mpx_peer_frame>(),
                                           n_other, nullptr, pm, pc, pi, arrays ? cap : 0, ns,
                                           nullptr) == MPX_OK);
    else
        CHECK(mpx_gather_commit_shorts(e, n_other ? buf.as<uint8_t>() : nullptr, len,
                                       n_other ? oth.as<mpx_peer_frame>() : nullptr, n_other, pm,
                                       pc, pi, arrays ? cap : 0, ns) == MPX_OK);
    CHECK(buf.intact() && oth.intact() && ns[0] == want && ns[1] == kOffGuard);
    if (arrays) CHECK(msgs.is(0, k * sizeof(mpx_accept_msg)) && cnt.is(1, k * 4) && idx.is(2, k * 4));
    else CHECK(msgs.untouched() && cnt.untouched() && idx.untouched());
}

static void gather(mpx_engine* e, int mode, int32_t N) {
    alignas(16) uint8_t buf[64] = {0};
    buf[0] = MPX_PEER_BEACON;
    buf[9] = MPX_PEER_COMMIT_SHORT;
    buf[26] = MPX_PEER_COMMIT_SHORT;
    mpx_peer_frame oth[3] = {{0, MPX_PEER_BEACON, {0, 0, 0}},
                             {9, MPX_PEER_COMMIT_SHORT, {0, 0, 0}},
                             {26, MPX_PEER_COMMIT_SHORT, {0, 0, 0}}};
    mpx_accept_msg msgs[2];
    int32_t cnt[2] = {-7, -7};
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
    // the device form: the same arguments, and the stream's alignment
    FAILS(e, mpx_gather_commit_shorts_dev(e, buf, 43, oth, 3, nullptr, msgs, cnt, idx, 2, nullptr, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_gather_commit_shorts_dev(e, buf + 1, 42, oth, 3, nullptr, msgs, cnt, idx, 2, &ns, nullptr), MPX_E_INVAL);
    CHECK(ns == 77 && cnt[0] == -7 && cnt[1] == -7);  // nothing was touched
    // ... which a frame of another code may (it is skipped)
    oth[2].code = MPX_PEER_PREPARE;
    CHECK(mpx_gather_commit_shorts(e, buf, 43, oth, 3, msgs, cnt, idx, 2, &ns) == MPX_OK && ns == 1);
    gather_case(e, buf, oth, 3, 2, true, false);
    oth[2] = mpx_peer_frame{26, MPX_PEER_COMMIT_SHORT, {0, 0, 0}};
    // valid calls: a capacity above and below the CommitShort count, of 0 with null arrays, and no
    // frame at all
    gather_case(e, buf, oth, 3, 3, true, false);
    gather_case(e, buf, oth, 3, 2, true, false);
    gather_case(e, buf, oth, 3, 1, true, false);
    gather_case(e, buf, oth, 3, 2, false, false);
    gather_case(e, buf, oth, 0, 2, true, false);
    gather_case(e, buf, oth, 90, 70, true, false);
    gather_case(e, buf, oth, 90, 50, true, false);
    // the device form never allocates: on a fresh handle it needs the family's reserve call first
    mpx_engine* f = open_engine(N, mode);
    if (!f) return;
    FAILS(f, mpx_gather_commit_shorts_dev(f, buf, 43, oth, 3, nullptr, msgs, cnt, idx, 2, &ns, nullptr), MPX_E_INVAL);
    CHECK(strstr(mpx_last_error(f), "mpx_gather_commit_shorts_dev") && strstr(mpx_last_error(f), "mpx_encode_commits_reserve"));
    gather_case(f, buf, oth, 0, 2, true, true);
    CHECK(mpx_encode_commits_reserve(f, 0, 3) == MPX_OK);
    gather_case(f, buf, oth, 3, 3, true, true);
    gather_case(f, buf, oth, 3, 1, true, true);
    CHECK(mpx_close(f) == MPX_OK);
}

int main() {
    for (int mode : {MPX_MODE_MIN, MPX_MODE_CLASSIC}) {
        for (int32_t N : {1, 3, 5}) {
            mpx_engine* e = open_engine(N, mode);
            if (!e) return 1;
            handle(e);
            encode(e, mode, N);
            gather(e, mode, N);
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
