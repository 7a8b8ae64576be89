// tests/san/accepts_stored_driver.cpp — TEST INFRASTRUCTURE ONLY: drives
// mpx_encode_accepts_stored and its _reserve / _dev forms of the CPU build of engine.cpp +
// accepts_stored.cpp over the stub runtime (hip_stub.cpp) and a stand-in for the launcher that
// really encodes (accepts_stored_stub.cpp), under ASan + UBSan. Every argument-validation path
// of both forms must answer its code before anything is staged; valid MIN and CLASSIC calls bring
// the hand-worked bytes of tests/accepts_stored_kat.py back through the staging on guarded
// buffers, and a 2^20-entry arena is staged as the referenced commands alone.
// Exit status 0 = all checks passed.
#include <string>

#include "san_check.hpp"

struct AsStubSeen {
    uint64_t calls, n_src, non_nil, flagged;
};
extern AsStubSeen as_stub_seen;

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

// the known answer "self2_lb" of tests/accepts_stored_kat.py: N = 3, one group of 8 at base 100,
// instance 103 sent at ballot 33 with last_committed 102 by replica 2; peer 0 takes the log from
// first_g (three records), peer 1 one record
static const char* kNew = "01 0500000000000000 0600000000000000 02 0700000000000000 0000000000000000";
static const char* kA2_4 = "01 2000000000000000 2100000000000000 01 2200000000000000 2300000000000000"
                           "03 2400000000000000 0000000000000000";
static const char* kA6 = "02 1000000000000000 0000000000000000";
static std::string head_min() { return std::string("09 02000000 67000000 21000000 66000000 04") + kNew; }
static std::string rec2() { return std::string("12000000 03000000 06") + kA2_4; }
static std::vector<uint8_t> want_min() {
    return unhex(head_min() + "06" + "10000000 03000000 00" + "11000000 02000000 02" + kA6 + rec2() +
                 head_min() + "02" + rec2());
}
static std::vector<uint8_t> want_classic() {  // peers 0 and 1: no LastCommitted, no log
    const std::string f = std::string("09 02000000 67000000 21000000 04") + kNew;
    return unhex(f + f);
}

struct Kat {
    alignas(16) mpx_accept_send sends[1] = {{103, 33, 102, MPX_PH_ACCEPT, 0, 2, 0}};
    alignas(16) mpx_proposer_group groups[1] = {{33, 2, 2, 2, 104, 102, {0, 0}}};
    alignas(16) int32_t pc[3] = {98, 101, 102};
    uint8_t op[2] = {1, 2};
    alignas(16) int64_t key[2] = {5, 7}, val[2] = {6, 0};
    alignas(16) mpx_acceptor_state st[8];
    alignas(16) mpx_inst_state lb[8];
    alignas(16) mpx_inst_cmds inst[8];
    std::vector<uint8_t> sop;
    std::vector<int64_t> skey, sval;
    mpx_accept_store_batch b{};
    // arena_size: 8, or larger with instance 2's range ending exactly at its end and instance 1's
    // in the middle
    explicit Kat(size_t arena_size = 8) {
        for (int i = 0; i < 8; ++i) {
            st[i] = mpx_acceptor_state{MPX_STATUS_NIL, 0, 0, 0};
            lb[i] = mpx_inst_state{MPX_STATUS_NIL, 0, 0, 0};
            inst[i] = mpx_inst_cmds{0, 0, 0};
        }
        st[0] = {MPX_COMMITTED, 16, 0, 0}, st[1] = {MPX_ACCEPTED, 17, 0, 0};
        st[2] = {MPX_PREPARED, 18, 0, 0}, st[3] = {MPX_PREPARED, 33, 0, 1};
        lb[1] = {MPX_ACCEPTED, 1, 0, 0}, lb[2] = {MPX_COMMITTED, 2, 0, 17}, lb[3] = {MPX_PREPARED, 0, 0, 0};
        sop.assign(arena_size, 0xEE), skey.assign(arena_size, -1), sval.assign(arena_size, -1);
        const size_t r2 = arena_size == 8 ? 2 : arena_size - 3, r1 = arena_size == 8 ? 6 : arena_size / 2;
        const uint8_t o[3] = {1, 1, 3};
        const int64_t k[3] = {0x20, 0x22, 0x24}, v[3] = {0x21, 0x23, 0};
        for (int i = 0; i < 3; ++i) sop[r2 + i] = o[i], skey[r2 + i] = k[i], sval[r2 + i] = v[i];
        sop[r1] = 2, skey[r1] = 0x10, sval[r1] = 0;
        inst[0] = {99, 7, 0};  // unflagged: Cmds == nil, first_cmd / n_cmds are not read
        inst[1] = {r1, 1, MPX_IC_HAS_CMDS}, inst[2] = {r2, 3, MPX_IC_HAS_CMDS};
        inst[5] = {r1, 1, MPX_IC_HAS_CMDS};  // outside every range
        b.sends = sends, b.n_sends = 1, b.inst_base = 100, b.ipg = 8, b.n_groups = 1;
        b.groups = groups, b.peer_commits = pc;
        b.cmd_op = op, b.cmd_key = key, b.cmd_val = val, b.n_cmds = 2;
        b.st = st, b.lb = lb, b.inst = inst;
        b.src_op = sop.data(), b.src_key = skey.data(), b.src_val = sval.data(), b.n_src = arena_size;
        b.alive_mask = 0xFFFF;
    }
};

// p moved by `by` bytes (a misaligned address for the device form)
template <typename T>
static void bump(const T*& p, size_t by) {
    p = reinterpret_cast<const T*>(reinterpret_cast<const char*>(p) + by);
}

// out holds `want` over its first bytes and its guard pattern behind them
static bool holds(const Out& out, const std::vector<uint8_t>& want, size_t n) {
    for (size_t i = 0; i < out.v.size(); ++i)
        if (out.v[i] != (i < n ? want[i] : kGuardByte)) return false;
    return true;
}

// a valid call on guarded copies of every array: the inputs come back intact, out holds the
// expected bytes and nothing behind them, dest_off is complete. spare < 0: out_cap is short.
static void valid_case(mpx_engine* e, int mode, const Kat& k, int spare, bool dev, bool store) {
    const bool min = mode == MPX_MODE_MIN;
    const std::vector<uint8_t> want = min ? want_min() : want_classic();
    const size_t total = want.size(), out_cap = total + spare;
    const uint64_t off_min[4] = {0, 148, 261, 261}, off_cl[4] = {0, 48, 96, 96};
    In snd = holding(k.sends, 1, 1), grp = holding(k.groups, 1, 2), pc = holding(k.pc, 3, 3),
       op = holding(k.op, 2, 4), key = holding(k.key, 2, 5), val = holding(k.val, 2, 6),
       st = holding(k.st, 8, 7), lb = holding(k.lb, 8, 8), inst = holding(k.inst, 8, 9),
       sop = holding(k.sop.data(), k.sop.size(), 10), skey = holding(k.skey.data(), k.skey.size(), 11),
       sval = holding(k.sval.data(), k.sval.size(), 12);
    mpx_accept_store_batch b = k.b;
    b.sends = snd.as<mpx_accept_send>(), b.groups = grp.as<mpx_proposer_group>();
    b.peer_commits = pc.as<int32_t>();
    b.cmd_op = op.as<uint8_t>(), b.cmd_key = key.as<int64_t>(), b.cmd_val = val.as<int64_t>();
    if (store) {
        b.st = st.as<mpx_acceptor_state>(), b.lb = lb.as<mpx_inst_state>();
        b.inst = inst.as<mpx_inst_cmds>();
        b.src_op = sop.as<uint8_t>(), b.src_key = skey.as<int64_t>(), b.src_val = sval.as<int64_t>();
    } else {  // CLASSIC reads none of them
        b.st = nullptr, b.lb = nullptr, b.inst = nullptr, b.peer_commits = nullptr;
        b.src_op = nullptr, b.src_key = nullptr, b.src_val = nullptr, b.n_src = 0;
    }
    Out out(spare < 0 ? total : out_cap);
    std::vector<uint64_t> off((size_t)N + 2, kOffGuard);
    const int rc = dev ? mpx_encode_accepts_stored_dev(e, &b, out.as<uint8_t>(), out_cap, off.data(), nullptr)
                       : mpx_encode_accepts_stored(e, &b, out.as<uint8_t>(), out_cap, off.data());
    if (spare < 0 && !dev) {  // (the device form leaves the comparison to its caller)
        CHECK(rc == MPX_E_INVAL && strstr(mpx_last_error(e), "out_cap"));
        CHECK(out.untouched());
    } else {
        if (rc != MPX_OK) fprintf(stderr, "  got %d: %s\n", rc, mpx_last_error(e));
        CHECK(rc == MPX_OK);
        CHECK(holds(out, want, total < out_cap ? total : out_cap));
    }
    for (int q = 0; q <= N; ++q) CHECK(off[q] == (min ? off_min : off_cl)[q]);
    CHECK(off[(size_t)N + 1] == kOffGuard);
    CHECK(snd.intact() && grp.intact() && pc.intact() && op.intact() && key.intact() && val.intact());
    CHECK(st.intact() && lb.intact() && inst.intact() && sop.intact() && skey.intact() && sval.intact());
}

static void validation(mpx_engine* e, int mode) {
    const bool min = mode == MPX_MODE_MIN;
    Kat k;
    Out guarded(4096);
    uint8_t* const out = guarded.as<uint8_t>();
    const size_t out_size = 4096;
    std::vector<uint64_t> off((size_t)N + 1, kOffGuard);
    auto call = [&](const mpx_accept_store_batch& x) {
        return mpx_encode_accepts_stored(e, &x, out, out_size, off.data());
    };
    const mpx_accept_store_batch& b = k.b;
    FAILS(e, mpx_encode_accepts_stored(e, nullptr, out, out_size, off.data()), MPX_E_INVAL);
    FAILS(e, mpx_encode_accepts_stored(e, &b, nullptr, out_size, off.data()), MPX_E_INVAL);
    FAILS(e, mpx_encode_accepts_stored(e, &b, out, out_size, nullptr), MPX_E_INVAL);
    mpx_accept_store_batch x = b;
    x.sends = nullptr;
    FAILS(e, call(x), MPX_E_INVAL);
    x = b, x.groups = nullptr;
    FAILS(e, call(x), MPX_E_INVAL);
    x = b, x.reserved = 1;
    FAILS(e, call(x), MPX_E_INVAL);
    x = b, x.ipg = 0;
    FAILS(e, call(x), MPX_E_INVAL);
    x = b, x.n_groups = 0;
    FAILS(e, call(x), MPX_E_INVAL);
    x = b, x.cmd_key = nullptr;
    FAILS(e, call(x), MPX_E_INVAL);
    x = b, x.n_sends = (size_t)1 << 32;
    FAILS(e, call(x), MPX_E_UNSUPPORTED);
    // a send outside the window, commands outside the arrays, self_id outside [0, N)
    k.sends[0].instance = 108;
    FAILS(e, call(b), MPX_E_INVAL);
    k.sends[0].instance = 99;
    FAILS(e, call(b), MPX_E_INVAL);
    k.sends[0].instance = 103;
    k.sends[0].first_cmd = 1;
    FAILS(e, call(b), MPX_E_INVAL);
    k.sends[0].first_cmd = ~0ull;
    FAILS(e, call(b), MPX_E_INVAL);
    k.sends[0].first_cmd = 0;
    k.groups[0].self_id = N;
    FAILS(e, call(b), MPX_E_INVAL);
    k.groups[0].self_id = -1;
    FAILS(e, call(b), MPX_E_INVAL);
    k.groups[0].self_id = 2;
    if (min) {
        x = b, x.peer_commits = nullptr;
        FAILS(e, call(x), MPX_E_INVAL);
        x = b, x.st = nullptr;
        FAILS(e, call(x), MPX_E_INVAL);
        x = b, x.inst = nullptr;
        FAILS(e, call(x), MPX_E_INVAL);
        // last_committed >= instance, and below first_g - 1
        k.sends[0].last_committed = 103;
        FAILS(e, call(b), MPX_E_INVAL);
        k.sends[0].last_committed = 98;
        FAILS(e, call(b), MPX_E_INVAL);
        k.sends[0].last_committed = 102;
        // a nil instance inside a catch-up range (peer 0 reads 100 .. 102)
        k.st[1].status = MPX_STATUS_NIL;
        FAILS(e, call(b), MPX_E_NIL_INSTANCE);
        k.st[1].status = MPX_ACCEPTED;
        // a flagged slot inside a range whose commands leave the arena, or have no arena
        k.inst[1].first_cmd = 8;
        FAILS(e, call(b), MPX_E_INVAL);
        k.inst[1].first_cmd = 9, k.inst[1].n_cmds = 0;
        FAILS(e, call(b), MPX_E_INVAL);
        k.inst[1].first_cmd = ~0ull, k.inst[1].n_cmds = 2;
        FAILS(e, call(b), MPX_E_INVAL);
        k.inst[1].first_cmd = 6, k.inst[1].n_cmds = 3;
        FAILS(e, call(b), MPX_E_INVAL);
        k.inst[1].n_cmds = 1;
        x = b, x.src_key = nullptr;
        FAILS(e, call(x), MPX_E_INVAL);
        CHECK(guarded.untouched() && off[0] == kOffGuard && off[(size_t)N] == kOffGuard);
        // slots outside every range are not judged: a nil, and a range that leaves the arena
        k.st[3].status = MPX_STATUS_NIL;
        k.inst[5].first_cmd = 1000;
        k.inst[6] = {~0ull, 5, MPX_IC_HAS_CMDS};
        CHECK(call(b) == MPX_OK && off[(size_t)N] == 261);
        k.pc[0] = 102, k.pc[1] = 102;  // no peer needs the log: nothing of it is judged
        k.st[1].status = MPX_STATUS_NIL, k.inst[2].first_cmd = 7;
        CHECK(call(b) == MPX_OK && off[(size_t)N] == 2 * 53);
        k.sends[0].flags = MPX_PH_REFUSED;  // ... or the slot is skipped
        k.pc[0] = 98;
        CHECK(call(b) == MPX_OK && off[(size_t)N] == 0);
    }
    FAILS(e, mpx_encode_accepts_stored_reserve(e, (size_t)1 << 32, 8), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_encode_accepts_stored_reserve(e, 8, ((size_t)1 << 32) + 1), MPX_E_UNSUPPORTED);
    // the device form: the same shape checks, and every alignment
    Kat d;
    const mpx_accept_store_batch& db = d.b;
    auto dev = [&](const mpx_accept_store_batch& y) {
        return mpx_encode_accepts_stored_dev(e, &y, out, out_size, off.data(), nullptr);
    };
    CHECK(mpx_encode_accepts_stored_reserve(e, 4, 8) == MPX_OK);
    FAILS(e, mpx_encode_accepts_stored_dev(e, nullptr, out, out_size, off.data(), nullptr), MPX_E_INVAL);
    FAILS(e, mpx_encode_accepts_stored_dev(e, &db, out, out_size, nullptr, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_encode_accepts_stored_dev(e, &db, nullptr, out_size, off.data(), nullptr), MPX_E_INVAL);
    x = db, x.ipg = 0;
    FAILS(e, dev(x), MPX_E_INVAL);
    x = db, x.reserved = 7;
    FAILS(e, dev(x), MPX_E_INVAL);
    if (min) {
        x = db, x.st = nullptr;
        FAILS(e, dev(x), MPX_E_INVAL);
        x = db, x.inst = nullptr;
        FAILS(e, dev(x), MPX_E_INVAL);
    }
    x = db, bump(x.sends, 8);
    FAILS(e, dev(x), MPX_E_INVAL);
    x = db, bump(x.groups, 8);
    FAILS(e, dev(x), MPX_E_INVAL);
    x = db, bump(x.st, 8);
    FAILS(e, dev(x), MPX_E_INVAL);
    x = db, bump(x.lb, 8);
    FAILS(e, dev(x), MPX_E_INVAL);
    x = db, bump(x.inst, 8);
    FAILS(e, dev(x), MPX_E_INVAL);
    x = db, bump(x.cmd_key, 4);
    FAILS(e, dev(x), MPX_E_INVAL);
    x = db, bump(x.cmd_val, 4);
    FAILS(e, dev(x), MPX_E_INVAL);
    x = db, bump(x.src_key, 4);
    FAILS(e, dev(x), MPX_E_INVAL);
    x = db, bump(x.src_val, 4);
    FAILS(e, dev(x), MPX_E_INVAL);
    x = db, bump(x.peer_commits, 2);
    FAILS(e, dev(x), MPX_E_INVAL);
    FAILS(e, mpx_encode_accepts_stored_dev(e, &db, out, out_size, (uint64_t*)((char*)off.data() + 4), nullptr),
          MPX_E_INVAL);
    CHECK(strstr(mpx_last_error(e), "aligned"));
}

int main() {
    for (int mode : {MPX_MODE_MIN, MPX_MODE_CLASSIC}) {
        const bool min = mode == MPX_MODE_MIN;
        mpx_engine* e = open_engine(mode);
        if (!e) return 1;
        validation(e, mode);
        // valid calls on guarded buffers: room to spare, an exact fit, a byte short
        Kat k;
        for (const int spare : {40, 0, -1}) valid_case(e, mode, k, spare, false, true);
        if (!min) valid_case(e, mode, k, 40, false, false);
        if (min) {
            // what the host form staged: the three slots of the ranges (instance 3's state and slot
            // 5's commands lie outside them) and, of the arena, the four referenced commands
            CHECK(as_stub_seen.n_src == 4 && as_stub_seen.non_nil == 3 && as_stub_seen.flagged == 2);
            // a 2^20-entry arena: instance 2's range ends exactly at its end
            Kat big((size_t)1 << 20);
            const uint64_t before = as_stub_seen.calls;
            valid_case(e, mode, big, 40, false, true);
            CHECK(as_stub_seen.calls == before + 1);
            CHECK(as_stub_seen.n_src == 4);  // 68 bytes of commands, not 17 MiB
            CHECK(as_stub_seen.non_nil == 3 && as_stub_seen.flagged == 2);
        }
        CHECK(mpx_close(e) == MPX_OK);
        // the device form never allocates: on a fresh handle it needs its reserve call first (an
        // empty call does not); the dense form's reserve of the same sizes is not enough in MIN
        mpx_engine* f = open_engine(mode);
        if (!f) return 1;
        Out out(4096);
        std::vector<uint64_t> off((size_t)N + 1, kOffGuard);
        FAILS(f, mpx_encode_accepts_stored_dev(f, &k.b, out.as<uint8_t>(), 4096, off.data(), nullptr), MPX_E_INVAL);
        CHECK(strstr(mpx_last_error(f), "mpx_encode_accepts_stored_dev") &&
              strstr(mpx_last_error(f), "mpx_encode_accepts_stored_reserve"));
        CHECK(out.untouched());
        mpx_accept_store_batch none = k.b;
        none.n_sends = 0;
        CHECK(mpx_encode_accepts_stored_dev(f, &none, out.as<uint8_t>(), 4096, off.data(), nullptr) == MPX_OK);
        CHECK(mpx_encode_accepts_stored_reserve(f, 1, 8) == MPX_OK);
        valid_case(f, mode, k, 40, true, true);
        valid_case(f, mode, k, -1, true, true);  // (never writes at or past out_cap)
        if (min) CHECK(as_stub_seen.n_src == 8 && as_stub_seen.non_nil == 4);  // nothing is staged
        CHECK(mpx_close(f) == MPX_OK);
    }
    CHECK(mpx_encode_accepts_stored(nullptr, nullptr, nullptr, 0, nullptr) == MPX_E_INVAL);
    CHECK(mpx_encode_accepts_stored_reserve(nullptr, 1, 1) == MPX_E_INVAL);
    CHECK(mpx_encode_accepts_stored_dev(nullptr, nullptr, nullptr, 0, nullptr, nullptr) == MPX_E_INVAL);
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("accepts_stored_driver: all checks passed\n");
    return failures ? 1 : 0;
}
