// tests/san/unmarshal_driver.cpp — TEST INFRASTRUCTURE ONLY: drives mpx_unmarshal_frames and its
// _reserve / _dev forms of the CPU build of engine.cpp over the stub runtime (hip_stub.cpp) under
// ASan + UBSan. Every validation path of the host form must answer its code (MPX_E_INVAL,
// MPX_E_UNSUPPORTED for a size limit) before anything is staged; a valid call answers MPX_OK and,
// over the stub's stand-ins for the unmarshal launchers, stages its arrays whole and apart (the
// staging checks of san_check.hpp). Exit status 0 = all checks passed.
#include <algorithm>
#include <utility>

#include "san_check.hpp"

static void put32(std::vector<uint8_t>& b, int32_t v) {
    for (int i = 0; i < 4; ++i) b.push_back((uint8_t)((uint32_t)v >> (8 * i)));
}
static void put_cmd(std::vector<uint8_t>& b, uint8_t op, int64_t k, int64_t v) {
    b.push_back(op);
    for (int i = 0; i < 8; ++i) b.push_back((uint8_t)((uint64_t)k >> (8 * i)));
    for (int i = 0; i < 8; ++i) b.push_back((uint8_t)((uint64_t)v >> (8 * i)));
}

// an Accept (2 commands; MIN: a log of one instance with one command), a Commit (1 command) and a
// PrepareReply (no command; MIN: an empty log), back to back, with their frame records
static void build(int mode, std::vector<uint8_t>& b, mpx_var_frame f[3]) {
    const bool min = mode == MPX_MODE_MIN;
    memset(f, 0, 3 * sizeof(mpx_var_frame));
    f[0].offset = 0;
    f[0].code = MPX_PEER_ACCEPT;
    b.push_back(MPX_PEER_ACCEPT);
    put32(b, 1);
    put32(b, 7);
    put32(b, 33);
    if (min) put32(b, 6);
    b.push_back(4);  // V(2)
    f[0].n_cmds = 2;
    f[0].cmds_off = (uint32_t)b.size();
    put_cmd(b, 1, 2, 3);
    put_cmd(b, 2, -1, -2);
    if (min) {
        b.push_back(2);  // V(1)
        f[0].n_log = 1;
        f[0].log_off = (uint32_t)b.size();
        put32(b, 33);
        put32(b, 3);
        b.push_back(2);
        put_cmd(b, 1, 5, 6);
    } else {
        f[0].log_off = (uint32_t)b.size();
    }
    f[0].length = (uint32_t)b.size();
    f[1].offset = (uint32_t)b.size();
    f[1].code = MPX_PEER_COMMIT;
    b.push_back(MPX_PEER_COMMIT);
    put32(b, 1);
    put32(b, 6);
    put32(b, 33);
    b.push_back(2);
    f[1].n_cmds = 1;
    f[1].cmds_off = (uint32_t)b.size();
    put_cmd(b, 1, 9, 9);
    f[1].log_off = (uint32_t)b.size();
    f[1].length = (uint32_t)b.size() - f[1].offset;
    f[2].offset = (uint32_t)b.size();
    f[2].code = MPX_PEER_PREPARE_REPLY;
    b.push_back(MPX_PEER_PREPARE_REPLY);
    if (min) put32(b, 2);
    put32(b, 7);
    b.push_back(1);
    put32(b, 33);
    if (min) put32(b, 6);
    b.push_back(0);
    f[2].cmds_off = (uint32_t)b.size();
    if (min) b.push_back(0);
    f[2].log_off = (uint32_t)b.size();
    f[2].length = (uint32_t)b.size() - f[2].offset;
}

// build()'s three frames `reps` times over, back to back
static void build_many(int mode, size_t reps, std::vector<uint8_t>& b, std::vector<mpx_var_frame>& f) {
    std::vector<uint8_t> one;
    mpx_var_frame g[3];
    build(mode, one, g);
    for (size_t r = 0; r < reps; ++r) {
        const uint32_t at = (uint32_t)b.size();
        b.insert(b.end(), one.begin(), one.end());
        for (mpx_var_frame x : g) {
            x.offset += at;
            x.cmds_off += at;
            x.log_off += at;
            f.push_back(x);
        }
    }
}

// A valid call over the first n_var of build()'s frames on guarded buffers. The stub counts the
// frames as the kernel does and gives every catch-up instance one command, so: buf and var come
// back intact, *res is complete, each output holds its pattern over min(capacity, count) elements
// and the offset arrays over n_var + 1 (log_cmd_off: written records + 1) entries. offs: with
// cmd_off / log_inst_off / log_cmd_off; arrays: with the other arrays (else null, capacities 0).
struct Caps {
    size_t acc, com, cmd, li, lc;
};
static void unmarshal_case(mpx_engine* e, const std::vector<uint8_t>& b,
                           const mpx_var_frame* f, size_t n_var, Caps c, bool offs, bool arrays,
                           bool dev) {
    mpx_unmarshal_result want{};
    for (size_t i = 0; i < n_var; ++i) {
        want.n_accepts += f[i].code == MPX_PEER_ACCEPT;
        want.n_commits += f[i].code == MPX_PEER_COMMIT;
        want.n_cmds += f[i].n_cmds;
        want.n_log_inst += f[i].n_log;
    }
    // the host form offers the kernel min(log_cmd_cap, len / 17) command slots
    const size_t lm = dev ? c.lc : want.n_log_inst ? std::min(c.lc, b.size() / 17) : 0;
    want.n_log_cmds = std::min<uint64_t>(lm, want.n_log_inst);
    want.n_var = n_var;
    const size_t na = std::min<uint64_t>(c.acc, want.n_accepts),
                 nc = std::min<uint64_t>(c.com, want.n_commits),
                 m = std::min<uint64_t>(c.cmd, want.n_cmds),
                 li = std::min<uint64_t>(c.li, want.n_log_inst), lc = want.n_log_cmds;
    // (the device form wants a 16-byte-aligned buffer: a vector's storage is)
    In buf = holding(b.data(), b.size(), 1), var = holding(f, n_var, 2);
    Out acc(c.acc * sizeof(mpx_accept_msg)), alc(c.acc * 4), com(c.com * sizeof(mpx_accept_msg)),
        coff((n_var + 1) * 8), op(c.cmd), key(c.cmd * 8), val(c.cmd * 8), loff((n_var + 1) * 8),
        lrec(c.li * sizeof(mpx_log_rec)), lcoff((c.li + 1) * 8), lop(c.lc), lkey(c.lc * 8),
        lval(c.lc * 8), res(sizeof(mpx_unmarshal_result));
    mpx_unmarshal_out o{};
    if (arrays) {
        o.accepts = acc.as<mpx_accept_msg>();
        o.accept_last_committed = alc.as<int32_t>();
        o.commits = com.as<mpx_accept_msg>();
        o.op = op.as<uint8_t>();
        o.key = key.as<int64_t>();
        o.val = val.as<int64_t>();
        o.log_recs = lrec.as<mpx_log_rec>();
        o.log_op = lop.as<uint8_t>();
        o.log_key = lkey.as<int64_t>();
        o.log_val = lval.as<int64_t>();
    }
    o.accept_cap = c.acc;
    o.commit_cap = c.com;
    o.cmd_cap = c.cmd;
    o.log_inst_cap = c.li;
    o.log_cmd_cap = c.lc;
    if (offs) {
        o.cmd_off = coff.as<uint64_t>();
        o.log_inst_off = loff.as<uint64_t>();
        o.log_cmd_off = lcoff.as<uint64_t>();
    }
    if (dev)
        CHECK(mpx_unmarshal_frames_dev(e, buf.as<uint8_t>(), b.size(), var.as<mpx_var_frame>(),
                                       n_var, nullptr, &o, res.as<mpx_unmarshal_result>(),
                                       nullptr) == MPX_OK);
    else
        CHECK(mpx_unmarshal_frames(e, buf.as<uint8_t>(), b.size(), var.as<mpx_var_frame>(), n_var,
                                   &o, res.as<mpx_unmarshal_result>()) == MPX_OK);
    CHECK(buf.intact() && var.intact());
    CHECK(!memcmp(res.v.data(), &want, sizeof(want)));
    for (size_t i = sizeof(want); i < res.v.size(); ++i) CHECK(res.v[i] == kGuardByte);
    if (arrays) {
        CHECK(acc.is(0, na * sizeof(mpx_accept_msg)) && alc.is(1, na * 4));
        CHECK(com.is(2, nc * sizeof(mpx_accept_msg)));
        CHECK(op.is(4, m) && key.is(5, m * 8) && val.is(6, m * 8));
        CHECK(lrec.is(8, li * sizeof(mpx_log_rec)));
        CHECK(lop.is(10, lc) && lkey.is(11, lc * 8) && lval.is(12, lc * 8));
    } else {
        CHECK(acc.untouched() && alc.untouched() && com.untouched() && op.untouched());
        CHECK(key.untouched() && val.untouched() && lrec.untouched() && lop.untouched());
        CHECK(lkey.untouched() && lval.untouched());
    }
    if (offs) CHECK(coff.is(3) && loff.is(7) && lcoff.is(9, (li + 1) * 8));
    else CHECK(coff.untouched() && loff.untouched() && lcoff.untouched());
}

static void run(mpx_engine* e, int mode) {
    const bool min = mode == MPX_MODE_MIN;
    std::vector<uint8_t> b;
    mpx_var_frame f[3];
    build(mode, b, f);
    mpx_accept_msg acc[2], com[2];
    int32_t alc[2];
    uint64_t coff[4], loff[4], lcoff[3];
    uint8_t op[4], lop[4];
    int64_t key[4], val[4], lkey[4], lval[4];
    mpx_log_rec lrec[2];
    mpx_unmarshal_out o{};
    o.accepts = acc;
    o.accept_last_committed = alc;
    o.accept_cap = 2;
    o.commits = com;
    o.commit_cap = 2;
    o.cmd_off = coff;
    o.op = op;
    o.key = key;
    o.val = val;
    o.cmd_cap = 4;
    o.log_inst_off = loff;
    o.log_recs = lrec;
    o.log_cmd_off = lcoff;
    o.log_inst_cap = 2;
    o.log_op = lop;
    o.log_key = lkey;
    o.log_val = lval;
    o.log_cmd_cap = 4;
    mpx_unmarshal_result res;
    auto call = [&](const mpx_var_frame* v, size_t n, size_t len, const mpx_unmarshal_out& x) {
        return mpx_unmarshal_frames(e, b.data(), len, v, n, &x, &res);
    };
    // null arguments, capacities without arrays
    FAILS(e, mpx_unmarshal_frames(e, nullptr, b.size(), f, 3, &o, &res), MPX_E_INVAL);
    FAILS(e, mpx_unmarshal_frames(e, b.data(), b.size(), nullptr, 3, &o, &res), MPX_E_INVAL);
    FAILS(e, mpx_unmarshal_frames(e, b.data(), b.size(), f, 3, nullptr, &res), MPX_E_INVAL);
    FAILS(e, mpx_unmarshal_frames(e, b.data(), b.size(), f, 3, &o, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_unmarshal_frames(e, b.data(), 0, f, 3, &o, &res), MPX_E_INVAL);
    FAILS(e, mpx_unmarshal_frames(e, nullptr, b.size(), nullptr, 0, &o, &res), MPX_E_INVAL);
    mpx_unmarshal_out x = o;
    x.accepts = nullptr;
    FAILS(e, call(f, 3, b.size(), x), MPX_E_INVAL);
    x = o;
    x.accept_last_committed = nullptr;
    FAILS(e, call(f, 3, b.size(), x), MPX_E_INVAL);
    x = o;
    x.commits = nullptr;
    FAILS(e, call(f, 3, b.size(), x), MPX_E_INVAL);
    x = o;
    x.key = nullptr;
    FAILS(e, call(f, 3, b.size(), x), MPX_E_INVAL);
    x = o;
    x.log_recs = nullptr;
    FAILS(e, call(f, 3, b.size(), x), MPX_E_INVAL);
    x = o;
    x.log_val = nullptr;
    FAILS(e, call(f, 3, b.size(), x), MPX_E_INVAL);
    // a frame outside [0, len): the buffer one byte short, an offset at len, a length of 0
    FAILS(e, call(f, 3, b.size() - 1, o), MPX_E_INVAL);
    mpx_var_frame g[3];
    auto reset = [&] { memcpy(g, f, sizeof(g)); };
    reset();
    g[2].offset = (uint32_t)b.size();
    FAILS(e, call(g, 3, b.size(), o), MPX_E_INVAL);
    reset();
    g[2].length = 0;
    FAILS(e, call(g, 3, b.size(), o), MPX_E_INVAL);
    reset();
    g[2].offset = 0xFFFFFFF0u;  // offset + length must not wrap
    g[2].length = 0x20u;
    FAILS(e, call(g, 3, b.size(), o), MPX_E_INVAL);
    // the Command slice: past the frame's end, before the header's end, a count that overflows
    reset();
    g[1].n_cmds = 2;
    FAILS(e, call(g, 3, b.size(), o), MPX_E_INVAL);
    reset();
    g[1].cmds_off = g[1].offset + 12;
    FAILS(e, call(g, 3, b.size(), o), MPX_E_INVAL);
    reset();
    g[1].cmds_off = g[1].offset + g[1].length + 1;
    g[1].n_cmds = 0;
    FAILS(e, call(g, 3, b.size(), o), MPX_E_INVAL);
    reset();
    g[0].n_cmds = 0xF0F0F0F1u;  // 17 n wraps 32 bits
    FAILS(e, call(g, 3, b.size(), o), MPX_E_INVAL);
    // log_off outside the frame or inside the Command slice
    reset();
    g[0].log_off = g[0].offset + g[0].length + 1;
    FAILS(e, call(g, 3, b.size(), o), MPX_E_INVAL);
    reset();
    g[0].log_off = g[0].cmds_off + 16;
    FAILS(e, call(g, 3, b.size(), o), MPX_E_INVAL);
    // n_log: more instances than the frame's bytes hold; any on a frame without a log
    reset();
    g[0].n_log = 1000;
    FAILS(e, call(g, 3, b.size(), o), MPX_E_INVAL);
    reset();
    g[1].n_log = 1;
    FAILS(e, call(g, 3, b.size(), o), MPX_E_INVAL);
    // a code other than 9, 10 or 12
    for (uint8_t code : {(uint8_t)0, (uint8_t)MPX_PEER_PREPARE, (uint8_t)MPX_PEER_COMMIT_SHORT,
                         (uint8_t)MPX_PEER_ACCEPT_REPLY, (uint8_t)255}) {
        reset();
        g[1].code = code;
        FAILS(e, call(g, 3, b.size(), o), MPX_E_INVAL);
    }
    // frames that overlap, and frames not ascending by offset
    reset();
    g[0].length += 1;
    FAILS(e, call(g, 3, b.size(), o), MPX_E_INVAL);
    reset();
    std::swap(g[0], g[1]);
    FAILS(e, call(g, 3, b.size(), o), MPX_E_INVAL);
    reset();
    g[1] = g[0];
    FAILS(e, call(g, 3, b.size(), o), MPX_E_INVAL);
    // a reserve beyond the record limit, and the device form: null arguments, a misaligned buffer
    FAILS(e, mpx_unmarshal_frames_reserve(e, (size_t)1 << 33, 16), MPX_E_UNSUPPORTED);
    alignas(16) uint8_t ab[256];
    memcpy(ab, b.data(), b.size());
    FAILS(e, mpx_unmarshal_frames_dev(e, ab, b.size(), f, 3, nullptr, nullptr, &res, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_unmarshal_frames_dev(e, ab, b.size(), f, 3, nullptr, &o, nullptr, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_unmarshal_frames_dev(e, nullptr, b.size(), f, 3, nullptr, &o, &res, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_unmarshal_frames_dev(e, ab + 8, b.size(), f, 3, nullptr, &o, &res, nullptr), MPX_E_INVAL);
    // the device form never allocates: it needs its reserve call first (no host form has run yet)
    FAILS(e, mpx_unmarshal_frames_dev(e, ab, b.size(), f, 3, nullptr, &o, &res, nullptr), MPX_E_INVAL);
    CHECK(strstr(mpx_last_error(e), "mpx_unmarshal_frames_dev") && strstr(mpx_last_error(e), "mpx_unmarshal_frames_reserve"));
    CHECK(mpx_unmarshal_frames_reserve(e, 16, 16) == MPX_OK);
    CHECK(mpx_unmarshal_frames_dev(e, ab, b.size(), f, 3, nullptr, &o, &res, nullptr) == MPX_OK);
    CHECK(res.n_var == 3 && res.n_accepts == 1 && res.n_commits == 1 && res.n_cmds == 3);
    const Caps all{2, 2, 4, 2, 4}, zero{0, 0, 0, 0, 0};
    unmarshal_case(e, b, f, 3, all, true, true, true);
    unmarshal_case(e, b, f, 3, zero, false, false, true);
    // valid calls of the host form
    CHECK(call(f, 3, b.size(), o) == MPX_OK);
    CHECK(res.n_var == 3 && res.n_log_inst == (min ? 1u : 0u));
    CHECK(call(f + 1, 2, b.size(), o) == MPX_OK && res.n_var == 2);  // (gaps between frames are legal)
    CHECK(call(f, 0, b.size(), o) == MPX_OK && res.n_var == 0);
    mpx_unmarshal_out none{};
    CHECK(call(f, 3, b.size(), none) == MPX_OK && res.n_cmds == 3);  // capacities of 0, null arrays
    CHECK(mpx_unmarshal_frames(e, nullptr, 0, nullptr, 0, &none, &res) == MPX_OK && res.n_var == 0);
    // ... on guarded buffers: every array given; capacities below the counts (the log's command
    // capacity above them: the second copy takes res->n_log_cmds of it); the offset arrays absent;
    // capacities of 0 with null arrays; fewer frames and none
    unmarshal_case(e, b, f, 3, all, true, true, false);
    unmarshal_case(e, b, f, 3, Caps{0, 0, 2, 0, 3}, true, true, false);
    unmarshal_case(e, b, f, 3, Caps{1, 1, 3, 1, 1}, true, true, false);
    unmarshal_case(e, b, f, 3, all, false, true, false);
    unmarshal_case(e, b, f, 3, zero, true, false, false);
    unmarshal_case(e, b, f, 3, zero, false, false, false);
    unmarshal_case(e, b, f, 1, all, true, true, false);
    unmarshal_case(e, b, f, 0, all, true, true, false);
    // ... and of a size at which the arrays have slots of more than one 256-byte unit
    std::vector<uint8_t> bb;
    std::vector<mpx_var_frame> ff;
    build_many(mode, 100, bb, ff);
    unmarshal_case(e, bb, ff.data(), 300, Caps{100, 100, 300, 100, 100}, true, true, false);
    unmarshal_case(e, bb, ff.data(), 300, Caps{120, 80, 290, 120, 70}, true, true, false);
    unmarshal_case(e, bb, ff.data(), 299, Caps{120, 120, 320, 120, 120}, false, true, false);
}

int main() {
    for (int mode : {MPX_MODE_MIN, MPX_MODE_CLASSIC}) {
        mpx_engine* e = nullptr;
        mpx_config cfg{3, mode, 1 << 10, 0, 0, 0};
        CHECK(mpx_open(0, &cfg, &e) == MPX_OK && e);
        if (!e) return 1;
        run(e, mode);
        CHECK(mpx_close(e) == MPX_OK);
    }
    mpx_unmarshal_out o{};
    mpx_unmarshal_result r;
    CHECK(mpx_unmarshal_frames(nullptr, nullptr, 0, nullptr, 0, &o, &r) == MPX_E_INVAL);
    CHECK(mpx_unmarshal_frames_reserve(nullptr, 1, 1) == MPX_E_INVAL);
    CHECK(mpx_unmarshal_frames_dev(nullptr, nullptr, 0, nullptr, 0, nullptr, &o, &r, nullptr) == MPX_E_INVAL);
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("unmarshal_driver: all checks passed\n");
    return failures ? 1 : 0;
}
