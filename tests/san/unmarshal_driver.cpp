// tests/san/unmarshal_driver.cpp — TEST INFRASTRUCTURE ONLY: drives mpx_unmarshal_frames and its
// _reserve / _dev forms of the CPU build of engine.cpp over the stub runtime (hip_stub.cpp) under
// ASan + UBSan. The stub has no stand-ins for the unmarshal launchers, so the weak symbols stay
// null: every validation path of the host form must answer its code before that is looked at,
// and a valid call answers MPX_E_UNSUPPORTED. Exit status 0 = all checks passed.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <utility>
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
    // valid calls: the kernels are not in this build
    FAILS(e, call(f, 3, b.size(), o), MPX_E_UNSUPPORTED);
    FAILS(e, call(f + 1, 2, b.size(), o), MPX_E_UNSUPPORTED);  // (gaps between frames are legal)
    FAILS(e, call(f, 0, b.size(), o), MPX_E_UNSUPPORTED);
    mpx_unmarshal_out none{};
    FAILS(e, call(f, 3, b.size(), none), MPX_E_UNSUPPORTED);  // capacities of 0, null arrays
    FAILS(e, mpx_unmarshal_frames(e, nullptr, 0, nullptr, 0, &none, &res), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_unmarshal_frames_reserve(e, 16, 16), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_unmarshal_frames_reserve(e, (size_t)1 << 33, 16), MPX_E_UNSUPPORTED);
    // the device form: null arguments, a misaligned buffer
    alignas(16) uint8_t ab[256];
    memcpy(ab, b.data(), b.size());
    FAILS(e, mpx_unmarshal_frames_dev(e, ab, b.size(), f, 3, nullptr, nullptr, &res, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_unmarshal_frames_dev(e, ab, b.size(), f, 3, nullptr, &o, nullptr, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_unmarshal_frames_dev(e, nullptr, b.size(), f, 3, nullptr, &o, &res, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_unmarshal_frames_dev(e, ab + 8, b.size(), f, 3, nullptr, &o, &res, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_unmarshal_frames_dev(e, ab, b.size(), f, 3, nullptr, &o, &res, nullptr), MPX_E_UNSUPPORTED);
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
