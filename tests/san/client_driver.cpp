// tests/san/client_driver.cpp — TEST INFRASTRUCTURE ONLY: drives mpx_decode_client_streams and its
// _reserve / _dev forms of the CPU build of engine.cpp + client.cpp over the stub runtime
// (hip_stub.cpp) and the framing stand-in of client_stub.cpp under ASan + UBSan. Every
// argument-validation path of both forms must answer its code before anything is staged or
// launched; valid calls on guarded buffers must bring back exactly the expected proposals,
// offsets and records through the staging arena, leave the inputs and the guard bytes alone and
// write nothing past the proposals the call produced. Exit status 0 = all checks passed.
#include <algorithm>
#include <string>

#include "san_check.hpp"

static mpx_engine* open_engine() {
    mpx_engine* e = nullptr;
    mpx_config cfg{5, MPX_MODE_MIN, 1 << 10, 0, 0, 0};
    CHECK(mpx_open(0, &cfg, &e) == MPX_OK && e);
    return e;
}

static bool guards_intact(const Out& o) {
    for (size_t i = o.bytes; i < o.v.size(); ++i)
        if (o.v[i] != kGuardByte) return false;
    return true;
}
static bool tail_untouched(const Out& o, size_t from) {
    for (size_t i = from; i < o.v.size(); ++i)
        if (o.v[i] != kGuardByte) return false;
    return true;
}

static std::string propose(int32_t id, uint8_t op, int64_t k, int64_t v, int64_t ts) {
    std::string s(30, '\0');
    memcpy(&s[1], &id, 4);
    s[5] = (char)op;
    memcpy(&s[6], &k, 8);
    memcpy(&s[14], &v, 8);
    memcpy(&s[22], &ts, 8);
    return s;
}

// conns[k] holds n_props[k] Proposes, then `tail[k]` bytes of a cut-off READ; laid out at
// 128-byte offsets in a guarded input; the outputs exactly cap long, guarded
static void valid_case(mpx_engine* e, std::vector<int> n_props, std::vector<int> tail,
                       std::vector<uint32_t> groups, size_t n_groups, size_t cap_short, bool dev) {
    const size_t C = n_props.size();
    std::vector<mpx_client_conn> conns(C ? C : 1);
    std::vector<std::string> bytes(C);
    size_t at = 0, total = 0;
    for (size_t k = 0; k < C; ++k) {
        bytes[k] += std::string(1, (char)0x07);  // an unknown byte first
        for (int i = 0; i < n_props[k]; ++i)
            bytes[k] += propose((int32_t)(k * 1000 + i), (uint8_t)(i & 7), -(int64_t)i, (int64_t)k, 77 + i);
        const std::string rd = std::string(1, (char)MPX_CLIENT_READ) + std::string(12, (char)0x04);
        bytes[k] += rd.substr(0, tail[k]);
        conns[k] = mpx_client_conn{at, (uint32_t)bytes[k].size(), groups[k]};
        at += (bytes[k].size() + 127) / 128 * 128;
        total += n_props[k];
    }
    const size_t len = at;
    In buf(len, 5);
    memset(buf.v.data(), 0, len);
    for (size_t k = 0; k < C; ++k) memcpy(buf.v.data() + conns[k].offset, bytes[k].data(), bytes[k].size());
    buf.orig = buf.v;
    In cin = holding(conns.data(), C, 6);
    const size_t cap = total - std::min(total, cap_short);
    Out op(cap), key(cap * 8), val(cap * 8), meta(cap * 16), po((n_groups + 1) * 8),
        so((n_groups + 1) * 8), cr(C * sizeof(mpx_client_conn_result));
    mpx_client_result res[2];
    memset(res, 0x5C, sizeof(res));
    mpx_client_out out{cap ? op.as<uint8_t>() : nullptr, cap ? key.as<int64_t>() : nullptr,
                       cap ? val.as<int64_t>() : nullptr, cap ? meta.as<mpx_proposal>() : nullptr,
                       cap, po.as<uint64_t>(), so.as<uint64_t>()};
    if (dev) {
        CHECK(mpx_decode_client_streams_reserve(e, len, C, n_groups) == MPX_OK);
        CHECK(mpx_decode_client_streams_dev(e, buf.as<uint8_t>(), len, cin.as<mpx_client_conn>(), C,
                                            n_groups, &out, cr.as<mpx_client_conn_result>(), res,
                                            nullptr) == MPX_OK);
        CHECK(mpx_synchronize(e) == MPX_OK);
    } else {
        CHECK(mpx_decode_client_streams(e, buf.as<uint8_t>(), len, cin.as<mpx_client_conn>(), C,
                                        n_groups, &out, cr.as<mpx_client_conn_result>(),
                                        res) == MPX_OK);
    }
    CHECK(buf.intact() && cin.intact());
    CHECK(res[0].n_proposals == total && res[0].n_dropped == C);
    size_t i = 0, partial = 0;
    std::vector<uint64_t> first(C);
    for (size_t k = 0; k < C; ++k) {
        const mpx_client_conn_result r = cr.as<mpx_client_conn_result>()[k];
        first[k] = i;
        CHECK(r.first == i && r.n_proposals == (uint32_t)n_props[k] && r.n_dropped == 1 && r.pad == 0);
        CHECK(r.consumed == 1u + 30u * n_props[k]);
        CHECK(tail[k] ? r.stop_reason == MPX_DECODE_PARTIAL && r.stop_code == MPX_CLIENT_READ
                      : r.stop_reason == MPX_DECODE_END && r.stop_code == -1);
        partial += tail[k] != 0;
        for (int j = 0; j < n_props[k]; ++j, ++i) {
            if (i >= cap) continue;
            const mpx_proposal m = meta.as<mpx_proposal>()[i];
            CHECK(op.as<uint8_t>()[i] == (uint8_t)(j & 7) && key.as<int64_t>()[i] == -(int64_t)j &&
                  val.as<int64_t>()[i] == (int64_t)k && m.timestamp == 77 + j &&
                  m.command_id == (int32_t)(k * 1000 + j) && m.client == k);
        }
    }
    CHECK(res[0].n_partial == partial);
    // offsets against a direct count
    uint64_t sends = 0;
    for (size_t g = 0; g <= n_groups; ++g) {
        uint64_t at_g = total, nx = total;
        for (size_t k = C; k-- > 0;) {
            if (groups[k] >= g) at_g = first[k];
            if (groups[k] >= g + 1) nx = first[k];
        }
        CHECK(po.as<uint64_t>()[g] == at_g && so.as<uint64_t>()[g] == sends);
        if (g < n_groups) sends += (nx - at_g + MPX_PROPOSE_MAX_BATCH - 1) / MPX_PROPOSE_MAX_BATCH;
    }
    CHECK(res[0].n_sends == sends);
    const size_t wrote = std::min(total, cap);
    CHECK(tail_untouched(op, wrote) && tail_untouched(key, wrote * 8) && tail_untouched(val, wrote * 8) &&
          tail_untouched(meta, wrote * 16));
    CHECK(guards_intact(po) && guards_intact(so) && guards_intact(cr));
    const uint8_t* after = (const uint8_t*)&res[1];
    for (size_t b = 0; b < sizeof(res[1]); ++b) CHECK(after[b] == 0x5C);
}

static void validation(mpx_engine* e) {
    alignas(16) uint8_t buf[512] = {0};
    alignas(16) mpx_client_conn conns[3] = {{0, 60, 0}, {128, 30, 1}, {256, 90, 1}};
    Out op(8), key(64), val(64), meta(128), po(24), so(24), cr(96);
    mpx_client_result res;
    memset(&res, 0x5C, sizeof(res));
    mpx_client_out out{op.as<uint8_t>(), key.as<int64_t>(), val.as<int64_t>(), meta.as<mpx_proposal>(),
                       8, po.as<uint64_t>(), so.as<uint64_t>()};
    mpx_client_conn_result* crp = cr.as<mpx_client_conn_result>();
    auto host = [&](const mpx_client_conn* c, size_t n, size_t ng, const mpx_client_out* o) {
        return mpx_decode_client_streams(e, buf, sizeof(buf), c, n, ng, o, crp, &res);
    };
    auto dev = [&](const uint8_t* b, const mpx_client_conn* c, size_t n, size_t ng,
                   const mpx_client_out* o, mpx_client_conn_result* r, mpx_client_result* rs) {
        return mpx_decode_client_streams_dev(e, b, sizeof(buf), c, n, ng, o, r, rs, nullptr);
    };
    CHECK(mpx_decode_client_streams_reserve(e, sizeof(buf), 3, 2) == MPX_OK);
    // null arguments (both forms share the checks)
    FAILS(e, host(conns, 3, 2, nullptr), MPX_E_INVAL);
    FAILS(e, host(nullptr, 3, 2, &out), MPX_E_INVAL);
    FAILS(e, mpx_decode_client_streams(e, nullptr, sizeof(buf), conns, 3, 2, &out, crp, &res), MPX_E_INVAL);
    FAILS(e, mpx_decode_client_streams(e, buf, sizeof(buf), conns, 3, 2, &out, nullptr, &res), MPX_E_INVAL);
    FAILS(e, mpx_decode_client_streams(e, buf, sizeof(buf), conns, 3, 2, &out, crp, nullptr), MPX_E_INVAL);
    FAILS(e, dev(buf, conns, 3, 2, nullptr, crp, &res), MPX_E_INVAL);
    FAILS(e, dev(buf, nullptr, 3, 2, &out, crp, &res), MPX_E_INVAL);
    FAILS(e, dev(buf, conns, 3, 2, &out, nullptr, &res), MPX_E_INVAL);
    FAILS(e, dev(buf, conns, 3, 2, &out, crp, nullptr), MPX_E_INVAL);
    mpx_client_out no_key = out;
    no_key.key = nullptr;  // a capacity with a null array
    FAILS(e, host(conns, 3, 2, &no_key), MPX_E_INVAL);
    FAILS(e, dev(buf, conns, 3, 2, &no_key, crp, &res), MPX_E_INVAL);
    // prop_off / send_off with n_groups == 0
    mpx_client_out only_so = out;
    only_so.prop_off = nullptr;
    FAILS(e, host(conns, 0, 0, &out), MPX_E_INVAL);
    FAILS(e, host(conns, 0, 0, &only_so), MPX_E_INVAL);
    FAILS(e, dev(buf, conns, 0, 0, &only_so, crp, &res), MPX_E_INVAL);
    // the connections, host form: offset not a multiple of 128, outside [0, len], overlapping, out
    // of order, group decreasing or >= n_groups
    auto with = [&](int k, mpx_client_conn c) {
        std::vector<mpx_client_conn> v(conns, conns + 3);
        v[k] = c;
        return v;
    };
    FAILS(e, host(with(1, {64, 30, 1}).data(), 3, 2, &out), MPX_E_INVAL);
    FAILS(e, host(with(2, {256, 257, 1}).data(), 3, 2, &out), MPX_E_INVAL);
    FAILS(e, host(with(2, {640, 0, 1}).data(), 3, 2, &out), MPX_E_INVAL);
    FAILS(e, host(with(1, {0, 30, 1}).data(), 3, 2, &out), MPX_E_INVAL);
    FAILS(e, host(with(0, {0, 129, 0}).data(), 3, 2, &out), MPX_E_INVAL);
    FAILS(e, host(with(1, {384, 30, 1}).data(), 3, 2, &out), MPX_E_INVAL);
    FAILS(e, host(with(2, {256, 90, 0}).data(), 3, 2, &out), MPX_E_INVAL);
    FAILS(e, host(with(2, {256, 90, 2}).data(), 3, 2, &out), MPX_E_INVAL);
    FAILS(e, host(conns, 3, 1, &out), MPX_E_INVAL);
    // the limits
    FAILS(e, mpx_decode_client_streams(e, buf, (size_t)MPX_DECODE_MAX_BYTES + 1, conns, 3, 2, &out, crp, &res), MPX_E_UNSUPPORTED);
    FAILS(e, host(conns, (size_t)MPX_CLIENT_MAX_CONNS + 1, 2, &out), MPX_E_UNSUPPORTED);
    FAILS(e, host(conns, 3, (size_t)MPX_CLIENT_MAX_GROUPS + 1, &out), MPX_E_UNSUPPORTED);
    FAILS(e, dev(buf, conns, (size_t)MPX_CLIENT_MAX_CONNS + 1, 2, &out, crp, &res), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_decode_client_streams_reserve(e, (size_t)MPX_DECODE_MAX_BYTES + 1, 1, 1), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_decode_client_streams_reserve(e, 1, (size_t)MPX_CLIENT_MAX_CONNS + 1, 1), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_decode_client_streams_reserve(e, 1, 1, (size_t)MPX_CLIENT_MAX_GROUPS + 1), MPX_E_UNSUPPORTED);
    // the device form's alignment rules
    FAILS(e, dev(buf + 8, conns, 3, 2, &out, crp, &res), MPX_E_INVAL);
    FAILS(e, dev(buf, (const mpx_client_conn*)((const char*)conns + 8), 3, 2, &out, crp, &res), MPX_E_INVAL);
    FAILS(e, dev(buf, conns, 3, 2, &out, (mpx_client_conn_result*)((char*)crp + 8), &res), MPX_E_INVAL);
    FAILS(e, dev(buf, conns, 3, 2, &out, crp, (mpx_client_result*)((char*)&res + 4)), MPX_E_INVAL);
    for (int f = 0; f < 5; ++f) {
        mpx_client_out o = out;
        if (f == 0) o.meta = (mpx_proposal*)((char*)o.meta + 8);
        if (f == 1) o.key = (int64_t*)((char*)o.key + 4);
        if (f == 2) o.val = (int64_t*)((char*)o.val + 4);
        if (f == 3) o.prop_off = (uint64_t*)((char*)o.prop_off + 4);
        if (f == 4) o.send_off = (uint64_t*)((char*)o.send_off + 4);
        FAILS(e, dev(buf, conns, 3, 2, &o, crp, &res), MPX_E_INVAL);
    }
    // nothing was touched
    CHECK(op.untouched() && key.untouched() && val.untouched() && meta.untouched() && po.untouched() &&
          so.untouched() && cr.untouched());
    const uint8_t* rb = (const uint8_t*)&res;
    for (size_t i = 0; i < sizeof(res); ++i) CHECK(rb[i] == 0x5C);
    // the device form reports a faulty connection through the error word: MPX_E_INVAL at the next
    // synchronising call, the connection frames nothing, its neighbours do
    {
        alignas(16) mpx_client_conn bad[3] = {{0, 60, 0}, {64, 30, 1}, {256, 90, 1}};
        CHECK(dev(buf, bad, 3, 2, &out, crp, &res) == MPX_OK);
        FAILS(e, mpx_synchronize(e), MPX_E_INVAL);
        CHECK(res.n_proposals == 5 && crp[1].consumed == 0 && crp[1].n_proposals == 0 &&
              crp[1].first == 2 && crp[2].first == 2 && crp[2].n_proposals == 3);
    }
    // ... and the same layout is legal once repaired; op may sit at any address
    mpx_client_out odd = out;
    odd.op = op.as<uint8_t>() + 1;
    odd.prop_cap = 5;
    CHECK(dev(buf, conns, 3, 2, &odd, crp, &res) == MPX_OK && mpx_synchronize(e) == MPX_OK);
    CHECK(host(conns, 3, 2, &out) == MPX_OK);
    CHECK(res.n_proposals == 6 && res.n_sends == 2 && res.n_partial == 0 && res.n_dropped == 0);
    CHECK(po.as<uint64_t>()[0] == 0 && po.as<uint64_t>()[1] == 2 && po.as<uint64_t>()[2] == 6);
    // no connection, no group, no capacity: legal, with null arrays
    mpx_client_out none{nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr};
    CHECK(mpx_decode_client_streams(e, nullptr, 0, nullptr, 0, 0, &none, nullptr, &res) == MPX_OK);
    CHECK(res.n_proposals == 0 && res.n_sends == 0);
    // a capacity of 0 with null arrays still counts
    CHECK(host(conns, 3, 2, &none) == MPX_OK && res.n_proposals == 6 && res.n_sends == 2);
}

int main() {
    mpx_engine* e = open_engine();
    if (!e) return 1;
    validation(e);
    for (const size_t cap_short : {(size_t)0, (size_t)1, (size_t)1000000}) {
        valid_case(e, {2}, {0}, {0}, 1, cap_short, false);
        valid_case(e, {0, 7, 0, 9}, {0, 5, 0, 12}, {0, 0, 2, 2}, 4, cap_short, false);
        // ... of a size at which the arrays have slots of more than one 256-byte unit
        valid_case(e, {300, 17, 0, 211}, {1, 0, 0, 3}, {1, 1, 1, 3}, 5, cap_short, false);
        valid_case(e, {}, {}, {}, 3, cap_short, false);
        valid_case(e, {0, 0}, {0, 0}, {0, 1}, 2, cap_short, false);
    }
    // the device form never allocates: on a fresh handle it needs its reserve call first (a call
    // of no connection does not)
    mpx_engine* f = open_engine();
    if (!f) return 1;
    {
        alignas(16) uint8_t buf[4096] = {0};
        alignas(16) mpx_client_conn c[1] = {{0, 60, 0}};
        alignas(16) mpx_client_conn_result cr[1];
        alignas(16) mpx_proposal meta[2];
        uint8_t op[2];
        int64_t key[2], val[2];
        uint64_t po[2], so[2];
        mpx_client_result res;
        mpx_client_out out{op, key, val, meta, 2, po, so};
        FAILS(f, mpx_decode_client_streams_dev(f, buf, 4096, c, 1, 1, &out, cr, &res, nullptr), MPX_E_INVAL);
        CHECK(strstr(mpx_last_error(f), "mpx_decode_client_streams_dev") &&
              strstr(mpx_last_error(f), "mpx_decode_client_streams_reserve"));
        CHECK(mpx_decode_client_streams_dev(f, buf, 4096, c, 0, 1, &out, nullptr, &res, nullptr) == MPX_OK);
        CHECK(res.n_proposals == 0 && po[1] == 0 && so[1] == 0);
        CHECK(mpx_decode_client_streams_reserve(f, 64, 1, 1) == MPX_OK);
        FAILS(f, mpx_decode_client_streams_dev(f, buf, 4096, c, 1, 1, &out, cr, &res, nullptr), MPX_E_INVAL);
        CHECK(mpx_decode_client_streams_reserve(f, 4096, 1, 1) == MPX_OK);
        CHECK(mpx_decode_client_streams_dev(f, buf, 4096, c, 1, 1, &out, cr, &res, nullptr) == MPX_OK);
        CHECK(mpx_synchronize(f) == MPX_OK && res.n_proposals == 2 && cr[0].consumed == 60);
    }
    valid_case(f, {300, 17, 0, 211}, {1, 0, 0, 3}, {1, 1, 1, 3}, 5, 0, true);
    valid_case(f, {300, 17, 0, 211}, {1, 0, 0, 3}, {1, 1, 1, 3}, 5, 100, true);
    CHECK(mpx_close(f) == MPX_OK);
    CHECK(mpx_close(e) == MPX_OK);
    mpx_client_out none{nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr};
    mpx_client_result res;
    CHECK(mpx_decode_client_streams(nullptr, nullptr, 0, nullptr, 0, 0, &none, nullptr, &res) == MPX_E_INVAL);
    CHECK(mpx_decode_client_streams_reserve(nullptr, 1, 1, 1) == MPX_E_INVAL);
    CHECK(mpx_decode_client_streams_dev(nullptr, nullptr, 0, nullptr, 0, 0, &none, nullptr, &res, nullptr) == MPX_E_INVAL);
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("client_driver: all checks passed\n");
    return failures ? 1 : 0;
}
