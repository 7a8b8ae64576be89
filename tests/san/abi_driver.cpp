// tests/san/abi_driver.cpp — TEST INFRASTRUCTURE ONLY: drives every host entry point of
// include/mpx.h over the stub runtime (hip_stub.cpp) with invalid and valid arguments, under
// ASan + UBSan. Checks return codes and that every failure on a live handle explains itself
// (mpx_last_error), and that every host form stages its arrays whole and apart ("staging
// checks" in san_check.hpp). Exit status 0 = all checks passed.
#include "san_check.hpp"

static void tally_case(mpx_engine* e, size_t n, size_t n_inst) {
    In recs(n * sizeof(mpx_accept_reply), 1), st(n_inst * sizeof(mpx_inst_state), 2), pc(5 * 4, 3);
    Out dec(n_inst);
    int32_t cu = 0x01234567;
    CHECK(mpx_accept_tally(e, recs.as<mpx_accept_reply>(), n, st.as<mpx_inst_state>(), n_inst, 0,
                           &cu, pc.as<int32_t>(), dec.as<uint8_t>()) == MPX_OK);
    CHECK(recs.intact() && st.intact() && pc.flipped() && cu == ~0x01234567 && dec.is(0));
    CHECK(mpx_accept_tally(e, recs.as<mpx_accept_reply>(), n, st.as<mpx_inst_state>(), n_inst, 0,
                           &cu, pc.as<int32_t>(), nullptr) == MPX_OK);
    CHECK(st.intact() && pc.intact() && cu == 0x01234567);  // (inverted twice)
    CHECK(mpx_committed_prefix(e, st.as<mpx_inst_state>(), n_inst, 0, &cu) == MPX_OK);
    CHECK(st.intact() && cu == ~0x01234567);
}

static void prepare_case(mpx_engine* e, size_t n, size_t n_inst) {
    In recs(n * sizeof(mpx_prepare_reply), 4), st(n_inst * sizeof(mpx_prep_state), 5);
    Out prep(n_inst);
    int32_t db = 0x07654321;
    CHECK(mpx_prepare_select(e, recs.as<mpx_prepare_reply>(), n, st.as<mpx_prep_state>(), n_inst,
                             0, &db, prep.as<uint8_t>()) == MPX_OK);
    CHECK(recs.intact() && st.intact() && db == ~0x07654321 && prep.is(0));
    // MIN: G groups of n / G records
    const size_t G = 3, N = 5;
    std::vector<uint64_t> off(G + 1);
    for (size_t g = 0; g <= G; ++g) off[g] = n * g / G;
    In rmin(n * sizeof(mpx_prepare_reply_min), 6), gst(G * sizeof(mpx_group_prep_state), 7),
        gpc(G * N * 4, 8);
    Out eff(n * sizeof(mpx_prepare_effect));
    CHECK(mpx_prepare_select_min(e, rmin.as<mpx_prepare_reply_min>(), n, off.data(),
                                 gst.as<mpx_group_prep_state>(), G, gpc.as<int32_t>(),
                                 eff.as<mpx_prepare_effect>()) == MPX_OK);
    CHECK(rmin.intact() && gst.intact() && gpc.flipped() && eff.is(0));
    CHECK(mpx_prepare_select_min(e, rmin.as<mpx_prepare_reply_min>(), n, off.data(),
                                 gst.as<mpx_group_prep_state>(), G, gpc.as<int32_t>(),
                                 nullptr) == MPX_OK);
    CHECK(gst.intact() && gpc.intact());  // (inverted twice)
}

// e: a handle with apply_path SORTED, so that a small call stages through the arena too
static void apply_case(mpx_engine* e, size_t m) {
    In op(m, 9), key(m * 8, 10), val(m * 8, 11);
    Out ret(m * 8), conf(m);
    CHECK(mpx_apply(e, op.as<uint8_t>(), key.as<int64_t>(), val.as<int64_t>(), m,
                    ret.as<int64_t>(), conf.as<uint8_t>()) == MPX_OK);
    CHECK(op.intact() && key.intact() && val.intact() && ret.is(0) && conf.is(1));
    Out ret2(m * 8);
    CHECK(mpx_apply(e, op.as<uint8_t>(), key.as<int64_t>(), val.as<int64_t>(), m,
                    ret2.as<int64_t>(), nullptr) == MPX_OK);
    CHECK(ret2.is(0));
    // consecutive instances of m / n_inst commands
    const size_t n_inst = 5;
    std::vector<uint64_t> off(n_inst + 1);
    for (size_t i = 0; i <= n_inst; ++i) off[i] = m * i / n_inst;
    Out cb(n_inst - 1);
    CHECK(mpx_conflict_batch(e, op.as<uint8_t>(), key.as<int64_t>(), off.data(), n_inst,
                             cb.as<uint8_t>()) == MPX_OK);
    CHECK(cb.is(0));
    CHECK(mpx_kv_import(e, key.as<int64_t>(), val.as<int64_t>(), m) == MPX_OK);
    CHECK(key.intact() && val.intact());
}

// G groups of ipg instances, 4 replies and cpi commands each, N = 5, kv_per_group = 64
static void group_case(mpx_engine* e, uint32_t G, uint32_t ipg, uint32_t cpi, bool optional) {
    const size_t ni = (size_t)G * ipg, nr = ni * 4, m = ni * cpi, N = 5, K = 64;
    std::vector<uint64_t> roff(G + 1);
    for (size_t g = 0; g <= G; ++g) roff[g] = g * ipg * 4;
    std::vector<uint32_t> coff(ni + 1);
    for (size_t i = 0; i <= ni; ++i) coff[i] = (uint32_t)(i * cpi);
    In recs(nr * sizeof(mpx_accept_reply), 12), st(ni * sizeof(mpx_inst_state), 13), ci(G * 4, 14),
        ei(G * 4, 15), pin(G * N * 4, 16), op(m, 17), key(m * 8, 18), val(m * 8, 19), has(ni, 20),
        ret(m * 8, 21), conf(m, 22), kc(G * 4, 23), kk(G * K * 8, 24), kv(G * K * 8, 25);
    Out co(G * 4), eo(G * 4), pout(G * N * 4), kc2(G * 4), kk2(G * K * 8), kv2(G * K * 8), dec(ni),
        nd(G * 4);
    mpx_group_batch b{G, ipg, recs.as<mpx_accept_reply>(), roff.data(), st.as<mpx_inst_state>(),
                      st.as<mpx_inst_state>(), ci.as<int32_t>(), co.as<int32_t>(),
                      ei.as<int32_t>(), eo.as<int32_t>(), pin.as<int32_t>(), pout.as<int32_t>(),
                      op.as<uint8_t>(), key.as<int64_t>(), val.as<int64_t>(), coff.data(),
                      optional ? has.as<uint8_t>() : nullptr, ret.as<int64_t>(),
                      optional ? conf.as<uint8_t>() : nullptr, kc.as<uint32_t>(),
                      kk.as<int64_t>(), kv.as<int64_t>(), kc2.as<uint32_t>(), kk2.as<int64_t>(),
                      kv2.as<int64_t>(), optional ? dec.as<uint8_t>() : nullptr,
                      optional ? nd.as<uint32_t>() : nullptr};
    CHECK(mpx_group_step(e, &b) == MPX_OK);
    CHECK(recs.intact() && st.intact() && ci.intact() && ei.intact() && pin.intact());
    CHECK(op.intact() && key.intact() && val.intact() && has.intact());
    // in/out (unexecuted commands keep the caller's values); conf_prev only when asked for
    CHECK(ret.flipped() && (optional ? conf.flipped() : conf.intact()));
    CHECK(kc.intact() && kk.intact() && kv.intact());
    CHECK(co.is(0) && eo.is(1) && pout.is(2));
    // the tables come out as they went in (separate arrays on the host, one slot on the device)
    CHECK(carries(kc2, kc) && carries(kk2, kk) && carries(kv2, kv));
    if (optional) CHECK(dec.is(3) && nd.is(4));
    else CHECK(dec.untouched() && nd.untouched());
}

static void decode_case(mpx_engine* e, size_t len, size_t cap) {
    In buf(len, 26);
    Out ar(cap * sizeof(mpx_accept_reply)), oth(cap * sizeof(mpx_peer_frame)),
        res(sizeof(mpx_decode_result));
    CHECK(mpx_decode_peer_stream(e, buf.as<uint8_t>(), len, ar.as<mpx_accept_reply>(), cap,
                                 oth.as<mpx_peer_frame>(), cap,
                                 res.as<mpx_decode_result>()) == MPX_OK);
    CHECK(buf.intact() && ar.is(0) && oth.is(1) && res.is(2));
    Out ar2(cap * sizeof(mpx_accept_reply)), prep(cap * sizeof(mpx_prepare_reply_min)),
        var(cap * sizeof(mpx_var_frame)), oth2(cap * sizeof(mpx_peer_frame)),
        sres(sizeof(mpx_stream_result));
    const mpx_decode_out out{ar2.as<mpx_accept_reply>(), cap, prep.as<void>(), cap,
                             var.as<mpx_var_frame>(), cap, oth2.as<mpx_peer_frame>(), cap};
    CHECK(mpx_decode_stream(e, buf.as<uint8_t>(), len, &out, sres.as<mpx_stream_result>()) == MPX_OK);
    CHECK(buf.intact() && ar2.is(0) && prep.is(1) && var.is(2) && oth2.is(3) && sres.is(4));
}

static void fanout_case(mpx_engine* e, size_t n, uint32_t n_clients) {
    In recs(n * sizeof(mpx_reply_rec), 27);
    Out out(n * MPX_PROPOSE_REPLY_BYTES), off(((size_t)n_clients + 1) * 8);
    CHECK(mpx_encode_replies(e, recs.as<mpx_reply_rec>(), n, n_clients, 1, 0, out.as<uint8_t>(),
                             off.as<uint64_t>()) == MPX_OK);
    CHECK(recs.intact() && out.is(0) && off.is(1));
}

// n Accepts over G groups of ipg instances, then their n replies for n_dest destinations (MIN)
static void acceptor_case(mpx_engine* e, size_t n, size_t G, uint32_t ipg, uint32_t n_dest) {
    const size_t n_inst = G * ipg;
    In msgs(n * sizeof(mpx_accept_msg), 28), st(n_inst * sizeof(mpx_acceptor_state), 29),
        groups(G * sizeof(mpx_acceptor_group), 30);
    Out rep(n * sizeof(mpx_accept_reply)), to(n * 4), eff(n);
    CHECK(mpx_accept_handle(e, msgs.as<mpx_accept_msg>(), n, st.as<mpx_acceptor_state>(), n_inst,
                            0, groups.as<mpx_acceptor_group>(), G, ipg,
                            rep.as<mpx_accept_reply>(), to.as<int32_t>(),
                            eff.as<uint8_t>()) == MPX_OK);
    CHECK(msgs.intact() && st.intact() && groups.intact() && rep.is(0) && to.is(1) && eff.is(2));
    In replies(n * sizeof(mpx_accept_reply), 31), reply_to(n * 4, 32);
    Out bytes(n * MPX_ACCEPT_REPLY_FRAME_MIN);
    std::vector<uint64_t> doff(n_dest + 2, 0x5C5C5C5C5C5C5C5Cull);
    CHECK(mpx_encode_accept_replies(e, replies.as<mpx_accept_reply>(), reply_to.as<int32_t>(), n,
                                    n_dest, bytes.as<uint8_t>(), doff.data()) == MPX_OK);
    CHECK(replies.intact() && reply_to.intact() && bytes.is(0));
    for (uint32_t d = 0; d <= n_dest; ++d)
        CHECK(doff[d] == n * d / n_dest * MPX_ACCEPT_REPLY_FRAME_MIN);
    CHECK(doff[n_dest + 1] == 0x5C5C5C5C5C5C5C5Cull);
}

// n records of cpr commands; the last record takes none of the final `spare` commands
static void log_case(mpx_engine* e, size_t n, size_t cpr, size_t spare) {
    const size_t m = n * cpr + spare;
    std::vector<uint64_t> coff(n + 1);
    for (size_t i = 0; i <= n; ++i) coff[i] = i * cpr;
    In recs(n * sizeof(mpx_log_rec), 33), op(m, 34), key(m * 8, 35), val(m * 8, 36);
    const size_t want = 18 * n + 17 * n * cpr;  // the stub's encoding size (<= the bound)
    CHECK(want <= mpx_encode_log_bound(n, m));
    Out out(want);
    std::vector<uint64_t> roff(n + 2, 0x5C5C5C5C5C5C5C5Cull);
    CHECK(mpx_encode_log(e, MPX_LOG_DURABLE, recs.as<mpx_log_rec>(), n, coff.data(),
                         op.as<uint8_t>(), key.as<int64_t>(), val.as<int64_t>(), m,
                         out.as<uint8_t>(), out.cap(), roff.data()) == MPX_OK);
    CHECK(recs.intact() && op.intact() && key.intact() && val.intact() && out.is(0));
    for (size_t i = 0; i <= n; ++i) CHECK(roff[i] == 18 * i + 17 * coff[i]);
    CHECK(roff[n + 1] == 0x5C5C5C5C5C5C5C5Cull);
    if (want) FAILS(e, mpx_encode_log(e, MPX_LOG_DURABLE, recs.as<mpx_log_rec>(), n, coff.data(),
                                      op.as<uint8_t>(), key.as<int64_t>(), val.as<int64_t>(), m,
                                      out.as<uint8_t>(), want - 1, roff.data()), MPX_E_INVAL);
}

static void replay_case(mpx_engine* e, size_t n, int32_t inst_cap) {
    In log(n * MPX_DURABLE_REC_BYTES, 37), last((size_t)inst_cap * 4, 38), sc(2 * 4, 39);
    Out recs(n * sizeof(mpx_log_rec)), op(n), key(n * 8), val(n * 8);
    CHECK(mpx_replay_durable(e, log.as<uint8_t>(), n * MPX_DURABLE_REC_BYTES, inst_cap, 0,
                             recs.as<mpx_log_rec>(), op.as<uint8_t>(), key.as<int64_t>(),
                             val.as<int64_t>(), last.as<int32_t>(), sc.as<int32_t>()) == MPX_OK);
    CHECK(log.intact() && (n ? last.flipped() && sc.flipped() : last.intact() && sc.intact()));
    CHECK(recs.is(0) && op.is(1) && key.is(2) && val.is(3));  // (n == 0: all untouched)
}

// every family once, at a size of about `s` elements
static void all_families(mpx_engine* e, mpx_engine* e_sorted, size_t s) {
    tally_case(e, 4 * s, s);
    group_case(e, (uint32_t)(1 + s / 64), (uint32_t)(s < 64 ? s : 64), 2, s % 2 == 0);
    tally_case(e, s / 8 + 1, s / 16 + 1);  // a small call right after a much larger one
    prepare_case(e, 3 * s, s);
    apply_case(e_sorted, 3 * s + 1);
    decode_case(e, 13 * s + 5, s / 4 + 1);
    fanout_case(e, s, 7);
    acceptor_case(e, 2 * s, 1 + s / 64, (uint32_t)(s < 64 ? s : 64), 5);
    log_case(e, s, 3, s % 5);
    replay_case(e, s, (int32_t)(s / 2 + 1));
}

int main() {
    CHECK(mpx_abi_version() == MPX_ABI_VERSION);
    int n = -1;
    CHECK(mpx_device_count(&n) == MPX_OK && n == 1);
    mpx_config bad{0, MPX_MODE_MIN, 0, 0, 0, 0};
    mpx_engine* e = nullptr;
    CHECK(mpx_open(0, &bad, &e) == MPX_E_INVAL && !e);
    bad.n_replicas = 17;
    CHECK(mpx_open(0, &bad, &e) == MPX_E_INVAL);
    bad.n_replicas = 5;
    bad.mode = 7;
    CHECK(mpx_open(0, &bad, &e) == MPX_E_INVAL);
    bad.mode = MPX_MODE_MIN;
    bad.kv_per_group = 2048;
    CHECK(mpx_open(0, &bad, &e) == MPX_E_UNSUPPORTED);
    CHECK(mpx_open(3, &bad, &e) == MPX_E_NODEV);
    mpx_config cfg{5, MPX_MODE_MIN, 1 << 10, 64, 0, 16};
    CHECK(mpx_open(0, &cfg, &e) == MPX_OK && e);
    CHECK(mpx_stream(e) != nullptr);

    // A1/A2
    std::vector<mpx_accept_reply> ar(8);
    for (int i = 0; i < 8; ++i) ar[i] = mpx_accept_reply{i / 4, 16, 1 + i % 4, 1, {0, 0, 0}};
    std::vector<mpx_inst_state> st(2, mpx_inst_state{MPX_PREPARED, 0, 0, 0});
    int32_t cu = -1, pc[5] = {0};
    std::vector<uint8_t> dec(2);
    FAILS(e, mpx_accept_tally(e, nullptr, 8, st.data(), 2, 0, &cu, pc, dec.data()), MPX_E_INVAL);
    FAILS(e, mpx_accept_tally(e, ar.data(), 8, st.data(), 2, 0, nullptr, pc, dec.data()), MPX_E_INVAL);
    CHECK(mpx_accept_tally(e, ar.data(), 8, st.data(), 2, 0, &cu, pc, dec.data()) == MPX_OK);
    CHECK(mpx_accept_tally(e, ar.data(), 0, st.data(), 2, 0, &cu, pc, nullptr) == MPX_OK);
    FAILS(e, mpx_accept_tally_dev(e, ar.data(), 8, nullptr, nullptr, 2, 0, pc, nullptr, nullptr), MPX_E_INVAL);
    CHECK(mpx_committed_prefix(e, st.data(), 2, 0, &cu) == MPX_OK);
    FAILS(e, mpx_committed_prefix(e, nullptr, 2, 0, &cu), MPX_E_INVAL);

    // A4 / A3
    std::vector<mpx_prepare_reply> pr(8, mpx_prepare_reply{0, 16, 1, 3});
    std::vector<mpx_prep_state> ps(2);
    int32_t db = -1;
    CHECK(mpx_prepare_select(e, pr.data(), 8, ps.data(), 2, 0, &db, dec.data()) == MPX_OK);
    FAILS(e, mpx_prepare_select(e, pr.data(), 8, ps.data(), 2, 0, nullptr, nullptr), MPX_E_INVAL);
    std::vector<mpx_prepare_reply_min> pm(4);
    std::vector<mpx_group_prep_state> gs(2);
    std::vector<int32_t> gpc(10);
    std::vector<mpx_prepare_effect> eff(4);
    uint64_t off_ok[3] = {0, 2, 4}, off_bad0[3] = {1, 2, 4}, off_dec[3] = {0, 3, 2};
    CHECK(mpx_prepare_select_min(e, pm.data(), 4, off_ok, gs.data(), 2, gpc.data(), eff.data()) == MPX_OK);
    FAILS(e, mpx_prepare_select_min(e, pm.data(), 4, off_bad0, gs.data(), 2, gpc.data(), nullptr), MPX_E_INVAL);
    FAILS(e, mpx_prepare_select_min(e, pm.data(), 4, off_dec, gs.data(), 2, gpc.data(), nullptr), MPX_E_INVAL);

    // A5/A6
    const size_t m = 100;
    std::vector<uint8_t> op(m, MPX_OP_PUT), conf(m);
    std::vector<int64_t> key(m), val(m), ret(m);
    for (size_t i = 0; i < m; ++i) key[i] = (int64_t)(i % 7), val[i] = (int64_t)i;
    CHECK(mpx_apply(e, op.data(), key.data(), val.data(), m, ret.data(), conf.data()) == MPX_OK);
    FAILS(e, mpx_apply(e, op.data(), nullptr, val.data(), m, ret.data(), nullptr), MPX_E_INVAL);
    FAILS(e, mpx_apply_dev(e, op.data(), key.data(), val.data(), 1u << 20, ret.data(), nullptr, nullptr), MPX_E_INVAL);
    CHECK(mpx_apply_reserve(e, m) == MPX_OK);
    mpx_apply_io aio{};
    CHECK(mpx_apply_buffers(e, m, &aio) == MPX_OK && aio.cap >= m && aio.op && aio.conf);
    for (size_t i = 0; i < m; ++i) aio.op[i] = op[i], aio.key[i] = key[i], aio.val[i] = val[i];
    CHECK(mpx_apply_staged(e, m) == MPX_OK);
    FAILS(e, mpx_apply_staged(e, aio.cap + 1), MPX_E_INVAL);
    FAILS(e, mpx_apply_buffers(e, 0, &aio), MPX_E_INVAL);
    FAILS(e, mpx_apply_buffers(e, MPX_APPLY_SMALL_MAX + 1, &aio), MPX_E_INVAL);
    size_t nk = 9;
    CHECK(mpx_kv_size(e, &nk) == MPX_OK);
    int64_t kk[4], kv[4];
    CHECK(mpx_kv_export(e, kk, kv, 4, &nk) == MPX_OK);
    CHECK(mpx_kv_import(e, key.data(), val.data(), 7) == MPX_OK);
    CHECK(mpx_kv_clear(e) == MPX_OK);
    uint64_t io[4] = {0, 30, 60, 100}, io_bad[4] = {0, 60, 30, 100};
    std::vector<uint8_t> cb(3);
    CHECK(mpx_conflict_batch(e, op.data(), key.data(), io, 3, cb.data()) == MPX_OK);
    FAILS(e, mpx_conflict_batch(e, op.data(), key.data(), io_bad, 3, cb.data()), MPX_E_INVAL);
    CHECK(mpx_conflict_batch_dev(e, op.data(), key.data(), io, 1, cb.data(), nullptr) == MPX_OK);

    // fused group step: offsets validated on the host
    const uint32_t G = 2, ipg = 4;
    std::vector<mpx_accept_reply> grec(G * ipg * 4);
    for (size_t i = 0; i < grec.size(); ++i)
        grec[i] = mpx_accept_reply{(int32_t)((i / 4) % ipg), 16, 1 + (int32_t)(i % 4), 1, {0, 0, 0}};
    uint64_t groff[3] = {0, 16, 32};
    std::vector<mpx_inst_state> gst(G * ipg, mpx_inst_state{MPX_PREPARED, 0, 0, 0});
    int32_t ci[2] = {-1, -1}, co[2], ei[2] = {-1, -1}, eo[2];
    std::vector<int32_t> pin(G * 5), pout(G * 5);
    std::vector<uint32_t> coff(G * ipg + 1);
    for (size_t i = 0; i < coff.size(); ++i) coff[i] = (uint32_t)(i * 2);
    std::vector<uint8_t> gop(16, MPX_OP_GET), gconf(16);
    std::vector<int64_t> gkey(16, 3), gval(16, 4), gret(16);
    std::vector<uint32_t> kc(G), kc2(G), nd(G);
    std::vector<int64_t> kk2(G * 64), kv2(G * 64), kk3(G * 64), kv3(G * 64);
    mpx_group_batch gb{G, ipg, grec.data(), groff, gst.data(), gst.data(), ci, co, ei, eo,
                       pin.data(), pout.data(), gop.data(), gkey.data(), gval.data(), coff.data(),
                       nullptr, gret.data(), gconf.data(), kc.data(), kk2.data(), kv2.data(),
                       kc2.data(), kk3.data(), kv3.data(), nullptr, nd.data()};
    CHECK(mpx_group_step(e, &gb) == MPX_OK);
    groff[1] = 40;  // not sorted
    FAILS(e, mpx_group_step(e, &gb), MPX_E_INVAL);
    groff[1] = 16;
    coff[3] = 0;  // not sorted
    FAILS(e, mpx_group_step(e, &gb), MPX_E_INVAL);
    coff[3] = 6;
    gb.ipg = 9000;
    FAILS(e, mpx_group_step_dev(e, &gb, nullptr), MPX_E_UNSUPPORTED);
    gb.ipg = ipg;
    gb.n_groups = 100;  // beyond max_groups (16)
    FAILS(e, mpx_group_step_dev(e, &gb, nullptr), MPX_E_INVAL);
    gb.n_groups = G;
    int64_t tot[3];
    CHECK(mpx_step_totals_dev(e, &gb, tot, nullptr) == MPX_OK);
    gb.n_decided = nullptr;
    FAILS(e, mpx_step_totals_dev(e, &gb, tot, nullptr), MPX_E_INVAL);

    // collectives
    int32_t wm[4] = {1, 2, 3, 4};
    FAILS(e, mpx_watermarks_allreduce(e, wm, wm + 2, 2), MPX_E_INVAL);  // no communicator yet
    unsigned char uid[128];
    CHECK(mpx_comm_unique_id(uid) == MPX_OK);
    CHECK(mpx_comm_init(e, 1, 0, uid) == MPX_OK);
    CHECK(mpx_comm_init(e, 2, 5, uid) == MPX_E_INVAL);
    CHECK(mpx_watermarks_allreduce(e, wm, wm + 2, 2) == MPX_OK);
    CHECK(mpx_step_allreduce_dev(e, wm, 2, tot, 3, nullptr) == MPX_OK);
    FAILS(e, mpx_step_allreduce_dev(e, nullptr, 2, tot, 3, nullptr), MPX_E_INVAL);

    // peer streams
    std::vector<uint8_t> buf(300, 13);
    std::vector<mpx_accept_reply> dar(40);
    std::vector<mpx_peer_frame> doth(40);
    mpx_decode_result dres;
    CHECK(mpx_decode_peer_stream(e, buf.data(), buf.size(), dar.data(), 40, doth.data(), 40, &dres) == MPX_OK);
    FAILS(e, mpx_decode_peer_stream(e, nullptr, 10, dar.data(), 40, doth.data(), 40, &dres), MPX_E_INVAL);
    std::vector<mpx_prepare_reply_min> dpr(40);
    std::vector<mpx_var_frame> dvar(40);
    mpx_decode_out out{dar.data(), 40, dpr.data(), 40, dvar.data(), 40, doth.data(), 40};
    mpx_stream_result sres;
    CHECK(mpx_decode_stream(e, buf.data(), buf.size(), &out, &sres) == MPX_OK);
    CHECK(mpx_decode_stream(e, buf.data(), 0, &out, &sres) == MPX_OK);
    mpx_decode_out out_bad = out;
    out_bad.var = nullptr;
    FAILS(e, mpx_decode_stream(e, buf.data(), buf.size(), &out_bad, &sres), MPX_E_INVAL);
    FAILS(e, mpx_decode_stream_dev(e, buf.data() + 1, 10, 0, &out, &sres, nullptr), MPX_E_INVAL);
    FAILS(e, mpx_decode_stream_dev(e, buf.data(), 10, 11, &out, &sres, nullptr), MPX_E_INVAL);
    CHECK(mpx_decode_stream_reserve(e, buf.size()) == MPX_OK);

    // fan-out, logs, replay
    std::vector<mpx_reply_rec> rr(10, mpx_reply_rec{1, 2, 3, 1});
    std::vector<uint8_t> rout(250);
    std::vector<uint64_t> roff(4);
    CHECK(mpx_encode_replies(e, rr.data(), 10, 3, 1, 0, rout.data(), roff.data()) == MPX_OK);
    CHECK(mpx_encode_replies(e, rr.data(), 10, 0, 1, 0, rout.data(), roff.data()) == MPX_E_INVAL);
    std::vector<mpx_log_rec> lr(3, mpx_log_rec{16, MPX_COMMITTED, 0, 0});
    uint64_t loff[4] = {0, 2, 4, 6}, loff_bad[4] = {0, 4, 2, 6};
    std::vector<uint8_t> lout(mpx_encode_log_bound(3, 6));
    std::vector<uint64_t> lro(4);
    CHECK(mpx_encode_log(e, MPX_LOG_CATCHUP, lr.data(), 3, loff, op.data(), key.data(), val.data(), 6, lout.data(), lout.size(), lro.data()) == MPX_OK);
    FAILS(e, mpx_encode_log(e, MPX_LOG_DURABLE, lr.data(), 3, loff_bad, op.data(), key.data(), val.data(), 6, lout.data(), lout.size(), lro.data()), MPX_E_INVAL);
    FAILS(e, mpx_encode_log(e, 5, lr.data(), 3, loff, op.data(), key.data(), val.data(), 6, lout.data(), lout.size(), lro.data()), MPX_E_INVAL);
    std::vector<uint8_t> log(29 * 4);
    std::vector<mpx_log_rec> rrec(4);
    std::vector<int32_t> last(8, -1);
    int32_t sc[2] = {0, -1};
    CHECK(mpx_replay_durable(e, log.data(), log.size(), 8, 0, rrec.data(), op.data(), key.data(), val.data(), last.data(), sc) == MPX_OK);
    FAILS(e, mpx_replay_durable(e, log.data(), log.size() - 1, 8, 0, rrec.data(), op.data(), key.data(), val.data(), last.data(), sc), MPX_E_INVAL);
    FAILS(e, mpx_replay_durable(e, log.data(), log.size(), 0, 0, rrec.data(), op.data(), key.data(), val.data(), last.data(), sc), MPX_E_NIL_INSTANCE);
    FAILS(e, mpx_replay_durable(e, log.data(), log.size(), 8, -1, rrec.data(), op.data(), key.data(), val.data(), last.data(), sc), MPX_E_INVAL);
    FAILS(e, mpx_replay_durable(e, log.data(), log.size(), 8, INT32_MAX - 2, rrec.data(), op.data(), key.data(), val.data(), last.data(), sc), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_replay_durable_dev(e, log.data(), log.size(), 0, 0, rrec.data(), op.data(), key.data(), val.data(), last.data(), sc, nullptr), MPX_E_NIL_INSTANCE);

    // the acceptor side, on a second handle (apply_path SORTED: its small applies stage through
    // the arena) whose AcceptReply scratch nothing has grown yet
    mpx_config cfg2{5, MPX_MODE_MIN, 1 << 10, 64, 0, 16, 0, MPX_APPLY_SORTED, 0, 0, 0};
    mpx_engine* e2 = nullptr;
    CHECK(mpx_open(0, &cfg2, &e2) == MPX_OK && e2);
    {
        const size_t an = 6, aG = 2;
        const uint32_t aipg = 4;
        std::vector<mpx_accept_msg> am(an);
        std::vector<mpx_acceptor_state> as(aG * aipg);
        std::vector<mpx_acceptor_group> ag(aG);
        std::vector<mpx_accept_reply> arep(an);
        std::vector<int32_t> ato(an);
        std::vector<uint8_t> aeff(an), abytes(an * MPX_ACCEPT_REPLY_FRAME_MIN);
        std::vector<uint64_t> aoff(MPX_MAX_REPLICAS + 2);
        CHECK(mpx_accept_handle(e2, am.data(), an, as.data(), aG * aipg, 0, ag.data(), aG, aipg, arep.data(), ato.data(), aeff.data()) == MPX_OK);
        CHECK(mpx_accept_handle_dev(e2, am.data(), an, as.data(), as.data(), aG * aipg, 0, ag.data(), aG, aipg, arep.data(), ato.data(), aeff.data(), nullptr) == MPX_OK);
        CHECK(mpx_accept_handle(e2, nullptr, 0, as.data(), aG * aipg, 0, ag.data(), aG, aipg, nullptr, nullptr, nullptr) == MPX_OK);
        FAILS(e2, mpx_accept_handle(e2, am.data(), an, as.data(), aG * aipg + 1, 0, ag.data(), aG, aipg, arep.data(), ato.data(), aeff.data()), MPX_E_INVAL);
        FAILS(e2, mpx_accept_handle_dev(e2, am.data(), an, as.data(), as.data(), aG * aipg + 1, 0, ag.data(), aG, aipg, arep.data(), ato.data(), aeff.data(), nullptr), MPX_E_INVAL);
        FAILS(e2, mpx_accept_handle(e2, am.data(), an, as.data(), aG * aipg, 0, ag.data(), aG, 0, arep.data(), ato.data(), aeff.data()), MPX_E_INVAL);
        FAILS(e2, mpx_accept_handle(e2, nullptr, an, as.data(), aG * aipg, 0, ag.data(), aG, aipg, arep.data(), ato.data(), aeff.data()), MPX_E_INVAL);
        FAILS(e2, mpx_accept_handle(e2, am.data(), an, as.data(), aG * aipg, 0, nullptr, aG, aipg, arep.data(), ato.data(), aeff.data()), MPX_E_INVAL);
        // too many records: refused by both forms before anything is allocated or read
        FAILS(e2, mpx_accept_handle(e2, am.data(), 0xFFFFFFFFull, as.data(), aG * aipg, 0, ag.data(), aG, aipg, arep.data(), ato.data(), aeff.data()), MPX_E_UNSUPPORTED);
        FAILS(e2, mpx_accept_handle_dev(e2, am.data(), 0xFFFFFFFFull, as.data(), as.data(), aG * aipg, 0, ag.data(), aG, aipg, arep.data(), ato.data(), aeff.data(), nullptr), MPX_E_UNSUPPORTED);
        // the _dev encoder never allocates: it needs its reserve call first (an empty call does not)
        FAILS(e2, mpx_encode_accept_replies_dev(e2, arep.data(), ato.data(), an, 5, abytes.data(), aoff.data(), nullptr), MPX_E_INVAL);
        CHECK(strstr(mpx_last_error(e2), "mpx_encode_accept_replies_dev") && strstr(mpx_last_error(e2), "mpx_encode_accept_replies_reserve"));
        CHECK(mpx_encode_accept_replies_dev(e2, nullptr, nullptr, 0, 5, nullptr, aoff.data(), nullptr) == MPX_OK);
        CHECK(mpx_encode_accept_replies_reserve(e2, an) == MPX_OK);
        CHECK(mpx_encode_accept_replies_dev(e2, arep.data(), ato.data(), an, 5, abytes.data(), aoff.data(), nullptr) == MPX_OK);
        CHECK(aoff[5] == an * MPX_ACCEPT_REPLY_FRAME_MIN);
        CHECK(mpx_encode_accept_replies(e2, arep.data(), ato.data(), an, MPX_MAX_REPLICAS, abytes.data(), aoff.data()) == MPX_OK);
        CHECK(mpx_encode_accept_replies(e2, nullptr, nullptr, 0, 5, nullptr, aoff.data()) == MPX_OK && aoff[5] == 0);
        FAILS(e2, mpx_encode_accept_replies(e2, arep.data(), ato.data(), an, 0, abytes.data(), aoff.data()), MPX_E_INVAL);
        FAILS(e2, mpx_encode_accept_replies(e2, arep.data(), ato.data(), an, MPX_MAX_REPLICAS + 1, abytes.data(), aoff.data()), MPX_E_INVAL);
        FAILS(e2, mpx_encode_accept_replies_dev(e2, arep.data(), ato.data(), an, 0, abytes.data(), aoff.data(), nullptr), MPX_E_INVAL);
        FAILS(e2, mpx_encode_accept_replies_dev(e2, arep.data(), ato.data(), an, MPX_MAX_REPLICAS + 1, abytes.data(), aoff.data(), nullptr), MPX_E_INVAL);
        FAILS(e2, mpx_encode_accept_replies(e2, arep.data(), nullptr, an, 5, abytes.data(), aoff.data()), MPX_E_INVAL);
        FAILS(e2, mpx_encode_accept_replies_reserve(e2, 1ull << 32), MPX_E_UNSUPPORTED);
        // the other _dev forms name their reserve call the same way
        FAILS(e2, mpx_encode_replies_dev(e2, rr.data(), 10, 3, 1, 0, rout.data(), roff.data(), nullptr), MPX_E_INVAL);
        CHECK(strstr(mpx_last_error(e2), "mpx_encode_replies_dev") && strstr(mpx_last_error(e2), "mpx_encode_replies_reserve"));
        FAILS(e2, mpx_apply_dev(e2, op.data(), key.data(), val.data(), m, ret.data(), nullptr, nullptr), MPX_E_INVAL);
        CHECK(strstr(mpx_last_error(e2), "mpx_apply_dev") && strstr(mpx_last_error(e2), "mpx_apply_reserve"));
    }

    // staging: every family on the two handles, sizes growing and then shrinking, so the arena
    // regrows between calls of different families and later calls use a part of it
    for (size_t s : {8, 600, 4096, 33, 1500, 5}) all_families(e, e2, s);
    CHECK(mpx_close(e2) == MPX_OK);

    // device utilities
    void* d = nullptr;
    CHECK(mpx_dev_alloc(e, 64, &d) == MPX_OK && d);
    CHECK(mpx_memset_async(e, d, 0xFF, 64, nullptr) == MPX_OK);
    CHECK(mpx_memcpy_async(e, d, buf.data(), 64, MPX_COPY_H2D, nullptr) == MPX_OK);
    FAILS(e, mpx_memcpy_async(e, d, buf.data(), 64, 9, nullptr), MPX_E_INVAL);
    void *s = nullptr, *ev0 = nullptr, *ev1 = nullptr;
    CHECK(mpx_stream_create(e, &s) == MPX_OK);
    CHECK(mpx_event_create(e, 1, &ev0) == MPX_OK && mpx_event_create(e, 0, &ev1) == MPX_OK);
    CHECK(mpx_event_record(e, ev0, s) == MPX_OK && mpx_stream_wait_event(e, nullptr, ev0) == MPX_OK);
    float ms = -1;
    CHECK(mpx_event_elapsed_ms(e, ev0, ev1, &ms) == MPX_OK);
    FAILS(e, mpx_stream_destroy(e, mpx_stream(e)), MPX_E_INVAL);
    CHECK(mpx_stream_destroy(e, s) == MPX_OK);
    CHECK(mpx_event_destroy(e, ev0) == MPX_OK && mpx_event_destroy(e, ev1) == MPX_OK);
    CHECK(mpx_dev_free(e, d) == MPX_OK && mpx_dev_free(e, nullptr) == MPX_OK);
    char info[8];
    const int full = mpx_runtime_info(info, sizeof(info));
    CHECK(full > 8 && strlen(info) == 7);
    CHECK(mpx_runtime_info(nullptr, 0) == full);

    CHECK(mpx_synchronize(e) == MPX_OK);
    CHECK(mpx_close(e) == MPX_OK);
    CHECK(mpx_close(nullptr) == MPX_E_INVAL);
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("abi_driver: all checks passed\n");
    return failures ? 1 : 0;
}
