// tests/san/execute_driver.cpp — TEST INFRASTRUCTURE ONLY: drives mpx_execute_gather and its
// _reserve / _dev forms of the CPU build of engine.cpp + execute.cpp over the stub runtime
// (hip_stub.cpp) and the walking, gathering stand-in of execute_stub.cpp under ASan + UBSan. Every
// argument-validation path of both forms must answer its code before anything is staged or
// launched; valid calls on guarded buffers must bring back exactly the expected commands, mask,
// cursors, offsets and counts through the staging arena, leave the inputs and the guard bytes
// alone and write nothing past what the call produced. Exit status 0 = all checks passed.
#include <algorithm>

#include "san_check.hpp"

static mpx_engine* open_engine() {
    mpx_engine* e = nullptr;
    mpx_config cfg{5, MPX_MODE_MIN, 1 << 10, 0, 0, 0};
    CHECK(mpx_open(0, &cfg, &e) == MPX_OK && e);
    return e;
}

static bool tail_untouched(const Out& o, size_t from) {
    for (size_t i = from; i < o.v.size(); ++i)
        if (o.v[i] != kGuardByte) return false;
    return true;
}

// G groups of ipg slots from instance 100; slot idx has n_cmds[idx % n_cmds.size()] commands laid
// out back to back from command 3 (so first_cmd is never 0), nil where nil[idx]; group g is
// committed up to first_g - 1 + cu[g] and has executed up to first_g - 1 + ex[g]; source command j
// is {j % 5, 1000 + j, -j}; sends name every third slot, one instance below the window and one past it
static void valid_case(mpx_engine* e, size_t G, uint32_t ipg, std::vector<uint32_t> n_cmds,
                       std::vector<uint8_t> nil, std::vector<int> cu, std::vector<int> ex,
                       size_t cap_short, size_t pad_extra, bool optional, bool dev,
                       uint32_t call_flags) {
    const size_t n = G * ipg;
    const int32_t base = 100;
    std::vector<mpx_inst_cmds> inst(n ? n : 1);
    size_t n_src = 3;
    for (size_t i = 0; i < n; ++i) {
        const uint32_t k = n_cmds[i % n_cmds.size()];
        inst[i] = mpx_inst_cmds{n_src, k, nil[i % nil.size()] ? 0u : MPX_IC_HAS_CMDS};
        n_src += k;
    }
    std::vector<uint8_t> sop(n_src);
    std::vector<int64_t> skey(n_src), sval(n_src);
    for (size_t j = 0; j < n_src; ++j) sop[j] = j % 5, skey[j] = 1000 + (int64_t)j, sval[j] = -(int64_t)j;
    std::vector<int32_t> vcu(G ? G : 1), vex(G ? G : 1);
    for (size_t g = 0; g < G; ++g) {
        vcu[g] = base + (int32_t)(g * ipg) - 1 + cu[g % cu.size()];
        vex[g] = base + (int32_t)(g * ipg) - 1 + ex[g % ex.size()];
    }
    std::vector<mpx_accept_send> sends;
    for (size_t i = 0; i < n; i += 3) sends.push_back(mpx_accept_send{base + (int32_t)i, 1, -1, MPX_PH_ACCEPT, 0, 0, 0});
    sends.push_back(mpx_accept_send{base - 1, 1, -1, MPX_PH_ACCEPT, 0, 0, 0});
    sends.push_back(mpx_accept_send{base + (int32_t)n, 1, -1, MPX_PH_ACCEPT, 0, 0, 0});
    const size_t S = sends.size();
    // what the call must produce: executeCommands, group by group
    std::vector<uint64_t> want_src, lens(n + 1, 0), want_goff;
    std::vector<uint8_t> want_mask(n, 0);
    std::vector<int32_t> want_ex(G);
    uint64_t ran = 0, moved = 0;
    for (size_t g = 0; g < G; ++g) {
        want_goff.push_back(want_src.size());
        int64_t i = (int64_t)vex[g] + 1;
        for (; i <= vcu[g] && (inst[i - base].flags & MPX_IC_HAS_CMDS); ++i) {
            want_mask[i - base] = 1, lens[i - base + 1] = inst[i - base].n_cmds, ++ran;
            for (uint32_t j = 0; j < inst[i - base].n_cmds; ++j) want_src.push_back(inst[i - base].first_cmd + j);
        }
        want_ex[g] = (int32_t)(i - 1);
        moved += want_ex[g] != vex[g];
    }
    want_goff.push_back(want_src.size());
    for (size_t i = 0; i < n; ++i) lens[i + 1] += lens[i];
    const size_t total = want_src.size();
    const bool pad = pad_extra != (size_t)-1;
    const size_t cap = pad ? total + pad_extra : total - std::min(total, cap_short);
    In d_inst = holding(inst.data(), n, 3), d_cu = holding(vcu.data(), G, 4), d_ex = holding(vex.data(), G, 5),
       d_sop = holding(sop.data(), n_src, 6), d_skey = holding(skey.data(), n_src, 7),
       d_sval = holding(sval.data(), n_src, 8), d_sends = holding(sends.data(), S, 9);
    Out op(cap), key(cap * 8), val(cap * 8), mask(n), exo(G * 4), ifirst(n * 8), rf(S * 8), goff((G + 1) * 8);
    mpx_execute_result res[2];
    memset(res, 0x5C, sizeof(res));
    mpx_execute_batch b{};
    b.inst = n ? d_inst.as<mpx_inst_cmds>() : nullptr, b.n_inst = n, b.inst_base = base, b.ipg = ipg;
    b.n_groups = G, b.committed_upto = G ? d_cu.as<int32_t>() : nullptr;
    b.executed_in = G ? d_ex.as<int32_t>() : nullptr, b.executed_out = G ? exo.as<int32_t>() : nullptr;
    b.src_op = d_sop.as<uint8_t>(), b.src_key = d_skey.as<int64_t>(), b.src_val = d_sval.as<int64_t>();
    b.n_src = n_src, b.flags = call_flags | (pad ? MPX_XG_PAD : 0u);
    mpx_execute_out o{};
    o.op = cap ? op.as<uint8_t>() : nullptr, o.key = cap ? key.as<int64_t>() : nullptr;
    o.val = cap ? val.as<int64_t>() : nullptr, o.cap = cap, o.mask = n ? mask.as<uint8_t>() : nullptr;
    if (optional) {
        b.sends = d_sends.as<mpx_accept_send>(), b.n_sends = S;
        o.inst_first = ifirst.as<uint64_t>(), o.ret_first = rf.as<uint64_t>(), o.grp_cmd_off = goff.as<uint64_t>();
    }
    if (dev) {
        CHECK(mpx_execute_gather_reserve(e, n, G) == MPX_OK);
        CHECK(mpx_execute_gather_dev(e, &b, &o, res, nullptr) == MPX_OK);
        CHECK(mpx_synchronize(e) == MPX_OK);
    } else {
        CHECK(mpx_execute_gather(e, &b, &o, res) == MPX_OK);
    }
    CHECK(d_inst.intact() && d_cu.intact() && d_ex.intact() && d_sop.intact() && d_skey.intact() &&
          d_sval.intact() && d_sends.intact());
    CHECK(res[0].n_cmds == total && res[0].n_inst == ran && res[0].n_groups == moved && res[0].reserved == 0);
    const size_t real = std::min(total, cap), wrote = pad ? cap : real;
    for (size_t i = 0; i < wrote; ++i) {
        const bool r = i < real;
        CHECK(op.as<uint8_t>()[i] == (r ? sop[want_src[i]] : 0));
        CHECK(key.as<int64_t>()[i] == (r ? skey[want_src[i]] : (int64_t)i));
        CHECK(val.as<int64_t>()[i] == (r ? sval[want_src[i]] : 0));
    }
    CHECK(tail_untouched(op, wrote) && tail_untouched(key, wrote * 8) && tail_untouched(val, wrote * 8));
    for (size_t i = 0; i < n; ++i) CHECK(mask.as<uint8_t>()[i] == want_mask[i]);
    for (size_t g = 0; g < G; ++g) CHECK(exo.as<int32_t>()[g] == want_ex[g]);
    CHECK(tail_untouched(mask, n) && tail_untouched(exo, G * 4));
    if (optional) {
        for (size_t i = 0; i < n; ++i) CHECK(ifirst.as<uint64_t>()[i] == lens[i]);
        for (size_t g = 0; g <= G; ++g) CHECK(goff.as<uint64_t>()[g] == want_goff[g]);
        for (size_t s = 0; s < S; ++s) {
            const int64_t rel = (int64_t)sends[s].instance - base;
            CHECK(rf.as<uint64_t>()[s] == (rel >= 0 && (size_t)rel < n ? lens[rel] : 0));
        }
        CHECK(tail_untouched(ifirst, n * 8) && tail_untouched(goff, (G + 1) * 8) && tail_untouched(rf, S * 8));
    } else {
        CHECK(ifirst.untouched() && rf.untouched() && goff.untouched());
    }
    const uint8_t* after = (const uint8_t*)&res[1];
    for (size_t i = 0; i < sizeof(res[1]); ++i) CHECK(after[i] == 0x5C);
}

static void validation(mpx_engine* e) {
    // two groups of two slots from instance 10; commands 0..5
    alignas(16) mpx_inst_cmds inst[4] = {{0, 2, 1}, {2, 1, 1}, {3, 2, 1}, {5, 1, 1}};
    alignas(16) int32_t cu[2] = {11, 13}, ex[2] = {9, 11}, exo[2] = {-7, -7};
    alignas(16) uint8_t sop[6] = {1, 2, 1, 2, 1, 2};
    alignas(16) int64_t skey[6] = {1, 2, 3, 4, 5, 6}, sval[6] = {7, 8, 9, 10, 11, 12};
    alignas(16) mpx_accept_send sends[1] = {{10, 1, -1, MPX_PH_ACCEPT, 0, 0, 0}};
    Out op(8), key(64), val(64), mask(4), ifirst(32), rf(8), goff(24);
    mpx_execute_result res;
    memset(&res, 0x5C, sizeof(res));
    CHECK(mpx_execute_gather_reserve(e, 4, 2) == MPX_OK);
    mpx_execute_batch ok{};
    ok.inst = inst, ok.n_inst = 4, ok.inst_base = 10, ok.ipg = 2, ok.n_groups = 2;
    ok.committed_upto = cu, ok.executed_in = ex, ok.executed_out = exo;
    ok.src_op = sop, ok.src_key = skey, ok.src_val = sval, ok.n_src = 6;
    ok.sends = sends, ok.n_sends = 1;
    mpx_execute_out oo{};
    oo.op = op.as<uint8_t>(), oo.key = key.as<int64_t>(), oo.val = val.as<int64_t>(), oo.cap = 8;
    oo.mask = mask.as<uint8_t>(), oo.inst_first = ifirst.as<uint64_t>(), oo.ret_first = rf.as<uint64_t>();
    oo.grp_cmd_off = goff.as<uint64_t>();
    auto both = [&](const mpx_execute_batch* b, const mpx_execute_out* o, mpx_execute_result* rs, int code) {
        FAILS(e, mpx_execute_gather(e, b, o, rs), code);
        FAILS(e, mpx_execute_gather_dev(e, b, o, rs, nullptr), code);
    };
    // null arguments
    both(nullptr, &oo, &res, MPX_E_INVAL);
    both(&ok, nullptr, &res, MPX_E_INVAL);
    both(&ok, &oo, nullptr, MPX_E_INVAL);
    mpx_execute_batch x = ok;
    mpx_execute_out y = oo;
    x.inst = nullptr;
    both(&x, &oo, &res, MPX_E_INVAL);
    x = ok, x.committed_upto = nullptr;
    both(&x, &oo, &res, MPX_E_INVAL);
    x = ok, x.executed_in = nullptr;
    both(&x, &oo, &res, MPX_E_INVAL);
    x = ok, x.executed_out = nullptr;
    both(&x, &oo, &res, MPX_E_INVAL);
    x = ok, x.src_op = nullptr;
    both(&x, &oo, &res, MPX_E_INVAL);
    x = ok, x.src_key = nullptr;
    both(&x, &oo, &res, MPX_E_INVAL);
    x = ok, x.src_val = nullptr;
    both(&x, &oo, &res, MPX_E_INVAL);
    y = oo, y.mask = nullptr;
    both(&ok, &y, &res, MPX_E_INVAL);
    y = oo, y.op = nullptr;
    both(&ok, &y, &res, MPX_E_INVAL);
    y = oo, y.key = nullptr;
    both(&ok, &y, &res, MPX_E_INVAL);
    y = oo, y.val = nullptr;
    both(&ok, &y, &res, MPX_E_INVAL);
    // the window's shape, unknown flags, reserved, ret_first without sends
    x = ok, x.n_inst = 3;
    both(&x, &oo, &res, MPX_E_INVAL);
    x = ok, x.ipg = 3;
    both(&x, &oo, &res, MPX_E_INVAL);
    x = ok, x.ipg = 0, x.n_inst = 0;
    both(&x, &oo, &res, MPX_E_INVAL);
    x = ok, x.flags = 4;
    both(&x, &oo, &res, MPX_E_INVAL);
    x = ok, x.reserved = 1;
    both(&x, &oo, &res, MPX_E_INVAL);
    x = ok, x.sends = nullptr, x.n_sends = 0;
    both(&x, &oo, &res, MPX_E_INVAL);
    x = ok, x.sends = nullptr;
    both(&x, &oo, &res, MPX_E_INVAL);
    // the limits
    x = ok, x.n_inst = (size_t)0xFFFFFFFFull, x.n_groups = 1, x.ipg = 0xFFFFFFFFu;
    both(&x, &oo, &res, MPX_E_UNSUPPORTED);
    FAILS(e, mpx_execute_gather_reserve(e, (size_t)0xFFFFFFFFull, 1), MPX_E_UNSUPPORTED);
    FAILS(e, mpx_execute_gather_reserve(e, 1, (size_t)0xFFFFFFFFull), MPX_E_UNSUPPORTED);
    inst[0].n_cmds = inst[1].n_cmds = 0x80000000u;  // 2^32 commands in all (refused before any is read)
    x = ok, x.n_src = (size_t)1 << 40;
    FAILS(e, mpx_execute_gather(e, &x, &oo, &res), MPX_E_UNSUPPORTED);
    inst[0].n_cmds = 2, inst[1].n_cmds = 1;
    // the groups and the instances, host form
    for (const int32_t bad : {8, 12}) {
        cu[0] = bad;
        FAILS(e, mpx_execute_gather(e, &ok, &oo, &res), MPX_E_INVAL);
        cu[0] = 11, ex[0] = bad;
        FAILS(e, mpx_execute_gather(e, &ok, &oo, &res), MPX_E_INVAL);
        ex[0] = 9;
    }
    cu[1] = 10;
    FAILS(e, mpx_execute_gather(e, &ok, &oo, &res), MPX_E_INVAL);
    cu[1] = 13;
    inst[1].n_cmds = 5;  // [2, 7) leaves [0, 6)
    FAILS(e, mpx_execute_gather(e, &ok, &oo, &res), MPX_E_INVAL);
    inst[1] = mpx_inst_cmds{7, 0, 1};
    FAILS(e, mpx_execute_gather(e, &ok, &oo, &res), MPX_E_INVAL);
    cu[0] = 10;  // ... not looked at when the walk does not reach it
    CHECK(mpx_execute_gather(e, &ok, &oo, &res) == MPX_OK && res.n_cmds == 5 && res.n_inst == 3 && res.n_groups == 2);
    CHECK(exo[0] == 10 && exo[1] == 13 && rf.as<uint64_t>()[0] == 0 && goff.as<uint64_t>()[1] == 2);
    cu[0] = 11;
    inst[1] = mpx_inst_cmds{2, 1, 1};
    for (Out* z : {&op, &key, &val, &mask, &ifirst, &rf, &goff}) memset(z->v.data(), kGuardByte, z->v.size());
    memset(&res, 0x5C, sizeof(res));
    exo[0] = exo[1] = -7;
    // the device form's alignment rules
    auto dev = [&](const mpx_execute_batch& b, const mpx_execute_out& o, mpx_execute_result* rs) {
        return mpx_execute_gather_dev(e, &b, &o, rs, nullptr);
    };
#define SHIFTED(T, p, by) ((T*)((char*)(p) + (by)))
    x = ok, x.inst = SHIFTED(const mpx_inst_cmds, inst, 8);
    FAILS(e, dev(x, oo, &res), MPX_E_INVAL);
    x = ok, x.sends = SHIFTED(const mpx_accept_send, sends, 8);
    FAILS(e, dev(x, oo, &res), MPX_E_INVAL);
    x = ok, x.src_key = SHIFTED(const int64_t, skey, 4);
    FAILS(e, dev(x, oo, &res), MPX_E_INVAL);
    x = ok, x.src_val = SHIFTED(const int64_t, sval, 4);
    FAILS(e, dev(x, oo, &res), MPX_E_INVAL);
    x = ok, x.committed_upto = SHIFTED(const int32_t, cu, 2);
    FAILS(e, dev(x, oo, &res), MPX_E_INVAL);
    x = ok, x.executed_in = SHIFTED(const int32_t, ex, 2);
    FAILS(e, dev(x, oo, &res), MPX_E_INVAL);
    x = ok, x.executed_out = SHIFTED(int32_t, exo, 2);
    FAILS(e, dev(x, oo, &res), MPX_E_INVAL);
    y = oo, y.key = SHIFTED(int64_t, oo.key, 4);
    FAILS(e, dev(ok, y, &res), MPX_E_INVAL);
    y = oo, y.val = SHIFTED(int64_t, oo.val, 4);
    FAILS(e, dev(ok, y, &res), MPX_E_INVAL);
    y = oo, y.inst_first = SHIFTED(uint64_t, oo.inst_first, 4);
    FAILS(e, dev(ok, y, &res), MPX_E_INVAL);
    y = oo, y.ret_first = SHIFTED(uint64_t, oo.ret_first, 4);
    FAILS(e, dev(ok, y, &res), MPX_E_INVAL);
    y = oo, y.grp_cmd_off = SHIFTED(uint64_t, oo.grp_cmd_off, 4);
    FAILS(e, dev(ok, y, &res), MPX_E_INVAL);
    FAILS(e, dev(ok, oo, SHIFTED(mpx_execute_result, &res, 4)), MPX_E_INVAL);
    // nothing was touched
    CHECK(op.untouched() && key.untouched() && val.untouched() && mask.untouched() && ifirst.untouched() &&
          rf.untouched() && goff.untouched() && exo[0] == -7 && exo[1] == -7);
    const uint8_t* rb = (const uint8_t*)&res;
    for (size_t i = 0; i < sizeof(res); ++i) CHECK(rb[i] == 0x5C);
    // the device form reports a faulty group or instance through the error word: the group does
    // nothing, the instance executes with no commands, the others are exact
    cu[0] = 12;
    CHECK(dev(ok, oo, &res) == MPX_OK);
    FAILS(e, mpx_synchronize(e), MPX_E_INVAL);
    CHECK(res.n_cmds == 3 && res.n_inst == 2 && res.n_groups == 1 && exo[0] == 9 && exo[1] == 13);
    cu[0] = 11, inst[1].n_cmds = 5;
    CHECK(dev(ok, oo, &res) == MPX_OK);
    FAILS(e, mpx_synchronize(e), MPX_E_INVAL);
    CHECK(res.n_cmds == 5 && res.n_inst == 4 && res.n_groups == 2 && exo[0] == 11 && mask.as<uint8_t>()[1] == 1 &&
          ifirst.as<uint64_t>()[2] == 2);
    inst[1].n_cmds = 1;
    // ... and the same call is legal once repaired; op, src_op and mask may sit at any address
    x = ok, x.src_op = sop + 1, x.n_src = 5;
    y = oo, y.op = oo.op + 1, y.mask = oo.mask + 1, y.cap = 7;
    inst[3].first_cmd = 4;
    CHECK(dev(x, y, &res) == MPX_OK && mpx_synchronize(e) == MPX_OK && res.n_cmds == 6 && res.n_inst == 4);
    inst[3].first_cmd = 5;
    // no slot, no capacity: legal, with null arrays
    mpx_execute_batch none{};
    mpx_execute_out nout{};
    CHECK(mpx_execute_gather(e, &none, &nout, &res) == MPX_OK);
    CHECK(res.n_cmds == 0 && res.n_inst == 0 && res.n_groups == 0);
    // a capacity of 0 with null command arrays still walks and counts
    y = oo, y.op = nullptr, y.key = nullptr, y.val = nullptr, y.cap = 0;
    CHECK(mpx_execute_gather(e, &ok, &y, &res) == MPX_OK && res.n_cmds == 6 && exo[0] == 11 && exo[1] == 13);
    // executed_in and executed_out may be one array
    x = ok, x.executed_out = ex;
    CHECK(mpx_execute_gather(e, &x, &oo, &res) == MPX_OK && ex[0] == 11 && ex[1] == 13);
    CHECK(mpx_execute_gather(e, &x, &oo, &res) == MPX_OK && res.n_cmds == 0 && res.n_groups == 0);
}

int main() {
    mpx_engine* e = open_engine();
    if (!e) return 1;
    validation(e);
    const size_t no_pad = (size_t)-1;
    for (const uint32_t call_flags : {0u, MPX_XG_GENERAL})
        for (const size_t cap_short : {(size_t)0, (size_t)1, (size_t)1000000}) {
            valid_case(e, 1, 3, {2, 1, 2}, {0}, {3}, {0}, cap_short, no_pad, true, false, call_flags);
            valid_case(e, 4, 5, {3, 0, 5, 1}, {0, 0, 0, 1, 0, 0, 0}, {5, 0, 3, 2}, {0, 0, 1, 4}, cap_short, no_pad,
                       true, false, call_flags);
            // ... of a size at which the arrays have slots of more than one 256-byte unit
            valid_case(e, 7, 40, {300, 17, 0, 2, 1}, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, {40, 13, 0, 7}, {0, 2, 0, 9},
                       cap_short, no_pad, cap_short != 1, false, call_flags);
            valid_case(e, 0, 0, {1}, {0}, {0}, {0}, cap_short, no_pad, true, false, call_flags);
            valid_case(e, 3, 2, {4}, {1}, {2}, {0}, cap_short, no_pad, true, false, call_flags);
        }
    for (const size_t pad_extra : {(size_t)0, (size_t)1, (size_t)40}) {
        valid_case(e, 7, 40, {300, 17, 0, 2, 1}, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, {40, 13, 0, 7}, {0, 2, 0, 9}, 0,
                   pad_extra, true, false, 0);
        valid_case(e, 0, 0, {1}, {0}, {0}, {0}, 0, pad_extra, false, false, MPX_XG_GENERAL);
    }
    // the device form never allocates: on a fresh handle it needs its reserve call first, and a
    // reserve that is too small in either size is refused as well
    mpx_engine* f = open_engine();
    if (!f) return 1;
    {
        alignas(16) mpx_inst_cmds inst[2] = {{0, 1, 1}, {1, 1, 1}};
        alignas(16) int32_t cu[2] = {0, 1}, ex[2] = {-1, 0}, exo[2];
        alignas(16) uint8_t sop[2] = {1, 2}, op[2], mask[2];
        alignas(16) int64_t skey[2] = {1, 2}, sval[2] = {3, 4}, key[2], val[2];
        alignas(16) mpx_execute_result res;
        mpx_execute_batch b{};
        b.inst = inst, b.n_inst = 2, b.ipg = 1, b.n_groups = 2, b.committed_upto = cu, b.executed_in = ex;
        b.executed_out = exo, b.src_op = sop, b.src_key = skey, b.src_val = sval, b.n_src = 2;
        mpx_execute_out o{};
        o.op = op, o.key = key, o.val = val, o.cap = 2, o.mask = mask;
        FAILS(f, mpx_execute_gather_dev(f, &b, &o, &res, nullptr), MPX_E_INVAL);
        CHECK(strstr(mpx_last_error(f), "mpx_execute_gather_dev") &&
              strstr(mpx_last_error(f), "mpx_execute_gather_reserve"));
        CHECK(mpx_execute_gather_reserve(f, 2, 1) == MPX_OK);
        FAILS(f, mpx_execute_gather_dev(f, &b, &o, &res, nullptr), MPX_E_INVAL);  // two groups
        CHECK(mpx_execute_gather_reserve(f, 1, 2) == MPX_OK);                     // (grows only)
        CHECK(mpx_execute_gather_dev(f, &b, &o, &res, nullptr) == MPX_OK);
        CHECK(mpx_synchronize(f) == MPX_OK && res.n_cmds == 2 && exo[0] == 0 && exo[1] == 1 && key[1] == 2);
        b.flags = MPX_XG_GENERAL;
        CHECK(mpx_execute_gather_dev(f, &b, &o, &res, nullptr) == MPX_OK);
        CHECK(mpx_synchronize(f) == MPX_OK && res.n_cmds == 2 && res.n_groups == 2);
    }
    for (const uint32_t call_flags : {0u, MPX_XG_GENERAL}) {
        // a larger group capacity moves the stop words' end over what was other scratch
        valid_case(f, 7, 40, {300, 17, 0, 2, 1}, {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}, {40, 13, 0, 7}, {0, 2, 0, 9}, 0,
                   no_pad, true, true, call_flags);
        valid_case(f, 300, 1, {2, 1}, {0, 0, 1}, {1}, {0}, 100, no_pad, true, true, call_flags);
        valid_case(f, 4, 5, {3, 0, 5, 1}, {0, 0, 0, 1, 0, 0, 0}, {5, 0, 3, 2}, {0, 0, 1, 4}, 0, 33, false, true,
                   call_flags);
    }
    CHECK(mpx_close(f) == MPX_OK);
    CHECK(mpx_close(e) == MPX_OK);
    mpx_execute_result res;
    mpx_execute_batch none{};
    mpx_execute_out nout{};
    CHECK(mpx_execute_gather(nullptr, &none, &nout, &res) == MPX_E_INVAL);
    CHECK(mpx_execute_gather_reserve(nullptr, 1, 1) == MPX_E_INVAL);
    CHECK(mpx_execute_gather_dev(nullptr, &none, &nout, &res, nullptr) == MPX_E_INVAL);
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("execute_driver: all checks passed\n");
    return failures ? 1 : 0;
}
