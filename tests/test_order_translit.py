"""Batch assembly on the CPU: the restatement of the shim's stable sort (tests/order_translit.py)
against answers worked out by hand, its error codes, the reach of the fuzz generator the GPU
tests run, and the boundary: struct sizes against the header, a null engine."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import order_translit as O
from minpaxos_amd import _lib
from minpaxos_amd import records as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(O.KAT))
@pytest.mark.parametrize("dtype", [R.ACCEPT_REPLY, R.ACCEPT_MSG], ids=["reply", "msg"])
def test_known_answers(name, dtype):
    case, (perm, n_runs, lo, hi, ordered) = O.kat_case(name, dtype)
    out, got_perm, res = O.order_records(**case)
    cat = np.concatenate(case["sources"])
    assert got_perm.tolist() == perm
    assert out.tobytes() == cat[np.array(perm, np.int64)].tobytes()
    assert (int(res["n"]), int(res["n_runs"]), int(res["lo"]), int(res["hi"])) == \
        (len(perm), n_runs, lo, hi)
    assert int(res["flags"]) == ordered and int(res["pad"]) == 0


def test_there_are_at_least_eight_known_answers():
    assert len(O.KAT) >= 8


def test_output_meets_the_handlers_contract():
    """grouped by instance, ascending; inside a group by arrival, then concatenation order"""
    for seed in O.FUZZ_SEEDS[:12]:
        case = O.fuzz_order(seed)
        out, perm, res = O.order_records(**case)
        assert np.all(np.diff(out["instance"].astype(np.int64)) >= 0)
        assert sorted(perm.tolist()) == list(range(len(perm)))
        same = np.diff(out["instance"]) == 0
        if case["arrivals"] is None:
            assert np.all(np.diff(perm.astype(np.int64))[same] > 0)
        else:
            arr = np.concatenate(case["arrivals"]).astype(np.int64)[perm]
            d = np.diff(arr)[same]
            assert np.all(d >= 0)
            assert np.all(np.diff(perm.astype(np.int64))[same][d == 0] > 0)
        assert int(res["n_runs"]) == len(np.unique(out["instance"]))


def _code(**kw):
    with pytest.raises(O.OrderError) as ei:
        O.order_records(**kw)
    return ei.value.code


def test_error_codes():
    r = O.records(R.ACCEPT_REPLY, [4, 5])
    a = np.array([1, 2], np.uint32)
    assert _code(sources=[O.records(R.ACCEPT_REPLY, [3, 5])], n_inst=2, inst_base=4) == \
        R.E_NIL_INSTANCE
    assert _code(sources=[O.records(R.ACCEPT_REPLY, [4, 6])], n_inst=2, inst_base=4) == \
        R.E_NIL_INSTANCE
    assert _code(sources=[r] * 17, n_inst=8) == R.E_INVAL
    assert _code(sources=[r, r], n_inst=8, arrivals=[a, None], arrival_bits=2) == R.E_INVAL
    assert _code(sources=[r], n_inst=8, arrivals=[a], arrival_bits=1) == R.E_INVAL
    assert _code(sources=[r], n_inst=8, arrival_bits=3) == R.E_INVAL
    assert _code(sources=[r], n_inst=8, arrivals=[a], arrival_bits=0) == R.E_INVAL
    assert _code(sources=[r], n_inst=0) == R.E_INVAL
    assert _code(sources=[r], n_inst=8, inst_base=0x7FFFFFFF - 6) == R.E_INVAL


def test_fuzz_generator_reaches_every_branch():
    """over the 24 seeds: records in an instance run of 2 or more, records in a run fed by 2 or
    more sources and descents of the concatenation are each at least 2 % of the records; cases
    with arrival keys, cases already ordered and cases needing the 64-bit key are each at least
    2 % of the cases; both sides of the one-launch boundary and both record types occur"""
    tot = dict(n=0, in_runs=0, in_shared_runs=0, descents=0)
    cases = dict(keyed=0, ordered=0, wide=0)
    sizes, dtypes = set(), set()
    for seed in O.FUZZ_SEEDS:
        case = O.fuzz_order(seed)
        assert 1 <= len(case["sources"]) <= R.ORDER_MAX_SRC
        r = O.reach(case)
        for k in tot:
            tot[k] += r[k]
        for k in cases:
            cases[k] += r[k]
        sizes.add(r["n"])
        dtypes.add(case["sources"][0].dtype)
    frac = {k: tot[k] / tot["n"] for k in ("in_runs", "in_shared_runs", "descents")}
    frac.update({k: v / len(O.FUZZ_SEEDS) for k, v in cases.items()})
    print("fuzz reach:", frac)
    assert min(frac.values()) >= 0.02, frac
    assert min(sizes) < R.ORDER_ONE_LAUNCH_MAX < max(sizes) and R.ORDER_ONE_LAUNCH_MAX in sizes
    assert dtypes == {R.ACCEPT_REPLY, R.ACCEPT_MSG}


def test_struct_sizes_match_header(tmp_path):
    src = r"""
    #include <stdio.h>
    #include <stddef.h>
    #include "mpx.h"
    int main(void) {
      printf("%zu %zu %zu %zu %zu %zu %d %d %u %u\n", sizeof(mpx_order_src),
        sizeof(mpx_order_result), offsetof(mpx_order_src, arrival), offsetof(mpx_order_src, n),
        offsetof(mpx_order_result, lo), offsetof(mpx_order_result, flags), MPX_ORDER_MAX_SRC,
        MPX_ORDER_ONE_LAUNCH_MAX, MPX_ORDER_GENERAL, MPX_ORD_WAS_ORDERED);
      return 0;
    }"""
    c, exe = str(tmp_path / "t.c"), str(tmp_path / "t")
    open(c, "w").write(src)
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True,
                                          check=True).stdout.split()]
    assert got == [C.sizeof(_lib.MpxOrderSrc), C.sizeof(_lib.MpxOrderResult),
                   _lib.MpxOrderSrc.arrival.offset, _lib.MpxOrderSrc.n.offset,
                   _lib.MpxOrderResult.lo.offset, _lib.MpxOrderResult.flags.offset,
                   R.ORDER_MAX_SRC, R.ORDER_ONE_LAUNCH_MAX, R.ORDER_GENERAL, R.ORD_WAS_ORDERED]
    assert got[1] == R.ORDER_RESULT.itemsize == 32
    assert got[4] == R.ORDER_RESULT.fields["lo"][1] and got[5] == R.ORDER_RESULT.fields["flags"][1]


def test_null_engine_is_rejected():
    lib = _lib.load()
    res = _lib.MpxOrderResult()
    src = (_lib.MpxOrderSrc * 1)()
    assert lib.mpx_order_records(None, src, 1, 8, 0, 0, 0, None, None, C.byref(res)) == R.E_INVAL
    assert lib.mpx_order_records_reserve(None, 16, 8) == R.E_INVAL
    assert lib.mpx_order_records_dev(None, src, 1, 8, 0, 0, 0, None, None, None, None) == R.E_INVAL
