"""The adapter of tests/accepts_stored_translit.py against hand-worked bytes, and against a second
opinion: the dense window-ordered log built on the host from the same store, through the
unchanged proposer_translit.encode_accepts. No GPU."""
import numpy as np
import pytest

import accepts_stored_kat as K
import accepts_stored_translit as S
import proposer_translit as P
from go_translit import GoPanic
from minpaxos_amd import records as R

MIN, CLASSIC = R.MODE_MIN, R.MODE_CLASSIC


@pytest.mark.parametrize("name", list(K.CASES))
def test_known_answers(name):
    a, want, want_off = K.CASES[name]
    out, off = S.encode_accepts_stored(MIN, K.N, **a)
    assert off.tolist() == want_off.tolist() == K.LENGTHS[name]
    assert out.tobytes() == want.tobytes()
    d_out, d_off = P.encode_accepts(MIN, K.N, **S.dense_args(a))  # the second opinion
    assert d_out.tobytes() == want.tobytes() and d_off.tolist() == want_off.tolist()


def test_known_answer_log_shapes():
    """what the cases are there for: the three ranges, the command counts, the unflagged slot"""
    a = K.CASES["self2_lb_null"][0]
    note = []
    S.encode_accepts_stored(MIN, K.N, note=note, **a)
    assert note == [("from_first", [0, 1, 2]), ("from_pc", [2])]
    note = []
    S.encode_accepts_stored(MIN, K.N, note=note, **K.CASES["self0_lb_null"][0])
    assert note == [("from_pc", [2]), ("from_pc", [])]
    assert [len(S.log_instance(a["st"], None, a["inst"], a["arena"], k)[2]) for k in range(3)] == \
        [0, 1, 3]
    assert not a["inst"]["flags"][0] and a["inst"][5] == a["inst"][1]
    first = a["inst"]["first_cmd"][1:3]
    assert first[0] > first[1]  # reverse window order in the arena
    s = K.CASES["self2_shared"][0]
    assert s["inst"][0] == s["inst"][1]
    lb = K.CASES["self2_lb"][0]
    assert [S.log_instance(lb["st"], lb["lb"], lb["inst"], lb["arena"], k)[1] for k in range(3)] == \
        [P.COMMITTED, P.ACCEPTED, P.COMMITTED]


def test_classic_reads_no_store():
    a = dict(K.CASES["self2_lb_null"][0], st=None, lb=None, inst=None, arena=None, peer_commits=None)
    out, off = S.encode_accepts_stored(CLASSIC, K.N, **a)
    d = {k: v for k, v in a.items() if k not in ("st", "lb", "inst", "arena")}
    w_out, w_off = P.encode_accepts(CLASSIC, K.N, **d)
    assert out.tobytes() == w_out.tobytes() and off.tolist() == w_off.tolist()
    assert out[:13].tobytes() == bytes.fromhex("09 02000000 67000000 21000000")


def test_nil_and_arena_errors():
    a = K.CASES["self2_lb_null"][0]
    bad = dict(a, st=a["st"].copy())
    bad["st"]["status"][1] = P.NIL
    with pytest.raises(GoPanic) as gp:
        S.encode_accepts_stored(MIN, K.N, **bad)
    assert gp.value.code == R.E_NIL_INSTANCE
    bad["st"]["status"][[1, 6]] = [P.ACCEPTED, P.NIL]  # a nil outside every range is not read
    S.encode_accepts_stored(MIN, K.N, **bad)
    bad = dict(a, inst=a["inst"].copy())
    bad["inst"]["first_cmd"][1] = 8
    with pytest.raises(GoPanic) as gp:
        S.encode_accepts_stored(MIN, K.N, **bad)
    assert gp.value.code == R.E_INVAL


@pytest.mark.parametrize("seed", P.FUZZ_SEEDS)
@pytest.mark.parametrize("mode", [MIN, CLASSIC], ids=["min", "classic"])
def test_fuzz_equals_the_dense_form(mode, seed):
    a = S.fuzz_stored(seed, 5, mode)
    out, off = S.encode_accepts_stored(mode, 5, **a)
    w_out, w_off = P.encode_accepts(mode, 5, **S.dense_args(a))
    assert off.tolist() == w_off.tolist() and out.tobytes() == w_out.tobytes()


def test_fuzz_generator_reaches_every_log_shape():
    """a condition on the generator, checked with the transliteration alone"""
    total, frames = dict.fromkeys(S.FRAME_KINDS, 0), 0
    lbs = set()
    for seed in P.FUZZ_SEEDS:
        a = S.fuzz_stored(seed, 5, MIN)
        c, n = S.frame_kinds(a, 5)
        frames += n
        lbs.add(a["lb"] is None)
        for k in S.FRAME_KINDS:
            total[k] += c[k]
    frac = {k: total[k] / frames for k in S.FRAME_KINDS}
    print(frames, frac)
    assert frames > 1000 and lbs == {True, False}
    assert all(f >= 0.02 for f in frac.values()), frac
