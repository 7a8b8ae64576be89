"""The client-side transliteration (tests/client_translit.py) against the hand-traced known
answers of tests/client_kat.py, and the mix of wire.random_client_stream: CPU only."""
import numpy as np
import pytest

import client_kat
import client_translit as T
from minpaxos_amd import records as R
from minpaxos_amd import wire

FUZZ_SEEDS = range(24)


def test_at_least_ten_known_answers():
    assert len(client_kat.KAT_CLIENT) >= 10
    assert len({c["name"] for c in client_kat.KAT_CLIENT}) == len(client_kat.KAT_CLIENT)


@pytest.mark.parametrize("case", client_kat.KAT_CLIENT, ids=lambda c: c["name"])
def test_known_answer(case):
    bufs = client_kat.kat_bytes(case)
    got = T.decode_client_streams(bufs, case["groups"], case["n_groups"])
    at = 0
    for k, (props, dropped, consumed, why, code) in enumerate(case["want"]):
        assert T.client_listener(bufs[k]) == (props, dropped, consumed, why, code)
        cr = got["conn_res"][k]
        assert (int(cr["first"]), int(cr["consumed"]), int(cr["n_proposals"]),
                int(cr["n_dropped"]), int(cr["stop_reason"]), int(cr["stop_code"])) == \
            (at, consumed, len(props), dropped, why, code)
        for i, (cid, op, key, val, ts) in enumerate(props):
            m = got["meta"][at + i]
            assert (int(m["command_id"]), int(got["op"][at + i]), int(got["key"][at + i]),
                    int(got["val"][at + i]), int(m["timestamp"]), int(m["client"])) == \
                (cid, op, key, val, ts, k)
        at += len(props)
    assert int(got["res"]["n_proposals"]) == at == len(got["op"])
    assert got["prop_off"].tolist() == case["prop_off"]
    assert got["send_off"].tolist() == case["send_off"]
    assert int(got["res"]["n_sends"]) == case["send_off"][-1]
    assert int(got["res"]["n_partial"]) == sum(w[3] == client_kat.PARTIAL for w in case["want"])


def test_frame_builders_are_what_the_reference_marshals():
    """Propose.Marshal / Read.Marshal / ProposeAndRead.Marshal behind their code bytes"""
    assert wire.propose(7, 1, 10, 20, 1000).hex() == client_kat._P1
    assert wire.read(9, 12).hex() == client_kat._R
    assert wire.propose_and_read(10, 1, 13, 14, 15).hex() == client_kat._PAR
    assert len(wire.propose(0, 0, 0, 0, 0)) == R.CLIENT_PROPOSE_FRAME
    assert len(wire.read(0, 0)) == R.CLIENT_READ_FRAME


def test_send_counts_follow_ceil():
    for n_g, sends in ((0, 0), (1, 1), (4999, 1), (5000, 1), (5001, 2), (10000, 2)):
        got = T.decode_client_streams([bytes(30 * n_g)], [0], 1)
        assert got["prop_off"].tolist() == [0, n_g] and got["send_off"].tolist() == [0, sends]


def test_random_client_stream_reaches_every_frame_kind():
    """each of PROPOSE, READ, PROPOSE_AND_READ and unknown is at least 0.02 of the frames the
    transliteration passes over the fuzz seeds"""
    kinds = {}
    for seed in FUZZ_SEEDS:
        rng = np.random.default_rng(1000 + seed)
        s = wire.random_client_stream(rng, 400)
        props, dropped, consumed, why, code = T.client_listener(s, kinds)
        assert consumed == len(s) and why == R.DECODE_END and code == -1
    total = sum(kinds.values())
    assert total == 24 * 400
    for kind in ("propose", "read", "propose_and_read", "unknown"):
        assert kinds.get(kind, 0) >= 0.02 * total, (kind, kinds)
