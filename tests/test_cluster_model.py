"""The whole-replica model on its own (cluster_model.py): safety over seeds x {MIN, CLASSIC} x N, and,
for every scenario the closed-loop tests run, the conditions that keep those tests from being
vacuous. Asserted here on the reference alone, so a scenario that stops exercising a seam fails on a
machine without a GPU."""
import struct

import pytest

import cluster_model as M
from minpaxos_amd import records as R

MIN, CLASSIC = M.MIN, M.CLASSIC
SAFETY = [(case, mode, n, seed, seed % 2 == 1) for mode in (MIN, CLASSIC) for n in (3, 5)
          for seed in range(6) for case in ("steady",)] + \
         [("thrifty", CLASSIC, 5, seed, seed % 2 == 1) for seed in range(4)]


def replies(logs, r, k):
    """the ProposeReplyTS frames connection k of replica r read, in order: (OK, CommandId, Value,
    Timestamp, Leader)"""
    out = []
    for log in logs:
        for station in ("propose", "tally", "execute"):
            b = bytes(log["client"][station].get((r, k), b""))
            assert len(b) % R.PROPOSE_REPLY_BYTES == 0
            out += [struct.unpack_from("<Biqqi", b, o) for o in range(0, len(b), R.PROPOSE_REPLY_BYTES)]
    return out


def check_safety(sc, cl, logs):
    N, G = sc["N"], sc["G"]
    for g in range(G):
        lead = cl.rep[g][g % N]
        for i in range(sc["ipg"]):
            held = [(r, x.space[i]) for r, x in enumerate(cl.rep[g]) if x.space[i] is not None]
            done = [(r, x) for r, x in held if x.Status == M.COMMITTED]
            for r, x in done:                       # committed instances agree
                assert (x.Cmds is None or x.Cmds == done[0][1].Cmds or done[0][1].Cmds is None) \
                    and x.Ballot == done[0][1].Ballot, (g, i, r)
            for r, x in held:                       # and nobody holds another value under the ballot
                if lead.space[i] is not None and x.Ballot == lead.space[i].Ballot and x.Cmds is not None:
                    assert x.Cmds == lead.space[i].Cmds, (g, i, r)
        for x in cl.rep[g]:                         # State = the executed prefix run in order
            st = {}
            for i in range(x.first, x.executed):
                for c in x.space[i - x.first].Cmds:
                    M.execute(c, st)
            assert st == x.State and x.executed <= x.committedUpTo + 1, (g, x.Id)
    # every proposal is answered: exactly once, but for the ones MIN drains behind a refused head
    sent = {}
    for (t, r, k, g, cid) in cl.proposed:
        sent.setdefault((r, k, g), []).append(cid)
    unanswered = {g: cl.rep[g][g % N].counts["unanswered"] for g in range(G)}
    seen_false = 0
    for (r, k, g), ids in sent.items():
        got = replies(logs, r, k)
        true_ids = [x[1] for x in got if x[0] == M.TRUE]
        falses = [x for x in got if x[0] == M.FALSE]
        assert all(x[1:4] == (-1, 0, 0) for x in falses)
        seen_false += len(falses)
        if r != g % N:                              # a non-leader answers FALSE, every time
            assert not true_ids and len(falses) == len(ids), (r, k)
            continue
        assert len(set(true_ids)) == len(true_ids) and set(true_ids) <= set(ids), (r, k)
        if sc["mode"] == CLASSIC:
            assert sorted(true_ids) == sorted(ids) and not falses, (r, k)
    for g in range(G):                              # per group: answered + lost = sent to the leader
        conns = [(r, k) for (r, k, g2) in sent if g2 == g and r == g % N]
        n_sent = sum(len(sent[(r, k, g)]) for r, k in conns)
        n_got = sum(len(replies(logs, r, k)) for r, k in conns)
        assert n_got + unanswered[g] == n_sent, g
    return seen_false


@pytest.mark.parametrize("case,mode,n,seed,dreply", SAFETY)
def test_safety(case, mode, n, seed, dreply):
    sc = M.scenario(case, mode, n, seed=seed, dreply=dreply)
    cl, logs, _, panic = M.run_model(sc)
    assert panic is None
    check_safety(sc, cl, logs)


def totals(cl, name):
    return [x.counts[name] for g in cl.rep for x in g]


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_the_gpu_scenarios_are_not_vacuous(case):
    name, mode, n, dreply = case
    sc = M.scenario(*case)
    cl, logs, commit_turns, panic = M.run_model(sc)
    N, G, turns = sc["N"], sc["G"], sc["turns"]
    if name == "window":                            # the fifth proposal finds no free slot
        assert panic is not None and panic[0] == 4 and panic[1].code == R.E_NIL_INSTANCE
        assert min(commit_turns) == 4
        return
    assert panic is None
    n_false = check_safety(sc, cl, logs)
    assert min(commit_turns) >= turns - 2, commit_turns
    catchup = [c for g in cl.rep for x in g for c in x.counts["catchup"]]
    if name in ("steady", "thrifty"):
        assert int(sc["hold"].any(axis=(1, 2)).sum()) >= 2       # a held connection in >= 2 turns
        assert sum(totals(cl, "get_hits")) >= 1                   # a GET meets an earlier PUT ...
        puts = {}                                                 # ... of an earlier turn
        hit = False
        for t, per in enumerate(sc["client_bytes"]):
            for r in range(N):
                for b in per[r]:
                    for o in range(0, len(b), R.CLIENT_PROPOSE_FRAME):
                        _, op, key = struct.unpack_from("<iBq", b, o + 1)
                        if op == M.PUT:
                            puts.setdefault(key, t)
                        elif op == M.GET and puts.get(key, t) < t:
                            hit = True
        assert hit
        assert n_false >= 1                                       # a proposal refused with FALSE
        assert any(n == 0 for log in logs for n in log["n_proposals"])  # a turn without proposals
    if name == "steady" and mode == MIN:
        assert sum(c >= 2 for c in catchup) >= 1 and sum(c == 0 for c in catchup) >= 1
    if name == "steady" and mode == CLASSIC:
        assert sum(totals(cl, "late_ignored")) >= 1               # a late AcceptReply, ignored
    if name == "thrifty":
        kinds = set()
        for log in logs:
            for b in log["commit"].values():
                kinds |= {type(m).__name__ for _, m in M.parse(mode, b)}
        assert kinds == {"Commit", "CommitShort"}
        assert sum(totals(cl, "nil_install")) >= 1                # a follower installs from nil
    if name == "replay":                            # replica 2 leads nothing, one command a record
        assert all(g % N != 2 for g in range(G)) and len(cl.store[2]) == G * turns * R.DURABLE_REC_BYTES
    if name == "wave":
        assert G == 65 and sum(c == 0 for c in catchup) >= G
    if name == "batch":
        lead = cl.rep[0][0]
        assert len(lead.space[0].Cmds) == M.MAX_BATCH and lead.executed >= lead.first + 1
        if mode == CLASSIC:                         # MAX_BATCH + 1 proposals: two instances, one turn
            assert len(logs[0]["accept"][(0, 1)]) > 17 * M.MAX_BATCH
            assert [len(m.Command) for _, m in M.parse(mode, logs[0]["accept"][(0, 1)])
                    if M.Cluster.group_of(cl, m.Instance) == 0] == [M.MAX_BATCH, 1]
        else:                                       # MIN refuses the second batch (bareminpaxos.go:671):
            assert lead.space[1] is not None and len(lead.space[1].Cmds) == 1  # it comes a turn later
            assert n_false >= 1
