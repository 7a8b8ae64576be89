"""The closed Phase-2 loop through the engine: N engines on one device, every replica leading some
groups and following the others, exchanging only the bytes the engines wrote (cluster_driver.py),
against the whole-replica model (cluster_model.py) after every station of every turn. The scenarios
are cluster_model.CASES; test_cluster_model.py asserts on the model alone that each of them reaches
the seams it is here for (held connections, catch-up logs of 0 and >= 2 instances, late AcceptReplies,
Commit and CommitShort, refusals, idle groups, the MAX_BATCH + 1 batch, the window's end)."""
import pytest

import cluster_driver as D
import cluster_model as M
from minpaxos_amd import records as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_closed_loop_through_the_engine(mk_engine, case):
    sc = M.scenario(*case)
    d = D.run(sc, [D.EngineBackend(mk_engine(sc["N"], sc["mode"])) for _ in range(sc["N"])])
    D.check_end(d)
    if case[0] == "window":     # the fifth proposal finds no free slot: engine and model refuse alike
        assert d.refused == (4, R.E_NIL_INSTANCE) and d.turn == 4
        return
    assert d.turn == sc["turns"]
    if case[0] == "replay":     # replica 2's whole log, read back as getDataFromStableStore reads it
        assert d.replayed == 1
    assert d.checked["accept"] and d.checked["accept_reply"] and d.checked["client"]
    assert d.checked["durable"] and bool(d.checked["commit"]) == (sc["mode"] == M.CLASSIC)
