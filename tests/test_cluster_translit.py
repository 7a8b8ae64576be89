"""The closed Phase-2 loop on the CPU: cluster_driver.py's turns over the batch transliterations
(TranslitBackend) against the whole-replica model (cluster_model.py), the scenarios and comparisons
of test_gpu_cluster.py. Two readings of the Go, one handler-batch at a time over the engine's arrays
and one message at a time over Go-shaped replicas, must write the same bytes on every connection and
file and hold the same state after every station of every turn."""
import pytest

import cluster_driver as D
import cluster_model as M
from minpaxos_amd import records as R


def backends(sc):
    return [D.TranslitBackend(sc["N"], sc["mode"]) for _ in range(sc["N"])]


@pytest.mark.parametrize("case", M.CASES, ids=M.case_id)
def test_closed_loop_over_the_transliterations(case):
    sc = M.scenario(*case)
    d = D.run(sc, backends(sc))
    D.check_end(d)
    if case[0] == "window":
        assert d.refused == (4, R.E_NIL_INSTANCE) and d.turn == 4
        return
    assert d.turn == sc["turns"]
    if case[0] == "replay":     # replica 2's whole log, read back as getDataFromStableStore reads it
        assert d.replayed == 1
    assert d.checked["accept"] and d.checked["accept_reply"] and d.checked["client"]
    assert d.checked["durable"] and bool(d.checked["commit"]) == (sc["mode"] == M.CLASSIC)


def test_the_comparison_names_the_station_and_the_turn():
    """a backend whose Accept encoder starts every catch-up log one instance late (an off-by-one in
    bareminpaxos.go:504's range) parts from the model where the first non-empty log is due: the
    second turn's proposals, in the Accept bytes"""
    sc = M.scenario("steady", M.MIN, 3)
    bes = backends(sc)
    for b in bes:
        stored = b.encode_accepts_stored
        b.encode_accepts_stored = lambda *a, _f=stored, **k: _f(
            *a, **{**k, "peer_commits": k["peer_commits"] + 1})
    with pytest.raises(D.Divergence, match=r"turn 1, replica \d, station propose: accept bytes"):
        D.run(sc, bes)


@pytest.mark.parametrize("seed", (1, 2, 3))
@pytest.mark.parametrize("n", (3, 5))
@pytest.mark.parametrize("mode", (M.MIN, M.CLASSIC), ids=("min", "classic"))
def test_more_schedules_on_the_cpu(mode, n, seed):
    """other seeds of the steady case (other clients, proposals and held connections), Dreply and,
    for CLASSIC with N = 5, Thrifty alternating with the seed"""
    case = "thrifty" if (mode == M.CLASSIC and n == 5 and seed == 2) else "steady"
    sc = M.scenario(case, mode, n, seed=seed, dreply=seed % 2 == 1)
    d = D.run(sc, backends(sc))
    D.check_end(d)
    assert d.turn == sc["turns"] and d.refused is None
