"""Host graph templates (learners/graphs.py) against the oracle's masked dense encoders' masks
(oracle.net.edge_masks, dense_graph) on irregular CNF instances: literal 0, a variable twice in a clause
(same sign: the adjacency counts 2; both signs), K = 2 and K = 1, variables in no clause, and agents with no
related clause and no neighbour.  Runs on the host; the helpers here are shared with the device tests
(tests/test_irregular_assemble_gpu.py)."""
import numpy as np
import pytest
import torch

import irregular_pools as ip
from oracle import net as onet
from oracle.sat_env import OracleSATEnv

POOLS = ["quirks23", "k2", "k1", "solo"]


def oracle_graphs(clauses, V, vpa):
    """What the reference's masks say each graph of one instance is: [(var ids, clause ids)] for the critic and
    every agent -- own variables in order then the visible others ascending (actor_logits' `nbr`), and the
    related clauses ascending -- plus the dense (V, C) A_pos, A_neg."""
    C = clauses.shape[0]
    ora = OracleSATEnv(V, C, 1, vars_per_agent=vpa)
    Ap, An = onet.dense_graph(clauses[None], V)
    av = torch.from_numpy(ora.agent_vars.astype(np.int64))
    em = onet.edge_masks(Ap, An, av)[0].numpy() > 0  # (A, V, C)
    out = [(np.arange(V), np.arange(C))]
    for i in range(ora.num_agents):
        own = ora.agent_vars[i][ora.agent_vars[i] >= 0]
        visible = em[i].any(-1)
        nbr = np.nonzero(visible & ~ora.own[i])[0]
        out.append((np.concatenate([own, nbr]), np.nonzero(em[i].any(0))[0]))
    return out, Ap[0].numpy(), An[0].numpy(), ora.num_agents


def dense_from_slots(slots, v0, nv, c0, nc):
    """(A_pos, A_neg) (nv, nc) of the graph with var rows v0..v0+nv and clause rows c0..c0+nc from the
    clause-side slots (row << 1 | neg, -1 = none); every slot must name a var row of the same graph."""
    Lp, Ln = np.zeros((nv, nc)), np.zeros((nv, nc))
    for c in range(nc):
        for sl in slots[c0 + c]:
            if sl < 0:
                assert sl == -1
                continue
            r = (int(sl) >> 1) - v0
            assert 0 <= r < nv, f"slot of clause row {c0 + c} names var row {int(sl) >> 1} outside its graph"
            (Ln if sl & 1 else Lp)[r, c] += 1
    return Lp, Ln


def dense_from_csr(ptr, inc, v0, nv, c0, nc):
    """The same from the var-side CSR (ptr (rows + 1,), inc = clause row << 1 | neg)."""
    Lp, Ln = np.zeros((nv, nc)), np.zeros((nv, nc))
    for r in range(nv):
        assert ptr[v0 + r] <= ptr[v0 + r + 1]
        for ent in inc[ptr[v0 + r]:ptr[v0 + r + 1]]:
            c = (int(ent) >> 1) - c0
            assert 0 <= c < nc, f"incidence of var row {v0 + r} names clause row {int(ent) >> 1} outside its graph"
            (Ln if ent & 1 else Lp)[r, c] += 1
    return Lp, Ln


def check_instance(clauses, V, vpa):
    """instance_graphs and build_templates of one instance against the oracle's masks; returns
    (isolated variables, agents without a related clause)."""
    from marlsat.learners.graphs import build_templates, instance_graphs

    ref, Ap, An, A = oracle_graphs(clauses, V, vpa)
    got = instance_graphs(clauses, V, A)
    assert len(got) == A + 1
    for g, ((gv_, gc_), (rv, rc)) in enumerate(zip(got, ref)):
        np.testing.assert_array_equal(gc_, rc, err_msg=f"graph {g}: related clauses")
        np.testing.assert_array_equal(gv_, rv, err_msg=f"graph {g}: own variables, then neighbours ascending")
    t = build_templates(clauses[None], V, A)
    assert t.voff.tolist() == [0, t.gv[0, -1]] and t.coff.tolist() == [0, t.gc[0, -1]]
    assert t.poff.tolist() == [0, t.gv[0, -1] + 1] and t.eoff.tolist() == [0, len(t.inc)] == [0, t.ge[0, -1]]
    assert t.ptr[0] == 0 and t.ptr[-1] == len(t.inc) and (np.diff(t.ptr) >= 0).all()
    assert t.slots.shape == (t.gc[0, -1], 3)
    for g, (rv, rc) in enumerate(ref):
        v0, c0 = int(t.gv[0, g]), int(t.gc[0, g])
        nv, nc = int(t.gv[0, g + 1]) - v0, int(t.gc[0, g + 1]) - c0
        assert (nv, nc) == (len(rv), len(rc))
        np.testing.assert_array_equal(t.vgid[v0:v0 + nv], rv)
        np.testing.assert_array_equal(t.cgid[c0:c0 + nc], rc)
        assert t.ge[0, g] == t.ptr[v0]
        want_p, want_n = Ap[np.ix_(rv, rc)], An[np.ix_(rv, rc)]
        for what, (Lp, Ln) in (("slots", dense_from_slots(t.slots, v0, nv, c0, nc)),
                               ("ptr/inc", dense_from_csr(t.ptr, t.inc, v0, nv, c0, nc))):
            np.testing.assert_array_equal(Lp, want_p, err_msg=f"graph {g}: A_pos from {what}")
            np.testing.assert_array_equal(Ln, want_n, err_msg=f"graph {g}: A_neg from {what}")
    return len(ip.isolated_vars(clauses, V)), sum(len(rc) == 0 for _, rc in ref[1:])


def test_random_irregular_instances_match_oracle_masks():
    rng = np.random.default_rng(2024)
    n_iso = n_empty = n_dup = n_zero = 0
    for _ in range(300):
        V, C, K = int(rng.integers(3, 25)), int(rng.integers(1, 30)), int(rng.integers(1, 4))
        hi = int(rng.integers(1, V + 1))  # literals on the first hi variables only: the others are in no clause
        clauses = rng.integers(-hi, hi + 1, (C, K)).astype(np.int32)
        vpa = int(rng.integers(1, V + 1))
        iso, empty = check_instance(clauses, V, vpa)
        n_iso += iso > 0
        n_empty += empty
        a = np.sort(np.abs(clauses), 1)
        n_dup += bool(((a[:, 1:] == a[:, :-1]) & (a[:, 1:] > 0)).any())
        n_zero += bool((clauses == 0).any())
    # the fuzz has to reach the cases it is for
    assert n_iso >= 100 and n_empty >= 100 and n_dup >= 100 and n_zero >= 100, (n_iso, n_empty, n_dup, n_zero)


@pytest.mark.parametrize("name", POOLS)
def test_named_pools_match_oracle_masks(name):
    p = ip.get(name)
    assert p.pool.shape[1:] == (p.C, p.K) and p.pool.dtype == np.int32 and len(p.names) == p.pool.shape[0]
    stats = [check_instance(cl, p.V, p.vpa) for cl in p.pool]
    if name == "quirks23":  # what each instance is there for
        assert [s[0] for s in stats] == [0, 0, 1, 8] and [s[1] for s in stats] == [0, 0, 0, 1]
        from marlsat.learners.graphs import build_templates

        t = build_templates(p.pool, p.V, 3)
        # instance 3, agent 1 (graph 2): 8 var rows, no clause row, no incidence, between two non-empty graphs
        assert t.gv[3, 3] - t.gv[3, 2] == 8 and t.gc[3, 3] == t.gc[3, 2] and t.ge[3, 3] == t.ge[3, 2]
        assert t.gc[3, 2] > t.gc[3, 1] and t.gc[3, 4] > t.gc[3, 3]


@pytest.mark.parametrize("name", POOLS)
def test_pool_samples_cover_every_instance_and_both_values_of_isolated_variables(name):
    p = ip.get(name)
    N, S = p.pool.shape[0], len(p.inst)
    assert S <= 6 and p.x.shape == (S, p.V) and p.x.dtype == np.uint8 and p.inst.dtype == np.int32
    counts = np.bincount(p.inst, minlength=N)
    assert (counts >= 1).all() and (counts >= 2).any()
    for n in range(N):
        iso = ip.isolated_vars(p.pool[n], p.V)
        if len(iso):
            xs = p.x[p.inst == n][:, iso]
            assert (xs == 0).all(1).any() and (xs == 1).all(1).any()
