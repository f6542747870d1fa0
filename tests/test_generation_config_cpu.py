"""The ``generation`` config section on the host (no GPU): marlsat/utils/generation.py parses and validates it,
says which train pool every update runs on, and names the keys the pools are drawn from; and the argument checks
of msat_pool_generate / msat_graph_template_* (MSAT_EBADARG with a message before any launch)."""
import os

import pytest

from marlsat.utils import generation as g

CFG = os.path.join(os.path.dirname(__file__), "..", "configs", "MAPPO_CONFIG.yaml")


def test_committed_config_has_the_section_disabled_with_the_documented_defaults():
    from marlsat.runners.mappo_runner import load_config

    cfg = load_config(CFG)
    assert cfg["generation"] == {"ENABLED": False, "NUM_TRAIN": 1024, "NUM_EVAL": 256, "REFRESH_EVERY": 0,
                                 "MAX_ATTEMPTS": 64}
    plan = g.parse_generation(cfg)
    assert plan == g.GenerationPlan(False, 1024, 256, 0, 64)
    assert g.parse_generation({}) == plan and g.parse_generation({"generation": None}) == plan
    on = g.parse_generation(load_config(CFG, ["generation.ENABLED=true", "generation.REFRESH_EVERY=5"]))
    assert on.enabled and on.refresh_every == 5 and on.num_train == 1024


@pytest.mark.parametrize("section,word", [
    ({"ENABLED": "yes"}, "ENABLED"),
    ({"ENABLED": 1}, "ENABLED"),
    ({"NUM_TRAIN": 0}, "NUM_TRAIN"),
    ({"NUM_TRAIN": 2.5}, "NUM_TRAIN"),
    ({"NUM_EVAL": -1}, "NUM_EVAL"),
    ({"NUM_EVAL": True}, "NUM_EVAL"),
    ({"REFRESH_EVERY": -1}, "REFRESH_EVERY"),
    ({"REFRESH_EVERY": "3"}, "REFRESH_EVERY"),
    ({"MAX_ATTEMPTS": 0}, "MAX_ATTEMPTS"),
    ({"MAX_ATTEMPTS": 256}, "MAX_ATTEMPTS"),
    ({"REFRESH": 3}, "REFRESH"),
    ([1, 2], "mapping"),
])
def test_bad_values_are_refused_with_a_message(section, word):
    with pytest.raises(ValueError, match=word):
        g.parse_generation({"generation": section})


def test_refresh_schedule():
    """Update u trains on pool u // REFRESH_EVERY; 0 never refreshes.  A new pool is drawn right before the first
    update of its block and never before update 0."""
    plan = lambda r: g.parse_generation({"generation": {"ENABLED": True, "REFRESH_EVERY": r}})
    assert plan(0).schedule(7) == [0, 0, 0, 0, 0, 0, 0]
    assert plan(1).schedule(7) == [0, 1, 2, 3, 4, 5, 6]
    assert plan(3).schedule(7) == [0, 0, 0, 1, 1, 1, 2]
    assert [u for u in range(7) if plan(0).refresh_before(u)] == []
    assert [u for u in range(7) if plan(1).refresh_before(u)] == [1, 2, 3, 4, 5, 6]
    assert [u for u in range(7) if plan(3).refresh_before(u)] == [3, 6]
    with pytest.raises(ValueError):
        plan(3).pool_of_update(-1)


def test_pool_keys_share_a_seed_and_never_share_a_counter():
    ev, t0, t1 = g.eval_pool_key(42), g.train_pool_key(42, 0), g.train_pool_key(42, 1)
    assert ev.seed == t0.seed == t1.seed
    assert len({ev.counter, t0.counter, t1.counter}) == 3
    assert g.eval_pool_key(43).seed != ev.seed
    from marlsat.random import PRNGKey, split

    assert ev.seed not in {k.seed for k in split(PRNGKey(42), 2)}  # not the runner's own chain
    assert g.instance_name(12, 0) == "uf12-001.cnf" and g.instance_name(200, 41) == "uf200-042.cnf"


def _gen(L, **kw):
    a = dict(N=4, V=20, C=40, K=3, seed=1, counter=0, reject=1, max_attempts=64, clauses=8, planted=8, attempts=8)
    a.update(kw)
    return L.msat_pool_generate(a["N"], a["V"], a["C"], a["K"], a["seed"], a["counter"], a["reject"],
                                a["max_attempts"], a["clauses"], a["planted"], a["attempts"], None)


@pytest.mark.parametrize("bad,word", [
    (dict(N=-1), "num_problems"),
    (dict(V=0), "num_vars"),
    (dict(V=32001, C=20000), "num_vars"),
    (dict(C=0), "num_clauses"),
    (dict(K=0), "clause_width"),
    (dict(K=4), "clause_width"),
    (dict(V=2, C=5, K=3), "distinct"),
    (dict(C=(1 << 24) - 1), "24-bit"),
    (dict(max_attempts=0), "max_attempts"),
    (dict(max_attempts=256), "max_attempts"),
    (dict(V=20, C=6, K=3), "never be accepted"),
    (dict(clauses=None), "NULL"),
    (dict(planted=None), "NULL"),
    (dict(attempts=None), "NULL"),
])
def test_pool_generate_refuses_bad_arguments(bad, word):
    from marlsat import _lib

    L = _lib.lib
    assert _gen(L, **bad) == -1
    assert word in L.msat_last_error().decode()


def test_pool_generate_empty_call_and_rejection_off():
    from marlsat import _lib

    L = _lib.lib
    assert _gen(L, N=0, clauses=None, planted=None, attempts=None) == 0  # no launch, no pointer needed
    assert _gen(L, N=0, V=20, C=6, reject=0, clauses=None, planted=None, attempts=None) == 0  # K C < V is fine then


def test_graph_template_entry_points_refuse_bad_arguments():
    from marlsat import _lib

    L = _lib.lib
    assert L.msat_graph_templates_lds_bytes(0, 10, 3) == 0 and L.msat_graph_templates_lds_bytes(10, 10, 4) == 0
    small, big = L.msat_graph_templates_lds_bytes(200, 860, 3), L.msat_graph_templates_lds_bytes(12, 2300, 3)
    assert 0 < small <= 65536 < big
    assert L.msat_graph_templates_lds_bytes(50, 218, 3) < small and small % 16 == 0
    counts = lambda N=2, C=40, K=3, V=12, A=3, cl=8, gv=8: L.msat_graph_template_counts(cl, N, C, K, V, A, gv, 8, 8,
                                                                                         None)
    for kw, word in ((dict(N=-1), "num_problems"), (dict(V=0), "num_vars"), (dict(C=0), "num_clauses"),
                     (dict(K=4), "clause_width"), (dict(A=0), "num_agents"), (dict(A=13), "num_agents"),
                     (dict(C=2300), "LDS"), (dict(cl=None), "NULL"), (dict(gv=None), "NULL")):
        assert counts(**kw) == -1, kw
        assert word in L.msat_last_error().decode(), (kw, L.msat_last_error())
    assert counts(N=0, cl=None, gv=None) == 0
    fill = lambda N=2, voff=8, vgid=8, tc=5, cgid=8, te=5, inc=8: L.msat_graph_template_fill(
        8, N, 40, 3, 12, 3, voff, 8, 8, 8, 7, tc, te, vgid, cgid, 8, 8, inc, None)
    for kw, word in ((dict(voff=None), "offset"), (dict(vgid=None), "output"), (dict(cgid=None), "output"),
                     (dict(inc=None), "output"), (dict(tc=-1), "negative")):
        assert fill(**kw) == -1, kw
        assert word in L.msat_last_error().decode(), (kw, L.msat_last_error())
    assert fill(N=0) == 0
