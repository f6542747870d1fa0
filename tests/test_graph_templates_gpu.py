"""GPU: the graph templates built on the device (learners/graphs.build_templates_device: msat_graph_template_counts,
a scan, msat_graph_template_fill) against the host builder build_templates, torch.equal on all twelve arrays: the
irregular pools of tests/irregular_pools.py (literal 0 and all-zero clauses, a variable twice in a clause, 1- and
2-wide clauses, isolated variables, an agent with no clause, an uneven partition) and generated uf50-218 / uf200-860
pools; the graph batches assembled over either are bitwise equal; a shape past the kernels' LDS bound takes the host
builder."""
import dataclasses

import numpy as np
import pytest
import torch

import irregular_pools as ip

pytestmark = pytest.mark.gpu

ARRAYS = ("vgid", "cgid", "slots", "ptr", "inc", "voff", "coff", "eoff", "poff", "gv", "gc", "ge")
DERIVED = ("full_v", "full_c", "full_e", "crit_v", "crit_c", "crit_e", "actor_v", "actor_c", "actor_e")


def _both(clauses: np.ndarray, V: int, A: int):
    from marlsat import ProblemPool
    from marlsat.learners.graphs import DeviceTemplates, build_templates, build_templates_device

    pool = ProblemPool(clauses, V, "cuda")
    host = DeviceTemplates(build_templates(clauses, V, A), A, "cuda")
    return pool, host, build_templates_device(pool, V, A)


def _assert_equal(dev, host):
    for f in ARRAYS + DERIVED:
        g, w = getattr(dev, f), getattr(host, f)
        assert g.dtype == w.dtype == torch.int32 and g.shape == w.shape, (f, g.dtype, tuple(g.shape), tuple(w.shape))
        assert g.is_contiguous() and torch.equal(g, w), f
    assert (dev.A, dev.G) == (host.A, host.G)
    assert dev.max_full_rows == host.max_full_rows
    assert dev.mean_full_rows == host.mean_full_rows and dev.mean_actor_rows == host.mean_actor_rows


def _agents(p):
    from marlsat.envs.multi_agent_sat_env import create_agent_groups

    return len(create_agent_groups(p.V, p.vpa))


@pytest.mark.parametrize("name", ["quirks23", "k2", "k1", "solo"])
def test_device_templates_equal_host_builder_on_irregular_pools(name):
    p = ip.get(name)
    _, host, dev = _both(p.pool, p.V, _agents(p))
    _assert_equal(dev, host)
    if name == "quirks23":  # the pool does hold what it is here for: an agent's graph with no clause row
        gc = host.gc.cpu().numpy()
        assert (np.diff(gc[3]) == 0).any()


@pytest.mark.parametrize("V,C,N,A", [(50, 218, 8, 10), (200, 860, 2, 25)])
def test_device_templates_equal_host_builder_on_generated_pools(V, C, N, A):
    from marlsat import ProblemPool

    gen = ProblemPool.generate((V, C, 3), N, 11)
    _, host, dev = _both(gen.clauses.cpu().numpy(), V, A)
    _assert_equal(dev, host)
    assert dev.gv.shape == (N, A + 2)


def test_more_instances_than_one_scan_block_and_one_instance():
    """The offsets come from a scan over N: 300 small instances (k2's shape), and N = 1."""
    from marlsat import ProblemPool

    gen = ProblemPool.generate((12, 20, 2), 300, 4, reject_isolated=False)
    cl = gen.clauses.cpu().numpy()
    for clauses, A in ((cl, 3), (cl[:1], 5)):
        _, host, dev = _both(clauses, 12, A)
        _assert_equal(dev, host)


def _batches_equal(a, b):
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if torch.is_tensor(x):
            assert x.dtype == y.dtype and x.shape == y.shape, f.name
            assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), f.name
        else:
            assert x == y, f.name


@pytest.mark.parametrize("kind", ["full", "actor_only", "critic_only"])
def test_assembled_batches_are_bitwise_equal(kind):
    from marlsat.learners.graphs import assemble

    p = ip.get("quirks23")
    pool, host, dev = _both(p.pool, p.V, _agents(p))
    svf = pool.static_var_features()
    inst, x = torch.from_numpy(p.inst).cuda(), torch.from_numpy(p.x).cuda()
    kw = dict(actor_only=kind == "actor_only", critic_only=kind == "critic_only")
    a = assemble(dev, pool.packed, svf, inst, x, **kw)
    b = assemble(host, pool.packed, svf, inst, x, **kw)
    assert a.S == len(p.inst) and a.Nv > 0 and a.Nc > 0 and a.nnz > 0
    _batches_equal(a, b)


def test_shape_past_the_lds_bound_takes_the_host_builder(monkeypatch):
    from marlsat import _lib
    from marlsat.learners import graphs

    V, C, A = 12, 2300, 3
    assert _lib.lib.msat_graph_templates_lds_bytes(V, C, 3) > graphs.TEMPLATE_LDS_LIMIT
    assert not graphs.device_templates_fit(V, C, 3) and graphs.device_templates_fit(200, 860, 3)
    from marlsat import ProblemPool

    cl = ProblemPool.generate((V, C, 3), 1, 2).clauses.cpu().numpy()
    calls = []
    real = graphs.build_templates
    monkeypatch.setattr(graphs, "build_templates", lambda *a: (calls.append(1), real(*a))[1])
    pool, host, dev = _both(cl, V, A)
    assert len(calls) == 2  # the reference and the fallback
    _assert_equal(dev, host)
    # and the kernels themselves refuse the shape with a message
    gv = torch.zeros((1, A + 2), dtype=torch.int32, device="cuda")
    rc = _lib.lib.msat_graph_template_counts(pool.clauses.data_ptr(), 1, C, 3, V, A, gv.data_ptr(), gv.data_ptr(),
                                             gv.data_ptr(), None)
    assert rc == -1 and "LDS" in _lib.lib.msat_last_error().decode()


def test_learners_take_device_templates():
    from marlsat import SATEnv
    from marlsat.learners.bc_learner import BCLearner
    from marlsat.learners.gnn import GNNActorCritic
    from marlsat.learners.mappo_gnn_sat_learner import MAPPOLearner

    p = ip.get("learner")
    env = SATEnv(p.V, p.C, max_steps=8, vars_per_agent=p.vpa)
    pool = env.make_pool(p.pool)
    net = GNNActorCritic(64, 2, env.num_agents, env.max_vars_per_agent, 0, p.V, device="cuda", seed=1)
    cfg = dict(NUM_ENVS=4, NUM_STEPS=2, MINIBATCH_SIZE=4)
    a, b = MAPPOLearner(cfg, env, net, pool), MAPPOLearner(cfg, env, net, pool, templates="device")
    assert a.templates == "host" and b.templates == "device"
    _assert_equal(b.tpl, a.tpl)
    assert (a.micro, a.chunk, a.actor_chunk) == (b.micro, b.chunk, b.actor_chunk)
    _assert_equal(BCLearner(cfg, env, net, pool, templates="device").tpl, BCLearner(cfg, env, net, pool).tpl)
    with pytest.raises(ValueError, match="templates"):
        MAPPOLearner(cfg, env, net, pool, templates="gpu")
