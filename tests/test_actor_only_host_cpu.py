"""CPU: the host side of actor-only graph batches: the per-instance counts and mean rows of DeviceTemplates, the
argument guards that fail before any launch, the BC switch and the CLI flag."""
import os

import numpy as np
import pytest
import torch

import irregular_pools as ip
from test_irregular_templates_cpu import POOLS

CFG = os.path.join(os.path.dirname(__file__), "..", "configs", "MAPPO_CONFIG.yaml")


@pytest.mark.parametrize("name", POOLS)
def test_actor_only_counts_are_full_less_critic(name):
    from marlsat.learners.graphs import DeviceTemplates, build_templates, instance_graphs

    p = ip.get(name)
    A = -(-p.V // p.vpa)
    t = build_templates(p.pool, p.V, A)
    tpl = DeviceTemplates(t, A, "cpu")
    rows = []
    for n, cl in enumerate(p.pool):
        gr = instance_graphs(cl, p.V, A)[1:]
        nv, nc = sum(len(v) for v, _ in gr), sum(len(c) for _, c in gr)
        vid = np.abs(cl).astype(np.int64) - 1
        ne = sum(int((cl[c] != 0).sum()) for _, c in gr)  # every literal of a related clause is an incidence
        assert (int(tpl.actor_v[n]), int(tpl.actor_c[n]), int(tpl.actor_e[n])) == (nv, nc, ne), n
        assert int(tpl.crit_v[n]) == p.V and int(tpl.crit_c[n]) == p.C and vid.max() < p.V
        rows.append(nv + nc)
    assert tpl.mean_actor_rows == pytest.approx(np.mean(rows))
    assert tpl.mean_actor_rows == pytest.approx(tpl.mean_full_rows - (p.V + p.C))
    for ao, co, want in ((False, False, "full"), (True, False, "actor"), (False, True, "crit")):
        got = tpl.counts(actor_only=ao, critic_only=co)
        assert all(g is getattr(tpl, f"{want}_{s}") for g, s in zip(got, "vce"))


def test_assemble_refuses_both_subsets_before_any_launch():
    from marlsat.learners.graphs import DeviceTemplates, assemble, build_templates

    p = ip.get("k1")
    tpl = DeviceTemplates(build_templates(p.pool, p.V, 2), 2, "cpu")
    z = torch.zeros(1)
    with pytest.raises(ValueError, match="mutually exclusive"):
        assemble(tpl, z, z, torch.zeros(1, dtype=torch.int32), z, critic_only=True, actor_only=True)


def test_graph_batch_records_its_first_graph():
    from marlsat.learners.graphs import GraphBatch

    z = torch.zeros(1)
    assert GraphBatch(1, 3, 0, 0, 0, *([z] * 10)).g0 == 0  # existing positional constructions: a full batch
    assert GraphBatch(1, 2, 0, 0, 0, *([z] * 10), g0=1).g0 == 1


def test_bc_switch_defaults_off():
    import yaml

    from marlsat.runners.behavioral_cloning import bc_settings

    assert bc_settings(None)["ACTOR_ONLY_GRAPHS"] is False
    assert bc_settings({"bc_training": {"ACTOR_ONLY_GRAPHS": True}})["ACTOR_ONLY_GRAPHS"] is True
    with open(CFG) as f:
        committed = yaml.safe_load(f)
    assert committed["bc_training"]["ACTOR_ONLY_GRAPHS"] is False
    assert bc_settings(committed)["ACTOR_ONLY_GRAPHS"] is False


def test_cli_flag_defaults_off():
    from marlsat.utils.policy_solver import build_parser

    base = ["--checkpoint", "c", "--cnf-dir", "d", "--sol-dir", "s"]
    assert build_parser().parse_args(base).actor_only is False
    assert build_parser().parse_args(base + ["--actor-only"]).actor_only is True
