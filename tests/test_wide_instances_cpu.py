"""Instances with more variables than the 256 lanes of the cold kernels' workgroups (tests/irregular_pools.py:
wide257, wide300, wide513k2, wide600), on the host: the host template builder against the oracle's masks at these
sizes, what each pool is there for, where the device template kernels' LDS plan ends at V = 600, and the LDS bound
of msat_static_var_features.  The device side is tests/test_wide_instances_gpu.py; the helpers here are shared
with it."""
import ctypes

import numpy as np
import pytest

import irregular_pools as ip
from test_irregular_templates_cpu import check_instance

WIDE = ip.WIDE
# name -> 0-based own range of the last agent (the clause-less one of the "low-vars" instance)
LAST_AGENT = {"wide257": (250, 257), "wide300": (240, 300), "wide513k2": (456, 513), "wide600": (560, 600)}


def num_agents(p) -> int:
    return -(-p.V // p.vpa)


def template_c_star(V: int = 600, K: int = 3) -> int:
    """The largest C whose graph-template LDS plan (msat_graph_templates_lds_bytes) is at most 65536 bytes, by
    bisection: the plan grows with C."""
    from marlsat import _lib

    need = lambda C: int(_lib.lib.msat_graph_templates_lds_bytes(V, C, K))
    lo, hi = 1, 1 << 15
    assert 0 < need(lo) <= 65536 < need(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if need(mid) <= 65536 else (lo, mid)
    return lo


@pytest.mark.parametrize("name", WIDE)
def test_wide_pools_match_oracle_masks(name):
    p = ip.get(name)
    assert p.pool.shape == (2, p.C, p.K) and p.pool.dtype == np.int32 and p.names == ["quirk-rows", "low-vars"]
    stats = [check_instance(cl, p.V, p.vpa) for cl in p.pool]
    lo, hi = LAST_AGENT[name]
    # low-vars: the last agent's variables (and more) in no clause, that agent (at least) without a related clause
    assert stats[1][0] >= hi - lo and stats[1][1] >= 1
    assert stats[0][1] == 0  # quirk-rows: every agent has a related clause


@pytest.mark.parametrize("name", WIDE)
def test_wide_pools_hold_what_they_are_for(name):
    from marlsat.envs.multi_agent_sat_env import create_agent_groups

    p = ip.get(name)
    V, C, K = p.V, p.C, p.K
    groups = list(create_agent_groups(V, p.vpa).values())
    A = {"wide257": 33, "wide300": 5, "wide513k2": 9, "wide600": 15}[name]
    assert len(groups) == A == num_agents(p) and (V, C, K) == {"wide257": (257, 300, 3), "wide300": (300, 400, 3),
                                                                 "wide513k2": (513, 704, 2),
                                                                 "wide600": (600, 1800, 3)}[name]
    assert (groups[-1][0], groups[-1][-1] + 1) == LAST_AGENT[name]
    D = 2 * V + C
    if name == "wide257":
        assert len({len(g) for g in groups}) == 2 and C % 32 != 0
    if name == "wide300":
        assert 4096 < A * D < 16384
    if name == "wide513k2":
        assert C % 64 == 0 and -(-V // 256) == 3
    if name == "wide600":
        assert A * D >= 16384
    q, low = p.pool
    var = np.abs(q)
    rows = np.arange(C)
    past = rows >= 256
    # a literal 0 among real literals, an all-zero clause, a variable twice with both signs: in clause rows past
    # 255, on variables past (0-based) 255
    mixed = past & (q == 0).any(1) & (var > 256).any(1)
    assert mixed.sum() >= 2
    assert (past & (q == 0).all(1)).sum() == 1
    both = [c for c in rows[past] if any(l > 256 and -l in q[c] for l in q[c])]
    assert len(both) >= 1
    # one variable in more than 64 clauses (its occurrence list is ranked by counting), itself past 255
    occ = np.bincount(var[var > 0] - 1, minlength=V)
    assert occ.argmax() == V - 1 and (var == V).any(1).sum() > 64
    # variables past 255 in no clause
    iso_q, iso_low = ip.isolated_vars(q, V), ip.isolated_vars(low, V)
    assert (iso_low >= 256).sum() >= 1 and V - 1 in iso_low.tolist()
    if V >= 300:
        assert V - 6 in iso_q.tolist() and V - 6 >= 256
    # the low-vars instance: no literal on the last agent's variables or past them, so no clause is related to it
    lo, hi = LAST_AGENT[name]
    assert np.abs(low).max() <= lo and (low != 0).all()
    if name in ("wide513k2", "wide600"):
        assert lo >= 256  # an agent whose own variables all lie past 255


@pytest.mark.parametrize("name", WIDE)
def test_wide_pool_samples_cover_every_instance_and_both_values_of_isolated_variables(name):
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


def test_template_lds_plan_ends_where_its_arithmetic_says():
    """At V = 600, K = 3 the largest C the template kernels take is C* = 1968 (found by bisection on
    msat_graph_templates_lds_bytes; the plan of csrc/graph_templates.hip restated below gives the same)."""
    from marlsat import _lib
    from marlsat.learners.graphs import TEMPLATE_LDS_LIMIT, device_templates_fit

    V, K = 600, 3
    assert TEMPLATE_LDS_LIMIT == 65536
    c_star = template_c_star(V, K)

    def plan_bytes(C):  # gt_plan: vptr, cnt, tmp, occ, relw, relpre, nbrw, nbrpre, scr (words), codes (u16 pairs)
        WC, WV = (C + 31) // 32, (V + 31) // 32
        words = (V + 1) + V + 3 * C + 3 * C + WC + (WC + 1) + WV + (WV + 1) + 257 + (3 * C + 1) // 2
        return (4 * words + 15) & ~15

    for C in (c_star - 1, c_star, c_star + 1, 1800):
        assert int(_lib.lib.msat_graph_templates_lds_bytes(V, C, K)) == plan_bytes(C)
    assert plan_bytes(c_star) <= 65536 < plan_bytes(c_star + 1)
    assert device_templates_fit(V, c_star, K) and not device_templates_fit(V, c_star + 1, K)
    assert c_star == 1968
    assert device_templates_fit(600, 1800, 3)  # wide600 itself


def test_static_var_features_refuses_more_lds_than_a_workgroup_has():
    """msat_static_var_features keeps 8 bytes of LDS per variable: past 160 KiB (V > 20480) it says so, before any
    pointer is read, where it used to leave the launch to fail."""
    from marlsat import _lib

    dummy = ctypes.c_void_p(64)  # never dereferenced: validation fails first
    rc = _lib.lib.msat_static_var_features(dummy, 1, 20481, 10, dummy, None)
    assert rc == -1
    err = _lib.lib.msat_last_error().decode()
    assert "LDS" in err and "static_var_features" in err
    rc = _lib.lib.msat_static_var_features(dummy, 1, 32000, 10, dummy, None)
    assert rc == -1 and "LDS" in _lib.lib.msat_last_error().decode()
    assert _lib.lib.msat_static_var_features(dummy, 0, 20480, 10, dummy, None) == 0  # an empty pool: no launch
