"""GPU: msat_graph_bases + msat_assemble_graph_batch (learners/graphs.assemble) on the irregular pools of
tests/irregular_pools.py against a host reconstruction from the oracle alone (oracle.net.edge_masks /
dense_graph, OracleSATEnv.clause_features / static_var_features): every output buffer, bit for bit, for the
full and the critic-only batch.  The feature buffers start as NaN (graphs.DEBUG_CHECKS), so a row the kernel
leaves unwritten shows up."""
import numpy as np
import pytest
import torch

import irregular_pools as ip
from oracle.sat_env import OracleSATEnv
from test_irregular_templates_cpu import POOLS, dense_from_csr, dense_from_slots, oracle_graphs

pytestmark = pytest.mark.gpu

_EXPECT = {}


def _expected(name):
    """Per pool, once: the oracle's features and, per instance, its graphs and dense adjacency."""
    if name not in _EXPECT:
        p = ip.get(name)
        ora = OracleSATEnv(p.V, p.C, 10, vars_per_agent=p.vpa)
        _, ost = ora.reset(p.pool[p.inst], p.x.astype(np.int32))
        _EXPECT[name] = {"svf": ora.static_var_features(p.pool), "cf": ora.clause_features(ost),
                         "graphs": [oracle_graphs(cl, p.V, p.vpa) for cl in p.pool], "A": ora.num_agents}
    return _EXPECT[name]


def _bits(a):
    a = np.ascontiguousarray(np.asarray(a, np.float32))
    return a.view(np.int32)


def check_assembled_batch(name, critic_only, monkeypatch):
    """assemble over the named pool's samples against the host reconstruction from the oracle (shared with
    tests/test_wide_instances_gpu.py)."""
    from marlsat import SATEnv
    from marlsat.learners import graphs
    from marlsat.learners.graphs import DeviceTemplates, assemble, batch_totals, build_templates

    monkeypatch.setattr(graphs, "DEBUG_CHECKS", True)
    p, e = ip.get(name), _expected(name)
    V, C, A, S = p.V, p.C, e["A"], len(p.inst)
    env = SATEnv(V, C, max_steps=10, vars_per_agent=p.vpa)
    assert env.num_agents == A
    dpool = env.make_pool(p.pool)
    svf = dpool.static_var_features()
    assert np.array_equal(_bits(svf.cpu().numpy()), _bits(e["svf"])), "static_var_features"
    tpl = DeviceTemplates(build_templates(p.pool, V, A), A, "cuda")
    d_inst, d_x = torch.from_numpy(p.inst).cuda(), torch.from_numpy(p.x).cuda()
    b = assemble(tpl, dpool.packed, svf, d_inst, d_x, critic_only=critic_only)
    G = 1 if critic_only else A + 1
    assert (b.S, b.G) == (S, G)
    # ---- the host reconstruction, sample by sample and graph by graph
    vfeat, cfeat, cdeg, dense = [], [], [], []
    vbase, nv, cbase, nc = [], [], [], []
    vr = cr = nnz = 0
    for s, n in enumerate(p.inst):
        gr, Ap, An, _ = e["graphs"][n]
        for rv, rc in gr[:G]:
            Lp, Ln = Ap[np.ix_(rv, rc)], An[np.ix_(rv, rc)]
            f = np.zeros((len(rv), 8), np.float32)
            f[:, 0] = p.x[s, rv]
            f[:, 1:4] = e["svf"][n, rv]
            f[:, 4], f[:, 5] = Lp.sum(1), Ln.sum(1)
            d = np.zeros((len(rc), 4), np.float32)
            d[:, 0], d[:, 1] = Lp.sum(0), Ln.sum(0)
            vfeat.append(f)
            cdeg.append(d)
            cfeat.append(e["cf"][s, rc])
            dense.append((Lp, Ln))
            vbase.append(vr)
            nv.append(len(rv))
            cbase.append(cr)
            nc.append(len(rc))
            vr, cr, nnz = vr + len(rv), cr + len(rc), nnz + int(Lp.sum() + Ln.sum())
    if name == "quirks23" and not critic_only:  # the clause-less agent, in the middle of the batch
        k = [i for i, c in enumerate(nc) if c == 0]
        assert k and all(0 < i < S * G - 1 and nv[i] == 8 and nc[i - 1] > 0 and nc[i + 1] > 0 for i in k)
    assert (b.Nv, b.Nc, b.nnz) == (vr, cr, nnz)
    host = lambda t: t.cpu().numpy()
    for what, got, want in (("vbase", b.vbase, vbase), ("nv", b.nv, nv), ("cbase", b.cbase, cbase), ("nc", b.nc, nc)):
        np.testing.assert_array_equal(host(got), np.array(want, np.int32), err_msg=what)
    got_v, got_c, got_d = host(b.vfeat), host(b.cfeat), host(b.cdeg)
    assert got_v.shape == (vr, 8) and got_c.shape == (cr, 3) and got_d.shape == (cr, 4)
    assert not np.isnan(got_v).any() and not np.isnan(got_c).any() and not np.isnan(got_d).any()
    want_v, want_c, want_d = np.concatenate(vfeat), np.concatenate(cfeat), np.concatenate(cdeg)
    for col, what in ((slice(0, 1), "x"), (slice(1, 4), "svf row"), (slice(4, 6), "incidence counts"), (slice(6, 8), "zeros")):
        assert np.array_equal(_bits(got_v[:, col]), _bits(want_v[:, col])), f"vfeat {what}"
    assert np.array_equal(_bits(got_d), _bits(want_d)), "cdeg"
    assert np.array_equal(_bits(got_c), _bits(want_c)), "cfeat vs OracleSATEnv.clause_features"
    ptr, inc, slots = host(b.ptr), host(b.inc), host(b.slots)
    assert ptr.shape == (vr + 1,) and ptr[0] == 0 and ptr[vr] == nnz and (np.diff(ptr) >= 0).all()
    assert slots.shape == (cr, 3) and (slots >= -1).all()
    for i, (Lp, Ln) in enumerate(dense):
        sp, sn = dense_from_slots(slots, vbase[i], nv[i], cbase[i], nc[i])
        pp, pn = dense_from_csr(ptr, inc, vbase[i], nv[i], cbase[i], nc[i])
        for what, a, w in (("A_pos slots", sp, Lp), ("A_neg slots", sn, Ln), ("A_pos ptr/inc", pp, Lp),
                           ("A_neg ptr/inc", pn, Ln)):
            np.testing.assert_array_equal(a, w, err_msg=f"sample {i // G} graph {i % G}: {what}")
    if critic_only:
        with pytest.raises(ValueError, match="critic_only"):
            assemble(tpl, dpool.packed, svf, d_inst, d_x, critic_only=True, totals=(vr, cr, nnz))
        return
    # planned totals (no device -> host read) give the same batch
    tot = batch_totals(tpl, d_inst, [0, S])
    assert tot == [(vr, cr, nnz)]
    b2 = assemble(tpl, dpool.packed, svf, d_inst, d_x, totals=tot[0])
    assert (b2.Nv, b2.Nc, b2.nnz) == (b.Nv, b.Nc, b.nnz)
    for f in ("vfeat", "cfeat", "cdeg", "slots", "ptr", "vbase", "nv", "cbase", "nc"):
        assert torch.equal(getattr(b, f), getattr(b2, f)), f
    assert torch.equal(b.inc[:nnz], b2.inc[:nnz])
    # two micro-batches planned at once: the second starts its scans at 0 again
    cut = S // 2
    t2 = batch_totals(tpl, d_inst, [0, cut, S])
    assert tuple(np.add(t2[0], t2[1])) == (vr, cr, nnz)
    b3 = assemble(tpl, dpool.packed, svf, d_inst[cut:], d_x[cut:], totals=t2[1])
    v0, c0 = t2[0][0], t2[0][1]
    assert torch.equal(b3.vfeat, b.vfeat[v0:]) and torch.equal(b3.cfeat, b.cfeat[c0:])
    assert torch.equal(b3.ptr, b.ptr[v0:] - t2[0][2])
    assert torch.equal(b3.cbase, b.cbase[cut * G:] - c0) and torch.equal(b3.nc, b.nc[cut * G:])


@pytest.mark.parametrize("critic_only", [False, True], ids=["full", "critic_only"])
@pytest.mark.parametrize("name", POOLS)
def test_assembled_batch_equals_host_reconstruction(name, critic_only, monkeypatch):
    check_assembled_batch(name, critic_only, monkeypatch)
