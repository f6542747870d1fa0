"""GPU: the actor-only graph batch (learners/graphs.assemble(actor_only=True), msat_assemble_graph_batch_from
with g0 = 1, G = A) on the irregular pools of tests/irregular_pools.py against the oracle-only host
reconstruction of tests/test_irregular_assemble_gpu.py restricted to graphs 1..A: every output buffer, bit for
bit, from NaN-poisoned feature rows (graphs.DEBUG_CHECKS).  The pools hold a padded agent slot, an agent with no
clause and no neighbour between two ordinary graphs, 2- and 1-wide clauses, isolated variables, one agent, and an
instance sampled twice.  Also: the planned totals (batch_totals(actor_only=True)) are the kernel's, and g0 = 0
through the new entry point is the old entry point's output bit for bit."""
import numpy as np
import pytest
import torch

import irregular_pools as ip
from test_irregular_assemble_gpu import _bits, _expected
from test_irregular_templates_cpu import POOLS, dense_from_csr, dense_from_slots

pytestmark = pytest.mark.gpu

FIELDS = ("vfeat", "cfeat", "cdeg", "slots", "ptr", "vbase", "nv", "cbase", "nc")


def _setup(name):
    from marlsat import SATEnv
    from marlsat.learners.graphs import DeviceTemplates, build_templates

    p, e = ip.get(name), _expected(name)
    env = SATEnv(p.V, p.C, max_steps=10, vars_per_agent=p.vpa)
    assert env.num_agents == e["A"]
    dpool = env.make_pool(p.pool)
    tpl = DeviceTemplates(build_templates(p.pool, p.V, e["A"]), e["A"], "cuda")
    return p, e, dpool, dpool.static_var_features(), tpl, torch.from_numpy(p.inst).cuda(), torch.from_numpy(p.x).cuda()


@pytest.mark.parametrize("name", POOLS)
def test_actor_only_batch_equals_host_reconstruction(name, monkeypatch):
    from marlsat.learners import graphs
    from marlsat.learners.graphs import assemble, batch_totals

    monkeypatch.setattr(graphs, "DEBUG_CHECKS", True)
    p, e, dpool, svf, tpl, d_inst, d_x = _setup(name)
    A, S = e["A"], len(p.inst)
    b = assemble(tpl, dpool.packed, svf, d_inst, d_x, actor_only=True)
    G = A
    assert (b.S, b.G, b.g0) == (S, G, 1)
    # ---- the host reconstruction, sample by sample, graphs 1..A
    vfeat, cfeat, cdeg, dense = [], [], [], []
    vbase, nv, cbase, nc = [], [], [], []
    vr = cr = nnz = 0
    for s, n in enumerate(p.inst):
        gr, Ap, An, _ = e["graphs"][n]
        assert len(gr) == A + 1
        for rv, rc in gr[1:]:
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
    if name == "quirks23":  # the clause-less agent, in the middle of the batch
        k = [i for i, c in enumerate(nc) if c == 0]
        assert k and all(0 < i < S * G - 1 and nv[i] == 8 and nc[i - 1] > 0 and nc[i + 1] > 0 for i in k)
    assert (b.Nv, b.Nc, b.nnz) == (vr, cr, nnz)
    host = lambda t: t.cpu().numpy()
    for what, got, want in (("vbase", b.vbase, vbase), ("nv", b.nv, nv), ("cbase", b.cbase, cbase), ("nc", b.nc, nc)):
        np.testing.assert_array_equal(host(got), np.array(want, np.int32), err_msg=what)
    got_v, got_c, got_d = host(b.vfeat), host(b.cfeat), host(b.cdeg)
    assert got_v.shape == (vr, 8) and got_c.shape == (cr, 3) and got_d.shape == (cr, 4)
    assert not np.isnan(got_v).any() and not np.isnan(got_c).any() and not np.isnan(got_d).any()
    want_v = np.concatenate(vfeat)
    want_c = np.concatenate(cfeat) if cr else np.zeros((0, 3), np.float32)
    want_d = np.concatenate(cdeg) if cr else np.zeros((0, 4), np.float32)
    assert np.array_equal(_bits(got_v), _bits(want_v)), "vfeat"
    assert np.array_equal(_bits(got_d), _bits(want_d)), "cdeg"
    assert np.array_equal(_bits(got_c), _bits(want_c)), "cfeat vs OracleSATEnv.clause_features"
    ptr, inc, slots = host(b.ptr), host(b.inc), host(b.slots)
    assert ptr.shape == (vr + 1,) and ptr[0] == 0 and ptr[vr] == nnz and (np.diff(ptr) >= 0).all()
    assert slots.shape == (cr, 3) and (slots >= -1).all() and (slots >> 1 < vr).all()
    assert (inc[:nnz] >= 0).all() and (inc[:nnz] >> 1 < cr).all()
    for i, (Lp, Ln) in enumerate(dense):
        sp, sn = dense_from_slots(slots, vbase[i], nv[i], cbase[i], nc[i])
        pp, pn = dense_from_csr(ptr, inc, vbase[i], nv[i], cbase[i], nc[i])
        for what, a, w in (("A_pos slots", sp, Lp), ("A_neg slots", sn, Ln), ("A_pos ptr/inc", pp, Lp),
                           ("A_neg ptr/inc", pn, Ln)):
            np.testing.assert_array_equal(a, w, err_msg=f"sample {i // G} agent {i % G}: {what}")
    # the actor-only batch is the full batch's rows of graphs 1..A, re-based: same feature bits per agent graph
    full = assemble(tpl, dpool.packed, svf, d_inst, d_x)
    fvb, fnv, fcb, fnc = (host(t).reshape(S, A + 1) for t in (full.vbase, full.nv, full.cbase, full.nc))
    for s in range(S):
        for i in range(A):
            k = s * G + i
            assert nv[k] == fnv[s, 1 + i] and nc[k] == fnc[s, 1 + i]
            assert torch.equal(b.vfeat[vbase[k]:vbase[k] + nv[k]], full.vfeat[fvb[s, 1 + i]:fvb[s, 1 + i] + nv[k]])
            assert torch.equal(b.cfeat[cbase[k]:cbase[k] + nc[k]], full.cfeat[fcb[s, 1 + i]:fcb[s, 1 + i] + nc[k]])
    # planned totals (no device -> host read; DEBUG_CHECKS compares them with msat_graph_bases) give the same batch
    tot = batch_totals(tpl, d_inst, [0, S], actor_only=True)
    assert tot == [(vr, cr, nnz)]
    assert batch_totals(tpl, d_inst, [0, S]) == [(full.Nv, full.Nc, full.nnz)]
    crit = assemble(tpl, dpool.packed, svf, d_inst, d_x, critic_only=True)
    assert (full.Nv - crit.Nv, full.Nc - crit.Nc, full.nnz - crit.nnz) == (vr, cr, nnz)
    b2 = assemble(tpl, dpool.packed, svf, d_inst, d_x, totals=tot[0], actor_only=True)
    assert (b2.Nv, b2.Nc, b2.nnz, b2.g0) == (b.Nv, b.Nc, b.nnz, 1)
    for f in FIELDS:
        assert torch.equal(getattr(b, f), getattr(b2, f)), f
    assert torch.equal(b.inc[:nnz], b2.inc[:nnz])
    # two micro-batches planned at once: the second starts its scans at 0 again
    cut = S // 2
    t2 = batch_totals(tpl, d_inst, [0, cut, S], actor_only=True)
    assert tuple(np.add(t2[0], t2[1])) == (vr, cr, nnz)
    b3 = assemble(tpl, dpool.packed, svf, d_inst[cut:], d_x[cut:], totals=t2[1], actor_only=True)
    v0, c0 = t2[0][0], t2[0][1]
    assert torch.equal(b3.vfeat, b.vfeat[v0:]) and torch.equal(b3.cfeat, b.cfeat[c0:])
    assert torch.equal(b3.ptr, b.ptr[v0:] - t2[0][2])
    assert torch.equal(b3.cbase, b.cbase[cut * G:] - c0) and torch.equal(b3.nc, b.nc[cut * G:])
    with pytest.raises(ValueError, match="mutually exclusive"):
        assemble(tpl, dpool.packed, svf, d_inst, d_x, critic_only=True, actor_only=True)


def _raw_assemble(entry, g0, G, tpl, dpool, svf, d_inst, d_x, sizes, counts):
    """One call of the old (g0 None) or the new entry point into NaN / -1 poisoned buffers."""
    from marlsat import _lib

    S, dev = int(d_inst.shape[0]), d_inst.device
    Nv, Nc, nnz = sizes
    sb = torch.empty((S, 3), dtype=torch.int32, device=dev)
    tot = torch.empty((3,), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib.msat_graph_bases(S, d_inst.data_ptr(), *(c.data_ptr() for c in counts), sb.data_ptr(),
                                         tot.data_ptr(), _lib.stream_ptr(dev)), "msat_graph_bases")
    assert tuple(tot.tolist()) == tuple(sizes)
    fl = lambda *shape: torch.full(shape, float("nan"), device=dev)
    it = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device=dev)
    out = {"vfeat": fl(Nv, 8), "cfeat": fl(Nc, 3), "cdeg": fl(Nc, 4), "slots": it(Nc, 3), "ptr": it(Nv + 1),
           "inc": it(max(nnz, 1)), "vbase": it(S * G), "nv": it(S * G), "cbase": it(S * G), "nc": it(S * G)}
    head = (S,) + (() if g0 is None else (g0,)) + (G, tpl.A, d_x.shape[1], dpool.packed.shape[1])
    _lib.check(getattr(_lib.lib, entry)(
        *head, d_inst.data_ptr(), d_x.data_ptr(), svf.data_ptr(), dpool.packed.data_ptr(), sb.data_ptr(),
        tpl.vgid.data_ptr(), tpl.cgid.data_ptr(), tpl.slots.data_ptr(), tpl.ptr.data_ptr(), tpl.inc.data_ptr(),
        tpl.voff.data_ptr(), tpl.coff.data_ptr(), tpl.eoff.data_ptr(), tpl.poff.data_ptr(), tpl.gv.data_ptr(),
        tpl.gc.data_ptr(), *(out[k].data_ptr() for k in ("vfeat", "cfeat", "cdeg", "slots", "ptr", "inc", "vbase",
                                                        "nv", "cbase", "nc")),
        Nv, nnz, _lib.stream_ptr(dev)), entry)
    return out


@pytest.mark.parametrize("name", POOLS)
def test_first_graph_zero_is_the_old_entry_point_bitwise(name):
    from marlsat import _lib
    from marlsat.learners.graphs import assemble

    p, e, dpool, svf, tpl, d_inst, d_x = _setup(name)
    A = e["A"]
    for G, counts in ((A + 1, tpl.counts()), (1, tpl.counts(critic_only=True))):
        ref = assemble(tpl, dpool.packed, svf, d_inst, d_x, critic_only=G == 1)
        sizes = (ref.Nv, ref.Nc, ref.nnz)
        old = _raw_assemble("msat_assemble_graph_batch", None, G, tpl, dpool, svf, d_inst, d_x, sizes, counts)
        new = _raw_assemble("msat_assemble_graph_batch_from", 0, G, tpl, dpool, svf, d_inst, d_x, sizes, counts)
        for k in old:
            # bit patterns (int32 view: NaN poison left in place would compare equal too, and is refused below)
            assert torch.equal(old[k].view(torch.int32), new[k].view(torch.int32)), (G, k)
        for k in ("vfeat", "cfeat", "cdeg"):
            assert not torch.isnan(new[k]).any(), k
        assert int(new["ptr"][-1]) == ref.nnz and not (new["inc"][:ref.nnz] == -7).any()
    # graphs outside 0..A are refused before any launch
    sb = torch.zeros((len(p.inst), 3), dtype=torch.int32, device="cuda")
    args = [d_inst.data_ptr(), d_x.data_ptr(), svf.data_ptr(), dpool.packed.data_ptr(), sb.data_ptr()] + [8] * 21
    for g0, G in ((1, A + 1), (-1, 1), (A + 1, 1), (1, 0)):
        rc = _lib.lib.msat_assemble_graph_batch_from(len(p.inst), g0, G, A, p.V, p.C, *args, 0, 0, None)
        assert rc == -1 and b"g0" in _lib.lib.msat_last_error(), (g0, G)
