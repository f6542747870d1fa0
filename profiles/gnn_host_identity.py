#!/usr/bin/env python3
"""Identity of the GNN's host code (marlsat/learners/gnn.py and what it imports) across a refactor: the library
calls it issues and what they compute.  Run once per source tree on the same built library, then compare:

    MARLSAT_LIB=<libmarlsat.so> python profiles/gnn_host_identity.py --tree <parent worktree> --out parent.json
    MARLSAT_LIB=<libmarlsat.so> python profiles/gnn_host_identity.py --out tree.json
    python profiles/gnn_host_identity.py --compare parent.json tree.json

(the parent as a `git worktree` outside the repository; --tree defaults to the tree this file is in).  `_lib.lib` is
replaced by a recording proxy before marlsat.learners.gnn is imported.  Per call it keeps the export's name, every
argument whose ctypes argtype is not a pointer, and of a pointer argument only whether it is null: addresses come
from the allocator and may differ, everything else may not.

Configurations: path_switches' three precision paths with fuse_phi on and off, the default path with one switch
off (use_planes, use_gru_h2, use_dgrad_h2, use_wgrad_h2 -- the last with the library on bf16x3 -- and use_dual), each
on three of tests/test_gnn_gpu.py's CASES as its _setup builds them; then, on the default path, a critic-only batch,
an actor-only batch and a forward without `save`.  Each runs forward(save=True), backward with seeded cotangents and
adam_step with ktimer = {}, and records: sha256 of logits, value, grads and params; GNNActorCritic.flops; per ktimer
label the launches and the sums of the recorded FLOPs and bytes; the number of calls and a sha256 of the trace (the
trace itself is kept as indices into a table of distinct calls, so --compare can print the first call that differs).

--dry needs no GPU: CPU tensors of made-up row counts, and the proxy answers every export that takes a pointer with
0 instead of calling it (size queries and settings are still called).  It compares traces, FLOPs and label tables;
the outputs it hashes are uninitialised memory's and are left out.
"""
import argparse
import ctypes
import hashlib
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(20, 91, 10, 128, 2, 3, 0), (23, 97, 10, 64, 2, 3, 0), (16, 60, 4, 64, 2, 4, 1)]  # V, C, vpa, H, L, S, mode
SINGLE = {"planes0": {"use_planes": False}, "gru_x3": {"use_gru_h2": False}, "dgrad_x3": {"use_dgrad_h2": False},
          "wgrad_x3": {"use_wgrad_h2": False}, "dual0": {"use_dual": False}}


class Recorder:
    """Stands in for _lib.lib: records (name, non-pointer arguments, null-ness of pointer arguments), forwards."""

    def __init__(self, lib, dry):
        self._lib, self._dry, self._wrapped = lib, dry, {}
        self.calls, self.index, self.trace = [], {}, []  # distinct calls, call -> its index, indices in call order

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name == "msat_last_error":
            return fn
        if name not in self._wrapped:
            ptr = [isinstance(t, type) and issubclass(t, (ctypes.c_void_p, ctypes._Pointer, ctypes.c_char_p))
                   for t in fn.argtypes]
            skip = self._dry and any(ptr)

            def call(*args, _fn=fn, _name=name, _ptr=ptr, _skip=skip):
                assert len(args) == len(_ptr), (_name, len(args), len(_ptr))
                key = _name + "(" + ", ".join(
                    ("null" if a is None or a == 0 else "ptr") if p else repr(a) for a, p in zip(args, _ptr)) + ")"
                i = self.index.get(key)
                if i is None:
                    i = self.index[key] = len(self.calls)
                    self.calls.append(key)
                self.trace.append(i)
                return 0 if _skip else _fn(*args)

            self._wrapped[name] = call
        return self._wrapped[name]

    def cut(self):
        """-> the calls since the last cut, as strings."""
        out, self.trace = [self.calls[i] for i in self.trace], []
        return out


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def fake_batch(case, kind, torch):
    """--dry: a GraphBatch-shaped namespace of CPU tensors (row counts made up, the same in every tree)."""
    V, C, vpa, H, L, S, mode = case
    A = -(-V // vpa)
    g0, G = {"full": (0, A + 1), "critic_only": (0, 1), "actor_only": (1, A)}[kind]
    Nv, Nc = S * V * (1 + (G > 1)), S * C * (1 + (G > 1))
    f, i = (lambda *s: torch.zeros(s)), (lambda *s: torch.zeros(s, dtype=torch.int32))
    return types.SimpleNamespace(S=S, G=G, Nv=Nv, Nc=Nc, nnz=3 * Nc, vfeat=f(Nv, 8), cfeat=f(Nc, 3), cdeg=f(Nc, 4),
                                 slots=i(Nc, 3), ptr=i(Nv + 1), inc=i(3 * Nc), vbase=i(S * G), nv=i(S * G),
                                 cbase=i(S * G), nc=i(S * G), g0=g0)


def run(tree, dry):
    sys.path[:0] = [tree, os.path.join(tree, "marl-sat_amd"), os.path.join(tree, "tests")]
    import numpy as np
    import torch

    from marlsat import _lib

    rec = _lib.lib = Recorder(_lib.lib, dry)
    if dry:
        _lib.stream_ptr = lambda device=None: 0
        torch.cuda.Event = lambda **kw: types.SimpleNamespace(record=lambda: None)  # ktimer's events
    from marlsat.learners import gnn
    from marlsat.learners.gnn import GNNActorCritic

    assert gnn.L_ is rec, "marlsat.learners.gnn was imported before the proxy was in place"
    dev = "cpu" if dry else "cuda"

    def setup(case, kind):
        V, C, vpa, H, L, S, mode = case
        if dry:
            A = -(-V // vpa)
            return GNNActorCritic(H, L, A, -(-V // A), mode, V, device=dev, seed=0), fake_batch(case, kind, torch)
        import test_gnn_gpu
        from marlsat import SATEnv
        from marlsat.learners.graphs import DeviceTemplates, assemble, build_templates
        from marlsat.utils.generate_cnf_dataset import generate_problem_pool

        net, b = test_gnn_gpu._setup(*case)[:2]
        if kind != "full":  # the same instances and samples (_setup's pool and draws) with one head's graphs only
            pool = generate_problem_pool(V, C, 4, size_id=7)
            env = SATEnv(V, C, max_steps=10, vars_per_agent=vpa)
            dpool = env.make_pool(pool)
            tpl = DeviceTemplates(build_templates(pool, V, env.num_agents), env.num_agents, "cuda")
            rng = np.random.default_rng(0)
            inst, x = rng.integers(0, 4, S).astype(np.int32), rng.integers(0, 2, (S, V)).astype(np.uint8)
            b = assemble(tpl, dpool.packed, dpool.static_var_features(), torch.from_numpy(inst).cuda(),
                         torch.from_numpy(x).cuda(), **{kind: True})
        return net, b

    def one(case, kind="full", save=True):
        net, b = setup(case, kind)
        rec.cut()  # the batch's own assembly is not the network's
        GNNActorCritic.flops, GNNActorCritic.ktimer = 0, {}
        actor, critic = kind != "critic_only", kind != "actor_only"
        logits, value, state = net.forward(b, actor=actor, critic=critic, save=save)
        out = {}
        if save:
            g = torch.Generator().manual_seed(3)
            dl = dv = None
            if actor:
                dl = torch.randn(logits.shape, generator=g).to(dev)
                dl = torch.where(torch.isfinite(logits), dl, torch.zeros_like(dl)).contiguous()
            if critic:
                dv = torch.randn(value.shape, generator=g).to(dev).contiguous()
            net.grads.zero_()
            net.backward(b, state, dl, dv)
            net.adam_step(1e-3)
        if not dry:
            torch.cuda.synchronize()
            out["sha256"] = {k: sha(t) for k, t in (("logits", logits), ("value", value), ("grads", net.grads),
                                                    ("params", net.params)) if t is not None}
        calls = rec.cut()
        out["flops"] = float(GNNActorCritic.flops)
        out["labels"] = {k: [len(v), sum(r[2] for r in v), sum(r[3] for r in v)]
                         for k, v in sorted(GNNActorCritic.ktimer.items())}
        out["calls"] = len(calls)
        out["trace_sha256"] = hashlib.sha256("\n".join(calls).encode()).hexdigest()
        out["trace"] = [rec.index[c] for c in calls]
        GNNActorCritic.ktimer = None
        return out

    configs = {}
    base = {k: getattr(GNNActorCritic, k) for k in list(gnn.path_switches("fp16x2")) + ["use_planes", "use_dual"]}
    code = int(rec.msat_get_precision())

    def with_switches(sw, lib_precision, f):
        for k, v in sw.items():
            setattr(GNNActorCritic, k, v)
        _lib.check(rec.msat_set_precision(gnn.PRECISION_CODES[lib_precision]), "msat_set_precision")
        try:
            return f()
        finally:
            for k, v in base.items():
                setattr(GNNActorCritic, k, v)
            _lib.check(rec.msat_set_precision(code), "msat_set_precision")

    default = dict(gnn.path_switches("fp16x2"), use_planes=True, use_dual=True)
    for case in CASES:
        tag = "-".join(map(str, case))
        for prec in ("fp16x2", "bf16x3", "fp32"):
            for fuse in (True, False):
                sw = {**default, **gnn.path_switches(prec), "fuse_phi": fuse}
                configs[f"{tag} {prec} fuse_phi={int(fuse)}"] = with_switches(sw, prec, lambda: one(case))
        for name, off in SINGLE.items():
            configs[f"{tag} {name}"] = with_switches(dict(default, **off), "bf16x3" if name == "wgrad_x3" else "fp16x2",
                                                     lambda: one(case))
        configs[f"{tag} critic_only"] = with_switches(default, "fp16x2", lambda: one(case, "critic_only"))
        configs[f"{tag} actor_only"] = with_switches(default, "fp16x2", lambda: one(case, "actor_only"))
        configs[f"{tag} forward save=False"] = with_switches(default, "fp16x2", lambda: one(case, save=False))
        print(f"{tag}: done, {len(rec.calls)} distinct calls so far", file=sys.stderr, flush=True)
    return {"dry": dry, "call_table": rec.calls, "configs": configs}


def compare(pa, pb, keys=("flops", "labels", "sha256", "calls"), tool="gnn_host_identity",
            what="traces, output hashes, flops and label tables"):
    """``keys``: what is compared per configuration besides the trace (learner_host_identity.py passes its own)."""
    a, b = (json.load(open(p)) for p in (pa, pb))
    if a["dry"] != b["dry"]:
        sys.exit(f"{tool}: one file is a --dry run, the other is not")
    bad = 0
    for name in sorted(set(a["configs"]) | set(b["configs"]), key=lambda n: list(a["configs"]).index(n)
                       if n in a["configs"] else 1 << 30):
        ca, cb = a["configs"].get(name), b["configs"].get(name)
        if ca is None or cb is None:
            bad += 1
            print(f"{name}: only in {pb if ca is None else pa}")
            continue
        ta, tb = ([f["call_table"][i] for i in c["trace"]] for f, c in ((a, ca), (b, cb)))
        diffs = []
        if ta != tb:
            i = next((i for i, (x, y) in enumerate(zip(ta, tb)) if x != y), min(len(ta), len(tb)))
            diffs.append(f"call {i} of {len(ta)} / {len(tb)}:\n    {ta[i] if i < len(ta) else '(end)'}\n    "
                         f"{tb[i] if i < len(tb) else '(end)'}")
        for key in keys:
            if ca.get(key) != cb.get(key):
                diffs.append(f"{key}: {ca.get(key)} != {cb.get(key)}")
        if diffs:
            bad += 1
            print(f"{name}: DIFFERS\n  " + "\n  ".join(diffs))
    n = len(a["configs"])
    calls = sum(c["calls"] for c in a["configs"].values())
    what = "traces, flops and label tables" if a["dry"] else what
    print(f"{tool}: {pa} vs {pb}: {n} configurations, {calls} calls; {what}: "
          f"{'identical' if not bad else f'{bad} configurations differ'}")
    sys.exit(1 if bad else 0)


def main(run=run, compare=compare, doc=__doc__, name="gnn_host_identity"):
    """--tree / --out / --dry / --compare over ``run(tree, dry)`` and ``compare(json, json)``."""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default=HERE, help="root of the source tree to run (default: this file's)")
    ap.add_argument("--out", default=None, help="JSON to write")
    ap.add_argument("--dry", action="store_true", help="no GPU: record the calls without making them")
    ap.add_argument("--compare", nargs=2, metavar="JSON")
    args = ap.parse_args()
    if args.compare:
        compare(*args.compare)
    if not args.out:
        ap.error("--out or --compare")
    res = run(os.path.abspath(args.tree), args.dry)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, separators=(",", ":"))
        f.write("\n")
    print(f"{name}: {len(res['configs'])} configurations, "
          f"{sum(c['calls'] for c in res['configs'].values())} calls -> {args.out}")


if __name__ == "__main__":
    main()
