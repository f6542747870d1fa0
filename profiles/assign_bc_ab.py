"""The assignment predictor's records (run on the GPU from the repo root):

    python profiles/assign_bc_ab.py [--alternations 3] [--skip-learning] [--out FILE]

Three records, no pass marks (there is no parent to race):

1. ``train_epoch`` samples/s of ``AssignLearner`` at uf50-218, H = 128, L = 16, minibatches of 256 (1024 generated
   instances: four Adam steps per epoch), beside ``SinglePPOLearner``'s ``train_cycle`` on the same box at the same
   network size -- a *different workload* (a rollout, two heads, GAE and a clip around the same encoder), there for
   scale only.
2. ``msat_assign_loss`` per call at S = 256 on uf50-218 and uf200-860 against the composition it replaces on the same
   inputs: a float64 torch cross-entropy with its gradient and arg-max, plus ``walksat(max_flips=0)`` on the arg-max for
   the satisfaction check.  Wall clock around ``--reps`` enqueued calls ending in a device synchronise.
3. A learning record: 256 generated uf20-91 instances, 30 epochs (H = 64, L = 4, LEARNING_RATE 1e-3), the three
   curves of both splits; then the median WalkSAT flips on the validation instances from the predicted start and from
   random starts at the same key.  Planted labels are one of many solutions: no bar.

After one untimed pass, timed passes alternate --alternations times; medians and spreads are recorded.  One JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "marl-sat_amd")]


def _stats(xs):
    m = statistics.median(xs)
    return {"runs": xs, "median": m, "spread": (max(xs) - min(xs)) / m if m else 0.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--skip-learning", action="store_true")
    ap.add_argument("--skip-epoch", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    from marlsat import ProblemPool, _lib
    from marlsat.learners.assign_gnn import GNNAssignmentPredictor
    from marlsat.learners.assign_learner import AssignLearner
    from marlsat.random import PRNGKey
    from marlsat.solvers.walksat import solve_pool, walksat

    if not torch.cuda.is_available():
        raise SystemExit("assign_bc_ab: no GPU; nothing is measured on the CPU")
    result = {"device": torch.cuda.get_device_name(0), "alternations": args.alternations, "reps": args.reps}

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    # ---- 1. train_epoch samples/s, beside SinglePPOLearner's train_cycle for scale
    if args.skip_epoch:
        result["train_epoch"] = "unmeasured"
    else:
        from marlsat.learners.single_gnn import GNNSingleActorCritic
        from marlsat.learners.single_ppo_learner import SinglePPOLearner, make_single_env

        V, C, H, L, MB, N = 50, 218, 128, 16, 256, args.instances
        pool = ProblemPool.generate((V, C), N, PRNGKey(V))
        net = GNNAssignmentPredictor(H, L, device="cuda", seed=1)
        learner = AssignLearner(dict(BATCH_SIZE=MB, LEARNING_RATE=1e-4), net, pool, templates="device")
        learner.set_data(np.arange(N, dtype=np.int32), torch.zeros((N, V), dtype=torch.uint8, device="cuda"),
                         pool.planted)
        g = torch.Generator().manual_seed(3)
        B, T = 64, N // 64
        senv = make_single_env(V, C, 8 * T, 5.0)
        snet = GNNSingleActorCritic(H, L, V, device="cuda", seed=1)
        single = SinglePPOLearner(dict(NUM_ENVS=B, NUM_STEPS=T, UPDATE_EPOCHS=1, NUM_MINIBATCHES=N // MB,
                                       NUM_CYCLES=1000, LR=1e-4, GAMMA=0.99, GAE_LAMBDA=0.95, CLIP_EPS=0.2,
                                       ENT_COEF=0.01, VF_COEF=0.5, ANNEAL_LR=False), senv, snet, pool)
        st = {"s": single.init_runner_state(PRNGKey(3))}
        gs = torch.Generator().manual_seed(3)

        def epoch():
            learner.train_epoch(g)

        def cycle():
            st["s"], _ = single.train_cycle(st["s"], gs)

        timed(epoch), timed(cycle)  # untimed pass of each
        ra, rs = [], []
        for _ in range(args.alternations):
            ra.append(N / timed(epoch))
            rs.append(N / timed(cycle))
            print(f"train_epoch {ra[-1]:.1f} samples/s; SinglePPOLearner.train_cycle {rs[-1]:.1f} samples/s",
                  file=sys.stderr, flush=True)
        result["train_epoch"] = {
            "shape": "uf50-218", "hidden": H, "layers": L, "minibatch": MB, "instances": N, "micro": learner.micro,
            "assign_samples_per_s": _stats(ra),
            "single_ppo_samples_per_s_different_workload": _stats(rs),
            "single_ppo_workload": f"train_cycle: {B} envs x {T} steps rollout, 1 epoch of {N // MB} minibatches"}
        del learner, single, net, snet, pool
        torch.cuda.empty_cache()

    # ---- 2. the loss kernel against the composition it replaces
    S, reps = 256, args.reps
    result["loss_kernel"] = {}
    for name, (V, C) in {"uf50-218": (50, 218), "uf200-860": (200, 860)}.items():
        pool = ProblemPool.generate((V, C), 64, PRNGKey(C))
        gen = torch.Generator().manual_seed(V)
        logits = (3.0 * torch.randn((S * V, 2), generator=gen)).cuda()
        labels = torch.randint(0, 2, (S, V), generator=gen, dtype=torch.uint8).cuda()
        pidx = torch.randint(0, 64, (S,), generator=gen, dtype=torch.int32).cuda()
        dl = torch.empty_like(logits)
        pred = torch.empty((S, V), dtype=torch.uint8, device="cuda")
        nll = torch.empty((S,), device="cuda")
        cor = torch.empty((S,), dtype=torch.int32, device="cuda")
        uns = torch.empty((S,), dtype=torch.int32, device="cuda")
        sol = torch.empty((S,), dtype=torch.uint8, device="cuda")
        sums = torch.zeros((5,), dtype=torch.float64, device="cuda")
        stream = _lib.stream_ptr()

        def kernel():
            for _ in range(reps):
                _lib.check(_lib.lib.msat_assign_loss(
                    logits.data_ptr(), S, V, labels.data_ptr(), S, pool.packed.data_ptr(), 64, C, pidx.data_ptr(),
                    dl.data_ptr(), pred.data_ptr(), nll.data_ptr(), cor.data_ptr(), uns.data_ptr(), sol.data_ptr(),
                    sums.data_ptr(), stream), "msat_assign_loss")

        lab64 = labels.long().reshape(-1)
        out = {}

        def composition():
            for _ in range(reps):
                lg = logits.double().requires_grad_(True)
                per = torch.nn.functional.cross_entropy(lg, lab64, reduction="none")
                (per.sum() / (S * V)).backward()
                p = (logits[:, 1] > logits[:, 0]).to(torch.uint8).reshape(S, V)
                correct = (p == labels).sum(1)
                _, solved, _, nun = walksat(pool, pidx, key=PRNGKey(1), max_flips=0, assignments=p)
                out.update(grad=lg.grad, per=per, pred=p, correct=correct, solved=solved, nun=nun)

        timed(kernel), timed(composition)  # untimed pass of each
        # the two compute the same thing (the sizes timed, one comparison): exact outputs equal, gradient to fp32
        same = (torch.equal(pred, out["pred"]) and torch.equal(uns, out["nun"])
                and torch.equal(cor, out["correct"].int())
                and torch.allclose(dl.double(), out["grad"], rtol=2.0 ** -22, atol=0.0))
        tk, tc = [], []
        for _ in range(args.alternations):
            tk.append(timed(kernel) / reps * 1e6)
            tc.append(timed(composition) / reps * 1e6)
            print(f"{name}: msat_assign_loss {tk[-1]:.1f} us/call, torch fp64 CE + walksat(0) {tc[-1]:.1f} us/call",
                  file=sys.stderr, flush=True)
        k, c = _stats(tk), _stats(tc)
        result["loss_kernel"][name] = {"S": S, "num_vars": V, "num_clauses": C, "outputs_match": bool(same),
                                       "kernel_us_per_call": k,
                                       "composition_us_per_call": c, "kernel_over_composition": k["median"] / c["median"]}

    # ---- 3. a learning record
    if args.skip_learning:
        result["learning"] = "unmeasured"
    else:
        V, C, N, E = 20, 91, 256, 30
        pool = ProblemPool.generate((V, C), N, PRNGKey(77))
        net = GNNAssignmentPredictor(64, 4, device="cuda", seed=0)
        learner = AssignLearner(dict(BATCH_SIZE=32, LEARNING_RATE=1e-3), net, pool, templates="device")
        learner.set_data(np.arange(N, dtype=np.int32), torch.zeros((N, V), dtype=torch.uint8, device="cuda"),
                         pool.planted)
        order = np.random.default_rng(0).permutation(N).astype(np.int32)
        tr_rows, va_rows = order[: int(0.8 * N)], order[int(0.8 * N):]
        g = torch.Generator().manual_seed(0)
        curves = {k: [] for k in ("train_loss", "train_var_acc", "train_sol_acc", "val_loss", "val_var_acc",
                                  "val_sol_acc")}
        for _ in range(E):
            tr = learner.train_epoch(g, rows=tr_rows)
            va = learner.evaluate(va_rows)
            for side, m in (("train", tr), ("val", va)):
                for k in ("loss", "var_acc", "sol_acc"):
                    curves[f"{side}_{k}"].append(round(m[k], 5))
        vpool = ProblemPool(pool.clauses[torch.from_numpy(va_rows).long().cuda()], V)
        vl = AssignLearner({}, net, vpool)
        n = len(va_rows)
        pred, _, pre = vl.predict(np.arange(n, dtype=np.int32), torch.zeros((n, V), dtype=torch.uint8, device="cuda"))
        kw = dict(tries=1, max_flips=100_000, max_rounds=1, key=PRNGKey(5))
        warm, cold = solve_pool(vpool, init_assignments=pred, **kw), solve_pool(vpool, **kw)
        result["learning"] = {
            "shape": "uf20-91", "instances": N, "epochs": E, "hidden": 64, "layers": 4, "lr": 1e-3, "curves": curves,
            "val_instances": n, "prediction_alone_solved": int((pre != 0).sum()),
            "walksat_median_flips_predicted_start": float(np.median(warm["flips"][warm["solved"]])),
            "walksat_median_flips_random_start": float(np.median(cold["flips"][cold["solved"]])),
            "walksat_solved_predicted_start": int(warm["solved"].sum()),
            "walksat_solved_random_start": int(cold["solved"].sum())}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
