"""GPU: the single-agent PPO runner end to end (marlsat/runners/single_rl_runner.py) in tmp_path: two cycles on a
generated pool with the evaluation gate at 0, the log's header and lines, the cycle_ / best_eval_ / final_model_
checkpoints, and a resume from them (body restored bitwise, six head tensors re-initialised, optimiser cleared)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(__file__), "..", "configs", "SINGLE_RL_PPO_CONFIG.yaml")
V, C, H, L = 12, 40, 64, 2


def _overrides(tmp_path, **extra):
    ov = {"SAVE_DIR": str(tmp_path / "runs"), "SEED": 7, "ENV_PARAMS.CNF_DATA_DIR": str(tmp_path / "no-such-dir"),
          "ENV_PARAMS.NUM_VARS": V, "ENV_PARAMS.NUM_CLAUSES": C, "ENV_PARAMS.WRAPPER_PARAMS.max_steps": 6,
          "MODEL_PARAMS.HIDDEN_DIM": H, "MODEL_PARAMS.NUM_MESSAGE_PASSING_STEP": L, "TRAIN_PARAMS.NUM_CYCLES": 2,
          "TRAIN_PARAMS.NUM_ENVS": 4, "TRAIN_PARAMS.NUM_STEPS": 4, "TRAIN_PARAMS.EVAL_EPISODES": 5,
          "TRAIN_PARAMS.EVAL_MIN_TRAIN_SOLVE_RATE": 0.0, "TRAIN_PARAMS.LR": 0.003, "PPO_PARAMS.UPDATE_EPOCHS": 1,
          "PPO_PARAMS.NUM_MINIBATCHES": 2, "generation.ENABLED": "true", "generation.NUM_TRAIN": 8}
    ov.update(extra)
    return [f"{k}={v}" for k, v in ov.items()]


def test_runner_two_cycles_checkpoints_and_resume(tmp_path):
    from marlsat.learners import params as Pm
    from marlsat.learners.single_gnn import GNNSingleActorCritic
    from marlsat.runners.single_rl_runner import LOG_FIELDS, load_config, resume, run
    from marlsat.utils import checkpoints as ck

    res = run(load_config(CFG, _overrides(tmp_path)), log=lambda *_: None)
    lines = open(res["log_path"], encoding="utf-8").read().splitlines()
    assert len(lines) == 4 and lines[0].startswith("# Train/Eval Log | start_time=") and lines[0].endswith("| seed=7")
    assert lines[1] + "\n" == LOG_FIELDS
    for n, line in enumerate(lines[2:], 1):
        groups = [g.split() for g in line.split(" | ")]
        assert [len(g) for g in groups] == [1, 4, 4, 4, 4] and groups[0] == [str(n)], line
        vals = [float(v) for g in groups[1:] for v in g]
        assert np.isfinite(vals).all(), line  # the gate is 0: the evaluation ran, no "inf" length
        ep, solve = int(groups[3][0]), float(groups[3][1])
        assert ep >= 4 and 0.0 <= solve <= 1.0
        assert int(groups[4][3]) == 5 and 0.0 <= float(groups[4][0]) <= 1.0 and 1.0 <= float(groups[4][1]) <= 6.0
    assert res["last_eval"]["eval_episodes"] == 5
    names = sorted(os.listdir(res["ckpt_dir"]))
    assert "cycle_1" in names and "cycle_2" in names and "final_model_2" in names
    best = [n for n in names if n.startswith("best_eval_")]
    assert len(best) == 1 and best[0] in ("best_eval_1", "best_eval_2")
    assert not any(n.endswith(".tmp") for n in names)
    # the final checkpoint is the last cycle's train state: two cycles x one epoch x two minibatches = 4 Adam steps
    fin = ck.restore_checkpoint(res["ckpt_dir"], "final_model_", 2)
    last = ck.restore_checkpoint(res["ckpt_dir"], "cycle_", None)
    assert int(fin["step"]) == 4 and int(fin["opt_state"]["0"]["count"]) == 4 and int(last["step"]) == 4
    fin_p, last_p = ck.flatten(fin["params"]), ck.flatten(last["params"])
    assert set(fin_p) == set(last_p) and all(np.array_equal(fin_p[k], last_p[k]) for k in fin_p)
    assert "actor_dense_1/kernel" in fin_p and "agent_id_embedding/embedding" not in fin_p
    assert any(np.abs(v).max() > 0 for v in ck.flatten(fin["opt_state"]["0"]["mu"]).values())
    # resume: the body bitwise, the six head tensors (three layers each) back to the seed's draw, no optimiser state
    net = GNNSingleActorCritic(H, L, V, device="cuda", seed=99)
    net.adam_m.fill_(1.0)
    net.adam_v.fill_(1.0)
    net.adam_count = 9
    resume(net, res["ckpt_dir"], 7, log=lambda *_: None)
    got = net.to_flax()
    init = Pm.single_to_flax(Pm.single_init_flat(H, L, 7), H, L)
    bits = lambda a: np.asarray(a, np.float32).view(np.int32)
    heads = [k for k in got if not k.startswith("encoder/")]
    assert sorted({k.split("/")[0] for k in heads}) == ["actor_dense_1", "actor_dense_2", "actor_output",
                                                         "critic_dense_0", "critic_dense_1", "critic_output"]
    for k in got:
        want = init[k] if k in heads else last_p[k]
        assert np.array_equal(bits(got[k]), bits(want)), k
    moved = [k for k in got if k.startswith("encoder/") and not np.array_equal(bits(last_p[k]), bits(init[k]))]
    assert moved  # training did move the body, so "restored" is not "re-initialised"
    assert any(not np.array_equal(bits(last_p[k]), bits(init[k])) for k in heads if k.endswith("kernel"))
    assert not net.adam_m.any() and not net.adam_v.any() and net.adam_count == 0
    # the runner resumes the same way and trains on
    res2 = run(load_config(CFG, _overrides(tmp_path, **{"TRAIN_PARAMS.RESUME_CKPT_PATH": res["ckpt_dir"],
                                                         "TRAIN_PARAMS.NUM_CYCLES": 1})), log=lambda *_: None)
    assert int(ck.restore_checkpoint(res2["ckpt_dir"], "final_model_", 1)["step"]) == 2


def test_resume_from_a_path_without_a_checkpoint_is_an_error(tmp_path):
    from marlsat.runners.single_rl_runner import load_config, run

    empty = tmp_path / "empty"
    empty.mkdir()
    for path in (str(empty), str(tmp_path / "missing")):
        with pytest.raises(FileNotFoundError, match="RESUME_CKPT_PATH"):
            run(load_config(CFG, _overrides(tmp_path, **{"TRAIN_PARAMS.RESUME_CKPT_PATH": path})), log=lambda *_: None)
