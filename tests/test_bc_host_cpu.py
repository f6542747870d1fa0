"""CPU tests of the behavioural-cloning host side: the planted expert solutions and their .sol files, the
``bc_training`` config validation, and the argument checks of msat_bc_loss / msat_bc_corrupt (no GPU work is
launched by these calls)."""
import os

import numpy as np
import pytest

from oracle.sat_env import OracleSATEnv


@pytest.mark.parametrize("V,C", [(20, 91), (50, 218)])
def test_planted_solution_satisfies_every_clause(V, C):
    from marlsat.utils.generate_cnf_dataset import generate_sat_clauses, generate_sat_solution

    for seed in (0, 1, 7, 1234, 99991, (1 << 30) - 1):
        cl = generate_sat_clauses(V, C, seed=seed)
        x = generate_sat_solution(V, seed)
        assert x.shape == (V,) and set(np.unique(x)) <= {0, 1}
        status, nun = OracleSATEnv.satisfaction(x[None].astype(np.int32), cl[None])
        assert int(nun[0]) == 0 and status.all(), seed


def test_dataset_with_sol_dir_writes_same_cnf_and_loadable_experts(tmp_path):
    from marlsat.runners.behavioral_cloning import load_expert_data
    from marlsat.utils.generate_cnf_dataset import generate_cnf_dataset_sat

    plain, cnf, sol = (str(tmp_path / d) for d in ("plain", "cnf", "sol"))
    generate_cnf_dataset_sat(5, 20, 91, plain, seed=3)
    generate_cnf_dataset_sat(5, 20, 91, cnf, seed=3, sol_dir=sol)
    names = sorted(os.listdir(plain))
    assert names == sorted(os.listdir(cnf)) == [f"uf20-{i:03d}.cnf" for i in range(1, 6)]
    for n in names:
        assert open(os.path.join(plain, n), "rb").read() == open(os.path.join(cnf, n), "rb").read(), n
    assert sorted(os.listdir(sol)) == [n[:-4] + ".sol" for n in names]
    first = open(os.path.join(sol, "uf20-001.sol")).read()
    assert first.endswith("\n") and first.count("\n") == 1
    assert [abs(int(t)) for t in first.split()] == list(range(1, 21))  # signed DIMACS model
    experts = load_expert_data(cnf, sol)
    assert [e["name"] for e in experts] == names
    for e in experts:
        x = e["expert_solution"]
        assert x.shape == (20,) and set(np.unique(x)) <= {0, 1}
        _, nun = OracleSATEnv.satisfaction(x[None].astype(np.int32), e["problem_clauses"][None])
        assert int(nun[0]) == 0, e["name"]


def test_bc_config_validation():
    from marlsat.runners.behavioral_cloning import bc_settings
    from marlsat.runners.mappo_runner import load_config

    path = os.path.join(os.path.dirname(__file__), "..", "configs", "MAPPO_CONFIG.yaml")
    bc = bc_settings(load_config(path))
    assert bc["NUM_SAMPLES_PER_EXPERT"] == 5 and bc["CORRUPTION_LEVEL"] == 3 and bc["TAU_IMPROVE"] == 0.0
    assert bc["SAVE_PATH"] == "models/bc_pretrained" and bc["SOL_DATA_DIR"]
    assert bc_settings({})["NUM_SAMPLES_PER_EXPERT"] == 5  # the reference's defaults without the section
    with pytest.raises(ValueError, match="MODE"):
        bc_settings(load_config(path, ["bc_training.MODE=single_active"]))
    for coef in ("CONSISTENCY_COEF", "NOOP_SUPERVISION_COEF"):
        with pytest.raises(ValueError, match=coef):
            bc_settings(load_config(path, [f"bc_training.{coef}=0.1"]))


def test_bc_learner_rejects_action_mode_1():
    from marlsat.learners.bc_learner import BCLearner

    class Env:
        action_mode = 1

    with pytest.raises(ValueError, match="mode-0"):
        BCLearner({"MINIBATCH_SIZE": 4}, Env(), None, None)


@pytest.mark.parametrize("bad,msg", [
    (dict(S=-1), "S -1"),
    (dict(A=0), "A 0"),
    (dict(M=0), "M 0"),
    (dict(minibatch=0), "minibatch 0"),
    (dict(logits=None), "NULL"),
    (dict(labels=None), "NULL"),
    (dict(dlogits=None), "NULL"),
    (dict(row_terms=None), "NULL"),
    (dict(sums=None), "NULL"),
])
def test_bc_loss_bad_arguments(bad, msg):
    from marlsat import _lib

    a = dict(logits=8, S=2, A=2, M=3, labels=8, minibatch=2, dlogits=8, row_terms=8, sums=8)  # never dereferenced
    a.update(bad)
    rc = _lib.lib.msat_bc_loss(a["logits"], a["S"], a["A"], a["M"], a["labels"], a["minibatch"], a["dlogits"],
                               a["row_terms"], a["sums"], None)
    assert rc == -1
    assert msg in _lib.lib.msat_last_error().decode()


@pytest.mark.parametrize("bad,msg", [
    (dict(S=-1), "S -1"),
    (dict(V=0), "V 0"),
    (dict(level=-1), "level -1"),
    (dict(n_src=0), "n_src 0"),
    (dict(src=None), "NULL"),
    (dict(src_row=None), "NULL"),
    (dict(dst=None), "NULL"),
])
def test_bc_corrupt_bad_arguments(bad, msg):
    from marlsat import _lib

    a = dict(src=8, n_src=1, src_row=8, S=2, V=5, level=1, dst=8)  # never dereferenced
    a.update(bad)
    rc = _lib.lib.msat_bc_corrupt(a["src"], a["n_src"], a["src_row"], a["S"], a["V"], a["level"], 1, 2, a["dst"], None)
    assert rc == -1
    assert msg in _lib.lib.msat_last_error().decode()


def test_empty_batches_need_no_pointers():
    """S = 0 is a no-op that launches nothing (NULL pointers are only refused with S > 0)."""
    from marlsat import _lib

    assert _lib.lib.msat_bc_loss(None, 0, 2, 3, None, 1, None, None, None, None) == 0
    assert _lib.lib.msat_bc_corrupt(None, 1, None, 0, 5, 1, 0, 0, None, None) == 0
