"""CPU: the host side of the assignment predictor -- msat_assign_loss' argument checks under AddressSanitizer
(tests/assign_host_check.cpp, a stand-alone program: nothing is loaded into Python under a sanitizer), the assign
parameter layout and its flax round trip on NumPy, the encoder block's exchange with the other two layouts, the config
(configs/ASSIGN_BC_CONFIG.yaml) and its validation, the log line, the split and solve_pool's signature."""
import inspect
import json
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

CONFIG = os.path.join(ROOT, "configs", "ASSIGN_BC_CONFIG.yaml")


def test_assign_host_glue_under_asan():
    """Every MSAT_EBADARG case of msat_assign_loss and S == 0, against the library's AddressSanitizer objects
    (marl-sat_amd/Makefile `debug`), with no ASan report.  Skips only where no build ran."""
    binary = os.path.join(ROOT, "marl-sat_amd", "build", "asan", "assign_host_check")
    status = os.path.join(ROOT, "marl-sat_amd", "marlsat", "lib", "debug_build_status.json")
    if not os.path.exists(binary):
        if os.path.exists(status):
            pytest.fail(f"assign_host_check missing: build()'s 'make debug' exited "
                        f"{json.load(open(status)).get('make_debug_rc')}")
        pytest.skip("assign_host_check not built (make -C marl-sat_amd debug; __graft_entry__.build() does)")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=23")
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "assign_host_check: ok" in r.stdout and "AddressSanitizer" not in r.stderr


def test_binding_and_header_declare_the_entry_point():
    from marlsat import _lib

    assert "msat_assign_loss" in _lib.EXPORTED and _lib.lib.msat_version() == 3
    assert len(_lib.lib.msat_assign_loss.argtypes) == 17


@pytest.mark.parametrize("H,L", [(64, 2), (128, 16), (32, 1)])
def test_assign_layout_offsets_and_round_trip(H, L):
    from marlsat.learners import params as P

    lay = P.assign_layout(H, L)
    full = P.layout(H, L, 1, 1)
    assert [k for k in lay if k.startswith("enc.")] == [k for k in full if k.startswith("enc.")]
    assert all(lay[k] == full[k] for k in lay if k in full)
    assert {k: lay[k] for k in lay if not k.startswith("enc.")} == {
        "assign.s0_w": (2 * H, 128), "assign.s0_b": (128,), "assign.s1_w": (128, 64), "assign.s1_b": (64,),
        "assign.so_w": (64, 2), "assign.so_b": (2,)}
    tab, total = P.offsets(lay)
    assert all(o % 4 == 0 for o, _ in tab.values()) and total % 4 == 0  # 16-byte aligned tensors
    ends = sorted((o, o + int(np.prod(shp))) for o, shp in tab.values())
    assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:])) and ends[-1][1] <= total
    flat = P.assign_init_flat(H, L, seed=3)
    assert flat.dtype == np.float32 and flat.shape == (total,)
    tree = P.assign_to_flax(flat, H, L)
    assert {"assign_dense_0/kernel", "assign_dense_1/bias", "assign_output/kernel", "encoder/update_c/hn/bias",
            f"encoder/LayerNorm_{3 * L - 1}/scale"} <= set(tree)
    assert not any(k.startswith(("agent_id_embedding", "critic_", "actor_")) for k in tree)
    assert tree["assign_output/kernel"].shape == (64, 2) and tree["assign_dense_0/kernel"].shape == (2 * H, 128)
    assert sum(v.size for v in tree.values()) == sum(int(np.prod(s)) for s in lay.values()) - 3 * 2 * H  # bh's zeros
    assert np.array_equal(P.assign_from_flax(tree, H, L).view(np.int32), flat.view(np.int32))
    rng = np.random.default_rng(0)
    rnd = {k: rng.standard_normal(v.shape).astype(np.float32) for k, v in tree.items()}
    again = P.assign_to_flax(P.assign_from_flax(rnd, H, L), H, L)
    assert set(again) == set(rnd)
    assert all(np.array_equal(again[k].view(np.int32), rnd[k].view(np.int32)) for k in rnd)
    # the encoder starts from what init_flat draws for it at the same seed
    other = P.to_flax(P.init_flat(H, L, 2, 5, 0, 16, seed=3), H, L, 2, 5)
    enc = [k for k in tree if k.startswith("encoder/")]
    assert enc and all(np.array_equal(tree[k].view(np.int32), other[k].view(np.int32)) for k in enc)


def test_an_encoder_written_here_reads_into_the_other_networks():
    """assign_to_flax's encoder block under the shared names: from_flax and single_from_flax take it bitwise."""
    from marlsat.learners import params as P

    H, L = 64, 2
    rng = np.random.default_rng(1)
    mine = P.assign_to_flax(rng.standard_normal(P.offsets(P.assign_layout(H, L))[1]).astype(np.float32), H, L)
    enc = {k: v for k, v in mine.items() if k.startswith("encoder/")}
    mappo = P.to_flax(P.init_flat(H, L, 2, 10, 0, 16, seed=5), H, L, 2, 10)
    single = P.single_to_flax(P.single_init_flat(H, L, seed=5), H, L)
    assert set(enc) == {k for k in mappo if k.startswith("encoder/")} == {k for k in single if k.startswith("encoder/")}
    got_m = P.to_flax(P.from_flax({**mappo, **enc}, H, L, 2, 10), H, L, 2, 10)
    got_s = P.single_to_flax(P.single_from_flax({**single, **enc}, H, L), H, L)
    for k, v in enc.items():
        assert np.array_equal(got_m[k].view(np.int32), v.view(np.int32)), k
        assert np.array_equal(got_s[k].view(np.int32), v.view(np.int32)), k
    assert np.array_equal(got_m["critic_output/kernel"], mappo["critic_output/kernel"])  # the rest is untouched


def _settings(*overrides):
    from marlsat.runners.bc_runner import assign_settings, load_config

    return assign_settings(load_config(CONFIG, overrides))


def test_config_loads_with_the_reference_defaults():
    s = _settings()
    assert (s["SEED"], s["LEARNING_RATE"], s["EPOCHS"], s["BATCH_SIZE"], s["TRAIN_RATIO"]) == (0, 1e-4, 100, 32, 0.8)
    assert s["SAVE_DIR"] == "experiments/bc" and s["INPUT"] == "zeros" and (s["H"], s["L"]) == (128, 8)
    assert s["SOLVE_MISSING_EXPERTS"] is False and not s["generation"].enabled and "MICROBATCH_BYTES" not in s
    from marlsat.runners.bc_runner import assign_settings

    bare = assign_settings({})  # an empty config is the reference's main()
    assert (bare["SEED"], bare["LEARNING_RATE"], bare["EPOCHS"], bare["BATCH_SIZE"], bare["TRAIN_RATIO"]) == (
        0, 1e-4, 100, 32, 0.8)
    s = _settings("generation.ENABLED=true", "generation.NUM_TRAIN=8", "NUM_VARS=12", "NUM_CLAUSES=40", "EPOCHS=2",
                  "network.H=64", "INPUT=corrupted", "MICROBATCH_BYTES=1000000000")
    assert s["generation"].enabled and s["generation"].num_train == 8 and (s["NUM_VARS"], s["NUM_CLAUSES"]) == (12, 40)
    assert s["H"] == 64 and s["INPUT"] == "corrupted" and s["MICROBATCH_BYTES"] == 1000000000


@pytest.mark.parametrize("override,needle", [
    ("MINIBATCH_SIZE=4", "MINIBATCH_SIZE"),  # unknown keys, at the top and in both sections
    ("training.LR=1", "training"),
    ("network.DEPTH=3", "DEPTH"),
    ("generation.COUNT=3", "COUNT"),
    ("EPOCHS=0", "EPOCHS"),
    ("EPOCHS=2.5", "EPOCHS"),
    ("BATCH_SIZE=0", "BATCH_SIZE"),
    ("LEARNING_RATE=0", "LEARNING_RATE"),
    ("TRAIN_RATIO=1.0", "TRAIN_RATIO"),
    ("TRAIN_RATIO=0", "TRAIN_RATIO"),
    ("INPUT=labels", "INPUT"),
    ("SOLVE_MISSING_EXPERTS=1", "SOLVE_MISSING_EXPERTS"),
    ("generation.REFRESH_EVERY=5", "REFRESH_EVERY"),
])
def test_unknown_or_inconsistent_keys_raise(override, needle):
    extra = ("generation.ENABLED=true",) if override.startswith("generation.REFRESH") else ()
    with pytest.raises(ValueError, match=needle):
        _settings(override, *extra)


def test_generation_needs_a_size():
    with pytest.raises(ValueError, match="NUM_VARS"):
        _settings("generation.ENABLED=true", "NUM_VARS=0")


def test_log_line_has_the_reference_fields_and_formats():
    from marlsat.runners.bc_runner import log_line

    tr = dict(loss=0.693147, var_acc=0.5, sol_acc=0.0)
    va = dict(loss=1.25, var_acc=0.71239, sol_acc=0.125)
    line = log_line(7, tr, va)
    assert line == ("Epoch 007 | Train Loss: 0.6931, Train Var-Acc: 0.5000, Train Sol-Acc: 0.0000 | "
                    "Val Loss: 1.2500, Val Var-Acc: 0.7124, Val Sol-Acc: 0.1250")
    m = re.fullmatch(r"Epoch (\d{3}) \| Train Loss: ([\d.]+), Train Var-Acc: ([\d.]+), Train Sol-Acc: ([\d.]+) \| "
                     r"Val Loss: ([\d.]+), Val Var-Acc: ([\d.]+), Val Sol-Acc: ([\d.]+)", line)
    assert m and m.group(1) == "007" and float(m.group(7)) == 0.125
    assert log_line(123, tr, va).startswith("Epoch 123 | ")


def test_split_is_seeded_and_keeps_both_sides():
    from marlsat.runners.bc_runner import split_instances

    a, b = split_instances(10, 0.8, 0)
    assert len(a) == 8 and len(b) == 2 and sorted(a.tolist() + b.tolist()) == list(range(10))
    a2, b2 = split_instances(10, 0.8, 0)
    assert a.tolist() == a2.tolist() and b.tolist() == b2.tolist()
    assert split_instances(10, 0.8, 1)[0].tolist() != a.tolist()
    with pytest.raises(ValueError, match="both splits"):
        split_instances(1, 0.8, 0)


def test_best_checkpoint_keeps_one(tmp_path):
    from marlsat.utils import checkpoints as ck

    d = str(tmp_path / "ck")
    for step in (2, 5):
        ck.prune_checkpoints(d, "best_", 0)
        ck.save_checkpoint(d, {"w": np.full(3, step, np.float32)}, step, "best_")
    assert os.listdir(d) == ["best_5"]
    assert np.array_equal(ck.restore_checkpoint(d, "best_", None)["w"], np.full(3, 5, np.float32))


def test_solve_pool_and_solver_defaults():
    from marlsat.solvers.walksat import solve_pool
    from marlsat.utils.sat_solver import build_parser, solve_directory

    p = inspect.signature(solve_pool).parameters["init_assignments"]
    assert p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    q = inspect.signature(solve_directory).parameters["init_model"]
    assert q.default is None and q.kind is inspect.Parameter.KEYWORD_ONLY
    a = build_parser().parse_args(["--cnf-dir", "a", "--sol-dir", "b"])
    assert a.init_model is None
    assert build_parser().parse_args(["--cnf-dir", "a", "--sol-dir", "b", "--init-model", "run"]).init_model == "run"
