"""GPU: msat_bc_corrupt (corrupted expert copies, Floyd's sample of distinct variables from the Philox stream)
bit-exact against a host restatement of the draw built on oracle.rng.philox4x32_10."""
import numpy as np
import pytest
import torch

from oracle.rng import philox4x32_10

pytestmark = pytest.mark.gpu

S = 37
SEED, COUNTER = 0x1234_5678_9ABC_DEF1, (7 << 32) + 5  # both words of the key and of the counter in use


def host_corrupt(src, src_row, V, level, seed, counter):
    """include/marlsat.h, msat_bc_corrupt: for i < n = min(level, V): j = V - n + i, t = (q * (j + 1)) >> 32 with
    q = philox((counter lo, counter hi, s, i), seed lo, seed hi).x; flip t unless already flipped, then j."""
    n_src = src.shape[0]
    rows = np.clip(src_row, 0, n_src - 1)
    out = src[rows].copy()
    n = min(level, V)
    k0, k1 = np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32)
    c0, c1 = np.uint32(counter & 0xFFFFFFFF), np.uint32(counter >> 32)
    s = np.arange(len(rows), dtype=np.uint32)
    for i in range(n):
        j = V - n + i
        q = philox4x32_10(c0, c1, s, np.uint32(i), k0, k1)[0]
        t = ((q.astype(np.uint64) * np.uint64(j + 1)) >> np.uint64(32)).astype(np.int64)
        taken = out[s, t] != src[rows, t]
        pick = np.where(taken, j, t)
        out[s, pick] ^= 1
    return out


def device_corrupt(src, src_row, V, level, seed=SEED, counter=COUNTER, guard=0):
    from marlsat import _lib

    src_d = torch.from_numpy(src).cuda()
    row_d = torch.from_numpy(src_row.astype(np.int32)).cuda()
    n = len(src_row)
    out = torch.full((n + guard, V), 0xAB, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib.msat_bc_corrupt(src_d.data_ptr(), src.shape[0], row_d.data_ptr(), n, V, level, seed, counter,
                                        out.data_ptr(), _lib.stream_ptr()), "msat_bc_corrupt")
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _experts(V, n_src=5, seed=0):
    return np.random.default_rng(seed + V).integers(0, 2, (n_src, V)).astype(np.uint8)


@pytest.mark.parametrize("V", [1, 7, 64, 65, 200])
def test_corrupt_is_the_host_floyd_draw(V):
    src = _experts(V)
    rows = np.arange(S) % src.shape[0]
    prev = None
    for level in (0, 1, 3, V, V + 5):
        got = device_corrupt(src, rows, V, level, guard=2)
        assert (got[S:] == 0xAB).all()  # nothing written past the S rows
        got = got[:S]
        assert np.array_equal(got, host_corrupt(src, rows, V, level, SEED, COUNTER)), (V, level)
        assert ((got != src[rows]).sum(1) == min(level, V)).all(), (V, level)
        assert set(np.unique(got)) <= {0, 1}
        if level == 0:
            assert np.array_equal(got, src[rows])
        prev = got
    assert np.array_equal(prev, 1 - src[rows])  # level >= V flips every variable


def test_counter_and_seed_select_the_stream():
    V, level = 64, 3
    src = _experts(V)
    rows = np.arange(S) % src.shape[0]
    a = device_corrupt(src, rows, V, level)
    assert np.array_equal(a, device_corrupt(src, rows, V, level))  # reproducible
    for kw in (dict(counter=COUNTER + 1), dict(counter=COUNTER + (1 << 32)), dict(seed=SEED + 1),
               dict(seed=SEED + (1 << 32))):
        b = device_corrupt(src, rows, V, level, **kw)
        assert np.array_equal(b, host_corrupt(src, rows, V, level, kw.get("seed", SEED), kw.get("counter", COUNTER)))
        assert (a != b).any(1).sum() > S // 2, kw  # 3 of 64 variables: two streams rarely agree on a row
    # samples of one expert differ from each other
    same = device_corrupt(src, np.zeros(S, np.int64), V, level)
    assert len({r.tobytes() for r in same}) > S // 2


def test_out_of_range_source_row_is_clamped():
    V, level = 7, 1
    src = _experts(V, n_src=3)
    rows = np.array([-5, -1, 0, 2, 3, 1000, 2 ** 31 - 1, -2 ** 31], dtype=np.int64)
    got = device_corrupt(src, rows, V, level, guard=1)
    assert (got[len(rows):] == 0xAB).all()
    got = got[:len(rows)]
    assert np.array_equal(got, host_corrupt(src, rows, V, level, SEED, COUNTER))
    clamped = np.clip(rows, 0, 2)
    assert ((got != src[clamped]).sum(1) == 1).all()


def test_corrupt_device_wrapper_and_preprocess():
    """runners.behavioral_cloning.corrupt_device: expert e's copies are rows e * num_samples + k, replayable from
    the key; preprocess(device_corrupt=True) labels exactly those assignments."""
    from marlsat import SATEnv
    from marlsat.random import PRNGKey
    from marlsat.runners.behavioral_cloning import compute_joint_labels, corrupt_device, preprocess
    from marlsat.utils.generate_cnf_dataset import generate_sat_clauses, generate_sat_solution

    V, C, n_exp, per, level = 20, 91, 4, 5, 3
    sols = np.stack([generate_sat_solution(V, s) for s in range(n_exp)])
    key = PRNGKey(11)
    x = corrupt_device(sols, per, level, key).cpu().numpy()
    rows = np.repeat(np.arange(n_exp), per)
    assert np.array_equal(x, host_corrupt(sols.astype(np.uint8), rows, V, level, key.seed, key.counter))
    env = SATEnv(V, C, max_steps=4, vars_per_agent=10)
    experts = [{"name": f"p{s}", "problem_clauses": generate_sat_clauses(V, C, seed=s), "expert_solution": sols[s]}
               for s in range(n_exp)]
    cfg = {"bc_training": {"NUM_SAMPLES_PER_EXPERT": per, "CORRUPTION_LEVEL": level}}
    data = preprocess(experts, env, cfg, seed=11, device_corrupt=True)
    assert np.array_equal(data["assignments"], x) and np.array_equal(data["problem_idx"], rows)
    pool = env.make_pool(data["clauses"])
    assert np.array_equal(data["labels"], compute_joint_labels(env, pool, rows, x).cpu().numpy())
    host = preprocess(experts, env, cfg, seed=11)  # the default path is the numpy one, unchanged
    assert ((host["assignments"] != sols[rows]).sum(1) == level).all()
