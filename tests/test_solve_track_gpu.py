"""GPU: the policy solver's search record (msat_solve_track_init / msat_solve_track / msat_solve_pick,
include/marlsat.h) against a NumPy restatement written here.  No env and no network: synthetic sequences of
(assign, solved, num_unsat) over 12 steps at B = 7 rows, V in {1, 20, 64, 65, 130} (less than a wave, a full wave,
a second and a third trip of the lane loops; B = 7 takes a second workgroup).

Rows: 0 already satisfied at init; 1 solves at step 1; 2 never solves and repeats its num_unsat (only a strict
improvement moves the record); 3 solves at step 5 and "unsolves" afterwards (frozen); 4 never changes its
assignment (flips stay 0); 5 and 6 random, 6 solving at the last step.
"""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, STEPS = 7, 12
FIELDS = ("prev_x", "best_x", "best_unsat", "best_step", "first_solve", "flips", "unsolved")


def _sequence(V, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 2, (STEPS + 1, B, V)).astype(np.uint8)
    nun = rng.integers(1, 9, (STEPS + 1, B)).astype(np.int32)
    solved = np.zeros((STEPS + 1, B), dtype=np.uint8)
    nun[0, 0] = 0                       # row 0: satisfied by the reset assignment
    solved[1, 1], nun[1, 1] = 1, 0      # row 1: solves at step 1
    nun[:, 2] = [5, 5, 4, 4, 6, 4, 3, 3, 7, 3, 5, 3, 3]  # row 2: ties after every improvement, never solved
    solved[5, 3], nun[5, 3] = 1, 0      # row 3: solves at step 5 ...
    nun[6:, 3] = 2                      # ... and the env walks on: lower counts than before must not register
    nun[:5, 3] = 4
    x[:, 4] = x[0, 4]                   # row 4: the assignment never changes
    solved[STEPS, 6], nun[STEPS, 6] = 1, 0
    return x, solved, nun


def _ref_init(x, nun):
    return {"prev_x": x.copy(), "best_x": x.copy(), "best_unsat": nun.copy(), "best_step": np.zeros(B, np.int32),
            "first_solve": np.where(nun == 0, 0, -1).astype(np.int32), "flips": np.zeros(B, np.int32),
            "unsolved": np.array([(nun != 0).sum()], np.int32)}


def _ref_track(s, step, x, solved, nun):
    for r in range(B):
        if s["first_solve"][r] >= 0:
            continue
        s["flips"][r] += int((s["prev_x"][r] ^ x[r]).sum())
        s["prev_x"][r] = x[r]
        if solved[r]:
            s["first_solve"][r], s["best_step"][r], s["best_unsat"][r] = step, step, 0
            s["best_x"][r] = x[r]
        elif nun[r] < s["best_unsat"][r]:
            s["best_unsat"][r], s["best_step"][r] = nun[r], step
            s["best_x"][r] = x[r]
    s["unsolved"][0] = (s["first_solve"] < 0).sum()


class _Dev:
    def __init__(self, V, rows=B):
        z = lambda shape, dt: torch.full(shape, 0x55, dtype=dt, device="cuda")  # the calls own every word
        self.t = {"prev_x": z((rows, V), torch.uint8), "best_x": z((rows, V), torch.uint8),
                  "best_unsat": z((rows,), torch.int32), "best_step": z((rows,), torch.int32),
                  "first_solve": z((rows,), torch.int32), "flips": z((rows,), torch.int32),
                  "unsolved": z((1,), torch.int32)}

    def c(self):
        from marlsat import _lib

        return _lib.SolveStateC(*(self.t[k].data_ptr() for k in FIELDS))

    def host(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.t.items()}


def _run(V, x, solved, nun, check=None):
    from marlsat import _lib

    L, d = _lib.lib, _Dev(V)
    dx, ds, dn = torch.from_numpy(x).cuda(), torch.from_numpy(solved).cuda(), torch.from_numpy(nun).cuda()
    c = d.c()
    _lib.check(L.msat_solve_track_init(B, V, dx[0].data_ptr(), dn[0].data_ptr(), ctypes.byref(c), _lib.stream_ptr()),
               "init")
    snaps = [d.host()]
    if check:
        check(0, snaps[-1])
    for t in range(1, STEPS + 1):
        _lib.check(L.msat_solve_track(B, V, t, dx[t].data_ptr(), ds[t].data_ptr(), dn[t].data_ptr(), ctypes.byref(c),
                                      _lib.stream_ptr()), "track")
        snaps.append(d.host())
        if check:
            check(t, snaps[-1])
    return snaps, d


@pytest.mark.parametrize("V", [1, 20, 64, 65, 130])
def test_track_matches_numpy_after_every_call(V):
    x, solved, nun = _sequence(V, V)
    ref = _ref_init(x[0], nun[0])
    want = [{k: v.copy() for k, v in ref.items()}]
    for t in range(1, STEPS + 1):
        _ref_track(ref, t, x[t], solved[t], nun[t])
        want.append({k: v.copy() for k, v in ref.items()})

    def check(t, got):
        for k in FIELDS:
            np.testing.assert_array_equal(got[k], want[t][k], err_msg=f"V={V} call {t} field {k}")

    snaps, _ = _run(V, x, solved, nun, check)
    end = snaps[-1]
    # the rows are what the docstring says they are
    assert end["first_solve"].tolist()[:5] == [0, 1, -1, 5, -1] and end["first_solve"][6] == STEPS
    assert (end["best_unsat"][2], end["best_step"][2]) == (3, 6)  # the first of the equal best counts
    assert (end["best_unsat"][3], end["best_step"][3]) == (0, 5) and np.array_equal(end["best_x"][3], x[5, 3])
    assert end["flips"][0] == 0 and end["flips"][4] == 0
    assert end["flips"][3] == int((x[:5, 3] ^ x[1:6, 3]).sum())  # up to the solve, not beyond
    assert end["unsolved"][0] == (end["first_solve"] < 0).sum() >= 2
    # a second identical run leaves identical words
    again, _ = _run(V, x, solved, nun)
    for a, b in zip(snaps, again):
        for k in FIELDS:
            assert a[k].tobytes() == b[k].tobytes(), k


def test_track_empty_batch_writes_only_the_count():
    from marlsat import _lib

    d = _Dev(4, rows=1)
    c = d.c()
    _lib.check(_lib.lib.msat_solve_track_init(0, 4, None, None, ctypes.byref(c), _lib.stream_ptr()), "init")
    h = d.host()
    assert h["unsolved"][0] == 0 and h["first_solve"][0] == 0x55


def _pick_ref(fs, fl, bu, bs, tries):
    out = []
    for p in range(len(fs) // tries):
        rows = range(p * tries, (p + 1) * tries)
        key = lambda r: (0, fs[r], fl[r], r) if fs[r] >= 0 else (1, bu[r], bs[r], r)
        out.append(min(rows, key=key))
    return np.array(out)


@pytest.mark.parametrize("V", [1, 65, 130])
@pytest.mark.parametrize("tries", [1, 3, 8, 70])
def test_pick_order_with_ties_at_every_level(tries, V):
    """P = 5 instances: 0 all unsolved, tie in best_unsat broken by best_step; 1 all unsolved and all equal (lowest
    try); 2 one solved among unsolved with lower counts (solved wins); 3 several solved, tie in first_solve broken
    by flips; 4 several solved, full tie (lowest try).  The last rows carry the winners where tries allows, so
    the lowest-try rule is not met by accident.  tries = 70: a second trip of the lane loop."""
    from marlsat import _lib

    P = 5
    rng = np.random.default_rng(tries * 100 + V)
    n = P * tries
    fs = np.full(n, -1, np.int32)
    fl = rng.integers(5, 50, n).astype(np.int32)
    bu = rng.integers(3, 9, n).astype(np.int32)
    bs = rng.integers(1, 12, n).astype(np.int32)
    last = tries - 1
    bu[0:tries] = 4
    bs[0:tries] = 7
    bs[0 * tries + last] = 2                     # instance 0: same best_unsat, the last try reached it first
    bu[tries:2 * tries], bs[tries:2 * tries] = 3, 5  # instance 1: all equal
    bu[2 * tries:3 * tries] = 1
    fs[2 * tries + last], bu[2 * tries + last], fl[2 * tries + last] = 9, 0, 49  # instance 2: the only solved try
    fs[3 * tries:4 * tries], bu[3 * tries:4 * tries] = 6, 0
    fl[3 * tries:4 * tries] = 20
    fl[3 * tries + last] = 11                    # instance 3: same steps, the last try flipped least
    if tries > 1:
        fs[3 * tries] = 8                        # ... and a later solve with fewer flips still loses
        fl[3 * tries] = 1
    fs[4 * tries:], bu[4 * tries:], fl[4 * tries:] = 4, 0, 13  # instance 4: full tie
    bs[fs >= 0] = fs[fs >= 0]
    bx = rng.integers(0, 2, (n, V)).astype(np.uint8)
    d = _Dev(V, rows=n)
    for k, a in (("first_solve", fs), ("flips", fl), ("best_unsat", bu), ("best_step", bs), ("best_x", bx)):
        d.t[k].copy_(torch.from_numpy(a))
    o = {k: torch.full((P,), -9, dtype=torch.int32, device="cuda")
         for k in ("try", "steps", "flips", "best_unsat", "best_step")}
    o_solved = torch.full((P,), 9, dtype=torch.uint8, device="cuda")
    o_x = torch.full((P, V), 9, dtype=torch.uint8, device="cuda")
    c = d.c()
    _lib.check(_lib.lib.msat_solve_pick(P, tries, V, ctypes.byref(c), o_solved.data_ptr(), o["try"].data_ptr(),
                                        o["steps"].data_ptr(), o["flips"].data_ptr(), o["best_unsat"].data_ptr(),
                                        o["best_step"].data_ptr(), o_x.data_ptr(), _lib.stream_ptr()), "pick")
    torch.cuda.synchronize()
    win = _pick_ref(fs, fl, bu, bs, tries)
    want_try = win - np.arange(P) * tries
    np.testing.assert_array_equal(o["try"].cpu().numpy(), want_try)
    assert want_try.tolist() == [last, 0, last, last, 0]
    np.testing.assert_array_equal(o_solved.cpu().numpy(), (fs[win] >= 0).astype(np.uint8))
    np.testing.assert_array_equal(o["steps"].cpu().numpy(), fs[win])
    np.testing.assert_array_equal(o["flips"].cpu().numpy(), fl[win])
    np.testing.assert_array_equal(o["best_unsat"].cpu().numpy(), bu[win])
    np.testing.assert_array_equal(o["best_step"].cpu().numpy(), bs[win])
    np.testing.assert_array_equal(o_x.cpu().numpy(), bx[win])
