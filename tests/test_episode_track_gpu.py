"""GPU: msat_episode_track (the bookkeeping of a greedy evaluation without auto-reset, single_rl_runner.py:218-229)
against the NumPy loop of tests/single_oracle.py: returns bitwise (fp32 sums in step order), lengths, solved flags
and finished flags exact; an env that has finished is not changed by later steps, whatever they carry."""
import numpy as np
import pytest
import torch

import single_oracle as so

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("B", (1, 3, 257))  # one lane; part of a wave; a second workgroup with one env
def test_episode_track_matches_numpy_loop(B):
    from marlsat import _lib

    T = 6
    rng = np.random.default_rng(B)
    rew = rng.standard_normal((T, B)).astype(np.float32)
    done = (rng.random((T, B)) < 0.3).astype(np.uint8)  # several dones per env: only the first counts
    done[:, 0] = 0  # an env that never finishes
    if B > 1:
        done[0, 1] = 1  # one that finishes at the first step
    solved = (rng.random((T, B)) < 0.5).astype(np.uint8)  # solved flags also where done is 0
    ret = torch.zeros(B, device="cuda")
    ln = torch.zeros(B, dtype=torch.int32, device="cuda")
    sv = torch.zeros(B, dtype=torch.uint8, device="cuda")
    fin = torch.zeros(B, dtype=torch.uint8, device="cuda")
    for t in range(T):
        r, d, s = (torch.from_numpy(a[t].copy()).cuda() for a in (rew, done, solved))
        _lib.check(_lib.lib.msat_episode_track(B, t, r.data_ptr(), d.data_ptr(), s.data_ptr(), ret.data_ptr(),
                                               ln.data_ptr(), sv.data_ptr(), fin.data_ptr(), _lib.stream_ptr()),
                   "msat_episode_track")
        torch.cuda.synchronize()
        want = so.episode_track(rew[:t + 1], done[:t + 1], solved[:t + 1])
        got = (ret.cpu().numpy(), ln.cpu().numpy(), sv.cpu().numpy(), fin.cpu().numpy())
        assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)), t
        for g, w in zip(got[1:], want[1:]):
            assert np.array_equal(g, w), t
    assert fin.cpu().numpy()[0] == 0 and ln.cpu().numpy()[0] == 0


def test_episode_track_argument_errors():
    from marlsat import _lib

    L = _lib.lib
    f = torch.zeros(4, device="cuda")
    p, st = f.data_ptr(), _lib.stream_ptr()
    assert L.msat_episode_track(0, 0, None, None, None, None, None, None, None, st) == 0
    assert L.msat_episode_track(-1, 0, p, p, p, p, p, p, p, st) == -1 and b"B -1" in L.msat_last_error()
    assert L.msat_episode_track(1, -1, p, p, p, p, p, p, p, st) == -1 and b"step index" in L.msat_last_error()
    for k in range(7):
        a = [p] * 7
        a[k] = None
        assert L.msat_episode_track(1, 0, *a, st) == -1 and b"NULL" in L.msat_last_error()
