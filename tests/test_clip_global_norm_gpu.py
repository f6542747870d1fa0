"""GPU: msat_clip_global_norm (optax.clip_by_global_norm, single_rl_learner.py:52-60) and msat_standardize_pop
(single_rl_learner.py:142) against float64 (tests/single_oracle.py).

Clip: a norm below max_norm leaves the gradient bitwise as it was; otherwise every element lies within
2^-23 * |exact| of g * max_norm / norm (one rounding of the scale, one of the product); norm_out within 2^-23
relative.  'Around max_norm' cases take max_norm itself from the float32 neighbours of the gradient's float64 norm,
so the decision is made within one ulp of the edge.  Standardise: within 2^-22 * max|x - mean| / (std + 1e-8)."""
import numpy as np
import pytest
import torch

import single_oracle as so

pytestmark = pytest.mark.gpu

NS = (0, 1, 3, 4, 1023, 1025, 300001)  # empty; below / at a float4; either side of four workgroups' 1024; 1024-block cap
ULP = 2.0 ** -23
GUARD = -3.5


def _grad(n, seed=0, scale=1.0):
    return (scale * np.random.default_rng(seed + n).standard_normal(n)).astype(np.float32)


def _clip(g, max_norm):
    """-> (clipped gradient, norm_out), with the gradient at an odd float offset between guard floats."""
    from marlsat import _lib

    n = g.size
    buf = torch.full((n + 8,), GUARD, device="cuda")
    buf[3:3 + n] = torch.from_numpy(g).cuda()
    ws = torch.full((int(_lib.lib.msat_clip_global_norm_workspace_doubles(n)) + 1,), -1.0, dtype=torch.float64,
                    device="cuda")
    norm = torch.full((3,), GUARD, device="cuda")
    _lib.check(_lib.lib.msat_clip_global_norm(buf[3:].data_ptr() if n else buf.data_ptr(), n, float(max_norm),
                                              ws.data_ptr(), norm[1:].data_ptr(), _lib.stream_ptr()),
               "msat_clip_global_norm")
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:3] == GUARD).all() and (h[3 + n:] == GUARD).all()
    assert float(ws[-1]) == -1.0 and float(norm[0]) == GUARD and float(norm[2]) == GUARD
    return h[3:3 + n].copy(), float(norm[1])


def _check(g, max_norm, what):
    got, norm = _clip(g, max_norm)
    ref, rnorm, touched = so.clip_global_norm(g, max_norm)
    print(f"clip n={g.size} {what}: norm {rnorm:.9g} max_norm {float(np.float32(max_norm)):.9g} clipped {touched}")
    assert abs(norm - rnorm) <= ULP * rnorm
    if not touched:
        assert np.array_equal(got.view(np.int32), g.view(np.int32))
    else:
        err = np.abs(got.astype(np.float64) - ref)
        assert (err <= ULP * np.abs(ref)).all(), (what, (err / np.maximum(np.abs(ref), 1e-300)).max())
    return got, touched


@pytest.mark.parametrize("n", NS)
def test_clip_below_above_and_around_the_norm(n):
    g = _grad(n)
    norm = so.global_norm(g)
    if n == 0:
        got, nrm = _clip(g, 1.0)  # no launch: nothing is written, norm_out included
        assert got.size == 0 and nrm == GUARD
        return
    _, touched = _check(g, 2.0 * norm, "below")
    assert not touched
    _, touched = _check(g, norm / 100.0, "far above")
    assert touched
    f = np.float32(norm)
    seen = set()
    for m in (np.nextafter(f, np.float32(0)), f, np.nextafter(f, np.float32(np.inf))):
        # the decision is the float64 comparison norm < max_norm; at float32(norm) == norm exactly the scale is 1
        _, touched = _check(g, m, "within one ulp")
        seen.add(touched)
    assert seen == {False, True}
    a, _ = _clip(g, norm / 3.0)
    b, _ = _clip(g, norm / 3.0)
    assert np.array_equal(a.view(np.int32), b.view(np.int32))  # fixed reduction order


def test_clip_large_values_zero_gradient_and_nan():
    from marlsat import _lib

    g = _grad(1025, seed=7, scale=1e25)  # the fp32 sum of squares would overflow
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.sum(g.astype(np.float32) ** 2, dtype=np.float32))
    _, touched = _check(g, 1.0, "values near 1e25")
    assert touched
    z = np.zeros(1025, np.float32)
    got, norm = _clip(z, 0.5)
    assert norm == 0.0 and np.array_equal(got.view(np.int32), z.view(np.int32))
    # a NaN element: NaN norm, NaN gradient, and the Adam step that follows reports itself
    g = _grad(1025, seed=9)
    g[77] = np.float32("nan")
    got, norm = _clip(g, 0.5)
    assert np.isnan(norm) and np.isnan(got).all()
    p = torch.ones(1025, device="cuda")
    gd, m, v = torch.from_numpy(got).cuda(), torch.zeros(1025, device="cuda"), torch.zeros(1025, device="cuda")
    first_bad = torch.full((1,), 2 ** 31 - 1, dtype=torch.int32, device="cuda")
    _lib.check(_lib.lib.msat_adam_checked(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), 1025, 1e-3, 0.9,
                                          0.999, 1e-5, 4, 1.0, first_bad.data_ptr(), _lib.stream_ptr()),
               "msat_adam_checked")
    assert int(first_bad.item()) == 4


def test_clip_argument_errors():
    from marlsat import _lib

    L = _lib.lib
    f = torch.zeros(8, device="cuda")
    w = torch.zeros(8, dtype=torch.float64, device="cuda")
    st = _lib.stream_ptr()
    assert L.msat_clip_global_norm_workspace_doubles(0) >= 1
    assert L.msat_clip_global_norm_workspace_doubles(300001) >= 1
    for mn in (0.0, -1.0, float("nan"), float("inf")):
        assert L.msat_clip_global_norm(f.data_ptr(), 8, mn, w.data_ptr(), f.data_ptr(), st) == -1
        assert "max_norm" in L.msat_last_error().decode()
    assert L.msat_clip_global_norm(None, 8, 1.0, w.data_ptr(), f.data_ptr(), st) == -1
    assert L.msat_clip_global_norm(f.data_ptr(), 8, 1.0, None, f.data_ptr(), st) == -1
    assert L.msat_clip_global_norm(f.data_ptr(), 8, 1.0, w.data_ptr(), None, st) == -1
    assert "NULL" in L.msat_last_error().decode()
    assert L.msat_standardize_pop(None, 8, w.data_ptr(), st) == -1
    assert L.msat_standardize_pop(f.data_ptr(), 8, None, st) == -1
    assert L.msat_standardize_pop(None, 0, None, st) == 0


def _standardize(x):
    from marlsat import _lib

    n = x.size
    buf = torch.full((n + 8,), GUARD, device="cuda")
    buf[3:3 + n] = torch.from_numpy(x).cuda()
    mom = torch.zeros(2, dtype=torch.float64, device="cuda")
    ws = torch.zeros(2 * 1024, dtype=torch.float64, device="cuda")
    st = _lib.stream_ptr()
    _lib.check(_lib.lib.msat_moments(buf[3:].data_ptr(), n, mom.data_ptr(), ws.data_ptr(), st), "msat_moments")
    _lib.check(_lib.lib.msat_standardize_pop(buf[3:].data_ptr(), n, mom.data_ptr(), st), "msat_standardize_pop")
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert (h[:3] == GUARD).all() and (h[3 + n:] == GUARD).all()
    return h[3:3 + n].copy()


@pytest.mark.parametrize("n", (1, 2, 257))
def test_standardize_pop_matches_float64(n):
    x = (0.3 + 1.7 * np.random.default_rng(40 + n).standard_normal(n)).astype(np.float32)
    got = _standardize(x)
    ref = so.standardize_pop(x)
    bar = 2.0 ** -22 * np.abs(ref).max()
    print(f"standardize_pop n={n}: max err {np.abs(got - ref).max():.3g} (bar {bar:.3g})")
    assert np.abs(got.astype(np.float64) - ref).max() <= bar
    if n == 1:
        assert got[0] == 0.0
    for c in (0.1, -3.0, 1e-30, 12345.678):  # a constant vector: all zeros, whatever the variance rounds to
        z = _standardize(np.full(n, c, np.float32))
        assert (z == 0.0).all(), (n, c, z[:4])
