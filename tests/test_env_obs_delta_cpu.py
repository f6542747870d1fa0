"""Host-side argument checks of msat_env_step_delta / msat_obs_shadow_words (no launch, no GPU)."""
import ctypes


def _desc(**kw):
    from marlsat import _lib

    d = dict(num_envs=8, num_vars=50, num_clauses=218, clause_width=3, num_agents=5, max_vars_per_agent=10,
             max_steps=16, action_mode=0, reward_mode=0, obs_dtype=0, num_problems=4, r_clause=0.02, r_sat=1.0,
             gamma=0.99)
    d.update(kw)
    return _lib.EnvDesc(**d)


def _step(desc, obs, shadow, group):
    from marlsat import _lib

    # every pointer is a dummy: the calls below are refused before anything is dereferenced or launched
    return _lib.lib.msat_env_step_delta(ctypes.byref(desc), None, None, None, 1, None, None, 0, 0, None, obs, shadow,
                                        group, None)


def test_shadow_words():
    from marlsat import _lib

    L = _lib.lib
    assert L.msat_obs_shadow_words(ctypes.byref(_desc())) == 8 * (1 + 2 + 7)  # idx, ceil(50/32), ceil(218/32)
    assert L.msat_obs_shadow_words(ctypes.byref(_desc(num_envs=3, num_vars=64, num_clauses=64,
                                                      num_agents=8, max_vars_per_agent=8))) == 3 * (1 + 2 + 2)
    assert L.msat_obs_shadow_words(ctypes.byref(_desc(num_envs=0))) == 0
    assert L.msat_obs_shadow_words(ctypes.byref(_desc(num_vars=0))) == 0  # invalid desc
    assert L.msat_obs_shadow_words(None) == 0


def test_step_delta_rejects_bad_arguments():
    from marlsat import _lib

    L = _lib.lib
    for g in (-16, 1, 8, 32, 48, 256):
        assert _step(_desc(), 0x1000, 0x2000, g) == -1, g
        assert b"delta_group_bytes" in L.msat_last_error()
    assert _step(_desc(), None, 0x2000, 64) == -1
    assert b"obs_shadow given with NULL obs" in L.msat_last_error()
    assert _step(_desc(), 0x1000, 0x2002, 64) == -1
    assert b"4-byte aligned" in L.msat_last_error()
    assert _step(_desc(num_vars=0), 0x1000, 0x2000, 64) == -1  # the desc is checked first
    # valid delta arguments get as far as the state check (NULL state), still without a launch
    for g in (0, 16, 64, 128):
        assert _step(_desc(), 0x1000, 0x2000, g) == -1
        assert b"state is NULL" in L.msat_last_error()
    assert _step(_desc(num_envs=0), 0x1000, 0x2000, 64) == 0  # an empty batch is a no-op
