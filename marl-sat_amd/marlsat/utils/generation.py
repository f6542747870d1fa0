"""The ``generation`` section of MAPPO_CONFIG.yaml: pools drawn on the device instead of read from CNF_DATA_DIR.

Host-only (no device call, no torch): the section's parsing and validation, which train pool each update runs
on, and the keys the pools are drawn from.  runners/mappo_runner.py acts on it.

    generation:
      ENABLED: false       # true: CNF_DATA_DIR is not read
      NUM_TRAIN: 1024      # instances per train pool
      NUM_EVAL: 256        # instances of the eval pool (drawn once)
      REFRESH_EVERY: 0     # a new train pool every this many updates; 0 = never
      MAX_ATTEMPTS: 64     # redraws per instance that leaves a variable in no clause (msat_pool_generate)

Schedule: update u (0-based) trains on pool u // REFRESH_EVERY (pool 0 throughout when REFRESH_EVERY is 0), so
the runner draws pool e + 1 right before update (e + 1) * REFRESH_EVERY.  Keys: one generation key derived from
the run's seed; the eval pool is drawn at its counter 0 and train pool e at counter 1 + e, so every rank draws
the same pools and no pool repeats another.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List

from ..random import Key, PRNGKey, split

DEFAULTS = {"ENABLED": False, "NUM_TRAIN": 1024, "NUM_EVAL": 256, "REFRESH_EVERY": 0, "MAX_ATTEMPTS": 64}
MAX_ATTEMPTS_LIMIT = 255  # msat_pool_generate: the attempt shares a counter word with the block index


@dataclass(frozen=True)
class GenerationPlan:
    enabled: bool
    num_train: int
    num_eval: int
    refresh_every: int
    max_attempts: int

    def pool_of_update(self, update: int) -> int:
        """The train pool update `update` (0-based) runs on."""
        if update < 0:
            raise ValueError(f"update {update} < 0")
        return update // self.refresh_every if self.refresh_every > 0 else 0

    def schedule(self, num_updates: int) -> List[int]:
        """pool_of_update for updates 0 .. num_updates - 1."""
        return [self.pool_of_update(u) for u in range(num_updates)]

    def refresh_before(self, update: int) -> bool:
        """True when a new train pool is drawn right before this update."""
        return update > 0 and self.pool_of_update(update) != self.pool_of_update(update - 1)


def _int(section: Dict, name: str, lo: int, hi: int = None) -> int:
    v = section.get(name, DEFAULTS[name])
    if isinstance(v, bool) or not isinstance(v, int):
        raise ValueError(f"generation.{name} must be an integer, got {v!r}")
    if v < lo or (hi is not None and v > hi):
        raise ValueError(f"generation.{name}={v} must be " + (f"in [{lo}, {hi}]" if hi is not None else f">= {lo}"))
    return v


def parse_generation(config: Dict) -> GenerationPlan:
    """The validated ``generation`` section of a loaded config (absent: the defaults, disabled).  Unknown keys and
    bad values are refused with a message that names the key."""
    section = config.get("generation")
    if section is None:
        section = {}
    if not isinstance(section, dict):
        raise ValueError(f"generation must be a mapping, got {section!r}")
    unknown = sorted(set(section) - set(DEFAULTS))
    if unknown:
        raise ValueError(f"generation: unknown key(s) {unknown}; known: {sorted(DEFAULTS)}")
    enabled = section.get("ENABLED", DEFAULTS["ENABLED"])
    if not isinstance(enabled, bool):
        raise ValueError(f"generation.ENABLED must be true or false, got {enabled!r}")
    return GenerationPlan(enabled, _int(section, "NUM_TRAIN", 1), _int(section, "NUM_EVAL", 1),
                          _int(section, "REFRESH_EVERY", 0), _int(section, "MAX_ATTEMPTS", 1, MAX_ATTEMPTS_LIMIT))


def generation_key(seed: int) -> Key:
    """The run's generation key: the third child of PRNGKey(seed) (the runner's own chain takes the first two)."""
    return split(PRNGKey(seed), 3)[2]


def eval_pool_key(seed: int) -> Key:
    return generation_key(seed).fold(0)


def train_pool_key(seed: int, pool: int) -> Key:
    if pool < 0:
        raise ValueError(f"pool {pool} < 0")
    return generation_key(seed).fold(1 + pool)


def instance_name(num_vars: int, index: int) -> str:
    """File name of generated instance `index` (0-based): uf{V}-{index + 1:03d}.cnf, the generator tools' naming."""
    return f"uf{num_vars}-{index + 1:03d}.cnf"
