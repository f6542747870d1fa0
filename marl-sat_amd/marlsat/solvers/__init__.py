"""Solvers on the device problem pool: WalkSAT (no learned policy involved) and a trained policy with sampled
restarts and a WalkSAT finish."""
from .policy import SearchRecord, policy_search, solve_pool_with_policy
from .walksat import solve_pool, walksat, walksat_forms

__all__ = ["walksat", "solve_pool", "walksat_forms", "policy_search", "solve_pool_with_policy", "SearchRecord"]
