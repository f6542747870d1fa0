"""Solvers on the device problem pool: WalkSAT (no learned policy involved), a trained policy with sampled
restarts and a WalkSAT finish, and DPLL, the complete search that also proves unsatisfiability."""
from .dpll import decide_pool, dpll
from .policy import SearchRecord, policy_search, solve_pool_with_policy
from .walksat import solve_pool, walksat, walksat_forms

__all__ = ["walksat", "solve_pool", "walksat_forms", "policy_search", "solve_pool_with_policy", "SearchRecord",
           "dpll", "decide_pool"]
