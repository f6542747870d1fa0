"""Classical solvers on the device problem pool (no learned policy involved)."""
from .walksat import solve_pool, walksat, walksat_forms

__all__ = ["walksat", "solve_pool", "walksat_forms"]
