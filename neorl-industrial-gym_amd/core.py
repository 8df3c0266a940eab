"""Boundary types of the hot path.

Field names and meanings follow the reference's `core/types.py` (SafetyConstraint :56-64,
SafetyMetrics :67-103, DatasetQuality :48-54) because downstream agents and harnesses read them;
the implementations are this package's own.  On the device a step's SafetyMetrics is two small
integers inside the per-lane flag word (include/nig.h NIG_FLAG_*); these classes are what the
Python surface rebuilds from it on demand.
"""
import enum
from dataclasses import dataclass, field
from typing import Any, Callable, Dict, Sequence, Tuple

import numpy as np


class DatasetQuality(enum.Enum):
    EXPERT = "expert"
    MEDIUM = "medium"
    MIXED = "mixed"
    RANDOM = "random"


@dataclass
class SafetyConstraint:
    """A named predicate over (state, action): check_fn returns True while the constraint holds.
    `penalty` is added to the reward of every violating step; a `critical` violation also ends
    the episode with an extra -1000 (reference step template, environments/base.py:179-198)."""
    name: str
    check_fn: Callable[[Any, Any], bool]
    penalty: float
    critical: bool = False
    description: str = ""


class BoxConstraint(SafetyConstraint):
    """A SafetyConstraint that is a box over rows of the step's pre-state and clipped action ("nig-limits-v1", include/nig.h):
    `bounds` maps ("state", r) / ("action", j) to a closed interval (lo, hi) of float32 bounds (+-inf allowed).  It holds while
    every listed row x has lo <= x and x <= hi; a NaN in a listed row violates, unlisted rows are never looked at.  Its
    check_fn is that statement in NumPy, so it works as any other constraint on the single env (and in the reference); being
    declarative, it is also what BatchedIndustrialEnv.add_safety_constraint evaluates on the device."""

    def __init__(self, name: str, bounds, penalty: float, critical: bool = False, description: str = ""):
        rows = {}
        for key, (lo, hi) in dict(bounds).items():
            kind, r = key
            if kind not in ("state", "action") or int(r) != r or int(r) < 0:
                raise ValueError(f"BoxConstraint row {key!r}: ('state', r) or ('action', j) with a non-negative index")
            lo, hi = np.float32(lo), np.float32(hi)
            if not lo <= hi:
                raise ValueError(f"BoxConstraint row {key!r}: lo > hi or a NaN bound")
            rows[(kind, int(r))] = (lo, hi)
        if not rows:
            raise ValueError("BoxConstraint needs at least one row")
        self.bounds = rows
        super().__init__(name=name, check_fn=self.holds, penalty=float(penalty), critical=bool(critical), description=description)

    def holds(self, state, action) -> bool:
        """True while the constraint holds (SafetyConstraint.check_fn): exact comparisons, a float64 element against the
        float32 bound widened by NumPy's promotion."""
        for (kind, r), (lo, hi) in self.bounds.items():
            x = (state if kind == "state" else action)[r]
            if not (lo <= x and x <= hi):
                return False
        return True

    def limit_rows(self, state_dim: int, action_dim: int):
        """(mask, {bit: (lo, hi)}) in nig_limit's numbering: bit r < S is state row r, bit S + j action row j."""
        mask, rows = 0, {}
        for (kind, r), b in self.bounds.items():
            if r >= (state_dim if kind == "state" else action_dim):
                raise ValueError(f"BoxConstraint '{self.name}': {kind} row {r} does not exist (S = {state_dim}, A = {action_dim})")
            bit = r if kind == "state" else state_dim + r
            mask |= 1 << bit
            rows[bit] = b
        return mask, rows


@dataclass
class SafetyMetrics:
    """Outcome of evaluating every constraint on one step's pre-state."""
    constraints_satisfied: int
    total_constraints: int
    violation_count: int
    critical_violations: int
    safety_score: float
    adaptive_threshold: float = 0.95
    confidence_interval: Tuple[float, float] = (0.0, 1.0)
    violation_severity: Dict[str, float] = field(default=None)

    def __post_init__(self):
        self.violation_severity = {} if self.violation_severity is None else self.violation_severity

    @property
    def satisfaction_rate(self) -> float:
        total = self.total_constraints
        return self.constraints_satisfied / total if total else 1.0

    @property
    def adaptive_safety_score(self) -> float:
        lo, hi = self.confidence_interval
        return max(self.safety_score - 0.1 * abs(hi - lo), 0.0)

    def update_adaptive_threshold(self, performance_history: Sequence[float]) -> None:
        recent = np.asarray(performance_history[-10:], dtype=float)
        if recent.size == 10:
            self.adaptive_threshold = float(np.clip(recent.mean() - 2.0 * recent.std(), 0.8, 0.99))


class Box:
    """Stand-in for gymnasium.spaces.Box when gymnasium is not installed: bounds, shape, dtype,
    `sample()` (from the global NumPy stream, like the envs) and `contains()`."""

    def __init__(self, low, high, shape=None, dtype=np.float32):
        self.dtype = np.dtype(dtype)
        self.shape = tuple(np.shape(low)) if shape is None else tuple(shape)
        self.low = np.broadcast_to(np.asarray(low, dtype=self.dtype), self.shape).copy()
        self.high = np.broadcast_to(np.asarray(high, dtype=self.dtype), self.shape).copy()
        self._lo = np.where(np.isfinite(self.low), self.low, -1e6).astype(np.float64)
        self._hi = np.where(np.isfinite(self.high), self.high, 1e6).astype(np.float64)

    def sample(self):
        return np.random.uniform(self._lo, self._hi).astype(self.dtype)

    def contains(self, x) -> bool:
        x = np.asarray(x)
        return x.shape == self.shape and bool((x >= self.low).all() and (x <= self.high).all())

    def __repr__(self):
        return f"Box({self.low.min()}, {self.high.max()}, {self.shape}, {self.dtype})"


def make_box(low, high, shape, dtype=np.float32):
    """gymnasium's Box when available, the stand-in otherwise."""
    try:
        import gymnasium
        return gymnasium.spaces.Box(low=low, high=high, shape=shape, dtype=dtype)
    except Exception:
        return Box(low, high, shape, dtype)
