"""Parameter sweeps inside one replica ensemble: the specification.

A ``Sweep`` is an ordered list of G parameter points over seven named axes
(``AXES``): the arrival rate, amplitude and period of either job type, and the
power cap.  An axis a sweep does not name takes the engine's base value (the
``ArrivalProcess`` arguments and ``power_cap=``).  Replicas map to groups by
GLOBAL replica id, ``group = gid // (replicas // G)``, so a group is a
contiguous run of replicas with its own Philox keys: bit for bit a shard of a
uniform run with that point's parameters (parallel/sharding.py).

Plain Python and numpy: nothing here needs a torch device.  The engine turns
``table()`` into the per-replica state tensors ``sw_arr`` / ``sw_cap``
(engine/state.py), which the arrival-ring generator and the cap_greedy kernel
read (ops/csrc/hip/arrival_ring.hpp, replica_engine.hip).
"""
import itertools
import math
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

AXES = ("inf_rate", "inf_amp", "inf_period",
        "trn_rate", "trn_amp", "trn_period", "power_cap")
# sw_arr[r, jtype, k]: k over (rate, amp, period)
ARR_FIELDS = ("rate", "amp", "period")


@dataclass(frozen=True)
class SweepBase:
    """The engine's own parameter point: what an axis not swept takes."""
    inf_rate: float
    inf_amp: float
    inf_period: float
    trn_rate: float
    trn_amp: float
    trn_period: float
    power_cap: float = 0.0
    inf_mode: str = "poisson"
    trn_mode: str = "poisson"

    @classmethod
    def of(cls, arrival_inf, arrival_trn, power_cap: float = 0.0):
        return cls(float(arrival_inf.rate), float(arrival_inf.amp),
                   float(arrival_inf.period), float(arrival_trn.rate),
                   float(arrival_trn.amp), float(arrival_trn.period),
                   float(power_cap), arrival_inf.mode, arrival_trn.mode)


def _check_value(axis: str, v, where: str) -> float:
    try:
        x = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"sweep {where}: {axis} = {v!r} is not a number")
    if not math.isfinite(x):
        raise ValueError(f"sweep {where}: {axis} = {x} is not finite")
    if axis.endswith("_rate") and x < 0:
        raise ValueError(f"sweep {where}: {axis} = {x}, a rate must be >= 0")
    if axis.endswith("_period") and x <= 0:
        raise ValueError(f"sweep {where}: {axis} = {x}, a period must be > 0")
    if axis == "power_cap" and x < 0:
        raise ValueError(f"sweep {where}: power_cap = {x} must be >= 0 "
                         "(0 = no control in that group)")
    return x


class Sweep:
    """G ordered points; build with ``Sweep.grid`` or ``Sweep.points``."""

    def __init__(self, axes: Sequence[str], rows: Sequence[Dict[str, float]]):
        self.axes: Tuple[str, ...] = tuple(axes)
        self._rows: List[Dict[str, float]] = [dict(r) for r in rows]
        if not self._rows:
            raise ValueError("a sweep needs at least one point")

    # ---------------- constructors ----------------
    @classmethod
    def grid(cls, **axes) -> "Sweep":
        """Cartesian product of the given axes, each a sequence of values;
        the last-named axis varies fastest."""
        if not axes:
            raise ValueError("Sweep.grid needs at least one axis")
        names = list(axes)
        values = []
        for name in names:
            if name not in AXES:
                raise ValueError(f"unknown sweep axis {name!r}; the axes are "
                                 f"{', '.join(AXES)}")
            vals = list(np.atleast_1d(np.asarray(axes[name], dtype=object)))
            if not vals:
                raise ValueError(f"sweep axis {name} has no values")
            values.append([_check_value(name, v, f"axis {name}")
                           for v in vals])
        rows = [dict(zip(names, combo))
                for combo in itertools.product(*values)]
        return cls(names, rows)

    @classmethod
    def points(cls, pts: Sequence[Dict[str, float]]) -> "Sweep":
        """An explicit list of points, each a dict over some of the axes."""
        pts = list(pts)
        names: List[str] = []
        rows = []
        for i, p in enumerate(pts):
            row = {}
            for name, v in dict(p).items():
                if name not in AXES:
                    raise ValueError(f"unknown sweep axis {name!r} in point "
                                     f"{i}; the axes are {', '.join(AXES)}")
                row[name] = _check_value(name, v, f"point {i}")
                if name not in names:
                    names.append(name)
            rows.append(row)
        # columns in AXES order, whatever order the dicts named them in
        return cls([a for a in AXES if a in names], rows)

    # ---------------- shape ----------------
    @property
    def n_groups(self) -> int:
        return len(self._rows)

    def __len__(self) -> int:
        return len(self._rows)

    @property
    def has_power_cap(self) -> bool:
        return "power_cap" in self.axes

    def group_size(self, replicas: int) -> int:
        G = self.n_groups
        if int(replicas) % G != 0 or int(replicas) < G:
            raise ValueError(
                f"replicas = {replicas} is not a multiple of the sweep's "
                f"{G} groups")
        return int(replicas) // G

    def group_of(self, gid: int, replicas: int) -> int:
        return int(gid) // self.group_size(replicas)

    def slice_of(self, g: int, shard) -> Tuple[int, int]:
        """Local ``[a, b)`` of group ``g`` on ``shard`` (a ReplicaShard);
        ``a == b`` where the shard holds none of it."""
        if not 0 <= int(g) < self.n_groups:
            raise ValueError(f"group {g} outside [0, {self.n_groups})")
        n = self.group_size(shard.global_replicas)
        a = min(max(g * n, shard.start), shard.end) - shard.start
        b = min(max((g + 1) * n, shard.start), shard.end) - shard.start
        return int(a), int(b)

    # ---------------- values ----------------
    def resolved(self, base: Optional[SweepBase] = None) -> np.ndarray:
        """[G, 7] f64 in AXES order; an axis a point does not name takes the
        base value (NaN without a base)."""
        out = np.empty((self.n_groups, len(AXES)))
        for g, row in enumerate(self._rows):
            for k, name in enumerate(AXES):
                out[g, k] = row[name] if name in row else (
                    getattr(base, name) if base is not None else np.nan)
        return out

    def point(self, g: int, base: Optional[SweepBase] = None) -> Dict[str, float]:
        """Group g's full parameter point (with a base) or its named axes."""
        if base is None:
            return dict(self._rows[g])
        return dict(zip(AXES, self.resolved(base)[g].tolist()))

    def table(self, shard, base: SweepBase):
        """``arr [count, 2, 3]`` f64 (job type; rate, amp, period) and ``cap
        [count]`` f64 for the shard's replicas."""
        n = self.group_size(shard.global_replicas)
        groups = np.arange(shard.start, shard.end) // n
        vals = self.resolved(base)[groups]              # [count, 7]
        arr = np.ascontiguousarray(vals[:, :6].reshape(-1, 2, 3))
        cap = np.ascontiguousarray(vals[:, 6])
        return arr, cap

    def frame(self, base: Optional[SweepBase] = None):
        """One row per group: ``group`` and its parameters (all seven with a
        base, the named axes without)."""
        import pandas as pd
        cols = list(AXES) if base is not None else list(self.axes)
        vals = self.resolved(base)
        data = {"group": np.arange(self.n_groups)}
        for name in cols:
            data[name] = vals[:, AXES.index(name)]
        return pd.DataFrame(data)

    # ---------------- validation against an engine ----------------
    def validate(self, *, base: SweepBase, algo: str, replicas: int,
                 arrival_trace=None, arrival_pregen: bool = True,
                 subwave: int = 64) -> None:
        """Raise ValueError, with the reason, where this sweep cannot run on
        an engine of that configuration."""
        self.group_size(replicas)
        if algo == "chsac_af":
            raise ValueError("sweep: chsac_af draws its arrivals inside the "
                             "advance kernel; sweeps live in the arrival-ring "
                             "generator")
        if arrival_trace is not None:
            raise ValueError("sweep: arrival_trace replays recorded arrivals; "
                             "there are no arrival parameters to sweep")
        if not arrival_pregen:
            raise ValueError("sweep: arrival_pregen=False has no arrival-ring "
                             "generator, which is where a sweep lives")
        if int(subwave) != 64:
            raise ValueError("sweep: the 8-lane build (subwave=8) has no "
                             "arrival-ring generator, which is where a sweep "
                             "lives")
        for jt, mode in (("inf", base.inf_mode), ("trn", base.trn_mode)):
            swept = [a for a in self.axes if a.startswith(jt + "_")]
            if swept and mode == "off":
                raise ValueError(
                    f"sweep: axis {swept[0]} sweeps a job type whose base "
                    "arrival mode is 'off' (modes are not swept)")
            if mode == "profile" and jt + "_amp" in self.axes:
                raise ValueError(
                    f"sweep: axis {jt}_amp sweeps a job type in arrival mode "
                    "'profile', which has no amplitude (its table sets the "
                    "shape; sweep the rate or the period)")
        if self.has_power_cap and algo != "cap_greedy":
            raise ValueError(
                f"sweep: a power_cap axis needs algo='cap_greedy', got "
                f"{algo!r} (cap_uniform is a no-op; eco_route and carbon_cost "
                "only test cap > 0)")
        # base values fill the axes a point leaves out: check those too
        for name, v in zip(AXES, self.resolved(base).T):
            for g, x in enumerate(v):
                _check_value(name, x, f"group {g}")

    def __repr__(self) -> str:
        return f"Sweep({self.n_groups} points over {', '.join(self.axes)})"
