"""lietorch operator surface (reference: cdvslam/lietorch/__init__.py:2).  SO3 and SE3 on the HIP backend,
forward and backward (autograd through exp, log, inv, mul, adj, adjT, act, act4, retr; see groups.py); RxSO3 / Sim3 belong to
loop closure (out of scope)."""
from .groups import SE3, SO3, LieGroup, cat, stack

__all__ = ["SE3", "SO3", "LieGroup", "cat", "stack"]
