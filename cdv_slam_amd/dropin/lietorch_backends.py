"""Drop-in for the reference's `lietorch_backends` extension (cdvslam/lietorch/src/lietorch.cpp:286-316).
Forward and backward ops of SO3 (group id 1) and SE3 (3), `projector` and `Jinv`; one HIP launch each (csrc/lie.hip,
lie_bwd.hip).  A group element's gradient is the left-perturbation row vector in the first K of its N words (DESIGN.md "The
lietorch backward").  RxSO3 (2) and Sim3 (4) raise NotImplementedError."""
from cdv_slam_amd import ops


def expm(group_id, a):
    return ops.lie_op(group_id, "exp", a)


def logm(group_id, X):
    return ops.lie_op(group_id, "log", X)


def inv(group_id, X):
    return ops.lie_op(group_id, "inv", X)


def mul(group_id, X, Y):
    return ops.lie_op(group_id, "mul", X, Y)


def adj(group_id, X, a):
    return ops.lie_op(group_id, "adj", X, a)


def adjT(group_id, X, a):
    return ops.lie_op(group_id, "adjT", X, a)


def act(group_id, X, p):
    return ops.lie_op(group_id, "act", X, p)


def act4(group_id, X, p):
    return ops.lie_op(group_id, "act4", X, p)


def as_matrix(group_id, X):
    return ops.lie_op(group_id, "matrix", X)


def projector(group_id, X):
    """[n, N, N]: the derivative of the stored row of Exp(eps) X by eps in the first K columns, the last column zero"""
    return ops.lie_op(group_id, "projector", X)


def Jinv(group_id, X, a):
    """Jl^-1(Log X) a, [n, K]"""
    return ops.lie_op(group_id, "Jinv", X, a)


def _backward(op):
    def f(group_id, grad, *inputs):
        return [g for g in ops.lie_backward(group_id, op, grad, *inputs) if g is not None]
    return f


# (group_id, grad, *inputs) -> the list of input gradients, as the reference's do: [da], [dX], [dX, dY], [dX, da], [dX, dp]
expm_backward = _backward("exp")
logm_backward = _backward("log")
inv_backward = _backward("inv")
mul_backward = _backward("mul")
adj_backward = _backward("adj")
adjT_backward = _backward("adjT")
act_backward = _backward("act")
act4_backward = _backward("act4")
