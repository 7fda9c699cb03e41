"""A plain numpy truth for the backward of the SO3 / SE3 operations, next to tests/lie_truth.py and in its style.

Convention (the package's, DESIGN.md "The lietorch backward"): the gradient of a scalar L with respect to a group element X
is the row vector dL/d eps at eps = 0 of L(Exp(eps) X); the incoming gradient of a group-valued output is read the same way;
tangents and points carry ordinary gradients.  With Ad the adjoint matrix, ad(b) the Lie-algebra adjoint, Jl the left
Jacobian and R / M the 3 x 3 / 4 x 4 matrix of X:

    exp(a)              da = dX Jl(a)
    log(X)              dX = da Jl^-1(Log X)
    inv(X)              dX = -dY Ad(X^-1)
    mul(X, Y)           dX = dZ,  dY = dZ Ad(X)
    adj(X, a), b = Ad(X) a      da = db Ad(X),  dX = -db ad(b)
    adjT(X, a)          da = (Ad(X) db)^T,  dX = -a ad(Ad(X) db)
    act(X, p), q = X p  dp = dq R,  dX = dq [I, -[q]x]          (SO3: -[q]x)
    act4(X, p)          dp = dq M,  dX = dq [[q_w I, -[q_xyz]x], [0]]   (SO3: the rotation columns)

Two evaluations, independent of each other:
  * `vjp` / `projector` / `jinv`: the closed forms above written as matrices from their definitions, taking a `dtype` as
    lie_truth does (REF is the truth; float32 / float64 say what the format costs and give the tests their bounds).  The
    coefficients of the SE3 coupling block Q(tau, phi) use their power series below `switch` (0.5 rad);
  * `fd_vjp` / `fd_projector` / `fd_jinv`: central differences with h = 2^-16, built from lie_truth.lie in REF alone: a group
    input is moved as Exp(h e_k) X, and the difference of a group output Z is Log(Z(h) Z^-1).
tests/test_lie_grad_truth_cpu.py holds the first against the second."""
from fractions import Fraction
from math import factorial

import numpy as np

import lie_cases as LC
import lie_truth as LT

REF, SO3, SE3, SWITCH = LT.REF, LT.SO3, LT.SE3, LT.SWITCH
H = 2.0 ** -16
BWD_OPS = ["exp", "log", "inv", "mul", "adj", "adjT", "act", "act4"]
EXTRA_OPS = ["projector", "Jinv"]
N_TERMS = LT.N_TERMS

# Q's coefficients in powers of theta^2, as exact fractions
_C_A = LT._C_2                                                                                  # (t - sin t) / t^3
_C_B = [Fraction((-1) ** k, factorial(2 * k + 4)) for k in range(N_TERMS)]                      # (t^2 + 2 cos t - 2) / 2 t^4
_C_C = [Fraction((-1) ** k * (k + 1), factorial(2 * k + 5)) for k in range(N_TERMS)]            # (2 t - 3 sin t + t cos t) / 2 t^5


def dims(group):
    """(K, N): tangent and embedded width"""
    return (6, 7) if group == SE3 else (3, 4)


def _vm(v, M):
    """row vectors times matrices"""
    return (v[..., :, None] * M).sum(-2)


def _mv(M, v):
    return (M * v[..., None, :]).sum(-1)


def q_coeffs(theta, switch=SWITCH):
    dt = theta.dtype.type
    small = theta < dt(switch)
    t = np.where(small, dt(1), theta)
    t2 = theta * theta
    s, c, sh = np.sin(t), np.cos(t), np.sin(dt(0.5) * t)
    ca = np.where(small, LT._poly(_C_A, t2), (t - s) / (t * t * t))
    cb = np.where(small, LT._poly(_C_B, t2), (dt(0.5) * t * t - dt(2) * sh * sh) / (t * t * t * t))
    cc = np.where(small, LT._poly(_C_C, t2), (dt(2) * t - dt(3) * s + t * c) / (dt(2) * t * t * t * t * t))
    return ca, cb, cc


def se3_Q(xi, dtype=REF, switch=SWITCH):
    """the coupling block of the SE3 left Jacobian (Barfoot, State Estimation for Robotics, 7.86b), T = [tau]x, P = [phi]x:
    Q = T / 2 + ca (P T + T P + P T P) + cb (P P T + T P P - 3 P T P) + cc (P T P P + P P T P)"""
    xi = np.asarray(xi, dtype)
    dt = xi.dtype.type
    T, P = LT.hat(xi[..., :3]), LT.hat(xi[..., 3:])
    ca, cb, cc = (c[..., None, None] for c in q_coeffs(LT._norm(xi[..., 3:]), switch))
    PT, TP = P @ T, T @ P
    PTP = PT @ P
    return dt(0.5) * T + ca * (PT + TP + PTP) + cb * (P @ PT + TP @ P - dt(3) * PTP) + cc * (PTP @ P + P @ PTP)


def _blocks(A, B, C, D):
    return np.concatenate([np.concatenate([A, B], -1), np.concatenate([C, D], -1)], -2)


def left_jacobian(group, a, dtype=REF, switch=SWITCH):
    """Jl(a): Exp(a + d) = Exp(Jl(a) d) Exp(a) to first order.  SE3: [[J, Q], [0, J]] on (tau, phi)"""
    a = np.asarray(a, dtype)
    if group == SO3:
        return LT.left_jacobian(a, dtype, switch)
    J = LT.left_jacobian(a[..., 3:], dtype, switch)
    return _blocks(J, se3_Q(a, dtype, switch), np.zeros_like(J), J)


def left_jacobian_inverse(group, a, dtype=REF, switch=SWITCH):
    """SE3: [[J^-1, -J^-1 Q J^-1], [0, J^-1]]"""
    a = np.asarray(a, dtype)
    if group == SO3:
        return LT.left_jacobian_inverse(a, dtype, switch)
    Ji = LT.left_jacobian_inverse(a[..., 3:], dtype, switch)
    return _blocks(Ji, -(Ji @ se3_Q(a, dtype, switch) @ Ji), np.zeros_like(Ji), Ji)


def Ad(group, X, dtype=REF):
    return LT.rotation_matrix(X, dtype) if group == SO3 else LT.se3_adjoint_matrix(X, dtype)


def ad(group, b):
    """ad(b) c = [b, c]: SO3 [b]x; SE3 [[P, T], [0, P]] for b = (tau, phi)"""
    if group == SO3:
        return LT.hat(b)
    T, P = LT.hat(b[..., :3]), LT.hat(b[..., 3:])
    return _blocks(P, T, np.zeros_like(P), P)


def _pad(g):
    """a group element's gradient as stored: K value words and a zero"""
    return np.concatenate([g, np.zeros_like(g[..., :1])], -1)


def vjp(group, op, grad, x, y=None, dtype=REF, switch=SWITCH):
    """(dx, dy) of the table in the module docstring, shaped as the package stores them (group gradients padded to N words);
    dy is None for a unary op"""
    K, N = dims(group)
    g = np.asarray(grad, dtype)
    x = np.asarray(x, dtype)
    y = None if y is None else np.asarray(y, dtype)
    with np.errstate(all="ignore"):
        if op == "exp":
            return _vm(g[..., :K], left_jacobian(group, x, dtype, switch)), None
        if op == "log":
            a = LT.lie(group, "log", x, dtype=dtype)
            return _pad(_vm(g, left_jacobian_inverse(group, a, dtype, switch))), None
        if op == "inv":
            return _pad(-_vm(g[..., :K], Ad(group, LT.lie(group, "inv", x, dtype=dtype), dtype))), None
        A = Ad(group, x, dtype)
        if op == "mul":
            return _pad(g[..., :K]), _pad(_vm(g[..., :K], A))
        if op == "adj":
            return _pad(-_vm(g, ad(group, _mv(A, y)))), _vm(g, A)
        if op == "adjT":
            c = _mv(A, g)
            return _pad(-_vm(y, ad(group, c))), c
        # act / act4
        R = LT.rotation_matrix(x[..., -4:], dtype)
        t = x[..., :3] if group == SE3 else np.zeros_like(x[..., :3])
        w = y[..., 3:] if op == "act4" else np.ones_like(y[..., :1])
        q = _mv(R, y[..., :3]) + w * t
        g3 = g[..., :3]
        rot = -_vm(g3, LT.hat(q))
        dx = np.concatenate([w * g3, rot], -1) if group == SE3 else rot
        dp = _vm(g3, R)
        if op == "act4":
            dp = np.concatenate([dp, (g3 * t).sum(-1, keepdims=True) + g[..., 3:]], -1)
        return _pad(dx), dp


def projector(group, X, dtype=REF):
    """[n, N, N]: column k < K is d(stored row of Exp(eps) X) / d eps_k at 0: t' = t + tau + phi x t and
    (v, w)' = (v, w) + (w phi + phi x v, -phi . v) / 2; the last column is zero"""
    K, N = dims(group)
    X = np.asarray(X, dtype)
    dt = X.dtype.type
    q = LT.quat_normalize(X[..., -4:], dtype)
    v, w = q[..., :3], q[..., 3]
    P = np.zeros(X.shape[:-1] + (N, N), dtype)
    r = N - 4
    P[..., r:r + 3, r:r + 3] = dt(0.5) * (w[..., None, None] * np.eye(3, dtype=dtype) - LT.hat(v))
    P[..., N - 1, r:r + 3] = -dt(0.5) * v
    if group == SE3:
        P[..., :3, :3] = np.eye(3, dtype=dtype)
        P[..., :3, 3:6] = -LT.hat(X[..., :3])
    return P


def jinv(group, X, a, dtype=REF, switch=SWITCH):
    """Jl^-1(Log X) a"""
    with np.errstate(all="ignore"):
        xi = LT.lie(group, "log", np.asarray(X, dtype), dtype=dtype)
        return _mv(left_jacobian_inverse(group, xi, dtype, switch), np.asarray(a, dtype))


# ---- central differences, from lie_truth.lie alone ---------------------------------------------------------------------

_GROUP_IN = {"exp": (False,), "log": (True,), "inv": (True,), "mul": (True, True), "adj": (True, False), "adjT": (True, False),
             "act": (True, False), "act4": (True, False)}
_GROUP_OUT = {"exp": True, "log": False, "inv": True, "mul": True, "adj": False, "adjT": False, "act": False, "act4": False}


def _moved(group, x, is_group, k, h):
    """input k-th direction: Exp(h e_k) X for a group element, x + h e_k otherwise"""
    if not is_group:
        x = x.copy()
        x[:, k] += REF(h)
        return x
    e = np.zeros((len(x), dims(group)[0]), REF)
    e[:, k] = REF(h)
    return LT.lie(group, "mul", LT.lie(group, "exp", e), x)


def fd_vjp(group, op, grad, x, y=None, h=H):
    """(dx, dy) by central differences, shaped like vjp's"""
    K, N = dims(group)
    g = np.asarray(grad, REF)
    args = [np.asarray(x, REF)] + ([] if y is None else [np.asarray(y, REF)])
    Zi = LT.lie(group, "inv", LT.lie(group, op, *args)) if _GROUP_OUT[op] else None

    def out(a):
        z = LT.lie(group, op, *a)
        return LT.lie(group, "log", LT.lie(group, "mul", z, Zi)) if _GROUP_OUT[op] else z

    res = []
    for i, is_group in enumerate(_GROUP_IN[op]):
        width = K if is_group else args[i].shape[1]
        d = np.zeros((len(g), width), REF)
        for k in range(width):
            hi = out([_moved(group, a, is_group, k, h) if j == i else a for j, a in enumerate(args)])
            lo = out([_moved(group, a, is_group, k, -h) if j == i else a for j, a in enumerate(args)])
            d[:, k] = (g[:, :hi.shape[1]] * (hi - lo)).sum(1) / REF(2 * h)
        res.append(_pad(d) if is_group else d)
    return res[0], (res[1] if len(res) > 1 else None)


def fd_projector(group, X, h=H):
    K, N = dims(group)
    X = np.asarray(X, REF)
    P = np.zeros((len(X), N, N), REF)
    for k in range(K):
        P[:, :, k] = (_moved(group, X, True, k, h) - _moved(group, X, True, k, -h)) / REF(2 * h)
    return P


def fd_jinv(group, X, a, h=H):
    """d Log(Exp(s a) X) / ds at 0"""
    X, a = np.asarray(X, REF), np.asarray(a, REF)
    hi = LT.lie(group, "log", LT.lie(group, "mul", LT.lie(group, "exp", REF(h) * a), X))
    lo = LT.lie(group, "log", LT.lie(group, "mul", LT.lie(group, "exp", REF(-h) * a), X))
    return (hi - lo) / REF(2 * h)


# ---- the input set and the bounds of the kernel tests --------------------------------------------------------------------

def case_args(cases, op, seed=7):
    """(grad, inputs, band, theta) of `op` on the input set `cases` (lie_cases.Cases); Jinv's second operand is the set's
    tangent operand, the projector has no gradient"""
    K, N = dims(cases.group)
    inputs, band, theta = cases.args({"projector": "log", "Jinv": "adj"}.get(op, op))
    width = {"exp": N, "log": K, "inv": N, "mul": N, "adj": K, "adjT": K, "act": 3, "act4": 4, "projector": 0, "Jinv": 0}[op]
    rng = np.random.default_rng(seed + LC.OPS.index(op) if op in LC.OPS else seed)
    grad = rng.standard_normal((len(inputs[0]), width)).astype(cases.dtype)
    if _GROUP_OUT.get(op):
        grad[:, K] = 0
    return grad, inputs, band, theta


def log_is_unique(cases):
    """rows whose rotation is away from pi: where phi and -phi are one rotation, Jl^-1(Log X) has two values.  Leaves out the
    band `pi` and the elements with |w| in lie_cases.W_SPECIAL -- for log and Jinv only"""
    band = cases.X_band // len(LC.TAU_SIZES)
    special = np.zeros(len(cases.X), bool)
    special[-len(LC.W_SPECIAL) * 2 * 11:] = True
    return (band != LC.THETA_BANDS.index("pi")) & ~special


def truth_outputs(group, op, grad, inputs, dtype=REF):
    """{name: rows} of what the package returns for `op`"""
    inputs = [np.asarray(a, REF) for a in inputs]
    if op == "projector":
        return {"P": projector(group, inputs[0], dtype).reshape(len(inputs[0]), -1)}
    if op == "Jinv":
        return {"Jinv": jinv(group, inputs[0], inputs[1], dtype)}
    dx, dy = vjp(group, op, np.asarray(grad, REF), *inputs, dtype=dtype)
    return {"dx": dx} if dy is None else {"dx": dx, "dy": dy}


def bounds(group, op, grad, inputs, band, dtype, rows=None):
    """(want, {name: {band: bound}}) in the style of lie_cases.bounds: per output and band, 4 x what the number format costs
    the closed forms on the same rows, plus 4 u max(1, |want|)"""
    dtype = np.dtype(dtype)
    want = truth_outputs(group, op, grad, inputs)
    low = truth_outputs(group, op, grad, inputs, dtype)
    rows = np.ones(len(band), bool) if rows is None else rows
    out = {}
    for k in want:
        c, s = LC.band_max((low[k] - want[k])[rows], band[rows]), LC.band_max(want[k][rows], band[rows])
        out[k] = {b: 4 * c[b] + 4 * LC.U[dtype] * max(1.0, s[b]) for b in c}
    return want, out
