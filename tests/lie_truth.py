"""A plain numpy truth for the SO3 / SE3 operations and the BA pose retraction.

Written from the textbook definitions (Rodrigues' formula, the left Jacobian V of SO3 and its inverse, the quaternion
product), and from nothing else: no code is shared with oracle/ or with the kernels.  Every function works on batches of
rows and takes a `dtype`:

  * dtype=REF is the truth the tests compare against;
  * dtype=np.float32 evaluates the *same* well-conditioned formulas with every intermediate rounded to float32.  Its
    distance from the float64 evaluation is what float32 must cost, and is the yardstick of the tests' bounds.

Conventions (those of the package): quaternion rows are (x, y, z, w); an SE3 row is (t[3], q[4]); an SE3 tangent row is
(tau[3], phi[3]); group elements are re-normalised when they are loaded (`load=True`, what every op of the Lie classes
does), except in the retraction, which uses the stored pose as it is.

Where a closed form loses digits to cancellation at small angles (sin(t/2)/t, (1 - cos t)/t^2, (t - sin t)/t^3,
(1 - (t/2) cot(t/2))/t^2) the power series is used below `switch` (0.5 rad) and the closed form above it; the two agree to
1e-15 where they overlap (tests/test_lie_truth_cpu.py).
"""
from fractions import Fraction
from math import factorial

import numpy as np

SWITCH = 0.5        # rad: power series below, closed forms above
LOG_SERIES = 1e-3   # |v| of a unit quaternion below which log uses the series of atan
N_TERMS = 14

# |B_2|, |B_4|, ... |B_28| (Bernoulli numbers): (t/2) cot(t/2) = 1 - sum_k |B_2k| t^2k / (2k)!
_BERNOULLI = [Fraction(1, 6), Fraction(1, 30), Fraction(1, 42), Fraction(1, 30), Fraction(5, 66), Fraction(691, 2730),
              Fraction(7, 6), Fraction(3617, 510), Fraction(43867, 798), Fraction(174611, 330), Fraction(854513, 138),
              Fraction(236364091, 2730), Fraction(8553103, 6), Fraction(23749461029, 870)]

# coefficients in powers of theta^2, as exact fractions (rounded once, to the dtype they are used in)
_C_S = [Fraction((-1) ** k, 2 * 4 ** k * factorial(2 * k + 1)) for k in range(N_TERMS)]    # sin(t/2) / t
_C_1 = [Fraction((-1) ** k, factorial(2 * k + 2)) for k in range(N_TERMS)]                 # (1 - cos t) / t^2
_C_2 = [Fraction((-1) ** k, factorial(2 * k + 3)) for k in range(N_TERMS)]                 # (t - sin t) / t^3
_C_D = [_BERNOULLI[k] / factorial(2 * k + 2) for k in range(N_TERMS)]                      # (1 - (t/2) cot(t/2)) / t^2
_C_ATAN = [Fraction((-1) ** k, 2 * k + 1) for k in range(6)]                               # atan(x) / x in x^2

# The reference evaluation.  float64 where the platform has nothing wider; x86's 80-bit long double where it has: the
# float64 evaluation of these formulas is itself a few 2^-53 from the exact value, and what float64 costs can only be
# measured against something finer.
REF = np.longdouble if np.finfo(np.longdouble).eps < 2.0 ** -60 else np.float64


def _a(x, dtype):
    return np.asarray(x, dtype=dtype)


def _poly(coeffs, x2):
    """sum_k coeffs[k] * x2^k by Horner's rule, in x2's dtype"""
    dt = x2.dtype.type
    co = [dt(c.numerator) / dt(c.denominator) for c in coeffs]
    acc = np.full_like(x2, co[-1])
    for c in co[-2::-1]:
        acc = acc * x2 + c
    return acc


def _norm(v):
    return np.sqrt((v * v).sum(-1))


def _pick(small, series, closed):
    return np.where(small, series, closed)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def hat(p):
    """[p]_x, the matrix of the cross product p x ."""
    z = np.zeros_like(p[..., 0])
    return np.stack([np.stack([z, -p[..., 2], p[..., 1]], -1),
                     np.stack([p[..., 2], z, -p[..., 0]], -1),
                     np.stack([-p[..., 1], p[..., 0], z], -1)], -2)


# ---- the scalar functions of the angle ---------------------------------------------------------------------------------

def half_sinc(theta, switch=SWITCH):
    """s(theta) = sin(theta / 2) / theta"""
    dt = theta.dtype.type
    small = theta < dt(switch)
    safe = np.where(small, dt(1), theta)
    return _pick(small, _poly(_C_S, theta * theta), np.sin(dt(0.5) * safe) / safe)


def v_coeffs(theta, switch=SWITCH):
    """c1 = (1 - cos t) / t^2 (as 2 sin^2(t/2) / t^2 in closed form) and c2 = (t - sin t) / t^3"""
    dt = theta.dtype.type
    small = theta < dt(switch)
    safe = np.where(small, dt(1), theta)
    th2 = theta * theta
    sh = np.sin(dt(0.5) * safe)
    c1 = _pick(small, _poly(_C_1, th2), dt(2) * sh * sh / (safe * safe))
    c2 = _pick(small, _poly(_C_2, th2), (safe - np.sin(safe)) / (safe * safe * safe))
    return c1, c2


def vinv_coeff(theta, switch=SWITCH):
    """d = (1 - (t/2) cot(t/2)) / t^2, the coefficient of Phi^2 in V^-1"""
    dt = theta.dtype.type
    small = theta < dt(switch)
    safe = np.where(small, dt(1), theta)
    half = dt(0.5) * safe
    return _pick(small, _poly(_C_D, theta * theta), (dt(1) - half * np.cos(half) / np.sin(half)) / (safe * safe))


# ---- quaternions and rotations ----------------------------------------------------------------------------------------

def quat_normalize(q, dtype=REF):
    q = _a(q, dtype)
    return q / _norm(q)[..., None]


def quat_mul(a, b, dtype=REF):
    """Hamilton product a b of (x, y, z, w) rows"""
    a, b = _a(a, dtype), _a(b, dtype)
    av, aw, bv, bw = a[..., :3], a[..., 3:], b[..., :3], b[..., 3:]
    v = aw * bv + bw * av + cross(av, bv)
    w = aw * bw - (av * bv).sum(-1, keepdims=True)
    return np.concatenate([v, w], -1)


def quat_conj(q):
    return np.concatenate([-q[..., :3], q[..., 3:]], -1)


def rotation_matrix(q, dtype=REF, load=True):
    """R(q) of a unit quaternion: (w^2 - v.v) I + 2 v v^T + 2 w [v]_x with |q| = 1, i.e. I + 2 w [v]_x + 2 [v]_x^2"""
    q = quat_normalize(q, dtype) if load else _a(q, dtype)
    dt = q.dtype.type
    V = hat(q[..., :3])
    w = q[..., 3][..., None, None]
    return np.eye(3, dtype=dtype) + dt(2) * w * V + dt(2) * (V @ V)


def rotate(q, p, dtype=REF, load=True):
    """R(q) p = p + 2 w (v x p) + 2 v x (v x p)"""
    q = quat_normalize(q, dtype) if load else _a(q, dtype)
    p = _a(p, dtype)
    dt = q.dtype.type
    v, w = q[..., :3], q[..., 3:]
    c = cross(v, p)
    return p + dt(2) * (w * c + cross(v, c))


# ---- SO3 ---------------------------------------------------------------------------------------------------------------

def so3_exp(phi, dtype=REF, switch=SWITCH):
    """Exp(phi) = (s(theta) phi, cos(theta / 2)), theta = |phi|"""
    phi = _a(phi, dtype)
    dt = phi.dtype.type
    theta = _norm(phi)
    return np.concatenate([half_sinc(theta, switch)[..., None] * phi, np.cos(dt(0.5) * theta)[..., None]], -1)


def so3_log(q, dtype=REF, flip=True, load=True):
    """Log(q) = 2 atan2(|v|, w) v / |v| of the unit quaternion with w >= 0 (q and -q are the same rotation)"""
    q = quat_normalize(q, dtype) if load else _a(q, dtype)
    dt = q.dtype.type
    if flip:
        q = np.where(q[..., 3:] < 0, -q, q)
    v, w = q[..., :3], q[..., 3]
    n = _norm(v)
    small = n < dt(LOG_SERIES)
    safe_n = np.where(small, dt(1), n)
    safe_w = np.where(small, w, dt(1))
    x = n / safe_w
    series = dt(2) / safe_w * _poly(_C_ATAN, x * x)          # 2 atan(n / w) / n
    closed = dt(2) * np.arctan2(safe_n, w) / safe_n
    return _pick(small, series, closed)[..., None] * v


def left_jacobian(phi, dtype=REF, switch=SWITCH, drop_c2=False):
    """V(phi) = I + c1 Phi + c2 Phi^2"""
    phi = _a(phi, dtype)
    c1, c2 = v_coeffs(_norm(phi), switch)
    Phi = hat(phi)
    V = np.eye(3, dtype=dtype) + c1[..., None, None] * Phi
    return V if drop_c2 else V + c2[..., None, None] * (Phi @ Phi)


def left_jacobian_inverse(phi, dtype=REF, switch=SWITCH):
    """V^-1(phi) = I - Phi / 2 + d Phi^2"""
    phi = _a(phi, dtype)
    dt = phi.dtype.type
    Phi = hat(phi)
    return np.eye(3, dtype=dtype) - dt(0.5) * Phi + vinv_coeff(_norm(phi), switch)[..., None, None] * (Phi @ Phi)


def _mv(M, v):
    return (M * v[..., None, :]).sum(-1)


# ---- SE3 ---------------------------------------------------------------------------------------------------------------

def se3_split(X, dtype=REF, load=True):
    X = _a(X, dtype)
    return X[..., :3], (quat_normalize(X[..., 3:], dtype) if load else X[..., 3:])


def se3_exp(xi, dtype=REF, switch=SWITCH, drop_c2=False):
    """Exp(tau, phi) = (V(phi) tau, Exp(phi))"""
    xi = _a(xi, dtype)
    t = _mv(left_jacobian(xi[..., 3:], dtype, switch, drop_c2), xi[..., :3])
    return np.concatenate([t, so3_exp(xi[..., 3:], dtype, switch)], -1)


def se3_log(X, dtype=REF, switch=SWITCH, flip=True, load=True):
    """Log(t, q) = (V^-1(phi) t, phi), phi = Log(q)"""
    t, _ = se3_split(X, dtype, load=False)
    phi = so3_log(_a(X, dtype)[..., 3:], dtype, flip, load)
    return np.concatenate([_mv(left_jacobian_inverse(phi, dtype, switch), t), phi], -1)


def se3_mul(X, Y, dtype=REF, load=True):
    """(t1, q1)(t2, q2) = (t1 + R(q1) t2, q1 q2)"""
    t1, q1 = se3_split(X, dtype, load)
    t2, q2 = se3_split(Y, dtype, load)
    q = quat_mul(q1, q2, dtype)
    return np.concatenate([t1 + rotate(q1, t2, dtype, load=False), quat_normalize(q, dtype) if load else q], -1)


def se3_inv(X, dtype=REF, load=True):
    """(t, q)^-1 = (-R(q)^T t, q*)"""
    t, q = se3_split(X, dtype, load)
    qi = quat_conj(q)
    return np.concatenate([-rotate(qi, t, dtype, load=False), qi], -1)


def se3_act(X, p, dtype=REF, load=True):
    t, q = se3_split(X, dtype, load)
    return rotate(q, p, dtype, load=False) + t


def se3_act4(X, p, dtype=REF, load=True):
    """homogeneous points (x, y, z, w): (R p + w t, w)"""
    t, q = se3_split(X, dtype, load)
    p = _a(p, dtype)
    return np.concatenate([rotate(q, p[..., :3], dtype, load=False) + p[..., 3:] * t, p[..., 3:]], -1)


def se3_adjoint_matrix(X, dtype=REF, load=True):
    """Ad(t, R) = [[R, [t]_x R], [0, R]] on tangents ordered (tau, phi)"""
    t, q = se3_split(X, dtype, load)
    R = rotation_matrix(q, dtype, load=False)
    Z = np.zeros_like(R)
    return np.concatenate([np.concatenate([R, hat(t) @ R], -1), np.concatenate([Z, R], -1)], -2)


def se3_adj(X, a, dtype=REF, load=True):
    return _mv(se3_adjoint_matrix(X, dtype, load), _a(a, dtype))


def se3_adjT(X, a, dtype=REF, load=True):
    return _mv(np.swapaxes(se3_adjoint_matrix(X, dtype, load), -1, -2), _a(a, dtype))


def se3_matrix(X, dtype=REF, load=True):
    t, q = se3_split(X, dtype, load)
    R = rotation_matrix(q, dtype, load=False)
    top = np.concatenate([R, t[..., :, None]], -1)
    bottom = np.broadcast_to(_a([0, 0, 0, 1], dtype), top.shape[:-2] + (1, 4))
    return np.concatenate([top, bottom], -2)


# ---- SO3 as a group of rows (x, y, z, w) -------------------------------------------------------------------------------

def so3_mul(X, Y, dtype=REF, load=True):
    q = quat_mul(quat_normalize(X, dtype) if load else X, quat_normalize(Y, dtype) if load else Y, dtype)
    return quat_normalize(q, dtype) if load else q


def so3_inv(X, dtype=REF, load=True):
    return quat_conj(quat_normalize(X, dtype) if load else _a(X, dtype))


def so3_act4(X, p, dtype=REF, load=True):
    p = _a(p, dtype)
    return np.concatenate([rotate(X, p[..., :3], dtype, load), p[..., 3:]], -1)


def so3_adj(X, a, dtype=REF, load=True):
    return _mv(rotation_matrix(X, dtype, load), _a(a, dtype))


def so3_adjT(X, a, dtype=REF, load=True):
    return _mv(np.swapaxes(rotation_matrix(X, dtype, load), -1, -2), _a(a, dtype))


def so3_matrix(X, dtype=REF, load=True):
    R = rotation_matrix(X, dtype, load)
    M = np.zeros(R.shape[:-2] + (4, 4), dtype=dtype)
    M[..., :3, :3] = R
    M[..., 3, 3] = 1
    return M


SO3, SE3 = 1, 3      # group ids of the package

_OPS = {
    SO3: {"exp": so3_exp, "log": so3_log, "inv": so3_inv, "mul": so3_mul, "act": rotate, "act4": so3_act4,
          "adj": so3_adj, "adjT": so3_adjT, "matrix": so3_matrix},
    SE3: {"exp": se3_exp, "log": se3_log, "inv": se3_inv, "mul": se3_mul, "act": se3_act, "act4": se3_act4,
          "adj": se3_adj, "adjT": se3_adjT, "matrix": se3_matrix},
}


def lie(group, op, x, y=None, dtype=REF, **kw):
    """the operation `op` of `group` on rows, with the call shape of the package's lie_op and of the oracle's lie"""
    fn = _OPS[group][op]
    with np.errstate(all="ignore"):
        return fn(x, dtype=dtype, **kw) if y is None else fn(x, y, dtype=dtype, **kw)


# ---- the BA pose retraction ---------------------------------------------------------------------------------------------

def retract(xi, P, dtype=REF):
    """P <- Exp(xi) P on stored poses (t, q) whose quaternions are used as they are (not normalised):
    t' = R(Exp(phi)) t + V(phi) tau,  q' = Exp(phi) q"""
    xi, P = _a(xi, dtype), _a(P, dtype)
    with np.errstate(all="ignore"):
        D = se3_exp(xi, dtype)
        t = rotate(D[..., 3:], P[..., :3], dtype, load=False) + D[..., :3]
        return np.concatenate([t, quat_mul(D[..., 3:], P[..., 3:], dtype)], -1)
