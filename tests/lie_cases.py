"""The input set, the compared quantities and the bounds of the Lie-op tests (tests/test_lie_truth_cpu.py on the CPU
oracle, tests/test_lie_angles.py on the kernels).  Everything here is numpy on tests/lie_truth.py: no bound looks at the
code under test.

Bands.  Every row carries a band: the decade of its rotation angle (plus `0`, `1-pi` and `pi`), and for SE3 the size of
its translation part (1e-3, 1, 100).  A bound is taken per op, compared quantity, band and dtype:

    4 * max | truth(dtype) - truth(REF) |  over the band's rows   +   4 u max(1, |want|_max over the band)

u = 2^-24 or 2^-53; REF is lie_truth.REF, float64 or wider.  (With a float64 REF the first term of a float64 bound is zero
and the bound is 4 u scale alone, which is below what a chain of five float64 roundings can keep: quaternion product,
normalisation and rotation matrix are that long.  Against the 80-bit REF the float64 truth is 2 u to 3 u off there.)
The first term is what the number format costs a well-conditioned evaluation, the second the rounding of the result itself; the factor 4: device sin / cos / atan are allowed 2 ulp where numpy's are within 1, and the
contraction of multiply-adds differs.
"""
import numpy as np

import lie_truth as LT

SO3, SE3, REF = LT.SO3, LT.SE3, LT.REF
U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
DECADES = list(range(-9, 0))                      # [1e-9, 1e-8) ... [1e-1, 1)
THETA_BANDS = ["0"] + ["1e%d" % d for d in DECADES] + ["1-pi", "pi"]
TAU_SIZES = [1e-3, 1.0, 100.0]
SCALES = [0.5, 2.0, 1 + 1e-3, 1 - 1e-3]           # stored quaternions that are not unit length
W_SPECIAL = [0.0, 1e-8, 1e-7, 9e-7, 1.1e-6]       # |w| around the near-pi branch of log (|w| < 1e-6)
N_PER_DECADE = 48
BATCHES = [1, 255, 256, 257]                      # around the 256 lanes of a workgroup; the full set is the large batch


def theta_band(theta):
    """index into THETA_BANDS of a rotation angle"""
    theta = np.asarray(theta, np.float64)
    out = np.empty(theta.shape, np.int64)
    with np.errstate(divide="ignore"):
        dec = np.floor(np.log10(np.maximum(theta, 1e-300))).astype(np.int64)
    out[:] = 1 + np.clip(dec, DECADES[0], DECADES[-1]) - DECADES[0]
    out[theta == 0] = 0
    out[theta >= 1] = THETA_BANDS.index("1-pi")
    out[theta >= np.pi - 1e-5] = THETA_BANDS.index("pi")
    return out


def _axes(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _f32_neighbours(x):
    c = np.float32(x)
    return [float(np.nextafter(c, np.float32(0))), float(c), float(np.nextafter(c, np.float32(1)))]


def rotation_vectors(rng):
    """phi rows: log-uniform angles in every decade from 1e-9 to 1 and uniform on [1, pi), random axes and the three
    coordinate axes; exactly 0 and exactly pi; both sides of the series thresholds"""
    rows = []
    eye = np.eye(3)
    for d in DECADES:
        th = 10.0 ** rng.uniform(d, d + 1, N_PER_DECADE + 3)
        rows.append(th[:, None] * np.concatenate([_axes(rng, N_PER_DECADE), eye]))
    th = rng.uniform(1.0, np.pi - 1e-3, N_PER_DECADE + 3)
    rows.append(th[:, None] * np.concatenate([_axes(rng, N_PER_DECADE), eye]))
    rows.append(np.zeros((2, 3)))
    rows.append(np.pi * np.concatenate([_axes(rng, 8), eye]))
    edges = [1e-6 * (1 - 2.0 ** -20), 1e-6 * (1 + 2.0 ** -20)]
    for x in (1e-6, 1e-4, 1e-2):
        edges += _f32_neighbours(x)
    edges = np.array(edges)
    rows.append(edges[:, None] * eye[np.arange(len(edges)) % 3])        # the angle is exactly the edge value
    rows.append(edges[:, None] * _axes(rng, len(edges)))
    return np.concatenate(rows)


class Cases:
    """one seeded input set of a group and dtype: tangents `a`, group elements `X` (built by the truth from the
    tangents, then as -q, scaled, and with |w| near 0), second operands, and the band of every row"""

    def __init__(self, group, dtype, seed=2024):
        self.group, self.dtype = group, np.dtype(dtype)
        rng = np.random.default_rng(seed + 10 * group)
        phi = rotation_vectors(rng)
        if group == SE3:
            m = len(phi)
            phi = np.tile(phi, (len(TAU_SIZES), 1))
            size = np.repeat(np.arange(len(TAU_SIZES)), m)
            tau = _axes(rng, len(phi)) * np.array(TAU_SIZES)[size][:, None]
            a = np.concatenate([tau, phi], 1)
        else:
            size = np.zeros(len(phi), np.int64)
            a = phi
        # what the code under test is given is the dtype's rounding of these rows; the truth starts from the same numbers
        self.a = np.ascontiguousarray(a.astype(dtype))
        a = self.a.astype(np.float64)
        self.a_theta = np.linalg.norm(a[:, -3:], axis=1)
        self.a_band = self._band(self.a_theta, size)

        X0 = LT.lie(group, "exp", a)
        variants = [X0, self._scaled(X0, -1.0)] + [self._scaled(X0, s) for s in SCALES]
        theta = [self.a_theta] * len(variants)
        sizes = [size] * len(variants)
        # |w| in W_SPECIAL, both signs: rotations by pi - 2 w
        ws = np.array([s * w for w in W_SPECIAL for s in (1.0, -1.0)])
        ax = np.concatenate([_axes(rng, 8), np.eye(3)])
        w = np.repeat(ws, len(ax))
        q = np.concatenate([np.sqrt(1 - w * w)[:, None] * np.tile(ax, (len(ws), 1)), w[:, None]], 1)
        if group == SE3:
            sz = np.arange(len(q)) % len(TAU_SIZES)
            q = np.concatenate([_axes(rng, len(q)) * np.array(TAU_SIZES)[sz][:, None], q], 1)
        else:
            sz = np.zeros(len(q), np.int64)
        variants.append(q)
        theta.append(np.pi - 2 * np.abs(w))
        sizes.append(sz)
        self.X = np.ascontiguousarray(np.concatenate(variants).astype(dtype))
        self.X_theta = np.concatenate(theta)
        self.X_band = self._band(self.X_theta, np.concatenate(sizes))
        n = len(self.X)
        K = 6 if group == SE3 else 3
        self.Y = np.ascontiguousarray(self.X[rng.permutation(n)])
        self.b = rng.standard_normal((n, K)).astype(dtype)
        self.p3 = rng.standard_normal((n, 3)).astype(dtype)
        self.p4 = rng.standard_normal((n, 4)).astype(dtype)

    def _scaled(self, X, s):
        X = X.copy()
        X[:, -4:] *= s
        return X

    def _band(self, theta, size):
        return theta_band(theta) * len(TAU_SIZES) + size

    def band_name(self, b):
        name = "theta " + THETA_BANDS[b // len(TAU_SIZES)]
        return name + (", |tau| %g" % TAU_SIZES[b % len(TAU_SIZES)] if self.group == SE3 else "")

    def args(self, op):
        """(inputs of `op`, band of every row, angle of every row)"""
        if op == "exp":
            return (self.a,), self.a_band, self.a_theta
        second = {"log": (), "inv": (), "matrix": (), "mul": (self.Y,), "adj": (self.b,), "adjT": (self.b,),
                  "act": (self.p3,), "act4": (self.p4,)}[op]
        return (self.X,) + second, self.X_band, self.X_theta


OPS = ["exp", "log", "inv", "mul", "adj", "adjT", "act", "act4", "matrix"]


def quantities(group, op, out, args, theta):
    """what is compared of an op's output `out`: each entry is well conditioned at every input of the set.

    exp: t and q as they are.  log: the rotation R(Exp(phi)) and the translation V(phi) tau it stands for, through the
    truth (near pi the sign of the axis hangs on the last bit of w, the rotation does not), and below theta = 3 also phi
    and tau themselves.  mul, inv: the rotation as a matrix (q and -q are one rotation), the norm of q, the translation.
    Everything else: as it is."""
    out = np.asarray(out, REF)
    n = len(out)
    se3 = group == SE3
    if op == "exp":
        return {"t": out[:, :3], "q": out[:, 3:]} if se3 else {"q": out}
    if op == "log":
        phi = out[:, -3:]
        direct = (theta < 3)[:, None]
        res = {"R(phi)": LT.rotation_matrix(LT.so3_exp(phi), load=False).reshape(n, 9), "phi, theta < 3": np.where(direct, phi, 0)}
        if se3:
            res["V(phi) tau"] = LT._mv(LT.left_jacobian(phi), out[:, :3])
            res["tau, theta < 3"] = np.where(direct, out[:, :3], 0)
        return res
    if op in ("mul", "inv"):
        q = out[:, -4:]
        res = {"R(q)": LT.rotation_matrix(q).reshape(n, 9), "|q|": np.linalg.norm(q, axis=1)[:, None]}
        if se3:
            res["t"] = out[:, :3]
        return res
    return {op: out.reshape(n, -1)}


def truth_quantities(group, op, args, theta, dtype=REF, **kw):
    """the compared quantities of the truth evaluated in `dtype` on the inputs `args` (converted exactly)"""
    a64 = [np.asarray(x, REF) for x in args]
    return quantities(group, op, LT.lie(group, op, *a64, dtype=dtype, **kw), args, theta)


def band_max(rows, band):
    """{band: max over its rows}"""
    rows = np.abs(rows).reshape(len(rows), -1).max(1)
    return {int(b): float(rows[band == b].max()) for b in np.unique(band)}


def bounds(group, op, args, band, theta, dtype):
    """{quantity: {band: bound}}: 4 x the error of the truth evaluated in `dtype`, plus 4 u scale"""
    dtype = np.dtype(dtype)
    want = truth_quantities(group, op, args, theta)
    low = truth_quantities(group, op, args, theta, dtype=dtype)
    cost = {k: low[k] - want[k] for k in want}
    out = {}
    for k in want:
        c, s = band_max(cost[k], band), band_max(want[k], band)
        out[k] = {b: 4 * c[b] + 4 * U[dtype] * max(1.0, s[b]) for b in c}
    return want, out


def errors(got_q, want_q, band):
    """{quantity: {band: max error}}"""
    return {k: band_max(got_q[k] - want_q[k], band) for k in want_q}


def report(cases, op, err, bnd, out=print):
    """prints the measured error next to each bound; returns the list of (quantity, band) that exceed it"""
    bad = []
    for k in bnd:
        for b in sorted(bnd[k]):
            e, t = err[k][b], bnd[k][b]
            ok = np.isfinite(e) and e <= t
            out("  %-4s %-15s %-28s err %.3e  bound %.3e  %s" % (op, k, cases.band_name(b), e, t, "ok" if ok else "EXCEEDS"))
            if not ok:
                bad.append((k, cases.band_name(b), e, t))
    return bad


FAILURE = "%s %s [%s]: err %.3e > bound %.3e"


def op_failures(cases, run, ops=OPS, out=print):
    """every op on every row of the set through `run(group, op, args)`: the list of (op, quantity, band, err, bound) that
    exceed their bound, after printing every error next to its bound"""
    bad = []
    for op in ops:
        args, band, theta = cases.args(op)
        want, bnd = bounds(cases.group, op, args, band, theta, cases.dtype)
        got = run(cases.group, op, args)
        assert got.dtype == cases.dtype and len(got) == len(args[0])
        err = errors(quantities(cases.group, op, got, args, theta), want, band)
        bad += [(op,) + b for b in report(cases, op, err, bnd, out)]
    return bad


def _twice(bnd):
    return {k: {b: 2 * v for b, v in d.items()} for k, d in bnd.items()}


def _loaded(X):
    X = np.asarray(X, REF).copy()
    X[:, -4:] = LT.quat_normalize(X[:, -4:])
    return X


def round_trip_failures(cases, run, out=print):
    """log(exp(a)) and exp(log(X)) through `run` alone, compared as group elements (the tangent is not unique at pi, and q
    and -q are one rotation).  Two ops in a row: the bound is twice that of one op producing a group element."""
    group, bad = cases.group, []
    (a,), band, theta = cases.args("exp")
    back = run(group, "log", (run(group, "exp", (a,)),))
    want, bnd = bounds(group, "exp", (a,), band, theta, cases.dtype)
    X = np.array(LT.lie(group, "exp", back.astype(REF)))
    X[(X[:, -4:] * want["q"]).sum(1) < 0, -4:] *= -1
    err = errors(quantities(group, "exp", X, (a,), theta), want, band)
    bad += [("log(exp(a))",) + b for b in report(cases, "l(e)", err, _twice(bnd), out)]
    (X,), band, theta = cases.args("log")
    again = run(group, "exp", (run(group, "log", (X,)),))
    _, bnd = bounds(group, "inv", (X,), band, theta, cases.dtype)          # the quantities of a group element: R, |q|, t
    want = quantities(group, "inv", _loaded(X), (X,), theta)
    err = errors(quantities(group, "inv", again, (X,), theta), want, band)
    bad += [("exp(log(X))",) + b for b in report(cases, "e(l)", err, _twice(bnd), out)]
    return bad
