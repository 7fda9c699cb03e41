"""The truth of tests/lie_truth.py checks itself; the CPU oracle's Lie arithmetic (oracle/lie_impl.h) against it on the
input set of tests/lie_cases.py (the set the kernels are held to in tests/test_lie_angles.py); the loss the reference's
float32 formula carries is written down; and the bounds are shown to fail what is wrong."""
import numpy as np
import pytest

import lie_cases as LC
import lie_truth as LT
from oracle import oracle as O

GROUPS = [(LC.SO3, "SO3"), (LC.SE3, "SE3")]
U64, U32 = 2.0 ** -53, 2.0 ** -24
# the decades of the rotation angle in which (1 - cos theta) / theta^2 costs the translation of exp more than the format
C1_BANDS = ["1e-6", "1e-5", "1e-4", "1e-3", "1e-2"]


def _oracle(group, op, args):
    return O.lie(group, op, *args, dtype=args[0].dtype)


def _quiet(line):
    pass


# ---- the truth checks itself --------------------------------------------------------------------------------------------

def test_series_and_closed_forms_agree_where_they_overlap():
    """theta in [0.3, 0.7]: the power series (switch above every angle) against the closed forms (switch at 0), in float64,
    on the coefficients and on what they produce for |tau| = 1"""
    rng = np.random.default_rng(0)
    theta = rng.uniform(0.3, 0.7, 2000)
    # (c2 and d enter as c2 Phi^2 and d Phi^2: compared with their theta^2)
    for fn in (LT.half_sinc, lambda t, s: LT.vinv_coeff(t, s) * t * t, lambda t, s: LT.v_coeffs(t, s)[0],
               lambda t, s: LT.v_coeffs(t, s)[1] * t * t):
        assert np.abs(fn(theta, 10.0) - fn(theta, 0.0)).max() <= 1e-15
    a = np.concatenate([LC._axes(rng, 2000), theta[:, None] * LC._axes(rng, 2000)], 1)
    Xs, Xc = LT.se3_exp(a, np.float64, switch=10.0), LT.se3_exp(a, np.float64, switch=0.0)
    assert np.abs(Xs - Xc).max() <= 1e-15
    assert np.abs(LT.se3_log(Xs, np.float64, switch=10.0) - LT.se3_log(Xs, np.float64, switch=0.0)).max() <= 1e-15


@pytest.mark.parametrize("group,gname", GROUPS, ids=[g[1] for g in GROUPS])
def test_truth_group_identities(group, gname):
    """exp o log, X X^-1 = 1, X Exp(a) = Exp(Ad_X a) X, act against the 4 x 4 matrix: float64, to a few roundings"""
    f = np.float64
    rng = np.random.default_rng(1)
    K = 6 if group == LC.SE3 else 3
    n = 500
    a = 0.5 * rng.standard_normal((n, K)) * 10.0 ** rng.uniform(-6, 0, (n, 1))      # angles below pi
    L = lambda op, *args: LT.lie(group, op, *args, dtype=f)
    X = L("exp", a)
    assert np.abs(L("log", X) - a).max() <= 16 * U64 * max(1, np.abs(a).max())
    eye = L("mul", X, L("inv", X))
    assert np.abs(np.abs(eye[:, -1]) - 1).max() <= 8 * U64 and np.abs(eye[:, :-1]).max() <= 16 * U64 * max(1, np.abs(X).max())
    b = rng.standard_normal((n, K))
    left, right = L("mul", X, L("exp", b)), L("mul", L("exp", L("adj", X, b)), X)
    assert np.abs(L("matrix", left) - L("matrix", right)).max() <= 64 * U64 * max(1, np.abs(left).max())
    p, p4 = rng.standard_normal((n, 3)), rng.standard_normal((n, 4))
    M = L("matrix", X)
    assert np.abs(L("act", X, p) - (M[:, :3, :3] @ p[:, :, None])[:, :, 0] - M[:, :3, 3]).max() <= 16 * U64 * 4
    assert np.abs(L("act4", X, p4) - (M @ p4[:, :, None])[:, :, 0]).max() <= 16 * U64 * 4
    Ad = np.stack([L("adj", X, np.tile(np.eye(K)[c], (n, 1))) for c in range(K)], -1)
    assert np.abs(L("adjT", X, b) - np.einsum("nji,nj->ni", Ad, b)).max() <= 16 * U64 * max(1, np.abs(Ad).max())


def test_retraction_is_exp_times_pose():
    rng = np.random.default_rng(2)
    xi = rng.standard_normal((200, 6)) * 10.0 ** rng.uniform(-6, 0, (200, 1))
    P = LT.se3_exp(rng.standard_normal((200, 6)))
    assert np.abs(LT.retract(xi, P) - LT.se3_mul(LT.se3_exp(xi), P)).max() <= 1e-15
    # a stored pose that is not unit length keeps its length: the retraction does not normalise
    P[:, 3:] *= 1.01
    assert np.allclose(np.linalg.norm(np.asarray(LT.retract(xi, P), np.float64)[:, 3:], axis=1), 1.01, atol=1e-14)


# ---- the float64 oracle against the truth -----------------------------------------------------------------------------

@pytest.mark.parametrize("group,gname", GROUPS, ids=[g[1] for g in GROUPS])
def test_oracle_f64_against_truth(group, gname):
    """oracle/lie_impl.h in float64 on the whole input set, row by row, against the error model
         translation of exp:   8 u (scale + |tau| / max(theta, 1e-6))      (the reference's c1 = (1 - cos theta) / theta^2)
         everything else:      8 u scale,                      scale = max(1, |want|_max over the row's band), u = 2^-53"""
    cases = LC.Cases(group, np.float64)
    for op in LC.OPS:
        args, band, theta = cases.args(op)
        want = LC.truth_quantities(group, op, args, theta)
        got = LC.quantities(group, op, _oracle(group, op, args), args, theta)
        for k in want:
            err = np.abs(got[k] - want[k]).max(1).astype(np.float64)
            scale = LC.band_max(want[k], band)
            model = 8 * U64 * np.maximum(1.0, np.array([scale[int(b)] for b in band]))
            if op == "exp" and k == "t":
                tau = np.linalg.norm(args[0][:, :3], axis=1)
                model = model + 8 * U64 * tau / np.maximum(theta, 1e-6)
            worst = np.argmax(err / model)
            assert np.all(err <= model), (op, k, cases.band_name(band[worst]), err[worst], model[worst])


@pytest.mark.parametrize("group,gname", GROUPS, ids=[g[1] for g in GROUPS])
def test_oracle_f64_round_trips(group, gname):
    bad = [b for b in LC.round_trip_failures(LC.Cases(group, np.float64), _oracle, out=_quiet) if not _is_c1(b)]
    assert not bad, "\n".join(LC.FAILURE % b for b in bad)


def _is_c1(failure):
    """a failure of exp's translation in the decades where the reference's c1 loses it"""
    return failure[1] == "t" and any(failure[2].startswith("theta %s," % b) for b in C1_BANDS)


# ---- the loss of the reference's float32 formula, written down ----------------------------------------------------------

def test_oracle_f32_loss_is_the_translation_of_exp_alone():
    """oracle/lie_impl.h in float32 restates the reference: c1 = (1 - cos theta) / theta^2.  In the decade 1e-4 ... 1e-3 its
    exp translation is more than 50 x further from the truth than the float32 evaluation of the truth's formulas is
    (measured: 3e-4 |tau| against 2e-7 |tau|).  Everything else -- every other op, quantity and band, SO3 and SE3, and
    exp's translation above 0.1 and below 1e-6 -- keeps the bound the kernels are held to."""
    cases = LC.Cases(LC.SE3, np.float32)
    (a,), band, theta = cases.args("exp")
    want = LC.truth_quantities(LC.SE3, "exp", (a,), theta)
    cost = LC.band_max(LC.truth_quantities(LC.SE3, "exp", (a,), theta, dtype=np.float32)["t"] - want["t"], band)
    err = LC.band_max(LC.quantities(LC.SE3, "exp", _oracle(LC.SE3, "exp", (a,)), (a,), theta)["t"] - want["t"], band)
    for b in sorted(err):
        print("exp t [%s]: oracle float32 %.2e, truth in float32 %.2e" % (cases.band_name(b), err[b], cost[b]))
        if cases.band_name(b).startswith("theta 1e-4,"):
            assert err[b] > 50 * cost[b], (cases.band_name(b), err[b], cost[b])
    for group, _ in GROUPS:
        c = LC.Cases(group, np.float32)
        bad = LC.op_failures(c, _oracle, out=_quiet) + LC.round_trip_failures(c, _oracle, out=_quiet)
        other = [b for b in bad if not _is_c1(b)]
        assert not other, "\n".join(LC.FAILURE % b for b in other)
        if group == LC.SE3:
            assert any(b[0] == "exp" for b in bad)


# ---- the bounds can fail -------------------------------------------------------------------------------------------------

def _textbook_v_coeffs(theta, switch=LT.SWITCH):
    """c1 as the textbook writes it, (1 - cos t) / t^2, above the switch"""
    c1, c2 = _half_angle_v_coeffs(theta, switch)
    dt = theta.dtype.type
    safe = np.where(theta < dt(switch), dt(1), theta)
    return np.where(theta < dt(switch), c1, (dt(1) - np.cos(safe)) / (safe * safe)), c2


_half_angle_v_coeffs = LT.v_coeffs


def _reference_pi_branch(group, op, args, dtype):
    """log with the reference's near-pi branch: the angle is taken to be pi where |w| < 1e-6"""
    out = np.array(LT.lie(group, op, *args, dtype=dtype))
    q = LT.quat_normalize(args[0][:, -4:], dtype)
    near = np.abs(q[:, 3]) < 1e-6
    v = q[:, :3] * np.where(q[:, 3:] < 0, -1, 1)
    out[near, -3:] = np.pi * v[near] / np.linalg.norm(v[near], axis=1, keepdims=True)
    return out


VARIANTS = {
    # name: (ops it changes, keywords of the truth's function)
    "c2_dropped": (["exp"], dict(drop_c2=True)),
    "switch_at_1e-3_textbook_c1": (["exp"], dict(switch=1e-3)),
    "log_without_the_w_flip": (["log"], dict(flip=False)),
    "no_renormalisation_on_load": (["log", "inv", "mul", "adj", "adjT", "act", "act4", "matrix"], dict(load=False)),
    "reference_pi_branch": (["log"], None),
}


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: d.__name__)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_wrong_variants_break_the_bound(variant, dtype, monkeypatch):
    """each deliberately wrong evaluation, in the dtype of the bound, exceeds the bound of tests/lie_cases.py on at least
    one band.  (reference_pi_branch is the reference's own log at |w| < 1e-6, 2 |w| off: what lie_impl.h and the kernel
    departed from.  It is 1.8e-6 rad at |w| = 9e-7: far outside the float64 bound, and outside the float32 one.)"""
    ops_changed, kw = VARIANTS[variant]
    if variant == "switch_at_1e-3_textbook_c1":
        monkeypatch.setattr(LT, "v_coeffs", _textbook_v_coeffs)
    cases = LC.Cases(LC.SE3, dtype)

    def run(group, op, args):
        if kw is None:
            return np.asarray(_reference_pi_branch(group, op, args, dtype), dtype)
        return np.asarray(LT.lie(group, op, *[np.asarray(x, LC.REF) for x in args], dtype=dtype, **kw), dtype)

    bad = LC.op_failures(cases, run, ops=ops_changed, out=_quiet)
    print("%s in %s breaks %d bounds, e.g. %s" % (variant, np.dtype(dtype).name, len(bad), LC.FAILURE % bad[0] if bad else "-"))
    assert bad, variant


def test_moved_switch_alone_is_harmless_with_half_angle_c1():
    """the series / closed-form switch moved from 0.5 to 1e-3 while c1 keeps its half-angle closed form 2 sin^2(t/2) / t^2
    stays INSIDE the bound: the cancellations that remain, t - sin t and 1 - (t/2) cot(t/2), are multiplied by theta^2 and
    cost at most u |tau| (so the moved switch is only a wrong variant together with the textbook c1, above).  This is why
    the kernel's fix touches c1 alone."""
    for dtype in (np.float32, np.float64):
        cases = LC.Cases(LC.SE3, dtype)
        run = lambda group, op, args: np.asarray(
            LT.lie(group, op, *[np.asarray(x, LC.REF) for x in args], dtype=dtype, switch=1e-3), dtype)
        bad = LC.op_failures(cases, run, ops=["exp", "log"], out=_quiet)
        assert not bad, "\n".join(LC.FAILURE % b for b in bad)
