"""The device's own log/exp routines against a high-precision reference.

fig_weights_n (fig_engine_shared.h: w = exp(0.5 log10 x), the weights of the shared-factor E-step) and fig_pweights
(fig_engine_partial.h: t = ln x and w = 10^t from the rounded t, the partial E-step) replace the library's routines with
hand-written sequences on v_rcp_f64 and the frexp builtins.  tools/probe/fig_mathprobe.hip calls the shipped functions on the
device, one thread per group of arguments; here its output is compared with mpmath at 60 digits on one fixed seeded set of
about 10^5 arguments (arguments() below).

Bounds, from the headers' own claims rounded up to whole ulps:
  fig_weights_n   |w - W| / W <= ulp(log10 x) + 2^-52: half of a 2-ulp error of log10 x carried into the exponent, plus one
                  ulp for the exp stage.
  fig_pweights    |t - ln x| <= 2 ulp;  |w - 10^t| <= 2 ulp AT THE DEVICE'S OWN ROUNDED t (the reference takes pow(10, log(p)) of
                  the rounded logarithm too, and a 1-ulp difference in t moves 10^t by up to ~10^3 ulp whatever computes it).
  exact           x = 0 -> w = 0, t = -inf;  x = 1 -> w = 1, t = 0.

Measured on an MI355X: MEASURED below."""
import math
import os
import subprocess

import numpy as np
import pytest

from tools import build_test_infra as infra

MEASURED = """
fig_weights_n<4>, 61 119 arguments: max |w - W| / W = 0.316 of the bound.  Read as an error of log10 x (which includes the exp
  stage and the final rounding of w): at most 2.38 ulp for x < 0.5, above 1 ulp on 1.0e-3 of the arguments (glibc's log10 and
  exp through the same measure: 2.47 ulp, 1.0e-3).  In ulps of w itself the figure says nothing: exp(0.5 L) turns one ulp of
  L near -300 into ~10^2 ulp of w whatever computes it.
fig_pweights<2>, 30 403 arguments: t within 0.9985 ulp of ln x, none above 1 ulp; w within 1.0 ulp of 10^t at the device's
  rounded t, none above 1 ulp."""

SEED = 20260
SQRT_HALF = 0.70710678118654752440


def _neighbours(x, k):
    out, lo, hi = [x], x, x
    for _ in range(k):
        lo = math.nextafter(lo, -math.inf); hi = math.nextafter(hi, math.inf)
        out += [lo, hi]
    return out


def arguments():
    """-> (x for fig_weights_n, x for fig_pweights): fixed, seeded, all in [0, 1]."""
    import mpmath
    mpmath.mp.dps = 60
    rng = np.random.default_rng(SEED)
    x = [10.0 ** rng.uniform(-300.0, 0.0, size=50000)]                          # products of the size the E-step produces, log-uniform
    x.append(np.ldexp(rng.uniform(0.5, 1.0, size=4000), rng.integers(-1073, -1021, size=4000)))      # subnormals
    x.append(np.array([math.ldexp(1.0, -e) for e in range(0, 1075)]))           # exact powers of two down to 2^-1074
    sw = []
    for e in list(range(0, -1022, -7)) + [-1021]:                              # mantissas in the last ulps either side of sqrt(1/2): `lowhalf`
        sw += [math.ldexp(m, e) for m in _neighbours(SQRT_HALF, 4)]
    x.append(np.array(sw))
    x.append(np.array([0.0, 1.0, 1.0 - 2.0 ** -53, 5e-324] + [1.0 - k * 2.0 ** -53 for k in range(2, 40)] + [1.0 - 2.0 ** -k for k in range(2, 53)]))
    x.append(1.0 - 10.0 ** rng.uniform(-16.0, -1.0, size=3000))                 # the neighbourhood of 1 (m - 1 cancels)
    # 0.5 log10(x) log2(e) within 2^-40 of a half-integer (the `rint` switch of the exp stage): x = 10^((2k + 1) ln 2)
    ln2 = mpmath.log(2)
    hs = []
    for k in range(-1, -234, -1):                                                # 2^-1074 <= x < 1
        hs += _neighbours(float(mpmath.power(10, (2 * k + 1) * ln2)), 3)
    x.append(np.array(hs))
    xw = np.concatenate(x).astype(np.float64)
    assert ((xw >= 0) & (xw <= 1)).all()
    lo = math.ldexp(1.0, -1070)
    xp = xw[(xw >= lo) | (xw == 0)][::2]                                        # fig_pweights: the same arguments over [2^-1070, 1], and 0
    xp = np.concatenate([xp, np.array([0.0, 1.0, 1.0 - 2.0 ** -53, lo])])
    return xw, xp


def _ulp(v):
    return math.ulp(float(v))


def check_weights(x, w):
    """-> figures; asserts the bound of fig_weights_n on every argument."""
    import mpmath
    mp = mpmath.mp; mp.dps = 60
    c = mpmath.mpf(1) / (2 * mpmath.log(10))
    il10 = 1 / mpmath.log(10)
    worst_ratio = worst_lg = 0.0; over1 = 0; n = 0
    for xv, wv in zip(x.tolist(), w.tolist()):
        if xv == 0.0:
            assert wv == 0.0 and not math.copysign(1.0, wv) < 0, "x = 0 must give w = 0"
            continue
        if xv == 1.0:
            assert wv == 1.0, f"x = 1 must give w = 1, got {wv!r}"
            continue
        lx = mpmath.log(mpmath.mpf(xv))
        W = mpmath.exp(lx * c)
        rel = float(abs(mpmath.mpf(wv) - W) / W)
        ul = _ulp(lx * il10)
        bound = ul + 2.0 ** -52
        # the whole error read as an error of log10 x, in its ulps (w = exp(0.5 log10 x): d w / w = 0.5 d log10 x); the exp
        # stage's own share is in there too, so near x = 1, where ulp(log10 x) is tiny, this figure is large and says little
        lg = rel / (0.5 * ul)
        n += 1
        if xv < 0.5:
            over1 += lg > 1.0; worst_lg = max(worst_lg, lg)
        worst_ratio = max(worst_ratio, rel / bound)
        assert rel <= bound, f"fig_weights_n({xv.hex()}) = {wv.hex()}: relative error {rel:.3e} > {bound:.3e}"
    return dict(n=n, max_error_over_bound=worst_ratio, max_as_ulp_of_log10_below_half=worst_lg, share_over_1ulp_of_log10_below_half=over1 / max(n, 1))


def check_pweights(x, t, w):
    import mpmath
    mp = mpmath.mp; mp.dps = 60
    l10 = mpmath.log(10)
    worst_t = worst_w = 0.0; over_t = over_w = 0; n = 0
    for xv, tv, wv in zip(x.tolist(), t.tolist(), w.tolist()):
        if xv == 0.0:
            assert tv == -math.inf and wv == 0.0, "x = 0 must give t = -inf, w = 0"
            continue
        if xv == 1.0:
            assert tv == 0.0 and wv == 1.0, f"x = 1 must give t = 0, w = 1, got {tv!r}, {wv!r}"
            continue
        T = mpmath.log(mpmath.mpf(xv))
        ut = float(abs(mpmath.mpf(tv) - T)) / _ulp(T)
        W = mpmath.exp(mpmath.mpf(tv) * l10)                   # at the device's own rounded t
        uw = float(abs(mpmath.mpf(wv) - W)) / _ulp(W)
        n += 1; over_t += ut > 1.0; over_w += uw > 1.0
        worst_t = max(worst_t, ut); worst_w = max(worst_w, uw)
        assert ut <= 2.0, f"fig_pweights({xv.hex()}): t = {tv.hex()} is {ut:.2f} ulp from ln x"
        assert uw <= 2.0, f"fig_pweights({xv.hex()}): w = {wv.hex()} is {uw:.2f} ulp from 10^t at t = {tv.hex()}"
    return dict(n=n, max_ulp_t=worst_t, share_t_over_1ulp=over_t / max(n, 1), max_ulp_w=worst_w, share_w_over_1ulp=over_w / max(n, 1))


def test_the_checker_accepts_the_library_and_rejects_a_wrong_last_digit():
    """The comparison itself, on the CPU: numpy's log10 / exp / log / power (each within 1 ulp) pass both bounds on a slice of
    the arguments; a log10 that is 4 ulp off, or a 10^t that is 3 ulp off, does not."""
    xw, xp = arguments()
    assert 9.0e4 < len(xw) + len(xp) < 1.2e5
    xs = np.concatenate([xw[::40], np.array([0.0, 1.0])])
    w = np.exp(0.5 * np.log10(np.where(xs == 0, 1, xs))); w[xs == 0] = 0.0
    assert check_weights(xs, w)["n"] > 1000
    l = np.log10(xs[(xs > 0) & (xs < 0.5)]); l4 = l + 4 * np.spacing(np.abs(l))
    with pytest.raises(AssertionError):
        check_weights(xs[(xs > 0) & (xs < 0.5)], np.exp(0.5 * l4))
    ps = np.concatenate([xp[::40], np.array([0.0, 1.0])])
    with np.errstate(divide="ignore"):
        t = np.log(ps)
    pw = np.array([10.0 ** v if v > -745 else 0.0 for v in t.tolist()])
    assert check_pweights(ps, t, pw)["n"] > 500
    bad = pw.copy(); k = int(np.argmax((pw > 1e-300) & (pw < 1))); bad[k] = pw[k] + 3 * np.spacing(pw[k])
    with pytest.raises(AssertionError):
        check_pweights(ps, t, bad)


@pytest.mark.gpu
def test_device_log_exp_routines_within_their_stated_bounds(tmp_path):
    """fig_weights_n<4> and fig_pweights<2> as shipped, on the device, against mpmath: the bounds of the module docstring on
    every argument.  The measured maxima are printed (and kept in MEASURED and in the headers' comments)."""
    assert os.path.exists(infra.MATHPROBE), "tests/emu/fig_mathprobe is not built (tools/build_test_infra.py needs hipcc)"
    xw, xp = arguments()
    fw, fp = str(tmp_path / "w.f64"), str(tmp_path / "p.f64")
    xw.astype("<f8").tofile(fw); xp.astype("<f8").tofile(fp)
    r = subprocess.run(["timeout", "-k", "10", "120", infra.MATHPROBE, fw, fp], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    W = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("W ")]
    P = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("P ")]
    assert len(W) == len(xw) and len(P) == len(xp)
    f64 = lambda col: np.array([int(h, 16) for h in col], dtype=np.uint64).view(np.float64)
    assert f64([f[1] for f in W]).tobytes() == xw.tobytes() and f64([f[1] for f in P]).tobytes() == xp.tobytes()
    fig_w = check_weights(xw, f64([f[2] for f in W]))
    print("fig_weights_n:", fig_w)
    fig_p = check_pweights(xp, f64([f[2] for f in P]), f64([f[3] for f in P]))
    print("fig_pweights:", fig_p)
