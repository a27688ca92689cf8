"""The rule by which the frame kernel answers an occlusion ray without a walk (prt_frame.h), restated in NumPy float32:
whenever the rule allows the skip, the light contribution an unoccluded answer would add,
    beta * (std_max(dot, 0) * lightIntensity / pi)          (path_tracer.cpp:226-231, 246-249)
is +-0 in every component, and adding it changes nothing but the sign of a zero."""
import itertools

import numpy as np

F = np.float32
PI = F(3.14159265358979323846)
DOTS = [F(-1.0), F(-0.0), F(0.0), F(1e-30), F(np.nan)]
BETAS = [F(0.0), F(1.0), F(np.inf), F(np.nan)]
INTENSITIES = [F(0.0), F(1.0), F(np.inf)]


def std_max(a, b):
    """std::max(a, b) = (a < b) ? b : a -- returns a when the comparison is unordered and keeps a -0."""
    return b if a < b else a


def skippable(dot, beta, intensity):
    return bool(dot <= F(0.0)) and bool(np.all(np.isfinite(beta))) and bool(np.all(np.isfinite(intensity)))


def addend(dot, beta, intensity):
    with np.errstate(invalid="ignore", over="ignore"):
        lr = (std_max(dot, F(0.0)) * intensity / PI).astype(np.float32)
        return (beta * lr).astype(np.float32)


def test_skippable_implies_the_addend_is_a_zero():
    seen_skip = seen_nan_traced = 0
    for dot in DOTS:
        for b in itertools.product(BETAS, repeat=3):
            for i in itertools.product(INTENSITIES, repeat=3):
                beta, inten = np.array(b, dtype=np.float32), np.array(i, dtype=np.float32)
                a = addend(dot, beta, inten)
                if skippable(dot, beta, inten):
                    seen_skip += 1
                    assert np.all(a == 0.0), (dot, b, i, a)  # +0 or -0, never NaN
                elif np.isnan(a).any():
                    seen_nan_traced += 1
    assert seen_skip > 0 and seen_nan_traced > 0  # the grid reaches both sides of the rule


def test_every_excluded_case_can_make_a_nan():
    """Why each condition is there: drop it and some case the rule would then skip has a NaN addend."""
    one, zero = np.ones(3, np.float32), np.zeros(3, np.float32)
    assert np.isnan(addend(F(np.nan), one, one)).all()                                   # NaN dot: std_max returns the NaN
    assert np.isnan(addend(F(-1.0), np.array([np.inf, 1, 1], np.float32), one))[0]          # inf * 0
    assert np.isnan(addend(F(-1.0), np.array([np.nan, 1, 1], np.float32), one))[0]
    assert np.isnan(addend(F(-1.0), one, np.array([np.inf, 1, 1], np.float32)))[0]          # 0 * inf
    assert not skippable(F(np.nan), one, one) and not skippable(F(1e-30), one, one)
    assert skippable(F(-0.0), one, zero) and skippable(F(0.0), zero, one)


def test_adding_a_zero_changes_at_most_the_sign_of_a_zero_which_the_packet_sum_erases():
    """result + (+-0) == result except (-0) + (+0) = +0, and the packet sum starts from +0: (+0) + (+-0) = +0, and a running sum
    that started at +0 is never -0, so the sum over the 8 slots is the same bits either way."""
    xs = np.array([0.0, -0.0, 1.0, -1.0, 1e-45, np.inf, -np.inf, 3.4e38], dtype=np.float32)
    for z in (F(0.0), F(-0.0)):
        y = (xs + z).astype(np.float32)
        differ = y.view(np.uint32) != xs.view(np.uint32)
        assert np.all(y[differ] == 0.0) and np.all(xs[differ] == 0.0)  # only a zero's sign
        for x in xs:
            res_a, res_b = F(0.0) + x, F(0.0) + (x + z)
            assert res_a.view(np.uint32) == res_b.view(np.uint32), (x, z)
