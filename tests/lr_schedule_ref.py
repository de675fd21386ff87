"""The learning-rate multiplier of a schedule in float64, written from its definition (include/mmego_hip.h, above MmegoLrSchedule) and
from nothing else: the tests of the kernels and of params.LrSchedule compare against it.

kind 0 constant, 1 cosine, 2 linear, 3 step; W warm-up steps, D span, r floor, E / g the step decay.  t >= 1 is the step about to be taken."""
import math

KINDS = {"constant": 0, "cosine": 1, "linear": 2, "step": 3}


def mult_ref(kind, t, W=0, D=1, r=0.0, E=1, g=1.0):
    kind = KINDS.get(kind, kind)
    t, W, D, r, E, g = float(t), float(W), float(D), float(r), float(E), float(g)
    w = t / W if (W > 0 and t < W) else 1.0
    s = max(0.0, t - W)
    if s == 0.0:
        return w * 1.0                                   # (d is exactly 1 where s == 0)
    x = min(s, D) / D
    if kind == 0:
        d = 1.0
    elif kind == 1:
        d = r + (1.0 - r) * (1.0 + math.cos(math.pi * x)) / 2.0
    elif kind == 2:
        d = r + (1.0 - r) * (1.0 - x)
    elif kind == 3:
        d = max(r, g ** math.floor(s / E))
    else:
        raise ValueError(kind)
    return w * d


def default_span(epochs, steps_per_epoch, warmup):
    """The span of a cosine or linear decay that is not given one: the rest of the run, at least one step."""
    return max(1, epochs * steps_per_epoch - warmup)
