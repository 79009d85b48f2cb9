"""CPU twins of the optimiser step (include/nrs.h, "optimiser"), written from the rule stated there, not from the kernel.

twin64 is the arbiter: every operation in float64 on the fp32 inputs taken as real numbers; only what the rule itself rounds is rounded -- the bias table's entries and
the EMA's a and b, once, to fp32.  twin32 is the same sequence of operations in float32 (numpy's IEEE single: correctly rounded +, *, /, sqrt, no contraction), and
so the reference's own gap: what float32 arithmetic costs against the real-number rule.  Both take and return a `State`; neither changes its input.

The EMA reads the STORED fp16 copy, a step function of the master weight: a master weight that lands within float32's reach of a rounding boundary of fp16 may be
stored one fp16 step apart by two correct implementations, and the EMA then differs by b x that step, far beyond any float32 bar.  `fp16_for_ema` therefore lets the
caller hand the twin the fp16 array that the implementation under test stored (its own test: bit-equal to the rounding of its own master), so that the EMA is
judged as what it is, one multiply-add per element on given inputs.
"""
import dataclasses

import numpy as np


@dataclasses.dataclass
class Hyper:
    beta1: float = 0.9
    beta2: float = 0.99
    epsilon: float = 1e-15
    l2_reg: float = 1e-6
    non_matrix_lr_factor: float = 1.0
    ema_decay: float = 0.95

    def f32(self, name):
        return np.float32(getattr(self, name))


@dataclasses.dataclass
class State:
    master: np.ndarray  # float32 values (twin64 returns float64)
    m: np.ndarray
    v: np.ndarray
    steps: np.ndarray   # uint32
    ema: np.ndarray
    fp16: np.ndarray    # float16
    step_count: int = 0

    def copy(self):
        return State(*(a.copy() for a in (self.master, self.m, self.v, self.steps, self.ema, self.fp16)), self.step_count)


def bias_table(beta1, beta2):
    """bias(t) = sqrt(1 - beta2^t) / (1 - beta1^t) in float64 on the fp32 betas, each value rounded once to fp32, for t = 1 .. T_sat at index t - 1; T_sat is the
    first t from which on the rounded value is exactly 1.0f.  Found by brute force up to 2^17 (independent of the library's closed-form bound)."""
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    t = np.arange(1, (1 << 17) + 1, dtype=np.float64)
    vals = (np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)).astype(np.float32)
    not_one = np.nonzero(vals != np.float32(1.0))[0]
    t_sat = int(not_one[-1]) + 2 if not_one.size else 1  # (index + 1 is the last t that is not 1; the next t is T_sat)
    assert t_sat < (1 << 17), "the table does not saturate within 2^17 steps"
    return vals[:t_sat]


def ema_coefficients(decay, T):
    """a = d (1 - d^(T-1)) / (1 - d^T), b = (1 - d) / (1 - d^T) in float64 on the fp32 decay, rounded once to fp32"""
    d = float(np.float32(decay))
    den = 1.0 - d ** T
    return np.float32(d * (1.0 - d ** (T - 1)) / den), np.float32((1.0 - d) / den)


def exponential_decay_lr(base, decay_start, decay_interval, decay_base, steps_done):
    k = 0 if steps_done < decay_start else (steps_done - decay_start) // max(decay_interval, 1) + 1
    return np.float32(float(np.float32(base)) * float(np.float32(decay_base)) ** k)


def _step(st, grad, hp, n_matrix, loss_scale, lr, table, dtype, fp16_for_ema):
    F = dtype
    f = lambda x: F(np.float32(x))  # a scalar of the rule: an fp32 value, carried in the twin's precision
    n = st.master.size
    matrix = np.arange(n) < n_matrix
    w, m, v = st.master.astype(F), st.m.astype(F), st.v.astype(F)
    with np.errstate(all="ignore"):
        g = grad.astype(F) / f(loss_scale)
        skip = ~matrix & (g == 0)
        g = np.where(matrix, g + f(hp.l2_reg) * w, g)
        m2 = f(hp.beta1) * m + (F(1) - f(hp.beta1)) * g
        v2 = f(hp.beta2) * v + (F(1) - f(hp.beta2)) * (g * g)
        t = st.steps + np.uint32(1)
        bias = table[np.minimum(t, np.uint32(table.size)).astype(np.int64) - 1].astype(F)
        lr_i = np.where(matrix, f(lr) * F(1), f(lr) * f(hp.non_matrix_lr_factor)) * bias
        w2 = w - (lr_i / (np.sqrt(v2) + f(hp.epsilon))) * m2
    out = State(np.where(skip, w, w2), np.where(skip, m, m2), np.where(skip, v, v2), np.where(skip, st.steps, t).astype(np.uint32), st.ema.astype(F),
                st.fp16.copy(), st.step_count + 1)
    with np.errstate(over="ignore"):
        out.fp16 = np.where(skip, st.fp16, out.master.astype(np.float16))
    if hp.ema_decay > 0:
        a, b = ema_coefficients(hp.ema_decay, out.step_count)
        h = out.fp16 if fp16_for_ema is None else fp16_for_ema
        with np.errstate(all="ignore"):
            out.ema = F(a) * st.ema.astype(F) + F(b) * h.astype(F)
    return out


def twin64(st, grad, hp, n_matrix, loss_scale, lr, table=None, fp16_for_ema=None):
    table = bias_table(hp.beta1, hp.beta2) if table is None else table
    return _step(st, grad, hp, n_matrix, loss_scale, lr, table, np.float64, fp16_for_ema)


def twin32(st, grad, hp, n_matrix, loss_scale, lr, table=None, fp16_for_ema=None):
    table = bias_table(hp.beta1, hp.beta2) if table is None else table
    return _step(st, grad, hp, n_matrix, loss_scale, lr, table, np.float32, fp16_for_ema)


def ulp_error(got, exact):
    """|got - exact| in fp32 steps at the exact value's size, per element (float64)"""
    exact = np.asarray(exact, dtype=np.float64)
    with np.errstate(over="ignore"):
        ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
    err = np.abs(np.asarray(got, dtype=np.float64) - exact) / ulp
    both_nonfinite = ~np.isfinite(exact) & ~np.isfinite(np.asarray(got, dtype=np.float64))
    return np.where(both_nonfinite, 0.0, err)


def random_state(rng, n, n_matrix, steps_max=40):
    """A state as training leaves it: weights of mixed size, first moments of either sign, second moments consistent with them, uneven step counts"""
    master = (rng.normal(size=n) * np.where(np.arange(n) < n_matrix, 0.2, 1e-3)).astype(np.float32)
    m = (rng.normal(size=n) * 1e-3).astype(np.float32)
    v = (rng.random(n) * 1e-5 + m.astype(np.float64) ** 2).astype(np.float32)
    steps = rng.integers(0, steps_max, size=n).astype(np.uint32)
    ema = (master + rng.normal(size=n).astype(np.float32) * 1e-4).astype(np.float32)
    return State(master, m, v, steps, ema, master.astype(np.float16), int(steps.max()))


def random_grad(rng, n, n_matrix, loss_scale, zero_share=0.5):
    """loss_scale x a gradient of mixed size; `zero_share` of the non-matrix entries exactly zero: in runs, singly inside a group of four, and one -0.0"""
    g = (rng.normal(size=n) * 10.0 ** rng.uniform(-6, -2, size=n) * loss_scale).astype(np.float32)
    idx = np.arange(n)
    zero = rng.random(n) < zero_share * 0.7
    run = (idx // 7) % 3 == int(rng.integers(0, 3))      # runs of seven
    single = idx % 4 == int(rng.integers(0, 4))          # one element of every group of four
    pick = rng.random(n) < zero_share
    zero |= (run | single) & pick
    zero &= idx >= n_matrix
    g[zero] = 0.0
    live = np.nonzero(zero)[0]
    if live.size:
        g[live[live.size // 2]] = -0.0
    return g
