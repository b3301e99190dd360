"""The solver step's arithmetic restated in numpy: the yardstick of test_solver_step_cpu.py and test_solver_step_gpu.py.
Imports nothing from the library.  Every operation is one numpy operation on arrays of the case's dtype, so it is rounded
once in that dtype (numpy's +, -, *, / and sqrt are correctly rounded and never fused); the hyper-parameters are cast to
the dtype first, and 1 + momentum, 1 - beta1, 1 - beta2 are formed in it.

What it restates (the reference's solvers):
  Normalize            sgd_solver.cpp:118-143   diff *= 1 / iter_size               -> diff_scale
  Regularize           sgd_solver.cpp:145-204   L2: diff += decay * w (155-160);  L1: diff += decay * sign(w) (161-168),
                                                caffe_cpu_sign: (0 < x) - (x < 0), so sign(+-0) = sign(NaN) = 0
  SGDUpdate            sgd_solver.cu:7-12       g = h = momentum*h + local_rate*g
  NesterovUpdate       nesterov_solver.cu:7-14  h' = momentum*h + local_rate*g;  g = (1+momentum)*h' - momentum*h
  AdamUpdate           adam_solver.cu:7-15      m = m*beta1 + g*(1-beta1);  v = v*beta2 + g*g*(1-beta2);
                                                g = corrected_local_rate*m / (sqrt(v) + eps_hat)
  Blob::Update         blob.cpp                 w = w - g
The float temporaries that the reference's Nesterov and Adam kernels keep in their double instantiation are not restated:
double cases compute in double throughout."""
import numpy as np

SGD, NESTEROV, ADAM = 0, 1, 2
REG_NONE, REG_L2, REG_L1 = 0, 1, 2
RULES = {"sgd": SGD, "nesterov": NESTEROV, "adam": ADAM}
REGS = {"none": REG_NONE, "L2": REG_L2, "L1": REG_L1}


def step(w, g, h, h2, type, regularization=REG_NONE, rate=0.0, momentum=0.0, momentum2=0.999, delta=1e-8, decay=0.0,
         diff_scale=1.0):
    """One step on flat arrays of one dtype.  Returns (w', h', h2') as new arrays; h2 may be None unless type is ADAM
    (h2' is then None).  The arguments are left unchanged."""
    dt = w.dtype.type
    assert all(a.dtype == w.dtype for a in (g, h)) and (h2 is None or h2.dtype == w.dtype)
    rate_t, mom, mom2, delta_t, decay_t, scale_t = dt(rate), dt(momentum), dt(momentum2), dt(delta), dt(decay), dt(diff_scale)
    one = dt(1)
    with np.errstate(all="ignore"):
        g = g.copy()
        if diff_scale != 1.0:
            g = scale_t * g
        if decay != 0.0 and regularization == REG_L2:
            r = decay_t * w
            g = g + r
        elif decay != 0.0 and regularization == REG_L1:
            sign = ((w > 0).astype(np.int32) - (w < 0).astype(np.int32)).astype(w.dtype)
            r = decay_t * sign
            g = g + r
        if type == ADAM:
            one_minus_b1, one_minus_b2 = one - mom, one - mom2
            a = h * mom
            b = g * one_minus_b1
            m = a + b
            gg = g * g
            c = h2 * mom2
            d = gg * one_minus_b2
            v = c + d
            num = rate_t * m
            den = np.sqrt(v) + delta_t
            u = num / den
            h_new, h2_new = m, v
        else:
            a = mom * h
            b = rate_t * g
            h_new = a + b
            h2_new = None
            if type == NESTEROV:
                one_plus = one + mom
                c = one_plus * h_new
                u = c - a
            else:
                u = h_new
        w_new = w - u
    for a in (w_new, h_new) + (() if h2_new is None else (h2_new,)):
        assert a.dtype == w.dtype
    return w_new, h_new, h2_new


def bits_equal(a, b):
    """Same dtype, shape and bytes (NaN == NaN, -0.0 != +0.0)."""
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def equal_up_to_nan_payload(a, b):
    """Same dtype and shape, NaN at the same positions, every other element the same bits (-0.0 != +0.0).  The rule
    promises one IEEE operation per step, and IEEE leaves a NaN's payload and sign open: bits_equal would compare them."""
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    bits = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(bits)[~na], b.view(bits)[~nb]))


def seeded_values(n, seed, dt, zeros=True):
    """n seeded values in (-1, 1); with `zeros` (and n >= 8) a few exactly 0 and one -0.0."""
    rs = np.random.RandomState(seed)
    v = rs.uniform(-1, 1, n).astype(dt)
    v[v == 0] = 0.5
    if zeros and n >= 8:
        pick = rs.choice(n, size=min(5, n // 2), replace=False)
        v[pick[1:]] = 0.0
        v[pick[0]] = -0.0
    return v
