"""SDE-DPM-Solver++(2M) restated in float64 with the standard library's math, for the tests of solver 'dpmpp2m_sde': the
coefficient rows (A, E, C, hx, he, G), the stored-noise rows (r, q) and the covariance recursion of (x, h) over a table on
Gaussian data.  It shares no arithmetic with diffusion/schedule.py: only the training schedule's alpha_bar (the oracle's) and
the list of sampling timesteps come from outside."""
import math

from oracle import ref_cpu as R


def alpha_bars(num_train_steps=1000):
    return [float(a) for a in R.alphas_cumprod(R.linear_beta_schedule(num_train_steps)).tolist()]


def rows64(ab, ts, eta):
    """-> ([S][6] coefficient rows, [S][2] stored-noise rows) of the loop over the timesteps ts (decreasing), float64"""
    lam = lambda t: 0.5 * math.log(ab[t] / (1.0 - ab[t]))
    S = len(ts)
    coef, rq = [], []
    for i, s in enumerate(ts):
        al_s, sg_s = math.sqrt(ab[s]), math.sqrt(1.0 - ab[s])
        hx, he = 1.0 / al_s, -sg_s / al_s
        if i == S - 1:                                                 # to alpha_bar = 1
            coef.append([1.0 / al_s, -sg_s / al_s, 0.0, hx, he, 0.0])
            rq.append([0.0, 0.0])
            continue
        t = ts[i + 1]
        al_t, sg_t = math.sqrt(ab[t]), math.sqrt(1.0 - ab[t])
        h = lam(t) - lam(s)
        c = h / (2.0 * (lam(s) - lam(ts[i - 1]))) if i > 0 else 0.0
        g = -al_t * math.expm1(-(1.0 + eta) * h)
        coef.append([(sg_t / sg_s) * math.exp(-eta * h) + g * (1.0 + c) / al_s, -g * (1.0 + c) * sg_s / al_s, -g * c, hx, he,
                     sg_t * math.sqrt(-math.expm1(-2.0 * eta * h))])
        rq.append([math.exp(-eta * h), math.sqrt(-math.expm1(-2.0 * eta * h))])
    return coef, rq


def gains(ab, ts, s2):
    """the analytic optimal denoiser of x0 ~ N(0, s2) at every level of the loop: eps = k x, k = sigma / (a s2 + 1 - a)"""
    return [math.sqrt(1.0 - ab[t]) / (ab[t] * s2 + 1.0 - ab[t]) for t in ts]


def final_variance(coef, ks):
    """Var x after the loop x' = A x + E k x + C h + G z', h' = hx x + he k x from x ~ N(0, 1), h = 0, z' a fresh unit normal
    per step: the exact covariance recursion of (x, h).  coef: rows of 6 floats (any table, e.g. the fp32 one)"""
    vxx, vxh, vhh = 1.0, 0.0, 0.0
    for (A, E, C, hx, he, G), k in zip(coef, ks):
        m, n = A + E * k, hx + he * k
        vxx, vxh, vhh = m * m * vxx + 2.0 * m * C * vxh + C * C * vhh + G * G, m * n * vxx + C * n * vxh, n * n * vxx
    return vxx


def first_order_ratio(ab, ts, eta, s2):
    """final variance / s2 of the first-order eta loop (DDIM eq. 12, 16) on the same data, float64"""
    v = 1.0
    for i, t in enumerate(ts):
        a, p = ab[t], (ab[ts[i + 1]] if i + 1 < len(ts) else 1.0)
        sg = eta * math.sqrt((1 - p) / (1 - a)) * math.sqrt(1 - a / p)
        cx = math.sqrt(p) / math.sqrt(a)
        ce = math.sqrt(max(1 - p - sg * sg, 0.0)) - math.sqrt(p) * math.sqrt(1 - a) / math.sqrt(a)
        k = math.sqrt(1 - a) / (a * s2 + 1 - a)
        v = (cx + ce * k) ** 2 * v + sg * sg
    return v / s2
