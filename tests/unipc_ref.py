"""UniPC (Zhao et al. 2023, arXiv:2302.04867) in float64 numpy, written from the paper's update formulas for the data-prediction
form — the yardstick of tests/test_unipc_cpu.py.  It imports nothing from asva_amd.schedulers: the tests hand it a sigma table.

With alpha = 1 / sqrt(1 + sigma^2), sigma_t = sigma alpha, lambda = log(alpha / sigma_t), one update of order p from s to t,
h = lambda_t - lambda_s, z = -h, uses the data prediction m0 at s and p - 1 (predictor) or p (corrector) further ones m_k at
lambda_s + r_k h:

    x_t = (sigma_t / sigma_s) x - alpha_t (e^z - 1) m0 - alpha_t B(z) sum_k rho_k (m_k - m0) / r_k
    R rho = b,   R[j][k] = r_k^j,   b[j] = z phi_{j+2}(z) (j + 1)! / B(z)     (j = 0 .. p - 1; the predictor drops the last
                                                                               row and column, whose r is 1: the point t itself)
    phi_0(z) = e^z,  phi_{k+1}(z) = (phi_k(z) - 1 / k!) / z,   B(z) = z (bh1) or e^z - 1 (bh2)

and, as the released implementation does, rho = 1/2 where one coefficient is left (order-2 predictor, order-1 corrector).
"""
import math

import numpy as np


def alpha_sigma(sig):
    a = 1.0 / math.sqrt(1.0 + sig * sig)
    return a, sig * a


def lam(sig):
    a, s = alpha_sigma(sig)
    return math.log(a) - math.log(s)


def phi(k, z):
    v = math.exp(z)
    for j in range(k):
        v = (v - 1.0 / math.factorial(j)) / z
    return v


def B(z, variant):
    return z if variant == "bh1" else math.expm1(z)


def rhos(rs, z, variant, corrector):
    """rs: the r_k of the earlier points; the corrector appends r = 1"""
    rs = list(rs) + [1.0]
    p = len(rs)
    R = np.array([[r ** j for r in rs] for j in range(p)], dtype=np.float64)
    b = np.array([z * phi(j + 2, z) * math.factorial(j + 1) / B(z, variant) for j in range(p)], dtype=np.float64)
    if corrector:
        return np.array([0.5]) if p == 1 else np.linalg.solve(R, b)
    if p == 1:
        return np.zeros(0)
    return np.array([0.5]) if p == 2 else np.linalg.solve(R[:-1, :-1], b[:-1])


def update(x, sig_s, sig_t, m0, earlier, variant, m_t=None):
    """earlier: [(sigma_k, m_k)] newest first; m_t given = corrector"""
    a_t, s_t = alpha_sigma(sig_t)
    if s_t == 0.0:                                   # h infinite: only valid at first order, where x_t = m0
        assert not earlier and m_t is None
        return m0.copy()
    h = lam(sig_t) - lam(sig_s)
    if h == 0.0:
        return x.copy()
    z = -h
    rs = [(lam(sk) - lam(sig_s)) / h for sk, _ in earlier]
    rho = rhos(rs, z, variant, corrector=m_t is not None)
    pts = [(r, mk) for r, (_, mk) in zip(rs, earlier)] + ([(1.0, m_t)] if m_t is not None else [])
    res = np.zeros_like(x)
    for c, (r, mk) in zip(rho, pts):
        res = res + c * (mk - m0) / r
    return (s_t / alpha_sigma(sig_s)[1]) * x - a_t * math.expm1(z) * m0 - a_t * B(z, variant) * res


def sample(sigmas, eps_fn, x, order, variant="bh2", lower_order_final=True, disable_corrector=()):
    """n forwards over the n + 1 sigmas; eps_fn(x, i) is the model at sigmas[i].  Returns the predictions x_1 .. x_n (the sample
    the model sees at step i + 1) and the corrected samples."""
    n = len(sigmas) - 1
    sig = [float(s) for s in sigmas]
    ms, outs, corrected = [], [], []
    last, prev_order = None, 0
    for i in range(n):
        a, s = alpha_sigma(sig[i])
        m_i = (x - s * eps_fn(x, i)) / a                                   # from the uncorrected sample the model saw
        if i > 0 and (i - 1) not in disable_corrector:
            q = prev_order
            x = update(last, sig[i - 1], sig[i], ms[i - 1], [(sig[i - 1 - k], ms[i - 1 - k]) for k in range(1, q)], variant, m_t=m_i)
        ms.append(m_i)
        p = min(order, n - i) if lower_order_final else order
        p = min(p, i + 1)
        if i == n - 1 and (sig[n] == 0.0 or sig[n] == sig[n - 1]):
            p = 1
        last, prev_order = x, p
        corrected.append(x)
        x = update(x, sig[i], sig[i + 1], m_i, [(sig[i - k], ms[i - k]) for k in range(1, p)], variant)
        outs.append(x)
    return outs, corrected
