"""numpy-float32 restatement of the K21 kernels and of the DDIM schedule they are fed from (test infrastructure only,
like adam_ema_ref_cpu.py): one IEEE operation per line, in the reference's order
(ldm/models/diffusion/ddim.py:284-374 p_sample_ddim, ldm/modules/diffusionmodules/util.py:56-96,
train-scripts/train-esd.py:307-311).  numpy evaluates each float32 line as one correctly rounded operation, which is
what the kernels are compared against bit for bit.
"""
import numpy as np

F = np.float32


# ------------------------------------------------------------------------------------------ schedule
def alphas_cumprod(T=1000, linear_start=0.00085, linear_end=0.0120):
    """The LDM "linear" schedule in float64 (util.py:24-30), rounded once to the fp32 buffer of the model."""
    betas = np.linspace(linear_start ** 0.5, linear_end ** 0.5, T, dtype=np.float64) ** 2
    return np.cumprod(1.0 - betas, axis=0).astype(F)


def ddim_tables(ac32, S, eta=0.0):
    """-> dict(timesteps, alphas f32, alphas_prev f64 (fp32 values), sigmas f64, sqrt_one_minus_alphas f32)."""
    ac32 = np.asarray(ac32, F)
    T = ac32.shape[0]
    ts = np.asarray(list(range(0, T, T // S))) + 1
    alphas = ac32[ts]
    alphas_prev = np.asarray([ac32[0]] + ac32[ts[:-1]].tolist(), np.float64)
    a64 = alphas.astype(np.float64)
    sigmas = eta * np.sqrt((1 - alphas_prev) / (1 - a64) * (1 - a64 / alphas_prev))
    one_minus = F(1.0) - alphas
    return dict(timesteps=ts, alphas=alphas, alphas_prev=alphas_prev, sigmas=sigmas, sqrt_one_minus_alphas=np.sqrt(one_minus))


def coefficients(tables, index):
    """(c_s1m, c_sqrt_at, c_dir, c_sqrt_aprev, c_sigma), each float32."""
    a_t = F(tables["alphas"][index])
    a_prev = F(tables["alphas_prev"][index])
    sigma = F(tables["sigmas"][index])
    c_s1m = F(tables["sqrt_one_minus_alphas"][index])
    c_sqrt_at = np.sqrt(a_t)
    one_minus_prev = F(1.0) - a_prev
    sigma_sq = sigma * sigma
    under = one_minus_prev - sigma_sq
    c_dir = np.sqrt(under)
    c_sqrt_aprev = np.sqrt(a_prev)
    return c_s1m, c_sqrt_at, c_dir, c_sqrt_aprev, sigma


# ------------------------------------------------------------------------------------------ 1a
def ldm_ddim_step(x, eps, scale, c_s1m, c_sqrt_at, c_dir, c_sqrt_aprev, c_sigma=0.0, z=None):
    """-> (x_prev, x0).  `eps` with 2B rows: rows [0, B) unconditional, [B, 2B) conditional; with B rows: no guidance."""
    x, eps = np.asarray(x, F), np.asarray(eps, F)
    B = x.shape[0]
    scale, c_s1m, c_sqrt_at, c_dir = F(scale), F(c_s1m), F(c_sqrt_at), F(c_dir)
    c_sqrt_aprev, c_sigma = F(c_sqrt_aprev), F(c_sigma)
    if eps.shape[0] == 2 * B:
        e_u, e_c = eps[:B], eps[B:]
        d = e_c - e_u
        sd = scale * d
        e = e_u + sd
    else:
        e = eps
    se = c_s1m * e
    num = x - se
    x0 = num / c_sqrt_at
    direction = c_dir * e
    ax = c_sqrt_aprev * x0
    x_prev = ax + direction
    if c_sigma != 0:
        sz = c_sigma * np.asarray(z, F)
        x_prev = x_prev + sz
    assert x_prev.dtype == F and x0.dtype == F
    return x_prev, x0


# ------------------------------------------------------------------------------------------ 1b
def esd_loss(e_n, e_0p, ng):
    """-> (loss float64 — the exact mean of the fp32 squares' float64 sum is what the device is bounded against —,
    d_e_n f32, target f32)."""
    e_n, e_0p = np.asarray(e_n, F), np.asarray(e_0p, F)
    B = e_n.shape[0]
    e_0, e_p = e_0p[:B], e_0p[B:]
    ng = F(ng)
    diff = e_p - e_0
    sc = ng * diff
    target = e_0 - sc
    d = e_n - target
    coef = F(2.0 / e_n.size)
    d_e_n = coef * d
    loss = float((d.astype(np.float64) ** 2).sum() / e_n.size)
    return loss, d_e_n, target
