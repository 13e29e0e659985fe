"""The linear multistep (LMS) sampler of the evaluation script (the reference's SD/eval-scripts/generate-images.py drives
diffusers' `LMSDiscreteScheduler`; diffusers is not part of the reference tree, so this is written from the published
algorithm: Karras et al. 2022's sigma parametrisation with the Adams-Bashforth-style multistep of k-diffusion).

Schedule (`LMSSchedule`): betas = linspace(sqrt(0.00085), sqrt(0.012), 1000)^2 and their cumulative product in fp32,
sigma = sqrt((1 - abar) / abar); `set_timesteps(n)`: t = linspace(0, 999, n)[::-1] (fractional), sigma interpolated over
t with np.interp, a final 0 appended, the result cast to fp32; init_noise_sigma = max sigma.

Step i: the U-Net reads x / sqrt(sigma_i^2 + 1) at the (float) timestep t_i; the derivative d_i is the guided epsilon;
with order = min(i + 1, 4)
    x <- x + sum_j c_ij d_(i-j),   c_ij = integral from sigma_i to sigma_(i+1) of prod_(k != j) (s - sigma_(i-k)) /
                                          (sigma_(i-j) - sigma_(i-k)) ds.
The integrand is a polynomial of degree <= 3: `coefficients(i)` integrates it in closed form in float64 (in the variable
u = s - sigma_i, so that the bounds are 0 and the step).  diffusers evaluates the same integral with
scipy.integrate.quad(epsrel=1e-4), whose Gauss-Kronrod rule is exact for a cubic up to rounding: the two agree to
float64 rounding, far below the fp32 value the step uses.

One step on the device is ONE batched U-Net pass and ONE launch of `salun_lms_step` (csrc/salun_sampler.hip), which
reads the two halves of the U-Net output in place, forms the guided d, stores it into a 4-deep history ring,
accumulates x + c_0 d + c_1 d_1 + ... in that order without contraction, writes the new x and writes
x_new / sqrt(sigma_(i+1)^2 + 1) twice into the [2B, ...] tensor the next pass reads.

Not reproduced: diffusers recomputes the derivative as (x - (x - sigma eps)) / sigma, which differs from eps by two
roundings and a division; here d = eps.  diffusers also sums the weighted derivatives first and adds x last; the kernel
adds them to x one by one.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import ops_sampler

ORDER = 4


class LMSSchedule:
    def __init__(self, beta_start: float = 0.00085, beta_end: float = 0.012, num_train_timesteps: int = 1000):
        betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
        ac = torch.cumprod(1.0 - betas, dim=0)
        self.train_sigmas = (((1 - ac) / ac) ** 0.5).numpy()          # fp32, ascending in t
        self.num_train_timesteps = int(num_train_timesteps)
        self.set_timesteps(num_train_timesteps)

    def set_timesteps(self, n: int) -> "LMSSchedule":
        if n < 1:
            raise ValueError("set_timesteps: at least one step")
        self.timesteps = np.linspace(0, self.num_train_timesteps - 1, n, dtype=float)[::-1].copy()
        s = np.interp(self.timesteps, np.arange(0, len(self.train_sigmas)), self.train_sigmas)
        self.sigmas = np.concatenate([s, [0.0]]).astype(np.float32)   # n + 1 values, descending, the last one 0
        self.init_noise_sigma = float(self.sigmas.max())
        return self

    def __len__(self):
        return len(self.timesteps)

    def input_divisor(self, i: int) -> float:
        """sqrt(sigma_i^2 + 1) in fp32 steps: the U-Net reads x / this."""
        s = np.float32(self.sigmas[i])
        return float(np.sqrt(s * s + np.float32(1.0)))

    def coefficients(self, i: int, order: Optional[int] = None) -> np.ndarray:
        """c_i0 ... c_i(order-1) in float64, newest derivative first."""
        order = min(i + 1, ORDER) if order is None else int(order)
        if not 1 <= order <= min(i + 1, ORDER):
            raise ValueError(f"coefficients: order {order} at step {i}")
        sig = self.sigmas.astype(np.float64)
        h = sig[i + 1] - sig[i]
        nodes = np.array([sig[i - k] - sig[i] for k in range(order)])          # in u = s - sigma_i; nodes[0] = 0
        out = np.empty(order)
        for j in range(order):
            others = np.delete(nodes, j)
            poly = np.poly1d(others, r=True) if len(others) else np.poly1d([1.0])
            out[j] = np.polyint(poly)(h) / np.prod(nodes[j] - others)
        return out


class LMSSampler:
    """The chain of the evaluation script on a LatentDiffusionLite `model`."""

    def __init__(self, model, schedule: Optional[LMSSchedule] = None):
        self.model, self.schedule = model, schedule or LMSSchedule()
        self.last_steps = 0

    @torch.no_grad()
    def sample(self, cond: torch.Tensor, uncond: Optional[torch.Tensor], scale: float, noise: torch.Tensor,
               steps: int, eps_fn=None) -> torch.Tensor:
        """`noise` [B, ...]: standard normal draws; the chain starts at noise * init_noise_sigma.  Guidance (one batched
        pass of 2B rows) when `uncond` is given.  `eps_fn(x_in, t_rows, context)` replaces the U-Net (tests)."""
        sch = self.schedule.set_timesteps(steps)
        B = noise.shape[0]
        guided = uncond is not None
        rows = 2 * B if guided else B
        dev = noise.device
        c_in = torch.cat([uncond, cond]) if guided else cond
        x = (noise.float() * sch.init_noise_sigma).contiguous()
        hist = torch.empty((ORDER,) + tuple(x.shape), dtype=torch.float32, device=dev)
        # a device divisor: an IEEE division as in the kernel (a host scalar would become a product by its reciprocal)
        den0 = torch.full((1,), sch.input_divisor(0), dtype=torch.float32, device=dev)
        x_in = (x / den0).repeat((2 if guided else 1,) + (1,) * (x.dim() - 1)).contiguous()
        model = eps_fn or self.model.apply_model
        self.last_steps = 0
        for i in range(len(sch)):
            t = torch.full((rows,), float(sch.timesteps[i]), dtype=torch.float32, device=dev)
            eps = model(x_in, t, c_in).float().contiguous()
            nxt = torch.empty_like(x_in)
            x = ops_sampler.lms_step(x, eps, scale if guided else 1.0, hist, i % ORDER, sch.coefficients(i),
                                     sch.input_divisor(i + 1), out=x, x_in=nxt)
            x_in = nxt
            self.last_steps += 1
        return x
