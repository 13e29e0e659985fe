"""DDIM sampling of latents with the SD U-Net: the slice of the reference's `DDIMSampler`
(SD/ldm/models/diffusion/ddim.py:43-110 make_schedule, :177-282 ddim_sampling, :284-374 p_sample_ddim) that the ESD
script uses — uniform discretisation, classifier-free guidance, `x_T` given, the chain stopped early by `till_T`.

One reverse step is ONE batched U-Net pass over cat([x, x]) / cat([uncond, cond]) and ONE launch of
`salun_ldm_ddim_step` (K21, csrc/salun_sampler.hip), which reads the two halves of the U-Net output in place.  The
tables are computed the way the reference computes them — from the fp32 `alphas_cumprod` through numpy — and live on
the sampler object; `LatentDiffusionLite` gets no new buffer (its state_dict is what the scripts save).  The five
coefficients of a step are fp32 host scalars in the reference's operation order; the kernel recomputes none.

Not reproduced: the reference draws a `randn` of the latent's shape on every step even when `ddim_eta = 0` and
multiplies it by sigma = 0 (ddim.py:369); here the noise term is skipped then, and no generator state is consumed.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .. import ops_sampler


def make_ddim_timesteps(num_ddim_timesteps: int, num_ddpm_timesteps: int) -> np.ndarray:
    """The "uniform" method of ldm/modules/diffusionmodules/util.py:56-76: arange(0, T, T // S) + 1."""
    c = num_ddpm_timesteps // num_ddim_timesteps
    return np.asarray(list(range(0, num_ddpm_timesteps, c))) + 1


def make_ddim_sampling_parameters(alphacums: np.ndarray, ddim_timesteps: np.ndarray, eta: float):
    """util.py:79-96 on the fp32 `alphas_cumprod`: -> (sigmas f64, alphas f32, alphas_prev f64 holding fp32 values).
    The reference's `alphas` stays an fp32 tensor and its `alphas_prev` becomes a float64 array of the same fp32
    values (`.tolist()`); sigma is evaluated in float64 from them (0 for the eta = 0 of every script here)."""
    alphacums = np.asarray(alphacums, np.float32)
    alphas = alphacums[ddim_timesteps]
    alphas_prev = np.asarray([alphacums[0]] + alphacums[ddim_timesteps[:-1]].tolist(), np.float64)
    a = alphas.astype(np.float64)
    sigmas = eta * np.sqrt((1 - alphas_prev) / (1 - a) * (1 - a / alphas_prev))
    return sigmas, alphas, alphas_prev


class DDIMSampler:
    def __init__(self, model):
        self.model = model
        self.ddpm_num_timesteps = int(model.num_timesteps)
        self.last_steps = 0   # U-Net passes of the last sample() call
        self._t_rows = {}

    def make_schedule(self, ddim_num_steps: int, ddim_eta: float = 0.0):
        T = self.ddpm_num_timesteps
        self.ddim_timesteps = make_ddim_timesteps(ddim_num_steps, T)
        ac = np.asarray(self.model.alphas_cumprod_f32, np.float32)
        assert ac.shape[0] == T, "alphas have to be defined for each timestep"
        self.ddim_sigmas, self.ddim_alphas, self.ddim_alphas_prev = make_ddim_sampling_parameters(
            ac, self.ddim_timesteps, ddim_eta)
        self.ddim_sqrt_one_minus_alphas = np.sqrt(np.float32(1.0) - self.ddim_alphas)
        self.ddim_eta = float(ddim_eta)
        self._t_rows = {}
        return self

    def coefficients(self, index: int):
        """(c_s1m, c_sqrt_at, c_dir, c_sqrt_aprev, c_sigma) of p_sample_ddim at `index`, each an fp32 value computed in
        numpy float32 in the reference's order (ddim.py:352-372: the table entries become fp32 `torch.full` tensors)."""
        one = np.float32(1.0)
        a_t = np.float32(self.ddim_alphas[index])
        a_prev = np.float32(self.ddim_alphas_prev[index])
        sigma = np.float32(self.ddim_sigmas[index])
        c_s1m = np.float32(self.ddim_sqrt_one_minus_alphas[index])
        c_sqrt_at = np.sqrt(a_t)
        c_dir = np.sqrt((one - a_prev) - sigma * sigma)
        c_sqrt_aprev = np.sqrt(a_prev)
        return float(c_s1m), float(c_sqrt_at), float(c_dir), float(c_sqrt_aprev), float(sigma)

    def _timestep_rows(self, rows: int, device) -> torch.Tensor:
        key = (rows, str(device))
        t = self._t_rows.get(key)
        if t is None:   # (steps, rows) int64: row i is the `ts` of chain position i, for the batched pass
            steps = np.flip(self.ddim_timesteps[:-1]).astype(np.int64)
            t = torch.from_numpy(np.repeat(steps[:, None], rows, axis=1).copy()).to(device)
            self._t_rows[key] = t
        return t

    @torch.no_grad()
    def sample(self, cond: torch.Tensor, uncond: Optional[torch.Tensor], scale: float, x_T: torch.Tensor,
               till_T: Optional[int] = None) -> torch.Tensor:
        """The chain from `x_T` as ddim_sampling runs it for the ESD script (ddim.py:226-282):

          * `timesteps = ddim_timesteps[:t_start]` with the script's `t_start = -1`: the LAST (noisiest) of the S DDIM
            timesteps is dropped, so the chain has S - 1 positions and starts at index S - 2;
          * the exit rule `if index + 1 == till: break` is checked AFTER the step: `till_T = k >= 1` takes S - k steps,
            `till_T` 0 or None never matches and runs all S - 1.

        Guidance (one batched pass of 2B rows) when `uncond` is given and `scale != 1`, as ddim.py:303.  With
        `ddim_eta != 0` a step draws its z like the reference (`randn` of the latent's shape on the device).
        `last_steps` counts the U-Net passes taken."""
        total = int(self.ddim_timesteps[:-1].shape[0])
        till = till_T if till_T is not None else 0
        B = x_T.shape[0]
        guided = uncond is not None and scale != 1.0
        rows = 2 * B if guided else B
        ts = self._timestep_rows(rows, x_T.device)
        c_in = torch.cat([uncond, cond]) if guided else cond
        x = x_T.contiguous().float()
        self.last_steps = 0
        for i in range(total):
            index = total - i - 1
            x_in = torch.cat([x, x]) if guided else x
            eps = self.model.apply_model(x_in, ts[i], c_in)
            c_s1m, c_sqrt_at, c_dir, c_sqrt_aprev, c_sigma = self.coefficients(index)
            z = torch.randn_like(x) if c_sigma != 0.0 else None
            # (a new tensor on the first step only: x_T stays the caller's)
            x = ops_sampler.ldm_ddim_step(x, eps.contiguous(), scale if guided else 1.0, c_s1m, c_sqrt_at, c_dir,
                                          c_sqrt_aprev, c_sigma, z, out=None if i == 0 else x)
            self.last_steps += 1
            if index + 1 == till:
                break
        return x
