"""Flow-matching DPM-Solver++ multistep sampler (host PyTorch + one fused HIP pass per step).

Same contract as ``FlowDPMSolverMultistepScheduler`` of ``videox_fun/utils/fm_solvers.py`` (diffusers ``SchedulerMixin``
style), with ``get_sampling_sigmas`` (:22-26) and ``retrieve_timesteps`` (:29-66): the constructor's arguments and defaults
(:129-147, every one of them in ``.config``, by key and by attribute; ``solver_type`` logrho / bh1 / bh2 -> midpoint and
``algorithm_type`` deis -> dpmsolver++ as there, :157-168), ``set_timesteps(num_inference_steps, device, sigmas, mu, shift)``,
``.timesteps`` (int64, truncated), ``.sigmas`` (float32, on the host), ``order = 1``, ``step(model_output, timestep, sample,
generator, variance_noise, return_dict)``, ``scale_model_input``, ``add_noise``, ``index_for_timestep`` (a timestep that occurs
twice resolves to its second position), ``set_begin_index``, ``step_index`` / ``begin_index``, ``len()``.

Supported: ``algorithm_type`` ``dpmsolver++`` and ``sde-dpmsolver++``; ``solver_order`` 1, 2, 3; ``solver_type`` midpoint and
heun; ``lower_order_final`` (lower orders at the last two steps when there are fewer than 15, :746-752); ``euler_at_final``;
``final_sigmas_type="zero"``; ``variance_noise``.  SDE noise is drawn as the reference's ``randn_tensor`` draws it: the model
output's shape, fp32, on the generator's device, then moved -- at every step, the last one included, so a seeded generator
ends in the reference's state.

Refused (with the reason):

- what the reference cannot run: ``final_sigmas_type="sigma_min"`` (its ``set_timesteps`` reads an ``alphas_cumprod`` the
  class never defines, :261-263) and therefore the deprecated ``dpmsolver`` / ``sde-dpmsolver`` types, which need it
  (:170-174) -- ``NotImplementedError``;
- what this path never builds: ``thresholding``, ``use_dynamic_shifting`` (``NotImplementedError``), a ``prediction_type``
  other than ``flow_prediction`` and a ``solver_order`` outside 1..3 (``ValueError``);
- ``sde-dpmsolver++`` at a step that needs the third-order update: the reference's third-order update has no SDE branch and
  ends in ``UnboundLocalError`` (:666-677); here ``NotImplementedError``, raised at the same step (the earlier steps run).

Own formulation: every update is a linear combination of {sample, v (the model output), m1, m2 (the two earlier x0
predictions), noise}.  The scalar algebra (:449-677) runs once per step on the host in float64 and takes LIMITS where the
reference relies on IEEE infinities: sigma_s = 1 at the first step (lambda = -inf, h = inf, exp(-h) = 0), sigma_t = 0 at the
last step, and r = inf for a history term that reaches back to sigma = 1 (its divided difference vanishes).  On the device
the whole step -- the x0 prediction stored in the latent dtype (the history entry) and the fp32 update from it -- is ONE
``wan_solver_step`` launch (include/wan_hip.h); CPU tensors take the torch path, the one the CPU tests pin to the reference.
"""
from __future__ import annotations

import inspect
import math
from typing import List, Optional, Union

import numpy as np
import torch

__all__ = ["FlowDPMSolverMultistepScheduler", "get_sampling_sigmas", "retrieve_timesteps"]


def get_sampling_sigmas(sampling_steps, shift):
    """fm_solvers.py:22-26: ``sampling_steps`` sigmas from 1 (inclusive) toward 0 (exclusive), shifted."""
    sigma = np.linspace(1, 0, sampling_steps + 1)[:sampling_steps]
    return shift * sigma / (1 + (shift - 1) * sigma)


def retrieve_timesteps(scheduler, num_inference_steps=None, device=None, timesteps=None, sigmas=None, **kwargs):
    """fm_solvers.py:29-66: ``scheduler.set_timesteps`` with custom ``timesteps`` or ``sigmas`` (if its ``set_timesteps`` takes
    them) or a step count; returns ``(scheduler.timesteps, number of steps)``."""
    if timesteps is not None and sigmas is not None:
        raise ValueError("Only one of `timesteps` or `sigmas` can be passed. Please choose one to set custom values")
    if timesteps is not None:
        if "timesteps" not in set(inspect.signature(scheduler.set_timesteps).parameters.keys()):
            raise ValueError(f"The current scheduler class {scheduler.__class__}'s `set_timesteps` does not support custom"
                             f" timestep schedules. Please check whether you are using the correct scheduler.")
        scheduler.set_timesteps(timesteps=timesteps, device=device, **kwargs)
        timesteps = scheduler.timesteps
        num_inference_steps = len(timesteps)
    elif sigmas is not None:
        if "sigmas" not in set(inspect.signature(scheduler.set_timesteps).parameters.keys()):
            raise ValueError(f"The current scheduler class {scheduler.__class__}'s `set_timesteps` does not support custom"
                             f" sigmas schedules. Please check whether you are using the correct scheduler.")
        scheduler.set_timesteps(sigmas=sigmas, device=device, **kwargs)
        timesteps = scheduler.timesteps
        num_inference_steps = len(timesteps)
    else:
        scheduler.set_timesteps(num_inference_steps, device=device, **kwargs)
        timesteps = scheduler.timesteps
    return timesteps, num_inference_steps


class SchedulerOutput:
    def __init__(self, prev_sample):
        self.prev_sample = prev_sample


class _Config(dict):
    """The constructor arguments, readable as attributes and as keys (diffusers' FrozenDict, without the freezing machinery)."""
    __getattr__ = dict.__getitem__


def _lam(sigma: float) -> float:
    """lambda = log(alpha) - log(sigma) with alpha = 1 - sigma (:461-462); -inf at sigma = 1, +inf at sigma = 0."""
    if sigma <= 0.0:
        return math.inf
    return math.log1p(-sigma) - math.log(sigma) if sigma < 1.0 else -math.inf


def _inv_ratio(h: float, h_k: float) -> float:
    """1 / r for r = h_k / h: 0 when h_k is infinite (the history term reaches back to sigma = 1)."""
    return 0.0 if math.isinf(h_k) else h / h_k


def _randn_like_reference(shape, generator, device) -> torch.Tensor:
    """diffusers' ``randn_tensor(shape, generator=, device=, dtype=float32)`` as fm_solvers.py:763-767 calls it: drawn on the
    generator's device (CPU generator -> CPU draw), one generator per batch entry for a list, then moved to ``device``."""
    device = torch.device(device)
    rand_device = device
    if generator is not None:
        gdev = (generator[0] if isinstance(generator, (list, tuple)) else generator).device
        if gdev.type != device.type and gdev.type == "cpu":
            rand_device = torch.device("cpu")
        elif gdev.type != device.type:
            raise ValueError(f"Cannot generate a {device} tensor from a generator of type {gdev.type}.")
    if isinstance(generator, (list, tuple)) and len(generator) == 1:
        generator = generator[0]
    if isinstance(generator, (list, tuple)):
        one = (1,) + tuple(shape[1:])
        draws = [torch.randn(one, generator=generator[b], device=rand_device, dtype=torch.float32) for b in range(shape[0])]
        return torch.cat(draws, dim=0).to(device)
    return torch.randn(tuple(shape), generator=generator, device=rand_device, dtype=torch.float32).to(device)


class FlowDPMSolverMultistepScheduler:
    order = 1

    @classmethod
    def from_config(cls, config, **kwargs):
        """diffusers' ``SchedulerMixin.from_config``: a scheduler from another one's ``.config`` (or a plain dict), keyword overrides on
        top; entries the constructor does not take are ignored (a ``FlowUniPCMultistepScheduler.config`` works: its ``bh2`` maps
        to midpoint, as in the reference)."""
        names = set(inspect.signature(cls.__init__).parameters) - {"self"}
        cfg = {k: v for k, v in dict(config).items() if k in names}
        cfg.update({k: v for k, v in kwargs.items() if k in names})
        return cls(**cfg)

    def __init__(self, num_train_timesteps: int = 1000, solver_order: int = 2, prediction_type: str = "flow_prediction",
                 shift: Optional[float] = 1.0, use_dynamic_shifting=False, thresholding: bool = False,
                 dynamic_thresholding_ratio: float = 0.995, sample_max_value: float = 1.0, algorithm_type: str = "dpmsolver++",
                 solver_type: str = "midpoint", lower_order_final: bool = True, euler_at_final: bool = False,
                 final_sigmas_type: Optional[str] = "zero", lambda_min_clipped: float = -math.inf,
                 variance_type: Optional[str] = None, invert_sigmas: bool = False):
        if algorithm_type == "deis":
            algorithm_type = "dpmsolver++"                                                   # :157-158
        if algorithm_type not in ("dpmsolver", "dpmsolver++", "sde-dpmsolver", "sde-dpmsolver++"):
            raise NotImplementedError(f"{algorithm_type} is not implemented for {self.__class__}")    # :159-161
        if solver_type in ("logrho", "bh1", "bh2"):
            solver_type = "midpoint"                                                         # :164-165
        if solver_type not in ("midpoint", "heun"):
            raise NotImplementedError(f"{solver_type} is not implemented for {self.__class__}")       # :166-168
        if algorithm_type in ("dpmsolver", "sde-dpmsolver"):
            if final_sigmas_type == "zero":                                                  # :170-174
                raise ValueError(f"`final_sigmas_type` {final_sigmas_type} is not supported for `algorithm_type` {algorithm_type}. "
                                 "Please choose `sigma_min` instead.")
            raise NotImplementedError(f"algorithm_type {algorithm_type!r} needs final_sigmas_type='sigma_min', which the reference "
                                      "cannot run (set_timesteps reads an undefined alphas_cumprod)")
        if final_sigmas_type == "sigma_min":
            raise NotImplementedError("final_sigmas_type='sigma_min': the reference cannot run it (set_timesteps reads an undefined "
                                      "alphas_cumprod); use 'zero'")
        if final_sigmas_type != "zero":
            raise ValueError(f"`final_sigmas_type` must be one of 'zero', or 'sigma_min', but got {final_sigmas_type}")
        if prediction_type != "flow_prediction":
            raise ValueError(f"prediction_type given as {prediction_type} must be `flow_prediction` for the "
                             "FlowDPMSolverMultistepScheduler")
        if thresholding or use_dynamic_shifting:
            raise NotImplementedError("thresholding / use_dynamic_shifting are not on the VideoCoF path")
        if int(solver_order) not in (1, 2, 3):
            raise ValueError(f"solver_order={solver_order}: the DPMSolver order can be 1, 2 or 3")
        # what diffusers' @register_to_config would hold: EVERY constructor argument (after the remapping), by attribute and by key
        self.config = _Config(
            num_train_timesteps=num_train_timesteps, solver_order=int(solver_order), prediction_type=prediction_type, shift=shift,
            use_dynamic_shifting=use_dynamic_shifting, thresholding=thresholding,
            dynamic_thresholding_ratio=dynamic_thresholding_ratio, sample_max_value=sample_max_value,
            algorithm_type=algorithm_type, solver_type=solver_type, lower_order_final=lower_order_final,
            euler_at_final=euler_at_final, final_sigmas_type=final_sigmas_type, lambda_min_clipped=lambda_min_clipped,
            variance_type=variance_type, invert_sigmas=invert_sigmas)
        alphas = np.linspace(1, 1 / num_train_timesteps, num_train_timesteps)[::-1].copy()
        sig = torch.from_numpy(1.0 - alphas).to(torch.float32)
        sig = shift * sig / (1 + (shift - 1) * sig)                                          # :183-187
        self.sigmas = sig
        self.timesteps = sig * num_train_timesteps
        self.sigma_min, self.sigma_max = self.sigmas[-1].item(), self.sigmas[0].item()
        self.num_inference_steps = None
        self._reset()

    def _reset(self):
        """Back to the state after set_timesteps: empty history, no step / begin index."""
        self.model_outputs: List[Optional[torch.Tensor]] = [None] * self.config.solver_order
        self.lower_order_nums = 0
        self._step_index = None
        self._begin_index = None

    @property
    def step_index(self):
        return self._step_index

    @property
    def begin_index(self):
        return self._begin_index

    def set_begin_index(self, begin_index: int = 0):
        self._begin_index = begin_index

    def set_timesteps(self, num_inference_steps: Union[int, None] = None, device: Union[str, torch.device] = None,
                      sigmas: Optional[List[float]] = None, mu: Optional[Union[float, None]] = None,
                      shift: Optional[Union[float, None]] = None):
        """:226-290: ``sigmas`` (default: ``num_inference_steps`` of linspace(sigma_max, sigma_min)) shifted by ``shift`` (default:
        the config's), timesteps = int64(sigmas * num_train_timesteps), and a final sigma of 0."""
        if sigmas is None:
            sigmas = np.linspace(self.sigma_max, self.sigma_min, num_inference_steps + 1).copy()[:-1]
        sigmas = np.asarray(sigmas, dtype=np.float64)
        if shift is None:
            shift = self.config.shift
        sigmas = shift * sigmas / (1 + (shift - 1) * sigmas)
        timesteps = sigmas * self.config.num_train_timesteps
        self.sigmas = torch.from_numpy(np.concatenate([sigmas, [0.0]]).astype(np.float32))   # stays on the host
        self.timesteps = torch.from_numpy(timesteps).to(device=device, dtype=torch.int64)    # truncation
        self.num_inference_steps = len(timesteps)
        self._reset()

    def scale_model_input(self, sample: torch.Tensor, *args, **kwargs) -> torch.Tensor:
        return sample

    def index_for_timestep(self, timestep, schedule_timesteps=None):
        """:679-691: a timestep that occurs twice resolves to its SECOND position."""
        idx = ((self.timesteps if schedule_timesteps is None else schedule_timesteps) == timestep).nonzero()
        return idx[1 if len(idx) > 1 else 0].item()

    def __len__(self):
        return self.config.num_train_timesteps

    def add_noise(self, original_samples: torch.Tensor, noise: torch.Tensor, timesteps: torch.IntTensor) -> torch.Tensor:
        """:815-854: (1 - sigma) x0 + sigma noise with sigma looked up per sample -- by timestep before a loop has a begin index,
        else at the current (or the begin) step."""
        sigmas = self.sigmas.to(device=original_samples.device, dtype=original_samples.dtype)
        ts = timesteps.to(original_samples.device)
        if self._begin_index is None:
            sched = self.timesteps.to(original_samples.device)
            idx = [self.index_for_timestep(t, sched) for t in ts]
        else:
            idx = [self._step_index if self._step_index is not None else self._begin_index] * ts.shape[0]
        sigma = sigmas[idx].flatten()
        sigma = sigma.view(-1, *([1] * (original_samples.dim() - 1)))
        return (1 - sigma) * original_samples + sigma * noise

    # ------------------------------------------------------------------ scalar algebra (float64, host)
    def _coeffs(self, i: int, order: int):
        """(c_s, c_0, c_1, c_2, c_n): prev = c_s*sample + c_0*m0 + c_1*m1 + c_2*m2 + c_n*noise for the step from sigma[i] to
        sigma[i+1], m0 = this step's x0 prediction, m1 / m2 the earlier ones.  dpm_solver_first_order_update (:454-483),
        multistep_dpm_solver_second_order_update (:528-593) and multistep_dpm_solver_third_order_update (:640-677), with the
        divided differences D1 / D2 expanded into the m_k."""
        s = self.sigmas.double()
        sig = lambda k: s[k].item()
        sigma_t, sigma_s0 = sig(i + 1), sig(i)
        alpha_t = 1.0 - sigma_t
        lam_t, lam_s0 = _lam(sigma_t), _lam(sigma_s0)
        h = lam_t - lam_s0                                           # > 0; inf at sigma_s0 = 1 or sigma_t = 0
        em1 = math.expm1(-h)                                         # exp(-h) - 1  (-1 at h = inf)
        e = em1 + 1.0
        sde = self.config.algorithm_type == "sde-dpmsolver++"
        heun = self.config.solver_type == "heun"
        c_s = sigma_t / sigma_s0
        c1 = c2 = 0.0
        if sde:
            one_m_e2 = -math.expm1(-2.0 * h)                         # 1 - exp(-2h)
            c_s *= e
            A = alpha_t * one_m_e2
            c_n = sigma_t * math.sqrt(one_m_e2)
            # heun: alpha_t * ((1 - exp(-2h)) / (-2h) + 1); the quotient is 0 at h = inf
            B = 0.5 * A if not heun else alpha_t * (1.0 - (one_m_e2 / (2.0 * h) if math.isfinite(h) else 0.0))
        else:
            A = -alpha_t * em1
            c_n = 0.0
            B = 0.5 * A if not heun else alpha_t * ((em1 / h if math.isfinite(h) else 0.0) + 1.0)
        c0 = A
        if order == 1:
            return c_s, c0, c1, c2, c_n
        lam_s1 = _lam(sig(i - 1))
        a = _inv_ratio(h, lam_s0 - lam_s1)                           # 1 / r0
        if order == 2:
            # D1 = (m0 - m1) / r0; midpoint: + B D1 with B = A / 2 (:550-553, :570-574); heun: + B D1 (:554-557, :575-580)
            return c_s, c0 + B * a, -B * a, 0.0, c_n
        # order 3 (dpmsolver++ only)
        lam_s2 = _lam(sig(i - 2))
        h1 = lam_s1 - lam_s2
        b = _inv_ratio(h, h1)                                        # 1 / r1
        r0 = 1.0 / a
        if math.isinf(h1):
            w = z = 0.0                                              # r1 = inf: r0 / (r0 + r1) = 1 / (r0 + r1) = 0
        else:
            r1 = h1 / h
            w, z = r0 / (r0 + r1), 1.0 / (r0 + r1)
        B3 = alpha_t * (em1 / h + 1.0)
        C3 = alpha_t * ((em1 + h) / (h * h) - 0.5)
        # D1 = (1 + w) a (m0 - m1) - w b (m1 - m2);  D2 = z (a (m0 - m1) - b (m1 - m2));  prev = ... + B3 D1 - C3 D2 (:667-671)
        c0 = A + B3 * (1.0 + w) * a - C3 * z * a
        c1 = -B3 * ((1.0 + w) * a + w * b) + C3 * z * (a + b)
        c2 = B3 * w * b - C3 * z * b
        return c_s, c0, c1, c2, c_n

    # ------------------------------------------------------------------ step
    def step(self, model_output: torch.Tensor, timestep: Union[int, torch.Tensor], sample: torch.Tensor, generator=None,
             variance_noise: Optional[torch.Tensor] = None, return_dict: bool = True):
        """:706-796.  One ``wan_solver_step`` launch for CUDA tensors; the torch path for CPU tensors."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if self._step_index is None:
            self._step_index = self._begin_index if self._begin_index is not None else self.index_for_timestep(
                timestep.to(self.timesteps.device) if torch.is_tensor(timestep) else timestep)
        i, n = self._step_index, len(self.timesteps)
        cfg = self.config
        lower_order_final = i == n - 1 and (cfg.euler_at_final or (cfg.lower_order_final and n < 15)
                                            or cfg.final_sigmas_type == "zero")              # :746-749
        lower_order_second = i == n - 2 and cfg.lower_order_final and n < 15                 # :750-752
        if cfg.solver_order == 1 or self.lower_order_nums < 1 or lower_order_final:
            order = 1
        elif cfg.solver_order == 2 or self.lower_order_nums < 2 or lower_order_second:
            order = 2
        else:
            order = 3
        sde = cfg.algorithm_type == "sde-dpmsolver++"
        noise = None
        if sde:
            if variance_noise is None:
                noise = _randn_like_reference(model_output.shape, generator, model_output.device)
            else:
                noise = variance_noise.to(device=model_output.device, dtype=torch.float32)
        sigma = float(self.sigmas[i])
        hist = self.model_outputs
        if sde and order == 3:
            # (the noise is drawn first, as the reference draws it before its third-order update fails, :760-787)
            raise NotImplementedError(f"sde-dpmsolver++ with solver_order=3 needs the third-order update at step {i}, which has no "
                                      "SDE form (the reference ends in UnboundLocalError there); use solver_order <= 2")
        c_s, c0, c1, c2, c_n = self._coeffs(i, order)
        m1 = hist[-1] if order >= 2 else None
        m2 = hist[-2] if order >= 3 else None
        xdt = torch.promote_types(sample.dtype, model_output.dtype)
        if sample.is_cuda:
            from . import ops                          # the whole step in one pass (wan_solver_step)
            x0, prev = ops.solver_step(sample.to(xdt), model_output.to(xdt), 1.0, -sigma, m1, m2, noise,
                                       c_s, c0, c1, c2, c_n)
        else:
            x0 = sample - torch.tensor(sigma, dtype=torch.float32) * model_output              # convert_model_output (:381-383)
            prev = sample.float() * c_s
            for c, t in ((c0, x0), (c1, m1), (c2, m2), (c_n, noise)):
                if t is not None:
                    prev.add_(t.float(), alpha=c)
        self.model_outputs = hist[1:] + [x0]
        if self.lower_order_nums < cfg.solver_order:
            self.lower_order_nums += 1
        prev_sample = prev.to(model_output.dtype)                                             # :789
        self._step_index += 1
        if not return_dict:
            return (prev_sample,)
        return SchedulerOutput(prev_sample=prev_sample)
