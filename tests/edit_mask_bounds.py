"""The one bound of the edit-mask tests (docs/TEST_BOUNDS.md, "Edit inside a mask"), shared by tests/test_edit_mask_host.py and
tests/test_gpu_edit_mask.py.

Where the mask is 0 the step's prediction is v' = round((x_t - s) / sigma) and both samplers form x0 = x_t - sigma * v'.  With
D = x_t - s, M = max(|x_t|, |s|) (so |D| <= 2 M) and u the unit roundoff of the tensors' dtype, the roundings between D and x0 are

    d  = round(x_t - s)          an error of at most |D| u  <= 2 M u
    v' = round(d / sigma)                                   <= 2 M u     (float32, then the dtype: counted once, in the dtype)
    t  = round(sigma * v')                                  <= 2 M u     (absent where the sampler fuses it into the subtraction)
    x0 = round(x_t - t)          half an ulp of the result, which is s to a few ulps: <= 0.5 ulp(M)

to first order (the second-order terms are below 2^-7 of these in bf16, 2^-23 in float32).  M u < ulp(M) because M < 2^(e + 1) where
ulp(M) = 2^(e + 1 - p): three terms below 2 ulps each and one of half an ulp, 6.5, stated as 7.  The device samplers accumulate in
float32 and round to the dtype once, so in bf16 they spend about 2.5 of them; the count above is what holds for every path, the host
schedulers' dtype-by-dtype arithmetic included.  The last step of both samplers (sigma_next = 0) returns x0 itself (coefficients
exactly 0 and 1), so the bound on x0 is the bound on the loop's result."""
import torch

ZERO_MASK_ULPS = 7
PRECISION = {torch.float32: 24, torch.bfloat16: 8}          # significand bits, the hidden one included


def ulp_of(m: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The spacing of `dtype` at magnitude `m` (float64): 2^(e - p) for m = f * 2^e, f in [0.5, 1)."""
    _, e = torch.frexp(m.double().abs())
    return torch.ldexp(torch.ones_like(m, dtype=torch.float64), e - PRECISION[dtype])


def zero_mask_excess(target: torch.Tensor, source: torch.Tensor, x_t: torch.Tensor) -> float:
    """max over the elements of |target - source| / ulp(max(|x_t|, |source|)), in ulps of the tensors' dtype: `target` = the loop's
    result where the mask is 0, `source` = the source block of the same state, `x_t` = the target entering the last step."""
    dtype = target.dtype
    target, source, x_t = (t.detach().cpu().double() for t in (target, source, x_t))
    m = torch.maximum(x_t.abs(), source.abs())
    err = (target - source).abs()
    live = m > 0                                             # (m == 0: x_t = s = 0 and every operation above is exact)
    assert bool((err[~live] == 0).all())
    return float((err[live] / ulp_of(m[live], dtype)).max()) if bool(live.any()) else 0.0
