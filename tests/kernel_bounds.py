"""Per-element error bounds, guard bands and decisive-key inputs for the kernel parity tests.

A rel-L2 over a whole tensor does not see a wrong tile, a wrong row segment or eight wrong elements (docs/TEST_BOUNDS.md):
here every element is held against a bound of its OWN, derived from the number formats and the operation count of the kernel
-- nothing below is fitted to what a kernel returns.  Everything is evaluated in fp64 on the CPU.

Unit roundoffs (round to nearest even, p significand bits -> u = 2^-p):  bf16 p = 8 -> 2^-8;  fp32 p = 24 -> 2^-24;  e4m3 p = 4 -> 2^-4.
A truncating conversion has 2 u; the bounds allow u for the output rounding, so truncation is rejected.

Plain module: no fixtures, no pytest hooks.  tests/test_kernel_bounds_host.py, tests/test_vae_bounds_host.py and
tests/test_fp8_bounds_host.py check it on the CPU (honest emulations inside, mutants outside); tests/test_gpu_kernel_elementwise.py,
tests/test_gpu_vae_elementwise.py and tests/test_gpu_fp8_elementwise.py use it on the kernels; tests/test_t5_bounds_host.py and
tests/test_gpu_t5_elementwise.py are the same pair for the umT5 text encoder's kernels.
"""
import math

import torch

U_BF16 = 2.0 ** -8
U_F32 = 2.0 ** -24
GELU_SLOPE = 1.13          # max |g'| of the tanh-form GELU is 1.1290 (at x = +1.41), rounded up


def u_of(dtype):
    return {torch.bfloat16: U_BF16, torch.float32: U_F32}[dtype]


def _d(t):
    return torch.as_tensor(t).detach().double().cpu()


# ------------------------------------------------------------------------------------------------ GEMM
def gemm_ref(a, w, bias=None):
    """fp64 product of the (bf16-valued) operands, + bias."""
    acc = _d(a) @ _d(w).t()
    return acc + _d(bias) if bias is not None else acc


def gemm_acc_term(a, w, bias, K):
    """Error of the fp32 accumulator (bias included) before any output rounding:
        2 K 2^-24 |a| @ |w|^T  +  2 2^-24 (|a| @ |w|^T + |bias|).

    * a product of two bf16 numbers has 16 significand bits: exact in fp32, no term;
    * K fp32 additions of those products, in ANY order (MFMA chains, K tiles, the stream-K / split-K combine, which only
      re-associate the same sum), each rounding or truncating (the matrix pipe's internal adds are not documented as RNE, so
      2 u = 2^-23 per addition is allowed):  |err| <= K 2^-23 sum_k |a_k w_k|  (Higham, Accuracy and Stability, eq. 4.4, with
      gamma_K ~ K u; the second-order terms are below 1e-3 of it for K <= 16 384);
    * the bias addition is ONE more addition: 2 u of its operands' magnitude, |acc| + |bias| <= sum_k |a_k w_k| + |bias|.  (Charging
      |bias| K times, as a first version did, is never tighter than this and would hide a bias taken from the wrong column group
      at large |bias| and K.)"""
    mag = _d(a).abs() @ _d(w).abs().t()
    term = 2.0 * K * U_F32 * mag
    if bias is not None:
        term = term + 2.0 * U_F32 * (mag + _d(bias).abs())
    return term


def gemm_bound(a, w, bias, K, out_dtype, ref=None, acc_term=None):
    """EPI_BF16 / EPI_BF16_T / EPI_F32:  u_out |ref| + gemm_acc_term.  The first term is the ONE rounding of the fp32 accumulator
    to the output type (u_out = 2^-8 bf16, 2^-24 fp32, round to nearest even)."""
    ref = gemm_ref(a, w, bias) if ref is None else ref
    acc_term = gemm_acc_term(a, w, bias, K) if acc_term is None else acc_term
    return u_of(out_dtype) * ref.abs() + acc_term


def resid_bound(ref_acc, acc_term, gate_rows, x0):
    """EPI_RESID_F32: out = x0 + (acc + bias) * gate in fp32, read-modify-write.  gate_rows: the gate row of every output row,
    [M, N] or None (gate 1).
    |gate| (2^-24 |acc| + acc_term): the accumulator (its own rounding when bias is added) scaled by the gate;
    2^-24 |acc gate|: the product's rounding (absent when the kernel fuses it into an fma -- allowed either way);
    2^-24 (|x0| + |result|): the add -- operand and result side of one fp32 rounding."""
    ref_acc, x0 = _d(ref_acc), _d(x0)
    g = torch.ones_like(ref_acc) if gate_rows is None else _d(gate_rows)
    result = x0 + ref_acc * g
    bound = g.abs() * (U_F32 * ref_acc.abs() + acc_term) + U_F32 * (ref_acc * g).abs() + U_F32 * (x0.abs() + result.abs())
    return result, bound


_K1 = 2.0 * 0.7978845608028654 * 1.4426950408889634      # |d(exponent)/dx| of the kernel's exp2 argument at x -> 0


def gelu_tanh(x):
    x = _d(x)
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def gelu_bound(ref_x, acc_term):
    """EPI_GELU_BF16: out = bf16(g(acc + bias)), g the tanh form.   2^-8 |g(ref)| + 1.13 acc_term + eval.

    * 2^-8 |g(ref)|: the output rounding;  * 1.13 acc_term: the accumulator error through g (|g'| <= 1.1290);
    * eval -- DERIVED, not measured.  The epilogue (videocof_amd/csrc/common.hpp, gelu_tanh_f32) evaluates g(x) = x / (1 + 2^a),
      a = (k3 x^2 + k1) x, with v_exp_f32 and v_rcp_f32, each documented at 1 ulp (= 2 u relative; CDNA ISA guide, and the
      comment at the function).  Roundings on `a`: the two constants, x*x, the fma, the final multiply -> relative 5 u, taken as 6;
      through 2^a that is a relative error ln2 |a| 6 u of e = 2^a, plus 2 u of v_exp_f32; r = 1 / (1 + e) inherits it damped by
      e / (1 + e) <= 1, plus u (the addition) + 2 u (v_rcp_f32); the product x r adds u:
          eval = 2^-24 |g(ref)| (6 + 6 ln2 |a|)  + 2^-120
      (6 = 2 + 1 + 2 + 1; the absolute floor covers the flush of 2^a below the normal range, where g is ~ x 2^-126)."""
    x = _d(ref_x)
    g = gelu_tanh(x)
    a = (_K1 * (1.0 + 0.044715 * x * x) * x).abs()
    ev = U_F32 * g.abs() * (6.0 + 6.0 * math.log(2.0) * a) + 2.0 ** -120
    return g, U_BF16 * g.abs() + GELU_SLOPE * acc_term + ev


def gelu_from_acc_bound(acc_f32):
    """The second, tighter GELU check: the epilogue's output against g applied to the kernel's OWN fp32 accumulator (the EPI_F32
    result of the same operands, bias, kernel family and plan -- the same MFMA chains in the same order), which takes the K-sized
    accumulation term out of the comparison.  What remains:  2^-8 |g(x)| (output rounding) + eval (as in gelu_bound) +
    1.13 * 2 * 2^-24 |x| -- one fp32 rounding of difference between the two epilogues' bias additions (one may fuse it).
    At K = 384 gelu_bound's accumulation term (~1e-3) exceeds the erf / tanh difference (4.8e-4); this bound does not have it, so an
    erf-form epilogue is rejected at every K.  Returns (g(x), bound)."""
    x = _d(acc_f32)
    g = gelu_tanh(x)
    a = (_K1 * (1.0 + 0.044715 * x * x) * x).abs()
    ev = U_F32 * g.abs() * (6.0 + 6.0 * math.log(2.0) * a) + 2.0 ** -120
    return g, U_BF16 * g.abs() + ev + GELU_SLOPE * 2.0 * U_F32 * x.abs()


# ------------------------------------------------------------------------------------------------ attention
ATTN_C_P = 1.0          # roundings of P to bf16 before P.V (one, round to nearest even), in units of 2^-8 (p @ |v|)


def attention_ref(q, k, v, scale, k_len=None):
    """fp64 softmax(q k^T scale) v for ONE head: q [Lq, D], k / v [Lk, D].  Returns (out, p)."""
    q, k, v = _d(q), _d(k), _d(v)
    if k_len is not None:
        k, v = k[:k_len], v[:k_len]
    p = torch.softmax(q @ k.t() * scale, dim=-1)
    return p @ v, p


def attention_bound(q, k, v, scale, k_len=None):
    """Per element   2^-8 |ref|  +  (c 2^-8 + s_i + f) (p @ |v|),   one head; returns (ref, bound).

    Derived from videocof_amd/csrc/attn_fwd.hip (every form: lazy reference, max-free, persistent, split-KV tail share the arithmetic):
    * out = (sum_j bf16(p_j) v_j) / (sum_j p_j): the kernel rounds P to bf16 (v_cvt_pk_bf16_f32, RNE) for the P.V MFMA and sums
      the row sum l from the UNROUNDED fp32 p.  Numerator error <= 2^-8 sum_j p_j |v_j|, denominator untouched:  c = 1.
      (q is compared at the bf16 value the kernel is given -- pre-scaled or not -- and plain q is scaled in fp32, so the q
      scaling adds no bf16 rounding; there is no second rounding of P.)
    * s_i, the fp32 score error of row i seen through exp2: a score is a 128-term fp32 MFMA sum (<= 128 2^-23 sum_d |q_d k_d|, as
      in gemm_acc_term), one fma with the scale / reference (2 u of |score| + |reference|, both <= max_j |q_i|.|k_j| scale log2e)
      and v_exp_f32 (1 ulp).  With S_i = scale log2(e) max_j sum_d |q_id k_jd| the log2-domain error is d_i <= 2^-23 (130 S_i + 2);
      every p_j moves by a factor within 2^(+-d_i), numerator and denominator both:  s_i = 2 (2^d_i - 1).
    * f, fp32 bookkeeping: Lk additions into O and into l (2 Lk 2^-24 each in the worst order, whichever way the keys are grouped
      into tiles, rescaled partial sums or split-KV partials), one rescale multiply of O and l per 64-key tile at most (the lazy
      reference rescales far less often; its p may exceed 1, which changes no RELATIVE rounding), 1 / l by v_rcp_f32 and the final
      multiply; the split-KV tail merge (attn_combine_kernel, at most 16 partials) puts on every partial one v_exp_f32 (2 u),
      the rounding of m_s - M seen through exp2 (< u) and one multiply (u) -- relative to that partial, not cumulative -- and
      adds them up (16 u): 20 u on the numerator, 20 u on the denominator, 2 u for the division = 42, taken as 64:
      f = 2^-24 (4 Lk + 2 (Lk / 64 + 1) + 4 + 64).
    * 2^-8 |ref|: the output rounding."""
    ref, p, s, f, pv = _attention_parts(q, k, v, scale, k_len)
    return ref, U_BF16 * ref.abs() + (ATTN_C_P * U_BF16 + s + f) * pv


def _attention_parts(q, k, v, scale, k_len=None):
    """(ref, p, s_i [Lq, 1], f, p @ |v|) of attention_bound's docstring, shared with the fp8 forms below."""
    ref, p = attention_ref(q, k, v, scale, k_len)
    qd, kd, vd = _d(q), _d(k), _d(v)
    if k_len is not None:
        kd, vd = kd[:k_len], vd[:k_len]
    Lk = kd.shape[0]
    S = (qd.abs() @ kd.abs().t()).max(dim=-1, keepdim=True).values * scale * 1.4426950408889634
    d = 2.0 ** -23 * (130.0 * S + 2.0)
    s = 2.0 * (torch.exp2(d) - 1.0)
    f = U_F32 * (4.0 * Lk + 2.0 * (Lk / 64.0 + 1.0) + 4.0 + 64.0)
    return ref, p, s, f, p @ vd.abs()


HEAVY = 400.0


def heavy_key(D=128):
    """The key the tests park in the rows of k BEHIND the last valid key (see decisive_qkv): finite, and decisive for every row."""
    hk = torch.zeros(D, dtype=torch.bfloat16)
    hk[0] = HEAVY
    return hk


def decisive_qkv(L, H, seed, mass=(0.5, 0.99), D=128):
    """Inputs in which key i decides query row i: k rows of norm sqrt(D) (random directions), q_i = t_i k_i with the temperature
    t_i bisected on the CPU until the fp64 softmax (scale 1 / sqrt(D)) puts a target share of row i on key i -- targets spread over
    [0.6, 0.95] row by row, inside the admitted (0.5, 0.99); the off-diagonal remainder keeps the P.V accumulation and the rescale
    path busy -- and v_j = small noise + a per-key offset in every channel, so that a dropped, admitted, duplicated or swapped key
    moves its row by O(1).
    Channel 0 is reserved for the guard key: k[.., 0] = 0 and q[.., 0] = 1 for every row, which changes no score among the real
    keys, while ``heavy_key()`` (HEAVY e_0) scores HEAVY / sqrt(D) ~ 35 with EVERY query: admitted by a wrong tail mask it takes all
    the mass of every row.  Returns bf16 q, k, v [L, H, D] and the temperatures [L, H]."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(L, H, D, generator=g, dtype=torch.float64)
    k[..., 0] = 0.0
    k = k / k.norm(dim=-1, keepdim=True) * math.sqrt(D)
    kb = k.to(torch.bfloat16)
    kd = kb.double()
    target = 0.6 + 0.35 * ((torch.arange(L) * 7) % 10).double() / 10.0
    temps = torch.zeros(L, H, dtype=torch.float64)
    q = torch.zeros(L, H, D, dtype=torch.bfloat16)
    for h in range(H):
        gram = kd[:, h] @ kd[:, h].t() / math.sqrt(D)
        lo, hi = torch.zeros(L, dtype=torch.float64), torch.full((L,), 8.0, dtype=torch.float64)
        for _ in range(40):
            t = 0.5 * (lo + hi)
            diag = torch.softmax(gram * t[:, None], dim=-1).diagonal()
            lo = torch.where(diag < target, t, lo)
            hi = torch.where(diag < target, hi, t)
        temps[:, h] = 0.5 * (lo + hi)
        q[:, h] = (kd[:, h] * temps[:, h, None]).to(torch.bfloat16)
        diag = torch.softmax(q[:, h].double() @ kd[:, h].t() / math.sqrt(D), dim=-1).diagonal()
        assert mass[0] <= float(diag.min()) and float(diag.max()) <= mass[1], (L, h, float(diag.min()), float(diag.max()))
    q[..., 0] = 1.0
    j = torch.arange(L, dtype=torch.float64)
    off = torch.stack([torch.sin(0.37 * j + 0.11 * d) + (1.0 if d % 2 else -1.0) * (j % 7) * 0.25 for d in range(D)], dim=-1)
    v = (0.2 * torch.randn(L, H, D, generator=g, dtype=torch.float64) + off[:, None, :]).to(torch.bfloat16)
    return q, kb, v, temps


# ------------------------------------------------------------------------------------------------ row kernels
def ln_modulate_bound(x, scale_rows, shift_rows, add_one, eps):
    """wan_ln_modulate: out = bf16(z a + c), z = (x - mean) rstd, a = add_one + scale, c = shift; x fp32 [rows, dim], a / c given per
    row ([rows, dim]) or None.  Returns (ref, bound):
        2^-8 |ref| + |a| rstd dim u mean|x| + |a z| (dim + 8) u + 4 u (|a z| + |c|),   u = 2^-24
    * the output rounding; * the fp32 mean: dim additions in any order, |d mean| <= dim u mean|x|, scaled by a rstd;
    * rstd from the two-pass sum of squares (videocof_amd/csrc/norm_kernels.hip: mean first, then sum (x - mean)^2): a sum of dim non-negative
      terms, relative error dim u, halved by the square root and doubled again by the rounding of each (x - mean) and its square,
      + division, eps add, v_rsq_f32 (1 ulp): (dim + 8) u relative on z;
    * four elementwise roundings (x - mean, * rstd, * a, + c)."""
    ref, e32 = _ln_modulate_parts(x, scale_rows, shift_rows, add_one, eps)
    return ref, U_BF16 * ref.abs() + e32


def _ln_modulate_parts(x, scale_rows, shift_rows, add_one, eps):
    """(ref, the fp32 part of ln_modulate_bound: everything but the output rounding)."""
    x = _d(x)
    dim = x.shape[-1]
    a = (1.0 if add_one else 0.0) + (_d(scale_rows) if scale_rows is not None else torch.zeros_like(x))
    if scale_rows is None and not add_one:
        a = torch.ones_like(x)
    c = _d(shift_rows) if shift_rows is not None else torch.zeros_like(x)
    mean = x.mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(dim=-1, keepdim=True) + eps)
    z = (x - mean) * rstd
    ref = z * a + c
    az = (a * z).abs()
    e32 = a.abs() * rstd * dim * U_F32 * x.abs().mean(dim=-1, keepdim=True) + az * (dim + 8) * U_F32 + 4 * U_F32 * (az + c.abs())
    return ref, e32


def rmsnorm_rope_bound(x, w, eps, post_scale=1.0, rotate=None, head_dim=128):
    """wan_rmsnorm_rope: y = x rstd w post_scale (rstd over the FULL row), then the pairwise rotation (y[2i], y[2i+1]) by the
    angle of the row, one bf16 rounding.  x bf16-valued [rows, dim]; rotate: None or (cos, sin) fp64 [rows, head_dim / 2] per row
    (the same for every head).  Returns (ref, bound):
        2^-8 |ref| + (dim + 16) u (|y[2i]| + |y[2i+1]|),  u = 2^-24
    * the output rounding; * rstd as in ln_modulate_bound (sum of dim squares, any order): (dim + 8) u relative on y; the three
      multiplies, the fp32 table entries (u each) and the two products + one add of the rotation: 8 u more; |cos|, |sin| <= 1 so
      both elements of a pair are charged with the pair's magnitude."""
    x = _d(x)
    rows, dim = x.shape
    rstd = 1.0 / torch.sqrt((x ** 2).mean(dim=-1, keepdim=True) + eps)
    y = x * rstd * _d(w) * post_scale
    pair = y.view(rows, dim // 2, 2)
    mag = pair.abs().sum(dim=-1, keepdim=True).expand(-1, -1, 2).reshape(rows, dim)
    ref = y
    if rotate is not None:
        cos, sin = (_d(t) for t in rotate)
        yh = y.view(rows, dim // head_dim, head_dim // 2, 2)
        re, im = yh[..., 0], yh[..., 1]
        cr, sr = cos[:, None, :], sin[:, None, :]
        ref = torch.stack([re * cr - im * sr, re * sr + im * cr], dim=-1).reshape(rows, dim)
    return ref, U_BF16 * ref.abs() + (dim + 16) * U_F32 * mag


# ------------------------------------------------------------------------------------------------ VAE convolutions
def conv_cl_im2col(x, hist, kernel, stride, pad, out_thw, upsample2x=False):
    """The A matrix of wan_conv_cl as the ABI defines it (include/wan_hip.h), by plain tensor indexing -- no kernel, no torch conv:
    A[(to, ho, wo), ((kt KH + kh) KW + kw) Cin + ci] = in[to st - pt + kt, ho sh - ph + kh, wo sw - pw + kw, ci], fp64 [M, ntaps Cin].
    x [T, H, W, Cin]; hist [nh, H, W, Cin] or None.  A negative frame index counts back from the END of hist (-1 = its last frame);
    frames before the start of hist and every spatial out-of-range tap are zero.  upsample2x: the tap addresses a virtual 2H x 2W
    plane (the range test is against 2H, 2W) and reads source pixel (hi >> 1, wi >> 1)."""
    x = _d(x)
    T, H, W, C = x.shape
    nh = 0 if hist is None else hist.shape[0]
    frames = torch.cat([_d(hist), x]) if nh else x                       # frame index f = ti + nh
    (KT, KH, KW), (st, sh, sw), (pt, ph, pw) = kernel, stride, pad
    To, Ho, Wo = out_thw
    Hl, Wl = (2 * H, 2 * W) if upsample2x else (H, W)
    to = torch.arange(To).view(To, 1, 1).expand(To, Ho, Wo).reshape(-1)
    ho = torch.arange(Ho).view(1, Ho, 1).expand(To, Ho, Wo).reshape(-1)
    wo = torch.arange(Wo).view(1, 1, Wo).expand(To, Ho, Wo).reshape(-1)
    cols = []
    for kt in range(KT):
        for kh in range(KH):
            for kw in range(KW):
                f, hi, wi = to * st - pt + kt + nh, ho * sh - ph + kh, wo * sw - pw + kw
                ok = (f >= 0) & (f < nh + T) & (hi >= 0) & (hi < Hl) & (wi >= 0) & (wi < Wl)
                hs, ws = (hi >> 1, wi >> 1) if upsample2x else (hi, wi)
                v = frames[f.clamp(0, nh + T - 1), hs.clamp(0, H - 1), ws.clamp(0, W - 1)]          # [M, C]
                cols.append(v * ok[:, None].double())
    return torch.cat(cols, dim=1)


def conv_geometry(mode, T, H, W):
    """(kernel, stride, pad, out_thw, upsample2x, time_interleave) of a wan_conv_cl mode as videocof_amd/wan_vae.py calls it."""
    if mode == "causal":
        return (3, 3, 3), (1, 1, 1), (2, 1, 1), (T, H, W), False, False
    if mode == "1x1":
        return (1, 1, 1), (1, 1, 1), (0, 0, 0), (T, H, W), False, False
    if mode == "down2d":          # ZeroPad2d((0, 1, 0, 1)) + stride 2: the bottom / right tap past the plane reads zero
        return (1, 3, 3), (1, 2, 2), (0, 0, 0), (T, (H - 2) // 2 + 1, (W - 2) // 2 + 1), False, False
    if mode == "up2d":
        return (1, 3, 3), (1, 1, 1), (0, 1, 1), (T, 2 * H, 2 * W), True, False
    if mode == "time":            # upsample3d's time_conv, channel -> time interleave in the store
        return (3, 1, 1), (1, 1, 1), (2, 0, 0), (T, H, W), False, True
    if mode == "down3d":
        return (3, 1, 1), (2, 1, 1), (1, 0, 0), ((T + 1 - 3) // 2 + 1, H, W), False, False
    raise ValueError(mode)


def conv_operands(cin, cout, kernel, T, H, W, nh, seed, resid_shape=None):
    """Operands of one wan_conv_cl test case on the CPU: unit-variance bf16 x [T, H, W, cin] and hist [nh, H, W, cin] (None for
    nh = 0), bf16 weights of variance 1 / K packed [cout, Kpad] in the ABI's K order (kt, kh, kw, ci) with zeros in [K, Kpad), an
    O(1) fp32 bias that differs per column, and a unit-variance bf16 residual of `resid_shape` (or None).  `wt` is the same
    weight as [cout, cin, KT, KH, KW] for torch's convolutions."""
    g = torch.Generator().manual_seed(seed)
    KT, KH, KW = kernel
    K = KT * KH * KW * cin
    Kpad = (K + 63) // 64 * 64
    x = torch.randn(T, H, W, cin, generator=g).to(torch.bfloat16)
    hist = torch.randn(nh, H, W, cin, generator=g).to(torch.bfloat16) if nh else None
    wt = (torch.randn(cout, cin, KT, KH, KW, generator=g) / math.sqrt(K)).to(torch.bfloat16)
    w = torch.zeros(cout, Kpad, dtype=torch.bfloat16)
    w[:, :K] = wt.permute(0, 2, 3, 4, 1).reshape(cout, K)
    bias = torch.randn(cout, generator=g) + 0.37 * torch.arange(cout) / cout
    resid = torch.randn(*resid_shape, generator=g).to(torch.bfloat16) if resid_shape is not None else None
    return dict(x=x, hist=hist, w=w, wt=wt, bias=bias, resid=resid, K=K, Kpad=Kpad)


def time_interleave(conv, out_thw):
    """[M, Cout] conv result -> the time-interleaved rows the kernel stores: out[2 t + half, h, w, c] = conv[t, h, w, half Ch + c]."""
    To, Ho, Wo = out_thw
    Ch = conv.shape[1] // 2
    return conv.view(To, Ho * Wo, 2, Ch).permute(0, 2, 1, 3).reshape(2 * To * Ho * Wo, Ch)


def conv_bound(A, w, bias, resid, K):
    """wan_conv_cl, all three kernels (conv_cl_kernel, conv3_patch_kernel, conv3_head_kernel in videocof_amd/csrc/vae_conv.hip):
    out = bf16(acc + bias (+ resid)), A from conv_cl_im2col, w [Cout, >= K] (only columns < K are used: K padding multiplies exact
    zeros).  Returns (ref, bound), [M, Cout], NOT interleaved (time_interleave() rearranges both):
        u16 |ref| + acc (+ 2 u32 (|acc + bias| + |resid|)),   acc = gemm_acc_term with K = ntaps Cin additions.
    * every kernel accumulates exact bf16 products in fp32 (MFMA chains over taps and channel chunks in three different orders:
      any order is covered), adds the fp32 bias, then the residual -- widened from bf16, exact -- as ONE more fp32 addition, and
      rounds ONCE to bf16, to nearest even: v_cvt_pk_bf16_f32 in the gather and the patch kernel (the patch kernel stages the fp32
      accumulators through LDS unrounded), a __bf16 cast of `acc + bias` in the head kernel.  Read in all three epilogues: none differs."""
    A, wd = _d(A), _d(w)[:, :K]
    ref = gemm_ref(A, wd, bias)
    term = gemm_acc_term(A, wd, bias, K)
    if resid is not None:
        r = _d(resid)
        term = term + 2.0 * U_F32 * (ref.abs() + r.abs())
        ref = ref + r
    return ref, U_BF16 * ref.abs() + term


# ------------------------------------------------------------------------------------------------ VAE row kernels
SILU_SLOPE = 1.1           # max |d/da a sigmoid(a)| = 1.0998 (at a = 2.3994), rounded up


def rmsnorm_silu_bound(x, gamma, silu):
    """wan_rmsnorm_silu_cl: a = x sqrt(C) / max(||x||, 1e-12) gamma per row (F.normalize's eps on the NORM), out = bf16(a) or
    bf16(a / (1 + e^-a)).  x bf16-valued [rows, C].  Returns (ref, bound):
        plain:  u16 |a| + (C + 8) u32 |a|
        SiLU:   u16 |g(a)| + 1.1 (C + 8) u32 |a| + u32 |g(a)| (6 + 2 |a|) + 2^-120
    * the sum of C squares in fp32, per lane 8 fused terms then a shuffle tree: non-negative terms, any order, relative error
      <= C u32, halved by the square root; sqrtf and the division are the correctly rounded expansions (gfx950 code of
      rmsnorm_silu_cl_kernel: v_sqrt_f32 + fma refinement; v_div_scale / v_rcp_f32 / v_div_fmas / v_div_fixup), sqrtf(C) one more
      rounding, two multiplies: (C / 2 + 5) u32, granted as (C + 8) u32 like rmsnorm_rope_bound's rstd;
    * SiLU: the error of `a` through g, |g'| <= 1.0998; the evaluation, from the same code: e = v_exp_f32(-a * log2e) -- the
      constant's and the multiply's rounding are 2 u32 of the argument, through 2^t a relative 2 u32 |a| of e, + 1 ulp = 2 u32 of
      v_exp_f32 (CDNA ISA guide) -- 1 + e one rounding, the division correctly rounded (u32); e's share is damped by e / (1 + e) <= 1:
      relative (2 |a| + 2 + 1 + 1) u32, the constant 4 taken as 6; the absolute floor covers e flushed below the normal range;
    * one rounding to bf16, to nearest even (v_cvt_pk_bf16_f32)."""
    x = _d(x)
    C = x.shape[-1]
    nrm = x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    a = x * math.sqrt(C) / nrm * _d(gamma)
    da = (C + 8) * U_F32 * a.abs()
    if not silu:
        return a, U_BF16 * a.abs() + da
    g = a / (1.0 + torch.exp(-a))
    return g, U_BF16 * g.abs() + SILU_SLOPE * da + U_F32 * g.abs() * (6.0 + 2.0 * a.abs()) + 2.0 ** -120


def softmax_rows_bound(s, n, scale):
    """wan_softmax_rows: p_i = e_i / sum_j e_j, e_i = __expf((s_i - mx) scale), i < n; s fp32 [rows, >= n].  Returns (ref, bound) [rows, n]:
        u16 p_i + p_i u32 (4 x_i + 2 + sum_j p_j (4 x_j + 2) + n + 4) + 2^-120,    x_i = (mx - s_i) scale >= 0
    * the exponent's argument: the subtraction, the multiply by scale, the multiply by the rounded log2(e) = 4 u32 relative on the
      argument, seen through e^x as a relative 4 u32 x_i of e_i (as the attention bound's s_i sees its score error), + v_exp_f32's 1 ulp
      = 2 u32; the max itself is exact;
    * the row sum: n fp32 additions of non-negative terms in any order (256 strided partial sums, a shuffle tree, four wave sums):
      n u32 relative, + the e_j's own errors weighted by their share p_j;
    * 1 / sum (gfx950 code of softmax_rows_kernel: the correctly rounded division expansion; 2 u32 granted so that a bare v_rcp_f32
      would pass as well), the multiply (u32), + 1 spare;  * one rounding to bf16, to nearest even;  * the floor: e_i flushed to zero."""
    sd = _d(s)[:, :n]
    x = (sd.max(dim=-1, keepdim=True).values - sd) * scale
    p = torch.softmax(-x, dim=-1)
    rel = 4.0 * x + 2.0
    row = (p * rel).sum(dim=-1, keepdim=True)
    return p, U_BF16 * p + p * U_F32 * (rel + row + n + 4.0) + 2.0 ** -120


# ------------------------------------------------------------------------------------------------ fp8 (OCP e4m3) kernels
# The fp8 mode is lossy because of the QUANTISATION; on the e4m3 operands a kernel is handed it is as exact as its bf16 sibling, and
# that is what these bounds state.  e4m3fn: 4 significand bits (u = 2^-4), smallest normal 2^-6, subnormal step 2^-9 (half: 2^-10).
FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
U_E4M3 = 2.0 ** -4
SUB_E4M3 = 2.0 ** -10      # half the subnormal step of e4m3, in units of the block / row scale
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453


def dq(q8, row_scale):
    """fp64 value of a row-scaled e4m3 GEMM operand: q8 [rows, K] * row_scale[rows] (exact: 4 x 24 significand bits)."""
    return q8.detach().cpu().float().double() * _d(row_scale)[:, None]


def dq_pow2(q8, exp):
    """fp64 value of an attention operand stored as e4m3(x 2^exp): undoes the power of two exactly."""
    return q8.detach().cpu().float().double() * 2.0 ** -exp


def gemm_fp8_ref_and_term(aq, sa, wq, sw, bias, K):
    """wan_gemm_fp8 / wan_gemm_fp8_ws: acc = (aq @ wq^T) * (sw[n] * sa[m]) (+ bias).  Returns (ref, acc_term) to be used with
    gemm_bound / resid_bound / gelu_bound / gelu_from_acc_bound exactly like the bf16 pair (gemm_ref, gemm_acc_term):
        acc_term = 2 K u32 |a| @ |w|^T + 3 u32 |a @ w^T| (+ 2 u32 (|a| @ |w|^T + |bias|)),   a, w the de-quantised operands
    * the product of two e4m3 numbers has 8 significand bits: exact in fp32, no term;
    * K fp32 additions in any order, each rounding or truncating (gemm_acc_term with the TRUE K): the 128-term sum inside one
      v_mfma_scale_f32_16x16x128_f8f6f4, the chain over K tiles, the two phases of the persistent kernel's schedule P and the
      stream-K combine only re-associate the same sum.  The term scales with the row and column scales like the sum itself, so it
      is evaluated on the de-quantised magnitudes.  (Assumes the matrix pipe's internal adder is at least as wide as an fp32
      truncating add; docs/TEST_BOUNDS.md records what was measured);
    * the scale application acc * (sw[n] * sa[m]): two products, and one more in case the order changes: 3 u32 |acc|;
    * the bias is one more addition, as in gemm_acc_term."""
    a, w = dq(aq, sa), dq(wq, sw)
    acc = a @ w.t()
    mag = a.abs() @ w.abs().t()
    term = 2.0 * K * U_F32 * mag + 3.0 * U_F32 * acc.abs()
    if bias is not None:
        term = term + 2.0 * U_F32 * (mag + _d(bias).abs())
        acc = acc + _d(bias)
    return acc, term


def gemm_fp8_bound(aq, sa, wq, sw, bias, K, out_dtype):
    """EPI_BF16 / EPI_BF16_T / EPI_F32 of the fp8 GEMMs: (ref, u_out |ref| + acc_term of gemm_fp8_ref_and_term)."""
    ref, term = gemm_fp8_ref_and_term(aq, sa, wq, sw, bias, K)
    return ref, gemm_bound(None, None, None, K, out_dtype, ref, term)


def _e4m3_cast(x32):
    """torch's float8_e4m3fn cast (round to nearest even, subnormals kept) of a float32 tensor clamped to the finite range."""
    return x32.clamp(-FP8_MAX, FP8_MAX).to(FP8)


def quantize_rows_fp8_ref(x):
    """EXACT definition of wan_quantize_rows_fp8 (quantize_rows_fp8_kernel, videocof_amd/csrc/norm_kernels.hip) in float32, the
    kernel's own operations in its own order:  amax = max(max|x|, 1e-12);  s = amax * fl(1 / 448);  q = e4m3(clamp(x * fl(448 / amax))).
    x bf16 [rows, cols] -> (codes uint8 [rows, cols], s float32 [rows]).  The only operation that is not a single correctly rounded
    IEEE operation by construction is the division; the build compiles it to the correctly rounded expansion."""
    xf = x.detach().cpu().float()
    amax = xf.abs().amax(dim=1).clamp_min(torch.tensor(1e-12, dtype=torch.float32))
    s = amax * (torch.tensor(1.0, dtype=torch.float32) / torch.tensor(448.0, dtype=torch.float32))
    inv = torch.tensor(448.0, dtype=torch.float32) / amax
    return _e4m3_cast(xf * inv[:, None]).view(torch.uint8), s


MX_POS = [32 * ((key >> 3) & 1) + 16 * (key >> 5) + 8 * ((key >> 4) & 1) + (key & 7) for key in range(64)]


def vt_quantize_mx_ref(vt, H, Lk):
    """EXACT definition of wan_vt_quantize_mx (vt_quantize_mx_kernel, videocof_amd/csrc/attn_fwd.hip).  vt bf16 [B, H * 128, >= pad],
    pad = roundup(Lk, 64).  Per channel row and per MX block of 32 CONSECUTIVE keys (key half kt of a 64-key tile):
        byte = max(biased_exponent(block max) - 7, 1)   (E8M0; an all-zero or denormal block takes the smallest normal scale)
        code = e4m3(v / 2^(byte - 127))                 (block max / scale in [128, 256): nothing saturates)
    stored with the key permutation of the attention kernel's P registers, position 32 hi + 16 kt + 8 g + j <- key 32 kt + 16 g + 8 hi + j
    (MX_POS[key]), and the scale bytes as [B][H][tile][32 kt + (d & 31)][d >> 5].
    Returns (codes uint8 [B, C, pad] in STORED order, scale bytes uint8 [B * H * tiles * 256], de-quantised V^T fp64 [B, C, pad] in
    KEY order)."""
    B, C = vt.shape[:2]
    pad = (Lk + 63) // 64 * 64
    nt = pad // 64
    x = vt.detach().cpu()[:, :, :pad].float().reshape(B, C, nt, 2, 32)
    amax = x.abs().amax(dim=-1)
    ebits = (amax.contiguous().view(torch.int32) >> 23) & 0xFF
    byte = (ebits - 7).clamp_min(1)                                         # [B, C, nt, 2]
    scale = torch.exp2((byte - 127).float())                                # exact powers of two, >= 2^-126
    codes_key = (x / scale[..., None]).to(FP8)                              # division by a power of two
    deq = (codes_key.float().double() * scale.double()[..., None]).reshape(B, C, pad)
    stored = torch.empty(B, C, nt, 64, dtype=torch.uint8)
    stored[..., torch.tensor(MX_POS)] = codes_key.view(torch.uint8).reshape(B, C, nt, 64)
    sc = byte.to(torch.uint8).view(B, H, 4, 32, nt, 2).permute(0, 1, 4, 5, 3, 2).reshape(-1)
    return stored.reshape(B, C, pad), sc.contiguous(), deq


def ln_modulate_fp8_bound(x, scale_rows, shift_rows, add_one, eps):
    """wan_ln_modulate_fp8: y as wan_ln_modulate in fp32 (NOT rounded to bf16), then the row quantiser: amax = max|y|, s = amax fl(1/448),
    q = e4m3(y fl(448 / amax)).  Returns (y_ref, bound on |q s - y_ref| per element, s_ref [rows], tolerance of s [rows]):
        bound = (1 + 2^-4) e32 + 2^-4 |y| + 2^-10 s (1 + 2^-20) + 4 u32 |y|
    * e32: the fp32 part of ln_modulate_bound (no bf16 term: there is no bf16 rounding); the quantiser sees the computed y, so its
      relative rounding applies to |y| + e32;  * 2^-4 |y|: the e4m3 half ulp;  * 2^-10 s: half the subnormal step of the code, times
      the scale (the 2^-20: s may be that much larger than s_ref, see below);
    * the scale's own error: s * fl(448 / amax) = 1 up to three roundings (the constant, the division, the product) and the product
      y * inv rounds once: 4 u32 |y|.  That amax itself is off by up to max e32 changes nothing in q * s: both factors move together.
    * s against s_ref = max|y_ref| / 448: |amax - amax_ref| <= max_c e32 (the fp32 ln term at the row's extreme elements), two
      roundings: tolerance max_c e32 / 448 + 2 u32 s_ref."""
    y, e32 = _ln_modulate_parts(x, scale_rows, shift_rows, add_one, eps)
    s_ref = y.abs().amax(dim=-1) / FP8_MAX
    s_tol = e32.amax(dim=-1) / FP8_MAX + 2.0 * U_F32 * s_ref
    bound = (1.0 + U_E4M3) * e32 + U_E4M3 * y.abs() + SUB_E4M3 * (1.0 + 2.0 ** -20) * s_ref[:, None] + 4.0 * U_F32 * y.abs()
    return y, bound, s_ref, s_tol


def attention_qk8_bound(qd, kd, v, k_len=None):
    """wan_attention_fwd_qk8, one head: attention_bound on the DE-QUANTISED q8 / k8 (dq_pow2) and the bf16 v, scale 1 in the exp2
    domain (q carries softmax_scale log2(e)).  Everything behind the scores is the lazy bf16 form (attn_fwd_w4_kernel<.., QK8 = true>
    shares its softmax and P.V code with the bf16 instantiation): P rounded to bf16 once, the row sum from the unrounded p, c = 1.
    The score: two v_mfma_scale_f32_32x32x64_f8f6f4 (channels 0-63, 64-127) chained through the accumulator = a 128-term sum of
    EXACT products (8 significand bits), the operand scales 2^-q_exp, 2^-k_exp are exponent adjustments -- the same term count as the
    bf16 form's 128-term MFMA chain, so d_i = 2^-23 (130 S_i + 2) is kept.  It stands for the same reason the fp8 GEMM's accumulation
    term does, and with a margin as thin: the fp8 matrix pipe's internal adder is NOT as wide as a truncating fp32 add (measured on the
    16x16x128 form: up to 0.95 x 2^-16 sum |a w| per instruction, docs/TEST_BOUNDS.md), and 128 2^-23 S_i happens to be 2^-16 S_i --
    what 128 truncating fp32 additions are granted is what the pipe's narrower adder needs.  Returns (ref, bound)."""
    return attention_bound(qd, kd, v, LN2, k_len)


def attention_f8_bound(qd, kd, vd, k_len=None):
    """wan_attention_fwd_f8 (max-free attempt), one head, against the fp64 softmax of the de-quantised q8 / k8 with the DE-QUANTISED
    V (vt_quantize_mx_ref).  Read in attn_fwd_f8_kernel: p~_j = exp2(s_j) (no reference subtracted), the row sum l adds the
    UNROUNDED fp32 p~ (sk[] / s1k0.. are summed before the conversion), every 32 consecutive keys form one MX block whose scale is
    2^(floor(log2 sigma_b) - 7), sigma_b the block's fp32 sum; codes e4m3(p~ / scale_b); the V scales are exact powers of two.
        bound = u16 |ref| + (s_i + f) (p @ |v|) + sum_j (2^-4 p_j + 2^-10 scale_b(j) / l) |v_j| + 2^-126 / l sum_j |v_j|
    * the qk8 bound with the P term c u16 (p @ |v|) replaced: each probability carries the e4m3 half ulp 2^-4 relative and half the
      subnormal step 2^-10 scale_b absolute (p~ / scale_b < 256: nothing saturates); scale_b from the REFERENCE's own block sums,
      taken one binade up where sigma_b (1 + s_i + 34 u32) crosses a power of two (the kernel's sum has the score error s_i and 32
      additions);  * s_i and f as in attention_bound (f's rescale allowance is unused here: the max-free form never rescales);
    * the last term: exp2 results below the normal range are flushed (p~ < 2^-126).
    Returns (ref, bound)."""
    ref, p, s, f, pv = _attention_parts(qd, kd, vd, LN2, k_len)
    q, k, v = _d(qd), _d(kd), _d(vd)
    if k_len is not None:
        k, v = k[:k_len], v[:k_len]
    Lk = k.shape[0]
    sc = q @ k.t()                                                          # log2-domain scores
    m = sc.max(dim=-1, keepdim=True).values
    l_rel = torch.exp2(sc - m).sum(dim=-1, keepdim=True)                    # l = l_rel 2^m
    nb = (Lk + 31) // 32
    pp = torch.zeros(q.shape[0], nb * 32, dtype=torch.float64)
    pp[:, :Lk] = p
    sig_rel = pp.view(-1, nb, 32).sum(dim=-1) * (1.0 + s + 34.0 * U_F32)    # sigma_b / l, widened
    # scale_b / l = 2^(floor(log2 sigma_b) - 7) / l  with  log2 sigma_b = log2 sig_rel + log2 l.  Evaluated in the log domain: l = l_rel 2^m
    # and sigma_b are unnormalised max-free quantities spanning 2^+-150 and more, where forming 2^m or sigma_b itself would overflow or
    # underflow; only the RATIO scale_b / l, which is at most 2^-7, is ever exponentiated
    log2_l = m + torch.log2(l_rel)
    e_b = torch.floor(torch.log2(sig_rel.clamp_min(1e-300)) + log2_l)
    scale_rel = torch.exp2(e_b - 7.0 - log2_l)                              # [Lq, nb]
    scale_rel = torch.where(sig_rel > 0, scale_rel, torch.zeros_like(scale_rel))
    va = torch.zeros(nb * 32, v.shape[1], dtype=torch.float64)
    va[:Lk] = v.abs()
    p_term = U_E4M3 * pv + SUB_E4M3 * (scale_rel @ va.view(nb, 32, -1).sum(dim=1))
    flush = torch.exp2(-126.0 - log2_l) * v.abs().sum(dim=0, keepdim=True)
    return ref, U_BF16 * ref.abs() + (s + f) * pv + p_term + flush


def decisive_qkv_e4m3(L, H, seed, q_exp=5, k_exp=2, D=128):
    """decisive_qkv as the fp8 attention kernels receive it: q pre-scaled by softmax_scale log2(e), rounded to bf16, then
    q8 = e4m3(q 2^q_exp), k8 = e4m3(k 2^k_exp).  Asserted here, on the CPU: nothing saturates; the fp64 softmax of the DE-QUANTISED
    operands keeps between 0.5 and 0.99 of row i on key i.
    The guard key (heavy_key() does not carry over: 400 2^k_exp saturates) is a channel-0 pair that is exact in e4m3: every real key has
    k_0 = 0, every query q_0 = 2^(6 - g), the guard key k_0 = 2^g e_0 with g = 8 - k_exp (code 256) -- score 64 in log2 units with EVERY
    query, asserted to exceed every real score of every row by at least 40 and to stay below 100 (exp2 stays finite in the max-free form:
    admitted, the key takes all the mass instead of tripping the redo check).
    Returns dict(q8, k8 [L, H, D] float8, v bf16 [L, H, D], guard float8 [D], qd, kd fp64 de-quantised)."""
    q, k, v, _ = decisive_qkv(L, H, seed, D=D)
    c = D ** -0.5 * LOG2E
    qp = (q.float() * c).to(torch.bfloat16)
    g = 8 - k_exp
    qp[..., 0] = 2.0 ** (6 - g)
    qx, kx = qp.float() * 2.0 ** q_exp, k.float() * 2.0 ** k_exp
    sat = int((qx.abs() > FP8_MAX).sum() + (kx.abs() > FP8_MAX).sum())
    assert sat == 0, (L, H, q_exp, k_exp, sat)
    q8, k8 = qx.to(FP8), kx.to(FP8)
    guard = torch.zeros(D)
    guard[0] = 2.0 ** g * 2.0 ** k_exp
    assert float(guard[0]) <= FP8_MAX
    guard8 = guard.to(FP8)
    qd, kd = dq_pow2(q8, q_exp), dq_pow2(k8, k_exp)
    assert float(qd[..., 0].min()) == float(qd[..., 0].max()) == 2.0 ** (6 - g) and float(kd[..., 0].abs().max()) == 0.0
    gscore = float(qd[0, 0, 0]) * float(guard8.float()[0]) * 2.0 ** -k_exp
    worst_real = -1e30
    for h in range(H):
        sc = qd[:, h] @ kd[:, h].t()
        diag = torch.softmax(sc * LN2, dim=-1).diagonal()
        assert 0.5 < float(diag.min()) and float(diag.max()) < 0.99, (L, h, q_exp, k_exp, float(diag.min()), float(diag.max()))
        worst_real = max(worst_real, float(sc.max()))
    assert gscore >= worst_real + 40.0 and gscore < 100.0, (gscore, worst_real)
    return dict(q8=q8, k8=k8, v=v, guard=guard8, qd=qd, kd=kd, guard_score=gscore, max_real_score=worst_real)


def wide_range_qkv_e4m3(Lq, Lk, seed, q_exp=5, k_exp=2, D=128):
    """One head of e4m3 operands whose exp2-domain scores span 150 binades: channel 1 of every query is 8, channel 1 of key 5 is
    +2.5 (score +20), whole 32-key blocks (every third block from block 1 on) carry -12, -13, -14, -15 or -16 there (scores -96 ... -128:
    in the max-free form their block sums are tiny, denormal or zero -- scale word 0 --, their exponentials flushed), every other key
    0; the remaining channels hold unit-variance noise (scores ~ N(0, 1.44^2)).  Channel 0 is the guard channel of
    decisive_qkv_e4m3.  Returns the same dict."""
    g = torch.Generator().manual_seed(seed)
    c = D ** -0.5 * LOG2E
    qp = (torch.randn(Lq, 1, D, generator=g) * c).to(torch.bfloat16)
    k = torch.randn(Lk, 1, D, generator=g).to(torch.bfloat16)
    gk = 8 - k_exp
    qp[..., 0], k[..., 0] = 2.0 ** (6 - gk), 0.0
    qp[..., 1], k[..., 1] = 8.0, 0.0
    k[5 % Lk, 0, 1] = 2.5
    deep = [-12.0, -13.0, -14.0, -15.0, -16.0]
    for i, b in enumerate(range(1, (Lk + 31) // 32, 3)):
        k[32 * b:32 * b + 32, 0, 1] = deep[i % 5]
    qx, kx = qp.float() * 2.0 ** q_exp, k.float() * 2.0 ** k_exp
    assert int((qx.abs() > FP8_MAX).sum() + (kx.abs() > FP8_MAX).sum()) == 0
    q8, k8 = qx.to(FP8), kx.to(FP8)
    assert torch.equal(q8.float()[..., 1], qx[..., 1]) and torch.equal(k8.float()[..., 1], kx[..., 1])      # exact in e4m3
    j = torch.arange(Lk, dtype=torch.float64)
    off = torch.stack([torch.sin(0.37 * j + 0.11 * d) + (1.0 if d % 2 else -1.0) * (j % 7) * 0.25 for d in range(D)], dim=-1)
    v = (0.2 * torch.randn(Lk, 1, D, generator=g, dtype=torch.float64) + off[:, None, :]).to(torch.bfloat16)
    guard = torch.zeros(D)
    guard[0] = 2.0 ** gk * 2.0 ** k_exp
    return dict(q8=q8, k8=k8, v=v, guard=guard.to(FP8), qd=dq_pow2(q8, q_exp), kd=dq_pow2(k8, k_exp))


def heavy_half_qkv_e4m3(Lq, Lk, seed, q_exp=5, k_exp=2, D=128):
    """One head of e4m3 operands in which the two MX blocks of a 64-key tile differ by 2^20 in mass and the HEAVY block carries no V:
    channel 1 of every query is 8; channel 1 of key 5 (tile 0, key half 0) and of key 104 (tile 1, key half 1) is 2.5 -- score +20 --
    and V is exactly zero over the 32 keys of each of those two blocks; every other key has unit-variance noise scores and random V, so
    the output is carried by blocks that hold about 2^-20 of their tile's mass.  A P scale taken per 64-key tile instead of per
    32-key block turns those probabilities into e4m3 subnormals (or zero) of the tile scale and loses the output of every row, while
    the per-block scale keeps them at full e4m3 precision.  Needs Lk >= 128.  Channel 0 is the guard channel of decisive_qkv_e4m3.
    Returns the same dict."""
    assert Lk >= 128
    g = torch.Generator().manual_seed(seed)
    c = D ** -0.5 * LOG2E
    qp = (torch.randn(Lq, 1, D, generator=g) * c).to(torch.bfloat16)
    k = torch.randn(Lk, 1, D, generator=g).to(torch.bfloat16)
    gk = 8 - k_exp
    qp[..., 0], k[..., 0] = 2.0 ** (6 - gk), 0.0
    qp[..., 1], k[..., 1] = 8.0, 0.0
    k[5, 0, 1] = k[104, 0, 1] = 2.5
    qx, kx = qp.float() * 2.0 ** q_exp, k.float() * 2.0 ** k_exp
    assert int((qx.abs() > FP8_MAX).sum() + (kx.abs() > FP8_MAX).sum()) == 0
    q8, k8 = qx.to(FP8), kx.to(FP8)
    assert torch.equal(q8.float()[..., 1], qx[..., 1]) and torch.equal(k8.float()[..., 1], kx[..., 1])      # exact in e4m3
    v = (torch.randn(Lk, 1, D, generator=g) + torch.linspace(-1, 1, D)).to(torch.bfloat16)
    v[0:32] = 0.0
    v[96:128] = 0.0
    guard = torch.zeros(D)
    guard[0] = 2.0 ** gk * 2.0 ** k_exp
    return dict(q8=q8, k8=k8, v=v, guard=guard.to(FP8), qd=dq_pow2(q8, q_exp), kd=dq_pow2(k8, k_exp))


# ------------------------------------------------------------------------------------------------ umT5 text encoder row kernels
def rmsnorm_rows_bound(x, w, eps, out_dtype):
    """wan_rmsnorm_rows (rmsnorm_rows_kernel<NV, OUT_F32>, videocof_amd/csrc/t5_kernels.hip): out = x rstd w, rstd = rsqrtf(ss / dim + eps),
    x, w fp32, out bf16 (one rounding to nearest even, v_cvt_pk_bf16_f32) or fp32 (none).  Returns (ref, bound), [rows, dim]:
        u_out |ref| (bf16 only)  +  ((dim + 16) u32 + 2^-127 / (mean x² + eps)) |ref|  +  2^-149
    ref: fp64 x / sqrt(mean(x²) + eps) w on the fp32 inputs, eps at the fp32 value the kernel is handed.  Counted on the gfx950 code:
    * ss: dim squares (one rounding each, u32 of a non-negative term) added in fp32 in any order -- per thread over strided float4
      chunks, a 64-lane shuffle tree, 0 + four wave sums -- relative (dim + 1) u32, HALVED by the root;
    * ss / (float)dim is the correctly rounded expansion (v_div_scale / v_rcp_f32 / v_div_fmas / v_div_fixup; (float)dim is exact
      below 2^24), + eps one addition: 2 u32 on the root's argument, halved;
    * rsqrtf is ONE v_rsq_f32 (1 ulp = 2 u32, CDNA ISA guide); an argument below 2^-126 is multiplied by 2^24 first and the result
      by 2^12, both exact;  * two multiplies (v_pk_mul_f32), u32 each:   (dim + 1) / 2 + 1 + 2 + 2 = dim / 2 + 5.5,
      granted as (dim + 16) u32 like rmsnorm_rope_bound's rstd -- the count is smaller at every dim;
    * squares below the normal range (|x| < 2^-63) are denormal (the kernels run with denormals on; a build that flushed them would
      lose at most 2^-126 per square, so at most 2^-126 of the MEAN): relative 2^-127 / (mean + eps) on rstd -- 1e-32 at eps = 1e-6;
    * 2^-149: a result below the normal range lands on the subnormal grid."""
    x, w = _d(x), _d(w)
    dim = x.shape[-1]
    eps32 = float(torch.tensor(float(eps), dtype=torch.float32))
    arg = (x * x).mean(dim=-1, keepdim=True) + eps32
    ref = x / torch.sqrt(arg) * w
    rel = (dim + 16) * U_F32 + 2.0 ** -127 / arg
    out_u = U_BF16 if out_dtype == torch.bfloat16 else 0.0
    return ref, out_u * ref.abs() + rel * ref.abs() + 2.0 ** -149


def t5_bias(table, lut, L):
    """bias[h, i, j] = table[lut[j - i + L - 1], h], fp64 [H, L, L]: the relative position bias as wan_t5_softmax_bias defines it
    (include/wan_hip.h), by plain indexing.  table [num_buckets, H]; lut int [2 L - 1], index = key minus query offset + L - 1."""
    i = torch.arange(L)
    idx = lut.long().cpu()[i[None, :] - i[:, None] + L - 1]                 # [L(i), L(j)]
    return _d(table)[idx].permute(2, 0, 1)


def t5_softmax_bias_bound(s, table, lut, H, k_len):
    """wan_t5_softmax_bias (t5_softmax_bias_kernel): p_j = e_j / sum_j e_j, e_j = __expf(t_j - mx), t_j = fl(s[h, i, j] + bias[h, i, j]),
    over j < k_len; s fp32 [H, L, L].  Returns (ref, bound), [H, L, k_len]; columns [k_len, npad) of the output must be exactly 0.
        u16 p_j + p_j u32 (r_j + sum_k p_k r_k + k_len + 4) + 2^-120,    r_j = |t_j| + 3 x_j + 2,   x_j = mx - t_j >= 0
    softmax_rows_bound with the scale multiply removed and one rounding added, counted on the gfx950 code of the kernel:
    * t_j = s + bias is ONE fp32 addition: an absolute u32 |t_j| on the exponent, seen through e^x as a relative u32 |t_j| of e_j -- in
      the numerator, and weighted by p_k in the row sum.  (The softmax is invariant under the shift by mx, so the maximum's own rounding
      cancels; the maximum of the computed t is found exactly.)
    * __expf(t - mx) is v_sub_f32, v_mul_f32 by the rounded constant 0x3fb8aa3b (log2 e), v_exp_f32 -- no range scaling: the
      subtraction, the constant and the multiply are 3 u32 RELATIVE on the argument, through e^x a relative 3 u32 x_j of e_j; v_exp_f32
      is 1 ulp = 2 u32;
    * the row sum: k_len fp32 additions of non-negative terms in any order (8 strided terms per thread, a 64-lane tree, four wave
      sums): k_len u32, + the terms' own errors weighted by their share;
    * 1.f / sum is the correctly rounded division expansion (u32; 2 u32 granted, so that a bare v_rcp_f32 would pass), the multiply
      u32, + 1 spare: the 4;  * one rounding to bf16, to nearest even (v_cvt_pk_bf16_f32);
    * 2^-120: exponentials below the normal range are flushed by v_exp_f32, and a bf16 result there lands on the subnormal grid."""
    sd = _d(s)
    L = sd.shape[-1]
    t = (sd + t5_bias(table, lut, L))[:, :, :k_len]
    x = t.max(dim=-1, keepdim=True).values - t
    p = torch.softmax(-x, dim=-1)
    r = t.abs() + 3.0 * x + 2.0
    row = (p * r).sum(dim=-1, keepdim=True)
    return p, U_BF16 * p + p * U_F32 * (r + row + k_len + 4.0) + 2.0 ** -120


GUARD_SCORE = 80.0


def t5_softmax_inputs(H, L, k_len, seed, lut, guard=False, num_buckets=32):
    """Scores fp32 [H, L, L] of std 3 and a bias table [num_buckets, H] of std 2 (fp32), checked here on the CPU: at L >= 260 the lut
    uses every bucket an offset can have (all but num_buckets / 2), so no reachable table row goes unread.  guard: the "guard score" input -- real scores are capped at 9 and every score
    BEHIND the mask, s[:, :, k_len:], is +80: a key admitted by a wrong mask (|bias| stays below 12: margin > 45) takes all the mass of
    its row, as heavy_key() does for attention.  On random scores an admitted key among hundreds stays inside every whole-tensor limit."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(H, L, L, generator=g) * 3.0
    table = torch.randn(num_buckets, H, generator=g) * 2.0
    assert lut.numel() == 2 * L - 1 and int(lut.min()) >= 0 and int(lut.max()) < num_buckets
    if L >= 260:
        # bucket num_buckets / 2 is "key behind the query at distance 0", which no offset has: 31 of the 32 buckets can be reached
        reachable = [b for b in range(num_buckets) if b != num_buckets // 2]
        assert sorted(set(lut.tolist())) == reachable, "the lut must reach every bucket an offset can have"
    if guard:
        s.clamp_(max=9.0)
        s[:, :, k_len:] = GUARD_SCORE
        assert float(s[:, :, :k_len].max()) < 10.0 and float(table.abs().max()) < 12.0
    return s, table


# ------------------------------------------------------------------------------------------------ comparison
def _ranges(idx):
    return [(int(idx[:, d].min()), int(idx[:, d].max())) for d in range(idx.shape[1])]


def assert_within(out, ref, bound, what):
    """Every element of `out` within `bound` of `ref` (NaN / inf in `out` violate).  A failure names the COUNT of violating
    elements, the worst ratio and the index ranges they fall in -- "rows 2944-2999, cols 1160-1163" names the tile.  Returns the
    worst |err| / bound (a result to record, never a limit: the limit is 1)."""
    o, r, b = _d(out), _d(ref), _d(bound)
    assert o.shape == r.shape == b.shape, (what, o.shape, r.shape, b.shape)
    err = (o - r).abs()
    ok = err <= b                                     # False for NaN
    ratio = torch.where(torch.isfinite(err), err / b.clamp_min(1e-300), torch.full_like(err, float("inf")))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if bool(ok.all()):
        return worst
    bad = (~ok).nonzero()
    names = ["rows", "cols"] if o.dim() == 2 else [f"dim{d}" for d in range(o.dim() - 2)] + ["rows", "cols"]
    where = ", ".join(f"{n} {lo}-{hi}" for n, (lo, hi) in zip(names, _ranges(bad)))
    first = tuple(int(i) for i in bad[0])
    raise AssertionError(f"{what}: {bad.shape[0]} of {o.numel()} elements outside the bound ({where}); worst |err|/bound = {worst:.3g}; "
                         f"first at {first}: got {float(o[first])!r}, reference {float(r[first])!r}, bound {float(b[first]):.3g}")


# ------------------------------------------------------------------------------------------------ guard bands
POISON16 = 0x7FC1        # as bf16: a NaN; twice in a row (0x7FC17FC1) as fp32: a NaN too
POISON8 = 0x7F           # as e4m3fn: a NaN (S.1111.111); the bytes of 0x7FC1 are not both NaN in e4m3 (0xC1 = -2.25)


class Guarded:
    """A [rows, cols] (or [batch, rows, cols]) tensor handed out as the strided interior of a larger buffer that is filled
    with a poison bit pattern (NaN in bf16 and fp32 alike -- 0x7F bytes, a NaN in e4m3fn, for the one-byte types -- so it doubles as
    input poison): `rows_before` / `rows_after` guard rows
    per batch entry, `cols_before` columns left of and `ld - cols_before - cols` columns right of every row.  ``view`` is the
    interior; ``check()`` asserts that every byte outside it still holds the pattern."""

    def __init__(self, shape, dtype, ld=None, rows_before=2, rows_after=2, cols_before=0, device="cpu", poison=None):
        self.batched = len(shape) == 3
        B, rows, cols = shape if self.batched else (1,) + tuple(shape)
        self.esize = torch.empty((), dtype=dtype).element_size()
        assert self.esize in (1, 2, 4)
        ld = cols_before + cols if ld is None else ld
        assert ld >= cols_before + cols
        self.B, self.rows, self.cols, self.ld, self.rb, self.c0 = B, rows, cols, ld, rows_before, cols_before
        # the buffer is held in `unit`s: bytes for the one-byte types (poison 0x7F: NaN as e4m3fn), 16-bit words otherwise
        unit = torch.uint8 if self.esize == 1 else torch.int16
        poison = (POISON8 if self.esize == 1 else POISON16) if poison is None else poison
        self.poison = poison - 0x10000 if poison >= 0x8000 else poison
        per16 = max(1, self.esize // 2)
        self.raw = torch.full((B, rows_before + rows + rows_after, ld * per16), self.poison, dtype=unit, device=device)
        typed = self.raw.view(dtype)                                        # [B, R, ld]
        v = typed[:, rows_before:rows_before + rows, cols_before:cols_before + cols]
        self.view = v if self.batched else v[0]
        self._per16 = per16
        self._unit = "bytes" if self.esize == 1 else "16-bit words"

    def fill(self, t):
        self.view.copy_(t)
        return self.view

    def check(self, what="guard band"):
        """Only the four border slabs are read (no copy of the interior)."""
        r0, r1 = self.rb, self.rb + self.rows
        c0, c1 = self.c0 * self._per16, (self.c0 + self.cols) * self._per16
        slabs = ((self.raw[:, :r0], 0, 0), (self.raw[:, r1:], r1, 0), (self.raw[:, r0:r1, :c0], r0, 0), (self.raw[:, r0:r1, c1:], r0, c1))
        bad = [(t != self.poison).nonzero().cpu() + torch.tensor([0, dr, dc]) for t, dr, dc in slabs if t.numel()]
        bad = torch.cat(bad) if bad else torch.zeros(0, 3, dtype=torch.long)
        if bad.shape[0]:
            b, r, c = (int(i) for i in bad[0])
            (b0, b1), (r0_, r1_), (c0_, c1_) = _ranges(bad)
            raise AssertionError(f"{what}: {bad.shape[0]} {self._unit} outside the tensor were written: batch {b0}-{b1}, rows "
                                 f"{r0_ - self.rb}-{r1_ - self.rb} of {self.rows}, cols {c0_ // self._per16 - self.c0}-"
                                 f"{c1_ // self._per16 - self.c0} of {self.cols} (first: batch {b}, row {r - self.rb}, col "
                                 f"{c // self._per16 - self.c0})")
