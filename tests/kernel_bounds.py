"""Per-element error bounds, guard bands and decisive-key inputs for the kernel parity tests.

A rel-L2 over a whole tensor does not see a wrong tile, a wrong row segment or eight wrong elements (docs/TEST_BOUNDS.md):
here every element is held against a bound of its OWN, derived from the number formats and the operation count of the kernel
-- nothing below is fitted to what a kernel returns.  Everything is evaluated in fp64 on the CPU.

Unit roundoffs (round to nearest even, p significand bits -> u = 2^-p):  bf16 p = 8 -> 2^-8;  fp32 p = 24 -> 2^-24.
A truncating conversion has 2 u; the bounds allow u for the output rounding, so truncation is rejected.

Plain module: no fixtures, no pytest hooks.  tests/test_kernel_bounds_host.py checks it on the CPU (honest emulations inside,
mutants outside); tests/test_gpu_kernel_elementwise.py and tests/test_gpu_vae_elementwise.py use it on the kernels.
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
    ref, p = attention_ref(q, k, v, scale, k_len)
    qd, kd, vd = _d(q), _d(k), _d(v)
    if k_len is not None:
        kd, vd = kd[:k_len], vd[:k_len]
    Lk = kd.shape[0]
    S = (qd.abs() @ kd.abs().t()).max(dim=-1, keepdim=True).values * scale * 1.4426950408889634
    d = 2.0 ** -23 * (130.0 * S + 2.0)
    s = 2.0 * (torch.exp2(d) - 1.0)
    f = U_F32 * (4.0 * Lk + 2.0 * (Lk / 64.0 + 1.0) + 4.0 + 64.0)
    return ref, U_BF16 * ref.abs() + (ATTN_C_P * U_BF16 + s + f) * (p @ vd.abs())


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
    bound = (U_BF16 * ref.abs() + a.abs() * rstd * dim * U_F32 * x.abs().mean(dim=-1, keepdim=True)
             + az * (dim + 8) * U_F32 + 4 * U_F32 * (az + c.abs()))
    return ref, bound


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


class Guarded:
    """A [rows, cols] (or [batch, rows, cols]) tensor handed out as the strided interior of a larger buffer that is filled
    with a poison bit pattern (NaN in bf16 and fp32 alike, so it doubles as input poison): `rows_before` / `rows_after` guard rows
    per batch entry, `cols_before` columns left of and `ld - cols_before - cols` columns right of every row.  ``view`` is the
    interior; ``check()`` asserts that every byte outside it still holds the pattern."""

    def __init__(self, shape, dtype, ld=None, rows_before=2, rows_after=2, cols_before=0, device="cpu", poison=POISON16):
        self.batched = len(shape) == 3
        B, rows, cols = shape if self.batched else (1,) + tuple(shape)
        self.esize = torch.empty((), dtype=dtype).element_size()
        assert self.esize in (2, 4)
        ld = cols_before + cols if ld is None else ld
        assert ld >= cols_before + cols
        self.B, self.rows, self.cols, self.ld, self.rb, self.c0 = B, rows, cols, ld, rows_before, cols_before
        self.poison = poison - 0x10000 if poison >= 0x8000 else poison
        per16 = self.esize // 2
        self.raw = torch.full((B, rows_before + rows + rows_after, ld * per16), self.poison, dtype=torch.int16, device=device)
        typed = self.raw.view(dtype)                                        # [B, R, ld]
        v = typed[:, rows_before:rows_before + rows, cols_before:cols_before + cols]
        self.view = v if self.batched else v[0]
        self._per16 = per16

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
            raise AssertionError(f"{what}: {bad.shape[0]} 16-bit words outside the tensor were written: batch {b0}-{b1}, rows "
                                 f"{r0_ - self.rb}-{r1_ - self.rb} of {self.rows}, cols {c0_ // self._per16 - self.c0}-"
                                 f"{c1_ // self._per16 - self.c0} of {self.cols} (first: batch {b}, row {r - self.rb}, col "
                                 f"{c // self._per16 - self.c0})")
