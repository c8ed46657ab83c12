"""cal_hid_relation_loss (utils/losses.py:295-304) on the 16-bit path: a float64 restatement with its analytic backward, and a per-element first-order
error model of the kernel sequence (csrc/hid.hip + the batched MFMA GEMMs), derived from the inputs alone -- no factor is fitted to what a GPU gave.

The sequence and where it rounds (u = 2^-8: bf16 unit roundoff, v = 2^-24: fp32's):
    inv  = 1 / max(|h|, 1e-12)                fp32: a sum of D squares (at most D/64 in one lane + 6 tree levels), sqrt, divide
    h^   = bf16(h * inv)                      ONE bf16 rounding per element                                       -> e_h = (u + e_inv + 2v) |h^|
    G    = h^ h^T per image                   exact bf16 x bf16 products, fp32 accumulation over D in the MFMA    -> e_G = E A^T + A E^T (+ E E^T) + D 2^-23 A A^T
    loss = sum (G_s - G_t)^2 / (B N^2 L)      fp32; the subtraction cancels, its error does not: e_d = e_Gs + e_Gt
    S    = bf16(c (G_s - G_t)), c = 4 up / (B N^2 L)      ONE bf16 rounding of the fp32 value                     -> e_S = c e_d + u |S| + ...
    dh^  = S h^ per image                     fp32 accumulation over the 256-wide window                          -> e_dh^ = e_S A + |S| E + 256 2^-23 |S| A
    dh   = inv (dh^ - h^ (h^ . dh^))          fp32
with A = |h^| and E = e_h.  MFMA accumulation is charged one ulp (2^-23) per added product: the instruction's internal rounding is not stated to be
round-to-nearest.  Every bound is absolute and per element, so a cancelling G_s - G_t (rows with a common offset: all Gram entries near 1) is covered.

`emulate` is an honest CPU emulation of that sequence (and, with a switch, of a lower-precision variant that the bounds must NOT hold)."""
import math

import torch

from _tail_model import ratio  # noqa: F401  (worst |got - ref| / bound over every element; callers use it as HM.ratio)
from oracle.detgen import det_array

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
V = 2.0 ** -24           # fp32 unit roundoff
U = 2.0 ** -8            # bf16 unit roundoff
EPS = 1e-12
TINY = 2.0 ** -126

# (B, N, Ds, Dt) of the GPU test: one token; a small odd-ish batch; N = 51 (a 112-pixel model), three images, the widest teacher; 197 / 198 (224 pixels,
# one and two tokens: Gram windows of 256 rows that reach into the next image and the zeroed overhang); 208, the most the kernels take
CASES = [(1, 1, 64, 64), (2, 6, 384, 768), (3, 51, 384, 1024), (2, 197, 384, 768), (2, 198, 384, 768), (1, 208, 384, 768)]
REGIMES = ("unit", "offset", "scaled", "zero_row", "same")


def inputs(B, N, Ds, Dt, regime):
    """(student fp32 [B, N, Ds], teacher fp32 [B, N, Dt]) of a regime:
    unit      unit-scale random rows
    offset    the same rows + 30: every normalised row is close to the all-ones direction, every Gram entry close to 1, G_s - G_t cancels
    scaled    rows multiplied by 1e-3 (even) and 1e3 (odd): the loss does not depend on a row's scale
    zero_row  one all-zero student row (and another teacher row): h^ = 0, inv = 1e12
    same      teacher == student (Dt = Ds): loss and gradient are exactly 0"""
    tag = f"hid/{regime}/{B}x{N}"
    s = torch.from_numpy(det_array(tag + f"/s{Ds}", (B, N, Ds)))
    t = torch.from_numpy(det_array(tag + f"/t{Dt}", (B, N, Dt)))
    if regime == "offset":
        s, t = s + 30.0, t + 30.0
    elif regime == "scaled":
        sc = torch.where(torch.arange(N) % 2 == 0, torch.tensor(1e-3), torch.tensor(1e3)).view(1, N, 1)
        s, t = s * sc, t * sc.flip(1)
    elif regime == "zero_row":
        s, t = s.clone(), t.clone()
        s[0, N // 2] = 0.0
        t[B - 1, 0] = 0.0
    elif regime == "same":
        t = s.clone()
    return s.contiguous(), t.contiguous()


def golden_inputs():
    """the two layer pairs of tests/golden/hid_relation.npz: B = 2, N = 7, student width 64, teacher width 128"""
    stu = [torch.from_numpy(det_array(f"hid/golden/s{i}", (2, 7, 64))) for i in range(2)]
    tea = [torch.from_numpy(det_array(f"hid/golden/t{i}", (2, 7, 128))) for i in range(2)]
    return stu, tea


# ------------------------------------------------------------------------------------------------ float64 restatement
def autograd_loss(stu, tea):
    """the definition, in torch ops of any dtype: rows x / max(|x|, 1e-12), Grams per image, mean squared difference, mean over the pairs"""
    total = 0.
    for s, t in zip(stu, tea):
        sn = s / s.norm(dim=-1, keepdim=True).clamp_min(EPS)
        tn = t / t.norm(dim=-1, keepdim=True).clamp_min(EPS)
        total = total + ((sn @ sn.transpose(-1, -2) - tn @ tn.transpose(-1, -2)) ** 2).mean()
    return total / len(stu)


def restate(s, t, layers=1, upstream=1.0):
    """float64 values of everything the kernels produce for one pair, backward analytic:
    dh^ = (4 up / (B N^2 L)) (G_s - G_t) h^_s;  dh = inv (dh^ - h^ (h^ . dh^))"""
    s, t = s.to(F64), t.to(F64)
    B, N, _ = s.shape
    inv_s = 1.0 / s.norm(dim=-1).clamp_min(EPS)
    inv_t = 1.0 / t.norm(dim=-1).clamp_min(EPS)
    hs, ht = s * inv_s[..., None], t * inv_t[..., None]
    gs, gt = hs @ hs.transpose(1, 2), ht @ ht.transpose(1, 2)
    d = gs - gt
    loss = (d * d).sum() / (B * N * N * layers)
    c = 4.0 * upstream / (B * N * N * layers)
    S = c * d
    dhn = S @ hs
    p = (hs * dhn).sum(-1, keepdim=True)
    dh = inv_s[..., None] * (dhn - hs * p)
    return dict(hs=hs, ht=ht, inv_s=inv_s, inv_t=inv_t, gs=gs, gt=gt, d=d, loss=loss, S=S, dhn=dhn, p=p, dh=dh, c=c)


def cal(stu, tea):
    """float64 (loss, [student gradients]) of the list form, through restate()"""
    L = len(stu)
    parts = [restate(s, t, L) for s, t in zip(stu, tea)]
    return sum(p["loss"] for p in parts), [p["dh"] for p in parts]


# ------------------------------------------------------------------------------------------------ the error model
def _norm_err(r, which, D):
    """(relative error of inv, E = per-element bound of h^) of one side"""
    e_inv = (D / 64 + 10) * V            # (D/64 + 6 adds + the squares' roundings) / 2 under the root, sqrt, divide, eps as an fp32 constant: an upper bound
    A = r["h" + which].abs()
    return e_inv, A * (U + e_inv + 2 * V) + TINY, A


def _gram_err(E, A, D):
    Ah = A + E
    return E @ A.transpose(1, 2) + A @ E.transpose(1, 2) + E @ E.transpose(1, 2) + D * 2.0 ** -23 * (Ah @ Ah.transpose(1, 2))


def bounds(s, t, layers=1, upstream=1.0):
    """(restate(...), per-element bounds of `hs`, `inv_s`, `loss`, `S`, `dh`) for the bf16 path"""
    r = restate(s, t, layers, upstream)
    B, N, Ds = s.shape
    Dt = t.shape[2]
    ei_s, Es, As = _norm_err(r, "s", Ds)
    ei_t, Et, At = _norm_err(r, "t", Dt)
    e_gs, e_gt = _gram_err(Es, As, Ds), _gram_err(Et, At, Dt)
    d = r["d"].abs()
    e_d = (e_gs + e_gt) * (1 + V) + V * d
    # loss: every term (d + e)^2, then a sum whose values pass through at most k additions (4 in a lane, 6 + 6 tree levels, ceil(B N / 8192) + 3 in a
    # thread, 16 at the end) and the final scale
    k = 4 + 6 + 6 + math.ceil(B * N / 8192) + 3 + 16 + 2
    sq = (d + e_d) ** 2
    e_loss = ((2 * d * e_d + e_d * e_d + V * sq).sum() + k * V * sq.sum()) / (B * N * N * layers)
    # S: upstream * coef (2 roundings), the difference's, the product's; then ONE bf16 rounding
    c = abs(r["c"])
    e_s32 = c * (e_gs + e_gt) + 4 * V * c * (d + e_gs + e_gt)
    e_S = e_s32 + U * (r["S"].abs() + e_s32) + TINY
    # dh^ = S h^: fp32 accumulation over the 256-wide window
    Ah, Sa = As + Es, r["S"].abs()
    e_dhn = e_S @ Ah + Sa @ Es + 256 * 2.0 ** -23 * ((Sa + e_S) @ Ah)
    dhn, p = r["dhn"].abs(), r["p"].abs()
    e_p = (Es * dhn + Ah * e_dhn).sum(-1, keepdim=True) + (Ds / 64 + 7) * V * (Ah * (dhn + e_dhn)).sum(-1, keepdim=True)
    inv = r["inv_s"][..., None]
    e_dh = inv * (e_dhn + Es * p + Ah * e_p + 3 * V * (dhn + e_dhn + Ah * (p + e_p))) + ei_s * inv * (dhn + As * p) + TINY
    return r, dict(hs=Es, inv_s=r["inv_s"] * ei_s, loss=e_loss, S=e_S, dh=e_dh)


# ------------------------------------------------------------------------------------------------ CPU emulations
def _bf16_accumulated_gram(h):
    """h^ h^T with the running sum kept in bf16 (every addition rounded to 8 bits): NOT what the kernels do"""
    acc = torch.zeros(h.shape[0], h.shape[1], h.shape[1], dtype=BF16)
    hf = h.to(F32)
    for k in range(h.shape[2]):
        acc = (acc.to(F32) + hf[:, :, k, None] * hf[:, None, :, k]).to(BF16)
    return acc.to(F32)


def emulate(s, t, layers=1, upstream=1.0, variant="kernel"):
    """The kernel sequence in torch on the CPU: fp32 arithmetic, h^ and S rounded once to bf16.  variant "gram_bf16": the Grams accumulated in bf16,
    an honest lower-precision form."""
    s, t = s.to(F32), t.to(F32)
    B, N, _ = s.shape

    def norm(x):
        inv = 1.0 / x.pow(2).sum(-1).sqrt().clamp_min(torch.tensor(EPS, dtype=F32))
        return (x * inv[..., None]).to(BF16), inv
    hs, inv_s = norm(s)
    ht, _ = norm(t)
    if variant == "gram_bf16":
        gs, gt = _bf16_accumulated_gram(hs), _bf16_accumulated_gram(ht)
    else:
        gs, gt = hs.to(F32) @ hs.to(F32).transpose(1, 2), ht.to(F32) @ ht.to(F32).transpose(1, 2)
    d = gs - gt
    loss = (d * d).sum() * torch.tensor(1.0 / (B * N * N * layers), dtype=F32)
    c = torch.tensor(upstream, dtype=F32) * torch.tensor(4.0 / (B * N * N * layers), dtype=F32)
    S = (d * c).to(BF16)
    dhn = S.to(F32) @ hs.to(F32)
    p = (hs.to(F32) * dhn).sum(-1, keepdim=True)
    dh = (dhn - hs.to(F32) * p) * inv_s[..., None]
    return dict(hs=hs, inv_s=inv_s, loss=loss, S=S, dh=dh)


# ------------------------------------------------------------------------------------------------ the injection kernel
def inject_cases():
    """(M, D, rows_per_scale or 0): M not a multiple of the 256-row padding, with and without a row scale; one whole multiple"""
    return [(18, 384, 6), (18, 384, 0), (396, 384, 198), (512, 128, 0), (255, 64, 51)]
