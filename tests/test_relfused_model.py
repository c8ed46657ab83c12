"""The launch sequence of csrc/relation.hip restated in float32 torch and held to the bound the GPU tests use (_attn_model.relation_bounds),
before a GPU sees the kernels: fp32 Grams, base-2 fp32 log-sum-exps, S_unit = coef (P_s + P_s^T - P_t - P_t^T) rounded to bf16 once WITHOUT the
upstream factor, an fp32 product S_unit F_s, the upstream factor in fp32, one bf16 rounding of d.  The bound must admit that sequence and
reject its obvious fault (S without its transposed half).

The second mutation the design note asks for -- S rounded to bf16 both before and after the upstream factor, bf16(bf16(S_unit) up) -- cannot
be told from the correct form by this bound, and is therefore measured and printed here, not asserted: the second rounding adds at most
u |S||F| to an error whose budget is u (|S||F| + |dF|) + ..., and the first rounding's error is a sum of ~200 independent terms that stays far
below its worst case u |S||F|, so the doubly rounded form sits inside the bound too (worst ratios below).  Nothing is loosened for it."""
import math

import pytest
import torch

import _attn_model as A

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
LOG2E = 1.4426950408889634


def fused_emulate(fs, ft, weight, hd_s, hd_t, mutate=None):
    """fs [B][N][Ds], ft [B][N][Dt] float64 holding 16-bit values -> d as the two launches round it (float64 holding bf16 values).
    mutate: None | "half" (S = G, the transposed half lost) | "twice" (bf16(bf16(S_unit) up) in front of the product)."""
    B = fs.shape[0]

    def soft2(f, hd):           # the scaled Gram and its row log-sum-exp in the base-2 domain, fp32
        R = (f.to(F32) @ f.to(F32).transpose(1, 2)) * torch.tensor(LOG2E / math.sqrt(hd), dtype=F32)
        m = R.max(-1, keepdim=True).values
        return R, (m + torch.log2(torch.exp2(R - m).sum(-1, keepdim=True))).squeeze(-1)

    (rs, ls), (rt, lt) = soft2(fs, hd_s), soft2(ft, hd_t)
    coef = torch.tensor(1.0 / (B * math.sqrt(hd_s)), dtype=F32)
    up = torch.tensor(float(weight), dtype=F32)
    if mutate == "half":
        S = (torch.exp2(rs - ls[:, :, None]) - torch.exp2(rt - lt[:, :, None])) * coef
    else:
        S = (torch.exp2(rs - ls[:, :, None]) + torch.exp2(rs - ls[:, None, :]) - torch.exp2(rt - lt[:, :, None])
             - torch.exp2(rt - lt[:, None, :])) * coef
    S16 = S.to(BF16)
    if mutate == "twice":
        return ((S16.to(F32) * up).to(BF16).to(F64) @ fs).to(F32).to(BF16).to(F64)
    return ((S16.to(F64) @ fs).to(F32) * up).to(BF16).to(F64)


def features(B, N, Ds, Dt, std):
    def rnd(shape, seed):
        g = torch.Generator(device="cpu").manual_seed(seed)
        return (torch.randn(shape, generator=g) * std).to(BF16)
    return rnd((B * N, 3 * Ds), 1), rnd((B * N, 3 * Dt), 2)


@pytest.mark.parametrize("std", [0.25, 1.0])
@pytest.mark.parametrize("Ds,Dt", [(128, 256), (384, 768)])
def test_fused_sequence_inside_relation_bounds(std, Ds, Dt):
    B, N = 3, 198
    s, t = features(B, N, Ds, Dt, std)
    for j, w in enumerate((0.2 / 12, 0.1 / 12, -0.3 / 12)):       # (one negative upstream: the bound is even in the weight)
        fs = s[:, j * Ds:(j + 1) * Ds].double().view(B, N, Ds)
        ft = t[:, j * Dt:(j + 1) * Dt].double().view(B, N, Dt)
        want, bound, _ = A.relation_bounds(fs, ft, w, 64, 64)
        good = A.ratio(fused_emulate(fs, ft, w, 64, 64), want, bound)
        half = A.ratio(fused_emulate(fs, ft, w, 64, 64, "half"), want, bound)
        twice = A.ratio(fused_emulate(fs, ft, w, 64, 64, "twice"), want, bound)
        old = A.ratio(A.relation_emulate(fs, ft, w, 64, 64), want, bound)
        print(f"std {std} widths {Ds}/{Dt} block {j}: fused {good:.3f}  unfused {old:.3f}  S without S^T {half:.3f}  rounded twice {twice:.3f} (not asserted)")
        assert good < 1.0, (std, j, good)
        if float(want.abs().max()) > 1e-6 * abs(w):
            assert half > 1.0, (std, j, half)
        else:           # unit-scale features 384 / 768 wide: R_ii ~ 48 and 96 above the rest of the row, both softmaxes ARE the identity in fp32 and the
            assert std == 1.0 and Ds == 384, (std, Ds, j)       # gradient is ~1e-10 of its weight: no fault of S can show on this input, only this one
