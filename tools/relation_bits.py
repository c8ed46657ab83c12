#!/usr/bin/env python3
"""The bits of the relation-loss entry points on seeded inputs: one line per (entry point, case) with the sha256 of every output buffer's bytes.  Two
libraries compute the same thing when the two files are equal: run once per library (DEVIT_LIB_PATH names the one to load, devit_amd/_lib.py), each
run its own process, and `cmp` the files.  Inputs are made on the CPU from a seeded generator; every output buffer is zeroed before the call, so an
element the kernels leave alone hashes the same in both runs.
  devit_relation_fused_fwd / _bwd : the losses, lse_t, lse_s, row_kl, the whole S, d[:B N]; bf16 and f16 teacher
  devit_qkv_pair_fwd / _bwd       : the loss, terms, the whole S, d[:B N]; both layouts, both cross values, bf16 and f16 teacher
  devit_relation_stats, devit_hid_stats, devit_soft_ce_rows_fwd : the row terms and the loss scalar (B = 48 takes the reduce round its loop twice)
usage: relation_bits.py OUT.txt"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from devit_amd import ops  # noqa: E402
from devit_amd._lib import ptr, stream_ptr  # noqa: E402

dev = torch.device("cuda")
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
REL_CASES = ((1, 5, 64, 64), (2, 17, 128, 256), (3, 198, 384, 768), (2, 208, 384, 768))          # B, N, student width, teacher width
QKV_CASES = ((1, 5, 128, 192), (2, 17, 128, 256), (3, 198, 384, 768), (2, 208, 384, 768))
lines = []


def rand(gen, shape, dtype, std):
    return (torch.randn(shape, generator=gen, dtype=F32) * std).to(dtype).to(dev)


def zeros(shape, dtype=F32):
    return torch.zeros(shape, dtype=dtype, device=dev)


def sha(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def report(entry, case, **bufs):
    torch.cuda.synchronize()
    lines.append(f"{entry} {case} " + " ".join(f"{k}={sha(v)}" for k, v in bufs.items()))


def packed(gen, B, N, Ds, Dt, tdtype):
    return rand(gen, (B * N, 3 * Ds), BF16, 0.5), rand(gen, (B * N, 3 * Dt), tdtype, 0.5)


for case, (B, N, Ds, Dt) in enumerate(REL_CASES):
    for tdtype in (BF16, F16):
        gen = torch.Generator().manual_seed(100 + case)
        s_buf, t_buf = packed(gen, B, N, Ds, Dt, tdtype)
        lse_t, lse_s, row_kl = zeros((3, B * N)), zeros((3, B * N)), zeros((3, B * N))
        S, loss3, d = zeros((3, B, 208, 224), BF16), zeros(3), zeros((B * N, 3 * Ds), BF16)
        up3 = torch.tensor([0.75, 1.25, -0.5], device=dev)
        tag = f"B{B}_N{N}_Ds{Ds}_Dt{Dt}_{'f16' if tdtype == F16 else 'bf16'}"
        ops.call("devit_relation_fused_fwd", ptr(s_buf), ptr(t_buf), B, N, Ds, Dt, 3 * Ds, 3 * Dt, 64, 64, int(tdtype == F16), ptr(lse_t), ptr(lse_s),
                 ptr(row_kl), ptr(S), ptr(loss3), stream_ptr())
        report("devit_relation_fused_fwd", tag, loss3=loss3, lse_t=lse_t, lse_s=lse_s, row_kl=row_kl, S=S)
        ops.call("devit_relation_fused_bwd", ptr(S), ptr(s_buf), ptr(up3), B, N, Ds, 3 * Ds, ptr(d), 3 * Ds, stream_ptr())
        report("devit_relation_fused_bwd", tag, d=d)

for case, (B, N, Ds, Dt) in enumerate(QKV_CASES):
    for tdtype in (BF16, F16):
        for layout in (0, 1):
            for cross in (0, 1):
                gen = torch.Generator().manual_seed(200 + case)
                s_buf, t_buf = packed(gen, B, N, Ds, Dt, tdtype)
                P = 9 if cross else 3
                terms, S, loss, d = zeros((P, B * N)), zeros((P, B, 208, 224), BF16), zeros(1), zeros((B * N, 3 * Ds), BF16)
                up = torch.tensor([1.5], device=dev)
                tag = f"B{B}_N{N}_Ds{Ds}_Dt{Dt}_{'f16' if tdtype == F16 else 'bf16'}_layout{layout}_cross{cross}"
                ops.call("devit_qkv_pair_fwd", ptr(s_buf), ptr(t_buf), B, N, Ds, Dt, 3 * Ds, 3 * Dt, 64, 64, int(tdtype == F16), cross, layout, 1,
                         ptr(terms), ptr(S), ptr(loss), stream_ptr())
                report("devit_qkv_pair_fwd", tag, loss=loss, terms=terms, S=S)
                ops.call("devit_qkv_pair_bwd", ptr(S), ptr(s_buf), ptr(up), B, N, Ds, 3 * Ds, 64, cross, layout, ptr(d), 3 * Ds, stream_ptr())
                report("devit_qkv_pair_bwd", tag, d=d)

for B, N in ((3, 198), (48, 198)):
    gen = torch.Generator().manual_seed(300 + B)
    g_t, g_s = rand(gen, (B, 256, 256), F32, 4.0), rand(gen, (B, 256, 256), F32, 4.0)
    lse_t, lse_s, row_kl, loss = zeros(B * N), zeros(B * N), zeros(B * N), zeros(1)
    ops.call("devit_relation_stats", ptr(g_t), ptr(g_s), B, N, 256, 64, 32, ptr(lse_t), ptr(lse_s), ptr(row_kl), ptr(loss), stream_ptr())
    report("devit_relation_stats", f"B{B}_N{N}", loss=loss, lse_t=lse_t, lse_s=lse_s, row_kl=row_kl)
    row_sq, loss = zeros(B * N), zeros(1)
    ops.call("devit_hid_stats", ptr(g_s), ptr(g_t), B, N, 256, 2, ptr(row_sq), ptr(loss), stream_ptr())
    report("devit_hid_stats", f"B{B}_N{N}", loss=loss, row_sq=row_sq)

for R, C in ((5, 7), (64, 198), (9000, 3)):
    gen = torch.Generator().manual_seed(400 + R)
    p, t = rand(gen, (R, C), F32, 3.0), rand(gen, (R, C), F32, 3.0)
    row_loss, loss = zeros(R), zeros(1)
    ops.call("devit_soft_ce_rows_fwd", ptr(p), ptr(t), R, C, ptr(row_loss), ptr(loss), stream_ptr())
    report("devit_soft_ce_rows_fwd", f"R{R}_C{C}", loss=loss, row_loss=row_loss)

txt = "\n".join(lines) + "\n"
sys.stdout.write(txt)
with open(sys.argv[1], "w") as f:
    f.write(txt)
