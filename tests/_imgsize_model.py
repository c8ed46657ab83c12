"""Size-general CPU restatement of the model's front for the image-size tests: oracle/devit_oracle.py hard-codes the 14 x 14 patch grid
of 224-pixel images in `state_keys`, `patch_embed` (and with it `embed_tokens`, `make_state`, `forward`, `distill_step`).  This module
restates exactly those for a square image of side S = 16 G and reuses the oracle's `block`, heads arithmetic and loss functions, which do
not depend on the token count.  Same expressions in the same order as the oracle's, and the same det_array names: at S = 224 the weights
and the forward are the oracle's bit for bit (tests/test_imgsize_host.py pins that, and pins S = 48 to a golden captured from the
reference's own VisionTransformer(img_size=48), tests/golden/make_golden_imgsize.py)."""
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle import devit_oracle as O
from oracle.detgen import det_array

SIZES = tuple(range(32, 225, 16))


def state_keys(geom, num_classes, S=224):
    """oracle.state_keys with pos_embed [1, (S/16)^2 + ntok, D]: same names, same order."""
    ntok = 2 if geom["distilled"] else 1
    T = (S // 16) ** 2
    return [(n, (1, T + ntok, sh[2]) if n == "pos_embed" else sh) for n, sh in O.state_keys(geom, num_classes)]


def make_state(geom, num_classes, tag, S=224):
    """oracle.make_state at image side S (the oracle's rule per name; at 224 the same arrays)."""
    st = OrderedDict()
    for name, shape in state_keys(geom, num_classes, S):
        full = f"{tag}/{name}"
        if name.endswith("norm1.weight") or name.endswith("norm2.weight") or name == "norm.weight":
            a = det_array(full, shape, std=0.05, mean=1.0)
        else:
            a = det_array(full, shape, std=0.02)
        st[name] = torch.from_numpy(a)
    return st


def patch_rows(img):
    """[B,3,S,S] -> [B, T, 768], k = c*256 + kh*16 + kw, t = py*G + px (what the im2row kernels produce)."""
    B, _, S, _ = img.shape
    G = S // 16
    return img.reshape(B, 3, G, 16, G, 16).permute(0, 2, 4, 1, 3, 5).reshape(B, G * G, 768)


def patch_embed(st, img):
    w = st["patch_embed.proj.weight"]
    return patch_rows(img) @ w.reshape(w.shape[0], 768).t() + st["patch_embed.proj.bias"]


def embed_tokens(st, img):
    x = patch_embed(st, img)
    B = x.shape[0]
    toks = [st["cls_token"].expand(B, -1, -1)]
    if "dist_token" in st:
        toks.append(st["dist_token"].expand(B, -1, -1))
    return torch.cat(toks + [x], dim=1) + st["pos_embed"]


def forward(st, geom, img, training=False, dp_scales=None):
    """oracle.forward behind the size-general embed_tokens."""
    H, depth = geom["num_heads"], geom["depth"]
    x = embed_tokens(st, img)
    enc, qkvs, atts = [x], [], []
    for i in range(depth):
        x, qkv, a = O.block(st, i, x, H, None if dp_scales is None else dp_scales[i], None, None)
        enc.append(x)
        qkvs.append(qkv)
        atts.append(a)
    D = x.shape[-1]
    x = F.layer_norm(x, (D,), st["norm.weight"], st["norm.bias"], O.LN_EPS)
    if geom["distilled"]:
        cls_t, dist_t = x[:, 0], x[:, 1]
        lo = F.linear(cls_t, st["head.weight"], st["head.bias"])
        lo_d = F.linear(dist_t, st["head_dist.weight"], st["head_dist.bias"])
        out = (lo, lo_d) if training else (lo + lo_d) / 2
        last = (cls_t, dist_t)
    else:
        last = x[:, 0]
        out = F.linear(last, st["head.weight"], st["head.bias"])
    return {"output": out, "qkv": qkvs, "attention": atts, "encoder": enc, "last_tokens": last}


def distill_step(st_s, geom_s, st_t, geom_t, img, soft_targets, gama=(0.2, 0.1, 0.3), kind="hard", alpha=0.5, tau=1.0, dp_scales=None):
    """oracle.distill_step on the size-general forward."""
    so = forward(st_s, geom_s, img, training=True, dp_scales=dp_scales)
    with torch.no_grad():
        to = forward(st_t, geom_t, img, training=False)
    cls_loss = O.distill_cls_loss(so["output"][0], so["output"][1], to["output"], soft_targets, kind, alpha, tau)
    ls, lt = geom_s["depth"], geom_t["depth"]
    s_qkv, t_qkv = so["qkv"][ls // 2 - 1], to["qkv"][lt // 2 - 1]
    q_loss, k_loss, v_loss = [O.feature_relation_loss(tv, sv) / ls for sv, tv in zip(s_qkv, t_qkv)]
    loss = cls_loss + gama[0] * q_loss + gama[1] * k_loss + gama[2] * v_loss
    return {"loss": loss, "cls_loss": cls_loss, "q_loss": q_loss, "k_loss": k_loss, "v_loss": v_loss, "student": so, "teacher": to}


def dp_scales_for(tag, B, depth=12, drop_path_rate=0.1):
    """Deterministic per-sample DropPath multipliers floor(keep + u) / keep for both branches of every block (block 0: keep 1)."""
    import numpy as np
    dpr = torch.linspace(0, drop_path_rate, depth).tolist()
    out = []
    for i in range(depth):
        keep = 1.0 - dpr[i]
        pair = []
        for j in range(2):
            u = torch.from_numpy(np.abs(det_array(f"{tag}/dp/{i}/{j}", (B,), std=1.0)) % 1.0).float()
            pair.append(torch.floor(keep + u) / keep)
        out.append(tuple(pair))
    return out


def pos_embed_input():
    """The deterministic [1, 198, 64] position table of the resize golden (2 token rows + a 14 x 14 grid)."""
    return torch.from_numpy(det_array("imgsize/posemb", (1, 198, 64), std=0.5))
