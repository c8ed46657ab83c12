"""CPU restatement of the DEKD step for a LIST of layer pairs (engine.distill_forward(relation_layers=...), --relation-layers): the q/k/v
relation losses of every selected student block against its teacher block, summed, where tests/_imgsize_model.distill_step (and the oracle)
take the middle pair alone.  No arithmetic of its own: the models are tests/_imgsize_model.forward, which returns every block's q/k/v and
encoder outputs, the losses oracle.devit_oracle.feature_relation_loss / distill_cls_loss.  With the middle pair the expressions are those of
_imgsize_model.distill_step in the same order, so its numbers come out bit for bit (tests/test_rellayers_host.py pins that)."""
import torch

import _imgsize_model as IM
from oracle import devit_oracle as O


def pairs_for(layers, ls, lt):
    """student blocks -> ((s, t), ...): teacher block t(s) = (s + 1) * (lt // ls) - 1, the last block of the s-th of ls equal groups"""
    assert lt % ls == 0
    return tuple((s, (s + 1) * (lt // ls) - 1) for s in sorted(set(layers)))


def layers_of(word, ls):
    return {"mid": [ls // 2 - 1], "last": [ls - 1], "all": list(range(ls))}[word] if isinstance(word, str) else list(word)


def distill_step(st_s, geom_s, st_t, geom_t, img, soft_targets, layers="mid", gama=(0.2, 0.1, 0.3), kind="hard", alpha=0.5, tau=1.0, dp_scales=None):
    """loss = cls + sum over the pairs of sum_j gama_j * feature_relation_loss_j(s, t) / ls.  q_loss / k_loss / v_loss: the sums over the pairs
    / ls; rel_layers: the unscaled per-pair losses [len(pairs), 3].  'student' / 'teacher': the forwards' dicts ('encoder'[i + 1] is block i's
    output: the list starts with the embedding)."""
    so = IM.forward(st_s, geom_s, img, training=True, dp_scales=dp_scales)
    with torch.no_grad():
        to = IM.forward(st_t, geom_t, img, training=False)
    cls_loss = O.distill_cls_loss(so["output"][0], so["output"][1], to["output"], soft_targets, kind, alpha, tau)
    ls, lt = geom_s["depth"], geom_t["depth"]
    pairs = pairs_for(layers_of(layers, ls), ls, lt)
    per = [[O.feature_relation_loss(tv, sv) for sv, tv in zip(so["qkv"][s], to["qkv"][t])] for s, t in pairs]
    q_loss, k_loss, v_loss = [sum(p[j] for p in per) / ls for j in range(3)]
    loss = cls_loss + gama[0] * q_loss + gama[1] * k_loss + gama[2] * v_loss
    return {"loss": loss, "cls_loss": cls_loss, "q_loss": q_loss, "k_loss": k_loss, "v_loss": v_loss, "pairs": pairs,
            "rel_layers": torch.stack([torch.stack([x.detach() for x in p]) for p in per]), "student": so, "teacher": to}
