"""Float64 statement, elementwise error bounds, case list and seeded inputs of the token KL loss of the ensemble stage (csrc/losses.hip: kldiv_kernel,
devit_token_kldiv), in the conventions of tests/_tail_model.py: u = 2^-24 times the sum of the absolute values of the terms that enter an element
times the number of roundings on the longest path, counted from the kernel source; a correctly rounded operation costs 1, `expf` and `/` cost 2
(documented at <= 1 ulp = 2 u on this target: the HIP math API's accuracy table for expf, IEEE-compliant fp32 division being the default of the
compiler -- the same figures _tail_model.py uses for them).  Nothing is fitted to what the kernel delivers."""
import torch

from _tail_model import F32, F64, U, gen, randn

KLDIV_NS = (1, 5, 1024, 1025, 3073)
_DIVISOR = {5: 5, 1024: 4, 1025: 5, 3073: 7}          # 3073 = 7 * 439; 1 has no divisor but 1


def kldiv_cases():
    """(n, batch): batch 1 and, where n has one, a proper divisor of n"""
    return [(n, b) for n in KLDIV_NS for b in ((1, _DIVISOR[n]) if n in _DIVISOR else (1,))]


def kldiv_inputs(n, batch):
    """t uniform in [-4, 4] with a few elements at +-12 (final-norm tokens reach |t| of 10 and more); s = t + N(0, 1): terms of both signs"""
    g = gen("kldiv", n, batch)
    t = (torch.rand(n, generator=g, dtype=F32) * 8.0 - 4.0)
    if n >= 5:
        t[1], t[n // 2], t[n - 1] = 12.0, -12.0, 12.0
    s = t + randn(g, n)
    return dict(s=s, t=t, loss0=torch.tensor([-2.5], dtype=F32))


def kldiv_ref(s, t, batch, loss0=None):
    s, t = s.to(F64), t.to(F64)
    term = t.exp() * (t - s)
    return dict(loss=term.sum() / batch + (0.0 if loss0 is None else float(loss0)), ds=-t.exp() / batch), term


def kldiv_bounds(s, t, batch, loss0=None):
    """loss (+)= sum e^t (t - s) / batch, ds = -e^t / batch.
    loss: a term is t - s 1, expf 2, their product 1: 4 relative to |term|; then ceil(n / 1024) adds per thread, 6 shuffle adds, 16 waves in
          sequence, the division by batch 2, the accumulate 1 -- all on sum |term| / batch (+ |loss0|), NOT on |loss|: the terms cancel.
    ds:   expf 2, the division by batch 2 (the negation is exact): 4 u |ds|"""
    ref, term = kldiv_ref(s, t, batch, loss0)
    n = s.numel()
    l0 = 0.0 if loss0 is None else abs(float(loss0))
    cnt = 4 + (n + 1023) // 1024 + 6 + 16 + 2 + 1
    return ref, dict(loss=U * cnt * (term.abs().sum() / batch + l0), ds=4 * U * ref["ds"].abs())
